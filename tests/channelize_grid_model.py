"""float64 model of the grid front end (k_channelize_grid.hip behind ofdmrx_util_channelize_grid), and the
tolerance the device is held to.

The definition.  Handle rate `rate`, decimation D in {2, 4, .. 512}, Rw = D rate, M = 2 D slots k = -M/2 .. M/2 - 1 with their centres
at k rate / 2, K = 12 D, T = 24 D + 1 = 12 M + 1.  The taps h are channelize_model.taps(D): section 4.14's formula in double,
normalised to sum 1, rounded once to fp32.  Input scaled as oracle_lib.pcm_to_cf scales it (fp32).
    y_k[n] = sum_{t = 0 .. T - 1} h[t] x[n D - t] exp(-2 pi i k (n D - t) / M),    x zero at negative indices.
W samples give ceil(W / D) outputs.  `direct` evaluates this sum as it stands in float64 (the exponent reduced mod M in integers).
`grid` evaluates the polyphase form in float64 - u_n[r] = sum_a h[r + M a] x[n D - r - M a], y_k[n] = (-1)^{k n} sum_r u_n[r]
exp(+2 pi i k r / M) through numpy.fft - which test_channelize_grid_model_cpu.py holds to `direct` and, at the slot centres, to
channelize_model.channelize.

The tolerance, per component of an output, derived here from the arithmetic the kernel performs and from nothing the device gives:
    tol = 2^-24 (A + B log2 M) S,    S = sum_t |h[t]| (|re| + |im|)(x[n D - t]),    A = 16, B = 6.
With u = 2^-24 (half an ulp, relative):
  * the input's conversion (S16 / U8: one division rounded to fp32) is part of the definition - the model starts from the fp32
    values - so it adds nothing; the rule keeps 1 u S for it all the same;
  * a branch sum u_n[r] is a chain of at most 13 fused multiply-adds per component: each rounds once, by at most u times the partial
    sum, which is at most sum_a |h[r + M a]| |x[..]|.  Over all r the chains' bounds add up to 13 u S (each component of x against
    its own share of S);
  * the sign (-1)^{k n} is exact.  A = 13 + 1 = 14 <= 16;
  * the transform is log2 M radix-2 stages (decimation in frequency): p = a + b, q = (a - b) w, w = exp(+2 pi i j / M) rounded once
    from double.  Per component and stage: the addition or subtraction rounds once (1 u); the root's components are each within u / 2
    of the truth (|w| <= 1), which moves a component of the product by at most u / 2 (|re| + |im|)(a - b); the product's two partial
    products round once each, weighted by |Re w| + |Im w| <= sqrt 2 (1.42 u), and their sum - one fused multiply-add - once more (1 u):
    at most 4 u of the magnitude that passes the stage.  What passes a stage is bounded, over all the paths that reach one output,
    by sum_r (|re| + |im|)(u_n[r]) <= S (both components of a complex value feed both components of the next, whence the l1 norm),
    and the later stages pass an earlier error on with factors of modulus 1, a component of it growing by at most sqrt 2 once (l2
    against l1).  4 sqrt 2 = 5.7 <= B = 6 per stage.
For F32 input nothing is added: the bound is homogeneous in x.  An fp32 numpy evaluation of the same arithmetic (grid_fp32 below)
stays under 0.05 of the rule on full-scale random int16 at every D (test_channelize_grid_model_cpu.py prints the figures)."""
import numpy as np

import channelize_model as CM

ALL_D = (2, 4, 8, 16, 32, 64, 128, 256, 512)
A_TOL, B_TOL = 16.0, 6.0

to_cf, worst, random_pcm, n_outputs = CM.to_cf, CM.worst, CM.random_pcm, CM.n_outputs


def taps64(D, **kw):
    return CM.taps64(D, **kw)


def taps(D):
    return taps64(D).astype(np.float32)


def all_slots(D):
    return np.arange(-D, D, dtype=np.int64)


def centres(D, rate=8000, slots=None):
    k = all_slots(D) if slots is None else np.asarray(slots, np.int64)
    return k.astype(np.float64) * (rate / 2.0)


def _windows(a, first, D, n_out, T, out_first):
    """-> [n_out, T]: column t of row j is a[n D - t], n = out_first + j (zero outside the positions first .. first + len(a) - 1)"""
    w, _ = CM._windows(a, first, D, n_out, T, out_first)
    return w[:, ::-1]


def bound(pcm, D, out_first=0, n_out=None, in_first=0):
    """-> tol [n_out]: the rule of the header, the same for every slot"""
    x = to_cf(pcm)
    if n_out is None:
        n_out = n_outputs(in_first + len(x), D) - out_first
    h = taps(D).astype(np.float64)
    S = _windows(np.abs(x.real) + np.abs(x.imag), in_first, D, n_out, len(h), out_first) @ np.abs(h)
    return 2.0 ** -24 * (A_TOL + B_TOL * np.log2(2 * D)) * S


def direct(pcm, D, slots, outputs, in_first=0):
    """the definition as it stands, for the outputs n in `outputs` -> [len(slots), len(outputs)] complex128"""
    x = to_cf(pcm)
    h = taps(D).astype(np.float64)
    T, M = len(h), 2 * D
    out = np.zeros((len(slots), len(outputs)), np.complex128)
    t = np.arange(T, dtype=np.int64)
    for j, n in enumerate(outputs):
        m = int(n) * D - t                                          # absolute positions
        ok = (m >= in_first) & (m < in_first + len(x))
        xs = np.where(ok, x[np.clip(m - in_first, 0, len(x) - 1)], 0.0)
        for i, k in enumerate(slots):
            ph = (int(k) * m) % M                                   # integers: exact
            out[i, j] = np.sum(h * xs * np.exp(-2j * np.pi * ph.astype(np.float64) / M))
    return out


VARIANTS = ("transform sign", "no (-1)^(k n)", "slot k + 1", "branch M - r", "output at n D + 1", "M = D", "scaled by 1 / M",
            "taps sum to D", "K = 8 D", "re / im swapped", "centre tap")


def grid(pcm, D, slots=None, out_first=0, n_out=None, in_first=0, variant=None):
    """-> (v [n_slots, n_out] complex128, tol [n_slots, n_out]).  pcm: the wideband positions in_first ..; slots None: all, ascending;
    variant: one of VARIANTS, a deliberately wrong model"""
    x = to_cf(pcm)
    if n_out is None:
        n_out = n_outputs(in_first + len(x), D) - out_first
    k = all_slots(D) if slots is None else np.asarray(slots, np.int64)
    kw = {}
    if variant == "taps sum to D":
        kw["total"] = float(D)
    if variant == "K = 8 D":
        kw["K_per_D"] = 8
    h = taps64(D, **kw).astype(np.float32).astype(np.float64)
    T = len(h)
    if variant == "centre tap":
        h[T // 2] *= 1.0 + 2.0 ** -10
    if variant == "re / im swapped":
        x = x.imag + 1j * x.real
    shift = 1 if variant == "output at n D + 1" else 0
    M = D if variant == "M = D" else 2 * D
    g = _windows(x, in_first - shift, D, n_out, T, out_first) * h   # [n_out, T]: h[t] x[n D - t]
    na = -(-T // M)
    u = np.zeros((n_out, na * M), np.complex128)
    u[:, :T] = g
    u = u.reshape(n_out, na, M).sum(axis=1)                         # the branch sums, a ascending
    if variant == "branch M - r":
        u = u[:, (-np.arange(M)) % M]
    Y = np.fft.fft(u, axis=1) if variant == "transform sign" else np.fft.ifft(u, axis=1) * M
    if variant == "scaled by 1 / M":
        Y = Y / M
    kk = k + 1 if variant == "slot k + 1" else k
    n = np.arange(n_out, dtype=np.int64) + out_first
    v = Y[:, kk % M].T                                              # [n_slots, n_out]
    if variant != "no (-1)^(k n)":
        # exp(-2 pi i k n D / M): at M = 2 D the sign (-1)^{k n}
        ph = (kk[:, None] * ((n * D) % M)[None, :]) % M
        v = v * np.where(2 * ph == M, -1.0, 1.0) if M == 2 * D else v * np.exp(-2j * np.pi * ph / M)
    tol = np.broadcast_to(bound(pcm, D, out_first, n_out, in_first), v.shape).copy()
    return v, tol


def rows(pcm, D, slots):
    """the model's rows over a whole long capture from position 0 -> float32 [n_slots, ceil(W / D), 2]: the same sum in float64,
    arranged per slot as a mix-down by the exact phase (k m mod M) and D branch convolutions (tap p + D j against sample n D - p -
    D j); test_channelize_grid_model_cpu.py holds it to `grid`"""
    x = to_cf(pcm)
    h = taps(D).astype(np.float64)
    M, W = 2 * D, len(x)
    n_out = n_outputs(W, D)
    m = np.arange(W, dtype=np.int64)
    out = np.zeros((len(slots), n_out, 2), np.float32)
    for i, k in enumerate(slots):
        xm = np.zeros(n_out * D, np.complex128)                     # positions 0 .. n_out D - 1 (zeros past the capture)
        xm[:W] = x * np.exp(-2j * np.pi * ((int(k) * m) % M).astype(np.float64) / M)
        y = np.zeros(n_out, np.complex128)
        for p in range(D):
            hp = h[p::D]
            # branch p: the samples n D - p, n = 0 ..  (p = 0: position n D; else position (n - 1) D + (D - p), zero at n = 0)
            xp = xm[0::D] if p == 0 else np.concatenate([[0.0], xm[D - p::D][:n_out - 1]])
            y += np.convolve(xp, hp)[:n_out]
        out[i, :, 0], out[i, :, 1] = y.real, y.imag
    return out


def roots32(M):
    j = np.arange(M // 2, dtype=np.float64)
    return (np.cos(2 * np.pi * j / M).astype(np.float32) + 1j * np.sin(2 * np.pi * j / M).astype(np.float32)).astype(np.complex64)


def grid_fp32(pcm, D, slots=None):
    """an fp32 numpy evaluation of the computed form from position 0: the branch chains with a ascending (products and sums rounded
    separately), a radix-2 decimation-in-frequency transform in complex64 with roots rounded once -> [n_slots, ceil(W / D)] complex64"""
    f32 = np.float32
    xc = CM.O.pcm_to_cf(np.ascontiguousarray(pcm))
    h = taps(D)
    T, M = len(h), 2 * D
    n_out = n_outputs(len(xc), D)
    k = all_slots(D) if slots is None else np.asarray(slots, np.int64)
    wr = _windows(xc[:, 0].astype(f32), 0, D, n_out, T, 0)
    wi = _windows(xc[:, 1].astype(f32), 0, D, n_out, T, 0)
    re, im = np.zeros((n_out, M), f32), np.zeros((n_out, M), f32)
    for a in range(12):
        re = re + h[a * M:(a + 1) * M] * wr[:, a * M:(a + 1) * M]
        im = im + h[a * M:(a + 1) * M] * wi[:, a * M:(a + 1) * M]
    re[:, 0] = re[:, 0] + h[12 * M] * wr[:, 12 * M]
    im[:, 0] = im[:, 0] + h[12 * M] * wi[:, 12 * M]
    z = (re + 1j * im).astype(np.complex64)
    w = roots32(M)
    H = M // 2
    while H >= 1:                                                   # in place: blocks of 2 H, natural order in, bit-reversed out
        zz = z.reshape(n_out, M // (2 * H), 2, H)
        p = (zz[:, :, 0] + zz[:, :, 1]).astype(np.complex64)
        q = ((zz[:, :, 0] - zz[:, :, 1]).astype(np.complex64) * w[::M // (2 * H)][None, None, :]).astype(np.complex64)
        z = np.stack([p, q], axis=2).reshape(n_out, M)
        H //= 2
    bits = M.bit_length() - 1
    rev = np.array([int(format(i, "0%db" % bits)[::-1], 2) for i in range(M)])
    n = np.arange(n_out, dtype=np.int64)
    out = z[:, rev[k % M]].T
    return np.where(((k[:, None] & 1) & (n[None, :] & 1)) == 1, -out, out).astype(np.complex64)
