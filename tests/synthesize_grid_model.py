"""float64 model of the grid synthesizer (k_synthesize_grid.hip behind ofdmrx_util_synthesize_grid), and the
tolerance the device is held to.

The definition.  Handle rate `rate`, interpolation D in {2, 4, .. 512}, Rw = D rate, M = 2 D slots k = -M/2 .. M/2 - 1 with their
centres at k rate / 2, K = 12 D, T = 24 D + 1.  The taps h are channelize_model.taps(D) - the bytes ofdmrx_util_channelize_grid_taps
writes: there is no new filter.  Row c = 0 .. C - 1:
    input   x_c[j], j = 0 .. n_in - 1, interleaved I/Q in S16 or F32, scaled as oracle_lib.pcm_to_cf scales it (fp32); zero outside
    slot    k_c, pairwise distinct
    start   start_c >= 0 in wideband samples, a multiple of D; sigma_c = start_c / D
    gain    G_c = D gain_c, formed in double, rounded once to fp32
and at absolute wideband index m
    w[m] = sum_c G_c exp(+2 pi i k_c m / M) sum_j h[m - start_c - j D] x_c[j]      over the j with 0 <= m - start_c - j D <= T - 1.
`direct` evaluates this as it stands in float64 (the exponent reduced mod M in integers).  It is section 4.15's output at the centres
k_c rate / 2 with inc = k_c 2^32 / M and no rounding of the increment.  `grid` evaluates the computed form in float64,
    X_j[k_c mod M] = (-1)^{k_c j} G_c x_c[j - sigma_c],   every other entry 0                  (j: absolute input time)
    V_j[r] = sum_k X_j[k] exp(+2 pi i k r / M),  r = 0 .. M - 1                               (numpy.fft.ifft times M)
    w[q D + b] = sum_{a = 0 .. 23, and a = 24 where b = 0} h[b + a D] V_{q - a}[b + (a mod 2) D],  0 <= b < D;  V_j = 0 for j < 0,
which test_synthesize_grid_model_cpu.py holds to `direct` and to synthesize_model.synthesize.  (With m = q D + b and j = q - a the
tap is h[b + a D]; k m / M = k j / 2 + k (b + a D) / M, the first term is the sign and (b + a D) mod M is b or b + D.)

The order the device keeps.  G_c x is one fp32 product per component, the sign is exact.  The transform is radix 2, decimation in
time: the points enter in bit-reversed order and the stage of half-length H = 1, 2 .. M / 2 makes (p, q) = (x[i] + w x[i + H], x[i] -
w x[i + H]), w = exp(+2 pi i j / (2 H)), j = i mod H, rounded once from double; an order fixed by M alone.  w[m] is one chain of fused
multiply-adds per component from +0, a ascending.  Every output passes through v + 0.f: a zero is always +0.  F32 output: (re, im)
of w[m]; S16 output: quantise() of it.

The tolerance, per component of an output, derived here from the arithmetic and from nothing the device gives.  With u = 2^-24
(half an ulp, relative) and
    S[m] = sum_c |G_c| sum_j |h[m - start_c - j D]| (|re| + |im|)(x_c[j]):        tol[m] = 2^-24 (A + B log2 M) S[m],  A = 28, B = 6.
  * a component of V_j[r] is at most N_j = sum_c |G_c| (|re| + |im|)(x_c[j - sigma_c]) in modulus, whatever r, and S[q D + b] =
    sum_a |h[b + a D]| N_{q - a}: S bounds every partial sum of an output's chain;
  * the output's chain is at most 25 fused multiply-adds per component, each rounding once by at most u times the partial sum: 25 u S;
  * the product G_c x rounds once per component (1 u |G_c x|); it passes the transform with factors of modulus 1, where a component
    of it can grow by sqrt 2 once (l2 against l1), and the filter with |h|: 1.42 u S.  The input's conversion is part of the
    definition (the model starts from the fp32 values); the rule keeps 1 u S for it all the same.  25 + 1.42 + 1 <= A = 28;
  * the transform: per component and stage the product w x rounds its two partial products (weighted by |Re w| + |Im w| <= sqrt 2:
    1.42 u) and their fused sum (1 u), the root's components are each within u / 2 of the truth (u / 2 of (|re| + |im|)), and the
    addition or subtraction rounds once (1 u): at most 4 u of the magnitude that passes the stage, which over all the paths to one
    point is at most N_j; later stages pass an error on with factors of modulus 1, a component growing by sqrt 2 at most once:
    4 sqrt 2 = 5.7 <= B = 6 per stage, and through the filter's |h|: 6 log2 M u S.  This is section 4.19's count; decimation in
    time multiplies before it adds where decimation in frequency adds before it multiplies, with the same roundings per stage.
The rule is homogeneous in x: for F32 input nothing is added.  Where no row reaches m, S[m] = 0: the tolerance is 0 and the output
must be +0 exactly.  An fp32 numpy evaluation in the documented order (grid_fp32 below; products and sums rounded separately, which
is pessimistic) stays under a quarter of the rule at every D (test_synthesize_grid_model_cpu.py prints the figures)."""
import numpy as np

import channelize_grid_model as G
import channelize_model as CM
import synthesize_model as SM

ALL_D = G.ALL_D
A_TOL, B_TOL = 28.0, 6.0

to_cf, gain32, quantise, worst, random_x, support, n_outputs = SM.to_cf, SM.gain32, SM.quantise, SM.worst, SM.random_x, SM.support, SM.n_outputs
taps, all_slots, centres, roots32 = G.taps, G.all_slots, G.centres, G.roots32


def tile(D):
    """input times per workgroup of the transform kernel (the tests put rows at its edges)"""
    return max(4096 // (2 * D), 8)


def filter_tile(D):
    """outputs per workgroup of the filter kernel: 8 output times per work item, 256 / D groups of D work items (one group from D = 256
    on), counted from out_first rounded down to a multiple of D (the tests put windows at its edges)"""
    return 8 * max(256, D)


def _check(x, D, slots, starts, gains, out_first, n_out):
    if D not in ALL_D:
        raise ValueError("interp must be a power of two 2 .. 512")
    if x.ndim != 3 or x.shape[2] != 2 or x.shape[0] < 1 or x.shape[1] < 1 or x.dtype not in (np.dtype(np.int16), np.dtype(np.float32)):
        raise ValueError("input must be [C, n_in, 2] of int16 or float32")
    if not (len(slots) == len(starts) == len(gains) == x.shape[0]) or x.shape[0] > 2 * D:
        raise ValueError("one slot, start and gain per row, at most M rows")
    if len(set(slots)) != len(slots) or not all(-D <= k < D for k in slots):
        raise ValueError("the slots are pairwise distinct and lie in -M/2 .. M/2 - 1")
    if not all(0 <= s <= 1 << 50 and s % D == 0 for s in starts) or not 0 <= int(out_first) <= 1 << 50:
        raise ValueError("a start or out_first is negative or above 2^50, or D does not divide a start")
    if not all(np.isfinite(np.float32(g)) and np.isfinite(gain32(D, g)) for g in gains):
        raise ValueError("a gain is not finite")
    if n_out is not None and n_out < 1:
        raise ValueError("n_out must be positive")


def _args(x, D, slots, starts, gains, out_first, n_out):
    x = np.ascontiguousarray(x)
    slots = [int(k) for k in (all_slots(D) if slots is None else np.atleast_1d(slots))]
    starts = [int(s) for s in np.atleast_1d(starts)]
    gains = [float(g) for g in np.atleast_1d(np.asarray(gains, np.float64))]
    _check(x, D, slots, starts, gains, out_first, n_out)
    if n_out is None:
        n_out = n_outputs(starts, x.shape[1], D) - out_first
    return x, slots, starts, gains, int(n_out)


def _times(q, na):
    """the input times the output times q meet: j0 .. j1"""
    return int(q.min()) - na, int(q.max())


def bound(x, D, slots, starts, gains, out_first=0, n_out=None):
    """-> tol [n_out]: the rule of the header, S[q D + b] = sum_a |h[b + a D]| N_{q - a}"""
    x, slots, starts, gains, n_out = _args(x, D, slots, starts, gains, out_first, n_out)
    h = np.abs(taps(D).astype(np.float64))
    n_in = x.shape[1]
    m = np.arange(n_out, dtype=np.int64) + out_first
    q, b = m // D, m % D
    j0, j1 = _times(q, 24)
    j = np.arange(j0, j1 + 1, dtype=np.int64)
    N = np.zeros(len(j), np.float64)
    for c in range(x.shape[0]):
        xc = to_cf(x[c])
        i = j - starts[c] // D
        ok = (i >= 0) & (i < n_in)
        N += np.where(ok, abs(float(gain32(D, gains[c]))) * (np.abs(xc.real) + np.abs(xc.imag))[np.clip(i, 0, n_in - 1)], 0.0)
    S = np.zeros(n_out, np.float64)
    for a in range(25):
        t = b + a * D
        S += np.where(t <= 24 * D, h[np.minimum(t, 24 * D)] * N[q - a - j0], 0.0)
    return 2.0 ** -24 * (A_TOL + B_TOL * np.log2(2 * D)) * S


def direct(x, D, slots, starts, gains, outputs):
    """the definition as it stands at the absolute wideband indices `outputs` -> [len(outputs)] complex128: for every row the j with
    0 <= m - start_c - j D <= T - 1 (written j = floor((m - start_c) / D) - a, a = 0 .. 24), the phase k_c m reduced mod M in integers"""
    x, slots, starts, gains, _ = _args(x, D, slots, starts, gains, 0, None)
    h = taps(D).astype(np.float64)
    T, M, n_in = len(h), 2 * D, x.shape[1]
    m = np.asarray(outputs, np.int64)
    xc = np.stack([to_cf(x[c]) for c in range(x.shape[0])])          # [C, n_in]
    r = m[None, :] - np.asarray(starts, np.int64)[:, None]            # [C, n]
    u = np.zeros(r.shape, np.complex128)
    rows = np.arange(x.shape[0])[:, None]
    for a in range(25):
        jj = r // D - a
        t = r - jj * D
        ok = (t >= 0) & (t <= T - 1) & (jj >= 0) & (jj < n_in)
        u += np.where(ok, h[np.clip(t, 0, T - 1)] * xc[rows, np.clip(jj, 0, n_in - 1)], 0.0)
    ph = (np.asarray(slots, np.int64)[:, None] * (m % M)[None, :]) % M   # integers: exact
    G = np.array([float(gain32(D, g)) for g in gains])
    return (G[:, None] * np.exp(2j * np.pi * ph.astype(np.float64) / M) * u).sum(axis=0)


VARIANTS = ("transform sign", "no (-1)^(k j)", "slot k + 1", "V rows exchanged", "gain without D", "start off by D", "output at m + 1",
            "re / im swapped", "M = D", "scaled by 1 / M", "K = 8 D")


def grid(x, D, slots, starts, gains, out_first=0, n_out=None, variant=None):
    """x: [C, n_in, 2] int16 or float32 -> (v [n_out] complex128, tol [n_out]): the computed form through numpy.fft.  slots None: all,
    ascending; variant: one of VARIANTS, a deliberately wrong model (its tol is the definition's)"""
    x, slots, starts, gains, n_out = _args(x, D, slots, starts, gains, out_first, n_out)
    tol = bound(x, D, slots, starts, gains, out_first, n_out)
    Cn, n_in = x.shape[0], x.shape[1]
    h = (CM.taps64(D, K_per_D=8) if variant == "K = 8 D" else CM.taps64(D)).astype(np.float32).astype(np.float64)
    na = (len(h) - 1) // D                                          # 24: the last tap index is na D
    M = D if variant == "M = D" else 2 * D
    shift = 1 if variant == "output at m + 1" else 0
    m = np.arange(n_out, dtype=np.int64) + out_first - shift
    q, b = m // D, m % D
    j0 = int(q.min()) - na                                          # the input times the window meets: j0 .. j1
    j1 = int(q.max())
    j = np.arange(j0, j1 + 1, dtype=np.int64)
    X = np.zeros((len(j), M), np.complex128)
    for c in range(Cn):
        xc = to_cf(x[c])
        if variant == "re / im swapped":
            xc = xc.imag + 1j * xc.real
        Gc = float(np.float32(gains[c])) if variant == "gain without D" else float(gain32(D, gains[c]))
        sg = starts[c] // D + (1 if variant == "start off by D" else 0)
        k = slots[c] + (1 if variant == "slot k + 1" else 0)
        i = j - sg
        ok = (i >= 0) & (i < n_in)
        val = np.where(ok, Gc * xc[np.clip(i, 0, n_in - 1)], 0.0)
        if variant != "no (-1)^(k j)":
            val = np.where((k * j) % 2 == 1, -val, val)
        X[:, k % M] += val
    V = np.fft.fft(X, axis=1) if variant == "transform sign" else np.fft.ifft(X, axis=1) * M
    if variant == "scaled by 1 / M":
        V = V / M
    v = np.zeros(n_out, np.complex128)
    for a in range(na + 1):
        t = b + a * D
        ok = (t <= len(h) - 1) & (q - a >= 0)
        odd = (a + 1) % 2 if variant == "V rows exchanged" else a % 2
        r = (b + odd * D) % M
        v += np.where(ok, h[np.minimum(t, len(h) - 1)] * V[np.clip(q - a - j0, 0, len(j) - 1), r], 0.0)
    return v, tol


def grid_fp32(x, D, slots, starts, gains, out_first=0, n_out=None):
    """an fp32 numpy evaluation of the computed form in the documented order: G x one fp32 product, the radix-2 decimation-in-time
    transform in complex64 with roots rounded once, the output's chain with a ascending (products and sums rounded separately, no
    fused multiply-add) -> [n_out] complex64"""
    f32 = np.float32
    x, slots, starts, gains, n_out = _args(x, D, slots, starts, gains, out_first, n_out)
    Cn, n_in = x.shape[0], x.shape[1]
    h = taps(D)
    M = 2 * D
    m = np.arange(n_out, dtype=np.int64) + out_first
    q, b = m // D, m % D
    j0, j1 = int(q.min()) - 24, int(q.max())
    j = np.arange(j0, j1 + 1, dtype=np.int64)
    bits = M.bit_length() - 1
    rev = np.array([int(format(i, "0%db" % bits)[::-1], 2) for i in range(M)])
    z = np.zeros((len(j), M), np.complex64)
    for c in range(Cn):
        xc = SM.O.pcm_to_cf(x[c]).astype(f32)
        g = gain32(D, gains[c])
        i = j - starts[c] // D
        ok = (i >= 0) & (i < n_in)
        ii = np.clip(i, 0, n_in - 1)
        re, im = np.where(ok, g * xc[ii, 0], f32(0)), np.where(ok, g * xc[ii, 1], f32(0))
        sign = np.where((slots[c] * j) % 2 == 1, f32(-1), f32(1))
        z[:, rev[slots[c] % M]] = (sign * re + 1j * (sign * im)).astype(np.complex64)
    w = roots32(M)
    H = 1
    while H <= M // 2:                                              # in place: blocks of 2 H, bit-reversed order in, natural out
        zz = z.reshape(len(j), M // (2 * H), 2, H)
        t = (zz[:, :, 1] * w[::M // (2 * H)][None, None, :]).astype(np.complex64)
        z = np.stack([(zz[:, :, 0] + t).astype(np.complex64), (zz[:, :, 0] - t).astype(np.complex64)], axis=2).reshape(len(j), M)
        H *= 2
    vr, vi = z.real.astype(f32), z.imag.astype(f32)
    wr, wi = np.zeros(n_out, f32), np.zeros(n_out, f32)
    for a in range(25):
        t = b + a * D
        ok = (t <= 24 * D) & (q - a >= 0)
        hk = h[np.minimum(t, 24 * D)]
        row, col = np.clip(q - a - j0, 0, len(j) - 1), b + (a % 2) * D
        wr = np.where(ok, wr + hk * vr[row, col], wr)
        wi = np.where(ok, wi + hk * vi[row, col], wi)
    return wr + 1j * wi
