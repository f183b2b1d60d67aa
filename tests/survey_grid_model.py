"""float64 model of the grid survey (k_survey_grid.hip behind ofdmrx_util_survey_grid), the tolerance the
device is held to, and a float64 restatement of the slot finder (ofdmrx_util_find_slots).

The definition.  Symbols are section 4.19's (channelize_grid_model.py): handle rate `rate`, D in {2, 4, .. 512}, M = 2 D slots
k = -M/2 .. M/2 - 1 at k rate / 2, T = 24 D + 1 taps h (channelize_model.taps(D): no new filter), y_k[n] the grid front end's output
at ABSOLUTE output time n with x zero at negative positions.  S = times_per_row is a multiple of 8 in 8 .. 65536.  Row r >= 0:
    P[r][k + M/2] = (1 / S) sum_{n = r S .. r S + S - 1} |y_k[n]|^2
in ascending slot order, with no further normalisation: white noise of power sigma^2 per complex sample reads sigma^2 sum h^2.  Row r
needs the wideband positions max(0, (r S - 24) D) .. ((r + 1) S - 1) D (`span`).  `power` evaluates this in float64 from the
polyphase form (the branch sums gathered by absolute position, numpy's inverse transform); the sign (-1)^{k n} of section 4.19 has
modulus 1 and is not applied - which also means that a kernel that forgot it could not be told from a correct one by any power, so
"no (-1)^(k n)" is NOT among the wrong variants below.  test_survey_grid_model_cpu.py holds `power` to channelize_grid_model.grid
and .rows.

The tolerance, per output, derived from the arithmetic the kernels perform and from nothing the device gives.  With u = 2^-24 and
e_n = sqrt 2 x (section 4.19's per-component bound at time n: channelize_grid_model.bound, the same for every slot) - the most the
computed y_k[n] is off in modulus:
    tol[r][k] = (1 / S) sum_n (2 |y_k[n]| e_n + e_n^2)  +  (8 + S / 8 + 4) u (P[r][k] + that)
  * | |y + d|^2 - |y|^2 | <= 2 |y| |d| + |d|^2 with |d| <= e_n: the first term, averaged like P;
  * the second term bounds the roundings of the sum itself, relative to the largest value it can reach (P plus the first term, all
    addends being non-negative): |y|^2 = fma(im, im, re re) rounds twice (2 u), the chain over the 8 times of a group adds at most 7
    more (together <= 8 u + the next item), the chain over a row's S / 8 groups at most S / 8, and the product with fp32(1 / S) - a
    rounded constant and one rounding - 2; 4 covers those and the second-order terms.
For F32 input nothing is added: the rule is homogeneous of degree 2 in x.  `power_fp32` evaluates the documented order in fp32 numpy
(on channelize_grid_model.grid_fp32's outputs); test_survey_grid_model_cpu.py prints how far it stays under the rule."""
import numpy as np

import channelize_grid_model as G
import channelize_model as CM

U = 2.0 ** -24
GROUP = 8
to_cf, random_pcm = CM.to_cf, CM.random_pcm

VARIANTS = ("natural slot order", "slot k + 1", "mirrored slot -k", "row starts at r S + 1", "1 / S missing", "|y| for |y|^2", "re only",
            "taps sum to D", "K = 8 D", "output at n D + 1", "U8 without its offset")


def span(D, S, row_first, n_rows):
    """-> (first position, count) the rows row_first .. row_first + n_rows - 1 need"""
    first = max(0, (row_first * S - 24) * D)
    return first, ((row_first + n_rows) * S - 1) * D - first + 1


def _gather(a, h, in_first, D, n0, n, shift=0):
    """sum_a h[r + M a] a[n D + shift - r - M a] -> [n, M] (a holds the positions in_first .. in_first + len(a) - 1, zero elsewhere)"""
    M, T = 2 * D, len(h)
    nn = (np.arange(n, dtype=np.int64) + n0)[:, None] * D + shift
    r = np.arange(M, dtype=np.int64)[None, :]
    u = np.zeros((n, M), a.dtype)
    for j in range(-(-T // M)):
        t = r + M * j
        ok_t = t < T
        idx = nn - t - in_first
        ok = ok_t & (idx >= 0) & (idx < len(a))
        u += np.where(ok_t, h[np.minimum(t, T - 1)], 0.0) * np.where(ok, a[np.clip(idx, 0, len(a) - 1)], 0.0)
    return u


def outputs(pcm, D, n0, n, in_first=0, variant=None):
    """-> (|.| of which is |y_k[n]|: complex128 [n, M], ascending slot order, the sign (-1)^{k n} left out;  e [n]: sqrt 2 x 4.19's
    per-component bound) for the absolute output times n0 .. n0 + n - 1"""
    if variant == "U8 without its offset":
        assert pcm.dtype == np.uint8
        f = (pcm.astype(np.float32) / np.float32(127)).astype(np.float64)
        x = f[:, 0] + 1j * f[:, 1]
    else:
        x = to_cf(pcm)
    kw = {}
    if variant == "taps sum to D":
        kw["total"] = float(D)
    if variant == "K = 8 D":
        kw["K_per_D"] = 8
    h = CM.taps64(D, **kw).astype(np.float32).astype(np.float64)
    M = 2 * D
    u = _gather(x, h, in_first, D, n0, n, shift=1 if variant == "output at n D + 1" else 0)
    Y = np.fft.ifft(u, axis=1) * M                                   # column k mod M
    k = G.all_slots(D)
    if variant == "natural slot order":
        k = np.arange(M)
    if variant == "slot k + 1":
        k = k + 1
    if variant == "mirrored slot -k":
        k = -k
    S1 = _gather(np.abs(x.real) + np.abs(x.imag), np.abs(G.taps(D).astype(np.float64)), in_first, D, n0, n)[:, :].sum(axis=1)
    e = np.sqrt(2.0) * U * (G.A_TOL + G.B_TOL * np.log2(M)) * S1
    return Y[:, k % M], e


def power(pcm, D, S, row_first=0, n_rows=1, in_first=0, variant=None):
    """-> (P [n_rows, M] float64, tol [n_rows, M]).  pcm: the wideband positions in_first ..; variant: one of VARIANTS, a deliberately
    wrong model.  Works row by row, so a long capture costs S x M values at a time"""
    assert S % GROUP == 0 and 8 <= S <= 65536
    M = 2 * D
    P, tol = np.zeros((n_rows, M)), np.zeros((n_rows, M))
    for j in range(n_rows):
        n0 = (row_first + j) * S + (1 if variant == "row starts at r S + 1" else 0)
        y, e = outputs(pcm, D, n0, S, in_first, variant)
        a = np.abs(y)
        if variant == "|y| for |y|^2":
            p = a.mean(axis=0)
        elif variant == "re only":
            p = (y.real ** 2).mean(axis=0)
        elif variant == "1 / S missing":
            p = (a ** 2).sum(axis=0)
        else:
            p = (a ** 2).mean(axis=0)
        first = (2.0 * a * e[:, None] + (e ** 2)[:, None]).mean(axis=0)
        P[j] = p
        tol[j] = first + (8 + S / 8 + 4) * U * (p + first)
    return P, tol


def worst(got, P, tol):
    """largest |got - P| / tol"""
    d = np.abs(np.asarray(got, np.float64) - P)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, d / np.where(tol > 0, tol, 1.0), np.where(d > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def power_fp32(pcm, D, S, n_rows):
    """the documented order in fp32 numpy, rows 0 .. n_rows - 1 of a capture from position 0: |y|^2 = fma(im, im, re re) (the product
    rounded, the fused step formed in double and rounded once), one chain over the 8 times of a group, one over the row's groups,
    one product with fp32(1 / S) -> float32 [n_rows, M]"""
    f32 = np.float32
    y = G.grid_fp32(pcm, D)[:, :n_rows * S]                          # [M, times], ascending slots
    assert y.shape[1] == n_rows * S
    re, im = y.real.astype(f32), y.imag.astype(f32)
    rr = (re * re).astype(f32)
    p = (im.astype(np.float64) * im.astype(np.float64) + rr.astype(np.float64)).astype(f32)
    p = p.reshape(2 * D, n_rows, S // GROUP, GROUP)
    g = np.zeros(p.shape[:3], f32)
    for t in range(GROUP):
        g = (g + p[..., t]).astype(f32)
    s = np.zeros(p.shape[:2], f32)
    for j in range(S // GROUP):
        s = (s + g[..., j]).astype(f32)
    return (s * f32(1.0 / S)).astype(f32).T


def tone_pcm(W, D, slot, dtype=np.int16, seed=1, amp=0.4, first=0):
    """full scale in sum: 0.6 x uniform random input plus a tone of amplitude amp on the centre of `slot` (k / M cycles per sample,
    its phase counted from absolute position 0)"""
    rng = np.random.default_rng(seed)
    M = 2 * D
    m = np.arange(W, dtype=np.int64) + first
    ph = 2.0 * np.pi * ((slot * m) % M).astype(np.float64) / M
    x = 0.6 * rng.uniform(-1.0, 1.0, size=(W, 2)) + amp * np.stack([np.cos(ph), np.sin(ph)], axis=1)
    if np.dtype(dtype) == np.int16:
        return np.rint(x * 32767.0).astype(np.int16)
    if np.dtype(dtype) == np.uint8:
        return np.clip(np.rint(x * 127.0 + 128.0), 1, 255).astype(np.uint8)
    return x.astype(np.float32)


def noise_reading(D, sigma2=1.0):
    """what white noise of power sigma2 per complex sample reads in every slot: sigma2 sum h^2"""
    return sigma2 * float((G.taps(D).astype(np.float64) ** 2).sum())


def find_slots(row, D, rate, thr_db=6.0, sep_db=8.0, abs_floor=0.0):
    """ofdmrx_util_find_slots restated in float64 -> ([(slot, centre_hz, power, level_db)], floor)"""
    p = np.asarray(row, np.float32).astype(np.float64)
    M = 2 * D
    assert p.shape == (M,)
    if abs_floor > 0:
        floor = float(abs_floor)
    else:
        v = np.sort(p)
        floor = 0.5 * (v[M // 2 - 1] + v[M // 2])
    level, sep = floor * 10.0 ** (thr_db / 10.0), 10.0 ** (sep_db / 10.0)
    out = []
    for i in range(M):
        if not (p[i] > level and p[i] > 0.0):
            continue
        if p[(i - 1) % M] > p[i] * sep or p[(i + 1) % M] > p[i] * sep:
            continue
        with np.errstate(divide="ignore"):
            out.append((i - D, (i - D) * rate / 2.0, p[i], np.float32(10.0 * np.log10(p[i] / floor))))
    return out, floor
