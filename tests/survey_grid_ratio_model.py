"""float64 model of the grid survey at a ratio (k_survey_grid_ratio.hip behind ofdmrx_util_survey_grid_ratio),
the tolerance the device is held to, and a float64 restatement of the slot finder at a ratio (ofdmrx_util_find_slots_ratio).

The definition.  Symbols are section 4.22's (channelize_grid_ratio_model.py): P / Q in lowest terms, 1 <= Q <= 16, 2 Q <= P <= 512,
P = 2^a 3^b 5^c; M = 2 P, T = 24 P div Q + 1, the taps h_q[j]; output times u_n = n P, i_n = u_n div Q, q_n = u_n mod Q; the slots
k_first = -(P div Q) .. k_first + n_all - 1, the k with -P <= k Q < P, ascending; y_k[n] the ratio grid front end's output at ABSOLUTE
output time n with x zero at negative positions.  S = times_per_row is a multiple of 8 in 8 .. 65536.  Row r >= 0:
    P[r][k - k_first] = (1 / S) sum_{n = r S .. r S + S - 1} |y_k[n]|^2
n_all floats in ascending slot order with no further normalisation.  Row r needs the wideband positions
max(0, (r S P) div Q - 24 P div Q) .. (((r + 1) S - 1) P) div Q (`span`).  `power` evaluates this in float64 on
channelize_grid_ratio_model.grid's outputs; the final rotation by the root of k Q i_n mod M has modulus 1 - a kernel that left it out
(the device's does) cannot be told from one that applied it by any power, so "no rotation" is NOT among the wrong variants below.

The tolerance is section 4.21's rule (survey_grid_model.py derives it term by term) with section 4.22's bound in place of 4.19's.
With u = 2^-24 and e_n = sqrt 2 x channelize_grid_ratio_model.bound at time n (per component, the same for every slot) - the most
the computed y_k[n] is off in modulus:
    tol[r][k] = (1 / S) sum_n (2 |y_k[n]| e_n + e_n^2)  +  (8 + S / 8 + 4) u (P[r][k] + that)
4.22's bound includes its constant C for the final rotation, which the survey does not perform: the bound is then a little wider
than the survey's arithmetic needs, never narrower.  For F32 input nothing is added: the rule is homogeneous of degree 2 in x.
`power_fp32` evaluates the documented order in fp32 numpy on channelize_grid_ratio_model.grid_fp32's outputs;
test_survey_grid_ratio_model_cpu.py prints how far it stays under the rule."""
import numpy as np

import channelize_grid_ratio_model as GR
import channelize_model as CM

U = 2.0 ** -24
GROUP = 8
to_cf, random_pcm = CM.to_cf, CM.random_pcm

VARIANTS = ("slot k + 1", "mirrored slot -k", "a row of M columns", "row starts at r S + 1", "1 / S missing", "|y| for |y|^2", "re only",
            "bin k in place of k Q", "taps of phase q + 1", "fraction ignored", "i_n rounded")
# the variants that are the definition itself at Q = 1 (a test holds them to it there, and rejects them at Q > 1)
VARIANTS_Q = ("a row of M columns", "bin k in place of k Q", "taps of phase q + 1", "fraction ignored", "i_n rounded")


def span(P, Q, S, row_first, n_rows):
    """-> (first position, count) the rows row_first .. row_first + n_rows - 1 need"""
    first = max(0, (row_first * S * P) // Q - 24 * P // Q)
    return first, (((row_first + n_rows) * S - 1) * P) // Q - first + 1


def outputs(pcm, P, Q, n0, n, in_first=0, variant=None):
    """-> (y [n, columns] complex128 whose modulus is |y_k[n]|, ascending slot order;  e [n]: sqrt 2 x 4.22's per-component bound)
    for the absolute output times n0 .. n0 + n - 1"""
    k = GR.all_slots(P, Q)
    gv = variant if variant in GR.VARIANTS else None
    if variant == "mirrored slot -k":
        k = -k
    if variant == "a row of M columns":                               # 4.21's row: column i is bin i - P of the transform
        k, gv = np.arange(-P, P, dtype=np.int64), "bin k in place of k Q"
    v, tol = GR.grid(pcm, P, Q, k, n0, n, in_first, variant=gv)     # (tol: the definition's bound, one row per slot, all alike)
    return v.T, np.sqrt(2.0) * tol[0]


def power(pcm, P, Q, S, row_first=0, n_rows=1, in_first=0, variant=None):
    """-> (P [n_rows, n_all] float64, tol [n_rows, n_all]).  pcm: the wideband positions in_first ..; variant: one of VARIANTS, a
    deliberately wrong model (M columns for "a row of M columns").  Works row by row"""
    assert S % GROUP == 0 and 8 <= S <= 65536
    Pw, tol = [], []
    for j in range(n_rows):
        n0 = (row_first + j) * S + (1 if variant == "row starts at r S + 1" else 0)
        y, e = outputs(pcm, P, Q, n0, S, in_first, variant)
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
        Pw.append(p)
        tol.append(first + (8 + S / 8 + 4) * U * (p + first))
    return np.array(Pw), np.array(tol)


def worst(got, P, tol):
    """largest |got - P| / tol; a row of another width is infinitely far"""
    got = np.asarray(got, np.float64)
    if got.shape != P.shape:
        return float("inf")
    d = np.abs(got - P)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, d / np.where(tol > 0, tol, 1.0), np.where(d > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def power_fp32(pcm, P, Q, S, n_rows):
    """the documented order in fp32 numpy, rows 0 .. n_rows - 1 of a capture from position 0: |y|^2 = fma(im, im, re re) (the product
    rounded, the fused step formed in double and rounded once), one chain over the 8 times of a group, one over the row's groups,
    one product with fp32(1 / S) -> float32 [n_rows, n_all]"""
    f32 = np.float32
    y = GR.grid_fp32(pcm, P, Q)[:, :n_rows * S]                      # [n_all, times], ascending slots
    assert y.shape[1] == n_rows * S
    re, im = y.real.astype(f32), y.imag.astype(f32)
    rr = (re * re).astype(f32)
    p = (im.astype(np.float64) * im.astype(np.float64) + rr.astype(np.float64)).astype(f32)
    p = p.reshape(y.shape[0], n_rows, S // GROUP, GROUP)
    g = np.zeros(p.shape[:3], f32)
    for t in range(GROUP):
        g = (g + p[..., t]).astype(f32)
    s = np.zeros(p.shape[:2], f32)
    for j in range(S // GROUP):
        s = (s + g[..., j]).astype(f32)
    return (s * f32(1.0 / S)).astype(f32).T


def tone_pcm(W, P, Q, slot, dtype=np.int16, seed=1, amp=0.4, first=0):
    """full scale in sum: 0.6 x uniform random input plus a tone of amplitude amp on the centre of `slot` (k Q / M cycles per sample,
    its phase counted from absolute position 0)"""
    rng = np.random.default_rng(seed)
    M = 2 * P
    m = np.arange(W, dtype=np.int64) + first
    ph = 2.0 * np.pi * ((slot * Q * (m % M)) % M).astype(np.float64) / M
    x = 0.6 * rng.uniform(-1.0, 1.0, size=(W, 2)) + amp * np.stack([np.cos(ph), np.sin(ph)], axis=1)
    if np.dtype(dtype) == np.int16:
        return np.rint(x * 32767.0).astype(np.int16)
    if np.dtype(dtype) == np.uint8:
        return np.clip(np.rint(x * 127.0 + 128.0), 1, 255).astype(np.uint8)
    return x.astype(np.float32)


def noise_reading(P, Q, sigma2=1.0):
    """what white noise of power sigma2 per complex sample reads in every slot over whole periods of Q output times: sigma2 times
    the mean over the tap phases of sum_j h_q[j]^2"""
    return sigma2 * float((GR.taps(P, Q).astype(np.float64) ** 2).sum(axis=1).mean())


def find_slots(row, P, Q, rate, thr_db=6.0, sep_db=8.0, abs_floor=0.0):
    """ofdmrx_util_find_slots_ratio restated in float64 -> ([(slot, centre_hz, power, level_db)], floor): find_slots' floor, occupied
    and shadowed rules on n_all values, neighbours cyclic only where the slots tile the circle, and the ends seen twice (below)"""
    p = np.asarray(row, np.float32).astype(np.float64)
    k0, N = GR.slot_range(P, Q)
    assert p.shape == (N,)
    cyclic = N * Q == 2 * P
    if abs_floor > 0:
        floor = float(abs_floor)
    else:
        v = np.sort(p)
        floor = v[N // 2] if N % 2 else 0.5 * (v[N // 2 - 1] + v[N // 2])
    level, sep = floor * 10.0 ** (thr_db / 10.0), 10.0 ** (sep_db / 10.0)
    keep = np.zeros(N, bool)
    for i in range(N):
        if not (p[i] > level and p[i] > 0.0):
            continue
        below = p[i - 1] if i > 0 else (p[N - 1] if cyclic else 0.0)
        above = p[i + 1] if i < N - 1 else (p[0] if cyclic else 0.0)
        if below > p[i] * sep or above > p[i] * sep:
            continue
        keep[i] = True
    # the ends seen twice: their centres lie 2 r bins apart across the band edge, r = P mod Q, a slot being Q bins; at half a slot or
    # less (0 < 4 r <= Q) both ends within sep_db of each other are one signal and the louder is reported (a tie: k_first)
    r = P % Q
    if not cyclic and 0 < 4 * r <= Q and keep[0] and keep[N - 1]:
        a, b = p[0], p[N - 1]
        if a >= b and not a > b * sep:
            keep[N - 1] = False
        elif b > a and not b > a * sep:
            keep[0] = False
    out = []
    for i in np.flatnonzero(keep):
        with np.errstate(divide="ignore"):
            out.append((k0 + int(i), (k0 + int(i)) * rate / 2.0, p[i], np.float32(10.0 * np.log10(p[i] / floor))))
    return out, floor
