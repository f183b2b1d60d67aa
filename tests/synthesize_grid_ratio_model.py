"""float64 model of the grid synthesizer at a ratio (k_synthesize_grid_ratio.hip behind
ofdmrx_util_synthesize_grid_ratio), and the tolerance the device is held to.

The definition.  Handle rate `rate`, ratio P / Q in lowest terms, 1 <= Q <= 16, 2 Q <= P <= 512, P = 2^a 3^b 5^c (section 4.22's
limits), Rw = rate P / Q, M = 2 P.  G[tn], tn = 0 .. 24 P, is section 4.18's sequence G[tn] = H[tn mod Q][tn div Q] over the fp32
table of rechannelize_model.taps(P, Q) (P / Q > 32: the same formula); there is no new filter.  Row c = 0 .. C - 1:
    input   x_c[j], j = 0 .. n_in - 1, interleaved I/Q in S16 or F32, scaled as oracle_lib.pcm_to_cf scales it (fp32); zero outside
    slot    k_c with -P <= k_c Q < P, pairwise distinct, centred at k_c rate / 2 = k_c Q / M cycles per wideband sample
    start   start_c >= 0 in wideband samples, a multiple of P; sigma_c = start_c / P: the row starts sigma_c Q input samples in
    gain    G_c = (P / Q) gain_c, formed in double, rounded once to fp32 (resynthesize_model.gain32)
and at absolute wideband index m, with J = (m Q) div P, beta = (m Q) mod P:
    w[m] = sum_c G_c exp(+2 pi i (k_c Q m mod M) / M) sum_a G[beta + a P] x_c[J - a - sigma_c Q]     a = 0 .. 23, and a = 24 where beta = 0.
`direct` evaluates this as it stands in float64, the exponent reduced mod M in integers.  It is section 4.18's output for the centres
k_c rate / 2 without that section's rounding of the phase increment.  `grid` evaluates the computed form in float64,
    X_j[(-k_c) mod M] = (-1)^{k_c j} (G_c x_c[j - sigma_c Q]),   every other entry 0             (j: absolute input time)
    V_j[r] = sum_b X_j[b] exp(-2 pi i b r / M),  r = 0 .. M - 1                                  (numpy.fft.fft)
    w[m]   = sum_a G[beta + a P] V_{J - a}[beta + (a mod 2) P],                                  V_j = 0 for j < 0.
(With m Q = J P + beta and j = J - a: k Q m / M = k j / 2 + k (beta + a P) / M; the first term is the sign, (beta + a P) mod M is
beta or beta + P, and the slot at bin -k turns e^{+2 pi i k r / M} into the forward transform's e^{-2 pi i b r / M}.  The transform
index is k, not k Q as in section 4.22.)

The order the device keeps.  G_c x is one fp32 product per component, the sign is exact.  The transform is section 4.22's plan run
the other way, decimation in time, in place (`transform_dit`): the sample of bin b enters at channelize_grid_ratio_model.rows(M)[b]
(digit-reversed order), and the plan's stages run from the last to the first - a lone 2, the 4s, the 3s, the 5s.  A stage of radix R
on blocks of N = R L points: the points i + t L, t = 1 .. R - 1, of a block (j = i mod L) are multiplied by w^(j t M / N), w =
exp(-2 pi i / M) rounded once from double (not at L = 1), then the R points go through the butterfly of length R
(channelize_grid_ratio_model._bfly: dev_common.h's) and stand at i + t L again.  Natural order out.  This is the transposed flow graph
of section 4.22's stage: the butterfly matrices are symmetric, the twiddles diagonal, and the DFT matrix is its own transpose.  w[m]
is one chain of fused multiply-adds per component from +0, a ascending, the 25th term only where beta = 0.  Every output passes
through v + 0.f: a zero is always +0.  F32 output: (re, im) of w[m]; S16 output: quantise() of it.

The tolerance, per component of an output, derived here from the arithmetic and from nothing the device gives.  With u = 2^-24 and
    S[m] = sum_c |G_c| sum_a |G[beta + a P]| (|re| + |im|)(x_c[J - a - sigma_c Q]):
    tol[m] = 2^-24 (A + sum over the plan's stages of B_R) S[m],   A = 28,  B_2 = 6,  B_4 = 7,  B_3 = 12,  B_5 = 18.
  * A is section 4.20's constant, term by term (synthesize_grid_model.py): a component of V_j[r] is at most N_j = sum_c |G_c|
    (|re| + |im|)(x_c[j - sigma_c Q]) whatever r, and S[m] = sum_a |G[beta + a P]| N_{J - a} bounds every partial sum of the chain;
    the chain is at most 25 fused multiply-adds (25 u S), the product G_c x rounds once and can grow by sqrt 2 once on its way
    (1.42 u S), and 1 u S is kept for the input's conversion: 25 + 1.42 + 1 <= 28.  Nothing in it looks at which taps a chain takes;
  * the B_R are section 4.22's, re-derived here for the order twiddle-before-butterfly.  There a stage is butterfly, then a product
    with a root on R - 1 of its outputs: (c_R + t) sqrt 2 with t = 0.5 + 1.42 + 1 = 2.92 u for the product (the root's own rounding,
    two partial products weighted by |Re w| + |Im w| <= sqrt 2, their fused sum) and c_R u for the butterfly (c_2 = 1, c_4 = 2,
    c_3 = 5.1, c_5 = 9.23), relative to the l1 magnitude passing the stage, which is at most N_j.  Here the product comes first, on
    R - 1 of the R inputs, each of which it moves by at most t u of its own magnitude; the butterfly then passes those errors on with
    factors of modulus at most 1 per input (every butterfly output is a sum of the inputs times numbers of modulus 1) and adds its
    own c_R u of the l1 magnitude of its inputs, which the roots of modulus 1 have not enlarged beyond the sqrt 2 the count already
    carries.  Per stage: at most (t + c_R) u of the magnitude that passes it, then the sqrt 2 of a component on its way out - the same
    sum in the other order, never more (point 0 of every block and every point at L = 1 is not multiplied at all).  So B_2 = 5.6 <= 6,
    B_4 = 7.0, B_3 = 11.4 <= 12, B_5 = 17.2 <= 18: neither order is larger, and the figures of 4.22 stand;
  * there is no final rotation (4.22's C): the phase is the transform's own.
The rule is homogeneous in x: for F32 input nothing is added.  Where no row reaches m, S[m] = 0: the tolerance is 0 and the output
must be +0 exactly.  An fp32 numpy evaluation in the documented order (grid_fp32 below; products and sums rounded separately, which
is pessimistic) stays well inside the rule (test_synthesize_grid_ratio_model_cpu.py prints the figures)."""
import numpy as np

import channelize_grid_ratio_model as CGR
import resynthesize_model as RS
import synthesize_grid_model as SG
import synthesize_model as SM

A_TOL = SG.A_TOL
B_TOL = CGR.B_TOL

to_cf, quantise, worst, random_x = SM.to_cf, SM.quantise, SM.worst, SM.random_x
reduce, is_plain_grid, plan, rows, all_slots, slot_range, centres = CGR.reduce, CGR.is_plain_grid, CGR.plan, CGR.rows, CGR.all_slots, CGR.slot_range, CGR.centres
sequence, gain32 = RS.sequence, RS.gain32


def tile(P, Q):
    """input times per workgroup of the transform kernel (the tests put rows at its edges): section 4.22's tile - 4096 points, 8 ..
    256 times where 60 KiB of LDS allow it, an even number"""
    M = 2 * P
    nt = min(max(4096 // M, 8), 256)
    nt = min(nt, (61440 - 8 * M) // (8 * M + 4))
    return nt & ~1


def filter_tile(P, Q):
    """outputs per workgroup of the filter kernel (the tests put windows at its edges).  Q > 1: 1024, a lane per output, counted from
    the call's first output; Q = 1: 8 output times per work item, 256 / P groups of P work items (one group from P = 256 on), counted
    from out_first rounded down to a multiple of P"""
    return 1024 if Q > 1 else 8 * P * max(256 // P, 1)


def filter_base(P, Q, out_first):
    """where the filter kernel's tiles are counted from"""
    return out_first if Q > 1 else out_first // P * P


def tol_factor(M):
    return A_TOL + sum(B_TOL[r] for r in plan(M))


def support(start, n_in, P, Q):
    """the last wideband index a row reaches"""
    return RS.support(start, n_in, P, Q)


def n_outputs(starts, n_in, P, Q):
    return RS.n_outputs(starts, n_in, P, Q)


def _check(x, P, Q, slots, starts, gains, out_first, n_out):
    if reduce(P, Q) != (P, Q):
        raise ValueError("P / Q in lowest terms: Q 1 .. 16, P 2 Q .. 512 with no prime factor other than 2, 3 and 5")
    k0, n_all = slot_range(P, Q)
    if x.ndim != 3 or x.shape[2] != 2 or x.shape[0] < 1 or x.shape[1] < 1 or x.dtype not in (np.dtype(np.int16), np.dtype(np.float32)):
        raise ValueError("input must be [C, n_in, 2] of int16 or float32")
    if not (len(slots) == len(starts) == len(gains) == x.shape[0]) or x.shape[0] > n_all:
        raise ValueError("one slot, start and gain per row, at most n_all rows")
    if len(set(slots)) != len(slots) or not all(k0 <= k < k0 + n_all for k in slots):
        raise ValueError("the slots are pairwise distinct and lie in -P <= k Q < P")
    if not all(0 <= s <= 1 << 50 and s % P == 0 for s in starts) or not 0 <= int(out_first) <= 1 << 50:
        raise ValueError("a start or out_first is negative or above 2^50, or P does not divide a start")
    if not all(np.isfinite(np.float32(g)) and np.isfinite(gain32(P, Q, g)) for g in gains):
        raise ValueError("a gain is not finite")
    if n_out is not None and n_out < 1:
        raise ValueError("n_out must be positive")


def _args(x, P, Q, slots, starts, gains, out_first, n_out):
    x = np.ascontiguousarray(x)
    slots = [int(k) for k in (all_slots(P, Q) if slots is None else np.atleast_1d(slots))]
    starts = [int(s) for s in np.atleast_1d(starts)]
    gains = [float(g) for g in np.atleast_1d(np.asarray(gains, np.float64))]
    _check(x, P, Q, slots, starts, gains, out_first, n_out)
    if n_out is None:
        n_out = n_outputs(starts, x.shape[1], P, Q) - out_first
    return x, slots, starts, gains, int(n_out)


def _gather(a, i):
    """a[i] where 0 <= i < len(a), else 0"""
    ok = (i >= 0) & (i < len(a))
    return np.where(ok, a[np.clip(i, 0, len(a) - 1)], 0)


def bound(x, P, Q, slots, starts, gains, out_first=0, n_out=None):
    """-> tol [n_out]: the rule of the header"""
    x, slots, starts, gains, n_out = _args(x, P, Q, slots, starts, gains, out_first, n_out)
    G = np.abs(sequence(P, Q))
    m = np.arange(n_out, dtype=np.int64) + out_first
    J, beta = (m * Q) // P, (m * Q) % P
    S = np.zeros(n_out, np.float64)
    for c in range(x.shape[0]):
        xc = to_cf(x[c])
        ax = abs(float(gain32(P, Q, gains[c]))) * (np.abs(xc.real) + np.abs(xc.imag))
        for a in range(25):
            t = beta + a * P
            S += np.where(t <= 24 * P, G[np.minimum(t, 24 * P)] * _gather(ax, J - a - starts[c] // P * Q), 0.0)
    return 2.0 ** -24 * tol_factor(2 * P) * S


def direct(x, P, Q, slots, starts, gains, outputs):
    """the definition as it stands at the absolute wideband indices `outputs` -> [len(outputs)] complex128"""
    x, slots, starts, gains, _ = _args(x, P, Q, slots, starts, gains, 0, None)
    G = sequence(P, Q)
    M = 2 * P
    m = np.asarray(outputs, np.int64)
    J, beta = (m * Q) // P, (m * Q) % P
    v = np.zeros(len(m), np.complex128)
    for c in range(x.shape[0]):
        xc = to_cf(x[c])
        u = np.zeros(len(m), np.complex128)
        for a in range(25):
            t = beta + a * P
            u += np.where(t <= 24 * P, G[np.minimum(t, 24 * P)] * _gather(xc, J - a - starts[c] // P * Q), 0.0)
        ph = ((slots[c] * Q) * (m % M)) % M                          # integers: exact
        v += float(gain32(P, Q, gains[c])) * np.exp(2j * np.pi * ph.astype(np.float64) / M) * u
    return v


def transform_dit(re, im, M, f=np.float64, conj3=False):
    """[n, M] -> [n, M]: the plan's forward transform run the other way, `rows` order in, natural order out; every operation rounds
    on its own in f"""
    wr, wi = CGR.roots(M, f)
    n, N = re.shape[0], 1
    for R in reversed(plan(M)):
        N *= R
        L = N // R
        zr, zi = re.reshape(n, M // N, R, L), im.reshape(n, M // N, R, L)
        pts = []
        for t in range(R):
            a, b = zr[:, :, t, :], zi[:, :, t, :]
            if t and L > 1:
                idx = np.arange(L) * t * (M // N)
                c, s = wr[idx], wi[idx]
                a, b = a * c - b * s, a * s + b * c
            pts.append((a, b))
        out = CGR._bfly(R, pts, f, conj3)
        nr, ni = np.empty_like(zr), np.empty_like(zi)
        for t in range(R):
            nr[:, :, t, :], ni[:, :, t, :] = out[t]
        re, im = nr.reshape(n, M), ni.reshape(n, M)
    return re, im


VARIANTS = ("bin +k", "no (-1)^(k j)", "V rows exchanged", "bin k Q", "gain without P / Q", "start off by P", "sigma in place of sigma Q",
            "J rounded", "beta of m", "radix-3 root conjugated", "re / im swapped", "M = P", "slot k + 1", "scaled by 1 / M", "output at m + 1")
# the variants that are the definition itself at Q = 1 (a test holds them to it there, and rejects them at Q > 1)
VARIANTS_Q = ("bin k Q", "sigma in place of sigma Q", "beta of m")


def grid(x, P, Q, slots, starts, gains, out_first=0, n_out=None, variant=None):
    """x: [C, n_in, 2] int16 or float32 -> (v [n_out] complex128, tol [n_out]): the computed form through numpy.fft.  slots None: all,
    ascending; variant: one of VARIANTS, a deliberately wrong model (its tol is the definition's).  Q = 1 with P a power of two is
    section 4.20 itself: its model, its tolerance"""
    if variant is None and is_plain_grid(P, Q):
        return SG.grid(x, P, slots, starts, gains, out_first, n_out)
    x, slots, starts, gains, n_out = _args(x, P, Q, slots, starts, gains, out_first, n_out)
    tol = bound(x, P, Q, slots, starts, gains, out_first, n_out)
    G = sequence(P, Q)
    M = P if variant == "M = P" else 2 * P
    m = np.arange(n_out, dtype=np.int64) + out_first - (1 if variant == "output at m + 1" else 0)
    J, beta = (m * Q) // P, (m * Q) % P
    if variant == "J rounded":
        J = (2 * m * Q + P) // (2 * P)
    if variant == "beta of m":
        beta = m % P
    j0, j1 = int(J.min()) - 24, int(J.max())
    j = np.arange(j0, j1 + 1, dtype=np.int64)
    X = np.zeros((len(j), M), np.complex128)
    for c in range(x.shape[0]):
        xc = to_cf(x[c])
        if variant == "re / im swapped":
            xc = xc.imag + 1j * xc.real
        Gc = float(np.float32(gains[c])) if variant == "gain without P / Q" else float(gain32(P, Q, gains[c]))
        sg = starts[c] // P + (1 if variant == "start off by P" else 0)
        k = slots[c] + (1 if variant == "slot k + 1" else 0)
        val = Gc * _gather(xc, j - (sg if variant == "sigma in place of sigma Q" else sg * Q))
        if variant != "no (-1)^(k j)":
            val = np.where((k * j) % 2 == 1, -val, val)
        b = k if variant == "bin +k" else -k * Q if variant == "bin k Q" else -k
        X[:, b % M] += val
    if variant == "radix-3 root conjugated":
        row = rows(M)
        re, im = transform_dit(X.real[:, np.argsort(row)].copy(), X.imag[:, np.argsort(row)].copy(), M, conj3=True)
        V = re + 1j * im
    else:
        V = np.fft.fft(X, axis=1)
    if variant == "scaled by 1 / M":
        V = V / M
    v = np.zeros(n_out, np.complex128)
    for a in range(25):
        t = beta + a * P
        odd = (a + 1) % 2 if variant == "V rows exchanged" else a % 2
        r = (beta + odd * P) % M
        ok = (t <= 24 * P) & (J - a >= j0)
        v += np.where(ok, G[np.minimum(t, 24 * P)] * V[np.clip(J - a - j0, 0, len(j) - 1), r], 0.0)
    return v, tol


def grid_fp32(x, P, Q, slots, starts, gains, out_first=0, n_out=None):
    """an fp32 numpy evaluation of the computed form in the documented order: G x one fp32 product, the decimation-in-time plan in
    fp32 with roots rounded once, the output's chain with a ascending (products and sums rounded separately, no fused multiply-add)
    -> [n_out] complex64"""
    f32 = np.float32
    x, slots, starts, gains, n_out = _args(x, P, Q, slots, starts, gains, out_first, n_out)
    G = sequence(P, Q).astype(f32)
    M = 2 * P
    m = np.arange(n_out, dtype=np.int64) + out_first
    J, beta = (m * Q) // P, (m * Q) % P
    j0, j1 = int(J.min()) - 24, int(J.max())
    j = np.arange(j0, j1 + 1, dtype=np.int64)
    row = rows(M)
    re, im = np.zeros((len(j), M), f32), np.zeros((len(j), M), f32)
    for c in range(x.shape[0]):
        xc = SM.O.pcm_to_cf(x[c]).astype(f32)
        g = gain32(P, Q, gains[c])
        i = j - starts[c] // P * Q
        ok = (i >= 0) & (i < x.shape[1])
        ii = np.clip(i, 0, x.shape[1] - 1)
        sign = np.where((slots[c] * j) % 2 == 1, f32(-1), f32(1))
        at = row[(-slots[c]) % M]
        re[:, at] = np.where(ok, sign * (g * xc[ii, 0]), f32(0))
        im[:, at] = np.where(ok, sign * (g * xc[ii, 1]), f32(0))
    vr, vi = transform_dit(re, im, M, f32)
    wr, wi = np.zeros(n_out, f32), np.zeros(n_out, f32)
    for a in range(25):
        t = beta + a * P
        ok = (t <= 24 * P) & (J - a >= j0)
        hk = G[np.minimum(t, 24 * P)]
        rw, col = np.clip(J - a - j0, 0, len(j) - 1), beta + (a % 2) * P
        wr = np.where(ok, wr + hk * vr[rw, col], wr)
        wi = np.where(ok, wi + hk * vi[rw, col], wi)
    return wr + 1j * wi
