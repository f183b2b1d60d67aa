"""float64 model of the grid front end at a ratio (k_channelize_grid_ratio.hip behind
ofdmrx_util_channelize_grid_ratio), and the tolerance the device is held to.

The definition.  Handle rate `rate`, ratio P / Q in lowest terms, 1 <= Q <= 16, 2 Q <= P <= 512, P = 2^a 3^b 5^c.  Rw = rate P / Q,
M = 2 P, T = floor(24 P / Q) + 1.  The taps h_q[j], q = 0 .. Q - 1, are rechannelize_model.taps(P, Q): section 4.17's formula in
double, each phase normalised to sum 1, rounded once to fp32 (P / Q > 32 is the same formula).  Output time as in 4.17: u_n = n P,
i_n = u_n div Q, q_n = u_n mod Q.  Slot k lies at k rate / 2 = k Q / M cycles per wideband sample; the slots are the k with
-P <= k Q < P, k = -(P div Q) .. ceil(P / Q) - 1.  Input scaled as oracle_lib.pcm_to_cf scales it (fp32).
    y_k[n] = sum_{j = 0 .. T - 1} h_{q_n}[j] x[i_n - j] exp(-2 pi i (k Q (i_n - j) mod M) / M),    x zero at negative indices.
W samples give ceil(W Q / P) outputs.  `direct` evaluates this sum as it stands in float64, the exponent reduced mod M in integers.
`grid` evaluates the computed form in float64:
    u_n[r] = sum_a h_{q_n}[r + M a] x[i_n - r - M a],  r = 0 .. M - 1, over the a with r + M a <= T - 1
    y_k[n] = W^{-(k Q i_n mod M)} sum_r u_n[r] W^{+(k Q mod M) r},  W = exp(2 pi i / M)
with the sum over r taken as bin (-k Q) mod M of a forward transform that follows the device's plan.

The plan of M = 2^a 3^b 5^c (`plan`): c stages of radix 5, then b of radix 3, a div 2 of radix 4, a mod 2 of radix 2; decimation in
frequency, in place.  A stage of radix R on blocks of N points, L = N / R: the points i + t L, t = 0 .. R - 1, of a block (j = i mod L)
go through the butterfly of length R; output t >= 1 is multiplied by w^(j t M / N), w = exp(-2 pi i / M) (not at L = 1), and stands at
i + t L.  Bin b of a block then stands at (b mod R) L + [bin b div R of the sub-block] (`rows`).  The butterflies are dev_common.h's:
    2: (a + b, a - b)
    4: s0 = v0 + v2, s1 = v0 - v2, s2 = v1 + v3, s3 = -i (v1 - v3); (s0 + s2, s1 + s3, s0 - s2, s1 - s3)
    3: a = v1 + v2, b = v1 - v2, m = v0 - a / 2, n = -i sin(pi / 3) b; (v0 + a, m + n, m - n)
    5: a1 = v1 + v4, a2 = v2 + v3, b1 = v1 - v4, b2 = v2 - v3, c_i = cos(2 pi i / 5), s_i = sin(2 pi i / 5),
       m1 = v0 + c1 a1 + c2 a2, m2 = v0 + c2 a1 + c1 a2, n1 = -i (s1 b1 + s2 b2), n2 = -i (s2 b1 - s1 b2);
       (v0 + (a1 + a2), m1 + n1, m2 + n2, m2 - n2, m1 - n1)

The tolerance, per component of an output, derived here from the arithmetic the kernel performs and from nothing the device gives:
    tol = 2^-24 (A + sum over the plan's stages of B_R + C) S,    S = sum_j |h_{q_n}[j]| (|re| + |im|)(x[i_n - j]),
    A = 16,  B_2 = 6,  B_4 = 7,  B_3 = 12,  B_5 = 18,  C = 5.
With u = 2^-24 (half an ulp, relative), and section 4.19's derivation (channelize_grid_model.py) term by term:
  * the branch chain is 4.19's: at most 13 fused multiply-adds per component (T <= 12 M + 1), 1 u for the input: A = 16;
  * a root (of a stage or of the final rotation) is rounded once from double, each component within u / 2; the product of a value z
    with it rounds its two partial products once each, weighted by |Re w| + |Im w| <= sqrt 2 (1.42 u), and their fused sum once more
    (1 u): a component moves by at most t = 0.5 + 1.42 + 1 = 2.92 u of (|re| + |im|)(z);
  * what passes a stage is bounded as in 4.19 by S, and a component of an earlier error grows by at most sqrt 2 once on its way
    out: a stage whose butterfly moves a component by at most c u of the l1 magnitude of its inputs costs (c + t) sqrt 2 u S;
  * radix 2: one addition, c = 1: (1 + 2.92) sqrt 2 = 5.6 <= 6, 4.19's figure;
  * radix 4: two additions in a row, the second passing the first's rounding on; the turn by -i is exact: c = 2, 4.92 sqrt 2 = 7.0;
  * radix 3: the rounding of a enters output 1 halved (0.5); m rounds once (1; a / 2 is exact); b's rounding, the constant's (within
    u of sin(pi / 3)) and the product's each weigh sin(pi / 3) = 0.87 (2.6); the last addition (1): c = 5.1, 8.02 sqrt 2 = 11.4 <= 12;
  * radix 5: the roundings of a1, a2, of the two constants and of the two products weigh at most |c2| = 0.81 each (2.43), the two
    additions of m (2); the roundings of b1, b2, of the constants, of the products and of n's addition weigh at most s1 = 0.95 each
    (3.8); the last addition (1): c = 9.23, 12.15 sqrt 2 = 17.2 <= 18.  (Output 0 of either butterfly is a plain sum of fewer terms.)
    Where the compiler contracts a product and a sum into one fused operation a rounding falls away: never more;
  * the final rotation is one product with a root, of a value whose l1 magnitude is at most sqrt 2 S: 2.92 sqrt 2 = 4.2 <= C = 5.
For F32 input nothing is added: the bound is homogeneous in x.  An fp32 numpy evaluation of the same plan (grid_fp32 below, products
and sums rounded separately) stays under 0.05 of the rule on full-scale random int16 (test_channelize_grid_ratio_model_cpu.py prints
the figures)."""
import math

import numpy as np

import channelize_grid_model as G
import channelize_model as CM
import rechannelize_model as RM

A_TOL, C_TOL = 16.0, 5.0
B_TOL = {2: 6.0, 4: 7.0, 3: 12.0, 5: 18.0}
CHUNK = 256                                                         # outputs formed at a time

to_cf, worst, random_pcm = CM.to_cf, CM.worst, CM.random_pcm
n_outputs, n_taps, _gather = RM.n_outputs, RM.n_taps, RM._gather


def reduce(P, Q):
    """-> (P, Q) in lowest terms, or None where the definition refuses the ratio"""
    if P <= 0 or Q <= 0:
        return None
    g = math.gcd(P, Q)
    P, Q = P // g, Q // g
    m = P
    for f in (2, 3, 5):
        while m % f == 0:
            m //= f
    if Q > 16 or P < 2 * Q or P > 512 or m != 1:
        return None
    return P, Q


def is_plain_grid(P, Q):
    """Q = 1 with P a power of two: section 4.19 itself - its kernel, its model, its tolerance"""
    return Q == 1 and P & (P - 1) == 0


def plan(M):
    """the radices of the stages, first stage first"""
    out, m = [], M
    for r in (5, 3, 4):
        while m % r == 0:
            out.append(r)
            m //= r
    if m == 2:
        out.append(2)
        m = 1
    assert m == 1, M
    return out


def rows(M, radices=None):
    """row[b]: where bin b stands behind the transform"""
    radices = plan(M) if radices is None else radices
    b = np.arange(M)
    row, n = np.zeros(M, np.int64), M
    for r in radices:
        n //= r
        row += (b % r) * n
        b = b // r
    return row


def slot_range(P, Q):
    """-> (k_first, n_all)"""
    return -(P // Q), -(-P // Q) + P // Q


def all_slots(P, Q):
    k0, n = slot_range(P, Q)
    return np.arange(k0, k0 + n, dtype=np.int64)


def centres(P, Q, rate=8000, slots=None):
    k = all_slots(P, Q) if slots is None else np.asarray(slots, np.int64)
    return k.astype(np.float64) * (rate / 2.0)


def taps(P, Q):
    """[Q, T] float32"""
    return RM.taps(P, Q)


def tol_factor(M):
    return A_TOL + sum(B_TOL[r] for r in plan(M)) + C_TOL


def _times(P, Q, out_first, n_out):
    u = (np.arange(n_out, dtype=np.int64) + out_first) * P
    return u // Q, u % Q


def bound(pcm, P, Q, out_first=0, n_out=None, in_first=0):
    """-> tol [n_out]: the rule of the header, the same for every slot"""
    x = to_cf(pcm)
    if n_out is None:
        n_out = n_outputs(in_first + len(x), P, Q) - out_first
    H = np.abs(taps(P, Q).astype(np.float64))
    absx = np.abs(x.real) + np.abs(x.imag)
    jt = np.arange(H.shape[1], dtype=np.int64)
    S = np.zeros(n_out, np.float64)
    for a in range(0, n_out, CHUNK):
        i_n, q_n = _times(P, Q, out_first + a, min(CHUNK, n_out - a))
        S[a:a + len(i_n)] = (H[q_n] * _gather(absx, in_first, i_n[:, None] - jt[None, :])).sum(axis=1)
    return 2.0 ** -24 * tol_factor(2 * P) * S


def direct(pcm, P, Q, slots, outputs, in_first=0):
    """the definition as it stands, for the outputs n in `outputs` -> [len(slots), len(outputs)] complex128"""
    x = to_cf(pcm)
    H = taps(P, Q).astype(np.float64)
    T, M = H.shape[1], 2 * P
    out = np.zeros((len(slots), len(outputs)), np.complex128)
    j = np.arange(T, dtype=np.int64)
    for jn, n in enumerate(outputs):
        un = int(n) * P
        i_n, q_n = un // Q, un % Q
        m = i_n - j
        xs = _gather(x, in_first, m)
        for i, k in enumerate(slots):
            ph = ((int(k) * Q) * (m % M)) % M                       # integers: exact
            out[i, jn] = np.sum(H[q_n] * xs * np.exp(-2j * np.pi * ph.astype(np.float64) / M))
    return out


# ---- the butterflies on (re, im) pairs of arrays of one dtype; every operation rounds on its own
def _add(a, b):
    return a[0] + b[0], a[1] + b[1]


def _sub(a, b):
    return a[0] - b[0], a[1] - b[1]


def _negj(a):
    return a[1], -a[0]


def _bfly(R, v, f, conj3=False):
    if R == 2:
        return [_add(v[0], v[1]), _sub(v[0], v[1])]
    if R == 4:
        s0, s1 = _add(v[0], v[2]), _sub(v[0], v[2])
        s2, s3 = _add(v[1], v[3]), _negj(_sub(v[1], v[3]))
        return [_add(s0, s2), _add(s1, s3), _sub(s0, s2), _sub(s1, s3)]
    if R == 3:
        s, half = f(math.sin(math.pi / 3)), f(0.5)
        a, b = _add(v[1], v[2]), _sub(v[1], v[2])
        m = (v[0][0] - half * a[0], v[0][1] - half * a[1])
        jn = _negj((s * b[0], s * b[1]))
        o1, o2 = _add(m, jn), _sub(m, jn)
        return [_add(v[0], a), o2, o1] if conj3 else [_add(v[0], a), o1, o2]
    c1, c2 = f(math.cos(2 * math.pi / 5)), f(math.cos(4 * math.pi / 5))
    s1, s2 = f(math.sin(2 * math.pi / 5)), f(math.sin(4 * math.pi / 5))
    a1, a2 = _add(v[1], v[4]), _add(v[2], v[3])
    b1, b2 = _sub(v[1], v[4]), _sub(v[2], v[3])
    m1 = (v[0][0] + c1 * a1[0] + c2 * a2[0], v[0][1] + c1 * a1[1] + c2 * a2[1])
    m2 = (v[0][0] + c2 * a1[0] + c1 * a2[0], v[0][1] + c2 * a1[1] + c1 * a2[1])
    n1 = (s1 * b1[0] + s2 * b2[0], s1 * b1[1] + s2 * b2[1])
    n2 = (s2 * b1[0] - s1 * b2[0], s2 * b1[1] - s1 * b2[1])
    j1, j2 = _negj(n1), _negj(n2)
    return [_add(v[0], _add(a1, a2)), _add(m1, j1), _add(m2, j2), _sub(m2, j2), _sub(m1, j1)]


def roots(M, f=np.float64):
    """exp(-2 pi i j / M), j = 0 .. M - 1, made in double (as the library makes them: from pi j / P) and rounded once"""
    j = np.arange(M, dtype=np.float64)
    return np.cos(np.pi * j / (M // 2)).astype(f), (-np.sin(np.pi * j / (M // 2))).astype(f)


def transform(re, im, M, f=np.float64, conj3=False):
    """[n, M] -> [n, M]: the plan's forward transform, natural order in, `rows` order out"""
    wr, wi = roots(M, f)
    n, N = re.shape[0], M
    for R in plan(M):
        L = N // R
        zr, zi = re.reshape(n, M // N, R, L), im.reshape(n, M // N, R, L)
        out = _bfly(R, [(zr[:, :, t, :], zi[:, :, t, :]) for t in range(R)], f, conj3)
        nr, ni = np.empty_like(zr), np.empty_like(zi)
        for t in range(R):
            a, b = out[t]
            if t and L > 1:
                idx = np.arange(L) * t * (M // N)
                c, s = wr[idx], wi[idx]
                a, b = a * c - b * s, a * s + b * c
            nr[:, :, t, :], ni[:, :, t, :] = a, b
        re, im = nr.reshape(n, M), ni.reshape(n, M)
        N = L
    return re, im


VARIANTS = ("bin k in place of k Q", "no rotation", "rotation by n", "taps of phase q + 1", "fraction ignored", "i_n rounded", "M = P",
            "transform sign", "radix-3 root conjugated", "branch M - r", "slot k + 1", "re / im swapped")
# the variants that are the definition itself at Q = 1 (a test holds them to it there, and rejects them at Q > 1)
VARIANTS_Q = ("bin k in place of k Q", "taps of phase q + 1", "fraction ignored", "i_n rounded")


def grid(pcm, P, Q, slots=None, out_first=0, n_out=None, in_first=0, variant=None):
    """-> (v [n_slots, n_out] complex128, tol [n_slots, n_out]).  pcm: the wideband positions in_first ..; slots None: all, ascending;
    variant: one of VARIANTS, a deliberately wrong model (tol is always the definition's)"""
    if variant is None and is_plain_grid(P, Q):
        return G.grid(pcm, P, slots, out_first, n_out, in_first)
    x = to_cf(pcm)
    if n_out is None:
        n_out = n_outputs(in_first + len(x), P, Q) - out_first
    k = all_slots(P, Q) if slots is None else np.asarray(slots, np.int64)
    H = taps(P, Q).astype(np.float64)
    T = H.shape[1]
    if variant == "re / im swapped":
        x = x.imag + 1j * x.real
    M = P if variant == "M = P" else 2 * P
    kk = k + 1 if variant == "slot k + 1" else k
    kq = (kk * Q) % M
    kbin = kk % M if variant == "bin k in place of k Q" else kq
    row = rows(M)
    na = -(-T // M)
    j = np.arange(T, dtype=np.int64)
    v = np.zeros((len(k), n_out), np.complex128)
    for a in range(0, n_out, CHUNK):
        nn = min(CHUNK, n_out - a)
        i_n, q_n = _times(P, Q, out_first + a, nn)
        n = np.arange(nn, dtype=np.int64) + out_first + a
        if variant == "fraction ignored":
            q_n = np.zeros_like(q_n)
        if variant == "taps of phase q + 1":
            q_n = (q_n + 1) % Q
        if variant == "i_n rounded":
            i_n = (2 * n * P + Q) // (2 * Q)
        g = np.zeros((nn, na * M), np.complex128)
        g[:, :T] = H[q_n] * _gather(x, in_first, i_n[:, None] - j[None, :])
        u = g.reshape(nn, na, M).sum(axis=1)                        # the branch sums, a ascending
        if variant == "branch M - r":
            u = u[:, (-np.arange(M)) % M]
        re, im = transform(u.real.copy(), u.imag.copy(), M, conj3=variant == "radix-3 root conjugated")
        X = re + 1j * im
        b = kbin if variant == "transform sign" else (-kbin) % M
        y = X[:, row[b]].T                                          # [n_slots, nn]
        if variant != "no rotation":
            at = n if variant == "rotation by n" else i_n
            ph = (kq[:, None] * (at % M)[None, :]) % M
            y = y * np.exp(-2j * np.pi * ph.astype(np.float64) / M)
        v[:, a:a + nn] = y
    tol = np.broadcast_to(bound(pcm, P, Q, out_first, n_out, in_first), v.shape).copy()
    return v, tol


def wide_rows(pcm, P, Q, slots):
    """the model's rows over a whole long capture from position 0 -> float32 [n_slots, ceil(W Q / P), 2]: the same sum in float64,
    arranged per slot as a mix-down by the exact phase (k Q m mod M) and, for the outputs n = c + Q t of one residue c mod Q (one tap
    phase, i_n = i_c + P t), P branch convolutions (tap b + P a against sample i_c - b + P (t - a));
    test_channelize_grid_ratio_model_cpu.py holds it to `grid`"""
    x = to_cf(pcm)
    H = taps(P, Q).astype(np.float64)
    M, W = 2 * P, len(x)
    n_out = n_outputs(W, P, Q)
    m = np.arange(W, dtype=np.int64)
    out = np.zeros((len(slots), n_out, 2), np.float32)
    for i, k in enumerate(slots):
        xm = np.zeros(P + (n_out // Q + 2) * P, np.complex128)      # positions -P .. (zeros before and past the capture)
        xm[P:P + W] = x * np.exp(-2j * np.pi * (((int(k) * Q) * (m % M)) % M).astype(np.float64) / M)
        y = np.zeros(n_out, np.complex128)
        for c in range(min(Q, n_out)):
            i_c, q_c = (c * P) // Q, (c * P) % Q
            nt = len(range(c, n_out, Q))
            acc = np.zeros(nt, np.complex128)
            for b in range(P):
                hb = H[q_c][b::P]
                if len(hb):
                    acc += np.convolve(xm[P + i_c - b::P][:nt], hb)[:nt]
            y[c::Q] = acc
        out[i, :, 0], out[i, :, 1] = y.real, y.imag
    return out


def grid_fp32(pcm, P, Q, slots=None):
    """an fp32 numpy evaluation of the computed form from position 0: the branch chains with a ascending, the plan's transform and the
    final rotation, every product and sum rounded to fp32 on its own (no fused multiply-add) -> [n_slots, n_out] complex64"""
    f32 = np.float32
    xc = CM.O.pcm_to_cf(np.ascontiguousarray(pcm))
    xr, xi = xc[:, 0].astype(f32), xc[:, 1].astype(f32)
    H = taps(P, Q)
    T, M = H.shape[1], 2 * P
    n_out = n_outputs(len(xr), P, Q)
    k = all_slots(P, Q) if slots is None else np.asarray(slots, np.int64)
    kq = (k * Q) % M
    i_n, q_n = _times(P, Q, 0, n_out)
    na = -(-T // M)
    j = np.arange(na * M, dtype=np.int64)
    hq = np.zeros((n_out, na * M), f32)
    hq[:, :T] = H[q_n]
    wr = _gather(xr, 0, i_n[:, None] - j[None, :]).astype(f32)
    wi = _gather(xi, 0, i_n[:, None] - j[None, :]).astype(f32)
    re, im = np.zeros((n_out, M), f32), np.zeros((n_out, M), f32)
    for a in range(na):
        re = re + hq[:, a * M:(a + 1) * M] * wr[:, a * M:(a + 1) * M]
        im = im + hq[:, a * M:(a + 1) * M] * wi[:, a * M:(a + 1) * M]
    re, im = transform(re, im, M, f32)
    row = rows(M)[(-kq) % M]
    cr, ci = roots(M, f32)
    idx = (kq[:, None] * (i_n % M)[None, :]) % M
    a, b, c, s = re[:, row].T, im[:, row].T, cr[idx], ci[idx]
    return ((a * c - b * s) + 1j * (a * s + b * c)).astype(np.complex64)
