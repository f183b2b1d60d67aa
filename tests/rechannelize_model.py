"""float64 model of the wideband front end at a rational decimation (k_rechannelize in k_channelize.hip behind
ofdmrx_util_channelize_ratio), and the tolerance the device is held to.

The definition.  Handle rate `rate`, ratio P / Q in lowest terms, 1 <= Q <= 16, 2 <= P / Q <= 32.  D = P / Q and K = 12 D are real,
Rw = rate P / Q (in double), T = floor(24 P / Q) + 1 taps per phase.  Input: interleaved I/Q in S16, U8 or F32, scaled as
oracle_lib.pcm_to_cf scales it (fp32).
    u_n = n P,  i_n = u_n div Q,  q_n = u_n mod Q:  output n stands at wideband time i_n + q_n / Q - K
    g(t) = sinc(0.75 t / D) (0.42 + 0.5 cos(pi t / K) + 0.08 cos(2 pi t / K)) for |t| <= K, 0 outside,  sinc(t) = sin(pi t) / (pi t)
    h_q[j] = g(j + q / Q - K),  j = 0 .. T - 1,  q = 0 .. Q - 1
in double, each phase normalised to sum 1, rounded once to fp32.  (With the integer tn = j Q + q - 12 P: t = tn / Q, t / D = tn / P,
t / K = tn / (12 P); the library and this model both evaluate the formula from tn.)  For Q = 1 the taps are 4.14's.
Channel c: inc_c = (uint32) llrint(f_c 2^32 / Rw), phi_c(m) = (inc_c m) mod 2^32 at the absolute wideband index m, and
    y_c[n] = sum_{j = 0 .. T - 1} h_{q_n}[j] x[i_n - j] exp(-2 pi i phi_c(i_n - j) / 2^32),    x zero at negative indices.
W samples give ceil(W Q / P) outputs.  The model evaluates this sum in float64 on the fp32 taps and the fp32-scaled input.

The tolerance, per component of an output, derived here and from nothing the device gives:
    tol = 2^-24 (T + 16) sum_j |h_{q_n}[j]| (|re| + |im|)(x[i_n - j])
The device evaluates exp(-i phi(i_n)) sum_j (h_q[j] exp(+i phi(j))) x[i_n - j] in fp32, j ascending.  With u = 2^-24 (half an ulp,
relative) the derivation is 4.14's (channelize_model.py), term by term:
  * a modulated tap h_q[j] (cos, sin): the phase's conversion to a signed fraction of a turn in fp32 is off by <= 2^-26 turns < 1.6 u
    rad, sincospif <= 2 ulp = 4 u, the product 1 u: each component within 6.6 u |h_q[j]|;
  * the sum: a component is a sum of 2 T products whose magnitudes sum to at most S = sum_j |h_q[j]| (|re| + |im|)(x[i_n - j]); each
    of the 2 T fused multiply-adds rounds by at most u |partial sum|.  With j ascending the partial sums grow with the taps taken so
    far, and a phase's taps are a sampling of the symmetric g, so sum_j |p_j| <= T S up to the phase's asymmetry of one sample in
    T: the sum is within T u S, the figure the rule uses (any order: 2 T u S; an fp32 evaluation stays at a few per cent of the
    rule - test_rechannelize_model_cpu.py holds it to a quarter);
  * the output rotation: its phasor as above (<= 5.6 u per component), two products and one addition of values bounded by S.
Together: (T + 6.6 + 5.6 + 3) u S < 2^-24 (T + 16) S.  Homogeneous in x: nothing is added for F32 input.

tie: the smallest distance of any f_c 2^32 / Rw from a half-integer: above 1e-6 the device's llrint and the model's cannot round
apart (Rw and the quotient are the same IEEE double operations on both sides)."""
import numpy as np

from channelize_model import inc_of, phase, turns, to_cf, worst, random_pcm  # noqa: F401
import channelize_model as CM
import oracle_lib as O

CHUNK = 4096                                                        # outputs the model forms at a time


def n_taps(P, Q):
    return 24 * P // Q + 1


def n_outputs(W, P, Q):
    return -(-W * Q // P)


def wide_rate(rate, P, Q):
    return float(rate) * float(P) / float(Q)


def taps64(P, Q, k_num=None, window="continuous", q_shift=0):
    """[Q, T] in double, before the rounding to fp32.  k_num: 12 P in the definition - the half length K is k_num / Q (a wrong
    variant passes another); window "grid": 4.14's window sampled at the integer j (a wrong variant)"""
    if k_num is None:
        k_num = 12 * P
    T = 2 * k_num // Q + 1
    j = np.arange(T, dtype=np.int64)
    h = np.zeros((Q, T), np.float64)
    for q in range(Q):
        tn = j * Q + ((q + q_shift) % Q) - k_num
        x = 0.75 * tn.astype(np.float64) / float(P)
        y = tn.astype(np.float64) / float(k_num)
        if window == "grid":
            w = 0.42 - 0.5 * np.cos(2 * np.pi * j / (T - 1)) + 0.08 * np.cos(4 * np.pi * j / (T - 1))
        else:
            w = 0.42 + 0.5 * np.cos(np.pi * y) + 0.08 * np.cos(2.0 * np.pi * y)
        v = np.where(np.abs(tn) <= k_num, np.sinc(x) * w, 0.0)
        h[q] = v / v.sum()
    return h


def taps(P, Q):
    """[Q, T] float32; Q = 1: the taps of 4.14"""
    if Q == 1:
        return CM.taps(P)[None, :]
    return taps64(P, Q).astype(np.float32)


def response(h, f_norm):
    return CM.response(h, f_norm)


def aligned_response(H, P, Q, f_norm):
    """[Q, F]: every phase's response with its own delay K - q / Q taken out - what remains is (nearly) real and (nearly) the same"""
    f = np.atleast_1d(np.asarray(f_norm, np.float64))
    K = 12.0 * P / Q
    return np.stack([response(H[q], f) * np.exp(2j * np.pi * f * (K - q / float(Q))) for q in range(Q)])


def _gather(a, first, idx):
    """a holds positions first .. first + len(a) - 1, zeros elsewhere -> a at the positions idx"""
    pos = idx - first
    ok = (pos >= 0) & (pos < len(a))
    return np.where(ok, a[np.clip(pos, 0, len(a) - 1)], 0)


def channelize(pcm, P, Q, centres_hz, rate=8000, out_first=0, n_out=None, in_first=0, variant=None):
    """-> (v [C, n_out] complex128, tol [C, n_out], tie).  pcm: the wideband positions in_first .. ; variant: one of VARIANTS, a
    deliberately wrong model (tol is always the definition's)"""
    x = to_cf(pcm)
    if n_out is None:
        n_out = n_outputs(in_first + len(x), P, Q) - out_first
    rw = wide_rate(rate, P, Q)
    H_true = taps(P, Q).astype(np.float64)
    T_true = H_true.shape[1]
    Pv, kw = P, {}
    if variant == "ratio (P + 1) / Q":
        Pv = P + 1
    if variant == "K = 12 ceil(D)":
        kw["k_num"] = 12 * (-(-P // Q)) * Q
    if variant == "window on the integer grid":
        kw["window"] = "grid"
    if variant == "taps of phase q + 1":
        kw["q_shift"] = 1
    H = H_true if (Pv == P and not kw) else taps64(Pv, Q, **kw).astype(np.float32).astype(np.float64)
    T = H.shape[1]
    centres = list(np.atleast_1d(np.asarray(centres_hz, np.float64)))
    if variant == "centres exchanged":
        centres[0], centres[-1] = centres[-1], centres[0]
    if variant == "re / im swapped":
        x = x.imag + 1j * x.real
    if variant == "inc with Rw = rate floor(D)":
        rw_inc = float(rate) * float(P // Q)
    else:
        rw_inc = rw
    incs, tie = [], np.inf
    for f in centres:
        inc, t = inc_of(f, rw_inc)
        incs.append(inc)
        tie = min(tie, t)
    m = np.arange(len(x), dtype=np.int64) + in_first
    sign = +1.0 if variant == "nco sign" else -1.0
    xm = [x * np.exp(sign * 2j * np.pi * turns(phase(inc, m))) for inc in incs]
    absx = np.abs(x.real) + np.abs(x.imag)
    v = np.zeros((len(centres), n_out), np.complex128)
    tol = np.zeros((len(centres), n_out), np.float64)
    jt, jv = np.arange(T_true, dtype=np.int64), np.arange(T, dtype=np.int64)
    for a in range(0, n_out, CHUNK):
        n = np.arange(a, min(a + CHUNK, n_out), dtype=np.int64) + out_first
        u = n * P
        i_t, q_t = u // Q, u % Q
        S = (np.abs(H_true)[q_t] * _gather(absx, in_first, i_t[:, None] - jt[None, :])).sum(axis=1)
        tol[:, a:a + len(n)] = 2.0 ** -24 * (T_true + 16) * S
        uv = n * Pv
        i_n, q_n = uv // Q, uv % Q
        if variant == "fraction ignored":
            q_n = np.zeros_like(q_n)
        if variant == "fraction negated":
            q_n = (Q - q_n) % Q
        if variant == "i_n rounded":
            i_n = (2 * uv + Q) // (2 * Q)
        idx = i_n[:, None] - jv[None, :]
        hq = H[q_n]
        for c, inc in enumerate(incs):
            y = (hq * _gather(xm[c], in_first, idx)).sum(axis=1)
            if variant == "phase at n":                             # the factored form's rotation taken at n instead of i_n
                y = y * np.exp(2j * np.pi * (turns(phase(inc, i_n)) - turns(phase(inc, n))))
            v[c, a:a + len(n)] = y
    return v, tol, tie


VARIANTS = ("fraction ignored", "fraction negated", "i_n rounded", "K = 12 ceil(D)", "window on the integer grid", "taps of phase q + 1",
            "inc with Rw = rate floor(D)", "phase at n", "ratio (P + 1) / Q", "re / im swapped", "centres exchanged", "nco sign")


def channelize_fp32(pcm, P, Q, centres_hz, rate=8000):
    """an fp32 numpy evaluation of the factored form exp(-i phi(i_n)) sum_j (h_q[j] exp(+i phi(j))) x[i_n - j], j ascending - the
    device's order - every product and sum rounded to fp32 (no fused multiply-add); from position 0 -> [C, n_out] complex64"""
    f32 = np.float32
    xc = O.pcm_to_cf(np.ascontiguousarray(pcm))
    xr, xi = xc[:, 0].astype(f32), xc[:, 1].astype(f32)
    H = taps(P, Q)
    T = H.shape[1]
    n_out = n_outputs(len(xr), P, Q)
    u = np.arange(n_out, dtype=np.int64) * P
    i_n, q_n = u // Q, u % Q
    idx = i_n[:, None] - np.arange(T, dtype=np.int64)[None, :]
    wr, wi, hq = _gather(xr, 0, idx).astype(f32), _gather(xi, 0, idx).astype(f32), H[q_n]
    out = np.zeros((len(np.atleast_1d(centres_hz)), n_out), np.complex64)

    def phasor(ph):                                                 # fp32 conversion of the phase, then a correctly rounded sincospi
        a = (ph.astype(np.int64).astype(np.uint32).view(np.int32).astype(f32) * f32(2.0 ** -32)).astype(np.float64)
        return np.cos(2 * np.pi * a).astype(f32), np.sin(2 * np.pi * a).astype(f32)

    for c, f in enumerate(np.atleast_1d(centres_hz)):
        inc, _ = inc_of(f, wide_rate(rate, P, Q))
        cs, sn = phasor(phase(inc, np.arange(T, dtype=np.int64)))
        re, im = np.zeros(n_out, f32), np.zeros(n_out, f32)
        for j in range(T):
            gr, gi = hq[:, j] * cs[j], hq[:, j] * sn[j]
            a, b = wr[:, j], wi[:, j]
            re = (re + gr * a) - gi * b
            im = (im + gr * b) + gi * a
        cs, sn = phasor(phase(inc, i_n))
        out[c] = (re * cs + im * sn) + 1j * (im * cs - re * sn)
    return out
