"""float64 model of the wideband front end for a REAL capture (k_channelize.hip behind
ofdmrx_util_channelize_real), and the tolerance the device is held to.

The definition.  Handle rate `rate`, ratio P / Q in lowest terms, 1 <= Q <= 16, 2 <= P / Q <= 32 (Q = 1: the integer decimation D =
P).  Rw = rate P / Q (in double), T = floor(24 P / Q) + 1; the taps h_q[j] (at Q = 1 the taps h of 4.14), the output times
    u_n = n P,  i_n = u_n div Q,  q_n = u_n mod Q
and the increment inc_c = (uint32) llrint(f_c 2^32 / Rw), phi_c(m) = (inc_c m) mod 2^32, are those of channelize_model.py and
rechannelize_model.py: nothing new.  Input: ONE value per wideband position in S16, U8 or F32, scaled as oracle_lib.pcm_to_cf scales
a component (fp32); x is zero at negative indices.  Output
    y_c[n] = 2 sum_{j = 0 .. T - 1} h_{q_n}[j] x[i_n - j] exp(-2 pi i phi_c(i_n - j) / 2^32).
The 2 makes a real cosine of amplitude A an analytic signal of amplitude A.  This model evaluates the REAL sum itself, in float64 on
the fp32 taps and the fp32-scaled input: one real sample times one complex factor per tap.  (That it equals twice the complex models
on the capture (x, 0) is a test, test_channelize_real_model_cpu.py, not the way it is computed.)

The tolerance, per component of an output, derived here and from nothing the device gives:
    tol = 2 x 2^-24 (T + 16) S,   S = sum_j |h_{q_n}[j]| |x[i_n - j]|
The device evaluates 2 exp(-i phi(i_n)) sum_j (h_q[j] exp(+i phi(j))) x[i_n - j] in fp32, j ascending at Q > 1 and in 4.14's order
(b = k mod D ascending, inside it a ascending) at Q = 1.  With u = 2^-24 the derivation is 4.14's and 4.17's, term by term, on the
capture (x, +0) - for which their S, sum |h| (|re| + |im|), is this S:
  * a modulated tap (h cos, h sin): the phase's conversion <= 2^-26 turns < 1.6 u rad, sincospif <= 4 u, the product 1 u: each
    component within 6.6 u |h_q[j]|;
  * the sum: a component is a sum of T products here (2 T there: the products by the zero component are left out, and adding them
    changed no bit), |product| summing to at most S; each of the T fused multiply-adds rounds by at most u |partial sum|, so the sum
    is within T u S by their argument a fortiori (half the roundings);
  * the output rotation: its phasor (<= 5.6 u per component), two products and one addition of values bounded by S.
Together (T + 6.6 + 5.6 + 3) u S < 2^-24 (T + 16) S for the undoubled output; the multiplication by 2 is exact and doubles value and
error alike: 2 x 2^-24 (T + 16) S.  Homogeneous in x: nothing is added for F32 input.

The centres a real capture admits (the library's rule, evaluated in the same IEEE double operations):
    refused:  f not finite,  |f| < rate / 4,  |f| > Rw / 2 - rate / 4     (edge = 0.25 rate, half = 0.5 Rw; |f| > half - edge)
A real capture holds every signal at +f and its conjugate at -f; the channel at f sees the mirror at distance 2 |f| (mod Rw), and the
pass band is flat to rate / 4 on either side, so inside those limits the mirror's pass band lies over the channel's own.

tie: as in the models this one stands beside."""
import numpy as np

from channelize_model import inc_of, phase, turns, worst  # noqa: F401
import rechannelize_model as RM
import oracle_lib as O

CHUNK = 4096

n_taps, n_outputs, wide_rate = RM.n_taps, RM.n_outputs, RM.wide_rate


def to_real(pcm):
    """[W] int16 / uint8 / float32 -> float64 of the fp32 values the decoder's input scaling gives a component"""
    a = np.ascontiguousarray(pcm)
    assert a.ndim == 1, a.shape
    return O.pcm_to_cf(np.ascontiguousarray(np.stack([a, a], axis=1)))[:, 0].astype(np.float64)


def random_real(W, dtype=np.int16, seed=1):
    """full-scale random real input, [W]"""
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.int16:
        return rng.integers(-32767, 32768, size=W).astype(np.int16)
    if np.dtype(dtype) == np.uint8:
        return rng.integers(1, 256, size=W).astype(np.uint8)
    return rng.uniform(-1.0, 1.0, size=W).astype(np.float32)


def with_zero_imag(pcm):
    """the analytic entries' capture (x, +0): [W, 2] of the same dtype (U8: the zero is 128)"""
    a = np.ascontiguousarray(pcm)
    z = np.full_like(a, 128) if a.dtype == np.uint8 else np.zeros_like(a)
    return np.ascontiguousarray(np.stack([a, z], axis=1))


def centre_ok(f_hz, rate, P, Q):
    """the library's rule for a real capture's centre, in its own operations"""
    f = abs(float(f_hz))
    rw, edge = wide_rate(rate, P, Q), 0.25 * float(rate)
    return bool(np.isfinite(f) and not (f > 0.5 * rw or f < edge or f > 0.5 * rw - edge))


def centre_edges(rate, P, Q):
    """(lowest, highest) |f| the rule admits"""
    return 0.25 * float(rate), 0.5 * wide_rate(rate, P, Q) - 0.25 * float(rate)


def _taps_cutoff(P, Q, cutoff):
    """4.17's formula with another cut-off (a wrong variant): [Q, T] float32"""
    T = 24 * P // Q + 1
    j = np.arange(T, dtype=np.int64)
    h = np.zeros((Q, T), np.float64)
    for q in range(Q):
        tn = j * Q + q - 12 * P
        y = tn.astype(np.float64) / float(12 * P)
        v = np.sinc(cutoff * tn.astype(np.float64) / float(P)) * (0.42 + 0.5 * np.cos(np.pi * y) + 0.08 * np.cos(2.0 * np.pi * y))
        h[q] = v / v.sum()
    return h.astype(np.float32)


def channelize(pcm, P, Q, centres_hz, rate=8000, out_first=0, n_out=None, in_first=0, variant=None):
    """-> (v [C, n_out] complex128, tol [C, n_out], tie).  pcm: [W], the wideband positions in_first .. ; variant: one of VARIANTS, a
    deliberately wrong model (tol is always the definition's)"""
    x = to_real(pcm)
    if n_out is None:
        n_out = n_outputs(in_first + len(x), P, Q) - out_first
    rw = wide_rate(rate, P, Q)
    H_true = RM.taps(P, Q).astype(np.float64)
    T = H_true.shape[1]
    H = _taps_cutoff(P, Q, 1.5).astype(np.float64) if variant == "mirror not rejected (cut-off 1.5)" else H_true
    factor = {"no doubling": 1.0, "doubling by sqrt 2": np.sqrt(2.0)}.get(variant, 2.0)
    xv = x
    if variant == "capture read as interleaved pairs":              # position m holds sample 2 (m - in_first)
        xv = np.zeros_like(x)
        xv[:(len(x) + 1) // 2] = x[::2]
    if variant == "imaginary part from the next sample":
        xv = x + 1j * np.concatenate([x[1:], [0.0]])
    centres = np.atleast_1d(np.asarray(centres_hz, np.float64))
    sign = +1.0 if variant == "nco sign" else -1.0
    m = np.arange(len(x), dtype=np.int64) + in_first
    absx = np.abs(x)
    v = np.zeros((len(centres), n_out), np.complex128)
    tol = np.zeros((len(centres), n_out), np.float64)
    tie = np.inf
    xm = []
    for f in centres:
        inc, t = inc_of(-f if variant == "centre negated" else f, 2.0 * rw if variant == "Rw of the analytic pair" else rw)
        tie = min(tie, t)
        xm.append(xv * np.exp(sign * 2j * np.pi * turns(phase(inc, m))))   # a real sample times one complex factor
    jt = np.arange(T, dtype=np.int64)
    for a in range(0, n_out, CHUNK):
        n = np.arange(a, min(a + CHUNK, n_out), dtype=np.int64) + out_first
        u = n * P
        i_n, q_n = u // Q, u % Q
        idx = i_n[:, None] - jt[None, :]
        S = (np.abs(H_true)[q_n] * RM._gather(absx, in_first, idx)).sum(axis=1)
        tol[:, a:a + len(n)] = 2.0 * 2.0 ** -24 * (T + 16) * S
        hq = H[q_n]
        for c in range(len(centres)):
            v[c, a:a + len(n)] = factor * (hq * RM._gather(xm[c], in_first, idx)).sum(axis=1)
    return v, tol, tie


VARIANTS = ("no doubling", "doubling by sqrt 2", "nco sign", "capture read as interleaved pairs", "imaginary part from the next sample",
            "centre negated", "Rw of the analytic pair", "mirror not rejected (cut-off 1.5)")


def channelize_fp32(pcm, P, Q, centres_hz, rate=8000):
    """an fp32 numpy evaluation of the factored form 2 exp(-i phi(i_n)) sum_j (h_q[j] exp(+i phi(j))) x[i_n - j] in the device's order
    - Q = 1: b = k mod D ascending, inside it a = k div D ascending; Q > 1: j ascending - every product and sum rounded to fp32 (no
    fused multiply-add); from position 0 -> [C, n_out] complex64"""
    f32 = np.float32
    x = to_real(pcm).astype(f32)
    H = RM.taps(P, Q)
    T = H.shape[1]
    n_out = n_outputs(len(x), P, Q)
    u = np.arange(n_out, dtype=np.int64) * P
    i_n, q_n = u // Q, u % Q
    w = RM._gather(x, 0, i_n[:, None] - np.arange(T, dtype=np.int64)[None, :]).astype(f32)
    hq = H[q_n]
    order = [a * P + b for b in range(P) for a in range(25 if b == 0 else 24)] if Q == 1 else list(range(T))
    assert sorted(order) == list(range(T))
    out = np.zeros((len(np.atleast_1d(centres_hz)), n_out), np.complex64)

    def phasor(ph):                                                 # fp32 conversion of the phase, then a correctly rounded sincospi
        a = (ph.astype(np.int64).astype(np.uint32).view(np.int32).astype(f32) * f32(2.0 ** -32)).astype(np.float64)
        return np.cos(2 * np.pi * a).astype(f32), np.sin(2 * np.pi * a).astype(f32)

    for c, f in enumerate(np.atleast_1d(centres_hz)):
        inc, _ = inc_of(f, wide_rate(rate, P, Q))
        cs, sn = phasor(phase(inc, np.arange(T, dtype=np.int64)))
        re, im = np.zeros(n_out, f32), np.zeros(n_out, f32)
        for j in order:
            re = re + (hq[:, j] * cs[j]) * w[:, j]
            im = im + (hq[:, j] * sn[j]) * w[:, j]
        cs, sn = phasor(phase(inc, i_n))
        out[c] = f32(2.0) * (re * cs + im * sn) + 1j * (f32(2.0) * (im * cs - re * sn))
    return out
