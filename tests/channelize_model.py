"""float64 model of the wideband front end (k_channelize.hip behind ofdmrx_util_channelize), and the
tolerance the device is held to.

The definition.  Handle rate `rate`, decimation D (2 .. 32), wideband rate Rw = D rate.  Input: interleaved I/Q in S16, U8 or F32,
scaled as oracle_lib.pcm_to_cf scales it (fp32).  K = 12 D, T = 2 K + 1,
    h[k] = (0.75 / D) sinc(0.75 (k - K) / D) blackman(k, T),   sinc(t) = sin(pi t) / (pi t),
    blackman(k, T) = 0.42 - 0.5 cos(2 pi k / (T - 1)) + 0.08 cos(4 pi k / (T - 1)),
in double, normalised to sum 1, rounded once to fp32.  Channel c: inc_c = (uint32) llrint(f_c 2^32 / Rw), the phase at absolute
wideband index m is phi_c(m) = (inc_c m) mod 2^32 - integers, exact at any stream length - and
    y_c[n] = sum_{k = 0 .. T - 1} h[k] x[n D - k] exp(-2 pi i phi_c(n D - k) / 2^32),    x zero at negative indices.
W samples give ceil(W / D) outputs.  The model evaluates this sum in float64 on the fp32 taps and the fp32-scaled input.

The tolerance, per component of an output, derived here and from nothing the device gives:
    tol = 2^-24 (T + 16) sum_k |h[k]| (|re| + |im|)(x[n D - k])
The device evaluates exp(-i phi(n D)) sum_k (h[k] exp(+i phi(k))) x[n D - k] in fp32.  With u = 2^-24 (half an ulp, relative):
  * a modulated tap h[k] (cos, sin): the phase's conversion to a signed fraction of a turn in fp32 is off by <= 2^-26 turns = 2 pi
    2^-26 rad < 1.6 u, sincospif <= 2 ulp = 4 u, the product 1 u: each component within 6.6 u |h[k]|;
  * the sum: a component is a sum of 2 T products, |product| summing to at most S = sum_k |h[k]| (|re| + |im|)(x[n D - k]).  Each of
    its 2 T roundings (a product and an addition, or one fused multiply-add) is at most u |partial sum|.  Summed with k ascending the
    partial sums grow with the taps taken so far and the taps are symmetric, so sum_j |p_j| <= T S and the sum is within T u S; that
    is the figure the rule uses.  (For an arbitrary order the worst case is 2 T u S; an fp32 evaluation stays at a few per cent of
    the rule - test_channelize_model_cpu.py holds it to a quarter - because roundings do not all point one way.);
  * the output rotation: its phasor as above (<= 5.6 u per component), two products and one addition of values bounded by S.
Together: (T + 6.6 + 5.6 + 3) u S < 2^-24 (T + 16) S.  For F32 input nothing is added: the bound is
homogeneous in x, so the input's own scale enters through |re| + |im|.

tie: the smallest distance of any f_c 2^32 / Rw from a half-integer: above 1e-6 the device's llrint and the model's cannot round
apart (the quotient is one IEEE double division on both sides)."""
import numpy as np

import oracle_lib as O

TILE = 256


def n_taps(D, K_per_D=12):
    return 2 * K_per_D * D + 1


def taps64(D, K_per_D=12, cutoff=0.75, window="blackman", total=1.0):
    """the taps in double, before the rounding to fp32"""
    K = K_per_D * D
    T = 2 * K + 1
    k = np.arange(T, dtype=np.float64)
    h = (cutoff / D) * np.sinc(cutoff * (k - K) / D)
    if window == "blackman":
        h = h * (0.42 - 0.5 * np.cos(2 * np.pi * k / (T - 1)) + 0.08 * np.cos(4 * np.pi * k / (T - 1)))
    else:                                                           # (a wrong variant: Hamming)
        h = h * (0.54 - 0.46 * np.cos(2 * np.pi * k / (T - 1)))
    return h * (total / h.sum())


def taps(D):
    return taps64(D).astype(np.float32)


def response(h, f_norm):
    """H(f) = sum_k h[k] exp(-2 pi i f k), f in cycles per wideband sample"""
    k = np.arange(len(h), dtype=np.float64)
    return np.exp(-2j * np.pi * np.outer(np.atleast_1d(f_norm), k)) @ np.asarray(h, np.float64)


def inc_of(f_hz, rw, fp32=False):
    """-> (inc as a Python int in [0, 2^32), distance of the quotient from a half-integer)"""
    if fp32:                                                        # (a wrong variant)
        q = float(np.float32(f_hz) * np.float32(4294967296.0) / np.float32(rw))
    else:
        q = float(np.float64(f_hz) * 4294967296.0 / np.float64(rw))
    tie = abs(abs(q - np.floor(q)) - 0.5)
    return int(np.rint(q)) & 0xffffffff, tie


def phase(inc, m):
    """(inc m) mod 2^32 for int64 positions m, exactly"""
    m32 = (np.asarray(m, np.int64) & 0xffffffff).astype(np.uint64)
    return (np.uint64(inc) * m32) & np.uint64(0xffffffff)


def turns(ph):
    """the phase as a signed fraction of a turn in [-1/2, 1/2), exactly (float64 holds 32 bits)"""
    return ph.astype(np.int64).astype(np.uint32).view(np.int32).astype(np.float64) / 4294967296.0


def to_cf(pcm):
    """[W, 2] int16 / uint8 / float32 -> complex128 of the fp32 values the decoder's input scaling gives"""
    f = O.pcm_to_cf(np.ascontiguousarray(pcm)).astype(np.float64)
    return f[:, 0] + 1j * f[:, 1]


def _windows(a, first, D, n_out, T, out_first):
    """a holds positions first .. first + len(a) - 1, zeros elsewhere -> [n_out, T] rows a[n D - T + 1 .. n D], n = out_first .."""
    lo = out_first * D - (T - 1)
    hi = (out_first + n_out - 1) * D
    buf = np.zeros(hi - lo + 1, a.dtype)
    s, e = max(lo, first), min(hi, first + len(a) - 1)
    if e >= s:
        buf[s - lo:e - lo + 1] = a[s - first:e - first + 1]
    return np.lib.stride_tricks.sliding_window_view(buf, T)[::D], lo


def n_outputs(W, D):
    return -(-W // D)


def channelize(pcm, D, centres_hz, rate=8000, out_first=0, n_out=None, in_first=0, variant=None):
    """-> (v [C, n_out] complex128, tol [C, n_out], tie).  pcm: the wideband positions in_first .. ; variant: one of VARIANTS, a
    deliberately wrong model"""
    x = to_cf(pcm)
    rw = float(D) * float(rate)
    if n_out is None:
        n_out = n_outputs(in_first + len(x), D) - out_first
    kw = {}
    if variant == "taps sum to D":
        kw["total"] = float(D)
    if variant == "hamming":
        kw["window"] = "hamming"
    if variant == "cutoff 0.5":
        kw["cutoff"] = 0.5
    if variant == "K = 8 D":
        kw["K_per_D"] = 8
    h = taps64(D, **kw).astype(np.float32).astype(np.float64)
    T = len(h)
    if variant == "centre tap":
        h[T // 2] *= 1.0 + 2.0 ** -10
    h_true = taps(D).astype(np.float64)
    centres = list(np.atleast_1d(np.asarray(centres_hz, np.float64)))
    if variant == "centres exchanged":
        centres[0], centres[-1] = centres[-1], centres[0]
    if variant == "re / im swapped":
        x = x.imag + 1j * x.real
    shift = 1 if variant == "output at n D + 1" else 0
    v = np.zeros((len(centres), n_out), np.complex128)
    tol = np.zeros((len(centres), n_out), np.float64)
    tie = np.inf
    absx, _ = _windows(np.abs(x.real) + np.abs(x.imag), in_first, D, n_out, len(h_true), out_first)
    bound = 2.0 ** -24 * (len(h_true) + 16) * (absx @ np.abs(h_true)[::-1])
    for c, f in enumerate(centres):
        inc, t = inc_of(f, rw, fp32=variant == "inc in fp32")
        tie = min(tie, t)
        m = np.arange(len(x), dtype=np.int64) + in_first
        ang = turns(phase(inc, m))
        sign = +1.0 if variant == "nco sign" else -1.0
        xm = x * np.exp(sign * 2j * np.pi * ang)
        win, _ = _windows(xm, in_first - shift, D, n_out, T, out_first)
        y = win @ h[::-1]
        if variant == "phase at n":                                 # the factored form's rotation taken at n instead of n D
            n = np.arange(n_out, dtype=np.int64) + out_first
            y = y * np.exp(2j * np.pi * (turns(phase(inc, n * D)) - turns(phase(inc, n))))
        v[c] = y
        tol[c] = bound
    return v, tol, tie


VARIANTS = ("nco sign", "phase at n", "output at n D + 1", "inc in fp32", "taps sum to D", "hamming", "cutoff 0.5", "K = 8 D",
            "re / im swapped", "centres exchanged", "centre tap")


def channelize_fp32(pcm, D, centres_hz, rate=8000):
    """an fp32 numpy evaluation of the factored form exp(-i phi(n D)) sum_k (h[k] exp(+i phi(k))) x[n D - k], k ascending, every
    product and sum rounded to fp32 (no fused multiply-add); from position 0 -> [C, ceil(W / D)] complex64"""
    f32 = np.float32
    xc = O.pcm_to_cf(np.ascontiguousarray(pcm))
    xr, xi = xc[:, 0].astype(f32), xc[:, 1].astype(f32)
    h = taps(D)
    T = len(h)
    n_out = n_outputs(len(xr), D)
    wr, _ = _windows(xr, 0, D, n_out, T, 0)
    wi, _ = _windows(xi, 0, D, n_out, T, 0)
    out = np.zeros((len(np.atleast_1d(centres_hz)), n_out), np.complex64)

    def phasor(ph):                                                 # fp32 conversion of the phase, then a correctly rounded sincospi
        a = (ph.astype(np.int64).astype(np.uint32).view(np.int32).astype(f32) * f32(2.0 ** -32)).astype(np.float64)
        return np.cos(2 * np.pi * a).astype(f32), np.sin(2 * np.pi * a).astype(f32)

    for c, f in enumerate(np.atleast_1d(centres_hz)):
        inc, _ = inc_of(f, float(D) * float(rate))
        cs, sn = phasor(phase(inc, np.arange(T, dtype=np.int64)))
        gr, gi = h * cs, h * sn
        re, im = np.zeros(n_out, f32), np.zeros(n_out, f32)
        for k in range(T):                                          # x[n D - k] is column T - 1 - k of the window
            a, b = wr[:, T - 1 - k], wi[:, T - 1 - k]
            re = (re + gr[k] * a) - gi[k] * b
            im = (im + gr[k] * b) + gi[k] * a
        cs, sn = phasor(phase(inc, np.arange(n_out, dtype=np.int64) * D))
        out[c] = (re * cs + im * sn) + 1j * (im * cs - re * sn)
    return out


def worst(got, v, tol):
    """largest |got - v| / tol over both components (got complex or [.., 2] floats)"""
    got = np.asarray(got)
    if not np.iscomplexobj(got):
        got = got[..., 0].astype(np.float64) + 1j * got[..., 1].astype(np.float64)
    d = np.maximum(np.abs(got.real - v.real), np.abs(got.imag - v.imag))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, d / np.where(tol > 0, tol, 1.0), np.where(d > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def random_pcm(W, dtype=np.int16, seed=1):
    """full-scale random input"""
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.int16:
        return rng.integers(-32767, 32768, size=(W, 2)).astype(np.int16)
    if np.dtype(dtype) == np.uint8:
        return rng.integers(1, 256, size=(W, 2)).astype(np.uint8)
    return rng.uniform(-1.0, 1.0, size=(W, 2)).astype(np.float32)
