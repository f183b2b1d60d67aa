"""float64 model of the wideband synthesizer (k_synthesize.hip behind ofdmrx_util_synthesize), and the
tolerance the device is held to.

The definition.  Handle rate `rate`, interpolation D (2 .. 32), wideband rate Rw = D rate, K = 12 D, T = 24 D + 1, h[k] the fp32
taps of the wideband front end (channelize_model.taps: there is no new filter).  Channel c = 0 .. C - 1:
    input   x_c[j], j = 0 .. n_in - 1, interleaved I/Q in S16 or F32, scaled as oracle_lib.pcm_to_cf scales it (fp32); zero outside
    centre  inc_c = (uint32) llrint(f_c 2^32 / Rw); the phase at ABSOLUTE wideband index m is phi_c(m) = (inc_c m) mod 2^32
    start   start_c >= 0 in wideband samples, any residue mod D
    gain    G_c = D gain_c, formed in double, rounded once to fp32
and at absolute wideband index m
    u_c[m] = sum_j h[m - start_c - j D] x_c[j]           over the j with 0 <= m - start_c - j D <= T - 1 (24 or 25 terms)
    w[m]   = sum_c G_c exp(+2 pi i phi_c(m) / 2^32) u_c[m]
F32 output: (re, im) of w[m], a zero always as +0 (a product that underflows to -0 does not show).  S16 output: quantise() of the F32 output, nearbyintf(32767 clamp(v, -1, 1)) in fp32.
The model evaluates this in float64 on the fp32 taps, the fp32-scaled input and the fp32 G_c.

The order the device keeps (a function of (c, m) alone).  With r = m - start_c, q = floor(r / D), b = r - q D:
    u_c: one chain of fused multiply-adds per component from +0 over a = 0 .. 23 (and a = 24 where b = 0): + h[b + a D] x_c[q - a];
    (cs, sn) = sincospif of phi_c(m) as a signed fraction of a turn, converted in fp32; gr = G_c cs, gi = G_c sn;
    w: one chain per component from +0 over c ascending: re: + gr u.re, - gi u.im;  im: + gr u.im, + gi u.re.

The tolerance, per component of an output, derived here and from nothing the device gives.  With u = 2^-24 (half an ulp, relative)
and S_c[m] = sum_j |h[m - start_c - j D]| (|re| + |im|)(x_c[j]):
    tol[m] = 2^-24 sum_c (25 + 8 + 2 rank_c[m]) |G_c| S_c[m]
  * the tap sums: a component of u_c is a chain of at most 25 fused multiply-adds, each rounding at most u |partial sum| <= u S_c:
    within 25 u S_c.  It enters the output times |G_c cs| or |G_c sn| <= |G_c|, both components together: 25 u |G_c| S_c;
  * the phasor: the phase's conversion to a signed fraction of a turn in fp32 is off by <= 2^-26 turns = 2 pi 2^-26 rad < 1.6 u,
    sincospif <= 2 ulp = 4 u, the product with G_c 1 u |G_c|: gr and gi each within 6.6 u |G_c|, and they multiply |u.re| + |u.im|
    <= S_c: 6.6 u |G_c| S_c;
  * the chain over c: a component takes two fused multiply-adds per channel, each rounding at most u |partial sum|, and the partial
    sum after channel c is at most sum_{c' <= c} |G_c'| S_c'.  A channel that is zero at m adds +0 and rounds nothing.  So |G_c|
    S_c is counted 2 u times for itself and every later channel that is not zero at m: 2 rank_c[m] u |G_c| S_c, rank_c[m] = the
    number of channels c' >= c with S_c'[m] > 0;
  * second-order terms (roundings of roundings) are below 1e-5 of the above.
Together: (25 + 6.6 + 2 rank_c) u |G_c| S_c < 2^-24 (25 + 8 + 2 rank_c) |G_c| S_c.  The rule is homogeneous in x: for F32 input
nothing is added.  Where no channel reaches m the tolerance is 0 and the output is exactly zero.

tie: the smallest distance of any f_c 2^32 / Rw from a half-integer, as in channelize_model: above 1e-6 the device's llrint and the
model's cannot round apart."""
import numpy as np

import channelize_model as CM
import oracle_lib as O

TERMS, CONST = 25, 8


def tile(D):
    """the kernel's tile of outputs, 256 / D groups of D threads with 5 outputs each (the tests put windows at its edges)"""
    return (256 // D) * D * 5


def to_cf(x, s16_scale=32767.0):
    """[n, 2] int16 / float32 -> complex128 of the fp32 values the decoder's input scaling gives"""
    x = np.ascontiguousarray(x)
    if x.dtype == np.int16 and s16_scale != 32767.0:                # (a wrong variant)
        f = (x.astype(np.float32) / np.float32(s16_scale)).astype(np.float64)
    else:
        f = O.pcm_to_cf(x).astype(np.float64)
    return f[:, 0] + 1j * f[:, 1]


def gain32(D, gain):
    """G = D gain in double, rounded once to fp32"""
    with np.errstate(over="ignore"):
        return np.float32(np.float64(D) * np.float64(np.float32(gain)))


def support(start, n_in, D):
    """the last wideband index a channel reaches"""
    return int(start) + (int(n_in) - 1) * D + 24 * D


def n_outputs(starts, n_in, D):
    """the length of a capture that holds every channel's support"""
    return max(support(s, n_in, D) for s in starts) + 1


def _stuffed(a, start, D, lo, hi):
    """a[j] at wideband index start + j D, zeros elsewhere -> the indices lo .. hi"""
    z = np.zeros(hi - lo + 1, a.dtype)
    j0 = max(0, -((start - lo) // D))                               # the first j with start + j D >= lo
    j1 = min(len(a) - 1, (hi - start) // D)
    if j1 >= j0:
        z[start + j0 * D - lo:start + j1 * D - lo + 1:D] = a[j0:j1 + 1]
    return z


def _check(x, D, centres, starts, gains, rate, out_first, n_out):
    if not 2 <= int(D) <= 32:
        raise ValueError("interp must be 2 .. 32")
    if x.ndim != 3 or x.shape[2] != 2 or x.shape[0] < 1 or x.shape[1] < 1 or x.dtype not in (np.dtype(np.int16), np.dtype(np.float32)):
        raise ValueError("input must be [C, n_in, 2] of int16 or float32")
    if not (len(centres) == len(starts) == len(gains) == x.shape[0]) or x.shape[0] > 65535:
        raise ValueError("one centre, start and gain per channel, at most 65535 channels")
    rw = float(D) * float(rate)
    if not all(np.isfinite(f) and abs(f) <= 0.5 * rw for f in centres):
        raise ValueError("a centre is not finite or lies outside +- Rw / 2")
    if not all(0 <= int(s) <= 1 << 50 for s in starts) or not 0 <= int(out_first) <= 1 << 50:
        raise ValueError("a start or out_first is negative or above 2^50")
    if not all(np.isfinite(np.float32(g)) and np.isfinite(gain32(D, g)) for g in gains):
        raise ValueError("a gain is not finite")
    if n_out is not None and n_out < 1:
        raise ValueError("n_out must be positive")


def synthesize(x, D, centres_hz, starts, gains, rate=8000, out_first=0, n_out=None, variant=None):
    """x: [C, n_in, 2] int16 or float32 -> (v [n_out] complex128, tol [n_out], tie).  variant: one of VARIANTS, a deliberately wrong
    model (its tol is the definition's)"""
    x = np.ascontiguousarray(x)
    centres = [float(f) for f in np.atleast_1d(np.asarray(centres_hz, np.float64))]
    starts = [int(s) for s in np.atleast_1d(starts)]
    gains = [float(g) for g in np.atleast_1d(np.asarray(gains, np.float64))]
    _check(x, D, centres, starts, gains, rate, out_first, n_out)
    Cn, n_in = x.shape[0], x.shape[1]
    rw = float(D) * float(rate)
    if n_out is None:
        n_out = n_outputs(starts, n_in, D) - out_first
    kw = {}
    if variant == "hamming":
        kw["window"] = "hamming"
    if variant == "K = 8 D":
        kw["K_per_D"] = 8
    h = CM.taps64(D, **kw).astype(np.float32).astype(np.float64)
    if variant == "tap index off by one":
        h = np.concatenate([h[1:], [0.0]])
    h_true = np.abs(CM.taps(D).astype(np.float64))
    if variant == "centres exchanged":
        centres[0], centres[-1] = centres[-1], centres[0]
    m = np.arange(n_out, dtype=np.int64) + out_first
    v = np.zeros(n_out, np.complex128)
    S = np.zeros((Cn, n_out), np.float64)
    G = np.zeros(Cn, np.float64)
    tie = np.inf
    for c in range(Cn):
        xc = to_cf(x[c], 32768.0 if variant == "s16 / 32768" else 32767.0)
        if variant == "re / im swapped":
            xc = xc.imag + 1j * xc.real
        start = starts[c] + (1 if variant == "start off by one" else 0)
        G[c] = float(np.float32(gains[c])) if variant == "gain without D" else float(gain32(D, gains[c]))
        inc, t = CM.inc_of(centres[c], rw, fp32=variant == "inc in fp32")
        tie = min(tie, t)
        lo, hi = out_first - (len(h) - 1), out_first + n_out - 1
        if starts[c] <= hi and support(starts[c], n_in, D) >= out_first:
            S[c] = np.convolve(_stuffed(np.abs(xc.real) + np.abs(xc.imag), starts[c], D, out_first - 24 * D, hi), h_true, "valid")
        if start > hi or start + (n_in - 1) * D + len(h) - 1 < out_first:
            continue
        u = np.convolve(_stuffed(xc, start, D, lo, hi), h, "valid")
        ang = CM.turns(CM.phase(inc, m - starts[c] if variant == "phase at m - start" else m))
        sign = -1.0 if variant == "nco sign" else +1.0
        v += G[c] * np.exp(sign * 2j * np.pi * ang) * u
    live = S > 0
    rank = np.cumsum(live[::-1], axis=0)[::-1]                      # channels c' >= c that are not zero at m
    tol = 2.0 ** -24 * ((TERMS + CONST + 2 * rank) * np.abs(G)[:, None] * S).sum(axis=0)
    return v, tol, tie


VARIANTS = ("nco sign", "phase at m - start", "gain without D", "start off by one", "tap index off by one", "re / im swapped",
            "centres exchanged", "s16 / 32768", "inc in fp32", "hamming", "K = 8 D")


def synthesize_fp32(x, D, centres_hz, starts, gains, rate=8000, out_first=0, n_out=None):
    """an fp32 numpy evaluation of the definition in the documented order, every product and sum rounded to fp32 (no fused
    multiply-add), the phasor a correctly rounded sincospi of the fp32-converted phase -> [n_out] complex64"""
    f32 = np.float32
    x = np.ascontiguousarray(x)
    Cn, n_in = x.shape[0], x.shape[1]
    starts = [int(s) for s in np.atleast_1d(starts)]
    if n_out is None:
        n_out = n_outputs(starts, n_in, D) - out_first
    h = CM.taps(D)
    T = len(h)
    m = np.arange(n_out, dtype=np.int64) + out_first
    wr, wi = np.zeros(n_out, f32), np.zeros(n_out, f32)
    for c in range(Cn):
        xc = O.pcm_to_cf(x[c])
        xr, xi = xc[:, 0].astype(f32), xc[:, 1].astype(f32)
        r = m - starts[c]
        q, b = r // D, r % D
        ur, ui = np.zeros(n_out, f32), np.zeros(n_out, f32)
        for a in range(25):
            k, j = b + a * D, q - a
            ok = (k <= T - 1) & (j >= 0) & (j < n_in)
            hk = np.where(ok, h[np.minimum(k, T - 1)], f32(0))
            jj = np.clip(j, 0, n_in - 1)
            ur = np.where(ok, ur + hk * xr[jj], ur)
            ui = np.where(ok, ui + hk * xi[jj], ui)
        inc, _ = CM.inc_of(float(np.atleast_1d(centres_hz)[c]), float(D) * float(rate))
        ph = CM.phase(inc, m)
        ang = (ph.astype(np.int64).astype(np.uint32).view(np.int32).astype(f32) * f32(2.0 ** -32)).astype(np.float64)
        cs, sn = np.cos(2 * np.pi * ang).astype(f32), np.sin(2 * np.pi * ang).astype(f32)
        g = gain32(D, np.atleast_1d(gains)[c])
        gr, gi = g * cs, g * sn
        wr = (wr + gr * ur) - gi * ui
        wi = (wi + gr * ui) + gi * ur
    return wr + 1j * wi


def quantise(v):
    """[.., 2] float32 -> int16: the channel kernels' quantiser, nearbyintf(32767.f clamp(v, -1, 1)) in fp32"""
    v = np.asarray(v, np.float32)
    return np.rint(np.float32(32767.0) * np.clip(v, np.float32(-1.0), np.float32(1.0))).astype(np.int16)


def worst(got, v, tol):
    """largest |got - v| / tol over both components; inf where tol is 0 and got is not exactly zero"""
    return CM.worst(got, v, tol)


def random_x(Cn, n_in, dtype=np.int16, seed=1):
    """full-scale random input rows"""
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.int16:
        return rng.integers(-32767, 32768, size=(Cn, n_in, 2)).astype(np.int16)
    return rng.uniform(-1.0, 1.0, size=(Cn, n_in, 2)).astype(np.float32)
