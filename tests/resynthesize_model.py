"""float64 model of the wideband synthesizer at a rational interpolation (k_resynthesize.hip behind
ofdmrx_util_synthesize_ratio), and the tolerance the device is held to.

The definition.  Handle rate `rate`, ratio P / Q in lowest terms (the entries reduce by the gcd themselves), 1 <= Q <= 16,
2 <= P / Q <= 32.  D = P / Q and K = 12 D are real, Rw = rate P / Q (in double).  H[q][j] is the fp32 table [Q][T], T = floor(24 P /
Q) + 1, of the ratio front end (rechannelize_model.taps: there is no new filter), read as ONE sequence on the grid of 1 / Q wideband
samples:
    G[tn] = H[tn mod Q][tn div Q],  tn = 0 .. 24 P          (g((tn - 12 P) / Q) of 4.17, each phase's normalisation kept)
Channel c = 0 .. C - 1:
    input   x_c[j], j = 0 .. n_in - 1, interleaved I/Q in S16 or F32, scaled as oracle_lib.pcm_to_cf scales it (fp32); zero outside
    centre  inc_c = (uint32) llrint(f_c 2^32 / Rw); the phase at ABSOLUTE wideband index m is phi_c(m) = (inc_c m) mod 2^32
    start   start_c >= 0 in wideband samples
    gain    G_c = D gain_c, D = (double)P / (double)Q, formed in double, rounded once to fp32
and at absolute wideband index m, with r = m - start_c (the channel contributes nothing where r < 0), nu = r Q, q0 = nu div P,
b = nu mod P:
    u_c[m] = sum_a G[b + a P] x_c[q0 - a]                   a = 0 .. 23, and a = 24 where b = 0
    w[m]   = sum_c G_c exp(+2 pi i phi_c(m) / 2^32) u_c[m]
F32 output: (re, im) of w[m], a zero always as +0.  S16 output: quantise() of the F32 output.  A channel's support is
start_c .. start_c + ((n_in - 1 + 24) P) div Q.  The model evaluates this in float64 on the fp32 taps, the fp32-scaled input and
the fp32 G_c.

The order the device keeps (a function of (c, m) alone): u_c is one chain of fused multiply-adds per component from +0 with a
ascending, the 25th term taken only where b = 0; (cs, sn) = sincospif of phi_c(m) as a signed fraction of a turn, converted in fp32;
gr = G_c cs, gi = G_c sn; w is one chain per component from +0 over c ascending: re: + gr u.re, - gi u.im; im: + gr u.im, + gi u.re.

The tolerance, per component of an output, is 4.15's (synthesize_model.py derives it term by term; nothing in the derivation looks at
which taps a chain takes, only at how many there are - at most 25 - and at the sum of the magnitudes of its products):
    tol[m] = 2^-24 sum_c (25 + 8 + 2 rank_c[m]) |G_c| S_c[m]
    S_c[m] = sum_a |G[b + a P]| (|re| + |im|)(x_c[q0 - a]),   rank_c[m] = the number of channels c' >= c with S_c'[m] > 0
25 u S_c for the chain of at most 25 fused multiply-adds, 6.6 u |G_c| S_c for the phasor and its product with the gain, 2 u per
channel at or behind c that is not zero at m for the chain over c.  Nothing the device gives enters it.  Where no channel reaches m
the tolerance is 0 and the output is exactly +0.

tie: the smallest distance of any f_c 2^32 / Rw from a half-integer, as in 4.17: above 1e-6 the device's llrint and the model's
cannot round apart."""
import math

import numpy as np

import channelize_model as CM
import oracle_lib as O
import rechannelize_model as RM
import synthesize_model as SM

TERMS, CONST = 25, 8
TILE = 1024                                                         # the kernel's tile of outputs (the tests put windows at its edges)
CHUNK = 1 << 15                                                     # outputs the model forms at a time

quantise = SM.quantise
worst = SM.worst
random_x = SM.random_x
to_cf = SM.to_cf


def reduce(P, Q):
    P, Q = int(P), int(Q)
    if P <= 0 or Q <= 0:
        raise ValueError("p and q must be positive")
    g = math.gcd(P, Q)
    P, Q = P // g, Q // g
    if Q > 16 or P < 2 * Q or P > 32 * Q:
        raise ValueError("the reduced q must be 1 .. 16 and p / q 2 .. 32")
    return P, Q


def sequence(P, Q, H=None):
    """G[tn], tn = 0 .. 24 P, float64 of the fp32 taps"""
    H = RM.taps(P, Q) if H is None else H
    tn = np.arange(24 * P + 1)
    return np.asarray(H, np.float64)[tn % Q, tn // Q]


def gain32(P, Q, gain):
    """G = D gain in double, D = P / Q in double, rounded once to fp32"""
    with np.errstate(over="ignore"):
        return np.float32((np.float64(P) / np.float64(Q)) * np.float64(np.float32(gain)))


def reach(n_in, P, Q):
    return ((int(n_in) - 1 + 24) * P) // Q


def support(start, n_in, P, Q):
    """the last wideband index a channel reaches"""
    return int(start) + reach(n_in, P, Q)


def n_outputs(starts, n_in, P, Q):
    """the length of a capture that holds every channel's support"""
    return max(support(s, n_in, P, Q) for s in starts) + 1


def _check(x, centres, starts, gains, rate, P, Q, out_first, n_out):
    if x.ndim != 3 or x.shape[2] != 2 or x.shape[0] < 1 or x.shape[1] < 1 or x.dtype not in (np.dtype(np.int16), np.dtype(np.float32)):
        raise ValueError("input must be [C, n_in, 2] of int16 or float32")
    if not (len(centres) == len(starts) == len(gains) == x.shape[0]) or x.shape[0] > 65535:
        raise ValueError("one centre, start and gain per channel, at most 65535 channels")
    rw = RM.wide_rate(rate, P, Q)
    if not all(np.isfinite(f) and abs(f) <= 0.5 * rw for f in centres):
        raise ValueError("a centre is not finite or lies outside +- Rw / 2")
    if not all(0 <= int(s) <= 1 << 50 for s in starts) or not 0 <= int(out_first) <= 1 << 50:
        raise ValueError("a start or out_first is negative or above 2^50")
    if not all(np.isfinite(np.float32(g)) and np.isfinite(gain32(P, Q, g)) for g in gains):
        raise ValueError("a gain is not finite")
    if n_out is not None and n_out < 1:
        raise ValueError("n_out must be positive")


def _terms(m, start, Pd, Q, n_in):
    """r, and per (output, a): the tap's place tn on the grid, the input index j, and whether the term is there"""
    r = m - start
    nu = r * Q
    q0, b = nu // Pd, nu % Pd
    a = np.arange(25, dtype=np.int64)
    tn = b[:, None] + a[None, :] * Pd
    j = q0[:, None] - a[None, :]
    return r, q0, tn, j


def synthesize(x, P, Q, centres_hz, starts, gains, rate=8000, out_first=0, n_out=None, variant=None, with_tol=True):
    """x: [C, n_in, 2] int16 or float32 -> (v [n_out] complex128, tol [n_out], tie).  variant: one of VARIANTS, a deliberately wrong
    model (its tol is the definition's); with_tol=False: tol is None (a long capture whose tolerance nobody reads)"""
    x = np.ascontiguousarray(x)
    P, Q = reduce(P, Q)
    centres = [float(f) for f in np.atleast_1d(np.asarray(centres_hz, np.float64))]
    starts = [int(s) for s in np.atleast_1d(starts)]
    gains = [float(g) for g in np.atleast_1d(np.asarray(gains, np.float64))]
    _check(x, centres, starts, gains, rate, P, Q, out_first, n_out)
    Cn, n_in = x.shape[0], x.shape[1]
    if n_out is None:
        n_out = n_outputs(starts, n_in, P, Q) - out_first
    rw = RM.wide_rate(rate, P, Q)
    G_true = sequence(P, Q)
    Pv = P + 1 if variant == "ratio (P + 1) / Q" else P
    Gv = G_true if Pv == P else sequence(Pv, Q, RM.taps64(Pv, Q).astype(np.float32))
    if variant == "integer taps at round(D)":
        Dr = int(round(P / Q))
        hr = CM.taps(Dr).astype(np.float64)
    if variant == "centres exchanged":
        centres[0], centres[-1] = centres[-1], centres[0]
    rw_inc = float(rate) * float(P // Q) if variant == "inc with Rw = rate floor(D)" else rw
    v = np.zeros(n_out, np.complex128)
    S = np.zeros((Cn, n_out), np.float64) if with_tol else None
    Gc = np.zeros(Cn, np.float64)
    tie = np.inf
    for c in range(Cn):
        xt = to_cf(x[c])
        xc = to_cf(x[c], 32768.0) if variant == "s16 / 32768" else xt
        if variant == "re / im swapped":
            xc = xc.imag + 1j * xc.real
        ax = np.abs(xt.real) + np.abs(xt.imag)
        start = starts[c] + (1 if variant == "start off by one" else 0)
        if variant == "gain without D":
            Gc[c] = float(np.float32(gains[c]))
        elif variant == "gain with floor(D)":
            Gc[c] = float(np.float32(np.float64(P // Q) * np.float64(np.float32(gains[c]))))
        else:
            Gc[c] = float(gain32(P, Q, gains[c]))
        inc, _ = CM.inc_of(centres[c], rw_inc)
        tie = min(tie, CM.inc_of(centres[c], rw)[1])
        # the outputs either the definition or the variant can reach
        lo = max(out_first, min(starts[c], start))
        hi = min(out_first + n_out - 1, max(starts[c], start) + ((n_in + 24) * max(P, Pv)) // Q + 1)
        for a0 in range(lo, hi + 1, CHUNK):
            m = np.arange(a0, min(a0 + CHUNK, hi + 1), dtype=np.int64)
            sl = slice(a0 - out_first, a0 - out_first + len(m))
            r, _, tn, j = _terms(m, starts[c], P, Q, n_in)
            ok = (tn <= 24 * P) & (r >= 0)[:, None] & (j >= 0) & (j < n_in)
            if with_tol:
                S[c, sl] = np.where(ok, np.abs(G_true)[np.clip(tn, 0, 24 * P)] * ax[np.clip(j, 0, n_in - 1)], 0.0).sum(axis=1)
            r, q0, tn, j = _terms(m, start, Pv, Q, n_in)
            if variant == "q0 rounded":
                q0 = (2 * r * Q + Pv) // (2 * Pv)
                j = q0[:, None] - np.arange(25, dtype=np.int64)[None, :]
            ok = (tn <= 24 * Pv) & (r >= 0)[:, None] & (j >= 0) & (j < n_in)
            tv = tn
            if variant == "fraction ignored":
                tv = tn - tn % Q
            if variant == "fraction negated":
                tv = tn - tn % Q + (Q - tn % Q) % Q
            if variant == "tap index off by one":
                tv = tn + 1
            if variant == "integer taps at round(D)":
                g = hr[np.clip((tn * Dr) // P, 0, 24 * Dr)]
            else:
                g = np.where(tv <= 24 * Pv, Gv[np.clip(tv, 0, 24 * Pv)], 0.0)
            u = np.where(ok, g * xc[np.clip(j, 0, n_in - 1)], 0.0).sum(axis=1)
            ang = CM.turns(CM.phase(inc, m - starts[c] if variant == "phase at m - start" else m))
            sign = -1.0 if variant == "nco sign" else +1.0
            v[sl] += Gc[c] * np.exp(sign * 2j * np.pi * ang) * u
        if variant in ("gain without D", "gain with floor(D)"):
            Gc[c] = float(gain32(P, Q, gains[c]))                   # (the tolerance is the definition's)
    if not with_tol:
        return v, None, tie
    live = S > 0
    rank = np.cumsum(live[::-1], axis=0)[::-1]                      # channels c' >= c that are not zero at m
    tol = 2.0 ** -24 * ((TERMS + CONST + 2 * rank) * np.abs(Gc)[:, None] * S).sum(axis=0)
    return v, tol, tie


VARIANTS = ("fraction ignored", "fraction negated", "q0 rounded", "start off by one", "tap index off by one", "gain without D",
            "gain with floor(D)", "integer taps at round(D)", "ratio (P + 1) / Q", "inc with Rw = rate floor(D)", "phase at m - start",
            "nco sign", "re / im swapped", "centres exchanged", "s16 / 32768")


def synthesize_fp32(x, P, Q, centres_hz, starts, gains, rate=8000, out_first=0, n_out=None):
    """an fp32 numpy evaluation of the definition in the documented order, every product and sum rounded to fp32 (no fused
    multiply-add), the phasor a correctly rounded sincospi of the fp32-converted phase -> [n_out] complex64"""
    f32 = np.float32
    x = np.ascontiguousarray(x)
    P, Q = reduce(P, Q)
    Cn, n_in = x.shape[0], x.shape[1]
    starts = [int(s) for s in np.atleast_1d(starts)]
    if n_out is None:
        n_out = n_outputs(starts, n_in, P, Q) - out_first
    G = sequence(P, Q).astype(f32)
    m = np.arange(n_out, dtype=np.int64) + out_first
    wr, wi = np.zeros(n_out, f32), np.zeros(n_out, f32)
    for c in range(Cn):
        xc = O.pcm_to_cf(x[c])
        xr, xi = xc[:, 0].astype(f32), xc[:, 1].astype(f32)
        r = m - starts[c]
        nu = r * Q
        q0, b = nu // P, nu % P
        ur, ui = np.zeros(n_out, f32), np.zeros(n_out, f32)
        for a in range(25):
            tn, j = b + a * P, q0 - a
            ok = (tn <= 24 * P) & (r >= 0) & (j >= 0) & (j < n_in)
            g = G[np.minimum(tn, 24 * P)]
            jj = np.clip(j, 0, n_in - 1)
            ur = np.where(ok, ur + g * xr[jj], ur)
            ui = np.where(ok, ui + g * xi[jj], ui)
        inc, _ = CM.inc_of(float(np.atleast_1d(centres_hz)[c]), RM.wide_rate(rate, P, Q))
        ph = CM.phase(inc, m)
        ang = (ph.astype(np.int64).astype(np.uint32).view(np.int32).astype(f32) * f32(2.0 ** -32)).astype(np.float64)
        cs, sn = np.cos(2 * np.pi * ang).astype(f32), np.sin(2 * np.pi * ang).astype(f32)
        g = gain32(P, Q, np.atleast_1d(gains)[c])
        gr, gi = g * cs, g * sn
        wr = (wr + gr * ur) - gi * ui
        wi = (wi + gr * ui) + gi * ur
    return wr + 1j * wi
