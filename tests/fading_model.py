"""A float64 model of the Watterson fading channel (k_fading of modem_amd/csrc/k_channel.hip) -- TEST
INFRASTRUCTURE.  numpy only; everything after the uniform variates is float64.  It shares splitmix64, field_to_uniform, explain, merge
and accept with noise_model.py and is held to the same rule: an int16 sample is explained if it equals rint(v) or is 1 off while v
lies within the tolerance of the rounding boundary between the two, and at most CAP of the samples of a comparison may differ at all.

The definition.  key = splitmix64(seed ^ splitmix64(frame + 0x46414445)); for path t and sinusoid k, q = 16 t + k,
w_f = splitmix64(key + 2 q), w_p = splitmix64(key + 2 q + 1); u1, u2 = bits 40..63 and 8..31 of w_f through field_to_uniform;
z = sqrt(-2 ln u1) cos(2 pi u2); f_hz = 0.5 spread_t z; inc = (uint32) rint(f_hz 2^32 / rate); phase0 = w_p >> 32;
G_t[j] = g_t / 4 * sum_k exp(i 2 pi ((phase0 + inc 32 j) mod 2^32) / 2^32) at knot j (sample 32 j); a path of spread 0 has
G_t = g_t; y[m] = sum_t (G_t[j] + (G_t[j + 1] - G_t[j]) r / 32) x[m - d_t], j = m >> 5, r = m & 31, x = int16 / 32767 and zero
before the frame; v = 32767 clip(y, -1, 1).

The tolerance, per sample and component, derived from the kernel's operations and not tuned.  Unit: u = 2^-24, half an ulp of a
number below 1 relative to 1, so that one fp32 rounding of a value of magnitude M is off by at most u M.  a_t = |g_t|,
X_t = |re| + |im| of x[m - d_t].
  One component of S = sum_k exp(i 2 pi theta_k), 16 terms:
    the phase is converted to fp32 as a signed fraction of a turn, |x| <= 1/2, where half an ulp is 2^-26 turns = 2 pi 2^-26 rad
    = 1.58 u; sine and cosine move by as much at most                                                        16 * 1.58 = 25.2
    sincospif is documented at <= 2 ulp on either output (HIP math API), |output| <= 1                      16 * 2    = 32
    the butterfly sum: at level l = 1..4 there are 16 / 2^l sums of magnitude <= 2^l, each off by <= 2^l u   4 * 16    = 64
                                                                                                     together 121.2 u
  One component of the knot gain G = (g / 4) S (the quarter is exact):
    the error of S through the complex product, (|c_re| + |c_im|) <= sqrt 2 a_t / 4                  0.354 * 121.2 = 42.9 a_t
    two products and their difference, each of magnitude <= |G| <= 4 a_t                                     3 * 4     = 12 a_t
  The interpolated gain G[j] + (G[j + 1] - G[j]) r / 32 (r / 32 is exact):
    the knots' errors enter with weights 1 - r/32 and r/32: no more than one knot's
    the difference of two knots, magnitude <= 8 a_t, times r / 32 < 1                                                   8 a_t
    the product and the sum (one rounding if fused; counted as one of magnitude <= 4 a_t and one <= 8 a_t)            12 a_t
                                                                                     a faded path's gain: e_G = 74.9 -> 75 u a_t
  A specular path's gain is g_t exactly (both knots hold g_t, their difference is 0): e_G = 0, and |G| <= a_t.
  The MAC of path t, with P_t = 4 a_t X_t for a faded path and a_t X_t for a specular one, P = sum_t P_t:
    the gain's error times the sample                                                                            e_G X_t
    the division of the int16 sample, carried through the gain                                                   P_t
    two products                                                                                                 P_t
    two additions into the accumulator, each of a partial sum <= P (FMA contraction only removes roundings)      2 P per path
  The quantiser's product 32767 y                                                                                P
  tol = 32767 u (75 sum_faded a_t X_t + (2 ntaps + 3) P).
The bound assumes |S| = 16, four times the root mean square, so that it holds for every draw; what keeps a loose tolerance from
hiding a broken kernel is the cap on the differing share, which no tolerance enters.

llrint's ties: the model also reports the smallest distance of any f_hz 2^32 / rate from a half-integer.  The device's and numpy's
double-precision log, sqrt and cos differ by some 1e-16 relative, 2e-9 absolute at the largest |f_hz 2^32 / rate| of 2e7: test seeds
are chosen so that the distance exceeds 1e-6, and then the two cannot round apart.

An fp32 numpy evaluation of the definition (evaluate_fp32 below: every operation of the kernel rounded to fp32, sine and cosine
correctly rounded) differs from this model in 0.09 % of the samples on the GPU test's short shapes pooled and in 0.07 % .. 0.13 % on
each of its long cases, all of them explained and none further than 0.04 of its tolerance from a boundary
(test_fading_model_cpu.py measures the shares and holds them to CAP / 2 = 0.5 %)."""
import math

import numpy as np

import noise_model as NM

KEY_OFFSET = 0x46414445
SINES, KNOT, MAX_DELAY = 16, 32, 1024
U = 2.0 ** -24
E_GAIN = 75.0
_U64 = np.uint64
M32 = (1 << 32) - 1


def frame_keys(seed, frames, offset=KEY_OFFSET):
    """splitmix64(seed ^ splitmix64(frame + offset)) for an array of frame indices, every sum modulo 2^64"""
    fr = np.array([(int(f) + offset) & NM.M64 for f in np.atleast_1d(frames)], dtype=np.uint64)
    return NM.splitmix64(_U64(int(seed) & NM.M64) ^ NM.splitmix64(fr))


def f32(x):
    return float(np.float32(x))


def sinusoids(seed, frames, spreads, rate, variant=None):
    """(inc, phase0) of every frame, path and sinusoid, uint64 arrays [F, T, 16] holding 32-bit values, and the smallest distance
    of f_hz 2^32 / rate from a half-integer over the faded paths"""
    vr = dict(variant or {})
    keys = frame_keys(seed, frames, vr.get("key_offset", KEY_OFFSET))
    T = len(spreads)
    q = np.arange(T * SINES, dtype=np.uint64).reshape(T, SINES)
    with np.errstate(over="ignore"):
        wf = NM.splitmix64(keys[:, None, None] + _U64(2) * q[None])
        wp = NM.splitmix64(keys[:, None, None] + _U64(2) * q[None] + _U64(1))
    if vr.get("swap_words"):
        wf, wp = wp, wf
    u1 = NM.field_to_uniform(wf >> _U64(40))
    u2 = NM.field_to_uniform((wf >> _U64(vr.get("u2_shift", 8))) & _U64(0xFFFFFF))
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)
    sp = np.array([f32(s) for s in spreads], np.float64)
    f_hz = vr.get("spread_factor", 0.5) * sp[None, :, None] * z
    a = f_hz * 4294967296.0 / float(rate)
    faded = sp != 0.0
    tie = float(np.abs(a[:, faded] - np.floor(a[:, faded]) - 0.5).min()) if faded.any() else 0.5
    inc = (np.rint(a).astype(np.int64) & M32).astype(np.uint64)
    ph0 = wp >> _U64(32)
    return inc, ph0, tie


def knot_gains(seed, frames, gains, spreads, rate, knots, variant=None):
    """G_t at the given knots (sample 32 j each): complex128 [F, T, len(knots)], and the tie distance"""
    vr = dict(variant or {})
    inc, ph0, tie = sinusoids(seed, frames, spreads, rate, vr)
    step = _U64(vr.get("knot", KNOT))
    j = np.asarray(knots, dtype=np.uint64)
    phase = (ph0[..., None] + inc[..., None] * (step * j)[None, None, None, :]) & _U64(M32)      # [F, T, 16, J], exact in uint64
    S = np.exp(2j * math.pi * (phase.astype(np.float64) / 4294967296.0)).sum(axis=2)
    g = np.array([complex(f32(complex(x).real), f32(complex(x).imag)) for x in gains])
    G = g[None, :, None] * vr.get("norm", 0.25) * S
    spec = np.array([f32(s) == 0.0 for s in spreads])
    if not vr.get("specular_faded"):
        G[:, spec, :] = g[None, spec, None]
    return G, tie


def fading(base_i16, paths, seed, first_frame=0, n_in=None, n_out=None, rate=8000, variant=None):
    """out frame f = base[f % n_in] through the realisation of (seed, first_frame + f).  base_i16: [n_in, spf, 2] int16; paths:
    [(delay, complex gain, spread_hz), ...].  Returns the unrounded v and the tolerance, both [n_out, spf, 2] float64, and the tie
    distance.  `variant` is for the teeth tests only: a dict that makes the model wrong in one named way."""
    vr = dict(variant or {})
    base = np.asarray(base_i16)
    if base.ndim == 2:
        base = base[None]
    n_in = base.shape[0] if n_in is None else int(n_in)
    n_out = n_in if n_out is None else int(n_out)
    spf = base.shape[1]
    knot = vr.get("knot", KNOT)
    nk = (spf + knot - 1) // knot + 1
    frames = [int(first_frame) + f for f in range(n_out)]
    delays = [int(p[0]) for p in paths]
    gains = [p[1] for p in paths]
    spreads = [p[2] for p in paths]
    G, tie = knot_gains(seed, frames, gains, spreads, rate, np.arange(nk), vr)                   # [F, T, nk]
    x = base.astype(np.float64) / 32767.0
    xc = (x[..., 0] + 1j * x[..., 1])[np.arange(n_out) % n_in]                                   # [F, spf]
    xa = (np.abs(x[..., 0]) + np.abs(x[..., 1]))[np.arange(n_out) % n_in]
    m = np.arange(spf)
    y = np.zeros((n_out, spf), np.complex128)
    eg = np.zeros((n_out, spf))
    P = np.zeros((n_out, spf))
    for t, d in enumerate(delays):
        mg = np.maximum(m - d, 0) if vr.get("gain_index_delayed") else m
        j, r = mg // knot, (mg % knot) / float(knot)
        Gi = G[:, t, j] + (G[:, t, j + 1] - G[:, t, j]) * r[None, :]
        xd = np.zeros_like(xc)
        xd[:, d:] = xc[:, :spf - d]
        Xd = np.zeros_like(xa)
        Xd[:, d:] = xa[:, :spf - d]
        y += Gi * xd
        a_t = abs(complex(f32(complex(gains[t]).real), f32(complex(gains[t]).imag)))
        if f32(spreads[t]) != 0.0:
            eg += a_t * Xd
            P += 4.0 * a_t * Xd
        else:
            P += a_t * Xd
    v = 32767.0 * np.clip(np.stack([y.real, y.imag], axis=2), -1.0, 1.0)
    tol = 32767.0 * U * (E_GAIN * eg + (2 * len(paths) + 3) * P)
    return v, np.repeat(tol[..., None], 2, axis=2), tie


def evaluate_fp32(base_i16, paths, seed, first_frame=0, n_in=None, n_out=None, rate=8000):
    """the definition evaluated as an honest fp32 kernel would: the kernel's operations in its order, each rounded to fp32 (no fused
    multiply-add), sine and cosine correctly rounded; the frequency draw is the float64 one.  Returns int16 [n_out, spf, 2]."""
    F = np.float32
    base = np.asarray(base_i16)
    n_in = base.shape[0] if n_in is None else int(n_in)
    n_out = n_in if n_out is None else int(n_out)
    spf = base.shape[1]
    nk = (spf + KNOT - 1) // KNOT + 1
    frames = [int(first_frame) + f for f in range(n_out)]
    spreads = [p[2] for p in paths]
    inc, ph0, _ = sinusoids(seed, frames, spreads, rate)
    j = np.arange(nk, dtype=np.uint64)
    phase = (ph0[..., None] + inc[..., None] * (_U64(KNOT) * j)[None, None, None, :]) & _U64(M32)
    turns = phase.astype(np.uint32).view(np.int32).astype(F) * F(2.0 ** -32)                     # signed, |x| <= 1/2
    ang = 2.0 * math.pi * turns.astype(np.float64)
    cs, sn = np.cos(ang).astype(F), np.sin(ang).astype(F)

    def tree(a):                                                                                 # the butterfly's order: k with k ^ 1, ^ 2, ^ 4, ^ 8
        for _ in range(4):
            a = a[:, :, 0::2, :] + a[:, :, 1::2, :]
        return a[:, :, 0, :]
    Sc, Ss = tree(cs), tree(sn)
    x = (base.astype(F) / F(32767.0))[np.arange(n_out) % n_in]
    m = np.arange(spf)
    jj, fr = m >> 5, ((m & 31).astype(F) * F(1.0 / 32.0))[None, :]
    re, im = np.zeros((n_out, spf), F), np.zeros((n_out, spf), F)
    for t, (d, g, s) in enumerate(paths):
        gr, gi = F(complex(g).real), F(complex(g).imag)
        if f32(s) != 0.0:
            cr, ci = F(0.25) * gr, F(0.25) * gi
            Gr, Gq = cr * Sc[:, t] - ci * Ss[:, t], cr * Ss[:, t] + ci * Sc[:, t]
        else:
            Gr, Gq = np.full((n_out, nk), gr, F), np.full((n_out, nk), gi, F)
        a = Gr[:, jj] + (Gr[:, jj + 1] - Gr[:, jj]) * fr
        b = Gq[:, jj] + (Gq[:, jj + 1] - Gq[:, jj]) * fr
        xr, xi = np.zeros((n_out, spf), F), np.zeros((n_out, spf), F)
        xr[:, d:], xi[:, d:] = x[:, :spf - d, 0], x[:, :spf - d, 1]
        live = (m >= d)[None, :]
        re = np.where(live, re + (xr * a - xi * b), re)
        im = np.where(live, im + (xr * b + xi * a), im)
    out = np.stack([np.clip(re, F(-1), F(1)), np.clip(im, F(-1), F(1))], axis=2)
    return np.rint(F(32767.0) * out).astype(np.int16)


# ---------------------------------------------------------------- shared inputs (the GPU test's and the fp32 evaluation's)
SPF_SHORT = (1, 31, 32, 33, 257)
TILE = 4096                                                                                      # samples per workgroup of k_fading
SPF_LONG = (TILE - 1, TILE, TILE + 1, 2 * TILE + 77)
TILINGS = ((1, 1), (1, 5), (3, 7), (5, 2))                                                       # (n_in, n_out)
FIRST = (0, 3, (1 << 32) - 2, 1 << 63)
SEEDS = (0, 1, NM.M64)


def path_sets(spf, rate=8000):
    """name -> [(delay, complex gain, spread_hz), ...], delays fitted to spf.  Gains off the decimal lattice (noise_model.channel_cases)."""
    last = spf - 1
    d = lambda x: min(int(x), last)
    pol = lambda a, phi: complex(a * math.cos(phi), a * math.sin(phi))
    lim = rate / 800.0
    return {
        "one path": [(0, pol(0.81, -0.52), 1.0)],
        "two paths": [(0, pol(0.62, 0.3), 0.5), (d(1), pol(0.55, 2.2), 2.0)],
        "eight paths": [(0, pol(0.31, 0.2), 1.0), (0, pol(0.26, 2.1), 0.1), (d(1), pol(0.25, 1.5), 3.0), (d(3), pol(0.18, -2.6), 0.5),
                        (spf // 2 if spf // 2 <= MAX_DELAY else 517, pol(0.2, 0.05), 2.0), (d(7), pol(0.11, 2.7), lim),
                        (min(last, MAX_DELAY), pol(0.22, -0.8), 1.5), (d(19), pol(0.054, 0.4), 0.25)],
        "specular and faded": [(0, pol(0.55, 0.9), 0.0), (d(2), pol(0.4, -1.1), 1.0), (d(5), pol(0.2, 2.9), 0.0), (d(11), pol(0.3, 0.4), 4.0)],
        "spread limits": [(0, pol(0.6, 1.3), lim), (d(3), pol(0.5, -0.7), 0.001)],
    }


def combos(spf):
    """(tiling, first_frame, seed): the full cross up to 257 samples, a rotation through the lists for the longer shapes"""
    if spf <= 257:
        return [(tl, fi, sd) for tl in TILINGS for fi in FIRST for sd in SEEDS]
    return [(TILINGS[(k + spf) % 4], FIRST[k % 4], SEEDS[k % 3]) for k in range(4)]


def case_list(spf, rate=8000):
    """every (name, paths, tiling, first_frame, seed) of one shape: each path set with every combination (short shapes) or with one
    combination of the rotation, a different one per path set (long shapes)"""
    sets = path_sets(spf, rate)
    cs = combos(spf)
    if spf <= 257:
        return [(name, p) + c for name, p in sets.items() for c in cs]
    return [(name, p) + cs[k % len(cs)] for k, (name, p) in enumerate(sets.items())]


def inputs(n_in, spf):
    return NM.base_frames(n_in, spf, 60 + n_in)
