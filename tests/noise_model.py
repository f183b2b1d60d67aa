"""A float64 model of the build-owned channel models (oracle/channel.c, modem_amd/csrc/k_channel.hip) -- TEST INFRASTRUCTURE.

No GPU and no oracle: numpy only.  Everything after the uniform variates is float64, so the model's own error (about 1e-12 LSB) is
nothing beside the fp32 roundings of the code it judges.  Three users:
  test_noise_model_cpu.py  the definition against its statistics, the oracle against the model, mutants of the model against both;
  test_gpu_channel.py      k_awgn_tile and k_channel against the model and the oracle.

The comparison rule (explain): an int16 sample is explained if it equals rint(v), or differs from it by exactly 1 while the
unrounded model value v lies within the tolerance of the rounding boundary between the two.  Tolerances (derived, not tuned):

  noise   tol = NOISE_REL * S = 2e-6 * S, S = |base| + 32767 * mag, per component.  The angle fl(2pi_f * u2) is off by the product's
          rounding (half an ulp of a number below 8, 2.4e-7) and by 2pi_f - 2pi (1.75e-7), under the loose bound 2pi * 2^-24 * 2 =
          7.5e-7; cos / sin move by as much and the sample by that times 32767 * mag.  sigma (powf, a product, sqrtf), the product
          by -2 (exact), sqrtf, the product by sigma, the product with cos / sin, the division of the base, the sum and the
          quantiser's product are at most nine roundings of 2^-24 = 5.4e-7 of S; logf (halved by the root) and sincosf at <= 2 ulp
          add 1.2e-7 + 2.4e-7.  With the tight angle figure 1.3e-6, with the loose one 1.65e-6: rounded up to 2e-6.  An fp32 numpy
          evaluation differs from this model in 0.03 % (-40 dB) .. 0.2 % (+6 dB) of the samples, all of them explained.

  chain   tol = (4 * ntaps + 8) * 2^-24 * A, A = 32767 * sum|g_t| * max_fr sum_k |sinc * w| (the last factor is 1 without SFO).
          Recount from stage12 of k_channel.hip, per output component, in units of 2^-24 * 32767 * G * W (G = sum|g|, W the
          resampler's factor; a sample of both components at full scale has magnitude sqrt 2, hence the factors of sqrt 2):
            int16 -> float division of both components, carried through the gains          sqrt2 G
            per tap two products and their difference  (|xr gr| + |xi gi| + |diff|)        2 sqrt2 |g_t|   -> 2 sqrt2 G
            accumulation: the first is exact (0 + x), the others round a partial sum       sqrt2 (ntaps - 1) G
            CFO: c and s rounded from double, two products, one sum                        3 sqrt2 G
            the resampler sums in double; its cast to float                                sqrt2 G W
            the quantiser's product 32767 * x                                              sqrt2 G W
          together sqrt2 (ntaps + 7) G W, which (4 ntaps + 8) G W bounds for every ntaps >= 1 (ntaps = 1: 11.4 against 12).  A
          pass-through runs as one tap of gain 1, so ntaps counts as max(ntaps, 1).  The device contracts products and sums into
          FMAs, which only removes roundings from this count.

The cap: in any comparison at most CAP of the samples may differ from rint(v); "explained" cannot hide a broken kernel behind it."""
import math
from collections import namedtuple

import numpy as np

M64 = (1 << 64) - 1
KEY_OFFSET = 0x1234567
NOISE_REL = 2e-6
CAP = 0.01
HALF = 16                    # the resampler's taps are k = -HALF + 1 .. HALF

_U64 = np.uint64


def splitmix64(x):
    """channel.c:14-20 on uint64 arrays (wrapping arithmetic)"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + _U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U64(27))) * _U64(0x94D049BB133111EB)
    return x ^ (x >> _U64(31))


def frame_key(seed, frame, offset=KEY_OFFSET):
    """channel.c:26: splitmix64(seed ^ splitmix64(frame + 0x1234567)), every sum modulo 2^64"""
    inner = int(splitmix64(np.array([(int(frame) + offset) & M64], dtype=np.uint64))[0])
    return int(splitmix64(np.array([(int(seed) & M64) ^ inner], dtype=np.uint64))[0])


def words(n, seed, frame, offset=KEY_OFFSET):
    """the 64-bit word of each of the n samples of a frame"""
    with np.errstate(over="ignore"):
        return splitmix64(_U64(frame_key(seed, frame, offset)) + np.arange(n, dtype=np.uint64))


def field_to_uniform(field):
    """channel.c:29-30: (float)field + 0.5f in fp32 (that rounding is part of the definition: above 2^23 the half is rounded away, to
    even, so u == 1.0 occurs and gives magnitude 0, never a NaN), then the exact scale by 2^-24"""
    f = field.astype(np.float32) + np.float32(0.5)
    return (f * np.float32(1.0 / 16777216.0)).astype(np.float64)


def uniforms(n, seed, frame, u2_shift=8, offset=KEY_OFFSET):
    """u1 from bits 40 .. 63 and u2 from bits 8 .. 31 of the sample's word, as float64 copies of the fp32 values"""
    r = words(n, seed, frame, offset)
    return field_to_uniform(r >> _U64(40)), field_to_uniform((r >> _U64(u2_shift)) & _U64(0xFFFFFF))


def sigma_of(noise_db):
    """api_tx.cpp:10 / channel.c:25 in fp32: sqrtf(0.5f * powf(10.f, noise_db / 10.f)); noise_db is a float argument"""
    db = np.float32(noise_db)
    return float(np.sqrt(np.float32(0.5) * np.power(np.float32(10.0), db / np.float32(10.0), dtype=np.float32), dtype=np.float32))


def gauss(n, seed, frame, **kw):
    """unit-sigma complex Gaussian of a frame, [n, 2] float64, and its magnitude [n]"""
    u1, u2 = uniforms(n, seed, frame, **kw)
    mag = np.sqrt(-2.0 * np.log(u1))
    a = 2.0 * math.pi * u2
    return np.stack([mag * np.cos(a), mag * np.sin(a)], axis=1), mag


def awgn(base_i16, noise_db, seed, first_frame=0, n_base=None, n_out=None, variant=None):
    """out frame f = base[f % n_base] / 32767 + sigma * sqrt(-2 ln u1) * (cos, sin)(2 pi u2), keyed by (seed, first_frame + f).
    base_i16: [n_base, spf, 2] int16.  Returns the unrounded v = 32767 * clip(x, -1, 1) and the scale S = |base| + 32767 * mag,
    both [n_out, spf, 2] float64.  `variant` is for the teeth tests only: a dict that makes the model wrong in one named way."""
    vr = dict(variant or {})
    base = np.asarray(base_i16)
    if base.ndim == 2:
        base = base[None]
    n_base = base.shape[0] if n_base is None else int(n_base)
    n_out = n_base if n_out is None else int(n_out)
    spf = base.shape[1]
    sigma = sigma_of(noise_db) * vr.get("sigma_scale", 1.0)
    v = np.empty((n_out, spf, 2), np.float64)
    S = np.empty((n_out, spf, 2), np.float64)
    for f in range(n_out):
        frame = (0 if vr.get("ignore_first_frame") else int(first_frame)) + f
        g, mag = gauss(spf, seed, frame, u2_shift=vr.get("u2_shift", 8), offset=vr.get("key_offset", KEY_OFFSET))
        if vr.get("swap"):
            g = g[:, ::-1]
        b = base[min(f, n_base - 1) if vr.get("clamp_base") else f % n_base].astype(np.float64)
        x = b / 32767.0 + sigma * g
        v[f] = 32767.0 * np.clip(x, vr.get("clip_lo", -1.0), 1.0)
        S[f] = np.abs(b) + 32767.0 * sigma * mag[:, None]
    return v, S


def resampler_weights(spf, sfo_ppm, k_lo=-HALF + 1):
    """channel.c:51-63: for every output i the window's first input index t0 + k_lo and the 32 weights sinc * Hann, [spf, 32]"""
    step = 1.0 + float(np.float32(sfo_ppm)) * 1e-6
    t = np.arange(spf, dtype=np.float64) * step
    t0 = np.floor(t)
    fr = t - t0
    k = np.arange(k_lo, k_lo + 2 * HALF, dtype=np.float64)
    x = k[None, :] - fr[:, None]
    safe = np.where(np.abs(x) < 1e-12, 1.0, x)
    sinc = np.where(np.abs(x) < 1e-12, 1.0, np.sin(math.pi * safe) / (math.pi * safe))
    w = 0.5 * (1.0 + np.cos(math.pi * x / HALF))
    return t0.astype(np.int64) + k_lo, sinc * w


def chain(pcm, cfo_hz=0.0, sfo_ppm=0.0, taps=(), rate=8000, variant=None):
    """multipath -> CFO -> 32-tap Hann-windowed sinc resampler on one frame [spf, 2] int16, in float64, with the index rules of
    channel.c / k_channel: zeros outside [0, spf), t0 = floor(i * step), taps k = -15 .. 16; cfo_hz, sfo_ppm and the gains are
    the float arguments' values.  Returns v [spf, 2] (unrounded, clipped to +-32767) and the frame's scale A (module docstring)."""
    vr = dict(variant or {})
    pcm = np.asarray(pcm)
    spf = pcm.shape[0]
    x = pcm[:, 0].astype(np.float64) / 32767.0 + 1j * (pcm[:, 1].astype(np.float64) / 32767.0)
    G = 1.0
    if len(taps):
        y = np.zeros(spf, np.complex128)
        G = 0.0
        for d, g in taps:
            g = complex(np.float32(complex(g).real), np.float32(complex(g).imag))
            d = int(d) * vr.get("delay_sign", 1)
            G += abs(g)
            if d >= 0:
                y[d:] += g * x[:spf - d]          # y[m] += g x[m - d]
            else:
                y[:spf + d] += g * x[-d:]
        x = y
    hz = float(np.float32(cfo_hz))
    if hz != 0.0:
        m = np.arange(spf, dtype=np.float64)
        x = x * np.exp(1j * vr.get("cfo_sign", 1) * (2.0 * math.pi * hz * m / float(rate)))
    W = 1.0
    if float(np.float32(sfo_ppm)) != 0.0:
        first, wt = resampler_weights(spf, sfo_ppm, vr.get("k_lo", -HALF + 1))
        idx = first[:, None] + np.arange(2 * HALF)[None, :]
        ok = (idx >= 0) & (idx < spf)
        x = (np.where(ok, x[np.clip(idx, 0, spf - 1)], 0.0) * wt).sum(axis=1)
        W = float(np.abs(wt).sum(axis=1).max())
    v = 32767.0 * np.clip(np.stack([x.real, x.imag], axis=1), -1.0, 1.0)
    return v, 32767.0 * G * W


def chain_tol(ntaps, A):
    return (4 * max(int(ntaps), 1) + 8) * 2.0 ** -24 * A


Explained = namedtuple("Explained", "n equal explained unexplained worst")


def explain(got_i16, v, tol_abs):
    """counts of samples equal to rint(v), explained (1 off, v within tol_abs of the boundary between the two) and unexplained,
    and the largest distance to a boundary among the explained ones as a fraction of its tolerance"""
    got = np.asarray(got_i16).astype(np.float64).ravel()
    v = np.asarray(v, np.float64).ravel()
    tol = np.broadcast_to(np.asarray(tol_abs, np.float64), np.shape(got_i16)).ravel()
    r = np.rint(v)
    d = got - r
    differ = d != 0
    dist = np.abs(v - (r + 0.5 * d))
    ok = differ & (np.abs(d) == 1) & (dist <= tol)
    frac = dist[ok] / np.maximum(tol[ok], 1e-300)
    return Explained(int(v.size), int((~differ).sum()), int(ok.sum()), int((differ & ~ok).sum()), float(frac.max()) if frac.size else 0.0)


def merge(results):
    """pool the counts of several comparisons (small shapes are judged against the cap together)"""
    results = list(results)
    return Explained(sum(r.n for r in results), sum(r.equal for r in results), sum(r.explained for r in results),
                     sum(r.unexplained for r in results), max([r.worst for r in results] or [0.0]))


def share(res):
    return (res.n - res.equal) / max(res.n, 1)


def accept(res):
    """the rule every comparison is held to: nothing unexplained, and the differing share within the cap"""
    return res.unexplained == 0 and (res.n - res.equal) <= CAP * res.n


def lsb_apart(a_i16, b_i16):
    """two int16 results of the same operation: (largest difference, differing share)"""
    d = np.abs(np.asarray(a_i16).astype(np.int32) - np.asarray(b_i16).astype(np.int32))
    return int(d.max()) if d.size else 0, float((d != 0).mean()) if d.size else 0.0


# ---------------------------------------------------------------- shared inputs
def base_frames(n, spf, seed):
    """[n, spf, 2] int16, every frame different: uniform over the whole int16 range, one sample in eight replaced by one of
    0, +-32767 and -32768 (both clips occur at every noise level, and -32768 has to leave as -32767 or above)"""
    rng = np.random.default_rng([int(seed), int(n), int(spf)])
    b = rng.integers(-32768, 32768, size=(n, spf, 2), dtype=np.int64).astype(np.int16)
    special = np.array([0, 32767, -32767, -32768], np.int16)
    pick = rng.random((n, spf, 2)) < 0.125
    b[pick] = special[rng.integers(0, 4, size=int(pick.sum()))]
    return b


def channel_cases(spf, rate=8000):
    """the parameter table of the chain comparisons (CPU against the oracle, GPU against both), delays fitted to spf: name -> keyword arguments"""
    last = spf - 1
    d = lambda x: min(int(x), last)
    three = [(0, 1 + 0j), (d(7), 0.3 - 0.2j), (d(19), -0.1 + 0.15j)]          # test_device_channel_chain_matches_oracle_models
    # Every other gain is a * e^{j phi} with phi in radians, off the decimal lattice: an int16 input through g = 0.7 - 0.4j gives
    # v = 0.7 a + 0.4 b, ON a half-integer for one sample in ten, where fp32 and float64 round apart by right and the cap means nothing.
    pol = lambda a, phi: complex(a * math.cos(phi), a * math.sin(phi))
    eight = [(0, pol(0.51, 0.2)), (0, pol(0.36, 2.1)), (d(1), pol(0.25, 1.5)), (d(3), pol(0.18, -2.6)), (spf // 2, pol(0.2, 0.05)),
             (spf // 2, pol(0.11, 2.7)), (last, pol(0.42, -0.8)), (d(7), pol(0.054, 0.4))]
    return {
        "pass-through": dict(),
        "one tap, delay 0": dict(taps=[(0, pol(0.81, -0.52))]),
        "one tap, delay spf-1": dict(taps=[(last, pol(0.78, 2.45))]),
        "eight taps": dict(taps=eight),
        "cfo +234.567": dict(cfo_hz=234.567),
        "cfo -234.567": dict(cfo_hz=-234.567),
        "cfo 0.001": dict(cfo_hz=0.001),
        "cfo rate/2": dict(cfo_hz=rate / 2.0),
        "sfo +147": dict(sfo_ppm=147.0),
        "sfo -147": dict(sfo_ppm=-147.0),
        "sfo +1000": dict(sfo_ppm=1000.0),
        "sfo -1000": dict(sfo_ppm=-1000.0),
        "sfo +0.001": dict(sfo_ppm=0.001),
        "full chain": dict(cfo_hz=-100.25, sfo_ppm=-80.0, taps=three),
        "saturating": dict(taps=[(0, 1 + 0j), (d(1), 0.6j)], full_scale=True),
    }


def channel_input(n, spf, seed, full_scale=False):
    """[n, spf, 2] int16 frames for the chain: base_frames, or +-full scale (with some -32768) so that a gain sum of 1.6 saturates"""
    if not full_scale:
        return base_frames(n, spf, seed)
    rng = np.random.default_rng([int(seed), 77, int(n), int(spf)])
    return np.array([32767, -32767, -32768, 32767], np.int16)[rng.integers(0, 4, size=(n, spf, 2))]
