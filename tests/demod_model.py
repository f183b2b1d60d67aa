"""A float64 model of the differential demodulator (decode.cc:453-477 with demod_or_erase, decode.cc:227-235, and for one-channel
input next_sample's BlockDC and Hilbert, decode.cc:294-301, 386) -- TEST INFRASTRUCTURE.  It judges the CONS_RAW tap of
oracle/decoder.c and of modem_amd/csrc/k_demod.hip carrier by carrier ("What pins the demodulator").

The model.  Inputs are the samples as the side read them (int16 / u8 / f32 scaled as pcm.hh does, one or two channels), the rate, the
mode, and the sc_start and cfo_rad THAT SIDE reported: one fp32 ulp of cfo_rad turns cons by 1.7e-4 rad per symbol, so each side
is compared with the model fed with its own value.  Symbol j = 0 .. rows (0 = the pilot) is

    t_j[i] = x[body0 + j stride + i] exp(-j cfo_rad (j stride + i)),   body0 = sc_start + 2 stride,   X_j = fft(t_j),

positions outside the recording read as zero, and c[j-1][i] = X_j[k] / X_{j-1}[k] with k = (i - cols / 2) mod symbol_len; a point is
erased (0) when |c|^2 > 4 or X_{j-1}[k] = 0.  (The reference's oscillator starts at the header symbol; that constant phase leaves
the quotient alone.)  One-channel input goes through a float64 front end from position 0 of the recording: the DC blocker of
oracle/dsp.c:171-196 with the fp32 values of a and b, then the Hilbert filter with the fp32 taps of orc_hilbert_coeffs_n, zero
history.  The model's own error: numpy's float64 transforms of at most 7680 points and a phase of at most 4e6 rad formed in
float64, below 1e-9 of a point's magnitude - a hundredth of the unit below.

The rule.  Per point d = |g - c| / u with

    u = 2^-24 ( (||t_j|| + |c| ||t_{j-1}||) / |X_{j-1}[k]| + |c| ):

an fp32 transform's error per bin scales with eps ||t||, and the quotient adds one rounding.  A comparison holds when every point
both sides deliver is within T u.  Where u = 0 (the current symbol silent, or both) the side must deliver exactly 0.  A point that
one side delivers and the other erases is an ERASURE TIE if ||c| - 2| <= T u, and UNEXPLAINED otherwise; ties may be at most
TIE_CAP = 0.1 % of a comparison's points, nothing may be unexplained.

The tolerance is a measurement of the oracle, never of the device.  MEASURED[channels] is the oracle's worst d over cases(),
two-channel and one-channel input apart (the front end adds roundings); test_demod_model_cpu.py re-measures both on every run and
holds them within 25 % of the constants, and profiles/demod_parity.txt records them case by case.  T = 4 x MEASURED, the margin
and the reasoning of tx_model.py's header: a correct fp32 evaluation in another order (a radix-5/7 front split and a 256-point
register transform where the oracle runs one mixed-radix plan, an NCO as a product of phasors where the oracle steps a rotation)
has about the oracle's sigma; the worst of ~1e6 roughly Gaussian errors sits near 5 sigma, and 4 x covers twice the sigma with
room for the tail.

  MEASURED = {2: 4.87, 1: 4.79}     (4.864 in "E 48 kHz mode 13 -12 dB", 4.783 in "F mono 44.1 kHz mode 13 -12 dB, DC")
  T        = {2: 19.48, 1: 19.16}   (profiles/demod_parity.txt; on a clean 8 kHz frame T u is about 2.5e-6 of |c| = 1)

What the rule cannot see, and so no variant below tests: the PCM scale (32768 for 32767: the quotient cancels it), a constant phase
of the oscillator, a gain or phase common to both channels.  What it sees only in noise: a one-sample shift (on a clean frame the
guard interval makes it a cyclic shift, whose phase ramp the quotient cancels; the first guard sample is the previous symbol's own
first sample) and a twiddle error (below): the first is held on a noisy frame, the second on a frame with a carrier wave beside the band.

One regime is outside the unit and in no case: one-channel input that goes SILENT (digital zeros) with symbols still to come.  What
the demodulator then reads is the front end's decaying tail, a near-constant whose Hilbert sum cancels to a thousandth of its
terms; the oracle itself reaches d = 22.8 there.  (A recording that ENDS is not that: positions outside it read as zero.)

The twiddle variant, 1e-6 rad on the last radix-2 stage's twiddle of one output bin, moves that bin by 1e-6 |X[k] - X[k + N/2]| / 2
per symbol, and the quotient cancels the X[k] part.  In noise alone that is at most about 8 units (over every bin of the waterfall
frame the worst d it reaches is 11.6 against T = 19.48; rejected on the most exposed bins from 2e-6 rad, on every bin from 8e-6
rad).  What exposes it at 1e-6 rad is energy half a transform away from the carrier: case "B .. carrier wave" puts a wave 12 dB under
the signal, outside the band, at tone_hz() = the twiddled carrier's frequency minus half the sample rate; the variant then reaches
d = 41.7 on the oracle's output and is rejected, and the same frame is in the device's table.

`variant=` makes the model wrong in one named way (VARIANTS) for the teeth tests; it has no other use."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np
from scipy.signal import lfilter

import oracle_lib as O
import tx_model as TX

MEASURED = {2: 4.87, 1: 4.79}
T = {ch: 4.0 * m for ch, m in MEASURED.items()}
TIE_CAP = 1e-3
EPS = 2.0 ** -24
TWIDDLE_RAD = 1e-6

VARIANTS = ("nco sign", "nco not advanced over the guard", "nco phase as an fp32 product", "cfo_rad one ulp off", "pilot body at sc_start + stride",
            "symbols one sample late", "code_off one carrier off", "negative bins clipped", "previous over current", "rows divided by the pilot",
            "erasure at |c| > 4", "one twiddle 1e-6 rad off")
MONO_VARIANTS = ("no dc blocker", "hilbert delay off by one", "im sign")


def symbol_len(rate):
    return TX.symbol_len(rate)


def stride_of(rate):
    return symbol_len(rate) + symbol_len(rate) // 8


def filter_len(rate):
    return (((21 * rate) // 8000) & ~3) | 1                                            # decode.cc:172


def geometry(mode):
    """cols, rows of a mode (decode.cc:302-374, 453)"""
    m = TX.MODES[mode]
    return m.cols, TX.rows_of(mode)


# ---------------------------------------------------------------- the front end (one channel)
def scaled(pcm):
    """the samples as pcm.hh delivers them (an fp32 quotient), in float64, [n, channels]"""
    pcm = np.asarray(pcm)
    return O.pcm_to_cf(pcm if pcm.ndim == 2 else pcm[:, None]).astype(np.float64)


def front_coefficients(rate):
    """the fp32 values a, b of BlockDC::samples(2 stride) (oracle/dsp.c:171-172) and the fp32 taps of Hilbert<cmplx, filter_len>"""
    s = np.float32(2 * stride_of(rate))
    a = (s - np.float32(1)) / s
    b = (np.float32(1) + a) / np.float32(2)
    fl = filter_len(rate)
    reco, imco = np.zeros(1, np.float32), np.zeros(32, np.float32)
    L = O.lib()
    L.orc_hilbert_coeffs_n.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.orc_hilbert_coeffs_n(fl, O.ptr(reco), O.ptr(imco))
    return float(a), float(b), float(reco[0]), imco[:(fl - 1) // 4].astype(np.float64)


def dc_blocked(x, rate, variant=None):
    a, b, _, _ = front_coefficients(rate)
    if variant == "no dc blocker":
        return np.array(x, np.float64)
    return lfilter([b, -b], [1.0, -a], np.asarray(x, np.float64))                      # y0 = b (x0 - x1) + a y1


def hilbert_kernels(rate):
    """re[i] = sum_m hre[m] dc[i - m], im[i] = sum_m him[m] dc[i - m] (oracle/dsp.c:198-209: the centre tap sits (filter_len - 1) / 2
    samples back, the odd taps 2 k + 1 on either side of it)"""
    _, _, reco, imco = front_coefficients(rate)
    fl = filter_len(rate)
    c = (fl - 1) // 2
    hre, him = np.zeros(fl), np.zeros(fl)
    hre[c] = reco
    for k, v in enumerate(imco):
        him[c + 2 * k + 1] += v
        him[c - (2 * k + 1)] -= v
    return hre, him


def analytic(pcm, rate, variant=None):
    """what the demodulator reads: [n] complex128.  Two channels: (re, im).  One: hilbert(blockdc(x)) from position 0"""
    x = scaled(pcm)
    if x.shape[1] == 2:
        return x[:, 0] + 1j * x[:, 1]
    n = x.shape[0]
    dc = dc_blocked(x[:, 0], rate, variant)
    hre, him = hilbert_kernels(rate)
    if variant == "hilbert delay off by one":
        hre = np.concatenate([[0.0], hre])
    re, im = np.convolve(dc, hre)[:n], np.convolve(dc, him)[:n]
    return re + 1j * (-im if variant == "im sign" else im)


FrontCheck = namedtuple("FrontCheck", "n worst_re worst_im bad")


def front_end_check(pcm, rate):
    """the model's analytic signal against orc_front_end_rate, sample by sample.  The oracle rounds the exact DC-blocked value to
    fp32 once (its recurrence runs in double), then forms re as one fp32 product and im as a sum of N = (filter_len - 1) / 4
    products of a difference, every step rounded: to first order

        |re - re_model| <= 2 eps |re_model|                                 (the rounding of dc, the rounding of the product)
        |im - im_model| <= (N + 2) eps sum_k |co_k| (|dc_k-| + |dc_k+|)      (two dc roundings carried by each term; the difference
                                                                             and the product rounded; N - 1 partial sums, each at
                                                                             most the sum of the terms' magnitudes)

    with eps = 2^-24; the factor 1.01 covers the second order.  Both recurrences run in double, y0 = b (x0 - x1) + a y1: each step
    rounds at most 3 x 2^-53 max|x| and the feedback a = 1 - 1 / (2 stride) sums those to at most 2 stride times as much, on either
    side.  That floor (6e-13 at 48 kHz with an offset of 0.09) matters only where the blocker's output has decayed below 1e-6 under a
    constant offset; it enters both bounds through the taps.  -> worst ratios to the bound, count above"""
    x = scaled(pcm)[:, 0]
    n = x.size
    pcm = np.ascontiguousarray(pcm)
    fmt = {np.dtype(np.int16): O.FMT_S16, np.dtype(np.uint8): O.FMT_U8, np.dtype(np.float32): O.FMT_F32}[pcm.dtype]
    z = np.zeros((n, 2), np.float32)
    L = O.lib()
    L.orc_front_end_rate.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p]
    L.orc_front_end_rate(rate, O.ptr(pcm), fmt, 1, n, O.ptr(z))
    m = analytic(pcm, rate)
    dc = np.abs(dc_blocked(x, rate))
    nim = (filter_len(rate) - 1) // 4
    hre, him = hilbert_kernels(rate)
    floor = 2 * 3 * 2.0 ** -53 * float(np.abs(x).max()) * 2 * stride_of(rate)
    bre = 1.01 * 2 * EPS * np.abs(m.real) + floor * np.abs(hre).sum() + 2.0 ** -126
    bim = 1.01 * (nim + 2) * EPS * np.convolve(dc, np.abs(him))[:n] + floor * np.abs(him).sum() + 2.0 ** -126
    rre, rim = np.abs(z[:, 0] - m.real) / bre, np.abs(z[:, 1] - m.imag) / bim
    return FrontCheck(n, float(rre.max()), float(rim.max()), int((rre > 1).sum() + (rim > 1).sum()))


# ---------------------------------------------------------------- the demodulator
Model = namedtuple("Model", "c raw u zero")       # delivered points, unerased quotients, units, "the model delivers exactly 0": [rows, cols]


def _odd_half(t):
    """W^k O[k] of the radix-2 split X[k] = E[k] + W^k O[k] of each row of t, every k"""
    odd = t.copy()
    odd[:, 0::2] = 0.0
    return np.fft.fft(odd, axis=1)


def demod(z, rate, mode, sc_start, cfo_rad, variant=None, twiddle_rad=TWIDDLE_RAD, twiddle_every_bin=False):
    """z: analytic(); sc_start, cfo_rad: as the side under comparison reported them -> Model"""
    assert variant is None or variant in VARIANTS, variant
    sl, st = symbol_len(rate), stride_of(rate)
    cols, rows = geometry(mode)
    z = np.asarray(z, np.complex128)
    w32 = np.float32(cfo_rad)
    if variant == "cfo_rad one ulp off":
        w32 = np.nextafter(w32, np.float32(np.inf))
    w = float(w32)
    body0 = int(sc_start) + (st if variant == "pilot body at sc_start + stride" else 2 * st)       # decode.cc:456
    if variant == "symbols one sample late":
        body0 += 1
    j, i = np.arange(rows + 1)[:, None], np.arange(sl)[None, :]
    pos = body0 + j * st + i
    inside = (pos >= 0) & (pos < z.size)
    t = np.where(inside, z[np.clip(pos, 0, max(z.size - 1, 0))], 0.0)
    k = j * (sl if variant == "nco not advanced over the guard" else st) + i                       # decode.cc:458-461
    if variant == "nco phase as an fp32 product":
        ph = (w32 * k.astype(np.float32)).astype(np.float64)
    else:
        ph = w * k
    t = t * np.exp((1j if variant == "nco sign" else -1j) * ph)
    X = np.fft.fft(t, axis=1)                                                                      # decode.cc:462, 473
    car = np.arange(cols) - cols // 2                                                              # decode.cc:454
    if variant == "code_off one carrier off":
        car = car + 1
    bins = np.clip(car, 0, sl - 1) if variant == "negative bins clipped" else car % sl            # decode.cc:219-222
    if variant == "one twiddle 1e-6 rad off":                                                      # the last radix-2 stage's twiddle of one output bin
        sel = bins if twiddle_every_bin else bins[twiddled_carrier(mode):][:1]                     # (every bin: each carrier as if its bin alone were off)
        X[:, sel] += (np.exp(1j * twiddle_rad) - 1.0) * _odd_half(t)[:, sel]
    cur, prv = X[1:, bins], X[:-1, bins]
    if variant == "rows divided by the pilot":
        prv = np.broadcast_to(X[:1, bins], cur.shape)
    if variant == "previous over current":
        cur, prv = prv, cur
    tn = np.sqrt((np.abs(t) ** 2).sum(axis=1))
    ap = np.abs(prv)
    live = ap > 0
    raw = np.where(live, cur / np.where(live, prv, 1.0), 0.0)                                      # decode.cc:227-235
    ar = np.abs(raw)
    u = np.where(live, EPS * ((tn[1:, None] + ar * tn[:-1, None]) / np.where(live, ap, 1.0) + ar), 0.0)
    limit = 16.0 if variant == "erasure at |c| > 4" else 4.0
    zero = ~live | (ar * ar > limit) | (raw == 0)
    return Model(np.where(zero, 0.0, raw), raw, u, zero)


Verdict = namedtuple("Verdict", "n worst median worst_abs ties unexplained d")


def judge(got, model, tol):
    """got: a side's CONS_RAW, [rows * cols, 2] float or [rows, cols] complex -> Verdict.  worst / median: d over the points both
    deliver; worst_abs: |g - c| over the same; d: every point's distance (0 where both are zero, inf where unexplained)"""
    g = np.asarray(got)
    if not np.iscomplexobj(g):
        g = g.astype(np.float64).reshape(-1, 2)
        g = g[:, 0] + 1j * g[:, 1]
    g = g.reshape(model.c.shape)
    gz = g == 0
    both = ~gz & ~model.zero
    err = np.abs(g - model.c)
    d = np.zeros(g.shape)
    d[both] = err[both] / model.u[both]
    mismatch = gz != model.zero
    tie = mismatch & (model.u > 0) & (np.abs(np.abs(model.raw) - 2.0) <= tol * model.u)
    bad = (both & (d > tol)) | (mismatch & ~tie)
    d[mismatch & ~tie] = np.inf
    db = d[both]
    return Verdict(g.size, float(db.max()) if db.size else 0.0, float(np.median(db)) if db.size else 0.0,
                   float(err[both].max()) if db.size else 0.0, int(tie.sum()), int(bad.sum()), d)


def accept(v):
    return v.unexplained == 0 and v.ties <= TIE_CAP * v.n


# ---------------------------------------------------------------- the case table (CPU: oracle against model; GPU: device against both)
Case = namedtuple("Case", "name rate mode channels fmt freq_off noise_db cfo_hz sfo_ppm multipath seed dc cut silent tone")
CALL_SIGN = "DEMOD"
TONE_LSB = 3000                                   # (the signal's rms is 8400 LSB per channel, the wave's 2100)
THREE_TAPS = ((0, 1.0 + 0.0j), (7, -0.55 + 0.3j), (19, 0.3 - 0.45j))


def _case(name, rate, mode, channels=2, fmt="s16", edge=None, noise_db=None, cfo_hz=0.0, sfo_ppm=0.0, multipath=None, seed=1, dc=0, cut=0, silent=None, tone_lsb=0):
    ok = TX.permitted_offsets(mode, rate, channels)
    edge = (-1 if mode % 2 == 0 else 0) if edge is None else edge
    tone = (tone_hz(mode, rate, ok[edge]), tone_lsb) if tone_lsb else None
    return Case(name, rate, mode, channels, fmt, ok[edge], noise_db, cfo_hz, sfo_ppm, multipath, seed, dc, cut, silent, tone)


def twiddled_carrier(mode):
    """the carrier whose bin the variant "one twiddle 1e-6 rad off" perturbs: three quarters up the band"""
    cols = geometry(mode)[0]
    return cols // 2 + cols // 4


def tone_hz(mode, rate, freq_off):
    """the frequency half a transform away from twiddled_carrier(mode): what the last radix-2 stage's twiddle of that bin multiplies is
    X[k] - X[k + N/2], so a carrier wave there is what makes an error of that twiddle visible"""
    car = twiddled_carrier(mode) - geometry(mode)[0] // 2
    return freq_off + (car - symbol_len(rate) // 2) * rate / symbol_len(rate)


def list1_level(mode):
    import mode_levels as ML
    return ML.LEVELS[mode]["list1"][0]


@functools.lru_cache(maxsize=None)
def cases():
    """A: every mode at 8 kHz, two channels, at a band edge of encode.cc:389 (even modes the upper, odd modes the lower), clean and at
    the mode's list-1 level.  B: the regimes - a waterfall-level frame with a CFO (5 - 10 % of its points erased), a negative CFO, an
    SFO, three-tap multipath with deep fades, a carrier wave beside the band.  C: u8 and f32.  D: a frame cut off inside a data symbol, one with a data symbol's
    body set to zero, and both at once in u8 and f32.  E: 16 / 44.1 / 48 kHz, a clean and a noisy frame each on the mode with the fewest carriers (13) and on
    the one with the most (10).  F: one channel at all four rates, with and without a DC offset; at 8 kHz also cut off, u8 and f32."""
    out = []
    for mode in range(6, 14):
        out.append(_case("A mode %d clean" % mode, 8000, mode, seed=100 + mode))
        out.append(_case("A mode %d list-1 level" % mode, 8000, mode, noise_db=list1_level(mode), seed=120 + mode))
    out += [_case("B mode 6 waterfall, +33.3 Hz", 8000, 6, noise_db=-10.0, cfo_hz=33.3, seed=201),
            _case("B mode 10 -15 dB, -80 Hz", 8000, 10, noise_db=-15.0, cfo_hz=-80.0, seed=202),
            _case("B mode 8 -17 dB, SFO 60 ppm", 8000, 8, noise_db=-17.0, sfo_ppm=60.0, seed=203),
            _case("B mode 13 -12 dB, three taps", 8000, 13, noise_db=-12.0, multipath=THREE_TAPS, seed=204),
            _case("B mode 6 -21 dB, carrier wave 12 dB under the signal", 8000, 6, noise_db=-21.0, seed=205, tone_lsb=TONE_LSB),
            _case("C mode 7 u8", 8000, 7, fmt="u8", seed=301),
            _case("C mode 11 f32 -21 dB", 8000, 11, fmt="f32", noise_db=-21.0, seed=302),
            _case("D mode 6 -20 dB cut off 16700 early", 8000, 6, noise_db=-20.0, cut=16700, seed=401),
            _case("D mode 9 -17 dB row 17 silent", 8000, 9, noise_db=-17.0, silent=17, seed=402),
            _case("D mode 7 u8 row 9 silent, cut off 16700 early", 8000, 7, fmt="u8", cut=16700, silent=9, seed=403),
            _case("D mode 11 f32 -21 dB row 30 silent, cut off 16700 early", 8000, 11, fmt="f32", noise_db=-21.0, cut=16700, silent=30, seed=404),
            _case("E 16 kHz mode 13 clean", 16000, 13, seed=501),
            _case("E 16 kHz mode 13 -12 dB", 16000, 13, noise_db=-12.0, seed=502),
            _case("E 16 kHz mode 10 clean", 16000, 10, seed=503),
            _case("E 16 kHz mode 10 -15 dB", 16000, 10, noise_db=-15.0, seed=504),
            _case("E 44.1 kHz mode 13 clean", 44100, 13, seed=511),
            _case("E 44.1 kHz mode 13 -12 dB", 44100, 13, noise_db=-12.0, seed=512),
            _case("E 44.1 kHz mode 10 clean", 44100, 10, seed=513),
            _case("E 44.1 kHz mode 10 -15 dB", 44100, 10, noise_db=-15.0, seed=514),
            _case("E 48 kHz mode 13 clean", 48000, 13, seed=521),
            _case("E 48 kHz mode 13 -12 dB", 48000, 13, noise_db=-12.0, seed=522),
            _case("E 48 kHz mode 10 clean", 48000, 10, seed=523),
            _case("E 48 kHz mode 10 -15 dB", 48000, 10, noise_db=-15.0, seed=524),
            _case("F mono 8 kHz mode 6 clean", 8000, 6, channels=1, edge=0, seed=601),
            _case("F mono 8 kHz mode 9 -17 dB, DC", 8000, 9, channels=1, edge=-1, noise_db=-17.0, dc=1500, seed=602),
            _case("F mono 8 kHz mode 6 -20 dB cut off 16700 early", 8000, 6, channels=1, edge=-1, noise_db=-20.0, cut=16700, seed=611),
            _case("F mono 8 kHz mode 8 u8", 8000, 8, channels=1, fmt="u8", edge=0, seed=612),
            _case("F mono 8 kHz mode 12 f32 -17 dB", 8000, 12, channels=1, fmt="f32", edge=-1, noise_db=-17.0, seed=613),
            _case("F mono 16 kHz mode 12 clean, DC", 16000, 12, channels=1, edge=0, dc=-2000, seed=603),
            _case("F mono 16 kHz mode 6 -20 dB", 16000, 6, channels=1, edge=-1, noise_db=-20.0, seed=604),
            _case("F mono 44.1 kHz mode 7 clean", 44100, 7, channels=1, edge=-1, seed=605),
            _case("F mono 44.1 kHz mode 13 -12 dB, DC", 44100, 13, channels=1, edge=0, noise_db=-12.0, dc=900, seed=606),
            _case("F mono 48 kHz mode 11 -15 dB", 48000, 11, channels=1, edge=0, noise_db=-15.0, seed=607),
            _case("F mono 48 kHz mode 10 clean, DC", 48000, 10, channels=1, edge=-1, dc=3000, seed=608)]
    return tuple(out)


def case(name):
    return {c.name: c for c in cases()}[name]


def payload_of(c):
    return O.payload_for(7000 + c.seed)


def body_span(c, row):
    """the samples of data row `row`'s body in a frame the encoder made (one second of silence, the leading pilot block, Schmidl-Cox,
    meta-data and pilot symbols in front)"""
    sl, st = symbol_len(c.rate), stride_of(c.rate)
    lo = c.rate + (4 + row) * st + (st - sl)
    return lo, lo + sl


@functools.lru_cache(maxsize=None)
def frame_of(c):
    """the recording of a case, as both sides read it: [samples, channels] int16 / uint8 / float32"""
    bits = 8 if c.fmt == "u8" else 16
    pcm = O.encode_pcm(payload_of(c), bits=16, channels=2, freq_off=c.freq_off, call_sign=CALL_SIGN, mode=c.mode, rate=c.rate)
    if c.noise_db is not None or c.cfo_hz or c.sfo_ppm or c.multipath or bits == 8:
        pcm = O.impair(pcm, noise_db=c.noise_db, cfo_hz=c.cfo_hz, sfo_ppm=c.sfo_ppm, multipath=list(c.multipath) if c.multipath else None,
                       seed=c.seed, frame=0, bits=bits, rate=c.rate)
    if c.tone:
        hz, lsb = c.tone
        w = lsb * np.exp(2j * np.pi * ((hz * np.arange(pcm.shape[0])) % c.rate) / c.rate)
        pcm = np.clip(pcm + np.rint(np.stack([w.real, w.imag], axis=1)), -32767, 32767).astype(np.int16)
    if c.fmt == "f32":
        pcm = O.pcm_to_cf(pcm)
    if c.silent is not None:
        lo, hi = body_span(c, c.silent)
        pcm = pcm.copy()
        pcm[lo:hi] = 128 if c.fmt == "u8" else 0
    if c.channels == 1:
        pcm = pcm[:, :1]
        if c.dc:
            pcm = np.clip(pcm.astype(np.int32) + c.dc, -32767, 32767).astype(np.int16)
    if c.cut:
        pcm = pcm[:pcm.shape[0] - c.cut]
    pcm = np.ascontiguousarray(pcm)
    pcm.setflags(write=False)
    return pcm


OracleTap = namedtuple("OracleTap", "status sc_start cfo_rad oper_mode cons payload")


def oracle_tap(pcm, rate, skip=0):
    """O.decode(taps=True) -> what the demodulator's comparison needs; cons: [rows * cols, 2] float32 of the decoded mode"""
    out, res, tb = O.decode(pcm, skip=skip, taps=True, rate=rate)
    n = 0
    if res.status in (0, 6):
        cols, rows = geometry(res.oper_mode)
        n = cols * rows
    return OracleTap(int(res.status), int(res.sc_start), np.float32(res.cfo_rad), int(res.oper_mode), tb.cons_raw[:n].copy(), out)


@functools.lru_cache(maxsize=None)
def oracle_of(c):
    return oracle_tap(frame_of(c), c.rate)


@functools.lru_cache(maxsize=None)
def analytic_of(c):
    return analytic(frame_of(c), c.rate)


def oracle_verdict(c):
    """the oracle against the model fed with the oracle's own sc_start and cfo_rad"""
    o = oracle_of(c)
    assert o.status in (0, 6) and o.oper_mode == c.mode, (c.name, o.status, o.oper_mode)
    return judge(o.cons, demod(analytic_of(c), c.rate, c.mode, o.sc_start, o.cfo_rad), T[c.channels])
