"""The wideband front end at a rational decimation without a GPU: the library's taps against the formula,
the filter every phase makes and how far the phases of a ratio differ, the float64 model of rechannelize_model.py on tones, the
tolerance rule on an fp32 evaluation in the device's order and on deliberately wrong models, and the argument errors of the new
entries that need no look into the handle.  (ofdmrx_bank_push on a ratio bank and the util calls while a bank is open need a real
handle: test_gpu_rechannelize_bank.py has them.)"""
import ctypes as C
import os

import numpy as np
import pytest

import channelize_model as CM
import rechannelize_model as RM

E_ARG = -1
NAMES = ("ofdmrx_util_channelize_ratio_taps", "ofdmrx_util_channelize_ratio", "ofdmrx_bank_begin_wideband_ratio")
RATIOS = [(5, 2), (33, 16), (31, 15), (25, 4), (64, 3), (125, 4), (511, 16), (32, 1)]
FRACTIONAL = [r for r in RATIOS if r[1] > 1]


@pytest.fixture(scope="module")
def lib():
    import modem_amd
    modem_amd.build()
    return modem_amd.load_library()


def test_symbols_exported_and_declared(lib):
    import modem_amd
    import modem_amd.ofdmrx as M
    text = open(os.path.join(os.path.dirname(M.HERE), "include", "ofdmrx.h")).read()
    for name in NAMES:
        assert name in M.EXPORTS
        getattr(lib, name)
        assert name + "(" in text and name in text.split("#define OFDMRX_ABI_MINOR")[0]
    assert lib.ofdmrx_abi_minor() == 9                               # additions within 1.9: detected by symbol
    assert callable(modem_amd.channelize_ratio_taps)


@pytest.mark.parametrize("P,Q", RATIOS)
def test_taps_match_the_formula(lib, P, Q):
    import modem_amd
    got = modem_amd.channelize_ratio_taps(P, Q)
    T = 24 * P // Q + 1
    assert got.dtype == np.float32 and got.shape == (Q, T)
    want = RM.taps(P, Q)
    off = int((got != want).sum())
    print("%d/%d: T %d, %s" % (P, Q, T, "equal as fp32" if off == 0 else "%d of %d taps off by one ulp (the double sums differ)" % (off, got.size)))
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
    assert (np.abs(got.astype(np.float64).sum(axis=1) - 1.0) <= T * 2.0 ** -24).all()
    if Q == 1:
        assert got[0].tobytes() == modem_amd.channelize_taps(P).tobytes()


def test_taps_reduce_by_the_gcd(lib):
    import modem_amd
    assert modem_amd.channelize_ratio_taps(50, 8).tobytes() == modem_amd.channelize_ratio_taps(25, 4).tobytes()
    assert modem_amd.channelize_ratio_taps(12, 2).tobytes() == modem_amd.channelize_taps(6).tobytes()
    assert modem_amd.channelize_ratio_taps(34 * 7, 17 * 7).tobytes() == modem_amd.channelize_taps(2).tobytes()   # (q = 119 reduces to 1)


def test_taps_refusals(lib):
    import modem_amd
    buf = np.full(16 * 769 + 8, 7.0, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    for bad in ((0, 1), (5, 0), (-5, 2), (5, -2), (35, 17), (3, 2), (1, 1), (65, 2), (33, 1), (513, 16), (1 << 20, 3)):
        assert lib.ofdmrx_util_channelize_ratio_taps(bad[0], bad[1], p) == E_ARG, bad
    assert lib.ofdmrx_util_channelize_ratio_taps(5, 2, None) == E_ARG
    assert (buf == 7.0).all()
    assert lib.ofdmrx_util_channelize_ratio_taps(5, 2, p) == 61 and (buf[122:] == 7.0).all()
    assert lib.ofdmrx_util_channelize_ratio_taps(511, 16, p) == 767 and (buf[16 * 767:] == 7.0).all()
    assert lib.ofdmrx_util_channelize_ratio_taps(4, 2, p) == 49                                   # 2/1: the lowest ratio
    for bad in ((35, 17), (3, 2), (0, 1)):
        with pytest.raises(modem_amd.OfdmRxError):
            modem_amd.channelize_ratio_taps(*bad)


@pytest.mark.parametrize("P,Q", RATIOS)
def test_filter_of_every_phase(lib, P, Q):
    """on the library's own taps, in float64, for every phase: |f| <= rate / 4 within +-0.01 dB, everything from rate / 2 to Rw / 2 at
    most -70 dB (f in cycles per wideband sample: rate / 4 is Q / (4 P)); and, each phase's own delay K - q / Q taken out, the phases
    differ from their mean by at most -100 dB over the pass band - the level of the spur a time-varying filter makes"""
    import modem_amd
    H = modem_amd.channelize_ratio_taps(P, Q).astype(np.float64)
    D = P / float(Q)
    N = 1 << 16
    f = np.arange(N // 2 + 1) / N
    pb_hi, pb_lo, sb = -np.inf, np.inf, -np.inf
    for q in range(Q):
        A = np.abs(np.fft.rfft(H[q], N))
        pb = np.concatenate([A[f <= 0.25 / D], np.abs(RM.response(H[q], [0.25 / D]))])
        st = np.concatenate([A[f >= 0.5 / D], np.abs(RM.response(H[q], [0.5 / D]))])
        pb_hi, pb_lo, sb = max(pb_hi, pb.max()), min(pb_lo, pb.min()), max(sb, st.max())
    fp = np.linspace(-0.25 / D, 0.25 / D, 129)
    R = RM.aligned_response(H, P, Q, fp)
    spread = np.abs(R - R.mean(axis=0)).max()
    pb_hi, pb_lo, sb_db = 20 * np.log10(pb_hi), 20 * np.log10(pb_lo), 20 * np.log10(sb)
    spread_db = 20 * np.log10(max(spread, 1e-300))
    print("%d/%d: passband %+.4f / %+.4f dB, stopband %.1f dB, phases about their mean %.1f dB, sum|h| %.3f .. %.3f"
          % (P, Q, pb_hi, pb_lo, sb_db, spread_db, np.abs(H).sum(axis=1).min(), np.abs(H).sum(axis=1).max()))
    assert pb_hi <= 0.01 and pb_lo >= -0.01, (P, Q, pb_hi, pb_lo)
    assert sb_db <= -70.0, (P, Q, sb_db)
    assert spread_db <= -100.0, (P, Q, spread_db)


TONES = [(P, Q, f_c, d) for P, Q, f_c in ((5, 2, 1000.0), (25, 4, -14000.0), (25, 4, 9000.25), (511, 16, -100000.0))
         for d in (500.0, -1999.0, 3000.0, 3999.0, 5000.0, -9000.0) if abs(f_c + d) <= 4000.0 * P / Q]   # (the tone lies inside the capture)


@pytest.mark.parametrize("P,Q,f_c,delta", TONES)
def test_model_on_a_tone(P, Q, f_c, delta):
    """a tone at f_c + delta comes out as a tone at delta, with the gain of the filter at delta and 12 output samples late: output n
    is A G(delta) exp(2 pi i delta (n - 12) / rate), G the mean of the phases' aligned responses (the phases differ from it by -100
    dB or less in the pass band: 1e-5 A)"""
    rate = 8000
    rw = RM.wide_rate(rate, P, Q)
    A = 0.5
    W = 60 * P // Q + 5
    m = np.arange(W)
    x = A * np.exp(2j * np.pi * (f_c + delta) * m / rw)
    pcm = np.stack([x.real, x.imag], axis=1).astype(np.float32)
    v, tol, tie = RM.channelize(pcm, P, Q, [f_c], rate)
    assert v.shape == (1, RM.n_outputs(W, P, Q)) and tie > 1e-6
    inc, _ = RM.inc_of(f_c, rw)
    f_nco = (inc if inc < 2 ** 31 else inc - 2 ** 32) * rw / 2.0 ** 32   # what the integer increment really mixes by
    d = f_c + delta - f_nco
    H = RM.taps(P, Q).astype(np.float64)
    R = RM.aligned_response(H, P, Q, [d / rw])[:, 0]
    n = np.arange(24, v.shape[1])                                    # past the filter's fill
    # exactly: phase q's own response at its own time i_n + q / Q - K = n D - K
    exact = A * R[(n * P) % Q] * np.exp(2j * np.pi * d * (n - 12) / rate)
    assert np.abs(v[0, 24:] - exact).max() <= 1e-6 * A               # (the fp32 rounding of the input: 6e-8 sum|h|)
    gain = np.abs(v[0, 24:]).mean() / A
    if abs(delta) <= rate / 4:
        want = A * R.mean() * np.exp(2j * np.pi * d * (n - 12) / rate)
        assert np.abs(v[0, 24:] - want).max() <= (1e-5 + 1e-6) * A
        assert abs(R.mean().imag) <= 1e-5 and abs(20 * np.log10(gain)) <= 0.01
    elif abs(delta) >= rate / 2:
        assert gain <= 10 ** (-70 / 20.0) + 1e-6
    else:
        assert abs(gain - np.abs(R).mean()) <= 1e-5 and 1e-4 < gain < 1.0


CENTRES = {(5, 2): [1234.5, -5000.0], (33, 16): [1234.5, -7000.25], (31, 15): [1234.5, 8000.0], (25, 4): [1234.5, -14000.0, 9000.0],
           (64, 3): [1234.5, -80000.3], (125, 4): [1234.5, 100001.3], (511, 16): [1234.5, -2718.28], (32, 1): [1234.5, 100001.3]}


@pytest.fixture(scope="module")
def cases():
    """full-scale random int16 input, the model on it: computed once, read only.  (Long enough for a phase increment that is off,
    or a ratio that is off, to drift.)"""
    out = {}
    for P, Q in FRACTIONAL:
        W = 400 * P // Q + 1 if P // Q < 20 else 40001
        pcm = RM.random_pcm(W, np.int16, seed=P)
        v, tol, tie = RM.channelize(pcm, P, Q, CENTRES[(P, Q)])
        for a in (pcm, v, tol):
            a.setflags(write=False)
        out[(P, Q)] = (pcm, v, tol, tie)
    return out


@pytest.mark.parametrize("P,Q", FRACTIONAL)
def test_fp32_evaluation_stays_under_a_quarter_of_tol(cases, P, Q):
    """the device's order, j ascending, in fp32 numpy"""
    pcm, v, tol, tie = cases[(P, Q)]
    assert tie > 1e-6 and (tol > 0).all()
    w = RM.worst(RM.channelize_fp32(pcm, P, Q, CENTRES[(P, Q)]), v, tol)
    print("%d/%d: fp32 evaluation, worst error / tol %.4f" % (P, Q, w))
    assert w <= 0.25, (P, Q, w)


def test_q_1_is_the_integer_model():
    pcm = RM.random_pcm(2001, np.int16, seed=3)
    a, ta, _ = RM.channelize(pcm, 6, 1, [1234.5, -13000.0])
    b, tb, _ = CM.channelize(pcm, 6, [1234.5, -13000.0])
    assert np.abs(a - b).max() <= 1e-12 and np.allclose(ta, tb, rtol=1e-12, atol=0)


# (at Q = 2 the negated fraction (Q - q) mod Q is q itself - the same model, nothing to see - so that pair is left out)
@pytest.mark.parametrize("P,Q,variant", [(P, Q, v) for v in RM.VARIANTS for (P, Q) in ((5, 2), (25, 4), (511, 16))
                                         if (Q, v) != (2, "fraction negated")])
def test_wrong_variants_are_rejected(cases, P, Q, variant):
    """each wrong model leaves the tolerance somewhere past the filter's fill: the rule tells them from the definition"""
    pcm, v, tol, _ = cases[(P, Q)]
    bad = RM.channelize(pcm, P, Q, CENTRES[(P, Q)], variant=variant, n_out=v.shape[1])[0]
    w = RM.worst(bad[:, 24:], v[:, 24:], tol[:, 24:])               # (past the fill, where a first tap of 1e-17 makes tol next to nothing)
    print("%d/%d %s: worst / tol %.3g" % (P, Q, variant, w))
    assert w > 1.0, (P, Q, variant, w)


@pytest.mark.parametrize("P,Q", [(25, 4), (33, 16)])
def test_model_cuts_into_blocks(cases, P, Q):
    """the model itself: a block with its history gives the outputs of the whole capture, for every residue of the first output"""
    pcm, v, tol, _ = cases[(P, Q)]
    T = 24 * P // Q + 1
    for o0 in range(40, 40 + Q):
        i0 = o0 * P // Q - (T - 1)
        assert i0 > 0
        part, ptol, _ = RM.channelize(pcm[i0:], P, Q, CENTRES[(P, Q)], out_first=o0, in_first=i0)
        assert np.array_equal(part, v[:, o0:]) and np.array_equal(ptol, tol[:, o0:])


def test_channelize_ratio_bad_arguments(lib):
    """every refusal that needs no look into the handle comes before any device call (and before the handle is touched)"""
    fake = C.c_void_p(1)
    f = np.array([1000.0, -2000.0], np.float64)
    pf = f.ctypes.data_as(C.c_void_p)
    din, dout = C.c_void_p(1 << 20), C.c_void_p(1 << 24)

    def call(h=fake, d_in=din, fmt=0, in_first=0, n_in=4096, p=25, q=4, centres=pf, n_ch=2, out_first=0, n_out=100, d_out=dout, stride=100):
        return lib.ofdmrx_util_channelize_ratio(h, d_in, fmt, in_first, n_in, p, q, centres, n_ch, out_first, n_out, d_out, stride)

    for bad in ((0, 4), (25, 0), (-25, 4), (25, -4), (35, 17), (7, 4), (129, 4), (513, 16)):   # bad p / q, Q above 16, ratio out of range
        assert call(p=bad[0], q=bad[1]) == E_ARG, bad
    assert call(p=33, q=1) == E_ARG and call(p=2, q=2) == E_ARG       # reduced q = 1: the integer entry's range
    assert call(h=None) == E_ARG and call(h=None, p=6, q=1) == E_ARG
    assert call(d_in=None) == E_ARG and call(d_out=None) == E_ARG and call(centres=None) == E_ARG
    assert call(n_in=0) == E_ARG and call(n_out=0) == E_ARG
    assert call(n_ch=0) == E_ARG and call(n_ch=65536) == E_ARG
    assert call(fmt=-1) == E_ARG and call(fmt=3) == E_ARG
    assert call(in_first=-1) == E_ARG and call(out_first=-1) == E_ARG
    assert call(stride=99) == E_ARG
    assert call(n_out=657, stride=657) == E_ARG                       # output 656 needs position 656 * 25 div 4 = 4100 of 4096
    assert call(in_first=1, out_first=24) == E_ARG                    # history: 24 * 25 div 4 - 150 = 0 < in_first
    assert call(d_out=C.c_void_p((1 << 20) + 8)) == E_ARG             # the output overlaps the input
    assert call(d_in=C.c_void_p((1 << 20) + 2)) == E_ARG              # off the sample-frame boundary
    assert call(d_out=C.c_void_p((1 << 24) + 4)) == E_ARG             # off 8 bytes
    for bad in (float("nan"), float("inf")):
        g = np.array([1000.0, bad], np.float64)
        assert call(centres=g.ctypes.data_as(C.c_void_p)) == E_ARG


def test_wideband_ratio_bank_bad_arguments(lib):
    """what needs no look into the handle is refused first"""
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(1)
    f = np.array([1000.0, -2000.0], np.float64)
    begin = lib.ofdmrx_bank_begin_wideband_ratio
    assert begin(None, 2, p(f), 25, 4, 0) == E_ARG
    assert begin(fake, 2, None, 25, 4, 0) == E_ARG
    assert begin(fake, 0, p(f), 25, 4, 0) == E_ARG and begin(fake, 65536, p(f), 25, 4, 0) == E_ARG
    for bad in ((0, 4), (25, 0), (-25, 4), (25, -4), (35, 17), (7, 4), (129, 4), (33, 1), (1, 1)):
        assert begin(fake, 2, p(f), bad[0], bad[1], 0) == E_ARG, bad
    assert begin(fake, 2, p(f), 25, 4, -1) == E_ARG and begin(fake, 2, p(f), 25, 4, 3) == E_ARG
    assert begin(fake, 2, p(f), 12, 2, 3) == E_ARG and begin(fake, 0, p(f), 12, 2, 0) == E_ARG    # (reduced q = 1: forwarded)


# ---- the capture of rechannelize_fixture.py

@pytest.fixture(scope="module")
def capture():
    import rechannelize_fixture as RF
    pcm, pays = RF.capture()
    v, _, tie = RM.channelize(pcm, RF.P, RF.Q, RF.CHANNEL_HZ, RF.RATE)
    rows = np.stack([v.real, v.imag], axis=2).astype(np.float32)
    for a in (pcm, pays, rows):
        a.setflags(write=False)
    return RF, pcm, pays, rows


def test_fixture_decodes_through_the_oracle(capture):
    """the float64 model's rows through the oracle: each frame from its channel, 12 samples late, no second preamble; the empty
    channel has none"""
    import oracle_lib as O
    RF, pcm, pays, rows = capture
    assert pcm.shape == (645021, 2) and rows.shape == (3, RM.n_outputs(645021, RF.P, RF.Q), 2)
    for c in range(2):
        out, r = O.decode(rows[c])
        print("channel %d at %.0f Hz: status %d, sc_start %d, %d flips" % (c, RF.CHANNEL_HZ[c], r.status, r.sc_start, r.bit_flips))
        assert r.status == 0 and (out == pays[c]).all() and r.bit_flips == 0 and r.sc_start == RF.SC_START[c], c
        assert O.decode(rows[c], skip=1)[1].status == 1, c
    assert RF.SC_START == (9612, 17615)
    assert O.decode(rows[2])[1].status == 1


def test_fixture_survey_finds_the_two_centres(capture):
    """before `auto` is relied on: the survey's float64 model over the whole capture, at Rw as it is, and the finder's defaults"""
    import survey_model as SM
    RF, pcm, pays, rows = capture
    bands, fl = SM.find_bands(SM.psd(pcm, 1280)[0][0], float(RF.WIDE_RATE))
    print("floor %.4g, centres %s, widths %s" % (fl, [b["centre_hz"] for b in bands], [b["width_hz"] for b in bands]))
    assert len(bands) == 2
    for b, f in zip(bands, RF.SIGNAL_HZ):
        assert abs(b["centre_hz"] - f) <= 100.0, (b, f)
