"""The float64 demodulator model (demod_model.py) against the oracle's CONS_RAW tap, carrier by carrier: the CPU link of DESIGN.md
section 4.3, "What pins the demodulator".  Every frame of demod_model.cases() goes through O.decode(taps=True) once (cached) and
through the model fed with the oracle's own sc_start and cfo_rad.

1. the oracle inside the rule, its worst d re-measured and held within 25 % of demod_model.MEASURED, its erasure ties inside the cap;
2. the one-channel front end of the model against orc_front_end_rate, sample by sample, by counted roundings (it guards the model);
3. every wrong variant of the model rejected by the rule against the oracle's output.
"""
import numpy as np
import pytest

import demod_model as D
from demod_record import record

CASES = D.cases()


@pytest.fixture(scope="module")
def verdicts():
    out = {}
    for c in CASES:
        out[c.name] = v = D.oracle_verdict(c)
        record("oracle", c.name, v, D.T[c.channels])
    return out


# ---------------------------------------------------------------- 1
def test_the_table_is_what_the_header_says():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    a = [c for c in CASES if c.name[0] == "A"]
    assert sorted((c.mode, c.noise_db is None) for c in a) == sorted((m, k) for m in range(6, 14) for k in (False, True))
    for c in CASES:
        ok = D.TX.permitted_offsets(c.mode, c.rate, c.channels)
        assert c.freq_off in (ok[0], ok[-1]), c.name
    assert {(c.rate, c.mode, c.noise_db is None) for c in CASES if c.name[0] == "E"} == {
        (r, m, k) for r in (16000, 44100, 48000) for m in (10, 13) for k in (False, True)}
    assert {(c.rate, c.dc != 0) for c in CASES if c.channels == 1} == {(r, k) for r in (8000, 16000, 44100, 48000) for k in (False, True)}
    assert {c.fmt for c in CASES} == {"s16", "u8", "f32"}


def test_oracle_decodes_every_frame_of_the_table():
    for c in CASES:
        o = D.oracle_of(c)
        assert o.status in (0, 6) and o.oper_mode == c.mode, (c.name, o.status)
        if c.noise_db is None and not c.cut:
            assert o.status == 0 and (o.payload == D.payload_of(c)).all(), c.name


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_oracle_against_model(verdicts, name):
    v = verdicts[name]
    print("%s: worst %.3f median %.3f abs %.2e ties %d unexplained %d" % (name, v.worst, v.median, v.worst_abs, v.ties, v.unexplained))
    assert D.accept(v), (name, v[:6])
    assert v.ties <= D.TIE_CAP * v.n
    assert 0.5 < v.median < 1.5, "the unit is flat across rates, modes, noise and fades"


@pytest.mark.parametrize("channels", [2, 1])
def test_measured_worst_is_the_recorded_one(verdicts, channels):
    """T = 4 x MEASURED cannot drift silently: the worst d of the oracle over the table, re-measured, within 25 % of the constant"""
    worst = max(verdicts[c.name].worst for c in CASES if c.channels == channels)
    print("channels %d: worst %.4f, recorded %.4f" % (channels, worst, D.MEASURED[channels]))
    assert 0.75 * D.MEASURED[channels] <= worst <= 1.25 * D.MEASURED[channels]
    assert D.T[channels] == 4.0 * D.MEASURED[channels]


def test_the_table_reaches_the_regimes_it_names(verdicts):
    def model(name):
        c = D.case(name)
        o = D.oracle_of(c)
        return c, D.demod(D.analytic_of(c), c.rate, c.mode, o.sc_start, o.cfo_rad)
    _, m = model("B mode 6 waterfall, +33.3 Hz")
    assert 0.05 <= m.zero.mean() <= 0.10                                       # erasures in 5 - 10 % of the points
    _, m = model("B mode 13 -12 dB, three taps")                               # deep fades: carriers 20 dB under the strongest
    c13 = D.case("B mode 13 -12 dB, three taps")
    taps = np.zeros(32, complex)
    for d, g in c13.multipath:
        taps[d] = g
    h = np.abs(np.fft.fft(taps, 1280))
    band = h[(np.arange(256) - 128 + round(c13.freq_off * 1280 / 8000)) % 1280]
    assert band.min() < 0.1 * band.max()
    c, m = model("D mode 6 -20 dB cut off 16700 early")                        # the recording ends inside a data symbol: one row partly there
    cols, rows = D.geometry(c.mode)
    o = D.oracle_of(c)
    n = D.frame_of(c).shape[0]
    st, sl = D.stride_of(c.rate), D.symbol_len(c.rate)
    part = [j for j in range(1, rows + 1) if o.sc_start + (2 + j) * st < n < o.sc_start + (2 + j) * st + sl]
    assert len(part) == 1 and part[0] < rows
    j = part[0]                                                                # row j - 1 of cons is the partial symbol over a whole one,
    assert not m.zero[j - 1].all() and m.zero[j + 1:].all() and (m.u[j + 1:] == 0).all()   # from row j + 1 on both are silent
    got = np.asarray(o.cons, np.float32).reshape(rows, cols, 2)
    assert (got[j + 1:] == 0).all()
    c, m = model("D mode 9 -17 dB row 17 silent")
    cols, rows = D.geometry(c.mode)
    got = np.asarray(D.oracle_of(c).cons, np.float32).reshape(rows, cols, 2)
    assert (m.u[17] == 0).all() and m.zero[17].all() and m.zero[18].all() and (got[17:19] == 0).all()
    assert not m.zero[16].all() and not m.zero[19].all()


# ---------------------------------------------------------------- 2
@pytest.mark.parametrize("name", [c.name for c in CASES if c.channels == 1])
def test_front_end_model_against_the_oracle(name):
    c = D.case(name)
    f = D.front_end_check(D.frame_of(c), c.rate)
    print("%s: %d samples, re at %.3f of its bound, im at %.3f" % (name, f.n, f.worst_re, f.worst_im))
    assert f.bad == 0, f


def test_front_end_check_has_teeth():
    """the same check run with a wrong model fails by orders of magnitude"""
    c = D.case("F mono 8 kHz mode 9 -17 dB, DC")
    real = D.analytic
    try:
        for v in D.MONO_VARIANTS:
            D.analytic = lambda pcm, rate, variant=None, v=v: real(pcm, rate, v)
            f = D.front_end_check(D.frame_of(c), c.rate)
            assert f.bad > 0.5 * f.n and max(f.worst_re, f.worst_im) > 1e3, (v, f)
    finally:
        D.analytic = real


# ---------------------------------------------------------------- 3
NOISY, WATERFALL, WAVE = "A mode 6 list-1 level", "B mode 6 waterfall, +33.3 Hz", "B mode 6 -21 dB, carrier wave 12 dB under the signal"
HELD_ON = {v: NOISY for v in D.VARIANTS}
HELD_ON["erasure at |c| > 4"] = WATERFALL                                      # needs points with 2 < |c| <= 4
HELD_ON["one twiddle 1e-6 rad off"] = WAVE                                     # needs energy in the bin half a transform away


def _variant_verdict(name, variant, **kw):
    c = D.case(name)
    o = D.oracle_of(c)
    return D.judge(o.cons, D.demod(D.analytic_of(c), c.rate, c.mode, o.sc_start, o.cfo_rad, variant, **kw), D.T[c.channels])


@pytest.mark.parametrize("variant", D.VARIANTS)
def test_wrong_variant_is_rejected(variant):
    """each variant on the frame that exposes it (HELD_ON): most on a noisy frame, the erasure limit on the waterfall frame, the
    twiddle on the frame with a carrier wave half a transform from the twiddled carrier (41.7 there; in noise alone 5.8, see
    test_twiddle_sensitivity)"""
    v = _variant_verdict(HELD_ON[variant], variant)
    print("%s on %s: worst %.3g median %.3g ties %d unexplained %d" % (variant, HELD_ON[variant], v.worst, v.median, v.ties, v.unexplained))
    assert not D.accept(v), (variant, v[:6])


def test_twiddle_sensitivity():
    """the size of twiddle error the rule rejects in noise ALONE, on the waterfall frame: from 2e-6 rad on its most exposed bins, from
    8e-6 rad on every bin (every carrier judged as if its bin alone were off); at 1e-6 rad on none - which is why the 1e-6 rad
    variant is held on the carrier-wave frame, whose wave sits where demod_model.tone_hz says"""
    c = D.case(WAVE)
    o = D.oracle_of(c)
    sl = D.symbol_len(c.rate)
    k0 = D.twiddled_carrier(c.mode) - D.geometry(c.mode)[0] // 2
    assert c.tone[0] == c.freq_off + (k0 - sl // 2) * c.rate / sl and abs(c.tone[0]) < c.rate / 2
    lo = c.freq_off - D.TX.MODES[c.mode].band_width / 2
    assert not lo <= c.tone[0] <= lo + D.TX.MODES[c.mode].band_width                  # outside the band
    assert o.status == 0 and (o.payload == D.payload_of(c)).all()
    cols = D.geometry(6)[0]
    worst = {}
    for rad in (1e-6, 2e-6, 8e-6):
        v = _variant_verdict(WATERFALL, "one twiddle 1e-6 rad off", twiddle_rad=rad, twiddle_every_bin=True)
        worst[rad] = np.where(np.isfinite(v.d), v.d, 0.0).max(axis=0)
        print("%.0e rad: worst bin %.2f, least exposed bin %.2f, bins above T %d of %d" % (
            rad, worst[rad].max(), worst[rad].min(), (worst[rad] > D.T[2]).sum(), cols))
    assert (worst[1e-6] <= D.T[2]).all()
    assert (worst[2e-6] > D.T[2]).any()
    assert (worst[8e-6] > D.T[2]).all()


@pytest.mark.parametrize("variant", D.MONO_VARIANTS)
@pytest.mark.parametrize("name", ["F mono 8 kHz mode 9 -17 dB, DC", "F mono 48 kHz mode 10 clean, DC"])
def test_wrong_front_end_is_rejected(name, variant):
    c = D.case(name)
    assert c.dc != 0                                                           # "no dc blocker" on an input with an offset
    o = D.oracle_of(c)
    v = D.judge(o.cons, D.demod(D.analytic(D.frame_of(c), c.rate, variant), c.rate, c.mode, o.sc_start, o.cfo_rad), D.T[1])
    assert not D.accept(v), (variant, v[:6])


def test_rule_on_constructed_points():
    """judge() itself: exact zeros where u = 0, ties only inside T u of |c| = 2, everything else unexplained"""
    raw = np.array([[1.0 + 0j, 2.0 + 1e-7, 0.0, 3.0, 1.0, 2.0 - 1e-7]])
    u = np.array([[1e-7, 1e-7, 0.0, 1e-7, 1e-7, 1e-7]])
    zero = np.array([[False, True, True, True, False, False]])
    m = D.Model(np.where(zero, 0, raw), raw, u, zero)
    ok = np.array([[1.0 + 5e-7j, 0.0, 0.0, 0.0, 1.0, 2.0 - 1e-7]])
    v = D.judge(ok, m, 10.0)
    assert v.unexplained == 0 and v.ties == 0 and abs(v.worst - 5.0) < 1e-6
    tie = ok.copy()
    tie[0, 1], tie[0, 5] = 2.0, 0.0                                            # delivered where the model erases, and the reverse: both at |c| = 2
    v = D.judge(tie, m, 10.0)
    assert v.unexplained == 0 and v.ties == 2 and not D.accept(v)              # 2 of 6 points is above the cap
    for k, val in ((0, 1.0 + 2e-6j), (2, 1e-30), (3, 3.0), (4, 0.0)):
        bad = ok.copy()
        bad[0, k] = val
        assert D.judge(bad, m, 10.0).unexplained == 1, k
