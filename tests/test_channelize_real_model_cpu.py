"""The wideband front end for a real capture without a GPU: the float64 model of channelize_real_model.py
against twice the analytic models on the capture (x, 0), on tones at the pass band's edge and on a tone beside its mirror, the
tolerance rule on an fp32 evaluation in the device's order and on deliberately wrong models, blocks against one call, the rule for
the centres at its edges, and the two captures of wideband_real_fixture.py through the oracle."""
import numpy as np
import pytest

import channelize_model as CM
import channelize_real_model as XM
import rechannelize_model as RM

RATE = 8000
RATIOS = [(2, 1), (6, 1), (25, 4)]
# inside the rule at every ratio's own Rw (D = 2: 2000 .. 6000 Hz), arbitrary, of both signs
CENTRES = {(2, 1): [2234.5, -5000.25], (6, 1): [3234.5, -17000.0, 11050.0], (25, 4): [2234.5, -14000.0, 9000.25]}


@pytest.fixture(scope="module")
def cases():
    """full-scale random int16 input, the model on it: computed once, read only"""
    out = {}
    for P, Q in RATIOS:
        W = 400 * P // Q + 1
        pcm = XM.random_real(W, np.int16, seed=P)
        v, tol, tie = XM.channelize(pcm, P, Q, CENTRES[(P, Q)], RATE)
        for a in (pcm, v, tol):
            a.setflags(write=False)
        out[(P, Q)] = (pcm, v, tol, tie)
    return out


@pytest.mark.parametrize("P,Q", RATIOS + [(32, 1), (125, 16)])
@pytest.mark.parametrize("dtype", [np.int16, np.uint8, np.float32])
def test_model_is_twice_the_analytic_models_on_a_zero_imaginary_part(P, Q, dtype):
    """to 1e-12 relative, value and tolerance, from inside a stream too"""
    rw = XM.wide_rate(RATE, P, Q)
    f = [0.3 * rw, -0.11 * rw]
    T = XM.n_taps(P, Q)
    pcm = XM.random_real(60 * P // Q + 7, dtype, seed=5)
    for in_first, out_first in ((0, 0), (3, -(-(3 + T - 1) * Q // P))):
        v, tol, _ = XM.channelize(pcm, P, Q, f, RATE, in_first=in_first, out_first=out_first)
        two = XM.with_zero_imag(pcm)
        if Q == 1:
            w, wtol, _ = CM.channelize(two, P, f, RATE, in_first=in_first, out_first=out_first)
        else:
            w, wtol, _ = RM.channelize(two, P, Q, f, RATE, in_first=in_first, out_first=out_first)
        assert v.shape == w.shape and v.shape[1] > 24
        assert np.abs(v - 2.0 * w).max() <= 1e-12 * np.abs(w).max()
        assert np.allclose(tol, 2.0 * wtol, rtol=1e-12, atol=0)


@pytest.mark.parametrize("P,Q", RATIOS)
@pytest.mark.parametrize("delta", [-2000.0, 2000.0, 500.0])
def test_a_real_tone_comes_out_as_its_analytic_signal(P, Q, delta):
    """a real cosine of amplitude A at f_c + delta, delta at the pass band's edge rate / 4 and inside: the channel at f_c gives
    A G(delta) exp(2 pi i delta (n - 12) / rate) - amplitude A, not A / 2 - plus the mirror through the stop band"""
    rw = XM.wide_rate(RATE, P, Q)
    f_c = 0.25 * rw                                                  # the mirror of every tone lies rate / 2 away or further
    A = 0.5
    W = 80 * P // Q + 5
    m = np.arange(W)
    x = (A * np.cos(2 * np.pi * (f_c + delta) * m / rw)).astype(np.float32)
    v, tol, tie = XM.channelize(x, P, Q, [f_c], RATE)
    inc, _ = XM.inc_of(f_c, rw)
    d = f_c + delta - inc * rw / 2.0 ** 32
    R = RM.aligned_response(RM.taps(P, Q).astype(np.float64), P, Q, [d / rw])[:, 0]
    n = np.arange(24, v.shape[1])
    want = A * R[(n * P) % Q] * np.exp(2j * np.pi * d * (n - 12) / RATE)
    err = np.abs(v[0, 24:] - want).max()
    print("%d/%d delta %+.0f: |y| %.6f A, off the analytic tone by %.2e A" % (P, Q, delta, np.abs(v[0, 24:]).mean() / A, err / A))
    assert err <= 2.0 * 10 ** (-70 / 20.0) * A                       # the mirror: at most -70 dB, doubled like the rest
    assert abs(20 * np.log10(np.abs(v[0, 24:]).mean() / A)) <= 0.01


@pytest.mark.parametrize("P,Q", RATIOS)
def test_a_tone_and_its_mirror(P, Q):
    """the channel at +f takes the tone, the channel at -f its conjugate: y_{-f} = conj y_{+f} for a real capture, to the rounding of
    the model (the increments of +f and -f are each other's negatives)"""
    rw = XM.wide_rate(RATE, P, Q)
    f_c, A = 0.25 * rw, 0.25
    m = np.arange(60 * P // Q + 3)
    x = (A * np.cos(2 * np.pi * (f_c + 700.0) * m / rw + 0.3)).astype(np.float32)
    v, tol, _ = XM.channelize(x, P, Q, [f_c, -f_c], RATE)
    assert np.abs(v[1] - np.conj(v[0])).max() <= 1e-12 * A
    assert np.abs(np.abs(v[0, 24:]) - A).max() <= 2e-3 * A           # (0.01 dB of ripple is 1.2e-3, the mirror at -70 dB 3e-4)


@pytest.mark.parametrize("P,Q", RATIOS)
def test_fp32_evaluation_stays_under_a_quarter_of_tol(cases, P, Q):
    """the device's order in fp32 numpy"""
    pcm, v, tol, tie = cases[(P, Q)]
    assert tie > 1e-6 and (tol[:, 24:] > 0).all()
    w = XM.worst(XM.channelize_fp32(pcm, P, Q, CENTRES[(P, Q)], RATE), v, tol)
    print("%d/%d: fp32 evaluation, worst error / tol %.4f" % (P, Q, w))
    assert w <= 0.25, (P, Q, w)


@pytest.mark.parametrize("P,Q,variant", [(P, Q, v) for v in XM.VARIANTS for (P, Q) in RATIOS])
def test_wrong_variants_are_rejected(cases, P, Q, variant):
    """each wrong model leaves the tolerance somewhere past the filter's fill"""
    pcm, v, tol, _ = cases[(P, Q)]
    bad = XM.channelize(pcm, P, Q, CENTRES[(P, Q)], RATE, variant=variant)[0]
    w = XM.worst(bad[:, 24:], v[:, 24:], tol[:, 24:])
    print("%d/%d %s: worst / tol %.3g" % (P, Q, variant, w))
    assert w > 1.0, (P, Q, variant, w)


def test_there_are_eight_variants():
    assert len(XM.VARIANTS) >= 8 and len(set(XM.VARIANTS)) == len(XM.VARIANTS)


@pytest.mark.parametrize("P,Q", RATIOS)
def test_model_cuts_into_blocks(cases, P, Q):
    """a block with its T - 1 samples of history gives the outputs of the whole capture, for every residue of the first output"""
    pcm, v, tol, _ = cases[(P, Q)]
    T = XM.n_taps(P, Q)
    for o0 in range(40, 40 + Q):
        i0 = o0 * P // Q - (T - 1)
        assert i0 > 0
        part, ptol, _ = XM.channelize(pcm[i0:], P, Q, CENTRES[(P, Q)], RATE, out_first=o0, in_first=i0)
        assert np.array_equal(part, v[:, o0:]) and np.array_equal(ptol, tol[:, o0:])


@pytest.mark.parametrize("rate,P,Q", [(8000, 2, 1), (8000, 6, 1), (8000, 25, 4), (48000, 64, 3), (44100, 125, 16)])
def test_centre_rule_at_its_edges(rate, P, Q):
    """each edge exactly on (admitted) and one ulp outside (refused), one ulp inside (admitted), for either sign"""
    lo, hi = XM.centre_edges(rate, P, Q)
    assert lo == rate / 4.0 and lo <= hi
    for s in (1.0, -1.0):
        assert XM.centre_ok(s * lo, rate, P, Q) and XM.centre_ok(s * hi, rate, P, Q)
        assert XM.centre_ok(s * np.nextafter(lo, np.inf), rate, P, Q) == (lo < hi)
        assert XM.centre_ok(s * np.nextafter(hi, 0.0), rate, P, Q) == (lo < hi)
        assert not XM.centre_ok(s * np.nextafter(lo, 0.0), rate, P, Q)
        assert not XM.centre_ok(s * np.nextafter(hi, np.inf), rate, P, Q)
    for bad in (0.0, float("nan"), float("inf"), -float("inf"), 0.5 * XM.wide_rate(rate, P, Q)):
        assert not XM.centre_ok(bad, rate, P, Q)
    assert XM.centre_ok(2000.0, 8000, 6, 1)                          # the reference's default offset: in the transition band, admitted


# ---- the captures of wideband_real_fixture.py

def _rows(pcm, P, Q, centres):
    v, _, tie = XM.channelize(pcm, P, Q, centres, RATE)
    assert tie > 1e-6
    return np.stack([v.real, v.imag], axis=2).astype(np.float32)


def test_the_48_khz_capture_decodes_through_the_oracle():
    import oracle_lib as O
    import wideband_real_fixture as XF
    pcm, pays = XF.capture48()
    assert pcm.ndim == 1 and pcm.dtype == np.int16
    rows = _rows(pcm, XF.DECIM48, 1, XF.CHANNEL48_HZ)
    for c in range(3):
        out, r = O.decode(rows[c])
        print("channel %d at %.0f Hz: status %d, sc_start %d, %d flips" % (c, XF.CHANNEL48_HZ[c], r.status, r.sc_start, r.bit_flips))
        assert r.status == 0 and (out == pays[c]).all() and r.bit_flips == 0 and r.sc_start == XF.SC_START48[c], c
        assert O.decode(rows[c], skip=1)[1].status == 1, c
    out, r = O.decode(rows[3])                                       # 4050 Hz above the strong frame: its header fails first
    assert r.status == 6 and abs(r.cfo_rad * RATE / (2 * np.pi) - 3950.0) < 1.0
    out, r = O.decode(rows[3], skip=1)
    assert r.status == 0 and (out == pays[3]).all() and r.bit_flips == 0 and r.sc_start == XF.SC_START48[3]
    assert abs(r.cfo_rad * RATE / (2 * np.pi) + 50.0) < 0.5
    assert O.decode(rows[3], skip=2)[1].status == 1
    assert XF.SC_START48 == (9612, 17613, 25615, 33613)
    assert O.decode(rows[4])[1].status == 1 and O.decode(rows[5])[1].status == 1   # the empty channel; the mirror of the first frame


def test_the_50_khz_capture_decodes_through_the_oracle():
    import oracle_lib as O
    import wideband_real_fixture as XF
    pcm, pays = XF.capture50()
    assert pcm.shape == (645021,) and pcm.dtype == np.int16
    rows = _rows(pcm, XF.P50, XF.Q50, XF.CHANNEL50_HZ)
    for c in range(2):
        out, r = O.decode(rows[c])
        print("channel %d at %.0f Hz: status %d, sc_start %d, %d flips" % (c, XF.CHANNEL50_HZ[c], r.status, r.sc_start, r.bit_flips))
        assert r.status == 0 and (out == pays[c]).all() and r.bit_flips == 0 and r.sc_start == XF.SC_START50[c], c
        assert O.decode(rows[c], skip=1)[1].status == 1, c
    assert XF.SC_START50 == (9612, 17615)
    assert O.decode(rows[2])[1].status == 1 and O.decode(rows[3])[1].status == 1
