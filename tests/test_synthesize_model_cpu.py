"""The wideband synthesizer without a GPU: the float64 model of synthesize_model.py and its tolerance rule
on an fp32 evaluation and on deliberately wrong models, the polyphase branch gains of the taps, the round trip through the float64
model of the wideband front end (synthesize, then channelize, is a delay), oracle frames through both models and the oracle's
decoder, and the model's argument errors."""
import numpy as np
import pytest

import channelize_model as CM
import oracle_lib as O
import synthesize_model as SM

CENTRES = {2: [1234.567, -5000.0, 7999.9, -0.001, 3000.25], 3: [-8000.0, 1234.567, 11999.0, 0.0, -4321.0],
           6: [-13000.0, 3000.25, 11050.0, 23999.5, -1.0], 32: [100001.3, -2718.28, 127999.0, -90000.7, 12.5]}


def geometry(D, Cn, n_in, seed=0):
    """centres, starts at every residue mod D (and far enough from 0 for a phase taken at m - start to differ), unequal gains of both
    signs"""
    rng = np.random.default_rng(10 * D + seed)
    starts = [int(50000 + c * (n_in * D // 3) + (c % D)) for c in range(Cn)]
    gains = [float(g) for g in rng.uniform(0.05, 0.5, Cn) * np.where(np.arange(Cn) % 3 == 2, -1.0, 1.0)]
    return CENTRES[D][:Cn], starts, gains


@pytest.fixture(scope="module")
def cases():
    """full-scale random int16 rows and the model on them: computed once, read only"""
    out = {}
    for D in (2, 3, 6, 32):
        for Cn in (1, 5):
            x = SM.random_x(Cn, 300, np.int16, seed=D + Cn)
            f, s, g = geometry(D, Cn, 300)
            first = s[0] - 7                                          # the window begins before the first start
            v, tol, tie = SM.synthesize(x, D, f, s, g, out_first=first, n_out=SM.n_outputs(s, 300, D) + 9 - first)
            for a in (x, v, tol):
                a.setflags(write=False)
            out[D, Cn] = (x, f, s, g, first, v, tol, tie)
    return out


@pytest.mark.parametrize("Cn", [1, 5])
@pytest.mark.parametrize("D", [2, 3, 6, 32])
def test_fp32_evaluation_stays_under_a_quarter_of_tol(cases, D, Cn):
    x, f, s, g, first, v, tol, tie = cases[D, Cn]
    assert tie > 1e-6
    got = SM.synthesize_fp32(x, D, f, s, g, out_first=first, n_out=len(v))
    assert (tol[:7] == 0).all() and (tol[-9:] == 0).all() and (tol[7:-9] > 0).any()
    w = SM.worst(got, v, tol)
    print("D %d, %d channels: fp32 evaluation, worst error / tol %.4f" % (D, Cn, w))
    assert w <= 0.25, (D, Cn, w)


@pytest.mark.parametrize("D", list(range(2, 33)))
def test_polyphase_branch_gains(D):
    """D sum_a h[b + a D] is the gain of branch b at zero frequency: 1 but for the D - 1 aliases of the stop band, each at most the
    10^(-75.4 / 20) that section 4.14 proves"""
    h = CM.taps(D).astype(np.float64)
    worst = max(abs(D * h[b::D].sum() - 1.0) for b in range(D))
    print("D %d: worst branch gain error %.3g" % (D, worst))
    assert worst <= (D - 1) * 10 ** (-75.4 / 20), (D, worst)


@pytest.mark.parametrize("D,centre", [(2, -3000.0), (3, 1234.567), (6, 11050.0), (32, -100000.25)])
def test_round_trip_is_a_delay(D, centre):
    """complex noise band-limited to |f| <= rate / 4 (and tapered at both ends), synthesized at a centre and a start that D divides and channelized at the same
    centre, is the input 24 + start / D samples late.  The cascade's impulse response at the handle's rate is g[n] = D (h * h)[n D];
    the error is x filtered by e = g - delta_24, so its rms is at most rms(x) times the largest |E(f)| over the band (which holds the
    pass band's ripple of the two filters and the aliases of their stop bands) plus the largest |E(f)| anywhere times the share of
    x outside the band (the taper's leakage), plus the rounding of the capture to fp32 on the way into the front end's model: all
    three are computed here from the taps and the signal, no constant is written in."""
    rate, n_in, start = 8000, 1500, 7 * D
    rng = np.random.default_rng(D)
    X = np.zeros(n_in, np.complex128)
    k = np.fft.fftfreq(n_in)
    band = np.abs(k) <= 0.25 - 4.0 / n_in                              # (the taper below widens every line by a bin either side)
    X[band] = rng.standard_normal(band.sum()) + 1j * rng.standard_normal(band.sum())
    x = np.fft.ifft(X)
    x *= np.hanning(n_in + 2)[1:-1] * 0.5 / np.abs(x).max()
    x32 = np.stack([x.real, x.imag], axis=1).astype(np.float32)
    xc = x32[:, 0].astype(np.float64) + 1j * x32[:, 1].astype(np.float64)
    v, _, tie = SM.synthesize(x32[None], D, [centre], [start], [1.0], rate)
    assert tie > 1e-6
    cap = np.stack([v.real, v.imag], axis=1).astype(np.float32)
    y, _, _ = CM.channelize(cap, D, [centre], rate)
    delay = 24 + start // D
    want = np.zeros(y.shape[1], np.complex128)
    want[delay:delay + n_in] = xc[:len(want) - delay]
    assert len(want) >= delay + n_in                                  # the whole input comes out
    err = np.sqrt(np.mean(np.abs(y[0] - want) ** 2)) / np.sqrt(np.mean(np.abs(want) ** 2))
    peak = np.abs(y[0] - want).max() / np.abs(want).max()
    h = CM.taps(D).astype(np.float64)
    g = D * np.convolve(h, h)[::D]
    assert len(g) == 49
    f = np.arange(-2048, 2048) / 4096.0
    E = CM.response(g, f) - np.exp(-2j * np.pi * f * 24)
    Xf = np.abs(np.fft.fft(xc, 1 << 16)) ** 2
    ff = np.fft.fftfreq(1 << 16)
    out_share = np.sqrt(Xf[np.abs(ff) > 0.25].sum() / Xf.sum())
    rounding = 2.0 ** -24 * 2 * np.abs(h).sum() * np.abs(v).max() / np.sqrt(np.mean(np.abs(want) ** 2))
    bound = np.abs(E[np.abs(f) <= 0.25]).max() + np.abs(E).max() * out_share + rounding
    print("D %d: rms error / rms %.3g, peak error / peak %.3g, bound %.3g (in band %.3g, out-of-band share %.3g)"
          % (D, err, peak, bound, np.abs(E[np.abs(f) <= 0.25]).max(), out_share))
    assert err <= bound, (D, err, bound)
    assert bound < 1e-2                                               # (the bound itself says something)


def _frame(mode, rate, seed):
    pay = O.payload_for(seed)
    return pay, O.encode_pcm(pay, channels=2, freq_off=0, mode=mode, rate=rate)


@pytest.mark.parametrize("rate,D,modes,centres,starts,gains", [
    (8000, 3, (6, 13, 6), (-8000.0, 0.0, 8000.0), (3000, 30001, 60002), (0.05, 0.5, 0.2)),
    (48000, 2, (6,), (-20000.0,), (4801,), (0.3,)),
], ids=["8 kHz", "48 kHz"])
def test_oracle_frames_through_both_models(rate, D, modes, centres, starts, gains):
    """oracle-encoded 2-channel frames at freq_off 0 -> synthesizer model -> noise floor, int16 -> front-end model -> oracle decoder:
    status 0, the payload, 0 flips, sc_start = the frame's own + 24 + start / D (within 1 where D does not divide start)"""
    frames = [_frame(m, rate, 40 + i) for i, m in enumerate(modes)]
    n_in = max(len(p) for _, p in frames)
    x = np.zeros((len(frames), n_in, 2), np.int16)
    for c, (_, p) in enumerate(frames):
        x[c, :len(p)] = p
    assert sorted(s % D for s in starts) == list(range(D)) or len(starts) == 1
    v, _, tie = SM.synthesize(x, D, centres, starts, gains, rate)
    assert tie > 1e-6
    rng = np.random.default_rng(7)
    v = v + 1e-3 * (rng.standard_normal(len(v)) + 1j * rng.standard_normal(len(v)))
    cap = SM.quantise(np.stack([v.real, v.imag], axis=1).astype(np.float32))
    rows, _, _ = CM.channelize(cap, D, centres, rate)
    for c, (pay, pcm) in enumerate(frames):
        _, own = O.decode(pcm, rate=rate)
        assert own.status == 0
        row = np.stack([rows[c].real, rows[c].imag], axis=1).astype(np.float32)
        out, res = O.decode(row, rate=rate)
        assert res.status == 0 and (out == pay).all() and res.bit_flips == 0, (c, res.status)
        want = own.sc_start + 24 + starts[c] / D
        print("rate %d channel %d: sc_start %d, the frame's own %d + 24 + %d / %d" % (rate, c, res.sc_start, own.sc_start, starts[c], D))
        if starts[c] % D == 0:
            assert res.sc_start == want, (c, res.sc_start, want)
        else:
            assert abs(res.sc_start - want) <= 1, (c, res.sc_start, want)


@pytest.mark.parametrize("D,variant", [(D, v) for v in SM.VARIANTS for D in (2, 6, 32)])
def test_wrong_variants_are_rejected(cases, D, variant):
    """each wrong model leaves the tolerance somewhere: the rule tells them from the definition"""
    x, f, s, g, first, v, tol, _ = cases[D, 5]
    w = SM.worst(SM.synthesize(x, D, f, s, g, out_first=first, n_out=len(v), variant=variant)[0], v, tol)
    print("D %d %s: worst / tol %.3g" % (D, variant, w))
    assert w > 1.0, (D, variant, w)


def test_model_cuts_into_windows(cases):
    """the model itself: a window of the capture is that part of the whole"""
    x, f, s, g, first, v, tol, _ = cases[6, 5]
    part, ptol, _ = SM.synthesize(x, 6, f, s, g, out_first=first + 1000, n_out=777)
    assert np.array_equal(part, v[1000:1777]) and np.array_equal(ptol, tol[1000:1777])


def test_quantiser_never_gives_minus_32768():
    v = np.array([[-5.0, -1.0], [1.0, 7.0], [0.25, -0.25], [-0.0, -np.inf]], np.float32)
    assert SM.quantise(v).tolist() == [[-32767, -32767], [32767, 32767], [8192, -8192], [0, -32767]]


def test_model_argument_errors():
    x = SM.random_x(2, 10)
    ok = dict(x=x, D=6, centres_hz=[0.0, 1000.0], starts=[0, 5], gains=[1.0, 0.5])
    SM.synthesize(**ok)
    for bad in (dict(D=1), dict(D=33), dict(centres_hz=[0.0]), dict(starts=[0, -1]), dict(starts=[0, (1 << 50) + 1]),
                dict(centres_hz=[0.0, 24000.5]), dict(centres_hz=[0.0, float("nan")]), dict(gains=[1.0, float("inf")]),
                dict(gains=[1.0, 3e38]), dict(x=x.astype(np.uint8)), dict(x=x[0]), dict(out_first=-1), dict(n_out=0)):
        with pytest.raises(ValueError):
            SM.synthesize(**dict(ok, **bad))
