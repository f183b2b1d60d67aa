"""The wideband synthesizer at a rational interpolation without a GPU: the float64 model of
resynthesize_model.py and its tolerance rule on an fp32 evaluation and on deliberately wrong models, the branch gains of the taps
read as one sequence, the round trip through the float64 model of the ratio front end (synthesize, then channelize, is a delay of
24 + start Q / P), oracle frames through both models and the oracle's decoder, and the model's windows and argument errors."""
import numpy as np
import pytest

import channelize_model as CM
import oracle_lib as O
import rechannelize_model as RM
import resynthesize_model as RS

RATIOS = [(5, 2, 8000), (33, 16, 8000), (25, 4, 8000), (64, 3, 48000), (125, 4, 8000), (511, 16, 8000)]
N_IN = 120


def geometry(P, Q, Cn, rate, seed=0):
    """centres anywhere inside +- Rw / 2, starts staggered through the residues mod P (and far enough from 0 for a phase taken at
    m - start to differ), unequal gains of both signs; the channels overlap"""
    rw = RM.wide_rate(rate, P, Q)
    rng = np.random.default_rng(1000 * P + Q + seed)
    f = [float(v) for v in rng.uniform(-0.49 * rw, 0.49 * rw, Cn)]
    s = [int(50000 + c * (N_IN * P // (3 * Q)) + (c * 7) % P) for c in range(Cn)]
    g = [float(v) for v in rng.uniform(0.05, 0.5, Cn) * np.where(np.arange(Cn) % 3 == 2, -1.0, 1.0)]
    return f, s, g


@pytest.fixture(scope="module")
def cases():
    """full-scale random int16 rows and the model on them: computed once, read only"""
    out = {}
    for P, Q, rate in RATIOS:
        for Cn in (1, 5):
            x = RS.random_x(Cn, N_IN, np.int16, seed=P + Cn)
            f, s, g = geometry(P, Q, Cn, rate)
            first = s[0] - 7                                          # the window begins before the first start
            v, tol, tie = RS.synthesize(x, P, Q, f, s, g, rate, out_first=first, n_out=RS.n_outputs(s, N_IN, P, Q) + 9 - first)
            for a in (x, v, tol):
                a.setflags(write=False)
            out[P, Q, Cn] = (x, f, s, g, first, v, tol, tie)
    return out


@pytest.mark.parametrize("Cn", [1, 5])
@pytest.mark.parametrize("P,Q,rate", RATIOS)
def test_fp32_evaluation_stays_under_a_quarter_of_tol(cases, P, Q, rate, Cn):
    x, f, s, g, first, v, tol, tie = cases[P, Q, Cn]
    assert tie > 1e-6
    got = RS.synthesize_fp32(x, P, Q, f, s, g, rate, out_first=first, n_out=len(v))
    assert (tol[:7] == 0).all() and (tol[-9:] == 0).all() and (tol[7:-9] > 0).all()
    assert (v[:7] == 0).all() and (v[-9:] == 0).all()
    w = RS.worst(got, v, tol)
    print("%d/%d, %d channels: fp32 evaluation, worst error / tol %.4f" % (P, Q, Cn, w))
    assert w <= 0.25, (P, Q, Cn, w)


def test_the_sequence_is_the_front_ends_table():
    """G[tn] = H[tn mod Q][tn div Q]; for Q = 1 it is the integer front end's h[k]; every tn of the table beyond 24 P holds 0"""
    for P, Q in ((5, 2), (25, 4), (511, 16)):
        H = RM.taps(P, Q)
        G = RS.sequence(P, Q)
        assert len(G) == 24 * P + 1
        flat = H.T.reshape(-1).astype(np.float64)                    # index j Q + q
        assert np.array_equal(flat[:24 * P + 1], G) and not flat[24 * P + 1:].any()
    assert np.array_equal(RS.sequence(6, 1), CM.taps(6).astype(np.float64))


@pytest.mark.parametrize("P,Q", [(p, q) for p, q, _ in RATIOS] + [(31, 15), (6, 1)])
def test_branch_gains(P, Q):
    """D sum_a G[b + a P] is the gain at zero frequency of the branch that makes the outputs with nu mod P = b.  G is a sequence at P
    times the handle's rate, and summing every P-th element of it from b is (1 / P) sum_k Gh(k / P) e^{2 pi i k b / P}, Gh the
    sequence's own transform: the k = 0 term times D is sum G / Q (the Q phases' normalisation, each 1 but for the rounding to fp32),
    the others are the stop band at the multiples of the handle's rate.  The bound is those terms' magnitudes, computed here from
    the taps; what section 4.17's filter test shows of the stop band (below -70 dB) makes it small"""
    G = RS.sequence(P, Q)
    D = P / Q
    gains = np.array([D * G[b::P].sum() for b in range(P)])
    Gh = CM.response(G, np.arange(P) / float(P))
    bound = abs(Gh[0].real / Q - 1.0) + np.abs(Gh[1:]).sum() / Q + 2.0 ** -40
    worst = np.abs(gains - 1.0).max()
    print("%d/%d: worst branch gain error %.3g, bound %.3g" % (P, Q, worst, bound))
    assert worst <= bound, (P, Q, worst, bound)
    assert bound < 1e-3                                               # (the bound itself says something)


def _cascade(P, Q, start, rho, span=80):
    """the cascade synthesize -> channelize_ratio at one centre, for the outputs n = rho (mod Q): y[n] = sum_k e[k] x[n - k],
    e[k] = D sum_i h_{q_n}[i_n - i] G[(i - start) Q - (n - k) P].  Advancing n by Q advances i_n by P and leaves q_n: the cascade is
    periodically time-varying with period Q, and e depends on n through rho alone.  -> e[0 .. span - 1]"""
    H = RM.taps(P, Q).astype(np.float64)
    G = RS.sequence(P, Q)
    T = H.shape[1]
    n = 1000 * Q + rho                                                # (any n of the residue: the expression is periodic)
    u = n * P
    i_n, q_n = u // Q, u % Q
    i = i_n - np.arange(T, dtype=np.int64)                            # tap j of the front end meets capture sample i_n - j
    k = np.arange(span, dtype=np.int64)
    tn = (i[:, None] - start) * Q - (n - k[None, :]) * P
    ok = (tn >= 0) & (tn <= 24 * P)
    return (P / Q) * (H[q_n][:, None] * np.where(ok, G[np.clip(tn, 0, 24 * P)], 0.0)).sum(axis=0)


@pytest.mark.parametrize("P,Q,start,centre", [(5, 2, 0, -3000.0), (25, 4, 7, 11050.0), (33, 16, 3, 1234.567), (125, 4, 11, -100000.25),
                                             (511, 16, 1022, 77000.5)])
def test_round_trip_is_a_delay(P, Q, start, centre):
    """complex noise band-limited to |f| <= rate / 4 (and tapered at both ends), synthesized at a centre and channelized by the
    ratio front end's model at the same centre, is the input d = 24 + start Q / P samples late - a fractional delay where P does not
    divide start.  The outputs n = rho (mod Q) are x through the filter e_rho of _cascade, so their error is x through E_rho(f) =
    e_rho's transform - e^{-2 pi i f d}.  As in 4.15's test the rms error is held to rms(x) times the largest |E_rho(f)| over the
    band, plus the largest |E_rho(f)| anywhere times the share of x outside the band, plus the rounding of the capture to fp32 on
    its way into the front end's model - the worst of the Q residues taken for each; all are computed here from the taps and the
    signal.  The expected output is x delayed by d with a transform long enough that nothing wraps round."""
    rate, n_in = 8000, 1500
    rng = np.random.default_rng(P)
    X = np.zeros(n_in, np.complex128)
    k = np.fft.fftfreq(n_in)
    band = np.abs(k) <= 0.25 - 4.0 / n_in                              # (the taper below widens every line by a bin either side)
    X[band] = rng.standard_normal(band.sum()) + 1j * rng.standard_normal(band.sum())
    x = np.fft.ifft(X)
    x *= np.hanning(n_in + 2)[1:-1] * 0.5 / np.abs(x).max()
    x32 = np.stack([x.real, x.imag], axis=1).astype(np.float32)
    xc = x32[:, 0].astype(np.float64) + 1j * x32[:, 1].astype(np.float64)
    v, _, tie = RS.synthesize(x32[None], P, Q, [centre], [start], [1.0], rate)
    assert tie > 1e-6
    cap = np.stack([v.real, v.imag], axis=1).astype(np.float32)
    y, _, _ = RM.channelize(cap, P, Q, [centre], rate)
    d = 24 + start * Q / P
    L = 1 << 13
    assert y.shape[1] >= n_in + int(d) and L >= 2 * y.shape[1]          # the whole input comes out
    ff = np.fft.fftfreq(L)
    want = np.fft.ifft(np.fft.fft(xc, L) * np.exp(-2j * np.pi * ff * d))[:y.shape[1]]
    rms = np.sqrt(np.mean(np.abs(want) ** 2))
    err = np.sqrt(np.mean(np.abs(y[0] - want) ** 2)) / rms
    f = np.arange(-2048, 2048) / 4096.0
    in_band, anywhere = 0.0, 0.0
    for rho in range(Q):
        e = _cascade(P, Q, start, rho, span=int(d) + 40)
        assert abs(e[0]) < 1e-12 and abs(e[-1]) < 1e-12               # the span holds the whole response
        E = CM.response(e, f) - np.exp(-2j * np.pi * f * d)
        in_band = max(in_band, np.abs(E[np.abs(f) <= 0.25]).max())
        anywhere = max(anywhere, np.abs(E).max())
    Xf = np.abs(np.fft.fft(xc, 1 << 16)) ** 2
    f16 = np.fft.fftfreq(1 << 16)
    out_share = np.sqrt(Xf[np.abs(f16) > 0.25].sum() / Xf.sum())
    rounding = 2.0 ** -24 * 2 * np.abs(RM.taps(P, Q).astype(np.float64)).sum(axis=1).max() * np.abs(v).max() / rms
    bound = in_band + anywhere * out_share + rounding
    print("%d/%d start %d: rms error / rms %.3g, bound %.3g (in band %.3g, out-of-band share %.3g)" % (P, Q, start, err, bound, in_band, out_share))
    assert err <= bound, (P, Q, err, bound)
    assert bound < 1e-2                                               # (the bound itself says something)


def _frame(mode, rate, seed):
    pay = O.payload_for(seed)
    return pay, O.encode_pcm(pay, channels=2, freq_off=0, mode=mode, rate=rate)


@pytest.mark.parametrize("rate,P,Q,modes,centres,starts,gains", [
    (8000, 25, 4, (6, 13, 6), (-14000.0, 9000.0, -3000.0), (7, 50021, 100002), (0.05, 0.5, 0.2)),
    (48000, 64, 3, (6,), (-200000.0,), (4801,), (0.3,)),
], ids=["8 kHz 25/4", "48 kHz 64/3"])
def test_oracle_frames_through_both_models(rate, P, Q, modes, centres, starts, gains):
    """oracle-encoded 2-channel frames at freq_off 0 -> synthesizer model -> noise floor, int16 -> ratio front-end model -> oracle
    decoder: status 0, the payload, 0 flips, sc_start within 1 of the frame's own + 24 + start Q / P"""
    frames = [_frame(m, rate, 40 + i) for i, m in enumerate(modes)]
    n_in = max(len(p) for _, p in frames)
    x = np.zeros((len(frames), n_in, 2), np.int16)
    for c, (_, p) in enumerate(frames):
        x[c, :len(p)] = p
    v, _, tie = RS.synthesize(x, P, Q, centres, starts, gains, rate, with_tol=False)
    assert tie > 1e-6
    rng = np.random.default_rng(7)
    v = v + 1e-3 * (rng.standard_normal(len(v)) + 1j * rng.standard_normal(len(v)))
    cap = RS.quantise(np.stack([v.real, v.imag], axis=1).astype(np.float32))
    rows, _, _ = RM.channelize(cap, P, Q, centres, rate)
    for c, (pay, pcm) in enumerate(frames):
        _, own = O.decode(pcm, rate=rate)
        assert own.status == 0
        row = np.stack([rows[c].real, rows[c].imag], axis=1).astype(np.float32)
        out, res = O.decode(row, rate=rate)
        assert res.status == 0 and (out == pay).all() and res.bit_flips == 0, (c, res.status)
        want = own.sc_start + 24 + starts[c] * Q / P
        print("rate %d channel %d: sc_start %d, the frame's own %d + 24 + %d x %d / %d = %.2f" % (rate, c, res.sc_start, own.sc_start, starts[c], Q, P, want))
        assert abs(res.sc_start - want) <= 1, (c, res.sc_start, want)


def _variants(Q):
    return [v for v in RS.VARIANTS if not (Q == 2 and v == "fraction negated")]   # (at Q = 2 negating the fraction is the definition)


@pytest.mark.parametrize("P,Q,variant", [(P, Q, v) for P, Q in ((5, 2), (25, 4), (511, 16)) for v in _variants(Q)])
def test_wrong_variants_are_rejected(cases, P, Q, variant):
    """each wrong model leaves the tolerance somewhere: the rule tells them from the definition"""
    x, f, s, g, first, v, tol, _ = cases[P, Q, 5]
    w = RS.worst(RS.synthesize(x, P, Q, f, s, g, out_first=first, n_out=len(v), variant=variant)[0], v, tol)
    print("%d/%d %s: worst / tol %.3g" % (P, Q, variant, w))
    assert w > 1.0, (P, Q, variant, w)


def test_there_are_at_least_twelve_variants():
    assert len(_variants(2)) >= 12 and len(set(RS.VARIANTS)) == len(RS.VARIANTS)


def test_model_cuts_into_windows(cases):
    """the model itself: a window of the capture is that part of the whole"""
    x, f, s, g, first, v, tol, _ = cases[25, 4, 5]
    for o, n in ((300, 777), (0, 8), (len(v) - 10, 10), (1023, 2)):
        part, ptol, _ = RS.synthesize(x, 25, 4, f, s, g, out_first=first + o, n_out=n)
        assert np.array_equal(part, v[o:o + n]) and np.array_equal(ptol, tol[o:o + n])


def test_the_ratio_reduces_and_q_1_is_the_integer_model():
    import synthesize_model as SM
    x = RS.random_x(2, 40, np.int16, seed=3)
    f, s, g = [1000.0, -7000.5], [11, 40], [0.3, -0.2]
    a = RS.synthesize(x, 25, 4, f, s, g)
    b = RS.synthesize(x, 50, 8, f, s, g)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    v, tol, _ = RS.synthesize(x, 12, 2, f, s, g)
    v6, tol6, _ = SM.synthesize(x, 6, f, s, g)
    assert len(v) == len(v6) and np.abs(v - v6).max() <= 1e-3 * tol6.max() and np.allclose(tol, tol6, rtol=1e-12, atol=0)


def test_model_argument_errors():
    x = RS.random_x(2, 10)
    ok = dict(x=x, P=25, Q=4, centres_hz=[0.0, 1000.0], starts=[0, 5], gains=[1.0, 0.5])
    RS.synthesize(**ok)
    for bad in (dict(P=0), dict(Q=0), dict(P=-25), dict(P=7, Q=4), dict(P=129, Q=4), dict(P=35, Q=17), dict(centres_hz=[0.0]),
                dict(starts=[0, -1]), dict(starts=[0, (1 << 50) + 1]), dict(centres_hz=[0.0, 25000.5]), dict(centres_hz=[0.0, float("nan")]),
                dict(gains=[1.0, float("inf")]), dict(gains=[1.0, 3e38]), dict(x=x.astype(np.uint8)), dict(x=x[0]), dict(out_first=-1),
                dict(n_out=0)):
        with pytest.raises(ValueError):
            RS.synthesize(**dict(ok, **bad))
