"""The grid synthesizer at a ratio without a GPU: the float64 model of synthesize_grid_ratio_model.py - the
decimation-in-time plan against numpy's transform, the computed form against the definition as it stands, against section 4.18's
model at the slot centres and against section 4.20's model where Q = 1 and P is a power of two; the tolerance rule on an fp32
evaluation and on deliberately wrong models; windows; the round trip through the grid front end's model at the same ratio; oracle
frames through both; argument errors."""
import numpy as np
import pytest

import channelize_grid_ratio_model as CGR
import channelize_model as CM
import oracle_lib as O
import rechannelize_model as RM
import resynthesize_model as RS
import synthesize_grid_model as SG
import synthesize_grid_ratio_model as R

RATIOS = [(3, 1), (5, 2), (6, 1), (15, 2), (25, 4), (45, 16), (75, 2), (243, 1), (500, 1)]
IDS = ["%d/%d" % r for r in RATIOS]
N_IN = 40


def _S(tol, P):
    return tol / (2.0 ** -24 * R.tol_factor(2 * P))


def geometry(P, Q, seed=0):
    """three rows: the two extreme slots and slot 0, starts 0 / P / several P, signed gains"""
    k0, n = R.slot_range(P, Q)
    rng = np.random.default_rng(1000 * P + Q + seed)
    slots = np.array([k0, 0, k0 + n - 1], np.int64)
    starts = np.array([0, P, int(rng.integers(3, 9)) * P], np.int64)
    gains = np.array([0.3, -0.2, 0.25], np.float32)
    return slots, starts, gains


@pytest.fixture(scope="module")
def cases():
    """full-scale random int16 rows and the model on them: computed once, read only"""
    out = {}
    for P, Q in RATIOS + [(512, 3)]:
        x = R.random_x(3, N_IN, np.int16, seed=P)
        k, s, g = geometry(P, Q)
        v, tol = R.grid(x, P, Q, k, s, g, out_first=3)
        for a in (x, k, s, g, v, tol):
            a.setflags(write=False)
        out[(P, Q)] = (x, k, s, g, v, tol)
    return out


def test_plans_and_tolerance_constants():
    """the stages run from the front end's last to its first; the tile is the front end's; the rule's factor"""
    want = {6: [2, 3], 10: [2, 5], 12: [4, 3], 30: [2, 3, 5], 50: [2, 5, 5], 90: [2, 3, 3, 5], 150: [2, 3, 5, 5], 486: [2, 3, 3, 3, 3, 3],
            1000: [2, 4, 5, 5, 5], 1024: [4, 4, 4, 4, 4]}
    for M, radices in want.items():
        assert list(reversed(R.plan(M))) == radices and int(np.prod(radices)) == M
    assert [R.tile(P, Q) for P, Q in RATIOS] == [256, 256, 256, 136, 80, 44, 26, 8, 6] and R.tile(512, 3) == 6
    for P, Q in RATIOS:
        assert 8 * 2 * P * (R.tile(P, Q) + 1) <= 61440 and R.tile(P, Q) % 2 == 0
    assert R.A_TOL == 28.0 and R.B_TOL == {2: 6.0, 4: 7.0, 3: 12.0, 5: 18.0}
    assert R.tol_factor(12) == 28 + 7 + 12 and R.tol_factor(1000) == 28 + 6 + 7 + 3 * 18
    # the count of the header: (t + c_R) sqrt 2 with t = 2.92
    for Rr, c in ((2, 1.0), (4, 2.0), (3, 5.1), (5, 9.23)):
        assert (2.92 + c) * np.sqrt(2.0) <= R.B_TOL[Rr]


@pytest.mark.parametrize("P,Q", RATIOS + [(512, 3)], ids=IDS + ["512/3"])
def test_the_plan_run_the_other_way_is_the_dft(P, Q):
    """digit-reversed order in (channelize_grid_ratio_model.rows), natural order out, in float64: numpy's forward transform"""
    M = 2 * P
    rng = np.random.default_rng(M)
    X = rng.standard_normal((4, M)) + 1j * rng.standard_normal((4, M))
    y = np.zeros_like(X)
    y[:, R.rows(M)] = X
    re, im = R.transform_dit(y.real.copy(), y.imag.copy(), M)
    want = np.fft.fft(X, axis=1)
    d = np.abs(re + 1j * im - want).max() / np.abs(want).max()
    print("M %d: the plan run the other way against numpy.fft.fft, worst relative difference %.3g" % (M, d))
    assert d <= 1e-14


@pytest.mark.parametrize("P,Q", RATIOS, ids=IDS)
def test_computed_form_equals_the_definition(cases, P, Q):
    """within a small multiple of 1e-16 S times the number of terms (25 taps, M points of the transform); outputs no row reaches are
    exactly zero in both"""
    x, k, s, g, v, tol = cases[(P, Q)]
    outs = np.arange(len(v)) if len(v) <= 4000 else np.unique(np.concatenate([np.arange(0, len(v), 7), np.arange(len(v) - 40, len(v))]))
    d = R.direct(x, P, Q, k, s, g, outs + 3)
    S, vv = _S(tol, P)[outs], v[outs]
    worst = float(np.max(np.abs(vv - d)[S > 0] / S[S > 0]))
    print("%d/%d: computed form against the definition at %d outputs, worst |difference| / S %.3g" % (P, Q, len(outs), worst))
    assert worst <= 4e-16 * (25 + np.log2(2 * P))
    assert (d[S == 0] == 0).all() and (vv[S == 0] == 0).all()


def test_outputs_no_row_reaches_are_zero():
    x = R.random_x(2, 10, np.int16, seed=1)
    v, tol = R.grid(x, 25, 4, [1, -2], [0, 25 * 40], [0.5, 0.5])
    gap = slice(R.support(0, 10, 25, 4) + 1, 25 * 40)
    assert gap.stop - gap.start > 100 and (v[gap] == 0).all() and (tol[gap] == 0).all() and (tol[:gap.start - 1] > 0).all()


@pytest.mark.parametrize("P,Q", [(3, 1), (5, 2), (6, 1), (15, 2), (25, 4), (45, 16)], ids=["3/1", "5/2", "6/1", "15/2", "25/4", "45/16"])
def test_model_equals_the_ratio_model_at_the_slot_centres(cases, P, Q):
    """section 4.18's model at the centres k rate / 2: the difference is that model's rounding of the phase increment, at most
    2 pi 2^-33 position S (section 4.22 adds the same term), plus float64 noise"""
    x, k, s, g, v, tol = cases[(P, Q)]
    w, _, tie = RS.synthesize(x, P, Q, R.centres(P, Q, 8000, k), s, g, 8000, out_first=3, n_out=len(v))
    S = _S(tol, P)
    m = np.arange(len(v)) + 3
    allowed = (2 * np.pi * 2.0 ** -33 * m + 1e-13) * S
    d = np.abs(v - w)
    print("%d/%d: against the ratio model, worst |difference| %.3g on outputs of magnitude %.2f, worst share of the increment term %.3f"
          % (P, Q, d.max(), np.abs(v).max(), float((d[S > 0] / allowed[S > 0]).max())))
    assert (d <= allowed).all() and (w[S == 0] == 0).all()


@pytest.mark.parametrize("D", [2, 8, 64, 512])
def test_a_power_of_two_is_the_grid_model(D):
    x = R.random_x(3, 30, np.int16, seed=D)
    k, s, g = geometry(D, 1)
    v, tol = R.grid(x, D, 1, k, s, g, out_first=5)
    w, wtol = SG.grid(x, D, k, s, g, out_first=5)
    assert np.array_equal(v, w) and np.array_equal(tol, wtol)


@pytest.mark.parametrize("P,Q", RATIOS + [(512, 3)], ids=IDS + ["512/3"])
def test_fp32_evaluation_stays_inside_the_tolerance(cases, P, Q):
    x, k, s, g, v, tol = cases[(P, Q)]
    got = R.grid_fp32(x, P, Q, k, s, g, out_first=3)
    w = R.worst(got, v, tol)
    print("%d/%d: fp32 evaluation, worst error / tol %.4f" % (P, Q, w))
    assert w <= 0.25, (P, Q, w)
    assert (got[tol == 0] == 0).all()


@pytest.mark.parametrize("variant", [v for v in R.VARIANTS if v not in R.VARIANTS_Q])
@pytest.mark.parametrize("P,Q", [(6, 1), (15, 2)], ids=["6/1", "15/2"])
def test_wrong_variants_are_rejected(cases, P, Q, variant):
    """each wrong model leaves the tolerance somewhere: the rule tells them from the definition"""
    x, k, s, g, v, tol = cases[(P, Q)]
    w = R.worst(R.grid(x, P, Q, k, s, g, out_first=3, variant=variant)[0], v, tol)
    print("%d/%d %s: worst / tol %.3g" % (P, Q, variant, w))
    assert w > 1.0, (P, Q, variant, w)


@pytest.mark.parametrize("variant", R.VARIANTS_Q)
def test_variants_that_are_the_definition_at_q_1(cases, variant):
    """rejected at 15/2; at 6/1 they are the definition itself"""
    x, k, s, g, v, tol = cases[(15, 2)]
    assert R.worst(R.grid(x, 15, 2, k, s, g, out_first=3, variant=variant)[0], v, tol) > 1.0
    x, k, s, g, v, tol = cases[(6, 1)]
    assert np.array_equal(R.grid(x, 6, 1, k, s, g, out_first=3, variant=variant)[0], v)


def test_there_are_at_least_twelve_variants():
    assert len([v for v in R.VARIANTS if v not in R.VARIANTS_Q]) >= 12 and set(R.VARIANTS_Q) <= set(R.VARIANTS)


@pytest.mark.parametrize("P,Q", [(6, 1), (25, 4)], ids=["6/1", "25/4"])
def test_the_model_cuts_into_windows(cases, P, Q):
    x, k, s, g, v, tol = cases[(P, Q)]
    n = len(v)
    for o, m in ((3, 1), (3 + P - 1, P + 1), (3 + 7 * P, 11 * P + 5), (n - 4, 7)):
        pv, pt = R.grid(x, P, Q, k, s, g, out_first=o, n_out=m)
        assert np.allclose(pv, v[o - 3:o - 3 + m], rtol=0, atol=1e-15) and np.array_equal(pt, tol[o - 3:o - 3 + m]), (o, m)
    pv, pt = R.grid(x, P, Q, k, s, g, out_first=3 + n + 30 * P, n_out=9)   # behind every row
    assert (pv == 0).all() and (pt == 0).all()


def _cascade(P, Q, sigma, rho, span):
    """section 4.18's cascade (test_resynthesize_model_cpu.py) for a start of sigma P: the outputs n = rho (mod Q) of the front end
    are x through e[k] = (P / Q) sum_i h_{q_n}[i_n - i] G[(i - sigma P) Q - (n - k) P]"""
    H = RM.taps(P, Q).astype(np.float64)
    G = RS.sequence(P, Q)
    T = H.shape[1]
    n = 1000 * Q + rho
    u = n * P
    i_n, q_n = u // Q, u % Q
    i = i_n - np.arange(T, dtype=np.int64)
    k = np.arange(span, dtype=np.int64)
    tn = (i[:, None] - sigma * P) * Q - (n - k[None, :]) * P
    ok = (tn >= 0) & (tn <= 24 * P)
    return (P / Q) * (H[q_n][:, None] * np.where(ok, G[np.clip(tn, 0, 24 * P)], 0.0)).sum(axis=0)


@pytest.mark.parametrize("P,Q,slot,sigma", [(6, 1, -5, 3), (25, 4, 6, 7), (15, 2, 0, 0), (75, 2, -37, 2)], ids=["6/1", "25/4", "15/2", "75/2"])
def test_round_trip_is_a_delay(P, Q, slot, sigma):
    """a tapered signal band-limited to |f| <= rate / 4 in one slot, through `grid` and then the grid front end's model at the same
    ratio and slot: the input 24 + sigma Q samples late, within section 4.18's bound computed here from the taps and the signal - the
    largest |E_rho(f)| over the band times rms(x), the largest anywhere times the share of x outside the band, and the rounding of
    the capture to fp32 - the worst of the Q residues taken for each (the cascade is periodically time-varying with period Q)"""
    n_in = 600
    rng = np.random.default_rng(P)
    X = np.zeros(n_in, np.complex128)
    kf = np.fft.fftfreq(n_in)
    band = np.abs(kf) <= 0.25 - 4.0 / n_in
    X[band] = rng.standard_normal(band.sum()) + 1j * rng.standard_normal(band.sum())
    x = np.fft.ifft(X)
    x *= np.hanning(n_in + 2)[1:-1] * 0.5 / np.abs(x).max()
    x32 = np.stack([x.real, x.imag], axis=1).astype(np.float32)
    xc = x32[:, 0].astype(np.float64) + 1j * x32[:, 1].astype(np.float64)
    v, _ = R.grid(x32[None], P, Q, [slot], [sigma * P], [1.0])
    cap = np.stack([v.real, v.imag], axis=1).astype(np.float32)
    y, _ = CGR.grid(cap, P, Q, [slot])
    d = 24 + sigma * Q
    want = np.zeros(y.shape[1], np.complex128)
    assert len(want) >= d + n_in                                       # the whole input comes out
    want[d:d + n_in] = xc
    rms = np.sqrt(np.mean(np.abs(want) ** 2))
    err = np.sqrt(np.mean(np.abs(y[0] - want) ** 2)) / rms
    f = np.arange(-2048, 2048) / 4096.0
    in_band, anywhere = 0.0, 0.0
    for rho in range(Q):
        e = _cascade(P, Q, sigma, rho, span=d + 40)
        assert abs(e[0]) < 1e-12 and abs(e[-1]) < 1e-12               # the span holds the whole response
        E = CM.response(e, f) - np.exp(-2j * np.pi * f * d)
        in_band = max(in_band, np.abs(E[np.abs(f) <= 0.25]).max())
        anywhere = max(anywhere, np.abs(E).max())
    Xf = np.abs(np.fft.fft(xc, 1 << 16)) ** 2
    f16 = np.fft.fftfreq(1 << 16)
    out_share = np.sqrt(Xf[np.abs(f16) > 0.25].sum() / Xf.sum())
    rounding = 2.0 ** -24 * 2 * np.abs(RM.taps(P, Q).astype(np.float64)).sum(axis=1).max() * np.abs(v).max() / rms
    bound = in_band + anywhere * out_share + rounding
    print("%d/%d slot %d sigma %d: rms error / rms %.3g, bound %.3g (in band %.3g, out-of-band share %.3g)" % (P, Q, slot, sigma, err, bound, in_band, out_share))
    assert err <= bound, (P, Q, err, bound)
    assert bound < 1e-2                                               # (the bound itself says something)


@pytest.mark.parametrize("P,Q,slots,sigmas", [(6, 1, (-5, 4), (0, 2001)), (25, 4, (-6, 4), (1, 800))], ids=["6/1", "25/4"])
def test_oracle_frames_through_both_models(P, Q, slots, sigmas):
    """one oracle-encoded mode-6 frame per slot (freq_off 0), unequal gains, a noise floor of -60 dB, int16 -> the grid front end's
    model at the same ratio -> the oracle decoder: status 0, the payload, sc_start the frame's own + 24 + sigma Q"""
    gains = (0.3, 0.2)
    pays = [O.payload_for(230 + P + c) for c in range(2)]
    x = np.stack([O.encode_pcm(p, channels=2, freq_off=0, mode=6, rate=8000) for p in pays])
    starts = [sg * P for sg in sigmas]
    v = np.zeros(R.n_outputs(starts, x.shape[1], P, Q), np.complex128)
    for c in range(2):                                                # (row by row: the model's transform of two long rows at once is no faster)
        vc, _ = R.grid(x[c:c + 1], P, Q, [slots[c]], [starts[c]], [gains[c]], n_out=len(v))
        v += vc
    rng = np.random.default_rng(8)
    v = v + 1e-3 * (rng.standard_normal(len(v)) + 1j * rng.standard_normal(len(v)))
    cap = R.quantise(np.stack([v.real, v.imag], axis=1))
    assert np.abs(cap).max() < 32767
    rows = CGR.wide_rows(cap, P, Q, list(slots))
    for c in range(2):
        _, own = O.decode(x[c])
        out, res = O.decode(rows[c])
        assert res.status == 0 and (out == pays[c]).all(), (c, res.status)
        assert abs(res.sc_start - (own.sc_start + 24 + sigmas[c] * Q)) <= 1, (c, res.sc_start, own.sc_start)


def test_model_argument_errors():
    x = R.random_x(2, 10, np.int16)
    ok = dict(P=25, Q=4, slots=[1, -2], starts=[0, 25], gains=[0.5, 0.5])

    def call(**kw):
        a = dict(ok, **kw)
        return R.grid(a.get("x", x), a["P"], a["Q"], a["slots"], a["starts"], a["gains"], a.get("out_first", 0), a.get("n_out"))

    call()
    for bad in (dict(P=50, Q=8), dict(P=7, Q=1), dict(P=3, Q=2), dict(P=513, Q=1), dict(slots=[1, 1]), dict(slots=[1, 7]), dict(slots=[1, -7]),
                dict(starts=[0, 24]), dict(starts=[0, -25]), dict(starts=[0, ((1 << 50) // 25 + 1) * 25]), dict(gains=[0.5, float("nan")]),
                dict(gains=[0.5, 3e38]), dict(slots=[1]), dict(n_out=0), dict(out_first=-1), dict(x=x[:, :, :1]), dict(x=x.astype(np.int32))):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(ValueError):
        R.grid(R.random_x(14, 4, np.int16), 25, 4, list(range(-6, 7)) + [0], [0] * 14, [0.1] * 14)
