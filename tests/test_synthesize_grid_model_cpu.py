"""The grid synthesizer without a GPU: the float64 model of synthesize_grid_model.py - the computed form
against the definition as it stands and against section 4.15's model at the slot centres, the tolerance rule on an fp32 evaluation
and on deliberately wrong models, windows, the round trip through the grid front end's model, and oracle frames through both."""
import numpy as np
import pytest

import channelize_grid_model as CG
import channelize_model as CM
import oracle_lib as O
import synthesize_grid_model as SG
import synthesize_model as SM

N_IN = 40


def _S(tol, D):
    return tol / (2.0 ** -24 * (SG.A_TOL + SG.B_TOL * np.log2(2 * D)))


def geometry(D, Cn, seed=0):
    """random distinct slots (all of them, shuffled, where Cn = M), starts that D divides, random signed gains"""
    rng = np.random.default_rng(1000 * D + seed)
    slots = rng.permutation(np.arange(-D, D))[:Cn].astype(np.int64)
    starts = (rng.integers(0, 30, Cn) * D).astype(np.int64)
    gains = (rng.uniform(0.05, 0.5, Cn) * rng.choice([-1.0, 1.0], Cn)).astype(np.float32)
    return slots, starts, gains


@pytest.fixture(scope="module")
def cases():
    """full-scale random int16 rows in min(M, 24) random slots and the model on them: computed once, read only"""
    out = {}
    for D in SG.ALL_D:
        Cn = min(2 * D, 24)
        x = SG.random_x(Cn, N_IN, np.int16, seed=D)
        k, s, g = geometry(D, Cn)
        v, tol = SG.grid(x, D, k, s, g, out_first=3)
        for a in (x, k, s, g, v, tol):
            a.setflags(write=False)
        out[D] = (x, k, s, g, v, tol)
    return out


@pytest.mark.parametrize("D", [2, 4, 64, 512])
def test_computed_form_equals_the_definition(D):
    """all slots (shuffled), full-scale random int16, signed gains: within 1e-14 S; outputs no row reaches are exactly zero"""
    x = SG.random_x(2 * D, 30, np.int16, seed=D)
    k, s, g = geometry(D, 2 * D, seed=1)
    s[0] += 200 * D                                                  # a gap no row reaches
    v, tol = SG.grid(x, D, k, s, g)
    outs = np.arange(len(v)) if len(v) * 2 * D <= 1 << 21 else np.unique(np.concatenate([np.arange(0, len(v), 37), np.arange(len(v) - 40, len(v))]))
    d = SG.direct(x, D, k, s, g, outs)
    S, v = _S(tol, D)[outs], v[outs]
    assert (S == 0).any() and (v[S == 0] == 0).all() and (d[S == 0] == 0).all()
    worst = float(np.max(np.abs(v - d)[S > 0] / S[S > 0]))
    print("D %d: computed form against the definition at %d outputs, worst |difference| / S %.3g" % (D, len(outs), worst))
    assert worst <= 1e-14


@pytest.mark.parametrize("D", [2, 4, 8, 32])
def test_model_equals_the_plain_model_at_the_slot_centres(D):
    x = SG.random_x(2 * D, 30, np.int16, seed=D + 1)
    k, s, g = geometry(D, 2 * D, seed=2)
    v, tol = SG.grid(x, D, k, s, g)
    w, _, tie = SM.synthesize(x, D, SG.centres(D, 8000, k), s, g, 8000)
    assert tie > 0.49                                                # k 2^32 / M is an integer: no rounding of the increment
    S = _S(tol, D)
    worst = float(np.max(np.abs(v - w)[S > 0] / S[S > 0]))
    print("D %d: grid model against the plain model, worst |difference| / S %.3g" % (D, worst))
    assert worst <= 1e-14 and (w[S == 0] == 0).all() and (v[S == 0] == 0).all()


@pytest.mark.parametrize("D", SG.ALL_D)
def test_fp32_evaluation_stays_inside_a_quarter_of_the_tolerance(cases, D):
    x, k, s, g, v, tol = cases[D]
    got = SG.grid_fp32(x, D, k, s, g, out_first=3)
    w = SG.worst(got, v, tol)
    print("D %d: fp32 evaluation, worst error / tol %.4f" % (D, w))
    assert w <= 0.25, (D, w)
    assert (got[tol == 0] == 0).all()


@pytest.mark.parametrize("D,variant", [(D, v) for v in SG.VARIANTS for D in (2, 64)])
def test_wrong_variants_are_rejected(cases, D, variant):
    """each wrong model leaves the tolerance somewhere: the rule tells them from the definition"""
    x, k, s, g, v, tol = cases[D]
    w = SG.worst(SG.grid(x, D, k, s, g, out_first=3, variant=variant)[0], v, tol)
    print("D %d %s: worst / tol %.3g" % (D, variant, w))
    assert w > 1.0, (D, variant, w)


@pytest.mark.parametrize("D", [2, 64])
def test_the_model_cuts_into_windows(cases, D):
    x, k, s, g, v, tol = cases[D]
    n = len(v)
    for o, m in ((3, 1), (3 + D - 1, D + 1), (3 + 7 * D, 31 * D + 5), (n - 4, 7)):
        pv, pt = SG.grid(x, D, k, s, g, out_first=o, n_out=m)
        assert np.array_equal(pv, v[o - 3:o - 3 + m]) and np.array_equal(pt, tol[o - 3:o - 3 + m]), (o, m)
    pv, pt = SG.grid(x, D, k, s, g, out_first=3 + n + 30 * D, n_out=9)   # behind every row
    assert (pv == 0).all() and (pt == 0).all()


@pytest.mark.parametrize("D", [4, 64])
def test_round_trip_is_a_delay(D):
    """three tapered signals band-limited to |f| <= 0.2 rate in slots that are not adjacent, through `grid` and then the grid front
    end's model at the same slots: row c is its input 24 + sigma_c samples late.  As in section 4.15's test the rms error is held to
    rms(x) times the largest |E(f)| over the band, E the cascade's response minus the delay's, plus the largest |E(f)| anywhere
    times the share of x outside the band, plus the rounding of the capture to fp32 - and, for the other rows, rms(x') times the
    largest response anywhere of the cascade from their slot into this one, g_d[n] = D sum_t h[t] e^{-2 pi i d t / M} h[n D - t],
    d the slots' distance (the sign (-1)^{d n} it comes with has modulus 1): all computed here from the taps and the signals"""
    n_in, M = 1500, 2 * D
    slots = np.array([-D + 1, -1, D - 2] if D > 4 else [-3, 0, 2], np.int64)
    assert np.abs(np.diff(np.sort(slots))).min() >= 2 and (np.sort(slots)[0] + M) - np.sort(slots)[-1] >= 2
    sg = np.array([7, 0, 19], np.int64)
    gains = np.array([1.0, -0.5, 0.7], np.float32)
    rng = np.random.default_rng(D)
    k = np.fft.fftfreq(n_in)
    band = np.abs(k) <= 0.2 - 4.0 / n_in                              # (the taper below widens every line by a bin either side)
    xs = []
    for c in range(3):
        X = np.zeros(n_in, np.complex128)
        X[band] = rng.standard_normal(band.sum()) + 1j * rng.standard_normal(band.sum())
        x = np.fft.ifft(X)
        x *= np.hanning(n_in + 2)[1:-1] * 0.5 / np.abs(x).max()
        xs.append(np.stack([x.real, x.imag], axis=1).astype(np.float32))
    x32 = np.stack(xs)
    v, _ = SG.grid(x32, D, slots, sg * D, gains)
    cap = np.stack([v.real, v.imag], axis=1).astype(np.float32)
    y, _ = CG.grid(cap, D, slots)
    h = CM.taps(D).astype(np.float64)
    t = np.arange(len(h), dtype=np.int64)
    f = np.arange(-2048, 2048) / 4096.0
    g0 = D * np.convolve(h, h)[::D]
    assert len(g0) == 49
    E = CM.response(g0, f) - np.exp(-2j * np.pi * f * 24)
    f16 = np.fft.fftfreq(1 << 16)
    for c in range(3):
        xc = x32[c, :, 0].astype(np.float64) + 1j * x32[c, :, 1].astype(np.float64)
        delay = 24 + int(sg[c])
        want = np.zeros(y.shape[1], np.complex128)
        assert len(want) >= delay + n_in                              # the whole input comes out
        want[delay:delay + n_in] = float(gains[c]) * xc
        rms = np.sqrt(np.mean(np.abs(want) ** 2))
        err = np.sqrt(np.mean(np.abs(y[c] - want) ** 2)) / rms
        Xf = np.abs(np.fft.fft(xc, 1 << 16)) ** 2
        out_share = np.sqrt(Xf[np.abs(f16) > 0.2].sum() / Xf.sum())
        rounding = 2.0 ** -24 * 2 * np.abs(h).sum() * np.abs(v).max() / rms
        cross = 0.0
        for o in range(3):
            if o != c:
                d = int(slots[o] - slots[c])
                gd = D * np.convolve(h * np.exp(-2j * np.pi * ((d * t) % M) / M), h)[::D]
                xo = x32[o, :, 0].astype(np.float64) + 1j * x32[o, :, 1].astype(np.float64)
                Gd = np.exp(-2j * np.pi * np.outer(f, np.arange(len(gd)))) @ gd      # (complex taps: CM.response takes real ones)
                cross += np.abs(Gd).max() * abs(float(gains[o])) * np.sqrt(np.sum(np.abs(xo) ** 2) / len(want)) / rms
        in_band = np.abs(E[np.abs(f) <= 0.2]).max()
        bound = in_band + np.abs(E).max() * out_share + rounding + cross
        print("D %d slot %d: rms error / rms %.3g, bound %.3g (in band %.3g, out-of-band share %.3g, other rows %.3g)"
              % (D, slots[c], err, bound, in_band, out_share, cross))
        assert err <= bound, (D, c, err, bound)
        assert bound < 1e-2                                           # (the bound itself says something)


def test_oracle_frames_through_both_grid_models():
    """two oracle-encoded mode-6 frames (freq_off 0) in slots two apart at D = 8, unequal gains and starts, a noise floor of -60 dB,
    int16: the grid front end's model gives rows the oracle decodes with status 0 and the payload"""
    D, slots, starts, gains = 8, [1, 3], [0, 8 * 1003], [0.3, 0.2]
    pays = [O.payload_for(90 + c) for c in range(2)]
    x = np.stack([O.encode_pcm(p, channels=2, freq_off=0, mode=6, rate=8000) for p in pays])
    v, _ = SG.grid(x, D, slots, starts, gains)
    rng = np.random.default_rng(8)
    v = v + 1e-3 * (rng.standard_normal(len(v)) + 1j * rng.standard_normal(len(v)))
    cap = SG.quantise(np.stack([v.real, v.imag], axis=1))
    assert np.abs(cap).max() < 32767
    rows = CG.rows(cap, D, slots)
    for c in range(2):
        out, res = O.decode(rows[c])
        assert res.status == 0 and (out == pays[c]).all(), (c, res.status)
