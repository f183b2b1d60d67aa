"""The Watterson fading definition held to its statistics, the model's teeth, and what an honest fp32 kernel
can reach on the inputs of test_gpu_fading.py.  No GPU: numpy only."""
import math

import numpy as np
import pytest

import fading_model as FM
import noise_model as NM

N_FRAMES = 4096


@pytest.fixture(scope="module")
def gains_8k():
    """one path of gain 0.6 - 0.5j and the largest spread of an 8 kHz handle, 4096 frames, at knots 0, 5, 12, 25 and 2000"""
    g, spread = 0.6 - 0.5j, 10.0
    knots = np.array([0, 5, 12, 25, 2000])
    G, _ = FM.knot_gains(12345, np.arange(N_FRAMES), [g], [spread], 8000, knots)
    return g, spread, knots, G[:, 0, :]


def test_mean_power_is_the_gains(gains_8k):
    """E |G_t|^2 = |g_t|^2 at every instant, within 5 standard errors of the mean over 4096 independent frames"""
    g, _, knots, G = gains_8k
    want = abs(complex(np.float32(g.real), np.float32(g.imag))) ** 2
    for c in range(len(knots)):
        p = np.abs(G[:, c]) ** 2
        se = p.std(ddof=1) / math.sqrt(N_FRAMES)
        assert abs(p.mean() - want) <= 5.0 * se, (int(knots[c]), p.mean(), want, se)
        assert abs(G[:, c].mean()) <= 5.0 * math.sqrt(want / N_FRAMES)        # zero mean


def test_autocorrelation_is_gaussian(gains_8k):
    """E G(0) conj G(tau) = |g|^2 exp(-2 pi^2 sigma^2 tau^2), sigma = spread / 2 (F.520's frequency spread is 2 sigma), at three lags"""
    g, spread, knots, G = gains_8k
    want0 = abs(complex(np.float32(g.real), np.float32(g.imag))) ** 2
    sigma = spread / 2.0
    for c in (1, 2, 3):
        tau = 32.0 * float(knots[c]) / 8000.0
        want = want0 * math.exp(-2.0 * math.pi ** 2 * sigma ** 2 * tau ** 2)
        prod = G[:, 0] * np.conj(G[:, c])
        se = prod.real.std(ddof=1) / math.sqrt(N_FRAMES)
        assert abs(prod.real.mean() - want) <= 5.0 * se, (tau, prod.real.mean(), want, se)
        assert abs(prod.imag.mean()) <= 5.0 * prod.imag.std(ddof=1) / math.sqrt(N_FRAMES)
    assert 0.75 < math.exp(-2.0 * math.pi ** 2 * sigma ** 2 * (32.0 * 5 / 8000.0) ** 2) < 0.9   # the lags span the curve
    assert math.exp(-2.0 * math.pi ** 2 * sigma ** 2 * (32.0 * 25 / 8000.0) ** 2) < 0.01


def test_rate_enters_the_increment():
    """the same draw at 48 kHz decorrelates over six times as many samples"""
    G8, _ = FM.knot_gains(5, np.arange(256), [1.0], [4.0], 8000, np.array([0, 10]))
    G48, _ = FM.knot_gains(5, np.arange(256), [1.0], [4.0], 48000, np.array([0, 60]))
    assert np.abs(G8 - G48).max() < 1e-4                                       # (the increments' rounding to 2^-32 turns per sample)


WRONG = {
    "key offset": dict(key_offset=NM.KEY_OFFSET),
    "w_f and w_p swapped": dict(swap_words=True),
    "spread taken as sigma": dict(spread_factor=1.0),
    "1 / sqrt K": dict(norm=1.0 / math.sqrt(15.0)),
    "knot 64": dict(knot=64),
    "gain indexed at m - d": dict(gain_index_delayed=True),
    "u2 shift": dict(u2_shift=16),
    "specular path faded": dict(specular_faded=True),
    "first frame ignored": None,
}


@pytest.mark.parametrize("name", list(WRONG))
def test_teeth(name):
    """each wrong variant of the model is rejected by the rule when judged against the right one's output"""
    spf, rate = 700, 8000
    base = FM.inputs(3, spf)
    paths = [(0, 0.55 + 0.3j, 0.0), (40, -0.3 + 0.45j, 10.0), (9, 0.2 - 0.35j, 6.0)]
    v, tol, _ = FM.fading(base, paths, 7, 3, 3, 5, rate)
    got = np.rint(v).astype(np.int16)
    assert NM.accept(NM.explain(got, v, tol))
    if WRONG[name] is None:
        w, wtol, _ = FM.fading(base, paths, 7, 0, 3, 5, rate)
    else:
        w, wtol, _ = FM.fading(base, paths, 7, 3, 3, 5, rate, variant=WRONG[name])
    res = NM.explain(got, w, wtol)
    assert not NM.accept(res) and res.unexplained > 0.05 * res.n, (name, res)


def _fp32_against_model(spf, rate=8000):
    out = []
    for name, paths, (n_in, n_out), first, seed in FM.case_list(spf, rate):
        base = FM.inputs(n_in, spf)
        v, tol, tie = FM.fading(base, paths, seed, first, n_in, n_out, rate)
        assert tie > 1e-6, (spf, name, first, seed, tie)                       # no draw sits on a tie of llrint
        res = NM.explain(FM.evaluate_fp32(base, paths, seed, first, n_in, n_out, rate), v, tol)
        assert res.unexplained == 0, (spf, name, n_in, n_out, first, seed, res)
        out.append(res)
    return out


def test_fp32_evaluation_meets_half_the_cap():
    """the cap is a condition on the inputs: an honest fp32 evaluation of the definition must stay within CAP / 2 on the GPU test's
    own inputs - pooled over the short shapes, per case on the long ones - with nothing unexplained.  Measured shares: see the end
    of fading_model.py's docstring."""
    short = [r for spf in FM.SPF_SHORT for r in _fp32_against_model(spf)]
    pooled = NM.merge(short)
    print("fp32 against the model, short shapes pooled: share %.4f %% worst %.3f of tol" % (100 * NM.share(pooled), pooled.worst))
    assert NM.share(pooled) <= NM.CAP / 2, pooled
    for spf in FM.SPF_LONG + (95200,):
        for res in _fp32_against_model(spf):
            print("fp32 against the model, spf %d: share %.4f %% worst %.3f of tol" % (spf, 100 * NM.share(res), res.worst))
            assert NM.share(res) <= NM.CAP / 2, (spf, res)
    for res in _fp32_against_model(8 * 1024 + 77, 48000)[:2]:
        assert NM.share(res) <= NM.CAP / 2, res
