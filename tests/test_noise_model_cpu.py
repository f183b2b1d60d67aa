"""The channel models' definition and the oracle's statement of it, on the CPU.

(a) the generator (noise_model.py, a float64 restatement of oracle/channel.c:23-35) against what channel.c says it is: complex
    Gaussian noise of power 10^(LEVEL/10), split equally between re and im, independent from sample to sample, frame to frame and
    seed to seed.  Every statistic is held within 5 standard deviations of its known sampling error; the seeds are fixed, so the
    test is deterministic.
(b) orc_chan_awgn + orc_quantise against the model, sample by sample (noise_model.explain).
(c) orc_chan_multipath / cfo / sfo against noise_model.chain in the same way.
(d) the comparison has teeth: deliberately wrong numpy variants of the model are rejected, by (b)/(c)'s rule or by (a)'s statistics.
"""
import math

import numpy as np
import pytest

import noise_model as NM
import oracle_lib as O
from channel_record import record

N = 1 << 22
SD = 5.0          # every statistic: within 5 standard deviations of its sampling error
KS = 2.7          # D * sqrt(N) of a Kolmogorov-Smirnov test at alpha ~ 1e-6


def _ndtr(x):
    try:
        from scipy.special import ndtr
        return ndtr(x)
    except ImportError:
        import torch
        return torch.special.ndtr(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def gauss_stats(z):
    """z: [n, 2] unit-variance samples.  name -> the statistic in units of its sampling standard deviation (KS: D * sqrt(n))"""
    n = z.shape[0]
    rn = math.sqrt(n)
    out = {}
    for c, name in enumerate(("re", "im")):
        x = z[:, c]
        out["mean " + name] = x.mean() * rn
        out["variance " + name] = ((x * x).mean() - 1.0) / math.sqrt(2.0 / n)
        out["fourth moment " + name] = ((x ** 4).mean() - 3.0) / math.sqrt(96.0 / n)
        cdf = _ndtr(np.sort(x))
        i = np.arange(1, n + 1, dtype=np.float64)
        out["KS " + name] = max((i / n - cdf).max(), (cdf - (i - 1) / n).max()) * rn
    out["re.im"] = (z[:, 0] * z[:, 1]).mean() * rn
    out["total power"] = (0.5 * (z * z).sum(axis=1).mean() - 1.0) * rn
    for lag in range(1, 5):
        for a, an in enumerate(("re", "im")):
            for b, bn in enumerate(("re", "im")):
                out["lag %d %s.%s" % (lag, an, bn)] = (z[:-lag, a] * z[lag:, b]).mean() * rn
    return out


def failures(stats):
    return {k: round(float(v), 2) for k, v in stats.items() if abs(v) > (KS if k.startswith("KS") else SD)}


def unit_noise(n, noise_db, seed, frame=0, sigma_scale=1.0, **variant):
    """the model's unrounded, unclipped noise on a zero base, divided by the TRUE sigma of the level"""
    g, _ = NM.gauss(n, seed, frame, **variant)
    sigma = NM.sigma_of(noise_db)
    return (sigma * sigma_scale) * g / sigma


# ---------------------------------------------------------------- (a) the generator against its definition
def test_sigma_is_the_levels_power_split_in_two():
    for db in (-40.0, -30.0, -14.6, -6.0, 0.0, 6.0):
        assert abs(2.0 * NM.sigma_of(db) ** 2 / 10.0 ** (float(np.float32(db)) / 10.0) - 1.0) < 4 * 2.0 ** -23


def test_uniforms_are_the_codes_fp32_values():
    """the half is rounded away above 2^23 (to even), so u = 1.0 occurs: magnitude 0, not NaN"""
    top = NM.field_to_uniform(np.array([0, 1, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 24) - 1], np.uint64))
    assert list(top * 2.0 ** 24) == [0.5, 1.5, (1 << 23) - 0.5, 1 << 23, (1 << 23) + 2, 1 << 24]
    assert top[-1] == 1.0 and math.sqrt(-2.0 * math.log(top[-1])) == 0.0
    u1, u2 = NM.uniforms(1 << 16, 5, 9)
    assert u1.min() > 0 and u2.min() > 0 and u1.max() <= 1.0 and u2.max() <= 1.0
    # the key schedule, spelt out once in Python integers
    def sm(x):
        x = (x + 0x9E3779B97F4A7C15) & NM.M64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & NM.M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & NM.M64
        return x ^ (x >> 31)
    for seed, frame in ((0, 0), (1, 3), (NM.M64, (1 << 64) - 0x1234567), (99, 1 << 63)):
        key = sm(seed ^ sm((frame + 0x1234567) & NM.M64))
        r = NM.words(5, seed, frame)
        assert [int(x) for x in r] == [sm((key + i) & NM.M64) for i in range(5)]


@pytest.mark.parametrize("noise_db,seed", [(-30.0, 1), (-14.6, 7), (-6.0, 99)])
def test_generator_statistics(noise_db, seed):
    stats = gauss_stats(unit_noise(N, noise_db, seed))
    assert not failures(stats), failures(stats)


def _max_corr(X, Y=None):
    """rows of X (and Y) hold m unit-variance values each.  The dot product of two independent rows is a sum of m products of
    variance 1, so its standard deviation is sqrt(m): dot / sqrt(m) is the pair's correlation coefficient * sqrt(m), in units of
    its own sampling error.  X alone: the largest magnitude over the pairs of different rows; with Y: over row i of X against row i
    of Y."""
    m = X.shape[1]
    c = (X @ X.T)[np.triu_indices(X.shape[0], 1)] if Y is None else (X * Y).sum(axis=1)
    return float(np.abs(c).max()) / math.sqrt(m)


def test_correlation_statistic_has_unit_sampling_error():
    """the normalisation of _max_corr, checked on numpy's own Gaussian rows of the shape the test below uses: over the 2016 pairs
    the statistic's standard deviation is 1 (within 5 of its own sampling errors 1 / sqrt(2 * 2016)), so "<= 5" is a bound of 5
    standard deviations and not of 10"""
    X = np.random.default_rng(1).standard_normal((64, 2 * 65536))
    c = (X @ X.T)[np.triu_indices(64, 1)] / math.sqrt(X.shape[1])
    assert abs(c.std() - 1.0) <= SD / math.sqrt(2.0 * c.size)
    assert _max_corr(X) == float(np.abs(c).max()) and _max_corr(X[:32], X[32:]) == float(np.abs((X[:32] * X[32:]).sum(axis=1)).max()) / math.sqrt(X.shape[1])


def test_frames_and_seeds_are_independent():
    n = 65536
    flat = lambda z: np.concatenate([z[:, 0], z[:, 1]])                       # one row per frame: re | im, 2n values of variance 1
    frames = np.stack([flat(unit_noise(n, -20.0, 11, f)) for f in range(64)])
    worst = {"frames": _max_corr(frames)}                                     # 2016 pairs of frames at one seed
    seeds = np.stack([flat(unit_noise(n, -20.0, 1000 + s, 5)) for s in range(64)])
    worst["seeds"] = _max_corr(seeds)                                         # 64 consecutive seeds at one frame
    a = np.stack([flat(unit_noise(n, -20.0, s, f)) for s in range(8) for f in range(8) if s != f])
    b = np.stack([flat(unit_noise(n, -20.0, f, s)) for s in range(8) for f in range(8) if s != f])
    worst["swapped"] = _max_corr(a, b)                                        # (seed s, frame f) against (seed f, frame s)
    print(worst)
    assert all(w <= SD for w in worst.values()), worst


def test_quantised_noise_keeps_its_variance():
    v, _ = NM.awgn(np.zeros((1, N, 2), np.int16), -30.0, 1)
    q = np.rint(v[0])
    want = (32767.0 * NM.sigma_of(-30.0)) ** 2 + 1.0 / 12.0
    for c in range(2):
        assert abs((q[:, c] ** 2).mean() / want - 1.0) <= SD * math.sqrt(2.0 / N)


def test_clipping_at_0_db():
    v, _ = NM.awgn(np.zeros((1, N, 2), np.int16), 0.0, 3)
    q = np.rint(v[0])
    p = math.erfc(1.0 / (NM.sigma_of(0.0) * math.sqrt(2.0)))
    n = q.size
    assert abs((np.abs(q) == 32767).mean() - p) <= SD * math.sqrt(p * (1 - p) / n)
    assert q.min() == -32767 and q.max() == 32767


# ---------------------------------------------------------------- (b) the oracle's noise against the model
LEVELS_B = (-40.0, -30.0, -20.0, -14.6, -6.0, 0.0, 6.0)
FRAMES_B = (0, 3, (1 << 32) - 1, 1 << 32, 1 << 63)
SEEDS_B = (0, 1, NM.M64)


def oracle_awgn(base, noise_db, seed, frame):
    z = O.pcm_to_cf(base)
    O.lib().orc_chan_awgn(O.ptr(z), z.shape[0], noise_db, seed, frame)
    return O.quantise(z, 16, 2)


@pytest.mark.parametrize("noise_db", LEVELS_B)
def test_oracle_awgn_matches_model(noise_db):
    spf = 8192
    base = NM.base_frames(1, spf, 5)
    for frame in FRAMES_B:
        for seed in SEEDS_B:
            got = oracle_awgn(base[0], noise_db, seed, frame)
            v, S = NM.awgn(base, noise_db, seed, frame)
            res = NM.explain(got, v[0], NM.NOISE_REL * S[0])
            record("oracle", "awgn %5.1f dB seed %d frame %d" % (noise_db, seed, frame), res)
            assert NM.accept(res), (noise_db, seed, frame, res)
            assert got.min() >= -32767


# ---------------------------------------------------------------- (c) the oracle's chain against the model
CHAIN_SPF = (1, 40, 257, 32768 + 300)


def oracle_chain(pcm, kw, rate=8000):
    return O.impair(pcm, noise_db=None, cfo_hz=kw.get("cfo_hz", 0.0), sfo_ppm=kw.get("sfo_ppm", 0.0), multipath=kw.get("taps"), rate=rate)


def chain_case(spf, kw, n=1, seed=21):
    kw = dict(kw)
    pcm = NM.channel_input(n, spf, seed, kw.pop("full_scale", False))
    return pcm, kw


def oracle_chain_results(spf, rate):
    """every case of the table at one frame length: name -> Explained"""
    out = {}
    for name, kw in NM.channel_cases(spf, rate).items():
        if rate != 8000 and not name.startswith("cfo"):
            continue                                                          # the rate enters through the CFO alone
        pcm, kw = chain_case(spf, kw)
        got = oracle_chain(pcm[0], kw, rate)
        v, A = NM.chain(pcm[0], rate=rate, **kw)
        res = NM.explain(got, v, NM.chain_tol(len(kw.get("taps", ())), A))
        record("oracle", "chain %d Hz spf %d: %s" % (rate, spf, name), res)
        assert res.unexplained == 0, (name, res)
        if name == "pass-through":
            assert (got == np.maximum(pcm[0], -32767)).all()
        out[name] = res
    return out


@pytest.mark.parametrize("rate", [8000, 48000])
def test_oracle_chain_matches_model(rate):
    """the long shape case by case; the three short ones (a few hundred samples each, where one differing sample is already more
    than the cap's share) are held to the cap together"""
    for name, res in oracle_chain_results(CHAIN_SPF[-1], rate).items():
        assert NM.accept(res), (name, res)
    short = NM.merge(r for spf in CHAIN_SPF[:-1] for r in oracle_chain_results(spf, rate).values())
    assert NM.accept(short), short


# ---------------------------------------------------------------- (d) the comparison has teeth
def _rejects_awgn(variant, noise_db=-30.0, seed=7, first_frame=3, n_base=3, n_out=7, spf=4096):
    base = NM.base_frames(n_base, spf, 9)
    v, S = NM.awgn(base, noise_db, seed, first_frame, n_base, n_out)
    wrong, _ = NM.awgn(base, noise_db, seed, first_frame, n_base, n_out, variant=variant)
    assert NM.accept(NM.explain(np.rint(v), v, NM.NOISE_REL * S))              # the right model passes its own rule
    return not NM.accept(NM.explain(np.rint(wrong), v, NM.NOISE_REL * S))


@pytest.mark.parametrize("variant", [
    dict(sigma_scale=1.01), dict(ignore_first_frame=True), dict(clamp_base=True), dict(swap=True), dict(u2_shift=16),
    dict(clip_lo=-32768.0 / 32767.0), dict(key_offset=0)], ids=lambda v: next(iter(v)))
def test_sample_comparison_rejects_wrong_noise(variant):
    assert _rejects_awgn(variant)
    # and at the quietest level of the GPU tests, where a wrong sigma moves a sample least
    assert _rejects_awgn(variant, noise_db=-40.0)


@pytest.mark.parametrize("name,variant", [
    ("sfo +1000", dict(k_lo=-NM.HALF)), ("sfo -1000", dict(k_lo=-NM.HALF)), ("cfo +234.567", dict(cfo_sign=-1)),
    ("full chain", dict(cfo_sign=-1)), ("eight taps", dict(delay_sign=-1)), ("full chain", dict(delay_sign=-1))],
    ids=lambda v: v if isinstance(v, str) else next(iter(v)))
def test_sample_comparison_rejects_wrong_chain(name, variant):
    spf = 2048
    pcm, kw = chain_case(spf, NM.channel_cases(spf)[name])
    v, A = NM.chain(pcm[0], **kw)
    wrong, _ = NM.chain(pcm[0], variant=variant, **kw)
    tol = NM.chain_tol(len(kw.get("taps", ())), A)
    assert NM.accept(NM.explain(np.rint(v), v, tol))
    assert not NM.accept(NM.explain(np.rint(wrong), v, tol))


@pytest.mark.parametrize("variant", [dict(sigma_scale=1.01), dict(u2_shift=36)], ids=lambda v: next(iter(v)))
def test_statistics_reject_what_parity_cannot_see(variant):
    """a generator 1 % hot, or one whose angle shares 20 of its 24 bits with the magnitude, would be wrong in the oracle and on the
    device alike: only the definition's statistics see it"""
    assert failures(gauss_stats(unit_noise(N, -14.6, 7, **variant)))
