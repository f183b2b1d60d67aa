"""The device channel models (k_awgn_tile, k_channel of modem_amd/csrc/k_channel.hip) against the float64 model of noise_model.py
and against oracle/channel.c, sample by sample.

Against the model: noise_model.explain -- nothing unexplained, at most 1 % of the samples off rint(v).  Against the oracle the
same two criteria: at most 1 LSB apart, the differing share within the cap.  Shapes are the smallest that reach each code path
(samples_per_frame is a free argument of both entries).  Shapes of a few hundred samples, where one differing sample is already
more than the cap's share, are held to the cap together with the other combinations of the same test case.
"""
import itertools
import math

import numpy as np
import pytest

import noise_model as NM
import oracle_lib as O
from channel_record import record

pytestmark = pytest.mark.gpu

LEVELS = (-40.0, -30.0, -14.6, -6.0, 6.0)
TILINGS = ((1, 1), (1, 5), (3, 7), (5, 5), (5, 2))           # (n_base, n_out)
FIRST = (0, 3, (1 << 32) - 2, 1 << 63)
SEEDS = (0, 1, NM.M64)


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1)
    yield r
    r.close()


@pytest.fixture(scope="module")
def rx48():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1, sample_rate=48000)
    yield r
    r.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _awgn_gpu(rx, d_base, n_base, n_out, spf, db, seed, first):
    import torch
    d_out = torch.full((n_out, spf, 2), 12345, dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()                                                   # the handle has a stream of its own
    rx.awgn_tile(d_base.data_ptr(), n_base, d_out.data_ptr(), n_out, spf, db, seed, first)
    rx.synchronize()
    return d_out


def _awgn_oracle(base, n_out, db, seed, first):
    out = np.empty((n_out,) + base.shape[1:], np.int16)
    for f in range(n_out):
        z = O.pcm_to_cf(base[f % base.shape[0]])
        O.lib().orc_chan_awgn(O.ptr(z), z.shape[0], db, seed, (first + f) & NM.M64)
        out[f] = O.quantise(z, 16, 2)
    return out


def _frame_lengths():
    import modem_amd
    lib = modem_amd.load_library()
    return int(lib.ofdmrx_frame_samples(8000, 6)), int(lib.ofdmrx_frame_samples(48000, 13))


def _combos(spf):
    """short frames (up to 257 samples): the whole cross of tilings, levels, frame indices and seeds, 300 calls of a few samples.
    Longer ones, for the cost of a model evaluation per call: five combinations that rotate through the lists, so that every value
    of every list occurs but NOT every pairing (first_frame 2^32 - 2 with tiling (1, 1), for instance, occurs only in the cross);
    the two whole frames: two calls and one.  Tiling, level and key do not interact with the pass count of the grid-stride loop
    (the key is formed once per frame, the level is one scale), so the pairings are left to the cross at the short lengths."""
    full = list(itertools.product(TILINGS, LEVELS, FIRST, SEEDS))
    if spf <= 257:
        return full
    if spf <= 3 * 16384:
        return [(TILINGS[j % 5], LEVELS[(j + spf) % 5], FIRST[j % 4], SEEDS[j % 3]) for j in range(5)]
    m6, m13 = _frame_lengths()
    if spf == m6:
        return [((3, 7), -14.6, (1 << 32) - 2, 1), ((1, 1), 6.0, 1 << 63, NM.M64)]
    return [((1, 1), -30.0, 3, 0)]                                            # 1 227 840 samples: the largest case


@pytest.mark.parametrize("shape", [1, 255, 256, 257, 16384, 16385, 2 * 16384 + 77, "mode 6 at 8 kHz", "mode 13 at 48 kHz"])
def test_awgn_tile_matches_model_and_oracle(rx, shape):
    """the launch is 64 x 256 threads per frame: 16384 samples a pass.  Only the lengths up to 257 samples run the complete cross of
    tilings x levels x first frames x seeds; the multi-pass lengths run a selection of it (_combos)"""
    spf = shape if isinstance(shape, int) else _frame_lengths()[0 if "mode 6" in shape else 1]
    bases = {nb: NM.base_frames(nb, spf, 40 + nb) for nb in sorted({t[0][0] for t in _combos(spf)})}
    d_bases = {nb: _dev(b) for nb, b in bases.items()}
    vs_model, worst_lsb, differ_orc, total, low, high = [], 0, 0, 0, False, False
    for (n_base, n_out), db, first, seed in _combos(spf):
        got = _awgn_gpu(rx, d_bases[n_base], n_base, n_out, spf, db, seed, first).cpu().numpy()
        v, S = NM.awgn(bases[n_base], db, seed, first, n_base, n_out)
        res = NM.explain(got, v, NM.NOISE_REL * S)
        assert res.unexplained == 0, (spf, n_base, n_out, db, first, seed, res)
        assert got.min() >= -32767, "-32768 left the quantiser"
        low, high = low or int(got.min()) == -32767, high or int(got.max()) == 32767
        ref = _awgn_oracle(bases[n_base], n_out, db, seed, first)
        d = np.abs(got.astype(np.int32) - ref)
        worst_lsb, differ_orc, total = max(worst_lsb, int(d.max())), differ_orc + int((d != 0).sum()), total + d.size
        if spf > 257:
            record("gpu", "awgn spf %d %d->%d %5.1f dB seed %d first %d" % (spf, n_base, n_out, db, seed, first), res)
            assert NM.accept(res), (spf, n_base, n_out, db, first, seed, res)
            assert (d != 0).mean() <= NM.CAP
        vs_model.append(res)
    pooled = NM.merge(vs_model)
    record("gpu", "awgn spf %d, all %d combinations" % (spf, len(vs_model)), pooled)
    assert NM.accept(pooled), pooled
    assert worst_lsb <= 1 and differ_orc <= NM.CAP * total, (worst_lsb, differ_orc, total)
    assert low and high                                                        # both clips occurred


def test_awgn_tile_keying(rx):
    """compared as bytes: the frame index is first_frame + f, the base frame f % n_base, and nothing else enters"""
    import torch
    spf, db = 777, -14.6
    base = NM.base_frames(4, spf, 3)
    d_base = _dev(base)
    whole = _awgn_gpu(rx, d_base, 4, 8, spf, db, 7, 0)
    halves = torch.cat([_awgn_gpu(rx, d_base, 4, 4, spf, db, 7, 0), _awgn_gpu(rx, d_base, 4, 4, spf, db, 7, 4)])
    assert torch.equal(whole, halves)
    assert torch.equal(whole, _awgn_gpu(rx, d_base, 4, 8, spf, db, 7, 0))     # the same call twice
    other = _awgn_gpu(rx, d_base, 4, 8, spf, db, 8, 0)
    assert not torch.equal(whole, other) and (whole != other).float().mean() > 0.9   # seed + 1: other noise everywhere
    assert not torch.equal(whole[:4], whole[4:])                               # the same base frames, other noise
    for n in (4, 3):                                                           # in place, as every sweep uses it (n_out <= n_base)
        d_io = d_base.clone()
        torch.cuda.synchronize()
        rx.awgn_tile(d_io.data_ptr(), 4, d_io.data_ptr(), n, spf, db, 7, 0)
        rx.synchronize()
        assert torch.equal(d_io[:n], whole[:n]) and torch.equal(d_io[n:], d_base[n:])


def test_awgn_tile_refuses_overlap_and_non_finite_levels(rx):
    """only d_out == d_base with n_out <= n_base is in place; every other overlap races (a block reads what another writes)"""
    import torch
    import modem_amd
    spf = 64
    buf = torch.zeros((12, spf, 2), dtype=torch.int16, device="cuda:0")
    before = buf.clone()
    torch.cuda.synchronize()
    p = lambda f: buf[f].data_ptr()
    for base, n_base, out, n_out in ((p(0), 4, p(0), 5),                      # same start, more frames out than in
                                     (p(0), 4, p(1), 4), (p(1), 4, p(0), 4),  # shifted by a frame, either way
                                     (p(0), 4, p(3), 2), (p(3), 2, p(0), 4),  # the last / first frame shared
                                     (p(2), 1, p(0), 8), (p(0), 8, p(2), 1),  # one inside the other
                                     (p(0), 2, buf[1].data_ptr() + 4, 1)):    # off by one sample
        with pytest.raises(modem_amd.OfdmRxError):
            rx.awgn_tile(base, n_base, out, n_out, spf, -20.0, 1, 0)
    for db in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(modem_amd.OfdmRxError):
            rx.awgn_tile(p(0), 4, p(4), 4, spf, db, 1, 0)
    rx.awgn_tile(p(0), 4, p(4), 4, spf, -20.0, 1, 0)                          # adjacent buffers do not overlap
    rx.awgn_tile(p(8), 4, p(8), 3, spf, -20.0, 1, 0)
    rx.synchronize()
    assert torch.equal(buf[:4], before[:4]) and torch.equal(buf[11], before[11])
    assert (buf[4:11] != 0).any(dim=2).any(dim=1).all()


def test_awgn_tile_statistics_on_device_samples(rx):
    """zero base, 32 frames of 65536 samples at -20 dB: the power the level names (plus the quantiser's 1/12 LSB^2) and zero mean,
    within 5 standard deviations of the sampling error"""
    import torch
    n_fr, spf = 32, 65536
    d_base = torch.zeros((1, spf, 2), dtype=torch.int16, device="cuda:0")
    q = _awgn_gpu(rx, d_base, 1, n_fr, spf, -20.0, 21, 0).cpu().numpy().astype(np.float64)
    N = n_fr * spf
    s = 32767.0 * NM.sigma_of(-20.0)
    want = 2.0 * (s * s + 1.0 / 12.0)
    assert abs(2.0 * NM.sigma_of(-20.0) ** 2 / 0.01 - 1.0) < 1e-6
    assert abs((q ** 2).sum(axis=2).mean() / want - 1.0) <= 5.0 / math.sqrt(N)
    for c in range(2):
        assert abs(q[..., c].mean()) <= 5.0 * s / math.sqrt(N)


# ---------------------------------------------------------------- the chain
CHAIN_SPF = (1, 40, 257, 32768 + 300)


def _channel_gpu(rx, d_in, n, spf, kw):
    import torch
    d_out = torch.full((n, spf, 2), 12345, dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    rx.channel(d_in.data_ptr(), d_out.data_ptr(), n, spf, cfo_hz=kw.get("cfo_hz", 0.0), sfo_ppm=kw.get("sfo_ppm", 0.0),
               multipath=kw.get("taps", ()))
    rx.synchronize()
    return d_out


def _chain_case(rx, rate, spf, name, kw, n_frames):
    """one case of the table on n_frames frames of different content: (against the model, LSBs from the oracle, share off the oracle)"""
    import torch
    kw = dict(kw)
    pcm = NM.channel_input(n_frames, spf, 21, kw.pop("full_scale", False))
    d_in = _dev(pcm)
    d_got = _channel_gpu(rx, d_in, n_frames, spf, kw)
    got = d_got.cpu().numpy()
    results, lsb, differ = [], 0, 0
    for f in range(n_frames):
        if n_frames > 1:                                                       # blockIdx.y: each frame as in a call of its own
            assert torch.equal(_channel_gpu(rx, d_in[f:f + 1], 1, spf, kw)[0], d_got[f]), (name, f)
        v, A = NM.chain(pcm[f], rate=rate, **kw)
        res = NM.explain(got[f], v, NM.chain_tol(len(kw.get("taps", ())), A))
        assert res.unexplained == 0, (rate, spf, name, f, res)
        ref = O.impair(pcm[f], noise_db=None, cfo_hz=kw.get("cfo_hz", 0.0), sfo_ppm=kw.get("sfo_ppm", 0.0), multipath=kw.get("taps"), rate=rate)
        d = np.abs(got[f].astype(np.int32) - ref)
        lsb, differ = max(lsb, int(d.max())), differ + int((d != 0).sum())
        results.append(res)
    if name == "pass-through":
        assert (got == np.maximum(pcm, -32767)).all()
    if name == "saturating" and spf >= 40:
        assert (got[..., 0] == 32767).any() and (got[..., 0] == -32767).any() and (got[..., 1] == 32767).any() and (got[..., 1] == -32767).any()
    assert got.min() >= -32767
    res = NM.merge(results)
    record("gpu", "chain %d Hz spf %d x %d: %s" % (rate, spf, n_frames, name), res)
    return res, lsb, differ


def _chain_shape(rx, rate, spf, n_frames, only_cfo=False):
    """the table at one shape.  The long shape is held to the cap case by case, the short ones over the whole table."""
    pooled, differ, total = [], 0, 0
    for name, kw in NM.channel_cases(spf, rate).items():
        if only_cfo and not name.startswith("cfo"):
            continue
        res, lsb, df = _chain_case(rx, rate, spf, name, kw, n_frames)
        assert lsb <= 1, (name, lsb)
        if spf >= 16384:
            assert NM.accept(res), (name, res)
            assert df <= NM.CAP * res.n, (name, df, res.n)
        pooled.append(res)
        differ, total = differ + df, total + res.n
    return NM.merge(pooled), differ, total


@pytest.mark.parametrize("n_frames", [1, 3])
def test_channel_long_shape_matches_model_and_oracle(rx, n_frames):
    """32768 + 300 samples: the launch is 128 x 256 threads per frame, so the last 300 are the loop's second pass; at +-1000 ppm the
    read position drifts 33 samples, off the end for positive ppm and to -1 at the start for negative ppm"""
    res, differ, total = _chain_shape(rx, 8000, CHAIN_SPF[-1], n_frames)
    assert NM.accept(res) and differ <= NM.CAP * total


@pytest.mark.parametrize("n_frames", [1, 3])
def test_channel_short_shapes_match_model_and_oracle(rx, n_frames):
    """1, 40 and 257 samples: the whole resampler window outside the frame, a window longer than the frame, one block and one thread"""
    parts = [_chain_shape(rx, 8000, spf, n_frames) for spf in CHAIN_SPF[:-1]]
    res = NM.merge(p[0] for p in parts)
    assert NM.accept(res), res
    assert sum(p[1] for p in parts) <= NM.CAP * sum(p[2] for p in parts)


def test_channel_cfo_at_another_rate(rx48):
    """the kernel's `rate` argument: the CFO cases on a 48 kHz handle"""
    res, differ, total = _chain_shape(rx48, 48000, CHAIN_SPF[-1], 1, only_cfo=True)
    assert NM.accept(res) and differ <= NM.CAP * total
    parts = [_chain_shape(rx48, 48000, spf, 3, only_cfo=True) for spf in CHAIN_SPF[:-1]]
    res = NM.merge(p[0] for p in parts)
    assert NM.accept(res), res
    assert sum(p[1] for p in parts) <= NM.CAP * sum(p[2] for p in parts)
