"""The Watterson fading channel on the device (k_fading of modem_amd/csrc/k_channel.hip behind ofdmrx_util_fading) against the float64
model of fading_model.py, sample by sample.

The rule is noise_model.explain: nothing unexplained, at most 1 % of the samples off rint(v).  Shapes of a few hundred samples, where
one differing sample is already more than the cap's share, are held to the cap together with the other combinations of the same
shape; the longer shapes case by case.  The inputs are those of fading_model.case_list, on which an fp32 numpy evaluation of the
definition stays within half the cap (test_fading_model_cpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import fading_model as FM
import noise_model as NM

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


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


def _fade(rx, d_in, n_in, n_out, spf, paths, seed, first):
    import torch
    d_out = torch.full((n_out, spf, 2), 12345, dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()                                                   # the handle has a stream of its own
    rx.fading(d_in.data_ptr(), n_in, d_out.data_ptr(), n_out, spf, paths, seed, first)
    rx.synchronize()
    return d_out


def _shape(rx, spf, rate, per_case):
    """every case of fading_model.case_list at one shape; returns the pooled comparison"""
    d_bases, results = {}, []
    for name, paths, (n_in, n_out), first, seed in FM.case_list(spf, rate):
        if n_in not in d_bases:
            d_bases[n_in] = (FM.inputs(n_in, spf), _dev(FM.inputs(n_in, spf)))
        base, d_base = d_bases[n_in]
        got = _fade(rx, d_base, n_in, n_out, spf, paths, seed, first).cpu().numpy()
        v, tol, tie = FM.fading(base, paths, seed, first, n_in, n_out, rate)
        assert tie > 1e-6, (spf, name, first, seed, tie)                       # no draw on a tie of llrint: device and model cannot round apart
        res = NM.explain(got, v, tol)
        print("fading %d Hz spf %d %s %d->%d first %d seed %d: %s share %.4f %%" % (rate, spf, name, n_in, n_out, first, seed, res, 100 * NM.share(res)))
        assert res.unexplained == 0, (spf, name, n_in, n_out, first, seed, res)
        assert got.min() >= -32767, "-32768 left the quantiser"
        if per_case:
            assert NM.accept(res), (spf, name, n_in, n_out, first, seed, res)
        results.append(res)
    pooled = NM.merge(results)
    print("fading %d Hz spf %d, all %d cases: %s share %.4f %%" % (rate, spf, len(results), pooled, 100 * NM.share(pooled)))
    return pooled


@pytest.mark.parametrize("spf", FM.SPF_SHORT)
def test_fading_short_shapes_match_model(rx, spf):
    """1, 31, 32, 33 and 257 samples - less than a knot interval, one, one and a sample, several - with the whole cross of path sets,
    tilings, first frames and seeds, pooled for the cap"""
    pooled = _shape(rx, spf, 8000, per_case=False)
    assert NM.accept(pooled), pooled


@pytest.mark.parametrize("spf", FM.SPF_LONG + ("mode 6 at 8 kHz",))
def test_fading_long_shapes_match_model(rx, spf):
    """the kernel's tile of 4096 samples less one, exactly, plus one, two tiles and 77, and a whole mode-6 frame (24 tiles, the last
    a quarter full) in a single call: every path set with one combination of the rotation, each held to the cap by itself"""
    import modem_amd
    if not isinstance(spf, int):
        spf = int(modem_amd.load_library().ofdmrx_frame_samples(8000, 6))
    assert NM.accept(_shape(rx, spf, 8000, per_case=True))


def test_fading_at_another_rate(rx48):
    """`rate` enters the phase increment (and the largest spread allowed, 60 Hz here)"""
    assert NM.accept(_shape(rx48, 2 * FM.TILE + 77, 48000, per_case=True))
    assert NM.accept(_shape(rx48, 33, 48000, per_case=False))


@pytest.mark.parametrize("spf", [40, 257, 1025])
def test_all_specular_paths_are_the_static_channel(rx, spf):
    """every path specular, the "eight taps" of noise_model.channel_cases: the output is explained by noise_model.chain with
    chain_tol - the existing model judging the new kernel - and at most 1 LSB from ofdmrx_util_channel with the same taps"""
    import torch
    taps = NM.channel_cases(spf)["eight taps"]["taps"]
    paths = [(d, g, 0.0) for d, g in taps]
    n = 3
    pcm = NM.channel_input(n, spf, 21)
    d_in = _dev(pcm)
    got = _fade(rx, d_in, n, n, spf, paths, 5, 9).cpu().numpy()
    d_ref = torch.full((n, spf, 2), 12345, dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    rx.channel(d_in.data_ptr(), d_ref.data_ptr(), n, spf, multipath=taps)
    rx.synchronize()
    lsb, share = NM.lsb_apart(got, d_ref.cpu().numpy())
    assert lsb <= 1 and share <= NM.CAP, (lsb, share)
    results = []
    for f in range(n):
        v, A = NM.chain(pcm[f], taps=taps)
        res = NM.explain(got[f], v, NM.chain_tol(len(taps), A))
        assert res.unexplained == 0, (spf, f, res)
        results.append(res)
    assert NM.accept(NM.merge(results))
    v, tol, _ = FM.fading(pcm, paths, 5, 9, n, n)
    assert NM.accept(NM.explain(got, v, tol))
    assert (_fade(rx, d_in, n, n, spf, paths, 6, 0).cpu().numpy() == got).all()   # no sinusoids: neither seed nor frame enters


def test_fading_keying(rx):
    """compared as bytes: the realisation is keyed by (seed, first_frame + f), the base frame is f % n_in, and nothing else enters"""
    import torch
    spf = FM.TILE + 777
    paths = FM.path_sets(spf)["specular and faded"]
    base = FM.inputs(4, spf)
    d_base = _dev(base)
    whole = _fade(rx, d_base, 4, 8, spf, paths, 7, 0)
    halves = torch.cat([_fade(rx, d_base, 4, 4, spf, paths, 7, 0), _fade(rx, d_base, 4, 4, spf, paths, 7, 4)])
    assert torch.equal(whole, halves)
    assert torch.equal(whole, _fade(rx, d_base, 4, 8, spf, paths, 7, 0))       # the same call twice
    other = _fade(rx, d_base, 4, 8, spf, paths, 8, 0)
    assert (whole != other).any(dim=2).float().mean() > 0.9                    # seed + 1: another channel everywhere
    assert (whole[:4] != whole[4:]).any(dim=2).float().mean() > 0.9            # the same base frames under other fades
    for f in (0, 3, 6):                                                        # a frame alone, or among fewer / other frames
        assert torch.equal(_fade(rx, d_base[f % 4:f % 4 + 1], 1, 1, spf, paths, 7, f)[0], whole[f])
    one = _fade(rx, d_base, 4, 5, spf, paths, 7, 0)
    assert torch.equal(one, whole[:5])                                         # n_out does not enter


def _raw(rx, d_in, n_in, d_out, n_out, spf, fd, seed=1, first=0):
    return rx._lib.ofdmrx_util_fading(rx._h, d_in, n_in, d_out, n_out, spf, fd, seed, first)


def _fd(paths):
    import modem_amd.ofdmrx as M
    fd = M.Fading()
    fd.ntaps = len(paths)
    for i, (d, g, s) in enumerate(paths[:8]):
        fd.delays[i], fd.gains_re[i], fd.gains_im[i], fd.spread_hz[i] = d, complex(g).real, complex(g).imag, s
    return fd


def test_fading_refusals(rx, rx48):
    """every argument the header names is refused with OFDMRX_E_ARG and the output buffer stays as it was; buffers that merely touch
    are accepted"""
    import torch
    spf = 2048
    buf = torch.zeros((12, spf, 2), dtype=torch.int16, device="cuda:0")
    buf[:4] = _dev(FM.inputs(4, spf))
    before = buf.clone()
    torch.cuda.synchronize()
    p = lambda f: buf[f].data_ptr()
    ok = [(0, 0.7 + 0.1j, 1.0), (5, 0.3 - 0.2j, 0.0)]
    good = C.byref(_fd(ok))
    inf, nan = float("inf"), float("nan")
    assert _raw(rx, None, 4, p(4), 4, spf, good) == -1 and _raw(rx, p(0), 4, None, 4, spf, good) == -1      # NULL pointers
    assert _raw(rx, p(0), 4, p(4), 4, spf, None) == -1
    assert _raw(rx, p(0), 0, p(4), 4, spf, good) == -1 and _raw(rx, p(0), 4, p(4), 0, spf, good) == -1      # zero counts
    assert _raw(rx, p(0), 4, p(4), 4, 0, good) == -1
    bad = {
        "no path": [],
        "nine paths": None,
        "negative delay": [(-1, 1.0, 1.0)],
        "delay = spf": [(0, 0.5, 1.0), (spf, 0.5, 1.0)],
        "delay above the limit": [(FM.MAX_DELAY + 1, 1.0, 1.0)],
        "gain nan": [(0, complex(nan, 0.0), 1.0)],
        "gain inf": [(0, complex(0.5, -inf), 1.0)],
        "spread nan": [(0, 1.0, nan)],
        "spread inf": [(0, 1.0, inf)],
        "spread negative": [(0, 1.0, -0.001)],
        "spread above rate / 800": [(0, 1.0, 10.001)],
    }
    for name, paths in bad.items():
        fd = _fd(paths if paths is not None else ok)
        if paths is None:
            fd.ntaps = 9
        assert _raw(rx, p(0), 4, p(4), 4, spf, C.byref(fd)) == -1, name
    assert _raw(rx, p(0), 1, p(4), 1, 700, C.byref(_fd([(700, 1.0, 1.0)]))) == -1                            # delay = spf below the limit
    assert _raw(rx48, p(0), 4, p(4), 4, spf, C.byref(_fd([(0, 1.0, 60.001)]))) == -1                         # the limit follows the rate
    for a, n_in, b, n_out in ((p(0), 4, p(0), 4),                              # the same buffer: there is no in-place form
                              (p(0), 4, p(0), 1), (p(0), 4, p(1), 4), (p(1), 4, p(0), 4),
                              (p(0), 4, p(3), 2), (p(3), 2, p(0), 4), (p(2), 1, p(0), 8), (p(0), 8, p(2), 1),
                              (p(0), 2, buf[1].data_ptr() + 4, 1)):            # off by one sample
        assert _raw(rx, a, n_in, b, n_out, spf, good) == -1, (a - p(0), n_in, b - p(0), n_out)
    assert _raw(rx, p(0), 4, p(4), 1 << 31, 1, good) == -1                     # more frames than the launch holds
    assert _raw(rx, p(0), 1, p(4), 1, 65535 * FM.TILE + 1, good) == -1         # more tiles per frame than the launch holds
    rx.synchronize()
    rx48.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    assert _raw(rx, p(0), 4, p(4), 4, spf, good) == 0                          # adjacent buffers: the input right before the output
    rx.synchronize()
    assert torch.equal(buf[:4], before[:4]) and torch.equal(buf[8:], before[8:])
    assert (buf[4:8] != 0).any(dim=2).any(dim=1).all()
    assert _raw(rx48, p(4), 4, p(0), 4, spf, C.byref(_fd([(0, 1.0, 60.0)]))) == 0   # and right behind it; the largest spread at 48 kHz
    rx48.synchronize()
    assert not torch.equal(buf[:4], before[:4]) and (buf[:4] != 0).any(dim=2).any(dim=1).all() and torch.equal(buf[8:], before[8:])


def test_fading_then_noise_decodes_as_the_oracle_does():
    """four mode-6 frames of tests/golden through watterson("good") and AWGN at -30 dB, all on the device; the receiver and the
    oracle decode the same device-made PCM and must agree on the payload and on every decided field (the parity tests' helper).
    How many of the frames decode is printed, not asserted: nobody has measured that."""
    import torch
    import modem_amd
    import test_gpu_parity as P
    parts = [np.load(os.path.join(HERE, "golden", "base_frames_2ch_%d.npz" % k)) for k in range(2)]
    base = np.concatenate([q["pcm"] for q in parts])
    pays = np.concatenate([q["payload"] for q in parts])
    n, spf = base.shape[0], base.shape[1]
    assert n == 4
    rxp = modem_amd.Receiver(device=0, chunk_frames=64, keep_raw_cons=True)
    try:
        d_base = _dev(base)
        d_pcm = torch.empty_like(d_base)
        torch.cuda.synchronize()
        rxp.fading(d_base.data_ptr(), n, d_pcm.data_ptr(), n, spf, modem_amd.watterson("good", 8000), 2024, 100)
        rxp.awgn_tile(d_pcm.data_ptr(), n, d_pcm.data_ptr(), n, spf, -30.0, 2024, 100)
        rxp.synchronize()
        pcm = d_pcm.cpu().numpy()
        assert not (pcm == base).all()
        decoded = 0
        for f in range(n):
            r, ores = P._check_against_oracle(rxp, pcm[f], pays[f], expect_ok=False)
            ok = int(r["status"]) == 0
            assert not ok or (rxp.decode(pcm[f][None])[0][0] == pays[f]).all()   # a frame that decodes gives its payload
            decoded += ok
        print("watterson good + AWGN -30 dB: %d of %d frames decode" % (decoded, n))
    finally:
        rxp.close()
