"""The wideband bank for a real capture (ofdmrx_bank_begin_wideband_real / ofdmrx_bank_push_wideband) on the
two captures of wideband_real_fixture.py: for every channel and any cutting of the capture into pushes, the records equal the stream
decode of that channel's row of ofdmrx_util_channelize_real over the whole capture - every payload byte, every byte of every result
- and the oracle agrees on those rows.  Then the command line: decode_stream --wideband-real."""
import ctypes as C
import os
import subprocess
import wave

import numpy as np
import pytest

import oracle_lib as O
import wideband_real_fixture as XF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "modem_amd", "bin", "decode_stream")
CASES = {"48k": (XF.DECIM48, np.array(XF.CHANNEL48_HZ)), "50k": ((XF.P50, XF.Q50), np.array(XF.CHANNEL50_HZ))}


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1)
    yield r
    r.close()


@pytest.fixture(scope="module")
def refs(rx):
    """per capture: the samples, the payloads, the channel rows from the device and their stream decode: computed once, read only"""
    import torch
    out = {}
    for name, (decim, centres) in CASES.items():
        pcm, pays = XF.capture48() if name == "48k" else XF.capture50()
        p, q = (decim, 1) if isinstance(decim, int) else decim
        n_out = -(-len(pcm) * q // p)
        d_in = torch.from_numpy(pcm).to("cuda:0")
        d_out = torch.full((len(centres), n_out, 2), 12345.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        rx.channelize_real(d_in.data_ptr(), 0, 0, len(pcm), decim, centres, 0, n_out, d_out.data_ptr())
        rx.synchronize()
        rows = d_out.cpu().numpy()
        recs = rx.decode_streams(list(rows))
        for a in (pcm, pays, rows):
            a.setflags(write=False)
        out[name] = (pcm, pays, rows, recs)
    return out


def _hz(res, k):
    return float(res[k]["cfo_rad"]) * XF.RATE / (2 * np.pi)


def _oracle_agrees(rows, recs):
    for c, (out, res, npre) in enumerate(recs):
        for k in range(npre + 1):
            o, r = O.decode(rows[c], skip=k)
            if k == npre:
                assert r.status == 1, c
                break
            assert r.status == int(res[k]["status"]) and (o == out[k]).all() and r.sc_start == int(res[k]["sc_start"]), (c, k)


def test_the_48_khz_capture_decodes(refs):
    """every frame from its channel; the channel 4050 Hz above the strong frame: a failed header first, then its frame; the empty
    channel and the mirror of the first frame: nothing.  The oracle on the device's own rows agrees in status, payload and sc_start"""
    pcm, pays, rows, recs = refs["48k"]
    assert [r[2] for r in recs] == [1, 1, 1, 2, 0, 0]
    for c in range(3):
        out, res, _ = recs[c]
        assert int(res[0]["status"]) == 0 and (out[0] == pays[c]).all() and int(res[0]["bit_flips"]) == 0
        assert int(res[0]["sc_start"]) == XF.SC_START48[c], c
    out, res, _ = recs[3]
    assert int(res[0]["status"]) == 6 and abs(_hz(res, 0) - 3950.0) < 1.0
    assert int(res[1]["status"]) == 0 and (out[1] == pays[3]).all() and int(res[1]["bit_flips"]) == 0
    assert int(res[1]["sc_start"]) == XF.SC_START48[3] and abs(_hz(res, 1) + 50.0) < 0.5
    assert XF.SC_START48 == (9612, 17613, 25615, 33613)
    _oracle_agrees(rows, recs)


def test_the_50_khz_capture_decodes(refs):
    pcm, pays, rows, recs = refs["50k"]
    assert [r[2] for r in recs] == [1, 1, 0, 0]
    for c in range(2):
        out, res, _ = recs[c]
        assert int(res[0]["status"]) == 0 and (out[0] == pays[c]).all() and int(res[0]["bit_flips"]) == 0
        assert int(res[0]["sc_start"]) == XF.SC_START50[c], c
    assert XF.SC_START50 == (9612, 17615)
    _oracle_agrees(rows, recs)


def _by_channel(parts, n_channels):
    """the tuples push / end returned, in order -> per channel (payload bytes, result bytes, indices)"""
    pay = np.concatenate([p[0] for p in parts])
    res = np.concatenate([p[1] for p in parts])
    ch = np.concatenate([p[2] for p in parts])
    ix = np.concatenate([p[3] for p in parts])
    return [(pay[ch == c].tobytes(), res[ch == c].tobytes(), list(ix[ch == c])) for c in range(n_channels)]


def _through_bank(rx, pcm, blocks, decim, centres, dtype=np.int16):
    bank = rx.wideband_real_bank(centres, decim, dtype=dtype)
    parts, at, i = [], 0, 0
    try:
        while at < len(pcm):
            n = min(blocks[i % len(blocks)], len(pcm) - at)
            parts.append(bank.push(pcm[at:at + n]))
            at += n
            i += 1
        assert bank.resident_samples(0) > 0
        parts.append(bank.end())
    finally:
        while bank.open:
            bank.end()
    return _by_channel(parts, len(centres))


# one push; blocks of one wideband second; blocks of a prime length; a block shorter than T - 1 (144 and 150 samples) between long ones,
# an empty one and a single sample
CUTTINGS = {"one push": (1 << 26,), "one second": None, "prime": (65537,), "short": (70001, 100, 0, 1)}


@pytest.mark.parametrize("cut", list(CUTTINGS))
@pytest.mark.parametrize("name", list(CASES))
def test_bank_equals_the_one_call_decode(rx, refs, name, cut):
    """per channel, byte for byte: payloads and all 56 bytes of every result"""
    decim, centres = CASES[name]
    pcm, pays, rows, recs = refs[name]
    blocks = CUTTINGS[cut] or ((48000,) if name == "48k" else (50000,))
    got = _through_bank(rx, pcm, blocks, decim, centres)
    for c, (out, res, npre) in enumerate(recs):
        assert got[c][2] == list(range(npre)), c
        assert got[c][0] == out.tobytes() and got[c][1] == res.tobytes(), c
        assert res.itemsize == 56


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_other_formats_decode_the_same_payloads(rx, refs, dtype):
    """the 48 kHz capture as U8 and as F32"""
    import modem_amd.ofdmrx as M
    decim, centres = CASES["48k"]
    pcm, pays, rows, recs = refs["48k"]
    x = pcm.astype(np.float64) / 32767.0
    cap = (np.rint(x * 127.0) + 128).astype(np.uint8) if dtype == np.uint8 else x.astype(np.float32)
    got = _through_bank(rx, cap, (200000,), decim, centres, dtype=dtype)
    for c in range(4):
        out = np.frombuffer(got[c][0], np.uint8).reshape(-1, 5380)
        ok = np.frombuffer(got[c][1], M.RESULT_DTYPE)["status"] == 0
        assert ok.sum() == 1 and (out[ok][0] == pays[c]).all(), c
    assert got[4][2] == [] and got[5][2] == []


@pytest.mark.parametrize("name", list(CASES))
def test_stage_ops_do_not_depend_on_the_channel_count(rx, refs, name):
    """the pushes before the first preamble: the same launches, copies and synchronisations for one channel and for all of them -
    one copy and one launch of the front end per push"""
    decim, centres = CASES[name]
    pcm = refs[name][0]
    ops = {}
    for n in (1, len(centres)):
        bank = rx.wideband_real_bank(centres[:n], decim)
        try:
            ops[n] = []
            for a, b in ((0, 48000), (48000, 52097), (52097, 52097), (52097, 52098)):
                bank.push(pcm[a:b])
                ops[n].append(bank.last_stage_ops)
        finally:
            while bank.open:
                bank.end()
    assert ops[1] == ops[len(centres)] and ops[1][0] > 0, ops


def test_the_banks_refuse_each_other(rx, refs):
    """the plain, the wideband and the real wideband begins and pushes; the real bank counts samples, not pairs"""
    import modem_amd.ofdmrx as M
    pcm = refs["48k"][0]
    D = XF.DECIM48
    out, res = np.zeros((4, 5380), np.uint8), np.zeros(4, M.RESULT_DTYPE)
    ch, ix = np.zeros(4, np.int32), np.zeros(4, np.int64)
    a, b = C.c_size_t(0), C.c_size_t(0)
    lens = np.zeros(2, np.uintp)
    p = M._ptr
    L, h = rx._lib, rx._h
    wide = lambda n=0, smp=None: L.ofdmrx_bank_push_wideband(h, smp, n, 0, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b))
    plain = lambda: L.ofdmrx_bank_push(h, None, 0, p(lens), None, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b))
    end = lambda: L.ofdmrx_bank_end(h, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b))
    f = np.array([3000.0, -17000.0])
    real = lambda g=f, pp=D, q=1, fmt=0, n=2: L.ofdmrx_bank_begin_wideband_real(h, n, None if g is None else p(g), pp, q, fmt)
    assert wide() == -1                                              # no bank open
    assert real(fmt=3) == -1 and real(pp=33) == -1 and real(g=None) == -1 and real(n=0) == -1
    for bad in (1000.0, -1999.9, 22000.5, 24000.0, float("nan")):   # the centre rule: 2000 <= |f| <= 22000 at 48 kHz
        assert real(g=np.array([3000.0, bad])) == -1, bad
    assert L.ofdmrx_bank_begin_wideband(h, 2, p(np.array([3000.0, 1000.0])), D, 0) == 0   # (the analytic bank takes 1000 Hz)
    assert real() == -1 and plain() == -1
    assert end() == 0
    assert L.ofdmrx_bank_begin(h, 2, 2, 2) == 0
    assert wide() == -1 and real() == -1
    assert end() == 0
    assert real(g=np.array([2000.0, -22000.0])) == 0                 # both edges, admitted
    assert plain() == -1 and L.ofdmrx_bank_begin(h, 2, 2, 2) == -1 and real() == -1
    assert L.ofdmrx_bank_begin_wideband(h, 2, p(f), D, 0) == -1 and L.ofdmrx_bank_begin_wideband_ratio(h, 2, p(f), 25, 4, 0) == -1
    assert wide(10, None) == -1                                      # NULL samples with a length
    blk = np.ascontiguousarray(pcm[:1000])
    assert wide(5, C.c_void_p(blk.ctypes.data + 1)) == -1            # off the sample's boundary
    assert L.ofdmrx_bank_push_wideband(h, p(blk), 1000, 0, 4, None, p(res), p(ch), p(ix), C.byref(a), C.byref(b)) == -1
    assert wide(1000, p(blk)) == 0 and L.ofdmrx_bank_resident_samples(h, 1) == 167       # ceil(1000 / 6): 1000 SAMPLES, 2000 bytes
    assert L.ofdmrx_bank_push_wideband(h, p(blk), 5, 1, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b)) == 0   # ... and the end
    assert wide(5, p(blk)) == -1                                     # samples after the end
    assert end() == 0 and b.value == 0


def _write_wav(path, pcm, channels, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(pcm).tobytes())


@pytest.mark.parametrize("name", list(CASES))
def test_command_line(refs, tmp_path, name):
    """decode_stream --wideband-real on the capture as a one-channel WAV writes the files and lines of the Python path"""
    decim, centres = CASES[name]
    pcm, pays, rows, recs = refs[name]
    spelled, rate = ("6", 48000) if name == "48k" else ("25/4", 50000)
    wav = tmp_path / "mono.wav"
    _write_wav(wav, pcm, 1, rate)
    root = tmp_path / "out"
    p = subprocess.run([EXE, "--wideband-real", spelled, ",".join("%g" % f for f in centres), str(root), str(wav)], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    lines = [l for l in p.stderr.splitlines() if ": sample " in l]
    assert len(lines) == sum(r[2] for r in recs)
    for c, (out, res, npre) in enumerate(recs):
        assert sorted(os.listdir(root / str(c))) == sorted("%d.dat" % k for k in range(npre))
        for k in range(npre):
            assert (root / str(c) / ("%d.dat" % k)).read_bytes() == out[k].tobytes(), (c, k)
            assert any(l.startswith("%d:%d: sample %d " % (c, k, int(res[k]["sc_start"]))) for l in lines), (c, k)


def test_command_line_refusals(refs, tmp_path):
    """a two-channel file under --wideband-real (the message names --wideband), `auto` under it, a centre inside rate / 4 - and the
    --wideband forms keep turning a one-channel file away with their own message"""
    pcm = refs["48k"][0]
    mono, two = tmp_path / "mono.wav", tmp_path / "two.wav"
    _write_wav(mono, pcm[:4800], 1, 48000)
    _write_wav(two, np.stack([pcm[:4800], pcm[:4800]], axis=1), 2, 48000)
    run = lambda *argv: subprocess.run([EXE] + list(argv), capture_output=True, text=True, timeout=60)
    p = run("--wideband-real", "6", "3000", str(tmp_path / "o1"), str(two))
    assert p.returncode == 1 and "--wideband" in p.stderr.replace("--wideband-real", "") and "one channel" in p.stderr
    p = run("--wideband-real", "6", "auto", str(tmp_path / "o2"), str(mono))
    assert p.returncode == 1 and "survey of a real capture is not built" in p.stderr
    p = run("--wideband-real", "6", "3000,1000", str(tmp_path / "o3"), str(mono))
    assert p.returncode == 1 and "ofdmrx_bank" in p.stderr
    for form in (("--wideband", "6", "3000"), ("--wideband", "6", "auto"), ("--grid", "8", "all")):
        p = run(*form, str(tmp_path / "o4"), str(mono))
        assert p.returncode == 1 and "A wideband capture is an analytic signal (two channels)." in p.stderr, form
    assert not any(os.path.exists(tmp_path / d / "0" / "0.dat") for d in ("o1", "o2", "o3", "o4"))
