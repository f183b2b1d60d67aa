"""The wideband bank (ofdmrx_bank_begin_wideband / ofdmrx_bank_push_wideband) on the capture of
wideband_fixture.py: for every channel and any cutting of the capture into pushes, the records equal the stream decode of that
channel's row of ofdmrx_util_channelize over the whole capture - every payload byte, every byte of every result."""
import os
import subprocess
import wave

import numpy as np
import pytest

import oracle_lib as O
import wideband_fixture as WF

pytestmark = pytest.mark.gpu

D = WF.DECIM
CENTRES = np.array(WF.CHANNEL_HZ)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1)
    yield r
    r.close()


@pytest.fixture(scope="module")
def ref(rx):
    """the capture, its channel rows from the device, and their stream decode: computed once, read only"""
    import torch
    pcm, pays = WF.capture()
    n_out = -(-len(pcm) // D)
    d_in = torch.from_numpy(pcm).to("cuda:0")
    d_out = torch.full((len(CENTRES), n_out, 2), 12345.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rx.channelize(d_in.data_ptr(), 0, 0, len(pcm), D, CENTRES, 0, n_out, d_out.data_ptr())
    rx.synchronize()
    rows = d_out.cpu().numpy()
    recs = rx.decode_streams(list(rows))
    for a in (pcm, pays, rows):
        a.setflags(write=False)
    return pcm, pays, rows, recs


def test_channels_decode_the_golden_payloads(ref):
    """(a) every frame from its channel; the channel 4050 Hz above the strong frame: a failed header first, then its frame; the empty
    channel: nothing.  The oracle on the device's own rows agrees in status, payload and sc_start."""
    pcm, pays, rows, recs = ref
    assert [r[2] for r in recs] == [1, 1, 1, 2, 0]
    for c in range(3):
        out, res, _ = recs[c]
        assert int(res[0]["status"]) == 0 and (out[0] == pays[c]).all() and int(res[0]["bit_flips"]) == 0
        assert int(res[0]["sc_start"]) == 9612 + WF.STARTS[c] // D, c                      # the frame's own 9600 + K / D, from its start
    out, res, _ = recs[3]
    assert int(res[0]["status"]) == 6 and abs(float(res[0]["cfo_rad"]) * WF.RATE / (2 * np.pi) - 3950.0) < 1.0
    assert int(res[1]["status"]) == 0 and (out[1] == pays[3]).all() and int(res[1]["sc_start"]) == 9612 + WF.STARTS[3] // D
    assert abs(float(res[1]["cfo_rad"]) * WF.RATE / (2 * np.pi) + 50.0) < 0.5                # tuned 50 Hz above the frame
    for c in range(5):
        out, res, npre = recs[c]
        for k in range(npre + 1):
            o, r = O.decode(rows[c], skip=k)
            if k == npre:
                assert r.status == 1
                break
            assert r.status == int(res[k]["status"]) and (o == out[k]).all() and r.sc_start == int(res[k]["sc_start"]), (c, k)


def _by_channel(parts, n_channels):
    """the tuples Bank.push / end returned, in order -> per channel (payload bytes, result bytes, indices)"""
    pay = np.concatenate([p[0] for p in parts])
    res = np.concatenate([p[1] for p in parts])
    ch = np.concatenate([p[2] for p in parts])
    ix = np.concatenate([p[3] for p in parts])
    return [(pay[ch == c].tobytes(), res[ch == c].tobytes(), list(ix[ch == c])) for c in range(n_channels)]


def _through_bank(rx, pcm, blocks, centres=CENTRES, dtype=np.int16):
    bank = rx.wideband_bank(centres, D, dtype=dtype)
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


@pytest.mark.parametrize("blocks", [(48000, 4097, 1, 0, 5, 7 * 4096 + 3), (1 << 26,)], ids=["blocks", "one push"])
def test_bank_equals_the_one_call_decode(rx, ref, blocks):
    """(b) per channel, byte for byte: payloads and all 56 bytes of every result"""
    pcm, pays, rows, recs = ref
    got = _through_bank(rx, pcm, blocks)
    for c, (out, res, npre) in enumerate(recs):
        assert got[c][2] == list(range(npre)), c
        assert got[c][0] == out.tobytes() and got[c][1] == res.tobytes(), c
        assert res.itemsize == 56


def test_stage_ops_do_not_depend_on_the_channel_count(rx, ref):
    """(c) the pushes before the first preamble: the same launches, copies and synchronisations for one channel and for five"""
    pcm = ref[0]
    ops = {}
    for n in (1, 5):
        bank = rx.wideband_bank(CENTRES[:n], D)
        try:
            ops[n] = []
            for a, b in ((0, 48000), (48000, 52097), (52097, 52097), (52097, 52098)):
                bank.push(pcm[a:b])
                ops[n].append(bank.last_stage_ops)
        finally:
            while bank.open:
                bank.end()
    assert ops[1] == ops[5] and ops[1][0] > 0, ops


def test_plain_and_wideband_entries_refuse_each_other(rx, ref):
    import ctypes as C
    import modem_amd.ofdmrx as M
    pcm = ref[0]
    out, res = np.zeros((4, 5380), np.uint8), np.zeros(4, M.RESULT_DTYPE)
    ch, ix = np.zeros(4, np.int32), np.zeros(4, np.int64)
    a, b = C.c_size_t(0), C.c_size_t(0)
    lens = np.zeros(2, np.uintp)
    p = M._ptr
    L, h = rx._lib, rx._h
    wide = lambda n=0, smp=None: L.ofdmrx_bank_push_wideband(h, smp, n, 0, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b))
    plain = lambda: L.ofdmrx_bank_push(h, None, 0, p(lens), None, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b))
    f = np.array([1000.0, -1000.0])
    assert wide() == -1                                              # no bank open
    assert L.ofdmrx_bank_begin_wideband(h, 2, p(f), D, 3) == -1 and L.ofdmrx_bank_begin_wideband(h, 2, p(f), 33, 0) == -1
    assert L.ofdmrx_bank_begin_wideband(h, 2, None, D, 0) == -1 and L.ofdmrx_bank_begin_wideband(h, 0, p(f), D, 0) == -1
    g = np.array([1000.0, 24000.5])
    assert L.ofdmrx_bank_begin_wideband(h, 2, p(g), D, 0) == -1      # a centre outside +- Rw / 2
    assert L.ofdmrx_bank_begin(h, 2, 2, 2) == 0
    assert wide() == -1 and L.ofdmrx_bank_begin_wideband(h, 2, p(f), D, 0) == -1
    assert L.ofdmrx_bank_end(h, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b)) == 0
    assert L.ofdmrx_bank_begin_wideband(h, 2, p(f), D, 0) == 0
    assert plain() == -1 and L.ofdmrx_bank_begin(h, 2, 2, 2) == -1
    assert wide(10, None) == -1                                      # NULL samples with a length
    blk = np.ascontiguousarray(pcm[:1000])
    assert L.ofdmrx_bank_push_wideband(h, p(blk), 1000, 0, 4, None, p(res), p(ch), p(ix), C.byref(a), C.byref(b)) == -1
    assert wide(1000, p(blk)) == 0 and L.ofdmrx_bank_resident_samples(h, 1) == 167       # ceil(1000 / 6)
    assert L.ofdmrx_bank_push_wideband(h, p(blk), 5, 1, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b)) == 0   # ... and the end
    assert wide(5, p(blk)) == -1                                     # samples after the end
    assert L.ofdmrx_bank_end(h, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b)) == 0 and b.value == 0


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_other_formats_decode_the_same_payloads(rx, ref, dtype):
    """(d) the capture as U8 and as F32"""
    pcm, pays, rows, recs = ref
    x = pcm.astype(np.float64) / 32767.0
    cap = (np.rint(x * 127.0) + 128).astype(np.uint8) if dtype == np.uint8 else x.astype(np.float32)
    got = _through_bank(rx, cap, (200000,), dtype=dtype)
    import modem_amd.ofdmrx as M
    for c in range(4):
        out = np.frombuffer(got[c][0], np.uint8).reshape(-1, 5380)
        ok = np.frombuffer(got[c][1], M.RESULT_DTYPE)["status"] == 0
        assert ok.sum() == 1 and (out[ok][0] == pays[c]).all(), c
    assert got[4][2] == []


def test_command_line(ref, tmp_path):
    """(e) decode_stream --wideband writes the .dat files of (a)"""
    pcm, pays, rows, recs = ref
    wav = tmp_path / "wide.wav"
    with wave.open(str(wav), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(D * WF.RATE)
        w.writeframes(pcm.tobytes())
    exe = os.path.join(ROOT, "modem_amd", "bin", "decode_stream")
    root = tmp_path / "out"
    p = subprocess.run([exe, "--wideband", str(D), ",".join("%g" % f for f in CENTRES), str(root), str(wav)], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    lines = [l for l in p.stderr.splitlines() if ": sample " in l]
    assert len(lines) == sum(r[2] for r in recs)
    for c, (out, res, npre) in enumerate(recs):
        assert sorted(os.listdir(root / str(c))) == sorted("%d.dat" % k for k in range(npre))
        for k in range(npre):
            assert (root / str(c) / ("%d.dat" % k)).read_bytes() == out[k].tobytes(), (c, k)
            assert any(l.startswith("%d:%d: sample %d " % (c, k, int(res[k]["sc_start"]))) for l in lines), (c, k)
    bad = tmp_path / "bad.wav"
    with wave.open(str(bad), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(50000)
        w.writeframes(pcm[:100].tobytes())
    p = subprocess.run([exe, "--wideband", str(D), "0", str(tmp_path / "o2"), str(bad)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "Unsupported sample rate." in p.stderr
