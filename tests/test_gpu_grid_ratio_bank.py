"""The grid bank at a ratio (ofdmrx_bank_begin_wideband_grid_ratio / ofdmrx_bank_push_wideband) on the
captures of grid_ratio_fixture.py: for every slot and any cutting of the capture into pushes, the records equal the stream decode of
that slot's row of ofdmrx_util_channelize_grid_ratio over the whole capture - every payload byte, every byte of every result - and
they are the records test_channelize_grid_ratio_model_cpu.py found with the oracle on the float64 model's rows."""
import ctypes as C
import os
import subprocess
import wave

import numpy as np
import pytest

import grid_ratio_fixture as GF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTTINGS = {"a": [(1 << 26,), (48000,), (40009, 0)], "b": [(1 << 26,), (50000,), (40009, 0)], "c": [(1 << 26,), (300000,), (1000003, 0)]}


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1)
    yield r
    r.close()


@pytest.fixture(scope="module")
def refs(rx):
    """per capture: the capture, its slot rows from the device, and their stream decode: computed once, read only"""
    import torch
    out = {}
    for name, cfg in GF.CONFIGS.items():
        pcm, pays = GF.capture(cfg)
        P, Q, slots = cfg["P"], cfg["Q"], list(cfg["open"])
        n_out = -(-len(pcm) * Q // P)
        d_in = torch.from_numpy(pcm).to("cuda:0")
        d_out = torch.full((len(slots), n_out, 2), 12345.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        rx.channelize_grid(d_in.data_ptr(), 0, 0, len(pcm), (P, Q), slots, 0, n_out, d_out.data_ptr())
        rx.synchronize()
        rows = d_out.cpu().numpy()
        recs = rx.decode_streams(list(rows))
        for a in (pcm, pays, rows):
            a.setflags(write=False)
        out[name] = (pcm, pays, rows, recs)
    return out


def _table(rec, pays):
    out, res, npre = rec
    assert len(res) == npre
    return [(int(res[k]["status"]), ([j for j in range(len(pays)) if (out[k] == pays[j]).all()] + [None])[0], int(res[k]["sc_start"]))
            for k in range(npre)]


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_slots_decode_the_golden_payloads(refs, name):
    """every slot's records are the table of the fixture, which the oracle gave on the model's rows; a decoded frame stands at its
    own sc_start with no flipped bit"""
    cfg, want = GF.CONFIGS[name], GF.EXPECTED[name]
    pcm, pays, rows, recs = refs[name]
    for i, k in enumerate(cfg["open"]):
        assert _table(recs[i], pays) == want[k], k
        out, res, npre = recs[i]
        for j, (status, frame, sc) in enumerate(want[k]):
            if status == 0:
                assert sc == GF.sc_start(cfg, frame) and int(res[j]["bit_flips"]) == 0 and (out[j] == pays[frame]).all(), (k, j)


def _by_channel(parts, n_channels):
    """the tuples push / end returned, in order -> per channel (payload bytes, result bytes, indices)"""
    pay = np.concatenate([p[0] for p in parts])
    res = np.concatenate([p[1] for p in parts])
    ch = np.concatenate([p[2] for p in parts])
    ix = np.concatenate([p[3] for p in parts])
    return [(pay[ch == c].tobytes(), res[ch == c].tobytes(), list(ix[ch == c])) for c in range(n_channels)]


def _push_all(bank, pcm, blocks):
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
    return _by_channel(parts, bank.n_channels)


@pytest.mark.parametrize("name,cut", [(n, c) for n in ("a", "b", "c") for c in range(3)])
def test_bank_equals_the_one_call_decode(rx, refs, name, cut):
    """one push, pushes of one wideband second, odd pushes with empty ones between: per slot byte for byte, payloads and all 56
    bytes of every result"""
    cfg = GF.CONFIGS[name]
    pcm, pays, rows, recs = refs[name]
    got = _push_all(rx.wideband_grid_bank(list(cfg["open"]), (cfg["P"], cfg["Q"])), pcm, CUTTINGS[name][cut])
    for c, (out, res, npre) in enumerate(recs):
        assert got[c][2] == list(range(npre)), c
        assert got[c][0] == out.tobytes() and got[c][1] == res.tobytes(), c
        assert res.itemsize == 56


def test_b_plain_ratio_bank_finds_the_same_frames(rx, refs):
    """25/4: a plain ratio bank at the same centres: record for record equal payload, status and sc_start (the sample bytes differ
    within the tolerances, so the float fields of the results may)"""
    import modem_amd
    import modem_amd.ofdmrx as M
    cfg = GF.B
    pcm, pays, rows, recs = refs["b"]
    f = modem_amd.grid_centres((cfg["P"], cfg["Q"]), GF.RATE, cfg["open"])
    got = _push_all(rx.wideband_bank(f, (cfg["P"], cfg["Q"])), pcm, (1 << 26,))
    for c, k in enumerate(cfg["open"]):
        out, res, npre = recs[c]
        p = np.frombuffer(got[c][0], np.uint8).reshape(-1, 5380)
        r = np.frombuffer(got[c][1], M.RESULT_DTYPE)
        assert len(r) == npre == 1
        assert (p == out).all() and (r["status"] == res["status"]).all() and (r["sc_start"] == res["sc_start"]).all(), k


def test_stage_ops_do_not_depend_on_the_slot_count(rx, refs):
    """the pushes before the first preamble: the same launches, copies and synchronisations for one slot and for all thirteen"""
    pcm = refs["b"][0]
    ops = {}
    for slots in ([3], None):
        bank = rx.wideband_grid_bank(slots, (25, 4))
        try:
            n = bank.n_channels
            ops[n] = []
            for a, b in ((0, 50000), (50000, 54097), (54097, 54097), (54097, 54098)):
                bank.push(pcm[a:b])
                ops[n].append(bank.last_stage_ops)
        finally:
            while bank.open:
                bank.end()
    assert ops[1] == ops[13] and ops[1][0] > 0, ops


def test_refusals_with_an_open_bank(rx, refs):
    import torch
    import modem_amd.ofdmrx as M
    pcm = refs["b"][0]
    out, res = np.zeros((4, 5380), np.uint8), np.zeros(4, M.RESULT_DTYPE)
    ch, ix = np.zeros(4, np.int32), np.zeros(4, np.int64)
    a, b = C.c_size_t(0), C.c_size_t(0)
    p = M._ptr
    L, h = rx._lib, rx._h
    wide = lambda n=0, smp=None: L.ofdmrx_bank_push_wideband(h, smp, n, 0, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b))
    k = np.array([3, -6], np.int32)
    f = np.array([1000.0, -1000.0])
    begin = L.ofdmrx_bank_begin_wideband_grid_ratio
    assert wide() == -1                                              # no bank open
    assert begin(h, 2, p(k), 25, 4, 3) == -1 and begin(h, 2, p(k), 7, 1, 0) == -1 and begin(h, 2, p(k), 3, 2, 0) == -1
    assert begin(h, 2, p(k), 513, 1, 0) == -1 and begin(h, 2, p(k), 36, 17, 0) == -1 and begin(h, 2, p(k), 511, 16, 0) == -1
    assert begin(h, 0, p(k), 25, 4, 0) == -1 and begin(h, 2, None, 25, 4, 0) == -1 and begin(h, 12, None, 25, 4, 0) == -1
    assert begin(h, 2, p(np.array([3, 7], np.int32)), 25, 4, 0) == -1 and begin(h, 2, p(np.array([-7, 3], np.int32)), 25, 4, 0) == -1
    assert begin(h, 2, p(k), 25, 4, 0) == 0
    assert begin(h, 2, p(k), 25, 4, 0) == -1 and L.ofdmrx_bank_begin_wideband_grid(h, 2, p(k), 8, 0) == -1
    # the front-end entries while the bank owns the device tables
    d_in = torch.from_numpy(np.array(pcm[:4096])).to("cuda:0")
    d_out = torch.full((2, 512, 2), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert L.ofdmrx_util_channelize_grid_ratio(h, d_in.data_ptr(), 0, 0, 4096, 25, 4, p(k), 2, 0, 512, d_out.data_ptr(), 512) == -1
    assert L.ofdmrx_util_channelize_ratio(h, d_in.data_ptr(), 0, 0, 4096, 25, 4, p(f), 2, 0, 512, d_out.data_ptr(), 512) == -1
    rx.synchronize()
    assert bool((d_out == 7.0).all())
    blk = np.ascontiguousarray(pcm[:1001])
    assert wide(1001, p(blk)) == 0 and L.ofdmrx_bank_resident_samples(h, 1) == 161       # ceil(1001 x 4 / 25)
    assert L.ofdmrx_bank_end(h, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b)) == 0 and b.value == 0
    assert begin(h, 13, None, 50, 8, 0) == 0                         # NULL slots with n_all; the ratio is reduced
    assert L.ofdmrx_bank_end(h, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b)) == 0
    assert L.ofdmrx_util_channelize_grid_ratio(h, d_in.data_ptr(), 0, 0, 4096, 25, 4, p(k), 2, 0, 512, d_out.data_ptr(), 512) == 0   # closed: served again
    rx.synchronize()
    assert not bool((d_out == 7.0).any())


def test_command_line(refs, tmp_path):
    """decode_stream --grid 25/4 all writes the .dat files of (b) and names every slot's centre; what is not built is refused"""
    pcm, pays, rows, recs = refs["b"]
    wav = tmp_path / "wide.wav"
    with wave.open(str(wav), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(50000)
        w.writeframes(pcm.tobytes())
    exe = os.path.join(ROOT, "modem_amd", "bin", "decode_stream")
    root = tmp_path / "out"
    p = subprocess.run([exe, "--grid", "25/4", "all", str(root), str(wav)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    for i, k in enumerate(range(-6, 7)):
        assert "%d: slot %d, centre %.17g Hz" % (i, k, k * 4000.0) in p.stderr.splitlines()
    want = {k + 6: recs[c] for c, k in enumerate(GF.B["open"])}
    lines = [l for l in p.stderr.splitlines() if ": sample " in l]
    for c in range(13):
        out, res, npre = want.get(c, (None, None, None))
        if out is None:
            continue
        assert sorted(os.listdir(root / str(c))) == sorted("%d.dat" % k for k in range(npre))
        for k in range(npre):
            assert (root / str(c) / ("%d.dat" % k)).read_bytes() == out[k].tobytes(), (c, k)
            assert any(l.startswith("%d:%d: sample %d " % (c, k, int(res[k]["sc_start"]))) for l in lines), (c, k)
    for bad in (["--grid", "7/1", "all"], ["--grid", "25/4", "7"], ["--grid", "25/4", "1,x"], ["--grid", "6", "all"], ["--grid", "3/2", "0"]):
        q = subprocess.run([exe] + bad + [str(tmp_path / "o2"), str(wav)], capture_output=True, text=True, timeout=60)
        assert q.returncode == 1 and not os.path.exists(tmp_path / "o2"), bad
    q = subprocess.run([exe, "--grid", "25/4", "auto", str(tmp_path / "o3"), str(wav)], capture_output=True, text=True, timeout=60)
    assert q.returncode == 1 and "not built" in q.stderr and not os.path.exists(tmp_path / "o3")
    q = subprocess.run([os.path.join(ROOT, "modem_amd", "bin", "survey"), "--grid", str(wav), "25/4"], capture_output=True, text=True, timeout=60)
    assert q.returncode == 1 and "not built" in q.stderr
    q = subprocess.run([os.path.join(ROOT, "modem_amd", "bin", "synthesize"), "--grid", str(tmp_path / "s.wav"), "25/4", "0:0:0:" + str(wav)],
                       capture_output=True, text=True, timeout=60)
    assert q.returncode == 1 and "not built" in q.stderr and not os.path.exists(tmp_path / "s.wav")
