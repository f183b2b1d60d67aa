"""The grid bank (ofdmrx_bank_begin_wideband_grid / ofdmrx_bank_push_wideband) on the captures of
grid_fixture.py: for every slot and any cutting of the capture into pushes, the records equal the stream decode of that slot's row
of ofdmrx_util_channelize_grid over the whole capture - every payload byte, every byte of every result - and they are the records
test_channelize_grid_model_cpu.py found with the oracle on the float64 model's rows."""
import ctypes as C
import os
import subprocess
import wave

import numpy as np
import pytest

import grid_fixture as GF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1)
    yield r
    r.close()


def _ref(rx, cfg, capture):
    """the capture, its slot rows from the device, and their stream decode: computed once, read only"""
    import torch
    pcm, pays = capture()
    D, slots = cfg["D"], list(cfg["open"])
    n_out = -(-len(pcm) // D)
    d_in = torch.from_numpy(pcm).to("cuda:0")
    d_out = torch.full((len(slots), n_out, 2), 12345.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rx.channelize_grid(d_in.data_ptr(), 0, 0, len(pcm), D, slots, 0, n_out, d_out.data_ptr())
    rx.synchronize()
    rows = d_out.cpu().numpy()
    recs = rx.decode_streams(list(rows))
    for a in (pcm, pays, rows):
        a.setflags(write=False)
    return pcm, pays, rows, recs


@pytest.fixture(scope="module")
def ref_a(rx):
    return _ref(rx, GF.A, GF.capture_a)


@pytest.fixture(scope="module")
def ref_b(rx):
    return _ref(rx, GF.B, GF.capture_b)


def _table(rec, pays):
    out, res, npre = rec
    assert len(res) == npre
    return [(int(res[k]["status"]), ([j for j in range(len(pays)) if (out[k] == pays[j]).all()] + [None])[0]) for k in range(npre)]


def _check_expected(cfg, want, ref):
    """every slot's records are the table of the fixture; a decoded frame stands at its own sc_start with no flipped bit; the oracle
    on the device's own rows agrees in status and sc_start, and in the payload of every decoded frame"""
    pcm, pays, rows, recs = ref
    for i, k in enumerate(cfg["open"]):
        assert _table(recs[i], pays) == want.get(k, []), k
        out, res, npre = recs[i]
        orc = GF.oracle_records(rows[i])
        assert len(orc) == npre, k
        for j, (status, frame) in enumerate(want.get(k, [])):
            o, r = orc[j]
            assert r.status == status and r.sc_start == int(res[j]["sc_start"]), (k, j)
            if status == 0:
                assert int(res[j]["sc_start"]) == GF.sc_start(cfg, frame) and int(res[j]["bit_flips"]) == 0, (k, j)
                assert (o == out[j]).all() and (out[j] == pays[frame]).all(), (k, j)


def test_a_slots_decode_the_golden_payloads(ref_a):
    _check_expected(GF.A, GF.EXPECTED_A, ref_a)


def test_b_slots_decode_the_golden_payloads(ref_b):
    """D = 64, a 512 kHz capture: frames at slots 37 and 39, nothing in slot 38 between them"""
    _check_expected(GF.B, GF.EXPECTED_B, ref_b)


def _by_channel(parts, n_channels):
    """the tuples push / end returned, in order -> per channel (payload bytes, result bytes, indices)"""
    pay = np.concatenate([p[0] for p in parts])
    res = np.concatenate([p[1] for p in parts])
    ch = np.concatenate([p[2] for p in parts])
    ix = np.concatenate([p[3] for p in parts])
    return [(pay[ch == c].tobytes(), res[ch == c].tobytes(), list(ix[ch == c])) for c in range(n_channels)]


def _through_bank(rx, pcm, blocks, cfg):
    bank = rx.wideband_grid_bank(list(cfg["open"]), cfg["D"])
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
    return _by_channel(parts, len(cfg["open"]))


def _bank_equals(rx, ref, blocks, cfg):
    pcm, pays, rows, recs = ref
    got = _through_bank(rx, pcm, blocks, cfg)
    for c, (out, res, npre) in enumerate(recs):
        assert got[c][2] == list(range(npre)), c
        assert got[c][0] == out.tobytes() and got[c][1] == res.tobytes(), c
        assert res.itemsize == 56


@pytest.mark.parametrize("blocks", [(1 << 26,), (64000,), (40009, 0)], ids=["one push", "seconds", "40009 and 0"])
def test_a_bank_equals_the_one_call_decode(rx, ref_a, blocks):
    """all 16 slots, per slot byte for byte: payloads and all 56 bytes of every result"""
    _bank_equals(rx, ref_a, blocks, GF.A)


def test_b_bank_equals_the_one_call_decode(rx, ref_b):
    """D = 64: pushes of one wideband second (the kept tail is 24 x 64 samples)"""
    _bank_equals(rx, ref_b, (512000,), GF.B)


def test_a_plain_bank_finds_the_same_frames(rx, ref_a):
    """a plain wideband bank at the four frames' centres: equal payload, status and sc_start (the sample bytes differ within the
    tolerances, so the float fields of the results may)"""
    import modem_amd
    import modem_amd.ofdmrx as M
    pcm, pays, rows, recs = ref_a
    f = modem_amd.grid_centres(GF.A["D"], GF.RATE, GF.A["slots"])
    bank = rx.wideband_bank(f, GF.A["D"])
    try:
        parts = [bank.push(pcm), bank.end()]
    finally:
        while bank.open:
            bank.end()
    got = _by_channel(parts, 4)
    for c, k in enumerate(GF.A["slots"]):
        out, res, npre = recs[GF.A["open"].index(k)]
        p = np.frombuffer(got[c][0], np.uint8).reshape(-1, 5380)
        r = np.frombuffer(got[c][1], M.RESULT_DTYPE)
        assert len(r) == npre == 1
        assert (p == out).all() and (r["status"] == res["status"]).all() and (r["sc_start"] == res["sc_start"]).all(), k


def test_stage_ops_do_not_depend_on_the_slot_count(rx, ref_a):
    """the pushes before the first preamble: the same launches, copies and synchronisations for one slot and for sixteen"""
    pcm = ref_a[0]
    ops = {}
    for n in (1, 16):
        bank = rx.wideband_grid_bank(list(GF.A["open"])[:n], GF.A["D"])
        try:
            ops[n] = []
            for a, b in ((0, 64000), (64000, 68097), (68097, 68097), (68097, 68098)):
                bank.push(pcm[a:b])
                ops[n].append(bank.last_stage_ops)
        finally:
            while bank.open:
                bank.end()
    assert ops[1] == ops[16] and ops[1][0] > 0, ops


def test_refusals_with_an_open_bank(rx, ref_a):
    import torch
    import modem_amd.ofdmrx as M
    pcm = ref_a[0]
    D = GF.A["D"]
    out, res = np.zeros((4, 5380), np.uint8), np.zeros(4, M.RESULT_DTYPE)
    ch, ix = np.zeros(4, np.int32), np.zeros(4, np.int64)
    a, b = C.c_size_t(0), C.c_size_t(0)
    lens = np.zeros(2, np.uintp)
    p = M._ptr
    L, h = rx._lib, rx._h
    wide = lambda n=0, smp=None: L.ofdmrx_bank_push_wideband(h, smp, n, 0, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b))
    plain = lambda: L.ofdmrx_bank_push(h, None, 0, p(lens), None, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b))
    k = np.array([3, -8], np.int32)
    f = np.array([1000.0, -1000.0])
    begin = L.ofdmrx_bank_begin_wideband_grid
    assert wide() == -1                                              # no bank open
    assert begin(h, 2, p(k), D, 3) == -1 and begin(h, 2, p(k), 6, 0) == -1 and begin(h, 2, p(k), 1024, 0) == -1
    assert begin(h, 0, p(k), D, 0) == -1 and begin(h, 2, None, D, 0) == -1
    assert begin(h, 2, p(np.array([3, 8], np.int32)), D, 0) == -1    # a slot outside -8 .. 7
    assert L.ofdmrx_bank_begin(h, 2, 2, 2) == 0
    assert wide() == -1 and begin(h, 2, p(k), D, 0) == -1            # another bank is open
    assert L.ofdmrx_bank_end(h, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b)) == 0
    assert begin(h, 2, p(k), D, 0) == 0
    assert plain() == -1 and L.ofdmrx_bank_begin(h, 2, 2, 2) == -1 and begin(h, 2, p(k), D, 0) == -1
    assert L.ofdmrx_bank_begin_wideband(h, 2, p(f), D, 0) == -1
    # the front-end entries while the bank owns the device tables
    d_in = torch.from_numpy(np.array(pcm[:4096])).to("cuda:0")
    d_out = torch.full((2, 512, 2), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert L.ofdmrx_util_channelize_grid(h, d_in.data_ptr(), 0, 0, 4096, D, p(k), 2, 0, 512, d_out.data_ptr(), 512) == -1
    assert L.ofdmrx_util_channelize(h, d_in.data_ptr(), 0, 0, 4096, D, p(f), 2, 0, 512, d_out.data_ptr(), 512) == -1
    assert L.ofdmrx_util_channelize_ratio(h, d_in.data_ptr(), 0, 0, 4096, 5, 2, p(f), 2, 0, 512, d_out.data_ptr(), 512) == -1
    rx.synchronize()
    assert bool((d_out == 7.0).all())
    assert wide(10, None) == -1                                      # NULL samples with a length
    blk = np.ascontiguousarray(pcm[:1001])
    assert wide(1001, p(blk)) == 0 and L.ofdmrx_bank_resident_samples(h, 1) == 126       # ceil(1001 / 8)
    assert L.ofdmrx_bank_push_wideband(h, p(blk), 5, 1, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b)) == 0   # ... and the end
    assert wide(5, p(blk)) == -1                                     # samples after the end
    assert L.ofdmrx_bank_end(h, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b)) == 0 and b.value == 0
    assert L.ofdmrx_util_channelize_grid(h, d_in.data_ptr(), 0, 0, 4096, D, p(k), 2, 0, 512, d_out.data_ptr(), 512) == 0   # closed: served again
    rx.synchronize()
    assert not bool((d_out == 7.0).any())


def test_command_line(ref_a, tmp_path):
    """decode_stream --grid 8 all writes the .dat files of (a) and names every slot's centre"""
    pcm, pays, rows, recs = ref_a
    D = GF.A["D"]
    wav = tmp_path / "wide.wav"
    with wave.open(str(wav), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(D * GF.RATE)
        w.writeframes(pcm.tobytes())
    exe = os.path.join(ROOT, "modem_amd", "bin", "decode_stream")
    root = tmp_path / "out"
    p = subprocess.run([exe, "--grid", str(D), "all", str(root), str(wav)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    for i, k in enumerate(GF.A["open"]):
        assert "%d: slot %d, centre %.17g Hz" % (i, k, k * 4000.0) in p.stderr.splitlines()
    lines = [l for l in p.stderr.splitlines() if ": sample " in l]
    assert len(lines) == sum(r[2] for r in recs)
    for c, (out, res, npre) in enumerate(recs):
        assert sorted(os.listdir(root / str(c))) == sorted("%d.dat" % k for k in range(npre))
        for k in range(npre):
            assert (root / str(c) / ("%d.dat" % k)).read_bytes() == out[k].tobytes(), (c, k)
            assert any(l.startswith("%d:%d: sample %d " % (c, k, int(res[k]["sc_start"]))) for l in lines), (c, k)
    for bad in (["--grid", "6", "all"], ["--grid", "8", "8"], ["--grid", "8", "1,x"]):
        q = subprocess.run([exe] + bad + [str(tmp_path / "o2"), str(wav)], capture_output=True, text=True, timeout=60)
        assert q.returncode == 1 and not os.path.exists(tmp_path / "o2"), bad
    odd = tmp_path / "odd.wav"
    with wave.open(str(odd), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(50000)
        w.writeframes(pcm[:100].tobytes())
    q = subprocess.run([exe, "--grid", str(D), "0", str(tmp_path / "o3"), str(odd)], capture_output=True, text=True, timeout=60)
    assert q.returncode == 1 and "Unsupported sample rate." in q.stderr
