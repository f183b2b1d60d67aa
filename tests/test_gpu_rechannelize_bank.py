"""The wideband bank at a rational decimation (ofdmrx_bank_begin_wideband_ratio / ofdmrx_bank_push_wideband)
on the 50 kHz capture of rechannelize_fixture.py: for every channel and any cutting of the capture into pushes, the records equal
the stream decode of that channel's row of ofdmrx_util_channelize_ratio over the whole capture - every payload byte, every byte of
every result - and the oracle on the float64 model's rows agrees; the refusals that need an open bank; the command lines."""
import ctypes as C
import os
import subprocess
import wave

import numpy as np
import pytest

import oracle_lib as O
import rechannelize_fixture as RF
import rechannelize_model as RM

pytestmark = pytest.mark.gpu

P, Q = RF.P, RF.Q
CENTRES = np.array(RF.CHANNEL_HZ)
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
    pcm, pays = RF.capture()
    n_out = RM.n_outputs(len(pcm), P, Q)
    d_in = torch.from_numpy(pcm).to("cuda:0")
    d_out = torch.full((len(CENTRES), n_out, 2), 12345.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rx.channelize(d_in.data_ptr(), 0, 0, len(pcm), (P, Q), CENTRES, 0, n_out, d_out.data_ptr())
    rx.synchronize()
    rows = d_out.cpu().numpy()
    recs = rx.decode_streams(list(rows))
    for a in (pcm, pays, rows):
        a.setflags(write=False)
    return pcm, pays, rows, recs


@pytest.fixture(scope="module")
def wav(ref, tmp_path_factory):
    path = tmp_path_factory.mktemp("rechannelize") / "wide.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(RF.WIDE_RATE)
        w.writeframes(ref[0].tobytes())
    return path


def test_channels_decode_the_golden_payloads(ref):
    """every frame from its channel, 12 samples late; the empty channel: nothing.  The device's rows are within tol of the float64
    model's, and the oracle on the MODEL's rows agrees in payload, status and sc_start (the other fields as the 4.14 bank test
    compares them: the oracle on the device's own rows)"""
    pcm, pays, rows, recs = ref
    assert [r[2] for r in recs] == [1, 1, 0]
    v, tol, tie = RM.channelize(pcm, P, Q, CENTRES, RF.RATE)
    w = RM.worst(rows, v, tol)
    print("rechannelize 25/4 fixture: 3 channels x %d outputs, worst |got - v| / tol %.4f" % (v.shape[1], w))
    assert tie > 1e-6 and w <= 1.0
    model_rows = np.stack([v.real, v.imag], axis=2).astype(np.float32)
    for c in range(2):
        out, res, _ = recs[c]
        assert int(res[0]["status"]) == 0 and (out[0] == pays[c]).all() and int(res[0]["bit_flips"]) == 0
        assert int(res[0]["sc_start"]) == RF.SC_START[c], c
        o, r = O.decode(model_rows[c])
        assert r.status == 0 and (o == out[0]).all() and r.sc_start == int(res[0]["sc_start"]), c
        assert O.decode(model_rows[c], skip=1)[1].status == 1, c
    assert O.decode(model_rows[2])[1].status == 1
    for c in range(3):
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


def _through_bank(rx, pcm, blocks, centres=CENTRES, decim=(P, Q)):
    bank = rx.wideband_bank(centres, decim)
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


CUTTINGS = {"one push": (1 << 26,), "blocks of 50000": (50000,), "blocks of 4097": (4097,), "blocks of 7": (7,),
            "mixed": (0, P - 1, 50000, 1, 0, 4097, P - 1, 7 * 4096 + 3)}


@pytest.mark.parametrize("cut", list(CUTTINGS))
def test_bank_equals_the_one_call_decode(rx, ref, cut):
    """per channel, byte for byte: payloads and all 56 bytes of every result"""
    pcm, pays, rows, recs = ref
    got = _through_bank(rx, pcm, CUTTINGS[cut])
    for c, (out, res, npre) in enumerate(recs):
        assert got[c][2] == list(range(npre)), c
        assert got[c][0] == out.tobytes() and got[c][1] == res.tobytes(), c
        assert res.itemsize == 56


def test_a_fraction_opens_the_same_bank(rx, ref):
    import fractions
    pcm, pays, rows, recs = ref
    got = _through_bank(rx, pcm, (200000,), decim=fractions.Fraction(50, 8))
    for c, (out, res, npre) in enumerate(recs):
        assert got[c][0] == out.tobytes() and got[c][1] == res.tobytes(), c


def test_stage_ops_do_not_depend_on_the_channel_count(rx, ref):
    """the pushes before the first preamble: the same launches, copies and synchronisations for one channel and for three"""
    pcm = ref[0]
    ops = {}
    for n in (1, 3):
        bank = rx.wideband_bank(CENTRES[:n], (P, Q))
        try:
            ops[n] = []
            for a, b in ((0, 50000), (50000, 54097), (54097, 54097), (54097, 54098), (54098, 54098 + P - 1)):
                bank.push(pcm[a:b])
                ops[n].append(bank.last_stage_ops)
        finally:
            while bank.open:
                bank.end()
    assert ops[1] == ops[3] and ops[1][0] > 0, ops


def test_refusals_that_need_a_bank(rx, ref):
    """ofdmrx_bank_push on a ratio bank; the util entries and a second begin while a bank is open; a centre outside +- Rw / 2"""
    import torch
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
    begin = L.ofdmrx_bank_begin_wideband_ratio
    f = np.array([1000.0, -1000.0])
    assert wide() == -1                                              # no bank open
    for bad in ((0, 4), (25, 0), (35, 17), (7, 4), (129, 4)):
        assert begin(h, 2, p(f), bad[0], bad[1], 0) == -1, bad
    assert begin(h, 2, p(f), P, Q, 3) == -1 and begin(h, 2, None, P, Q, 0) == -1 and begin(h, 0, p(f), P, Q, 0) == -1
    g = np.array([1000.0, 25000.5])
    assert begin(h, 2, p(g), P, Q, 0) == -1                          # a centre outside +- Rw / 2 = 25000
    assert L.ofdmrx_bank_begin(h, 2, 2, 2) == 0
    assert wide() == -1 and begin(h, 2, p(f), P, Q, 0) == -1
    assert L.ofdmrx_bank_end(h, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b)) == 0
    assert begin(h, 2, p(f), 2 * P, 2 * Q, 0) == 0                   # (50, 8) is (25, 4)
    assert plain() == -1 and L.ofdmrx_bank_begin(h, 2, 2, 2) == -1 and begin(h, 2, p(f), P, Q, 0) == -1
    assert L.ofdmrx_bank_begin_wideband(h, 2, p(f), 6, 0) == -1
    d_in = torch.from_numpy(pcm[:4096].copy()).to("cuda:0")
    d_out = torch.full((2, 700, 2), 12345.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert L.ofdmrx_util_channelize_ratio(h, d_in.data_ptr(), 0, 0, 4096, P, Q, p(f), 2, 0, 656, d_out.data_ptr(), 700) == -1
    assert L.ofdmrx_util_channelize(h, d_in.data_ptr(), 0, 0, 4096, 6, p(f), 2, 0, 683, d_out.data_ptr(), 700) == -1
    assert wide(10, None) == -1                                      # NULL samples with a length
    blk = np.ascontiguousarray(pcm[:1000])
    assert wide(1000, p(blk)) == 0 and L.ofdmrx_bank_resident_samples(h, 1) == 160       # ceil(1000 x 4 / 25)
    assert wide(3, p(blk)) == 0 and L.ofdmrx_bank_resident_samples(h, 1) == 161          # ceil(1003 x 4 / 25)
    assert L.ofdmrx_bank_push_wideband(h, p(blk), 5, 1, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b)) == 0   # ... and the end
    assert wide(5, p(blk)) == -1                                     # samples after the end
    assert L.ofdmrx_bank_end(h, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b)) == 0 and b.value == 0
    torch.cuda.synchronize()
    assert bool((d_out == 12345.0).all())
    assert L.ofdmrx_util_channelize_ratio(h, d_in.data_ptr(), 0, 0, 4096, P, Q, p(f), 2, 0, 656, d_out.data_ptr(), 700) == 0   # the bank is gone
    rx.synchronize()


# ---- the command lines

def _run(args, timeout=120):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=timeout)


def test_decode_stream_takes_a_ratio(ref, wav, tmp_path):
    """decode_stream --wideband 25/4 -14000,9000 writes the two payloads"""
    pcm, pays, rows, recs = ref
    exe = os.path.join(ROOT, "modem_amd", "bin", "decode_stream")
    root = tmp_path / "out"
    p = _run([exe, "--wideband", "25/4", "-14000,9000", root, wav])
    assert p.returncode == 0, p.stderr
    lines = [l for l in p.stderr.splitlines() if ": sample " in l]
    assert len(lines) == 2
    for c in range(2):
        out, res, npre = recs[c]
        assert os.listdir(root / str(c)) == ["0.dat"]
        assert (root / str(c) / "0.dat").read_bytes() == out[0].tobytes() == pays[c].tobytes(), c
        assert any(l.startswith("%d:0: sample %d " % (c, RF.SC_START[c])) for l in lines), c
    p = _run([exe, "--wideband", "50/8", "-14000,9000", tmp_path / "o2", wav])          # the entries reduce by the gcd themselves
    assert p.returncode == 0 and (tmp_path / "o2" / "1" / "0.dat").read_bytes() == pays[1].tobytes()
    p = _run([exe, "--wideband", "25/3", "0", tmp_path / "o3", wav])                     # 50000 x 3 / 25 = 6000: no supported rate
    assert p.returncode == 1 and not (tmp_path / "o3").exists()
    p = _run([exe, "--wideband", "27/4", "0", tmp_path / "o4", wav])                     # 50000 x 4 / 27: no integer
    assert p.returncode == 1 and "Unsupported sample rate." in p.stderr
    p = _run([exe, "--wideband", "35/17", "0", tmp_path / "o5", wav])
    assert p.returncode == 1 and "A wideband bank takes" in p.stderr


def test_auto_and_survey_find_the_two_centres(ref, wav, tmp_path):
    """--wideband 25/4 auto finds the two centres within 100 Hz and decodes from them; survey wide.wav 25/4 prints the same centres"""
    pcm, pays, rows, recs = ref
    exe = os.path.join(ROOT, "modem_amd", "bin", "decode_stream")
    root = tmp_path / "auto"
    p = _run([exe, "--wideband", "25/4", "auto", root, wav])
    assert p.returncode == 0, p.stderr
    line = [l for l in p.stderr.splitlines() if l.startswith("survey: ")]
    assert len(line) == 1
    found = [float(t) for t in line[0].split("centres ")[1].split(",")]
    assert len(found) == 2 and all(abs(a - b) <= 100.0 for a, b in zip(found, RF.SIGNAL_HZ)), found
    for c in range(2):
        assert (root / str(c) / "0.dat").read_bytes() == pays[c].tobytes(), c
    s = _run([os.path.join(ROOT, "modem_amd", "bin", "survey"), wav, "25/4"])
    assert s.returncode == 0, s.stderr
    printed = [float(l.split()[0]) for l in s.stdout.splitlines()]
    assert len(printed) == 2 and all(abs(a - b) < 0.005 for a, b in zip(printed, found)), (printed, found)


def test_an_integer_argument_behaves_as_before(tmp_path):
    """--wideband 6 on the 48 kHz capture of wideband_fixture.py: its old output (test_gpu_wideband_bank.py: one record per signal
    channel, two on the channel above the strong frame, none on the empty one)"""
    import wideband_fixture as WF
    pcm, pays = WF.capture()
    w48 = tmp_path / "wide48.wav"
    with wave.open(str(w48), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(WF.DECIM * WF.RATE)
        w.writeframes(pcm.tobytes())
    exe = os.path.join(ROOT, "modem_amd", "bin", "decode_stream")
    root = tmp_path / "out"
    p = _run([exe, "--wideband", "6", ",".join("%g" % f for f in WF.CHANNEL_HZ), root, w48])
    assert p.returncode == 0, p.stderr
    assert [sorted(os.listdir(root / str(c))) for c in range(5)] == [["0.dat"], ["0.dat"], ["0.dat"], ["0.dat", "1.dat"], []]
    for c, k in ((0, 0), (1, 0), (2, 0), (3, 1)):
        assert (root / str(c) / ("%d.dat" % k)).read_bytes() == pays[c].tobytes(), c
    r = _run([exe, "--wideband", "6/1", ",".join("%g" % f for f in WF.CHANNEL_HZ), tmp_path / "out2", w48])   # a ratio with Q = 1: the same bank
    assert r.returncode == 0, r.stderr
    for c in range(5):
        assert sorted(os.listdir(tmp_path / "out2" / str(c))) == sorted(os.listdir(root / str(c)))
        for name in os.listdir(root / str(c)):
            assert (tmp_path / "out2" / str(c) / name).read_bytes() == (root / str(c) / name).read_bytes()
    bad = _run([exe, "--wideband", "33", "0", tmp_path / "o3", w48])
    assert bad.returncode == 1 and "A wideband bank takes" in bad.stderr
