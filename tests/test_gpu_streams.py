"""Many recordings in one call (ofdmrx_decode_streams*, added within revision 1.7): the records of recording s are,
byte for byte, what ofdmrx_decode_stream returns for that recording alone, however the recordings are batched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from stream_model import RATES, adversarial, serial_edges
from streams_model import leak_pair
from test_gpu_stream import _check_records

pytestmark = pytest.mark.gpu

E_ARG = -1


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=16)
    yield r
    r.close()


class Inputs:
    """the two oracle encodings everything else is derived from, made once"""

    def __init__(self):
        self.P4 = O.encode_pcm(O.payload_for(300, count=4), channels=2)
        self.F1 = O.encode_pcm(O.payload_for(310), channels=2)
        assert self.P4.shape == (324160, 2) and self.F1.shape == (95200, 2)
        self.P4.setflags(write=False)
        self.F1.setflags(write=False)
        # the middle of the second Schmidl-Cox symbol of P4: the oracle's second preamble, half a correlator length in
        self.cut = int(O.decode(self.P4, skip=1)[1].sc_start) + 640
        assert 80000 < self.cut < 100000

    def noisy_p4(self, seed):
        return O.impair(self.P4, noise_db=-30, seed=seed, frame=0)

    def ragged(self):
        rng = np.random.default_rng(77)
        P4, F1 = self.P4, self.F1
        gap = 24 * 4096 + 1 - len(F1)
        cutp = self.noisy_p4(12)
        s = [self.noisy_p4(11), np.zeros((3000, 2), np.int16), F1[:47600], F1[47600:],
             rng.normal(0, 1500, size=(5 * 4096, 2)).astype(np.int16),
             np.concatenate([rng.normal(0, 200, size=(gap, 2)).astype(np.int16), F1]),
             cutp[:self.cut], cutp[self.cut:], self.noisy_p4(13), self.noisy_p4(14), self.noisy_p4(15)]
        assert len(s[4]) == 5 * 4096 and len(s[5]) % 4096 == 1
        return [np.ascontiguousarray(x) for x in s]


@pytest.fixture(scope="module")
def inp():
    return Inputs()


def _call(rx, streams, per, cap, pad, entry="ofdmrx_decode_streams", sentinel=False, null_out=False):
    """the C entry on a buffer whose padding behind every recording is filled with copies of `pad` (a valid frame: a read past
    n_samples[s] shows up as an extra or changed record) -> (rc, payloads, results, n_preambles, first_record)"""
    import modem_amd.ofdmrx as M
    ch, dt = streams[0].shape[1], streams[0].dtype
    lens = np.array([len(x) for x in streams], np.uintp)
    stride = int(lens.max()) + len(pad)
    fill = np.concatenate([pad] * (stride // len(pad) + 1))
    buf = np.zeros((len(streams), stride, ch), dt)
    for q, x in enumerate(streams):
        buf[q, :len(x)] = x
        buf[q, len(x):] = fill[:stride - len(x)]
    out = np.full((max(cap, 1) + 3, M.PAYLOAD_BYTES), 0xA5 if sentinel else 0, np.uint8)
    res = np.zeros(max(cap, 1) + 3, M.RESULT_DTYPE)
    if sentinel:
        res["status"] = 77
    npre, first = np.zeros(len(streams), np.uintp), np.zeros(len(streams) + 1, np.uintp)
    rc = getattr(rx._lib, entry)(rx._h, M._ptr(buf), rx._fmt(dt), ch, len(streams), stride * ch * dt.itemsize, M._ptr(lens), per, cap,
                                 None if null_out else M._ptr(out), None if null_out else M._ptr(res), M._ptr(npre), M._ptr(first))
    return rc, out, res, npre.astype(np.int64), first.astype(np.int64)


def _same_as_one_call(rx, streams, out, res, npre, first, per=None):
    """per recording: payload bytes, every byte of the results and the preamble count equal the one-call entry's"""
    at = 0
    refs = []
    for q, x in enumerate(streams):
        if len(x):
            ro, rr, rn = rx.decode_stream(x)
        else:
            ro, rr, rn = np.zeros((0, 5380), np.uint8), res[:0], 0
        k = rn if per is None else min(rn, per)
        assert int(npre[q]) == rn, (q, int(npre[q]), rn)
        assert int(first[q]) == at, (q, int(first[q]), at)
        assert out[at:at + k].tobytes() == ro[:k].tobytes(), q
        assert res[at:at + k].tobytes() == rr[:k].tobytes(), (q, res[at:at + k], rr[:k])
        refs.append((ro, rr, rn))
        at += k
    assert int(first[len(streams)]) == at
    return refs


@pytest.mark.parametrize("channels", [2, 1])
def test_ragged_batch_equals_one_call(rx, inp, channels):
    streams = inp.ragged()
    pad = inp.F1
    if channels == 1:
        streams = [np.ascontiguousarray(x[:, :1]) for x in streams]
        pad = np.ascontiguousarray(pad[:, :1])
    rc, out, res, npre, first = _call(rx, streams, 2 ** 40, 64, pad)
    assert rc == 0
    refs = _same_as_one_call(rx, streams, out, res, npre, first)
    assert int(first[-1]) > 16                                   # more records than a chunk of 16: chunks mix recordings
    assert npre[0] == 4 and npre[1] == 0 and npre[4] == 0 and npre[5] == 1 and (npre[8:] == 4).all()
    assert npre[6] >= 1 and npre[7] >= 2                         # (the frames that lie wholly in one half of the cut recording)
    # two of the recordings against the oracle's skip-k decode as well
    for q in (5, 2):
        a, b = int(first[q]), int(first[q + 1])
        _check_records(out[a:b], res[a:b], int(npre[q]), streams[q])
    assert [len(r[1]) for r in refs][1] == 0


def test_caps(rx, inp):
    streams = [inp.noisy_p4(21), inp.noisy_p4(22), inp.noisy_p4(23)]
    rc, out, res, npre, first = _call(rx, streams, 2, 5, inp.F1, sentinel=True)
    assert rc == 0 and list(npre) == [4, 4, 4] and list(first) == [0, 2, 4, 6]
    at = 0
    for q, k in enumerate([2, 2, 1]):                            # [s0:2, s1:2, s2:1]
        ro, rr, rn = rx.decode_stream(streams[q])
        assert out[at:at + k].tobytes() == ro[:k].tobytes() and res[at:at + k].tobytes() == rr[:k].tobytes(), q
        at += k
    assert (out[5:] == 0xA5).all() and (res["status"][5:] == 77).all()   # nothing behind record 4 is touched
    rc, out, res, npre, first = _call(rx, streams, 2, 0, inp.F1, null_out=True)
    assert rc == 0 and list(npre) == [4, 4, 4] and list(first) == [0, 2, 4, 6]   # a count-only call


def test_device_entry(rx, inp):
    import torch
    import modem_amd.ofdmrx as M
    streams = [inp.noisy_p4(31), np.ascontiguousarray(inp.F1[:47600]), np.ascontiguousarray(inp.F1), inp.noisy_p4(32)]
    rc, ho, hr, hn, hf = _call(rx, streams, 2 ** 40, 16, inp.F1)
    assert rc == 0
    n_rec = int(hf[-1])
    assert n_rec >= 9
    lens = [len(x) for x in streams]
    stride = max(lens) + 1000
    buf = np.zeros((len(streams), stride, 2), np.int16)
    for q, x in enumerate(streams):
        buf[q, :len(x)] = x
        k = min(stride - len(x), len(inp.F1))
        buf[q, len(x):len(x) + k] = inp.F1[:k]
    d_pcm = torch.from_numpy(buf).cuda()
    d_out = torch.zeros((16, 5380), dtype=torch.uint8, device="cuda")
    d_res = torch.zeros((16, M.RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    npre, first = rx.decode_streams_device(d_pcm.data_ptr(), 0, 2, lens, stride * 4, 2 ** 40, 16, d_out.data_ptr(), d_res.data_ptr())
    rx.synchronize()
    assert list(npre) == list(hn) and list(first) == list(hf)
    assert d_out.cpu().numpy()[:n_rec].tobytes() == ho[:n_rec].tobytes()
    assert d_res.cpu().numpy()[:n_rec].tobytes() == hr[:n_rec].tobytes()
    p_out = torch.zeros((16, 5380), dtype=torch.uint8).pin_memory()
    p_res = torch.zeros((16, M.RESULT_DTYPE.itemsize), dtype=torch.uint8).pin_memory()
    npre, first = rx.decode_streams_device(d_pcm.data_ptr(), 0, 2, lens, stride * 4, 2 ** 40, 16, p_out.data_ptr(), p_res.data_ptr())
    rx.synchronize()
    assert list(npre) == list(hn) and list(first) == list(hf)
    assert p_out.numpy()[:n_rec].tobytes() == ho[:n_rec].tobytes() and p_res.numpy()[:n_rec].tobytes() == hr[:n_rec].tobytes()


def _wrapper_equals_one_call(r, streams):
    got = r.decode_streams(streams)
    assert len(got) == len(streams)
    total = 0
    for x, (o, rs, n) in zip(streams, got):
        ro, rr, rn = r.decode_stream(x)
        assert n == rn and o.tobytes() == ro.tobytes() and rs.tobytes() == rr.tobytes()
        total += rn
    return total


def test_48k_mono():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=16, sample_rate=48000)
    try:
        a = O.impair(O.encode_pcm(O.payload_for(320, count=2), channels=2, rate=48000), noise_db=-30, seed=2, frame=0, rate=48000)
        b = O.encode_pcm(O.payload_for(321), channels=2, rate=48000)
        streams = [np.ascontiguousarray(a[:, :1]), np.ascontiguousarray(b[:len(b) - 12345, :1])]
        assert _wrapper_equals_one_call(r, streams) >= 3
    finally:
        r.close()


@pytest.mark.parametrize("fmt", ["u8", "f32"])
def test_formats(rx, inp, fmt):
    a = O.encode_pcm(O.payload_for(330, count=2), channels=2, bits=8 if fmt == "u8" else 16)
    b = O.encode_pcm(O.payload_for(331), channels=2, bits=8 if fmt == "u8" else 16)
    if fmt == "f32":
        a, b = O.pcm_to_cf(a), O.pcm_to_cf(b)
    streams = [a, np.ascontiguousarray(b[:60001]), b]
    assert _wrapper_equals_one_call(rx, streams) >= 3


def test_debug_streams_edges(rx):
    ml, hs, gl = RATES[8000]
    a, b = leak_pair(ml, 4096, 4097)                             # a ends with its trigger on; b starts between lo and hi, then falls below lo
    seqs = [adversarial(1, 1, ml), adversarial(4095, 2, ml), a, b, adversarial(3 * 4096 + 17, 3, ml), adversarial(4097, 4, ml)]
    assert [len(s) for s in seqs] == [1, 4095, 4096, 4097, 3 * 4096 + 17, 4097]
    got = rx.debug_streams_edges(seqs)
    total = 0
    for s, (te, tm, im, n) in zip(seqs, got):
        se, st, si = serial_edges(s, ml, hs, gl)
        assert n == len(se)
        np.testing.assert_array_equal(te, se)
        np.testing.assert_array_equal(tm, st)
        np.testing.assert_array_equal(im, si)
        total += n
    assert got[3][3] == 0 and total > 20                         # a leaked state would have emitted an edge in b
    small = rx.debug_streams_edges(seqs, max_edges_per_stream=2)
    for (te, tm, im, n), (fe, fm, fi, fn) in zip(small, got):
        assert n == fn                                           # a small buffer still counts every edge
        np.testing.assert_array_equal(te, fe[:2])
        np.testing.assert_array_equal(tm, fm[:2])
        np.testing.assert_array_equal(im, fi[:2])


def test_esn0_rows_and_open_feed(rx, inp):
    import modem_amd.ofdmrx as M
    streams = [inp.noisy_p4(41), np.ascontiguousarray(inp.F1), inp.noisy_p4(42)]
    got = rx.decode_streams(streams, esn0_rows=True)
    for x, (o, rs, n, rows) in zip(streams, got):
        ro, rr, rn, rrows = rx.decode_stream(x, esn0_rows=True)
        assert n == rn and len(rows) == rn and rows.tobytes() == rrows.tobytes()   # row block i belongs to packed record i
        assert np.abs(rows[:, :50]).max() > 0
    f = rx.feed(2)
    try:
        with pytest.raises(M.OfdmRxError):
            rx.decode_streams(streams)
        rc = _call(rx, streams, 4, 16, inp.F1)[0]
        assert rc == E_ARG
        rc = _call(rx, streams, 4, 16, inp.F1, entry="ofdmrx_decode_streams_device")[0]   # (refused before the pointers are looked at)
        assert rc == E_ARG
    finally:
        f.end()
    assert rx.decode_streams(streams)[0][2] == 4


def test_analytic_tap_is_refused_after_a_streams_call(rx, inp):
    """the ANALYTIC tap forms a frame's analytic signal from the last chunk's samples at frame * stride: after a streams call (whose
    pipeline frames are records of several recordings, stride 0, 2-channel data) it answers OFDMRX_E_ARG and reads nothing"""
    import modem_amd.ofdmrx as M
    streams = [np.ascontiguousarray(inp.F1[:, :1]), np.ascontiguousarray(inp.noisy_p4(51)[:, :1])]
    got = rx.decode_streams(streams)
    assert got[0][2] == 1 and got[1][2] == 4
    a = np.zeros((100, 2), np.float32)
    for frame in (0, 1, 4):
        assert rx._lib.ofdmrx_debug_dump(rx._h, M.TAPS["ANALYTIC"], frame, M._ptr(a), a.nbytes) == E_ARG
    assert len(rx.tap("HDR_SOFT", 4)) == 255                     # (the per-frame taps of the last chunk are there: 5 records)


def test_cli_batch(tmp_path):
    """`decode_stream --batch OUTROOT A.wav B.wav C.wav` writes OUTROOT/<i>/<k>.dat: the files three runs of the existing command line
    write, and its summary lines are theirs prefixed with `<i>:`"""
    bin_dir = os.path.join(O.ROOT, "modem_amd", "bin")
    wavs = []
    for i, count in enumerate([2, 1, 3]):
        files = []
        for k in range(count):
            f = tmp_path / ("p%d_%d.dat" % (i, k))
            f.write_bytes(bytes(O.payload_for(1800 + 10 * i + k)))
            files.append(str(f))
        wav = tmp_path / ("w%d.wav" % i)
        subprocess.check_call([os.path.join(bin_dir, "encode"), str(wav), "8000", "16", "2", "1500", "6", "CALL %d" % i] + files)
        wavs.append(str(wav))
    root = tmp_path / "root"
    p = subprocess.run([os.path.join(bin_dir, "decode_stream"), "--batch", str(root)] + wavs, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    lines = p.stderr.strip().splitlines()
    for i, count in enumerate([2, 1, 3]):
        one = tmp_path / ("one%d" % i)
        one.mkdir()
        q = subprocess.run([os.path.join(bin_dir, "decode_stream"), str(one), wavs[i]], capture_output=True, text=True)
        assert q.returncode == 0, q.stderr
        assert sorted(os.listdir(root / str(i))) == sorted(os.listdir(one)) == ["%d.dat" % k for k in range(count)]
        for k in range(count):
            assert (root / str(i) / ("%d.dat" % k)).read_bytes() == (one / ("%d.dat" % k)).read_bytes(), (i, k)
        assert [l for l in lines if l.startswith("%d:" % i)] == ["%d:%s" % (i, l) for l in q.stderr.strip().splitlines()]
    # a WAV without sample frames is a recording of length 0: an empty directory, no lines, the others unchanged
    import struct
    empty = tmp_path / "empty.wav"
    empty.write_bytes(b"RIFF" + struct.pack("<I", 36) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 2, 8000, 32000, 4, 16) + b"data" + struct.pack("<I", 0))
    root3 = tmp_path / "root3"
    p3 = subprocess.run([os.path.join(bin_dir, "decode_stream"), "--batch", str(root3), str(empty), wavs[1]], capture_output=True, text=True)
    assert p3.returncode == 0, p3.stderr
    assert os.listdir(root3 / "0") == [] and os.listdir(root3 / "1") == ["0.dat"]
    assert (root3 / "1" / "0.dat").read_bytes() == (root / "1" / "0.dat").read_bytes()
    assert all(l.startswith("1:") for l in p3.stderr.strip().splitlines())
    # inputs that do not share rate, channels and format are refused with a message
    other = tmp_path / "mono.wav"
    f = tmp_path / "p.dat"
    f.write_bytes(bytes(O.payload_for(1)))
    subprocess.check_call([os.path.join(bin_dir, "encode"), str(other), "8000", "16", "1", "1500", "6", "CALL 9", str(f)])
    bad = subprocess.run([os.path.join(bin_dir, "decode_stream"), "--batch", str(tmp_path / "root2"), wavs[0], str(other)], capture_output=True, text=True)
    assert bad.returncode != 0 and "share" in bad.stderr
