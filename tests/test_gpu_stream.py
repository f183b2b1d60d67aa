"""Stream decode (ofdmrx_decode_stream*, revision 1.7) against the oracle: record k of a recording is what the oracle's decoder gives
with SKIP = k on the same samples, *n_preambles the first k it answers with NO_SYNC."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from stream_model import RATES, adversarial, serial_edges

pytestmark = pytest.mark.gpu

REL = 1e-5


def _flips_ok(gpu, oracle):
    return abs(int(gpu) - int(oracle)) <= (2 if int(oracle) > 0 else 0)


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=16)
    yield r
    r.close()


def _rx(rate, **kw):
    import modem_amd
    return modem_amd.Receiver(device=0, chunk_frames=16, sample_rate=rate, **kw)


def _check_records(out, res, npre, pcm, rate=8000, payloads=None):
    """every record against the oracle's skip-k decode; the count against its first NO_SYNC"""
    k = 0
    while True:
        o, r = O.decode(pcm, skip=k, rate=rate)
        if r.status == 1:
            break
        assert k < len(res), (k, len(res), npre)
        g = res[k]
        assert int(g["status"]) == r.status, (k, int(g["status"]), r.status)
        assert (out[k] == o).all(), k
        assert int(g["sc_start"]) == r.sc_start and int(g["symbol_pos"]) == r.symbol_pos, k
        assert int(g["n_sync_rejects"]) == r.n_sync_rejects, k
        assert abs(float(g["cfo_rad"]) - r.cfo_rad) <= REL, k
        if r.status in (0, 6):
            assert int(g["oper_mode"]) == r.oper_mode and int(g["call_sign"]) == r.call_sign, k
            assert int(g["best_lane"]) == r.best_lane, k
            assert abs(float(g["cfo_fine"]) - r.cfo_fine) <= REL and abs(float(g["esn0_db_last"]) - r.esn0_db_last) < 1e-3, k
        if r.status == 0:
            assert _flips_ok(g["bit_flips"], r.bit_flips), k
            if payloads is not None and k < len(payloads):
                assert (out[k] == payloads[k]).all(), k
        k += 1
    assert npre == k, (npre, k)
    return k


def test_twelve_payload_stream(rx):
    pay = O.payload_for(40, count=12)
    pcm = O.impair(O.encode_pcm(pay, channels=2), noise_db=-30, seed=3, frame=0)
    out, res, npre = rx.decode_stream(pcm)
    assert npre == 12 and (res["status"] == 0).all()
    assert _check_records(out, res, npre, pcm, payloads=pay.reshape(12, -1)) == 12


def _mixed(channels, seed=5):
    rng = np.random.default_rng(seed)
    parts, pays = [], []
    for i, mode in enumerate([6, 7, 8, 9, 10, 11, 12, 13]):
        p = O.payload_for(100 + i)
        pcm = O.encode_pcm(p, channels=2, mode=mode, call_sign="CALL%d" % i)
        gap = int(rng.integers(0, 3 * 8000)) | 1                 # 0 .. 3 s at an odd offset
        noise = (rng.normal(0, 300, size=(gap, 2)) if i % 2 else np.zeros((gap, 2))).astype(np.int16)
        if i == 3:                                               # the header destroyed
            sc = 8000 + 1440                                     # pilot, then the S&C symbol and the header symbol
            pcm = pcm.copy()
            pcm[sc + 1440: sc + 3 * 1440] = rng.integers(-3000, 3000, size=(2 * 1440, 2))
        if i == 5:                                               # the payload destroyed
            pcm = pcm.copy()
            pcm[8000 + 6 * 1440: 8000 + 20 * 1440] = rng.integers(-3000, 3000, size=(14 * 1440, 2))
        parts += [noise, pcm]
        pays.append(p)
    last = O.encode_pcm(O.payload_for(199), channels=2)
    parts.append(last[: len(last) // 2])                         # cut off inside its payload
    s = np.concatenate(parts)
    s = O.impair(s, noise_db=-30, seed=seed, frame=0)
    if channels == 1:
        s = np.ascontiguousarray(s[:, :1])
    return s, pays


@pytest.mark.parametrize("channels", [2, 1])
def test_mixed_recording(rx, channels):
    pcm, pays = _mixed(channels)
    out, res, npre = rx.decode_stream(pcm)
    k = _check_records(out, res, npre, pcm)
    assert k >= 8


@pytest.mark.parametrize("rate,channels", [(48000, 2), (44100, 1)])
def test_other_rates(rate, channels):
    r = _rx(rate)
    try:
        pay = O.payload_for(60, count=3)
        pcm = O.encode_pcm(pay, channels=2, rate=rate)
        pcm = O.impair(pcm, noise_db=-30, seed=2, frame=0, rate=rate)
        if channels == 1:
            pcm = np.ascontiguousarray(pcm[:, :1])
        out, res, npre = r.decode_stream(pcm)
        assert _check_records(out, res, npre, pcm, rate=rate, payloads=pay.reshape(3, -1)) == 3
    finally:
        r.close()


@pytest.mark.parametrize("fmt", ["u8", "f32"])
def test_formats(rx, fmt):
    pay = O.payload_for(70, count=2)
    pcm = O.encode_pcm(pay, channels=2, bits=8 if fmt == "u8" else 16)
    if fmt == "f32":
        pcm = O.pcm_to_cf(pcm)
    out, res, npre = rx.decode_stream(pcm)
    assert _check_records(out, res, npre, pcm, payloads=pay.reshape(2, -1)) == 2


def test_against_batch_skip(rx):
    pay = O.payload_for(80, count=5)
    pcm = O.impair(O.encode_pcm(pay, channels=2), noise_db=-30, seed=4, frame=0)
    out, res, npre = rx.decode_stream(pcm)
    n = min(npre, 65)
    bo, br = rx.decode(np.repeat(pcm[None], n + 1, axis=0), skip=np.arange(n + 1, dtype=np.int32))
    for k in range(n):
        assert (bo[k] == out[k]).all() and br[k]["status"] == res[k]["status"] and br[k]["sc_start"] == res[k]["sc_start"]
        assert br[k]["n_sync_rejects"] == res[k]["n_sync_rejects"] and br[k]["symbol_pos"] == res[k]["symbol_pos"]
    assert br[n]["status"] == 1


def test_capacity(rx):
    import modem_amd.ofdmrx as M
    pay = O.payload_for(90, count=6)
    pcm = O.encode_pcm(pay, channels=2)
    out = np.full((5, 5380), 0xA5, np.uint8)
    res = np.zeros(5, M.RESULT_DTYPE)
    res["status"] = 77
    npre = C.c_size_t(0)
    rc = rx._lib.ofdmrx_decode_stream(rx._h, M._ptr(pcm), 0, 2, len(pcm), 3, M._ptr(out), M._ptr(res), C.byref(npre))
    assert rc == 0 and npre.value == 6
    assert (res["status"][:3] == 0).all() and (res["status"][3:] == 77).all() and (out[3:] == 0xA5).all()
    assert (out[:3] == pay.reshape(6, -1)[:3]).all()
    o, r, n = rx.decode_stream(pcm, max_frames=0)
    assert n == 6 and len(r) == 0


def test_nothing_to_find(rx):
    rng = np.random.default_rng(1)
    for pcm in (np.zeros((200000, 2), np.int16), rng.normal(0, 2000, size=(200000, 2)).astype(np.int16),
                O.encode_pcm(O.payload_for(1), channels=2)[:9000]):
        out, res, npre = rx.decode_stream(pcm)
        assert npre == 0 and len(res) == 0
        assert O.decode(pcm)[1].status == 1


def test_device_entry(rx):
    import torch
    import modem_amd.ofdmrx as M
    pay = O.payload_for(95, count=4)
    pcm = O.impair(O.encode_pcm(pay, channels=2), noise_db=-30, seed=6, frame=0)
    ho, hr, hn = rx.decode_stream(pcm)
    d_pcm = torch.from_numpy(pcm).cuda()
    d_out = torch.zeros((8, 5380), dtype=torch.uint8, device="cuda")
    d_res = torch.zeros((8, M.RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = rx.decode_stream_device(d_pcm.data_ptr(), 0, 2, len(pcm), 8, d_out.data_ptr(), d_res.data_ptr())
    rx.synchronize()
    assert n == hn == 4
    assert (d_out.cpu().numpy()[:4] == ho).all()
    assert (d_res.cpu().numpy()[:4].view(M.RESULT_DTYPE).ravel() == hr).all()
    p_out = torch.zeros((8, 5380), dtype=torch.uint8).pin_memory()
    p_res = torch.zeros((8, M.RESULT_DTYPE.itemsize), dtype=torch.uint8).pin_memory()
    n = rx.decode_stream_device(d_pcm.data_ptr(), 0, 2, len(pcm), 8, p_out.data_ptr(), p_res.data_ptr())
    rx.synchronize()
    assert n == 4 and (p_out.numpy()[:4] == ho).all() and (p_res.numpy()[:4].view(M.RESULT_DTYPE).ravel() == hr).all()


def test_keep_raw_cons_taps():
    r = _rx(8000, keep_raw_cons=True)
    try:
        pay = O.payload_for(97, count=2)
        pcm = O.impair(O.encode_pcm(pay, channels=2), noise_db=-25, seed=8, frame=0)
        out, res, npre = r.decode_stream(pcm)
        assert npre == 2 and r._lib.ofdmrx_last_chunk_first_frame(r._h) == 0
        for k in range(2):
            o, orr, tb = O.decode(pcm, skip=k, taps=True)
            assert (out[k] == o).all() and int(res[k]["sc_start"]) == orr.sc_start
            np.testing.assert_allclose(r.tap("CONS_RAW", k), tb.cons_raw[:21600], rtol=0, atol=2e-4)
            np.testing.assert_allclose(r.tap("LLR", k)[:64800], tb.llr[:64800], rtol=1e-3, atol=2e-3)
    finally:
        r.close()


@pytest.mark.parametrize("rate", [8000, 48000])
def test_debug_edges_match_serial(rate):
    r = _rx(rate)
    try:
        ml, hs, gl = RATES[rate]
        for seed in range(2):
            t = adversarial(1 << 20, seed, ml)
            te, tm, im, n = r.debug_stream_edges(t)
            se, st, si = serial_edges(t, ml, hs, gl)
            assert n == len(se) > 100
            np.testing.assert_array_equal(te, se)
            np.testing.assert_array_equal(tm, st)
            np.testing.assert_array_equal(im, si)
    finally:
        r.close()


def test_cli(tmp_path):
    """`encode` with four payload files, `decode_stream`: every OUTDIR/k.dat is what `decode OUT x.wav k` writes, and the payload"""
    import os
    import subprocess
    bin_dir = os.path.join(O.ROOT, "modem_amd", "bin")
    files = []
    for i in range(4):
        f = tmp_path / ("p%d.dat" % i)
        f.write_bytes(bytes(O.payload_for(1700 + i)))
        files.append(f)
    wav = tmp_path / "x.wav"
    subprocess.check_call([os.path.join(bin_dir, "encode"), str(wav), "8000", "16", "2", "1500", "6", "CALL 1"] + [str(f) for f in files])
    outdir = tmp_path / "out"
    outdir.mkdir()
    p = subprocess.run([os.path.join(bin_dir, "decode_stream"), str(outdir), str(wav)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert len(p.stderr.strip().splitlines()) == 4 and sorted(os.listdir(outdir)) == ["%d.dat" % k for k in range(4)]
    for k in range(4):
        one = tmp_path / ("one%d.dat" % k)
        subprocess.check_call([os.path.join(bin_dir, "decode"), str(one), str(wav), str(k)], stderr=subprocess.DEVNULL)
        got = (outdir / ("%d.dat" % k)).read_bytes()
        assert got == one.read_bytes() and got == files[k].read_bytes(), k
    bad = subprocess.run([os.path.join(bin_dir, "decode_stream"), str(outdir), str(tmp_path / "missing.wav")], capture_output=True)
    assert bad.returncode == 1
