"""The live feed (ofdmrx_feed_*): a recording pushed block by block gives the records ofdmrx_decode_stream gives
for the whole recording - byte for byte with 2-channel input, however the stream is cut - each one as soon as its frame is in."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import feed_fixture as F
import oracle_lib as O

pytestmark = pytest.mark.gpu

REL = 1e-5
TILE = 4096
E_ARG = -1


def _flips_ok(gpu, oracle):
    return abs(int(gpu) - int(oracle)) <= (2 if int(oracle) > 0 else 0)


def _rx(rate=8000, **kw):
    import modem_amd
    return modem_amd.Receiver(device=0, chunk_frames=16, sample_rate=rate, **kw)


@pytest.fixture(scope="module")
def rx():
    r = _rx()
    yield r
    r.close()


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


def _cat(parts):
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _feed_cuts(r, pcm, cuts, **kw):
    """the recording pushed in the pieces the cut positions make of it (equal neighbours: a zero-length push) -> (payloads, results)"""
    pcm = pcm if pcm.ndim == 2 else pcm[:, None]
    got = []
    with r.feed(pcm.shape[1], pcm.dtype, **kw) as f:
        edges = [0] + [int(c) for c in cuts] + [len(pcm)]
        for a, b in zip(edges[:-1], edges[1:]):
            got.append(f.push(pcm[a:b]))
        got.append(f.end())
        assert not f.open
    return _cat(got)


def _blocks(n, size):
    return list(range(size, n, size))


def _same(got, want):
    assert len(got[1]) == len(want[1]), (len(got[1]), len(want[1]))
    assert got[0].tobytes() == want[0].tobytes()
    assert got[1].tobytes() == want[1].tobytes()


@functools.lru_cache(maxsize=None)
def _three():
    pay = O.payload_for(300, count=3)
    pcm = O.impair(O.encode_pcm(pay, channels=2), noise_db=-30, seed=11, frame=0)
    pcm.setflags(write=False)
    return pcm


@functools.lru_cache(maxsize=None)
def _mixed2():
    pcm, _ = _mixed(2)
    pcm.setflags(write=False)
    return pcm


@pytest.fixture(scope="module")
def three_truth(rx):
    out, res, npre = rx.decode_stream(_three())
    assert npre == 3 and (res["status"] == 0).all()
    return out, res


@pytest.fixture(scope="module")
def mixed_truth(rx):
    out, res, npre = rx.decode_stream(_mixed2())
    assert npre == len(res) >= 9
    return out, res


def _cut_sets(name, n, truth):
    if name == "one":
        return []
    if name == "8000":
        return _blocks(n, 8000)
    if name == "4096":
        return _blocks(n, 4096)
    if name == "4095":
        return _blocks(n, 4095)
    if name == "4097":
        return _blocks(n, 4097)
    if name == "random":
        rng = np.random.default_rng(7)
        sizes = [int(x) for x in rng.integers(1, 20001, size=n // 5000)]      # (more than the recording takes)
        for extra in (1, 0):                                     # a one-sample and a zero-length push among the first of them
            sizes.insert(int(rng.integers(1, 10)), extra)
        cuts = np.cumsum(sizes)
        assert cuts[-1] >= n and cuts[11] < n
        return [int(c) for c in cuts[cuts < n]]
    sc = sorted(int(s) for s in truth[1]["sc_start"])
    return sc if name == "sc_start" else [s + 1 for s in sc]


@pytest.mark.parametrize("cuts", ["one", "8000", "4096", "4095", "4097", "random", "sc_start", "sc_start+1"])
def test_cuts_two_channel(rx, three_truth, cuts):
    pcm = _three()
    c = _cut_sets(cuts, len(pcm), three_truth)
    if cuts == "random":
        d = np.diff([0] + c)
        assert (d == 0).any() and (d == 1).any()
    _same(_feed_cuts(rx, pcm, c), three_truth)


def test_mixed_two_channel(rx, mixed_truth):
    pcm = _mixed2()
    _same(_feed_cuts(rx, pcm, _blocks(len(pcm), 8000)), mixed_truth)


def test_mixed_mono(rx):
    pcm, _ = _mixed(1)
    out, res, npre = rx.decode_stream(pcm)
    fo, fr = _feed_cuts(rx, pcm, _blocks(len(pcm), 8000))
    F.check("feed_mixed_mono", pcm, np.diff([0] + _blocks(len(pcm), 8000) + [len(pcm)]), (fo, fr))   # the recorded single-window feed
    assert len(fr) == npre == len(res)
    assert fo.tobytes() == out.tobytes()
    for name in ("status", "sc_start", "symbol_pos", "n_sync_rejects", "oper_mode", "call_sign", "best_lane"):
        assert (fr[name] == res[name]).all(), name
    for name in ("cfo_rad", "cfo_fine", "sfo_slope", "esn0_db_last"):
        assert np.abs(fr[name].astype(np.float64) - res[name].astype(np.float64)).max() <= REL, name
    assert all(_flips_ok(a, b) for a, b in zip(fr["bit_flips"], res["bit_flips"]))
    assert _check_records(fo, fr, len(fr), pcm) >= 8


def test_due_times(rx, mixed_truth):
    """each record leaves with the push that brings the last sample of its frame (destroyed header: of its header symbol, once the
    scan's tile is complete); the frame the recording cuts off leaves with end()"""
    import modem_amd.ofdmrx as M
    pcm = _mixed2()
    rate, block = 8000, 2000
    stride = 1440 * rate // 8000
    buffer_len = 6 * stride
    fs = rx._lib.ofdmrx_frame_samples
    at = []
    with rx.feed(2) as f:
        lag = f.lag
        assert 0 <= lag <= stride
        for a in range(0, len(pcm), block):
            o, r = f.push(pcm[a:a + block])
            at += [min(a + block, len(pcm))] * len(r)
        n_pushed = len(at)
        o, r = f.end()
        at += [None] * len(r)
    res = mixed_truth[1]
    assert len(at) == len(res)
    assert n_pushed == len(res) - 1 and at[-1] is None           # the cut-off last frame: only end() returns it
    failed = 0
    for k in range(n_pushed):
        sc = int(res[k]["sc_start"])
        if int(res[k]["status"]) in (0, 6):
            bound = sc + fs(rate, int(res[k]["oper_mode"])) - 2 * rate + lag
        else:
            bound = sc + buffer_len + TILE + lag
            failed += 1
        assert at[k] - block <= bound, (k, at[k], bound)
    assert failed == 1


def test_bounded_window(rx):
    import modem_amd.ofdmrx as M
    rng = np.random.default_rng(21)
    n, block = 2_000_000, 65536
    pcm = rng.normal(0, 300, size=(n, 2)).astype(np.int16)
    for i, at in enumerate((300_000, 1_500_000)):
        fr = O.encode_pcm(O.payload_for(400 + i), channels=2)
        pcm[at:at + len(fr)] = np.clip(pcm[at:at + len(fr)].astype(np.int32) + fr, -32768, 32767).astype(np.int16)
    rate = 8000
    bound = rx._lib.ofdmrx_frame_samples(rate, 13) + 6 * 1440 + 3 * TILE + block
    got = []
    with rx.feed(2) as f:
        for a in range(0, n, block):
            got.append(f.push(pcm[a:a + block]))
            assert f.resident_samples <= bound, (a, f.resident_samples, bound)
        got.append(f.end())
    out, res, npre = rx.decode_stream(pcm)
    assert npre >= 2 and (res["status"] == 0).sum() == 2
    _same(_cat(got), (out, res))


def test_max_frames_and_draining(rx):
    import modem_amd.ofdmrx as M
    L, h = rx._lib, rx._h
    pay = O.payload_for(500, count=4)
    pcm = O.encode_pcm(pay, channels=2)
    want_o, want_r, npre = rx.decode_stream(pcm)
    assert npre == 4
    out = np.full((4, 5380), 0xA5, np.uint8)
    res = np.zeros(4, M.RESULT_DTYPE)
    res["status"] = 77
    nrec, nleft = C.c_size_t(9), C.c_size_t(9)
    assert L.ofdmrx_feed_begin(h, 0, 2) == 0
    try:
        assert L.ofdmrx_feed_push(h, M._ptr(pcm), len(pcm), 1, M._ptr(out), M._ptr(res), C.byref(nrec), C.byref(nleft)) == 0
        ready = nrec.value + nleft.value                          # (the last frame ends before the recording's trailing silence does)
        assert nrec.value == 1 and nleft.value == ready - 1 and ready >= 3
        assert (res["status"][1:] == 77).all() and (out[1:] == 0xA5).all()
        got_o, got_r = [out[:1].copy()], [res[:1].copy()]
        assert L.ofdmrx_feed_push(h, None, 0, 1, M._ptr(out), M._ptr(res), C.byref(nrec), C.byref(nleft)) == 0
        assert nrec.value == 1 and nleft.value == ready - 2
        assert (res["status"][1:] == 77).all() and (out[1:] == 0xA5).all()
        got_o.append(out[:1].copy())
        got_r.append(res[:1].copy())
        assert L.ofdmrx_feed_push(h, None, 0, 0, None, None, C.byref(nrec), C.byref(nleft)) == 0
        assert nrec.value == 0 and nleft.value == ready - 2
        assert L.ofdmrx_feed_end(h, 1, M._ptr(out), M._ptr(res), C.byref(nrec), C.byref(nleft)) == 0
        assert nrec.value == 1 and nleft.value == 1
        got_o.append(out[:1].copy())
        got_r.append(res[:1].copy())
        assert L.ofdmrx_feed_lag(h) == 0                          # still open: one record is left
        assert L.ofdmrx_feed_end(h, 4, M._ptr(out), M._ptr(res), C.byref(nrec), C.byref(nleft)) == 0
        assert nrec.value == 1 and nleft.value == 0
        assert (res["status"][1:] == 77).all() and (out[1:] == 0xA5).all()
        got_o.append(out[:1].copy())
        got_r.append(res[:1].copy())
        assert L.ofdmrx_feed_lag(h) == E_ARG                      # closed
    finally:
        while L.ofdmrx_feed_lag(h) >= 0:
            L.ofdmrx_feed_end(h, 4, M._ptr(out), M._ptr(res), C.byref(nrec), C.byref(nleft))
    _same((np.concatenate(got_o), np.concatenate(got_r)), (want_o, want_r))
    assert (want_o == pay.reshape(4, -1)).all()


def test_rate_48k_two_channel():
    r = _rx(48000)
    try:
        pay = O.payload_for(60, count=2)
        pcm = O.impair(O.encode_pcm(pay, channels=2, rate=48000), noise_db=-30, seed=2, frame=0, rate=48000)
        out, res, npre = r.decode_stream(pcm)
        assert npre == 2 and (out == pay.reshape(2, -1)).all()
        _same(_feed_cuts(r, pcm, _blocks(len(pcm), 48000)), (out, res))
    finally:
        r.close()


def test_rate_44k_mono():
    r = _rx(44100)
    try:
        pay = O.payload_for(61, count=2)
        pcm = O.impair(O.encode_pcm(pay, channels=2, rate=44100), noise_db=-30, seed=2, frame=0, rate=44100)
        pcm = np.ascontiguousarray(pcm[:, :1])
        fo, fr = _feed_cuts(r, pcm, _blocks(len(pcm), 44100))
        F.check("feed_44k_mono", pcm, np.diff([0] + _blocks(len(pcm), 44100) + [len(pcm)]), (fo, fr))
        assert _check_records(fo, fr, len(fr), pcm, rate=44100, payloads=pay.reshape(2, -1)) == 2
    finally:
        r.close()


@pytest.mark.parametrize("fmt", ["u8", "f32"])
def test_formats(rx, fmt):
    pay = O.payload_for(70, count=2)
    pcm = O.encode_pcm(pay, channels=2, bits=8 if fmt == "u8" else 16)
    if fmt == "f32":
        pcm = O.pcm_to_cf(pcm)
    out, res, npre = rx.decode_stream(pcm)
    assert npre == 2 and (out == pay.reshape(2, -1)).all()
    _same(_feed_cuts(rx, pcm, _blocks(len(pcm), 8000)), (out, res))


def test_lifecycle(rx, three_truth):
    import modem_amd.ofdmrx as M
    L, h = rx._lib, rx._h
    pcm = _three()
    out = np.zeros((4, 5380), np.uint8)
    res = np.zeros(4, M.RESULT_DTYPE)
    nrec, nleft, npre = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    a = (M._ptr(out), M._ptr(res), C.byref(nrec), C.byref(nleft))
    one = rx.decode(pcm[None, :95200])
    # without a feed
    assert L.ofdmrx_feed_push(h, M._ptr(pcm), 100, 4, *a) == E_ARG
    assert L.ofdmrx_feed_end(h, 4, *a) == E_ARG
    assert L.ofdmrx_feed_lag(h) == E_ARG and L.ofdmrx_feed_resident_samples(h) == E_ARG
    assert L.ofdmrx_feed_begin(h, 3, 2) == E_ARG and L.ofdmrx_feed_begin(h, 0, 3) == E_ARG and L.ofdmrx_feed_begin(h, 0, 0) == E_ARG
    assert L.ofdmrx_feed_begin(h, 0, 2) == 0
    try:
        assert L.ofdmrx_feed_begin(h, 0, 2) == E_ARG             # one feed per handle
        assert L.ofdmrx_bank_begin(h, 1, 0, 2) == E_ARG          # ... and no bank beside it; the bank entries refuse the feed
        rc, ri, one_len = np.zeros(4, np.int32), np.zeros(4, np.int64), np.zeros(1, np.uintp)
        ba = (M._ptr(out), M._ptr(res), M._ptr(rc), M._ptr(ri), C.byref(nrec), C.byref(nleft))
        assert L.ofdmrx_bank_push(h, None, 0, M._ptr(one_len), None, 4, *ba) == E_ARG and L.ofdmrx_bank_end(h, 4, *ba) == E_ARG
        assert L.ofdmrx_bank_resident_samples(h, 0) == E_ARG and L.ofdmrx_bank_preambles(h, 0) == E_ARG
        assert L.ofdmrx_bank_last_stage_ops(h) == E_ARG
        assert L.ofdmrx_feed_lag(h) == 0                         # (still open)
        assert L.ofdmrx_feed_push(h, None, 100, 4, *a) == E_ARG
        assert L.ofdmrx_feed_push(h, M._ptr(pcm), 100, 4, None, M._ptr(res), C.byref(nrec), C.byref(nleft)) == E_ARG
        assert L.ofdmrx_feed_push(h, M._ptr(pcm), 100, 4, M._ptr(out), None, C.byref(nrec), C.byref(nleft)) == E_ARG
        assert L.ofdmrx_feed_push(h, M._ptr(pcm), 100, 4, M._ptr(out), M._ptr(res), None, C.byref(nleft)) == E_ARG
        assert L.ofdmrx_feed_push(h, M._ptr(pcm), 100, 4, M._ptr(out), M._ptr(res), C.byref(nrec), None) == E_ARG
        assert L.ofdmrx_feed_push(h, C.c_void_p(pcm.ctypes.data + 2), 100, 4, *a) == E_ARG   # not on an I/Q pair
        assert L.ofdmrx_feed_end(h, 4, None, M._ptr(res), C.byref(nrec), C.byref(nleft)) == E_ARG
        # the other decode entries refuse a handle with an open feed
        assert L.ofdmrx_decode_stream(h, M._ptr(pcm), 0, 2, len(pcm), 4, M._ptr(out), M._ptr(res), C.byref(npre)) == E_ARG
        assert L.ofdmrx_decode_stream_device(h, M._ptr(pcm), 0, 2, len(pcm), 4, M._ptr(out), M._ptr(res), C.byref(npre)) == E_ARG
        assert L.ofdmrx_decode_batch(h, M._ptr(pcm), 0, 2, 95200, 95200 * 4, 1, None, M._ptr(out), M._ptr(res)) == E_ARG
        assert L.ofdmrx_decode_batch_device(h, M._ptr(pcm), 0, 2, 95200, 95200 * 4, 1, None, M._ptr(out), M._ptr(res)) == E_ARG
        assert L.ofdmrx_feed_push(h, M._ptr(pcm), 0, 0, None, None, C.byref(nrec), C.byref(nleft)) == 0   # nothing in, nothing asked
        assert L.ofdmrx_feed_resident_samples(h) == 0
    finally:
        assert L.ofdmrx_feed_end(h, 4, *a) == 0 and nrec.value == 0 and nleft.value == 0
    # two feeds in a row: positions and record numbers start over
    for _ in range(2):
        _same(_feed_cuts(rx, pcm, _blocks(len(pcm), 30000)), three_truth)
    # ... and the one-call and batch entries answer as before
    o2, r2, n2 = rx.decode_stream(pcm)
    assert n2 == 3
    _same((o2, r2), three_truth)
    again = rx.decode(pcm[None, :95200])
    assert again[0].tobytes() == one[0].tobytes() and again[1].tobytes() == one[1].tobytes()
    # a handle destroyed with an open feed frees it
    r = _rx()
    f = r.feed(2)
    f.push(pcm[:50000])
    r.close()


def test_positions_past_2_31(rx):
    """positions are 64-bit: a frame behind more than 2^31 samples of silence decodes as the same frame behind a little silence.
    Mono 8-bit input (one byte per sample; all three windows - samples, DC-blocker states, analytic signal - are in use); silence
    leaves the DC blocker's state at exactly 0 and the two lead-ins differ by a multiple of the scan's tile (4096) and of the front
    end's stretch (7936), so every byte of the result but sc_start is the same."""
    unit = 4096 * 31                                             # lcm(4096, 7936)
    block = np.full(unit * 512, 128, np.uint8)                   # 65 011 712 samples of silence, pushed again and again
    frame = O.encode_pcm(O.payload_for(600), channels=1, bits=8).reshape(-1)
    got = {}
    for name, lead in (("near", [block[:unit]]), ("far", [block] * 34)):
        parts = []
        with rx.feed(1, np.uint8) as f:
            for b in lead:
                parts.append(f.push(b))
            assert f.resident_samples <= rx._lib.ofdmrx_frame_samples(8000, 13) + 6 * 1440 + 3 * TILE + len(block)
            parts.append(f.push(frame))
            parts.append(f.end())
        got[name] = _cat(parts) + (sum(len(b) for b in lead),)
    (no, nr, nz), (fo, fr, fz) = got["near"], got["far"]
    assert fz > 2 ** 31 and len(nr) == len(fr) == 1 and int(nr["status"][0]) == 0
    assert fo.tobytes() == no.tobytes() and (fo[0] == O.payload_for(600)).all()
    assert int(fr["sc_start"][0]) - int(nr["sc_start"][0]) == fz - nz and int(fr["sc_start"][0]) > 2 ** 31
    fr = fr.copy()
    fr["sc_start"] = nr["sc_start"]
    assert fr.tobytes() == nr.tobytes()


def test_esn0_rows(rx):
    pcm = _three()
    out, res, npre, rows = rx.decode_stream(pcm, esn0_rows=True)
    got = []
    with rx.feed(2, esn0_rows=True) as f:
        for a in range(0, len(pcm), 50000):
            got.append(f.push(pcm[a:a + 50000]))
        got.append(f.end())
    fo = np.concatenate([g[0] for g in got])
    frows = np.concatenate([g[2] for g in got])
    assert fo.tobytes() == out.tobytes() and frows.shape == rows.shape == (3, 126)
    assert frows.tobytes() == rows.tobytes() and (rows[:, :50] != 0).all()


def test_cli_live(tmp_path):
    """`decode_stream --live` on a file and on a pipe: the files and the stderr lines of `decode_stream` without it"""
    bin_dir = os.path.join(O.ROOT, "modem_amd", "bin")
    files = []
    for i in range(4):
        f = tmp_path / ("p%d.dat" % i)
        f.write_bytes(bytes(O.payload_for(1800 + i)))
        files.append(f)
    wav = tmp_path / "x.wav"
    subprocess.check_call([os.path.join(bin_dir, "encode"), str(wav), "8000", "16", "2", "1500", "6", "CALL 1"] + [str(f) for f in files])
    runs = {}
    for name, args, stdin in (("plain", [str(wav)], None), ("live", ["--live", str(wav)], None), ("pipe", ["--live", "-"], wav)):
        outdir = tmp_path / name
        outdir.mkdir()
        argv = [os.path.join(bin_dir, "decode_stream")] + args[:-1] + [str(outdir), args[-1]]
        with (open(stdin, "rb") if stdin else open(os.devnull, "rb")) as inp:
            p = subprocess.run(argv, stdin=inp, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        runs[name] = (p.stderr, {k: (outdir / k).read_bytes() for k in sorted(os.listdir(outdir))})
    assert sorted(runs["plain"][1]) == ["%d.dat" % k for k in range(4)]
    assert len(runs["plain"][0].strip().splitlines()) == 4
    for k in range(4):
        assert runs["plain"][1]["%d.dat" % k] == files[k].read_bytes()
    assert runs["live"] == runs["plain"] and runs["pipe"] == runs["plain"]
