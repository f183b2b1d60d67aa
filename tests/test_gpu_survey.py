"""The wideband survey on the device (k_survey.hip behind ofdmrx_util_survey) against the float64 model of survey_model.py (DESIGN.md
section 4.16): |got - P| <= tol on every bin of every row, nothing exempt; the tolerance is derived in the model's header.  Every
output buffer is filled with a sentinel first and has a spare row behind the last, which must come back untouched.  Each test
prints its worst |got - P| / tol (profiles/survey_parity.txt keeps them).  Then the contract of the summation order - one call
against pieces, as bytes - the refusals, the loop survey -> find_bands -> wideband bank on the capture of wideband_fixture.py, and
the command line."""
import ctypes as C
import os
import subprocess
import wave

import numpy as np
import pytest

import channelize_model as CM
import survey_model as SM
import wideband_fixture as WF

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
G = SM.G
FMT = {np.dtype(np.int16): 0, np.dtype(np.uint8): 1, np.dtype(np.float32): 2}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RW = float(WF.DECIM * WF.RATE)


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1)
    yield r
    r.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")     # (a copy: the shared fixtures are read-only)


def _call(rx, d_in, fmt, in_first, n_in, N, S, row_first, n_rows, d_out):
    return rx._lib.ofdmrx_util_survey(rx._h, d_in, fmt, in_first, n_in, N, S, row_first, n_rows, d_out)


def _run(rx, pcm, N, S, row_first=0, n_rows=1, in_first=0):
    """-> [n_rows, N] float32 from the device; checks the spare row"""
    import torch
    pcm = np.ascontiguousarray(pcm)
    out = torch.full((n_rows + 1, N), SENTINEL, dtype=torch.float32, device="cuda:0")
    d_in = _dev(pcm)
    torch.cuda.synchronize()                                         # the handle has a stream of its own
    assert _call(rx, d_in.data_ptr(), FMT[pcm.dtype], in_first, len(pcm), N, S, row_first, n_rows, out.data_ptr()) == 0
    rx.synchronize()
    got = out.cpu().numpy()
    assert (got[n_rows] == SENTINEL).all()
    return got[:n_rows]


def _check(rx, pcm, N, S, what, **kw):
    got = _run(rx, pcm, N, S, **kw)
    P, tol = SM.psd(pcm, N, S, row_first=kw.get("row_first", 0), n_rows=kw.get("n_rows", 1), in_first=kw.get("in_first", 0))
    assert got.shape == P.shape and np.isfinite(got).all() and (got >= 0).all()
    w = SM.worst(got, P, tol)
    print("survey N %d S %d %s: %d rows, worst |got - P| / tol %.4f" % (N, S, what, P.shape[0], w))
    assert w <= 1.0, (N, S, what, w)
    return got, w


def _len(N, S, rows, extra=0):
    """positions that rows 0 .. rows - 1 of S segments need, and a few more"""
    return (N // 2) * (rows * S + 1) + extra


@pytest.mark.parametrize("n_rows", [1, 3])
@pytest.mark.parametrize("S", [1, 2, G, G + 1, 2 * G + 1])
def test_rows_match_model(rx, S, n_rows):
    """one segment, two, a whole group, a group and one, two groups and one; one row and three"""
    pcm = CM.random_pcm(_len(1280, S, n_rows, 7), np.int16, seed=10 * S + n_rows)
    _check(rx, pcm, 1280, S, "int16", n_rows=n_rows)


@pytest.mark.parametrize("N", [2560, 5120])
def test_longer_transforms_match_model(rx, N):
    pcm = CM.random_pcm(_len(N, 2, 2, 3), np.int16, seed=N)
    _check(rx, pcm, N, 2, "int16", n_rows=2)


@pytest.mark.parametrize("N", SM.NFFT)
def test_formats(rx, N):
    """U8 and F32 input; F32 input scaled by 2^12 gives exactly the outputs scaled by 2^24"""
    n = _len(N, 3, 2, 1)
    _check(rx, CM.random_pcm(n, np.uint8, seed=2), N, 3, "u8", n_rows=2)
    x = CM.random_pcm(n, np.float32, seed=3)
    got, _ = _check(rx, x, N, 3, "f32", n_rows=2)
    big, _ = _check(rx, x * np.float32(4096.0), N, 3, "f32 x 4096", n_rows=2)
    assert (big == got * np.float32(4096.0 * 4096.0)).all()


@pytest.mark.parametrize("N", SM.NFFT)
def test_tones_and_silence(rx, N):
    """a tone on a bin centre (the other bins hold only what the tolerance allows), a tone between two bins, and all-zero input:
    every output +0"""
    n = np.arange(_len(N, 3, 2))
    for k0, what in ((N // 5, "tone on a bin"), (-N // 3 + 0.5, "tone between bins")):
        x = 0.5 * np.exp(2j * np.pi * k0 * n / N)
        pcm = np.rint(np.stack([x.real, x.imag], axis=1) * 32767.0).astype(np.int16)
        got, _ = _check(rx, pcm, N, 3, what, n_rows=2)
        assert abs(int(got[0].argmax()) - (k0 + N // 2)) <= 0.5
    got = _run(rx, np.zeros((len(n), 2), np.int16), N, 3, n_rows=2)
    assert (got.view(np.uint32) == 0).all()
    got = _run(rx, np.zeros((len(n), 2), np.float32), N, 3, n_rows=2)
    assert (got.view(np.uint32) == 0).all()


def test_far_positions(rx):
    """a row whose first position lies above 2^41: the buffer holds just that row"""
    N, S = 1280, 2
    row_first = 2 ** 31 + 5
    pcm = CM.random_pcm(_len(N, S, 1), np.int16, seed=41)
    _check(rx, pcm, N, S, "row_first 2^31 + 5", row_first=row_first, n_rows=1, in_first=row_first * S * (N // 2))


@pytest.mark.parametrize("N,S", [(1280, 2 * G + 1), (2560, 3)])
def test_one_call_equals_pieces_as_bytes(rx, N, S):
    """the whole capture in one call; row by row, each call given only the samples its row needs; rows 2 .. on the full buffer"""
    H, rows = N // 2, 4
    pcm = CM.random_pcm(_len(N, S, rows, 11), np.int16, seed=N + 1)
    whole = _run(rx, pcm, N, S, n_rows=rows)
    for r in range(rows):
        lo, hi = r * S * H, (r + 1) * S * H + H
        piece = _run(rx, pcm[lo:hi], N, S, row_first=r, n_rows=1, in_first=lo)
        assert piece.tobytes() == whole[r:r + 1].tobytes(), r
    tail = _run(rx, pcm, N, S, row_first=2, n_rows=rows - 2)
    assert tail.tobytes() == whole[2:].tobytes()


def test_back_to_back_calls_with_different_lengths(rx):
    """two calls on the stream, nothing between them: the second's tables and partial sums do not disturb the first"""
    import torch
    pcm = CM.random_pcm(_len(5120, 3, 2, 5), np.int16, seed=77)
    want = {N: _run(rx, pcm, N, 3, n_rows=2) for N in (1280, 5120)}
    d_in = _dev(pcm)
    outs = {N: torch.full((3, N), SENTINEL, dtype=torch.float32, device="cuda:0") for N in (1280, 5120, 2560)}
    torch.cuda.synchronize()
    for N in (5120, 1280, 2560):
        assert _call(rx, d_in.data_ptr(), 0, 0, len(pcm), N, 3, 0, 2, outs[N].data_ptr()) == 0
    rx.synchronize()
    for N in (1280, 5120):
        got = outs[N].cpu().numpy()
        assert got[:2].tobytes() == want[N].tobytes() and (got[2] == SENTINEL).all(), N


def test_refusals_leave_the_output_untouched(rx):
    import torch
    N, S = 1280, 2
    pcm = CM.random_pcm(5120, np.int16, seed=5)
    d_in = _dev(pcm)
    out = torch.full((4, N), SENTINEL, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    a = dict(d_in=d_in.data_ptr(), fmt=0, in_first=0, n_in=5120, N=N, S=S, row_first=0, n_rows=2, d_out=out.data_ptr())

    def call(**kw):
        b = dict(a)
        b.update(kw)
        return _call(rx, b["d_in"], b["fmt"], b["in_first"], b["n_in"], b["N"], b["S"], b["row_first"], b["n_rows"], b["d_out"])

    bad = [dict(d_in=None), dict(d_out=None), dict(n_in=0), dict(n_rows=0), dict(fmt=3), dict(fmt=-1), dict(N=1024), dict(N=640), dict(N=0),
           dict(S=0), dict(S=65537), dict(in_first=-1), dict(row_first=-1), dict(n_in=3199), dict(in_first=1), dict(row_first=2, n_rows=2),
           dict(n_rows=4), dict(d_in=d_in.data_ptr() + 2), dict(d_out=out.data_ptr() + 2), dict(d_out=d_in.data_ptr() + 1280),
           dict(in_first=(1 << 50) + 1), dict(n_in=(1 << 50) + 1), dict(n_rows=(1 << 50) + 1), dict(S=8, n_rows=(1 << 28) // 1280 + 1, n_in=1 << 40)]
    for kw in bad:
        assert call(**kw) == -1, kw
    rx.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and (d_in.cpu().numpy() == pcm).all()
    bank = rx.wideband_bank([1000.0], 6)                             # a handle with an open bank surveys nothing
    try:
        assert call() == -1
    finally:
        while bank.open:
            bank.end()
    rx.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    assert call(n_rows=3, n_in=4480) == 0                            # rows 0 .. 2 end at 4480: exactly what the buffer holds
    rx.synchronize()
    got = out.cpu().numpy()
    assert (got[3] == SENTINEL).all() and (got[:3] != SENTINEL).all()


# ---- the loop on the capture of wideband_fixture.py

@pytest.fixture(scope="module")
def loop(rx):
    """the capture, the device's row over all of it and the bands found in it: computed once, read only"""
    import modem_amd
    pcm, pays = WF.capture()
    row = rx.survey(_dev(pcm), modem_amd.FMT_S16, nfft=1280).cpu().numpy()
    bands = modem_amd.find_bands(row[0], RW)
    for a in (pcm, pays, row):
        a.setflags(write=False)
    return pcm, pays, row, bands


def test_receiver_survey_finds_the_models_bands(rx, loop):
    import modem_amd
    pcm, pays, row, bands = loop
    assert row.shape == (1, 1280) and row.dtype == np.float32
    P, tol = SM.psd(pcm, 1280)
    w = SM.worst(row, P, tol)
    print("survey N 1280 fixture capture, %d segments: worst |got - P| / tol %.4f" % (SM.n_segments(len(pcm), 1280), w))
    assert w <= 1.0
    want, floor = SM.find_bands(P[0], RW)
    assert len(bands) == len(want) == 4
    for b, m, f in zip(bands, want, WF.SIGNAL_HZ):
        assert abs(b["first_bin"] - m["first_bin"]) <= 1 and abs(b["last_bin"] - m["last_bin"]) <= 1, (b, m)
        assert abs(b["centre_hz"] - f) <= RW / 1280
    got, gfl = modem_amd.find_bands(row[0], RW, with_floor=True)
    assert got == bands and abs(gfl / floor - 1.0) < 1e-4
    # the waterfall through the same entry: rows of 64 segments, every whole row the buffer holds
    wf = rx.survey(_dev(pcm), modem_amd.FMT_S16, nfft=1280, segs_per_row=64).cpu().numpy()
    Pw, tolw = SM.psd(pcm, 1280, 64)
    assert wf.shape == Pw.shape == (17, 1280) and SM.worst(wf, Pw, tolw) <= 1.0
    part = rx.survey(_dev(pcm[64 * 640 * 3:]), modem_amd.FMT_S16, nfft=1280, segs_per_row=64, in_first=64 * 640 * 3, row_first=3, n_rows=2)
    assert part.cpu().numpy().tobytes() == wf[3:5].tobytes()


def _by_channel(parts, n_channels):
    pay = np.concatenate([p[0] for p in parts])
    res = np.concatenate([p[1] for p in parts])
    ch = np.concatenate([p[2] for p in parts])
    ix = np.concatenate([p[3] for p in parts])
    return [(pay[ch == c].tobytes(), res[ch == c].tobytes(), list(ix[ch == c])) for c in range(n_channels)]


def test_bank_on_the_found_centres_decodes_every_frame(rx, loop):
    """survey -> find_bands -> wideband_bank(found centres) pushed in blocks: per channel the records equal the one-call decode of
    that channel's ofdmrx_util_channelize row byte for byte, and contain the golden payload with status 0"""
    import torch
    pcm, pays, row, bands = loop
    D = WF.DECIM
    centres = np.array([b["centre_hz"] for b in bands])
    n_out = -(-len(pcm) // D)
    d_in = _dev(pcm)
    d_out = torch.full((len(centres), n_out, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rx.channelize(d_in.data_ptr(), 0, 0, len(pcm), D, centres, 0, n_out, d_out.data_ptr())
    rx.synchronize()
    recs = rx.decode_streams(list(d_out.cpu().numpy()))
    bank = rx.wideband_bank(centres, D)
    parts, at, i = [], 0, 0
    blocks = (48000, 4097, 1, 0, 5, 7 * 4096 + 3)
    try:
        while at < len(pcm):
            n = min(blocks[i % len(blocks)], len(pcm) - at)
            parts.append(bank.push(pcm[at:at + n]))
            at += n
            i += 1
        parts.append(bank.end())
    finally:
        while bank.open:
            bank.end()
    got = _by_channel(parts, len(centres))
    for c, (out, res, npre) in enumerate(recs):
        assert got[c][2] == list(range(npre)), c
        assert got[c][0] == out.tobytes() and got[c][1] == res.tobytes(), c
        ok = [k for k in range(npre) if int(res[k]["status"]) == 0]
        assert len(ok) == 1 and (out[ok[0]] == pays[c]).all(), (c, [int(r["status"]) for r in res[:npre]])


def _write_wav(path, pcm, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(pcm).tobytes())


def test_command_line(loop, tmp_path):
    """`survey` prints the four bands; `decode_stream --wideband 6 auto` writes the four payload files; `auto -` and a capture
    without bands are refused"""
    pcm, pays, row, bands = loop
    wav = tmp_path / "wide.wav"
    _write_wav(wav, pcm, int(RW))
    exe = os.path.join(ROOT, "modem_amd", "bin", "survey")
    p = subprocess.run([exe, str(wav), str(WF.DECIM)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "floor" in p.stderr, p.stderr
    lines = [[float(v) for v in l.split()] for l in p.stdout.splitlines()]
    assert len(lines) == 4
    for l, b in zip(lines, bands):
        assert abs(l[0] - b["centre_hz"]) <= 0.01 and abs(l[1] - b["width_hz"]) <= 0.01 and abs(l[2] - b["level_db"]) <= 0.01
    p = subprocess.run([exe, str(wav), str(WF.DECIM), "1000"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1
    dec = os.path.join(ROOT, "modem_amd", "bin", "decode_stream")
    root = tmp_path / "out"
    p = subprocess.run([dec, "--wideband", str(WF.DECIM), "auto", str(root), str(wav)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "survey: floor" in p.stderr, p.stderr
    for c in range(4):
        files = sorted(os.listdir(root / str(c)))
        hits = [f for f in files if (root / str(c) / f).read_bytes() == pays[c].tobytes()]
        assert len(hits) == 1, (c, files)
    byhand = tmp_path / "byhand"
    q = subprocess.run([dec, "--wideband", str(WF.DECIM), ",".join("%.17g" % b["centre_hz"] for b in bands), str(byhand), str(wav)],
                       capture_output=True, text=True, timeout=120)
    assert q.returncode == 0
    assert [l for l in q.stderr.splitlines() if ": sample " in l] == [l for l in p.stderr.splitlines() if ": sample " in l]
    p = subprocess.run([dec, "--wideband", str(WF.DECIM), "auto", str(tmp_path / "o2"), "-"], capture_output=True, text=True, timeout=60,
                       stdin=subprocess.DEVNULL)
    assert p.returncode == 1 and "standard input" in p.stderr and not (tmp_path / "o2").exists()
    empty = tmp_path / "empty.wav"
    _write_wav(empty, np.zeros((48000, 2), np.int16), int(RW))
    p = subprocess.run([dec, "--wideband", str(WF.DECIM), "auto", str(tmp_path / "o3"), str(empty)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "no occupied band" in p.stderr and not (tmp_path / "o3").exists()
