"""The grid loop on the device, in the pattern of test_gpu_wideband_loop.py: payloads -> tx_encode (2
channels, freq_off 0, mode 6) -> synthesize_grid (unequal gains, unequal starts on the grid of D) -> awgn_tile on the capture at
-60 dB -> the grid bank and ofdmrx_util_channelize_grid -> payloads.  The capture never leaves the device before it is decoded; it is
copied out once for the checks.  Then the same loop through the command line.
  (1) D = 8: four frames in slots -6, -2, 2 and 6, all 16 slots opened;
  (2) D = 64: two frames in slots 37 and 39, slots 37, 38 and 39 opened - the only capture of millions of samples."""
import os
import subprocess
import wave

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

RATE, MODE, NOISE_DB = 8000, 6, -60.0
CASES = {
    1: dict(D=8, slots=(-6, -2, 2, 6), gains=(0.05, 0.3, 0.2, 0.1), starts=(8, 48008, 96016, 144008), open=tuple(range(-8, 8)),
            blocks=(48000, 4097, 1, 0, 5, 7 * 4096 + 3)),
    2: dict(D=64, slots=(37, 39), gains=(0.3, 0.1), starts=(64 * 7, 64 * 8001), open=(37, 38, 39), blocks=(512000, 70001, 0, 1)),
}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "modem_amd", "bin")


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1)
    yield r
    r.close()


@pytest.fixture(scope="module", params=[1, 2])
def loop(rx, request):
    """the capture made on the device, the rows of the opened slots from the device and their stream decode: computed once per
    case, read only"""
    import torch
    cfg = CASES[request.param]
    D, C = cfg["D"], len(cfg["slots"])
    assert all(s % D == 0 for s in cfg["starts"]) and len(set(cfg["starts"])) == C
    pays = np.stack([O.payload_for(160 + 10 * request.param + c) for c in range(C)])
    n_in = rx.tx_frame_samples(MODE)
    d_pay = torch.from_numpy(pays).to("cuda:0")
    d_pcm = torch.zeros((C, n_in, 2), dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    for c in range(C):
        rx.tx_encode(d_pay[c].data_ptr(), 1, d_pcm[c].data_ptr(), mode=MODE, freq_off=0, channels=2)
    W = max(cfg["starts"]) + (n_in - 1) * D + 24 * D + 1
    d_cap = torch.full((W + 1, 2), 12345, dtype=torch.int16, device="cuda:0")
    rx.synthesize_grid(d_pcm.data_ptr(), 0, n_in, D, cfg["slots"], cfg["starts"], cfg["gains"], 0, W, d_cap.data_ptr(), 0)
    rx.awgn_tile(d_cap.data_ptr(), 1, d_cap.data_ptr(), 1, W, NOISE_DB, 48, 0)
    n_out = -(-W // D)
    d_rows = torch.full((len(cfg["open"]), n_out, 2), 12345.0, dtype=torch.float32, device="cuda:0")
    rx.channelize_grid(d_cap.data_ptr(), 0, 0, W, D, list(cfg["open"]), 0, n_out, d_rows.data_ptr())
    rx.synchronize()
    cap = d_cap.cpu().numpy()
    assert (cap[W] == 12345).all() and cap[:W].min() >= -32767 and np.abs(cap[:W]).max() < 32767      # nothing clipped
    cap = np.ascontiguousarray(cap[:W])
    rows = d_rows.cpu().numpy()
    recs = rx.decode_streams(list(rows))
    own = [int(r[1][0]["sc_start"]) for r in rx.decode_streams([p for p in d_pcm.cpu().numpy()])]
    for a in (cap, pays, rows):
        a.setflags(write=False)
    return cfg, cap, pays, rows, recs, own


def test_every_frame_decodes_from_its_slot(loop):
    """status 0 and the payload from the frame's own slot, where section 4.15 puts it: its own sc_start + 24 + start / D"""
    cfg, cap, pays, rows, recs, own = loop
    for c, k in enumerate(cfg["slots"]):
        out, res, npre = recs[cfg["open"].index(k)]
        ok = [i for i in range(len(res)) if int(res[i]["status"]) == 0]
        assert len(ok) == 1, (k, [int(s) for s in res["status"]])
        i = ok[0]
        assert (out[i] == pays[c]).all() and int(res[i]["bit_flips"]) == 0 and int(res[i]["oper_mode"]) == MODE
        assert abs(int(res[i]["sc_start"]) - (own[c] + 24 + cfg["starts"][c] // cfg["D"])) <= 1, (k, int(res[i]["sc_start"]), own[c])
    for j, k in enumerate(cfg["open"]):                               # no other slot gives a payload
        if k not in cfg["slots"]:
            assert not any(int(s) == 0 for s in recs[j][1]["status"]), k


def _by_channel(parts, n_channels):
    pay = np.concatenate([p[0] for p in parts])
    res = np.concatenate([p[1] for p in parts])
    ch = np.concatenate([p[2] for p in parts])
    ix = np.concatenate([p[3] for p in parts])
    return [(pay[ch == c].tobytes(), res[ch == c].tobytes(), list(ix[ch == c])) for c in range(n_channels)]


def test_bank_equals_the_one_call_decode(rx, loop):
    """section 4.19's contract on a capture made on the device: the capture pushed in uneven blocks through a grid bank gives, per
    opened slot and byte for byte, the payloads and results of the one-call decode of ofdmrx_util_channelize_grid's rows"""
    cfg, cap, pays, rows, recs, own = loop
    blocks = cfg["blocks"]
    bank = rx.wideband_grid_bank(list(cfg["open"]), cfg["D"])
    parts, at, i = [], 0, 0
    try:
        while at < len(cap):
            n = min(blocks[i % len(blocks)], len(cap) - at)
            parts.append(bank.push(cap[at:at + n]))
            at += n
            i += 1
        parts.append(bank.end())
    finally:
        while bank.open:
            bank.end()
    got = _by_channel(parts, len(cfg["open"]))
    for c, (out, res, npre) in enumerate(recs):
        assert got[c][2] == list(range(npre)), c
        assert got[c][0] == out.tobytes() and got[c][1] == res.tobytes(), c


@pytest.mark.parametrize("case", [1, 2])
def test_command_line(tmp_path, case):
    """encode ... 2 0 6 ... per frame -> synthesize --grid -> decode_stream --grid gives the payload files back"""
    cfg = CASES[case]
    D = cfg["D"]
    pays, wavs = [], []
    for i in range(len(cfg["slots"])):
        pay = tmp_path / ("pay%d.bin" % i)
        pay.write_bytes(O.payload_for(180 + 10 * case + i).tobytes())
        wav = tmp_path / ("tx%d.wav" % i)
        p = subprocess.run([os.path.join(BIN, "encode"), str(wav), str(RATE), "16", "2", "0", "6", "ANONYMOUS", str(pay)],
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        pays.append(pay)
        wavs.append(wav)
    gains_db = [20.0 * np.log10(g) for g in cfg["gains"]]
    wide = tmp_path / "wide.wav"
    exe = os.path.join(BIN, "synthesize")
    spec = ["%d:%d:%g:%s" % (k, s, g, w) for k, s, g, w in zip(cfg["slots"], cfg["starts"], gains_db, wavs)]
    p = subprocess.run([exe, "--grid", str(wide), str(D)] + spec, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    with wave.open(str(wide), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (2, 2, D * RATE)
        assert w.getnframes() == max(cfg["starts"]) + (95200 - 1) * D + 24 * D + 1
    root = tmp_path / "out"
    p = subprocess.run([os.path.join(BIN, "decode_stream"), "--grid", str(D), ",".join("%d" % k for k in cfg["slots"]), str(root), str(wide)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    for c in range(len(cfg["slots"])):
        files = sorted(os.listdir(root / str(c)))
        assert any((root / str(c) / f).read_bytes() == pays[c].read_bytes() for f in files), (c, files, p.stderr)
    if case == 1:
        # what the program refuses: a bad interpolation, a slot off the grid or given twice, a start off the grid, the plain form's centre
        for argv, text in ((["--grid", str(wide), "6"] + spec, "power of two"), (["--grid", str(wide), str(D), "8:0:0:%s" % wavs[0]], "SLOT:START:GAIN_DB:IN.wav"),
                           (["--grid", str(wide), str(D), "2.5:0:0:%s" % wavs[0]], "SLOT:START:GAIN_DB:IN.wav"),
                           (["--grid", str(wide), str(D), "2:4:0:%s" % wavs[0]], "SLOT:START:GAIN_DB:IN.wav"),
                           (["--grid", str(wide), str(D), spec[0], spec[0]], "given once"), (["--grid", str(wide)], "usage")):
            q = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=60)
            assert q.returncode == 1 and text in q.stderr, (argv, q.stderr)
