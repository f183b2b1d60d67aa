"""The wideband loop on the device at a rational capture rate: payloads -> tx_encode (2 channels, freq_off 0,
modes 6 and 13) -> synthesize at 25/4 (three channels, unequal gains, starts that 25 does not divide) -> awgn_tile on the capture ->
the ratio wideband bank and ofdmrx_util_channelize_ratio -> payloads.  The capture never leaves the device before it is decoded; it
is copied out once for the checks.  Then the same loop through the command line, and tools/adjacent_channel.py --ratio at a tiny size."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import oracle_lib as O
import rechannelize_model as RM

pytestmark = pytest.mark.gpu

P, Q, RATE = 25, 4, 8000
CENTRES = np.array([-14000.0, 9000.0, -3000.0])
MODES = (6, 13, 6)
GAINS = (0.05, 0.5, 0.2)
STARTS = (7, 50021, 100002)
NOISE_DB = -60.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "modem_amd", "bin")


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1)
    yield r
    r.close()


@pytest.fixture(scope="module")
def loop(rx):
    """the capture made on the device, its channel rows from the device and their stream decode: computed once, read only"""
    import modem_amd
    import torch
    assert all(s % P for s in STARTS)
    pays = np.stack([O.payload_for(40 + c) for c in range(3)])
    spf = [rx.tx_frame_samples(m) for m in MODES]
    n_in = max(spf)
    d_pay = torch.from_numpy(pays).to("cuda:0")
    d_pcm = torch.zeros((3, n_in, 2), dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    for c, m in enumerate(MODES):
        rx.tx_encode(d_pay[c].data_ptr(), 1, d_pcm[c].data_ptr(), mode=m, freq_off=0, channels=2)
    W = max(STARTS) + modem_amd.synthesize_support(n_in, (P, Q))
    d_cap = torch.full((W + 1, 2), 12345, dtype=torch.int16, device="cuda:0")
    rx.synthesize(d_pcm.data_ptr(), 0, n_in, (P, Q), CENTRES, STARTS, GAINS, 0, W, d_cap.data_ptr(), 0)
    rx.awgn_tile(d_cap.data_ptr(), 1, d_cap.data_ptr(), 1, W, NOISE_DB, 48, 0)
    n_out = RM.n_outputs(W, P, Q)
    d_rows = torch.full((3, n_out, 2), 12345.0, dtype=torch.float32, device="cuda:0")
    rx.channelize(d_cap.data_ptr(), 0, 0, W, (P, Q), CENTRES, 0, n_out, d_rows.data_ptr())
    rx.synchronize()
    cap = d_cap.cpu().numpy()
    assert (cap[W] == 12345).all() and cap[:W].min() >= -32767 and np.abs(cap[:W]).max() < 32767      # nothing clipped
    cap = np.ascontiguousarray(cap[:W])
    rows = d_rows.cpu().numpy()
    recs = rx.decode_streams(list(rows))
    own = [int(r[1][0]["sc_start"]) for r in rx.decode_streams([p[:n] for p, n in zip(d_pcm.cpu().numpy(), spf)])]
    for a in (cap, pays, rows):
        a.setflags(write=False)
    return cap, pays, rows, recs, own


def test_every_frame_decodes_from_its_channel(loop):
    cap, pays, rows, recs, own = loop
    for c in range(3):
        out, res, npre = recs[c]
        ok = [k for k in range(len(res)) if int(res[k]["status"]) == 0]
        assert len(ok) == 1, (c, [int(s) for s in res["status"]])
        k = ok[0]
        assert (out[k] == pays[c]).all() and int(res[k]["bit_flips"]) == 0 and int(res[k]["oper_mode"]) == MODES[c]
        assert abs(int(res[k]["sc_start"]) - (own[c] + 24 + STARTS[c] * Q / P)) <= 1, (c, int(res[k]["sc_start"]), own[c])


def _by_channel(parts, n_channels):
    pay = np.concatenate([p[0] for p in parts])
    res = np.concatenate([p[1] for p in parts])
    ch = np.concatenate([p[2] for p in parts])
    ix = np.concatenate([p[3] for p in parts])
    return [(pay[ch == c].tobytes(), res[ch == c].tobytes(), list(ix[ch == c])) for c in range(n_channels)]


@pytest.mark.parametrize("blocks", [(1 << 40,), (50000,), (4097,), (48000, 4097, 1, 0, P - 1, 7 * 4096 + 3)],
                         ids=["one push", "50000", "4097", "mixed"])
def test_ratio_bank_equals_the_one_call_decode(rx, loop, blocks):
    """section 4.17's contract on a capture made on the device: the capture pushed in uneven blocks through a ratio wideband bank
    gives, per channel and byte for byte, the payloads and results of the one-call decode of ofdmrx_util_channelize_ratio's rows"""
    cap, pays, rows, recs, own = loop
    bank = rx.wideband_bank(CENTRES, (P, Q), dtype=np.int16)
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
    got = _by_channel(parts, 3)
    for c, (out, res, npre) in enumerate(recs):
        assert got[c][2] == list(range(npre)), c
        assert got[c][0] == out.tobytes() and got[c][1] == res.tobytes(), c


@pytest.mark.parametrize("c", [0, 1])
def test_oracle_on_the_model_rows_agrees(loop, c):
    """the float64 model of the ratio front end on the device's own capture bytes, then the oracle's decoder: every record of the
    channel agrees in status, payload and sc_start (one channel of either mode)"""
    cap, pays, rows, recs, own = loop
    v, tol, _ = RM.channelize(cap, P, Q, [CENTRES[c]], RATE)
    assert RM.worst(rows[c][None], v, tol) <= 1.0                     # (the device's rows are the model's, within 4.17's tolerance)
    row = np.stack([v[0].real, v[0].imag], axis=1).astype(np.float32)
    out, res, npre = recs[c]
    assert npre >= 1
    for k in range(npre + 1):
        o, r = O.decode(row, skip=k)
        if k == npre:
            assert r.status == 1
            break
        assert r.status == int(res[k]["status"]) and (o == out[k]).all() and r.sc_start == int(res[k]["sc_start"]), (c, k)


def test_command_line(tmp_path):
    """encode ... 2 0 6 ... twice -> synthesize wide.wav 25/4 -> decode_stream --wideband 25/4 gives the two payload files back; a
    ratio that gives no integer rate is refused with a message"""
    pays, wavs = [], []
    for i in range(2):
        pay = tmp_path / ("pay%d.bin" % i)
        pay.write_bytes(O.payload_for(70 + i).tobytes())
        wav = tmp_path / ("tx%d.wav" % i)
        p = subprocess.run([os.path.join(BIN, "encode"), str(wav), str(RATE), "16", "2", "0", "6", "ANONYMOUS", str(pay)],
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        pays.append(pay)
        wavs.append(wav)
    centres, starts, gains = (-14000.0, 9000.0), (7, 50021), (-20.0, -6.0)
    wide = tmp_path / "wide.wav"
    exe = os.path.join(BIN, "synthesize")
    spec = ["%g:%d:%g:%s" % (f, s, g, w) for f, s, g, w in zip(centres, starts, gains, wavs)]
    p = subprocess.run([exe, str(wide), "%d/%d" % (P, Q)] + spec, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    with wave.open(str(wide), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (2, 2, RATE * P // Q)
        assert w.getnframes() == starts[1] + ((95200 - 1 + 24) * P) // Q + 1
    root = tmp_path / "out"
    p = subprocess.run([os.path.join(BIN, "decode_stream"), "--wideband", "%d/%d" % (P, Q), ",".join("%g" % f for f in centres), str(root),
                        str(wide)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    for c in range(2):
        files = sorted(os.listdir(root / str(c)))
        assert any((root / str(c) / f).read_bytes() == pays[c].read_bytes() for f in files), (c, files, p.stderr)
    # what the program refuses: a rate that is no integer, a ratio out of range
    for argv, text in (([str(wide), "64/3"] + spec, "is not an integer"), ([str(wide), "7/4"] + spec, "interpolation"),
                       ([str(wide), "25/0"] + spec, "interpolation"), ([str(wide), "35/17"] + spec, "interpolation")):
        q = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=60)
        assert q.returncode == 1 and text in q.stderr, (argv, q.stderr)


def test_adjacent_channel_tool_at_a_ratio_and_a_tiny_size():
    """neighbours a full 8000 Hz away at the victim's level cost nothing; a co-channel neighbour 20 dB above it costs every frame"""
    exe = os.path.join(ROOT, "tools", "adjacent_channel.py")
    p = subprocess.run([sys.executable, exe, "--ratio", "%d/%d" % (P, Q), "--frames", "2", "--spacings", "8000", "0", "--levels", "0", "20",
                        "--timeout", "100"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    last = json.loads(p.stdout.strip().splitlines()[-1])
    assert last["tool"] == "adjacent_channel" and last["interp"] == "25/4" and len(last["rows"]) == 4
    by = {(r["spacing_hz"], r["level_db"]): r for r in last["rows"]}
    print(p.stdout)
    assert by[8000.0, 0.0]["fer"] == 0.0 and by[8000.0, 0.0]["ber"] == 0.0
    assert by[0.0, 20.0]["fer"] == 1.0
