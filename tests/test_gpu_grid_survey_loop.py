"""The grid survey in the loop: a capture -> Receiver.survey_grid -> peak hold over the rows -> find_slots ->
a grid bank on the slots FOUND -> payloads.
  (1) the captures of grid_fixture.py: capture A (D = 8, four frames; an absolute floor of twice the predicted noise reading, since
      12 of its 16 slots carry a frame or its edge) and capture B (D = 64, two frames; the median floor) give the slots
      test_survey_grid_model_cpu.py gets from the float64 model, and the bank on them returns the golden payloads - byte for byte what
      the one-call decode of ofdmrx_util_channelize_grid's rows gives;
  (2) the device loop: payloads -> tx_encode -> synthesize_grid -> awgn_tile -> survey_grid -> find_slots -> grid bank at D = 8
      recovers the payloads from slots it was not told (the floor: twice what a noise-only capture of the same noise reads);
  (3) the same through the command line: `survey --grid` and `decode_stream --grid D auto[:FLOOR_DB]` against the explicit list."""
import os
import subprocess
import wave

import numpy as np
import pytest

import grid_fixture as GF
import oracle_lib as O
import survey_grid_model as SG

pytestmark = pytest.mark.gpu

RATE, MODE, NOISE_DB, S = 8000, 6, -60.0, 4096
LOOP = dict(D=8, slots=(-6, -2, 2, 6), gains=(0.05, 0.3, 0.2, 0.1), starts=(8, 48008, 96016, 144008))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "modem_amd", "bin")


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1)
    yield r
    r.close()


def _peak_row(rx, d_cap, D):
    rows = rx.survey_grid(d_cap, 0, D, S)
    assert rows.shape[0] >= 1 and rows.shape[1] == 2 * D
    return rows.max(dim=0).values


def _bank(rx, cap, slots, D, blocks):
    bank = rx.wideband_grid_bank(list(slots), D)
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
    pay = np.concatenate([p[0] for p in parts])
    res = np.concatenate([p[1] for p in parts])
    ch = np.concatenate([p[2] for p in parts])
    return [(pay[ch == c], res[ch == c]) for c in range(len(slots))]


def _one_call(rx, cap, slots, D):
    import torch
    d_cap = torch.from_numpy(cap).to("cuda:0")
    n_out = -(-len(cap) // D)
    d_rows = torch.zeros((len(slots), n_out, 2), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rx.channelize_grid(d_cap.data_ptr(), 0, 0, len(cap), D, list(slots), 0, n_out, d_rows.data_ptr())
    rx.synchronize()
    return rx.decode_streams(list(d_rows.cpu().numpy()))


@pytest.mark.parametrize("which", ["a", "b"])
def test_fixture_capture_survey_find_bank(rx, which):
    import modem_amd
    import torch
    cfg, cap = (GF.A, GF.capture_a) if which == "a" else (GF.B, GF.capture_b)
    pcm, pays = cap()
    D = cfg["D"]
    d_cap = torch.from_numpy(pcm).to("cuda:0")
    peak = _peak_row(rx, d_cap, D)
    floor = 2 * SG.noise_reading(D, 2 * GF.SIGMA ** 2) if which == "a" else 0.0
    found = [s["slot"] for s in modem_amd.find_slots(peak, D, RATE, abs_floor=floor)]
    print("capture %s: found %s" % (which, found))
    assert found == list(cfg["slots"])
    if which == "a":
        assert [s["slot"] for s in modem_amd.find_slots(peak, D, RATE)] == [3, 6]       # the median is no noise floor here
    got = _bank(rx, pcm, found, D, (48000, 4097, 1, 0, 5, 7 * 4096 + 3) if which == "a" else (512000, 70001, 0, 1))
    want = _one_call(rx, pcm, found, D)
    for c in range(len(found)):
        out, res, npre = want[c]
        assert got[c][0].tobytes() == out.tobytes() and got[c][1].tobytes() == res.tobytes(), c
        ok = [i for i in range(len(res)) if int(res[i]["status"]) == 0]
        assert len(ok) == 1 and (out[ok[0]] == pays[c]).all(), (c, [int(s) for s in res["status"]])


@pytest.fixture(scope="module")
def loop(rx):
    """the capture made on the device and the noise-only reading: computed once, read only"""
    import torch
    D, C = LOOP["D"], len(LOOP["slots"])
    pays = np.stack([O.payload_for(260 + c) for c in range(C)])
    n_in = rx.tx_frame_samples(MODE)
    d_pay = torch.from_numpy(pays).to("cuda:0")
    d_pcm = torch.zeros((C, n_in, 2), dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    for c in range(C):
        rx.tx_encode(d_pay[c].data_ptr(), 1, d_pcm[c].data_ptr(), mode=MODE, freq_off=0, channels=2)
    W = max(LOOP["starts"]) + (n_in - 1) * D + 24 * D + 1
    d_cap = torch.zeros((W, 2), dtype=torch.int16, device="cuda:0")
    d_noise = torch.zeros((S * D, 2), dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    rx.synthesize_grid(d_pcm.data_ptr(), 0, n_in, D, LOOP["slots"], LOOP["starts"], LOOP["gains"], 0, W, d_cap.data_ptr(), 0)
    rx.awgn_tile(d_cap.data_ptr(), 1, d_cap.data_ptr(), 1, W, NOISE_DB, 48, 0)
    rx.awgn_tile(d_noise.data_ptr(), 1, d_noise.data_ptr(), 1, S * D, NOISE_DB, 49, 0)
    rx.synchronize()
    noise = float(rx.survey_grid(d_noise, 0, D, S).median())
    peak = _peak_row(rx, d_cap, D).cpu().numpy()
    cap = d_cap.cpu().numpy()
    for a in (cap, pays, peak):
        a.setflags(write=False)
    return cap, pays, peak, noise


def test_device_loop_recovers_payloads_from_found_slots(rx, loop):
    import modem_amd
    cap, pays, peak, noise = loop
    assert noise > 0
    found = [s["slot"] for s in modem_amd.find_slots(peak, LOOP["D"], RATE, abs_floor=2 * noise)]
    print("device loop: noise reads %.4g, found %s" % (noise, found))
    assert found == list(LOOP["slots"])
    got = _bank(rx, cap, found, LOOP["D"], (48000, 4097, 1, 0, 5, 7 * 4096 + 3))
    for c in range(len(found)):
        out, res = got[c]
        ok = [i for i in range(len(res)) if int(res[i]["status"]) == 0]
        assert len(ok) == 1 and (out[ok[0]] == pays[c]).all(), c


def _write_wav(path, pcm, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(pcm, dtype="<i2").tobytes())


def _tree(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def test_command_line(tmp_path, loop):
    """`survey --grid` prints the slots; `decode_stream --grid D auto[:FLOOR_DB]` writes the files of the explicit list"""
    cap, pays, peak, noise = loop
    D = LOOP["D"]
    wide = tmp_path / "wide.wav"
    _write_wav(wide, cap, D * RATE)
    floor_db = "%.3f" % (10 * np.log10(2 * noise))
    survey, dec = os.path.join(BIN, "survey"), os.path.join(BIN, "decode_stream")
    lists = {}
    for how, extra in (("floor", [floor_db]), ("median", [])):
        p = subprocess.run([survey, "--grid", str(wide), str(D)] + extra, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        lines = [l.split() for l in p.stdout.splitlines()]
        lists[how] = [int(l[0]) for l in lines]
        assert all(float(l[1]) == int(l[0]) * RATE / 2 for l in lines) and len(lists[how]) >= 1
    assert lists["floor"] == list(LOOP["slots"])
    for how, arg in (("floor", "auto:" + floor_db), ("median", "auto")):
        a, b = tmp_path / ("auto_" + how), tmp_path / ("list_" + how)
        p = subprocess.run([dec, "--grid", str(D), arg, str(a), str(wide)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert "slots " + ",".join("%d" % k for k in lists[how]) in p.stderr
        q = subprocess.run([dec, "--grid", str(D), ",".join("%d" % k for k in lists[how]), str(b), str(wide)], capture_output=True, text=True,
                           timeout=120)
        assert q.returncode == 0, q.stderr
        ta, tb = _tree(a), _tree(b)
        assert ta == tb and len(ta) >= len(lists[how])
        if how == "floor":
            for c in range(len(pays)):
                assert any(v == pays[c].tobytes() for k, v in ta.items() if k.startswith("%d/" % c)), c


def test_command_line_refusals(tmp_path):
    """`auto` from standard input is refused; pure silence ends with the no-slot error; a file shorter than one row is an error"""
    D = 8
    dec, survey = os.path.join(BIN, "decode_stream"), os.path.join(BIN, "survey")
    p = subprocess.run([dec, "--grid", str(D), "auto", str(tmp_path / "o"), "-"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert p.returncode == 1 and "standard input" in p.stderr
    silence = tmp_path / "silence.wav"
    _write_wav(silence, np.zeros((S * D, 2), np.int16), D * RATE)
    p = subprocess.run([dec, "--grid", str(D), "auto", str(tmp_path / "o"), str(silence)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "no occupied slot" in p.stderr
    p = subprocess.run([survey, "--grid", str(silence), str(D)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout == ""
    short = tmp_path / "short.wav"
    _write_wav(short, np.zeros(((S - 1) * D, 2), np.int16), D * RATE)
    p = subprocess.run([survey, "--grid", str(short), str(D)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "shorter than one row" in p.stderr
    for argv in ([survey, "--grid", str(silence), "6"], [survey, "--grid", str(silence), str(D), "x"], [dec, "--grid", "6", "auto", str(tmp_path / "o"), str(silence)],
                 [dec, "--grid", str(D), "auto:x", str(tmp_path / "o"), str(silence)]):
        p = subprocess.run(argv, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1, argv
