"""The grid survey at a ratio in the loop: a capture -> Receiver.survey_grid at (p, q) -> peak hold over the
rows of 4096 output times -> find_slots at (p, q) -> a grid bank at the ratio on the slots FOUND -> the records of
grid_ratio_fixture.EXPECTED, byte for byte what the bank on the explicit list gives; and the same through the command line: `survey
--grid-ratio` and `decode_stream --grid-ratio P/Q auto[:FLOOR_DB]` against `decode_stream --grid P/Q LIST`.  The captures are
grid_ratio_fixture's A (48 kHz, 6/1: the placed slots -6 and 5 are cyclic neighbours) and B (50 kHz, 25/4: slot -6 is k_first); the
finder's parameters are the ones test_survey_grid_ratio_model_cpu.py fixed from the model: the defaults and the median floor.

In capture B the last slot 6 lies half a slot from the first slot -6 across the band edge and reads the frame placed in slot -6 at
-22.18 dB re full scale, 0.4 dB under slot -6's own -21.79 dB: the finder takes the two ends for one signal and reports the louder."""
import os
import subprocess
import wave

import numpy as np
import pytest

import grid_ratio_fixture as GF
from test_survey_grid_ratio_model_cpu import FIXTURE_FLOOR

pytestmark = pytest.mark.gpu

S = 4096
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "modem_amd", "bin")


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1)
    yield r
    r.close()


@pytest.fixture(scope="module")
def captures():
    """the fixture captures: computed once, read only"""
    out = {}
    for name in ("a", "b"):
        pcm, pays = GF.capture(GF.CONFIGS[name])
        pcm.setflags(write=False)
        pays.setflags(write=False)
        out[name] = (pcm, pays)
    return out


def _bank(rx, cap, slots, ratio, blocks):
    bank = rx.wideband_grid_bank(list(slots), ratio)
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


def _table(out, res, pays):
    return [(int(res[k]["status"]), ([j for j in range(len(pays)) if (out[k] == pays[j]).all()] + [None])[0], int(res[k]["sc_start"]))
            for k in range(len(res))]


@pytest.mark.parametrize("name", ["a", "b"])
def test_fixture_capture_survey_find_bank(rx, captures, name):
    import modem_amd
    import torch
    cfg = GF.CONFIGS[name]
    pcm, pays = captures[name]
    ratio = (cfg["P"], cfg["Q"])
    d_cap = torch.from_numpy(pcm.copy()).to("cuda:0")
    rows = rx.survey_grid(d_cap, 0, ratio, S)
    assert rows.shape[0] == ((len(pcm) * cfg["Q"] - 1) // cfg["P"] + 1) // S and rows.shape[1] == len(modem_amd.grid_centres(ratio, GF.RATE))
    peak = rows.max(dim=0).values
    print("capture %s, peak-hold row in dB re full scale: %s" % (name, " ".join("%.2f" % v for v in 10 * np.log10(peak.cpu().numpy()))))
    found = [s["slot"] for s in modem_amd.find_slots(peak, ratio, GF.RATE, abs_floor=FIXTURE_FLOOR[name])]
    placed = sorted(cfg["slots"])
    print("capture %s: found %s, placed %s" % (name, found, placed))
    assert found == placed
    blocks = (48000, 4097, 1, 0, 5, 7 * 4096 + 3)
    got = _bank(rx, pcm, found, ratio, blocks)
    want = _bank(rx, pcm, placed, ratio, blocks)
    for c, k in enumerate(placed):
        assert got[c][0].tobytes() == want[c][0].tobytes() and got[c][1].tobytes() == want[c][1].tobytes(), k
        assert _table(got[c][0], got[c][1], pays) == GF.EXPECTED[name][k], k


def _write_wav(path, pcm, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(pcm, dtype="<i2").tobytes())


def _tree(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


@pytest.mark.parametrize("name", ["a", "b"])
def test_command_line(tmp_path, captures, name):
    """`survey --grid-ratio` prints the placed slots; `decode_stream --grid-ratio P/Q auto` writes the files of `--grid P/Q LIST`"""
    cfg = GF.CONFIGS[name]
    pcm, pays = captures[name]
    P, Q = cfg["P"], cfg["Q"]
    ratio = "%d/%d" % (P, Q)
    placed = sorted(cfg["slots"])
    wide = tmp_path / "wide.wav"
    _write_wav(wide, pcm, GF.RATE * P // Q)
    survey, dec = os.path.join(BIN, "survey"), os.path.join(BIN, "decode_stream")
    floor = FIXTURE_FLOOR[name]
    extra = ["%.3f" % (10 * np.log10(floor))] if floor > 0 else []
    p = subprocess.run([survey, "--grid-ratio", str(wide), ratio] + extra, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = [l.split() for l in p.stdout.splitlines()]
    print("survey --grid-ratio %s: %s" % (ratio, p.stdout.replace("\n", "; ")))
    assert all(float(l[1]) == int(l[0]) * GF.RATE / 2 for l in lines)
    assert [int(l[0]) for l in lines] == placed
    a, b = tmp_path / "auto", tmp_path / "list"
    p = subprocess.run([dec, "--grid-ratio", ratio, "auto" + (":" + extra[0] if extra else ""), str(a), str(wide)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert "slots " + ",".join("%d" % k for k in placed) in p.stderr
    q = subprocess.run([dec, "--grid", ratio, ",".join("%d" % k for k in placed), str(b), str(wide)], capture_output=True, text=True, timeout=120)
    assert q.returncode == 0, q.stderr
    ta, tb = _tree(a), _tree(b)
    assert ta == tb and len(ta) >= len(placed)
    for c, k in enumerate(placed):
        for status, frame, sc in GF.EXPECTED[name][k]:
            if status == 0:
                assert any(v == pays[frame].tobytes() for f, v in ta.items() if f.startswith("%d/" % c)), k


def test_command_line_list_and_all_are_the_grid_form(tmp_path, captures):
    """`--grid-ratio P/Q LIST` and `all` behave exactly as `--grid P/Q` does: the same files"""
    pcm, pays = captures["b"]
    wide = tmp_path / "wide.wav"
    _write_wav(wide, pcm, 50000)
    dec = os.path.join(BIN, "decode_stream")
    for how in ("-6,3", "all"):
        a, b = tmp_path / ("r_" + how), tmp_path / ("g_" + how)
        p = subprocess.run([dec, "--grid-ratio", "25/4", how, str(a), str(wide)], capture_output=True, text=True, timeout=120)
        q = subprocess.run([dec, "--grid", "25/4", how, str(b), str(wide)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and q.returncode == 0, (p.stderr, q.stderr)
        assert _tree(a) == _tree(b) and p.stdout == q.stdout


def test_command_line_refusals(tmp_path):
    """`auto` from standard input, pure silence, a file shorter than a row and a bad `auto:x` exit 1 and write nothing"""
    P, Q = 25, 4
    dec, survey = os.path.join(BIN, "decode_stream"), os.path.join(BIN, "survey")
    out = tmp_path / "o"
    p = subprocess.run([dec, "--grid-ratio", "25/4", "auto", str(out), "-"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert p.returncode == 1 and "standard input" in p.stderr and not out.exists()
    row = ((S - 1) * P) // Q + 1                                     # the samples of one row
    silence = tmp_path / "silence.wav"
    _write_wav(silence, np.zeros((row, 2), np.int16), 50000)
    p = subprocess.run([dec, "--grid-ratio", "25/4", "auto", str(out), str(silence)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "no occupied slot" in p.stderr and not out.exists()
    p = subprocess.run([survey, "--grid-ratio", str(silence), "25/4"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout == ""
    short = tmp_path / "short.wav"
    _write_wav(short, np.zeros((row - 1, 2), np.int16), 50000)
    p = subprocess.run([survey, "--grid-ratio", str(short), "25/4"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "shorter than one row" in p.stderr
    p = subprocess.run([dec, "--grid-ratio", "25/4", "auto", str(out), str(short)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "shorter than one row" in p.stderr and not out.exists()
    p = subprocess.run([dec, "--grid-ratio", "25/4", "auto:x", str(out), str(silence)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and not out.exists()
    w48 = tmp_path / "w48.wav"
    _write_wav(w48, np.zeros((row, 2), np.int16), 48000)                # 48000 x 4 / 25 is no supported rate
    p = subprocess.run([survey, "--grid-ratio", str(w48), "25/4"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "sample rate" in p.stderr
