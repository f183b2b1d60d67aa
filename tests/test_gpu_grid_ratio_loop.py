"""The grid loop at a ratio on the device, in the pattern of test_gpu_grid_loop.py: payloads -> tx_encode (2
channels, freq_off 0, mode 6) -> synthesize_grid at P / Q (unequal gains, unequal starts on the grid of P) -> awgn_tile on the
capture at -60 dB -> the grid bank at the same ratio and ofdmrx_util_channelize_grid_ratio -> payloads.  The capture never leaves the
device before it is decoded; it is copied out once for the checks.  Then the same loop through the command line.
  (1) 6/1, 48 kHz: three frames in slots -5, 2 and 3.  Slots 2 and 3 are neighbours, 4000 Hz apart, and each sees the other's frame
      through the filter's transition band: their frames follow one another in time; the frame in slot -5 overlaps the one in slot 2;
  (2) 25/4, 50 kHz: two frames in slots -6 and 3 that overlap in time."""
import os
import subprocess
import wave

import numpy as np
import pytest

import channelize_grid_ratio_model as CGR
import grid_fixture as GF
import oracle_lib as O

pytestmark = pytest.mark.gpu

RATE, MODE, NOISE_DB = 8000, 6, -60.0
CASES = {
    1: dict(P=6, Q=1, slots=(-5, 2, 3), gains=(0.1, 0.3, 0.2), starts=(6, 6 * 8001, 6 * 104000), open=(-5, 2, 3),
            cuttings=((1 << 26,), (48000,), (40009, 0, 1))),
    2: dict(P=25, Q=4, slots=(-6, 3), gains=(0.3, 0.15), starts=(25, 25 * 800), open=(-6, 3),
            cuttings=((1 << 26,), (50000,), (40009, 0, 5))),
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
    import modem_amd
    import torch
    cfg = CASES[request.param]
    P, Q, C = cfg["P"], cfg["Q"], len(cfg["slots"])
    assert all(s % P == 0 for s in cfg["starts"]) and len(set(cfg["starts"])) == C
    pays = np.stack([O.payload_for(260 + 10 * request.param + c) for c in range(C)])
    n_in = rx.tx_frame_samples(MODE)
    d_pay = torch.from_numpy(pays).to("cuda:0")
    d_pcm = torch.zeros((C, n_in, 2), dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    for c in range(C):
        rx.tx_encode(d_pay[c].data_ptr(), 1, d_pcm[c].data_ptr(), mode=MODE, freq_off=0, channels=2)
    W = max(cfg["starts"]) + modem_amd.synthesize_support(n_in, (P, Q))
    d_cap = torch.full((W + 1, 2), 12345, dtype=torch.int16, device="cuda:0")
    rx.synthesize_grid(d_pcm.data_ptr(), 0, n_in, (P, Q), cfg["slots"], cfg["starts"], cfg["gains"], 0, W, d_cap.data_ptr(), 0)
    rx.awgn_tile(d_cap.data_ptr(), 1, d_cap.data_ptr(), 1, W, NOISE_DB, 48, 0)
    n_out = -(-W * Q // P)
    d_rows = torch.full((len(cfg["open"]), n_out, 2), 12345.0, dtype=torch.float32, device="cuda:0")
    rx.channelize_grid(d_cap.data_ptr(), 0, 0, W, (P, Q), list(cfg["open"]), 0, n_out, d_rows.data_ptr())
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


def _table(rec, pays):
    out, res, npre = rec
    assert len(res) == npre
    return [(int(res[k]["status"]), ([j for j in range(len(pays)) if (out[k] == pays[j]).all()] + [None])[0], int(res[k]["sc_start"]))
            for k in range(npre)]


def test_every_frame_decodes_from_its_slot(loop):
    """status 0 and the payload from the frame's own slot, where section 4.23 puts it: its own sc_start + 24 + start Q / P"""
    cfg, cap, pays, rows, recs, own = loop
    for c, k in enumerate(cfg["slots"]):
        out, res, npre = recs[cfg["open"].index(k)]
        ok = [i for i in range(len(res)) if int(res[i]["status"]) == 0]
        assert len(ok) == 1, (k, [int(s) for s in res["status"]])
        i = ok[0]
        assert (out[i] == pays[c]).all() and int(res[i]["bit_flips"]) == 0 and int(res[i]["oper_mode"]) == MODE
        want = own[c] + 24 + cfg["starts"][c] // cfg["P"] * cfg["Q"]
        assert abs(int(res[i]["sc_start"]) - want) <= 1, (k, int(res[i]["sc_start"]), own[c])


def test_the_oracle_finds_the_same_records_on_the_models_rows(loop):
    """the float64 model of the front end on the capture's own bytes, every preamble the oracle finds in each row: the same status,
    payload and sc_start, record for record"""
    cfg, cap, pays, rows, recs, own = loop
    model = CGR.wide_rows(cap, cfg["P"], cfg["Q"], list(cfg["open"]))
    for j, k in enumerate(cfg["open"]):
        orecs = GF.oracle_records(model[j])
        want = [(s, f, int(r.sc_start)) for (s, f), (_, r) in zip(GF.table(orecs, pays), orecs)]
        assert _table(recs[j], pays) == want, (k, _table(recs[j], pays), want)


def _by_channel(parts, n_channels):
    pay = np.concatenate([p[0] for p in parts])
    res = np.concatenate([p[1] for p in parts])
    ch = np.concatenate([p[2] for p in parts])
    ix = np.concatenate([p[3] for p in parts])
    return [(pay[ch == c].tobytes(), res[ch == c].tobytes(), list(ix[ch == c])) for c in range(n_channels)]


@pytest.mark.parametrize("cut", [0, 1, 2])
def test_bank_equals_the_one_call_decode(rx, loop, cut):
    """section 4.22's contract on a capture made on the device: the capture pushed in one block, in blocks of a wideband second and in
    odd blocks with empty ones between through a grid bank at the ratio gives, per opened slot and byte for byte, the payloads and
    results of the one-call decode of ofdmrx_util_channelize_grid_ratio's rows"""
    cfg, cap, pays, rows, recs, own = loop
    blocks = cfg["cuttings"][cut]
    bank = rx.wideband_grid_bank(list(cfg["open"]), (cfg["P"], cfg["Q"]))
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


def test_command_line(tmp_path):
    """encode ... 2 0 6 ... per frame -> synthesize --grid-ratio 25/4 -> decode_stream --grid 25/4 gives the payload files back"""
    cfg = CASES[2]
    P, Q = cfg["P"], cfg["Q"]
    pays, wavs = [], []
    for i in range(len(cfg["slots"])):
        pay = tmp_path / ("pay%d.bin" % i)
        pay.write_bytes(O.payload_for(280 + i).tobytes())
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
    p = subprocess.run([exe, "--grid-ratio", str(wide), "%d/%d" % (P, Q)] + spec, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    with wave.open(str(wide), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (2, 2, RATE * P // Q)
        assert w.getnframes() == max(cfg["starts"]) + ((95200 - 1 + 24) * P) // Q + 1
    root = tmp_path / "out"
    p = subprocess.run([os.path.join(BIN, "decode_stream"), "--grid", "%d/%d" % (P, Q), ",".join("%d" % k for k in cfg["slots"]), str(root), str(wide)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    for c in range(len(cfg["slots"])):
        files = sorted(os.listdir(root / str(c)))
        assert any((root / str(c) / f).read_bytes() == pays[c].read_bytes() for f in files), (c, files, p.stderr)
    # the unreduced ratio is the same capture; what the program refuses
    wide2 = tmp_path / "wide2.wav"
    p = subprocess.run([exe, "--grid-ratio", str(wide2), "%d/%d" % (2 * P, 2 * Q)] + spec, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and wide2.read_bytes() == wide.read_bytes(), p.stderr
    for argv, text in ((["--grid-ratio", str(wide), "25/4", "7:0:0:%s" % wavs[0]], "slot"), (["--grid-ratio", str(wide), "25/4", "2:24:0:%s" % wavs[0]], "START"),
                       (["--grid-ratio", str(wide), "25/4", spec[0], spec[0]], "twice"), (["--grid-ratio", str(wide), "25/3", spec[0]], "integer"),
                       (["--grid-ratio", str(wide), "6", spec[0]], "ratio"), (["--grid", str(wide), "25/4", spec[0]], "not built")):
        q = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=60)
        assert q.returncode == 1 and text in q.stderr, (argv, q.stderr)
