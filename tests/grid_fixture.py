"""The wideband captures test_gpu_grid_bank.py decodes through the grid front end, in the style of
wideband_fixture.py: golden mode-6 frames of tests/golden/base_frames_2ch_*.npz interpolated x D by a zero-padded FFT and moved to
slot centres k rate / 2 (the frames are centred at +2000 Hz: mixed by k 4000 - 2000), under complex noise of sigma 1e-3 per
component, rounded to int16.
  (a) capture_a: D = 8, 64 kHz.  The four frames at slots -7, -2, 3 and 6, started 64007, 64011 and 63988 samples after one another,
      amplitudes 0.05, 0.05, 0.5 and 0.2.  The bank opens all 16 slots.
  (b) capture_b: D = 64, 512 kHz.  Frames 0 and 1 at slots 37 and 39, the second 512007 samples after the first, amplitudes 0.2 and
      0.1; slots 37, 38 and 39 are opened.
Checked on the CPU with the oracle on the float64 model's rows (test_channelize_grid_model_cpu.py): EXPECTED_A / EXPECTED_B list, per
opened slot, the records the oracle finds in stream order as (status, frame or None): every frame decodes from its own slot (status
0, payload equal) at sc_start 9612 + start / D, rounded.  A slot next to a frame's slot lies rate / 2 = 4000 Hz from its centre: it sees the
frame's near edge through the filter's transition band, and where that gives the oracle a preamble with a failed header the table
says so and the device must give the same."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RATE = 8000
SIGMA = 1e-3

A = dict(D=8, slots=(-7, -2, 3, 6), frames=(0, 1, 2, 3), amplitude=(0.05, 0.05, 0.5, 0.2),
         starts=(0, 64007, 64007 + 64011, 64007 + 64011 + 63988), seed=64, open=tuple(range(-8, 8)))
B = dict(D=64, slots=(37, 39), frames=(0, 1), amplitude=(0.2, 0.1), starts=(0, 512007), seed=512, open=(37, 38, 39))


def golden():
    parts = [np.load(os.path.join(HERE, "golden", "base_frames_2ch_%d.npz" % k)) for k in range(2)]
    return np.concatenate([q["pcm"] for q in parts]), np.concatenate([q["payload"] for q in parts])


def _capture(cfg):
    base, pays = golden()
    D = cfg["D"]
    n = base.shape[1]
    rw = D * RATE
    W = cfg["starts"][-1] + D * n
    x = np.zeros(W, np.complex128)
    m = np.arange(D * n, dtype=np.int64)
    for f, k, amp, s in zip(cfg["frames"], cfg["slots"], cfg["amplitude"], cfg["starts"]):
        z = base[f].astype(np.float64) / 32767.0
        Z = np.fft.fft(z[:, 0] + 1j * z[:, 1])
        Y = np.zeros(D * n, np.complex128)
        Y[:n // 2] = Z[:n // 2]
        Y[-(n - n // 2):] = Z[n // 2:]
        y = np.fft.ifft(Y) * D
        hz = k * (RATE // 2) - 2000                                  # an integer number of Hz: the phase is exact mod rw
        x[s:s + D * n] += amp * y * np.exp(2j * np.pi * ((hz * m) % rw).astype(np.float64) / rw)
    rng = np.random.default_rng(cfg["seed"])
    x += SIGMA * (rng.standard_normal(W) + 1j * rng.standard_normal(W))
    pcm = np.stack([x.real, x.imag], axis=1)
    return np.rint(np.clip(pcm, -1.0, 1.0) * 32767.0).astype(np.int16), pays[list(cfg["frames"])]


def capture_a():
    """-> (int16 [W, 2] at 64 kHz, payloads [4, 5380])"""
    return _capture(A)


def capture_b():
    """-> (int16 [W, 2] at 512 kHz, payloads [2, 5380])"""
    return _capture(B)


def sc_start(cfg, i):
    """where frame i's record stands in its slot's row: the frame's own 9600 + K / D, from its start (which lies between two output
    times: the nearer one; no start of the fixtures is a tie)"""
    return 9612 + int(round(cfg["starts"][i] / cfg["D"]))


# per opened slot, in stream order: (status, index of the frame whose payload the record carries, or None)
EXPECTED_A = {-7: [(0, 0)], -2: [(0, 1)], 2: [(6, None)], 3: [(0, 2)], 4: [(6, None)], 6: [(0, 3)]}
EXPECTED_B = {37: [(0, 0)], 38: [], 39: [(0, 1)]}


def oracle_records(row, limit=8):
    """every preamble the oracle finds in a channel row, in stream order -> [(payload, result)].  Its skip-k decode returns the k-th
    preamble; past the last one it returns NO_SYNC - or, when the last preamble's header failed, that preamble's record once more"""
    import oracle_lib as O
    recs = []
    for k in range(limit):
        o, r = O.decode(row, skip=k)
        if r.status == 1 or (recs and recs[-1][1].status in (2, 3, 4, 5) and r.status == recs[-1][1].status and r.sc_start == recs[-1][1].sc_start):
            break
        recs.append((o, r))
    return recs


def table(recs, pays):
    """[(payload, result-like with .status)] -> [(status, frame or None)]"""
    out = []
    for o, r in recs:
        hit = [j for j in range(len(pays)) if (np.asarray(o) == pays[j]).all()]
        out.append((int(r.status), hit[0] if hit else None))
    return out
