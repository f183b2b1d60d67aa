"""The wideband captures test_gpu_grid_ratio_bank.py decodes through the grid front end at a ratio, built as
grid_fixture.py builds its captures: golden mode-6 frames of tests/golden/base_frames_2ch_*.npz interpolated x P / Q by a zero-padded
FFT (their 95 200 samples are divisible by every Q used) and moved to slot centres k rate / 2 (the frames are centred at +2000 Hz:
mixed by k 4000 - 2000 Hz, the exact integer phase (2 k - 1) Q m mod 4 P), under complex noise of sigma 1e-3 per component, rounded
to int16.
  (a) capture_a: 6/1, 48 kHz.  Frames 0 and 1 at slots -6 and 5, the second 600 001 samples after the first, amplitudes 0.2 and 0.1;
      slots -6, 5 and 0 open.
  (b) capture_b: 25/4, 50 kHz.  Frames 0 and 1 at slots -6 and 3, the second 74 382 samples after the first, amplitudes 0.2 and 0.1;
      slots -6 and 3 open.
  (c) capture_c: 75/2, 300 kHz (M = 150 = 2 3 5^2, beyond the ratio front end's 32).  Frames 0 and 1 at slots 37 and -37, the second
      3 600 007 samples after the first, amplitudes 0.2 and 0.1; slots 37, -37 and 36 open.
Checked on the CPU with the oracle on the float64 model's rows (test_channelize_grid_ratio_model_cpu.py): EXPECTED lists, per opened
slot, the records the oracle finds in stream order as (status, frame or None, sc_start): every frame decodes from its own slot
(status 0, payload equal) at sc_start 9612 + start Q / P, rounded.  Slots -6 and 5 of (a) are neighbours across the band edge - the
slots repeat with period 2 P - so slot 5 sees slot -6's frame through the filter's transition band: where that gives the oracle a
preamble with a failed header the table says so and the device must give the same."""
import numpy as np

from grid_fixture import RATE, SIGMA, golden, oracle_records, table  # noqa: F401

A = dict(P=6, Q=1, slots=(-6, 5), frames=(0, 1), amplitude=(0.2, 0.1), starts=(0, 600001), seed=48, open=(-6, 5, 0))
B = dict(P=25, Q=4, slots=(-6, 3), frames=(0, 1), amplitude=(0.2, 0.1), starts=(0, 74382), seed=50, open=(-6, 3))
C = dict(P=75, Q=2, slots=(37, -37), frames=(0, 1), amplitude=(0.2, 0.1), starts=(0, 3600007), seed=300, open=(37, -37, 36))
CONFIGS = {"a": A, "b": B, "c": C}


def capture(cfg):
    """-> (int16 [W, 2] at rate P / Q, payloads [frames, 5380])"""
    base, pays = golden()
    P, Q = cfg["P"], cfg["Q"]
    n = base.shape[1]
    assert n % Q == 0
    nw = n * P // Q
    W = max(cfg["starts"]) + nw
    x = np.zeros(W, np.complex128)
    m = np.arange(nw, dtype=np.int64)
    for f, k, amp, s in zip(cfg["frames"], cfg["slots"], cfg["amplitude"], cfg["starts"]):
        z = base[f].astype(np.float64) / 32767.0
        Z = np.fft.fft(z[:, 0] + 1j * z[:, 1])
        Y = np.zeros(nw, np.complex128)
        Y[:n // 2] = Z[:n // 2]
        Y[-(n - n // 2):] = Z[n // 2:]
        y = np.fft.ifft(Y) * (P / Q)
        ph = ((2 * k - 1) * Q * m) % (4 * P)                        # (k 4000 - 2000) / Rw = (2 k - 1) Q / (4 P) cycles per sample
        x[s:s + nw] += amp * y * np.exp(2j * np.pi * ph.astype(np.float64) / (4 * P))
    rng = np.random.default_rng(cfg["seed"])
    x += SIGMA * (rng.standard_normal(W) + 1j * rng.standard_normal(W))
    pcm = np.stack([x.real, x.imag], axis=1)
    return np.rint(np.clip(pcm, -1.0, 1.0) * 32767.0).astype(np.int16), pays[list(cfg["frames"])]


def sc_start(cfg, i):
    """where frame i's record stands in its slot's row: the frame's own 9600 + 12, from its start in output samples (no start of the
    fixtures is a tie)"""
    return 9612 + int(round(cfg["starts"][i] * cfg["Q"] / cfg["P"]))


def table3(recs, pays):
    """[(payload, result)] -> [(status, frame or None, sc_start)]"""
    return [(s, f, int(r.sc_start)) for (s, f), (_, r) in zip(table(recs, pays), recs)]


# per opened slot, in stream order: (status, index of the frame whose payload the record carries or None, sc_start)
EXPECTED = {
    "a": {-6: [(0, 0, 9612)], 5: [(3, None, 9617), (0, 1, 109612)], 0: []},
    "b": {-6: [(0, 0, 9612)], 3: [(0, 1, 21513)]},
    "c": {37: [(0, 0, 9612)], -37: [(0, 1, 105612)], 36: [(6, None, 9614)]},
}
