"""The wideband capture test_gpu_wideband_bank.py decodes: the four golden mode-6 frames of tests/golden/base_frames_2ch_*.npz
interpolated x 6 by a zero-padded FFT, moved to the signal centres -13000, 3000, 7000 and 11000 Hz of a 48 kHz capture (the frames
are centred at +2000 Hz: mixed by centre - 2000), started 48007, 48013 and 47988 samples after one another, with amplitudes 0.05,
0.05, 0.5 and 0.2, under complex noise of sigma 1e-3 per component, rounded to int16.

Checked on the CPU with the oracle on the float64 model's rows: every frame decodes from its channel (status 0, payload equal, 0
flips) at sc_start 9612 + start / 6 = the frame's own 9600 + K / D; an empty channel at -5000 Hz gives no preamble.  The strong
frame at 7000 Hz leaks through the transition band of the channel 4050 Hz above it and gives that channel one failed-header record
(status 6, cfo near 3950 Hz) before its real one: the channel for the 11000 Hz frame is therefore kept at 11050 Hz, and the test
asserts the pair."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DECIM, RATE = 6, 8000
SIGNAL_HZ = (-13000.0, 3000.0, 7000.0, 11000.0)
CHANNEL_HZ = (-13000.0, 3000.0, 7000.0, 11050.0, -5000.0)           # the last one is empty
AMPLITUDE = (0.05, 0.05, 0.5, 0.2)
STARTS = (0, 48007, 48007 + 48013, 48007 + 48013 + 47988)
SIGMA = 1e-3


def golden():
    parts = [np.load(os.path.join(HERE, "golden", "base_frames_2ch_%d.npz" % k)) for k in range(2)]
    return np.concatenate([q["pcm"] for q in parts]), np.concatenate([q["payload"] for q in parts])


def capture():
    """-> (int16 [W, 2] at 48 kHz, payloads [4, 5380])"""
    base, pays = golden()
    assert base.shape[0] == 4
    n = base.shape[1]
    rw = DECIM * RATE
    W = STARTS[-1] + DECIM * n
    x = np.zeros(W, np.complex128)
    for f in range(4):
        z = base[f].astype(np.float64) / 32767.0
        Z = np.fft.fft(z[:, 0] + 1j * z[:, 1])
        Y = np.zeros(DECIM * n, np.complex128)
        Y[:n // 2] = Z[:n // 2]
        Y[-(n - n // 2):] = Z[n // 2:]
        y = np.fft.ifft(Y) * DECIM
        m = np.arange(DECIM * n, dtype=np.float64)
        x[STARTS[f]:STARTS[f] + DECIM * n] += AMPLITUDE[f] * y * np.exp(2j * np.pi * (SIGNAL_HZ[f] - 2000.0) * m / rw)
    rng = np.random.default_rng(48)
    x += SIGMA * (rng.standard_normal(W) + 1j * rng.standard_normal(W))
    pcm = np.stack([x.real, x.imag], axis=1)
    return np.rint(np.clip(pcm, -1.0, 1.0) * 32767.0).astype(np.int16), pays
