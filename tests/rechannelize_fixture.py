"""The 50 kHz capture (25/4 x 8000) test_gpu_rechannelize_bank.py decodes: the first two golden mode-6 frames of
tests/golden/base_frames_2ch_0.npz, each interpolated x 25 by a zero-padded FFT with every 4th sample kept, moved to the signal
centres -14000 and +9000 Hz (the frames are centred at +2000 Hz: mixed by centre - 2000), started 0 and 50021 wideband samples in,
with amplitudes 0.05 and 0.2, under complex noise of sigma 1e-3 per component (seed 50), rounded to int16: 50021 + 95200 x 25 / 4 =
645021 wideband samples.

Checked on the CPU with the oracle on the float64 model's rows (test_rechannelize_model_cpu.py asserts exactly this): the channel
at -14000 Hz decodes payload 0 (status 0, 0 flips) at sc_start 9612, the channel at +9000 Hz payload 1 at sc_start 17615 = 9612 +
floor(50021 x 4 / 25), neither has a second preamble, and an empty channel at -3000 Hz has none.  The survey's float64 model
(survey_model.py) with the finder's default parameters returns two bands within 100 Hz of the two centres at these amplitudes: the
weak one needed no raising."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
P, Q, RATE = 25, 4, 8000
WIDE_RATE = 50000
SIGNAL_HZ = (-14000.0, 9000.0)
CHANNEL_HZ = (-14000.0, 9000.0, -3000.0)                            # the last one is empty
AMPLITUDE = (0.05, 0.2)
STARTS = (0, 50021)
SC_START = (9612, 9612 + 50021 * Q // P)
SIGMA = 1e-3


def golden():
    q = np.load(os.path.join(HERE, "golden", "base_frames_2ch_0.npz"))
    return q["pcm"], q["payload"]


def capture():
    """-> (int16 [W, 2] at 50 kHz, payloads [2, 5380])"""
    base, pays = golden()
    assert base.shape[0] == 2
    n = base.shape[1]
    assert (P * n) % Q == 0
    L = P * n // Q
    W = STARTS[-1] + L
    x = np.zeros(W, np.complex128)
    for f in range(2):
        z = base[f].astype(np.float64) / 32767.0
        Z = np.fft.fft(z[:, 0] + 1j * z[:, 1])
        Y = np.zeros(P * n, np.complex128)
        Y[:n // 2] = Z[:n // 2]
        Y[-(n - n // 2):] = Z[n // 2:]
        y = (np.fft.ifft(Y) * P)[::Q]
        m = np.arange(L, dtype=np.float64)
        x[STARTS[f]:STARTS[f] + L] += AMPLITUDE[f] * y * np.exp(2j * np.pi * (SIGNAL_HZ[f] - 2000.0) * m / WIDE_RATE)
    rng = np.random.default_rng(50)
    x += SIGMA * (rng.standard_normal(W) + 1j * rng.standard_normal(W))
    pcm = np.stack([x.real, x.imag], axis=1)
    return np.rint(np.clip(pcm, -1.0, 1.0) * 32767.0).astype(np.int16), pays
