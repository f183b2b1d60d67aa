"""The two REAL captures test_gpu_wideband_real_bank.py decodes, each the real part of a capture made by
the recipe of its analytic neighbour, plus real noise of sigma 1e-3, rounded to int16.

  * capture48(): 48 kHz (D = 6), wideband_fixture.capture()'s recipe - the four golden mode-6 frames interpolated x 6, its
    amplitudes 0.05, 0.05, 0.5, 0.2 and its STARTS - at the signal centres -17000, 3000, 7000 and 11000 Hz, noise from
    default_rng(481).  Channels (-17000, 3000, 7000, 11050, 21000, +17000): payloads 0 .. 3 decode from the first four (status 0, 0
    flips) at sc_start 9612, 17613, 25615 and 33613; the channel at 11050 Hz gives one failed-header record first (status 6, cfo
    within 1 Hz of 3950 Hz: the strong frame 4050 Hz below, through the transition band) and tunes its own frame at -50 Hz; the
    channels at 21000 Hz (empty) and at +17000 Hz (the MIRROR of the first frame: its conjugate spectrum) give no preamble.
  * capture50(): 50 kHz (25/4), rechannelize_fixture.capture()'s recipe - the first two golden frames, amplitudes 0.05 and 0.2,
    starts 0 and 50021 - at the centres -14000 and 9000 Hz, noise from default_rng(501).  Channels (-14000, 9000, -3000, +14000):
    payloads 0 and 1 decode at sc_start 9612 and 17615 (status 0, 0 flips); the empty channel and the mirror give no preamble.
test_channelize_real_model_cpu.py asserts exactly this with the oracle on the float64 model's rows.

No two signals of a real capture may share |f| within a channel width: the real part puts every signal at +f AND its conjugate at
-f.  That is why this fixture does not reuse wideband_fixture's centres: with -13000 Hz beside 11000 Hz the 11000 Hz frame's mirror at
-11000 Hz lies 2 kHz beside the -13000 Hz frame and is four times as strong, and that frame failed its header."""
import numpy as np

import rechannelize_fixture as RF
import wideband_fixture as WF

RATE = 8000
SIGMA = 1e-3

DECIM48 = 6
SIGNAL48_HZ = (-17000.0, 3000.0, 7000.0, 11000.0)
CHANNEL48_HZ = (-17000.0, 3000.0, 7000.0, 11050.0, 21000.0, 17000.0)  # the last two: empty, and the first frame's mirror
SC_START48 = (9612, 17613, 25615, 33613)

P50, Q50 = 25, 4
SIGNAL50_HZ = (-14000.0, 9000.0)
CHANNEL50_HZ = (-14000.0, 9000.0, -3000.0, 14000.0)                  # the last two: empty, and the first frame's mirror
SC_START50 = (9612, 17615)


def _interpolated(frame, up, keep):
    """one golden frame [n, 2] int16 -> its analytic signal at up / keep times the rate (a zero-padded FFT, every keep-th sample)"""
    n = frame.shape[0]
    z = frame.astype(np.float64) / 32767.0
    Z = np.fft.fft(z[:, 0] + 1j * z[:, 1])
    Y = np.zeros(up * n, np.complex128)
    Y[:n // 2] = Z[:n // 2]
    Y[-(n - n // 2):] = Z[n // 2:]
    return (np.fft.ifft(Y) * up)[::keep]


def _capture(base, up, keep, centres, amplitudes, starts, seed):
    n = base.shape[1]
    L = up * n // keep
    rw = float(RATE) * up / keep
    W = starts[-1] + L
    x = np.zeros(W, np.complex128)
    for f in range(len(centres)):
        y = _interpolated(base[f], up, keep)
        m = np.arange(L, dtype=np.float64)
        x[starts[f]:starts[f] + L] += amplitudes[f] * y * np.exp(2j * np.pi * (centres[f] - 2000.0) * m / rw)
    real = x.real + SIGMA * np.random.default_rng(seed).standard_normal(W)
    return np.rint(np.clip(real, -1.0, 1.0) * 32767.0).astype(np.int16)


def capture48():
    """-> (int16 [W] at 48 kHz, payloads [4, 5380])"""
    base, pays = WF.golden()
    return _capture(base, DECIM48, 1, SIGNAL48_HZ, WF.AMPLITUDE, WF.STARTS, 481), pays


def capture50():
    """-> (int16 [W] at 50 kHz, payloads [2, 5380])"""
    base, pays = RF.golden()
    return _capture(base, P50, Q50, SIGNAL50_HZ, RF.AMPLITUDE, RF.STARTS, 501), pays
