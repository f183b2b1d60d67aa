"""The segmented trigger scan of ofdmrx_decode_streams as a model (streams_model.py): composing every recording's
tiles in one scan that resets at recording starts gives, per recording, exactly the serial trigger of decode.cc:93-116 run on that
recording alone."""
import numpy as np
import pytest

from stream_model import RATES, adversarial, serial_edges, thresholds
from streams_model import leak_pair, segmented_edges


def _same(timings, tile, rate=8000):
    ml, hs, gl = RATES[rate]
    got = segmented_edges(timings, tile, ml, hs, gl)
    total = 0
    for t, g in zip(timings, got):
        ref = serial_edges(t, ml, hs, gl)
        for x, y in zip(ref, g):
            np.testing.assert_array_equal(x, y)
        total += len(ref[0])
    return total


def _batch(seed, lens, ml=161):
    return [adversarial(n, seed + 31 * q, ml) if n else np.zeros(0, np.float32) for q, n in enumerate(lens)]


@pytest.mark.parametrize("tile", [1, 2, 3, 7, 64, 257, 1000, 4095, 4096])
def test_segmented_equals_serial_per_recording(tile):
    # lengths around the tile and around 4096, an empty recording, a one-sample one
    lens = [1, tile, tile + 1, 0, max(1, tile - 1), 3 * tile + 17, 2500, 1]
    total = _same(_batch(tile, lens), tile)
    rng = np.random.default_rng(tile)
    total += _same([rng.uniform(0, 60, size=n).astype(np.float32) for n in (700, 1, 1300)], tile)
    assert total > 20


@pytest.mark.parametrize("tile", [1, 5, 96, 4096])
def test_no_state_crosses_a_recording_start(tile):
    a, b = leak_pair()
    lo, hi = thresholds(161)
    ra, rb = segmented_edges([a, b], tile)
    assert len(ra[0]) == 0 and len(rb[0]) == 0                   # a: still collecting at its end; b: never set
    assert len(serial_edges(np.concatenate([a, b]))[0]) == 1     # (the leak this guards against: one stream, one edge)
    # the running maximum does not cross either: b's own run reports its own maximum, not a's larger one
    b2 = b.copy()
    b2[10] = np.nextafter(hi, np.float32(100))
    r = segmented_edges([a, b2, a, b2], tile)
    assert list(r[1][0]) == [len(b) // 2] and list(r[1][1]) == [10]
    assert list(r[3][0]) == [len(b) // 2] and list(r[3][1]) == [10]
    _same([a, b2, a, b2], tile)


@pytest.mark.parametrize("rate", [16000, 48000])
def test_other_rates(rate):
    ml, _, _ = RATES[rate]
    _same(_batch(5, [4097, 1, 9000, 33], ml), 4096, rate)
    _same(_batch(6, [700, 0, 900], ml), 33, rate)
