"""The stream scan's trigger (k_stream.hip) as a model: tiles + a scan over per-tile functions give exactly the falling edges, t_max
and index_max of the serial trigger of decode.cc:93-116."""
import numpy as np
import pytest

from stream_model import RATES, adversarial, serial_edges, thresholds, tiled_edges


def _same(timing, tile, rate=8000):
    ml, hs, gl = RATES[rate]
    a = serial_edges(timing, ml, hs, gl)
    b = tiled_edges(timing, tile, ml, hs, gl)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    return len(a[0])


@pytest.mark.parametrize("tile", [1, 2, 3, 7, 64, 257, 4096])
def test_random_and_adversarial(tile):
    rng = np.random.default_rng(tile)
    total = 0
    for seed in range(3):
        total += _same(adversarial(6000, seed), tile)
        total += _same(rng.uniform(0, 60, size=3000).astype(np.float32), tile)
    assert total > 50


def test_values_exactly_at_the_thresholds():
    lo, hi = thresholds(161)
    seq = np.array([hi, hi, 2 * hi, hi, lo, lo, np.nextafter(lo, np.float32(0)), hi, np.nextafter(hi, np.float32(99)), lo,
                    np.nextafter(lo, np.float32(0))], np.float32)
    te, tm, im = serial_edges(seq)
    assert list(te) == [6, 10] and list(tm) == [2, 8]        # hi itself sets nothing, lo itself clears nothing
    for tile in (1, 2, 3, 4, 16):
        _same(seq, tile)


def test_runs_over_many_tiles_ties_and_saturation():
    lo, hi = thresholds(161)
    seq = np.full(50000, (lo + hi) / 2, np.float32)
    seq[100] = 2 * hi                                          # a run that starts here, holds over ~12 tiles of 4096
    seq[30000] = 2 * hi                                        # a tie: the first index keeps the maximum
    seq[49000] = lo / 2                                        # its falling edge
    te, tm, im = serial_edges(seq)
    assert list(te) == [49000] and list(tm) == [100] and list(im) == [640 + 160 + 80]   # saturated
    for tile in (1, 5, 4096):
        _same(seq, tile)


def test_run_open_at_the_end_and_edge_on_a_tile_boundary():
    lo, hi = thresholds(161)
    seq = np.zeros(3 * 4096, np.float32)
    seq[4000:4096] = 2 * hi
    seq[4096] = 0                                              # an edge on the first sample of a tile
    seq[8000:] = 2 * hi                                        # still collecting when the stream ends
    te, tm, im = serial_edges(seq)
    assert list(te) == [4096] and list(tm) == [4000] and list(im) == [80 + 96]
    for tile in (1, 4096, 2048, 96):
        _same(seq, tile)


@pytest.mark.parametrize("rate", [16000, 44100, 48000])
def test_other_rates(rate):
    ml, _, _ = RATES[rate]
    _same(adversarial(20000, 7, ml), 4096, rate)
    _same(adversarial(20000, 8, ml), 33, rate)
