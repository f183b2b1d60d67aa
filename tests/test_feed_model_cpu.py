"""The live feed's carry logic without a GPU: an adversarial timing sequence cut at random positions and scanned push by push
(feed_model.py) gives the falling edges, t_max and index_max of the serial transcription of decode.cc:93-116."""
import numpy as np
import pytest

from feed_model import feed_edges
from stream_model import RATES, adversarial, serial_edges

N = 1 << 18


@pytest.fixture(scope="module", params=[8000, 48000])
def case(request):
    ml, hs, gl = RATES[request.param]
    t = adversarial(N, 3, ml)
    return (ml, hs, gl), t, serial_edges(t, ml, hs, gl)


@pytest.mark.parametrize("seed", [0, 1])
def test_random_cuts(case, seed):
    (ml, hs, gl), t, want = case
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(0, N + 1, size=40))
    cuts = np.concatenate([cuts, cuts[:3], [4096, 4097, 8191]])      # zero-length pushes, cuts on and beside tile boundaries
    got = feed_edges(t, np.sort(cuts), match_len=ml, symbol_len=hs, guard_len=gl)
    assert len(want[0]) > 20
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_one_sample_pushes(case):
    (ml, hs, gl), t, want = case
    n = 3 * 4096 + 5
    w = serial_edges(t[:n], ml, hs, gl)
    got = feed_edges(t[:n], list(range(1, n)), match_len=ml, symbol_len=hs, guard_len=gl)
    for g, x in zip(got, w):
        np.testing.assert_array_equal(g, x)
