"""The live feed bank's segmented windowed scan without a GPU: several adversarial timing sequences, cut at random positions per
channel and pushed in interleaved rounds through ONE driver (bank_model.py), give for every channel the falling edges, t_max and
index_max of the serial transcription of decode.cc:93-116 run on that channel alone."""
import numpy as np
import pytest

from bank_model import bank_edges
from stream_model import RATES, adversarial, serial_edges

N = 1 << 17
C = 5


@pytest.fixture(scope="module", params=[8000, 48000])
def case(request):
    ml, hs, gl = RATES[request.param]
    ts = [adversarial(N - 3000 * c, 3 + c, ml) for c in range(C)]
    return (ml, hs, gl), ts, [serial_edges(t, ml, hs, gl) for t in ts]


def _rounds(ts, rng, n_rounds, early=None):
    """random cut sets per channel, zero-length shares among them, as rounds[r][c]; early: {channel: samples it stops after}"""
    cols = []
    for c, t in enumerate(ts):
        n = len(t) if not early or c not in early else early[c]
        cuts = np.sort(rng.integers(0, n + 1, size=n_rounds - 1))
        cuts[rng.integers(0, n_rounds - 1, size=4)] = rng.choice([4096, 4097, 8191, 8192], size=4)   # on and beside tile boundaries
        cuts = np.sort(cuts)
        pos = np.concatenate([[0], cuts, [n]])
        cols.append(np.diff(pos).tolist())
    return [[col[r] for col in cols] for r in range(n_rounds)]


@pytest.mark.parametrize("seed", [0, 1])
def test_random_interleaved_cuts(case, seed):
    (ml, hs, gl), ts, want = case
    rng = np.random.default_rng(seed)
    rounds = _rounds(ts, rng, 30)
    assert any(n == 0 for r in rounds for n in r)                # zero-length shares
    got = bank_edges(ts, rounds, match_len=ml, symbol_len=hs, guard_len=gl)
    for c in range(C):
        assert len(want[c][0]) > 10
        for g, w in zip(got[c], want[c]):
            np.testing.assert_array_equal(g, w)


def test_channels_that_end_early(case):
    """two channels stop early - one on a tile boundary, one inside a tile - while their neighbours go on: each equals the serial scan
    of what it was fed, and the neighbours are unaffected"""
    (ml, hs, gl), ts, want = case
    rng = np.random.default_rng(5)
    early = {1: 6 * 4096, 3: 40000 + 17}
    rounds = _rounds(ts, rng, 24, early=early)
    ends = {}
    for c in early:                                              # the channel ends with the round that brings its last sample
        last = max(r for r in range(len(rounds)) if rounds[r][c] > 0)
        ends.setdefault(last, []).append(c)
    got = bank_edges(ts, rounds, ends=ends, match_len=ml, symbol_len=hs, guard_len=gl)
    for c in range(C):
        w = serial_edges(ts[c][:early[c]], ml, hs, gl) if c in early else want[c]
        for g, x in zip(got[c], w):
            np.testing.assert_array_equal(g, x)


def test_a_silent_neighbour_and_a_late_starter(case):
    """one channel gets everything in its first push, one nothing until the others have finished"""
    (ml, hs, gl), ts, want = case
    ts = ts[:3]
    n = [len(t) for t in ts]
    rounds = [[n[0], 5000, 0]] + [[0, 7000, 0]] * ((n[1] - 5000 + 6999) // 7000) + [[0, 0, n[2]]]
    rounds = [[min(x, left) for x, left in zip(r, [n[c] - sum(q[c] for q in rounds[:i]) for c in range(3)])] for i, r in enumerate(rounds)]
    got = bank_edges(ts, rounds, match_len=ml, symbol_len=hs, guard_len=gl)
    for c in range(3):
        for g, w in zip(got[c], want[c]):
            np.testing.assert_array_equal(g, w)
