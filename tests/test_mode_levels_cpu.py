"""The noise levels of tests/mode_levels.py, re-derived from the oracle alone (no GPU): these are conditions on the INPUTS of
test_gpu_modes.py and of the per-mode sweeps, not measurements of the receiver.  Every mode 6 - 13 has a list-1 level (every frame
decodes with raw bit errors, and the sign-following path satisfies the list-1 pass's rule), a list level (decodes, the rule fails)
and a waterfall level (the oracle decodes between 25 % and 75 % of 48 frames); in each frozen table a vector is won by a lane above 0
(the constructed lane vectors: mode_levels.py says why no AWGN frame does)."""
import numpy as np
import pytest

import mode_levels as ML
import oracle_lib as O


@pytest.mark.parametrize("mode", ML.MODES)
def test_levels_of_a_mode(mode):
    m = ML.mode_of(mode)
    got = {}
    for kind in ("list1", "list", "waterfall"):
        pcm = ML.frames(mode, kind)
        out, res = ML.decode_batch(pcm, threads=16)
        ok = res["status"] == 0
        assert (res["oper_mode"] == mode).all() and set(res["status"].tolist()) <= {0, 6}      # every header found, whatever the payload
        for k in np.nonzero(ok)[0]:
            assert (out[k] == ML.payload(mode, int(k))).all(), (kind, k)
        got[kind] = (len(pcm), int(ok.sum()), int((ok & (res["best_lane"] > 0)).sum()))
        if kind == "waterfall":
            assert 12 <= ok.sum() <= 36, (mode, int(ok.sum()))                                 # 25 % .. 75 % of 48
            good, bad = ML.PICKS[mode]
            assert ok[good] and not ok[bad]
        else:
            assert ok.all(), (mode, kind, res["status"])
            assert (res["bit_flips"] > 0).all(), (mode, kind, res["bit_flips"])
            _, r0, tb = O.decode(pcm[0], taps=True)
            assert r0.status == 0 and r0.bit_flips == res["bit_flips"][0]
            assert ML.sc_rule(tb.llr, m.table) == (kind == "list1"), (mode, kind)              # which decoder the frame needs
            if kind == "list":
                # the lane vector of this mode: the oracle's list decoder delivers the transmitted message from a lane above 0, L = 8 and 4
                assert ML.lane_position(mode) == ML.LANE[mode][0]
                v = ML.lane_vector(mode, tb.llr)
                for L in (8, 4):
                    mesg, metric, best = ML.lanes(v, m.table, L)
                    assert best == ML.LANE[mode][1] > 0, (mode, L, best)
                    want = ML.payload(mode, 0).copy()
                    O.lib().orc_scramble(O.ptr(want), want.size)
                    assert (mesg[best][:5380] == want).all()
                    assert metric[0] < metric[best]                                            # a better path that fails the CRC-32
    assert got == ML.ORACLE[mode], (mode, got)


def test_table_is_complete():
    assert sorted(ML.LEVELS) == sorted(ML.ORACLE) == sorted(ML.PICKS) == sorted(ML.LANE) == list(ML.MODES)
    for table in (0, 1):
        modes = [m for m in ML.MODES if ML.mode_of(m).table == table]
        assert len(modes) == 4 and any(ML.LANE[m][1] > 0 for m in modes)                       # a lane above 0 wins in each frozen table
    for mode in ML.MODES:
        l1, ls, wf = (ML.LEVELS[mode][k][0] for k in ("list1", "list", "waterfall"))
        assert l1 < ls < wf
