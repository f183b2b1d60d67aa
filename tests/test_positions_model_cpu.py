"""The inputs of test_gpu_positions.py are sound, and the reference alone meets every condition the GPU tests impose: the oracle on
a sparse subset of each sweep (every 64th offset, the ends, the three offsets around each crossing of a multiple of 1024) and on the
whole stream-end and stream-head sets.  No GPU."""
import pytest

import positions as P


@pytest.mark.parametrize("name", P.FULL + P.PARTIAL)
def test_sparse_windows_decode_and_the_edge_moves_one_per_offset(name):
    sw = P.sweep(name)
    offs = P.seam_offsets(name)
    refs = sw.refs(offs)
    for d, r in zip(offs, refs):
        assert r.status == 0 and (r.payload == sw.payload).all(), (name, d, r.status)
        assert r.oper_mode == 6 and r.n_sync_rejects == (1 if sw.with_burst else 0), (name, d, r.n_sync_rejects)
    # the prefix length did what it was chosen for: g = residue (mod 4096) at offset 0, one less per offset - measured at the sampled
    # offsets, which include both ends and the crossing, so the consecutive offsets between them take every residue in between
    g = [P.falling_edge(r, sw.rate) for r in refs]
    assert [(gi + d) % P.STREAM_TILE for gi, d in zip(g, offs)] == [sw.residue] * len(offs)
    assert [gi + d for gi, d in zip(g, offs)] == [g[0] + offs[0]] * len(offs)
    res1024 = {(sw.residue - d) % P.SYNC_TILE for d in sw.offsets}
    res4096 = {(sw.residue - d) % P.STREAM_TILE for d in sw.offsets}
    got1024 = set(P.edge_residues(sw, refs, offs, P.SYNC_TILE))
    assert {P.SYNC_TILE - 1, 0, 1} <= got1024 <= res1024
    if name in P.FULL:
        assert res1024 == set(range(P.SYNC_TILE)) and {P.STREAM_TILE - 1, 0, 1} <= res4096
        assert {P.STREAM_TILE - 1, 0, 1} <= set(P.edge_residues(sw, refs, offs, P.STREAM_TILE))
        # n_preambles of the streams sweep: the oracle finds nothing behind the frame
        probe = [offs[0], offs[-1]] + P.crossing_offsets(name)
        assert all(r.status == 1 for r in sw.refs(probe, skip=1))
    assert sw.L + max(sw.offsets) == len(sw.stream) and min(sw.offsets) >= 0


@pytest.mark.parametrize("name", ["8k2", "8k1"])
def test_stream_end_threshold_flips_once(name):
    sw = P.sweep(name)
    n_star, lengths = P.end_lengths(name)
    refs = P.end_refs(name, lengths)
    assert len(lengths) == 21 and n_star in lengths
    assert [r.status == 1 for r in refs] == [n < n_star for n in lengths]   # NO_SYNC below n*, an accepted preamble from n* on
    full = P.oracle_run(name, sw.stream, [(0, len(sw.stream))], sw.rate)[0]
    rc = P.rate_cfg(sw.rate)
    assert full.sc_start < n_star <= full.sc_start + rc.buffer_len
    for n, r in zip(lengths, refs):
        if r.status != 1:
            assert (r.sc_start, r.symbol_pos, r.n_sync_rejects) == (full.sc_start, full.symbol_pos, 0), n
            assert r.oper_mode == 6 and r.call_sign == full.call_sign, n
    # a buffer that holds the last payload symbol decodes to the payload
    pay_end = max(lengths) - 3
    assert all(r.status == 0 and (r.payload == sw.payload).all() for n, r in zip(lengths, refs) if n >= pay_end)


@pytest.mark.parametrize("name", ["8k2", "8k1"])
def test_stream_head_cuts(name):
    sw = P.sweep(name)
    frame, c_star, cuts = P.head_cuts(name)
    refs = P.head_refs(name, frame, cuts)
    assert set(sw.rate - k for k in P.HEAD_KEEP) <= set(cuts) and {c_star + k for k in range(-3, 4)} <= set(cuts)
    by = dict(zip(cuts, refs))
    assert by[c_star].status == 1 and by[c_star - 1].status != 1 and c_star > sw.rate
    whole = by[sw.rate - 1025]
    for c, r in zip(cuts, refs):
        if c <= sw.rate:                                          # only silence is cut: the frame decodes, at the same stream position
            assert r.status == 0 and (r.payload == sw.payload).all(), c
            assert r.sc_start + c == whole.sc_start + sw.rate - 1025, c
        elif r.status == 0:
            assert (r.payload == sw.payload).all(), c
