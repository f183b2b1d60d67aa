"""The preamble's position swept through every alignment of the scan tiles (tests/positions.py builds the inputs).

Every synchronisation kernel walks a recording in fixed tiles - k_sync: 64 lanes x SYNC_PER sample times, the stream scan: 4096 - and
carries the window sums, the Schmitt trigger, the running maximum, the m ring and (mono) the analytic-signal cover from one tile to
the next; k_header / k_demod chunk the mono front end by 8, 5 and 64 samples.  One clean mode-6 frame behind a noise prefix is
decoded from the windows S[d : d + L] of consecutive offsets d, so that the trigger's rising edge, its arg-max and its falling edge
g = sc_start - symbol_pos + BUFFER_LEN - 1 land on every residue of those tiles, through ofdmrx_decode_batch and through
ofdmrx_decode_streams, at 8 kHz (2-channel, with a rejected trigger in front, mono) and, for 256 offsets, at 48 kHz 2-channel and
44.1 kHz mono (and 16 kHz mono: the same SPLIT code with smaller constants); then the buffers that end around the point where the preamble is first accepted, and the ones that begin inside the
leading silence and the pilot symbol.  Every window is compared with the oracle's decode of the same window.
"""
import numpy as np
import pytest

import positions as P

pytestmark = pytest.mark.gpu

# cfo_rad: the tolerances of test_gpu_parity.py (REL at 8 kHz, 2e-7 in test_other_rates_decode_matches_oracle)
CFO_TOL = {8000: 1e-5, 16000: 2e-7, 44100: 2e-7, 48000: 2e-7}


@pytest.fixture(scope="module")
def rxs():
    """default handles (chunk_frames = 64, no debug flag: the product path), one per rate, made when first asked for"""
    import modem_amd
    made = {}

    def get(rate):
        if rate not in made:
            made[rate] = modem_amd.Receiver(device=0, chunk_frames=64, sample_rate=rate)
        return made[rate]
    yield get
    for r in made.values():
        r.close()


def _must_decode(tag, g, out, ref, payload, rate):
    """a window that holds the whole frame: status 0 and the transmitted payload (no oracle needed), the integer sync fields and the
    header fields equal to the oracle's for that window, cfo_rad within the project's tolerance -> list of what differs"""
    bad = []
    if int(g["status"]) != 0 or not (out == payload).all():
        bad.append((tag, "status/payload", int(g["status"]), int((out != payload).sum())))
    if ref.status != 0 or not (ref.payload == payload).all():
        bad.append((tag, "oracle status/payload", ref.status))
    for name in ("sc_start", "symbol_pos", "n_sync_rejects", "oper_mode", "call_sign"):
        if int(g[name]) != getattr(ref, name):
            bad.append((tag, name, int(g[name]), getattr(ref, name)))
    if not abs(float(g["cfo_rad"]) - ref.cfo_rad) <= CFO_TOL[rate]:
        bad.append((tag, "cfo_rad", float(g["cfo_rad"]), ref.cfo_rad))
    return bad


def _as_oracle(tag, g, out, ref, rate):
    """a buffer that may hold only part of the frame: status and sc_start as the oracle's; for an accepted preamble the other sync
    fields, for a header that decoded its fields, for status 0 the payload"""
    bad = []
    for name in ("status", "sc_start"):
        if int(g[name]) != getattr(ref, name):
            bad.append((tag, name, int(g[name]), getattr(ref, name)))
    if ref.status != 1:
        for name in ("symbol_pos", "n_sync_rejects"):
            if int(g[name]) != getattr(ref, name):
                bad.append((tag, name, int(g[name]), getattr(ref, name)))
        if not abs(float(g["cfo_rad"]) - ref.cfo_rad) <= CFO_TOL[rate]:
            bad.append((tag, "cfo_rad", float(g["cfo_rad"]), ref.cfo_rad))
    if ref.status in (0, 6):
        for name in ("oper_mode", "call_sign"):
            if int(g[name]) != getattr(ref, name):
                bad.append((tag, name, int(g[name]), getattr(ref, name)))
    if ref.status == 0 and not (out == ref.payload).all():
        bad.append((tag, "payload", int((out != ref.payload).sum())))
    return bad


# ---------------------------------------------------------------- ofdmrx_decode_batch over the windows
@pytest.mark.parametrize("name,k", P.piece_ids())
def test_batch_sweep(rxs, name, k):
    """PIECE consecutive offsets of one sweep in one call of Receiver.decode.  8k2 / 8k2b / 8k1: k_sync<8000, SPLIT, MONO> and
    k_sync_accept, twice for 8k2b (a rejected trigger, then the accepted one), the fused mono path for 8k1 - the payload of every
    window is the check on k_header / k_demod at every residue modulo 64, 320 and 512.  48k2 / 44k1 / 44k1b / 16k1: the SPLIT scan of the
    other rates, launch_front_end over the whole stream for mono"""
    sw = P.sweep(name)
    offs = sw.pieces()[k]
    refs = sw.refs(offs)
    out, res = rxs(sw.rate).decode(sw.windows(offs))
    bad = []
    for i, d in enumerate(offs):
        bad += _must_decode(d, res[i], out[i], refs[i], sw.payload, sw.rate)
        if sw.with_burst and refs[i].n_sync_rejects < 1:
            bad.append((d, "the burst did not trigger in the oracle"))
    assert not bad, (name, len(bad), bad[:24])


# ---------------------------------------------------------------- ofdmrx_decode_streams over the same windows
@pytest.mark.parametrize("name,k", P.piece_ids(P.FULL))
def test_streams_sweep(rxs, name, k):
    """the same windows (and the same oracle results) as recordings of one ofdmrx_decode_streams call: k_stream_tile, the segmented
    trigger scan over tiles of 4096 and k_stream_accept.  Two recordings that hold the prefix only (all of it, half of it) sit in
    front of and between the windows, so the batch is ragged and a trigger state that leaked into the next recording would show.
    Every window gives exactly one record; n_preambles is the number of ACCEPTED preambles (ofdmrx.h: the smallest k for which
    the oracle's decode with SKIP = k reports NO_SYNC), 1 here - the rejected trigger of 8k2b is counted in the record's
    n_sync_rejects, which must be the oracle's.  The oracle's SKIP = 1 run is made for the first and the last window of the piece and
    for the windows around a multiple of 1024."""
    sw = P.sweep(name)
    offs = sw.pieces()[k]
    refs = sw.refs(offs)
    extra = [(0, sw.frame_at), (0, sw.frame_at // 2 + 1)]
    xrefs = P.oracle_run(name, sw.stream, extra, sw.rate)
    half = len(offs) // 2
    recs = [sw.stream[:extra[0][1]]] + [sw.window(d) for d in offs[:half]] + [sw.stream[:extra[1][1]]] + [sw.window(d) for d in offs[half:]]
    want = [xrefs[0]] + refs[:half] + [xrefs[1]] + refs[half:]
    tags = ["prefix"] + offs[:half] + ["half prefix"] + offs[half:]
    got = rxs(sw.rate).decode_streams(recs, stride_samples=(sw.L + 1) // 2 * 2)
    assert len(got) == len(recs)
    bad = []
    for tag, ref, (o, r, npre) in zip(tags, want, got):
        if isinstance(tag, str):
            if ref.status != 1 or npre != 0 or len(r) != 0:
                bad.append((tag, "a recording without a frame", ref.status, npre))
            continue
        if npre != 1 or len(r) != 1:
            bad.append((tag, "n_preambles", npre, len(r)))
            continue
        bad += _must_decode(tag, r[0], o[0], ref, sw.payload, sw.rate)
    assert not bad, (name, len(bad), bad[:24])
    probe = sorted({offs[0], offs[-1]} | (set(P.crossing_offsets(name)) & set(offs)))
    assert all(r.status == 1 for r in sw.refs(probe, skip=1)), "the oracle finds a second preamble"


# ---------------------------------------------------------------- the sweeps did reach the seams
@pytest.mark.parametrize("name", P.FULL)
def test_full_sweeps_cover_every_tile_residue(name):
    """from the oracle's own results for the windows above: the falling edge takes every residue modulo 1024 (so also modulo a tile
    of 512), and 4095, 0 and 1 modulo the stream tile"""
    sw = P.sweep(name)
    refs = sw.refs(sw.offsets)
    assert set(P.edge_residues(sw, refs, sw.offsets, P.SYNC_TILE)) == set(range(P.SYNC_TILE))
    assert {4095, 0, 1} <= set(P.edge_residues(sw, refs, sw.offsets, P.STREAM_TILE))
    if sw.with_burst:
        assert all(r.n_sync_rejects >= 1 for r in refs)


@pytest.mark.parametrize("name", P.PARTIAL)
def test_partial_sweeps_cross_a_tile(name):
    sw = P.sweep(name)
    refs = sw.refs(sw.offsets)
    assert {1023, 0, 1} <= set(P.edge_residues(sw, refs, sw.offsets, P.SYNC_TILE))
    if sw.with_burst:
        assert all(r.n_sync_rejects >= 1 for r in refs)


# ---------------------------------------------------------------- the stream ends / begins inside the preamble
def _each_and_together(rx, bufs, refs, tags, rate):
    """every buffer in a call of its own (ofdmrx_decode_batch takes one length per call), then all of them as the recordings of one
    ofdmrx_decode_streams call: no record where the oracle reports NO_SYNC, one otherwise"""
    bad = []
    for tag, x, ref in zip(tags, bufs, refs):
        out, res = rx.decode(x[None])
        bad += _as_oracle(("batch", tag), res[0], out[0], ref, rate)
    got = rx.decode_streams(bufs, stride_samples=(max(len(x) for x in bufs) + 1) // 2 * 2)
    for tag, ref, (o, r, npre) in zip(tags, refs, got):
        if npre != (0 if ref.status == 1 else 1) or len(r) != npre:
            bad.append((("streams", tag), "n_preambles", npre, len(r), ref.status))
        elif npre:
            bad += _as_oracle(("streams", tag), r[0], o[0], ref, rate)
    return bad


@pytest.mark.parametrize("name", ["8k2", "8k1"])
def test_stream_end(rxs, name):
    """S[:n] for n around n* (the shortest buffer in which the oracle accepts the preamble: tile_end == n inside the trigger's run),
    around the end of the header symbol and around the end of the last payload symbol"""
    sw = P.sweep(name)
    n_star, lengths = P.end_lengths(name)
    refs = P.end_refs(name, lengths)
    assert [r.status == 1 for r in refs] == [n < n_star for n in lengths]
    assert any(r.status == 0 for r in refs)
    bad = _each_and_together(rxs(sw.rate), [sw.stream[:n] for n in lengths], refs, lengths, sw.rate)
    assert not bad, (name, n_star, len(bad), bad[:24])


@pytest.mark.parametrize("name", ["8k2", "8k1"])
def test_stream_head(rxs, name):
    """F[c:]: the frame's leading silence cut to 0 .. 1025 samples, then cuts into the pilot symbol and on into the preamble until
    the oracle no longer accepts it (the head-of-stream branches of the scan: w_lo < 0, FIRST, tp >= 0, t - MATCH_LEN >= 0; a
    preamble that begins before sample 0 has a negative sc_start)"""
    sw = P.sweep(name)
    frame, c_star, cuts = P.head_cuts(name)
    refs = P.head_refs(name, frame, cuts)
    assert refs[0].status == 0 and refs[-1].status == 1
    bad = _each_and_together(rxs(sw.rate), [frame[c:] for c in cuts], refs, cuts, sw.rate)
    assert not bad, (name, c_star, len(bad), bad[:24])
