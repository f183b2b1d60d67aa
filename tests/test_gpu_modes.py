"""Every mode of the mode table (decode.cc:302-374) held to the oracle stage by stage: the list decoder's eight lanes
(ofdmrx_debug_polar_modes), the back end on every route (ofdmrx_debug_decode_cons_modes) and the QPSK soft demapper on the
reference's own vectors - what test_gpu_parity.py proves in mode 6, for both frozen tables, QPSK and 8PSK, 256 .. 512 carriers per row
and both code lengths.  The frames and their noise levels are tests/mode_levels.py's (fixed with the oracle alone,
tests/test_mode_levels_cpu.py); the per-mode sweeps through the default path are in test_gpu_sweeps.py.

Bars: decoded bits, lanes, path metrics and every integer decision bit-exact; fp32 intermediates within REL = 1e-5 of the largest
magnitude of the compared array."""
import json
import os

import numpy as np
import pytest

import mode_levels as ML
import oracle_lib as O
from test_gpu_parity import REL, _close, _flips_ok

pytestmark = pytest.mark.gpu

KINDS = ("clean", "list1", "wf_ok", "wf_lost", "list")


@pytest.fixture(scope="module")
def frames():
    """the oracle-made frames of the stage tests with the oracle's own decode and taps: (mode, kind) -> dict.  Per mode a clean
    frame (modes 7 - 13), the first frame of the list-1 level, two frames of the waterfall level (one the oracle decodes, one it
    loses) and the first frame of the list level (the "-17 dB class")"""
    fr = {}
    for mode in ML.MODES:
        good, lost = ML.PICKS[mode]
        src = dict(clean=lambda: ML.clean(mode, 0), list1=lambda: ML.frame(mode, "list1", 0), wf_ok=lambda: ML.frame(mode, "waterfall", good),
                   wf_lost=lambda: ML.frame(mode, "waterfall", lost), list=lambda: ML.frame(mode, "list", 0))
        pay = dict(clean=0, list1=0, wf_ok=good, wf_lost=lost, list=0)
        for kind in KINDS:
            if mode == 6 and kind == "clean":
                continue                                              # (mode 6 has its own tests; it is here as a neighbour of the other table)
            pcm = src[kind]()
            out, res, tb = O.decode(pcm, taps=True)
            assert res.oper_mode == mode
            fr[(mode, kind)] = dict(pcm=pcm, payload=ML.payload(mode, pay[kind]), out=out.copy(), status=res.status, best_lane=res.best_lane,
                                    bit_flips=res.bit_flips, llr=tb.llr.copy(), cons_rot=tb.cons_rot.copy().view(np.complex64).reshape(-1),
                                    precision=tb.precision.copy())
        assert fr[(mode, "list1")]["status"] == 0 and fr[(mode, "list")]["status"] == 0
        assert fr[(mode, "wf_ok")]["status"] == 0 and fr[(mode, "wf_lost")]["status"] == 6
    return fr


@pytest.fixture(scope="module")
def polar_vectors(frames):
    """the LLR vectors of the list decoder's test: (mode, name, llr), 27 of table 0 and 28 of table 1.  The oracle's own LLRs of the
    frames above, the mode's lane vector (mode_levels.py: the oracle delivers it from lane 1), and per table a garbage vector, an
    all-erased vector and a vector with one exact zero - in these the shortened tail [cons_bits:] is 9000 for that mode's cons_bits -
    and the UNSHORTENED codeword of a random message of mesg_bits bits.  That one is there for the message's LENGTH: the message bits
    behind the CRC-32 (bit 43072 on) are the shortened code positions (encode.cc:180-186), which lengthen() marks as known zeros, so
    bytes 5384 .. 5511 are zero in every lane of every vector with that tail, and a message cut short at 5476 bytes in table 1 would go
    unnoticed; the list decoder itself takes any 65536 LLRs"""
    vec = []
    for (mode, kind), f in frames.items():
        vec.append((mode, kind, f["llr"]))
        if kind == "list":
            vec.append((mode, "lane", ML.lane_vector(mode, f["llr"])))
    rng = np.random.default_rng(60)
    for mode, name in ((7, "garbage"), (8, "erased"), (9, "zero"), (11, "garbage"), (12, "erased"), (13, "zero")):
        cb = ML.mode_of(mode).cons_bits
        if name == "garbage":
            v = rng.normal(0, 5, 65536).astype(np.float32)            # not a codeword at all
        elif name == "erased":
            v = np.zeros(65536, np.float32)                           # all-erased payload: every metric ties
        else:
            v = frames[(mode, "clean")]["llr"].copy()
            v[1234] = 0.0                                             # one exact zero among clean soft bits
        v[cb:] = 9000
        vec.append((mode, name, v))
    for mode in (6, 10):
        m = ML.mode_of(mode)
        mesg = (1 - 2 * rng.integers(0, 2, m.mesg_bits)).astype(np.int8)          # NRZ
        code = np.zeros(65536, np.int8)
        O.lib().orc_polar_sysenc(O.ptr(code), O.ptr(mesg), O.ptr(O.frozen(m.table)), 16)
        v = np.float32(3.0) * code.astype(np.float32)             # (no shortening: every message bit is free)
        om, _, _ = ML.lanes(v, m.table)
        assert (om[0][:m.mesg_bits // 8] == np.packbits(mesg < 0, bitorder="little")).all() and om[0][m.mesg_bits // 8 - 36:m.mesg_bits // 8].any()
        vec.append((mode, "random_message", v))
    for mode, name, v in vec:
        assert name == "random_message" or (v[ML.mode_of(mode).cons_bits:] == 9000).all()
    return vec


_oracle_lanes = {}


def _lanes(key, llr, table, L):
    """the oracle's lanes of a vector, computed once per list size and shared by the tests"""
    if (key, L) not in _oracle_lanes:
        _oracle_lanes[(key, L)] = ML.lanes(llr, table, L)
    return _oracle_lanes[(key, L)]


def _ordered(vec, order):
    t = [[v for v in vec if ML.mode_of(v[0]).table == tab] for tab in (0, 1)]
    for part in t:
        part.sort(key=lambda v: (v[1], v[0]))                         # neighbours within a table are of different modes
    if order == "grouped":                                            # neighbours share a table (but for the one in the middle)
        return t[0] + t[1]
    assert len(t[1]) == len(t[0]) + 1                                 # alternating: every neighbour is of the other table
    out = []
    for i in range(len(t[1])):
        out.append(t[1][i])
        if i < len(t[0]):
            out.append(t[0][i])
    return out


@pytest.mark.parametrize("order", ["alternating", "grouped"])
@pytest.mark.parametrize("list_size", [8, 4])
def test_list_decoder_all_lanes_in_every_mode(polar_vectors, list_size, order):
    """k_polar + k_finish's message gather (ofdmrx_debug_polar_modes) on identical LLRs against CODE::PolarListDecoder + systematic()
    with that mode's frozen table: all lanes' messages (mesg_bits / 8 bytes: 5476 in modes 6 - 9, 5512 in modes 10 - 13, zeros behind) and
    path metrics bit-exact.  One call of 55 vectors - an odd count - in which every neighbour is of the other frozen table, and one
    in which neighbours share a table; on the list_size 4 handle that is where same-table neighbours are decoded as a pair (two
    codewords per wave, one byte array, k_finish unpacks the nibbles) against the oracle's L = 4."""
    import modem_amd
    vec = _ordered(polar_vectors, order)
    assert len(vec) == 55
    tables = [ML.mode_of(v[0]).table for v in vec]
    changes = sum(a != b for a, b in zip(tables, tables[1:]))
    assert changes == (54 if order == "alternating" else 1)
    rx = modem_amd.Receiver(device=0, chunk_frames=64, list_size=list_size)
    try:
        mesg, metric = rx.polar(np.stack([v[2] for v in vec]), modes=[v[0] for v in vec])
    finally:
        rx.close()
    L = list_size
    assert mesg.shape == (55, 8, 5512)
    later, bad = 0, []
    for i, (mode, name, llr) in enumerate(vec):
        m = ML.mode_of(mode)
        om, omet, best = _lanes((mode, name), llr, m.table, L)
        if not ((metric[i][:L] == omet).all() and (mesg[i][:L] == om).all() and not mesg[i][:L, m.mesg_bits // 8:].any()):
            bad.append((i, mode, name, "metric" if not (metric[i][:L] == omet).all() else "message"))
        if name == "lane":
            assert best == ML.LANE[mode][1] > 0
            later += 1
    assert bad == [], (order, L, bad)
    assert later == 8


def _stack_cons(items):
    cons = np.zeros((len(items), 32400), np.complex64)
    for i, (mode, f) in enumerate(items):
        cnt = ML.mode_of(mode).cons_cnt
        cons[i, :cnt] = f["cons_rot"][:cnt]
    return cons


def test_back_end_on_every_route_in_every_mode(frames):
    """k_back, k_sc, k_polar and k_finish chained as the pipeline chains them (ofdmrx_debug_decode_cons_modes) on the oracle's rotated
    constellations of the frames of every mode in ONE batch - the list-1 pass's ring and the list decoder's queue hold both frozen
    tables - through the four routes: list decoder only; syndrome certificate first; certificate, list-1 pass, list decoder (the
    default chain); list-1 pass and list decoder.  The routes agree byte for byte; against the oracle's decode of the same frame
    payload, status and winning lane are exact, the flip count within its slack; and every route is taken in every mode."""
    import modem_amd
    keys = sorted(frames, key=lambda k: (KINDS.index(k[1]), k[0] % 4, k[0]))      # neighbouring frames: different modes, mixed tables
    items = [(k[0], frames[k]) for k in keys]
    cons = _stack_cons(items)
    modes = [k[0] for k in keys]
    rx = modem_amd.Receiver(device=0, chunk_frames=64)
    try:
        got = [rx.decode_cons(cons, use_cert=u, modes=modes) for u in (0, 1, 2, 3)]
    finally:
        rx.close()
    out0, res0, who0 = got[0]
    for u in (1, 2, 3):
        out, res, _ = got[u]
        assert (out == out0).all(), u
        for name in ("status", "best_lane", "bit_flips", "esn0_db_last", "oper_mode"):
            assert (res[name] == res0[name]).all(), (u, name, res[name], res0[name])
    assert list(res0["oper_mode"]) == modes and (who0 == 0).all()
    for i, ((mode, kind), (_, f)) in enumerate(zip(keys, items)):
        assert int(res0["status"][i]) == f["status"] and int(res0["best_lane"][i]) == f["best_lane"], (mode, kind, res0["status"][i], res0["best_lane"][i])
        assert (out0[i] == f["out"]).all(), (mode, kind)
        if f["status"] == 0:
            assert (out0[i] == f["payload"]).all() and _flips_ok(res0["bit_flips"][i], f["bit_flips"]), (mode, kind, res0["bit_flips"][i], f["bit_flips"])
    who = {u: dict(zip(keys, got[u][2])) for u in (1, 2, 3)}
    for mode in range(7, 14):
        assert who[1][(mode, "clean")] == 1 and who[2][(mode, "clean")] == 1, mode           # certified
        assert who[3][(mode, "clean")] == 2, mode                                            # without the certificate: the list-1 pass
    for mode in ML.MODES:
        assert who[1][(mode, "list1")] == 0 and who[2][(mode, "list1")] == 2 and who[3][(mode, "list1")] == 2, mode   # finished by the list-1 pass
        assert who[2][(mode, "list")] == 0 and who[3][(mode, "list")] == 0, mode             # the rule fails (test_mode_levels_cpu.py)
    for table in (0, 1):
        assert any(who[2][(mode, kind)] == 0 for mode in ML.MODES if ML.mode_of(mode).table == table for kind in ("wf_ok", "wf_lost"))


def test_back_end_taps_at_the_list1_level_in_every_mode(frames):
    """the per-row precision (decode.cc:516) and the LLRs (decode.cc:520-529) of k_back from the oracle's rotated constellation of a frame
    with raw bit errors, every mode in one batch: within REL of the oracle's taps; the shortened tail is lengthen()'s 9000"""
    import modem_amd
    keys = [(mode, "list1") for mode in (13, 7, 12, 8, 11, 9, 10, 6)]
    rx = modem_amd.Receiver(device=0, chunk_frames=16, keep_raw_cons=True)
    try:
        out, res, _ = rx.decode_cons(_stack_cons([(k[0], frames[k]) for k in keys]), use_cert=0, modes=[k[0] for k in keys])
        for i, k in enumerate(keys):
            m, f = ML.mode_of(k[0]), frames[k]
            assert int(res["status"][i]) == 0 and (out[i] == f["payload"]).all()
            _close(rx.tap("PRECISION", i, rows=m.cons_rows), f["precision"][:m.cons_rows], what="precision, mode %d" % k[0])
            llr = rx.tap("LLR", i)
            _close(llr[:m.cons_bits], f["llr"][:m.cons_bits], what="llr, mode %d" % k[0])
            assert (llr[m.cons_bits:] == 9000).all(), k
    finally:
        rx.close()


@pytest.mark.parametrize("mode,row", [(8, 17), (13, 101)])
def test_qpsk_demapper_on_the_reference_vectors(frames, mode, row):
    """psk.hh:76-80 on the GPU against the vectors the REAL header produced (tests/golden/psk_vectors.json, psk4: zeros of either sign,
    axes, diagonals, tiny and huge magnitudes): the 206 points are planted into one row of a clean frame's constellation - mode 8, 400
    columns, and mode 13, 256 columns - and go through k_back like any other (use_cert 0, rotation = identity).  The row's precision
    is the frame's own (decode.cc:516), so a soft value is the vector's times the ratio of the two precisions: exact zeros stay exact
    and every sign is the header's `hard`.  Magnitudes: the QPSK soft bit is value * (DIST * precision), TWO roundings (the product
    DIST * precision, then the product with the value) where the 8PSK test's worst bit has four; each side's result is within
    (1 + u)^2 of the exact product, u = 2^-24, so the two differ by at most 4 u (1 + 2 u) of the value - 2 ulps, not the 4 of the 8PSK test."""
    import modem_amd
    vec = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "psk_vectors.json")))["psk4"]
    m = ML.mode_of(mode)
    assert m.mod_bits == 2 and len(vec) <= m.cons_cols and row < m.cons_rows
    cons = np.zeros((1, 32400), np.complex64)
    cons[0, :m.cons_cnt] = frames[(mode, "clean")]["cons_rot"][:m.cons_cnt]
    pts = np.array([complex(float.fromhex(v["re"]), float.fromhex(v["im"])) for v in vec], np.complex64)
    at = row * m.cons_cols
    cons[0, at:at + len(pts)] = pts
    rx = modem_amd.Receiver(device=0, chunk_frames=16, keep_raw_cons=True)
    try:
        rx.decode_cons(cons, use_cert=0, modes=[mode])
        llr = rx.tap("LLR", 0)
        prec = rx.tap("PRECISION", 0, rows=m.cons_rows)[row]
    finally:
        rx.close()
    assert prec > 0
    bound = 4 * 2.0 ** -24 * (1 + 2.0 ** -23)
    checked = zeros = 0
    for i, v in enumerate(vec):
        got = llr[2 * (at + i): 2 * (at + i) + 2]
        ratio = np.float64(prec) / float.fromhex(v["precision"])
        for b in range(2):
            want = float.fromhex(v["soft"][b])
            if want == 0.0:
                assert got[b] == 0.0, (i, b, got[b])                  # a zero coordinate stays an exact zero
                zeros += 1
            else:
                assert (got[b] < 0) == (v["hard"][b] < 0) and (got[b] < 0) == (want < 0), (i, b, got[b], want)
                if np.isfinite(want * ratio) and abs(want * ratio) > 1e-30:
                    assert abs(got[b] - want * ratio) <= bound * abs(want * ratio), (i, b, got[b], want * ratio)
            checked += 1
    assert checked == 2 * len(vec) and zeros >= 6
    assert (llr[m.cons_bits:] == 9000).all()


@pytest.mark.parametrize("mode", [8, 12])
def test_a_later_lane_wins_through_the_back_end(frames, mode):
    """k_finish chooses a lane above 0 in both frozen tables: the list-level frame of a QPSK mode with the coordinates that carry the
    soft bits of mode_levels.py's weight-32 codeword turned weakly (factor -0.3; psk.hh:76-80: bit 0 is re, bit 1 is im) goes through
    k_back, k_polar and k_finish.  The reference is the oracle's list decoder on the LLRs k_back made (the LLR tap): same metrics, and
    the payload is that of the lane decode.cc:532-541 takes - a lane above 0 - on every route (all lanes' messages on identical LLRs:
    test_list_decoder_all_lanes_in_every_mode)."""
    import modem_amd
    m, f = ML.mode_of(mode), frames[(mode, "list")]
    cons = np.zeros((1, 32400), np.complex64)
    cons[0, :m.cons_cnt] = f["cons_rot"][:m.cons_cnt]
    v = cons.view(np.float32).reshape(-1)                            # (re, im) pairs: QPSK soft bit p is coordinate p
    v[np.flatnonzero(ML.codeword_of(ML.LANE[mode][0]))] *= np.float32(ML.LANE_FACTOR)
    rxk = modem_amd.Receiver(device=0, chunk_frames=16, keep_raw_cons=True)
    try:
        out, res, _ = rxk.decode_cons(cons, use_cert=0, modes=[mode])
        llr, metric = rxk.tap("LLR", 0), rxk.tap("METRIC", 0)
    finally:
        rxk.close()
    om, omet, best = ML.lanes(llr, m.table)
    assert best >= 1, best                                            # (a condition on the input: the turned codeword's path fails the CRC-32)
    assert (metric == omet).all(), (metric, omet)
    want = om[best][:5380].copy()
    O.lib().orc_scramble(O.ptr(want), want.size)                      # decode.cc:613-615
    assert int(res["status"][0]) == 0 and int(res["best_lane"][0]) == best and (out[0] == want).all() and (want == f["payload"]).all()
    rx = modem_amd.Receiver(device=0, chunk_frames=16)
    try:
        for u in (1, 2, 3):
            o, r, who = rx.decode_cons(cons, use_cert=u, modes=[mode])
            assert who[0] == 0 and (o == out).all(), u
            for name in ("status", "best_lane", "bit_flips", "esn0_db_last", "oper_mode"):
                assert r[name][0] == res[name][0], (u, name)
    finally:
        rx.close()
