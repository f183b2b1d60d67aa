"""The premises of tests/osd_vectors.py, checked on the CPU oracle alone (no GPU): what test_gpu_header.py then asks of the kernels
rests on these."""
import ctypes as C

import numpy as np

import oracle_lib as O
import osd_vectors as V


def test_mrb_restates_the_oracles_information_set():
    """flips placed at ranks taken from mrb() are exactly the flips the oracle's search undoes: constructed() asserts the premise per
    vector, the oracle returns the constructed codeword and calls it unique for every one of them - runs of three and four ranks
    from 0 to 70, the extremes, random patterns, marginal premises, plateaus, -128, 0 - 9 column swaps"""
    vecs = V.constructed()
    assert len(vecs) == 68 + 69 + len(V.EXTREMES) + 4 * 24 + 24
    V.constructed_conditions(vecs)
    bits, uniq = V.oracle_osd(np.stack([v.soft for v in vecs]))
    bad = [v for v, b, u in zip(vecs, bits, uniq) if u != 1 or not (b == v.c).all()]
    assert not bad, bad


def test_constructed_vectors_take_the_route_their_order_predicts():
    """order 0: the hard decisions are the codeword (route 1).  Orders 1 and 2: c is among the 2557 candidates and, being the strict
    optimum of the code by a margin the bound sees, certified (route 2).  Orders 3 and 4: c is not among them, and no other codeword
    may be certified: route 3"""
    for v in V.constructed():
        r, c = V.route_detail(v.soft)
        k = len(v.ranks)
        assert r == (1 if k == 0 else 2 if k <= 2 else 3), v
        if r != 3:
            assert (c == v.c).all(), v


def test_tie_families_hold_both_kinds():
    """between 25 % and 85 % of each family is unique under the oracle (a property of the inputs: the GPU test must not pass on a
    sample of one kind); every one of the 256 words needs the full search"""
    for fam in V.ties():
        _, uniq = V.oracle_osd(fam)
        share = uniq.mean()
        assert 0.25 <= share <= 0.85, share
        assert all(V.route(s) == 3 for s in fam)


def test_route_names_what_the_exhaustive_search_returns():
    """the rule behind shortcut 2 (and 1) on the oracle: wherever route() says 1 or 2, the oracle's full order-4 search returns the
    codeword that route names, and calls it unique"""
    rng = np.random.default_rng(64)
    softs = []
    for t in range(64):
        c = V._random_codeword(rng)
        amp, sigma = [(40, 12), (24, 14), (16, 14), (12, 13)][t % 4]
        s = np.rint(amp * (1 - 2 * c.astype(np.int32)) + rng.normal(0, sigma, V.N))
        if t % 8 == 5:
            s[rng.choice(V.N, 20, replace=False)] = 0                # more zeros than route 1 allows
        softs.append(np.clip(s, -128, 127).astype(np.int8))
    softs = np.stack(softs)
    named = [V.route_detail(s) for s in softs]
    routes = [r for r, _ in named]
    assert routes.count(1) >= 8 and routes.count(2) >= 8 and routes.count(3) >= 8, np.bincount(routes)
    bits, uniq = V.oracle_osd(softs)
    for i, (r, c) in enumerate(named):
        if r != 3:
            assert uniq[i] == 1 and (bits[i] == c).all(), (i, r)


def test_header_fields():
    """decode.cc:417-446 on words made for every branch, the CRC against the oracle's, the whole against the oracle's decode of a frame"""
    for md in (0, 1, 0x123456789abcd, (1 << 55) - 1):
        assert V.crc16((md << 9) & 0xffffffffffffffff) == O.lib().orc_crc16_u64(0xA8F4, C.c_uint64((md << 9) & 0xffffffffffffffff))
    call = int(O.lib().orc_base37_encode(b"HEADER"))

    def hard(mode, cs, flip=None):
        c = V.encode(V.header_word(mode, cs))
        if flip is not None:
            c = V.encode(c[:V.K] ^ (np.arange(V.K) == flip))
        return np.packbits(np.concatenate([c, [0]]).astype(np.uint8))

    assert V.header_fields(hard(6, call)) == (0, 6, call)
    assert V.header_fields(hard(13, 1)) == (0, 13, 1)
    assert V.header_fields(hard(6, call), unique=0) == (2, 0, 0)
    assert V.header_fields(hard(6, call, flip=3)) == (3, 0, 0)
    assert V.header_fields(hard(6, call, flip=60)) == (3, 0, 0)
    assert V.header_fields(hard(5, call))[:2] == (4, 5) and V.header_fields(hard(14, call))[:2] == (4, 14)
    assert V.header_fields(hard(6, 0)) == (5, 6, 0)
    assert V.header_fields(hard(7, 129961739795077)) == (5, 7, 129961739795077)
    assert V.header_fields(hard(7, 129961739795076)) == (0, 7, 129961739795076)
    _, pcm, _ = V.clean_frame(0)
    _, res, tb = O.decode(pcm, taps=True)
    h, u = O.osd(tb.hdr_soft)
    assert V.header_fields(h, u) == (res.status, res.oper_mode, res.call_sign) == (0, 6, call)
    assert V.route(tb.hdr_soft) == 1                                 # a clean header leaves by the syndrome certificate


def test_header_levels_rederived():
    """the three header levels from the oracle alone, 48 frames each (level_counts also asserts that the payload decodes in every
    frame whose header does and is zeros otherwise: the noise does not reach it)"""
    got = {db: V.level_counts(db) for db in V.HDR_ORACLE}
    assert got == V.HDR_ORACLE
    n = V.HDR_FRAMES

    def search_ok(c):
        return c[1] >= 46 and c[2] == 0

    assert search_ok(got[V.HDR_SEARCH_DB]) and not search_ok(got[V.HDR_SEARCH_DB + 1.0])          # the noisiest such level
    assert all(search_ok(got[db]) for db in got if db < V.HDR_SEARCH_DB)
    assert got[V.HDR_SEARCH_DB][4] == n                                                           # every frame searched in full
    assert V.HDR_EDGE_DB == V.HDR_SEARCH_DB + 1.0 and n // 4 <= got[V.HDR_EDGE_DB][1] <= 3 * n // 4
    assert min(got[V.HDR_MIXED_DB][3:5]) >= n // 4
    assert got[V.HDR_MIXED_DB - 1.0][4] == 0 and got[V.HDR_MIXED_DB + 1.0][3] < n // 4            # the only such level


def test_header_levels_carry_to_mono_and_other_rates():
    """the 16-frame sets of test_gpu_header.py (mono, 48 kHz) re-derived: the recorded counts exactly; the search level is the noisiest
    1 dB step with at least 14 of 16 headers decoded, none on route 1 and every frame searched in full; at the edge level the header
    decodes in 25 - 75 % of the frames, so that at least a quarter ends with a header status; the payload follows the header everywhere
    (level_counts asserts it - for mono too: the tails of the front end's filter stay inside the guard intervals)"""
    for (rate, ch), levels in V.HDR_SMALL.items():
        got = {name: V.level_counts(db, 16, rate=rate, channels=ch) for name, (db, _) in levels.items()}
        assert got == {name: c for name, (_, c) in levels.items()}, (rate, ch, got)
        assert levels["above_search"][0] == levels["search"][0] + 1.0
        assert got["search"][1] >= 14 and got["search"][2] == 0 and got["search"][4] == 16 and got["above_search"][1] < 14
        assert 4 <= got["edge"][1] <= 12 and got["edge"][2] == 0 and got["edge"][4] == 16
