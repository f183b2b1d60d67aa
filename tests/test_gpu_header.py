"""The header's ordered-statistics decoder (k_header.hip: k_header and k_osd_only) on every route, at every order, on ties and in
noise.  The inputs and the numpy restatement that predicts a word's route are tests/osd_vectors.py; their premises
are checked on the oracle alone by tests/test_osd_vectors_cpu.py."""
import warnings

import numpy as np
import pytest

import bank_inputs as B
import oracle_lib as O
import osd_vectors as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=64, keep_raw_cons=True)
    yield r
    r.close()


def _receiver(rate, **kw):
    import modem_amd
    return modem_amd.Receiver(device=0, sample_rate=rate, **kw)


def test_osd_constructed_orders(rx):
    """every constructed order-k vector (k = 0 .. 4: sliding runs over all 71 ranks, the ends of the pair and triple tables and of the
    d loop, random and marginal patterns, plateaus, -128, up to nine column swaps): the kernel returns the constructed codeword and
    calls it unique.  By construction that codeword is the strict optimum of the whole code and sits at order k and no lower, so a
    missing candidate, a wrong table entry or a certificate that passes on the best of orders 0 - 2 all show as a wrong word"""
    vecs = V.constructed()
    hard, uniq = rx.osd(np.stack([v.soft for v in vecs]))
    bits = V.bits_of(hard)
    bad = [v for v, b, u in zip(vecs, bits, uniq) if int(u) != 1 or not (b == v.c).all()]
    assert not bad, "%d of %d: %s" % (len(bad), len(vecs), bad[:12])


def test_osd_ties(rx):
    """256 words of +-1 (half of them with erasures): best and runner-up tie at non-zero metrics in about a third of them.  The
    uniqueness flag equals the oracle's for every word, the codeword wherever the oracle calls it unique (all of them go through the
    full search: the runner-up has to survive the per-thread tracks and their reduction across the waves)"""
    for fam in V.ties():
        hard, uniq = rx.osd(fam)
        obits, ouniq = V.oracle_osd(fam)
        assert 0.25 <= ouniq.mean() <= 0.85
        assert (uniq == ouniq).all(), np.flatnonzero(uniq != ouniq)
        same = (V.bits_of(hard) == obits).all(axis=1)
        assert same[ouniq == 1].all(), np.flatnonzero(~same & (ouniq == 1))


# ---------------------------------------------------------------- frames with noise on the header symbol only
N_SOFT = 16           # frames per case whose tap is compared with the oracle's own soft values
ERASURE_CAP = 2       # soft values further than 1 apart, one side exactly 0 (an erasure tie of demod_or_erase): whole module


@pytest.fixture(scope="module")
def erasure_ties():
    """the erasure ties of all cases of one run of this module (each is reported as a warning when it is met)"""
    return []


def _header_case(r, db, n, rate, channels, ties, want_routes=None, min_failed=0):
    pays, pcms = V.header_frames(V.equivalent_db(db, rate, channels), n, rate, channels)
    out, res = r.decode(pcms)
    assert r.last_chunk_first_frame() == 0
    taps = np.stack([r.tap("HDR_SOFT", i) for i in range(n)])
    # the frame's verdict is the oracle's OSD and decode.cc:417-446 on the GPU's own soft values
    obits, ouniq = V.oracle_osd(taps)
    ohard = np.packbits(np.concatenate([obits, np.zeros((n, 1), np.uint8)], axis=1), axis=1)
    for i in range(n):
        st, mode, call = V.header_fields(ohard[i], ouniq[i])
        g = res[i]
        assert int(g["status"]) == st, (i, int(g["status"]), st)
        assert int(g["oper_mode"]) == mode, (i, st)
        if call is not None:
            assert int(g["call_sign"]) == call, (i, st)
        assert (out[i] == pays[i]).all() if st == 0 else not out[i].any(), (i, st)   # the noise does not reach the payload
    # k_osd_only is the same function on these natural inputs (plateaus at +-127, erasure zeros, -128)
    hard, uniq = r.osd(taps)
    assert (uniq == ouniq).all(), np.flatnonzero(uniq != ouniq)
    same = (V.bits_of(hard) == obits).all(axis=1)
    assert same[ouniq == 1].all(), np.flatnonzero(~same & (ouniq == 1))
    # which routes these frames took
    routes = [V.route(t) for t in taps]
    if want_routes is not None:
        forbidden, floor = want_routes
        for q in forbidden:
            assert routes.count(q) == 0, (q, routes)
        for q, least in floor.items():
            assert routes.count(q) >= least, (q, least, routes)
    assert int((res["status"] != 0).sum()) >= min_failed, res["status"]
    # the soft values themselves against the oracle's
    for i, (_, _, osoft) in enumerate(V.oracle_header(pcms[:N_SOFT], rate=rate)):
        d = np.abs(taps[i].astype(np.int32) - osoft.astype(np.int32))
        for p in np.flatnonzero(d > 1):
            assert taps[i][p] == 0 or osoft[p] == 0, (i, p, int(taps[i][p]), int(osoft[p]))
            ties.append((rate, channels, db, i, int(p), int(taps[i][p]), int(osoft[p])))
            warnings.warn("erasure tie (rate, channels, level, frame, position, HDR_SOFT, oracle): %s" % (ties[-1],))
    assert len(ties) <= ERASURE_CAP, ties
    return routes


@pytest.fixture(scope="module")
def rx48():
    r = _receiver(48000, chunk_frames=16, keep_raw_cons=True)
    yield r
    r.close()


CASES = [("search", 8000, 2, 64), ("mixed", 8000, 2, 64), ("edge", 8000, 2, 64),
         ("search", 8000, 1, 16), ("edge", 8000, 1, 16), ("search", 48000, 2, 16), ("edge", 48000, 2, 16)]


@pytest.mark.parametrize("level,rate,channels,n", CASES, ids=["%s-%d-%dch" % c[:3] for c in CASES])
def test_header_in_noise(rx, rx48, erasure_ties, level, rate, channels, n):
    """Frames whose header symbol alone is noisy, through the batch entry; the verdict of every frame against the oracle's search and
    decode.cc:417-446 on the GPU's own HDR_SOFT tap (_header_case).
      search  HDR_SEARCH_DB: most headers decode, none by the syndrome certificate, every frame goes through the full order-4 search
              inside k_header itself
      mixed   HDR_MIXED_DB: routes 2 and 3 side by side in one launch (route 2 does not occur at the search level)
      edge    HDR_EDGE_DB, the header's own waterfall: at least a quarter of the frames end with a header status (2: the search's
              best is not unique, 3: it is, and fails the CRC-16)
    64 frames per level at 8 kHz, 2 channels; 16 at the search and edge levels through k_header<8000, true> (mono: the symbol's analytic
    signal is made inside the kernel) and through k_header<48000, false>, at the levels osd_vectors.HDR_SMALL records for them.  In
    every case no frame is on route 1, routes 2 and 3 hold at least half the share the oracle's derivation found, and at the edge at
    least a quarter of the frames fail"""
    if n == 64:
        db = dict(search=V.HDR_SEARCH_DB, mixed=V.HDR_MIXED_DB, edge=V.HDR_EDGE_DB)[level]
        counts = V.HDR_ORACLE[db]
    else:
        db, counts = V.HDR_SMALL[(rate, channels)][level]
    assert counts[0] - counts[1] >= counts[0] // 4 or level != "edge"  # (the oracle's own frames meet the quarter)
    floor = {q: (counts[1 + q] * n) // (2 * counts[0]) for q in (2, 3)}
    _header_case(rx48 if rate == 48000 else rx, db, n, rate, channels, erasure_ties, want_routes=((1,), floor),
                 min_failed=n // 4 if level == "edge" else 0)


def test_header_in_noise_through_streams_and_bank():
    """one recording of six frames at HDR_EDGE_DB between stretches of silence: record k of decode_stream, of decode_streams (a clean
    recording beside it) and of a bank fed in blocks of 8000 is what the batch entry gives on the same recording with skip = k - the
    SourceBatch and WindowBatch instantiations of k_header on the search route, failed headers included"""
    rng = np.random.default_rng(6)
    parts, pays = [], []
    for k in range(6):
        pay, pcm = V.noisy_header_frame(k, V.HDR_EDGE_DB, 1000 * V.HDR_SEED + 100 + k)
        parts += [np.zeros((int(rng.integers(1000, 5000)) | 1, 2), np.int16), pcm]
        pays.append(pay)
    rec = np.concatenate(parts)
    clean = np.array(V.clean_frame(1)[1])
    rb = _receiver(8000, chunk_frames=8, max_samples=len(rec))
    try:
        bout, bres = rb.decode(np.stack([rec] * 6), skip=np.arange(6))
    finally:
        rb.close()
    ok = bres["status"] == 0
    assert 0 < ok.sum() < 6 and set(bres["status"].tolist()) <= {0, 2, 3}, bres["status"]
    for k in range(6):
        assert (bout[k] == pays[k]).all() if ok[k] else not bout[k].any(), k

    def same(out, res, what):
        assert len(res) == 6, (what, len(res))
        for k in range(6):
            for f in ("status", "sc_start"):
                assert res[k][f] == bres[k][f], (what, k, f, res[k][f], bres[k][f])
            # Mode and call sign: the batch entry's where the header decoded.  Behind a failed header the batch entry with skip = k
            # still shows what an EARLIER attempt of the same decode left there (decode.cc's oper_mode survives the `continue` of
            # :418-442; the oracle's skip-k decode does the same), while a record of a stream is a decode of its own: its fields
            # are the untouched zeros that header_fields() gives for statuses 2 and 3
            want = (bres[k]["oper_mode"], bres[k]["call_sign"]) if ok[k] else (0, 0)
            assert (int(res[k]["oper_mode"]), int(res[k]["call_sign"])) == (int(want[0]), int(want[1])), (what, k, res[k], bres[k])
            assert (out[k] == bout[k]).all(), (what, k)

    r = _receiver(8000, chunk_frames=16)
    try:
        out, res, npre = r.decode_stream(rec)
        assert npre == 6
        same(out, res, "decode_stream")
        (out, res, npre), (cout, cres, cpre) = r.decode_streams([rec, clean])
        assert npre == 6 and cpre == 1 and int(cres[0]["status"]) == 0 and (cout[0] == V.clean_frame(1)[0]).all()
        same(out, res, "decode_streams")
        per, _, _ = B.run_bank(r, [rec, clean], B.block_rounds([len(rec), len(clean)], 8000))
        same(per[0][0], per[0][1], "bank")
        assert len(per[1][1]) == 1 and int(per[1][1][0]["status"]) == 0 and (per[1][0][0] == V.clean_frame(1)[0]).all()
    finally:
        r.close()


@pytest.mark.parametrize("rate", [16000, 44100, 48000])
def test_header_soft_values_at_every_rate(rate):
    """HDR_SOFT against the oracle's soft values, within 1 (the int8 rounding of an fp32 value), on a clean and a -28 dB frame,
    2-channel and mono, at the three rates where it was not compared before"""
    r = _receiver(rate, chunk_frames=4, keep_raw_cons=True)
    try:
        pay = O.payload_for(5100 + rate // 1000)
        clean2 = O.encode_pcm(pay, channels=2, freq_off=1500, call_sign="SOFT%d" % (rate // 1000), rate=rate)
        noisy2 = O.impair(clean2, noise_db=-28, seed=rate, frame=1, rate=rate)
        for channels in (2, 1):
            pcms = np.stack([clean2, noisy2])[:, :, :channels]
            out, res = r.decode(pcms)
            assert (res["status"] == 0).all() and (out == pay).all()
            for i in range(2):
                _, ores, tb = O.decode(pcms[i], taps=True, rate=rate)
                assert ores.status == 0
                d = np.abs(r.tap("HDR_SOFT", i).astype(np.int32) - tb.hdr_soft.astype(np.int32))
                assert d.max() <= 1, (rate, channels, i, int(d.max()), np.flatnonzero(d > 1))
    finally:
        r.close()
