"""The live feed bank (ofdmrx_bank_*): many live channels pushed and decoded in one call.  The truth of every test is
never another run of the bank: ofdmrx_decode_stream on the same handle configuration for 2-channel input; for mono input the answers
the single-window feed gave for the same push lengths, recorded from the last commit that had one (tests/golden/feed_mono_parent.json,
feed_fixture.py).  ofdmrx_feed_* is a bank of one channel since, so the mono tests' comparison with it says that a channel among
neighbours equals the channel alone."""
import ctypes as C

import numpy as np
import pytest

import bank_inputs as B
import feed_fixture as F
import oracle_lib as O

pytestmark = pytest.mark.gpu

REL = 1e-5
TILE = 4096
E_ARG = -1


def _rx(rate=8000, **kw):
    import modem_amd
    return modem_amd.Receiver(device=0, chunk_frames=16, sample_rate=rate, **kw)


@pytest.fixture(scope="module")
def rx():
    r = _rx()
    yield r
    r.close()


@pytest.fixture(scope="module")
def staggered_truth(rx):
    """decode_stream of every staggered channel, computed once"""
    truth = []
    for ch in B.staggered():
        out, res, npre = rx.decode_stream(ch)
        assert npre == 3 and (res["status"] == 0).all()
        truth.append((out, res))
    return truth


def _flips_ok(gpu, one):
    return abs(int(gpu) - int(one)) <= (2 if int(one) > 0 else 0)


def test_staggered_alignments(rx, staggered_truth):
    chans = B.staggered()
    per, calls, ops = B.run_bank(rx, chans, B.block_rounds([len(c) for c in chans], 8000))
    for c, want in enumerate(staggered_truth):
        B.same(per[c][:2], want)
        assert per[c][2].tolist() == [0, 1, 2], c
        assert [int(s) - B.LEADS[c] for s in per[c][1]["sc_start"]] == [int(s) for s in staggered_truth[0][1]["sc_start"]]
    B.call_order_ok(calls)
    assert any(len(set(rc.tolist())) > 1 for rc, _ in calls)     # some call returned records of several channels


def test_ragged_pushes(rx, staggered_truth):
    chans = B.staggered()
    lens = [len(c) for c in chans]
    rng = np.random.default_rng(3)
    cols = []
    for c, n in enumerate(lens):
        if c == 1:                                               # everything in its first push
            cols.append([n])
            continue
        sizes, left = [], n
        while left:
            k = min(left, int(rng.integers(1, 20001)))
            sizes.append(k)
            left -= k
        cols.append(sizes)
    n_rounds = max(len(s) for s in cols)
    cols[4] = [0] * n_rounds + cols[4]                           # nothing until the others have finished
    # a zero-length share for channel 2 in a round in which channels 0 and 3 both complete tiles
    tiles = lambda c, r: sum(cols[c][:r]) // TILE
    r0 = next(r for r in range(1, 15) if all(tiles(c, r + 1) > tiles(c, r) for c in (0, 3)))
    cols[2].insert(r0, 0)
    n_rounds = max(len(s) for s in cols)
    rounds = [[s[r] if r < len(s) else 0 for s in cols] for r in range(n_rounds)]
    assert rounds[r0][2] == 0 and rounds[r0][0] > 0 and rounds[r0][3] > 0
    per, calls, ops = B.run_bank(rx, chans, rounds)
    for c, want in enumerate(staggered_truth):
        B.same(per[c][:2], want)
        assert per[c][2].tolist() == [0, 1, 2], c
    B.call_order_ok(calls)


def test_channel_independence(rx, staggered_truth):
    chans = B.staggered()
    me = chans[2]
    rounds1 = B.block_rounds([len(me)], 8000)
    alone, _, ops1 = B.run_bank(rx, [me], rounds1)
    six, _, ops6 = B.run_bank(rx, chans, B.block_rounds([len(c) for c in chans], 8000))
    noisy = [me if c == 2 else B.noise(len(me), 40 + c) for c in range(6)]
    among, _, _ = B.run_bank(rx, noisy, B.block_rounds([len(c) for c in noisy], 8000))
    B.same(alone[0][:2], staggered_truth[2])
    for got in (six[2], among[2]):
        B.same(got[:2], alone[0][:2])
        assert got[2].tolist() == alone[0][2].tolist()


def test_mixed_modes_and_failures(rx):
    a, m = B.mixed(2), B.mixed(2, mirror=True)
    truth = []
    for ch in (a, m):
        out, res, npre = rx.decode_stream(ch)
        assert npre == len(res) >= 9
        truth.append((out, res))
    rounds = B.block_rounds([len(a), len(m)], 8000)
    per, calls, _ = B.run_bank(rx, [a, m], rounds)
    for c in range(2):
        B.same(per[c][:2], truth[c])
        assert per[c][2].tolist() == list(range(len(truth[c][1])))
        st = truth[c][1]["status"]
        assert ((st != 0) & (st != 6)).sum() >= 1                # a record with a failed header appears
    B.call_order_ok(calls)
    # the cut-off frame of either channel leaves only with the end
    rc, ri = calls[-1]
    for c in range(2):
        assert ri[rc == c].tolist()[-1:] == [len(truth[c][1]) - 1]
        assert all(len(truth[c][1]) - 1 not in ri_[rc_ == c].tolist() for rc_, ri_ in calls[:-1])


def _mono_compare(rx, chans, blocks, fixture, rate=8000, relation=True):
    lens = [len(c) for c in chans]
    rounds = B.block_rounds(lens, blocks)
    per, calls, _ = B.run_bank(rx, chans, rounds)
    for c, ch in enumerate(chans):
        pushes = [r[c] for r in rounds]
        F.check(fixture % c, ch, pushes, per[c][:2])             # the recorded single-window feed, byte for byte
        want = B.run_feed(rx, ch, pushes)                        # the channel alone (a bank of one)
        F.check(fixture % c, ch, pushes, want)
        B.same(per[c][:2], want)
        assert per[c][2].tolist() == list(range(len(want[1])))
        if relation:                                             # the feed's documented relation to the one-call decode
            out, res, npre = rx.decode_stream(ch)
            fo, fr = per[c][:2]
            assert len(fr) == npre == len(res) and fo.tobytes() == out.tobytes()
            for name in ("status", "sc_start", "symbol_pos", "n_sync_rejects", "oper_mode", "call_sign", "best_lane"):
                assert (fr[name] == res[name]).all(), name
            for name in ("cfo_rad", "cfo_fine", "sfo_slope", "esn0_db_last"):
                assert np.abs(fr[name].astype(np.float64) - res[name].astype(np.float64)).max() <= REL, name
            assert all(_flips_ok(x, y) for x, y in zip(fr["bit_flips"], res["bit_flips"]))
    B.call_order_ok(calls)
    return per


def test_mono(rx):
    real = B.mixed(1).reshape(-1)
    chans = [np.concatenate([np.zeros(lead, np.int16), real]) for lead in (0, 1, 4097)]
    per = _mono_compare(rx, chans, [8000, 4095, 7937], "bank_mono_c%d")
    assert all(len(p[1]) >= 9 for p in per)


def test_ends(rx):
    import modem_amd.ofdmrx as M
    # every channel stops inside its last frame: channel 0 first, by `ends` in the middle of the call sequence, the others by end()
    chans = [c[:lead + (192240 if i == 0 else 215000)] for i, (c, lead) in enumerate(zip(B.staggered()[:3], B.LEADS))]
    want = [rx.decode_stream(c) for c in chans]
    assert all(w[2] == 3 and int(w[1]["status"][2]) != 0 for w in want)
    rounds = B.block_rounds([len(c) for c in chans], 8000)
    r_end = (len(chans[0]) + 7999) // 8000 - 1                   # the round that brings channel 0's last samples
    assert rounds[r_end][0] > 0 and r_end + 2 < len(rounds)
    got = [[] for _ in chans]
    at = [0] * 3

    def take(ret):
        for c in range(3):
            got[c].append((ret[0][ret[2] == c], ret[1][ret[2] == c]))

    with rx.bank(3, 2) as b:
        for r, ln in enumerate(rounds):
            blocks = [chans[c][at[c]:at[c] + n] for c, n in enumerate(ln)]
            ret = b.push(blocks, ends=[True, False, False] if r == r_end else None)
            at = [x + n for x, n in zip(at, ln)]
            take(ret)
            rc, ri = ret[2], ret[3]
            if r == r_end:                                       # its pending and cut-off frames arrive in that call
                assert ri[rc == 0].tolist()[-1] == 2 and sum(len(g[1]) for g in got[0]) == 3
            if r > r_end:
                assert (rc != 0).all()
            if r == r_end + 1:                                   # samples for an ended channel
                with pytest.raises(M.OfdmRxError):
                    b.push([chans[0][:10], None, None])
        assert sum(len(g[1]) for g in got[1]) == 2 and sum(len(g[1]) for g in got[2]) == 2
        ret = b.end(max_records=0)                               # the neighbours' cut-off frames: staged
        assert len(ret[1]) == 0 and b.n_left == 2 and b.open
        ret = b.end(max_records=1)
        assert len(ret[1]) == 1 and b.n_left == 1 and b.open
        take(ret)
        ret = b.end(max_records=1)
        assert len(ret[1]) == 1 and b.n_left == 0 and not b.open
        take(ret)
    for c in range(3):
        B.same(B.cat(got[c]), want[c][:2])


def test_max_records_and_draining(rx):
    import modem_amd.ofdmrx as M
    L, h = rx._lib, rx._h
    pay = O.payload_for(500, count=2)
    pcm = O.encode_pcm(pay, channels=2)
    chans = [pcm, np.concatenate([np.zeros((4097, 2), np.int16), pcm])]
    want = [rx.decode_stream(c) for c in chans]
    assert all(w[2] == 2 for w in want)
    n = max(len(c) for c in chans)
    buf = np.zeros((2, n, 2), np.int16)
    for c, ch in enumerate(chans):
        buf[c, :len(ch)] = ch
    lens = np.array([len(c) for c in chans], np.uintp)
    zero = np.zeros(2, np.uintp)
    out = np.full((4, 5380), 0xA5, np.uint8)
    res = np.zeros(4, M.RESULT_DTYPE)
    rc = np.full(4, 77, np.int32)
    ri = np.full(4, 77, np.int64)
    nrec, nleft = C.c_size_t(9), C.c_size_t(9)
    a = (M._ptr(out), M._ptr(res), M._ptr(rc), M._ptr(ri), C.byref(nrec), C.byref(nleft))
    got = []

    def untouched(k):
        assert (out[k:] == 0xA5).all() and (rc[k:] == 77).all() and (ri[k:] == 77).all()
        assert res[k:].tobytes() == keep[k:].tobytes()

    res["status"] = 77
    keep = res.copy()

    def took(k):
        for i in range(k):
            got.append((out[i].copy(), res[i].copy(), int(rc[i]), int(ri[i])))
            out[i] = 0xA5
            res[i] = keep[i]
            rc[i] = ri[i] = 77

    assert L.ofdmrx_bank_begin(h, 2, 0, 2) == 0
    try:
        assert L.ofdmrx_bank_push(h, M._ptr(buf), buf.strides[0], M._ptr(lens), None, 1, *a) == 0
        ready = nrec.value + nleft.value
        assert nrec.value == 1 and ready >= 3                    # (the last frames end before the trailing silence does)
        untouched(1)
        took(1)
        assert L.ofdmrx_bank_push(h, None, 0, M._ptr(zero), None, 0, None, None, None, None, C.byref(nrec), C.byref(nleft)) == 0
        assert nrec.value == 0 and nleft.value == ready - 1
        assert L.ofdmrx_bank_push(h, None, 0, M._ptr(zero), None, 2, *a) == 0
        assert nrec.value == 2 and nleft.value == ready - 3
        untouched(2)
        took(2)
        assert L.ofdmrx_bank_end(h, 0, None, None, None, None, C.byref(nrec), C.byref(nleft)) == 0
        assert nrec.value == 0 and nleft.value == 1
        assert L.ofdmrx_bank_resident_samples(h, 0) >= 0         # still open: one record is left
        assert L.ofdmrx_bank_end(h, 4, *a) == 0
        assert nrec.value == 1 and nleft.value == 0
        untouched(1)
        took(1)
        assert L.ofdmrx_bank_resident_samples(h, 0) == E_ARG     # closed
    finally:
        while L.ofdmrx_bank_resident_samples(h, 0) >= 0:
            L.ofdmrx_bank_end(h, 4, *a)
    assert [(g[2], g[3]) for g in got] == [(0, 0), (0, 1), (1, 0), (1, 1)]   # first in, first out: by channel, then by preamble
    for c in range(2):
        mine = [g for g in got if g[2] == c]
        B.same((np.stack([g[0] for g in mine]), np.stack([g[1] for g in mine])), want[c][:2])


def test_rate_48k_two_channel():
    r = _rx(48000)
    try:
        pcm = O.impair(O.encode_pcm(O.payload_for(60), channels=2, rate=48000), noise_db=-30, seed=2, frame=0, rate=48000)
        chans = [pcm, np.concatenate([np.zeros((4097, 2), np.int16), pcm])]
        per, calls, _ = B.run_bank(r, chans, B.block_rounds([len(c) for c in chans], 48000))
        for c, ch in enumerate(chans):
            out, res, npre = r.decode_stream(ch)
            assert npre == 1 and (out[0] == O.payload_for(60)).all()
            B.same(per[c][:2], (out, res))
    finally:
        r.close()


def test_rate_44k_mono():
    r = _rx(44100)
    try:
        pcm = O.impair(O.encode_pcm(O.payload_for(61), channels=2, rate=44100), noise_db=-30, seed=2, frame=0, rate=44100)
        mono = np.ascontiguousarray(pcm[:, 0])
        chans = [mono, np.concatenate([np.zeros(4097, np.int16), mono])]
        per = _mono_compare(r, chans, 44100, "bank_44k_mono_c%d", rate=44100)
        assert all(len(p[1]) == 1 and (p[0][0] == O.payload_for(61)).all() for p in per)
    finally:
        r.close()


@pytest.mark.parametrize("fmt", ["u8", "f32"])
def test_formats(rx, fmt):
    pay = O.payload_for(70)
    pcm = O.encode_pcm(pay, channels=2, bits=8 if fmt == "u8" else 16)
    if fmt == "f32":
        pcm = O.pcm_to_cf(pcm)
    zero = np.full((4097, 2), 128, np.uint8) if fmt == "u8" else np.zeros((4097, 2), pcm.dtype)
    chans = [pcm, np.concatenate([zero, pcm])]
    per, calls, _ = B.run_bank(rx, chans, B.block_rounds([len(c) for c in chans], 8000))
    for c, ch in enumerate(chans):
        out, res, npre = rx.decode_stream(ch)
        assert npre == 1 and (out[0] == pay).all()
        B.same(per[c][:2], (out, res))


def test_positions_past_2_31(rx):
    """two mono u8 channels: channel 0 behind more than 2^31 samples of silence, channel 1 behind one block of 4096 * 31; then the same
    frame on both.  Silence leaves the DC blocker's state at exactly 0 and the lead-ins differ by a multiple of the scan's tile and of
    the front end's stretch, so the two records are the same bytes but for sc_start."""
    unit = 4096 * 31
    block = np.full(unit * 512, 128, np.uint8)
    frame = O.encode_pcm(O.payload_for(600), channels=1, bits=8).reshape(-1)
    got = [[], []]
    bound = rx._lib.ofdmrx_frame_samples(8000, 13) + 6 * 1440 + 3 * TILE + len(block)
    with rx.bank(2, 1, np.uint8) as b:
        for i in range(34):
            ret = b.push([block, block[:unit] if i == 0 else None])
            assert len(ret[1]) == 0
            assert b.resident_samples(0) <= bound, (i, b.resident_samples(0))
        for ret in (b.push([frame, frame]), b.end()):
            for c in range(2):
                got[c].append((ret[0][ret[2] == c], ret[1][ret[2] == c]))
    (fo, fr), (no, nr) = B.cat(got[0]), B.cat(got[1])
    far, near = 34 * len(block), unit
    assert far > 2 ** 31 and len(nr) == len(fr) == 1 and int(nr["status"][0]) == 0
    assert fo.tobytes() == no.tobytes() and (fo[0] == O.payload_for(600)).all()
    assert int(fr["sc_start"][0]) - int(nr["sc_start"][0]) == far - near and int(fr["sc_start"][0]) > 2 ** 31
    fr = fr.copy()
    fr["sc_start"] = nr["sc_start"]
    assert fr.tobytes() == nr.tobytes()


def test_bounded_window_per_channel(rx):
    rng = np.random.default_rng(21)
    n, block = 1_000_000, 65536
    a = rng.normal(0, 300, size=(n, 2)).astype(np.int16)
    for i, at in enumerate((200_000, 600_000)):
        fr = O.encode_pcm(O.payload_for(400 + i), channels=2)
        a[at:at + len(fr)] = np.clip(a[at:at + len(fr)].astype(np.int32) + fr, -32768, 32767).astype(np.int16)
    chans = [a, B.noise(n, 22)]
    bound = rx._lib.ofdmrx_frame_samples(8000, 13) + 6 * 1440 + 3 * TILE + block
    got = [[], []]
    with rx.bank(2, 2) as b:
        for s in range(0, n, block):
            ret = b.push([c[s:s + block] for c in chans])
            for c in range(2):
                got[c].append((ret[0][ret[2] == c], ret[1][ret[2] == c]))
                assert b.resident_samples(c) <= bound, (s, c, b.resident_samples(c), bound)
        ret = b.end()
        for c in range(2):
            got[c].append((ret[0][ret[2] == c], ret[1][ret[2] == c]))
    for c in range(2):
        out, res, npre = rx.decode_stream(chans[c])
        if c == 0:
            assert (res["status"] == 0).sum() == 2
        B.same(B.cat(got[c]), (out, res))


def test_stage_ops_do_not_follow_the_channels(rx):
    """the launches, copies and synchronisations of a push's own stages: the same for 2 and for 16 channels of the same stream (16: the
    pending preambles of all channels still fit one chunk of the header stage, whose loop over chunks is the documented exception)"""
    me = B.staggered()[0][:60000]
    counts = []
    for n_ch in (2, 16):
        _, _, ops = B.run_bank(rx, [me] * n_ch, B.block_rounds([len(me)] * n_ch, 20000), end=False)
        counts.append(ops)
    assert counts[0] == counts[1] and all(0 < k <= 40 for k in counts[0]), counts


def test_esn0_rows(rx):
    chans = B.staggered()[:2]
    want = [rx.decode_stream(c, esn0_rows=True) for c in chans]
    rows = [[], []]
    with rx.bank(2, 2, esn0_rows=True) as b:
        rets = [b.push([c[s:s + 50000] for c in chans]) for s in range(0, max(len(c) for c in chans), 50000)]
        rets.append(b.end())
    for ret in rets:
        for c in range(2):
            rows[c].append(ret[4][ret[2] == c])
    for c in range(2):
        got = np.concatenate(rows[c])
        assert got.shape == want[c][3].shape == (3, 126) and got.tobytes() == want[c][3].tobytes()


def test_lifecycle(rx, staggered_truth):
    import modem_amd.ofdmrx as M
    L, h = rx._lib, rx._h
    pcm = B.staggered()[0]
    out = np.zeros((4, 5380), np.uint8)
    res = np.zeros(4, M.RESULT_DTYPE)
    rc, ri = np.zeros(4, np.int32), np.zeros(4, np.int64)
    nrec, nleft, npre = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    a = (M._ptr(out), M._ptr(res), M._ptr(rc), M._ptr(ri), C.byref(nrec), C.byref(nleft))
    buf = np.ascontiguousarray(np.stack([pcm[:1000], pcm[:1000]]))
    lens = np.array([1000, 1000], np.uintp)
    push = lambda s, stride, n, ends, cap, *o: L.ofdmrx_bank_push(h, s, stride, n, ends, cap, *o)
    # without a bank
    assert push(M._ptr(buf), 4000, M._ptr(lens), None, 4, *a) == E_ARG
    assert L.ofdmrx_bank_end(h, 4, *a) == E_ARG
    assert L.ofdmrx_bank_resident_samples(h, 0) == E_ARG and L.ofdmrx_bank_preambles(h, 0) == E_ARG
    for bad in ((0, 0, 2), (65536, 0, 2), (2, 3, 2), (2, -1, 2), (2, 0, 3), (2, 0, 0)):
        assert L.ofdmrx_bank_begin(h, *bad) == E_ARG, bad
    assert L.ofdmrx_bank_begin(h, 2, 0, 2) == 0
    try:
        assert L.ofdmrx_bank_begin(h, 2, 0, 2) == E_ARG          # one bank per handle
        assert L.ofdmrx_feed_begin(h, 0, 2) == E_ARG             # ... and no feed beside it; the feed entries refuse the bank
        fa = (M._ptr(out), M._ptr(res), C.byref(nrec), C.byref(nleft))
        assert L.ofdmrx_feed_push(h, None, 0, 4, *fa) == E_ARG and L.ofdmrx_feed_end(h, 4, *fa) == E_ARG
        assert L.ofdmrx_feed_lag(h) == E_ARG and L.ofdmrx_feed_resident_samples(h) == E_ARG
        assert L.ofdmrx_bank_resident_samples(h, 0) == 0         # (still open)
        assert push(None, 4000, M._ptr(lens), None, 4, *a) == E_ARG
        assert push(M._ptr(buf), 4000, None, None, 4, *a) == E_ARG
        for k in range(4):                                       # any of the four arrays
            o = list(a)
            o[k] = None
            assert push(M._ptr(buf), 4000, M._ptr(lens), None, 4, *o) == E_ARG
            assert L.ofdmrx_bank_end(h, 4, *o) == E_ARG
        assert push(M._ptr(buf), 4000, M._ptr(lens), None, 4, *a[:4], None, C.byref(nleft)) == E_ARG
        assert push(M._ptr(buf), 4000, M._ptr(lens), None, 4, *a[:4], C.byref(nrec), None) == E_ARG
        assert push(M._ptr(buf), 3998, M._ptr(lens), None, 4, *a) == E_ARG      # the stride: not a multiple of the sample frame
        assert push(M._ptr(buf), 3996, M._ptr(lens), None, 4, *a) == E_ARG      # ... shorter than the longest share
        assert push(C.c_void_p(buf.ctypes.data + 2), 4000, M._ptr(lens), None, 4, *a) == E_ARG   # not on an I/Q pair
        big = np.array([(1 << 26) + 1, 0], np.uintp)
        assert push(M._ptr(buf), 1 << 30, M._ptr(big), None, 4, *a) == E_ARG
        assert L.ofdmrx_bank_resident_samples(h, 2) == E_ARG and L.ofdmrx_bank_preambles(h, 2) == E_ARG
        # the other decode entries refuse a handle with an open bank
        assert L.ofdmrx_decode_stream(h, M._ptr(pcm), 0, 2, len(pcm), 4, M._ptr(out), M._ptr(res), C.byref(npre)) == E_ARG
        assert L.ofdmrx_decode_stream_device(h, M._ptr(pcm), 0, 2, len(pcm), 4, M._ptr(out), M._ptr(res), C.byref(npre)) == E_ARG
        assert L.ofdmrx_decode_batch(h, M._ptr(pcm), 0, 2, 95200, 95200 * 4, 1, None, M._ptr(out), M._ptr(res)) == E_ARG
        assert L.ofdmrx_decode_batch_device(h, M._ptr(pcm), 0, 2, 95200, 95200 * 4, 1, None, M._ptr(out), M._ptr(res)) == E_ARG
        n1 = np.array([len(pcm)], np.uintp)
        assert L.ofdmrx_decode_streams(h, M._ptr(pcm), 0, 2, 1, len(pcm) * 4, M._ptr(n1), 4, 4, M._ptr(out), M._ptr(res), M._ptr(n1.copy()),
                                       M._ptr(np.zeros(2, np.uintp))) == E_ARG
        zero = np.zeros(2, np.uintp)
        assert push(None, 0, M._ptr(zero), None, 0, None, None, None, None, C.byref(nrec), C.byref(nleft)) == 0   # nothing in, nothing asked
        assert L.ofdmrx_bank_resident_samples(h, 1) == 0 and L.ofdmrx_bank_preambles(h, 1) == 0
        assert L.ofdmrx_bank_last_stage_ops(h) >= 0
    finally:
        assert L.ofdmrx_bank_end(h, 4, *a) == 0 and nrec.value == 0 and nleft.value == 0
    # two banks in a row: positions and record numbers start over; the one-call entry answers as before
    for _ in range(2):
        per, _, _ = B.run_bank(rx, [pcm], B.block_rounds([len(pcm)], 30000))
        B.same(per[0][:2], staggered_truth[0])
    o2, r2, n2 = rx.decode_stream(pcm)
    B.same((o2, r2), staggered_truth[0])
    # a handle destroyed with an open bank frees it
    r = _rx()
    b = r.bank(2, 2)
    b.push([pcm[:50000], pcm[:30000]])
    r.close()


def test_cli_live_batch(tmp_path):
    """`decode_stream --live --batch OUTROOT A.wav B.wav C.wav`: the files and the summary lines of `--batch`, up to the order of the lines"""
    import os
    import struct
    import subprocess
    bin_dir = os.path.join(O.ROOT, "modem_amd", "bin")
    wavs = []
    for i, count in enumerate([2, 1, 3]):
        files = []
        for k in range(count):
            f = tmp_path / ("p%d_%d.dat" % (i, k))
            f.write_bytes(bytes(O.payload_for(1800 + 10 * i + k)))
            files.append(str(f))
        wav = tmp_path / ("w%d.wav" % i)
        subprocess.check_call([os.path.join(bin_dir, "encode"), str(wav), "8000", "16", "2", "1500", "6", "CALL %d" % i] + files)
        wavs.append(str(wav))
    empty = tmp_path / "empty.wav"                               # a WAV without sample frames: a channel that ends at once
    empty.write_bytes(b"RIFF" + struct.pack("<I", 36) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 2, 8000, 32000, 4, 16) + b"data" + struct.pack("<I", 0))
    wavs.insert(1, str(empty))
    runs = {}
    for name, flags in (("batch", ["--batch"]), ("live", ["--live", "--batch"])):
        root = tmp_path / name
        p = subprocess.run([os.path.join(bin_dir, "decode_stream")] + flags + [str(root)] + wavs, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        files = {(d, k): (root / d / k).read_bytes() for d in sorted(os.listdir(root)) for k in sorted(os.listdir(root / d))}
        runs[name] = (sorted(p.stderr.strip().splitlines()), files, sorted(os.listdir(root)))
    assert runs["batch"][2] == ["0", "1", "2", "3"] and len(runs["batch"][1]) == 6 and len(runs["batch"][0]) == 6
    assert runs["live"] == runs["batch"]
