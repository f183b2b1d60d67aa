"""Inputs for the header's ordered-statistics decoder and a plain numpy restatement of what decides its route (test infrastructure
shared by test_osd_vectors_cpu.py and test_gpu_header.py).

k_header.hip's OSD leaves by one of three routes: 1 the syndrome certificate, 2 orders 0-2 plus the d_min bound,
3 the full order-4 search.  Nothing in the product says which one a word took, so this module predicts it from the input:

  mrb(soft)            the information set: stable-descending reliabilities, Gauss-Jordan with the oracle's pivot rule
  route(soft)          1, 2 or 3, and the codeword routes 1 and 2 name
  header_fields(hard)  status / oper_mode / call_sign of decode.cc:417-446 from a decoded word

and it builds the inputs, all from fixed seeds:

  constructed()        order-k vectors: a codeword c, magnitudes <= 127, the signs flipped at k chosen RANKS of the information set.
                       Reliabilities do not change with a sign, so the information set is that of the unflipped word.  Premise (asserted
                       per vector): the k flipped magnitudes sum to strictly less than the 59 - k smallest of the others.  Any other
                       codeword differs from c in >= 59 positions (BCH bound); going from c to it gains at most the flipped magnitudes
                       and loses at least the 59 - k smallest others, so c is the strict optimum of the WHOLE code, it needs exactly k
                       flips of the order-0 candidate, and the decoder must return (c, unique) - no oracle involved.
  ties()               +-1 words (and +-1 with erasures): small integer metrics, best and runner-up often tie at a non-zero metric
  noisy_header_frame() an oracle-encoded frame with Gaussian noise on the 1280 samples of the header symbol only: sync and payload stay
                       exact while the header works at its own waterfall

The header levels below were fixed with the oracle alone (level_counts(); test_osd_vectors_cpu.py re-derives them)."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_lib as O

N, K, DMIN = 255, 71, 59
MAX_THREADS = 16


def pool_map(fn, items, threads=MAX_THREADS):
    """fn over items on at most 16 threads (the oracle's C calls release the GIL; never sized by the machine's CPU count)"""
    items = list(items)
    if not items:
        return []
    with ThreadPoolExecutor(max_workers=max(1, min(int(threads), MAX_THREADS, len(items)))) as ex:
        return list(ex.map(fn, items))


# ---------------------------------------------------------------- the code
@functools.lru_cache(maxsize=None)
def genmat():
    g = np.zeros((K, N), np.int8)
    O.lib().orc_bch_genmat(O.ptr(g))
    g = g.astype(np.uint8)
    g.setflags(write=False)
    return g


def encode(data71):
    """systematic codeword [255] of 71 data bits (orc_bch_encode)"""
    data71 = np.asarray(data71, np.uint8)
    data = np.packbits(np.concatenate([data71, [0]]).astype(np.uint8))
    par = np.zeros(23, np.uint8)
    O.lib().orc_bch_encode(O.ptr(np.ascontiguousarray(data)), O.ptr(par))
    return np.concatenate([data71, np.unpackbits(par)[:N - K]]).astype(np.uint8)


def is_codeword(h):
    h = np.asarray(h, np.uint8)
    return bool(((h[:K].astype(np.int64) @ genmat().astype(np.int64)) % 2 == h).all())


def bits_of(hard32):
    return np.unpackbits(np.asarray(hard32, np.uint8).reshape(-1, 32), axis=1)[:, :N]


def clamp(soft):
    return np.maximum(np.asarray(soft, np.int32), -127)


# ---------------------------------------------------------------- the information set
def mrb(soft, reduced=False):
    """-> perm, n_column_swaps (and the reduced generator [I | P] in permuted order).  Reliabilities |max(soft, -127)|, most reliable
    first, stable; Gauss-Jordan on the permuted generator: the pivot of step k is the first row >= k with a one in column k, else the
    first later column with a one in some row >= k is swapped with column k (in the matrix and in perm)"""
    rel = np.abs(clamp(soft))
    perm = np.argsort(-rel, kind="stable")
    M = genmat()[:, perm].copy()
    swaps = 0
    for k in range(K):
        rows = np.flatnonzero(M[k:, k])
        if rows.size == 0:
            c = k + 1 + int(np.flatnonzero(M[k:, k + 1:].any(axis=0))[0])
            M[:, [k, c]] = M[:, [c, k]]
            perm[[k, c]] = perm[[c, k]]
            swaps += 1
            rows = np.flatnonzero(M[k:, k])
        p = k + int(rows[0])
        if p != k:
            M[[k, p]] = M[[p, k]]
        hit = np.flatnonzero(M[:, k])
        hit = hit[hit != k]
        M[hit] ^= M[k]
    return (perm, swaps, M) if reduced else (perm, swaps)


def bound_holds(c, x, dmin=DMIN):
    """the d_min bound of osd_certify for codeword bits c on clamped soft values x (any common order): with w = (1 - 2 c) x, n_neg the
    number of negative w: n_neg < dmin and the dmin - n_neg smallest non-negative w sum to strictly more than |w| over the negative"""
    w = (1 - 2 * np.asarray(c, np.int64)) * np.asarray(x, np.int64)
    neg = w < 0
    need = dmin - int(neg.sum())
    if need <= 0:
        return False
    pos = np.sort(w[~neg])
    return bool(pos[:need].sum() > -w[neg].sum()) and pos.size >= need


def low_order_best(soft):
    """a best one of the 2557 candidates of orders 0-2, as code bits in natural order.  Which one of several equally good ones does
    not matter to route(): the bound below holds for none of them then (it implies a strictly best codeword)"""
    perm, _, M = mrb(soft, reduced=True)
    x = clamp(soft)[perm].astype(np.int64)
    cw0 = np.zeros(N, np.uint8)
    for i in np.flatnonzero(x[:K] < 0):
        cw0 ^= M[i]
    ia, ib = np.triu_indices(K, 1)
    allc = np.concatenate([cw0[None], cw0[None] ^ M, cw0[None] ^ M[ia] ^ M[ib]])
    assert allc.shape[0] == 2557
    met = (1 - 2 * allc.astype(np.int64)) @ x
    c = np.zeros(N, np.uint8)
    c[perm] = allc[int(np.argmax(met))]
    return c


def route_detail(soft, dmin=DMIN):
    """-> (route, codeword bits [255] that route 1 or 2 names, None on route 3)"""
    soft = np.asarray(soft, np.int8)
    h = (soft < 0).astype(np.uint8)
    if int((soft == 0).sum()) <= 16 and is_codeword(h):
        return 1, h
    c = low_order_best(soft)
    if bound_holds(c, clamp(soft), dmin):
        return 2, c
    return 3, None


def route(soft):
    return route_detail(soft)[0]


# ---------------------------------------------------------------- the header's fields
def crc16(md):
    """CRC<uint16_t>(0xA8F4) over the 64 bits of md, low bit first (decode.cc:428-429)"""
    crc = 0
    for i in range(64):
        t = (crc ^ (md >> i)) & 1
        crc = (crc >> 1) ^ (0xA8F4 if t else 0)
    return crc & 0xffff


def header_fields(hard32, unique=1):
    """decode.cc:417-446 -> (status, oper_mode, call_sign).  oper_mode is assigned once the CRC holds (decode.cc:433), a call sign only
    when the mode is one of the table's; the fields not reached keep their initial zero"""
    if not unique:
        return 2, 0, 0
    b = bits_of(hard32)[0]
    md = sum(int(b[i]) << i for i in range(55))
    cs = sum(int(b[55 + i]) << i for i in range(16))
    if crc16((md << 9) & 0xffffffffffffffff) != cs:
        return 3, 0, 0
    mode = md & 255
    if mode < 6 or mode > 13:
        return 4, mode, None                                       # (decode.cc never forms a call sign here: not compared)
    call = md >> 8
    if call == 0 or call >= 129961739795077:
        return 5, mode, call
    return 0, mode, call


def header_word(mode, call):
    """the 71 data bits of a header: 55 metadata bits + CRC-16 (encode.cc:272-278's layout, as decode.cc:422-429 reads it)"""
    md = (int(call) << 8) | (int(mode) & 255)
    cs = crc16((md << 9) & 0xffffffffffffffff)
    return np.array([(md >> i) & 1 for i in range(55)] + [(cs >> i) & 1 for i in range(16)], np.uint8)


# ---------------------------------------------------------------- constructed order-k vectors
class Vec:
    __slots__ = ("kind", "ranks", "c", "soft", "swaps", "margin")

    def __init__(self, kind, ranks, c, soft, swaps, margin):
        self.kind, self.ranks, self.c, self.soft, self.swaps, self.margin = kind, tuple(ranks), c, soft, swaps, margin

    def __repr__(self):
        return "<%s order %d ranks %s swaps %d margin %.3f>" % (self.kind, len(self.ranks), list(self.ranks), self.swaps, self.margin)


def _random_codeword(rng):
    return encode(rng.integers(0, 2, K).astype(np.uint8))


def premise(mags, flipped):
    """(sum of the flipped magnitudes, sum of the 59 - k smallest magnitudes elsewhere)"""
    mags = np.asarray(mags, np.int64)
    rest = np.delete(mags, list(flipped))
    return int(mags[list(flipped)].sum()), int(np.sort(rest)[:DMIN - len(flipped)].sum())


def make_vector(kind, c, mags, ranks, rng=None, minus128=False):
    """flip the signs of (1 - 2 c) mags at the information-set ranks; asserts the unchanged information set and the premise"""
    mags = np.asarray(mags, np.int32)
    assert mags.min() >= 0 and mags.max() <= 127
    clean = (1 - 2 * c.astype(np.int32)) * mags
    perm, swaps = mrb(clean)
    pos = [int(perm[r]) for r in ranks]
    soft = clean.copy()
    soft[pos] = -soft[pos]
    if minus128:                                                    # -128 clamps to -127: same reliability, same metric
        sat = np.flatnonzero(soft == -127)
        soft[sat[rng.random(sat.size) < 0.5]] = -128
    soft = soft.astype(np.int8)
    perm2, swaps2 = mrb(soft)
    assert (perm2 == perm).all() and swaps2 == swaps
    F, S = premise(mags, pos)
    assert F < S, (kind, ranks, F, S)
    return Vec(kind, ranks, c, soft, swaps, (S - F) / S)


def _mags(rng, style):
    if style == "plateau":                                          # many equal reliabilities: the stable order decides perm
        return rng.choice(np.array([127, 127, 90, 40, 12]), N)
    if style == "narrow":
        return rng.integers(20, 28, N)
    return rng.integers(1, 128, N)


def _ensure(rng, kind, ranks, style="random", minus128=False):
    """random codeword and magnitudes until the premise holds (it does for nearly every draw: the 55 smallest of 251 random
    magnitudes sum to about 800, four flipped ones to at most 508)"""
    for _ in range(50):
        c, mags = _random_codeword(rng), _mags(rng, style)
        perm, _ = mrb((1 - 2 * c.astype(np.int32)) * mags)
        F, S = premise(mags, [int(perm[r]) for r in ranks])
        if F < S:
            return make_vector(kind, c, mags, ranks, rng, minus128)
    raise AssertionError("no magnitudes with the premise for %s %s" % (kind, ranks))


def _marginal(rng, k):
    """order-k vector whose premise holds by less than 5 % of its right-hand side: large flipped magnitudes, 59 - k small ones
    elsewhere that sum to just above them"""
    for _ in range(200):
        c = _random_codeword(rng)
        n_small = DMIN - k
        small_pos = rng.choice(N, n_small, replace=False)
        mags = rng.integers(40, 128, N)
        mags[small_pos] = 1
        perm, _ = mrb((1 - 2 * c.astype(np.int32)) * mags)
        ranks = sorted(int(r) for r in rng.choice(K, k, replace=False))
        pos = [int(perm[r]) for r in ranks]
        if set(pos) & set(int(p) for p in small_pos):
            continue
        F = int(mags[pos].sum())
        S = F + 1 + int(rng.integers(0, max(1, int(0.05 * F) - 1)))   # S - F < 0.05 S
        if not (S - F) < 0.05 * S:
            continue
        base, extra = divmod(S, n_small)
        vals = np.full(n_small, base)
        vals[:extra] += 1
        for _ in range(3 * n_small):                                # spread them a little, the sum stays
            i, j = rng.integers(0, n_small, 2)
            if i != j and vals[i] > 2 and vals[j] < 38:
                vals[i] -= 1
                vals[j] += 1
        if vals.max() >= 40:
            continue
        mags[small_pos] = vals
        perm2, _ = mrb((1 - 2 * c.astype(np.int32)) * mags)
        if [int(perm2[r]) for r in ranks] != pos:
            continue
        v = make_vector("d-marginal", c, mags, ranks)
        assert v.margin < 0.05
        return v
    raise AssertionError("no marginal vector of order %d" % k)


EXTREMES = [(), (0,), (70,), (0, 1), (69, 70), (0, 70), (0, 1, 2), (68, 69, 70), (0, 35, 70), (0, 1, 2, 3), (67, 68, 69, 70),
            (0, 1, 69, 70), (0, 23, 46, 70)]
STYLES = ("random", "plateau", "narrow")


@functools.lru_cache(maxsize=None)
def constructed():
    """every constructed vector (fixed seeds).  (a) sliding runs of four and three ranks, (b) the extremes of the pair, triple and
    quad tables, (c) 24 random patterns per order 1-4, (d) 24 marginal vectors of orders 3 and 4; magnitude plateaus and -128 on
    every third vector of (a) - (c)"""
    rng = np.random.default_rng(20259)
    out, n = [], 0

    def add(kind, ranks):
        nonlocal n
        out.append(_ensure(rng, kind, ranks, STYLES[n % 3], minus128=n % 3 == 1))
        n += 1

    for r in range(68):
        add("a-run4", (r, r + 1, r + 2, r + 3))
    for r in range(69):
        add("a-run3", (r, r + 1, r + 2))
    for ranks in EXTREMES:
        add("b-extreme", ranks)
    for k in (1, 2, 3, 4):
        for _ in range(24):
            add("c-random", sorted(int(r) for r in rng.choice(K, k, replace=False)))
    for i in range(24):
        out.append(_marginal(rng, 3 + i % 2))
    return tuple(out)


def constructed_conditions(vecs):
    """conditions on the inputs themselves: at least a quarter needs a column swap, some need three or more; every rank takes every
    role of a triple and a quad"""
    swaps = np.array([v.swaps for v in vecs])
    assert (swaps >= 1).mean() >= 0.25 and (swaps >= 3).any(), np.bincount(swaps)
    for k in (3, 4):
        for role in range(k):
            seen = {v.ranks[role] for v in vecs if len(v.ranks) == k}
            assert seen >= set(range(role, K - (k - 1 - role))), (k, role)
    assert any((v.soft == -128).any() for v in vecs)
    assert sum(v.margin < 0.05 for v in vecs if v.kind == "d-marginal") == 24


# ---------------------------------------------------------------- tie vectors
N_TIES = 128


@functools.lru_cache(maxsize=None)
def ties():
    """-> (uniform +-1 words [128, 255], +-1 words with each position zeroed with probability 0.12 [128, 255])"""
    rng = np.random.default_rng(7711)
    a = (1 - 2 * rng.integers(0, 2, (N_TIES, N))).astype(np.int8)
    b = (1 - 2 * rng.integers(0, 2, (N_TIES, N))).astype(np.int8)
    b[rng.random((N_TIES, N)) < 0.12] = 0
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def oracle_osd(softs, threads=MAX_THREADS):
    """O.osd over many words on at most 16 threads -> code bits [n, 255], unique [n]"""
    softs = np.ascontiguousarray(softs, np.int8).reshape(-1, N)
    res = pool_map(lambda s: O.osd(s), softs, threads)
    return np.stack([bits_of(h)[0] for h, _ in res]), np.array([int(u) for _, u in res])


# ---------------------------------------------------------------- frames with noise on the header symbol only
# Levels: noise power on the header symbol's samples relative to full scale, fixed with the oracle alone on HDR_FRAMES frames of mode 6,
# 8 kHz, 2 channels, in 1 dB steps (frame k: payload k % 4, noise seed 1000 HDR_SEED + k).  test_osd_vectors_cpu.py re-derives them.
#   HDR_SEARCH_DB  the noisiest level at which the oracle's header status is 0 in at least 46 of 48 frames and no frame is on route 1
#                  (one dB up only 29 of 48 headers decode).  Every frame is on route 3 there
#   HDR_MIXED_DB   the level at which routes 2 and 3 both hold at least a quarter of the frames (route 2 has none at HDR_SEARCH_DB;
#                  at -7 dB it has them all)
#   HDR_EDGE_DB    the header's own waterfall: status 0 in 25 - 75 % of the frames
# HDR_ORACLE: level -> (frames, header status 0, on route 1, on route 2, on route 3) of the oracle
HDR_SEED = 41
HDR_FRAMES = 48
HDR_SEARCH_DB = -4.0
HDR_MIXED_DB = -6.0
HDR_EDGE_DB = -3.0
HDR_ORACLE = {
    -7.0: (48, 48, 0, 48, 0),
    -6.0: (48, 48, 0, 29, 19),
    -5.0: (48, 48, 0, 1, 47),
    -4.0: (48, 46, 0, 0, 48),
    -3.0: (48, 29, 0, 0, 48),
}
HDR_PAYLOAD_BASE = 5000
# The 16-frame sets of mono input and of 48 kHz: (rate, channels) -> level name -> (level as an 8 kHz 2-channel level, which
# equivalent_db() carries over, (frames, header status 0, route 1, route 2, route 3) of the oracle).  Chosen like the levels above, in
# 1 dB steps with the oracle alone: search = the noisiest with at least 14 of 16 headers decoded and none on route 1, edge = status 0 in
# 25 - 75 % of the frames.  equivalent_db() is the first-order account; mono input sits 1 dB further down than it says (one dB
# below its edge level 13 of 16 mono headers decode: fewer than a quarter fail), 48 kHz where it says.
HDR_SMALL = {
    (8000, 1): dict(search=(-4.0, (16, 16, 0, 0, 16)), above_search=(-3.0, (16, 13, 0, 0, 16)), edge=(-2.0, (16, 5, 0, 0, 16))),
    (48000, 2): dict(search=(-4.0, (16, 14, 0, 0, 16)), above_search=(-3.0, (16, 6, 0, 0, 16)), edge=(-3.0, (16, 6, 0, 0, 16))),
}


def equivalent_db(db, rate=8000, channels=2):
    """the level that puts on the header's carriers the noise that db puts there at 8 kHz, 2 channels.  The symbol lasts rate / 8000
    times as many samples, so each carrier collects that much less of a given per-sample power: + 10 log10(rate / 8000).  A mono
    recording carries the real part alone; the analytic signal the receiver rebuilds doubles the amplitude of what lies at positive
    frequencies, noise included, while the one channel got half the power: twice the density on the carriers, - 3.01 dB"""
    return db + 10.0 * np.log10(rate / 8000.0) - (10.0 * np.log10(2.0) if channels == 1 else 0.0)


def symbol_geometry(rate):
    """(symbol length, symbol + guard) in samples"""
    return 1280 * rate // 8000, 1440 * rate // 8000


@functools.lru_cache(maxsize=None)
def clean_frame(k4, rate=8000, channels=2):
    """-> (payload, oracle-encoded mode-6 frame, sc_start of the oracle's decode of it)"""
    pay = O.payload_for(HDR_PAYLOAD_BASE + k4)
    pcm = O.encode_pcm(pay, channels=channels, mode=6, freq_off=1500, call_sign="HEADER", rate=rate)
    out, res = O.decode(pcm, rate=rate)
    assert res.status == 0 and (out == pay).all()
    pcm.setflags(write=False)
    return pay, pcm, int(res.sc_start)


def add_header_noise(pcm, sc_start, db, seed, rate=8000):
    """Gaussian noise of power 10^(db/10) of full scale (half of it in each of two channels; a mono recording gets the one half) on
    the samples of the header symbol, rounded and clipped to int16"""
    sl, stride = symbol_geometry(rate)
    a = sc_start + stride
    rng = np.random.default_rng([int(seed), rate, pcm.shape[1]])             # (the same unit noise at every level)
    noise = rng.normal(0.0, np.sqrt(0.5 * 10.0 ** (db / 10.0)), (sl, pcm.shape[1])) * 32767.0
    out = pcm.copy()
    out[a:a + sl] = np.clip(np.rint(pcm[a:a + sl].astype(np.float64) + noise), -32768, 32767).astype(np.int16)
    return out


def noisy_header_frame(payload_k, db, seed, rate=8000, channels=2):
    """frame of payload payload_k % 4 with header-only noise -> (payload, pcm [samples, channels] int16)"""
    pay, pcm, sc = clean_frame(int(payload_k) % 4, rate, channels)
    return pay, add_header_noise(pcm, sc, db, seed, rate)


def header_frames(db, n, rate=8000, channels=2, seed=HDR_SEED):
    """n frames at one level -> (payloads [n, 5380], pcm [n, samples, channels])"""
    made = [noisy_header_frame(k, db, 1000 * seed + k, rate, channels) for k in range(n)]
    return np.stack([p for p, _ in made]), np.stack([f for _, f in made])


def oracle_header(pcms, rate=8000, threads=MAX_THREADS):
    """the oracle on every frame -> list of (status, payload, hdr_soft [255] int8)"""
    def one(pcm):
        out, res, tb = O.decode(pcm, taps=True, rate=rate)
        return int(res.status), out, tb.hdr_soft.copy()
    return pool_map(one, list(pcms), threads)


def level_counts(db, n=HDR_FRAMES, threads=MAX_THREADS, rate=8000, channels=2):
    """-> (frames, header status 0 [payload decoded in each of them: asserted], route 1, route 2, route 3) of the oracle; db is the
    8 kHz 2-channel level, carried over to another rate or to mono by equivalent_db()"""
    pays, pcms = header_frames(equivalent_db(db, rate, channels), n, rate, channels)
    res = oracle_header(pcms, rate=rate, threads=threads)
    routes = pool_map(lambda r: route(r[2]), res, threads)
    for (st, out, _), pay in zip(res, pays):
        assert st in (0, 2, 3, 4, 5), st                            # never 6: the noise does not reach the payload
        assert (out == pay).all() if st == 0 else not out.any()
    return (n, sum(r[0] == 0 for r in res)) + tuple(routes.count(q) for q in (1, 2, 3))
