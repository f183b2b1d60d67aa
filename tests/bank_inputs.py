"""Shared inputs and drivers of the live feed bank's tests (ofdmrx_bank_*): the channels, the push schedules, one
driver that pushes a schedule through a bank and one that pushes a single channel through a feed."""
import functools

import numpy as np

import oracle_lib as O

TILE = 4096
LEADS = (0, 1, 4095, 4096, 4097, 10000)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def three():
    """the three-frame mode-6 stream at -30 dB"""
    pay = O.payload_for(300, count=3)
    return _frozen(O.impair(O.encode_pcm(pay, channels=2), noise_db=-30, seed=11, frame=0))


@functools.lru_cache(maxsize=None)
def staggered():
    """six 2-channel channels: the three-frame stream behind 0, 1, 4095, 4096, 4097 and 10 000 samples of leading zeros"""
    return tuple(_frozen(np.concatenate([np.zeros((lead, 2), np.int16), three()])) for lead in LEADS)


@functools.lru_cache(maxsize=None)
def mixed(channels=2, mirror=False, seed=5):
    """the feed tests' mixed stream: modes 6 - 13 behind gaps of silence or noise, the header of one frame and the payload of another
    destroyed, a last frame cut off inside its payload; mirror: the same parts in reverse order (the cut-off frame stays last)"""
    rng = np.random.default_rng(seed)
    parts = []
    for i, mode in enumerate([6, 7, 8, 9, 10, 11, 12, 13]):
        p = O.payload_for(100 + i)
        pcm = O.encode_pcm(p, channels=2, mode=mode, call_sign="CALL%d" % i)
        gap = int(rng.integers(0, 3 * 8000)) | 1                 # 0 .. 3 s at an odd offset
        noise = (rng.normal(0, 300, size=(gap, 2)) if i % 2 else np.zeros((gap, 2))).astype(np.int16)
        if i == 3:                                               # the header destroyed
            sc = 8000 + 1440                                     # pilot, then the S&C symbol and the header symbol
            pcm = pcm.copy()
            pcm[sc + 1440: sc + 3 * 1440] = rng.integers(-3000, 3000, size=(2 * 1440, 2))
        if i == 5:                                               # the payload destroyed
            pcm = pcm.copy()
            pcm[8000 + 6 * 1440: 8000 + 20 * 1440] = rng.integers(-3000, 3000, size=(14 * 1440, 2))
        parts.append([noise, pcm])
    if mirror:
        parts.reverse()
    last = O.encode_pcm(O.payload_for(199), channels=2)
    s = np.concatenate([a for pair in parts for a in pair] + [last[: len(last) // 2]])   # cut off inside its payload
    s = O.impair(s, noise_db=-30, seed=seed, frame=0)
    if channels == 1:
        s = np.ascontiguousarray(s[:, :1])
    return _frozen(s)


def noise(n, seed, sigma=300):
    return np.random.default_rng(seed).normal(0, sigma, size=(n, 2)).astype(np.int16)


def block_rounds(lengths, blocks):
    """every channel in blocks of its own size, in lock step -> rounds[r][c] = samples channel c brings in round r"""
    blocks = [blocks] * len(lengths) if np.isscalar(blocks) else list(blocks)
    n_rounds = max((n + b - 1) // b for n, b in zip(lengths, blocks))
    return [[max(0, min(b, n - r * b)) for n, b in zip(lengths, blocks)] for r in range(n_rounds)]


def cat(parts):
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def same(got, want):
    assert len(got[1]) == len(want[1]), (len(got[1]), len(want[1]))
    assert got[0].tobytes() == want[0].tobytes()
    assert got[1].tobytes() == want[1].tobytes()


def run_bank(rx, chans, rounds, ends=None, end=True):
    """push the schedule through one bank.  ends: {round: [channels that end with that round's block]}.
    -> (per channel (payloads, results, indices), per call (record_channel, record_index), ops per push call)"""
    chans = [c if c.ndim == 2 else c[:, None] for c in chans]
    at = [0] * len(chans)
    calls, ops = [], []
    per = [[] for _ in chans]

    def take(ret):
        o, r, rc, ri = ret[:4]
        calls.append((rc.copy(), ri.copy()))
        for c in range(len(chans)):
            m = rc == c
            per[c].append((o[m], r[m], ri[m]))

    with rx.bank(len(chans), chans[0].shape[1], chans[0].dtype) as b:
        for r, lens in enumerate(rounds):
            blocks = [chans[c][at[c]:at[c] + n] for c, n in enumerate(lens)]
            e = None
            if ends and r in ends:
                e = [c in ends[r] for c in range(len(chans))]
            take(b.push(blocks, ends=e))
            ops.append(b.last_stage_ops)
            at = [a + n for a, n in zip(at, lens)]
        if end:
            take(b.end())
            assert not b.open
    out = [(np.concatenate([p[0] for p in q]), np.concatenate([p[1] for p in q]), np.concatenate([p[2] for p in q])) for q in per]
    return out, calls, ops


def run_feed(rx, chan, lens):
    """one channel through a single feed with the given push lengths (zero lengths left out) -> (payloads, results)"""
    chan = chan if chan.ndim == 2 else chan[:, None]
    got, at = [], 0
    with rx.feed(chan.shape[1], chan.dtype) as f:
        for n in lens:
            if n:
                got.append(f.push(chan[at:at + n]))
                at += n
        got.append(f.end())
    return cat(got)


def call_order_ok(calls):
    """within every call: by channel index, then by preamble order"""
    for rc, ri in calls:
        key = list(zip(rc.tolist(), ri.tolist()))
        assert key == sorted(key), key
