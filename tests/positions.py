"""Inputs of the position sweeps (test_gpu_positions.py, test_positions_model_cpu.py): one clean mode-6 frame behind a noise prefix
whose length puts the accepted trigger's falling edge at a wanted residue modulo the scan tiles, the windows cut from it, the
stream-end and stream-head sets, and the oracle runs over them (a thread pool, cached for the whole test session).

The falling edge of a window is  g = sc_start - symbol_pos + BUFFER_LEN - 1  (k_sync.hip: st.sc_start = g - (BUFFER_LEN - 1) + sp);
the batch scan walks tiles of 64 lanes x SYNC_PER sample times (512 or 1024), the stream scan tiles of 4096.
"""
import ctypes as C
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_lib as O

ORACLE_THREADS = 16          # a constant: the machines that run the suite grant 16 CPUs whatever they report
NOISE_STD = 0.02             # prefix noise, of full scale
STREAM_TILE = 4096
SYNC_TILE = 1024
PIECE = 128                  # consecutive offsets per test case
ROWS = 50                    # constellation rows of mode 6

Ref = namedtuple("Ref", "status sc_start symbol_pos cfo_rad n_sync_rejects oper_mode call_sign payload")


class _RateCfg(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("rate", "symbol_len", "guard_len", "filter_len", "buffer_len", "search_pos")]


def rate_cfg(rate):
    rc = _RateCfg()
    assert O.lib().orc_rate_lookup(C.c_int(rate), C.byref(rc)) == 1
    return rc


def falling_edge(ref, rate):
    """time of the accepted trigger's falling edge in the window's own coordinates"""
    assert ref.sc_start >= 0
    return ref.sc_start - ref.symbol_pos + rate_cfg(rate).buffer_len - 1


# ---------------------------------------------------------------- the oracle, pooled and cached
_REFS = {}


def _one(args):
    pcm, rate, skip = args
    out, r = O.decode(pcm, skip=skip, rate=rate)
    return Ref(int(r.status), int(r.sc_start), int(r.symbol_pos), float(r.cfo_rad), int(r.n_sync_rejects), int(r.oper_mode),
               int(r.call_sign), out)


def oracle_run(key, stream, cuts, rate, skip=0):
    """the oracle on stream[a:b] for every (a, b) of cuts -> list of Ref.  `key` names the stream: results are kept per
    (key, a, b, skip), so the tests that share a sweep pay for it once"""
    O.lib()                                                       # (built and bound before the threads start)
    todo = [(a, b) for a, b in dict.fromkeys(cuts) if (key, a, b, skip) not in _REFS]
    if todo:
        with ThreadPoolExecutor(max_workers=ORACLE_THREADS) as pool:
            got = list(pool.map(_one, [(stream[a:b], rate, skip) for a, b in todo]))
        for (a, b), r in zip(todo, got):
            _REFS[(key, a, b, skip)] = r
    return [_REFS[(key, a, b, skip)] for a, b in cuts]


# ---------------------------------------------------------------- the streams
def _burst(rate, channels, seed):
    """one false trigger, as _with_false_triggers (test_gpu_parity.py) builds them: 3 half symbols of silence, then a noise segment
    of half a symbol three times over (the Schmidl-Cox metric fires on it, the MLS correlation of the accept path does not)"""
    hs = 640 * rate // 8000
    rng = np.random.default_rng(seed)
    seg = (rng.normal(0, 0.12, (hs, 2)) * 32767).astype(np.int16)[:, :channels]
    return np.concatenate([np.zeros((3 * hs, channels), np.int16), seg, seg, seg], axis=0)


class Sweep:
    """S = prefix + frame and its windows S[d : d + L], d in offsets.  The prefix is Gaussian noise (int16) with, for with_burst, one
    false trigger in it; the frame (O.encode_pcm: a second of silence, pilot, preamble, header, payload, a second of silence) stays
    noise-free.  The prefix is cut so that g = residue (mod 4096) at d = 0; since g falls by one per offset, residue = len(offsets) / 2
    makes it cross a multiple of 4096 (and of 1024) in the middle of the sweep."""

    def __init__(self, name, rate, channels, with_burst, offsets, residue, seed):
        self.name, self.rate, self.channels, self.with_burst = name, rate, channels, with_burst
        self.offsets = list(offsets)
        self.residue = residue
        hs = 640 * rate // 8000
        self.payload = O.payload_for(seed)
        frame = O.encode_pcm(self.payload, channels=channels, mode=6, rate=rate)
        base = max(self.offsets) + 12 * hs                        # lead-in, the burst's 6 half symbols, 5 quiet ones behind it
        rng = np.random.default_rng(seed)
        noise = np.rint(rng.normal(0, NOISE_STD * 32767, (base + STREAM_TILE, channels))).astype(np.int16)
        if with_burst:
            noise[len(noise) - 11 * hs: len(noise) - 5 * hs] = _burst(rate, channels, seed + 1)
        # the prefix grows at its FRONT, so nothing moves relative to the frame: measure g with the shortest prefix, add the difference
        s0 = np.concatenate([noise[STREAM_TILE:], frame], axis=0)
        g0 = falling_edge(oracle_run(name + "/calib", s0, [(0, len(s0))], rate)[0], rate)
        delta = (residue - g0) % STREAM_TILE
        self.stream = np.ascontiguousarray(np.concatenate([noise[STREAM_TILE - delta:], frame], axis=0))
        self.stream.setflags(write=False)
        self.frame_at = base + delta
        self.L = len(self.stream) - max(self.offsets)             # every window holds the whole frame
        assert self.frame_at + len(frame) == len(self.stream)

    def window(self, d):
        return self.stream[d: d + self.L]

    def windows(self, offsets):
        return np.stack([self.window(d) for d in offsets])

    def refs(self, offsets, skip=0):
        return oracle_run(self.name, self.stream, [(d, d + self.L) for d in offsets], self.rate, skip)

    def pieces(self):
        size = piece_size(self.name)
        return [self.offsets[i: i + size] for i in range(0, len(self.offsets), size)]


# name -> (rate, channels, with_burst, offsets, residue, payload seed).  The full sweeps cross the multiple of 4096 at d = 512, the
# partial ones at d = 128; the 44.1 kHz burst sweep covers the 64 offsets around its crossing
SWEEPS = {
    "8k2": (8000, 2, False, range(1024), 512, 1501),
    "8k2b": (8000, 2, True, range(1024), 512, 1502),
    "8k1": (8000, 1, False, range(1024), 512, 1503),
    "48k2": (48000, 2, False, range(256), 128, 1504),
    "44k1": (44100, 1, False, range(256), 128, 1505),
    "44k1b": (44100, 1, True, range(96, 160), 128, 1506),
    "16k1": (16000, 1, False, range(256), 128, 1507),
}
FULL = ("8k2", "8k2b", "8k1")
PARTIAL = ("48k2", "44k1", "44k1b", "16k1")
_SWEEPS = {}


def sweep(name):
    if name not in _SWEEPS:
        rate, channels, with_burst, offsets, residue, seed = SWEEPS[name]
        _SWEEPS[name] = Sweep(name, rate, channels, with_burst, offsets, residue, seed)
    return _SWEEPS[name]


def piece_size(name):
    """consecutive offsets per test case: about 2 s of oracle time on 16 threads (a window of the higher rates costs more)"""
    return PIECE if SWEEPS[name][0] == 8000 else PIECE // 2


def piece_ids(names=FULL + PARTIAL):
    """(sweep name, piece index) of every case of a sweep test"""
    return [(name, k) for name in names for k in range((len(SWEEPS[name][3]) + piece_size(name) - 1) // piece_size(name))]


def crossing_offsets(name):
    """the offsets at which g is one below, at, and one above a multiple of 1024"""
    _, _, _, offsets, residue, _ = SWEEPS[name]
    return [d for d in offsets if (residue - d) % SYNC_TILE in (SYNC_TILE - 1, 0, 1)]


def seam_offsets(name):
    """the sparse subset of a sweep: every 64th offset, the ends, the three offsets around each crossing of a multiple of 1024"""
    sw = sweep(name)
    lo, hi = sw.offsets[0], sw.offsets[-1]
    return sorted(set(range(lo, hi + 1, 64)) | {lo, lo + 1, hi} | set(crossing_offsets(name)))


def edge_residues(sw, refs, offsets, modulus):
    """g mod modulus of every window, with g checked against the shift rule (the oracle's own numbers: every window accepted)"""
    out = []
    for d, r in zip(offsets, refs):
        assert r.status == 0, (sw.name, d, r.status)
        out.append(falling_edge(r, sw.rate) % modulus)
    return out


# ---------------------------------------------------------------- stream end and stream head (8 kHz)
def _accepted(key, stream, a, b, rate):
    return oracle_run(key, stream, [(a, b)], rate)[0].status != 1


def end_lengths(name):
    """the buffers S[:n] of a sweep's stream: n* (the shortest buffer in which the oracle accepts the preamble, by bisection) and
    the lengths n* - 3 .. n* + 3, the seven around the end of the header symbol and the seven around the end of the last payload
    symbol -> (n*, sorted lengths)"""
    sw = sweep(name)
    rc = rate_cfg(sw.rate)
    sym = rc.symbol_len + rc.guard_len
    full = oracle_run(name, sw.stream, [(0, len(sw.stream))], sw.rate)[0]
    assert full.status == 0
    lo, hi = full.sc_start, full.sc_start + 2 * rc.buffer_len    # NO_SYNC at lo, accepted at hi
    assert not _accepted(name, sw.stream, 0, lo, sw.rate) and _accepted(name, sw.stream, 0, hi, sw.rate)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _accepted(name, sw.stream, 0, mid, sw.rate):
            hi = mid
        else:
            lo = mid
    hdr_end = full.sc_start + sym + rc.symbol_len                # decoder.c: the header's body starts one symbol behind sc_start,
    pay_end = full.sc_start + (2 + ROWS) * sym + rc.symbol_len   # row j's body at sc_start + (3 + j) symbols
    assert pay_end + 3 <= len(sw.stream)
    ns = {c + k for c in (hi, hdr_end, pay_end) for k in range(-3, 4)}
    return hi, sorted(ns)


def end_refs(name, lengths):
    sw = sweep(name)
    return oracle_run(name, sw.stream, [(0, n) for n in lengths], sw.rate)


HEAD_KEEP = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025)             # samples of the leading silence that remain
HEAD_STEP = 128


def head_cuts(name):
    """the frame of a sweep without its prefix, F[c:]: the leading second of silence cut down to HEAD_KEEP samples, then cuts into
    the pilot symbol every HEAD_STEP samples until the oracle first answers NO_SYNC, the exact cut c* at which it first does
    (bisection inside that last step) and c* - 3 .. c* + 3 -> (frame, c*, sorted cuts)"""
    sw = sweep(name)
    rc = rate_cfg(sw.rate)
    frame = sw.stream[sw.frame_at:]
    key = name + "/head"
    cuts = [sw.rate - k for k in HEAD_KEEP]
    c = sw.rate
    limit = sw.rate + 4 * (rc.symbol_len + rc.guard_len)
    while _accepted(key, frame, c, len(frame), sw.rate):
        cuts.append(c)
        c += HEAD_STEP
        assert c <= limit, "the oracle still accepts a preamble that is no longer in the buffer"
    cuts.append(c)
    lo, hi = c - HEAD_STEP, c                                     # accepted at lo, NO_SYNC at hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _accepted(key, frame, mid, len(frame), sw.rate):
            lo = mid
        else:
            hi = mid
    cuts += [hi + k for k in range(-3, 4)]
    return frame, hi, sorted(set(cuts))


def head_refs(name, frame, cuts):
    return oracle_run(name + "/head", frame, [(c, len(frame)) for c in cuts], sweep(name).rate)
