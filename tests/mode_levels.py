"""Noise levels per mode of the mode table, fixed with the oracle alone (test infrastructure shared by test_mode_levels_cpu.py,
test_gpu_modes.py and the per-mode sweeps).

The waterfall of the eight modes is not the same: the QPSK modes (8, 9, 12, 13) decode 4 - 6 dB further down than the 8PSK modes, and the
width of the band (256 .. 512 carriers at the same total power) moves it by another dB.  For every mode three noise levels (orc_chan_awgn's
noise_db: per-sample noise power relative to full scale) are written down here with the seed of their frames:

  list1      every frame decodes, every frame has raw bit errors (bit_flips > 0), and the sign-following path of the oracle's list
             decoder satisfies the rule "min_fork > metric" (oracle/polar.c: orc_polar_sc_path): the list-1 pass's regime
  list       the frames decode, but that rule fails: only the list decoder can finish them (the "-17 dB class" of mode 6)
  waterfall  the oracle decodes between a quarter and three quarters of 48 frames

Frames are oracle-made - frame k of (mode, kind) is O.encode_pcm of payload_for(PAYLOAD_BASE + 100 mode + k % 4) in that mode, then
O.impair with the level, the kind's seed and frame = k - so the same frames can be decoded by anything.  ORACLE records what the oracle
made of them (frames, decoded, decoded from a lane above 0); tests/test_mode_levels_cpu.py re-derives all of it.

Lanes above 0.  On AWGN (and under the multipath model) the oracle's list-8 decoder never delivered from a lane above 0: none of 4600
waterfall frames over the eight modes (13 seeds each) and none of 1100 frames behind a deep two-path notch did.  That is what the code
predicts: the final lanes are ordered by path metric, a wrong path that survives to the end beside the transmitted one differs from
it by a codeword of weight >= 32 and has the better metric only if most of that codeword's soft bits were received wrong.  So the
vectors that make the list decoder replace its best path by a CRC-failing one and k_finish choose a later lane are CONSTRUCTED from
an oracle-made frame (lane_vector below): the list-level frame's own LLRs, with the soft bits on the support of a
weight-32 codeword turned weakly (factor -0.3) against the transmitted codeword.  The path that follows them costs nothing and
fails the CRC-32; the transmitted path pays 0.3 |llr| on 32 positions and is delivered from lane 1 (two such
codewords at once push the transmitted path out of a list of 8 at the list level: status 6).  The condition "a lane
above 0 wins in each frozen table" is checked on these vectors, from the oracle alone, like the others."""
import ctypes as C
import functools

import numpy as np

import oracle_lib as O

MODES = tuple(range(6, 14))
PAYLOAD_BASE = 3000
N = dict(list1=4, list=2, waterfall=48)
#        mode: kind -> (noise_db, seed)
LEVELS = {
    6: dict(list1=(-21.0, 11), list=(-17.0, 12), waterfall=(-14.5, 13)),
    7: dict(list1=(-21.0, 11), list=(-17.0, 12), waterfall=(-14.1, 13)),
    8: dict(list1=(-17.0, 11), list=(-12.5, 12), waterfall=(-10.7, 13)),
    9: dict(list1=(-17.0, 11), list=(-12.5, 12), waterfall=(-10.25, 13)),
    10: dict(list1=(-21.0, 11), list=(-17.0, 12), waterfall=(-15.25, 13)),
    11: dict(list1=(-21.0, 11), list=(-17.0, 12), waterfall=(-14.0, 13)),
    12: dict(list1=(-17.0, 11), list=(-12.5, 12), waterfall=(-10.6, 13)),
    13: dict(list1=(-14.0, 11), list=(-11.0, 12), waterfall=(-8.8, 13)),
}
#        mode: kind -> (frames, decoded by the oracle, decoded from a lane above 0)
ORACLE = {
    6: dict(list1=(4, 4, 0), list=(2, 2, 0), waterfall=(48, 28, 0)),
    7: dict(list1=(4, 4, 0), list=(2, 2, 0), waterfall=(48, 20, 0)),
    8: dict(list1=(4, 4, 0), list=(2, 2, 0), waterfall=(48, 24, 0)),
    9: dict(list1=(4, 4, 0), list=(2, 2, 0), waterfall=(48, 21, 0)),
    10: dict(list1=(4, 4, 0), list=(2, 2, 0), waterfall=(48, 22, 0)),
    11: dict(list1=(4, 4, 0), list=(2, 2, 0), waterfall=(48, 23, 0)),
    12: dict(list1=(4, 4, 0), list=(2, 2, 0), waterfall=(48, 31, 0)),
    13: dict(list1=(4, 4, 0), list=(2, 2, 0), waterfall=(48, 21, 0)),
}
# the two waterfall frames per mode that the GPU stage tests take: (one the oracle decodes, one it loses)
PICKS = {6: (1, 0), 7: (1, 0), 8: (0, 1), 9: (5, 0), 10: (1, 0), 11: (0, 1), 12: (1, 0), 13: (0, 3)}
# lane vectors: mode -> (information position whose weight-32 codeword is turned, the lane the oracle then delivers from, L = 8 and L = 4)
LANE = {6: (46592, 1), 7: (57604, 1), 8: (46592, 1), 9: (57604, 1), 10: (46336, 1), 11: (57488, 1), 12: (46336, 1), 13: (57488, 1)}
LANE_FACTOR = -0.3


@functools.lru_cache(maxsize=None)
def mode_of(mode):
    m = O.Mode()
    assert O.lib().orc_mode_lookup(mode, C.byref(m))
    return m


def payload(mode, k):
    return O.payload_for(PAYLOAD_BASE + 100 * mode + k % 4)


@functools.lru_cache(maxsize=None)
def clean(mode, k4=0):
    return O.encode_pcm(payload(mode, k4), channels=2, mode=mode, freq_off=1500, call_sign="MODE%d" % mode)


def frame(mode, kind, k):
    db, seed = LEVELS[mode][kind]
    return O.impair(clean(mode, k % 4), noise_db=db, seed=seed, frame=k)


def frames(mode, kind):
    return np.stack([frame(mode, kind, k) for k in range(N[kind])])


def decode_batch(pcm, threads=16, list_size=8):
    """orc_decode_batch on [n, samples, 2] int16 -> payloads [n, 5380], results (structured array)"""
    from modem_amd.ofdmrx import RESULT_DTYPE
    pcm = np.ascontiguousarray(pcm)
    n, spf, ch = pcm.shape
    out = np.zeros((n, 5380), np.uint8)
    res = np.zeros(n * 56, np.uint8)
    O.lib().orc_decode_batch(O.ptr(pcm), O.FMT_S16, ch, spf, spf * 2 * ch, n, list_size, O.ptr(out), O.ptr(res), min(threads, 16))
    return out, res.view(RESULT_DTYPE).reshape(-1)


def lanes(llr, table, L=8):
    """the oracle's list decoder on one LLR vector: per-lane messages [L, 5512] (mesg_bits / 8 bytes, zero-padded), metrics [L], and
    the lane decode.cc:532-541 delivers from: the first whose CRC-32 over 43072 bits is zero (-1: none)"""
    llr = np.ascontiguousarray(llr, np.float32)
    fr = O.frozen(table)
    mesg = np.zeros((L, 5512), np.uint8)
    metric = np.zeros(L, np.float32)
    O.lib().orc_polar_lane_mesg(O.ptr(llr), O.ptr(fr), 16, L, O.ptr(mesg), 5512, O.ptr(metric))
    best = -1
    for k in range(L - 1, -1, -1):
        if O.lib().orc_crc32_bytes(0xD419CC15, O.ptr(mesg[k]), 43072 // 8) == 0:
            best = k
    return mesg, metric, best


def sc_rule(llr, table):
    """does the sign-following path satisfy the list-1 pass's rule: min_fork > metric"""
    _, metric, fork = O.polar_sc_path(llr, O.frozen(table))
    return bool(fork > metric)


def frozen_bits(table):
    fz = O.frozen(table)
    return ((fz[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(np.uint8).reshape(-1)


def codeword_of(i):
    """x = u F^(x16) for u = e_i, in the decoder's order (at every level the left half of a block takes the XOR of the right half)"""
    x = np.zeros(65536, np.uint8)
    x[i] = 1
    d = 1
    while d < x.size:
        v = x.reshape(-1, 2, d)
        v[:, 0, :] ^= v[:, 1, :]
        d *= 2
    return x


def lane_position(mode):
    """an unfrozen position of that mode's table whose index has five ones (a codeword of weight 32 inside the unshortened part): the
    first one for the even modes, the middle one for the odd modes"""
    m = mode_of(mode)
    fz = frozen_bits(m.table)
    cand = [i for i in range(m.cons_bits) if not fz[i] and bin(i).count("1") == 5]
    return cand[len(cand) // 2 if mode & 1 else 0]


def lane_vector(mode, llr):
    """the LLRs of an oracle-made frame with the soft bits of LANE[mode]'s codeword turned weakly against the transmitted codeword"""
    m = mode_of(mode)
    llr = np.array(llr, np.float32)
    cw = codeword_of(LANE[mode][0])
    assert cw.sum() == 32 and not cw[m.cons_bits:].any()
    llr[cw == 1] *= np.float32(LANE_FACTOR)
    return llr
