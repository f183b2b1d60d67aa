"""The wideband front end at a rational decimation on the device (k_rechannelize in k_channelize.hip, behind
ofdmrx_util_channelize_ratio) against the float64 model of rechannelize_model.py: |got - v| <= tol on every
component of every output, nothing exempt; the tolerance is derived in the model's header.  Every output buffer is filled with a
sentinel first and has spare columns and a spare row, which must come back untouched.  Each test prints its worst |got - v| / tol
(profiles/rechannelize_parity.txt keeps them)."""
import ctypes as C

import numpy as np
import pytest

import channelize_tile as CT
import rechannelize_model as RM

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
RATIOS_8K = ((5, 2), (33, 16), (25, 4), (125, 4), (511, 16))
SLOT_RATIOS = ((49, 2), (472, 15))                                  # k_rechannelize<.., NP> at NP = 3 and NP = 1: no ratio above selects them
FMT = {np.dtype(np.int16): 0, np.dtype(np.uint8): 1, np.dtype(np.float32): 2}


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1)
    yield r
    r.close()


@pytest.fixture(scope="module")
def rx48():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1, sample_rate=48000)
    yield r
    r.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def tile_of(P, Q):
    """the outputs of one workgroup's tile (k_channelize.hip: rechannelize_shape), for a span of float2"""
    return CT.tile_shape(P, Q, 8)[0]


def samples_for(n, P, Q):
    """the shortest capture that gives n outputs: its last sample is the last one output n - 1 reads"""
    return (n - 1) * P // Q + 1


def centres_for(P, Q, n, rate=8000, seed=0):
    """an arbitrary centre first, then 0, +-Rw / 2, +-1e-3 Hz, then arbitrary ones"""
    rw = RM.wide_rate(rate, P, Q)
    rng = np.random.default_rng(100 * P + Q + seed)
    arb = rng.uniform(-rw / 2, rw / 2, size=max(n, 6))
    f = np.concatenate([arb[:1], [0.0, rw / 2, -rw / 2, 1e-3, -1e-3], arb[1:]])
    return f[:n].copy()


def _run(rx, pcm, P, Q, centres, in_first=0, out_first=0, n_out=None, spare=3):
    """-> [C, n_out, 2] float32 from the device; checks the spare columns and the spare row"""
    import torch
    pcm = np.ascontiguousarray(pcm)
    if n_out is None:
        n_out = RM.n_outputs(in_first + len(pcm), P, Q) - out_first
    Cn = len(centres)
    out = torch.full((Cn + 1, n_out + spare, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    d_in = _dev(pcm)
    torch.cuda.synchronize()                                         # the handle has a stream of its own
    rx.channelize(d_in.data_ptr(), FMT[pcm.dtype], in_first, len(pcm), (P, Q), centres, out_first, n_out, out.data_ptr(), n_out + spare)
    rx.synchronize()
    got = out.cpu().numpy()
    assert (got[Cn] == SENTINEL).all() and (got[:, n_out:] == SENTINEL).all()
    return got[:Cn, :n_out]


def _check(rx, pcm, P, Q, centres, what, rate=8000, **kw):
    got = _run(rx, pcm, P, Q, centres, **kw)
    v, tol, tie = RM.channelize(pcm, P, Q, centres, rate, out_first=kw.get("out_first", 0), n_out=kw.get("n_out"), in_first=kw.get("in_first", 0))
    assert tie > 1e-6, (what, tie)                                   # device and model cannot round an increment apart
    assert got.shape[:2] == v.shape and np.isfinite(got).all()
    w = RM.worst(got, v, tol)
    print("rechannelize %d/%d %s: %d channels x %d outputs, worst |got - v| / tol %.4f" % (P, Q, what, v.shape[0], v.shape[1], w))
    assert w <= 1.0, (P, Q, what, w)
    return got, w


def sizes(P, Q):
    T, tile = 24 * P // Q + 1, tile_of(P, Q)
    return (1, T - 1, T, T + 1, samples_for(tile - 1, P, Q), samples_for(tile, P, Q), samples_for(tile + 1, P, Q),
            samples_for(3 * tile + 5, P, Q))


def test_tiles_of_the_tested_ratios():
    """(the sizes below are cut around these; k_channelize.hip has the rule)"""
    assert [tile_of(P, Q) for P, Q in RATIOS_8K + ((64, 3),) + SLOT_RATIOS] == [256, 256, 256, 128, 112, 255, 192, 60]


@pytest.mark.parametrize("n_channels", [1, 3, 65])
@pytest.mark.parametrize("P,Q", RATIOS_8K)
def test_shapes_match_model(rx, P, Q, n_channels):
    """one sample, a filter length less one, exactly, plus one, a tile of outputs less one, exactly, plus one, three tiles and five
    outputs; one channel, three (part of a workgroup's four), 65 (sixteen workgroups and one channel)"""
    f = centres_for(P, Q, n_channels)
    worst = 0.0
    for n_in in sizes(P, Q):
        pcm = RM.random_pcm(n_in, np.int16, seed=n_in)
        worst = max(worst, _check(rx, pcm, P, Q, f, "n_in %d" % n_in)[1])
    print("rechannelize %d/%d, %d channels, all sizes: worst %.4f" % (P, Q, n_channels, worst))


@pytest.mark.parametrize("n_channels", [1, 3, 65])
def test_a_48_khz_handle(rx48, n_channels):
    """64/3 x 48 kHz = 1.024 MHz: the handle's rate enters the wideband rate, and with it the phase increments"""
    P, Q = 64, 3
    f = centres_for(P, Q, n_channels, rate=48000, seed=3)
    worst = 0.0
    for n_in in sizes(P, Q):
        pcm = RM.random_pcm(n_in, np.int16, seed=n_in)
        worst = max(worst, _check(rx48, pcm, P, Q, f, "48 kHz n_in %d" % n_in, rate=48000)[1])
    print("rechannelize %d/%d at 48 kHz, %d channels, all sizes: worst %.4f" % (P, Q, n_channels, worst))


def test_slots_per_lane_of_the_tested_ratios():
    """the k_rechannelize<.., NP> each ratio runs: 5/2 and 125/4 above at NP = 4 and 2, SLOT_RATIOS at NP = 3 and 1"""
    assert [CT.tile_shape(P, Q, 8)[1] for P, Q in ((5, 2), (125, 4)) + SLOT_RATIOS] == [4, 2, 3, 1]


@pytest.mark.parametrize("n_channels", [1, 5])
@pytest.mark.parametrize("P,Q", SLOT_RATIOS)
def test_three_and_one_slots_per_lane_match_model(rx, rx48, P, Q, n_channels):
    """49/2 (NP = 3, a tile of 192) and 472/15 (NP = 1, a tile of 60; on the 48 kHz handle, where its wideband rate is a whole
    number of hertz): a tile of outputs less one, exactly, plus one, three tiles and five; one channel and five (a second workgroup of
    one).  Then the longest capture in two blocks, cut inside its second tile, against the one call as bytes"""
    import torch
    r, rate = (rx48, 48000) if Q == 15 else (rx, 8000)
    T, tile = 24 * P // Q + 1, tile_of(P, Q)
    f = centres_for(P, Q, n_channels, rate=rate, seed=6)
    for n in (tile - 1, tile, tile + 1, 3 * tile + 5):
        pcm = RM.random_pcm(samples_for(n, P, Q), np.int16, seed=n)
        whole, _ = _check(r, pcm, P, Q, f, "%d outputs" % n, rate=rate)
    W, n_all = len(pcm), 3 * tile + 5
    assert whole.shape[1] == n_all
    d_in = _dev(pcm)
    out = torch.full((n_channels, n_all + 2, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    fed = 0
    for new in (samples_for(tile + tile // 3, P, Q), W):
        o0, o1 = RM.n_outputs(fed, P, Q), RM.n_outputs(new, P, Q)
        fed = new
        assert o1 > o0
        i0 = max(0, o0 * P // Q - (T - 1))
        r.channelize(d_in.data_ptr() + 4 * i0, 0, i0, fed - i0, (P, Q), f, o0, o1 - o0, out.data_ptr() + 8 * o0, n_all + 2)
    r.synchronize()
    got = out.cpu().numpy()
    assert (got[:, n_all:] == SENTINEL).all()
    assert got[:, :n_all].tobytes() == whole.tobytes()


@pytest.mark.parametrize("P,Q", RATIOS_8K)
def test_formats(rx, P, Q):
    """U8 and F32 input; F32 input scaled by 2^12 gives exactly the scaled outputs"""
    n_in = samples_for(3 * tile_of(P, Q) + 5, P, Q)
    f = centres_for(P, Q, 3, seed=1)
    _check(rx, RM.random_pcm(n_in, np.uint8, seed=2), P, Q, f, "u8")
    x = RM.random_pcm(n_in, np.float32, seed=3)
    got, _ = _check(rx, x, P, Q, f, "f32")
    big, _ = _check(rx, x * np.float32(4096.0), P, Q, f, "f32 x 4096")
    assert (big == got * np.float32(4096.0)).all()


@pytest.mark.parametrize("P,Q", RATIOS_8K)
def test_every_residue_first_and_last(rx, P, Q):
    """out_first sweeps Q consecutive values with a fixed count: every residue n mod Q is the first and the last output of a call,
    on a buffer that begins inside the stream with exactly the history the first output needs and ends on the last sample read"""
    T = 24 * P // Q + 1
    f = centres_for(P, Q, 3, seed=5)
    n_out = tile_of(P, Q) + Q + 3
    base = 7 * tile_of(P, Q) + 40
    for out_first in range(base, base + Q):
        in_first = out_first * P // Q - (T - 1)
        assert in_first > 0
        n_in = (out_first + n_out - 1) * P // Q - in_first + 1
        pcm = RM.random_pcm(n_in, np.int16, seed=out_first)
        _check(rx, pcm, P, Q, f, "out_first %d (residue %d)" % (out_first, out_first % Q), in_first=in_first, out_first=out_first, n_out=n_out)


@pytest.mark.parametrize("P,Q", RATIOS_8K)
def test_positions(rx, P, Q):
    """outputs whose wideband positions lie just below 2^32, just above it and above 2^40, each beginning on an output with
    n P no multiple of Q"""
    T = 24 * P // Q + 1
    f = centres_for(P, Q, 3, seed=2)
    n_out = 300
    for pos in (2 ** 32 - 3 * P, 2 ** 32 + P, 2 ** 40 + 12345):
        out_first = -(-pos * Q // P)
        while out_first * P % Q == 0:
            out_first += 1
        in_first = out_first * P // Q - (T - 1)
        pcm = RM.random_pcm((out_first + n_out - 1) * P // Q - in_first + 3, np.int16, seed=5)
        _check(rx, pcm, P, Q, f, "out_first %d (position %d)" % (out_first, out_first * P // Q), in_first=in_first, out_first=out_first, n_out=n_out)


@pytest.mark.parametrize("P,Q", RATIOS_8K)
def test_blocks_are_byte_identical(rx, P, Q):
    """one call over a capture against the same capture arriving in blocks of 1, 4097, P - 1 and 0 samples, each call reading the
    block's outputs from the samples so far with T - 1 samples of history"""
    import torch
    T = 24 * P // Q + 1
    W = samples_for(5 * tile_of(P, Q), P, Q) + 17
    f = centres_for(P, Q, 3, seed=4)
    pcm = RM.random_pcm(W, np.int16, seed=7)
    whole, _ = _check(rx, pcm, P, Q, f, "whole capture")
    n_all = RM.n_outputs(W, P, Q)
    d_in = _dev(pcm)
    out = torch.full((3, n_all + 2, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    fed, calls, blocks = 0, 0, [1, 4097, P - 1, 0]
    while fed < W:
        for b in blocks:
            new = min(fed + b, W)
            o0, o1 = RM.n_outputs(fed, P, Q), RM.n_outputs(new, P, Q)
            fed = new
            if o1 == o0:
                continue
            i0 = max(0, o0 * P // Q - (T - 1))
            rx.channelize(d_in.data_ptr() + 4 * i0, 0, i0, fed - i0, (P, Q), f, o0, o1 - o0, out.data_ptr() + 8 * o0, n_all + 2)
            calls += 1
    rx.synchronize()
    got = out.cpu().numpy()
    assert calls >= 2 and (got[:, n_all:] == SENTINEL).all()
    assert got[:, :n_all].tobytes() == whole.tobytes()


def test_a_reduced_q_of_1_is_the_integer_front_end(rx):
    """(12, 2), (6, 1) and a Fraction are ofdmrx_util_channelize at decim 6: the same bytes"""
    import fractions
    import torch
    W = 3 * 256 * 6 + 5
    pcm = RM.random_pcm(W, np.int16, seed=9)
    f = np.array([1234.5, -13000.0, 20000.0])
    n_out = RM.n_outputs(W, 6, 1)
    d_in = _dev(pcm)
    got = []
    for decim in (6, (12, 2), (6, 1), fractions.Fraction(18, 3)):
        out = torch.full((3, n_out, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        rx.channelize(d_in.data_ptr(), 0, 0, W, decim, f, 0, n_out, out.data_ptr())
        rx.synchronize()
        got.append(out.cpu().numpy().tobytes())
    assert got[1] == got[0] and got[2] == got[0] and got[3] == got[0]
    assert not (np.frombuffer(got[0], np.float32) == SENTINEL).any()


def test_refusals_leave_the_output_untouched(rx):
    """every argument the header names is refused with OFDMRX_E_ARG before anything runs; buffers that merely touch are accepted"""
    import torch
    P, Q, W = 25, 4, 4096
    T = 24 * P // Q + 1
    n_out = RM.n_outputs(W, P, Q)                                    # 656
    buf = torch.full((W * 4 + 2 * 2 * (n_out + 1) * 4 + 64,), 77, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    assert base % 8 == 0
    d_in, d_out = base, base + 4 * W                                 # the input right before the output
    pcm = RM.random_pcm(W, np.int16, seed=8)
    buf[:4 * W] = _dev(pcm.view(np.uint8).reshape(-1))
    before = buf.clone()
    torch.cuda.synchronize()
    f = np.array([1000.0, -2000.0], np.float64)
    pf = f.ctypes.data_as(C.c_void_p)

    def call(d_in=d_in, fmt=0, in_first=0, n_in=W, p=P, q=Q, centres=pf, n_ch=2, out_first=0, n_out=n_out, d_out=d_out, stride=n_out + 1):
        return rx._lib.ofdmrx_util_channelize_ratio(rx._h, d_in, fmt, in_first, n_in, p, q, centres, n_ch, out_first, n_out, d_out, stride)

    for bad in ((0, 4), (25, 0), (-25, 4), (25, -4), (35, 17), (7, 4), (129, 4), (513, 16), (33, 1), (1, 1)):
        assert call(p=bad[0], q=bad[1]) == -1, bad                   # bad p / q, Q above 16, the ratio outside 2 .. 32
    assert call(d_in=None) == -1 and call(d_out=None) == -1 and call(centres=None) == -1      # NULL pointers
    assert call(n_in=0) == -1 and call(n_out=0) == -1 and call(n_ch=0) == -1                 # zero counts
    assert call(n_ch=65536) == -1
    assert call(fmt=-1) == -1 and call(fmt=3) == -1
    assert call(in_first=-1) == -1 and call(out_first=-1) == -1
    assert call(stride=n_out - 1) == -1
    for bad in (float("nan"), float("inf"), -float("inf"), 25000.001, -25000.001):           # |f_c| <= Rw / 2 = 25000
        g = np.array([1000.0, bad], np.float64)
        assert call(centres=g.ctypes.data_as(C.c_void_p)) == -1, bad
    assert call(n_out=n_out + 1) == -1                                # output 656 needs position 4100 of 4096
    assert call(n_in=W - 5, n_out=n_out) == -1                        # output 655 needs position 4093 of 4091
    assert call(in_first=1, n_in=W - 1, out_first=24, n_out=100) == -1        # history: 24 P div Q - (T - 1) = 0 lies below in_first = 1
    assert call(in_first=7, n_in=W - 7, out_first=25, n_out=100) == -1        # 25 P div Q - (T - 1) = 6 lies below in_first = 7
    for off in (8, 4 * W - 8, -8, -(2 * n_out + 1) * 8 + 8):                  # the output overlaps the input, from either side
        assert call(d_out=d_in + off) == -1, off
    assert call(d_in=d_in + 2) == -1 and call(d_out=d_out + 4) == -1          # off the sample-frame boundary / off 8 bytes
    rx.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    assert call(in_first=6, n_in=W - 6, out_first=25, n_out=100, d_in=d_in + 4 * 6) == 0     # 25 P div Q - (T - 1) = 6: just inside
    assert call() == 0                                                # adjacent buffers (the same stream: it runs second)
    rx.synchronize()
    assert torch.equal(buf[:4 * W], before[:4 * W])
    got = buf[4 * W:4 * W + 2 * (n_out + 1) * 8].cpu().numpy().view(np.float32).reshape(2, n_out + 1, 2)
    v, tol, _ = RM.channelize(pcm, P, Q, f)
    assert RM.worst(got[:, :n_out], v, tol) <= 1.0
    assert (got[:, n_out:].view(np.uint8) == 77).all() and (buf[4 * W + 2 * (n_out + 1) * 8:] == 77).all()


def test_one_handle_serves_integer_and_ratio_calls_in_turn(rx):
    """the handle keeps ONE set of front-end parameters, keyed by the reduced (p, q) and the increments: D = 5 and 5/2 share p, and
    10/4 must meet 5/2's.  Integer and ratio calls alternate on one handle, with the same centres, other centres and fewer of them;
    every output equals, byte for byte, the same call on a second handle on which a call at 64/3 precedes it - so that handle uploads
    its parameters anew every time.  4096 samples give 820 outputs at D = 5, 1639 at 5/2 and 656 at 25/4: more than one tile each;
    three channels leave a workgroup partly filled"""
    import modem_amd
    import torch
    W = 4096
    pcm = RM.random_pcm(W, np.int16, seed=11)
    d_in = _dev(pcm)
    f = np.array([1234.5, -9000.0, 10000.0])                         # inside +-10 kHz, half the wideband rate of 5/2
    g = np.array([-3333.25, 0.0, 7000.125])
    calls = ((5, f), ((5, 2), f), (5, f), ((5, 2), f), ((5, 2), g), ((5, 2), g[:2]), ((25, 4), f), ((10, 4), f))
    assert [RM.n_outputs(W, 5, 1), RM.n_outputs(W, 5, 2), RM.n_outputs(W, 25, 4)] == [820, 1639, 656]
    assert tile_of(5, 2) < 1639 and tile_of(25, 4) < 656 and 256 < 820

    def run(r, decim, centres):
        P, Q = decim if isinstance(decim, tuple) else (decim, 1)
        n_out = RM.n_outputs(W, P, Q)
        out = torch.full((len(centres), n_out, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        r.channelize(d_in.data_ptr(), 0, 0, W, decim, centres, 0, n_out, out.data_ptr())
        r.synchronize()
        return out.cpu().numpy()

    ref = modem_amd.Receiver(device=0, chunk_frames=1)
    try:
        for k, (decim, centres) in enumerate(calls):
            run(ref, (64, 3), f)
            want = run(ref, decim, centres)
            got = run(rx, decim, centres)
            assert not (want == SENTINEL).any(), (k, decim)
            assert got.tobytes() == want.tobytes(), (k, decim)
    finally:
        ref.close()
