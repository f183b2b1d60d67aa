"""The wideband front end for a real capture on the device (k_channelize.hip's kernels instantiated for a real capture, behind
ofdmrx_util_channelize_real) against the float64 model of channelize_real_model.py: |got - v| <= tol on every
component of every output, nothing exempt; the tolerance is derived in the model's header.  And as bytes: against twice the analytic
entries on the same samples with a +0 imaginary part, blocks against one call, calls in turn on one handle.  Every output buffer is
filled with a sentinel first and has spare columns and a spare row, which must come back untouched.

The launch has one shape at every integer D (a tile of 256 outputs; k_channelize.hip: channelize_outputs_per_lane), so there is no D
at which it changes: D = 16 and 17 are here because the ANALYTIC instantiation the bytes are compared with changes its tile between
them."""
import ctypes as C
import fractions

import numpy as np
import pytest

import channelize_real_model as XM
import channelize_tile as CT

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
RATE = 8000
INTEGER = ((2, 1), (6, 1), (16, 1), (17, 1), (32, 1))
FRACTIONAL = ((25, 4), (64, 3), (125, 16))
RATIOS = INTEGER + FRACTIONAL
SLOT_RATIOS = ((49, 2), (472, 15))                                  # here 4 slots per lane, 3 and 1 in the analytic kernel compared with
FMT = {np.dtype(np.int16): 0, np.dtype(np.uint8): 1, np.dtype(np.float32): 2}


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1)
    yield r
    r.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def tile_of(P, Q):
    """the outputs of one workgroup's tile for a span of float: 256 at an integer D, Q M at a ratio (k_channelize.hip:
    rechannelize_shape)"""
    return CT.tile_shape(P, Q, 4)[0]


def samples_for(n, P, Q):
    """the shortest capture that gives n outputs: its last sample is the last one output n - 1 reads"""
    return (n - 1) * P // Q + 1


def centres_for(P, Q, n, seed=0):
    """both edges of the rule (admitted, of either sign), then arbitrary centres inside it of either sign"""
    lo, hi = XM.centre_edges(RATE, P, Q)
    rng = np.random.default_rng(100 * P + Q + seed)
    arb = rng.uniform(lo, hi, size=max(n, 4)) * rng.choice([-1.0, 1.0], size=max(n, 4))
    return np.concatenate([arb[:1], [lo, -hi], arb[1:]])[:n].copy()


def _call(rx, x, P, Q, centres, in_first=0, out_first=0, n_out=None, spare=3, real=True):
    """-> [C, n_out, 2] float32 from the device.  real: x [W] through channelize_real; else x [W, 2] through channelize, doubled on
    the device.  Checks the spare columns and the spare row"""
    import torch
    x = np.ascontiguousarray(x)
    if n_out is None:
        n_out = XM.n_outputs(in_first + len(x), P, Q) - out_first
    Cn = len(centres)
    out = torch.full((Cn + 1, n_out + spare, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    d_in = _dev(x)
    torch.cuda.synchronize()                                         # the handle has a stream of its own
    decim = P if Q == 1 else (P, Q)
    f = rx.channelize_real if real else rx.channelize
    f(d_in.data_ptr(), FMT[x.dtype], in_first, len(x), decim, centres, out_first, n_out, out.data_ptr(), n_out + spare)
    rx.synchronize()
    got = out.cpu().numpy()
    assert (got[Cn] == SENTINEL).all() and (got[:, n_out:] == SENTINEL).all()
    if not real:
        got = (2.0 * out[:Cn, :n_out]).cpu().numpy()                 # the doubling, in torch
        return got
    return got[:Cn, :n_out]


def _check(rx, x, P, Q, centres, what, **kw):
    """the device against the model, and against twice the analytic entry as bytes"""
    got = _call(rx, x, P, Q, centres, **kw)
    v, tol, tie = XM.channelize(x, P, Q, centres, RATE, out_first=kw.get("out_first", 0), n_out=kw.get("n_out"), in_first=kw.get("in_first", 0))
    assert tie > 1e-6, (what, tie)
    assert got.shape[:2] == v.shape and np.isfinite(got).all()
    w = XM.worst(got, v, tol)
    print("channelize_real %d/%d %s: %d channels x %d outputs, worst |got - v| / tol %.4f" % (P, Q, what, v.shape[0], v.shape[1], w))
    assert w <= 1.0, (P, Q, what, w)
    twice = _call(rx, XM.with_zero_imag(x), P, Q, centres, real=False, **kw)
    assert got.tobytes() == twice.tobytes(), (P, Q, what)
    return got, w


def test_tiles_of_the_tested_ratios():
    """(the sizes below are cut around these)"""
    assert [tile_of(P, Q) for P, Q in RATIOS + SLOT_RATIOS] == [256, 256, 256, 256, 256, 256, 255, 256, 256, 255]


@pytest.mark.parametrize("n_channels", [1, 4, 5])
@pytest.mark.parametrize("P,Q", RATIOS + SLOT_RATIOS)
def test_shapes_match_model(rx, P, Q, n_channels):
    """one output, a tile less one, a tile, a tile and one; one channel, four (a workgroup's waves), five (a second group of one).
    At SLOT_RATIOS the bytes compared are those of the analytic kernel at 3 and at 1 slots per lane"""
    f = centres_for(P, Q, n_channels)
    tile = tile_of(P, Q)
    for n in (1, tile - 1, tile, tile + 1):
        x = XM.random_real(samples_for(n, P, Q), np.int16, seed=n)
        _check(rx, x, P, Q, f, "%d outputs" % n)


@pytest.mark.parametrize("P,Q", [(6, 1), (32, 1), (25, 4), (125, 16)])
def test_positions(rx, P, Q):
    """a first output at 0, 1, P - 1, P, P + 1 and 2^40 + 3: from position 0 while its history reaches below it, else from inside the
    stream with exactly the T - 1 samples of history the first output needs - and one fewer is refused"""
    import torch
    T = 24 * P // Q + 1
    f = centres_for(P, Q, 3, seed=2)
    n_out = 70
    for out_first in (0, 1, P - 1, P, P + 1, 2 ** 40 + 3):
        in_first = max(0, out_first * P // Q - (T - 1))
        n_in = (out_first + n_out - 1) * P // Q - in_first + 1
        x = XM.random_real(n_in, np.int16, seed=out_first % 1000)
        _check(rx, x, P, Q, f, "out_first %d" % out_first, in_first=in_first, out_first=out_first, n_out=n_out)
        if in_first > 0:
            d_in = _dev(x)
            out = torch.full((3, n_out, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            r = rx._lib.ofdmrx_util_channelize_real(rx._h, d_in.data_ptr() + 2, 0, in_first + 1, n_in - 1, P, Q, f.ctypes.data_as(C.c_void_p), 3,
                                                    out_first, n_out, out.data_ptr(), n_out)
            rx.synchronize()
            assert r == -1 and (out == SENTINEL).all().item()


@pytest.mark.parametrize("P,Q", [(6, 1), (25, 4)])
def test_formats(rx, P, Q):
    """U8 and F32 input; F32 input scaled by 2^12 gives exactly the scaled outputs"""
    n_in = samples_for(tile_of(P, Q) + 5, P, Q)
    f = centres_for(P, Q, 3, seed=1)
    _check(rx, XM.random_real(n_in, np.uint8, seed=2), P, Q, f, "u8")
    x = XM.random_real(n_in, np.float32, seed=3)
    got, _ = _check(rx, x, P, Q, f, "f32")
    big, _ = _check(rx, x * np.float32(4096.0), P, Q, f, "f32 x 4096")
    assert (big == got * np.float32(4096.0)).all()


@pytest.mark.parametrize("P,Q", [(6, 1), (17, 1), (25, 4), (64, 3)])
def test_three_unequal_blocks_are_byte_identical(rx, P, Q):
    """one call over a capture against the same capture in three unequal blocks, each call reading the block's outputs from the
    samples so far with T - 1 samples of history"""
    import torch
    T = 24 * P // Q + 1
    W = samples_for(2 * tile_of(P, Q), P, Q) + 17
    f = centres_for(P, Q, 3, seed=4)
    x = XM.random_real(W, np.int16, seed=7)
    whole = _call(rx, x, P, Q, f)
    n_all = XM.n_outputs(W, P, Q)
    d_in = _dev(x)
    out = torch.full((3, n_all + 2, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    fed, calls = 0, 0
    for b in (T + 3, W // 3 + 1, W):
        new = min(fed + b, W)
        o0, o1 = XM.n_outputs(fed, P, Q), XM.n_outputs(new, P, Q)
        fed = new
        assert o1 > o0
        i0 = max(0, o0 * P // Q - (T - 1))
        rx.channelize_real(d_in.data_ptr() + 2 * i0, 0, i0, fed - i0, (P, Q), f, o0, o1 - o0, out.data_ptr() + 8 * o0, n_all + 2)
        calls += 1
    rx.synchronize()
    got = out.cpu().numpy()
    assert fed == W and calls == 3 and (got[:, n_all:] == SENTINEL).all()
    assert got[:, :n_all].tobytes() == whole.tobytes()


def test_a_reduced_q_of_1_runs_the_integer_kernel(rx):
    """3/1, 6/2 and a Fraction through the one entry: the bytes of twice ofdmrx_util_channelize at D = 3"""
    W = 3 * 256 * 3 + 5
    x = XM.random_real(W, np.int16, seed=9)
    f = np.array([2234.5, -9000.0, 10000.0])                         # inside 2000 .. 10000 Hz
    want = _call(rx, XM.with_zero_imag(x), 3, 1, f, real=False)
    import torch
    n_out = XM.n_outputs(W, 3, 1)
    d_in = _dev(x)
    for decim in (3, (3, 1), (6, 2), fractions.Fraction(9, 3)):
        out = torch.full((3, n_out, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        rx.channelize_real(d_in.data_ptr(), 0, 0, W, decim, f, 0, n_out, out.data_ptr())
        rx.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes(), decim
    assert not (want == SENTINEL).any()


def test_a_negative_centre_is_the_conjugate_of_the_positive_one(rx):
    """within tolerance only (the two chains round apart): y_{-f} = conj y_{+f}"""
    for P, Q in ((6, 1), (25, 4)):
        x = XM.random_real(samples_for(300, P, Q), np.int16, seed=13)
        f = np.array([7000.5, -7000.5])
        got = _call(rx, x, P, Q, f)
        _, tol, _ = XM.channelize(x, P, Q, f, RATE)
        assert (np.abs(got[0, :, 0] - got[1, :, 0]) <= tol[0] + tol[1]).all()
        assert (np.abs(got[0, :, 1] + got[1, :, 1]) <= tol[0] + tol[1]).all()
        assert np.abs(got[0, 24:, 1]).max() > 100 * tol.max()        # (the imaginary parts are not nothing)


def test_one_handle_serves_real_and_analytic_calls_in_turn(rx):
    """the handle keeps ONE set of taps and increments, keyed by the reduced (p, q) and the increments, and the real entry shares it
    with the analytic ones.  Real and analytic calls alternate across ratios, centres and channel counts on one handle; every output
    equals, byte for byte, the same call on a second handle on which a call at 64/3 precedes it - that handle uploads anew every time"""
    import modem_amd
    W = 4096
    x = XM.random_real(W, np.int16, seed=11)
    two = XM.with_zero_imag(x)
    f = np.array([2234.5, -9000.0, 9500.0])                          # inside 2000 .. 8000 Hz of 5/2's rule
    f = np.clip(np.abs(f), 2000.0, 8000.0) * np.sign(f)
    g = np.array([-3333.25, 2000.0, 7000.125])
    calls = ((True, 5, 1, f), (False, 5, 1, f), (True, 5, 2, f), (False, 5, 2, f), (True, 5, 2, g), (True, 5, 2, g[:2]), (False, 5, 2, g[:2]),
             (True, 25, 4, f), (True, 10, 4, f), (True, 5, 1, f))
    ref = modem_amd.Receiver(device=0, chunk_frames=1)
    try:
        for k, (real, P, Q, centres) in enumerate(calls):
            src = x if real else two
            _call(ref, src, 64, 3, f, real=real)
            Pr, Qr = (P // 2, Q // 2) if (P, Q) == (10, 4) else (P, Q)
            want = _call(ref, src, P, Q, centres, real=real, n_out=XM.n_outputs(W, Pr, Qr))
            got = _call(rx, src, P, Q, centres, real=real, n_out=XM.n_outputs(W, Pr, Qr))
            assert not (want == SENTINEL).any(), k
            assert got.tobytes() == want.tobytes(), (k, real, P, Q)
    finally:
        ref.close()


def test_refusals_leave_the_output_untouched(rx):
    """every argument the header names is refused with OFDMRX_E_ARG before anything runs; the centre rule's edges are admitted and one
    ulp beyond them refused; buffers that merely touch are accepted"""
    import torch
    P, Q, W = 25, 4, 4096
    T = 24 * P // Q + 1
    n_out = XM.n_outputs(W, P, Q)                                    # 656
    buf = torch.full((W * 2 + 2 * 2 * (n_out + 1) * 4 + 64,), 77, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    assert base % 8 == 0
    d_in, d_out = base, base + 2 * W                                 # the input right before the output
    x = XM.random_real(W, np.int16, seed=8)
    buf[:2 * W] = _dev(x.view(np.uint8).reshape(-1))
    before = buf.clone()
    torch.cuda.synchronize()
    f = np.array([3000.0, -5000.0], np.float64)
    pf = f.ctypes.data_as(C.c_void_p)

    def call(d_in=d_in, fmt=0, in_first=0, n_in=W, p=P, q=Q, centres=pf, n_ch=2, out_first=0, n_out=n_out, d_out=d_out, stride=n_out + 1):
        return rx._lib.ofdmrx_util_channelize_real(rx._h, d_in, fmt, in_first, n_in, p, q, centres, n_ch, out_first, n_out, d_out, stride)

    def centre(v, **kw):
        g = np.array([3000.0, v], np.float64)
        return call(centres=g.ctypes.data_as(C.c_void_p), **kw)

    for bad in ((0, 4), (25, 0), (-25, 4), (25, -4), (35, 17), (7, 4), (129, 4), (513, 16), (33, 1), (1, 1)):
        assert call(p=bad[0], q=bad[1]) == -1, bad
    assert call(d_in=None) == -1 and call(d_out=None) == -1 and call(centres=None) == -1
    assert call(n_in=0) == -1 and call(n_out=0) == -1 and call(n_ch=0) == -1 and call(n_ch=65536) == -1
    assert call(fmt=-1) == -1 and call(fmt=3) == -1
    assert call(in_first=-1) == -1 and call(out_first=-1) == -1
    assert call(stride=n_out - 1) == -1
    lo, hi = XM.centre_edges(RATE, P, Q)                             # 2000 and 23000 Hz
    assert (lo, hi) == (2000.0, 23000.0)
    for bad in (float("nan"), float("inf"), -float("inf"), 0.0, 1999.0, -1999.0, 24000.0, -25000.0, 25000.001,
                np.nextafter(lo, 0.0), -np.nextafter(lo, 0.0), np.nextafter(hi, np.inf), -np.nextafter(hi, np.inf)):
        assert centre(bad) == -1, bad
        assert not XM.centre_ok(bad, RATE, P, Q)
    assert centre(np.nextafter(2000.0, 0.0), p=6, q=1) == -1 and centre(np.nextafter(22000.0, np.inf), p=6, q=1) == -1   # (D = 6: the same rule)
    assert call(n_out=n_out + 1) == -1                                # output 656 needs position 4100 of 4096
    assert call(n_in=W - 5, n_out=n_out) == -1                        # output 655 needs position 4093 of 4091
    assert call(in_first=1, n_in=W - 1, out_first=24, n_out=100) == -1        # history: 24 P div Q - (T - 1) = 0 lies below in_first = 1
    assert call(in_first=7, n_in=W - 7, out_first=25, n_out=100) == -1        # 25 P div Q - (T - 1) = 6 lies below in_first = 7
    for off in (8, 2 * W - 8, -8, -(2 * n_out + 1) * 8 + 8):                  # the output overlaps the input, from either side
        assert call(d_out=d_in + off) == -1, off
    assert call(d_in=d_in + 1) == -1 and call(d_out=d_out + 4) == -1          # off the sample's boundary / off 8 bytes
    assert call(fmt=2, d_in=d_in + 2, n_in=W // 2 - 1, n_out=100) == -1       # F32: 2 bytes off
    bank = rx.wideband_real_bank(f, (P, Q))                          # while a bank is open
    try:
        assert call() == -1
    finally:
        bank.end()
    rx.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    for good in (lo, -lo, hi, -hi, np.nextafter(lo, np.inf), -np.nextafter(hi, 0.0)):
        assert centre(good) == 0, good
        assert XM.centre_ok(good, RATE, P, Q)
    assert call(in_first=6, n_in=W - 6, out_first=25, n_out=100, d_in=d_in + 2 * 6) == 0     # 25 P div Q - (T - 1) = 6: just inside
    assert call(fmt=1, d_in=d_in + 1, n_in=2 * W - 1, n_out=100) == 0         # U8: any byte is a sample's boundary
    assert call() == 0                                                # adjacent buffers (the same stream: it runs last)
    rx.synchronize()
    assert torch.equal(buf[:2 * W], before[:2 * W])
    got = buf[2 * W:2 * W + 2 * (n_out + 1) * 8].cpu().numpy().view(np.float32).reshape(2, n_out + 1, 2)
    v, tol, _ = XM.channelize(x, P, Q, f, RATE)
    assert XM.worst(got[:, :n_out], v, tol) <= 1.0
    assert (got[:, n_out:].view(np.uint8) == 77).all() and (buf[2 * W + 2 * (n_out + 1) * 8:] == 77).all()
