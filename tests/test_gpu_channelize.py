"""The wideband front end on the device (k_channelize.hip behind ofdmrx_util_channelize) against the float64 model of
channelize_model.py: |got - v| <= tol on every component of every output, nothing exempt; the tolerance is
derived in the model's header.  Every output buffer is filled with a sentinel first and has spare columns and a spare row, which
must come back untouched.  Each test prints its worst |got - v| / tol (profiles/channelize_parity.txt keeps them)."""
import ctypes as C

import numpy as np
import pytest

import channelize_model as CM

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
ALL_D = (2, 3, 6, 32)
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


def centres_for(D, n, rate=8000, seed=0):
    """an arbitrary centre first, then 0, +-Rw / 2, +-1e-3 Hz, then arbitrary ones"""
    rw = float(D * rate)
    rng = np.random.default_rng(100 * D + seed)
    arb = rng.uniform(-rw / 2, rw / 2, size=max(n, 6))
    f = np.concatenate([arb[:1], [0.0, rw / 2, -rw / 2, 1e-3, -1e-3], arb[1:]])
    return f[:n].copy()


def _run(rx, pcm, D, centres, in_first=0, out_first=0, n_out=None, spare=3, d_in=None):
    """-> [C, n_out, 2] float32 from the device; checks the spare columns and the spare row"""
    import torch
    pcm = np.ascontiguousarray(pcm)
    if n_out is None:
        n_out = CM.n_outputs(in_first + len(pcm), D) - out_first
    Cn = len(centres)
    out = torch.full((Cn + 1, n_out + spare, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    d_in = _dev(pcm) if d_in is None else d_in
    torch.cuda.synchronize()                                         # the handle has a stream of its own
    rx.channelize(d_in.data_ptr(), FMT[pcm.dtype], in_first, len(pcm), D, centres, out_first, n_out, out.data_ptr(), n_out + spare)
    rx.synchronize()
    got = out.cpu().numpy()
    assert (got[Cn] == SENTINEL).all() and (got[:, n_out:] == SENTINEL).all()
    return got[:Cn, :n_out]


def _check(rx, pcm, D, centres, what, rate=8000, **kw):
    got = _run(rx, pcm, D, centres, **kw)
    v, tol, tie = CM.channelize(pcm, D, centres, rate, out_first=kw.get("out_first", 0), n_out=kw.get("n_out"), in_first=kw.get("in_first", 0))
    assert tie > 1e-6, (what, tie)                                   # device and model cannot round an increment apart
    assert got.shape[:2] == v.shape and np.isfinite(got).all()
    w = CM.worst(got, v, tol)
    print("channelize D %d %s: %d channels x %d outputs, worst |got - v| / tol %.4f" % (D, what, v.shape[0], v.shape[1], w))
    assert w <= 1.0, (D, what, w)
    return got, w


def sizes(D):
    T = 24 * D + 1
    return (1, T - 1, T, T + 1, 256 * D - 1, 256 * D, 256 * D + 1, 3 * 256 * D + 5)


@pytest.mark.parametrize("n_channels", [1, 3, 65])
@pytest.mark.parametrize("D", ALL_D)
def test_shapes_match_model(rx, D, n_channels):
    """one sample, a filter length less one, exactly, plus one, a tile of 256 outputs less a sample, exactly, plus one, three tiles and
    five samples; one channel, three (part of a workgroup's four), 65 (sixteen workgroups and one channel)"""
    f = centres_for(D, n_channels)
    worst = 0.0
    for n_in in sizes(D):
        pcm = CM.random_pcm(n_in, np.int16, seed=n_in)
        worst = max(worst, _check(rx, pcm, D, f, "n_in %d" % n_in)[1])
    print("channelize D %d, %d channels, all sizes: worst %.4f" % (D, n_channels, worst))


@pytest.mark.parametrize("D", ALL_D)
def test_formats(rx, D):
    """U8 and F32 input; F32 input scaled by 2^12 gives exactly the scaled outputs"""
    n_in = 3 * 256 * D + 5
    f = centres_for(D, 3, seed=1)
    _check(rx, CM.random_pcm(n_in, np.uint8, seed=2), D, f, "u8")
    x = CM.random_pcm(n_in, np.float32, seed=3)
    got, _ = _check(rx, x, D, f, "f32")
    big, _ = _check(rx, x * np.float32(4096.0), D, f, "f32 x 4096")
    assert (big == got * np.float32(4096.0)).all()


@pytest.mark.parametrize("D", ALL_D)
def test_positions(rx, D):
    """a buffer that starts inside the stream: the first output whose history it holds, and outputs at wideband positions just
    below 2^32, just above it, and at 2^40"""
    T = 24 * D + 1
    f = centres_for(D, 3, seed=2)
    n_out = 300
    in_first = 1000 * D + 1
    out_first = -(-(in_first + T - 1) // D)
    pcm = CM.random_pcm((out_first + n_out - 1) * D - in_first + 1, np.int16, seed=4)
    _check(rx, pcm, D, f, "in_first %d out_first %d" % (in_first, out_first), in_first=in_first, out_first=out_first, n_out=n_out)
    for pos in (2 ** 32 - 3 * D, 2 ** 32 + D, 2 ** 40):
        out_first = pos // D                                         # (the multiple of D at or just below it)
        in_first = out_first * D - (T - 1)
        pcm = CM.random_pcm((n_out - 1) * D + T + 2, np.int16, seed=5)
        _check(rx, pcm, D, f, "out_first D = %d" % pos, in_first=in_first, out_first=out_first, n_out=n_out)


def test_a_48_khz_handle(rx48):
    """the handle's rate enters the wideband rate, and with it the phase increments"""
    D = 3
    f = centres_for(D, 5, rate=48000, seed=3)
    _check(rx48, CM.random_pcm(2 * 256 * D + 11, np.int16, seed=6), D, f, "48 kHz", rate=48000)


@pytest.mark.parametrize("D", ALL_D)
def test_blocks_are_byte_identical(rx, D):
    """one call over a capture of 5 x 256 D + 17 samples against the same capture arriving in blocks of 4097, 1, D - 1 and 0 samples,
    each call reading the block's outputs from the samples so far with T - 1 samples of history"""
    import torch
    T = 24 * D + 1
    W = 5 * 256 * D + 17
    f = centres_for(D, 3, seed=4)
    pcm = CM.random_pcm(W, np.int16, seed=7)
    whole, _ = _check(rx, pcm, D, f, "whole capture")
    n_all = CM.n_outputs(W, D)
    d_in = _dev(pcm)
    out = torch.full((3, n_all + 2, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    fed, calls, blocks = 0, 0, [1, 4097, D - 1, 0]
    while fed < W:
        for b in blocks:
            new = min(fed + b, W)
            o0, o1 = CM.n_outputs(fed, D), CM.n_outputs(new, D)
            fed = new
            if o1 == o0:
                continue
            i0 = max(0, o0 * D - (T - 1))
            rx.channelize(d_in.data_ptr() + 4 * i0, 0, i0, fed - i0, D, f, o0, o1 - o0, out.data_ptr() + 8 * o0, n_all + 2)
            calls += 1
    rx.synchronize()
    got = out.cpu().numpy()
    assert calls >= 2 and (got[:, n_all:] == SENTINEL).all()
    assert got[:, :n_all].tobytes() == whole.tobytes()


def test_refusals_leave_the_output_untouched(rx):
    """every argument the header names is refused with OFDMRX_E_ARG before anything runs; buffers that merely touch are accepted"""
    import torch
    D, W = 6, 4096
    T = 24 * D + 1
    n_out = CM.n_outputs(W, D)
    buf = torch.full((W * 4 + 2 * 2 * (n_out + 1) * 4 + 64,), 77, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    assert base % 8 == 0
    d_in, d_out = base, base + 4 * W                                 # the input right before the output
    pcm = CM.random_pcm(W, np.int16, seed=8)
    buf[:4 * W] = _dev(pcm.view(np.uint8).reshape(-1))
    before = buf.clone()
    torch.cuda.synchronize()
    f = np.array([1000.0, -2000.0], np.float64)
    pf = f.ctypes.data_as(C.c_void_p)

    def call(d_in=d_in, fmt=0, in_first=0, n_in=W, decim=D, centres=pf, n_ch=2, out_first=0, n_out=n_out, d_out=d_out, stride=n_out + 1):
        return rx._lib.ofdmrx_util_channelize(rx._h, d_in, fmt, in_first, n_in, decim, centres, n_ch, out_first, n_out, d_out, stride)

    assert call(d_in=None) == -1 and call(d_out=None) == -1 and call(centres=None) == -1      # NULL pointers
    assert call(n_in=0) == -1 and call(n_out=0) == -1 and call(n_ch=0) == -1                 # zero counts
    assert call(n_ch=65536) == -1
    assert call(decim=1) == -1 and call(decim=33) == -1 and call(decim=0) == -1
    assert call(fmt=-1) == -1 and call(fmt=3) == -1
    assert call(in_first=-1) == -1 and call(out_first=-1) == -1
    assert call(stride=n_out - 1) == -1
    for bad in (float("nan"), float("inf"), -float("inf"), 24000.001, -24000.001):           # |f_c| <= Rw / 2 = 24000
        g = np.array([1000.0, bad], np.float64)
        assert call(centres=g.ctypes.data_as(C.c_void_p)) == -1, bad
    assert call(n_out=n_out + 1) == -1                                # the last output needs a position behind the buffer
    assert call(n_in=W - 5, n_out=n_out) == -1
    assert call(in_first=1, n_in=W - 1, out_first=24, n_out=100) == -1        # history: 24 D - (T - 1) = 0 lies below in_first = 1
    assert call(in_first=D, n_in=W - D, out_first=24, n_out=100) == -1
    for off in (8, 4 * W - 8, -8, -(2 * n_out + 1) * 8 + 8):                  # the output overlaps the input, from either side
        assert call(d_out=d_in + off) == -1, off
    assert call(d_in=d_in + 2) == -1 and call(d_out=d_out + 4) == -1          # off the sample-frame boundary / off 8 bytes
    rx.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    assert call(in_first=D, n_in=W - D, out_first=25, n_out=100, d_in=d_in + 4 * D) == 0     # 25 D - (T - 1) = D: just inside
    assert call() == 0                                                # adjacent buffers (the same stream: it runs second)
    rx.synchronize()
    assert torch.equal(buf[:4 * W], before[:4 * W])
    got = buf[4 * W:4 * W + 2 * (n_out + 1) * 8].cpu().numpy().view(np.float32).reshape(2, n_out + 1, 2)
    v, tol, _ = CM.channelize(pcm, D, f)
    assert CM.worst(got[:, :n_out], v, tol) <= 1.0
    assert (got[:, n_out:].view(np.uint8) == 77).all() and (buf[4 * W + 2 * (n_out + 1) * 8:] == 77).all()
