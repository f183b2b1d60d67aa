"""The grid front end on the device (k_channelize_grid.hip behind ofdmrx_util_channelize_grid) against the float64 model of
channelize_grid_model.py: |got - v| <= tol on every component of every output, nothing exempt; the tolerance
is derived in the model's header.  Every output buffer is filled with a sentinel first and has spare columns and a spare row, which
must come back untouched.  Each test prints its worst |got - v| / tol (profiles/channelize_grid_parity.txt keeps them)."""
import ctypes as C

import numpy as np
import pytest

import channelize_grid_model as G
import channelize_model as CM

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
DS = (2, 4, 32, 64, 512)          # M = 4; 8; 64: one point per lane of a wave; the first D the plain entries refuse; M = 1024
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


def tile(D):
    """the kernel's tile of output times"""
    return max(8, 4096 // (2 * D))


def subset(D):
    """the edge slots and the two about the centre, in a shuffled order"""
    return [-1, D - 1, -D, 0]


def _run(rx, pcm, D, slots, in_first=0, out_first=0, n_out=None, spare=3, d_in=None):
    """-> [n_slots, n_out, 2] float32 from the device; checks the spare columns and the spare row"""
    import torch
    pcm = np.ascontiguousarray(pcm)
    if n_out is None:
        n_out = G.n_outputs(in_first + len(pcm), D) - out_first
    n = 2 * D if slots is None else len(slots)
    out = torch.full((n + 1, n_out + spare, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    d_in = _dev(pcm) if d_in is None else d_in
    torch.cuda.synchronize()                                         # the handle has a stream of its own
    rx.channelize_grid(d_in.data_ptr(), FMT[pcm.dtype], in_first, len(pcm), D, slots, out_first, n_out, out.data_ptr(), n_out + spare)
    rx.synchronize()
    got = out.cpu().numpy()
    assert (got[n] == SENTINEL).all() and (got[:, n_out:] == SENTINEL).all()
    return got[:n, :n_out]


def _check(rx, pcm, D, slots, what, **kw):
    got = _run(rx, pcm, D, slots, **kw)
    v, tol = G.grid(pcm, D, slots, out_first=kw.get("out_first", 0), n_out=kw.get("n_out"), in_first=kw.get("in_first", 0))
    assert got.shape[:2] == v.shape and np.isfinite(got).all()
    w = G.worst(got, v, tol)
    print("channelize_grid D %d %s: %d slots x %d outputs, worst |got - v| / tol %.4f" % (D, what, v.shape[0], v.shape[1], w))
    assert w <= 1.0, (D, what, w)
    return got, w


@pytest.mark.parametrize("D", DS)
def test_shapes_match_model(rx, D):
    """from position 0 (the leading positions are zeros): 1, 63, 64, 65 outputs and one past the kernel's tile of times; all slots and
    the shuffled subset"""
    worst = 0.0
    for n_out in (1, 63, 64, 65, tile(D) + 1):
        pcm = G.random_pcm((n_out - 1) * D + 1, np.int16, seed=n_out)
        worst = max(worst, _check(rx, pcm, D, None, "n_out %d" % n_out, n_out=n_out)[1])
        worst = max(worst, _check(rx, pcm, D, subset(D), "n_out %d, subset" % n_out, n_out=n_out)[1])
    print("channelize_grid D %d, all sizes: worst %.4f" % (D, worst))


@pytest.mark.parametrize("D", DS)
def test_formats(rx, D):
    """U8 and F32 input; F32 input scaled by 2^12 gives exactly the scaled outputs"""
    n_in = (tile(D) + 70) * D + 5
    _check(rx, G.random_pcm(n_in, np.uint8, seed=2), D, None, "u8")
    x = G.random_pcm(n_in, np.float32, seed=3)
    got, _ = _check(rx, x, D, subset(D), "f32")
    big, _ = _check(rx, x * np.float32(4096.0), D, subset(D), "f32 x 4096")
    assert (big == got * np.float32(4096.0)).all()


@pytest.mark.parametrize("D", DS)
def test_positions(rx, D):
    """a buffer that starts inside the stream, holding exactly the history of its first output: out_first even, odd and 2^40 + 3"""
    T = 24 * D + 1
    n_out = 70
    for out_first in (1000, 1001, 2 ** 40 + 3):
        in_first = out_first * D - (T - 1)
        pcm = G.random_pcm((n_out - 1) * D + T + 2, np.int16, seed=5)
        _check(rx, pcm, D, None, "out_first %d" % out_first, in_first=in_first, out_first=out_first, n_out=n_out)
        _check(rx, pcm, D, subset(D), "out_first %d, subset" % out_first, in_first=in_first, out_first=out_first, n_out=n_out)


def test_blocks_are_byte_identical(rx):
    """D = 64: one call over a capture against the same capture arriving in blocks of 1, 4097, D - 1 and 0 samples, each call reading
    the block's outputs from the samples so far with T - 1 samples of history"""
    import torch
    D = 64
    T = 24 * D + 1
    W = 5 * 4097 + 17
    slots = subset(D) + [17]
    pcm = G.random_pcm(W, np.int16, seed=7)
    whole, _ = _check(rx, pcm, D, slots, "whole capture")
    n_all = G.n_outputs(W, D)
    d_in = _dev(pcm)
    out = torch.full((len(slots), n_all + 2, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    fed, calls, blocks = 0, 0, [1, 4097, D - 1, 0]
    while fed < W:
        for b in blocks:
            new = min(fed + b, W)
            o0, o1 = G.n_outputs(fed, D), G.n_outputs(new, D)
            fed = new
            if o1 == o0:
                continue
            i0 = max(0, o0 * D - (T - 1))
            rx.channelize_grid(d_in.data_ptr() + 4 * i0, 0, i0, fed - i0, D, slots, o0, o1 - o0, out.data_ptr() + 8 * o0, n_all + 2)
            calls += 1
    rx.synchronize()
    got = out.cpu().numpy()
    assert calls >= 2 and (got[:, n_all:] == SENTINEL).all()
    assert got[:, :n_all].tobytes() == whole.tobytes()


@pytest.mark.parametrize("D", [4, 32])
def test_against_the_plain_front_end(rx, D):
    """all slots against ofdmrx_util_channelize at grid_centres on the device: per component the difference is at most the sum of
    the two models' tolerances"""
    import modem_amd
    import torch
    pcm = G.random_pcm(300 * D + 3, np.int16, seed=11)
    n_out = G.n_outputs(len(pcm), D)
    grid = _run(rx, pcm, D, None)
    f = modem_amd.grid_centres(D, 8000)
    assert (f == G.centres(D)).all()
    out = torch.full((2 * D, n_out, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    d_in = _dev(pcm)
    torch.cuda.synchronize()
    rx.channelize(d_in.data_ptr(), 0, 0, len(pcm), D, f, 0, n_out, out.data_ptr())
    rx.synchronize()
    plain = out.cpu().numpy()
    _, tol_g = G.grid(pcm, D)
    _, tol_p, tie = CM.channelize(pcm, D, f)
    assert tie > 0.49
    d = np.abs(grid.astype(np.float64) - plain.astype(np.float64)).max(axis=2)
    w = float((d / (tol_g + tol_p)).max())
    print("channelize_grid D %d against channelize: worst |difference| / (tol + tol) %.4f" % (D, w))
    assert w <= 1.0


def test_grid_and_plain_tables_do_not_mix(rx):
    """a grid call, a plain call, a grid call and a plain call at the same D and the same centres: each equals its own first result
    as bytes (the device table's key tells a grid table from a plain one)"""
    import modem_amd
    import torch
    D = 8
    pcm = G.random_pcm(100 * D, np.int16, seed=13)
    n_out = G.n_outputs(len(pcm), D)
    slots = [3, -8, 0]
    f = modem_amd.grid_centres(D, 8000, slots)
    d_in = _dev(pcm)

    def plain():
        out = torch.full((3, n_out, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        rx.channelize(d_in.data_ptr(), 0, 0, len(pcm), D, f, 0, n_out, out.data_ptr())
        rx.synchronize()
        return out.cpu().numpy()

    g1 = _run(rx, pcm, D, slots)
    p1 = plain()
    g2 = _run(rx, pcm, D, slots)
    p2 = plain()
    v, tol = G.grid(pcm, D, slots)
    assert G.worst(g1, v, tol) <= 1.0
    assert g1.tobytes() == g2.tobytes() and p1.tobytes() == p2.tobytes()
    assert not (p1 == SENTINEL).any() and CM.worst(p1, *CM.channelize(pcm, D, f)[:2]) <= 1.0


def test_refusals_leave_the_output_untouched(rx):
    """every argument the header names is refused with OFDMRX_E_ARG before anything runs; buffers that merely touch are accepted"""
    import torch
    D, W = 16, 4096
    n_out = G.n_outputs(W, D)
    buf = torch.full((W * 4 + 2 * 2 * (n_out + 1) * 4 + 64,), 77, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    assert base % 8 == 0
    d_in, d_out = base, base + 4 * W                                 # the input right before the output
    pcm = G.random_pcm(W, np.int16, seed=8)
    buf[:4 * W] = _dev(pcm.view(np.uint8).reshape(-1))
    before = buf.clone()
    torch.cuda.synchronize()
    k = np.array([5, -16], np.int32)
    pk = k.ctypes.data_as(C.c_void_p)

    def call(d_in=d_in, fmt=0, in_first=0, n_in=W, decim=D, slots=pk, n=2, out_first=0, n_out=n_out, d_out=d_out, stride=n_out + 1):
        return rx._lib.ofdmrx_util_channelize_grid(rx._h, d_in, fmt, in_first, n_in, decim, slots, n, out_first, n_out, d_out, stride)

    assert call(d_in=None) == -1 and call(d_out=None) == -1          # NULL pointers
    assert call(slots=None) == -1 and call(slots=None, n=31) == -1   # NULL slots: only with n_slots = M
    assert call(n_in=0) == -1 and call(n_out=0) == -1 and call(n=0) == -1 and call(n=65536) == -1
    for bad in (0, 1, 3, 12, 48, 1024, -16):
        assert call(decim=bad) == -1, bad
    for bad in (16, -17, 1 << 30):
        g = np.array([5, bad], np.int32)
        assert call(slots=g.ctypes.data_as(C.c_void_p)) == -1, bad
    assert call(fmt=-1) == -1 and call(fmt=3) == -1
    assert call(in_first=-1) == -1 and call(out_first=-1) == -1
    assert call(stride=n_out - 1) == -1
    assert call(n_out=n_out + 1) == -1                                # the last output needs a position behind the buffer
    assert call(n_in=W - 20, n_out=n_out) == -1
    assert call(in_first=1, n_in=W - 1, out_first=24, n_out=100) == -1        # history: 24 D - (T - 1) = 0 lies below in_first = 1
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
    v, tol = G.grid(pcm, D, [5, -16])
    assert G.worst(got[:, :n_out], v, tol) <= 1.0
    assert (got[:, n_out:].view(np.uint8) == 77).all() and (buf[4 * W + 2 * (n_out + 1) * 8:] == 77).all()
