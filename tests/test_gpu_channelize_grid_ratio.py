"""The grid front end at a ratio on the device (k_channelize_grid_ratio.hip behind ofdmrx_util_channelize_grid_ratio) against the
float64 model of channelize_grid_ratio_model.py: |got - v| <= tol on every component of every output, nothing
exempt; the tolerance is derived in the model's header.  Every output buffer is filled with a sentinel first and has spare columns
and a spare row, which must come back untouched.  Each test prints its worst |got - v| / tol
(profiles/channelize_grid_ratio_parity.txt keeps them)."""
import ctypes as C

import numpy as np
import pytest

import channelize_grid_model as G
import channelize_grid_ratio_model as R
import rechannelize_model as RM

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
# M = 6, 10, 12, 18; 30: all three radices, Q even; 50; 90: the largest Q; 250; 600; 1000: the largest tile that is no power of two
RATIOS = ((3, 1), (5, 1), (6, 1), (9, 4), (15, 2), (25, 4), (45, 16), (125, 4), (300, 1), (500, 1))
FMT = {np.dtype(np.int16): 0, np.dtype(np.uint8): 1, np.dtype(np.float32): 2}
IDS = ["%d/%d" % r for r in RATIOS]


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1)
    yield r
    r.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def tile(P, Q):
    """the kernel's tile of output times"""
    M = 2 * P
    return min(max(8, min(256, 4096 // M)), (61440 - 8 * M) // (8 * M + 4)) & ~1


def subset(P, Q):
    """the edge slots and the two about the centre, in a shuffled order"""
    k0, n = R.slot_range(P, Q)
    return [-1, k0 + n - 1, k0, 0]


def n_in_for(P, Q, n_out, out_first=0):
    """positions up to the last output's own"""
    return ((out_first + n_out - 1) * P) // Q + 1


def _run(rx, pcm, P, Q, slots, in_first=0, out_first=0, n_out=None, spare=3, d_in=None):
    """-> [n_slots, n_out, 2] float32 from the device; checks the spare columns and the spare row"""
    import torch
    pcm = np.ascontiguousarray(pcm)
    if n_out is None:
        n_out = R.n_outputs(in_first + len(pcm), P, Q) - out_first
    n = R.slot_range(P, Q)[1] if slots is None else len(slots)
    out = torch.full((n + 1, n_out + spare, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    d_in = _dev(pcm) if d_in is None else d_in
    torch.cuda.synchronize()                                         # the handle has a stream of its own
    rx.channelize_grid(d_in.data_ptr(), FMT[pcm.dtype], in_first, len(pcm), (P, Q), slots, out_first, n_out, out.data_ptr(), n_out + spare)
    rx.synchronize()
    got = out.cpu().numpy()
    assert (got[n] == SENTINEL).all() and (got[:, n_out:] == SENTINEL).all()
    return got[:n, :n_out]


def _check(rx, pcm, P, Q, slots, what, **kw):
    got = _run(rx, pcm, P, Q, slots, **kw)
    v, tol = R.grid(pcm, P, Q, slots, out_first=kw.get("out_first", 0), n_out=kw.get("n_out"), in_first=kw.get("in_first", 0))
    assert got.shape[:2] == v.shape and np.isfinite(got).all()
    w = R.worst(got, v, tol)
    print("channelize_grid_ratio %d/%d %s: %d slots x %d outputs, worst |got - v| / tol %.4f" % (P, Q, what, v.shape[0], v.shape[1], w))
    assert w <= 1.0, (P, Q, what, w)
    return got, w


@pytest.mark.parametrize("P,Q", RATIOS, ids=IDS)
def test_shapes_match_model(rx, P, Q):
    """from position 0 (the leading positions are zeros): three tiles and one output with all slots; 1 output, one short of a tile, a
    tile and one past it with the shuffled subset"""
    NT = tile(P, Q)
    worst = 0.0
    n_out = 3 * NT + 1
    worst = max(worst, _check(rx, R.random_pcm(n_in_for(P, Q, n_out), np.int16, seed=P), P, Q, None, "n_out %d" % n_out, n_out=n_out)[1])
    for n_out in (1, NT - 1, NT, NT + 1):
        pcm = R.random_pcm(n_in_for(P, Q, n_out), np.int16, seed=n_out)
        worst = max(worst, _check(rx, pcm, P, Q, subset(P, Q), "n_out %d, subset" % n_out, n_out=n_out)[1])
    print("channelize_grid_ratio %d/%d, all sizes: worst %.4f" % (P, Q, worst))


@pytest.mark.parametrize("P,Q", RATIOS, ids=IDS)
def test_formats(rx, P, Q):
    """U8 and F32 input; F32 input scaled by 2^12 gives exactly the scaled outputs"""
    n_in = n_in_for(P, Q, tile(P, Q) + 5) + 3
    _check(rx, R.random_pcm(n_in, np.uint8, seed=2), P, Q, None, "u8")
    x = R.random_pcm(n_in, np.float32, seed=3)
    got, _ = _check(rx, x, P, Q, subset(P, Q), "f32")
    big, _ = _check(rx, x * np.float32(4096.0), P, Q, subset(P, Q), "f32 x 4096")
    assert (big == got * np.float32(4096.0)).all()


@pytest.mark.parametrize("P,Q", RATIOS, ids=IDS)
def test_positions(rx, P, Q):
    """a buffer that starts inside the stream, holding exactly the history of its first output: out_first on every residue mod Q (and
    so mod 2 Q over two rounds at Q = 1), and near 2^40"""
    T = R.n_taps(P, Q)
    n_out = tile(P, Q) + 2
    firsts = [1000 + r for r in range(max(Q, 2))] + [2 ** 40 + 3]
    for out_first in firsts:
        in_first = out_first * P // Q - (T - 1)
        pcm = R.random_pcm(n_in_for(P, Q, n_out, out_first) - in_first + 2, np.int16, seed=5)
        sl = None if out_first in (1000, 2 ** 40 + 3) and P <= 125 else subset(P, Q)
        _check(rx, pcm, P, Q, sl, "out_first %d" % out_first, in_first=in_first, out_first=out_first, n_out=n_out)


@pytest.mark.parametrize("P,Q", [(25, 4), (6, 1)], ids=["25/4", "6/1"])
def test_blocks_are_byte_identical(rx, P, Q):
    """one call over a capture against the same capture arriving in blocks of 1, 4097, P - 1 and 0 samples, each call reading the
    block's outputs from the samples so far with T - 1 samples of history"""
    import torch
    T = R.n_taps(P, Q)
    W = 3 * 4097 + 17
    slots = subset(P, Q) + [2]
    pcm = R.random_pcm(W, np.int16, seed=7)
    whole = _run(rx, pcm, P, Q, slots)
    n_all = R.n_outputs(W, P, Q)
    v, tol = R.grid(pcm[:n_in_for(P, Q, 200)], P, Q, slots, n_out=200)
    assert R.worst(whole[:, :200], v, tol) <= 1.0
    d_in = _dev(pcm)
    out = torch.full((len(slots), n_all + 2, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    fed, calls, blocks = 0, 0, [1, 4097, P - 1, 0]
    while fed < W:
        for b in blocks:
            new = min(fed + b, W)
            o0, o1 = R.n_outputs(fed, P, Q), R.n_outputs(new, P, Q)
            fed = new
            if o1 == o0:
                continue
            i0 = max(0, o0 * P // Q - (T - 1))
            rx.channelize_grid(d_in.data_ptr() + 4 * i0, 0, i0, fed - i0, (P, Q), slots, o0, o1 - o0, out.data_ptr() + 8 * o0, n_all + 2)
            calls += 1
    rx.synchronize()
    got = out.cpu().numpy()
    assert calls >= 2 and (got[:, n_all:] == SENTINEL).all()
    assert got[:, :n_all].tobytes() == whole.tobytes()


@pytest.mark.parametrize("D", [64, 8])
def test_a_power_of_two_is_the_grid_entry(rx, D):
    """Q = 1 and P a power of two: the bytes of ofdmrx_util_channelize_grid, through either spelling of the ratio"""
    import torch
    pcm = R.random_pcm(70 * D + 3, np.int16, seed=D)
    n_out = R.n_outputs(len(pcm), D, 1)
    a = _run(rx, pcm, D, 1, None)
    b = _run(rx, pcm, 3 * D, 3, subset(D, 1))
    out = torch.full((2 * D, n_out, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    d_in = _dev(pcm)
    torch.cuda.synchronize()
    rx.channelize_grid(d_in.data_ptr(), 0, 0, len(pcm), D, None, 0, n_out, out.data_ptr())
    rx.synchronize()
    want = out.cpu().numpy()
    assert a.tobytes() == want.tobytes()
    assert b.tobytes() == want[[k + D for k in subset(D, 1)]].tobytes()
    v, tol = G.grid(pcm, D)
    assert G.worst(a, v, tol) <= 1.0


def test_against_the_ratio_front_end(rx):
    """25/4, all slots, against ofdmrx_util_channelize_ratio at the slot centres on the device: per component the difference is at
    most the sum of the two models' tolerances and the rounding of 4.17's increment, 2 pi 2^-33 position S"""
    import modem_amd
    import torch
    P, Q = 25, 4
    pcm = R.random_pcm(300 * P // Q + 3, np.int16, seed=11)
    n_out = R.n_outputs(len(pcm), P, Q)
    grid = _run(rx, pcm, P, Q, None)
    f = modem_amd.grid_centres((P, Q), 8000)
    assert (f == R.centres(P, Q)).all() and len(f) == 13
    out = torch.full((len(f), n_out, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    d_in = _dev(pcm)
    torch.cuda.synchronize()
    rx.channelize(d_in.data_ptr(), 0, 0, len(pcm), (P, Q), f, 0, n_out, out.data_ptr())
    rx.synchronize()
    plain = out.cpu().numpy()
    _, tol_g = R.grid(pcm, P, Q)
    _, tol_p, _ = RM.channelize(pcm, P, Q, f)
    S = tol_g / (2.0 ** -24 * R.tol_factor(2 * P))
    inc = 2 * np.pi * 2.0 ** -33 * float(len(pcm)) * S
    d = np.abs(grid.astype(np.float64) - plain.astype(np.float64)).max(axis=2)
    w = float((d / (tol_g + tol_p + inc)).max())
    print("channelize_grid_ratio 25/4 against channelize_ratio: worst |difference| / (tol + tol + increment) %.4f" % w)
    assert w <= 1.0


def test_tables_do_not_mix(rx):
    """a plain call, a grid call and a ratio-grid call in turn, twice over: each equals its own first result as bytes (the device
    table's key tells the three kinds apart at one p and q)"""
    import modem_amd
    import torch
    pcm = R.random_pcm(800, np.int16, seed=13)
    d_in = _dev(pcm)

    def plain(decim, f):
        n_out = R.n_outputs(len(pcm), *(decim if isinstance(decim, tuple) else (decim, 1)))
        out = torch.full((len(f), n_out, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        rx.channelize(d_in.data_ptr(), 0, 0, len(pcm), decim, f, 0, n_out, out.data_ptr())
        rx.synchronize()
        return out.cpu().numpy()

    slots = [2, -2, 0]
    f6, f83, f8 = (modem_amd.grid_centres(d, 8000, slots) for d in ((6, 1), (8, 3), 8))
    first = None
    for _ in range(2):
        got = [plain(6, f6), _run(rx, pcm, 6, 1, slots), plain((8, 3), f83), _run(rx, pcm, 8, 3, slots), _run(rx, pcm, 8, 1, slots), plain(8, f8)]
        assert not any((g == SENTINEL).any() for g in got)
        if first is None:
            first = got
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, first))
    for (P, Q), g in (((6, 1), first[1]), ((8, 3), first[3]), ((8, 1), first[4])):
        assert R.worst(g, *R.grid(pcm, P, Q, slots)) <= 1.0


def test_refusals_leave_the_output_untouched(rx):
    """every argument the header names is refused with OFDMRX_E_ARG before anything runs; buffers that merely touch are accepted"""
    import torch
    P, Q, W = 25, 4, 4000
    T = R.n_taps(P, Q)
    n_out = R.n_outputs(W, P, Q)
    buf = torch.full((W * 4 + 2 * 2 * (n_out + 1) * 4 + 64,), 77, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    assert base % 8 == 0
    d_in, d_out = base, base + 4 * W                                 # the input right before the output
    pcm = R.random_pcm(W, np.int16, seed=8)
    buf[:4 * W] = _dev(pcm.view(np.uint8).reshape(-1))
    before = buf.clone()
    torch.cuda.synchronize()
    k = np.array([5, -6], np.int32)
    pk = k.ctypes.data_as(C.c_void_p)

    def call(d_in=d_in, fmt=0, in_first=0, n_in=W, p=P, q=Q, slots=pk, n=2, out_first=0, n_out=n_out, d_out=d_out, stride=n_out + 1):
        return rx._lib.ofdmrx_util_channelize_grid_ratio(rx._h, d_in, fmt, in_first, n_in, p, q, slots, n, out_first, n_out, d_out, stride)

    assert call(d_in=None) == -1 and call(d_out=None) == -1          # NULL pointers
    assert call(slots=None) == -1 and call(slots=None, n=12) == -1   # NULL slots: only with n_slots = n_all = 13
    assert call(n_in=0) == -1 and call(n_out=0) == -1 and call(n=0) == -1 and call(n=65536) == -1
    for bad in ((7, 1), (511, 16), (3, 2), (513, 1), (36, 17), (0, 1), (6, 0), (-6, 1), (1024, 1), (1, 1)):
        assert call(p=bad[0], q=bad[1]) == -1, bad
    for bad in (7, -7, 1 << 30):
        g = np.array([5, bad], np.int32)
        assert call(slots=g.ctypes.data_as(C.c_void_p)) == -1, bad
    assert call(fmt=-1) == -1 and call(fmt=3) == -1
    assert call(in_first=-1) == -1 and call(out_first=-1) == -1
    assert call(stride=n_out - 1) == -1
    assert call(n_out=n_out + 1) == -1                                # the last output needs a position behind the buffer
    assert call(n_in=W - 20, n_out=n_out) == -1
    assert call(in_first=1, n_in=W - 1, out_first=24, n_out=100) == -1        # history: 24 P / Q - (T - 1) = 0 lies below in_first = 1
    for off in (8, 4 * W - 8, -8, -(2 * n_out + 1) * 8 + 8):                  # the output overlaps the input, from either side
        assert call(d_out=d_in + off) == -1, off
    assert call(d_in=d_in + 2) == -1 and call(d_out=d_out + 4) == -1          # off the sample-frame boundary / off 8 bytes
    for decim in (3, 12, 48):                                         # the grid entry itself keeps its refusals
        assert rx._lib.ofdmrx_util_channelize_grid(rx._h, d_in, 0, 0, W, decim, pk, 2, 0, 10, d_out, 11) == -1
    rx.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    i1 = 28 * P // Q - (T - 1)                                        # output 28 stands at 175: its history begins at 25
    assert i1 == 25 and call(in_first=i1, n_in=W - i1, out_first=28, n_out=100, d_in=d_in + 4 * i1) == 0     # just inside
    assert call() == 0                                                # adjacent buffers (the same stream: it runs second)
    rx.synchronize()
    assert torch.equal(buf[:4 * W], before[:4 * W])
    got = buf[4 * W:4 * W + 2 * (n_out + 1) * 8].cpu().numpy().view(np.float32).reshape(2, n_out + 1, 2)
    v, tol = R.grid(pcm, P, Q, [5, -6])
    assert R.worst(got[:, :n_out], v, tol) <= 1.0
    assert (got[:, n_out:].view(np.uint8) == 77).all() and (buf[4 * W + 2 * (n_out + 1) * 8:] == 77).all()
