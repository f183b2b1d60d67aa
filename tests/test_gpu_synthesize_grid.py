"""The grid synthesizer on the device (k_synthesize_grid.hip behind ofdmrx_util_synthesize_grid) against the float64 model of
synthesize_grid_model.py: |got - v| <= tol on every component of every F32 output, +0 by bit pattern where
tol is 0, nothing exempt; the tolerance is derived in the model's header.  The S16 output is the quantiser applied to the device's
own F32 output of the same arguments, as bytes.  Every output buffer is filled with a sentinel first and has spare sample frames
behind it, which must come back untouched.  Each test prints its worst |got - v| / tol (profiles/synthesize_grid_parity.txt keeps
them)."""
import ctypes as C

import numpy as np
import pytest

import synthesize_grid_model as SG
import synthesize_model as SM

pytestmark = pytest.mark.gpu

SENTINEL = 12345
ALL_D = (2, 4, 32, 64, 512)
FMT = {np.dtype(np.int16): 0, np.dtype(np.float32): 2}


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1)
    yield r
    r.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def subset(D):
    """the shuffled subset of the slots: both ends of the range, the two around zero"""
    return np.array([-1, D - 1, -D, 0], np.int64)


def geometry(D, slots, seed=0, base=0, spread=5):
    """unequal starts on the grid of D from `base` (a multiple of D) on, unequal signed gains (row 1 is negative)"""
    rng = np.random.default_rng(100 * D + seed)
    Cn = len(slots)
    s = base + (rng.integers(0, spread + 1, Cn) * D).astype(np.int64)
    s[0] = base
    g = rng.uniform(0.05, 0.5, Cn).astype(np.float32) * rng.choice([-1.0, 1.0], Cn).astype(np.float32)
    g[min(1, Cn - 1)] = -abs(g[min(1, Cn - 1)])
    if Cn > 4:
        g *= np.float32(4.0 / Cn)                                     # (many full-scale rows: keep the sum near full scale)
    return s, g


def window_of(s, D, n_in):
    """a window that begins 7 positions before the first start and ends 9 behind the last support"""
    first = max(int(min(s)) - 7, 0)
    return first, SG.n_outputs(s, n_in, D) + 9 - first


def _run(rx, x, D, k, s, g, out_first, n_out, out_fmt=2, stride=None, spare=3, d_in=None):
    """-> [n_out, 2] float32 or int16 from the device; checks the spare sample frames"""
    import torch
    x = np.ascontiguousarray(x)
    Cn, n_in = x.shape[:2]
    if stride is not None and d_in is None:
        pad = np.full((Cn, stride, 2), 9, x.dtype)
        pad[:, :n_in] = x
        d_in = _dev(pad)
    d_in = _dev(x) if d_in is None else d_in
    out = torch.full((n_out + spare, 2), SENTINEL, dtype=torch.float32 if out_fmt == 2 else torch.int16, device="cuda:0")
    torch.cuda.synchronize()                                         # the handle has a stream of its own
    rx.synthesize_grid(d_in.data_ptr(), FMT[x.dtype], n_in, D, k, s, g, out_first, n_out, out.data_ptr(), out_fmt, in_stride=stride)
    rx.synchronize()
    got = out.cpu().numpy()
    assert (got[n_out:] == SENTINEL).all()
    return got[:n_out]


def _hold(got, x, D, k, s, g, out_first, n_out, what):
    v, tol = SG.grid(x, D, k, s, g, out_first=out_first, n_out=n_out)
    assert got.shape == (n_out, 2) and np.isfinite(got).all()
    w = SG.worst(got, v, tol)
    print("synthesize_grid D %d %s: %d rows, %d outputs, worst |got - v| / tol %.4f" % (D, what, x.shape[0], n_out, w))
    assert w <= 1.0, (D, what, w)
    assert not got[tol == 0].view(np.uint32).any()                   # +0 by bit pattern
    return w


def _check(rx, x, D, k, s, g, out_first, n_out, what, **kw):
    got = _run(rx, x, D, k, s, g, out_first, n_out, **kw)
    return got, _hold(got, x, D, k, s, g, out_first, n_out, what)


def _s16_is_the_quantised_f32(rx, x, D, k, s, g, out_first, n_out, got32, **kw):
    got16 = _run(rx, x, D, k, s, g, out_first, n_out, out_fmt=0, **kw)
    assert got16.dtype == np.int16 and got16.tobytes() == SG.quantise(got32).tobytes()
    assert got16.min() >= -32767
    return got16


@pytest.mark.parametrize("which", ["all", "subset"])
@pytest.mark.parametrize("D", ALL_D)
def test_transform_tile_edges(rx, D, which):
    """rows of 1, tile - 1, tile and tile + 1 input times of the transform kernel's tile, in all slots (row c in slot c - D) and in
    the shuffled subset, unequal starts, signed gains; a window from before the first start to behind the last support; both output
    formats"""
    k = SG.all_slots(D) if which == "all" else subset(D)
    for n_in in (1, SG.tile(D) - 1, SG.tile(D), SG.tile(D) + 1):
        x = SG.random_x(len(k), n_in, np.int16, seed=D + n_in)
        s, g = geometry(D, k, seed=n_in, base=3 * D)
        first, n_out = window_of(s, D, n_in)
        got, _ = _check(rx, x, D, None if which == "all" else k, s, g, first, n_out, "%s slots, n_in %d" % (which, n_in))
        assert np.abs(got).max() > 0.01
        _s16_is_the_quantised_f32(rx, x, D, None if which == "all" else k, s, g, first, n_out, got)


@pytest.mark.parametrize("D", ALL_D)
def test_f32_input_and_a_stride(rx, D):
    """F32 input in rows longer than n_in (what lies behind a row's n_in sample frames is never read: the padding is 9.0); F32 input
    scaled by 2^12 gives exactly the scaled outputs; S16 input with a stride"""
    k, n_in = subset(D), 75
    x = SG.random_x(4, n_in, np.float32, seed=D)
    s, g = geometry(D, k, seed=1, base=2 * D)
    first, n_out = window_of(s, D, n_in)
    got, _ = _check(rx, x, D, k, s, g, first, n_out, "f32, stride", stride=n_in + 37)
    big, _ = _check(rx, x * np.float32(4096.0), D, k, s, g, first, n_out, "f32 x 4096", stride=n_in + 37)
    assert (big == got * np.float32(4096.0)).all()
    x16 = SG.random_x(4, n_in, np.int16, seed=D)
    got, _ = _check(rx, x16, D, k, s, g, first, n_out, "s16, stride", stride=n_in + 1)
    _s16_is_the_quantised_f32(rx, x16, D, k, s, g, first, n_out, got, stride=n_in + 1)


def test_a_saturating_gain_never_gives_minus_32768(rx):
    D, n_in = 4, 200
    k = np.array([-4, 3], np.int64)
    x = SG.random_x(2, n_in, np.int16, seed=13)
    s, g = np.array([0, 8], np.int64), np.array([1e6, -3e5], np.float32)
    first, n_out = window_of(s, D, n_in)
    got = _run(rx, x, D, k, s, g, first, n_out)
    got16 = _s16_is_the_quantised_f32(rx, x, D, k, s, g, first, n_out, got)
    assert got16.max() == 32767 and got16.min() == -32767


@pytest.mark.parametrize("D", ALL_D)
def test_window_edges(rx, D):
    """out_first and n_out one below, at and one above multiples of the filter kernel's tile, inside the rows' support, and a
    window that begins before any row's start: byte for byte the same positions of one call over everything, which is held to the
    model"""
    TILE = SG.filter_tile(D)
    n_in = 4 * TILE // D + 60
    k = subset(D)
    x = SG.random_x(4, n_in, np.int16, seed=3 * D)
    s, g = geometry(D, k, seed=2, base=TILE)
    first, n_all = window_of(s, D, n_in)
    assert first < TILE and first + n_all > 5 * TILE + 2
    whole, _ = _check(rx, x, D, k, s, g, first, n_all, "whole")
    d_in = _dev(x)
    for o in (first + TILE - 1, first + TILE, first + TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 2 * TILE + D - 1):
        for n in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
            got = _run(rx, x, D, k, s, g, o, n, d_in=d_in)
            assert got.tobytes() == whole[o - first:o - first + n].tobytes(), (o, n)
    early = _run(rx, x, D, k, s, g, 0, first + 40, d_in=d_in)           # begins before any row's start
    assert not early[:first + 7].view(np.uint32).any() and early[first:].tobytes() == whole[:40].tobytes()


@pytest.mark.parametrize("D", ALL_D)
def test_far_positions(rx, D):
    """starts and out_first just below 2^32, just above it and beyond 2^40: positions are 64-bit throughout"""
    k, n_in = subset(D), 30
    x = SG.random_x(4, n_in, np.int16, seed=5 * D)
    for pos in (2 ** 32 - 40 * D, 2 ** 32 + 3 * D, 2 ** 40 + 12345 * D):
        s, g = geometry(D, k, seed=3, base=pos)
        first, n_out = window_of(s, D, n_in)
        _check(rx, x, D, k, s, g, first, n_out, "start %d" % pos)


@pytest.mark.parametrize("D", ALL_D)
def test_outputs_no_row_reaches_are_plus_zero(rx, D):
    """two rows with a gap between their supports, the first at a negative gain, F32 inputs of +-1e-38 at gains of +-1e-9 (every
    product underflows, to -0 where it is negative) and full-scale rows: the gap, what lies before the first row and what lies
    behind the last are +0 by bit pattern, however the window is cut"""
    n_in = 20
    k = np.array([-1, 0], np.int64)
    s = np.array([2 * D, (2 + n_in + 24 + 9) * D], np.int64)
    first, n_out = 0, SG.n_outputs(s, n_in, D) + 5
    tiny = np.full((2, n_in, 2), 1e-38, np.float32)
    tiny[:, ::2] *= -1.0
    tiny[1, :, 0] *= -1.0
    got = _run(rx, tiny, D, k, s, np.array([-1e-9, 1e-9], np.float32), first, n_out)
    assert not got.view(np.uint32).any()                              # +0 everywhere: no sign bit either
    x = SG.random_x(2, n_in, np.int16, seed=D)
    g = np.array([-0.4, 0.3], np.float32)
    got, _ = _check(rx, x, D, k, s, g, first, n_out, "a gap")
    gap = slice(SG.support(s[0], n_in, D) + 1, int(s[1]))
    assert gap.stop - gap.start == 10 * D - 1 and not got[gap].view(np.uint32).any() and not got[:2 * D].view(np.uint32).any()
    d_in = _dev(x)
    for o, n in ((0, 2 * D), (gap.start, 8 * D), (gap.start - 1, 3), (int(s[1]) - 1, 2), (n_out - 5, 5)):
        assert _run(rx, x, D, k, s, g, o, n, d_in=d_in).tobytes() == got[o:o + n].tobytes(), (o, n)


@pytest.mark.parametrize("D", ALL_D)
def test_pieces_are_byte_identical(rx, D):
    """a window in one call against the same window made in pieces of 1, D - 1, 4097 and D + 1 positions"""
    import torch
    n_in = 9000 // D + 40                                              # (the window holds every piece size more than once)
    k = subset(D)
    x = SG.random_x(4, n_in, np.int16, seed=7 * D)
    s, g = geometry(D, k, seed=5, base=D)
    first, n_all = window_of(s, D, n_in)
    whole, _ = _check(rx, x, D, k, s, g, first, n_all, "whole")
    d_in = _dev(x)
    out = torch.full((n_all + 2, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    at, calls, pieces = 0, 0, [1, 4097, D - 1, D + 1]
    while at < n_all:
        for p in pieces:
            n = min(p, n_all - at)
            if n:
                rx.synthesize_grid(d_in.data_ptr(), 0, n_in, D, k, s, g, first + at, n, out.data_ptr() + 8 * at, 2)
                calls += 1
                at += n
    rx.synchronize()
    got = out.cpu().numpy()
    assert calls >= 6 and (got[n_all:] == SENTINEL).all()
    assert got[:n_all].tobytes() == whole.tobytes()


@pytest.mark.parametrize("D", [2, 512])
def test_a_call_across_a_chunk_seam(rx, D):
    """one call that crosses the host's chunk seam against the same capture made in two pieces that end and begin at the seam: the
    same bytes; and the call is held to the model on windows of 2 T outputs around the seam (the rows begin shortly before it)"""
    import modem_amd
    import torch
    chunk = modem_amd.synthesize_grid_chunk(D)
    T = 24 * D + 1
    out_first = 5 * D + 3                                              # the seam lies `chunk` behind out_first rounded down to the grid
    seam = out_first // D * D + chunk
    n_in = 130
    k = subset(D)
    x = SG.random_x(4, n_in, np.int16, seed=11 * D)
    s, g = geometry(D, k, seed=6, base=seam - 60 * D)
    n_out = seam + 2 * T + 7 - out_first
    assert SG.support(int(s.max()), n_in, D) > seam + T and s.min() + 24 * D < seam - T
    d_in = _dev(x)
    one = torch.full((n_out + 2, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    two = torch.full((n_out + 2, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rx.synthesize_grid(d_in.data_ptr(), 0, n_in, D, k, s, g, out_first, n_out, one.data_ptr(), 2)
    rx.synthesize_grid(d_in.data_ptr(), 0, n_in, D, k, s, g, out_first, seam - out_first, two.data_ptr(), 2)
    rx.synthesize_grid(d_in.data_ptr(), 0, n_in, D, k, s, g, seam, n_out - (seam - out_first), two.data_ptr() + 8 * (seam - out_first), 2)
    rx.synchronize()
    assert torch.equal(one, two)
    at = seam - T - out_first
    got = one[at:at + 2 * T].cpu().numpy()
    assert (one[n_out:] == SENTINEL).all().item() and np.abs(got).max() > 0.01
    _hold(got, x, D, k, s, g, seam - T, 2 * T, "around the seam at %d" % seam)
    head = one[:s.min() - out_first].view(torch.int32)
    assert not head.any().item()                                       # no row reaches the first chunk's outputs: +0


@pytest.mark.parametrize("D", [4, 32])
def test_against_the_plain_entry(rx, D):
    """the same rows through ofdmrx_util_synthesize at the slots' centres, starts and gains: within the sum of the two tolerances"""
    n_in = 90
    k = np.concatenate([subset(D), [D // 2, -D // 2 - 1]]).astype(np.int64)
    x = SG.random_x(len(k), n_in, np.int16, seed=17 * D)
    s, g = geometry(D, k, seed=7, base=4 * D)
    first, n_out = window_of(s, D, n_in)
    got, _ = _check(rx, x, D, k, s, g, first, n_out, "against the plain entry")
    import torch
    f = SG.centres(D, 8000, k)
    out = torch.full((n_out + 3, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    d_in = _dev(x)
    torch.cuda.synchronize()
    rx.synthesize(d_in.data_ptr(), 0, n_in, D, f, s, g, first, n_out, out.data_ptr(), 2)
    rx.synchronize()
    plain = out.cpu().numpy()
    assert (plain[n_out:] == SENTINEL).all()
    _, tol = SG.grid(x, D, k, s, g, out_first=first, n_out=n_out)
    v, ptol, tie = SM.synthesize(x, D, f, s, g, 8000, out_first=first, n_out=n_out)
    assert tie > 0.49 and SM.worst(plain[:n_out], v, ptol) <= 1.0
    both = tol + ptol
    d = np.abs(got.astype(np.float64) - plain[:n_out].astype(np.float64)).max(axis=1)
    assert (d[both == 0] == 0).all()
    w = float((d[both > 0] / both[both > 0]).max())
    print("synthesize_grid D %d against ofdmrx_util_synthesize: worst |difference| / (tol + tol) %.4f" % (D, w))
    assert w <= 1.0


def test_grid_and_plain_calls_interleaved_on_one_handle(rx):
    """six calls at one D, grid and plain by turns with other parameter arrays each (more than the ring of parameter sets holds),
    issued back to back and synchronized only after the last: each equals the same call on a handle of its own, as bytes"""
    import modem_amd
    import torch
    D, n_in = 8, 120
    x = SG.random_x(4, n_in, np.int16, seed=19)
    d_in = _dev(x)
    k = subset(D)
    sets = [geometry(D, k, seed=30 + i, base=D * i) for i in range(6)]
    wins = [window_of(s, D, n_in) for s, g in sets]
    outs = [torch.full((n + 2, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0") for _, n in wins]
    f = SG.centres(D, 8000, k)

    def call(r, i, out):
        (s, g), (first, n) = sets[i], wins[i]
        if i % 2 == 0:
            r.synthesize_grid(d_in.data_ptr(), 0, n_in, D, k, s, g, first, n, out.data_ptr(), 2)
        else:
            r.synthesize(d_in.data_ptr(), 0, n_in, D, f, s, g, first, n, out.data_ptr(), 2)

    torch.cuda.synchronize()
    for i in range(6):
        call(rx, i, outs[i])
    # the same parameter arrays through the other entry right after: a grid set is not taken for a plain one
    again = [torch.full((wins[0][1] + 2, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    rx.synthesize(d_in.data_ptr(), 0, n_in, D, f, sets[0][0], sets[0][1], wins[0][0], wins[0][1], again[0].data_ptr(), 2)
    rx.synthesize_grid(d_in.data_ptr(), 0, n_in, D, k, sets[0][0], sets[0][1], wins[0][0], wins[0][1], again[1].data_ptr(), 2)
    rx.synchronize()
    for i in range(6):
        one = modem_amd.Receiver(device=0, chunk_frames=1)
        try:
            want = torch.full_like(outs[i], float(SENTINEL))
            torch.cuda.synchronize()
            call(one, i, want)
            one.synchronize()
            if i == 0:
                assert torch.equal(again[1], want)
                plain = torch.full_like(want, float(SENTINEL))
                torch.cuda.synchronize()
                one.synthesize(d_in.data_ptr(), 0, n_in, D, f, sets[0][0], sets[0][1], wins[0][0], wins[0][1], plain.data_ptr(), 2)
                one.synchronize()
                assert torch.equal(again[0], plain)
        finally:
            one.close()
        assert (outs[i][wins[i][1]:] == SENTINEL).all().item() and torch.equal(outs[i], want), i


def test_refusals_leave_the_output_untouched(rx):
    """every argument the header names is refused with OFDMRX_E_ARG before anything runs; buffers that merely touch are accepted"""
    import torch
    D, n_in = 8, 100
    k = np.array([3, -8], np.int32)
    x = SG.random_x(2, n_in, np.int16, seed=17)
    s, g = np.array([16, 0], np.int64), np.array([0.3, -0.2], np.float32)
    n_out = SG.n_outputs(s, n_in, D)
    in_bytes = 2 * n_in * 4
    buf = torch.full((in_bytes + n_out * 8 + 64,), 77, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    assert base % 8 == 0 and in_bytes % 8 == 0
    d_in, d_out = base, base + in_bytes                               # the input right before the output
    buf[:in_bytes] = _dev(x.view(np.uint8).reshape(-1))
    before = buf.clone()
    torch.cuda.synchronize()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(d_in=d_in, ifmt=0, stride=n_in, n_in=n_in, interp=D, sl=k, st=s, gn=g, n=2, out_first=0, n_out=n_out, d_out=d_out, ofmt=2):
        return rx._lib.ofdmrx_util_synthesize_grid(rx._h, d_in, ifmt, stride, n_in, interp, p(sl), p(st), p(gn), n, out_first, n_out, d_out, ofmt)

    assert call(d_in=None) == -1 and call(d_out=None) == -1 and call(st=None) == -1 and call(gn=None) == -1
    assert call(n_in=0) == -1 and call(n_out=0) == -1 and call(n=0) == -1 and call(n=17) == -1
    assert call(sl=None) == -1 and call(sl=None, n=15) == -1
    for bad in (0, 1, 3, 6, 12, 33, 1024):
        assert call(interp=bad) == -1, bad
    for bad in (8, -9, 3):                                             # outside -8 .. 7; given twice
        assert call(sl=np.array([3, bad], np.int32)) == -1, bad
    for bad in (-8, 1, 7, 12):                                         # negative; not on the grid of D
        assert call(st=np.array([16, bad], np.int64)) == -1, bad
    assert call(st=np.array([16, (1 << 50) + 8], np.int64)) == -1
    assert call(ifmt=-1) == -1 and call(ifmt=1) == -1 and call(ifmt=3) == -1
    assert call(ofmt=-1) == -1 and call(ofmt=1) == -1 and call(ofmt=3) == -1
    assert call(stride=n_in - 1) == -1 and call(out_first=-1) == -1 and call(out_first=(1 << 50) + 1) == -1
    for bad in (float("nan"), float("inf"), -float("inf"), 3e38):
        assert call(gn=np.array([1.0, bad], np.float32)) == -1, bad
    assert call(n_out=(1 << 50) + 1) == -1 and call(n_in=(1 << 50) + 1, stride=(1 << 50) + 1) == -1
    for off in (8, in_bytes - 8, -8, -n_out * 8 + 8):                  # the output overlaps the input, from either side
        assert call(d_out=d_in + off) == -1, off
    assert call(d_in=d_in + 2) == -1 and call(d_out=d_out + 4) == -1  # off the sample-frame boundary
    with rx.feed(2):                                                   # a handle with an open feed
        assert call() == -1
    rx.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    assert call() == 0                                                # adjacent buffers
    rx.synchronize()
    assert torch.equal(buf[:in_bytes], before[:in_bytes])
    got = buf[in_bytes:in_bytes + n_out * 8].cpu().numpy().view(np.float32).reshape(n_out, 2)
    _hold(got, x, D, k, s, g, 0, n_out, "adjacent buffers")
    assert (buf[in_bytes + n_out * 8:] == 77).all()
