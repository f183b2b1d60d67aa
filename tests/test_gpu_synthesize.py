"""The wideband synthesizer on the device (k_synthesize.hip behind ofdmrx_util_synthesize) against the float64 model of
synthesize_model.py: |got - v| <= tol on every component of every F32 output, exact zeros where tol is 0,
nothing exempt; the tolerance is derived in the model's header.  The S16 output is the quantiser applied to the device's own F32
output of the same arguments, as bytes.  Every output buffer is filled with a sentinel first and has spare sample frames behind it,
which must come back untouched.  Each test prints its worst |got - v| / tol (profiles/synthesize_parity.txt keeps them)."""
import ctypes as C

import numpy as np
import pytest

import synthesize_model as SM

pytestmark = pytest.mark.gpu

SENTINEL = 12345
ALL_D = (2, 3, 6, 32)
FMT = {np.dtype(np.int16): 0, np.dtype(np.float32): 2}
N_IN = 300


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1)
    yield r
    r.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def geometry(D, Cn, rate=8000, seed=0, base=5000):
    """centres: an arbitrary one, 0, +-Rw / 2, +-1e-3 Hz, then arbitrary ones; starts: staggered, channel c at residue (base + c) mod D; gains:
    unequal.  From five channels on: channel 1 has a negative gain, one channel sits at channel 0's centre and overlaps it, one has
    gain 0, one lies wholly behind every window the tests take"""
    rw = float(D * rate)
    rng = np.random.default_rng(100 * D + seed)
    arb = rng.uniform(-rw / 2, rw / 2, size=max(Cn, 6))
    f = np.concatenate([arb[:1], [0.0, rw / 2, -rw / 2, 1e-3, -1e-3], arb[1:]])[:Cn].copy()
    s = np.array([base + c * (7 * D + 1) for c in range(Cn)], np.int64)      # residue (base + c) mod D
    g = rng.uniform(0.05, 0.5, Cn).astype(np.float32)
    if Cn >= 5:
        twin, far, mute = (3, 4, 2) if Cn < 9 else (6, 7, 8)
        f[twin] = f[0]
        g[1], g[mute] = -g[1], 0.0
        s[far] = base + 10 ** 7 * D + far                            # (its residue stays (base + far) mod D)
    assert len({int(v) % D for v in s}) == min(Cn, D)                # every residue mod D once there are D channels
    return f, s, g


def window_of(s, D, n_in=N_IN):
    """a window that begins 7 positions before the first start and ends 9 behind the last support of the channels near the base"""
    near = [int(v) for v in s if v < s.min() + 10 ** 6]                # (a channel 1e7 D behind the base is not near)
    first = min(near) - 7
    return first, SM.n_outputs(near, n_in, D) + 9 - first


def _run(rx, x, D, f, s, g, out_first, n_out, out_fmt=2, stride=None, spare=3, d_in=None):
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
    rx.synthesize(d_in.data_ptr(), FMT[x.dtype], n_in, D, f, s, g, out_first, n_out, out.data_ptr(), out_fmt, in_stride=stride)
    rx.synchronize()
    got = out.cpu().numpy()
    assert (got[n_out:] == SENTINEL).all()
    return got[:n_out]


def _check(rx, x, D, f, s, g, out_first, n_out, what, rate=8000, **kw):
    got = _run(rx, x, D, f, s, g, out_first, n_out, **kw)
    v, tol, tie = SM.synthesize(x, D, f, s, g, rate, out_first=out_first, n_out=n_out)
    assert tie > 1e-6, (what, tie)                                   # device and model cannot round an increment apart
    assert got.shape == (n_out, 2) and np.isfinite(got).all()
    w = SM.worst(got, v, tol)
    print("synthesize D %d %s: %d channels, %d outputs, worst |got - v| / tol %.4f" % (D, what, x.shape[0], n_out, w))
    assert w <= 1.0, (D, what, w)
    zero = tol == 0
    assert (got[zero] == 0).all()
    return got, w


def _s16_is_the_quantised_f32(rx, x, D, f, s, g, out_first, n_out, got32, **kw):
    got16 = _run(rx, x, D, f, s, g, out_first, n_out, out_fmt=0, **kw)
    assert got16.dtype == np.int16 and got16.tobytes() == SM.quantise(got32).tobytes()
    assert got16.min() >= -32767
    return got16


@pytest.mark.parametrize("n_channels", [1, 5, 65])
@pytest.mark.parametrize("D", ALL_D)
def test_shapes_match_model(rx, D, n_channels):
    """one channel, five (two at one centre and overlapping, one with gain 0, one negative, one wholly behind the window), 65 (the same; starts
    at every residue mod D); a window from before the first start to behind the last support; both output formats"""
    x = SM.random_x(n_channels, N_IN, np.int16, seed=D + n_channels)
    f, s, g = geometry(D, n_channels)
    first, n_out = window_of(s, D)
    got, _ = _check(rx, x, D, f, s, g, first, n_out, "shapes")
    assert (got[:7] == 0).all() and (got[-9:] == 0).all() and np.abs(got).max() > 0.01
    _s16_is_the_quantised_f32(rx, x, D, f, s, g, first, n_out, got)


@pytest.mark.parametrize("D", ALL_D)
def test_f32_input_and_a_stride(rx, D):
    """F32 input in rows longer than n_in (what lies behind a row's n_in sample frames is never read: the padding is 9.0); F32 input
    scaled by 2^12 gives exactly the scaled outputs"""
    x = SM.random_x(5, N_IN, np.float32, seed=D)
    f, s, g = geometry(D, 5, seed=1)
    first, n_out = window_of(s, D)
    got, _ = _check(rx, x, D, f, s, g, first, n_out, "f32, stride", stride=N_IN + 37)
    big, _ = _check(rx, x * np.float32(4096.0), D, f, s, g, first, n_out, "f32 x 4096", stride=N_IN + 37)
    assert (big == got * np.float32(4096.0)).all()
    x16 = SM.random_x(5, N_IN, np.int16, seed=D)
    got, _ = _check(rx, x16, D, f, s, g, first, n_out, "s16, stride", stride=N_IN + 1)
    _s16_is_the_quantised_f32(rx, x16, D, f, s, g, first, n_out, got, stride=N_IN + 1)


@pytest.mark.parametrize("D", ALL_D)
def test_window_edges(rx, D):
    """out_first and n_out one below, at and one above multiples of the kernel's tile - counted from the first window's start and from
    position 0 - inside the channels' support: byte for byte the same positions of one call over everything, which is held to the
    model"""
    TILE = SM.tile(D)
    n_in = max(N_IN, 4 * TILE // D + 50)
    x = SM.random_x(5, n_in, np.int16, seed=3 * D)
    f, s, g = geometry(D, 5, seed=2, base=3 * TILE)
    first, n_all = window_of(s, D, n_in)
    assert first < 4 * TILE - 1 and first + n_all > 6 * TILE + 2
    whole, _ = _check(rx, x, D, f, s, g, first, n_all, "whole")
    d_in = _dev(x)
    for o in (first + TILE - 1, first + TILE, first + TILE + 1, 4 * TILE - 1, 4 * TILE, 4 * TILE + 1):
        for n in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
            got = _run(rx, x, D, f, s, g, o, n, d_in=d_in)
            assert got.tobytes() == whole[o - first:o - first + n].tobytes(), (o, n)


@pytest.mark.parametrize("D", ALL_D)
def test_far_positions(rx, D):
    """starts and out_first just below 2^32, just above it and beyond 2^40: the phase is taken at the absolute index"""
    x = SM.random_x(3, N_IN, np.int16, seed=5 * D)
    for pos in (2 ** 32 - 40 * D, 2 ** 32 + 3, 2 ** 40 + 12345):
        f, s, g = geometry(D, 3, seed=3, base=pos)
        first, n_out = window_of(s, D)
        _check(rx, x, D, f, s, g, first, n_out, "start %d" % pos)


def test_a_48_khz_handle():
    """the handle's rate enters the wideband rate, and with it the phase increments"""
    import modem_amd
    rx48 = modem_amd.Receiver(device=0, chunk_frames=1, sample_rate=48000)
    try:
        D = 3
        x = SM.random_x(5, N_IN, np.int16, seed=48)
        f, s, g = geometry(D, 5, rate=48000, seed=4)
        first, n_out = window_of(s, D)
        _check(rx48, x, D, f, s, g, first, n_out, "48 kHz", rate=48000)
    finally:
        rx48.close()


@pytest.mark.parametrize("D", ALL_D)
def test_pieces_are_byte_identical(rx, D):
    """a window in one call against the same window made in pieces of 1, D - 1 and 4097 positions; and both again with an extra
    channel far behind the window, which contributes nothing: the same bytes"""
    import torch
    n_in = max(N_IN, 9000 // D + 1)                                   # (the window holds every piece size more than once)
    x = SM.random_x(6, n_in, np.int16, seed=7 * D)
    f, s, g = geometry(D, 6, seed=5)
    first, n_all = window_of(s[:5], D, n_in)
    s[5] = first + n_all + 10 ** 9
    whole, _ = _check(rx, x[:5], D, f[:5], s[:5], g[:5], first, n_all, "whole")
    d_in = _dev(x)
    for Cn in (5, 6):
        out = torch.full((n_all + 2, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        at, calls, pieces = 0, 0, [1, 4097, D - 1]
        while at < n_all:
            for p in pieces:
                n = min(p, n_all - at)
                if n:
                    rx.synthesize(d_in.data_ptr(), 0, n_in, D, f[:Cn], s[:Cn], g[:Cn], first + at, n, out.data_ptr() + 8 * at, 2)
                    calls += 1
                    at += n
        rx.synchronize()
        got = out.cpu().numpy()
        assert calls >= 6 and (got[n_all:] == SENTINEL).all()
        assert got[:n_all].tobytes() == whole.tobytes(), Cn
        assert _run(rx, x[:Cn], D, f[:Cn], s[:Cn], g[:Cn], first, n_all, d_in=d_in).tobytes() == whole.tobytes()


def test_back_to_back_calls_with_other_parameters(rx):
    """six calls with six different parameter arrays (more than the ring of parameter sets holds), issued back to back and
    synchronized only after the last: each equals the same call on a handle of its own, as bytes"""
    import modem_amd
    import torch
    D = 6
    x = SM.random_x(5, N_IN, np.int16, seed=11)
    d_in = _dev(x)
    sets = [geometry(D if k % 2 == 0 else 3, 5 - k % 3, seed=20 + k) for k in range(6)]
    wins = [window_of(s, D if k % 2 == 0 else 3) for k, (f, s, g) in enumerate(sets)]
    outs = [torch.full((n + 2, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0") for _, n in wins]
    torch.cuda.synchronize()
    for k, ((f, s, g), (first, n)) in enumerate(zip(sets, wins)):
        rx.synthesize(d_in.data_ptr(), 0, N_IN, D if k % 2 == 0 else 3, f, s, g, first, n, outs[k].data_ptr(), 2, in_stride=N_IN)
    rx.synchronize()
    for k, ((f, s, g), (first, n)) in enumerate(zip(sets, wins)):
        one = modem_amd.Receiver(device=0, chunk_frames=1)
        try:
            want = _run(one, x[:len(f)], D if k % 2 == 0 else 3, f, s, g, first, n)
        finally:
            one.close()
        got = outs[k].cpu().numpy()
        assert (got[n:] == SENTINEL).all() and got[:n].tobytes() == want.tobytes(), k


def test_a_saturating_gain_never_gives_minus_32768(rx):
    D = 6
    x = SM.random_x(2, N_IN, np.int16, seed=13)
    f, s, g = geometry(D, 2, seed=6)
    g = np.array([1e6, -3e5], np.float32)
    first, n_out = window_of(s, D)
    got = _run(rx, x, D, f, s, g, first, n_out)
    got16 = _s16_is_the_quantised_f32(rx, x, D, f, s, g, first, n_out, got)
    assert got16.max() == 32767 and got16.min() == -32767


@pytest.mark.parametrize("D", ALL_D)
def test_every_residue_of_the_start_against_the_model(rx, D):
    """D channels (and one more), one at every residue of start mod D, each alone in its stretch of the capture and all of them
    overlapping in a second call; F32 input; the window begins at a position that is no multiple of D either"""
    Cn = D + 1
    x = SM.random_x(Cn, 40, np.float32, seed=9 * D)
    rng = np.random.default_rng(9 * D)
    rw = D * 8000.0
    f = rng.uniform(-rw / 2, rw / 2, Cn)
    g = rng.uniform(0.05, 0.5, Cn).astype(np.float32)
    for what, step in (("apart", 66 * D), ("overlapping", 2 * D)):       # (a channel reaches over 63 D + 1 positions)
        s = np.array([1001 + c * (step + 1) for c in range(Cn)], np.int64)
        assert {int(v) % D for v in s} == set(range(D))
        first = 1001 - 5
        _check(rx, x, D, f, s, g, first, SM.n_outputs(s, 40, D) + 4 - first, "every residue, " + what)


def test_products_that_underflow_give_plus_zero_however_the_window_is_cut(rx):
    """F32 inputs of +-1e-38 at a gain of 1e-9: every product with the gain underflows, to -0 where it is negative.  A zero is
    always written as +0 - in one call, and where a cut lets the tile skip the second channel - so the bytes do not depend on the cut"""
    D, n_in = 6, 400
    x = np.full((2, n_in, 2), 1e-38, np.float32)
    x[:, ::2] *= -1.0
    x[1, :, 0] *= -1.0
    f, s, g = np.array([1234.5, -7000.25]), np.array([0, 2001], np.int64), np.array([1e-9, -1e-9], np.float32)
    n_all = SM.n_outputs(s, n_in, D)
    whole = _run(rx, x, D, f, s, g, 0, n_all)
    assert not whole.view(np.uint32).any()                            # +0 everywhere: no sign bit either
    d_in = _dev(x)
    for o, n in ((0, 1500), (1500, 900), (2001, 1), (1990, n_all - 1990)):
        assert not _run(rx, x, D, f, s, g, o, n, d_in=d_in).view(np.uint32).any(), (o, n)


def test_refusals_leave_the_output_untouched(rx):
    """every argument the header names is refused with OFDMRX_E_ARG before anything runs; buffers that merely touch are accepted"""
    import torch
    D, Cn, n_in = 6, 2, N_IN
    x = SM.random_x(Cn, n_in, np.int16, seed=17)
    f, s, g = geometry(D, Cn, seed=7, base=100)
    n_out = SM.n_outputs(s, n_in, D)
    in_bytes = Cn * n_in * 4
    buf = torch.full((in_bytes + n_out * 8 + 64,), 77, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    assert base % 8 == 0 and in_bytes % 8 == 0
    d_in, d_out = base, base + in_bytes                               # the input right before the output
    buf[:in_bytes] = _dev(x.view(np.uint8).reshape(-1))
    before = buf.clone()
    torch.cuda.synchronize()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    s0 = s.astype(np.int64)

    def call(d_in=d_in, ifmt=0, stride=n_in, n_in=n_in, interp=D, cf=f, st=s0, gn=g, n_ch=Cn, out_first=0, n_out=n_out, d_out=d_out, ofmt=2):
        return rx._lib.ofdmrx_util_synthesize(rx._h, d_in, ifmt, stride, n_in, interp, p(cf), p(st), p(gn), n_ch, out_first, n_out, d_out, ofmt)

    assert call(d_in=None) == -1 and call(d_out=None) == -1                                   # NULL pointers
    assert call(cf=None) == -1 and call(st=None) == -1 and call(gn=None) == -1
    assert call(n_in=0) == -1 and call(n_out=0) == -1 and call(n_ch=0) == -1                   # zero counts
    assert call(n_ch=65536) == -1
    assert call(interp=1) == -1 and call(interp=33) == -1 and call(interp=0) == -1
    assert call(ifmt=-1) == -1 and call(ifmt=1) == -1 and call(ifmt=3) == -1
    assert call(ofmt=-1) == -1 and call(ofmt=1) == -1 and call(ofmt=3) == -1
    assert call(stride=n_in - 1) == -1
    assert call(out_first=-1) == -1
    assert call(st=np.array([0, -1], np.int64)) == -1
    for bad in (float("nan"), float("inf"), -float("inf"), 24000.001, -24000.001):           # |f_c| <= Rw / 2 = 24000
        assert call(cf=np.array([1000.0, bad], np.float64)) == -1, bad
    for bad in (float("nan"), float("inf"), -float("inf"), 3e38):                              # (6 x 3e38 is not an fp32 number)
        assert call(gn=np.array([1.0, bad], np.float32)) == -1, bad
    assert call(out_first=(1 << 50) + 1) == -1 and call(st=np.array([0, (1 << 50) + 1], np.int64)) == -1
    assert call(n_out=(1 << 50) + 1) == -1 and call(n_in=(1 << 50) + 1, stride=(1 << 50) + 1) == -1
    for off in (8, in_bytes - 8, -8, -n_out * 8 + 8):                                          # the output overlaps the input, from either side
        assert call(d_out=d_in + off) == -1, off
    assert call(d_in=d_in + 2) == -1 and call(d_out=d_out + 4) == -1                          # off the sample-frame boundary
    assert call(ofmt=0, d_out=d_out + 2) == -1 and call(ifmt=2, stride=n_in // 2, n_in=n_in // 2, d_in=d_in + 4) == -1
    with rx.feed(2):                                                                           # a handle with an open feed
        assert call() == -1
    assert rx._lib.ofdmrx_bank_begin(rx._h, 2, 2, 2) == 0                                      # a handle with an open bank
    try:
        assert call() == -1
    finally:
        out, res = np.zeros((4, 5380), np.uint8), np.zeros(4 * 56, np.uint8)
        ch, ix = np.zeros(4, np.int32), np.zeros(4, np.int64)
        a, b = C.c_size_t(0), C.c_size_t(0)
        assert rx._lib.ofdmrx_bank_end(rx._h, 4, p(out), p(res), p(ch), p(ix), C.byref(a), C.byref(b)) == 0
    rx.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    assert call() == 0                                                # adjacent buffers
    rx.synchronize()
    assert torch.equal(buf[:in_bytes], before[:in_bytes])
    got = buf[in_bytes:in_bytes + n_out * 8].cpu().numpy().view(np.float32).reshape(n_out, 2)
    v, tol, _ = SM.synthesize(x, D, f, s, g)
    assert SM.worst(got, v, tol) <= 1.0
    assert (buf[in_bytes + n_out * 8:] == 77).all()
