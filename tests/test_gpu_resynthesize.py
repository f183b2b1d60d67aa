"""The wideband synthesizer at a rational interpolation on the device (k_resynthesize.hip behind ofdmrx_util_synthesize_ratio)
against the float64 model of resynthesize_model.py: |got - v| <= tol on every component of every F32
output, exact +0 where tol is 0, nothing exempt; the tolerance is derived in the model's header.  The S16 output is the quantiser
applied to the device's own F32 output of the same arguments, as bytes.  Every output buffer is filled with a sentinel first and
has spare sample frames behind it, which must come back untouched.  Each test prints its worst |got - v| / tol
(profiles/resynthesize_parity.txt keeps them)."""
import ctypes as C
import fractions

import numpy as np
import pytest

import resynthesize_model as RS
import rechannelize_model as RM

pytestmark = pytest.mark.gpu

SENTINEL = 12345
RATIOS = [(5, 2, 8000), (33, 16, 8000), (25, 4, 8000), (125, 4, 8000), (511, 16, 8000), (64, 3, 48000)]
FMT = {np.dtype(np.int16): 0, np.dtype(np.float32): 2}
N_IN = 120
TILE = RS.TILE


@pytest.fixture(scope="module")
def handles():
    import modem_amd
    made = {rate: modem_amd.Receiver(device=0, chunk_frames=1, sample_rate=rate) for rate in (8000, 48000)}
    yield made
    for r in made.values():
        r.close()


@pytest.fixture(scope="module")
def rx(handles):
    return handles[8000]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def geometry(P, Q, Cn, rate=8000, seed=0, base=0, n_in=N_IN):
    """centres: an arbitrary one, 0, +-Rw / 2, +-1e-3 Hz; starts: channel 0 at base, the others staggered behind it at other residues mod P
    so that they overlap; gains: unequal.  With five channels: channel 1 has a negative gain, channel 3 sits at channel 0's centre
    and overlaps it, channel 2 has gain 0, channel 4 lies wholly behind every window the tests take"""
    rw = RM.wide_rate(rate, P, Q)
    rng = np.random.default_rng(100 * P + Q + seed)
    arb = rng.uniform(-0.49 * rw, 0.49 * rw, size=6)
    f = np.concatenate([arb[:1], [0.0, rw / 2, -rw / 2, 1e-3, -1e-3]])[:Cn].copy()
    step = (n_in * P) // (4 * Q)
    s = np.array([base + c * step + (c * (Q + 1)) % P for c in range(Cn)], np.int64)
    g = rng.uniform(0.05, 0.5, Cn).astype(np.float32)
    if Cn >= 5:
        f[3] = f[0]
        g[1], g[2] = -g[1], 0.0
        s[4] = base + 10 ** 7 * P + 4
    return f, s, g


def window_of(s, P, Q, n_in=N_IN, before=7):
    """a window that begins `before` positions before the first start (or at 0) and ends 9 behind the last support of the channels
    near the base"""
    near = [int(v) for v in s if v < s.min() + 10 ** 6]
    first = max(min(near) - before, 0)
    return first, RS.n_outputs(near, n_in, P, Q) + 9 - first


def _run(rx, x, P, Q, f, s, g, out_first, n_out, out_fmt=2, stride=None, spare=3, d_in=None, interp=None):
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
    rx.synthesize(d_in.data_ptr(), FMT[x.dtype], n_in, (P, Q) if interp is None else interp, f, s, g, out_first, n_out, out.data_ptr(), out_fmt,
                  in_stride=stride)
    rx.synchronize()
    got = out.cpu().numpy()
    assert (got[n_out:] == SENTINEL).all()
    return got[:n_out]


def _check(rx, x, P, Q, f, s, g, out_first, n_out, what, rate=8000, **kw):
    got = _run(rx, x, P, Q, f, s, g, out_first, n_out, **kw)
    v, tol, tie = RS.synthesize(x, P, Q, f, s, g, rate, out_first=out_first, n_out=n_out)
    assert tie > 1e-6, (what, tie)                                   # device and model cannot round an increment apart
    assert got.shape == (n_out, 2) and np.isfinite(got).all()
    w = RS.worst(got, v, tol)
    print("synthesize %d/%d %s: %d channels, %d outputs, worst |got - v| / tol %.4f" % (P, Q, what, x.shape[0], n_out, w))
    assert w <= 1.0, (P, Q, what, w)
    zero = tol == 0
    assert not got[zero].view(np.uint32).any()                       # exactly +0
    return got, w


def _s16_is_the_quantised_f32(rx, x, P, Q, f, s, g, out_first, n_out, got32, **kw):
    got16 = _run(rx, x, P, Q, f, s, g, out_first, n_out, out_fmt=0, **kw)
    assert got16.dtype == np.int16 and got16.tobytes() == RS.quantise(got32).tobytes()
    assert got16.min() >= -32767
    return got16


def _starts(P):
    return (0, 1, P - 1, P, P + 1, 2 ** 40 + 3)


@pytest.mark.parametrize("n_channels", [1, 5])
@pytest.mark.parametrize("P,Q,rate", RATIOS)
def test_shapes_match_model(handles, P, Q, rate, n_channels):
    """one channel and five (two at one centre and overlapping, one with gain 0, one negative, one wholly behind the window), the first
    start at 0, 1, P - 1, P, P + 1 and 2^40 + 3 with out_first following it - P consecutive outputs visit every b, and a channel's
    support holds many times P; a window from before the first start to behind the last support; both output formats"""
    rx = handles[rate]
    x = RS.random_x(n_channels, N_IN, np.int16, seed=P + n_channels)
    d_in = _dev(x)
    worst = 0.0
    for base in _starts(P):
        f, s, g = geometry(P, Q, n_channels, rate, base=base)
        first, n_out = window_of(s, P, Q)
        assert n_out <= 4800 + 3 * N_IN * P // (4 * Q)
        got, w = _check(rx, x, P, Q, f, s, g, first, n_out, "start %d" % base, rate=rate, d_in=d_in)
        worst = max(worst, w)
        assert (got[-9:] == 0).all() and np.abs(got).max() > 0.01
        if base >= 7:
            assert (got[:7] == 0).all()
        _s16_is_the_quantised_f32(rx, x, P, Q, f, s, g, first, n_out, got, d_in=d_in)
    print("synthesize %d/%d, %d channels: worst over the starts %.4f" % (P, Q, n_channels, worst))


@pytest.mark.parametrize("P,Q,rate", RATIOS)
def test_f32_input_and_a_stride(handles, P, Q, rate):
    """F32 input in rows longer than n_in (what lies behind a row's n_in sample frames is never read: the padding is 9.0); F32 input
    scaled by 2^12 gives exactly the scaled outputs; S16 input in padded rows; a ratio that is not in lowest terms and a Fraction"""
    rx = handles[rate]
    x = RS.random_x(5, N_IN, np.float32, seed=P)
    f, s, g = geometry(P, Q, 5, rate, seed=1, base=1000 + P)
    first, n_out = window_of(s, P, Q)
    got, _ = _check(rx, x, P, Q, f, s, g, first, n_out, "f32, stride", rate=rate, stride=N_IN + 37)
    big, _ = _check(rx, x * np.float32(4096.0), P, Q, f, s, g, first, n_out, "f32 x 4096", rate=rate, stride=N_IN + 37)
    assert (big == got * np.float32(4096.0)).all()
    assert _run(rx, x, P, Q, f, s, g, first, n_out, interp=(2 * P, 2 * Q)).tobytes() == got.tobytes()
    assert _run(rx, x, P, Q, f, s, g, first, n_out, interp=fractions.Fraction(P, Q)).tobytes() == got.tobytes()
    x16 = RS.random_x(5, N_IN, np.int16, seed=P)
    got, _ = _check(rx, x16, P, Q, f, s, g, first, n_out, "s16, stride", rate=rate, stride=N_IN + 1)
    _s16_is_the_quantised_f32(rx, x16, P, Q, f, s, g, first, n_out, got, stride=N_IN + 1)


@pytest.mark.parametrize("P,Q,rate", RATIOS)
def test_window_edges(handles, P, Q, rate):
    """out_first and the window's end one below, at and one above multiples of the kernel's tile - counted from the first window's
    start and from position 0 - and a window that ends one output past a channel's support: byte for byte the same positions of one
    call over everything, which is held to the model"""
    rx = handles[rate]
    n_in = 3 * TILE * Q // P + 50
    x = RS.random_x(3, n_in, np.int16, seed=3 * P)
    f, s, g = geometry(P, Q, 3, rate, seed=2, base=3 * TILE - 5, n_in=40)
    first, n_all = window_of(s, P, Q, n_in)
    assert first < 3 * TILE and first + n_all > 5 * TILE + 2
    whole, _ = _check(rx, x, P, Q, f, s, g, first, n_all, "whole", rate=rate)
    d_in = _dev(x)
    for o in (first + TILE - 1, first + TILE, first + TILE + 1, 4 * TILE - 1, 4 * TILE, 4 * TILE + 1):
        for n in (1, TILE - 1, TILE, TILE + 1):
            got = _run(rx, x, P, Q, f, s, g, o, n, d_in=d_in)
            assert got.tobytes() == whole[o - first:o - first + n].tobytes(), (o, n)
    end = RS.support(int(s[0]), n_in, P, Q)                           # channel 0's last output
    assert whole[end - first].any() or whole[end - 1 - first].any()
    for o in (end - 1, end, end + 1):
        got = _run(rx, x, P, Q, f, s, g, o, end + 2 - o, d_in=d_in)
        assert got.tobytes() == whole[o - first:end + 2 - first].tobytes(), o
    alone = _run(rx, x[:1], P, Q, f[:1], s[:1], g[:1], end - 2, 4, d_in=d_in)
    assert not alone[3].view(np.uint32).any() and alone[:3].any()      # one output past the support of a channel alone: +0


@pytest.mark.parametrize("P,Q,rate", RATIOS)
def test_pieces_are_byte_identical(handles, P, Q, rate):
    """a window in one call against the same window made in pieces of 1, 4097 and P - 1 positions; and both again with an extra
    channel far behind the window, which contributes nothing: the same bytes"""
    import torch
    rx = handles[rate]
    n_in = (2 * (4097 + P) + 200) * Q // P + 1                        # (the window holds every piece size more than once)
    x = RS.random_x(4, n_in, np.int16, seed=7 * P)
    f, s, g = geometry(P, Q, 4, rate, seed=5, base=77, n_in=40)
    first, n_all = window_of(s[:3], P, Q, n_in)
    s[3] = first + n_all + 10 ** 9
    whole, _ = _check(rx, x[:3], P, Q, f[:3], s[:3], g[:3], first, n_all, "whole", rate=rate)
    d_in = _dev(x)
    for Cn in (3, 4):
        out = torch.full((n_all + 2, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        at, calls, pieces = 0, 0, [1, 4097, P - 1]
        while at < n_all:
            for p in pieces:
                n = min(p, n_all - at)
                if n:
                    rx.synthesize(d_in.data_ptr(), 0, n_in, (P, Q), f[:Cn], s[:Cn], g[:Cn], first + at, n, out.data_ptr() + 8 * at, 2)
                    calls += 1
                    at += n
        rx.synchronize()
        got = out.cpu().numpy()
        assert calls >= 6 and (got[n_all:] == SENTINEL).all()
        assert got[:n_all].tobytes() == whole.tobytes(), Cn
        assert _run(rx, x[:Cn], P, Q, f[:Cn], s[:Cn], g[:Cn], first, n_all, d_in=d_in).tobytes() == whole.tobytes()


def test_back_to_back_calls_with_other_parameters(rx):
    """six calls with six different parameter sets (more than the ring holds) - the ratios 25/4, 25/3 and 6 in turn, so that a set
    of one ratio is followed by a set with the same p or the same channels at another ratio - issued back to back and synchronized
    only after the last: each equals the same call on a handle of its own, as bytes"""
    import modem_amd
    import torch
    x = RS.random_x(5, N_IN, np.int16, seed=11)
    d_in = _dev(x)
    ratios = [(25, 4), (25, 3), (6, 1), (25, 3), (25, 4), (6, 1)]
    sets = [geometry(25, 4, 5 - k % 3, seed=20 + k // 3, base=100) for k in range(6)]   # (sets 0 and 3, 1 and 4, 2 and 5 share channel counts)
    rng = np.random.default_rng(21)
    sets = [(rng.uniform(-20000.0, 20000.0, len(f)), s, g) for f, s, g in sets]   # other centres every time, inside every ratio's band
    sets[1] = sets[0]                                                # the same centres, starts and gains at 25/4 and then at 25/3
    interps = [(p, q) if q > 1 else p for p, q in ratios]
    wins = [(0, max(int(s[:4].max()), 0) + RS.reach(N_IN, p, q) + 5) for (p, q), (f, s, g) in zip(ratios, sets)]
    outs = [torch.full((n + 2, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0") for _, n in wins]
    torch.cuda.synchronize()
    for k, ((f, s, g), (first, n)) in enumerate(zip(sets, wins)):
        rx.synthesize(d_in.data_ptr(), 0, N_IN, interps[k], f, s, g, first, n, outs[k].data_ptr(), 2, in_stride=N_IN)
    rx.synchronize()
    for k, ((f, s, g), (first, n)) in enumerate(zip(sets, wins)):
        one = modem_amd.Receiver(device=0, chunk_frames=1)
        try:
            want = _run(one, x[:len(f)], 0, 0, f, s, g, first, n, interp=interps[k])
        finally:
            one.close()
        got = outs[k].cpu().numpy()
        assert (got[n:] == SENTINEL).all() and got[:n].tobytes() == want.tobytes(), k
        assert np.abs(want).max() > 0.01
    assert outs[0].cpu().numpy()[150:400].tobytes() != outs[1].cpu().numpy()[150:400].tobytes()   # (the starts are 100 and later)


def test_a_ratio_with_q_1_is_the_integer_synthesizer(rx):
    """(12, 2) reduces to 6 / 1 and forwards: the bytes of ofdmrx_util_synthesize at 6, in both output formats"""
    x = RS.random_x(5, N_IN, np.int16, seed=12)
    f, s, g = geometry(6, 1, 5, seed=8, base=1234)
    first, n_out = window_of(s, 6, 1)
    for fmt in (2, 0):
        a = _run(rx, x, 6, 1, f, s, g, first, n_out, out_fmt=fmt, interp=(12, 2))
        b = _run(rx, x, 6, 1, f, s, g, first, n_out, out_fmt=fmt, interp=6)
        assert a.tobytes() == b.tobytes() and a.any()


def test_a_saturating_gain_never_gives_minus_32768(rx):
    P, Q = 25, 4
    x = RS.random_x(2, N_IN, np.int16, seed=13)
    f, s, g = geometry(P, Q, 2, seed=6, base=10)
    g = np.array([1e6, -3e5], np.float32)
    first, n_out = window_of(s, P, Q)
    got = _run(rx, x, P, Q, f, s, g, first, n_out)
    got16 = _s16_is_the_quantised_f32(rx, x, P, Q, f, s, g, first, n_out, got)
    assert got16.max() == 32767 and got16.min() == -32767


@pytest.mark.parametrize("P,Q", [(5, 2), (25, 4), (511, 16)])
def test_products_that_underflow_give_plus_zero_however_the_window_is_cut(rx, P, Q):
    """F32 inputs of +-1e-38 at gains of +-1e-30: every product with the gain underflows, to -0 where it is negative.  A zero is
    always written as +0 - in one call, and where a cut lets the tile skip the second channel - so the bytes do not depend on the cut"""
    n_in = 2 * TILE * Q // P + 40
    x = np.full((2, n_in, 2), 1e-38, np.float32)
    x[:, ::2] *= -1.0
    x[1, :, 0] *= -1.0
    second = TILE + 333
    f, s, g = np.array([1234.5, -7000.25]), np.array([0, second], np.int64), np.array([1e-30, -1e-30], np.float32)
    n_all = RS.n_outputs(s, n_in, P, Q)
    assert n_all > 3 * TILE
    whole = _run(rx, x, P, Q, f, s, g, 0, n_all)
    assert not whole.view(np.uint32).any()                            # +0 everywhere: no sign bit either
    d_in = _dev(x)
    for o, n in ((0, TILE), (0, second), (second, 1), (second - 10, n_all - second + 10), (TILE, TILE)):
        assert not _run(rx, x, P, Q, f, s, g, o, n, d_in=d_in).view(np.uint32).any(), (o, n)
    # the same cuts on inputs that do not underflow: skipping the second channel in the first tile changes no byte
    y = RS.random_x(2, n_in, np.float32, seed=P)
    g2 = np.array([0.3, -0.2], np.float32)
    whole = _run(rx, y, P, Q, f, s, g2, 0, n_all)
    d_in = _dev(y)
    for o, n in ((0, TILE), (0, second), (second, 1), (second - 10, n_all - second + 10), (TILE, TILE)):
        assert _run(rx, y, P, Q, f, s, g2, o, n, d_in=d_in).tobytes() == whole[o:o + n].tobytes(), (o, n)


def test_refusals_leave_the_output_untouched(rx):
    """every argument the header names is refused with OFDMRX_E_ARG before anything runs; buffers that merely touch are accepted"""
    import torch
    P, Q, Cn, n_in = 25, 4, 2, N_IN
    x = RS.random_x(Cn, n_in, np.int16, seed=17)
    f, s, g = geometry(P, Q, Cn, seed=7, base=100)
    n_out = RS.n_outputs(s, n_in, P, Q)
    n_out += n_out % 2                                                # (the buffers below stay on 8-byte boundaries)
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

    def call(d_in=d_in, ifmt=0, stride=n_in, n_in=n_in, pq=(P, Q), cf=f, st=s0, gn=g, n_ch=Cn, out_first=0, n_out=n_out, d_out=d_out, ofmt=2):
        return rx._lib.ofdmrx_util_synthesize_ratio(rx._h, d_in, ifmt, stride, n_in, pq[0], pq[1], p(cf), p(st), p(gn), n_ch, out_first, n_out,
                                                    d_out, ofmt)

    for pq in ((0, 4), (25, 0), (-25, 4), (25, -4), (35, 17), (7, 4), (129, 4), (1, 1), (33, 1)):   # the ratio's limits
        assert call(pq=pq) == -1, pq
    assert call(d_in=None) == -1 and call(d_out=None) == -1                                   # NULL pointers
    assert call(cf=None) == -1 and call(st=None) == -1 and call(gn=None) == -1
    assert call(n_in=0) == -1 and call(n_out=0) == -1 and call(n_ch=0) == -1                   # zero counts
    assert call(n_ch=65536) == -1
    assert call(ifmt=-1) == -1 and call(ifmt=1) == -1 and call(ifmt=3) == -1
    assert call(ofmt=-1) == -1 and call(ofmt=1) == -1 and call(ofmt=3) == -1
    assert call(stride=n_in - 1) == -1
    assert call(out_first=-1) == -1
    assert call(st=np.array([0, -1], np.int64)) == -1
    for bad in (float("nan"), float("inf"), -float("inf"), 25000.001, -25000.001):           # |f_c| <= Rw / 2 = 25000
        assert call(cf=np.array([1000.0, bad], np.float64)) == -1, bad
    assert call(cf=np.array([25000.0, -25000.0], np.float64), n_out=2) == 0                    # (the band's edges themselves are centres)
    rx.synchronize()
    buf.copy_(before)
    torch.cuda.synchronize()
    for bad in (float("nan"), float("inf"), -float("inf"), 3e38):                              # (6.25 x 3e38 is not an fp32 number)
        assert call(gn=np.array([1.0, bad], np.float32)) == -1, bad
    assert call(out_first=(1 << 50) + 1) == -1 and call(st=np.array([0, (1 << 50) + 1], np.int64)) == -1
    assert call(n_out=(1 << 50) + 1) == -1 and call(n_in=(1 << 50) + 1, stride=(1 << 50) + 1) == -1
    assert call(n_out=TILE * (2 ** 31 - 1) + 1) == -1                                          # more than the launch holds
    for off in (8, in_bytes - 8, -8, -n_out * 8 + 8):                                          # the output overlaps the input, from either side
        assert call(d_out=d_in + off) == -1, off
    assert call(d_in=d_in + 2) == -1 and call(d_out=d_out + 4) == -1                          # off the sample-frame boundary
    assert call(ofmt=0, d_out=d_out + 2) == -1 and call(ifmt=2, stride=n_in // 2, n_in=n_in // 2, d_in=d_in + 4) == -1
    with rx.feed(2):                                                                           # a handle with an open feed
        assert call() == -1 and call(pq=(50, 8)) == -1
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
    assert call(pq=(50, 8)) == 0                                      # adjacent buffers; (50, 8) is (25, 4)
    rx.synchronize()
    assert torch.equal(buf[:in_bytes], before[:in_bytes])
    got = buf[in_bytes:in_bytes + n_out * 8].cpu().numpy().view(np.float32).reshape(n_out, 2)
    v, tol, _ = RS.synthesize(x, P, Q, f, s, g, n_out=n_out)
    assert RS.worst(got, v, tol) <= 1.0
    assert (buf[in_bytes + n_out * 8:] == 77).all()
