"""The grid synthesizer at a ratio on the device (k_synthesize_grid_ratio.hip behind ofdmrx_util_synthesize_grid_ratio) against the
float64 model of synthesize_grid_ratio_model.py: |got - v| <= tol on every component of every F32 output,
+0 by bit pattern where tol is 0, nothing exempt; the tolerance is derived in the model's header.  The S16 output is the quantiser
applied to the device's own F32 output of the same arguments, as bytes.  Every output buffer is filled with a sentinel first and has
spare sample frames behind it, which must come back untouched.  Each test prints its worst |got - v| / tol; with
OFDMRX_PARITY_OUT=FILE in the environment the worst per ratio is written there (profiles/synthesize_grid_ratio_parity.txt keeps a
copy)."""
import ctypes as C
import os

import numpy as np
import pytest

import resynthesize_model as RS
import synthesize_grid_ratio_model as R

pytestmark = pytest.mark.gpu

SENTINEL = 12345
RATIOS = [(3, 1), (5, 2), (6, 1), (15, 2), (25, 4), (45, 16), (75, 2), (243, 1), (500, 1)]
IDS = ["%d/%d" % r for r in RATIOS]
FMT = {np.dtype(np.int16): 0, np.dtype(np.float32): 2}
WORST = {}


@pytest.fixture(scope="module")
def rx():
    import modem_amd
    r = modem_amd.Receiver(device=0, chunk_frames=1)
    yield r
    r.close()
    path = os.environ.get("OFDMRX_PARITY_OUT")
    if path and WORST:
        with open(path, "w") as f:
            f.write("ofdmrx_util_synthesize_grid_ratio against synthesize_grid_ratio_model.grid: worst |got - v| / tol over this module's cases\n")
            for (P, Q), (w, n) in sorted(WORST.items()):
                f.write("%3d/%-2d  M %4d  plan %-18s worst %.4f  (%d outputs held)\n" % (P, Q, 2 * P, " ".join(map(str, reversed(R.plan(2 * P)))), w, n))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def subset(P, Q):
    """a shuffled subset of the slots: the two extreme slots, slot 0 and its neighbours where they exist"""
    k0, n = R.slot_range(P, Q)
    k = [-1, k0 + n - 1, k0, 0, 1]
    return np.array(list(dict.fromkeys(k)), np.int64)


def gains_for(Cn, seed):
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.05, 0.5, Cn).astype(np.float32) * rng.choice([-1.0, 1.0], Cn).astype(np.float32)
    g[min(1, Cn - 1)] = -abs(g[min(1, Cn - 1)])
    if Cn > 4:
        g *= np.float32(4.0 / Cn)                                     # (many full-scale rows: keep the sum near full scale)
    return g


def geometry(P, Q, slots, seed=0, base=0, spread=5):
    """unequal starts on the grid of P from `base` (a multiple of P) on, unequal signed gains (row 1 is negative)"""
    rng = np.random.default_rng(100 * P + Q + seed)
    s = base + (rng.integers(0, spread + 1, len(slots)) * P).astype(np.int64)
    s[0] = base
    return s, gains_for(len(slots), 100 * P + seed)


def window_of(s, P, Q, n_in):
    """a window that begins 7 positions before the first start and ends 9 behind the last support"""
    first = max(int(min(s)) - 7, 0)
    return first, R.n_outputs(s, n_in, P, Q) + 9 - first


def _run(rx, x, P, Q, k, s, g, out_first, n_out, out_fmt=2, stride=None, spare=3, d_in=None):
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
    rx.synthesize_grid(d_in.data_ptr(), FMT[x.dtype], n_in, (P, Q), k, s, g, out_first, n_out, out.data_ptr(), out_fmt, in_stride=stride)
    rx.synchronize()
    got = out.cpu().numpy()
    assert (got[n_out:] == SENTINEL).all()
    return got[:n_out]


def _hold(got, x, P, Q, k, s, g, out_first, n_out, what):
    v, tol = R.grid(x, P, Q, k, s, g, out_first=out_first, n_out=n_out)
    assert got.shape == (n_out, 2) and np.isfinite(got).all()
    w = R.worst(got, v, tol)
    print("synthesize_grid %d/%d %s: %d rows, %d outputs, worst |got - v| / tol %.4f" % (P, Q, what, x.shape[0], n_out, w))
    assert w <= 1.0, (P, Q, what, w)
    assert not got[tol == 0].view(np.uint32).any()                   # +0 by bit pattern
    old = WORST.get((P, Q), (0.0, 0))
    WORST[(P, Q)] = (max(old[0], w), old[1] + n_out)
    return w


def _check(rx, x, P, Q, k, s, g, out_first, n_out, what, **kw):
    got = _run(rx, x, P, Q, k, s, g, out_first, n_out, **kw)
    return got, _hold(got, x, P, Q, k, s, g, out_first, n_out, what)


def _s16_is_the_quantised_f32(rx, x, P, Q, k, s, g, out_first, n_out, got32, **kw):
    got16 = _run(rx, x, P, Q, k, s, g, out_first, n_out, out_fmt=0, **kw)
    assert got16.dtype == np.int16 and got16.tobytes() == R.quantise(got32).tobytes()
    assert got16.min() >= -32767
    return got16


@pytest.mark.parametrize("which", ["all", "subset"])
@pytest.mark.parametrize("P,Q", RATIOS, ids=IDS)
def test_rows_at_every_edge(rx, P, Q, which):
    """rows that start at 0, P, (NT - 1) P, NT P and floor(2^40 / P) P (NT the transform kernel's tile) by turns, NT + 1 input times
    long, in every slot (S16 input) and in the subset with the two extreme slots and slot 0 (F32 input), signed gains: the window
    over the near rows and the window over the far ones, both output formats"""
    NT = R.tile(P, Q)
    k = R.all_slots(P, Q) if which == "all" else subset(P, Q)
    far = (2 ** 40 // P) * P
    edges = [0, P, (NT - 1) * P, NT * P, far]
    s = np.array([edges[c % 5] for c in range(len(k))], np.int64)
    g = gains_for(len(k), P + Q)
    n_in = NT + 1
    x = R.random_x(len(k), n_in, np.int16 if which == "all" else np.float32, seed=P + n_in)
    ks = None if which == "all" else k
    for first, n_out in ((0, R.support(NT * P, n_in, P, Q) + 10), (far - 7, R.support(far, n_in, P, Q) + 10 - (far - 7))):
        got, _ = _check(rx, x, P, Q, ks, s, g, first, n_out, "%s slots, window at %d" % (which, first))
        assert np.abs(got).max() > 0.01
        _s16_is_the_quantised_f32(rx, x, P, Q, ks, s, g, first, n_out, got)


@pytest.mark.parametrize("P,Q", RATIOS, ids=IDS)
def test_a_stride_and_scaled_f32_input(rx, P, Q):
    """rows longer than n_in (what lies behind a row's n_in sample frames is never read: the padding is 9); F32 input scaled by 2^12
    gives exactly the scaled outputs"""
    k, n_in = subset(P, Q), 45
    x = R.random_x(len(k), n_in, np.float32, seed=P)
    s, g = geometry(P, Q, k, seed=1, base=2 * P)
    first, n_out = window_of(s, P, Q, n_in)
    got, _ = _check(rx, x, P, Q, k, s, g, first, n_out, "f32, stride", stride=n_in + 37)
    big = _run(rx, x * np.float32(4096.0), P, Q, k, s, g, first, n_out, stride=n_in + 37)
    assert (big == got * np.float32(4096.0)).all()
    x16 = R.random_x(len(k), n_in, np.int16, seed=P)
    got, _ = _check(rx, x16, P, Q, k, s, g, first, n_out, "s16, stride", stride=n_in + 1)


def test_a_saturating_gain_never_gives_minus_32768(rx):
    P, Q, n_in = 25, 4, 200
    k = np.array([-6, 6], np.int64)
    x = R.random_x(2, n_in, np.int16, seed=13)
    s, g = np.array([0, 50], np.int64), np.array([1e6, -3e5], np.float32)
    first, n_out = window_of(s, P, Q, n_in)
    got = _run(rx, x, P, Q, k, s, g, first, n_out)
    got16 = _s16_is_the_quantised_f32(rx, x, P, Q, k, s, g, first, n_out, got)
    assert got16.max() == 32767 and got16.min() == -32767


@pytest.mark.parametrize("P,Q", RATIOS, ids=IDS)
def test_window_edges(rx, P, Q):
    """windows that open and close at the first and last outputs of the filter kernel's tiles and of the transform kernel's tiles
    of the whole call, and at out_first = 0, 1 and P - 1 (mod P): byte for byte the same positions of one call over everything,
    which is held to the model; and a window that begins before any row's start"""
    NT, FT = R.tile(P, Q), R.filter_tile(P, Q)
    n_in = max(2 * NT, 2 * FT * Q // P) + 30
    k = subset(P, Q)
    x = R.random_x(len(k), n_in, np.int16, seed=3 * P)
    s, g = geometry(P, Q, k, seed=2, base=2 * P, spread=2)
    first, n_all = window_of(s, P, Q, n_in)
    whole, _ = _check(rx, x, P, Q, k, s, g, first, n_all, "whole")
    j_first = first * Q // P - 24                                     # the whole call's scratch begins at this input time
    fb = R.filter_base(P, Q, first)
    edges = {fb + FT, fb + 2 * FT, (first // P + 2) * P, (first // P + 3) * P + 1, (first // P + 4) * P - 1}
    for n in (1, 2):                                                  # the first output of the transform's tile n: the first m with m Q div P = j
        j = j_first + n * NT
        if j > 0:
            edges.add(-(-j * P // Q))
    assert len(edges) >= 5
    d_in = _dev(x)
    for e in sorted(edges):
        for o, n in ((e, 1), (e - 1, 2), (e, FT + 1), (first + 3, e - first - 3), (first + 3, e - first - 2), (e - 1, n_all - (e - 1 - first))):
            if n < 1 or o < first or o + n > first + n_all:
                continue
            got = _run(rx, x, P, Q, k, s, g, o, n, d_in=d_in)
            assert got.tobytes() == whole[o - first:o - first + n].tobytes(), (e, o, n)
    smin = int(s.min())
    early = _run(rx, x, P, Q, k, s, g, 0, first + 40, d_in=d_in)       # begins before any row's start
    assert not early[:smin].view(np.uint32).any() and early[first:].tobytes() == whole[:40].tobytes()


@pytest.mark.parametrize("P,Q", RATIOS, ids=IDS)
def test_outputs_no_row_reaches_are_plus_zero(rx, P, Q):
    """two rows with a gap between their supports, the first at a negative gain, F32 inputs of +-1e-38 at gains of +-1e-9 (every
    product underflows, to -0 where it is negative) and full-scale rows: the gap, what lies before the first row and what lies
    behind the last are +0 by bit pattern, however the window is cut"""
    n_in = 20
    k = np.array([-1, 0], np.int64)
    s = np.array([2 * P, (2 + (n_in + 24 + 9 + Q - 1) // Q) * P], np.int64)
    first, n_out = 0, R.n_outputs(s, n_in, P, Q) + 5
    tiny = np.full((2, n_in, 2), 1e-38, np.float32)
    tiny[:, ::2] *= -1.0
    tiny[1, :, 0] *= -1.0
    got = _run(rx, tiny, P, Q, k, s, np.array([-1e-9, 1e-9], np.float32), first, n_out)
    assert not got.view(np.uint32).any()                              # +0 everywhere: no sign bit either
    x = R.random_x(2, n_in, np.int16, seed=P)
    g = np.array([-0.4, 0.3], np.float32)
    got, _ = _check(rx, x, P, Q, k, s, g, first, n_out, "a gap")
    gap = slice(R.support(s[0], n_in, P, Q) + 1, int(s[1]))
    assert gap.stop - gap.start >= P and not got[gap].view(np.uint32).any() and not got[:2 * P].view(np.uint32).any()
    d_in = _dev(x)
    for o, n in ((0, 2 * P), (gap.start, gap.stop - gap.start), (gap.start - 1, 3), (int(s[1]) - 1, 2), (n_out - 5, 5)):
        assert _run(rx, x, P, Q, k, s, g, o, n, d_in=d_in).tobytes() == got[o:o + n].tobytes(), (o, n)


@pytest.mark.parametrize("P,Q", RATIOS, ids=IDS)
def test_pieces_are_byte_identical(rx, P, Q):
    """a window in one call against the same window made in pieces of 1, P - 1, a filter tile + 1 positions and the rest"""
    import torch
    n_in = 3 * R.filter_tile(P, Q) * Q // P + 40
    k = subset(P, Q)
    x = R.random_x(len(k), n_in, np.int16, seed=7 * P)
    s, g = geometry(P, Q, k, seed=5, base=P)
    first, n_all = window_of(s, P, Q, n_in)
    whole, _ = _check(rx, x, P, Q, k, s, g, first, n_all, "whole")
    d_in = _dev(x)
    out = torch.full((n_all + 2, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    at, calls = 0, 0
    for p in (1, P - 1, R.filter_tile(P, Q) + 1, 1, P - 1, n_all):
        n = min(p, n_all - at)
        if n:
            rx.synthesize_grid(d_in.data_ptr(), 0, n_in, (P, Q), k, s, g, first + at, n, out.data_ptr() + 8 * at, 2)
            calls += 1
            at += n
    rx.synchronize()
    got = out.cpu().numpy()
    assert calls == 6 and at == n_all and (got[n_all:] == SENTINEL).all()
    assert got[:n_all].tobytes() == whole.tobytes()


@pytest.mark.parametrize("P,Q", [(3, 1), (512, 3)], ids=["3/1", "512/3"])
def test_a_call_across_a_chunk_seam(rx, P, Q):
    """the smallest and the largest M: one call that crosses the host's chunk seam against the same capture made in two pieces that
    end and begin at the seam: the same bytes; and the call is held to the model on a window around the seam (the rows begin shortly
    before it)"""
    import modem_amd
    import torch
    chunk = modem_amd.synthesize_grid_chunk((P, Q))
    assert chunk % P == 0
    span = 24 * P // Q + 1
    out_first = 5 * P + 3                                              # the seam lies `chunk` behind out_first rounded down to the grid of P
    seam = out_first // P * P + chunk
    n_in = 130
    k = subset(P, Q)
    x = R.random_x(len(k), n_in, np.int16, seed=11 * P)
    s, g = geometry(P, Q, k, seed=6, base=seam - (60 + Q - 1) // Q * P)
    n_out = seam + 2 * span + 7 - out_first
    assert R.support(int(s.max()), n_in, P, Q) > seam + span and s.min() + span < seam - span
    d_in = _dev(x)
    one = torch.full((n_out + 2, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    two = torch.full((n_out + 2, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rx.synthesize_grid(d_in.data_ptr(), 0, n_in, (P, Q), k, s, g, out_first, n_out, one.data_ptr(), 2)
    rx.synthesize_grid(d_in.data_ptr(), 0, n_in, (P, Q), k, s, g, out_first, seam - out_first, two.data_ptr(), 2)
    rx.synthesize_grid(d_in.data_ptr(), 0, n_in, (P, Q), k, s, g, seam, n_out - (seam - out_first), two.data_ptr() + 8 * (seam - out_first), 2)
    rx.synchronize()
    assert torch.equal(one, two)
    at = seam - span - out_first
    got = one[at:at + 2 * span].cpu().numpy()
    assert (one[n_out:] == SENTINEL).all().item() and np.abs(got).max() > 0.01
    _hold(got, x, P, Q, k, s, g, seam - span, 2 * span, "around the seam at %d" % seam)
    head = one[:int(s.min()) - out_first].view(torch.int32)
    assert not head.any().item()                                       # no row reaches the first chunk's outputs: +0


@pytest.mark.parametrize("p,q,D", [(2, 1, 2), (64, 1, 64), (128, 2, 64), (512, 1, 512)])
def test_a_power_of_two_is_the_grid_entry(rx, p, q, D):
    """q = 1 with p a power of two (after the reduction) gives the bytes of ofdmrx_util_synthesize_grid"""
    import torch
    n_in = 60
    k = np.array([-1, D - 1, -D, 0], np.int64)
    x = R.random_x(4, n_in, np.int16, seed=D)
    s, g = geometry(D, 1, k, seed=9, base=D)
    first, n_out = window_of(s, D, 1, n_in)
    d_in = _dev(x)
    a = torch.full((n_out + 2, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    b = torch.full((n_out + 2, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rx.synthesize_grid(d_in.data_ptr(), 0, n_in, (p, q), k, s, g, first, n_out, a.data_ptr(), 2)
    rx.synthesize_grid(d_in.data_ptr(), 0, n_in, D, k, s, g, first, n_out, b.data_ptr(), 2)
    rx.synchronize()
    assert torch.equal(a, b) and a[:n_out].abs().max().item() > 0.01 and (a[n_out:] == SENTINEL).all().item()


@pytest.mark.parametrize("P,Q", [(6, 1), (25, 4)], ids=["6/1", "25/4"])
def test_against_the_ratio_synthesizer(rx, P, Q):
    """the same rows through ofdmrx_util_synthesize_ratio at the slots' centres, starts and gains: within the sum of the two
    tolerances plus that entry's rounding of the phase increment, 2 pi 2^-33 m S[m]"""
    import torch
    n_in = 90
    k = subset(P, Q)
    x = R.random_x(len(k), n_in, np.int16, seed=17 * P)
    s, g = geometry(P, Q, k, seed=7, base=4 * P)
    first, n_out = window_of(s, P, Q, n_in)
    got, _ = _check(rx, x, P, Q, k, s, g, first, n_out, "against the ratio synthesizer")
    f = R.centres(P, Q, 8000, k)
    out = torch.full((n_out + 3, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    d_in = _dev(x)
    torch.cuda.synchronize()
    rx.synthesize(d_in.data_ptr(), 0, n_in, (P, Q), f, s, g, first, n_out, out.data_ptr(), 2)
    rx.synchronize()
    plain = out.cpu().numpy()
    assert (plain[n_out:] == SENTINEL).all()
    _, tol = R.grid(x, P, Q, k, s, g, out_first=first, n_out=n_out)
    v, ptol, tie = RS.synthesize(x, P, Q, f, s, g, 8000, out_first=first, n_out=n_out)
    assert tie > 1e-6 and RS.worst(plain[:n_out], v, ptol) <= 1.0
    S = tol / (2.0 ** -24 * R.tol_factor(2 * P))
    both = tol + ptol + 2 * np.pi * 2.0 ** -33 * (np.arange(n_out) + first) * S
    d = np.abs(got.astype(np.float64) - plain[:n_out].astype(np.float64)).max(axis=1)
    assert (d[both == 0] == 0).all()
    w = float((d[both > 0] / both[both > 0]).max())
    print("synthesize_grid %d/%d against ofdmrx_util_synthesize_ratio: worst |difference| / (tol + tol + increment) %.4f" % (P, Q, w))
    assert w <= 1.0


def test_ratio_grid_grid_and_plain_calls_interleaved_on_one_handle(rx):
    """nine calls - ratio-grid at 6/1, grid at 8, plain at 6/1 by turns, with other parameter arrays each (more than the ring of
    parameter sets holds), issued back to back and synchronized only after the last: each equals the same call on a handle of its
    own, as bytes.  Then one row in slot 0 at start 0 - whose parameter bytes are the same for the ratio-grid and the plain entry at
    6/1 - through both entries back to back: a ratio-grid set is not taken for a plain one, nor the reverse"""
    import modem_amd
    import torch
    n_in = 120
    x = R.random_x(3, n_in, np.int16, seed=19)
    d_in = _dev(x)
    k = np.array([-1, 2, 0], np.int64)
    kinds = [((6, 1), "grid"), (8, "grid"), (6, "plain")] * 3
    sets, wins = [], []
    for i, (ratio, _) in enumerate(kinds):
        P = ratio[0] if isinstance(ratio, tuple) else ratio
        s, g = geometry(P, 1, k, seed=30 + i, base=P * i)
        sets.append((s, g))
        wins.append(window_of(s, P, 1, n_in))
    outs = [torch.full((n + 2, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0") for _, n in wins]

    def call(r, i, out):
        (ratio, kind), (s, g), (first, n) = kinds[i], sets[i], wins[i]
        if kind == "grid":
            r.synthesize_grid(d_in.data_ptr(), 0, n_in, ratio, k, s, g, first, n, out.data_ptr(), 2)
        else:
            r.synthesize(d_in.data_ptr(), 0, n_in, ratio, k.astype(np.float64) * 4000.0, s, g, first, n, out.data_ptr(), 2)

    def same(r, grid, out):
        z, g1 = np.array([0], np.int64), np.array([0.25], np.float32)
        if grid:
            r.synthesize_grid(d_in.data_ptr(), 0, n_in, (6, 1), z, z, g1, 0, 500, out.data_ptr(), 2)
        else:
            r.synthesize(d_in.data_ptr(), 0, n_in, 6, np.array([0.0]), z, g1, 0, 500, out.data_ptr(), 2)

    again = [torch.full((502, 2), float(SENTINEL), dtype=torch.float32, device="cuda:0") for _ in range(4)]
    torch.cuda.synchronize()
    for i in range(9):
        call(rx, i, outs[i])
    for i in range(4):
        same(rx, i % 2 == 0, again[i])
    rx.synchronize()
    one = modem_amd.Receiver(device=0, chunk_frames=1)
    try:
        for i in range(9):
            want = torch.full_like(outs[i], float(SENTINEL))
            torch.cuda.synchronize()
            call(one, i, want)
            one.synchronize()
            assert (outs[i][wins[i][1]:] == SENTINEL).all().item() and torch.equal(outs[i], want), i
        for grid in (True, False):
            one.close()
            one = modem_amd.Receiver(device=0, chunk_frames=1)        # (a fresh handle: its first set)
            want = torch.full_like(again[0], float(SENTINEL))
            torch.cuda.synchronize()
            same(one, grid, want)
            one.synchronize()
            assert torch.equal(again[0 if grid else 1], want) and torch.equal(again[2 if grid else 3], want), grid
    finally:
        one.close()
    assert not torch.equal(again[0], again[1])                         # (the two entries do differ in their last bits or more)


def test_refusals_leave_the_output_untouched(rx):
    """every argument the header names is refused with OFDMRX_E_ARG before anything runs; buffers that merely touch are accepted"""
    import torch
    P, Q, n_in = 25, 4, 100
    k = np.array([3, -6], np.int32)
    x = R.random_x(2, n_in, np.int16, seed=17)
    s, g = np.array([50, 0], np.int64), np.array([0.3, -0.2], np.float32)
    n_out = R.n_outputs(s, n_in, P, Q)
    in_bytes = 2 * n_in * 4
    buf = torch.full((in_bytes + n_out * 8 + 64,), 77, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    assert base % 8 == 0 and in_bytes % 8 == 0
    d_in, d_out = base, base + in_bytes                               # the input right before the output
    buf[:in_bytes] = _dev(x.view(np.uint8).reshape(-1))
    before = buf.clone()
    torch.cuda.synchronize()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(d_in=d_in, ifmt=0, stride=n_in, n_in=n_in, pq=(P, Q), sl=k, st=s, gn=g, n=2, out_first=0, n_out=n_out, d_out=d_out, ofmt=2):
        return rx._lib.ofdmrx_util_synthesize_grid_ratio(rx._h, d_in, ifmt, stride, n_in, pq[0], pq[1], p(sl), p(st), p(gn), n, out_first, n_out, d_out, ofmt)

    assert call(d_in=None) == -1 and call(d_out=None) == -1 and call(st=None) == -1 and call(gn=None) == -1
    assert call(n_in=0) == -1 and call(n_out=0) == -1 and call(n=0) == -1 and call(n=14) == -1       # (n_all is 13)
    assert call(sl=None) == -1 and call(sl=None, n=12) == -1
    for bad in ((0, 1), (1, 0), (-25, 4), (25, -4), (7, 1), (14, 4), (3, 2), (1, 1), (1024, 1), (513, 1), (512, 17), (77, 2)):
        assert call(pq=bad) == -1, bad
    for bad in (7, -7, 3):                                             # outside -6 .. 6; given twice
        assert call(sl=np.array([3, bad], np.int32)) == -1, bad
    for bad in (-25, 1, 24, 4, 30):                                    # negative; not on the grid of P
        assert call(st=np.array([50, bad], np.int64)) == -1, bad
    assert call(st=np.array([50, (1 << 50) // 25 * 25 + 25], np.int64)) == -1
    assert call(ifmt=-1) == -1 and call(ifmt=1) == -1 and call(ifmt=3) == -1
    assert call(ofmt=-1) == -1 and call(ofmt=1) == -1 and call(ofmt=3) == -1
    assert call(stride=n_in - 1) == -1 and call(out_first=-1) == -1 and call(out_first=(1 << 50) + 1) == -1
    for bad in (float("nan"), float("inf"), -float("inf"), 3e38):
        assert call(gn=np.array([1.0, bad], np.float32)) == -1, bad
    assert call(n_out=(1 << 41) - 1023) == -1                          # the bound on n_out: 2^41 - 1024
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
    assert call(pq=(50, 8)) == 0                                      # the ratio is reduced by the entry
    rx.synchronize()
    assert torch.equal(buf[:in_bytes], before[:in_bytes])
    got = buf[in_bytes:in_bytes + n_out * 8].cpu().numpy().view(np.float32).reshape(n_out, 2)
    _hold(got, x, P, Q, k, s, g, 0, n_out, "adjacent buffers")
    assert (buf[in_bytes + n_out * 8:] == 77).all()
