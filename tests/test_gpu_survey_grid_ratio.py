"""The grid survey at a ratio on the device (k_survey_grid_ratio.hip behind ofdmrx_util_survey_grid_ratio) against the float64 model
of survey_grid_ratio_model.py: |got - P| <= tol on every slot of every row, nothing exempt; the tolerance is
derived in the model's header.  Input is full scale in sum: random values plus a tone on a slot centre.  Unless a test says otherwise
the buffer starts exactly at the first position its rows need and ends at the last.  Each test prints its worst |got - P| / tol
(profiles/survey_grid_ratio_parity.txt keeps them)."""
import numpy as np
import pytest

import channelize_grid_ratio_model as GR
import survey_grid_ratio_model as SR

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
# 3/1: M = 6, 256 times per tile; 5/1; 6/1: 12 slots; 9/4, 45/16, 512/3: open ends; 15/2: Q = 2, cyclic; 25/4: 13 slots; 125/4: 16 times
# per tile; 300/1: 8 times; 500/1 and 512/3: the 8-time tile with more than 64 KiB of LDS
RATIOS = ((3, 1), (5, 1), (6, 1), (9, 4), (15, 2), (25, 4), (45, 16), (125, 4), (300, 1), (500, 1), (512, 3))
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


def tile(P):
    """the survey kernel's tile of output times: the front end's (4096 points, 8 .. 256 times, 61440 bytes of LDS with the i_n mod M
    array, even) rounded down to a multiple of 8, and 8 where that leaves nothing"""
    M = 2 * P
    nt = min(max(4096 // M, 8), 256, (61440 - 8 * M) // (8 * M + 4)) & ~1
    return max(8, nt & ~7)


def test_tile_restated():
    assert [tile(P) for P in (3, 6, 25, 125, 300, 400, 432, 500, 512)] == [256, 256, 80, 16, 8, 8, 8, 8, 8]
    assert 2 * 500 * 9 * 8 > 65536 and 2 * 512 * 9 * 8 == 73728


def _input(P, Q, S, row_first, n_rows, dtype=np.int16, seed=1, slot=1):
    first, count = SR.span(P, Q, S, row_first, n_rows)
    return SR.tone_pcm(count, P, Q, slot, dtype, seed=seed, first=first), first


def _run(rx, pcm, P, Q, S, row_first, n_rows, in_first):
    got = rx.survey_grid(_dev(pcm), FMT[pcm.dtype], (P, Q), S, in_first=in_first, row_first=row_first, n_rows=n_rows).cpu().numpy()
    assert got.shape == (n_rows, GR.slot_range(P, Q)[1]) and got.dtype == np.float32
    return got


def _check(rx, P, Q, S, row_first, n_rows, what="", dtype=np.int16, seed=1):
    pcm, first = _input(P, Q, S, row_first, n_rows, dtype, seed)
    got = _run(rx, pcm, P, Q, S, row_first, n_rows, first)
    Pw, tol = SR.power(pcm, P, Q, S, row_first, n_rows, in_first=first)
    assert np.isfinite(got).all() and (tol > 0).all()
    w = SR.worst(got, Pw, tol)
    print("survey_grid_ratio %d/%d S %d rows %d.. x %d %s: worst |got - P| / tol %.4f" % (P, Q, S, row_first, n_rows, what, w))
    assert w <= 1.0, (P, Q, S, row_first, n_rows, what, w)
    return got, w


@pytest.mark.parametrize("P,Q", RATIOS)
def test_shapes_match_model(rx, P, Q):
    """S = 8; S = 16 with 3 rows; S = the tile and the tile + 8 (a row boundary inside a tile); n_rows 1 and 5, row_first 0 and 3"""
    NT = tile(P)
    shapes = [(8, 0, 1), (8, 3, 5), (16, 0, 3), (NT, 0, 1), (NT, 3, 5), (NT + 8, 0, 1), (NT + 8, 3, 5), (NT + 8, 0, 5)]
    worst = 0.0
    for S, row_first, n_rows in shapes:
        worst = max(worst, _check(rx, P, Q, S, row_first, n_rows, seed=S)[1])
    print("survey_grid_ratio %d/%d, all shapes: worst %.4f" % (P, Q, worst))


@pytest.mark.parametrize("P,Q", [(6, 1), (25, 4)])
@pytest.mark.parametrize("S", [504, 512, 8200])
def test_long_rows(rx, P, Q, S):
    """63, 64 and 1025 groups per row: the rows kernel's batches of 32 and 8 loads and its tail (one rows kernel: there is no
    staged variant to agree with)"""
    _check(rx, P, Q, S, 1, 2, "long", seed=5)


@pytest.mark.parametrize("P,Q", [(6, 1), (25, 4)])
def test_formats(rx, P, Q):
    """S16, U8 and F32 input; F32 input scaled by 2^6 gives exactly the outputs scaled by 2^12"""
    S = tile(P) + 8
    for dt in (np.int16, np.uint8, np.float32):
        _check(rx, P, Q, S, 1, 2, np.dtype(dt).name, dtype=dt, seed=3)
    x, first = _input(P, Q, S, 1, 2, np.float32, seed=4)
    a = _run(rx, x, P, Q, S, 1, 2, first)
    b = _run(rx, x * np.float32(64.0), P, Q, S, 1, 2, first)
    assert (b == a * np.float32(4096.0)).all()


@pytest.mark.parametrize("P,Q", [(25, 4), (6, 1)])
def test_far_position(rx, P, Q):
    """rows beyond position 2^40"""
    S = 64
    row_first = (2 ** 40 * Q) // (S * P) + 2
    assert SR.span(P, Q, S, row_first, 2)[0] > 2 ** 40
    _check(rx, P, Q, S, row_first, 2, "far", seed=6)


@pytest.mark.parametrize("P,Q", [(3, 1), (25, 4), (512, 3)])
def test_zero_input_gives_plus_zero(rx, P, Q):
    S = tile(P) + 8
    first, count = SR.span(P, Q, S, 0, 3)
    for dt in (np.int16, np.float32):
        got = _run(rx, np.zeros((count, 2), dt), P, Q, S, 0, 3, first)
        assert (got.view(np.uint32) == 0).all()


@pytest.mark.parametrize("P,Q", [(6, 1), (25, 4), (500, 1)])
def test_one_call_equals_row_by_row(rx, P, Q):
    """no state: the rows 0 .. 4 in one call against the same rows one call each, every call given only the positions its row needs"""
    S = tile(P) + 8
    n_rows = 5
    pcm, first = _input(P, Q, S, 0, n_rows, seed=8)
    assert first == 0
    whole, _ = _check(rx, P, Q, S, 0, n_rows, "whole", seed=8)
    for r in range(n_rows):
        f, c = SR.span(P, Q, S, r, 1)
        one = _run(rx, pcm[f:f + c], P, Q, S, r, 1, f)
        assert one.tobytes() == whole[r:r + 1].tobytes(), r


@pytest.mark.parametrize("D", [8, 64])
def test_power_of_two_is_the_grid_survey(rx, D):
    """q = 1 with p a power of two: ofdmrx_util_survey_grid's bytes (also from an unreduced 2 D / 2)"""
    import survey_grid_model as SG
    S, n_rows = 72, 3
    first, count = SG.span(D, S, 1, n_rows)
    assert (first, count) == SR.span(D, 1, S, 1, n_rows)
    pcm = SG.tone_pcm(count, D, 1, seed=14, first=first)
    d = _dev(pcm)
    want = rx.survey_grid(d, 0, D, S, in_first=first, row_first=1, n_rows=n_rows).cpu().numpy()
    for ratio in ((D, 1), (2 * D, 2)):
        got = rx.survey_grid(d, 0, ratio, S, in_first=first, row_first=1, n_rows=n_rows).cpu().numpy()
        assert got.shape == (n_rows, 2 * D) and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("P,Q", [(6, 1), (25, 4)])
def test_buffer_larger_than_the_span(rx, P, Q):
    """a buffer that starts before the span and ends behind it gives the same bytes; a sentinel behind the last row stays"""
    import torch
    S, n_rows, r0 = 24, 3, 2
    first, count = SR.span(P, Q, S, r0, n_rows)
    assert first > 7
    big = SR.tone_pcm(count + 7 + 11, P, Q, 1, seed=15, first=first - 7)
    exact = _run(rx, big[7:7 + count], P, Q, S, r0, n_rows, first)
    Pw, tol = SR.power(big[7:7 + count], P, Q, S, r0, n_rows, in_first=first)
    assert SR.worst(exact, Pw, tol) <= 1.0
    n_all = GR.slot_range(P, Q)[1]
    out = torch.full((n_rows + 1, n_all), SENTINEL, dtype=torch.float32, device="cuda:0")
    d = _dev(big)
    torch.cuda.synchronize()
    assert rx._lib.ofdmrx_util_survey_grid_ratio(rx._h, d.data_ptr(), 0, first - 7, len(big), P, Q, S, r0, n_rows, out.data_ptr()) == 0
    rx.synchronize()
    got = out.cpu().numpy()
    assert got[:n_rows].tobytes() == exact.tobytes() and (got[n_rows] == SENTINEL).all()


def test_tables_do_not_mix(rx):
    """the table key: the front end on two slots, the survey, the front end again - identical bytes, each equal to a fresh handle's;
    the same around a power-of-two grid call"""
    import modem_amd
    import torch
    P, Q, S, n_rows = 25, 4, 24, 3
    pcm, first = _input(P, Q, S, 0, n_rows, seed=10)
    n_out = S * n_rows
    slots = [3, -6]
    d_in = _dev(pcm)

    def front(r, decim=(P, Q), k=slots, n=n_out):
        out = torch.full((len(k), n, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        r.channelize_grid(d_in.data_ptr(), 0, 0, len(pcm), decim, k, 0, n, out.data_ptr())
        r.synchronize()
        return out.cpu().numpy().tobytes()

    def pow2(r):
        return front(r, 8, [1, -8], n_out // 2)

    def survey(r):
        return _run(r, pcm, P, Q, S, 0, n_rows, 0).tobytes()

    want = {}
    for name, fn in (("survey", survey), ("front", front), ("pow2", pow2)):
        fresh = modem_amd.Receiver(device=0, chunk_frames=1)
        try:
            want[name] = fn(fresh)
        finally:
            fresh.close()
    Pw, tol = SR.power(pcm, P, Q, S, 0, n_rows)
    assert SR.worst(np.frombuffer(want["survey"], np.float32).reshape(n_rows, -1), Pw, tol) <= 1.0
    for name, fn in (("front", front), ("survey", survey), ("front", front), ("survey", survey), ("pow2", pow2), ("survey", survey),
                     ("pow2", pow2), ("front", front)):
        assert fn(rx) == want[name], name


def test_identity_with_the_ratio_front_end(rx):
    """P = mean |channelize_grid at the ratio|^2 on the device's own rows, within the sum of both tolerances (as 4.21's test)"""
    import torch
    P, Q = 25, 4
    S, n_rows = tile(P) + 8, 3
    n_all = GR.slot_range(P, Q)[1]
    pcm, first = _input(P, Q, S, 0, n_rows, seed=11)
    got = _run(rx, pcm, P, Q, S, 0, n_rows, 0)
    n_out = S * n_rows
    out = torch.full((n_all, n_out, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    d_in = _dev(pcm)
    torch.cuda.synchronize()
    rx.channelize_grid(d_in.data_ptr(), 0, 0, len(pcm), (P, Q), None, 0, n_out, out.data_ptr())
    rx.synchronize()
    y = out.cpu().numpy().astype(np.float64)
    Pc = (y[..., 0] ** 2 + y[..., 1] ** 2).reshape(n_all, n_rows, S).mean(axis=2).T
    Pw, tol = SR.power(pcm, P, Q, S, 0, n_rows)
    c = (8 + S / 8 + 4) * SR.U
    first_term = (tol - c * Pw) / (1 + c)                            # tol = first + c (P + first)
    assert (first_term > 0).all()
    w = float(np.max(np.abs(got - Pc) / (tol + first_term)))
    print("survey_grid_ratio %d/%d against mean |channelize_grid|^2: worst |difference| / (tol + tol) %.4f" % (P, Q, w))
    assert w <= 1.0


def test_refusals_leave_the_output_untouched(rx):
    """every argument the header names is refused with OFDMRX_E_ARG before anything runs; buffers that merely touch are accepted"""
    import torch
    P, Q, S, n_rows = 25, 4, 64, 2
    n_all = GR.slot_range(P, Q)[1]
    W = ((n_rows * S - 1) * P) // Q + 1
    assert (0, W) == SR.span(P, Q, S, 0, n_rows)
    out_bytes = n_rows * n_all * 4
    buf = torch.full((W * 4 + out_bytes + 64,), 77, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    assert base % 8 == 0
    d_in, d_out = base, base + 4 * W                                 # the input right before the output
    pcm = SR.tone_pcm(W, P, Q, 1, seed=12)
    buf[:4 * W] = _dev(pcm.view(np.uint8).reshape(-1))
    before = buf.clone()
    torch.cuda.synchronize()

    def call(d_in=d_in, fmt=0, in_first=0, n_in=W, p=P, q=Q, S=S, row_first=0, n_rows=n_rows, d_out=d_out):
        return rx._lib.ofdmrx_util_survey_grid_ratio(rx._h, d_in, fmt, in_first, n_in, p, q, S, row_first, n_rows, d_out)

    assert call(d_in=None) == -1 and call(d_out=None) == -1
    assert call(n_in=0) == -1 and call(n_rows=0) == -1
    for bad in ((0, 1), (25, 0), (-25, 4), (25, -4), (7, 1), (25, 13), (3, 2), (17, 16), (513, 1), (1024, 1), (600, 1), (77, 4)):
        assert call(p=bad[0], q=bad[1]) == -1, bad
    for bad in (0, 4, 12, 63, 65, 65544, -8):
        assert call(S=bad) == -1, bad
    assert call(fmt=-1) == -1 and call(fmt=3) == -1
    assert call(in_first=-1) == -1 and call(row_first=-1) == -1
    assert call(n_in=W - 1) == -1 and call(n_rows=n_rows + 1) == -1           # the last time's position is not there
    assert call(in_first=1, n_in=W - 1, d_in=d_in + 4) == -1                  # rows from 0 need position 0
    f1, c1 = SR.span(P, Q, S, 1, 1)
    assert f1 > 0 and f1 + c1 == W
    assert call(row_first=1, n_rows=1, in_first=f1 + 1, n_in=c1 - 1, d_in=d_in + 4 * (f1 + 1)) == -1   # one position of history missing
    assert call(p=512, q=1, S=65536, n_rows=33) == -1 and call(p=500, q=1, S=65536, n_rows=40) == -1   # (also too many partials)
    for off in (4, 4 * W - 4, -4, -out_bytes + 4):                            # the output overlaps the input, from either side
        assert call(d_out=d_in + off) == -1, off
    assert call(d_in=d_in + 2) == -1 and call(d_out=d_out + 2) == -1          # off the sample-frame boundary / off 4 bytes
    bank = rx.wideband_grid_bank([0], (P, Q))                                  # a live handle
    try:
        assert call() == -1
    finally:
        while bank.open:
            bank.end()
    rx.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    assert call(row_first=1, n_rows=1, in_first=f1, n_in=c1, d_in=d_in + 4 * f1, d_out=d_out + n_all * 4) == 0   # just inside
    rx.synchronize()
    row1 = buf[4 * W + n_all * 4:4 * W + out_bytes].cpu().numpy().view(np.float32).copy()
    assert (buf[4 * W:4 * W + n_all * 4] == 77).all()
    assert call() == 0                                                # adjacent buffers (the same stream: it runs second)
    rx.synchronize()
    assert torch.equal(buf[:4 * W], before[:4 * W])
    got = buf[4 * W:4 * W + out_bytes].cpu().numpy().view(np.float32).reshape(n_rows, n_all)
    Pw, tol = SR.power(pcm, P, Q, S, 0, n_rows)
    assert SR.worst(got, Pw, tol) <= 1.0 and got[1].tobytes() == row1.tobytes()
    assert (buf[4 * W + out_bytes:] == 77).all()
