"""The grid survey on the device (k_survey_grid.hip behind ofdmrx_util_survey_grid) against the float64 model of
survey_grid_model.py: |got - P| <= tol on every slot of every row, nothing exempt; the tolerance is derived
in the model's header.  Input is full scale in sum: random values plus a tone on a slot centre.  Unless a test says otherwise the
buffer starts exactly at the first position its rows need and ends at the last.  Each test prints its worst |got - P| / tol
(profiles/survey_grid_parity.txt keeps them)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import channelize_grid_model as G
import survey_grid_model as SG

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
# M = 4: 1024 times per tile, 128 groups; 8; 64: 64 times per tile, where the transform's lanes switch to the time axis; 128: 32 times;
# 256: runs of 8 times; 1024: 8 times, one group per tile, 72 KiB of LDS
DS = (2, 4, 32, 64, 128, 512)
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


def _input(D, S, row_first, n_rows, dtype=np.int16, seed=1, slot=1):
    first, count = SG.span(D, S, row_first, n_rows)
    return SG.tone_pcm(count, D, slot, dtype, seed=seed, first=first), first


def _run(rx, pcm, D, S, row_first, n_rows, in_first):
    got = rx.survey_grid(_dev(pcm), FMT[pcm.dtype], D, S, in_first=in_first, row_first=row_first, n_rows=n_rows).cpu().numpy()
    assert got.shape == (n_rows, 2 * D) and got.dtype == np.float32
    return got


def _check(rx, D, S, row_first, n_rows, what="", dtype=np.int16, seed=1):
    pcm, first = _input(D, S, row_first, n_rows, dtype, seed)
    got = _run(rx, pcm, D, S, row_first, n_rows, first)
    P, tol = SG.power(pcm, D, S, row_first, n_rows, in_first=first)
    assert np.isfinite(got).all() and (tol > 0).all()
    w = SG.worst(got, P, tol)
    print("survey_grid M %d S %d rows %d.. x %d %s: worst |got - P| / tol %.4f" % (2 * D, S, row_first, n_rows, what, w))
    assert w <= 1.0, (D, S, row_first, n_rows, what, w)
    return got, w


@pytest.mark.parametrize("D", DS)
def test_shapes_match_model(rx, D):
    """S = 8; S = 16 with 3 rows; S = the tile and the tile + 8 (a row boundary inside a tile); n_rows 1 and 5, row_first 0 and 3"""
    NT = tile(D)
    shapes = [(8, 0, 1), (8, 3, 5), (16, 0, 3), (NT, 0, 1), (NT, 3, 5), (NT + 8, 0, 1), (NT + 8, 3, 5), (NT + 8, 0, 5)]
    if D == 2:
        shapes.append((1032, 3, 5))
    worst = 0.0
    for S, row_first, n_rows in shapes:
        worst = max(worst, _check(rx, D, S, row_first, n_rows, seed=S)[1])
    print("survey_grid M %d, all shapes: worst %.4f" % (2 * D, worst))


@pytest.mark.parametrize("D,S", [(4, 504), (4, 512), (2, 8200), (16, 1024), (16, 2056), (32, 2056)])
def test_long_rows(rx, D, S):
    """the second launch takes another kernel for M <= 32 from 64 groups per row on (S = 512), which passes a row's partials through
    LDS in chunks of 4096 floats: one group below the threshold and at it; 1025 groups at M = 4 (a chunk and one group); one chunk
    exactly and 257 groups at M = 32 (two chunks and one group); M = 64 at that length takes the plain kernel"""
    _check(rx, D, S, 1, 2, "long", seed=5)


@pytest.mark.parametrize("D", [4, 64])
def test_formats(rx, D):
    """S16, U8 and F32 input; F32 input scaled by 2^6 gives exactly the outputs scaled by 2^12"""
    S = tile(D) + 8
    for dt in (np.int16, np.uint8, np.float32):
        _check(rx, D, S, 1, 2, np.dtype(dt).name, dtype=dt, seed=3)
    x, first = _input(D, S, 1, 2, np.float32, seed=4)
    a = _run(rx, x, D, S, 1, 2, first)
    b = _run(rx, x * np.float32(64.0), D, S, 1, 2, first)
    assert (b == a * np.float32(4096.0)).all()


def test_far_position(rx):
    """positions above 2^40: rows from row_first S D ~ 2^40 on"""
    D, S = 64, 64
    row_first = 2 ** 40 // (S * D) + 1
    assert SG.span(D, S, row_first, 2)[0] > 2 ** 40
    _check(rx, D, S, row_first, 2, "far", seed=6)
    _check(rx, 2, 1032, 2 ** 40 // (1032 * 2) + 1, 2, "far", seed=7)


@pytest.mark.parametrize("D", [2, 64, 512])
def test_zero_input_gives_plus_zero(rx, D):
    S = tile(D) + 8
    first, count = SG.span(D, S, 0, 3)
    for dt in (np.int16, np.float32):
        got = _run(rx, np.zeros((count, 2), dt), D, S, 0, 3, first)
        assert (got.view(np.uint32) == 0).all()


@pytest.mark.parametrize("D", [2, 32, 512])
def test_one_call_equals_row_by_row(rx, D):
    """no state: the rows 0 .. 4 in one call against the same rows one call each, every call given only the positions its row needs"""
    S = tile(D) + 8
    n_rows = 5
    pcm, first = _input(D, S, 0, n_rows, seed=8)
    assert first == 0
    whole, _ = _check(rx, D, S, 0, n_rows, "whole", seed=8)
    for r in range(n_rows):
        f, c = SG.span(D, S, r, 1)
        one = _run(rx, pcm[f:f + c], D, S, r, 1, f)
        assert one.tobytes() == whole[r:r + 1].tobytes(), r


def test_two_decimations_back_to_back(rx):
    a1, _ = _check(rx, 8, 24, 1, 2, "first", seed=9)
    b1, _ = _check(rx, 64, 40, 1, 2, "second", seed=9)
    a2, _ = _check(rx, 8, 24, 1, 2, "third", seed=9)
    b2, _ = _check(rx, 64, 40, 1, 2, "fourth", seed=9)
    assert a1.tobytes() == a2.tobytes() and b1.tobytes() == b2.tobytes()


def test_tables_do_not_mix(rx):
    """survey_grid between channelize_grid calls and a plain channelize call at the same D on one handle: each equals, byte for
    byte, what a fresh handle gives"""
    import modem_amd
    import torch
    D, S, n_rows = 8, 24, 3
    pcm, first = _input(D, S, 0, n_rows, seed=10)
    n_out = S * n_rows
    slots = [3, -8, 0]
    f = modem_amd.grid_centres(D, 8000, slots)
    d_in = _dev(pcm)

    def grid(r):
        out = torch.full((3, n_out, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        r.channelize_grid(d_in.data_ptr(), 0, 0, len(pcm), D, slots, 0, n_out, out.data_ptr())
        r.synchronize()
        return out.cpu().numpy().tobytes()

    def plain(r):
        out = torch.full((3, n_out, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        r.channelize(d_in.data_ptr(), 0, 0, len(pcm), D, f, 0, n_out, out.data_ptr())
        r.synchronize()
        return out.cpu().numpy().tobytes()

    def survey(r):
        return _run(r, pcm, D, S, 0, n_rows, 0).tobytes()

    want = {}
    for name, fn in (("survey", survey), ("grid", grid), ("plain", plain)):
        fresh = modem_amd.Receiver(device=0, chunk_frames=1)
        try:
            want[name] = fn(fresh)
        finally:
            fresh.close()
    P, tol = SG.power(pcm, D, S, 0, n_rows)
    assert SG.worst(np.frombuffer(want["survey"], np.float32).reshape(n_rows, 2 * D), P, tol) <= 1.0
    for name, fn in (("survey", survey), ("grid", grid), ("survey", survey), ("plain", plain), ("survey", survey), ("grid", grid),
                     ("plain", plain), ("survey", survey)):
        assert fn(rx) == want[name], name


@pytest.mark.parametrize("D", [4, 32])
def test_identity_with_the_grid_front_end(rx, D):
    """P = mean |channelize_grid|^2 on the device's own rows, within the sum of both tolerances: the survey's, and what section
    4.19's bound on the front end's outputs allows their mean power (the first term of the survey's rule)"""
    import torch
    S, n_rows = tile(D) + 8, 3
    pcm, first = _input(D, S, 0, n_rows, seed=11)
    got = _run(rx, pcm, D, S, 0, n_rows, 0)
    n_out = S * n_rows
    out = torch.full((2 * D, n_out, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    d_in = _dev(pcm)
    torch.cuda.synchronize()
    rx.channelize_grid(d_in.data_ptr(), 0, 0, len(pcm), D, None, 0, n_out, out.data_ptr())
    rx.synchronize()
    y = out.cpu().numpy().astype(np.float64)
    Pc = (y[..., 0] ** 2 + y[..., 1] ** 2).reshape(2 * D, n_rows, S).mean(axis=2).T
    P, tol = SG.power(pcm, D, S, 0, n_rows)
    c = (8 + S / 8 + 4) * SG.U
    first_term = (tol - c * P) / (1 + c)                             # tol = first + c (P + first)
    assert (first_term > 0).all()
    w = float(np.max(np.abs(got - Pc) / (tol + first_term)))
    print("survey_grid M %d against mean |channelize_grid|^2: worst |difference| / (tol + tol) %.4f" % (2 * D, w))
    assert w <= 1.0


def _round_fp32(e):
    """the fp32 nearest the rational e, ties to even: the better of the neighbours of a first guess, which lies within one step"""
    c = np.float32(float(e))
    cands = (c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf)))
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - e), int(v.view(np.uint32)) & 1))


def _power_fp32_exact(y):
    """fma(im, im, re re) as the kernel forms it: re re rounded to fp32, then im im + that formed exactly and rounded once (float64
    would round twice)"""
    rr = y[..., 0] * y[..., 0]
    assert rr.dtype == np.float32
    p = [_round_fp32(Fraction(im) * Fraction(im) + Fraction(a)) for im, a in zip(y[..., 1].ravel().tolist(), rr.ravel().tolist())]
    return np.array(p, np.float32).reshape(rr.shape)


@pytest.mark.parametrize("D", [2, 32, 128])
def test_bytes_follow_from_the_grid_front_end(rx, D):
    """the survey's steps 1 and 2 are the front end's code (grid_bank.h), so its rows are a function of the front end's bytes:
    channelize_grid over all slots and survey_grid on one device buffer, then on the host |y|^2 = fma(im, im, re re), the fp32 chain
    over the 8 times of a group, the fp32 chain over a row's groups and the product with fp32(1 / S), in the order section 4.21
    fixes - byte for byte.  M = 4: lanes along the time axis in the transform; 64: one point per lane; 256: the instantiation with
    the most registers"""
    import torch
    S, n_rows = tile(D) + 8, 3
    pcm, first = _input(D, S, 0, n_rows, seed=13)
    assert first == 0
    n_out = S * n_rows
    d_in = _dev(pcm)
    out = torch.full((2 * D, n_out, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rx.channelize_grid(d_in.data_ptr(), 0, 0, len(pcm), D, None, 0, n_out, out.data_ptr())
    got = rx.survey_grid(d_in, 0, D, S, in_first=0, row_first=0, n_rows=n_rows).cpu().numpy()
    rx.synchronize()
    assert got.shape == (n_rows, 2 * D) and got.dtype == np.float32
    p = _power_fp32_exact(out.cpu().numpy()).reshape(2 * D, n_rows, S // 8, 8)    # [slot][row][group][time]
    grp = p[..., 0]
    for t in range(1, 8):
        grp = grp + p[..., t]
    row = grp[..., 0]
    for g in range(1, S // 8):
        row = row + grp[..., g]
    want = np.ascontiguousarray((row * np.float32(1.0 / S)).T)
    assert want.dtype == np.float32
    print("survey_grid M %d from channelize_grid's bytes: %d of %d values differ" % (2 * D, int((want.view(np.uint32) != got.view(np.uint32)).sum()), want.size))
    assert want.tobytes() == got.tobytes()


def test_refusals_leave_the_output_untouched(rx):
    """every argument the header names is refused with OFDMRX_E_ARG before anything runs; buffers that merely touch are accepted"""
    import torch
    D, S, n_rows = 16, 64, 2
    W = (n_rows * S - 1) * D + 1
    out_bytes = n_rows * 2 * D * 4
    buf = torch.full((W * 4 + out_bytes + 64,), 77, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    assert base % 8 == 0
    d_in, d_out = base, base + 4 * W                                 # the input right before the output
    pcm = SG.tone_pcm(W, D, 1, seed=12)
    buf[:4 * W] = _dev(pcm.view(np.uint8).reshape(-1))
    before = buf.clone()
    torch.cuda.synchronize()

    def call(d_in=d_in, fmt=0, in_first=0, n_in=W, decim=D, S=S, row_first=0, n_rows=n_rows, d_out=d_out):
        return rx._lib.ofdmrx_util_survey_grid(rx._h, d_in, fmt, in_first, n_in, decim, S, row_first, n_rows, d_out)

    assert call(d_in=None) == -1 and call(d_out=None) == -1
    assert call(n_in=0) == -1 and call(n_rows=0) == -1
    for bad in (0, 1, 3, 12, 48, 1024, -16):
        assert call(decim=bad) == -1, bad
    for bad in (0, 4, 12, 63, 65, 65544, -8):
        assert call(S=bad) == -1, bad
    assert call(fmt=-1) == -1 and call(fmt=3) == -1
    assert call(in_first=-1) == -1 and call(row_first=-1) == -1
    assert call(n_in=W - 1) == -1 and call(n_rows=n_rows + 1) == -1           # the last time's position is not there
    assert call(in_first=1, n_in=W - 1, d_in=d_in + 4) == -1                  # rows from 0 need position 0
    assert call(row_first=1, n_rows=1, in_first=(S - 24) * D + 1, n_in=W - (S - 24) * D - 1, d_in=d_in + 4 * ((S - 24) * D + 1)) == -1
    assert call(decim=512, S=65536, n_rows=33) == -1                          # (also too many partials)
    for off in (4, 4 * W - 4, -4, -out_bytes + 4):                            # the output overlaps the input, from either side
        assert call(d_out=d_in + off) == -1, off
    assert call(d_in=d_in + 2) == -1 and call(d_out=d_out + 2) == -1          # off the sample-frame boundary / off 4 bytes
    bank = rx.wideband_grid_bank([0], D)                                       # a live handle
    try:
        assert call() == -1
    finally:
        while bank.open:
            bank.end()
    rx.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    f1 = (S - 24) * D
    assert call(row_first=1, n_rows=1, in_first=f1, n_in=W - f1, d_in=d_in + 4 * f1, d_out=d_out + 2 * D * 4) == 0   # just inside
    rx.synchronize()
    row1 = buf[4 * W + 2 * D * 4:4 * W + out_bytes].cpu().numpy().view(np.float32).copy()
    assert (buf[4 * W:4 * W + 2 * D * 4] == 77).all()
    assert call() == 0                                                # adjacent buffers (the same stream: it runs second)
    rx.synchronize()
    assert torch.equal(buf[:4 * W], before[:4 * W])
    got = buf[4 * W:4 * W + out_bytes].cpu().numpy().view(np.float32).reshape(n_rows, 2 * D)
    P, tol = SG.power(pcm, D, S, 0, n_rows)
    assert SG.worst(got, P, tol) <= 1.0 and got[1].tobytes() == row1.tobytes()
    assert (buf[4 * W + out_bytes:] == 77).all()
