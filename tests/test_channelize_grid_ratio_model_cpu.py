"""The grid front end at a ratio without a GPU: the float64 model of channelize_grid_ratio_model.py against
its own direct sum, against section 4.17's model at the slot centres and against section 4.19's model where Q = 1 and P is a power of
two; the library's taps and slot range, the tolerance rule on an fp32 evaluation of the plan and on deliberately wrong models, the
argument errors that need no look into the handle, and the captures of grid_ratio_fixture.py through the oracle on the model's rows -
which fixes what test_gpu_grid_ratio_bank.py expects."""
import ctypes as C
import os

import numpy as np
import pytest

import channelize_grid_model as G
import channelize_grid_ratio_model as R
import grid_ratio_fixture as GF
import rechannelize_model as RM

E_ARG = -1
NAMES = ("ofdmrx_util_channelize_grid_ratio_taps", "ofdmrx_util_grid_ratio_slots", "ofdmrx_util_channelize_grid_ratio",
         "ofdmrx_bank_begin_wideband_grid_ratio")
RATIOS = ((3, 1), (5, 1), (6, 1), (9, 4), (15, 2), (25, 4), (45, 16), (75, 2), (125, 4), (300, 1), (500, 1), (512, 3))
IDS = ["%d/%d" % r for r in RATIOS]


@pytest.fixture(scope="module")
def lib():
    import modem_amd
    modem_amd.build()
    return modem_amd.load_library()


def _S(tol, P):
    return tol / (2.0 ** -24 * R.tol_factor(2 * P))


def test_symbols_exported_and_declared(lib):
    import fractions
    import modem_amd
    import modem_amd.ofdmrx as M
    text = open(os.path.join(os.path.dirname(M.HERE), "include", "ofdmrx.h")).read()
    for name in NAMES:
        assert name in M.EXPORTS
        getattr(lib, name)
        assert name + "(" in text and name in text.split("#define OFDMRX_ABI_MINOR")[0]
    assert lib.ofdmrx_abi_minor() == 9                               # additions within 1.9: detected by symbol
    assert (modem_amd.grid_centres((6, 1), 8000) == np.arange(-6, 6) * 4000.0).all()
    assert (modem_amd.grid_centres(fractions.Fraction(25, 4), 8000) == np.arange(-6, 7) * 4000.0).all()
    assert (modem_amd.grid_centres((50, 8), 8000, [6, -6]) == [24000.0, -24000.0]).all()
    assert (modem_amd.grid_centres(8, 8000) == modem_amd.grid_centres((8, 1), 8000)).all()
    for bad in ((7, 1), (3, 2), (513, 1), (36, 17)):
        with pytest.raises(modem_amd.OfdmRxError):
            modem_amd.grid_centres(bad, 8000)
    with pytest.raises(modem_amd.OfdmRxError):
        modem_amd.grid_centres((25, 4), 8000, [7])
    with pytest.raises(modem_amd.OfdmRxError):
        modem_amd.grid_centres(6, 8000)                             # an int goes where it goes today


def test_plans():
    """every accepted M has a plan whose radices multiply to M, and `rows` is a permutation"""
    n = 0
    for P in range(2, 513):
        if R.reduce(P, 1) is None:
            continue
        n += 1
        M = 2 * P
        pl = R.plan(M)
        assert int(np.prod(pl)) == M and set(pl) <= {2, 3, 4, 5} and pl.count(2) <= 1 and len(pl) <= 8
        assert sorted(pl, key=lambda r: (5, 3, 4, 2).index(r)) == pl
        assert sorted(R.rows(M)) == list(range(M))
    assert n == 67 and R.plan(150) == [5, 5, 3, 2] and R.plan(1000) == [5, 5, 5, 4, 2] and R.plan(12) == [3, 4]


def test_transform_is_the_dft():
    for M in (6, 10, 12, 18, 30, 50, 90, 150, 600, 1000, 1024, 972):
        rng = np.random.default_rng(M)
        z = rng.standard_normal((3, M)) + 1j * rng.standard_normal((3, M))
        re, im = R.transform(z.real.copy(), z.imag.copy(), M)
        want = np.fft.fft(z, axis=1)
        assert np.abs((re + 1j * im)[:, R.rows(M)] - want).max() <= 1e-12 * np.abs(want).max(), M


@pytest.mark.parametrize("P,Q", RATIOS, ids=IDS)
def test_model_equals_the_direct_sum(P, Q):
    k = R.all_slots(P, Q)
    slots = [int(k[0]), -3 if k[0] <= -3 else -1, 0, 1, int(k[-1])]
    pcm = R.random_pcm(30 * P // Q + 7, np.int16, seed=P)
    v, tol = R.grid(pcm, P, Q, slots)
    outs = [0, 1, 7, v.shape[1] - 1]
    d = R.direct(pcm, P, Q, slots, outs)
    worst = float(np.max(np.abs(v[:, outs] - d) / _S(tol, P)[:, outs]))
    print("%d/%d: grid model against the direct sum, worst |difference| / S %.3g" % (P, Q, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize("P,Q", [(6, 1), (25, 4), (125, 4), (15, 2)], ids=["6/1", "25/4", "125/4", "15/2"])
def test_model_equals_the_ratio_model_at_the_slot_centres(P, Q):
    """all slots, 40 P samples from position 0: section 4.17's sum at the centres k rate / 2.  4.17 rounds the phase increment to an
    integer (by at most 1/2), which turns the phase at position m by at most 2 pi 2^-33 m: the bound adds that term, times S"""
    W = 40 * P
    pcm = R.random_pcm(W, np.int16, seed=P)
    v, tol = R.grid(pcm, P, Q)
    w, wtol, _ = RM.channelize(pcm, P, Q, R.centres(P, Q))
    assert v.shape == w.shape == (R.slot_range(P, Q)[1], R.n_outputs(W, P, Q))
    S = _S(tol, P)
    frac = float(np.max(np.abs(v - w) / wtol))
    print("%d/%d: grid model against the ratio model, worst |difference| / (4.17's tolerance) %.4f" % (P, Q, frac))
    assert (np.abs(v - w) <= 1e-12 * S + 2 * np.pi * 2.0 ** -33 * W * S).all()
    assert frac <= 0.05


@pytest.mark.parametrize("D", [2, 8, 64, 512])
def test_a_power_of_two_is_the_grid_model(D):
    """Q = 1 and P a power of two: section 4.19's function values and tolerance, exactly"""
    pcm = R.random_pcm(30 * D + 7, np.int16, seed=D)
    a, atol = R.grid(pcm, D, 1, [-D, 0, D - 1])
    b, btol = G.grid(pcm, D, [-D, 0, D - 1])
    assert np.array_equal(a, b) and np.array_equal(atol, btol)
    assert R.reduce(3 * D, 3) == (D, 1) and R.is_plain_grid(D, 1)
    assert (R.taps(D, 1)[0] == G.taps(D)).all() and R.slot_range(D, 1) == (-D, 2 * D)


def test_model_positions_and_rows():
    """the model itself: a block with its history gives the outputs of the whole capture; `wide_rows` is the same sum"""
    for P, Q in ((25, 4), (6, 1), (75, 2)):
        pcm = R.random_pcm(60 * P // Q + 5, np.int16, seed=3)
        v, tol = R.grid(pcm, P, Q)
        o0 = 30
        i0 = o0 * P // Q - (R.n_taps(P, Q) - 1)
        part, ptol = R.grid(pcm[i0:], P, Q, out_first=o0, in_first=i0)
        assert np.array_equal(part, v[:, o0:]) and np.array_equal(ptol, tol[:, o0:])
        r = R.wide_rows(pcm, P, Q, R.all_slots(P, Q))
        assert np.abs((r[..., 0] + 1j * r[..., 1]) - v).max() <= 2.0 ** -22 * np.abs(v).max()      # (rows are rounded to fp32)


@pytest.mark.parametrize("P,Q", RATIOS, ids=IDS)
def test_taps_and_slots_are_the_models(lib, P, Q):
    import modem_amd
    got = modem_amd.channelize_grid_taps((P, Q))
    assert got.dtype == np.float32 and got.shape == (Q, 24 * P // Q + 1)
    assert got.tobytes() == R.taps(P, Q).tobytes()
    assert modem_amd.channelize_grid_taps((3 * P, 3 * Q)).tobytes() == got.tobytes()
    if P <= 32 * Q:
        assert got.tobytes() == modem_amd.channelize_ratio_taps(P, Q).tobytes()
    k0, n = C.c_int32(0), C.c_size_t(0)
    assert lib.ofdmrx_util_grid_ratio_slots(P, Q, C.byref(k0), C.byref(n)) == 0
    assert (k0.value, n.value) == R.slot_range(P, Q)
    k = R.all_slots(P, Q)
    assert (-P <= k * Q).all() and (k * Q < P).all() and (k[0] - 1) * Q < -P and (k[-1] + 1) * Q >= P
    assert R.slot_range(25, 4)[1] == 13 and R.slot_range(6, 1) == (-6, 12)


def test_refusals_without_a_handle(lib):
    """every refusal that needs no look into the handle comes before any device call (and before the handle is touched)"""
    buf = np.full(16 * 12289 + 2, 7.0, np.float32)
    pb = buf.ctypes.data_as(C.c_void_p)
    k0, n = C.c_int32(99), C.c_size_t(99)
    bad_ratios = ((7, 1), (511, 16), (3, 2), (513, 1), (36, 17), (0, 1), (6, 0), (-6, 1), (6, -1), (1, 1), (1026, 2), (14, 3), (77, 5))
    for p, q in bad_ratios:
        assert R.reduce(p, q) is None
        assert lib.ofdmrx_util_channelize_grid_ratio_taps(p, q, pb) == E_ARG, (p, q)
        assert lib.ofdmrx_util_grid_ratio_slots(p, q, C.byref(k0), C.byref(n)) == E_ARG, (p, q)
    assert lib.ofdmrx_util_channelize_grid_ratio_taps(6, 1, None) == E_ARG
    assert lib.ofdmrx_util_grid_ratio_slots(6, 1, None, C.byref(n)) == E_ARG and lib.ofdmrx_util_grid_ratio_slots(6, 1, C.byref(k0), None) == E_ARG
    assert (buf == 7.0).all() and k0.value == 99 and n.value == 99
    assert lib.ofdmrx_util_channelize_grid_ratio_taps(512, 16, pb) == 769 and (buf[16 * 769:] == 7.0).all()
    assert lib.ofdmrx_util_channelize_grid_ratio_taps(1024, 4, pb) == 24 * 256 + 1                 # reduced first: 256 / 1
    for decim in (3, 12, 48):                                        # the grid entries keep their refusals
        assert lib.ofdmrx_util_channelize_grid_taps(decim, pb) == E_ARG

    fake = C.c_void_p(1)
    k = np.array([3, -6], np.int32)
    pk = k.ctypes.data_as(C.c_void_p)
    din, dout = C.c_void_p(1 << 20), C.c_void_p(1 << 24)

    def call(h=fake, d_in=din, fmt=0, in_first=0, n_in=4096, p=25, q=4, slots=pk, n=2, out_first=0, n_out=100, d_out=dout, stride=100):
        return lib.ofdmrx_util_channelize_grid_ratio(h, d_in, fmt, in_first, n_in, p, q, slots, n, out_first, n_out, d_out, stride)

    assert call(h=None) == E_ARG
    assert call(d_in=None) == E_ARG and call(d_out=None) == E_ARG
    assert call(n_in=0) == E_ARG and call(n_out=0) == E_ARG
    assert call(n=0) == E_ARG and call(n=65536) == E_ARG
    assert call(slots=None) == E_ARG and call(slots=None, n=12) == E_ARG and call(slots=None, n=14) == E_ARG   # NULL slots: n_all = 13
    for p, q in bad_ratios:
        assert call(p=p, q=q) == E_ARG, (p, q)
    for bad in (7, -7, 1 << 20, -(1 << 31)):                         # one past either end, and far out
        g = np.array([3, bad], np.int32)
        assert call(slots=g.ctypes.data_as(C.c_void_p)) == E_ARG, bad
    for bad in (6, -7):                                              # 6/1: slots -6 .. 5
        g = np.array([3, bad], np.int32)
        assert call(p=6, q=1, slots=g.ctypes.data_as(C.c_void_p)) == E_ARG, bad
    assert call(fmt=-1) == E_ARG and call(fmt=3) == E_ARG
    assert call(in_first=-1) == E_ARG and call(out_first=-1) == E_ARG
    assert call(stride=99) == E_ARG
    assert call(n_out=657) == E_ARG                                  # output 656 stands at position 4100 of 4096
    assert call(in_first=1, out_first=24) == E_ARG                   # history: 24 x 25 / 4 - 150 = 0 < in_first
    assert call(d_out=C.c_void_p((1 << 20) + 8)) == E_ARG            # the output overlaps the input
    assert call(d_in=C.c_void_p((1 << 20) + 2)) == E_ARG             # off the sample-frame boundary

    p_ = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    begin = lib.ofdmrx_bank_begin_wideband_grid_ratio
    assert begin(None, 2, p_(k), 25, 4, 0) == E_ARG
    assert begin(fake, 0, p_(k), 25, 4, 0) == E_ARG and begin(fake, 65536, p_(k), 25, 4, 0) == E_ARG
    assert begin(fake, 2, None, 25, 4, 0) == E_ARG and begin(fake, 12, None, 25, 4, 0) == E_ARG
    for p, q in bad_ratios:
        assert begin(fake, 2, p_(k), p, q, 0) == E_ARG, (p, q)
    assert begin(fake, 2, p_(k), 25, 4, -1) == E_ARG and begin(fake, 2, p_(k), 25, 4, 3) == E_ARG
    assert begin(fake, 2, p_(np.array([3, 7], np.int32)), 25, 4, 0) == E_ARG and begin(fake, 2, p_(np.array([-7, 3], np.int32)), 25, 4, 0) == E_ARG


@pytest.fixture(scope="module")
def cases():
    """full-scale random int16 input and the model on it, all slots: computed once, read only"""
    out = {}
    for P, Q in RATIOS:
        pcm = R.random_pcm(40 * P // Q + 7, np.int16, seed=P)
        v, tol = R.grid(pcm, P, Q)
        for a in (pcm, v, tol):
            a.setflags(write=False)
        out[(P, Q)] = (pcm, v, tol)
    return out


@pytest.mark.parametrize("P,Q", RATIOS, ids=IDS)
def test_fp32_evaluation_stays_inside_the_tolerance(cases, P, Q):
    pcm, v, tol = cases[(P, Q)]
    assert (tol > 0).all()
    w = R.worst(R.grid_fp32(pcm, P, Q), v, tol)
    print("%d/%d (plan %s, factor %g): fp32 evaluation, worst error / tol %.4f" % (P, Q, R.plan(2 * P), R.tol_factor(2 * P), w))
    assert w <= 1.0, (P, Q, w)


def test_tolerance_constants():
    """the rule's constants are the header's sums, rounded up"""
    t, r2 = 0.5 + 2 ** 0.5 + 1.0, 2 ** 0.5
    s3, c2, s1 = np.sin(np.pi / 3), abs(np.cos(4 * np.pi / 5)), np.sin(2 * np.pi / 5)
    c = {2: 1.0, 4: 2.0, 3: 0.5 + 1 + 3 * s3 + 1, 5: 3 * c2 + 2 + 4 * s1 + 1}
    for radix, b in R.B_TOL.items():
        assert (c[radix] + t) * r2 <= b <= (c[radix] + t) * r2 + 1.0, radix
    assert t * r2 <= R.C_TOL <= t * r2 + 1.0 and R.A_TOL == G.A_TOL and R.B_TOL[2] == G.B_TOL
    assert R.tol_factor(150) == 16 + 18 + 18 + 12 + 6 + 5


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("P,Q", [(6, 1), (15, 2)], ids=["6/1", "15/2"])
def test_wrong_variants_are_rejected(cases, P, Q, variant):
    """each wrong model leaves the tolerance somewhere: the rule tells them from the definition.  Four of them are the definition
    itself at Q = 1 (k Q = k, one tap phase, i_n an integer): there they must give the definition's values, and at 15/2 be rejected"""
    pcm, v, tol = cases[(P, Q)]
    w = R.worst(R.grid(pcm, P, Q, variant=variant)[0], v, tol)
    print("%d/%d %s: worst / tol %.3g" % (P, Q, variant, w))
    if Q == 1 and variant in R.VARIANTS_Q:
        assert w == 0.0, (P, Q, variant, w)
    else:
        assert w > 1.0, (P, Q, variant, w)


def test_enough_variants():
    assert len(R.VARIANTS) >= 12 and set(R.VARIANTS_Q) <= set(R.VARIANTS)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fixture_through_the_oracle(name):
    """the CPU twin of test_gpu_grid_ratio_bank.py: the oracle on the model's rows of every opened slot gives exactly the table the
    fixture states - every frame from its own slot at the frame's own sc_start, and the failed records of the neighbour slots"""
    cfg, want = GF.CONFIGS[name], GF.EXPECTED[name]
    pcm, pays = GF.capture(cfg)
    rows = R.wide_rows(pcm, cfg["P"], cfg["Q"], cfg["open"])
    for i, k in enumerate(cfg["open"]):
        recs = GF.oracle_records(rows[i])
        assert GF.table3(recs, pays) == want[k], k
        for (o, r), (status, frame, sc) in zip(recs, want[k]):
            if status == 0:
                assert r.sc_start == GF.sc_start(cfg, frame) and r.bit_flips == 0, (k, r.sc_start)
