"""The grid survey at a ratio without a GPU: the float64 model of survey_grid_ratio_model.py against section
4.22's and 4.21's models, the tolerance rule on an fp32 evaluation in the documented order and on deliberately wrong models, what a
tone and noise read, and the slot finder at a ratio against its float64 restatement - on random rows, on the end rule, against
ofdmrx_util_find_slots at a power of two, on every refusal and on the captures of grid_ratio_fixture.py.

What test_finder_on_the_fixtures shows for capture B (25/4, frames placed at slots -6 and 3), from the model alone: the peak-hold
row reads, in dB re full scale, slot -6 -21.79, slot 3 -27.86 and slot 6 -22.18, the other slots below -34.  Slot 6 is k_last and slot
-6 is k_first: at 25/4 the 13 slots cover 52 of the circle's 50 bins, so the two lie half a slot apart across the band edge (+24 kHz
and -24 kHz = +26 kHz at 50 kHz) and the frame placed in slot -6 reads 0.4 dB lower in slot 6.  Neither end shadows the other; the
finder's rule for ends that lie half a slot apart or less (0 < 4 (P mod Q) <= Q) takes two ends within sep_db of each other for one
signal and reports the louder, so it returns the placed (-6, 3).  Capture A (6/1, cyclic) gives its placed slots (-6, 5).  Both at
the default floor, the median."""
import ctypes as C

import numpy as np
import pytest

import channelize_grid_ratio_model as GR
import grid_ratio_fixture as GF
import survey_grid_model as SG
import survey_grid_ratio_model as SR

E_ARG = -1
# the parameters of the finder on the fixtures, fixed here from the model alone (test_gpu_grid_ratio_survey_loop.py uses them): the
# defaults thr_db = 6, sep_db = 8 and the median floor
FIXTURE_FLOOR = {"a": 0.0, "b": 0.0}


@pytest.fixture(scope="module")
def lib():
    import modem_amd
    modem_amd.build()
    return modem_amd.load_library()


@pytest.mark.parametrize("P,Q", [(6, 1), (15, 2), (25, 4), (45, 16)])
def test_model_is_the_mean_power_of_the_ratio_grid_models_outputs(P, Q):
    """P equals the mean of |channelize_grid_ratio_model.grid|^2 within 1e-12 relative, e is sqrt 2 x its bound, and a block with
    only the positions its rows need gives the same values"""
    S, n_rows = 16, 3
    n_all = GR.slot_range(P, Q)[1]
    pcm = SR.tone_pcm(SR.span(P, Q, S, 0, n_rows + 1)[1], P, Q, 1, seed=P)
    Pw, tol = SR.power(pcm, P, Q, S, 0, n_rows)
    assert Pw.shape == (n_rows, n_all)
    v, _ = GR.grid(pcm, P, Q, None, n_out=S * n_rows)
    want = (np.abs(v) ** 2).reshape(n_all, n_rows, S).mean(axis=2).T
    rel = float(np.max(np.abs(Pw - want) / want))
    print("%d/%d: model against mean |grid|^2, worst relative difference %.3g" % (P, Q, rel))
    assert rel <= 1e-12
    _, e = SR.outputs(pcm, P, Q, 0, S * n_rows)
    b = np.sqrt(2.0) * GR.bound(pcm, P, Q, 0, S * n_rows)
    assert np.max(np.abs(e - b)) <= 1e-12 * b.max()
    first, count = SR.span(P, Q, S, 1, 2)
    assert (first, count) == (max(0, (S * P) // Q - 24 * P // Q), ((3 * S - 1) * P) // Q - max(0, (S * P) // Q - 24 * P // Q) + 1)
    part, ptol = SR.power(pcm[first:first + count], P, Q, S, 1, 2, in_first=first)
    assert np.max(np.abs(part - Pw[1:]) / Pw[1:]) <= 1e-12 and np.max(np.abs(ptol - tol[1:]) / tol[1:]) <= 1e-9


@pytest.mark.parametrize("D", [8, 64])
def test_power_of_two_is_the_grid_survey_model(D):
    S, n_rows = 16, 3
    pcm = SG.tone_pcm(S * n_rows * D + 1, D, 1, seed=D)
    a, atol = SR.power(pcm, D, 1, S, 0, n_rows)
    b, btol = SG.power(pcm, D, S, 0, n_rows)
    assert a.shape == b.shape == (n_rows, 2 * D)
    assert np.max(np.abs(a - b) / b) <= 1e-12 and np.max(np.abs(atol - btol) / btol) <= 1e-9
    assert SR.span(D, 1, S, 2, 3) == SG.span(D, S, 2, 3)


@pytest.mark.parametrize("P,Q", [(3, 1), (6, 1), (15, 2), (25, 4), (45, 16), (125, 4)])
def test_fp32_evaluation_stays_inside_the_tolerance(P, Q):
    S, n_rows = 32, 2
    pcm = SR.tone_pcm(SR.span(P, Q, S, 0, n_rows)[1], P, Q, 1, seed=P)
    Pw, tol = SR.power(pcm, P, Q, S, 0, n_rows)
    assert (tol > 0).all()
    w = SR.worst(SR.power_fp32(pcm, P, Q, S, n_rows), Pw, tol)
    print("%d/%d: fp32 evaluation in the documented order, worst error / tol %.4f" % (P, Q, w))
    assert w <= 1.0, (P, Q, w)


def test_fp32_evaluation_long_row():
    P, Q, S = 6, 1, 4096
    pcm = SR.tone_pcm(SR.span(P, Q, S, 0, 1)[1], P, Q, 1, seed=9)
    Pw, tol = SR.power(pcm, P, Q, S, 0, 1)
    w = SR.worst(SR.power_fp32(pcm, P, Q, S, 1), Pw, tol)
    print("6/1, S 4096: fp32 evaluation, worst error / tol %.4f" % w)
    assert w <= 1.0


@pytest.fixture(scope="module")
def cases():
    """per ratio: int16 input with a tone and the model on it: computed once, read only"""
    out = {}
    for P, Q, slot in ((6, 1, 1), (15, 2, 3)):
        S, n_rows = 16, 3
        pcm = SR.tone_pcm(SR.span(P, Q, S, 0, n_rows)[1] + 1, P, Q, slot, seed=P)
        Pw, tol = SR.power(pcm, P, Q, S, 0, n_rows)
        for a in (pcm, Pw, tol):
            a.setflags(write=False)
        out[P, Q] = (pcm, S, n_rows, Pw, tol)
    return out


def test_there_are_eleven_variants():
    assert len(SR.VARIANTS) >= 11 and len(set(SR.VARIANTS)) == len(SR.VARIANTS) and set(SR.VARIANTS_Q) < set(SR.VARIANTS)


@pytest.mark.parametrize("P,Q,variant", [(P, Q, v) for v in SR.VARIANTS for P, Q in ((6, 1), (15, 2))])
def test_wrong_variants_are_rejected(cases, P, Q, variant):
    """each wrong model leaves the tolerance somewhere (a row of another width is infinitely far); those that are the definition
    itself at Q = 1 are held to be exactly that there"""
    pcm, S, n_rows, Pw, tol = cases[P, Q]
    got = SR.power(pcm, P, Q, S, 0, n_rows, variant=variant)[0]
    w = SR.worst(got, Pw, tol)
    print("%d/%d %s: worst / tol %.3g" % (P, Q, variant, w))
    if Q == 1 and variant in SR.VARIANTS_Q:
        assert got.shape == Pw.shape and np.max(np.abs(got - Pw) / Pw) <= 1e-12, (variant, w)
    else:
        assert w > 1.0, (P, Q, variant, w)


@pytest.mark.parametrize("P,Q,k", [(6, 1, 5), (15, 2, -7), (25, 4, 6), (25, 4, -6), (45, 16, 2)])
def test_tone_reads_its_power_in_its_slot(P, Q, k):
    """a tone of amplitude A on slot centre k reads A^2 in slot k (within 0.01 dB) and below -70 dB of that two slots or more away
    on the circle, once the filter is full"""
    S, A = 64, 0.5
    M = 2 * P
    k0, n_all = GR.slot_range(P, Q)
    first, count = SR.span(P, Q, S, 1, 1)
    m = np.arange(first + count, dtype=np.int64)
    ph = 2.0 * np.pi * ((k * Q * (m % M)) % M) / M
    x = (A * np.stack([np.cos(ph), np.sin(ph)], axis=1)).astype(np.float32)
    Pw, _ = SR.power(x, P, Q, S, 1, 1)
    i = k - k0
    assert abs(10 * np.log10(Pw[0, i] / A ** 2)) < 0.01
    far = [j for j in range(n_all) if min(((j - i) * Q) % M, ((i - j) * Q) % M) >= 2 * Q]
    assert far and 10 * np.log10(Pw[0, far].max() / A ** 2) < -70.0


def test_noise_reads_sigma2_mean_sum_h2():
    P, Q, S, sigma = 25, 4, 4096, 0.1
    rng = np.random.default_rng(5)
    first, count = SR.span(P, Q, S, 1, 1)
    x = (sigma * np.sqrt(0.5) * rng.standard_normal((first + count, 2))).astype(np.float32)
    Pw, _ = SR.power(x, P, Q, S, 1, 1)
    want = SR.noise_reading(P, Q, sigma ** 2)
    print("noise at 25/4: predicted %.4g, read %.4g (mean of %d slots)" % (want, Pw.mean(), Pw.shape[1]))
    assert abs(Pw.mean() / want - 1.0) < 0.03 and np.max(np.abs(Pw / want - 1.0)) < 0.12


# ---- the finder

def _lib_find(lib, row, P, Q, rate, thr_db=6.0, sep_db=8.0, abs_floor=0.0, max_slots=None):
    import modem_amd.ofdmrx as M
    row = np.ascontiguousarray(row, np.float32)
    cap = len(row) if max_slots is None else max_slots
    slots = (M.Slot * max(cap, 1))()
    n, floor = C.c_size_t(0), C.c_double(-1.0)
    r = lib.ofdmrx_util_find_slots_ratio(row.ctypes.data_as(C.c_void_p), P, Q, rate, thr_db, sep_db, abs_floor, cap, slots, C.byref(n), C.byref(floor))
    assert r == 0
    return [(s.slot, s.centre_hz, s.power, s.level_db) for s in slots[:min(n.value, cap)]], n.value, floor.value


def _same(lib, row, P, Q, rate=8000.0, **kw):
    got, n, floor = _lib_find(lib, row, P, Q, rate, **kw)
    want, wfloor = SR.find_slots(row, P, Q, rate, **kw)
    assert n == len(want) and floor == wfloor
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[0] == w[0] and g[1] == w[1] and g[2] == w[2]
        assert g[3] == w[3] or abs(g[3] - w[3]) <= 1e-5 * abs(w[3])
    return [g[0] for g in got]


@pytest.mark.parametrize("P,Q", [(6, 1), (15, 2), (25, 4)])
def test_finder_on_random_rows(lib, P, Q):
    """6/1: cyclic; 15/2: cyclic with Q = 2; 25/4: open ends and an odd count (the median is the middle value)"""
    n_all = GR.slot_range(P, Q)[1]
    assert (n_all * Q == 2 * P) == (Q <= 2)
    rng = np.random.default_rng(P)
    found = 0
    for trial in range(200):
        row = 10.0 ** rng.uniform(-3, 0, n_all)
        row[rng.integers(0, n_all, 3)] *= 10.0 ** rng.uniform(0, 3, 3)
        if trial % 4 == 0:
            row[[0, -1]] *= 100.0                                      # both ends loud
        kw = dict(thr_db=float(rng.uniform(0, 12)), sep_db=float(rng.uniform(0, 12)), abs_floor=float(rng.choice([0.0, 0.05])))
        found += len(_same(lib, row, P, Q, **kw))
    assert found > 100
    if n_all % 2:
        row = np.arange(1, n_all + 1, dtype=np.float32)
        assert _lib_find(lib, row, P, Q, 8000.0)[2] == float(n_all // 2 + 1)


def test_the_end_rule(lib):
    """a strong slot at k_last shadows k_first where the slots tile the circle (6/1) and does not where they do not (25/4)"""
    for (P, Q), want in (((6, 1), [5]), ((15, 2), [7]), ((25, 4), [-6, 6]), ((45, 16), [-2, 2])):
        k0, n_all = GR.slot_range(P, Q)
        row = np.ones(n_all)
        row[-1], row[0] = 1000.0, 10.0
        assert _same(lib, row, P, Q) == want, (P, Q)
        row[-1], row[0] = 10.0, 1000.0
        assert _same(lib, row, P, Q) == ([k0] if len(want) == 1 else want), (P, Q)


def test_ends_half_a_slot_apart_are_one_signal(lib):
    """25/4 and 9/4: the centres of k_last and k_first lie half a slot apart across the band edge (0 < 4 (P mod Q) <= Q): both ends
    within sep_db of each other are one signal, the louder is reported, a tie goes to k_first; further apart than sep_db both stay
    (the end rule: neither shadows the other).  10/3 (two thirds of a slot apart), 45/16 (a gap) and 15/2 (cyclic) keep both"""
    for P, Q in ((25, 4), (9, 4)):
        k0, n_all = GR.slot_range(P, Q)
        assert 0 < 4 * (P % Q) <= Q
        row = np.ones(n_all)
        row[0], row[-1] = 100.0, 90.0
        assert _same(lib, row, P, Q) == [k0]
        row[0], row[-1] = 90.0, 100.0
        assert _same(lib, row, P, Q) == [k0 + n_all - 1]
        row[0], row[-1] = 100.0, 100.0
        assert _same(lib, row, P, Q) == [k0]
        row[0], row[-1] = 100.0, np.float32(100.0 / 10 ** 0.8)            # exactly sep_db apart in double: still one
        assert len(_same(lib, row, P, Q)) == 1
        row[0], row[-1] = 100.0, 15.0                                      # 8.2 dB: two
        assert _same(lib, row, P, Q) == [k0, k0 + n_all - 1]
        assert _same(lib, row, P, Q, sep_db=9.0) == [k0]
        row[0], row[-1] = 100.0, 90.0
        row[1] = 1000.0                                                    # k_first is its neighbour's edge: k_last stands alone
        assert _same(lib, row, P, Q, abs_floor=1.0) == [k0 + 1, k0 + n_all - 1]      # (five slots: the median is no floor here)
    for P, Q in ((10, 3), (45, 16), (15, 2)):
        k0, n_all = GR.slot_range(P, Q)
        row = np.ones(n_all)
        row[0], row[-1] = 100.0, 90.0
        assert _same(lib, row, P, Q) == [k0, k0 + n_all - 1], (P, Q)


@pytest.mark.parametrize("D", [8, 64])
def test_power_of_two_is_find_slots(lib, D):
    import modem_amd
    import modem_amd.ofdmrx as M
    rng = np.random.default_rng(D)
    for trial in range(50):
        row = (10.0 ** rng.uniform(-3, 0, 2 * D)).astype(np.float32)
        row[rng.integers(0, 2 * D, 3)] *= 100.0
        row[[0, -1]] *= np.float32(rng.choice([1.0, 300.0]))
        a = (M.Slot * (2 * D))()
        na, fa = C.c_size_t(0), C.c_double(0)
        assert lib.ofdmrx_util_find_slots(row.ctypes.data_as(C.c_void_p), D, 8000.0, 6.0, 8.0, 0.0, 2 * D, a, C.byref(na), C.byref(fa)) == 0
        for p, q in ((D, 1), (3 * D, 3)):
            got, n, floor = _lib_find(lib, row, p, q, 8000.0)
            assert n == na.value and floor == fa.value
            assert got == [(s.slot, s.centre_hz, s.power, s.level_db) for s in a[:n]]
        assert modem_amd.find_slots(row, (D, 1), 8000) == modem_amd.find_slots(row, D, 8000)


def test_finder_refusals(lib):
    import modem_amd
    import modem_amd.ofdmrx as M
    row = np.ones(13, np.float32)
    p = row.ctypes.data_as(C.c_void_p)
    slots = (M.Slot * 16)()
    n = C.c_size_t(99)

    def call(row=p, P=25, Q=4, rate=8000.0, thr=6.0, sep=8.0, floor=0.0, out=slots, cnt=C.byref(n)):
        return lib.ofdmrx_util_find_slots_ratio(row, P, Q, rate, thr, sep, floor, 16, out, cnt, None)

    assert call() == 0 and n.value == 0
    n.value = 99
    assert call(row=None) == E_ARG and call(out=None) == E_ARG and call(cnt=None) == E_ARG
    for bad in ((0, 1), (25, 0), (-25, 4), (25, -4), (7, 1), (3, 2), (25, 13), (17, 16), (513, 1), (1024, 1), (77, 4), (1, 1)):
        assert call(P=bad[0], Q=bad[1]) == E_ARG, bad
    for bad in (0.0, -8000.0, float("nan"), float("inf")):
        assert call(rate=bad) == E_ARG, bad
    for bad in (-0.1, float("nan"), float("inf")):
        assert call(thr=bad) == E_ARG and call(sep=bad) == E_ARG and call(floor=bad) == E_ARG, bad
    assert n.value == 99
    with pytest.raises(modem_amd.OfdmRxError):
        modem_amd.find_slots(np.ones(12, np.float32), (25, 4), 8000)      # 12 values are no row of 25/4
    with pytest.raises(modem_amd.OfdmRxError):
        modem_amd.find_slots(row, (7, 1), 8000)
    with pytest.raises(modem_amd.OfdmRxError):
        modem_amd.find_slots(row, (25, 4), 8000, sep_db=-1.0)
    got = modem_amd.find_slots(np.where(np.arange(13) == 9, 100.0, 1.0), (50, 8), 8000)
    assert [(s["slot"], s["centre_hz"]) for s in got] == [(3, 12000.0)]


@pytest.fixture(scope="module")
def fixture_rows():
    """the model's survey of captures A and B at S = 4096: the peak-hold row over the whole rows of each, as float32"""
    out = {}
    for name in ("a", "b"):
        cfg = GF.CONFIGS[name]
        pcm, pays = GF.capture(cfg)
        P, Q, S = cfg["P"], cfg["Q"], 4096
        n_rows = ((len(pcm) * Q - 1) // P + 1) // S
        Pw, _ = SR.power(pcm, P, Q, S, 0, n_rows)
        out[name] = Pw.max(axis=0).astype(np.float32)
    return out


@pytest.mark.parametrize("name", ["a", "b"])
def test_finder_on_the_fixtures(lib, fixture_rows, name):
    """the model's peak-hold row of the capture through the finder with the parameters fixed above gives exactly the placed slots.
    In capture B slot 6 = k_last reads the frame of slot -6 = k_first at -22.18 dB against -21.79 dB: the ends seen twice, one signal"""
    import modem_amd
    cfg, row = GF.CONFIGS[name], fixture_rows[name]
    P, Q = cfg["P"], cfg["Q"]
    k0 = GR.slot_range(P, Q)[0]
    print("capture %s, peak-hold row in dB re full scale: %s" % (name, " ".join("%d:%.2f" % (k0 + i, 10 * np.log10(v)) for i, v in enumerate(row))))
    noise = SR.noise_reading(P, Q, 2 * GF.SIGMA ** 2)
    print("predicted noise reading %.4g, the row's median %.4g" % (noise, np.median(row)))
    found = _same(lib, row, P, Q, abs_floor=FIXTURE_FLOOR[name])
    print("capture %s: the finder gives %s, placed %s" % (name, found, sorted(cfg["slots"])))
    assert [s["slot"] for s in modem_amd.find_slots(row, (P, Q), GF.RATE, abs_floor=FIXTURE_FLOOR[name])] == found
    assert found == sorted(cfg["slots"])
