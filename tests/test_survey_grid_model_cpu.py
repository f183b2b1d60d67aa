"""The grid survey without a GPU: the float64 model of survey_grid_model.py against section 4.19's models,
the tolerance rule on an fp32 evaluation in the documented order and on deliberately wrong models, what noise and a tone read, the
slot finder against its float64 restatement - on the captures of grid_fixture.py, on a sweep of sep_db, on edge cases and on every
refusal - and the oracle on the model's rows at the slots the finder gives."""
import ctypes as C

import numpy as np
import pytest

import channelize_grid_model as G
import grid_fixture as GF
import survey_grid_model as SG

E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    import modem_amd
    modem_amd.build()
    return modem_amd.load_library()


@pytest.mark.parametrize("D", [2, 8, 64])
def test_model_is_the_mean_power_of_the_grid_models_outputs(D):
    """P equals the mean of |grid|^2 and of |rows|^2 (rows are rounded to fp32: compared at that precision) and the bound is
    channelize_grid_model.bound; a block with only the positions its rows need gives the same values"""
    S, n_rows = 16, 3
    pcm = SG.tone_pcm(S * (n_rows + 1) * D, D, 1, seed=D)
    P, tol = SG.power(pcm, D, S, 0, n_rows)
    v, _ = G.grid(pcm, D, None, n_out=S * n_rows)
    want = (np.abs(v) ** 2).reshape(2 * D, n_rows, S).mean(axis=2).T
    rel = float(np.max(np.abs(P - want) / want))
    print("D %d: model against mean |grid|^2, worst relative difference %.3g" % (D, rel))
    assert rel <= 1e-12
    r = G.rows(pcm, D, G.all_slots(D))[:, :S * n_rows].astype(np.float64)
    want_r = (r[..., 0] ** 2 + r[..., 1] ** 2).reshape(2 * D, n_rows, S).mean(axis=2).T
    assert np.max(np.abs(P - want_r) / want_r) <= 2.0 ** -21
    _, e = SG.outputs(pcm, D, 0, S * n_rows)
    b = np.sqrt(2.0) * G.bound(pcm, D, 0, S * n_rows)
    assert np.max(np.abs(e - b)) <= 1e-12 * b.max()
    first, count = SG.span(D, S, 1, 2)
    assert (first, count) == (max(0, (S - 24) * D), (3 * S - 1) * D - max(0, (S - 24) * D) + 1)
    part, ptol = SG.power(pcm[first:first + count], D, S, 1, 2, in_first=first)
    assert np.max(np.abs(part - P[1:]) / P[1:]) <= 1e-12 and np.max(np.abs(ptol - tol[1:]) / tol[1:]) <= 1e-9


@pytest.fixture(scope="module")
def cases():
    """per D: (int16 input with a tone, the model on it), (uint8 likewise): computed once, read only"""
    out = {}
    for D, slot in ((2, 1), (64, 5)):
        S, n_rows = 16, 3
        for dt in (np.int16, np.uint8):
            pcm = SG.tone_pcm(S * n_rows * D + 1, D, slot, dt, seed=D)
            P, tol = SG.power(pcm, D, S, 0, n_rows)
            for a in (pcm, P, tol):
                a.setflags(write=False)
            out[D, np.dtype(dt)] = (pcm, S, n_rows, P, tol)
    return out


@pytest.mark.parametrize("D", G.ALL_D)
def test_fp32_evaluation_stays_inside_the_tolerance(D):
    S, n_rows = 32, 2
    pcm = SG.tone_pcm(S * n_rows * D, D, 1, seed=D)
    P, tol = SG.power(pcm, D, S, 0, n_rows)
    assert (tol > 0).all()
    w = SG.worst(SG.power_fp32(pcm, D, S, n_rows), P, tol)
    print("D %d: fp32 evaluation in the documented order, worst error / tol %.4f" % (D, w))
    assert w <= 1.0, (D, w)


def test_fp32_evaluation_long_row():
    """S = 4096 at D = 2: the S / 8 term of the rule is what a long chain needs"""
    D, S = 2, 4096
    pcm = SG.tone_pcm(S * D, D, 1, seed=9)
    P, tol = SG.power(pcm, D, S, 0, 1)
    w = SG.worst(SG.power_fp32(pcm, D, S, 1), P, tol)
    print("D 2, S 4096: fp32 evaluation, worst error / tol %.4f" % w)
    assert w <= 1.0


@pytest.mark.parametrize("D,variant", [(D, v) for v in SG.VARIANTS for D in (2, 64)])
def test_wrong_variants_are_rejected(cases, D, variant):
    """each wrong model leaves the tolerance somewhere: the rule tells them from the definition.  (A missing (-1)^{k n} is not in
    the list: no power can show it.)"""
    pcm, S, n_rows, P, tol = cases[D, np.dtype(np.uint8 if variant.startswith("U8") else np.int16)]
    w = SG.worst(SG.power(pcm, D, S, 0, n_rows, variant=variant)[0], P, tol)
    print("D %d %s: worst / tol %.3g" % (D, variant, w))
    assert w > 1.0, (D, variant, w)


def test_noise_reads_sigma2_sum_h2():
    """white noise of power sigma^2 per complex sample reads sigma^2 sum h^2 ~ 0.7071 sigma^2 / D in every slot"""
    D, S, sigma = 8, 4096, 0.1
    rng = np.random.default_rng(5)
    first, count = SG.span(D, S, 1, 1)
    x = (sigma * np.sqrt(0.5) * rng.standard_normal((first + count, 2))).astype(np.float32)
    P, _ = SG.power(x, D, S, 1, 1)
    want = SG.noise_reading(D, sigma ** 2)
    print("noise: predicted %.4g, read %.4g (mean of %d slots), 0.7071 sigma^2 / D = %.4g" % (want, P.mean(), 2 * D, 0.7071 * sigma ** 2 / D))
    assert abs(want / (0.7071 * sigma ** 2 / D) - 1.0) < 2e-3
    assert abs(P.mean() / want - 1.0) < 0.03 and np.max(np.abs(P / want - 1.0)) < 0.12


@pytest.mark.parametrize("D,k", [(2, 1), (8, -3), (64, 63), (64, -64)])
def test_tone_reads_its_power_in_its_slot(D, k):
    """a tone of amplitude A on slot centre k reads A^2 in slot k (the passband is flat within 0.01 dB) and below -70 dB of that two
    slots away, once the filter is full"""
    S, A = 64, 0.5
    M = 2 * D
    first, count = SG.span(D, S, 1, 1)
    m = np.arange(first + count, dtype=np.int64)
    ph = 2.0 * np.pi * ((k * m) % M) / M
    x = (A * np.stack([np.cos(ph), np.sin(ph)], axis=1)).astype(np.float32)
    P, _ = SG.power(x, D, S, 1, 1)
    i = k + D
    assert abs(10 * np.log10(P[0, i] / A ** 2)) < 0.01
    far = [j for j in range(M) if min((j - i) % M, (i - j) % M) >= 2]
    if far:
        assert 10 * np.log10(P[0, far].max() / A ** 2) < -70.0


# ---- the finder

def _lib_find(lib, row, D, rate, thr_db=6.0, sep_db=8.0, abs_floor=0.0, max_slots=None):
    import modem_amd.ofdmrx as M
    row = np.ascontiguousarray(row, np.float32)
    cap = 2 * D if max_slots is None else max_slots
    slots = (M.Slot * max(cap, 1))()
    n, floor = C.c_size_t(0), C.c_double(-1.0)
    r = lib.ofdmrx_util_find_slots(row.ctypes.data_as(C.c_void_p), D, rate, thr_db, sep_db, abs_floor, cap, slots, C.byref(n), C.byref(floor))
    assert r == 0
    return [(s.slot, s.centre_hz, s.power, s.level_db) for s in slots[:min(n.value, cap)]], n.value, floor.value


def _same(lib, row, D, rate=8000.0, **kw):
    got, n, floor = _lib_find(lib, row, D, rate, **kw)
    want, wfloor = SG.find_slots(row, D, rate, **kw)
    assert n == len(want) and floor == wfloor
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[0] == w[0] and g[1] == w[1] and g[2] == w[2]
        assert g[3] == w[3] or abs(g[3] - w[3]) <= 1e-5 * abs(w[3])
    return [g[0] for g in got]


@pytest.fixture(scope="module")
def fixture_rows():
    """the model's survey of captures A and B at S = 4096: (mean row, peak-hold row) over the whole rows of each, as float32"""
    out = {}
    for name, cfg, cap in (("a", GF.A, GF.capture_a), ("b", GF.B, GF.capture_b)):
        pcm, pays = cap()
        D, S = cfg["D"], 4096
        n_rows = (len(pcm) - 1) // D // S                            # the whole rows the capture holds
        P, _ = SG.power(pcm, D, S, 0, n_rows)
        out[name] = (pcm, pays, P.mean(axis=0).astype(np.float32), P.max(axis=0).astype(np.float32))
    return out


def test_finder_on_the_fixtures(lib, fixture_rows):
    """capture A (D = 8, four frames: 12 of 16 slots carry a frame or its edge, so the median is no noise floor) gives -7, -2, 3, 6
    with abs_floor = 2 x the predicted noise reading, and only 3 and 6 on the median; capture B gives 37, 39 on the median - on the
    mean row and on the peak-hold row, for every sep_db 3 .. 10"""
    import modem_amd
    noise_a = SG.noise_reading(8, 2 * GF.SIGMA ** 2)
    noise_b = SG.noise_reading(64, 2 * GF.SIGMA ** 2)
    print("predicted noise readings: A %.4g, B %.4g" % (noise_a, noise_b))
    for which in (2, 3):
        ra, rb = fixture_rows["a"][which], fixture_rows["b"][which]
        if which == 2:
            print("read (median of the mean row): A quiet slots %.4g, B %.4g" % (np.sort(ra)[:4].mean(), np.median(rb)))
            assert abs(np.sort(ra)[:4].mean() / noise_a - 1) < 0.05 and abs(np.median(rb) / noise_b - 1) < 0.05
        assert _same(lib, ra, 8) == [3, 6]
        for sep in range(3, 11):
            assert _same(lib, ra, 8, sep_db=float(sep), abs_floor=2 * noise_a) == list(GF.A["slots"]), sep
            assert _same(lib, rb, 64, sep_db=float(sep)) == list(GF.B["slots"]), sep
        got = modem_amd.find_slots(ra, 8, 8000, abs_floor=2 * noise_a)
        assert [s["slot"] for s in got] == list(GF.A["slots"]) and [s["centre_hz"] for s in got] == [-28000.0, -8000.0, 12000.0, 24000.0]
        # a centred mode-6 frame reads about 11 dB lower in the slots beside its own: what the default sep_db = 8 rests on
        for k in GF.A["slots"]:
            # (the louder neighbour; the sweep above needs more than 10 dB, and at 12 edges of the strong frames come back)
            edge = 10 * np.log10(ra[k + 8] / max(ra[(k + 9) % 16], ra[(k + 7) % 16]))
            print("capture A, %s row, slot %d: %.1f dB over its louder neighbour" % ("mean" if which == 2 else "peak-hold", k, edge))
            assert edge > 10.0, (k, edge)
    strong = SG.find_slots(fixture_rows["a"][2], 8, 8000.0, sep_db=12.0, abs_floor=2 * noise_a)[0]
    assert len(strong) > 4 and set(GF.A["slots"]) < set(s[0] for s in strong)


def test_finder_edge_cases(lib):
    import modem_amd
    M = 16
    assert _same(lib, np.full(M, 3.0), 8) == []                                      # all equal: nothing above the floor
    assert _same(lib, np.zeros(M), 8) == []
    row = np.ones(M)
    row[5] = 100.0
    assert _same(lib, row, 8) == [-3]                                                # one slot
    assert _same(lib, [1.0, 1.0, 50.0, 1.0], 2) == [0] and _same(lib, [50.0, 1.0, 1.0, 1.0], 2) == [-2]   # M = 4
    row = np.ones(M)
    row[M - 1], row[0] = 100.0, 10.0                                                 # the wrap: slot -M/2 is the edge of slot M/2 - 1
    assert _same(lib, row, 8) == [7]
    row[M - 1], row[0] = 10.0, 100.0
    assert _same(lib, row, 8) == [-8]
    row = np.ones(M)
    row[4] = row[5] = 100.0                                                          # a strict tie: neither shadows the other
    assert _same(lib, row, 8) == [-4, -3]
    row[5] = np.float32(100.0 * 10 ** 0.8) * (1 + 2.0 ** -20)                          # just past sep_db: the weaker one goes
    assert _same(lib, row, 8) == [-3]
    row = np.ones(M)
    row[[2, 6, 10]] = 100.0
    got, n, _ = _lib_find(lib, row, 8, 8000.0, max_slots=2)                          # max_slots below the count
    assert n == 3 and [g[0] for g in got] == [-6, -2]
    assert _same(lib, row, 8, thr_db=20.0) == [] and _same(lib, row, 8, thr_db=19.9) == [-6, -2, 2]
    assert _same(lib, row, 8, abs_floor=200.0, thr_db=0.0) == [] and _same(lib, row, 8, abs_floor=50.0, thr_db=0.0) == [-6, -2, 2]
    slots, floor = modem_amd.find_slots(row, 8, 8000, with_floor=True)
    assert floor == 1.0 and [s["slot"] for s in slots] == [-6, -2, 2] and abs(slots[0]["level_db"] - 20.0) < 1e-5


def test_finder_refusals(lib):
    import modem_amd
    import modem_amd.ofdmrx as M
    row = np.ones(16, np.float32)
    p = row.ctypes.data_as(C.c_void_p)
    slots = (M.Slot * 16)()
    n = C.c_size_t(99)

    def call(row=p, decim=8, rate=8000.0, thr=6.0, sep=8.0, floor=0.0, out=slots, cnt=C.byref(n)):
        return lib.ofdmrx_util_find_slots(row, decim, rate, thr, sep, floor, 16, out, cnt, None)

    assert call() == 0 and n.value == 0
    n.value = 99
    assert call(row=None) == E_ARG and call(out=None) == E_ARG and call(cnt=None) == E_ARG
    for bad in (-8, 0, 1, 3, 12, 1024):
        assert call(decim=bad) == E_ARG, bad
    for bad in (0.0, -8000.0, float("nan"), float("inf")):
        assert call(rate=bad) == E_ARG, bad
    for bad in (-0.1, float("nan"), float("inf")):
        assert call(thr=bad) == E_ARG and call(sep=bad) == E_ARG and call(floor=bad) == E_ARG, bad
    assert n.value == 99
    with pytest.raises(modem_amd.OfdmRxError):
        modem_amd.find_slots(row, 4, 8000)                              # 16 values are no row of decim 4
    with pytest.raises(modem_amd.OfdmRxError):
        modem_amd.find_slots(row, 8, 8000, sep_db=-1.0)


def test_found_slots_through_the_oracle(lib, fixture_rows):
    """the loop's CPU twin: the oracle on the model's rows at the FOUND slots of capture A: one status-0 record with the golden
    payload each"""
    import modem_amd
    pcm, pays, mean_row, _ = fixture_rows["a"]
    found = [s["slot"] for s in modem_amd.find_slots(mean_row, 8, GF.RATE, abs_floor=2 * SG.noise_reading(8, 2 * GF.SIGMA ** 2))]
    assert found == list(GF.A["slots"])
    rows = G.rows(pcm, 8, found)
    for i, k in enumerate(found):
        recs = GF.oracle_records(rows[i])
        assert GF.table(recs, pays) == [(0, i)], k
