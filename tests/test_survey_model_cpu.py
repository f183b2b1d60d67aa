"""The wideband survey without a GPU: the float64 model of survey_model.py - its tolerance rule on an fp32
evaluation and on deliberately wrong models, its statistics on noise and a tone - the library's window and band finder against it,
the finder's edge cases, the argument errors that need no look into the handle, and the model on the capture of
wideband_fixture.py: the bands it finds, the waterfall, and the oracle on the front-end model's rows at the FOUND centres."""
import ctypes as C
import os

import numpy as np
import pytest

import channelize_model as CM
import oracle_lib as O
import survey_model as SM
import wideband_fixture as WF

E_ARG, E_NODEV = -1, -4
NAMES = ("ofdmrx_util_survey_window", "ofdmrx_util_survey", "ofdmrx_util_find_bands")
RW = float(WF.DECIM * WF.RATE)


@pytest.fixture(scope="module")
def lib():
    import modem_amd
    modem_amd.build()
    return modem_amd.load_library()


# ---- the ABI, in the style of test_synthesize_abi_cpu.py

def test_symbols_exported_and_minor_unchanged(lib):
    import modem_amd
    import modem_amd.ofdmrx as M
    text = open(os.path.join(os.path.dirname(M.HERE), "include", "ofdmrx.h")).read()
    for name in NAMES:
        assert name in M.EXPORTS
        getattr(lib, name)
        assert name + "(" in text and name in text.split("#define OFDMRX_ABI_MINOR")[0]
    assert lib.ofdmrx_abi_minor() == 9                               # additions within 1.9: detected by symbol
    assert hasattr(M.Receiver, "survey") and callable(modem_amd.survey_window) and callable(modem_amd.find_bands)
    assert os.path.exists(os.path.join(M.HERE, "bin", "survey"))
    assert "ofdmrx_band" in text and C.sizeof(M.Band) == 40


@pytest.mark.parametrize("name,count", [("ofdmrx_util_survey_window", 2), ("ofdmrx_util_survey", 10), ("ofdmrx_util_find_bands", 11)])
def test_ctypes_signatures_match_the_header(lib, name, count):
    import modem_amd.ofdmrx as M
    text = open(os.path.join(os.path.dirname(M.HERE), "include", "ofdmrx.h")).read()
    decl = text.split("int " + name + "(")[1].split(");")[0]
    kinds = []
    for arg in decl.split(","):
        arg = " ".join(arg.split())
        kinds.append(C.c_void_p if "*" in arg else {"int": C.c_int, "size_t": C.c_size_t, "long long": C.c_longlong,
                                                    "double": C.c_double}[arg.rsplit(" ", 1)[0]])
    assert len(kinds) == count and list(getattr(lib, name).argtypes) == kinds


def test_survey_refusals_come_before_the_handle_is_touched(lib):
    fake = C.c_void_p(1)
    din, dout = C.c_void_p(1 << 20), C.c_void_p(1 << 24)

    def call(h=fake, d_in=din, fmt=0, in_first=0, n_in=1280 * 4, nfft=1280, S=2, row_first=0, n_rows=2, d_out=dout):
        return lib.ofdmrx_util_survey(h, d_in, fmt, in_first, n_in, nfft, S, row_first, n_rows, d_out)

    assert call(h=None) == E_ARG and call(d_in=None) == E_ARG and call(d_out=None) == E_ARG
    assert call(n_in=0) == E_ARG and call(n_rows=0) == E_ARG
    assert call(fmt=-1) == E_ARG and call(fmt=3) == E_ARG
    for bad in (0, -1280, 640, 1024, 1279, 1281, 3840, 10240):
        assert call(nfft=bad) == E_ARG
    assert call(S=0) == E_ARG and call(S=-1) == E_ARG and call(S=65537) == E_ARG
    assert call(in_first=-1) == E_ARG and call(row_first=-1) == E_ARG
    assert call(n_in=1280 * 2 + 639) == E_ARG                         # rows 0 and 1 of two segments need 5 halves = 3200 positions
    assert call(in_first=1) == E_ARG                                  # row 0 begins at position 0
    assert call(row_first=1, n_rows=1, in_first=1281, n_in=4000) == E_ARG   # row 1 begins at position 1280
    assert call(row_first=2, n_rows=2) == E_ARG                       # rows 2 and 3 end at 5760 of 5120
    assert call(n_rows=3, n_in=4479) == E_ARG                         # rows 0 .. 2 end at 4480
    assert call(d_in=C.c_void_p((1 << 20) + 2)) == E_ARG              # off the sample-frame boundary
    assert call(fmt=2, d_in=C.c_void_p((1 << 20) + 4)) == E_ARG
    assert call(d_out=C.c_void_p((1 << 24) + 2)) == E_ARG             # off 4 bytes
    assert call(d_out=C.c_void_p((1 << 20) + 8)) == E_ARG             # the output overlaps the input
    assert call(d_in=C.c_void_p((1 << 24) + 1280 * 8 - 4)) == E_ARG   # ... from the other side
    assert call(in_first=(1 << 50) + 1) == E_ARG and call(row_first=(1 << 50) + 1) == E_ARG
    assert call(n_in=(1 << 50) + 1) == E_ARG and call(n_rows=(1 << 50) + 1, n_in=1 << 50) == E_ARG
    assert call(S=65536, n_rows=1 << 30, n_in=1 << 50) == E_ARG       # positions above 2^50
    assert call(S=8, n_rows=(1 << 28) // 1280 + 1, n_in=1 << 40) == E_ARG   # more partial sums than a launch holds


def test_create_reports_no_device_where_there_is_none(lib):
    """without a GPU the handle cannot be made: there is no CPU path behind the survey (with one, it is made)"""
    import torch
    import modem_amd.ofdmrx as M
    cfg = M.Config(1, 8000, 8, 0, 1, 0, 1, 0, None)
    h = C.c_void_p()
    r = lib.ofdmrx_create(C.byref(cfg), C.byref(h))
    if torch.cuda.is_available():
        assert r == 0
        lib.ofdmrx_destroy(h)
    else:
        assert r == E_NODEV and not h.value


# ---- the window

@pytest.mark.parametrize("N", SM.NFFT)
def test_library_window_equals_the_model(lib, N):
    import modem_amd
    got = modem_amd.survey_window(N)
    assert got.dtype == np.float32 and got.shape == (N,)
    assert np.array_equal(got, SM.window(N))
    assert got[0] == 0.0 and got[N // 2] == 1.0 and (got[1:] == got[1:][::-1]).all()
    assert abs(float((got.astype(np.float64) ** 2).sum()) - 0.375 * N) < 1e-3      # U = 3 N / 8


def test_window_refusals(lib):
    import modem_amd
    buf = np.full(5120 + 8, 7.0, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    for bad in (-1, 0, 640, 1024, 2048, 3840, 5121, 10240):
        assert lib.ofdmrx_util_survey_window(bad, p) == E_ARG
    assert lib.ofdmrx_util_survey_window(1280, None) == E_ARG
    assert (buf == 7.0).all()
    assert lib.ofdmrx_util_survey_window(1280, p) == 1280 and (buf[1280:] == 7.0).all()
    with pytest.raises(modem_amd.OfdmRxError):
        modem_amd.survey_window(1024)


# ---- the model: its tolerance on an fp32 evaluation and on wrong models

@pytest.fixture(scope="module")
def cases():
    """full-scale random input of 21 half segments and 37 samples, two rows of four segments, the model on it: computed once, read only"""
    out = {}
    for dt in (np.int16, np.uint8):
        pcm = CM.random_pcm(640 * 21 + 37, dt, seed=3)
        P, tol = SM.psd(pcm, 1280, 4, n_rows=2)
        for a in (pcm, P, tol):
            a.setflags(write=False)
        out[np.dtype(dt).name] = (pcm, P, tol)
    return out


@pytest.mark.parametrize("N,S", [(1280, 4), (1280, 9), (2560, 2), (5120, 2)])
def test_fp32_evaluation_stays_under_a_quarter_of_tol(N, S):
    pcm = CM.random_pcm((N // 2) * (2 * S + 1) + 5, np.int16, seed=N + S)
    P, tol = SM.psd(pcm, N, S, n_rows=2)
    assert P.shape == (2, N) and (tol > 0).all()
    w = SM.worst(SM.psd_fp32(pcm, N, S, n_rows=2), P, tol)
    print("N %d S %d: fp32 evaluation, worst error / tol %.4f; tol / P %.2e .. %.2e" % (N, S, w, (tol / P).min(), (tol / P).max()))
    assert w <= 0.25, (N, S, w)


@pytest.mark.parametrize("variant", SM.VARIANTS)
def test_wrong_variants_are_rejected(cases, variant):
    """each wrong model leaves the tolerance somewhere: the rule tells them from the definition"""
    pcm, P, tol = cases["uint8" if variant == "u8 without offset" else "int16"]
    w = SM.worst(SM.psd(pcm, 1280, 4, n_rows=2, variant=variant)[0], P, tol)
    print("%s: worst / tol %.3g" % (variant, w))
    assert w > 1.0, (variant, w)


def test_model_rows_do_not_depend_on_the_cut(cases):
    """the model itself: a row from only the samples it needs, with row_first > 0"""
    pcm, P, tol = cases["int16"]
    part, _ = SM.psd(pcm[2560:2560 + 3200], 1280, 4, row_first=1, n_rows=1, in_first=2560)
    assert np.array_equal(part[0], P[1])
    with pytest.raises(AssertionError):
        SM.psd(pcm[2560:2560 + 3199], 1280, 4, row_first=1, n_rows=1, in_first=2560)


@pytest.mark.parametrize("N", SM.NFFT)
def test_white_noise_reads_its_power(N):
    """complex white noise of power sigma^2 reads sigma^2: the mean over the bins within 5 / sqrt(S H) (the spectrum's mean is a
    weighted mean of |x|^2 over S H independent samples, relative deviation 1 each, weights between 1/2 and 1), every bin within 6
    / sqrt(S) x 1.03 (2 S degrees of freedom, less the overlap's 1/18 correlation at a hop of N / 2)"""
    S, sigma2 = 200, 0.02
    rng = np.random.default_rng(N)
    W = (N // 2) * (S + 1)
    x = np.sqrt(sigma2 / 2) * (rng.standard_normal(W) + 1j * rng.standard_normal(W))
    pcm = np.stack([x.real, x.imag], axis=1).astype(np.float32)
    P, _ = SM.psd(pcm, N)
    assert P.shape == (1, N)
    print("N %d: mean %.5f of %.5f, bins %.4f .. %.4f" % (N, P.mean(), sigma2, P.min(), P.max()))
    assert abs(P.mean() / sigma2 - 1.0) <= 5.0 / np.sqrt(S * N / 2)
    assert np.abs(P / sigma2 - 1.0).max() <= 6.0 * 1.03 / np.sqrt(S)


@pytest.mark.parametrize("N,k0", [(1280, 100), (1280, -640), (2560, -7), (5120, 2559)])
def test_a_tone_on_a_bin_centre_reads_its_height(N, k0):
    """A e^{2 pi i k0 n / N} reads A^2 (sum w)^2 / U at index k0 + N / 2, whatever the segment count"""
    A = 0.25
    n = np.arange(N // 2 * 7)
    x = A * np.exp(2j * np.pi * k0 * n / N)
    pcm = np.stack([x.real, x.imag], axis=1).astype(np.float32)
    P, tol = SM.psd(pcm, N, 3, n_rows=2)
    w = SM.window(N).astype(np.float64)
    want = A * A * w.sum() ** 2 / (w * w).sum()
    assert int(P[0].argmax()) == k0 + N // 2 and int(P[1].argmax()) == k0 + N // 2
    assert abs(P[0, k0 + N // 2] / want - 1.0) < 1e-6                 # (the fp32 rounding of the input)
    far = np.ones(N, bool)
    far[[(k0 + N // 2 + d) % N for d in (-1, 0, 1)]] = False          # Hann: the two neighbours (round the edge too) carry a quarter each
    assert P[0, far].max() < 1e-12 * want


# ---- the finder

def _lib_bands(row, rate=RW, max_bands=None, **kw):
    import modem_amd.ofdmrx as M
    L = M.load_library()
    row = np.ascontiguousarray(row, np.float32)
    cap = len(row) if max_bands is None else max_bands
    bands = (M.Band * max(cap, 1))()
    n, fl = C.c_size_t(0), C.c_double(-1.0)
    a = dict(thr_db=6.0, gap_hz=200.0, min_width_hz=1000.0, abs_floor=0.0)
    a.update(kw)
    r = L.ofdmrx_util_find_bands(row.ctypes.data_as(C.c_void_p), len(row), rate, a["thr_db"], a["gap_hz"], a["min_width_hz"], a["abs_floor"],
                                 cap, bands, C.byref(n), C.byref(fl))
    assert r == 0
    return [{k: getattr(bands[i], k) for k, _ in M.Band._fields_} for i in range(min(n.value, cap))], n.value, fl.value


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g["first_bin"] == w["first_bin"] and g["last_bin"] == w["last_bin"]
        for k in ("centre_hz", "width_hz", "power", "level_db"):
            if np.isfinite(w[k]):
                assert abs(g[k] - w[k]) <= 1e-9 * abs(w[k]), (k, g[k], w[k])
            else:
                assert g[k] == w[k]


def _row(N, runs, level=100.0, floor=1.0):
    row = np.full(N, floor, np.float32)
    for a, b in runs:
        row[a:b + 1] = level
    return row


def test_gaps_at_and_one_above_the_limit(lib):
    """37.5 Hz bins: a gap of 200 Hz bridges floor(200 / 37.5) = 5 unoccupied bins, not 6"""
    for gap, count in ((5, 1), (6, 2)):
        row = _row(1280, [(100, 139), (140 + gap, 179 + gap)])
        got, n, fl = _lib_bands(row)
        want, wfl = SM.find_bands(row, RW)
        assert n == count == len(want) and fl == wfl == 1.0
        _same(got, want)
    assert got[0]["first_bin"] == 100 and got[0]["last_bin"] == 139 and got[1]["first_bin"] == 146 and got[1]["last_bin"] == 185
    assert got[0]["centre_hz"] == (119.5 - 640) * 37.5 and got[0]["width_hz"] == 1500.0
    assert got[0]["power"] == 100.0 and abs(got[0]["level_db"] - 20.0) < 1e-6
    row = _row(1280, [(100, 139), (145, 184)])                       # bridged: the gap's bins count in width and power
    got, n, _ = _lib_bands(row)
    assert n == 1 and got[0]["last_bin"] == 184 and abs(got[0]["power"] - (80 * 100.0 + 5.0) / 85) < 1e-9
    got, n, _ = _lib_bands(row, gap_hz=0.0)
    assert n == 2


def test_runs_at_the_band_edges_do_not_wrap(lib):
    row = _row(1280, [(0, 39), (1240, 1279)])
    got, n, _ = _lib_bands(row)
    want, _ = SM.find_bands(row, RW)
    assert n == 2
    _same(got, want)
    assert (got[0]["first_bin"], got[0]["last_bin"], got[1]["first_bin"], got[1]["last_bin"]) == (0, 39, 1240, 1279)
    assert got[0]["centre_hz"] == (19.5 - 640) * 37.5 and got[1]["centre_hz"] == (1259.5 - 640) * 37.5


def test_a_spike_is_dropped_by_the_width(lib):
    row = _row(1280, [(640, 640), (700, 725), (800, 826)])           # DC spike; 26 bins = 975 Hz; 27 bins = 1012.5 Hz
    got, n, _ = _lib_bands(row)
    want, _ = SM.find_bands(row, RW)
    assert n == 1 and got[0]["first_bin"] == 800
    _same(got, want)
    got, n, _ = _lib_bands(row, min_width_hz=0.0)
    assert n == 3
    got, n, _ = _lib_bands(row, min_width_hz=975.0)                   # kept when the width is >= the limit
    assert n == 2


def test_max_bands_smaller_than_the_count(lib):
    row = _row(1280, [(100, 139), (300, 339), (500, 539)])
    got, n, _ = _lib_bands(row, max_bands=2)
    assert n == 3 and [g["first_bin"] for g in got] == [100, 300]
    import modem_amd.ofdmrx as M
    bands = (M.Band * 4)()
    C.memset(bands, 0x5a, C.sizeof(bands))
    cnt = C.c_size_t(0)
    assert lib.ofdmrx_util_find_bands(row.ctypes.data_as(C.c_void_p), 1280, RW, 6.0, 200.0, 1000.0, 0.0, 0, bands, C.byref(cnt), None) == 0
    assert cnt.value == 3 and bytes(bands) == b"\x5a" * C.sizeof(bands)       # max_bands 0: counted, nothing written; floor_out may be NULL


def test_an_all_zero_row(lib):
    row = np.zeros(1280, np.float32)
    for kw in ({}, {"abs_floor": 1e-6}):
        got, n, fl = _lib_bands(row, **kw)
        want, wfl = SM.find_bands(row, RW, **kw)
        assert n == 0 and want == [] and fl == wfl == kw.get("abs_floor", 0.0)
    row[100:140] = 1e-5                                               # less than half occupied over zeros: the median is 0
    got, n, fl = _lib_bands(row)
    assert n == 1 and fl == 0.0 and got[0]["level_db"] == np.inf and got[0]["first_bin"] == 100
    _same(got, SM.find_bands(row, RW)[0])
    got, n, fl = _lib_bands(row, abs_floor=1e-6)
    assert n == 1 and fl == 1e-6 and abs(got[0]["level_db"] - 10.0) < 1e-5
    got, n, fl = _lib_bands(row, abs_floor=1e-5)                      # not above floor 10^(6/10)
    assert n == 0


def test_library_finder_equals_the_model_on_noisy_rows(lib):
    rng = np.random.default_rng(7)
    for N in SM.NFFT:
        for trial in range(4):
            row = rng.chisquare(8, N) / 8.0
            for _ in range(5):
                a = int(rng.integers(0, N - 200))
                row[a:a + int(rng.integers(1, 200))] *= rng.uniform(2.0, 30.0)
            row = row.astype(np.float32)
            for kw in ({}, {"thr_db": 3.0, "gap_hz": 75.0, "min_width_hz": 0.0}, {"thr_db": 10.0, "gap_hz": 1000.0, "abs_floor": 1.5}):
                got, n, fl = _lib_bands(row, rate=RW * (1 + trial), **kw)
                want, wfl = SM.find_bands(row, RW * (1 + trial), **kw)
                assert n == len(want) and fl == wfl
                _same(got, want)


def test_finder_refusals(lib):
    import modem_amd
    import modem_amd.ofdmrx as M
    row = _row(1280, [(100, 139)])
    bands = (M.Band * 4)()
    C.memset(bands, 0x5a, C.sizeof(bands))
    n, fl = C.c_size_t(77), C.c_double(-3.0)
    p = row.ctypes.data_as(C.c_void_p)

    def call(psd=p, nfft=1280, rate=RW, thr=6.0, gap=200.0, width=1000.0, floor=0.0, b=bands, cnt=C.byref(n)):
        return lib.ofdmrx_util_find_bands(psd, nfft, rate, thr, gap, width, floor, 4, b, cnt, C.byref(fl))

    assert call(psd=None) == E_ARG and call(b=None) == E_ARG and call(cnt=None) == E_ARG
    for bad in (0, -1, 640, 1024, 1281, 10240):
        assert call(nfft=bad) == E_ARG
    nan, inf = float("nan"), float("inf")
    for bad in (0.0, -48000.0, nan, inf, -inf):
        assert call(rate=bad) == E_ARG
    for k in ("thr", "gap", "width", "floor"):
        for bad in (-1e-9, nan, inf, -inf):
            assert call(**{k: bad}) == E_ARG, (k, bad)
    assert n.value == 77 and fl.value == -3.0 and bytes(bands) == b"\x5a" * C.sizeof(bands)
    assert call() == 0 and n.value == 1 and fl.value == 1.0
    with pytest.raises(modem_amd.OfdmRxError):
        modem_amd.find_bands(row, -1.0)
    got = modem_amd.find_bands(row, RW)
    assert len(got) == 1 and got[0]["first_bin"] == 100 and got[0]["last_bin"] == 139


# ---- the capture of wideband_fixture.py

@pytest.fixture(scope="module")
def capture():
    pcm, pays = WF.capture()
    rows = {N: SM.psd(pcm, N)[0][0] for N in SM.NFFT}
    for a in (pcm, pays) + tuple(rows.values()):
        a.setflags(write=False)
    return pcm, pays, rows


@pytest.mark.parametrize("thr", [6.0, 10.0])
@pytest.mark.parametrize("N", SM.NFFT)
def test_fixture_capture_has_four_bands(lib, capture, N, thr):
    """one row over the whole capture: exactly four bands, centres within one bin width of SIGNAL_HZ, the floor within 5 % of the
    fixture's 2 sigma^2; the library's finder on the fp32 row agrees with the model's"""
    pcm, pays, rows = capture
    bands, fl = SM.find_bands(rows[N], RW, thr_db=thr, gap_hz=200.0, min_width_hz=1000.0)
    print("N %d thr %g: floor %.4g, centres %s, widths %s" % (N, thr, fl, [b["centre_hz"] for b in bands], [b["width_hz"] for b in bands]))
    assert len(bands) == 4
    for b, f in zip(bands, WF.SIGNAL_HZ):
        assert abs(b["centre_hz"] - f) <= RW / N, (b, f)
        assert 2700.0 <= b["width_hz"] <= 3000.0
    assert abs(fl / (2 * WF.SIGMA ** 2) - 1.0) <= 0.05
    row32 = rows[N].astype(np.float32)
    got, n, gfl = _lib_bands(row32, thr_db=thr)
    want, wfl = SM.find_bands(row32, RW, thr_db=thr)
    assert n == 4 and gfl == wfl
    _same(got, want)
    if N == 1280 and thr == 6.0:
        assert [b["centre_hz"] for b in bands] == [-13012.5, 3000.0, 7012.5, 10987.5]


def test_fixture_waterfall(capture):
    """N = 1280, S = 64: 17 rows; the four frames start one after another and show in rows 1-12, 2-13, 3-14 and 4-16"""
    pcm, pays, rows = capture
    P, _ = SM.psd(pcm, 1280, 64)
    assert P.shape == (17, 1280)
    seen = [[] for _ in WF.SIGNAL_HZ]
    for r in range(17):
        for b in SM.find_bands(P[r], RW)[0]:
            k = int(np.argmin([abs(b["centre_hz"] - f) for f in WF.SIGNAL_HZ]))
            assert abs(b["centre_hz"] - WF.SIGNAL_HZ[k]) <= 400.0
            seen[k].append(r)
    assert seen == [list(range(1, 13)), list(range(2, 14)), list(range(3, 15)), list(range(4, 17))]


def test_oracle_decodes_the_found_centres(capture):
    """the loop's twin on the CPU: the front-end model's rows at the FOUND centres through the oracle.  Every channel yields exactly
    one status-0 record, whose payload is the golden one; a failed-header record beside it is allowed only in the channel next above
    the strong frame (wideband_fixture.py)"""
    pcm, pays, rows = capture
    bands, _ = SM.find_bands(rows[1280], RW)
    centres = [b["centre_hz"] for b in bands]
    assert len(centres) == 4
    v, _, _ = CM.channelize(pcm, WF.DECIM, centres)
    for c in range(4):
        row = np.stack([v[c].real, v[c].imag], axis=1).astype(np.float32)
        good, failed = 0, 0
        for k in range(4):
            out, r = O.decode(row, skip=k)
            if r.status == 1:                                        # no further preamble
                break
            if r.status == 0:
                good += 1
                assert (out == pays[c]).all(), c
            else:
                failed += 1
        print("channel %d at %.1f Hz: %d decoded, %d failed headers" % (c, centres[c], good, failed))
        assert good == 1, (c, good)
        assert failed == 0 or c == 3, (c, failed)
