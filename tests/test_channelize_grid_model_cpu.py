"""The grid front end without a GPU: the float64 model of channelize_grid_model.py against section 4.14's
model at the slot centres and against the direct sum, the library's taps and the filter they make at the new decimations, the
tolerance rule on an fp32 evaluation and on deliberately wrong models, the argument errors that need no look into the handle, and
the captures of grid_fixture.py through the oracle on the model's rows - which fixes what test_gpu_grid_bank.py expects."""
import ctypes as C
import os

import numpy as np
import pytest

import channelize_grid_model as G
import channelize_model as CM
import grid_fixture as GF

E_ARG = -1
NAMES = ("ofdmrx_util_channelize_grid_taps", "ofdmrx_util_channelize_grid", "ofdmrx_bank_begin_wideband_grid")


@pytest.fixture(scope="module")
def lib():
    import modem_amd
    modem_amd.build()
    return modem_amd.load_library()


def _S(tol, D):
    return tol / (2.0 ** -24 * (G.A_TOL + G.B_TOL * np.log2(2 * D)))


def test_symbols_exported_and_declared(lib):
    import modem_amd
    import modem_amd.ofdmrx as M
    text = open(os.path.join(os.path.dirname(M.HERE), "include", "ofdmrx.h")).read()
    for name in NAMES:
        assert name in M.EXPORTS
        getattr(lib, name)
        assert name + "(" in text and name in text.split("#define OFDMRX_ABI_MINOR")[0]
    assert lib.ofdmrx_abi_minor() == 9                               # additions within 1.9: detected by symbol
    assert hasattr(M.Receiver, "channelize_grid") and callable(modem_amd.channelize_grid_taps) and callable(modem_amd.grid_centres)
    assert hasattr(M.Receiver, "wideband_grid_bank") and issubclass(M.WidebandGridBank, M.WidebandBank)
    assert (modem_amd.grid_centres(2, 8000) == [-8000.0, -4000.0, 0.0, 4000.0]).all()
    assert (modem_amd.grid_centres(512, 8000, [511, -512]) == [511 * 4000.0, -512 * 4000.0]).all()


@pytest.mark.parametrize("D", [2, 4, 16, 32])
def test_model_equals_the_plain_model_at_the_slot_centres(D):
    """all slots, full-scale random int16: the polyphase form is section 4.14's sum at the centres k rate / 2, within 1e-12 S"""
    pcm = G.random_pcm(60 * D + 7, np.int16, seed=D)
    v, tol = G.grid(pcm, D)
    w, _, tie = CM.channelize(pcm, D, G.centres(D))
    assert tie > 0.49                                                # k 2^32 / M is an integer: no rounding of the increment
    assert v.shape == w.shape == (2 * D, G.n_outputs(60 * D + 7, D))
    worst = float(np.max(np.abs(v - w) / _S(tol, D)))
    print("D %d: grid model against the plain model, worst |difference| / S %.3g" % (D, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize("D", [64, 512])
def test_model_equals_the_direct_sum(D):
    M = 2 * D
    slots = [-M // 2, -3, 0, 1, M // 2 - 1]
    pcm = G.random_pcm(30 * D + 7, np.int16, seed=D)
    v, tol = G.grid(pcm, D, slots)
    outs = [0, 1, 7, v.shape[1] - 1]
    d = G.direct(pcm, D, slots, outs)
    worst = float(np.max(np.abs(v[:, outs] - d) / _S(tol, D)[:, outs]))
    print("D %d: grid model against the direct sum, worst |difference| / S %.3g" % (D, worst))
    assert worst <= 1e-12


def test_model_positions_and_rows():
    """the model itself: a block with its history gives the outputs of the whole capture; `rows` is the same sum"""
    D = 8
    pcm = G.random_pcm(60 * D + 5, np.int16, seed=3)
    v, tol = G.grid(pcm, D)
    o0 = 30
    i0 = o0 * D - 24 * D
    part, ptol = G.grid(pcm[i0:], D, out_first=o0, in_first=i0)
    assert np.array_equal(part, v[:, o0:]) and np.array_equal(ptol, tol[:, o0:])
    r = G.rows(pcm, D, G.all_slots(D))
    assert np.abs((r[..., 0] + 1j * r[..., 1]) - v).max() <= 2.0 ** -23 * np.abs(v).max()      # (rows are rounded to fp32)


@pytest.mark.parametrize("D", G.ALL_D)
def test_taps_are_the_models_bytes(lib, D):
    import modem_amd
    got = modem_amd.channelize_grid_taps(D)
    assert got.dtype == np.float32 and got.shape == (24 * D + 1,)
    assert got.tobytes() == G.taps(D).tobytes()
    if D <= 32:
        assert got.tobytes() == modem_amd.channelize_taps(D).tobytes()


def test_taps_refusals(lib):
    import modem_amd
    buf = np.full(24 * 512 + 2, 7.0, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    for bad in (-2, 0, 1, 3, 6, 48, 1024, 1 << 20):
        assert lib.ofdmrx_util_channelize_grid_taps(bad, p) == E_ARG, bad
    assert lib.ofdmrx_util_channelize_grid_taps(8, None) == E_ARG
    assert (buf == 7.0).all()
    assert lib.ofdmrx_util_channelize_grid_taps(2, p) == 49 and (buf[49:] == 7.0).all()
    assert lib.ofdmrx_util_channelize_grid_taps(512, p) == 12289 and buf[12289] == 7.0
    with pytest.raises(modem_amd.OfdmRxError):
        modem_amd.channelize_grid_taps(6)
    with pytest.raises(modem_amd.OfdmRxError):
        modem_amd.grid_centres(8, 8000, [8])


@pytest.mark.parametrize("D", [64, 128, 256, 512])
def test_filter_passband_and_stopband(lib, D):
    """on the library's own taps, in float64: |f| <= rate / 4 within +-0.01 dB, |f| >= rate / 2 at most -70 dB"""
    import modem_amd
    h = modem_amd.channelize_grid_taps(D).astype(np.float64)
    N = 1 << 20
    H = np.abs(np.fft.rfft(h, N))
    f = np.arange(N // 2 + 1) / N
    pb = np.concatenate([H[f <= 0.25 / D], np.abs(CM.response(h, [0.25 / D]))])
    sb = np.concatenate([H[f >= 0.5 / D], np.abs(CM.response(h, [0.5 / D]))])
    pb_db, sb_db = 20 * np.log10(pb), 20 * np.log10(sb.max())
    print("D %d: passband %+.4f / %+.4f dB, stopband %.1f dB, sum|h| %.4f, h[0] %.3g" % (D, pb_db.max(), pb_db.min(), sb_db, np.abs(h).sum(), h[0]))
    assert pb_db.max() <= 0.01 and pb_db.min() >= -0.01, (D, pb_db.max(), pb_db.min())
    assert sb_db <= -70.0, (D, sb_db)


@pytest.fixture(scope="module")
def cases():
    """full-scale random int16 input and the model on it, all slots: computed once, read only"""
    out = {}
    for D in G.ALL_D:
        pcm = G.random_pcm(40 * D + 7, np.int16, seed=D)
        v, tol = G.grid(pcm, D)
        for a in (pcm, v, tol):
            a.setflags(write=False)
        out[D] = (pcm, v, tol)
    return out


@pytest.mark.parametrize("D", G.ALL_D)
def test_fp32_evaluation_stays_inside_the_tolerance(cases, D):
    pcm, v, tol = cases[D]
    assert (tol > 0).all()
    w = G.worst(G.grid_fp32(pcm, D), v, tol)
    print("D %d: fp32 evaluation, worst error / tol %.4f" % (D, w))
    assert w <= 1.0, (D, w)


@pytest.mark.parametrize("D,variant", [(D, v) for v in G.VARIANTS for D in (2, 64)])
def test_wrong_variants_are_rejected(cases, D, variant):
    """each wrong model leaves the tolerance somewhere: the rule tells them from the definition"""
    pcm, v, tol = cases[D]
    w = G.worst(G.grid(pcm, D, variant=variant)[0], v, tol)
    print("D %d %s: worst / tol %.3g" % (D, variant, w))
    assert w > 1.0, (D, variant, w)


def test_grid_bad_arguments(lib):
    """every refusal that needs no look into the handle comes before any device call (and before the handle is touched)"""
    fake = C.c_void_p(1)
    k = np.array([3, -16], np.int32)
    pk = k.ctypes.data_as(C.c_void_p)
    din, dout = C.c_void_p(1 << 20), C.c_void_p(1 << 24)

    def call(h=fake, d_in=din, fmt=0, in_first=0, n_in=4096, decim=16, slots=pk, n=2, out_first=0, n_out=100, d_out=dout, stride=100):
        return lib.ofdmrx_util_channelize_grid(h, d_in, fmt, in_first, n_in, decim, slots, n, out_first, n_out, d_out, stride)

    assert call(h=None) == E_ARG
    assert call(d_in=None) == E_ARG and call(d_out=None) == E_ARG
    assert call(n_in=0) == E_ARG and call(n_out=0) == E_ARG
    assert call(n=0) == E_ARG and call(n=65536) == E_ARG
    assert call(slots=None) == E_ARG and call(slots=None, n=31) == E_ARG          # NULL slots: only with n_slots = M = 32
    for bad in (-16, 0, 1, 3, 12, 24, 33, 1024):
        assert call(decim=bad) == E_ARG, bad
    for bad in (16, -17, 1 << 20, -(1 << 31)):
        g = np.array([3, bad], np.int32)
        assert call(slots=g.ctypes.data_as(C.c_void_p)) == E_ARG, bad
    assert call(fmt=-1) == E_ARG and call(fmt=3) == E_ARG
    assert call(in_first=-1) == E_ARG and call(out_first=-1) == E_ARG
    assert call(stride=99) == E_ARG
    assert call(n_out=258) == E_ARG                                   # output 257 needs position 4112 of 4096
    assert call(in_first=1, out_first=24) == E_ARG                    # history: out_first D - 384 = 0 < in_first
    assert call(d_out=C.c_void_p((1 << 20) + 8)) == E_ARG             # the output overlaps the input
    assert call(d_in=C.c_void_p((1 << 20) + 2)) == E_ARG              # off the sample-frame boundary


def test_grid_bank_bad_arguments(lib):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(1)
    k = np.array([3, -16], np.int32)
    begin = lib.ofdmrx_bank_begin_wideband_grid
    assert begin(None, 2, p(k), 16, 0) == E_ARG
    assert begin(fake, 0, p(k), 16, 0) == E_ARG and begin(fake, 65536, p(k), 16, 0) == E_ARG
    assert begin(fake, 2, None, 16, 0) == E_ARG and begin(fake, 31, None, 16, 0) == E_ARG
    for bad in (1, 6, 48, 1024):
        assert begin(fake, 2, p(k), bad, 0) == E_ARG, bad
    assert begin(fake, 2, p(k), 16, -1) == E_ARG and begin(fake, 2, p(k), 16, 3) == E_ARG
    assert begin(fake, 2, p(np.array([3, 16], np.int32)), 16, 0) == E_ARG and begin(fake, 2, p(np.array([-17, 3], np.int32)), 16, 0) == E_ARG


@pytest.mark.parametrize("which", ["a", "b"])
def test_fixture_through_the_oracle(which):
    """the CPU twin of test_gpu_grid_bank.py: the oracle on the model's rows of every opened slot gives exactly the table the fixture
    states - every frame from its own slot at the frame's own sc_start, and the failed records of the slots beside a strong frame"""
    cfg, cap, want = (GF.A, GF.capture_a, GF.EXPECTED_A) if which == "a" else (GF.B, GF.capture_b, GF.EXPECTED_B)
    pcm, pays = cap()
    rows = G.rows(pcm, cfg["D"], cfg["open"])
    for i, k in enumerate(cfg["open"]):
        recs = GF.oracle_records(rows[i])
        assert GF.table(recs, pays) == want.get(k, []), k
        for (o, r), (status, frame) in zip(recs, want.get(k, [])):
            if status == 0:
                assert r.sc_start == GF.sc_start(cfg, frame) and r.bit_flips == 0, (k, r.sc_start)
