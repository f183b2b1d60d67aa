"""The wideband front end without a GPU: the library's taps against the formula, the filter they make, the
float64 model of channelize_model.py on tones, the tolerance rule on an fp32 evaluation and on deliberately wrong models, and the
argument errors of the new entries that need no look into the handle."""
import ctypes as C
import os

import numpy as np
import pytest

import channelize_model as CM

E_ARG = -1
NAMES = ("ofdmrx_util_channelize_taps", "ofdmrx_util_channelize", "ofdmrx_bank_begin_wideband", "ofdmrx_bank_push_wideband")
ALL_D = list(range(2, 33))


@pytest.fixture(scope="module")
def lib():
    import modem_amd
    modem_amd.build()
    return modem_amd.load_library()


def test_symbols_exported_and_declared(lib):
    import modem_amd
    import modem_amd.ofdmrx as M
    text = open(os.path.join(os.path.dirname(M.HERE), "include", "ofdmrx.h")).read()
    for name in NAMES:
        assert name in M.EXPORTS
        getattr(lib, name)
        assert name + "(" in text and name in text.split("#define OFDMRX_ABI_MINOR")[0]
    assert lib.ofdmrx_abi_minor() == 9                               # additions within 1.9: detected by symbol
    assert hasattr(M.Receiver, "channelize") and callable(modem_amd.channelize_taps)
    assert hasattr(M.Receiver, "wideband_bank") and issubclass(M.WidebandBank, M.Bank)


@pytest.mark.parametrize("D", ALL_D)
def test_taps_match_the_formula(lib, D):
    import modem_amd
    got = modem_amd.channelize_taps(D)
    T = 24 * D + 1
    assert got.dtype == np.float32 and got.shape == (T,)
    want = CM.taps(D)
    ulp = np.spacing(np.abs(want))
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    assert abs(got.astype(np.float64).sum() - 1.0) <= T * 2.0 ** -24
    assert (got == got[::-1]).all()


def test_taps_refusals(lib):
    import modem_amd
    buf = np.full(24 * 33 + 1, 7.0, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    for bad in (-1, 0, 1, 33, 1 << 20):
        assert lib.ofdmrx_util_channelize_taps(bad, p) == E_ARG
    assert lib.ofdmrx_util_channelize_taps(6, None) == E_ARG
    assert (buf == 7.0).all()
    assert lib.ofdmrx_util_channelize_taps(2, p) == 49 and (buf[49:] == 7.0).all()
    with pytest.raises(modem_amd.OfdmRxError):
        modem_amd.channelize_taps(33)


@pytest.mark.parametrize("D", ALL_D)
def test_filter_passband_and_stopband(lib, D):
    """on the library's own taps, in float64: |f| <= rate / 4 within +-0.01 dB, |f| >= rate / 2 at most -70 dB (f in cycles per
    wideband sample: rate / 4 is 1 / (4 D))"""
    import modem_amd
    h = modem_amd.channelize_taps(D).astype(np.float64)
    N = 1 << 16
    H = np.abs(np.fft.rfft(h, N))
    f = np.arange(N // 2 + 1) / N
    pb = np.concatenate([H[f <= 0.25 / D], np.abs(CM.response(h, [0.25 / D]))])
    sb = np.concatenate([H[f >= 0.5 / D], np.abs(CM.response(h, [0.5 / D]))])
    pb_db, sb_db = 20 * np.log10(pb), 20 * np.log10(sb.max())
    print("D %d: passband %+.4f / %+.4f dB, stopband %.1f dB, sum|h| %.3f" % (D, pb_db.max(), pb_db.min(), sb_db, np.abs(h).sum()))
    assert pb_db.max() <= 0.01 and pb_db.min() >= -0.01, (D, pb_db.max(), pb_db.min())
    assert sb_db <= -70.0, (D, sb_db)


TONES = [(D, f_c, d) for D, f_c in ((2, 1000.0), (6, -13000.0), (6, 7000.25), (32, -100000.0))
         for d in (500.0, -1999.0, 3000.0, 3999.0, 5000.0, -9000.0) if abs(f_c + d) <= D * 4000]   # (the tone lies inside the capture)


@pytest.mark.parametrize("D,f_c,delta", TONES)
def test_model_on_a_tone(D, f_c, delta):
    """a tone at f_c + delta comes out as a tone at delta of gain |H(delta)|: pass band, transition band, stop band; negative f_c"""
    rate = 8000
    rw = D * rate
    A = 0.5
    W = 60 * D + 5
    m = np.arange(W)
    x = A * np.exp(2j * np.pi * (f_c + delta) * m / rw)
    pcm = np.stack([x.real, x.imag], axis=1).astype(np.float32)
    v, tol, tie = CM.channelize(pcm, D, [f_c], rate)
    assert v.shape == (1, CM.n_outputs(W, D)) and tie > 1e-6
    inc, _ = CM.inc_of(f_c, rw)
    f_nco = (inc if inc < 2 ** 31 else inc - 2 ** 32) * rw / 2.0 ** 32   # what the integer increment really mixes by
    d = f_c + delta - f_nco
    Hd = CM.response(CM.taps(D), [d / rw])[0]
    n = np.arange(24, v.shape[1])                                    # past the filter's fill
    want = A * Hd * np.exp(2j * np.pi * d * n * D / rw)
    assert np.abs(v[0, 24:] - want).max() <= 1e-6 * A                # (the fp32 rounding of the input: 6e-8 sum|h|)
    gain = np.abs(v[0, 24:]).mean() / A
    if abs(delta) <= rate / 4:
        assert abs(20 * np.log10(gain)) <= 0.01
    elif abs(delta) >= rate / 2:
        assert gain <= 10 ** (-70 / 20.0) + 1e-6
    else:
        assert abs(gain - abs(Hd)) <= 1e-6 and 1e-4 < gain < 1.0


CENTRES = {2: [1234.567, -5000.0], 6: [-13000.0, 3000.25, 11050.0], 32: [100001.3, -2718.28]}


@pytest.fixture(scope="module")
def cases():
    """full-scale random int16 input, the model on it: computed once, read only"""
    out = {}
    for D in (2, 6, 32):
        W = {2: 4001, 6: 4001, 32: 40001}[D]                         # (long enough for a phase increment that is off to drift)
        pcm = CM.random_pcm(W, np.int16, seed=D)
        v, tol, tie = CM.channelize(pcm, D, CENTRES[D])
        for a in (pcm, v, tol):
            a.setflags(write=False)
        out[D] = (pcm, v, tol, tie)
    return out


@pytest.mark.parametrize("D", [2, 6, 32])
def test_fp32_evaluation_stays_under_a_quarter_of_tol(cases, D):
    pcm, v, tol, tie = cases[D]
    assert tie > 1e-6 and (tol > 0).all()
    w = CM.worst(CM.channelize_fp32(pcm, D, CENTRES[D]), v, tol)
    print("D %d: fp32 evaluation, worst error / tol %.4f" % (D, w))
    assert w <= 0.25, (D, w)


# (a centre tap scaled by 1 + 2^-10 moves an output by 0.4 tol at D = 32: the rule cannot see it there, so that pair is left out)
@pytest.mark.parametrize("D,variant", [(D, v) for v in CM.VARIANTS for D in (2, 6, 32) if (D, v) != (32, "centre tap")])
def test_wrong_variants_are_rejected(cases, D, variant):
    """each wrong model leaves the tolerance somewhere: the rule tells them from the definition"""
    pcm, v, tol, _ = cases[D]
    w = CM.worst(CM.channelize(pcm, D, CENTRES[D], variant=variant)[0], v, tol)
    print("D %d %s: worst / tol %.3g" % (D, variant, w))
    assert w > 1.0, (D, variant, w)


def test_model_cuts_into_blocks(cases):
    """the model itself: a block with its history gives the outputs of the whole capture"""
    D = 6
    pcm, v, tol, _ = cases[D]
    T = 24 * D + 1
    o0 = 40
    i0 = o0 * D - (T - 1)
    part, _, _ = CM.channelize(pcm[i0:], D, CENTRES[D], out_first=o0, in_first=i0)
    assert np.array_equal(part, v[:, o0:])


def test_channelize_bad_arguments(lib):
    """every refusal that needs no look into the handle comes before any device call (and before the handle is touched)"""
    fake = C.c_void_p(1)
    f = np.array([1000.0, -2000.0], np.float64)
    pf = f.ctypes.data_as(C.c_void_p)
    din, dout = C.c_void_p(1 << 20), C.c_void_p(1 << 24)

    def call(h=fake, d_in=din, fmt=0, in_first=0, n_in=4096, decim=6, centres=pf, n_ch=2, out_first=0, n_out=100, d_out=dout, stride=100):
        return lib.ofdmrx_util_channelize(h, d_in, fmt, in_first, n_in, decim, centres, n_ch, out_first, n_out, d_out, stride)

    assert call(h=None) == E_ARG
    assert call(d_in=None) == E_ARG and call(d_out=None) == E_ARG and call(centres=None) == E_ARG
    assert call(n_in=0) == E_ARG and call(n_out=0) == E_ARG
    assert call(n_ch=0) == E_ARG and call(n_ch=65536) == E_ARG
    assert call(decim=1) == E_ARG and call(decim=33) == E_ARG
    assert call(fmt=-1) == E_ARG and call(fmt=3) == E_ARG
    assert call(in_first=-1) == E_ARG and call(out_first=-1) == E_ARG
    assert call(stride=99) == E_ARG
    assert call(n_out=684) == E_ARG                                   # output 683 needs position 4098 of 4096
    assert call(in_first=1, out_first=24) == E_ARG                    # history: out_first D - 144 = 0 < in_first
    assert call(d_out=C.c_void_p((1 << 20) + 8)) == E_ARG             # the output overlaps the input
    assert call(d_in=C.c_void_p((1 << 20) + 2)) == E_ARG              # off the sample-frame boundary
    for bad in (float("nan"), float("inf")):
        g = np.array([1000.0, bad], np.float64)
        assert call(centres=g.ctypes.data_as(C.c_void_p)) == E_ARG


def test_wideband_bank_bad_arguments(lib):
    """as test_bank_abi_cpu.py: what needs no look into the handle is refused first"""
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(1)
    f = np.array([1000.0, -2000.0], np.float64)
    begin = lib.ofdmrx_bank_begin_wideband
    assert begin(None, 2, p(f), 6, 0) == E_ARG
    assert begin(fake, 2, None, 6, 0) == E_ARG
    assert begin(fake, 0, p(f), 6, 0) == E_ARG and begin(fake, 65536, p(f), 6, 0) == E_ARG
    assert begin(fake, 2, p(f), 1, 0) == E_ARG and begin(fake, 2, p(f), 33, 0) == E_ARG
    assert begin(fake, 2, p(f), 6, -1) == E_ARG and begin(fake, 2, p(f), 6, 3) == E_ARG
    pcm = np.zeros((1000, 2), np.int16)
    out, res = np.zeros((8, 5380), np.uint8), np.zeros(8 * 56, np.uint8)
    rc, ri = np.zeros(8, np.int32), np.zeros(8, np.int64)
    nrec, nleft = np.zeros(1, np.uintp), np.zeros(1, np.uintp)
    cnt = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_size_t))

    def push(h=fake, smp=pcm, n=1000, cap=8, o=out, r=res, c=rc, i=ri, a=nrec, b=nleft):
        return lib.ofdmrx_bank_push_wideband(h, p(smp), n, 0, cap, p(o), p(r), p(c), p(i), cnt(a), cnt(b))

    assert push(h=None) == E_ARG
    assert push(a=None) == E_ARG and push(b=None) == E_ARG
    for k in "oric":                                             # NULL outputs (any of the four arrays) with max_records > 0
        assert push(**{k: None}) == E_ARG
