"""The entries of the wideband front end for a real capture without a GPU: both symbols exported and
declared, every refusal that needs no look into the handle, and the Python wrappers' argument handling (on a stand-in for the
library that records what it is called with).  The centre rule reads the handle's rate, and the refusals between open banks need a
handle too: test_gpu_channelize_real.py and test_gpu_wideband_real_bank.py have them."""
import ctypes as C
import fractions
import os

import numpy as np
import pytest

E_ARG = -1
NAMES = ("ofdmrx_util_channelize_real", "ofdmrx_bank_begin_wideband_real")


@pytest.fixture(scope="module")
def lib():
    import modem_amd
    modem_amd.build()
    return modem_amd.load_library()


def test_symbols_exported_and_declared(lib):
    import modem_amd.ofdmrx as M
    text = open(os.path.join(os.path.dirname(M.HERE), "include", "ofdmrx.h")).read()
    for name in NAMES:
        assert name in M.EXPORTS
        getattr(lib, name)
        assert name + "(" in text and name in text.split("#define OFDMRX_ABI_MINOR")[0]
    assert lib.ofdmrx_abi_minor() == 9                               # additions within 1.9: detected by symbol
    assert callable(M.Receiver.channelize_real) and callable(M.Receiver.wideband_real_bank)
    assert issubclass(M.WidebandRealBank, M.WidebandBank)


def test_channelize_real_bad_arguments(lib):
    """every refusal that needs no look into the handle comes before any device call (and before the handle is touched)"""
    fake = C.c_void_p(1)
    f = np.array([3000.0, -5000.0], np.float64)
    pf = f.ctypes.data_as(C.c_void_p)
    din, dout = C.c_void_p(1 << 20), C.c_void_p(1 << 24)

    def call(h=fake, d_in=din, fmt=0, in_first=0, n_in=4096, p=25, q=4, centres=pf, n_ch=2, out_first=0, n_out=100, d_out=dout, stride=100):
        return lib.ofdmrx_util_channelize_real(h, d_in, fmt, in_first, n_in, p, q, centres, n_ch, out_first, n_out, d_out, stride)

    for bad in ((0, 4), (25, 0), (-25, 4), (25, -4), (35, 17), (7, 4), (129, 4), (513, 16), (33, 1), (1, 1), (2, 2), (6, 0)):
        assert call(p=bad[0], q=bad[1]) == E_ARG, bad                # bad p / q, Q above 16, the ratio outside 2 .. 32
    assert call(h=None) == E_ARG and call(h=None, p=6, q=1) == E_ARG
    assert call(d_in=None) == E_ARG and call(d_out=None) == E_ARG and call(centres=None) == E_ARG
    assert call(n_in=0) == E_ARG and call(n_out=0) == E_ARG
    assert call(n_ch=0) == E_ARG and call(n_ch=65536) == E_ARG
    assert call(fmt=-1) == E_ARG and call(fmt=3) == E_ARG
    assert call(in_first=-1) == E_ARG and call(out_first=-1) == E_ARG
    assert call(stride=99) == E_ARG
    assert call(n_out=657, stride=657) == E_ARG                       # output 656 needs position 656 * 25 div 4 = 4100 of 4096
    assert call(p=6, q=1, n_out=684, stride=684) == E_ARG             # D = 6: output 683 needs position 4098 of 4096
    assert call(in_first=1, out_first=24) == E_ARG                    # history: 24 * 25 div 4 - 150 = 0 < in_first
    assert call(d_out=C.c_void_p((1 << 20) + 8)) == E_ARG             # the output overlaps the input
    assert call(d_out=C.c_void_p((1 << 20) + 2 * 4096 - 8)) == E_ARG  # ... its last sample (n_in counts 2-byte samples)
    assert call(d_in=C.c_void_p((1 << 20) + 1)) == E_ARG              # S16 off the sample's boundary
    assert call(fmt=2, d_in=C.c_void_p((1 << 20) + 2)) == E_ARG       # F32 off the sample's boundary
    assert call(d_out=C.c_void_p((1 << 24) + 4)) == E_ARG             # off 8 bytes
    assert call(n_in=1 << 51) == E_ARG and call(out_first=(1 << 50) + 1) == E_ARG
    for bad in (float("nan"), float("inf"), -float("inf")):
        g = np.array([3000.0, bad], np.float64)
        assert call(centres=g.ctypes.data_as(C.c_void_p)) == E_ARG


def test_wideband_real_bank_bad_arguments(lib):
    """what needs no look into the handle is refused first"""
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(1)
    f = np.array([3000.0, -5000.0], np.float64)
    begin = lib.ofdmrx_bank_begin_wideband_real
    assert begin(None, 2, p(f), 25, 4, 0) == E_ARG and begin(None, 2, p(f), 6, 1, 0) == E_ARG
    assert begin(fake, 2, None, 25, 4, 0) == E_ARG
    assert begin(fake, 0, p(f), 25, 4, 0) == E_ARG and begin(fake, 65536, p(f), 25, 4, 0) == E_ARG
    for bad in ((0, 4), (25, 0), (-25, 4), (25, -4), (35, 17), (7, 4), (129, 4), (33, 1), (1, 1)):
        assert begin(fake, 2, p(f), bad[0], bad[1], 0) == E_ARG, bad
    assert begin(fake, 2, p(f), 25, 4, -1) == E_ARG and begin(fake, 2, p(f), 25, 4, 3) == E_ARG
    assert begin(fake, 2, p(f), 12, 2, 3) == E_ARG and begin(fake, 0, p(f), 12, 2, 0) == E_ARG


class _Recorder:
    """stands in for the library: records the last call of each entry, answers 0"""

    def __init__(self):
        self.calls = {}

    def __getattr__(self, name):
        def f(*args):
            self.calls[name] = args
            return 0
        return f


def _receiver():
    import modem_amd.ofdmrx as M
    rx = object.__new__(M.Receiver)
    rx._lib, rx._h, rx.sample_rate = _Recorder(), C.c_void_p(), 8000   # (an empty handle: close() has nothing to destroy)
    return rx


@pytest.mark.parametrize("decim,p,q", [(6, 6, 1), ((25, 4), 25, 4), ([50, 8], 50, 8), (fractions.Fraction(50, 8), 25, 4), (fractions.Fraction(6), 6, 1)])
def test_channelize_real_wrapper_arguments(decim, p, q):
    """decim as an int, a pair and a Fraction; the centres as doubles; out_stride defaults to n_out"""
    rx = _receiver()
    rx.channelize_real(1 << 20, 0, 7, 4096, decim, [3000, -5000.5, 7000], 40, 100, 1 << 24)
    a = rx._lib.calls["ofdmrx_util_channelize_real"]
    assert a[1:7] == (1 << 20, 0, 7, 4096, p, q) and a[8:] == (3, 40, 100, 1 << 24, 100)
    got = np.ctypeslib.as_array(C.cast(a[7], C.POINTER(C.c_double)), shape=(3,))
    assert list(got) == [3000.0, -5000.5, 7000.0]
    rx.channelize_real(1 << 20, 2, 0, 4096, decim, 3000.0, 0, 100, 1 << 24, out_stride=128)
    a = rx._lib.calls["ofdmrx_util_channelize_real"]
    assert a[2] == 2 and a[5:7] == (p, q) and a[8] == 1 and a[12] == 128


@pytest.mark.parametrize("dtype,fmt", [(np.int16, 0), (np.uint8, 1), (np.float32, 2)])
def test_wideband_real_bank_wrapper_arguments(dtype, fmt):
    """the begin's arguments, and push: a 1-D block of the bank's dtype, its length in samples; anything else is refused in Python"""
    import modem_amd.ofdmrx as M
    rx = _receiver()
    bank = rx.wideband_real_bank([3000.0, -17000.0], (12, 2), dtype=dtype)
    a = rx._lib.calls["ofdmrx_bank_begin_wideband_real"]
    assert a[1] == 2 and a[3:] == (12, 2, fmt)
    assert isinstance(bank, M.WidebandRealBank) and bank.n_channels == 2 and bank.channels == 2 and bank.decim == (12, 2)
    assert rx.wideband_real_bank([3000.0], 6, dtype=dtype).decim == 6
    assert rx._lib.calls["ofdmrx_bank_begin_wideband_real"][3:] == (6, 1, fmt)
    bank.push(np.arange(10))                                         # (converted to the bank's dtype)
    a = rx._lib.calls["ofdmrx_bank_push_wideband"]
    assert a[1] is not None and a[2] == 10 and a[3] == 0
    bank.push(np.zeros(0, dtype), end=True)
    a = rx._lib.calls["ofdmrx_bank_push_wideband"]
    assert a[1] is None and a[2] == 0 and a[3] == 1
    for bad in (np.zeros((10, 2), dtype), np.zeros((10, 1), dtype), np.zeros((), dtype)):
        with pytest.raises(M.OfdmRxError):
            bank.push(bad)
    with pytest.raises(KeyError):
        rx.wideband_real_bank([3000.0], 6, dtype=np.int32)
