"""CPU-side checks of ofdmrx_decode_streams* and ofdmrx_debug_streams_edges (added within revision 1.7): exported, declared, and
every argument error is reported before any device call."""
import ctypes as C
import os

import numpy as np
import pytest

E_ARG = -1
NAMES = ("ofdmrx_decode_streams", "ofdmrx_decode_streams_device", "ofdmrx_debug_streams_edges")


@pytest.fixture(scope="module")
def lib():
    import modem_amd
    modem_amd.build()
    return modem_amd.load_library()


def test_streams_symbols_exported(lib):
    import modem_amd.ofdmrx as M
    for name in NAMES:
        assert name in M.EXPORTS
        getattr(lib, name)
    assert lib.ofdmrx_abi_minor() == 9                           # additions within 1.7: detected by symbol


def test_streams_header_declares_them():
    import modem_amd.ofdmrx as M
    text = open(os.path.join(os.path.dirname(M.HERE), "include", "ofdmrx.h")).read()
    for name in NAMES:
        assert name + "(" in text
    assert "ofdmrx_decode_streams" in text.split("#define OFDMRX_ABI_MINOR")[0]   # named in the "added within 1.7" comment


@pytest.mark.parametrize("entry", NAMES[:2])
def test_streams_bad_arguments(lib, entry):
    f = getattr(lib, entry)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(1)                                         # never dereferenced: the checks come first
    S, stride = 3, 1000 * 4
    pcm = np.zeros((S, 1000, 2), np.int16)
    lens = np.array([1000, 0, 700], np.uintp)
    out, res = np.zeros((8, 5380), np.uint8), np.zeros(8 * 56, np.uint8)
    npre, first = np.zeros(S, np.uintp), np.zeros(S + 1, np.uintp)

    def call(h=fake, smp=pcm, fmt=0, ch=2, n=S, st=stride, ln=lens, per=4, cap=8, o=out, r=res, a=npre, b=first):
        q = lambda x: None if x is None else p(x)
        return f(h, q(smp), fmt, ch, n, st, q(ln), per, cap, q(o), q(r), q(a), q(b))

    assert call(h=None) == E_ARG                                 # NULL handle
    assert call(smp=None) == E_ARG and call(ln=None) == E_ARG    # NULL samples, lengths
    assert call(a=None) == E_ARG and call(b=None) == E_ARG       # NULL counts, offsets
    assert call(n=0) == E_ARG and call(n=65536) == E_ARG         # n_streams outside 1 .. 65535
    big = lens.copy()
    big[1] = 0x7fffffff // 2 + 1
    assert call(ln=big, st=1 << 40) == E_ARG                     # a length above 0x7fffffff / 2
    assert call(st=stride + 2) == E_ARG                          # a stride off the sample-frame boundary
    assert call(st=999 * 4) == E_ARG                             # ... smaller than the longest recording
    assert call(st=0) == E_ARG
    assert call(fmt=3) == E_ARG and call(fmt=-1) == E_ARG        # bad format
    assert call(ch=0) == E_ARG and call(ch=3) == E_ARG           # bad channel count
    assert call(o=None) == E_ARG and call(r=None) == E_ARG       # NULL outputs with max_records > 0
    odd = np.zeros(4 * 1000 * S + 4, np.uint8)[2:]               # samples off the sample-frame boundary
    assert f(fake, C.c_void_p(odd.ctypes.data), 0, 2, S, stride, p(lens), 4, 8, p(out), p(res), p(npre), p(first)) == E_ARG


def test_streams_edges_bad_arguments(lib):
    f = lib.ofdmrx_debug_streams_edges
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(1)
    t = np.zeros(100, np.float32)
    n = np.array([60, 40], np.uintp)
    te, tm, im, ne = np.zeros((2, 4), np.int64), np.zeros((2, 4), np.int64), np.zeros((2, 4), np.int32), np.zeros(2, np.uintp)
    assert f(None, p(t), 2, p(n), 4, p(te), p(tm), p(im), p(ne)) == E_ARG
    assert f(fake, None, 2, p(n), 4, p(te), p(tm), p(im), p(ne)) == E_ARG
    assert f(fake, p(t), 2, None, 4, p(te), p(tm), p(im), p(ne)) == E_ARG
    assert f(fake, p(t), 2, p(n), 4, p(te), p(tm), p(im), None) == E_ARG
    assert f(fake, p(t), 0, p(n), 4, p(te), p(tm), p(im), p(ne)) == E_ARG
    assert f(fake, p(t), 65536, p(n), 4, p(te), p(tm), p(im), p(ne)) == E_ARG
    assert f(fake, p(t), 2, p(n), 4, None, p(tm), p(im), p(ne)) == E_ARG
    assert f(fake, p(t), 2, p(n), 4, p(te), None, p(im), p(ne)) == E_ARG
    assert f(fake, p(t), 2, p(n), 4, p(te), p(tm), None, p(ne)) == E_ARG
    big = np.array([60, 0x7fffffff // 2 + 1], np.uintp)
    assert f(fake, p(t), 2, p(big), 4, p(te), p(tm), p(im), p(ne)) == E_ARG
