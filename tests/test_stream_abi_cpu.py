"""CPU-side checks of the stream decode entries (revision 1.7): exported, and argument errors are reported before any device is
touched."""
import ctypes as C

import numpy as np
import pytest

E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    import modem_amd
    modem_amd.build()
    return modem_amd.load_library()


def test_stream_symbols_exported(lib):
    import modem_amd.ofdmrx as M
    for name in ("ofdmrx_decode_stream", "ofdmrx_decode_stream_device", "ofdmrx_debug_stream_edges"):
        assert name in M.EXPORTS
        getattr(lib, name)
    assert lib.ofdmrx_abi_minor() == 9


@pytest.mark.parametrize("entry", ["ofdmrx_decode_stream", "ofdmrx_decode_stream_device"])
def test_stream_bad_arguments(lib, entry):
    f = getattr(lib, entry)
    pcm = np.zeros((1000, 2), np.int16)
    out = np.zeros((4, 5380), np.uint8)
    res = np.zeros(4 * 48, np.uint8)
    npre = C.c_size_t(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    assert f(None, p(pcm), 0, 2, 1000, 4, p(out), p(res), C.byref(npre)) == E_ARG            # NULL handle
    fake = C.c_void_p(1)                                                                     # never dereferenced: the checks come first
    assert f(fake, None, 0, 2, 1000, 4, p(out), p(res), C.byref(npre)) == E_ARG             # NULL samples
    assert f(fake, p(pcm), 0, 2, 0, 4, p(out), p(res), C.byref(npre)) == E_ARG              # n_samples = 0
    assert f(fake, p(pcm), 0, 2, 0x7fffffff, 4, p(out), p(res), C.byref(npre)) == E_ARG     # too long
    assert f(fake, p(pcm), 3, 2, 1000, 4, p(out), p(res), C.byref(npre)) == E_ARG           # bad format
    assert f(fake, p(pcm), 0, 3, 1000, 4, p(out), p(res), C.byref(npre)) == E_ARG           # bad channel count
    assert f(fake, p(pcm), 0, 2, 1000, 4, None, p(res), C.byref(npre)) == E_ARG             # NULL payload with room for records
    assert f(fake, p(pcm), 0, 2, 1000, 4, p(out), None, C.byref(npre)) == E_ARG             # NULL results
    assert f(fake, p(pcm), 0, 2, 1000, 4, p(out), p(res), None) == E_ARG                    # NULL count
    assert f(fake, C.c_void_p(pcm.ctypes.data + 2), 0, 2, 999, 4, p(out), p(res), C.byref(npre)) == E_ARG   # not on an I/Q pair


def test_stream_edges_bad_arguments(lib):
    f = lib.ofdmrx_debug_stream_edges
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    t = np.zeros(100, np.float32)
    n = C.c_size_t(0)
    p = t.ctypes.data_as(C.c_void_p)
    assert f(None, p, 100, 0, None, None, None, C.byref(n)) == E_ARG
    assert f(C.c_void_p(1), None, 100, 0, None, None, None, C.byref(n)) == E_ARG
    assert f(C.c_void_p(1), p, 0, 0, None, None, None, C.byref(n)) == E_ARG
    assert f(C.c_void_p(1), p, 100, 4, None, None, None, C.byref(n)) == E_ARG
