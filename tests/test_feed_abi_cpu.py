"""CPU-side checks of the live feed entries (added within revision 1.7): exported, and argument errors are reported before any
device is touched."""
import ctypes as C

import numpy as np
import pytest

E_ARG = -1
NAMES = ("ofdmrx_feed_begin", "ofdmrx_feed_push", "ofdmrx_feed_end", "ofdmrx_feed_lag", "ofdmrx_feed_resident_samples")


@pytest.fixture(scope="module")
def lib():
    import modem_amd
    modem_amd.build()
    return modem_amd.load_library()


def test_feed_symbols_exported(lib):
    import modem_amd.ofdmrx as M
    for name in NAMES:
        assert name in M.EXPORTS
        getattr(lib, name)
    assert lib.ofdmrx_abi_minor() == 9                                                       # additions within 1.7: detected by symbol


def test_feed_header_declares_them():
    import os
    import modem_amd.ofdmrx as M
    text = open(os.path.join(os.path.dirname(M.HERE), "include", "ofdmrx.h")).read()
    for name in NAMES:
        assert name + "(" in text


def test_feed_bad_arguments(lib):
    begin, push, end = lib.ofdmrx_feed_begin, lib.ofdmrx_feed_push, lib.ofdmrx_feed_end
    pcm = np.zeros((1000, 2), np.int16)
    out = np.zeros((4, 5380), np.uint8)
    res = np.zeros(4 * 48, np.uint8)
    nrec, nleft = C.c_size_t(0), C.c_size_t(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(1)                                                                     # never dereferenced: the checks come first
    assert begin(None, 0, 2) == E_ARG                                                        # NULL handle
    assert begin(fake, 3, 2) == E_ARG and begin(fake, -1, 2) == E_ARG                        # bad format
    assert begin(fake, 0, 0) == E_ARG and begin(fake, 0, 3) == E_ARG                         # bad channel count
    assert push(None, p(pcm), 1000, 4, p(out), p(res), C.byref(nrec), C.byref(nleft)) == E_ARG
    assert push(fake, None, 1000, 4, p(out), p(res), C.byref(nrec), C.byref(nleft)) == E_ARG   # NULL samples with n_samples > 0
    assert push(fake, p(pcm), 1000, 4, None, p(res), C.byref(nrec), C.byref(nleft)) == E_ARG   # NULL payload with room for records
    assert push(fake, p(pcm), 1000, 4, p(out), None, C.byref(nrec), C.byref(nleft)) == E_ARG   # NULL results
    assert push(fake, p(pcm), 1000, 4, p(out), p(res), None, C.byref(nleft)) == E_ARG          # NULL n_records
    assert push(fake, p(pcm), 1000, 4, p(out), p(res), C.byref(nrec), None) == E_ARG           # NULL n_left
    assert end(None, 4, p(out), p(res), C.byref(nrec), C.byref(nleft)) == E_ARG
    assert end(fake, 4, None, p(res), C.byref(nrec), C.byref(nleft)) == E_ARG
    assert end(fake, 4, p(out), None, C.byref(nrec), C.byref(nleft)) == E_ARG
    assert end(fake, 4, p(out), p(res), None, C.byref(nleft)) == E_ARG
    assert end(fake, 4, p(out), p(res), C.byref(nrec), None) == E_ARG
    assert lib.ofdmrx_feed_lag(None) == E_ARG and lib.ofdmrx_feed_resident_samples(None) == E_ARG
