"""CPU-side checks of ofdmrx_bank_* (added within revision 1.7): exported, declared, named in the header's revision comment, and every
argument error that needs no look into the handle is reported before any device call."""
import ctypes as C
import os

import numpy as np
import pytest

E_ARG = -1
NAMES = ("ofdmrx_bank_begin", "ofdmrx_bank_push", "ofdmrx_bank_end", "ofdmrx_bank_resident_samples", "ofdmrx_bank_preambles",
         "ofdmrx_bank_last_stage_ops")


@pytest.fixture(scope="module")
def lib():
    import modem_amd
    modem_amd.build()
    return modem_amd.load_library()


def test_bank_symbols_exported(lib):
    import modem_amd.ofdmrx as M
    for name in NAMES:
        assert name in M.EXPORTS
        getattr(lib, name)
    assert lib.ofdmrx_abi_minor() == 9                           # additions within 1.7: detected by symbol
    assert hasattr(M.Receiver, "bank") and hasattr(M, "Bank")


def test_bank_header_declares_them():
    import modem_amd.ofdmrx as M
    text = open(os.path.join(os.path.dirname(M.HERE), "include", "ofdmrx.h")).read()
    head = text.split("#define OFDMRX_ABI_MINOR")[0]
    for name in NAMES:
        assert name + "(" in text
        assert name in head                                      # named in the "added within 1.7" comment


def test_bank_bad_arguments(lib):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(1)                                         # never dereferenced: these checks come first
    begin = lib.ofdmrx_bank_begin
    assert begin(None, 4, 0, 2) == E_ARG                         # NULL handle
    assert begin(fake, 0, 0, 2) == E_ARG and begin(fake, 65536, 0, 2) == E_ARG   # n_channels outside 1 .. 65535
    assert begin(fake, 4, 3, 2) == E_ARG and begin(fake, 4, -1, 2) == E_ARG      # bad format
    assert begin(fake, 4, 0, 0) == E_ARG and begin(fake, 4, 0, 3) == E_ARG       # bad channel count
    pcm = np.zeros((2, 1000, 2), np.int16)
    lens = np.array([1000, 700], np.uintp)
    out, res = np.zeros((8, 5380), np.uint8), np.zeros(8 * 56, np.uint8)
    rc, ri = np.zeros(8, np.int32), np.zeros(8, np.int64)
    nrec, nleft = np.zeros(1, np.uintp), np.zeros(1, np.uintp)

    def push(h=fake, smp=pcm, st=4000, ln=lens, cap=8, o=out, r=res, c=rc, i=ri, a=nrec, b=nleft):
        return lib.ofdmrx_bank_push(h, p(smp), st, p(ln), None, cap, p(o), p(r), p(c), p(i), a.ctypes.data_as(C.POINTER(C.c_size_t)) if a is not None else None,
                                    b.ctypes.data_as(C.POINTER(C.c_size_t)) if b is not None else None)

    def end(h=fake, cap=8, o=out, r=res, c=rc, i=ri, a=nrec, b=nleft):
        return lib.ofdmrx_bank_end(h, cap, p(o), p(r), p(c), p(i), a.ctypes.data_as(C.POINTER(C.c_size_t)) if a is not None else None,
                                   b.ctypes.data_as(C.POINTER(C.c_size_t)) if b is not None else None)

    assert push(h=None) == E_ARG and end(h=None) == E_ARG        # NULL handle
    assert push(ln=None) == E_ARG                                # NULL lengths
    assert push(a=None) == E_ARG and push(b=None) == E_ARG       # NULL counts
    assert end(a=None) == E_ARG and end(b=None) == E_ARG
    for k in "oric":                                             # NULL outputs (any of the four arrays) with max_records > 0
        assert push(**{k: None}) == E_ARG and end(**{k: None}) == E_ARG
    assert lib.ofdmrx_bank_resident_samples(None, 0) == E_ARG
    assert lib.ofdmrx_bank_preambles(None, 0) == E_ARG
    assert lib.ofdmrx_bank_last_stage_ops(None) == E_ARG
