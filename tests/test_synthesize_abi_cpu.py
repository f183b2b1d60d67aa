"""CPU-side checks of ofdmrx_util_synthesize (added within revision 1.9, detected by symbol): exported, declared, named in the
header's revision comment, mirrored by ctypes, refused without a handle; what needs no look into the handle is refused first."""
import ctypes as C
import os

import numpy as np
import pytest

E_ARG, E_NODEV = -1, -4
NAME = "ofdmrx_util_synthesize"


@pytest.fixture(scope="module")
def lib():
    import modem_amd
    modem_amd.build()
    return modem_amd.load_library()


def test_symbol_exported_and_minor_unchanged(lib):
    import modem_amd.ofdmrx as M
    assert NAME in M.EXPORTS
    getattr(lib, NAME)
    assert lib.ofdmrx_abi_minor() == 9                               # an addition within 1.9: detected by symbol
    assert hasattr(M.Receiver, "synthesize")
    text = open(os.path.join(os.path.dirname(M.HERE), "include", "ofdmrx.h")).read()
    assert NAME + "(" in text and NAME in text.split("#define OFDMRX_ABI_MINOR")[0]
    assert os.path.exists(os.path.join(M.HERE, "bin", "synthesize"))


def test_ctypes_signature_matches_the_header(lib):
    """handle, d_in, in_format, in_stride, n_in, interp, centre_hz, start, gain, n_channels, out_first, n_out, d_out, out_format"""
    import modem_amd.ofdmrx as M
    text = open(os.path.join(os.path.dirname(M.HERE), "include", "ofdmrx.h")).read()
    decl = text.split("int " + NAME + "(")[1].split(");")[0]
    kinds = []
    for arg in decl.split(","):
        arg = " ".join(arg.split())
        kinds.append(C.c_void_p if "*" in arg else {"int": C.c_int, "size_t": C.c_size_t, "long long": C.c_longlong}[arg.rsplit(" ", 1)[0]])
    assert len(kinds) == 14 and list(lib.ofdmrx_util_synthesize.argtypes) == kinds


def test_without_a_handle_is_an_argument_error(lib):
    f, s, g = np.array([1000.0]), np.array([0], np.int64), np.array([1.0], np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.ofdmrx_util_synthesize(None, C.c_void_p(1 << 20), 0, 100, 100, 6, p(f), p(s), p(g), 1, 0, 1000, C.c_void_p(1 << 24), 0) == E_ARG
    assert lib.ofdmrx_util_synthesize(None, None, 0, 0, 0, 0, None, None, None, 0, 0, 0, None, 0) == E_ARG


def test_bad_arguments_are_refused_before_the_handle_is_touched(lib):
    fake = C.c_void_p(1)
    f, s, g = np.array([1000.0, -2000.0]), np.array([0, 7], np.int64), np.array([1.0, 0.5], np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    din, dout = C.c_void_p(1 << 20), C.c_void_p(1 << 24)

    def call(d_in=din, ifmt=0, stride=100, n_in=100, interp=6, cf=f, st=s, gn=g, n_ch=2, out_first=0, n_out=1000, d_out=dout, ofmt=0):
        return lib.ofdmrx_util_synthesize(fake, d_in, ifmt, stride, n_in, interp, p(cf), p(st), p(gn), n_ch, out_first, n_out, d_out, ofmt)

    assert call(d_in=None) == E_ARG and call(d_out=None) == E_ARG
    assert call(cf=None) == E_ARG and call(st=None) == E_ARG and call(gn=None) == E_ARG
    assert call(n_in=0, stride=0) == E_ARG and call(n_out=0) == E_ARG
    assert call(n_ch=0) == E_ARG and call(n_ch=65536) == E_ARG
    assert call(interp=1) == E_ARG and call(interp=33) == E_ARG
    assert call(ifmt=1) == E_ARG and call(ifmt=3) == E_ARG and call(ifmt=-1) == E_ARG     # U8 is no input format here
    assert call(ofmt=1) == E_ARG and call(ofmt=3) == E_ARG
    assert call(stride=99) == E_ARG
    assert call(out_first=-1) == E_ARG and call(out_first=(1 << 50) + 1) == E_ARG
    assert call(n_out=(1 << 50) + 1) == E_ARG and call(n_in=(1 << 50) + 1, stride=(1 << 50) + 1) == E_ARG
    assert call(d_out=C.c_void_p((1 << 20) + 8)) == E_ARG             # the output overlaps the input
    assert call(d_in=C.c_void_p((1 << 20) + 2)) == E_ARG and call(d_out=C.c_void_p((1 << 24) + 2)) == E_ARG
    assert call(ifmt=2, d_in=C.c_void_p((1 << 20) + 4)) == E_ARG and call(ofmt=2, d_out=C.c_void_p((1 << 24) + 4)) == E_ARG


def test_create_reports_no_device_where_there_is_none(lib):
    """without a GPU the handle cannot be made: there is no CPU path behind the entry (with one, it is made)"""
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
