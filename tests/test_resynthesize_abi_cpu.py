"""CPU-side checks of ofdmrx_util_synthesize_ratio (added within revision 1.9, detected by symbol): exported, declared, named in the
header's revision comment, mirrored by ctypes, refused without a handle; what needs no look into the handle is refused first - the
ratio's limits before everything else; modem_amd.synthesize_support against the model."""
import ctypes as C
import fractions
import os

import numpy as np
import pytest

import resynthesize_model as RS

E_ARG = -1
NAME = "ofdmrx_util_synthesize_ratio"


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
    text = open(os.path.join(os.path.dirname(M.HERE), "include", "ofdmrx.h")).read()
    assert NAME + "(" in text and NAME in text.split("#define OFDMRX_ABI_MINOR")[0]
    assert os.path.exists(os.path.join(M.HERE, "bin", "synthesize"))


def test_ctypes_signature_matches_the_header(lib):
    """handle, d_in, in_format, in_stride, n_in, p, q, centre_hz, start, gain, n_channels, out_first, n_out, d_out, out_format"""
    import modem_amd.ofdmrx as M
    text = open(os.path.join(os.path.dirname(M.HERE), "include", "ofdmrx.h")).read()
    decl = text.split("int " + NAME + "(")[1].split(");")[0]
    kinds = []
    for arg in decl.split(","):
        arg = " ".join(arg.split())
        kinds.append(C.c_void_p if "*" in arg else {"int": C.c_int, "size_t": C.c_size_t, "long long": C.c_longlong}[arg.rsplit(" ", 1)[0]])
    assert len(kinds) == 15 and list(lib.ofdmrx_util_synthesize_ratio.argtypes) == kinds


def test_without_a_handle_is_an_argument_error(lib):
    f, s, g = np.array([1000.0]), np.array([0], np.int64), np.array([1.0], np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for pq in ((25, 4), (50, 8), (12, 2), (6, 1)):                   # (q = 1 forwards to the integer entry, which refuses the same)
        assert lib.ofdmrx_util_synthesize_ratio(None, C.c_void_p(1 << 20), 0, 100, 100, pq[0], pq[1], p(f), p(s), p(g), 1, 0, 1000,
                                                C.c_void_p(1 << 24), 0) == E_ARG
    assert lib.ofdmrx_util_synthesize_ratio(None, None, 0, 0, 0, 0, 0, None, None, None, 0, 0, 0, None, 0) == E_ARG


def test_bad_arguments_are_refused_before_the_handle_is_touched(lib):
    """a fake handle: anything that looked into it would fault"""
    fake = C.c_void_p(1)
    f, s, g = np.array([1000.0, -2000.0]), np.array([0, 7], np.int64), np.array([1.0, 0.5], np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    din, dout = C.c_void_p(1 << 20), C.c_void_p(1 << 24)

    def call(d_in=din, ifmt=0, stride=100, n_in=100, pq=(25, 4), cf=f, st=s, gn=g, n_ch=2, out_first=0, n_out=1000, d_out=dout, ofmt=0):
        return lib.ofdmrx_util_synthesize_ratio(fake, d_in, ifmt, stride, n_in, pq[0], pq[1], p(cf), p(st), p(gn), n_ch, out_first, n_out, d_out, ofmt)

    for pq in ((0, 4), (25, 0), (-25, 4), (25, -4), (-25, -4), (35, 17), (7, 4), (129, 4), (1, 1), (33, 1), (3, 2), (2 ** 31 - 1, 1)):
        assert call(pq=pq) == E_ARG, pq                               # p or q <= 0, a reduced q above 16, p / q outside 2 .. 32
    for pq in ((25, 4), (50, 8), (12, 2)):                           # (50, 8) is accepted wherever (25, 4) is: every refusal is another argument's
        assert call(pq=pq, d_in=None) == E_ARG and call(pq=pq, d_out=None) == E_ARG
        assert call(pq=pq, cf=None) == E_ARG and call(pq=pq, st=None) == E_ARG and call(pq=pq, gn=None) == E_ARG
        assert call(pq=pq, n_in=0, stride=0) == E_ARG and call(pq=pq, n_out=0) == E_ARG
        assert call(pq=pq, n_ch=0) == E_ARG and call(pq=pq, n_ch=65536) == E_ARG
        assert call(pq=pq, ifmt=1) == E_ARG and call(pq=pq, ifmt=3) == E_ARG and call(pq=pq, ifmt=-1) == E_ARG   # U8 is no input format here
        assert call(pq=pq, ofmt=1) == E_ARG and call(pq=pq, ofmt=3) == E_ARG
        assert call(pq=pq, stride=99) == E_ARG
        assert call(pq=pq, out_first=-1) == E_ARG and call(pq=pq, out_first=(1 << 50) + 1) == E_ARG
        assert call(pq=pq, n_out=(1 << 50) + 1) == E_ARG and call(pq=pq, n_out=1024 * (2 ** 31 - 1) + 1) == E_ARG
        assert call(pq=pq, n_in=(1 << 50) + 1, stride=(1 << 50) + 1) == E_ARG
        assert call(pq=pq, d_out=C.c_void_p((1 << 20) + 8)) == E_ARG      # the output overlaps the input
        assert call(pq=pq, d_in=C.c_void_p((1 << 20) + 2)) == E_ARG and call(pq=pq, d_out=C.c_void_p((1 << 24) + 2)) == E_ARG
        assert call(pq=pq, ifmt=2, d_in=C.c_void_p((1 << 20) + 4)) == E_ARG and call(pq=pq, ofmt=2, d_out=C.c_void_p((1 << 24) + 4)) == E_ARG


def test_receiver_takes_a_ratio():
    import inspect
    import modem_amd.ofdmrx as M
    assert hasattr(M.Receiver, "synthesize") and "_ratio(interp)" in inspect.getsource(M.Receiver.synthesize)
    assert M._ratio(fractions.Fraction(50, 8)) == (25, 4) and M._ratio((50, 8)) == (50, 8) and M._ratio(6) == (6, None)


def test_synthesize_support_is_the_models():
    import modem_amd
    for n_in in (1, 2, 119, 120, 95200):
        for P, Q in ((5, 2), (33, 16), (25, 4), (64, 3), (125, 4), (511, 16)):
            want = RS.support(0, n_in, P, Q) + 1
            assert modem_amd.synthesize_support(n_in, (P, Q)) == want == ((n_in - 1 + 24) * P) // Q + 1
            assert modem_amd.synthesize_support(n_in, (2 * P, 2 * Q)) == want
            assert modem_amd.synthesize_support(n_in, fractions.Fraction(P, Q)) == want
        for D in (2, 6, 32):
            assert modem_amd.synthesize_support(n_in, D) == (n_in - 1) * D + 24 * D + 1
            assert modem_amd.synthesize_support(n_in, (2 * D, 2)) == (n_in - 1) * D + 24 * D + 1
    for bad in ((0, 6), (10, 0), (10, (25, 0)), (10, (-25, 4))):
        with pytest.raises(modem_amd.OfdmRxError):
            modem_amd.synthesize_support(*bad)
