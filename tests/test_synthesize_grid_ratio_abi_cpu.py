"""CPU-side checks of ofdmrx_util_synthesize_grid_ratio and ofdmrx_util_synthesize_grid_ratio_chunk (added within revision 1.9,
detected by symbol): exported, declared, named in the header's revision comment, mirrored by ctypes, refused
without a handle; everything that needs no look into the handle is refused first; modem_amd.synthesize_grid_chunk at a ratio; how
Receiver.synthesize_grid reads its interp; the command line's refusals that need no device."""
import ctypes as C
import fractions
import os
import subprocess

import numpy as np
import pytest

import synthesize_grid_ratio_model as R

E_ARG = -1
NAME = "ofdmrx_util_synthesize_grid_ratio"
SCRATCH = 32 << 20


@pytest.fixture(scope="module")
def lib():
    import modem_amd
    modem_amd.build()
    return modem_amd.load_library()


def test_symbols_exported_and_minor_unchanged(lib):
    import modem_amd.ofdmrx as M
    text = open(os.path.join(os.path.dirname(M.HERE), "include", "ofdmrx.h")).read()
    for name in (NAME, NAME + "_chunk"):
        assert name in M.EXPORTS
        getattr(lib, name)
        assert name + "(" in text and name in text.split("#define OFDMRX_ABI_MINOR")[0]
    assert lib.ofdmrx_abi_minor() == 9                               # an addition within 1.9: detected by symbol


def test_ctypes_signature_matches_the_header(lib):
    """handle, d_in, in_format, in_stride, n_in, p, q, slots, start, gain, n_slots, out_first, n_out, d_out, out_format"""
    import modem_amd.ofdmrx as M
    text = open(os.path.join(os.path.dirname(M.HERE), "include", "ofdmrx.h")).read()
    decl = text.split("int " + NAME + "(")[1].split(");")[0]
    kinds = []
    for arg in decl.split(","):
        arg = " ".join(arg.split())
        kinds.append(C.c_void_p if "*" in arg else {"int": C.c_int, "size_t": C.c_size_t, "long long": C.c_longlong}[arg.rsplit(" ", 1)[0]])
    assert len(kinds) == 15 and list(lib.ofdmrx_util_synthesize_grid_ratio.argtypes) == kinds
    assert list(lib.ofdmrx_util_synthesize_grid_ratio_chunk.argtypes) == [C.c_int, C.c_int]
    assert lib.ofdmrx_util_synthesize_grid_ratio_chunk.restype == C.c_longlong


def test_without_a_handle_is_an_argument_error(lib):
    k, s, g = np.array([1], np.int32), np.array([0], np.int64), np.array([1.0], np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for pq in ((25, 4), (50, 8), (6, 1), (8, 1), (300, 1)):            # (8 / 1 is the grid entry's, which refuses the same)
        assert lib.ofdmrx_util_synthesize_grid_ratio(None, C.c_void_p(1 << 20), 0, 100, 100, pq[0], pq[1], p(k), p(s), p(g), 1, 0, 1000,
                                                     C.c_void_p(1 << 24), 0) == E_ARG
    assert lib.ofdmrx_util_synthesize_grid_ratio(None, None, 0, 0, 0, 0, 0, None, None, None, 0, 0, 0, None, 0) == E_ARG


def test_bad_arguments_are_refused_before_the_handle_is_touched(lib):
    """a fake handle: anything that looked into it would fault"""
    fake = C.c_void_p(1)
    k, s, g = np.array([3, -6], np.int32), np.array([0, 50], np.int64), np.array([1.0, 0.5], np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    din, dout = C.c_void_p(1 << 20), C.c_void_p(1 << 24)

    def call(d_in=din, ifmt=0, stride=100, n_in=100, pq=(25, 4), sl=k, st=s, gn=g, n=2, out_first=0, n_out=1000, d_out=dout, ofmt=0):
        return lib.ofdmrx_util_synthesize_grid_ratio(fake, d_in, ifmt, stride, n_in, pq[0], pq[1], p(sl), p(st), p(gn), n, out_first, n_out, d_out, ofmt)

    # p or q <= 0; a reduced q above 16; p below 2 q or above 512; a prime factor other than 2, 3 and 5
    for pq in ((0, 4), (25, 0), (-25, 4), (25, -4), (-25, -4), (512, 17), (7, 4), (3, 2), (1, 1), (513, 1), (1024, 1), (7, 1), (77, 2), (2 ** 31 - 1, 1)):
        assert call(pq=pq) == E_ARG, pq
    for pq in ((25, 4), (50, 8)):                                     # (50, 8) is accepted wherever (25, 4) is: every refusal is another argument's
        assert call(pq=pq, d_in=None) == E_ARG and call(pq=pq, d_out=None) == E_ARG
        assert call(pq=pq, st=None) == E_ARG and call(pq=pq, gn=None) == E_ARG
        assert call(pq=pq, n_in=0, stride=0) == E_ARG and call(pq=pq, n_out=0) == E_ARG
        assert call(pq=pq, n=0) == E_ARG and call(pq=pq, n=14) == E_ARG           # n_all = 13 at 25 / 4
        assert call(pq=pq, sl=None) == E_ARG and call(pq=pq, sl=None, n=12) == E_ARG
        for bad in (7, -7, 3):                                        # outside -6 .. 6 (-25 <= 4 k < 25); given twice
            assert call(pq=pq, sl=np.array([3, bad], np.int32)) == E_ARG, bad
        for bad in (-25, 1, 24, 26, 5):                               # negative; P does not divide it
            assert call(pq=pq, st=np.array([0, bad], np.int64)) == E_ARG, bad
        assert call(pq=pq, st=np.array([0, ((1 << 50) // 25 + 1) * 25], np.int64)) == E_ARG
        for bad in (float("nan"), float("inf"), 3e38):
            assert call(pq=pq, gn=np.array([1.0, bad], np.float32)) == E_ARG, bad
        assert call(pq=pq, ifmt=1) == E_ARG and call(pq=pq, ifmt=3) == E_ARG and call(pq=pq, ifmt=-1) == E_ARG   # U8 is no input format here
        assert call(pq=pq, ofmt=1) == E_ARG and call(pq=pq, ofmt=3) == E_ARG
        assert call(pq=pq, stride=99) == E_ARG
        assert call(pq=pq, out_first=-1) == E_ARG and call(pq=pq, out_first=(1 << 50) + 1) == E_ARG
        assert call(pq=pq, n_out=(1 << 50) + 1) == E_ARG and call(pq=pq, n_out=1024 * (2 ** 31 - 1) + 1) == E_ARG   # the bound: 2^41 - 1024
        assert call(pq=pq, n_in=(1 << 50) + 1, stride=(1 << 50) + 1) == E_ARG
        assert call(pq=pq, d_out=C.c_void_p((1 << 20) + 8)) == E_ARG      # the output overlaps the input
        assert call(pq=pq, d_in=C.c_void_p((1 << 20) + 2)) == E_ARG and call(pq=pq, d_out=C.c_void_p((1 << 24) + 2)) == E_ARG
        assert call(pq=pq, ifmt=2, d_in=C.c_void_p((1 << 20) + 4)) == E_ARG and call(pq=pq, ofmt=2, d_out=C.c_void_p((1 << 24) + 4)) == E_ARG
    # the existing entry keeps its rule: no power of two, no call
    for bad in (3, 6, 25, 300):
        assert lib.ofdmrx_util_synthesize_grid(fake, din, 0, 100, 100, bad, p(k), p(s), p(g), 2, 0, 1000, dout, 0) == E_ARG


def test_chunk_at_a_ratio(lib):
    """the outputs per chunk: a multiple of P whose input times (chunk Q / P of them), 24 more, a transform tile of them - and at
    Q = 1 the 7 a work item of the filter may reach past the last - fit the scratch with M float2 each; the reduction; a power of two at Q = 1 is the grid entry's number; refusals"""
    import modem_amd
    for P, Q in [(3, 1), (5, 2), (6, 1), (15, 2), (25, 4), (45, 16), (75, 2), (243, 1), (500, 1), (512, 3)]:
        n = modem_amd.synthesize_grid_chunk((P, Q))
        assert n == lib.ofdmrx_util_synthesize_grid_ratio_chunk(P, Q) == modem_amd.synthesize_grid_chunk(fractions.Fraction(P, Q))
        assert n == modem_amd.synthesize_grid_chunk((3 * P, 3 * Q)) and n > 0 and n % P == 0
        times = n // P * Q
        per_time = 2 * P * 8
        more = 24 + R.tile(P, Q) + (7 if Q == 1 else 0)
        assert (times + more) * per_time <= SCRATCH < (times + Q + more) * per_time
    for D in (2, 64, 512):
        assert modem_amd.synthesize_grid_chunk((D, 1)) == modem_amd.synthesize_grid_chunk(D) == modem_amd.synthesize_grid_chunk((2 * D, 2))
    for bad in ((7, 1), (3, 2), (513, 1), (25, 0), (0, 4), (-25, 4), (512, 17)):
        assert lib.ofdmrx_util_synthesize_grid_ratio_chunk(*bad) == E_ARG
        with pytest.raises(modem_amd.OfdmRxError):
            modem_amd.synthesize_grid_chunk(bad)
    for bad in (3, 6, 1024):                                          # an int goes where it went
        with pytest.raises(modem_amd.OfdmRxError):
            modem_amd.synthesize_grid_chunk(bad)


class _Lib:
    """records the call Receiver.synthesize_grid makes"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append((name, a))
            return 0
        return f


def test_receiver_parses_its_interp(lib):
    """a pair or a Fraction goes to the ratio entry, reduced, with the ratio's slots; an int goes where it went"""
    import modem_amd
    import modem_amd.ofdmrx as M
    rx = M.Receiver.__new__(M.Receiver)
    rx._lib, rx._h = _Lib(), C.c_void_p(1)
    rx._check = lambda r: None
    s, g = [0, 50], [0.5, 0.25]
    for interp in ((25, 4), (50, 8), fractions.Fraction(25, 4)):
        rx.synthesize_grid(1 << 20, 0, 100, interp, [3, -6], s, g, 7, 1000, 1 << 24, 2)
        name, a = rx._lib.calls[-1]
        assert name == NAME and a[5:7] == (25, 4) and a[10:13] == (2, 7, 1000) and a[3:5] == (100, 100)
    rx.synthesize_grid(1 << 20, 0, 100, (25, 4), None, np.zeros(13, np.int64), np.ones(13, np.float32), 0, 10, 1 << 24, 0)
    assert rx._lib.calls[-1][1][10] == 13                             # slots None: all 13 of them
    rx.synthesize_grid(1 << 20, 0, 100, 8, [3, -8], [0, 8], g, 0, 10, 1 << 24, 0, in_stride=120)
    name, a = rx._lib.calls[-1]
    assert name == "ofdmrx_util_synthesize_grid" and a[5] == 8 and a[3] == 120
    n = len(rx._lib.calls)
    for interp, slots in (((25, 4), [3, 7]), ((25, 4), [3, -7]), ((7, 1), [0, 1]), ((3, 2), [0, 1]), (6, [0, 1]), ((25, 4), [0, 1, 2])):
        with pytest.raises(modem_amd.OfdmRxError):
            rx.synthesize_grid(1 << 20, 0, 100, interp, slots, s, g, 0, 10, 1 << 24, 0)
    assert len(rx._lib.calls) == n


def test_command_line_refusals(lib, tmp_path):
    """synthesize --grid-ratio refuses, with a message and status 1 and before it opens a device: a ratio for which rate P / Q is no
    integer, a START that P does not divide, a slot outside the range or given twice; --grid with a ratio keeps its refusal"""
    import modem_amd.ofdmrx as M
    import wave
    exe = os.path.join(M.HERE, "bin", "synthesize")
    wav = str(tmp_path / "in.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(8000)
        w.writeframes(np.zeros((64, 2), np.int16).tobytes())
    out = str(tmp_path / "out.wav")

    def run(*args):
        r = subprocess.run([exe] + list(args), capture_output=True, text=True)
        return r.returncode, r.stderr

    for args, word in ((("--grid-ratio", out, "25/3", "0:0:0:" + wav), "integer"),
                       (("--grid-ratio", out, "25/4", "0:10:0:" + wav), "START"),
                       (("--grid-ratio", out, "25/4", "7:0:0:" + wav), "slot"),
                       (("--grid-ratio", out, "25/4", "1:0:0:" + wav, "1:25:0:" + wav), "twice"),
                       (("--grid-ratio", out, "7/1", "0:0:0:" + wav), "ratio"),
                       (("--grid", out, "25/4", "0:0:0:" + wav), "not built")):
        code, err = run(*args)
        assert code == 1 and word in err, (args, code, err)
        assert not os.path.exists(out)
