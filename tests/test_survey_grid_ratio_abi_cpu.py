"""The grid survey at a ratio: its ABI without a GPU: the symbols and their place in the header, the Python
mirror, every refusal of ofdmrx_util_survey_grid_ratio that needs no look into the handle - they come before any device call - the
span at a ratio, the unchanged behaviour of a bare int, and what the command lines refuse before they open a device."""
import ctypes as C
import os
import subprocess
import wave
from fractions import Fraction

import numpy as np
import pytest

import survey_grid_ratio_model as SR

E_ARG = -1
NAMES = ("ofdmrx_util_survey_grid_ratio", "ofdmrx_util_find_slots_ratio")


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
    assert len(lib.ofdmrx_util_survey_grid_ratio.argtypes) == 11 and len(lib.ofdmrx_util_find_slots_ratio.argtypes) == 11
    a = lib.ofdmrx_util_survey_grid_ratio.argtypes
    assert a[3] is C.c_longlong and a[8] is C.c_longlong and a[4] is C.c_size_t and a[9] is C.c_size_t and a[5:8] == [C.c_int] * 3
    assert lib.ofdmrx_util_find_slots_ratio.argtypes[1:3] == [C.c_int] * 2 and lib.ofdmrx_util_find_slots_ratio.argtypes[3:7] == [C.c_double] * 4


def test_span_at_a_ratio():
    import modem_amd
    assert modem_amd.survey_grid_span((25, 4), 16, 0, 1) == (0, (15 * 25) // 4 + 1)
    assert modem_amd.survey_grid_span((25, 4), 16, 1, 1) == (0, (31 * 25) // 4 + 1)          # 100 - 150 lies below 0
    assert modem_amd.survey_grid_span((25, 4), 16, 2, 3) == (50, (79 * 25) // 4 - 50 + 1)
    for P, Q, S, r, n in ((6, 1, 8, 0, 1), (25, 4, 1032, 3, 5), (512, 3, 65536, 1 << 20, 7), (45, 16, 24, 7, 2)):
        assert modem_amd.survey_grid_span((P, Q), S, r, n) == SR.span(P, Q, S, r, n)
        assert modem_amd.survey_grid_span(Fraction(P, Q), S, r, n) == SR.span(P, Q, S, r, n)
        assert modem_amd.survey_grid_span((3 * P, 3 * Q), S, r, n) == SR.span(P, Q, S, r, n)
    for bad in (((7, 1), 16, 0, 1), ((3, 2), 16, 0, 1), ((1024, 1), 16, 0, 1), ((25, 4), 12, 0, 1), ((25, 4), 0, 0, 1), ((25, 4), 65544, 0, 1),
                ((25, 4), 16, -1, 1), ((25, 4), 16, 0, 0)):
        with pytest.raises(modem_amd.OfdmRxError):
            modem_amd.survey_grid_span(*bad)


def test_a_bare_int_keeps_its_values():
    import modem_amd
    assert modem_amd.survey_grid_span(8, 16, 2, 3) == (64, (5 * 16 - 1) * 8 - 64 + 1)
    assert modem_amd.survey_grid_span(512, 4096, 5, 2) == ((5 * 4096 - 24) * 512, (2 * 4096 + 23) * 512 + 1)
    for bad in ((6, 16, 0, 1), (3, 16, 0, 1), (1024, 16, 0, 1)):                       # an int is a power of two, as before
        with pytest.raises(modem_amd.OfdmRxError):
            modem_amd.survey_grid_span(*bad)
    row = np.ones(16, np.float32)
    row[5] = 100.0
    got = modem_amd.find_slots(row, 8, 8000)
    assert [(s["slot"], s["centre_hz"]) for s in got] == [(-3, -12000.0)]
    with pytest.raises(modem_amd.OfdmRxError):
        modem_amd.find_slots(np.ones(12, np.float32), 6, 8000)


def test_survey_grid_ratio_bad_arguments(lib):
    fake = C.c_void_p(1)
    din, dout = C.c_void_p(1 << 20), C.c_void_p(1 << 24)
    # 25/4, S = 64, rows 0 and 1: positions 0 .. (127 x 25) div 4 = 793
    def call(h=fake, d_in=din, fmt=0, in_first=0, n_in=794, p=25, q=4, S=64, row_first=0, n_rows=2, d_out=dout):
        return lib.ofdmrx_util_survey_grid_ratio(h, d_in, fmt, in_first, n_in, p, q, S, row_first, n_rows, d_out)

    assert call(h=None) == E_ARG and call(d_in=None) == E_ARG and call(d_out=None) == E_ARG
    assert call(n_in=0) == E_ARG and call(n_rows=0) == E_ARG
    for bad in ((0, 1), (25, 0), (-25, 4), (25, -4), (7, 1), (3, 2), (25, 13), (17, 16), (513, 1), (1024, 1), (600, 1), (77, 4), (1, 1)):
        assert call(p=bad[0], q=bad[1]) == E_ARG, bad
    for bad in (-8, 0, 4, 12, 63, 65, 65544, 1 << 20):
        assert call(S=bad) == E_ARG, bad
    assert call(fmt=-1) == E_ARG and call(fmt=3) == E_ARG
    assert call(in_first=-1) == E_ARG and call(row_first=-1) == E_ARG
    assert call(in_first=(1 << 50) + 1) == E_ARG and call(row_first=(1 << 50) + 1) == E_ARG
    assert call(n_in=793) == E_ARG                                    # the last time's own position is missing
    assert call(in_first=1, n_in=793) == E_ARG                        # rows from 0 need position 0
    f1 = (64 * 25) // 4 - 150                                         # row 1 starts its history at 250
    assert SR.span(25, 4, 64, 1, 1) == (f1, 794 - f1)
    assert call(row_first=1, n_rows=1, in_first=f1 + 1, n_in=794) == E_ARG    # one position of history missing
    assert call(row_first=1, n_rows=2) == E_ARG                       # row 2 ends at position 1193
    assert call(d_out=C.c_void_p((1 << 20) + 8)) == E_ARG             # the output overlaps the input
    assert call(d_in=C.c_void_p((1 << 20) + 2)) == E_ARG and call(d_out=C.c_void_p((1 << 24) + 2)) == E_ARG
    # too many partials: n_rows (S / 8) n_all above 2^28 - refused whatever the buffer holds; 500/1 has 1000 slots
    assert call(p=500, q=1, S=65536, n_rows=33, n_in=1 << 49) == E_ARG
    assert call(p=25, q=4, S=65536, n_rows=1 << 40, n_in=1 << 49) == E_ARG
    # a power of two goes to ofdmrx_util_survey_grid and meets its refusals
    assert call(p=16, q=1, n_in=2032) == E_ARG and call(p=32, q=2, S=12, n_in=2033) == E_ARG and call(p=16, q=1, h=None, n_in=2033) == E_ARG


def _wav(path, frames, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.zeros((frames, 2), np.int16).tobytes())
    return str(path)


def test_command_lines_refuse_before_a_device(lib, tmp_path):
    """the old spellings stay refused with "not built" and name the new form; the new forms refuse a bare integer, a ratio outside
    the set, a bad floor, a rate that is not rate P / Q of a supported rate, a file shorter than a row's first check, and `auto` from
    standard input - all with status 1, before a device is opened, and nothing is written"""
    import modem_amd.ofdmrx as M
    survey, dec = os.path.join(M.HERE, "bin", "survey"), os.path.join(M.HERE, "bin", "decode_stream")
    w50 = _wav(tmp_path / "w50.wav", 64, 50000)
    w44 = _wav(tmp_path / "w44.wav", 64, 44100)
    out = str(tmp_path / "o")

    def run(*args):
        r = subprocess.run(list(args), capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=60)
        return r.returncode, r.stderr

    code, err = run(survey, "--grid", w50, "25/4")
    assert code == 1 and "not built" in err and "--grid-ratio" in err
    code, err = run(dec, "--grid", "25/4", "auto", out, w50)
    assert code == 1 and "not built" in err and "--grid-ratio" in err and not os.path.exists(out)
    for args in ((survey, "--grid-ratio", w50, "6"), (survey, "--grid-ratio", w50, "7/1"), (survey, "--grid-ratio", w50, "3/2"),
                 (survey, "--grid-ratio", w50, "25/4", "x"), (survey, "--grid-ratio", w44, "25/4"), (survey, "--grid-ratio", str(tmp_path / "none.wav"), "25/4"),
                 (dec, "--grid-ratio", "6", "auto", out, w50), (dec, "--grid-ratio", "7/1", "auto", out, w50), (dec, "--grid-ratio", "25/4", "auto:x", out, w50),
                 (dec, "--grid-ratio", "25/4", "auto", out, w44), (dec, "--grid-ratio", "25/4", "7", out, w50), (dec, "--grid-ratio", "25/4", "1,x", out, w50),
                 (dec, "--grid-ratio", "6", "all", out, w50)):
        code, err = run(*args)
        assert code == 1 and err, args
        assert not os.path.exists(out), args
    code, err = run(dec, "--grid-ratio", "25/4", "auto", out, "-")
    assert code == 1 and "standard input" in err and not os.path.exists(out)
    code, err = run(survey)
    assert code == 1 and "--grid-ratio WIDE.wav P/Q [FLOOR_DB]" in err
    code, err = run(dec)
    assert code == 1 and "--grid-ratio P/Q K1,K2,...|all|auto[:FLOOR_DB]" in err
