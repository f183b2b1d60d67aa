"""The grid survey's ABI without a GPU: the symbols and their place in the header, the Python mirror, and
every refusal of ofdmrx_util_survey_grid that needs no look into the handle - they come before any device call."""
import ctypes as C
import os

import numpy as np
import pytest

import survey_grid_model as SG

E_ARG = -1
NAMES = ("ofdmrx_util_survey_grid", "ofdmrx_util_find_slots")


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
    assert "typedef struct ofdmrx_slot" in text
    assert lib.ofdmrx_abi_minor() == 9                               # additions within 1.9: detected by symbol
    assert len(lib.ofdmrx_util_survey_grid.argtypes) == 10 and len(lib.ofdmrx_util_find_slots.argtypes) == 10
    assert lib.ofdmrx_util_survey_grid.argtypes[3] is C.c_longlong and lib.ofdmrx_util_survey_grid.argtypes[7] is C.c_longlong
    assert lib.ofdmrx_util_find_slots.argtypes[2:6] == [C.c_double] * 4
    assert [n for n, _ in M.Slot._fields_] == ["slot", "centre_hz", "power", "level_db"] and C.sizeof(M.Slot) == 32
    assert hasattr(M.Receiver, "survey_grid") and callable(modem_amd.find_slots) and callable(modem_amd.survey_grid_span)
    assert "find_slots" in modem_amd.__all__ and "survey_grid_span" in modem_amd.__all__


def test_span():
    import modem_amd
    assert modem_amd.survey_grid_span(8, 16, 0, 1) == (0, 15 * 8 + 1)
    assert modem_amd.survey_grid_span(8, 16, 1, 1) == (0, 31 * 8 + 1)                # (16 - 24) D lies below 0
    assert modem_amd.survey_grid_span(8, 16, 2, 3) == (64, (5 * 16 - 1) * 8 - 64 + 1)
    assert modem_amd.survey_grid_span(512, 4096, 5, 2) == ((5 * 4096 - 24) * 512, (2 * 4096 + 23) * 512 + 1)
    for D, S, r, n in ((2, 8, 0, 1), (64, 1032, 3, 5), (512, 65536, 1 << 20, 7)):
        assert modem_amd.survey_grid_span(D, S, r, n) == SG.span(D, S, r, n)
    for bad in ((3, 16, 0, 1), (1024, 16, 0, 1), (8, 12, 0, 1), (8, 0, 0, 1), (8, 65544, 0, 1), (8, 16, -1, 1), (8, 16, 0, 0)):
        with pytest.raises(modem_amd.OfdmRxError):
            modem_amd.survey_grid_span(*bad)


def test_survey_grid_bad_arguments(lib):
    fake = C.c_void_p(1)
    din, dout = C.c_void_p(1 << 20), C.c_void_p(1 << 24)
    # D = 16, S = 64, rows 0 and 1: positions 0 .. 127 x 16 = 2032
    def call(h=fake, d_in=din, fmt=0, in_first=0, n_in=2033, decim=16, S=64, row_first=0, n_rows=2, d_out=dout):
        return lib.ofdmrx_util_survey_grid(h, d_in, fmt, in_first, n_in, decim, S, row_first, n_rows, d_out)

    assert call(h=None) == E_ARG and call(d_in=None) == E_ARG and call(d_out=None) == E_ARG
    assert call(n_in=0) == E_ARG and call(n_rows=0) == E_ARG
    for bad in (-16, 0, 1, 3, 12, 24, 33, 1024):
        assert call(decim=bad) == E_ARG, bad
    for bad in (-8, 0, 4, 12, 63, 65, 65544, 1 << 20):
        assert call(S=bad) == E_ARG, bad
    assert call(fmt=-1) == E_ARG and call(fmt=3) == E_ARG
    assert call(in_first=-1) == E_ARG and call(row_first=-1) == E_ARG
    assert call(in_first=(1 << 50) + 1) == E_ARG and call(row_first=(1 << 50) + 1) == E_ARG
    assert call(n_in=2032) == E_ARG                                   # the last time's own position is missing
    assert call(in_first=1, n_in=2032) == E_ARG                       # rows from 0 need position 0
    assert call(row_first=1, n_rows=1, in_first=(64 - 24) * 16 + 1, n_in=2033) == E_ARG       # one position of history missing
    assert call(row_first=1, n_rows=2) == E_ARG                       # row 2 ends at position 3056
    assert call(d_out=C.c_void_p((1 << 20) + 8)) == E_ARG             # the output overlaps the input
    assert call(d_in=C.c_void_p((1 << 20) + 2)) == E_ARG and call(d_out=C.c_void_p((1 << 24) + 2)) == E_ARG
    # too many partials: n_rows (S / 8) M above 2^28 - refused whatever the buffer holds
    assert call(decim=512, S=65536, n_rows=33, n_in=1 << 49) == E_ARG
    assert call(decim=512, S=65536, n_rows=1 << 40, n_in=1 << 49) == E_ARG
