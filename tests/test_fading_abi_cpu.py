"""CPU-side checks of ofdmrx_util_fading (added within revision 1.9, detected by symbol): exported, declared, named in the header's
revision comment, refused without a handle, and the F.520 presets of modem_amd.watterson."""
import ctypes as C
import math
import os

import pytest

E_ARG = -1
NAME = "ofdmrx_util_fading"


@pytest.fixture(scope="module")
def lib():
    import modem_amd
    modem_amd.build()
    return modem_amd.load_library()


def _header():
    import modem_amd.ofdmrx as M
    return open(os.path.join(os.path.dirname(M.HERE), "include", "ofdmrx.h")).read()


def test_fading_symbol_exported_and_minor_unchanged(lib):
    import modem_amd.ofdmrx as M
    assert NAME in M.EXPORTS
    getattr(lib, NAME)
    assert lib.ofdmrx_abi_minor() == 9                               # an addition within 1.9: detected by symbol
    assert hasattr(M.Receiver, "fading")


def test_fading_header_declares_it_and_its_constants():
    import modem_amd.ofdmrx as M
    text = _header()
    assert NAME + "(" in text and "} ofdmrx_fading;" in text
    assert NAME in text.split("#define OFDMRX_ABI_MINOR")[0]         # named in the revision comment above the minor
    for name, value in (("OFDMRX_FADING_SINES", 16), ("OFDMRX_FADING_KNOT", 32), ("OFDMRX_FADING_MAX_DELAY", 1024)):
        assert "#define %s %d" % (name, value) in text
    assert (M.FADING_SINES, M.FADING_KNOT, M.FADING_MAX_DELAY) == (16, 32, 1024)
    assert C.sizeof(M.Fading) == 4 + 4 * 8 + 3 * 4 * 8


def test_fading_without_a_handle_is_an_argument_error(lib):
    import modem_amd.ofdmrx as M
    fd = M.Fading()
    fd.ntaps = 1
    fd.gains_re[0] = 1.0
    assert lib.ofdmrx_util_fading(None, C.c_void_p(4096), 1, C.c_void_p(1 << 20), 1, 64, C.byref(fd), 1, 0) == E_ARG
    assert lib.ofdmrx_util_fading(None, None, 1, None, 1, 64, None, 1, 0) == E_ARG


def test_watterson_presets():
    import modem_amd
    r = math.sqrt(0.5)
    for rate, want in ((8000, dict(good=4, moderate=8, poor=16)), (48000, dict(good=24, moderate=48, poor=96))):
        for preset, spread in (("good", 0.1), ("moderate", 0.5), ("poor", 1.0)):
            paths = modem_amd.watterson(preset, rate)
            assert [p[0] for p in paths] == [0, want[preset]]
            assert all(abs(complex(p[1]) - r) < 1e-15 and p[2] == spread for p in paths)
    assert [p[0] for p in modem_amd.watterson("good", 44100)] == [0, 22]       # round(22.05)
    with pytest.raises(ValueError):
        modem_amd.watterson("awful", 8000)
