"""ctypes mirror of include/ofdmrx.h (the drop-in boundary for decode.cc's Decoder seam)."""
import ctypes as C
import fractions
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")

FMT_S16, FMT_U8, FMT_F32 = 0, 1, 2
PAYLOAD_BYTES = 5380
CODE_LEN = 65536
FRAME_SAMPLES = 95200
MESG_BYTES = 5476
MESG_BYTES_MAX = 5512   # modes 10-13 (44096 message bits); Receiver.polar(modes=...) returns this many per lane
CONS_MAX = 32400
STATUS_NAMES = ["OK", "NO_SYNC", "OSD_ERROR", "HEADER_CRC", "BAD_MODE", "BAD_CALLSIGN", "PAYLOAD_CRC"]
TAPS = dict(HDR_SOFT=1, CONS_RAW=2, CONS_ROT=3, SLOPE=4, YINT=5, PRECISION=6, LLR=7, METRIC=8, LANE_MESG=9, ANALYTIC=10)
STAGES = ["front", "sync", "header", "demod", "theilsen", "llr", "polar", "finish", "total"]

# every symbol include/ofdmrx.h declares
EXPORTS = [
    "ofdmrx_abi_version", "ofdmrx_abi_minor", "ofdmrx_strerror", "ofdmrx_create", "ofdmrx_destroy", "ofdmrx_decode_batch",
    "ofdmrx_decode_batch_device", "ofdmrx_synchronize", "ofdmrx_get_timing", "ofdmrx_chunk_frames", "ofdmrx_last_chunk_first_frame", "ofdmrx_list_decoded_frames", "ofdmrx_sc_decided_frames", "ofdmrx_get_sc_timing", "ofdmrx_set_esn0_rows", "ofdmrx_set_attempt_log",
    "ofdmrx_debug_dump", "ofdmrx_debug_polar", "ofdmrx_debug_sc_path", "ofdmrx_debug_decode_cons", "ofdmrx_debug_polar_modes",
    "ofdmrx_debug_decode_cons_modes", "ofdmrx_debug_theil_sen", "ofdmrx_debug_osd", "ofdmrx_debug_fft",
    "ofdmrx_util_awgn_tile", "ofdmrx_util_channel", "ofdmrx_frame_samples", "ofdmrx_tx_frame_samples",
    "ofdmrx_tx_encode_device", "ofdmrx_stream_samples", "ofdmrx_tx_encode_stream_device", "ofdmrx_tx_encode_stream",
    "ofdmrx_callsign_value", "ofdmrx_decode_stream", "ofdmrx_decode_stream_device", "ofdmrx_debug_stream_edges",
    "ofdmrx_feed_begin", "ofdmrx_feed_push", "ofdmrx_feed_end", "ofdmrx_feed_lag", "ofdmrx_feed_resident_samples",
    "ofdmrx_decode_streams", "ofdmrx_decode_streams_device", "ofdmrx_debug_streams_edges",
    "ofdmrx_bank_begin", "ofdmrx_bank_push", "ofdmrx_bank_end", "ofdmrx_bank_resident_samples", "ofdmrx_bank_preambles",
    "ofdmrx_bank_last_stage_ops", "ofdmrx_util_fading", "ofdmrx_util_channelize_taps", "ofdmrx_util_channelize",
    "ofdmrx_bank_begin_wideband", "ofdmrx_bank_push_wideband", "ofdmrx_util_synthesize",
    "ofdmrx_util_survey_window", "ofdmrx_util_survey", "ofdmrx_util_find_bands",
    "ofdmrx_util_channelize_ratio_taps", "ofdmrx_util_channelize_ratio", "ofdmrx_bank_begin_wideband_ratio",
    "ofdmrx_util_synthesize_ratio",
    "ofdmrx_util_channelize_grid_taps", "ofdmrx_util_channelize_grid", "ofdmrx_bank_begin_wideband_grid",
    "ofdmrx_util_synthesize_grid", "ofdmrx_util_synthesize_grid_chunk",
    "ofdmrx_util_survey_grid", "ofdmrx_util_find_slots",
    "ofdmrx_util_channelize_grid_ratio_taps", "ofdmrx_util_grid_ratio_slots", "ofdmrx_util_channelize_grid_ratio",
    "ofdmrx_bank_begin_wideband_grid_ratio",
    "ofdmrx_util_synthesize_grid_ratio", "ofdmrx_util_synthesize_grid_ratio_chunk",
    "ofdmrx_util_survey_grid_ratio", "ofdmrx_util_find_slots_ratio",
    "ofdmrx_util_channelize_real", "ofdmrx_bank_begin_wideband_real",
]


class OfdmRxError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("sample_rate", C.c_int32), ("list_size", C.c_int32),
                ("device", C.c_int32), ("chunk_frames", C.c_int32), ("max_samples", C.c_int32),
                ("descramble", C.c_int32), ("flags", C.c_int32), ("stream", C.c_void_p)]


class FrameResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("symbol_pos", C.c_int32), ("sc_start", C.c_int64),
                ("cfo_rad", C.c_float), ("cfo_fine", C.c_float), ("sfo_slope", C.c_float),
                ("oper_mode", C.c_int32), ("call_sign", C.c_uint64), ("best_lane", C.c_int32),
                ("bit_flips", C.c_int32), ("esn0_db_last", C.c_float), ("n_sync_rejects", C.c_int32)]


RESULT_DTYPE = np.dtype([("status", "<i4"), ("symbol_pos", "<i4"), ("sc_start", "<i8"), ("cfo_rad", "<f4"),
                         ("cfo_fine", "<f4"), ("sfo_slope", "<f4"), ("oper_mode", "<i4"), ("call_sign", "<u8"),
                         ("best_lane", "<i4"), ("bit_flips", "<i4"), ("esn0_db_last", "<f4"),
                         ("n_sync_rejects", "<i4")], align=True)
assert RESULT_DTYPE.itemsize == C.sizeof(FrameResult)
# ofdmrx_attempt: one preamble of a frame's SKIP loop (decode.cc:390-448)
ATTEMPT_DTYPE = np.dtype([("status", "<i4"), ("symbol_pos", "<i4"), ("cfo_rad", "<f4"), ("oper_mode", "<i4"), ("call_sign", "<u8")], align=True)
assert ATTEMPT_DTYPE.itemsize == 24
MAX_SKIP = 64


class Channel(C.Structure):
    _fields_ = [("cfo_hz", C.c_float), ("sfo_ppm", C.c_float), ("ntaps", C.c_int32), ("delays", C.c_int32 * 8),
                ("gains_re", C.c_float * 8), ("gains_im", C.c_float * 8)]


class Fading(C.Structure):
    _fields_ = [("ntaps", C.c_int32), ("delays", C.c_int32 * 8), ("gains_re", C.c_float * 8), ("gains_im", C.c_float * 8),
                ("spread_hz", C.c_float * 8)]


FADING_SINES, FADING_KNOT, FADING_MAX_DELAY = 16, 32, 1024
# ITU-R F.520 presets: two paths of equal mean power, (differential delay in ms, frequency spread (2 sigma) in Hz)
WATTERSON = {"good": (0.5, 0.1), "moderate": (1.0, 0.5), "poor": (2.0, 1.0)}


def watterson(preset, sample_rate):
    """the paths [(delay, complex gain, spread_hz), ...] of an F.520 preset for Receiver.fading: two paths of gain 1 / sqrt 2, the
    second delayed by round(ms * rate / 1000) samples"""
    try:
        ms, spread = WATTERSON[preset]
    except KeyError:
        raise ValueError("watterson: preset must be one of %s" % ", ".join(WATTERSON))
    g = complex(0.5 ** 0.5, 0.0)
    return [(0, g, spread), (int(round(ms * sample_rate / 1000.0)), g, spread)]


def channelize_taps(decim):
    """the 24 decim + 1 fp32 taps of the wideband front end's low pass for decimation decim (2 .. 32): DESIGN.md section 4.14"""
    decim = int(decim)
    taps = np.zeros(24 * max(decim, 0) + 1, np.float32)
    n = load_library().ofdmrx_util_channelize_taps(decim, _ptr(taps))
    if n != taps.size:
        raise OfdmRxError("channelize_taps: decim must be 2 .. 32")
    return taps


def channelize_grid_taps(decim):
    """the 24 decim + 1 fp32 taps of the grid front end's prototype low pass for decimation decim (a power of two 2 .. 512): DESIGN.md
    section 4.19; for decim <= 32 they are channelize_taps(decim).  A ratio - a pair (p, q) or a fractions.Fraction - gives the taps
    [q', T] of the grid front end at that ratio"""
    decim, q = _ratio(decim)
    if q is not None:
        p, q, _, _ = _grid_ratio(decim, q)
        taps = np.zeros((q, 24 * p // q + 1), np.float32)
        if load_library().ofdmrx_util_channelize_grid_ratio_taps(p, q, _ptr(taps)) != taps.shape[1]:
            raise OfdmRxError("channelize_grid_taps: the library refused the ratio")
        return taps
    taps = np.zeros(24 * min(max(decim, 0), 512) + 1, np.float32)
    n = load_library().ofdmrx_util_channelize_grid_taps(decim, _ptr(taps))
    if n != taps.size:
        raise OfdmRxError("channelize_grid_taps: decim must be a power of two 2 .. 512")
    return taps


def _grid_ratio(p, q):
    """-> (p', q', k_first, n_all) of the grid front end at the ratio p / q, reduced to lowest terms"""
    p, q = int(p), int(q)
    k0, n = C.c_int32(0), C.c_size_t(0)
    if p <= 0 or q <= 0 or load_library().ofdmrx_util_grid_ratio_slots(p, q, C.byref(k0), C.byref(n)):
        raise OfdmRxError("grid: in lowest terms q must be 1 .. 16, p 2 q .. 512 with no prime factor other than 2, 3 and 5")
    g = math.gcd(p, q)
    return p // g, q // g, k0.value, n.value


def _grid_ratio_slots(p, q, slots):
    """-> (p', q', the slots as int32 (None: all of them, ascending))"""
    p, q, k0, n = _grid_ratio(p, q)
    k = np.arange(k0, k0 + n, dtype=np.int32) if slots is None else np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
    if k.size < 1 or k.size > 65535 or k.min() < k0 or k.max() > k0 + n - 1:
        raise OfdmRxError("grid: 1 .. 65535 slots, each %d .. %d" % (k0, k0 + n - 1))
    return p, q, k


def _grid_slots(decim, slots):
    """-> the slots of a grid of decimation decim as int32 (None: all 2 decim of them, ascending)"""
    decim, q = _ratio(decim)
    if q is not None:
        return _grid_ratio_slots(decim, q, slots)[2]
    if decim < 2 or decim > 512 or decim & (decim - 1):
        raise OfdmRxError("grid: decim must be a power of two 2 .. 512")
    k = np.arange(-decim, decim, dtype=np.int32) if slots is None else np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
    if k.size < 1 or k.size > 65535 or k.min() < -decim or k.max() > decim - 1:
        raise OfdmRxError("grid: 1 .. 65535 slots, each -decim .. decim - 1")
    return k


def grid_centres(decim, rate, slots=None):
    """the centre frequencies in Hz of the slots of the grid front end: slot k of decimation decim at the
    handle rate `rate` lies at k rate / 2, k = -decim .. decim - 1 (slots None: all of them, ascending).  decim: an int, or a ratio - a
    pair (p, q) or a fractions.Fraction - whose slots are the k with -p <= k q < p (section 4.22)"""
    return _grid_slots(decim, slots).astype(np.float64) * (float(rate) / 2.0)


def _ratio(decim):
    """decim as the front end takes it: an int -> (decim, None), the integer entries; a pair (p, q) or a fractions.Fraction ->
    (p, q), the ratio entries"""
    if isinstance(decim, fractions.Fraction):
        return int(decim.numerator), int(decim.denominator)
    if isinstance(decim, (tuple, list)):
        p, q = decim
        return int(p), int(q)
    return int(decim), None


def channelize_ratio_taps(p, q):
    """the fp32 taps [q', T] of the wideband front end at the decimation p / q, reduced to lowest terms p' / q' (q' <= 16, 2 <= p / q
    <= 32), T = 24 p' // q' + 1: DESIGN.md section 4.17"""
    p, q = int(p), int(q)
    if p <= 0 or q <= 0:
        raise OfdmRxError("channelize_ratio_taps: p and q must be positive")
    g = math.gcd(p, q)
    p, q = p // g, q // g
    T = 24 * p // q + 1
    taps = np.zeros((min(q, 16), T), np.float32)
    if q > 16 or load_library().ofdmrx_util_channelize_ratio_taps(p, q, _ptr(taps)) != T:
        raise OfdmRxError("channelize_ratio_taps: the reduced q must be 1 .. 16 and p / q 2 .. 32")
    return taps


def synthesize_support(n_in, interp):
    """the length of a channel's support in the wideband synthesizer's capture, counted from its start: ((n_in - 1 + 24) p) // q + 1
    for interp p / q - an int, a pair (p, q) or a fractions.Fraction (DESIGN.md sections 4.15 and 4.18)"""
    p, q = _ratio(interp)
    q = 1 if q is None else q
    if p <= 0 or q <= 0 or int(n_in) < 1:
        raise OfdmRxError("synthesize_support: n_in, p and q must be positive")
    g = math.gcd(p, q)
    return ((int(n_in) - 1 + 24) * (p // g)) // (q // g) + 1


def synthesize_grid_chunk(interp):
    """the outputs per host chunk of the grid synthesizer at interpolation interp (a power of two 2 .. 512), counted from out_first
    rounded down to a multiple of interp: DESIGN.md section 4.20.  A seam changes no byte; the number is there for the curious.
    interp may be a ratio - a pair (p, q) or a fractions.Fraction: the outputs per chunk of the grid synthesizer at that ratio, counted
    from out_first rounded down to a multiple of the reduced p (section 4.23)"""
    L = load_library()
    interp, q = _ratio(interp)
    if q is not None:
        n = L.ofdmrx_util_synthesize_grid_ratio_chunk(interp, q) if interp > 0 and q > 0 else -1
        if n <= 0:
            raise OfdmRxError("synthesize_grid_chunk: in lowest terms q must be 1 .. 16, p 2 q .. 512 with no prime factor other than 2, 3 and 5")
        return int(n)
    n = L.ofdmrx_util_synthesize_grid_chunk(int(interp))
    if n <= 0:
        raise OfdmRxError("synthesize_grid_chunk: interp must be a power of two 2 .. 512")
    return int(n)


SURVEY_NFFT = (1280, 2560, 5120)


class Band(C.Structure):
    _fields_ = [("centre_hz", C.c_double), ("width_hz", C.c_double), ("power", C.c_double), ("level_db", C.c_float),
                ("first_bin", C.c_int32), ("last_bin", C.c_int32)]


def survey_window(nfft):
    """the nfft fp32 values of the survey's periodic Hann window (nfft 1280, 2560 or 5120): DESIGN.md section 4.16"""
    nfft = int(nfft)
    w = np.zeros(max(nfft, 1), np.float32)
    if nfft not in SURVEY_NFFT or load_library().ofdmrx_util_survey_window(nfft, _ptr(w)) != nfft:
        raise OfdmRxError("survey_window: nfft must be 1280, 2560 or 5120")
    return w


def find_bands(psd_row, rate_wide, thr_db=6.0, gap_hz=200.0, min_width_hz=1000.0, abs_floor=0.0, with_floor=False):
    """the occupied bands of ONE survey row (fp32 [nfft], ascending frequency, on the host or a device tensor) of a capture at rate_wide
    -> a list of dicts (centre_hz, width_hz, power, level_db, first_bin, last_bin) in ascending frequency; with_floor: -> (list, floor).
    The floor is the row's median (or abs_floor where that is larger): the noise floor only while less than half the band is occupied"""
    if hasattr(psd_row, "detach"):
        psd_row = psd_row.detach().cpu().numpy()
    row = np.ascontiguousarray(psd_row, dtype=np.float32).reshape(-1)
    L = load_library()
    bands = (Band * row.size)()
    n, floor = C.c_size_t(0), C.c_double(0.0)
    r = L.ofdmrx_util_find_bands(_ptr(row), row.size, rate_wide, thr_db, gap_hz, min_width_hz, abs_floor, row.size, bands, C.byref(n), C.byref(floor))
    if r != 0:
        raise OfdmRxError("find_bands: %s (%d)" % (L.ofdmrx_strerror(r).decode(), r))
    out = [{k: getattr(bands[i], k) for k, _ in Band._fields_} for i in range(n.value)]
    return (out, floor.value) if with_floor else out


class Slot(C.Structure):
    _fields_ = [("slot", C.c_int), ("centre_hz", C.c_double), ("power", C.c_double), ("level_db", C.c_float)]


def survey_grid_span(decim, times_per_row, row_first, n_rows):
    """the wideband positions the rows row_first .. row_first + n_rows - 1 of the grid survey need -> (first position, count):
    max(0, (row_first S - 24) D) .. ((row_first + n_rows) S - 1) D with S = times_per_row, D = decim.  decim may
    be a ratio - a pair (p, q) or a fractions.Fraction: max(0, (row_first S p) // q - 24 p // q) .. (((row_first + n_rows) S - 1) p) // q
    with p / q in lowest terms (section 4.24)"""
    D, q = _ratio(decim)
    S, r0, n = int(times_per_row), int(row_first), int(n_rows)
    if q is not None:
        p, q, _, _ = _grid_ratio(D, q)
    else:
        _grid_slots(D, None)
    if S < 8 or S > 65536 or S % 8 or r0 < 0 or n < 1:
        raise OfdmRxError("survey_grid_span: times_per_row a multiple of 8 in 8 .. 65536, row_first >= 0, n_rows >= 1")
    if q is not None:
        first = max(0, (r0 * S * p) // q - 24 * p // q)
        return first, (((r0 + n) * S - 1) * p) // q - first + 1
    first = max(0, (r0 * S - 24) * D)
    return first, ((r0 + n) * S - 1) * D - first + 1


def find_slots(row, decim, rate, thr_db=6.0, sep_db=8.0, abs_floor=0.0, with_floor=False):
    """the occupied slots of ONE grid survey row (fp32 [2 decim], ascending slot order, on the host or a device tensor) at the handle
    rate `rate` -> a list of dicts (slot, centre_hz, power, level_db) in ascending order; with_floor: -> (list, floor).  The floor is
    abs_floor where that is > 0, else the row's median; a slot more than sep_db below a cyclic neighbour is taken for that
    neighbour's edge and dropped - so a real signal that far below a neighbouring one is not found.  decim
    may be a ratio - a pair (p, q) or a fractions.Fraction: the row then holds the n_all slots of the grid at that ratio, whose first
    and last slot are neighbours only where the slots tile the circle (the reduced q is 1 or 2); where they lie half a slot apart or
    less across the band edge and within sep_db of each other they are one signal and the louder is reported (section 4.24)"""
    if hasattr(row, "detach"):
        row = row.detach().cpu().numpy()
    row = np.ascontiguousarray(row, dtype=np.float32).reshape(-1)
    decim, q = _ratio(decim)
    L = load_library()
    if q is not None:
        p, q, _, n_all = _grid_ratio(decim, q)
        if row.size != n_all:
            raise OfdmRxError("find_slots: the row of the ratio %d/%d has %d values" % (p, q, n_all))
    elif decim < 2 or decim > 512 or decim & (decim - 1) or row.size != 2 * decim:
        raise OfdmRxError("find_slots: decim must be a power of two 2 .. 512 and the row 2 decim values")
    slots = (Slot * row.size)()
    n, floor = C.c_size_t(0), C.c_double(0.0)
    if q is not None:
        r = L.ofdmrx_util_find_slots_ratio(_ptr(row), p, q, rate, thr_db, sep_db, abs_floor, row.size, slots, C.byref(n), C.byref(floor))
    else:
        r = L.ofdmrx_util_find_slots(_ptr(row), decim, rate, thr_db, sep_db, abs_floor, row.size, slots, C.byref(n), C.byref(floor))
    if r != 0:
        raise OfdmRxError("find_slots: %s (%d)" % (L.ofdmrx_strerror(r).decode(), r))
    out = [{k: getattr(slots[i], k) for k, _ in Slot._fields_} for i in range(n.value)]
    return (out, floor.value) if with_floor else out


class Timing(C.Structure):
    _fields_ = [("ms", C.c_float * 9), ("launches", C.c_int32 * 9)]


def lib_path():
    """MODEM_AMD_LIB selects an alternative build of the same library (A/B runs of kernel variants)"""
    return os.environ.get("MODEM_AMD_LIB") or os.path.join(HERE, "lib", "libofdmrx.so")


def build(force=False):
    """compile every HIP source for gfx950 (hipcc cross-compiles without a GPU)"""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", CSRC, "-j8", "all"], stdout=subprocess.DEVNULL)
    return lib_path()


_LIB = None


def load_library():
    """dlopen libofdmrx.so; fails loudly when the HIP extension has not been built"""
    global _LIB
    if _LIB is not None:
        return _LIB
    # torch bundles its own HIP runtime (same SONAME libamdhip64.so.7).  Two HIP runtimes in one
    # process cannot both see the GPU, so when torch is importable it is loaded FIRST and libofdmrx
    # binds to the runtime already in the process.  MODEM_AMD_NO_TORCH=1 skips this (pure C ABI use).
    if not os.environ.get("MODEM_AMD_NO_TORCH"):
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    path = lib_path()
    if not os.path.exists(path):
        raise OfdmRxError("libofdmrx.so is missing (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "-- the receive path has no CPU fallback" % path)
    L = C.CDLL(path)
    L.ofdmrx_abi_version.restype = C.c_int
    L.ofdmrx_strerror.restype = C.c_char_p
    L.ofdmrx_strerror.argtypes = [C.c_int]
    L.ofdmrx_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
    L.ofdmrx_destroy.argtypes = [C.c_void_p]
    L.ofdmrx_destroy.restype = None
    batch = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ofdmrx_decode_batch.argtypes = batch
    L.ofdmrx_decode_batch_device.argtypes = batch
    stream = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    L.ofdmrx_decode_stream.argtypes = stream
    L.ofdmrx_decode_stream_device.argtypes = stream
    L.ofdmrx_debug_stream_edges.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(C.c_size_t)]
    streams = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
               C.c_void_p, C.c_void_p]
    L.ofdmrx_decode_streams.argtypes = streams
    L.ofdmrx_decode_streams_device.argtypes = streams
    L.ofdmrx_debug_streams_edges.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]
    L.ofdmrx_feed_begin.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.ofdmrx_feed_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t),
                                   C.POINTER(C.c_size_t)]
    L.ofdmrx_feed_end.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.ofdmrx_feed_lag.argtypes = [C.c_void_p]
    L.ofdmrx_feed_lag.restype = C.c_longlong
    L.ofdmrx_feed_resident_samples.argtypes = [C.c_void_p]
    L.ofdmrx_feed_resident_samples.restype = C.c_longlong
    L.ofdmrx_bank_begin.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    L.ofdmrx_bank_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.ofdmrx_bank_end.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t),
                                  C.POINTER(C.c_size_t)]
    L.ofdmrx_bank_begin_wideband.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int]
    L.ofdmrx_bank_push_wideband.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    for f in (L.ofdmrx_bank_resident_samples, L.ofdmrx_bank_preambles):
        f.argtypes = [C.c_void_p, C.c_size_t]
        f.restype = C.c_longlong
    L.ofdmrx_bank_last_stage_ops.argtypes = [C.c_void_p]
    L.ofdmrx_bank_last_stage_ops.restype = C.c_longlong
    L.ofdmrx_synchronize.argtypes = [C.c_void_p]
    L.ofdmrx_get_timing.argtypes = [C.c_void_p, C.POINTER(Timing)]
    L.ofdmrx_chunk_frames.argtypes = [C.c_void_p]
    L.ofdmrx_set_esn0_rows.argtypes = [C.c_void_p, C.c_void_p]
    L.ofdmrx_set_attempt_log.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ofdmrx_list_decoded_frames.argtypes = [C.c_void_p]
    L.ofdmrx_list_decoded_frames.restype = C.c_longlong
    L.ofdmrx_last_chunk_first_frame.argtypes = [C.c_void_p]
    L.ofdmrx_last_chunk_first_frame.restype = C.c_longlong
    L.ofdmrx_sc_decided_frames.argtypes = [C.c_void_p]
    L.ofdmrx_sc_decided_frames.restype = C.c_longlong
    L.ofdmrx_get_sc_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
    L.ofdmrx_debug_sc_path.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ofdmrx_debug_dump.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t]
    L.ofdmrx_debug_polar.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.ofdmrx_debug_decode_cons.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ofdmrx_debug_polar_modes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ofdmrx_debug_decode_cons_modes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]
    L.ofdmrx_debug_theil_sen.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    L.ofdmrx_debug_osd.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.ofdmrx_debug_fft.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    L.ofdmrx_util_awgn_tile.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                        C.c_float, C.c_uint64, C.c_uint64]
    L.ofdmrx_util_channel.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(Channel)]
    L.ofdmrx_util_fading.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(Fading),
                                     C.c_uint64, C.c_uint64]
    L.ofdmrx_util_channelize_taps.argtypes = [C.c_int, C.c_void_p]
    L.ofdmrx_util_channelize_ratio_taps.argtypes = [C.c_int, C.c_int, C.c_void_p]
    L.ofdmrx_util_channelize_ratio.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                               C.c_size_t, C.c_longlong, C.c_size_t, C.c_void_p, C.c_size_t]
    L.ofdmrx_bank_begin_wideband_ratio.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.ofdmrx_util_channelize_real.argtypes = L.ofdmrx_util_channelize_ratio.argtypes
    L.ofdmrx_bank_begin_wideband_real.argtypes = L.ofdmrx_bank_begin_wideband_ratio.argtypes
    L.ofdmrx_util_channelize_grid_taps.argtypes = [C.c_int, C.c_void_p]
    L.ofdmrx_util_channelize_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                              C.c_longlong, C.c_size_t, C.c_void_p, C.c_size_t]
    L.ofdmrx_bank_begin_wideband_grid.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int]
    L.ofdmrx_util_channelize_grid_ratio_taps.argtypes = [C.c_int, C.c_int, C.c_void_p]
    L.ofdmrx_util_grid_ratio_slots.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.ofdmrx_util_channelize_grid_ratio.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                                    C.c_size_t, C.c_longlong, C.c_size_t, C.c_void_p, C.c_size_t]
    L.ofdmrx_bank_begin_wideband_grid_ratio.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.ofdmrx_util_channelize.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                         C.c_longlong, C.c_size_t, C.c_void_p, C.c_size_t]
    L.ofdmrx_util_synthesize.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.c_longlong, C.c_size_t, C.c_void_p, C.c_int]
    L.ofdmrx_util_synthesize_ratio.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_size_t, C.c_longlong, C.c_size_t, C.c_void_p, C.c_int]
    L.ofdmrx_util_synthesize_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_size_t, C.c_longlong, C.c_size_t, C.c_void_p, C.c_int]
    L.ofdmrx_util_synthesize_grid_chunk.argtypes = [C.c_int]
    L.ofdmrx_util_synthesize_grid_chunk.restype = C.c_longlong
    L.ofdmrx_util_synthesize_grid_ratio.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_size_t, C.c_longlong, C.c_size_t, C.c_void_p, C.c_int]
    L.ofdmrx_util_synthesize_grid_ratio_chunk.argtypes = [C.c_int, C.c_int]
    L.ofdmrx_util_synthesize_grid_ratio_chunk.restype = C.c_longlong
    L.ofdmrx_util_survey_window.argtypes = [C.c_int, C.c_void_p]
    L.ofdmrx_util_survey.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_size_t, C.c_int, C.c_int, C.c_longlong, C.c_size_t,
                                     C.c_void_p]
    L.ofdmrx_util_find_bands.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_size_t,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
    L.ofdmrx_util_survey_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_size_t, C.c_int, C.c_int, C.c_longlong,
                                          C.c_size_t, C.c_void_p]
    L.ofdmrx_util_find_slots.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_size_t, C.c_void_p,
                                         C.c_void_p, C.c_void_p]
    L.ofdmrx_util_survey_grid_ratio.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                                C.c_longlong, C.c_size_t, C.c_void_p]
    L.ofdmrx_util_find_slots_ratio.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_size_t,
                                               C.c_void_p, C.c_void_p, C.c_void_p]
    L.ofdmrx_tx_frame_samples.restype = C.c_long
    L.ofdmrx_tx_frame_samples.argtypes = [C.c_int]
    L.ofdmrx_frame_samples.restype = C.c_long
    L.ofdmrx_frame_samples.argtypes = [C.c_int, C.c_int]
    L.ofdmrx_stream_samples.restype = C.c_long
    L.ofdmrx_stream_samples.argtypes = [C.c_int, C.c_int, C.c_int]
    L.ofdmrx_tx_encode_stream_device.restype = C.c_int
    L.ofdmrx_tx_encode_stream_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_char_p,
                                                 C.c_int, C.c_int, C.c_void_p]
    L.ofdmrx_tx_encode_stream.restype = C.c_int
    L.ofdmrx_tx_encode_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int,
                                          C.c_void_p]
    L.ofdmrx_callsign_value.restype = C.c_longlong
    L.ofdmrx_callsign_value.argtypes = [C.c_char_p]
    L.ofdmrx_tx_encode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_void_p]
    _LIB = L
    return L


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Receiver:
    """Batch counterpart of `new Decoder<float, Complex<float>, 8000>(out, pcm, skip)` (decode.cc:592).

    stream: a hipStream_t handle (int) to run on.  None / 0 (note: torch's DEFAULT stream has handle 0) makes the
    library create its own non-blocking stream - then synchronise explicitly before sharing device buffers with
    other libraries, or pass a non-default stream (torch.cuda.Stream().cuda_stream) and use it on both sides.

    decode(pcm) takes raw PCM frames [n_frames, samples, channels] (int16 / uint8 / float32, what
    DSP::ReadWAV would deliver) and returns (payload[n_frames, 5380] uint8, results structured array).
    """

    def __init__(self, device=0, chunk_frames=0, max_samples=0, descramble=True, keep_raw_cons=False, stream=None,
                 sample_rate=8000, list_size=8, scl_always=False, no_sc=False, two_lanes=False):
        self._lib = load_library()
        if self._lib.ofdmrx_abi_version() != 1:
            raise OfdmRxError("ABI mismatch")
        self.sample_rate = int(sample_rate)
        cfg = Config(1, self.sample_rate, int(list_size), device, chunk_frames, max_samples, 1 if descramble else 0,
                     (1 if keep_raw_cons else 0) | (2 if scl_always else 0) | (4 if no_sc else 0) | (8 if two_lanes else 0), stream)
        self._h = C.c_void_p()
        self._check(self._lib.ofdmrx_create(C.byref(cfg), C.byref(self._h)))

    def _check(self, r):
        if r != 0:
            raise OfdmRxError("ofdmrx: %s (%d)" % (self._lib.ofdmrx_strerror(r).decode(), r))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.ofdmrx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def chunk_frames(self):
        return self._lib.ofdmrx_chunk_frames(self._h)

    @staticmethod
    def _fmt(dtype):
        return {np.dtype(np.int16): FMT_S16, np.dtype(np.uint8): FMT_U8, np.dtype(np.float32): FMT_F32}[np.dtype(dtype)]

    def decode(self, pcm, skip=None, esn0_rows=False, attempts=False):
        """-> (payload, results[, esn0 rows][, (attempt log [n, 65], counts [n])])"""
        pcm = np.ascontiguousarray(pcm)
        if pcm.ndim == 2:
            pcm = pcm[None]
        n, spf, ch = pcm.shape
        stride = spf * ch * pcm.dtype.itemsize
        if stride % 4:
            pad = np.zeros((n, (stride + 3) // 4 * 4), np.uint8)
            pad[:, :stride] = pcm.reshape(n, -1).view(np.uint8)
            buf, stride = pad, pad.shape[1]
        else:
            buf = pcm
        out = np.zeros((n, PAYLOAD_BYTES), np.uint8)
        res = np.zeros(n, RESULT_DTYPE)
        sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.int32)
        rows = np.zeros((n, 126), np.float32) if esn0_rows else None
        if esn0_rows:
            self._check(self._lib.ofdmrx_set_esn0_rows(self._h, _ptr(rows)))
        if attempts:
            alog, acnt = np.zeros((n, MAX_SKIP + 1), ATTEMPT_DTYPE), np.zeros(n, np.int32)
            self._check(self._lib.ofdmrx_set_attempt_log(self._h, _ptr(alog), _ptr(acnt)))
        try:
            self._check(self._lib.ofdmrx_decode_batch(self._h, _ptr(buf), self._fmt(pcm.dtype), ch, spf, stride, n,
                                                      _ptr(sk) if sk is not None else None, _ptr(out), _ptr(res)))
        finally:
            if esn0_rows:
                self._lib.ofdmrx_set_esn0_rows(self._h, None)
            if attempts:
                self._lib.ofdmrx_set_attempt_log(self._h, None, None)
        ret = (out, res) + ((rows,) if esn0_rows else ()) + (((alog, acnt),) if attempts else ())
        return ret

    def decode_stream(self, pcm, max_frames=None, esn0_rows=False):
        """one recording [samples, channels] (or [samples] mono) -> (payloads [k, 5380], results [k], n_preambles[, esn0 rows]),
        k = min(n_preambles, max_frames); max_frames None: every preamble (the call is made twice when the first guess is short)"""
        pcm = np.ascontiguousarray(pcm)
        if pcm.ndim == 1:
            pcm = pcm[:, None]
        n, ch = pcm.shape
        cap = max_frames if max_frames is not None else max(16, n // 20000)
        while True:
            out = np.zeros((max(cap, 1), PAYLOAD_BYTES), np.uint8)
            res = np.zeros(max(cap, 1), RESULT_DTYPE)
            rows = np.zeros((max(cap, 1), 126), np.float32) if esn0_rows else None
            npre = C.c_size_t(0)
            if esn0_rows:
                self._check(self._lib.ofdmrx_set_esn0_rows(self._h, _ptr(rows)))
            try:
                self._check(self._lib.ofdmrx_decode_stream(self._h, _ptr(pcm), self._fmt(pcm.dtype), ch, n, cap, _ptr(out), _ptr(res),
                                                           C.byref(npre)))
            finally:
                if esn0_rows:
                    self._lib.ofdmrx_set_esn0_rows(self._h, None)
            if max_frames is not None or npre.value <= cap:
                break
            cap = npre.value
        k = min(npre.value, cap)
        return (out[:k], res[:k], npre.value) + ((rows[:k],) if esn0_rows else ())

    def feed(self, channels, dtype=np.int16, esn0_rows=False):
        """open a live feed of `channels` interleaved values of dtype: push blocks as they arrive, take each record when it is due"""
        return Feed(self, channels, dtype, esn0_rows)

    def bank(self, n_channels, channels, dtype=np.int16, esn0_rows=False):
        """open a bank of n_channels live channels of `channels` interleaved values of dtype: push one block per channel per call"""
        return Bank(self, n_channels, channels, dtype, esn0_rows)

    def wideband_bank(self, centres_hz, decim, dtype=np.int16, esn0_rows=False):
        """open a bank whose channels are cut from one wideband I/Q capture (decim x the handle's rate, interleaved I/Q of dtype) at
        the centre frequencies centres_hz: push the capture block by block.  decim: an int, or a ratio - a pair (p, q) or a
        fractions.Fraction"""
        return WidebandBank(self, centres_hz, decim, dtype, esn0_rows)

    def wideband_real_bank(self, centres_hz, decim, dtype=np.int16, esn0_rows=False):
        """open a bank whose channels are cut from one REAL wideband capture (decim x the handle's rate, one value of dtype per
        position) at the centre frequencies centres_hz: push the capture as 1-D blocks.  decim: an int, a
        pair (p, q) or a fractions.Fraction.  The centres obey Receiver.channelize_real's rule"""
        return WidebandRealBank(self, centres_hz, decim, dtype, esn0_rows)

    def wideband_grid_bank(self, slots, decim, dtype=np.int16, esn0_rows=False):
        """open a bank whose channels are slots of the raster rate / 2 of one wideband I/Q capture at decim x the handle's rate (decim a
        power of two 2 .. 512; slots None: all 2 decim): push the capture block by block.  decim may be a ratio
        - a pair (p, q) or a fractions.Fraction (section 4.22)"""
        return WidebandGridBank(self, slots, decim, dtype, esn0_rows)

    def decode_stream_device(self, d_samples, fmt, channels, n_samples, max_frames, d_payload, d_results):
        """device pointers (ints), or pinned host outputs; -> n_preambles (the call synchronises once, after the scan)"""
        npre = C.c_size_t(0)
        self._check(self._lib.ofdmrx_decode_stream_device(self._h, d_samples, fmt, channels, n_samples, max_frames, d_payload, d_results,
                                                          C.byref(npre)))
        return npre.value

    def debug_stream_edges(self, timing, max_edges=None):
        """the stream scan's trigger on a timing sequence -> (t_edge, t_max, index_max) of every falling edge"""
        timing = np.ascontiguousarray(timing, dtype=np.float32)
        cap = max_edges if max_edges is not None else max(1, len(timing) // 2 + 1)
        te, tm, im = np.zeros(cap, np.int64), np.zeros(cap, np.int64), np.zeros(cap, np.int32)
        ne = C.c_size_t(0)
        self._check(self._lib.ofdmrx_debug_stream_edges(self._h, _ptr(timing), len(timing), cap, _ptr(te), _ptr(tm), _ptr(im), C.byref(ne)))
        k = min(ne.value, cap)
        return te[:k], tm[:k], im[:k], ne.value

    def decode_streams(self, pcms, max_frames_per_stream=None, esn0_rows=False, max_records=None, stride_samples=None):
        """many recordings in one call: pcms is a list of arrays [samples, channels] (or [samples] mono) of one dtype and channel
        count, lengths may differ -> a list of (payloads [k, 5380], results [k], n_preambles) per recording, k =
        min(n_preambles, max_frames_per_stream) (less for the recordings max_records cuts); with esn0_rows each tuple ends with its
        rows.  max_records None: every record (the call is made twice when the first guess is short)"""
        pcms = [np.ascontiguousarray(p) for p in pcms]
        pcms = [p[:, None] if p.ndim == 1 else p for p in pcms]
        if not pcms or any(p.dtype != pcms[0].dtype or p.shape[1] != pcms[0].shape[1] for p in pcms):
            raise OfdmRxError("decode_streams: the recordings must share dtype and channel count")
        dt, ch, S = pcms[0].dtype, pcms[0].shape[1], len(pcms)
        lens = np.array([p.shape[0] for p in pcms], np.uintp)
        stride = max(int(lens.max()), 1) if stride_samples is None else int(stride_samples)
        buf = np.zeros((S, stride, ch), dt)
        for q, p in enumerate(pcms):
            buf[q, :p.shape[0]] = p
        per = np.iinfo(np.uintp).max if max_frames_per_stream is None else int(max_frames_per_stream)
        cap = int(max_records) if max_records is not None else int(sum(min(per, max(16, int(n) // 20000)) for n in lens))
        npre, first = np.zeros(S, np.uintp), np.zeros(S + 1, np.uintp)
        while True:
            out = np.zeros((max(cap, 1), PAYLOAD_BYTES), np.uint8)
            res = np.zeros(max(cap, 1), RESULT_DTYPE)
            rows = np.zeros((max(cap, 1), 126), np.float32) if esn0_rows else None
            if esn0_rows:
                self._check(self._lib.ofdmrx_set_esn0_rows(self._h, _ptr(rows)))
            try:
                self._check(self._lib.ofdmrx_decode_streams(self._h, _ptr(buf), self._fmt(dt), ch, S, stride * ch * dt.itemsize, _ptr(lens), per, cap,
                                                            _ptr(out) if cap else None, _ptr(res) if cap else None, _ptr(npre), _ptr(first)))
            finally:
                if esn0_rows:
                    self._lib.ofdmrx_set_esn0_rows(self._h, None)
            if max_records is not None or int(first[S]) <= cap:
                break
            cap = int(first[S])
        ret = []
        for q in range(S):
            a, b = min(int(first[q]), cap), min(int(first[q + 1]), cap)
            ret.append((out[a:b], res[a:b], int(npre[q])) + ((rows[a:b],) if esn0_rows else ()))
        return ret

    def decode_streams_device(self, d_samples, fmt, channels, n_samples, stride_bytes, max_frames_per_stream, max_records, d_payload, d_results):
        """device pointers (ints), or pinned host outputs; n_samples: the recordings' lengths (host) -> (n_preambles [S], first_record
        [S + 1]); the call synchronises once, after the scan of all recordings"""
        lens = np.ascontiguousarray(n_samples, dtype=np.uintp)
        S = len(lens)
        npre, first = np.zeros(S, np.uintp), np.zeros(S + 1, np.uintp)
        self._check(self._lib.ofdmrx_decode_streams_device(self._h, d_samples, fmt, channels, S, stride_bytes, _ptr(lens), max_frames_per_stream,
                                                           max_records, d_payload, d_results, _ptr(npre), _ptr(first)))
        return npre.astype(np.int64), first.astype(np.int64)

    def debug_streams_edges(self, timings, max_edges_per_stream=None):
        """the segmented trigger scan on several timing sequences -> per sequence (t_edge, t_max, index_max, n_edges)"""
        timings = [np.ascontiguousarray(t, dtype=np.float32) for t in timings]
        lens = np.array([len(t) for t in timings], np.uintp)
        S = len(timings)
        cap = max_edges_per_stream if max_edges_per_stream is not None else max(1, int(lens.max()) // 2 + 1)
        packed = np.concatenate(timings) if S else np.zeros(0, np.float32)
        te, tm, im = np.zeros((S, cap), np.int64), np.zeros((S, cap), np.int64), np.zeros((S, cap), np.int32)
        ne = np.zeros(S, np.uintp)
        self._check(self._lib.ofdmrx_debug_streams_edges(self._h, _ptr(packed), S, _ptr(lens), cap, _ptr(te), _ptr(tm), _ptr(im), _ptr(ne)))
        return [(te[q, :min(int(ne[q]), cap)], tm[q, :min(int(ne[q]), cap)], im[q, :min(int(ne[q]), cap)], int(ne[q])) for q in range(S)]

    def set_esn0_rows(self, d_rows):
        """device pointer (int) to n x 126 floats for the decode_device calls that follow, or None"""
        self._check(self._lib.ofdmrx_set_esn0_rows(self._h, d_rows))

    def decode_device(self, d_samples, fmt, channels, spf, stride, n, d_payload, d_results, d_skip=None):
        """device pointers (ints); asynchronous on the handle's stream"""
        self._check(self._lib.ofdmrx_decode_batch_device(self._h, d_samples, fmt, channels, spf, stride, n,
                                                         d_skip, d_payload, d_results))

    def list_decoded_frames(self):
        """frames of the last decode call the syndrome certificate left to the list decoder (-1: certificate off)"""
        return int(self._lib.ofdmrx_list_decoded_frames(self._h))

    def last_chunk_first_frame(self):
        """index, in the last decode call, of the first frame of the chunk the taps belong to"""
        return int(self._lib.ofdmrx_last_chunk_first_frame(self._h))

    def sc_decided_frames(self):
        """frames of the last decode call finished by the list-1 pass (-1: that pass is off)"""
        return int(self._lib.ofdmrx_sc_decided_frames(self._h))

    def sc_timing(self):
        ms, n = C.c_float(), C.c_int32()
        self._check(self._lib.ofdmrx_get_sc_timing(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def synchronize(self):
        self._check(self._lib.ofdmrx_synchronize(self._h))

    def timing(self):
        t = Timing()
        self._check(self._lib.ofdmrx_get_timing(self._h, C.byref(t)))
        return {s: (t.ms[i], t.launches[i]) for i, s in enumerate(STAGES)}

    def tap(self, name, frame, samples=None, cons_cnt=21600, rows=50):
        """stage tap of the last resident chunk; cons_cnt / rows default to mode 6 (other modes: up to 32400 / 126)"""
        shapes = dict(HDR_SOFT=((255,), np.int8), CONS_RAW=((cons_cnt, 2), np.float32), CONS_ROT=((cons_cnt, 2), np.float32),
                      SLOPE=((rows,), np.float32), YINT=((rows,), np.float32), PRECISION=((rows,), np.float32),
                      LLR=((CODE_LEN,), np.float32), METRIC=((8,), np.float32), LANE_MESG=((8, MESG_BYTES), np.uint8),
                      ANALYTIC=((samples or 0, 2), np.float32))
        shape, dt = shapes[name]
        a = np.zeros(shape, dt)
        self._check(self._lib.ofdmrx_debug_dump(self._h, TAPS[name], frame, _ptr(a), a.nbytes))
        return a

    # ---- single-stage entry points (parity tests)
    def polar(self, llr, modes=None):
        """the list decoder alone: per-lane messages and path metrics.  modes None: mode-6 codewords, messages [n, 8, 5476]
        (ofdmrx_debug_polar); else the operation mode of every vector (6..13), messages [n, 8, 5512] with mesg_bits / 8 bytes of
        message per lane and zeros behind (ofdmrx_debug_polar_modes)"""
        llr = np.ascontiguousarray(llr, dtype=np.float32).reshape(-1, CODE_LEN)
        n = llr.shape[0]
        metric = np.zeros((n, 8), np.float32)
        if modes is None:
            mesg = np.zeros((n, 8, MESG_BYTES), np.uint8)
            self._check(self._lib.ofdmrx_debug_polar(self._h, _ptr(llr), n, _ptr(mesg), _ptr(metric)))
        else:
            mode = np.ascontiguousarray(np.broadcast_to(np.asarray(modes, np.int32), (n,)))
            mesg = np.zeros((n, 8, MESG_BYTES_MAX), np.uint8)
            self._check(self._lib.ofdmrx_debug_polar_modes(self._h, _ptr(llr), n, _ptr(mode), _ptr(mesg), _ptr(metric)))
        return mesg, metric

    def sc_path(self, llr, modes=None):
        """k_sc alone: codeword bits [n, 65536], hard decisions of the LLRs [n, 65536], metric, min_fork, rule [n]; modes: the
        operation mode of every vector (its frozen table), None = all mode 6"""
        llr = np.ascontiguousarray(llr, dtype=np.float32).reshape(-1, CODE_LEN)
        n = llr.shape[0]
        mode = None if modes is None else _ptr(np.ascontiguousarray(np.broadcast_to(np.asarray(modes, np.int32), (n,))))
        cw = np.zeros((n, CODE_LEN // 8), np.uint8)
        hd = np.zeros((n, CODE_LEN // 8), np.uint8)
        metric, fork, ok = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
        self._check(self._lib.ofdmrx_debug_sc_path(self._h, _ptr(llr), n, mode, _ptr(cw), _ptr(hd), _ptr(metric), _ptr(fork), _ptr(ok)))
        return np.unpackbits(cw, axis=1, bitorder="little"), np.unpackbits(hd, axis=1, bitorder="little"), metric, fork, ok

    def decode_cons(self, cons, use_cert=True, modes=None):
        """rotated constellation rows (n x 21600 complex64, mode 6) -> payloads, results, who finished each frame (1 the syndrome
        certificate, 2 the list-1 pass, 0 the list decoder).  use_cert: 0 / False list decoder only, 1 / True syndrome certificate
        first, 2 the default chain (certificate, list-1 pass, list decoder), 3 list-1 pass then list decoder.  modes: the operation
        mode of every frame (6..13); cons is then [n, stride] with a frame's cols x rows points first (stride <= 32400 will do)"""
        out_res = lambda n: (np.zeros((n, 5380), np.uint8), np.zeros(n, RESULT_DTYPE), np.zeros(n, np.int32))
        if modes is None:
            cons = np.ascontiguousarray(cons, dtype=np.complex64).reshape(-1, 21600)
            n = cons.shape[0]
            out, res, cert = out_res(n)
            self._check(self._lib.ofdmrx_debug_decode_cons(self._h, _ptr(cons), n, int(use_cert), _ptr(out), _ptr(res), _ptr(cert)))
            return out, res, cert
        cons = np.ascontiguousarray(cons, dtype=np.complex64)
        assert cons.ndim == 2
        n, stride = cons.shape
        mode = np.ascontiguousarray(np.broadcast_to(np.asarray(modes, np.int32), (n,)))
        out, res, cert = out_res(n)
        self._check(self._lib.ofdmrx_debug_decode_cons_modes(self._h, _ptr(cons), stride, n, _ptr(mode), int(use_cert), _ptr(out), _ptr(res),
                                                             _ptr(cert)))
        return out, res, cert

    def theil_sen(self, y):
        y = np.ascontiguousarray(y, dtype=np.float32)
        rows, cols = y.shape
        s, i = np.zeros(rows, np.float32), np.zeros(rows, np.float32)
        self._check(self._lib.ofdmrx_debug_theil_sen(self._h, _ptr(y), rows, cols, _ptr(s), _ptr(i)))
        return s, i

    def osd(self, soft):
        soft = np.ascontiguousarray(soft, dtype=np.int8).reshape(-1, 255)
        n = soft.shape[0]
        hard, uniq = np.zeros((n, 32), np.uint8), np.zeros(n, np.int32)
        self._check(self._lib.ofdmrx_debug_osd(self._h, _ptr(soft), n, _ptr(hard), _ptr(uniq)))
        return hard, uniq

    def fft(self, x, sign=-1):
        x = np.ascontiguousarray(x, dtype=np.complex64)
        if x.ndim == 1:
            x = x[None]
        out = np.zeros_like(x)
        self._check(self._lib.ofdmrx_debug_fft(self._h, _ptr(x), x.shape[0], x.shape[1], sign, _ptr(out)))
        return out

    def awgn_tile(self, d_base, n_base, d_out, n_out, spf, noise_db, seed, first_frame=0):
        self._check(self._lib.ofdmrx_util_awgn_tile(self._h, d_base, n_base, d_out, n_out, spf, noise_db, seed, first_frame))

    def channel(self, d_in, d_out, n, spf, cfo_hz=0.0, sfo_ppm=0.0, multipath=()):
        """multipath | cfo | sfo on n device-resident 2-channel int16 frames (multipath = [(delay, complex gain), ...])"""
        ch = Channel()
        ch.cfo_hz, ch.sfo_ppm, ch.ntaps = cfo_hz, sfo_ppm, len(multipath)
        for i, (d, g) in enumerate(multipath):
            ch.delays[i], ch.gains_re[i], ch.gains_im[i] = int(d), float(complex(g).real), float(complex(g).imag)
        self._check(self._lib.ofdmrx_util_channel(self._h, d_in, d_out, n, spf, C.byref(ch)))

    def fading(self, d_in, n_in, d_out, n_out, spf, paths, seed, first_frame=0):
        """Watterson fading on device-resident 2-channel int16 frames: out frame f = in frame f % n_in under the realisation of
        (seed, first_frame + f); paths = [(delay, complex gain, spread_hz), ...] (watterson() gives the F.520 presets); asynchronous"""
        fd = Fading()
        if len(paths) > 8:
            raise OfdmRxError("fading: at most 8 paths")
        fd.ntaps = len(paths)
        for i, (d, g, s) in enumerate(paths):
            fd.delays[i], fd.gains_re[i], fd.gains_im[i], fd.spread_hz[i] = int(d), float(complex(g).real), float(complex(g).imag), float(s)
        self._check(self._lib.ofdmrx_util_fading(self._h, d_in, n_in, d_out, n_out, spf, C.byref(fd), seed, first_frame))

    def channelize(self, d_in, fmt, in_first, n_in, decim, centres_hz, out_first, n_out, d_out, out_stride=None):
        """the wideband front end on device buffers (ints): d_in holds the wideband positions in_first .. in_first + n_in - 1 of an
        interleaved I/Q capture at decim x the handle's rate; output n (out_first .. out_first + n_out - 1) of the channel centred at
        centres_hz[c] goes to d_out + 8 (c out_stride + n - out_first) as fp32 I/Q; asynchronous on the handle's stream.  decim: an
        int, or a ratio - a pair (p, q) or a fractions.Fraction"""
        f = np.ascontiguousarray(centres_hz, dtype=np.float64).reshape(-1)
        decim, q = _ratio(decim)
        if q is not None:
            self._check(self._lib.ofdmrx_util_channelize_ratio(self._h, d_in, fmt, in_first, n_in, decim, q, _ptr(f), f.size, out_first, n_out,
                                                               d_out, n_out if out_stride is None else out_stride))
            return
        self._check(self._lib.ofdmrx_util_channelize(self._h, d_in, fmt, in_first, n_in, decim, _ptr(f), f.size, out_first, n_out, d_out,
                                                     n_out if out_stride is None else out_stride))

    def channelize_real(self, d_in, fmt, in_first, n_in, decim, centres_hz, out_first, n_out, d_out, out_stride=None):
        """the wideband front end for a REAL capture on device buffers (ints): as channelize, but d_in holds
        ONE value of fmt per wideband position and n_in counts samples; the output is twice what channelize gives for the same
        samples with a zero imaginary part.  A centre with |f| < rate / 4 or |f| > decim rate / 2 - rate / 4 is refused (its mirror
        image overlaps it); a negative centre gives the conjugate spectrum's channel.  decim: an int, a pair (p, q) or a
        fractions.Fraction"""
        f = np.ascontiguousarray(centres_hz, dtype=np.float64).reshape(-1)
        p, q = _ratio(decim)
        self._check(self._lib.ofdmrx_util_channelize_real(self._h, d_in, fmt, in_first, n_in, p, 1 if q is None else q, _ptr(f), f.size,
                                                          out_first, n_out, d_out, n_out if out_stride is None else out_stride))

    def channelize_grid(self, d_in, fmt, in_first, n_in, decim, slots, out_first, n_out, d_out, out_stride=None):
        """the grid front end on device buffers (ints): as channelize, for a decim that is a power of two 2 ..
        512 and channels on the raster rate / 2: row j of the output is slot slots[j] (-decim .. decim - 1; None: every slot, ascending),
        centred at grid_centres(decim, rate, slots)[j].  decim may be a ratio - a pair (p, q) or a fractions.Fraction (section 4.22)"""
        decim, q = _ratio(decim)
        if q is not None:
            p, q, k = _grid_ratio_slots(decim, q, slots)
            self._check(self._lib.ofdmrx_util_channelize_grid_ratio(self._h, d_in, fmt, in_first, n_in, p, q, _ptr(k), k.size, out_first, n_out,
                                                                    d_out, n_out if out_stride is None else out_stride))
            return
        k = _grid_slots(decim, slots)
        self._check(self._lib.ofdmrx_util_channelize_grid(self._h, d_in, fmt, in_first, n_in, int(decim), _ptr(k), k.size, out_first, n_out,
                                                          d_out, n_out if out_stride is None else out_stride))

    def synthesize(self, d_in, in_fmt, n_in, interp, centres_hz, starts, gains, out_first, n_out, d_out, out_fmt, in_stride=None):
        """the wideband synthesizer on device buffers (ints): channel c's n_in sample frames (interleaved I/Q of in_fmt, S16 or F32) lie
        at d_in + c in_stride sample frames; it is placed at centres_hz[c], starts[c] wideband samples in, at gains[c], and the sum's
        positions out_first .. out_first + n_out - 1 at interp x the handle's rate go to d_out as out_fmt (S16 or F32); asynchronous on
        the handle's stream.  interp: an int, or a ratio - a pair (p, q) or a fractions.Fraction (section 4.18)"""
        f = np.ascontiguousarray(centres_hz, dtype=np.float64).reshape(-1)
        s = np.ascontiguousarray(starts, dtype=np.int64).reshape(-1)
        g = np.ascontiguousarray(gains, dtype=np.float32).reshape(-1)
        if not (f.size == s.size == g.size):
            raise OfdmRxError("synthesize: centres_hz, starts and gains must have one length")
        interp, q = _ratio(interp)
        if q is not None:
            self._check(self._lib.ofdmrx_util_synthesize_ratio(self._h, d_in, in_fmt, n_in if in_stride is None else in_stride, n_in, interp, q,
                                                               _ptr(f), _ptr(s), _ptr(g), f.size, out_first, n_out, d_out, out_fmt))
            return
        self._check(self._lib.ofdmrx_util_synthesize(self._h, d_in, in_fmt, n_in if in_stride is None else in_stride, n_in, interp, _ptr(f), _ptr(s),
                                                     _ptr(g), f.size, out_first, n_out, d_out, out_fmt))

    def synthesize_grid(self, d_in, in_fmt, n_in, interp, slots, starts, gains, out_first, n_out, d_out, out_fmt, in_stride=None):
        """the grid synthesizer on device buffers (ints): as synthesize, for an interp that is a power of two
        2 .. 512 and rows on the raster rate / 2: row c belongs to slot slots[c] (-interp .. interp - 1, pairwise distinct; None: every
        slot, ascending), centred at grid_centres(interp, rate, slots)[c]; starts are multiples of interp.  interp may be a ratio - a
        pair (p, q) or a fractions.Fraction (section 4.23): the slots are the k with -p <= k q < p, starts multiples of the reduced p"""
        interp, q = _ratio(interp)
        if q is not None:
            p, q, k = _grid_ratio_slots(interp, q, slots)
        else:
            k = _grid_slots(interp, slots)
        s = np.ascontiguousarray(starts, dtype=np.int64).reshape(-1)
        g = np.ascontiguousarray(gains, dtype=np.float32).reshape(-1)
        if not (k.size == s.size == g.size):
            raise OfdmRxError("synthesize_grid: slots, starts and gains must have one length")
        if q is not None:
            self._check(self._lib.ofdmrx_util_synthesize_grid_ratio(self._h, d_in, in_fmt, n_in if in_stride is None else in_stride, n_in, p, q,
                                                                    _ptr(k), _ptr(s), _ptr(g), k.size, out_first, n_out, d_out, out_fmt))
            return
        self._check(self._lib.ofdmrx_util_synthesize_grid(self._h, d_in, in_fmt, n_in if in_stride is None else in_stride, n_in, int(interp),
                                                          _ptr(k), _ptr(s), _ptr(g), k.size, out_first, n_out, d_out, out_fmt))

    def survey(self, d_wide, sample_format, nfft=1280, segs_per_row=None, in_first=0, row_first=0, n_rows=None):
        """the wideband survey: d_wide, a contiguous device tensor of interleaved I/Q of sample_format, holds
        the wideband positions in_first .. of a capture -> the Welch power spectrum torch.float32 [n_rows, nfft] on the device, rows
        row_first .. of segs_per_row half-overlapping Hann segments each, bins in ascending frequency (bin i: (i - nfft / 2) rate / nfft).
        segs_per_row=None: one row over everything the buffer holds (its first 65536 segments if it holds more); n_rows=None: every whole row from row_first on that the buffer
        holds.  Waits for torch's current stream before the launch and for the handle's stream after it"""
        import torch
        unit = {FMT_S16: 4, FMT_U8: 2, FMT_F32: 8}[sample_format]
        n_in = d_wide.numel() * d_wide.element_size() // unit
        hop = nfft // 2
        last = (in_first + n_in - hop) // hop                      # segments 0 .. last - 1 end inside the buffer
        if segs_per_row is None:
            if in_first or row_first:
                raise OfdmRxError("survey: segs_per_row=None surveys a buffer that starts at position 0, as row 0")
            segs_per_row, n_rows = min(max(last, 0), 65536), 1
        if n_rows is None:
            n_rows = last // max(segs_per_row, 1) - row_first
        out = torch.empty((max(n_rows, 0), nfft), dtype=torch.float32, device=d_wide.device)
        torch.cuda.current_stream(d_wide.device).synchronize()
        self._check(self._lib.ofdmrx_util_survey(self._h, d_wide.data_ptr(), sample_format, in_first, n_in, nfft, segs_per_row, row_first,
                                                 max(n_rows, 0), out.data_ptr()))
        self.synchronize()
        return out

    def survey_grid(self, d_wide, sample_format, decim, times_per_row=None, in_first=0, row_first=0, n_rows=None):
        """the grid survey: d_wide, a contiguous device tensor of interleaved I/Q of sample_format, holds the
        wideband positions in_first .. of a capture at decim x the handle's rate -> the mean power of every slot of the grid front
        end's bank, torch.float32 [n_rows, 2 decim] on the device in ascending slot order (index i: slot i - decim at (i - decim) rate
        / 2), rows row_first .. of times_per_row output times each (a multiple of 8).  times_per_row=None: one row over every whole
        group of 8 output times the buffer holds (its first 65536 times if it holds more); n_rows=None: every whole row from row_first
        on that the buffer holds.  decim may be a ratio - a pair (p, q) or a fractions.Fraction: the result is [n_rows, n_all], the slots
        of the grid front end at that ratio in ascending order from k_first.  Waits for torch's current stream
        before the launch and for the handle's stream after it"""
        import torch
        unit = {FMT_S16: 4, FMT_U8: 2, FMT_F32: 8}[sample_format]
        decim, q = _ratio(decim)
        if q is not None:
            return self._survey_grid_ratio(d_wide, sample_format, unit, decim, q, times_per_row, in_first, row_first, n_rows)
        n_in = d_wide.numel() * d_wide.element_size() // unit
        times = (in_first + n_in - 1) // max(decim, 1) + 1 if n_in else 0   # the output times 0 .. times - 1 end inside the buffer
        if times_per_row is None:
            if in_first or row_first:
                raise OfdmRxError("survey_grid: times_per_row=None surveys a buffer that starts at position 0, as row 0")
            times_per_row, n_rows = min(times // 8 * 8, 65536), 1
        if n_rows is None:
            n_rows = times // max(times_per_row, 1) - row_first
        out = torch.empty((max(n_rows, 0), 2 * max(decim, 0)), dtype=torch.float32, device=d_wide.device)
        torch.cuda.current_stream(d_wide.device).synchronize()
        self._check(self._lib.ofdmrx_util_survey_grid(self._h, d_wide.data_ptr(), sample_format, in_first, n_in, decim, times_per_row,
                                                      row_first, max(n_rows, 0), out.data_ptr()))
        self.synchronize()
        return out

    def _survey_grid_ratio(self, d_wide, sample_format, unit, p, q, times_per_row, in_first, row_first, n_rows):
        """survey_grid at the ratio p / q -> [n_rows, n_all]: output time n ends inside the buffer where
        (n p') // q' does, p' / q' the ratio in lowest terms"""
        import torch
        p, q, _, n_all = _grid_ratio(p, q)
        n_in = d_wide.numel() * d_wide.element_size() // unit
        times = ((in_first + n_in) * q - 1) // p + 1 if n_in else 0     # the n with (n p) // q <= in_first + n_in - 1
        if times_per_row is None:
            if in_first or row_first:
                raise OfdmRxError("survey_grid: times_per_row=None surveys a buffer that starts at position 0, as row 0")
            times_per_row, n_rows = min(times // 8 * 8, 65536), 1
        if n_rows is None:
            n_rows = times // max(times_per_row, 1) - row_first
        out = torch.empty((max(n_rows, 0), n_all), dtype=torch.float32, device=d_wide.device)
        torch.cuda.current_stream(d_wide.device).synchronize()
        self._check(self._lib.ofdmrx_util_survey_grid_ratio(self._h, d_wide.data_ptr(), sample_format, in_first, n_in, p, q, times_per_row,
                                                            row_first, max(n_rows, 0), out.data_ptr()))
        self.synchronize()
        return out

    def tx_frame_samples(self, mode=6):
        return int(self._lib.ofdmrx_frame_samples(self.sample_rate, mode))

    def encode_stream(self, payloads, mode=6, freq_off=2000, call_sign="ANONYMOUS", channels=1, bits=16):
        """host convenience (the `encode` CLI's call): payloads [count, 5380] uint8 -> one PCM stream [samples, channels]"""
        payloads = np.ascontiguousarray(payloads, dtype=np.uint8).reshape(-1, PAYLOAD_BYTES)
        count = payloads.shape[0]
        n = int(self._lib.ofdmrx_stream_samples(self.sample_rate, mode, count))
        if n < 0:
            raise OfdmRxError("bad mode / count")
        pcm = np.zeros((n, channels), np.int16 if bits == 16 else np.uint8)
        self._check(self._lib.ofdmrx_tx_encode_stream(self._h, _ptr(payloads), count, mode, freq_off, call_sign.encode(),
                                                      channels, bits, _ptr(pcm)))
        return pcm

    def tx_encode_streams(self, d_payload, n_streams, count, d_pcm, mode=6, freq_off=2000, call_sign="ANONYMOUS", channels=2, bits=16):
        """device transmitter, streams of `count` payloads: n_streams x count x 5380 payload bytes -> n_streams x
        ofdmrx_stream_samples(rate, mode, count) x channels samples of 8 (unsigned) or 16 bits (device pointers; asynchronous)"""
        self._check(self._lib.ofdmrx_tx_encode_stream_device(self._h, d_payload, n_streams, count, mode, freq_off, call_sign.encode(),
                                                             channels, bits, d_pcm))

    def tx_encode(self, d_payload, n, d_pcm, mode=6, freq_off=2000, call_sign="ANONYMOUS", channels=2):
        """device transmitter: n x 5380 payload bytes -> n x tx_frame_samples(mode) x channels int16 (device pointers)"""
        self._check(self._lib.ofdmrx_tx_encode_device(self._h, d_payload, n, mode, freq_off, call_sign.encode(), channels, d_pcm))


class Feed:
    """A recording decoded block by block (ofdmrx_feed_*): push(pcm) returns the records that have become due, end() the rest.
    The records of all calls, concatenated, are what Receiver.decode_stream returns for the concatenated samples.  One feed per
    Receiver at a time; a context manager ends (and discards what is left of) a feed that was not ended."""

    def __init__(self, rx, channels, dtype=np.int16, esn0_rows=False):
        self._rx, self._lib, self._h = rx, rx._lib, rx._h
        self.channels, self.dtype, self._rows = int(channels), np.dtype(dtype), bool(esn0_rows)
        rx._check(self._lib.ofdmrx_feed_begin(self._h, rx._fmt(self.dtype), self.channels))
        self.open = True
        self.n_left = 0

    @property
    def lag(self):
        return int(self._lib.ofdmrx_feed_lag(self._h))

    @property
    def resident_samples(self):
        return int(self._lib.ofdmrx_feed_resident_samples(self._h))

    def _call(self, f, max_frames, ending=False):
        """f(cap, payload, results, n_records, n_left) until nothing is left (max_frames None) or once"""
        pays, ress, rows = [], [], []
        cap = 16 if max_frames is None else int(max_frames)
        first = True
        while first or (max_frames is None and self.n_left > 0 and self.open):
            out = np.zeros((max(cap, 1), PAYLOAD_BYTES), np.uint8)
            res = np.zeros(max(cap, 1), RESULT_DTYPE)
            rw = np.zeros((max(cap, 1), 126), np.float32) if self._rows else None
            nrec, nleft = C.c_size_t(0), C.c_size_t(0)
            if self._rows:
                self._rx._check(self._lib.ofdmrx_set_esn0_rows(self._h, _ptr(rw)))
            try:
                self._rx._check(f(first, cap, _ptr(out) if cap else None, _ptr(res) if cap else None, C.byref(nrec), C.byref(nleft)))
            finally:
                if self._rows:
                    self._lib.ofdmrx_set_esn0_rows(self._h, None)
            first = False
            self.n_left = nleft.value
            pays.append(out[:nrec.value])
            ress.append(res[:nrec.value])
            if self._rows:
                rows.append(rw[:nrec.value])
            if ending and nleft.value == 0:
                self.open = False
        ret = (np.concatenate(pays), np.concatenate(ress))
        return ret + ((np.concatenate(rows),) if self._rows else ())

    def push(self, pcm, max_frames=None):
        """more samples [k, channels] (or [k] mono; k may be 0) -> (payloads, results[, esn0 rows]) of the records now due;
        max_frames None: everything that is ready (else the rest stays staged: n_left)"""
        pcm = np.ascontiguousarray(pcm, dtype=self.dtype).reshape(-1, self.channels)
        n = pcm.shape[0]
        return self._call(lambda first, cap, o, r, a, b: self._lib.ofdmrx_feed_push(self._h, _ptr(pcm) if n and first else None,
                                                                                   n if first else 0, cap, o, r, a, b), max_frames)

    def _end(self, first, cap, o, r, a, b):
        return self._lib.ofdmrx_feed_end(self._h, cap, o, r, a, b)

    def end(self, max_frames=None):
        """the stream is over -> the remaining records; the feed is closed once nothing is left"""
        return self._call(self._end, max_frames, ending=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        while self.open:
            self.end()
        return False


class Bank:
    """Many live channels pushed and decoded in one call (ofdmrx_bank_*): push(blocks) takes one block per channel and returns the
    records that have become due on any of them, end() the rest.  The records of channel c over all calls are what a Feed of that
    channel alone returns.  One bank per Receiver at a time, never beside a feed; a context manager ends a bank that was not ended."""

    def __init__(self, rx, n_channels, channels, dtype=np.int16, esn0_rows=False):
        self._rx, self._lib, self._h = rx, rx._lib, rx._h
        self.n_channels, self.channels, self.dtype, self._rows = int(n_channels), int(channels), np.dtype(dtype), bool(esn0_rows)
        rx._check(self._lib.ofdmrx_bank_begin(self._h, self.n_channels, rx._fmt(self.dtype), self.channels))
        self.open = True
        self.n_left = 0
        self._ops = 0

    def resident_samples(self, c):
        return int(self._lib.ofdmrx_bank_resident_samples(self._h, int(c)))

    def preambles(self, c):
        return int(self._lib.ofdmrx_bank_preambles(self._h, int(c)))

    @property
    def last_stage_ops(self):
        """launches + copies + synchronisations the bank's own stages enqueued in the last push / end (not the record pipeline's, and not
        those of the further calls that only drain staged records)"""
        return self._ops

    def _call(self, f, max_records, ending=False):
        """f(first, cap, payload, results, channel, index, n_records, n_left) until nothing is left (max_records None) or once"""
        pays, ress, chans, idxs, rows = [], [], [], [], []
        cap = 16 if max_records is None else int(max_records)
        first = True
        while first or (max_records is None and self.n_left > 0 and self.open):
            out = np.zeros((max(cap, 1), PAYLOAD_BYTES), np.uint8)
            res = np.zeros(max(cap, 1), RESULT_DTYPE)
            ch = np.zeros(max(cap, 1), np.int32)
            ix = np.zeros(max(cap, 1), np.int64)
            rw = np.zeros((max(cap, 1), 126), np.float32) if self._rows else None
            nrec, nleft = C.c_size_t(0), C.c_size_t(0)
            if self._rows:
                self._rx._check(self._lib.ofdmrx_set_esn0_rows(self._h, _ptr(rw)))
            try:
                self._rx._check(f(first, cap, _ptr(out) if cap else None, _ptr(res) if cap else None, _ptr(ch) if cap else None,
                                  _ptr(ix) if cap else None, C.byref(nrec), C.byref(nleft)))
            finally:
                if self._rows:
                    self._lib.ofdmrx_set_esn0_rows(self._h, None)
            if first and not (ending and nleft.value == 0):       # (an end call that leaves nothing has closed the bank)
                self._ops = int(self._lib.ofdmrx_bank_last_stage_ops(self._h))
            first = False
            self.n_left = nleft.value
            pays.append(out[:nrec.value])
            ress.append(res[:nrec.value])
            chans.append(ch[:nrec.value])
            idxs.append(ix[:nrec.value])
            if self._rows:
                rows.append(rw[:nrec.value])
            if ending and nleft.value == 0:
                self.open = False
        ret = (np.concatenate(pays), np.concatenate(ress), np.concatenate(chans), np.concatenate(idxs))
        return ret + ((np.concatenate(rows),) if self._rows else ())

    def push(self, blocks, ends=None, max_records=None):
        """one block [k, channels] (or [k] mono) per channel - None or an empty array: no samples for that channel; ends (nullable):
        per channel, true = its stream is over after this block -> (payloads, results, record_channel, record_index[, esn0 rows])"""
        if len(blocks) != self.n_channels:
            raise ValueError("one block per channel")
        arrs = [np.zeros((0, self.channels), self.dtype) if b is None else np.ascontiguousarray(b, dtype=self.dtype).reshape(-1, self.channels)
                for b in blocks]
        lens = np.array([a.shape[0] for a in arrs], dtype=np.uintp)
        longest = int(lens.max())
        buf = np.zeros((self.n_channels, max(longest, 1), self.channels), self.dtype)
        for c, a in enumerate(arrs):
            buf[c, :a.shape[0]] = a
        zero = np.zeros(self.n_channels, dtype=np.uintp)
        e = None if ends is None else np.ascontiguousarray(np.asarray(ends) != 0, dtype=np.uint8)
        if e is not None and e.shape != (self.n_channels,):
            raise ValueError("one end flag per channel")
        stride = buf.strides[0]
        return self._call(lambda first, cap, o, r, ch, ix, a, b: self._lib.ofdmrx_bank_push(
            self._h, _ptr(buf) if longest and first else None, stride, _ptr(lens if first else zero), _ptr(e) if e is not None and first else None,
            cap, o, r, ch, ix, a, b), max_records)

    def _end(self, first, cap, o, r, ch, ix, a, b):
        return self._lib.ofdmrx_bank_end(self._h, cap, o, r, ch, ix, a, b)

    def end(self, max_records=None):
        """every channel still open ends -> the remaining records; the bank is closed once nothing is left"""
        return self._call(self._end, max_records, ending=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        while self.open:
            self.end()
        return False


class WidebandBank(Bank):
    """A bank fed one wideband capture (ofdmrx_bank_begin_wideband / ofdmrx_bank_push_wideband): push(block) takes the next wideband
    sample frames [k, 2] and returns what Bank.push returns - the records that have become due on any channel.  The records of channel
    c are what Receiver.decode_stream returns for row c of Receiver.channelize over the whole capture, however it is cut."""

    def __init__(self, rx, centres_hz, decim, dtype=np.int16, esn0_rows=False):
        self._rx, self._lib, self._h = rx, rx._lib, rx._h
        f = np.ascontiguousarray(centres_hz, dtype=np.float64).reshape(-1)
        p, q = _ratio(decim)
        self.centres_hz, self.decim = f, p if q is None else (p, q)
        self.n_channels, self.channels, self.dtype, self._rows = f.size, 2, np.dtype(dtype), bool(esn0_rows)
        if q is None:
            rx._check(self._lib.ofdmrx_bank_begin_wideband(self._h, f.size, _ptr(f), p, rx._fmt(self.dtype)))
        else:
            rx._check(self._lib.ofdmrx_bank_begin_wideband_ratio(self._h, f.size, _ptr(f), p, q, rx._fmt(self.dtype)))
        self.open = True
        self.n_left = 0
        self._ops = 0

    def push(self, block, end=False, max_records=None):
        """more wideband samples [k, 2] (k may be 0); end: every channel's stream is over after them -> (payloads, results,
        record_channel, record_index[, esn0 rows])"""
        pcm = np.ascontiguousarray(block, dtype=self.dtype).reshape(-1, 2)
        n = pcm.shape[0]
        return self._call(lambda first, cap, o, r, ch, ix, a, b: self._lib.ofdmrx_bank_push_wideband(
            self._h, _ptr(pcm) if n and first else None, n if first else 0, 1 if end and first else 0, cap, o, r, ch, ix, a, b), max_records)


class WidebandRealBank(WidebandBank):
    """A wideband bank fed one REAL capture (ofdmrx_bank_begin_wideband_real): push(block) takes the next
    samples as a 1-D block; end and the queries are WidebandBank's.  The records of channel c are what Receiver.decode_stream returns
    for row c of Receiver.channelize_real over the whole capture, however it is cut."""

    def __init__(self, rx, centres_hz, decim, dtype=np.int16, esn0_rows=False):
        self._rx, self._lib, self._h = rx, rx._lib, rx._h
        f = np.ascontiguousarray(centres_hz, dtype=np.float64).reshape(-1)
        p, q = _ratio(decim)
        self.centres_hz, self.decim = f, p if q is None else (p, q)
        self.n_channels, self.channels, self.dtype, self._rows = f.size, 2, np.dtype(dtype), bool(esn0_rows)
        rx._check(self._lib.ofdmrx_bank_begin_wideband_real(self._h, f.size, _ptr(f), p, 1 if q is None else q, rx._fmt(self.dtype)))
        self.open = True
        self.n_left = 0
        self._ops = 0

    def push(self, block, end=False, max_records=None):
        """more real wideband samples, a 1-D block (it may be empty); end: every channel's stream is over after them -> what
        WidebandBank.push returns"""
        pcm = np.asarray(block)
        if pcm.ndim != 1:
            raise OfdmRxError("WidebandRealBank.push: a real capture arrives as a 1-D block, got shape %s" % (pcm.shape,))
        pcm = np.ascontiguousarray(pcm, dtype=self.dtype)
        n = pcm.shape[0]
        return self._call(lambda first, cap, o, r, ch, ix, a, b: self._lib.ofdmrx_bank_push_wideband(
            self._h, _ptr(pcm) if n and first else None, n if first else 0, 1 if end and first else 0, cap, o, r, ch, ix, a, b), max_records)


class WidebandGridBank(WidebandBank):
    """A wideband bank whose channels are slots of the grid front end (ofdmrx_bank_begin_wideband_grid): channel
    j is slot slots[j], centred at centres_hz[j]; push and end are WidebandBank's.  The records of channel j are what
    Receiver.decode_stream returns for row j of Receiver.channelize_grid over the whole capture, however it is cut."""

    def __init__(self, rx, slots, decim, dtype=np.int16, esn0_rows=False):
        self._rx, self._lib, self._h = rx, rx._lib, rx._h
        p, q = _ratio(decim)
        if q is not None:
            p, q, k = _grid_ratio_slots(p, q, slots)
            self.slots, self.decim, self.centres_hz = k, (p, q), k.astype(np.float64) * (float(rx.sample_rate) / 2.0)
            self.n_channels, self.channels, self.dtype, self._rows = k.size, 2, np.dtype(dtype), bool(esn0_rows)
            rx._check(self._lib.ofdmrx_bank_begin_wideband_grid_ratio(self._h, k.size, _ptr(k), p, q, rx._fmt(self.dtype)))
            self.open = True
            self.n_left = 0
            self._ops = 0
            return
        k = _grid_slots(decim, slots)
        self.slots, self.decim, self.centres_hz = k, int(decim), grid_centres(decim, rx.sample_rate, k)
        self.n_channels, self.channels, self.dtype, self._rows = k.size, 2, np.dtype(dtype), bool(esn0_rows)
        rx._check(self._lib.ofdmrx_bank_begin_wideband_grid(self._h, k.size, _ptr(k), self.decim, rx._fmt(self.dtype)))
        self.open = True
        self.n_left = 0
        self._ops = 0
