"""The device demodulator (modem_amd/csrc/k_demod.hip: the register transform and its radix-5/7 front split, the four-factor NCO,
the carrier placement, the parked previous carriers, the fused mono span recurrence; at 44.1 kHz what k_theil_sen forms from the
carriers) against the float64 model of demod_model.py and against the oracle, carrier by carrier: the GPU link of DESIGN.md
section 4.3, "What pins the demodulator".

The CONS_RAW tap of every record with status 0 or 6 is judged by demod_model.judge against the model fed with the DEVICE's own
sc_start and cfo_rad, under T = 4 x the oracle's measured worst distance (no device figure enters T).  Against the oracle's tap:
|g - o| <= T u + MEASURED u' + |c - c'| point by point, where c, u are the model and its unit at the device's parameters and c', u'
at the oracle's (the triangle inequality; the two models coincide when the parameters are bit-equal, and a point one side erases and
the other delivers must be an erasure tie of either model).  Handles have chunk_frames <= 64, so every record of a call sits in the
last chunk and the tap serves it.
"""
import numpy as np
import pytest

import demod_model as D
import oracle_lib as O
from demod_record import record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles():
    """one Receiver per (sample rate, keep_raw_cons), made when first asked for"""
    import modem_amd
    made = {}

    def get(rate=8000, keep_raw=False):
        if (rate, keep_raw) not in made:
            made[rate, keep_raw] = modem_amd.Receiver(device=0, chunk_frames=16, sample_rate=rate, keep_raw_cons=keep_raw)
        return made[rate, keep_raw]
    yield get
    for r in made.values():
        r.close()


def _row_quarters(d, rows):
    """worst finite d in each quarter of the rows: an NCO that degrades along the frame shows as a slope"""
    f = np.where(np.isfinite(d), d, 0.0).max(axis=1)
    q = [f[a:b].max() for a, b in zip(np.linspace(0, rows, 5).astype(int)[:-1], np.linspace(0, rows, 5).astype(int)[1:])]
    return "/".join("%.2f" % x for x in q)


def _hold(label, rx, k, pcm, rate, r, orc=None, z=None):
    """record k of the handle's last chunk against the model at the device's parameters, and against the oracle's tap of the same
    samples (orc: demod_model.OracleTap) -> the device's points [rows, cols] complex64"""
    assert int(r["status"]) in (0, 6), (label, int(r["status"]))
    mode = int(r["oper_mode"])
    cols, rows = D.geometry(mode)
    ch = pcm.shape[1]
    tol = D.T[ch]
    raw = rx.tap("CONS_RAW", k, cons_cnt=cols * rows)
    g = (raw[:, 0] + 1j * raw[:, 1]).reshape(rows, cols)
    z = D.analytic(pcm, rate) if z is None else z
    cfo = np.float32(r["cfo_rad"])
    m = D.demod(z, rate, mode, int(r["sc_start"]), cfo)
    v = D.judge(g, m, tol)
    quarters = _row_quarters(v.d, rows)
    record("gpu", "%s [rows by quarter %s]" % (label, quarters), v, tol)
    print("%s: worst %.3f median %.3f abs %.2e ties %d unexplained %d of %d, T %.2f, rows by quarter %s" % (
        label, v.worst, v.median, v.worst_abs, v.ties, v.unexplained, v.n, tol, quarters))
    assert D.accept(v), (label, v[:6])
    if orc is not None:
        assert orc.status in (0, 6) and orc.oper_mode == mode and orc.sc_start == int(r["sc_start"]), (label, orc[:4])
        assert abs(float(orc.cfo_rad) - float(cfo)) <= 2e-7, (label, orc.cfo_rad, cfo)
        mo = m if orc.cfo_rad == cfo else D.demod(z, rate, mode, orc.sc_start, orc.cfo_rad)
        o = np.asarray(orc.cons, np.float32).reshape(rows, cols, 2)
        o = o[..., 0] + 1j * o[..., 1]
        both = (g != 0) & (o != 0)
        bound = tol * m.u + D.MEASURED[ch] * mo.u + np.abs(m.raw - mo.raw)
        over = both & (np.abs(g - o) > bound)
        differ = (g == 0) != (o == 0)
        tie = differ & ((np.abs(np.abs(m.raw) - 2.0) <= tol * m.u) | (np.abs(np.abs(mo.raw) - 2.0) <= D.MEASURED[ch] * mo.u))
        print("%s: against the oracle: worst %.3e, beyond the bound %d, erased on one side %d" % (
            label, float(np.abs(g - o)[both].max()) if both.any() else 0.0, int(over.sum()), int(differ.sum())))
        assert not over.any() and not (differ & ~tie).any() and differ.sum() <= 2 * D.TIE_CAP * g.size, label
    return g.astype(np.complex64)


def _batch(frames):
    """frames [samples, channels] of one dtype -> [n, longest, channels], the shorter ones followed by silence (zeros; 128 for u8)"""
    n = max(f.shape[0] for f in frames)
    out = np.full((len(frames), n, frames[0].shape[1]), 128 if frames[0].dtype == np.uint8 else 0, frames[0].dtype)
    for k, f in enumerate(frames):
        out[k, :f.shape[0]] = f
    return out


def _run_cases(rx, names, pad=True):
    """the named cases of demod_model.cases() in ONE batch call (pad: the shorter frames followed by silence, which neither the model
    nor the oracle sees: for two channels silence is what lies outside a recording, for one the front end is causal and the data
    symbols end a second before the frame does), each record held against the model and the oracle"""
    cs = [D.case(n) for n in names]
    frames = [D.frame_of(c) for c in cs]
    assert pad or len({f.shape for f in frames}) == 1
    out, res = rx.decode(_batch(frames))
    got = []
    for k, c in enumerate(cs):
        assert int(res[k]["oper_mode"]) == c.mode
        got.append(_hold(c.name, rx, k, frames[k], c.rate, res[k], D.oracle_of(c), D.analytic_of(c)))
    return cs, res, got


# ---------------------------------------------------------------- every mode in one call
@pytest.mark.parametrize("keep_raw", [True, False], ids=["keep_raw_cons", "default"])
@pytest.mark.parametrize("level", ["clean", "list-1 level"])
def test_every_mode_in_one_batch(handles, level, keep_raw):
    """one frame of every mode 6 - 13 at its band edge: the mode differs per workgroup, cols 256 .. 512 put carriers on e = 1 where
    NT = 320, rows 42 .. 126 index symrot[] up to ROWS_MAX"""
    cs, res, _ = _run_cases(handles(8000, keep_raw), ["A mode %d %s" % (m, level) for m in range(6, 14)])
    assert sorted(D.geometry(c.mode) for c in cs)[0] == (256, 126) and max(D.geometry(c.mode)[0] for c in cs) == 512
    assert (res["status"] == 0).all()


# ---------------------------------------------------------------- the regimes
def test_cfo_sfo_multipath_waterfall(handles):
    """CFO of both signs, SFO, a three-tap fade, waterfall noise (9 % of the points erased); the rows' worst d by quarter is recorded"""
    _run_cases(handles(), [c.name for c in D.cases() if c.name[0] == "B"])


# ---------------------------------------------------------------- formats
def test_u8_and_f32(handles):
    for name in ("C mode 7 u8", "C mode 11 f32 -21 dB"):
        _run_cases(handles(), [name])


def test_f32_power_of_two_scaling_is_exact(handles):
    """the same f32 frame scaled by a power of two: every product, sum and quotient of the receiver scales exactly, so sc_start,
    cfo_rad and every point of cons are bit-identical to the unscaled frame's (zero tolerance).  Scaled DOWN the receiver is not
    scale-free: decode.cc:88 holds the Schmidl-Cox power at no less than 0.0001 per sample, this frame's is 0.008, and at 2^-20 and
    2^-40 the oracle finds no preamble - there the device must report the same, and no cons exist to compare.  Scaled UP nothing
    has a floor; the largest factor whose squared correlation sums stay inside fp32 is about 2^30.  So: 2^-2 (still above the
    floor), 2^12 and 2^24 bit-identical, 2^-20 and 2^-40 NO_SYNC like the oracle"""
    c = D.case("C mode 11 f32 -21 dB")
    x = D.frame_of(c)
    rx = handles()
    scales = (0, -2, 12, 24, -20, -40)
    out, res = rx.decode(np.stack([x * np.float32(2.0 ** e) for e in scales]))
    cols, rows = D.geometry(c.mode)
    taps = [rx.tap("CONS_RAW", k, cons_cnt=cols * rows) for k in range(4)]
    for k, e in enumerate(scales):
        assert int(res[k]["status"]) == O.decode(x * np.float32(2.0 ** e))[1].status == (0 if k < 4 else 1), e
    assert len(set(res["sc_start"][:4].tolist())) == 1 and len({res["cfo_rad"][k].tobytes() for k in range(4)}) == 1
    assert taps[0].any()
    for k in range(1, 4):
        assert taps[k].tobytes() == taps[0].tobytes(), scales[k]
    _hold(c.name + " (scaled batch)", rx, 0, x, c.rate, res[0], D.oracle_of(c), D.analytic_of(c))


# ---------------------------------------------------------------- cut-off and silent symbols
@pytest.mark.parametrize("name", [c.name for c in D.cases() if c.name[0] == "D"])
def test_cut_off_and_silent_symbols(handles, name):
    """exact zeros where the model says so (judge() leaves a non-zero point at u = 0 unexplained), in int16, u8 and f32; the frame
    is its own call, so a cut-off frame ends where its samples end"""
    cs, res, got = _run_cases(handles(), [name], pad=False)
    c, g = cs[0], got[0]
    m = D.demod(D.analytic_of(c), c.rate, c.mode, int(res[0]["sc_start"]), np.float32(res[0]["cfo_rad"]))
    dead = m.u == 0
    assert dead.any() and (g[dead] == 0).all()
    if c.silent is not None:
        assert dead[c.silent].all() and (g[c.silent:c.silent + 2] == 0).all()
    if c.cut:
        assert dead[-1].all() and (g[-1] == 0).all()


# ---------------------------------------------------------------- one channel at 8 kHz (k_demod<8000, 2>)
MONO_8K = [c.name for c in D.cases() if c.channels == 1 and c.rate == 8000]


@pytest.mark.parametrize("name", MONO_8K)
def test_mono_8k(handles, name):
    """int16 frames inside the frame (the packed loads), a cut-off frame (the clamped path), u8, f32, a DC offset"""
    assert {D.case(n).fmt for n in MONO_8K} == {"s16", "u8", "f32"} and any(D.case(n).cut for n in MONO_8K) and any(D.case(n).dc for n in MONO_8K)
    _run_cases(handles(), [name], pad=False)


def test_mono_8k_odd_samples_per_frame(handles):
    """two int16 frames of an odd number of samples each, the stride no more than that: frame 1 starts 2 bytes off a 4-byte boundary"""
    import modem_amd.ofdmrx as M
    rx = handles()
    a = D.case("F mono 8 kHz mode 6 clean")
    b = D.case("F mono 8 kHz mode 6 -20 dB cut off 16700 early")._replace(name="F mono 8 kHz mode 6 -20 dB", cut=0)
    fa, fb = D.frame_of(a), D.frame_of(b)
    spf = fa.shape[0] - 1                                                      # (a frame ends in a second of silence)
    assert spf % 2 == 1 and fb.shape == fa.shape
    buf = np.ascontiguousarray(np.stack([fa[:spf], fb[:spf]]))
    out, res = np.zeros((2, M.PAYLOAD_BYTES), np.uint8), np.zeros(2, M.RESULT_DTYPE)
    rx._check(rx._lib.ofdmrx_decode_batch(rx._h, M._ptr(buf), O.FMT_S16, 1, spf, spf * 2, 2, None, M._ptr(out), M._ptr(res)))
    assert (spf * 2) % 4 == 2 and buf.strides[0] == spf * 2
    for k in range(2):
        _hold("odd samples_per_frame, frame %d" % k, rx, k, buf[k], 8000, res[k], D.oracle_tap(buf[k], 8000))


# ---------------------------------------------------------------- the other rates
@pytest.mark.parametrize("channels", [2, 1])
@pytest.mark.parametrize("rate", [16000, 44100, 48000])
def test_other_rates(handles, rate, channels):
    """16 / 44.1 / 48 kHz, the CPU table's frames; at 44.1 kHz the tap is what k_theil_sen forms from the carriers"""
    names = [c.name for c in D.cases() if c.rate == rate and c.channels == channels]
    assert len(names) == (4 if channels == 2 else 2)
    _run_cases(handles(rate), names)


# ---------------------------------------------------------------- SourceBatch
def _recordings(rate, channels, modes, seed):
    """one recording per mode, two payloads each, lightly noisy: [samples, channels] int16"""
    recs = []
    for q, mode in enumerate(modes):
        off = D.TX.permitted_offsets(mode, rate, channels)[-1 if q % 2 else 0]
        pcm = O.encode_pcm(O.payload_for(8000 + seed + q, 2), channels=2, freq_off=off, call_sign=D.CALL_SIGN, mode=mode, rate=rate)
        pcm = O.impair(pcm, noise_db=-24.0, seed=seed, frame=q, rate=rate)
        recs.append(np.ascontiguousarray(pcm[:, :channels]))
    return recs


@pytest.mark.parametrize("rate,channels,modes", [(8000, 2, (6, 13, 10)), (8000, 1, (9, 10, 7)), (48000, 1, (10, 6, 11))],
                         ids=["8 kHz two channels", "8 kHz mono", "48 kHz mono"])
def test_decode_streams(handles, rate, channels, modes):
    """three recordings of different lengths, two payloads each, modes mixed; the padding behind each recording is another frame.
    Every record against the model run on its own recording at its stream sc_start, and against the oracle's decode of that
    recording with skip = the record's index"""
    import modem_amd.ofdmrx as M
    rx = handles(rate)
    recs = _recordings(rate, channels, modes, 31)
    lens = np.array([len(x) for x in recs], np.uintp)
    assert len(set(lens.tolist())) == 3
    pad = recs[0][rate:]                                                       # a frame with its preamble, right behind each recording
    stride = int(lens.max()) + len(pad)
    buf = np.zeros((3, stride, channels), np.int16)
    for q, x in enumerate(recs):
        buf[q, :len(x)] = x
        buf[q, len(x):] = np.concatenate([pad] * (stride // len(pad) + 1))[:stride - len(x)]
    out, res = np.zeros((8, M.PAYLOAD_BYTES), np.uint8), np.zeros(8, M.RESULT_DTYPE)
    npre, first = np.zeros(3, np.uintp), np.zeros(4, np.uintp)
    rx._check(rx._lib.ofdmrx_decode_streams(rx._h, M._ptr(buf), O.FMT_S16, channels, 3, stride * channels * 2, M._ptr(lens), 8, 8,
                                            M._ptr(out), M._ptr(res), M._ptr(npre), M._ptr(first)))
    assert npre.tolist() == [2, 2, 2] and first.tolist() == [0, 2, 4, 6] and rx.last_chunk_first_frame() == 0
    for q, x in enumerate(recs):
        z = D.analytic(x, rate)
        for i in range(2):
            k = 2 * q + i
            assert int(res[k]["status"]) == 0 and int(res[k]["oper_mode"]) == modes[q]
            _hold("decode_streams %d Hz %d ch, recording %d (mode %d) record %d" % (rate, channels, q, modes[q], i), rx, k, x, rate, res[k],
                  D.oracle_tap(x, rate, skip=i), z)


# ---------------------------------------------------------------- WindowBatch
def test_bank_of_two_channels_in_uneven_blocks(handles):
    """a bank of two live channels fed in uneven blocks: the records of the push that delivers them, tapped right after it, against
    the model run on the channel's whole stream at the record's stream sc_start"""
    rx = handles()
    chans = _recordings(8000, 2, (8, 11), 47)
    zs = [D.analytic(x, 8000) for x in chans]
    seen = [0, 0]
    with rx.bank(2, 2) as b:
        at = [0, 0]
        blocks = [(30011, 50000), (70001, 12345), (64000, 90000), (10 ** 7, 10 ** 7)]
        for r, sizes in enumerate(blocks + [None]):
            if sizes is None:
                ret = b.end(max_records=16)
            else:
                ret = b.push([chans[c][at[c]:at[c] + sizes[c]] for c in range(2)], max_records=16)
                at = [at[c] + sizes[c] for c in range(2)]
            pays, res, ch, ix = ret[:4]
            assert b.n_left == 0
            for k in range(len(res)):
                c, i = int(ch[k]), int(ix[k])
                assert int(res[k]["status"]) == 0 and i == seen[c]
                seen[c] += 1
                _hold("bank push %d, channel %d record %d" % (r, c, i), rx, k, chans[c], 8000, res[k], D.oracle_tap(chans[c], 8000, skip=i), zs[c])
    assert seen == [2, 2]
