"""The device transmitter (modem_amd/csrc/k_tx.hip behind ofdmrx_tx_encode_stream_device and its two callers) against the float64
model of tx_model.py and against the oracle encoder, sample by sample.

Against the model: noise_model.explain with tx_model's measured tolerance - nothing unexplained, at most 1 % of the samples off
rint(v) - and every comparison recorded (tx_record.py).  Against the oracle: at most 1 LSB apart, at most 2 x CAP of the samples
different (where the two differ, at least one of them is off rint(v), and each side is allowed CAP of those).  Every payload in a
call is distinct, and every offset of the cases A to C is a band edge of encode.cc:389.
"""

import numpy as np
import pytest

import noise_model as NM
import oracle_lib as O
import tx_model as T
from tx_record import record

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in T.cases()}
FILL16, FILL8 = 12345, 0x5A
E_ARG = -1


@pytest.fixture(scope="module")
def handles():
    """one Receiver per sample rate, made when first asked for"""
    import modem_amd
    made = {}

    def get(rate):
        if rate not in made:
            made[rate] = modem_amd.Receiver(device=0, chunk_frames=4, sample_rate=rate)
        return made[rate]
    yield get
    for r in made.values():
        r.close()


def _out(n_streams, samples, channels, bits):
    import torch
    return torch.full((n_streams, samples, channels), FILL16 if bits == 16 else FILL8, dtype=torch.int16 if bits == 16 else torch.uint8,
                      device="cuda:0")


def _prepare(rate, pays, mode, channels, bits):
    """the device buffers of one call: payloads uploaded, output filled with the pattern (on torch's stream: synchronize before use)"""
    import torch
    n_streams, count = pays.shape[:2]
    d_pay = torch.from_numpy(np.ascontiguousarray(pays)).to("cuda:0")
    return d_pay, _out(n_streams, T.stream_samples(rate, mode, count), channels, bits)


def _issue(rx, d_pay, d_pcm, mode, freq_off, channels, bits, call_sign=T.CALL_SIGN):
    """the library call alone, asynchronous on the handle's stream; one payload per stream at 16 bit goes through
    ofdmrx_tx_encode_device, everything else through the stream entry"""
    n_streams, count = d_pay.shape[:2]
    if count == 1 and bits == 16:
        rx.tx_encode(d_pay.data_ptr(), n_streams, d_pcm.data_ptr(), mode=mode, freq_off=freq_off, call_sign=call_sign, channels=channels)
    else:
        rx.tx_encode_streams(d_pay.data_ptr(), n_streams, count, d_pcm.data_ptr(), mode=mode, freq_off=freq_off, call_sign=call_sign,
                             channels=channels, bits=bits)


def _transmit(rx, pays, mode, freq_off, channels, bits):
    """pays [n_streams, count, 5380] -> device tensor [n_streams, samples, channels], finished"""
    import torch
    d_pay, d_pcm = _prepare(rx.sample_rate, pays, mode, channels, bits)
    torch.cuda.synchronize()                                                   # the handle has a stream of its own
    _issue(rx, d_pay, d_pcm, mode, freq_off, channels, bits)
    rx.synchronize()
    return d_pcm, d_pay


def _hold(case, label, got, pays):
    """one stream against the model (the rule, recorded) and against the oracle encoder"""
    v = T.model_of(case, pays)
    assert got.shape == v.shape, (label, got.shape, v.shape)
    res = NM.explain(got, v, T.tol_lsb(case.bits))
    record("gpu", label, res, case.bits)
    ref = T.oracle_of(case, pays)
    lsb, differing = NM.lsb_apart(got, ref)
    print("%s: off rint(v) %.4f %%, unexplained %d, worst %.3f tol; off the oracle %.4f %%, %d LSB" % (
        label, 100 * NM.share(res), res.unexplained, res.worst, 100 * differing, lsb))
    assert NM.accept(res), (label, res)
    assert lsb <= 1 and differing <= 2 * NM.CAP, (label, lsb, differing)
    return ref


def _run_case(handles, case):
    pays = T.case_payloads(case)
    d_pcm, _ = _transmit(handles(case.rate), pays, case.mode, case.freq_off, case.channels, case.bits)
    got = d_pcm.cpu().numpy()
    refs = [_hold(case, "%s, stream %d, %d Hz" % (case.name, s, case.freq_off), got[s], pays[s]) for s in range(case.n_streams)]
    return pays, got, refs


# ---------------------------------------------------------------- A
@pytest.mark.parametrize("mode", range(6, 14))
def test_every_mode_at_a_band_edge(handles, mode):
    """8 kHz, 2 channels, 16 bit, two frames per call; even modes at the upper edge, odd modes at the lower one; frame 1 decodes on
    both sides"""
    case = CASES["A mode %d" % mode]
    assert case.freq_off == (2650, -2750, 2750, -2850, 2400, -2800, 2800, -3200)[mode - 6]
    pays, got, _ = _run_case(handles, case)
    o, r = O.decode(got[1])
    assert r.status == 0 and (o == pays[1, 0]).all() and r.oper_mode == mode and r.call_sign == O.lib().orc_base37_encode(T.CALL_SIGN.encode())
    out, res = handles(8000).decode(got)
    assert (res["status"] == 0).all() and (out == pays[:, 0]).all() and (res["oper_mode"] == mode).all()


# ---------------------------------------------------------------- B, C
@pytest.mark.parametrize("name", [n for n in CASES if n[0] in "BC"])
def test_mono_edges_and_other_rates(handles, name):
    """B: mono at 8 kHz, the lowest carrier at 0 Hz (modes 6, 10) or the highest at Nyquist (modes 9, 13).  C: 16 / 44.1 / 48 kHz, one
    case at 8 bit; the 48 kHz case reaches the quantiser's clamp"""
    case = CASES[name]
    assert case.freq_off in (T.permitted_offsets(case.mode, case.rate, case.channels)[0], T.permitted_offsets(case.mode, case.rate, case.channels)[-1])
    _, got, refs = _run_case(handles, case)
    if name == "C 48 kHz mode 13 mono":
        assert int(np.abs(got.astype(np.int32)).max()) == 32767 and int(np.abs(refs[0].astype(np.int32)).max()) == 32767
    assert got.astype(np.int32).min() >= (-32767 if case.bits == 16 else 1)


# ---------------------------------------------------------------- D
@pytest.mark.parametrize("name", [n for n in CASES if n[0] == "D"])
def test_streams_of_several_payloads(handles, name):
    """several streams of several payloads each: stream 0 makes the pilot, Schmidl-Cox, meta-data and zero symbols that every other
    stream's cross-fade reads (tx_symbol_slot); every stream against the model of its own payloads.  The 48 kHz case is the
    global-scratch path with count > 1"""
    case = CASES[name]
    assert case.count > 1 and case.n_streams > 1
    pays, got, _ = _run_case(handles, case)
    if name == "D mode 12 count 3 x 2 streams":                                # the host entry: byte-equal to the device entry
        host = handles(case.rate).encode_stream(pays[0], mode=case.mode, freq_off=case.freq_off, call_sign=T.CALL_SIGN,
                                                channels=case.channels, bits=case.bits)
        assert host.dtype == got.dtype and (host == got[0]).all()


# ---------------------------------------------------------------- E
def test_launch_split_with_several_payloads_per_stream(handles):
    """8 kHz, mode 6, count 2, 513 streams: the budget of 1024 payloads gives 512 streams per launch, so stream 512 is a launch of its
    own whose payload and output pointers are offset by 512 streams.  Streams 0, 511 and 512 carry payloads of their own; the others
    repeat stream 0's and must equal it byte for byte.  (350 MB of output.  The same split at 44.1 / 48 kHz needs 1.4 GB of PAPR
    scratch for the same host loop and is left out.)"""
    import torch
    case = T.Case("E mode 6 count 2 x 513 streams", 8000, 6, 2, 16, 2000, 2, 513, 501)
    own = {0: 0, 511: 1, 512: 2}
    distinct = T.case_payloads(case._replace(n_streams=3))
    pays = np.repeat(distinct[:1], case.n_streams, axis=0)
    for s, k in own.items():
        pays[s] = distinct[k]
    d_pcm, _ = _transmit(handles(8000), pays, case.mode, case.freq_off, case.channels, case.bits)
    for s in own:
        _hold(case, "%s, stream %d, %d Hz" % (case.name, s, case.freq_off), d_pcm[s].cpu().numpy(), pays[s])
    for s in range(1, 511):                                                    # compared on the device, stream by stream
        assert torch.equal(d_pcm[s], d_pcm[0]), s
    assert not torch.equal(d_pcm[511], d_pcm[0]) and not torch.equal(d_pcm[512], d_pcm[0]) and not torch.equal(d_pcm[512], d_pcm[511])


# ---------------------------------------------------------------- F
def test_scratch_reuse_and_growth(handles):
    """one handle runs a small call, a large one (its scratch grows) and the small one again.  Every buffer of the three calls is
    allocated and filled first and torch is synchronized once; then the three library calls are issued back to back with nothing in
    between, and the handle is synchronized only after the third: each result is what a fresh handle gives, and the large one is
    what the model says.  What this can see: an ordering error between back-to-back calls that share scratch (the large call and the
    second small one), and wrong bytes after a growth.  What it cannot: the entry's own hipStreamSynchronize before it replaces a
    buffer - the hipFree inside the replacement waits for the device anyway, so the result is the same without it"""
    import torch
    import modem_amd
    small_case = CASES["B mode 13 mono"]
    large_case = T.Case("F mode 10 count 3 x 4 streams", 8000, 10, 2, 16, -1000, 3, 4, 601)
    calls = [(c, T.case_payloads(c)) for c in (small_case, large_case, small_case)]
    bufs = [_prepare(8000, pays, c.mode, c.channels, c.bits) for c, pays in calls]
    rx = modem_amd.Receiver(device=0, chunk_frames=1)
    try:
        torch.cuda.synchronize()
        for (c, _), (d_pay, d_pcm) in zip(calls, bufs):
            _issue(rx, d_pay, d_pcm, c.mode, c.freq_off, c.channels, c.bits)
        rx.synchronize()
    finally:
        rx.close()
    (_, a), (_, b), (_, third) = bufs
    assert torch.equal(a, third)                                               # the same call twice
    for (c, pays), got in ((calls[0], a), (calls[1], b)):
        fresh = modem_amd.Receiver(device=0, chunk_frames=1)
        try:
            want, _ = _transmit(fresh, pays, c.mode, c.freq_off, c.channels, c.bits)
        finally:
            fresh.close()
        assert torch.equal(got, want)
    assert (a != FILL16).any() and (b != FILL16).any()
    _hold(large_case, "%s, stream 3, %d Hz" % (large_case.name, large_case.freq_off), b[3].cpu().numpy(), calls[1][1][3])


# ---------------------------------------------------------------- G
def _refused(lib, rx, d_pay, d_pcm, n_streams=1, count=1, mode=6, freq_off=2000, call_sign=b"REFUSED", channels=2, bits=16, h=True):
    return lib.ofdmrx_tx_encode_stream_device(rx._h if h else None, d_pay, n_streams, count, mode, freq_off, call_sign, channels, bits, d_pcm)


@pytest.mark.parametrize("rate", [8000, 48000])
def test_refusals_leave_the_output_untouched(handles, rate):
    """every argument main() refuses (encode.cc:353, 358, 389, 394) and every one the entry cannot work with: OFDMRX_E_ARG, nothing
    launched, the output's fill pattern intact.  The band edges for one and for two channels, one step of 50 outside, through all
    three entries"""
    import torch
    rx = handles(rate)
    lib = rx._lib
    pays = O.payload_for(700, 2).reshape(1, 2, O.DATA_BYTES)
    d_pay = torch.from_numpy(pays).to("cuda:0")
    d_pcm = _out(1, T.stream_samples(rate, 13, 1), 2, 16)                      # mode 13 has the most rows: room for any mode's one-payload stream
    before = d_pcm.clone()
    torch.cuda.synchronize()
    p, q = d_pay.data_ptr(), d_pcm.data_ptr()
    limit = 129961739795077                                                    # encode.cc:358: 37^9, "0" followed by nine blanks
    at, past = b"0" + b" " * 9, b"0" + b" " * 8 + b"0"
    assert (O.lib().orc_base37_encode(b"ZZZZZZZZZ"), O.lib().orc_base37_encode(at), O.lib().orc_base37_encode(past)) == (limit - 1, limit, limit + 1)
    bad = [dict(mode=5), dict(mode=14), dict(freq_off=2025), dict(count=0), dict(count=4097), dict(bits=12), dict(channels=0),
           dict(channels=3), dict(call_sign=b""), dict(call_sign=b"!!"), dict(call_sign=at), dict(call_sign=past), dict(n_streams=0),
           dict(h=False), dict(call_sign=None)]
    for kw in bad:
        assert _refused(lib, rx, p, q, **kw) == E_ARG, kw
    assert _refused(lib, rx, None, q) == E_ARG and _refused(lib, rx, p, None) == E_ARG
    host_out = np.full((T.stream_samples(rate, 13, 1), 2), FILL16, np.int16)   # room for any mode, like d_pcm
    for mode in range(6, 14):
        for channels in (1, 2):
            ok = T.permitted_offsets(mode, rate, channels)
            for f in (ok[0] - 50, ok[-1] + 50):
                assert _refused(lib, rx, p, q, mode=mode, freq_off=f, channels=channels) == E_ARG, (mode, channels, f)
                assert lib.ofdmrx_tx_encode_device(rx._h, p, 1, mode, f, b"REFUSED", channels, q) == E_ARG
                assert lib.ofdmrx_tx_encode_stream(rx._h, O.ptr(pays), 1, mode, f, b"REFUSED", channels, 16, O.ptr(host_out)) == E_ARG
    rx.synchronize()
    assert torch.equal(d_pcm, before) and (host_out == FILL16).all()
    assert _refused(lib, rx, p, q, call_sign=b"ZZZZZZZZZ") == 0                # the largest call sign, and the edges themselves, pass
    for channels in (1, 2):
        ok = T.permitted_offsets(13, rate, channels)
        for f in (ok[0], ok[-1]):
            assert _refused(lib, rx, p, q, mode=13, freq_off=f, channels=channels) == 0
    rx.synchronize()
    assert not torch.equal(d_pcm, before)
