"""The one-call stream decode's answers as its own driver and kernel forms gave them (tests/golden/stream_parent.json):
recorded on the GPU from the last commit in which ofdmrx_decode_stream* had a driver of its own (api_stream.cpp, the FrameBatch forms
of k_stream.hip) beside the batched entries, by tests/golden/gen_stream_parent.py.  Every field of every result record, the SHA-256
of every payload and n_preambles, per case; the case's input is held by its SHA-256."""
import functools
import hashlib
import json
import os

import numpy as np

import bank_inputs as B
import oracle_lib as O

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_parent.json")
INT_FIELDS = ("status", "symbol_pos", "sc_start", "oper_mode", "call_sign", "best_lane", "bit_flips", "n_sync_rejects")
FLOAT_FIELDS = ("cfo_rad", "cfo_fine", "sfo_slope", "esn0_db_last")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _mono(pcm):
    return np.ascontiguousarray(pcm[:, :1])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (rate, recording [samples, channels]): what the recorder hands to ofdmrx_decode_stream"""
    out = {}
    mixed = B.mixed(2)
    out["mixed_2ch"] = (8000, mixed)
    out["mixed_mono"] = (8000, B.mixed(1))
    pcm = O.impair(O.encode_pcm(O.payload_for(61, count=2), channels=2, rate=44100), noise_db=-30, seed=2, frame=0, rate=44100)
    out["two_44k_mono"] = (44100, _mono(pcm))                    # (the recording of feed_fixture's feed_44k_mono)
    out["one_48k_2ch"] = (48000, O.impair(O.encode_pcm(O.payload_for(60), channels=2, rate=48000), noise_db=-30, seed=2, frame=0, rate=48000))
    out["mixed_u8"] = (8000, ((mixed.astype(np.int32) >> 8) + 128).astype(np.uint8))
    out["mixed_f32"] = (8000, O.pcm_to_cf(mixed))
    # the other recordings of the batched calls that stand around a one-call decode on one handle (test_gpu_stream_parent.py)
    out["three_2ch"] = (8000, B.three())
    out["three_mono"] = (8000, _mono(B.three()))
    out["mirror_2ch"] = (8000, B.mixed(2, mirror=True))
    out["mirror_mono"] = (8000, B.mixed(1, mirror=True))
    return out


def encode(rate, pcm, got):
    """one case of the fixture from (payloads, results, n_preambles)"""
    out, res, npre = got
    records = []
    for k in range(len(res)):
        rec = {name: int(res[name][k]) for name in INT_FIELDS}
        rec.update({name: float(res[name][k]).hex() for name in FLOAT_FIELDS})
        rec["payload_sha256"] = _sha(out[k])
        records.append(rec)
    return {"rate": rate, "shape": list(pcm.shape), "dtype": str(pcm.dtype), "input_sha256": _sha(pcm), "n_preambles": int(npre), "records": records}


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(PATH) as f:
        return json.load(f)


def check(name, pcm, got):
    """(payloads, results, n_preambles) of a recording equal the recorded case byte for byte; the input is the recorded one"""
    import modem_amd.ofdmrx as M
    want = _fixture()["cases"][name]
    assert want["shape"] == list(pcm.shape) and want["dtype"] == str(pcm.dtype) and want["input_sha256"] == _sha(pcm), name
    out, res, npre = got
    assert int(npre) == want["n_preambles"], (name, int(npre), want["n_preambles"])
    assert len(res) == len(out) == len(want["records"]), (name, len(res), len(want["records"]))
    ref = np.zeros(len(res), M.RESULT_DTYPE)
    assert set(ref.dtype.names) == set(INT_FIELDS + FLOAT_FIELDS)
    for k, rec in enumerate(want["records"]):
        for f in INT_FIELDS:
            ref[f][k] = rec[f]
        for f in FLOAT_FIELDS:
            ref[f][k] = np.float32(float.fromhex(rec[f]))
        assert _sha(out[k]) == rec["payload_sha256"], (name, k)
    assert np.ascontiguousarray(res).tobytes() == ref.tobytes(), name
