"""The mono feed's answers as the single-window driver gave them (tests/golden/feed_mono_parent.json): recorded on the
GPU from the last commit that had a feed of its own beside the bank, by tests/golden/gen_feed_mono_parent.py.  Every field of every
result record and the SHA-256 of every payload, per case; the case's input is held by its SHA-256 and its push lengths."""
import functools
import hashlib
import itertools
import json
import os

import numpy as np

import bank_inputs as B
import oracle_lib as O

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feed_mono_parent.json")
INT_FIELDS = ("status", "symbol_pos", "sc_start", "oper_mode", "call_sign", "best_lane", "bit_flips", "n_sync_rejects")
FLOAT_FIELDS = ("cfo_rad", "cfo_fine", "sfo_slope", "esn0_db_last")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _runs(pushes):
    """the push lengths without the zero ones, as [length, how many in a row]"""
    return [[int(k), len(list(g))] for k, g in itertools.groupby(int(p) for p in pushes if p)]


def _pushes(n, block):
    return [min(block, n - a) for a in range(0, n, block)]


def cases():
    """name -> (rate, mono int16 samples, push lengths): what the recorder pushes through ofdmrx_feed_*"""
    out = {}
    mixed = B.mixed(1).reshape(-1)
    out["feed_mixed_mono"] = (8000, mixed, _pushes(len(mixed), 8000))
    pcm = O.impair(O.encode_pcm(O.payload_for(61, count=2), channels=2, rate=44100), noise_db=-30, seed=2, frame=0, rate=44100)
    two = np.ascontiguousarray(pcm[:, 0])
    out["feed_44k_mono"] = (44100, two, _pushes(len(two), 44100))
    chans = [np.concatenate([np.zeros(lead, np.int16), mixed]) for lead in (0, 1, 4097)]
    rounds = B.block_rounds([len(c) for c in chans], [8000, 4095, 7937])
    for c, ch in enumerate(chans):
        out["bank_mono_c%d" % c] = (8000, ch, [r[c] for r in rounds if r[c]])
    pcm = O.impair(O.encode_pcm(O.payload_for(61), channels=2, rate=44100), noise_db=-30, seed=2, frame=0, rate=44100)
    one = np.ascontiguousarray(pcm[:, 0])
    chans = [one, np.concatenate([np.zeros(4097, np.int16), one])]
    rounds = B.block_rounds([len(c) for c in chans], 44100)
    for c, ch in enumerate(chans):
        out["bank_44k_mono_c%d" % c] = (44100, ch, [r[c] for r in rounds if r[c]])
    return out


def encode(rate, samples, pushes, got):
    """one case of the fixture from (payloads, results)"""
    out, res = got
    records = []
    for k in range(len(res)):
        rec = {name: int(res[name][k]) for name in INT_FIELDS}
        rec.update({name: float(res[name][k]).hex() for name in FLOAT_FIELDS})
        rec["payload_sha256"] = _sha(out[k])
        records.append(rec)
    return {"rate": rate, "n_samples": len(samples), "input_sha256": _sha(samples), "pushes": _runs(pushes), "records": records}


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(PATH) as f:
        return json.load(f)


def check(name, samples, pushes, got):
    """(payloads, results) of a feed, or of one bank channel, equal the recorded case byte for byte; the input is the recorded one"""
    import modem_amd.ofdmrx as M
    want = _fixture()["cases"][name]
    samples = np.ascontiguousarray(samples).reshape(-1)
    assert want["n_samples"] == len(samples) and want["input_sha256"] == _sha(samples), name
    assert want["pushes"] == _runs(pushes), name
    out, res = got
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
