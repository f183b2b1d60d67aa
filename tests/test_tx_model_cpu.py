"""The transmitter's float64 model (tx_model.py) against the oracle encoder, on the CPU.

(a) the case-table helper: the permitted offsets of encode.cc:389 per (mode, rate, channels), and the table's cases at their edges.
(b) orc_encode_pcm_rate against the model on every stream of every case, sample by sample (noise_model.explain / accept), each
    comparison recorded; the oracle's worst boundary distance re-measured against the constant the tolerance is four times of.
(c) the comparison has teeth: every named wrong variant of the model is rejected by the same rule against the oracle's output.
"""
import numpy as np
import pytest

import noise_model as NM
import tx_model as T
from tx_record import record

CASES = {c.name: c for c in T.cases()}


@pytest.fixture(scope="module")
def oracle_pcm():
    """name -> (payloads [n_streams, count, 5380], [oracle PCM of each stream]); computed once, never written to"""
    out = {}
    for c in T.cases():
        pays = T.case_payloads(c)
        out[c.name] = (pays, [T.oracle_of(c, pays[s]) for s in range(c.n_streams)])
    return out


# ---------------------------------------------------------------- (a)
def test_permitted_offsets_are_encode_cc_389():
    """the condition of encode.cc:389 and 394, evaluated literally (C's integer halves), against the helper, for every mode, rate and
    channel count; and the edges the device tests name"""
    for mode, m in T.MODES.items():
        for rate in T.RATES:
            for channels in (1, 2):
                bw = m.band_width
                ok = [f for f in range(-rate, rate + 1, 50)
                      if not ((channels == 1 and f < bw // 2) or f < bw // 2 - rate // 2 or f > rate // 2 - bw // 2)]
                assert ok == T.permitted_offsets(mode, rate, channels) and len(ok) > 1
    edge = lambda mode, rate, ch, i: T.permitted_offsets(mode, rate, ch)[i]
    assert [edge(mode, 8000, 2, -1 if mode % 2 == 0 else 0) for mode in range(6, 14)] == [2650, -2750, 2750, -2850, 2400, -2800, 2800, -3200]
    assert (edge(6, 8000, 1, 0), edge(9, 8000, 1, -1), edge(10, 8000, 1, 0), edge(13, 8000, 1, -1)) == (1350, 2850, 1600, 3200)
    assert (edge(6, 16000, 1, 0), edge(11, 16000, 2, -1), edge(10, 44100, 2, 0), edge(13, 48000, 1, -1)) == (1350, 6800, -20450, 23200)
    assert 2000 in T.permitted_offsets(6, 8000, 1)                             # what bench.py and most of the suite transmit at


def test_case_table_is_inside_the_band_and_covers_the_scope():
    cs = T.cases()
    for c in cs:
        assert c.freq_off in T.permitted_offsets(c.mode, c.rate, c.channels), c
    assert {c.mode for c in cs} == set(range(6, 14)) and {c.rate for c in cs} == set(T.RATES)
    assert {(c.channels, c.bits) for c in cs} == {(1, 16), (2, 16), (1, 8), (2, 8)}
    assert any(c.count > 1 and c.n_streams > 1 for c in cs)
    for c in cs:                                                               # every payload of a case is distinct
        p = T.case_payloads(c).reshape(-1, 5380)
        assert len({bytes(x) for x in p}) == p.shape[0] == c.count * c.n_streams


def test_stream_lengths_and_silences():
    c = CASES["B mode 13 mono"]
    v = T.model_of(c, T.case_payloads(c)[0])
    assert v.shape == (T.stream_samples(c.rate, c.mode, c.count), 1)
    assert not v[:c.rate].any() and not v[-c.rate:].any() and v[c.rate + 1].any()
    c = CASES["C 16 kHz mode 11 8 bit"]
    v = T.model_of(c, T.case_payloads(c)[0])
    assert (v[:c.rate] == 128.0).all() and (v[-c.rate:] == 128.0).all() and v.min() >= 1.0 and v.max() <= 255.0


def test_shorten_removes_the_tail_of_the_code_word():
    """encode.cc:180-186 in both frozen tables: the positions removed are [cons_bits, 65536), all of them message positions past the
    CRC.  So a code word "taken without shortening" is the same prefix; the variant "tail message bits not fixed" therefore leaves
    those message bits unfixed instead (tx_model.code_bits)"""
    for mode, m in T.MODES.items():
        fz = T._frozen_bits(m.table)
        keep = fz | (np.cumsum(~fz) - 1 < T.CRC_BITS)
        assert keep[:m.cons_bits].all() and not keep[m.cons_bits:].any() and int((~fz).sum()) == m.mesg_bits


# ---------------------------------------------------------------- (b)
def test_oracle_encoder_matches_model_on_the_whole_case_table(oracle_pcm):
    """the rule holds on every comparison; the oracle alone stays below the cap (0.41 % at worst, 8PSK at 16 bit); its worst boundary
    distance is the figure in tx_model.py's header, and four times that figure is below a quarter LSB of 16 bit"""
    worst_fs, worst_share = 0.0, 0.0
    for c in T.cases():
        pays, refs = oracle_pcm[c.name]
        for s, ref in enumerate(refs):
            v = T.model_of(c, pays[s])
            assert v.shape == ref.shape
            res = NM.explain(ref, v, T.tol_lsb(c.bits))
            record("oracle", "%s, stream %d, %d Hz" % (c.name, s, c.freq_off), res, c.bits)
            assert NM.accept(res), (c, s, res)
            worst_fs, worst_share = max(worst_fs, res.worst * T.TOL_FS), max(worst_share, NM.share(res))
            if c.name == "C 48 kHz mode 13 mono":
                assert int(np.abs(ref.astype(np.int32)).max()) == 32767 and (np.abs(v) == 32767.0).any(), "the clamp is not reached"
    print("oracle: worst boundary distance %.3e of full scale, worst share %.4f %%" % (worst_fs, 100 * worst_share))
    assert 0.5 * T.MEASURED_FS <= worst_fs <= T.MEASURED_FS, worst_fs
    assert T.TOL_FS == 4.0 * T.MEASURED_FS and T.tol_lsb(16) < 0.25
    assert worst_share <= 0.5 * NM.CAP


# ---------------------------------------------------------------- (c)
TEETH_16 = [v for v in T.VARIANTS if v != "8-bit offset 127"]


@pytest.mark.parametrize("variant", T.VARIANTS)
def test_wrong_variants_of_the_model_are_rejected(oracle_pcm, variant):
    """8PSK and two channels; the 8-bit variant at 8 bit, the payload boundary in a stream of three payloads"""
    c = CASES[{"8-bit offset 127": "C 16 kHz mode 11 8 bit", "tail forgotten at a payload boundary": "D mode 12 count 3 x 2 streams"}.get(variant, "A mode 10")]
    pays, refs = oracle_pcm[c.name]
    res = NM.explain(refs[0], T.model_of(c, pays[0], variant), T.tol_lsb(c.bits))
    assert not NM.accept(res), (variant, res)
    assert res.unexplained > 0, (variant, res)


@pytest.mark.parametrize("variant", [v for v in TEETH_16 if v != "tail forgotten at a payload boundary"])
def test_wrong_variants_are_rejected_in_a_mono_qpsk_stream_too(oracle_pcm, variant):
    c = CASES["B mode 9 mono"]
    pays, refs = oracle_pcm[c.name]
    res = NM.explain(refs[0], T.model_of(c, pays[0], variant), T.tol_lsb(c.bits))
    assert not NM.accept(res) and res.unexplained > 0, (variant, res)


def test_variant_names_are_checked():
    c = CASES["B mode 13 mono"]
    with pytest.raises(AssertionError):
        T.model_of(c, T.case_payloads(c)[0], "no such variant")
