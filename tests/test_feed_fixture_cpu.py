"""tests/golden/feed_mono_parent.json (feed_fixture.py): the recorded cases are the inputs the GPU tests push - made by the CPU
oracle's encoder and seeded numpy, so the same on every machine - and every record is complete."""
import json

import feed_fixture as F


def test_fixture_inputs_and_records():
    with open(F.PATH) as f:
        fx = json.load(f)
    assert len(fx["recorded_from_commit"]) == 40
    cases = F.cases()
    assert sorted(fx["cases"]) == sorted(cases)
    for name, (rate, samples, pushes) in cases.items():
        want = fx["cases"][name]
        assert want["rate"] == rate and want["n_samples"] == len(samples) and want["input_sha256"] == F._sha(samples), name
        assert want["pushes"] == F._runs(pushes) and sum(k * n for k, n in want["pushes"]) == len(samples), name
        assert len(want["records"]) >= 1
        for rec in want["records"]:
            assert sorted(rec) == sorted(F.INT_FIELDS + F.FLOAT_FIELDS + ("payload_sha256",)), name
            assert len(rec["payload_sha256"]) == 64 and all(float.fromhex(rec[k]) == float.fromhex(rec[k]) for k in F.FLOAT_FIELDS)
