"""bench.py's command line: --dump-outputs (what the timed path returned in its last step) and the plain run next to --full."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_cli_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _records(n, seed):
    import modem_amd.ofdmrx as M
    rng = np.random.default_rng(seed)
    res = np.zeros(n, M.RESULT_DTYPE)
    for name in res.dtype.names:
        res[name] = rng.integers(0, 1 << 20, n)
    res["sc_start"] += 190400 * np.arange(n) + (1 << 40)          # beyond float32's exact integers
    res["call_sign"] += (1 << 50) + 3
    return res


def test_dump_outputs_sample_is_fixed_and_exact(tmp_path, monkeypatch):
    """float32 / float64 only; the same sample of frames on every call; payload bytes and result fields exact; the record sample
    kicks in above DUMP_RESULT_FRAMES; at the headline's batch a dump stays under 64 MB"""
    b = _bench_module()
    monkeypatch.setattr(b, "DUMP_RESULT_FRAMES", 1000)
    n = 3000
    pay = np.random.default_rng(1).integers(0, 256, (n, 5380), dtype=np.uint8)
    res = _records(n, 2)
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        b.dump_outputs(str(d), pay, res)
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert {"payload.npy", "payload_frames.npy", "result_frames.npy", "result_status.npy", "result_sc_start.npy"} <= set(names)
    got = {}
    for nm in names:
        x, y = np.load(dirs[0] / nm), np.load(dirs[1] / nm)
        assert x.dtype in (np.float32, np.float64), nm
        assert x.dtype == y.dtype and (x == y).all(), nm
        got[nm[:-4]] = x
    pick = got["payload_frames"].astype(np.int64)
    assert len(pick) == min(n, b.DUMP_PAYLOAD_FRAMES) and (np.diff(pick) > 0).all()
    assert (got["payload"] == pay[pick]).all()
    rows = got["result_frames"].astype(np.int64)
    assert len(rows) == 1000 and (np.diff(rows) > 0).all()
    for name in res.dtype.names:
        assert (got["result_" + name] == res[name][rows]).all(), name
    # the headline batch: 65536 frames
    per_record = sum(8 if res.dtype[name].itemsize == 8 else 4 for name in res.dtype.names) + 8
    total = b.DUMP_PAYLOAD_FRAMES * (5380 * 4 + 8) + 65536 * per_record
    assert total <= 64 * 2 ** 20


def _run_bench(args, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "MODEM_AMD_NO_TORCH"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return lines[0]


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    """two plain runs with the same arguments: the headline fields, --steps timed steps, none of the --full figures, and
    identical dumps (the inputs are seeded, the outputs deterministic)"""
    n = 4096
    lines = []
    for d in ("a", "b"):
        lines.append(_run_bench(["--gpus", "1", "--frames", str(n), "--steps", "3", "--warmup", "1",
                                 "--dump-outputs", str(tmp_path / d)]))
    for ln in lines:
        assert ln["steps"] == 3 and ln["warmup"] == 1 and ln["ms_per_step"] > 0 and ln["value"] > 0
        assert ln["unit"] == "frames/s" and ln["higher_is_better"] is True and ln["dtype"] == "f32"
        assert ln["frames"] == n and ln["frames_ok"] == n and ln["fer"] == 0.0
        assert abs(ln["value"] - n * 3 / (ln["ms_per_step"] * 3 / 1e3)) <= 1e-6 * ln["value"]
        for k in ("value_kernel_only", "value_scl_forced", "value_host", "roofline", "cpu_baseline", "value_config3"):
            assert k not in ln, k
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "payload.npy" in names
    assert sum(os.path.getsize(tmp_path / "a" / nm) for nm in names) <= 64 * 2 ** 20
    real = {"result_cfo_rad.npy", "result_cfo_fine.npy", "result_sfo_slope.npy", "result_esn0_db_last.npy"}
    for nm in names:
        x, y = np.load(tmp_path / "a" / nm), np.load(tmp_path / "b" / nm)
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape, nm
        if nm in real:
            assert np.allclose(x, y, rtol=1e-6, atol=0, equal_nan=True), nm
        else:
            assert (x == y).all(), nm
    assert np.load(tmp_path / "a" / "payload.npy").shape == (min(n, 2048), 5380)
    assert (np.load(tmp_path / "a" / "result_status.npy") == 0).all()
