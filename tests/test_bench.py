"""bench.py's plain / --full split and --dump-outputs: the dump's sampling on the CPU, and one small plain
run on the GPU (its line carries the headline fields and none of the --full legs, its dump is the Gram)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    import importlib
    return importlib.import_module("bench")


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    bench = _bench()
    K = torch.arange(37 * 11, dtype=torch.float64).reshape(37, 11)
    info = bench.dump_outputs(str(tmp_path / "a"), K)
    got = np.load(tmp_path / "a" / "K.npy")
    assert got.dtype == np.float32 and info["K"]["rows"] == "all"
    np.testing.assert_array_equal(got, K.numpy().astype(np.float32))
    # above the byte budget: a sorted sample of whole rows, the same on every call
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 10 * 11 * 4 + 7)
    bench.dump_outputs(str(tmp_path / "b"), K)
    bench.dump_outputs(str(tmp_path / "c"), K)
    b, c = np.load(tmp_path / "b" / "K.npy"), np.load(tmp_path / "c" / "K.npy")
    assert b.shape == (10, 11) and b.nbytes <= bench.DUMP_MAX_BYTES
    np.testing.assert_array_equal(b, c)
    rows = (b[:, 0] / 11).astype(int)
    assert np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(b, K.numpy().astype(np.float32)[rows])


def test_dump_budget_is_under_64_mb():
    assert _bench().DUMP_MAX_BYTES <= 64 * 10**6


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_gram(tmp_path):
    import gpsig_amd
    n, l, d, m = 96, 128, 5, 5
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--nseq", str(n), "--dump-outputs", str(tmp_path / "out")]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["unit"] == "entries/s" and out["dtype"] == "f32" and out["higher_is_better"]
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(n * n / (out["ms_per_step"] / 1e3), rel=1e-9)
    assert out["breakdown"]["gram_launches"] == 1  # events of the 3 timed steps only
    for leg in ("max_abs_err", "cpu_baseline"):
        assert leg not in out
    assert out["roofline"]["peak_probe"] is None
    K = np.load(tmp_path / "out" / "K.npy")
    assert K.dtype == np.float32 and K.shape == (n, n)
    X = torch.as_tensor(_bench().synthetic(n, l, d).reshape(n, l * d), device="cuda:0")
    ref = gpsig_amd.SignatureRBF(l * d, d, m).K(X).cpu().numpy()
    # the project's parity criterion (norm-relative 1e-5 in fp32): K() and the bench step may differ in launch
    assert np.isfinite(K).all()
    assert np.abs(K.astype(np.float64) - ref).max() / np.abs(ref).max() < 1e-5
