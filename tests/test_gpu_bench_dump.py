"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` run times exactly K
steps of the C4 workload and writes what that step(K) call returned and left on the device; the
sections beside the headline stay out of it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_bench_dumps_the_timed_steps(tmp_path):
    from gpk.problems import make_solver
    W, K = 2, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K),
                        "--warmup", str(W), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == K and out["warmup"] == W and out["full"] is False
    assert out["unit"] == "iters/s" and out["dtype"] == "f64" and out["higher_is_better"] is True
    assert out["value"] == pytest.approx(1e3 / out["ms_per_step"])
    for key in ("roofline", "train_regime", "step1_per_call", "spd_inverse_gflops", "cpu_baseline",
                "cpu_baseline_1core", "large_factors", "sharded"):
        assert out[key] is None, key
    got = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["adam_mu", "adam_nu", "losses", "params"]
    assert all(v.dtype == np.float64 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64e6
    # the same problem (seed = rank 0) stepped W + K times here: the step is deterministic
    # (fixed-order reductions, no floating-point atomics), so the dump is bit for bit this state
    s = make_solver("C4", seed=0)
    try:
        s.step(W)
        losses = s.step(K)
        count, mu, nu = s.get_opt_state()
        flat = s.get_flat()
    finally:
        s.close()
    assert count == W + K and out["final_loss"] == losses[-1]
    print("max |dump - rerun|:", {k: float(np.max(np.abs(got[k] - v))) for k, v in
                                  (("losses", losses), ("params", flat), ("adam_mu", mu), ("adam_nu", nu))})
    assert got["losses"].shape == (K,) and np.array_equal(got["losses"], losses)
    assert np.array_equal(got["params"], flat)
    assert np.array_equal(got["adam_mu"], mu) and np.array_equal(got["adam_nu"], nu)
