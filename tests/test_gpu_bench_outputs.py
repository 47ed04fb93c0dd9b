"""A plain `bench.py` run (no --full) is the headline alone -- no CPU baseline, no other workloads -- and `--dump-outputs DIR`
writes what the timed path computed in its last step: float arrays, within 64 MB, the sampled paths consistent with the
population's path lengths."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_the_headline_and_dumps_its_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "out"
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                         "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stderr[-2000:]
    d = json.loads([ln for ln in pr.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "evals/s" and d["dtype"] == "f64"
    assert d["higher_is_better"] is True and d["cpu_baseline"] is None and "extra" not in d
    z = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert {"stats", "path_len", "order", "path_agents", "path_cells"} <= set(z)
    assert all(a.dtype in (np.float32, np.float64) for a in z.values())
    assert sum(a.nbytes for a in z.values()) <= 64 << 20
    n = d["config"]["agents_per_gpu"]
    assert z["stats"].shape == (n, 5) and z["path_len"].shape == (n,) and sorted(z["order"]) == list(range(n))
    fit = z["stats"][z["order"].astype(int), 4]
    assert np.all(fit[1:] >= fit[:-1])                                            # the list is sorted by fitness
    ids = z["path_agents"].astype(int)
    assert len(ids) > 0 and z["path_cells"].size == int(z["path_len"][ids].sum())
