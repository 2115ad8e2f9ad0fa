"""bench.py as a command on the GPU, at a tiny shape (one slot, two 64-DV
batches per launch): a plain run times exactly --steps steps, prints the one
result line without the side measurements of --full, and --dump-outputs
writes the last timed step's outputs -- valid partials, aggregated duties."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_KEYS = ("api_pipeline", "small_batch_latency", "isolated_batch_ms", "isolated_kernel_ms", "roofline",
             "roofline_pipeline", "cpu_baseline", "host_signing_roots")


def test_plain_run_line_and_dumped_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dvs", "64", "--inflight", "1", "--merge", "2", "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["ms_per_step"] > 0 and d["higher_is_better"] is True
    # value and ms_per_step state the same measurement: 64 DV-duties per step
    assert abs(d["value"] - 64 * 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]
    assert not [k for k in SIDE_KEYS if k in d]
    assert d["ranks_exact_after_clock"] == [{"rank": 0, "device": 0, "exact": True}]
    ps, ds, agg = (np.load(out / (n + ".npy")) for n in ("partial_status", "duty_status", "agg"))
    assert ps.dtype == ds.dtype == agg.dtype == np.float32
    assert ps.shape == (256,) and ds.shape == (64,) and agg.shape == (64, 96)
    assert (ps == 1).all() and (ds == 0).all()       # PS_VALID, DS_OK
    assert ((agg[:, 0].astype(np.uint8) & 0x80) != 0).all()  # compressed G2 points
    assert len(np.unique(agg, axis=0)) == 64
