"""bench.py's two kinds of run: a plain run (set-up, warm-up, timed steps, --dump-outputs, the result line) and --full (everything
else it measures or checks).  The option parsing is checked on CPU; the plain line end to end on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.util import ROOT


def test_plain_run_is_the_default_and_full_is_opt_in():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "2"])
    assert not a.full and a.steps == 3 and a.warmup == 2 and a.dump_outputs is None
    assert bench.parse_args(["--full", "--no-pmc"]).full


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_without_the_extras(tmp_path):
    """A plain run prints the headline line and writes --dump-outputs; the CPU baseline, parity self-check, secondary lines,
    stand-alone / in-situ step and host enqueue measurements are left to --full."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "XG_FORCE_DIST"):
        env.pop(k, None)
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    o = json.loads(lines[0])
    assert o["metric"] == "decoder timesteps/sec (train fwd+bwd) at batch 128, MSRVTT 26x1536+1024"
    assert o["unit"] == "decoder timesteps/s" and o["higher_is_better"] is True and o["dtype"] == "f32"
    assert o["steps"] == 2 and o["warmup"] == 1 and o["ms_per_step"] > 0
    assert abs(o["value"] - 128 * 21 / (o["ms_per_step"] * 1e-3)) <= 1e-3 * o["value"]
    assert np.isfinite(o["final_loss"])
    for k in ("cpu_baseline", "parity", "parity_loss_delta", "secondary", "host_enqueue_ms_per_step", "comm"):
        assert k not in o, k
    assert set(o["roofline"]) == {"iteration"} and o["roofline"]["iteration"]["achieved"] > 0
    d = o["dump_outputs"]
    names = sorted(os.listdir(dump))
    assert len(names) == d["arrays"] and "loss.npy" in names
    assert np.isfinite(np.load(dump / "loss.npy")).all()
