"""-m gpu: bench.py's plain run -- the headline step alone -- and what --dump-outputs writes: the last timed step's outputs and
parameter gradients, the same from run to run on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + list(args), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    dumps = []
    for name in ("a", "b"):
        d = tmp_path / name
        line = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(d))
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["unit"] == "views/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert not {"step_8_views", "with_depth_gradient", "roofline_full", "cpu_baseline"} & set(line)
        assert "dynamic_stage_iters_per_sec" not in line["config"]
        files = sorted(os.listdir(d))
        assert {"color.npy", "depth.npy", "alpha.npy", "radii.npy"} <= set(files) and any(f.startswith("grad.") for f in files)
        arrays = {f: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert all(np.isfinite(a).all() for a in arrays.values())
        assert np.abs(arrays["color.npy"]).max() > 0 and any(np.abs(a).max() > 0 for f, a in arrays.items() if f.startswith("grad."))
        dumps.append(arrays)
    assert dumps[0].keys() == dumps[1].keys()
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f
