#!/usr/bin/env python
"""Wall times of mesh extraction from Gaussians on the device ("Mesh extraction from Gaussians").

    python tools/isosurface_timing.py [--out DIR]        every step in a child process under its own `timeout`; the first step
                                                         that fails ends the run (nothing more is started on the device)
    python tools/isosurface_timing.py --step device | trace --resolution R      one step, in this process

The scene: N = 200 k Gaussians on a bumpy closed surface, standard deviations of 0.4 .. 1.2 % of its extent, random
orientations, anisotropy up to 3:1, with colours; num_blocks = 16.  Steps, per resolution (128 and 256):
* device: after one warm-up call of every shape, the median over `runs` of the whole ``gaussian_density_field`` call and the
  whole ``marching_cubes`` call (host clock around a call that ends in a device synchronise: these include the sort, the prefix
  sums and the host visits for the counts), and of the field kernel alone (device events around ``dm4d_iso_density_field``),
  from which the pair rate follows: one pair evaluation = one (Gaussian, voxel) pair = n_pairs * (R / num_blocks)^3 per call;
* trace: the device step under ``rocprofv3 --kernel-trace --stats``: per-kernel times of the ``k_iso_*`` / ``k_mc_*`` kernels and
  the largest torch kernels between them.
One JSON line per step.  Needs a HIP device.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dreammesh4d_amd import _lib, isosurface as iso  # noqa: E402

# v_exp_f32 issues once per 8 cycles per SIMD for a 64-lane wave: 8 lanes / cycle / SIMD, 1024 SIMDs, 2.4 GHz
CHIP_EXP_PER_SECOND = 8 * 1024 * 2.4e9


def scene(n, seed=0):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = 0.5 + 0.08 * np.sin(5 * d[:, 0:1]) * np.cos(4 * d[:, 1:2]) + 0.05 * np.sin(7 * d[:, 2:3])
    sigma = rng.uniform(0.004, 0.012, (n, 1)) * np.exp(rng.uniform(0, np.log(3.0), (n, 3)))
    g = {"xyz": d * r * np.array([1.0, 0.8, 0.6]), "scaling": sigma, "rotation": rng.normal(size=(n, 4)),
         "opacity": rng.uniform(0.05, 1.0, n), "rgb": rng.uniform(0, 1, (n, 3))}
    return {k: torch.from_numpy(v.astype(np.float32)).cuda() for k, v in g.items()}


def device_step(n, R, num_blocks, thresh, runs):
    if not torch.cuda.is_available():
        sys.exit("isosurface_timing: no HIP device; a timing taken anywhere else says nothing")
    g = scene(n)
    kernel_ms = []
    call = _lib.call

    def timed_call(name, *a):
        if name != "dm4d_iso_density_field":
            return call(name, *a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = call(name, *a)
        e1.record()
        e1.synchronize()
        kernel_ms.append(e0.elapsed_time(e1))
        return rc

    _lib.call = timed_call
    run_field = lambda: iso.gaussian_density_field(g["xyz"], g["scaling"], g["rotation"], g["opacity"], g["rgb"], resolution=R,
                                                   num_blocks=num_blocks)
    field = run_field()                                       # warm-up of every shape
    iso.marching_cubes(field["occ"], thresh, field["csum"])
    torch.cuda.synchronize()
    kernel_ms.clear()
    t_field, t_mc = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        field = run_field()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        mesh = iso.marching_cubes(field["occ"], thresh, field["csum"])
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_field.append((t1 - t0) * 1e3)
        t_mc.append((t2 - t1) * 1e3)
    k = statistics.median(kernel_ms)
    evals = field["n_pairs"] * (R // num_blocks) ** 3
    return {"step": "device", "device": torch.cuda.get_device_name(0), "n": n, "n_kept": field["n_kept"], "resolution": R,
            "num_blocks": num_blocks, "runs": runs, "n_pairs": field["n_pairs"], "pair_evaluations": evals,
            "field_call_ms": round(statistics.median(t_field), 3), "field_call_ms_min_max": [round(min(t_field), 3), round(max(t_field), 3)],
            "field_kernel_ms": round(k, 3), "field_kernel_ms_min_max": [round(min(kernel_ms), 3), round(max(kernel_ms), 3)],
            "marching_cubes_call_ms": round(statistics.median(t_mc), 3),
            "marching_cubes_call_ms_min_max": [round(min(t_mc), 3), round(max(t_mc), 3)],
            "pair_evaluations_per_second": evals / (k * 1e-3), "share_of_chip_exp_rate": evals / (k * 1e-3) / CHIP_EXP_PER_SECOND,
            "vertices": int(mesh["verts"].shape[0]), "faces": int(mesh["faces"].shape[0])}


def trace_step(out_dir, n, R, runs):
    """The device step under rocprofv3 (the program goes after `--`); per-kernel totals divided by the number of calls."""
    d = os.path.join(out_dir, f"isosurface_trace_{R}")
    calls = runs + 1
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "isosurface", "--",
           sys.executable, os.path.abspath(__file__), "--step", "device", "--resolution", str(R), "--n", str(n), "--runs", str(runs)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    path = sorted(glob.glob(os.path.join(d, "**", "isosurface_kernel_stats.csv"), recursive=True))[0]
    rows = list(csv.DictReader(open(path)))
    mine = lambda r: "k_iso_" in r["Name"] or "k_mc_" in r["Name"]
    ours = {r["Name"].split("(")[0]: {"calls_per_run": int(r["Calls"]) / calls, "us_per_run": round(float(r["TotalDurationNs"]) / calls / 1e3, 2)}
            for r in rows if mine(r)}
    rest = sorted((r for r in rows if not mine(r)), key=lambda r: -float(r["TotalDurationNs"]))
    return {"step": "trace", "resolution": R, "calls": calls, "kernel_us_per_run_all": round(sum(float(r["TotalDurationNs"]) for r in rows) / calls / 1e3, 2),
            "isosurface_kernels": ours,
            "largest_other_kernels": [{"name": r["Name"][:96], "calls_per_run": int(r["Calls"]) / calls,
                                       "us_per_run": round(float(r["TotalDurationNs"]) / calls / 1e3, 2)} for r in rest[:6]]}


LIMITS = {"device": 240, "trace": 300}                        # seconds per child; torch's start-up is most of a short step


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--step", choices=("device", "trace"))
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "isosurface_timing"))
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--num_blocks", type=int, default=16)
    ap.add_argument("--density_thresh", type=float, default=0.8)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if a.step == "device":
        print(json.dumps(device_step(a.n, a.resolution, a.num_blocks, a.density_thresh, a.runs)), flush=True)
    elif a.step == "trace":
        print(json.dumps(trace_step(a.out, a.n, a.resolution, a.runs)), flush=True)
    else:
        os.makedirs(a.out, exist_ok=True)
        for step in ("device", "trace"):
            for R in a.resolutions:
                r = subprocess.run(["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
                                    "--resolution", str(R), "--n", str(a.n), "--runs", str(a.runs), "--out", a.out], stdout=subprocess.PIPE, text=True)
                if r.returncode != 0:
                    print(json.dumps({"tool": "isosurface_timing", "failed_step": step, "resolution": R, "exit_status": r.returncode}), flush=True)
                    sys.exit(r.returncode)
                print(r.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
