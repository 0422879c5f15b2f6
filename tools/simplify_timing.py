"""Timing of mesh simplification by vertex clustering on the million-vertex scene of the tests (about 1.0 M vertices, 2.0 M faces,
scale 128): the device operator, the numpy float64 restatement on this box's host, and the per-kernel times of one
`rocprofv3 --kernel-trace --stats` run.  One JSON line per step, and one for the whole.

    python tools/simplify_timing.py [--out DIR]      every step in a child process under its own `timeout`; the first step that
                                                     fails ends the run (nothing more is started on the device)
    python tools/simplify_timing.py --step host | device | trace      one step, in this process

The device time is wall clock around the whole call with a device synchronise at both ends: the operator synchronises by itself
four times (the bounds, the cluster count, the two counts of faces), and those round trips are part of what a caller waits for."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCALE = 128
LIMITS = {"host": 300, "device": 300, "trace": 420}       # seconds; scene construction on the host is ~10 s of each


def scene():
    from tests import mesh_simplify_common as mc

    return mc.million_scene()


def host_step(runs):
    import numpy as np

    from tests import mesh_simplify_common as mc

    v, f, c = scene()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        ref = mc.simplify_reference(v, f, c, scale=SCALE)
        times.append(time.perf_counter() - t0)
    return {"step": "host", "what": "numpy float64 restatement (tests/mesh_simplify_common.py)", "numpy": np.__version__,
            "cpus_allowed": len(os.sched_getaffinity(0)), "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
            "vertices": len(v), "faces": len(f), "out_vertices": ref["n_vertices"], "out_faces": ref["n_faces"],
            "seconds_min": round(min(times), 3), "seconds_all": [round(t, 3) for t in times]}


def device_step(runs, warmup):
    import torch

    from dreammesh4d_amd import mesh_simplify as ms

    if not torch.cuda.is_available():
        raise SystemExit("simplify_timing: no HIP device (the device steps do not fall back)")
    dev = torch.device("cuda:0")
    v, f, c = scene()
    tv, tf, tc = (torch.from_numpy(a).to(dev) for a in (v, f, c))
    times = []
    for i in range(warmup + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ms.simplify_vertex_clustering(tv, tf, tc, scale=SCALE)
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(1e3 * (time.perf_counter() - t0))
    times.sort()
    return {"step": "device", "device": torch.cuda.get_device_name(0), "vertices": len(v), "faces": len(f),
            "out_vertices": out["n_vertices"], "out_faces": out["n_faces"], "runs": runs,
            "ms_median": round(times[len(times) // 2], 3), "ms_min": round(times[0], 3), "ms_max": round(times[-1], 3)}


def trace_step(out_dir, runs):
    """The device step under rocprofv3 (the program goes after `--`); per-kernel totals divided by the number of calls."""
    d = os.path.join(out_dir, "simplify_trace")
    calls = runs + 1
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "simplify", "--",
           sys.executable, os.path.abspath(__file__), "--step", "device", "--runs", str(runs), "--warmup", "1"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    path = sorted(glob.glob(os.path.join(d, "**", "simplify_kernel_stats.csv"), recursive=True))[0]
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    ours = {r["Name"].split("(")[0]: {"calls_per_run": int(r["Calls"]) / calls, "us_per_run": round(float(r["TotalDurationNs"]) / calls / 1e3, 2)}
            for r in rows if "k_simplify_" in r["Name"]}
    rest = sorted((r for r in rows if "k_simplify_" not in r["Name"]), key=lambda r: -float(r["TotalDurationNs"]))
    return {"step": "trace", "csv": os.path.relpath(path, ROOT), "calls": calls, "kernel_us_per_run_all": round(total / calls / 1e3, 2),
            "simplify_kernels": ours,
            "largest_other_kernels": [{"name": r["Name"][:96], "calls_per_run": int(r["Calls"]) / calls,
                                       "us_per_run": round(float(r["TotalDurationNs"]) / calls / 1e3, 2)} for r in rest[:8]]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--step", choices=("host", "device", "trace"))
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "simplify_timing"))
    ap.add_argument("--runs", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.step == "host":
        print(json.dumps(host_step(a.runs or 3)), flush=True)
    elif a.step == "device":
        print(json.dumps(device_step(a.runs or 20, a.warmup)), flush=True)
    elif a.step == "trace":
        print(json.dumps(trace_step(a.out, a.runs or 5)), flush=True)
    else:
        os.makedirs(a.out, exist_ok=True)
        results = {}
        for step in ("device", "trace", "host"):
            r = subprocess.run(["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--out", a.out],
                               stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                print(json.dumps({"tool": "simplify_timing", "failed_step": step, "exit_status": r.returncode, "done": results}), flush=True)
                sys.exit(r.returncode)
            results[step] = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(results[step]), flush=True)
        with open(os.path.join(a.out, "simplify_timing.json"), "w") as fh:
            json.dump(results, fh, indent=1)
        print(json.dumps({"tool": "simplify_timing", "scale": SCALE, "device_ms_median": results["device"]["ms_median"],
                          "host_numpy_s": results["host"]["seconds_min"],
                          "simplify_kernels_us": {k: v["us_per_run"] for k, v in results["trace"]["simplify_kernels"].items()}}), flush=True)


if __name__ == "__main__":
    main()
