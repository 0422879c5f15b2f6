"""Timing of knn_points (csrc/knn.hip): the exhaustive search against the box search over cloud sizes, `torch.cdist` + `topk` on the
same device, and the per-kernel times of one `rocprofv3 --kernel-trace --stats` run.  One JSON line per step, and one for the whole.

    python tools/knn_timing.py [--out DIR]      every step in a child process under its own `timeout`; the first step that fails
                                                ends the run (nothing more is started on the device)
    python tools/knn_timing.py --step sweep | cdist | trace | traced      one step, in this process

Times are wall clock around the whole call with a device synchronise at both ends (scratch allocation and the int64 copy of the
indices included: what a caller waits for), median of --runs.  Clouds are seeded uniform points in the unit cube, searched in
themselves with exclude_self.  Where both methods run at a size their outputs are compared, and must be equal."""
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
SIZES = (1000, 4000, 16000, 64000, 256000, 1000000)
BRUTE_FEW_RUNS_ABOVE = 100000            # the exhaustive search is quadratic: 3 runs instead of --runs above this size
LIMITS = {"sweep": 420, "cdist": 240, "trace": 300}


def _device():
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("knn_timing: no HIP device (the steps do not fall back)")
    return torch.device("cuda:0")


def _median_ms(fn, runs, warmup):
    import torch

    times = []
    for i in range(warmup + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(1e3 * (time.perf_counter() - t0))
    times.sort()
    return round(times[len(times) // 2], 3), out


def _cloud(n, dev, seed=0):
    import torch

    return torch.rand(n, 3, generator=torch.Generator().manual_seed(seed + n)).to(dev)


def sweep_step(runs, warmup, sizes=SIZES):
    import torch

    from dreammesh4d_amd.knn import knn_points

    dev = _device()
    rows = []
    for K in (8, 16):
        for n in sizes:
            x = _cloud(n, dev)
            few = n > BRUTE_FEW_RUNS_ABOVE
            b_ms, b = _median_ms(lambda: knn_points(x, x, K, exclude_self=True, method="brute"), 3 if few else runs, 1 if few else warmup)
            x_ms, bx = _median_ms(lambda: knn_points(x, x, K, exclude_self=True, method="boxes"), runs, warmup)
            same = bool(torch.equal(b.dists, bx.dists) and torch.equal(b.idx, bx.idx))
            rows.append({"K": K, "N": n, "brute_ms": b_ms, "brute_runs": 3 if few else runs, "boxes_ms": x_ms, "identical": same})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            if not same:
                raise SystemExit(f"knn_timing: brute and boxes differ at N = {n}, K = {K}")
    return {"step": "sweep", "device": torch.cuda.get_device_name(0), "runs": runs, "rows": rows}


def cdist_step(runs, warmup):
    """`torch.cdist` + `topk` (what graph_build's eucdisc mode does) against knn_points on the same inputs: 83k vertices against
    1000 nodes at K = 6, and self searches at sizes whose N x N float32 matrix the device holds comfortably."""
    import torch

    from dreammesh4d_amd.knn import knn_points

    dev = _device()
    rows = []

    def one(name, q, p, K, exclude):
        def dense():
            d = torch.cdist(q, p)
            if exclude:
                d.fill_diagonal_(float("inf"))
            return torch.topk(d, K, dim=1, largest=False)

        c_ms, _ = _median_ms(dense, runs, warmup)
        for m in ("brute", "boxes"):
            k_ms, _ = _median_ms(lambda: knn_points(q, p, K, exclude_self=exclude, method=m), runs, warmup)
            rows.append({"case": name, "Nq": int(q.shape[0]), "Np": int(p.shape[0]), "K": K, "cdist_topk_ms": c_ms, "method": m, "knn_points_ms": k_ms,
                         "matrix_GiB": round(q.shape[0] * p.shape[0] * 4 / 2 ** 30, 2)})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)

    one("vertices x nodes", _cloud(83000, dev), _cloud(1000, dev, seed=1), 6, False)
    for n in (32768, 65536):
        x = _cloud(n, dev)
        one("self", x, x, 8, True)
    return {"step": "cdist", "device": torch.cuda.get_device_name(0), "runs": runs, "rows": rows}


def traced_step():
    """What the trace step runs under the profiler: a few calls of each method."""
    from dreammesh4d_amd.knn import knn_points

    dev = _device()
    big, small, query = _cloud(1000000, dev), _cloud(64000, dev), _cloud(100000, dev, seed=2)
    for _ in range(TRACE_CALLS):
        knn_points(big, big, 8, exclude_self=True, method="boxes")
        knn_points(query, big, 8, method="boxes")
        knn_points(small, small, 8, exclude_self=True, method="brute")
    import torch

    torch.cuda.synchronize()
    return {"step": "traced", "calls": TRACE_CALLS}


TRACE_CALLS = 4


def trace_step(out_dir):
    """The traced step under rocprofv3 (the program goes after `--`); per-kernel totals divided by the number of calls."""
    d = os.path.join(out_dir, "knn_trace")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "knn", "--",
           sys.executable, os.path.abspath(__file__), "--step", "traced"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    path = sorted(glob.glob(os.path.join(d, "**", "knn_kernel_stats.csv"), recursive=True))[0]
    rows = list(csv.DictReader(open(path)))
    ours = {r["Name"].split("(")[0].replace("void dm4d::", ""): {"calls": int(r["Calls"]), "us_per_call": round(float(r["TotalDurationNs"]) / int(r["Calls"]) / 1e3, 2),
                                                                "us_total": round(float(r["TotalDurationNs"]) / 1e3, 1)}
            for r in rows if "k_knn" in r["Name"]}
    return {"step": "trace", "csv": os.path.relpath(path, ROOT), "what": "per call: boxes 1 M self K = 8; boxes 100 k queries in 1 M points K = 8; brute 64 k self K = 8",
            "calls_of_each": TRACE_CALLS, "knn_kernels": ours}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--step", choices=("sweep", "cdist", "trace", "traced"))
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "knn_timing"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.step == "sweep":
        print(json.dumps(sweep_step(a.runs, a.warmup)), flush=True)
    elif a.step == "cdist":
        print(json.dumps(cdist_step(a.runs, a.warmup)), flush=True)
    elif a.step == "traced":
        print(json.dumps(traced_step()), flush=True)
    elif a.step == "trace":
        print(json.dumps(trace_step(a.out)), flush=True)
    else:
        os.makedirs(a.out, exist_ok=True)
        results = {}
        for step in ("sweep", "cdist", "trace"):
            r = subprocess.run(["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--out", a.out,
                                "--runs", str(a.runs), "--warmup", str(a.warmup)], stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                print(json.dumps({"tool": "knn_timing", "failed_step": step, "exit_status": r.returncode, "done": results}), flush=True)
                sys.exit(r.returncode)
            results[step] = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(results[step]), flush=True)
        with open(os.path.join(a.out, "knn_timing.json"), "w") as fh:
            json.dump(results, fh, indent=1)
        print(json.dumps({"tool": "knn_timing", "sizes": SIZES, "out": os.path.relpath(a.out, ROOT)}), flush=True)


if __name__ == "__main__":
    main()
