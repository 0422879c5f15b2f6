"""Wall time of clean_mesh and connected_components on the marching-cubes mesh of the R = 256 blob-plus-floaters field, beside the
numpy / scipy restatement on the CPU ("Mesh cleaning").  Prints one JSON line; --out also writes it to a file.

    python tools/mesh_clean_timing.py [--resolution 256] [--runs 30] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dreammesh4d_amd import isosurface as iso, mesh_clean as mc
from tests import mesh_clean_common as cm



def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--resolution", default=256, type=int)
    p.add_argument("--runs", default=30, type=int)
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_clean_timing: no HIP device; nothing is measured without one")
    dev = "cuda:0"
    occ = torch.from_numpy(cm.blob_field(args.resolution)).to(dev)
    mesh = iso.marching_cubes(occ, 0.0)
    V, F = len(mesh["verts"]), len(mesh["faces"])
    colors = torch.rand(V, 3, device=dev)

    def timed(fn, runs):
        fn()                                                           # warm-up
        out = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t))
        return res, {"median": float(np.median(out)), "min": min(out), "max": max(out), "runs": runs}

    res, t_clean = timed(lambda: mc.clean_mesh(mesh["verts"], mesh["faces"], colors), args.runs)
    _, t_cc = timed(lambda: mc.connected_components(mesh["faces"], V), args.runs)
    v, f, c = mesh["verts"].cpu().numpy(), mesh["faces"].cpu().numpy(), colors.cpu().numpy()
    cpu = []
    for _ in range(3):
        t = time.perf_counter()
        want = cm.restate(v, f, c)
        cpu.append(1e3 * (time.perf_counter() - t))
    got = {k: (x.cpu().numpy() if torch.is_tensor(x) else x) for k, x in res.items()}
    out = {"resolution": args.resolution, "V": V, "F": F, "V_out": len(got["verts"]), "F_out": len(got["faces"]),
           "n_components": got["n_components"], "n_small": got["n_small"], "n_null": got["n_null"], "differences": cm.differences(got, want),
           "clean_mesh_ms": t_clean, "connected_components_ms": t_cc,
           "restatement_ms": {"median": float(np.median(cpu)), "min": min(cpu), "max": max(cpu), "runs": len(cpu)}}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
