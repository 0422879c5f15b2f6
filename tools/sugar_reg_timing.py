#!/usr/bin/env python
"""Times the SuGaR density and normal regularisation ("SuGaR density and normal regularisation"; profiles/sugar_reg.md).

Protocol: one process, median of 20 after 3 warm-ups, device events around the whole call (forward AND backward of
``sugar_density_reg`` with the reverse table kept by the caller, as ``SuGaRRegularizer`` calls it), at the reference's own size
S = 500,000, K = 16, N = 100,000, with and without the normal loss.  Baselines: the reference's expressions written in torch,
float32, on the same device; the bytes the algorithm needs against the copy rate measured in the same process.  Also: the share of
the grouping sort and tables in the call, and the peak memory of both formulations.

    python tools/sugar_reg_timing.py [--n 100000] [--k 16] [--s 500000] [--out sugar_reg_timing.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dreammesh4d_amd import knn, sugar_reg as sr  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, reps=20, warmup=3):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def torch_formulation(xyz, s, q, op, knn_idx, g, eps, normal):
    """The reference's expressions (sugar_utils.py:226-228, 256-262, 305-311, 355-372, 420-423, 708-757) in torch."""
    x = xyz[g] + sr.quaternion_apply(q[g], 1.5 * s[g] * eps)
    R = sr.quaternion_to_matrix(q)
    M = R * (1.0 / s.clamp(min=1e-8))[:, None]
    J = knn_idx[g]
    warped = M[J].transpose(-1, -2) @ (x[:, None] - xyz[J])[..., None]
    w = op[J] * torch.exp(-0.5 * (warped[..., 0] * warped[..., 0]).sum(dim=-1).clamp(min=0.0, max=1e8))
    density = w.sum(dim=-1)
    m, cs = s.min(dim=-1)
    n = R.gather(2, cs[:, None, None].expand(-1, 3, -1)).squeeze(2)
    beta = m[J].mean(dim=1)
    ng = n[g]
    sdf = ((x - xyz[g]) * ng).sum(dim=-1)
    loss = (density - torch.exp(-0.5 * sdf.pow(2) / beta.pow(2))).abs().mean()
    if normal:
        cn = n[J]
        cn = cn * torch.sign((cn * ng[:, None]).sum(dim=-1, keepdim=True)).detach()
        nw = ((x[:, None] - xyz[J]) * cn).sum(dim=-1).abs().detach()
        nw = w.detach() * nw / m[J].detach().clamp(min=1e-6) ** 2
        nw = nw / nw.sum(dim=-1).detach().unsqueeze(-1).clamp(min=1e-6)
        loss = loss + (ng - (nw[..., None] * cn).sum(dim=-2)).pow(2).sum(dim=-1).mean()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--s", type=int, default=500000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, K, S = a.n, a.k, a.s
    gen = torch.Generator(device=DEV).manual_seed(0)
    xyz = torch.randn(N, 3, device=DEV, generator=gen)
    xyz = (xyz / xyz.norm(dim=1, keepdim=True) * 0.8 * torch.rand(N, 1, device=DEV, generator=gen) ** (1 / 3)).requires_grad_(True)
    spacing = 0.8 * (4.0 / N) ** (1 / 3)
    s = (spacing * 10 ** (torch.rand(N, 3, device=DEV, generator=gen) * 2 - 1.7)).requires_grad_(True)
    q = torch.nn.functional.normalize(torch.randn(N, 4, device=DEV, generator=gen), dim=-1).requires_grad_(True)
    op = (0.05 + 0.94 * torch.rand(N, device=DEV, generator=gen)).requires_grad_(True)
    knn_idx = knn.knn_points(xyz.detach(), xyz.detach(), K).idx
    knn32 = knn_idx.to(torch.int32).contiguous()
    reverse = sr.reverse_table(knn32)
    g = torch.randint(0, N, (S,), device=DEV, generator=gen)
    g32 = g.to(torch.int32)
    eps = torch.randn(S, 3, device=DEV, generator=gen)
    leaves = (xyz, s, q, op)

    def clear():
        for t in leaves:
            t.grad = None

    def fused(normal):
        clear()
        out = sr.sugar_density_reg(xyz, s, q, op, knn32, g32, eps, with_normal_loss=normal, reverse=reverse, validate=False)
        (out.density_regulation + (out.normal_regulation if normal else 0.0)).backward()

    def torch_way(normal):
        clear()
        torch_formulation(xyz, s, q, op, knn_idx, g, eps, normal).backward()

    res = {"N": N, "K": K, "S": S, "device": torch.cuda.get_device_name(0), "protocol": "median of 20 after 3 warm-ups, device events, forward + backward"}
    big = torch.empty(64 * 2 ** 20, dtype=torch.float32, device=DEV)
    dst = torch.empty_like(big)
    t = timed(lambda: dst.copy_(big))
    res["copy_GBps"] = 2 * big.numel() * 4 / t["median_ms"] / 1e6
    del big, dst
    for normal in (False, True):
        tag = "normal" if normal else "plain"
        res[f"fused_{tag}"] = timed(lambda: fused(normal))
        res[f"fused_{tag}_peak_MiB"] = peak(lambda: fused(normal))
        res[f"torch_{tag}"] = timed(lambda: torch_way(normal))
        res[f"torch_{tag}_peak_MiB"] = peak(lambda: torch_way(normal))
    res["fused_plain_default_checks"] = timed(lambda: (clear(), sr.sugar_density_reg(xyz, s, q, op, knn32, g32, eps).density_regulation.backward()))
    res["grouping_tables"] = timed(lambda: sr._segments(g32, N))
    res["reverse_table"] = timed(lambda: sr.reverse_table(knn32))
    chunks = (S + sr.CHUNK - 1) // sr.CHUNK + min(N, S)
    need = {"inputs": N * 11 * 4 * 2 + N * K * 4 * 2 + S * 5 * 4 * 2 + S * 4 * 2, "records": N * 18 * 4 * 3, "per-sample outputs": S * 4 * 4,
            "gradient records (written, read)": 2 * chunks * (K * 17 + 13) * 4, "outputs": N * 11 * 4}
    res["bytes_needed"] = need
    res["bytes_needed_ms_at_copy_rate"] = sum(need.values()) / res["copy_GBps"] / 1e6
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
