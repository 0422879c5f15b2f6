#!/usr/bin/env python
"""Generates tests/golden/eval_sh.npz from the REFERENCE's own spherical-harmonics evaluation.

Run in the authoring container only (needs /root/reference, which does not exist on the GPU box):
    python tests/golden/make_golden_sh.py
Nothing from /root/reference is copied: ``eval_sh`` and its constants ``C0`` .. ``C4``
(custom/threestudio-dreammesh4d/geometry/sugar.py:733-820) are pulled out of the module by AST (the module itself needs
pytorch3d / open3d) and executed in float64 on the CPU; the fixture holds arrays only.

  eval_sh.npz   the view-dependent branch of SuGaRModel.get_points_rgb (sugar.py:640-661),
                clamp_min(eval_sh(deg, sh, normalize(points - campos)) + 0.5, 0), for deg 0..3 and two camera centres:
      points [N,3] f32      seeded, inside the unit ball
      sh     [N,16,3] f32   N(0,1) coefficients (the first (deg + 1)^2 are used)
      campos [2,3] f32      camera centres outside the ball
      grad   [N,3] f32      the upstream gradient dL/drgb
      v_d{deg}_c{cam}  [N,3] f64   eval_sh + 0.5 BEFORE the clamp (rgb = max(v, 0), clamped = v < 0)
      A_d{deg}_c{cam}  [N,3] f32   0.5 + sum_k |B_k(dir)| |sh_k|: the scale of the forward's rounding error
      dsh_d{deg}_c{cam}  [NG,(deg+1)^2,3] f32, dpoints_d{deg}_c{cam} [NG,3] f64
                            autograd of sum(grad * rgb) with respect to the coefficients and the points, for the first
                            NG points (each point's colour depends on its own row only; the coefficient gradients are
                            stored in float32 -- they are compared at 1e-4 relative -- to keep the file small)
  N = 1024 and NG = 256 keep the file (about 0.75 MB) under the 1 MiB limit for a committed file.
"""
import ast
import os

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference"
SUGAR = os.path.join(REF, "custom", "threestudio-dreammesh4d", "geometry", "sugar.py")
OUT = os.path.dirname(os.path.abspath(__file__))
N, NG = 1024, 256


def extract_eval_sh(path):
    """eval_sh with the module-level constants C0..C4 it reads (same approach as make_golden.py::extract_function)."""
    tree = ast.parse(open(path).read())
    keep = []
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) and \
                node.targets[0].id in ("C0", "C1", "C2", "C3", "C4"):
            keep.append(node)
        if isinstance(node, ast.FunctionDef) and node.name == "eval_sh":
            node.returns = None
            for a in node.args.args + node.args.kwonlyargs:
                a.annotation = None
            keep.append(node)
    ns = {}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns["eval_sh"]


def main():
    eval_sh = extract_eval_sh(SUGAR)
    rng = np.random.default_rng(20240607)
    u = rng.standard_normal((N, 3))
    points = (u / np.linalg.norm(u, axis=1, keepdims=True) * rng.random((N, 1)) ** (1.0 / 3.0)).astype(np.float32)
    sh = rng.standard_normal((N, 16, 3)).astype(np.float32)
    campos = np.array([[0.3, -3.2, 0.6], [2.1, 1.7, -0.9]], np.float32)
    grad = rng.standard_normal((N, 3)).astype(np.float32)
    out = dict(points=points, sh=sh, campos=campos, grad=grad)
    frac = {}
    for deg in range(4):
        K = (deg + 1) ** 2
        for c in range(2):
            p = torch.tensor(points, dtype=torch.float64, requires_grad=True)
            s = torch.tensor(sh[:, :K], dtype=torch.float64, requires_grad=True)
            cam = torch.tensor(campos[c], dtype=torch.float64)
            dirs = F.normalize(p - cam[None], dim=-1)
            # the reference's layout: [N, 3, K] (sugar.py:655-658)
            v = eval_sh(deg, s.transpose(-1, -2).reshape(-1, 3, K), dirs) + 0.5
            rgb = torch.clamp_min(v, 0.0)
            (rgb * torch.tensor(grad, dtype=torch.float64)).sum().backward()
            with torch.no_grad():
                eye = torch.eye(K, dtype=torch.float64)
                # B_k(dir) = eval_sh of the k-th unit coefficient vector
                B = torch.stack([eval_sh(deg, eye[k][None, None, :].expand(N, 1, K), dirs)[:, 0] for k in range(K)], dim=1)   # [N,K]
                A = 0.5 + (B.abs()[:, :, None] * s.abs()).sum(dim=1)
            tag = f"d{deg}_c{c}"
            out["v_" + tag] = v.detach().numpy()
            out["A_" + tag] = A.numpy().astype(np.float32)
            out["dsh_" + tag] = s.grad[:NG].numpy().astype(np.float32)
            out["dpoints_" + tag] = p.grad[:NG].numpy() if p.grad is not None else np.zeros((NG, 3))   # degree 0: no direction term
            frac[tag] = float((v < 0).double().mean())
    path = os.path.join(OUT, "eval_sh.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; clamped fraction", {k: round(x, 3) for k, x in frac.items()})


if __name__ == "__main__":
    main()
