#!/usr/bin/env python
"""Generates tests/golden/arap_fit.npz from the REFERENCE's own ARAPCoach, called the way its signature invites:
``compute_arap_energy(xyz_prime)`` with ``vert_rotations=None`` (custom/threestudio-dreammesh4d/utils/arap_utils.py:195-214:
covariance of the one-ring, batched SVD, R = W U^T, flip of the smallest singular value's column where det <= 0).

Run in the authoring container only (needs the reference tree beside the repository, as tests/golden/make_golden.py does):
    python tests/golden/make_golden_arap_fit.py
Nothing of the reference is copied: the fixture holds arrays only -- the mesh, a few deformed vertex sets, and what the reference
computes for them.

The reference runs under ``torch.set_default_dtype(torch.float64)`` with float64 vertices (its ``torch.zeros`` buffers take the
default dtype; in its shipped float32 the fit is the thing under test, not a yardstick).  Every input value is rounded to float32
first, so the float32 kernels see exactly the numbers the reference saw.  R is not an output of the reference's method: it is
recorded by wrapping ``torch.det``, which the method calls on R before the flip (:209), and reapplying the flip it then performs
in place (:211-214) -- checked against the energy the method returns.

Cases (a 320-face uv sphere, 162 vertices):
  smooth   x A^T + 0.002 noise   a smooth deformation (at this resolution the sphere's curvature decides every determinant: no flip)
  mid      x A^T + 0.02 noise
  noisy    x A^T + 0.1 noise     both flip outcomes occur in bulk
  rigid    x Q^T + c             a rigid motion: R = Q everywhere, energy 0
  yz       only y and z move     every vertex is "unchanged" by the reference's rule (:201-202) => R = I, energy sum w |e' - e|^2
"""
import importlib.util
import os
import sys
import types
import typing

import numpy as np
import torch

REF = "/root/reference"
C_DIR = os.path.join(REF, "custom", "threestudio-dreammesh4d")
OUT = os.path.dirname(os.path.abspath(__file__))


def load_reference():
    ty = types.ModuleType("threestudio.utils.typing")
    for n in dir(typing):
        if not n.startswith("_"):
            setattr(ty, n, getattr(typing, n))

    class _SubMeta(type):
        def __getitem__(cls, k):
            return cls

    class _Sub(metaclass=_SubMeta):
        pass

    ty.Float = ty.Int = ty.Num = ty.Bool = _Sub
    ty.Tensor = torch.Tensor
    sys.modules.update({"threestudio": types.ModuleType("threestudio"), "threestudio.utils": types.ModuleType("threestudio.utils"),
                        "threestudio.utils.typing": ty, "open3d": types.ModuleType("open3d")})
    spec = importlib.util.spec_from_file_location("ref_arap", os.path.join(C_DIR, "utils", "arap_utils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def run(coach, ref, xyz_prime):
    """The reference's energy, autograd gradient, and the R / singular values it computed on the way."""
    seen = {}
    real_det, real_svd = torch.det, ref.batch_svd

    def det(R):
        d = real_det(R)
        seen["R"], seen["det"] = R, d.detach().clone()       # R is flipped in place afterwards: keep the handle
        return d

    def svd(S):
        U, sig, W = real_svd(S)
        seen["sig"] = sig.detach().clone()
        return U, sig, W

    x = xyz_prime.clone().requires_grad_(True)
    torch.det, ref.batch_svd = det, svd
    try:
        E = coach.compute_arap_energy(x)
    finally:
        torch.det, ref.batch_svd = real_det, real_svd
    (g,) = torch.autograd.grad(E, x)
    return {"xyz_prime": xyz_prime.numpy(), "R": seen["R"].detach().numpy(), "flip": (seen["det"] <= 0).numpy(),
            "sig": seen["sig"].numpy(), "energy": np.float64(E.item()), "g_xyz": g.numpy()}


def main():
    if not os.path.isdir(REF):
        sys.exit("needs the reference tree (authoring container only)")
    torch.set_default_dtype(torch.float64)
    ref = load_reference()
    sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
    from dreammesh4d_amd import synthetic as syn

    verts_np, faces_np = syn.uv_sphere(320, radius=0.6)
    verts_np, faces_np = np.asarray(verts_np, np.float32), np.asarray(faces_np, np.int64)
    verts = torch.tensor(verts_np.astype(np.float64))
    coach = ref.ARAPCoach(verts, faces_np, torch.device("cpu"))
    g = torch.Generator().manual_seed(4)
    f32 = lambda t: t.float().double()                        # the values the float32 kernels will be given
    A = torch.eye(3) + 0.2 * torch.randn(3, 3, generator=g)
    q = torch.nn.functional.normalize(torch.randn(4, generator=g), dim=0)
    x, y, z, w = q.tolist()
    Q = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    yz = verts.clone()
    yz[:, 1:] += 0.05 * torch.randn(len(verts), 2, generator=g)
    cases = {"smooth": f32(verts @ A.T + 0.002 * torch.randn(verts.shape, generator=g)),
             "mid": f32(verts @ A.T + 0.02 * torch.randn(verts.shape, generator=g)),
             "noisy": f32(verts @ A.T + 0.1 * torch.randn(verts.shape, generator=g)),
             "rigid": f32(verts @ Q.T + torch.tensor([0.3, -0.2, 0.1])),
             "yz": f32(yz)}
    out = {"verts": verts_np, "faces": faces_np, "cases": np.array(sorted(cases)), "rigid_Q": Q.numpy()}
    for name in sorted(cases):
        r = run(coach, ref, cases[name])
        sig, flip = r["sig"], r["flip"]
        gap = (sig[:, 1] + np.where(flip, -1.0, 1.0) * sig[:, 2]) / np.maximum(sig[:, 0], 1e-300)
        moved = sig[:, 0] > 0
        print(f"{name:7s} E {r['energy']:.9g}  flipped {int(flip.sum())}/{len(flip)}  S = 0 at {int((~moved).sum())}  "
              f"min sig3/sig1 {float((sig[moved, 2] / sig[moved, 0]).min()) if moved.any() else float('nan'):.3e}  "
              f"min gap {float(gap[moved].min()) if moved.any() else float('nan'):.3e}  |g|max {np.abs(r['g_xyz']).max():.3e}")
        # the recorded R is the one the energy was computed with
        P, Pp, wn = coach.edge_matrix_nfmt, coach.produce_edge_matrix_nfmt(cases[name]), coach.edge_cot_weights
        E2 = (wn * (Pp - torch.einsum("vab,vnb->vna", torch.tensor(r["R"]), P)).square().sum(-1)).sum()
        assert abs(float(E2) - r["energy"]) <= 1e-12 * max(1.0, abs(r["energy"])), (float(E2), r["energy"])
        for k, v in r.items():
            out[f"{name}_{k}"] = v
    assert 0.1 * len(verts) < out["noisy_flip"].sum() < 0.9 * len(verts)
    assert (out["yz_sig"] == 0).all() and np.array_equal(out["yz_R"], np.broadcast_to(np.eye(3), out["yz_R"].shape))
    path = os.path.join(OUT, "arap_fit.npz")
    np.savez_compressed(path, **out)
    print("arap_fit.npz: V", len(verts), "F", len(faces_np), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
