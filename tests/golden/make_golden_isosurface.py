#!/usr/bin/env python
"""Generates tests/golden/gaussian_field.npz from the REFERENCE's own occupancy field.

Run in the authoring container only (needs /root/reference, which does not exist on the GPU box):
    python tests/golden/make_golden_isosurface.py
Nothing from /root/reference is copied: the fixture is data (seeded inputs and the grids the reference computes for them).

The functions are taken from the reference's files by AST, as make_golden.py takes ``C`` and ``strain_tensor_to_matrix`` (the
enclosing modules import mcubes, plyfile, simple_knn, threestudio): ``GaussianIO.extract_fields``
(custom/threestudio-dreammesh4d/geometry/gaussian_io.py:174-265) and, from geometry/gaussian_base.py, ``gaussian_3d_coeff``,
``build_rotation``, ``build_scaling_rotation``, ``strip_lowerdiag``, ``strip_symmetric`` and the nested
``build_covariance_from_scaling_rotation``.  They run on the CPU on a stand-in ``self``.  Two stubs: ``tqdm`` is the identity, and
``torch`` is a proxy whose ``zeros`` drops ``device="cuda"`` and the hard-coded ``dtype=torch.float`` (the default dtype decides)
and whose ``linspace`` always yields the float32 grid coordinates (cast to the default dtype) -- so that the SAME functions run
once as they are (float32: ``occ``) and once on float64 inputs under a float64 default dtype (``occ_f64``), on the same grid.

  case A   N = 300, R = 32, num_blocks = 4
  case B   the same Gaussians, num_blocks = 16: block_size * relax_ratio = 0.1875, the hard cut-off removes real contributions
  case C   case B plus 40 Gaussians at opacity <= 0.005 outside the others' bounding box: the filter changes the normalisation

Stored per case: the inputs (cases A and B share theirs: stored once, under ``A/``), ``occ`` (float32), ``center``, ``scale``,
``err_ref = max|occ - occ_f64| / max(occ_f64)`` -- the reference's own float32 error, the unit of the device test's bound -- and
the float64 grid as ``occ_res = float32(occ_f64 - occ)``: ``occ_f64 = float64(occ) + float64(occ_res)`` up to the residual's own
float32 rounding, 2^-24 of a difference of 1e-6, which is 1e-13 (``isosurface_common.golden_case`` puts it together).  This
halves the file.
No normalised centre lies within 1e-6 of a block bound (asserted; the seed moves on until it holds), so float32 and float64
take the same cull decisions.
"""
import ast
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
GEO = os.path.join(REF, "custom", "threestudio-dreammesh4d", "geometry")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))


class _Torch:
    """torch, except: zeros ignores device / dtype, linspace is the float32 grid in the default dtype."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def zeros(*args, **kw):
        kw.pop("device", None)
        kw.pop("dtype", None)
        return torch.zeros(*args, **kw)

    @staticmethod
    def linspace(*args, **kw):
        return torch.linspace(*args, dtype=torch.float32, **kw).to(torch.get_default_dtype())


def find_function(path, names):
    """The FunctionDef reached by following `names` through classes / functions of the file."""
    node = ast.parse(open(path).read())
    for name in names:
        node = next(n for n in ast.walk(node) if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name == name)
    node.returns = None
    for a in node.args.args + node.args.kwonlyargs:
        a.annotation = None
    return node


def load_reference():
    ns = {"torch": _Torch(), "tqdm": lambda it: it}
    base = os.path.join(GEO, "gaussian_base.py")
    for names in (["gaussian_3d_coeff"], ["build_rotation"], ["build_scaling_rotation"], ["strip_lowerdiag"], ["strip_symmetric"],
                  ["setup_functions", "build_covariance_from_scaling_rotation"]):
        exec(compile(ast.Module(body=[find_function(base, names)], type_ignores=[]), base, "exec"), ns)
    io = os.path.join(GEO, "gaussian_io.py")
    exec(compile(ast.Module(body=[find_function(io, ["GaussianIO", "extract_fields"])], type_ignores=[]), io, "exec"), ns)
    return ns


def run_reference(ns, g, dtype, resolution, num_blocks):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
        me = types.SimpleNamespace(get_opacity=t(g["opacity"]).reshape(-1, 1), get_xyz=t(g["xyz"]), get_scaling=t(g["scaling"]),
                                   _rotation=t(g["rotation"]), covariance_activation=ns["build_covariance_from_scaling_rotation"])
        occ = ns["extract_fields"](me, resolution=resolution, num_blocks=num_blocks)
        return occ.numpy(), me.center.numpy(), float(me.scale)
    finally:
        torch.set_default_dtype(old)


def clear_of_block_bounds(g, resolution, num_blocks, margin=1e-6):
    from tests import isosurface_common as ic

    mask, center, scale = ic.normalisation(g["xyz"], g["opacity"])
    xyzn = (g["xyz"][mask] - center) * np.float32(scale)
    _, vmin, vmax = ic.block_bounds(resolution, num_blocks)
    bounds = np.concatenate([vmin, vmax]).astype(np.float64)
    return float(np.abs(xyzn.astype(np.float64)[..., None] - bounds).min()) > margin


def scene(seed):
    from tests import isosurface_common as ic

    g = ic.random_gaussians(300, seed)
    rng = np.random.default_rng(seed + 1000)
    far = ic.random_gaussians(40, seed + 2000)
    far["xyz"] = (far["xyz"] * 0.3 + np.array([1.6, 0.9, -0.7])).astype(np.float32)           # outside the others' bounding box
    far["opacity"] = rng.choice(np.array([0.005, 0.004, 0.001, 0.0], np.float32), 40)
    order = rng.permutation(340)
    both = {k: np.concatenate([g[k], far[k]])[order] for k in g}
    return g, both


def main():
    if not os.path.isdir(REF):
        sys.exit("needs /root/reference (authoring container only)")
    ns = load_reference()
    seed = 100
    while True:
        g, both = scene(seed)
        if all(clear_of_block_bounds(x, 32, nb) for x, nb in ((g, 4), (g, 16), (both, 16))):
            break
        seed += 1
    out = {"seed": np.int64(seed)}
    for name, x, nb in (("A", g, 4), ("B", g, 16), ("C", both, 16)):
        occ32, center, scale = run_reference(ns, x, torch.float32, 32, nb)
        occ64, center64, scale64 = run_reference(ns, x, torch.float64, 32, nb)
        assert occ32.dtype == np.float32 and occ64.dtype == np.float64 and center.dtype == np.float32
        assert np.abs(center - center64).max() < 1e-6 and abs(scale - scale64) < 1e-6 * scale
        assert not (occ64[occ32 != 0] == 0).any()                  # float32 underflows to 0 far earlier than float64, never later
        err = float(np.abs(occ32 - occ64).max() / occ64.max())
        res = (occ64 - occ32.astype(np.float64)).astype(np.float32)
        assert np.abs(occ32.astype(np.float64) + res.astype(np.float64) - occ64).max() <= 1e-12
        if name != "B":                                          # B runs on A's inputs
            for k in ("xyz", "scaling", "rotation", "opacity"):
                out[f"{name}/{k}"] = x[k]
        out.update({f"{name}/occ": occ32, f"{name}/occ_res": res, f"{name}/center": center, f"{name}/scale": np.float64(scale),
                    f"{name}/err_ref": np.float64(err), f"{name}/num_blocks": np.int64(nb), f"{name}/resolution": np.int64(32)})
        print(f"case {name}: N {len(x['xyz'])}, num_blocks {nb}, max occ {occ64.max():.4f}, zero voxels {(occ32 == 0).mean():.3f}, "
              f"err_ref {err:.3e}, scale {scale:.6f}")
    path = os.path.join(OUT, "gaussian_field.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes (seed {seed})")


if __name__ == "__main__":
    main()
