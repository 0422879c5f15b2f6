#!/usr/bin/env python
"""Generates tests/golden/sugar_reg.npz from the REFERENCE's own SuGaR regulariser.

Run in the authoring container only (needs /root/reference, which does not exist on the GPU box):
    python tests/golden/make_golden_sugar_reg.py
Nothing from /root/reference is copied: the fixture is data (seeded inputs and what the reference computes for them).

The methods are taken from ``SuGaRRegularizer`` (custom/threestudio-dreammesh4d/utils/sugar_utils.py) by AST, as
make_golden_density_control.py takes the density control: ``sample_points_in_gaussians``, ``get_covariance``,
``get_field_values``, ``get_beta``, ``get_smallest_axis``, ``get_normals``, ``coarse_density_regulation``.  They run on the CPU as
methods of a stand-in class whose properties (``points``, ``scaling``, ``strengths``, ``quaternions``) return seeded leaf tensors.
``torch`` is a proxy: ``multinomial`` returns the stored ``sample_idx``, ``randn_like`` the stored ``eps`` (in the dtype asked
for), and ``Tensor.cuda`` is the identity while the methods run.  pytorch3d is not installed here: ``quaternion_to_matrix`` and
``quaternion_apply`` are the stand-ins of tests/sugar_reg_common.py, written from their documented formulae.

  N = 400, K = 16, S = 3000; ``knn_idx`` from an exact float64 search; anisotropic scales over two decades, quaternions normalised
  in float32, opacities in (0.05, 0.99)

The regulariser runs with ``use_sdf_better_normal_loss`` in float32 as the reference is written and on float64 copies of the same
inputs; the four gradients by ``autograd`` of the density term alone (``d``), the normal term alone (``n``) and their sum (``dn``).
Without the normal loss the reference computes the same density term (asserted to 1e-13 in float64), so one set serves both.  Stored: the
inputs, the float64 results and ``err_ref = max|f32 - f64|`` per tensor, the reference's own float32 error and the unit of the
device bounds.  The per-sample arrays are read from ``get_field_values`` and from the loss expressions by wrapping ``mean``.
No decision quantity lies within MARGIN (1e-4 relative) of its threshold (asserted; the seed moves on until it holds), so float32
and float64 take the same decisions: the two smallest scales of every Gaussian, n_j.n_g against 0, density - target against 0,
every max(., 1e-6) / max(., 1e-8) argument and the clamp at 1e8 against their bounds.  No sample is excluded.
"""
import ast
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

REF = "/root/reference"
BASE = os.path.join(REF, "custom", "threestudio-dreammesh4d", "utils", "sugar_utils.py")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

from tests import sugar_reg_common as cm  # noqa: E402

METHODS = ["sample_points_in_gaussians", "get_covariance", "get_field_values", "get_beta", "get_smallest_axis", "get_normals",
           "coarse_density_regulation"]
N, K, S = 400, 16, 3000
MARGIN = 1e-4


class _Torch:
    """torch, except multinomial / randn_like (see the module docstring)."""

    def __init__(self):
        self.sample_idx, self.eps = None, None

    def __getattr__(self, name):
        return getattr(torch, name)

    def multinomial(self, probs, num_samples, replacement):
        assert num_samples == len(self.sample_idx) and replacement and probs.shape == (N,)
        return self.sample_idx.clone()

    def randn_like(self, t):
        assert tuple(t.shape) == tuple(self.eps.shape)
        return self.eps.to(t.dtype)


def load_reference(proxy):
    tree = ast.parse(open(BASE).read())
    ns = {"torch": proxy, "np": np, "quaternion_to_matrix": cm.quaternion_to_matrix, "quaternion_apply": cm.quaternion_apply}
    top = {n.name: n for n in tree.body if isinstance(n, ast.ClassDef)}
    methods = {n.name: n for n in top["SuGaRRegularizer"].body if isinstance(n, ast.FunctionDef)}
    body = []
    for name in METHODS:
        node = methods[name]
        node.returns = None
        for a in node.args.args + node.args.kwonlyargs:
            a.annotation = None
        body.append(node)
    cls = ast.ClassDef(name="Ref", bases=[], keywords=[], body=body, decorator_list=[])
    exec(compile(ast.fix_missing_locations(ast.Module(body=[cls], type_ignores=[])), BASE, "exec"), ns)
    return ns["Ref"]


def run(Ref, proxy, inp, dtype):
    """The reference on `inp` in `dtype` with the normal loss -> the same keys as cm.restate, per upstream in cm.UPSTREAMS."""
    leaf = lambda k: torch.tensor(inp[k], dtype=dtype, requires_grad=True)
    xyz, s, q, op = leaf("xyz"), leaf("scales"), leaf("quats"), leaf("opac")
    me = Ref()
    me.beta_mode, me.binded_to_surface_mesh = "average", False
    me.knn_idx = torch.tensor(inp["knn_idx"], dtype=torch.int64)
    me.gaussians = types.SimpleNamespace(_xyz=xyz)
    cls = type(me)
    cls.points, cls.scaling = property(lambda self: xyz), property(lambda self: s)
    cls.strengths, cls.quaternions = property(lambda self: op[:, None]), property(lambda self: q)
    cls.n_points, cls.device = property(lambda self: N), property(lambda self: torch.device("cpu"))
    proxy.sample_idx, proxy.eps = torch.tensor(inp["sample_idx"], dtype=torch.int64), torch.tensor(inp["eps"])
    seen = {}
    fields = cls.get_field_values

    def spy_fields(self, *a, **kw):
        out = fields(self, *a, **kw)
        seen["density"], seen["beta"] = out["density"].detach().clone(), out["beta"].detach().clone()
        return out

    mean = torch.Tensor.mean

    def spy_mean(t, *a, **kw):
        if t.ndim == 1 and t.shape[0] == S and not a and not kw:
            seen.setdefault("terms", []).append(t.detach().clone())
        return mean(t, *a, **kw)

    cuda = getattr(torch.Tensor, "cuda")
    cls.get_field_values, torch.Tensor.mean, torch.Tensor.cuda = spy_fields, spy_mean, lambda t, *a, **kw: t
    try:
        results = {}
        for flag in (False, True):
            seen.clear()
            args = types.SimpleNamespace(n_samples_for_sdf_regularization=S, use_sdf_better_normal_loss=flag)
            loss = me.coarse_density_regulation(args)
            terms = seen["terms"]
            assert len(terms) == (2 if flag else 1)
            f = lambda t: t.detach().double().numpy().copy()
            base = {"density": f(seen["density"]), "beta": f(seen["beta"]), "density_term": f(terms[0]), "loss_d": f(loss["density_regulation"])}
            if flag:
                base.update(normal_term=f(terms[1]), loss_n=f(loss["normal_regulation"]))
            ups = cm.UPSTREAMS if flag else {"d": cm.UPSTREAMS["d"]}
            for tag, up in ups.items():
                total = up[0] * loss["density_regulation"] + (up[1] * loss["normal_regulation"] if flag else 0)
                grads = torch.autograd.grad(total, (xyz, s, q, op), retain_graph=True, allow_unused=True)
                results[(flag, tag)] = dict(base, **{n: f(torch.zeros_like(t) if g is None else g) for n, g, t in zip(cm.GRADS, grads, (xyz, s, q, op))})
        return results
    finally:
        cls.get_field_values, torch.Tensor.mean, torch.Tensor.cuda = fields, mean, cuda


def margins_hold(inp):
    """True when every decision quantity of the float64 restatement is clear of its threshold by MARGIN."""
    xyz, s, q, op = (np.asarray(inp[k], np.float64) for k in cm.INPUTS[:4])
    clear = lambda v, t: bool((np.abs(v - t) > MARGIN * np.maximum(np.abs(t), np.abs(v))).all())
    two = np.sort(s, axis=1)
    ok = clear(two[:, 0], two[:, 1]) and clear(s, 1e-8)
    R = cm._rotation(q)
    n = R[np.arange(N), :, np.argmin(s, 1)]
    m = s.min(1)
    g, J = inp["sample_idx"].astype(np.int64), inp["knn_idx"].astype(np.int64)[inp["sample_idx"].astype(np.int64)]
    dots = (n[J] * n[g][:, None]).sum(-1)
    ok &= bool((np.abs(dots) > MARGIN).all()) and clear(m, 1e-6)
    r = cm.restate(inp, True)
    x = xyz[g] + cm.quaternion_apply(torch.tensor(q[g]), torch.tensor(1.5 * s[g] * inp["eps"].astype(np.float64))).numpy()
    sdf = ((x - xyz[g]) * n[g]).sum(1)
    target = np.exp(-0.5 * sdf ** 2 / r["beta"] ** 2)
    ok &= clear(r["density"], target)
    a = 1.0 / np.maximum(s, 1e-8)
    u = np.einsum("skrc,skr->skc", (R * a[:, None, :])[J], x[:, None] - xyz[J])
    uu = (u * u).sum(-1)
    ok &= clear(uu, 1e8)
    sg = np.sign(dots)
    vk = op[J] * np.exp(-0.5 * np.clip(uu, 0, 1e8)) * np.abs(((x[:, None] - xyz[J]) * n[J] * sg[..., None]).sum(-1)) / np.maximum(m[J], 1e-6) ** 2
    return ok and clear(vk.sum(1), 1e-6)


def main():
    if not os.path.isdir(REF):
        sys.exit("needs /root/reference (authoring container only)")
    torch.set_num_threads(1)                                # index_add's order of accumulation: the fixture regenerates bit for bit
    torch.use_deterministic_algorithms(True)
    proxy = _Torch()
    Ref = load_reference(proxy)
    seed = 100
    while True:
        inp = cm.random_case(N, K, S, seed)
        if margins_hold(inp):
            break
        seed += 1
    r32, r64 = run(Ref, proxy, inp, torch.float32), run(Ref, proxy, inp, torch.float64)
    for k, v in r64[(False, "d")].items():                  # the density term does not depend on the flag (autograd's order of
        assert np.abs(v - r64[(True, "d")][k]).max() <= 1e-13 * np.abs(v).max(), k       # accumulation does, in the last bits)
    out = {"seed": np.int64(seed), "sampling_scale": np.float64(1.5), "density_factor": np.float64(1.0)}
    out.update({f"in/{k}": inp[k] for k in cm.INPUTS})
    for tag in cm.UPSTREAMS:
        a32, a64 = r32[(True, tag)], r64[(True, tag)]
        for k in a64:
            per_upstream = k in cm.GRADS
            if not per_upstream and tag != "dn":
                continue
            key = f"{tag}/{k}" if per_upstream else k
            err = float(np.abs(a32[k] - a64[k]).max())
            out[key], out[key + "_err_ref"] = a64[k], np.float64(err)
            print(f"    {key}: max |f64| {np.abs(a64[k]).max():.3e}, err_ref {err:.3e}")
    path = os.path.join(OUT, "sugar_reg.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:         # an .npz with fixed member dates: it regenerates bit for bit
        for k, v in out.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    print(f"{path}: {os.path.getsize(path)} bytes (seed {seed})")


if __name__ == "__main__":
    main()
