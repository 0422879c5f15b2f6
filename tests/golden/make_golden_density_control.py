#!/usr/bin/env python
"""Generates tests/golden/density_control.npz from the REFERENCE's own density control.

Run in the authoring container only (needs /root/reference, which does not exist on the GPU box):
    python tests/golden/make_golden_density_control.py
Nothing from /root/reference is copied: the fixture is data (seeded inputs and what the reference computes for them).

The methods are taken from ``GaussianBaseModel`` (custom/threestudio-dreammesh4d/geometry/gaussian_base.py) by AST, as
make_golden_isosurface.py takes ``extract_fields``: ``densify_and_clone``, ``densify_and_split``, ``densification_postfix``,
``cat_tensors_to_optimizer``, ``_prune_optimizer``, ``prune_points``, ``replace_tensor_to_optimizer``, ``densify``, ``prune``,
``reset_opacity``, ``add_densification_stats``, ``update_states``, the properties ``get_scaling`` / ``get_opacity`` / ``get_xyz``,
and the module's ``build_rotation`` and ``inverse_sigmoid``.  They run on the CPU as methods of a stand-in class whose instance
holds real ``nn.Parameter``s and a real ``torch.optim.Adam(eps=1e-15)`` that has taken two steps.  ``optimize_params`` of the
stand-in includes ``normal`` (with the reference's own list ``prune_points`` raises KeyError under ``pred_normal``).  ``torch`` is
a proxy: ``zeros`` drops ``device=``, ``normal`` returns ``mean + std * eps`` with pre-drawn seeded ``eps`` (rows by copy and rank
among the selected), ``randperm`` returns the stored permutation, ``cuda.empty_cache`` does nothing.

  case A   N = 400, sh_degree 1, pred_normal: statistics of 3 views -> densify -> statistics of 3 views + prune with
           prune_big_points -> opacity reset -> the random cap (max_num 200) -> sugar_prune_at
  case B   the same inputs with sphere = True

Each case runs once in float32 as the reference is written and once on float64 inputs under a float64 default dtype.  Stored:
the inputs (once, under ``A/``), and per case and stage the row plan ``src`` (the row of the stage's input every output row comes
from) and ``new`` (its moments are zero) -- the maker ASSERTS that every tensor the reference leaves behind is exactly that
gather of its input (bit for bit; moments zero where ``new``), except the computed tensors, which are stored in full in float32
and float64 with ``err_ref = max|f32 - f64|``, the reference's own float32 error and the unit of the device bounds.  ``eps`` is
re-indexed from (copy, rank) to (copy, source row) and stored as the API's ``noise``.
No decision quantity (mean gradient, scale norm, sigmoid of the opacity, max radius against its limit) lies within 1e-4 relative
of its threshold (asserted; the seed moves on until it holds), so float32 and float64 take the same decisions.
"""
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REF = "/root/reference"
BASE = os.path.join(REF, "custom", "threestudio-dreammesh4d", "geometry", "gaussian_base.py")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

from tests import density_control_common as cm  # noqa: E402

METHODS = ["densify_and_clone", "densify_and_split", "densification_postfix", "cat_tensors_to_optimizer", "_prune_optimizer",
           "prune_points", "replace_tensor_to_optimizer", "densify", "prune", "reset_opacity", "add_densification_stats",
           "update_states", "get_scaling", "get_opacity", "get_xyz"]
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
        "rotation": "_rotation", "normal": "_normal"}
N, SH, VIEWS, S = 400, 1, 3, 2
GRAD_T, SPLIT_T, MIN_OPA, SUGAR_T, MAX_NUM = 0.012, 0.035, 0.3, 0.5, 200
MARGIN = 1e-4


class _Torch:
    """torch, except zeros / normal / randperm / cuda.empty_cache (see the module docstring)."""

    def __init__(self):
        self.eps, self.perm = None, None
        self.cuda = types.SimpleNamespace(empty_cache=lambda: None)

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def zeros(*args, **kw):
        kw.pop("device", None)
        return torch.zeros(*args, **kw)

    def normal(self, mean, std):
        k = std.shape[0] // S
        eps = torch.cat([self.eps[c, :k] for c in range(S)]).to(std.dtype)
        return mean + std * eps

    def randperm(self, n):
        assert len(self.perm) == n
        return self.perm.clone()


def load_reference(proxy):
    tree = ast.parse(open(BASE).read())
    ns = {"torch": proxy, "nn": nn}
    top = {n.name: n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
    for name in ("build_rotation", "inverse_sigmoid"):
        exec(compile(ast.Module(body=[top[name]], type_ignores=[]), BASE, "exec"), ns)
    methods = {n.name: n for n in top["GaussianBaseModel"].body if isinstance(n, ast.FunctionDef)}
    body = []
    for name in METHODS:
        node = methods[name]
        node.returns = None
        for a in node.args.args + node.args.kwonlyargs:
            a.annotation = None
        body.append(node)
    cls = ast.ClassDef(name="Ref", bases=[], keywords=[], body=body, decorator_list=[])
    mod = ast.fix_missing_locations(ast.Module(body=[cls], type_ignores=[]))
    exec(compile(mod, BASE, "exec"), ns)
    return ns


def inputs(seed):
    """Seeded start: parameters after two CPU Adam steps with their moments, two sets of views, eps, the permutation."""
    st = cm.random_state(N, SH, seed, with_moments=False)
    rng = np.random.default_rng(seed + 1)
    params = {k: nn.Parameter(v.clone()) for k, v in st["params"].items()}
    opt = torch.optim.Adam([{"params": [p], "lr": 1e-3, "name": k} for k, p in params.items()], lr=0.0, eps=1e-15)
    for _ in range(2):
        for p in params.values():
            p.grad = torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32))
        opt.step()
    out = {"params": {k: p.detach().clone() for k, p in params.items()},
           "m1": {k: opt.state[p]["exp_avg"].clone() for k, p in params.items()},
           "m2": {k: opt.state[p]["exp_avg_sq"].clone() for k, p in params.items()}}

    def views(n):
        g = (rng.standard_normal((VIEWS, n, 3)) * 0.01).astype(np.float32)
        r = rng.integers(1, 40, (VIEWS, n)).astype(np.int32)
        r[rng.random((VIEWS, n)) < 0.5] = 0
        r[rng.random((VIEWS, n)) < 0.05] = -1
        r[rng.random((VIEWS, n)) < 0.03] = 150
        return torch.from_numpy(g), torch.from_numpy(r)

    out["views0"] = views(N)
    out["views1_full"] = views(3 * N)                    # cut to the row count after densify
    out["eps"] = torch.from_numpy(rng.standard_normal((S, 3 * N, 3)).astype(np.float32))
    out["fill"] = torch.from_numpy(rng.standard_normal((S, N, 3)).astype(np.float32))
    out["perm_seed"] = seed + 2
    return out


def make_self(ns, inp, dtype, sphere):
    me = ns["Ref"]()
    me.cfg = types.SimpleNamespace(pred_normal=True, sphere=sphere, split_thresh=SPLIT_T, prune_big_points=True, max_num=10 ** 9,
                                   sugar_prune_at=None, sugar_prune_threshold=SUGAR_T, prune_from_iter=0, prune_until_iter=10 ** 9,
                                   prune_interval=10 ** 9, opacity_reset_interval=10 ** 9, densify_from_iter=0,
                                   densify_until_iter=10 ** 9, densification_interval=10 ** 9, densify_grad_threshold=GRAD_T,
                                   min_opac_prune=MIN_OPA, radii2d_thresh=1000)
    groups = []
    for name in cm.NAMES:
        p = nn.Parameter(inp["params"][name].to(dtype).clone())
        setattr(me, ATTR[name], p)
        groups.append({"params": [p], "lr": 1e-3, "name": name})
    me.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for g in groups:
        p = g["params"][0]
        me.optimizer.state[p] = {"step": torch.tensor(2.0), "exp_avg": inp["m1"][g["name"]].to(dtype).clone(),
                                 "exp_avg_sq": inp["m2"][g["name"]].to(dtype).clone()}
    me.optimize_params = list(cm.NAMES)
    me.scaling_activation, me.scaling_inverse_activation = torch.exp, torch.log
    me.opacity_activation, me.inverse_opacity_activation = torch.sigmoid, ns["inverse_sigmoid"]
    me.xyz_gradient_accum, me.denom, me.max_radii2D = torch.zeros(N, 1, dtype=dtype), torch.zeros(N, 1, dtype=dtype), torch.zeros(N, dtype=dtype)
    return me


def snapshot(me):
    st = {"params": {}, "m1": {}, "m2": {}}
    for g in me.optimizer.param_groups:
        p = g["params"][0]
        assert getattr(me, ATTR[g["name"]]) is p and float(me.optimizer.state[p]["step"]) == 2.0
        st["params"][g["name"]] = p.detach().clone()
        st["m1"][g["name"]] = me.optimizer.state[p]["exp_avg"].clone()
        st["m2"][g["name"]] = me.optimizer.state[p]["exp_avg_sq"].clone()
    assert len(me.optimizer.state) == len(me.optimizer.param_groups)
    st.update(accum=me.xyz_gradient_accum.clone(), denom=me.denom.clone(), max_radii=me.max_radii2D.clone())
    return st


def check_margins(st64, sphere, stage):
    """True when the decisions of `stage` on the float64 state are clear of their thresholds."""
    clear = lambda v, t: bool(((v - t).abs() > MARGIN * abs(t)).all())
    if stage == "densify":
        g = st64["accum"] / st64["denom"]
        g[g.isnan()] = 0.0
        return clear(g, GRAD_T) and clear(torch.norm(cm.get_scaling(st64["params"]["scaling"], sphere), dim=1), SPLIT_T)
    opa = torch.sigmoid(st64["params"]["opacity"])
    if stage == "prune":
        return clear(opa, MIN_OPA) and clear(st64["max_radii"], float(st64["max_radii"].mean() * 3))
    return clear(opa, SUGAR_T)


def run(ns, proxy, inp, dtype, sphere):
    """The six stages on the reference; -> list of (stage, state after it), the margins' verdict, the views of stage 3."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        me = make_self(ns, inp, dtype, sphere)
        proxy.eps = inp["eps"]
        states, ok = [], True
        vsp = lambda g: [types.SimpleNamespace(grad=x.to(dtype)) for x in g]
        g0, r0 = inp["views0"]
        me.update_states(1, [r > 0 for r in r0], list(r0), vsp(g0))
        states.append(("stats", snapshot(me)))
        ok &= check_margins(snapshot(me), sphere, "densify")
        me.densify(GRAD_T)
        states.append(("densify", snapshot(me)))
        m1 = me._xyz.shape[0]
        g1, r1 = inp["views1_full"][0][:, :m1].contiguous(), inp["views1_full"][1][:, :m1].contiguous()
        pre = snapshot(me)
        pre = cm.stats(pre, g1.to(dtype), r1)
        ok &= check_margins(pre, sphere, "prune")
        me.cfg.prune_interval = 200
        me.cfg.densify_until_iter = 0
        me.update_states(200, [r > 0 for r in r1], list(r1), vsp(g1))
        me.cfg.prune_interval = 10 ** 9
        states.append(("prune", snapshot(me)))
        me.reset_opacity()
        states.append(("reset", snapshot(me)))
        ok &= check_margins(snapshot(me), sphere, "sugar")
        m3 = me._xyz.shape[0]
        assert m3 >= MAX_NUM + 100, m3
        proxy.perm = torch.randperm(m3, generator=torch.Generator().manual_seed(inp["perm_seed"]))
        me.cfg.max_num = MAX_NUM
        me.update_states(201, None, None, None)
        me.cfg.max_num = 10 ** 9
        states.append(("cap", snapshot(me)))
        me.cfg.sugar_prune_at = 202
        me.update_states(202, None, None, None)
        states.append(("sugar", snapshot(me)))
        return states, ok, (g1, r1), proxy.perm.clone()
    finally:
        torch.set_default_dtype(old)


def row_plan(prev, cur):
    """src / new of `cur`'s rows from `prev`'s.  `normal` and its first moment are never computed, and together with `xyz` they
    tell every row of `prev` apart (a clone has its source's values but zero moments, two children differ in xyz); a child row,
    whose xyz is computed, is found by `normal` alone among the rows with moments."""
    key = lambda st, i, with_xyz: (st["params"]["normal"][i].numpy().tobytes(), st["m1"]["normal"][i].numpy().tobytes(),
                                   st["params"]["xyz"][i].numpy().tobytes() if with_xyz else b"")
    n = prev["params"]["normal"].shape[0]
    exact = {key(prev, i, True): i for i in range(n)}
    assert len(exact) == n
    by_normal = {}
    for i in range(n):
        if bool((prev["m1"]["normal"][i] != 0).any()):
            by_normal[prev["params"]["normal"][i].numpy().tobytes()] = i
    new = (cur["m1"]["normal"] == 0).all(dim=1).numpy()
    src = np.empty(len(new), np.int32)
    for j in range(len(new)):
        hit = exact.get(key(cur, j, True))
        src[j] = hit if hit is not None else by_normal[cur["params"]["normal"][j].numpy().tobytes()]
    return src, new


def assert_is_gather(prev, cur, src, new, computed, stats_zero):
    """Everything the reference left in `cur` is prev[src], bit for bit (moments: zero where new), but for `computed`."""
    s = torch.from_numpy(src.astype(np.int64))
    for name in cm.NAMES:
        want = prev["params"][name][s]
        same = cm.bits(cur["params"][name]) == cm.bits(want)
        if name in computed:
            same = same.reshape(len(src), -1)[~computed[name]]
        assert same.all(), name
        for m in ("m1", "m2"):
            want = prev[m][name][s].clone()
            want[torch.from_numpy(new)] = 0
            if name in computed and computed[name].all():
                want[:] = 0                                # reset_opacity
            assert (cm.bits(cur[m][name]) == cm.bits(want)).all(), (m, name)
    for k in ("accum", "denom", "max_radii"):
        want = torch.zeros_like(cur[k]) if stats_zero else prev[k][s]
        assert (cm.bits(cur[k]) == cm.bits(want)).all(), k


def main():
    if not os.path.isdir(REF):
        sys.exit("needs /root/reference (authoring container only)")
    proxy = _Torch()
    ns = load_reference(proxy)
    seed = 100
    while True:
        inp = inputs(seed)
        runs = {}
        for case, sphere in (("A", False), ("B", True)):
            runs[case] = (run(ns, proxy, inp, torch.float32, sphere), run(ns, proxy, inp_f64(inp), torch.float64, sphere))
        if all(r32[1] and r64[1] for r32, r64 in runs.values()):
            break
        seed += 1
    out = {"seed": np.int64(seed), "grad_threshold": np.float64(GRAD_T), "split_thresh": np.float64(SPLIT_T), "min_opacity": np.float64(MIN_OPA),
           "sugar_threshold": np.float64(SUGAR_T), "max_num": np.int64(MAX_NUM), "perm_seed": np.int64(inp["perm_seed"])}
    for name in cm.NAMES:
        out[f"A/in/{name}"] = inp["params"][name].numpy()
        out[f"A/in/m1/{name}"] = inp["m1"][name].numpy()
        out[f"A/in/m2/{name}"] = inp["m2"][name].numpy()
    out["A/in/grad2d_0"], out["A/in/radii_0"] = (t.numpy() for t in inp["views0"])
    for case, (r32, r64) in runs.items():
        (s32, _, (g1, r1), perm), (s64, _, _, _) = r32, r64
        out[f"{case}/grad2d_1"], out[f"{case}/radii_1"], out[f"{case}/perm"] = g1.numpy(), r1.numpy(), perm.numpy()
        prev32 = cm.golden_inputs({k: v for k, v in out.items()}, "A")
        prev64 = cm.cast(prev32, torch.float64)
        for (stage, c32), (_, c64) in zip(s32, s64):
            p = f"{case}/{stage}/"
            if stage == "stats":
                src, new = np.arange(N, dtype=np.int32), np.zeros(N, bool)
                for k in ("denom", "max_radii"):
                    assert (c32[k].double() == c64[k]).all()
                    out[p + k] = c32[k].numpy()
                assert_is_gather(dict(prev32, accum=c32["accum"], denom=c32["denom"], max_radii=c32["max_radii"]), c32, src, new, {}, False)
                stored = {"accum": (c32["accum"], c64["accum"])}
            else:
                src, new = row_plan(prev32, c32)
                src64, new64 = row_plan(prev64, c64)
                assert (src == src64).all() and (new == new64).all(), "float32 and float64 took different decisions"
                computed = {}
                if stage == "densify":
                    child = new & (cm.bits(c32["params"]["xyz"]) != cm.bits(prev32["params"]["xyz"][torch.from_numpy(src.astype(np.int64))])).any(1)
                    computed = {"xyz": child, "scaling": child}
                    k = int(child.sum()) // S
                    first = len(src) - S * k
                    assert child[first:].all() and not child[:first].any()
                    noise = inp["fill"].clone()
                    for c in range(S):
                        noise[c, torch.from_numpy(src[first + c * k:first + (c + 1) * k].astype(np.int64))] = inp["eps"][c, :k]
                    out[f"{case}/noise"] = noise.numpy()
                    kinds = cm.kinds_densify(prev32, GRAD_T, SPLIT_T, case == "B").numpy()
                    counts = [int((kinds == q).sum()) for q in range(4)]
                    assert min(counts[0], counts[2], counts[3]) >= 30, counts
                    es, er = cm.expected_rows(kinds, S)
                    assert (es == src).all() and ((er > 0) == new).all()
                    print(f"case {case} densify: keep {counts[0]}, clone {counts[2]}, split {counts[3]} -> {len(src)} rows")
                    stored = {"xyz": (c32["params"]["xyz"], c64["params"]["xyz"]), "scaling": (c32["params"]["scaling"], c64["params"]["scaling"])}
                elif stage == "reset":
                    computed = {"opacity": np.ones(len(src), bool)}
                    stored = {"opacity": (c32["params"]["opacity"], c64["params"]["opacity"])}
                elif stage == "prune":
                    # the statistics of the second set of views went in before the prune: the gather is of the state after them
                    prev32, prev64 = cm.stats(prev32, g1, r1), cm.stats(prev64, g1.double(), r1)
                    stored = {"accum": (c32["accum"], c64["accum"])}
                    out[p + "denom"], out[p + "max_radii"] = c32["denom"].numpy(), c32["max_radii"].numpy()
                    assert len(prev32["params"]["xyz"]) - len(src) >= 30
                else:
                    stored = {}
                assert_is_gather(prev32, c32, src, new, computed, stage == "densify")
                print(f"case {case} {stage}: {len(prev32['params']['xyz'])} -> {len(src)} rows, {int(new.sum())} new")
            out[p + "src"], out[p + "new"] = src, new
            for k, (a32, a64) in stored.items():
                err = float((a32.double() - a64).abs().max())
                assert a32.dtype == torch.float32 and a64.dtype == torch.float64 and err > 0
                out[p + k], out[p + k + "_f64"], out[p + k + "_err_ref"] = a32.numpy(), a64.numpy(), np.float64(err)
                print(f"    {k}: err_ref {err:.3e}")
            prev32, prev64 = c32, c64
    path = os.path.join(OUT, "density_control.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes (seed {seed})")


def inp_f64(inp):
    """The same inputs with float64 parameters and moments (views, eps and the permutation seed as they are)."""
    out = dict(inp)
    for k in ("params", "m1", "m2"):
        out[k] = {n: v.double() for n, v in inp[k].items()}
    return out


if __name__ == "__main__":
    main()
