"""Shared by the density-control tests and tests/golden/make_golden_density_control.py: a restatement of the semantics in plain
torch (any dtype: float32 to compare row order and copies, float64 as the reference of computed values), the case builders and
the comparison helper.

The restatement is written from custom/threestudio-dreammesh4d/geometry/gaussian_base.py:575-579, 606-870 in MASK-INDEXING form
-- boolean masks, ``cat`` and ``repeat`` per tensor, clone first and split on the enlarged set second -- on purpose unlike the
kernels' classify -> scan -> gather.

A *state* is a dict: ``params`` name -> [N, ...], ``m1`` / ``m2`` name -> the Adam moments or None, ``accum`` [N,1], ``denom`` [N,1],
``max_radii`` [N].  Every function returns a new state plus ``src`` (the input row of every output row) and ``new`` (bool: the
row's moments are zero).
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "density_control.npz")
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "normal")
WIDTH_TAIL = {"xyz": (3,), "opacity": (1,), "scaling": (3,), "rotation": (4,), "normal": (3,)}


def param_shapes(sh_degree, pred_normal=True):
    k = (sh_degree + 1) ** 2 - 1
    shapes = dict(WIDTH_TAIL, f_dc=(1, 3), f_rest=(k, 3))
    return {n: shapes[n] for n in NAMES if pred_normal or n != "normal"}


def random_state(n, sh_degree, seed, pred_normal=True, with_moments=True, log_scale=-4.0):
    """Seeded float32 state: scales exp(N(log_scale, 0.5)) per axis, raw quaternions of norm 0.5 .. 2, logits N(0, 2)."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    params = {}
    for name, tail in param_shapes(sh_degree, pred_normal).items():
        params[name] = f(n, *tail)
    params["scaling"] = (log_scale + 0.5 * params["scaling"]).astype(np.float32)
    q = params["rotation"] / np.linalg.norm(params["rotation"], axis=1, keepdims=True)
    params["rotation"] = (q * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    params["opacity"] = (2.0 * params["opacity"]).astype(np.float32)
    st = {"params": {k: torch.from_numpy(v) for k, v in params.items()}}
    for m in ("m1", "m2"):
        st[m] = {k: (torch.from_numpy(np.abs(f(*v.shape)) * 1e-3) if with_moments else None) for k, v in params.items()}
    st["accum"] = torch.from_numpy(np.abs(f(n, 1)) * 0.02)
    st["denom"] = torch.from_numpy(rng.integers(0, 4, (n, 1)).astype(np.float32))
    st["max_radii"] = torch.from_numpy(rng.integers(0, 40, (n,)).astype(np.float32))
    return st


def cast(state, dtype=None, device=None):
    t = lambda v: None if v is None else v.to(dtype=dtype, device=device).clone()
    return {k: ({n: t(x) for n, x in v.items()} if isinstance(v, dict) else t(v)) for k, v in state.items()}


# ------------------------------------------------------------------------------------------------ the restatement
def build_rotation(r):
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), dtype=r.dtype)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - w * z)
    R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y)
    R[:, 2, 1] = 2 * (y * z + w * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def get_scaling(scaling, sphere):
    if sphere:
        return torch.exp(torch.mean(scaling, dim=-1).unsqueeze(-1).repeat(1, 3))
    return torch.exp(scaling)


def stats(state, grad2d, radii):
    """The loop of update_states (:846-852) over the views; visible = radii > 0."""
    out = cast(state)
    dt = out["accum"].dtype
    for b in range(grad2d.shape[0]):
        vis = radii[b] > 0
        out["max_radii"] = torch.max(out["max_radii"], radii[b].to(dt))
        out["accum"][vis] += torch.norm(grad2d[b].to(dt)[vis, :2], dim=-1, keepdim=True)
        out["denom"][vis] += 1
    return out


def _cat(state, src, extension):
    """cat_tensors_to_optimizer + densification_postfix: rows `src` appended with `extension` values, their moments zero."""
    out = {"params": {}, "m1": {}, "m2": {}}
    for name, p in state["params"].items():
        ext = extension[name] if name in extension else p[src]
        out["params"][name] = torch.cat((p, ext), dim=0)
        for m in ("m1", "m2"):
            mm = state[m][name]
            out[m][name] = None if mm is None else torch.cat((mm, torch.zeros_like(ext)), dim=0)
    n = out["params"]["xyz"].shape[0]
    dt = state["accum"].dtype
    out.update(accum=torch.zeros((n, 1), dtype=dt), denom=torch.zeros((n, 1), dtype=dt), max_radii=torch.zeros((n,), dtype=dt))
    return out


def prune(state, mask):
    """prune_points (:629-645): the rows where `mask` is false, everything row-selected.  -> state, src, new"""
    valid = ~mask
    out = {"params": {k: v[valid] for k, v in state["params"].items()}}
    for m in ("m1", "m2"):
        out[m] = {k: (None if v is None else v[valid]) for k, v in state[m].items()}
    out.update(accum=state["accum"][valid], denom=state["denom"][valid], max_radii=state["max_radii"][valid])
    src = torch.nonzero(valid).reshape(-1)
    return out, src, torch.zeros(len(src), dtype=torch.bool)


def densify(state, grad_threshold, split_thresh, sphere, noise, S=2):
    """densify (:800-805): clone, then split on the ENLARGED set with the gradient padded by zeros, then prune the split sources.
    noise [S,N,3] by copy and source row.  -> state, src (rows of the input state), new"""
    n = state["params"]["xyz"].shape[0]
    grads = state["accum"] / state["denom"]
    grads[grads.isnan()] = 0.0
    idx = torch.arange(n)
    # densify_and_clone
    sel = (torch.norm(grads, dim=-1) >= grad_threshold) & (torch.norm(get_scaling(state["params"]["scaling"], sphere), dim=1) <= split_thresh)
    st = _cat(state, sel, {})
    src = torch.cat((idx, idx[sel]))
    new = torch.cat((torch.zeros(n, dtype=torch.bool), torch.ones(int(sel.sum()), dtype=torch.bool)))
    # densify_and_split
    n1 = st["params"]["xyz"].shape[0]
    padded = torch.zeros(n1, dtype=grads.dtype)
    padded[:n] = grads.squeeze(-1)
    s_all = get_scaling(st["params"]["scaling"], sphere)
    sel2 = (padded >= grad_threshold) & (torch.norm(s_all, dim=1) > split_thresh)
    assert not bool(sel2[n:].any())
    stds = s_all[sel2].repeat(S, 1) / S
    eps = torch.cat([noise[c].to(stds.dtype)[src[sel2]] for c in range(S)])
    samples = stds * eps
    rots = build_rotation(st["params"]["rotation"][sel2]).repeat(S, 1, 1)
    ext = {"xyz": torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + st["params"]["xyz"][sel2].repeat(S, 1),
           "scaling": torch.log(s_all[sel2].repeat(S, 1) / (0.8 * S))}
    for name, p in st["params"].items():
        if name not in ext:
            ext[name] = p[sel2].repeat(S, *([1] * (p.ndim - 1)))
    k = int(sel2.sum())
    st2 = _cat(st, None, ext)
    src = torch.cat((src, src[sel2].repeat(S)))
    new = torch.cat((new, torch.ones(S * k, dtype=torch.bool)))
    out, kept, _ = prune(st2, torch.cat((sel2, torch.zeros(S * k, dtype=torch.bool))))
    return out, src[kept], new[kept]


def prune_mask(state, min_opacity, big_points):
    mask = (torch.sigmoid(state["params"]["opacity"]) < min_opacity).squeeze(-1)
    if big_points:
        mask = mask | (state["max_radii"] > torch.mean(state["max_radii"]) * 3)
    return mask


def reset_opacity(state):
    out = cast(state)
    x = torch.sigmoid(out["params"]["opacity"]) * 0.9
    out["params"]["opacity"] = torch.log(x / (1 - x))
    for m in ("m1", "m2"):
        if out[m]["opacity"] is not None:
            out[m]["opacity"] = torch.zeros_like(out[m]["opacity"])
    return out


def kinds_densify(state, grad_threshold, split_thresh, sphere):
    """kind per row (0 keep, 2 clone, 3 split) by the same masks."""
    g = state["accum"] / state["denom"]
    g[g.isnan()] = 0.0
    hot = torch.norm(g, dim=-1) >= grad_threshold
    big = torch.norm(get_scaling(state["params"]["scaling"], sphere), dim=1) > split_thresh
    kind = torch.zeros(len(hot), dtype=torch.uint8)
    kind[hot & ~big] = 2
    kind[hot & big] = 3
    return kind


def children(params, sources, noise, S, sphere):
    """(xyz, scaling) of the S * len(sources) child rows of densify_and_split (:732-741), copy-major, in the dtype of `params`."""
    sel = torch.zeros(params["xyz"].shape[0], dtype=torch.bool)
    sel[torch.as_tensor(np.asarray(sources, np.int64))] = True
    s_all = get_scaling(params["scaling"], sphere)
    stds = s_all[sel].repeat(S, 1) / S
    samples = stds * torch.cat([noise[c].to(stds.dtype)[sel] for c in range(S)])
    rots = build_rotation(params["rotation"][sel]).repeat(S, 1, 1)
    xyz = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + params["xyz"][sel].repeat(S, 1)
    return xyz, torch.log(s_all[sel].repeat(S, 1) / (0.8 * S))


def expected_rows(kind, S=2):
    """(src, role) of the output rows of `kind` (numpy uint8), by mask indexing."""
    kind = np.asarray(kind) & 3
    idx = np.arange(len(kind))
    kept, clone, split = idx[(kind == 0) | (kind == 2)], idx[kind == 2], idx[kind == 3]
    src = np.concatenate([kept, clone] + [split] * S)
    role = np.concatenate([np.zeros(len(kept)), np.ones(len(clone))] + [np.full(len(split), 2 + c) for c in range(S)])
    return src.astype(np.int32), role.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ golden and comparison
STAGES = ("stats", "densify", "prune", "reset", "cap", "sugar")


def golden():
    return np.load(GOLDEN)


def golden_inputs(z, case):
    """The float32 start state of a golden case (after the two Adam steps) and its configuration."""
    p = f"{case}/in/"
    st = {"params": {}, "m1": {}, "m2": {}}
    for name in NAMES:
        st["params"][name] = torch.from_numpy(z[p + name])
        st["m1"][name] = torch.from_numpy(z[p + "m1/" + name])
        st["m2"][name] = torch.from_numpy(z[p + "m2/" + name])
    n = st["params"]["xyz"].shape[0]
    st.update(accum=torch.zeros(n, 1), denom=torch.zeros(n, 1), max_radii=torch.zeros(n))
    return st


def _gather(prev, src, new):
    s = torch.from_numpy(np.asarray(src, np.int64))
    out = {"params": {k: v[s] for k, v in prev["params"].items()}}
    for m in ("m1", "m2"):
        out[m] = {}
        for k, v in prev[m].items():
            out[m][k] = v[s].clone()
            out[m][k][torch.from_numpy(np.asarray(new, bool))] = 0
    out.update(accum=prev["accum"][s], denom=prev["denom"][s], max_radii=prev["max_radii"][s])
    return out


def golden_stages(z, case):
    """What the REFERENCE left behind after every stage of a golden case, put together from the fixture alone: a list of dicts
    ``stage``, ``state`` (float32; copied rows are the gather ``src`` of the stage before, computed tensors as stored), ``src``,
    ``new``, ``computed`` name -> (float64 values, err_ref, bool mask of the rows that are computed and not copies)."""
    T = torch.from_numpy
    prev, out = golden_inputs(z, "A"), []
    for stage in STAGES:
        p = f"{case}/{stage}/"
        src, new = z[p + "src"], z[p + "new"]
        st = _gather(prev, src, new)
        every = np.ones(len(src), bool)
        computed = {}
        if stage in ("stats", "prune"):
            st.update(accum=T(z[p + "accum"]), denom=T(z[p + "denom"]), max_radii=T(z[p + "max_radii"]))
            computed["accum"] = (z[p + "accum_f64"], float(z[p + "accum_err_ref"]), every)
        elif stage == "densify":
            child = new & (bits(T(z[p + "xyz"])) != bits(st["params"]["xyz"])).any(1)
            for k in ("xyz", "scaling"):
                st["params"][k] = T(z[p + k])
                computed[k] = (z[p + k + "_f64"], float(z[p + k + "_err_ref"]), child)
            n = len(src)
            st.update(accum=torch.zeros(n, 1), denom=torch.zeros(n, 1), max_radii=torch.zeros(n))
        elif stage == "reset":
            st["params"]["opacity"] = T(z[p + "opacity"])
            st["m1"]["opacity"], st["m2"]["opacity"] = torch.zeros(len(src), 1), torch.zeros(len(src), 1)
            computed["opacity"] = (z[p + "opacity_f64"], float(z[p + "opacity_err_ref"]), every)
        out.append({"stage": stage, "state": st, "src": src, "new": new, "computed": computed})
        prev = st
    return out


def replay(z, case, dtype):
    """The restatement through the six stages of a golden case in `dtype` -> list of (stage, state, src, new)."""
    sphere = case == "B"
    T = torch.from_numpy
    gt, st_, mo, su, mx = (float(z[k]) for k in ("grad_threshold", "split_thresh", "min_opacity", "sugar_threshold", "max_num"))
    st = cast(golden_inputs(z, "A"), dtype)
    n = st["params"]["xyz"].shape[0]
    out = []
    st = stats(st, T(z["A/in/grad2d_0"]), T(z["A/in/radii_0"]))
    out.append(("stats", st, torch.arange(n), torch.zeros(n, dtype=torch.bool)))
    st, src, new = densify(st, gt, st_, sphere, T(z[f"{case}/noise"]), 2)
    out.append(("densify", st, src, new))
    st = stats(st, T(z[f"{case}/grad2d_1"]), T(z[f"{case}/radii_1"]))
    st, src, new = prune(st, prune_mask(st, mo, True))
    out.append(("prune", st, src, new))
    st = reset_opacity(st)
    m = st["params"]["xyz"].shape[0]
    out.append(("reset", st, torch.arange(m), torch.zeros(m, dtype=torch.bool)))
    st, src, new = prune(st, T(z[f"{case}/perm"]) > mx)
    out.append(("cap", st, src, new))
    st, src, new = prune(st, prune_mask(st, su, False))
    out.append(("sugar", st, src, new))
    return out


CHAIN = ("xyz", "scaling", "opacity", "accum")            # tensors that hold computed values at some stage


def compare_state(got, want, what, factor=None, atol=None, prev=None):
    """`got` (a state, any device / dtype) against one entry of ``golden_stages``: row count, every copied row bit for bit (when
    `got` is float32), computed values per element within ``factor * err_ref`` (or `atol`) of the float64 golden.  Returns the
    largest error / err_ref per computed tensor.

    `prev`: the state `got` was made from (a copy taken before the stage).  The ``CHAIN`` tensors hold values an earlier stage
    COMPUTED, equal to the reference's only within that stage's bound, so their copied rows are compared bit for bit with the
    gather ``prev[src]`` (moments zero where new) -- the reference's own relation between the two states, which the maker
    asserted -- where all other tensors are compared with the reference's bits themselves."""
    exp, computed = want["state"], want["computed"]
    if prev is not None:
        own = _gather(cast(prev, device="cpu"), want["src"], want["new"])
        exp = {"params": dict(exp["params"]), "m1": exp["m1"], "m2": exp["m2"], "accum": exp["accum"], "denom": exp["denom"],
               "max_radii": exp["max_radii"]}
        for name in CHAIN:
            if name == "accum":
                if want["stage"] != "densify":              # zeros after densify, as the reference's
                    exp["accum"] = own["accum"]
            else:
                exp["params"][name] = own["params"][name]
    f32 = got["accum"].dtype == torch.float32
    ratios = {}

    def one(name, g, e):
        assert g is not None, f"{what}: {name} is missing"
        g = g.detach().cpu()
        assert tuple(g.shape) == tuple(e.shape), f"{what}: {name} has shape {tuple(g.shape)}, the reference {tuple(e.shape)}"
        if name in computed:
            f64, err_ref, rows = computed[name]
            if f32 and not rows.all():
                assert_bit_equal(g[torch.from_numpy(~rows)], e[torch.from_numpy(~rows)], f"{what}: copied rows of {name}")
            if atol is not None:
                err = float(np.abs(g.numpy().astype(np.float64) - f64).max())
                assert err <= atol, f"{what}: {name} differs from the float64 golden by {err:.3e} > {atol}"
            else:
                ratios[name] = assert_within(g, f64, err_ref, f"{what}: {name}", factor)
        elif f32:
            assert_bit_equal(g, e, f"{what}: {name}")
        elif name not in CHAIN:      # a float64 run: these carry float64 results of earlier stages
            assert torch.equal(g, e.to(g.dtype)), f"{what}: {name} is not the float32 golden's copy"

    for name, e in exp["params"].items():
        one(name, got["params"][name], e)
        for m in ("m1", "m2"):
            one(f"{m}/{name}", got[m][name], exp[m][name])
    for name in ("accum", "denom", "max_radii"):
        one(name, got[name], exp[name])
    return ratios


def restatement_unit(w32, w64):
    """The unit of a device bound where no golden err_ref exists: the restatement's own float32 error against float64, but no
    less than half an ulp of the tensor's largest magnitude -- over a handful of elements (N = 1) the observed error of a
    correctly rounded result can be anywhere between 0 and that, and a sample that happens to round well is no bound."""
    half_ulp = float(np.spacing(np.float32(w64.abs().max().item()))) / 2 if w64.numel() else 0.0
    return max(float((w32.double() - w64).abs().max()) if w64.numel() else 0.0, half_ulp)


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_bit_equal(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    bad = np.flatnonzero((g != w).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} elements differ in their bits, first at flat index {bad[0]}"


def assert_within(got, f64, err_ref, what, factor=4.0):
    """Per element |got - f64| <= factor * err_ref; prints and returns the largest ratio."""
    g = got.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got) else np.asarray(got, np.float64)
    w = f64.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(f64) else np.asarray(f64, np.float64)
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    assert np.isfinite(g).all(), f"{what}: non-finite values"
    err = np.abs(g - w)
    ratio = float(err.max() / err_ref) if err.size else 0.0
    print(f"{what}: max |got - f64| = {err.max() if err.size else 0.0:.3e}, err_ref = {err_ref:.3e}, ratio = {ratio:.3f} (bound {factor})")
    assert ratio <= factor, f"{what}: max error {err.max():.3e} is {ratio:.2f} x err_ref = {err_ref:.3e} (bound {factor})"
    return ratio
