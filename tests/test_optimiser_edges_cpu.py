"""Pins the reference, the restatement, the cases and the yardsticks that tests/test_optimiser_edges_gpu.py judges csrc/gradpack.hip
by, and runs what needs no device (CPU only).

* The yardsticks are re-measured: 0.8 x constant <= measured <= constant.  The case list reaches what it claims.
* The float32 restatement meets the float64 bound on every case, whole, sliced, masked and along the trajectory.
* One-token mutants of the restatement, fed to the comparison functions in place of the device output: each is rejected.
* distributed.ShardedAdamW with `fused = False` (the torch-operator form, CPU tensors) through every case it can express and along
  the trajectory, against the same reference and bounds.
* The host refusals of dm4d_grad_pack / _unpack / dm4d_adamw_message / dm4d_adamw_step: each returns before any launch.
"""
import ctypes as C

import numpy as np
import pytest

from tests import optimiser_edges as oe

ALL = oe.CASES + list(oe.MESSAGE_CASES)


# ------------------------------------------------------------------------------------------------ yardsticks, cases, restatement
def test_yardsticks_are_what_the_restatement_measures():
    worst = {}
    for name in ALL:
        for k, w in oe.yard_units(name).items():
            worst[k] = max(worst.get(k, (0.0, None)), (w, name))
    print({k: (round(w, 4), n) for k, (w, n) in worst.items()})
    for k, const in oe.YARD.items():
        assert 0.8 * const <= worst[k][0] <= const, (k, worst[k], const)


def test_cases_reach_what_they_claim():
    oe.assert_reach()
    total = sum(oe.problem(n)[1]["total"] for n in ALL)
    assert total < 2_000_000, total
    for n in ALL:                                                   # index lists: sorted, unique, first and last storage element
        bufs, call = oe.problem(n)
        for s in call["segs"]:
            if s["index"] is not None and s["count"] >= 2:
                ix = bufs[s["index"][0]]
                assert (np.diff(ix) > 0).all() and ix[0] == 0 and ix[-1] == len(bufs[s["param"][0]]) - 1


@pytest.mark.parametrize("name", ALL)
def test_restatement_meets_the_float64_bound(name):
    bufs, call = oe.problem(name)
    worst, fails = oe.judge(call, oe.run_f32(bufs, call), oe.reference(name), name)
    assert not fails, "\n".join(fails)
    assert 0 < worst["param"] <= 1 and worst["exp_avg"] <= 1 and worst["exp_avg_sq"] <= 1


def _run_slices(bufs, calls, mut=()):
    out, refs = None, None
    for c in calls:
        out = oe.run_f32(bufs, c, mut, out={k: v.copy() for k, v in bufs.items()} if out is None else out)
        refs = oe.run_f64(bufs, c, refs)
    return out, refs


def test_sliced_restatement_equals_the_whole_message_one():
    bufs, call = oe.problem(oe.SLICED)
    whole = oe.run_f32(bufs, call)
    sb, calls = oe.slice_calls(oe.SLICED)
    out, refs = _run_slices(sb, calls)
    names = [k for k in whole if k[0] == "P"] + ["M", "V", "OUT"]
    assert oe.not_identical(out, whole, names) == 0
    fails = [f for c in calls for f in oe.judge(c, out, refs, "slices")[1]]
    assert not fails, "\n".join(fails)
    # a masked call and skipped segments: nothing moves, the send slices hold the current values
    for masked, skip in ((True, ()), (False, oe.SLICE_SKIP)):
        sb, calls = oe.slice_calls(oe.SLICED, masked=masked, skip=skip)
        out, refs = _run_slices(sb, calls)
        assert not [f for c in calls for f in oe.judge(c, out, refs, "slices")[1]]
        for k in (range(len(call["segs"])) if masked else skip):
            s = call["segs"][k]
            assert oe.same_bits(out[f"P{k}"], bufs[f"P{k}"])
            cur = bufs[f"P{k}"] if s["index"] is None else bufs[f"P{k}"][bufs[f"IX{k}"]]
            assert oe.same_bits(out["OUT"][oe.GUARD + s["offset"]:oe.GUARD + s["offset"] + s["count"]], cur)


def _trajectory(step_fn):
    """Drive the 6-step trajectory: `step_fn(t, bufs, call)` -> buffers after step t; the reference restarts from them."""
    start = oe.trajectory_start()
    params, index = [p for p, _ in start], [ix for _, ix in start]
    n = sum(c for c, _ in oe.TRAJECTORY_SEGMENTS)
    m, v, steps, pend = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(len(start)), np.ones(len(start))
    worst = {}
    for t in range(len(oe.TRAJECTORY)):
        bufs, call = oe.trajectory_call(t, params, index, m, v, steps, pend)
        out = step_fn(t, bufs, call)
        refs = oe.run_f64(bufs, call)
        w, fails = oe.judge(call, out, refs if "scal" in out else oe.message_only(refs, call), f"trajectory step {t}")
        assert not fails, "\n".join(fails)
        for k, x in w.items():
            worst[k] = max(worst.get(k, 0.0), x)
        params = [np.asarray(out[f"P{k}"]) for k in range(len(start))]
        m, v, steps, pend = (np.asarray(out[k]) for k in ("M", "V", "step", "pending"))
    assert steps.tolist() == [4.0, 3.0, 3.0, 4.0]                      # two masked steps, segments 1 and 2 skipped once each
    return worst


def test_trajectory_of_the_restatement():
    print(_trajectory(lambda t, bufs, call: oe.run_f32(bufs, call)))


# ------------------------------------------------------------------------------------------------ mutants
def _mutant_rejected(mut):
    if mut == "unpack_no_scale":
        bufs, call = oe.problem("len-indexed-seventh")
        b = dict(bufs, MSG=oe.pack_reference(bufs, call["segs"]))
        want, got = oe.unpack_reference(b, call["segs"], 1.0 / 3.0), oe.unpack_reference(b, call["segs"], 1.0 / 3.0, (mut,))
        return any(not oe.same_bits(got[k], want[k]) for k in want)
    if mut in ("index_shift", "last_unwritten", "neighbour_overwritten"):      # ... also in pack
        bufs, call = oe.problem("len-indexed-seventh")
        if oe.same_bits(oe.pack_reference(bufs, call["segs"], (mut,)), oe.pack_reference(bufs, call["segs"])):
            return False
    if mut == "grad_at_e":
        sb, calls = oe.slice_calls(oe.SLICED)
        out, refs = _run_slices(sb, calls, (mut,))
        return any(oe.judge(c, out, refs, mut)[1] for c in calls)
    if mut == "step_on_masked":
        bufs, call = oe.whole_call("hyper-a-first", masked=True)
        return bool(oe.judge(call, oe.run_f32(bufs, call, (mut,)), oe.run_f64(bufs, call), mut)[1])
    for name in ALL:
        bufs, call = oe.problem(name)
        if oe.judge(call, oe.run_f32(bufs, call, (mut,)), oe.reference(name), mut)[1]:
            return True
    return False


@pytest.mark.parametrize("mut", oe.MUTANTS)
def test_mutant_is_rejected(mut):
    assert _mutant_rejected(mut), f"the bound or the cases are too loose: mutant {mut} passes every case"


def test_lerp_forms_agree_only_at_their_equality_point():
    """beta1 = 0.5: both forms of torch.lerp have the same weights -- the mutant that swaps them is invisible there and only there."""
    hit = {}
    for name in ("hyper-a-seventh", "hyper-b-seventh"):
        bufs, call = oe.problem(name)
        out, mutant = oe.run_f32(bufs, call), oe.run_f32(bufs, call, ("lerp_other_weight",))
        for k, s in enumerate(call["segs"]):
            lr, b1 = call["hyper"][s["group"]][:2]
            if lr == 0.0:                                               # (no update to see the moment in)
                continue
            hit.setdefault(b1, []).append(oe.same_bits(out[f"P{k}"], mutant[f"P{k}"]))
    assert all(hit[0.5]) and not any(x for b1, v in hit.items() if b1 != 0.5 for x in v)


# ------------------------------------------------------------------------------------------------ ShardedAdamW, torch-operator form
def sharded_step(bufs, call, device, fused, state=None):
    """One step of distributed.ShardedAdamW over the problem's parameters FROM the problem's state -> the buffers after it
    (P{k}, M, V, step, pending).  `state`: (params, optimiser) of an earlier call to continue with (the trajectory)."""
    import torch

    from dreammesh4d_amd import distributed as D

    segs = call["segs"]
    assert call["m"][1] in (0, oe.GUARD) and all(s["pout"] is None and not s["gmsg"] for s in segs) and call["gs"] == 1.0

    def tensor(arr, mode):
        shape = oe.storage_shape(len(arr), "dense") if mode in ("dense", "null") else None
        if mode == "cl":
            t = torch.empty((1, 4, len(arr) // 8, 2), device=device).contiguous(memory_format=torch.channels_last)
        elif mode == "ix":
            t = torch.empty((1, 4, len(arr) // 8, 2), device=device)
        else:
            t = torch.empty(shape, device=device)
        D.storage_flat(t).copy_(torch.from_numpy(np.ascontiguousarray(arr)))
        return t

    if state is None:
        params = [torch.nn.Parameter(tensor(bufs[f"P{k}"], s["mode"])) for k, s in enumerate(segs)]
        touched = {p: torch.from_numpy(bufs[s["index"][0]]).to(device) for p, s in zip(params, segs) if s["index"] is not None}
        groups = [{"params": [p for p, s in zip(params, segs) if s["group"] == g], "lr": h[0], "betas": (h[1], h[2]), "eps": h[3], "weight_decay": h[4]}
                  for g, h in enumerate(call["hyper"])]
        opt = D.ShardedAdamW(groups, D.GradAllReducer(params, touched=touched))
        opt.fused = fused
        lo = call["m"][1]
        opt.exp_avg.copy_(torch.from_numpy(bufs["M"][lo:lo + call["total"]]))
        opt.exp_avg_sq.copy_(torch.from_numpy(bufs["V"][lo:lo + call["total"]]))
        opt.step_t.copy_(torch.from_numpy(bufs["step"]))
        opt.pending_decay.copy_(torch.from_numpy(bufs["pending"]))
    else:
        params, opt = state
    for g, h in zip(opt.param_groups, call["hyper"]):
        g["lr"] = h[0]
    for k, (p, s) in enumerate(zip(params, segs)):
        p.grad = None if s["skip"] else tensor(bufs[f"G{k}"], s["mode"])
    fi = call["found_inf"]
    opt.step(found_inf=None if fi is None else torch.tensor(fi, device=device))
    out = {f"P{k}": D.storage_flat(p.data).cpu().numpy().copy() for k, p in enumerate(params)}
    out.update(M=opt.exp_avg.cpu().numpy().copy(), V=opt.exp_avg_sq.cpu().numpy().copy(), step=opt.step_t.cpu().numpy().copy(),
               pending=opt.pending_decay.cpu().numpy().copy())
    return out, (params, opt)


@pytest.mark.parametrize("name", oe.EXPRESSIBLE)
def test_torch_operator_form_meets_the_float64_bound(name):
    bufs, call = oe.problem(name)
    out, _ = sharded_step(bufs, call, "cpu", False)
    worst, fails = oe.judge(call, out, oe.message_only(oe.reference(name), call), f"{name} (torch operators)")
    print(name, {k: round(v, 3) for k, v in worst.items()})
    assert not fails, "\n".join(fails)


def test_torch_operator_form_along_the_trajectory():
    state = [None]

    def step(t, bufs, call):
        out, state[0] = sharded_step(bufs, call, "cpu", False, state[0])
        return out

    print(_trajectory(step))


def test_more_than_64_gradient_tensors_are_refused():
    import torch

    from dreammesh4d_amd import distributed as D

    params = [torch.nn.Parameter(torch.zeros(3)) for _ in range(oe.MAX_SEG + 1)]
    with pytest.raises(ValueError, match="more than 64"):
        D.GradAllReducer(params)._segments(False)
    D.GradAllReducer(params[:oe.MAX_SEG])._segments(False)


# ------------------------------------------------------------------------------------------------ host refusals
P = 0x1000          # a non-null pointer no refused call ever follows


def _valid(n_seg=2, n_groups=2):
    from dreammesh4d_amd import _lib

    seg, a, old = _lib.GradSegments(), _lib.AdamwStepArgs(), _lib.AdamwArgs()
    seg.n_segments = n_seg
    for k in range(n_seg):
        seg.grad[k], seg.index[k], seg.count[k], seg.offset[k] = P, None, 8, 8 * k
        a.group[k], a.param[k] = k % n_groups, P
        old.group[k], old.param[k] = k % n_groups, P
    a.n_groups = old.n_groups = n_groups
    for g in range(n_groups):
        a.lr[g], a.beta1[g], a.beta2[g], a.eps[g], a.weight_decay[g] = 1e-2, 0.9, 0.99, 1e-15, 0.01
        old.lr[g] = 1e-2
    old.beta1, old.beta2, old.eps, old.weight_decay = 0.9, 0.99, 1e-15, 0.01
    for x in (a, old):
        x.exp_avg, x.exp_avg_sq, x.step, x.pending_decay, x.found_inf, x.scratch = P, P, P, None, None, P
    return seg, a, old


def _set(obj, field, k, value):
    if k is None:
        setattr(obj, field, value)
    else:
        getattr(obj, field)[k] = value


# name -> (which struct, field, index, value, functions that must refuse, text in dm4d_last_error())
SEG_FNS = ("dm4d_grad_pack", "dm4d_grad_unpack", "dm4d_adamw_message", "dm4d_adamw_step")
REFUSALS = {
    "65 segments": ("seg", "n_segments", None, 65, SEG_FNS, "bad count"),
    "negative segment count": ("seg", "n_segments", None, -1, SEG_FNS, "bad count"),
    "negative count": ("seg", "count", 1, -1, SEG_FNS, "negative count/offset"),
    "negative offset": ("seg", "offset", 0, -4, SEG_FNS, "negative count/offset"),
    "unpack with a NULL gradient tensor": ("seg", "grad", 1, None, ("dm4d_grad_unpack",), "unpack needs every gradient tensor"),
    "group out of range": ("args", "group", 1, 2, ("dm4d_adamw_message", "dm4d_adamw_step"), "in group 2"),
    "negative group": ("args", "group", 0, -1, ("dm4d_adamw_message", "dm4d_adamw_step"), "in group -1"),
    "0 groups": ("args", "n_groups", None, 0, ("dm4d_adamw_message", "dm4d_adamw_step"), "0 groups"),
    "9 groups": ("args", "n_groups", None, 9, ("dm4d_adamw_message", "dm4d_adamw_step"), "9 groups"),
    "beta1 = 1": ("args", "beta1", 1, 1.0, ("dm4d_adamw_message", "dm4d_adamw_step"), "out of range"),
    "beta1 < 0": ("args", "beta1", 0, -0.1, ("dm4d_adamw_message", "dm4d_adamw_step"), "out of range"),
    "beta2 = 1": ("args", "beta2", 0, 1.0, ("dm4d_adamw_message", "dm4d_adamw_step"), "out of range"),
    "beta2 NaN": ("args", "beta2", 1, float("nan"), ("dm4d_adamw_message", "dm4d_adamw_step"), "out of range"),
    "negative eps": ("args", "eps", 1, -1e-15, ("dm4d_adamw_message", "dm4d_adamw_step"), "out of range"),
    "NULL parameter on a non-empty segment": ("args", "param", 1, None, ("dm4d_adamw_message", "dm4d_adamw_step"), "null parameter storage (segment 1)"),
    "NULL moments": ("args", "exp_avg_sq", None, None, ("dm4d_adamw_message", "dm4d_adamw_step"), "null state"),
    "NULL scratch": ("args", "scratch", None, None, ("dm4d_adamw_message", "dm4d_adamw_step"), "null state"),
    "grad_in_message with a NULL gradient": ("args", "grad_in_message", 0, 1, ("dm4d_adamw_step",), "a message-layout gradient cannot be NULL"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_entry_point_refuses_before_any_launch(name):
    from dreammesh4d_amd import _lib

    which, field, k, value, fns, text = REFUSALS[name]
    L = _lib.lib()
    for fn in fns:
        seg, a, old = _valid()
        args = old if fn == "dm4d_adamw_message" else a
        if which == "seg":
            _set(seg, field, k, value)
        elif fn == "dm4d_adamw_message" and field in ("beta1", "beta2", "eps"):      # one set of hyperparameters: not indexed
            _set(args, field, None, value)
        else:
            _set(args, field, k, value)
        if name.startswith("grad_in_message"):
            seg.grad[0] = None
        call = {"dm4d_grad_pack": lambda: L.dm4d_grad_pack(C.byref(seg), P, None),
                "dm4d_grad_unpack": lambda: L.dm4d_grad_unpack(C.byref(seg), P, 1.0, None),
                "dm4d_adamw_message": lambda: L.dm4d_adamw_message(C.byref(seg), C.byref(args), 1.0, None),
                "dm4d_adamw_step": lambda: L.dm4d_adamw_step(C.byref(seg), C.byref(args), 1.0, None)}[fn]
        rc = call()
        assert rc == _lib._CONSTANTS["DM4D_ERR_INVALID"] and text in L.dm4d_last_error().decode(), (fn, rc, L.dm4d_last_error().decode())


def test_null_message_and_null_arguments_are_refused():
    from dreammesh4d_amd import _lib

    L = _lib.lib()
    seg, a, old = _valid()
    bad = _lib._CONSTANTS["DM4D_ERR_INVALID"]
    assert L.dm4d_grad_pack(C.byref(seg), None, None) == bad and "null message" in L.dm4d_last_error().decode()
    assert L.dm4d_grad_unpack(C.byref(seg), None, 1.0, None) == bad and "null message" in L.dm4d_last_error().decode()
    assert L.dm4d_grad_pack(None, P, None) == bad and L.dm4d_adamw_step(C.byref(seg), None, 1.0, None) == bad
    assert L.dm4d_adamw_message(C.byref(seg), None, 1.0, None) == bad
    seg.n_segments = 0                                              # nothing to do is not an error, and launches nothing
    assert L.dm4d_grad_pack(C.byref(seg), None, None) == _lib.OK and L.dm4d_grad_unpack(C.byref(seg), None, 1.0, None) == _lib.OK
