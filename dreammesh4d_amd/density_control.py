"""Adaptive density control of free Gaussians on the HIP device: a functional layer over device tensors.

Replaces the density control of ``GaussianBaseModel`` (custom/threestudio-dreammesh4d/geometry/gaussian_base.py:575-579,
606-870: boolean-mask indexing, ``repeat``, ``cat`` and ``bmm`` over seven parameter tensors and fourteen moment tensors) with the
kernels of ``csrc/density_control.hip`` (C ABI ``include/dm4d_density.h``; DESIGN.md, "Adaptive density control"):

* ``accumulate_stats``   the statistics of all views of a step in one launch
* ``classify_densify`` / ``classify_prune``   -> ``kind`` [N] uint8 (KEEP, DROP, CLONE, SPLIT); a boolean mask is a valid kind
* ``apply``              plan (reduce-then-scan), ONE host read of the four counts, one row move for all arrays and moments, the
                         split children's ``xyz`` and ``scaling``
* ``reset_opacity``

The output order is the reference's: kept originals by ascending index, clones by ascending source, then child 0 of every split
source by ascending index, child 1, ...  There is no CPU path.
"""
import ctypes

import torch

from . import _lib
from ._args import no_cpu_path as _no_cpu_path

KEEP, DROP, CLONE, SPLIT = _lib.DM4D_DC_KEEP, _lib.DM4D_DC_DROP, _lib.DM4D_DC_CLONE, _lib.DM4D_DC_SPLIT
ROLE_KEPT, ROLE_CLONE, ROLE_CHILD = _lib.DM4D_DC_ROLE_KEPT, _lib.DM4D_DC_ROLE_CLONE, _lib.DM4D_DC_ROLE_CHILD
MAX_ARRAYS = _lib.DM4D_DC_MAX_ARRAYS


def _device_of(what, *tensors):
    """The one HIP device all of `tensors` (None skipped) live on."""
    ts = [t for t in tensors if t is not None]
    for t in ts:
        if not torch.is_tensor(t):
            raise TypeError(f"{what}: expected torch tensors (got {type(t).__name__})")
    dev = ts[0].device
    if dev.type != "cuda" or any(t.device != dev for t in ts):
        raise _no_cpu_path(what)
    return dev


def _flat(what, name, t, n, dtype=torch.float32):
    """`t` as it is when it is a contiguous `dtype` tensor of n elements; otherwise an error (in-place outputs are never copied)."""
    if t.dtype != dtype or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} tensor of {n} elements (got {t.dtype} {tuple(t.shape)})")
    return t


def accumulate_stats(grad2d, radii, accum, denom, max_radii):
    """In place, for the B views of one step: ``accum[i] += |grad2d[b,i,:2]|`` and ``denom[i] += 1`` where ``radii[b,i] > 0``,
    views in ascending order; ``max_radii[i] = max(max_radii[i], radii[b,i])`` for every view.

    grad2d [B,N,3] float32 (the ``.grad`` of the viewspace points), radii [B,N] int32, accum / denom [N] or [N,1] float32,
    max_radii [N] float32."""
    what = "accumulate_stats"
    dev = _device_of(what, grad2d, radii, accum, denom, max_radii)
    if grad2d.ndim != 3 or grad2d.shape[2] != 3 or grad2d.dtype != torch.float32:
        raise ValueError(f"{what}: grad2d must be float32 [B,N,3] (got {grad2d.dtype} {tuple(grad2d.shape)})")
    B, N = int(grad2d.shape[0]), int(grad2d.shape[1])
    if tuple(radii.shape) != (B, N):
        raise ValueError(f"{what}: radii must be [{B},{N}] (got {tuple(radii.shape)})")
    grad2d = grad2d.detach().contiguous()
    radii = radii.detach().to(torch.int32).contiguous()
    for name, t in (("accum", accum), ("denom", denom), ("max_radii", max_radii)):
        _flat(what, name, t, N)
    with torch.cuda.device(dev):
        _lib.call("dm4d_dc_accumulate_stats", B, N, grad2d.data_ptr(), radii.data_ptr(), accum.data_ptr(), denom.data_ptr(),
                  max_radii.data_ptr(), _lib.stream(dev))


def classify_densify(accum, denom, scaling, grad_threshold, split_thresh, sphere=False):
    """kind [N] uint8: CLONE where ``accum / denom`` (0 where ``denom == 0``) ``>= grad_threshold`` and the norm of the scales
    ``exp(scaling)`` is ``<= split_thresh``, SPLIT where it is larger, otherwise KEEP.  scaling [N,3]: the log-scales; with
    ``sphere`` the exp of their mean is used on all three axes.  ``grad_threshold`` must be > 0."""
    what = "classify_densify"
    dev = _device_of(what, accum, denom, scaling)
    N = int(scaling.shape[0])
    if scaling.ndim != 2 or scaling.shape[1] != 3:
        raise ValueError(f"{what}: scaling must be [N,3] (got {tuple(scaling.shape)})")
    scaling = _flat(what, "scaling", scaling.detach(), 3 * N)
    _flat(what, "accum", accum, N), _flat(what, "denom", denom, N)
    kind = torch.empty(N, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.call("dm4d_dc_classify_densify", N, accum.data_ptr(), denom.data_ptr(), scaling.data_ptr(), float(grad_threshold),
                  float(split_thresh), int(bool(sphere)), kind.data_ptr(), _lib.stream(dev))
    return kind


def classify_prune(opacity, min_opacity, max_radii=None, radius_limit=None):
    """kind [N] uint8: DROP where ``sigmoid(opacity) < min_opacity`` or (with ``radius_limit``, a one-element device tensor)
    ``max_radii > radius_limit``; otherwise KEEP.  opacity [N] or [N,1]: the logits."""
    what = "classify_prune"
    dev = _device_of(what, opacity, max_radii, radius_limit)
    N = int(opacity.shape[0])
    opacity = _flat(what, "opacity", opacity.detach(), N)
    if radius_limit is not None:
        if max_radii is None:
            raise ValueError(f"{what}: radius_limit needs max_radii")
        _flat(what, "max_radii", max_radii, N), _flat(what, "radius_limit", radius_limit, 1)
    kind = torch.empty(N, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.call("dm4d_dc_classify_prune", N, opacity.data_ptr(), float(min_opacity), _lib.ptr(max_radii if radius_limit is not None else None),
                  _lib.ptr(radius_limit), kind.data_ptr(), _lib.stream(dev))
    return kind


def plan(kind, S=2):
    """(src [M] int32, role [M] uint8, counts) of ``kind`` [N] (uint8 or bool): output row j is a copy of input row ``src[j]`` as
    the kept original (role 0), its clone (1) or its child k (2 + k).  counts: dict(keep, drop, clone, split, M) with keep the
    number of KEEP rows.  One host read (the four counts)."""
    what = "density_control.plan"
    dev = _device_of(what, kind)
    if kind.ndim != 1 or kind.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"{what}: kind must be a [N] uint8 or bool tensor (got {kind.dtype} {tuple(kind.shape)})")
    kind = kind.contiguous()
    N, S = int(kind.shape[0]), int(S)
    with torch.cuda.device(dev):
        st = _lib.stream(dev)
        nbytes = _lib.call("dm4d_dc_plan_scratch_bytes", N)
        scratch = torch.empty(nbytes // 16, 2, dtype=torch.int64, device=dev)
        totals = torch.empty(4, dtype=torch.int64, device=dev)
        _lib.call("dm4d_dc_plan_count", N, _lib.ptr(kind) if N else None, scratch.data_ptr(), nbytes, totals.data_ptr(), st)
        keep, drop, clone, split = (int(v) for v in totals.cpu())
        M = keep + 2 * clone + S * split
        src = torch.empty(M, dtype=torch.int32, device=dev)
        role = torch.empty(M, dtype=torch.uint8, device=dev)
        if M:
            _lib.call("dm4d_dc_plan_rows", N, kind.data_ptr(), S, scratch.data_ptr(), nbytes, totals.data_ptr(), M, src.data_ptr(),
                      role.data_ptr(), st)
    return src, role, {"keep": keep, "drop": drop, "clone": clone, "split": split, "M": M}


def move_rows(src, role, N, entries):
    """``out = in[src]`` for every ``(in, flags)`` of `entries` in ONE launch per ``MAX_ARRAYS`` arrays; returns the outputs (an
    array without columns is returned empty without a launch).  Rows the flags leave out (SKIP_CHILDREN) are uninitialised."""
    M = int(src.shape[0])
    dev = src.device
    outs, table = [], []
    for t, flags in entries:
        if t.dtype != torch.float32 or t.shape[0] != N or not t.is_contiguous():
            raise ValueError(f"density_control.apply: every array must be a contiguous float32 [{N}, ...] tensor (got {t.dtype} {tuple(t.shape)})")
        out = torch.empty((M,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev)
        outs.append(out)
        width = t.numel() // N if N else 0
        if width and M:
            table.append((t, out, width, flags))
    with torch.cuda.device(dev):
        for first in range(0, len(table), MAX_ARRAYS):
            part = table[first:first + MAX_ARRAYS]
            A = _lib.DcArrays()
            A.count = len(part)
            for a, (t, out, width, flags) in enumerate(part):
                getattr(A, "in")[a], A.out[a], A.width[a], A.flags[a] = t.data_ptr(), out.data_ptr(), width, flags
            _lib.call("dm4d_dc_move", N, M, src.data_ptr(), role.data_ptr(), ctypes.byref(A), _lib.stream(dev))
    return outs


def apply(kind, arrays, moments, noise=None, S=2, sphere=False):
    """Apply ``kind`` [N] to every array and moment -> (new arrays, new moments, counts).

    arrays:  dict name -> float32 [N, ...] on the device.  With SPLIT rows it must hold ``xyz`` [N,3], ``scaling`` [N,3] (the
             log-scales) and ``rotation`` [N,4] (w, x, y, z; raw), and ``noise`` [S,N,3] (standard normal, indexed by copy and SOURCE
             row) must be given: child k of row i gets ``xyz_i + R(q_i / |q_i|) (noise[k,i] * s_i / S)`` and
             ``log(s_i / (0.8 S))``, every other array a copy of its source.
    moments: dict name -> (exp_avg, exp_avg_sq) or None, names from ``arrays``: kept rows are copied, every new row is zero.
    counts:  dict(keep, drop, clone, split, M);  M = keep + 2 * clone + S * split rows come out.
    Copied rows are bit copies.  Inputs are not modified."""
    what = "density_control.apply"
    moments = moments or {}
    pairs = [m for m in moments.values() if m is not None]
    dev = _device_of(what, kind, noise, *arrays.values(), *[t for m in pairs for t in m])
    unknown = [k for k in moments if k not in arrays]
    if unknown:
        raise ValueError(f"{what}: moments of unknown arrays {unknown}")
    N = int(kind.shape[0])
    src, role, counts = plan(kind, S)
    children = counts["split"] > 0
    if children:
        missing = [k for k in ("xyz", "scaling", "rotation") if k not in arrays]
        if missing or noise is None:
            raise ValueError(f"{what}: SPLIT rows need arrays xyz, scaling, rotation and noise (missing: {missing + ([] if noise is not None else ['noise'])})")
        if tuple(noise.shape) != (int(S), N, 3) or noise.dtype != torch.float32:
            raise ValueError(f"{what}: noise must be float32 [{int(S)},{N},3] (got {noise.dtype} {tuple(noise.shape)})")
        for k, w in (("xyz", 3), ("scaling", 3), ("rotation", 4)):
            if tuple(arrays[k].shape) != (N, w):
                raise ValueError(f"{what}: {k} must be [{N},{w}] (got {tuple(arrays[k].shape)})")
    ins = {k: v.detach().contiguous() for k, v in arrays.items()}
    entries, slots = [], []
    for k, t in ins.items():
        entries.append((t, _lib.DM4D_DC_SKIP_CHILDREN if children and k in ("xyz", "scaling") else 0))
        slots.append((k, None))
        if moments.get(k) is not None:
            for q, m in enumerate(moments[k]):
                if m.shape != t.shape:
                    raise ValueError(f"{what}: moment {q} of {k} has shape {tuple(m.shape)}, the array {tuple(t.shape)}")
                entries.append((m.detach().contiguous(), _lib.DM4D_DC_ZERO_NEW))
                slots.append((k, q))
    outs = move_rows(src, role, N, entries)
    new_arrays, new_moments = {}, {k: None for k in moments}
    for (k, q), out in zip(slots, outs):
        if q is None:
            new_arrays[k] = out
        else:
            new_moments[k] = (out,) if q == 0 else new_moments[k] + (out,)
    if children:
        M = counts["M"]
        with torch.cuda.device(dev):
            _lib.call("dm4d_dc_split_children", N, M, counts["keep"] + 2 * counts["clone"], int(S), int(bool(sphere)), src.data_ptr(),
                      role.data_ptr(), ins["xyz"].data_ptr(), ins["scaling"].data_ptr(), ins["rotation"].data_ptr(),
                      noise.detach().contiguous().data_ptr(), new_arrays["xyz"].data_ptr(), new_arrays["scaling"].data_ptr(), _lib.stream(dev))
    return new_arrays, new_moments, counts


def reset_opacity(opacity, exp_avg=None, exp_avg_sq=None):
    """In place: ``opacity = logit(sigmoid(opacity) * 0.9)``, both moments (when given) zero."""
    what = "reset_opacity"
    dev = _device_of(what, opacity, exp_avg, exp_avg_sq)
    N = opacity.numel()
    for name, t in (("opacity", opacity), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        if t is not None:
            _flat(what, name, t, N)
    with torch.cuda.device(dev):
        _lib.call("dm4d_dc_reset_opacity", N, opacity.data_ptr(), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq), _lib.stream(dev))
