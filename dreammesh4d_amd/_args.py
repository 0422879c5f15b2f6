"""Argument checks that the mesh and point-cloud front ends share (mesh_simplify, mesh_clean, isosurface, density_control,
sugar_reg).  Each raises what its callers document; the texts are pinned by the tests of those modules."""
import torch

FACE_INDICES = "face indices span [{lo}, {hi}], the mesh has {n} vertices"


def no_cpu_path(what):
    """The Dm4dError (returned, not raised) for tensors that are not on one HIP device."""
    from . import _lib

    return _lib.Dm4dError(f"{what}: tensors must live on one HIP device; there is no CPU path")


def check_face_tensor(what, faces):
    """Raises ValueError unless the tensor `faces` is int32 / int64 [F,3]."""
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: faces must be int32 / int64 [F,3] (got {faces.dtype} {tuple(faces.shape)})")


def check_span(what, name_or_template, lo, hi, n):
    """Raises ValueError unless [lo, hi] lies in [0, n).  `name_or_template` is the name of the tensor, or a sentence of its own
    with the fields {lo}, {hi}, {n} such as FACE_INDICES."""
    if lo < 0 or hi >= n:
        template = name_or_template if "{" in name_or_template else name_or_template + " has values in [{lo}, {hi}], outside [0, {n})"
        raise ValueError(f"{what}: " + template.format(lo=lo, hi=hi, n=n))


def check_index_range(what, name_or_template, t, n):
    """Values of the non-empty device tensor `t` lie in [0, n): one host read, then check_span."""
    lo, hi = (int(v) for v in torch.stack((t.min(), t.max())).cpu())
    check_span(what, name_or_template, lo, hi, n)
