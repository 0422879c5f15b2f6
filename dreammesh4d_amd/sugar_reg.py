"""SuGaR density and normal regularisation of free Gaussians on the HIP device.

Replaces ``SuGaRRegularizer.coarse_density_regulation`` (custom/threestudio-dreammesh4d/utils/sugar_utils.py:79-759, called every
iteration of stage "gaussian" by system/sugar_static.py:98-113, 215-240): per-sample gathers of the 16 tracked neighbours as
``[S,16,3]``, ``[S,16,3,3]`` and ``[S,16]`` tensors, batched products over them and autograd through all of it.  Here the kernels
of ``csrc/sugar_reg.hip`` (C ABI ``include/dm4d_sugar_reg.h``; DESIGN.md, "SuGaR density and normal regularisation") prepare one
18-float record per Gaussian, a sample reads the records of its Gaussian's neighbours, and the backward recomputes the forward.

* ``sugar_density_reg``   the operator on ACTIVATED values (scales after ``exp``, opacities after ``sigmoid``, quaternions as
                          ``get_rotation`` returns them); a ``torch.autograd.Function``, so gradients continue into the model
* ``SuGaRRegularizer``    the reference's class: neighbours, the sampler with its quirk, normals, ``coarse_density_regulation``

The CONTENTS of ``knn_idx`` and ``sample_idx`` (values in ``[0, N)``) are the caller's contract with the library; this layer
checks them on the device (``min`` / ``max``) before a call.  There is no CPU path.
"""
from collections import namedtuple

import torch

from . import _lib, knn as _knn
from ._args import check_index_range as _check_range

K_MAX = _lib.DM4D_SR_MAX_K
CHUNK = _lib.DM4D_SR_CHUNK

SugarReg = namedtuple("SugarReg", ["density_regulation", "normal_regulation", "density", "beta", "density_term", "normal_term"])


def reverse_table(knn_idx):
    """(rev_ptr [N+1], rev_pos [N*K]) int32 of ``knn_idx`` [N,K]: ``rev_pos[rev_ptr[j]:rev_ptr[j+1]]`` are the flat positions
    ``g * K + k`` with ``knn_idx[g,k] == j``, ascending (a stable device sort of the flat table)."""
    n = int(knn_idx.shape[0])
    flat = knn_idx.reshape(-1).to(torch.int64)
    rev_pos = torch.sort(flat, stable=True)[1].to(torch.int32)
    rev_ptr = torch.zeros(n + 1, dtype=torch.int32, device=knn_idx.device)
    rev_ptr[1:] = torch.cumsum(torch.bincount(flat, minlength=n), 0)
    return rev_ptr, rev_pos


def _segments(sample_idx, n):
    """(order [S], seg_ptr [N+1], chunk_ptr [N+1]) int32: the stable sort of the samples by Gaussian, the segment of every
    Gaussian in it, and the exclusive scan of its number of chunks of ``CHUNK`` samples."""
    order = torch.sort(sample_idx.to(torch.int64), stable=True)[1].to(torch.int32)
    count = torch.bincount(sample_idx.to(torch.int64), minlength=n)
    seg_ptr = torch.zeros(n + 1, dtype=torch.int32, device=sample_idx.device)
    seg_ptr[1:] = torch.cumsum(count, 0)
    chunk_ptr = torch.zeros(n + 1, dtype=torch.int32, device=sample_idx.device)
    chunk_ptr[1:] = torch.cumsum((count + (CHUNK - 1)) // CHUNK, 0)
    return order, seg_ptr, chunk_ptr


def _scratch(n, k, s, dev):
    nbytes = _lib.call("dm4d_sr_scratch_bytes", n, k, s)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


class _SugarDensityReg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, scales, quats, opac, knn_idx, sample_idx, eps, sampling_scale, density_factor, with_normal, reverse):
        dev = xyz.device
        n, k, s = int(xyz.shape[0]), int(knn_idx.shape[1]), int(sample_idx.shape[0])
        order, seg_ptr, chunk_ptr = _segments(sample_idx, n)
        density, beta, dterm = (torch.empty(s, dtype=torch.float32, device=dev) for _ in range(3))
        nterm = torch.empty(s, dtype=torch.float32, device=dev) if with_normal else None
        losses = torch.empty(2, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            scratch, nbytes = _scratch(n, k, s, dev)
            _lib.call("dm4d_sr_forward", n, k, s, xyz.data_ptr(), scales.data_ptr(), quats.data_ptr(), opac.data_ptr(), knn_idx.data_ptr(),
                      sample_idx.data_ptr(), order.data_ptr(), eps.data_ptr(), float(sampling_scale), float(density_factor),
                      int(with_normal), scratch.data_ptr(), nbytes, density.data_ptr(), beta.data_ptr(), dterm.data_ptr(),
                      _lib.ptr(nterm), losses.data_ptr(), _lib.stream(dev))
        ctx.save_for_backward(xyz, scales, quats, opac, knn_idx, sample_idx, eps, order, seg_ptr, chunk_ptr)
        ctx.args = (float(sampling_scale), float(density_factor), bool(with_normal))
        ctx.reverse = reverse
        outs = (density, beta, dterm) + ((nterm,) if with_normal else ())
        ctx.mark_non_differentiable(*outs)
        return (losses[0].clone(), losses[1].clone()) + outs

    @staticmethod
    def backward(ctx, g_density, g_normal, *_):
        xyz, scales, quats, opac, knn_idx, sample_idx, eps, order, seg_ptr, chunk_ptr = ctx.saved_tensors
        ss, df, with_normal = ctx.args
        dev = xyz.device
        n, k, s = int(xyz.shape[0]), int(knn_idx.shape[1]), int(sample_idx.shape[0])
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        upstream = torch.stack([zero if g is None else g.to(torch.float32).reshape(()) for g in (g_density, g_normal)])
        rev_ptr, rev_pos = ctx.reverse if ctx.reverse is not None else reverse_table(knn_idx)
        grads = [torch.empty_like(t) if need else None for t, need in zip((xyz, scales, quats, opac), ctx.needs_input_grad[:4])]
        with torch.cuda.device(dev):
            scratch, nbytes = _scratch(n, k, s, dev)
            _lib.call("dm4d_sr_backward", n, k, s, xyz.data_ptr(), scales.data_ptr(), quats.data_ptr(), opac.data_ptr(), knn_idx.data_ptr(),
                      sample_idx.data_ptr(), order.data_ptr(), eps.data_ptr(), ss, df, int(with_normal), upstream.data_ptr(),
                      seg_ptr.data_ptr(), chunk_ptr.data_ptr(), rev_ptr.data_ptr(), rev_pos.data_ptr(), scratch.data_ptr(), nbytes,
                      *[_lib.ptr(g) for g in grads], _lib.stream(dev))
        return tuple(grads) + (None,) * 7


def _prepare(what, xyz, scales, quats, opac, knn_idx, sample_idx, eps):
    """Shapes and dtypes, then devices checked (a call on CPU tensors alone is refused last, by name); -> the tensors as the library reads them (opac [N], indices int32, all contiguous)."""
    named = (("xyz", xyz), ("scales", scales), ("quats", quats), ("opac", opac), ("knn_idx", knn_idx), ("sample_idx", sample_idx), ("eps", eps))
    for name, t in named:
        if not torch.is_tensor(t):
            raise ValueError(f"{what}: {name} must be a tensor (got {type(t).__name__})")
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{what}: xyz must be [N,3] (got {tuple(xyz.shape)})")
    n = int(xyz.shape[0])
    if tuple(scales.shape) != (n, 3) or tuple(quats.shape) != (n, 4):
        raise ValueError(f"{what}: scales must be [{n},3] and quats [{n},4] (got {tuple(scales.shape)}, {tuple(quats.shape)})")
    if tuple(opac.shape) not in ((n,), (n, 1)):
        raise ValueError(f"{what}: opac must be [{n}] or [{n},1] (got {tuple(opac.shape)})")
    if knn_idx.ndim != 2 or knn_idx.shape[0] != n or not 1 <= knn_idx.shape[1] <= K_MAX:
        raise ValueError(f"{what}: knn_idx must be [{n},K] with 1 <= K <= {K_MAX} (got {tuple(knn_idx.shape)})")
    if sample_idx.ndim != 1:
        raise ValueError(f"{what}: sample_idx must be [S] (got {tuple(sample_idx.shape)})")
    s = int(sample_idx.shape[0])
    if tuple(eps.shape) != (s, 3):
        raise ValueError(f"{what}: eps must be [{s},3] (got {tuple(eps.shape)})")
    if n == 0 or s == 0:
        raise ValueError(f"{what}: needs at least one Gaussian and one sample (N = {n}, S = {s})")
    if n > _lib.DM4D_SR_MAX_POINTS or s > _lib.DM4D_SR_MAX_SAMPLES:
        raise ValueError(f"{what}: N = {n} / S = {s} above {_lib.DM4D_SR_MAX_POINTS} / {_lib.DM4D_SR_MAX_SAMPLES}")
    for name, t in named[:4] + named[6:]:
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: {name} must be float32 (got {t.dtype})")
    for name, t in named[4:6]:
        if t.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{what}: {name} must be int32 or int64 (got {t.dtype})")
    if not any(t.is_cuda for _, t in named):
        raise _lib.Dm4dError(f"{what} runs on the HIP device (no CPU fallback in the product)")
    dev = xyz.device
    for name, t in named:
        if t.device != dev:
            raise ValueError(f"{what}: {name} on {t.device}, xyz on {dev}")
    return (xyz.contiguous(), scales.contiguous(), quats.contiguous(), opac.reshape(n).contiguous(),
            knn_idx.detach().to(torch.int32).contiguous(), sample_idx.detach().to(torch.int32).contiguous(), eps.detach().contiguous())


def sugar_density_reg(xyz, scales, quats, opac, knn_idx, sample_idx, eps, *, sampling_scale=1.5, density_factor=1.0,
                      with_normal_loss=False, reverse=None, validate=True):
    """The two regularisation terms of ``coarse_density_regulation`` for the samples ``(sample_idx, eps)``.

    xyz [N,3], scales [N,3] (positive, after ``exp``), quats [N,4] (real part first, as ``get_rotation`` returns them; they need
    not be unit), opac [N] or [N,1] (after ``sigmoid``): float32 on one HIP device, any of them may require grad.
    knn_idx [N,K] int32/int64, 1 <= K <= 32, values in [0,N): ANY table (a row may repeat a value).  sample_idx [S] in [0,N), any
    order; eps [S,3] float32 standard normals.  Sample i lies at ``xyz_g + quaternion_apply(q_g, sampling_scale * s_g * eps_i)``.

    Returns ``SugarReg``: ``density_regulation`` = mean |density - target| and ``normal_regulation`` (``None`` without
    ``with_normal_loss``), 0-dim and differentiable; ``density``, ``beta``, ``density_term``, ``normal_term`` [S], detached, in the
    caller's sample order.  On exact ties of the two smallest scales the LOWEST axis is the normal's (torch leaves it open).
    Two calls on the same inputs return the same bytes, gradients included.

    ``reverse``: ``reverse_table(knn_idx)`` when the caller keeps it (it is built in the backward otherwise).  ``validate``: check
    the contents of ``knn_idx`` and ``sample_idx`` on the device (one host read); they are the caller's contract otherwise."""
    what = "sugar_density_reg"
    for name, v in (("sampling_scale", sampling_scale), ("density_factor", density_factor)):
        if not float("-inf") < float(v) < float("inf"):
            raise ValueError(f"{what}: {name} = {v} is not finite")
    x, s, q, o, kn, si, e = _prepare(what, xyz, scales, quats, opac, knn_idx, sample_idx, eps)
    n = int(x.shape[0])
    if reverse is not None:
        rp, rpos = reverse
        if rp.dtype != torch.int32 or rpos.dtype != torch.int32 or rp.numel() != n + 1 or rpos.numel() != kn.numel() or rp.device != x.device or rpos.device != x.device:
            raise ValueError(f"{what}: reverse must be reverse_table(knn_idx) on {x.device}")
        reverse = (rp.contiguous(), rpos.contiguous())
    if validate:
        _check_range(what, "knn_idx", kn, n)
        _check_range(what, "sample_idx", si, n)
    out = _SugarDensityReg.apply(x, s, q, o, kn, si, e, float(sampling_scale), float(density_factor), bool(with_normal_loss), reverse)
    return SugarReg(out[0], out[1] if with_normal_loss else None, out[2], out[3], out[4], out[5] if with_normal_loss else None)


# ------------------------------------------------------------------------------------------------ pytorch3d's two functions
def quaternion_to_matrix(q):
    """pytorch3d.transforms.quaternion_to_matrix (real part first, ``two_s = 2 / (q.q)``)."""
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def _raw_multiply(a, b):
    aw, ax, ay, az = torch.unbind(a, -1)
    bw, bx, by, bz = torch.unbind(b, -1)
    return torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)


def quaternion_apply(q, v):
    """pytorch3d.transforms.quaternion_apply: ``q (0,v) conj(q)`` -- the conjugate, not the inverse."""
    conj = q * q.new_tensor([1.0, -1.0, -1.0, -1.0])
    return _raw_multiply(_raw_multiply(q, torch.cat((torch.zeros_like(v[..., :1]), v), -1)), conj)[..., 1:]


class SuGaRRegularizer:
    """The reference's ``SuGaRRegularizer`` (sugar_utils.py:79-759) over a ``GaussianModel``, the coarse regularisation on the HIP
    kernels.  ``beta_mode`` 'learnable' and 'weighted_average', ``estimate_from_points=True`` and a bound surface mesh are not
    offered (the system never constructs them)."""

    def __init__(self, gaussians, initialize=True, keep_track_of_knn=False, knn_to_track=16, surface_mesh_to_bind=None, beta_mode="average"):
        if surface_mesh_to_bind is not None:
            raise NotImplementedError("SuGaRRegularizer: surface_mesh_to_bind is not supported")
        if beta_mode != "average":
            if beta_mode in ("learnable", "weighted_average"):
                raise NotImplementedError(f"SuGaRRegularizer: beta_mode {beta_mode!r} is not supported (only 'average')")
            raise ValueError("Unknown beta_mode.")
        self.gaussians = gaussians
        self.binded_to_surface_mesh = False
        self.keep_track_of_knn = keep_track_of_knn
        self.knn_to_track = knn_to_track
        self.beta_mode = beta_mode
        self.knn_idx = self.knn_dists = None
        self._knn_i32 = self._reverse = None

    points = property(lambda self: self.gaussians.get_xyz)
    scaling = property(lambda self: self.gaussians.get_scaling)
    strengths = property(lambda self: self.gaussians.get_opacity)
    quaternions = property(lambda self: self.gaussians.get_rotation)
    n_points = property(lambda self: len(self.gaussians.get_xyz))
    device = property(lambda self: self.gaussians.get_xyz.device)

    @torch.no_grad()
    def reset_neighbors(self, knn_to_track=None):
        """``knn_idx`` / ``knn_dists`` [N,K] of every Gaussian among all of them (itself included, as in the reference), and the
        reverse table the backward reads.  Not hot: once per ``reset_neighbors_every`` iterations."""
        if knn_to_track is None:
            knn_to_track = self.knn_to_track
        self.knn_to_track = knn_to_track
        x = self.points.detach()
        knns = _knn.knn_points(x, x, knn_to_track)
        self.knn_dists, self.knn_idx = knns.dists, knns.idx
        self._knn_i32 = knns.idx.to(torch.int32).contiguous()
        _check_range("SuGaRRegularizer.reset_neighbors", "knn_idx", self._knn_i32, x.shape[0])
        self._reverse = reverse_table(self._knn_i32)

    def sampling_weights(self, mask=None, probabilities_proportional_to_opacity=False, probabilities_proportional_to_volume=True):
        """The weights the reference hands to ``torch.multinomial`` (:203-214), AS WRITTEN: the CUMULATIVE probabilities
        ``areas.cumsum() / areas.sum()``, not the probabilities -- Gaussian i is drawn with a weight proportional to the total
        area of Gaussians 0 .. i.  A quirk of the reference that is kept."""
        scaling = self.scaling if mask is None else self.scaling[mask]
        areas = scaling[..., 0] * scaling[..., 1] * scaling[..., 2] if probabilities_proportional_to_volume else torch.ones_like(scaling[..., 0])
        if probabilities_proportional_to_opacity:
            areas = areas * (self.strengths.view(-1) if mask is None else self.strengths[mask].view(-1))
        areas = areas.abs()
        return areas.cumsum(dim=-1) / areas.sum(dim=-1, keepdim=True)

    def sample_points_in_gaussians(self, num_samples, sampling_scale_factor=1.0, mask=None, probabilities_proportional_to_opacity=False,
                                   probabilities_proportional_to_volume=True, generator=None):
        """``(points [S,3], idx [S])``: Gaussians drawn by ``torch.multinomial`` over ``sampling_weights`` (the reference's
        cumulative quirk, see there), a point in each at ``xyz + quaternion_apply(q, factor * s * randn)``."""
        with torch.no_grad():
            cum_probs = self.sampling_weights(mask, probabilities_proportional_to_opacity, probabilities_proportional_to_volume)
            idx = torch.multinomial(cum_probs, num_samples=num_samples, replacement=True, generator=generator)
            if mask is not None:
                idx = torch.arange(self.n_points, device=self.device)[mask][idx]
            eps = torch.randn(num_samples, 3, device=self.device, generator=generator)
        points = self.points[idx] + quaternion_apply(self.quaternions[idx], sampling_scale_factor * self.scaling[idx] * eps)
        return points, idx

    def get_smallest_axis(self, return_idx=False):
        """Column of the rotation matrix along the smallest scale [N,3] (the LOWEST axis on exact ties), optionally its index."""
        s = self.scaling
        idx = torch.zeros(s.shape[0], dtype=torch.int64, device=s.device)
        idx = torch.where(s[:, 1] < s[:, 0], torch.ones_like(idx), idx)
        idx = torch.where(s[:, 2] < torch.minimum(s[:, 0], s[:, 1]), torch.full_like(idx, 2), idx)
        axis = quaternion_to_matrix(self.quaternions).gather(2, idx[:, None, None].expand(-1, 3, -1)).squeeze(2)
        return (axis, idx) if return_idx else axis

    def get_normals(self, estimate_from_points=False, neighborhood_size=32):
        if estimate_from_points:
            raise NotImplementedError("SuGaRRegularizer.get_normals: estimate_from_points=True is not supported")
        return self.get_smallest_axis()

    def coarse_density_regulation(self, args, sample_idx=None, eps=None, generator=None):
        """``{"density_regulation", "normal_regulation"}`` of one iteration (sugar_utils.py:682-759): ``sampling_scale`` 1.5,
        ``density_factor`` 1, every Gaussian sampled with the reference's weights for ``probabilities_proportional_to_volume =
        False``.  args: ``n_samples_for_sdf_regularization``, ``use_sdf_better_normal_loss``.  ``sample_idx`` [S] / ``eps`` [S,3]
        replace the draw (from ``generator`` otherwise), as ``noise`` does in density control.  ``normal_regulation`` is 0
        without the normal loss, as in the reference."""
        if self.knn_idx is None or self._knn_i32.shape[0] != self.n_points:
            raise RuntimeError("SuGaRRegularizer.coarse_density_regulation: call reset_neighbors() first (and again after the Gaussians change)")
        num = int(args.n_samples_for_sdf_regularization)
        drawn = sample_idx is None
        if drawn:
            with torch.no_grad():
                weights = self.sampling_weights(probabilities_proportional_to_volume=False)
                sample_idx = torch.multinomial(weights, num_samples=num, replacement=True, generator=generator)
        if eps is None:
            eps = torch.randn(int(sample_idx.shape[0]), 3, device=self.device, generator=generator)
        normal = bool(args.use_sdf_better_normal_loss)
        out = sugar_density_reg(self.points, self.scaling, self.quaternions, self.strengths, self._knn_i32, sample_idx, eps, sampling_scale=1.5,
                                density_factor=1.0, with_normal_loss=normal, reverse=self._reverse, validate=not drawn)
        return {"density_regulation": out.density_regulation, "normal_regulation": out.normal_regulation if normal else 0}
