"""``gaussian-splatting``: free 3D Gaussians with adaptive density control -- the geometry that produces the ``.ply``
``python -m dreammesh4d_amd.isosurface`` consumes.

Mirrors ``GaussianBaseModel`` (custom/threestudio-dreammesh4d/geometry/gaussian_base.py:187-872) and its ``GaussianIO`` mixin's
``save_ply`` / ``load_ply`` (geometry/gaussian_io.py:50-172): the same attributes, properties, Adam groups and schedule.  The
density control itself -- the statistics, clone / split / prune, the opacity reset and the surgery on the Adam moments -- runs on
the kernels of ``density_control`` (one plan and one row move per call) where the reference indexes every tensor with boolean
masks.  Importing this module registers the class with ``threestudio_host``.

Where this differs from the reference, on purpose:

* a Gaussian counts as visible in a view when ``radii > 0`` (what the renderers' ``visibility_filter`` is); ``update_states`` takes
  the filter for the signature's sake and does not read it;
* ``densify_grad_threshold`` must be > 0 (with 0 the reference would select its own fresh clones for splitting);
* the ``normal`` group takes part in the surgery under ``pred_normal`` (the reference's ``optimize_params`` leaves it out and then
  fails with a ``KeyError`` at the first prune);
* the random cap's permutation and the split noise come from generators the caller supplies, so a run can be repeated;
* ``init_num_pts = 0`` leaves the model empty (for ``create_from_pcd`` / ``load_ply``); the shap-e / LRM initialisations are
  not restated.
"""
import os
from dataclasses import dataclass
from typing import Any, NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from . import density_control as dc
from . import threestudio_host as host
from . import wire_formats as wf
from .schedule import C

C0 = 0.28209479177387814


def RGB2SH(rgb):
    return (rgb - 0.5) / C0


def SH2RGB(sh):
    return sh * C0 + 0.5


def inverse_sigmoid(x):
    return torch.log(x / (1 - x))


class BasicPointCloud(NamedTuple):
    points: np.ndarray
    colors: np.ndarray
    normals: np.ndarray


@host.register("gaussian-splatting")
class GaussianModel(host.BaseModule):
    @dataclass
    class Config(host.BaseModule.Config):
        max_num: int = 500000
        sh_degree: int = 0
        position_lr: Any = 0.001
        feature_lr: Any = 0.01
        opacity_lr: Any = 0.05
        scaling_lr: Any = 0.005
        rotation_lr: Any = 0.005
        pred_normal: bool = False
        normal_lr: Any = 0.001

        densification_interval: int = 50
        prune_interval: int = 50
        opacity_reset_interval: int = 100000
        densify_from_iter: int = 100
        prune_from_iter: int = 100
        densify_until_iter: int = 2000
        prune_until_iter: int = 2000
        densify_grad_threshold: Any = 0.01
        min_opac_prune: Any = 0.005
        split_thresh: Any = 0.02
        radii2d_thresh: Any = 1000

        sphere: bool = False
        prune_big_points: bool = False
        color_clip: Any = 2.0

        geometry_convert_from: str = ""
        init_num_pts: int = 100
        pc_init_radius: float = 0.8
        opacity_init: float = 0.1

        sugar_prune_at: Any = None
        sugar_prune_threshold: float = 0.5

    cfg: Config
    SPLIT_CHILDREN = 2                                   # densify_and_split's N

    def configure(self):
        self.device = host.get_device()
        self.pruned_or_densified = False
        self.active_sh_degree = 0
        self.max_sh_degree = self.cfg.sh_degree
        self.sh_levels = self.cfg.sh_degree + 1
        self.color_clip = C(self.cfg.color_clip, 0, 0)
        self._xyz = torch.empty(0)
        self._features_dc = torch.empty(0)
        self._features_rest = torch.empty(0)
        self._scaling = torch.empty(0)
        self._rotation = torch.empty(0)
        self._opacity = torch.empty(0)
        self.max_radii2D = torch.empty(0)
        self.xyz_gradient_accum = torch.empty(0)
        self.denom = torch.empty(0)
        if self.cfg.pred_normal:
            self._normal = torch.empty(0)
        self.optimizer = None
        src = self.cfg.geometry_convert_from
        if src.endswith(".ply") and os.path.exists(src):
            self.load_ply(src)
            self.training_setup()
        elif src:
            raise ValueError(f"gaussian-splatting: geometry_convert_from = {src!r} is not an existing .ply file")
        elif self.cfg.init_num_pts > 0:                  # random points in a ball (gaussian_base.py:350-370)
            n = self.cfg.init_num_pts
            phis = np.random.random((n,)) * 2 * np.pi
            thetas = np.arccos(np.random.random((n,)) * 2 - 1)
            radius = self.cfg.pc_init_radius * np.cbrt(np.random.random((n,)))
            xyz = np.stack((radius * np.sin(thetas) * np.cos(phis), radius * np.sin(thetas) * np.sin(phis), radius * np.cos(thetas)), axis=1)
            color = np.random.random((n, 3)) / 255.0 * C0 + 0.5
            self.create_from_pcd(BasicPointCloud(points=xyz, colors=color, normals=np.zeros((n, 3))), 10)
            self.training_setup()

    # ---------------------------------------------------------------------------------------------- the get_* surface
    @property
    def get_scaling(self):
        if self.cfg.sphere:
            return torch.exp(torch.mean(self._scaling, dim=-1).unsqueeze(-1).repeat(1, 3))
        return torch.exp(self._scaling)

    @property
    def get_rotation(self):
        return torch.nn.functional.normalize(self._rotation, dim=-1)

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):
        return torch.cat((self._features_dc.clip(-self.color_clip, self.color_clip), self._features_rest), dim=1)

    @property
    def get_opacity(self):
        return torch.sigmoid(self._opacity)

    @property
    def get_normal(self):
        if self.cfg.pred_normal:
            return self._normal
        raise ValueError("Normal is not predicted")

    def get_points_rgb(self):
        """The degree-0 colour ``SH2RGB(f_dc)`` [N,3] (what ``isosurface.extract_mesh`` colours the mesh with)."""
        return SH2RGB(self._features_dc[:, 0, :])

    # ---------------------------------------------------------------------------------------------- set-up
    def create_from_pcd(self, pcd, spatial_lr_scale):
        from .simple_knn._C import distCUDA2

        dev = self.device
        self.spatial_lr_scale = spatial_lr_scale
        points = torch.tensor(np.asarray(pcd.points)).float().to(dev)
        fused_color = RGB2SH(torch.tensor(np.asarray(pcd.colors)).float().to(dev))
        n = points.shape[0]
        features = torch.zeros((n, 3, (self.max_sh_degree + 1) ** 2), device=dev)
        features[:, :3, 0] = fused_color
        dist2 = torch.clamp_min(distCUDA2(points), 0.0000001)
        scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
        rots = torch.zeros((n, 4), device=dev)
        rots[:, 0] = 1
        opacities = inverse_sigmoid(self.cfg.opacity_init * torch.ones((n, 1), dtype=torch.float, device=dev))
        self._xyz = nn.Parameter(points.requires_grad_(True))
        self._features_dc = nn.Parameter(features[:, :, 0:1].transpose(1, 2).contiguous().requires_grad_(True))
        self._features_rest = nn.Parameter(features[:, :, 1:].transpose(1, 2).contiguous().requires_grad_(True))
        self._scaling = nn.Parameter(scales.requires_grad_(True))
        self._rotation = nn.Parameter(rots.requires_grad_(True))
        self._opacity = nn.Parameter(opacities.requires_grad_(True))
        if self.cfg.pred_normal:
            self._normal = nn.Parameter(torch.zeros((n, 3), device=dev).requires_grad_(True))
        self.max_radii2D = torch.zeros((n,), device=dev)

    # name of the Adam group -> attribute
    _GROUPS = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
               "rotation": "_rotation", "normal": "_normal"}

    def training_setup(self):
        c = self.cfg
        n, dev = self._xyz.shape[0], self._xyz.device
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        groups = [
            {"params": [self._xyz], "lr": C(c.position_lr, 0, 0), "name": "xyz"},
            {"params": [self._features_dc], "lr": C(c.feature_lr, 0, 0), "name": "f_dc"},
            {"params": [self._features_rest], "lr": C(c.feature_lr, 0, 0) / 20.0, "name": "f_rest"},
            {"params": [self._opacity], "lr": C(c.opacity_lr, 0, 0), "name": "opacity"},
            {"params": [self._scaling], "lr": C(c.scaling_lr, 0, 0), "name": "scaling"},
            {"params": [self._rotation], "lr": C(c.rotation_lr, 0, 0), "name": "rotation"},
        ]
        self.optimize_params = ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
        if c.pred_normal:
            groups.append({"params": [self._normal], "lr": C(c.normal_lr, 0, 0), "name": "normal"})
            self.optimize_params.append("normal")
        self.optimize_list = groups
        self.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)

    def update_learning_rate(self, iteration):
        c = self.cfg
        lr = {"xyz": c.position_lr, "scaling": c.scaling_lr, "f_dc": c.feature_lr, "f_rest": c.feature_lr, "opacity": c.opacity_lr,
              "rotation": c.rotation_lr, "normal": c.normal_lr}
        for group in self.optimizer.param_groups:
            name = group.get("name")
            if name in lr:
                group["lr"] = C(lr[name], 0, iteration, interpolation="exp") / (20.0 if name == "f_rest" else 1.0)
        self.color_clip = C(c.color_clip, 0, iteration)

    def update_step(self, epoch, global_step, on_load_weights=False):
        if self.optimizer is not None:
            self.update_learning_rate(global_step)

    # ---------------------------------------------------------------------------------------------- density control
    def _named_groups(self):
        return [g for g in self.optimizer.param_groups if g.get("name") in self.optimize_params]

    def _apply_kind(self, kind, noise=None, with_stats=False):
        """(Not ``_apply``: that is ``nn.Module``'s hook behind ``.to()`` / ``.float()``.)  One plan and one row move for every parameter, its moments and (``with_stats``) the three statistics; the optimiser's
        groups get new Parameters, their state entries move to the new keys with the moved moments (``step`` as it was)."""
        arrays, moments = {}, {}
        for g in self._named_groups():
            p = g["params"][0]
            arrays[g["name"]] = p.data
            st = self.optimizer.state.get(p, None)
            moments[g["name"]] = None if st is None else (st["exp_avg"], st["exp_avg_sq"])
        if with_stats:
            arrays.update({"#accum": self.xyz_gradient_accum, "#denom": self.denom, "#max_radii": self.max_radii2D})
        new, new_m, counts = dc.apply(kind, arrays, moments, noise=noise, S=self.SPLIT_CHILDREN, sphere=self.cfg.sphere)
        for g in self._named_groups():
            name, old = g["name"], g["params"][0]
            p = nn.Parameter(new[name].requires_grad_(True))
            st = self.optimizer.state.get(old, None)
            if st is not None:
                st["exp_avg"], st["exp_avg_sq"] = new_m[name]
                del self.optimizer.state[old]
                self.optimizer.state[p] = st
            g["params"][0] = p
            setattr(self, self._GROUPS[name], p)
        if with_stats:
            self.xyz_gradient_accum, self.denom, self.max_radii2D = new["#accum"], new["#denom"], new["#max_radii"]
        return counts

    def prune_points(self, mask):
        """Remove the rows where the boolean ``mask`` is true (a mask is a valid ``kind``: true = DROP)."""
        return self._apply_kind(mask.to(torch.bool).reshape(-1), with_stats=True)

    def densify(self, max_grad, noise=None, generator=None):
        """Clone the small and split the large Gaussians whose mean screen-space gradient reaches ``max_grad``; the statistics
        restart as zeros of the new length.  ``noise`` [2,N,3]: the standard normals of the children, by copy and source row
        (drawn from ``generator`` on the device when not given)."""
        n, dev = self._xyz.shape[0], self._xyz.device
        kind = dc.classify_densify(self.xyz_gradient_accum, self.denom, self._scaling.data, max_grad, self.cfg.split_thresh, self.cfg.sphere)
        if noise is None:
            noise = torch.randn(self.SPLIT_CHILDREN, n, 3, device=dev, generator=generator)
        counts = self._apply_kind(kind, noise=noise)
        m = counts["M"]
        self.xyz_gradient_accum = torch.zeros((m, 1), device=dev)
        self.denom = torch.zeros((m, 1), device=dev)
        self.max_radii2D = torch.zeros((m,), device=dev)
        return counts

    def prune(self, min_opacity, max_screen_size=None):
        limit = (torch.mean(self.max_radii2D) * 3).reshape(1) if self.cfg.prune_big_points else None
        return self.prune_points(dc.classify_prune(self._opacity.data, min_opacity, self.max_radii2D, limit))

    def reset_opacity(self):
        g = next(g for g in self.optimizer.param_groups if g.get("name") == "opacity")
        old = g["params"][0]
        st = self.optimizer.state.get(old, None)
        dc.reset_opacity(old.data, *((None, None) if st is None else (st["exp_avg"], st["exp_avg_sq"])))
        p = nn.Parameter(old.data.requires_grad_(True))
        if st is not None:
            del self.optimizer.state[old]
            self.optimizer.state[p] = st
        g["params"][0] = p
        self._opacity = p

    def add_densification_stats(self, viewspace_grad, radii):
        """viewspace_grad [B,N,3] (or [N,3]): the ``.grad`` of the viewspace points; radii [B,N] (or [N]) int."""
        if viewspace_grad.ndim == 2:
            viewspace_grad, radii = viewspace_grad[None], radii[None]
        dc.accumulate_stats(viewspace_grad, radii, self.xyz_gradient_accum, self.denom, self.max_radii2D)

    @torch.no_grad()
    def update_states(self, iteration, visibility_filter, radii, viewspace_point_tensor, generator=None, noise=None):
        """The reference's schedule (gaussian_base.py:822-870).  radii: [B,N] or a list of [N]; viewspace_point_tensor: a list of
        tensors whose ``.grad`` is [N,3] (or one [B,N,3] tensor with a ``.grad``).  ``generator``: a CPU ``torch.Generator`` for the
        random cap's permutation; ``noise``: see ``densify``."""
        c = self.cfg
        self.pruned_or_densified = False
        if c.sugar_prune_at is not None and iteration == c.sugar_prune_at:
            self.pruned_or_densified = True
            self.prune_points(dc.classify_prune(self._opacity.data, c.sugar_prune_threshold))
            return
        n = self._xyz.shape[0]
        if n >= c.max_num + 100:
            self.pruned_or_densified = True
            perm = torch.randperm(n, generator=generator).to(self._xyz.device)
            self.prune_points(perm > c.max_num)
            return
        if torch.is_tensor(viewspace_point_tensor):
            grads = viewspace_point_tensor.grad
        else:
            grads = torch.stack([v.grad for v in viewspace_point_tensor])
        radii = radii if torch.is_tensor(radii) else torch.stack(list(radii))
        self.add_densification_stats(grads, radii)
        if iteration > c.prune_from_iter and iteration < c.prune_until_iter and iteration % c.prune_interval == 0:
            self.pruned_or_densified = True
            self.prune(c.min_opac_prune, c.radii2d_thresh)
            if iteration % c.opacity_reset_interval == 0:
                self.reset_opacity()
        if iteration > c.densify_from_iter and iteration < c.densify_until_iter and iteration % c.densification_interval == 0:
            self.pruned_or_densified = True
            self.densify(c.densify_grad_threshold, noise=noise)

    # ---------------------------------------------------------------------------------------------- the 3DGS .ply
    def save_ply(self, path):
        t = lambda x: x.detach().cpu().numpy()
        wf.write_gaussian_ply(path, t(self._xyz), t(self._features_dc.transpose(1, 2).flatten(start_dim=1)),
                              t(self._features_rest.transpose(1, 2).flatten(start_dim=1)), t(self._opacity), t(self._scaling), t(self._rotation))

    def load_ply(self, path):
        g = wf.read_gaussian_ply(path)
        n, k = len(g["xyz"]), (self.max_sh_degree + 1) ** 2 - 1
        if g["f_rest"].shape[1] != 3 * k:
            raise ValueError(f"{path}: {g['f_rest'].shape[1]} f_rest columns, sh_degree {self.max_sh_degree} needs {3 * k}")
        dev = self.device
        P = lambda a: nn.Parameter(torch.tensor(np.ascontiguousarray(a), dtype=torch.float, device=dev).contiguous().requires_grad_(True))
        self._xyz = P(g["xyz"])
        self._features_dc = P(g["f_dc"].reshape(n, 3, 1).transpose(0, 2, 1))
        self._features_rest = P(g["f_rest"].reshape(n, 3, k).transpose(0, 2, 1))
        self._opacity = P(g["opacity_raw"].reshape(n, 1))
        self._scaling = P(g["scale_raw"])
        self._rotation = P(g["rotation"])
        if self.cfg.pred_normal:
            self._normal = P(np.zeros((n, 3), np.float32))
        self.max_radii2D = torch.zeros((n,), device=dev)
        self.active_sh_degree = self.max_sh_degree
