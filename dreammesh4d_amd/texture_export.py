"""Textured mesh export: the predict path of the sugar / dynamic-sugar systems (``launch.py --export``, reference README.md:91-93).

After training, the reference bakes ONE texture of the canonical surface mesh and writes it with the deformed meshes:

* ``build_atlas``     the square-packed UV atlas and the initial texture from the Gaussians' SH colours
                      (C/system/base.py:72-209; kernel ``dm4d_tex_atlas_init``)
* ``predict_cameras`` the predict dataset: 120 random views at 1024^2 (C/data/temporal_image.py:502-522, C/data/uncond.py:479-600)
* ``TextureBaker``    per view, the canonical Gaussian render averaged into the texels the mesh shows at its pixels
                      (C/system/base.py:253-292; kernels ``dm4d_mesh_raster`` and ``dm4d_tex_accumulate``)
* ``bake_texture``    the two above over all views, rendered in chunks through ``gviews.render_gaussian_views``
* ``export_textured_sequence`` / ``export_textured_mesh``  the OBJ + MTL + PNG files (C/system/sugar_4dgen.py:594-640,
                      C/system/base.py:294-323)

(C/ = custom/threestudio-dreammesh4d/.)  The reference rasterizes the mesh and samples the index texture with pytorch3d, which has no
ROCm build; its conventions are restated in csrc/texbake.hip.  Where they could not be checked against pytorch3d (edge coverage,
the float arithmetic of the nearest sample) the parity is unpinned.  Everything on the device is HIP; there is no CPU path.
"""
import math
import os
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, gviews
from ._lib import ptr as _p, stream as _stream
from .ops import _f32
from .renderer import cam_info_gaussian

SH_C0 = 0.28209479177387814
N_PREDICT_VIEWS = 120
PREDICT_RESOLUTION = 1024


@dataclass
class Atlas:
    """faces_uv [F,3] int64 (= arange(3F)), verts_uv [6 n^2, 2] float32 (every square's six corners, as the reference keeps them),
    texture_size, texture [T,T,3] float32: the SH-initialised texture, after the reference's transpose and flip."""
    faces_uv: torch.Tensor
    verts_uv: torch.Tensor
    texture_size: int
    texture: torch.Tensor


def atlas_size(n_faces, square_size):
    """(texture_size, n_square_per_axis) of C/system/base.py:84-87."""
    n_axis = int(math.sqrt(n_faces // 2 + 1) + 1)
    return square_size * n_axis, n_axis


def atlas_uv(n_faces, square_size, device=None):
    """(faces_uv [F,3] int64, verts_uv [6 n^2, 2] float32) of C/system/base.py:89-131: square k = (a, b) = (k // n, k % n) gets the
    corners, in texels, bottom (a+1, b) S + (-2, 1), (a, b) S + (2, 1), (a+1, b+1) S + (-2, -3) and top (a, b+1) S + (1, -1),
    (a, b) S + (1, 3), (a+1, b+1) S + (-3, -1), divided by texture_size."""
    T, n = atlas_size(n_faces, square_size)
    S = int(square_size)
    k = torch.arange(n * n, device=device)
    a, b = (k // n)[:, None], (k % n)[:, None]
    cu = torch.cat([(a + 1) * S - 2, a * S + 2, (a + 1) * S - 2, a * S + 1, a * S + 1, (a + 1) * S - 3], 1)
    cv = torch.cat([b * S + 1, b * S + 1, (b + 1) * S - 3, (b + 1) * S - 1, b * S + 3, (b + 1) * S - 1], 1)
    verts_uv = torch.stack([cu, cv], -1).reshape(-1, 2).to(torch.float32) / T
    faces_uv = torch.arange(3 * n_faces, device=device).view(n_faces, 3)
    return faces_uv, verts_uv


def atlas_texels(n_faces, square_size, device=None):
    """The texels the atlas gives each face (C/system/base.py:133-181), in the closed form k_tex_atlas_init evaluates per thread:
    (face, row, col [F*K] int64, bary [F*K,3] float32), K = S(S-1)/2 texels per triangle.  Bottom triangle: (ti, tj), tj <= ti < S-1,
    bary (1 - b1 - b2, (S-2-ti) / (S-3), (tj-1) / (S-3)); top: ti < tj < S, bary (1 - b1 - b2, (ti-1) / (S-3), (S-1-tj) / (S-3)).
    The texel sits at row T-1-(b S + tj), column a S + ti of the final image (the reference's transpose, then flip of axis 0)."""
    T, n = atlas_size(n_faces, square_size)
    S = int(square_size)
    bot, top = torch.tril_indices(S - 1, S - 1, device=device), torch.triu_indices(S, S, offset=1, device=device)
    den = float(S - 3)
    bb = torch.stack([(S - 2 - bot[0]).float() / den, (bot[1] - 1).float() / den], -1)
    bt = torch.stack([(top[0] - 1).float() / den, (S - 1 - top[1]).float() / den], -1)
    face = torch.arange(n_faces, device=device)[:, None].expand(-1, bot.shape[1])
    is_top = (face % 2 == 1)
    ti = torch.where(is_top, top[0][None], bot[0][None])
    tj = torch.where(is_top, top[1][None], bot[1][None])
    b12 = torch.where(is_top[..., None], bt[None], bb[None])
    bary = torch.cat([1.0 - (b12[..., :1] + b12[..., 1:]), b12], -1)
    sq = face // 2
    a, b = sq // n, sq % n
    return face.reshape(-1), (T - 1 - (b * S + tj)).reshape(-1), (a * S + ti).reshape(-1), bary.reshape(-1, 3)


def _n_per_face(geometry):
    return int(geometry.cfg_n_gaussians_per_surface_triangle)


def _i32(t):
    return t.to(torch.int32).contiguous()


def build_atlas(geometry, square_size=20) -> Atlas:
    """Atlas and SH-initialised texture of the geometry's canonical surface mesh (``on_predict_start``, C/system/base.py:72-209).
    `geometry`: ``sugar.SuGaR`` or ``sugar.DynamicSuGaR`` on the HIP device."""
    L = _lib.lib()
    dev = geometry.device
    if dev.type != "cuda":
        raise _lib.Dm4dError("build_atlas runs on the HIP device (there is no CPU fallback in the product)")
    verts, faces = _f32(geometry.get_xyz_verts), _i32(geometry.get_faces)
    Fn, G = int(faces.shape[0]), _n_per_face(geometry)
    T = int(L.dm4d_tex_atlas_size(Fn, int(square_size)))
    if T < 0:
        raise ValueError(f"build_atlas: square_size {square_size} must be >= 4 (and the mesh non-empty)")
    if T != atlas_size(Fn, int(square_size))[0]:
        raise RuntimeError("dm4d_tex_atlas_size disagrees with the atlas formula")
    if Fn and (int(faces.min()) < 0 or int(faces.max()) >= int(verts.shape[0])):
        raise ValueError("build_atlas: face indices out of range")
    with torch.no_grad():
        means, rot, scales = _f32(geometry.get_xyz), _f32(geometry.get_rotation), _f32(geometry.get_scaling)
        dc = _f32(geometry._sh_coordinates_dc).reshape(-1, 3)
    if tuple(means.shape) != (Fn * G, 3) or tuple(rot.shape) != (Fn * G, 4) or tuple(dc.shape) != (Fn * G, 3):
        raise ValueError("build_atlas: the geometry's Gaussians are not F x G")
    texture = torch.full((T, T, 3), 0.5, dtype=torch.float32, device=dev)        # SH2RGB of the reference's zero image
    with torch.cuda.device(dev):
        _lib.call("dm4d_tex_atlas_init", Fn, G, int(square_size), _p(verts), _p(faces), _p(means), _p(rot), _p(scales), _p(dc), _p(texture),
                  _stream(dev))
    faces_uv, verts_uv = atlas_uv(Fn, int(square_size), dev)
    return Atlas(faces_uv, verts_uv, T, texture)


def predict_cameras(n=N_PREDICT_VIEWS, height=PREDICT_RESOLUTION, width=PREDICT_RESOLUTION, seed=0, azimuth_range=(-180.0, 180.0),
                    elevation_range=(-10.0, 80.0), camera_distance_range=(3.8, 3.8), fovy_deg=20.0, batch_uniform_azimuth=False):
    """The predict dataset (``RandomCameraArbiraryDataset``, C/data/uncond.py:479-600, with the ranges of
    C/data/temporal_image.py:502-522), drawn once from a seeded ``torch.Generator`` on the host: azimuth uniform in its range (or
    stratified with `batch_uniform_azimuth`); elevation with probability 1/2 uniform in degrees, else uniform on the sphere (one coin
    for the whole set); distance uniform; fovy = eval_fovy_deg (the shipped configurations: ${data.default_fovy_deg} = 20).
    Returns the batch dict: c2w [n,4,4], fovy [n] (radians), elevation_deg, azimuth_deg, camera_distances [n], height, width."""
    g = torch.Generator().manual_seed(int(seed))
    rand = lambda k: torch.rand(k, generator=g)
    a0, a1 = azimuth_range
    if batch_uniform_azimuth:
        azimuth_deg = (rand(n) + torch.arange(n)) / n * (a1 - a0) + a0
    else:
        azimuth_deg = rand(n) * (a1 - a0) + a0
    e0, e1 = elevation_range
    if float(rand(1)) < 0.5:
        elevation_deg = rand(n) * (e1 - e0) + e0
    else:
        s0, s1 = math.sin(e0 / 180.0 * math.pi), math.sin(e1 / 180.0 * math.pi)
        elevation_deg = torch.asin(rand(n) * (s1 - s0) + s0) / math.pi * 180.0
    d0, d1 = camera_distance_range
    dist = rand(n) * (d1 - d0) + d0
    el, az = elevation_deg * math.pi / 180, azimuth_deg * math.pi / 180
    pos = torch.stack([dist * torch.cos(el) * torch.cos(az), dist * torch.cos(el) * torch.sin(az), dist * torch.sin(el)], -1)
    up = torch.tensor([0.0, 0.0, 1.0])[None].repeat(n, 1)
    lookat = F.normalize(-pos, dim=-1)
    right = F.normalize(torch.cross(lookat, up, dim=-1), dim=-1)
    up = F.normalize(torch.cross(right, lookat, dim=-1), dim=-1)
    c2w = torch.zeros(n, 4, 4)
    c2w[:, :3, :3] = torch.stack([right, up, -lookat], -1)
    c2w[:, :3, 3] = pos
    c2w[:, 3, 3] = 1.0
    return {"c2w": c2w, "fovy": torch.full((n,), fovy_deg * math.pi / 180), "elevation_deg": elevation_deg, "azimuth_deg": azimuth_deg,
            "camera_distances": dist, "height": int(height), "width": int(width)}


class TextureBaker:
    """The per-view texel update of ``predict_step`` (C/system/base.py:253-292) on the canonical surface mesh.

    ``add_views(rgb, viewmats, projmats)``: rgb [B,3,H,W] (the rendered ``comp_rgb``, channels first), cameras [B,4,4] in the
    rasterizer's row-vector convention.  For each view, in order: the mesh is rasterized (``dm4d_mesh_raster``), every covered pixel
    finds its texel by the nearest sample of the atlas, and among a view's pixels on one texel the lowest linear pixel index adds its
    colour to the texel's sum and 1 to its count -- the reference's index-put keeps "one of them" (unspecified which); this is a
    fixed instance of it.  ``texture()``: sum / count where visited, the initial texture elsewhere (``on_predict_epoch_end``)."""

    def __init__(self, geometry, atlas: Atlas, resolution=PREDICT_RESOLUTION):
        L = _lib.lib()
        self.device = dev = geometry.device
        if dev.type != "cuda":
            raise _lib.Dm4dError("TextureBaker runs on the HIP device (there is no CPU fallback in the product)")
        self.H = self.W = int(resolution)
        self.verts, self.faces = _f32(geometry.get_xyz_verts), _i32(geometry.get_faces)
        self.F = int(self.faces.shape[0])
        if self.F and (int(self.faces.min()) < 0 or int(self.faces.max()) >= int(self.verts.shape[0])):
            raise ValueError("TextureBaker: face indices out of range")
        self.atlas = atlas
        self.T = int(atlas.texture_size)
        self.verts_uv, self.faces_uv = _f32(atlas.verts_uv).to(dev), _i32(atlas.faces_uv).to(dev)
        if tuple(self.faces_uv.shape) != (self.F, 3) or int(self.faces_uv.min()) < 0 or int(self.faces_uv.max()) >= int(self.verts_uv.shape[0]):
            raise ValueError("TextureBaker: faces_uv must be [F,3] indices into verts_uv")
        n = self.T * self.T
        self.sum = torch.zeros(n, 3, dtype=torch.float32, device=dev)
        self.count = torch.zeros(n, dtype=torch.float32, device=dev)
        self.claim = torch.zeros(int(L.dm4d_tex_claim_bytes(n)) // 8, dtype=torch.int64, device=dev)
        self.epoch = 0
        self._scratch = None

    def rasterize(self, viewmats, projmats, with_faces=False):
        """texel [B,H,W] int32 (-1 = uncovered) of B views; with_faces: also (face [B,H,W] int32, bary [B,H,W,3] float32)."""
        L = _lib.lib()
        dev, H, W = self.device, self.H, self.W
        vm, pm = _f32(viewmats).to(dev).reshape(-1, 16), _f32(projmats).to(dev).reshape(-1, 16)
        B = int(vm.shape[0])
        need = int(L.dm4d_mesh_raster_scratch_bytes(B, H, W, self.F))
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        texel = torch.empty(B, H, W, dtype=torch.int32, device=dev)
        face = torch.empty(B, H, W, dtype=torch.int32, device=dev) if with_faces else None
        bary = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev) if with_faces else None
        with torch.cuda.device(dev):
            _lib.call("dm4d_mesh_raster", B, H, W, self.F, _p(self.verts), _p(self.faces), _p(vm), _p(pm), _p(self.verts_uv), _p(self.faces_uv),
                      self.T, _p(self._scratch), self._scratch.numel(), _p(texel), _p(face), _p(bary), _stream(dev))
        return (texel, face, bary) if with_faces else texel

    def accumulate(self, texel, rgb):
        """One view: texel [H,W] int32, rgb [3,H,W] float32 (both on the device)."""
        texel, rgb = texel.to(torch.int32).contiguous(), _f32(rgb)
        n = int(texel.numel())
        if texel.dim() != 2 or tuple(rgb.shape) != (3, *texel.shape):
            raise ValueError(f"TextureBaker.accumulate: rgb must be [3,H,W] for a texel map {tuple(texel.shape)}, got {tuple(rgb.shape)}")
        self.epoch += 1
        with torch.cuda.device(self.device):
            _lib.call("dm4d_tex_accumulate", n, _p(texel), _p(rgb), n, self.epoch, _p(self.claim), self.claim.numel() * 8, self.T * self.T,
                      _p(self.sum), _p(self.count), _stream(self.device))

    def add_views(self, rgb, viewmats, projmats):
        texel = self.rasterize(viewmats, projmats)
        rgb = _f32(rgb).to(self.device)
        if tuple(rgb.shape) != (texel.shape[0], 3, self.H, self.W):
            raise ValueError(f"TextureBaker.add_views: rgb must be [B,3,{self.H},{self.W}], got {tuple(rgb.shape)}")
        for b in range(int(texel.shape[0])):
            self.accumulate(texel[b], rgb[b])

    def texture(self):
        """[T,T,3]: sum / max(count, 1) where visited (the SH-initialised colour was discarded there), the initial texture elsewhere."""
        init = self.atlas.texture.reshape(-1, 3)
        c = self.count[:, None]
        return torch.where(c > 0, self.sum / c.clamp(min=1), init).reshape(self.T, self.T, 3)


def canonical_gaussians(geometry):
    """(means3D, rotations, scales, opacities, colors6) of the canonical Gaussians as the reference renders them with no timestamp
    (C/renderer/diff_sugar_rasterizer_temporal.py:149-157: ``shs = get_features``; the rasterizer's degree-0 SH colour is
    max(SH2RGB(dc), 0)); the normal half of colors6 is zero (no normal pass in that branch)."""
    from .geometry import require_sh_levels_1

    require_sh_levels_1(geometry, "texture_export.canonical_gaussians")
    rgb = geometry.get_points_rgb().clamp_min(0.0)
    return (geometry.get_xyz, geometry.get_rotation, geometry.get_scaling, geometry.get_opacity.reshape(-1),
            torch.cat([rgb, torch.zeros_like(rgb)], 1))


def bake_texture(geometry, atlas: Atlas, cameras, chunk=8, renderer=None):
    """The predict epoch: every camera of `cameras` (a ``predict_cameras`` dict) renders the canonical Gaussians on the evaluation
    (black) background, ``comp_rgb`` = clamp(0, 1), and is added to a ``TextureBaker``; `chunk` views are resident at a time.
    Returns the baker (``.texture()``)."""
    dev = geometry.device
    H, W = int(cameras["height"]), int(cameras["width"])
    if H != W:
        raise NotImplementedError("the predict dataset renders square images (export_resolution^2)")
    fovy = torch.as_tensor(cameras["fovy"], dtype=torch.float32).reshape(-1)
    if not bool((fovy == fovy[0]).all()):
        raise NotImplementedError("one fovy for all predict views (eval_fovy_deg)")
    wv, full, _ = cam_info_gaussian(cameras["c2w"].to(torch.float32).cpu(), fovy, fovy)
    baker = TextureBaker(geometry, atlas, H)
    with torch.no_grad():
        m, q, s, o, c6 = canonical_gaussians(geometry)
        r = renderer or gviews.GaussianViews(int(m.shape[0]), H, W, math.tan(0.5 * float(fovy[0])), dev)
        bg6 = torch.zeros(6, dtype=torch.float32, device=dev)
        for i in range(0, int(wv.shape[0]), int(chunk)):
            vm, pm = wv[i:i + chunk].to(dev), full[i:i + chunk].to(dev)
            out = gviews.render_gaussian_views(r, m, q, s, o, c6, vm, pm, bg6)
            baker.add_views(out["color"][:, :3].clamp(0, 1), vm, pm)
    return baker


def predict_timestamps(video_length=32):
    """The 32 export timestamps of C/system/sugar_4dgen.py:597-600: np.linspace(0, 1, L + 2)[1:-1] as float32."""
    return torch.as_tensor(np.linspace(0, 1, video_length + 2, endpoint=True), dtype=torch.float32)[1:-1]


def export_textured_sequence(out_dir, geometry, texture, timestamps, atlas: Atlas):
    """``extracted_textured_meshes/extracted_mesh_{i}.obj`` (+ .mtl, .png) for every timestamp (C/system/sugar_4dgen.py:594-640): the
    deformed surface mesh of ``geometry.get_timed_surface_mesh`` with the atlas' UVs and `texture` [T,T,3] clamped to [0, 1]
    (shared: encoded once, the same PNG bytes in every file).  Returns the OBJ paths."""
    from .wire_formats import encode_png, write_obj

    d = os.path.join(str(out_dir), "extracted_textured_meshes")
    os.makedirs(d, exist_ok=True)
    ts = torch.as_tensor(timestamps, dtype=torch.float32).reshape(-1).to(geometry.device)
    vuv, fuv = atlas.verts_uv.cpu().numpy(), atlas.faces_uv.cpu().numpy()
    png = encode_png(texture.detach().cpu().numpy())
    paths = []
    for i in range(len(ts)):
        with torch.no_grad():                               # one timestamp per call, as the reference (:612)
            verts, faces = geometry.get_timed_surface_mesh(ts[i:i + 1])
        p = os.path.join(d, f"extracted_mesh_{i}.obj")
        write_obj(p, verts[0].detach().cpu().numpy(), faces.cpu().numpy(), vuv, fuv, png)
        paths.append(p)
    return paths


def export_textured_mesh(out_dir, geometry, texture, atlas: Atlas):
    """``extracted_mesh.obj`` (+ .mtl, .png) of the canonical surface mesh (C/system/base.py:294-323)."""
    from .wire_formats import write_obj

    os.makedirs(str(out_dir), exist_ok=True)
    p = os.path.join(str(out_dir), "extracted_mesh.obj")
    write_obj(p, geometry.get_xyz_verts.detach().cpu().numpy(), geometry.get_faces.cpu().numpy(), atlas.verts_uv.cpu().numpy(),
              atlas.faces_uv.cpu().numpy(), texture.detach().cpu().numpy())
    return p
