"""Timing of the textured mesh export at the shipped sizes (200 k Gaussians = 33,330 faces x 6, 120 predict views at 1024^2,
square_size_in_texture 20, 32 frames): one JSON line.  GPU parts with HIP events after one warm-up pass; host writing wall-clock.
The timed bake is the one texture_export.bake_texture runs, split into its three parts."""
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dreammesh4d_amd import gviews, sugar, synthetic as syn, texture_export as tx, wire_formats as wf  # noqa: E402
from dreammesh4d_amd.renderer import cam_info_gaussian  # noqa: E402

dev = torch.device("cuda:0")
verts, faces = syn.uv_sphere(33_330, radius=0.6)
rng = np.random.default_rng(0)
g = sugar.SuGaR(verts, faces, vertex_colors=rng.random((len(verts), 3)), device=dev)
n_views, chunk, S = tx.N_PREDICT_VIEWS, 8, 20
cams = tx.predict_cameras(n_views, seed=0)
H = W = int(cams["height"])
fovy = cams["fovy"]
wv, full, _ = cam_info_gaussian(cams["c2w"], fovy, fovy)
ev = lambda: torch.cuda.Event(enable_timing=True)


def timed(fn):
    a, b = ev(), ev()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def bake(atlas):
    baker = tx.TextureBaker(g, atlas, H)
    r = gviews.GaussianViews(g.n_gaussians, H, W, math.tan(0.5 * float(fovy[0])), dev)
    t = dict(render=0.0, raster=0.0, accumulate=0.0)
    with torch.no_grad():
        m, q, s, o, c6 = tx.canonical_gaussians(g)
        bg6 = torch.zeros(6, device=dev)
        for i in range(0, n_views, chunk):
            vm, pm = wv[i:i + chunk].to(dev), full[i:i + chunk].to(dev)
            out, ms = timed(lambda: gviews.render_gaussian_views(r, m, q, s, o, c6, vm, pm, bg6))
            t["render"] += ms
            rgb = out["color"][:, :3].clamp(0, 1).contiguous()
            texel, ms = timed(lambda: baker.rasterize(vm, pm))
            t["raster"] += ms
            _, ms = timed(lambda: [baker.accumulate(texel[b], rgb[b]) for b in range(texel.shape[0])])
            t["accumulate"] += ms
    return baker, t


atlas, _ = timed(lambda: tx.build_atlas(g, S))                  # warm-up
bake(atlas)
atlas, t_atlas = timed(lambda: tx.build_atlas(g, S))
baker, t = bake(atlas)
tex = baker.texture()
torch.cuda.synchronize()
with tempfile.TemporaryDirectory() as d:
    vuv, fuv = atlas.verts_uv.cpu().numpy(), atlas.faces_uv.cpu().numpy()
    v, f = g.get_xyz_verts.detach().cpu().numpy(), g.get_faces.cpu().numpy()
    t0 = time.perf_counter()
    png = wf.encode_png(tex.cpu().numpy())
    t1 = time.perf_counter()
    for i in range(32):
        wf.write_obj(os.path.join(d, f"extracted_mesh_{i}.obj"), v, f, vuv, fuv, png)
    t2 = time.perf_counter()
    obj_mb = os.path.getsize(os.path.join(d, "extracted_mesh_0.obj")) / 2**20
gpu_ms = t_atlas + t["render"] + t["raster"] + t["accumulate"]
print(json.dumps({"tool": "export_timing", "gaussians": g.n_gaussians, "faces": int(g.get_faces.shape[0]), "views": n_views, "resolution": H,
                  "square_size": S, "texture_size": atlas.texture_size, "visited_texels": int((baker.count > 0).sum()),
                  "atlas_init_ms": round(t_atlas, 3), "mesh_raster_resolve_ms_per_view": round(t["raster"] / n_views, 4),
                  "claim_accumulate_ms_per_view": round(t["accumulate"] / n_views, 4), "canonical_renders_ms": round(t["render"], 2),
                  "gpu_total_ms": round(gpu_ms, 2), "host_png_encode_s": round(t1 - t0, 3), "host_write_32_frames_s": round(t2 - t1, 3),
                  "obj_mb_per_frame": round(obj_mb, 2)}))
