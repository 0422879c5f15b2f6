"""Mesh extraction from Gaussians on the HIP device: the occupancy field of a set of Gaussians and marching cubes on it -- the
step that produces the coarse mesh ``mesh_simplify`` then turns into the bind mesh.

Replaces ``GaussianIO.extract_fields`` / ``extract_mesh`` (custom/threestudio-dreammesh4d/geometry/gaussian_io.py:174-291: a
triple Python loop over blocks, then ``mcubes.marching_cubes`` on the CPU) with the kernels of ``csrc/isosurface.hip``
("Mesh extraction from Gaussians"):

* the field follows ``extract_fields`` line by line -- opacity filter ``> 0.005``, normalisation to about [-1, 1] by the kept
  Gaussians' bounding box, the per-block hard cut-off ``vmin < centre < vmax`` -- with the reference's float32 operations wherever
  they decide something (so the cull decisions are the reference's), the inverse covariance in float64 rounded once, and a
  float64 sum per voxel in ascending Gaussian index rounded once.  No atomics: two runs give the same bytes;
* marching cubes is a function of the field alone: one vertex per crossed grid edge, numbered by ascending
  ``3 * voxel + axis``; faces cube by cube in ascending voxel index, in the order of the generated table
  (``tools/gen_mc_table.py`` -> ``csrc/mc_table.h``), normals toward lower field values.

The reference's ``clean_mesh`` up to its repair filters -- unreferenced vertices, null and duplicate faces, small connected
components -- is ``dreammesh4d_amd.mesh_clean`` (``extract_mesh(..., clean=True)``, ``--clean``).  Not restated: the repair and
remeshing half of ``clean_mesh(remesh=True)`` and ``decimate_mesh`` (pymeshlab).  The next step here is
``python -m dreammesh4d_amd.mesh_simplify``.  The sort of the pair keys and the prefix sums are torch calls on the device;
everything else is HIP.  There is no CPU path.

    python -m dreammesh4d_amd.isosurface --ply gaussians.ply --resolution 128 --density_thresh 0.8 --output out_dir [--clean]
"""
import argparse
import math
import os

import numpy as np
import torch

from ._args import no_cpu_path as _no_cpu_path

OPACITY_FLOOR = 0.005


def _checked_grid(resolution, num_blocks):
    from . import _lib

    for name, v in (("resolution", resolution), ("num_blocks", num_blocks)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"gaussian_density_field: {name} must be an integer (got {v!r})")
    R, nb = int(resolution), int(num_blocks)
    if R < 2 or R > _lib.ISO_MAX_RESOLUTION:
        raise ValueError(f"gaussian_density_field: resolution must lie in [2, {_lib.ISO_MAX_RESOLUTION}] (got {R})")
    if nb < 1 or R % nb != 0:
        raise ValueError(f"gaussian_density_field: resolution {R} must be a multiple of num_blocks = {nb}")
    return R, nb


def block_bounds(resolution, num_blocks, relax_ratio=1.5):
    """(coords [R], vmin [num_blocks], vmax [num_blocks]) as float32 CPU tensors, by the reference's float32 operations: the grid
    coordinates ``torch.linspace(-1, 1, R)``, and per block the first coordinate minus / the last plus
    ``block_size * relax_ratio`` with ``block_size = 2 / num_blocks``."""
    R, nb = _checked_grid(resolution, num_blocks)
    s = R // nb
    coords = torch.linspace(-1, 1, R)
    block_size = 2 / nb
    vmin = coords[0::s].clone()
    vmax = coords[s - 1::s].clone()
    vmin -= block_size * relax_ratio
    vmax += block_size * relax_ratio
    return coords, vmin, vmax


def gaussian_density_field(xyz, scaling, rotation, opacity, rgb=None, resolution=128, num_blocks=16, relax_ratio=1.5):
    """xyz [N,3], scaling [N,3] (standard deviations), rotation [N,4] (w, x, y, z; raw, normalised here), opacity [N] or [N,1],
    rgb [N,3] or None -- float32 tensors on one HIP device.

    -> dict(occ [R,R,R] float32, csum [R,R,R,3] float32 (the opacity-weighted colour sum; ``csum / occ`` is the colour) or None,
    center [3] float32 tensor, scale (float), n_kept (Gaussians with opacity > 0.005), n_pairs ((Gaussian, block) pairs)).

    Raises ValueError for a resolution outside [2, 512] or no multiple of ``num_blocks``, N == 0, nothing left after the
    opacity filter, a bounding box without extent and non-finite input; ``_lib.Dm4dError`` for CPU tensors."""
    from . import _lib

    what = "gaussian_density_field"
    tensors = [("xyz", xyz, 3), ("scaling", scaling, 3), ("rotation", rotation, 4), ("opacity", opacity, 1)]
    if rgb is not None:
        tensors.append(("rgb", rgb, 3))
    for name, t, _ in tensors:
        if not torch.is_tensor(t):
            raise TypeError(f"{what}: {name} must be a torch tensor")
    R, nb = _checked_grid(resolution, num_blocks)
    if not (isinstance(relax_ratio, (int, float)) and math.isfinite(relax_ratio)):
        raise ValueError(f"{what}: relax_ratio must be a finite number (got {relax_ratio!r})")
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{what}: xyz must be [N,3] (got {tuple(xyz.shape)})")
    N = int(xyz.shape[0])
    if N == 0:
        raise ValueError(f"{what}: no Gaussians (N == 0)")
    for name, t, k in tensors:
        ok = tuple(t.shape) == (N, k) or (name == "opacity" and tuple(t.shape) == (N,))
        if not ok or t.dtype != torch.float32:
            raise ValueError(f"{what}: {name} must be float32 [{N},{k}] (got {t.dtype} {tuple(t.shape)})")
    dev = xyz.device
    if any(t.device != dev for _, t, _ in tensors):
        raise _no_cpu_path(what)
    xyz, scaling, rotation = xyz.detach(), scaling.detach(), rotation.detach()
    opacity = opacity.detach().reshape(N)
    rgb = None if rgb is None else rgb.detach()
    # the data-dependent refusals are plain torch, so they read the same on any device; one host visit for all of them
    finite = torch.stack([torch.isfinite(t).all() for t in (xyz, scaling, rotation, opacity) + (() if rgb is None else (rgb,))]).all()
    mask = opacity > OPACITY_FLOOR
    n_kept = int(mask.sum())
    if not bool(finite):
        raise ValueError(f"{what}: the input is not all finite")
    if n_kept == 0:
        raise ValueError(f"{what}: no Gaussian has opacity > {OPACITY_FLOOR}")
    xyz_k = xyz[mask]
    mn, mx = xyz_k.amin(0), xyz_k.amax(0)
    center = (mn + mx) / 2
    extent = (mx - mn).amax().item()
    if not (extent > 0.0 and math.isfinite(extent)):
        raise ValueError(f"{what}: the kept Gaussians' bounding box has no extent")
    scale = 1.8 / extent
    if dev.type != "cuda":
        raise _no_cpu_path(what)
    xyzn = ((xyz_k - center) * scale).contiguous()                  # fl32((x - center) * fl32(scale)), as the reference
    stdn = (scaling[mask] * scale).contiguous()
    rot_k = rotation[mask].contiguous()
    opa_k = opacity[mask].contiguous()
    rgb_k = None if rgb is None else rgb[mask].contiguous()
    coords, vmin, vmax = (t.to(dev) for t in block_bounds(R, nb, relax_ratio))
    f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = _lib.stream(dev)
        records = torch.empty(n_kept, _lib.ISO_RECORD_FLOATS, **f32)
        box = torch.empty(n_kept, 6, dtype=torch.int32, device=dev)
        count = torch.empty(n_kept, **i64)
        _lib.call("dm4d_iso_gaussian_records", n_kept, xyzn.data_ptr(), stdn.data_ptr(), rot_k.data_ptr(), opa_k.data_ptr(), _lib.ptr(rgb_k),
                  nb, vmin.data_ptr(), vmax.data_ptr(), records.data_ptr(), box.data_ptr(), count.data_ptr(), st)
        ends = torch.cumsum(count, 0)
        n_pairs = int(ends[-1])
        offset = (ends - count).contiguous()
        keys = torch.empty(n_pairs, **i64)
        _lib.call("dm4d_iso_pair_keys", n_kept, n_pairs, nb, box.data_ptr(), offset.data_ptr(), keys.data_ptr(), st)
        keys = torch.sort(keys).values                              # keys are distinct: block-major, ascending Gaussian within a block
        block_start = torch.searchsorted(keys, torch.arange(nb ** 3 + 1, **i64) * n_kept).contiguous()
        occ = torch.empty(R, R, R, **f32)
        csum = None if rgb is None else torch.empty(R, R, R, 3, **f32)
        _lib.call("dm4d_iso_density_field", n_kept, n_pairs, R, nb, coords.data_ptr(), records.data_ptr(), keys.data_ptr(),
                  block_start.data_ptr(), occ.data_ptr(), _lib.ptr(csum), st)
    return {"occ": occ, "csum": csum, "center": center, "scale": scale, "n_kept": n_kept, "n_pairs": n_pairs}


def marching_cubes(occ, threshold, csum=None):
    """occ [R0,R1,R2] float32 on a HIP device, threshold a number, csum [R0,R1,R2,3] float32 or None.

    -> dict(verts [V,3] float32 in INDEX coordinates, faces [F,3] int64, colors [V,3] float32 or None).  A grid point is inside
    when ``occ >= threshold``; the output is welded (one vertex per crossed edge) and a function of the input alone -- see the
    module docstring for the order of vertices and faces."""
    from . import _lib

    what = "marching_cubes"
    if not torch.is_tensor(occ) or (csum is not None and not torch.is_tensor(csum)):
        raise TypeError(f"{what}: occ and csum must be torch tensors")
    if occ.ndim != 3 or occ.dtype != torch.float32 or min(occ.shape) < 1:
        raise ValueError(f"{what}: occ must be float32 [R0,R1,R2] (got {occ.dtype} {tuple(occ.shape)})")
    if csum is not None and (tuple(csum.shape) != tuple(occ.shape) + (3,) or csum.dtype != torch.float32):
        raise ValueError(f"{what}: csum must be float32 {tuple(occ.shape) + (3,)} (got {csum.dtype} {tuple(csum.shape)})")
    threshold = float(threshold)
    if math.isnan(threshold):
        raise ValueError(f"{what}: the threshold is not a number")
    R0, R1, R2 = (int(x) for x in occ.shape)
    total = R0 * R1 * R2
    if 3 * total >= 1 << 31:
        raise ValueError(f"{what}: a {R0} x {R1} x {R2} grid has more than 2^31 edges")
    dev = occ.device
    if dev.type != "cuda" or (csum is not None and csum.device != dev):
        raise _no_cpu_path(what)
    occ = occ.detach().contiguous()
    csum = None if csum is None else csum.detach().contiguous()
    i32 = dict(dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = _lib.stream(dev)
        code, n_tris, n_verts = torch.empty(total, **i32), torch.empty(total, **i32), torch.empty(total, **i32)
        _lib.call("dm4d_iso_mc_classify", R0, R1, R2, occ.data_ptr(), threshold, code.data_ptr(), n_tris.data_ptr(), n_verts.data_ptr(), st)
        vert_end = torch.cumsum(n_verts, 0, dtype=torch.int64)
        tri_end = torch.cumsum(n_tris, 0, dtype=torch.int64)
        V, F = (int(x) for x in torch.stack([vert_end[-1], tri_end[-1]]).cpu())
        vert_start, tri_start = (vert_end - n_verts).contiguous(), (tri_end - n_tris).contiguous()
        verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
        colors = None if csum is None else torch.empty(V, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(F, 3, dtype=torch.int64, device=dev)
        edge_vertex = torch.empty(3 * total, **i32)                 # dense; only the slots of crossed edges are written and read
        _lib.call("dm4d_iso_mc_vertices", R0, R1, R2, occ.data_ptr(), _lib.ptr(csum), threshold, code.data_ptr(), vert_start.data_ptr(), V,
                  verts.data_ptr(), _lib.ptr(colors), edge_vertex.data_ptr(), st)
        _lib.call("dm4d_iso_mc_faces", R0, R1, R2, code.data_ptr(), tri_start.data_ptr(), edge_vertex.data_ptr(), F, faces.data_ptr(), st)
    return {"verts": verts, "faces": faces, "colors": colors}


def _gaussians_of(geometry_or_dict):
    """(xyz, scaling, rotation, opacity, rgb or None) of a dict of tensors or of an object with the ``get_*`` surface."""
    g = geometry_or_dict
    if isinstance(g, dict):
        missing = [k for k in ("xyz", "scaling", "rotation", "opacity") if k not in g]
        if missing:
            raise ValueError(f"extract_mesh: the dict lacks {missing}")
        return g["xyz"], g["scaling"], g["rotation"], g["opacity"], g.get("rgb")
    val = lambda name: getattr(g, name)() if callable(getattr(g, name)) else getattr(g, name)       # properties here, methods elsewhere
    rgb = None
    if int(getattr(g, "sh_levels", 1)) == 1 and hasattr(g, "get_points_rgb"):
        rgb = g.get_points_rgb()
    return val("get_xyz"), val("get_scaling"), val("get_rotation"), val("get_opacity"), rgb


def extract_mesh(geometry_or_dict, density_thresh=0.8, resolution=128, num_blocks=16, clean=False, min_f=64, min_d=20.0, keep="all"):
    """The coloured mesh of a set of Gaussians: ``gaussian_density_field`` then ``marching_cubes`` at ``density_thresh``, vertices
    back in world coordinates ``(v / (R - 1) * 2 - 1) / scale + center``.

    ``geometry_or_dict``: a dict of tensors (xyz, scaling, rotation, opacity, optional rgb) or any object with ``get_xyz``,
    ``get_scaling``, ``get_rotation`` and ``get_opacity`` (the ``SuGaR`` classes); its colour is ``get_points_rgb()`` when
    ``sh_levels == 1``, otherwise the mesh has no colour.

    -> dict(verts [V,3] float32, faces [F,3] int64, colors [V,3] float32 or None, n_kept, n_pairs, center, scale).

    The reference's ``extract_mesh`` goes on to ``clean_mesh(remesh=True)`` and ``decimate_mesh``.  ``clean=True`` runs
    ``mesh_clean.clean_mesh(verts, faces, colors, min_f, min_d, keep)`` on the mesh: verts, faces and colors are then the cleaned
    ones and the dict also carries vertex_map, face_map, labels, n_components, n_null, n_duplicate and n_small.  The default leaves
    the output as marching cubes made it.  The repair and remeshing filters and ``decimate_mesh`` need pymeshlab; they are not
    restated.  The next step here is ``dreammesh4d_amd.mesh_simplify``."""
    with torch.no_grad():
        xyz, scaling, rotation, opacity, rgb = _gaussians_of(geometry_or_dict)
        f32 = lambda t: None if t is None else t.detach().to(torch.float32)
        field = gaussian_density_field(f32(xyz), f32(scaling), f32(rotation), f32(opacity), f32(rgb), resolution=resolution,
                                       num_blocks=num_blocks)
        mesh = marching_cubes(field["occ"], density_thresh, field["csum"])
        R = int(resolution)
        verts = (mesh["verts"] / (R - 1.0) * 2 - 1) / field["scale"] + field["center"]
    res = {"verts": verts, "faces": mesh["faces"], "colors": mesh["colors"], "n_kept": field["n_kept"], "n_pairs": field["n_pairs"],
           "center": field["center"], "scale": field["scale"]}
    if clean:
        from . import mesh_clean

        res.update(mesh_clean.clean_mesh(verts, mesh["faces"], mesh["colors"], min_f=min_f, min_d=min_d, keep=keep))
    return res


def output_path(ply_path, output):
    """``{output}/{stem}_mc.ply``, stem = the file name up to its first dot."""
    return os.path.join(output, os.path.basename(ply_path).split(".")[0] + "_mc.ply")


def _parser():
    from . import mesh_clean

    p = argparse.ArgumentParser(prog="python -m dreammesh4d_amd.isosurface", description=__doc__.split("\n")[0])
    p.add_argument("--ply", required=True, help="3D Gaussian splatting .ply (the layout of GaussianIO.save_ply)")
    p.add_argument("--resolution", default=128, type=int, help="grid points per axis")
    p.add_argument("--num_blocks", default=16, type=int, help="blocks per axis of the cut-off")
    p.add_argument("--density_thresh", default=0.8, type=float, help="iso value of the occupancy")
    p.add_argument("--output", required=True, help="directory of the output mesh")
    p.add_argument("--clean", action="store_true", help="remove null and duplicate faces and small components (mesh_clean) before writing")
    mesh_clean.add_arguments(p)
    return p


def main(argv=None):
    from . import wire_formats as wf

    args = _parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise _no_cpu_path("isosurface")
    g = wf.read_gaussian_ply(args.ply)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    res = extract_mesh({k: t(g[k]) for k in ("xyz", "scaling", "rotation", "opacity", "rgb")}, density_thresh=args.density_thresh,
                       resolution=args.resolution, num_blocks=args.num_blocks, clean=args.clean, min_f=args.min_f, min_d=args.min_d, keep=args.keep)
    print(f"{len(g['xyz'])} Gaussians, {res['n_kept']} kept (opacity > {OPACITY_FLOOR}), {res['n_pairs']} (Gaussian, block) pairs")
    if args.clean:
        print(f"{res['n_null']} null and {res['n_duplicate']} duplicate faces, {res['n_components']} components, {res['n_small']} of them small")
    print(f"Extracted mesh has {len(res['verts'])} vertices and {len(res['faces'])} triangles")
    os.makedirs(args.output, exist_ok=True)
    path = output_path(args.ply, args.output)
    wf.write_ply(path, res["verts"].cpu().numpy(), res["faces"].cpu().numpy(), colors=None if res["colors"] is None else res["colors"].cpu().numpy())
    return path


if __name__ == "__main__":
    main()
