"""Restatements shared by the mesh-extraction tests (tests/test_isosurface_cpu.py, tests/test_isosurface_gpu.py), numpy only.

* ``field_reference``: the occupancy field of DESIGN.md "Mesh extraction from Gaussians" with explicit loops over blocks and
  Gaussians.  Everything that decides something (opacity filter, centre, scale, normalised centres, block bounds, the strict
  cut-off) is float32 exactly as on the host; everything after it is float64 and never rounded.  Small N and R only.
* ``marching_cubes_reference``: marching cubes cube by cube through the table of tools/gen_mc_table.py, with the ordering rules
  of the operator: vertex ids are the ranks of ``3 * voxel + axis`` over the crossed edges, faces go cube by cube in ascending
  voxel index and in the table's order, positions / colours are float64 expressions rounded once to float32.
"""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gaussian_field.npz")


def load_generator():
    """tools/gen_mc_table.py as a module (tools/ is not a package)."""
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = load_generator()
TRI_COUNT, TRIS, MAX_TRIS = GEN.build_table()


def golden_case(z, case):
    """Case A, B or C of tests/golden/gaussian_field.npz (loaded as `z`): dict(xyz, scaling, rotation, opacity, num_blocks, occ
    (the reference's float32 grid), occ_f64 (its float64 grid: occ plus the stored float32 residual), center, scale, err_ref).
    Case B runs on case A's inputs."""
    src = "A" if case == "B" else case
    out = {k: z[f"{src}/{k}"] for k in ("xyz", "scaling", "rotation", "opacity")}
    out.update({k: z[f"{case}/{k}"] for k in ("occ", "center")})
    out.update(num_blocks=int(z[f"{case}/num_blocks"]), scale=float(z[f"{case}/scale"]), err_ref=float(z[f"{case}/err_ref"]),
               occ_f64=z[f"{case}/occ"].astype(np.float64) + z[f"{case}/occ_res"].astype(np.float64))
    return out


# ------------------------------------------------------------------------------------------------------------- the field
def normalisation(xyz, opacity):
    """(mask, center float32 [3], scale python float) by the reference's float32 operations."""
    mask = np.asarray(opacity, np.float32).reshape(-1) > np.float32(0.005)
    kept = np.asarray(xyz, np.float32)[mask]
    mn, mx = kept.min(0), kept.max(0)
    center = (mn + mx) / np.float32(2)
    scale = 1.8 / float((mx - mn).max())
    return mask, center, scale


def block_bounds(R, nb, relax_ratio=1.5):
    """float32 (coords, vmin, vmax); torch.linspace's float32 values come from the operator's own host function."""
    from dreammesh4d_amd import isosurface as iso

    return tuple(t.numpy() for t in iso.block_bounds(R, nb, relax_ratio))


def inverse_covariance(stdn, rotation):
    """[N,6] float64 (ia, ib, ic, id, ie, if): gaussian_3d_coeff's cofactor formula on cov = R diag(s^2) R^T, in float64."""
    out = np.zeros((len(stdn), 6))
    for g in range(len(stdn)):
        q = np.asarray(rotation[g], np.float64)
        w, x, y, z = q / np.sqrt((q * q).sum())
        Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                       [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                       [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        cov = Rm @ np.diag(np.asarray(stdn[g], np.float64) ** 2) @ Rm.T
        a, b, c, d, e, f = cov[0, 0], cov[0, 1], cov[0, 2], cov[1, 1], cov[1, 2], cov[2, 2]
        inv_det = 1.0 / (a * d * f + 2 * e * c * b - e ** 2 * a - c ** 2 * d - b ** 2 * f + 1e-24)
        out[g] = [(d * f - e ** 2) * inv_det, (e * c - b * f) * inv_det, (e * b - c * d) * inv_det, (a * f - c ** 2) * inv_det,
                  (b * c - e * a) * inv_det, (a * d - b ** 2) * inv_det]
    return out


def field_reference(xyz, scaling, rotation, opacity, rgb=None, resolution=32, num_blocks=4, relax_ratio=1.5):
    """-> dict(occ [R,R,R] float64, csum [R,R,R,3] float64 or None, center, scale, n_kept, n_pairs, hit [nb,nb,nb] bool: the blocks
    at least one Gaussian reaches)."""
    R, nb = int(resolution), int(num_blocks)
    s = R // nb
    mask, center, scale = normalisation(xyz, opacity)
    xyzn = (np.asarray(xyz, np.float32)[mask] - center) * np.float32(scale)
    stdn = np.asarray(scaling, np.float32)[mask] * np.float32(scale)
    assert xyzn.dtype == np.float32 and stdn.dtype == np.float32
    opa = np.asarray(opacity, np.float32).reshape(-1)[mask].astype(np.float64)
    col = None if rgb is None else np.asarray(rgb, np.float32)[mask].astype(np.float64)
    inv = inverse_covariance(stdn, np.asarray(rotation, np.float32)[mask])
    coords, vmin, vmax = block_bounds(R, nb, relax_ratio)
    occ = np.zeros((R, R, R))
    csum = None if rgb is None else np.zeros((R, R, R, 3))
    hit = np.zeros((nb, nb, nb), bool)
    n_pairs = 0
    c64 = coords.astype(np.float64)
    for bx in range(nb):
        for by in range(nb):
            for bz in range(nb):
                lo = np.array([vmin[bx], vmin[by], vmin[bz]], np.float32)
                hi = np.array([vmax[bx], vmax[by], vmax[bz]], np.float32)
                sel = np.nonzero(((xyzn > lo) & (xyzn < hi)).all(1))[0]              # float32 comparisons, strict
                n_pairs += len(sel)
                hit[bx, by, bz] = len(sel) > 0
                sx, sy, sz = (slice(b * s, (b + 1) * s) for b in (bx, by, bz))
                X, Y, Z = np.meshgrid(c64[sx], c64[sy], c64[sz], indexing="ij")
                for g in sel:                                                        # ascending Gaussian index
                    x, y, z = X - float(xyzn[g, 0]), Y - float(xyzn[g, 1]), Z - float(xyzn[g, 2])
                    ia, ib, ic, id_, ie, if_ = inv[g]
                    power = -0.5 * (x * x * ia + y * y * id_ + z * z * if_) - x * y * ib - x * z * ic - y * z * ie
                    w = np.where(power > 0, 0.0, np.exp(np.minimum(power, 0.0)))
                    occ[sx, sy, sz] += opa[g] * w
                    if csum is not None:
                        csum[sx, sy, sz] += (opa[g] * w)[..., None] * col[g]
    return {"occ": occ, "csum": csum, "center": center, "scale": scale, "n_kept": int(mask.sum()), "n_pairs": n_pairs, "hit": hit}


# ------------------------------------------------------------------------------------------------------- marching cubes
def marching_cubes_reference(f, threshold, csum=None):
    """f [R0,R1,R2] float32 -> dict(verts [V,3] float32 (index coordinates), faces [F,3] int64, colors [V,3] float32 or None,
    cases: the set of case indices that occurred)."""
    f = np.asarray(f)
    assert f.dtype == np.float32 and f.ndim == 3
    dims = f.shape
    threshold = float(threshold)
    f64 = f.astype(np.float64)
    inside = f64 >= threshold
    c64 = None if csum is None else np.asarray(csum, np.float32).astype(np.float64)
    verts, colors, edge_vertex = [], [], {}
    for i in range(dims[0]):
        for j in range(dims[1]):
            for k in range(dims[2]):
                a = (i, j, k)
                n = (i * dims[1] + j) * dims[2] + k
                for ax in range(3):
                    if a[ax] + 1 >= dims[ax]:
                        continue
                    b = tuple(a[d] + (d == ax) for d in range(3))
                    if inside[a] == inside[b]:
                        continue
                    fa, fb = f64[a], f64[b]
                    with np.errstate(all="ignore"):
                        t = (threshold - fa) / (fb - fa)
                        pos = [np.float32(a[d] + t) if d == ax else np.float32(a[d]) for d in range(3)]
                        if c64 is not None:
                            colors.append(np.float32((c64[a] + t * (c64[b] - c64[a])) / (fa + t * (fb - fa))))
                    edge_vertex[3 * n + ax] = len(verts)                             # visited in ascending 3 * n + ax
                    verts.append(pos)
    faces, cases = [], set()
    for i in range(dims[0] - 1):
        for j in range(dims[1] - 1):
            for k in range(dims[2] - 1):
                case = 0
                for c in range(8):
                    o = GEN.corner_offset(c)
                    case |= int(inside[i + o[0], j + o[1], k + o[2]]) << c
                cases.add(case)
                for t in range(TRI_COUNT[case]):
                    tri = []
                    for e in TRIS[case, t]:
                        o, ax = GEN.EDGE_BASE[e], GEN.EDGE_AXIS[e]
                        m = ((i + o[0]) * dims[1] + j + o[1]) * dims[2] + k + o[2]
                        tri.append(edge_vertex[3 * m + ax])
                    faces.append(tri)
    return {"verts": np.asarray(verts, np.float32).reshape(-1, 3), "faces": np.asarray(faces, np.int64).reshape(-1, 3),
            "colors": None if csum is None else np.asarray(colors, np.float32).reshape(-1, 3), "cases": cases}


def manifold_defects(faces):
    """(directed edges that occur more than once, directed edges whose reverse does not occur exactly once): (0, 0) for a closed,
    consistently oriented 2-manifold."""
    faces = np.asarray(faces, np.int64)
    d = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    _, count = np.unique(d, axis=0, return_counts=True)
    fwd = {(int(a), int(b)) for a, b in d}
    unmatched = sum((b, a) not in fwd for a, b in fwd)
    return int((count > 1).sum()), int(unmatched)


def euler_characteristic(n_verts, faces):
    faces = np.asarray(faces, np.int64)
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    return int(n_verts) - len(np.unique(e, axis=0)) + len(faces)


# --------------------------------------------------------------------------------------------- fields of the mesh tests
def random_sign_field(n=20, seed=0):
    """A random-sign n^3 field (values +-(0.25 .. 1)) padded with a layer of outside values: threshold 0; every sign pattern of a
    cube is equally likely, so all 256 cases occur (asserted where it is used)."""
    rng = np.random.default_rng(seed)
    f = -np.ones((n + 2,) * 3, np.float32)
    f[1:-1, 1:-1, 1:-1] = (rng.uniform(0.25, 1.0, (n,) * 3) * rng.choice([-1.0, 1.0], (n,) * 3)).astype(np.float32)
    csum = (rng.uniform(0.0, 1.0, f.shape + (3,)) * np.abs(f)[..., None]).astype(np.float32)
    return f, csum


def sphere_field(R=24, radius=0.6):
    """f = radius - |p| on [-1, 1]^3 (inside positive, threshold 0) and its gradient direction -p / |p|."""
    x = np.linspace(-1, 1, R)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    return (radius - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32)


def mesh_fields():
    """name -> (f float32, threshold, csum or None): the marching-cubes cases of the device test."""
    rng = np.random.default_rng(5)
    f_rand, c_rand = random_sign_field()
    noncubic = rng.normal(size=(7, 9, 5)).astype(np.float32)
    on_threshold = rng.integers(-2, 3, size=(9, 8, 10)).astype(np.float32) * 0.5     # many samples == threshold 0.5 exactly
    boundary = sphere_field(16, radius=1.2)                                          # the sphere leaves the grid: an open mesh
    return {"random_sign": (f_rand, 0.0, c_rand), "noncubic": (noncubic, 0.1, None), "on_threshold": (on_threshold, 0.5, None),
            "all_outside": (-np.ones((6, 6, 6), np.float32), 0.0, np.ones((6, 6, 6, 3), np.float32)),
            "boundary": (boundary, 0.0, np.abs(rng.normal(size=boundary.shape + (3,))).astype(np.float32))}


# --------------------------------------------------------------------------------------------------- Gaussian scenes
def random_gaussians(n, seed, extent=(1.0, 0.45, 0.3), sigma=(0.004, 0.008), anisotropy=4.0):
    """n Gaussians in an ellipsoid of half-axes `extent`: standard deviations sigma[0] .. sigma[1] times up to `anisotropy`
    between a Gaussian's axes, random raw quaternions, opacity 0.1 .. 1, random colours.  float32."""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3))
    p = p / np.linalg.norm(p, axis=1, keepdims=True) * rng.uniform(0, 1, (n, 1)) ** (1 / 3) * np.asarray(extent)
    base = rng.uniform(sigma[0], sigma[1], (n, 1))
    scaling = base * np.exp(rng.uniform(0, np.log(anisotropy), (n, 3)))
    rot = rng.normal(size=(n, 4)) * rng.uniform(0.5, 2.0, (n, 1))
    return {"xyz": p.astype(np.float32), "scaling": scaling.astype(np.float32), "rotation": rot.astype(np.float32),
            "opacity": rng.uniform(0.1, 1.0, n).astype(np.float32), "rgb": rng.uniform(0, 1, (n, 3)).astype(np.float32)}


def sphere_gaussians(n=2000, radius=0.5):
    """n small Gaussians spread evenly over a sphere (a golden-angle spiral, so the density has no thin spots), coloured by
    hemisphere (z >= 0: COLOR_UP, else COLOR_DOWN).  Standard deviation 5 % of the radius: the 0.8 level set of the field lies
    about 1.4 standard deviations off the sphere, inside the grid (the normalisation leaves 10 % of the bounding box as margin)."""
    k = np.arange(n) + 0.5
    z = 1 - 2 * k / n
    phi = k * np.pi * (3 - np.sqrt(5))
    p = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1) * radius
    rgb = np.where(p[:, 2:3] >= 0, np.array(COLOR_UP), np.array(COLOR_DOWN))
    return {"xyz": p.astype(np.float32), "scaling": np.full((n, 3), 0.05 * radius, np.float32),
            "rotation": np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1)), "opacity": np.full(n, 0.9, np.float32),
            "rgb": rgb.astype(np.float32)}


COLOR_UP, COLOR_DOWN = (0.9, 0.2, 0.1), (0.1, 0.3, 0.8)
