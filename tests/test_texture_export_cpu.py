"""CPU checks of the textured mesh export's host side: the UV atlas and its texel layout against an independent loop restatement of
C/system/base.py:78-209 (C/ = custom/threestudio-dreammesh4d/), hand-computed values, the OBJ / MTL / PNG round trip and the predict
camera sampler."""
import math

import numpy as np
import pytest
import torch

from dreammesh4d_amd import texture_export as tx
from dreammesh4d_amd import wire_formats as wf


def _loop_atlas(F, S):
    """Restatement with explicit loops: texture_size, per-face UV corners in texels, and {(row, col): (face, bary)} after the
    transpose and flip."""
    n = int(math.sqrt(F // 2 + 1) + 1)
    T = S * n
    corners = {}
    texels = {}
    bottom = [(i, j) for i in range(S - 1) for j in range(i + 1)]
    top = [(i, j) for i in range(S) for j in range(i + 1, S)]
    for f in range(F):
        k, is_top = f // 2, f % 2
        a, b = k // n, k % n
        if not is_top:
            corners[f] = [((a + 1) * S - 2, b * S + 1), (a * S + 2, b * S + 1), ((a + 1) * S - 2, (b + 1) * S - 3)]
        else:
            corners[f] = [(a * S + 1, (b + 1) * S - 1), (a * S + 1, b * S + 3), ((a + 1) * S - 3, (b + 1) * S - 1)]
        for ti, tj in (top if is_top else bottom):
            if not is_top:
                b1, b2 = (S - 2 - ti) / (S - 3), (tj - 1) / (S - 3)
            else:
                b1, b2 = (ti - 1) / (S - 3), (S - 1 - tj) / (S - 3)
            i, j = a * S + ti, b * S + tj                     # texture_img[i, j]
            r, c = T - 1 - j, i                               # transpose, then flip(0)
            assert (r, c) not in texels
            texels[(r, c)] = (f, (1 - b1 - b2, b1, b2))
    return T, n, corners, texels


@pytest.mark.parametrize("F", [1, 2, 5, 37, 1001])
@pytest.mark.parametrize("S", [4, 20])
def test_atlas_matches_a_loop_restatement(F, S):
    T, n, corners, texels = _loop_atlas(F, S)
    assert tx.atlas_size(F, S) == (T, n)
    faces_uv, verts_uv = tx.atlas_uv(F, S)
    assert faces_uv.dtype == torch.int64 and torch.equal(faces_uv, torch.arange(3 * F).view(F, 3))
    assert tuple(verts_uv.shape) == (6 * n * n, 2) and verts_uv.dtype == torch.float32
    uv_texels = verts_uv.double() * T
    for f in range(F):
        got = uv_texels[faces_uv[f]]
        assert torch.equal(verts_uv[faces_uv[f]], torch.tensor(corners[f], dtype=torch.float32) / T), f    # int / int in float32
        # inside the face's own square (squares are disjoint cells of the n x n grid)
        a, b = (f // 2) // n, (f // 2) % n
        assert bool(((got[:, 0] >= a * S) & (got[:, 0] <= (a + 1) * S) & (got[:, 1] >= b * S) & (got[:, 1] <= (b + 1) * S)).all())
    face, row, col, bary = tx.atlas_texels(F, S)
    K = S * (S - 1) // 2
    assert face.numel() == F * K == len(texels)
    pos = set()
    for i in range(face.numel()):
        key = (int(row[i]), int(col[i]))
        assert key not in pos                                 # every written texel belongs to exactly one face
        pos.add(key)
        f_ref, b_ref = texels[key]
        assert int(face[i]) == f_ref
        assert np.allclose(bary[i].numpy(), b_ref, atol=1e-6)
    assert torch.allclose(bary.sum(-1), torch.ones(F * K), atol=1e-6)
    assert int(row.min()) >= 0 and int(row.max()) < T and int(col.min()) >= 0 and int(col.max()) < T


def test_atlas_hand_computed_two_faces_square_size_4():
    """F = 2, S = 4: n = int(sqrt(2) + 1) = 2, T = 8; both faces in square (0, 0)."""
    faces_uv, verts_uv = tx.atlas_uv(2, 4)
    assert tx.atlas_size(2, 4) == (8, 2)
    # bottom: (1,0)*4+(-2,1), (0,0)*4+(2,1), (1,1)*4+(-2,-3); top: (0,1)*4+(1,-1), (0,0)*4+(1,3), (1,1)*4+(-3,-1); / 8
    want = torch.tensor([[2, 1], [2, 1], [2, 1], [1, 3], [1, 3], [1, 3]], dtype=torch.float32) / 8
    assert torch.equal(verts_uv[:6], want) and torch.equal(faces_uv, torch.tensor([[0, 1, 2], [3, 4, 5]]))
    assert torch.equal(verts_uv[6:12], torch.tensor([[2, 5], [2, 5], [2, 5], [1, 7], [1, 7], [1, 7]], dtype=torch.float32) / 8)
    face, row, col, bary = tx.atlas_texels(2, 4)
    # bottom (ti, tj): (0,0) (1,0) (1,1) (2,0) (2,1) (2,2) -> row 7 - tj, col ti; top (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
    assert face.tolist() == [0] * 6 + [1] * 6
    assert row.tolist() == [7, 7, 6, 7, 6, 5, 6, 5, 4, 5, 4, 4]
    assert col.tolist() == [0, 1, 1, 2, 2, 2, 0, 0, 0, 1, 1, 2]
    # S - 3 = 1: bottom (1 - b1 - b2, 2 - ti, tj - 1), top (1 - b1 - b2, ti - 1, 3 - tj)
    assert bary[:3].tolist() == [[0.0, 2.0, -1.0], [1.0, 1.0, -1.0], [0.0, 1.0, 0.0]]
    assert bary[6:9].tolist() == [[0.0, -1.0, 2.0], [1.0, -1.0, 1.0], [2.0, -1.0, 0.0]]


def test_obj_mtl_png_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    v = (rng.normal(size=(200, 3)) * 10.0 ** rng.integers(-6, 4, size=(200, 1))).astype(np.float32)
    f = rng.integers(0, 200, size=(300, 3))
    vt = rng.random((900, 2)).astype(np.float32)
    ft = np.arange(900).reshape(300, 3)
    tex = rng.random((33, 47, 3)).astype(np.float32) * 1.4 - 0.2
    tex[0, 0] = [0.5 / 255, 1.5 / 255, 2.5 / 255]                      # rounding ties
    p = tmp_path / "sub" / "mesh_a.obj"
    p.parent.mkdir()
    wf.write_obj(str(p), v, f, vt, ft, tex)
    text = p.read_text().splitlines()
    assert text[0] == "mtllib mesh_a.mtl" and (tmp_path / "sub" / "mesh_a.png").exists()
    assert "map_Kd mesh_a.png" in (tmp_path / "sub" / "mesh_a.mtl").read_text()
    assert sum(ln.startswith("f ") for ln in text) == 300 and "/" in [ln for ln in text if ln.startswith("f ")][0]
    r = wf.read_obj(str(p))
    assert r["verts"].dtype == np.float32 and np.array_equal(r["verts"].view(np.uint32), v.view(np.uint32))
    assert np.array_equal(r["verts_uvs"].view(np.uint32), vt.view(np.uint32))
    assert np.array_equal(r["faces"], f) and np.array_equal(r["faces_uvs"], ft)
    want = np.rint(np.clip(tex.astype(np.float64), 0, 1) * 255).astype(np.uint8)
    assert np.array_equal(r["texture"], want)
    # PNG bytes given directly are written as they are
    png = wf.encode_png(tex)
    wf.write_obj(str(tmp_path / "b.obj"), v, f, vt, ft, png)
    assert (tmp_path / "b.png").read_bytes() == png == (tmp_path / "sub" / "mesh_a.png").read_bytes()


def test_predict_cameras_seeded_with_the_reference_ranges():
    a = tx.predict_cameras(seed=3)
    b = tx.predict_cameras(seed=3)
    c = tx.predict_cameras(seed=4)
    assert all(torch.equal(a[k], b[k]) for k in ("c2w", "fovy", "elevation_deg", "azimuth_deg", "camera_distances"))
    assert not torch.equal(a["c2w"], c["c2w"])
    assert a["c2w"].shape == (120, 4, 4) and a["height"] == a["width"] == 1024
    assert torch.allclose(a["fovy"], torch.full((120,), math.radians(20.0)))
    for s in range(8):
        d = tx.predict_cameras(seed=s)
        assert bool((d["azimuth_deg"] >= -180).all() and (d["azimuth_deg"] < 180).all())
        assert bool((d["elevation_deg"] >= -10 - 1e-4).all() and (d["elevation_deg"] <= 80 + 1e-4).all())
        assert torch.allclose(d["camera_distances"], torch.full((120,), 3.8))
        pos = d["c2w"][:, :3, 3]
        assert torch.allclose(pos.norm(dim=-1), torch.full((120,), 3.8), atol=1e-5)
        el = torch.rad2deg(torch.asin(pos[:, 2] / 3.8))
        assert torch.allclose(el, d["elevation_deg"], atol=1e-3)
        R = d["c2w"][:, :3, :3]
        assert torch.allclose(R.transpose(1, 2) @ R, torch.eye(3).expand(120, 3, 3), atol=1e-5)
        assert torch.allclose(R[:, :, 2], pos / 3.8, atol=1e-5)                  # camera looks at the origin (-z axis)
    u = tx.predict_cameras(n=16, seed=0, batch_uniform_azimuth=True)
    k = ((u["azimuth_deg"] + 180) / 360 * 16).floor()
    assert torch.equal(k, torch.arange(16, dtype=k.dtype))


def test_predict_timestamps_are_the_reference_float32_linspace():
    t = tx.predict_timestamps()
    assert t.dtype == torch.float32 and t.numel() == 32
    assert np.array_equal(t.numpy(), np.linspace(0, 1, 34).astype(np.float32)[1:-1])


def test_export_keys_of_the_system_config():
    from dreammesh4d_amd import threestudio_host as ts

    c = ts.parse_structured(ts._BaseSuGaRSystemConfig, {})
    assert (c.postprocess, c.square_size_in_texture, c.export_resolution) == (False, 20, 1024)
    assert (c.postprocess_density_threshold, c.postprocess_iterations) == (0.1, 5)
