"""ARAPCoach(verts, None, device): the point-cloud branch of the reference's coach (utils/arap_utils.py:46-70) on the kNN graph
of dreammesh4d_amd.knn, against a float64 autograd restatement of the reference's energy on the DIRECTED 8-neighbour graph."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arap_small.npz")
V, T, K = 200, 2, 8


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _rotations(gen, shape, scale):
    q = torch.nn.functional.normalize(torch.cat([scale * torch.randn(*shape, 3, generator=gen), torch.ones(*shape, 1)], -1), dim=-1)
    x, y, z, w = q.double().unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w),
                        1 - 2 * (x * x + z * z), 2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w),
                        1 - 2 * (x * x + y * y)], -1).reshape(*shape, 3, 3)


@functools.lru_cache(maxsize=None)
def _case():
    from dreammesh4d_amd.knn import knn_points
    from dreammesh4d_amd.mesh_reg import ARAPCoach

    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(21)
    verts = torch.rand(V, 3, generator=gen)
    coach = ARAPCoach(verts, None, dev)
    nn = knn_points(verts.to(dev), verts.to(dev), K, exclude_self=True)
    idx, d2 = nn.idx.cpu(), nn.dists.cpu()
    w = torch.exp(-(d2 - d2.min(dim=1, keepdim=True).values) / d2.max(dim=1, keepdim=True).values)      # float32
    xyz = verts[None] + 0.02 * torch.randn(T, V, 3, generator=gen)
    R = _rotations(gen, (T, V), 0.1).float()
    return coach, verts, idx, d2, w, xyz, R


def _energy64(verts, idx, w, x, R):
    """The reference's compute_arap_energy with given rotations (arap_utils.py:192-193,219-222) on the directed graph, float64:
    sum_i sum_n w_in |(x'_i - x'_j) - R_i (x_i - x_j)|^2 with j = idx[i, n].  x [T,V,3], R [T,V,3,3] -> [T]."""
    P = (verts[:, None, :] - verts[idx]).double()                         # [V,K,3]
    Pp = x[:, :, None, :] - x[:, idx]                                      # [T,V,K,3]
    rot = torch.einsum("tvab,vkb->tvka", R, P)
    return (w.double()[None] * ((Pp - rot) ** 2).sum(-1)).sum(dim=(1, 2))


def test_neighbours_and_weights():
    _need_gpu()
    coach, verts, idx, d2, w, _, _ = _case()
    assert coach.max_n_neighbors == K and coach.n_verts == V and coach.is_knn
    assert [coach.one_ring_neighbors[i] for i in range(V)] == idx.tolist()
    off = coach._off.cpu().numpy()
    src, nbr, we = coach.edge_sources, coach.edge_targets, coach.edge_weights
    assert len(src) == len(nbr) == len(we) == off[-1] and np.array_equal(np.repeat(np.arange(V), np.diff(off)), src)
    for i in range(V):
        assert np.array_equal(nbr[off[i]:off[i] + K], idx[i].numpy())                      # kNN edges first, in kNN order
        assert np.array_equal(we[off[i]:off[i] + K], w[i].numpy())                         # the float32 formula, bit for bit
        assert (we[off[i] + K:off[i + 1]] == 0).all()                                      # then the reverse-only ones
    assert float(w.max()) == 1.0 and float(w.min()) >= float(np.exp(np.float32(-1.0))) * (1 - 1e-6)
    # the reverse index is an involution onto the opposite edge, the rest edges are x_src - x_nbr
    rev = coach._rev.cpu().numpy()
    assert np.array_equal(src[rev], nbr) and np.array_equal(nbr[rev], src) and np.array_equal(rev[rev], np.arange(len(rev)))
    assert np.array_equal(coach._e.cpu().numpy(), (verts[src] - verts[nbr]).numpy())


def test_energy_and_gradients_against_float64():
    _need_gpu()
    coach, verts, idx, _, w, xyz, R = _case()
    dev = coach.device
    wts = torch.tensor([1.0, -0.5])
    xc, Rc = xyz.double().requires_grad_(True), R.double().requires_grad_(True)
    Eo = _energy64(verts, idx, w, xc, Rc)
    (Eo * wts.double()).sum().backward()
    xg, Rg = xyz.to(dev).requires_grad_(True), R.to(dev).requires_grad_(True)
    Eh = coach.compute_arap_energy(xg, Rg)
    assert Eh.shape == (T,)
    print("energy", Eh.tolist(), Eo.tolist())
    # the bars of tests/test_mesh_reg_gpu.py for the mesh coach against its oracle
    assert (Eh.cpu().double() - Eo.detach()).abs().max() <= 1e-4 * Eo.detach().abs().max()
    (Eh * wts.to(dev)).sum().backward()
    assert (xg.grad.cpu().double() - xc.grad).abs().max() <= 1e-4 * xc.grad.abs().max()
    assert (Rg.grad.cpu().double() - Rc.grad).abs().max() <= 1e-4 * Rc.grad.abs().max()
    # the single form is the T = 1 batch
    x1, R1 = xyz[0].to(dev).requires_grad_(True), R[0].to(dev).requires_grad_(True)
    E1 = coach.compute_arap_energy(x1, R1)
    assert E1.dim() == 0 and float(E1.detach()) == float(Eh[0].detach())
    E1.backward()
    x2, R2 = xyz.to(dev).requires_grad_(True), R.to(dev).requires_grad_(True)
    coach.compute_arap_energy(x2, R2)[0].backward()
    assert torch.equal(x1.grad, x2.grad[0]) and torch.equal(R1.grad, R2.grad[0])


def test_rest_pose_and_rigid_motion():
    _need_gpu()
    coach, verts, _, _, _, xyz, _ = _case()
    dev = coach.device
    eye = torch.eye(3, device=dev).expand(V, 3, 3).contiguous()
    assert float(coach.compute_arap_energy(verts.to(dev), eye)) == 0.0
    gen = torch.Generator().manual_seed(4)
    Q = _rotations(gen, (), 1.0)                                               # one large rotation, float64
    t = torch.tensor([0.3, -0.2, 0.5], dtype=torch.float64)
    moved = (verts.double() @ Q.T + t).float()
    size = float((moved - verts).norm(dim=1).mean())
    E_rigid = float(coach.compute_arap_energy(moved.to(dev), Q.float().expand(V, 3, 3).contiguous().to(dev)))
    noise = torch.randn(V, 3, generator=gen)
    noise = noise * size / noise.norm(dim=1).mean()
    E_rand = float(coach.compute_arap_energy((verts + noise).to(dev), eye))
    # float32 rounding of one residual component: x'_i, x'_j and their difference (2 ulp of the largest coordinate), the
    # rounded rotation and its three products and two sums on an edge no longer than 2 * scale -- under 32 * 2^-24 * scale
    # in all; at most 8 edges of weight <= 1 per vertex, three components
    scale = float(moved.abs().max())
    bound = 8 * V * 3 * (32 * 2.0 ** -24 * scale) ** 2
    print(f"rigid {E_rigid:.3e} (rounding bound {bound:.3e}), random displacement of equal size {E_rand:.3e}")
    assert 0.0 <= E_rigid <= bound
    assert bound < 1e-8 * E_rand


def test_symmetric_and_asymmetric_pairs():
    _need_gpu()
    coach, verts, idx, _, w, xyz, R = _case()
    dev = coach.device
    nb = [set(r) for r in idx.tolist()]
    sym = next((i, j) for i in range(V) for j in idx[i].tolist() if i in nb[j])
    asym = next((i, j) for i in range(V) for j in idx[i].tolist() if i not in nb[j])
    off, nbr, we = coach._off.cpu().numpy(), coach.edge_targets, coach.edge_weights
    edge = lambda a, b: off[a] + int(np.flatnonzero(nbr[off[a]:off[a + 1]] == b)[0])
    i, j = sym
    assert we[edge(i, j)] > 0 and we[edge(j, i)] > 0 and edge(i, j) < off[i] + K and edge(j, i) < off[j] + K
    i, j = asym
    back = edge(j, i)
    assert we[edge(i, j)] == w[i, idx[i].tolist().index(j)] > 0
    assert back >= off[j] + K and we[back] == 0.0                             # added, weightless, behind j's own 8
    assert coach._rev.cpu().numpy()[back] == edge(i, j)
    assert np.array_equal(coach._e.cpu().numpy()[back], (verts[j] - verts[i]).numpy())
    assert j in coach.one_ring_neighbors[i] and i not in coach.one_ring_neighbors[j]
    # the energy is quadratic in x', so a central difference is exact up to the rounding of the two energies: each is a
    # float32 sum of fewer than 64 roundings deep (<= 6 per term, <= 24 terms per vertex, pairwise over the vertices)
    x0, R0 = xyz[0].to(dev), R[0].to(dev)
    xg = x0.clone().requires_grad_(True)
    coach.compute_arap_energy(xg, R0).backward()
    h, c = 0.05, 1
    step = torch.zeros_like(x0)
    step[j, c] = h
    Ep, Em = float(coach.compute_arap_energy(x0 + step, R0)), float(coach.compute_arap_energy(x0 - step, R0))
    fd, g = (Ep - Em) / (2 * h), float(xg.grad[j, c])
    tol = 64 * 2.0 ** -24 * (Ep + Em) / (2 * h) + 1e-4 * abs(g)
    # and the float64 restatement says how much of that gradient reaches j only through i's edge
    xc = xyz[0].double().requires_grad_(True)
    _energy64(verts, idx, w, xc[None], R[:1].double())[0].backward()
    print(f"asymmetric pair {asym}: dE/dx'[{j},{c}] = {g:.6f}, central difference {fd:.6f} (tolerance {tol:.2e}), float64 {float(xc.grad[j, c]):.6f}")
    assert abs(fd - g) <= tol
    assert abs(g - float(xc.grad[j, c])) <= 1e-4 * float(xc.grad.abs().max())


def test_fitted_rotations_are_refused():
    _need_gpu()
    coach, _, _, _, _, xyz, _ = _case()
    x = xyz[0].to(coach.device)
    with pytest.raises(NotImplementedError, match="kNN"):
        coach.compute_arap_energy(x)
    with pytest.raises(NotImplementedError, match="kNN"):
        coach.compute_arap_energy(x, vert_rotations=None)
    with pytest.raises(NotImplementedError, match="kNN"):
        coach.fit_rotations(x)
    with pytest.raises(ValueError):
        from dreammesh4d_amd.mesh_reg import ARAPCoach

        ARAPCoach(torch.rand(8, 3), None, coach.device)                        # 7 other vertices


def test_mesh_coach_beside_it_is_unchanged():
    _need_gpu()
    from dreammesh4d_amd.mesh_reg import ARAPCoach

    _case()
    dev = torch.device("cuda:0")
    g = np.load(GOLD)
    coach = ARAPCoach(g["verts"], g["faces"], dev)
    assert not coach.is_knn and coach.n_faces == len(g["faces"])
    xyz = torch.tensor(g["xyz_prime"], device=dev, requires_grad=True)
    R = torch.tensor(g["rotations"], device=dev, requires_grad=True)
    E = coach.compute_arap_energy(xyz, R)
    assert abs(float(E) - float(g["energy"])) <= 5e-6 * abs(float(g["energy"]))
    E.backward()
    assert np.abs(xyz.grad.cpu().numpy() - g["g_xyz"]).max() <= 2e-5 * np.abs(g["g_xyz"]).max()
    assert np.abs(R.grad.cpu().numpy() - g["g_rot"]).max() <= 2e-5 * np.abs(g["g_rot"]).max()
    assert coach.fit_rotations(xyz.detach()).shape == (len(g["verts"]), 3, 3)
