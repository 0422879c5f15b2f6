"""GPU tests of the fitted-rotation ARAP path: csrc/meshreg.hip::k_arap_fit through ARAPCoach.fit_rotations and
ARAPCoach.compute_arap_energy(xyz_prime) (the reference's default vert_rotations=None), against the reference's own class
(tests/golden/arap_fit.npz) and against its float64 restatement (tests/arap_fit_common.py, pinned to that fixture on the CPU).

The bar on R itself: err = max_i max|R_hip,i - R_f64,i| gap_i may be R_BAR_FACTOR = 4 times the same quantity of the reference's
float32 path on the CPU (torch.svd in float32 on the same inputs), computed in the test from that CPU fit.  No vertex is excluded.
Measured on MI355X, err_hip / err_cpu32 (max|dR| hip / cpu32):
  fixture  mid 0.093 (9.4e-8 / 6.7e-7)  noisy 0.40 (3.4e-7 / 7.6e-7)  rigid 0.19 (4.3e-8 / 8.0e-7)  smooth 0.11 (4.5e-8 / 8.7e-7)
           yz: R = I exactly on both
  sphere   noise 0.002: 0.12 (3.0e-8 / 1.6e-5)   0.02: 0.086 (3.0e-8 / 8.4e-6)   0.1: 0.057 (3.0e-8 / 1.3e-5)
(the kernel fits in double: against the float64 restatement on the same float32 inputs its R differs by the final rounding to
float32; on the fixture the rest is the product's float32 cotangent weights against the reference's float64 ones).
Determinant-flip flags on the sphere: 441 / 1396 / 1514 of 3002 vertices flip (15 % / 46 % / 50 %); flag and restatement disagree
at 0 vertices, also among the 995 / 503 / 341 with sig3 / sig1 <= 1e-3.  Energy on the fixture: 2e-8 ... 1e-7 relative (bar 5e-6),
gradient 4e-8 ... 7e-7 of its maximum (bar 2e-5); on the sphere 7e-8 and 6e-8 (bars 1e-4).  Rigid motion: |R - Q| 2.7e-7 (bar
1.6e-5), E 4.9e-13 (bar 1.7e-9).  Minimality: fitted 0.2477 against skinned 0.4480 per timestamp."""
import numpy as np
import pytest
import torch

from dreammesh4d_amd import synthetic as syn
from tests import arap_fit_common as afc

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _coach_edges(coach):
    """The float32 adjacency the kernels read, on the CPU."""
    return (torch.as_tensor(coach.edge_sources), torch.as_tensor(coach.edge_targets), torch.as_tensor(coach.edge_weights),
            coach._e.cpu())


def _assert_rotations(tag, R_hip, flags, x32, edges, R64, sig64, flip64):
    """R against the float64 yardstick under the bar of the module docstring (every vertex counts), the flag bytes against the
    yardstick's branches, orthogonality and orientation of every R.  Returns the share of flipped vertices per flag."""
    src, nbr, w32, e32 = edges
    gap = afc.gap(sig64, flip64)
    R32, _, _, unchanged32 = afc.fit(src, nbr, w32, e32, x32)                  # the reference's float32 path on the CPU
    err_cpu, d_cpu = afc.r_error(R32, R64, gap)
    err_hip, d_hip = afc.r_error(R_hip, R64, gap)
    unchanged64 = sig64[:, 0] == 0
    hip_unchanged, hip_flip = (flags & 1).bool(), (flags & 2).bool()
    decided = (sig64[:, 2] > afc.SIGN_RATIO * sig64[:, 0]) & ~unchanged64
    wrong = int((hip_flip != flip64)[decided].sum())
    wrong_below = int((hip_flip != flip64)[~decided & ~unchanged64].sum())
    orth, det_min = afc.orthogonality(R_hip)
    print(f"{tag}: err_hip {err_hip:.3e} err_cpu32 {err_cpu:.3e} ratio {err_hip / err_cpu if err_cpu else 0.0:.3f} | max|dR| hip {d_hip:.3e} "
          f"cpu32 {d_cpu:.3e} | min gap {float(gap[~unchanged64].min()) if (~unchanged64).any() else float('nan'):.3e} | flipped "
          f"hip {int(hip_flip.sum())} f64 {int(flip64.sum())} of {len(gap)}, disagree {wrong} decided + {wrong_below} of "
          f"{int((~decided & ~unchanged64).sum())} with sig3/sig1 <= {afc.SIGN_RATIO} | unchanged hip {int(hip_unchanged.sum())} "
          f"f64 {int(unchanged64.sum())} | |RtR - I| {orth:.2e} det min {det_min:.7f}")
    assert torch.equal(hip_unchanged, unchanged64) and torch.equal(unchanged32, unchanged64)
    assert wrong == 0
    assert err_hip <= afc.R_BAR_FACTOR * err_cpu
    assert orth <= 1e-5 and det_min > 0
    return float(hip_flip.float().mean())


def test_fixture_parity_through_the_coach():
    """(d) every fixture case through ARAPCoach with the reference's default argument: R under the 4x-CPU-float32 bar, flags, the
    energy to 5e-6 relative and the gradient to 2e-5 of its maximum (the bars of the explicit-rotation test beside this one).  The
    rigid case's reference energy is rounding noise (3.5e-13) and has no relative bar: see test_rigid_motion."""
    _need_gpu()
    from dreammesh4d_amd.mesh_reg import ARAPCoach

    dev = torch.device("cuda:0")
    fx = afc.load()
    coach = ARAPCoach(fx["verts"], fx["faces"], dev)
    edges = _coach_edges(coach)
    for name in fx["cases"]:
        x32 = torch.tensor(fx[f"{name}_xyz_prime"]).float()
        xg = x32.to(dev).requires_grad_(True)
        R, flags = coach.fit_rotations(xg, return_flags=True)
        assert R.shape == (len(x32), 3, 3) and R.dtype == torch.float32 and not R.requires_grad and flags.dtype == torch.uint8
        _assert_rotations(f"fixture {name}", R.cpu(), flags.cpu(), x32, edges, torch.tensor(fx[f"{name}_R"]),
                          torch.tensor(fx[f"{name}_sig"]), torch.tensor(fx[f"{name}_flip"]))
        if name == "yz":
            assert torch.equal(R.cpu(), torch.eye(3).expand(len(x32), 3, 3)) and bool((flags == ARAPCoach.FLAG_UNCHANGED).all())
        E = coach.compute_arap_energy(xg)
        E.backward()
        Ew, gw = float(fx[f"{name}_energy"]), fx[f"{name}_g_xyz"]
        dg = float(np.abs(xg.grad.cpu().numpy() - gw).max())
        print(f"fixture {name}: E {float(E):.9g} ref {Ew:.9g} rel {abs(float(E) - Ew) / abs(Ew):.2e} | |dg| {dg:.2e} of {np.abs(gw).max():.2e}")
        if name != "rigid":
            assert abs(float(E) - Ew) <= 5e-6 * abs(Ew)
            assert dg <= 2e-5 * np.abs(gw).max()


def _sphere_case(dev):
    from dreammesh4d_amd.mesh_reg import ARAPCoach
    from oracle import mesh_reg as M

    verts, faces = syn.uv_sphere(6000, radius=0.6)
    coach = ARAPCoach(verts, faces, dev)
    adj = M.build(verts, faces)
    assert np.allclose(coach.edge_weights, adj["w"], rtol=1e-6, atol=1e-7) and np.array_equal(coach.edge_targets, adj["nbr"])
    gen = torch.Generator().manual_seed(4)
    x0 = torch.tensor(np.asarray(verts, np.float64))
    A = torch.eye(3, dtype=torch.float64) + 0.2 * torch.randn(3, 3, generator=gen, dtype=torch.float64)
    x = torch.stack([x0 @ A.T + noise * torch.randn(len(x0), 3, generator=gen, dtype=torch.float64) for noise in (0.002, 0.02, 0.1)])
    return coach, x.float()


def test_batched_fit_on_a_large_mesh_against_the_float64_restatement():
    """(e) uv_sphere(6000) (3002 vertices, two high-valence poles), T = 3 in one launch, x A^T + noise of 0.002 / 0.02 / 0.1.
    Branch coverage is a condition: per input at least 10 % of the vertices take the determinant flip and 10 % do not, by the
    flag byte and by the restatement, and the two agree wherever sig3 / sig1 > 1e-3.  R under the 4x bar with no vertex excluded;
    energy and gradient to 1e-4 of their maxima."""
    _need_gpu()
    dev = torch.device("cuda:0")
    coach, x32 = _sphere_case(dev)
    src, nbr, w32, e32 = edges = _coach_edges(coach)
    T, V = x32.shape[:2]
    R, flags = coach.fit_rotations(x32.to(dev), return_flags=True)
    assert R.shape == (T, V, 3, 3) and flags.shape == (T, V)
    wts = torch.tensor([1.0, -0.5, 2.0])
    x64 = x32.double().requires_grad_(True)
    E64 = []
    for t in range(T):
        R64, sig, flip, _ = afc.fit(src, nbr, w32.double(), e32.double(), x64[t])
        share = _assert_rotations(f"sphere t={t}", R[t].cpu(), flags[t].cpu(), x32[t], edges, R64.detach(), sig, flip)
        assert 0.1 <= share <= 0.9 and 0.1 <= float(flip.float().mean()) <= 0.9
        E64.append(afc.energy(src, nbr, w32.double(), e32.double(), x64[t], R64))
    E64 = torch.stack(E64)
    (E64 * wts.double()).sum().backward()
    xg = x32.to(dev).requires_grad_(True)
    Eh = coach.compute_arap_energy(xg)
    (Eh * wts.to(dev)).sum().backward()
    dE, dg = float((Eh.cpu().double() - E64.detach()).abs().max()), float((xg.grad.cpu().double() - x64.grad).abs().max())
    print(f"sphere: |dE| {dE:.3e} of {float(E64.detach().abs().max()):.3e} | |dg| {dg:.3e} of {float(x64.grad.abs().max()):.3e}")
    assert Eh.shape == (T,)
    assert dE <= 1e-4 * float(E64.detach().abs().max())
    assert dg <= 1e-4 * float(x64.grad.abs().max())


def test_default_argument_is_fit_then_the_explicit_path_bit_for_bit():
    """(f) compute_arap_energy(x) == compute_arap_energy(x, fit_rotations(x)) bitwise, twice in a row (determinism), and so is the
    gradient to x; the rotations are constants of the graph.  A single [V,3] mesh is the T = 1 batch."""
    _need_gpu()
    dev = torch.device("cuda:0")
    coach, x32 = _sphere_case(dev)
    wts = torch.tensor([1.0, -0.5, 2.0], device=dev)
    runs = []
    for explicit in (False, True, False, True):
        xg = x32.to(dev).requires_grad_(True)
        R = coach.fit_rotations(xg)
        E = coach.compute_arap_energy(xg, R) if explicit else coach.compute_arap_energy(xg)
        (E * wts).sum().backward()
        runs.append((E.detach(), xg.grad, R))
    for E, g, R in runs[1:]:
        assert torch.equal(E, runs[0][0]) and torch.equal(g, runs[0][1]) and torch.equal(R, runs[0][2])
    x1 = x32[1].to(dev).requires_grad_(True)
    E1 = coach.compute_arap_energy(x1)
    E1.backward()
    assert E1.dim() == 0 and torch.equal(E1.detach(), coach.compute_arap_energy(x1.detach(), coach.fit_rotations(x1)))
    assert abs(float(E1) - float(runs[0][0][1])) <= 1e-6 * float(runs[0][0][1])     # (torch sums the rows of [1,V] and [3,V] in its own order)
    assert torch.equal(coach.fit_rotations(x1), runs[0][2][1])
    assert torch.equal(x1.grad * wts[1], runs[0][1][1])                   # (-0.5: a power of two, the scaling is exact)


def test_rigid_motion():
    """(g) x' = Q x + c: every vertex gets Q, and the energy is zero up to float32 rounding.  Bars from the number format: the
    inputs x' are rounded to float32, which moves an edge by up to eps32 max|x'| per component, ~8 eps32 relative to the shortest
    edges of this mesh, and R answers a relative perturbation of S with that over the gap: |R - Q| <= 16 eps32 / min gap.  A
    residual component is then at most ~8 eps32 max|x'|, so |E| <= sum |w| 3 (8 eps32 max|x'|)^2."""
    _need_gpu()
    from dreammesh4d_amd.mesh_reg import ARAPCoach

    dev = torch.device("cuda:0")
    fx = afc.load()
    coach = ARAPCoach(fx["verts"], fx["faces"], dev)
    x = torch.tensor(fx["rigid_xyz_prime"]).float().to(dev)
    R = coach.fit_rotations(x)
    gap_min = float(afc.gap(torch.tensor(fx["rigid_sig"]), torch.tensor(fx["rigid_flip"])).min())
    dQ = float((R.cpu().double() - torch.tensor(fx["rigid_Q"])).abs().max())
    E = float(coach.compute_arap_energy(x))
    E_bar = float(np.abs(coach.edge_weights).sum()) * 3.0 * (8.0 * afc.EPS32 * float(x.abs().max())) ** 2
    print(f"rigid: |R - Q| {dQ:.3e} (bar {16 * afc.EPS32 / gap_min:.3e}, min gap {gap_min:.3e}) | E {E:.3e} (bar {E_bar:.3e})")
    assert dQ <= 16 * afc.EPS32 / gap_min
    assert abs(E) <= E_bar                                 # (cotangent weights can be negative: so can a rounding-noise energy)


def test_fitted_rotations_do_not_cost_more_than_the_skinned_ones():
    """(h) minimality: on the perturbed scene of tests/test_mesh_reg_gpu.py::test_arap_through_the_geometry_accessors the energy
    under the fitted rotations is at most (1 + 1e-5) times the energy under the skinned rotations, per timestamp; no vertex is
    flagged unchanged there.  (i) every fitted R is orthogonal to 1e-5 with det > 0."""
    _need_gpu()
    from dreammesh4d_amd import sugar
    from dreammesh4d_amd.mesh_reg import ARAPCoach

    dev = torch.device("cuda:0")
    sc = syn.mesh_bound_scene(1200, n_nodes=60, k=4, seed=2)
    geo = sugar.DynamicSuGaR(sc["verts"], sc["faces"], sc["nodes"], sc["nbr_idx"], sc["nbr_w"],
                             deformation_kwargs=dict(resolution=(16, 16, 16, 9), multires=(1, 2)), device=dev)
    coach = ARAPCoach(geo.get_xyz_verts, geo.get_faces, dev)
    ts = torch.tensor([0.25, 0.6], device=dev)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for n, p in geo._deformation.named_parameters():
            if "_deform" in n:
                p.add_((0.05 * torch.randn(p.shape, generator=g)).to(dev))
        xyz = geo.get_timed_vertex_xyz(ts)
        E_skin = coach.compute_arap_energy(xyz, geo.get_timed_vertex_rotation(ts, return_matrix=True))
        R, flags = coach.fit_rotations(xyz, return_flags=True)
        E_fit = coach.compute_arap_energy(xyz)
    orth, det_min = afc.orthogonality(R.cpu())
    print(f"skinned {E_skin.tolist()} fitted {E_fit.tolist()} | unchanged {int((flags & 1).sum())} flipped {int(((flags & 2) > 0).sum())} "
          f"of {flags.numel()} | |RtR - I| {orth:.2e} det min {det_min:.7f}")
    assert float(E_skin.sum()) > 1e-4 and int((flags & 1).sum()) == 0
    assert bool((E_fit <= (1 + 1e-5) * E_skin).all())
    assert orth <= 1e-5 and det_min > 0


def test_every_fitted_rotation_is_a_proper_rotation():
    """(i) |R^T R - I| <= 1e-5 and det > 0 for every vertex of the large-mesh inputs, and for a mesh whose vertices did not move
    at all (every vertex unchanged: identities)."""
    _need_gpu()
    dev = torch.device("cuda:0")
    coach, x32 = _sphere_case(dev)
    orth, det_min = afc.orthogonality(coach.fit_rotations(x32.to(dev)).cpu())
    print(f"sphere: |RtR - I| {orth:.2e} det min {det_min:.7f}")
    assert orth <= 1e-5 and det_min > 0
    R, flags = coach.fit_rotations(coach.verts, return_flags=True)
    assert torch.equal(R.cpu(), torch.eye(3).expand(coach.n_verts, 3, 3)) and bool((flags == 1).all())
    assert float(coach.compute_arap_energy(coach.verts)) == 0.0
