"""GPU test of the dynamic-stage iteration driver (dreammesh4d_amd/dynamic_stage.py): the full loop
HexPlane -> skinning -> fused raster -> losses (rgb/mask [+ SDS]) -> backward -> AdamW runs, is finite,
and actually fits reference frames rendered from a known deformation."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _build(dev, with_guidance, with_nc=False, size=128):
    from dreammesh4d_amd import geometry as geo, ops, synthetic as syn, views, zero123 as z
    from dreammesh4d_amd.deformation import DeformationNetwork
    from dreammesh4d_amd.dynamic_stage import DynamicStage

    H = W = size
    M, L = 100, 8
    sc = syn.mesh_bound_scene(2000, n_nodes=M, k=4, seed=0)
    T = lambda a: torch.tensor(a, device=dev)
    graph = ops.DeformGraph(sc["verts"], sc["nbr_idx"], sc["nbr_w"], M, dev)
    topo = ops.MeshTopology(sc["faces"], len(sc["verts"]), 6, dev)
    verts, faces = T(sc["verts"]), T(sc["faces"])
    static = {"q_static": geo.quaternions(verts, faces, T(sc["complex"]), 6),
              "scales": geo.scaling(T(sc["log_scales"]) + 1.0, syn.THICKNESS),      # bigger splats for a 128^2 image
              "opacities": geo.strengths(T(sc["densities"])), "rgb": geo.points_rgb(T(sc["sh_dc"]))}
    cam = syn.make_camera(H, W, elev_deg=5.0, azim_deg=0.0)
    r = views.ViewRenderer(graph, topo, H, W, cam.tanfov, method="hybrid")
    torch.manual_seed(0)
    net = DeformationNetwork(resolution=(16, 16, 16, 8), multires=(1, 2), no_ds=False, no_dr=False, no_do=False).to(dev)
    target = copy.deepcopy(net)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n, p in target.named_parameters():
            if "_deform" in n:
                p.add_((0.08 * torch.randn(p.shape, generator=g)).to(dev))
    ts = torch.linspace(0, 1, L + 2)[1:-1].to(dev)
    nodes = T(sc["nodes"])
    with torch.no_grad():
        dx, dr, ds, do = target.node_outputs(nodes, ts)
        vm, pm = T(cam.viewmatrix)[None].expand(L, 4, 4).contiguous(), T(cam.projmatrix)[None].expand(L, 4, 4).contiguous()
        out = views.render_views(r, dx, dr, ds, do, static["q_static"], static["scales"], static["opacities"],
                                 static["rgb"], vm, pm, torch.ones(6, device=dev))
        ref_img = out["color"][:, :3].clamp(0, 1).permute(0, 2, 3, 1).contiguous()
        ref_mask = out["alpha"].permute(0, 2, 3, 1).contiguous()
    guid = None
    if with_guidance:
        model = z.Zero123(unet_kwargs=dict(model_channels=32, context_dim=32, num_heads=4), vae_kwargs=dict(ch=32))
        for p in model.model.diffusion_model.out.parameters():
            torch.nn.init.normal_(p, std=0.05)
        # fp32 weights: a RANDOM-INIT UNet can overflow fp16 at some timesteps (the real checkpoint does not)
        guid = z.TemporalStableZero123Guidance(model, torch.randn(L, 1, 32), torch.randn(L, 4, 32, 32),
                                               cond_elevation_deg=5.0, half_precision_weights=False).to(dev)
    from dreammesh4d_amd.mesh_reg import ARAPCoach, MeshNormalConsistency

    stage = DynamicStage(r, net, nodes, static, ts, ref_img, ref_mask, cam, guidance=guid, frames_per_step=4,
                         random_views_per_frame=1, deformation_lr=2e-3, grid_lr=2e-2,
                         normal_consistency=MeshNormalConsistency(sc["faces"], len(sc["verts"]), dev) if with_nc else None,
                         arap=ARAPCoach(sc["verts"], sc["faces"], dev) if with_nc else None, milestone_arap_reg=1,
                         inter_frame_reg=1)
    return stage


def test_iteration_fits_reference_frames():
    _need_gpu()
    stage = _build(torch.device("cuda:0"), with_guidance=False)
    losses = [float(stage.iteration()["rgb"]) for _ in range(40)]
    assert np.isfinite(losses).all()
    # AdamW with eps 1e-15 is sign-like, so the trajectory is sensitive to rounding: only require a clear decrease
    assert np.mean(losses[-8:]) < 0.8 * np.mean(losses[:8]), losses
    stage.r.check()
    assert stage.global_step == 40
    assert {g["name"] for g in stage.opt.param_groups} == {"deformation", "grid"}
    # the reference's EFFECTIVE hyperparameters of these two groups (training_setup_dynamic's Adam fills the dicts in place)
    assert all(tuple(g["betas"]) == (0.9, 0.999) and g["weight_decay"] == 0.0 and g["eps"] == 1e-15 for g in stage.opt.param_groups)
    assert all(tuple(g["betas"]) == (0.9, 0.999) and g["weight_decay"] == 0.0 for g in stage.sharded.param_groups)


def test_iteration_with_zero123_sds_runs_and_updates_the_network():
    _need_gpu()
    stage = _build(torch.device("cuda:0"), with_guidance=True, with_nc=True)
    before = [p.detach().clone() for p in stage.net.get_mlp_parameters()]
    out = stage.iteration()
    assert {"rgb", "mask", "sds", "normal_consistency", "loss"} <= set(out) and all(torch.isfinite(v) for v in out.values())
    assert 0.0 <= float(out["normal_consistency"]) < 0.2      # a smooth sphere: neighbouring faces are nearly coplanar
    assert "arap_reg_key_frame" not in out                    # before milestone_arap_reg
    # the heads are zero-initialised (deformation.py:507-512), so the grids only get gradient from step 2 on
    out = stage.iteration()
    assert all(torch.isfinite(v) for v in out.values())
    assert {"arap_reg_key_frame", "arap_reg_inter_frame"} <= set(out) and float(out["arap_reg_key_frame"]) >= 0.0
    grid_grad = [p.grad for p in stage.net.get_grid_parameters() if p.requires_grad]   # aabb is frozen
    assert all(g is not None and torch.isfinite(g).all() for g in grid_grad) and any(g.abs().sum() > 0 for g in grid_grad)
    after = stage.net.get_mlp_parameters()
    assert any(not torch.equal(a, b) for a, b in zip(after, before))
    assert stage.guidance.max_step == 500 and stage.guidance.min_step == 20      # yaml:118-119 (0.02 / 0.5)


def test_optional_loss_terms_with_a_weight_run_instead_of_raising():
    """system/sugar_4dgen.py:181-207,236-300: the terms whose weight is 0 in the shipped YAML (depth, depth_rel, normal, normal_smooth, rgb / depth /
    normal TV, normal-depth consistency, ref_xyz, obj_centric, laplacian_smoothing).  Round 4's from_cfg raised NotImplementedError for any
    of them; now they are computed (the reference's torch expressions on renderer.compose_outputs' images), once per substep where the
    reference does so, and the renderer stops skipping the normal pass's backward when one of them reads comp_normal."""
    _need_gpu()
    from dreammesh4d_amd import synthetic as syn
    from dreammesh4d_amd.dynamic_stage import DynamicStage, OPTIONAL_TERMS
    from dreammesh4d_amd.mesh_reg import MeshLaplacianSmoothing

    dev = torch.device("cuda:0")
    base = _build(dev, with_guidance=False)
    assert base.r.rgb_gradient_only                     # shipped weights: nothing reads the normal image
    L, H, W = int(base.timestamps.shape[0]), base.r.H, base.r.W
    g = torch.Generator().manual_seed(0)
    sc = syn.mesh_bound_scene(2000, n_nodes=100, k=4, seed=0)
    loss_cfg = {"lambda_rgb": 5000.0, "lambda_mask": 500.0, "lambda_sds_zero123": 0.0, "lambda_depth": 1.0, "lambda_depth_rel": 0.5, "lambda_normal": 0.3,
                "lambda_normal_smooth": 0.2, "lambda_rgb_tv": 1.0, "lambda_depth_tv": 1.0, "lambda_normal_tv": [0, 0.5, 1.0, 100],
                "lambda_normal_depth_consistency": 0.1, "lambda_ref_xyz": 2.0, "lambda_obj_centric": 1.0, "lambda_laplacian_smoothing": 1.0,
                "lambda_normal_consistency": 0.0, "lambda_arap_reg_key_frame": 0.0, "lambda_arap_reg_inter_frame": 0.0, "lambda_3d_normal_smooth": 0.0}
    with pytest.raises(ValueError):                      # lambda_depth without ref_depths
        DynamicStage.from_cfg({"loss": loss_cfg}, base.r, base.net, base.nodes, base.static, base.timestamps, base.ref_images, base.ref_masks, base.ref_camera)
    stage = DynamicStage.from_cfg({"loss": loss_cfg}, base.r, base.net, base.nodes, base.static, base.timestamps, base.ref_images, base.ref_masks,
                                  base.ref_camera, ref_depths=torch.rand(L, H, W, 1, generator=g) + 3.0, ref_normals=torch.rand(L, H, W, 3, generator=g),
                                  laplacian_smoothing=MeshLaplacianSmoothing(sc["faces"], len(sc["verts"]), dev), random_views_per_frame=1)
    assert not stage.r.rgb_gradient_only                # lambda_normal* set: the normal pass's backward is needed again
    out = stage.iteration()
    want = {f"{k}/ref" for k in OPTIONAL_TERMS} | {f"{k}/zero123" for k in ("normal_smooth", "rgb_tv", "depth_tv", "normal_tv", "normal_depth_consistency", "obj_centric")}
    assert want <= set(out), sorted(want - set(out))
    assert all(torch.isfinite(v) for v in out.values())
    assert 0.0 <= float(out["depth_rel/ref"]) <= 2.0 and 0.0 <= float(out["normal/ref"]) <= 2.0 and float(out["rgb_tv/ref"]) > 0
    grads = [p.grad for p in stage.net.get_mlp_parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(x).all() for x in grads)
    with pytest.raises(NotImplementedError):             # a name the reference does not have is still refused
        DynamicStage.from_cfg({"loss": {"lambda_made_up": 1.0}}, base.r, base.net, base.nodes, base.static, base.timestamps, base.ref_images,
                              base.ref_masks, base.ref_camera)


def test_checkpoint_resume_continues_the_optimiser(tmp_path):
    """the optimiser that STEPS on a HIP device is the message-space one; `stage.opt` (what a host would save by default)
    never steps.  save_checkpoint(..., optimizer_states=[stage.optimizer_state_dict()]) + load into a freshly built stage: the third
    iteration of the resumed run is bit-identical to the uninterrupted run's (moments, per-segment step counters = bias corrections,
    iteration count = schedules, sampler state); without the optimiser state it is not."""
    _need_gpu()
    from dreammesh4d_amd import wire_formats as wf

    dev = torch.device("cuda:0")
    a = _build(dev, with_guidance=False)
    assert a.sharded is not None and len(a.opt.state_dict()["state"]) == 0
    for _ in range(3):
        a.iteration()
    want = [p.detach().clone() for p in a.net.parameters()]
    b = _build(dev, with_guidance=False)
    for _ in range(2):
        b.iteration()
    b.state_for_checkpoint()
    path = str(tmp_path / "dyn.ckpt")
    wf.save_checkpoint(path, {"geometry._deformation": b.net}, global_step=b.global_step, optimizer_states=[b.optimizer_state_dict()])
    assert len(b.opt.state_dict()["state"]) == 0          # the torch optimiser indeed holds nothing
    got = {}
    for with_state in (True, False):
        c = _build(dev, with_guidance=False)
        sd, _, step = wf.load_module_weights(path, module_name="geometry._deformation")
        c.net.load_state_dict(sd, strict=True)
        if with_state:
            (osd,) = wf.load_optimizer_states(path)
            c.load_optimizer_state_dict(osd)
            assert c.global_step == 2 and c.sharded.step_t.tolist() == b.sharded.step_t.tolist()
        else:
            c.global_step = step
            c.gen.set_state(b.gen.get_state())
        c.iteration()
        got[with_state] = [p.detach().clone() for p in c.net.parameters()]
    assert all(torch.equal(x, y) for x, y in zip(want, got[True]))
    assert not all(torch.equal(x, y) for x, y in zip(want, got[False]))
    with pytest.raises(ValueError):
        c.load_optimizer_state_dict({"kind": "torch.optim.AdamW", "state": {}})


def _torchrun(args, env=None, timeout=600, nproc=2):
    import os, socket, subprocess, sys

    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **(env or {}))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(port)] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=e, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.mark.parametrize("mode", ["replicated", "sharded", "compare"])
def test_two_rank_rehearsal_replicas_stay_identical(mode):
    """The N > 1 control flow end to end with 2 ranks sharing the one GPU of the box over gloo: frames sharded, the
    structured-sparse gradient exchange, AdamW (replicated after an all-reduce, or sharded: reduce-scatter -> AdamW on the
    slice -> all-gather): bit-identical parameters on both ranks after 2 iterations.  compare: 3 iterations through both
    optimisers from the same seeds -- the sharded one (created in the constructor, moments never reset, overflow flag
    honoured, untouched texels decayed lazily) reproduces the replicated parameters to float32 rounding."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    r = _torchrun(["tests/dp_rehearsal_worker.py", mode])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert f"DP_REHEARSAL_OK mode={mode} world=2" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("mode", ["replicated", "compare"])
def test_eight_rank_rehearsal_of_cfg4_partition(mode):
    """BASELINE configs[3]'s exact partition with 8 ranks sharing the one GPU of the box over gloo (no 8-GPU node has been
    available to any round): 32 frames, rank r owns frames 4r .. 4r + 3 (data/temporal_image.py:292-322),
    ONE structured-sparse message per iteration, replicas bit-identical on all 8 ranks after 2 iterations (replicated AdamW
    after the all-reduce); compare: 3 iterations through the replicated and the sharded optimiser (reduce-scatter -> AdamW on
    1/8 of the message -> all-gather) agree to float32 rounding.  A control-flow rehearsal, never a performance number."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    r = _torchrun(["tests/dp_rehearsal_worker.py", mode], env={"DM4D_REHEARSAL_FRAMES": "32", "OMP_NUM_THREADS": "4"}, nproc=8, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert f"DP_REHEARSAL_OK mode={mode} world=8" in r.stdout, r.stdout[-2000:]


def test_bench_rehearsal_two_ranks_over_gloo():
    """bench.py's own N = 2 launch line (torch.distributed.run, one rank per GPU) in its rehearsal mode."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import json

    r = _torchrun(["bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-iters"], env={"DM4D_BENCH_BACKEND": "gloo"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["steps"] == 2 and "REHEARSAL" in line["data"]
    assert line["config"]["allreduce_bytes_per_step"] == line["config"]["allreduce_message_bytes"] < line["config"]["dense_gradient_bytes"] / 5


def test_bench_spawns_its_own_ranks_from_gpus_flag():
    """`python bench.py --gpus 2 ...` with NO launcher in the command (the driver's command shape): bench.py starts the two
    ranks itself (reference: launch.py:114,166,228-235 -- the launcher owns the per-GPU processes) and rank 0's line says
    n_gpus = 2.  Rehearsal mode (gloo, ranks share the one GPU); with the RCCL backend and fewer devices than ranks it
    refuses loudly instead of rendering on one GPU and printing n_gpus = 1 (round 4's behaviour)."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import json, os, subprocess, sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-iters"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(env, DM4D_BENCH_BACKEND="gloo"), cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and "REHEARSAL" in line["data"]
    if torch.cuda.device_count() < 2:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=root)
        assert r.returncode != 0 and "HIP device" in (r.stdout + r.stderr)


@pytest.mark.parametrize("H,W,C", [(512, 512, 6), (64, 96, 3)])
def test_image_head_equals_the_torch_composition(H, W, C):
    """image_head (csrc/imagehead.hip) against what it replaces in DynamicStage.iteration: clamp(render, 0, 1); MSE against the
    reference images / masks on the reference views (system/sugar_4dgen.py:164-172); the random views resized to half the size with
    bilinear interpolation (the guidance's first step at 512 x 512) -- values, and the gradients on the renderer's colour and alpha
    images including torch.clamp's pass-through at the bounds (pixels at exactly 0 and 1 are in the data).  Full size and wiring;
    the edges (ragged tails, the workgroup cap, view roles, null pointers, the neighbours of 0 and 1) are in
    tests/test_dynamic_glue_edges_gpu.py."""
    _need_gpu()
    import torch.nn.functional as F

    from dreammesh4d_amd.image_head import image_head

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(H + C)
    B, L = 6, 5
    color = (torch.rand(B, C, H, W, generator=g) * 1.6 - 0.3)
    color[:, :, ::7, ::5] = 0.0
    color[:, :, 3::11, 1::4] = 1.0
    alpha = torch.rand(B, 1, H, W, generator=g)
    color, alpha = color.to(dev).requires_grad_(True), alpha.to(dev).requires_grad_(True)
    ref_images, ref_masks = torch.rand(L, H, W, 3, generator=g).to(dev), (torch.rand(L, H, W, 1, generator=g) > 0.5).float().to(dev)
    ref_idx, rnd_idx = [0, 3, 4], [1, 2, 5]
    fidx_ref = torch.tensor([4, 0, 2], device=dev)
    ref_pos = torch.tensor([0, -1, -1, 1, 2, -1], dtype=torch.int32, device=dev)
    rnd_pos = torch.tensor([-1, 0, 1, -1, -1, 2], dtype=torch.int32, device=dev)
    w_rgb, w_mask = 3.0, 0.7
    gh = torch.randn(3, H // 2, W // 2, 3, generator=g).to(dev)
    # the operator
    m_rgb, m_mask, half = image_head(color, alpha, ref_pos, rnd_pos, ref_images, ref_masks, fidx_ref, 3, 3)
    (w_rgb * m_rgb + w_mask * m_mask + (half * gh).sum()).backward()
    got = (m_rgb.detach(), m_mask.detach(), half.detach(), color.grad.clone(), alpha.grad.clone())
    color.grad = alpha.grad = None
    # the composition
    rgb = color[:, :3].clamp(0, 1).permute(0, 2, 3, 1)
    mask = alpha.permute(0, 2, 3, 1)
    ri, ni = torch.tensor(ref_idx, device=dev), torch.tensor(rnd_idx, device=dev)
    r_rgb = F.mse_loss(ref_images.index_select(0, fidx_ref), rgb.index_select(0, ri))
    r_mask = F.mse_loss(mask.index_select(0, ri), ref_masks.index_select(0, fidx_ref))
    r_half = F.interpolate(rgb.index_select(0, ni).permute(0, 3, 1, 2), (H // 2, W // 2), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    (w_rgb * r_rgb + w_mask * r_mask + (r_half * gh).sum()).backward()
    assert abs(float(got[0]) - float(r_rgb)) <= 2e-6 * float(r_rgb) and abs(float(got[1]) - float(r_mask)) <= 2e-6 * float(r_mask)
    assert got[2].shape == r_half.shape and float((got[2] - r_half).abs().max()) <= 1e-7
    assert float((got[3] - color.grad).abs().max()) <= 1e-6 * float(color.grad.abs().max())
    assert float((got[4] - alpha.grad).abs().max()) <= 1e-6 * float(alpha.grad.abs().max())
    if C > 3:
        assert float(got[3][:, 3:].abs().max()) == 0.0


def test_iteration_with_the_fused_image_head_equals_the_torch_composition():
    """At the shipped 512 x 512 DynamicStage.iteration takes the fused image head: the same loss terms and the same parameter
    update as the torch composition it replaces (same seeds, two copies of the stage)."""
    _need_gpu()
    dev = torch.device("cuda:0")
    res = {}
    for fused in (True, False):
        torch.manual_seed(0)
        stage = _build(dev, with_guidance=False, size=512)
        stage.fused_image_head = fused
        out = [stage.iteration() for _ in range(2)]
        torch.cuda.synchronize()
        res[fused] = ([{k: float(v) for k, v in o.items() if torch.is_tensor(v)} for o in out],
                      torch.cat([p.detach().flatten() for p in stage.net.get_mlp_parameters()]).clone())
    for a, b in zip(res[True][0], res[False][0]):
        assert a.keys() == b.keys()
        for k in a:
            assert abs(a[k] - b[k]) <= 2e-5 * abs(b[k]) + 1e-9, (k, a[k], b[k])
    assert float((res[True][1] - res[False][1]).abs().max()) <= 2e-4 * float(res[False][1].abs().max())
