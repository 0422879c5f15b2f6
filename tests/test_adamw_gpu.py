"""-m gpu: the optimiser step of the path in MESSAGE space as two launches (csrc/gradpack.hip, ``dm4d_adamw_message``,
``distributed.ShardedAdamW`` with one process on a HIP device) against ``torch.optim.AdamW`` over ALL elements and against the
torch-operator form of the same class: dense and index-listed parameters (a contiguous and a channels_last plane), two groups with
different learning rates, a step skipped on the device by ``found_inf``, the deferred weight decay of the elements outside the
message applied by ``materialize()``."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _setup(dev, seed):
    g = torch.Generator().manual_seed(seed)
    mlp = torch.nn.Parameter(torch.randn(64, 48, generator=g).to(dev))
    bias = torch.nn.Parameter(torch.randn(48, generator=g).to(dev))
    plane_a = torch.nn.Parameter(torch.randn(1, 16, 24, 20, generator=g).to(dev))
    plane_b = torch.nn.Parameter(torch.randn(1, 16, 12, 10, generator=g).to(dev).contiguous(memory_format=torch.channels_last))
    ia = torch.randperm(plane_a.numel(), generator=g)[:900].sort().values.to(dev)
    ib = torch.randperm(plane_b.numel(), generator=g)[:300].sort().values.to(dev)
    return [mlp, bias, plane_a, plane_b], {plane_a: ia, plane_b: ib}


def _grads(params, touched, step, dev):
    from dreammesh4d_amd.distributed import storage_flat

    g = torch.Generator().manual_seed(1000 + step)
    out = []
    for p in params:
        gr = torch.randn(p.shape, generator=g).to(dev).contiguous(memory_format=torch.channels_last if p.dim() == 4 and not p.is_contiguous() else torch.contiguous_format)
        if p in touched:                     # gradient only where the message has an element (as the HexPlane planes)
            m = torch.zeros(p.numel(), device=dev)
            m[touched[p]] = 1.0
            gr = (storage_flat(gr) * m).view_as(storage_flat(gr)).as_strided(p.shape, p.stride())
        out.append(gr)
    return out


@pytest.mark.parametrize("hyper", ["adamw_defaults", "reference_mix"])
def test_message_space_adamw_equals_the_dense_optimiser(hyper):
    """reference_mix: the first group with the hyperparameters the reference's geometry groups EFFECTIVELY run (betas (0.9, 0.999), no
    decay: distributed.REFERENCE_GEOMETRY_GROUP), the second with its own eps and decay -- per-group in the kernel (dm4d_adamw_step)."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from dreammesh4d_amd import distributed as D

    dev = torch.device("cuda:0")
    runs = {}
    extra = ({}, {}) if hyper == "adamw_defaults" else (dict(D.REFERENCE_GEOMETRY_GROUP), {"weight_decay": 0.03, "eps": 1e-10, "betas": (0.8, 0.95)})
    for mode in ("torch", "ops", "fused"):
        params, touched = _setup(dev, 3)
        groups = [{"params": params[:2], "lr": 3.2e-3, "name": "deformation", **extra[0]}, {"params": params[2:], "lr": 3.2e-2, "name": "grid", **extra[1]}]
        if mode == "torch":
            opt = torch.optim.AdamW(groups, lr=0.0, betas=(0.9, 0.99), eps=1e-15, fused=True)
        else:
            red = D.GradAllReducer(params, touched=touched)
            opt = D.ShardedAdamW(groups, red, betas=(0.9, 0.99), eps=1e-15)
            opt.fused = mode == "fused"
        for step in range(6):
            for p, gr in zip(params, _grads(params, touched, step, dev)):
                p.grad = gr
            flag = torch.tensor(1.0 if step == 2 else 0.0, device=dev)       # step 2 is skipped on the device
            lr_scale = 0.97 ** step                                            # the schedule moves the rates between steps
            for gq, base in zip(opt.param_groups, (3.2e-3, 3.2e-2)):
                gq["lr"] = base * lr_scale
            if mode == "torch":
                opt.found_inf, opt.grad_scale = flag, None
                opt.step()
            else:
                opt.step(found_inf=flag)
        if mode != "torch":
            assert opt.step_t.tolist() == [5.0] * 4               # per segment; the step skipped on the device does not count
            opt.materialize()
        runs[mode] = [p.detach().clone() for p in params]
    for k, (a, b, c) in enumerate(zip(runs["torch"], runs["ops"], runs["fused"])):
        scale = float(a.abs().max())
        assert float((a - c).abs().max()) <= 2e-6 * scale, (k, float((a - c).abs().max()), scale)
        assert float((b - c).abs().max()) <= 2e-6 * scale, (k, float((b - c).abs().max()), scale)
    # the parameters moved (the check above is not comparing initial values), also outside the message (weight decay)
    p0, _ = _setup(dev, 3)
    assert all(float((x - y).abs().max()) > 1e-4 for x, y in zip(p0, runs["fused"]))


def test_optimiser_state_round_trip():
    """state_dict / load_state_dict of the message-space optimiser: a second instance continued from the first one's state takes
    the same steps bit for bit."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from dreammesh4d_amd import distributed as D

    dev = torch.device("cuda:0")
    out = []
    for resume in (False, True):
        params, touched = _setup(dev, 4)
        groups = [{"params": params[:2], "lr": 3.2e-3, "name": "deformation"}, {"params": params[2:], "lr": 3.2e-2, "name": "grid"}]
        opt = D.ShardedAdamW(groups, D.GradAllReducer(params, touched=touched), betas=(0.9, 0.99), eps=1e-15)
        for step in range(4):
            if resume and step == 2:
                sd, vals = opt.state_dict(), [p.detach().clone() for p in params]
                params, touched = _setup(dev, 4)
                with torch.no_grad():
                    for p, v in zip(params, vals):
                        p.copy_(v)
                groups = [{"params": params[:2], "lr": 1.0, "name": "deformation"}, {"params": params[2:], "lr": 1.0, "name": "grid"}]
                opt = D.ShardedAdamW(groups, D.GradAllReducer(params, touched=touched), betas=(0.9, 0.99), eps=1e-15)
                opt.load_state_dict(sd)
            for p, gr in zip(params, _grads(params, touched, step, dev)):
                p.grad = gr
            opt.step()
        opt.materialize()
        out.append([p.detach().clone() for p in params])
    assert all(torch.equal(a, b) for a, b in zip(*out))


def test_segment_without_gradient_is_skipped_like_torch_skips_it():
    """torch.optim leaves a parameter whose .grad is None alone (no decay, no moment decay, its step counter stays); the kernel's
    skip[] does the same per segment -- and the elements of that tensor OUTSIDE the message take no pending decay for that step."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from dreammesh4d_amd import distributed as D

    dev = torch.device("cuda:0")
    runs = {}
    for mode in ("torch", "fused"):
        params, touched = _setup(dev, 6)
        groups = [{"params": params[:2], "lr": 3.2e-3, **D.REFERENCE_GEOMETRY_GROUP}, {"params": params[2:], "lr": 3.2e-2, "weight_decay": 0.05}]
        opt = torch.optim.AdamW(groups, lr=0.0, betas=(0.9, 0.99), eps=1e-15, fused=True) if mode == "torch" else \
            D.ShardedAdamW(groups, D.GradAllReducer(params, touched=touched), betas=(0.9, 0.99), eps=1e-15)
        for step in range(4):
            for k, (p, gr) in enumerate(zip(params, _grads(params, touched, step, dev))):
                p.grad = None if (step == 1 and k in (1, 2)) or (step == 2 and k == 3) else gr
            opt.step()
        if mode == "fused":
            assert opt.step_t.tolist() == [4.0, 3.0, 3.0, 3.0]
            opt.materialize()
        runs[mode] = [p.detach().clone() for p in params]
    for k, (a, c) in enumerate(zip(runs["torch"], runs["fused"])):
        scale = float(a.abs().max())
        assert float((a - c).abs().max()) <= 2e-6 * scale, (k, float((a - c).abs().max()), scale)


def test_abi_of_round_4_still_steps():
    """dm4d_adamw_message (round 4's entry point: one set of hyperparameters, one step counter) is kept for callers built against it."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ctypes as C

    from dreammesh4d_amd import _lib

    dev = torch.device("cuda:0")
    p = torch.randn(1000, device=dev)
    g = torch.randn(1000, device=dev)
    ref = torch.nn.Parameter(p.clone())
    ref.grad = g.clone()
    torch.optim.AdamW([ref], lr=1e-2, betas=(0.9, 0.99), eps=1e-15, weight_decay=0.01).step()
    seg, a = _lib.GradSegments(), _lib.AdamwArgs()
    seg.n_segments, seg.grad[0], seg.index[0], seg.count[0], seg.offset[0] = 1, g.data_ptr(), None, 1000, 0
    m, v = torch.zeros(1000, device=dev), torch.zeros(1000, device=dev)
    st, scr = torch.zeros((), dtype=torch.float64, device=dev), torch.zeros(4, device=dev)
    a.beta1, a.beta2, a.eps, a.weight_decay, a.n_groups = 0.9, 0.99, 1e-15, 0.01, 1
    a.lr[0], a.group[0], a.param[0] = 1e-2, 0, p.data_ptr()
    a.exp_avg, a.exp_avg_sq, a.step, a.pending_decay, a.found_inf, a.scratch = m.data_ptr(), v.data_ptr(), st.data_ptr(), None, None, scr.data_ptr()
    _lib.call("dm4d_adamw_message", C.byref(seg), C.byref(a), 1.0, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert float(st) == 1.0 and float((p - ref.detach()).abs().max()) <= 2e-6 * float(p.abs().max())


def test_slice_form_equals_the_whole_message_step():
    """dm4d_adamw_step's data-parallel SLICE form on one device, without a process group: the message is cut into three slices as three
    ranks would hold them (gradient = the slice of the packed, reduced message: `grad_in_message`; parameters addressed in their storages
    through the index lists; updated values also into the all-gather's send slice: `param_out`), each slice stepped by its own call with
    its own slice of the moments -- parameters, moments and send slices must equal ONE call over the whole message bit for bit, a step
    masked by found_inf must leave everything alone and still fill the send slices."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ctypes as C

    from dreammesh4d_amd import _lib, distributed as D
    from dreammesh4d_amd.distributed import storage_flat

    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    hyper = [(3.2e-3, 0.9, 0.999, 1e-15, 0.0), (3.2e-2, 0.8, 0.95, 1e-10, 0.03)]

    def fill(a, n_seg):
        a.n_groups = 2
        for gi, (lr, b1, b2, eps, wd) in enumerate(hyper):
            a.lr[gi], a.beta1[gi], a.beta2[gi], a.eps[gi], a.weight_decay[gi] = lr, b1, b2, eps, wd
        for k in range(n_seg):
            a.group[k] = 0 if k < 2 else 1

    results = {}
    for mode in ("whole", "slices"):
        params, touched = _setup(dev, 9)
        red = D.GradAllReducer(params, touched=touched)
        n = red.flat.numel()
        W = 3
        chunk = (n + W - 1) // W
        m, v = torch.zeros(chunk * W, device=dev), torch.zeros(chunk * W, device=dev)
        send = torch.full((chunk * W,), float("nan"), device=dev)
        steps = [torch.zeros(len(params), dtype=torch.float64, device=dev) for _ in range(W if mode == "slices" else 1)]
        scal = torch.zeros(1 + 2 * _lib.MAX_GRAD_SEGMENTS, device=dev)
        for it in range(3):
            for p, gr in zip(params, _grads(params, touched, it, dev)):
                p.grad = gr
            red.pack()                                              # the "reduced" message (world 1: the gradients themselves)
            msg = red.flat.clone()
            flag = torch.tensor(1.0 if it == 1 else 0.0, device=dev)
            for r in range(W if mode == "slices" else 1):
                lo, hi = (r * chunk, (r + 1) * chunk) if mode == "slices" else (0, chunk * W)
                seg, a = _lib.GradSegments(), _lib.AdamwStepArgs()
                seg.n_segments = len(params)
                fill(a, len(params))
                for k, (p, o, ix) in enumerate(zip(red.params, red.offsets, red.index)):
                    cnt = p.numel() if ix is None else ix.numel()
                    s0, s1 = max(o, lo), min(o + cnt, hi)
                    base = storage_flat(p.data).data_ptr()
                    if s1 <= s0:
                        seg.count[k], seg.offset[k], seg.grad[k], seg.index[k], a.param[k] = 0, 0, None, None, base
                        continue
                    seg.count[k], seg.offset[k] = s1 - s0, s0 - lo
                    seg.grad[k] = msg.data_ptr() + 4 * s0
                    a.grad_in_message[k] = 1
                    a.param_out[k] = send.data_ptr() + 4 * s0
                    if ix is None:
                        seg.index[k], a.param[k] = None, base + 4 * (s0 - o)
                    else:
                        seg.index[k], a.param[k] = ix.data_ptr() + 8 * (s0 - o), base
                a.exp_avg, a.exp_avg_sq = m.data_ptr() + 4 * lo, v.data_ptr() + 4 * lo
                a.step, a.pending_decay, a.found_inf, a.scratch = steps[r].data_ptr(), None, flag.data_ptr(), scal.data_ptr()
                _lib.call("dm4d_adamw_step", C.byref(seg), C.byref(a), 1.0, st)
            if it == 1:                                             # masked step: the send slices hold the CURRENT parameter values
                cur = D.ShardedAdamW([{"params": params, "lr": 0.0}], red)
                cur._pack_params()
                assert torch.equal(send[:n], cur.padded[:n])
        torch.cuda.synchronize()
        results[mode] = ([p.detach().clone() for p in params], m[:n].clone(), v[:n].clone(), send[:n].clone(), [s.clone() for s in steps])
    (pw, mw, vw, sw, stw), (ps, ms, vs, ss, sts) = results["whole"], results["slices"]
    assert all(torch.equal(a, b) for a, b in zip(pw, ps)) and torch.equal(mw, ms) and torch.equal(vw, vs) and torch.equal(sw, ss)
    assert stw[0].tolist() == [2.0] * 4 and all(s.tolist() == [2.0] * 4 for s in sts)      # the masked step does not count
    assert torch.isfinite(sw).all() and float(mw.abs().max()) > 0
