"""-m gpu: the HIP kernels and the PyTorch-ROCm mirrors against the REFERENCE's golden vectors directly on the
device (tests/golden/*.npz were computed by the reference's own Python in the authoring container,
tests/golden/make_golden.py) -- no intermediate "torch-op path of the same module" in between.

  * HexPlane query + deformation MLP (csrc/hexplane.hip, csrc/deform_mlp.hip) vs deformation_nodes.npz: outputs and
    the gradient of EVERY parameter (custom/threestudio-dreammesh4d/geometry/deformation.py:88-305,430-436).
  * Zero123 UNet / VAE encoder mirror (dreammesh4d_amd/zero123.py) vs zero123_small.npz in fp32 and fp16
    (extern/ldm_zero123/modules/diffusionmodules/openaimodel.py:429-842, model.py Encoder).
Tolerances are written next to each assert."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@pytest.mark.parametrize("layout", ["channels_last", "contiguous"])
def test_hexplane_mlp_hip_vs_reference_golden(layout):
    _need_gpu()
    from dreammesh4d_amd.deformation import DeformationNetwork

    dev = torch.device("cuda:0")
    z = np.load(os.path.join(G, "deformation_small.npz"))
    n = np.load(os.path.join(G, "deformation_nodes.npz"))
    net = DeformationNetwork(net_width=int(z["net_width"]), bounds=float(z["bounds"]), resolution=tuple(z["resolution"]),
                             multires=tuple(z["multires"]), no_ds=False, no_dr=False, no_do=False)
    net.load_state_dict({k[len("state/"):]: torch.tensor(z[k]) for k in z.files if k.startswith("state/")}, strict=True)
    net = net.to(dev)
    if layout == "contiguous":          # the reference's own [1,32,H,W] storage (a loaded reference checkpoint)
        for grid in net.deformation_net.grid.grids:
            for p in grid:
                p.data = p.data.contiguous()
    nodes, ts = torch.tensor(n["nodes"], device=dev), torch.tensor(n["ts"], device=dev)
    out = net.node_outputs(nodes, ts)                          # the fused HIP path (raises without libdm4d_hip.so)
    assert getattr(net, "_hex_plan", None) is not None         # ... and it really was the HIP path
    for name, got in zip(("dx", "dr", "ds", "do"), out):
        err = np.abs(got.detach().cpu().numpy() - n[name]).max()
        assert err < 2e-6, (name, err)                         # absolute; outputs are O(0.1)
    loss = sum((a * torch.tensor(n[f"w{i}"], device=dev).view(a.shape)).sum() for i, a in enumerate(out))
    assert abs(loss.item() - float(n["loss"])) < 2e-5
    loss.backward()
    worst = 0.0
    for k, p in net.named_parameters():
        want = n["grad/" + k]
        got = np.zeros_like(want) if p.grad is None else p.grad.cpu().numpy()
        assert got.shape == want.shape, k
        # per element: |got - want| <= 1e-4 |want| + 2e-6 max|want|  (float32, different summation order)
        bound = 1e-4 * np.abs(want) + 2e-6 * (np.abs(want).max() + 1e-30)
        ratio = float((np.abs(got - want) / bound).max()) if want.size else 0.0
        worst = max(worst, ratio)
        assert ratio <= 1.0, (k, ratio)
        if not np.any(want):
            assert not np.any(got), k                         # the unused timenet etc. receive exact zeros / None
    print(f"HexPlane+MLP ({layout}) vs reference golden: worst gradient error / bound = {worst:.3f}")


def _seeded_fill(module, base, scale=0.05):
    from tests.test_zero123_cpu import seeded_fill

    return seeded_fill(module, base, scale)


@pytest.mark.parametrize("dtype,tol_unet,tol_enc,fast_path", [(torch.float32, 5e-5, 5e-5, False), (torch.float16, 2e-2, 2e-2, False),
                                                             (torch.float16, 2e-2, 2e-2, True)])
def test_zero123_mirror_on_device_vs_reference_golden(dtype, tol_unet, tol_enc, fast_path, monkeypatch):
    """tol = max |y - y_ref| / max |y_ref| (the reference values are fp32 on CPU).  fp32: MIOpen / rocBLAS pick other
    algorithms and summation orders than the CPU; fp16: 10-bit mantissa through ~60 conv / attention layers.

    fast_path: the configuration the guidance step runs -- FROZEN float16 parameters, channels-last -- so that the golden
    vectors of the reference go through the hand-written MFMA convolutions (3x3 stride 1 / stride 2 / narrow), the MFMA linear
    layers (thresholds lowered so that every supported shape takes them) and the fused norms; no convolution may fall back to
    the library (the dispatch counters of zero123._library_fallback).  The 4/8/16-wide attention heads of this reduced model
    are outside csrc/attention.hip's head sizes (40 / 64 / 80 / 160) and stay on the library: tests/test_attention_gpu.py
    and tests/test_zero123_fullsize_gpu.py (the full-size model, every kernel call against float64 at the production
    dispatch) cover that kernel."""
    _need_gpu()
    from dreammesh4d_amd import conv_mfma, fused_norm, zero123 as z

    dev = torch.device("cuda:0")
    g = np.load(os.path.join(G, "zero123_small.npz"))
    if fast_path:
        monkeypatch.setattr(z, "MFMA_LINEAR_MIN_ROWS", 1)
        monkeypatch.setattr(z, "MFMA_LINEAR_RES_MIN_ROWS", 1)
    unet = z.UNetModel(in_channels=8, out_channels=4, model_channels=32, attention_resolutions=(4, 2, 1), num_res_blocks=2,
                       channel_mult=(1, 2, 4, 4), num_heads=8, context_dim=48).eval()
    assert _seeded_fill(unet, base=1000) == g["unet_keys"].tolist()
    unet = unet.to(dev, dtype)
    if fast_path:
        unet = unet.requires_grad_(False).to(memory_format=torch.channels_last)
    before = dict(fused_norm.FALLBACKS)
    flops0 = conv_mfma.FLOPS[0]
    with torch.no_grad():
        y = unet(torch.tensor(g["x"], device=dev, dtype=dtype), torch.tensor(g["t"], device=dev),
                 torch.tensor(g["ctx"], device=dev, dtype=dtype)).float().cpu().numpy()
    e_unet = np.abs(y - g["y"]).max() / np.abs(g["y"]).max()
    enc = z.VaeEncoder(ch=32, ch_mult=(1, 2, 4, 4), num_res_blocks=2, in_channels=3, z_channels=4).eval()
    assert _seeded_fill(enc, base=5000) == g["enc_keys"].tolist()
    enc = enc.to(dev, dtype)
    if fast_path:
        enc = enc.requires_grad_(False).to(memory_format=torch.channels_last)
    with torch.no_grad():
        m = enc(torch.tensor(g["img"], device=dev, dtype=dtype)).float().cpu().numpy()
    e_enc = np.abs(m - g["moments"]).max() / np.abs(g["moments"]).max()
    print(f"Zero123 mirror on device ({dtype}, fast_path={fast_path}): UNet rel err {e_unet:.2e}, VAE encoder rel err {e_enc:.2e}")
    assert np.isfinite(y).all() and np.isfinite(m).all()
    assert e_unet < tol_unet, e_unet
    assert e_enc < tol_enc, e_enc
    if fast_path:
        new = {k: v - before.get(k, 0) for k, v in fused_norm.FALLBACKS.items() if v != before.get(k, 0)}
        assert not new, f"library / torch fallbacks on the fast path: {new}"
        # 2 x (conv flops of the reduced UNet + encoder) must have gone through csrc/conv_mfma.hip: > 0.5 GFLOP here
        assert conv_mfma.FLOPS[0] - flops0 > 5.0e8, conv_mfma.FLOPS[0] - flops0
