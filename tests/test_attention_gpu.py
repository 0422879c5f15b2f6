"""csrc/attention.hip (dm4d_attention_f16): the UNet's self-attention on the matrix cores against softmax(q k^T / sqrt(d)) v in
float32 (extern/ldm_zero123/modules/attention.py:152-194), for the head dimensions and token counts of the Zero123 UNet at batch 8
(8 heads of 40 / 80 / 160 channels over 1024 / 256 / 64 tokens) and a few more."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,L,H,D", [(8, 1024, 8, 40), (8, 256, 8, 80), (8, 64, 8, 160), (2, 128, 3, 64), (1, 192, 2, 40), (3, 64, 1, 80)])
def test_attention_matches_float32_reference(B, L, H, D):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from dreammesh4d_amd import conv_mfma

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(L + D)
    qkv = torch.randn(B, L, 3, H, D, generator=g).to(dev).half()
    qkv[:, :, 0] *= 2.0                      # (peaked rows: the running maximum has work to do)
    out = conv_mfma.attention_qkv(qkv)
    q, k, v = (qkv[:, :, i].float().transpose(1, 2) for i in range(3))          # [B, H, L, D]
    ref = torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5, dim=-1) @ v
    ref = ref.transpose(1, 2).reshape(B, L, H * D)
    assert out.shape == ref.shape and out.dtype == torch.float16
    err = float((out.float() - ref).abs().max())
    assert err <= 4e-3 * max(1.0, float(ref.abs().max())), err                 # float16 probabilities and output


def test_attention_rejects_what_it_does_not_take():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from dreammesh4d_amd import conv_mfma

    dev = torch.device("cuda:0")
    with pytest.raises(ValueError):
        conv_mfma.attention_qkv(torch.zeros(1, 64, 3, 2, 48, device=dev, dtype=torch.float16))      # head dimension
    with pytest.raises(ValueError):
        conv_mfma.attention_qkv(torch.zeros(1, 48, 3, 2, 40, device=dev, dtype=torch.float16))      # L % 64


# ----------------------------------------------------------------------------- per-element float64 bar, adversarial rows
# bar (tests/zero123_shadow.py::attention_ref): |o - o_ref| <= 2 (2^-11 sum_j p_ij |v_j| + 2^-11 |o_ref|) + tiny, p in float64

def _check(out, qkv, scale=None, what=""):
    from tests.zero123_shadow import attention_qkv_ref

    ref, bound = attention_qkv_ref(qkv, scale)
    assert out.shape == ref.shape and out.dtype == torch.float16 and bool(torch.isfinite(out).all()), what
    ratio = float(((out.double() - ref).abs() / bound).max())
    assert ratio <= 1.0, (what, ratio)
    return ref


def _rows(case, B, L, H, D, g):
    """qkv [B, L, 3, H, D] float32 for one adversarial case (scores written as the SCALED logits s = q.k / sqrt(D))."""
    r = lambda *s: torch.randn(*s, generator=g)
    qkv = r(B, L, 3, H, D)
    sq = D ** 0.5
    if case == "rising":              # logits rise across the key tiles: the running maximum moves at every tile
        qkv[:, :, 0] = 0.1 * r(B, L, H, D)
        qkv[:, :, 0, :, 0] = 4.0
        qkv[:, :, 1, :, 0] = (torch.arange(L) / 64.0 * 2.5 * sq / 4.0)[None, :, None]
    elif case == "last_tile":         # the only large logit in the LAST key tile (one key per (batch, head))
        qkv[:, :, 0] = 0.2 * r(B, L, H, D)
        qkv[:, :, 0, :, 0] = 4.0
        qkv[:, :, 1, :, 0] = 0.0
        qkv[:, L - 1 - torch.randint(0, 64, (1,), generator=g).item(), 1, :, 0] = 12.0 * sq / 4.0
    elif case == "large":             # scaled scores of about +-60: most float16 probabilities underflow
        qkv[:, :, 0] = r(B, L, H, D)
        qkv[:, :, 1] = r(B, L, H, D)
        s = (qkv[:, :, 0].transpose(1, 2) @ qkv[:, :, 1].transpose(1, 2).transpose(-1, -2)).abs().amax() / sq
        qkv[:, :, 0] *= 60.0 / float(s)
    elif case == "one_hot":           # query i matches key i only: the output is v_i
        u = r(B, L, H, D)
        u = u / u.norm(dim=-1, keepdim=True)
        qkv[:, :, 0], qkv[:, :, 1] = 100.0 * sq * u / 8.0, 8.0 * u
    elif case == "uniform":           # q = 0: every row is the mean of v
        qkv[:, :, 0] = 0.0
    elif case == "big_v":             # |v| in the thousands
        qkv[:, :, 0] *= 2.0
        qkv[:, :, 2] *= 3000.0
    return qkv


CASES = ["random", "rising", "last_tile", "large", "one_hot", "uniform", "big_v", "scale"]


@pytest.mark.parametrize("B", [1, 8, 16])
@pytest.mark.parametrize("L", [64, 128, 192, 256, 1024])
@pytest.mark.parametrize("D", [40, 64, 80, 160])
def test_attention_adversarial_rows_against_float64(D, L, B):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from dreammesh4d_amd import conv_mfma

    dev = torch.device("cuda:0")
    H = 2
    g = torch.Generator().manual_seed(1000 * D + L + B)
    for case in CASES:
        qkv = _rows(case, B, L, H, D, g).to(dev).half()
        scale = 0.37 if case == "scale" else None
        out = conv_mfma.attention_qkv(qkv, scale=scale)
        _check(out, qkv, scale, (case, B, L, D))
        if case == "one_hot":         # that key's v, to within float16
            v = qkv[:, :, 2].reshape(B, L, H * D).double()
            assert float(((out.double() - v).abs() - 2.0 ** -10 * v.abs() - 2.0 ** -24).max()) <= 0.0, (case, B, L, D)
        if case == "uniform":         # the mean of v
            v = qkv[:, :, 2].double().mean(1).reshape(B, 1, H * D)
            vabs = qkv[:, :, 2].double().abs().mean(1).reshape(B, 1, H * D)
            assert float(((out.double() - v).abs() - 2.0 ** -10 * (vabs + v.abs()) - L * 2.0 ** -24).max()) <= 0.0, (case, B, L, D)


@pytest.mark.parametrize("B,L,H,D", [(8, 1024, 8, 40), (8, 256, 8, 80), (8, 64, 8, 160), (2, 192, 3, 64)])
def test_attention_on_the_strided_view_of_the_qkv_gemm(B, L, H, D):
    """qkv exactly as CrossAttention.attend builds it: the [B L, 3 H D] result of the fused projection viewed [B, L, 3, H, D]."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from dreammesh4d_amd import conv_mfma

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B * L + D)
    C = H * D
    x = torch.randn(B, L, C, generator=g).to(dev).half()
    wqkv = (torch.randn(3 * C, C, generator=g) * (2.0 / C ** 0.5)).to(dev).half()
    qkv = torch.nn.functional.linear(x, wqkv).view(B, L, 3, H, -1)
    _check(conv_mfma.attention_qkv(qkv), qkv, None, (B, L, H, D))


@pytest.mark.parametrize("B,L,H,D", [(3, 192, 2, 40), (1, 64, 3, 160), (2, 128, 1, 80), (1, 256, 2, 64)])
def test_attention_writes_only_its_output_and_is_deterministic(B, L, H, D):
    """dm4d_attention_f16 through the C ABI with `out` carved from a larger buffer of sentinels: the bytes before and after stay
    untouched; two runs give bit-identical output."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from dreammesh4d_amd import _lib

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(L + D + H)
    qkv = (torch.randn(B, L, 3, H, D, generator=g) * 1.5).to(dev).half()
    n, pad = B * L * H * D, 4096                            # (pad: a multiple of 8 halves, so `out` stays 16-byte aligned)
    outs = []
    for _ in range(2):
        buf = torch.full((pad + n + pad,), 0x5A5A, dtype=torch.int16, device=dev)
        out = buf[pad:pad + n]
        base = qkv.data_ptr()
        with torch.cuda.device(dev):
            _lib.call("dm4d_attention_f16", B, L, H, D, base, base + H * D * 2, base + 2 * H * D * 2, L * 3 * H * D, 3 * H * D, out.data_ptr(),
                      float(D ** -0.5), torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        assert bool((buf[:pad] == 0x5A5A).all()) and bool((buf[pad + n:] == 0x5A5A).all()), "write outside out"
        outs.append(out.clone())
        _check(out.view(torch.float16).view(B, L, H * D), qkv)
    assert torch.equal(outs[0], outs[1])
