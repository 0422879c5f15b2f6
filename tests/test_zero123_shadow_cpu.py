"""The shadow harness of tests/test_zero123_fullsize_gpu.py (tests/zero123_shadow.py) on the CPU: a fake "kernel" that returns
the float64 reference plus a planted error at one element must be reported at 4x its bar and pass at 0.5x -- so a harness that
compared the wrong tensors, or sized its bars wrongly, cannot pass the GPU test silently."""
import pytest
import torch

from tests import zero123_shadow as zs


def _plant(ref, bound, factor, at):
    out = ref.contiguous().clone()
    out.view(-1)[at] += factor * bound.contiguous().view(-1)[at]
    return out


def _cases():
    g = torch.Generator().manual_seed(3)
    x16 = lambda *s: torch.randn(*s, generator=g).half()
    x = x16(2, 16, 64)
    w, bias, res = x16(96, 64) * 0.125, x16(96), x16(2, 16, 96)
    wg, bg = x16(128, 64) * 0.125, x16(128)
    xc = x16(2, 32, 6, 5).contiguous(memory_format=torch.channels_last)
    wc = x16(32, 3, 3, 32) * 0.06
    qkv = x16(2, 64, 3, 2, 40)
    return [
        ("linear", lambda f: zs.linear_ref(x, w, bias, res), lambda f: f(x, w, bias, res)),
        ("linear", lambda f: zs.linear_ref(x, wg, bg, act="geglu"), lambda f: f(x, wg, bg, act="geglu")),
        ("conv3x3", lambda f: zs.conv_ref(xc, wc.permute(0, 3, 1, 2), None, None, 2, 0), lambda f: f(xc, wc, None, None, stride=2, pad=0)),
        ("conv3x3", lambda f: zs.conv_ref(xc, wc.permute(0, 3, 1, 2), bias[:32]), lambda f: f(xc, wc, bias[:32])),
        ("attention_qkv", lambda f: zs.attention_qkv_ref(qkv), lambda f: f(qkv)),
    ]


@pytest.mark.parametrize("case", range(5))
@pytest.mark.parametrize("factor,fails", [(4.0, True), (0.5, False), (0.0, False)])
def test_shadow_reports_a_planted_error_over_its_bar(case, factor, fails, monkeypatch):
    from dreammesh4d_amd import conv_mfma

    name, reference, call = _cases()[case]
    ref, bound = reference(None)
    at = ref.numel() // 3

    def fake(*args, **kw):          # "the kernel": the reference itself, off by factor x bar at one element
        return _plant(ref, bound, factor, at)

    monkeypatch.setattr(conv_mfma, name, fake)
    sh = zs.install(zs.Shadow(), monkeypatch)
    out = call(getattr(conv_mfma, name))
    assert torch.equal(out, _plant(ref, bound, factor, at))         # the wrapper hands the kernel's result on untouched
    assert len(sh.records) == 1
    r = sh.records[0]
    assert r.ratio == pytest.approx(factor, rel=1e-9, abs=1e-12)
    assert bool(sh.failures()) == fails
    assert r.op in sh.table()


def test_shadow_flags_non_finite_and_misshapen_results(monkeypatch):
    from dreammesh4d_amd import conv_mfma

    name, reference, call = _cases()[0]
    ref, _ = reference(None)
    bad = ref.contiguous().clone()
    bad.view(-1)[5] = float("nan")
    monkeypatch.setattr(conv_mfma, name, lambda *a, **k: bad)
    sh = zs.install(zs.Shadow(), monkeypatch)
    call(getattr(conv_mfma, name))
    monkeypatch.setattr(conv_mfma, name, lambda *a, **k: ref[:, :8])
    sh2 = zs.install(zs.Shadow(), monkeypatch)
    call(getattr(conv_mfma, name))
    assert sh.failures() and sh2.failures()


def test_bars_are_the_derived_rounding_terms():
    """Spot values of the bars: output rounding 2 x 2^-11 |ref| (+ the float32 accumulation term on sum |a b|), attention's
    uniform row (p = 1/L: the bar is 2 x 2^-11 (mean |v| + |mean v|) + the subnormal floor)."""
    x = torch.ones(1, 32, dtype=torch.float16)
    w = torch.ones(8, 32, dtype=torch.float16)
    ref, bound = zs.linear_ref(x, w)
    assert torch.all(ref == 32.0)
    assert torch.allclose(bound, torch.full_like(bound, 2 * (2.0 ** -11 * 32 + 2.0 ** -20 * 32) + 2 * 2.0 ** -25))
    L, D = 128, 40
    v = torch.randn(1, L, D).half()
    q = torch.zeros(1, L, D, dtype=torch.float16)
    ref, bound = zs.attention_ref(q, q, v, D ** -0.5)
    mean = v.double().mean(1, keepdim=True).expand(1, L, D)
    assert torch.allclose(ref, mean)
    want = 2 * 2.0 ** -11 * (v.double().abs().mean(1, keepdim=True) + mean.abs()) + L * 2.0 ** -25 * v.double().abs().max() + 2 * 2.0 ** -25
    assert torch.allclose(bound, want)
