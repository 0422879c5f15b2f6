"""Shadow check of the Zero123 SDS step's hand-written kernels: every Python entry point that reaches a HIP kernel is wrapped;
the wrapper calls the original, then recomputes the same operation in FLOAT64 with plain torch operators from the same float16
inputs the kernel received, and records (op, shapes, max |error| / bound).  Used by tests/test_zero123_fullsize_gpu.py (the
full-size model) and tests/test_attention_gpu.py (the attention bar); tests/test_zero123_shadow_cpu.py keeps the harness itself
honest on the CPU.

Convolutions are recomputed in float64 as well (torch's direct convolution on the device); only the magnitude sums that size
the float32-accumulation term below are float32.

Bars, per element, all of the form  SAFETY * (sum of the rounding terms of the kernel's arithmetic) + a subnormal floor:
  * float16 output rounding: U16 |ref| (U16 = 2^-11, the unit roundoff), or SUB16 = 2^-25 below float16's normal range;
  * a second rounding where the kernel re-rounds an intermediate: the conv / linear epilogue rounds acc + bias to float16
    before it adds the residual (U16 |acc + bias|), the GEGLU epilogue rounds the value and the gate projections, the
    attention kernel rounds its probabilities, add_layer_norm rounds x + tok;
  * float32 accumulation of K float16 products (exact in float32): ACC32 sum_k |a_k b_k|.  Blocked MFMA / split-K sums
    make the observed error ~2^-24 sum |a b| whatever K; ACC32 = 2^-20 keeps a 16x margin on that and does NOT grow with K
    (a K-proportional worst-case term would be looser than the output rounding at K = 2560 x 9);
  * float32 statistics (group / layer norms): STAT32 |gamma| (|xhat| + 1) for the forward (shifted / two-pass float32
    sums over up to 2^18 elements: relative mean / variance errors far below 2^-16), and the same relative size on the
    group sums of the backward;
  * SAFETY = 2.
"""
import collections
import math

import torch
import torch.nn.functional as F

U16 = 2.0 ** -11
SUB16 = 2.0 ** -25
ACC32 = 2.0 ** -20
STAT32 = 2.0 ** -16
SAFETY = 2.0
TINY = SAFETY * SUB16

Record = collections.namedtuple("Record", "op shape ratio max_err")


# ----------------------------------------------------------------------------- float64 references and their bars
def _d(t):
    return None if t is None else t.detach().double()


def _conv(x, w, stride, pad, f32=False):
    """y = conv(x, w) (3x3); pad 0 with stride 2 is the VAE encoder's Downsample: one zero row / column BEHIND each axis."""
    if f32:
        x, w = x.float().abs(), w.float().abs()
    if stride == 2 and pad == 0:
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, None, 2, 0)
    return F.conv2d(x, w, None, stride, pad)


def conv_ref(x, w_oihw, bias=None, residual=None, stride=1, pad=1):
    """(ref, bound) of conv_mfma.conv3x3: y = fp16(fp16(acc + bias) + residual) (split-K: one rounding of the sum)."""
    acc = _conv(_d(x), _d(w_oihw), stride, pad)
    pre = acc if bias is None else acc + _d(bias).view(1, -1, 1, 1)
    ref = pre if residual is None else pre + _d(residual)
    mag = _conv(x, w_oihw, stride, pad, f32=True).double()
    bound = U16 * ref.abs() + ACC32 * mag
    if residual is not None:
        bound = bound + U16 * pre.abs() + SUB16
    return ref, SAFETY * bound + TINY


def conv_dgrad_ref(dy, w_oihw, in_shape, stride=1, pad=1):
    """(ref, bound) of dL/dx of a 3x3 convolution with filter w_oihw, from dL/dy (one float16 rounding)."""
    N, C, H, W = in_shape

    def g(dy_, w_):
        if stride == 2 and pad == 0:
            return torch.nn.grad.conv2d_input((N, C, H + 1, W + 1), w_, dy_, stride=2, padding=0)[:, :, :H, :W]
        return torch.nn.grad.conv2d_input((N, C, H, W), w_, dy_, stride=stride, padding=pad)

    ref = g(_d(dy), _d(w_oihw))
    mag = g(dy.detach().float().abs(), w_oihw.detach().float().abs()).double()
    return ref, SAFETY * (U16 * ref.abs() + ACC32 * mag) + TINY


def _gelu(g):
    return 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))


def _gelu_slope(g):
    return 0.5 * (1.0 + torch.erf(g / math.sqrt(2.0))) + g * torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)


def linear_ref(x, w, bias=None, residual=None, act=None):
    """(ref, bound) of conv_mfma.linear.  act="geglu": w / bias packed by conv_mfma.pack_geglu (blocks of 64 value rows, then 64
    gate rows); the epilogue rounds both projections to float16 and evaluates value x gelu(gate) in float32."""
    xd, wd = _d(x), _d(w)
    acc = xd @ wd.t()
    pre = acc if bias is None else acc + _d(bias)
    mag = (x.detach().float().abs() @ w.detach().float().abs().t()).double()
    if act == "geglu":
        lead = pre.shape[:-1]
        pv, pm = (t.reshape(*lead, -1, 2, 64) for t in (pre, mag))
        v, g, mv, mg = pv[..., 0, :], pv[..., 1, :], pm[..., 0, :], pm[..., 1, :]
        ref = v * _gelu(g)
        s = _gelu_slope(g).abs()
        # value: rounded (U16 |v|) after float32 accumulation (ACC32 mv); gate: the same through gelu's slope; output rounding
        bound = U16 * ref.abs() + (U16 * v.abs() + ACC32 * mv) * _gelu(g).abs() + v.abs() * s * (U16 * g.abs() + ACC32 * mg) + SUB16
        return ref.reshape(*lead, -1), (SAFETY * bound + TINY).reshape(*lead, -1)
    ref = pre if residual is None else pre + _d(residual)
    bound = U16 * ref.abs() + ACC32 * mag
    if residual is not None:
        bound = bound + U16 * pre.abs() + SUB16
    return ref, SAFETY * bound + TINY


def attention_ref(q, k, v, scale):
    """(ref, bound) of softmax(q k^T scale) v for q, k, v [..., L, D] (any float dtype; the kernel's inputs are float16).
    |o - o_ref| <= 2 (2^-11 sum_j p_ij |v_j| (1 + e_ij) + 2^-11 |o_ref|) + tiny:
      2^-11 p |v|: the float16 probabilities (relative to the running maximum, <= 1) that meet v on the matrix cores;
      e_ij = 2^9 ACC32 scale sum_d |q_d k_d|: the float32 score's accumulation error, relative, through exp (~0 unless the
          scores are large);
      2^-11 |o_ref|: the output rounding;
      tiny = L 2^-25 max_j |v_j| + 2 SUB16: probabilities below float16's normal range (2^-14 of the running maximum) carry an
          absolute error up to 2^-25 each (or underflow to 0), and the normaliser is >= 1."""
    qd, kd, vd = _d(q), _d(k), _d(v)
    p = torch.softmax((qd @ kd.transpose(-1, -2)) * scale, dim=-1)
    ref = p @ vd
    es = (2.0 ** 9 * ACC32 * scale) * (q.detach().float().abs() @ k.detach().float().abs().transpose(-1, -2)).double()
    L = q.shape[-2]
    vmax = vd.abs().amax(dim=(-1, -2), keepdim=True)
    bound = SAFETY * (U16 * ((p * (1.0 + es)) @ vd.abs()) + U16 * ref.abs()) + L * SUB16 * vmax + TINY
    return ref, bound


def attention_qkv_ref(qkv, scale=None):
    """attention_ref for conv_mfma.attention_qkv's [B, L, 3, H, D] input -> ([B, L, H D], bound)."""
    B, L, _, H, D = qkv.shape
    s = float(D ** -0.5 if scale is None else scale)
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))                      # [B, H, L, D]
    ref, bound = attention_ref(q, k, v, s)
    return ref.transpose(1, 2).reshape(B, L, H * D), bound.transpose(1, 2).reshape(B, L, H * D)


def _group_stats(xa, groups, eps):
    N, C = xa.shape[:2]
    xg = xa.reshape(N, groups, -1)
    mean = xg.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(xg.var(-1, unbiased=False, keepdim=True) + eps)
    return ((xg - mean) * rstd).reshape(xa.shape), rstd.expand_as(xg).reshape(xa.shape)


def _with_add(x, add):
    xa = _d(x).contiguous()
    if add is not None:
        xa = xa + _d(add).reshape(-1, x.shape[1], 1, 1)
    return xa


def group_norm_ref(x, gamma, beta, add, groups, eps, silu):
    """(ref, bound) of silu?((x + add - mean) rstd gamma + beta) (fused_norm._GroupNormNHWC.forward)."""
    xh, _ = _group_stats(_with_add(x, add), groups, eps)
    gm = _d(gamma).view(1, -1, 1, 1)
    z = xh * gm + _d(beta).view(1, -1, 1, 1)
    ref = z * torch.sigmoid(z) if silu else z
    bound = U16 * ref.abs() + STAT32 * gm.abs() * (xh.abs() + 1.0) * (1.1 if silu else 1.0)     # (|silu'| <= 1.1)
    return ref, SAFETY * bound + TINY


def group_norm_bwd_ref(x, gamma, beta, add, groups, eps, silu, dy, d_skip=None):
    """(ref, bound) of dL/dx of group_norm_ref (frozen gamma / beta, `add` a constant), + d_skip (the branch around the norm):
    dx = rstd (g - mean_group(g) - xhat mean_group(g xhat)), g = dy silu'(z) gamma; float32 group sums -> STAT32 on their size."""
    xa = _with_add(x, add)
    xh, rstd = _group_stats(xa, groups, eps)
    gm = _d(gamma).view(1, -1, 1, 1)
    z = xh * gm + _d(beta).view(1, -1, 1, 1)
    dz = _d(dy).contiguous()
    if silu:
        s = torch.sigmoid(z)
        dz = dz * s * (1.0 + z * (1.0 - s))
    g = dz * gm
    N, G = x.shape[0], groups
    gmean = lambda t: t.reshape(N, G, -1).mean(-1, keepdim=True).expand(N, G, t[0].numel() // G).reshape(t.shape)
    ref = rstd * (g - gmean(g) - xh * gmean(g * xh))
    if d_skip is not None:
        ref = ref + _d(d_skip)
    bound = U16 * ref.abs() + STAT32 * rstd * (g.abs() + gmean(g.abs()) * (1.0 + xh.abs()))
    return ref, SAFETY * bound + TINY


def add_bias_ref(a, b, bias):
    ref = _d(a) + _d(b) + _d(bias).view(1, -1, 1, 1)
    return ref, SAFETY * U16 * ref.abs() + TINY


def geglu_ref(proj):
    """(ref, bound) of x gelu(gate), proj = [x | gate] (float32 evaluation, one rounding)."""
    x, g = _d(proj).chunk(2, dim=-1)
    ref = x * _gelu(g)
    return ref, SAFETY * (U16 * ref.abs() + STAT32 * x.abs() * (g.abs() + 1.0)) + TINY


def add_layer_norm_ref(gamma, beta, eps, x, tok=None, bias2=None):
    """((n_ref, n_bound), (xb_ref, xb_bound)) of fused_norm.add_layer_norm: s = x + tok (rounded to float16 in the kernel, like
    the separate add it replaces), n = LayerNorm(s) gamma + beta, xb = s + bias2 (float16)."""
    B, L, C = x.shape
    s = _d(x)
    if tok is not None:
        s = s + _d(tok).reshape(B, 1, C)
    mean = s.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(s.var(-1, unbiased=False, keepdim=True) + eps)
    xh = (s - mean) * rstd
    gm = _d(gamma)
    n = xh * gm + _d(beta)
    nb = U16 * n.abs() + STAT32 * gm.abs() * (xh.abs() + 1.0)
    sb = torch.zeros_like(s)
    if tok is not None:         # the rounding of s moves xhat by up to 2^-11 (|s| + mean |s| (1 + |xhat|)) rstd
        sb = U16 * s.abs() + SUB16
        nb = nb + gm.abs() * rstd * (sb + sb.mean(-1, keepdim=True) * (1.0 + xh.abs()))
    xb = s if bias2 is None else s + _d(bias2)
    return (n, SAFETY * nb + TINY), (xb, SAFETY * (U16 * xb.abs() + sb) + TINY)


# ----------------------------------------------------------------------------- the recorder
class Shadow:
    """Records of checked kernel calls.  Nested entry points (conv3x3 inside a frozen convolution's backward, ...) are counted
    in `calls` but checked by the outermost wrapper only."""

    def __init__(self):
        self.records, self.calls, self.flops, self.depth = [], collections.Counter(), 0, 0

    def record(self, op, shape, got, ref, bound):
        got = got.detach().double()
        if got.shape != ref.shape:
            self.records.append(Record(op, shape, math.inf, math.inf))
            return
        err = (got - ref).abs()
        ratio = float((err / bound).max()) if err.numel() else 0.0
        if not bool(torch.isfinite(got).all()):
            ratio = math.inf
        self.records.append(Record(op, shape, ratio, float(err.max()) if err.numel() else 0.0))

    def failures(self):
        return [r for r in self.records if not r.ratio <= 1.0]

    def count(self):
        return collections.Counter(r.op for r in self.records)

    def worst(self):
        out = {}
        for r in self.records:
            if r.op not in out or not r.ratio <= out[r.op].ratio:
                out[r.op] = r
        return out

    def table(self):
        n = self.count()
        lines = [f"{'op':28s} {'calls':>5s} {'worst err/bound':>15s}  worst shape"]
        for op, r in sorted(self.worst().items()):
            lines.append(f"{op:28s} {n[op]:5d} {r.ratio:15.4f}  {r.shape}")
        return "\n".join(lines)


def _shape(*ts):
    return tuple(tuple(t.shape) if torch.is_tensor(t) else t for t in ts)


def install(shadow, monkeypatch):
    """Wrap every entry point of the SDS step that reaches a hand-written kernel (conv_mfma, fused_norm, and the names zero123
    bound at import: geglu, add_layer_norm)."""
    from dreammesh4d_amd import conv_mfma as cm, fused_norm as fn, zero123 as z

    def checked(fn_, check, tally=None):
        """call fn_; tally(*args, **kw) at every depth (launch counts, flops); at depth 0 check(result, *args, **kw) -> iterable
        of (op, shape, got, ref, bound)."""
        def run(*args, **kw):
            outer = shadow.depth == 0
            shadow.depth += 1
            try:
                out = fn_(*args, **kw)
            finally:
                shadow.depth -= 1
            if tally is not None:
                tally(*args, **kw)
            if outer:
                with torch.no_grad():
                    for rec in check(out, *args, **kw):
                        shadow.record(*rec)
            return out
        return run

    # --- conv_mfma
    def n_conv(x, w_ohwi, bias=None, residual=None, stride=1, pad=1):
        N, Ci, H, W = x.shape
        H, W = (H, W) if stride == 1 else (((H + 1) // 2, (W + 1) // 2) if pad else (H // 2, W // 2))
        shadow.calls["conv3x3" if stride == 1 else "conv3x3_s2"] += 1
        shadow.flops += 2 * N * H * W * Ci * int(w_ohwi.shape[0]) * 9

    def chk_conv(y, x, w_ohwi, bias=None, residual=None, stride=1, pad=1):
        ref, b = conv_ref(x, w_ohwi.permute(0, 3, 1, 2), bias, residual, stride, pad)
        yield ("conv3x3" if stride == 1 else f"conv3x3_s2_pad{pad}") + ("_res" if residual is not None else ""), \
            _shape(x, w_ohwi), y, ref, b

    def n_linear(x, w, bias=None, residual=None, act=None):
        shadow.calls["linear"] += 1
        shadow.flops += 2 * (x.numel() // x.shape[-1]) * int(x.shape[-1]) * int(w.shape[0])

    def chk_linear(y, x, w, bias=None, residual=None, act=None):
        ref, b = linear_ref(x, w, bias, residual, act)
        yield "linear" + ("_geglu" if act else "") + ("_res" if residual is not None else ""), _shape(x, w), y, ref, b

    def n_attn(qkv, scale=None):
        B, L, _, H, D = qkv.shape
        shadow.calls["attention"] += 1
        shadow.flops += 4 * B * H * L * L * D

    def chk_attn(o, qkv, scale=None):
        ref, b = attention_qkv_ref(qkv, scale)
        yield "attention", _shape(qkv), o, ref, b

    def n_s2_dgrad(dy, w_cls, in_shape):
        N, Ci, H, W = in_shape
        shadow.calls["conv3x3_s2_dgrad"] += 1
        shadow.flops += 2 * N * (H // 2) * (W // 2) * Ci * int(dy.shape[1]) * 9

    monkeypatch.setattr(cm, "conv3x3", checked(cm.conv3x3, chk_conv, n_conv))
    monkeypatch.setattr(cm, "linear", checked(cm.linear, chk_linear, n_linear))
    monkeypatch.setattr(cm, "attention_qkv", checked(cm.attention_qkv, chk_attn, n_attn))
    # (its only caller is the stride-2 backward below, which checks it against the forward's own filter)
    monkeypatch.setattr(cm, "conv3x3_s2_dgrad", checked(cm.conv3x3_s2_dgrad, lambda *a: (), n_s2_dgrad))

    # the frozen convolutions' data gradients, against the FILTER OF THE FORWARD (not the packed transposed copy the kernel reads)
    f3 = cm._Conv3x3Frozen
    fwd3, bwd3 = f3.forward, f3.backward

    def fwd3_(ctx, x, w_ohwi, w_t, bias, residual):
        ctx.shadow_w, ctx.shadow_in = w_ohwi, tuple(x.shape)
        return fwd3(ctx, x, w_ohwi, w_t, bias, residual)

    def chk_bwd3(out, ctx, dy):
        if out[0] is not None:
            ref, b = conv_dgrad_ref(dy, ctx.shadow_w.permute(0, 3, 1, 2), ctx.shadow_in)
            yield "conv3x3_dgrad", _shape(dy, ctx.shadow_w), out[0], ref, b

    monkeypatch.setattr(f3, "forward", staticmethod(fwd3_))
    monkeypatch.setattr(f3, "backward", staticmethod(checked(bwd3, chk_bwd3)))

    ff = cm._ConvFirstFrozen
    fwdf, bwdf = ff.forward, ff.backward

    def fwdf_(ctx, x, w, b, w_t, w_pad=None, b_pad=None):
        ctx.shadow_w, ctx.shadow_in = w, tuple(x.shape)
        return fwdf(ctx, x, w, b, w_t, w_pad, b_pad)

    def n_bwdf(ctx, dy):
        if ctx.needs_input_grad[0]:
            N, Ci, H, W = ctx.shadow_in
            shadow.calls["conv3x3_c128_small_dgrad"] += 1
            shadow.flops += 2 * N * H * W * Ci * int(dy.shape[1]) * 9

    def chk_bwdf(out, ctx, dy):
        if out[0] is not None:
            ref, b = conv_dgrad_ref(dy, ctx.shadow_w, ctx.shadow_in)
            yield "conv3x3_c128_small_dgrad", _shape(dy, ctx.shadow_w), out[0], ref, b

    monkeypatch.setattr(ff, "forward", staticmethod(fwdf_))
    monkeypatch.setattr(ff, "backward", staticmethod(checked(bwdf, chk_bwdf, n_bwdf)))

    fs2 = cm._Conv3x3Stride2Frozen

    def chk_bwds2(out, ctx, dy):
        if out[0] is not None:
            (w,) = ctx.saved_tensors
            ref, b = conv_dgrad_ref(dy, w, ctx.in_shape, stride=2, pad=ctx.pad)
            yield f"conv3x3_s2_pad{ctx.pad}_dgrad", _shape(dy, w), out[0], ref, b

    monkeypatch.setattr(fs2, "backward", staticmethod(checked(fs2.backward, chk_bwds2)))

    # --- fused_norm: group norm (forward / backward), add_bias, geglu, add_layer_norm
    gn = fn._GroupNormNHWC
    gfwd, gbwd = gn.forward, gn.backward

    def chk_gfwd(out, ctx, x, weight, bias, add, groups, eps, silu, skip=False):
        ctx.shadow_eps = eps
        y = out[0] if skip else out
        ref, b = group_norm_ref(x, weight, bias, add, groups, eps, silu)
        yield "group_norm" + ("_add" if add is not None else "") + ("_silu" if silu else ""), _shape(x), y, ref, b

    def chk_gbwd(out, ctx, dy, d_skip=None):
        if dy is None:
            return
        x, weight, bias, stats, add = ctx.saved_tensors
        groups, silu, _, _ = ctx.cfg
        ref, b = group_norm_bwd_ref(x, weight, bias, add, groups, ctx.shadow_eps, silu, dy, d_skip)
        yield "group_norm_bwd" + ("_skip" if d_skip is not None else ""), _shape(x), out[0], ref, b

    monkeypatch.setattr(gn, "forward", staticmethod(checked(gfwd, chk_gfwd)))
    monkeypatch.setattr(gn, "backward", staticmethod(checked(gbwd, chk_gbwd)))

    ab = fn._AddBias

    def chk_ab(y, ctx, a, b, bias):
        ref, bd = add_bias_ref(a, b, bias)
        yield "add_bias", _shape(a), y, ref, bd

    monkeypatch.setattr(ab, "forward", staticmethod(checked(ab.forward, chk_ab)))

    def chk_geglu(y, proj):
        if proj.is_cuda:
            ref, b = geglu_ref(proj)
            yield "geglu", _shape(proj), y, ref, b

    def chk_aln(out, norm, x, tok=None, bias2=None, want_sum=True):
        (nr, nb), (xr, xbb) = add_layer_norm_ref(norm.weight, norm.bias, norm.eps, x, tok, bias2)
        yield "add_layer_norm", _shape(x), out[0], nr, nb
        if want_sum:
            yield "add_layer_norm_sum", _shape(x), out[1], xr, xbb

    geglu, aln = checked(fn.geglu, chk_geglu), checked(fn.add_layer_norm, chk_aln)
    for mod in (fn, z):          # (zero123 bound both names at import)
        monkeypatch.setattr(mod, "geglu", geglu)
        monkeypatch.setattr(mod, "add_layer_norm", aln)
    return shadow
