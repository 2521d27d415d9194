"""Backward of GridAttn (mvdfusion/view_attn_efficient2.py:269-442) on the HIP path: from the gradient of the feature frustum
(V, S, S, D, 768) -- what the view-aligned transformers of the UNet hand back (backward_unet.py) -- to every `view_attn.*`
parameter and to the conditioning vector c (ViewFusion.time_embed).

Recompute-then-backward like the UNet blocks: the UNFUSED forward chain (token kernel, GEMMs, view attention, pooling) is re-run
keeping its intermediates, then

  final_layer_b  <- softmax-over-V pooling (weight_layer)  <- 3 x DiTBlock (adaLN-Zero: LayerNorm without affine + modulate, timm
  attention over the V reference views, GELU MLP, gates)   <- pre_layer_b (Linear 723 -> 256 + GELU)  <- token matrix
  <- bilinear gathers of the z-embedded latents (grid_sample backward = mvd_gridattn_tokens_backward)  <- z_embedder.

Matrix products run on the split-operand MFMA GEMM (backward.linear_backward), attention over V on mvd_attention_backward with
sequences of length V (the window W with keep_top_k_views: the chain below runs over W rows per 3-D point), LayerNorm+modulate on mvd_layernorm_backward with weight (1 + scale); elementwise glue (GELU', gates, the
(nseq, V, C) pooling algebra, the 5-channel z-embedding) is torch.
"""
import math

import torch
import torch.nn.functional as F

from . import backward as bw
from . import hip


def _gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z * 0.7071067811865476)) + z * torch.exp(-0.5 * z * z) * 0.3989422804014327


def _silu_grad(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def _modulation(blk, c):
    """(SiLU(c), the six adaLN vectors): (R, C) views of the (R, 6C) modulation, one row per conditioning row c (R, C)."""
    C = blk.hidden_size
    lin = blk.adaLN_modulation[1]
    sc_ = F.silu(c)
    mod = sc_ @ lin.weight.t() + lin.bias                                    # (R, 6C)   host glue
    return sc_, [mod[:, i * C:(i + 1) * C] for i in range(6)]


def _ln_modulate(h, out, scale, shift, T, C):
    """LayerNorm(h) * (1 + scale) + shift; scale / shift (R, C) apply to R equal scene-major row groups (mvd_layernorm_groups)."""
    return hip.layernorm_groups(h, out, scale, shift, T, C, T // scale.shape[0], eps=1e-6, w_plus_one=True)


def _gate(g, x):
    """g * x with the gate g (R, C): one row per R equal scene-major row groups of x (rows, C)."""
    R, C = g.shape
    return (x.reshape(R, -1, C) * g[:, None, :]).reshape(x.shape)


def _dit_block_backward(tape, blk, h, c, dh2, T, V):
    """One DiTBlock (view_attn_efficient2.py:42-67).  h (T, C) block input, c (R, C) conditioning (one row per scene with per-scene
    timesteps, each conditioning T / R scene-major rows), dh2 gradient at the block output.  Returns (dh, {name: grad}, dc (R, C))."""
    C, H = blk.hidden_size, blk.num_heads
    R = c.shape[0]
    dh_ = C // H
    lin = blk.adaLN_modulation[1]
    sc_, (sh1, s1, g1, sh2, s2, g2) = _modulation(blk, c)
    dev = h.device
    # ---- forward (unfused)
    m1 = hip.planes_like(T, C, dev)
    _ln_modulate(h, m1, s1, sh1, T, C)
    qkv = tape.linear(m1, blk.attn.qkv.weight, blk.attn.qkv.bias)           # (T, 3C): [q | k | v], each [heads][dhead]
    att = hip.planes_like(T, C, dev)
    hip.check(hip.lib().mvd_view_mha(hip.ptr(qkv), hip.ptr(att), T // V, V, H, dh_, hip.stream()))
    a_out = tape.linear(att, blk.attn.proj.weight, blk.attn.proj.bias)
    h1 = h + _gate(g1, a_out)
    m2 = hip.planes_like(T, C, dev)
    _ln_modulate(h1, m2, s2, sh2, T, C)
    f1 = tape.linear(m2, blk.mlp.fc1.weight, blk.mlp.fc1.bias)              # pre-activation (T, hidden)
    gel, _ = bw.act_planes(f1, hip.ACT_GELU)                               # GELU + operand split in one pass (mvd_act_planes)
    f2 = tape.linear(gel, blk.mlp.fc2.weight, blk.mlp.fc2.bias)
    # ---- backward
    g = {}
    dg2 = bw.col_sum_groups(dh2 * f2, R)
    dgel, g["mlp.fc2.weight"], g["mlp.fc2.bias"] = tape.linear_bwd(gel, blk.mlp.fc2.weight, _gate(g2, dh2))
    dm2, g["mlp.fc1.weight"], g["mlp.fc1.bias"] = tape.linear_bwd(m2, blk.mlp.fc1.weight, bw.act_backward(dgel, f1, hip.ACT_GELU))
    dx, ds2, dsh2 = bw.layernorm_backward_groups(h1.contiguous(), dm2.contiguous(), (1.0 + s2).contiguous(), 1e-6, R)
    dh1 = dh2 + dx
    dg1 = bw.col_sum_groups(dh1 * a_out, R)
    datt, g["attn.proj.weight"], g["attn.proj.bias"] = tape.linear_bwd(att, blk.attn.proj.weight, _gate(g1, dh1))
    q, k, v = (qkv[:, i * C:(i + 1) * C].contiguous() for i in range(3))
    dq, dk, dv = bw.attention_backward(q, k, v, datt.contiguous(), T // V, H, V, dh_)
    dm1, g["attn.qkv.weight"], g["attn.qkv.bias"] = tape.linear_bwd(m1, blk.attn.qkv.weight, torch.cat([dq, dk, dv], dim=1))
    dx, ds1, dsh1 = bw.layernorm_backward_groups(h.contiguous(), dm1.contiguous(), (1.0 + s1).contiguous(), 1e-6, R)
    dh = dh1 + dx
    dmod = torch.cat([dsh1, ds1, dg1, dsh2, ds2, dg2], dim=1)                # (R, 6C): one row per scene
    g["adaLN_modulation.1.bias"] = dmod.sum(0)
    g["adaLN_modulation.1.weight"] = dmod.t() @ sc_
    dc = (dmod @ lin.weight) * _silu_grad(c)
    return dh, g, dc


def fixed_point_scale(mx):
    """The power of two mvd_gridattn_tokens_backward* multiplies by before it rounds to its 64-bit fixed-point accumulators, for token
    gradients of largest magnitude mx: the largest gradient lands in [2^40, 2^41), which leaves 40 fractional bits below it and 22 bits
    of headroom above it for the sum over the rows that reach one texel.  The kernels take the scale as a C float, so the exponent stops
    at 127: for mx < 2^-87 the largest gradient lands lower (at 2^27 for mx = 2^-100, still past the 24 bits of an fp32 gradient).
    mx = 0 or not finite: 1."""
    if not (mx > 0 and math.isfinite(mx)):
        return 1.0
    return 2.0 ** min(40 - math.floor(math.log2(mx)), 127)


def gridattn_backward(ga, tape, eng, c, dvol, V, S, D):
    """ga: GridAttn; eng: the StepEngine whose buffers hold this step's inputs (x, depth noise, step table, cameras, input latents);
    c (R, 256) conditioning (eng.t_rows: N rows with per-scene timesteps, else 1); dvol (N*V*S*S*D, 768) gradient of the frustum of the
    engine's N*V views, scene-major.  Returns ({view_attn-relative name: grad}, dc (R, 256))."""
    L = hip.lib()
    dev = dvol.device
    C = ga.hidden_size
    N, sst = eng.N, eng.steps_scene_stride
    nseq = N * V * S * S * D
    W = ga.window                   # keep_top_k_views: W rig neighbours per point instead of all V views (0 = all)
    R = ga.rows_per_point(V)        # rows per 3-D point = the attention / pooling sequence length of everything below
    T = nseq * R
    agg = ga.aggregation_transformer
    # ---- forward (unfused chain, view_attn_efficient2.py GridAttn.run)
    z = ga.z_embedder[0]
    feat = torch.empty(N * V, S, S, 256, dtype=torch.float32, device=dev)
    in_feat = torch.empty(N, S, S, 256, dtype=torch.float32, device=dev)
    hip.check(L.mvd_zembed(hip.ptr(eng.x), hip.ptr(z.weight), hip.ptr(z.bias), hip.ptr(feat), N * V, S, hip.stream()))
    hip.check(L.mvd_zembed(hip.ptr(eng.input_latents), hip.ptr(z.weight), hip.ptr(z.bias), hip.ptr(in_feat), N, S, hip.stream()))
    half = 1.0 / float(S)
    grid_lin = torch.linspace(1.0 - half, -1.0 + half, S, dtype=torch.float32).to(dev)
    tokens = hip.planes_like(T, hip.TOKEN_LD, dev)
    dsrc, dsteps = eng.depth_geo()          # (the depth source the forward used: x itself, or an overwrite_attn_depth map)
    geo = (hip.ptr(dsrc), hip.ptr(eng.depth_noise), hip.ptr(dsteps), hip.ptr(eng.iter), hip.ptr(grid_lin))
    hip.check(L.mvd_gridattn_tokens_window(*geo, hip.ptr(feat), hip.ptr(in_feat), hip.ptr(eng.cams), hip.ptr(eng.in_cam), hip.ptr(tokens),
                                           N, V, 0, V, S, D, float(ga.depth_scale), float(ga.depth_shift), sst, W, hip.stream()))
    pre = ga.pre_layer_b[0]
    z0 = tape.linear(tokens, pre.weight, pre.bias)                             # (T, 256) pre-activation
    hs = [bw.act_planes(z0, hip.ACT_GELU, planes=False, f32=True)[1]]
    for blk in agg.layer_list:
        hcur = hs[-1]
        # block output via the inference path's own kernels (DiTBlock.run mutates its buffers: use the unfused algebra here)
        hs.append(_dit_forward(tape, blk, hcur, c, T, R))
    hL = hs[-1].view(nseq, R, C)
    wl = agg.weight_layer
    lg = hL @ wl.weight[0] + wl.bias                                           # (nseq, V)        host glue
    p = torch.softmax(lg, dim=1)
    pooled = (p[:, :, None] * hL).sum(1)                                       # (nseq, C)
    poolp = tape.planes(pooled)
    # ---- backward
    g = {}
    fin = ga.final_layer_b
    dpool, g["final_layer_b.weight"], g["final_layer_b.bias"] = tape.linear_bwd(poolp, fin.weight, dvol)
    a = (dpool[:, None, :] * hL).sum(2)                                        # (nseq, V): d pooled . h_v
    dlg = p * (a - (p * a).sum(1, keepdim=True))
    dh = (p[:, :, None] * dpool[:, None, :] + dlg[:, :, None] * wl.weight[0]).reshape(T, C)
    g["aggregation_transformer.weight_layer.weight"] = (dlg[:, :, None] * hL).sum((0, 1))[None, :]
    g["aggregation_transformer.weight_layer.bias"] = dlg.sum().reshape(1)
    dc = torch.zeros_like(c)
    for bi in range(len(agg.layer_list) - 1, -1, -1):
        dh, gb, dcb = _dit_block_backward(tape, agg.layer_list[bi], hs[bi], c, dh.contiguous(), T, R)
        g.update({f"aggregation_transformer.layer_list.{bi}.{k}": v for k, v in gb.items()})
        dc += dcb
    dtok, g["pre_layer_b.0.weight"], g["pre_layer_b.0.bias"] = tape.linear_bwd(tokens, pre.weight, bw.act_backward(dh, z0, hip.ACT_GELU))
    # ---- grid_sample backward into the z-embedded feature maps, then the 5 -> 256 z-embedding
    dtok = dtok.contiguous() if dtok.is_contiguous() else dtok
    base = dtok if dtok.storage_offset() == 0 else dtok.contiguous()
    ldt = base.stride(0)
    scale = fixed_point_scale(float(dtok[:, :512].abs().max()))
    dfeat_acc = torch.zeros(N * V, S, S, 256, dtype=torch.int64, device=dev)
    din_acc = torch.zeros(N, S, S, 256, dtype=torch.int64, device=dev)
    hip.check(L.mvd_gridattn_tokens_backward_window(*geo, hip.ptr(eng.cams), hip.ptr(eng.in_cam), hip.ptr(base), ldt, hip.ptr(dfeat_acc),
                                                    hip.ptr(din_acc), float(scale), N, V, 0, V, S, D, float(ga.depth_scale),
                                                    float(ga.depth_shift), sst, W, hip.stream()))
    dW = torch.zeros_like(z.weight)
    db = torch.zeros_like(z.bias)
    for lat, acc, n in ((eng.x, dfeat_acc, N * V), (eng.input_latents, din_acc, N)):
        xp = lat.reshape(n, 5, S * S).permute(0, 2, 1).reshape(n * S * S, 5)
        zz = xp @ z.weight.t() + z.bias
        dz = (acc.double() / scale).float().reshape(n * S * S, 256) * _gelu_grad(zz)
        dW += dz.t() @ xp
        db += dz.sum(0)
    g["z_embedder.0.weight"], g["z_embedder.0.bias"] = dW, db
    return g, dc


def _dit_forward(tape, blk, h, c, T, V):
    """Unfused DiTBlock forward returning the block output (same algebra as _dit_block_backward's forward half); c (R, C)."""
    C, H = blk.hidden_size, blk.num_heads
    _, (sh1, s1, g1, sh2, s2, g2) = _modulation(blk, c)
    dev = h.device
    m1 = hip.planes_like(T, C, dev)
    _ln_modulate(h, m1, s1, sh1, T, C)
    qkv = tape.linear(m1, blk.attn.qkv.weight, blk.attn.qkv.bias)
    att = hip.planes_like(T, C, dev)
    hip.check(hip.lib().mvd_view_mha(hip.ptr(qkv), hip.ptr(att), T // V, V, H, C // H, hip.stream()))
    h1 = _gated_residual(tape, att, blk.attn.proj, h, g1)
    m2 = hip.planes_like(T, C, dev)
    _ln_modulate(h1, m2, s2, sh2, T, C)
    f1 = tape.linear(m2, blk.mlp.fc1.weight, blk.mlp.fc1.bias)
    return _gated_residual(tape, bw.act_planes(f1, hip.ACT_GELU)[0], blk.mlp.fc2, h1, g2)


def _gated_residual(tape, a, lin, res, g):
    """res + g * lin(a).  A gate shared by every row (g (1, C)) is the GEMM's own epilogue; one gate row per scene is elementwise glue."""
    if g.shape[0] == 1:
        return tape.linear(a, lin.weight, lin.bias, res=res, colscale=g[0])
    return res + _gate(g, tape.linear(a, lin.weight, lin.bias))


def time_embed_backward(time_embed, t_sin, dc):
    """ViewFusion.time_embed = Linear(256,256) / SiLU / Linear(256,256) on the sinusoid of t; only row 0 feeds GridAttn
    (viewfusion_zero_depth_rgb.py:276-279, 303).  Host glue.  Returns {relative name: grad}."""
    l1, l2 = time_embed[0], time_embed[2]
    z1 = t_sin @ l1.weight.t() + l1.bias
    e1 = F.silu(z1)
    g = {"2.weight": dc.t() @ e1, "2.bias": dc.sum(0)}                      # (one row per scene: summed over the scenes)
    dz1 = (dc @ l2.weight) * _silu_grad(z1)
    g["0.weight"], g["0.bias"] = dz1.t() @ t_sin, dz1.sum(0)
    return g
