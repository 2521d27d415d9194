"""tests/norm_f64.py on the CPU: every reference against an independent torch FLOAT64 statement (F.group_norm, F.layer_norm,
torch.softmax, autograd) on every fixture, the conditions the fixtures promise, and the proof that the bars have teeth on the exact
case lists tests/test_gpu_norm_f64.py parametrises over: every mutant of a reference is rejected by at least one of those cases (at the
LOOSEST bar the GPU file applies, the bf16 flavour's PL), and a float32 emulation of gn_stats_kernel + gn_apply_kernel -- the
kernel's own summation order -- stays under half of the GroupNorm forward bar (at the TIGHTEST one, the fp16 flavour's PL) on all of them.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import attention_f64 as A
import norm_f64 as N

PL_F16, PL_BF16 = 1e-6, 2e-5          # tests/test_gpu_ops.py PL of the two flavours


def _ids(cases):
    return ["-".join(str(x) for x in (c if isinstance(c, tuple) else (c,))) for c in cases]


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


# ------------------------------------------------------------------------------------------------ references against torch float64
def _torch_gn(x, gm, bt, G, eps, silu):
    y = F.group_norm(x.permute(0, 2, 1), G, gm, bt, eps=eps).permute(0, 2, 1)
    return F.silu(y) if silu else y


@pytest.mark.parametrize("shape", N.GN_SHAPES + [N.GN_BIG], ids=_ids(N.GN_SHAPES + [N.GN_BIG]))
def test_groupnorm_references_equal_torch_float64(shape):
    B, HW, C, G = shape
    gm, bt = (t.double() for t in N.gn_params(C))
    eps = N.f32(N.GN_EPS)
    for fx in (("big",) if shape == N.GN_BIG else N.GN_FIXTURES):
        x = N.gn_fixture(fx, *shape).double()
        for silu in (False, True):
            assert _rel(N.gn_forward(x, gm, bt, G, N.GN_EPS, silu), _torch_gn(x, gm, bt, G, eps, silu)) < 1e-12, (fx, silu)
            if shape not in N.GN_BWD_SHAPES or fx not in N.GN_BWD_FIXTURES:
                continue
            x = N.gn_fixture(fx, *shape, full=True).double()
            xa, ga, ba = (t.clone().requires_grad_() for t in (x, gm, bt))
            dy = N.gn_dy(B, HW, C).double()
            _torch_gn(xa, ga, ba, G, eps, silu).backward(dy)
            dx, dg, db = N.gn_backward(x, dy, gm, bt, G, N.GN_EPS, silu)
            assert _rel(dx, xa.grad) < 1e-12 and _rel(dg, ga.grad) < 1e-12 and _rel(db, ba.grad) < 1e-12, (fx, silu)


def test_groupnorm_fp16_rounding_flag_reference():
    shape, fx = N.GN_F16_CASE
    x, (gm, bt) = N.gn_fixture(fx, *shape).double(), (t.double() for t in N.gn_params(shape[2]))
    y = _torch_gn(x, gm, bt, shape[3], N.f32(N.GN_EPS), False).float().half().double()
    assert _rel(N.gn_forward(x, gm, bt, shape[3], N.GN_EPS, True, round_f16=True), y * torch.sigmoid(y)) < 1e-12


@pytest.mark.parametrize("rows,C,rpg,wp1", N.ln_cases(), ids=_ids(N.ln_cases()))
def test_layernorm_forward_reference_equals_torch_float64(rows, C, rpg, wp1):
    ng = rows // rpg if rpg else 1
    w, b = (t.double() for t in N.ln_params(ng, C, 6 if rpg else 1))
    for fx in N.LN_FIXTURES:
        x = N.ln_fixture(fx, rows, C).double()
        pick = torch.arange(rows) // (rpg or rows)
        want = F.layer_norm(x, (C,), eps=N.f32(N.LN_EPS)) * ((1 + w if wp1 else w)[pick]) + b[pick]
        assert _rel(N.ln_forward(x, w, b, N.LN_EPS, wp1, rpg or None), want) < 1e-12, fx
    want = F.layer_norm(x, (C,), eps=N.f32(N.LN_EPS))
    assert _rel(N.ln_forward(x, None, None, N.LN_EPS), want) < 1e-12


@pytest.mark.parametrize("rows,C,rpg", N.ln_bwd_cases(), ids=_ids(N.ln_bwd_cases()))
def test_layernorm_backward_reference_equals_autograd_float64(rows, C, rpg):
    ng = rows // rpg if rpg else 1
    w = N.ln_params(ng, C, 6 if rpg else 1)[0].double()
    dy = torch.randn(rows, C, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    pick = torch.arange(rows) // (rpg or rows)
    for fx in N.LN_FIXTURES:
        x = N.ln_fixture(fx, rows, C).double()
        xa, wa, ba = x.clone().requires_grad_(), w.clone().requires_grad_(), torch.zeros(ng, C, dtype=torch.float64, requires_grad=True)
        (F.layer_norm(xa, (C,), eps=N.f32(N.LN_EPS)) * wa[pick] + ba[pick]).backward(dy)
        dx, dw, db = N.ln_backward(x, dy, w, N.LN_EPS, rpg or None)
        assert _rel(dx, xa.grad) < 1e-12 and _rel(dw, wa.grad) < 1e-12 and _rel(db, ba.grad) < 1e-12, fx


def test_softmax_and_column_sum_references():
    for (rows, cols, ldx), fx, sc in N.softmax_cases():
        x = N.softmax_fixture(fx, rows, cols, ldx, sc).double()
        want = N.SOFTMAX_OUT_SCALE * torch.softmax(x[:, :cols] * N.f32(sc), 1)
        assert _rel(N.softmax_rows(x[:, :cols], sc, N.SOFTMAX_OUT_SCALE), want) < 1e-12, (rows, cols, fx, sc)
    x = N.col_sum_fixture(513, 33, 40)
    assert torch.equal(N.col_sum(x[:, :33])[0], x[:, :33].double().sum(0))
    xg = N.col_sum_fixture(900, 31)
    assert torch.equal(N.col_sum(xg, 3), torch.stack([xg[i * 300:(i + 1) * 300].double().sum(0) for i in range(3)]))
    for m, s in [(1e6, 2.0 ** -9), (1024.0, 1.0), (2047.9, 1.0), (2048.0, 0.5), (3e-7, 2.0 ** 32), (0.0, 1.0)]:
        assert N.pow2_scale(torch.tensor([0.0, -m, m / 3])) == (s, 1.0 / s), m
        assert m == 0.0 or 1024.0 <= m * s < 2048.0


def test_elementwise_references_equal_autograd_float64():
    for rows, cols in N.ELEMENTWISE_SHAPES:
        x = N.value_grid(rows, cols, "x").double()
        dy = N.value_grid(rows, cols, "dy").double()
        for act, fn in ((N.ACT_GELU, F.gelu), (N.ACT_SILU, F.silu)):
            xa = x.clone().requires_grad_()
            y = fn(xa)
            y.backward(dy)
            y = y.detach()
            assert float((N.act_forward(x, act) - y).abs().max()) <= 1e-12 * float(y.abs().max() + 1)
            assert bool(((N.act_backward(dy, x, act) - xa.grad).abs() <= 1e-12 * (dy.abs() + xa.grad.abs())).all()), act
        h = N.value_grid(rows, 2 * cols, "h").double().requires_grad_()
        a, g = h.chunk(2, dim=-1)
        (a * F.gelu(g)).backward(dy)
        dh, floor = N.geglu_backward(h, dy)
        assert bool(((dh - h.grad).abs() <= 1e-12 * (floor + h.grad.abs())).all())
        assert bool(torch.isfinite(dh).all())
    vals = set(N.value_grid(37, 50).flatten().tolist())
    assert all(v in vals for v in torch.tensor(N.VALUE_GRID).tolist())


@pytest.mark.parametrize("P,D,H,d", N.PIXEL_BWD_CASES, ids=_ids(N.PIXEL_BWD_CASES))
def test_pixel_cross_attn_backward_reference_equals_autograd(P, D, H, d):
    for fx in N.PIXEL_BWD_FIXTURES:
        q, k, v, dout = (t.double() for t in N.pixel_bwd_fixture(fx, P, D, H, d))
        qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))
        qh = qa.view(P, 1, H, d).permute(0, 2, 1, 3)
        kh, vh = (t.view(P, D, H, d).permute(0, 2, 1, 3) for t in (ka, va))
        o = torch.softmax(qh @ kh.transpose(-1, -2) * d ** -0.5, dim=-1) @ vh
        assert _rel(o.permute(0, 2, 1, 3).reshape(P, H * d), A.pixel_cross_attention(q, k, v, P, D, H, d)[0]) < 1e-12
        o.permute(0, 2, 1, 3).reshape(P, H * d).backward(dout)
        (dq, dk, dv), (sq, sk, sv) = N.pixel_xattn_backward(q, k, v, dout, P, D, H, d)
        # to 1e-12 of the per-(pixel, head) scale the GPU test measures against
        assert N.worst(dq.reshape(P * H, d), qa.grad.reshape(P * H, d), 1e-12 * sq + 1e-300, P * H) <= 1.0
        assert N.worst(N.pixel_by_head(dk, P, D, H, d), N.pixel_by_head(ka.grad, P, D, H, d), 1e-12 * sk + 1e-300, P * H) <= 1.0
        assert N.worst(N.pixel_by_head(dv, P, D, H, d), N.pixel_by_head(va.grad, P, D, H, d), 1e-12 * sv + 1e-300, P * H) <= 1.0


# ------------------------------------------------------------------------------------------------ what the fixtures promise
def test_fixture_conditions():
    k = lambda fx, shape: N.gn_kappa(N.gn_fixture(fx, *shape), shape[3], N.GN_EPS)
    for shape in [(2, 64, 320, 32), (1, 1024, 64, 32)]:
        assert float((k("plain", shape) - 1.0625).abs().max()) < 0.2
        assert float((k("offset8", shape) / 65 - 1).abs().max()) < 0.25 and float((k("offset64", shape) / 4097 - 1).abs().max()) < 0.25
        assert float(k("tiny", shape).max()) < 2e-3                    # var = 1e-8 << eps
        xc = N.by_group(N.gn_fixture("chan_offset", *shape).double(), shape[3])
        assert float(xc.var(1).median()) > 4                           # the channel means carry the group variance (N(0, 1) alone: 1)
        kc = k("const", shape)
        assert float(kc[0]) == pytest.approx(3.7 ** 2 / N.GN_EPS, rel=1e-6) and float(kc[1:].max()) < 1.3
        assert float(k("outlier", shape).max()) < 1.2
        x = N.by_group(N.gn_fixture("outlier", *shape), shape[3])
        assert bool(((x == 1e3).sum(1) == 1).all())
        sign = N.by_group(N.gn_fixture("offset64", *shape), shape[3]).mean(1).sign().reshape(shape[0], shape[3])
        assert torch.equal(sign[:, ::2], torch.ones_like(sign[:, ::2])) and torch.equal(sign[:, 1::2], -torch.ones_like(sign[:, 1::2]))
    # big: sum x^2 of a slot ~ 1e11, below a quarter of the documented capacity of the fixed-point slot (common.hpp: |total| < 5.5e11)
    xb = N.by_group(N.gn_fixture("big", *N.GN_BIG).double(), 32)
    sq = (xb * xb).sum(1)
    assert 5.5e11 / 5.2 < float(sq.min()) and float(sq.max()) < 5.5e11 / 4          # "a fifth" of include/mvd_hip.h
    assert float(N.gn_kappa(N.gn_fixture("big", *N.GN_BIG), 32, N.GN_EPS).max()) < 3.0
    # LayerNorm rows
    assert float((N.ln_kappa(N.ln_fixture("offset64", 37, 1280), N.LN_EPS) / 4097 - 1).abs().max()) < 0.3
    assert float(N.ln_kappa(N.ln_fixture("offset64", 37, 36), N.LN_EPS).min()) > 2000
    for fx, k in (("offset8", 65), ("offset64", 4097)):          # the backward's fixtures keep the full offset in small groups
        assert float((N.gn_kappa(N.gn_fixture(fx, 1, 16, 128, 64, full=True), 64, N.GN_EPS) / k).min()) > 0.4
    assert float(N.ln_kappa(N.ln_fixture("const", 5, 32), N.LN_EPS)[0]) == pytest.approx(3.7 ** 2 / N.LN_EPS, rel=1e-6)
    # softmax: what the name says AFTER scaling
    for (rows, cols, ldx), fx, sc in N.softmax_cases():
        x = N.softmax_fixture(fx, rows, cols, ldx, sc)
        p = N.softmax_rows(x[:, :cols], sc)
        z = x[:, :cols].double() * N.f32(sc)
        if fx == "one_hot":
            top = z.topk(2, 1).values
            assert float((top[:, 0] - top[:, 1]).min()) > 9e3 and float(p.amax(1).min()) == 1.0
        elif fx == "equal":
            assert float((p * cols - 1).abs().max()) < 1e-12
        else:
            assert float(z.abs().max()) < 12 and float(p.amax(1).max()) < 0.9
        assert ldx == cols or bool((x[:, cols:] == 3e4).all())
    # column sums: a running fp32 accumulator misses the bar in the pair's column
    for rows in (255, 16385):
        x = N.col_sum_fixture(rows, 33)
        ref = N.col_sum(x)
        acc = torch.zeros(33)
        for r in range(rows):
            acc = acc + x[r]
        assert N.worst(acc, ref, N.col_sum_bar(x, ref), 33) > 100


# ------------------------------------------------------------------------------------------------ the GroupNorm algorithm passes
def emulate_gn_fp32(x, gamma, beta, G, eps, silu):
    """gn_stats_kernel + gn_apply_kernel in float32 in the kernel's order: per (chunk, ty slice, channel) a sequential fp32 sum of x and
    x * x over the slice's rows, the TY slices added in fp32, channels of a group and chunks in fp64; mean / rstd rounded to fp32,
    a = rstd * gamma, b = beta - mean * a, y = x * a + b, SiLU in fp32."""
    B, HW, C = x.shape
    chunks, TY = N.gn_chunks(HW), N.gn_ty(C)
    rows = HW // chunks
    steps = -(-rows // TY)
    xp = torch.zeros(B, chunks, steps * TY, C)
    xp[:, :, :rows] = x.reshape(B, chunks, rows, C)
    xp = xp.reshape(B, chunks, steps, TY, C)
    s, q = torch.zeros(B, chunks, TY, C), torch.zeros(B, chunks, TY, C)
    for st in range(steps):
        v = xp[:, :, st]
        s, q = s + v, q + v * v
    ssum, qsum = s[:, :, 0], q[:, :, 0]
    for t in range(1, TY):
        ssum, qsum = ssum + s[:, :, t], qsum + q[:, :, t]
    cg, n = C // G, HW * (C // G)
    sd = ssum.double().reshape(B, chunks, G, cg).sum((1, 3))
    qd = qsum.double().reshape(B, chunks, G, cg).sum((1, 3))
    mean = sd / n
    var = (qd / n - mean * mean).clamp_min(0.0)
    rstd = (1.0 / (var + N.f32(eps)).sqrt()).float()
    full = lambda t: t.reshape(B, 1, G, 1).expand(B, 1, G, cg).reshape(B, 1, C)
    a = full(rstd) * gamma
    y = x * a + (beta - full(mean.float()) * a)
    return y * torch.sigmoid(y) if silu else y


@pytest.mark.parametrize("shape", N.GN_SHAPES + [N.GN_BIG], ids=_ids(N.GN_SHAPES + [N.GN_BIG]))
def test_fp32_emulation_stays_under_half_the_groupnorm_bar(shape):
    B, HW, C, G = shape
    gm, bt = N.gn_params(C)
    R = N.gn_accum_len(HW, C)
    for s, fx in [c for c in N.gn_cases() if c[0] == shape]:
        x = N.gn_fixture(fx, *shape)
        kappa = N.gn_kappa(x, G, N.GN_EPS)
        for silu in (False, True):
            ref = N.by_group(N.gn_forward(x, gm, bt, G, N.GN_EPS, silu), G)
            got = N.by_group(emulate_gn_fp32(x, gm, bt, G, N.GN_EPS, silu), G)
            bar = N.gn_forward_bar(kappa, N.group_max(ref, B * G), PL_F16, R)
            r = N.worst(got, ref, bar, B * G)
            print(f"emulation {shape} R={R} {fx} silu={int(silu)}: worst err / bar {r:.3f}")
            assert r <= 0.5, (shape, fx, silu, r)


# ------------------------------------------------------------------------------------------------ every mutant is rejected
def _gn_forward_kills(m):
    for (B, HW, C, G), fx in N.gn_cases():
        x, (gm, bt) = N.gn_fixture(fx, B, HW, C, G), N.gn_params(C)
        ref = N.by_group(N.gn_forward(x, gm, bt, G, N.GN_EPS), G)
        bar = N.gn_forward_bar(N.gn_kappa(x, G, N.GN_EPS), N.group_max(ref, B * G), PL_BF16, N.gn_accum_len(HW, C))
        yield ((B, HW, C, G), fx), N.worst(N.by_group(N.gn_forward(x, gm, bt, G, N.GN_EPS, mutant=m), G), ref, bar, B * G)


def _gn_backward_kills(m):
    for (B, HW, C, G), fx in N.gn_bwd_cases():
        x, (gm, bt), dy = N.gn_fixture(fx, B, HW, C, G, full=True), N.gn_params(C), N.gn_dy(B, HW, C)
        ref = N.by_group(N.gn_backward(x, dy, gm, bt, G, N.GN_EPS, True)[0], G)
        bar = N.stable_bar(5e-6, N.gn_kappa(x, G, N.GN_EPS), N.group_max(ref, B * G))
        yield ((B, HW, C, G), fx), N.worst(N.by_group(N.gn_backward(x, dy, gm, bt, G, N.GN_EPS, True, mutant=m)[0], G), ref, bar, B * G)


def _gn_param_kills(m):
    """dgamma and dbeta at the bars the GPU file applies to them (norm_f64.gn_param_bar)"""
    for (B, HW, C, G), fx in N.gn_bwd_cases():
        x, (gm, bt), dy = N.gn_fixture(fx, B, HW, C, G, full=True), N.gn_params(C), N.gn_dy(B, HW, C)
        _, rdg, rdb, adg, adb, shb = N.gn_backward(x, dy, gm, bt, G, N.GN_EPS, True, with_abs=True)
        _, mdg, mdb = N.gn_backward(x, dy, gm, bt, G, N.GN_EPS, True, mutant=m)
        kg = N.gn_kappa(x, G, N.GN_EPS).reshape(B, G).amax(0)
        yield ((B, HW, C, G), fx), min(N.worst(mdg, rdg, N.gn_param_bar(rdg, kg, G, adg, adb), C), N.worst(mdb, rdb, N.gn_param_bar(rdb, kg, G, adb, shb), C))


def _ln_dw_kills(m):
    """dw and db at the bars the GPU file applies to them (norm_f64.ln_dw_bar; 2e-6 max|db| of the group)"""
    for rows, C, rpg in N.ln_bwd_cases():
        rpg = rpg or rows
        w = N.ln_params(rows // rpg, C, 6 if rpg != rows else 1)[0]
        dy = N.gn_dy(1, rows, C)[0]
        for fx in N.LN_FIXTURES:
            x = N.ln_fixture(fx, rows, C)
            _, dw, db = N.ln_backward(x, dy, w, N.LN_EPS, rpg)
            _, mw, mb = N.ln_backward(x, dy, w, N.LN_EPS, rpg, mutant=m)
            ng = rows // rpg
            yield ((rows, C, rpg), fx), min(N.worst(mw, dw, N.ln_dw_bar(x, dy, dw, N.LN_EPS, rpg), ng * C),
                                            N.worst(mb, db, 2e-6 * N.group_max(db, ng), ng))


def _ln_kills(m):
    for rows, C, rpg, wp1 in N.ln_cases():
        w, b = N.ln_params(rows // rpg if rpg else 1, C, 6 if rpg else 1)
        for fx in N.LN_FIXTURES:
            x = N.ln_fixture(fx, rows, C)
            ref = N.ln_forward(x, w, b, N.LN_EPS, wp1, rpg or None)
            bar = N.stable_bar(PL_BF16 + 3e-6, N.ln_kappa(x, N.LN_EPS), N.group_max(ref, rows))
            yield ((rows, C, rpg, wp1), fx), N.worst(N.ln_forward(x, w, b, N.LN_EPS, wp1, rpg or None, mutant=m), ref, bar, rows)


def _ln_backward_kills(m):
    for rows, C, rpg in N.ln_bwd_cases():
        w = N.ln_params(rows // rpg if rpg else 1, C, 6 if rpg else 1)[0]
        dy = N.gn_dy(1, rows, C)[0]
        for fx in N.LN_FIXTURES:
            x = N.ln_fixture(fx, rows, C)
            ref = N.ln_backward(x, dy, w, N.LN_EPS, rpg or None)[0]
            bar = N.stable_bar(5e-6, N.ln_kappa(x, N.LN_EPS), N.group_max(ref, rows))
            yield ((rows, C, rpg), fx), N.worst(N.ln_backward(x, dy, w, N.LN_EPS, rpg or None, mutant=m)[0], ref, bar, rows)


def _softmax_kills(m):
    for (rows, cols, ldx), fx, sc in N.softmax_cases():
        x = N.softmax_fixture(fx, rows, cols, ldx, sc)[:, :cols]
        ref = N.softmax_rows(x, sc)
        yield ((rows, cols, ldx), fx, sc), N.worst(N.softmax_rows(x, sc, mutant=m), ref, (2e-6 + PL_BF16) * N.group_max(ref, rows), rows)


def _col_sum_kills(m):
    for rows in N.COL_SUM_ROWS:
        for cols in N.COL_SUM_COLS:
            x = N.col_sum_fixture(rows, cols)
            ref = N.col_sum(x)
            yield (rows, cols), N.worst(N.col_sum(x, mutant=m), ref, N.col_sum_bar(x, ref), cols)
    for ng, rpg in N.COL_SUM_GROUPS:
        x = N.col_sum_fixture(ng * rpg, 33)
        ref = N.col_sum(x, ng)
        yield (ng, rpg), N.worst(N.col_sum(x, ng, mutant=m), ref, N.col_sum_bar(x, ref, ng), ng * 33)


def _act_backward_kills(m):
    for rows, cols in N.ELEMENTWISE_SHAPES + [N.ACT_BIG]:
        x, dy = N.value_grid(rows, cols, "x"), N.value_grid(rows, cols, "dy")
        ref = N.act_backward(dy, x, N.ACT_SILU)
        yield (rows, cols), N.worst(N.act_backward(dy, x, N.ACT_SILU, mutant=m), ref, N.elementwise_bar(ref, dy.abs()) + 1e-300, rows * cols)


KILLERS = {
    "eps_outside_sqrt": [_gn_forward_kills], "var_n_minus_1": [_gn_forward_kills], "per_channel_stats": [_gn_forward_kills],
    "batch_shared_stats": [_gn_forward_kills], "silu_grad_no_z_term": [_gn_backward_kills, _act_backward_kills],
    "no_gamma_in_ds_db": [_gn_backward_kills], "inv_n_of_32_groups": [_gn_backward_kills], "ignore_w_plus_one": [_ln_kills],
    "group_row_by_block": [_ln_kills, _ln_backward_kills], "param_sum_skips_last_image": [_gn_param_kills],
    "dw_drops_group_last_row": [_ln_dw_kills], "drop_last_row_of_split": [_col_sum_kills], "scale_after_max": [_softmax_kills],
}


def test_every_mutant_has_a_killer():
    assert sorted(KILLERS) == sorted(N.MUTANTS)


@pytest.mark.parametrize("mutant", N.MUTANTS)
def test_mutant_is_rejected_by_the_gpu_case_list(mutant):
    """In EVERY family the mutant applies to, at least one (fixture, shape) of the GPU file's own list exceeds its bar."""
    for family in KILLERS[mutant]:
        results = list(family(mutant))
        killed = [(c, r) for c, r in results if r > 1.0]
        print(f"{mutant} / {family.__name__}: rejected by {len(killed)} of {len(results)} cases, e.g. {killed[:2]}")
        assert killed, (mutant, family.__name__)
