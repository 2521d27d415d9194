"""tests/attention_f64.py on the CPU: the oracles against independent torch float64 statements, the conditions the fixtures promise,
and the proof that the acceptance rule has teeth -- deliberately wrong references are rejected, a float32 emulation of the kernel's
own split-operand algorithm is accepted, both at the bar of the four-product precision in the fp16 flavour (2 * 2e-6 + 1e-6 of the
group's max|v|: tests/test_gpu_ops.py TOL[4], PL), the tightest one the GPU file applies."""
import math

import pytest
import torch
import torch.nn.functional as F

import attention_f64 as A

TOL_X4 = 2 * 2e-6 + 1e-6          # 2 * TOL[4] + PL of tests/test_gpu_ops.py, fp16 flavour
TOL_VALU = 1e-6 + 2e-6            # PL + 2e-6
ALL_SELF = [c[:5] for c in A.ONE_TILE_CASES] + A.TWO_TILE_CASES


def _ids(cases):
    return ["-".join(map(str, c)) for c in cases]


# ------------------------------------------------------------------------------------------------ oracles
@pytest.mark.parametrize("B,H,L,Lk,d", [(2, 3, 20, 17, 12), (1, 2, 68, 64, 32), (2, 2, 37, 0, 40)])
def test_self_attention_oracle_equals_sdpa(B, H, L, Lk, d):
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(B * L, H * d, generator=g, dtype=torch.float64) for _ in range(3))
    out, scale = A.self_attention(q, k, v, B, H, L, d, Lk)
    mask = (torch.arange(L) < (Lk or L)).expand(L, L)
    qh, kh, vh = (A.heads_first(t, B, H, L, d) for t in (q, k, v))
    want = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask).permute(0, 2, 1, 3).reshape(B * L, H * d)
    assert float((out - want).abs().max()) < 1e-13
    assert torch.equal(scale, vh[:, :, :Lk or L].abs().amax((2, 3)).reshape(-1))


def test_valu_oracles_equal_direct_statements():
    g = torch.Generator().manual_seed(2)
    P, D, H, d = 7, 3, 2, 12
    q, k, v = (torch.randn(n, H * d, generator=g, dtype=torch.float64) for n in (P, P * D, P * D))
    out, scale = A.pixel_cross_attention(q, k, v, P, D, H, d)
    for p in range(P):
        for h in range(H):
            sl = slice(h * d, (h + 1) * d)
            w = torch.softmax(k[p * D:(p + 1) * D, sl] @ q[p, sl] / math.sqrt(d), 0)
            assert float((out[p, sl] - w @ v[p * D:(p + 1) * D, sl]).abs().max()) < 1e-13
        assert float(scale[p]) == float(v[p * D:(p + 1) * D].abs().max())
    N, V, H, d = 5, 3, 2, 8
    C = H * d
    qkv = torch.randn(N * V, 3 * C, generator=g, dtype=torch.float64)
    out, scale = A.view_mha(qkv, N, V, H, d)
    t = qkv.view(N, V, 3, H, d).permute(2, 0, 3, 1, 4)          # the statement of tests/test_gpu_ops.py::test_view_mha_and_pool
    want = (((t[0] * d ** -0.5) @ t[1].transpose(-2, -1)).softmax(-1) @ t[2]).transpose(1, 2).reshape(N * V, C)
    assert float((out - want).abs().max()) < 1e-13
    assert torch.equal(scale, qkv.view(N, V, 3, C)[:, :, 2].abs().amax((1, 2)))
    x = torch.randn(N, V, C, generator=g, dtype=torch.float64)
    w, b = torch.randn(1, C, generator=g, dtype=torch.float64), torch.randn(1, generator=g, dtype=torch.float64)
    out, scale = A.view_pool(x.view(N * V, C), w, b, N, V, C)
    want = (x * F.linear(x, w, b).softmax(dim=-2)).sum(-2)
    assert float((out - want).abs().max()) < 1e-13 and torch.equal(scale, x.abs().amax((1, 2)))


def test_accept_is_per_group():
    ref = torch.zeros(3, 4, 2, dtype=torch.float64)
    got = ref.clone()
    got[1, 2, 0] = 1e-3
    got[2, 0, 1] = float("nan")
    r = A.accept(got, ref, torch.tensor([1.0, 10.0, 1.0]), 1e-3)
    assert float(r[0]) == 0.0 and abs(float(r[1]) - 0.1) < 1e-12 and math.isinf(float(r[2]))


# ------------------------------------------------------------------------------------------------ fixture conditions
MASKED_SELF = [c for c in ALL_SELF if 0 < c[3] < c[2]]


@pytest.mark.parametrize("case", MASKED_SELF, ids=_ids(MASKED_SELF))
def test_masked_fixture_conditions(case):
    B, H, L, Lk, d = case
    # one_hot: every key in [0, Lk) wins, with p >= 0.5, for at least one query
    q, k, v, ref, scale = A.self_case("one_hot", *case)
    qh, kh = (A.heads_first(t.double(), B, H, L, d) for t in (q, k))
    p = torch.softmax(qh @ kh[:, :, :Lk].transpose(-1, -2) / math.sqrt(d), -1)              # (B, H, L, Lk)
    assert float(p.amax(2).min()) >= 0.5, float(p.amax(2).min())
    # sentinel: key Lk alone moves every query row by more than 100 x the widest tolerance any flavour applies to it
    q, k, v, ref, scale = A.self_case("sentinel", *case)
    moved, _ = A.self_attention(q, k, v, B, H, L, d, Lk + 1)
    shift = A.by_head((moved - ref).abs(), B, H, L, d).amax(-1)                             # (B*H, L)
    for tol in (TOL_X4, 2 * 3e-3 + 1e-6, 2 * 2e-2 + 2e-5):                                 # x4 fp16; one product fp16; one product bf16
        assert bool((shift > 100 * tol * scale[:, None]).all()), (tol, float((shift / (tol * scale[:, None])).min()))


def _logits_pixel(q, k, P, D, H, d):
    return (k.double().view(P, D, H, d) * q.double().view(P, 1, H, d)).sum(-1) / math.sqrt(d)        # (P, D, H)


def test_large_logit_fixture_conditions():
    def check(lg, axis):          # winner leads by >= 30 nats; some logit beyond 100 in magnitude
        top = lg.topk(min(2, lg.shape[axis]), dim=axis).values
        if lg.shape[axis] > 1:
            lead = top.select(axis, 0) - top.select(axis, 1)
            assert float(lead.min()) >= 30.0, float(lead.min())
        assert float(lg.abs().max()) > 100.0
    for P, D, H, d in A.PIXEL_CASES:
        q, k, v = A.pixel_fixture("large", P, D, H, d)
        check(_logits_pixel(q, k, P, D, H, d), 1)
    for N, V, H, d in [(n, v, 8, 32) for n, v in A.VIEW_MHA_FAST_CASES] + A.VIEW_MHA_GENERIC_CASES:
        t = A.view_mha_fixture("large", N, V, H, d).double().view(N, V, 3, H, d).permute(2, 0, 3, 1, 4)
        check(t[0] @ t[1].transpose(-1, -2) / math.sqrt(d), -1)
    for N, V, C in A.VIEW_POOL_CASES:
        x, w, b = A.view_pool_fixture("large", N, V, C)
        check(x.double().view(N, V, C) @ w.double().view(C) + b.double(), 1)


# ------------------------------------------------------------------------------------------------ wrong references
def _wrong_lk(delta):
    def f(q, k, v, B, H, L, Lk, d):
        kk = (Lk or L) + delta
        return A.self_attention(q, k, v, B, H, L, d, kk)[0] if 0 < kk <= L else None
    return f


def _wrong_v_slot(q, k, v, B, H, L, Lk, d):
    """two key positions of V swapped inside one 32-key half-tile (the last two keys that take part)"""
    kk = Lk or L
    a, b = kk - 1, kk - 2
    if b < 0 or a // 32 != b // 32:
        return None
    v2 = v.clone().view(B, L, H * d)
    v2[:, [a, b]] = v2[:, [b, a]]
    return A.self_attention(q, k, v2.view(B * L, H * d), B, H, L, d, Lk)[0]


def _wrong_head_v(q, k, v, B, H, L, Lk, d):
    """head h reads the values of head h + 1"""
    if H == 1:
        return None
    return A.self_attention(q, k, v.view(B * L, H, d).roll(-1, 1).reshape(B * L, H * d), B, H, L, d, Lk)[0]


def _wrong_scale(q, k, v, B, H, L, Lk, d):
    """roundup(d, 16)^-0.5 in place of d^-0.5"""
    if d % 16 == 0 or Lk == 1:             # (a single key: no logit matters)
        return None
    return A.self_attention(q * math.sqrt(d / A.dpad(d)), k, v, B, H, L, d, Lk)[0]


def _wrong_pad_channels(q, k, v, B, H, L, Lk, d):
    """channels [dhead, dpad) of a K row taken from the next head instead of the zero padding.  (The products see them through the same
    channels of the q row; with those at zero a wrong K alone changes nothing, so the q row reads on in the same way.)"""
    n = A.dpad(d) - d
    if n == 0 or H == 1 or Lk == 1:        # (a single key: no logit matters)
        return None
    nxt = ((torch.arange(H)[:, None] + 1) * d + torch.arange(n)[None, :]) % (H * d)         # the n channels behind head h's own (wrapping)
    ext = lambda t: torch.cat([t.view(B * L, H, d), t[:, nxt]], 2).reshape(B * L, H * (d + n))
    v2 = torch.cat([v.view(B * L, H, d), torch.zeros(B * L, H, n)], 2).reshape(B * L, H * (d + n))
    out = A.self_attention(ext(q) * math.sqrt((d + n) / d), ext(k), v2, B, H, L, d + n, Lk)[0]
    return out.view(B * L, H, d + n)[:, :, :d].reshape(B * L, H * d)


def _wrong_batch_stride(q, k, v, B, H, L, Lk, d):
    """batch item b stores its rows from b * Lpad instead of b * L; rows nobody wrote keep a NaN"""
    if B == 1 or A.lpad(L) == L:
        return None
    ref = A.self_attention(q, k, v, B, H, L, d, Lk)[0]
    out = torch.full((B * A.lpad(L), H * d), float("nan"), dtype=torch.float64)
    for b in range(B):
        out[b * A.lpad(L):b * A.lpad(L) + L] = ref[b * L:(b + 1) * L]
    return out[:B * L]


WRONG = {"Lk+1": _wrong_lk(1), "Lk-1": _wrong_lk(-1), "v_slot": _wrong_v_slot, "head_v": _wrong_head_v, "scale": _wrong_scale,
         "pad_channels": _wrong_pad_channels, "batch_stride": _wrong_batch_stride}


@pytest.mark.parametrize("name", sorted(WRONG))
def test_wrong_reference_is_rejected(name):
    """Over the fixtures of the one-tile case list: every wrong reference is rejected on at least one -- and here on EVERY fixture it
    applies to and can show on: a one-hot fixture cannot see a changed softmax scale or a few more channels under the dot product
    (the winner still wins); those are what the sentinel and diffuse fixtures are for."""
    blind = {("scale", "one_hot"), ("pad_channels", "one_hot")}
    rejected, applied = 0, 0
    for case in A.ONE_TILE_CASES:
        B, H, L, Lk, d = case[:5]
        for fx in A.fixtures_for(L, Lk):
            q, k, v, ref, scale = A.self_case(fx, B, H, L, Lk, d)
            got = WRONG[name](q, k, v, B, H, L, Lk, d)
            if got is None:
                continue
            applied += 1
            worst = float(A.accept(A.by_head(got, B, H, L, d), A.by_head(ref, B, H, L, d), scale, TOL_X4).max())
            if (name, fx) not in blind:
                assert worst > 1.0, (name, case, fx, worst)
            rejected += worst > 1.0
    assert applied >= 2 and rejected >= 1, (name, applied, rejected)


# ------------------------------------------------------------------------------------------------ the algorithm itself passes
def _split16(x):
    hi = x.half().float()
    return hi + (x - hi).half().float()


def _emulate(q, k, v, B, H, L, Lk, d):
    """float32 emulation of attn_kernel in the four-product fp16 flavour: operands = fp16 hi + lo (q pre-scaled by d^-0.5 log2 e), base-2
    softmax over the keys [0, Lk), P split before P V, the output stored as split planes."""
    Lk = Lk or L
    qh, kh, vh = (A.heads_first(t, B, H, L, d) for t in (q, k, v))
    qs, ks, vs = _split16(qh * (d ** -0.5 * 1.4426950408889634)), _split16(kh)[:, :, :Lk], _split16(vh)[:, :, :Lk]
    s = qs @ ks.transpose(-1, -2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    out = (_split16(p) @ vs) / p.sum(-1, keepdim=True)
    return _split16(out).permute(0, 2, 1, 3).reshape(B * L, H * d)


@pytest.mark.parametrize("case", ALL_SELF, ids=_ids(ALL_SELF))
def test_split_operand_emulation_is_accepted(case):
    B, H, L, Lk, d = case
    for fx in A.fixtures_for(L, Lk):
        q, k, v, ref, scale = A.self_case(fx, *case)
        got = _emulate(q, k, v, B, H, L, Lk, d)
        worst = float(A.accept(A.by_head(got, B, H, L, d), A.by_head(ref, B, H, L, d), scale, TOL_X4).max())
        print(f"emulation {case} {fx}: worst err / bar {worst:.3f}")
        assert worst <= 1.0, (case, fx, worst)
