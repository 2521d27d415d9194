"""The attention family of csrc/attention.hip against FLOAT64 (tests/attention_f64.py) at ragged and edge shapes, through the C ABI,
into sentinel-filled outputs with four spare rows behind the result.

Acceptance (attention_f64.accept): per (batch, head)  |got - ref| <= (2 TOL[prec] + PL) max|v| over the keys that take part for
mvd_attention, per pixel / sequence  |got - ref| <= (PL + 2e-6) max|v|  for the fp32 kernels -- the bars of tests/test_gpu_ops.py, applied
per group.  Every test prints the worst ratio error / bar of its case (pytest -s shows them).

Operand planes come from the QKV GEMM with an identity weight (q, k, v are then the fixture itself to the precision of the split), except
for heads * dhead % 32 != 0 (57 x 3 x 80), which that GEMM refuses: there the planes are packed on the host (host_planes, itself checked
against the GEMM's planes).

Measured on an MI355X, worst error / bar of a family over its cases, fixtures and precisions (the bar allows 1):
                                             | fp16 flavour | bf16 flavour
  one-tile kernel, diffuse                   |        0.094 |        0.099      (1,3,132,0,160)
  one-tile kernel, one_hot                   |        0.077 |        0.143
  one-tile kernel, sentinel                  |        0.022 |        0.079
  two-tile kernel = forced one-tile, one_hot |        0.388 |        0.552      (64,8,20,17,4: x1 | x3; the other cases <= 0.150)
  two-tile kernel = forced one-tile, sentinel|        0.024 |        0.039
  pixel_cross_attn                           |        0.052 |        0.319
  view_mha, templated kernel                 |        0.145 |        0.314
  view_mha, generic kernel                   |        0.123 |        0.329
  view_pool                                  |        0.124 |        0.341
The CPU emulation of the split-operand algorithm (tests/test_cpu_attention_f64.py) gives 0.01 .. 0.14 on the same fixtures.  The
bf16 figures of the fp32 kernels are the split-plane rounding of the stored result, which PL is there for.
"""
import math
import os

import pytest
import torch

import attention_f64 as A
from conftest import planes_to_float, rel_err
from test_gpu_ops import PL, TOL

pytestmark = pytest.mark.gpu

SENT = 0x5A5A          # every 16-bit word of an output before the call
LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


@pytest.fixture(scope="module")
def ws():
    return torch.empty(8 * 1024 * 1024, device="cuda")


def _ids(cases):
    return ["-".join(str(int(x)) for x in c) for c in cases]


# ------------------------------------------------------------------------------------------------ operand planes and outputs
def _enc(hip, x):
    """fp32 -> (hi, lo) 16-bit planes of the operand format (round to nearest even, as csrc/common.hpp split_op16)"""
    t = torch.bfloat16 if hip.OPERAND_FORMAT == "bf16" else torch.float16
    hi = x.to(t)
    lo = (x - hi.float()).to(t)
    return hi.view(torch.int16), lo.view(torch.int16)


def _dec(hip, hi, lo):
    t = torch.bfloat16 if hip.OPERAND_FORMAT == "bf16" else torch.float16
    return hi.view(t).float() + lo.view(t).float()


def host_planes(hip, q, k, v, B, H, L, d):
    """The six operand planes of include/mvd_hip.h packed on the host: q / k [B][H][Lpad][dpad] (q scaled by d^-0.5 log2 e in fp32),
    vt [B][H][dpad][Lpad], zero padded."""
    Lp, dp = A.lpad(L), A.dpad(d)
    qs = A.heads_first(q, B, H, L, d) * torch.tensor(d ** -0.5 * LOG2E, dtype=torch.float32)
    out = []
    for x in (qs, A.heads_first(k, B, H, L, d)):
        p = torch.zeros(B, H, Lp, dp)
        p[:, :, :L, :d] = x
        out += [t.reshape(-1) for t in _enc(hip, p)]
    p = torch.zeros(B, H, dp, Lp)
    p[:, :, :d, :L] = A.heads_first(v, B, H, L, d).transpose(-1, -2)
    out += [t.reshape(-1) for t in _enc(hip, p)]
    return tuple(t.cuda() for t in out)


def gemm_planes(hip, ws, q, k, v, B, H, L, d):
    """The planes as the library itself produces them: [q | k | v] rows through the QKV routing epilogue with an identity weight."""
    C = H * d
    planes = hip.alloc_attn_planes(B, H, L, d, "cuda")
    Wp = hip.pack_linear(torch.eye(3 * C, device="cuda"))
    hip.gemm(hip.split_planes(torch.cat([q, k, v], 1).cuda()), Wp, None, prec=4, epi=hip.EPI_QKV,
             qkv=dict(planes=planes, heads=H, dhead=d, L=L), workspace=ws)
    return planes


def make_planes(hip, ws, q, k, v, B, H, L, d):
    if (H * d) % 32 == 0:
        return gemm_planes(hip, ws, q, k, v, B, H, L, d)
    planes = hip.alloc_attn_planes(B, H, L, d, "cuda")
    for dst, src in zip(planes, host_planes(hip, q, k, v, B, H, L, d)):
        assert dst.shape == src.shape
        dst.copy_(src)
    return planes


def sentinel_out(rows, ld):
    return torch.full((rows + 4, 2 * ld), SENT, dtype=torch.int16, device="cuda")


def read_out(raw, rows, C):
    """The spare rows and the columns [C, ld) must keep their bits; -> the (rows, C) result."""
    raw = raw.cpu()
    ld = raw.shape[1] // 2
    assert bool((raw[rows:] == SENT).all()), "rows behind the result were written"
    if ld > C:
        cols = raw[:rows].view(rows, ld // 32, 2, 32).permute(0, 2, 1, 3).reshape(rows, 2, ld)
        assert bool((cols[:, :, C:] == SENT).all()), "columns behind the result were written"
    return planes_to_float(raw[:rows])[:, :C]


def run_attention(hip, planes, B, H, L, Lk, d, prec, force_one_tile=False):
    C = H * d
    out = sentinel_out(B * L, (C + 31) // 32 * 32)
    if force_one_tile:
        os.environ["MVD_ATTN_QT1"] = "1"
    try:
        hip.attention(planes, out, B, H, L, d, prec=prec, Lkeys=Lk)
        torch.cuda.synchronize()
    finally:
        os.environ.pop("MVD_ATTN_QT1", None)
    return out.cpu()


def worst_ratio(got, ref, scale, B, H, L, d, tol):
    return float(A.accept(A.by_head(got, B, H, L, d), A.by_head(ref, B, H, L, d), scale, tol).max())


def two_tile_workgroups(B, H, L):
    return (A.lpad(L) + 127) // 128 * H * B


# ------------------------------------------------------------------------------------------------ self-attention
def test_host_planes_match_the_qkv_gemm(hip, ws):
    """host_planes (used where the QKV GEMM refuses the shape) against the planes the GEMM writes: equal to the precision of the split,
    padding exactly zero in both."""
    B, H, L, Lk, d = 2, 8, 20, 17, 12
    q, k, v, _, _ = A.self_case("sentinel", B, H, L, Lk, d)
    a, b = gemm_planes(hip, ws, q, k, v, B, H, L, d), host_planes(hip, q, k, v, B, H, L, d)
    for i in range(3):
        fa, fb = _dec(hip, a[2 * i].cpu(), a[2 * i + 1].cpu()), _dec(hip, b[2 * i].cpu(), b[2 * i + 1].cpu())
        assert rel_err(fa, fb) < 2 * PL, i
        assert torch.equal(fa == 0, fb == 0), i


ONE_TILE = [c[:5] + (p,) for c in A.ONE_TILE_CASES for p in ((4, 3, 1) if c[5] else (4,))]


@pytest.mark.parametrize("B,H,L,Lk,d,prec", ONE_TILE, ids=_ids(ONE_TILE))
def test_attention_one_tile_kernel(hip, ws, B, H, L, Lk, d, prec):
    assert two_tile_workgroups(B, H, L) < 512
    for fx in A.fixtures_for(L, Lk):
        q, k, v, ref, scale = A.self_case(fx, B, H, L, Lk, d)
        planes = make_planes(hip, ws, q, k, v, B, H, L, d)
        got = read_out(run_attention(hip, planes, B, H, L, Lk, d, prec), B * L, H * d)
        r = worst_ratio(got, ref, scale, B, H, L, d, 2 * TOL[prec] + PL)
        print(f"RATIO one-tile {B},{H},{L},{Lk},{d} x{prec} {fx}: {r:.3f}")
        assert r <= 1.0, (fx, r)


@pytest.mark.parametrize("B,H,L,Lk,d", A.TWO_TILE_CASES, ids=_ids(A.TWO_TILE_CASES))
def test_attention_two_tile_kernel(hip, ws, B, H, L, Lk, d):
    """As dispatched (two query tiles per wavefront) and with MVD_ATTN_QT1=1: both against float64, and against each other as
    tests/test_gpu_ops.py::test_attention_phased_equals_single_tile demands."""
    assert two_tile_workgroups(B, H, L) >= 512
    for fx in A.fixtures_for(L, Lk):
        q, k, v, ref, scale = A.self_case(fx, B, H, L, Lk, d)
        planes = make_planes(hip, ws, q, k, v, B, H, L, d)
        for prec in (4, 3, 1):
            raws = [run_attention(hip, planes, B, H, L, Lk, d, prec, force_one_tile=f) for f in (False, True)]
            gots = [read_out(raw, B * L, H * d) for raw in raws]
            for which, got in zip(("two-tile", "forced one-tile"), gots):
                r = worst_ratio(got, ref, scale, B, H, L, d, 2 * TOL[prec] + PL)
                print(f"RATIO {which} {B},{H},{L},{Lk},{d} x{prec} {fx}: {r:.3f}")
                assert r <= 1.0, (which, fx, prec, r)
            if prec >= 3:
                assert torch.equal(raws[0], raws[1]), (fx, prec)
            else:
                assert rel_err(gots[0], gots[1]) < TOL[1], fx


@pytest.mark.parametrize("B,H,L,Lk,d", [(2, 8, 68, 65, 36), (2, 8, 68, 65, 68), (64, 8, 20, 17, 4)],
                         ids=["two_buffers_one_tile", "one_buffer_one_tile", "two_buffers_two_tiles"])
def test_attention_ignores_the_padding_rows(hip, ws, B, H, L, Lk, d):
    """Key rows / V^T columns [Lkeys, Lpad) and query rows [L, Lpad) filled with large finite values: the output keeps its bits (masked
    scores are -inf, their P is exactly 0, and the query rows behind L are never stored).  Channels [dhead, dpad) of q and k are zero
    as the GEMM leaves them -- the part of the padding the kernel relies on."""
    Lp, dp = A.lpad(L), A.dpad(d)
    q, k, v, ref, scale = A.self_case("sentinel", B, H, L, Lk, d)
    planes = make_planes(hip, ws, q, k, v, B, H, L, d)
    before = {prec: run_attention(hip, planes, B, H, L, Lk, d, prec) for prec in (4, 3, 1)}
    big = [t.item() for t in _enc(hip, torch.tensor([3.0e4, -5.0]))[0]]                  # hi planes 3e4, lo planes -5
    for i, p in enumerate(planes):
        fill = big[i % 2]
        if i < 4:
            t = p.view(B, H, Lp, dp)
            assert bool((t[..., d:] == 0).all())
            t[:, :, (L if i < 2 else Lk):, :d] = fill
        else:
            p.view(B, H, dp, Lp)[:, :, :d, Lk:] = fill
    for prec in (4, 3, 1):
        after = run_attention(hip, planes, B, H, L, Lk, d, prec)
        assert torch.equal(before[prec], after), prec
    r = worst_ratio(read_out(before[4], B * L, H * d), ref, scale, B, H, L, d, 2 * TOL[4] + PL)
    assert r <= 1.0, r


# ------------------------------------------------------------------------------------------------ refusals
def _refused(hip, rc, entry):
    assert rc != 0
    msg = hip.lib().mvd_last_error().decode()
    assert msg.startswith(entry + ":"), msg
    return msg


def _attention_rc(hip, planes, out, ldo, B, H, L, Lk, d, prec=4):
    return hip.lib().mvd_attention(*[hip.ptr(p) for p in planes], hip.ptr(out), ldo, B, H, L, Lk, d, prec, hip.stream())


@pytest.mark.parametrize("d", [84, 96, 100, 144, 164])
def test_attention_refuses_unserved_head_widths(hip, d):
    B, H, L = 1, 8, 8
    planes = hip.alloc_attn_planes(B, H, L, d, "cuda")
    out = sentinel_out(B * L, H * d)
    msg = _refused(hip, _attention_rc(hip, planes, out, H * d, B, H, L, 0, d), "mvd_attention")
    assert "16, 32, 48, 64, 80, 160" in msg, msg
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


def test_attention_refuses_bad_arguments(hip):
    B, H, L, d = 1, 8, 8, 32
    planes = hip.alloc_attn_planes(B, H, L, 40, "cuda")
    out = sentinel_out(B * L, 512)
    _refused(hip, _attention_rc(hip, planes, out, 8 * 34, B, H, L, 0, 34), "mvd_attention")           # dhead % 4 != 0
    _refused(hip, _attention_rc(hip, planes, out, H * d, B, H, L, L + 1, d), "mvd_attention")          # Lkeys > L
    _refused(hip, _attention_rc(hip, planes, out, H * d + 16, B, H, L, 0, d), "mvd_attention")         # ldo % 32 != 0
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


def test_valu_entries_refuse_bad_arguments(hip):
    x = torch.zeros(1 << 16, device="cuda")
    out = sentinel_out(64, 512)
    lib, p, s = hip.lib(), hip.ptr, hip.stream()
    _refused(hip, lib.mvd_pixel_cross_attn(p(x), p(x), p(x), p(out), 4, 9, 8, 4, s), "mvd_pixel_cross_attn")      # D = 9
    _refused(hip, lib.mvd_pixel_cross_attn(p(x), p(x), p(x), p(out), 4, 2, 3, 24, s), "mvd_pixel_cross_attn")     # heads * dhead = 72
    _refused(hip, lib.mvd_view_mha(p(x), p(out), 2, 17, 8, 4, s), "mvd_view_mha")                                 # V = 17
    _refused(hip, lib.mvd_view_mha(p(x), p(out), 2, 4, 3, 24, s), "mvd_view_mha")
    _refused(hip, lib.mvd_view_pool(p(x), p(x), p(x), p(out), 2, 17, 32, s), "mvd_view_pool")
    _refused(hip, lib.mvd_view_pool(p(x), p(x), p(x), p(out), 2, 4, 72, s), "mvd_view_pool")
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


@pytest.mark.parametrize("H,d", [(3, 24), (2, 24)])
def test_qkv_gemm_refuses_heads_times_dhead_off_32(hip, ws, H, d):
    """MVD_EPI_QKV routes whole 32-column blocks to q, k or v: with heads * dhead = 72 or 48 a block straddles a boundary, so the shape
    is refused before anything is launched (with 48, N = 144 passes every other argument check)."""
    B, L = 2, 8
    C = H * d
    planes = [torch.full_like(t, SENT) for t in hip.alloc_attn_planes(B, H, L, d, "cuda")]
    Wp = hip.pack_linear(torch.eye(3 * C, device="cuda"))
    xp = hip.split_planes(torch.randn(B * L, 3 * C, generator=torch.Generator().manual_seed(3)).cuda())
    with pytest.raises(RuntimeError, match=r"mvd_gemm: QKV needs heads\*dhead % 32 == 0"):
        hip.gemm(xp, Wp, None, prec=4, epi=hip.EPI_QKV, qkv=dict(planes=planes, heads=H, dhead=d, L=L), workspace=ws)
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in planes)


# ------------------------------------------------------------------------------------------------ the fp32 kernels
VALU_TOL = PL + 2e-6


def _check_valu(name, case, fx, raw, ref, scale, groups):
    rows, C = ref.shape
    got = read_out(raw, rows, C)
    r = float(A.accept(A.by_rows(got, groups), A.by_rows(ref, groups), scale, VALU_TOL).max())
    print(f"RATIO {name} {case} {fx}: {r:.3f}")
    assert r <= 1.0, (name, case, fx, r)


@pytest.mark.parametrize("P,D,H,d", A.PIXEL_CASES, ids=_ids(A.PIXEL_CASES))
def test_pixel_cross_attn(hip, P, D, H, d):
    for fx in ("diffuse", "large"):
        q, k, v = A.pixel_fixture(fx, P, D, H, d)
        ref, scale = A.pixel_cross_attention(q, k, v, P, D, H, d)
        out = sentinel_out(P, H * d)
        qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
        hip.check(hip.lib().mvd_pixel_cross_attn(hip.ptr(qc), hip.ptr(kc), hip.ptr(vc), hip.ptr(out), P, D, H, d, hip.stream()))
        torch.cuda.synchronize()
        _check_valu("pixel_cross_attn", (P, D, H, d), fx, out, ref, scale, P)


def _run_view_mha(hip, qkv, N, V, H, d, offset=False):
    out = sentinel_out(N * V, H * d)
    buf = torch.empty(qkv.numel() + 4, device="cuda")
    dev = buf[1:1 + qkv.numel()] if offset else buf[:qkv.numel()]          # offset: 4 bytes off the 16-byte alignment
    dev.copy_(qkv.reshape(-1))
    assert (dev.data_ptr() % 16 == 4) == offset
    hip.check(hip.lib().mvd_view_mha(hip.ptr(dev), hip.ptr(out), N, V, H, d, hip.stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("N,V", A.VIEW_MHA_FAST_CASES, ids=_ids(A.VIEW_MHA_FAST_CASES))
def test_view_mha_templated_kernel(hip, N, V):
    H, d = 8, 32
    for fx in ("diffuse", "large"):
        qkv = A.view_mha_fixture(fx, N, V, H, d)
        ref, scale = A.view_mha(qkv, N, V, H, d)
        _check_valu("view_mha", (N, V, H, d), fx, _run_view_mha(hip, qkv, N, V, H, d), ref, scale, N)


_GENERIC = A.VIEW_MHA_GENERIC_CASES + [(5, 4, 8, 32), A.VIEW_MHA_GRID_STRIDE_CASE]


@pytest.mark.parametrize("N,V,H,d", _GENERIC, ids=_ids(_GENERIC))
def test_view_mha_generic_kernel(hip, N, V, H, d):
    """V outside {2, 3, 4, 8}, heads x dhead other than 8 x 32, the templated shape behind a pointer that is not 16-byte aligned, and
    more work items than one pass of the grid-stride loop."""
    offset = (V, H, d) == (4, 8, 32)
    for fx in ("diffuse", "large"):
        qkv = A.view_mha_fixture(fx, N, V, H, d)
        ref, scale = A.view_mha(qkv, N, V, H, d)
        _check_valu("view_mha generic", (N, V, H, d), fx, _run_view_mha(hip, qkv, N, V, H, d, offset), ref, scale, N)


@pytest.mark.parametrize("N,V,C", A.VIEW_POOL_CASES, ids=_ids(A.VIEW_POOL_CASES))
def test_view_pool(hip, N, V, C):
    for fx in ("diffuse", "large"):
        x, w, b = A.view_pool_fixture(fx, N, V, C)
        ref, scale = A.view_pool(x, w, b, N, V, C)
        out = sentinel_out(N, C)
        xc, wc, bc = x.cuda(), w.cuda(), b.cuda()
        hip.check(hip.lib().mvd_view_pool(hip.ptr(xc), hip.ptr(wc), hip.ptr(bc), hip.ptr(out), N, V, C, hip.stream()))
        torch.cuda.synchronize()
        _check_valu("view_pool", (N, V, C), fx, out, ref, scale, N)
