"""The normalisation / reduction family of csrc/norm.hip, the GroupNorm statistics its producers emit and the small backward kernels of
csrc/backward.hip against FLOAT64 (tests/norm_f64.py), at the shapes where the launch geometry changes and on data whose conditioning
the rest of the suite never leaves (|mean| / sigma <= 1 there).  Through the C ABI, into sentinel-filled outputs with four spare rows
behind the result; the spare rows and the padding columns must keep their bits.

Bars (norm_f64: gn_forward_bar, stable_bar, col_sum_bar, elementwise_bar), applied per (image, group), per row, per column or per
element -- never per tensor.  Every test prints the worst  error / bar  of its cases (pytest -s shows them); the bar allows 1.
tests/test_cpu_norm_f64.py shows that each realistic bug of norm_f64.MUTANTS is rejected by a case of the lists used here.

Fixtures and shapes: norm_f64.  For the ONE-PASS GroupNorm forward the offsets of offset8 / offset64 / chan_offset are milder for groups
under 512 elements (see there); the GroupNorm backward and the LayerNorm kernels see the full 64 sigma at every size.
Where a path's fp32 summation is longer than the 16 terms the kappa bound of gn_forward_bar is derived for, its bar takes the length R
of that chain as c = (R + 1) / 2, as the header comment of include/mvd_hip.h states: (1, 1021, 128) of mvd_groupnorm_nhwc (prime HW,
R = 256), mvd_concat_channels and the split-K reduce (R = C / groups + 6), the GEMM tile epilogue (R = 64 + C / groups - 1).  With c = 1
those paths measured 2.6 (emulation), 3.5, 1.003 of the bar on offset64: the algorithm, not a kernel fault.  Where the TEST writes the
slot (leg 1) the bar also carries the slot's resolution (norm_f64.gn_slot_quantum; it only shows at (1, 1, 32)).

Where the bars differ from the issue's text, each with its derivation in norm_f64:
  dgamma / dbeta / dw   the issue's bar on max|ref| of the group PLUS a rounding floor of 4 * 2^-24 * sum |terms| per channel and the shift
                        of xhat by the fp32 mean (gn_param_bar, ln_dw_bar): in a group of one channel max|ref| cancels to nearly nothing
  act forward           floor min(|x|, 1) (there is no dy);  GEGLU: |dy| min(|g|, 1) for the a half, |dy a| for the g half
  act_planes planes     + 2^-24 absolute in the fp16 flavour (gelu(1e-8) = 5e-9 is below what hi + lo resolve: operand range contract)
  layernorm, no affine  the constant row's reference is 0: absolute 2^-23 sqrt(kappa) there

Found by these tests: mvd_layernorm refused an fp32-only output (y_sp NULL) unless C % 32 == 0, although only the split planes need
that (C = 4, 36, 260 here); the check now applies to y_sp alone.

Measured on an MI355X, worst error / bar of a family over its shapes (the bar allows 1); 86 tests, 2.3 s (fp16 flavour) / 1.8 s (bf16):
                                                          | fp16 flavour | bf16 flavour
  groupnorm, own statistics        plain                  |        0.069 |        0.317
                                   offset8                |        0.133 |        0.313
                                   offset64               |        0.313 |        0.297      (1, 4096, 32, 32); emulation 0.31
                                   chan_offset            |        0.146 |        0.307
                                   tiny                   |        0.076 |        0.326
                                   const                  |        0.064 |        0.322
                                   outlier                |        0.176 |        0.314
                                   big                    |        0.058 |        0.260
  groupnorm, fp16 flag             plain                  | 1.5e-4 of the elements flipped (< 1e-3), worst 8.4e-4 relative (< 2.5e-3)
  groupnorm_from_stats, written    plain                  |        0.083 |        0.326
                                   offset64               |        0.401 |        0.297      (1, 1, 32): the slot's resolution
                                   const                  |        0.074 |        0.307
                                   outlier                |        0.170 |        0.314
  behind mvd_concat_channels       offset8 | offset64     | 0.100  0.091 | 0.299  0.302      slot 0.103 | 0.078
  mvd_concat_groupnorm             offset8 | offset64     | 0.070  0.056 | 0.247  0.062      slot 0.024 | 0.025
  behind the GEMM tile epilogue    offset8 | offset64     | 0.074  0.057 | 0.267  0.267      slot 0.116 | 0.078 (0.146 | 0.081 bf16)
  behind the split-K reduce        offset8 | offset64     | 0.260  0.598 | 0.291  0.324      (2, 256, 320), c = 1
  fused reduce + apply (gna)       offset8 | offset64     | 0.109  0.083 | 0.291  0.291
  layernorm                        plain                  |        0.087 |        0.318
                                   offset64               |        0.900 |        0.900      C = 4, fp32 output: a row of FOUR elements at 64 sigma
                                   tiny                   |        0.164 |        0.289
                                   const                  |        0.550 |        0.550      a row of 3.7: the fp32 mean of C equal values
  layernorm_groups                 plain ... const        | 0.067 0.588 0.043 0.680 | 0.283 0.588 0.291 0.680
  layernorm fold (ln_stats)        offset8                |        0.226 |        0.324
  softmax                          diffuse | one_hot | equal | 0.109 0.000 0.040 | 0.295 0.000 0.173
  groupnorm_backward dx            plain ... outlier      | 0.067 0.356 0.097 0.050 0.137          (fp32 outputs: the same in both flavours)
                     dgamma                               | 0.106 0.386 0.158 0.130 0.152
                     dbeta                                | 0.104 0.236 0.134 0.065 0.107
  layernorm_backward               plain ... const        | 0.040 0.205 0.037 0.541
  layernorm_backward_groups        plain ... const        | 0.029 0.281 0.034 0.033
  col_sum | _groups | _pow2                               | 0.491 0.495 0.483                      (the fp32 rounding of the result: 0.5)
  geglu_backward                                          |        0.067
  act_planes planes | fp32, act_backward                  | 0.493  0.041  0.234 | 0.334  0.041  0.234
  pixel_cross_attn_backward        diffuse dq | dk | dv   | 0.017 0.021 0.029                      (one_hot: 0.000, dS vanishes)
"""
import pytest
import torch

import norm_f64 as N
from conftest import planes_to_float
from test_gpu_attention_f64 import SENT, read_out, sentinel_out
from test_gpu_ops import PL

pytestmark = pytest.mark.gpu

SENT32 = 0x5A5A5A5A          # every 32-bit word of an fp32 output before the call (1.5e16 as a float)


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


def f32_out(rows, cols):
    return torch.full((rows + 4, cols), SENT32, dtype=torch.int32, device="cuda")


def read_f32(raw, rows, cols=None):
    """The four spare rows and the columns [cols, ld) must keep their bits; -> the (rows, cols) result."""
    raw = raw.cpu()
    assert bool((raw[rows:] == SENT32).all()), "rows behind the result were written"
    cols = raw.shape[1] if cols is None else cols
    assert bool((raw[:rows, cols:] == SENT32).all()), "columns behind the result were written"
    return raw[:rows, :cols].contiguous().view(torch.float32)


def untouched(*raws):
    torch.cuda.synchronize()
    return all(bool((r == (SENT if r.dtype == torch.int16 else SENT32)).all()) for r in raws)


def refused(hip, rc):
    assert rc != 0
    assert hip.lib().mvd_last_error().decode().startswith("mvd_")


def report(name, ratios):
    """ratios: {case: worst error / bar}.  Prints all of them, then demands every one <= 1."""
    for k, r in ratios.items():
        print(f"RATIO {name} {k}: {r:.3f}")
    bad = {k: r for k, r in ratios.items() if not r <= 1.0}
    assert not bad, (name, bad)


# ------------------------------------------------------------------------------------------------ GroupNorm, own statistics
def run_groupnorm(hip, xc, gc, bc, B, HW, C, G, flags):
    L = hip.lib()
    assert L.mvd_groupnorm_chunks(HW) == N.gn_chunks(HW)          # the geometry norm_f64's accumulation length is derived from
    y = sentinel_out(B * HW, C)
    ws = torch.empty(B * N.gn_chunks(HW) * G * 2, dtype=torch.float64, device="cuda")
    hip.check(L.mvd_groupnorm_nhwc(hip.ptr(xc), hip.ptr(y), hip.ptr(gc), hip.ptr(bc), B, HW, C, G, N.GN_EPS, flags, hip.ptr(ws), ws.numel(),
                                   hip.stream()))
    torch.cuda.synchronize()
    return read_out(y, B * HW, C).view(B, HW, C)


def gn_ratio(got, x, gm, bt, G, silu, R, slot=False):
    B = x.shape[0]
    ref = N.by_group(N.gn_forward(x, gm, bt, G, N.GN_EPS, silu), G)
    bar = N.gn_forward_bar(N.gn_kappa(x, G, N.GN_EPS), N.group_max(ref, B * G), PL, R)
    if slot:          # statistics written into the 2^24 fixed-point slot by the test (it shows at (1, 1, 32): groups of one element)
        bar = bar + N.gn_slot_quantum(x, gm, G, N.GN_EPS)
    return N.worst(N.by_group(got, G), ref, bar, B * G)


_GN = N.GN_SHAPES + [N.GN_BIG]


@pytest.mark.parametrize("B,HW,C,G", _GN, ids=_ids(_GN))
def test_groupnorm_own_statistics(hip, B, HW, C, G):
    gm, bt = N.gn_params(C)
    gc, bc = gm.cuda(), bt.cuda()
    ratios = {}
    for shape, fx in [c for c in N.gn_cases() if c[0] == (B, HW, C, G)]:
        x = N.gn_fixture(fx, B, HW, C, G)
        xc = x.cuda()
        for silu in (0, 1):
            got = run_groupnorm(hip, xc, gc, bc, B, HW, C, G, silu)
            ratios[(fx, silu)] = gn_ratio(got, x, gm, bt, G, bool(silu), N.gn_accum_len(HW, C))
    report(f"groupnorm {(B, HW, C, G)}", ratios)


def test_groupnorm_fp16_rounding_flag(hip):
    """silu flag bit 1 (the normalised value is rounded to fp16 before the swish): the rule of
    tests/test_gpu_ops.py::test_groupnorm_fp16_kept_output, unchanged, against the float64 reference."""
    (B, HW, C, G), fx = N.GN_F16_CASE
    x, (gm, bt) = N.gn_fixture(fx, B, HW, C, G), N.gn_params(C)
    got = run_groupnorm(hip, x.cuda(), gm.cuda(), bt.cuda(), B, HW, C, G, 3).double()
    ref = N.gn_forward(x, gm, bt, G, N.GN_EPS, True, round_f16=True)
    d = (got - ref).abs()
    flips = float((d > (2e-6 + 2 * PL) * (1 + ref.abs())).double().mean())
    worst = float((d / (1e-3 + ref.abs())).max())
    print(f"RATIO groupnorm fp16 flag: flipped {flips:.2e} of the elements (< 1e-3), worst relative {worst:.2e} (< 2.5e-3)")
    assert flips < 1e-3 and worst < 2.5e-3


# ------------------------------------------------------------------------------------------------ GroupNorm behind producer statistics
def run_from_stats(hip, xc, gc, bc, st, B, HW, C, G, flags):
    y = sentinel_out(B * HW, C)
    hip.check(hip.lib().mvd_groupnorm_from_stats(hip.ptr(xc), hip.ptr(y), hip.ptr(gc), hip.ptr(bc), hip.ptr(st), B, HW, C, G, N.GN_EPS, flags,
                                                 hip.stream()))
    torch.cuda.synchronize()
    return read_out(y, B * HW, C).view(B, HW, C)


@pytest.mark.parametrize("B,HW,C", N.GN_STATS_SHAPES, ids=_ids(N.GN_STATS_SHAPES))
def test_groupnorm_from_written_statistics(hip, B, HW, C):
    """Leg 1: the slot written by the test as llrint(sum * 2^24) from float64 -- the two apply kernels alone, at any HW."""
    gm, bt = N.gn_params(C)
    gc, bc = gm.cuda(), bt.cuda()
    ratios = {}
    for shape, fx in [c for c in N.gn_stats_cases() if c[0] == (B, HW, C, 32)]:
        x = N.gn_fixture(fx, B, HW, C, 32)
        xc, st = x.cuda(), N.gn_fixed_point_stats(x, 32).cuda()
        for silu in (0, 1):
            ratios[(fx, silu)] = gn_ratio(run_from_stats(hip, xc, gc, bc, st, B, HW, C, 32, silu), x, gm, bt, 32, bool(silu), 1, slot=True)
    report(f"groupnorm_from_stats {(B, HW, C)}", ratios)


def slot_ratio(st, out, G):
    """The slot against float64 sums of the STORED output, by the rule of tests/test_gpu_ops.py::test_gemm_groupnorm_statistics:
    |slot / 2^24 - sum| <= 2e-6 (1 + sum |x|) and likewise for the squares."""
    B = out.shape[0]
    xg = N.by_group(out.double(), G)
    sums = torch.stack([xg.sum(1), (xg * xg).sum(1)], 1)
    mags = torch.stack([xg.abs().sum(1), (xg * xg).sum(1)], 1)
    return float(((st.cpu().double().reshape(B * G, 2) / 2.0 ** 24 - sums).abs() / (2e-6 * (1.0 + mags))).max())


PRODUCER_FIXTURES = ("offset8", "offset64")


@pytest.mark.parametrize("B,HW,ca,cb", [(2, 64, 1280, 1280), (4, 16, 16, 16)], ids=_ids([(2, 64, 1280, 1280), (4, 16, 16, 16)]))
def test_groupnorm_behind_the_concat_producers(hip, B, HW, ca, cb):
    """Leg 2: mvd_concat_channels (slot) -> mvd_groupnorm_from_stats, and mvd_concat_groupnorm (one launch, where it serves the shape)."""
    L, C, M = hip.lib(), ca + cb, B * HW
    gm, bt = N.gn_params(C)
    gc, bc = gm.cuda(), bt.cuda()
    ratios = {}
    for fx in PRODUCER_FIXTURES:
        x = N.gn_fixture(fx, B, HW, C, 32)
        ad, bd = x.reshape(M, C)[:, :ca].contiguous().cuda(), x.reshape(M, C)[:, ca:].contiguous().cuda()
        out, outp = f32_out(M, C), sentinel_out(M, C)
        st = torch.zeros(B, 32, 2, dtype=torch.int64, device="cuda")
        hip.check(L.mvd_concat_channels(hip.ptr(ad), ca, hip.ptr(bd), cb, hip.ptr(out), hip.ptr(outp), M, hip.ptr(st), HW, 32, hip.stream()))
        torch.cuda.synchronize()
        assert torch.equal(read_f32(out, M), x.reshape(M, C))
        ratios[(fx, "concat_channels slot")] = slot_ratio(st, x, 32)
        ratios[(fx, "concat_channels planes")] = N.worst(read_out(outp, M, C), x.reshape(M, C), PL * N.group_max(x, M), M)
        for silu in (0, 1):
            got = run_from_stats(hip, out[:M].view(torch.float32), gc, bc, st, B, HW, C, 32, silu)
            ratios[(fx, "concat_channels", silu)] = gn_ratio(got, x, gm, bt, 32, bool(silu), N.producer_accum_len("slab", C // 32))
        if L.mvd_concat_groupnorm_fits(ca, cb, HW, 32):
            for silu in (0, 1):
                out2, raw, y = f32_out(M, C), sentinel_out(M, C), sentinel_out(M, C)
                st2 = torch.zeros(B, 32, 2, dtype=torch.int64, device="cuda")
                hip.check(L.mvd_concat_groupnorm(hip.ptr(ad), ca, hip.ptr(bd), cb, hip.ptr(out2), hip.ptr(raw), hip.ptr(y), hip.ptr(gc), hip.ptr(bc),
                                                 hip.ptr(st2), B, HW, 32, N.GN_EPS, silu, hip.stream()))
                torch.cuda.synchronize()
                assert torch.equal(read_f32(out2, M), x.reshape(M, C))
                ratios[(fx, "concat_groupnorm", silu)] = gn_ratio(read_out(y, M, C).view(B, HW, C), x, gm, bt, 32, bool(silu), 1)
                ratios[(fx, "concat_groupnorm slot", silu)] = slot_ratio(st2, x, 32)
    report(f"concat producers {(B, HW, ca, cb)}", ratios)


@pytest.mark.parametrize("B,HW,C", [(2, 256, 320), (4, 16, 32)], ids=_ids([(2, 256, 320), (4, 16, 32)]))
def test_groupnorm_behind_the_gemm_producers(hip, B, HW, C):
    """Leg 2: the GEMM tile epilogue (splitk = 1), the split-K reduce (splitk = 3) and the fused reduce + apply (gna_out_sp) as producers.
    An identity weight carries N(0, 1) rows, the bias carries the offset of the group; the normalised planes are compared with the
    float64 GroupNorm of the STORED fp32 output, the slot with float64 sums of it."""
    M = B * HW
    gm, bt = N.gn_params(C)
    gc, bc = gm.cuda(), bt.cuda()
    ws = torch.empty(8 * 1024 * 1024, device="cuda")
    ap = hip.split_planes(N.gn_fixture("tiny", B, HW, C, 32).reshape(M, C).cuda() * 1e4)          # N(0, 1)
    ratios = {}
    for fx in PRODUCER_FIXTURES:
        sign = torch.where(torch.arange(C) // (C // 32) % 2 == 0, 1.0, -1.0)
        Wp = hip.pack_linear(torch.eye(C, device="cuda"), (sign * N.gn_offset(fx, HW * (C // 32))).cuda())
        for splitk in (1, 3):
            out = f32_out(M, C)
            st = torch.zeros(B, 32, 2, dtype=torch.int64, device="cuda")
            hip.gemm(ap, Wp, out[:M].view(torch.float32), prec=4, workspace=ws, splitk=splitk, gn_stats=st, gn_hw=HW)
            torch.cuda.synchronize()
            x = read_f32(out, M).view(B, HW, C)
            kap = N.gn_kappa(x, 32, N.GN_EPS)
            assert float(kap.min()) > 0.5 * (1 + N.gn_offset(fx, HW * (C // 32)) ** 2), "the stored output does not carry the offset"
            ratios[(fx, splitk, "slot")] = slot_ratio(st, x, 32)
            for silu in (0, 1):
                got = run_from_stats(hip, out[:M].view(torch.float32), gc, bc, st, B, HW, C, 32, silu)
                R = N.producer_accum_len("tile" if splitk == 1 else "slab", C // 32)
                ratios[(fx, splitk, "from_stats", silu)] = gn_ratio(got, x, gm, bt, 32, bool(silu), R)
        for silu in (0, 1):          # fused reduce + apply behind the split GEMM (the library falls back to slot + apply where it must)
            out, y = f32_out(M, C), sentinel_out(M, C)
            st = torch.zeros(B, 32, 2, dtype=torch.int64, device="cuda")
            hip.gemm(ap, Wp, out[:M].view(torch.float32), prec=4, workspace=ws, splitk=3, gn_stats=st, gn_hw=HW,
                     gn_apply=(gc, bc, N.GN_EPS, silu, y[:M]))
            torch.cuda.synchronize()
            x = read_f32(out, M).view(B, HW, C)
            ratios[(fx, "gna", silu)] = gn_ratio(read_out(y, M, C).view(B, HW, C), x, gm, bt, 32, bool(silu), 1)
            ratios[(fx, "gna slot", silu)] = slot_ratio(st, x, 32)
    report(f"gemm producers {(B, HW, C)}", ratios)


# ------------------------------------------------------------------------------------------------ LayerNorm
def run_layernorm(hip, xc, wc, bc, ldw, rows, rpg, C, wp1, planes):
    y, yf = (sentinel_out(rows, C) if planes else None), f32_out(rows, C)
    hip.check(hip.lib().mvd_layernorm_groups(hip.ptr(xc), hip.ptr(y), hip.ptr(yf), hip.ptr(wc), hip.ptr(bc), ldw, rows, rpg, C, N.LN_EPS,
                                             int(wp1), hip.stream()))
    torch.cuda.synchronize()
    return (read_out(y, rows, C) if planes else None), read_f32(yf, rows)


def ln_ratios(got_planes, got_f32, ref, x, affine=True):
    """Without an affine (w = 1, b = 0) the reference of a constant row is 0: there the bar is the absolute 2^-23 sqrt(kappa) the fp32 mean
    moves xhat by (stable_bar with the weight's 1 in place of max|ref|)."""
    rows = x.shape[0]
    kap, mx = N.ln_kappa(x, N.LN_EPS), N.group_max(ref, rows)
    zero = torch.zeros_like(mx) if affine else 2.0 * N.U24 * kap.sqrt() * (mx == 0)
    r = N.worst(got_f32, ref, N.stable_bar(3e-6, kap, mx) + zero, rows)
    return r if got_planes is None else max(r, N.worst(got_planes, ref, N.stable_bar(PL + 3e-6, kap, mx) + zero, rows))


@pytest.mark.parametrize("C", N.LN_PLANES_C + N.LN_F32_C)
def test_layernorm(hip, C):
    """mvd_layernorm: split planes + fp32 output (C % 32 == 0) or the fp32 output alone (any C % 4 == 0), no affine / affine / modulate."""
    w, b = N.ln_params(1, C, 1)
    wc, bc = w.cuda(), b.cuda()
    ratios = {}
    for rows, _, _, wp1 in [c for c in N.ln_cases() if c[1] == C and not c[2]]:
        for fx in N.LN_FIXTURES:
            x = N.ln_fixture(fx, rows, C)
            xc = x.cuda()
            yp, yf = run_layernorm(hip, xc, wc, bc, 0, rows, rows, C, wp1, C % 32 == 0)
            ratios[(rows, fx, wp1)] = ln_ratios(yp, yf, N.ln_forward(x, w, b, N.LN_EPS, wp1), x)
            if not wp1:
                yp, yf = run_layernorm(hip, xc, None, None, 0, rows, rows, C, False, C % 32 == 0)
                ratios[(rows, fx, "no affine")] = ln_ratios(yp, yf, N.ln_forward(x, None, None, N.LN_EPS), x, affine=False)
    report(f"layernorm C={C}", ratios)


_LN_GROUPS = [(rpg, ng, C) for rpg, ng in N.LN_GROUPS for C in N.LN_GROUPS_C]


@pytest.mark.parametrize("rpg,ng,C", _LN_GROUPS, ids=_ids(_LN_GROUPS))
def test_layernorm_row_groups(hip, rpg, ng, C):
    """mvd_layernorm_groups: w / b are column slices of an (ngroups, 6 C) modulation tensor; a 4-row block of the kernel straddles groups."""
    rows = rpg * ng
    modc = N.ln_modulation(ng, C).cuda()
    w, b = N.ln_params(ng, C)
    ratios = {}
    for fx in N.LN_FIXTURES:
        x = N.ln_fixture(fx, rows, C)
        yp, yf = run_layernorm(hip, x.cuda(), modc[:, C:2 * C], modc[:, 3 * C:4 * C], 6 * C, rows, rpg, C, True, True)
        ratios[fx] = ln_ratios(yp, yf, N.ln_forward(x, w, b, N.LN_EPS, True, rpg), x)
    report(f"layernorm_groups {(rpg, ng, C)}", ratios)


def test_layernorm_folded_into_the_gemm(hip):
    """mvd_gemm_desc.ln_stats: the producer GEMM emits per-row {sum, sum of squares} in ONE pass (fp32 partial sums per wave tile), the
    consumer finishes  rstd (x.W' - mean colsum(W')) + W beta  in its epilogue.  Rows with mean = 8 sigma (identity producer weight, the
    offset in its bias); an identity consumer weight per q / k / v block makes the attention operand planes the LayerNorm itself.  Per row
      |got - ref| <= (4 TOL[4] + PL + 2^-24 kappa) max|ref_row|:
    4 TOL[4] + PL is the bar of tests/test_gpu_ops.py::test_gemm_layernorm_fold; the one-pass variance carries the kappa term of the
    GroupNorm forward."""
    import torch.nn as nn
    from test_gpu_ops import TOL, layernorm_fold_producer
    B, L, H, d = 2, 64, 8, 64
    M, C = B * L, H * d
    g = N._gen("ln_fold", M, C)
    offs = N.gn_offset("offset8", C)
    ws = torch.empty(8 * 1024 * 1024, device="cuda")
    tt, tp, rs = layernorm_fold_producer(hip, torch.randn(M, C, generator=g), torch.eye(C), torch.full((C,), offs), torch.zeros(M, C), ws)
    t = tt.cpu()
    norm = nn.LayerNorm(C)
    with torch.no_grad():
        norm.weight.copy_(1.0 + 0.3 * torch.randn(C, generator=g))
        norm.bias.copy_(0.2 * torch.randn(C, generator=g))
    ref = N.ln_forward(t, norm.weight, norm.bias, norm.eps)
    kap = N.ln_kappa(t, norm.eps)
    assert float(kap.min()) > 0.5 * (1 + offs * offs), "the stored rows do not carry the offset"
    fold = hip.LnFold(torch.eye(C).repeat(3, 1).cuda(), None, norm.cuda())
    planes = hip.alloc_attn_planes(B, H, L, d, "cuda")
    for p in planes:
        p.zero_()
    hip.gemm(tp, fold.w, None, epi=hip.EPI_QKV, qkv=dict(planes=planes, heads=H, dhead=d, L=L), workspace=ws, ln=(rs, fold))
    torch.cuda.synchronize()
    dt = torch.bfloat16 if hip.OPERAND_FORMAT == "bf16" else torch.float16
    dec = lambda i: (planes[2 * i].view(dt).float() + planes[2 * i + 1].view(dt).float()).cpu()
    Lp = hip.lib().mvd_attn_lpad(L)
    rows = lambda p: p.view(B, H, Lp, d)[:, :, :L].permute(0, 2, 1, 3).reshape(M, C)
    got = {"q": rows(dec(0)) / (d ** -0.5 * 1.4426950408889634), "k": rows(dec(1)),
           "v": dec(2).view(B, H, d, Lp)[:, :, :, :L].permute(0, 3, 1, 2).reshape(M, C)}
    bar = (4 * TOL[4] + PL + N.U24 * kap) * N.group_max(ref, M)
    report("layernorm fold", {k: N.worst(v, ref, bar, M) for k, v in got.items()})


# ------------------------------------------------------------------------------------------------ softmax
@pytest.mark.parametrize("rows,cols,ldx", N.SOFTMAX_SHAPES, ids=_ids(N.SOFTMAX_SHAPES))
def test_softmax_rows(hip, rows, cols, ldx):
    ratios = {}
    for shape, fx, sc in [c for c in N.softmax_cases() if c[0] == (rows, cols, ldx)]:
        x = N.softmax_fixture(fx, rows, cols, ldx, sc)
        xc, y = x.cuda(), sentinel_out(rows, cols)
        hip.check(hip.lib().mvd_softmax_rows(hip.ptr(xc), hip.ptr(y), rows, cols, ldx, sc, N.SOFTMAX_OUT_SCALE, hip.stream()))
        torch.cuda.synchronize()
        ref = N.softmax_rows(x[:, :cols], sc)
        ratios[(fx, sc)] = N.worst(read_out(y, rows, cols) / N.SOFTMAX_OUT_SCALE, ref, (2e-6 + PL) * N.group_max(ref, rows), rows)
    report(f"softmax {(rows, cols, ldx)}", ratios)


# ------------------------------------------------------------------------------------------------ GroupNorm / LayerNorm backward
@pytest.mark.parametrize("B,HW,C,G", N.GN_BWD_SHAPES, ids=_ids(N.GN_BWD_SHAPES))
def test_groupnorm_backward(hip, B, HW, C, G):
    L = hip.lib()
    gm, bt = N.gn_params(C)
    gc, bc = gm.cuda(), bt.cuda()
    dy = N.gn_dy(B, HW, C)
    dyc = dy.cuda()
    n_ws = B * G * 2 + B * C * 2
    ratios = {}
    for shape, fx in [c for c in N.gn_bwd_cases() if c[0] == (B, HW, C, G)]:
        x = N.gn_fixture(fx, B, HW, C, G, full=True)          # (fp64 moments: the full offsets at every group size)
        xc = x.cuda()
        kap = N.gn_kappa(x, G, N.GN_EPS)
        for silu in (0, 1):
            runs = []
            for rep in range(2):
                dx, dg, db = f32_out(B * HW, C), f32_out(1, C), f32_out(1, C)
                ws = torch.empty(n_ws, device="cuda")
                hip.check(L.mvd_groupnorm_backward(hip.ptr(xc), hip.ptr(dyc), hip.ptr(gc), hip.ptr(bc), B, HW, C, G, N.GN_EPS, silu, hip.ptr(dx),
                                                   hip.ptr(dg), hip.ptr(db), hip.ptr(ws), n_ws, hip.stream()))
                torch.cuda.synchronize()
                runs.append((read_f32(dx, B * HW), read_f32(dg, 1), read_f32(db, 1)))
            assert all(torch.equal(a, b) for a, b in zip(*runs)), "a second evaluation is not bit-identical"
            rdx, rdg, rdb, adg, adb, shb = N.gn_backward(x, dy, gm, bt, G, N.GN_EPS, bool(silu), with_abs=True)
            rdxg = N.by_group(rdx, G)
            ratios[(fx, silu, "dx")] = N.worst(N.by_group(runs[0][0].view(B, HW, C), G), rdxg, N.stable_bar(5e-6, kap, N.group_max(rdxg, B * G)), B * G)
            # dgamma / dbeta per channel: the issue's bar on max|ref| of the channel's group (the worst image's kappa) plus the rounding
            # floor of norm_f64.gn_param_bar
            kg = kap.reshape(B, G).amax(0)
            ratios[(fx, silu, "dgamma")] = N.worst(runs[0][1], rdg, N.gn_param_bar(rdg, kg, G, adg, adb), C)
            ratios[(fx, silu, "dbeta")] = N.worst(runs[0][2], rdb, N.gn_param_bar(rdb, kg, G, adb, shb), C)
    report(f"groupnorm_backward {(B, HW, C, G)}", ratios)


def run_ln_backward(hip, xc, dyc, wc, ldw, rows, rpg, C):
    L = hip.lib()
    ng = rows // rpg
    dx, t, dw, db = f32_out(rows, C), f32_out(rows, C), f32_out(ng, C), f32_out(ng, C)
    n = L.mvd_col_sum_groups_workspace_doubles(ng, rpg, C)
    ws = torch.empty(n, dtype=torch.float64, device="cuda")
    hip.check(L.mvd_layernorm_backward_groups(hip.ptr(xc), hip.ptr(dyc), hip.ptr(wc), ldw, rows, rpg, C, N.LN_EPS, hip.ptr(dx), hip.ptr(t),
                                              hip.ptr(dw), hip.ptr(db), hip.ptr(ws), n, hip.stream()))
    torch.cuda.synchronize()
    return read_f32(dx, rows), read_f32(t, rows), read_f32(dw, ng), read_f32(db, ng)


def ln_bwd_ratio(got, x, dy, w, rpg):
    """dx per row; dw per element at norm_f64.ln_dw_bar (the issue's bar on max|dw| of the row group plus a rounding floor); db per row
    group against 2e-6 max|ref| (x does not enter)."""
    rows, C = x.shape
    ng = rows // rpg
    dx, dw, db = N.ln_backward(x, dy, w, N.LN_EPS, rpg)
    kap = N.ln_kappa(x, N.LN_EPS)
    r = N.worst(got[0], dx, N.stable_bar(5e-6, kap, N.group_max(dx, rows)), rows)
    r = max(r, N.worst(got[2], dw, N.ln_dw_bar(x, dy, dw, N.LN_EPS, rpg), ng * C))
    return max(r, N.worst(got[3], db, 2e-6 * N.group_max(db, ng), ng))


@pytest.mark.parametrize("C", N.LN_BWD_C)
def test_layernorm_backward(hip, C):
    """mvd_layernorm_backward (dx, dy * xhat) and the one-group mvd_layernorm_backward_groups (the same plus dw, db)."""
    w = N.ln_params(1, C, 1)[0]
    wc = w.cuda()
    ratios = {}
    for rows in N.LN_ROWS:
        dy = N.gn_dy(1, rows, C)[0]
        dyc = dy.cuda()
        for fx in N.LN_FIXTURES:
            x = N.ln_fixture(fx, rows, C)
            xc = x.cuda()
            got = run_ln_backward(hip, xc, dyc, wc, 0, rows, rows, C)
            ratios[(rows, fx)] = ln_bwd_ratio(got, x, dy, w, rows)
            dx, t = f32_out(rows, C), f32_out(rows, C)
            hip.check(hip.lib().mvd_layernorm_backward(hip.ptr(xc), hip.ptr(dyc), hip.ptr(wc), rows, C, N.LN_EPS, hip.ptr(dx), hip.ptr(t), hip.stream()))
            torch.cuda.synchronize()
            assert torch.equal(read_f32(dx, rows), got[0]) and torch.equal(read_f32(t, rows), got[1])
    report(f"layernorm_backward C={C}", ratios)


_LN_BWD_GROUPS = [c for c in N.ln_bwd_cases() if c[2]]


@pytest.mark.parametrize("rows,C,rpg", _LN_BWD_GROUPS, ids=_ids(_LN_BWD_GROUPS))
def test_layernorm_backward_row_groups(hip, rows, C, rpg):
    """Per-group dw / db against float64 -- not against the single-group kernels."""
    ng = rows // rpg
    modc = N.ln_modulation(ng, C).cuda()
    w = N.ln_params(ng, C)[0]
    dy = N.gn_dy(1, rows, C)[0]
    ratios = {}
    for fx in N.LN_FIXTURES:
        x = N.ln_fixture(fx, rows, C)
        ratios[fx] = ln_bwd_ratio(run_ln_backward(hip, x.cuda(), dy.cuda(), modc[:, C:2 * C], 6 * C, rows, rpg, C), x, dy, w, rpg)
    report(f"layernorm_backward_groups {(rows, C, rpg)}", ratios)


# ------------------------------------------------------------------------------------------------ column sums
def run_col_sum(hip, xc, rows, cols, ldx, ngroups=1):
    L = hip.lib()
    out = f32_out(ngroups, cols)
    if ngroups == 1:
        n = L.mvd_col_sum_workspace_doubles(rows, cols)
        ws = torch.empty(n, dtype=torch.float64, device="cuda")
        hip.check(L.mvd_col_sum(hip.ptr(xc), rows, cols, ldx, hip.ptr(out), hip.ptr(ws), n, hip.stream()))
    else:
        n = L.mvd_col_sum_groups_workspace_doubles(ngroups, rows, cols)
        ws = torch.empty(n, dtype=torch.float64, device="cuda")
        hip.check(L.mvd_col_sum_groups(hip.ptr(xc), ngroups, rows, cols, ldx, hip.ptr(out), hip.ptr(ws), n, hip.stream()))
    torch.cuda.synchronize()
    return read_f32(out, ngroups)


@pytest.mark.parametrize("rows", N.COL_SUM_ROWS)
def test_col_sum(hip, rows):
    ratios = {}
    for cols in N.COL_SUM_COLS:
        for ld in (cols, cols + 5):          # contiguous, and a column view of a wider matrix
            x = N.col_sum_fixture(rows, cols, ld)
            ref = N.col_sum(x[:, :cols])
            ratios[(cols, ld)] = N.worst(run_col_sum(hip, x.cuda(), rows, cols, ld), ref, N.col_sum_bar(x[:, :cols], ref), cols)
    report(f"col_sum rows={rows}", ratios)


@pytest.mark.parametrize("ng,rpg", N.COL_SUM_GROUPS, ids=_ids(N.COL_SUM_GROUPS))
def test_col_sum_groups(hip, ng, rpg):
    ratios = {}
    for cols in N.COL_SUM_COLS:
        x = N.col_sum_fixture(ng * rpg, cols, cols + 5)
        ref = N.col_sum(x[:, :cols], ng)
        ratios[cols] = N.worst(run_col_sum(hip, x.cuda(), rpg, cols, cols + 5, ng), ref, N.col_sum_bar(x[:, :cols], ref, ng), ng * cols)
    report(f"col_sum_groups {(ng, rpg)}", ratios)


@pytest.mark.parametrize("rows,cols", [(7, 31), (257, 320), (16385, 33)], ids=_ids([(7, 31), (257, 320), (16385, 33)]))
def test_col_sum_pow2(hip, rows, cols):
    """One pass: the sums of mvd_col_sum (bit for bit) and {s, 1/s} of mvd_pow2_scale, exactly; the scratch word is left zero."""
    L = hip.lib()
    ratios = {}
    for name, x in (("pair", N.col_sum_fixture(rows, cols)), ("small", N.col_sum_fixture(rows, cols) * 3e-7), ("zero", torch.zeros(rows, cols))):
        if name == "small":
            x[0, cols // 2], x[rows - 1, cols // 2] = 0.3, -0.3
        xc = x.cuda()
        out, out2 = f32_out(1, cols), f32_out(1, 2)
        scratch = torch.zeros(1, dtype=torch.int32, device="cuda")
        n = L.mvd_col_sum_workspace_doubles(rows, cols)
        ws = torch.empty(n, dtype=torch.float64, device="cuda")
        hip.check(L.mvd_col_sum_pow2(hip.ptr(xc), rows, cols, cols, hip.ptr(out), hip.ptr(ws), n, hip.ptr(out2), hip.ptr(scratch), hip.stream()))
        torch.cuda.synchronize()
        got = read_f32(out, 1)
        assert torch.equal(got, run_col_sum(hip, xc, rows, cols, cols))
        assert tuple(read_f32(out2, 1)[0].tolist()) == N.pow2_scale(x), name
        assert int(scratch.item()) == 0
        ref = N.col_sum(x)
        ratios[name] = N.worst(got, ref, N.col_sum_bar(x, ref), cols)
    report(f"col_sum_pow2 {(rows, cols)}", ratios)


# ------------------------------------------------------------------------------------------------ elementwise kernels
def check_finite(t):
    assert bool(torch.isfinite(t).all()), "a finite input gave a value that is not finite"
    return t


@pytest.mark.parametrize("rows,half", N.ELEMENTWISE_SHAPES + [N.GEGLU_BIG], ids=_ids(N.ELEMENTWISE_SHAPES + [N.GEGLU_BIG]))
def test_geglu_backward(hip, rows, half):
    h, dy = N.value_grid(rows, 2 * half, "h"), N.value_grid(rows, half, "dy")
    hc, dc, dh = h.cuda(), dy.cuda(), f32_out(rows, 2 * half)
    hip.check(hip.lib().mvd_geglu_backward(hip.ptr(hc), hip.ptr(dc), rows, half, hip.ptr(dh), hip.stream()))
    torch.cuda.synchronize()
    ref, floor = N.geglu_backward(h, dy)
    report(f"geglu_backward {(rows, half)}",
           {"dh": N.worst(check_finite(read_f32(dh, rows)), ref, N.elementwise_bar(ref, floor), rows * 2 * half)})


@pytest.mark.parametrize("rows,cols", N.ELEMENTWISE_SHAPES + [N.ACT_BIG], ids=_ids(N.ELEMENTWISE_SHAPES + [N.ACT_BIG]))
def test_act_planes_and_act_backward(hip, rows, cols):
    L = hip.lib()
    x, dy = N.value_grid(rows, cols, "x"), N.value_grid(rows, cols, "dy")
    xc, dc = x.cuda(), dy.cuda()
    ldp, ldy, n = (cols + 31) // 32 * 32, cols + 3, rows * cols
    ratios = {}
    for act in (N.ACT_GELU, N.ACT_SILU):
        sp, y = sentinel_out(rows, ldp), f32_out(rows, ldy)
        hip.check(L.mvd_act_planes(hip.ptr(xc), hip.ptr(sp), hip.ptr(y), rows, cols, cols, ldp, ldy, act, hip.stream()))
        dx = f32_out(rows, cols)
        hip.check(L.mvd_act_backward(hip.ptr(dc), hip.ptr(xc), hip.ptr(dx), n, act, hip.stream()))
        torch.cuda.synchronize()
        raw = sp.cpu()
        assert bool((raw[rows:] == SENT).all()), "rows behind the planes were written"
        planes = planes_to_float(raw[:rows])
        assert bool((planes[:, cols:] == 0).all()), "padded plane columns must be zero"
        ref = N.act_forward(x, act)
        # (fp16 flavour: hi and lo resolve 2^-25 each below 6e-5 -- the operand range contract of include/mvd_hip.h)
        plane_abs = 0.0 if hip.OPERAND_FORMAT == "bf16" else 2.0 ** -24
        ratios[(act, "planes")] = N.worst(check_finite(planes[:, :cols]), ref, N.elementwise_bar(ref, x.abs().clamp_max(1.0), PL + 3e-6) + plane_abs, n)
        ratios[(act, "f32")] = N.worst(check_finite(read_f32(y, rows, cols)), ref, N.elementwise_bar(ref, x.abs().clamp_max(1.0)), n)
        ref = N.act_backward(dy, x, act)
        ratios[(act, "backward")] = N.worst(check_finite(read_f32(dx, rows)), ref, N.elementwise_bar(ref, dy.abs()), n)
    report(f"act {(rows, cols)}", ratios)


# ------------------------------------------------------------------------------------------------ per-pixel cross-attention backward
@pytest.mark.parametrize("P,D,H,d", N.PIXEL_BWD_CASES, ids=_ids(N.PIXEL_BWD_CASES))
def test_pixel_cross_attn_backward(hip, P, D, H, d):
    """P * heads % 4 != 0 (a partly filled last workgroup), dhead below / above the 64 lanes of the wave, heads * dhead off 32."""
    C = H * d
    ratios = {}
    for fx in N.PIXEL_BWD_FIXTURES:
        q, k, v, dout = N.pixel_bwd_fixture(fx, P, D, H, d)
        dev = [t.cuda() for t in (q, k, v, dout)]
        dq, dk, dv = f32_out(P, C), f32_out(P * D, C), f32_out(P * D, C)
        hip.check(hip.lib().mvd_pixel_cross_attn_backward(*[hip.ptr(t) for t in dev], P, D, H, d, hip.ptr(dq), hip.ptr(dk), hip.ptr(dv), hip.stream()))
        torch.cuda.synchronize()
        (rq, rk, rv), (sq, sk, sv) = N.pixel_xattn_backward(q, k, v, dout, P, D, H, d)
        ratios[(fx, "dq")] = N.worst(read_f32(dq, P).reshape(P * H, d), rq.reshape(P * H, d), 5e-6 * sq, P * H)
        ratios[(fx, "dk")] = N.worst(N.pixel_by_head(read_f32(dk, P * D), P, D, H, d), N.pixel_by_head(rk, P, D, H, d), 5e-6 * sk, P * H)
        ratios[(fx, "dv")] = N.worst(N.pixel_by_head(read_f32(dv, P * D), P, D, H, d), N.pixel_by_head(rv, P, D, H, d), 5e-6 * sv, P * H)
    report(f"pixel_cross_attn_backward {(P, D, H, d)}", ratios)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_alone(hip):
    L, p, s = hip.lib(), hip.ptr, hip.stream()
    x = torch.zeros(1 << 16, device="cuda")
    wsd = torch.empty(1 << 14, dtype=torch.float64, device="cuda")
    y, yf = sentinel_out(64, 4160), f32_out(64, 4160)
    gn = lambda B, HW, C, G: L.mvd_groupnorm_nhwc(p(x), p(y), p(x), p(x), B, HW, C, G, 1e-5, 0, p(wsd), wsd.numel(), s)
    refused(hip, gn(1, 4, 2080, 65))                 # groups = 65
    refused(hip, gn(1, 4, 96, 64))                   # C % groups != 0
    refused(hip, gn(1, 4, 2592, 32))                 # C = 2592 > 2560
    st = torch.zeros(64 * 2, dtype=torch.int64, device="cuda")
    refused(hip, L.mvd_groupnorm_from_stats(p(x), p(y), p(x), p(x), p(st), 1, 4, 2592, 32, 1e-5, 0, s))
    refused(hip, L.mvd_softmax_rows(p(x), p(y), 4, 4128, 4128, 1.0, 1.0, s))          # cols = 4128 > 4096
    refused(hip, L.mvd_softmax_rows(p(x), p(y), 4, 48, 48, 1.0, 1.0, s))              # cols = 48, not a multiple of 32
    refused(hip, L.mvd_layernorm(p(x), p(y), p(yf), None, None, 4, 1312, 1e-5, 0, s))                      # C = 1312 > 1280
    refused(hip, L.mvd_layernorm_groups(p(x), p(y), p(yf), p(x), p(x), 32, 10, 3, 32, 1e-5, 0, s))         # 3 does not divide 10 rows
    refused(hip, L.mvd_layernorm(p(x), p(y), None, None, None, 4, 36, 1e-5, 0, s))                         # planes need C % 32 == 0
    ws = torch.empty(1 * 32 * 2 + 1 * 64 * 2 - 1, device="cuda")
    refused(hip, L.mvd_groupnorm_backward(p(x), p(x), p(x), p(x), 1, 4, 64, 32, 1e-5, 0, p(yf), p(yf), p(yf), p(ws), ws.numel(), s))   # ws one short
    refused(hip, L.mvd_pixel_cross_attn_backward(p(x), p(x), p(x), p(x), 4, 9, 2, 8, p(yf), p(yf), p(yf), s))                            # D = 9
    assert untouched(y, yf)
