"""Four-tap form of a convolution behind a nearest-2x upsample on the GPU (mvd_gemm_desc.tap_mode = MVD_TAPS_UP4): each output parity is a
2x2 convolution of the LOW-resolution image with composed weights (hip.pack_conv3x3_up4), K = 4 Cin instead of 9 Cin.
Reference: the float64 PyTorch-CPU convolution of the upsampled input.  Tolerances: the constants of tests/test_gpu_ops.py (TOL per
operand precision, PL for a value stored as split planes); the nine-tap launch on the same operands must meet them too, and the
difference between the two forms is printed."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import planes_to_float, rel_err
from test_gpu_ops import PL, TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    assert h.lib().mvd_version() == 100
    return h


def g(seed):
    return torch.Generator().manual_seed(seed)


# name -> (B, Hin, Win, Cin, Cout[, magnitude of the weights of the first 32 input channels (their inputs carry the inverse)])
CASES = {
    "baseline": (2, 8, 8, 64, 64),              # Mq = 128 rows per parity: one 128-row tile or two 64-row tiles
    "tiles": (3, 8, 8, 64, 64),                 # Mq = 192: several tiles per parity, a ragged last tile, tiles that cross an image boundary
    "raggedMq": (1, 3, 5, 32, 48),              # Mq = 15: not a multiple of 16
    "nonsquare": (3, 2, 6, 32, 48),
    "padding": (2, 1, 1, 32, 48),               # three of the four taps of every parity fall into the zero padding
    "raggedN": (2, 8, 8, 64, 40),               # Cout neither a multiple of 16 nor of a tile width
    "splitk": (2, 8, 8, 256, 64),               # 32 k-tiles per parity: 2 divides, 3 does not
    # the four parity images share ONE pack scale taken from the composed weights: weights three orders of magnitude apart, the inputs
    # scaled the other way so that both halves weigh the same in the output and lost low bits of the smaller weights would show
    "range": (2, 8, 8, 64, 64, 1e-3),
}
_MADE = {}


class _Case:
    pass


def _make(hip, name):
    if name in _MADE:
        return _MADE[name]
    B, H, W, Ci, Co = CASES[name][:5]
    sw = (CASES[name][5:] or (1.0,))[0]
    c = _Case()
    c.B, c.H, c.W, c.Ci, c.Co, c.Mq, c.M = B, H, W, Ci, Co, B * H * W, 4 * B * H * W
    x = torch.randn(B, Ci, H, W, generator=g(70)) * 1.5 + 0.2
    w = torch.randn(Co, Ci, 3, 3, generator=g(71)) / math.sqrt(9 * Ci)
    b = torch.randn(Co, generator=g(72))
    x[:, :32] /= sw
    w[:, :32] *= sw
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), w.double(), b.double(), padding=1)
    c.ref = ref.permute(0, 2, 3, 1).reshape(c.M, Co).cuda()               # float64, on the GPU: the matrices below compare there
    c.ref_max = float(c.ref.abs().max())
    c.xp = hip.split_planes(x.permute(0, 2, 3, 1).reshape(c.Mq, Ci).contiguous().cuda())
    c.W4, c.W9 = hip.pack_conv3x3_up4(w.cuda(), b.cuda()), hip.pack_conv3x3(w.cuda(), b.cuda())
    c.conv = dict(B=B, Hin=H, Win=W, Cin=Ci, Hout=2 * H, Wout=2 * W, stride=1, upsample=1)
    c.ldo = (Co + 3) // 4 * 4
    c.ws = torch.empty(4 * 1024 * 1024, device="cuda")
    _MADE[name] = c
    return c


def _err(c, out):
    return float((out[:, :c.Co].double() - c.ref).abs().max()) / (c.ref_max + 1e-30)


def _run(hip, c, W, **kw):
    out = torch.full((c.M, c.ldo), float("nan"), device="cuda")
    hip.gemm(c.xp, W, out, workspace=c.ws, ldo=c.ldo, conv=kw.pop("conv", c.conv), **kw)
    return out


def _desc(hip, c):
    """The problem as mvd_gemm_cfg_supported needs it."""
    d = hip.GemmDesc()
    d.M, d.N, d.K, d.a_mode, d.epi = c.M, c.W4.N, c.W4.K, hip.A_CONV3X3, hip.EPI_STORE
    d.B, d.Hin, d.Win, d.Cin, d.Hout, d.Wout, d.stride, d.upsample = c.B, c.H, c.W, c.Ci, 2 * c.H, 2 * c.W, 1, 1
    d.tap_mode = hip.TAPS_UP4
    return d


@pytest.mark.parametrize("prec", [4, 3, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_four_tap_matches_float64_and_the_nine_tap_launch(hip, name, prec):
    c = _make(hip, name)
    assert c.W4.up4 and c.W4.K == 4 * c.Ci and c.W4.n_real == c.Co and c.W4.N == (c.Co + 15) // 16 * 16
    assert c.W4.data.numel() == 16 * c.Ci * c.W4.N * 4          # four parity images of N x 4 Cin operands, 4 bytes each (hi + lo)
    for splitk in (0, 1, 2, 3):
        out = _run(hip, c, c.W4, prec=prec, splitk=splitk)
        old = _run(hip, c, c.W9, prec=prec, splitk=splitk)
        e_new, e_old = _err(c, out), _err(c, old)
        e_pair = float((out[:, :c.Co].double() - old[:, :c.Co].double()).abs().max()) / (c.ref_max + 1e-30)
        print(f"[up4] {name} prec={prec} splitk={splitk}: four-tap {e_new:.3e}  nine-tap {e_old:.3e}  four-tap vs nine-tap {e_pair:.3e}")
        assert e_new < TOL[prec], (name, prec, splitk)
        assert e_old < TOL[prec], (name, prec, splitk)
        assert torch.equal(out, _run(hip, c, c.W4, prec=prec, splitk=splitk))          # deterministic, split or not; every element written
        if c.Co % 32 == 0:          # the planes output of the same launch (a GEMM consumer's operand)
            op = hip.planes_like(c.M, c.Co, "cuda")
            out_p = _run(hip, c, c.W4, prec=prec, splitk=splitk, out_planes=op)
            assert _err(c, out_p) < TOL[prec] and rel_err(planes_to_float(op), out_p) < PL, (name, prec, splitk)


@pytest.mark.parametrize("name", ["baseline", "tiles", "raggedMq", "raggedN", "splitk"])
def test_four_tap_every_configuration(hip, name):
    """Every cfg mvd_gemm_cfg_supported admits for the mode, unsplit (bit-equal to each other: one k order per parity) and with a forced
    split that does not divide the k-tiles; the input-patch kernel declines, and mvd_gemm rejects it by name."""
    c = _make(hip, name)
    d = _desc(hip, c)
    served = declined = 0
    base = None
    for cfg in hip.gemm_configs(hip.EPI_STORE, conv=True):
        if not hip.cfg_supported(d, cfg):
            assert cfg in hip.PATCH_CONFIGS, cfg
            with pytest.raises(RuntimeError, match="does not serve"):
                _run(hip, c, c.W4, prec=4, cfg=cfg, splitk=1)
            declined += 1
            continue
        served += 1
        for splitk in (1, 3):
            out = _run(hip, c, c.W4, prec=4, cfg=cfg, splitk=splitk)
            assert _err(c, out) < TOL[4], (name, cfg, splitk)
            if splitk == 1:
                base = out if base is None else base
                assert torch.equal(out, base), (name, cfg)
            else:
                assert torch.equal(out, _run(hip, c, c.W4, prec=4, cfg=cfg, splitk=splitk)), (name, cfg)
    assert served == len(hip.GEMM_CONFIGS) and declined == len(hip.PATCH_CONFIGS)


def _group_norm_ref(x, B, HW, C, gm, bt, silu=True):
    y = F.group_norm(x.view(B, HW, C).permute(0, 2, 1), 32, gm, bt, eps=1e-5).permute(0, 2, 1).reshape(B * HW, C)
    return F.silu(y) if silu else y


@pytest.mark.parametrize("name", ["baseline", "tiles", "splitk"])
def test_four_tap_with_groupnorm_outputs(hip, name):
    """The launch's other writers (Hin * Win % 16 == 0): gn_stats alone, gna_out_sp (GroupNorm + SiLU behind the GEMM) and cat_b / cat_raw_sp
    (over the concatenation with a skip tensor), unsplit (tile epilogue + the library's apply launch) and split (the fused reduce), on the
    plain and the role-split kernel.  Each is checked against F.group_norm of the launch's own fp32 output (PL + 4e-6, the bound of
    tests/test_gpu_tap_schedule.py) and against the NINE-tap launch with the same outputs.  Bounds of the comparison with the nine-tap launch,
    from the reference and the operand precision alone: the two fp32 outputs differ by at most d = 2 TOL[3] ref_max per element, so
      statistics  {sum, sum of squares} of n values differ by at most n d and 2 n ref_max d; relative to the largest statistic, n E[x^2]:
                  2 (2 TOL[3]) ref_max^2 / E[ref^2];
      planes      y = silu(gamma (x - mean) / std + beta): |dy| <= 1.1 |gamma|max (2 + zmax) d / std_min, zmax = the largest |x - mean| / std
                  (the element, the mean and the std each move by at most d), plus the two plane roundings 2 PL."""
    c = _make(hip, name)
    B, HW, N, M = c.B, 4 * c.H * c.W, c.Co, c.M
    cb = 64
    gm, bt = torch.randn(N, generator=g(90)) + 1.0, torch.randn(N, generator=g(91))
    gmc, btc = torch.randn(N + cb, generator=g(92)) + 1.0, torch.randn(N + cb, generator=g(93))
    sk = (torch.randn(M, cb, generator=g(94)) * 1.5 + 0.3).cuda()
    gd, bd, gcd, bcd = gm.cuda(), bt.cuda(), gmc.cuda(), btc.cuda()
    L = hip.lib()
    assert L.mvd_concat_groupnorm_fits(N, cb, HW, 32)
    refc = c.ref.cpu()
    d_abs = 2 * TOL[3] * c.ref_max
    st_bound = 2 * (2 * TOL[3]) * c.ref_max ** 2 / float((refc ** 2).mean())

    def plane_bound(x, gamma, want):
        xg = x.view(B, HW, 32, -1).permute(0, 2, 1, 3).reshape(B, 32, -1)
        std = xg.std(dim=2, unbiased=False)
        zmax = float(((xg - xg.mean(dim=2, keepdim=True)).abs() / std[..., None]).max())
        return 1.1 * float(gamma.abs().max()) * (2 + zmax) * d_abs / float(std.min()) / float(want.abs().max()) + 2 * PL

    for cfg in (0, hip.make_cfg(1, hip.WS_LOOP)):
        for splitk in (1, 3):
            both = {}
            for form, W in (("four", c.W4), ("nine", c.W9)):
                plain = _run(hip, c, W, prec=3, cfg=cfg, splitk=splitk)
                assert _err(c, plain) < TOL[3]
                # ---- gn_stats alone
                st = torch.zeros(B, 32, 2, dtype=torch.int64, device="cuda")
                out = _run(hip, c, W, prec=3, cfg=cfg, splitk=splitk, gn_stats=st, gn_hw=HW)
                assert torch.equal(out, plain)
                y_st = hip.planes_like(M, N, "cuda")
                hip.groupnorm_from_stats(out, y_st, gd, bd, st, B, HW, N, 1e-5, True)
                want = _group_norm_ref(out.cpu(), B, HW, N, gm, bt)
                assert rel_err(planes_to_float(y_st), want) < PL + 4e-6, (name, form, cfg, splitk)
                # ---- gna_out_sp: the same planes from the GEMM's own launches
                st2 = torch.zeros_like(st)
                y = hip.planes_like(M, N, "cuda")
                y.fill_(0x7e00)
                out2 = _run(hip, c, W, prec=3, cfg=cfg, splitk=splitk, gn_stats=st2, gn_hw=HW, gn_apply=(gd, bd, 1e-5, hip.GNA_SILU, y))
                assert _err(c, out2) < TOL[3]
                assert rel_err(planes_to_float(y), want) < PL + 4e-6, (name, form, cfg, splitk)
                assert rel_err(st2.double(), st.double()) < 1e-5
                # ---- cat_b / cat_raw_sp: GroupNorm over [out | sk]
                st3 = torch.zeros_like(st)
                yc, raw = hip.planes_like(M, N + cb, "cuda"), hip.planes_like(M, N + cb, "cuda")
                out3 = _run(hip, c, W, prec=3, cfg=cfg, splitk=splitk, gn_stats=st3, gn_hw=HW,
                            gn_apply=(gcd, bcd, 1e-5, hip.GNA_SILU | hip.GNA_OUT_UNUSED, yc), cat=(sk, raw))
                del out3          # (GNA_OUT_UNUSED: the fused path may leave it unwritten)
                cat = torch.cat([plain.cpu(), sk.cpu()], 1)
                wantc = _group_norm_ref(cat, B, HW, N + cb, gmc, btc)
                assert rel_err(planes_to_float(yc), wantc) < PL + 4e-6, (name, form, cfg, splitk)
                assert rel_err(planes_to_float(raw), cat) < TOL[3] + PL, (name, form, cfg, splitk)
                both[form] = (st, planes_to_float(y), want, planes_to_float(yc), wantc, st3)
            f4, f9 = both["four"], both["nine"]
            e_st, e_y, e_yc = rel_err(f4[0].double(), f9[0].double()), rel_err(f4[1], f9[1]), rel_err(f4[3], f9[3])
            y_bound = plane_bound(refc.float(), gm, f9[2])
            yc_bound = plane_bound(torch.cat([refc.float(), sk.cpu()], 1), gmc, f9[4])
            print(f"[up4] {name} cfg={cfg} splitk={splitk}: four-tap vs nine-tap  statistics {e_st:.3e} (< {st_bound:.3e})  planes {e_y:.3e} "
                  f"(< {y_bound:.3e})  concat planes {e_yc:.3e} (< {yc_bound:.3e})")
            assert e_st < st_bound, (name, cfg, splitk)
            assert e_y < y_bound, (name, cfg, splitk)
            assert e_yc < yc_bound, (name, cfg, splitk)
            assert rel_err(f4[5].double(), f9[5].double()) < st_bound          # (statistics slot of the concatenation)


def test_four_tap_rejects_what_it_does_not_serve(hip):
    """include/mvd_hip.h, MVD_TAPS_UP4 "REFUSED": res, bias_b, colscale, rs_out, the GEGLU / QKV epilogues, no_pad_tl; a convolution
    without the upsample; gn_stats when Hin * Win is no multiple of 16; a weight whose K is not 4 Cin."""
    c = _make(hip, "baseline")
    res = torch.zeros(c.M, c.ldo, device="cuda")
    vec = torch.zeros(c.Co, device="cuda")
    takes_no = "takes no res, bias_b, colscale or rs_out"
    for kw in (dict(res=res), dict(bias_b=torch.zeros(c.B, c.Co, device="cuda"), rows_per_batch=c.M // c.B), dict(colscale=vec),
               dict(row_stats=hip.RowStats(c.M, c.Co, "cuda"))):
        with pytest.raises(RuntimeError, match=takes_no):
            _run(hip, c, c.W4, prec=3, **kw)
    with pytest.raises(RuntimeError, match="MVD_TAPS_UP4.*serves MVD_EPI_STORE only"):
        _run(hip, c, c.W4, prec=3, epi=hip.EPI_GEGLU)
    planes = hip.alloc_attn_planes(c.B, 2, 4 * c.H * c.W, 32, "cuda")
    with pytest.raises(RuntimeError, match="MVD_TAPS_UP4.*serves MVD_EPI_STORE only"):
        _run(hip, c, c.W4, prec=3, epi=hip.EPI_QKV, qkv=dict(planes=planes, heads=2, dhead=32, L=4 * c.H * c.W))
    geometry = "MVD_TAPS_UP4.*serves stride-1 padded convolutions behind a nearest-2x upsample"
    with pytest.raises(RuntimeError, match=geometry):
        _run(hip, c, c.W4, prec=3, conv=dict(c.conv, no_pad_tl=1))
    with pytest.raises(RuntimeError, match=geometry):          # no upsample: the same image as a plain 3x3 convolution
        hip.gemm(c.xp, c.W4, torch.empty(c.Mq, c.ldo, device="cuda"), prec=3, ldo=c.ldo,
                 conv=dict(B=c.B, Hin=c.H, Win=c.W, Cin=c.Ci, Hout=c.H, Wout=c.W, stride=1, upsample=0))
    r = _make(hip, "nonsquare")          # Hin * Win = 12
    st = torch.zeros(r.B, 32, 2, dtype=torch.int64, device="cuda")
    o48 = torch.empty(r.M, 64, device="cuda")
    with pytest.raises(RuntimeError, match="MVD_TAPS_UP4.*gn_stats needs Hin"):
        hip.gemm(r.xp, r.W4, o48, prec=3, ldo=64, conv=r.conv, gn_stats=st, gn_hw=4 * r.H * r.W, gn_groups=16)
    with pytest.raises(AssertionError):          # a four-tap weight on a convolution of another width
        _run(hip, c, c.W4, prec=3, conv=dict(c.conv, Cin=2 * c.Ci))
    d = _desc(hip, c)          # ... and the library's own check of K
    out = torch.empty(c.M, c.ldo, device="cuda")
    d.K = 9 * c.Ci
    d.A, d.Wp, d.out, d.ldo, d.prec = c.xp.data_ptr(), c.W9.data.data_ptr(), out.data_ptr(), c.ldo, 3
    assert hip.lib().mvd_gemm(hip.C.byref(d), hip.stream()) != 0 and b"4*Cin in the four-tap form" in hip.lib().mvd_last_error()


def test_upsample_layers_choose_the_form_per_launch(hip, monkeypatch):
    """unet.py: Upsample.run takes the four-tap form from hip.UP4_MIN_ROWS low-resolution rows upward and nine taps below, in training
    forwards and with MVD_UP4_MIN_ROWS=0; both agree within the GEMM tolerance."""
    from mvdfusion_amd.engine import Ctx
    from mvdfusion_amd.unet import Upsample
    torch.manual_seed(7)
    B, H, C = 2, 8, 64
    up = Upsample(C, True).cuda()
    x = (torch.randn(B * H * H, C) * 1.3).cuda()
    real, outs = hip.gemm, {}
    for label, min_rows, training in (("four", B * H * H, False), ("below", B * H * H + 1, False), ("training", 1, True), ("off", 0, False)):
        monkeypatch.setattr(hip, "UP4_MIN_ROWS", min_rows)
        _, prec, pol = hip.parse_precision("f16x3")
        ctx = Ctx("cuda", prec=prec, policy=pol)
        ctx.B, ctx.keep_fp32 = B, training
        ctx.begin_step()
        modes = []

        def recording(A, W, *a, **kw):
            modes.append(bool(W.up4))
            return real(A, W, *a, **kw)
        monkeypatch.setattr(hip, "gemm", recording)
        out, Ho, Wo = up.run(ctx, x, H, H)
        monkeypatch.setattr(hip, "gemm", real)
        outs[label] = out.clone()
        assert (Ho, Wo) == (2 * H, 2 * H) and modes == [label == "four"], (label, modes)
    ref = F.conv2d(F.interpolate(x.view(B, H, H, C).permute(0, 3, 1, 2).double().cpu(), scale_factor=2, mode="nearest"),
                   up.conv.weight.double().cpu(), up.conv.bias.double().cpu(), padding=1).permute(0, 2, 3, 1).reshape(-1, C)
    for label, out in outs.items():
        assert rel_err(out, ref) < TOL[3], label
