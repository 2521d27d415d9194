"""Conv tap schedule on the GPU (mvd_gemm_desc.tap_mode = MVD_TAPS_CENTRE_TAIL): conv3x3(a2) + conv1x1(x) as ONE implicit GEMM whose last
k-tiles read the second operand at the centre tap -- a ResBlock's conv2 with its 1x1 skip convolution (unet.py: ResBlock.run).
References: a float64 PyTorch-CPU statement of the two convolutions, and the two-launch path it replaces (skip GEMM -> fp32 -> `res=`).
Tolerances: the constants of tests/test_gpu_ops.py (TOL per operand precision, PL for a value stored as split planes)."""
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


# name -> (B, H, W, conv channels in, channels out, skip channels in).  The UNet's ResBlocks with a skip convolution at the benchmark's
# CFG batch of 8 views (conv2 is Co -> Co, the skip reads the block input / the decoder's concatenation), the same at an 8-way rank
# share's batch of 2, and one ragged case: a 64 x 64 latent, Cout neither a multiple of a tile width nor of 16.
CASES = {
    "960->320@32": (8, 32, 32, 320, 320, 960),
    "1920->1280@8": (8, 8, 8, 1280, 1280, 1920),
    "2560->1280@4": (8, 4, 4, 1280, 1280, 2560),
    "2560->1280@8": (8, 8, 8, 1280, 1280, 2560),
    "640->1280@8": (8, 8, 8, 1280, 1280, 640),
    "960->320@32,B=2": (2, 32, 32, 320, 320, 960),
    "2560->1280@4,B=2": (2, 4, 4, 1280, 1280, 2560),
    "ragged@64": (1, 64, 64, 64, 72, 96),
    # [W2 | Wsk] shares ONE pack scale (the two-launch path scales each matrix by itself): weights three orders of magnitude apart, with
    # the inputs scaled the other way so that both terms weigh the same in the output and lost low bits of the smaller matrix would show
    "Wsk*1e-3,x*1e3": (2, 8, 8, 64, 64, 96, 1.0, 1e-3),
    "W2*1e-3,a*1e3": (2, 8, 8, 64, 64, 96, 1e-3, 1.0),
}
_MADE = {}


class _Case:
    pass


def _make(hip, name):
    if name in _MADE:
        return _MADE[name]
    B, H, W, Ca, Co, Cx = CASES[name][:6]
    sw, swt = CASES[name][6:] or (1.0, 1.0)          # weight magnitudes (the inputs carry the inverse)
    c = _Case()
    c.B, c.H, c.W, c.Ca, c.Co, c.Cx, c.M = B, H, W, Ca, Co, Cx, B * H * W
    a = F.silu(torch.randn(B, Ca, H, W, generator=g(80))) / sw                  # conv2 reads SiLU(GroupNorm(h))
    x = (torch.randn(B, Cx, H, W, generator=g(81)) * 1.5 + 0.2) / swt
    w = torch.randn(Co, Ca, 3, 3, generator=g(82)) / math.sqrt(9 * Ca) * sw
    wt = torch.randn(Co, Cx, 1, 1, generator=g(83)) / math.sqrt(Cx) * swt
    b, bt = torch.randn(Co, generator=g(84)), torch.randn(Co, generator=g(85))
    ref = F.conv2d(a.double(), w.double(), b.double(), padding=1) + F.conv2d(x.double(), wt.double(), bt.double())
    c.ref = ref.permute(0, 2, 3, 1).reshape(c.M, Co).cuda()               # float64, on the GPU: the matrices below compare there
    c.ref_max = float(c.ref.abs().max())
    c.ap = hip.split_planes(a.permute(0, 2, 3, 1).reshape(c.M, Ca).contiguous().cuda())
    c.xp = hip.split_planes(x.permute(0, 2, 3, 1).reshape(c.M, Cx).contiguous().cuda())
    wd, wtd, bd, btd = w.cuda(), wt.cuda(), b.cuda(), bt.cuda()
    c.Wtail = hip.pack_conv3x3_tail(wd, bd, wtd, btd)
    c.Wconv, c.Wskip = hip.pack_conv3x3(wd, bd), hip.pack_linear(wtd, btd)
    c.conv = dict(B=B, Hin=H, Win=W, Cin=Ca, Hout=H, Wout=W, stride=1, upsample=0)
    c.ldo = (Co + 3) // 4 * 4
    c.ws = torch.empty(16 * 1024 * 1024, device="cuda")
    _MADE[name] = c
    return c


def _err(c, out):
    return float((out[:, :c.Co].double() - c.ref).abs().max()) / (c.ref_max + 1e-30)


def _tail(hip, c, **kw):
    out = torch.full((c.M, c.ldo), float("nan"), device="cuda")
    hip.gemm(c.ap, c.Wtail, out, workspace=c.ws, ldo=c.ldo, conv=c.conv, a2=c.xp, **kw)
    return out


def _two_launches(hip, c, prec):
    skip = torch.empty(c.M, c.ldo, device="cuda")
    hip.gemm(c.xp, c.Wskip, skip, prec=prec, workspace=c.ws, ldo=c.ldo)
    out = torch.full((c.M, c.ldo), float("nan"), device="cuda")
    hip.gemm(c.ap, c.Wconv, out, prec=prec, workspace=c.ws, ldo=c.ldo, conv=c.conv, res=skip)
    return out


def _desc(hip, c):
    """The problem as mvd_gemm_cfg_supported needs it."""
    d = hip.GemmDesc()
    d.M, d.N, d.K, d.a_mode, d.epi = c.M, c.Wtail.N, c.Wtail.K, hip.A_CONV3X3, hip.EPI_STORE
    d.B, d.Hin, d.Win, d.Cin, d.Hout, d.Wout, d.stride = c.B, c.H, c.W, c.Ca, c.H, c.W, 1
    d.tap_mode, d.Cin2, d.lda2 = hip.TAPS_CENTRE_TAIL, c.Cx, c.Cx
    return d


@pytest.mark.parametrize("prec", [4, 3, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_tail_matches_float64_and_the_two_launch_path(hip, name, prec):
    c = _make(hip, name)
    assert c.Wtail.K == 9 * c.Ca + c.Cx and c.Wtail.n_real == c.Co and c.Wtail.N == (c.Co + 15) // 16 * 16
    for splitk in (0, 1, 3):
        out = _tail(hip, c, prec=prec, splitk=splitk)
        old = _two_launches(hip, c, prec)
        e_new, e_old = _err(c, out), _err(c, old)
        e_pair = float((out[:, :c.Co].double() - old[:, :c.Co].double()).abs().max()) / (c.ref_max + 1e-30)
        print(f"[tap_schedule] {name} prec={prec} splitk={splitk}: tail {e_new:.3e}  two launches {e_old:.3e}  tail vs two launches {e_pair:.3e}")
        assert e_new < TOL[prec], (name, prec, splitk)
        assert e_old < TOL[prec] and e_pair < TOL[prec], (name, prec, splitk)
        assert torch.equal(out, _tail(hip, c, prec=prec, splitk=splitk))          # deterministic, split or not
        if c.Co % 32 == 0:          # the planes output of the same launch (a GEMM consumer's operand)
            op = hip.planes_like(c.M, c.Co, "cuda")
            out_p = torch.full((c.M, c.ldo), float("nan"), device="cuda")
            hip.gemm(c.ap, c.Wtail, out_p, prec=prec, workspace=c.ws, ldo=c.ldo, conv=c.conv, a2=c.xp, splitk=splitk, out_planes=op)
            assert _err(c, out_p) < TOL[prec] and rel_err(planes_to_float(op), out_p) < PL, (name, prec, splitk)


@pytest.mark.parametrize("name", list(CASES))
def test_tail_every_configuration(hip, name):
    """Every cfg mvd_gemm_cfg_supported admits, unsplit (bit-equal to each other: one k order) and with a forced split; the input-patch
    kernel declines the schedule and mvd_gemm rejects it by name."""
    c = _make(hip, name)
    d = _desc(hip, c)
    served = declined = 0
    base = None
    for cfg in hip.gemm_configs(hip.EPI_STORE, conv=True):
        if not hip.cfg_supported(d, cfg):
            assert cfg in hip.PATCH_CONFIGS, cfg
            with pytest.raises(RuntimeError, match="does not serve"):
                _tail(hip, c, prec=4, cfg=cfg, splitk=1)
            declined += 1
            continue
        served += 1
        for splitk in (1, 3):
            out = _tail(hip, c, prec=4, cfg=cfg, splitk=splitk)
            assert _err(c, out) < TOL[4], (name, cfg, splitk)
            if splitk == 1:
                base = out if base is None else base
                assert torch.equal(out, base), (name, cfg)
            else:
                assert torch.equal(out, _tail(hip, c, prec=4, cfg=cfg, splitk=splitk)), (name, cfg)
    assert served == len(hip.GEMM_CONFIGS) and declined == len(hip.PATCH_CONFIGS)


def _group_norm_ref(x, B, HW, C, gm, bt, silu=True):
    y = F.group_norm(x.view(B, HW, C).permute(0, 2, 1), 32, gm, bt, eps=1e-5).permute(0, 2, 1).reshape(B * HW, C)
    return F.silu(y) if silu else y


@pytest.mark.parametrize("name", ["960->320@32", "1920->1280@8", "2560->1280@4", "960->320@32,B=2"])
def test_tail_with_groupnorm_outputs(hip, name):
    """The launch's other writers: gn_stats alone, gna_out_sp (GroupNorm + SiLU behind the GEMM) and cat_b / cat_raw_sp (over the
    concatenation with a skip tensor), unsplit (tile epilogue + the library's apply launch) and split (the fused reduce), on the plain
    and the role-split kernel -- against mvd_groupnorm_from_stats / mvd_concat_groupnorm run on the fp32 result, and against F.group_norm."""
    c = _make(hip, name)
    B, HW, N, M = c.B, c.H * c.W, c.Co, c.M
    cb = 64 if N == 320 else 640           # the decoder's next concat: 320 + 64 = 12 channels per group, 1280 + 640 = 60
    gm, bt = torch.randn(N, generator=g(90)) + 1.0, torch.randn(N, generator=g(91))
    gmc, btc = torch.randn(N + cb, generator=g(92)) + 1.0, torch.randn(N + cb, generator=g(93))
    sk = (torch.randn(M, cb, generator=g(94)) * 1.5 + 0.3).cuda()
    gd, bd, gcd, bcd = gm.cuda(), bt.cuda(), gmc.cuda(), btc.cuda()
    L = hip.lib()
    assert L.mvd_concat_groupnorm_fits(N, cb, HW, 32)
    for cfg in (0, hip.make_cfg(1, hip.WS_LOOP)):
        for splitk in (1, 3):
            plain = _tail(hip, c, prec=3, cfg=cfg, splitk=splitk)
            assert _err(c, plain) < TOL[3]
            # ---- gn_stats alone
            st = torch.zeros(B, 32, 2, dtype=torch.int64, device="cuda")
            out = _tail(hip, c, prec=3, cfg=cfg, splitk=splitk, gn_stats=st, gn_hw=HW)
            assert _err(c, out) < TOL[3]
            y_st = hip.planes_like(M, N, "cuda")
            hip.groupnorm_from_stats(out, y_st, gd, bd, st, B, HW, N, 1e-5, True)
            want = _group_norm_ref(out.cpu(), B, HW, N, gm, bt)
            assert rel_err(planes_to_float(y_st), want) < PL + 4e-6, (name, cfg, splitk)
            # ---- gna_out_sp: the same planes from the GEMM's own launches
            st2 = torch.zeros_like(st)
            y = hip.planes_like(M, N, "cuda")
            y.fill_(0x7e00)
            out2 = _tail(hip, c, prec=3, cfg=cfg, splitk=splitk, gn_stats=st2, gn_hw=HW, gn_apply=(gd, bd, 1e-5, hip.GNA_SILU, y))
            assert _err(c, out2) < TOL[3]
            assert rel_err(planes_to_float(y), want) < PL + 4e-6, (name, cfg, splitk)
            assert rel_err(planes_to_float(y), planes_to_float(y_st)) < 2 * PL + 4e-6, (name, cfg, splitk)      # (two plane roundings)
            assert rel_err(st2.double(), st.double()) < 1e-5
            # ---- cat_b / cat_raw_sp: GroupNorm over [out | sk] against mvd_concat_groupnorm on the fp32 result
            st3 = torch.zeros_like(st)
            yc, raw = hip.planes_like(M, N + cb, "cuda"), hip.planes_like(M, N + cb, "cuda")
            out3 = _tail(hip, c, prec=3, cfg=cfg, splitk=splitk, gn_stats=st3, gn_hw=HW,
                         gn_apply=(gcd, bcd, 1e-5, hip.GNA_SILU, yc), cat=(sk, raw))
            assert _err(c, out3) < TOL[3]
            st4 = torch.zeros_like(st)
            yc2, raw2 = hip.planes_like(M, N + cb, "cuda"), hip.planes_like(M, N + cb, "cuda")
            hip.check(L.mvd_concat_groupnorm(hip.ptr(plain), N, hip.ptr(sk), cb, None, hip.ptr(raw2), hip.ptr(yc2), hip.ptr(gcd), hip.ptr(bcd),
                                             hip.ptr(st4), B, HW, 32, 1e-5, 1, hip.stream()))
            cat = torch.cat([plain.cpu(), sk.cpu()], 1)
            wantc = _group_norm_ref(cat, B, HW, N + cb, gmc, btc)
            assert rel_err(planes_to_float(yc), wantc) < PL + 4e-6, (name, cfg, splitk)
            assert rel_err(planes_to_float(yc), planes_to_float(yc2)) < 2 * PL + 4e-6, (name, cfg, splitk)
            assert rel_err(planes_to_float(raw), cat) < TOL[3] + PL and rel_err(planes_to_float(raw), planes_to_float(raw2)) < TOL[3] + 2 * PL, (name, cfg, splitk)
            assert rel_err(st3.double(), st4.double()) < 1e-5


def test_tail_rejects_what_it_does_not_serve(hip):
    c = _make(hip, "ragged@64")
    half = c.M // 4
    xp_half = c.xp[:half].contiguous()
    out = torch.empty(half, c.ldo, device="cuda")
    with pytest.raises(RuntimeError, match="centre-tap tail serves stride-1"):          # a strided convolution: the centre pixel is not row m
        hip.gemm(c.ap, c.Wtail, out, prec=3, ldo=c.ldo, a2=xp_half,
                 conv=dict(B=c.B, Hin=c.H, Win=c.W, Cin=c.Ca, Hout=c.H // 2, Wout=c.W // 2, stride=2, upsample=0))
    with pytest.raises(AssertionError):                                                  # a tail weight without its second operand
        hip.gemm(c.ap, c.Wtail, torch.empty(c.M, c.ldo, device="cuda"), prec=3, ldo=c.ldo, conv=c.conv)
    with pytest.raises(AssertionError):                                                  # ... and a second operand without a tail weight
        hip.gemm(c.ap, c.Wconv, torch.empty(c.M, c.ldo, device="cuda"), prec=3, ldo=c.ldo, conv=c.conv, a2=c.xp)
    d = _desc(hip, c)
    d.tap_mode = 1                                                                        # reserved, not served
    d.A, d.Wp, d.A2, d.out, d.ldo, d.prec = c.ap.data_ptr(), c.Wtail.data.data_ptr(), c.xp.data_ptr(), out.data_ptr(), c.ldo, 3
    assert hip.lib().mvd_gemm(hip.C.byref(d), hip.stream()) != 0
    assert b"tap_mode" in hip.lib().mvd_last_error()


def test_resblock_fuses_its_skip_convolution(hip):
    """ResBlock.run with a skip convolution launches two GEMMs (conv1, conv2 + tail) instead of three; a precision policy that sets the
    skip apart keeps the three-launch path, and the two agree within the GEMM tolerance (conv1 and both GroupNorms are the same launches)."""
    from mvdfusion_amd.engine import Ctx
    from mvdfusion_amd.unet import ResBlock
    torch.manual_seed(5)
    B, H, Ci, Co = 2, 8, 96, 64
    rb = ResBlock(Ci, 128, 0.0, out_channels=Co).cuda()
    x = (torch.randn(B * H * H, Ci) * 1.3).cuda()
    eb = torch.randn(1, Co).cuda()
    real, outs = hip.gemm, {}
    for policy, n in (("f16x3", 2), ("f16x3:skip=4", 3)):
        _, prec, pol = hip.parse_precision(policy)
        ctx = Ctx("cuda", prec=prec, policy=pol)
        ctx.B = B
        ctx.begin_step()
        ctx.emb_bias = {rb: eb}
        launches = []

        def counting(*a, **kw):
            launches.append(kw.get("a2") is not None)
            return real(*a, **kw)
        hip.gemm = counting
        try:
            outs[policy] = rb.run(ctx, x, H, H).clone()
        finally:
            hip.gemm = real
        assert len(launches) == n and sum(launches) == (1 if n == 2 else 0), (policy, launches)
    assert rel_err(outs["f16x3"], outs["f16x3:skip=4"]) < TOL[3]
