"""The GEMM family (csrc/gemm.hip, gemm_device.hpp, gemm_plain*.hip, gemm_patch.hip, gemm_ws.hip) and the weight packers against FLOAT64
PER ELEMENT (tests/gemm_f64.py: oracles, fixtures, bars, case lists), through hip.gemm and the C ABI, into sentinel-filled outputs with
four spare rows behind the result and the pitches of the `window` layout; spare rows and padding columns must keep their bits, in fp32
outputs, in planes outputs and behind the split-K slabs.  tests/test_cpu_gemm_f64.py shows that every mutant of gemm_f64.MUTANTS is
rejected by a (case, fixture) of the lists used here and that an fp32 emulation of the algorithm stays below half of every bar.

Every dense and convolution case x fixture x prec (4, 3, 1) runs with the library's own choice (cfg=None, splitk=0); the x4 leg also runs
under one configuration per (tile, loop) that mvd_gemm_cfg_supported accepts -- the dense cases crossed with the split counts 1, 2, 3, nk,
nk + 3, the convolutions with the split counts in rotation over the configurations (conftest.cfg_splitk_matrix).  On the `geometry`
fixtures the result equals the oracle bit for bit; elsewhere every element is under its bar and the per-tensor TOL[prec] of
tests/test_gpu_ops.py holds as before.  Every test prints its worst error / bar (pytest -s; the bar allows 1).

Found by these tests: nothing in the kernels.  Every geometry case is bit-exact under every configuration and split in both flavours, no
spare row, padding column or word behind the slabs was written, and the packers write the documented image with the documented hi / lo
split bit for bit.  hip.gemm gained ldr= (the residual's pitch was always res.shape[-1], so ldr != ldo could not be reached from Python).

Measured on an MI355X, worst error / bar of a family over its cases and fixtures (the bar allows 1); 176 tests, 3.1 s (fp16 flavour) /
3.5 s (bf16), next to the 2.3 s of tests/test_gpu_norm_f64.py.  x4 | x3 | x1 per flavour; the exact fixture: 0 everywhere.
                                              |    fp16 flavour     |    bf16 flavour
  dense store            plain                | 0.084  0.087  0.208 | 0.098  0.118  0.310
                         graded               | 0.295  0.295  0.266 | 0.096  0.088  0.306      fp16: the CPU emulation gives the same 0.295
                         cancel               | 0.048  0.052  0.268 | 0.078  0.081  0.175
    every cfg x split    plain, x4            | 0.073               | 0.080
    planes output        plain (fp32 next to) | 0.074  0.070  0.175 | 0.109  0.087  0.224      (0.073  0.076  0.176 | 0.080  0.081  0.224)
  GEGLU                                       | 0.028  0.027  0.173 | 0.062  0.044  0.187
  planes B operand, acc_scale                 | 0.073  0.075  0.161 | 0.066  0.065  0.211
  conv stride 1          plain|graded|cancel  | 0.057 0.114 0.022   x1 0.261 | 0.052 0.128 0.038   x1 0.282
  conv stride 2, padded                       | 0.034 0.086 0.018   x1 0.273 | 0.048 0.096 0.037   x1 0.242
  conv stride 2, no_pad_tl                    | 0.031 0.089 0.017   x1 0.202 | 0.035 0.083 0.036   x1 0.199
  conv nine-tap upsample                      | 0.040 0.086 0.027   x1 0.253 | 0.050 0.079 0.036   x1 0.184
  four-tap form                               | 0.069 0.174 0.034   x1 0.349 | 0.084 0.108 0.076   x1 0.344
  centre-tap tail                             | 0.037 0.099 0.022   x1 0.217 | 0.035 0.106 0.031   x1 0.227
  linear_backward        dx                   | 0.206  0.230  0.643 | 0.255  0.233  0.582
                         dW | db              | 0.073  0.059  0.217 | 0.043 | 0.073  0.066  0.189 | 0.043
  conv3x3_backward       dx                   | 0.049  0.072  0.360 | 0.107  0.097  0.323
                         dW | db              | 0.116  0.113  0.444 | 0.177 | 0.174  0.191  0.437 | 0.177
  packers                linear | _t | conv   | 0.500  0.500  0.543 | 0.479  0.479  0.495
Above half of the bar: linear_backward dx with one product at (130, 5, 32) -- the contraction runs over N = 5 terms, whose hi-only operand
roundings (2^-11 / 2^-8 each, the whole of that bar) do not average out over so few; the same element is at 0.21 / 0.26 with hi + lo.  The
packers sit at half by construction: the contract's 2^-22 / 2^-16 is the rounding of lo relative to the binade's lower end, and a
mantissa in the middle of the binade meets half of it (0.543: the 2^-25 absolute floor of a weight 1e-7 of the largest).
"""
import math

import pytest
import torch

import gemm_f64 as G
from conftest import cfg_splitk_matrix
from test_gpu_attention_f64 import read_out, sentinel_out
from test_gpu_norm_f64 import SENT32, f32_out
from test_gpu_ops import PL, TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


@pytest.fixture(scope="module")
def ws():
    return torch.empty(4 * 1024 * 1024, device="cuda")


def _fmt(hip):
    return "bf16" if hip.OPERAND_FORMAT == "bf16" else "f16"


def _ids(cases):
    return [G.case_id(c) for c in cases]


def _pad(n, q):
    return (n + q - 1) // q * q


def dev64(t):
    return t.double().cuda()


def judge(raw, M, N, ref, bar=None):
    """raw: int32 (M + 4, ld) sentinel-filled output after the launch; ref, bar: float64 on the GPU (bar None: the result must EQUAL ref).
    The four spare rows and the columns [N, ld) must keep their bits.  -> (worst error / bar | 0 or 1 for an exact fixture, max|err| / max|ref|)."""
    got = raw[:M, :N].view(torch.float32).double()
    intact = (raw[M:] == SENT32).all() & (raw[:M, N:] == SENT32).all()
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    if bar is None:
        worst = (err != 0).any().double()
    else:
        worst = torch.where(err == 0, torch.zeros_like(err), err / bar.clamp_min(1e-300)).max()
    rel = err.max() / ref.abs().max().clamp_min(1e-30)
    intact, worst, rel = torch.stack([intact.double(), worst, rel]).tolist()
    assert intact == 1.0, "rows behind the result or columns behind N were written"
    return worst, rel


class Worst:
    """Collects  error / bar  per key, prints them, demands <= 1 each (and the per-tensor tolerance next to it)."""

    def __init__(self, name):
        self.name, self.r = name, {}

    def add(self, key, worst, rel=None, tol=None, exact=False):
        if exact:
            assert worst == 0.0, (self.name, key, "not bit-equal to the oracle on the exact fixture")
        assert tol is None or rel < tol, (self.name, key, "per-tensor", rel, tol)
        self.r[key] = max(self.r.get(key, 0.0), worst)

    def done(self):
        for k, r in self.r.items():
            print(f"RATIO {self.name} {k}: {r:.3f}")
        bad = {k: r for k, r in self.r.items() if not r <= 1.0}
        assert not bad, (self.name, bad)


# ------------------------------------------------------------------------------------------------ dense MVD_EPI_STORE
class DenseRun:
    """The device side of one (case, fixture, layout): operands converted and packed once."""

    def __init__(self, hip, case, fixture, layout):
        M, N, K = case
        self.hip, self.case, self.fixture = hip, case, fixture
        self.fx = fx = G.dense_fixture(fixture, M, N, K)
        self.lay = lay = G.dense_layout(fx, layout, M, N, K)
        self.Ap = hip.split_planes(lay["A_buf"].cuda())[:, 2 * lay["a_col0"]:]          # the column window of the wider planes buffer
        self.W = hip.pack_linear(fx["W"].cuda(), fx["bias"].cuda())
        self.res, self.bb = lay["res_buf"].cuda(), lay["bias_b_buf"].cuda()
        self.cs = torch.zeros(_pad(N, 16) + 16, device="cuda")
        self.cs[:N] = fx["colscale"].cuda()
        self.raw = f32_out(M, lay["ldo"])

    def terms(self, epi, rpb):
        return G.dense_terms(self.fx["A"], self.fx["W"], layout=self.lay, **G.epilogue_args(self.fx, G.EPILOGUES[epi], rpb))

    def launch(self, epi, rpb, prec, ws, cfg=None, splitk=0, out_planes=None, out=True):
        M, N, K = self.case
        e, lay = G.EPILOGUES[epi], self.lay
        kw = dict(bias=bool(e.get("bias")), act=e.get("act", 0))
        if e.get("res"):
            kw.update(res=self.res, ldr=lay["ldr"])
        if e.get("colscale"):
            kw["colscale"] = self.cs
        if e.get("bias_b"):
            kw.update(bias_b=self.bb, rows_per_batch=rpb)
        self.raw.fill_(SENT32)
        self.hip.gemm(self.Ap, self.W, self.raw if out else None, M=M, lda=lay["lda"], ldo=lay["ldo"], prec=prec, workspace=ws, cfg=cfg, splitk=splitk,
                      out_planes=out_planes, **kw)
        return self.raw


@pytest.mark.parametrize("layout", G.LAYOUTS)
@pytest.mark.parametrize("fixture", G.DENSE_FIXTURES)
@pytest.mark.parametrize("case", G.DENSE_CASES, ids=_ids(G.DENSE_CASES))
def test_dense_store(hip, ws, case, fixture, layout):
    """Every option of the store epilogue, every rows_per_batch, prec 4 / 3 / 1, the library's own cfg and split."""
    M, N, K = case
    run, fmt, w = DenseRun(hip, case, fixture, layout), _fmt(hip), Worst(f"dense {G.case_id(case)} {fixture} {layout}")
    for epi, rpb in G.dense_epilogue_runs(M, fixture):
        t = run.terms(epi, rpb)
        ref = dev64(t["ref"])
        for prec in G.PRECS:
            bar = None if fixture == "geometry" else dev64(G.bar(t, fmt, prec, K // 32, 1, G.EPILOGUES[epi].get("act", 0)))
            worst, rel = judge(run.launch(epi, rpb, prec, ws), M, N, ref, bar)
            w.add(f"x{prec}", worst, rel, TOL[prec], exact=bar is None)
    w.done()


def _dense_desc(hip, M, N, K, epi=0, b_mode=0):
    d = hip.GemmDesc()
    d.M, d.N, d.K, d.a_mode, d.epi, d.b_mode = M, _pad(N, 16), _pad(K, 32), hip.A_DENSE, epi, b_mode
    return d


def slab_workspace(elems):
    """A workspace of exactly `elems` floats with 4096 sentinel words behind it: (the fp32 view to pass, the raw buffer to inspect)."""
    raw = torch.full((elems + 4096,), SENT32, dtype=torch.int32, device="cuda")
    return raw[:elems].view(torch.float32), raw


@pytest.mark.parametrize("case", G.DENSE_CASES, ids=_ids(G.DENSE_CASES))
def test_dense_every_configuration(hip, case):
    """x4 under one configuration per (tile, loop) the library accepts, crossed with the split counts 1, 2, 3, nk, nk + 3 (the last clamped):
    the exact fixture bit for bit, the plain one (window layout, bias + residual) under its bar; the slabs of a ragged last tile stay inside
    splits * M * N floats of the workspace."""
    M, N, K = case
    nk, fmt = K // 32, _fmt(hip)
    d = _dense_desc(hip, M, N, K)
    cfgs = [c for c in hip.GEMM_CONFIGS[::2] if hip.cfg_supported(d, c)]
    assert len(cfgs) >= 20, cfgs
    wsv, wsraw = slab_workspace(nk * M * _pad(N, 16))
    w = Worst(f"dense cfg x split {G.case_id(case)}")
    for fixture, layout, epi in (("geometry", "packed", "none"), ("plain", "window", "bias_res")):
        run = DenseRun(hip, case, fixture, layout)
        t = run.terms(epi, 0)
        ref = dev64(t["ref"])
        for sp in G.split_counts(nk):
            bar = None if fixture == "geometry" else dev64(G.bar(t, fmt, 4, nk, min(sp, nk)))
            for cfg in cfgs:
                worst, rel = judge(run.launch(epi, 0, 4, wsv, cfg=cfg, splitk=sp), M, N, ref, bar)
                w.add(fixture, worst, rel, TOL[4], exact=bar is None)
    assert bool((wsraw[nk * M * _pad(N, 16):] == SENT32).all()), "a split-K slab was written past splits * M * N"
    w.done()


@pytest.mark.parametrize("case", G.DENSE_CASES, ids=_ids(G.DENSE_CASES))
def test_dense_planes_output(hip, ws, case):
    """The split-planes output (alone, and next to the fp32 output) in a sentinel-filled buffer one 32-column block wider than the result."""
    M, N, K = case
    fmt, w = _fmt(hip), Worst(f"dense planes output {G.case_id(case)}")
    run = DenseRun(hip, case, "plain", "window")
    t = run.terms("bias_res", 0)
    ldp = _pad(N, 32) + 32
    for prec in G.PRECS:
        bar = G.bar(t, fmt, prec, K // 32, 1, planes_out=True, PL=PL)
        for with_out in (False, True):
            op = sentinel_out(M, ldp)
            raw = run.launch("bias_res", 0, prec, ws, out_planes=op, out=with_out)
            torch.cuda.synchronize()
            got = read_out(op, M, N)
            w.add(f"x{prec}", G.worst(got, t["ref"], bar))
            assert float((got.double() - t["ref"]).abs().max() / t["ref"].abs().max()) < TOL[prec] + PL
            if with_out:
                worst, rel = judge(raw, M, N, dev64(t["ref"]), dev64(G.bar(t, fmt, prec, K // 32, 1)))
                w.add(f"x{prec} fp32 alongside", worst, rel, TOL[prec])
            else:
                assert bool((raw == SENT32).all()), "the fp32 output was written although out is NULL"
    w.done()


# ------------------------------------------------------------------------------------------------ GEGLU, planes B operand
@pytest.mark.parametrize("case", G.GEGLU_CASES, ids=_ids(G.GEGLU_CASES))
def test_geglu(hip, ws, case):
    M, N, K = case
    fmt, h, w = _fmt(hip), N // 2, Worst(f"geglu {G.case_id(case)}")
    fx = G.dense_fixture("plain", M, N, K)
    t = G.dense_terms(fx["A"], fx["W"], bias=fx["bias"], geglu=True)
    ref = dev64(t["ref"])
    Ap = hip.split_planes(torch.cat([fx["A"], G._junk((G.SPARE_A_ROWS, K), "geglu", M, N, K)]).cuda())
    Wp = hip.pack_linear(fx["W"].cuda(), fx["bias"].cuda(), geglu=True)
    raw = f32_out(M, h + 8)
    cfgs = [c for c in hip.gemm_configs(hip.EPI_GEGLU)[::2] if hip.cfg_supported(_dense_desc(hip, M, N, K, hip.EPI_GEGLU), c)]
    for prec in G.PRECS:
        for cfg, sp in [(None, 0)] + (cfg_splitk_matrix(cfgs, G.split_counts(K // 32)) if prec == 4 else []):
            raw.fill_(SENT32)
            hip.gemm(Ap, Wp, raw, M=M, ldo=h + 8, prec=prec, epi=hip.EPI_GEGLU, workspace=ws, cfg=cfg, splitk=sp)
            worst, rel = judge(raw, M, h, ref, dev64(G.bar(t, fmt, prec, K // 32, max(1, min(sp, K // 32)), G.ACT_GELU)))
            w.add(f"x{prec}", worst, rel, TOL[prec])
    w.done()


@pytest.mark.parametrize("case", G.PLANES_CASES, ids=_ids(G.PLANES_CASES))
def test_planes_b_operand(hip, ws, case):
    """MVD_B_PLANES with acc_scale: B is columns [32, 32 + K) of a wider planes buffer with spare rows, both filled with +-3e4 elsewhere."""
    M, N, K = case
    fmt, w = _fmt(hip), Worst(f"planes B {G.case_id(case)}")
    fx = G.dense_fixture("plain", M, N, K)
    t = G.dense_terms(fx["A"], fx["W"], bias=fx["bias"], acc_scale=G.ACC_SCALE_PLANES, scale=1.0)
    ref = dev64(t["ref"])
    Ap = hip.split_planes(torch.cat([fx["A"], G._junk((G.SPARE_A_ROWS, K), "pa", M, N, K)]).cuda())
    Bbuf = G._junk((N + G.SPARE_A_ROWS, K + 64), "pb", M, N, K)
    Bbuf[:N, 32:32 + K] = fx["W"]
    Bop = hip.PlanesOperand(hip.split_planes(Bbuf.cuda())[:, 64:], N=N, K=K, bias=fx["bias"].cuda(), acc_scale=G.ACC_SCALE_PLANES, ld=K + 64)
    raw = f32_out(M, N + 8)
    cfgs = [c for c in hip.GEMM_CONFIGS[::2] if hip.cfg_supported(_dense_desc(hip, M, N, K, b_mode=1), c)]
    for prec in G.PRECS:
        for cfg, sp in [(None, 0)] + (cfg_splitk_matrix(cfgs, G.split_counts(K // 32)) if prec == 4 else []):
            raw.fill_(SENT32)
            hip.gemm(Ap, Bop, raw, M=M, ldo=N + 8, prec=prec, workspace=ws, cfg=cfg, splitk=sp)
            worst, rel = judge(raw, M, N, ref, dev64(G.bar(t, fmt, prec, K // 32, max(1, min(sp, K // 32)))))
            w.add(f"x{prec}", worst, rel, TOL[prec])
    w.done()


# ------------------------------------------------------------------------------------------------ convolutions
def _conv_dict(c):
    return dict(B=c.B, Hin=c.Hin, Win=c.Win, Cin=c.Cin, Hout=c.Hout, Wout=c.Wout, stride=c.stride, upsample=c.upsample, no_pad_tl=c.no_pad_tl)


def _conv_desc(hip, c, Wp):
    d = hip.GemmDesc()
    d.M, d.N, d.K, d.a_mode, d.epi = G.conv_M(c), Wp.N, Wp.K, hip.A_CONV3X3, hip.EPI_STORE
    for k, v in _conv_dict(c).items():
        setattr(d, k, v)
    if c.kind == "up4":
        d.tap_mode = hip.TAPS_UP4
    if c.tail:
        d.tap_mode, d.Cin2, d.lda2 = hip.TAPS_CENTRE_TAIL, c.tail, c.tail
    return d


class ConvRun:
    def __init__(self, hip, c, fixture):
        self.hip, self.c = hip, c
        self.fx = fx = G.conv_fixture(fixture, c)
        M = G.conv_M(c)
        x_rows = fx["x"].reshape(-1, c.Cin)
        self.xp = hip.split_planes(torch.cat([x_rows, G._junk((G.SPARE_A_ROWS, c.Cin), "cx", tuple(c))]).cuda())
        self.a2 = None
        wc, bc = fx["w"].cuda(), fx["bias"].cuda()
        if c.tail:
            self.a2 = hip.split_planes(torch.cat([fx["x2"], G._junk((G.SPARE_A_ROWS, c.tail), "cx2", tuple(c))]).cuda())[:M]
            self.W = hip.pack_conv3x3_tail(wc, bc, fx["wt"].cuda(), None)
        elif c.kind == "up4":
            self.W = hip.pack_conv3x3_up4(wc, bc)
        else:
            self.W = hip.pack_conv3x3(wc, bc)
        self.lay = {name: G.conv_res_layout(fx, c, name) for name in G.LAYOUTS}
        self.res = {name: self.lay[name]["res_buf"].cuda() for name in G.LAYOUTS}
        self.raw = {name: f32_out(M, self.lay[name]["ldo"]) for name in G.LAYOUTS}

    def launch(self, bias, res, layout, prec, ws, cfg=None, splitk=0):
        lay, raw = self.lay[layout], self.raw[layout]
        kw = dict(res=self.res[layout], ldr=lay["ldr"]) if res else {}
        raw.fill_(SENT32)
        self.hip.gemm(self.xp, self.W, raw, prec=prec, conv=_conv_dict(self.c), ldo=lay["ldo"], bias=bias, a2=self.a2, workspace=ws, cfg=cfg,
                      splitk=splitk, **kw)
        return raw


@pytest.mark.parametrize("fixture", G.CONV_FIXTURES)
@pytest.mark.parametrize("c", G.CONV_CASES, ids=_ids(G.CONV_CASES))
def test_conv(hip, c, fixture):
    """prec 4 / 3 / 1 with the library's own choice; x4 under every configuration the library accepts (the input-patch kernel where it serves
    the geometry), the split counts in rotation; a configuration it does not accept is refused by name before anything is launched."""
    fmt, M, N, nk = _fmt(hip), G.conv_M(c), c.Cout, G.conv_K(c) // 32
    run = ConvRun(hip, c, fixture)
    composed = c.kind == "up4"
    d = _conv_desc(hip, c, run.W)
    allc = hip.gemm_configs(hip.EPI_STORE, conv=True)[::2]
    cfgs = [cf for cf in allc if hip.cfg_supported(d, cf)]
    declined = [cf for cf in allc if cf not in cfgs]
    assert len(cfgs) >= 20 and all(cf in hip.PATCH_CONFIGS for cf in declined), (cfgs, declined)
    wsv, wsraw = slab_workspace(nk * M * run.W.N)
    w = Worst(f"conv {G.case_id(c)} {fixture}")
    for bias, res, layout in G.conv_runs(c, fixture):
        t = G.conv_terms(run.fx, c, bias=bias, res=res, layout=run.lay[layout] if res else None)
        ref = dev64(t["ref"])
        legs = [(prec, None, 0) for prec in G.PRECS]
        if fixture in ("geometry", "plain"):
            legs += [(4, cf, sp) for cf, sp in cfg_splitk_matrix(cfgs, G.split_counts(nk))]
        for prec, cfg, sp in legs:
            bar = None if fixture == "geometry" else dev64(G.bar(t, fmt, prec, nk, max(1, min(sp, nk)), composed=composed))
            worst, rel = judge(run.launch(bias, res, layout, prec, wsv, cfg, sp), M, N, ref, bar)
            w.add(f"x{prec}" + (" cfgs" if cfg else ""), worst, rel, TOL[prec], exact=bar is None)
    assert bool((wsraw[nk * M * run.W.N:] == SENT32).all()), "a split-K slab was written past splits * M * N"
    if declined:
        with pytest.raises(RuntimeError, match="does not serve"):
            run.launch(True, False, "packed", 4, wsv, declined[0], 1)
        assert bool((run.raw["packed"] == SENT32).all())
    if c.kind == "s1" and (c.Hin * c.Win) % 128 == 0 and 128 % c.Win == 0:
        assert any(cf in hip.PATCH_CONFIGS for cf in cfgs), "the input-patch kernel serves a tile of whole image rows"
    w.done()


# ------------------------------------------------------------------------------------------------ backward
def _bw_terms(ref_S, F):
    return dict(ref=ref_S[0], S=ref_S[1], F=F)


def _grad_scale(dy):
    return G.pack_scale(dy)          # backward._pow2_scale: the power of two that brings max|dy| to [1024, 2048)


@pytest.mark.parametrize("case", G.LINEAR_BACKWARD_CASES, ids=_ids(G.LINEAR_BACKWARD_CASES))
def test_linear_backward(hip, ws, case):
    """dx = dy W (operands dy * s and the packed W^T), dW = dy^T x (two activation operands, K = the M rows), db = the column sums.  The floor:
    2^-25 per element of dy * s, of W * scale and of x."""
    from mvdfusion_amd import backward
    M, N, K = case
    fmt, w = _fmt(hip), Worst(f"linear_backward {G.case_id(case)}")
    g = G._gen("lbw", M, N, K)
    x, wt, dy = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K), 1e-4 * torch.randn(M, N, generator=g)
    xp = hip.split_planes(x.cuda(), ldp=_pad(K, 32))
    r = G.linear_backward_ref(x, wt, dy)
    s, sw = _grad_scale(dy), G.pack_scale(wt)
    F = dict(dx=wt.double().abs().sum(0)[None, :] / s + dy.double().abs().sum(1)[:, None] / sw,
             dW=x.double().abs().sum(0)[None, :] / s + dy.double().abs().sum(0)[:, None], db=torch.zeros(N, dtype=torch.float64))
    nk = dict(dx=_pad(N, 32) // 32, dW=_pad(M, 32) // 32)
    for prec in G.PRECS:
        dx, dW, db = backward.linear_backward(xp, wt.cuda(), dy.cuda(), ws, prec=prec)
        torch.cuda.synchronize()
        for name, got in (("dx", dx), ("dW", dW)):
            t = _bw_terms(r[name], F[name])
            w.add(f"{name} x{prec}", G.worst(got, t["ref"], G.bar(t, fmt, prec, nk[name], 1)))
            assert float((got.double().cpu() - t["ref"]).abs().max() / t["ref"].abs().max()) < TOL[prec]
        w.add("db", G.worst(db, r["db"][0], 2.0 * G.U24 * r["db"][1]))          # summed in fp64, rounded once (tests/norm_f64.py: col_sum_bar)
    w.done()


@pytest.mark.parametrize("case", G.CONV_BACKWARD_CASES, ids=_ids(G.CONV_BACKWARD_CASES))
def test_conv3x3_backward(hip, ws, case):
    from mvdfusion_amd import backward
    B, H, W, Cin, Cout = case
    M = B * H * W
    fmt, w = _fmt(hip), Worst(f"conv3x3_backward {G.case_id(case)}")
    g = G._gen("cbw", *case)
    x, wt = torch.randn(B, H, W, Cin, generator=g), torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    dy = 1e-4 * torch.randn(M, Cout, generator=g)
    xp = hip.split_planes(x.reshape(M, Cin).cuda(), ldp=_pad(Cin, 32))
    r = G.conv3x3_backward_ref(x, wt, dy, B, H, W)
    s, sw = _grad_scale(dy), G.pack_scale(wt)
    ones = G.conv3x3_backward_ref(torch.ones_like(x), wt.abs(), torch.ones_like(dy), B, H, W)          # sum |w| over the taps that reach a pixel
    absd = G.conv3x3_backward_ref(x.abs(), torch.ones_like(wt), dy.abs(), B, H, W)                      # sum |dy| over them; sum |x| per tap
    F = dict(dx=ones["dx"][0] / s + absd["dx"][0] / sw,
             dW=G.conv3x3_backward_ref(x.abs(), wt, torch.ones_like(dy), B, H, W)["dW"][0] / s + dy.double().abs().sum(0).view(-1, 1, 1, 1).expand(Cout, Cin, 3, 3))
    nk = dict(dx=9 * _pad(Cout, 32) // 32, dW=_pad(M, 32) // 32)
    for prec in G.PRECS:
        dx, dW, db = backward.conv3x3_backward(xp, wt.cuda(), dy.cuda(), B, H, W, ws, prec=prec)
        torch.cuda.synchronize()
        for name, got in (("dx", dx), ("dW", dW)):
            t = _bw_terms(r[name], F[name])
            w.add(f"{name} x{prec}", G.worst(got, t["ref"], G.bar(t, fmt, prec, nk[name], 1)))
            assert float((got.double().cpu() - t["ref"]).abs().max() / t["ref"].abs().max()) < TOL[prec]
        w.add("db", G.worst(db, r["db"][0], 2.0 * G.U24 * r["db"][1]))
    w.done()


# ------------------------------------------------------------------------------------------------ packed images against the header
def _check_image(hip, Wp, m, N, K, name):
    """Wp: PackedWeight; m: the (N, K) fp32 matrix whose image it is.  hi + lo == m * scale within the contract, hi and lo are the split of
    csrc/common.hpp bit for bit, the padding is exactly 0."""
    fmt, scale = _fmt(hip), 1.0 / Wp.acc_scale
    assert scale == G.pack_scale(m)
    torch.cuda.synchronize()
    hi, lo = G.decode_packed(Wp.data.cpu().view(torch.int16), N, K, fmt)
    assert tuple(hi.shape) == (Wp.N, Wp.K), name
    pad = torch.ones_like(hi, dtype=torch.bool)
    pad[:N, :K] = False
    assert bool((hi[pad] == 0).all()) and bool((lo[pad] == 0).all()), f"{name}: padding is not zero"
    err = ((hi + lo)[:N, :K].double() - m.double() * scale).abs()
    r = float((err / G.pack_bar(m, scale, fmt)).max())
    h, l = G.split_op(m * scale, fmt)
    assert torch.equal(hi[:N, :K], h) and torch.equal(lo[:N, :K], l), f"{name}: not the documented hi / lo split"
    return r


def test_packed_images_match_the_header(hip):
    w = Worst("packers")
    for N, K in G.PACK_LINEAR_CASES:
        m = torch.randn(N, K, generator=G._gen("pack", N, K)) * 3.0
        m[0, 0] = 1e-7 * float(m.abs().max())          # (a weight far below the 2^-13 window: the absolute floor)
        w.add("pack_linear", _check_image(hip, hip.pack_linear(m.cuda()), m, N, K, f"pack_linear {N}x{K}"))
        w.add("pack_linear_t", _check_image(hip, hip.pack_linear_t(m.t().contiguous().cuda()), m, N, K, f"pack_linear_t {N}x{K}"))
    for Cout, Cin in G.PACK_CONV_CASES:
        cw = torch.randn(Cout, Cin, 3, 3, generator=G._gen("packc", Cout, Cin))
        cin_pad = _pad(Cin, 32)
        w.add("pack_conv3x3", _check_image(hip, hip.pack_conv3x3(cw.cuda()), G.conv_weight_matrix(cw, cin_pad), Cout, 9 * cin_pad, f"pack_conv3x3 {Cout}x{Cin}"))
    w.done()


# ------------------------------------------------------------------------------------------------ refusals
def test_documented_refusals(hip, ws):
    """What include/mvd_hip.h says mvd_gemm refuses is refused by the host-side argument checks, by name, and nothing is written."""
    c = G.CONV_CASES[10]                                            # stride 2
    assert c.stride == 2
    run = ConvRun(hip, c, "plain")
    patch = hip.make_cfg(1, hip.PATCH_LOOP)
    with pytest.raises(RuntimeError, match="does not serve"):      # the input-patch kernel on a stride-2 convolution
        run.launch(True, False, "packed", 4, ws, patch, 1)
    dr = DenseRun(hip, (65, 80, 96), "plain", "window")
    with pytest.raises(RuntimeError, match="does not serve"):      # ... on a dense problem
        dr.launch("bias", 0, 4, ws, cfg=patch, splitk=1)
    for loop in hip.REMOVED_LOOPS:
        with pytest.raises(RuntimeError, match="does not serve"):
            dr.launch("bias", 0, 4, ws, cfg=hip.make_cfg(1, loop), splitk=1)
    with pytest.raises(RuntimeError, match="ldr"):                 # a residual pitch that is no multiple of 4 floats
        hip.gemm(dr.Ap, dr.W, dr.raw, M=65, lda=dr.lay["lda"], ldo=dr.lay["ldo"], res=dr.res, ldr=81, workspace=ws)
    with pytest.raises(RuntimeError, match="ldo"):
        hip.gemm(dr.Ap, dr.W, dr.raw, M=65, lda=dr.lay["lda"], ldo=81, workspace=ws)
    with pytest.raises(RuntimeError, match="lda"):                 # a window narrower than K
        hip.gemm(dr.Ap, dr.W, dr.raw, M=65, lda=96 + 16, ldo=dr.lay["ldo"], workspace=ws)
    up = ConvRun(hip, [x for x in G.CONV_CASES if x.kind == "up4"][0], "plain")
    with pytest.raises(RuntimeError, match="four-tap form"):       # the four-tap form takes no residual
        up.launch(True, True, "window", 4, ws)
    tail = [x for x in G.CONV_CASES if x.tail][0]
    tr = ConvRun(hip, tail, "plain")
    with pytest.raises(RuntimeError, match="does not serve"):      # the centre-tap tail: every cfg except the input-patch kernel
        tr.launch(True, False, "packed", 4, ws, hip.make_cfg(2, hip.PATCH_LOOP), 1)
    tr.c = tail._replace(stride=2)
    with pytest.raises(RuntimeError, match="centre-tap tail"):     # ... and stride-1 convolutions only
        tr.launch(True, False, "packed", 4, ws)
    torch.cuda.synchronize()
    for r in (run.raw["packed"], dr.raw, up.raw["window"], tr.raw["packed"]):
        assert bool((r == SENT32).all()), "a refused call wrote to its output"
