"""The GridAttn point geometry (csrc/gridattn_common.hpp) through its three kernels against a FLOAT64 reference (tests/gridattn_f64.py:
oracle/ref_torch.gridattn_tokens evaluated in float64 on the fp32 inputs the kernels receive; anchored to the reference's own fixtures
by tests/test_cpu_gridattn_f64.py).

  forward  : mvd_gridattn_tokens / _scenes_t / _window, every token column, per column family
  backward : mvd_gridattn_tokens_backward / _scenes / _window, every pixel and channel of both accumulators, against float64 autograd;
             row strides 512 and 736; gradients scaled by 2^-40, 2^20 and 2^-100 through backward_gridattn.fixed_point_scale
  fused    : g4_fused_kernel (its own sin / cos) and the unfused chain against oracle/ref_torch.gridattn_forward in float64

Cases (kept small; x = 0.5 N(0, 1), timesteps 981 / 21 clip most / few depth samples, so both clamp sides of the border rule and the
skipped tap beyond the last row or column are hit): the GSO rig every other test uses; GENERAL rigs (fy ~ 1.3 fx, +-20 % focal jitter,
principal points up to +-0.15, an extra rotation, translation jitter: gridattn_f64.make_rig); a general rig with every length (camera
translations, depth_scale, depth_shift) scaled by 20, which multiplies the harmonic arguments of the moment / distance / depth
embeddings by 20 (up to ~320 rad); two scenes with a step row each; a query-view shard; windows W < V and W > V.

Bounds -- none of them taken from what the kernels give:
  forward, per family over the kept rows :  max|kernel - f64| <= M max|fp32 oracle - f64| + PL max|f64|
  backward, per accumulator              :  max|acc / scale - f64 grad| <= M max|fp32 autograd - f64 grad| + 0.5 (4 rows) / scale
  fused, per output                      :  max|out - f64| <= M max|fp32 oracle forward - f64| + PL max|f64|
with M = 4 (kernel and oracle are two fp32 evaluation orders of the same formulas, with different sin / cos), PL the split-plane
representation error of tests/test_gpu_ops.py, and 0.5 / scale the rounding of one of at most 4 x rows contributions to a texel.
Exclusion rule: a (point, camera) pair with |z| < 0.1 x rig distance in float64 is left out (the projection is ill-conditioned there and
the border it hits is decided by the last bit); at most 1 % of a case's pairs may be, asserted before anything else; an excluded
reference pair removes its row's sample columns (and zeroes its dtok block), an excluded input-view pair the point's rows.

Measured on an MI355X, kernel error / fp32-oracle error (the bound allows 4 + the PL or quantisation term):
  forward          |   ref samples | input samples |   ref Plucker |  ref distance | query Plucker |   query depth
  gso_v4           |          0.74 |          1.00 |          1.00 |          1.00 |          1.08 |          0.99
  general_v3       |          1.00 |          1.02 |          0.96 |          0.96 |          0.91 |          1.00
  general_v5_s12   |          0.93 |          1.00 |          0.99 |          0.99 |          1.00 |          1.00
  general_v1_d3    |          1.00 |          1.00 |          0.86 |          1.00 |          1.02 |          1.02
  general_x20_v3   |          1.00 |          1.00 |          1.01 |          1.00 |          0.99 |          1.00
  two_scenes_v3    |          0.99 |          1.00 |          0.96 |          0.96 |          0.91 |          1.02
  shard_v4_q1      |          1.23 |          1.00 |          1.11 |          0.99 |          1.17 |          1.02
  window_v8_w5     |          1.00 |          1.00 |          0.98 |          0.99 |          0.99 |          1.02
  window_v3_w5     |          1.00 |          1.00 |          0.97 |          0.99 |          1.02 |          0.99

  backward (ldt = 512 and 736 give the same figures; so do the gradients scaled by 2^-40, 2^20 and 2^-100 on general_v3 and
  window_v3_w5 -- at 2^-100 the quantisation term is 1.4e-35 next to an oracle error of 8.6e-36, everywhere else it is < 1e-3 of it)
                   | dfeat | din_feat
  gso_v4           |  0.84 |     1.11
  general_v3       |  0.97 |     1.00
  general_v5_s12   |  0.89 |     0.98
  general_v1_d3    |  1.00 |     1.04
  general_x20_v3   |  1.00 |     1.00
  two_scenes_v3    |  0.98 |     1.01
  shard_v4_q1      |  0.96 |     0.98
  window_v8_w5     |  1.01 |     0.93
  window_v3_w5     |  1.01 |     0.96

  GridAttn.run     | fused x4 | unfused x4 | fused x3
  general_x20      |     1.00 |       1.00 |     1.00
  general          |     1.02 |       0.99 |     0.98

No family needs more than 1.23.  Ratios of 1.00 are expected: the largest error of a case sits at one badly conditioned point, where
kernel and oracle round the same fp32 world point and differ only after it.  At the 20x rig the oracle's own error is 20 - 200 times
larger than at the unit rigs (2e-4 on the samples, 7e-4 on the moment embedding: fp32 coordinates of size 50 under sin / cos at up
to 6.4 rad per unit), so that case proves the large-argument sin / cos paths agree with float64 to fp32 rounding of the ARGUMENT, not
more.
"""
import functools

import pytest
import torch

import gridattn_f64 as G
from conftest import build_model, planes_to_float
from test_gpu_ops import PL

pytestmark = pytest.mark.gpu

# name: (V, S, D, general rig, timesteps, seed, extra arguments of gridattn_f64.make_case)
CASES = {
    "gso_v4": (4, 8, 2, False, [21], 1, {}),
    "general_v3": (3, 8, 2, True, [981], 0, {}),
    "general_v5_s12": (5, 12, 1, True, [981], 0, {}),
    "general_v1_d3": (1, 8, 3, True, [21], 0, {}),
    "general_x20_v3": (3, 8, 2, True, [981], 3, dict(length_scale=20.0)),
    "two_scenes_v3": (3, 8, 2, True, [999, 10], 0, dict(per_scene_steps=True)),
    "shard_v4_q1": (4, 8, 2, True, [981], 3, dict(q0=1, Vq=3)),
    "window_v8_w5": (8, 12, 1, True, [981], 1, dict(window=5)),
    "window_v3_w5": (3, 8, 2, True, [21], 2, dict(window=5)),
}
LDTS = (512, 736)


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


@functools.lru_cache(maxsize=None)
def _case(name):
    """(case, f64 reference with gradients, fp32 oracle with gradients, (bad_ref, bad_in), dtok (T, 736)) -- computed once per case and
    shared, read-only, by the tests below.  The exclusion cap is asserted here, before any comparison."""
    V, S, D, general, ts, seed, kw = CASES[name]
    case = G.make_case(V, S, D, general, ts, seed=seed, **kw)
    with torch.no_grad():
        bad = G.excluded(case, G.reference(case))
    dtok = torch.randn(case.npts * case.slots, 736, generator=torch.Generator().manual_seed(97))
    G.zero_excluded(dtok, *bad)
    return case, G.reference(case, dtok), G.reference(case, dtok, dtype=torch.float32), bad, dtok


def _geo(hip, case):
    cams, in_cam = case.packed()
    S = case.S
    dev = dict(x=case.x, dn=case.depth_noise, steps=case.steps, it=torch.full((1,), case.it, dtype=torch.int32),
               lin=torch.linspace(1.0 - 1.0 / S, -1.0 + 1.0 / S, S), cams=cams, in_cam=in_cam, feat=case.feat, in_feat=case.in_feat)
    return {k: v.contiguous().cuda() for k, v in dev.items()}


def _entry(case):
    """The narrowest entry point that can express the case: all three of a family are exercised across the cases."""
    return "window" if case.window else "scenes" if case.nscene > 1 else "plain"


def _tokens(hip, case, q, entry):
    L = hip.lib()
    T = case.npts * case.slots
    tok = hip.planes_like(T, hip.TOKEN_LD, "cuda")
    head = [hip.ptr(q[k]) for k in ("x", "dn", "steps", "it", "lin", "feat", "in_feat", "cams", "in_cam")] + [hip.ptr(tok)]
    shape = (case.V, case.q0, case.Vq, case.S, case.D, float(case.depth_scale), float(case.depth_shift))
    if entry == "plain":
        assert case.nscene == 1 and not case.window
        rc = L.mvd_gridattn_tokens(*head, *shape, hip.stream())
    elif entry == "scenes":
        assert not case.window
        rc = L.mvd_gridattn_tokens_scenes_t(*head, case.nscene, *shape, case.steps_scene_stride, hip.stream())
    else:
        rc = L.mvd_gridattn_tokens_window(*head, case.nscene, *shape, case.steps_scene_stride, case.window, hip.stream())
    hip.check(rc)
    torch.cuda.synchronize()
    return tok


def _backward(hip, case, q, dtok, scale, entry):
    """acc (nscene * V, S, S, 256), acc_in (nscene, S, S, 256) int64 of one launch; dtok (T, ldt) contiguous on the device."""
    L = hip.lib()
    assert dtok.is_contiguous() and dtok.shape[0] == case.npts * case.slots
    acc = torch.zeros(case.nscene * case.V, case.S, case.S, 256, dtype=torch.int64, device="cuda")
    acc_in = torch.zeros(case.nscene, case.S, case.S, 256, dtype=torch.int64, device="cuda")
    head = [hip.ptr(q[k]) for k in ("x", "dn", "steps", "it", "lin", "cams", "in_cam")] + \
        [hip.ptr(dtok), dtok.shape[1], hip.ptr(acc), hip.ptr(acc_in), float(scale)]
    shape = (case.V, case.q0, case.Vq, case.S, case.D, float(case.depth_scale), float(case.depth_shift))
    if entry == "plain":
        assert case.nscene == 1 and not case.window
        rc = L.mvd_gridattn_tokens_backward(*head, *shape, hip.stream())
    elif entry == "scenes":
        assert not case.window
        rc = L.mvd_gridattn_tokens_backward_scenes(*head, case.nscene, *shape, case.steps_scene_stride, hip.stream())
    else:
        rc = L.mvd_gridattn_tokens_backward_window(*head, case.nscene, *shape, case.steps_scene_stride, case.window, hip.stream())
    hip.check(rc)
    torch.cuda.synchronize()
    return acc, acc_in


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name", list(CASES))
def test_tokens_vs_float64(hip, name):
    case, ref, o32, (bad_ref, bad_in), _ = _case(name)
    if case.V > 1:          # the border rule is exercised: a projection outside the image clamps
        assert ref.outside >= 0.10, ref.outside
    tok = planes_to_float(_tokens(hip, case, _geo(hip, case), _entry(case))).double()
    assert tok.shape == (case.npts * case.slots, hip.TOKEN_LD)
    fails = []
    for fam, c0, c1 in G.FAMILIES:
        keep = G.family_rows(fam, bad_ref, bad_in)
        want = ref.tokens[keep, c0:c1]
        oracle_err = float((o32.tokens[keep, c0:c1].double() - want).abs().max())
        err = float((tok[keep, c0:c1] - want).abs().max())
        bound = G.MARGIN * oracle_err + PL * float(want.abs().max())
        print(f"RATIO forward {name} | {fam} | kernel {err:.2e} oracle {oracle_err:.2e} ratio {err / oracle_err:.2f} bound {bound:.2e} "
              f"rows {int(keep.sum())}/{keep.numel()} outside {ref.outside:.2f}")
        if not err <= bound:
            fails.append((fam, err, bound))
    assert not fails, fails
    assert bool((tok[:, 722] == 1.0).all()) and float(tok[:, 723:].abs().max()) == 0.0


def test_tokens_entry_points_agree(hip):
    """_scenes_t / _window with nscene = 1, window = 0 are the plain entry point, bit for bit."""
    case = _case("general_v3")[0]
    q = _geo(hip, case)
    plain = _tokens(hip, case, q, "plain")
    assert torch.equal(plain, _tokens(hip, case, q, "scenes")) and torch.equal(plain, _tokens(hip, case, q, "window"))


# ------------------------------------------------------------------------------------------------ backward
def _check_backward(hip, name, ldt, factor, tag):
    from mvdfusion_amd.backward_gridattn import fixed_point_scale
    case, ref, o32, _, dtok = _case(name)
    d = (dtok[:, :ldt] * factor).contiguous().cuda()
    scale = fixed_point_scale(float(d[:, :512].abs().max()))
    q = _geo(hip, case)
    acc, acc_in = _backward(hip, case, q, d, scale, _entry(case))
    acc2, acc_in2 = _backward(hip, case, q, d, scale, _entry(case))
    assert torch.equal(acc, acc2) and torch.equal(acc_in, acc_in2)          # integer atomics: order independent
    quant = 0.5 * 4 * d.shape[0] / scale
    fails = []
    for what, a, want, o in (("dfeat", acc, ref.dfeat, o32.dfeat), ("din_feat", acc_in, ref.din_feat, o32.din_feat)):
        # a power of two scales the reference exactly: the float64 / fp32 autograd of the unscaled gradient serves every factor
        oracle_err = factor * float((o.double() - want).abs().max())
        err = float((a.cpu().double() / scale - factor * want).abs().max())
        bound = G.MARGIN * oracle_err + quant
        print(f"RATIO backward {name} ldt={ldt} {tag} | {what} | kernel {err:.2e} oracle {oracle_err:.2e} ratio {err / oracle_err:.2f} "
              f"bound {bound:.2e} quant {quant:.1e} scale 2^{scale.hex().split('p')[1]} max|grad| {factor * float(want.abs().max()):.2e}")
        if not err <= bound:
            fails.append((what, err, bound))
    assert not fails, fails


@pytest.mark.parametrize("ldt", LDTS)
@pytest.mark.parametrize("name", list(CASES))
def test_tokens_backward_vs_float64_autograd(hip, name, ldt):
    _check_backward(hip, name, ldt, 1.0, "x1")


@pytest.mark.parametrize("exp", [-40, 20, -100])
@pytest.mark.parametrize("name", ["general_v3", "window_v3_w5"])
def test_tokens_backward_fixed_point_scale(hip, name, exp):
    """Token gradients far from O(1) through the scale rule of the training step: the same RELATIVE bound.  At 2^-100 the rule's exponent
    stops at 127 (a C float), so the largest gradient lands near 2^27 instead of 2^40."""
    _check_backward(hip, name, 512, 2.0 ** exp, f"x2^{exp}")


def test_tokens_backward_entry_points_agree(hip):
    """_scenes / _window with nscene = 1, window = 0 are the plain entry point, bit for bit."""
    case, _, _, _, dtok = _case("general_v3")
    q = _geo(hip, case)
    d = dtok.contiguous().cuda()
    plain = _backward(hip, case, q, d, 2.0 ** 38, "plain")
    for entry in ("scenes", "window"):
        got = _backward(hip, case, q, d, 2.0 ** 38, entry)
        assert torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1]), entry
    assert int(plain[0].abs().max()) > 0 and int(plain[1].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ fused kernel
@pytest.mark.parametrize("rig,length_scale,tval", [("general_x20", 20.0, 981), ("general", 1.0, 21)])
def test_gridattn_forward_vs_float64(hip, rig, length_scale, tval):
    """GridAttn.run (fused x4, unfused x4, fused x3) against oracle/ref_torch.gridattn_forward in float64 on the general rig and on the
    20x rig -- where the fused kernel's own sin / cos sees arguments in the hundreds.  Points with an excluded pair are left out."""
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.engine import Ctx
    from mvdfusion_amd.scheduler import make_tables
    from oracle import ref_torch as O
    V, S, D = 3, 16, 2
    ga = build_model(32, D=D).view_attn
    case = G.make_case(V, S, D, True, [tval], seed=40 + int(length_scale), length_scale=length_scale)
    case.feat, case.in_feat = torch.zeros_like(case.feat), torch.zeros_like(case.in_feat)      # (only the geometry is used from `case`)
    with torch.no_grad():
        bad_ref, bad_in = G.excluded(case, G.reference(case))
    keep = ~(bad_ref.any(1) | bad_in)
    g = torch.Generator().manual_seed(5)
    c = torch.randn(1, 256, generator=g) * 0.5
    input_latents = syn.make_inputs(V, S, 3)["input_latents"]
    tab = make_tables()
    t = torch.full((V,), tval, dtype=torch.long)

    def oracle(dtype):
        sd = {"view_attn." + k: v.detach().cpu().to(dtype) for k, v in ga.state_dict().items()}
        with torch.no_grad():
            out = O.gridattn_forward(sd, "view_attn.", case.x.to(dtype), G._cam_dict(case.cams, slice(0, V), dtype), c.to(dtype), t, tab,
                                     case.depth_noise[0].to(dtype), input_latents.to(dtype), G._cam_dict(case.in_cam, slice(0, 1), dtype),
                                     n_pts_per_ray=D, depth_scale=case.depth_scale, depth_shift=case.depth_shift)
        return out.reshape(-1, 768).double()[keep]

    want = oracle(torch.float64)
    oracle_err = float((oracle(torch.float32) - want).abs().max())
    bound = G.MARGIN * oracle_err + PL * float(want.abs().max())
    cams, in_cam = case.packed()
    args = (case.x.cuda(), case.depth_noise.cuda(), case.steps.cuda(), torch.zeros(1, dtype=torch.int32, device="cuda"), cams.cuda(),
            in_cam.cuda(), input_latents.cuda(), c.cuda())
    assert ga.fused_supported(V, V * S * S * D * V)
    saved = ga.depth_scale, ga.depth_shift
    fails = []
    try:
        ga.depth_scale, ga.depth_shift = case.depth_scale, case.depth_shift
        for what, prec, fused in (("fused x4", hip.PREC_X4, True), ("unfused x4", hip.PREC_X4, False), ("fused x3", hip.PREC_X3, True)):
            vol = torch.zeros(V * S * S * D, 768, device="cuda")
            ga.run(Ctx("cuda", prec=prec), *args, vol, V, S, D, fused=fused)
            err = float((vol.cpu().double()[keep] - want).abs().max())
            print(f"RATIO fused {rig} | {what} | kernel {err:.2e} oracle {oracle_err:.2e} ratio {err / oracle_err:.2f} bound {bound:.2e} "
                  f"max|f64| {float(want.abs().max()):.2f} points {int(keep.sum())}/{keep.numel()}")
            if not err <= bound:
                fails.append((what, err, bound))
    finally:
        ga.depth_scale, ga.depth_shift = saved
    assert not fails, fails
