"""View fusion on the GPU: mvd_fuse_points / mvd_compact_points (csrc/fusion.hip) through the C ABI against the float64 reference of
tests/fusion_f64.py, and the host path (mvdfusion_amd/fusion.py, ViewFusion.fuse).

Bounds -- none taken from what the kernels give:
  xyz             max|kernel - f64| <= 4 max|fp32 oracle - f64| + 2^-23 max|f64|   (two fp32 evaluation orders of the same formulas, plus
                  one rounding of the result)
  support/conflict  EQUAL to float64 on every compared point (fusion_f64.undecidable: pairs within the fp32 oracle's own error of one of
                  the rule's comparisons are left out, at most 1 % of a case's pairs, asserted first)
  colour, compaction, determinism: bit equality.
Both forms of the fuse kernel (global reads, LDS-staged) run every parity case and must give the same bits.

Measured on an MI355X: xyz kernel error / fp32-oracle error = 1.00 on all six cases (1.5e-7 ... 2.5e-7 against bounds of 7.4e-7 ... 1.2e-6:
kernel and oracle round the same fp32 operations), no count mismatch on 192 / 762 / 720 / 4096 / 384 / 256 compared points; sphere:
| |X| - 0.6 | = 9.5e-8 (bound 9.6e-7), no conflicts, 0.951 of the foreground kept in every view.
"""
import functools

import pytest
import torch

import fusion_f64 as F
from conftest import build_model

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


@functools.lru_cache(maxsize=None)
def _refs(name):
    """(case, float64 reference, fp32 oracle, undecidable pairs) -- computed once per case, shared read-only.  The cap is asserted here."""
    case = F.make_case(name)
    ref, o32 = F.reference(case), F.reference(case, torch.float32)
    return case, ref, o32, F.undecidable(case, ref, o32)[0]


@functools.lru_cache(maxsize=None)
def _sphere(pull_view=None):
    case = F.sphere_case(pull_view=pull_view)
    return case, F.reference(case), F.reference(case, torch.float32)


def _fuse(hip, case, rgb=None, stage=0, lat=None, color=True):
    """One mvd_fuse_points launch; every output buffer is pre-filled, the colour buffer is passed even without rgb."""
    n = case.npts
    dev = "cuda"
    out = dict(xyz=torch.full((n, 3), SENTINEL, device=dev), color=torch.full((n, 3), SENTINEL, device=dev) if color else None,
               support=torch.full((n,), 99, dtype=torch.uint8, device=dev), conflict=torch.full((n,), 99, dtype=torch.uint8, device=dev),
               flags=torch.full((n,), 99, dtype=torch.uint8, device=dev))
    lat = (case.lat if lat is None else lat).contiguous().cuda()
    cams, lin = case.packed().cuda(), F.ndc_lin(case.P).cuda()
    rc = hip.lib().mvd_fuse_points(hip.ptr(lat), hip.ptr(rgb), hip.ptr(cams), hip.ptr(lin), hip.ptr(out["xyz"]), hip.ptr(out["color"]),
                                   hip.ptr(out["support"]), hip.ptr(out["conflict"]), hip.ptr(out["flags"]), case.nscene, case.V, case.S,
                                   case.up, float(case.depth_scale), float(case.depth_shift), float(case.lo), float(case.hi),
                                   float(case.tau), stage, hip.stream())
    hip.check(rc)
    torch.cuda.synchronize()
    return out


def _compact(hip, fused, min_support, max_conflicts, color=True):
    """One mvd_compact_points call on the arrays of _fuse; outputs pre-filled with sentinels.  Returns (out dict, count)."""
    L = hip.lib()
    n = fused["support"].numel()
    dev = "cuda"
    out = dict(xyz=torch.full((n, 3), SENTINEL, device=dev), color=torch.full((n, 3), SENTINEL, device=dev) if color else None,
               support=torch.full((n,), 99, dtype=torch.uint8, device=dev), index=torch.full((n,), -5, dtype=torch.int32, device=dev))
    count = torch.full((1,), 12345, dtype=torch.int32, device=dev)
    nbytes = int(L.mvd_compact_points_scratch(n))
    scratch = torch.full((nbytes // 4,), -1, dtype=torch.int32, device=dev)
    rc = L.mvd_compact_points(hip.ptr(fused["xyz"]), hip.ptr(fused["color"]) if color else None, hip.ptr(fused["support"]),
                              hip.ptr(fused["conflict"]), hip.ptr(fused["flags"]), n, min_support, max_conflicts, hip.ptr(out["xyz"]),
                              hip.ptr(out["color"]), hip.ptr(out["support"]), hip.ptr(out["index"]), hip.ptr(count), hip.ptr(scratch), nbytes,
                              hip.stream())
    hip.check(rc)
    torch.cuda.synchronize()
    return out, int(count.item())


def _xyz_bound(ref, o32):
    return F.MARGIN * float((o32.xyz.double() - ref.xyz).abs().max()) + 2.0 ** -23 * float(ref.xyz.abs().max())


def _same(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------ 1. parity against float64
@pytest.mark.parametrize("name", list(F.CASES))
def test_fuse_points_vs_float64(hip, name):
    case, ref, o32, bad = _refs(name)
    keep = F.compared_points(bad)
    P = case.P
    rgb = torch.rand(case.nscene * case.V, 3, P, P, generator=torch.Generator().manual_seed(11)).cuda()
    got = _fuse(hip, case, rgb=rgb, stage=hip.FUSE_STAGE_GLOBAL)
    assert _same(got, _fuse(hip, case, rgb=rgb, stage=hip.FUSE_STAGE_LDS))           # the two forms of the kernel
    assert _same(got, _fuse(hip, case, rgb=rgb, stage=hip.FUSE_STAGE_AUTO))
    err, bound = float((got["xyz"].cpu().double() - ref.xyz).abs().max()), _xyz_bound(ref, o32)
    sup, con = got["support"].cpu().long(), got["conflict"].cpu().long()
    wrong = int(((sup != ref.support) | (con != ref.conflict))[keep].sum())
    print(f"RATIO fuse {name} | xyz kernel {err:.2e} oracle {float((o32.xyz.double() - ref.xyz).abs().max()):.2e} bound {bound:.2e} | "
          f"compared points {int(keep.sum())}/{keep.numel()} count mismatches {wrong} | foreground {float(ref.fg.float().mean()):.3f}")
    assert err <= bound, (err, bound)
    assert wrong == 0
    assert torch.equal(got["flags"].cpu() == hip.FUSE_FOREGROUND, ref.fg) and int(got["flags"].max()) <= hip.FUSE_FOREGROUND
    if case.V == 1:
        assert int(sup.sum()) == 0 and int(con.sum()) == 0
    # colour: the input pixel, bit for bit
    want = rgb.reshape(case.nscene * case.V, 3, P * P).permute(0, 2, 1).reshape(-1, 3)
    assert torch.equal(got["color"], want)
    # rgb = NULL: the colour buffer is not touched, everything else is the same
    plain = _fuse(hip, case, rgb=None, stage=hip.FUSE_STAGE_GLOBAL)
    assert bool((plain["color"] == SENTINEL).all())
    assert all(torch.equal(plain[k], got[k]) for k in ("xyz", "support", "conflict", "flags"))


# ------------------------------------------------------------------------------------------------ 2. sphere known answer
def _kept(out):
    return (out["flags"] == 1) & (out["support"] >= 1) & (out["conflict"] <= 0)


def test_sphere_known_answer(hip):
    case, ref, o32 = _sphere()
    V, n = case.V, case.P * case.P
    got = _fuse(hip, case)
    keep = _kept(got).cpu()
    bound = _xyz_bound(ref, o32)
    radial = float((got["xyz"].cpu().double()[keep].norm(dim=1) - F.SPHERE_R).abs().max())
    fg = (got["flags"].cpu() == 1).reshape(V, n)
    share = keep.reshape(V, n).sum(1).double() / fg.sum(1).double()
    print(f"sphere: | |X| - r | {radial:.2e} (bound {bound:.2e}), conflicts {int(got['conflict'].cpu()[ref.fg].sum())}, kept share per view "
          f"{[round(float(s), 3) for s in share]}")
    assert radial <= bound
    assert int(got["conflict"].cpu()[ref.fg].sum()) == 0
    assert torch.equal(fg.reshape(-1), ref.fg) and float(share.min()) >= 0.9

    # view 1's surface 0.3 nearer its camera: it loses every point, the views that do not border it are unchanged
    case2, _, _ = _sphere(1)
    keep2 = _kept(_fuse(hip, case2)).cpu().reshape(V, n)
    keep = keep.reshape(V, n)
    assert int(keep2[1].sum()) == 0
    for v in (3, 4, 5, 6, 7):
        assert torch.equal(keep2[v], keep[v]), v
    for v in (0, 2):
        assert bool((keep2[v] <= keep[v]).all()), v


# ------------------------------------------------------------------------------------------------ 3. compaction
def _random_case(V, S, up, seed):
    from gridattn_f64 import make_rig
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(V, 5, S, S, generator=g)
    lat[:, 4] *= 0.5
    return F.Case(lat=lat, cams=make_rig(V, True, seed)[0], V=V, S=S, up=up)


@pytest.mark.parametrize("V,S,up", [(3, 5, 1), (4, 32, 1), (2, 32, 8)], ids=["n75", "n4096", "n131072"])
def test_compact_points_is_masked_selection(hip, V, S, up):
    case = _random_case(V, S, up, seed=V * 100 + S)
    P, n = case.P, case.npts
    assert n == {5: 75, 32: 4096 if up == 1 else 131072}[S]
    rgb = torch.rand(V, 3, P, P, generator=torch.Generator().manual_seed(5)).cuda()
    fused = _fuse(hip, case, rgb=rgb)
    fg = fused["flags"] == 1
    assert 0 < int(fg.sum()) < n
    for min_support, max_conflicts in ((1, 0), (0, 255), (0, 0), (1, 1)):
        mask = fg & (fused["support"] >= min_support) & (fused["conflict"] <= max_conflicts)
        want_n = int(mask.sum())
        out, count = _compact(hip, fused, min_support, max_conflicts)
        assert count == want_n, (min_support, max_conflicts, count, want_n)
        if (min_support, max_conflicts) == (0, 255):
            assert count == int(fg.sum())                                # min_support = 0 keeps all foreground
        assert torch.equal(out["index"][:count].long(), torch.nonzero(mask).reshape(-1))
        assert torch.equal(out["xyz"][:count], fused["xyz"][mask]) and torch.equal(out["color"][:count], fused["color"][mask])
        assert torch.equal(out["support"][:count], fused["support"][mask])
        # rows past the count are not touched
        assert bool((out["xyz"][count:] == SENTINEL).all()) and bool((out["color"][count:] == SENTINEL).all())
        assert bool((out["support"][count:] == 99).all()) and bool((out["index"][count:] == -5).all())
        again, count2 = _compact(hip, fused, min_support, max_conflicts)
        assert count2 == count and _same(out, again)                     # two runs: the same bits
    assert any(int((fg & (fused["support"] >= 1) & (fused["conflict"] <= c)).sum()) > 0 for c in (0, 1))
    # min_support = 255 keeps none: count 0, outputs untouched
    out, count = _compact(hip, fused, 255, 255)
    assert count == 0 and bool((out["xyz"] == SENTINEL).all()) and bool((out["index"] == -5).all()) and bool((out["support"] == 99).all())
    # without colour
    out, count = _compact(hip, fused, 0, 255, color=False)
    assert count == int(fg.sum()) and torch.equal(out["xyz"][:count], fused["xyz"][fg])


# ------------------------------------------------------------------------------------------------ 4. bad arguments
def test_bad_arguments_return_an_error(hip):
    L = hip.lib()
    case = F.make_case("general_v3_s8")
    n = case.npts
    lat, cams, lin = case.lat.cuda(), case.packed().cuda(), F.ndc_lin(case.P).cuda()
    xyz, color = torch.zeros(n, 3, device="cuda"), torch.zeros(n, 3, device="cuda")
    sup, con, fl = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(3))
    rgb = torch.zeros(case.V, 3, case.P, case.P, device="cuda")
    good = dict(lat=lat, rgb=None, cams=cams, lin=lin, xyz=xyz, color=color, sup=sup, con=con, fl=fl, nscene=1, V=case.V, S=case.S, up=1,
                ds=2.0, dsh=0.5, lo=0.02, hi=0.98, tau=0.05, stage=0)

    def fuse(**kw):
        a = dict(good)
        a.update(kw)
        p = hip.ptr
        return L.mvd_fuse_points(p(a["lat"]), p(a["rgb"]), p(a["cams"]), p(a["lin"]), p(a["xyz"]), p(a["color"]), p(a["sup"]), p(a["con"]),
                                 p(a["fl"]), a["nscene"], a["V"], a["S"], a["up"], a["ds"], a["dsh"], a["lo"], a["hi"], a["tau"], a["stage"],
                                 hip.stream())

    assert fuse() == 0
    for kw in (dict(lat=None), dict(cams=None), dict(lin=None), dict(xyz=None), dict(sup=None), dict(con=None), dict(fl=None),
               dict(rgb=rgb, color=None), dict(nscene=0), dict(V=0), dict(V=256), dict(S=1), dict(up=0), dict(up=-3), dict(lo=0.5, hi=0.5),
               dict(lo=0.9, hi=0.1), dict(tau=-0.01), dict(tau=float("nan")), dict(stage=3), dict(stage=-1),
               dict(V=255, S=32, up=128),                        # 255 * 4096^2 points: beyond 2^31
               dict(V=255, S=64, stage=hip.FUSE_STAGE_LDS)):      # 4 MiB of depth planes do not fit the LDS
        assert fuse(**kw) != 0, kw
        assert b"mvd_fuse_points" in L.mvd_last_error(), kw
    torch.cuda.synchronize()

    idx = torch.zeros(n, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    nbytes = int(L.mvd_compact_points_scratch(n))
    assert nbytes >= 4 * ((n + 255) // 256) and int(L.mvd_compact_points_scratch(1 << 20)) >= 4 * 4096
    scratch = torch.zeros(nbytes // 4, dtype=torch.int32, device="cuda")
    cgood = dict(xyz=xyz, color=color, sup=sup, con=con, fl=fl, n=n, ms=1, mc=0, oxyz=xyz.clone(), ocolor=color.clone(), osup=sup.clone(),
                 oidx=idx, count=count, scratch=scratch, nbytes=nbytes)

    def compact(**kw):
        a = dict(cgood)
        a.update(kw)
        p = hip.ptr
        return L.mvd_compact_points(p(a["xyz"]), p(a["color"]), p(a["sup"]), p(a["con"]), p(a["fl"]), a["n"], a["ms"], a["mc"], p(a["oxyz"]),
                                    p(a["ocolor"]), p(a["osup"]), p(a["oidx"]), p(a["count"]), p(a["scratch"]), a["nbytes"], hip.stream())

    assert compact() == 0
    for kw in (dict(xyz=None), dict(sup=None), dict(con=None), dict(fl=None), dict(oxyz=None), dict(osup=None), dict(oidx=None),
               dict(count=None), dict(scratch=None), dict(color=None), dict(ocolor=None), dict(n=0), dict(n=1 << 31), dict(ms=-1),
               dict(mc=-1), dict(nbytes=nbytes - 4), dict(nbytes=0)):
        assert compact(**kw) != 0, kw
        assert b"mvd_compact_points" in L.mvd_last_error(), kw
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. host round trip
def _small_vae():
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.load_model import instantiate_from_config
    dd = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2, 4, 4], num_res_blocks=2,
              attn_resolutions=[], dropout=0.0)
    vae = instantiate_from_config(dict(target="external.sd1.ldm.models.autoencoder.AutoencoderKL",
                                       params=dict(embed_dim=4, ddconfig=dd, lossconfig=dict(target="torch.nn.Identity"))))
    syn.fill_module_(vae, "vae.")
    return vae.cuda().eval()


def _cloud_equal(a, b):
    return all((getattr(a, k) is None and getattr(b, k) is None) or torch.equal(getattr(a, k), getattr(b, k))
               for k in ("xyz", "rgb", "support", "scene", "view", "pixel", "index"))


def test_viewfusion_fuse_round_trip():
    """After a 2-step sample on the reduced-width model: ViewFusion.fuse == fuse_views with the decoded image and the model's depth map;
    the (N, V, ...) form == the per-scene calls one after the other."""
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.fusion import fuse_views
    V, S, up = 2, 32, 8
    m = build_model(32)
    inp = syn.make_inputs(V, S, seed=2)
    x = m.ddim.sample(inp["batch_cameras"], inp["input_latents"], inp["input_cameras"], inp["clip_v_embed"], unconditional_scale=2.5,
                      depth=True, verbose=False, x_T=inp["x_T"].cuda(), num_steps=2)
    assert x.shape == (V, 5, S, S)
    assert not hasattr(m, "vae")
    m.vae = _small_vae()                      # (the cached test model is built without one)
    try:
        kw = dict(min_support=0, max_conflicts=255)          # (two steps of an untrained model agree on nothing: keep the foreground)
        pc = m.fuse(x, inp["batch_cameras"], up=up, **kw)
        img = m.decode(x[:, :4])
        assert img.shape == (V, 3, 8 * S, 8 * S)
        want = fuse_views(x, inp["batch_cameras"], rgb=img, up=up, depth_scale=m.view_attn.depth_scale, depth_shift=m.view_attn.depth_shift,
                          **kw)
        assert _cloud_equal(pc, want)
        P = S * up
        assert 0 < len(pc) <= V * P * P
        assert bool(torch.isfinite(pc.xyz).all()) and bool(torch.isfinite(pc.rgb).all())
        i = pc.index.long()
        assert torch.equal((pc.scene * V + pc.view) * P * P + pc.pixel[:, 0] * P + pc.pixel[:, 1], i)
        assert bool((i[1:] > i[:-1]).all()) and int(pc.scene.max()) == 0
        assert torch.equal(pc.rgb, img[pc.view, :, pc.pixel[:, 0], pc.pixel[:, 1]])
        lo = m.fuse(x, inp["batch_cameras"], up=2, **kw)          # the decoded image is area-resized to the coarser grid
        assert 0 < len(lo) <= V * (2 * S) ** 2 and bool(torch.isfinite(lo.rgb).all())
        plain = m.fuse(x, inp["batch_cameras"], up=up, decode=False, **kw)
        assert plain.rgb is None and torch.equal(plain.xyz, pc.xyz)

        # two scenes on rigs of their own
        from gridattn_f64 import make_rig
        cams = [inp["batch_cameras"], make_rig(V, True, seed=3)[0]]
        xs = torch.stack([x, x.flip(0) * 0.9])
        imgs = torch.stack([m.decode(xs[n, :, :4]) for n in range(2)])          # (decoded once: this compares the fusion, not the decoder)
        both = m.fuse(xs, cams, up=2, decode=False, rgb=imgs, **kw)
        one = [m.fuse(xs[n], cams[n], up=2, decode=False, rgb=imgs[n], **kw) for n in range(2)]
        assert len(both) == len(one[0]) + len(one[1]) and len(one[1]) > 0
        for k in ("xyz", "rgb", "support", "view", "pixel"):
            assert torch.equal(getattr(both, k), torch.cat([getattr(c, k) for c in one])), k
        assert torch.equal(both.scene, torch.cat([torch.full_like(one[n].scene, n) for n in range(2)]))
    finally:
        del m.vae
