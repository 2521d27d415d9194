"""The point renderer on the GPU: mvd_render_points (csrc/fusion.hip) through the C ABI against the float64 reference of
tests/render_f64.py, and the host path (fusion.render_points, ViewFusion.render).

Bounds -- none taken from what the kernels give:
  index, hit      EQUAL to float64 on every compared pixel (render_f64.excluded_pixels: pixels where float64 sits within the fp32 oracle's
                  own error of one of the rule's comparisons are left out, at most 1 % of a case's pixels, asserted first)
  depth           max|kernel - f64| <= 4 max|fp32 oracle - f64| + 2^-23 max|f64| on those pixels (two fp32 evaluation orders of the same
                  formulas, plus one rounding of the result)
  on EVERY pixel  depth is, bit for bit, the kernel's own camera z of the point `index` names (each point rendered alone), and rgb is
                  color[index] bit for bit
  ties, determinism, the integer minimum at size: bit equality.

Measured on an MI355X: no index mismatch on 512 / 512 / 3071 / 3072 / 3072 / 4096 / 6144 / 1024 compared pixels (one pixel of 21 504 left
out); depth kernel error / fp32-oracle error = 0.4 - 1.0 (8.3e-8 ... 2.1e-7 against bounds of 8.9e-7 ... 1.1e-6); own-view round trip: every
point on its own pixel, depth error 4.8e-7 (bound 9.6e-7); depth_latent round trip exact (bound 1.2e-7); size: 0 of 131 072 pixels differ.
"""
import ctypes

import pytest
import torch

import fusion_f64 as F
import render_f64 as R
from conftest import build_model

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
BACKGROUND = (0.25, 0.5, 0.75)
EMPTY_DEPTH = -3.0


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


def _buffers(ncam, P, nbytes):
    dev = "cuda"
    return dict(index=torch.full((ncam, P, P), -5, dtype=torch.int32, device=dev), depth=torch.full((ncam, P, P), SENTINEL, device=dev),
                rgb=torch.full((ncam, 3, P, P), SENTINEL, device=dev), scratch=torch.full((max(nbytes // 8, 1),), 0x1234, dtype=torch.int64, device=dev))


def _untouched(out):
    return bool((out["index"] == -5).all()) and bool((out["depth"] == SENTINEL).all()) and bool((out["rgb"] == SENTINEL).all()) and \
        bool((out["scratch"] == 0x1234).all())


def _call(hip, out, xyz, color, start, cams, n, nscene, M, P, r, znear=1e-3, rgb=True, nbytes=None, background=BACKGROUND, index=True,
          depth=True, scratch=True):
    bg = None if background is None else (ctypes.c_float * 3)(*background)
    p = hip.ptr
    nbytes = out["scratch"].numel() * 8 if nbytes is None else nbytes
    return hip.lib().mvd_render_points(p(xyz), p(color), p(start), p(cams), n, nscene, M, P, r, znear, EMPTY_DEPTH, bg,
                                       p(out["index"]) if index else None, p(out["depth"]) if depth else None,
                                       p(out["rgb"]) if rgb else None, p(out["scratch"]) if scratch else None, nbytes, hip.stream())


def _render(hip, case, color=True, P=None, r=None, start=None, nscene=None, M=None, cams=None):
    """One mvd_render_points call; every output buffer is pre-filled, the rgb buffer is passed even without colour."""
    P, r = case.P if P is None else P, case.r if r is None else r
    nscene, M = case.nscene if nscene is None else nscene, case.M if M is None else M
    nbytes = int(hip.lib().mvd_render_points_scratch(nscene * M, P))
    assert nbytes == nscene * M * P * P * 8
    out = _buffers(nscene * M, P, nbytes)
    xyz = case.xyz.contiguous().cuda()
    col = case.color.contiguous().cuda() if color else None
    start = (case.scene_start() if start is None else start).cuda()
    cams = (case.packed() if cams is None else cams).cuda()
    hip.check(_call(hip, out, xyz, col, start, cams, case.n, nscene, M, P, r, znear=case.znear))
    torch.cuda.synchronize()
    return out


def _own_depths(hip, case):
    """(n, M): the kernel's camera z of every (point, camera of its scene) pair that draws at all -- every point rendered ALONE, as a
    scene of its own with its scene's cameras, into one pixel under the largest footprint (camera z does not depend on P)."""
    n, M = case.n, case.M
    cams = case.packed().reshape(case.nscene, M, -1)[case.scene].reshape(n * M, -1)
    out = _render(hip, case, color=False, P=1, r=hip.SPLAT_MAX_RADIUS, start=torch.arange(n + 1, dtype=torch.int32), nscene=n, M=M, cams=cams)
    assert bool(((out["index"].reshape(n, M) == torch.arange(n, device="cuda")[:, None]) | (out["index"].reshape(n, M) == -1)).all())
    return out["depth"].reshape(n, M)


def _check_every_pixel(hip, case, got):
    """depth is the kernel's own zc of `index`, rgb is color[index] or the background -- on every pixel, compared with float64 or not."""
    M, P = case.M, case.P
    idx = got["index"].long()
    hit = idx >= 0
    own = _own_depths(hip, case)
    cam = torch.arange(case.nscene * M, device="cuda")[:, None, None].expand_as(idx)
    scene = case.scene.cuda()[idx.clamp(min=0)]
    assert bool((scene == cam // M)[hit].all())                                     # a camera shows only its own scene's points
    want = own[idx.clamp(min=0), cam % M]
    assert torch.equal(got["depth"][hit].view(torch.int32), want[hit].view(torch.int32))
    assert bool((got["depth"][~hit] == EMPTY_DEPTH).all())
    rgb = case.color.cuda()[idx.clamp(min=0)].permute(0, 3, 1, 2)
    bg = torch.tensor(BACKGROUND, device="cuda").reshape(1, 3, 1, 1).expand_as(rgb)
    assert torch.equal(got["rgb"], torch.where(hit[:, None], rgb, bg))
    assert bool((got["scratch"] != 0x1234).all())


# ------------------------------------------------------------------------------------------------ 1. parity against float64
@pytest.mark.parametrize("name", list(R.CASES))
def test_render_points_vs_float64(hip, name):
    case, image, ref, bad, m = R.refs(name)          # asserts the cap
    keep = ~bad
    got = _render(hip, case)
    idx, depth = got["index"].cpu().long(), got["depth"].cpu()
    wrong = int((idx != image.index)[keep].sum())
    both = keep & image.hit & (idx >= 0)
    err = float((depth.double() - image.depth)[both].abs().max()) if bool(both.any()) else 0.0
    bound = R.depth_bound(m)
    print(f"RATIO render {name} | compared pixels {int(keep.sum())}/{keep.numel()} index mismatches {wrong} | depth kernel {err:.2e} oracle "
          f"{m.oracle_z:.2e} bound {bound:.2e} | hit {float(image.hit.float().mean()):.3f}")
    assert wrong == 0
    assert torch.equal((idx >= 0)[keep], image.hit[keep])
    assert err <= bound, (err, bound)
    assert int(idx.min()) >= -1 and int(idx.max()) < case.n
    _check_every_pixel(hip, case, got)
    start = case.scene_start().tolist()
    for s in range(case.nscene):          # no pixel of a scene's cameras holds another scene's index
        mine = idx[s * case.M:(s + 1) * case.M]
        assert bool(((mine == -1) | ((mine >= start[s]) & (mine < start[s + 1]))).all()), s
    if name.startswith("empty_first"):
        assert bool((idx[:case.M] == -1).all()) and bool((idx[case.M:] >= 0).any())


# ------------------------------------------------------------------------------------------------ 2. tie rule and determinism
def test_ties_go_to_the_first_point_and_runs_are_identical(hip):
    case = R.make_case("main_r1")
    dup = R.duplicated(case)
    one, two = _render(hip, case), _render(hip, dup)
    assert int(two["index"].max()) < case.n and int(two["index"].max()) >= 0
    for k in ("index", "depth", "rgb"):
        assert torch.equal(one[k], two[k]), k
    _check_every_pixel(hip, dup, two)
    again = _render(hip, dup)
    for k in ("index", "depth", "rgb", "scratch"):
        assert torch.equal(two[k], again[k]), k


# ------------------------------------------------------------------------------------------------ 3. own-view round trip
def test_a_view_rendered_into_its_own_camera_lands_on_its_own_pixels(hip):
    """Fuse the sphere, take every view's points alone (a scene each, one camera: the view's own) and render at P = S, r = 0: each point
    lands on its own pixel, and the depth there is the latent's metric depth."""
    fcase = F.sphere_case()
    V, S = fcase.V, fcase.S
    n = fcase.npts
    ref, o32 = F.reference(fcase), F.reference(fcase, torch.float32)
    xyz = torch.full((n, 3), SENTINEL, device="cuda")
    sup, con, fl = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(3))
    lat, cams, lin = fcase.lat.cuda(), fcase.packed().cuda(), F.ndc_lin(S).cuda()
    hip.check(hip.lib().mvd_fuse_points(hip.ptr(lat), None, hip.ptr(cams), hip.ptr(lin), hip.ptr(xyz), None, hip.ptr(sup), hip.ptr(con),
                                        hip.ptr(fl), 1, V, S, 1, fcase.depth_scale, fcase.depth_shift, fcase.lo, fcase.hi, fcase.tau, 0,
                                        hip.stream()))
    case = R.Case(xyz=xyz.cpu(), color=None, scene=torch.arange(V).repeat_interleave(S * S), cams=fcase.cams, nscene=V, M=1, P=S, r=0)
    got = _render(hip, case, color=False)
    assert torch.equal(got["index"].cpu().long().reshape(-1), torch.arange(n))
    z = F.metric_depth(fcase, torch.float64)
    bound = F.MARGIN * float((o32.xyz.double() - ref.xyz).abs().max()) + 2.0 ** -23 * float(ref.xyz.abs().max())
    err = float((got["depth"].cpu().double() - z).abs().max())
    print(f"round trip: depth kernel {err:.2e} bound {bound:.2e}")
    assert err <= bound, (err, bound)


# ------------------------------------------------------------------------------------------------ 4. color = NULL
def test_without_colour_the_rgb_buffer_is_not_touched(hip):
    case = R.make_case("main_r1")
    plain, full = _render(hip, case, color=False), _render(hip, case)
    assert bool((plain["rgb"] == SENTINEL).all()) and not bool((full["rgb"] == SENTINEL).any())
    assert torch.equal(plain["index"], full["index"]) and torch.equal(plain["depth"], full["depth"])


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_bad_arguments_return_an_error_and_write_nothing(hip):
    L = hip.lib()
    case = R.make_case("sub_wavefront_r0")
    P, M, n = case.P, case.M, case.n
    nbytes = int(L.mvd_render_points_scratch(M, P))
    assert int(L.mvd_render_points_scratch(0, P)) == 0 and int(L.mvd_render_points_scratch(M, 0)) == 0
    xyz, col, start, cams = case.xyz.cuda(), case.color.cuda(), case.scene_start().cuda(), case.packed().cuda()
    out = _buffers(M, P, nbytes)
    good = dict(xyz=xyz, color=col, start=start, cams=cams, n=n, nscene=1, M=M, P=P, r=1)
    bad = [dict(r=hip.SPLAT_MAX_RADIUS + 1), dict(r=-1), dict(P=0), dict(P=-2), dict(xyz=None), dict(nbytes=nbytes - 8), dict(nbytes=0),
           dict(start=None), dict(cams=None), dict(index=False), dict(depth=False), dict(scratch=False), dict(rgb=False),
           dict(background=None), dict(znear=-0.5), dict(znear=float("nan")), dict(nscene=0), dict(M=0), dict(n=1 << 31),
           dict(nscene=4096, M=16),                      # 65536 cameras
           dict(P=1 << 15, nbytes=1 << 62)]              # 2 x 2^30 pixels
    for kw in bad:
        a = dict(good)
        a.update(kw)
        assert _call(hip, out, **a) != 0, kw
        assert b"mvd_render_points" in L.mvd_last_error(), kw
    torch.cuda.synchronize()
    assert _untouched(out)
    assert _call(hip, out, xyz=None, color=None, start=torch.zeros(2, dtype=torch.int32, device="cuda"), cams=cams, n=0, nscene=1, M=M, P=P,
                 r=1, rgb=False, background=None) == 0          # no points, no colour: every pixel empty
    assert _call(hip, _buffers(M, P, nbytes), **good) == 0
    torch.cuda.synchronize()
    assert bool((out["index"] == -1).all()) and bool((out["depth"] == EMPTY_DEPTH).all()) and bool((out["rgb"] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 6. host path
def test_render_points_host_path(hip):
    from gridattn_f64 import make_rig
    from mvdfusion_amd import fusion
    fcase = F.make_case("two_scenes_v3_s8")
    N, V, S, up, P = fcase.nscene, fcase.V, fcase.S, 2, 24
    lat = fcase.lat.reshape(N, V, 5, S, S).cuda()
    rigs = [F.get_camera_slice(fcase.cams, list(range(s * V, (s + 1) * V))) for s in range(N)]
    img = torch.rand(N, V, 3, S * up, S * up, generator=torch.Generator().manual_seed(3)).cuda()
    cloud = fusion.fuse_views(lat, rigs, rgb=img, up=up, min_support=0, max_conflicts=255)
    assert 0 < len(cloud) and int(cloud.scene.max()) == 1
    targets = [make_rig(2, True, seed=40 + s)[0] for s in range(N)]          # two novel cameras per scene
    rv = fusion.render_points(cloud, targets, size=P, radius=1, background=BACKGROUND, empty_depth=EMPTY_DEPTH)
    case = R.Case(xyz=cloud.xyz.cpu(), color=cloud.rgb.cpu(), scene=cloud.scene.cpu(), cams=R.cat_cameras(targets), nscene=N, M=2, P=P, r=1)
    got = _render(hip, case)
    assert rv.rgb.shape == (N, 2, 3, P, P) and rv.depth.shape == rv.index.shape == rv.hit.shape == (N, 2, P, P)
    assert torch.equal(rv.index.reshape(-1, P, P), got["index"]) and torch.equal(rv.depth.reshape(-1, P, P), got["depth"])
    assert torch.equal(rv.rgb.reshape(-1, 3, P, P), got["rgb"]) and torch.equal(rv.hit, rv.index >= 0)
    assert bool(rv.hit.any()) and bool((~rv.hit).any())
    # one scene with its bare camera set: no leading dimension, the same pixels
    first = fusion.PointCloud(**{k: getattr(cloud, k)[cloud.scene == 0] if getattr(cloud, k) is not None else None
                                 for k in ("xyz", "rgb", "support", "scene", "view", "pixel", "index")})
    one = fusion.render_points(first, targets[0], size=P, radius=1, background=BACKGROUND, empty_depth=EMPTY_DEPTH)
    assert one.depth.shape == (2, P, P) and torch.equal(one.depth, rv.depth[0]) and torch.equal(one.rgb, rv.rgb[0])
    assert torch.equal(one.index, rv.index[0])
    bare = fusion.render_points(first.xyz, targets[0], size=P, radius=1, empty_depth=EMPTY_DEPTH)
    assert bare.rgb is None and torch.equal(bare.index, one.index)
    # depth_latent: +1 on empty pixels, and in [-1, 1]
    dl = rv.depth_latent()
    assert bool((dl[~rv.hit] == 1.0).all()) and float(dl.min()) >= -1.0 and float(dl.max()) <= 1.0


def test_depth_latent_inverts_the_fuse_map():
    """z = clamp((lat + 1) / 2, 0, 1) * scale + shift (fuse_views), then depth_latent: back at lat to within the fp32 rounding of the two
    affine maps -- MARGIN x the error of the same two expressions evaluated in fp32 on the CPU against float64, plus one rounding."""
    from mvdfusion_amd import fusion
    scale, shift = fusion.DEPTH_SCALE, fusion.DEPTH_SHIFT
    lat = torch.linspace(-1.0, 1.0, 4097, dtype=torch.float32)
    there = lambda t: torch.clip((t + 1.0) / 2.0, 0.0, 1.0) * scale + shift
    back = lambda z: torch.clamp(2.0 * (z - shift) / scale - 1.0, -1.0, 1.0)
    oracle = float((back(there(lat)).double() - back(there(lat.double()))).abs().max())
    bound = R.MARGIN * oracle + 2.0 ** -23
    z = there(lat.cuda())
    index = torch.zeros(lat.shape, dtype=torch.int32, device="cuda")
    rv = fusion.RenderedViews(rgb=None, depth=z, index=index, hit=index >= 0)
    err = float((rv.depth_latent().cpu().double() - lat.double()).abs().max())
    print(f"depth_latent: error {err:.2e} oracle {oracle:.2e} bound {bound:.2e}")
    assert err <= bound, (err, bound)


def test_viewfusion_render_binds_the_models_depth_map():
    from gridattn_f64 import make_rig
    from mvdfusion_amd import fusion
    m = build_model(32)
    case = R.make_case("sub_wavefront_r2")
    cams = make_rig(case.M, True, 0)[0]
    cloud = case.xyz.cuda()
    keep = m.view_attn.depth_scale, m.view_attn.depth_shift
    try:
        m.view_attn.depth_scale, m.view_attn.depth_shift = 3.0, 0.25          # (not the interface defaults: the binding must show)
        rv = m.render(cloud, cams, size=16, radius=2)
        want = fusion.render_points(cloud, cams, size=16, radius=2)
        assert torch.equal(rv.index, want.index) and torch.equal(rv.depth, want.depth) and bool(rv.hit.any())
        assert torch.equal(rv.depth_latent(), want.depth_latent(depth_scale=3.0, depth_shift=0.25))
        assert not torch.equal(rv.depth_latent(), want.depth_latent())
        assert torch.equal(rv.depth_latent(fusion.DEPTH_SCALE, fusion.DEPTH_SHIFT), want.depth_latent())
    finally:
        m.view_attn.depth_scale, m.view_attn.depth_shift = keep


# ------------------------------------------------------------------------------------------------ 7. size
def test_the_largest_size_against_integer_minima_in_torch(hip):
    """131 072 points into P = 256, M = 2, r = 1 against render_f64.torch_rule on the GPU: both are the minimum of the same 64-bit
    integers, so index is equal bit for bit and nothing is excluded."""
    n, P, M, r = 131072, 256, 2, 1
    g = torch.Generator().manual_seed(77)
    from gridattn_f64 import make_rig
    case = R.Case(xyz=(torch.rand(n, 3, generator=g) - 0.5) * R.CUBE, color=torch.rand(n, 3, generator=g), scene=torch.zeros(n, dtype=torch.long),
                  cams=make_rig(M, True, 5)[0], nscene=1, M=M, P=P, r=r)
    got = _render(hip, case)
    want = R.torch_rule(case.xyz.cuda(), [0, n], case.cams.to("cuda"), M, P, r, case.znear)
    idx = got["index"].long()
    print(f"size: {int((idx != want).sum())} of {idx.numel()} pixels differ, hit {float((idx >= 0).float().mean()):.3f}")
    assert torch.equal(idx, want)
    hit = idx >= 0
    assert torch.equal(got["rgb"].permute(0, 2, 3, 1)[hit], case.color.cuda()[idx[hit]]) and bool(hit.any())
