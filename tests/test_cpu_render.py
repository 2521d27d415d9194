"""The point renderer without a GPU: the float64 reference of tests/render_f64.py against hand-computed answers, the exclusion cap of
every parity case of tests/test_gpu_render.py, and the host side of fusion.render_points (argument validation before the library is
touched; the depth-latent map)."""
import os
import re

import pytest
import torch

import gridattn_f64 as G
import render_f64 as R
from mvdfusion_amd import fusion, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = (0.25, -0.25, 0.0)          # u = 0.125, cx = 3.0; w = -0.125, cy = 4.0; zc = 2 in R.unit_camera() at P = 8


@pytest.mark.parametrize("name", list(R.CASES))
def test_parity_cases_respect_the_exclusion_cap(name):
    """... and are worth running: pixels are hit (and at r = 0 some are left empty), and the fp32 oracle agrees with float64 on every compared pixel (so the
    index CAN be asserted equal)."""
    case, image, ref, bad, m = R.refs(name)          # asserts the cap
    o32, _ = R.render(case, torch.float32)
    keep = ~bad
    print(f"{name}: excluded {float(bad.float().mean()):.3%} of {bad.numel()} pixels, m_p {m.m_p:.1e}, m_z {m.m_z:.1e}, hit "
          f"{float(image.hit.float().mean()):.3f}, depth bound {R.depth_bound(m):.1e}")
    assert float(bad.float().mean()) <= R.MAX_EXCLUDED
    assert torch.equal(o32.index[keep], image.index[keep]) and torch.equal(o32.hit[keep], image.hit[keep])
    both = keep & image.hit
    assert float((o32.depth.double() - image.depth)[both].abs().max()) <= R.depth_bound(m)
    assert bool(image.hit.any()) and (case.r > 0 or bool((~image.hit).any()))
    start = case.scene_start().tolist()
    for s in range(case.nscene):          # a camera shows only its own scene's points
        idx = image.index[s * case.M:(s + 1) * case.M]
        assert bool(((idx == -1) | ((idx >= start[s]) & (idx < start[s + 1]))).all())
    if name.startswith("empty_first"):
        assert not bool(image.hit[:case.M].any()) and bool(image.hit[case.M:].any())


def _image(points, **kw):
    case = R.unit_case(points, **kw)
    return case, R.render(case)[0]


def test_known_answers_of_the_reference():
    case, im = _image([A])
    proj = R.project(case)
    assert (float(proj.cx), float(proj.cy), float(proj.zc)) == (3.0, 4.0, 2.0)
    assert torch.nonzero(im.hit[0]).tolist() == [[4, 3]] and int(im.index[0, 4, 3]) == 0 and float(im.depth[0, 4, 3]) == 2.0
    assert int((im.index == -1).sum()) == 63 and bool(torch.isinf(im.depth[~im.hit]).all())
    # r = 1: exactly the 3 x 3 block around that pixel
    _, im = _image([A], r=1)
    want = torch.zeros(8, 8, dtype=torch.bool)
    want[3:6, 2:5] = True
    assert torch.equal(im.hit[0], want) and bool((im.index[0][want] == 0).all()) and bool((im.depth[0][want] == 2.0).all())
    # a second point behind it on the same ray (camera centre (0, 0, -2): X = C + t (A - C)) loses, in either order
    behind = (0.375, -0.375, 1.0)
    for pts, winner in (([A, behind], 0), ([behind, A], 1)):
        case, im = _image(pts)
        assert (float(R.project(case).cx[1 - winner]), float(R.project(case).cy[1 - winner])) == (3.0, 4.0)
        assert torch.nonzero(im.hit[0]).tolist() == [[4, 3]] and int(im.index[0, 4, 3]) == winner and float(im.depth[0, 4, 3]) == 2.0
    # a duplicate with a higher index loses
    _, im = _image([A, A, A], r=1)
    assert bool((im.index[0][want] == 0).all()) and int(im.hit.sum()) == 9
    # zc <= znear draws nothing: zc = 0.5 with znear = 0.5, and a point behind the camera
    _, im = _image([(0.0, 0.0, -1.5), (0.0, 0.0, -3.0)], znear=0.5)
    assert not bool(im.hit.any())
    _, im = _image([(0.0, 0.0, -1.5)], znear=0.25)
    assert int(im.hit.sum()) == 1
    # a centre one pixel outside the image (cx = -1: u = 1.125, x = 2.25): a one-pixel-wide strip at r = 1, nothing at r = 0
    case, im = _image([(2.25, -0.25, 0.0)], r=1)
    assert (float(R.project(case).cx), float(R.project(case).cy)) == (-1.0, 4.0)
    strip = torch.zeros(8, 8, dtype=torch.bool)
    strip[3:6, 0] = True
    assert torch.equal(im.hit[0], strip)
    assert not bool(_image([(2.25, -0.25, 0.0)], r=0)[1].hit.any())
    # colours follow the index; empty pixels take the background
    case, im = _image([A, behind], r=1)
    rgb = R.colours(case, im, (1.0, 0.5, 0.25))
    assert torch.equal(rgb[0, :, 4, 3], case.color[0]) and rgb[0, :, 0, 0].tolist() == [1.0, 0.5, 0.25]


def test_render_points_validates_its_arguments(monkeypatch):
    calls = []

    def run(xyz, color, scene_start, cams, N, M, P, radius, znear, empty_depth, background):
        calls.append(dict(xyz=xyz, color=color, scene_start=scene_start, cams=cams, N=N, M=M, P=P, radius=radius, znear=znear,
                          empty_depth=empty_depth, background=background))
        return (None if color is None else torch.zeros(N * M, 3, P, P), torch.full((N * M, P, P), empty_depth),
                torch.full((N * M, P, P), -1, dtype=torch.int32))

    monkeypatch.setattr(fusion, "_render", run)
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("the library was touched"))
    M, n = 3, 10
    cams = G.make_rig(M, True)[0]
    xyz = torch.rand(n, 3)
    scene = torch.tensor([0] * 4 + [1] * 6)
    cloud = fusion.PointCloud(xyz=xyz, rgb=torch.rand(n, 3), support=torch.ones(n, dtype=torch.uint8), scene=scene,
                              view=torch.zeros(n, dtype=torch.long), pixel=torch.zeros(n, 2, dtype=torch.long),
                              index=torch.arange(n, dtype=torch.int32))
    two = [cams, G.make_rig(M, True, seed=1)[0]]
    bad = [
        dict(radius=-1), dict(radius=hip.SPLAT_MAX_RADIUS + 1), dict(radius=1.5), dict(size=0), dict(size=-4), dict(size=2.5),
        dict(cameras=[cams]), dict(cameras=cams),                                  # one camera set, listed or bare, for a cloud of two scenes
        dict(cameras=[cams, G.make_rig(M + 1, True)[0]]), dict(cameras=[]),      # unequal M; no set
        dict(cloud=xyz, cameras=two),                                              # an (n, 3) tensor is one scene
        dict(cloud=xyz[:, :2]), dict(cloud=xyz.reshape(-1)), dict(cloud=xyz[None]), dict(cloud="cloud"),
        dict(size=2 ** 15),                                                        # 2 x 3 x 2^30 pixels
        dict(znear=-1.0), dict(znear=float("nan")), dict(background=(1.0, 1.0)),
    ]
    for kw in bad:
        args = dict(cloud=cloud, cameras=two)
        args.update(kw)
        with pytest.raises(ValueError):
            fusion.render_points(**args)
    assert not calls                                   # nothing reached the library
    assert fusion.render_points(cloud, two + [cams], size=8).depth.shape == (3, M, 8, 8)          # more sets than scenes: cloud.scene < N holds
    out = fusion.render_points(cloud, two)             # the defaults, as documented
    c = calls[-1]
    assert (c["N"], c["M"], c["P"], c["radius"]) == (2, M, 256, 1) and c["cams"].shape == (2 * M, hip.CAM_RECORD)
    assert c["background"] == (1.0, 1.0, 1.0) and c["znear"] == 1e-3 and c["empty_depth"] == float("inf")
    assert c["scene_start"].tolist() == [0, 4, 10] and c["scene_start"].dtype == torch.int32
    assert out.rgb.shape == (2, M, 3, 256, 256) and out.depth.shape == out.index.shape == out.hit.shape == (2, M, 256, 256)
    assert out.hit.dtype == torch.bool and not bool(out.hit.any())
    one = fusion.render_points(xyz, cams, size=16, radius=0)          # an (n, 3) tensor: one scene, no colour, no leading dimension
    assert one.rgb is None and one.depth.shape == (M, 16, 16) and calls[-1]["scene_start"].tolist() == [0, n] and calls[-1]["color"] is None


def test_depth_latent_is_the_inverse_of_the_fuse_map():
    depth = torch.tensor([[0.5, 1.5, 2.5, 3.0, 0.25, float("inf")]])
    index = torch.tensor([[0, 1, 2, 3, 4, -1]], dtype=torch.int32)
    rv = fusion.RenderedViews(rgb=None, depth=depth, index=index, hit=index >= 0)
    assert rv.depth_latent().tolist() == [[-1.0, 0.0, 1.0, 1.0, -1.0, 1.0]]          # scale 2, shift 0.5; clamped; empty = +1
    assert rv.depth_latent(depth_scale=4.0, depth_shift=0.5).tolist() == [[-1.0, -0.5, 0.0, 0.25, -1.0, 1.0]]
    assert [f.name for f in __import__("dataclasses").fields(rv)] == ["rgb", "depth", "index", "hit"]


def test_splat_max_radius_mirrors_the_header():
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    assert int(re.search(r"#define\s+MVD_SPLAT_MAX_RADIUS\s+(\d+)", hdr).group(1)) == hip.SPLAT_MAX_RADIUS == 4
    stages = {k: int(v) for k, v in re.findall(r"#define\s+MVD_RENDER_(\w+)\s+(\d+)", hdr)}
    assert stages == dict(FILL=hip.RENDER_FILL, SPLAT=hip.RENDER_SPLAT, RESOLVE=hip.RENDER_RESOLVE, ALL=hip.RENDER_ALL)
