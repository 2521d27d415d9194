"""The mesh rasteriser without a GPU: the float64 reference of tests/raster_f64.py held to known answers, the exclusion cap of every parity
case of tests/test_gpu_raster.py, and the host side of fusion.render_mesh (argument validation before the library is touched)."""
import dataclasses
import math
import os
import re

import pytest
import torch

import gridattn_f64 as G
import raster_f64 as R
from mvdfusion_amd import fusion, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(R.CASES))
def test_parity_cases_respect_the_exclusion_cap(name):
    """... and are worth running: the fp32 oracle agrees with float64 on every compared pixel (so `face` CAN be asserted equal), and each
    case reaches what it is there for."""
    ref = R.refs(name)          # asserts the cap
    case, im, o32, keep = ref.case, ref.image, ref.o32, ~ref.bad
    print(f"{name}: {case.nface} faces, excluded {float(ref.bad.float().mean()):.3%} of {ref.bad.numel()} pixels, m_z {ref.m_z:.1e}, hit "
          f"{float(im.hit.float().mean()):.3f}, bounds " + ", ".join(f"{k} {b:.1e} (oracle {e:.1e})" for k, (e, b) in ref.bounds.items()))
    assert float(ref.bad.float().mean()) <= R.MAX_EXCLUDED
    assert torch.equal(o32.face[keep], im.face[keep]) and torch.equal(o32.hit[keep], im.hit[keep])
    assert bool(im.hit.any()) and bool((~im.hit).any()) != (name == "big_and_small")          # (its big triangle covers the image)
    assert set(ref.bounds) == ({"depth", "bary", "normal", "rgb"} if case.colors is not None else {"depth", "bary", "normal"})
    scene = R.face_scene(case)
    cam_scene = torch.arange(case.nscene * case.M)[:, None, None].expand_as(im.face) // case.M
    assert bool((scene[im.face.clamp(min=0)] == cam_scene)[im.hit].all())          # a camera shows only its own scene's faces
    s = R.setup(case)
    drawn = R.draws(case, s, torch.float64)
    box = lambda c: (c.amax(-1).floor().clamp(max=case.P - 1) - c.amin(-1).ceil().clamp(min=0) + 1).clamp(min=0)
    pixels = box(s.px) * box(s.py)
    if name == "icosahedron":
        assert case.nface == 20 < 64
    if name == "big_and_small":
        assert bool((s.px[0, 0].abs() > case.P).any()) and int(pixels[0, 0]) == case.P ** 2          # all outside, the box is the image
        assert int((pixels[1:, 0] > 64).sum()) >= 3 and int(((pixels[1:, 0] <= 64) & (pixels[1:, 0] > 0)).sum()) >= 50
        won = im.face[im.hit]
        assert bool((won == 0).any()) and bool((won > 0).any())
        assert float((im.face == 0).float().mean()) > 0.3          # the big triangle is what most pixels show
    if name.startswith("sphere"):
        other = R.refs("sphere_cull1" if name == "sphere_cull0" else "sphere_cull0")
        both = keep & ~other.bad
        assert torch.equal(im.face[both], other.image.face[both])          # closed, wound outward, seen from outside
        assert bool((~s.front & drawn).any()) == (not case.cull)          # cull 0 draws the back faces, behind the front ones
    if name == "two_scenes_empty_first":
        assert not bool(im.hit[:case.M].any()) and bool(im.hit[case.M:].any())
    if name == "drop_rules":
        znear = float(R._znear(case, torch.float64))
        ok = s.ids_ok[:, None] & R.finite(s)
        straddle = ok & (s.zc > znear).any(-1) & (s.zc <= znear).any(-1)
        assert bool(straddle.any()) and bool((ok & (s.zc <= znear).all(-1)).any())
        appended = (~s.ids_ok) | (s.area2 == 0).all(1) | ~R.finite(s).all(1)
        assert int(appended.sum()) == 13 and not bool(drawn[appended].any())
        assert not bool(appended[im.face[im.hit]].any())
        assert bool((~s.front)[im.face[im.hit], 0].any())          # the back of the sphere shows through the hole


# ------------------------------------------------------------------------------------------------ known answers
def test_a_fronto_parallel_square_has_constant_depth_and_the_analytic_coverage():
    """x, y in [-1, 1] at world z = 0 in the unit camera at P = 8: px, py in [1.5, 5.5], camera z = 2.  4 x 4 pixel centres are inside; the
    centres (2, 2) ... (5, 5) lie exactly on the diagonal both triangles share: both cover them at the same depth, the lower id wins."""
    v = [(1, 1, 0), (-1, 1, 0), (-1, -1, 0), (1, -1, 0)]          # px = 1.5, 5.5, 5.5, 1.5; py = 1.5, 1.5, 5.5, 5.5
    for faces in ([(0, 1, 2), (0, 2, 3)], [(0, 2, 3), (0, 1, 2)], [(0, 2, 1), (0, 2, 3)]):
        case = R.unit_case(v, faces)
        s = R.setup(case)
        assert s.px[0, 0].tolist() == [1.5, 5.5, 5.5] or s.px[0, 0].tolist() == [1.5, 5.5, 1.5]
        im = R.render(case)
        want = torch.zeros(8, 8, dtype=torch.bool)
        want[2:6, 2:6] = True
        assert torch.equal(im.hit[0], want) and int(im.hit.sum()) == 16
        assert float((im.depth[0][want] - 2.0).abs().max()) <= 2 * 2.0 * 2.0 ** -52
        assert im.face[0][[2, 3, 4, 5], [2, 3, 4, 5]].tolist() == [0, 0, 0, 0]          # the diagonal: covered by both, shown once
        assert bool((im.face[0][want] == 1).any())
        assert float((im.bary[0].sum(0)[want] - 1.0).abs().max()) <= 1e-15 and float(im.bary.min()) >= 0.0
        assert torch.allclose(im.normal[0][:, want], torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64)[:, None].expand(3, 16))
        o32 = R.render(case, torch.float32)
        assert torch.equal(o32.face, im.face) and float((o32.depth[0][want] - 2.0).abs().max()) <= 2 * 2.0 * 2.0 ** -23
    # culling: (0, 1, 2) is wound clockwise on the screen seen from the camera at z = -2 ... decided geometrically
    front = R.setup(R.unit_case(v, [(0, 1, 2), (0, 2, 1)])).front[:, 0].tolist()
    assert sorted(front) == [False, True]
    one = R.render(R.unit_case(v, [(0, 1, 2), (0, 2, 1)], cull=1))
    assert int(one.hit.sum()) == 10 and set(one.face[one.hit].tolist()) == {front.index(True)}          # half the square with its diagonal
    # znear: nothing at or behind it; a face with one vertex behind is dropped whole
    assert not bool(R.render(R.unit_case(v, [(0, 1, 2)], znear=2.0)).hit.any())
    assert bool(R.render(R.unit_case(v, [(0, 1, 2)], znear=1.99)).hit.any())
    tilted = [(1, 1, 0), (-1, 1, 0), (-1, -1, -1.5)]
    assert bool(R.render(R.unit_case(tilted, [(0, 1, 2)], znear=0.4)).hit.any())
    assert not bool(R.render(R.unit_case(tilted, [(0, 1, 2)], znear=0.5)).hit.any())
    # zero-area, NaN and out-of-range faces draw nothing and poison nothing
    junk = R.unit_case(v + [(float("nan"), 0, 0)], [(0, 0, 1), (0, 1, 4), (0, 1, 5), (-1, 1, 2), (0, 1, 2), (0, 2, 3)])
    im = R.render(junk)
    assert int(im.hit.sum()) == 16 and set(im.face[im.hit].tolist()) == {4, 5} and bool(torch.isfinite(im.depth[im.hit]).all())


def test_interpolation_is_perspective_correct():
    """Vertex colours that are an affine function of world position: at every hit pixel rgb equals that function at the point
    unprojected from (x, y, depth).  True of perspective-correct interpolation; screen-space-linear weights miss it by orders more."""
    cams = G.make_rig(1, True, 7)[0]
    v = torch.tensor([(-0.5, -0.5, -0.3), (0.5, -0.5, 0.3), (0.5, 0.5, 0.3), (-0.5, 0.5, -0.3)], dtype=torch.float64)
    v = v.float().double()                                          # (the values the case holds)
    A = torch.tensor([[0.3, -0.2, 0.5], [0.1, 0.4, -0.3], [-0.2, 0.25, 0.15]], dtype=torch.float64)
    b0 = torch.tensor([0.5, 0.4, 0.6], dtype=torch.float64)
    case = R.unit_case(v, [(0, 1, 2), (0, 2, 3)], colors=v @ A.T + b0, P=24, cams=cams)
    im = R.render(case)
    assert int(im.hit.sum()) > 60
    y, x = torch.nonzero(im.hit[0], as_tuple=True)
    X = R.unproject(cams, 0, x.double(), y.double(), im.depth[0][im.hit[0]], case.P)
    got = im.rgb[0][:, im.hit[0]].T
    assert float((got - (X @ A.T + b0)).abs().max()) <= 1e-12
    # the same pixels with screen-space-linear weights e_i / area2
    s = R.setup(case)
    c = R.candidates(case, s, R.draws(case, s, torch.float64))
    ev = R.evaluate(case, s, c, torch.float64)
    lin = ev.e / s.area2[c.face, c.col].abs()[:, None]
    col = case.colors[case.faces[c.face]]
    flat = (lin[:, :, None] * col).sum(1)
    drawn = R._drawn(case, s, c, ev, torch.float64)
    Xc = R.unproject(cams, 0, c.x.double(), c.y.double(), ev.z, case.P)
    assert float((flat - (Xc @ A.T + b0)).abs()[drawn].max()) > 1e-3


def test_the_sphere_mesh_renders_as_a_sphere():
    """tsdf_f64.march of the exact SDF at G = 24: depth against the ray-sphere intersection within one lattice edge (h = 1.5 / 24); cull on
    and off show the same faces (closed, wound outward, seen from outside); the normals are within the faceting angle -- the longest lattice
    edge, sqrt(3) h, seen from the centre: sqrt(3) h / r -- of the radial direction."""
    Gv, P, M = 24, 48, 2
    v, f = R.sphere_mesh(Gv)
    cams = G.make_rig(M, True, 4)[0]
    h = 1.5 / Gv
    images = {}
    for cull in (0, 1):
        images[cull] = R.render(R._one_scene(v, f, None, cams, M=M, P=P, cull=cull))
    im = images[1]
    assert torch.equal(images[0].face, im.face) and torch.equal(images[0].depth, im.depth)
    assert 0.15 < float(im.hit.float().mean()) < 0.9
    worst_d, worst_a = 0.0, 0.0
    for j in range(M):
        y, x = torch.nonzero(im.hit[j], as_tuple=True)
        p1 = R.unproject(cams, j, x.double(), y.double(), torch.ones(x.numel(), dtype=torch.float64), P)
        p2 = R.unproject(cams, j, x.double(), y.double(), 2.0 * torch.ones(x.numel(), dtype=torch.float64), P)
        d = p2 - p1                                              # X(z) = p1 + (z - 1) d
        a, b, c = (d * d).sum(-1), 2.0 * (p1 * d).sum(-1), (p1 * p1).sum(-1) - R.SPHERE_R ** 2
        disc = b * b - 4 * a * c
        on = disc > 0                                            # the ray meets the sphere itself (the mesh's silhouette pixels may not)
        assert float(on.float().mean()) > 0.9
        z = 1.0 + (-b - disc.clamp(min=0).sqrt()) / (2 * a)
        worst_d = max(worst_d, float((im.depth[j][im.hit[j]] - z)[on].abs().max()))
        X = R.unproject(cams, j, x.double(), y.double(), im.depth[j][im.hit[j]], P)
        radial = (X / X.norm(dim=1, keepdim=True)) @ cams.R[j].double()
        n = im.normal[j][:, im.hit[j]].T
        assert float((n.norm(dim=1) - 1).abs().max()) <= 1e-12 and float(n[:, 2].max()) <= 0.0
        worst_a = max(worst_a, float(torch.acos((n * radial).sum(1).abs().clamp(max=1.0)).max()))
    print(f"sphere G = {Gv}: depth error {worst_d:.4f} (lattice edge {h:.4f}), normal angle {worst_a:.4f} rad (faceting {math.sqrt(3) * h / R.SPHERE_R:.4f})")
    assert worst_d <= h
    assert worst_a <= math.sqrt(3) * h / R.SPHERE_R


# ------------------------------------------------------------------------------------------------ the host side
def _mesh(n_scenes=2, colour=True):
    g = torch.Generator().manual_seed(1)
    nv, nf = [0, 6, 10][:n_scenes + 1], [0, 3, 8][:n_scenes + 1]
    faces = torch.cat([torch.randint(nv[s], nv[s + 1], (nf[s + 1] - nf[s], 3), generator=g) for s in range(n_scenes)]).to(torch.int32)
    return fusion.TriangleMesh(vertices=torch.rand(nv[-1], 3, generator=g), faces=faces, rgb=torch.rand(nv[-1], 3, generator=g) if colour else None,
                               vertex_start=torch.tensor(nv, dtype=torch.int32), face_start=torch.tensor(nf, dtype=torch.int32))


def test_render_mesh_validates_its_arguments(monkeypatch):
    calls = []

    def run(vertices, colors, faces, vertex_start, face_start, cams, N, M, P, cull, znear, empty_depth, background):
        calls.append(dict(vertices=vertices, colors=colors, faces=faces, vertex_start=vertex_start, face_start=face_start, cams=cams, N=N, M=M,
                          P=P, cull=cull, znear=znear, empty_depth=empty_depth, background=background))
        return (None if colors is None else torch.zeros(N * M, 3, P, P), torch.full((N * M, P, P), empty_depth),
                torch.full((N * M, P, P), -1, dtype=torch.int32), torch.zeros(N * M, 3, P, P), torch.zeros(N * M, 3, P, P))

    monkeypatch.setattr(fusion, "_raster", run)
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("the library was touched"))
    M = 3
    cams = G.make_rig(M, True)[0]
    two = [cams, G.make_rig(M, True, seed=1)[0]]
    mesh = _mesh()
    rep = lambda **kw: dataclasses.replace(mesh, **kw)
    bad = [
        dict(size=0), dict(size=-4), dict(size=2.5), dict(size=2 ** 15),              # 2 x 3 x 2^30 pixels
        dict(cameras=[cams]), dict(cameras=cams), dict(cameras=two + [cams]),         # the sets must number the mesh's scenes
        dict(cameras=[cams, G.make_rig(M + 1, True)[0]]), dict(cameras=[]),           # unequal M; no set
        dict(mesh=mesh.vertices), dict(mesh="mesh"),
        dict(mesh=rep(vertices=mesh.vertices[:, :2])), dict(mesh=rep(faces=mesh.faces.long())), dict(mesh=rep(faces=mesh.faces[:, :2])),
        dict(mesh=rep(rgb=mesh.rgb[:-1])), dict(mesh=rep(face_start=mesh.face_start[:-1])),
        dict(znear=-1.0), dict(znear=float("nan")), dict(background=(1.0, 1.0)), dict(cull=2),
    ]
    for kw in bad:
        args = dict(mesh=mesh, cameras=two)
        args.update(kw)
        with pytest.raises(ValueError):
            fusion.render_mesh(**args)
    assert not calls                                   # nothing reached the library
    out = fusion.render_mesh(mesh, two)                # the defaults, as documented
    c = calls[-1]
    assert (c["N"], c["M"], c["P"], c["cull"]) == (2, M, 256, True) and c["cams"].shape == (2 * M, hip.CAM_RECORD)
    assert c["background"] == (1.0, 1.0, 1.0) and c["znear"] == 1e-3 and c["empty_depth"] == float("inf")
    assert c["vertex_start"].tolist() == [0, 6, 10] and c["face_start"].tolist() == [0, 3, 8]
    assert c["vertex_start"].dtype == c["face_start"].dtype == c["faces"].dtype == torch.int32
    assert out.rgb.shape == out.bary.shape == out.normal.shape == (2, M, 3, 256, 256)
    assert out.depth.shape == out.face.shape == out.hit.shape == (2, M, 256, 256)
    assert out.hit.dtype == torch.bool and not bool(out.hit.any())
    assert [f.name for f in dataclasses.fields(out)] == ["rgb", "depth", "face", "bary", "normal", "hit"]
    one = fusion.render_mesh(_mesh(1, colour=False), cams, size=16, cull=False)          # one scene, bare cameras: no leading dimension
    assert one.rgb is None and one.depth.shape == (M, 16, 16) and one.bary.shape == (M, 3, 16, 16) and calls[-1]["colors"] is None
    assert calls[-1]["cull"] is False
    assert fusion.render_mesh(_mesh(1), [cams], size=8).depth.shape == (1, M, 8, 8)      # ... listed: a leading 1


def test_depth_latent_is_shared_with_the_point_renderer_and_shaded_is_a_headlight():
    depth = torch.tensor([[[0.5, 1.5, 2.5], [3.0, 0.25, float("inf")]]])
    face = torch.tensor([[[0, 1, 2], [3, 4, -1]]], dtype=torch.int32)
    normal = torch.zeros(1, 3, 2, 3)
    normal[0, 2] = torch.tensor([[-1.0, -0.5, 0.0], [0.25, -2.0, 0.0]])
    rm = fusion.RenderedMesh(rgb=None, depth=depth, face=face, bary=torch.zeros(1, 3, 2, 3), normal=normal, hit=face >= 0)
    rv = fusion.RenderedViews(rgb=None, depth=depth, index=face, hit=face >= 0)
    assert rm.depth_latent().tolist() == [[[-1.0, 0.0, 1.0], [1.0, -1.0, 1.0]]]          # scale 2, shift 0.5; clamped; empty = +1
    for kw in (dict(), dict(depth_scale=4.0, depth_shift=0.5), dict(depth_scale=3.0)):
        assert torch.equal(rm.depth_latent(**kw), rv.depth_latent(**kw))
    sh = rm.shaded(background=(0.1, 0.2, 0.3))
    assert sh.shape == (1, 3, 2, 3) and sh[0, :, 0, 0].tolist() == [1.0, 1.0, 1.0] and sh[0, :, 0, 1].tolist() == [0.5, 0.5, 0.5]
    assert sh[0, :, 1, 0].tolist() == [0.0, 0.0, 0.0] and sh[0, :, 1, 1].tolist() == [1.0, 1.0, 1.0]          # clamped both ways
    assert torch.allclose(sh[0, :, 1, 2], torch.tensor([0.1, 0.2, 0.3]))


def test_the_header_and_the_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    stages = {k: int(v) for k, v in re.findall(r"#define\s+MVD_RENDER_(\w+)\s+(\d+)", hdr)}
    assert stages == dict(FILL=hip.RENDER_FILL, SPLAT=hip.RENDER_SPLAT, RESOLVE=hip.RENDER_RESOLVE, ALL=hip.RENDER_ALL)
    for name, extra in (("mvd_render_mesh_scratch", 0), ("mvd_render_mesh", 23), ("mvd_render_mesh_stages", 24)):
        decl = re.search(r"^\w+ " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
        assert decl is not None and name in hip.SIGNATURES
        assert len(hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == (extra or 2)
