"""The mesh rasteriser on the GPU: mvd_render_mesh (csrc/raster.hip) through the C ABI against the float64 reference of
tests/raster_f64.py, and the host path (fusion.render_mesh, ViewFusion.render_mesh).

Bounds -- none taken from what the kernels give:
  face, hit       EQUAL to float64 on every compared pixel (raster_f64.excluded_pixels: pixels where float64 sits within the fp32 oracle's
                  own error of one of the rule's comparisons are left out, at most 1 % of a case's pixels, asserted first)
  depth, bary,    max|kernel - f64| <= 4 max|fp32 oracle - f64| + 2^-23 max|f64| on those pixels, each output with its own figures (two
  normal, rgb     fp32 evaluation orders of the same formulas, plus one rounding of the result)
  on EVERY pixel  depth finite and > znear where hit, empty_depth elsewhere; bary >= 0 with |sum - 1| <= 4 * 2^-23; |normal| = 1 within
                  4 * 2^-23 and normal_z <= 0; rgb within 3 * 2^-23 max|c| of the sum formed in torch from the kernel's own bary; the
                  z-buffer fully overwritten; and rendering ONLY the winning faces (gathered in ascending id order) gives the same bits in
                  depth, bary, normal and rgb and the same faces after relabelling -- a minimum over a subset that holds the winner
  ties, determinism, stages: bit equality.

Measured on an MI355X (icosahedron / big_and_small / sphere_cull0 / sphere_cull1 / two_scenes_empty_first / drop_rules): no face mismatch
on 512 / 1 024 / 6 912 / 6 912 / 1 024 / 2 048 compared pixels (none left out); kernel error / fp32-oracle error: depth 1.00 on every case
(3.5e-7 ... 2.3e-6 against bounds of 1.6e-6 ... 9.2e-6), bary 1.00 (7.1e-7 ... 3.5e-5 against 2.9e-6 ... 1.4e-4), rgb 1.00 (4.0e-7 ...
2.5e-5 against 1.7e-6 ... 1.0e-4), normal 0.93 / 0.85 / 1.19 / 1.19 / 0.58 / 1.50 (5.2e-8 ... 2.5e-7 against 4.2e-7 ... 9.5e-7).  End to
end: 12 340 faces, max|depth_latent - input| = 0.090912 against the float64 chain's 0.090911 (bound 0.090918: the discretisation of a 32^3
volume, at a silhouette pixel); no hole in the 153 closed rows of 240 (mesh 0, points at radius 0 also 0), in all rows mesh 51, points 160.
"""
import ctypes

import pytest
import torch

import fusion_f64 as F
import raster_f64 as R
import tsdf_f64 as T
from conftest import build_model

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
BACKGROUND = (0.25, 0.5, 0.75)
EMPTY_DEPTH = -3.0
EPS = 2.0 ** -23
OUTPUTS = ("face", "depth", "bary", "normal", "rgb")


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


def _buffers(ncam, P, nbytes):
    dev = "cuda"
    return dict(face=torch.full((ncam, P, P), -5, dtype=torch.int32, device=dev), depth=torch.full((ncam, P, P), SENTINEL, device=dev),
                bary=torch.full((ncam, 3, P, P), SENTINEL, device=dev), normal=torch.full((ncam, 3, P, P), SENTINEL, device=dev),
                rgb=torch.full((ncam, 3, P, P), SENTINEL, device=dev),
                scratch=torch.full((max(nbytes // 8, 1),), 0x1234, dtype=torch.int64, device=dev))


def _untouched(out):
    return bool((out["face"] == -5).all()) and all(bool((out[k] == SENTINEL).all()) for k in ("depth", "bary", "normal", "rgb")) and \
        bool((out["scratch"] == 0x1234).all())


def _call(hip, out, vertices, colors, faces, vstart, fstart, cams, nvert, nface, nscene, M, P, cull, znear=1e-3, rgb=True, nbytes=None,
          background=BACKGROUND, face=True, depth=True, bary=True, normal=True, scratch=True, stages=None, scratch_offset=0):
    bg = None if background is None else (ctypes.c_float * 3)(*background)
    p = hip.ptr
    nbytes = out["scratch"].numel() * 8 if nbytes is None else nbytes
    sc = ctypes.c_void_p(out["scratch"].data_ptr() + scratch_offset) if scratch else None
    args = [p(vertices), p(colors), p(faces), p(vstart), p(fstart), p(cams), nvert, nface, nscene, M, P, cull, znear, EMPTY_DEPTH, bg,
            p(out["face"]) if face else None, p(out["depth"]) if depth else None, p(out["bary"]) if bary else None,
            p(out["normal"]) if normal else None, p(out["rgb"]) if rgb else None, sc, nbytes]
    if stages is None:
        return hip.lib().mvd_render_mesh(*args, hip.stream())
    return hip.lib().mvd_render_mesh_stages(*args, stages, hip.stream())


def _device(case, color=True):
    i32 = lambda t: t.to(torch.int32).contiguous().cuda()
    return dict(vertices=case.vertices.contiguous().cuda(), colors=case.colors.float().contiguous().cuda() if color and case.colors is not None else None,
                faces=i32(case.faces), vstart=i32(case.vertex_start), fstart=i32(case.face_start), cams=case.packed().cuda(),
                nvert=case.nvert, nface=case.nface, nscene=case.nscene, M=case.M, P=case.P, cull=case.cull, znear=case.znear)


def _render(hip, case, color=True, stages=(None,), out=None):
    """mvd_render_mesh (or the given stage calls, in order) with every output buffer pre-filled."""
    nbytes = int(hip.lib().mvd_render_mesh_scratch(case.nscene * case.M, case.P))
    assert nbytes == case.pixels * 8
    out = _buffers(case.nscene * case.M, case.P, nbytes) if out is None else out
    dev = _device(case, color)
    for st in stages:
        hip.check(_call(hip, out, rgb=dev["colors"] is not None, stages=st, **dev))
    torch.cuda.synchronize()
    return out


def _check_every_pixel(hip, case, got):
    ncam, P = case.nscene * case.M, case.P
    face = got["face"].long()
    hit = face >= 0
    h3 = hit[:, None].expand(ncam, 3, P, P)
    assert int(face.min()) >= -1 and int(face.max()) < case.nface
    depth = got["depth"]
    assert bool(torch.isfinite(depth[hit]).all()) and bool((depth[hit] > case.znear).all()) and bool((depth[~hit] == EMPTY_DEPTH).all())
    bary = got["bary"]
    assert bool((bary >= 0).all()) and bool((bary[~h3] == 0).all())
    assert float((bary.double().sum(1) - 1.0)[hit].abs().max()) <= 4 * EPS
    n = got["normal"].double()
    assert float((n.norm(dim=1) - 1.0)[hit].abs().max()) <= 4 * EPS and bool((n[:, 2] <= 0).all()) and bool((n[~h3] == 0).all())
    if case.colors is not None:
        col = case.colors.float().cuda()[case.faces.cuda()[face.clamp(min=0)]]          # (ncam, P, P, 3 vertices, 3 channels)
        b = bary.permute(0, 2, 3, 1)
        want = (b[..., 0, None] * col[..., 0, :] + b[..., 1, None] * col[..., 1, :]) + b[..., 2, None] * col[..., 2, :]
        bg = torch.tensor(BACKGROUND, device="cuda").expand_as(want)
        want = torch.where(hit[..., None], want, bg).permute(0, 3, 1, 2)
        assert float((got["rgb"] - want).abs().max()) <= 3 * EPS * float(case.colors.abs().max())
        assert torch.equal(got["rgb"][~h3], want[~h3])
    assert bool((got["scratch"] != 0x1234).all())
    scene = R.face_scene(case).cuda()
    cam = torch.arange(ncam, device="cuda")[:, None, None].expand_as(face)
    assert bool((scene[face.clamp(min=0)] == cam // case.M)[hit].all())          # a camera shows only its own scene's faces
    # only the winners, in ascending id order: the same minimum
    keep = torch.unique(face[hit]).cpu()
    again = _render(hip, R.only_faces(case, keep))
    for k in ("depth", "bary", "normal", "rgb"):
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), k
    relabel = torch.where(again["face"] >= 0, keep.cuda()[again["face"].long().clamp(min=0)], torch.full_like(face, -1))
    assert torch.equal(relabel, face)


# ------------------------------------------------------------------------------------------------ 1. parity against float64
@pytest.mark.parametrize("name", list(R.CASES))
def test_render_mesh_vs_float64(hip, name):
    ref = R.refs(name)          # asserts the cap
    case, image, keep = ref.case, ref.image, ~ref.bad
    got = _render(hip, case)
    face = got["face"].cpu().long()
    wrong = int((face != image.face)[keep].sum())
    both = keep & image.hit & (face == image.face)
    line, failed = [], []
    for k, (oracle, bound) in ref.bounds.items():
        a, b = got[k].cpu().double(), getattr(image, k)
        m = both if a.dim() == 3 else both[:, None].expand_as(a)
        err = float((a - b)[m].abs().max()) if bool(m.any()) else 0.0
        line.append(f"{k} kernel {err:.2e} oracle {oracle:.2e} bound {bound:.2e} ratio {err / oracle if oracle else 0.0:.2f}")
        if not err <= bound:
            failed.append((k, err, bound))
    print(f"RATIO raster {name} | faces {case.nface} compared pixels {int(keep.sum())}/{keep.numel()} face mismatches {wrong} | "
          + " | ".join(line) + f" | hit {float(image.hit.float().mean()):.3f}")
    assert wrong == 0
    assert torch.equal((face >= 0)[keep], image.hit[keep])
    assert not failed, failed
    _check_every_pixel(hip, case, got)
    if name == "two_scenes_empty_first":
        assert bool((face[:case.M] == -1).all()) and bool((face[case.M:] >= 0).any())


# ------------------------------------------------------------------------------------------------ 2. bit equality
@pytest.mark.parametrize("name", ["big_and_small", "sphere_cull0"])
def test_runs_are_identical_and_a_duplicated_face_list_changes_nothing(hip, name):
    case = R.make_case(name)
    one, again = _render(hip, case), _render(hip, case)
    for k in OUTPUTS + ("scratch",):
        assert torch.equal(one[k].view(torch.int32 if k != "scratch" else torch.int64), again[k].view(torch.int32 if k != "scratch" else torch.int64)), k
    two = _render(hip, R.duplicated(case))
    assert 0 <= int(two["face"].max()) < case.nface          # the second copy has the higher ids and loses every tie
    for k in OUTPUTS:
        assert torch.equal(one[k].view(torch.int32), two[k].view(torch.int32)), k


def test_the_stages_compose_to_the_one_call(hip):
    case = R.make_case("big_and_small")
    one = _render(hip, case)
    staged = _render(hip, case, stages=(hip.RENDER_FILL | hip.RENDER_SPLAT,))
    assert bool((staged["face"] == -5).all()) and bool((staged["depth"] == SENTINEL).all())          # nothing resolved yet
    assert torch.equal(staged["scratch"], one["scratch"])
    staged = _render(hip, case, stages=(hip.RENDER_RESOLVE,), out=staged)
    for k in OUTPUTS + ("scratch",):
        assert torch.equal(one[k], staged[k]), k
    three = _render(hip, case, stages=(hip.RENDER_FILL, hip.RENDER_SPLAT, hip.RENDER_RESOLVE))
    for k in OUTPUTS:
        assert torch.equal(one[k], three[k]), k


def test_without_colour_the_other_outputs_are_the_same(hip):
    case = R.make_case("icosahedron")
    plain, full = _render(hip, case, color=False), _render(hip, case)
    assert bool((plain["rgb"] == SENTINEL).all()) and not bool((full["rgb"] == SENTINEL).any())
    for k in ("face", "depth", "bary", "normal"):
        assert torch.equal(plain[k], full[k]), k


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_bad_arguments_return_an_error_and_write_nothing(hip):
    L = hip.lib()
    case = R.make_case("icosahedron")
    P, M = case.P, case.M
    nbytes = int(L.mvd_render_mesh_scratch(M, P))
    assert nbytes == M * P * P * 8
    assert int(L.mvd_render_mesh_scratch(0, P)) == 0 and int(L.mvd_render_mesh_scratch(M, 0)) == 0 and int(L.mvd_render_mesh_scratch(-1, -1)) == 0
    good = _device(case)
    out = _buffers(M, P, nbytes)
    bad = [dict(vertices=None), dict(faces=None), dict(vstart=None), dict(fstart=None), dict(cams=None), dict(face=False), dict(depth=False),
           dict(bary=False), dict(normal=False), dict(scratch=False),
           dict(rgb=False), dict(colors=None), dict(background=None),              # colour and rgb go together; colour needs a background
           dict(P=0), dict(P=-2), dict(nscene=0), dict(M=0), dict(nscene=-1), dict(nscene=4096, M=16),          # 65536 cameras
           dict(P=1 << 15, nbytes=1 << 62),                                      # 2 x 2^30 pixels
           dict(nface=1 << 31), dict(cull=2), dict(cull=-1), dict(znear=-0.5), dict(znear=float("nan")),
           dict(nbytes=nbytes - 8), dict(nbytes=0), dict(scratch_offset=4, nbytes=nbytes - 8)]
    for stages in (None, hip.RENDER_SPLAT):
        for kw in bad:
            a = dict(good)
            a.update(kw)
            assert _call(hip, out, stages=stages, **a) != 0, kw
            assert (b"mvd_render_mesh_stages" if stages else b"mvd_render_mesh:") in L.mvd_last_error(), (kw, L.mvd_last_error())
    for stages in (0, 8):
        assert _call(hip, out, stages=stages, **good) != 0 and b"mvd_render_mesh_stages" in L.mvd_last_error()
    torch.cuda.synchronize()
    assert _untouched(out)
    # no face at all: a valid call, every pixel empty, with and without colour
    empty = dict(good, vertices=None, faces=None, nvert=0, nface=0)
    assert _call(hip, out, **empty) == 0
    torch.cuda.synchronize()
    assert bool((out["face"] == -1).all()) and bool((out["depth"] == EMPTY_DEPTH).all()) and bool((out["bary"] == 0).all())
    assert bool((out["normal"] == 0).all()) and bool((out["scratch"] == -1).all())
    assert torch.equal(out["rgb"], torch.tensor(BACKGROUND, device="cuda").reshape(1, 3, 1, 1).expand(M, 3, P, P))
    out = _buffers(M, P, nbytes)
    assert _call(hip, out, rgb=False, background=None, **dict(empty, colors=None)) == 0
    torch.cuda.synchronize()
    assert bool((out["face"] == -1).all()) and bool((out["rgb"] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 4. host path
def _triangle_mesh(case, colour=True):
    from mvdfusion_amd import fusion
    return fusion.TriangleMesh(vertices=case.vertices.cuda(), faces=case.faces.to(torch.int32).cuda(),
                               rgb=case.colors.float().cuda() if colour else None, vertex_start=case.vertex_start.to(torch.int32),
                               face_start=case.face_start.to(torch.int32))


def _sets(case):
    return [F.get_camera_slice(case.cams, list(range(s * case.M, (s + 1) * case.M))) for s in range(case.nscene)]


def test_render_mesh_host_path(hip):
    from mvdfusion_amd import fusion
    for name in ("icosahedron", "two_scenes_empty_first"):
        case = R.make_case(name)
        N, M, P = case.nscene, case.M, case.P
        got = _render(hip, case)
        sets = _sets(case)
        rm = fusion.render_mesh(_triangle_mesh(case), sets if N > 1 else sets[0], size=P, cull=bool(case.cull), background=BACKGROUND,
                                empty_depth=EMPTY_DEPTH)
        lead = (N, M) if N > 1 else (M,)
        assert rm.rgb.shape == rm.bary.shape == rm.normal.shape == (*lead, 3, P, P)
        assert rm.depth.shape == rm.face.shape == rm.hit.shape == (*lead, P, P) and rm.face.dtype == torch.int32
        for k in OUTPUTS:
            assert torch.equal(getattr(rm, k).reshape(got[k].shape), got[k]), (name, k)
        assert torch.equal(rm.hit, rm.face >= 0) and bool(rm.hit.any()) and bool((~rm.hit).any())
        bare = fusion.render_mesh(_triangle_mesh(case, colour=False), sets if N > 1 else sets[0], size=P, cull=bool(case.cull),
                                  empty_depth=EMPTY_DEPTH)
        assert bare.rgb is None and torch.equal(bare.face, rm.face) and torch.equal(bare.bary, rm.bary)
        rv = fusion.RenderedViews(rgb=None, depth=rm.depth, index=rm.face, hit=rm.hit)
        for kw in (dict(), dict(depth_scale=3.0, depth_shift=0.25)):
            assert torch.equal(rm.depth_latent(**kw), rv.depth_latent(**kw))
        dl = rm.depth_latent()
        assert bool((dl[~rm.hit] == 1.0).all()) and float(dl.min()) >= -1.0 and float(dl[rm.hit].max()) < 1.0
        sh = rm.shaded(background=BACKGROUND)
        assert sh.shape == rm.normal.shape and torch.equal(sh[..., 0, :, :][rm.hit], (-rm.normal[..., 2, :, :]).clamp(0, 1)[rm.hit])
        if N > 1:          # a listed single set gets the leading 1; a wrong number of sets is refused
            first = _triangle_mesh(case).scene(1)
            one = fusion.render_mesh(first, [sets[1]], size=P, background=BACKGROUND, empty_depth=EMPTY_DEPTH)
            assert one.depth.shape == (1, M, P, P) and torch.equal(one.depth[0], rm.depth[1]) and torch.equal(one.rgb[0], rm.rgb[1])
            for cams in (sets[0], sets[:1], sets + sets[:1]):
                with pytest.raises(ValueError):
                    fusion.render_mesh(_triangle_mesh(case), cams, size=P)
        with pytest.raises(ValueError):
            fusion.render_mesh(_triangle_mesh(case), sets if N > 1 else sets[0], size=0)
        with pytest.raises(ValueError):
            fusion.render_mesh(case.vertices.cuda(), sets[0], size=P)


def test_viewfusion_render_mesh_binds_the_models_depth_map():
    from mvdfusion_amd import fusion
    m = build_model(32)
    case = R.make_case("icosahedron")
    mesh, cams = _triangle_mesh(case, colour=False), _sets(case)[0]
    keep = m.view_attn.depth_scale, m.view_attn.depth_shift
    try:
        m.view_attn.depth_scale, m.view_attn.depth_shift = 3.0, 0.25          # (not the interface defaults: the binding must show)
        rm = m.render_mesh(mesh, cams, size=16)
        want = fusion.render_mesh(mesh, cams, size=16)
        assert rm.rgb is None and torch.equal(rm.face, want.face) and torch.equal(rm.depth, want.depth) and bool(rm.hit.any())
        assert torch.equal(rm.depth_latent(), want.depth_latent(depth_scale=3.0, depth_shift=0.25))
        assert not torch.equal(rm.depth_latent(), want.depth_latent())
        assert torch.equal(rm.depth_latent(fusion.DEPTH_SCALE, fusion.DEPTH_SHIFT), want.depth_latent())
        both = m.render_mesh(mesh, cams, size=16, cull=False, empty_depth=EMPTY_DEPTH)
        assert torch.equal(both.face, want.face) and bool((both.depth[~both.hit] == EMPTY_DEPTH).all())          # closed, seen from outside
    finally:
        m.view_attn.depth_scale, m.view_attn.depth_shift = keep


# ------------------------------------------------------------------------------------------------ 5. end to end
def _row_holes(hit, fg, rows):
    """Over the (view, row) pairs of `rows` ((V, S) bool) with input foreground: the pixels of the foreground's extent that lie between
    the row's first and last hit and are not hit."""
    holes = 0
    for v, y in torch.nonzero(rows & fg.any(2)).tolist():
        xs = torch.nonzero(fg[v, y]).reshape(-1)
        row = hit[v, y, int(xs[0]):int(xs[-1]) + 1]
        on = torch.nonzero(row).reshape(-1)
        if on.numel():
            holes += int((~row[int(on[0]):int(on[-1]) + 1]).sum())
    return holes


def _open_rows(vertices, faces, cams, P):
    """(V, P) bool: the rows a visible opening of the mesh touches.  An opening is bounded by boundary edges (tsdf_f64.boundary_edges); on
    this data -- a sphere of radius r around the origin -- an edge is on the side camera C sees when an end has X . C > r^2.  Its rows
    are those its projection spans, grown by a pixel."""
    e = torch.from_numpy(T.boundary_edges(faces)[0])
    V = len(cams)
    edges = R.Case(vertices=vertices, colors=None, faces=torch.stack([e[:, 0], e[:, 1], e[:, 1]], dim=1), vertex_start=torch.tensor([0, vertices.shape[0]]),
                   face_start=torch.tensor([0, e.shape[0]]), cams=cams, nscene=1, M=V, P=P, cull=0)
    py = R.setup(edges).py[..., :2]                          # (edges, V, 2 ends)
    X = vertices.double()[e]
    out = torch.zeros(V, P, dtype=torch.bool)
    for v in range(V):
        C = -cams.T[v].double() @ torch.linalg.inv(cams.R[v].double())
        seen = ((X @ C) > F.SPHERE_R ** 2).any(1)
        lo, hi = (py[seen, v].amin(-1) - 1).floor().clamp(0, P - 1).long(), (py[seen, v].amax(-1) + 1).ceil().clamp(0, P - 1).long()
        for y0, y1 in zip(lo.tolist(), hi.tolist()):
            out[v, y0:y1 + 1] = True
    return out


def test_views_to_mesh_to_views_gives_back_the_depth_maps_without_holes(hip):
    """sphere_case(V = 8, S = 32) -> integrate_tsdf(grid = 32) -> extract_mesh -> render_mesh into the rig's own cameras at size 32.  Over
    the pixels that are hit and foreground in the input, max|depth_latent - input depth channel| is the discretisation of a 32^3 volume:
    recorded, and held to the same quantity of the float64 chain (tsdf_f64.integrate -> march -> raster_f64.render) plus the parity bound
    of that render.  The mesh of this case is open at the poles of the sphere, which lie on silhouettes or behind every view of the rig
    (the section on the volumetric fusion: 510 boundary edges): the rows a visible opening touches (_open_rows) are counted and
    printed but belong to no closed part.  In every other row `hit` is one contiguous run inside the input's foreground run: the closed
    part of the surface has no holes.  The hole counts of render_points at radius 0 on the fused cloud of the same views are printed
    next to the mesh's."""
    from mvdfusion_amd import fusion
    fcase = F.sphere_case(V=8, S=32)
    V, S = fcase.V, fcase.S
    lat = fcase.lat.cuda()
    mesh = fusion.extract_mesh(fusion.integrate_tsdf(lat, fcase.cams, grid=32))
    rm = fusion.render_mesh(mesh, fcase.cams, size=S)
    fg = F.foreground(fcase)
    hit = rm.hit.cpu()
    on = hit & fg
    err = float((rm.depth_latent().cpu() - fcase.lat[:, 4])[on].abs().max())
    # the float64 chain
    tcase = T.TCase(views=fcase, G=32)
    vol = T.integrate(tcase)
    m64 = T.march(vol.tsdf.float(), vol.weight)
    case = R.Case(vertices=m64.vertices.float(), colors=None, faces=m64.faces, vertex_start=m64.vertex_start, face_start=m64.face_start,
                  cams=fcase.cams, nscene=1, M=V, P=S, cull=1)
    ref = R.reference(case)
    lat64 = torch.clamp(2.0 * (ref.image.depth - fcase.depth_shift) / fcase.depth_scale - 1.0, -1.0, 1.0)
    on64 = ref.image.hit & fg
    err64 = float((lat64 - fcase.lat[:, 4].double())[on64].abs().max())
    bound = err64 + ref.bounds["depth"][1] * 2.0 / fcase.depth_scale
    cloud = fusion.fuse_views(lat, fcase.cams)
    pts = fusion.render_points(cloud, fcase.cams, size=S, radius=0)
    closed = ~_open_rows(mesh.vertices.cpu(), mesh.faces.cpu().long(), fcase.cams, S)
    every = torch.ones_like(closed)
    holes_mesh, holes_points = _row_holes(hit, fg, closed), _row_holes(pts.hit.cpu(), fg, closed)
    print(f"end to end: {len(mesh)} faces, hit {float(hit.float().mean()):.3f} (foreground {float(fg.float().mean()):.3f}), depth latent error "
          f"{err:.6f} float64 chain {err64:.6f} bound {bound:.6f} | row holes in the {int((closed & fg.any(2)).sum())} closed rows of "
          f"{int(fg.any(2).sum())}: mesh {holes_mesh}, points at radius 0 {holes_points}; in all rows: mesh {_row_holes(hit, fg, every)}, "
          f"points {_row_holes(pts.hit.cpu(), fg, every)}")
    assert int((closed & fg.any(2)).sum()) >= int(fg.any(2).sum()) // 2
    assert len(mesh) > 1000 and float(on.float().mean()) > 0.8 * float(fg.float().mean())
    assert err <= bound, (err, bound)
    assert holes_mesh == 0
