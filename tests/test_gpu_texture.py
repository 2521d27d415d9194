"""Texturing on the GPU: mvd_texture_bake and mvd_texture_sample (csrc/texture.hip) through the C ABI against the float64 reference of
tests/texture_f64.py, and the host path (fusion.bake_texture, render_mesh(texture=...), sample_texture, write_obj, ViewFusion.texture).

Bounds -- none taken from what the kernels give:
  views, best     EQUAL to float64 on every kept owned texel (texture_f64.ambiguous: a texel with a (texel, view) pair where float64 sits
                  within the fp32 oracle's own error of one of the rule's comparisons is left out, at most 1 % of a case's owned
                  texels, asserted first)
  texture         max|kernel - f64| <= 4 max|fp32 oracle - f64| on those texels (two fp32 evaluations of the same formulas)
  on EVERY texel  no face: fill, views 0, best 255, exactly; views <= V; best < V exactly where views > 0
  lookup          nearest: EQUAL to float64 away from the rounding boundaries; bilinear: 4 x the fp32 oracle's error
  determinism, a scene alone against the batch, NULL outputs, the host path against the ABI: bit equality.
  end to end      mse(textured render) < mse(vertex-colour render) against the source views; the float64 chain alone shows the
                  inequality by a factor of 53 (tests/test_cpu_texture.py).

Measured on an MI355X: the figures stand in the docstring of each test; every kernel-to-oracle error ratio is 1.00.
"""
import ctypes

import pytest
import torch

import fusion_f64 as F
import raster_f64 as R
import texture_f64 as X

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
BACKGROUND = (0.25, 0.5, 0.75)


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


def _device(case):
    m = case.mesh
    i32 = lambda t: t.to(torch.int32).contiguous().cuda()
    return dict(vertices=m.vertices.contiguous().cuda(), colors=None if m.colors is None else m.colors.float().contiguous().cuda(),
                faces=i32(m.faces), vstart=i32(m.vertex_start), fstart=i32(m.face_start), cams=m.packed().cuda(), rgb=case.rgb.contiguous().cuda(),
                depth=case.depth.contiguous().cuda(), nvert=m.nvert, nface=m.nface, nscene=m.nscene, V=case.V, H=case.H, Pd=case.Pd,
                texels=case.texels, A=case.A, tol=case.tol, min_cos=case.min_cos, power=case.power, cull=m.cull, blend=case.blend, znear=m.znear)


def _buffers(nscene, A):
    return dict(texture=torch.full((nscene, 3, A, A), SENTINEL, device="cuda"), views=torch.full((nscene, A, A), 77, dtype=torch.uint8, device="cuda"),
                best=torch.full((nscene, A, A), 77, dtype=torch.uint8, device="cuda"))


def _untouched(out):
    return bool((out["texture"] == SENTINEL).all()) and bool((out["views"] == 77).all()) and bool((out["best"] == 77).all())


def _call(hip, out, d, texture=True, views=True, best=True, fill=X.FILL):
    p = lambda t: hip.ptr(t) if t is not None and t.numel() else None
    fl = None if fill is None else (ctypes.c_float * 3)(*fill)
    return hip.lib().mvd_texture_bake(p(d["vertices"]), p(d["colors"]), p(d["faces"]), hip.ptr(d["vstart"]), hip.ptr(d["fstart"]),
                                      hip.ptr(d["cams"]), hip.ptr(d["rgb"]), hip.ptr(d["depth"]), d["nvert"], d["nface"], d["nscene"], d["V"],
                                      d["H"], d["Pd"], d["texels"], d["A"], d["tol"], d["min_cos"], d["power"], d["cull"], d["blend"],
                                      d["znear"], fl, hip.ptr(out["texture"]) if texture else None, hip.ptr(out["views"]) if views else None,
                                      hip.ptr(out["best"]) if best else None, hip.stream())


def _bake(hip, case, **kw):
    out = _buffers(case.mesh.nscene, case.A)
    hip.check(_call(hip, out, _device(case), **kw))
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


# ------------------------------------------------------------------------------------------------ 1. parity against float64
@pytest.mark.parametrize("name", list(X.CASES))
def test_bake_vs_float64(hip, name):
    """Measured on an MI355X: kernel error / fp32-oracle error of the texture 1.00 on every case (0 ... 6.2e-7 against bounds of 0 ...
    2.5e-6); no views or best mismatch on the kept texels; left out 0 / 0 / 0 / 0 / 0 / 0 / 3 / 16 / 0 / 6 of 0 / 4 / 106 / 24 / 265 /
    10 464 / 20 928 / 138 648 / 200 / 20 960 owned texels."""
    ref = X.refs(name)          # asserts the cap
    case, want = ref.case, ref.baked
    got = {k: v.cpu() for k, v in _bake(hip, case).items()}
    V, owned, keep = case.V, want.owned, want.owned & ~ref.bad
    views, best = got["views"].long(), got["best"].long()
    wrong_views, wrong_best = int((views != want.views)[keep].sum()), int((best != want.best)[keep].sum())
    k3 = keep[:, None].expand_as(want.texture)
    err = float((got["texture"].double() - want.texture)[k3].abs().max()) if bool(keep.any()) else 0.0
    print(f"RATIO texture {name} | faces {case.mesh.nface} A {case.A} kept {int(keep.sum())}/{int(owned.sum())} owned texels | views mismatches "
          f"{wrong_views} best mismatches {wrong_best} | texture kernel {err:.2e} oracle {ref.oracle_err:.2e} bound {ref.bound:.2e} ratio "
          f"{err / ref.oracle_err if ref.oracle_err else 0.0:.2f} | seen {float((want.views > 0)[owned].float().mean()) if bool(owned.any()) else 0.0:.3f} "
          f"| oracle sets differ {ref.sets_differ}")
    assert wrong_views == 0 and wrong_best == 0
    assert err <= ref.bound
    # every texel, kept or not
    fill = torch.tensor(X.FILL).reshape(1, 3, 1, 1).expand_as(got["texture"])
    n3 = ~owned[:, None].expand_as(fill)
    assert torch.equal(got["texture"][n3], fill[n3]) and bool((views[~owned] == 0).all()) and bool((best[~owned] == 255).all())
    assert int(views.max()) <= V and torch.equal(best < V, views > 0) and bool((best[views == 0] == 255).all())
    assert bool(torch.isfinite(got["texture"]).all())
    if name == "three_scenes_empty_middle":
        assert bool((views[1] == 0).all()) and torch.equal(got["texture"][1], fill[1]) and bool((views[2] > 0).any())
    if name == "broken_faces_view_behind":
        assert bool((best != 2).all())          # the view behind the mesh contributes nowhere
        l, _, _ = X.chart_map(case.texels, case.C)
        for f, colour in ((30, "fill"), (31, "fill"), (case.mesh.nface - 2, "nan"), (case.mesh.nface - 1, "vertex")):
            m = (l == f)[None]
            assert int(m.sum()) == 8 and bool((views[m] == 0).all()), f
            if colour == "fill":          # an id outside the scene's vertices: no vertex is read
                assert torch.equal(got["texture"][m[:, None].expand_as(fill)], fill[m[:, None].expand_as(fill)]), f


# ------------------------------------------------------------------------------------------------ 2. bit equality
@pytest.mark.parametrize("name", ["sphere_t2_best_wide", "broken_faces_view_behind"])
def test_runs_are_identical_and_null_outputs_change_nothing(hip, name):
    case = X.refs(name).case
    one, again = _bake(hip, case), _bake(hip, case)
    for k in one:
        assert torch.equal(_bits(one[k]), _bits(again[k])), k
    for views, best in ((False, True), (True, False), (False, False)):
        part = _bake(hip, case, views=views, best=best)
        assert torch.equal(_bits(part["texture"]), _bits(one["texture"]))
        assert torch.equal(part["views"], one["views"]) if views else bool((part["views"] == 77).all())
        assert torch.equal(part["best"], one["best"]) if best else bool((part["best"] == 77).all())


def test_a_scene_alone_gives_what_it_gives_in_the_batch(hip):
    case = X.refs("three_scenes_empty_middle").case
    m, V = case.mesh, case.V
    batch = _bake(hip, case)
    for s in range(m.nscene):
        v0, v1, f0, f1 = (int(t[i]) for t in (m.vertex_start, m.face_start) for i in (s, s + 1))
        alone = R.Case(vertices=m.vertices[v0:v1], colors=m.colors[v0:v1], faces=m.faces[f0:f1] - v0, vertex_start=torch.tensor([0, v1 - v0]),
                       face_start=torch.tensor([0, f1 - f0]), cams=F.get_camera_slice(m.cams, list(range(s * V, (s + 1) * V))), nscene=1, M=V,
                       P=m.P, cull=m.cull)
        one = X.BakeCase(mesh=alone, rgb=case.rgb[s * V:(s + 1) * V], depth=case.depth[s * V:(s + 1) * V], texels=case.texels, side=case.A)
        got = _bake(hip, one)
        for k in got:
            assert torch.equal(_bits(got[k][0]), _bits(batch[k][s])), (s, k)


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refused_calls_write_nothing_and_name_themselves(hip):
    L = hip.lib()
    case = X.refs("nf5_t8_cull0").case
    good = _device(case)
    out = _buffers(1, case.A)
    bad = [dict(vertices=None), dict(faces=None), dict(nscene=0), dict(V=0), dict(V=255), dict(H=0), dict(Pd=0), dict(texels=0), dict(texels=65),
           dict(A=case.A + 1), dict(A=0), dict(texels=64, A=67 * 245), dict(nscene=9, A=11 * 1489), dict(tol=-1.0), dict(tol=float("nan")),
           dict(min_cos=1.0), dict(min_cos=-0.5), dict(power=-1), dict(power=9), dict(cull=2), dict(blend=2), dict(znear=-1.0),
           dict(nface=1 << 31)]
    for kw in bad:
        assert _call(hip, out, dict(good, **kw)) != 0, kw
        assert b"mvd_texture_bake" in L.mvd_last_error(), (kw, L.mvd_last_error())
    for kw in (dict(texture=False), dict(fill=None)):
        assert _call(hip, out, good, **kw) != 0 and b"mvd_texture_bake" in L.mvd_last_error(), kw
    torch.cuda.synchronize()
    assert _untouched(out)
    # the lookup
    P, M = 8, 2
    face = torch.zeros(M, P, P, dtype=torch.int32, device="cuda")
    bary, tex = torch.full((M, 3, P, P), 1.0 / 3.0, device="cuda"), torch.rand(1, 3, case.A, case.A, device="cuda")
    rgb = torch.full((M, 3, P, P), SENTINEL, device="cuda")
    bg = (ctypes.c_float * 3)(*BACKGROUND)
    good = dict(face=hip.ptr(face), bary=hip.ptr(bary), fstart=hip.ptr(_device(case)["fstart"]), texture=hip.ptr(tex), nface=5, nscene=1, M=M, P=P,
                texels=case.texels, A=case.A, filter=X.BILINEAR, background=bg, rgb=hip.ptr(rgb))
    bad = [dict(face=None), dict(bary=None), dict(fstart=None), dict(texture=None), dict(background=None), dict(rgb=None), dict(nscene=0),
           dict(M=0), dict(nscene=256, M=256), dict(P=0), dict(P=46341), dict(texels=0), dict(texels=65), dict(A=case.A - 1), dict(filter=2),
           dict(filter=-1), dict(nface=1 << 31)]
    for kw in bad:
        assert L.mvd_texture_sample(*dict(good, **kw).values(), hip.stream()) != 0, kw
        assert b"mvd_texture_sample" in L.mvd_last_error(), (kw, L.mvd_last_error())
    torch.cuda.synchronize()
    assert bool((rgb == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 4. the lookup
def _raster_case(case):
    """fusion._raster of a raster_f64 case -> (face (ncam, P, P) int32, bary (ncam, 3, P, P)) on the GPU."""
    from mvdfusion_amd import fusion
    i32 = lambda t: t.to(torch.int32).contiguous().cuda()
    _, _, face, bary, _ = fusion._raster(case.vertices.contiguous().cuda(), None, i32(case.faces), i32(case.vertex_start), i32(case.face_start),
                                         case.packed().cuda(), case.nscene, case.M, case.P, case.cull, case.znear, float("inf"), BACKGROUND)
    return face, bary


def _lookup(hip, face, bary, fstart, tex, nface, nscene, M, T, filt):
    P = face.shape[-1]
    rgb = torch.full((nscene * M, 3, P, P), SENTINEL, device="cuda")
    hip.check(hip.lib().mvd_texture_sample(hip.ptr(face), hip.ptr(bary), hip.ptr(fstart), hip.ptr(tex), nface, nscene, M, P, T, int(tex.shape[-1]),
                                           filt, (ctypes.c_float * 3)(*BACKGROUND), hip.ptr(rgb), hip.stream()))
    torch.cuda.synchronize()
    return rgb


@pytest.mark.parametrize("name,T", [("sphere_cull1", 3), ("two_scenes_empty_first", 1), ("big_and_small", 8)])
def test_sample_vs_float64(hip, name, T):
    """Measured on an MI355X (sphere_cull1 / two_scenes_empty_first / big_and_small): nearest equal on all 5 364 / 263 / 1 017 compared
    pixels; bilinear kernel error / fp32-oracle error 1.00 on every case (1.8e-5 / 7.0e-7 / 3.3e-6 against bounds of four times that)."""
    case = R.make_case(name)
    face, bary = _raster_case(case)
    fs = case.face_start.clamp(0, case.nface)
    C = X.cells_per_row(int((fs[1:] - fs[:-1]).max()))
    A = C * (T + 3)
    tex = torch.rand(case.nscene, 3, A, A, generator=torch.Generator().manual_seed(11))
    # pixels that are no face of the camera's scene: -1 is there already; an id past the faces, and a face of the other scene
    face = face.clone()
    face[:, 0, :4] = torch.tensor([case.nface, case.nface + 5, -2, 2 ** 31 - 1], dtype=torch.int32, device="cuda")
    if case.nscene > 1:
        face[:case.M, 1, :3] = int(fs[1])          # scene 0 (no face of its own) shows a face of scene 1
    fstart = fs.to(torch.int32).cuda()
    fc, bc = face.cpu().long(), bary.cpu()
    for filt in (X.NEAREST, X.BILINEAR):
        got = _lookup(hip, face, bary, fstart, tex.cuda(), case.nface, case.nscene, case.M, T, filt).cpu()
        want, near = X.sample(fc, bc, fs, case.nface, case.M, tex, T, filt, BACKGROUND)
        o32, _ = X.sample(fc, bc, fs, case.nface, case.M, tex, T, filt, BACKGROUND, dtype=torch.float32)
        scene = torch.arange(case.nscene * case.M)[:, None, None].expand_as(fc) // case.M
        inside = (fc >= fs[scene]) & (fc < fs[scene + 1])
        bg = torch.tensor(BACKGROUND).reshape(1, 3, 1, 1).expand_as(got)
        o3 = ~inside[:, None].expand_as(got)
        assert torch.equal(got[o3], bg[o3]) and bool(inside.any()) and not bool(inside[:, 0, :4].any())
        keep = (inside & ~near)[:, None].expand_as(got)
        assert float(near.float().mean()) <= X.MAX_EXCLUDED
        err, oracle = float((got.double() - want)[keep].abs().max()), float((o32.double() - want)[keep].abs().max())
        print(f"RATIO texture sample {name} filter {filt} | compared {int(keep.sum()) // 3} pixels | kernel {err:.2e} oracle {oracle:.2e} "
              f"ratio {err / oracle if oracle else 0.0:.2f}")
        if filt == X.NEAREST:
            assert err == 0.0
        else:
            assert err <= X.MARGIN * oracle


# ------------------------------------------------------------------------------------------------ 5. host path
def _triangle_mesh(m, colour=True):
    from mvdfusion_amd import fusion
    return fusion.TriangleMesh(vertices=m.vertices.cuda(), faces=m.faces.to(torch.int32).cuda(),
                               rgb=m.colors.float().cuda() if colour and m.colors is not None else None,
                               vertex_start=m.vertex_start.to(torch.int32), face_start=m.face_start.to(torch.int32))


def _sets(m):
    return [F.get_camera_slice(m.cams, list(range(s * m.M, (s + 1) * m.M))) for s in range(m.nscene)]


@pytest.mark.parametrize("name", ["sphere_t2_best_wide", "three_scenes_empty_middle"])
def test_host_path_equals_the_abi(hip, name, tmp_path):
    from mvdfusion_amd import fusion
    case = X.refs(name).case
    if case.side is not None:
        case = X.BakeCase(**{**vars(case), "side": None})          # the host always bakes the smallest atlas
    m, V, N = case.mesh, case.V, case.mesh.nscene
    want = _bake(hip, case)
    mesh, sets = _triangle_mesh(m), _sets(m)
    rgb, depth = case.rgb.reshape(N, V, 3, case.H, case.H).cuda(), case.depth.reshape(N, V, case.Pd, case.Pd).cuda()
    kw = dict(texels=case.texels, tolerance=case.tol, min_cos=case.min_cos, power=case.power, blend=("mean", "best")[case.blend],
              cull=bool(m.cull), fill=X.FILL)
    tex = fusion.bake_texture(mesh, rgb if N > 1 else rgb[0], sets if N > 1 else sets[0], depth=depth if N > 1 else depth[0], **kw)
    lead = (N,) if N > 1 else ()
    assert tex.image.shape == (*lead, 3, case.A, case.A) and tex.views.shape == tex.best.shape == (*lead, case.A, case.A)
    assert (tex.texels, tex.cells_per_row, tex.side) == (case.texels, case.C, case.A)
    for k, t in (("texture", tex.image), ("views", tex.views), ("best", tex.best)):
        assert torch.equal(_bits(t.reshape(want[k].shape)), _bits(want[k])), k
    own = tex.texel_face(mesh)
    cov = tex.coverage().reshape(-1).cpu()
    for s in range(N):
        o = own.reshape(N, case.A, case.A)[s] >= 0
        seen = float((want["views"][s].cpu() > 0)[o].float().mean()) if bool(o.any()) else 0.0
        assert abs(float(cov[s]) - seen) < 1e-6
    # depth=None renders the mesh's own depth: the rasteriser's, at the asked size
    auto = fusion.bake_texture(mesh, rgb if N > 1 else rgb[0], sets if N > 1 else sets[0], size=case.Pd, **kw)
    rm = fusion.render_mesh(_triangle_mesh(m, colour=False), sets if N > 1 else sets[0], size=case.Pd, cull=bool(m.cull))
    by_hand = fusion.bake_texture(mesh, rgb if N > 1 else rgb[0], sets if N > 1 else sets[0], depth=rm.depth, **kw)
    assert torch.equal(_bits(auto.image), _bits(by_hand.image)) and torch.equal(auto.views, by_hand.views) and bool((auto.views > 0).any())
    # render_mesh(texture=...) is the rasteriser followed by the lookup, for a mesh with or without colour
    P = 40
    i32 = lambda t: t.to(torch.int32).contiguous().cuda()
    for filt, code in (("bilinear", X.BILINEAR), ("nearest", X.NEAREST)):
        got = fusion.render_mesh(_triangle_mesh(m, colour=False), sets if N > 1 else sets[0], size=P, cull=bool(m.cull), background=BACKGROUND,
                                 texture=tex, filter=filt)
        plain = fusion.render_mesh(mesh, sets if N > 1 else sets[0], size=P, cull=bool(m.cull), background=BACKGROUND)
        assert torch.equal(got.face, plain.face) and torch.equal(_bits(got.bary), _bits(plain.bary)) and torch.equal(_bits(got.depth), _bits(plain.depth))
        abi = _lookup(hip, plain.face.reshape(N * V, P, P), plain.bary.reshape(N * V, 3, P, P), i32(m.face_start), want["texture"], m.nface, N, V,
                      case.texels, code)
        assert got.rgb.shape == plain.rgb.shape and torch.equal(_bits(got.rgb.reshape(abi.shape)), _bits(abi))
        assert torch.equal(got.rgb[(~got.hit).unsqueeze(-3).expand_as(got.rgb)], plain.rgb[(~plain.hit).unsqueeze(-3).expand_as(plain.rgb)])
        again = fusion.sample_texture(plain, mesh, tex, filter=filt, background=BACKGROUND)
        assert torch.equal(_bits(again.rgb), _bits(got.rgb)) and again.face is plain.face
    # write_obj from device tensors
    path = str(tmp_path / "mesh.obj")
    fusion.write_obj(path, mesh, tex, scene=N - 1 if N > 1 else None)
    text = open(path).read().splitlines()
    nf = int(m.face_start[N] - m.face_start[N - 1])
    assert sum(l.startswith("f ") for l in text) == nf and sum(l.startswith("vt ") for l in text) == 3 * nf
    assert open(str(tmp_path / "mesh.png"), "rb").read()[:8] == b"\x89PNG\r\n\x1a\n"


def test_viewfusion_texture_binds_the_decoder():
    """On the reduced-width model with test_gpu_fusion's small VAE and the shapes of test_gpu_simplify.py's keyword test."""
    from conftest import build_model
    from mvdfusion_amd import fusion
    from mvdfusion_amd import synthetic as syn
    from test_gpu_fusion import _small_vae
    V, S, up, G = 2, 32, 2, 32
    m = build_model(32)
    inp = syn.make_inputs(V, S, seed=2)
    x = (0.5 * torch.randn(V, 5, S, S, generator=torch.Generator().manual_seed(8))).cuda()
    assert not hasattr(m, "vae")
    m.vae = _small_vae()
    try:
        kw = dict(grid=G, up=up, simplify=8, half_extent=1.5, trunc=0.5)
        cams = inp["batch_cameras"]
        mesh = m.mesh(x, cams, **kw)
        assert isinstance(mesh, fusion.TriangleMesh) and len(mesh) > 0          # without the keyword the return value is what it was
        both = m.mesh(x, cams, texture=2, **kw)
        assert isinstance(both, tuple) and len(both) == 2
        for k in ("vertices", "faces", "rgb", "vertex_start", "face_start"):
            assert torch.equal(getattr(both[0], k), getattr(mesh, k)), k
        img = m._decoded(x)
        want = fusion.bake_texture(mesh, img, cams, texels=2)
        tex = m.texture(mesh, x, cams, texels=2)
        given = m.texture(mesh, x, cams, texels=2, decode=False, rgb=img)
        for t in (both[1], tex, given):
            assert torch.equal(_bits(t.image), _bits(want.image)) and torch.equal(t.views, want.views) and torch.equal(t.best, want.best)
        assert want.side == want.cells_per_row * 5 and bool((want.views > 0).any())
        with pytest.raises(ValueError, match="needs images"):
            m.texture(mesh, x, cams, decode=False)
        with pytest.raises(ValueError, match="needs images"):
            m.mesh(x, cams, decode=False, texture=2, **kw)
    finally:
        del m.vae


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_a_texture_keeps_the_detail_the_vertices_lose(hip):
    """The exact sphere at G = 24 with a colour wave finer than the cells of simplify_mesh(cells=6), rendered into three 64 x 64 views;
    the simplified mesh textured from those views at texels = 8 (a texel is 0.8 pixels) and rendered back into the same cameras, against
    its own vertex-colour render, on the pixels both meshes hit and whose four texture taps were all seen.

    Measured on an MI355X: 10 296 -> 252 faces, A = 132, coverage 0.627; on 7 724 pixels mse 0.00146 textured against 0.07813 with
    vertex colours (a factor of 53.7; the float64 chain alone: 0.00146 against 0.0781); max|kernel lookup - float64 lookup of the
    kernel's texture| 4.3e-6 against a bound of 7.9e-5."""
    from mvdfusion_amd import fusion
    fine = X.e2e_fine()
    P, T, cams = fine.P, X.E2E["texels"], _sets(fine)[0]
    src = fusion.render_mesh(_triangle_mesh(fine), cams, size=P, background=(0.0, 0.0, 0.0))
    coarse = fusion.simplify_mesh(_triangle_mesh(fine), cells=X.E2E["cells"])
    assert coarse.rgb is not None and 100 < len(coarse) < len(fine.faces) // 10
    tex = fusion.bake_texture(coarse, src.rgb, cams, texels=T, fill=X.FILL)
    vertex = fusion.render_mesh(coarse, cams, size=P, background=(0.0, 0.0, 0.0))
    textured = fusion.render_mesh(coarse, cams, size=P, background=(0.0, 0.0, 0.0), texture=tex)
    assert torch.equal(textured.face, vertex.face)
    mse_t, mse_v, pixels = X.e2e_errors(src.rgb.cpu(), src.hit.cpu(), vertex.face.cpu().long(), vertex.bary.cpu(), vertex.rgb.cpu(),
                                        coarse.face_start.long(), len(coarse), tex.image.cpu()[None], tex.views.cpu()[None], T)
    # the kernel's own lookup against this file's float64 lookup of the same texture, on those pixels' images
    look, _ = X.sample(vertex.face.cpu().long(), vertex.bary.cpu(), coarse.face_start.long(), len(coarse), fine.M, tex.image.cpu()[None], T,
                       X.BILINEAR, (0.0, 0.0, 0.0))
    diff = float((textured.rgb.cpu().double() - look).abs().max())
    print(f"E2E texture | faces {len(fine.faces)} -> {len(coarse)} | A {tex.side} coverage {float(tex.coverage()):.3f} | pixels {pixels} | "
          f"mse textured {mse_t:.5f} vertex colours {mse_v:.5f} ratio {mse_v / mse_t:.1f} | max|kernel lookup - f64 lookup| {diff:.2e}")
    assert pixels > 5000
    assert mse_t < mse_v
    # t is three products and two sums of numbers <= A per axis: at most 5 * 2^-24 A texels off, and a texel-to-texel step of the texture
    # is at most 1; the mix adds six roundings of values <= 1
    assert diff <= (10 * tex.side + 6) * 2.0 ** -24
