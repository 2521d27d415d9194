"""Volumetric fusion on the GPU: mvd_tsdf_integrate / mvd_mesh_count / mvd_mesh_emit (csrc/tsdf.hip) through the C ABI against the float64
reference of tests/tsdf_f64.py, and the host path (mvdfusion_amd/fusion.py integrate_tsdf / extract_mesh, ViewFusion.mesh).

Bounds -- none taken from what the kernels give:
  weight, cweight   EQUAL to float64 on every compared voxel (tsdf_f64.undecidable: pairs within the fp32 oracle's own error of one of the
                    rule's comparisons are left out, at most 1 % of a case's pairs, asserted first)
  tsdf, colour      max|kernel - f64| <= 4 max|fp32 oracle - f64| + 2^-23 over the compared voxels (two fp32 evaluation orders of the same
                    formulas, plus one rounding of a result of magnitude <= 1)
  weight == 0       => tsdf == 1.0f exactly, on EVERY voxel
  faces, vertex_start, face_start   EQUAL to the marching oracle's (the signs of a caller-made volume are exact inputs)
  vertices, vertex colours          max|kernel - f64| <= 4 max|fp32 oracle - f64| + 2^-23 max|f64|
  determinism       bit equality of two runs.
Measured on an MI355X: tsdf kernel error / fp32-oracle error = 1.00 on four cases and 1.08 at G = 33 (4.5e-7 ... 9.5e-6 against bounds of
1.9e-6 ... 3.5e-5), colour 1.00 (6.1e-7, 2.0e-6 against 2.6e-6, 8.3e-6), no count mismatch on 125 / 729 / 35 931 / 1 458 / 729 compared
voxels; marching: vertices 1.00 x the oracle's error on every volume (8.9e-8 ... 1.1e-7 against 4.3e-7 ... 5.3e-7), faces and offsets equal;
sphere: 6 505 vertices, 12 340 faces, max | |x| - 0.6 | = 2.572352e-2 against the float64 oracle's 2.572356e-2 + 2.1e-7.
"""
import functools
import math

import pytest
import torch

import tsdf_f64 as T
from conftest import build_model

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
F = T.F


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


@functools.lru_cache(maxsize=None)
def _refs(name):
    """(case, float64 reference, fp32 oracle, undecidable pairs for tsdf, for colour) -- once per case, shared read-only; the cap is
    asserted here."""
    case = T.make_case(name)
    ref, o32 = T.integrate(case), T.integrate(case, torch.float32)
    bad, bad_colour, _, _ = T.undecidable(case, ref, o32)
    return case, ref, o32, bad, bad_colour


def _integrate(hip, case, colour=True, **kw):
    """One mvd_tsdf_integrate launch; every output buffer is pre-filled, the colour buffers are passed even without rgb."""
    c = case.views
    N, G = c.nscene, case.G
    dev = "cuda"
    out = dict(tsdf=torch.full((N, G, G, G), SENTINEL, device=dev), weight=torch.full((N, G, G, G), 99, dtype=torch.uint8, device=dev),
               color=torch.full((N, G, G, G, 3), SENTINEL, device=dev), cweight=torch.full((N, G, G, G), 99, dtype=torch.uint8, device=dev))
    lat, cams = c.lat.contiguous().cuda(), c.packed().cuda()
    rgb = case.rgb.contiguous().cuda() if colour and case.rgb is not None else None
    a = dict(nscene=N, V=c.V, S=c.S, up=c.up, G=G, center=case.center, half_extent=case.half_extent, trunc=case.trunc, carve=case.carve,
             lo=c.lo, hi=c.hi)
    a.update(kw)
    rc = hip.lib().mvd_tsdf_integrate(hip.ptr(lat), hip.ptr(rgb), hip.ptr(cams), hip.ptr(out["tsdf"]), hip.ptr(out["weight"]),
                                      hip.ptr(out["color"]), hip.ptr(out["cweight"]), a["nscene"], a["V"], a["S"], a["up"], a["G"],
                                      *(float(v) for v in a["center"]), float(a["half_extent"]), float(a["trunc"]), int(a["carve"]),
                                      float(c.depth_scale), float(c.depth_shift), float(a["lo"]), float(a["hi"]), hip.stream())
    torch.cuda.synchronize()
    return rc, out


def _mesh(hip, tsdf, weight=None, color=None, cweight=None, center=(0.0, 0.0, 0.0), half_extent=0.75, fill=(0.5, 0.5, 0.5)):
    """mvd_mesh_count, the read of the offsets, mvd_mesh_emit into exact, pre-filled outputs -- all through the C ABI."""
    import ctypes
    L = hip.lib()
    N, G = tsdf.shape[0], tsdf.shape[1]
    dev = "cuda"
    tsdf = tsdf.float().contiguous().cuda()
    weight = (torch.ones(N, G, G, G, dtype=torch.uint8) if weight is None else weight).contiguous().cuda()
    color, cweight = (None if t is None else t.contiguous().cuda() for t in (color, cweight))
    nbytes = int(L.mvd_mesh_scratch(N, G))
    assert nbytes >= 4 * (7 * N * G ** 3 + N * (G - 1) ** 3)
    scratch = torch.full((nbytes // 4,), -3, dtype=torch.int32, device=dev)
    starts = torch.full((2, N + 1), -9, dtype=torch.int32, device=dev)
    hip.check(L.mvd_mesh_count(hip.ptr(tsdf), hip.ptr(weight), N, G, hip.ptr(starts[0]), hip.ptr(starts[1]), hip.ptr(scratch), nbytes,
                               hip.stream()))
    starts = starts.cpu()
    nv, nf = int(starts[0, N]), int(starts[1, N])
    assert 0 <= nv <= 7 * N * G ** 3 and 0 <= nf <= 12 * N * (G - 1) ** 3
    vertices = torch.full((nv, 3), SENTINEL, device=dev)
    colors = torch.full((nv, 3), SENTINEL, device=dev) if color is not None else None
    faces = torch.full((nf, 3), -5, dtype=torch.int32, device=dev)
    p = lambda t: hip.ptr(t) if t is not None and t.numel() else None
    hip.check(L.mvd_mesh_emit(hip.ptr(tsdf), hip.ptr(weight), hip.ptr(color), hip.ptr(cweight), N, G, *(float(v) for v in center),
                              float(half_extent), (ctypes.c_float * 3)(*fill), p(vertices), p(colors), p(faces), nv, nf, hip.ptr(scratch),
                              nbytes, hip.stream()))
    torch.cuda.synchronize()
    return dict(vertices=vertices.cpu(), colors=None if colors is None else colors.cpu(), faces=faces.cpu(), vertex_start=starts[0],
                face_start=starts[1])


# ------------------------------------------------------------------------------------------------ 1. integrate against float64
@pytest.mark.parametrize("name", list(T.CASES))
def test_tsdf_integrate_vs_float64(hip, name):
    case, ref, o32, bad, bad_colour = _refs(name)
    keep = T.compared(bad, case)
    rc, got = _integrate(hip, case)
    hip.check(rc)
    tsdf, weight = got["tsdf"].cpu(), got["weight"].cpu().long()
    err = float((tsdf.double() - ref.tsdf).abs()[keep].max())
    oerr = float((o32.tsdf.double() - ref.tsdf).abs()[keep].max())
    bound = T.MARGIN * oerr + 2.0 ** -23
    wrong = int((weight != ref.weight)[keep].sum())
    line = (f"RATIO tsdf {name} | kernel {err:.2e} oracle {oerr:.2e} bound {bound:.2e} | compared voxels {int(keep.sum())}/{keep.numel()} "
            f"weight mismatches {wrong} | observed {float((weight > 0).float().mean()):.3f}")
    if case.rgb is not None:
        keepc = T.compared(bad_colour, case)
        color, cweight = got["color"].cpu(), got["cweight"].cpu().long()
        cerr = float((color.double() - ref.color).abs()[keepc].max())
        coerr = float((o32.color.double() - ref.color).abs()[keepc].max())
        cbound = T.MARGIN * coerr + 2.0 ** -23
        cwrong = int((cweight != ref.cweight)[keepc].sum())
        line += f" | colour kernel {cerr:.2e} oracle {coerr:.2e} bound {cbound:.2e} cweight mismatches {cwrong}"
    print(line)
    assert wrong == 0
    assert err <= bound, (err, bound)
    assert bool((tsdf[weight == 0] == 1.0).all()) and int((weight == 0).sum()) > 0          # EVERY voxel, compared or not
    assert int(weight.max()) <= case.views.V
    if case.rgb is not None:
        assert cwrong == 0
        assert cerr <= cbound, (cerr, cbound)
        assert bool((color[cweight == 0] == 0).all()) and bool((cweight <= weight).all())
        # rgb = NULL: the colour buffers are not touched, everything else is the same
        rc, plain = _integrate(hip, case, colour=False)
        hip.check(rc)
        assert bool((plain["color"] == SENTINEL).all()) and bool((plain["cweight"] == 99).all())
        assert torch.equal(plain["tsdf"], got["tsdf"]) and torch.equal(plain["weight"], got["weight"])
    else:
        assert bool((got["color"] == SENTINEL).all()) and bool((got["cweight"] == 99).all())


def test_tsdf_bad_arguments_return_an_error(hip):
    L = hip.lib()
    case = T.make_case("v3_s8_g5")
    rc, _ = _integrate(hip, case)
    assert rc == 0
    for kw in (dict(G=1), dict(G=257), dict(G=256, nscene=19), dict(trunc=0.0), dict(trunc=-0.1), dict(trunc=float("nan")),
               dict(half_extent=0.0), dict(half_extent=-1.0), dict(half_extent=float("nan")), dict(V=0), dict(V=256), dict(S=1), dict(up=0),
               dict(nscene=0), dict(lo=0.5, hi=0.5)):
        rc, out = _integrate(hip, case, **kw)
        assert rc != 0, kw
        assert b"mvd_tsdf_integrate" in L.mvd_last_error(), kw
        assert bool((out["tsdf"] == SENTINEL).all())
    assert int(L.mvd_mesh_scratch(1, 1)) == 0 and int(L.mvd_mesh_scratch(19, 256)) == 0 and int(L.mvd_mesh_scratch(0, 8)) == 0
    vol, w = torch.zeros(1, 4, 4, 4, device="cuda"), torch.ones(1, 4, 4, 4, dtype=torch.uint8, device="cuda")
    starts = torch.zeros(2, 2, dtype=torch.int32, device="cuda")
    nbytes = int(L.mvd_mesh_scratch(1, 4))
    scratch = torch.zeros(nbytes // 4, dtype=torch.int32, device="cuda")
    p = hip.ptr
    count = lambda **a: L.mvd_mesh_count(p(a.get("vol", vol)), p(a.get("w", w)), 1, a.get("G", 4), p(starts[0]), p(starts[1]),
                                         p(a.get("scratch", scratch)), a.get("nbytes", nbytes), hip.stream())
    assert count() == 0
    for a in (dict(vol=None), dict(w=None), dict(scratch=None), dict(G=1), dict(G=257), dict(nbytes=nbytes - 4)):
        assert count(**a) != 0, a
        assert b"mvd_mesh_count" in L.mvd_last_error(), a
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. marching against the oracle
def _unobserved(shape, share, seed):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) >= share).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def _volume(name):
    """(tsdf, weight or None, color or None, cweight or None) of a caller-made volume."""
    g = torch.Generator().manual_seed(31)
    if name == "smooth_g5":
        return T.smooth_volume(5, 0), None, None, None
    if name == "smooth_g9_rgb":
        return T.smooth_volume(9, 1), None, torch.rand(1, 9, 9, 9, 3, generator=g), _unobserved((1, 9, 9, 9), 0.3, 5)
    if name == "smooth_g33":                                   # 7 * 33^3 edges = 983 blocks of 256
        return T.smooth_volume(33, 2), None, None, None
    if name == "smooth_g65":                                   # 7 510 edge blocks: the scan takes 2 048 counts a trip, its carry loop runs four
        return T.smooth_volume(65, 8), None, None, None
    if name == "unobserved_g9_rgb":                            # about 20 % of the voxels unobserved
        return T.smooth_volume(9, 3), _unobserved((1, 9, 9, 9), 0.2, 6), torch.rand(1, 9, 9, 9, 3, generator=g), _unobserved((1, 9, 9, 9), 0.5, 7)
    if name == "two_scenes_first_empty":
        return torch.cat([torch.ones(1, 9, 9, 9), T.smooth_volume(9, 4)]), None, None, None
    if name == "no_crossing":
        return torch.full((2, 5, 5, 5), 0.25), None, None, None
    raise KeyError(name)


VOLUMES = ("smooth_g5", "smooth_g9_rgb", "smooth_g33", "smooth_g65", "unobserved_g9_rgb", "two_scenes_first_empty", "no_crossing")


@functools.lru_cache(maxsize=None)
def _marched(name):
    vol = _volume(name)
    fill = (0.25, 0.5, 0.75)
    return T.march(*vol, fill=fill), T.march(*vol, fill=fill, dtype=torch.float32), fill


def _vertex_bound(ref, o32, key="vertices"):
    a, b = getattr(ref, key), getattr(o32, key)
    if a.numel() == 0:
        return 0.0, 0.0
    oerr = float((b.double() - a).abs().max())
    return oerr, T.MARGIN * oerr + 2.0 ** -23 * float(a.abs().max())


@pytest.mark.parametrize("name", VOLUMES)
def test_mesh_vs_oracle(hip, name):
    tsdf, weight, color, cweight = _volume(name)
    ref, o32, fill = _marched(name)
    got = _mesh(hip, tsdf, weight, color, cweight, fill=fill)
    N = tsdf.shape[0]
    assert torch.equal(got["vertex_start"].long(), ref.vertex_start) and torch.equal(got["face_start"].long(), ref.face_start)
    assert torch.equal(got["faces"].long(), ref.faces)
    oerr, bound = _vertex_bound(ref, o32)
    err = float((got["vertices"].double() - ref.vertices).abs().max()) if len(ref.vertices) else 0.0
    line = f"RATIO mesh {name} | vertices {len(ref.vertices)} faces {len(ref.faces)} | kernel {err:.2e} oracle {oerr:.2e} bound {bound:.2e}"
    assert err <= bound, (err, bound)
    if color is not None:
        coerr, cbound = _vertex_bound(ref, o32, "colors")
        cerr = float((got["colors"].double() - ref.colors).abs().max())
        line += f" | colour kernel {cerr:.2e} oracle {coerr:.2e} bound {cbound:.2e}"
        assert cerr <= cbound, (cerr, cbound)
        assert bool((got["colors"] == torch.tensor(fill)).all(1).any())          # the fill colour occurs
    print(line)
    if name == "two_scenes_first_empty":
        assert int(got["vertex_start"][1]) == 0 and int(got["face_start"][1]) == 0 and len(ref.faces) > 0
    elif name == "no_crossing":
        assert got["vertex_start"].tolist() == [0] * (N + 1) and got["face_start"].tolist() == [0] * (N + 1)
    else:
        assert len(ref.faces) > 0
    if name == "smooth_g33":
        assert (7 * 33 ** 3 + 255) // 256 == 983
    if name == "smooth_g65":
        assert (7 * 65 ** 3 + 255) // 256 > 3 * 8 * 256
    if name == "unobserved_g9_rgb":
        assert 0.1 < float((weight == 0).float().mean()) < 0.3


# ------------------------------------------------------------------------------------------------ 3. determinism, end to end
@functools.lru_cache(maxsize=None)
def _sphere():
    """The sphere seen by 8 views at S = 32 in a 32^3 volume: (case, float64 volume, float64 mesh of it)."""
    case = T.TCase(views=F.sphere_case(V=8, S=32), G=32, half_extent=0.75)
    ref = T.integrate(case)
    return case, ref, T.march(ref.tsdf, ref.weight, half_extent=0.75)


def test_two_runs_give_the_same_bits():
    from mvdfusion_amd.fusion import extract_mesh, integrate_tsdf
    case = T.make_case("v5_s12_g9_up2_rgb")
    c = case.views
    runs = []
    for _ in range(2):
        vol = integrate_tsdf(c.lat.cuda(), c.cams, rgb=case.rgb.cuda(), grid=17, up=c.up)
        mesh = extract_mesh(vol)
        runs.append([vol.tsdf, vol.weight, vol.rgb, vol.cweight, mesh.vertices, mesh.faces, mesh.rgb, mesh.vertex_start, mesh.face_start])
    assert len(runs[0][5]) > 0
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8) if a.is_floating_point() else a, b.view(torch.uint8) if b.is_floating_point() else b)


def test_sphere_end_to_end():
    from mvdfusion_amd.fusion import TriangleMesh, TSDFVolume, extract_mesh, integrate_tsdf
    case, ref, mref = _sphere()
    c = case.views
    G, he = case.G, case.half_extent
    vol = integrate_tsdf(c.lat.cuda(), c.cams, grid=G, half_extent=he)
    mesh = extract_mesh(vol)
    assert isinstance(vol, TSDFVolume) and isinstance(mesh, TriangleMesh) and vol.tsdf.shape == (G, G, G) and vol.rgb is None
    assert vol.trunc == 3 * 2 * he / G and len(mesh) > 0 and mesh.rgb is None
    x, f = mesh.vertices.cpu().double(), mesh.faces.cpu().long()
    assert int(f.max()) < len(x) and mesh.vertex_start.tolist() == [0, len(x)] and mesh.face_start.tolist() == [0, len(f)]
    tri = x[f]
    normal = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert bool(((normal * tri.mean(1)).sum(1) > 0).all())          # every face normal points away from the origin
    # the vertex parity bound of test_mesh_vs_oracle, on the kernel's own volume
    tsdf, weight = vol.tsdf.cpu()[None], vol.weight.cpu()[None]
    o64, o32 = T.march(tsdf, weight, half_extent=he), T.march(tsdf, weight, half_extent=he, dtype=torch.float32)
    _, parity = _vertex_bound(o64, o32)
    radial = float((x.norm(dim=1) - F.SPHERE_R).abs().max())
    oracle = float((mref.vertices.norm(dim=1) - F.SPHERE_R).abs().max())          # discretisation error of the float64 rule on this rig
    print(f"sphere: {len(x)} vertices {len(f)} faces | max | |x| - r | kernel {radial:.6e} float64 oracle {oracle:.6e} parity bound {parity:.2e} | "
          f"observed {float((weight > 0).float().mean()):.3f}")
    assert radial <= oracle + parity, (radial, oracle, parity)
    # carving: an observed voxel farther than trunc + sqrt(3) voxels outside the sphere is free space in every view that observed it
    ax = T.voxel_axes(G, case.center, he, torch.float64)
    zz, yy, xx = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    far = ((xx ** 2 + yy ** 2 + zz ** 2).sqrt() - F.SPHERE_R > vol.trunc + math.sqrt(3.0) * 2 * he / G) & (weight[0] > 0)
    assert int(far.sum()) > 0 and bool((tsdf[0][far] == 1.0).all())


# ------------------------------------------------------------------------------------------------ 4. the model's own call
def test_viewfusion_mesh_round_trip():
    """On the reduced-width model: ViewFusion.mesh == integrate_tsdf + extract_mesh by hand with the decoded image and the model's depth
    map.  The latents are random (0.5 N(0, 1), as the parity cases): what is under test is the plumbing, not a sample."""
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.fusion import TriangleMesh, extract_mesh, integrate_tsdf
    from test_gpu_fusion import _small_vae
    V, S, up, G = 2, 32, 2, 32
    m = build_model(32)
    inp = syn.make_inputs(V, S, seed=2)
    x = (0.5 * torch.randn(V, 5, S, S, generator=torch.Generator().manual_seed(8))).cuda()
    assert not hasattr(m, "vae")
    m.vae = _small_vae()
    try:
        kw = dict(half_extent=1.5, trunc=0.5, fill=(0.0, 1.0, 0.0))
        mesh = m.mesh(x, inp["batch_cameras"], grid=G, up=up, **kw)
        assert isinstance(mesh, TriangleMesh) and mesh.vertices.device == x.device and mesh.faces.device == x.device
        assert len(mesh) > 0 and int(mesh.faces.max()) < len(mesh.vertices) and int(mesh.faces.min()) >= 0
        assert mesh.rgb.shape == mesh.vertices.shape and bool(torch.isfinite(mesh.vertices).all()) and bool(torch.isfinite(mesh.rgb).all())
        img = m.decode(x[:, :4])
        vol = integrate_tsdf(x, inp["batch_cameras"], rgb=img, grid=G, up=up, depth_scale=m.view_attn.depth_scale,
                             depth_shift=m.view_attn.depth_shift, half_extent=kw["half_extent"], trunc=kw["trunc"])
        want = extract_mesh(vol, fill=kw["fill"])
        for k in ("vertices", "faces", "rgb", "vertex_start", "face_start"):
            assert torch.equal(getattr(mesh, k), getattr(want, k)), k
        plain = m.mesh(x, inp["batch_cameras"], grid=G, decode=False, **kw)
        assert plain.rgb is None and torch.equal(plain.vertices, mesh.vertices) and torch.equal(plain.faces, mesh.faces)
    finally:
        del m.vae
