"""Texturing, host side (no GPU): the atlas layout by brute force, the host functions' conventions and refusals, write_obj parsed back,
the float64 oracle of tests/texture_f64.py on scenes with a known answer, and the C ABI of the new entry points."""
import itertools
import struct
import zlib

import pytest
import torch

import texture_f64 as X
from mvdfusion_amd import fusion as F
from mvdfusion_amd.fusion import MeshTexture, TriangleMesh

LAYOUT_T = (1, 2, 3, 8)
LAYOUT_NF = (1, 2, 3, 5, 8, 9, 51)


def _mesh(nf, nv=None, scenes=None):
    """A CPU TriangleMesh of nf faces on 3 nf vertices (one scene, or the face counts `scenes`)."""
    counts = [nf] if scenes is None else list(scenes)
    nf = sum(counts)
    g = torch.Generator().manual_seed(3)
    fs = torch.tensor([0] + list(itertools.accumulate(counts)), dtype=torch.int32)
    return TriangleMesh(vertices=torch.rand(3 * nf, 3, generator=g), faces=torch.arange(3 * nf, dtype=torch.int32).reshape(nf, 3), rgb=None,
                        vertex_start=fs * 3, face_start=fs)


def _texture(mesh, T):
    counts = tuple(int(n) for n in (mesh.face_start[1:] - mesh.face_start[:-1]))
    C, A = F.atlas_layout(max(counts), T, len(counts))
    lead = () if len(counts) == 1 else (len(counts),)
    return MeshTexture(image=torch.zeros(*lead, 3, A, A), views=torch.zeros(*lead, A, A, dtype=torch.uint8),
                       best=torch.full((*lead, A, A), 255, dtype=torch.uint8), texels=T, cells_per_row=C, side=A, faces=counts)


def _lattice(T, sub=4):
    """The points of the closed texel triangle of a chart with legs T on a lattice of 1 / sub texel, in chart coordinates."""
    n = T * sub
    return [(i / sub, j / sub) for i in range(n + 1) for j in range(n + 1 - i)]


def _taps(px, py):
    """The taps of non-zero weight of a bilinear lookup at (px, py) >= 0."""
    x0, y0 = int(px // 1), int(py // 1)
    return {(x0 + dx, y0 + dy) for dx in ((0, 1) if px != x0 else (0,)) for dy in ((0, 1) if py != y0 else (0,))}


@pytest.mark.parametrize("T", LAYOUT_T)
@pytest.mark.parametrize("nf", LAYOUT_NF)
def test_layout_properties_by_brute_force(T, nf):
    mesh = _mesh(nf)
    tex = _texture(mesh, T)
    C, A, K = tex.cells_per_row, tex.side, T + 3
    assert C == X.cells_per_row(nf) and A == C * K and 2 * C * C >= nf and (C == 1 or 2 * (C - 1) ** 2 < nf)
    own = tex.texel_face(mesh)
    assert tuple(own.shape) == (A, A)
    # the map of fusion.py is the closed form of the header, written a second time in texture_f64
    l, _, _ = X.chart_map(T, C)
    assert torch.equal(own, torch.where((l >= 0) & (l < nf), l, torch.full_like(l, -1)))
    # 1. every face owns exactly (T + 1)(T + 2) / 2 + T texels; 2. the sets are disjoint (each texel is counted once, through its cell)
    owned = {f: set() for f in range(nf)}
    for y in range(A):
        for x in range(A):
            o = X.owner(x % K, y % K, T)
            f = -1 if o is None else 2 * ((y // K) * C + x // K) + o[0]
            assert int(own[y, x]) == (f if 0 <= f < nf else -1)
            if 0 <= f < nf:
                owned[f].add((x, y))
    assert all(len(s) == (T + 1) * (T + 2) // 2 + T for s in owned.values())
    assert sum(len(s) for s in owned.values()) == len(set().union(*owned.values()))
    # 3. every tap of non-zero weight of a lookup anywhere in a face's closed texel triangle is its own; 4. every owned texel is such a tap
    corners = tex.corners(mesh)
    for f in range(nf):
        (ax, ay), (bx, by), (cx, cy) = X.corners(f, T, C)
        assert corners[f].tolist() == [[ax, ay], [bx, by], [cx, cy]]
        ex, ey = (bx - ax) // T, (cy - ay) // T          # +1 for the lower half, -1 for the mirrored one
        taps = set()
        for i, j in _lattice(T):
            taps |= _taps(ax + ex * i, ay + ey * j)
        assert taps == owned[f], f


@pytest.mark.parametrize("T", LAYOUT_T)
def test_round_trip_texel_to_face_and_barycentrics_to_texel(T):
    nf = 9
    C = X.cells_per_row(nf)
    l, ci, cj = X.chart_map(T, C)
    y, x = torch.nonzero((l >= 0) & (l < nf), as_tuple=True)
    bb, bc = ci[y, x].double() / T, cj[y, x].double() / T
    ba = (1.0 - bb) - bc
    cor = torch.tensor([X.corners(int(f), T, C) for f in l[y, x]], dtype=torch.float64)              # (K, 3, 2)
    t = (ba[:, None] * cor[:, 0] + bb[:, None] * cor[:, 1]) + bc[:, None] * cor[:, 2]
    assert float((t - torch.stack([x, y], dim=1)).abs().max()) <= 1e-12 * C * (T + 3)
    # ... and through the lookup of the oracle: a texture that holds its own coordinates reads them back at its own barycentrics
    A = C * (T + 3)
    yy, xx = torch.meshgrid(torch.arange(A), torch.arange(A), indexing="ij")
    tex = torch.stack([xx, yy, xx + yy]).float()[None]
    face, bary = l[y, x][None, None], torch.stack([ba, bb, bc]).float()[None, :, None]
    for filt in (X.NEAREST, X.BILINEAR):
        got, _ = X.sample(face, bary, torch.tensor([0, nf]), nf, 1, tex, T, filt, (-1.0, -1.0, -1.0))
        assert float((got[0, 0, 0] - x).abs().max()) <= 1e-5 and float((got[0, 1, 0] - y).abs().max()) <= 1e-5


def test_uv_follows_the_corners_with_v_up():
    mesh = _mesh(0, scenes=(3, 0, 5))
    tex = _texture(mesh, 2)
    uv, cor = tex.uv(mesh), tex.corners(mesh)
    assert tuple(uv.shape) == (8, 3, 2) and float(uv.min()) > 0 and float(uv.max()) < 1
    assert torch.allclose(uv[..., 0] * tex.side - 0.5, cor[..., 0].float(), atol=1e-4)
    assert torch.allclose((1 - uv[..., 1]) * tex.side - 0.5, cor[..., 1].float(), atol=1e-4)
    assert cor[3].tolist() == cor[0].tolist()                      # local face 0 of scene 2 sits where local face 0 of scene 0 sits
    own = tex.texel_face(mesh)
    assert tuple(own.shape) == (3, tex.side, tex.side) and bool((own[1] == -1).all())
    assert sorted(own[2].unique().tolist()) == [-1, 3, 4, 5, 6, 7]
    tex.faces, tex.views = (3, 0, 5), (own >= 0).to(torch.uint8) * torch.tensor([1, 1, 0], dtype=torch.uint8)[:, None, None]
    assert tex.coverage().tolist() == [1.0, 0.0, 0.0]


def test_atlas_side_agrees_with_the_library_and_refuses_what_it_refuses():
    from mvdfusion_amd import hip
    L = hip.lib()
    for nf, T, n in itertools.product((0, 1, 2, 3, 8, 9, 51, 2616, 10 ** 6, 2 ** 31 - 1), (1, 2, 8, 64), (1, 3)):
        try:
            want = F.atlas_layout(nf, T, n)[1]
        except ValueError:
            want = 0
        assert L.mvd_texture_atlas_side(nf, T, n) == want, (nf, T, n)
    assert L.mvd_texture_atlas_side(0, 1, 1) == 4 and L.mvd_texture_atlas_side(2616, 4, 1) == 37 * 7
    assert L.mvd_texture_atlas_side(8, 0, 1) == 0 and L.mvd_texture_atlas_side(8, 65, 1) == 0 and L.mvd_texture_atlas_side(8, 4, 0) == 0
    assert L.mvd_texture_atlas_side(2 * 250 ** 2, 64, 1) == 0                        # 250 * 67 = 16 750 > 16 384
    assert L.mvd_texture_atlas_side(2 * 1000 ** 2, 8, 1) == 11000 and L.mvd_texture_atlas_side(2 * 1000 ** 2, 8, 18) == 0


def test_host_refusals_fire_before_any_device_work():
    from mvdfusion_amd.cameras import Cameras
    cams = lambda n: Cameras(torch.eye(3).repeat(n, 1, 1), torch.tensor([[0.0, 0.0, 2.0]]).repeat(n, 1), torch.ones(n, 2), torch.zeros(n, 2))
    mesh, two = _mesh(4), _mesh(0, scenes=(2, 3))
    rgb = torch.zeros(2, 3, 8, 8)
    bad = [
        (dict(mesh="mesh"), "TriangleMesh"),
        (dict(rgb=torch.zeros(3, 8, 8)), "rgb must be"),
        (dict(rgb=torch.zeros(2, 4, 8, 8)), "3 channels"),
        (dict(rgb=torch.zeros(2, 3, 8, 9)), "square"),
        (dict(rgb=torch.zeros(255, 3, 2, 2), cameras=cams(255)), r"V = 255"),
        (dict(cameras=[cams(2)]), "not a list"),
        (dict(cameras=cams(3)), "cameras"),
        (dict(mesh=two), "scene"),
        (dict(mesh=two, rgb=torch.zeros(2, 2, 3, 8, 8), cameras=[cams(2)]), "list of N = 2"),
        (dict(mesh=two, rgb=torch.zeros(3, 2, 3, 8, 8), cameras=[cams(2)] * 3), r"3 camera set\(s\) for a mesh of 2"),
        (dict(texels=0), "texels"), (dict(texels=65), "texels"), (dict(texels=2.5), "texels"),
        (dict(blend="max"), "blend"), (dict(power=9), "power"), (dict(power=1.5), "power"), (dict(min_cos=1.0), "min_cos"),
        (dict(min_cos=-0.1), "min_cos"), (dict(tolerance=-1.0), "tolerance"), (dict(tolerance=float("inf")), "tolerance"),
        (dict(znear=-1.0), "znear"), (dict(cull=2), "cull"), (dict(fill=(0.5, 0.5)), "fill"), (dict(size=0), "size"),
        (dict(depth=torch.zeros(3, 8, 8)), "depth"), (dict(depth=torch.zeros(2, 8, 9)), "depth"),
    ]
    for kw, match in bad:
        args = dict(mesh=mesh, rgb=rgb, cameras=cams(2))
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            F.bake_texture(**args)
    with pytest.raises(ValueError, match="simplify the mesh or lower texels"):
        F.bake_texture(_mesh(0, scenes=(1,)).__class__(vertices=torch.zeros(3, 3), faces=torch.zeros(0, 3, dtype=torch.int32), rgb=None,
                                                     vertex_start=torch.tensor([0, 3], dtype=torch.int32),
                                                     face_start=torch.tensor([0, 2 * 300 ** 2], dtype=torch.int32)), rgb, cams(2), texels=64)
    tex = _texture(mesh, 2)
    with pytest.raises(ValueError, match="MeshTexture"):
        F.render_mesh(mesh, cams(1), size=8, texture="tex")
    with pytest.raises(ValueError, match="filter"):
        F.render_mesh(mesh, cams(1), size=8, texture=tex, filter="cubic")
    with pytest.raises(ValueError, match=r"baked for 1 scene\(s\), the mesh has 2"):
        F.render_mesh(two, [cams(1)] * 2, size=8, texture=tex)
    with pytest.raises(ValueError, match="RenderedMesh"):
        F.sample_texture("image", mesh, tex)
    with pytest.raises(ValueError, match="takes scene="):
        F.write_obj("unused.obj", two, _texture(two, 2))


def _decode_png(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        chunks.append((tag, body))
        pos += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(chunks[1][1])
    assert len(raw) == h * (1 + 3 * w)
    rows = [raw[y * (1 + 3 * w):(y + 1) * (1 + 3 * w)] for y in range(h)]
    assert all(r[0] == 0 for r in rows)
    return torch.tensor([list(r[1:]) for r in rows], dtype=torch.uint8).reshape(h, w, 3)


@pytest.mark.parametrize("scene", [None, 1])
def test_write_obj_parses_back(tmp_path, scene):
    mesh = _mesh(5) if scene is None else _mesh(0, scenes=(2, 5))
    tex = _texture(mesh, 3)
    g = torch.Generator().manual_seed(5)
    tex.image = torch.rand(*tex.image.shape, generator=g) * 1.4 - 0.2                # (values outside [0, 1] are clipped)
    path = str(tmp_path / "object.obj")
    F.write_obj(path, mesh, tex, scene=scene)
    lines = open(path).read().splitlines()
    kind = lambda k: [l.split()[1:] for l in lines if l.split()[0] == k]
    sub = mesh if scene is None else mesh.scene(scene)
    f0 = 0 if scene is None else int(mesh.face_start[scene])
    assert kind("mtllib") == [["object.obj.mtl"]] and kind("usemtl") == [["object"]]
    v = torch.tensor([[float(t) for t in r] for r in kind("v")])
    assert torch.equal(v, sub.vertices)
    vt = torch.tensor([[float(t) for t in r] for r in kind("vt")])
    assert tuple(vt.shape) == (15, 2) and float(vt.min()) >= 0 and float(vt.max()) <= 1
    assert torch.allclose(vt.reshape(5, 3, 2), tex.uv(mesh)[f0:f0 + 5], atol=1e-7)
    faces = kind("f")
    assert len(faces) == 5
    for k, row in enumerate(faces):
        ids = [tuple(int(t) for t in c.split("/")) for c in row]
        assert [a - 1 for a, _ in ids] == sub.faces[k].tolist() and [t for _, t in ids] == [3 * k + 1, 3 * k + 2, 3 * k + 3]
    mtl = open(path + ".mtl").read().split()
    assert mtl[mtl.index("map_Kd") + 1] == "object.png" and mtl[mtl.index("newmtl") + 1] == "object"
    image = tex.image if scene is None else tex.image[scene]
    want = torch.round(255.0 * image.clamp(0.0, 1.0)).to(torch.uint8).permute(1, 2, 0)
    assert torch.equal(_decode_png(open(str(tmp_path / "object.png"), "rb").read()), want)


# ------------------------------------------------------------------------------------------------ the oracle on scenes with a known answer
@pytest.mark.parametrize("blend", [X.MEAN, X.BEST])
def test_oracle_constant_images_give_a_constant_texture(blend):
    case = X.sphere_case(texels=2, blend=blend)
    colour = torch.tensor([0.3, 0.55, 0.8])
    case.rgb = colour.reshape(1, 3, 1, 1).expand_as(case.rgb).contiguous()
    for dtype in (torch.float64, torch.float32):
        b = X.bake(case, dtype)
        seen = b.owned & (b.views > 0)
        assert 0.4 < float(seen.sum()) / float(b.owned.sum()) < 0.7
        err = (b.texture.double() - colour.double().reshape(1, 3, 1, 1)).abs().amax(1)[seen].max()
        # BEST copies one lookup of four equal taps; the mix of four equal values z is z ((1 - wx) + wx) ((1 - wy) + wy) up to five
        # roundings.  MEAN adds per view one product and one sum in numerator and denominator and one division: (2 V + 2) more.
        ulps = 5 if blend == X.BEST else 5 + 2 * case.V + 2
        assert float(err) <= ulps * torch.finfo(dtype).eps * float(colour.max())
        assert bool((b.best[seen] < case.V).all()) and bool((b.best[b.owned & ~seen] == 255).all())
        assert bool((b.views[~b.owned] == 0).all()) and bool((b.best[~b.owned] == 255).all())
        fill = torch.tensor(X.FILL, dtype=torch.float32).to(dtype).reshape(1, 3, 1, 1).expand_as(b.texture)
        assert torch.equal(b.texture[~b.owned[:, None].expand_as(fill)], fill[~b.owned[:, None].expand_as(fill)])


@pytest.mark.parametrize("blend", [X.MEAN, X.BEST])
def test_oracle_a_hidden_quad_takes_the_colour_of_the_view_that_sees_it(blend):
    case = X.two_quads_case(blend=blend)
    for dtype in (torch.float64, torch.float32):
        b = X.bake(case, dtype)
        l, _, _ = X.chart_map(case.texels, case.C)
        front, rear = (l[None] >= 0) & (l[None] < 2), (l[None] >= 2) & (l[None] < 4)
        assert int(rear.sum()) == 2 * ((case.texels + 1) * (case.texels + 2) // 2 + case.texels)
        assert bool((b.best[rear] == 1).all()) and bool((b.views[rear] == 1).all())
        green = torch.tensor([0.0, 1.0, 0.0], dtype=dtype).reshape(1, 3, 1, 1).expand_as(b.texture)
        m = rear[:, None].expand_as(green)
        assert torch.equal(b.texture[m], green[m])
        # view 1 never reaches the front quad: where that is seen at all it is view 0's (its border projects between pixel centres, on to
        # empty depth pixels: those texels have no view)
        assert bool((b.best[front] != 1).all()) and float((b.best[front] == 0).float().mean()) > 0.4


def test_oracle_reference_numbers_of_the_sphere_case():
    """The figures the parity test rests on: texels = 4, tol = 0.05, min_cos = 0.1 on raster_f64's sphere_cull1."""
    ref = X.reference(X.sphere_case(texels=4))
    owned = int(ref.baked.owned.sum())
    assert owned == 2616 * 19 and int(ref.bad.sum()) <= owned // 1000 and ref.sets_differ == 0
    assert 0 < ref.oracle_err < 1e-5


# ------------------------------------------------------------------------------------------------ the C ABI
TEXTURE_ENTRY_POINTS = {"mvd_texture_atlas_side": 3, "mvd_texture_bake": 27, "mvd_texture_sample": 14}


def test_texture_entry_points_are_declared_and_exported():
    import ctypes
    import os
    import re
    from conftest import ROOT
    from mvdfusion_amd import hip
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    declared = set(re.findall(r"\b(mvd_[a-z0-9_]+)\s*\(", hdr))
    for fmt in ("f16", "bf16"):
        so = ctypes.CDLL(hip.LIB_PATHS[fmt])
        for name, nargs in TEXTURE_ENTRY_POINTS.items():
            assert name in declared, name
            assert name in hip.SIGNATURES and len(hip.SIGNATURES[name][1]) == nargs, name
            assert hasattr(so, name), name
    for macro, value in (("MVD_TEX_MEAN", hip.TEX_MEAN), ("MVD_TEX_BEST", hip.TEX_BEST), ("MVD_TEX_NEAREST", hip.TEX_NEAREST),
                         ("MVD_TEX_BILINEAR", hip.TEX_BILINEAR), ("MVD_TEX_MAX_TEXELS", hip.TEX_MAX_TEXELS),
                         ("MVD_TEX_MAX_SIDE", hip.TEX_MAX_SIDE), ("MVD_TEX_MAX_VIEWS", hip.TEX_MAX_VIEWS)):
        assert re.search(rf"#define {macro} {value}\b", hdr), macro
    from mvdfusion_amd.csrc.build import SOURCES
    assert "texture.hip" in SOURCES


def test_the_library_refuses_bad_arguments_before_any_launch():
    """Every check fires before anything is enqueued, so the refusals can be exercised without a device (host memory stands in)."""
    import ctypes
    from mvdfusion_amd import hip
    L = hip.lib()
    buf = torch.zeros(4096)
    p, i = hip.ptr(buf), hip.ptr(torch.zeros(8, dtype=torch.int32))
    fill = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    good = dict(vertices=p, colors=None, faces=i, vstart=i, fstart=i, cams=p, rgb=p, depth=p, nvert=3, nface=1, nscene=1, V=1, H=8, Pd=8,
                texels=2, A=5, tol=0.05, min_cos=0.1, power=2, cull=1, blend=0, znear=1e-3, fill=fill, texture=p, views=None, best=None)
    bad = [dict(vertices=None), dict(faces=None), dict(vstart=None), dict(fstart=None), dict(cams=None), dict(rgb=None), dict(depth=None),
           dict(fill=None), dict(texture=None), dict(nscene=0), dict(nscene=65536), dict(V=0), dict(V=255), dict(H=0), dict(Pd=0),
           dict(H=32769), dict(texels=0), dict(texels=65), dict(A=6), dict(A=0), dict(A=4), dict(texels=64, A=67 * 245), dict(nscene=9, A=5 * 3276),
           dict(tol=-1.0), dict(tol=float("inf")), dict(tol=float("nan")), dict(min_cos=1.0), dict(min_cos=-0.5), dict(power=-1), dict(power=9),
           dict(cull=2), dict(blend=2), dict(znear=-1.0), dict(nface=2 ** 31), dict(nvert=2 ** 31)]
    for kw in bad:
        a = dict(good)
        a.update(kw)
        assert L.mvd_texture_bake(*a.values(), None) != 0, kw
        assert b"mvd_texture_bake" in L.mvd_last_error(), kw
    bg = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    good = dict(face=i, bary=p, fstart=i, texture=p, nface=1, nscene=1, M=1, P=4, texels=2, A=5, filter=1, background=bg, rgb=p)
    bad = [dict(face=None), dict(bary=None), dict(fstart=None), dict(texture=None), dict(background=None), dict(rgb=None), dict(nscene=0),
           dict(M=0), dict(nscene=256, M=256), dict(P=0), dict(P=46341), dict(texels=0), dict(texels=65), dict(A=7), dict(filter=2),
           dict(filter=-1), dict(nface=2 ** 31)]
    for kw in bad:
        a = dict(good)
        a.update(kw)
        assert L.mvd_texture_sample(*a.values(), None) != 0, kw
        assert b"mvd_texture_sample" in L.mvd_last_error(), kw


def test_oracle_end_to_end_texture_keeps_detail_the_vertices_lose():
    """The design check of tests/test_gpu_texture.py's end-to-end case, in float64 alone: the textured render of the simplified sphere is
    closer to the source views than its vertex-colour render by far more than the factor two the GPU test's inequality needs.
    Float64 chain: mse 0.00146 textured against 0.0781 vertex colours on 7 724 pixels."""
    textured, vertex, pixels = X.e2e_oracle()
    print(f"E2E oracle: mse textured {textured:.5f} vertex {vertex:.5f} pixels {pixels}")
    assert pixels > 5000 and 2.0 * textured < vertex
