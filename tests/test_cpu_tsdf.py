"""Volumetric fusion without a GPU: the exclusion cap of every parity case of tests/test_gpu_tsdf.py, known answers of the marching oracle of
tests/tsdf_f64.py (which the kernels are then held to), and the host side of mvdfusion_amd/fusion.py (argument validation with the launches
stubbed; write_ply of a mesh, and of a cloud byte for byte as before)."""
import functools
import math

import numpy as np
import pytest
import torch

import gridattn_f64 as G
import tsdf_f64 as T
from mvdfusion_amd import fusion
from mvdfusion_amd.cameras import get_camera_slice


@functools.lru_cache(maxsize=None)
def _refs(name):
    case = T.make_case(name)
    return case, T.integrate(case), T.integrate(case, torch.float32)


# ------------------------------------------------------------------------------------------------ 1. the parity cases
@pytest.mark.parametrize("name", list(T.CASES))
def test_parity_cases_respect_the_exclusion_cap(name):
    """... and are worth running: observed and unobserved voxels, hidden voxels, background and silhouette lookups all occur, and the fp32
    oracle agrees with float64 on the counts of every compared voxel (so they CAN be asserted equal)."""
    case, ref, o32 = _refs(name)
    bad, bad_colour, m_z, m_n = T.undecidable(case, ref, o32)          # asserts the cap
    keep = T.compared(bad, case)
    trunc = float(torch.tensor(case.trunc, dtype=torch.float32))
    hidden = ref.fg4 & (ref.sdf < -trunc)
    print(f"{name}: undecidable pairs {float(bad_colour.sum()) / bad.numel():.3%}, m_z {m_z:.1e}, m_n {m_n:.1e}, compared voxels "
          f"{int(keep.sum())}/{keep.numel()}, observed {float((ref.weight > 0).float().mean()):.3f}, hidden pairs {int(hidden.sum())}, "
          f"fp32 oracle tsdf {float((o32.tsdf.double() - ref.tsdf).abs()[keep].max()):.1e}")
    assert torch.equal(o32.weight[keep], ref.weight[keep])
    assert bool((ref.weight > 0).any()) and bool(hidden.any()) and bool((ref.seen & ~ref.fg4).any())
    assert bool((ref.tsdf < 0).any()) and bool((ref.tsdf[ref.weight == 0] == 1).all())
    if case.carve:
        assert bool((ref.tsdf[ref.weight > 0] == 1).any())
    if case.rgb is not None:
        keepc = T.compared(bad_colour, case)
        assert torch.equal(o32.cweight[keepc], ref.cweight[keepc]) and 0 < int((ref.cweight > 0).sum()) < int((ref.weight > 0).sum())


# ------------------------------------------------------------------------------------------------ 2. marching: known answers
@functools.lru_cache(maxsize=None)
def _sphere_mesh():
    return T.march(T.sphere_volume(24, 0.75), half_extent=0.75, dtype=torch.float32)


def test_sphere_mesh_is_closed_oriented_and_near_the_sphere():
    m = _sphere_mesh()
    nv, nf = int(m.vertex_start[-1]), len(m.faces)
    assert nv == len(m.vertices) > 0 and nf == int(m.face_start[-1]) > 0
    boundary, repeated = T.boundary_edges(m.faces)
    assert len(boundary) == 0 and not repeated          # every directed edge occurs once and its reverse once
    f = m.faces.numpy()
    und = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    assert len(np.unique(f)) == nv and nv - len(und) + nf == 2          # a sphere: V - E + F = 2
    x = m.vertices.double()
    tri = x[m.faces]
    normal = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert bool(((normal * tri.mean(1)).sum(1) > 0).all())
    assert bool((m.faces[:, 0] < m.faces[:, 1]).all()) and bool((m.faces[:, 0] < m.faces[:, 2]).all())
    # a vertex lies on a lattice edge whose ends are on either side of the surface, and the distance field is 1-Lipschitz
    assert float((x.norm(dim=1) - T.F.SPHERE_R).abs().max()) <= math.sqrt(3.0) * 2 * 0.75 / 24


def test_no_sign_change_gives_an_empty_mesh():
    for vol in (torch.full((2, 5, 5, 5), 0.25), -torch.ones(1, 5, 5, 5), torch.zeros(1, 4, 4, 4)):          # zero is outside
        m = T.march(vol)
        assert len(m.vertices) == 0 and len(m.faces) == 0
        assert m.vertex_start.tolist() == [0] * (vol.shape[0] + 1) and m.face_start.tolist() == [0] * (vol.shape[0] + 1)


def test_unobserved_block_opens_the_mesh_only_there():
    Gv, he = 24, 0.75
    vol = T.sphere_volume(Gv, he)
    weight = torch.ones(1, Gv, Gv, Gv, dtype=torch.uint8)
    weight[0, 10:15, 3:9, 8:16] = 0          # a block across the surface
    m = T.march(vol, weight, half_extent=he)
    closed = _sphere_mesh()
    assert 0 < len(m.faces) < len(closed.faces)
    boundary, repeated = T.boundary_edges(m.faces)
    assert len(boundary) > 0 and not repeated
    ax = T.voxel_axes(Gv, (0.0, 0.0, 0.0), he, torch.float64)
    k, j, i = torch.nonzero(weight[0] == 0, as_tuple=True)
    holes = torch.stack([ax[0][i], ax[1][j], ax[2][k]], dim=1)
    # the tetrahedron missing behind a boundary edge has an unobserved corner, in the same cell as both ends of the edge
    ends = m.vertices[torch.from_numpy(boundary)]
    far = torch.maximum(torch.cdist(ends[:, 0], holes), torch.cdist(ends[:, 1], holes)).min(1).values
    assert float(far.max()) <= math.sqrt(3.0) * 2 * he / Gv + 1e-9


def test_marching_oracle_colours_and_scenes():
    """Two scenes, the first all outside: ids are global, the empty scene owns nothing; colours follow the availability rule."""
    vol = torch.cat([torch.ones(1, 6, 6, 6), T.smooth_volume(6, 7)])
    color = torch.rand(2, 6, 6, 6, 3, generator=torch.Generator().manual_seed(2))
    cweight = (torch.rand(2, 6, 6, 6, generator=torch.Generator().manual_seed(3)) < 0.5).to(torch.uint8)
    m = T.march(vol, None, color, cweight, fill=(0.1, 0.2, 0.3))
    assert m.vertex_start[1] == 0 and m.face_start[1] == 0 and m.vertex_start[2] == len(m.vertices) > 0
    one = T.march(vol[1:], None, color[1:], cweight[1:], fill=(0.1, 0.2, 0.3))
    assert torch.equal(one.faces, m.faces) and torch.equal(one.vertices, m.vertices) and torch.equal(one.colors, m.colors)
    assert bool((m.colors == torch.tensor([0.1, 0.2, 0.3]).double()).all(1).any())          # (fill arrives as C floats)
    assert float(m.colors.min()) >= 0 and float(m.colors.max()) <= 1


# ------------------------------------------------------------------------------------------------ 3. host
def _stub(monkeypatch):
    calls = []

    def integrate(lat, rgb, cams, N, V, S, up, Gv, center, half_extent, trunc, carve, depth_scale, depth_shift, lo, hi):
        calls.append(dict(lat=lat, rgb=rgb, cams=cams, N=N, V=V, S=S, up=up, G=Gv, center=center, half_extent=half_extent, trunc=trunc,
                          carve=carve, depth_scale=depth_scale, depth_shift=depth_shift, lo=lo, hi=hi))
        u8 = torch.ones(N, Gv, Gv, Gv, dtype=torch.uint8)
        return torch.zeros(N, Gv, Gv, Gv), u8, None if rgb is None else torch.zeros(N, Gv, Gv, Gv, 3), None if rgb is None else u8

    def march(tsdf, weight, color, cweight, N, Gv, center, half_extent, fill):
        calls.append(dict(tsdf=tsdf, weight=weight, color=color, cweight=cweight, N=N, G=Gv, center=center, half_extent=half_extent, fill=fill))
        m = T.march(tsdf, weight, color, cweight, center, half_extent, fill, dtype=torch.float32)
        return m.vertices, m.colors, m.faces.int(), m.vertex_start.int(), m.face_start.int()

    monkeypatch.setattr(fusion, "_integrate", integrate)
    monkeypatch.setattr(fusion, "_march", march)
    return calls


def test_integrate_tsdf_validates_its_arguments(monkeypatch):
    calls = _stub(monkeypatch)
    V, S = 3, 8
    cams = G.make_rig(V, True)[0]
    lat = torch.zeros(V, 5, S, S)
    bad = [
        dict(latents=lat[:, :4]), dict(latents=lat[0]), dict(latents=lat[:, :, :, :7]), dict(cameras=[cams]),
        dict(cameras=get_camera_slice(cams, [0, 1])), dict(up=0), dict(up=1.5), dict(foreground=(0.5, 0.5)),
        dict(rgb=torch.zeros(V, 3, 4, 4)), dict(rgb=torch.zeros(V, 3, 16, 16), up=4), dict(rgb=torch.zeros(V, 4, 16, 16)),
        dict(latents=lat[None], cameras=cams), dict(latents=lat[None].expand(2, -1, -1, -1, -1), cameras=[cams]),
        dict(latents=torch.zeros(256, 5, 2, 2), cameras=get_camera_slice(cams, [0] * 256)),
        dict(grid=1), dict(grid=257), dict(grid=16.5), dict(half_extent=0.0), dict(half_extent=-1.0), dict(half_extent=float("nan")),
        dict(trunc=0.0), dict(trunc=-0.1), dict(trunc=float("nan")), dict(center=(0.0, 0.0)),
        dict(latents=lat[None].expand(19, -1, -1, -1, -1), cameras=[cams] * 19, grid=256),          # 7 * 19 * 256^3 >= 2^31
    ]
    for kw in bad:
        args = dict(latents=lat, cameras=cams)
        args.update(kw)
        with pytest.raises(ValueError):
            fusion.integrate_tsdf(**args)
    assert not calls                              # nothing reached the library
    vol = fusion.integrate_tsdf(lat, cams)        # the defaults, as documented
    c = calls[-1]
    assert (c["N"], c["V"], c["S"], c["up"], c["G"]) == (1, V, S, 1, 128) and c["rgb"] is None and c["cams"].shape == (V, 20)
    assert (c["lo"], c["hi"], c["carve"], c["center"], c["half_extent"]) == (0.02, 0.98, True, (0.0, 0.0, 0.0), 0.75)
    assert (c["depth_scale"], c["depth_shift"]) == (2.0, 0.5) and c["trunc"] == 3 * 2 * 0.75 / 128
    assert vol.tsdf.shape == (128, 128, 128) and vol.weight.shape == (128, 128, 128) and vol.rgb is None and vol.cweight is None
    assert (vol.center, vol.half_extent, vol.trunc) == ((0.0, 0.0, 0.0), 0.75, c["trunc"])
    # a list of scenes keeps its leading dimension; the image is area-resized to P
    rgb = torch.rand(2, V, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    vol = fusion.integrate_tsdf(lat[None].expand(2, -1, -1, -1, -1), [cams, cams], rgb=rgb, up=2, grid=4, half_extent=0.5, carve=False)
    c = calls[-1]
    assert vol.tsdf.shape == (2, 4, 4, 4) and vol.rgb.shape == (2, 4, 4, 4, 3) and c["trunc"] == 3 * 2 * 0.5 / 4 and c["carve"] is False
    assert torch.equal(c["rgb"], torch.nn.functional.interpolate(rgb.reshape(2 * V, 3, 32, 32), size=(16, 16), mode="area"))


def test_extract_mesh_validates_its_arguments(monkeypatch):
    calls = _stub(monkeypatch)
    sphere = T.sphere_volume(8)
    ones = torch.ones(8, 8, 8, dtype=torch.uint8)
    vol = lambda **kw: fusion.TSDFVolume(**{**dict(tsdf=sphere[0], weight=ones, rgb=None, cweight=None, center=(0.0, 0.0, 0.0),
                                                   half_extent=0.75, trunc=0.1), **kw})
    for volume, kw in ((None, {}), ([1, 2], {}), (torch.zeros(8, 8), {}), (torch.zeros(2, 2, 8, 8, 8), {}), (torch.zeros(8, 8, 7), {}),
                       (torch.zeros(1, 1, 1), {}), (torch.zeros(0, 8, 8, 8), {}), (torch.empty(19, 256, 256, 256, device="meta"), {}),
                       (sphere, dict(fill=(0.5, 0.5))), (vol(weight=ones[:4]), {}), (vol(rgb=torch.zeros(8, 8, 8, 3)), {}),
                       (vol(rgb=torch.zeros(8, 8, 8), cweight=ones), {}), (vol(rgb=torch.zeros(8, 8, 8, 3), cweight=ones[:4]), {}),
                       (vol(half_extent=0.0), {}), (vol(center=(0.0,)), {})):
        with pytest.raises(ValueError):
            fusion.extract_mesh(volume, **kw)
    assert not calls
    mesh = fusion.extract_mesh(sphere[0])                       # a bare (G, G, G) tensor: all observed, no colour, the default box
    c = calls[-1]
    assert c["weight"] is None and c["color"] is None and (c["N"], c["G"], c["center"], c["half_extent"]) == (1, 8, (0.0, 0.0, 0.0), 0.75)
    assert c["fill"] == (0.5, 0.5, 0.5) and c["tsdf"].shape == (1, 8, 8, 8)
    assert len(mesh) == len(mesh.faces) > 0 and mesh.rgb is None and int(mesh.faces.max()) < len(mesh.vertices)
    # two scenes: scene(s) is the sub-mesh with rebased faces
    two = fusion.extract_mesh(torch.cat([T.smooth_volume(8, 1), sphere]))
    a, b = two.scene(0), two.scene(1)
    assert len(a) + len(b) == len(two) and len(a.vertices) + len(b.vertices) == len(two.vertices) and len(a) > 0
    assert torch.equal(b.vertices, mesh.vertices) and torch.equal(b.faces, mesh.faces) and int(a.faces.max()) < len(a.vertices)
    assert b.vertex_start.tolist() == [0, len(mesh.vertices)] and b.face_start.tolist() == [0, len(mesh)]
    with pytest.raises(ValueError):
        two.scene(2)
    coloured = fusion.extract_mesh(vol(rgb=torch.rand(8, 8, 8, 3), cweight=ones), fill=(0.0, 1.0, 0.0))
    assert coloured.rgb.shape == coloured.vertices.shape and calls[-1]["fill"] == (0.0, 1.0, 0.0) and calls[-1]["weight"].shape == (1, 8, 8, 8)


@pytest.mark.parametrize("colour", [True, False])
def test_write_ply_of_a_mesh_round_trip(tmp_path, colour):
    m = T.march(T.sphere_volume(6), dtype=torch.float32)
    rgb = torch.rand(len(m.vertices), 3, generator=torch.Generator().manual_seed(4)) if colour else None
    mesh = fusion.TriangleMesh(vertices=m.vertices, faces=m.faces.int(), rgb=rgb, vertex_start=m.vertex_start.int(), face_start=m.face_start.int())
    path = tmp_path / "mesh.ply"
    fusion.write_ply(str(path), mesh)
    raw = path.read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii").splitlines()
    nv, nf = len(mesh.vertices), len(mesh)
    assert header[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {nv}"]
    assert header[-3:] == [f"element face {nf}", "property list uchar int vertex_indices", "end_header"]
    props = [tuple(line.split()[1:]) for line in header[3:-3]]
    assert props == [("float", "x"), ("float", "y"), ("float", "z")] + ([("uchar", "red"), ("uchar", "green"), ("uchar", "blue")] if colour else [])
    dt = np.dtype([(k, {"float": "<f4", "uchar": "u1"}[t]) for t, k in props])
    v = np.frombuffer(raw[end:end + nv * dt.itemsize], dtype=dt)
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), mesh.vertices.numpy())
    if colour:
        assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], 1), np.rint(rgb.numpy() * 255.0).astype(np.uint8))
    f = np.frombuffer(raw[end + nv * dt.itemsize:], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    assert f.shape == (nf,) and bool((f["n"] == 3).all()) and np.array_equal(f["v"], mesh.faces.numpy())


@pytest.mark.parametrize("colour", [True, False])
def test_write_ply_of_a_cloud_is_unchanged(tmp_path, colour):
    """Byte for byte the file the function wrote before it knew meshes: the layout is spelled out here."""
    g = torch.Generator().manual_seed(3)
    n = 11
    rgb = torch.rand(n, 3, generator=g) if colour else None
    cloud = fusion.PointCloud(xyz=torch.randn(n, 3, generator=g), rgb=rgb, support=torch.ones(n, dtype=torch.uint8),
                              scene=torch.zeros(n, dtype=torch.long), view=torch.zeros(n, dtype=torch.long),
                              pixel=torch.zeros(n, 2, dtype=torch.long), index=torch.arange(n, dtype=torch.int32))
    path = tmp_path / "cloud.ply"
    fusion.write_ply(str(path), cloud)
    want = f"ply\nformat binary_little_endian 1.0\nelement vertex {n}\nproperty float x\nproperty float y\nproperty float z\n"
    if colour:
        want += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    want = (want + "end_header\n").encode("ascii")
    for r in range(n):
        want += cloud.xyz[r].numpy().astype("<f4").tobytes()
        if colour:
            want += np.rint(np.clip(rgb[r].numpy(), 0.0, 1.0) * 255.0).astype("u1").tobytes()
    assert path.read_bytes() == want
