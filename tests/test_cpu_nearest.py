"""The nearest-point search without a GPU: the fp32 restatement of tests/nearest_f64.py held to the float64 brute force on every case
(where the figures quoted in tests/test_gpu_nearest.py come from), header, binding and constants, the host side of
fusion.nearest_points and fusion.compare_geometry against a stub library, the metrics on hand-made distances, and fusion.sample_mesh on
CPU tensors."""
import dataclasses
import os
import re

import pytest
import torch

import nearest_f64 as NN
import raster_f64 as R
from mvdfusion_amd import fusion, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -23


# ------------------------------------------------------------------------------------------------ the restatement and the cases
@pytest.mark.parametrize("name", list(NN.CASES))
def test_the_restatement_meets_the_float64_bounds_and_the_cases_reach_what_they_are_for(name):
    ref = NN.refs(name)
    case = ref.case
    ok, w1, w2 = NN.float64_bounds(ref, ref.index, ref.dist2)
    print(f"{name}: nq {case.nq} nt {case.nt} scenes {case.nscene}, winners {int((ref.index >= 0).sum())}, index == float64's "
          f"{float((ref.index == ref.index64).float().mean()):.4f}, dist2 {w1:.2f} x 2^-23 (bound 3), winner {w2:.2f} x 2^-23 (bound 6)")
    assert ok and w1 <= 3 and w2 <= 6
    won = ref.index >= 0
    assert torch.equal(won, ref.index64 >= 0) and bool((ref.dist2[~won] == float("inf")).all()) and bool(torch.isfinite(ref.dist2[won]).all())
    d2 = NN._d2(case.query, case.target, torch.float32)
    ties = ((d2 == ref.dist2[:, None]).sum(1) > 1) & won
    if name == "random":
        assert case.nq % 64 and case.nt % 64 and case.nt % 256
    if name == "tile_edge":
        assert case.nt > 1024 and case.nt % 1024          # more than one LDS tile of the brute kernel, and a ragged last one
    if name == "three_scenes":
        assert not bool(won[:50].any()) and bool(won[50:].all()) and bool((ref.index[50:] >= 1).all())
    if name == "duplicates":
        on = ref.dist2 == 0
        print(f"  on a target {float(on.float().mean()):.3f}, exact ties {float(ties.float().mean()):.3f}")
        assert float(on.float().mean()) > 0.98 and float(ties.float().mean()) > 0.9
        first = torch.where(d2 == ref.dist2[:, None], torch.arange(case.nt)[None], torch.full((1, 1), case.nt)).min(1).values
        assert torch.equal(first, ref.index)              # the lowest index among the ties
    if name == "half_lattice":
        assert bool((ref.dist2 == 3 * 0.0625 ** 2).all()) and bool(((d2 == ref.dist2[:, None]).sum(1) == 16).all())
    if name == "far_and_hollow":
        assert float(case.query.abs().max()) == 10 * 2 * NN.SPHERE_R and float(ref.dist2.sqrt().min()) > 0.5 * NN.SPHERE_R
    if name.startswith("degenerate"):
        ext = case.target.max(0).values - case.target.min(0).values
        assert int((ext == 0).sum()) == {"degenerate_coincident": 3, "degenerate_plane": 1, "degenerate_line": 0}[name]
        if name == "degenerate_line":
            assert int(torch.linalg.matrix_rank(case.target.double() - case.target.double().mean(0), tol=1e-6)) == 1
        assert bool((ref.dist2[:8] == 0).all()) and bool((ref.dist2[8:] > 0).any())
    if name == "nonfinite":
        assert int((~torch.isfinite(case.query).all(1)).sum()) >= 50 and int((~torch.isfinite(case.target).all(1)).sum()) >= 50
        assert not bool(won[~torch.isfinite(case.query).all(1)].any()) and bool(won[torch.isfinite(case.query).all(1)].all())
        assert bool(torch.isfinite(case.target[ref.index[won]]).all())          # a non-finite target is never chosen


# ------------------------------------------------------------------------------------------------ header, binding, constants
def test_the_header_and_the_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define\s+MVD_NN_(\w+)\s+(\d+)", hdr)}
    assert consts == dict(AUTO=hip.NN_AUTO, BRUTE=hip.NN_BRUTE, GRID=hip.NN_GRID, BUILD=hip.NN_BUILD, QUERY=hip.NN_QUERY, ALL=hip.NN_ALL)
    assert hip.NN_ALL == hip.NN_BUILD | hip.NN_QUERY and fusion.NN_METHODS == dict(auto=hip.NN_AUTO, brute=hip.NN_BRUTE, grid=hip.NN_GRID)
    for name, count in (("mvd_nearest_points_scratch", 4), ("mvd_nearest_points", 14), ("mvd_nearest_points_stages", 15)):
        decl = re.search(r"^\w+ " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
        assert decl is not None and name in hip.SIGNATURES
        assert len(hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == count
    src = open(os.path.join(ROOT, "mvdfusion_amd", "csrc", "nearest.hip")).read()
    assert int(re.search(r"kMaxGrid = (\d+);", src).group(1)) == hip.NN_MAX_GRID == 256
    build = open(os.path.join(ROOT, "mvdfusion_amd", "csrc", "build.py")).read()
    assert '"nearest.hip"' in build


# ------------------------------------------------------------------------------------------------ the host side
def _cloud(scene, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = len(scene)
    z = torch.zeros(n, dtype=torch.int64)
    return fusion.PointCloud(xyz=torch.rand(n, 3, generator=g), rgb=None, support=z.to(torch.uint8), scene=torch.tensor(scene, dtype=torch.int64),
                             view=z, pixel=torch.zeros(n, 2, dtype=torch.int64), index=z.to(torch.int32))


@pytest.fixture
def stub(monkeypatch):
    calls = []

    def run(query, query_start, target, target_start, N, method, grid):
        calls.append(dict(query=query, query_start=query_start, target=target, target_start=target_start, N=N, method=method, grid=grid))
        nq = query.shape[0]
        return torch.arange(nq, dtype=torch.int32) % max(int(target.shape[0]), 1), torch.full((nq,), 0.25)

    monkeypatch.setattr(fusion, "_nearest", run)
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("the library was touched"))
    return calls


def test_nearest_points_validates_its_arguments(stub):
    a, b = _cloud([0, 0, 1, 1, 1, 2]), _cloud([0, 2, 2, 2], seed=1)
    mesh = fusion.TriangleMesh(vertices=torch.rand(3, 3), faces=torch.tensor([[0, 1, 2]], dtype=torch.int32), rgb=None,
                               vertex_start=torch.tensor([0, 3], dtype=torch.int32), face_start=torch.tensor([0, 1], dtype=torch.int32))
    bad = [dict(scenes=0), dict(scenes=65536), dict(scenes=2.5), dict(scenes=2),                      # scene id 2 with two scenes
           dict(method="kdtree"), dict(method=1), dict(grid=0), dict(grid=257), dict(grid=2.5), dict(grid=-1),
           dict(query=torch.rand(5, 2)), dict(query=torch.rand(5)), dict(target=torch.rand(3, 4)), dict(query="cloud"),
           dict(query=dataclasses.replace(a, scene=a.scene[:-1])), dict(target=dataclasses.replace(b, xyz=b.xyz[:, :2])),
           dict(query=mesh), dict(target=mesh)]
    for kw in bad:
        args = dict(query=a, target=b, scenes=3)
        args.update(kw)
        with pytest.raises(ValueError):
            fusion.nearest_points(**args)
    with pytest.raises(ValueError, match="sample_mesh"):
        fusion.nearest_points(a, mesh, scenes=3)
    assert not stub                                         # nothing reached the library
    out = fusion.nearest_points(a, b, scenes=3)
    c = stub[-1]
    assert (c["N"], c["method"], c["grid"]) == (3, hip.NN_AUTO, 0)
    assert c["query_start"].tolist() == [0, 2, 5, 6] and c["target_start"].tolist() == [0, 1, 1, 4]
    assert c["query_start"].dtype == c["target_start"].dtype == torch.int32
    assert c["query"].dtype == c["target"].dtype == torch.float32 and c["query"].is_contiguous() and c["target"].is_contiguous()
    assert torch.equal(c["query"], a.xyz) and torch.equal(c["target"], b.xyz)
    assert [f.name for f in dataclasses.fields(out)] == ["index", "dist2"]
    assert out.index.shape == out.dist2.shape == out.dist.shape == out.hit.shape == (6,) and out.index.dtype == torch.int32
    assert out.hit.dtype == torch.bool and bool(out.hit.all()) and torch.equal(out.dist, torch.full((6,), 0.5))
    fusion.nearest_points(a.xyz.double()[:, [2, 0, 1]], b.xyz, method="grid", grid=64)          # bare tensors: one scene; fp64, strided
    c = stub[-1]
    assert (c["N"], c["method"], c["grid"]) == (1, hip.NN_GRID, 64) and c["query_start"].tolist() == [0, 6] and c["target_start"].tolist() == [0, 4]
    assert c["query"].dtype == torch.float32 and c["query"].is_contiguous()
    fusion.nearest_points(a.xyz, torch.zeros(0, 3), scenes=2, method="brute")          # an empty side is a valid call
    c = stub[-1]
    assert c["method"] == hip.NN_BRUTE and c["query_start"].tolist() == [0, 6, 6] and c["target_start"].tolist() == [0, 0, 0]
    samples = fusion.SurfaceSamples(xyz=torch.rand(4, 3), rgb=None, scene=torch.tensor([0, 0, 1, 1]), face=torch.zeros(4, dtype=torch.int32),
                                    bary=torch.zeros(4, 3))
    fusion.nearest_points(samples, a, scenes=3)
    assert stub[-1]["query_start"].tolist() == [0, 2, 4, 4]


def test_compare_geometry_validates_and_reduces(stub):
    a, b = _cloud([0, 0, 1, 1, 1, 2]), _cloud([0, 2, 2, 2], seed=1)
    for kw in (dict(threshold=-1.0), dict(threshold=float("nan")), dict(samples=0), dict(samples=2.5), dict(scenes=2), dict(method="fast")):
        args = dict(a=a, b=b, scenes=3)
        args.update(kw)
        with pytest.raises(ValueError):
            fusion.compare_geometry(**args)
    assert not stub
    d = fusion.compare_geometry(a, b, scenes=3, threshold=0.5, method="brute")
    assert len(stub) == 2 and [c["method"] for c in stub] == [hip.NN_BRUTE] * 2
    assert torch.equal(stub[0]["query"], a.xyz) and torch.equal(stub[0]["target"], b.xyz) and torch.equal(stub[1]["query"], b.xyz)
    assert [f.name for f in dataclasses.fields(d)] == ["a_to_b", "b_to_a", "accuracy", "completeness", "chamfer", "chamfer_sq", "precision", "recall",
                                                       "fscore"]
    assert d.a_to_b.index.shape == (6,) and d.b_to_a.index.shape == (4,)
    for k in ("accuracy", "completeness", "chamfer", "chamfer_sq", "precision", "recall", "fscore"):
        v = getattr(d, k)
        assert v.shape == (3,) and v.dtype == torch.float64 and bool(torch.isnan(v[1])), k          # scene 1 of b is empty
    assert d.accuracy[[0, 2]].tolist() == [0.5, 0.5] and d.chamfer[[0, 2]].tolist() == [1.0, 1.0] and d.chamfer_sq[[0, 2]].tolist() == [0.5, 0.5]
    assert d.fscore[[0, 2]].tolist() == [1.0, 1.0]
    # a mesh goes through sample_mesh first; the default number of samples is the documented one
    v, f = R.icosahedron()
    mesh = fusion.TriangleMesh(vertices=v.float(), faces=f.to(torch.int32), rgb=None, vertex_start=torch.tensor([0, 12], dtype=torch.int32),
                               face_start=torch.tensor([0, 20], dtype=torch.int32))
    d = fusion.compare_geometry(mesh, a.xyz, samples=300)
    assert stub[-2]["query"].shape == (300, 3) and d.a_to_b.index.shape == (300,) and stub[-1]["target"].shape == (300, 3)
    fusion.compare_geometry(a.xyz, mesh)
    assert stub[-1]["query"].shape == (fusion.COMPARE_SAMPLES, 3) and fusion.COMPARE_SAMPLES == 65536
    two = dataclasses.replace(mesh, vertex_start=torch.tensor([0, 12, 12], dtype=torch.int32), face_start=torch.tensor([0, 20, 20], dtype=torch.int32))
    with pytest.raises(ValueError):
        fusion.compare_geometry(two, a.xyz, samples=10)          # two scenes with scenes = 1


def test_the_metrics_on_hand_made_distances():
    a = torch.tensor([0.0, 0.09, 0.16, 1.0, 4.0])          # distances 0, 0.3, 0.4 | 1, 2
    b = torch.tensor([0.25, 0.25, 9.0])                    # 0.5, 0.5 | 3
    m = fusion.geometry_metrics(a, torch.tensor([0, 0, 0, 1, 1]), b, torch.tensor([0, 0, 1]), 3, 0.45)
    f32 = lambda *v: torch.tensor(v, dtype=torch.float32).double()
    acc0, comp0 = float(f32(0.0, 0.09, 0.16).sqrt().sum() / 3), 0.5
    assert m["accuracy"][:2].tolist() == [acc0, 1.5] and m["completeness"][:2].tolist() == [comp0, 3.0]
    assert abs(acc0 - 0.7 / 3) < 1e-7
    assert m["chamfer"][:2].tolist() == [acc0 + comp0, 4.5]
    assert m["chamfer_sq"][:2].tolist() == [float(f32(0.0, 0.09, 0.16).sum() / 3 + 0.25), 2.5 + 9.0]
    assert m["precision"][:2].tolist() == [1.0, 0.0] and m["recall"][:2].tolist() == [0.0, 0.0]
    assert m["fscore"][:2].tolist() == [0.0, 0.0]          # P + R == 0 gives 0 (scene 1), P R == 0 too (scene 0)
    assert all(bool(torch.isnan(v[2])) and v.dtype == torch.float64 and v.shape == (3,) for v in m.values())          # scene 2: both sides empty
    assert set(m) == {"accuracy", "completeness", "chamfer", "chamfer_sq", "precision", "recall", "fscore"}
    m = fusion.geometry_metrics(a, None, b, None, 1, 0.5)          # no scene ids: one scene; the threshold is inclusive
    assert m["precision"].tolist() == [0.6] and m["recall"].tolist() == [2 / 3]
    assert m["fscore"].tolist() == [2 * 0.6 * (2 / 3) / (0.6 + 2 / 3)]
    one_sided = fusion.geometry_metrics(a, None, torch.zeros(0), None, 1, 0.5)
    assert all(bool(torch.isnan(v).all()) for v in one_sided.values())
    again = fusion.geometry_metrics(a, None, b, None, 1, 0.5)
    assert all(torch.equal(m[k], again[k]) for k in m)


# ------------------------------------------------------------------------------------------------ sample_mesh
def _meshes():
    v, f = R.icosahedron()
    ico = fusion.TriangleMesh(vertices=v.float(), faces=f.to(torch.int32), rgb=(v.float() * 0.5 + 0.5),
                              vertex_start=torch.tensor([0, 12], dtype=torch.int32), face_start=torch.tensor([0, 20], dtype=torch.int32))
    sv, sf = R.sphere_mesh(8)
    sph = fusion.TriangleMesh(vertices=sv.float(), faces=sf.to(torch.int32), rgb=None, vertex_start=torch.tensor([0, sv.shape[0]], dtype=torch.int32),
                              face_start=torch.tensor([0, sf.shape[0]], dtype=torch.int32))
    return ico, sph


def _check_samples(mesh, s, n, f0, f1, rows):
    """rows: the samples of one scene, whose faces are [f0, f1)."""
    bary, face = s.bary[rows], s.face[rows].long()
    assert rows.stop - rows.start == n and bool((face >= f0).all()) and bool((face < f1).all()) and s.face.dtype == torch.int32
    assert bool((bary >= 0).all()) and float((bary.double().sum(1) - 1.0).abs().max()) <= 4 * EPS
    tri = mesh.vertices.double()[mesh.faces.long()[face]]
    mix = (bary.double()[:, :, None] * tri).sum(1)
    assert float((s.xyz[rows].double() - mix).abs().max()) <= 3 * EPS * float(mesh.vertices.abs().max())
    if mesh.rgb is not None:
        col = (bary.double()[:, :, None] * mesh.rgb.double()[mesh.faces.long()[face]]).sum(1)
        assert float((s.rgb[rows].double() - col).abs().max()) <= 3 * EPS * float(mesh.rgb.abs().max())
    alltri = mesh.vertices.double()[mesh.faces.long()[f0:f1]]
    area = 0.5 * torch.linalg.cross(alltri[:, 1] - alltri[:, 0], alltri[:, 2] - alltri[:, 0]).norm(dim=1)
    count = torch.bincount(face - f0, minlength=f1 - f0).double()
    assert float((count - n * area / area.sum()).abs().max()) <= 2          # the stratification
    assert bool((face[1:] >= face[:-1]).all())


@pytest.mark.parametrize("n", [1, 257, 5000])
def test_sample_mesh_is_stratified_by_area_and_deterministic(n, tmp_path):
    for mesh in _meshes():
        s = fusion.sample_mesh(mesh, n)
        assert len(s) == n and s.xyz.shape == s.bary.shape == (n, 3) and s.xyz.dtype == s.bary.dtype == torch.float32
        assert s.scene.dtype == torch.int64 and bool((s.scene == 0).all()) and (s.rgb is None) == (mesh.rgb is None)
        _check_samples(mesh, s, n, 0, len(mesh), slice(0, n))
        again = fusion.sample_mesh(mesh, n)
        for k in ("xyz", "scene", "face", "bary"):
            assert torch.equal(getattr(s, k), getattr(again, k)), k
        if n == 5000:          # on the surface: inside the sphere the mesh approximates, never outside the vertices' radius
            r = s.xyz.double().norm(dim=1)
            assert float(r.max()) <= float(mesh.vertices.double().norm(dim=1).max()) * (1 + 4 * EPS) and float(r.min()) > 0.75 * R.SPHERE_R
            # the barycentrics fill the triangle: the R2 sequence folded, every third of the simplex gets its share within 2 %
            share = torch.bincount(s.bary.argmax(1), minlength=3).double() / n
            assert float((share - 1 / 3).abs().max()) < 0.02
    ico, _ = _meshes()
    s = fusion.sample_mesh(ico, 100)
    path = tmp_path / "samples.ply"
    fusion.write_ply(str(path), s)          # a SurfaceSamples saves like a cloud
    raw = path.read_bytes()
    head, body = raw.split(b"end_header\n")
    assert b"element vertex 100" in head and b"property uchar red" in head and b"element face" not in head and len(body) == 100 * 15
    import numpy as np
    rec = np.frombuffer(body, dtype=np.dtype([("xyz", "<f4", (3,)), ("rgb", "u1", (3,))]))
    assert np.array_equal(rec["xyz"], s.xyz.numpy()) and np.array_equal(rec["rgb"], np.rint(s.rgb.clamp(0, 1).numpy() * 255).astype("u1"))


def test_sample_mesh_takes_scenes_one_by_one():
    ico, sph = _meshes()
    nv, nf = ico.vertices.shape[0], len(ico)
    # scene 0: the icosahedron; scene 1: no face; scene 2: the sphere; scene 3: faces of zero area
    flat = torch.tensor([[0, 0, 1], [2, 2, 2]], dtype=torch.int32) + nv + sph.vertices.shape[0]
    mesh = fusion.TriangleMesh(vertices=torch.cat([ico.vertices, sph.vertices, torch.rand(3, 3)]),
                               faces=torch.cat([ico.faces, sph.faces + nv, flat]), rgb=None,
                               vertex_start=torch.tensor([0, nv, nv, nv + sph.vertices.shape[0], nv + sph.vertices.shape[0] + 3], dtype=torch.int32),
                               face_start=torch.tensor([0, nf, nf, nf + len(sph), nf + len(sph) + 2], dtype=torch.int32))
    n = 400
    s = fusion.sample_mesh(mesh, n)
    assert len(s) == 2 * n and s.scene.tolist() == [0] * n + [2] * n
    _check_samples(mesh, s, n, 0, nf, slice(0, n))
    _check_samples(mesh, s, n, nf, nf + len(sph), slice(n, 2 * n))
    alone = fusion.sample_mesh(sph, n)
    assert torch.equal(s.xyz[n:], alone.xyz) and torch.equal(s.face[n:], alone.face + nf) and torch.equal(s.bary[n:], alone.bary)
    empty = fusion.sample_mesh(mesh.scene(1), n)
    assert len(empty) == 0 and empty.xyz.shape == (0, 3) and empty.bary.shape == (0, 3) and empty.face.dtype == torch.int32
    assert len(fusion.sample_mesh(mesh.scene(3), n)) == 0
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            fusion.sample_mesh(sph, bad)
    with pytest.raises(ValueError):
        fusion.sample_mesh(sph.vertices, n)
