"""The neighbourhood entries without a GPU: the restatements of tests/knn_f64.py held to what they are for (where the figures quoted in
tests/test_gpu_knn.py come from), header, binding and constants, the host side of fusion.knn_points and fusion.estimate_normals
against stub enqueues, fusion.sample_normals on CPU tensors and fusion.write_ply with normals."""
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import knn_f64 as K
import nearest_f64 as NN
import raster_f64 as R
from mvdfusion_amd import fusion, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the k-nearest restatement and its cases
@pytest.mark.parametrize("name", K.CASES)
def test_the_knn_restatement_orders_by_distance_then_row_and_the_cases_reach_what_they_are_for(name):
    case = K.make_case(name)
    index, dist2 = K.refs(name)
    assert index.shape == dist2.shape == (case.nq, K.MAX_K) and dist2.dtype == np.float32
    filled = index >= 0
    assert np.array_equal(filled, dist2 < np.inf) and (filled[:, 1:] <= filled[:, :-1]).all()          # the empty slots are behind
    both = filled[:, 1:]
    d_up = dist2[:, 1:] > dist2[:, :-1]
    tie = (dist2[:, 1:] == dist2[:, :-1]) & (index[:, 1:] > index[:, :-1])
    assert ((d_up | tie) | ~both).all()                                                                # strictly ascending in (d2, j)
    if name in NN.CASES:          # column 0 is the nearest-point restatement, bit for bit
        one = NN.refs(name)
        assert np.array_equal(index[:, 0], one.index.numpy()) and np.array_equal(dist2[:, 0].view(np.int32), one.dist2.numpy().view(np.int32))
    # against float64: the k-th distance is within the five roundings of the rule (3 * 2^-23, nearest_f64.float64_bounds) of float64's k-th
    i64, d64 = K.knn(case, K.MAX_K, dtype=np.float64)
    with np.errstate(invalid="ignore"):          # (inf - inf in the empty slots, which `filled` leaves out)
        rel = np.abs(dist2.astype(np.float64) - d64)[filled] / np.maximum(d64[filled], 1e-300)
    worst = float(rel[d64[filled] > 0].max()) / 2.0 ** -23 if (d64[filled] > 0).any() else 0.0
    print(f"{name}: nq {case.nq} nt {case.nt} scenes {case.nscene}, filled {float(filled.mean()):.3f}, index == float64's "
          f"{float((index == i64).mean()):.4f}, dist2 {worst:.2f} x 2^-23 (bound 3)")
    assert np.array_equal(filled, i64 >= 0) and worst <= 3
    count = filled.sum(1)
    if name == "random":
        assert case.nq % 64 and case.nt % 64 and case.nt % 256
    if name == "duplicates":          # several j at d2 = 0: the tie rule decides the order
        zeros = (dist2 == 0).sum(1)
        print(f"  rows with at least two targets at d2 = 0: {float((zeros >= 2).mean()):.3f}, most {int(zeros.max())}")
        assert float((zeros >= 2).mean()) > 0.9 and zeros.max() >= 8
    if name == "half_lattice":
        assert (dist2[:, :16] == np.float32(3 * 0.0625 ** 2)).all() and (dist2[:, 16] > dist2[:, 15]).all()
    if name == "three_scenes":
        assert (count[:50] == 0).all() and (count[50:] == 32).all()
    if name == "nonfinite":
        bad = ~np.isfinite(case.query).all(1)
        assert (count[bad] == 0).all() and (count[~bad] == 32).all() and np.isfinite(case.target[index[filled]]).all()
    if name == "sphere_self":
        assert case.query is case.target and np.array_equal(index[:, 0], np.arange(case.nq)) and (dist2[:, 0] == 0).all() and case.nq % 64
    if name == "four_scenes":
        assert np.diff(case.query_start).tolist() == [700, 2, 0, 1301] and (count[700:702] == 2).all() and (count[:700] == 32).all()
        for s in (0, 1, 3):       # a scene alone has the batch's lists
            alone, t0 = K.scene_case(case, s)
            i, d = K.knn(alone, K.MAX_K)
            q0, q1 = int(case.query_start[s]), int(case.query_start[s + 1])
            assert np.array_equal(np.where(i >= 0, i + t0, -1), index[q0:q1]) and np.array_equal(d, dist2[q0:q1])
    if name == "few_targets":
        assert (count[:300] == 5).all() and (count[300:] == 32).all() and (index[:300] < 5).all() and (index[300:, 0] >= 5).all()
    if name == "far_and_hollow":
        assert float(np.abs(case.query).max()) == 10 * 2 * NN.SPHERE_R


# ------------------------------------------------------------------------------------------------ the normal restatement and its cases
@pytest.mark.parametrize("name", list(K.NORMAL_CASES))
def test_the_normal_cases_stay_clear_of_the_floor_and_of_the_rank_band(name):
    ref = K.normal_refs(name)
    case = ref.case
    n, k = case.index.shape
    enough = ref.m >= 3
    with np.errstate(all="ignore"):
        rank = np.where(enough & (ref.lam[:, 2] > 0), ref.lam[:, 1] / ref.lam[:, 2], 0.0)
    # no point between "exactly degenerate" and "clearly spanning a plane": oracle and kernel cannot disagree about valid
    assert not ((rank > 2.0 ** -40) & (rank <= 2.0 ** -20)).any()
    below = ref.valid & ~ref.compared
    share = float(below.sum()) / max(int(ref.valid.sum()), 1)
    print(f"{name}: points {n} k {k} valid {int(ref.valid.sum())}, below the gap floor {share:.4f} (cap {K.GAP_CAP}), largest bound "
          f"{float(K.normal_bound(ref)[ref.compared].max()):.3e}")
    assert share <= K.GAP_CAP and ref.compared.any()
    unit = np.linalg.norm(ref.normal[ref.valid], axis=1)
    assert np.abs(unit - 1).max() <= 16 * 2.0 ** -53 and not ref.normal[~ref.valid].any() and np.isnan(ref.variation[~ref.valid]).all()
    assert (ref.variation[ref.valid] >= 0).all() and (ref.variation[ref.valid] <= 1 / 3 + 1e-12).all()
    if case.truth is not None:
        angle = K.angle_to(ref.normal[ref.compared], case.truth[ref.compared])
        print(f"  angle to the analytic normal: largest {float(angle.max()):.6f} rad, mean {float(angle.mean()):.6f} rad")
        assert angle.max() < 0.2
    if name == "lattice_plane":
        assert ref.valid.all() and (ref.normal == [0.0, 0.0, 1.0]).all() and (ref.variation == 0).all()
    if name == "odd_rows":
        assert ref.valid.tolist() == [False] * 5 + [True] * 3 and ref.m.tolist() == [6, 6, 6, 2, 2, 3, 6, 4]
        assert ref.normal[5].tolist() == [0.0, 0.0, 1.0] and np.abs(ref.normal[7] - 3 ** -0.5).max() < 1e-15
    if name in ("sphere", "ellipsoid", "uniform"):
        assert ref.valid.all() and n % 64 and np.array_equal(case.index[:, 0], np.arange(n))          # every point leads its own list


def test_the_sign_rule_of_the_oracle():
    v = np.array([[0.1, -0.9, 0.2], [-0.5, 0.5, 0.1], [0.5, -0.5, 0.1], [0.0, 0.0, -1.0], [-0.6, 0.0, 0.6]])
    assert K.sign_rule(v).tolist() == [[-0.1, 0.9, -0.2], [0.5, -0.5, -0.1], [0.5, -0.5, 0.1], [0.0, 0.0, 1.0], [0.6, 0.0, -0.6]]


# ------------------------------------------------------------------------------------------------ header, binding, constants
def test_the_header_and_the_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define\s+MVD_(KNN_\w+|NORMALS_\w+)\s+(\d+)", hdr)}
    assert consts == dict(KNN_MAX_K=hip.KNN_MAX_K, NORMALS_MAX_K=hip.NORMALS_MAX_K, NORMALS_SWEEPS=hip.NORMALS_SWEEPS) and hip.KNN_MAX_K == K.MAX_K == 32
    for name, count in (("mvd_knn_points", 15), ("mvd_knn_points_stages", 16), ("mvd_point_normals", 10)):
        decl = re.search(r"^\w+ " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
        assert decl is not None and name in hip.SIGNATURES
        assert len(hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == count
    build = open(os.path.join(ROOT, "mvdfusion_amd", "csrc", "build.py")).read()
    assert '"normals.hip"' in build and '"nearest.hip"' in build
    # one copy of the grid build: the k-nearest search lives beside the nearest-point search and launches its kernels
    src = open(os.path.join(ROOT, "mvdfusion_amd", "csrc", "nearest.hip")).read()
    assert src.count("void box_kernel(") == 1 and src.count("void cell_kernel(") == 1 and src.count("nn_build(fn, a, p, st)") == 2
    assert "mvd_knn_points_stages(" in src and max(K.KS) == hip.KNN_MAX_K
    others = [f for f in os.listdir(os.path.join(ROOT, "mvdfusion_amd", "csrc")) if f.endswith((".hip", ".hpp")) and f != "nearest.hip"]
    assert not any("box_kernel" in open(os.path.join(ROOT, "mvdfusion_amd", "csrc", f)).read() for f in others)


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

    def knn(query, query_start, target, target_start, N, k, method, grid):
        calls.append(dict(fn="knn", query=query, query_start=query_start, target=target, target_start=target_start, N=N, k=k, method=method, grid=grid))
        nq = query.shape[0]
        index = (torch.arange(nq, dtype=torch.int32)[:, None] + torch.arange(k, dtype=torch.int32)[None]) % max(int(target.shape[0]), 1)
        index[:, k - 1] = -1
        return index, torch.where(index >= 0, 0.25, float("inf")).float()

    def normals(target, index, points, toward):
        calls.append(dict(fn="normals", target=target, index=index, points=points, toward=toward))
        n = index.shape[0]
        variation = torch.full((n,), 0.125)
        variation[0] = float("nan")
        return torch.zeros(n, 3), variation

    monkeypatch.setattr(fusion, "_knn", knn)
    monkeypatch.setattr(fusion, "_normals", normals)
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("the library was touched"))
    return calls


def test_knn_points_validates_its_arguments(stub):
    a, b = _cloud([0, 0, 1, 1, 1, 2]), _cloud([0, 2, 2, 2], seed=1)
    mesh = fusion.TriangleMesh(vertices=torch.rand(3, 3), faces=torch.tensor([[0, 1, 2]], dtype=torch.int32), rgb=None,
                               vertex_start=torch.tensor([0, 3], dtype=torch.int32), face_start=torch.tensor([0, 1], dtype=torch.int32))
    bad = [dict(k=0), dict(k=33), dict(k=2.5), dict(k=True), dict(k=-1), dict(scenes=0), dict(scenes=65536), dict(scenes=2), dict(method="kdtree"),
           dict(grid=0), dict(grid=257), dict(query=torch.rand(5, 2)), dict(target=torch.rand(3, 4)), dict(query="cloud"), dict(query=mesh),
           dict(target=mesh), dict(query=dataclasses.replace(a, scene=a.scene[:-1]))]
    for kw in bad:
        args = dict(query=a, target=b, k=4, scenes=3)
        args.update(kw)
        with pytest.raises(ValueError):
            fusion.knn_points(**args)
    with pytest.raises(ValueError, match=r"k = 33: an integer in \[1, 32\]"):
        fusion.knn_points(a, b, 33, scenes=3)
    with pytest.raises(ValueError, match="sample_mesh"):
        fusion.knn_points(a, mesh, 4, scenes=3)
    assert not stub                                         # nothing reached the library
    out = fusion.knn_points(a, b, 4, scenes=3)
    c = stub[-1]
    assert (c["N"], c["k"], c["method"], c["grid"]) == (3, 4, hip.NN_AUTO, 0)
    assert c["query_start"].tolist() == [0, 2, 5, 6] and c["target_start"].tolist() == [0, 1, 1, 4] and c["query_start"].dtype == torch.int32
    assert torch.equal(c["query"], a.xyz) and torch.equal(c["target"], b.xyz) and c["query"].is_contiguous()
    assert isinstance(out, fusion.NeighbourPoints) and [f.name for f in dataclasses.fields(out)] == ["index", "dist2"]
    assert out.index.shape == out.dist2.shape == out.dist.shape == out.hit.shape == (6, 4) and out.count.tolist() == [3] * 6
    assert torch.equal(out.dist[:, 0], torch.full((6,), 0.5)) and bool(torch.isposinf(out.dist[:, 3]).all()) and out.hit.dtype == torch.bool
    fusion.knn_points(a.xyz.double()[:, [2, 0, 1]], b.xyz, 32, method="grid", grid=64)          # bare tensors: one scene; fp64, strided
    c = stub[-1]
    assert (c["N"], c["k"], c["method"], c["grid"]) == (1, 32, hip.NN_GRID, 64) and c["query"].dtype == torch.float32 and c["query"].is_contiguous()
    assert "no exclude flag" in fusion.knn_points.__doc__ and "STAYS" in fusion.knn_points.__doc__


def test_estimate_normals_validates_and_passes_on(stub):
    a = _cloud([0, 0, 0, 1, 1, 1, 2])
    lists = fusion.NeighbourPoints(index=torch.zeros(7, 5, dtype=torch.int32), dist2=torch.zeros(7, 5))
    bad = [dict(k=2), dict(k=33), dict(k=2.5), dict(scenes=2), dict(method="fast"), dict(grid=0), dict(toward=torch.zeros(2, 3)),
           dict(toward=torch.zeros(3, 2)), dict(toward=[0, 0, 0]), dict(neighbours=(lists.index, lists.dist2)),
           dict(neighbours=fusion.NeighbourPoints(index=lists.index[:6], dist2=lists.dist2[:6])),
           dict(neighbours=fusion.NeighbourPoints(index=lists.index.long(), dist2=lists.dist2)),
           dict(neighbours=fusion.NearestPoints(index=lists.index[:, 0], dist2=lists.dist2[:, 0]))]
    for kw in bad:
        args = dict(points=a, scenes=3)
        args.update(kw)
        with pytest.raises(ValueError):
            fusion.estimate_normals(**args)
    assert not stub
    out = fusion.estimate_normals(a, scenes=3)
    search, call = stub[-2], stub[-1]
    assert (search["fn"], search["k"], search["N"], search["method"]) == ("knn", fusion.NORMALS_K, 3, hip.NN_AUTO) and fusion.NORMALS_K == 16
    assert search["query"] is search["target"] and search["query_start"].tolist() == [0, 3, 6, 7]          # the cloud against itself
    assert call["fn"] == "normals" and call["toward"] is None and call["index"].shape == (7, 16) and torch.equal(call["target"], a.xyz)
    assert [f.name for f in dataclasses.fields(out)] == ["normal", "variation", "valid", "neighbours"]
    assert out.valid.tolist() == [False] + [True] * 6 and out.neighbours.index.shape == (7, 16)
    eyes = torch.tensor([[1.0, 0, 0], [0, 2.0, 0], [0, 0, 3.0]])
    fusion.estimate_normals(a, scenes=3, toward=eyes, neighbours=lists)
    assert len(stub) == 3 and stub[-1]["index"].shape == (7, 5)                                            # no search: the lists are reused
    assert torch.equal(stub[-1]["toward"], eyes[a.scene]) and torch.equal(stub[-1]["points"], a.xyz)       # a viewpoint per scene
    per_point = torch.rand(7, 3)
    fusion.estimate_normals(a.xyz, toward=per_point, k=8)
    assert torch.equal(stub[-1]["toward"], per_point) and stub[-2]["k"] == 8 and stub[-2]["N"] == 1
    fusion.estimate_normals(a.xyz, toward=torch.tensor([[0.0, 0.0, 9.0]]), k=3)                             # one scene, one viewpoint
    assert stub[-1]["toward"].shape == (7, 3) and bool((stub[-1]["toward"] == torch.tensor([0.0, 0.0, 9.0])).all())
    assert "nobody has tuned" in fusion.estimate_normals.__doc__


# ------------------------------------------------------------------------------------------------ sample_normals, write_ply
def test_sample_normals_against_the_float64_cross_product():
    sv, sf = R.sphere_mesh(8)
    flat = torch.tensor([[0, 0, 1], [2, 2, 2]], dtype=torch.int32)
    mesh = fusion.TriangleMesh(vertices=sv.float(), faces=torch.cat([sf.to(torch.int32), flat]), rgb=None,
                               vertex_start=torch.tensor([0, sv.shape[0]], dtype=torch.int32),
                               face_start=torch.tensor([0, sf.shape[0] + 2], dtype=torch.int32))
    samples = fusion.sample_mesh(mesh, 2000)
    got = fusion.sample_normals(mesh, samples)
    assert got.shape == (2000, 3) and got.dtype == torch.float32
    tri = sv.float().double()[sf.long()[samples.face.long()]]
    want = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    want = want / want.norm(dim=1, keepdim=True)
    assert float((got.double() - want).abs().max()) <= 2.0 ** -24                  # one rounding to fp32 of a component of magnitude <= 1
    assert float((got.double() * samples.xyz.double()).sum(1).min()) > 0           # this sphere winds outward
    # a sample on a face of zero area gets the zero normal
    on_flat = dataclasses.replace(samples, face=torch.full_like(samples.face, sf.shape[0]))
    assert not bool(fusion.sample_normals(mesh, on_flat).any())
    for bad in (dict(mesh=sv, samples=samples), dict(mesh=mesh, samples=samples.xyz),
                dict(mesh=mesh, samples=dataclasses.replace(samples, face=samples.face + 10 ** 6))):
        with pytest.raises(ValueError):
            fusion.sample_normals(**bad)


def test_write_ply_with_normals(tmp_path):
    cloud = dataclasses.replace(_cloud([0] * 9), rgb=torch.rand(9, 3))
    normals = torch.nn.functional.normalize(torch.randn(9, 3), dim=1)
    plain, with_n, with_pn = tmp_path / "a.ply", tmp_path / "b.ply", tmp_path / "c.ply"
    fusion.write_ply(str(plain), cloud)
    fusion.write_ply(str(with_n), cloud, normals=normals)
    fusion.write_ply(str(with_pn), cloud, fusion.PointNormals(normal=normals, variation=torch.zeros(9), valid=torch.ones(9, dtype=torch.bool),
                                                             neighbours=None))
    # without normals: byte for byte the file of before -- header and the 15-byte records rebuilt here by hand
    rec = np.zeros(9, dtype=np.dtype([("xyz", "<f4", (3,)), ("rgb", "u1", (3,))]))
    rec["xyz"], rec["rgb"] = cloud.xyz.numpy(), np.rint(cloud.rgb.clamp(0, 1).numpy() * 255).astype("u1")
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex 9\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert plain.read_bytes() == head.encode("ascii") + rec.tobytes()
    raw = with_n.read_bytes()
    assert raw == with_pn.read_bytes()
    h, body = raw.split(b"end_header\n")
    assert h.decode().splitlines()[3:] == [f"property float {c}" for c in ("x", "y", "z", "nx", "ny", "nz")] + \
        [f"property uchar {c}" for c in ("red", "green", "blue")]
    got = np.frombuffer(body, dtype=np.dtype([("xyz", "<f4", (3,)), ("n", "<f4", (3,)), ("rgb", "u1", (3,))]))
    assert len(body) == 9 * 27 and np.array_equal(got["xyz"], cloud.xyz.numpy()) and np.array_equal(got["n"], normals.numpy())
    assert np.array_equal(got["rgb"], rec["rgb"])
    for bad in (normals[:8], normals[:, :2], "normals"):
        with pytest.raises(ValueError):
            fusion.write_ply(str(plain), cloud, normals=bad)
