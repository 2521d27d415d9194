"""The point-to-mesh entries without a GPU: the two oracles of tests/meshdist_f64.py held to each other and to what the cases are for
(where the figures quoted in tests/test_gpu_meshdist.py come from), header, binding and constants, and the host side of
fusion.nearest_on_mesh, fusion.compare_geometry(exact=True) and fusion.align_to_mesh against stub enqueues.

Bounds: tests/meshdist_f64.py derives them (one fp32 ulp of the exact d2 rounded to fp32, from the smallest altitude of each case's
faces); none is taken from what the code under test gives.

Measured (the float64 restatement against exact rational arithmetic): on the 2 461 pairs of 357 queries of the ten cases fl32(d2) differs
from fl32(d2_exact) on no pair (bound: one ulp); the float64 d2 itself is within 4.3e-13 relative of the exact value at worst (sphere;
9.4e-14 on scenes, a few 1e-15 elsewhere, exactly equal on the dyadic cases; the premise needs < 2^-25 = 3e-8); the chosen face is an
exact minimiser on every sampled query.  The ICP oracle on the 1 984-face ellipsoid ends 7.6e-4 from the truth (the faceting), plane rms
0.0252 -> 0.00166, rank 6 on every row, clearance 1.1e7.
"""
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import meshdist_f64 as M
import plane_f64 as P
from mvdfusion_amd import fusion, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement and its cases
@pytest.mark.parametrize("name", M.CASES)
def test_the_restatement_and_the_cases_reach_what_they_are_for(name):
    case, ref = M.make_case(name), M.refs(name)
    ok, tri = M.candidates(case)
    hit = ref.face >= 0
    assert np.array_equal(hit, ref.dist2 < np.inf) and np.array_equal(hit, ref.region >= 0) and np.array_equal(hit, ~np.isnan(ref.point).any(1))
    assert ok[ref.face[hit]].all() and not ref.bary[~hit].any() and not ref.normal[~hit].any() and (ref.region[hit] <= 6).all()
    b = ref.bary[hit].astype(np.float64)
    assert (b >= 0).all() and np.abs(b.sum(1) - 1).max(initial=0) <= 2.0 ** -22          # (three fp32 roundings of a partition of one)
    kinds = (ref.region[hit] <= 2), (ref.region[hit] >= 3) & (ref.region[hit] <= 5), ref.region[hit] == 6
    assert ((b == 1).sum(1)[kinds[0]] == 1).all() and ((b == 0).sum(1)[kinds[1]] >= 1).all()
    print(f"{name}: nq {case.nq} nf {case.nf} candidates {int(ok.sum())} scenes {case.nscene} | found {int(hit.sum())} | regions "
          f"{np.bincount(ref.region[hit], minlength=7).tolist()}")
    if name == "one_triangle":
        told = case.region >= 0
        assert told.sum() == 24 and np.array_equal(ref.region[told], case.region[told]) and set(case.region[told]) == set(range(7))
        on = case.region == -2
        assert (ref.dist2[on][:6] == 0).all() and (ref.dist2[on][6:] > 1e11).all()          # on the triangle: exactly 0; far away: 1e6
        assert (ref.dist2[(case.region == 6)][:2] == 0).all()                                 # in the plane, inside
    if name in ("tie_pair", "tie_pair_swapped"):
        assert (ref.face[[0, 1, 10]] == 0).all() and (ref.region[[0, 1]] >= 3).all()          # above / on the shared edge: the lowest row
        other = M.refs("tie_pair_swapped" if name == "tie_pair" else "tie_pair")
        assert np.array_equal(ref.dist2.view(np.int32), other.dist2.view(np.int32))           # the listing order changes no distance
    if name == "tetrahedron":
        assert ref.face[0] == 0 and len({float(M.closest(case.query[0].astype(np.float64), t)[0]) for t in tri}) == 1      # the centre: a four-way tie
    if name == "cube":
        d = np.sqrt(ref.dist2.astype(np.float64))
        assert d[13] == 0.5 and (np.delete(d[:27], 13) == 0).all()          # the centre; face centres, edge midpoints and corners lie ON the cube
        assert ref.face[13] == 0                                                              # the centre: all twelve faces tie
    if name == "sphere":
        assert case.nf == 1280 and case.nq == 3001 and case.nq % 64 and all(k.any() for k in kinds)
    if name == "mixed":
        big = np.nonzero(M.aspect2(tri) < np.inf)[0][np.argsort(-np.ptp(tri.reshape(-1, 3, 3), axis=1).max(1))[:2]]
        assert case.nf == 2002 and np.isin(ref.face, big).sum() > 20 and (~np.isin(ref.face, big)).sum() > 20      # both paths win queries
    if name == "odd":
        assert int((~ok).sum()) == 10 and int((M.aspect2(tri[ok]) == np.inf).sum()) == 6 and not hit[380:].any() and not hit[20:24].any()
        shape = M.aspect2(tri[ok])
        assert ((shape <= 16) | (shape == np.inf)).all()          # well shaped or exactly degenerate, nothing between
        flat = np.isin(ref.face, np.nonzero(ok & (M.aspect2(tri) == np.inf))[0])
        assert flat.sum() >= 4 and not ref.normal[flat].any() and hit[:20].all()              # a degenerate face is found, with a zero normal
    if name == "scenes":
        assert np.diff(case.face_start).tolist() == [700, 2, 0, 1301] and not hit[890:].any() and not hit[350:390].any() and hit[:350].all()
        for s in (0, 1, 3):       # a scene alone has the batch's results
            alone, f0, (q0, q1) = M.scene_case(case, s)
            one = M.search(alone)
            assert np.array_equal(one.face + f0, ref.face[q0:q1]) and np.array_equal(one.dist2.view(np.int32), ref.dist2[q0:q1].view(np.int32))


@pytest.mark.parametrize("name", M.CASES)
def test_the_float64_rule_meets_exact_rational_arithmetic(name):
    case, ref = M.make_case(name), M.refs(name)
    _, tri = M.candidates(case)
    pairs = M.exact_pairs(name)
    worst_rel, n, off = 0.0, 0, 0
    for i, rows in pairs.items():
        q = case.query[i].astype(np.float64)
        exact = {f: M.exact_d2(case.query[i], tri[f].astype(np.float32)) for f in rows}
        for f in rows:
            got = float(M.closest(q, tri[f])[0])
            want32 = M.fl32(exact[f])
            assert M.conditioning_ok(case, i, f, exact[f]), (name, i, f)
            assert M.within_one_ulp(M.fl32(got), want32), (name, i, f, got, float(exact[f]))
            off += M.fl32(got) != want32
            if exact[f] > 0:
                worst_rel = max(worst_rel, abs(got - float(exact[f])) / float(exact[f]))
            n += 1
        chosen = int(ref.face[i])
        assert chosen in exact and M.within_one_ulp(M.fl32(exact[chosen]), M.fl32(min(exact.values()))), (name, i, chosen)
        assert M.within_one_ulp(float(ref.dist2[i]), M.fl32(min(exact.values())))
    print(f"{name}: {len(pairs)} queries, {n} pairs | fl32(d2) off by one ulp on {off} | float64 d2 within {worst_rel:.3g} relative of the exact value")
    assert n >= (1 if case.nf <= 2 else 20)


# ------------------------------------------------------------------------------------------------ the ICP oracle
def test_the_icp_oracle_converges_to_the_faceting_and_keeps_clear_of_the_rank_threshold():
    case, ref = M.icp_case(), M.icp_ref()
    own = float(np.abs(ref.matrix - case.truth).max())
    print(f"mesh icp oracle: faces {len(case.faces)} n {case.source.shape[0]} iters {case.iters} | |M - truth| {own:.4g} | plane rms "
          f"{ref.history[0, 0]:.4g} -> {ref.history[-1, 0]:.4g} | clearance {ref.worst_clearance:.3g}")
    assert len(case.faces) == 1984 and case.source.shape[0] == 1024 and case.iters == 12
    assert (ref.history[:, 1] == 1024).all() and (ref.history[:, 3] == 6).all() and ref.worst_clearance >= P.CLEAR
    assert own < 5e-3 and ref.history[-1, 0] < ref.history[0, 0] / 10
    cube = M.cube_icp_case()
    flat = M.icp(cube)
    assert (flat.history[:, 3] == 3).all() and flat.worst_clearance >= P.CLEAR and (flat.found.face >= 0).all()
    assert flat.history[-1, 0] <= 1e-6
    # the plane fixes z and the two tilts; ONE step leaves x, y and the turn about z exactly where they were (the rows of H for them are
    # exactly zero: every normal is (0, 0, 1)).  Steps do not commute, so the composition of several shows second-order terms there.
    one = M.icp(cube, iters=1).matrix
    assert abs(one[0, 3]) <= 1e-12 and abs(one[1, 3]) <= 1e-12 and abs(one[1, 0] - one[0, 1]) <= 1e-12 and abs(one[2, 3]) > 1e-3


# ------------------------------------------------------------------------------------------------ header, binding, constants
def test_the_header_and_the_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    assert int(re.search(r"#define\s+MVD_MESH_SPAN\s+(\d+)", hdr).group(1)) == hip.MESH_SPAN == M.SPAN == 3
    for name, count in (("mvd_nearest_on_mesh_scratch", 4), ("mvd_nearest_on_mesh", 20), ("mvd_nearest_on_mesh_stages", 21), ("mvd_mesh_icp_scratch", 5),
                        ("mvd_mesh_icp", 23)):
        decl = re.search(r"^\w+ " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
        assert decl is not None and name in hip.SIGNATURES, name
        assert len(hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == count, name
    csrc = os.path.join(ROOT, "mvdfusion_amd", "csrc")
    build = open(os.path.join(csrc, "build.py")).read()
    assert '"meshdist.hip"' in build and '"nn_grid.hpp"' in build
    # one copy of the grid pieces: both searches include the header, neither defines them
    shared = open(os.path.join(csrc, "nn_grid.hpp")).read()
    for unit in ("nearest.hip", "meshdist.hip"):
        src = open(os.path.join(csrc, unit)).read()
        assert '#include "nn_grid.hpp"' in src
        for piece in ("SceneGrid nn_scene_grid(", "int nn_cell(", "void nn_walk_grid(", "void chunk_scan_kernel(", "unsigned nn_key("):
            assert piece in shared and piece not in src, (unit, piece)
    src = open(os.path.join(csrc, "meshdist.hip")).read()
    assert "atomicAdd(p, 1u)" in src and src.count("atomicAdd") == 1 and "float atomics" not in src          # integer atomics only
    assert "mvd_nearest_on_mesh_stages(" in open(os.path.join(csrc, "align.hip")).read()


# ------------------------------------------------------------------------------------------------ the host side
def _mesh(scenes=1, colour=True):
    case = M.make_case("cube")
    v, f = torch.from_numpy(case.vertices), torch.from_numpy(case.faces)
    nv, nf = len(v), len(f)
    vertices = torch.cat([v + 2.0 * s for s in range(scenes)])
    faces = torch.cat([f + nv * s for s in range(scenes)])
    return fusion.TriangleMesh(vertices=vertices, faces=faces, rgb=(vertices + 0.5).clamp(0, 1) if colour else None,
                               vertex_start=torch.arange(scenes + 1, dtype=torch.int32) * nv, face_start=torch.arange(scenes + 1, dtype=torch.int32) * nf)


@pytest.fixture
def stub(monkeypatch):
    """fusion._nearest_on_mesh replaced by the oracle: the host side runs on CPU tensors and nothing reaches the library."""
    calls = []

    def fake(query, query_start, vertices, faces, face_start, N, method, grid):
        calls.append(dict(query=query, query_start=query_start, vertices=vertices, faces=faces, face_start=face_start, N=N, method=method, grid=grid))
        found = M.search(M._case(query.numpy(), vertices.numpy(), faces.numpy(), query_start=query_start.numpy(), face_start=face_start.numpy()))
        t = torch.from_numpy
        return fusion.NearestOnMesh(face=t(found.face), dist2=t(found.dist2), point=t(found.point), bary=t(found.bary), region=t(found.region),
                                    normal=t(found.normal))
    monkeypatch.setattr(fusion, "_nearest_on_mesh", fake)
    return calls


def test_nearest_on_mesh_validates_its_arguments_and_passes_the_offsets_down(stub):
    mesh = _mesh(2)
    q = torch.tensor([[0.0, 0.0, 0.75], [2.0, 2.0, 2.0], [0.25, 0.25, 0.5]])
    cloud = dataclasses.make_dataclass("Cloud", ["xyz", "scene"])(xyz=q, scene=torch.tensor([0, 1, 1]))
    for kw in (dict(mesh=q), dict(mesh=cloud), dict(scenes=1), dict(scenes=0), dict(method="bvh"), dict(grid=0), dict(grid=257), dict(query=mesh),
               dict(query=torch.rand(4, 2)), dict(mesh=dataclasses.replace(mesh, face_start=torch.tensor([0, 30], dtype=torch.int32))),
               dict(mesh=dataclasses.replace(mesh, faces=mesh.faces[:, :2]))):
        args = dict(query=cloud, mesh=mesh, scenes=2)
        args.update(kw)
        with pytest.raises(ValueError):
            fusion.nearest_on_mesh(**args)
    assert not stub
    with pytest.raises(ValueError, match="nearest_on_mesh"):          # the point search still refuses a mesh, and says where to go
        fusion.nearest_points(q, mesh)
    out = fusion.nearest_on_mesh(cloud, mesh, scenes=3, method="grid", grid=5)
    c = stub[-1]
    assert (c["N"], c["method"], c["grid"]) == (3, hip.NN_GRID, 5) and c["face_start"].tolist() == [0, 12, 24, 24] and c["face_start"].dtype == torch.int32
    assert c["query_start"].tolist() == [0, 1, 3, 3] and c["faces"].dtype == torch.int32 and c["vertices"].dtype == torch.float32
    assert [f.name for f in dataclasses.fields(out)] == ["face", "dist2", "point", "bary", "region", "normal"]
    assert out.hit.tolist() == [True, True, True] and torch.equal(out.dist, out.dist2.sqrt()) and out.dist2.tolist() == [0.0625, 0.25, 4.125]
    assert out.face[0] < 12 <= out.face[1] and out.face[2] >= 12          # a scene searches its own faces (global rows)
    rgb = out.rgb(mesh)
    want = (out.point + 0.5).clamp(0, 1)          # the colour is linear in the position on this mesh, away from the clamp
    assert rgb.shape == (3, 3) and torch.allclose(rgb[0], want[0], atol=1e-6) and rgb[0].tolist() == [0.5, 0.5, 1.0]
    with pytest.raises(ValueError):
        out.rgb(_mesh(2, colour=False))


def test_compare_geometry_exact_measures_to_the_triangles_and_leaves_the_default_alone(stub, monkeypatch):
    mesh = _mesh(1)
    nearest = []
    real = fusion.nearest_points

    def points(query, target, scenes=1, method="auto", grid=None):
        nearest.append((query, target))
        n = len(query.xyz if hasattr(query, "xyz") else query)
        return fusion.NearestPoints(index=torch.zeros(n, dtype=torch.int32), dist2=torch.full((n,), 0.25))
    monkeypatch.setattr(fusion, "nearest_points", points)
    cloud = torch.tensor([[0.0, 0.0, 0.75], [0.5, 0.5, 0.5], [0.0, 0.25, 0.0]])
    plain = fusion.compare_geometry(cloud, mesh, samples=64)
    assert len(nearest) == 2 and not stub and isinstance(plain.a_to_b, fusion.NearestPoints)          # exact=False: the sampled route, untouched
    exact = fusion.compare_geometry(cloud, mesh, samples=64, exact=True, threshold=0.2)
    assert len(nearest) == 3 and len(stub) == 1 and isinstance(exact.a_to_b, fusion.NearestOnMesh) and isinstance(exact.b_to_a, fusion.NearestPoints)
    assert exact.a_to_b.dist.tolist() == [0.25, 0.0, 0.25] and float(exact.accuracy[0]) == 0.5 / 3 and float(exact.precision[0]) == 1 / 3
    assert isinstance(nearest[-1][0], fusion.SurfaceSamples)          # the points taken FROM the mesh are still its samples
    both = fusion.compare_geometry(mesh, mesh, samples=64, exact=True)
    assert len(stub) == 3 and float(both.chamfer[0]) <= 1e-7
    with pytest.raises(ValueError):
        fusion.compare_geometry(cloud, _mesh(2), exact=True)
    assert real is not points and "exact" in fusion.compare_geometry.__doc__


def test_align_to_mesh_validates_before_it_reaches_the_library(monkeypatch):
    reached = []
    monkeypatch.setattr(fusion, "_mesh_icp", lambda *a: reached.append(a))
    mesh, src = _mesh(1), torch.rand(10, 3)
    for kw in (dict(iters=-1), dict(iters=1025), dict(iters=2.5), dict(iters=True), dict(max_distance=-1.0), dict(init="pca"), dict(scenes=0),
               dict(method="bvh"), dict(grid=300), dict(mesh=src), dict(source=mesh), dict(mesh=_mesh(2)), dict(init=torch.eye(3))):
        args = dict(source=src, mesh=mesh)
        args.update(kw)
        with pytest.raises(ValueError):
            fusion.align_to_mesh(**args)
    assert not reached
    for text in ("mvd_mesh_icp", "rigid", "interface defaults"):
        assert text in fusion.align_to_mesh.__doc__, text
    assert "copied, never written into" in fusion.align_geometry.__doc__ and "align_to_mesh" in fusion.align_geometry.__doc__
