"""The mesh-topology oracle (tests/meshtopo_f64.py) held to answers known by hand, and every refusal of the host API
(mvdfusion_amd/fusion.py: mesh_components, mesh_topology, filter_mesh, keep_components, vertex_normals, smooth_mesh).  No GPU.

Taubin smoothing of the marched exact sphere at G = 24 (20 passes, lam 0.5, mu -0.53), measured with this oracle: the mean angle between
the vertex normals and the radial direction falls from 1.8867 to 0.9046 degrees over 5 150 vertices, the mean radius moves from 0.599503
to 0.599674, by 1.7e-4 (a voxel is 6.25e-2).
"""
import math

import numpy as np
import pytest
import torch

import fusion_f64 as F
import meshtopo_f64 as M
import tsdf_f64 as T


def _totals(m):
    t, flags = M.topology(m)
    return [dict(zip(M.TOTALS, (int(x) for x in row))) for row in t], flags


def test_tetrahedron_is_closed_manifold_oriented():
    (t,), flags = _totals(M.tetrahedron())
    assert t["components"] == 1 and t["boundary_edges"] == 0 and t["nonmanifold_edges"] == 0 and t["misoriented_edges"] == 0
    assert t["edges"] == 6 and t["euler"] == 2 and t["vertices_used"] == 4 and t["faces_regular"] == 4 and not flags.any()


def test_cube_and_cube_with_a_face_pair_removed():
    (t,), flags = _totals(M.cube())
    assert (t["edges"], t["boundary_edges"], t["misoriented_edges"], t["euler"], t["components"]) == (18, 0, 0, 2, 1)
    (t,), flags = _totals(M.cube(1))
    assert (t["edges"], t["boundary_edges"], t["nonmanifold_edges"], t["misoriented_edges"], t["euler"]) == (17, 4, 0, 0, 1)
    assert sorted(np.nonzero(flags & M.FLAG_BOUNDARY)[0].tolist()) == [1, 3, 5, 7]      # the corners of the missing x = 1 quad


def test_two_triangles_wound_alike_across_their_edge():
    v = np.zeros((4, 3))
    (t,), _ = _totals(M.make(v, [(0, 1, 2), (3, 1, 2)]))
    assert t["misoriented_edges"] == 1 and t["edges"] == 5 and t["boundary_edges"] == 4
    (t,), _ = _totals(M.make(v, [(0, 1, 2), (1, 3, 2)]))
    assert t["misoriented_edges"] == 0


def test_three_triangles_on_one_edge():
    (t,), flags = _totals(M.make(np.zeros((5, 3)), [(0, 1, 2), (1, 0, 3), (0, 1, 4)]))
    assert t["nonmanifold_edges"] == 1 and t["edges"] == 7 and t["boundary_edges"] == 6 and t["misoriented_edges"] == 0
    assert flags.tolist() == [3, 3, 1, 1, 1]


def test_unreferenced_vertex_is_counted_and_labelled_minus_one():
    m = M.make(np.zeros((5, 3)), [(0, 1, 2), (2, 1, 4)])
    (t,), _ = _totals(m)
    c = M.components(m)
    assert t["unreferenced"] == 1 and t["vertices_used"] == 4
    assert c["vertex_component"].tolist() == [0, 0, 0, -1, 0] and c["vertices"].tolist() == [4]


def test_repeated_face_joins_two_pieces_and_adds_no_edge():
    pieces = [(0, 1, 2), (3, 4, 5)]
    (apart,), _ = _totals(M.make(np.zeros((6, 3)), pieces))
    m = M.make(np.zeros((6, 3)), pieces + [(2, 3, 3)])
    (joined,), _ = _totals(m)
    assert apart["components"] == 2 and joined["components"] == 1
    assert joined["edges"] == apart["edges"] == 6 and joined["faces_repeated"] == 1 and joined["faces_regular"] == 2
    c = M.components(m)
    assert c["face_component"].tolist() == [0, 0, 0] and c["faces"].tolist() == [3] and c["root"].tolist() == [0]
    inc_start, inc = M.incidence(m)
    assert len(inc) == 6 and inc_start.tolist() == [0, 1, 2, 3, 4, 5, 6]      # no incidence entry of the repeated face


def test_invalid_faces_and_the_batch_tables():
    m = M.mixed_batch()
    t, _ = _totals(m)
    assert [x["faces_invalid"] for x in t] == [0, 3] and [x["faces_repeated"] for x in t] == [0, 1]
    assert [x["components"] for x in t] == [2, 2] and [x["unreferenced"] for x in t] == [1, 0]
    assert (t[0]["boundary_edges"], t[0]["euler"]) == (0, 4) and (t[1]["nonmanifold_edges"], t[1]["misoriented_edges"]) == (1, 2)
    c = M.components(m)
    assert c["component_start"].tolist() == [0, 2, 4] and c["root"].tolist() == [0, 8, 13, 22] and c["face_component"][-3:].tolist() == [-1] * 3
    alone = M.components(M.scene_of(m, 1))                            # a scene alone: the same components, ids un-shifted
    f0, v0 = m.face_start[1], m.vertex_start[1]
    assert np.array_equal(alone["face_component"], np.where(c["face_component"][f0:] < 0, -1, c["face_component"][f0:] - 2))
    assert np.array_equal(alone["root"], c["root"][2:] - v0)


def test_filter_keeps_order_and_rebases():
    m = M.mixed_batch()
    keep = M.largest(m, M.components(m), 1)
    assert keep.sum() == 12 + 7
    out, vi, fi = M.filter_faces(m, keep)
    assert out.vertex_start.tolist() == [0, 8, 17] and out.face_start.tolist() == [0, 12, 19]
    assert np.array_equal(out.vertices, m.vertices[vi]) and np.array_equal(out.rgb, m.rgb[vi]) and np.array_equal(vi[out.faces], m.faces[fi])
    everything, _, fi = M.filter_faces(m, np.ones(len(m.faces), dtype=bool))
    assert len(fi) == len(m.faces) - 3 and len(everything.vertices) == len(m.vertices) - 1      # invalid faces are never kept
    (t,), _ = _totals(M.scene_of(out, 0))
    assert t["components"] == 1 and t["euler"] == 2


def test_host_largest_matches_the_oracle():
    from mvdfusion_amd.fusion import MeshComponents
    m = M.concat([M.tetrahedra(3), M.scene_of(M.mixed_batch(), 0), M.make(np.zeros((0, 3)), np.zeros((0, 3)))])
    c = M.components(m)
    host = MeshComponents(**{k: torch.from_numpy(v) for k, v in c.items()})
    for k in (1, 2, 5):
        assert np.array_equal(host.largest(k).numpy(), M.largest(m, c, k)), k
    assert M.largest(m, c, 1).sum() == 4 + 12      # equal counts: the lower id (the first tetrahedron); the cube over the tetrahedron


def _sphere_mesh():
    ref = T.march(T.sphere_volume(24))
    return M.make(ref.vertices.numpy(), ref.faces.numpy())


def _radial_angle(m):
    n = M.vertex_normals(m)[0]
    x = m.vertices.astype(np.float64)
    r = np.linalg.norm(x, axis=1)
    cos = np.clip((n * x).sum(1) / r, -1.0, 1.0)
    return float(np.degrees(np.arccos(cos)).mean()), float(r.mean())


def test_taubin_on_the_marched_sphere():
    """Directions and a derived bound, not tuned thresholds: smoothing must bring the normals closer to the radial direction, and a
    smoothing that does not shrink cannot move the mean radius by a voxel."""
    m = _sphere_mesh()
    (t,), flags = _totals(m)
    assert t["components"] == 1 and t["boundary_edges"] == 0 and t["nonmanifold_edges"] == 0 and t["misoriented_edges"] == 0 and t["euler"] == 2
    before, r0 = _radial_angle(m)
    smooth = M.Mesh(M.smooth(m, 20, 0.5, -0.53, flags, M.FLAG_BOUNDARY), m.faces, m.vertex_start, m.face_start)
    after, r1 = _radial_angle(smooth)
    voxel = 2 * 0.75 / 24
    print(f"taubin sphere G=24: {len(m.vertices)} vertices | mean angle to radial {before:.4f} -> {after:.4f} deg | mean radius {r0:.6f} -> {r1:.6f} "
          f"(moved {abs(r1 - r0):.3e}, voxel {voxel:.3e}, sphere {F.SPHERE_R})")
    assert after < before
    assert abs(r1 - r0) < voxel


def test_pinned_and_isolated_vertices_do_not_move():
    m = M.mixed_batch()
    _, flags = M.topology(m)
    x = M.smooth(m, 3, 0.5, -0.53, flags, M.FLAG_BOUNDARY)
    pinned = (flags & M.FLAG_BOUNDARY) != 0
    assert pinned.any() and np.array_equal(x[pinned], m.vertices[pinned]) and np.array_equal(x[12], m.vertices[12])
    assert not np.array_equal(x[:8], m.vertices[:8])
    free = M.smooth(m, 3, 0.5, -0.53)
    assert not np.array_equal(free[pinned], m.vertices[pinned])
    bad = M.Mesh(m.vertices.copy(), m.faces, m.vertex_start, m.face_start)
    bad.vertices[0, 1] = np.inf
    y = M.smooth(bad, 1, 0.5, -0.53)
    touched = np.unique(m.faces[:12][(m.faces[:12] == 0).any(1)])
    assert np.array_equal(y[touched], bad.vertices[touched])           # a vertex that would read a non-finite coordinate stays


def test_floater_placement_leaves_the_big_sphere_alone():
    """What the GPU end-to-end test rests on, on the oracle: U == B at every corner of every cell the big surface crosses, so the marcher
    gives the big sphere the same vertices and faces in the same order in both; the largest component of march(U) is march(B) bit for
    bit; the floaters are three closed spheres that do not reach the box."""
    B, U = M.blob_volumes()
    G = M.BLOB_G
    inside = (B < 0).numpy()
    corners = [inside[dz:G - 1 + dz, dy:G - 1 + dy, dx:G - 1 + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    crossed = np.stack(corners).any(0) & ~np.stack(corners).all(0)                       # (G - 1)^3 cells
    near = np.zeros((G, G, G), dtype=bool)                                               # the corners of the crossed cells
    for k, j, i in zip(*np.nonzero(crossed)):
        near[k:k + 2, j:j + 2, i:i + 2] = True
    assert crossed.sum() > 0 and np.array_equal(U.numpy()[near], B.numpy()[near])
    assert int((U != B).sum()) > 0 and not (U.numpy() < 0)[[0, -1]].any() and not (U.numpy() < 0)[:, [0, -1]].any() and not (U.numpy() < 0)[:, :, [0, -1]].any()
    mb, mu = T.march(B[None]), T.march(U[None])
    big, all_ = M.make(mb.vertices.numpy(), mb.faces.numpy()), M.make(mu.vertices.numpy(), mu.faces.numpy())
    (t,), _ = _totals(all_)
    assert (t["components"], t["boundary_edges"], t["nonmanifold_edges"], t["misoriented_edges"], t["euler"]) == (4, 0, 0, 0, 8)
    kept, _, _ = M.filter_faces(all_, M.largest(all_, M.components(all_), 1))
    assert np.array_equal(kept.vertices, big.vertices) and np.array_equal(kept.faces, big.faces)
    assert kept.vertex_start.tolist() == [0, len(big.vertices)] and kept.face_start.tolist() == [0, len(big.faces)]


# ------------------------------------------------------------------------------------------------ refusals of the host API
def _host_mesh(m=None, **over):
    from mvdfusion_amd.fusion import TriangleMesh
    m = M.tetrahedron() if m is None else m
    kw = dict(vertices=torch.from_numpy(m.vertices), faces=torch.from_numpy(m.faces), rgb=None,
              vertex_start=torch.from_numpy(m.vertex_start).int(), face_start=torch.from_numpy(m.face_start).int())
    kw.update(over)
    return TriangleMesh(**kw)


def test_host_api_refusals():
    from mvdfusion_amd import fusion as fz
    good = _host_mesh()
    entries = [fz.mesh_components, fz.mesh_topology, fz.vertex_normals, fz.smooth_mesh, lambda m: fz.filter_mesh(m, torch.ones(4, dtype=torch.bool)),
               lambda m: fz.keep_components(m, largest=1)]
    bad = [torch.zeros(4, 3),                                                    # not a TriangleMesh
           _host_mesh(vertices=torch.zeros(4, 2)), _host_mesh(faces=torch.zeros(4, 4, dtype=torch.int32)), _host_mesh(faces=torch.zeros(12, dtype=torch.int32)),
           _host_mesh(rgb=torch.zeros(3, 3)),
           _host_mesh(face_start=torch.tensor([0, 5], dtype=torch.int32)), _host_mesh(vertex_start=torch.tensor([0, 9], dtype=torch.int32)),
           _host_mesh(face_start=torch.tensor([2, 1, 4], dtype=torch.int32), vertex_start=torch.tensor([0, 2, 4], dtype=torch.int32)),
           _host_mesh(face_start=torch.tensor([0, 2, 4], dtype=torch.int32)),    # tables of different scene counts
           _host_mesh(vertex_start=torch.tensor([0], dtype=torch.int32), face_start=torch.tensor([0], dtype=torch.int32))]
    for fn in entries:
        for mesh in bad:
            with pytest.raises(ValueError):
                fn(mesh)
    for keep in (torch.ones(3, dtype=torch.bool), torch.ones(5, dtype=torch.uint8), torch.ones(4, 1, dtype=torch.bool), torch.ones(4), [1, 1, 1, 1]):
        with pytest.raises(ValueError, match="keep_faces"):
            fz.filter_mesh(good, keep)
    with pytest.raises(ValueError, match="at least one"):
        fz.keep_components(good)
    for kw in (dict(largest=0), dict(largest=1.5), dict(largest=-1), dict(min_faces=-1), dict(min_faces=2.5), dict(min_fraction=1.5),
               dict(min_fraction=-0.1), dict(min_fraction=float("nan"))):
        with pytest.raises(ValueError):
            fz.keep_components(good, **kw)
    for kw in (dict(iters=-1), dict(iters=1001), dict(iters=2.5), dict(lam=float("nan")), dict(lam=float("inf")), dict(mu=float("-inf")),
               dict(mu=float("nan"))):
        with pytest.raises(ValueError):
            fz.smooth_mesh(good, **kw)
    comp = fz.MeshComponents(**{k: torch.from_numpy(v) for k, v in M.components(M.tetrahedron()).items()})
    for k in (0, -1, 1.5):
        with pytest.raises(ValueError, match="k ="):
            comp.largest(k)
    assert comp.largest(1).tolist() == [True] * 4


def test_write_ply_takes_vertex_normals(tmp_path):
    """An (n, 3) tensor -- what vertex_normals returns -- goes behind x y z; without it the file is what it was."""
    from mvdfusion_amd.fusion import write_ply
    m = M.tetrahedron()
    mesh = _host_mesh(m)
    write_ply(tmp_path / "plain.ply", mesh)
    write_ply(tmp_path / "normals.ply", mesh, torch.from_numpy(M.vertex_normals(m)[1]))
    plain, withn = (tmp_path / "plain.ply").read_bytes(), (tmp_path / "normals.ply").read_bytes()
    assert b"property float nx" in withn and b"property float nx" not in plain
    assert len(withn) - len(plain) == 4 * 12 + len(b"property float nx\nproperty float ny\nproperty float nz\n")
    body = np.frombuffer(withn[withn.index(b"end_header\n") + 11:][:4 * 24], dtype="<f4").reshape(4, 6)
    assert np.array_equal(body[:, :3], m.vertices) and np.array_equal(body[:, 3:], M.vertex_normals(m)[1])
    assert all(math.isclose(float(np.linalg.norm(r)), 1.0, rel_tol=1e-6) for r in body[:, 3:])


def test_constants_match_the_header():
    import os
    import re
    from mvdfusion_amd import hip
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mvd_hip.h")).read()
    value = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))
    assert value("MVD_TOPO_TOTALS") == hip.TOPO_TOTALS == len(hip.TOPO_FIELDS) == len(M.TOTALS) and hip.TOPO_FIELDS == M.TOTALS
    assert (value("MVD_TOPO_FLAG_BOUNDARY"), value("MVD_TOPO_FLAG_NONMANIFOLD")) == (hip.TOPO_FLAG_BOUNDARY, hip.TOPO_FLAG_NONMANIFOLD) == (1, 2)
    assert value("MVD_SMOOTH_MAX_PASSES") == hip.SMOOTH_MAX_PASSES == 2000
