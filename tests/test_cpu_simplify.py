"""tests/simplify_f64.py held to answers known by hand, the margins of every fixture of tests/test_gpu_simplify.py, the refusals of
fusion.simplify_mesh (raised before anything is enqueued, so no GPU is needed) and the header's constants."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import meshtopo_f64 as M
import simplify_f64 as S
import tsdf_f64 as T


def _totals(m):
    totals, _ = M.topology(m)
    return dict(zip(M.TOTALS, (int(t) for t in totals[0])))


def test_subdivided_cube_collapses_to_the_cube():
    c = S.subdivided_cube()
    assert (len(c.vertices), len(c.faces)) == (98, 192)
    r = S.simplify(c, 2)
    corners = np.array([[i & 1, (i >> 1) & 1, i >> 2] for i in range(8)], dtype=np.float64)
    assert r["out64"].shape == (8, 3) and np.abs(r["out64"] - corners).max() <= 1e-12
    assert r["final_rank"].tolist() == [3] * 8 and r["final_placed"].tolist() == [S.PLACED_QUADRIC] * 8
    t = _totals(r["out"])
    assert (t["faces_regular"], t["edges"], t["boundary_edges"], t["nonmanifold_edges"], t["misoriented_edges"], t["euler"]) == (12, 18, 0, 0, 0, 2)
    assert int(r["size"].sum()) == 98 and (r["final_vertex_cluster"] >= 0).all()
    mean = S.simplify(c, 2, S.MEAN)
    assert np.allclose(mean["out64"][0], 0.75 / 7.0, atol=1e-15) and abs(mean["out64"][0, 0] - 0.107) < 5e-4      # the corner is rounded off
    assert mean["final_rank"].tolist() == [0] * 8 and mean["final_placed"].tolist() == [S.PLACED_MEAN] * 8
    assert np.array_equal(mean["out"].faces, r["out"].faces)


def test_one_cell_leaves_nothing():
    for m in (S.subdivided_cube(), M.tetrahedron(), M.mixed_batch()):
        r = S.simplify(m, 1)
        assert len(r["out"].vertices) == 0 and len(r["out"].faces) == 0 and not r["keep"].any()
        assert len(r["members"]) == int((np.diff(r["cluster_start"]) > 0).sum())      # one cluster per scene that has a member
        assert (r["final_vertex_cluster"] == -1).all()


def test_flat_grid_stays_in_its_plane():
    r = S.simplify(S.flat_grid(), 4)
    assert len(r["out"].faces) > 0 and (r["final_rank"] == 1).all() and (r["final_placed"] == S.PLACED_QUADRIC).all()
    assert (r["out"].vertices[:, 2] == np.float32(0.25)).all()
    # along the plane nothing is determined: the point is the members' mean there
    mean = S.simplify(S.flat_grid(), 4, S.MEAN)
    assert np.abs(r["out64"] - mean["out64"]).max() <= 1e-12


def test_two_sheets_closer_than_a_cell_give_one():
    one, two = S.simplify(S.flat_grid(), 4), S.simplify(S.two_sheets(), 4)
    nf = len(S.flat_grid().faces)
    assert int(two["keep"].sum()) == 2 * int(one["keep"].sum()) and int(two["keep_deduped"].sum()) == int(one["keep_deduped"].sum())
    assert (two["face_index"] < nf).all() and np.array_equal(two["out"].faces, one["out"].faces)      # the lower rows: the first sheet
    assert _totals(two["out"])["nonmanifold_edges"] == 0


def test_bad_and_unused_vertices_vanish():
    clean = M.quad_grid(8, seed=3)
    m, a, b = S.with_bad_vertices(clean, seed=1)
    r = S.simplify(m, 4)
    assert r["vertex_cluster"][a] == -1 and r["vertex_cluster"][b] == -1 and r["vertex_cluster"][len(m.vertices) - 1] == -1
    touched = (m.faces == a).any(1) | (m.faces == b).any(1)
    assert touched.any() and not r["keep"][touched].any() and (r["mapped_faces"][touched] == -1).any(1).all()
    assert np.isfinite(r["vertices64"]).all() and np.isfinite(r["out"].vertices).all()
    assert int(r["size"].sum()) == len(clean.vertices) - 2


def test_uv_sphere_radius_error():
    """What the docstring of simplify_mesh states: on a smooth surface the quadric point is no closer than the mean."""
    sphere = S.uv_sphere()
    for cells, want in ((4, 0.0128), (8, 0.0030), (16, 0.0011)):
        for placement in (S.QUADRIC, S.MEAN):
            r = S.simplify(sphere, cells, placement)
            err = float(np.abs(np.linalg.norm(r["out64"], axis=1) - 0.45).max())
            print(f"uv sphere cells={cells} placement={placement}: {len(r['out'].faces)} faces, worst radius error {err:.4f}")
            assert abs(err - want) < 1e-4, (cells, placement, err)


@pytest.mark.parametrize("name", sorted(S.GPU_CASES))
def test_every_gpu_fixture_has_margins(name):
    m = S.gpu_case(name)
    for cells in S.GPU_CASES[name]:
        r = S.simplify(m, cells, S.QUADRIC)
        print(name, cells, {k: f"{v:.3g}" for k, v in r["margins"].items()})
        for k, v in r["margins"].items():
            assert v > 1e-6, (name, cells, k, v)


@functools.lru_cache(maxsize=None)
def _marched_sphere():
    B, _ = M.blob_volumes()
    ref = T.march(B[None])
    return M.make(ref.vertices.numpy(), ref.faces.numpy())


def test_every_cluster_of_the_marched_sphere_survives():
    """What the GPU end-to-end test rests on: at cells = 8 every cluster of the marched G = 24 sphere keeps its vertex through the
    filter, so the distance bound there covers every member and leaves nothing out; and the bound itself on the oracle."""
    m = _marched_sphere()
    r = S.simplify(m, 8)
    assert len(r["vertex_index"]) == len(r["members"]) > 0 and (r["final_vertex_cluster"][r["vertex_cluster"] >= 0] >= 0).all()
    assert 0 < len(r["out"].faces) < len(m.faces)
    for k, v in r["margins"].items():
        assert v > 1e-6, (k, v)
    member = r["vertex_cluster"] >= 0
    d = np.linalg.norm(m.vertices[member].astype(np.float64) - r["out64"][r["final_vertex_cluster"][member]], axis=1) / r["h"][0]
    print(f"marched sphere: {len(m.faces)} -> {len(r['out'].faces)} faces, member to its own vertex at most {d.max():.3f} h")
    assert d.max() <= math.sqrt(3.0) * (1.0 + 1.0 / 512.0)


# ------------------------------------------------------------------------------------------------ the host API
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
    for cells in (0, 257, 2.5, -1, True):
        with pytest.raises(ValueError, match="cells"):
            fz.simplify_mesh(good, cells=cells)
    with pytest.raises(ValueError, match="placement"):
        fz.simplify_mesh(good, placement="median")
    for bad in (torch.zeros(4, 3), None, _host_mesh(vertices=torch.zeros(4, 2)), _host_mesh(face_start=torch.tensor([0, 5], dtype=torch.int32))):
        with pytest.raises(ValueError):
            fz.simplify_mesh(bad)
    batch = M.concat([M.tetrahedron()] * 17)
    with pytest.raises(ValueError, match="2\\^28"):
        fz.simplify_mesh(_host_mesh(batch), cells=256)             # 17 * 256^3 > 2^28
    assert fz.SIMPLIFY_CELLS == 64 and "nobody has tuned" in fz.simplify_mesh.__doc__


def test_viewfusion_mesh_takes_simplify():
    import inspect
    from mvdfusion_amd.viewfusion_zero_depth_rgb import ViewFusion
    assert inspect.signature(ViewFusion.mesh).parameters["simplify"].default is None


def test_constants_match_the_header():
    from mvdfusion_amd import hip
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mvd_hip.h")).read()
    value = lambda name: re.search(rf"#define {name} (\S+)", hdr).group(1)
    assert int(value("MVD_SIMPLIFY_MAX_CELLS")) == hip.SIMPLIFY_MAX_CELLS == S.MAX_CELLS == 256
    assert (int(value("MVD_SIMPLIFY_MEAN")), int(value("MVD_SIMPLIFY_QUADRIC"))) == (hip.SIMPLIFY_MEAN, hip.SIMPLIFY_QUADRIC) == (S.MEAN, S.QUADRIC)
    placed = tuple(int(value(f"MVD_SIMPLIFY_PLACED_{k}")) for k in ("MEAN", "QUADRIC", "FALLBACK"))
    assert placed == (hip.SIMPLIFY_PLACED_MEAN, hip.SIMPLIFY_PLACED_QUADRIC, hip.SIMPLIFY_PLACED_FALLBACK) == (S.PLACED_MEAN, S.PLACED_QUADRIC, S.PLACED_FALLBACK)
    assert float(value("MVD_SIMPLIFY_RANK_RATIO")) == hip.SIMPLIFY_RANK_RATIO == S.RANK_RATIO == 1e-3
    assert int(value("MVD_SIMPLIFY_BOX_SLACK_DIV")) == hip.SIMPLIFY_BOX_SLACK_DIV == S.BOX_SLACK_DIV == 1024
    assert int(value("MVD_NORMALS_SWEEPS")) == S.SWEEPS and hip.SIMPLIFY_MAX_TABLE == S.MAX_TABLE
    for name in ("mvd_mesh_cluster_scratch", "mvd_mesh_cluster_count", "mvd_mesh_cluster_emit", "mvd_mesh_cluster_dedupe"):
        assert name in hip.SIGNATURES and re.search(rf"\b{name}\(", hdr), name
