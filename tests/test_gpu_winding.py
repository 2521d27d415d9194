"""The winding-number entries on the GPU: mvd_winding_number (csrc/winding.hip) through the C ABI against oracle (a) of
tests/winding_f64.py, and the host path (fusion.winding_number, signed_distance, voxelize_mesh, volume_iou).

Bounds -- none taken from what the kernels give (tests/winding_f64.py derives them):
  MVD_WIND_CELLS, beta = 0   w EQUAL to (a) in bits on every query of every case: the path uses + - * /, floor and sqrt only.  It pins
                             the grid, the member order and the moments.
  every other setting        |w - w_a| <= nf_s * 2^-48, nf_s the candidate faces of the query's scene; NaN exactly where (a) has NaN.
                             cells = 1 with beta = +inf EQUAL in bits to MVD_WIND_EXACT of the same build.
  inside                     equal on every query whose oracle |w - 0.5| exceeds that tolerance; the queries left out are counted and
                             are exactly the case's constructed on-surface ones (tests/test_cpu_winding.py asserts the count per case).
  bit equalities             two runs; BUILD + QUERY against ALL; a scene alone against the scene inside the batch; each NULL-output
                             subset against the full call.
  refusals                   non-zero, the entry's name in mvd_last_error(), every pre-filled buffer untouched.
  end to end                 a marched sphere (G = 24, radius 0.45): voxelize_mesh against the analytic inside test on every voxel
                             centre farther than one voxel diagonal from the sphere (the mesh lies within half a voxel of the sphere,
                             the far field is off by ~2e-2 and a voxel that far from the surface has w within ~0.1 of 0 or 1);
                             volume_iou(m, m) == 1 exactly; the IoU of two spheres offset by 0.1 against the analytic count, equal
                             outside the union of the two bands; signed_distance against nearest_on_mesh.

Cases (tests/winding_f64.py: CASES): nf in {0, 1, 511, 512, 513} around the LDS face tile of 512; 127, 128, 129 occupied cells around the
cell-record tile of 128; nq in {0, 1, 255, 256, 257}; five scenes whose query ranges split inside one workgroup, an empty one in the
middle, one with faces and no queries; faces with ids -1 and nv, a NaN and an inf vertex, exactly collinear dyadic faces, a mesh of
nothing else; NaN and inf queries, queries 1e3 extents outside the box, on a vertex, an edge and a face of the dyadic cube; cells in
{1, 2, 7, 64} x beta in {0, 2, +inf}.

Measured on an MI355X: with beta = 0, w bit-equal to (a) on every query of all 22 cases at all four cells; elsewhere the largest
|w - w_a| is 4.4e-16 (sphere, 3 968 faces, bound 1.41e-11), and sqrt gave no difference anywhere; inside equal on every judged query, the
queries not judged are the 3 face queries of the cube and the 24 rim-plane queries of the hemisphere.  End to end: 2 880 of 13 824 voxels
lie in the one-diagonal band of either sphere; IoU 0.710240 (intersection 1 304, union 1 836), the same as the analytic test on the same
voxels.  The 31 tests take 3.6 s.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import winding_f64 as W

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
math_sqrt3 = 3.0 ** 0.5
OUTPUTS = ("winding", "inside")


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


def _device(case):
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).contiguous().cuda()
    return dict(query=dev(case.query, torch.float32), qstart=dev(case.query_start, torch.int32), vertices=dev(case.vertices, torch.float32),
                faces=dev(case.faces, torch.int32), fstart=dev(case.face_start, torch.int32), nq=case.nq, nv=case.nv, nf=case.nf, nscene=case.nscene)


def _buffers(nq, nbytes):
    n = max(nq, 1)
    return dict(winding=torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda"), inside=torch.full((n,), 77, dtype=torch.uint8, device="cuda"),
                scratch=torch.full((max((nbytes + 7) // 8, 2),), 0x1234, dtype=torch.int64, device="cuda"))


def _untouched(out):
    return bool((out["winding"] == SENTINEL).all()) and bool((out["inside"] == 77).all()) and bool((out["scratch"] == 0x1234).all())


def _call(hip, out, query, qstart, vertices, faces, fstart, nq, nv, nf, nscene, method, cells, beta=2.0, nbytes=None, stages=None, scratch=True,
          scratch_offset=0, skip=(), winding_offset=0):
    p = lambda t: None if t is None or t.numel() == 0 else hip.ptr(t)
    nbytes = out["scratch"].numel() * 8 if nbytes is None else nbytes
    sc = ctypes.c_void_p(out["scratch"].data_ptr() + scratch_offset) if scratch else None
    outs = [None if k in skip else hip.ptr(out[k]) for k in OUTPUTS]
    if winding_offset:
        outs[0] = ctypes.c_void_p(out["winding"].data_ptr() + winding_offset)
    tables = [None if t is None else hip.ptr(t) for t in (qstart, fstart)]
    args = [p(query), tables[0], p(vertices), p(faces), tables[1], nq, nv, nf, nscene, method, cells, beta, *outs, sc, nbytes]
    L = hip.lib()
    if stages is None:
        return L.mvd_winding_number(*args, hip.stream())
    return L.mvd_winding_number_stages(*args, stages, hip.stream())


def _run(hip, case, method, cells=0, beta=2.0, stages=(None,), out=None, skip=()):
    nbytes = int(hip.lib().mvd_winding_scratch(case.nf, case.nscene, method, cells))
    out = _buffers(case.nq, nbytes) if out is None else out
    dev = _device(case)
    for st in stages:
        hip.check(_call(hip, out, method=method, cells=cells, beta=beta, nbytes=nbytes, stages=st, skip=skip, **dev))
    torch.cuda.synchronize()
    return out


def _w(out, nq):
    return out["winding"][:nq].cpu().numpy()


def _same(a, b, nq, keys=OUTPUTS):
    return all(np.array_equal(a[k][:nq].cpu().numpy().view(np.int64 if k == "winding" else np.uint8),
                              b[k][:nq].cpu().numpy().view(np.int64 if k == "winding" else np.uint8)) for k in keys)


# ------------------------------------------------------------------------------------------------ 1. against (a)
@pytest.mark.parametrize("name", W.CASES)
def test_every_setting_meets_the_rule(hip, name):
    case = W.make_case(name)
    tol = W.tolerance(case)
    exact_bits = None
    for method, cells, beta in W.SETTINGS:
        ref = W.refs(name, method, cells, beta)
        out = _run(hip, case, method, cells, beta)
        w, inside = _w(out, case.nq), out["inside"][:case.nq].cpu().numpy()
        label = (name, method, cells, beta)
        assert np.array_equal(np.isnan(w), np.isnan(ref.w)), label
        with np.errstate(invalid="ignore"):
            err = np.nan_to_num(np.abs(w - ref.w))
            judged = np.nan_to_num(np.abs(ref.w - 0.5), nan=1.0) > tol
        other = int((w.view(np.int64) != ref.w.view(np.int64)).sum())
        print(f"RATIO winding {name} method {method} cells {cells} beta {beta} | nq {case.nq} nf {case.nf} occupied {ref.occupied} | largest |w - w_a| "
              f"{err.max(initial=0):.3g} (bound {tol.max(initial=0):.3g}) | other bits {other} | inside not judged {int((~judged).sum())}")
        if method == W.CELLS and beta == 0.0:
            assert other == 0, label
        assert (err <= tol).all(), (label, float(err.max()))
        assert np.array_equal(inside[judged], ref.inside[judged]), label
        # (a far field moves w at an on-surface query away from 0.5 by its own error, and the query is then judged like any other)
        assert int((~judged).sum()) == case.on_surface if (method == W.EXACT or beta == W.INF) else int((~judged).sum()) <= case.on_surface, label
        assert not inside[np.isnan(ref.w)].any(), label
        if method == W.EXACT:
            exact_bits = w.view(np.int64).copy()
        if method == W.CELLS and cells == 1 and beta == W.INF:
            assert np.array_equal(w.view(np.int64), exact_bits), label
    auto = _w(_run(hip, case, W.AUTO, 0, 2.0), case.nq)          # what is known by hand, under the library's own choice of method
    for i, known in case.known:
        assert abs(auto[i] - known) <= tol[i], (name, i, auto[i], known)


# ------------------------------------------------------------------------------------------------ 2. determinism, stages, scenes, NULLs
@pytest.mark.parametrize("name", ["odd", "scenes", "cells_129"])
def test_two_runs_and_the_stages_give_equal_bits(hip, name):
    case = W.make_case(name)
    for method, cells, beta in [(W.EXACT, 0, 2.0), (W.CELLS, 2, 2.0), (W.CELLS, 7, 2.0), (W.CELLS, 7, 0.0), (W.CELLS, 0, W.INF), (W.AUTO, 0, 2.0)]:
        one, again = _run(hip, case, method, cells, beta), _run(hip, case, method, cells, beta)
        assert not bool((one["winding"][:case.nq] == SENTINEL).any()) and not bool((one["inside"][:case.nq] == 77).any())
        assert _same(one, again, case.nq), (method, cells, beta)
        built = _run(hip, case, method, cells, beta, stages=(hip.NN_BUILD,))
        assert bool((built["winding"] == SENTINEL).all()) and bool((built["inside"] == 77).all())          # nothing queried yet
        assert _same(one, _run(hip, case, method, cells, beta, stages=(hip.NN_QUERY,), out=built), case.nq), (method, cells, beta)
        assert _same(one, _run(hip, case, method, cells, beta, stages=(hip.NN_BUILD, hip.NN_QUERY, hip.NN_QUERY)), case.nq), (method, cells, beta)


def test_a_scene_alone_gives_the_bits_it_gives_in_the_batch(hip):
    case = W.make_case("scenes")
    for method, cells, beta in [(W.EXACT, 0, 2.0), (W.CELLS, 1, W.INF), (W.CELLS, 7, 2.0), (W.CELLS, 64, 0.0)]:
        batch = _run(hip, case, method, cells, beta)
        for s in range(case.nscene):
            alone, (q0, q1) = W.scene_case(case, s)
            if q1 == q0:
                continue
            one = _run(hip, alone, method, cells, beta)
            assert np.array_equal(_w(one, alone.nq).view(np.int64), batch["winding"][q0:q1].cpu().numpy().view(np.int64)), (method, cells, beta, s)
            assert torch.equal(one["inside"][:alone.nq], batch["inside"][q0:q1]), (method, cells, beta, s)


def test_every_subset_of_null_outputs_leaves_the_others_unchanged(hip):
    case = W.make_case("odd")
    for method, cells in ((W.EXACT, 0), (W.CELLS, 7)):
        full = _run(hip, case, method, cells)
        for r in (1, 2):
            for skip in itertools.combinations(OUTPUTS, r):
                out = _run(hip, case, method, cells, skip=skip)
                kept = tuple(k for k in OUTPUTS if k not in skip)
                assert _same(full, out, case.nq, kept), (method, skip)
                assert all(bool((out[k] == (SENTINEL if k == "winding" else 77)).all()) for k in skip), (method, skip)


# ------------------------------------------------------------------------------------------------ 3. refusals, empty calls
def test_bad_arguments_return_an_error_and_write_nothing(hip):
    L = hip.lib()
    case = W.make_case("odd")
    nbytes = int(L.mvd_winding_scratch(case.nf, 1, hip.WIND_CELLS, 7))
    assert nbytes > 0 and int(L.mvd_winding_scratch(case.nf, 1, hip.WIND_EXACT, 0)) == 0 and int(L.mvd_winding_scratch(case.nf, 1, hip.WIND_AUTO, 0)) == 0
    assert int(L.mvd_winding_scratch(4096, 1, hip.WIND_AUTO, 0)) == int(L.mvd_winding_scratch(4096, 1, hip.WIND_CELLS, 0)) > 0
    assert int(L.mvd_winding_scratch(case.nf, 0, hip.WIND_CELLS, 7)) == 0 and int(L.mvd_winding_scratch(case.nf, 1, hip.WIND_CELLS, 65)) == 0
    assert int(L.mvd_winding_scratch(case.nf, 1, 3, 7)) == 0 and int(L.mvd_winding_scratch(case.nf, 1025, hip.WIND_CELLS, 64)) == 0
    good = dict(_device(case), method=hip.WIND_CELLS, cells=7, nbytes=nbytes)
    out = _buffers(case.nq, nbytes)
    bad = [dict(nbytes=nbytes - 16), dict(nbytes=0), dict(scratch=False), dict(scratch_offset=8), dict(winding_offset=4), dict(nscene=0), dict(nscene=-1),
           dict(nscene=65536), dict(method=3), dict(method=-1), dict(cells=65), dict(cells=-1), dict(beta=float("nan")), dict(beta=-1.0),
           dict(beta=-float("inf")), dict(query=None), dict(qstart=None), dict(vertices=None), dict(faces=None), dict(fstart=None), dict(nq=1 << 31),
           dict(nv=1 << 31), dict(nf=1 << 31, nbytes=1 << 62), dict(nscene=1025, cells=64, nbytes=1 << 62)]
    for stages in (None, hip.NN_QUERY, hip.NN_BUILD):
        for kw in bad:
            a = dict(good)
            a.update(kw)
            assert _call(hip, out, stages=stages, **a) != 0, kw
            assert (b"mvd_winding_number_stages" if stages else b"mvd_winding_number:") in L.mvd_last_error(), (kw, L.mvd_last_error())
    for stages in (0, 4, -1):
        assert _call(hip, out, stages=stages, **good) != 0 and b"mvd_winding_number_stages" in L.mvd_last_error()
    exact = dict(good, method=hip.WIND_EXACT, cells=0, scratch=False, nbytes=0)
    for kw in (dict(beta=float("nan")), dict(beta=-0.5), dict(method=7)):
        assert _call(hip, out, **dict(exact, **kw)) != 0
    torch.cuda.synchronize()
    assert _untouched(out)
    # an empty mesh and an empty query set are valid calls
    empty = dict(_device(case), vertices=None, faces=None, nv=0, nf=0, fstart=torch.zeros(2, dtype=torch.int32, device="cuda"))
    for method in (hip.WIND_EXACT, hip.WIND_CELLS, hip.WIND_AUTO):
        out = _buffers(case.nq, 0)
        assert _call(hip, out, method=method, cells=0, scratch=False, nbytes=0, **empty) == 0
        torch.cuda.synchronize()
        w = out["winding"][:case.nq].cpu().numpy()
        assert np.array_equal(np.isnan(w), ~np.isfinite(case.query).all(1)) and not np.nan_to_num(w).any() and not bool(out["inside"][:case.nq].any())
        out = _buffers(0, nbytes)
        assert _call(hip, out, **dict(good, query=None, nq=0, method=method)) == 0
        torch.cuda.synchronize()
        assert bool((out["winding"] == SENTINEL).all()) and bool((out["inside"] == 77).all())


# ------------------------------------------------------------------------------------------------ 4. host path
def _tri_mesh(case):
    from mvdfusion_amd import fusion
    t = lambda a: torch.from_numpy(a).cuda()
    return fusion.TriangleMesh(vertices=t(case.vertices), faces=t(case.faces), rgb=None, vertex_start=torch.tensor([0, case.nv], dtype=torch.int32),
                               face_start=torch.from_numpy(case.face_start.copy()))


def test_winding_number_is_the_abi_call(hip):
    from mvdfusion_amd import fusion
    case = W.make_case("scenes")
    mesh = _tri_mesh(case)
    scene = torch.from_numpy(np.repeat(np.arange(case.nscene), np.diff(case.query_start))).cuda()
    cloud = fusion.SurfaceSamples(xyz=torch.from_numpy(case.query).cuda(), rgb=None, scene=scene, face=None, bary=None)
    for method, m, cells, beta in (("auto", hip.WIND_AUTO, None, 2.0), ("exact", hip.WIND_EXACT, None, 2.0), ("cells", hip.WIND_CELLS, 7, 3.0)):
        got = fusion.winding_number(cloud, mesh, scenes=case.nscene, method=method, cells=cells, beta=beta)
        want = _run(hip, case, m, cells or 0, beta)
        assert got.value.dtype == torch.float64 and got.inside.dtype == torch.bool and torch.equal(got.scene, scene)
        assert np.array_equal(got.value.cpu().numpy().view(np.int64), _w(want, case.nq).view(np.int64)), method
        assert torch.equal(got.inside, want["inside"][:case.nq].bool()), method
    with pytest.raises(ValueError):
        fusion.winding_number(cloud, mesh, scenes=3)


@pytest.fixture(scope="module")
def spheres():
    """Two marched spheres of radius 0.45 on the G = 24 volume, the second offset by 0.1 along x, and the voxel centres."""
    from mvdfusion_amd import fusion
    G, R = 24, 0.45
    centres = fusion.voxel_centres(G).double()
    meshes = []
    for off in (0.0, 0.1):
        sdf = ((centres - torch.tensor([off, 0.0, 0.0], dtype=torch.float64)).norm(dim=1) - R).reshape(G, G, G)
        meshes.append(fusion.extract_mesh(sdf.float().cuda()))
    return G, R, centres, meshes


def test_voxelize_mesh_and_volume_iou_meet_the_analytic_sphere(hip, spheres):
    from mvdfusion_amd import fusion
    G, R, centres, (m0, m1) = spheres
    diag = math_sqrt3 * 1.5 / G
    vols, truths, clear = [], [], []
    for mesh, off in ((m0, 0.0), (m1, 0.1)):
        d = (centres - torch.tensor([off, 0.0, 0.0], dtype=torch.float64)).norm(dim=1) - R
        vol = fusion.voxelize_mesh(mesh, grid=G)
        assert vol.occupied.shape == (1, G, G, G) and vol.occupied.dtype == torch.bool and vol.center == (0.0, 0.0, 0.0) and vol.half_extent == 0.75
        got, truth, far = vol.occupied.reshape(-1).cpu(), d < 0, d.abs() > diag
        assert torch.equal(got[far], truth[far]) and int(far.sum()) > G ** 3 // 2
        for method, cells in (("exact", None), ("cells", 5)):
            other = fusion.voxelize_mesh(mesh, grid=G, method=method, cells=cells).occupied.reshape(-1).cpu()
            assert torch.equal(other[far], truth[far]), method
        vols.append(vol), truths.append(truth), clear.append(far)
    same = fusion.volume_iou(m0, m0, grid=G)
    assert float(same.iou[0]) == 1.0 and int(same.intersection[0]) == int(same.union[0]) == int(vols[0].occupied.sum()) > 0
    assert same.intersection.dtype == same.union.dtype == torch.int64 and same.iou.dtype == torch.float64
    both = fusion.volume_iou(m0, m1, grid=G)
    again = fusion.volume_iou(vols[0], m1)
    assert torch.equal(both.intersection, again.intersection) and torch.equal(both.union, again.union) and torch.equal(both.iou.cpu(), again.iou.cpu())
    safe = clear[0] & clear[1]
    a, b = vols[0].occupied.reshape(-1).cpu(), vols[1].occupied.reshape(-1).cpu()
    assert int((a & b)[safe].sum()) == int((truths[0] & truths[1])[safe].sum()) and int((a | b)[safe].sum()) == int((truths[0] | truths[1])[safe].sum())
    band = int((~safe).sum())
    analytic = int((truths[0] & truths[1]).sum()) / int((truths[0] | truths[1]).sum())
    print(f"RATIO winding iou | G {G} | band voxels {band} of {G ** 3} | iou {float(both.iou[0]):.6f} analytic on the same voxels {analytic:.6f} | "
          f"intersection {int(both.intersection[0])} union {int(both.union[0])}")
    assert abs(int(both.intersection[0]) - int((truths[0] & truths[1]).sum())) <= band and abs(int(both.union[0]) - int((truths[0] | truths[1]).sum())) <= band
    empty = fusion.OccupancyVolume(occupied=torch.zeros_like(vols[0].occupied), center=vols[0].center, half_extent=vols[0].half_extent)
    none = fusion.volume_iou(empty, empty)
    assert int(none.union[0]) == 0 and bool(torch.isnan(none.iou[0]))


def test_signed_distance_signs_nearest_on_mesh(hip, spheres):
    from mvdfusion_amd import fusion
    G, R, centres, (m0, _) = spheres
    q = (torch.rand(1500, 3, generator=torch.Generator().manual_seed(3)) * 1.2 - 0.6).cuda()
    sd = fusion.signed_distance(q, m0)
    near, wind = fusion.nearest_on_mesh(q, m0), fusion.winding_number(q, m0)
    assert sd.distance.dtype == torch.float32 and torch.equal(sd.distance.abs(), near.dist) and torch.equal(sd.inside, wind.inside)
    assert torch.equal(sd.nearest.face, near.face) and torch.equal(sd.nearest.dist2, near.dist2)
    moving = near.dist > 0
    assert torch.equal((sd.distance < 0)[moving], sd.inside[moving]) and int(sd.inside.sum()) > 100 and int((~sd.inside).sum()) > 100
    r = q.double().norm(dim=1).cpu()
    far = (r - R).abs() > math_sqrt3 * 1.5 / G
    assert torch.equal(sd.inside.cpu()[far], (r < R)[far])
