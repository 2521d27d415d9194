"""The neighbourhood entries on the GPU: mvd_knn_points and mvd_point_normals (csrc/nearest.hip, csrc/normals.hip) through the C ABI
against the restatements of tests/knn_f64.py, and the host path (fusion.knn_points, fusion.estimate_normals, fusion.sample_normals).

Bounds -- none taken from what the kernels give:
  k nearest       index and dist2 EQUAL, bit for bit, on every slot of every query to the fp32 restatement of the rule, for k = 1, 3, 8,
                  16, 32, MVD_NN_BRUTE and MVD_NN_GRID at grid = 1, 7 and the library's choice, on the ten inputs of the nearest-point
                  tests and three of this feature's own (a noisy sphere against itself, four scenes of 700 / 2 / 0 / 1301 points, scenes
                  with fewer targets than k).  No query is left out.  k = 1: the bits of mvd_nearest_points.  Determinism, stages, a grid
                  built by the other search, a scene alone against the batch: bit equality.  Refusals: non-zero, the entry's name in
                  mvd_last_error(), nothing written.
  normals         fed the ORACLE's neighbour lists.  Up to sign, per component: 64 * 2^-53 * l2 / (l1 - l0) + 2^-24
                  (knn_f64.normal_bound has the derivation) on every valid point with (l1 - l0) / l2 >= 2^-10 -- every valid point of
                  every case, as test_cpu_knn.py asserts on the oracle alone.  variation: 16 * 2^-53 * l2 / (l0 + l1 + l2) + 2^-24
                  relative-to-one (an eigenvalue of a backward-stable solver moves by at most ~8 * 2^-53 * l2, two solvers; the quotient
                  is at most 1 / 3 and is rounded to fp32 once).  valid EQUAL to the oracle's on every point.  The sign rule wherever the
                  two largest magnitudes of the oracle's normal differ by more than twice the bound.  Lattice plane: exactly (0, 0, 1)
                  and exactly 0.  Analytic surfaces: the angle to the true normal at most 2 x the oracle's own largest angle on the case
                  (sphere 0.1045 rad, ellipsoid 0.1416 rad at 16 neighbours: the estimator's error, not the kernel's).
  sample_normals  the float64 cross product of the face, rounded to fp32 once per component: 2^-24.

Measured on an MI355X: no mismatch on any slot of the thirteen inputs for any k and method; normals at most 0.500 of the bound (the
fp32 rounding of the output), variation at most 0.219 of its bound (the `uniform` input), | |n| - 1 | at most 4.5e-8; the largest angle
to the analytic normal 0.104476 rad (sphere) and 0.141627 rad (ellipsoid), the oracle's own figures to the digit.
"""
import ctypes

import numpy as np
import pytest
import torch

import knn_f64 as K
import raster_f64 as R

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
GRIDS = (1, 7, 0)


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


def _device(case):
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).contiguous().cuda()
    return dict(query=dev(case.query, torch.float32), qstart=dev(case.query_start, torch.int32), target=dev(case.target, torch.float32),
                tstart=dev(case.target_start, torch.int32), nq=case.nq, nt=case.nt, nscene=case.nscene)


def _buffers(nq, k, nbytes):
    return dict(index=torch.full((max(nq, 1), k), -5, dtype=torch.int32, device="cuda"),
                dist2=torch.full((max(nq, 1), k), SENTINEL, device="cuda"),
                scratch=torch.full((max((nbytes + 7) // 8, 2),), 0x1234, dtype=torch.int64, device="cuda"))


def _untouched(out):
    return bool((out["index"] == -5).all()) and bool((out["dist2"] == SENTINEL).all()) and bool((out["scratch"] == 0x1234).all())


def _call(hip, out, query, qstart, target, tstart, nq, nt, nscene, k, method, grid, nbytes=None, stages=None, scratch=True, scratch_offset=0,
          index_offset=0, nearest=False):
    p = hip.ptr
    nbytes = out["scratch"].numel() * 8 if nbytes is None else nbytes
    sc = ctypes.c_void_p(out["scratch"].data_ptr() + scratch_offset) if scratch else None
    head = [p(query), p(qstart), p(target), p(tstart), nq, nt, nscene]
    tail = [method, grid, ctypes.c_void_p(out["index"].data_ptr() + index_offset), p(out["dist2"]), sc, nbytes]
    L = hip.lib()
    if nearest:
        return L.mvd_nearest_points_stages(*head, *tail, hip.NN_ALL if stages is None else stages, hip.stream())
    if stages is None:
        return L.mvd_knn_points(*head, k, *tail, hip.stream())
    return L.mvd_knn_points_stages(*head, k, *tail, stages, hip.stream())


def _search(hip, case, k, method, grid=0, stages=(None,), out=None, nearest=()):
    """mvd_knn_points (or the given stage calls in order; those listed in `nearest` go to mvd_nearest_points_stages) on pre-filled buffers."""
    nbytes = int(hip.lib().mvd_nearest_points_scratch(case.nt, case.nscene, method, grid))
    out = _buffers(case.nq, k, nbytes) if out is None else out
    dev = _device(case)
    for n, st in enumerate(stages):
        hip.check(_call(hip, out, k=k, method=method, grid=grid, nbytes=nbytes, stages=st, nearest=n in nearest, **dev))
    torch.cuda.synchronize()
    return out


def _bits(out, nq):
    return out["index"][:nq].cpu().numpy(), out["dist2"][:nq].cpu().numpy().view(np.int32)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", K.CASES)
def test_every_k_and_method_gives_the_bits_of_the_rule(hip, name):
    case = K.make_case(name)
    ref_i, ref_d = K.refs(name)
    runs = [("brute", hip.NN_BRUTE, 0)] + [(f"grid{g}", hip.NN_GRID, g) for g in GRIDS]
    wrong = {}
    for k in K.KS:
        want_i, want_d = ref_i[:, :k], np.ascontiguousarray(ref_d[:, :k]).view(np.int32)
        for label, method, grid in runs:
            index, dist2 = _bits(_search(hip, case, k, method, grid), case.nq)
            bad = (index != want_i) | (dist2 != want_d)
            if bad.any():
                i, s = np.argwhere(bad)[0]
                wrong[(k, label)] = (int(bad.sum()), int(i), int(s), int(index[i, s]), int(want_i[i, s]))
        print(f"RATIO knn {name} k {k} | nq {case.nq} nt {case.nt} scenes {case.nscene} slots {case.nq * k} filled "
              f"{float((want_i >= 0).mean()):.3f} | mismatches {sum(v[0] for key, v in wrong.items() if key[0] == k)}")
    assert not wrong, wrong


def test_k_1_is_the_nearest_point_search(hip):
    for name in ("random", "duplicates", "nonfinite", "three_scenes", "four_scenes"):
        case = K.make_case(name)
        for method, grid in ((hip.NN_BRUTE, 0), (hip.NN_GRID, 7), (hip.NN_AUTO, 0)):
            one = _search(hip, case, 1, method, grid)
            nn = _search(hip, case, 1, method, grid, nearest=(0,))
            assert all(np.array_equal(a, b) for a, b in zip(_bits(one, case.nq), _bits(nn, case.nq))), (name, method, grid)


# ------------------------------------------------------------------------------------------------ 2. determinism, stages, scenes
@pytest.mark.parametrize("name", ["duplicates", "sphere_self", "four_scenes"])
def test_two_runs_the_stages_and_a_grid_of_the_other_search_give_equal_bits(hip, name):
    case = K.make_case(name)
    k = 16
    for method, grid in ((hip.NN_BRUTE, 0), (hip.NN_GRID, 7), (hip.NN_GRID, 0)):
        one, again = _search(hip, case, k, method, grid), _search(hip, case, k, method, grid)
        assert not bool((one["index"][:case.nq] == -5).any()) and not bool((one["dist2"][:case.nq] == SENTINEL).any())          # every element
        same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(_bits(a, case.nq), _bits(b, case.nq)))
        assert same(one, again)
        built = _search(hip, case, k, method, grid, stages=(hip.NN_BUILD,))
        assert bool((built["index"] == -5).all()) and bool((built["dist2"] == SENTINEL).all())          # nothing queried yet
        assert same(one, _search(hip, case, k, method, grid, stages=(hip.NN_QUERY,), out=built))
        # the grid that mvd_nearest_points_stages builds serves this query
        assert same(one, _search(hip, case, k, method, grid, stages=(hip.NN_BUILD, hip.NN_QUERY), nearest=(0,)))


def test_a_scene_alone_gives_the_bits_it_gives_in_the_batch(hip):
    case = K.make_case("four_scenes")
    for k, method, grid in ((8, hip.NN_BRUTE, 0), (32, hip.NN_GRID, 0), (3, hip.NN_GRID, 7)):
        batch_i, batch_d = _bits(_search(hip, case, k, method, grid), case.nq)
        for s in range(case.nscene):
            alone, t0 = K.scene_case(case, s)
            q0, q1 = int(case.query_start[s]), int(case.query_start[s + 1])
            if q1 == q0:
                continue
            i, d = _bits(_search(hip, alone, k, method, grid), alone.nq)
            assert np.array_equal(np.where(i >= 0, i + t0, -1), batch_i[q0:q1]) and np.array_equal(d, batch_d[q0:q1]), (k, method, s)


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_bad_arguments_return_an_error_and_write_nothing(hip):
    L = hip.lib()
    case = K.make_case("random")
    k = 8
    nbytes = int(L.mvd_nearest_points_scratch(case.nt, 1, hip.NN_GRID, 7))
    good = dict(_device(case), k=k, method=hip.NN_GRID, grid=7, nbytes=nbytes)
    out = _buffers(case.nq, k, nbytes)
    bad = [dict(k=0), dict(k=33), dict(k=-1), dict(nbytes=nbytes - 16), dict(nbytes=0), dict(scratch=False), dict(scratch_offset=8),
           dict(index_offset=2), dict(nscene=0), dict(nscene=-1), dict(nscene=65536), dict(method=3), dict(grid=257), dict(query=None),
           dict(qstart=None), dict(target=None), dict(tstart=None), dict(nq=1 << 31), dict(nt=1 << 31, nbytes=1 << 62)]
    for stages in (None, hip.NN_QUERY):
        for kw in bad:
            a = dict(good)
            a.update(kw)
            assert _call(hip, out, stages=stages, **a) != 0, kw
            assert (b"mvd_knn_points_stages" if stages else b"mvd_knn_points:") in L.mvd_last_error(), (kw, L.mvd_last_error())
    for stages in (0, 4, -1):
        assert _call(hip, out, stages=stages, **good) != 0 and b"mvd_knn_points_stages" in L.mvd_last_error()
    torch.cuda.synchronize()
    assert _untouched(out)
    # an empty target side is a valid call: every slot empty
    empty = dict(_device(case), target=None, nt=0, tstart=torch.zeros(2, dtype=torch.int32, device="cuda"))
    for method in (hip.NN_BRUTE, hip.NN_GRID, hip.NN_AUTO):
        out = _buffers(case.nq, k, 0)
        assert _call(hip, out, k=k, method=method, grid=0, scratch=False, nbytes=0, **empty) == 0
        torch.cuda.synchronize()
        assert bool((out["index"] == -1).all()) and bool(torch.isposinf(out["dist2"]).all())


# ------------------------------------------------------------------------------------------------ 4. host path
def test_knn_points_on_a_cloud_with_scenes(hip):
    from mvdfusion_amd import fusion
    case = K.make_case("four_scenes")
    ref_i, ref_d = K.refs("four_scenes")
    xyz = torch.from_numpy(case.query).cuda()
    scene = torch.from_numpy(np.repeat(np.arange(4), np.diff(case.query_start))).cuda()
    z = torch.zeros(case.nq, dtype=torch.int64, device="cuda")
    cloud = fusion.PointCloud(xyz=xyz, rgb=None, support=z.to(torch.uint8), scene=scene, view=z, pixel=torch.zeros(case.nq, 2, dtype=torch.int64),
                              index=z.to(torch.int32))
    for k, method in ((16, "auto"), (5, "brute"), (32, "grid")):
        out = fusion.knn_points(cloud, cloud, k, scenes=4, method=method)
        assert out.index.shape == out.dist2.shape == (case.nq, k) and out.index.dtype == torch.int32 and out.dist2.dtype == torch.float32
        assert np.array_equal(out.index.cpu().numpy(), ref_i[:, :k]) and np.array_equal(out.dist2.cpu().numpy(), ref_d[:, :k])
        count = out.count.cpu().numpy()
        assert np.array_equal(count, (ref_i[:, :k] >= 0).sum(1)) and count[700] == 2 and count[0] == k          # the scene of two points
        assert torch.equal(out.hit, out.index >= 0) and torch.equal(out.dist, out.dist2.sqrt())
        # a point is its own neighbour 0 at distance 0 and stays in the list
        rows = torch.arange(case.nq, dtype=torch.int32, device="cuda")
        assert torch.equal(out.index[:, 0], rows) and bool((out.dist2[:, 0] == 0).all())
    one = fusion.knn_points(xyz[:700], xyz[:700], 1)
    nn = fusion.nearest_points(xyz[:700], xyz[:700])
    assert torch.equal(one.index[:, 0], nn.index) and torch.equal(one.dist2[:, 0], nn.dist2)


# ------------------------------------------------------------------------------------------------ 5. normals
def _normals(hip, case, toward=None, sentinel=True):
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).contiguous().cuda()
    target, index, points = dev(case.target, torch.float32), dev(case.index, torch.int32), dev(case.points, torch.float32)
    n, k = case.index.shape
    normal = torch.full((n, 3), SENTINEL, device="cuda")
    variation = torch.full((n,), SENTINEL, device="cuda")
    tw = None if toward is None else dev(toward, torch.float32)
    hip.check(hip.lib().mvd_point_normals(hip.ptr(target), case.target.shape[0], hip.ptr(index), n, k, hip.ptr(points) if tw is not None else None,
                                          hip.ptr(tw), hip.ptr(normal), hip.ptr(variation), hip.stream()))
    torch.cuda.synchronize()
    return normal.cpu().numpy(), variation.cpu().numpy()


@pytest.mark.parametrize("name", list(K.NORMAL_CASES))
def test_normals_meet_the_float64_oracle_on_its_own_neighbour_lists(hip, name):
    ref = K.normal_refs(name)
    case = ref.case
    normal, variation = _normals(hip, case)
    assert not (normal == SENTINEL).any() and not (variation == SENTINEL).any()          # every element is written
    valid = ~np.isnan(variation)
    assert np.array_equal(valid, ref.valid)
    assert not normal[~valid].any() and np.array_equal(np.isnan(variation), ~ref.valid)          # invalid: the zero normal, NaN
    keep, bound = ref.compared, K.normal_bound(ref)
    n64 = normal.astype(np.float64)
    err = np.minimum(np.abs(n64 - ref.normal).max(1), np.abs(n64 + ref.normal).max(1))
    vbound = 16 * 2.0 ** -53 * ref.lam[:, 2] / np.where(valid, ref.lam.sum(1), 1.0) + 2.0 ** -24
    verr = np.abs(variation.astype(np.float64) - ref.variation)
    length = np.abs(np.linalg.norm(n64[valid], axis=1) - 1.0).max()
    print(f"RATIO normals {name} | points {valid.size} valid {int(valid.sum())} compared {int(keep.sum())} | worst error / bound "
          f"{float((err[keep] / bound[keep]).max()):.3f}, variation {float((verr[valid] / vbound[valid]).max()):.3f} | |length - 1| {length:.2e}")
    assert (err[keep] <= bound[keep]).all() and (verr[valid] <= vbound[valid]).all() and length <= 4 * 2.0 ** -24
    # the sign rule, wherever the oracle's two largest magnitudes are further apart than the two results can differ
    mag = np.sort(np.abs(ref.normal), axis=1)
    clear = keep & (mag[:, 2] - mag[:, 1] > 2 * bound)
    assert clear.any() and (np.abs(n64 - ref.normal).max(1)[clear] <= bound[clear]).all()
    lead = np.take_along_axis(n64, np.argmax(np.abs(ref.normal), axis=1)[:, None], axis=1)[:, 0]
    assert (lead[clear] > 0).all()
    again, again_v = _normals(hip, case)
    assert np.array_equal(normal.view(np.int32), again.view(np.int32)) and np.array_equal(variation.view(np.int32), again_v.view(np.int32))
    if name == "lattice_plane":
        assert valid.all() and (normal == np.array([0.0, 0.0, 1.0], dtype=np.float32)).all() and (variation == 0).all()
    if name == "odd_rows":
        assert valid.tolist() == [False] * 5 + [True] * 3 and normal[5].tolist() == [0.0, 0.0, 1.0] and variation[5] == 0
    if case.truth is not None and name != "lattice_plane":
        own, got = K.angle_to(ref.normal[keep], case.truth[keep]).max(), K.angle_to(n64[keep], case.truth[keep]).max()
        print(f"  angle to the analytic normal: oracle {own:.6f} rad, kernel {got:.6f} rad")
        assert got <= 2 * own


def test_toward_turns_the_normals_of_a_sphere_outward_and_inward(hip):
    ref = K.normal_refs("sphere")
    case = ref.case
    plain, _ = _normals(hip, case)
    p = case.points.astype(np.float64)
    outward, v_out = _normals(hip, case, toward=(10.0 * case.points))
    inward, _ = _normals(hip, case, toward=np.zeros_like(case.points))
    assert ((outward.astype(np.float64) * p).sum(1) > 0.5).all() and ((inward.astype(np.float64) * p).sum(1) < -0.5).all()
    assert np.array_equal(outward, -inward) and np.array_equal(np.abs(outward), np.abs(plain))          # a sign, nothing else
    # one viewpoint outside: n . (toward - p) >= 0 in float64 wherever it is not within rounding of 0
    eye = np.array([2.0, -1.0, 0.5], dtype=np.float32)
    seen, _ = _normals(hip, case, toward=np.tile(eye, (p.shape[0], 1)))
    side = (seen.astype(np.float64) * (eye.astype(np.float64) - p)).sum(1)
    assert (side >= -2.0 ** -20).all() and np.array_equal(np.abs(seen), np.abs(plain))


def test_estimate_normals_and_the_refusals(hip):
    from mvdfusion_amd import fusion
    L = hip.lib()
    ref = K.normal_refs("ellipsoid")
    case = ref.case
    xyz = torch.from_numpy(case.points).cuda()
    out = fusion.estimate_normals(xyz, k=16)
    assert out.normal.shape == (xyz.shape[0], 3) and out.variation.shape == out.valid.shape == (xyz.shape[0],) and out.valid.dtype == torch.bool
    assert np.array_equal(out.neighbours.index.cpu().numpy(), case.index)          # the search gives the oracle's lists ...
    direct, direct_v = _normals(hip, case)
    assert np.array_equal(out.normal.cpu().numpy(), direct) and np.array_equal(out.variation.cpu().numpy(), direct_v) and bool(out.valid.all())
    reused = fusion.estimate_normals(xyz, neighbours=out.neighbours, toward=torch.zeros(1, 3))          # one viewpoint per scene: the centre
    assert torch.equal(reused.normal.abs(), out.normal.abs()) and bool(((reused.normal * xyz).sum(1) < 0).all())
    per_point = fusion.estimate_normals(xyz, neighbours=out.neighbours, toward=(10 * xyz))
    assert torch.equal(per_point.normal, -reused.normal)
    # refusals of the entry: non-zero, its name, nothing written
    t, idx = xyz.contiguous(), out.neighbours.index.contiguous()
    normal, variation = torch.full((xyz.shape[0], 3), SENTINEL, device="cuda"), torch.full((xyz.shape[0],), SENTINEL, device="cuda")
    p = hip.ptr
    good = dict(target=p(t), nt=t.shape[0], index=p(idx), n=idx.shape[0], k=16, points=None, toward=None, normal=p(normal), variation=p(variation))
    for kw in (dict(k=0), dict(k=257), dict(target=None), dict(index=None), dict(normal=None), dict(variation=None), dict(toward=p(t)),
               dict(nt=1 << 31), dict(n=1 << 31), dict(normal=ctypes.c_void_p(normal.data_ptr() + 2))):
        a = dict(good)
        a.update(kw)
        assert L.mvd_point_normals(*a.values(), hip.stream()) != 0 and b"mvd_point_normals" in L.mvd_last_error(), kw
    torch.cuda.synchronize()
    assert bool((normal == SENTINEL).all()) and bool((variation == SENTINEL).all())


def test_sample_normals_are_the_face_normals(hip):
    from mvdfusion_amd import fusion
    sv, sf = R.sphere_mesh(8)
    mesh = fusion.TriangleMesh(vertices=sv.float().cuda(), faces=sf.to(torch.int32).cuda(), rgb=None,
                               vertex_start=torch.tensor([0, sv.shape[0]], dtype=torch.int32), face_start=torch.tensor([0, sf.shape[0]], dtype=torch.int32))
    samples = fusion.sample_mesh(mesh, 3000)
    got = fusion.sample_normals(mesh, samples)
    assert got.shape == (3000, 3) and got.dtype == torch.float32 and got.is_cuda
    tri = sv.float().double()[sf.long()[samples.face.cpu().long()]]
    want = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    want = want / want.norm(dim=1, keepdim=True)
    assert float((got.cpu().double() - want).abs().max()) <= 2.0 ** -24
    assert float((got.cpu().double() * samples.xyz.cpu().double()).sum(1).min()) > 0          # the raster tests' sphere winds outward
