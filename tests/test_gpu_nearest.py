"""The nearest-point search on the GPU: mvd_nearest_points (csrc/nearest.hip) through the C ABI against the fp32 restatement and the float64
brute force of tests/nearest_f64.py, and the host path (fusion.nearest_points, fusion.compare_geometry).

Bounds -- none taken from what the kernels give:
  index, dist2    EQUAL, bit for bit, to the fp32 restatement of the rule on EVERY query of every case, for MVD_NN_BRUTE, MVD_NN_GRID at
                  grid = 0, 1, 2, 7, 64 and MVD_NN_AUTO.  No query is left out: there is no exclusion cap.
  against float64 on the finite queries with a winner: |dist2 - min_j d2_64| <= 3 * 2^-23 * min_j d2_64 and
                  d2_64(i, index[i]) <= (1 + 6 * 2^-23) * min_j d2_64 (nearest_f64.float64_bounds has the derivation).
  determinism, stages: bit equality.  Refusals: non-zero, the function's name in mvd_last_error(), nothing written.
  host path       identical clouds: zeros and fscore 1; a copy shifted by delta: every distance <= delta (1 + 2^-20) -- the point's own
                  copy is a candidate at exactly the shift (both clouds on the fp32 lattice of 2^-23), d2 and the square root round once.

Measured on an MI355X: no mismatch on any query of the ten inputs for any method; against float64 at most 1.34 x 2^-23 (dist2) and
0.05 x 2^-23 (winner) -- the restatement's own figures, the bits being equal.  Shifted copy: 5 568 points, largest distance 0.010000,
chamfer 0.018696, precision 0.003 at delta / 4.
"""
import ctypes

import pytest
import torch

import fusion_f64 as F
import nearest_f64 as NN

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
GRIDS = (0, 1, 2, 7, 64)


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


def _device(case):
    i32 = lambda t: t.to(torch.int32).contiguous().cuda()
    return dict(query=case.query.contiguous().cuda(), qstart=i32(case.query_start), target=case.target.contiguous().cuda(),
                tstart=i32(case.target_start), nq=case.nq, nt=case.nt, nscene=case.nscene)


def _buffers(nq, nbytes):
    return dict(index=torch.full((max(nq, 1),), -5, dtype=torch.int32, device="cuda"), dist2=torch.full((max(nq, 1),), SENTINEL, device="cuda"),
                scratch=torch.full((max((nbytes + 7) // 8, 2),), 0x1234, dtype=torch.int64, device="cuda"))


def _untouched(out):
    return bool((out["index"] == -5).all()) and bool((out["dist2"] == SENTINEL).all()) and bool((out["scratch"] == 0x1234).all())


def _call(hip, out, query, qstart, target, tstart, nq, nt, nscene, method, grid, index=True, dist2=True, scratch=True, nbytes=None, stages=None,
          scratch_offset=0):
    p = hip.ptr
    nbytes = out["scratch"].numel() * 8 if nbytes is None else nbytes
    sc = ctypes.c_void_p(out["scratch"].data_ptr() + scratch_offset) if scratch else None
    args = [p(query), p(qstart), p(target), p(tstart), nq, nt, nscene, method, grid, p(out["index"]) if index else None,
            p(out["dist2"]) if dist2 else None, sc, nbytes]
    if stages is None:
        return hip.lib().mvd_nearest_points(*args, hip.stream())
    return hip.lib().mvd_nearest_points_stages(*args, stages, hip.stream())


def _search(hip, case, method, grid=0, stages=(None,), out=None):
    """mvd_nearest_points (or the given stage calls, in order) with the outputs and the scratch pre-filled."""
    nbytes = int(hip.lib().mvd_nearest_points_scratch(case.nt, case.nscene, method, grid))
    out = _buffers(case.nq, nbytes) if out is None else out
    dev = _device(case)
    for st in stages:
        hip.check(_call(hip, out, method=method, grid=grid, nbytes=nbytes, stages=st, **dev))
    torch.cuda.synchronize()
    return out


def _equal(ref, out, nq):
    index, dist2 = out["index"][:nq].cpu(), out["dist2"][:nq].cpu()
    return torch.equal(index.long(), ref.index) and torch.equal(dist2.view(torch.int32), ref.dist2.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1, 2. parity
@pytest.mark.parametrize("name", list(NN.CASES))
def test_every_method_gives_the_bits_of_the_rule(hip, name):
    ref = NN.refs(name)
    case = ref.case
    runs = [("brute", hip.NN_BRUTE, 0), ("auto", hip.NN_AUTO, 0)] + [(f"grid{g}", hip.NN_GRID, g) for g in GRIDS]
    wrong = {}
    for label, method, grid in runs:
        out = _search(hip, case, method, grid)
        index, dist2 = out["index"][:case.nq].cpu(), out["dist2"][:case.nq].cpu()
        bad = (index.long() != ref.index) | (dist2.view(torch.int32) != ref.dist2.view(torch.int32))
        if bool(bad.any()):
            i = int(torch.nonzero(bad)[0])
            wrong[label] = (int(bad.sum()), i, int(index[i]), float(dist2[i]), int(ref.index[i]), float(ref.dist2[i]))
        ok, w1, w2 = NN.float64_bounds(ref, index.long(), dist2)
        print(f"RATIO nearest {name} {label} | nq {case.nq} nt {case.nt} scenes {case.nscene} mismatches {int(bad.sum())} | float64: dist2 "
              f"{w1:.2f} x 2^-23 (bound 3), winner {w2:.2f} x 2^-23 (bound 6) | hit {float((index >= 0).float().mean()):.3f}")
        assert ok, (label, w1, w2)
    assert not wrong, wrong
    if name == "three_scenes":
        index = _search(hip, case, hip.NN_GRID, 7)["index"].cpu()
        assert bool((index[:50] == -1).all()) and bool((index[50:] >= 1).all())          # scene 0 has queries and no target


# ------------------------------------------------------------------------------------------------ 3. every element, determinism, stages
@pytest.mark.parametrize("name", ["duplicates", "nonfinite", "three_scenes"])
def test_outputs_are_fully_written_identical_run_to_run_and_the_stages_compose(hip, name):
    ref = NN.refs(name)
    case = ref.case
    for method, grid in ((hip.NN_BRUTE, 0), (hip.NN_GRID, 7), (hip.NN_GRID, 0)):
        one, again = _search(hip, case, method, grid), _search(hip, case, method, grid)
        assert not bool((one["index"][:case.nq] == -5).any()) and not bool((one["dist2"][:case.nq] == SENTINEL).any())
        for k in ("index", "dist2"):
            assert torch.equal(one[k].view(torch.int32), again[k].view(torch.int32)), k
        built = _search(hip, case, method, grid, stages=(hip.NN_BUILD,))
        assert bool((built["index"] == -5).all()) and bool((built["dist2"] == SENTINEL).all())          # nothing queried yet
        staged = _search(hip, case, method, grid, stages=(hip.NN_QUERY,), out=built)
        both = _search(hip, case, method, grid, stages=(hip.NN_BUILD, hip.NN_QUERY))
        for k in ("index", "dist2"):
            assert torch.equal(one[k].view(torch.int32), staged[k].view(torch.int32)) and torch.equal(one[k].view(torch.int32), both[k].view(torch.int32)), k
        assert _equal(ref, one, case.nq)


def test_empty_sides_are_valid_calls(hip):
    case = NN.make_case("random")
    dev = _device(case)
    for method in (hip.NN_BRUTE, hip.NN_GRID, hip.NN_AUTO):
        out = _buffers(case.nq, 0)
        empty = dict(dev, target=None, nt=0, tstart=torch.zeros(2, dtype=torch.int32, device="cuda"))
        assert int(hip.lib().mvd_nearest_points_scratch(0, 1, method, 0)) == 0
        assert _call(hip, out, method=method, grid=0, scratch=False, nbytes=0, **empty) == 0
        torch.cuda.synchronize()
        assert bool((out["index"] == -1).all()) and bool(torch.isposinf(out["dist2"]).all())
        out = _buffers(4, int(hip.lib().mvd_nearest_points_scratch(case.nt, 1, method, 0)))
        none = dict(dev, query=None, nq=0, qstart=torch.zeros(2, dtype=torch.int32, device="cuda"))
        assert _call(hip, out, method=method, grid=0, index=False, dist2=False, **none) == 0
        torch.cuda.synchronize()
        assert bool((out["index"] == -5).all()) and bool((out["dist2"] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_bad_arguments_return_an_error_and_write_nothing(hip):
    L = hip.lib()
    case = NN.make_case("random")
    nbytes = int(L.mvd_nearest_points_scratch(case.nt, 1, hip.NN_GRID, 7))
    assert nbytes >= case.nt * 16 + 7 ** 3 * 4
    for args in ((0, 1, hip.NN_GRID, 7), (case.nt, 0, hip.NN_GRID, 7), (case.nt, -1, hip.NN_GRID, 7), (case.nt, 1, -1, 7), (case.nt, 1, 3, 7),
                 (case.nt, 1, hip.NN_GRID, -1), (case.nt, 1, hip.NN_GRID, 257), (case.nt, 65536, hip.NN_GRID, 7), (case.nt, 65535, hip.NN_GRID, 256)):
        assert int(L.mvd_nearest_points_scratch(*args)) == 0, args
    assert int(L.mvd_nearest_points_scratch(case.nt, 1, hip.NN_BRUTE, 0)) == 0          # the brute kernel needs none
    good = dict(_device(case), method=hip.NN_GRID, grid=7, nbytes=nbytes)
    out = _buffers(case.nq, nbytes)
    bad = [dict(query=None), dict(qstart=None), dict(target=None), dict(tstart=None), dict(index=False), dict(dist2=False), dict(scratch=False),
           dict(method=3), dict(method=-1), dict(grid=-1), dict(grid=257), dict(nscene=0), dict(nscene=-1), dict(nscene=65536),
           dict(nscene=65535, grid=256, nbytes=1 << 62),                                 # 2^40 cells
           dict(nq=1 << 31), dict(nt=1 << 31, nbytes=1 << 62),
           dict(nbytes=nbytes - 16), dict(nbytes=0), dict(scratch_offset=8, nbytes=nbytes)]
    for stages in (None, hip.NN_QUERY):
        for kw in bad:
            a = dict(good)
            a.update(kw)
            assert _call(hip, out, stages=stages, **a) != 0, kw
            assert (b"mvd_nearest_points_stages" if stages else b"mvd_nearest_points:") in L.mvd_last_error(), (kw, L.mvd_last_error())
    for stages in (0, 4, -1):
        assert _call(hip, out, stages=stages, **good) != 0 and b"mvd_nearest_points_stages" in L.mvd_last_error()
    torch.cuda.synchronize()
    assert _untouched(out)


# ------------------------------------------------------------------------------------------------ 5. host path
@pytest.fixture(scope="module")
def sphere_cloud():
    from mvdfusion_amd import fusion
    case = F.sphere_case()
    return case, fusion.fuse_views(case.lat.cuda(), case.cams)


def test_identical_clouds_are_at_distance_zero(hip, sphere_cloud):
    from mvdfusion_amd import fusion
    _, cloud = sphere_cloud
    n = len(cloud)
    assert n > 1000
    for method in ("auto", "brute", "grid"):
        d = fusion.compare_geometry(cloud, cloud, method=method)
        for k in ("accuracy", "completeness", "chamfer", "chamfer_sq"):
            assert getattr(d, k).shape == (1,) and getattr(d, k).dtype == torch.float64 and float(getattr(d, k)) == 0.0, k
        assert float(d.precision) == float(d.recall) == float(d.fscore) == 1.0
        assert bool((d.a_to_b.dist2 == 0).all()) and bool(d.a_to_b.hit.all()) and d.a_to_b.index.dtype == torch.int32
        # where the cloud has no duplicate point the nearest point is the point itself; a duplicate finds its first copy
        uniq, inverse, counts = torch.unique(cloud.xyz, dim=0, return_inverse=True, return_counts=True)
        single = counts[inverse] == 1
        rows = torch.arange(n, device="cuda", dtype=torch.int32)
        assert bool(single.any()) and torch.equal(d.a_to_b.index[single], rows[single]) and bool((d.a_to_b.index <= rows).all())
        assert torch.equal(cloud.xyz[d.a_to_b.index.long()], cloud.xyz)


def test_a_shifted_copy_is_at_most_the_shift_away(hip, sphere_cloud):
    """delta = 0.01 along z.  So that the bound is about the search and not about the rounding of z + delta (half an ulp of z is up to
    3e-6 of delta), both clouds live on the fp32 lattice of 2^-23: z is rounded to it and the shift is floor(delta 2^23) 2^-23 =
    delta (1 - 9.5e-7), exact in fp32 on both sides.  A point's own copy is then a candidate at exactly that distance; d2 and the square
    root round once each (2^-24 relative), so every distance is <= delta (1 + 2^-20)."""
    from mvdfusion_amd import fusion
    import dataclasses
    _, cloud = sphere_cloud
    delta = 0.01
    step = float(int(delta * 2 ** 23)) / 2 ** 23
    xyz = cloud.xyz.clone()
    xyz[:, 2] = torch.round(xyz[:, 2] * 2 ** 23) / 2 ** 23
    assert float(xyz.abs().max()) < 0.99
    cloud = dataclasses.replace(cloud, xyz=xyz)
    moved = dataclasses.replace(cloud, xyz=xyz + torch.tensor([0.0, 0.0, step], device="cuda"))
    assert bool(((moved.xyz[:, 2].double() - xyz[:, 2].double()) == step).all())
    cap = delta * (1 + 2.0 ** -20)
    d = fusion.compare_geometry(cloud, moved, threshold=0.011)
    for side in (d.a_to_b, d.b_to_a):
        assert bool(side.hit.all()) and float(side.dist.max()) <= cap and float(side.dist.max()) > 0
    assert float(d.chamfer) <= 2 * cap and float(d.accuracy) <= cap and float(d.completeness) <= cap and float(d.chamfer) > 0
    assert float(d.precision) == float(d.recall) == float(d.fscore) == 1.0
    tight = fusion.compare_geometry(cloud, moved, threshold=delta / 4)
    assert float(tight.precision) < 1.0 and float(tight.recall) < 1.0
    assert torch.equal(tight.a_to_b.dist2, d.a_to_b.dist2)
    print(f"shifted copy: {len(cloud)} points, delta {delta}, max dist {float(d.a_to_b.dist.max()):.6f}, chamfer {float(d.chamfer):.6f}, "
          f"precision at delta / 4 {float(tight.precision):.3f}")


def test_two_scenes_equal_the_two_single_scene_results(hip, sphere_cloud):
    from mvdfusion_amd import fusion
    case, cloud = sphere_cloud
    other = F.sphere_case(pull_view=2)
    both = fusion.fuse_views(torch.stack([case.lat, other.lat]).cuda(), [case.cams, other.cams])
    second = fusion.fuse_views(other.lat.cuda(), other.cams)
    assert int((both.scene == 0).sum()) == len(cloud) and int((both.scene == 1).sum()) == len(second)
    shift = torch.tensor([0.004, -0.003, 0.005], device="cuda")
    import dataclasses
    move = lambda c: dataclasses.replace(c, xyz=c.xyz + shift)
    d2 = fusion.compare_geometry(both, move(both), scenes=2, threshold=0.007)
    singles = [fusion.compare_geometry(c, move(c), threshold=0.007) for c in (cloud, second)]
    n0 = len(cloud)
    for k in ("accuracy", "completeness", "chamfer", "chamfer_sq", "precision", "recall", "fscore"):
        assert getattr(d2, k).shape == (2,)
        assert torch.equal(getattr(d2, k), torch.cat([getattr(s, k) for s in singles])), k
    for side in ("a_to_b", "b_to_a"):
        got = getattr(d2, side)
        assert torch.equal(got.dist2, torch.cat([getattr(s, side).dist2 for s in singles]))
        assert torch.equal(got.index, torch.cat([singles[0].a_to_b.index if side == "a_to_b" else singles[0].b_to_a.index,
                                                 (singles[1].a_to_b.index if side == "a_to_b" else singles[1].b_to_a.index) + n0]))
    # a cloud against the other scene's: scene ids decide who meets whom
    cross = fusion.nearest_points(both, dataclasses.replace(both, scene=1 - both.scene.flip(0), xyz=both.xyz.flip(0)), scenes=2)
    assert bool(cross.hit.all()) and bool((cross.index[:n0] < len(second)).all()) and bool((cross.index[n0:] >= len(second)).all())
