"""The global registration on the GPU: mvd_register_score and mvd_register_select (csrc/register.hip) through the C ABI against the float64
oracle of tests/register_f64.py, and the host path fusion.register_geometry.

Bounds -- none taken from what the kernels give:
  inliers         EQUAL to the oracle's count on every (scene, hypothesis): the apply rule and the search are specified to the bit and
                  the comparison with trunc2 is in fp32.
  score           |score - oracle| <= (n 2^-53 + 2^-52) * oracle, n the rows of the scene: every addend is an exact fp32 value >= 0, only
                  the n - 1 additions of the sum round (2^-53 relative each, in whatever order), and the oracle is math.fsum, correctly
                  rounded (half of 2^-52).  A scene without rows scores exactly 0.
  grid / brute / auto, run to run: the same bits.
  far hypotheses  exactly n * trunc2 (n <= 2^13 copies of one 24-bit value: exact in fp64 in any order) and 0 inliers.
  cross-check     against mvd_align_apply + mvd_nearest_points + torch where / sum in fp64 on 20 000 rows per call: inliers equal, score
                  within twice the bound (both sums round).
  select          EQUAL to the greedy rule in numpy (tests/register_f64.py: select), top and top_score.
  end to end      four poses of the table (tests/register_f64.py: GPU_POSES; the oracle recovers all 27, tests/test_cpu_register.py) as one
                  4-scene batch: final correspondences = the permutation on EVERY point; |matrix - truth| <= 2^-20 (test_gpu_align's ICP
                  bound: the fp32 rounding of both point sets, 2 * 2^-25 * 1 / 0.15, no credit for averaging); chosen's score is the
                  minimum of candidate_score; align_geometry(init="centroid") on the same input ends > 0.5 from the truth in every scene.
  determinism, batching: bit equality.  Refusals: non-zero, the entry's name in mvd_last_error(), nothing written.

Measured on an MI355X: no inlier mismatch on any (scene, hypothesis) of the six cases and the cross-check; score relative error 0 on
every one against bounds of 7.8e-14 .. 2.4e-12 (sums of a few thousand 24-bit values of like size are exact in fp64); grid, brute and
auto the same bits; select equal to the numpy rule on all 18 tables.  End to end, poses 3 / 14 / 22 / 26: |matrix - truth| 3.04e-11 /
4.19e-11 / 2.91e-11 / 1.99e-10 against 9.54e-7 (the oracle's own figures to every printed digit), every correspondence right, the
chosen candidate's score 0.108 / 2.3e-16 / 1.8e-17 / 2.9e-18 against 0.72 .. 0.94 for the others; centroid ICP ends 1.74 / 1.53 / 1.79 /
2.00 from the truth.  The file runs in 2.2 s.
"""
import ctypes
import dataclasses
import math

import numpy as np
import pytest
import torch

import align_f64 as A
import register_f64 as RG

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
ICP_BOUND = 2.0 ** -20
INF = float("inf")


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


def _i32(v):
    return torch.tensor(v, dtype=torch.int32).cuda()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else (t.view(torch.int32) if t.dtype == torch.float32 else t)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _scratch(nbytes):
    return torch.full((max((nbytes + 7) // 8, 2),), 0x1234, dtype=torch.int64, device="cuda")


def _device(case):
    return dict(points=case.points.contiguous().cuda(), start=_i32(case.start), target=case.target.contiguous().cuda(), tstart=_i32(case.tstart),
                hyp=torch.from_numpy(case.hyp).contiguous().cuda(), ns=int(case.points.shape[0]), nt=int(case.target.shape[0]), nscene=case.nscene,
                H=case.H, trunc2=case.trunc2)


def _score_call(hip, dev, out, method, grid, kw=None):
    a = dict(points=hip.ptr(dev["points"]), start=hip.ptr(dev["start"]), target=hip.ptr(dev["target"]), tstart=hip.ptr(dev["tstart"]), ns=dev["ns"],
             nt=dev["nt"], nscene=dev["nscene"], H=dev["H"], hyp=hip.ptr(dev["hyp"]), trunc2=dev["trunc2"], method=method, grid=grid,
             score=hip.ptr(out["score"]), inliers=hip.ptr(out["inliers"]), scratch=hip.ptr(out["scratch"]), nbytes=out["nbytes"])
    a.update(kw or {})
    return hip.lib().mvd_register_score(*a.values(), hip.stream())


def _score_buffers(hip, dev, method, grid):
    nbytes = int(hip.lib().mvd_register_scratch(dev["ns"], dev["nt"], dev["nscene"], dev["H"], method, grid))
    assert nbytes > 0
    return dict(score=torch.full((dev["nscene"], dev["H"]), SENTINEL, dtype=torch.float64, device="cuda"),
                inliers=torch.full((dev["nscene"], dev["H"]), -5, dtype=torch.int32, device="cuda"), scratch=_scratch(nbytes), nbytes=nbytes)


def _build(hip, dev, out, method, grid):
    hip.check(hip.lib().mvd_nearest_points_stages(None, hip.ptr(dev["tstart"]), hip.ptr(dev["target"]), hip.ptr(dev["tstart"]), 0, dev["nt"],
                                                  dev["nscene"], method, grid, None, None, hip.ptr(out["scratch"]), out["nbytes"], hip.NN_BUILD,
                                                  hip.stream()))


def _score(hip, dev, method, grid):
    out = _score_buffers(hip, dev, method, grid)
    _build(hip, dev, out, method, grid)
    hip.check(_score_call(hip, dev, out, method, grid))
    torch.cuda.synchronize()
    return out["score"].cpu(), out["inliers"].cpu()


def _check_score(name, case, got, got_inl, want, want_inl, slack=1.0):
    rows = np.diff(np.clip(np.asarray(case.start, dtype=np.int64), 0, case.points.shape[0]))
    bound = (rows * 2.0 ** -53 + 2.0 ** -52)[:, None] * want * slack
    err = np.abs(got.numpy() - want)
    rel = float((err / np.maximum(want, 1e-300)).max())
    print(f"RATIO register score {name} | worst relative error {rel:.2e} (bound {float((rows * 2.0 ** -53 + 2.0 ** -52).max() * slack):.2e}) | "
          f"inlier mismatches {int((got_inl.numpy() != want_inl).sum())} of {want_inl.size}")
    assert np.array_equal(got_inl.numpy(), want_inl), name
    assert bool((err <= bound).all()), name


# ------------------------------------------------------------------------------------------------ score
@pytest.mark.parametrize("name", list(RG.SCORE_CASES))
def test_score_and_inliers_meet_the_oracle_and_every_method_gives_the_same_bits(hip, name):
    case = RG.score_case(name)
    want, want_inl = RG.score_ref(name)
    dev = _device(case)
    first = None
    for method, grid in ((hip.NN_GRID, 0), (hip.NN_GRID, 5), (hip.NN_BRUTE, 0), (hip.NN_AUTO, 0), (hip.NN_GRID, 0)):
        got, got_inl = _score(hip, dev, method, grid)
        if first is None:
            first = (got, got_inl)
            _check_score(name, case, got, got_inl, want, want_inl)
        assert _same(got, first[0]) and torch.equal(got_inl, first[1]), (name, method, grid)
    if name == "far":
        rows = np.diff(case.start)
        assert np.array_equal(first[0].numpy(), rows[:, None] * np.full((1, case.H), case.trunc2)) and int(first[1].sum()) == 0
    if name == "lattice":
        _, _, d2, _ = RG.row_costs(case.hyp[:, 0].reshape(1, 3, 4), case.points, case.start, case.target, case.tstart, case.trunc2)
        assert int((d2 == case.trunc2).sum()) > 0 and int((d2 > case.trunc2).sum()) > 0      # the threshold is a value that occurs
        assert np.array_equal(first[0].numpy(), want)                                          # every sum is exact on the lattice


@pytest.mark.parametrize("H", [1, 3])
def test_fewer_hypotheses_are_the_first_columns(hip, H):
    case = RG.score_case("many_hypotheses")
    want, want_inl = RG.score_ref("many_hypotheses")
    dev = _device(case)
    dev["hyp"], dev["H"] = dev["hyp"][:, :H].contiguous(), H
    for method in (hip.NN_GRID, hip.NN_BRUTE):
        got, got_inl = _score(hip, dev, method, 0)
        _check_score(f"many_hypotheses H={H}", case, got, got_inl, want[:, :H], want_inl[:, :H])


def test_score_against_apply_and_nearest_points_with_no_oracle(hip):
    from mvdfusion_amd import fusion
    lens, H = [9000, 11000], 3
    start = [0, 9000, 20000]
    case = RG._scenes_case(lens, [10000, 10000], H, 8400)
    dev = _device(case)
    got, got_inl = _score(hip, dev, hip.NN_AUTO, 0)
    brute, brute_inl = _score(hip, dev, hip.NN_BRUTE, 0)
    assert _same(got, brute) and torch.equal(got_inl, brute_inl)
    want, want_inl = np.zeros((2, H)), np.zeros((2, H), dtype=np.int64)
    t2 = torch.tensor(case.trunc2, dtype=torch.float32, device="cuda")
    for h in range(H):
        moved = fusion._align_apply(dev["points"], dev["start"], 2, dev["hyp"][:, h].contiguous())
        _, d2 = fusion._nearest(moved, dev["start"], dev["target"], dev["tstart"], 2, hip.NN_AUTO, 0)
        inl = d2 <= t2
        cost = torch.where(inl, d2, t2).double()
        for s in range(2):
            want[s, h] = float(cost[start[s]:start[s + 1]].sum())
            want_inl[s, h] = int(inl[start[s]:start[s + 1]].sum())
    _check_score("cross-check", case, got, got_inl, want, want_inl, slack=2.0)


# ------------------------------------------------------------------------------------------------ select
def _select(hip, score, quat, K, cos_half, kw=None, out=None):
    N, H = score.shape
    out = out or dict(top=torch.full((N, K), -5, dtype=torch.int32, device="cuda"), top_score=torch.full((N, K), SENTINEL, dtype=torch.float64, device="cuda"))
    a = dict(score=hip.ptr(score), quat=hip.ptr(quat), nscene=N, H=H, K=K, cos_half=cos_half, top=hip.ptr(out["top"]), top_score=hip.ptr(out["top_score"]))
    a.update(kw or {})
    rc = hip.lib().mvd_register_select(*a.values(), hip.stream())
    torch.cuda.synchronize()
    return rc, out["top"].cpu(), out["top_score"].cpu()


def _check_select(hip, score, quat, K, cos_half, name):
    rc, top, top_score = _select(hip, torch.from_numpy(score).cuda(), torch.from_numpy(quat).cuda(), K, cos_half)
    assert rc == 0
    for s in range(score.shape[0]):
        want, want_score = RG.select(score[s], quat, cos_half, K)
        assert top[s].tolist() == want.tolist() and np.array_equal(top_score[s].numpy(), want_score), (name, s, top[s].tolist(), want.tolist())
    print(f"RATIO register select {name}: equal to the numpy rule; scene 0 takes {top[0].tolist()[:8]}")
    return top, top_score


@pytest.mark.parametrize("H, K", [(1, 1), (1, 4), (300, 8), (4096, 32), (16384, 16)])
def test_select_is_the_greedy_rule(hip, H, K):
    rng = np.random.default_rng(8500 + H)
    quat = RG.rotation_grid(H)
    score = rng.uniform(0.0, 1.0, size=(3, H))
    score[1, rng.integers(0, H, size=H // 3 + 1)] = 0.25                       # ties: the lowest h
    score[2, ::2] = float("nan")
    score[2, 1 % H] = INF
    for sep in (30.0, 90.0):
        _check_select(hip, score, quat, K, math.cos(math.radians(sep) / 2), f"H={H} K={K} sep={sep:.0f}")
    _check_select(hip, score, quat, K, 2.0, f"H={H} K={K} no suppression")


def test_select_duplicates_suppression_and_what_is_left(hip):
    # two copies of every rotation with equal bits in score and quaternion: the lower h wins; its twin is within 0 degrees of it
    quat = np.concatenate([RG.rotation_grid(8), RG.rotation_grid(8)])
    score = np.tile(np.linspace(0.1, 0.8, 8), 2)[None]
    top, _ = _check_select(hip, score, quat, 4, math.cos(math.radians(30.0) / 2), "duplicates at 30 degrees")
    assert top[0, 0] == 0 and 8 not in top[0].tolist()
    top, top_score = _check_select(hip, score, quat, 4, 2.0, "duplicates, no suppression")
    assert top[0].tolist() == [0, 8, 1, 9] and top_score[0, 0] == top_score[0, 1]
    # NaN is never taken, +inf is, and more asked for than alive gives -1 / +inf
    score = np.array([[float("nan"), INF, 0.5, float("nan"), 0.25, INF]])
    top, top_score = _check_select(hip, score, RG.rotation_grid(6), 6, 2.0, "nan and inf")
    assert top[0].tolist() == [4, 2, 1, 5, -1, -1] and top_score[0].tolist() == [0.25, 0.5, INF, INF, INF, INF]
    top, _ = _check_select(hip, np.full((1, 5), float("nan")), RG.rotation_grid(5), 3, 2.0, "all nan")
    assert top[0].tolist() == [-1, -1, -1]
    top, _ = _check_select(hip, np.ones((1, 40)), RG.rotation_grid(40), 32, math.cos(math.radians(120.0) / 2), "suppression empties the set")
    assert top[0, 0] == 0 and top[0, -1] == -1


# ------------------------------------------------------------------------------------------------ end to end
@dataclasses.dataclass
class Cloud:
    """The least ``nearest_points`` takes: points and their sorted scene ids."""
    xyz: torch.Tensor
    scene: torch.Tensor


def _batch(poses):
    cases = [RG.pose_case(k) for k in poses]
    n = cases[0].n
    scene = torch.arange(len(poses)).repeat_interleave(n).cuda()
    src = Cloud(xyz=torch.cat([c.source for c in cases]).cuda(), scene=scene)
    tgt = Cloud(xyz=torch.cat([c.target for c in cases]).cuda(), scene=scene)
    perm = torch.cat([c.perm + k * n for k, c in enumerate(cases)])
    return cases, src, tgt, perm


@pytest.fixture(scope="module")
def batch_result(hip):
    from mvdfusion_amd import fusion
    cases, src, tgt, perm = _batch(RG.GPU_POSES)
    reg = fusion.register_geometry(src, tgt, scenes=len(cases), trunc=0.04)
    torch.cuda.synchronize()
    return cases, src, tgt, perm, reg


def test_register_geometry_recovers_the_poses_plain_icp_does_not(hip, batch_result):
    from mvdfusion_amd import fusion
    cases, src, tgt, perm, reg = batch_result
    N = len(cases)
    assert isinstance(reg, fusion.Registration) and isinstance(reg, fusion.Alignment)
    plain = fusion.align_geometry(src, tgt, scenes=N, init="centroid")
    right = reg.nearest.index.cpu().long() == perm
    for s, case in enumerate(cases):
        err = float(np.abs(reg.matrix[s].cpu().numpy() - case.truth[0]).max())
        err_plain = float(np.abs(plain.matrix[s].cpu().numpy() - case.truth[0]).max())
        sc = reg.candidate_score[s].cpu().numpy()
        cand = np.abs(reg.candidates[s].cpu().numpy() - case.truth[0][None]).reshape(sc.size, -1).max(1)
        print(f"RATIO register pose {RG.GPU_POSES[s]} ({RG.pose_angle(RG.GPU_POSES[s]):.1f} deg) | |M - truth| {err:.2e} (bound {ICP_BOUND:.2e}) | right "
              f"{int(right[s * case.n:(s + 1) * case.n].sum())}/{case.n} | chosen {int(reg.chosen[s])} scores {np.array2string(sc, precision=3)} "
              f"candidate errors {np.array2string(cand, precision=1)} | inliers {reg.candidate_inliers[s].tolist()} | centroid ICP {err_plain:.2e}")
        assert err <= ICP_BOUND and bool(right[s * case.n:(s + 1) * case.n].all()), s
        assert sc[int(reg.chosen[s])] == sc.min(), s
        assert err_plain > 0.5, s
    assert tuple(reg.candidates.shape) == (N, fusion.REGISTER_CANDIDATES, 4, 4) and tuple(reg.grid_score.shape) == (N, fusion.REGISTER_ROTATIONS)
    assert tuple(reg.rms.shape) == (fusion.ALIGN_ITERS + 1, N) and bool((reg.scale == 1).all())
    moved = reg.apply(src)
    assert _same(moved.xyz, reg.xyz)


def test_a_scene_alone_and_in_the_batch_and_two_runs_give_the_same_bits(hip, batch_result):
    from mvdfusion_amd import fusion
    cases, src, tgt, perm, reg = batch_result
    again = fusion.register_geometry(src, tgt, scenes=len(cases), trunc=0.04)
    for f in ("matrix", "candidates", "candidate_score", "candidate_inliers", "chosen", "grid_score", "rms", "xyz"):
        assert _same(getattr(again, f), getattr(reg, f)), f
    s = 1
    alone = fusion.register_geometry(cases[s].source.cuda(), cases[s].target.cuda(), trunc=0.04)
    for f in ("matrix", "candidates", "candidate_score", "candidate_inliers", "chosen", "grid_score"):
        assert _same(getattr(alone, f)[0], getattr(reg, f)[s]), f
    assert _same(alone.rms[:, 0], reg.rms[:, s])


def test_the_result_is_an_init_of_the_aligners(hip, batch_result):
    from mvdfusion_amd import fusion
    cases, src, tgt, perm, reg = batch_result
    N = len(cases)
    al = fusion.align_to_surface(src, tgt, scenes=N, init=reg, iters=2)
    pp = fusion.align_geometry(src, tgt, scenes=N, init=reg, iters=1)
    torch.cuda.synchronize()
    assert isinstance(al, fusion.PlaneAlignment) and bool(torch.isfinite(al.matrix).all()) and tuple(al.matrix.shape) == (N, 4, 4)
    for s, case in enumerate(cases):
        assert float(np.abs(pp.matrix[s].cpu().numpy() - case.truth[0]).max()) <= ICP_BOUND
    # given rotations: the identity alone is init="centroid" + ICP
    one = fusion.register_geometry(src, tgt, scenes=N, rotations=torch.eye(3)[None], candidates=1, refine_iters=0, trunc=0.04)
    plain = fusion.align_geometry(src, tgt, scenes=N, init="centroid")
    assert _same(one.matrix, plain.matrix)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(hip):
    L = hip.lib()
    case = RG.score_case("many_hypotheses")
    dev = _device(case)
    out = _score_buffers(hip, dev, hip.NN_GRID, 5)
    odd = lambda t, by: ctypes.c_void_p(t.data_ptr() + by)
    bad = [dict(points=None), dict(start=None), dict(target=None), dict(tstart=None), dict(hyp=None), dict(score=None), dict(inliers=None),
           dict(scratch=None), dict(hyp=odd(dev["hyp"], 4)), dict(score=odd(out["score"], 4)), dict(inliers=odd(out["inliers"], 2)),
           dict(points=odd(dev["points"], 2)), dict(scratch=odd(out["scratch"], 8)), dict(nscene=0), dict(nscene=65536), dict(H=0),
           dict(H=hip.REGISTER_MAX_H + 1), dict(method=3), dict(method=-1), dict(grid=-1), dict(grid=257), dict(ns=1 << 31), dict(nt=1 << 31),
           dict(trunc2=0.0), dict(trunc2=-1.0), dict(trunc2=INF), dict(trunc2=float("nan")), dict(nbytes=out["nbytes"] - 16), dict(nbytes=0),
           dict(nscene=65535, grid=256, nbytes=1 << 62)]
    for kw in bad:
        assert _score_call(hip, dev, out, hip.NN_GRID, 5, kw=kw) != 0, kw
        assert b"mvd_register_score" in L.mvd_last_error(), (kw, L.mvd_last_error())
    torch.cuda.synchronize()
    assert bool((out["score"] == SENTINEL).all()) and bool((out["inliers"] == -5).all()) and bool((out["scratch"] == 0x1234).all())
    score, quat = torch.rand(2, 50, dtype=torch.float64).cuda(), torch.from_numpy(RG.rotation_grid(50)).cuda()
    keep = dict(top=torch.full((2, 4), -5, dtype=torch.int32, device="cuda"), top_score=torch.full((2, 4), SENTINEL, dtype=torch.float64, device="cuda"))
    for kw in (dict(score=None), dict(quat=None), dict(top=None), dict(top_score=None), dict(score=odd(score, 4)), dict(quat=odd(quat, 4)),
               dict(top_score=odd(keep["top_score"], 4)), dict(top=odd(keep["top"], 2)), dict(nscene=0), dict(nscene=65536), dict(H=0),
               dict(H=hip.REGISTER_MAX_H + 1), dict(K=0), dict(K=hip.REGISTER_MAX_K + 1), dict(cos_half=float("nan"))):
        rc, _, _ = _select(hip, score, quat, 4, 0.9, kw=kw, out=keep)
        assert rc != 0 and b"mvd_register_select" in L.mvd_last_error(), (kw, L.mvd_last_error())
    assert bool((keep["top"] == -5).all()) and bool((keep["top_score"] == SENTINEL).all())
