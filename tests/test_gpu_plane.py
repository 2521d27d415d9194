"""The point-to-plane entries on the GPU: mvd_plane_fit and mvd_plane_icp (csrc/align.hip) through the C ABI against the float64 oracle
of tests/plane_f64.py, and the host path (fusion.fit_plane_step, fusion.align_to_surface).

Bounds -- none taken from what the kernels give:
  pairs, rank     EQUAL to the oracle's on every scene of every case (the cases keep every eigenvalue a factor 16 clear of the rank
                  threshold, tests/test_cpu_plane.py asserts it on the oracle).
  plane rms, rms  relative (n + 4) * 2^-53: a sum of n non-negative addends formed as the oracle forms them and added in some order is
                  within n * 2^-53 relative of the exact sum (the oracle adds exactly); the quotient and the root add 2 roundings each.
  step            plane_f64.solve_bound with the sums' n * 2^-53: (128 + 16 n) * 2^-53 * kappa * |g| / lambda_min + 32 * 2^-53.
                  |R^T R - I| <= 32 * 2^-53 on the composed transform's rotation (one product with the identity), det > 0.
  determinism     bit equality run to run, and of a scene alone against the same scene in a batch.
  ICP, exact      final correspondences = the permutation on every point; |M - truth| <= 2^-20; last plane rms and rms <= 2^-22.
  ICP, sliding    |M_gpu - M_oracle| <= 1 / 16 of the oracle's own |M - truth| (7.9e-4: the method's sampling noise); moved, index and
                  dist2 EQUAL to mvd_align_apply + mvd_nearest_points of the returned transform.
  refusals        non-zero, the entry's name in mvd_last_error(), nothing written.

Measured on an MI355X: pairs and rank equal on every scene; plane rms at most 1.85 x 2^-53 relative (bound n + 4); step error 5.2e-17 ..
7.6e-16 against bounds 4.1e-14 .. 7.9e-10, and 2.8e-12 on `offset`, whose derived bound (1.57 at kappa 2e5) checks nothing there; exact
partners |M - truth| 2.22e-10, last plane rms 4.5e-10, rms 1.3e-9, |M - M_oracle| 5.1e-16; sliding |M_gpu - M_oracle| 3.5e-15 (bound 4.95e-5),
align_geometry 0.0607 against align_to_surface 0.000792 from the truth.
"""
import ctypes

import numpy as np
import pytest
import torch

import align_f64 as A
import plane_f64 as P

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
INF = float("inf")
ORTHO_BOUND = 32 * 2.0 ** -53


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def _identity(n):
    return torch.eye(3, 4, dtype=torch.float64).reshape(1, 12).repeat(n, 1).cuda()


def _fit(hip, moved, start, target, normals, index, dist2, n, nt, nscene, flags, max_d2, transform, row, scratch=None, nbytes=None):
    L = hip.lib()
    need = int(L.mvd_plane_scratch(n, 0, nscene, hip.NN_BRUTE, 0))
    scratch = torch.full(((need + 7) // 8 + 2,), 0x1234, dtype=torch.int64, device="cuda") if scratch is None else scratch
    p = hip.ptr
    return L.mvd_plane_fit(p(moved), p(start), p(target), p(normals), p(index), p(dist2), n, nt, nscene, flags, max_d2, p(transform), p(row),
                           p(scratch), need if nbytes is None else nbytes, hip.stream())


def _run_fit(hip, case, rows=None, offsets=None, flags=0):
    """mvd_plane_fit on the case's own pairing (or on the source rows `rows` as scenes `offsets`) from the identity."""
    base = case.base
    if rows is None:
        rows, offsets = slice(0, base.n), base.start
        target, normals = base.target, case.normals
        index, dist2 = base.index, base.dist2
    else:          # a scene alone: row i with row i
        target, normals, index, dist2 = base.target[rows], case.normals[rows], None, None
    moved = base.source[rows].contiguous().cuda()
    nscene = len(offsets) - 1
    transform = _identity(nscene)
    row = torch.full((nscene, 4), SENTINEL, dtype=torch.float64, device="cuda")
    dev = lambda t: None if t is None else t.contiguous().cuda()
    hip.check(_fit(hip, moved, _i32(offsets), dev(target), dev(normals), dev(index), dev(dist2), moved.shape[0], target.shape[0], nscene, flags,
                   base.max_d2, transform, row))
    torch.cuda.synchronize()
    return transform.cpu().numpy().reshape(nscene, 3, 4), row.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the fit
@pytest.mark.parametrize("name", list(P.FIT_CASES))
def test_one_step_meets_the_oracle(hip, name):
    ref = P.fit_refs(name)
    case = ref.case
    D, row = _run_fit(hip, case)
    again_D, again_row = _run_fit(hip, case)
    assert np.array_equal(D.view(np.int64), again_D.view(np.int64)) and np.array_equal(row.view(np.int64), again_row.view(np.int64))
    for s, (sums, sol) in enumerate(zip(ref.sums, ref.solves)):
        n = int(sums[0])
        assert row[s, 1] == n and row[s, 3] == sol.rank == case.rank[s], (s, row[s], n, sol.rank)          # counts and rank: equal
        want_row = ref.rows[s]
        if n == 0:
            assert np.isnan(row[s, 0]) and np.isnan(row[s, 2])
        else:
            rel = (n + 4) * 2.0 ** -53
            assert abs(row[s, 0] - want_row[0]) <= rel * want_row[0] and abs(row[s, 2] - want_row[2]) <= rel * want_row[2], (s, row[s], want_row)
        want = np.concatenate([sol.R, sol.t[:, None]], axis=1)
        err = float(np.abs(D[s] - want).max())
        R = D[s][:, :3]
        if sol.rank == 0:
            assert np.array_equal(D[s], np.eye(3, 4))
            continue
        print(f"RATIO plane fit {name} scene {s} | pairs {n} rank {sol.rank} | step error {err:.3g} (bound {sol.bound:.3g}) | plane rms "
              f"{row[s, 0]:.6g} rel err {abs(row[s, 0] - want_row[0]) / want_row[0] / 2.0 ** -53:.2f} x 2^-53 (bound {n + 4})")
        assert err <= sol.bound and float(np.abs(R.T @ R - np.eye(3)).max()) <= ORTHO_BOUND and np.linalg.det(R) > 0
    if name == "plane":
        assert abs(D[0][0, 3]) < 2.0 ** -40 and abs(D[0][1, 3]) < 2.0 ** -40 and abs(D[0][1, 0] - D[0][0, 1]) / 2 < 2.0 ** -40
    # MVD_PLANE_NO_STEP: the same row, the transform left alone
    kept, row2 = _run_fit(hip, case, flags=hip.PLANE_NO_STEP)
    assert np.array_equal(kept, np.tile(np.eye(3, 4), (case.base.nscene, 1, 1))) and np.array_equal(row2.view(np.int64), row.view(np.int64))


@pytest.mark.parametrize("name", ["chunk_edges", "few_pairs"])
def test_a_scene_alone_gives_the_bits_it_gives_in_the_batch(hip, name):
    case = P.make_case(name)
    D, row = _run_fit(hip, case)
    start = case.base.start
    for s in range(case.base.nscene):
        alone_D, alone_row = _run_fit(hip, case, rows=slice(start[s], start[s + 1]), offsets=[0, start[s + 1] - start[s]])
        assert np.array_equal(alone_D[0].view(np.int64), D[s].view(np.int64)) and np.array_equal(alone_row[0].view(np.int64), row[s].view(np.int64)), s


def test_bad_fit_arguments_return_an_error_and_write_nothing(hip):
    L = hip.lib()
    case = P.make_case("generic")
    base = case.base
    n = base.n
    moved, target, normals, start = base.source.cuda(), base.target.cuda(), case.normals.contiguous().cuda(), _i32(base.start)
    transform, row = torch.full((1, 12), SENTINEL, dtype=torch.float64, device="cuda"), torch.full((1, 4), SENTINEL, dtype=torch.float64, device="cuda")
    need = int(L.mvd_plane_scratch(n, 0, 1, hip.NN_BRUTE, 0))
    scratch = torch.full(((need + 7) // 8 + 2,), 0x1234, dtype=torch.int64, device="cuda")
    good = dict(moved=moved, start=start, target=target, normals=normals, index=None, dist2=None, n=n, nt=n, nscene=1, flags=0, max_d2=INF,
                transform=transform, row=row, scratch=scratch, nbytes=need)
    bad = [dict(nscene=0), dict(nscene=65536), dict(n=1 << 31), dict(nt=1 << 31), dict(flags=1), dict(flags=4), dict(max_d2=-1.0),
           dict(max_d2=float("nan")), dict(start=None), dict(transform=None), dict(row=None), dict(moved=None), dict(target=None), dict(normals=None),
           dict(nbytes=need - 16), dict(nbytes=0)]
    for kw in bad:
        a = dict(good)
        a.update(kw)
        assert _fit(hip, **a) != 0 and b"mvd_plane_fit" in L.mvd_last_error(), kw
    torch.cuda.synchronize()
    assert bool((transform == SENTINEL).all()) and bool((row == SENTINEL).all()) and bool((scratch == 0x1234).all())


# ------------------------------------------------------------------------------------------------ 2. ICP
def _icp(hip, case, iters, method=None, grid=0, init=None, call_iters=None, **override):
    L = hip.lib()
    base = case.base
    method = hip.NN_AUTO if method is None else method
    source, target, normals = base.source.cuda(), base.target.cuda(), case.normals.contiguous().cuda()
    nq, nt = base.n, base.nt
    transform = _identity(1) if init is None else torch.tensor(np.asarray(init)[:3].reshape(1, 12), dtype=torch.float64).cuda()
    out = dict(history=torch.full((iters + 1, 1, 4), SENTINEL, dtype=torch.float64, device="cuda"), moved=torch.full((nq, 3), SENTINEL, device="cuda"),
               index=torch.full((nq,), -5, dtype=torch.int32, device="cuda"), dist2=torch.full((nq,), SENTINEL, device="cuda"), transform=transform)
    need = int(L.mvd_plane_scratch(nq, nt, 1, method, grid))
    out["scratch"] = torch.full(((need + 7) // 8 + 2,), 0x1234, dtype=torch.int64, device="cuda")
    p = hip.ptr
    a = dict(source=p(source), sstart=p(_i32(base.start)), target=p(target), tstart=p(_i32(base.tstart)), normals=p(normals), nq=nq, nt=nt, nscene=1,
             method=method, grid=grid, iters=iters, max_d2=base.max_d2, transform=p(transform), history=p(out["history"]), moved=p(out["moved"]),
             index=p(out["index"]), dist2=p(out["dist2"]), scratch=p(out["scratch"]), nbytes=need)
    a.update(override)
    if call_iters is not None:
        a["iters"] = call_iters
    rc = L.mvd_plane_icp(*a.values(), hip.stream())
    torch.cuda.synchronize()
    return rc, out, (source, target)


def _matrix(out):
    M = np.eye(4)
    M[:3] = out["transform"].cpu().numpy().reshape(3, 4)
    return M


def _final_pass_is_apply_and_search(hip, case, out, source, target):
    """moved, index, dist2 EQUAL to mvd_align_apply + mvd_nearest_points of the returned transform."""
    L = hip.lib()
    base = case.base
    p = hip.ptr
    moved = torch.empty_like(source)
    hip.check(L.mvd_align_apply(p(source), p(_i32(base.start)), base.n, 1, p(out["transform"]), p(moved), hip.stream()))
    index, dist2 = torch.empty(base.n, dtype=torch.int32, device="cuda"), torch.empty(base.n, device="cuda")
    need = int(L.mvd_nearest_points_scratch(base.nt, 1, hip.NN_AUTO, 0))
    scratch = torch.empty((need + 7) // 8 + 2, dtype=torch.int64, device="cuda")
    hip.check(L.mvd_nearest_points(p(moved), p(_i32(base.start)), p(target), p(_i32(base.tstart)), base.n, base.nt, 1, hip.NN_AUTO, 0, p(index),
                                   p(dist2), p(scratch), need, hip.stream()))
    torch.cuda.synchronize()
    return torch.equal(moved.view(torch.int32), out["moved"].view(torch.int32)) and torch.equal(index, out["index"]) and \
        torch.equal(dist2.view(torch.int32), out["dist2"].view(torch.int32))


def test_exact_partners_converge_to_the_permutation(hip):
    ref = P.icp_refs("icp_exact")
    case = ref.case
    rc, out, (source, target) = _icp(hip, case, case.iters)
    assert rc == 0, hip.lib().mvd_last_error()
    M, history = _matrix(out), out["history"].cpu().numpy()[:, 0]
    err = float(np.abs(M - case.truth).max())
    print(f"RATIO plane icp exact | n {case.base.n} iters {case.iters} | |M - truth| {err:.3g} (bound 2^-20 = 9.5e-7) | last plane rms {history[-1, 0]:.3g} "
          f"rms {history[-1, 2]:.3g} (bound 2^-22 = 2.4e-7) | |M - M_oracle| {float(np.abs(M - ref.matrix).max()):.3g}")
    assert torch.equal(out["index"].cpu().long(), case.base.perm) and err <= 2.0 ** -20
    assert history[-1, 0] <= 2.0 ** -22 and history[-1, 2] <= 2.0 ** -22 and (history[:, 1] == case.base.n).all() and (history[:, 3] == 6).all()
    R = M[:3, :3]
    assert float(np.abs(R.T @ R - np.eye(3)).max()) <= (case.iters + 1) * ORTHO_BOUND and np.linalg.det(R) > 0
    assert _final_pass_is_apply_and_search(hip, case, out, source, target)
    for method, grid in ((hip.NN_BRUTE, 0), (hip.NN_GRID, 9)):          # the search's method changes no bit
        rc, other, _ = _icp(hip, case, case.iters, method=method, grid=grid)
        assert rc == 0 and all(torch.equal(out[k].view(torch.int32), other[k].view(torch.int32)) for k in ("moved", "index", "dist2"))
        assert torch.equal(out["transform"], other["transform"]) and torch.equal(out["history"], other["history"])


def _by_hand(hip, case, iters, method, grid):
    """The sequence mvd_plane_icp stands for, issued by the caller: mvd_nearest_points_stages(BUILD) once, then per row mvd_align_apply,
    mvd_nearest_points_stages(QUERY) and mvd_plane_fit on the pairs and distances the search left."""
    L, p, base = hip.lib(), hip.ptr, case.base
    source, target, normals = base.source.cuda(), base.target.cuda(), case.normals.contiguous().cuda()
    sstart, tstart, nq, nt = _i32(base.start), _i32(base.tstart), base.n, base.nt
    transform = _identity(1)
    history = torch.full((iters + 1, 1, 4), SENTINEL, dtype=torch.float64, device="cuda")
    moved, index, dist2 = torch.empty_like(source), torch.empty(nq, dtype=torch.int32, device="cuda"), torch.empty(nq, device="cuda")
    nn_bytes = int(L.mvd_nearest_points_scratch(nt, 1, method, grid))
    nn = torch.empty((nn_bytes + 7) // 8 + 2, dtype=torch.int64, device="cuda")
    search = lambda stages: hip.check(L.mvd_nearest_points_stages(p(moved), p(sstart), p(target), p(tstart), nq, nt, 1, method, grid, p(index), p(dist2),
                                                                  p(nn) if nn_bytes else None, nn_bytes, stages, hip.stream()))
    search(hip.NN_BUILD)
    for k in range(iters + 1):
        hip.check(L.mvd_align_apply(p(source), p(sstart), nq, 1, p(transform), p(moved), hip.stream()))
        search(hip.NN_QUERY)
        hip.check(_fit(hip, moved, sstart, target, normals, index, dist2, nq, nt, 1, 0 if k < iters else hip.PLANE_NO_STEP, base.max_d2, transform,
                       history[k]))
    torch.cuda.synchronize()
    return dict(transform=transform, history=history, moved=moved, index=index, dist2=dist2)


@pytest.mark.parametrize("method, grid", [("NN_AUTO", 0), ("NN_BRUTE", 0), ("NN_GRID", 9)])
def test_the_loop_is_the_sequence_it_stands_for(hip, method, grid):
    """mvd_plane_icp against the caller-issued sequence: every output and every history column, bit for bit (no column is carried from
    row to row)."""
    case, iters, method = P.make_case("icp_exact"), 4, getattr(hip, method)
    rc, out, _ = _icp(hip, case, iters, method=method, grid=grid)
    assert rc == 0, hip.lib().mvd_last_error()
    hand = _by_hand(hip, case, iters, method, grid)
    bits = lambda t: t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)
    assert not bool((out["history"] == SENTINEL).any()) and not torch.equal(out["transform"], _identity(1))
    for k in ("transform", "history", "moved", "index", "dist2"):
        assert torch.equal(bits(hand[k]), bits(out[k])), k


def test_sliding_follows_the_oracle_to_a_sixteenth_of_its_own_error(hip):
    ref = P.icp_refs("icp_sliding")
    case = ref.case
    rc, out, (source, target) = _icp(hip, case, case.iters)
    assert rc == 0, hip.lib().mvd_last_error()
    M, history = _matrix(out), out["history"].cpu().numpy()[:, 0]
    own = float(np.abs(ref.matrix - case.truth).max())
    gap = float(np.abs(M - ref.matrix).max())
    print(f"RATIO plane icp sliding | n {case.base.n} iters {case.iters} | oracle |M - truth| {own:.4g}, |M_gpu - M_oracle| {gap:.3g} (bound {own / 16:.3g}) | "
          f"last plane rms {history[-1, 0]:.6g} (oracle {ref.history[-1, 0]:.6g}) rms {history[-1, 2]:.6g}")
    assert gap <= own / 16
    assert (history[:, 1] == ref.history[:, 1]).all() and (history[:, 3] == 6).all()
    assert _final_pass_is_apply_and_search(hip, case, out, source, target)
    # iters = 0 returns the start with one history row
    rc, zero, _ = _icp(hip, case, 0, init=P.TRUTH_SLIDE)
    assert rc == 0 and np.array_equal(_matrix(zero), P.TRUTH_SLIDE) and not bool((zero["history"] == SENTINEL).any())
    assert float(zero["history"][0, 0, 0]) < 0.01 and int(zero["history"][0, 0, 1]) == case.base.n


def test_bad_icp_arguments_return_an_error_and_write_nothing(hip):
    L = hip.lib()
    case = P.make_case("icp_sliding")
    bad = [dict(method=3), dict(grid=257), dict(nscene=0), dict(nscene=65536), dict(call_iters=-1), dict(call_iters=1025), dict(nq=1 << 31), dict(max_d2=-1.0),
           dict(sstart=None), dict(tstart=None), dict(transform=None), dict(history=None), dict(source=None), dict(moved=None), dict(index=None),
           dict(dist2=None), dict(target=None), dict(normals=None), dict(scratch=None), dict(nbytes=16)]
    for kw in bad:
        args = dict(method=hip.NN_GRID, grid=7)
        args.update(kw)
        rc, out, _ = _icp(hip, case, 3, **args)          # (a bad `iters` goes to the call alone: the buffers are those of 3 iterations)
        assert rc != 0 and b"mvd_plane_icp" in L.mvd_last_error(), kw
        assert bool((out["history"] == SENTINEL).all()) and bool((out["moved"] == SENTINEL).all()) and bool((out["index"] == -5).all())
        assert bool((out["scratch"] == 0x1234).all()) and torch.equal(out["transform"], _identity(1))


# ------------------------------------------------------------------------------------------------ 3. host path
def test_align_to_surface_with_its_own_normals_and_a_device_init(hip):
    from mvdfusion_amd import fusion
    ref = P.icp_refs("icp_sliding")
    case = ref.case
    src, tgt = case.base.source.cuda(), case.base.target.cuda()
    al = fusion.align_to_surface(src, tgt, k=16, iters=case.iters)          # normals: estimate_normals(target, 16) on the GPU
    own = float(np.abs(ref.matrix - case.truth).max())
    gap = float(np.abs(al.matrix[0].cpu().numpy() - ref.matrix).max())
    point = fusion.align_geometry(src, tgt, iters=case.iters)
    e_point = float(np.abs(point.matrix[0].cpu().numpy() - case.truth).max())
    e_plane = float(np.abs(al.matrix[0].cpu().numpy() - case.truth).max())
    print(f"RATIO align_to_surface sliding | |M - truth| align_geometry {e_point:.4g}, align_to_surface {e_plane:.4g} | against the oracle {gap:.3g} "
          f"(bound {own / 16:.3g}) | rms {float(al.rms[-1, 0]):.5f} plane rms {float(al.plane_rms[-1, 0]):.6f} rank {al.rank[-1].tolist()}")
    assert gap <= own / 16 and e_plane <= e_point / 20
    assert al.rms.shape == al.plane_rms.shape == al.rank.shape == al.pairs.shape == (case.iters + 1, 1) and al.xyz.shape == src.shape
    assert torch.equal(al.apply(src), al.xyz)                                # Alignment.apply on a PlaneAlignment
    d = fusion.compare_geometry(al.apply(src), tgt)                          # ... and what takes an Alignment's output
    assert float(d.accuracy) < float(fusion.compare_geometry(point.apply(src), tgt).accuracy)
    # the recipe, and a GPU-resident init taken as given: iters = 0 returns it
    fine = fusion.align_to_surface(src, tgt, init=fusion.align_geometry(src, tgt, iters=5), iters=10)
    assert float(np.abs(fine.matrix[0].cpu().numpy() - case.truth).max()) <= 2 * own
    start = torch.tensor(P.TRUTH_SLIDE, dtype=torch.float64).cuda()
    zero = fusion.align_to_surface(src, tgt, init=start, iters=0, normals=case.normals.cuda())
    assert torch.equal(zero.matrix[0], start) and zero.rms.shape == (1, 1) and int(zero.rank[0, 0]) == 6
    # one known-pairs step on the exact-partner case moves towards the truth
    exact = P.make_case("icp_exact")
    s, t = exact.base.source.cuda(), exact.base.target.cuda()
    pairs = exact.base.perm.to(torch.int32).cuda()
    step = fusion.fit_plane_step(s, t, exact.normals.cuda(), pairs=pairs)
    once = P.solve(P.plane_sums(exact.base.source, exact, index=pairs.cpu(), dist2=None)[0], exact.base.n * 2.0 ** -53)
    assert float(np.abs(step.matrix[0, :3].cpu().numpy() - np.concatenate([once.R, once.t[:, None]], 1)).max()) <= once.bound
    assert torch.equal(step.nearest.index, pairs) and int(step.pairs[0, 0]) == exact.base.n
