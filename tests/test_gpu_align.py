"""The alignment on the GPU: mvd_align_apply, mvd_align_fit and mvd_align_icp (csrc/align.hip) through the C ABI against the float64 oracle of
tests/align_f64.py, and the host path (fusion.fit_similarity, fusion.align_geometry, Alignment.apply).

Bounds -- none taken from what the kernels give:
  moved           EQUAL, bit for bit, to the apply rule restated in numpy float64 on EVERY row of every case, rows of no scene and
                  non-finite rows included.  (Where the rule gives a NaN both sides must hold a NaN: its sign and payload are not part
                  of the rule -- an x86 and a gfx950 make different ones from inf - inf.)
  index, dist2    EQUAL to mvd_nearest_points on `moved`, and to the fp32 restatement of the search on the oracle's `moved`.
  pairs           EQUAL to the oracle's count on every scene: the acceptance compare is specified in fp32.
  rms             n 2^-53 relative (the additions of the sum; every addend is exact) plus 2^-52 (the division and the square root).
  step (s, R, t)  2^-32 against the SVD oracle fed the same pairs -- R's entries, s relatively, t relative to 1 + |t|.  Worst case: sum
                  error n 2^-53 ~ 9e-13 at n <= 8 192, times the raw-moment factor <= 8 inside the +-0.75 box, times the inverse
                  relative eigen-gap of Horn's matrix <= 2.5 for this shape: 2e-11; 2^-32 is 13 times that.  `offset` (the shape moved
                  by +8 per axis) gets the bound times 1 + |mu|^2 / sigma^2, computed from the case (about 10^3).
                  |R^T R - I| <= 32 * 2^-53 and det R > 0 on every case.
  ICP             final correspondences = the permutation on EVERY point; |matrix - truth| <= 2^-20 (the fp32 rounding of both point
                  sets, 2 * 2^-25 * 1 / 0.15, no credit for averaging; the oracle sits at 3e-11); last rms <= 2^-22; pairs = n in every
                  row; rms[0] within 1e-6 relative of the oracle's.
  determinism, batching: bit equality.  Refusals: non-zero, the entry's name in mvd_last_error(), nothing written.

The oracle's own figures (tests/test_cpu_align.py prints them): SVD against a quaternion solve 2e-16 .. 9e-16 (offset 2e-15); the
library's solve on the host against the SVD 1e-16 .. 9e-16 in R, <= 3e-16 in s, <= 3e-17 in t (offset: s 1.4e-13, t 1.5e-12, bound
2.2e-7); icp_sim5 has every correspondence right from iteration 6, icp_rigid10 from 12, |M - truth| 3.3e-11 and 3.4e-11.

Measured on an MI355X: no mismatch in moved, index, dist2 or pairs on any row of the ten inputs; the step against the SVD oracle at
most 8.9e-16 in R, 2.8e-16 in s, 2.3e-17 in t (offset: 1.2e-13, 2.3e-13, 3.2e-12 against 2.2e-7); |R^T R - I| at most 4.4e-16;
icp_sim5 / icp_rigid10 end with every correspondence right, |M - truth| 3.30e-11 / 3.39e-11 and rms 5.5e-11 / 1.5e-11.
The 262 145-row scene: R 6.7e-16, s 3.4e-16, t 4.6e-17 against its bound 5.8e-10; equal bits alone and in the batch.
"""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import align_f64 as A
import nearest_f64 as NN

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
STEP_BOUND = 2.0 ** -32
ORTHO_BOUND = 32 * 2.0 ** -53
INF = float("inf")


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


def _i32(v):
    return torch.tensor(v, dtype=torch.int32).cuda()


def _device(case):
    return dict(source=case.source.contiguous().cuda(), start=_i32(case.start), target=case.target.contiguous().cuda(), tstart=_i32(case.tstart))


def _bits(t):
    """fp32 / fp64 values as integers, every NaN as one value."""
    t = t.detach().cpu()
    if t.dtype in (torch.float32, torch.float64):
        t = torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t).contiguous()
        return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)
    return t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _transforms(n, seed=0):
    """(n, 3, 4) float64: a different similarity per scene."""
    return np.stack([A.similarity(0.8 + 0.15 * ((k + seed) % 5), 17.0 + 23 * k, (1 + k, 2, 3 - k), (0.1 * k - 0.2, 0.05, -0.03 * k))[:3] for k in range(n)])


def _identity(n):
    return torch.eye(3, 4, dtype=torch.float64).reshape(1, 12).repeat(n, 1).cuda()


def _apply(hip, src, start, n, nscene, transform, out):
    return hip.lib().mvd_align_apply(hip.ptr(src), hip.ptr(start), n, nscene, hip.ptr(transform), hip.ptr(out), hip.stream())


def _scratch(nbytes):
    return torch.full((max((nbytes + 7) // 8, 2),), 0x1234, dtype=torch.int64, device="cuda")


def _fit(hip, moved, start, target, index, dist2, n, nt, nscene, flags, max_d2, transform, row, scratch=None, nbytes=None):
    L = hip.lib()
    need = int(L.mvd_align_scratch(n, 0, max(min(nscene, 65535), 1), hip.NN_BRUTE, 0))
    scratch = _scratch(need) if scratch is None else scratch
    return L.mvd_align_fit(hip.ptr(moved), hip.ptr(start), hip.ptr(target), hip.ptr(index), hip.ptr(dist2), n, nt, nscene, flags, max_d2,
                           hip.ptr(transform), hip.ptr(row), hip.ptr(scratch), need if nbytes is None else nbytes, hip.stream())


def _icp_buffers(hip, case, iters, method, grid):
    nbytes = int(hip.lib().mvd_align_scratch(case.n, case.nt, case.nscene, method, grid))
    return dict(history=torch.full((iters + 1, case.nscene, 3), SENTINEL, dtype=torch.float64, device="cuda"),
                moved=torch.full((max(case.n, 1), 3), SENTINEL, device="cuda"), index=torch.full((max(case.n, 1),), -5, dtype=torch.int32, device="cuda"),
                dist2=torch.full((max(case.n, 1),), SENTINEL, device="cuda"), scratch=_scratch(nbytes), nbytes=nbytes)


def _icp(hip, dev, case, out, transform, iters, flags, max_d2, method=0, grid=0, kw=None):
    a = dict(source=hip.ptr(dev["source"]), start=hip.ptr(dev["start"]), target=hip.ptr(dev["target"]), tstart=hip.ptr(dev["tstart"]), nq=case.n,
             nt=case.nt, nscene=case.nscene, method=method, grid=grid, iters=iters, flags=flags, max_d2=max_d2, transform=hip.ptr(transform),
             history=hip.ptr(out["history"]), moved=hip.ptr(out["moved"]), index=hip.ptr(out["index"]), dist2=hip.ptr(out["dist2"]),
             scratch=hip.ptr(out["scratch"]), nbytes=out["nbytes"])
    a.update(kw or {})
    return hip.lib().mvd_align_icp(*a.values(), hip.stream())


def _step_of(m12):
    """(s, R, t) of a 12-double step taken from the identity: s from the rows' common norm is not used -- the history carries it."""
    m = np.asarray(m12, dtype=np.float64).reshape(3, 4)
    return m[:, :3], m[:, 3]


def _check_step(name, case, k, got12, s, want, bound):
    sR, t = _step_of(got12)
    R = sR / s
    s0, R0, t0 = want
    eR, es, et = float(np.abs(R - R0).max()), abs(s - s0) / s0, float(np.abs(t - t0).max()) / (1 + float(np.abs(t0).max()))
    ortho = float(np.abs(R.T @ R - np.eye(3)).max())
    print(f"RATIO align {name} scene {k} | R {eR:.2e} s {es:.2e} t {et:.2e} (bound {bound:.2e}) | |R^T R - I| {ortho:.2e} det {np.linalg.det(R):+.6f}")
    assert max(eR, es, et) <= bound and ortho <= ORTHO_BOUND and np.linalg.det(R) > 0, (name, k)
    if not case.scale:
        assert s == 1.0


def _check_rms(got, sums):
    n, want = sums[0], (np.sqrt(sums[18] / sums[0]) if sums[0] > 0 else np.nan)
    if n == 0:
        assert np.isnan(got)
    else:
        assert abs(got - want) <= (n * 2.0 ** -53 + 2.0 ** -52) * want, (got, want)


# ------------------------------------------------------------------------------------------------ 1. apply
@pytest.mark.parametrize("name", list(A.CASES))
def test_apply_gives_the_bits_of_the_rule_on_every_row(hip, name):
    case = A.make_case(name)
    src = case.source.contiguous().cuda()
    tables = [case.start]
    if case.n >= 10:
        tables.append([min(max(v, 3), case.n - 2) for v in case.start])          # rows of no scene at both ends
        tables.append([v - 7 if k == 0 else v + 9 if k == case.nscene else v for k, v in enumerate(case.start)])          # offsets to be clamped
    for seed, start in enumerate(tables):
        m = _transforms(case.nscene, seed)
        out = torch.full((case.n, 3), SENTINEL, device="cuda")
        hip.check(_apply(hip, src, _i32(start), case.n, case.nscene, torch.from_numpy(m).reshape(-1, 12).cuda(), out))
        want = A.apply(m, case.source, start)
        bad = (_bits(out) != _bits(want)).any(1)
        assert not bool(bad.any()), (name, start[:2], int(bad.sum()), int(torch.nonzero(bad)[0]))
        outside = torch.from_numpy(A.scene_of(start, case.n) < 0)
        assert _same(out.cpu()[outside], case.source[outside]) and (seed != 1 or bool(outside.any()))
    if name == "nonfinite":
        assert int(torch.isnan(out).any(1).sum()) >= 10


# ------------------------------------------------------------------------------------------------ 2. one fit step
@pytest.mark.parametrize("name", list(A.FIT_CASES))
def test_one_fit_step_on_given_pairs(hip, name):
    ref = A.fit_refs(name)
    case = ref.case
    dev = _device(case)
    index = None if case.index is None else case.index.cuda()
    dist2 = None if case.dist2 is None else case.dist2.cuda()
    transform = _identity(case.nscene)
    row = torch.full((case.nscene, 3), SENTINEL, dtype=torch.float64, device="cuda")
    hip.check(_fit(hip, dev["source"], dev["start"], dev["target"], index, dist2, case.n, case.nt, case.nscene, hip.ALIGN_SCALE if case.scale else 0,
                   case.max_d2, transform, row))
    row, steps = row.cpu().numpy(), transform.cpu().numpy()
    bound = STEP_BOUND * (A.spread_factor(case.source) if name == "offset" else 1.0)
    assert row[:, 1].tolist() == ref.pairs.tolist()
    for k in range(case.nscene):
        _check_rms(row[k, 0], ref.sums[k])
        _check_step(name, case, k, steps[k], row[k, 2], ref.steps[k], bound)
        if ref.pairs[k] < 3:
            assert np.array_equal(steps[k], np.eye(3, 4).ravel()) and row[k, 2] == 1.0
        if case.truth[k] is not None:
            assert float(np.abs(steps[k].reshape(3, 4) - case.truth[k][:3]).max()) <= 2.0 ** -20 * (bound / STEP_BOUND)
    # MVD_ALIGN_NO_STEP: the same row, the transform left alone
    again = torch.full((case.nscene, 3), SENTINEL, dtype=torch.float64, device="cuda")
    before = transform.clone()
    hip.check(_fit(hip, dev["source"], dev["start"], dev["target"], index, dist2, case.n, case.nt, case.nscene,
                   (hip.ALIGN_SCALE if case.scale else 0) | hip.ALIGN_NO_STEP, case.max_d2, transform, again))
    assert torch.equal(transform, before) and _same(again[:, :2], torch.from_numpy(row[:, :2])) and bool((again[:, 2] == 1).all())


@pytest.mark.parametrize("name", list(A.FIT_CASES))
def test_one_icp_step_from_a_given_transform(hip, name):
    """iters = 1 from a start that is not the identity: row 0 describes the pairs under the start, the returned transform is the step
    composed onto it, and moved / index / dist2 are those of the returned transform."""
    case = A.make_case(name)
    dev = _device(case)
    lattice = name == "gate"                                       # (the lattice stays a lattice under the identity only)
    init = np.stack([np.eye(3, 4)] * case.nscene) if lattice else np.stack([A.similarity(1.02, 3.0, (1, -1, 2), (0.01, 0.02, -0.01))[:3]] * case.nscene)
    transform = torch.from_numpy(init).reshape(-1, 12).contiguous().cuda()
    # the oracle's pass under the start
    moved0 = A.apply(init, case.source, case.start)
    qs, ts = torch.tensor(case.start), torch.tensor(case.tstart)
    index0, dist20 = NN.nearest(NN.Case(query=moved0, target=case.target, query_start=qs, target_start=ts))
    sums = A.moment_sums(moved0, case.target, index0, dist20, case.max_d2, case.start)
    for method, grid in ((hip.NN_BRUTE, 0), (hip.NN_GRID, 7)):
        out = _icp_buffers(hip, case, 1, method, grid)
        t = transform.clone()
        hip.check(_icp(hip, dev, case, out, t, 1, hip.ALIGN_SCALE if case.scale else 0, case.max_d2, method, grid))
        torch.cuda.synchronize()
        hist = out["history"].cpu().numpy()
        assert hist[0, :, 1].tolist() == sums[:, 0].tolist(), name          # pairs: EQUAL
        bound = STEP_BOUND * (A.spread_factor(case.source) if name == "offset" else 1.0)
        got = t.cpu().numpy().reshape(-1, 3, 4)
        for k in range(case.nscene):
            _check_rms(hist[0, k, 0], sums[k])
            # the step itself, at the bound of the fit: D = returned * start^-1 in float64 (the start is a similarity of scale 1.02: its
            # inverse and the product add a few 2^-53), its scale the history's
            D = (np.vstack([got[k], [0, 0, 0, 1]]) @ np.linalg.inv(np.vstack([init[k], [0, 0, 0, 1]])))[:3]
            _check_step(name + (" brute" if method == hip.NN_BRUTE else " grid"), case, k, D.ravel(), hist[0, k, 2], A.solve_svd(sums[k], case.scale), bound)
        # the last pass: the rule applied to the returned transform, the search on that
        moved1 = A.apply(got, case.source, case.start)
        assert _same(out["moved"][:case.n], moved1), name
        index1, dist21 = NN.nearest(NN.Case(query=moved1, target=case.target, query_start=qs, target_start=ts))
        assert torch.equal(out["index"][:case.n].cpu().long(), index1) and _same(out["dist2"][:case.n], dist21), name
        nbytes = int(hip.lib().mvd_nearest_points_scratch(case.nt, case.nscene, method, grid))
        index = torch.full((case.n,), -5, dtype=torch.int32, device="cuda")
        dist2 = torch.full((case.n,), SENTINEL, device="cuda")
        scratch = _scratch(nbytes)
        hip.check(hip.lib().mvd_nearest_points(hip.ptr(out["moved"]), hip.ptr(dev["start"]), hip.ptr(dev["target"]), hip.ptr(dev["tstart"]), case.n,
                                               case.nt, case.nscene, method, grid, hip.ptr(index), hip.ptr(dist2), hip.ptr(scratch), nbytes, hip.stream()))
        assert torch.equal(index, out["index"][:case.n]) and _same(dist2, out["dist2"][:case.n])
        sums1 = A.moment_sums(moved1, case.target, index1, dist21, case.max_d2, case.start)
        assert hist[1, :, 1].tolist() == sums1[:, 0].tolist() and np.array_equal(hist[1, :, 2], hist[0, :, 2])          # (the scale is carried on)
        for k in range(case.nscene):
            _check_rms(hist[1, k, 0], sums1[k])


# ------------------------------------------------------------------------------------------------ 3. ICP
@pytest.fixture(scope="module")
def icp_runs():
    from mvdfusion_amd import fusion
    runs = {}
    for name in A.ICP_CASES:
        case = A.make_case(name)
        runs[name] = fusion.align_geometry(case.source.cuda(), case.target.cuda(), iters=case.iters, scale=case.scale)
    return runs


@pytest.mark.parametrize("name", list(A.ICP_CASES))
def test_icp_recovers_every_correspondence_and_the_transform(hip, icp_runs, name):
    ref, al = A.icp_refs(name), icp_runs[name]
    case = ref.case
    err = float((al.matrix[0].cpu() - torch.from_numpy(case.truth[0])).abs().max())
    right = int((al.nearest.index.cpu().long() == case.perm).sum())
    print(f"RATIO align {name} | right {right} / {case.n} | |M - truth| {err:.2e} (bound {2.0 ** -20:.2e}, oracle {float(np.abs(ref.matrix - case.truth[0]).max()):.2e}) "
          f"| rms {float(al.rms[0, 0]):.6f} -> {float(al.rms[-1, 0]):.2e} (oracle {ref.rms[0]:.6f} -> {ref.rms[-1]:.2e})")
    assert right == case.n and err <= 2.0 ** -20
    assert al.rms.shape == al.pairs.shape == (case.iters + 1, 1) and al.rms.dtype == torch.float64 and al.pairs.dtype == torch.int64
    assert float(al.rms[-1, 0]) <= 2.0 ** -22 and bool((al.pairs == case.n).all())
    assert abs(float(al.rms[0, 0]) - ref.rms[0]) <= 1e-6 * ref.rms[0]
    assert al.matrix.shape == (1, 4, 4) and al.matrix[0, 3].tolist() == [0, 0, 0, 1] and al.xyz.shape == (case.n, 3) and al.xyz.dtype == torch.float32
    R = al.rotation[0].cpu().numpy()
    assert float(np.abs(R.T @ R - np.eye(3)).max()) <= case.iters * ORTHO_BOUND and np.linalg.det(R) > 0          # (one step's bound per composition)
    assert torch.equal(al.translation[0], al.matrix[0, :3, 3])
    assert float(al.scale[0]) == 1.0 if not case.scale else abs(float(al.scale[0]) - 1.05) <= 2 * 2.0 ** -20          # (a row of s R: sqrt(3) entries' worth)
    assert _same(al.xyz, A.apply(al.matrix[:, :3].cpu().numpy(), case.source, case.start))
    assert bool(al.nearest.hit.all()) and float(al.nearest.dist2.max()) <= (2.0 ** -22) ** 2 * case.n


def _by_hand(hip, dev, case, iters, method, grid):
    """The sequence mvd_align_icp stands for, issued by the caller: mvd_nearest_points_stages(BUILD) once, then per row mvd_align_apply,
    mvd_nearest_points_stages(QUERY) and mvd_align_fit (with MVD_ALIGN_SCALE) on the pairs and distances the search left."""
    L, p = hip.lib(), hip.ptr
    out = _icp_buffers(hip, case, iters, method, grid)
    transform = _identity(case.nscene)
    nn_bytes = int(L.mvd_nearest_points_scratch(case.nt, case.nscene, method, grid))
    nn = _scratch(nn_bytes)
    search = lambda stages: hip.check(L.mvd_nearest_points_stages(p(out["moved"]), p(dev["start"]), p(dev["target"]), p(dev["tstart"]), case.n, case.nt,
                                                                  case.nscene, method, grid, p(out["index"]), p(out["dist2"]),
                                                                  p(nn) if nn_bytes else None, nn_bytes, stages, hip.stream()))
    search(hip.NN_BUILD)
    for k in range(iters + 1):
        hip.check(_apply(hip, dev["source"], dev["start"], case.n, case.nscene, transform, out["moved"]))
        search(hip.NN_QUERY)
        hip.check(_fit(hip, out["moved"], dev["start"], dev["target"], out["index"], out["dist2"], case.n, case.nt, case.nscene,
                       hip.ALIGN_SCALE | (0 if k < iters else hip.ALIGN_NO_STEP), INF, transform, out["history"][k]))
    torch.cuda.synchronize()
    return dict(out, transform=transform)


def _loop_is_the_sequence(hip, case, iters, method, grid):
    dev = _device(case)
    out, transform = _icp_buffers(hip, case, iters, method, grid), _identity(case.nscene)
    hip.check(_icp(hip, dev, case, out, transform, iters, hip.ALIGN_SCALE, INF, method, grid))
    torch.cuda.synchronize()
    hand = _by_hand(hip, dev, case, iters, method, grid)
    assert not bool((out["history"] == SENTINEL).any())
    assert _same(hand["transform"], transform)
    for k in ("moved", "index", "dist2"):
        assert _same(hand[k], out[k]), k
    assert _same(hand["history"][:, :, :2], out["history"][:, :, :2])
    # column 2, the scale so far: a fit called by hand starts every row from 1, the loop carries the row before on -- one IEEE multiply
    # per row, as al_finish forms it; the last row takes no step
    r = hand["history"][:, :, 2].cpu().numpy()
    carried = np.empty_like(r)
    carried[0] = r[0]
    for k in range(1, iters):
        carried[k] = carried[k - 1] * r[k]
    carried[iters] = carried[iters - 1]
    assert np.array_equal(carried.view(np.int64), out["history"][:, :, 2].cpu().numpy().view(np.int64))
    return out, transform


@pytest.mark.parametrize("method, grid", [("NN_AUTO", 0), ("NN_BRUTE", 0), ("NN_GRID", 9)])
def test_the_loop_is_the_sequence_it_stands_for(hip, method, grid):
    """mvd_align_icp against the caller-issued sequence, bit for bit, on icp_sim5 with a scale fitted: the carried scale is the one thing
    the point loop has that the plane loops have not."""
    case = A.make_case("icp_sim5")
    assert case.n == 1537 and case.scale
    out, transform = _loop_is_the_sequence(hip, case, 4, getattr(hip, method), grid)
    assert not torch.equal(transform, _identity(1)) and float(out["history"][-1, 0, 2]) != 1.0          # (a scale was fitted and carried)


def test_the_loop_is_the_sequence_with_empty_and_tiny_scenes(hip):
    """icp_sim5 in one batch with the scenes of 0, 1, 2 and 3 points of small_scenes: an empty scene and scenes with fewer than 3 pairs go
    through the same loop and keep the identity; three pairs are fitted."""
    a, b = A.make_case("icp_sim5"), A.make_case("small_scenes")
    assert b.start[:5] == [0, 0, 1, 3, 6]
    start = [0] + [a.n + v for v in b.start[:5]]
    case = A.Case(source=torch.cat([a.source, b.source[:6]]), start=start, target=torch.cat([a.target, b.target[:6]]), tstart=start)
    out, transform = _loop_is_the_sequence(hip, case, 2, hip.NN_AUTO, 0)
    hist = out["history"].cpu()
    assert torch.equal(transform[1:4].cpu(), _identity(3).cpu()) and not torch.equal(transform[0].cpu(), _identity(1)[0].cpu())
    assert not torch.equal(transform[4].cpu(), _identity(1)[0].cpu())
    assert hist[:, :, 1].tolist() == [[a.n, 0, 1, 2, 3]] * 3 and bool(torch.isnan(hist[:, 1, 0]).all()) and bool((hist[:, 1:4, 2] == 1.0).all())


def test_no_aligner_writes_into_its_init(hip):
    """``init`` is copied: a float64 (4, 4) matrix on the GPU, of which one scene's first three rows are contiguous as they lie, and the
    matrix of a previous result keep their bits through every aligner, whose result is another transform."""
    from mvdfusion_amd import fusion
    import meshdist_f64 as M
    n = 200
    src = A.bulged_ellipsoid(n, 8190)
    tgt = A.apply(A.similarity(1.0, 4.0, (1, -2, 0.5), (0.02, -0.01, 0.015))[:3][None], src, [0, n])
    src, tgt = src.cuda(), tgt.cuda()
    cube = M.make_case("cube")
    mesh = fusion.TriangleMesh(vertices=torch.from_numpy(cube.vertices).cuda(), faces=torch.from_numpy(cube.faces).cuda(), rgb=None,
                               vertex_start=torch.tensor([0, len(cube.vertices)], dtype=torch.int32),
                               face_start=torch.tensor([0, len(cube.faces)], dtype=torch.int32))
    aligners = dict(align_geometry=lambda init: fusion.align_geometry(src, tgt, iters=2, init=init),
                    align_to_surface=lambda init: fusion.align_to_surface(src, tgt, iters=2, init=init),
                    align_to_mesh=lambda init: fusion.align_to_mesh(src, mesh, iters=2, init=init))
    inits = dict(matrix=lambda: torch.from_numpy(A.similarity(1.0, 1.0, (0, 0, 1), (0.01, 0.0, -0.01))).cuda(),
                 alignment=lambda: fusion.align_geometry(src, tgt, iters=1),
                 registration=lambda: fusion.register_geometry(src, tgt, rotations=16, samples=64, candidates=2, refine_iters=2, iters=2))
    written = []
    for form, make in inits.items():
        for name, run in aligners.items():
            init = make()
            held = init if torch.is_tensor(init) else init.matrix
            assert held.dtype == torch.float64 and held.is_cuda
            before = held.clone()
            result = run(init)
            torch.cuda.synchronize()
            assert not torch.equal(result.matrix.reshape(4, 4), before.reshape(4, 4)), (form, name)          # (so the check below is not vacuous)
            if not _same(held, before):
                written.append((form, name))
    assert not written, written


# ------------------------------------------------------------------------------------------------ 4. determinism and batching
def test_runs_repeat_and_a_batch_equals_its_scenes(hip):
    from mvdfusion_amd import fusion
    a, b = A.make_case("icp_sim5"), A.make_case("icp_rigid10")
    fields = lambda al: dict(matrix=al.matrix, rms=al.rms, pairs=al.pairs, xyz=al.xyz, index=al.nearest.index, dist2=al.nearest.dist2,
                             rotation=al.rotation, translation=al.translation, scale=al.scale)
    singles = [fields(fusion.align_geometry(c.source.cuda(), c.target.cuda(), iters=30, scale=True)) for c in (a, b)]
    again = fields(fusion.align_geometry(a.source.cuda(), a.target.cuda(), iters=30, scale=True))
    for k, v in singles[0].items():
        assert _same(v, again[k]), k
    cloud = lambda x, y: fusion.SurfaceSamples(xyz=torch.cat([x, y]).cuda(), rgb=None, scene=torch.cat([torch.zeros(len(x)), torch.ones(len(y))]).long().cuda(),
                                               face=torch.zeros(len(x) + len(y), dtype=torch.int32).cuda(), bary=torch.zeros(len(x) + len(y), 3).cuda())
    for method in ("auto", "brute"):
        both = fields(fusion.align_geometry(cloud(a.source, b.source), cloud(a.target, b.target), scenes=2, iters=30, scale=True, method=method))
        for k in ("matrix", "rotation", "translation", "scale"):
            assert _same(both[k], torch.cat([s[k] for s in singles])), (method, k)
        for k in ("rms", "pairs"):
            assert _same(both[k], torch.cat([s[k] for s in singles], dim=1)), (method, k)
        assert _same(both["xyz"], torch.cat([s["xyz"] for s in singles])) and _same(both["dist2"], torch.cat([s["dist2"] for s in singles]))
        assert torch.equal(both["index"], torch.cat([singles[0]["index"], singles[1]["index"] + a.nt]))


def test_a_scene_of_more_than_two_solve_tiles(hip):
    """The per-scene sum stages the chunk sums through LDS kSolveTile chunks at a time: a scene of 2 * kSolveTile * chunk + 1 rows goes
    round that loop three times, the last time for one chunk of one row.  A small scene sits behind it.  Against the oracle, and the
    batch against each scene alone, bit for bit.  The step's bound at this size: the derivation's n 2^-53 * 8 * 2.5 is 5.8e-10 at
    n = 262 145, above 2^-32, so the bound here is 20 n 2^-53; rms and pairs as everywhere."""
    import os
    import re
    src_text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mvdfusion_amd", "csrc", "align.hip")).read()
    tile = int(re.search(r"kSolveTile = (\d+);", src_text).group(1))
    big, small = 2 * tile * hip.ALIGN_CHUNK + 1, 777
    assert big > 2 * 128 * 1024
    src = A.bulged_ellipsoid(big + small, 8120)
    truth = [A.TRUTH_PAIRS, A.similarity(0.9, 25.0, (2, -1, 1), (0.05, 0.1, -0.2))]
    start = [0, big, big + small]
    tgt = A.apply(np.stack([t[:3] for t in truth]), src, start)
    case = A.Case(source=src, start=start, target=tgt, tstart=start, truth=truth)
    ref = A.fit_ref(case)

    def run(rows, nscene, offsets):
        moved, target = src[rows].contiguous().cuda(), tgt[rows].contiguous().cuda()
        transform, row = _identity(nscene), torch.full((nscene, 3), SENTINEL, dtype=torch.float64, device="cuda")
        hip.check(_fit(hip, moved, _i32(offsets), target, None, None, moved.shape[0], target.shape[0], nscene, hip.ALIGN_SCALE, INF, transform, row))
        return transform.cpu(), row.cpu()

    both = run(slice(0, big + small), 2, start)
    alone = [run(slice(0, big), 1, [0, big]), run(slice(big, big + small), 1, [0, small])]
    again = run(slice(0, big + small), 2, start)
    assert _same(both[0], again[0]) and _same(both[1], again[1])
    for k in range(2):
        assert _same(both[0][k], alone[k][0][0]) and _same(both[1][k], alone[k][1][0]), k
        n = (big, small)[k]
        bound = max(STEP_BOUND, 20 * n * 2.0 ** -53)
        assert int(both[1][k, 1]) == ref.pairs[k] == n
        _check_rms(float(both[1][k, 0]), ref.sums[k])
        _check_step("solve_tiles", case, k, both[0][k].numpy(), float(both[1][k, 2]), ref.steps[k], bound)
        assert float(np.abs(both[0][k].numpy().reshape(3, 4) - truth[k][:3]).max()) <= 2.0 ** -20


def test_rows_paired_by_position_equal_an_explicit_arange(hip):
    case = A.make_case("pairs_4099")
    dev = _device(case)
    got = []
    for index in (None, torch.arange(case.n, dtype=torch.int32).cuda()):
        transform, row = _identity(1), torch.full((1, 3), SENTINEL, dtype=torch.float64, device="cuda")
        hip.check(_fit(hip, dev["source"], dev["start"], dev["target"], index, None, case.n, case.nt, 1, hip.ALIGN_SCALE, INF, transform, row))
        got.append((transform, row))
    assert _same(got[0][0], got[1][0]) and _same(got[0][1], got[1][1])


# ------------------------------------------------------------------------------------------------ 5. iters = 0, the centroid start
def test_no_iteration_returns_the_start_and_the_centroid_start_is_the_float64_map(hip):
    from mvdfusion_amd import fusion
    case = A.make_case("pairs_4099")
    src, tgt = case.source.cuda(), case.target.cuda()
    T = torch.from_numpy(A.similarity(1.2, 30.0, (1, 2, 3), (0.1, -0.1, 0.0)))
    al = fusion.align_geometry(src, tgt, iters=0, init=T, scale=True)
    assert torch.equal(al.matrix[0].cpu(), T) and al.rms.shape == al.pairs.shape == (1, 1) and abs(float(al.scale[0]) - 1.2) <= 1e-14
    assert _same(al.xyz, A.apply(T[:3].numpy()[None], case.source, case.start))
    ref = fusion.nearest_points(al.xyz, tgt)
    assert torch.equal(ref.index, al.nearest.index) and _same(ref.dist2, al.nearest.dist2) and int(al.pairs[0, 0]) == case.n
    assert abs(float(al.rms[0, 0]) - float(ref.dist2.double().mean().sqrt())) <= 1e-12
    p, q = case.source.double().numpy(), case.target.double().numpy()
    for scale in (False, True):
        al = fusion.align_geometry(src, tgt, iters=0, init="centroid", scale=scale)
        k = np.sqrt(((q - q.mean(0)) ** 2).sum(1).mean() / ((p - p.mean(0)) ** 2).sum(1).mean()) if scale else 1.0
        m = al.matrix[0].cpu().numpy()
        assert np.abs(m[:3, :3] - k * np.eye(3)).max() <= 1e-12 and np.abs(m[:3, 3] - (q.mean(0) - k * p.mean(0))).max() <= 1e-12
        assert abs(float(al.scale[0]) - k) <= 1e-12 and (scale or float(al.scale[0]) == 1.0)
    # fit_similarity: the closed form through the host path, against the oracle
    fit, ref = fusion.fit_similarity(src, tgt), A.fit_refs("pairs_4099")
    s0, R0, t0 = ref.steps[0]
    assert float((fit.matrix[0].cpu() - torch.from_numpy(A.step_matrix(s0, R0, t0))).abs().max()) <= STEP_BOUND * 3          # ((1 + s) bound per entry of s R)
    assert abs(float(fit.scale[0]) - s0) <= STEP_BOUND * s0 and fit.rms.shape == (1, 1) and int(fit.pairs[0, 0]) == case.n
    assert float(fit.rms[0, 0]) <= 2.0 ** -22 and fit.nearest.index.tolist() == list(range(case.n))
    assert _same(fit.xyz, A.apply(fit.matrix[:, :3].cpu().numpy(), case.source, case.start))
    assert _same(fit.nearest.dist2, A.d2_rows(fit.xyz.cpu(), case.target))


# ------------------------------------------------------------------------------------------------ 6. every element, refusals
def test_outputs_are_fully_written_and_refusals_write_nothing(hip):
    L = hip.lib()
    case = A.make_case("small_scenes")
    dev = _device(case)
    out = _icp_buffers(hip, case, 2, hip.NN_GRID, 7)
    transform = _identity(case.nscene)
    hip.check(_icp(hip, dev, case, out, transform, 2, hip.ALIGN_SCALE, INF, hip.NN_GRID, 7))
    torch.cuda.synchronize()
    hist = out["history"].cpu()
    assert not bool((hist == SENTINEL).any()) and not bool((out["moved"][:case.n] == SENTINEL).any()) and not bool((out["index"][:case.n] == -5).any())
    assert not bool((out["dist2"][:case.n] == SENTINEL).any())
    assert bool(torch.isnan(hist[:, 0, 0]).all()) and bool((hist[:, 0, 1] == 0).all()) and hist[:, 1:, 1].tolist() == [[1, 2, 3, 500]] * 3
    assert torch.equal(transform[:3].cpu(), _identity(3).cpu()) and not torch.equal(transform[3:].cpu(), _identity(2).cpu())
    # refusals
    out = _icp_buffers(hip, case, 2, hip.NN_GRID, 7)
    transform = torch.full((case.nscene, 12), SENTINEL, dtype=torch.float64, device="cuda")
    odd = ctypes.c_void_p(out["scratch"].data_ptr() + 8)
    bad = [dict(source=None), dict(start=None), dict(target=None), dict(tstart=None), dict(transform=None), dict(history=None), dict(moved=None),
           dict(index=None), dict(dist2=None), dict(scratch=None), dict(nscene=0), dict(nscene=65536), dict(iters=-1), dict(iters=1025),
           dict(flags=2), dict(flags=4), dict(flags=-1), dict(method=3), dict(method=-1), dict(grid=-1), dict(grid=257), dict(max_d2=-1.0),
           dict(max_d2=float("nan")), dict(nq=1 << 31), dict(nt=1 << 31), dict(nbytes=out["nbytes"] - 16), dict(nbytes=0), dict(scratch=odd),
           dict(nscene=65535, grid=256, method=hip.NN_GRID, nbytes=1 << 62), dict(transform=ctypes.c_void_p(transform.data_ptr() + 4))]
    for kw in bad:
        assert _icp(hip, dev, case, out, transform, 2, hip.ALIGN_SCALE, INF, hip.NN_GRID, 7, kw=kw) != 0, kw
        assert b"mvd_align_icp" in L.mvd_last_error(), (kw, L.mvd_last_error())
    row = torch.full((case.nscene, 3), SENTINEL, dtype=torch.float64, device="cuda")
    need = int(L.mvd_align_scratch(case.n, 0, case.nscene, hip.NN_BRUTE, 0))
    fit = lambda **kw: _fit(hip, **{**dict(moved=dev["source"], start=dev["start"], target=dev["target"], index=None, dist2=None, n=case.n, nt=case.nt,
                                           nscene=case.nscene, flags=0, max_d2=INF, transform=transform, row=row, scratch=out["scratch"]), **kw})
    for kw in (dict(moved=None), dict(start=None), dict(target=None), dict(transform=None), dict(row=None), dict(nscene=0), dict(nscene=65536),
               dict(flags=4), dict(flags=-1), dict(max_d2=-0.5), dict(max_d2=float("nan")), dict(n=1 << 31), dict(nt=1 << 31), dict(nbytes=need - 8),
               dict(nbytes=0)):
        assert fit(**kw) != 0 and b"mvd_align_fit" in L.mvd_last_error(), (kw, L.mvd_last_error())
    moved = out["moved"]
    for kw in (dict(src=None), dict(start=None), dict(transform=None), dict(out=None), dict(nscene=0), dict(nscene=65536), dict(n=1 << 31)):
        a = dict(src=dev["source"], start=dev["start"], n=case.n, nscene=case.nscene, transform=transform, out=moved)
        a.update(kw)
        assert _apply(hip, **a) != 0 and b"mvd_align_apply" in L.mvd_last_error(), (kw, L.mvd_last_error())
    torch.cuda.synchronize()
    assert bool((out["history"] == SENTINEL).all()) and bool((out["moved"] == SENTINEL).all()) and bool((out["index"] == -5).all())
    assert bool((out["dist2"] == SENTINEL).all()) and bool((out["scratch"] == 0x1234).all()) and bool((transform == SENTINEL).all())
    assert bool((row == SENTINEL).all())
    # empty sides are valid calls
    empty = A.Case(source=torch.zeros(0, 3), start=[0, 0], target=case.target, tstart=[0, case.nt])
    out = _icp_buffers(hip, empty, 1, hip.NN_AUTO, 0)
    transform = _identity(1)
    assert _icp(hip, dict(_device(empty), source=None), empty, out, transform, 1, 0, INF, kw=dict(moved=None, index=None, dist2=None)) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out["history"][:, 0, 0]).all()) and bool((out["history"][:, 0, 1] == 0).all()) and torch.equal(transform, _identity(1))
    none = A.Case(source=case.source, start=[0, case.n], target=torch.zeros(0, 3), tstart=[0, 0])
    out = _icp_buffers(hip, none, 1, hip.NN_AUTO, 0)
    assert _icp(hip, dict(_device(none), target=None), none, out, transform, 1, 0, INF) == 0
    torch.cuda.synchronize()
    assert bool((out["index"] == -1).all()) and bool((out["history"][:, 0, 1] == 0).all()) and torch.equal(transform, _identity(1))


# ------------------------------------------------------------------------------------------------ 7. Alignment.apply
def test_alignment_apply_moves_every_geometry_type_by_the_rule(hip, icp_runs):
    from mvdfusion_amd import fusion
    case = A.make_case("icp_rigid10")
    al = icp_runs["icp_rigid10"]
    src, tgt = case.source.cuda(), case.target.cuda()
    want = A.apply(al.matrix[:, :3].cpu().numpy(), case.source, case.start)
    assert _same(al.apply(src), want) and _same(al.apply(src), al.xyz)
    n = case.n
    z = torch.zeros(n, dtype=torch.int64, device="cuda")
    cloud = fusion.PointCloud(xyz=src, rgb=torch.rand(n, 3, device="cuda"), support=z.to(torch.uint8), scene=z, view=z, pixel=torch.zeros(n, 2, dtype=torch.int64).cuda(),
                              index=z.to(torch.int32))
    samples = fusion.SurfaceSamples(xyz=src, rgb=None, scene=z, face=z.to(torch.int32), bary=torch.zeros(n, 3, device="cuda"))
    mesh = fusion.TriangleMesh(vertices=src, faces=torch.arange(3 * (n // 3), dtype=torch.int32).reshape(-1, 3).cuda(), rgb=cloud.rgb,
                               vertex_start=torch.tensor([0, n], dtype=torch.int32), face_start=torch.tensor([0, n // 3], dtype=torch.int32))
    for geometry, key in ((cloud, "xyz"), (samples, "xyz"), (mesh, "vertices")):
        out = al.apply(geometry)
        assert type(out) is type(geometry) and _same(getattr(out, key), want)
        for f in dataclasses.fields(geometry):
            assert f.name == key or getattr(out, f.name) is getattr(geometry, f.name), f.name
    before = fusion.compare_geometry(src, tgt, threshold=1e-4)
    after = fusion.compare_geometry(al.apply(cloud), tgt, threshold=1e-4)
    print(f"icp_rigid10: chamfer {float(before.chamfer):.4f} -> {float(after.chamfer):.2e}, fscore at 1e-4 {float(before.fscore):.4f} -> {float(after.fscore):.1f}")
    assert float(before.fscore) < 0.05 and float(after.chamfer) <= 2 * 2.0 ** -22 and float(after.fscore) == 1.0
    # two scenes, the second of which is left where it is
    two = dataclasses.replace(al, matrix=torch.cat([al.matrix, torch.eye(4, dtype=torch.float64, device="cuda")[None]]))
    both = dataclasses.replace(samples, xyz=torch.cat([src, src]), scene=torch.cat([z, z + 1]), face=torch.cat([samples.face] * 2), bary=torch.cat([samples.bary] * 2))
    moved = two.apply(both).xyz
    assert _same(moved[:n], want) and _same(moved[n:], src)
    with pytest.raises(ValueError):
        two.apply(src)
