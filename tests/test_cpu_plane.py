"""The point-to-plane entries without a GPU: mvd_plane_solve -- the very solve of the kernel, on the host -- against the float64 oracle of
tests/plane_f64.py (numpy.linalg.eigh) on the oracle's sums of every case, the oracle's own ICP held to what the cases are for (where
the figures quoted in tests/test_gpu_plane.py come from), header, binding and constants, and the host side of fusion.fit_plane_step
and fusion.align_to_surface against stub enqueues.

Bounds -- none taken from what the library gives:
  step            |D - D_oracle|_max <= 128 * 2^-53 * kappa * |g| / lambda_min_kept + 32 * 2^-53 (plane_f64.solve_bound has the derivation);
                  |R^T R - I| <= 32 * 2^-53 and det R > 0; the rank EQUAL, every eigenvalue of every case a factor 16 clear of
                  MVD_PLANE_EPS_RANK * lambda_max on either side, asserted on the oracle.
  left alone      the step's component along every direction the oracle drops: at most the step bound + 2^-40 (plane target: in-plane
                  translation and the rotation about the normal; sphere: the three rotations about its centre).
  ICP, exact      final correspondences = the permutation; |M - truth| <= 2^-20; last plane rms and rms <= 2^-22; all right within
                  iters / 2.
  ICP, sliding    the oracle's point-to-plane |M - truth| at most 1 / 20 of the oracle's point-to-point |M - truth|.

Measured: step error at most 7.6e-16 (bounds 1.6e-14 .. 1.7e-12; offset case 1.2e-12 of 3.1e-3, its kappa being 2e5); exact partners:
every correspondence right from iteration 2 of 30, |M - truth| 2.2e-10; sliding: 7.9e-4 against point-to-point's 6.1e-2, 1 / 77.
"""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import align_f64 as A
import plane_f64 as P
from mvdfusion_amd import fusion, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORTHO_BOUND = 32 * 2.0 ** -53


def lib_solve(sums):
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    step, rank = np.full(12, -7.25), ctypes.c_int(-1)
    assert hip.lib().mvd_plane_solve(sums.ctypes.data_as(ctypes.c_void_p), step.ctypes.data_as(ctypes.c_void_p), ctypes.byref(rank)) == 0
    return step.reshape(3, 4), rank.value


def small_motion(D):
    """(omega, t) of a step by the first-order log map: vee(R - R^T) / 2 = omega sin(a) / a, exact to a^2 / 6 relative."""
    R = D[:, :3]
    return np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 2 * D[0, 3], 2 * D[1, 3], 2 * D[2, 3]]) / 2


# ------------------------------------------------------------------------------------------------ the solve
@pytest.mark.parametrize("name", list(P.FIT_CASES))
def test_the_host_solve_meets_the_oracle_on_its_sums(name):
    ref = P.fit_refs(name)
    for s, (sums, sol) in enumerate(zip(ref.sums, ref.solves)):
        D, rank = lib_solve(sums)
        want = np.concatenate([sol.R, sol.t[:, None]], axis=1)
        R = D[:, :3]
        assert rank == sol.rank == ref.case.rank[s] and int(sums[0]) == int(ref.accepted[ref.case.base.start[s]:ref.case.base.start[s + 1]].sum())
        if sol.rank == 0:
            assert np.array_equal(D, np.eye(3, 4)) and sums[0] < 3          # the exact identity
            continue
        kept = sol.lam > P.EPS_RANK * sol.lam.max()
        bound = P.solve_bound(sol.lam, kept, P.unpack(sums)[1])
        err, clear = float(np.abs(D - want).max()), P.clearance(sol.lam)
        print(f"{name} scene {s}: pairs {int(sums[0])} rank {rank} kappa {sol.lam.max() / sol.lam[kept].min():.3g} clearance {clear:.3g} | "
              f"step error {err:.3g} (bound {bound:.3g}) | |R^T R - I| {float(np.abs(R.T @ R - np.eye(3)).max()):.2g}")
        assert clear >= P.CLEAR and err <= bound
        assert float(np.abs(R.T @ R - np.eye(3)).max()) <= ORTHO_BOUND and np.linalg.det(R) > 0
        if rank < 6:          # what the data does not constrain is left alone
            null = np.linalg.eigh(P.unpack(sums)[0])[1][:, :6 - rank]
            along = float(np.abs(null.T @ small_motion(D)).max())
            print(f"  along the {6 - rank} dropped directions: {along:.3g}")
            assert along <= bound + 2.0 ** -40
        if name == "plane":   # in-plane translation and the rotation about the normal (0, 0, 1)
            x = small_motion(D)
            assert max(abs(x[2]), abs(x[3]), abs(x[4])) < 2.0 ** -40 and abs(x[5]) > 1e-3
    if name == "gate":        # pairs exactly at the threshold are in
        base = ref.case.base
        at = base.dist2 == torch.tensor(base.max_d2)
        assert int(at.sum()) > 0 and bool(ref.accepted[at].all()) and 0 < int(ref.accepted.sum()) < base.n
    if name == "invalid_normals":
        bad = ~(torch.isfinite(ref.case.normals).all(1) & (ref.case.normals != 0).any(1))
        assert int(bad.sum()) == 45 and not bool(ref.accepted[bad].any()) and bool(ref.accepted[~bad].all())
    if name == "nonfinite":
        assert int(ref.sums[0, 0]) == 940
    if name == "chunk_edges":
        assert np.diff(ref.case.base.start).tolist() == [A.CHUNK - 1, A.CHUNK, A.CHUNK + 1, 2 * A.CHUNK + 1]


def test_what_cannot_be_solved_gives_the_exact_identity():
    good = P.fit_refs("generic").sums[0]
    cases = []
    for k in (0, 5, 22, 28, 29):
        for v in (float("nan"), float("inf")):
            bad = good.copy()
            bad[k] = v
            cases.append(bad)
    for n in (0.0, 1.0, 2.0, 2.5):
        few = good.copy()
        few[0] = n
        cases.append(few)
    flat = np.zeros(P.SUMS)
    flat[0] = 10.0
    cases.append(flat)                                     # lambda_max is not positive
    for sums in cases:
        D, rank = lib_solve(sums)
        assert np.array_equal(D, np.eye(3, 4)) and rank == 0
    L = hip.lib()
    assert L.mvd_plane_solve(None, None, None) != 0 and b"mvd_plane_solve" in L.mvd_last_error()


def test_a_large_step_is_still_a_proper_rotation():
    """g scaled up until the step is a rotation of several radians: the quaternion keeps R proper; below the series threshold too."""
    sums = P.fit_refs("generic").sums[0].copy()
    for factor in (1e-9, 1e-3, 1.0, 30.0, 1e3):
        s = sums.copy()
        s[22:28] *= factor
        D, rank = lib_solve(s)
        R = D[:, :3]
        want = P.solve(s)
        assert rank == 6 and float(np.abs(R.T @ R - np.eye(3)).max()) <= ORTHO_BOUND and np.linalg.det(R) > 0
        assert float(np.abs(R - want.R).max()) <= 1e-9 * max(1.0, float(np.abs(want.x).max()))          # the same rotation, any angle


# ------------------------------------------------------------------------------------------------ the oracle's ICP
def test_exact_partners_converge_to_the_permutation():
    ref = P.icp_refs("icp_exact")
    case = ref.case
    iters = case.iters
    err = float(np.abs(ref.matrix - case.truth).max())
    first = int(np.argmax(ref.right == case.base.n))
    print(f"exact partners: n {case.base.n} iters {iters}, every correspondence right from iteration {first}, |M - truth| {err:.3g}, "
          f"last plane rms {ref.history[-1, 0]:.3g} rms {ref.history[-1, 2]:.3g}, rank {ref.history[:, 3].tolist()[:3]}.., clearance {ref.worst_clearance:.3g}")
    assert bool((ref.index == case.base.perm).all()) and ref.right[-1] == case.base.n and (ref.right[first:] == case.base.n).all()
    assert first <= iters // 2 and err <= 2.0 ** -20 and ref.history[-1, 0] <= 2.0 ** -22 and ref.history[-1, 2] <= 2.0 ** -22
    assert (ref.history[:, 3] == 6).all() and (ref.history[:, 1] == case.base.n).all() and ref.worst_clearance >= P.CLEAR


def test_point_to_plane_does_not_slide_where_point_to_point_does():
    ref = P.icp_refs("icp_sliding")
    case = ref.case
    plane = float(np.abs(ref.matrix - case.truth).max())
    point = float(np.abs(A.icp(case.base, iters=case.iters).matrix - case.truth).max())
    settled = int(np.argmax(np.abs(ref.history[:, 0] - ref.history[-1, 0]) <= 0.01 * ref.history[-1, 0]))
    print(f"sliding: n {case.base.n} iters {case.iters}: |M - truth| point-to-point {point:.4g}, point-to-plane {plane:.4g} (1 / {point / plane:.0f}), "
          f"plane rms within 1 % of its last value from iteration {settled}; last row {ref.history[-1].tolist()}")
    assert plane <= point / 20 and ref.worst_clearance >= P.CLEAR and (ref.history[:, 3] == 6).all()
    assert not bool((case.base.source[:, None] == case.base.target[None]).all(2).any())          # no point of one side is one of the other


# ------------------------------------------------------------------------------------------------ header, binding, constants
def test_the_header_and_the_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    consts = dict(re.findall(r"#define\s+MVD_PLANE_(\w+)\s+(\S+)", hdr))
    assert consts == dict(NO_STEP=str(hip.PLANE_NO_STEP), SUMS=str(hip.PLANE_SUMS), HISTORY=str(hip.PLANE_HISTORY), EPS_RANK="1e-9")
    assert float(consts["EPS_RANK"]) == hip.PLANE_EPS_RANK == P.EPS_RANK and (hip.PLANE_SUMS, hip.PLANE_HISTORY) == (P.SUMS, P.HISTORY)
    assert hip.PLANE_NO_STEP == hip.ALIGN_NO_STEP
    for name, count in (("mvd_plane_scratch", 5), ("mvd_plane_solve", 3), ("mvd_plane_fit", 16), ("mvd_plane_icp", 20)):
        decl = re.search(r"^\w+ " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
        assert decl is not None and name in hip.SIGNATURES, name
        assert len(hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == count, name
    src = open(os.path.join(ROOT, "mvdfusion_amd", "csrc", "align.hip")).read()
    # one copy of the reduction: both fits go through the same two kernels and the same chunk map
    assert src.count("void accumulate_kernel(") == 1 and src.count("void solve_kernel(") == 1 and src.count("void chunk_count_kernel(") == 1
    assert "al_fit<PlaneFit>(" in src and "al_icp<PlaneFit>(" in src and src.count("al_launch_fit<Fit>(") == 2 and "atomicAdd" not in src
    assert src.count("k <= iters") == 1          # one host loop for the three ICP entries
    L = hip.lib()
    assert int(L.mvd_plane_scratch(5000, 0, 3, hip.NN_BRUTE, 0)) >= (5 + 3) * 30 * 8 + 4 * 4
    assert int(L.mvd_plane_scratch(5000, 5000, 1, hip.NN_GRID, 7)) >= int(L.mvd_plane_scratch(5000, 0, 1, hip.NN_BRUTE, 0)) + \
        int(L.mvd_nearest_points_scratch(5000, 1, hip.NN_GRID, 7))
    for args in ((100, 100, 0, 0, 0), (100, 100, 65536, 0, 0), (100, 100, 1, 3, 0), (100, 100, 1, 0, 257), (1 << 31, 100, 1, 0, 0)):
        assert int(L.mvd_plane_scratch(*args)) == 0, args


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

    def apply(xyz, start, N, transform):
        calls.append(dict(fn="apply", xyz=xyz, transform=transform.clone()))
        return xyz + 1.0

    def plane_fit(moved, start, target, normals, index, N, flags, max_d2, transform):
        calls.append(dict(fn="plane_fit", moved=moved, start=start, target=target, normals=normals, index=index, N=N, flags=flags, max_d2=max_d2))
        if not flags & hip.PLANE_NO_STEP:
            transform[:, 3] += 0.5
        return torch.tensor([[0.125, 3.0, 0.5, 6.0]], dtype=torch.float64).repeat(N, 1)

    def plane_icp(source, source_start, target, target_start, normals, N, method, grid, iters, max_d2, transform):
        calls.append(dict(fn="plane_icp", source=source, source_start=source_start, target=target, target_start=target_start, normals=normals, N=N,
                          method=method, grid=grid, iters=iters, max_d2=max_d2, transform=transform.clone()))
        n = source.shape[0]
        transform[:, 3] += 0.25
        history = torch.tensor([0.125, float(n), 0.5, 5.0], dtype=torch.float64).repeat(iters + 1, N, 1)
        return history, source + 1.0, torch.arange(n, dtype=torch.int32), torch.full((n,), 0.0625)

    def align_icp(source, source_start, target, target_start, N, method, grid, iters, flags, max_d2, transform):
        calls.append(dict(fn="icp", iters=iters))
        n = source.shape[0]
        transform[:, 7] += 2.0
        return torch.tensor([0.25, float(n), 1.0], dtype=torch.float64).repeat(iters + 1, N, 1), source + 1.0, torch.arange(n, dtype=torch.int32), \
            torch.full((n,), 0.0625)

    def knn(query, query_start, target, target_start, N, k, method, grid):
        calls.append(dict(fn="knn", k=k, N=N, target=target, query=query, method=method))
        return torch.zeros(query.shape[0], k, dtype=torch.int32), torch.zeros(query.shape[0], k)

    def normals(target, index, points, toward):
        calls.append(dict(fn="normals", index=index, toward=toward))
        return torch.full((index.shape[0], 3), 0.5), torch.zeros(index.shape[0])

    for name, fn in (("_align_apply", apply), ("_plane_fit", plane_fit), ("_plane_icp", plane_icp), ("_align_icp", align_icp), ("_knn", knn),
                     ("_normals", normals)):
        monkeypatch.setattr(fusion, name, fn)
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("the library was touched"))
    return calls


@pytest.fixture
def no_host_reads(monkeypatch):
    for name in ("item", "cpu", "tolist", "numpy", "__bool__", "__float__", "__int__", "__index__"):
        monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _n=name, **k: pytest.fail(f"Tensor.{_n}() was called"), raising=True)


def test_align_to_surface_validates_and_enqueues(stub):
    a, b = _cloud([0, 0, 1, 1, 1, 2]), _cloud([0, 2, 2, 2], seed=1)
    mesh = fusion.TriangleMesh(vertices=torch.rand(3, 3), faces=torch.tensor([[0, 1, 2]], dtype=torch.int32), rgb=None,
                               vertex_start=torch.tensor([0, 3], dtype=torch.int32), face_start=torch.tensor([0, 1], dtype=torch.int32))
    bad = [(dict(scenes=0), "scenes = 0"), (dict(scenes=2), "scenes"), (dict(iters=-1), "iters = -1"), (dict(iters=1025), "iters = 1025"),
           (dict(iters=2.5), "iters = 2.5"), (dict(max_distance=-1.0), "max_distance = -1.0"), (dict(k=2), "at least 3 neighbours"),
           (dict(k=33), r"k = 33: an integer in \[1, 32\]"), (dict(normals=torch.rand(5, 3)), r"normals: None, a PointNormals or an \(4, 3\) tensor"),
           (dict(normals="pca"), "normals"), (dict(init="pca"), "init = 'pca'"), (dict(init=torch.eye(3)), "init"), (dict(method="kdtree"), "method"),
           (dict(grid=0), "grid = 0"), (dict(source=mesh), "sample_mesh"), (dict(target=mesh), "sample_mesh"), (dict(source=torch.rand(6, 2)), "source")]
    for kw, message in bad:
        args = dict(source=a, target=b, scenes=3)
        args.update(kw)
        with pytest.raises(ValueError, match=message):
            fusion.align_to_surface(**args)
    assert not stub                                         # nothing reached the library
    al = fusion.align_to_surface(a, b, scenes=3, max_distance=0.25, method="grid", grid=9)
    search, made, icp = stub
    assert (search["fn"], search["k"], search["N"], search["method"]) == ("knn", 16, 3, hip.NN_GRID) and search["query"] is search["target"]
    assert torch.equal(search["target"], b.xyz) and made["fn"] == "normals" and made["toward"] is None          # estimate_normals(target, k)
    assert icp["fn"] == "plane_icp" and (icp["N"], icp["method"], icp["grid"], icp["iters"], icp["max_d2"]) == (3, hip.NN_GRID, 9, fusion.ALIGN_ITERS, 0.0625)
    assert icp["source_start"].tolist() == [0, 2, 5, 6] and icp["target_start"].tolist() == [0, 1, 1, 4] and icp["normals"].shape == (4, 3)
    assert torch.equal(icp["transform"], torch.eye(3, 4, dtype=torch.float64).reshape(1, 12).repeat(3, 1))
    assert isinstance(al, fusion.PlaneAlignment) and isinstance(al, fusion.Alignment)
    assert [f.name for f in dataclasses.fields(al)] == [f.name for f in dataclasses.fields(fusion.Alignment)] + ["plane_rms", "rank"]
    assert al.rms.shape == al.plane_rms.shape == al.pairs.shape == al.rank.shape == (fusion.ALIGN_ITERS + 1, 3)
    assert float(al.rms[0, 0]) == 0.5 and float(al.plane_rms[0, 0]) == 0.125 and al.rank.dtype == al.pairs.dtype == torch.int64 and int(al.rank[0, 0]) == 5
    assert torch.equal(al.translation, torch.tensor([[0.25, 0.0, 0.0]] * 3, dtype=torch.float64)) and torch.equal(al.scale, torch.ones(3, dtype=torch.float64))
    assert torch.equal(al.xyz, a.xyz + 1.0) and al.nearest.index.dtype == torch.int32
    assert torch.equal(al.apply(a).xyz, a.xyz + 1.0) and stub[-1]["fn"] == "apply"                            # Alignment.apply, unchanged
    # given normals: no search.  iters = 0 returns init with its one history row.  A scale in init is carried through untouched
    given = torch.rand(4, 3)
    start = torch.eye(4, dtype=torch.float64)
    start[:3, :3] *= 2.0
    del stub[:]
    al = fusion.align_to_surface(a, b, normals=given, scenes=3, iters=0, init=start)
    assert [c["fn"] for c in stub] == ["plane_icp"] and torch.equal(stub[0]["normals"], given) and stub[0]["iters"] == 0
    assert torch.equal(stub[0]["transform"][:, [0, 5, 10]], torch.full((3, 3), 2.0, dtype=torch.float64)) and al.rms.shape == (1, 3)
    assert torch.equal(al.scale, torch.full((3,), 2.0, dtype=torch.float64)) and torch.equal(al.rotation, torch.eye(3, dtype=torch.float64).expand(3, 3, 3))
    pn = fusion.PointNormals(normal=given, variation=torch.zeros(4), valid=torch.ones(4, dtype=torch.bool), neighbours=None)
    fusion.align_to_surface(a, b, normals=pn, scenes=3, iters=2)
    assert torch.equal(stub[-1]["normals"], given) and stub[-1]["iters"] == 2
    for text in ("larger basin", "init=align_geometry(source, target, iters=5)", "RIGID", "sample_normals"):
        assert text in fusion.align_to_surface.__doc__, text


def test_fit_plane_step_validates_and_enqueues(stub):
    a, b = _cloud([0, 0, 1, 1, 1, 2]), _cloud([0, 0, 1, 1, 1, 2], seed=1)
    nrm = torch.rand(6, 3)
    bad = [dict(scenes=0), dict(scenes=2), dict(normals=None), dict(normals=torch.rand(5, 3)), dict(target=_cloud([0, 0, 1])),
           dict(pairs=torch.zeros(6, dtype=torch.int64)), dict(pairs=torch.zeros(5, dtype=torch.int32)), dict(pairs=[0] * 6), dict(source=torch.rand(6, 2))]
    for kw in bad:
        args = dict(source=a, target=b, normals=nrm, scenes=3)
        args.update(kw)
        with pytest.raises(ValueError):
            fusion.fit_plane_step(**args)
    assert not stub
    al = fusion.fit_plane_step(a, b, nrm, scenes=3)
    assert [c["fn"] for c in stub] == ["plane_fit", "apply", "plane_fit"]
    first, moved, last = stub
    assert first["flags"] == 0 and last["flags"] == hip.PLANE_NO_STEP and first["max_d2"] == float("inf") and first["index"] is None
    assert first["start"].tolist() == [0, 2, 5, 6] and torch.equal(first["normals"], nrm) and torch.equal(first["moved"], a.xyz)
    assert torch.equal(last["moved"], a.xyz + 1.0) and float(moved["transform"][0, 3]) == 0.5
    assert isinstance(al, fusion.PlaneAlignment) and al.rms.shape == al.plane_rms.shape == al.rank.shape == (1, 3) and al.rank.tolist() == [[6] * 3]
    assert al.pairs.tolist() == [[3] * 3] and torch.equal(al.xyz, a.xyz + 1.0) and al.nearest.index.tolist() == list(range(6))
    pairs = torch.tensor([3, -1, 0, 7, 2, 1], dtype=torch.int32)
    al = fusion.fit_plane_step(a.xyz, b.xyz[:4], nrm[:4], pairs=pairs)
    assert torch.equal(stub[-3]["index"], pairs) and al.nearest.index.tolist() == [3, -1, 0, -1, 2, 1]


def test_the_recipe_runs_without_a_host_synchronisation(stub, no_host_reads):
    """align_geometry(iters=5) -> align_to_surface(init=...): bare tensors, every enqueue stubbed, every Tensor read-back a failure."""
    src, tgt = torch.rand(50, 3), torch.rand(60, 3)
    coarse = fusion.align_geometry(src, tgt, iters=5)
    fine = fusion.align_to_surface(src, tgt, init=coarse, iters=7)
    assert [c["fn"] for c in stub] == ["icp", "knn", "normals", "plane_icp"] and stub[0]["iters"] == 5 and stub[3]["iters"] == 7
    start = stub[3]["transform"]
    assert start.shape == (1, 12) and torch.equal(start, coarse.matrix[:, :3, :].reshape(1, 12))          # the coarse result, taken unread
    again = fusion.align_to_surface(src, tgt, init=fine, iters=1, normals=torch.rand(60, 3))                # a PlaneAlignment is an init too
    assert torch.equal(stub[-1]["transform"], fine.matrix[:, :3, :].reshape(1, 12)) and again.rank.shape == (2, 1)
