"""The alignment without a GPU: the float64 oracle's own figures on every case of tests/align_f64.py (the numbers tests/test_gpu_align.py
quotes), the library's solve run on the host (mvd_align_solve is the very function the kernel calls) against the SVD oracle, header,
binding and constants, and the host side of fusion.fit_similarity, fusion.align_geometry and Alignment.apply against stub enqueues."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import align_f64 as A
from mvdfusion_amd import fusion, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_BOUND = 2.0 ** -32          # tests/test_gpu_align.py has the derivation
ORTHO_BOUND = 32 * 2.0 ** -53


# ------------------------------------------------------------------------------------------------ the oracle and the cases
@pytest.mark.parametrize("name", list(A.FIT_CASES))
def test_the_oracle_on_the_fit_cases_and_the_cases_reach_what_they_are_for(name):
    ref = A.fit_refs(name)
    case = ref.case
    gap = 0.0
    for k, (s, R, t) in enumerate(ref.steps):
        assert abs(np.linalg.det(R) - 1.0) < 1e-14 and s > 0
        if ref.pairs[k] >= 3:
            qs, qR, qt = A.quaternion_solve(ref.sums[k], case.scale)
            gap = max(gap, float(np.abs(qR - R).max()), abs(qs - s) / s, float(np.abs(qt - t).max()) / (1 + float(np.abs(t).max())))
        if case.truth[k] is not None:
            err = float(np.abs(A.step_matrix(s, R, t) - case.truth[k]).max())
            print(f"{name} scene {k}: pairs {ref.pairs[k]}, |M - truth| {err:.2e}")
            assert err <= 2.0 ** -20 * (A.spread_factor(case.source) if name == "offset" else 1.0)
    print(f"{name}: n {case.n} scenes {case.nscene} pairs {ref.pairs.tolist()} rms {ref.rms.tolist()}, SVD-quaternion gap {gap:.2e}")
    assert gap <= 1e-12 * (A.spread_factor(case.source) if name == "offset" else 1.0)
    if name == "pairs_4099":
        assert case.n % 64 and case.n % 256 and case.n % A.CHUNK
    if name == "chunk_edges":
        assert np.diff(case.start).tolist() == [A.CHUNK - 1, A.CHUNK, A.CHUNK + 1, 2 * A.CHUNK + 1] and case.start[1] % 64
    if name == "small_scenes":
        assert ref.pairs.tolist() == [0, 1, 2, 3, 500] and np.isnan(ref.rms[0]) and not np.isnan(ref.rms[1:]).any()
        for s, R, t in ref.steps[:3]:
            assert s == 1.0 and np.array_equal(R, np.eye(3)) and not t.any()
    if name == "planar":
        assert not bool(case.source[:, 2].any())
    if name == "mirrored":
        assert ref.rms[0] > 0.1          # no proper rotation fits a reflection
    if name == "offset":
        assert 500 < A.spread_factor(case.source) < 2000
    if name == "gate":
        rejected = 1.0 - ref.pairs[0] / case.n
        at = int((case.dist2 == case.max_d2).sum())
        print(f"  rejected {rejected:.3f}, exactly at the threshold {at}")
        assert 0.25 <= rejected <= 0.75 and at > 50 and case.max_d2 == 9 / 256 and bool(ref.accepted[case.dist2 == case.max_d2].all())
    if name == "nonfinite":
        assert int((~torch.isfinite(case.source).all(1)).sum()) == 30 and int((~torch.isfinite(case.target).all(1)).sum()) == 30
        assert ref.pairs[0] == int((torch.isfinite(case.source).all(1) & torch.isfinite(case.target).all(1)).sum())


@pytest.mark.parametrize("name,by", [("icp_sim5", 6), ("icp_rigid10", 13)])
def test_the_oracle_converges_on_the_icp_cases(name, by):
    ref = A.icp_refs(name)
    case = ref.case
    first = int(np.argmax(ref.right == case.n))
    err = float(np.abs(ref.matrix - case.truth[0]).max())
    print(f"{name}: n {case.n}, every correspondence right from iteration {first}, |M - truth| {err:.2e}, rms {ref.rms[0]:.4f} -> {ref.rms[-1]:.2e}")
    assert ref.right[-1] == case.n and first <= by and 2 * first <= case.iters and err <= 4e-11
    assert torch.equal(ref.index, case.perm) and (ref.pairs == case.n).all()
    assert ref.rms[-1] <= 2.0 ** -22
    if name == "icp_rigid10":
        assert abs(ref.rms[0] - 0.044) < 1e-3


# ------------------------------------------------------------------------------------------------ the library's solve, on the host
@pytest.fixture(scope="module", autouse=True)
def built_library():
    if not os.path.exists(hip.LIB_PATH):          # (tests/test_cpu_oracle_and_host.py does the same)
        import __graft_entry__ as ge
        ge.build()


def lib_solve(sums, scale):
    arr = (ctypes.c_double * 19)(*[float(v) for v in sums])
    step, s = (ctypes.c_double * 12)(), ctypes.c_double(-1.0)
    assert hip.lib().mvd_align_solve(arr, hip.ALIGN_SCALE if scale else 0, step, ctypes.byref(s)) == 0
    m = np.array(list(step)).reshape(3, 4)
    return s.value, m[:, :3] / s.value, m[:, 3]


def step_errors(got, want):
    (s, R, t), (s0, R0, t0) = got, want
    return float(np.abs(R - R0).max()), abs(s - s0) / s0, float(np.abs(t - t0).max()) / (1 + float(np.abs(t0).max()))


@pytest.mark.parametrize("name", list(A.CASES))
def test_the_library_solve_meets_the_svd_oracle(name):
    case = A.make_case(name)
    if name in A.ICP_CASES:          # the sums of the first iteration: wrong correspondences, a small step
        first = A.icp(case, iters=0)
        sums = A.moment_sums(first.moved, case.target, first.index, None, A.INF, case.start)
    else:
        sums = A.fit_refs(name).sums
    bound = STEP_BOUND * (A.spread_factor(case.source) if name == "offset" else 1.0)
    for k, row in enumerate(sums):
        got, want = lib_solve(row, case.scale), A.solve_svd(row, case.scale)
        eR, es, et = step_errors(got, want)
        ortho = float(np.abs(got[1].T @ got[1] - np.eye(3)).max())
        print(f"{name} scene {k}: pairs {int(row[0])}, R {eR:.2e} s {es:.2e} t {et:.2e} (bound {bound:.2e}), |R^T R - I| {ortho:.2e}")
        assert max(eR, es, et) <= bound and ortho <= ORTHO_BOUND and np.linalg.det(got[1]) > 0
        if row[0] < 3:
            assert got[0] == 1.0 and np.array_equal(got[1], np.eye(3)) and not got[2].any()
        if not case.scale:
            assert got[0] == 1.0


def test_the_library_solve_gives_the_identity_where_the_rule_says_so():
    good = A.fit_refs("pairs_4099").sums[0]
    assert lib_solve(good, True)[0] > 1.2
    cases = {"no pair": np.zeros(19), "two pairs": np.where(np.arange(19) == 0, 2.0, good / good[0] * 2)}
    flat = np.zeros(19)
    flat[[0, 1, 16]] = 10.0                                        # ten times p = (1, 0, 0): no spread
    cases["zero spread"] = flat
    for k, v in ((9, np.nan), (3, np.inf), (18, -np.inf), (0, np.nan)):
        bad = good.copy()
        bad[k] = v
        cases[f"sums[{k}] = {v}"] = bad
    for label, sums in cases.items():
        s, R, t = lib_solve(sums, True)
        assert s == 1.0 and np.array_equal(R, np.eye(3)) and not t.any(), label
    L = hip.lib()
    step, s = (ctypes.c_double * 12)(*([-7.0] * 12)), ctypes.c_double(-7.0)
    arr = (ctypes.c_double * 19)(*good)
    for args in ((None, 0, step, ctypes.byref(s)), (arr, 0, None, ctypes.byref(s)), (arr, 0, step, None), (arr, 2, step, ctypes.byref(s)),
                 (arr, -1, step, ctypes.byref(s))):
        assert L.mvd_align_solve(*args) != 0 and b"mvd_align_solve" in L.mvd_last_error()
    assert list(step) == [-7.0] * 12 and s.value == -7.0


@pytest.mark.parametrize("tiny", [1e-201, -1e-201, 1e-300, 5e-324])
def test_a_jacobi_theta_beyond_1e200_does_not_overflow(tiny):
    """Moments diag(1, 0.5, 0.25) with one off-diagonal entry of `tiny`: Horn's matrix gets an off-diagonal of that size against
    diagonal differences of order 1, so theta = difference / (2 off-diagonal) passes 1e200 and theta^2 overflows."""
    sums = np.zeros(19)
    sums[[0, 7, 11, 15, 12, 16, 17]] = [4, 4 * 1.0, 4 * 0.5, 4 * 0.25, 4 * tiny, 4 * 1.75, 4 * 1.3125]
    s, R, t = lib_solve(sums, True)
    want = A.solve_svd(sums, True)
    assert np.isfinite(R).all() and np.isfinite(t).all() and max(step_errors((s, R, t), want)) <= STEP_BOUND
    assert abs(s - 1.0) <= 1e-15 and float(np.abs(R - np.eye(3)).max()) <= 1e-15 and float(np.abs(R.T @ R - np.eye(3)).max()) <= ORTHO_BOUND


# ------------------------------------------------------------------------------------------------ header, binding, constants
def test_the_header_and_the_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define\s+MVD_ALIGN_(\w+)\s+(\d+)", hdr)}
    assert consts == dict(SCALE=hip.ALIGN_SCALE, NO_STEP=hip.ALIGN_NO_STEP, CHUNK=hip.ALIGN_CHUNK, SUMS=hip.ALIGN_SUMS, HISTORY=hip.ALIGN_HISTORY,
                          MAX_ITERS=hip.ALIGN_MAX_ITERS)
    assert hip.ALIGN_CHUNK == A.CHUNK and hip.ALIGN_SUMS == 19 and hip.ALIGN_MAX_ITERS == 1024 and hip.ALIGN_CHUNK % 256 == 0
    assert not re.search(r"#define\s+MVD_NN_ALIGN", hdr)
    for name, count in (("mvd_align_scratch", 5), ("mvd_align_solve", 4), ("mvd_align_apply", 7), ("mvd_align_fit", 15), ("mvd_align_icp", 20)):
        decl = re.search(r"^\w+ " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
        assert decl is not None and name in hip.SIGNATURES, name
        assert len(hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == count, name
    build = open(os.path.join(ROOT, "mvdfusion_amd", "csrc", "build.py")).read()
    assert '"align.hip"' in build and '"nearest.hip"' in build
    src = open(os.path.join(ROOT, "mvdfusion_amd", "csrc", "align.hip")).read()
    assert "atomicAdd" not in src and "mvd_nearest_points_stages(" in src          # no float atomics; the search is the exported one
    L = hip.lib()
    assert int(L.mvd_align_scratch(5000, 0, 3, hip.NN_BRUTE, 0)) >= (5 + 3) * 19 * 8 + 4 * 4
    assert int(L.mvd_align_scratch(5000, 5000, 1, hip.NN_GRID, 7)) >= int(L.mvd_align_scratch(5000, 0, 1, hip.NN_BRUTE, 0)) + \
        int(L.mvd_nearest_points_scratch(5000, 1, hip.NN_GRID, 7))
    for args in ((100, 100, 0, 0, 0), (100, 100, 65536, 0, 0), (100, 100, 1, 3, 0), (100, 100, 1, 0, 257), (1 << 31, 100, 1, 0, 0),
                 (100, 100, 65535, hip.NN_GRID, 256)):
        assert int(L.mvd_align_scratch(*args)) == 0, args


# ------------------------------------------------------------------------------------------------ the host side
def _cloud(scene, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = len(scene)
    z = torch.zeros(n, dtype=torch.int64)
    return fusion.PointCloud(xyz=torch.rand(n, 3, generator=g), rgb=torch.rand(n, 3, generator=g), support=z.to(torch.uint8),
                             scene=torch.tensor(scene, dtype=torch.int64), view=z, pixel=torch.zeros(n, 2, dtype=torch.int64), index=z.to(torch.int32))


@pytest.fixture
def stub(monkeypatch):
    calls = []

    def apply(xyz, start, N, transform):
        calls.append(dict(fn="apply", xyz=xyz, start=start, N=N, transform=transform.clone()))
        return xyz + 1.0

    def fit(moved, start, target, index, N, flags, max_d2, transform):
        calls.append(dict(fn="fit", moved=moved, start=start, target=target, index=index, N=N, flags=flags, max_d2=max_d2, transform=transform.clone()))
        if not flags & hip.ALIGN_NO_STEP:
            transform *= 2.0
        return torch.tensor([[0.5, 3.0, 2.0]], dtype=torch.float64).repeat(N, 1)

    def icp(source, source_start, target, target_start, N, method, grid, iters, flags, max_d2, transform):
        calls.append(dict(fn="icp", source=source, source_start=source_start, target=target, target_start=target_start, N=N, method=method,
                          grid=grid, iters=iters, flags=flags, max_d2=max_d2, transform=transform.clone()))
        n = source.shape[0]
        history = torch.tensor([0.25, float(n), 1.0], dtype=torch.float64).repeat(iters + 1, N, 1)
        if flags & hip.ALIGN_SCALE:          # every step doubles the scale; the rows carry the product
            history[:, :, 2] = 2.0 ** torch.arange(1, iters + 2, dtype=torch.float64).clamp(max=iters)[:, None]
        return history, source + 1.0, torch.arange(n, dtype=torch.int32), torch.full((n,), 0.0625)

    monkeypatch.setattr(fusion, "_align_apply", apply)
    monkeypatch.setattr(fusion, "_align_fit", fit)
    monkeypatch.setattr(fusion, "_align_icp", icp)
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("the library was touched"))
    return calls


@pytest.fixture
def no_host_reads(monkeypatch):
    for name in ("item", "cpu", "tolist", "numpy", "__bool__", "__float__", "__int__", "__index__"):
        monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _n=name, **k: pytest.fail(f"Tensor.{_n}() was called"), raising=True)


IDENTITY12 = torch.eye(3, 4, dtype=torch.float64).reshape(1, 12)


def test_fit_similarity_validates_and_enqueues(stub):
    a, b = _cloud([0, 0, 1, 1, 1, 2]), _cloud([0, 0, 1, 1, 1, 2], seed=1)
    mesh = fusion.TriangleMesh(vertices=torch.rand(3, 3), faces=torch.tensor([[0, 1, 2]], dtype=torch.int32), rgb=None,
                               vertex_start=torch.tensor([0, 3], dtype=torch.int32), face_start=torch.tensor([0, 1], dtype=torch.int32))
    bad = [dict(scenes=0), dict(scenes=2), dict(scenes=2.5), dict(scale=1), dict(scale=None), dict(target=_cloud([0, 0, 1])),
           dict(pairs=torch.zeros(6, dtype=torch.int64)), dict(pairs=torch.zeros(5, dtype=torch.int32)), dict(pairs=[0] * 6),
           dict(source=mesh), dict(target=mesh), dict(source=torch.rand(6, 2)), dict(source="cloud")]
    for kw in bad:
        args = dict(source=a, target=b, scenes=3)
        args.update(kw)
        with pytest.raises(ValueError):
            fusion.fit_similarity(**args)
    with pytest.raises(ValueError, match="sample_mesh"):
        fusion.fit_similarity(mesh, b, scenes=3)
    assert not stub
    al = fusion.fit_similarity(a, b, scenes=3)
    assert [c["fn"] for c in stub] == ["fit", "apply", "fit"]
    first, moved, last = stub
    assert first["flags"] == hip.ALIGN_SCALE and last["flags"] == hip.ALIGN_SCALE | hip.ALIGN_NO_STEP and first["max_d2"] == float("inf")
    assert first["start"].tolist() == [0, 2, 5, 6] and first["start"].dtype == torch.int32 and first["index"] is None and first["N"] == 3
    assert torch.equal(first["moved"], a.xyz) and torch.equal(first["target"], b.xyz) and torch.equal(first["transform"], IDENTITY12.repeat(3, 1))
    assert torch.equal(moved["transform"], 2 * IDENTITY12.repeat(3, 1)) and torch.equal(last["moved"], a.xyz + 1.0)
    assert [f.name for f in dataclasses.fields(al)] == ["matrix", "rotation", "translation", "scale", "rms", "pairs", "xyz", "nearest"]
    assert al.matrix.shape == (3, 4, 4) and al.matrix.dtype == torch.float64 and torch.equal(al.matrix[:, 3], torch.tensor([[0.0, 0, 0, 1]] * 3).double())
    assert torch.equal(al.scale, torch.full((3,), 2.0, dtype=torch.float64)) and torch.equal(al.rotation, torch.eye(3, dtype=torch.float64).expand(3, 3, 3))
    assert al.translation.shape == (3, 3) and al.rms.shape == al.pairs.shape == (1, 3) and al.pairs.dtype == torch.int64 and al.pairs.tolist() == [[3] * 3]
    assert torch.equal(al.xyz, a.xyz + 1.0) and al.nearest.index.tolist() == list(range(6)) and al.nearest.index.dtype == torch.int32
    d = a.xyz + 1.0 - b.xyz
    assert torch.equal(al.nearest.dist2, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    pairs = torch.tensor([3, -1, 0, 7, 2, 1], dtype=torch.int32)
    al = fusion.fit_similarity(a.xyz.double(), b.xyz[:4], scale=False, pairs=pairs)          # bare tensors: one scene; lengths may differ
    assert stub[-3]["flags"] == 0 and torch.equal(stub[-3]["index"], pairs) and stub[-3]["start"].tolist() == [0, 6] and stub[-3]["moved"].dtype == torch.float32
    assert al.nearest.index.tolist() == [3, -1, 0, -1, 2, 1] and bool(torch.isinf(al.nearest.dist2[[1, 3]]).all()) and bool(torch.isfinite(al.nearest.dist2[[0, 2, 4, 5]]).all())


def test_align_geometry_validates_and_enqueues(stub):
    a, b = _cloud([0, 0, 1, 1, 1, 2]), _cloud([0, 2, 2, 2], seed=1)
    mesh = fusion.TriangleMesh(vertices=torch.rand(3, 3), faces=torch.tensor([[0, 1, 2]], dtype=torch.int32), rgb=None,
                               vertex_start=torch.tensor([0, 3], dtype=torch.int32), face_start=torch.tensor([0, 1], dtype=torch.int32))
    flip = torch.diag(torch.tensor([-1.0, 1, 1, 1]))
    bad = [dict(scenes=0), dict(scenes=2), dict(iters=-1), dict(iters=1025), dict(iters=2.5), dict(iters=True), dict(iters=None), dict(iters="3"), dict(scale=1), dict(max_distance=-0.1),
           dict(max_distance=float("nan")), dict(init="pca"), dict(init=torch.eye(3)), dict(init=torch.eye(4).expand(2, 4, 4)), dict(init=flip),
           dict(init=torch.full((4, 4), float("nan"))), dict(init=torch.ones(4, 4)), dict(method="kdtree"), dict(grid=0), dict(grid=257),
           dict(source=mesh), dict(target=mesh), dict(source=torch.rand(5, 2))]
    for kw in bad:
        args = dict(source=a, target=b, scenes=3)
        args.update(kw)
        with pytest.raises(ValueError):
            fusion.align_geometry(**args)
    with pytest.raises(ValueError, match="sample_mesh"):
        fusion.align_geometry(a, mesh, scenes=3)
    assert not stub
    al = fusion.align_geometry(a, b, scenes=3)
    c = stub[-1]
    assert len(stub) == 1 and (c["N"], c["method"], c["grid"], c["iters"], c["flags"], c["max_d2"]) == (3, hip.NN_AUTO, 0, 30, 0, float("inf"))
    assert fusion.ALIGN_ITERS == 30 and c["source_start"].tolist() == [0, 2, 5, 6] and c["target_start"].tolist() == [0, 1, 1, 4]
    assert torch.equal(c["transform"], IDENTITY12.repeat(3, 1)) and torch.equal(c["source"], a.xyz) and torch.equal(c["target"], b.xyz)
    assert al.rms.shape == al.pairs.shape == (31, 3) and torch.equal(al.scale, torch.ones(3, dtype=torch.float64)) and al.xyz.shape == (6, 3)
    assert al.nearest.index.shape == (6,) and float(al.nearest.dist[0]) == 0.25
    al = fusion.align_geometry(a.xyz, b.xyz, iters=3, scale=True, max_distance=0.1, method="grid", grid=9)
    c = stub[-1]
    f32 = np.float32(0.1)
    assert (c["N"], c["method"], c["grid"], c["iters"], c["flags"]) == (1, hip.NN_GRID, 9, 3, hip.ALIGN_SCALE) and c["max_d2"] == float(np.float32(f32 * f32))
    assert al.scale.tolist() == [8.0] and al.rms.shape == (4, 1)          # three steps of scale 2 each
    assert fusion.align_geometry(a.xyz, b.xyz, iters=0).rms.shape == (1, 1) and stub[-1]["iters"] == 0
    assert fusion.align_geometry(a.xyz, b.xyz, max_distance=1e30).nearest is not None and stub[-1]["max_d2"] == float("inf")          # fl32 overflow
    # init: a matrix, a batch of matrices, an Alignment
    T = torch.from_numpy(A.similarity(2.0, 30.0, (1, 2, 3), (0.1, 0.2, 0.3)))
    al = fusion.align_geometry(a, b, scenes=3, init=T, iters=2)
    assert torch.equal(stub[-1]["transform"], T[:3].reshape(1, 12).repeat(3, 1)) and float((al.scale - 2.0).abs().max()) < 1e-15
    both = torch.stack([torch.eye(4, dtype=torch.float64), T, T])
    again = fusion.align_geometry(a, b, scenes=3, init=both.float(), iters=2)
    assert torch.equal(stub[-1]["transform"][0], IDENTITY12[0]) and float((again.scale - torch.tensor([1.0, 2.0, 2.0])).abs().max()) < 1e-6
    chained = fusion.align_geometry(a, b, scenes=3, init=al, scale=True, iters=1)
    assert torch.equal(stub[-1]["transform"], al.matrix[:, :3].reshape(3, 12)) and torch.equal(chained.scale, al.scale * 2.0)
    with pytest.raises(ValueError):
        fusion.align_geometry(a.xyz, b.xyz, init=al)          # three scenes into one


def test_the_start_transform_shares_no_storage_with_init():
    """The loop writes its result into the start transform.  With one scene the first three rows of a float64 (4, 4) matrix are
    contiguous as they lie, so a reshape of them is a view of the caller's tensor: the start must be a copy, for every form of init."""
    T = torch.from_numpy(A.similarity(1.25, 30.0, (1, 2, 3), (0.1, 0.2, 0.3)))
    assert T[None][:, :3, :].reshape(1, 12).contiguous().data_ptr() == T.data_ptr()          # (the view this guards against)
    m34 = T[:3].reshape(1, 3, 4)
    by_hand = fusion.Alignment(matrix=T[None].clone(), rotation=m34[:, :, :3] / 1.25, translation=m34[:, :, 3].clone(), scale=torch.tensor([1.25]).double(),
                               rms=torch.zeros(1, 1).double(), pairs=torch.zeros(1, 1, dtype=torch.int64), xyz=torch.zeros(0, 3), nearest=None)
    never = lambda: pytest.fail("the centroid start was asked for")
    for init in (T.clone(), T[None].clone(), by_hand):
        held = init.matrix if isinstance(init, fusion.Alignment) else init
        before = held.clone()
        transform, scale0 = fusion._start_transform(init, 1, "cpu", never)
        assert transform.shape == (1, 12) and transform.dtype == torch.float64 and torch.equal(transform, T[:3].reshape(1, 12))
        assert abs(float(scale0[0]) - 1.25) <= 1e-14
        assert transform.untyped_storage().data_ptr() != held.untyped_storage().data_ptr()
        transform.fill_(-7.25)
        scale0.fill_(-7.25)
        assert torch.equal(held, before) and (not isinstance(init, fusion.Alignment) or float(init.scale[0]) == 1.25)
    transform, scale0 = fusion._start_transform(None, 3, "cpu", never)
    assert torch.equal(transform, IDENTITY12.repeat(3, 1)) and torch.equal(scale0, torch.ones(3, dtype=torch.float64))
    assert transform.untyped_storage().data_ptr() != fusion._start_transform(None, 3, "cpu", never)[0].untyped_storage().data_ptr()
    given = (torch.full((2, 12), 0.5, dtype=torch.float64), torch.full((2,), 2.0, dtype=torch.float64))
    got = fusion._start_transform("centroid", 2, "cpu", lambda: given)
    assert got[0] is given[0] and got[1] is given[1]
    for init, text in (("pca", r"init = 'pca': None, 'centroid', an Alignment, or a \(4, 4\) or \(1, 4, 4\) matrix"),
                       (torch.eye(3), r"init: None, 'centroid', an Alignment, or a \(4, 4\) or \(1, 4, 4\) matrix"),
                       (torch.eye(4).expand(2, 4, 4), r"init: None, 'centroid', an Alignment, or a \(4, 4\) or \(1, 4, 4\) matrix"),
                       (torch.diag(torch.tensor([-1.0, 1, 1, 1])), r"init: the 3 x 3 block must have a positive determinant \(a similarity, not a reflection\)"),
                       (torch.zeros(4, 4), r"init: a finite matrix whose last row is \(0, 0, 0, 1\)")):
        with pytest.raises(ValueError, match=text):
            fusion._start_transform(init, 1, "cpu", never)


def test_the_shared_icp_checks():
    for iters in (-1, 1025, 1.5, True):
        with pytest.raises(ValueError, match=r"iters = .*: an integer in \[0, 1024\]"):
            fusion._check_icp(iters, None)
    for max_distance in (-1, float("nan")):
        with pytest.raises(ValueError, match="max_distance = .*: None or a distance >= 0"):
            fusion._check_icp(3, max_distance)
    with pytest.raises(ValueError, match="scale = 1: True or False"):
        fusion._check_icp(3, None, 1)
    assert fusion._check_icp(0, None) == (0, float("inf")) and fusion._check_icp(1024.0, None, True) == (1024, float("inf"))
    iters, max_d2 = fusion._check_icp(7, 0.1875)
    assert type(iters) is int and iters == 7 and max_d2 == 0.1875 ** 2 == float(np.float32(0.1875) * np.float32(0.1875))
    f32 = np.float32(0.1)
    assert fusion._check_icp(7, 0.1)[1] == float(np.float32(f32 * f32)) and fusion._check_icp(7, 1e30)[1] == float("inf")


def test_the_centroid_start_is_the_float64_map(stub):
    case = A.make_case("pairs_4099")
    for scale in (False, True):
        fusion.align_geometry(case.source, case.target, init="centroid", scale=scale, iters=1)
        m = stub[-1]["transform"].reshape(3, 4).numpy()
        p, q = case.source.double().numpy(), case.target.double().numpy()
        k = np.sqrt(((q - q.mean(0)) ** 2).sum(1).mean() / ((p - p.mean(0)) ** 2).sum(1).mean()) if scale else 1.0
        assert np.abs(m[:, :3] - k * np.eye(3)).max() <= 1e-12 and np.abs(m[:, 3] - (q.mean(0) - k * p.mean(0))).max() <= 1e-12
        assert not scale or abs(k - 1.3) < 1e-3
    # scene by scene; a scene with an empty side keeps the identity; non-finite rows do not count
    a, b = _cloud([0, 0, 1, 1, 1, 2]), _cloud([0, 2, 2, 2], seed=1)
    a.xyz[3, 1] = float("nan")
    fusion.align_geometry(a, b, scenes=3, init="centroid")
    m = stub[-1]["transform"].reshape(3, 3, 4)
    assert torch.equal(m[1], IDENTITY12.reshape(3, 4)) and bool(torch.isfinite(m).all())
    assert torch.allclose(m[0, :, 3], b.xyz[:1].double().mean(0) - a.xyz[:2].double().mean(0), atol=1e-15)
    assert torch.allclose(m[2, :, 3], b.xyz[1:].double().mean(0) - a.xyz[5:].double().mean(0), atol=1e-15)


def test_nothing_is_read_back_outside_the_centroid_start(stub, no_host_reads):
    src, tgt = torch.rand(50, 3), torch.rand(60, 3)
    al = fusion.align_geometry(src, tgt, iters=2, scale=True, max_distance=0.5)
    fusion.align_geometry(src, tgt, init=al, iters=1)          # (a matrix in host memory is checked with host reads: not the path meant here)
    fusion.fit_similarity(src, tgt[:50])
    fusion.fit_similarity(src, tgt, pairs=torch.arange(50, dtype=torch.int32))
    al.apply(src)
    assert len(stub) == 2 + 3 + 3 + 1
    with pytest.raises(pytest.fail.Exception, match="tolist"):
        fusion.align_geometry(src, tgt, init="centroid")


def test_alignment_apply_moves_coordinates_and_nothing_else(stub):
    a = _cloud([0, 0, 1, 1, 1, 2])
    al = fusion.align_geometry(a, a, scenes=3, iters=1)
    T = torch.from_numpy(A.similarity(2.0, 30.0, (1, 2, 3), (0.1, 0.2, 0.3)))
    al = dataclasses.replace(al, matrix=torch.stack([torch.eye(4, dtype=torch.float64), T, T]))
    out = al.apply(a)
    c = stub[-1]
    assert c["fn"] == "apply" and c["start"].tolist() == [0, 2, 5, 6] and c["N"] == 3 and torch.equal(c["transform"][1], T[:3].reshape(12))
    assert isinstance(out, fusion.PointCloud) and torch.equal(out.xyz, a.xyz + 1.0)
    for f in dataclasses.fields(a):
        assert f.name == "xyz" or getattr(out, f.name) is getattr(a, f.name), f.name
    samples = fusion.SurfaceSamples(xyz=torch.rand(4, 3), rgb=None, scene=torch.tensor([0, 0, 2, 2]), face=torch.zeros(4, dtype=torch.int32),
                                    bary=torch.zeros(4, 3))
    out = al.apply(samples)
    assert isinstance(out, fusion.SurfaceSamples) and stub[-1]["start"].tolist() == [0, 2, 2, 4] and out.face is samples.face and out.bary is samples.bary
    mesh = fusion.TriangleMesh(vertices=torch.rand(7, 3), faces=torch.tensor([[0, 1, 2], [4, 5, 6]], dtype=torch.int32), rgb=torch.rand(7, 3),
                               vertex_start=torch.tensor([0, 3, 3, 7], dtype=torch.int32), face_start=torch.tensor([0, 1, 1, 2], dtype=torch.int32))
    out = al.apply(mesh)
    assert isinstance(out, fusion.TriangleMesh) and stub[-1]["start"].tolist() == [0, 3, 3, 7] and torch.equal(out.vertices, mesh.vertices + 1.0)
    assert out.faces is mesh.faces and out.rgb is mesh.rgb and out.vertex_start is mesh.vertex_start and out.face_start is mesh.face_start
    one = dataclasses.replace(al, matrix=T[None])
    moved = one.apply(torch.rand(5, 3).double())
    assert torch.is_tensor(moved) and moved.dtype == torch.float32 and stub[-1]["start"].tolist() == [0, 5] and stub[-1]["xyz"].dtype == torch.float32
    for bad in (torch.rand(5, 3), mesh.scene(0), "cloud", torch.rand(5, 2)):
        with pytest.raises(ValueError):
            (al if not (torch.is_tensor(bad) and bad.shape[1] == 2) else one).apply(bad)
