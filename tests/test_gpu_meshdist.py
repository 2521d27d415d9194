"""The point-to-mesh entries on the GPU: mvd_nearest_on_mesh and mvd_mesh_icp (csrc/meshdist.hip, csrc/align.hip) through the C ABI
against the two oracles of tests/meshdist_f64.py, and the host path (fusion.nearest_on_mesh, fusion.compare_geometry(exact=True),
fusion.align_to_mesh).

Bounds -- none taken from what the kernels give (tests/meshdist_f64.py derives them):
  against (a)     face, region and the bits of dist2 EQUAL on every query of every case, MVD_NN_BRUTE and MVD_NN_GRID at grid = 1, 7 and
                  the library's choice.  No query is left out.  point, bary, normal: one fp32 rounding of the float64 value, 2^-24
                  relative per component (NaN where (a) has NaN); the count of components whose bits differ is printed.
  bit equalities  two runs; BUILD + QUERY against ALL; a scene alone against the scene inside the batch; every one of the 64 subsets
                  of NULL outputs against the full call.
  refusals        non-zero, the entry's name in mvd_last_error(), every pre-filled buffer untouched.
  against (b)     on the subset of meshdist_f64.exact_pairs: dist2 within one fp32 ulp of the exact minimum rounded to fp32, and the
                  chosen face one whose exact d2 (rounded to fp32) is within one ulp of that minimum.  All ten cases (case 5 too: its
                  faces are well shaped or exactly degenerate, see the oracle's docstring).
  compare_geometry(exact=True)   a sample of sample_mesh is the fp32 rounding of a float64 mix b0 A + b1 B + b2 C of a face's vertices:
                  it lies within 2^-24 * max|coordinate| per axis of a point of the face (half an ulp of a value below 1 is at most
                  2^-25; the mix itself adds three roundings of 2^-53), so its exact distance to the mesh is at most sqrt(3) * 2^-24 *
                  max|coordinate| <= 1.1e-7 * 0.75, and the kernel's fp64 evaluation adds ~2^-50.  accuracy <= 2^-23 * max|coordinate|
                  (twice that, for the rounding of sqrt and the mean) and precision == 1 at threshold 1e-5.
  mesh ICP        pairs and rank EQUAL to the oracle's on every history row; |M_gpu - M_oracle| <= 1 / 16 of the oracle's own
                  |M - truth| (the faceting of the 1 984-face target; test_gpu_plane.py derives its sliding bound the same way); moved,
                  face, dist2 EQUAL to mvd_align_apply + mvd_nearest_on_mesh of the returned transform; the whole call EQUAL, bit for
                  bit, to the caller-issued sequence of mvd_align_apply, mvd_nearest_on_mesh_stages and mvd_plane_fit; a scene alone
                  EQUAL to the scene in a batch of two; a cube with a source on one face keeps rank 3 and one step leaves x, y and the
                  turn about z at 0 (<= 1e-12: the rows of H for them are exactly zero).

Measured on an MI355X: no mismatch of face, region or dist2 on any query of the ten cases under any of the four method / grid settings,
and point, bary and normal bit-equal to (a) on every component (the asserted bar is 2^-24 relative; equal bits is what was seen).
Against (b), 357 queries / 2 461 pairs: dist2 off by one ulp on none, the chosen face an exact minimiser on all.  compare_geometry
exact: accuracy 7.5e-9 against the bound 5.9e-8 (largest distance 2.8e-8; exactly 0 on 1.6 % of the samples), precision 1.  Mesh ICP:
|M_gpu - M_oracle| 6.3e-16 against the bound 4.75e-5 (the oracle's own |M - truth| 7.6e-4, plane rms 0.0252 -> 0.00166), pairs 1 024 and
rank 6 on all 13 rows, bit-equal to the caller-issued sequence under AUTO, BRUTE and GRID 9; cube: rank 3 on every row, one step t =
(0, 0, -0.01008) and no turn about z, exactly.  Recorded, not asserted: |M - truth| of align_to_mesh 7.60e-4, of align_to_surface on
4 096 / 65 536 samples of the same mesh 6.43e-4 / 5.37e-4 -- all three the faceting of the 1 984-face target; the mesh route has no
sampling parameter, the sampled route's figure moves with it.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import meshdist_f64 as M
import plane_f64 as P

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
OUTPUTS = ("face", "dist2", "point", "bary", "region", "normal")


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


def _runs(hip):
    return [("brute", hip.NN_BRUTE, 0)] + [(f"grid{g}", hip.NN_GRID, g) for g in M.GRIDS]


def _device(case):
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).contiguous().cuda()
    return dict(query=dev(case.query, torch.float32), qstart=dev(case.query_start, torch.int32), vertices=dev(case.vertices, torch.float32),
                faces=dev(case.faces, torch.int32), fstart=dev(case.face_start, torch.int32), nq=case.nq, nv=case.nv, nf=case.nf, nscene=case.nscene)


def _buffers(nq, nbytes):
    n = max(nq, 1)
    i32 = lambda *s: torch.full(s, -5, dtype=torch.int32, device="cuda")
    f32 = lambda *s: torch.full(s, SENTINEL, device="cuda")
    return dict(face=i32(n), dist2=f32(n), point=f32(n, 3), bary=f32(n, 3), region=i32(n), normal=f32(n, 3),
                scratch=torch.full((max((nbytes + 7) // 8, 2),), 0x1234, dtype=torch.int64, device="cuda"))


def _untouched(out):
    return all(bool((out[k] == (-5 if out[k].dtype == torch.int32 else SENTINEL)).all()) for k in OUTPUTS) and bool((out["scratch"] == 0x1234).all())


def _call(hip, out, query, qstart, vertices, faces, fstart, nq, nv, nf, nscene, method, grid, nbytes=None, stages=None, scratch=True,
          scratch_offset=0, skip=(), face_offset=0):
    p = lambda t: None if t is None else hip.ptr(t)
    nbytes = out["scratch"].numel() * 8 if nbytes is None else nbytes
    sc = ctypes.c_void_p(out["scratch"].data_ptr() + scratch_offset) if scratch else None
    outs = [None if k in skip else p(out[k]) for k in OUTPUTS]
    if face_offset:
        outs[0] = ctypes.c_void_p(out["face"].data_ptr() + face_offset)
    args = [p(query), p(qstart), p(vertices), p(faces), p(fstart), nq, nv, nf, nscene, method, grid, *outs, sc, nbytes]
    L = hip.lib()
    if stages is None:
        return L.mvd_nearest_on_mesh(*args, hip.stream())
    return L.mvd_nearest_on_mesh_stages(*args, stages, hip.stream())


def _search(hip, case, method, grid=0, stages=(None,), out=None, skip=()):
    nbytes = int(hip.lib().mvd_nearest_on_mesh_scratch(case.nf, case.nscene, method, grid))
    out = _buffers(case.nq, nbytes) if out is None else out
    dev = _device(case)
    for st in stages:
        hip.check(_call(hip, out, method=method, grid=grid, nbytes=nbytes, stages=st, skip=skip, **dev))
    torch.cuda.synchronize()
    return out


def _bits(out, nq, keys=OUTPUTS):
    return [out[k][:nq].cpu().numpy().view(np.int32) for k in keys]


def _same(a, b, nq, keys=OUTPUTS):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a, nq, keys), _bits(b, nq, keys)))


# ------------------------------------------------------------------------------------------------ 1. against (a)
@pytest.mark.parametrize("name", M.CASES)
def test_every_method_gives_the_bits_of_the_rule(hip, name):
    case, ref = M.make_case(name), M.refs(name)
    wrong, loose = {}, 0
    for label, method, grid in _runs(hip):
        out = _search(hip, case, method, grid)
        got = {k: out[k][:case.nq].cpu().numpy() for k in OUTPUTS}
        bad = (got["face"] != ref.face) | (got["region"] != ref.region) | (got["dist2"].view(np.int32) != ref.dist2.view(np.int32))
        if bad.any():
            i = int(np.argmax(bad))
            wrong[label] = (int(bad.sum()), i, int(got["face"][i]), int(ref.face[i]), float(got["dist2"][i]), float(ref.dist2[i]))
        for k in ("point", "bary", "normal"):
            want = getattr(ref, k)
            assert np.array_equal(np.isnan(got[k]), np.isnan(want)), (label, k)
            with np.errstate(invalid="ignore"):
                err = np.abs(got[k].astype(np.float64) - want.astype(np.float64))
                over = np.nan_to_num(err) > 2.0 ** -24 * np.abs(np.nan_to_num(want.astype(np.float64)))
            assert not over.any(), (label, k, int(over.sum()))
            loose += int((got[k].view(np.int32) != want.view(np.int32)).sum())
        print(f"RATIO meshdist {name} {label} | nq {case.nq} nf {case.nf} scenes {case.nscene} found {int((ref.face >= 0).sum())} | face / region / "
              f"dist2 mismatches {int(bad.sum())} | point / bary / normal components with other bits so far {loose}")
    assert not wrong, wrong


# ------------------------------------------------------------------------------------------------ 2. against (b)
@pytest.mark.parametrize("name", M.CASES)
def test_the_kernels_meet_exact_rational_arithmetic(hip, name):
    case = M.make_case(name)
    exact = M.exact_minima(name)
    for label, method, grid in (("brute", hip.NN_BRUTE, 0), ("grid", hip.NN_GRID, 0)):
        out = _search(hip, case, method, grid)
        face, dist2 = out["face"][:case.nq].cpu().numpy(), out["dist2"][:case.nq].cpu().numpy()
        off = 0
        for i, (least, per_face) in exact.items():
            assert M.within_one_ulp(float(dist2[i]), least), (name, label, i, float(dist2[i]), least)
            assert int(face[i]) in per_face and M.within_one_ulp(per_face[int(face[i])], least), (name, label, i, int(face[i]))
            off += float(dist2[i]) != least
        print(f"RATIO meshdist exact {name} {label} | queries {len(exact)} pairs {sum(len(v[1]) for v in exact.values())} | dist2 off by one ulp on "
              f"{off} (bound: one ulp on any) | chosen face not an exact minimiser on 0")


# ------------------------------------------------------------------------------------------------ 3. determinism, stages, scenes, NULLs
@pytest.mark.parametrize("name", ["mixed", "odd", "scenes"])
def test_two_runs_and_the_stages_give_equal_bits(hip, name):
    case = M.make_case(name)
    for label, method, grid in _runs(hip):
        one, again = _search(hip, case, method, grid), _search(hip, case, method, grid)
        assert not any(bool((one[k][:case.nq] == (-5 if one[k].dtype == torch.int32 else SENTINEL)).any()) for k in ("face", "dist2", "region"))
        assert _same(one, again, case.nq), label
        built = _search(hip, case, method, grid, stages=(hip.NN_BUILD,))
        assert all(bool((built[k] == (-5 if built[k].dtype == torch.int32 else SENTINEL)).all()) for k in OUTPUTS)          # nothing queried yet
        assert _same(one, _search(hip, case, method, grid, stages=(hip.NN_QUERY,), out=built), case.nq), label
        assert _same(one, _search(hip, case, method, grid, stages=(hip.NN_BUILD, hip.NN_QUERY, hip.NN_QUERY)), case.nq), label


def test_a_scene_alone_gives_the_bits_it_gives_in_the_batch(hip):
    case = M.make_case("scenes")
    for label, method, grid in _runs(hip):
        batch = _search(hip, case, method, grid)
        for s in range(case.nscene):
            alone, f0, (q0, q1) = M.scene_case(case, s)
            if q1 == q0:
                continue
            one = _search(hip, alone, method, grid)
            face = one["face"][:alone.nq]
            assert torch.equal(torch.where(face >= 0, face + f0, face), batch["face"][q0:q1]), (label, s)
            for k in OUTPUTS[1:]:
                assert np.array_equal(one[k][:alone.nq].cpu().numpy().view(np.int32), batch[k][q0:q1].cpu().numpy().view(np.int32)), (label, s, k)


def test_every_subset_of_null_outputs_leaves_the_others_unchanged(hip):
    case = M.make_case("odd")
    for method, grid in ((hip.NN_BRUTE, 0), (hip.NN_GRID, 7)):
        full = _search(hip, case, method, grid)
        for r in range(1, len(OUTPUTS) + 1):
            for skip in itertools.combinations(OUTPUTS, r):
                out = _search(hip, case, method, grid, skip=skip)
                kept = tuple(k for k in OUTPUTS if k not in skip)
                assert _same(full, out, case.nq, kept), (method, skip)
                assert all(bool((out[k] == (-5 if out[k].dtype == torch.int32 else SENTINEL)).all()) for k in skip), (method, skip)


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_bad_arguments_return_an_error_and_write_nothing(hip):
    L = hip.lib()
    case = M.make_case("mixed")
    nbytes = int(L.mvd_nearest_on_mesh_scratch(case.nf, 1, hip.NN_GRID, 7))
    assert nbytes > 0 and int(L.mvd_nearest_on_mesh_scratch(case.nf, 1, hip.NN_BRUTE, 0)) == 0
    assert int(L.mvd_nearest_on_mesh_scratch(case.nf, 0, hip.NN_GRID, 7)) == 0 and int(L.mvd_nearest_on_mesh_scratch(case.nf, 1, hip.NN_GRID, 257)) == 0
    assert int(L.mvd_nearest_on_mesh_scratch((2 ** 31 - 1) // 27 + 1, 1, hip.NN_GRID, 7)) == 0
    good = dict(_device(case), method=hip.NN_GRID, grid=7, nbytes=nbytes)
    out = _buffers(case.nq, nbytes)
    bad = [dict(nbytes=nbytes - 16), dict(nbytes=0), dict(scratch=False), dict(scratch_offset=8), dict(face_offset=2), dict(nscene=0), dict(nscene=-1),
           dict(nscene=65536), dict(method=3), dict(method=-1), dict(grid=257), dict(grid=-1), dict(query=None), dict(qstart=None), dict(vertices=None),
           dict(faces=None), dict(fstart=None), dict(nq=1 << 31), dict(nv=1 << 31), dict(nf=1 << 31, nbytes=1 << 62),
           dict(nf=(2 ** 31 - 1) // 27 + 1, nbytes=1 << 62)]
    for stages in (None, hip.NN_QUERY, hip.NN_BUILD):
        for kw in bad:
            a = dict(good)
            a.update(kw)
            assert _call(hip, out, stages=stages, **a) != 0, kw
            assert (b"mvd_nearest_on_mesh_stages" if stages else b"mvd_nearest_on_mesh:") in L.mvd_last_error(), (kw, L.mvd_last_error())
    for stages in (0, 4, -1):
        assert _call(hip, out, stages=stages, **good) != 0 and b"mvd_nearest_on_mesh_stages" in L.mvd_last_error()
    torch.cuda.synchronize()
    assert _untouched(out)
    # an empty mesh is a valid call: nothing is found
    empty = dict(_device(case), vertices=None, faces=None, nv=0, nf=0, fstart=torch.zeros(2, dtype=torch.int32, device="cuda"))
    for method in (hip.NN_BRUTE, hip.NN_GRID, hip.NN_AUTO):
        out = _buffers(case.nq, 0)
        assert _call(hip, out, method=method, grid=0, scratch=False, nbytes=0, **empty) == 0
        torch.cuda.synchronize()
        assert bool((out["face"] == -1).all()) and bool(torch.isposinf(out["dist2"]).all()) and bool(torch.isnan(out["point"]).all())
        assert bool((out["region"] == -1).all()) and not bool(out["bary"].any()) and not bool(out["normal"].any())


# ------------------------------------------------------------------------------------------------ 5. host path
def _tri_mesh(case):
    from mvdfusion_amd import fusion
    t = lambda a: torch.from_numpy(a).cuda()
    return fusion.TriangleMesh(vertices=t(case.vertices), faces=t(case.faces), rgb=None, vertex_start=torch.tensor([0, case.nv], dtype=torch.int32),
                               face_start=torch.from_numpy(case.face_start.copy()))


def test_nearest_on_mesh_is_the_abi_call(hip):
    from mvdfusion_amd import fusion
    case = M.make_case("scenes")
    mesh = _tri_mesh(case)
    mesh.rgb = torch.rand(case.nv, 3, device="cuda")
    scene = torch.from_numpy(np.repeat(np.arange(5), np.diff(np.concatenate([case.query_start, [case.nq]])))).cuda()
    cloud = fusion.SurfaceSamples(xyz=torch.from_numpy(case.query).cuda(), rgb=None, scene=scene, face=None, bary=None)
    for method, m, grid in (("auto", hip.NN_AUTO, None), ("brute", hip.NN_BRUTE, None), ("grid", hip.NN_GRID, 7)):
        got = fusion.nearest_on_mesh(cloud, mesh, scenes=4, method=method, grid=grid)
        want = _search(hip, case, m, grid or 0)
        for k in OUTPUTS:
            assert np.array_equal(getattr(got, k).cpu().numpy().view(np.int32), want[k][:case.nq].cpu().numpy().view(np.int32)), (method, k)
        assert torch.equal(got.hit, got.face >= 0) and torch.equal(got.dist, got.dist2.sqrt())
    rgb = got.rgb(mesh)
    ids = mesh.faces.long()[got.face.long().clamp(min=0)]
    mix = (got.bary.double()[:, :, None] * mesh.rgb.double()[ids]).sum(1).float()
    assert torch.equal(rgb[got.hit], mix[got.hit]) and bool(torch.isnan(rgb[~got.hit]).all()) and int((~got.hit).sum()) == 77
    with pytest.raises(ValueError):
        fusion.nearest_on_mesh(cloud, mesh, scenes=3)


def test_compare_geometry_exact_measures_to_the_triangles(hip):
    from mvdfusion_amd import fusion
    G = 16
    ax = ((torch.arange(G, dtype=torch.float64) + 0.5) * (1.5 / G) - 0.75).cuda()
    zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
    mesh = fusion.extract_mesh(((xx ** 2 + yy ** 2 + zz ** 2).sqrt() - 0.5).float())
    samples = fusion.sample_mesh(mesh, 2048)
    big = float(mesh.vertices.abs().max())
    exact = fusion.compare_geometry(samples, mesh, threshold=1e-5, samples=2048, exact=True)
    plain = fusion.compare_geometry(samples, mesh, threshold=1e-5, samples=2048)
    direct = fusion.nearest_points(samples, fusion.sample_mesh(mesh, 2048))
    worst = float(exact.a_to_b.dist.max())
    print(f"RATIO compare exact | faces {len(mesh)} samples {len(samples)} max|coordinate| {big:.3f} | accuracy exact {float(exact.accuracy[0]):.3g} "
          f"(bound {2.0 ** -23 * big:.3g}), largest distance {worst:.3g}, exactly 0 on {float((exact.a_to_b.dist2 == 0).float().mean()):.3f} | sampled route "
          f"{float(plain.accuracy[0]):.3g}, completeness exact {float(exact.completeness[0]):.3g}")
    assert isinstance(exact.a_to_b, fusion.NearestOnMesh) and isinstance(exact.b_to_a, fusion.NearestPoints) and bool(exact.a_to_b.hit.all())
    assert float(exact.accuracy[0]) <= 2.0 ** -23 * big and float(exact.precision[0]) == 1.0
    # exact=False returns the bits it returns today: the search on the samples
    assert isinstance(plain.a_to_b, fusion.NearestPoints) and torch.equal(plain.a_to_b.index, direct.index)
    assert torch.equal(plain.a_to_b.dist2.view(torch.int32), direct.dist2.view(torch.int32)) and float(plain.accuracy[0]) == 0.0
    assert torch.equal(exact.b_to_a.dist2.view(torch.int32), plain.b_to_a.dist2.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 6. mesh ICP
def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def _identity(n):
    return torch.eye(3, 4, dtype=torch.float64).reshape(1, 12).repeat(n, 1).cuda()


def _icp(hip, source, sstart, vertices, faces, fstart, nscene, iters, method=None, grid=0, transform=None, override=None):
    """mvd_mesh_icp on pre-filled buffers sized by the arguments; `override` replaces arguments of the call itself (by name, below)."""
    L = hip.lib()
    method = hip.NN_AUTO if method is None else method
    nq, nv, nf = int(source.shape[0]), int(vertices.shape[0]), int(faces.shape[0])
    transform = _identity(nscene) if transform is None else transform
    out = dict(history=torch.full((iters + 1, nscene, 4), SENTINEL, dtype=torch.float64, device="cuda"), moved=torch.full((nq, 3), SENTINEL, device="cuda"),
               face=torch.full((nq,), -5, dtype=torch.int32, device="cuda"), dist2=torch.full((nq,), SENTINEL, device="cuda"),
               point=torch.full((nq, 3), SENTINEL, device="cuda"), normal=torch.full((nq, 3), SENTINEL, device="cuda"), transform=transform)
    need = int(L.mvd_mesh_icp_scratch(nq, nf, nscene, method, grid))
    out["scratch"] = torch.full(((need + 7) // 8 + 2,), 0x1234, dtype=torch.int64, device="cuda")
    p = hip.ptr
    a = dict(source=p(source), sstart=p(sstart), vertices=p(vertices), faces=p(faces), fstart=p(fstart), nq=nq, nv=nv, nf=nf, nscene=nscene, method=method,
             grid=grid, iters=iters, max_d2=float("inf"), transform=p(transform), history=p(out["history"]), moved=p(out["moved"]), face=p(out["face"]),
             dist2=p(out["dist2"]), point=p(out["point"]), normal=p(out["normal"]), scratch=p(out["scratch"]), nbytes=need)
    a.update(override or {})
    rc = L.mvd_mesh_icp(*a.values(), hip.stream())
    torch.cuda.synchronize()
    return rc, out


def _ellipsoid(case):
    return (case.source.cuda(), _i32([0, case.source.shape[0]]), torch.from_numpy(case.vertices).cuda(), torch.from_numpy(case.faces).cuda(),
            _i32([0, len(case.faces)]))


def _matrix(out, s=0):
    m = np.eye(4)
    m[:3] = out["transform"][s].cpu().numpy().reshape(3, 4)
    return m


def _by_hand(hip, source, sstart, vertices, faces, fstart, nscene, iters, method, grid):
    """The sequence mvd_mesh_icp stands for, issued by the caller: mvd_align_apply, mvd_nearest_on_mesh_stages, mvd_plane_fit."""
    L, p = hip.lib(), hip.ptr
    nq, nv, nf = int(source.shape[0]), int(vertices.shape[0]), int(faces.shape[0])
    transform = _identity(nscene)
    history = torch.empty(iters + 1, nscene, 4, dtype=torch.float64, device="cuda")
    moved, point, normal = torch.empty_like(source), torch.empty_like(source), torch.empty_like(source)
    face, dist2 = torch.empty(nq, dtype=torch.int32, device="cuda"), torch.empty(nq, device="cuda")
    nn_bytes = int(L.mvd_nearest_on_mesh_scratch(nf, nscene, method, grid))
    nn = torch.empty((nn_bytes + 7) // 8 + 2, dtype=torch.int64, device="cuda")
    fit_bytes = int(L.mvd_plane_scratch(nq, 0, nscene, hip.NN_BRUTE, 0))
    fit = torch.empty((fit_bytes + 7) // 8 + 2, dtype=torch.int64, device="cuda")
    search = lambda stages: hip.check(L.mvd_nearest_on_mesh_stages(p(moved), p(sstart), p(vertices), p(faces), p(fstart), nq, nv, nf, nscene, method, grid,
                                                                   p(face), p(dist2), p(point), None, None, p(normal), p(nn) if nn_bytes else None,
                                                                   nn_bytes, stages, hip.stream()))
    search(hip.NN_BUILD)
    for k in range(iters + 1):
        hip.check(L.mvd_align_apply(p(source), p(sstart), nq, nscene, p(transform), p(moved), hip.stream()))
        search(hip.NN_QUERY)
        hip.check(L.mvd_plane_fit(p(moved), p(sstart), p(point), p(normal), None, p(dist2), nq, nq, nscene, 0 if k < iters else hip.PLANE_NO_STEP,
                                  float("inf"), p(transform), p(history[k]), p(fit), fit_bytes, hip.stream()))
    torch.cuda.synchronize()
    return dict(transform=transform, history=history, moved=moved, face=face, dist2=dist2, point=point, normal=normal)


def test_mesh_icp_follows_the_oracle_and_is_the_sequence_it_stands_for(hip):
    case, ref = M.icp_case(), M.icp_ref()
    dev = _ellipsoid(case)
    rc, out = _icp(hip, *dev, 1, case.iters)
    assert rc == 0, hip.lib().mvd_last_error()
    Mg, history = _matrix(out), out["history"].cpu().numpy()[:, 0]
    own, gap = float(np.abs(ref.matrix - case.truth).max()), float(np.abs(Mg - ref.matrix).max())
    print(f"RATIO mesh icp | faces {len(case.faces)} n {case.source.shape[0]} iters {case.iters} | oracle |M - truth| {own:.4g}, |M_gpu - M_oracle| {gap:.3g} "
          f"(bound {own / 16:.3g}) | plane rms {history[0, 0]:.4g} -> {history[-1, 0]:.6g} (oracle {ref.history[-1, 0]:.6g}) rms {history[-1, 2]:.6g}")
    assert (history[:, 1] == ref.history[:, 1]).all() and (history[:, 3] == ref.history[:, 3]).all() and (history[:, 3] == 6).all()
    assert gap <= own / 16
    # moved, face, dist2 are the apply and the search of the returned transform
    L, p = hip.lib(), hip.ptr
    moved = torch.empty_like(dev[0])
    hip.check(L.mvd_align_apply(p(dev[0]), p(dev[1]), case.source.shape[0], 1, p(out["transform"]), p(moved), hip.stream()))
    again = _search(hip, M._case(moved.cpu().numpy(), case.vertices, case.faces), hip.NN_BRUTE)
    assert torch.equal(moved.view(torch.int32), out["moved"].view(torch.int32))
    assert all(torch.equal(again[k].view(torch.int32), out[k].view(torch.int32)) for k in ("face", "dist2", "point", "normal"))
    # the whole call against the caller-issued sequence, and the search's method changes no bit
    for method, grid in ((hip.NN_AUTO, 0), (hip.NN_BRUTE, 0), (hip.NN_GRID, 9)):
        hand = _by_hand(hip, *dev, 1, case.iters, method, grid)
        rc, other = _icp(hip, *dev, 1, case.iters, method=method, grid=grid)
        assert rc == 0
        bits = lambda t: t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)
        for k in ("transform", "history", "moved", "face", "dist2", "point", "normal"):
            assert torch.equal(bits(hand[k]), bits(other[k])), (method, k)
            assert torch.equal(bits(out[k]), bits(other[k])), (method, k)
    # iters = 0 returns the start with one history row
    start = torch.tensor(P.TRUTH_SLIDE[:3].reshape(1, 12), dtype=torch.float64).cuda()
    rc, zero = _icp(hip, *dev, 1, 0, transform=start)
    assert rc == 0 and np.array_equal(_matrix(zero), P.TRUTH_SLIDE) and not bool((zero["history"] == SENTINEL).any())
    assert float(zero["history"][0, 0, 0]) < 0.01 and int(zero["history"][0, 0, 1]) == case.source.shape[0]


def test_mesh_icp_of_a_scene_alone_is_the_scene_in_a_batch_of_two(hip):
    case, cube = M.icp_case(), M.cube_icp_case()
    n0, n1 = int(case.source.shape[0]), int(cube.source.shape[0])
    source = torch.cat([case.source, cube.source]).cuda()
    vertices = torch.from_numpy(np.concatenate([case.vertices, cube.vertices])).cuda()
    faces = torch.from_numpy(np.concatenate([case.faces, cube.faces + len(case.vertices)])).cuda()
    sstart, fstart = _i32([0, n0, n0 + n1]), _i32([0, len(case.faces), len(case.faces) + len(cube.faces)])
    for method, grid in ((hip.NN_BRUTE, 0), (hip.NN_GRID, 7)):
        rc, both = _icp(hip, source, sstart, vertices, faces, fstart, 2, 4, method=method, grid=grid)
        assert rc == 0, hip.lib().mvd_last_error()
        parts = [(case, 0, slice(0, n0), 0), (cube, 1, slice(n0, n0 + n1), len(case.faces))]
        for part, s, rows, f0 in parts:
            rc, one = _icp(hip, part.source.cuda(), _i32([0, part.source.shape[0]]), torch.from_numpy(part.vertices).cuda(),
                           torch.from_numpy(part.faces).cuda(), _i32([0, len(part.faces)]), 1, 4, method=method, grid=grid)
            assert rc == 0
            assert torch.equal(one["transform"][0], both["transform"][s]) and torch.equal(one["history"][:, 0], both["history"][:, s]), (method, s)
            assert torch.equal(one["face"] + f0, both["face"][rows]) and torch.equal(one["dist2"].view(torch.int32), both["dist2"][rows].view(torch.int32))
            assert torch.equal(one["moved"].view(torch.int32), both["moved"][rows].view(torch.int32))
        # the cube's scene: a source on one face only keeps rank 3
        assert (both["history"][:, 1, 3] == 3).all() and (both["history"][:, 0, 3] == 6).all()
    cube_dev = (cube.source.cuda(), _i32([0, n1]), torch.from_numpy(cube.vertices).cuda(), torch.from_numpy(cube.faces).cuda(), _i32([0, len(cube.faces)]))
    rc, one = _icp(hip, *cube_dev, 1, 1)
    m = _matrix(one)
    print(f"RATIO mesh icp cube | one step: t = ({m[0, 3]:.3g}, {m[1, 3]:.3g}, {m[2, 3]:.4g}), turn about z {m[1, 0] - m[0, 1]:.3g} (bound 1e-12) | rank "
          f"{one['history'][:, 0, 3].tolist()}")
    assert rc == 0 and abs(m[0, 3]) <= 1e-12 and abs(m[1, 3]) <= 1e-12 and abs(m[1, 0] - m[0, 1]) <= 1e-12 and abs(m[2, 3]) > 1e-3


def test_bad_icp_arguments_return_an_error_and_write_nothing(hip):
    L = hip.lib()
    case = M.icp_case()
    dev = _ellipsoid(case)
    for kw in (dict(iters=-1), dict(iters=1025), dict(method=3), dict(grid=257), dict(nscene=0), dict(max_d2=-1.0), dict(source=None), dict(sstart=None),
               dict(vertices=None), dict(faces=None), dict(fstart=None), dict(transform=None), dict(history=None), dict(moved=None), dict(face=None),
               dict(dist2=None), dict(point=None), dict(normal=None), dict(scratch=None), dict(nbytes=16), dict(nq=1 << 31), dict(nf=1 << 31)):
        rc, out = _icp(hip, *dev, 1, 3, method=hip.NN_GRID, grid=7, override=kw)
        assert rc != 0 and b"mvd_mesh_icp" in L.mvd_last_error(), kw
        assert all(bool((out[k] == (-5 if out[k].dtype == torch.int32 else SENTINEL)).all()) for k in ("history", "moved", "face", "dist2", "point", "normal"))
        assert bool((out["scratch"] == 0x1234).all()) and torch.equal(out["transform"], _identity(1)), kw


def test_align_to_mesh_does_not_depend_on_a_sampling_of_the_target(hip):
    from mvdfusion_amd import fusion
    case, ref = M.icp_case(), M.icp_ref()
    mesh = _tri_mesh(M._case(np.zeros((0, 3)), case.vertices, case.faces))
    source = case.source.cuda()
    init = torch.eye(4, dtype=torch.float64).cuda()
    al = fusion.align_to_mesh(source, mesh, iters=case.iters, init=init)
    assert torch.equal(init, torch.eye(4, dtype=torch.float64).cuda())          # the caller's init is never written into
    assert isinstance(al, fusion.PlaneAlignment) and isinstance(al.nearest, fusion.NearestOnMesh)
    rc, out = _icp(hip, *_ellipsoid(case), 1, case.iters)
    assert rc == 0 and torch.equal(al.matrix[0, :3].reshape(12), out["transform"][0]) and torch.equal(al.nearest.face, out["face"])
    assert torch.equal(al.nearest.dist2.view(torch.int32), out["dist2"].view(torch.int32)) and al.rank[-1].tolist() == [6]
    err = float(np.abs(al.matrix[0].cpu().numpy() - case.truth).max())
    line = f"RATIO align_to_mesh | iters {case.iters} | |M - truth| {err:.4g} (oracle {float(np.abs(ref.matrix - case.truth).max()):.4g})"
    for n in (4096, 65536):          # recorded, not asserted: the sampled route at equal iterations
        samples = fusion.sample_mesh(mesh, n)
        sampled = fusion.align_to_surface(source, samples, normals=fusion.sample_normals(mesh, samples), iters=case.iters)
        line += f" | align_to_surface at {n} samples {float(np.abs(sampled.matrix[0].cpu().numpy() - case.truth).max()):.4g}"
    print(line)
