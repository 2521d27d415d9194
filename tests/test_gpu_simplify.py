"""The mesh simplification kernels (include/mvd_hip.h: the mesh simplification section; csrc/meshsimplify.hip) against
tests/simplify_f64.py, through the C ABI into sentinel-filled outputs and through fusion.simplify_mesh.

  integers   vertex_cluster, cluster_start, size, rank, placed, mapped_faces, both keep masks, and the final faces, offsets and index
             maps: EQUAL on every element.
  mean       vertices with placement "mean", and rgb always: EQUAL in bits (fp64 sums in the stated order, one division, one rounding).
  quadric    |gpu - x64| <= 2^-24 |x64| + 1e-9 h per coordinate: one fp32 rounding (the bar test_gpu_meshtopo.py sets for normals) plus
             the fp64 error of a solve whose kept eigenvalues span at most 1e3 (about 1e3 x a few hundred eps; it matters where a
             coordinate is near 0).
  bit-equal  two runs; a scene alone against the scene inside a batch; a refused call leaves outputs and scratch at their sentinels.
No cluster and no face is left out of a comparison: tests/test_cpu_simplify.py asserts that every decision of every fixture here has a
margin above 1e-6.  The fixtures (simplify_f64.GPU_CASES) are the smallest at which each kernel can still go wrong: fewer rows than a
wavefront; nothing at all; a batch with an empty middle scene; every face class with global ids and a box per scene; the subdivided
cube; 4 099 permuted ids in one, two and many clusters (a member list longer than 4 096, many workgroups); about 4 200 occupied cells
(the cluster count crosses a scan chunk) and the same grid in 76; a fan of 300; a two-sheet plate (duplicates); NaN and inf vertices.
"""
import functools
import math

import numpy as np
import pytest
import torch

import meshtopo_f64 as M
import simplify_f64 as S

pytestmark = pytest.mark.gpu

RUNS = [(name, cells) for name in S.GPU_CASES for cells in S.GPU_CASES[name]]
PLACEMENTS = {"quadric": S.QUADRIC, "mean": S.MEAN}
INTEGERS = ("vertex_cluster", "cluster_start", "size", "rank", "placed", "mapped_faces", "keep", "keep_deduped")
SENT_I, SENT_F, SENT_B, SENT_S = -77, -7.25, 0xab, 0x5a5a5a5a5a5a5a5a


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


@functools.lru_cache(maxsize=None)
def _ref(name, cells, placement):
    return S.simplify(S.gpu_case(name), cells, placement)


def _i32(a):
    return torch.tensor(np.asarray(a), dtype=torch.int32).cuda()


def _device(m):
    return dict(v=torch.from_numpy(m.vertices).cuda(), f=torch.from_numpy(m.faces).cuda(), c=None if m.rgb is None else torch.from_numpy(m.rgb).cuda(),
                vs=_i32(m.vertex_start), fs=_i32(m.face_start), nv=len(m.vertices), nf=len(m.faces), N=m.nscene)


def _scratch(nbytes):
    return torch.full(((int(nbytes) + 7) // 8,), SENT_S, dtype=torch.int64, device="cuda")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _incidence(hip, faces, vs, fs, nv, nf, N):
    L, p = hip.lib(), (lambda t: hip.ptr(t) if t is not None and t.numel() else None)
    inc_start, inc = torch.full((nv + 1,), SENT_I, dtype=torch.int32, device="cuda"), torch.full((3 * nf,), SENT_I, dtype=torch.int32, device="cuda")
    nb = int(L.mvd_mesh_incidence_scratch(nv, nf))
    sc = _scratch(nb)
    assert L.mvd_mesh_incidence(p(faces), hip.ptr(vs), hip.ptr(fs), nv, nf, N, hip.ptr(inc_start), p(inc), hip.ptr(sc), nb, hip.stream()) == 0, L.mvd_last_error()
    return inc_start, inc


def _abi(hip, m, cells, placement):
    """The three entries through the C ABI into sentinel-filled outputs -> numpy arrays under the oracle's names."""
    L, p, st = hip.lib(), (lambda t: hip.ptr(t) if t is not None and t.numel() else None), hip.stream()
    d = _device(m)
    nv, nf, N = d["nv"], d["nf"], d["N"]
    i32 = lambda *s: torch.full(s, SENT_I, dtype=torch.int32, device="cuda")
    f32 = lambda *s: torch.full(s, SENT_F, dtype=torch.float32, device="cuda")
    u8 = lambda *s: torch.full(s, SENT_B, dtype=torch.uint8, device="cuda")
    inc_start, inc = _incidence(hip, d["f"], d["vs"], d["fs"], nv, nf, N)
    nb = int(L.mvd_mesh_cluster_scratch(nv, nf, N, cells))
    assert nb > 0
    sc = _scratch(nb)
    vc, cs = i32(nv), i32(N + 1)
    assert L.mvd_mesh_cluster_count(p(d["v"]), hip.ptr(d["vs"]), hip.ptr(inc_start), nv, nf, N, cells, p(vc), hip.ptr(cs), hip.ptr(sc), nb, st) == 0, \
        L.mvd_last_error()
    nc = int(cs[N])
    out_v, out_c = f32(nc, 3), (f32(nc, 3) if d["c"] is not None else None)
    size, rank, placed, mapped, keep, keep2 = i32(nc), i32(nc), i32(nc), i32(nf, 3), u8(nf), u8(nf)
    assert L.mvd_mesh_cluster_emit(p(d["v"]), p(d["c"]), p(d["f"]), hip.ptr(d["vs"]), hip.ptr(d["fs"]), hip.ptr(inc_start), p(inc), p(vc), nv, nf, N, cells,
                                   placement, nc, p(out_v), p(out_c), p(size), p(rank), p(placed), p(mapped), p(keep), hip.ptr(sc), nb, st) == 0, \
        L.mvd_last_error()
    cinc_start, cinc = _incidence(hip, mapped, cs, d["fs"], nc, nf, N)
    assert L.mvd_mesh_cluster_dedupe(p(mapped), p(keep), hip.ptr(cinc_start), p(cinc), nc, nf, p(keep2), st) == 0, L.mvd_last_error()
    out = dict(vertex_cluster=vc, cluster_start=cs, vertices=out_v, size=size, rank=rank, placed=placed, mapped_faces=mapped, keep=keep, keep_deduped=keep2)
    if out_c is not None:
        out["rgb"] = out_c
    return {k: t.cpu().numpy() for k, t in out.items()}


def _close(got, want64, h, label):
    err = np.abs(got.astype(np.float64) - want64)
    bound = 2.0 ** -24 * np.abs(want64) + 1e-9 * np.asarray(h)[:, None]
    differ = int((_bits(got) != _bits(want64.astype(np.float32))).sum())
    print(f"{label}: {got.size} coordinates, {differ} differ in bits from the oracle's rounding, worst error / bound "
          f"{float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0:.3f}")
    assert (err <= bound).all(), (label, float(err.max()))


def _check(out, ref, placement, label):
    for k in INTEGERS:
        assert out[k].shape == ref[k].shape and out[k].dtype == ref[k].dtype, (label, k, out[k].shape, ref[k].shape, out[k].dtype, ref[k].dtype)
        assert np.array_equal(out[k], ref[k]), (label, k, int((out[k] != ref[k]).sum()))
    if ref["rgb"] is not None:
        assert np.array_equal(_bits(out["rgb"]), _bits(ref["rgb"])), (label, "rgb")
    if placement == S.MEAN:
        assert np.array_equal(_bits(out["vertices"]), _bits(ref["vertices"])), (label, "vertices")
    else:
        _close(out["vertices"], ref["vertices64"], ref["h"], label)


@pytest.mark.parametrize("placement", sorted(PLACEMENTS))
@pytest.mark.parametrize("name,cells", RUNS)
def test_every_entry_against_the_oracle(hip, name, cells, placement):
    out = _abi(hip, S.gpu_case(name), cells, PLACEMENTS[placement])
    _check(out, _ref(name, cells, PLACEMENTS[placement]), PLACEMENTS[placement], (name, cells, placement))


@pytest.mark.parametrize("name,cells", RUNS)
def test_two_runs_give_the_same_bits(hip, name, cells):
    one, two = _abi(hip, S.gpu_case(name), cells, S.QUADRIC), _abi(hip, S.gpu_case(name), cells, S.QUADRIC)
    for k in one:
        assert np.array_equal(one[k].view(np.uint8), two[k].view(np.uint8)), (name, cells, k)


def _host_mesh(m):
    from mvdfusion_amd.fusion import TriangleMesh
    return TriangleMesh(vertices=torch.from_numpy(m.vertices).cuda(), faces=torch.from_numpy(m.faces).cuda(),
                        rgb=None if m.rgb is None else torch.from_numpy(m.rgb).cuda(),
                        vertex_start=torch.from_numpy(m.vertex_start).int(), face_start=torch.from_numpy(m.face_start).int())


@pytest.mark.parametrize("placement", sorted(PLACEMENTS))
@pytest.mark.parametrize("name,cells", RUNS)
def test_simplify_mesh_against_the_oracle(hip, name, cells, placement):
    from mvdfusion_amd import fusion
    ref = _ref(name, cells, PLACEMENTS[placement])
    mesh = _host_mesh(S.gpu_case(name))
    got, vc, fi, cl = fusion.simplify_mesh(mesh, cells=cells, placement=placement, return_index=True)
    want = ref["out"]
    label = (name, cells, placement)
    assert got.faces.dtype == torch.int32 and np.array_equal(got.faces.cpu().numpy(), want.faces), label
    assert got.vertex_start.tolist() == want.vertex_start.tolist() and got.face_start.tolist() == want.face_start.tolist(), label
    assert not got.vertex_start.is_cuda and not got.face_start.is_cuda
    for t, w in ((vc, ref["final_vertex_cluster"]), (fi, ref["face_index"]), (cl.size, ref["final_size"]), (cl.rank, ref["final_rank"]),
                 (cl.placed, ref["final_placed"])):
        assert t.dtype == torch.int32 and np.array_equal(t.cpu().numpy(), w), label
    assert len(cl) == len(want.vertices)
    assert (got.rgb is None) == (want.rgb is None) and (want.rgb is None or np.array_equal(_bits(got.rgb.cpu().numpy()), _bits(want.rgb))), label
    if placement == "mean":
        assert np.array_equal(_bits(got.vertices.cpu().numpy()), _bits(want.vertices)), label
    else:
        _close(got.vertices.cpu().numpy(), ref["out64"], ref["out_h"], label)
    plain = fusion.simplify_mesh(mesh, cells=cells, placement=placement)
    assert torch.equal(plain.faces, got.faces) and np.array_equal(_bits(plain.vertices.cpu().numpy()), _bits(got.vertices.cpu().numpy())), label


def test_a_scene_alone_gives_what_it_gives_in_the_batch(hip):
    for name, cells in (("mixed", 4), ("hole", 2)):
        m = S.gpu_case(name)
        batch = _abi(hip, m, cells, S.QUADRIC)
        for s in range(m.nscene):
            alone = _abi(hip, M.scene_of(m, s), cells, S.QUADRIC)
            v0, v1, f0, f1 = int(m.vertex_start[s]), int(m.vertex_start[s + 1]), int(m.face_start[s]), int(m.face_start[s + 1])
            c0, c1 = int(batch["cluster_start"][s]), int(batch["cluster_start"][s + 1])
            unshift = lambda a: np.where(a < 0, a, a - c0)
            assert alone["cluster_start"].tolist() == [0, c1 - c0], (name, s)
            assert np.array_equal(alone["vertex_cluster"], unshift(batch["vertex_cluster"][v0:v1])), (name, s)
            assert np.array_equal(alone["mapped_faces"], unshift(batch["mapped_faces"][f0:f1])), (name, s)
            for k in ("keep", "keep_deduped"):
                assert np.array_equal(alone[k], batch[k][f0:f1]), (name, s, k)
            for k in ("size", "rank", "placed"):
                assert np.array_equal(alone[k], batch[k][c0:c1]), (name, s, k)
            for k in ("vertices", "rgb"):
                assert np.array_equal(_bits(alone[k]), _bits(batch[k][c0:c1])), (name, s, k)


def test_refused_calls_write_nothing_and_name_themselves(hip):
    L, st = hip.lib(), hip.stream()
    m, cells = S.gpu_case("mixed"), 4
    d = _device(m)
    nv, nf, N = d["nv"], d["nf"], d["N"]
    inc_start, inc = _incidence(hip, d["f"], d["vs"], d["fs"], nv, nf, N)
    good = _abi(hip, m, cells, S.QUADRIC)
    nc = len(good["size"])
    vc, cs, mapped = _i32(good["vertex_cluster"]), _i32(good["cluster_start"]), _i32(good["mapped_faces"])
    keep = torch.from_numpy(good["keep"]).cuda()
    cinc_start, cinc = _incidence(hip, mapped, cs, d["fs"], nc, nf, N)
    nb = int(L.mvd_mesh_cluster_scratch(nv, nf, N, cells))
    outs = {k: torch.full((4 * (nv + nf) + 64,), SENT_I, dtype=torch.int32, device="cuda") for k in "abcdefg"}
    outs["scratch"] = _scratch(nb)
    A, B, Cc, D, E, F_, G, SC = (outs[k].data_ptr() for k in ("a", "b", "c", "d", "e", "f", "g", "scratch"))
    V, RGB, F, VS, FS, IS, INC, VC = (t.data_ptr() for t in (d["v"], d["c"], d["f"], d["vs"], d["fs"], inc_start, inc, vc))
    entries = {
        "mvd_mesh_cluster_count": [V, VS, IS, nv, nf, N, cells, A, B, SC, nb, st],
        "mvd_mesh_cluster_emit": [V, RGB, F, VS, FS, IS, INC, VC, nv, nf, N, cells, S.QUADRIC, nc, A, B, Cc, D, E, F_, G, SC, nb, st],
        "mvd_mesh_cluster_dedupe": [mapped.data_ptr(), keep.data_ptr(), cinc_start.data_ptr(), cinc.data_ptr(), nc, nf, A, st],
    }
    bad = [("mvd_mesh_cluster_count", 0, None), ("mvd_mesh_cluster_count", 1, None), ("mvd_mesh_cluster_count", 2, None),
           ("mvd_mesh_cluster_count", 3, 2 ** 31), ("mvd_mesh_cluster_count", 4, 2 ** 31 // 3 + 1), ("mvd_mesh_cluster_count", 5, 0),
           ("mvd_mesh_cluster_count", 5, 65536), ("mvd_mesh_cluster_count", 6, 0), ("mvd_mesh_cluster_count", 6, 257), ("mvd_mesh_cluster_count", 6, -3),
           ("mvd_mesh_cluster_count", 7, None), ("mvd_mesh_cluster_count", 8, None), ("mvd_mesh_cluster_count", 7, A + 2), ("mvd_mesh_cluster_count", 9, None),
           ("mvd_mesh_cluster_count", 9, SC + 8), ("mvd_mesh_cluster_count", 10, nb - 16), ("mvd_mesh_cluster_count", 10, 64),
           ("mvd_mesh_cluster_emit", 0, None), ("mvd_mesh_cluster_emit", 2, None), ("mvd_mesh_cluster_emit", 3, None), ("mvd_mesh_cluster_emit", 4, None),
           ("mvd_mesh_cluster_emit", 5, None), ("mvd_mesh_cluster_emit", 6, None), ("mvd_mesh_cluster_emit", 7, None), ("mvd_mesh_cluster_emit", 10, 0),
           ("mvd_mesh_cluster_emit", 11, 0), ("mvd_mesh_cluster_emit", 11, 257), ("mvd_mesh_cluster_emit", 12, 2), ("mvd_mesh_cluster_emit", 12, -1),
           ("mvd_mesh_cluster_emit", 13, nv + 1), ("mvd_mesh_cluster_emit", 14, None), ("mvd_mesh_cluster_emit", 15, None), ("mvd_mesh_cluster_emit", 16, None),
           ("mvd_mesh_cluster_emit", 17, None), ("mvd_mesh_cluster_emit", 18, None), ("mvd_mesh_cluster_emit", 19, None), ("mvd_mesh_cluster_emit", 20, None),
           ("mvd_mesh_cluster_emit", 14, A + 2), ("mvd_mesh_cluster_emit", 21, None), ("mvd_mesh_cluster_emit", 21, SC + 4), ("mvd_mesh_cluster_emit", 22, nb - 16),
           ("mvd_mesh_cluster_emit", 9, 2 ** 31 // 3 + 1),
           ("mvd_mesh_cluster_dedupe", 0, None), ("mvd_mesh_cluster_dedupe", 1, None), ("mvd_mesh_cluster_dedupe", 2, None), ("mvd_mesh_cluster_dedupe", 3, None),
           ("mvd_mesh_cluster_dedupe", 6, None), ("mvd_mesh_cluster_dedupe", 6, keep.data_ptr()), ("mvd_mesh_cluster_dedupe", 4, 2 ** 31),
           ("mvd_mesh_cluster_dedupe", 5, 2 ** 31 // 3 + 1), ("mvd_mesh_cluster_dedupe", 0, mapped.data_ptr() + 2)]
    for entry, pos, value in bad:
        args = list(entries[entry])
        args[pos] = value
        assert getattr(L, entry)(*args) != 0, (entry, pos, value)
        assert entry.encode() + b":" in L.mvd_last_error(), (entry, pos, value, L.mvd_last_error())
    torch.cuda.synchronize()
    for k in "abcdefg":
        assert bool((outs[k] == SENT_I).all()), k
    assert bool((outs["scratch"] == SENT_S).all())
    assert L.mvd_mesh_cluster_scratch(nv, nf, N, cells) > 0 and L.mvd_mesh_cluster_scratch(0, 0, 1, 1) > 0
    for args in ((2 ** 31, nf, N, cells), (nv, 2 ** 31 // 3 + 1, N, cells), (nv, nf, 0, cells), (nv, nf, N, 0), (nv, nf, N, 257), (nv, nf, 17, 256)):
        assert L.mvd_mesh_cluster_scratch(*args) == 0, args
    # an nc other than the count call's: compared on the device, so the call returns 0 -- and writes nothing, neither outputs nor scratch
    assert L.mvd_mesh_cluster_count(*entries["mvd_mesh_cluster_count"]) == 0, L.mvd_last_error()
    torch.cuda.synchronize()
    assert int(outs["b"][N]) == nc
    outs["a"].fill_(SENT_I), outs["b"].fill_(SENT_I)
    before = outs["scratch"].clone()
    for wrong in (nc - 1, nc + 1, 0):
        args = list(entries["mvd_mesh_cluster_emit"])
        args[13] = wrong
        assert L.mvd_mesh_cluster_emit(*args) == 0, L.mvd_last_error()
    torch.cuda.synchronize()
    for k in "abcdefg":
        assert bool((outs[k] == SENT_I).all()), k
    assert torch.equal(outs["scratch"], before)
    # and every entry still works afterwards with the good arguments
    assert L.mvd_mesh_cluster_emit(*entries["mvd_mesh_cluster_emit"]) == 0, L.mvd_last_error()
    assert L.mvd_mesh_cluster_dedupe(*entries["mvd_mesh_cluster_dedupe"]) == 0, L.mvd_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(outs["c"][:nc].cpu().numpy(), good["size"]) and np.array_equal(outs["f"][:3 * nf].cpu().numpy().reshape(nf, 3), good["mapped_faces"])
    assert np.array_equal(outs["a"].view(torch.uint8)[:nf].cpu().numpy(), good["keep_deduped"])


def test_marched_sphere_end_to_end(hip):
    """The G = 24 sphere of radius 0.45 of test_gpu_meshtopo.py's end-to-end case at cells = 8: fewer faces, and every member vertex of the
    input within sqrt(3) h (1 + 1 / 512) of the result -- a vertex of the grown cell is within the cell's diagonal of every member, and
    every cluster keeps its vertex (asserted here on the extracted mesh and in test_cpu_simplify.py on the oracle's), so no member is
    left out."""
    from mvdfusion_amd import fusion
    B, _ = M.blob_volumes("cuda")
    mesh = fusion.extract_mesh(B)
    out, vc, fi, cl = fusion.simplify_mesh(mesh, cells=8, return_index=True)
    ref = S.simplify(M.make(mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()), 8)
    assert len(ref["vertex_index"]) == len(ref["members"]) == len(out.vertices) and np.array_equal(out.faces.cpu().numpy(), ref["out"].faces)
    assert 0 < len(out) < len(mesh)
    member = vc >= 0
    assert bool(member.all()) and int(cl.size.sum()) == len(mesh.vertices)
    h = float(ref["h"][0])
    near = fusion.nearest_on_mesh(mesh.vertices[member], out)
    worst = float(near.dist2.max().sqrt())
    topo = fusion.mesh_topology(out)
    print(f"marched sphere G=24 cells=8: {len(mesh)} -> {len(out)} faces, {len(mesh.vertices)} -> {len(out.vertices)} vertices; worst member distance "
          f"{worst / h:.3f} h (bound {math.sqrt(3.0) * (1 + 1 / 512):.3f} h); boundary, non-manifold edges = "
          f"{int(topo.boundary_edges[0])}, {int(topo.nonmanifold_edges[0])}; placed fallback {int((cl.placed == 2).sum())}")
    assert worst <= math.sqrt(3.0) * h * (1.0 + 1.0 / 512.0)


def test_viewfusion_mesh_forwards_simplify():
    """On the reduced-width model and the shapes of test_gpu_meshtopo.py's keyword test: simplify = None gives integrate_tsdf +
    extract_mesh bit for bit; simplify = 8 behind largest and smooth gives the sequence issued by hand."""
    from conftest import build_model
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.fusion import extract_mesh, integrate_tsdf, keep_components, simplify_mesh, smooth_mesh
    from test_gpu_fusion import _small_vae
    V, S_, up, G = 2, 32, 2, 32
    m = build_model(32)
    inp = syn.make_inputs(V, S_, seed=2)
    x = (0.5 * torch.randn(V, 5, S_, S_, generator=torch.Generator().manual_seed(8))).cuda()
    assert not hasattr(m, "vae")
    m.vae = _small_vae()
    try:
        kw = dict(half_extent=1.5, trunc=0.5, fill=(0.0, 1.0, 0.0))
        img = m.decode(x[:, :4])
        vol = integrate_tsdf(x, inp["batch_cameras"], rgb=img, grid=G, up=up, depth_scale=m.view_attn.depth_scale,
                             depth_shift=m.view_attn.depth_shift, half_extent=kw["half_extent"], trunc=kw["trunc"])
        want = extract_mesh(vol, fill=kw["fill"])
        fields = ("vertices", "faces", "rgb", "vertex_start", "face_start")
        plain = m.mesh(x, inp["batch_cameras"], grid=G, up=up, simplify=None, **kw)
        for k in fields:
            assert torch.equal(getattr(plain, k), getattr(want, k)), k
        coarse = m.mesh(x, inp["batch_cameras"], grid=G, up=up, simplify=8, **kw)
        by_hand = simplify_mesh(want, cells=8)
        for k in fields:
            assert torch.equal(getattr(coarse, k), getattr(by_hand, k)), k
        assert 0 < len(coarse) < len(want) and bool(torch.isfinite(coarse.vertices).all())
        cleaned = m.mesh(x, inp["batch_cameras"], grid=G, up=up, largest=1, smooth=2, simplify=8, **kw)
        last = simplify_mesh(smooth_mesh(keep_components(want, largest=1), iters=2), cells=8)
        for k in fields:
            assert torch.equal(getattr(cleaned, k), getattr(last, k)), k
    finally:
        del m.vae
