"""The mesh-topology kernels (include/mvd_hip.h: the mesh topology section; csrc/meshtopo.hip) against tests/meshtopo_f64.py, through the
C ABI and through mvdfusion_amd/fusion.py.

  integers    incidence table, both label arrays, the component table, every per-scene total and vertex_flags: EQUAL on every element.
  filter      faces, both offset tables, both index maps, vertices and rgb: EQUAL (bit for bit), for the masks all, none, largest(1) and
              a seeded random half.
  smoothing   EQUAL bits after 1 pass and after iters = 10, pinned and free: every operation is an IEEE fp64 add, multiply or divide in
              the stated order without contraction, then one rounding to fp32.
  normals     within one fp32 rounding of the oracle's fp64 value (2^-24 relative per component, the bar of test_gpu_meshdist.py for
              `normal`); the number of components whose bits differ from the oracle's own rounding is printed.
  bit-equal   two runs of everything; a scene alone against the scene inside a batch; a refused call leaves sentinel-filled outputs and
              scratch untouched and names itself in mvd_last_error().
The cases are the smallest at which each kernel can still go wrong: fewer faces than a wavefront; nothing at all; a batch with an empty
middle scene; every face class in a batch with global ids; a component whose diameter is the mesh (4 097 triangles, ids permuted and
descending, many workgroups); a list longer than a wavefront that every face hooks to at once (a fan of 300); a component count that
crosses a scan block (257); a holed grid of 8 192 faces with permuted ids.
"""
import functools

import numpy as np
import pytest
import torch

import meshtopo_f64 as M

pytestmark = pytest.mark.gpu

CASES = ("tetrahedron", "empty", "hole", "mixed", "strip_permuted", "strip_descending", "fan", "tetrahedra", "grid")
LAM, MU = 0.5, -0.53


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


@functools.lru_cache(maxsize=None)
def _case(name):
    rng = np.random.default_rng(77)
    if name == "tetrahedron":
        return M.with_rgb(M.tetrahedron())
    if name == "empty":
        return M.make(np.zeros((0, 3)), np.zeros((0, 3)))
    if name == "hole":
        return M.with_rgb(M.concat([M.tetrahedron(), M.make(np.ones((2, 3)), np.zeros((0, 3))), M.cube(1)]), 1)
    if name == "mixed":
        return M.mixed_batch()
    if name == "strip_permuted":
        return M.with_rgb(M.permuted(M.strip(4097, seed=1), rng.permutation(4099)), 2)
    if name == "strip_descending":
        return M.permuted(M.strip(4097, seed=1), np.arange(4099)[::-1].copy())
    if name == "fan":
        return M.with_rgb(M.fan(300, seed=2), 4)
    if name == "tetrahedra":
        return M.tetrahedra(257)
    if name == "grid":
        g = M.quad_grid(64, seed=6, drop=0.05)
        return M.with_rgb(M.permuted(g, rng.permutation(len(g.vertices))), 5)
    raise KeyError(name)


def _masks(m):
    nf = len(m.faces)
    return dict(all=np.ones(nf, dtype=bool), none=np.zeros(nf, dtype=bool), largest=M.largest(m, M.components(m), 1),
                half=np.random.default_rng(nf + 11).random(nf) < 0.5)


def _reference(m):
    inc_start, inc = M.incidence(m)
    totals, flags = M.topology(m)
    ref = dict(M.components(m), inc_start=inc_start, inc=inc, totals=totals, vertex_flags=flags)
    n64, n32 = M.vertex_normals(m)
    ref.update(normals64=n64, normals=n32)
    for pin in (0, M.FLAG_BOUNDARY):
        ref[f"smooth1_{pin}"] = M.smooth(m, 1, LAM, MU, flags, pin)
        ref[f"smooth20_{pin}"] = M.smooth(m, 20, LAM, MU, flags, pin)
    return ref


@functools.lru_cache(maxsize=None)
def _ref(name):
    return _reference(_case(name))


def _i32(a):
    return torch.tensor(np.asarray(a), dtype=torch.int32).cuda()


def _p(hip, t):
    return hip.ptr(t) if t is not None and t.numel() else None


def _device(m):
    return dict(v=torch.from_numpy(m.vertices).cuda(), f=torch.from_numpy(m.faces).cuda(), vs=_i32(m.vertex_start), fs=_i32(m.face_start),
                nv=len(m.vertices), nf=len(m.faces), N=m.nscene)


def _scratch(nbytes):
    return torch.full(((int(nbytes) + 7) // 8,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda")


def _abi(hip, m):
    """Every entry but the filter through the C ABI into sentinel-filled outputs -> numpy arrays under the oracle's names."""
    L, p, st = hip.lib(), (lambda t: _p(hip, t)), hip.stream()
    d = _device(m)
    nv, nf, N = d["nv"], d["nf"], d["N"]
    i32 = lambda *s: torch.full(s, -77, dtype=torch.int32, device="cuda")
    f32 = lambda *s: torch.full(s, -7.25, dtype=torch.float32, device="cuda")
    mesh = (p(d["f"]), hip.ptr(d["vs"]), hip.ptr(d["fs"]), nv, nf, N)
    inc_start, inc = i32(nv + 1), i32(3 * nf)
    nb = int(L.mvd_mesh_incidence_scratch(nv, nf))
    assert nb > 0
    sc = _scratch(nb)
    assert L.mvd_mesh_incidence(*mesh, hip.ptr(inc_start), p(inc), hip.ptr(sc), nb, st) == 0, L.mvd_last_error()
    vc, fc, cs = i32(nv), i32(nf), i32(N + 1)
    nb = int(L.mvd_mesh_label_scratch(nv, nf))
    sc = _scratch(nb)
    assert L.mvd_mesh_label(*mesh, p(vc), p(fc), hip.ptr(cs), hip.ptr(sc), nb, st) == 0, L.mvd_last_error()
    ncomp = int(cs[N])
    root, cfaces, cverts = i32(ncomp), i32(ncomp), i32(ncomp)
    assert L.mvd_mesh_component_table(p(vc), p(fc), nv, nf, ncomp, p(root), p(cfaces), p(cverts), st) == 0, L.mvd_last_error()
    totals = i32(N, hip.TOPO_TOTALS)
    flags = torch.full((nv,), 0xab, dtype=torch.uint8, device="cuda")
    nb = int(L.mvd_mesh_topology_scratch(nv, nf))
    sc = _scratch(nb)
    assert L.mvd_mesh_topology(*mesh, hip.ptr(inc_start), p(inc), p(vc), hip.ptr(cs), hip.ptr(totals), p(flags), hip.ptr(sc), nb, st) == 0, \
        L.mvd_last_error()
    normals = f32(nv, 3)
    assert L.mvd_mesh_vertex_normals(p(d["v"]), p(d["f"]), hip.ptr(inc_start), p(inc), nv, nf, p(normals), st) == 0, L.mvd_last_error()
    out = dict(inc_start=inc_start, inc_all=inc, vertex_component=vc, face_component=fc, component_start=cs, root=root, faces=cfaces, vertices=cverts,
               totals=totals, vertex_flags=flags, normals=normals)
    for pin in (0, M.FLAG_BOUNDARY):
        for passes in (1, 20):
            res, tmp = f32(nv, 3), f32(nv, 3)
            assert L.mvd_mesh_smooth(p(d["v"]), p(d["f"]), hip.ptr(inc_start), p(inc), p(flags), nv, nf, passes, LAM, MU, pin, p(res), p(tmp), st) == 0, \
                L.mvd_last_error()
            out[f"smooth{passes}_{pin}"] = res
    out = {k: t.cpu().numpy() for k, t in out.items()}
    total = int(out["inc_start"][nv])
    out["inc"] = out["inc_all"][:total]
    assert (out.pop("inc_all")[total:] == -77).all()      # nothing behind the last list is touched
    return out


INTEGERS = ("inc_start", "inc", "vertex_component", "face_component", "component_start", "root", "faces", "vertices", "totals", "vertex_flags")
SMOOTHED = tuple(f"smooth{n}_{pin}" for n in (1, 20) for pin in (0, M.FLAG_BOUNDARY))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(out, ref, label):
    for k in INTEGERS:
        assert out[k].shape == ref[k].shape and out[k].dtype == ref[k].dtype, (label, k, out[k].shape, ref[k].shape, out[k].dtype)
        assert np.array_equal(out[k], ref[k]), (label, k, int((out[k] != ref[k]).sum()))
    for k in SMOOTHED:
        assert np.array_equal(_bits(out[k]), _bits(ref[k])), (label, k, int((_bits(out[k]) != _bits(ref[k])).sum()))
    differ = int((_bits(out["normals"]) != _bits(ref["normals"])).sum())
    err = np.abs(out["normals"].astype(np.float64) - ref["normals64"])
    print(f"{label}: normals {out['normals'].size} components, {differ} differ in bits from the oracle's rounding, max error "
          f"{float(err.max()) if err.size else 0.0:.3e}")
    assert (err <= 2.0 ** -24 * np.abs(ref["normals64"])).all(), (label, float(err.max()))


@pytest.mark.parametrize("name", CASES)
def test_every_entry_against_the_oracle(hip, name):
    _check(_abi(hip, _case(name)), _ref(name), name)


@pytest.mark.parametrize("name", CASES)
def test_two_runs_give_the_same_bits(hip, name):
    one, two = _abi(hip, _case(name)), _abi(hip, _case(name))
    for k in one:
        assert np.array_equal(one[k].view(np.uint8), two[k].view(np.uint8)), (name, k)


def _host_mesh(m):
    from mvdfusion_amd.fusion import TriangleMesh
    return TriangleMesh(vertices=torch.from_numpy(m.vertices).cuda(), faces=torch.from_numpy(m.faces).cuda(),
                        rgb=None if m.rgb is None else torch.from_numpy(m.rgb).cuda(),
                        vertex_start=torch.from_numpy(m.vertex_start).int(), face_start=torch.from_numpy(m.face_start).int())


def _same_mesh(got, want, label):
    assert np.array_equal(got.faces.cpu().numpy(), want.faces), label
    assert got.vertex_start.tolist() == want.vertex_start.tolist() and got.face_start.tolist() == want.face_start.tolist(), label
    assert np.array_equal(_bits(got.vertices.cpu().numpy()), _bits(want.vertices)), label
    assert (got.rgb is None) == (want.rgb is None) and (want.rgb is None or np.array_equal(_bits(got.rgb.cpu().numpy()), _bits(want.rgb))), label


@pytest.mark.parametrize("name", CASES)
def test_filter_against_the_oracle(hip, name):
    from mvdfusion_amd import fusion
    m = _case(name)
    mesh = _host_mesh(m)
    for label, keep in _masks(m).items():
        want, vi, fi = M.filter_faces(m, keep)
        got, gvi, gfi = fusion.filter_mesh(mesh, torch.from_numpy(keep).cuda(), return_index=True)
        _same_mesh(got, want, (name, label))
        assert gvi.dtype == gfi.dtype == torch.int32 and np.array_equal(gvi.cpu().numpy(), vi) and np.array_equal(gfi.cpu().numpy(), fi), (name, label)
        again = fusion.filter_mesh(mesh, torch.from_numpy(keep.astype(np.uint8)), return_index=False)
        _same_mesh(again, want, (name, label, "again"))
    if len(M.components(m)["root"]):
        _same_mesh(fusion.keep_components(mesh, largest=1), M.filter_faces(m, _masks(m)["largest"])[0], (name, "keep_components"))


@pytest.mark.parametrize("name", ("tetrahedron", "empty", "hole", "mixed", "fan", "grid"))
def test_the_host_api_is_the_abi_calls(hip, name):
    from mvdfusion_amd import fusion
    m, ref = _case(name), _ref(name)
    mesh = _host_mesh(m)
    comp, topo = fusion.mesh_components(mesh), fusion.mesh_topology(mesh)
    for k in ("vertex_component", "face_component", "component_start", "root", "faces", "vertices"):
        assert np.array_equal(getattr(comp, k).cpu().numpy(), ref[k]), (name, k)
    assert not comp.component_start.is_cuda and len(comp) == len(ref["root"])
    for k, field in enumerate(M.TOTALS):
        assert getattr(topo, field).tolist() == ref["totals"][:, k].tolist(), (name, field)
    assert np.array_equal(topo.vertex_flags.cpu().numpy(), ref["vertex_flags"])
    assert topo.closed.tolist() == (ref["totals"][:, 6] == 0).tolist() and topo.watertight.tolist() == (ref["totals"][:, 6:9] == 0).all(1).tolist()
    assert np.array_equal(comp.largest(1).cpu().numpy(), M.largest(m, M.components(m), 1))
    assert np.array_equal(comp.largest(2).cpu().numpy(), M.largest(m, M.components(m), 2))
    normals = fusion.vertex_normals(mesh)
    err = np.abs(normals.cpu().numpy().astype(np.float64) - ref["normals64"])
    assert normals.shape == mesh.vertices.shape and (err <= 2.0 ** -24 * np.abs(ref["normals64"])).all()
    for pin in (True, False):
        got = fusion.smooth_mesh(mesh, iters=10, pin_boundary=pin)
        assert np.array_equal(_bits(got.vertices.cpu().numpy()), _bits(ref[f"smooth20_{M.FLAG_BOUNDARY if pin else 0}"])), (name, pin)
        assert got.faces is mesh.faces and got.rgb is mesh.rgb
    assert torch.equal(fusion.smooth_mesh(mesh, iters=0).vertices, mesh.vertices)
    # min_faces / min_fraction against the oracle's component table
    c = M.components(m)
    if len(c["root"]):
        scene = np.repeat(np.arange(m.nscene), np.diff(c["component_start"]))
        total = np.bincount(scene, weights=c["faces"], minlength=m.nscene)[scene]
        keep = (c["faces"] >= 5) & (c["faces"].astype(np.float64) >= 0.3 * total)
        want = M.filter_faces(m, (c["face_component"] >= 0) & keep[np.maximum(c["face_component"], 0)])[0]
        _same_mesh(fusion.keep_components(mesh, min_faces=5, min_fraction=0.3), want, (name, "min_faces"))


def test_a_scene_alone_gives_what_it_gives_in_the_batch(hip):
    m = _case("mixed")
    batch = _abi(hip, m)
    comp_shift = {0: 0, 1: int(batch["component_start"][1])}
    for s in (0, 1):
        alone = _abi(hip, M.scene_of(m, s))
        v0, v1, f0, f1 = int(m.vertex_start[s]), int(m.vertex_start[s + 1]), int(m.face_start[s]), int(m.face_start[s + 1])
        c0, c1 = int(batch["component_start"][s]), int(batch["component_start"][s + 1])
        unshift = lambda a, by: np.where(a < 0, a, a - by)
        assert np.array_equal(alone["vertex_component"], unshift(batch["vertex_component"][v0:v1], comp_shift[s]))
        assert np.array_equal(alone["face_component"], unshift(batch["face_component"][f0:f1], comp_shift[s]))
        assert np.array_equal(alone["root"], batch["root"][c0:c1] - v0)
        assert np.array_equal(alone["faces"], batch["faces"][c0:c1]) and np.array_equal(alone["vertices"], batch["vertices"][c0:c1])
        assert np.array_equal(alone["totals"][0], batch["totals"][s]) and np.array_equal(alone["vertex_flags"], batch["vertex_flags"][v0:v1])
        lists = lambda o, a, b: [(o["inc"][o["inc_start"][v]:o["inc_start"][v + 1]]).tolist() for v in range(a, b)]
        assert lists(alone, 0, v1 - v0) == [[e - 3 * f0 for e in row] for row in lists(batch, v0, v1)]
        for k in SMOOTHED + ("normals",):
            assert np.array_equal(_bits(alone[k]), _bits(batch[k][v0:v1])), (s, k)


def test_refused_calls_write_nothing_and_name_themselves(hip):
    L, st = hip.lib(), hip.stream()
    m = _case("mixed")
    d = _device(m)
    nv, nf, N = d["nv"], d["nf"], d["N"]
    good = _abi(hip, m)
    dev = {k: torch.from_numpy(np.ascontiguousarray(good[k])).cuda() for k in ("inc_start", "vertex_component", "face_component", "component_start", "vertex_flags")}
    dev["inc"] = torch.from_numpy(np.concatenate([good["inc"], np.zeros(3 * nf - len(good["inc"]), dtype=np.int32)])).cuda()
    keep = torch.ones(nf, dtype=torch.uint8, device="cuda")
    ptr = hip.ptr
    outs = dict(a=torch.full((4 * (nv + nf) + 64,), -77, dtype=torch.int32, device="cuda"), b=torch.full((4 * (nv + nf) + 64,), -77, dtype=torch.int32, device="cuda"),
                c=torch.full((4 * (nv + nf) + 64,), -77, dtype=torch.int32, device="cuda"), scratch=_scratch(1 << 20))
    A, B, Cc, S = (outs[k].data_ptr() for k in ("a", "b", "c", "scratch"))
    V, F, VS, FS = (d[k].data_ptr() for k in ("v", "f", "vs", "fs"))
    IS, INC, VC, FC, CS, FL = (dev[k].data_ptr() for k in ("inc_start", "inc", "vertex_component", "face_component", "component_start", "vertex_flags"))
    big = 1 << 20
    entries = {
        "mvd_mesh_incidence": [F, VS, FS, nv, nf, N, A, B, S, big, st],
        "mvd_mesh_label": [F, VS, FS, nv, nf, N, A, B, Cc, S, big, st],
        "mvd_mesh_component_table": [VC, FC, nv, nf, 4, A, B, Cc, st],
        "mvd_mesh_topology": [F, VS, FS, nv, nf, N, IS, INC, VC, CS, A, B, S, big, st],
        "mvd_mesh_filter_count": [F, keep.data_ptr(), VS, FS, nv, nf, N, A, B, S, big, st],
        "mvd_mesh_filter_emit": [V, None, F, nv, nf, A, None, B, Cc, Cc + 4 * nv, nv, nf, S, big, st],
        "mvd_mesh_vertex_normals": [V, F, IS, INC, nv, nf, A, st],
        "mvd_mesh_smooth": [V, F, IS, INC, FL, nv, nf, 3, LAM, MU, 1, A, B, st],
    }
    # (entry, position, bad value): one argument wrong at a time
    with_mesh = ("mvd_mesh_incidence", "mvd_mesh_label", "mvd_mesh_topology")
    bad = [(e, 5, 0) for e in with_mesh] + [(e, 5, 65536) for e in with_mesh] + [(e, 4, 2 ** 31 // 3 + 1) for e in with_mesh] + \
        [(e, 3, 2 ** 31) for e in with_mesh] + [(e, 0, None) for e in with_mesh] + [(e, 1, None) for e in with_mesh] + [(e, 2, F + 2) for e in with_mesh]
    bad += [("mvd_mesh_incidence", 6, None), ("mvd_mesh_incidence", 7, None), ("mvd_mesh_incidence", 8, None), ("mvd_mesh_incidence", 8, S + 4),
            ("mvd_mesh_incidence", 9, 64), ("mvd_mesh_incidence", 6, A + 1),
            ("mvd_mesh_label", 6, None), ("mvd_mesh_label", 8, None), ("mvd_mesh_label", 9, None), ("mvd_mesh_label", 10, 64), ("mvd_mesh_label", 9, S + 8),
            ("mvd_mesh_component_table", 4, nv + 1), ("mvd_mesh_component_table", 0, None), ("mvd_mesh_component_table", 5, None),
            ("mvd_mesh_component_table", 3, 2 ** 31), ("mvd_mesh_component_table", 6, B + 2),
            ("mvd_mesh_topology", 6, None), ("mvd_mesh_topology", 8, None), ("mvd_mesh_topology", 9, None), ("mvd_mesh_topology", 10, None),
            ("mvd_mesh_topology", 11, None), ("mvd_mesh_topology", 12, None), ("mvd_mesh_topology", 13, 8), ("mvd_mesh_topology", 10, A + 2),
            ("mvd_mesh_filter_count", 6, 0), ("mvd_mesh_filter_count", 1, None), ("mvd_mesh_filter_count", 7, None), ("mvd_mesh_filter_count", 10, 64),
            ("mvd_mesh_filter_count", 9, None), ("mvd_mesh_filter_count", 5, 2 ** 31 // 3 + 1),
            ("mvd_mesh_filter_emit", 10, nv + 1), ("mvd_mesh_filter_emit", 11, nf + 1), ("mvd_mesh_filter_emit", 5, None), ("mvd_mesh_filter_emit", 8, None),
            ("mvd_mesh_filter_emit", 1, V), ("mvd_mesh_filter_emit", 12, None), ("mvd_mesh_filter_emit", 13, 64), ("mvd_mesh_filter_emit", 0, None),
            ("mvd_mesh_vertex_normals", 2, None), ("mvd_mesh_vertex_normals", 6, None), ("mvd_mesh_vertex_normals", 0, None),
            ("mvd_mesh_vertex_normals", 5, 2 ** 31 // 3 + 1), ("mvd_mesh_vertex_normals", 6, A + 2),
            ("mvd_mesh_smooth", 7, -1), ("mvd_mesh_smooth", 7, hip.SMOOTH_MAX_PASSES + 1), ("mvd_mesh_smooth", 8, float("nan")),
            ("mvd_mesh_smooth", 9, float("inf")), ("mvd_mesh_smooth", 10, 256), ("mvd_mesh_smooth", 10, -1), ("mvd_mesh_smooth", 4, None),
            ("mvd_mesh_smooth", 11, None), ("mvd_mesh_smooth", 12, None), ("mvd_mesh_smooth", 11, V), ("mvd_mesh_smooth", 12, A), ("mvd_mesh_smooth", 2, None)]
    for entry, pos, value in bad:
        args = list(entries[entry])
        args[pos] = value
        assert getattr(L, entry)(*args) != 0, (entry, pos, value)
        assert entry.encode() + b":" in L.mvd_last_error(), (entry, pos, value, L.mvd_last_error())
    torch.cuda.synchronize()
    for k in ("a", "b", "c"):
        assert bool((outs[k] == -77).all()), k
    assert bool((outs["scratch"] == 0x5a5a5a5a5a5a5a5a).all())
    for fn in ("incidence", "label", "topology", "filter"):
        scratch = getattr(L, f"mvd_mesh_{fn}_scratch")
        assert scratch(nv, nf) > 0 and scratch(0, 0) > 0 and scratch(2 ** 31, nf) == 0 and scratch(nv, 2 ** 31 // 3 + 1) == 0, fn
    # and every entry still works afterwards with the good arguments
    for entry, args in entries.items():
        assert getattr(L, entry)(*args) == 0, (entry, L.mvd_last_error())
    torch.cuda.synchronize()


def test_floaters_removed_end_to_end(hip):
    """Caller-made volumes at G = 24: the big sphere alone, and its minimum with three small spheres well away from it (the placement is
    checked on the oracle by test_cpu_meshtopo.py).  The marcher numbers vertices and faces in lattice order and U == B round the big
    surface, so dropping everything but the largest component of extract_mesh(U) must give extract_mesh(B) bit for bit."""
    from mvdfusion_amd import fusion
    B, U = M.blob_volumes("cuda")
    big, both = fusion.extract_mesh(B), fusion.extract_mesh(U)
    assert len(both) > len(big) > 1000
    topo = fusion.mesh_topology(both)
    got = (int(topo.components[0]), int(topo.boundary_edges[0]), int(topo.nonmanifold_edges[0]), int(topo.misoriented_edges[0]), int(topo.euler[0]))
    print(f"floaters: {len(both.vertices)} vertices {len(both)} faces, of which {len(both) - len(big)} in floaters | components, boundary, non-manifold, "
          f"misoriented, euler = {got}")
    assert got == (4, 0, 0, 0, 8) and bool(topo.watertight[0])
    kept, vi, fi = fusion.keep_components(both, largest=1, return_index=True)
    for k in ("vertices", "faces", "vertex_start", "face_start"):
        assert torch.equal(getattr(kept, k), getattr(big, k)), k
    assert kept.rgb is None and torch.equal(both.vertices[vi.long()], big.vertices) and int(fi.numel()) == len(big)
    comp = fusion.mesh_components(both)
    assert sorted(comp.faces.tolist())[-1] == len(big) and len(comp) == 4
    same = fusion.keep_components(both, min_fraction=0.5)
    assert torch.equal(same.faces, big.faces) and torch.equal(same.vertices, big.vertices)
    # and a batch of the two volumes: scene 0 keeps all it has, scene 1 loses its floaters
    pair = fusion.keep_components(fusion.extract_mesh(torch.stack([B, U])), largest=1)
    assert pair.face_start.tolist() == [0, len(big), 2 * len(big)] and torch.equal(pair.scene(1).vertices, big.vertices)
    assert torch.equal(pair.scene(1).faces, big.faces)


def test_viewfusion_mesh_forwards_the_new_keywords():
    """On the reduced-width model and the shapes of test_gpu_tsdf.py's round trip: the defaults give integrate_tsdf + extract_mesh bit for
    bit; largest = 1, smooth = 2 gives the sequence issued by hand."""
    from conftest import build_model
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.fusion import extract_mesh, integrate_tsdf, keep_components, smooth_mesh
    from test_gpu_fusion import _small_vae
    V, S, up, G = 2, 32, 2, 32
    m = build_model(32)
    inp = syn.make_inputs(V, S, seed=2)
    x = (0.5 * torch.randn(V, 5, S, S, generator=torch.Generator().manual_seed(8))).cuda()
    assert not hasattr(m, "vae")
    m.vae = _small_vae()
    try:
        kw = dict(half_extent=1.5, trunc=0.5, fill=(0.0, 1.0, 0.0))
        img = m.decode(x[:, :4])
        vol = integrate_tsdf(x, inp["batch_cameras"], rgb=img, grid=G, up=up, depth_scale=m.view_attn.depth_scale,
                             depth_shift=m.view_attn.depth_shift, half_extent=kw["half_extent"], trunc=kw["trunc"])
        want = extract_mesh(vol, fill=kw["fill"])
        plain = m.mesh(x, inp["batch_cameras"], grid=G, up=up, **kw)
        fields = ("vertices", "faces", "rgb", "vertex_start", "face_start")
        for k in fields:
            assert torch.equal(getattr(plain, k), getattr(want, k)), k
        cleaned = m.mesh(x, inp["batch_cameras"], grid=G, up=up, largest=1, smooth=2, **kw)
        by_hand = smooth_mesh(keep_components(want, largest=1), iters=2)
        for k in fields:
            assert torch.equal(getattr(cleaned, k), getattr(by_hand, k)), k
        assert 0 < len(cleaned) <= len(want) and bool(torch.isfinite(cleaned.vertices).all())
    finally:
        del m.vae
