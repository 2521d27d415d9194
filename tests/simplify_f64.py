"""Integer / float64 restatement of the mesh simplification section of include/mvd_hip.h (csrc/meshsimplify.hip): members, the box and
grid of a scene, cluster ids, the ascending member lists, the per-vertex and per-cluster quadric sums, the 3 x 3 Jacobi in the kernel's
sweep order, the placement with its acceptance box, the mapped faces with both keep masks, and the final compaction.  Not collected by
pytest; tests/test_cpu_simplify.py holds it to answers known by hand, tests/test_gpu_simplify.py holds the kernels to it.

Every float64 operation is one Python float operation (IEEE binary64, round to nearest) in the order the header states, in plain
loops where numpy would reorder a sum; the single rounding to fp32 is where the header says.

MARGINS.  For every decision that a last-bit difference could flip, `simplify` also returns how far the decided value was from the
threshold:
  eig    per cluster: |lambda_i / lambda_max - 1e-3| / 1e-3, the least over i (inf where lambda_max is not positive);
  box    per cluster whose quadric point was tested: the least signed distance of y to the six faces of the grown box, over h, in
         absolute value (the point is inside iff that least distance is >= 0);
  cell   per member and axis: the distance of u = (x_a - lo_a) / h to the nearest of the integers 1 .. n_a - 1, the only values at
         which the cell changes (u == 0 of the box's own corner and the clamped top are no thresholds);
  grid   per scene and axis: the distance of extent_a / h to the nearest of the integers 1 .. cells - 1, where n_a changes.
  A `cell` or `grid` margin below 1e-6 counts as inf when the computed float64 quotient EQUALS the exact rational quotient of the fp32
  inputs (checked with fractions.Fraction): the decision is then that of exact arithmetic and no rounding took part in it.  A grid of
  vertices at i / 64 clustered with cells = 64 sits on every threshold by construction and is exact throughout.
"""
import math
from fractions import Fraction

import numpy as np

import meshtopo_f64 as M

MAX_CELLS, MAX_TABLE = 256, 2 ** 28
MEAN, QUADRIC = 0, 1
PLACED_MEAN, PLACED_QUADRIC, PLACED_FALLBACK = 0, 1, 2
RANK_RATIO, BOX_SLACK_DIV = 1e-3, 1024
SWEEPS, THETA_BIG = 10, 1e150
INF = float("inf")


def jacobi3(A):
    """The cyclic Jacobi of csrc/jacobi3.hpp on a symmetric 3 x 3 (lists of Python floats) -> (A diagonalised, V with the eigenvectors in
    its columns)."""
    A = [list(r) for r in A]
    V = [[1.0 if r == c else 0.0 for c in range(3)] for r in range(3)]
    for _ in range(SWEEPS):
        for p in range(2):
            for q in range(p + 1, 3):
                apq = A[p][q]
                if apq != 0.0:
                    theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                    at = abs(theta)
                    t = 0.5 / at if at > THETA_BIG else 1.0 / (at + math.sqrt(at * at + 1.0))
                    if theta < 0.0:
                        t = -t
                    c = 1.0 / math.sqrt(t * t + 1.0)
                    sn = t * c
                    for k in range(3):
                        akp, akq = A[k][p], A[k][q]
                        A[k][p], A[k][q] = c * akp - sn * akq, sn * akp + c * akq
                    for k in range(3):
                        apk, aqk = A[p][k], A[q][k]
                        A[p][k], A[q][k] = c * apk - sn * aqk, sn * apk + c * aqk
                    A[p][q] = A[q][p] = 0.0
                    for k in range(3):
                        vkp, vkq = V[k][p], V[k][q]
                        V[k][p], V[k][q] = c * vkp - sn * vkq, sn * vkp + c * vkq
    return A, V


def _near_integer(u, top):
    """The distance of u to the nearest of the integers 1 .. top (inf without one)."""
    if top < 1:
        return INF
    k = min(max(round(u), 1), top)
    return abs(u - k)


def _vertex_scene(m):
    nv = len(m.vertices)
    vs = np.clip(m.vertex_start, 0, nv)
    v = np.arange(nv)
    scene = np.searchsorted(vs, v, side="right") - 1
    return np.where((v >= vs[0]) & (v < vs[-1]), np.minimum(scene, m.nscene - 1), -1)


def clusters(m, cells):
    """The count call: dict(vertex_cluster, cluster_start, grid (per scene: lo, h, n), cell (nv, 3), members (list per cluster,
    ascending), margins cell / grid)."""
    assert 1 <= cells <= MAX_CELLS and m.nscene * cells ** 3 <= MAX_TABLE
    nv = len(m.vertices)
    inc_start, _ = M.incidence(m)
    scene = _vertex_scene(m)
    member = (scene >= 0) & np.isfinite(m.vertices).all(1) & (np.diff(inc_start.astype(np.int64)) > 0) if nv else np.zeros(0, dtype=bool)
    grids, grid_margin = [], INF
    for s in range(m.nscene):
        mine = np.nonzero(member & (scene == s))[0]
        if len(mine) == 0:
            grids.append(None)
            continue
        lo32, hi32 = m.vertices[mine].min(0), m.vertices[mine].max(0)
        lo = [float(lo32[a]) for a in range(3)]
        ext = [float(hi32[a]) - lo[a] for a in range(3)]
        exact = [Fraction(float(hi32[a])) - Fraction(lo[a]) for a in range(3)]      # the extents without the float64 rounding
        big = 0.0
        for a in range(3):
            big = ext[a] if ext[a] > big else big
        h = big / float(cells)
        n = [1, 1, 1]
        if h > 0.0:
            for a in range(3):
                q = ext[a] / h
                n[a] = int(min(max(math.floor(q) + 1.0, 1.0), float(cells)))
                d = _near_integer(q, cells - 1)
                if d < 1e-6 and Fraction(q) == exact[a] * cells / max(exact):
                    d = INF
                grid_margin = min(grid_margin, d)
        grids.append(dict(lo=lo, h=h, n=n, big=max(exact)))
    cell = np.zeros((nv, 3), dtype=np.int64)
    word = np.full(nv, -1, dtype=np.int64)
    cell_margin = INF
    for v in np.nonzero(member)[0]:
        G = grids[scene[v]]
        if G["h"] > 0.0:
            for a in range(3):
                x = float(m.vertices[v, a])
                u = (x - G["lo"][a]) / G["h"]
                cell[v, a] = int(min(max(math.floor(u), 0.0), float(G["n"][a] - 1)))
                d = _near_integer(u, G["n"][a] - 1)
                if d < 1e-6 and Fraction(u) == (Fraction(x) - Fraction(G["lo"][a])) * cells / G["big"]:
                    d = INF
                cell_margin = min(cell_margin, d)
        word[v] = scene[v] * cells ** 3 + (cell[v, 2] * G["n"][1] + cell[v, 1]) * G["n"][0] + cell[v, 0]
    occupied = np.unique(word[member])
    vc = np.full(nv, -1, dtype=np.int32)
    vc[member] = np.searchsorted(occupied, word[member]).astype(np.int32)
    cluster_start = np.searchsorted(occupied, np.arange(m.nscene + 1) * cells ** 3).astype(np.int32)
    members = [[] for _ in range(len(occupied))]
    for v in np.nonzero(member)[0]:
        members[vc[v]].append(int(v))
    return dict(vertex_cluster=vc, cluster_start=cluster_start, grid=grids, cell=cell, members=members, scene=scene,
                margins=dict(cell=cell_margin, grid=grid_margin))


def vertex_quadrics(m, member):
    """(nv, 9) float64: A_v (xx xy xz yy yz zz) and g_v per member, summed over its incidence list in list order."""
    inc_start, inc = M.incidence(m)
    x = m.vertices
    fin = np.isfinite(x).all(1)
    quad = np.zeros((len(x), 9), dtype=np.float64)
    for v in np.nonzero(member)[0]:
        q = [0.0] * 9
        for ent in inc[inc_start[v]:inc_start[v + 1]]:
            ids = m.faces[ent // 3]
            if not fin[ids].all():
                continue
            T = [[float(x[i, a]) for a in range(3)] for i in ids]
            ab = [T[1][a] - T[0][a] for a in range(3)]
            ac = [T[2][a] - T[0][a] for a in range(3)]
            n = [ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]]
            ln = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            if not (ln > 0.0) or not math.isfinite(ln):
                continue
            u = [n[0] / ln, n[1] / ln, n[2] / ln]
            w = ln / 2.0
            wu = [w * u[0], w * u[1], w * u[2]]
            d = (u[0] * T[0][0] + u[1] * T[0][1]) + u[2] * T[0][2]
            q[0] += wu[0] * u[0]
            q[1] += wu[0] * u[1]
            q[2] += wu[0] * u[2]
            q[3] += wu[1] * u[1]
            q[4] += wu[1] * u[2]
            q[5] += wu[2] * u[2]
            q[6] += wu[0] * d
            q[7] += wu[1] * d
            q[8] += wu[2] * d
        quad[v] = q
    return quad


def place(m, cl, cells, placement):
    """The per-cluster pass: dict(vertices64 (nc, 3), vertices fp32, rgb fp32 or None, size, rank, placed, h (nc,), margins eig / box)."""
    nc = len(cl["members"])
    quad = vertex_quadrics(m, cl["vertex_cluster"] >= 0) if placement == QUADRIC else None
    out64, rgb = np.zeros((nc, 3)), (None if m.rgb is None else np.zeros((nc, 3), dtype=np.float32))
    size, rank, placed, hs = np.zeros(nc, dtype=np.int32), np.zeros(nc, dtype=np.int32), np.zeros(nc, dtype=np.int32), np.zeros(nc)
    eig_margin, box_margin = np.full(nc, INF), np.full(nc, INF)
    for c, mem in enumerate(cl["members"]):
        sx, sc, q = [0.0] * 3, [0.0] * 3, [0.0] * 9
        for v in mem:
            for a in range(3):
                sx[a] += float(m.vertices[v, a])
                if m.rgb is not None:
                    sc[a] += float(m.rgb[v, a])
            if placement == QUADRIC:
                for j in range(9):
                    q[j] += float(quad[v, j])
        cnt = float(len(mem))
        mean = [sx[a] / cnt for a in range(3)]
        G = cl["grid"][cl["scene"][mem[0]]]
        x, r, how = list(mean), 0, PLACED_MEAN
        if placement == QUADRIC:
            how = PLACED_FALLBACK
            b = [((q[0] * mean[0] + q[1] * mean[1]) + q[2] * mean[2]) - q[6], ((q[1] * mean[0] + q[3] * mean[1]) + q[4] * mean[2]) - q[7],
                 ((q[2] * mean[0] + q[4] * mean[1]) + q[5] * mean[2]) - q[8]]
            A, V = jacobi3([[q[0], q[1], q[2]], [q[1], q[3], q[4]], [q[2], q[4], q[5]]])
            lam = [A[0][0], A[1][1], A[2][2]]
            top = lam[0] if lam[0] > lam[1] else lam[1]
            top = top if top > lam[2] else lam[2]
            y = list(mean)
            if top > 0.0 and math.isfinite(top):
                for i in range(3):
                    eig_margin[c] = min(eig_margin[c], abs(lam[i] / top - RANK_RATIO) / RANK_RATIO)
                    if lam[i] > RANK_RATIO * top:
                        r += 1
                        t = ((V[0][i] * b[0] + V[1][i] * b[1]) + V[2][i] * b[2]) / lam[i]
                        for a in range(3):
                            y[a] = y[a] - t * V[a][i]
            if r > 0 and all(math.isfinite(t) for t in y):
                slack = G["h"] * (1.0 / float(BOX_SLACK_DIV))
                least = INF
                for a in range(3):
                    ia = int(cl["cell"][mem[0], a])
                    lo = (G["lo"][a] + float(ia) * G["h"]) - slack
                    hi = (G["lo"][a] + float(ia + 1) * G["h"]) + slack
                    least = min(least, y[a] - lo, hi - y[a])
                inside = least >= 0.0
                box_margin[c] = abs(least) / G["h"] if G["h"] > 0.0 else INF
                if inside:
                    x, how = y, PLACED_QUADRIC
        out64[c] = x
        if rgb is not None:
            rgb[c] = [np.float32(sc[a] / cnt) for a in range(3)]
        size[c], rank[c], placed[c], hs[c] = len(mem), r, how, G["h"]
    return dict(vertices64=out64, vertices=out64.astype(np.float32), rgb=rgb, size=size, rank=rank, placed=placed, h=hs,
                margins=dict(eig=float(eig_margin.min()) if nc else INF, box=float(box_margin.min()) if nc else INF),
                eig_margin=eig_margin, box_margin=box_margin)


def map_faces(m, vc):
    """(mapped_faces (nf, 3) int32, keep (nf,) uint8, keep after the dedupe (nf,) uint8)."""
    cls, _ = M.classify(m)
    nf = len(m.faces)
    mapped = np.full((nf, 3), -1, dtype=np.int32)
    ok = cls != M.INVALID
    mapped[ok] = vc[m.faces[ok]]
    keep = (cls == M.REGULAR) & (mapped >= 0).all(1) & (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 0] != mapped[:, 2])
    seen, keep2 = set(), keep.copy()
    for f in np.nonzero(keep)[0]:                                   # ascending rows: the lowest row of a set survives
        key = tuple(sorted(int(t) for t in mapped[f]))
        if key in seen:
            keep2[f] = False
        seen.add(key)
    return mapped, keep.astype(np.uint8), keep2.astype(np.uint8)


def simplify(m, cells, placement=QUADRIC):
    """Everything: the dicts of `clusters`, `place` and `map_faces` merged, the final mesh `out` (a meshtopo_f64.Mesh; `out64` its float64
    vertices, `out_h` the cell side per final vertex), vertex_index / face_index of the filter, final_vertex_cluster (nv,), final size /
    rank / placed, and margins (eig, box, cell, grid)."""
    cl = clusters(m, cells)
    pl = place(m, cl, cells, placement)
    mapped, keep, keep2 = map_faces(m, cl["vertex_cluster"])
    coarse = M.Mesh(pl["vertices"], mapped, cl["cluster_start"].astype(np.int64), m.face_start, pl["rgb"])
    out, vi, fi = M.filter_faces(coarse, keep2)
    nc = len(cl["members"])
    new_id = np.full(nc + 1, -1, dtype=np.int32)
    new_id[vi] = np.arange(len(vi), dtype=np.int32)
    vc = cl["vertex_cluster"]
    res = dict(cl)
    res.update({k: v for k, v in pl.items() if k != "margins"})
    res.update(mapped_faces=mapped, keep=keep, keep_deduped=keep2, out=out, out64=pl["vertices64"][vi], out_h=pl["h"][vi], vertex_index=vi,
               face_index=fi, final_vertex_cluster=new_id[np.where(vc >= 0, vc, nc)], final_size=pl["size"][vi], final_rank=pl["rank"][vi],
               final_placed=pl["placed"][vi], margins=dict(cl["margins"], **pl["margins"]))
    return res


# ------------------------------------------------------------------------------------------------ meshes for the tests
def subdivided_cube(n=4):
    """The unit cube, every side an n x n quad grid wound outward and cut along one diagonal: 6 n^2 + 2 vertices in (z, y, x) order,
    12 n^2 faces."""
    ids, quads = {}, []
    for axis in range(3):
        ua, va = (axis + 1) % 3, (axis + 2) % 3                     # e_u x e_v = e_axis
        for side in (0, 1):
            for j in range(n):
                for i in range(n):
                    corner = []
                    for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[ua], p[va] = side * n, i + du, j + dv
                        corner.append(tuple(p))
                    quads.append(corner if side else corner[::-1])
    points = sorted({p for qd in quads for p in qd}, key=lambda p: (p[2], p[1], p[0]))
    ids = {p: k for k, p in enumerate(points)}
    faces = M._quads([tuple(ids[p] for p in qd) for qd in quads])
    return M.make(np.array(points, dtype=np.float64) / n, faces)


def flat_grid(n=12, seed=0, z=0.25):
    """An n x n quad grid in the plane z = const with jittered interior positions."""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    jitter = 0.3 / n * (rng.random((2,) + i.shape) - 0.5)
    v = np.stack([i / n + jitter[0], j / n + jitter[1], np.full(i.shape, z)], axis=-1).reshape(-1, 3)
    at = lambda jj, ii: jj * (n + 1) + ii
    return M.make(v, M._quads([(at(jj, ii), at(jj, ii + 1), at(jj + 1, ii + 1), at(jj + 1, ii)) for jj in range(n) for ii in range(n)]))


def two_sheets(n=12, seed=0, gap=0.01):
    """flat_grid and a copy `gap` above it, wound the other way: a plate thinner than a cell of any grid of up to 1 / gap cells."""
    a = flat_grid(n, seed)
    top = a.vertices.copy()
    top[:, 2] += np.float32(gap)
    nv = len(a.vertices)
    return M.make(np.concatenate([a.vertices, top]), np.concatenate([a.faces, a.faces[:, ::-1] + np.int32(nv)]))


def uv_sphere(radius=0.45, rings=32, segments=64):
    """A closed UV sphere: rings x segments subdivisions, poles as single vertices, wound outward."""
    v = [(0.0, 0.0, radius)]
    for r in range(1, rings):
        t = math.pi * r / rings
        for s in range(segments):
            p = 2.0 * math.pi * s / segments
            v.append((radius * math.sin(t) * math.cos(p), radius * math.sin(t) * math.sin(p), radius * math.cos(t)))
    v.append((0.0, 0.0, -radius))
    at = lambda r, s: 1 + (r - 1) * segments + s % segments
    f = [(0, at(1, s), at(1, s + 1)) for s in range(segments)]
    for r in range(1, rings - 1):
        for s in range(segments):
            f += [(at(r, s), at(r + 1, s), at(r + 1, s + 1)), (at(r, s), at(r + 1, s + 1), at(r, s + 1))]
    last = len(v) - 1
    f += [(last, at(rings - 1, s + 1), at(rings - 1, s)) for s in range(segments)]
    return M.make(v, f)


def with_bad_vertices(m, seed=0):
    """A copy of a one-scene mesh with one NaN and one inf vertex (both used by faces) and one extra vertex that no face uses."""
    rng = np.random.default_rng(seed)
    v = np.concatenate([m.vertices, [[0.5, 0.5, 0.5]]]).astype(np.float32)
    used = np.unique(m.faces)
    a, b = rng.choice(used, 2, replace=False)
    v[a, 1], v[b, 0] = np.nan, np.inf
    rgb = None if m.rgb is None else np.concatenate([m.rgb, [[0.1, 0.2, 0.3]]]).astype(np.float32)
    return M.make(v, m.faces, rgb=rgb), int(a), int(b)


# ------------------------------------------------------------------------------------------------ the fixtures of the GPU comparison
GPU_CASES = {"tetrahedron": (1, 4), "empty": (4,), "hole": (2,), "mixed": (2, 4), "cube": (2,), "strip_permuted": (2, 1, 64), "grid": (64, 8),
             "fan": (4,), "sheets": (4,), "bad": (4,)}


def gpu_case(name):
    """The mesh of a GPU_CASES entry.  tests/test_cpu_simplify.py asserts that every margin of every (case, cells, placement) exceeds
    1e-6; a case that fails that is given another seed, never left out."""
    rng = np.random.default_rng(77)
    if name == "tetrahedron":
        return M.with_rgb(M.tetrahedron())
    if name == "empty":
        return M.make(np.zeros((0, 3)), np.zeros((0, 3)))
    if name == "hole":
        return M.with_rgb(M.concat([M.tetrahedron(), M.make(np.ones((2, 3)), np.zeros((0, 3))), M.cube(1)]), 1)
    if name == "mixed":
        return M.mixed_batch()
    if name == "cube":
        return M.with_rgb(subdivided_cube(), 6)
    if name == "strip_permuted":
        return M.with_rgb(M.permuted(M.strip(4097, seed=1), rng.permutation(4099)), 2)
    if name == "grid":
        g = M.quad_grid(64, seed=6)
        return M.with_rgb(M.permuted(g, rng.permutation(len(g.vertices))), 5)
    if name == "fan":
        return M.with_rgb(M.fan(300, seed=2), 4)
    if name == "sheets":
        return two_sheets()
    if name == "bad":
        return with_bad_vertices(M.with_rgb(M.quad_grid(8, seed=3), 7), seed=1)[0]
    raise KeyError(name)
