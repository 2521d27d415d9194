"""Test infrastructure of the point-to-mesh entries (include/mvd_hip.h: mvd_nearest_on_mesh, mvd_mesh_icp): the case table and two
oracles.  Importable without a GPU.

(a) THE RULE RESTATED in numpy float64, operation for operation in the header's order (`closest`, `unit_normal`), searched by brute force
    with the (d2, row) order (`search`).  numpy's float64 + - * / round once each, as the library's do (it is compiled without
    contraction), so this oracle is held to EQUAL bits: face, region, dist2.
(b) AN INDEPENDENT ONE in exact rational arithmetic (`exact_d2`, fractions.Fraction on the fp32 inputs): the plane projection when it
    falls inside the triangle, otherwise the best of the three clamped segment projections -- another decomposition than the Voronoi
    regions of (a), and no rounding at all.  It costs milliseconds per pair, so it runs on a subset (`exact_pairs`): for each sampled
    query the faces whose float64 d2 lies within 2^-20 relative of the float64 minimum (every face that can be the exact minimiser: the
    float64 rule is accurate to far better than 2^-25 on these cases, see below; test_cpu_meshdist.py prints what it measures) and
    eight faces drawn at random; on the small cases every pair.

Bounds, none taken from what the code under test gives:
  dist2 against (b)   |fl32(d2) - fl32(d2_exact)| <= 1 ulp of fp32 at fl32(d2_exact), on cases 1 - 4 and 6.  Why one ulp suffices: the
                      float64 rule forms the barycentrics from dot products of differences of fp32 values; their relative error is a few
                      2^-53 times the conditioning of the region's quotient, which is bounded by (longest edge / smallest altitude)^2 of
                      the face (`aspect2`).  The closest point c then carries an absolute error <= ~8 * 2^-53 * aspect2 * scale
                      (scale: the largest coordinate magnitude or edge) and d2 = |p - c|^2 an absolute error <= 2 d * that + its square.
                      For this to stay below half an fp32 ulp of d2 (2^-25 d2) the distance must satisfy d >= 2^-24 * aspect2 * scale
                      roughly (2^4 * 2^-53 * aspect2 * scale / 2^-25); a query nearer than that to the surface must have an EXACT float64
                      evaluation instead.  `conditioning_ok` asserts this per sampled pair from the face's smallest altitude: every
                      sampled pair either has d_exact >= 2^-24 * aspect2 * scale, or an exact distance of 0 (then the one-ulp window
                      is the smallest subnormal and demands an exact 0), or lies on cases 1 and 2, whose coordinates are small dyadic
                      numbers and whose on-surface queries have dyadic barycentrics, so that the float64 rule is exact there.  A
                      GENERIC point on a face does not get 0 from the rule but a d2 of the order (2^-50 * scale)^2 -- the closest point
                      is formed from rounded barycentrics -- which is why the cases' on-surface queries are the dyadic ones.
                      The second rounding (float64 -> fp32 of an already rounded value) is what widens "equal" to one ulp.
  face against (b)    the chosen face has an exact d2 within that same one-ulp-of-fp32 window of the exact minimum (compared after
                      rounding both to fp32): no query of the subset is excused.
  case 5 (slivers)    the same bound, derived from its geometry: its candidate faces are either near-equilateral (aspect2 <= ~3) or
                      EXACTLY collinear / coincident (dyadic coordinates, float64 normal exactly 0), which the rule searches as three
                      segments; a segment projection is one quotient of conditioning 1, so an exactly degenerate face counts with
                      aspect2 = 1 in `conditioning_ok`.  No face lies between the two (test_cpu_meshdist.py asserts it).
  point, bary, normal one fp32 rounding of a float64 value: 2^-24 relative per component (plus nothing: (a) and the library form the same
                      float64 value).  The bar the GPU test reports is equal bits.
  mesh ICP            pairs and rank equal on every row; |M_gpu - M_oracle| <= 1 / 16 of the oracle's own |M - truth| (the faceting of
                      the ~2 000-face target against the analytic surface the source lies on), as tests/test_gpu_plane.py derives its
                      sliding bound from the method's own error.
"""
import functools
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np
import torch

import align_f64 as A
import knn_f64 as K
import plane_f64 as P

INF = float("inf")
SPAN = 3                          # MVD_MESH_SPAN (tests/test_cpu_meshdist.py holds it to the header)
REGION_NAMES = ("A", "B", "C", "AB", "BC", "CA", "interior")


@dataclass
class Case:
    """The arguments of one mvd_nearest_on_mesh call as CPU numpy data."""
    query: np.ndarray                 # (nq, 3) fp32
    query_start: np.ndarray           # (nscene + 1,) int32
    vertices: np.ndarray              # (nv, 3) fp32
    faces: np.ndarray                 # (nf, 3) int32, global rows of vertices
    face_start: np.ndarray            # (nscene + 1,) int32
    region: np.ndarray = None         # (nq,) the region the construction puts each query in, -2 where it says nothing
    dyadic: bool = False              # small dyadic coordinates, and dyadic barycentrics where a query lies ON the mesh: the rule is exact there

    @property
    def nq(self):
        return int(self.query.shape[0])

    @property
    def nv(self):
        return int(self.vertices.shape[0])

    @property
    def nf(self):
        return int(self.faces.shape[0])

    @property
    def nscene(self):
        return int(self.face_start.shape[0]) - 1


def _case(query, vertices, faces, query_start=None, face_start=None, **kw):
    query = np.ascontiguousarray(np.asarray(query, dtype=np.float32).reshape(-1, 3))
    vertices = np.ascontiguousarray(np.asarray(vertices, dtype=np.float32).reshape(-1, 3))
    faces = np.ascontiguousarray(np.asarray(faces, dtype=np.int32).reshape(-1, 3))
    qs = np.asarray([0, len(query)] if query_start is None else query_start, dtype=np.int32)
    fs = np.asarray([0, len(faces)] if face_start is None else face_start, dtype=np.int32)
    return Case(query=query, query_start=qs, vertices=vertices, faces=faces, face_start=fs, **kw)


# ------------------------------------------------------------------------------------------------ (a) the rule restated
def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _sub(u, v):
    return [u[0] - v[0], u[1] - v[1], u[2] - v[2]]


def _finish(p, V, b):
    c = [(b[0] * V[0][k] + b[1] * V[1][k]) + b[2] * V[2][k] for k in range(3)]
    d = _sub(p, c)
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], c


def _safe(den):
    return np.where(den == 0.0, 1.0, den)


def _segments(p, V, shape):
    """The DEGENERATE rule: (b0, b1, b2, region) of the best of A -> B, B -> C, C -> A, a later one only when strictly nearer."""
    best = None
    for e in range(3):
        s, f = e, (e + 1) % 3
        se, sp = _sub(V[f], V[s]), _sub(p, V[s])
        len2 = _dot(se, se)
        t = np.where(len2 != 0.0, _dot(sp, se) / _safe(len2), 0.0)
        t = np.where(t > 0.0, t, 0.0)
        t = np.where(t > 1.0, 1.0, t)
        b = [np.zeros(shape), np.zeros(shape), np.zeros(shape)]
        b[s], b[f] = 1.0 - t, t + np.zeros(shape)
        region = np.where(t == 0.0, s, np.where(t == 1.0, f, 3 + e)) + np.zeros(shape, dtype=np.int64)
        d2, _ = _finish(p, V, b)
        if best is None:
            best = (b, region, d2)
        else:
            take = d2 < best[2]
            best = ([np.where(take, b[k], best[0][k]) for k in range(3)], np.where(take, region, best[1]), np.where(take, d2, best[2]))
    return best[0], best[1]


def closest(p, T):
    """THE per-pair rule.  p (..., 3) and T (..., 9) float64, broadcastable -> (d2, b (..., 3), c (..., 3), region)."""
    p, T = np.asarray(p, dtype=np.float64), np.asarray(T, dtype=np.float64)
    shape = np.broadcast_shapes(p.shape[:-1], T.shape[:-1])
    pv = [p[..., k] for k in range(3)]
    V = [[T[..., 3 * v + k] for k in range(3)] for v in range(3)]
    with np.errstate(all="ignore"):
        ab, ac = _sub(V[1], V[0]), _sub(V[2], V[0])
        nx, ny, nz = ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]
        flat = (nx == 0.0) & (ny == 0.0) & (nz == 0.0)
        ap = _sub(pv, V[0])
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = _sub(pv, V[1])
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = _sub(pv, V[2])
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va, e43, e56 = d3 * d6 - d5 * d4, d4 - d3, d5 - d6
        den = (va + vb) + vc
        v_ab = np.where((d1 - d3) == 0.0, 0.0, d1 / _safe(d1 - d3))
        w_ca = np.where((d2 - d6) == 0.0, 0.0, d2 / _safe(d2 - d6))
        w_bc = np.where((e43 + e56) == 0.0, 0.0, e43 / _safe(e43 + e56))
        v_in, w_in = vb / _safe(den), vc / _safe(den)
        conds = [(d1 <= 0.0) & (d2 <= 0.0), (d3 >= 0.0) & (d4 <= d3), (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), (d6 >= 0.0) & (d5 <= d6),
                 (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), (va <= 0.0) & (e43 >= 0.0) & (e56 >= 0.0), den != 0.0]
        one, zero = np.ones(shape), np.zeros(shape)
        bs = [(one, zero, zero), (zero, one, zero), (1.0 - v_ab, v_ab, zero), (zero, zero, one), (1.0 - w_ca, zero, w_ca),
              (zero, 1.0 - w_bc, w_bc), ((1.0 - v_in) - w_in, v_in, w_in)]
        codes = [0, 1, 3, 2, 5, 4, 6]
        seg_b, seg_region = _segments(pv, V, shape)
        conds = [flat] + [c & ~flat for c in conds]
        b = [np.select(conds, [seg_b[k]] + [x[k] for x in bs], default=seg_b[k]) for k in range(3)]
        region = np.select(conds, [seg_region] + [np.full(shape, c) for c in codes], default=seg_region)
        dist2, c = _finish(pv, V, b)
    return dist2, np.stack(np.broadcast_arrays(*b), axis=-1), np.stack(np.broadcast_arrays(*c), axis=-1), region.astype(np.int64)


def unit_normal(T):
    """THE normal of the header: (B - A) x (C - A) / its length in float64, 0 without one.  T (..., 9) float64."""
    T = np.asarray(T, dtype=np.float64)
    V = [[T[..., 3 * v + k] for k in range(3)] for v in range(3)]
    with np.errstate(all="ignore"):
        ab, ac = _sub(V[1], V[0]), _sub(V[2], V[0])
        n = [ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]]
        length = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        ok = (length > 0.0) & (length < INF)
        return np.stack([np.where(ok, n[k] / np.where(ok, length, 1.0), 0.0) for k in range(3)], axis=-1)


def candidates(case):
    """(nf,) bool: ids in [0, nv) and nine finite coordinates; and (nf, 9) float64 coordinates (0 where not a candidate)."""
    f = case.faces.astype(np.int64)
    ok = ((f >= 0) & (f < case.nv)).all(1)
    tri = case.vertices[np.clip(f, 0, max(case.nv - 1, 0))].reshape(-1, 9) if case.nv else np.zeros((case.nf, 9), dtype=np.float32)
    ok = ok & np.isfinite(tri).all(1)
    return ok, np.where(ok[:, None], tri, 0.0).astype(np.float64)


def scene_ranges(start, n):
    s = np.clip(np.asarray(start, dtype=np.int64), 0, n)
    return [(int(s[k]), int(s[k + 1])) for k in range(len(s) - 1)]


@dataclass
class Found:
    face: np.ndarray                  # (nq,) int32
    dist2: np.ndarray                 # (nq,) fp32
    point: np.ndarray                 # (nq, 3) fp32
    bary: np.ndarray                  # (nq, 3) fp32
    region: np.ndarray                # (nq,) int32
    normal: np.ndarray                # (nq, 3) fp32
    d2: np.ndarray                    # (nq,) float64: before the rounding


def search(case, chunk=256):
    """Brute force of the rule: per query the minimum of (d2 in float64, face row) over the candidates of its scene."""
    nq = case.nq
    ok, tri = candidates(case)
    out = Found(face=np.full(nq, -1, np.int32), dist2=np.full(nq, INF, np.float32), point=np.full((nq, 3), np.nan, np.float32),
                bary=np.zeros((nq, 3), np.float32), region=np.full(nq, -1, np.int32), normal=np.zeros((nq, 3), np.float32), d2=np.full(nq, INF))
    normals = unit_normal(tri)
    for (q0, q1), (f0, f1) in zip(scene_ranges(case.query_start, nq), scene_ranges(case.face_start, case.nf)):
        rows = np.arange(f0, f1)[ok[f0:f1]]
        if q1 <= q0 or rows.size == 0:
            continue
        for base in range(q0, q1, chunk):
            q = case.query[base:min(base + chunk, q1)].astype(np.float64)
            fin = np.isfinite(q).all(1)
            d2, b, c, region = closest(np.where(fin[:, None], q, 0.0)[:, None, :], tri[rows][None, :, :])
            best = np.argmin(d2, axis=1)                          # (the first minimum: the lowest row)
            i = np.arange(len(q))
            win = fin & (d2[i, best] < INF)
            at = base + i[win]
            out.face[at], out.d2[at] = rows[best[win]], d2[i[win], best[win]]
            with np.errstate(over="ignore"):
                out.dist2[at] = d2[i[win], best[win]].astype(np.float32)
            out.point[at], out.bary[at] = c[i[win], best[win]].astype(np.float32), b[i[win], best[win]].astype(np.float32)
            out.region[at], out.normal[at] = region[i[win], best[win]], normals[rows[best[win]]].astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------ (b) exact rational arithmetic
def _fr(v):
    return [Fraction(float(x)) for x in v]


def _fdot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def _fcross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def _fsegment(p, s, e):
    se, sp = _sub(e, s), _sub(p, s)
    len2 = _fdot(se, se)
    t = Fraction(0) if len2 == 0 else min(max(_fdot(sp, se) / len2, Fraction(0)), Fraction(1))
    d = [sp[k] - t * se[k] for k in range(3)]
    return _fdot(d, d)


def exact_d2(p, tri):
    """The exact squared distance of the fp32 point p (3,) to the fp32 triangle tri (9,), a Fraction."""
    p, a, b, c = _fr(p), _fr(tri[0:3]), _fr(tri[3:6]), _fr(tri[6:9])
    n = _fcross(_sub(b, a), _sub(c, a))
    nn = _fdot(n, n)
    if nn != 0:
        t = _fdot(_sub(p, a), n) / nn
        foot = [p[k] - t * n[k] for k in range(3)]
        inside = all(_fdot(_fcross(_sub(u, foot), _sub(v, foot)), n) >= 0 for u, v in ((a, b), (b, c), (c, a)))
        if inside:
            return t * t * nn
    return min(_fsegment(p, a, b), _fsegment(p, b, c), _fsegment(p, c, a))


def fl32(x):
    """A Fraction (or float) rounded once to fp32, as a float (+inf beyond the range)."""
    if isinstance(x, Fraction):
        # round-to-nearest-even of an exact rational: through the integer quotient at 24 significant bits
        if x == 0:
            return 0.0
        e = x.numerator.bit_length() - x.denominator.bit_length()
        if Fraction(2) ** e > x:
            e -= 1
        e = max(e, -126)
        unit = Fraction(2) ** (e - 23)
        q = x / unit
        k = q.numerator // q.denominator
        rem = q - k
        if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and k % 2 == 1):
            k += 1
        v = float(k * unit)
        return v if v < 2.0 ** 128 else INF
    with np.errstate(over="ignore"):
        return float(np.float32(x))


def ulp32(v):
    v = np.float32(abs(v))
    return float(np.nextafter(v, np.float32(INF)) - v)


def within_one_ulp(got, want):
    """|got - want| <= 1 ulp of fp32 at `want` (both floats that are fp32 values)."""
    if want == INF or got == INF:
        return got == want
    return abs(got - want) <= ulp32(want)


def exact_pairs(name, queries=24, extra=8, seed=5):
    """The subset (b) runs on: {query row: [face rows]} -- per sampled query (every query where the scene has at most 1 000 pairs) the
    faces within 2^-20 relative of the float64 minimum and `extra` random candidates of its scene (every face of a scene of at most 16)."""
    case = make_case(name)
    ok, tri = candidates(case)
    rng = np.random.default_rng(seed)
    pairs = {}
    for (q0, q1), (f0, f1) in zip(scene_ranges(case.query_start, case.nq), scene_ranges(case.face_start, case.nf)):
        rows = np.arange(f0, f1)[ok[f0:f1]]
        live = [i for i in range(q0, q1) if np.isfinite(case.query[i]).all()]
        if not live or rows.size == 0:
            continue
        chosen = live if len(live) * rows.size <= 1000 else sorted(rng.choice(live, size=min(queries, len(live)), replace=False).tolist())
        for i in chosen:
            if rows.size <= 16:
                pairs[i] = rows.tolist()
                continue
            d2 = closest(case.query[i].astype(np.float64)[None, :], tri[rows])[0]
            near = rows[d2 <= d2.min() * (1.0 + 2.0 ** -20) + 1e-300]
            pairs[i] = sorted(set(near.tolist()) | set(rng.choice(rows, size=min(extra, rows.size), replace=False).tolist()))
    return pairs


@functools.lru_cache(maxsize=None)
def exact_minima(name):
    """{query row: (fl32 of the exact minimum over the subset's faces, {face row: fl32 of its exact d2})} for the rows of exact_pairs."""
    case = make_case(name)
    _, tri = candidates(case)
    out = {}
    for i, rows in exact_pairs(name).items():
        exact = {f: exact_d2(case.query[i], tri[f].astype(np.float32)) for f in rows}
        out[i] = (fl32(min(exact.values())), {f: fl32(v) for f, v in exact.items()})
    return out


def aspect2(tri):
    """(longest edge / smallest altitude)^2 of float64 triangles (m, 9); inf for a face without area."""
    a, b, c = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
    area2 = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    longest = np.max([np.linalg.norm(b - a, axis=1), np.linalg.norm(c - b, axis=1), np.linalg.norm(a - c, axis=1)], axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(area2 > 0, (longest * longest / area2) ** 2, INF)


# ------------------------------------------------------------------------------------------------ cases
def icosphere(levels, radius=0.5):
    """A closed sphere mesh: the icosahedron subdivided `levels` times (20 * 4^levels faces), outward winding."""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(levels):
        mid, nf = {}, []

        def middle(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, dtype=np.int32)


def _case_one_triangle(seed):
    """One triangle in the plane z = 1/8 with dyadic coordinates; queries built INTO each of the seven regions on both sides of the plane,
    on each vertex, on each edge, in the plane inside and outside, and far away."""
    V = np.array([[-0.5, -0.25, 0.125], [1.0, 0.0, 0.125], [0.25, 1.5, 0.125]])
    cen, other = 0.5 * V[0] + 0.25 * V[1] + 0.25 * V[2], 0.25 * V[0] + 0.25 * V[1] + 0.5 * V[2]      # dyadic barycentrics: exact in the plane
    q, region = [], []
    for z in (0.0, 0.375, -0.25):
        for k in range(3):
            q.append(V[k] + 0.5 * (V[k] - cen) + [0, 0, z]), region.append(k)                     # beyond a vertex
            a, b = V[k], V[(k + 1) % 3]
            edge = b - a
            out = np.array([edge[1], -edge[0], 0.0])                                              # in-plane, away from the third vertex
            q.append((a + b) / 2 + 0.25 * out + [0, 0, z]), region.append(3 + k)
        q.append(cen + [0, 0, z]), region.append(6)
        q.append(other + [0, 0, z]), region.append(6)
    for k in range(3):
        q.append(V[k]), region.append(-2)                                                         # on a vertex: a boundary, any code
        q.append((V[k] + V[(k + 1) % 3]) / 2), region.append(-2)                                  # on an edge
    for s in (1.0, -1.0):
        for k in range(3):
            far = np.zeros(3)
            far[k] = s * 1e6
            q.append(far), region.append(-2)
    q.append([1e6, 1e6, -1e6]), region.append(-2)
    return _case(q, V, [[0, 1, 2]], region=np.array(region), dyadic=True)


def _pair_queries():
    return [[0.5, 0.5, 0.25], [0.5, 0.5, -1.0], [0.25, 0.75, 0.5], [0.75, 0.25, 0.0], [0.25, 0.25, 0.5], [0.75, 0.75, 0.5], [2.0, 2.0, 0.0],
            [-1.0, 2.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 2.0], [0.5, 0.5, 0.0]]


def _case_tie_pair(seed, swapped=False):
    """Two faces sharing the edge (1, 0, 0) - (0, 1, 0); queries above and on that edge are equally far from both: the lowest row wins."""
    V = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]]
    F = [[0, 1, 2], [1, 3, 2]]
    return _case(_pair_queries(), V, F[::-1] if swapped else F, dyadic=True)


def _case_tetrahedron(seed):
    V = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64) * 0.5
    F = [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]
    q = [[0, 0, 0]] + V.tolist() + [((V[i] + V[j]) / 2).tolist() for i in range(4) for j in range(i + 1, 4)] + (V * 2).tolist() + \
        [(V[[a, b, c]].sum(0) / 4).tolist() for a, b, c in F] + [[0.125, 0.0625, -0.25], [3.0, 0.0, 0.0]]
    return _case(q, V, F, dyadic=True)


def _case_cube(seed):
    """The cube [-1/2, 1/2]^3 as 12 faces; queries at its centre, face centres, edge midpoints and corners, and pushed outward."""
    V = np.array([[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)])
    F = [[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]]
    lattice = np.array([[x, y, z] for z in (-0.5, 0, 0.5) for y in (-0.5, 0, 0.5) for x in (-0.5, 0, 0.5)])      # centre, faces, edges, corners
    q = np.concatenate([lattice, lattice * 1.5, lattice * 0.5, [[0.125, 0.25, 0.375], [0.0, 0.0, 0.4375]]])
    return _case(q, V, F, dyadic=True)


def _case_sphere(seed):
    """A closed sphere of 1 280 faces against 3 001 points of a noisy sphere (inside and outside, all three region kinds)."""
    V, F = icosphere(3)
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((3001, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return _case(d * 0.5 * (1.0 + 0.08 * rng.standard_normal((3001, 1))), V, F)


def _small_triangles(rng, n, half, size):
    """3 n vertices: n nearly equilateral triangles of circumradius `size` (corners jittered by a fifth of it) in random planes."""
    centre = rng.uniform(-half, half, (n, 1, 3))
    frame = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    angle = rng.uniform(0, 2 * math.pi, (n, 1)) + np.array([0.0, 2.0, 4.0]) * math.pi / 3
    corners = np.cos(angle)[:, :, None] * frame[:, None, :, 0] + np.sin(angle)[:, :, None] * frame[:, None, :, 1]
    return (centre + size * (corners + rng.uniform(-0.2, 0.2, (n, 3, 3)))).reshape(-1, 3)


def _case_mixed(seed):
    """Two triangles spanning the whole box (the oversize path at any grid) and 2 000 small ones (the walk)."""
    rng = np.random.default_rng(seed)
    big = np.array([[-0.75, -0.75, -0.75], [0.75, -0.75, 0.75], [-0.75, 0.75, 0.75], [0.75, 0.75, -0.75], [-0.75, 0.75, -0.625], [0.75, -0.75, -0.75]])
    V = np.concatenate([big, _small_triangles(rng, 2000, 0.7, 0.02)])
    F = np.concatenate([[[0, 1, 2], [3, 4, 5]], 6 + np.arange(6000).reshape(-1, 3)])
    order = rng.permutation(len(F))                                   # the huge faces somewhere in the middle
    return _case(rng.uniform(-0.85, 0.85, (1501, 3)), V, F[order])


def _case_huge_only(seed):
    rng = np.random.default_rng(seed)
    V = rng.uniform(-0.75, 0.75, (15, 3))
    return _case(rng.uniform(-0.9, 0.9, (517, 3)), V, np.arange(15).reshape(5, 3))


def _case_odd(seed):
    """Collinear and coincident-vertex faces next to valid ones; ids of -1 and nv; a NaN and an inf vertex; NaN and inf queries; a second
    scene without any candidate face."""
    rng = np.random.default_rng(seed)
    V = np.concatenate([_small_triangles(rng, 40, 0.5, 0.1), [[0, 0, 0], [0.25, 0.25, 0.25], [0.5, 0.5, 0.5], [0.125, -0.25, 0.375]],
                        [[np.nan, 0, 0], [0.1, np.inf, 0.2], [0.3, 0.3, 0.3]]]).astype(np.float32)
    nv = len(V)
    good = np.arange(120).reshape(-1, 3)
    odd = [[120, 121, 122], [122, 120, 121], [120, 120, 122], [123, 123, 123], [121, 122, 122], [120, 122, 120],      # collinear / coincident
           [-1, 0, 1], [0, nv, 1], [2, 3, -7], [124, 0, 1], [0, 125, 2], [126, 124, 125], [nv + 5, nv, -1]]           # no candidates
    F = np.concatenate([good[:20], odd, good[20:], [[-1, 0, 1], [124, 125, 126], [0, 1, nv]]])
    n0 = len(F) - 3                                                   # scene 1: the last three faces, none a candidate
    q = rng.uniform(-0.7, 0.7, (400, 3)).astype(np.float32)
    q[:12] = [[0.25, 0.25, 0.25], [0.375, 0.375, 0.375], [1, 1, 1], [-1, -1, -1], [0.125, -0.25, 0.375], [0.3, 0.2, 0.4], [0, 0, 0], [0.5, 0.5, 0.5],
              [0.2, 0.3, 0.25], [0.25, 0.3, 0.2], [0.0625, 0.0625, 0.0625], [0.4, 0.45, 0.5]]
    q[20], q[21], q[22], q[23] = [np.nan, 0, 0], [0, np.inf, 0], [0.1, 0.1, -np.inf], [np.nan, np.nan, np.nan]
    q[390] = [np.nan, 0.5, 0.5]
    return _case(q, V, F, query_start=[0, 380, 400], face_start=[0, n0, len(F)])


def _case_scenes(seed):
    """Four scenes of 700 / 2 / 0 / 1 301 faces over one shared vertex array with global ids; the last 37 queries belong to no scene."""
    rng = np.random.default_rng(seed)
    lens = [700, 2, 0, 1301]
    centres = [(-0.3, 0.0, 0.1), (0.4, 0.4, -0.2), (0.0, 0.0, 0.0), (0.1, -0.2, 0.3)]
    V = np.concatenate([_small_triangles(rng, n, 0.4, 0.03) + np.array(c) for n, c in zip(lens, centres) if n])
    F = np.arange(3 * sum(lens)).reshape(-1, 3)
    V, F = V[::-1].copy(), (3 * sum(lens) - 1) - F                    # ids that do not run with the rows
    fs = np.concatenate([[0], np.cumsum(lens)])
    qn = [300, 50, 40, 500]
    q = np.concatenate([rng.uniform(-0.5, 0.5, (n, 3)) + np.array(c) for n, c in zip(qn, centres)] + [rng.uniform(-0.5, 0.5, (37, 3))])
    return _case(q, V, F, query_start=np.concatenate([[0], np.cumsum(qn)]), face_start=fs)


CASES = {
    "one_triangle": (_case_one_triangle, 0),
    "tie_pair": (_case_tie_pair, 1),
    "tie_pair_swapped": (lambda seed: _case_tie_pair(seed, swapped=True), 1),
    "tetrahedron": (_case_tetrahedron, 2),
    "cube": (_case_cube, 3),
    "sphere": (_case_sphere, 4),
    "mixed": (_case_mixed, 5),
    "huge_only": (_case_huge_only, 6),
    "odd": (_case_odd, 7),
    "scenes": (_case_scenes, 8),
}
GRIDS = (1, 7, 0)


@functools.lru_cache(maxsize=None)
def make_case(name):
    fn, seed = CASES[name]
    return fn(7300 + seed)


@functools.lru_cache(maxsize=None)
def refs(name):
    return search(make_case(name))


def scene_case(case, s):
    """Scene s of a batched case as a call of its own (the shared vertex array is kept: ids are global) and its first face row."""
    (q0, q1), (f0, f1) = scene_ranges(case.query_start, case.nq)[s], scene_ranges(case.face_start, case.nf)[s]
    return _case(case.query[q0:q1], case.vertices, case.faces[f0:f1]), f0, (q0, q1)


# ------------------------------------------------------------------------------------------------ mesh ICP
def ellipsoid_mesh(rings=32, segments=32):
    """A latitude-longitude triangulation of plane_f64's bumped ellipsoid, its vertices ON the analytic surface: 2 * segments *
    (rings - 1) = 1 984 faces, outward winding."""
    v0 = np.array([1.0, 1.0, 0.5]) / 1.5

    def surface(d):
        bump = 0.25 * np.exp(-((d - v0) ** 2).sum(-1) / (2 * 0.3 ** 2))
        return d * np.array(K.ELLIPSOID) * (1.0 + bump)[..., None]
    dirs = [[0.0, 0.0, 1.0]]
    for r in range(1, rings):
        th = math.pi * r / rings
        dirs += [[math.sin(th) * math.cos(2 * math.pi * s / segments), math.sin(th) * math.sin(2 * math.pi * s / segments), math.cos(th)]
                 for s in range(segments)]
    dirs.append([0.0, 0.0, -1.0])
    ring = lambda r, s: 1 + (r - 1) * segments + s % segments
    F = [[0, ring(1, s), ring(1, s + 1)] for s in range(segments)]
    for r in range(1, rings - 1):
        for s in range(segments):
            F += [[ring(r, s), ring(r + 1, s), ring(r + 1, s + 1)], [ring(r, s), ring(r + 1, s + 1), ring(r, s + 1)]]
    last = len(dirs) - 1
    F += [[ring(rings - 1, s + 1), ring(rings - 1, s), last] for s in range(segments)]
    return surface(np.array(dirs)).astype(np.float32), np.array(F, dtype=np.int32)


@dataclass
class IcpCase:
    source: torch.Tensor              # (n, 3) fp32
    vertices: np.ndarray
    faces: np.ndarray
    iters: int
    truth: np.ndarray


@functools.lru_cache(maxsize=None)
def icp_case():
    V, F = ellipsoid_mesh()
    on_surface = P.bumped_ellipsoid(1024, 7391)
    src = A.apply(np.linalg.inv(P.TRUTH_SLIDE)[:3][None], on_surface, [0, 1024])
    return IcpCase(source=src, vertices=V, faces=F, iters=12, truth=P.TRUTH_SLIDE)


@dataclass
class IcpRef:
    matrix: np.ndarray                # (4, 4) after iters steps
    history: np.ndarray               # (iters + 1, 4)
    found: Found                      # the last pass
    moved: torch.Tensor
    worst_clearance: float


def icp(case, iters=None, init=None):
    """The loop of the rule: apply, brute force (a), plane_f64's sums and solve on the pairs (moved, point, normal); one scene."""
    iters = case.iters if iters is None else iters
    n = int(case.source.shape[0])
    m = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    rows, clear = [], INF
    for k in range(iters + 1):
        moved = A.apply(m[:3][None], case.source, [0, n])
        found = search(_case(moved.numpy(), case.vertices, case.faces))
        pairs = P.Case(base=A.Case(source=moved, start=[0, n], target=torch.from_numpy(found.point), tstart=[0, n], scale=False),
                       normals=torch.from_numpy(found.normal))
        sums = P.plane_sums(moved, pairs, None, torch.from_numpy(found.dist2))[0]
        sol = P.solve(sums)
        rows.append(P.history_row(sums, sol.rank))
        clear = min(clear, P.clearance(sol.lam)) if sol.rank else clear
        if k < iters:
            m = P.step44(sol.R, sol.t) @ m
    return IcpRef(matrix=m, history=np.stack(rows), found=found, moved=moved, worst_clearance=clear)


@functools.lru_cache(maxsize=None)
def icp_ref():
    return icp(icp_case())


def cube_icp_case():
    """A cube target and a source on its face z = +1/2 only, lifted by 0.01 and tilted by one degree: the plane constrains three of the
    six directions (rank 3) and the in-plane ones must stay where they are."""
    cube = make_case("cube")
    g = np.random.default_rng(7399)
    flat = np.concatenate([g.uniform(-0.4, 0.4, (600, 2)), np.full((600, 1), 0.5)], axis=1).astype(np.float32)
    move = A.similarity(1.0, 1.0, (1, 0.5, 0), (0.0, 0.0, 0.01))
    src = A.apply(move[:3][None], torch.from_numpy(flat), [0, 600])
    return IcpCase(source=src, vertices=cube.vertices, faces=cube.faces, iters=4, truth=np.linalg.inv(move))


def conditioning_ok(case, i, f, d2_exact):
    """The premise of the one-ulp bound for the pair (query i, face f): the distance is at least 2^-24 * aspect2 * scale (the module
    docstring derives it), or the case is dyadic, where the float64 rule is exact on the mesh itself."""
    _, tri = candidates(case)
    scale = max(float(np.abs(tri[f]).max()), float(np.abs(case.query[i]).max()) if np.isfinite(case.query[i]).all() else 0.0)
    if d2_exact == 0:                 # (the one-ulp window at 0 is the smallest fp32 subnormal: the check itself demands an exact 0)
        return True
    shape = float(aspect2(tri[f:f + 1])[0])
    shape = 1.0 if shape == INF else shape          # an exactly degenerate face is three segments: a segment projection has conditioning 1
    return case.dyadic or math.sqrt(float(d2_exact)) >= 2.0 ** -24 * shape * scale


def dump_cases(directory, names=None):
    """Every case with the oracle's face, region and dist2 as the binary files tools/meshdist_host.hip reads (its head comment has the
    layout); the ICP target with its source as queries too."""
    import os
    os.makedirs(directory, exist_ok=True)
    cases = {name: make_case(name) for name in (names or CASES)}
    if names is None:
        icp = icp_case()
        cases["icp_ellipsoid"] = _case(icp.source.numpy(), icp.vertices, icp.faces)
    for name, case in cases.items():
        ref = search(case)
        with open(os.path.join(directory, name + ".bin"), "wb") as f:
            f.write(np.array([case.nq, case.nv, case.nf, case.nscene], dtype=np.int32).tobytes())
            for a in (case.query, case.query_start, case.face_start, case.vertices, case.faces, ref.face, ref.region, ref.dist2):
                f.write(np.ascontiguousarray(a).tobytes())
