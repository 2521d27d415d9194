"""Test infrastructure of the winding-number entries (include/mvd_hip.h: mvd_winding_number): the case table and two oracles.  Importable
without a GPU; not collected by pytest.

THE RULE, restated from the header.
  Candidate face: three ids in [0, nv), nine finite coordinates, and an fp64 normal n = (B - A) x (C - A) whose three components are not
    all exactly 0, each component one subtraction of two products (n_x = ab_y ac_z - ab_z ac_y, ...).  A face that is no candidate
    contributes nothing under either method.
  Per pair: fp64 on exact conversions of the fp32 inputs, no contraction.  dot(u, v) = (u_x v_x + u_y v_y) + u_z v_z.  With q the query:
    a = A - q, b = B - q, c = C - q; la = sqrt(dot(a, a)), lb, lc likewise; x = b x c; num = dot(a, x);
    den = (((la lb) lc + dot(a, b) lc) + dot(b, c) la) + dot(c, a) lb.  Omega = 0 when num == 0, else 2 atan2(num, den).
  EXACT: S = the sum of Omega over the scene's faces in ascending face row, started from 0.
  CELLS(cells, beta): per scene the box of the vertices of its candidate faces; h = longest extent / cells;
    n_k = clamp(floor(extent_k / h) + 1, 1, cells); a face belongs to the cell of its centroid g = ((A + B) + C) / 3 per axis, cell index
    clamp(floor((g_k - lo_k) / h), 0, n_k - 1), linear id (iz n_y + iy) n_x + ix; member lists ascend by face row.  Per occupied cell
    over its members ascending, m_f = sqrt(dot(n_f, n_f)): M = sum m_f, p = (sum m_f g_f) / M per axis, N = 0.5 * sum n_f per axis,
    rho2 = max over the members' three vertices X of dot(X - p, X - p).  Query: over the occupied cells in ascending cell id, d = p - q,
    r2 = dot(d, d); FAR iff r2 > (beta * beta) * rho2 (strictly); a far cell contributes dot(N, d) / (r2 * sqrt(r2)), a near cell the
    sum of Omega over its members ascending started from 0; S = the sum of the contributions in that order.
  Outputs: w = S / (4.0 * 3.141592653589793) in fp64; inside = w >= 0.5.  A query with a non-finite coordinate or of no scene: w = NaN,
    inside = 0.  A scene without a candidate face: w = 0.

(a) `winding` is that rule in numpy float64, operation for operation: every + - * /, floor and sqrt of numpy rounds once, as the library's
    do, and a sum "in order" is a loop of vector additions, never numpy.sum.  Omega of every (query, face) pair is formed once per case
    (`omega_matrix`); the two methods differ only in the order and grouping of the additions.
(b) `excess_mp` is an independent oracle in mpmath at 50 digits by another decomposition: the spherical excess A + B + C - pi of the
    triangle the three unit directions span, from its three dihedral angles, signed by the determinant.

Bounds, none taken from the code under test:
  CELLS with beta = 0      w EQUAL to (a) in bits: the path uses + - * /, floor and sqrt only.
  every other setting      |w - w_a| <= nf_s * 2^-48, nf_s the scene's candidate faces (`tolerance`): num and den are bit-equal on both
                           sides and only atan2's last bits differ, at most 3 ulp taking both sides together; |atan2| < 4 and the
                           doubling make one ulp at most 2^-50, so a term differs by <= 3 * 2^-50 < 2^-48; the rounding of a sum whose
                           terms differ by that much adds less; dividing by 4 pi only helps.
  inside                   compared on every query whose oracle |w - 0.5| exceeds that tolerance; the cases are built so that this
                           leaves out only the constructed queries ON the surface (`Case.on_surface` has their count).
  (a) against (b)          |w_a - w_b| <= nf * 2^-48 on queries at least 1e-3 of the scene's extent from the surface.
"""
import functools
import math
from dataclasses import dataclass

import numpy as np

AUTO, EXACT, CELLS = 0, 1, 2
MAX_CELLS, MAX_TABLE = 64, 2 ** 28
FACE_TILE, CELL_TILE = 512, 128          # MVD_WIND_FACE_TILE, MVD_WIND_CELL_TILE (tests/test_cpu_winding.py holds them to the header)
FOUR_PI = 4.0 * 3.141592653589793
INF = float("inf")
SETTINGS = [(EXACT, 0, 2.0)] + [(CELLS, c, b) for c in (1, 2, 7, 64) for b in (0.0, 2.0, INF)]


@dataclass
class Case:
    """The arguments of one mvd_winding_number call as CPU numpy data."""
    query: np.ndarray                 # (nq, 3) fp32
    query_start: np.ndarray           # (nscene + 1,) int32
    vertices: np.ndarray              # (nv, 3) fp32
    faces: np.ndarray                 # (nf, 3) int32, global rows of vertices
    face_start: np.ndarray            # (nscene + 1,) int32
    on_surface: int = 0               # the constructed queries whose winding number is 0.5 (on a face, or in the rim plane of an open shell)
    known: tuple = ()                 # (query row, winding number known by hand)

    nq = property(lambda self: int(self.query.shape[0]))
    nv = property(lambda self: int(self.vertices.shape[0]))
    nf = property(lambda self: int(self.faces.shape[0]))
    nscene = property(lambda self: int(self.face_start.shape[0]) - 1)


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


def _cross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def candidates(case):
    """(ok (nf,) bool, tri (nf, 9) float64 -- zeros where not ok --, normal (nf, 3) float64)."""
    f = case.faces.astype(np.int64)
    ids_ok = ((f >= 0) & (f < case.nv)).all(1) if case.nf else np.zeros(0, dtype=bool)
    tri = np.zeros((case.nf, 9))
    if case.nv:
        tri[ids_ok] = case.vertices[f[ids_ok]].astype(np.float64).reshape(-1, 9)
    finite = np.isfinite(tri).all(1)
    tri[~finite] = 0.0
    A, B, C = ([tri[:, 3 * j + k] for k in range(3)] for j in range(3))
    n = np.stack(_cross([B[k] - A[k] for k in range(3)], [C[k] - A[k] for k in range(3)]), axis=1) if case.nf else np.zeros((0, 3))
    ok = ids_ok & finite & ~((n == 0.0).all(1))
    tri[~ok] = 0.0
    return ok, tri, n


def omega(q, T):
    """Omega of the rule.  q (..., 3) and T (..., 9) float64, broadcastable."""
    q, T = np.asarray(q, dtype=np.float64), np.asarray(T, dtype=np.float64)
    a, b, c = ([T[..., 3 * j + k] - q[..., k] for k in range(3)] for j in range(3))
    la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
    num = _dot(a, _cross(b, c))
    den = (((la * lb) * lc + _dot(a, b) * lc) + _dot(b, c) * la) + _dot(c, a) * lb
    return np.where(num == 0.0, 0.0, 2.0 * np.arctan2(num, den))


def scene_of(start, n, nscene):
    """The scene of every row 0 .. n - 1 under the clamped start table, -1 for a row of no scene."""
    st = np.clip(start.astype(np.int64), 0, n)
    rows = np.arange(n)
    s = np.searchsorted(st, rows, side="right") - 1
    s = np.minimum(s, nscene - 1)
    inside = (s >= 0) & (rows >= st[np.maximum(s, 0)]) & (rows < st[np.maximum(s, 0) + 1])
    return np.where(inside, s, -1)


def omega_matrix(case):
    """(nq, nf) float64: Omega of every pair of a VALID query and a CANDIDATE face of its scene, 0 elsewhere; plus valid, q scene, ok."""
    ok, tri, _ = candidates(case)
    qs, fs = scene_of(case.query_start, case.nq, case.nscene), scene_of(case.face_start, case.nf, case.nscene)
    valid = (qs >= 0) & np.isfinite(case.query).all(1) if case.nq else np.zeros(0, dtype=bool)
    Om = np.zeros((case.nq, case.nf))
    q64 = case.query.astype(np.float64)
    for s in range(case.nscene):
        qi, fi = np.nonzero(valid & (qs == s))[0], np.nonzero(ok & (fs == s))[0]
        for lo in range(0, len(qi), 256):
            rows = qi[lo:lo + 256]
            if len(fi):
                with np.errstate(all="ignore"):
                    Om[np.ix_(rows, fi)] = omega(q64[rows][:, None, :], tri[fi][None, :, :])
    return Om, valid, qs, fs, ok


def scene_cells(case, s, cells, parts=None):
    """The occupied cells of scene s in ascending cell id: a list of dict(id, members (ascending face rows), p, N, rho2), in Python floats."""
    ok, tri, normal = parts if parts is not None else candidates(case)
    fs = scene_of(case.face_start, case.nf, case.nscene)
    mine = np.nonzero(ok & (fs == s))[0]
    if len(mine) == 0:
        return []
    pts = case.vertices[case.faces[mine].astype(np.int64)].reshape(-1, 3)
    lo32, hi32 = pts.min(0), pts.max(0)
    lo = [float(lo32[k]) for k in range(3)]
    ext = [float(hi32[k]) - lo[k] for k in range(3)]
    big = 0.0
    for k in range(3):
        big = ext[k] if ext[k] > big else big
    h = big / float(cells)
    n = [1, 1, 1]
    if h > 0.0:
        n = [int(min(max(math.floor(ext[k] / h) + 1.0, 1.0), float(cells))) for k in range(3)]
    lists = {}
    cent = {}
    for f in mine:
        T = [float(t) for t in tri[f]]
        g = [((T[k] + T[3 + k]) + T[6 + k]) / 3.0 for k in range(3)]
        idx = [0, 0, 0]
        if h > 0.0:
            idx = [int(min(max(math.floor((g[k] - lo[k]) / h), 0.0), float(n[k] - 1))) for k in range(3)]
        lists.setdefault((idx[2] * n[1] + idx[1]) * n[0] + idx[0], []).append(int(f))
        cent[int(f)] = g
    out = []
    for cid in sorted(lists):
        M, sg, sn = 0.0, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        for f in lists[cid]:
            nf_ = [float(t) for t in normal[f]]
            m = math.sqrt(_dot(nf_, nf_))
            M += m
            for k in range(3):
                sg[k] += m * cent[f][k]
                sn[k] += nf_[k]
        p, N = [sg[k] / M for k in range(3)], [0.5 * sn[k] for k in range(3)]
        rho2 = 0.0
        for f in lists[cid]:
            for j in range(3):
                d = [float(tri[f][3 * j + k]) - p[k] for k in range(3)]
                r = _dot(d, d)
                rho2 = r if r > rho2 else rho2
        out.append(dict(id=cid, members=lists[cid], p=p, N=N, rho2=rho2))
    return out


@dataclass
class Result:
    w: np.ndarray                     # (nq,) float64
    inside: np.ndarray                # (nq,) uint8
    occupied: int = 0                 # occupied cells over all scenes (CELLS)
    near_faces: float = 0.0           # mean faces evaluated per valid query (CELLS)


def winding(case, method=EXACT, cells=0, beta=2.0, parts=None):
    """THE rule -> Result.  `parts`: a cached omega_matrix(case)."""
    Om, valid, qs, fs, ok = parts if parts is not None else omega_matrix(case)
    S = np.zeros(case.nq)
    occupied, near_total = 0, 0
    cand = candidates(case) if method == CELLS else None
    q64 = case.query.astype(np.float64)
    bb = beta * beta
    for s in range(case.nscene):
        qi = np.nonzero(valid & (qs == s))[0]
        if method == EXACT:
            acc = np.zeros(len(qi))
            for f in np.nonzero(ok & (fs == s))[0]:
                acc = acc + Om[qi, f]
            S[qi] = acc
            continue
        acc = np.zeros(len(qi))
        for c in scene_cells(case, s, cells, cand):
            occupied += 1
            d = [c["p"][k] - q64[qi, k] for k in range(3)]
            r2 = _dot(d, d)
            with np.errstate(all="ignore"):
                far = r2 > bb * c["rho2"]
                dip = _dot(c["N"], d) / (r2 * np.sqrt(r2))
            near = np.nonzero(~far)[0]
            t = np.zeros(len(near))
            for f in c["members"]:
                t = t + Om[qi[near], f]
            near_total += len(near) * len(c["members"])
            term = dip.copy()
            term[near] = t
            acc = acc + term
        S[qi] = acc
    w = np.where(valid, S / FOUR_PI, np.nan)
    with np.errstate(invalid="ignore"):
        inside = (w >= 0.5).astype(np.uint8)
    return Result(w=w, inside=inside, occupied=occupied, near_faces=near_total / max(int(valid.sum()), 1))


def tolerance(case):
    """(nq,) the bound nf_s * 2^-48 of each query's scene (0 for a query of no scene)."""
    ok, _, _ = candidates(case)
    qs, fs = scene_of(case.query_start, case.nq, case.nscene), scene_of(case.face_start, case.nf, case.nscene)
    per = np.array([int((ok & (fs == s)).sum()) for s in range(case.nscene)] + [0])
    return per[qs] * 2.0 ** -48


# ------------------------------------------------------------------------------------------------ (b) the independent oracle
def excess_mp(q, T):
    """The signed solid angle of triangle T (9 floats) seen from q by the spherical excess of its three dihedral angles, mpmath 50 digits."""
    import mpmath as mp
    mp.mp.dps = 50
    u = [[mp.mpf(float(T[3 * j + k])) - mp.mpf(float(q[k])) for k in range(3)] for j in range(3)]
    dot = lambda x, y: x[0] * y[0] + x[1] * y[1] + x[2] * y[2]
    cross = lambda x, y: [x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]]
    det = dot(u[0], cross(u[1], u[2]))
    if det == 0:
        return mp.mpf(0)
    total = mp.mpf(0)
    for j in range(3):
        # the dihedral angle along direction j: between the planes (u_j, u_j+1) and (u_j, u_j+2)
        n1, n2 = cross(u[j], u[(j + 1) % 3]), cross(u[j], u[(j + 2) % 3])
        total += mp.acos(dot(n1, n2) / mp.sqrt(dot(n1, n1) * dot(n2, n2)))
    return (total - mp.pi) * mp.sign(det)


def winding_mp(case, rows):
    """w of the queries `rows` by oracle (b), as Python floats (rounded once from 50 digits)."""
    import mpmath as mp
    ok, tri, _ = candidates(case)
    qs, fs = scene_of(case.query_start, case.nq, case.nscene), scene_of(case.face_start, case.nf, case.nscene)
    out = []
    for i in rows:
        total = mp.mpf(0)
        for f in np.nonzero(ok & (fs == qs[i]))[0]:
            total += excess_mp(case.query[i], tri[f])
        out.append(float(total / (4 * mp.pi)))
    return np.array(out)


def surface_distance(case, rows):
    """A lower estimate of the distance of the queries `rows` to their scene's candidate faces: the least distance to a dense sampling of
    the faces minus the sample spacing (enough to tell "at least 1e-3 of the extent away")."""
    ok, tri, _ = candidates(case)
    T = tri[ok].reshape(-1, 3, 3)
    k = 6
    bary = np.array([[i, j, k - i - j] for i in range(k + 1) for j in range(k + 1 - i)], dtype=np.float64) / k
    pts = np.einsum("sb,fbc->fsc", bary, T).reshape(-1, 3)
    edge = max(float(np.linalg.norm(T - np.roll(T, 1, axis=1), axis=2).max()), 0.0) / k
    q = case.query[rows].astype(np.float64)
    return np.array([np.sqrt(((pts - x) ** 2).sum(1).min()) for x in q]) - edge


# ------------------------------------------------------------------------------------------------ meshes
_QUADS = ((4, 5, 7, 6), (0, 2, 3, 1), (1, 3, 7, 5), (0, 4, 6, 2), (2, 6, 7, 3), (0, 1, 5, 4))      # +z -z +x -x +y -y, corner = x + 2 y + 4 z


def cube(half=0.5, center=(0.0, 0.0, 0.0), flip=False):
    v = np.array([[(i & 1), (i >> 1) & 1, (i >> 2) & 1] for i in range(8)], dtype=np.float64) * (2 * half) - half + np.asarray(center)
    f = np.array([t for a, b, c, d in _QUADS for t in ((a, b, c), (a, c, d))])
    return v, (f[:, ::-1] if flip else f)


def uv_sphere(radius=0.45, nlat=32, nlon=64, center=(0.0, 0.0, 0.0), cap=0, hemisphere=False):
    """A UV sphere wound with its normals out: nlat bands between the poles, nlon sectors.  cap: that many bands are left out at the north
    pole (an open shell).  hemisphere: only the bands of the northern half (nlat even), the rim EXACTLY at z = center_z."""
    v = [[0.0, 0.0, radius]]
    for i in range(1, nlat):
        th = math.pi * i / nlat
        z = 0.0 if (hemisphere and 2 * i == nlat) else radius * math.cos(th)
        v += [[radius * math.sin(th) * math.cos(2 * math.pi * j / nlon), radius * math.sin(th) * math.sin(2 * math.pi * j / nlon), z] for j in range(nlon)]
    v.append([0.0, 0.0, -radius])
    ring = lambda i, j: 1 + (i - 1) * nlon + (j % nlon)
    south = len(v) - 1
    f = []
    last = nlat // 2 if hemisphere else nlat
    for i in range(last):
        for j in range(nlon):
            if i < cap:
                continue
            if i == 0:
                f.append((0, ring(1, j), ring(1, j + 1)))
            elif i == nlat - 1:
                f.append((south, ring(i, j + 1), ring(i, j)))
            else:
                f += [(ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)), (ring(i, j), ring(i + 1, j + 1), ring(i, j + 1))]
    return np.array(v) + np.asarray(center), np.array(f)


def tetrahedron():
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64) * 0.25
    return v, np.array([(1, 3, 2), (0, 2, 3), (0, 3, 1), (0, 1, 2)])


def _ball_queries(rng, n, radius=0.7):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True) * (radius * rng.random((n, 1)) ** (1 / 3))


def _lattice(k, seed):
    """k tiny dyadic triangles in k DISTINCT cells of a 7^3 grid, the two corner cells among them, in a shuffled face order."""
    rng = np.random.default_rng(seed)
    pick = rng.permutation(np.arange(1, 342))[:k - 2]
    cellsid = rng.permutation(np.concatenate([[0, 342], pick]))
    c = np.stack([cellsid % 7, (cellsid // 7) % 7, cellsid // 49], axis=1).astype(np.float64)
    v = np.stack([c, c + [0.25, 0, 0], c + [0, 0.25, 0]], axis=1).reshape(-1, 3)
    return v, np.arange(3 * k).reshape(k, 3)


CASES = ("cube", "nested", "tetra_face", "hemisphere", "sphere", "sphere_open", "odd", "all_bad", "scenes", "one_face", "no_face",
         "faces_511", "faces_512", "faces_513", "cells_127", "cells_128", "cells_129", "nq_0", "nq_1", "nq_255", "nq_256", "nq_257")


@functools.lru_cache(maxsize=None)
def make_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "cube" or name.startswith("nq_"):
        v, f = cube()
        q = [(0, 0, 0), (0.25, -0.125, 0.375), (0.75, 0, 0), (0, -2, 0.25), (0.5, 0, 0), (0, 0, -0.5), (0.5, 0.5, 0), (0, -0.5, 0.5), (0.5, 0.5, 0.5),
             (-0.5, 0.5, -0.5), (0.5, 0.25, 0.125), (1000, 0, 0), (-1000, 1000, 1000), (0, 0, 1e6)]
        known = ((0, 1.0), (1, 1.0), (2, 0.0), (3, 0.0), (4, 0.5), (5, 0.5), (6, 0.25), (7, 0.25), (8, 0.125), (9, 0.125), (10, 0.5))
        if name == "cube":
            q = np.concatenate([np.array(q, dtype=np.float64), rng.uniform(-0.9, 0.9, (120, 3))])
            return _case(q, v, f, on_surface=3, known=known)
        n = int(name[3:])
        return _case(np.concatenate([np.array(q, dtype=np.float64), rng.uniform(-0.9, 0.9, (300, 3))])[:n], v, f, on_surface=sum(i < n for i in (4, 5, 10)),
                     known=known[:min(n, 11)])
    if name == "nested":
        v0, f0 = cube(0.5)
        v1, f1 = cube(0.25, flip=True)
        q = np.concatenate([[(0, 0, 0), (0.125, 0.0625, -0.125), (0.375, 0, 0), (-0.375, 0.375, 0.3125), (0.75, 0, 0)], rng.uniform(-0.7, 0.7, (100, 3))])
        return _case(q, np.concatenate([v0, v1]), np.concatenate([f0, f1 + 8]), known=((0, 0.0), (1, 0.0), (2, 1.0), (3, 1.0), (4, 0.0)))
    if name == "tetra_face":
        v, f = tetrahedron()
        return _case(np.concatenate([v[:1], _ball_queries(rng, 40)]), v, f[:1], known=((0, math.acos(23 / 27) / (4 * math.pi)),))
    if name == "hemisphere":
        v, f = uv_sphere(0.5, 16, 32, hemisphere=True)
        rim = np.concatenate([0.4 * _ball_queries(rng, 24)[:, :2], np.zeros((24, 1))], axis=1)
        return _case(np.concatenate([rim, _ball_queries(rng, 200) + [0, 0, 0.05]]), v, f, on_surface=24, known=tuple((i, 0.5) for i in range(24)))
    if name in ("sphere", "sphere_open"):
        v, f = uv_sphere(cap=4 if name == "sphere_open" else 0)
        return _case(_ball_queries(np.random.default_rng(7), 500), v, f)
    if name == "odd":
        v, f = uv_sphere(0.45, 12, 24)
        nv = len(v)
        extra = np.array([[np.nan, 0, 0], [np.inf, 0.1, 0.2], [0.125, 0.125, 0.125], [0.25, 0.25, 0.25], [0.5, 0.5, 0.5], [0.125, 0.125, 0.125]])
        bad = np.array([(-1, 0, 1), (2, nv + 6, 3), (0, nv, 5), (7, 8, nv + 1), (nv + 2, nv + 3, nv + 4), (nv + 2, nv + 2, nv + 3), (nv + 2, nv + 5, nv + 3),
                        (3, 3, 3)])
        order = rng.permutation(len(f) + len(bad))
        faces = np.concatenate([f, bad])[order]
        q = np.concatenate([[(np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (0, 0, 0), (900, 0, 0)], _ball_queries(rng, 300)])
        return _case(q, np.concatenate([v, extra]), faces, known=((3, 1.0),))
    if name == "all_bad":
        v = np.array([[0, 0, 0], [0.25, 0.25, 0.25], [0.5, 0.5, 0.5], [np.nan, 0, 0], [0, np.inf, 0], [1, 0, 0]])
        f = np.array([(0, 1, 2), (0, 0, 1), (3, 0, 5), (4, 5, 0), (-1, 0, 5), (0, 5, 6), (2, 1, 0)])
        return _case(np.concatenate([[(0.1, 0.2, 0.3), (np.nan, 0, 0)], _ball_queries(rng, 30)]), v, f)
    if name == "scenes":
        meshes = [cube(), uv_sphere(0.4, 8, 16, center=(0.1, 0, 0)), None, uv_sphere(0.3, 6, 12), tetrahedron()]
        counts = [100, 100, 30, 0, 70]
        vs, fs, fstart, nv = [], [], [0], 0
        for m in meshes:
            if m is not None:
                vs.append(m[0]), fs.append(m[1] + nv)
                nv += len(m[0])
            fstart.append(fstart[-1] + (0 if m is None else len(m[1])))
        qstart = np.concatenate([[0], np.cumsum(counts)])
        return _case(_ball_queries(rng, 300), np.concatenate(vs), np.concatenate(fs), query_start=qstart, face_start=fstart)
    if name == "one_face":
        v, f = tetrahedron()
        return _case(_ball_queries(rng, 40), v, f[:1])
    if name == "no_face":
        return _case(_ball_queries(rng, 40), np.zeros((0, 3)), np.zeros((0, 3)))
    if name.startswith("faces_"):
        v, f = uv_sphere(0.45, 10, 32)                     # 576 faces: the first k of them, an open shell
        return _case(_ball_queries(rng, 48), v, f[:int(name[6:])])
    if name.startswith("cells_"):
        v, f = _lattice(int(name[6:]), 11)
        return _case(rng.uniform(-1, 7.5, (48, 3)), v, f)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def parts(name):
    return omega_matrix(make_case(name))


@functools.lru_cache(maxsize=None)
def refs(name, method=EXACT, cells=0, beta=2.0):
    """The oracle's Result for a case and a setting, computed once and shared; callers must not write into it."""
    return winding(make_case(name), method, cells, beta, parts(name))


def scene_case(case, s):
    """Scene s of a case as a case of its own: (case, (q0, q1))."""
    q0, q1 = (int(np.clip(case.query_start[k], 0, case.nq)) for k in (s, s + 1))
    f0, f1 = (int(np.clip(case.face_start[k], 0, case.nf)) for k in (s, s + 1))
    return _case(case.query[q0:q1], case.vertices, case.faces[f0:f1]), (q0, q1)
