"""Test infrastructure of the neighbourhood entries (include/mvd_hip.h: mvd_knn_points, mvd_point_normals): the case tables, an fp32
restatement of the k-nearest rule and a float64 restatement of the normal rule, in numpy alone -- importable without a GPU.

knn()      forms d2 with elementwise float32 sub, mul and add in the rule's order (every numpy op rounds once, nothing is contracted) and
           sorts each query's candidates by (d2, j) with a stable sort over ascending j.  It reproduces the rule bit for bit without
           being the code under test.
normals()  forms centre and covariance in float64 in list order (a loop over the k columns, never numpy's pairwise sum) and takes the
           eigenvectors from numpy.linalg.eigh -- another solver than the kernel's Jacobi, which is the point of the comparison.

The search cases are those of tests/nearest_f64.py (imported, not edited) and three of this file's own.  Shapes are a few thousand
points; every reference is computed once (functools.lru_cache)."""
import functools
from dataclasses import dataclass

import numpy as np

import nearest_f64 as NN

KS = (1, 3, 8, 16, 32)
MAX_K = 32
ELLIPSOID = (0.6, 0.45, 0.3)          # semi-axes of the analytic ellipsoid
GAP_FLOOR = 2.0 ** -10                # a normal is compared only where (l1 - l0) / l2 reaches this
GAP_CAP = 0.01                        # ... and at most this share of a case's valid points may lie below it


@dataclass
class Case:
    """The arguments of one mvd_knn_points call as numpy arrays."""
    query: np.ndarray                 # (nq, 3) float32
    target: np.ndarray                # (nt, 3) float32
    query_start: np.ndarray           # (nscene + 1,) int64
    target_start: np.ndarray

    @property
    def nq(self):
        return int(self.query.shape[0])

    @property
    def nt(self):
        return int(self.target.shape[0])

    @property
    def nscene(self):
        return int(self.query_start.size) - 1


def _self(points, start=None):
    points = np.ascontiguousarray(points, dtype=np.float32)
    start = np.array([0, points.shape[0]]) if start is None else np.asarray(start)
    return Case(query=points, target=points, query_start=start.astype(np.int64), target_start=start.astype(np.int64))


def sphere_surface(n, seed, noise=0.002):
    """n points around the sphere of radius nearest_f64.SPHERE_R with radial noise of that standard deviation."""
    return NN.sphere_points(n, seed, noise).numpy()


def ellipsoid_surface(n, seed):
    """(points (n, 3) float32 on the ellipsoid ELLIPSOID to fp32 rounding, the true unit normals (n, 3) float64 at those points)."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    p = (v * np.array(ELLIPSOID)).astype(np.float32)
    g = p.astype(np.float64) / np.array(ELLIPSOID) ** 2
    return p, g / np.linalg.norm(g, axis=1, keepdims=True)


def _case_sphere_self():
    return _self(sphere_surface(3001, 11))          # the query set IS the target set: every point its own neighbour 0


def _case_four_scenes():
    """Scenes of 700, 2 (fewer than any k > 2), 0 and 1301 points, each searched against itself."""
    sizes = (700, 2, 0, 1301)
    pts = np.concatenate([sphere_surface(m, 20 + s) + np.float32(0.1 * s) for s, m in enumerate(sizes) if m])
    return _self(pts, np.concatenate([[0], np.cumsum(sizes)]))


def _case_few_targets():
    """Two scenes: 5 targets for 300 queries (fewer than k for k = 8, 16, 32), and 40 targets for 77 queries."""
    rng = np.random.default_rng(5)
    u = lambda n: ((rng.random((n, 3)) * 2 - 1) * NN.BOX).astype(np.float32)
    return Case(query=u(377), target=u(45), query_start=np.array([0, 300, 377]), target_start=np.array([0, 5, 45]))


OWN = {"sphere_self": _case_sphere_self, "four_scenes": _case_four_scenes, "few_targets": _case_few_targets}
CASES = list(NN.CASES) + list(OWN)


@functools.lru_cache(maxsize=None)
def make_case(name):
    if name in OWN:
        return OWN[name]()
    c = NN.make_case(name)
    return Case(query=c.query.numpy(), target=c.target.numpy(), query_start=c.query_start.numpy().astype(np.int64),
                target_start=c.target_start.numpy().astype(np.int64))


def scene_case(case, s):
    """Scene s of a case as a case of its own, and the row offset of its targets in the batch."""
    q0, q1, t0, t1 = int(case.query_start[s]), int(case.query_start[s + 1]), int(case.target_start[s]), int(case.target_start[s + 1])
    return Case(query=case.query[q0:q1], target=case.target[t0:t1], query_start=np.array([0, q1 - q0]), target_start=np.array([0, t1 - t0])), t0


def _scene_of(start, n):
    i = np.arange(n)
    s = np.searchsorted(start[1:], i, side="right")
    return np.where(i >= start[0], s, start.size - 1)


def _d2(q, t, dtype):
    q, t = q.astype(dtype), t.astype(dtype)
    with np.errstate(all="ignore"):
        d = [q[:, None, a] - t[None, :, a] for a in range(3)]
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def knn(case, k, dtype=np.float32, chunk=256):
    """The rule restated -> (index (nq, k) int64, dist2 (nq, k) `dtype`): per query the first k candidates in (d2, j) order, -1 / +inf
    in the slots behind them.  A candidate is a target of the query's scene whose d2 is < +inf."""
    nq, nt, N = case.nq, case.nt, case.nscene
    index = np.full((nq, k), -1, dtype=np.int64)
    dist2 = np.full((nq, k), np.inf, dtype=dtype)
    if nq == 0 or nt == 0:
        return index, dist2
    qs, ts = _scene_of(case.query_start, nq), _scene_of(case.target_start, nt)
    for a in range(0, nq, chunk):
        b = min(a + chunk, nq)
        d2 = _d2(case.query[a:b], case.target, dtype)
        ok = (d2 < np.inf) & (qs[a:b, None] == ts[None, :]) & (qs[a:b, None] < N)
        d2 = np.where(ok, d2, np.asarray(np.inf, dtype=dtype))
        order = np.argsort(d2, axis=1, kind="stable")[:, :k]          # stable over ascending j: the lexicographic (d2, j) order
        best = np.take_along_axis(d2, order, axis=1)
        m = order.shape[1]
        index[a:b, :m] = np.where(best < np.inf, order, -1)
        dist2[a:b, :m] = best
    return index, dist2


@functools.lru_cache(maxsize=None)
def refs(name):
    """(index (nq, MAX_K), dist2 (nq, MAX_K)) of a case: the lists of every k <= MAX_K are their first k columns."""
    return knn(make_case(name), MAX_K)


# ------------------------------------------------------------------------------------------------ normals
@dataclass
class NormalCase:
    target: np.ndarray                # (nt, 3) float32
    index: np.ndarray                 # (n, k) int32 neighbour rows (the oracle's own lists, or hand-made ones)
    points: np.ndarray                # (n, 3) float32: the points the normals belong to (for `toward`)
    truth: object = None              # (n, 3) float64 analytic normals, where the surface has them


def _knn_lists(points, k):
    return knn(_self(points), k)[0].astype(np.int32)


def _ncase_sphere():
    p = sphere_surface(2000, 31)
    t = p.astype(np.float64)
    return NormalCase(target=p, index=_knn_lists(p, 16), points=p, truth=t / np.linalg.norm(t, axis=1, keepdims=True))


def _ncase_ellipsoid():
    p, truth = ellipsoid_surface(2500, 32)
    return NormalCase(target=p, index=_knn_lists(p, 16), points=p, truth=truth)


def _ncase_uniform():
    rng = np.random.default_rng(33)
    p = ((rng.random((1500, 3)) * 2 - 1) * NN.BOX).astype(np.float32)
    return NormalCase(target=p, index=_knn_lists(p, 8), points=p)


def _ncase_lattice_plane():
    """A 24 x 24 lattice of spacing 1 / 16 in the plane z = 0.375: every coordinate dyadic, every centred difference and product exact."""
    i, j = np.meshgrid(np.arange(24), np.arange(24), indexing="ij")
    p = np.stack([i.ravel() / 16 - 0.75, j.ravel() / 16 - 0.5, np.full(i.size, 0.375)], axis=1).astype(np.float32)
    return NormalCase(target=p, index=_knn_lists(p, 16), points=p, truth=np.tile([0.0, 0.0, 1.0], (p.shape[0], 1)))


def _ncase_odd_rows():
    """Hand-made rows over a small target: the rule's invalid and skipped entries, one per point."""
    t = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0],          # 0..3 collinear along x
                  [1, 1, 0], [2, 2, 0], [0, 1, 0], [0, 0, 1],          # 4, 5 with 0: collinear on the diagonal; 6, 7 span the rest
                  [np.nan, 0, 0], [0, np.inf, 0], [0.5, 0.25, -1]], dtype=np.float32) * np.float32(0.25)
    rows = [[0, 0, 0, 0, 0, 0],              # coincident: invalid
            [0, 1, 2, 3, 1, 2],              # collinear along an axis: invalid
            [0, 4, 5, 0, 4, 5],              # collinear along the diagonal: invalid
            [0, 1, -1, -1, -1, -1],          # two usable rows: invalid
            [0, 1, 8, 9, -1, 11],            # non-finite, -1 and out-of-range entries are skipped: two usable rows, invalid
            [0, 1, 6, -1, 8, 11],            # ... three usable rows in the plane z = 0: valid, normal (0, 0, 1)
            [0, 1, 6, 7, 10, 4],             # a generic valid row
            [7, 6, 1, 0, 9, -5]]             # valid, with skipped entries behind
    idx = np.array(rows, dtype=np.int32)
    return NormalCase(target=t, index=idx, points=np.ascontiguousarray(t[np.clip(idx[:, 0], 0, None)]))


NORMAL_CASES = {"sphere": _ncase_sphere, "ellipsoid": _ncase_ellipsoid, "uniform": _ncase_uniform, "lattice_plane": _ncase_lattice_plane,
                "odd_rows": _ncase_odd_rows}


@functools.lru_cache(maxsize=None)
def make_normal_case(name):
    return NORMAL_CASES[name]()


@dataclass
class NormalRef:
    case: NormalCase
    normal: np.ndarray                # (n, 3) float64 unit eigenvector of l0 under the sign rule without `toward`; 0 where not valid
    lam: np.ndarray                   # (n, 3) float64 eigenvalues, ascending, raised to 0
    variation: np.ndarray             # (n,) float64, NaN where not valid
    valid: np.ndarray                 # (n,) bool
    m: np.ndarray                     # (n,) used rows
    exact: np.ndarray                 # (n,) bool: not valid because the rows are exactly degenerate (l1 at rounding level) or m < 3
    compared: np.ndarray              # (n,) bool: valid with (l1 - l0) / l2 >= GAP_FLOOR


def sign_rule(v):
    """The rule's sign without `toward`: the component of largest magnitude positive, the lowest axis between equal magnitudes."""
    lead = np.argmax(np.abs(v), axis=1)          # (the first of equal maxima)
    s = np.where(np.take_along_axis(v, lead[:, None], axis=1)[:, 0] < 0, -1.0, 1.0)
    return v * s[:, None]


def normals(case):
    """The rule restated in float64 with numpy.linalg.eigh as the solver."""
    t, idx = case.target, case.index.astype(np.int64)
    n, k = idx.shape
    nt = t.shape[0]
    inside = (idx >= 0) & (idx < nt)
    x = t[np.clip(idx, 0, max(nt - 1, 0))].astype(np.float64)          # (n, k, 3)
    used = inside & np.isfinite(x).all(axis=2)
    m = used.sum(axis=1)
    total = np.zeros((n, 3))
    for e in range(k):                                                 # list order
        total += np.where(used[:, e, None], x[:, e], 0.0)
    with np.errstate(all="ignore"):
        c = total / m[:, None]
    C = np.zeros((n, 3, 3))
    for e in range(k):
        d = np.where(used[:, e, None], x[:, e] - c, 0.0)
        C += d[:, :, None] * d[:, None, :]
    enough = m >= 3
    lam, vec = np.linalg.eigh(np.where(enough[:, None, None], C, np.eye(3)))
    lam = np.maximum(lam, 0.0)
    # eigh leaves l1 of an exactly degenerate row at rounding level (a few 2^-53 l2) where the rule's Jacobi, whose rotations of these
    # hand-made rows are exact, gives 0: everything at or below 2^-40 l2 is degenerate HERE, and test_cpu_knn.py asserts that no
    # case holds a point between 2^-40 and 2^-20, so that the two can never disagree.
    valid = enough & (lam[:, 1] > 2.0 ** -40 * lam[:, 2]) & (lam[:, 2] > 0)
    normal = np.where(valid[:, None], sign_rule(vec[:, :, 0]), 0.0)
    with np.errstate(all="ignore"):
        variation = np.where(valid, lam[:, 0] / ((lam[:, 0] + lam[:, 1]) + lam[:, 2]), np.nan)
        gap = np.where(valid, (lam[:, 1] - lam[:, 0]) / lam[:, 2], 0.0)
    return NormalRef(case=case, normal=normal, lam=lam, variation=variation, valid=valid, m=m, exact=~valid, compared=valid & (gap >= GAP_FLOOR))


@functools.lru_cache(maxsize=None)
def normal_refs(name):
    return normals(make_normal_case(name))


def normal_bound(ref):
    """(n,) the bound on max_a |n_kernel - n_oracle|_a (after matching the sign) for the compared points:
        64 * 2^-53 * l2 / (l1 - l0) + 2^-24.
    Both sides decompose the SAME covariance bits (same operations in the same order).  A symmetric 3 x 3 eigen solver -- LAPACK's or a
    few Jacobi sweeps -- is backward stable with an error of norm at most ~8 * 2^-53 * l2; by Davis-Kahan the eigenvector of l0 then
    turns by at most 2 * 8 * 2^-53 * l2 / (l1 - l0); two solvers: 32; doubled for the normalisation and the slack of '~': 64.  The
    kernel rounds each component (magnitude <= 1) to fp32 once: at most 2^-25, stated as 2^-24."""
    with np.errstate(all="ignore"):
        return 64 * 2.0 ** -53 * ref.lam[:, 2] / (ref.lam[:, 1] - ref.lam[:, 0]) + 2.0 ** -24


def angle_to(a, b):
    """(n,) the angle in radians between unit vectors up to sign."""
    return np.arcsin(np.clip(np.linalg.norm(np.cross(a, b), axis=1), 0.0, 1.0))
