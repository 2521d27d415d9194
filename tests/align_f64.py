"""Test infrastructure of the alignment (include/mvd_hip.h: mvd_align_apply, mvd_align_fit, mvd_align_icp): the case table and a float64
oracle that shares no method with the code under test.

  apply    the rule restated in numpy float64 -- every numpy op rounds once, there is no contraction -- with one cast to fp32: it
           reproduces the kernel bit for bit.
  sums     the nineteen moment sums of the accepted pairs by math.fsum over the exact fp64 products: correctly rounded, no order.
  solve    Kabsch / Umeyama by SVD with the determinant correction, not by quaternion.
  icp      the loop on nearest_f64's brute force (the fp32 restatement of the search: the correspondences the library must find).

The shape is the surface of an ellipsoid of radii (0.6, 0.42, 0.25) with a one-sided bulge, so that no rotation maps it onto itself.
Every reference is a few thousand points and is computed once (functools.lru_cache)."""
import functools
import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

import nearest_f64 as NN

CHUNK = 1024                      # MVD_ALIGN_CHUNK (tests/test_cpu_align.py holds it to the header)
RADII = (0.6, 0.42, 0.25)
INF = float("inf")


# ------------------------------------------------------------------------------------------------ shapes and transforms
def bulged_ellipsoid(n, seed):
    """(n, 3) fp32 points on the bulged ellipsoid, unit directions drawn from a seeded normal."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, 3, generator=g, dtype=torch.float64)
    v = (v / v.norm(dim=1, keepdim=True)).float()
    p = v * torch.tensor(RADII)
    bulge = ((v * torch.tensor([1.0, 1.0, 0.5])).sum(1) / 1.5 - 0.6).clamp(min=0.0)
    return (p * (1.0 + 0.35 * bulge)[:, None]).contiguous()


def similarity(s, degrees, axis, t):
    """(4, 4) float64 [[s R, t], [0, 1]] with R the rotation by `degrees` about `axis` (Rodrigues)."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = math.radians(degrees)
    R = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = s * R, t
    return M


def scene_of(start, n):
    """(n,) scene of every row, -1 for a row of no scene; start: nscene + 1 offsets."""
    start = np.clip(np.asarray(start, dtype=np.int64), 0, n)
    i = np.arange(n)
    s = np.searchsorted(start[1:], i, side="right")
    return np.where((i >= start[0]) & (s < len(start) - 1), s, -1)


def apply(m, xyz, start):
    """THE apply rule restated: m (N, 3, 4) float64, xyz (n, 3) fp32 tensor, start N + 1 offsets -> (n, 3) fp32 tensor."""
    x = xyz.numpy().astype(np.float64)
    m = np.asarray(m, dtype=np.float64).reshape(-1, 3, 4)
    sc = scene_of(start, x.shape[0])
    mm = m[np.clip(sc, 0, None)]                                  # (n, 3, 4)
    with np.errstate(all="ignore"):
        moved = ((mm[:, :, 0] * x[:, None, 0] + mm[:, :, 1] * x[:, None, 1]) + mm[:, :, 2] * x[:, None, 2]) + mm[:, :, 3]
        out = np.where(sc[:, None] >= 0, moved.astype(np.float32), xyz.numpy())
    return torch.from_numpy(np.ascontiguousarray(out))


def d2_rows(p, q):
    """fp32 d2 of row pairs in the search's order (torch ops: one rounding each)."""
    d = p - q
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


# ------------------------------------------------------------------------------------------------ sums and solve
def accepted_pairs(moved, target, index, dist2, max_d2):
    """The pair rule restated -> (accepted (n,) bool, j (n,) int64, d2 (n,) fp32)."""
    n, nt = moved.shape[0], target.shape[0]
    j = torch.arange(n) if index is None else index.long()
    has = (j >= 0) & (j < nt)
    q = target[j.clamp(0, max(nt - 1, 0))] if nt else torch.zeros(n, 3)
    d2 = d2_rows(moved, q) if dist2 is None else dist2
    ok = has & (d2 < torch.tensor(INF)) & (d2 <= torch.tensor(max_d2, dtype=torch.float32))
    return ok, j, d2


def moment_sums(moved, target, index, dist2, max_d2, start):
    """(N, 19) float64: the sums of every scene, each correctly rounded (math.fsum of exact products)."""
    ok, j, d2 = accepted_pairs(moved, target, index, dist2, max_d2)
    sc = scene_of(start, moved.shape[0])
    out = np.zeros((len(start) - 1, 19))
    for s in range(len(start) - 1):
        rows = torch.from_numpy((sc == s)) & ok
        p = moved[rows].numpy().astype(np.float64)
        q = target[j[rows]].numpy().astype(np.float64)
        cols = [np.ones(len(p))] + [p[:, a] for a in range(3)] + [q[:, a] for a in range(3)] + \
            [p[:, a] * q[:, b] for a in range(3) for b in range(3)]
        cols = [math.fsum(c.tolist()) for c in cols]
        cols.append(math.fsum((p * p).ravel().tolist()))
        cols.append(math.fsum((q * q).ravel().tolist()))
        cols.append(math.fsum(d2[rows].double().tolist()))
        out[s] = cols
    return out


def solve_svd(sums, scale):
    """Umeyama from the nineteen sums -> (s, R (3, 3), t (3,)), the identity where the rule says so."""
    ident = (1.0, np.eye(3), np.zeros(3))
    n = sums[0]
    if not np.all(np.isfinite(sums)) or not n >= 3:
        return ident
    mp, mq = sums[1:4] / n, sums[4:7] / n
    M = sums[7:16].reshape(3, 3) / n - np.outer(mp, mq)          # M[a][b] = cov(p_a, q_b)
    var = sums[16] / n - mp @ mp
    if not var > 0:
        return ident
    U, S, Vt = np.linalg.svd(M.T)                                # M^T = cov(q, p) = U S V^T;  R = U D V^T
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt)) or 1.0])
    R = U @ D @ Vt
    s = float((S * np.diag(D)).sum() / var) if scale else 1.0
    if not s > 0:
        return ident
    return s, R, mq - s * R @ mp


def step_matrix(s, R, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = s * R, t
    return M


def spread_factor(points):
    """1 + |mu|^2 / sigma^2 of a point set: what raw moments lose against centred ones."""
    p = points.double().numpy()
    p = p[np.isfinite(p).all(1)]
    mu = p.mean(0)
    return 1.0 + float(mu @ mu) / float(((p - mu) ** 2).sum(1).mean())


# ------------------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    """The arguments of one alignment call as CPU data.  index None: row i goes with row i."""
    source: torch.Tensor                  # (n, 3) fp32
    start: list                           # nscene + 1 offsets of source
    target: torch.Tensor                  # (nt, 3) fp32
    tstart: list
    index: Optional[torch.Tensor] = None  # (n,) int32: fit cases with a given pairing
    dist2: Optional[torch.Tensor] = None
    max_distance: Optional[float] = None
    scale: bool = True
    truth: list = field(default_factory=list)      # per scene a (4, 4) the fit must find, or None
    iters: int = 0                        # > 0: an ICP case
    perm: Optional[torch.Tensor] = None   # ICP cases: target row of source row i

    @property
    def n(self):
        return int(self.source.shape[0])

    @property
    def nt(self):
        return int(self.target.shape[0])

    @property
    def nscene(self):
        return len(self.start) - 1

    @property
    def max_d2(self):
        """fl32(fl32(max_distance)^2): what the host passes down."""
        if self.max_distance is None:
            return INF
        m = np.float32(self.max_distance)
        return float(np.float32(m * m))


TRUTH_PAIRS = similarity(1.3, 37.0, (1, 2, 3), (0.2, -0.1, 0.05))
TRUTH_SIM5 = similarity(1.05, 5.0, (0.3, -1, 0.5), (0.02, -0.01, 0.0067))
TRUTH_RIGID10 = similarity(1.0, 10.0, (0.3, -1, 0.5), (0.05, -0.025, 0.0167))


def _image(src, M):
    return apply(M[:3][None], src, [0, src.shape[0]])


def _case_pairs(seed):
    src = bulged_ellipsoid(4099, seed)
    return Case(source=src, start=[0, 4099], target=_image(src, TRUTH_PAIRS), tstart=[0, 4099], truth=[TRUTH_PAIRS])


def _case_chunk_edges(seed):
    lens = [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
    start = [0] + np.cumsum(lens).tolist()
    src = bulged_ellipsoid(start[-1], seed)
    truth = [similarity(1.0 + 0.1 * k, 20.0 + 15 * k, (1, k, 2 - k), (0.1 * k, -0.05, 0.02 * k)) for k in range(4)]
    tgt = apply(np.stack([t[:3] for t in truth]), src, start)
    return Case(source=src, start=start, target=tgt, tstart=start, truth=truth)


def _case_small_scenes(seed):
    lens = [0, 1, 2, 3, 500]
    start = [0] + np.cumsum(lens).tolist()
    src = bulged_ellipsoid(start[-1], seed)
    T = similarity(0.9, 25.0, (2, -1, 1), (0.05, 0.1, -0.2))
    return Case(source=src, start=start, target=_image(src, T), tstart=start, truth=[None, None, None, None, T])


def _case_planar(seed):
    src = bulged_ellipsoid(777, seed)
    src[:, 2] = 0.0
    T = similarity(1.1, 50.0, (1, 1, 1), (0.1, 0.0, -0.1))
    return Case(source=src, start=[0, 777], target=_image(src, T), tstart=[0, 777], truth=[T])


def _case_mirrored(seed):
    src = bulged_ellipsoid(777, seed)
    tgt = _image(src, similarity(1.0, 30.0, (0, 1, 1), (0.0, 0.1, 0.0)))
    tgt[:, 0] = -tgt[:, 0]
    return Case(source=src, start=[0, 777], target=tgt, tstart=[0, 777], truth=[None])


def _case_offset(seed):
    src = bulged_ellipsoid(4099, seed) + 8.0
    return Case(source=src, start=[0, 4099], target=_image(src, TRUTH_PAIRS), tstart=[0, 4099], truth=[TRUTH_PAIRS])


def _case_gate(seed):
    """An ICP step's input on a dyadic lattice: 40 targets on multiples of 1/8, sources on multiples of 1/16 -- every d2 is an exact
    multiple of 1/256 in fp32, and max_distance = 3/16 puts the threshold 9/256 on a value that occurs."""
    g = torch.Generator().manual_seed(seed)
    tgt = torch.randint(0, 9, (40, 3), generator=g).float() * 0.125 - 0.5
    src = torch.randint(0, 17, (1200, 3), generator=g).float() * 0.0625 - 0.5
    index, dist2 = NN.nearest(NN.Case(query=src, target=tgt, query_start=torch.tensor([0, 1200]), target_start=torch.tensor([0, 40])))
    return Case(source=src.contiguous(), start=[0, 1200], target=tgt.contiguous(), tstart=[0, 40], index=index.to(torch.int32), dist2=dist2,
                max_distance=0.1875, scale=False, truth=[None])


def _case_nonfinite(seed):
    src = bulged_ellipsoid(1000, seed)
    T = similarity(1.2, 15.0, (1, 0, 1), (0.0, 0.05, 0.1))
    tgt = _image(src, T)
    bad = [float("nan"), INF, -INF]
    for k in range(30):
        src[(k * 37) % 1000, k % 3] = bad[k % 3]
        tgt[(k * 61 + 5) % 1000, (k + 1) % 3] = bad[(k + 1) % 3]
    return Case(source=src, start=[0, 1000], target=tgt, tstart=[0, 1000], truth=[T])


def _icp_case(n, T, seed, iters, scale):
    src = bulged_ellipsoid(n, seed)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed + 1))
    tgt = torch.empty(n, 3)
    tgt[perm] = _image(src, T)                                   # source row i sits at target row perm[i]
    return Case(source=src, start=[0, n], target=tgt.contiguous(), tstart=[0, n], scale=scale, truth=[T], iters=iters, perm=perm)


FIT_CASES = {
    "pairs_4099": (_case_pairs, 0),
    "chunk_edges": (_case_chunk_edges, 1),
    "small_scenes": (_case_small_scenes, 2),
    "planar": (_case_planar, 3),
    "mirrored": (_case_mirrored, 4),
    "offset": (_case_offset, 0),
    "gate": (_case_gate, 6),
    "nonfinite": (_case_nonfinite, 7),
}
ICP_CASES = {
    "icp_sim5": (lambda seed: _icp_case(1537, TRUTH_SIM5, seed, 20, True), 8),
    "icp_rigid10": (lambda seed: _icp_case(2048, TRUTH_RIGID10, seed, 30, False), 9),
}
CASES = {**FIT_CASES, **ICP_CASES}


@functools.lru_cache(maxsize=None)
def make_case(name):
    fn, seed = CASES[name]
    return fn(8100 + seed)


@dataclass
class FitRef:
    case: Case
    accepted: torch.Tensor            # (n,) bool
    sums: np.ndarray                  # (N, 19)
    steps: list                       # per scene (s, R, t) by SVD
    rms: np.ndarray                   # (N,) NaN without a pair
    pairs: np.ndarray                 # (N,) int64


def fit_ref(case, moved=None):
    """One fit step of the oracle on `moved` (default: the source as it is) against the case's pairing."""
    moved = case.source if moved is None else moved
    ok, _, _ = accepted_pairs(moved, case.target, case.index, case.dist2, case.max_d2)
    sums = moment_sums(moved, case.target, case.index, case.dist2, case.max_d2, case.start)
    with np.errstate(all="ignore"):
        rms = np.where(sums[:, 0] > 0, np.sqrt(sums[:, 18] / np.maximum(sums[:, 0], 1)), np.nan)
    return FitRef(case=case, accepted=ok, sums=sums, steps=[solve_svd(s, case.scale) for s in sums], rms=rms, pairs=sums[:, 0].astype(np.int64))


@functools.lru_cache(maxsize=None)
def fit_refs(name):
    return fit_ref(make_case(name))


@dataclass
class IcpRef:
    case: Case
    matrix: np.ndarray                # (4, 4)
    rms: np.ndarray                   # (iters + 1,)
    pairs: np.ndarray
    right: np.ndarray                 # (iters + 1,) correspondences equal to the permutation
    index: torch.Tensor               # the final correspondences
    moved: torch.Tensor


def icp(case, iters=None, init=None):
    """The ICP loop of the rule on the brute-force search, one scene."""
    iters = case.iters if iters is None else iters
    m = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    rms, pairs, right = [], [], []
    qs, ts = torch.tensor(case.start), torch.tensor(case.tstart)
    for k in range(iters + 1):
        moved = apply(m[:3][None], case.source, case.start)
        index, dist2 = NN.nearest(NN.Case(query=moved, target=case.target, query_start=qs, target_start=ts))
        sums = moment_sums(moved, case.target, index, dist2, case.max_d2, case.start)[0]
        rms.append(math.sqrt(sums[18] / sums[0]) if sums[0] > 0 else float("nan"))
        pairs.append(int(sums[0]))
        right.append(int((index == case.perm).sum()) if case.perm is not None else -1)
        if k < iters:
            m = step_matrix(*solve_svd(sums, case.scale)) @ m
    return IcpRef(case=case, matrix=m, rms=np.array(rms), pairs=np.array(pairs), right=np.array(right), index=index, moved=moved)


@functools.lru_cache(maxsize=None)
def icp_refs(name):
    return icp(make_case(name))


def quaternion_solve(sums, scale):
    """Horn's solve with numpy's symmetric eigensolver: the method of the library in other code, for the SVD-quaternion gap."""
    n = sums[0]
    mp, mq = sums[1:4] / n, sums[4:7] / n
    M = sums[7:16].reshape(3, 3) / n - np.outer(mp, mq)
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, M[1, 1] - M[0, 0] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, M[2, 2] - M[0, 0] - M[1, 1]]])
    N = N + np.triu(N, 1).T
    w, x, y, z = np.linalg.eigh(N)[1][:, -1]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    s = float((R.T * M).sum() / (sums[16] / n - mp @ mp)) if scale else 1.0
    return s, R, mq - s * R @ mp
