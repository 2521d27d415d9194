"""Test infrastructure of the point-to-plane entries (include/mvd_hip.h: mvd_plane_fit, mvd_plane_icp, mvd_plane_solve): the case
table and a float64 restatement of the rule -- the pair rule of tests/align_f64.py (imported, not edited), the thirty sums with every
product formed as the rule forms it and the additions done exactly (math.fsum), and the solve through numpy.linalg.eigh, another
solver than the library's Jacobi.  Normals of a target come from the oracle of tests/knn_f64.py.  Importable without a GPU."""
import functools
import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

import align_f64 as A
import knn_f64 as K
import nearest_f64 as NN

SUMS, HISTORY = 30, 4
EPS_RANK = 1e-9                   # MVD_PLANE_EPS_RANK (tests/test_cpu_plane.py holds it to the header)
CLEAR = 16.0                      # every eigenvalue of every case is this factor away from EPS_RANK * lambda_max, on either side
INF = float("inf")
TRUTH_SLIDE = A.similarity(1.0, 8.0, (1, 2, 3), (0.03, -0.02, 0.01))
SMALL = A.similarity(1.0, 3.0, (2, -1, 1), (0.01, 0.02, -0.015))


def target_normals(target, start, k=16):
    """(nt, 3) fp32: the oracle's k-neighbour normals of a target cloud, scene by scene (zero where the oracle has none)."""
    t = target.numpy()
    st = np.asarray(start, dtype=np.int64)
    index = K.knn(K.Case(query=t, target=t, query_start=st, target_start=st), k)[0].astype(np.int32)
    return torch.from_numpy(K.normals(K.NormalCase(target=t, index=index, points=t)).normal.astype(np.float32))


def bumped_ellipsoid(n, seed):
    """(n, 3) fp32 on the ellipsoid of semi-axes 0.6 / 0.45 / 0.3 with a Gaussian bump of height 25 % and width 0.3 around (1, 1, 0.5)."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v0 = np.array([1.0, 1.0, 0.5]) / 1.5
    bump = 0.25 * np.exp(-((v - v0) ** 2).sum(1) / (2 * 0.3 ** 2))
    return torch.from_numpy((v * np.array(K.ELLIPSOID) * (1.0 + bump)[:, None]).astype(np.float32))


@dataclass
class Case:
    """An alignment case of tests/align_f64.py with the normals of its target."""
    base: A.Case
    normals: torch.Tensor             # (nt, 3) fp32
    rank: list = field(default_factory=list)       # per scene the rank the solve must keep (None: not stated)
    iters: int = 0
    truth: Optional[np.ndarray] = None


def _image(src, M):
    return A.apply(M[:3][None], src, [0, src.shape[0]])


def _case_generic(seed, n=4099, offset=0.0):
    tgt = A.bulged_ellipsoid(n, seed)
    nrm = target_normals(tgt, [0, n])
    tgt = tgt + offset
    src = _image(tgt, np.linalg.inv(SMALL))          # row i of the source goes with row i of the target
    return Case(base=A.Case(source=src, start=[0, n], target=tgt, tstart=[0, n], scale=False), normals=nrm, rank=[6])


def _case_plane(seed):
    """A target in the plane z = 0.25 with the exact normal: in-plane shifts and the rotation about the normal are not constrained."""
    g = torch.Generator().manual_seed(seed)
    n = 1500
    tgt = torch.cat([(torch.rand(n, 2, generator=g) * 2 - 1) * 0.6, torch.full((n, 1), 0.25)], dim=1)
    nrm = torch.tensor([[0.0, 0.0, 1.0]]).repeat(n, 1)
    src = _image(tgt, A.similarity(1.0, 2.0, (1, -2, 0.5), (0.02, -0.03, 0.01)))
    return Case(base=A.Case(source=src, start=[0, n], target=tgt, tstart=[0, n], scale=False), normals=nrm, rank=[3])


def _case_sphere(seed):
    """A target on the sphere about the origin with radial normals: the three rotations are not constrained."""
    n = 1500
    tgt = NN.sphere_points(n, seed)
    t64 = tgt.double()
    nrm = (t64 / t64.norm(dim=1, keepdim=True)).float()
    src = (tgt.double() * 1.01 + torch.tensor([0.01, -0.005, 0.002], dtype=torch.float64)).float()
    return Case(base=A.Case(source=src, start=[0, n], target=tgt, tstart=[0, n], scale=False), normals=nrm, rank=[3])


def _case_few_pairs(seed):
    lens = [0, 1, 2, 600]
    start = [0] + np.cumsum(lens).tolist()
    tgt = A.bulged_ellipsoid(start[-1], seed)
    nrm = torch.cat([torch.tensor([[0.0, 0.0, 1.0]]).repeat(3, 1), target_normals(tgt[3:], [0, 600])])
    src = _image(tgt, np.linalg.inv(SMALL))
    return Case(base=A.Case(source=src, start=start, target=tgt, tstart=start, scale=False), normals=nrm, rank=[0, 0, 0, 6])


def _case_gate(seed):
    """align_f64's gate case -- lattice distances, pairs exactly at the threshold -- with a unit normal per target."""
    base = A.make_case("gate")
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(base.nt, 3, generator=g, dtype=torch.float64)
    return Case(base=base, normals=(v / v.norm(dim=1, keepdim=True)).float(), rank=[6])


def _case_invalid_normals(seed):
    case = _case_generic(seed, n=1500)
    nrm = case.normals.clone()
    bad = [float("nan"), INF, -INF]
    for k in range(45):
        if k % 3 == 0:
            nrm[(k * 31) % 1500] = 0.0
        else:
            nrm[(k * 31) % 1500, k % 3] = bad[k % 3]
    return Case(base=case.base, normals=nrm, rank=[6])


def _case_nonfinite(seed):
    case = _case_generic(seed, n=1000)
    src, tgt = case.base.source.clone(), case.base.target.clone()
    bad = [float("nan"), INF, -INF]
    for k in range(30):
        src[(k * 37) % 1000, k % 3] = bad[k % 3]
        tgt[(k * 61 + 5) % 1000, (k + 1) % 3] = bad[(k + 1) % 3]
    return Case(base=A.Case(source=src, start=[0, 1000], target=tgt, tstart=[0, 1000], scale=False), normals=case.normals, rank=[6])


def _case_chunk_edges(seed):
    lens = [A.CHUNK - 1, A.CHUNK, A.CHUNK + 1, 2 * A.CHUNK + 1]
    start = [0] + np.cumsum(lens).tolist()
    tgt = A.bulged_ellipsoid(start[-1], seed)
    nrm = target_normals(tgt, start)
    moves = [np.linalg.inv(A.similarity(1.0, 1.0 + k, (1, k, 2 - k), (0.01 * k, -0.005, 0.002 * k))) for k in range(4)]
    src = A.apply(np.stack([m[:3] for m in moves]), tgt, start)
    return Case(base=A.Case(source=src, start=start, target=tgt, tstart=start, scale=False), normals=nrm, rank=[6] * 4)


def _case_icp_exact(seed):
    base = A.make_case("icp_rigid10")
    return Case(base=base, normals=target_normals(base.target, base.tstart), iters=30, truth=A.TRUTH_RIGID10)


def _case_icp_sliding(seed):
    """The case the feature exists for: two INDEPENDENT samplings of one smooth surface, the source moved by 8 degrees about (1, 2, 3)
    and by (0.03, -0.02, 0.01); no point of one side is a point of the other."""
    n = 2048
    tgt, other = bumped_ellipsoid(n, seed), bumped_ellipsoid(n, seed + 1)
    src = _image(other, np.linalg.inv(TRUTH_SLIDE))
    return Case(base=A.Case(source=src, start=[0, n], target=tgt, tstart=[0, n], scale=False, iters=30), normals=target_normals(tgt, [0, n]),
                iters=30, truth=TRUTH_SLIDE)


FIT_CASES = {
    "generic": (_case_generic, 0),
    "plane": (_case_plane, 1),
    "sphere": (_case_sphere, 2),
    "few_pairs": (_case_few_pairs, 3),
    "gate": (_case_gate, 4),
    "invalid_normals": (_case_invalid_normals, 5),
    "nonfinite": (_case_nonfinite, 6),
    "chunk_edges": (_case_chunk_edges, 7),
    "offset": (lambda seed: _case_generic(seed, offset=8.0), 0),
}
ICP_CASES = {"icp_exact": (_case_icp_exact, 8), "icp_sliding": (_case_icp_sliding, 9)}
CASES = {**FIT_CASES, **ICP_CASES}


@functools.lru_cache(maxsize=None)
def make_case(name):
    fn, seed = CASES[name]
    return fn(9100 + seed)


# ------------------------------------------------------------------------------------------------ the rule restated
def accepted_pairs(moved, case, index=None, dist2=None):
    """align_f64's pair rule and a finite non-zero normal at the target -> (accepted (n,) bool, j (n,) int64, d2 (n,) fp32)."""
    base = case.base
    index = base.index if index is None else index
    dist2 = base.dist2 if dist2 is None else dist2
    ok, j, d2 = A.accepted_pairs(moved, base.target, index, dist2, base.max_d2)
    nrm = case.normals[j.clamp(0, max(base.nt - 1, 0))]
    return ok & torch.isfinite(nrm).all(1) & (nrm != 0).any(1), j, d2


def plane_sums(moved, case, index=None, dist2=None):
    """(N, 30) float64: every addend formed as the rule forms it (float64 numpy ops, one rounding each), added exactly."""
    base = case.base
    ok, j, d2 = accepted_pairs(moved, case, index, dist2)
    sc = A.scene_of(base.start, moved.shape[0])
    out = np.zeros((base.nscene, SUMS))
    for s in range(base.nscene):
        rows = torch.from_numpy(sc == s) & ok
        p, q = moved[rows].numpy().astype(np.float64), base.target[j[rows]].numpy().astype(np.float64)
        n = case.normals[j[rows]].numpy().astype(np.float64)
        e = p - q
        r = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]
        c = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2], p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0]], axis=1)
        a = np.concatenate([c, n], axis=1)
        cols = [np.ones(len(p))] + [a[:, i] * a[:, k] for i in range(6) for k in range(i, 6)] + [a[:, i] * r for i in range(6)] + [r * r]
        out[s] = [math.fsum(col.tolist()) for col in cols] + [math.fsum(d2[rows].double().tolist())]
    return out


def unpack(sums):
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = sums[1:22]
    return H + np.triu(H, 1).T, sums[22:28]


def rotation(omega):
    """exp([omega]x) by Rodrigues in float64."""
    a = float(np.linalg.norm(omega))
    Kx = np.array([[0, -omega[2], omega[1]], [omega[2], 0, -omega[0]], [-omega[1], omega[0], 0]])
    if a < 1e-8:
        return np.eye(3) + Kx + 0.5 * Kx @ Kx
    return np.eye(3) + math.sin(a) / a * Kx + (1 - math.cos(a)) / (a * a) * Kx @ Kx


@dataclass
class Solve:
    R: np.ndarray
    t: np.ndarray
    rank: int
    lam: np.ndarray                   # the six eigenvalues, ascending (zeros where the rule returns the identity early)
    x: np.ndarray
    bound: float                      # on |D - D_library|_max for the SAME sums (solve_bound)


def solve_bound(lam, kept, g, n_rel=0.0):
    """The bound on the step for given sums (n_rel = 0), or for sums that differ by a relative n_rel in every entry:
        (128 + 16 n_rel / 2^-53) * 2^-53 * kappa * |g| / lambda_min_kept + 32 * 2^-53,      kappa = lambda_max / lambda_min_kept.
    x = -P (H|kept)^-1 P g.  A symmetric eigen solver is backward stable: it decomposes H + E with |E| <= ~16 * 2^-53 * lambda_max.  The
    inverse on the kept spectrum moves by |E| / lambda_min^2, the kept subspace turns by |E| / gap against the dropped one with
    gap >= (1 - 1 / CLEAR^2) lambda_min: together <= 2 |E| |g| / lambda_min^2 = 32 * 2^-53 * kappa * |g| / lambda_min per solver, two
    solvers, and a factor 2 from x to the entries of D = [exp(omega) | t]: 128.  Sums that differ by n_rel per entry are an |E| of
    6 n_rel lambda_max more (a 6 x 6 norm against its entries) and the same of g: 16 n_rel after the same factors.  The rotation's sin,
    cos, normalisation and nine products add a few 2^-53 on entries of magnitude <= 1: 32 * 2^-53.  An offset cloud needs no separate
    factor (align_f64.spread_factor): it raises kappa, which is in the bound."""
    if not kept.any():
        return 32 * 2.0 ** -53
    lmin, lmax = float(lam[kept].min()), float(lam.max())
    return (128 * 2.0 ** -53 + 16 * n_rel) * (lmax / lmin) * float(np.linalg.norm(g)) / lmin + 32 * 2.0 ** -53


def solve(sums, n_rel=0.0):
    """The solve of the rule with numpy.linalg.eigh."""
    ident = Solve(R=np.eye(3), t=np.zeros(3), rank=0, lam=np.zeros(6), x=np.zeros(6), bound=0.0)
    if not np.all(np.isfinite(sums)) or not sums[0] >= 3:
        return ident
    H, g = unpack(sums)
    lam, V = np.linalg.eigh(H)
    if not lam.max() > 0:
        return ident
    kept = lam > EPS_RANK * lam.max()
    x = -sum(V[:, i] * (V[:, i] @ g) / lam[i] for i in range(6) if kept[i])
    return Solve(R=rotation(x[:3]), t=x[3:].copy(), rank=int(kept.sum()), lam=lam, x=x, bound=solve_bound(lam, kept, g, n_rel))


def clearance(lam):
    """How far the eigenvalues stay from the rank threshold: min over i of max(lam_i / thr, thr / lam_i), thr = EPS_RANK * lambda_max
    (inf for an eigenvalue that is exactly 0 or negative by rounding)."""
    thr = EPS_RANK * lam.max()
    with np.errstate(divide="ignore"):
        return float(np.min(np.where(lam > thr, lam / thr, np.where(lam > 0, thr / np.where(lam > 0, lam, 1.0), np.inf))))


def step44(R, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    return M


def history_row(sums, rank):
    n = sums[0]
    nan = float("nan")
    return np.array([math.sqrt(sums[28] / n) if n > 0 else nan, n, math.sqrt(sums[29] / n) if n > 0 else nan, rank])


@dataclass
class FitRef:
    case: Case
    accepted: torch.Tensor
    sums: np.ndarray                  # (N, 30)
    solves: list                      # per scene a Solve
    rows: np.ndarray                  # (N, 4) history rows


@functools.lru_cache(maxsize=None)
def fit_refs(name):
    case = make_case(name)
    ok, _, _ = accepted_pairs(case.base.source, case)
    sums = plane_sums(case.base.source, case)
    n_rel = max(case.base.n, 1) * 2.0 ** -53
    solves = [solve(s, n_rel) for s in sums]
    return FitRef(case=case, accepted=ok, sums=sums, solves=solves, rows=np.stack([history_row(s, v.rank) for s, v in zip(sums, solves)]))


@dataclass
class IcpRef:
    case: Case
    matrix: np.ndarray                # (4, 4) after iters steps
    history: np.ndarray               # (iters + 1, 4)
    right: np.ndarray                 # (iters + 1,) correspondences equal to the permutation (-1 without one)
    index: torch.Tensor
    dist2: torch.Tensor
    moved: torch.Tensor
    worst_clearance: float


def icp(case, iters=None, init=None):
    """The loop of the rule on the brute-force restatement of the search, one scene."""
    base = case.base
    iters = case.iters if iters is None else iters
    m = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    rows, right, clear = [], [], INF
    qs, ts = torch.tensor(base.start), torch.tensor(base.tstart)
    for k in range(iters + 1):
        moved = A.apply(m[:3][None], base.source, base.start)
        index, dist2 = NN.nearest(NN.Case(query=moved, target=base.target, query_start=qs, target_start=ts))
        sums = plane_sums(moved, case, index, dist2)[0]
        sol = solve(sums)
        rows.append(history_row(sums, sol.rank))
        right.append(int((index == base.perm).sum()) if base.perm is not None else -1)
        clear = min(clear, clearance(sol.lam)) if sol.rank else clear
        if k < iters:
            m = step44(sol.R, sol.t) @ m
    return IcpRef(case=case, matrix=m, history=np.stack(rows), right=np.array(right), index=index, dist2=dist2, moved=moved, worst_clearance=clear)


@functools.lru_cache(maxsize=None)
def icp_refs(name):
    return icp(make_case(name))
