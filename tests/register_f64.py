"""Test infrastructure of the global registration (include/mvd_hip.h: mvd_register_score, mvd_register_select; host:
fusion.register_geometry): the pose table and a float64 oracle that shares no method with the code under test.

  rotation_grid  the super-Fibonacci spiral restated (Alexa, "Super-Fibonacci Spirals", CVPR 2022) in numpy float64.
  row_costs      the per-row rule: align_f64.apply (the apply rule, bit for bit) + nearest_f64's brute force (the search's bits) + the
                 comparison with trunc2 in fp32.
  score          math.fsum of the fp32 costs: correctly rounded, no order.  inliers: a count.
  select         the greedy rule in numpy.
  register       the whole pipeline, one scene.  The H-hypothesis score of the sample and the K refinements are the expensive part (H *
                 samples * nt distances), so `register` forms them with a k-d tree (scipy.spatial.cKDTree: the exact float64 nearest
                 target within the truncation, the cost then evaluated in fp32 in the search's order) and with numpy sums -- a cost may
                 differ from row_costs' by an ulp of fp32 where two targets are within rounding of each other, which moves no selection
                 here (the tests print the score gaps).  The final polish of the winner is align_f64.icp itself.

The case is align_f64's bulged ellipsoid, n = 1 537, the target an exact permuted image of the source: truth and correspondences are
exact, as in icp_rigid10.  Every reference is computed once (functools.lru_cache)."""
import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

import align_f64 as AL
import nearest_f64 as NN

N_POINTS = 1537
DEFAULTS = dict(H=4096, samples=256, K=4, separation=30.0, refine_iters=20, iters=30)      # fusion.register_geometry's (test_cpu_register holds them equal)
GPU_POSES = (3, 14, 22, 26)       # the end-to-end batch of tests/test_gpu_register.py: 3 converges slowly, 14 and 22 a 1 024-rotation grid loses, 26 is a flip
PHI = math.sqrt(2.0)
PSI = 1.533751168755204288118041
INF = float("inf")


# ------------------------------------------------------------------------------------------------ rotations
def rotation_grid(H):
    """(H, 4) float64 unit quaternions (w, x, y, z): point i of the super-Fibonacci spiral with s = i + 1/2, t = s / H:
    (sqrt(t) sin(2 pi s / PHI), sqrt(t) cos(2 pi s / PHI), sqrt(1 - t) sin(2 pi s / PSI), sqrt(1 - t) cos(2 pi s / PSI))."""
    s = np.arange(H, dtype=np.float64) + 0.5
    t = s / float(H)
    r, R = np.sqrt(t), np.sqrt(1.0 - t)
    a, b = 2.0 * np.pi * s / PHI, 2.0 * np.pi * s / PSI
    return np.stack([r * np.sin(a), r * np.cos(a), R * np.sin(b), R * np.cos(b)], axis=1)


def quat_matrix(q):
    """(H, 4) (w, x, y, z) -> (H, 3, 3), the formula of the solve in the header."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)
    return R.reshape(-1, 3, 3)


def matrix_quat(R):
    """(3, 3) -> (4,) (w, x, y, z), through the symmetric eigenproblem (any rotation, 180 degrees included)."""
    R = np.asarray(R, dtype=np.float64)
    K = np.array([[R[0, 0] + R[1, 1] + R[2, 2], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]],
                  [0, R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]],
                  [0, 0, R[1, 1] - R[0, 0] - R[2, 2], R[1, 2] + R[2, 1]],
                  [0, 0, 0, R[2, 2] - R[0, 0] - R[1, 1]]])
    K = K + np.triu(K, 1).T
    return np.linalg.eigh(K)[1][:, -1]


def angle_between(qa, qb):
    """degrees of the relative rotation of unit quaternions (broadcast)."""
    return np.degrees(2.0 * np.arccos(np.clip(np.abs((qa * qb).sum(-1)), 0.0, 1.0)))


def covering_radius(H, trials=4000, seed=0):
    """The largest angle from `trials` random rotations to their nearest grid rotation, in degrees."""
    q = rotation_grid(H)
    g = np.random.default_rng(seed).normal(size=(trials, 4))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    return float(np.degrees(2.0 * np.arccos(np.clip(np.abs(g @ q.T).max(1), 0.0, 1.0))).max())


# ------------------------------------------------------------------------------------------------ the pose table
@functools.lru_cache(maxsize=None)
def pose_table():
    """24 poses from numpy.random.default_rng(5) -- axis normal, angle uniform in [40, 180] degrees, t uniform in +-0.3 -- and the
    three 180 degree flips about x, y, z (no translation): 27 (4, 4) float64 matrices."""
    rng = np.random.default_rng(5)
    out = []
    for _ in range(24):
        axis = rng.normal(size=3)
        angle = rng.uniform(40.0, 180.0)
        t = rng.uniform(-0.3, 0.3, size=3)
        out.append(AL.similarity(1.0, angle, axis, t))
    for axis in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        out.append(AL.similarity(1.0, 180.0, axis, (0.0, 0.0, 0.0)))
    return out


def pose_angle(k):
    R = pose_table()[k][:3, :3]
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(R) - 1.0) / 2.0))))


@functools.lru_cache(maxsize=None)
def pose_case(k):
    """Pose k of the table as an align_f64.Case: the bulged ellipsoid and its exact, permuted image."""
    return AL._icp_case(N_POINTS, pose_table()[k], 8200 + k, 0, False)


# ------------------------------------------------------------------------------------------------ the rule, per row
def row_costs(m, points, start, target, tstart, trunc2):
    """m (N, 3, 4) float64 -> (cost (n,) fp32, inlier (n,) bool, d2 (n,) fp32, in_scene (n,) bool): the rule of mvd_register_score."""
    moved = AL.apply(m, points, start)
    _, d2 = NN.nearest(NN.Case(query=moved, target=target, query_start=torch.tensor(start), target_start=torch.tensor(tstart)))
    t2 = torch.tensor(trunc2, dtype=torch.float32)
    inl = d2 <= t2                                        # (a NaN compares false; nearest gives +inf when nothing is found)
    cost = torch.where(inl, d2, t2)
    in_scene = torch.from_numpy(AL.scene_of(start, points.shape[0]) >= 0)
    return cost, inl & in_scene, d2, in_scene


def score(hyp, points, start, target, tstart, trunc2):
    """hyp (N, H, 12) float64 -> (score (N, H) float64, correctly rounded; inliers (N, H) int64)."""
    hyp = np.asarray(hyp, dtype=np.float64)
    N, H = hyp.shape[:2]
    sc = AL.scene_of(start, points.shape[0])
    out, cnt = np.zeros((N, H)), np.zeros((N, H), dtype=np.int64)
    for h in range(H):
        cost, inl, _, _ = row_costs(hyp[:, h].reshape(N, 3, 4), points, start, target, tstart, trunc2)
        for s in range(N):
            rows = torch.from_numpy(sc == s)
            out[s, h] = math.fsum(cost[rows].double().tolist())
            cnt[s, h] = int(inl[rows].sum())
    return out, cnt


def select(score_row, quat, cos_half, K):
    """The greedy rule for one scene -> (top (K,) int64, top_score (K,) float64)."""
    score_row, quat = np.asarray(score_row, dtype=np.float64), np.asarray(quat, dtype=np.float64)
    live = ~np.isnan(score_row)
    top, top_score = np.full(K, -1, dtype=np.int64), np.full(K, INF)
    for k in range(K):
        if not live.any():
            break
        cand = np.flatnonzero(live)
        h = int(cand[np.argmin(score_row[cand])])          # (argmin: the first of equal minima, the lowest h)
        top[k], top_score[k] = h, score_row[h]
        q = quat[h]
        dot = ((quat[:, 0] * q[0] + quat[:, 1] * q[1]) + quat[:, 2] * q[2]) + quat[:, 3] * q[3]      # (the rule's order: one rounding per op)
        live &= ~(np.abs(dot) >= cos_half)
        live[h] = False
    return top, top_score


# ------------------------------------------------------------------------------------------------ the pipeline
def centroid_stats(points):
    """(centroid (3,), mean squared radius) of the finite rows, float64."""
    p = points.double().numpy()
    p = p[np.isfinite(p).all(1)]
    c = p.mean(0)
    return c, float(((p - c) ** 2).sum(1).mean())


def hypotheses(R, source, target, scale=False):
    """R (H, 3, 3) -> (H, 3, 4): k R_h with the centroids matched, k the ratio of the RMS radii with `scale`."""
    (cs, rs), (ct, rt) = centroid_stats(source), centroid_stats(target)
    k = math.sqrt(rt / rs) if scale else 1.0
    A = k * np.asarray(R, dtype=np.float64)
    return np.concatenate([A, (ct[None] - A @ cs)[:, :, None]], axis=2)


def sample_rows(n, samples):
    return np.arange(0, n, -(-n // samples)) if n else np.zeros(0, dtype=np.int64)


def _apply_many(m, xyz):
    """m (H, 3, 4), xyz (n, 3) fp32 numpy -> (H, n, 3) fp32: the apply rule."""
    x = xyz.astype(np.float64)
    moved = ((m[:, None, :, 0] * x[None, :, None, 0] + m[:, None, :, 1] * x[None, :, None, 1]) + m[:, None, :, 2] * x[None, :, None, 2]) \
        + m[:, None, :, 3]
    return moved.astype(np.float32)


def _tree_costs(tree, target, moved, trunc2):
    """moved (..., 3) fp32 -> (cost fp32, inlier): the nearest target within the truncation by the tree, its d2 in fp32 in the search's order."""
    flat = moved.reshape(-1, 3)
    reach = math.sqrt(trunc2) * 1.001 + 1e-6
    _, j = tree.query(flat.astype(np.float64), distance_upper_bound=reach, workers=-1)
    found = j < target.shape[0]
    q = target[np.where(found, j, 0)]
    d = flat - q
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    t2 = np.float32(trunc2)
    inl = found & (d2 <= t2)
    return np.where(inl, d2, t2).reshape(moved.shape[:-1]), inl.reshape(moved.shape[:-1])


def _icp_tree(tree, src, tgt, m, iters):
    """Point-to-point ICP from the (4, 4) m, every pair accepted: tree correspondences, numpy float64 moments, the SVD solve."""
    tq = tgt.astype(np.float64)
    for _ in range(iters):
        p = _apply_many(m[None, :3], src)[0].astype(np.float64)
        q = tq[tree.query(p, workers=-1)[1]]
        n = float(len(p))
        sums = np.concatenate([[n], p.sum(0), q.sum(0), (p[:, :, None] * q[:, None, :]).sum(0).ravel(), [(p * p).sum(), (q * q).sum(), 0.0]])
        m = AL.step_matrix(*AL.solve_svd(sums, False)) @ m
    return m


@dataclass
class RegisterRef:
    matrix: np.ndarray                # (4, 4): the polished winner
    error: float                      # max |matrix - truth|
    right: int                        # final correspondences equal to the permutation
    grid_score: np.ndarray            # (H,)
    top: np.ndarray                   # (K,) grid rows refined
    candidates: np.ndarray            # (K, 4, 4) refined
    candidate_score: np.ndarray       # (K,)
    candidate_error: np.ndarray       # (K,) max |candidate - truth|
    chosen: int


def register(case, H, samples, K, separation=30.0, refine_iters=20, iters=30, trunc=None, polish=True):
    """The pipeline of fusion.register_geometry on one scene, rigid.  polish=False ends the winner with the tree ICP too (the sweep)."""
    from scipy.spatial import cKDTree
    quat = rotation_grid(H)
    src, tgt = case.source.numpy(), case.target.numpy()
    n = src.shape[0]
    _, rt = centroid_stats(case.target)
    trunc = 0.1 * math.sqrt(rt) if trunc is None else trunc
    t = np.float32(trunc)
    trunc2 = float(np.float32(t * t))
    hyp = hypotheses(quat_matrix(quat), case.source, case.target)
    tree = cKDTree(tgt.astype(np.float64))
    rows = sample_rows(n, samples)
    grid_score = np.zeros(H)
    for a in range(0, H, 512):
        cost, _ = _tree_costs(tree, tgt, _apply_many(hyp[a:a + 512], src[rows]), trunc2)
        grid_score[a:a + 512] = cost.astype(np.float64).sum(1)
    cos_half = math.cos(math.radians(separation) / 2.0) if separation > 0 else 2.0
    top, _ = select(grid_score, quat, cos_half, K)
    bottom = np.array([[0.0, 0.0, 0.0, 1.0]])
    cands = np.stack([_icp_tree(tree, src, tgt, np.concatenate([hyp[max(h, 0)], bottom]), refine_iters) for h in top])
    cost, _ = _tree_costs(tree, tgt, _apply_many(cands[:, :3], src), trunc2)
    cand_score = np.where(top >= 0, cost.astype(np.float64).sum(1), INF)
    chosen = int(select(cand_score, np.zeros((K, 4)), 2.0, 1)[0][0])
    truth = case.truth[0]
    if polish:
        ref = AL.icp(case, iters=iters, init=cands[chosen])
        matrix, right = ref.matrix, int(ref.right[-1])
    else:
        matrix = _icp_tree(tree, src, tgt, cands[chosen], iters)
        j = tree.query(_apply_many(matrix[None, :3], src)[0].astype(np.float64))[1]
        right = int((j == case.perm.numpy()).sum())
    return RegisterRef(matrix=matrix, error=float(np.abs(matrix - truth).max()), right=right, grid_score=grid_score, top=top, candidates=cands,
                       candidate_score=cand_score, candidate_error=np.abs(cands - truth[None]).reshape(K, -1).max(1), chosen=chosen)


@functools.lru_cache(maxsize=None)
def register_ref(k):
    """The oracle's pipeline on pose k at the defaults."""
    d = DEFAULTS
    return register(pose_case(k), d["H"], d["samples"], d["K"], separation=d["separation"], refine_iters=d["refine_iters"], iters=d["iters"])


@functools.lru_cache(maxsize=None)
def centroid_icp_error(k):
    """max |M - truth| of align_f64.icp from the centroid start (the identity rotation) on pose k, the default 30 iterations."""
    case = pose_case(k)
    start = np.concatenate([hypotheses(np.eye(3)[None], case.source, case.target)[0], [[0.0, 0.0, 0.0, 1.0]]])
    return float(np.abs(AL.icp(case, iters=DEFAULTS["iters"], init=start).matrix - case.truth[0]).max())


# ------------------------------------------------------------------------------------------------ the cases of the score
CHUNK = AL.CHUNK
TRUNC = 0.05


@dataclass
class ScoreCase:
    """The arguments of one mvd_register_score call as CPU data."""
    points: torch.Tensor              # (ns, 3) fp32
    start: list                       # nscene + 1 offsets
    target: torch.Tensor              # (nt, 3) fp32
    tstart: list
    hyp: np.ndarray                   # (nscene, H, 12) float64
    trunc2: float                     # an fp32 value

    @property
    def nscene(self):
        return len(self.start) - 1

    @property
    def H(self):
        return int(self.hyp.shape[1])


def fl32_square(v):
    v = np.float32(v)
    return float(np.float32(v * v))


def _hyps(truths, H, seed):
    """(N, H, 12): the scene's truth turned by 0, 2, 5, 15, 60, 170, .. degrees about a seeded axis and shifted a little: from every
    row an inlier to none."""
    rng = np.random.default_rng(seed)
    angles = (0.0, 2.0, 5.0, 15.0, 60.0, 170.0)
    out = np.zeros((len(truths), H, 12))
    for s, T in enumerate(truths):
        for h in range(H):
            P = AL.similarity(1.0, angles[h % 6], rng.normal(size=3), rng.uniform(-0.01, 0.01, size=3) * (h % 6 > 0))
            out[s, h] = (P @ T)[:3].ravel()
    return out


def _scenes_case(lens, tlens, H, seed):
    start, tstart = [0] + np.cumsum(lens).tolist(), [0] + np.cumsum(tlens).tolist()
    truths = [AL.similarity(1.0, 20.0 + 31 * k, (1, k, 2 - k), (0.1 * k - 0.2, -0.05, 0.02 * k)) for k in range(len(lens))]
    points = AL.bulged_ellipsoid(start[-1], seed)
    target = AL.apply(np.stack([t[:3] for t in truths]), AL.bulged_ellipsoid(tstart[-1], seed + 1), tstart)      # another sample of the surface
    return ScoreCase(points=points, start=start, target=target, tstart=tstart, hyp=_hyps(truths, H, seed + 2), trunc2=fl32_square(TRUNC))


def _case_lattice(seed):
    """mvd_align's gate case as a score: 40 targets on multiples of 1/8, 1 200 rows on multiples of 1/16, hypotheses that shift by
    multiples of 1/16 -- every product and sum of the apply is exact, every d2 an exact multiple of 1/256, and trunc2 = 9/256 is a
    value that occurs: the comparison is <=."""
    g = torch.Generator().manual_seed(seed)
    tgt = torch.randint(0, 9, (40, 3), generator=g).float() * 0.125 - 0.5
    src = torch.randint(0, 17, (1200, 3), generator=g).float() * 0.0625 - 0.5
    hyp = np.stack([AL.similarity(1.0, 0.0, (0, 0, 1), t)[:3].ravel() for t in ((0, 0, 0), (0.0625, 0, 0), (0, -0.125, 0.0625))])[None]
    return ScoreCase(points=src.contiguous(), start=[0, 1200], target=tgt.contiguous(), tstart=[0, 40], hyp=hyp, trunc2=fl32_square(0.1875))


def _case_far(seed):
    """Hypotheses that throw the cloud 10 box sizes (10 x 1.5) away: no row has a target within the truncation."""
    case = _scenes_case([700, 1500], [600, 1300], 3, seed)
    for s in range(2):
        for h, t in enumerate(((15.0, 0, 0), (0, -15.0, 0), (15.0, 15.0, 15.0))):
            case.hyp[s, h] = AL.similarity(1.0, 30.0 * h, (1, 1, 0), t)[:3].ravel()
    return case


def _case_nonfinite(seed, start=None, tstart=None):
    base = AL._case_nonfinite(seed)
    return ScoreCase(points=base.source, start=start or base.start, target=base.target, tstart=tstart or base.tstart,
                     hyp=_hyps([base.truth[0]], 3, seed), trunc2=fl32_square(TRUNC))


SCORE_CASES = {
    "chunk_edges": lambda: _scenes_case([0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1], [400, 0, 400, 400, 400, 400], 3, 8300),
    "many_hypotheses": lambda: _scenes_case([0, 1, 700], [50, 0, 600], 65, 8310),
    "lattice": lambda: _case_lattice(8320),
    "far": lambda: _case_far(8330),
    "nonfinite": lambda: _case_nonfinite(8340),
    "rows_of_no_scene": lambda: _case_nonfinite(8340, [37, 911], [5, 990]),
}


@functools.lru_cache(maxsize=None)
def score_case(name):
    return SCORE_CASES[name]()


@functools.lru_cache(maxsize=None)
def score_ref(name):
    """(score (N, H) float64, inliers (N, H) int64) of the oracle."""
    c = score_case(name)
    return score(c.hyp, c.points, c.start, c.target, c.tstart, c.trunc2)
