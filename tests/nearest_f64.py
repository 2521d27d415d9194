"""Test infrastructure of the nearest-point search (include/mvd_hip.h: mvd_nearest_points): the case table, an fp32 restatement of the
rule in plain CPU torch ops, and a float64 brute force.

The restatement forms d2 with elementwise sub, mul and add in the rule's order -- every torch op rounds once, there is no contraction --
and takes the minimum with the lowest index between equal minima, chunked over the queries.  It reproduces the rule bit for bit without
being the code under test.  The float64 brute force is the oracle of the two derived bounds (tests/test_gpu_nearest.py).

Shapes are a few thousand points: each reference takes well under a second and is computed once (functools.lru_cache)."""
import functools
from dataclasses import dataclass

import torch

EPS = 2.0 ** -23
SPHERE_R = 0.6
BOX = 0.75


@dataclass
class Case:
    """The arguments of one mvd_nearest_points call as CPU tensors."""
    query: torch.Tensor               # (nq, 3) fp32
    target: torch.Tensor              # (nt, 3) fp32
    query_start: torch.Tensor         # (nscene + 1,) int64
    target_start: torch.Tensor        # (nscene + 1,) int64

    @property
    def nq(self):
        return int(self.query.shape[0])

    @property
    def nt(self):
        return int(self.target.shape[0])

    @property
    def nscene(self):
        return int(self.query_start.numel()) - 1


def _one(query, target):
    return Case(query=query.float().contiguous(), target=target.float().contiguous(), query_start=torch.tensor([0, query.shape[0]]),
                target_start=torch.tensor([0, target.shape[0]]))


def _uniform(g, n):
    return (torch.rand(n, 3, generator=g) * 2.0 - 1.0) * BOX


def _lattice(g, n):
    """n points on {-0.5, -0.375, ..., 0.5}^3 (729 sites: dyadic coordinates, every difference and square exact in fp32)."""
    return torch.randint(0, 9, (n, 3), generator=g).float() * 0.125 - 0.5


def _case_random(g):
    return _one(_uniform(g, 1000), _uniform(g, 1537))


def _case_tile_edge(g):
    return _one(_uniform(g, 64), _uniform(g, 5000))


def _case_three_scenes(g):
    nt, nq = (0, 1, 700), (50, 0, 333)
    off = lambda c: torch.tensor([0, c[0], c[0] + c[1], sum(c)])
    return Case(query=_uniform(g, sum(nq)), target=_uniform(g, sum(nt)), query_start=off(nq), target_start=off(nt))


def _case_duplicates(g):
    return _one(_lattice(g, 1000), _lattice(g, 4097))


def _case_half_lattice(g):
    """Queries at the centres of the lattice's cells; the targets are every site twice over in a shuffled order, so the eight corners
    of a query's cell are exactly equidistant (3 * 0.0625^2) and each occurs twice."""
    sites = torch.stack(torch.meshgrid(*[torch.arange(9)] * 3, indexing="ij"), dim=-1).reshape(-1, 3).float() * 0.125 - 0.5
    target = torch.cat([sites, sites])[torch.randperm(2 * 729, generator=g)]
    query = torch.randint(0, 8, (500, 3), generator=g).float() * 0.125 - 0.4375
    return _one(query, target)


def _case_far_and_hollow(g):
    v = torch.randn(500, 3, generator=g, dtype=torch.float64)
    target = (v / v.norm(dim=1, keepdim=True) * SPHERE_R).float()
    dirs = torch.tensor([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], dtype=torch.float32)
    query = torch.cat([torch.zeros(1, 3), dirs * (10 * 2 * SPHERE_R), _uniform(g, 36) * 0.05])          # the centre, 10 box sizes out, near the centre
    return _one(query, target)


def _degenerate_queries(g, target):
    return torch.cat([target[:8], _uniform(g, 120), target[:4] + torch.tensor([0.0, 0.0, 0.25])])


def _case_coincident(g):
    target = torch.tensor([[0.25, -0.125, 0.5]]).repeat(300, 1)
    return _one(_degenerate_queries(g, target), target)


def _case_plane(g):
    target = _uniform(g, 300)
    target[:, 2] = 0.3
    return _one(_degenerate_queries(g, target), target)


def _case_line(g):
    s = (torch.rand(300, generator=g) * 2.0 - 1.0) * BOX
    target = torch.stack([s, 0.5 * s, -s], dim=1)
    return _one(_degenerate_queries(g, target), target)


def _case_nonfinite(g):
    case = _case_random(g)
    bad = [float("nan"), float("inf"), float("-inf")]
    for k in range(60):
        case.query[(k * 37) % case.nq, k % 3] = bad[k % 3]
        case.target[(k * 61) % case.nt, (k + 1) % 3] = bad[(k + 1) % 3]
    return case


CASES = {
    "random": (_case_random, 0),
    "tile_edge": (_case_tile_edge, 1),
    "three_scenes": (_case_three_scenes, 2),
    "duplicates": (_case_duplicates, 3),
    "half_lattice": (_case_half_lattice, 4),
    "far_and_hollow": (_case_far_and_hollow, 5),
    "degenerate_coincident": (_case_coincident, 6),
    "degenerate_plane": (_case_plane, 7),
    "degenerate_line": (_case_line, 8),
    "nonfinite": (_case_nonfinite, 9),
}


@functools.lru_cache(maxsize=None)
def make_case(name):
    fn, seed = CASES[name]
    return fn(torch.Generator().manual_seed(7300 + seed))


def _scene_of(start, n):
    """(n,) scene of every row (the number of scenes when it is in none), from the offsets."""
    i = torch.arange(n)
    s = torch.searchsorted(start[1:].contiguous(), i, right=True)
    return torch.where(i >= start[0], s, torch.full_like(s, start.numel() - 1))


def _d2(q, t, dtype):
    """(nq, nt) squared distances in the rule's order; in fp32 every op rounds once."""
    q, t = q.to(dtype), t.to(dtype)
    d = [q[:, None, k] - t[None, :, k] for k in range(3)]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def nearest(case, dtype=torch.float32, chunk=256):
    """The rule restated -> (index (nq,) int64, dist2 (nq,) `dtype`).  A candidate is a target of the query's scene; a d2 that is not
    < +inf (NaN, +inf) never wins; between equal minima the lowest index wins."""
    nq, nt, N = case.nq, case.nt, case.nscene
    index = torch.full((nq,), -1, dtype=torch.int64)
    dist2 = torch.full((nq,), float("inf"), dtype=dtype)
    if nq == 0 or nt == 0:
        return index, dist2
    qs, ts = _scene_of(case.query_start, nq), _scene_of(case.target_start, nt)
    inf = torch.tensor(float("inf"), dtype=dtype)
    rows = torch.arange(nt)
    for a in range(0, nq, chunk):
        b = min(a + chunk, nq)
        d2 = _d2(case.query[a:b], case.target, dtype)
        ok = (d2 < inf) & (qs[a:b, None] == ts[None, :]) & (qs[a:b, None] < N)
        d2 = torch.where(ok, d2, inf)
        m = d2.min(dim=1).values
        first = torch.where(d2 == m[:, None], rows[None, :], torch.full((1, 1), nt)).min(dim=1).values
        won = m < inf
        index[a:b] = torch.where(won, first, torch.full_like(first, -1))
        dist2[a:b] = m
    return index, dist2


@dataclass
class Ref:
    case: Case
    index: torch.Tensor               # fp32 restatement: what the kernels must give, bit for bit
    dist2: torch.Tensor
    index64: torch.Tensor             # float64 brute force
    dist2_64: torch.Tensor
    at_winner64: torch.Tensor         # float64 d2 between each query and the fp32 restatement's winner (+inf without one)
    finite: torch.Tensor              # (nq,) the queries the float64 bounds are stated on: finite, with a winner


@functools.lru_cache(maxsize=None)
def refs(name):
    case = make_case(name)
    index, dist2 = nearest(case, torch.float32)
    index64, dist2_64 = nearest(case, torch.float64)
    return Ref(case=case, index=index, dist2=dist2, index64=index64, dist2_64=dist2_64, at_winner64=d2_at(case, index),
               finite=torch.isfinite(case.query).all(1) & (index64 >= 0))


def d2_at(case, index):
    """float64 d2 between query i and target index[i] (+inf where index is -1)."""
    t = case.target[index.clamp(min=0).long()].double()
    q = case.query.double()
    d = q - t
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return torch.where(index >= 0, d2, torch.full_like(d2, float("inf")))


def float64_bounds(ref, index, dist2):
    """The two derived bounds of a result against float64, on ref.finite:
        |dist2 - min_j d2_64| <= 3 * 2^-23 * min_j d2_64      and      d2_64(i, index[i]) <= (1 + 6 * 2^-23) * min_j d2_64.
    The rule is five roundings of relative error 2^-24 each (a subtraction and a square per axis, two additions: every term passes at
    most five): 2.5 * 2^-23, and the fp32 minimum can sit that far on either side.  Returns (both hold everywhere, the worst of the two
    left-hand sides relative to min_j d2_64 in units of 2^-23 -- over the queries with a non-zero minimum; a zero minimum must be met
    exactly, which the two inequalities say themselves)."""
    keep = ref.finite
    m, got, at = ref.dist2_64[keep], dist2.double()[keep], d2_at(ref.case, index)[keep]
    ok = bool(((got - m).abs() <= 3 * EPS * m).all()) and bool((at <= (1 + 6 * EPS) * m).all())
    pos = m > 0
    worst = lambda e: float(e.max()) / EPS if e.numel() else 0.0
    return ok, worst((got - m).abs()[pos] / m[pos]), worst((at - m)[pos] / m[pos])


def sphere_points(n, seed, noise=0.0):
    """n points on the sphere of radius SPHERE_R with radial noise of that standard deviation (tools/bench_nearest.py's point set too)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, 3, generator=g, dtype=torch.float64)
    r = SPHERE_R + noise * torch.randn(n, 1, generator=g, dtype=torch.float64)
    return (v / v.norm(dim=1, keepdim=True) * r).float()

