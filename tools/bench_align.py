#!/usr/bin/env python
"""Alignment (mvd_align_icp, mvdfusion_amd/fusion.py align_geometry): the ICP loop of the library against the same loop in torch ops, the
only thing a user had until now, and what a gate does to the result when the source carries outliers.

One workload = (point set, n) with nq = nt = n, one scene:
  sphere              the noisy sphere of tools/bench_nearest.py, two independent draws (timing only: a sphere has no pose to find)
  ellipsoid           the bulged ellipsoid of tests/align_f64.py against an independent resampling of itself, the source moved by the
                      inverse of (8 degrees about (0.3, -1, 0.5), t = (0.03, -0.015, 0.01)): no point has an exact partner
  ellipsoid_outliers  the same with 10 % of the source replaced by points uniform in the +-0.75 box
each without a gate and (the ellipsoids) with max_distance = 0.1.  Defaults: n in {4 096, 65 536, 1 048 576}, 30 iterations, rigid; the
outliers up to --outlier-max points (65 536): a point far from the target's surface makes the grid search walk many shells of empty
cells, a query of such a set takes 20 ms at 65 536 points and far longer at a million.
One JSON line per workload:
  us_icp, us_per_iter   the whole mvd_align_icp call (build, `iters` iterations, the last pass), and (us_icp - us_icp at iters = 0) / iters
  us_apply, us_query, us_fit    one mvd_align_apply, one MVD_NN_QUERY of mvd_nearest_points_stages and one mvd_align_fit (sums, solve and
                        composition) alone, all three on the state AFTER the 30 iterations: the source sits on the target as well as
                        it ever will, so their sum is the cost of a late iteration, not of the average one
  us_query_start        the same query on the source as given, before any iteration: what the first iteration pays
  us_build              MVD_NN_BUILD alone
  us_torch_icp          the same loop in torch ops: fusion.nearest_points + float64 torch.sum moments + torch.linalg.svd with its host
                        reads, up to --torch-max points (65 536)
  err, rms_first, rms_last, pairs_last   |matrix - truth|_max (ellipsoids), and the history's ends -- reported, nothing is asserted
Every time is the median over --blocks blocks of HIP-event times on torch's current stream, after a warm-up of every launch; a block
is `reps` calls between two events, reps chosen so that a block lasts about --block-ms.  min / max give the spread.

  python tools/bench_align.py
  python tools/bench_align.py --sets ellipsoid_outliers --sizes 65536 --iters 50

There is no CPU path: without a GPU this exits with an error.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_nearest import _event_blocks, points          # noqa: E402

GATE = 0.1


def ellipsoid(n, seed):
    """tests/align_f64.py: bulged_ellipsoid."""
    import torch
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, 3, generator=g, dtype=torch.float64)
    v = (v / v.norm(dim=1, keepdim=True)).float()
    bulge = ((v * torch.tensor([1.0, 1.0, 0.5])).sum(1) / 1.5 - 0.6).clamp(min=0.0)
    return (v * torch.tensor([0.6, 0.42, 0.25]) * (1.0 + 0.35 * bulge)[:, None]).contiguous()


def truth_matrix():
    import torch
    a = torch.tensor([0.3, -1.0, 0.5], dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    th = math.radians(8.0)
    M = torch.eye(4, dtype=torch.float64)
    M[:3, :3] = torch.eye(3, dtype=torch.float64) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    M[:3, 3] = torch.tensor([0.03, -0.015, 0.01], dtype=torch.float64)
    return M


def workload(kind, n):
    """(source, target, truth or None) on the CPU."""
    import torch
    if kind == "sphere":
        return points("sphere", n, 1), points("sphere", n, 2), None
    T = truth_matrix()
    inv = torch.linalg.inv(T)
    src = ellipsoid(n, 1)
    if kind == "ellipsoid_outliers":
        g = torch.Generator().manual_seed(3)
        rows = torch.randperm(n, generator=g)[:n // 10]
        src[rows] = (torch.rand(len(rows), 3, generator=g) * 2.0 - 1.0) * 0.75
    src = (src.double() @ inv[:3, :3].T + inv[:3, 3]).float()
    return src, ellipsoid(n, 2), T


class Icp:
    """One (source, target) pair on the GPU with its buffers; the entries of csrc/align.hip one by one."""

    def __init__(self, src, tgt, iters):
        import torch
        from mvdfusion_amd import hip
        self.hip, self.L, self.n, self.iters = hip, hip.lib(), int(src.shape[0]), iters
        dev = "cuda"
        self.src, self.tgt = src.to(dev), tgt.to(dev)
        self.start = torch.tensor([0, self.n], dtype=torch.int32).to(dev)
        self.moved = torch.empty_like(self.src)
        self.index = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.dist2 = torch.empty(self.n, device=dev)
        self.history = torch.empty(iters + 1, 1, hip.ALIGN_HISTORY, dtype=torch.float64, device=dev)
        self.identity = torch.eye(3, 4, dtype=torch.float64, device=dev).reshape(1, 12)
        self.transform = self.identity.clone()
        self.saved = self.identity.clone()
        self.nbytes = int(self.L.mvd_align_scratch(self.n, self.n, 1, hip.NN_AUTO, 0))
        self.scratch = torch.empty(self.nbytes // 8 + 1, dtype=torch.int64, device=dev)
        self.nn_bytes = int(self.L.mvd_nearest_points_scratch(self.n, 1, hip.NN_AUTO, 0))
        self.nn_scratch = torch.empty(self.nn_bytes // 8 + 1, dtype=torch.int64, device=dev)

    def icp(self, iters, max_d2):
        h = self.hip
        self.transform.copy_(self.identity)
        h.check(self.L.mvd_align_icp(h.ptr(self.src), h.ptr(self.start), h.ptr(self.tgt), h.ptr(self.start), self.n, self.n, 1, h.NN_AUTO, 0, iters,
                                     0, max_d2, h.ptr(self.transform), h.ptr(self.history), h.ptr(self.moved), h.ptr(self.index), h.ptr(self.dist2),
                                     h.ptr(self.scratch), self.nbytes, h.stream()))

    def apply(self):
        h = self.hip
        h.check(self.L.mvd_align_apply(h.ptr(self.src), h.ptr(self.start), self.n, 1, h.ptr(self.transform), h.ptr(self.moved), h.stream()))

    def search(self, stages):
        h = self.hip
        h.check(self.L.mvd_nearest_points_stages(h.ptr(self.moved), h.ptr(self.start), h.ptr(self.tgt), h.ptr(self.start), self.n, self.n, 1, h.NN_AUTO,
                                                 0, h.ptr(self.index), h.ptr(self.dist2), h.ptr(self.nn_scratch) if self.nn_bytes else None,
                                                 self.nn_bytes, stages, h.stream()))

    def fit(self, max_d2):
        """Sums, solve and composition, onto a transform restored first (a 96-byte device copy, inside the time)."""
        h = self.hip
        self.transform.copy_(self.saved)
        h.check(self.L.mvd_align_fit(h.ptr(self.moved), h.ptr(self.start), h.ptr(self.tgt), h.ptr(self.index), h.ptr(self.dist2), self.n, self.n, 1,
                                     0, max_d2, h.ptr(self.transform), h.ptr(self.history), h.ptr(self.scratch), self.nbytes, h.stream()))


def torch_icp(src, tgt, iters, max_d2):
    """The loop a user would write: the library's search, everything else torch ops, the reflection test read on the host."""
    import torch
    from mvdfusion_amd import fusion
    M = torch.eye(4, dtype=torch.float64, device=src.device)
    s64 = src.double()
    for _ in range(iters):
        moved = (s64 @ M[:3, :3].T + M[:3, 3]).float()
        nn = fusion.nearest_points(moved, tgt)
        ok = nn.hit & (nn.dist2 <= max_d2)
        p, q = moved[ok].double(), tgt[nn.index[ok].long()].double()
        mp, mq = p.mean(0), q.mean(0)
        U, _, Vt = torch.linalg.svd((q - mq).T @ (p - mp))
        D = torch.eye(3, dtype=torch.float64, device=src.device)
        if float(torch.linalg.det(U) * torch.linalg.det(Vt)) < 0:
            D[2, 2] = -1.0
        R = U @ D @ Vt
        step = torch.eye(4, dtype=torch.float64, device=src.device)
        step[:3, :3], step[:3, 3] = R, mq - R @ mp
        M = step @ M
    return M


def run_one(kind, n, gate, a):
    import torch
    from mvdfusion_amd import hip
    src, tgt, truth = workload(kind, n)
    s = Icp(src, tgt, a.iters)
    max_d2 = float(torch.tensor(gate, dtype=torch.float32) ** 2) if gate else float("inf")
    res = dict(metric="align_icp", set=kind, n=n, iters=a.iters, max_distance=gate,
               method_auto="grid" if int(s.L.mvd_nearest_points_scratch(n, 1, hip.NN_AUTO, 0)) else "brute")
    s.apply()          # the start: the source as it is
    s.search(hip.NN_BUILD)
    t_query0 = _event_blocks(lambda: s.search(hip.NN_QUERY), a.blocks, a.block_ms)
    t_icp = _event_blocks(lambda: s.icp(a.iters, max_d2), a.blocks, a.block_ms)
    t_zero = _event_blocks(lambda: s.icp(0, max_d2), a.blocks, a.block_ms)
    s.icp(a.iters, max_d2)
    torch.cuda.synchronize()
    hist = s.history.cpu()
    s.saved.copy_(s.transform)
    matrix = torch.cat([s.transform.reshape(3, 4).cpu(), torch.tensor([[0.0, 0, 0, 1]], dtype=torch.float64)])
    t_apply = _event_blocks(s.apply, a.blocks, a.block_ms)
    t_build = _event_blocks(lambda: s.search(hip.NN_BUILD), a.blocks, a.block_ms)
    t_query = _event_blocks(lambda: s.search(hip.NN_QUERY), a.blocks, a.block_ms)
    t_fit = _event_blocks(lambda: s.fit(max_d2), a.blocks, a.block_ms)
    for name, t in (("us_icp", t_icp), ("us_icp_iters0", t_zero), ("us_apply", t_apply), ("us_build", t_build), ("us_query", t_query), ("us_query_start", t_query0), ("us_fit", t_fit)):
        res.update({name: t["med"], name + "_min": t["min"], name + "_max": t["max"]})
    res["us_per_iter"] = round((t_icp["med"] - t_zero["med"]) / max(a.iters, 1), 2)
    res["us_apply_query_fit"] = round(t_apply["med"] + t_query["med"] + t_fit["med"], 2)
    res.update(rms_first=float(hist[0, 0, 0]), rms_last=float(hist[-1, 0, 0]), pairs_first=int(hist[0, 0, 1]), pairs_last=int(hist[-1, 0, 1]))
    if truth is not None:
        res["err"] = float((matrix - truth).abs().max())
    if n <= a.torch_max:
        t_torch = _event_blocks(lambda: torch_icp(s.src, s.tgt, a.iters, max_d2), a.blocks, a.block_ms)
        res.update(us_torch_icp=t_torch["med"], us_torch_icp_min=t_torch["min"], us_torch_icp_max=t_torch["max"],
                   torch_over_icp=round(t_torch["med"] / t_icp["med"], 2))
        if truth is not None:
            res["err_torch"] = float((torch_icp(s.src, s.tgt, a.iters, max_d2).cpu() - truth).abs().max())
    res.update(blocks=a.blocks, lib=os.path.basename(hip.LIB_PATHS[hip.OPERAND_FORMAT]), gpu=torch.cuda.get_device_name(0))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sets = ["sphere", "ellipsoid", "ellipsoid_outliers"]
    ap.add_argument("--sets", nargs="*", default=sets, choices=sets)
    ap.add_argument("--sizes", type=int, nargs="*", default=[4096, 65536, 1048576])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--torch-max", type=int, default=65536)
    ap.add_argument("--outlier-max", type=int, default=65536)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-ms", type=float, default=100.0)
    a = ap.parse_args()
    if a.blocks < 3:
        ap.error("--blocks must be >= 3")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_align: no GPU visible (there is no CPU path)")
    for kind in a.sets:
        for n in sorted(a.sizes):
            if kind == "ellipsoid_outliers" and n > a.outlier_max:
                continue
            for gate in ([None] if kind == "sphere" else [None, GATE]):
                print(json.dumps(run_one(kind, n, gate, a)), flush=True)


if __name__ == "__main__":
    main()
