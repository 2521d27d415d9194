#!/usr/bin/env python
"""Nearest-point search (mvd_nearest_points, mvdfusion_amd/fusion.py nearest_points): the grid against the brute-force kernel and
against chunked torch.cdist + min on the GPU, the only thing a user had until now.

One workload = (point set, n) with nq = nt = n, one scene: `sphere` is a noisy sphere surface (radius 0.6, radial noise 0.005: what a
fused cloud looks like), `uniform` fills the +-0.75 box; queries and targets are two independent draws.  Defaults: both sets at n in
{4 096, 65 536, 1 048 576}.  One JSON line per workload:
  us_grid, us_grid_build, us_grid_query   MVD_NN_GRID: the whole call, and the two stages alone through mvd_nearest_points_stages
  us_brute              MVD_NN_BRUTE, up to --brute-max points (65 536); above, ONE untimed-warm-up-free call if the time extrapolated from
                        the largest timed size stays under --brute-once-s seconds (us_brute_once)
  us_torch_cdist        torch.cdist + min over query chunks of at most 2^26 distances, up to --brute-max points
  grid_over_brute       us_grid / us_brute (below 1: the grid wins)
  grid, method_auto     the cells per axis the library chose (--grid 0) or was given; what MVD_NN_AUTO resolves to at this size
  mismatch              queries whose GRID index or dist2 bits differ from BRUTE's after the timed calls (expected 0)
--sweep : instead, nq = nt in powers of two from 256 to 65 536 on the sphere set, GRID (whole call) and BRUTE side by side -- the
          crossover of MVD_NN_AUTO is the first size where GRID wins, rounded up to a power of two (csrc/nearest.hip: kGridMinTargets).
--grids G [G ...] : the workloads with these forced `grid` values next to the library's choice (kGridDivisor).
Every figure is the median over --blocks blocks of HIP-event times on torch's current stream, after a warm-up of every launch; a block
is `reps` calls between two events, reps chosen so that a block lasts about --block-ms.  min / max give the spread.

  python tools/bench_nearest.py
  python tools/bench_nearest.py --sweep
  python tools/bench_nearest.py --sets sphere --sizes 1048576 --grids 128 181 256

There is no CPU path: without a GPU this exits with an error.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _event_blocks(fn, blocks, block_ms):
    """Median / min / max µs per call of fn over `blocks` blocks of reps calls; reps from one timed call after the warm-up."""
    import torch
    for _ in range(2):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    reps = int(max(1, min(200, block_ms / max(a.elapsed_time(b), 1e-3))))
    times = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / reps)
    return dict(med=round(statistics.median(times), 2), min=round(min(times), 2), max=round(max(times), 2), reps=reps)


def points(kind, n, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    if kind == "uniform":
        return (torch.rand(n, 3, generator=g) * 2.0 - 1.0) * 0.75
    v = torch.randn(n, 3, generator=g, dtype=torch.float64)
    r = 0.6 + 0.005 * torch.randn(n, 1, generator=g, dtype=torch.float64)
    return (v / v.norm(dim=1, keepdim=True) * r).float()


def torch_cdist_min(q, t, chunk):
    import torch
    best, idx = [], []
    for a in range(0, q.shape[0], chunk):
        d, i = torch.cdist(q[a:a + chunk], t).min(dim=1)
        best.append(d)
        idx.append(i)
    return torch.cat(best), torch.cat(idx)


class Search:
    """One (query, target) pair on the GPU with its buffers; call(method, grid, stages) enqueues mvd_nearest_points_stages."""

    def __init__(self, kind, n):
        import torch
        from mvdfusion_amd import hip
        self.hip, self.L, self.n = hip, hip.lib(), n
        dev = "cuda"
        self.q, self.t = points(kind, n, 1).to(dev), points(kind, n, 2).to(dev)
        self.start = torch.tensor([0, n], dtype=torch.int32).to(dev)
        self.index = torch.empty(n, dtype=torch.int32, device=dev)
        self.dist2 = torch.empty(n, device=dev)
        self.nbytes = max(int(self.L.mvd_nearest_points_scratch(n, 1, hip.NN_GRID, g)) for g in (0, 1, 256))
        self.scratch = torch.empty(self.nbytes // 8 + 1, dtype=torch.int64, device=dev)

    def call(self, method, grid=0, stages=None):
        h = self.hip
        h.check(self.L.mvd_nearest_points_stages(h.ptr(self.q), h.ptr(self.start), h.ptr(self.t), h.ptr(self.start), self.n, self.n, 1, method,
                                                 grid, h.ptr(self.index), h.ptr(self.dist2), h.ptr(self.scratch), self.nbytes,
                                                 h.NN_ALL if stages is None else stages, h.stream()))

    def result(self, method, grid=0):
        import torch
        self.call(method, grid)
        torch.cuda.synchronize()
        return self.index.clone(), self.dist2.clone()


def library_grid(n):
    """The library's own choice of `grid` for n targets in one scene: csrc/nearest.hip's host rule round(sqrt(n / kGridDivisor)) in
    [1, 256], with the constant read from the source (the C ABI does not return it); checked against the scratch size the library asks for."""
    import math
    import re
    from mvdfusion_amd import hip
    src = open(os.path.join(ROOT, "mvdfusion_amd", "csrc", "nearest.hip")).read()
    div = float(re.search(r"kGridDivisor = ([0-9.]+)f;", src).group(1))
    g = int(min(max(math.floor(math.sqrt(n / div) + 0.5), 1), hip.NN_MAX_GRID))
    L = hip.lib()
    assert int(L.mvd_nearest_points_scratch(n, 1, hip.NN_GRID, 0)) == int(L.mvd_nearest_points_scratch(n, 1, hip.NN_GRID, g)), (n, g)
    return g


def run_one(kind, n, grid, a, brute_scale):
    import torch
    from mvdfusion_amd import hip
    s = Search(kind, n)
    L = s.L
    res = dict(metric="nearest_points", set=kind, n=n, grid=grid if grid else library_grid(n), grid_forced=bool(grid),
               method_auto="grid" if int(L.mvd_nearest_points_scratch(n, 1, hip.NN_AUTO, 0)) else "brute")
    t_all = _event_blocks(lambda: s.call(hip.NN_GRID, grid), a.blocks, a.block_ms)
    t_build = _event_blocks(lambda: s.call(hip.NN_GRID, grid, hip.NN_BUILD), a.blocks, a.block_ms)
    t_query = _event_blocks(lambda: s.call(hip.NN_GRID, grid, hip.NN_QUERY), a.blocks, a.block_ms)          # (the grid of the build above)
    for name, t in (("us_grid", t_all), ("us_grid_build", t_build), ("us_grid_query", t_query)):
        res.update({name: t["med"], name + "_min": t["min"], name + "_max": t["max"]})
    gi, gd = s.result(hip.NN_GRID, grid)
    res["mean_dist"] = round(float(gd.sqrt().double().mean()), 6)
    if n <= a.brute_max:
        t_brute = _event_blocks(lambda: s.call(hip.NN_BRUTE), a.blocks, a.block_ms)
        res.update(us_brute=t_brute["med"], us_brute_min=t_brute["min"], us_brute_max=t_brute["max"],
                   grid_over_brute=round(t_all["med"] / t_brute["med"], 4))
        bi, bd = s.result(hip.NN_BRUTE)
        res["mismatch"] = int(((bi != gi) | (bd.view(torch.int32) != gd.view(torch.int32))).sum())
        chunk = max(1, (1 << 26) // n)
        t_torch = _event_blocks(lambda: torch_cdist_min(s.q, s.t, chunk), a.blocks, a.block_ms)
        res.update(us_torch_cdist=t_torch["med"], us_torch_cdist_min=t_torch["min"], us_torch_cdist_max=t_torch["max"],
                   torch_over_grid=round(t_torch["med"] / t_all["med"], 1))
        brute_scale[kind] = (n, t_brute["med"])
    elif kind in brute_scale:
        n0, us0 = brute_scale[kind]
        guess = us0 * (n / n0) ** 2 * 1e-6
        res["brute_extrapolated_s"] = round(guess, 2)
        if guess <= a.brute_once_s:
            ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ea.record()
            s.call(hip.NN_BRUTE)
            eb.record()
            eb.synchronize()
            bi, bd = s.index.clone(), s.dist2.clone()
            res.update(us_brute_once=round(ea.elapsed_time(eb) * 1e3, 1), grid_over_brute=round(t_all["med"] / (ea.elapsed_time(eb) * 1e3), 6),
                       mismatch=int(((bi != gi) | (bd.view(torch.int32) != gd.view(torch.int32))).sum()))
    res.update(blocks=a.blocks, lib=os.path.basename(hip.LIB_PATHS[hip.OPERAND_FORMAT]), gpu=torch.cuda.get_device_name(0))
    return res


def sweep(a):
    import torch
    from mvdfusion_amd import hip
    first = None
    n = 256
    while n <= 65536:
        s = Search("sphere", n)
        tg = _event_blocks(lambda: s.call(hip.NN_GRID, 0), a.blocks, a.block_ms)
        tb = _event_blocks(lambda: s.call(hip.NN_BRUTE), a.blocks, a.block_ms)
        gi, gd = s.result(hip.NN_GRID)
        bi, bd = s.result(hip.NN_BRUTE)
        if first is None and tg["med"] < tb["med"]:
            first = n
        print(json.dumps(dict(metric="nearest_points_sweep", set="sphere", n=n, grid=library_grid(n), us_grid=tg["med"], us_grid_min=tg["min"],
                              us_grid_max=tg["max"], us_brute=tb["med"], us_brute_min=tb["min"], us_brute_max=tb["max"],
                              grid_over_brute=round(tg["med"] / tb["med"], 3),
                              mismatch=int(((bi != gi) | (bd.view(torch.int32) != gd.view(torch.int32))).sum()))), flush=True)
        n *= 2
    print(json.dumps(dict(metric="nearest_points_crossover", first_n_where_grid_wins=first, gpu=torch.cuda.get_device_name(0))), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sets", nargs="*", default=["sphere", "uniform"], choices=["sphere", "uniform"])
    ap.add_argument("--sizes", type=int, nargs="*", default=[4096, 65536, 1048576])
    ap.add_argument("--grids", type=int, nargs="*", default=[], help="forced grid values to time next to the library's choice")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--brute-max", type=int, default=65536)
    ap.add_argument("--brute-once-s", type=float, default=5.0)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-ms", type=float, default=100.0)
    a = ap.parse_args()
    if a.blocks < 3:
        ap.error("--blocks must be >= 3")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_nearest: no GPU visible (there is no CPU path)")
    if a.sweep:
        return sweep(a)
    brute_scale = {}
    for kind in a.sets:
        for n in sorted(a.sizes):
            for grid in [0] + list(a.grids):
                print(json.dumps(run_one(kind, n, grid, a, brute_scale)), flush=True)


if __name__ == "__main__":
    main()
