#!/usr/bin/env python
"""Neighbourhoods and point-to-plane ICP (mvd_knn_points, mvd_point_normals, mvd_plane_icp; mvdfusion_amd/fusion.py knn_points,
estimate_normals, align_to_surface) against the same work in torch ops, and point-to-plane against point-to-point on the sets of
tools/bench_align.py.

One workload = (set, n) with nq = nt = n, one scene; sets `ellipsoid` and `ellipsoid_outliers` of tools/bench_align.py (two independent
samplings of the bulged ellipsoid, the source moved by the inverse of 8 degrees about (0.3, -1, 0.5) and (0.03, -0.015, 0.01); the
outliers up to --outlier-max points).  One JSON line per workload:
  us_knn_k{1,8,16,32}   mvd_knn_points of the target against itself, MVD_NN_AUTO (build and query)
  us_knn_build, us_knn_query_k16   MVD_NN_BUILD alone, and MVD_NN_QUERY alone at k = 16
  us_knn_brute_k16      MVD_NN_BRUTE at k = 16, up to --brute-max points (65 536)
  us_normals            mvd_point_normals on the k = 16 lists
  us_icp, us_per_iter   the whole mvd_plane_icp call (`iters` iterations and the last pass) on given normals, and
                        (us_icp - us_icp at iters = 0) / iters
  us_apply, us_query, us_fit   one mvd_align_apply, one MVD_NN_QUERY of mvd_nearest_points_stages and one mvd_plane_fit alone, on the
                        state after the iterations
  us_torch_knn_k16, us_torch_eigh, us_torch_icp   the same in torch ops up to --torch-max points (65 536): torch.cdist + topk in
                        chunks of 4 096 queries; centred covariance + torch.linalg.eigh (float64); a loop of apply, the library's
                        nearest_points and torch.linalg.lstsq on the n x 6 system (float64)
  err_point, err_plane, err_recipe   |matrix - truth|_max after `iters` iterations of align_geometry, of align_to_surface, and of
                        align_to_surface started from 5 iterations of align_geometry; the gate of tools/bench_align.py (0.1) on the
                        outlier set, none otherwise -- reported, nothing is asserted
Every time is the median over --blocks blocks of HIP-event times on torch's current stream, after a warm-up of every launch
(tools/bench_nearest.py: _event_blocks); min / max give the spread.

  python tools/bench_plane.py
  python tools/bench_plane.py --sets ellipsoid --sizes 65536 --iters 10

There is no CPU path: without a GPU this exits with an error.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_align import GATE, workload          # noqa: E402
from bench_nearest import _event_blocks         # noqa: E402

KS = (1, 8, 16, 32)


class Plane:
    """One (source, target) pair on the GPU with its buffers; the entries one by one."""

    def __init__(self, src, tgt, iters):
        import torch
        from mvdfusion_amd import hip
        self.hip, self.L, self.n, self.iters = hip, hip.lib(), int(src.shape[0]), iters
        dev = "cuda"
        n = self.n
        self.src, self.tgt = src.to(dev), tgt.to(dev)
        self.start = torch.tensor([0, n], dtype=torch.int32).to(dev)
        self.knn_index = torch.empty(n, 32, dtype=torch.int32, device=dev)
        self.knn_dist2 = torch.empty(n, 32, device=dev)
        self.normal = torch.empty(n, 3, device=dev)
        self.variation = torch.empty(n, device=dev)
        self.moved = torch.empty_like(self.src)
        self.index = torch.empty(n, dtype=torch.int32, device=dev)
        self.dist2 = torch.empty(n, device=dev)
        self.history = torch.empty(iters + 1, 1, hip.PLANE_HISTORY, dtype=torch.float64, device=dev)
        self.identity = torch.eye(3, 4, dtype=torch.float64, device=dev).reshape(1, 12)
        self.transform, self.saved = self.identity.clone(), self.identity.clone()
        self.nbytes = int(self.L.mvd_plane_scratch(n, n, 1, hip.NN_AUTO, 0))
        self.scratch = torch.empty(self.nbytes // 8 + 1, dtype=torch.int64, device=dev)
        self.nn_bytes = int(self.L.mvd_nearest_points_scratch(n, 1, hip.NN_AUTO, 0))
        self.nn_scratch = torch.empty(self.nn_bytes // 8 + 1, dtype=torch.int64, device=dev)

    def knn(self, k, method, stages):
        h = self.hip
        sc = h.ptr(self.nn_scratch) if self.nn_bytes and method != h.NN_BRUTE else None
        h.check(self.L.mvd_knn_points_stages(h.ptr(self.tgt), h.ptr(self.start), h.ptr(self.tgt), h.ptr(self.start), self.n, self.n, 1, k, method, 0,
                                             h.ptr(self.knn_index), h.ptr(self.knn_dist2), sc, self.nn_bytes if sc else 0, stages, h.stream()))

    def normals(self, k):
        h = self.hip
        h.check(self.L.mvd_point_normals(h.ptr(self.tgt), self.n, h.ptr(self.knn_index), self.n, k, None, None, h.ptr(self.normal),
                                         h.ptr(self.variation), h.stream()))

    def icp(self, iters, max_d2):
        h = self.hip
        self.transform.copy_(self.identity)
        h.check(self.L.mvd_plane_icp(h.ptr(self.src), h.ptr(self.start), h.ptr(self.tgt), h.ptr(self.start), h.ptr(self.normal), self.n, self.n, 1,
                                     h.NN_AUTO, 0, iters, max_d2, h.ptr(self.transform), h.ptr(self.history), h.ptr(self.moved), h.ptr(self.index),
                                     h.ptr(self.dist2), h.ptr(self.scratch), self.nbytes, h.stream()))

    def apply(self):
        h = self.hip
        h.check(self.L.mvd_align_apply(h.ptr(self.src), h.ptr(self.start), self.n, 1, h.ptr(self.transform), h.ptr(self.moved), h.stream()))

    def search(self, stages):
        h = self.hip
        h.check(self.L.mvd_nearest_points_stages(h.ptr(self.moved), h.ptr(self.start), h.ptr(self.tgt), h.ptr(self.start), self.n, self.n, 1, h.NN_AUTO,
                                                 0, h.ptr(self.index), h.ptr(self.dist2), h.ptr(self.nn_scratch) if self.nn_bytes else None,
                                                 self.nn_bytes, stages, h.stream()))

    def fit(self, max_d2):
        h = self.hip
        self.transform.copy_(self.saved)
        h.check(self.L.mvd_plane_fit(h.ptr(self.moved), h.ptr(self.start), h.ptr(self.tgt), h.ptr(self.normal), h.ptr(self.index), h.ptr(self.dist2),
                                     self.n, self.n, 1, 0, max_d2, h.ptr(self.transform), h.ptr(self.history), h.ptr(self.scratch), self.nbytes,
                                     h.stream()))


def torch_knn(points, k, chunk=4096):
    import torch
    out = []
    for a in range(0, points.shape[0], chunk):
        out.append(torch.cdist(points[a:a + chunk], points).topk(k, dim=1, largest=False).indices)
    return torch.cat(out)


def torch_normals(points, index):
    import torch
    x = points[index.long()].double()
    d = x - x.mean(1, keepdim=True)
    return torch.linalg.eigh(d.transpose(1, 2) @ d)[1][:, :, 0]


def torch_icp(src, tgt, normals, iters, max_d2):
    """The loop a user would write: the library's search, the n x 6 system through torch.linalg.lstsq in float64."""
    import torch
    from mvdfusion_amd import fusion
    M = torch.eye(4, dtype=torch.float64, device=src.device)
    s64, n64 = src.double(), normals.double()
    for _ in range(iters):
        p = s64 @ M[:3, :3].T + M[:3, 3]
        nn = fusion.nearest_points(p.float(), tgt)
        ok = (nn.hit & (nn.dist2 <= max_d2)).double()[:, None]
        j = nn.index.long().clamp(min=0)
        q, n = tgt[j].double(), n64[j]
        A = torch.cat([torch.linalg.cross(p, n), n], dim=1) * ok
        r = ((p - q) * n).sum(1, keepdim=True) * ok
        x = torch.linalg.lstsq(A, -r).solution[:, 0]
        K = torch.zeros(3, 3, dtype=torch.float64, device=src.device)
        K[0, 1], K[0, 2], K[1, 0], K[1, 2], K[2, 0], K[2, 1] = -x[2], x[1], x[2], -x[0], -x[1], x[0]
        step = torch.eye(4, dtype=torch.float64, device=src.device)
        step[:3, :3], step[:3, 3] = torch.linalg.matrix_exp(K), x[3:]
        M = step @ M
    return M


def run_one(kind, n, a):
    import torch
    from mvdfusion_amd import fusion, hip
    src, tgt, truth = workload(kind, n)
    gate = GATE if kind == "ellipsoid_outliers" else None
    max_d2 = float(torch.tensor(gate, dtype=torch.float32) ** 2) if gate else float("inf")
    s = Plane(src, tgt, a.iters)
    blocks = lambda fn: _event_blocks(fn, a.blocks, a.block_ms)
    res = dict(metric="plane_icp", set=kind, n=n, iters=a.iters, max_distance=gate,
               method_auto="grid" if s.nn_bytes else "brute")
    times = {}
    for k in KS:
        times[f"us_knn_k{k}"] = blocks(lambda: s.knn(k, hip.NN_AUTO, hip.NN_ALL))
    times["us_knn_build"] = blocks(lambda: s.knn(16, hip.NN_AUTO, hip.NN_BUILD))
    times["us_knn_query_k16"] = blocks(lambda: s.knn(16, hip.NN_AUTO, hip.NN_QUERY))
    if n <= a.brute_max:
        times["us_knn_brute_k16"] = blocks(lambda: s.knn(16, hip.NN_BRUTE, hip.NN_ALL))
    s.knn(16, hip.NN_AUTO, hip.NN_ALL)
    times["us_normals"] = blocks(lambda: s.normals(16))
    s.normals(16)
    times["us_icp"] = blocks(lambda: s.icp(a.iters, max_d2))
    times["us_icp_iters0"] = blocks(lambda: s.icp(0, max_d2))
    s.icp(a.iters, max_d2)
    torch.cuda.synchronize()
    hist = s.history.cpu()
    s.saved.copy_(s.transform)
    times["us_apply"] = blocks(s.apply)
    times["us_query"] = blocks(lambda: s.search(hip.NN_QUERY))
    times["us_fit"] = blocks(lambda: s.fit(max_d2))
    for name, t in times.items():
        res.update({name: t["med"], name + "_min": t["min"], name + "_max": t["max"]})
    res["us_per_iter"] = round((times["us_icp"]["med"] - times["us_icp_iters0"]["med"]) / max(a.iters, 1), 2)
    res.update(plane_rms_first=float(hist[0, 0, 0]), plane_rms_last=float(hist[-1, 0, 0]), rms_last=float(hist[-1, 0, 2]), pairs_last=int(hist[-1, 0, 1]),
               rank_last=int(hist[-1, 0, 3]))
    err = lambda al: float((al.matrix[0].cpu() - truth).abs().max())
    point = fusion.align_geometry(s.src, s.tgt, iters=a.iters, max_distance=gate)
    plane = fusion.align_to_surface(s.src, s.tgt, normals=s.normal, iters=a.iters, max_distance=gate)
    recipe = fusion.align_to_surface(s.src, s.tgt, normals=s.normal, iters=a.iters, max_distance=gate,
                                     init=fusion.align_geometry(s.src, s.tgt, iters=5, max_distance=gate))
    res.update(err_point=err(point), err_plane=err(plane), err_recipe=err(recipe))
    if n <= a.torch_max:
        t = blocks(lambda: torch_knn(s.tgt, 16))
        res.update(us_torch_knn_k16=t["med"], us_torch_knn_k16_min=t["min"], us_torch_knn_k16_max=t["max"],
                   torch_over_knn=round(t["med"] / times["us_knn_k16"]["med"], 2))
        t = blocks(lambda: torch_normals(s.tgt, s.knn_index[:, :16]))
        res.update(us_torch_eigh=t["med"], us_torch_eigh_min=t["min"], us_torch_eigh_max=t["max"], torch_over_normals=round(t["med"] / times["us_normals"]["med"], 2))
        t = blocks(lambda: torch_icp(s.src, s.tgt, s.normal, a.iters, max_d2))
        res.update(us_torch_icp=t["med"], us_torch_icp_min=t["min"], us_torch_icp_max=t["max"], torch_over_icp=round(t["med"] / times["us_icp"]["med"], 2),
                   err_torch=float((torch_icp(s.src, s.tgt, s.normal, a.iters, max_d2).cpu() - truth).abs().max()))
    res.update(blocks=a.blocks, lib=os.path.basename(hip.LIB_PATHS[hip.OPERAND_FORMAT]), gpu=torch.cuda.get_device_name(0))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sets = ["ellipsoid", "ellipsoid_outliers"]
    ap.add_argument("--sets", nargs="*", default=sets, choices=sets)
    ap.add_argument("--sizes", type=int, nargs="*", default=[4096, 65536, 1048576])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--torch-max", type=int, default=65536)
    ap.add_argument("--brute-max", type=int, default=65536)
    ap.add_argument("--outlier-max", type=int, default=65536)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-ms", type=float, default=100.0)
    a = ap.parse_args()
    if a.blocks < 3:
        ap.error("--blocks must be >= 3")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_plane: no GPU visible (there is no CPU path)")
    for kind in a.sets:
        for n in sorted(a.sizes):
            if kind == "ellipsoid_outliers" and n > a.outlier_max:
                continue
            print(json.dumps(run_one(kind, n, a)), flush=True)


if __name__ == "__main__":
    main()
