#!/usr/bin/env python
"""The exact point-to-mesh distance (mvd_nearest_on_mesh, mvdfusion_amd/fusion.py nearest_on_mesh) next to the route it replaces --
mvd_nearest_points against sample_mesh(mesh, 65 536) of the same mesh -- and a mesh-ICP iteration next to a mvd_plane_icp iteration.

One workload = (mesh, nq).  Mesh: extract_mesh of the exact signed distance |X| - 0.6 at G^3 voxels in the default box (bench_mesh_render's
sphere), G in {64, 128}.  Queries: nq points of a noisy sphere (radius 0.6 * (1 + 0.05 gauss)), seeded.  One JSON line per workload:
  us_build, us_query      MVD_NN_BUILD and MVD_NN_QUERY of mvd_nearest_on_mesh_stages alone, MVD_NN_GRID at the library's grid (--mesh-grid
                          sweeps it; with --search-only these two are the whole line)
  us_brute                MVD_NN_BRUTE, one call (skipped -- null -- where faces * nq exceeds --brute-pairs)
  us_points_build, us_points_query   mvd_nearest_points_stages against the 65 536 samples, MVD_NN_AUTO
  us_mesh_icp_iter, us_plane_icp_iter   (a call of `--iters` iterations minus a call of 0 iterations) / iters of mvd_mesh_icp on the mesh
                          and of mvd_plane_icp on the samples with sample_normals, the queries as the source
  mean_dist_mesh, mean_dist_points   what the two routes report as the mean distance of the queries (the second is the upper bound)
Every time is the median over --blocks blocks of HIP-event times on torch's current stream, after a warm-up of every launch; a block is
--reps calls between two events.  min / max give the spread.  One process, one GPU, one table.

  python tools/bench_mesh_distance.py
  python tools/bench_mesh_distance.py --grid 64 --queries 4096 65536

There is no CPU path: without a GPU this exits with an error.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_render import _event_blocks          # noqa: E402
from bench_mesh_render import RADIUS, sphere_mesh          # noqa: E402

SAMPLES = 65536


def run_one(mesh, G, nq, blocks, reps, iters, brute_pairs, grid=0, search_only=False):
    import torch
    from mvdfusion_amd import fusion, hip
    L, p, dev = hip.lib(), hip.ptr, "cuda"
    g = torch.Generator().manual_seed(1000 + G)
    d = torch.randn(nq, 3, generator=g, dtype=torch.float64)
    query = (d / d.norm(dim=1, keepdim=True) * RADIUS * (1.0 + 0.05 * torch.randn(nq, 1, generator=g, dtype=torch.float64))).float().to(dev)
    nv, nf = int(mesh.vertices.shape[0]), len(mesh)
    qstart, fstart = torch.tensor([0, nq], dtype=torch.int32).to(dev), mesh.face_start.to(dev)
    face, region = torch.empty(nq, dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.int32, device=dev)
    dist2 = torch.empty(nq, device=dev)
    point, bary, normal = (torch.empty(nq, 3, device=dev) for _ in range(3))

    def on_mesh(method, stages):
        nbytes = int(L.mvd_nearest_on_mesh_scratch(nf, 1, method, grid))
        scratch = torch.empty((nbytes + 7) // 8 + 2, dtype=torch.int64, device=dev)
        return lambda: hip.check(L.mvd_nearest_on_mesh_stages(p(query), p(qstart), p(mesh.vertices), p(mesh.faces), p(fstart), nq, nv, nf, 1, method, grid,
                                                             p(face), p(dist2), p(point), p(bary), p(region), p(normal), p(scratch), nbytes, stages,
                                                             hip.stream()))
    t = {}
    # build and query share one scratch: the query reads what the build wrote
    nbytes = int(L.mvd_nearest_on_mesh_scratch(nf, 1, hip.NN_GRID, grid))
    scratch = torch.empty((nbytes + 7) // 8 + 2, dtype=torch.int64, device=dev)
    stage = lambda stages: (lambda: hip.check(L.mvd_nearest_on_mesh_stages(p(query), p(qstart), p(mesh.vertices), p(mesh.faces), p(fstart), nq, nv, nf, 1,
                                                                          hip.NN_GRID, grid, p(face), p(dist2), p(point), p(bary), p(region), p(normal),
                                                                          p(scratch), nbytes, stages, hip.stream())))
    build, query_grid = stage(hip.NN_BUILD), stage(hip.NN_QUERY)
    t["us_build"] = _event_blocks(build, blocks, reps)
    t["us_query"] = _event_blocks(query_grid, blocks, reps)
    mean_mesh = float(dist2.double().sqrt().mean())
    grid_bits = dist2.clone()
    if nf * nq <= brute_pairs and not search_only:
        t["us_brute"] = _event_blocks(on_mesh(hip.NN_BRUTE, hip.NN_ALL), blocks, max(reps // 10, 2))
        assert torch.equal(grid_bits.view(torch.int32), dist2.view(torch.int32)), "brute and grid disagree"
    res = dict(metric="mesh_distance", G=G, faces=nf, vertices=nv, nq=nq, grid=grid, mean_dist_mesh=mean_mesh)
    if search_only:
        for key in ("us_build", "us_query"):
            res.update({key: t[key]["med"], key + "_min": t[key]["min"], key + "_max": t[key]["max"]})
        return res
    # the route exact=True replaces: the nearest of 65 536 samples
    samples = fusion.sample_mesh(mesh, SAMPLES)
    target, tstart = samples.xyz.contiguous(), torch.tensor([0, len(samples)], dtype=torch.int32).to(dev)
    index = torch.empty(nq, dtype=torch.int32, device=dev)
    pbytes = int(L.mvd_nearest_points_scratch(len(samples), 1, hip.NN_AUTO, 0))
    pscratch = torch.empty((pbytes + 7) // 8 + 2, dtype=torch.int64, device=dev)
    points = lambda stages: (lambda: hip.check(L.mvd_nearest_points_stages(p(query), p(qstart), p(target), p(tstart), nq, len(samples), 1, hip.NN_AUTO, 0,
                                                                          p(index), p(dist2), p(pscratch), pbytes, stages, hip.stream())))
    t["us_points_build"] = _event_blocks(points(hip.NN_BUILD), blocks, reps)
    t["us_points_query"] = _event_blocks(points(hip.NN_QUERY), blocks, reps)
    mean_points = float(dist2.double().sqrt().mean())
    # one ICP iteration: a call of `iters` iterations minus a call of none
    normals = fusion.sample_normals(mesh, samples).contiguous()
    moved = torch.empty_like(query)
    ident = torch.eye(3, 4, dtype=torch.float64).reshape(1, 12).to(dev)
    transform = ident.clone()
    history = torch.empty(iters + 1, 1, hip.PLANE_HISTORY, dtype=torch.float64, device=dev)
    mbytes = int(L.mvd_mesh_icp_scratch(nq, nf, 1, hip.NN_AUTO, grid))
    mscratch = torch.empty((mbytes + 7) // 8 + 2, dtype=torch.int64, device=dev)
    sbytes = int(L.mvd_plane_scratch(nq, len(samples), 1, hip.NN_AUTO, 0))
    sscratch = torch.empty((sbytes + 7) // 8 + 2, dtype=torch.int64, device=dev)

    def mesh_icp(k):
        def call():
            transform.copy_(ident)
            hip.check(L.mvd_mesh_icp(p(query), p(qstart), p(mesh.vertices), p(mesh.faces), p(fstart), nq, nv, nf, 1, hip.NN_AUTO, grid, k, float("inf"),
                                     p(transform), p(history), p(moved), p(face), p(dist2), p(point), p(normal), p(mscratch), mbytes, hip.stream()))
        return call

    def plane_icp(k):
        def call():
            transform.copy_(ident)
            hip.check(L.mvd_plane_icp(p(query), p(qstart), p(target), p(tstart), p(normals), nq, len(samples), 1, hip.NN_AUTO, 0, k, float("inf"),
                                      p(transform), p(history), p(moved), p(index), p(dist2), p(sscratch), sbytes, hip.stream()))
        return call
    icp_reps = max(reps // 10, 2)
    per_iter = {}
    for key, fn in (("us_mesh_icp_iter", mesh_icp), ("us_plane_icp_iter", plane_icp)):
        full, none = _event_blocks(fn(iters), blocks, icp_reps), _event_blocks(fn(0), blocks, icp_reps)
        per_iter[key] = round((full["med"] - none["med"]) / iters, 2)
    res.update(samples=len(samples), mean_dist_points=mean_points)
    for key in ("us_build", "us_query", "us_brute", "us_points_build", "us_points_query"):
        v = t.get(key)
        res.update({key: v and v["med"], key + "_min": v and v["min"], key + "_max": v and v["max"]})
    res.update(per_iter, icp_iters=iters, blocks=blocks, reps=reps, lib=os.path.basename(hip.LIB_PATHS[hip.OPERAND_FORMAT]), gpu=torch.cuda.get_device_name(0))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--queries", type=int, nargs="*", default=[4096, 65536, 1048576])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=8, help="iterations of the two ICP calls that are timed")
    ap.add_argument("--mesh-grid", type=int, nargs="*", default=[0], help="cells per axis of the mesh search (0: the library's choice); several: a sweep")
    ap.add_argument("--search-only", action="store_true", help="us_build and us_query only (for a sweep of --mesh-grid)")
    ap.add_argument("--brute-pairs", type=float, default=1e10, help="MVD_NN_BRUTE is timed up to this many face-query pairs")
    a = ap.parse_args()
    if a.blocks < 3 or a.iters < 1:
        ap.error("--blocks must be >= 3 and --iters >= 1")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_distance: no GPU visible (there is no CPU path)")
    for G in a.grid:
        mesh = sphere_mesh(G)
        for nq in a.queries:
            for grid in a.mesh_grid:
                print(json.dumps(run_one(mesh, G, nq, a.blocks, a.reps, a.iters, a.brute_pairs, grid, a.search_only)), flush=True)


if __name__ == "__main__":
    main()
