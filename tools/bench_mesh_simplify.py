#!/usr/bin/env python
"""Mesh simplification (include/mvd_hip.h: mvd_mesh_cluster_count, _emit, _dedupe; fusion.simplify_mesh) on marched meshes, next to
mean-placement clustering written with torch ops on the GPU.

One workload = (G voxels per side, data, cells).  The meshes are those of tools/bench_mesh_topology.py: "sphere" is extract_mesh of the
exact signed distance of a sphere of radius 0.6, "random" that of integrate_tsdf of 8 views at S = 32 with a random depth latent.
Defaults G in {64, 128} x both x cells in {16, 64}, quadric placement.  One JSON line per workload:
  faces_in, vertices_in, clusters, faces_out, vertices_out, longest_member_list, placed_fallback
  the totals of fusion.mesh_topology on the result (clustering promises neither a closed nor a manifold result: here is what it gave)
  accuracy_h            compare_geometry(original vertices, simplified mesh, exact=True).accuracy in units of the cell side h
  us_per_incidence      mvd_mesh_incidence of the input (what the count call needs)
  us_per_count          mvd_mesh_cluster_count (box, flags, scan of cells^3 words, ids, list offsets)
  us_per_emit           mvd_mesh_cluster_emit (member lists, per-vertex quadrics, per-cluster solve, mapped faces)
  us_per_dedupe         mvd_mesh_incidence of the mapped faces + mvd_mesh_cluster_dedupe
  us_per_filter         mvd_mesh_filter_count + _emit of the result
  us_per_torch_mean     mean-placement clustering with torch ops (floor, unique, index_add_, unique over sorted face ids) -- what a
                        user would otherwise write; it averages with float atomics, so its bits are not reproducible
  us_simplify_mesh      the whole host call fusion.simplify_mesh: launches, allocations and two host reads, wall clock
Every device figure is the median of --blocks blocks between HIP events on torch's stream; a block repeats the call until it lasts
about --block-seconds (min / max give the spread).  All launches of a workload are warmed up before any is timed.

  python tools/bench_mesh_simplify.py
  python tools/bench_mesh_simplify.py --grid 128 --data random --cells 64

There is no CPU path: without a GPU this exits with an error.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def torch_mean_clustering(v, f, cells):
    """(vertices, faces) of mean-placement clustering of a one-scene mesh with finite, used vertices."""
    import torch
    lo, hi = v.min(0).values.double(), v.max(0).values.double()
    h = (hi - lo).max() / cells
    n = ((hi - lo) / h).floor().add(1).clamp(1, cells).long()
    cell = torch.minimum(((v.double() - lo) / h).floor().long().clamp(min=0), n - 1)
    lin = (cell[:, 2] * n[1] + cell[:, 1]) * n[0] + cell[:, 0]
    _, cid = torch.unique(lin, return_inverse=True)
    nc = int(cid.max()) + 1
    s = torch.zeros(nc, 3, dtype=torch.float64, device=v.device).index_add_(0, cid, v.double())
    c = torch.zeros(nc, dtype=torch.float64, device=v.device).index_add_(0, cid, torch.ones_like(cid, dtype=torch.float64))
    mf = cid[f.long()]
    mf = mf[(mf[:, 0] != mf[:, 1]) & (mf[:, 1] != mf[:, 2]) & (mf[:, 0] != mf[:, 2])]
    key = mf.sort(dim=1).values
    key = (key[:, 0] * nc + key[:, 1]) * nc + key[:, 2]
    order = torch.sort(key, stable=True)
    first = torch.ones_like(key, dtype=torch.bool)
    first[1:] = order.values[1:] != order.values[:-1]
    return (s / c[:, None]).float(), mf[order.indices[first].sort().values]


def run_one(G, data, cells, blocks, block_seconds):
    import torch
    from bench_mesh_topology import make_mesh
    from bench_tsdf import _timed
    from mvdfusion_amd import fusion, hip
    L, st = hip.lib(), hip.stream
    mesh = make_mesh(G, data)
    v, f, rgb = mesh.vertices, mesh.faces, mesh.rgb
    nv, nf, dev = int(v.shape[0]), int(f.shape[0]), v.device
    vs, fs = mesh.vertex_start.to(dev), mesh.face_start.to(dev)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    p = lambda t: hip.ptr(t) if t is not None and t.numel() else None
    words = lambda n: torch.empty((int(n) + 7) // 8, dtype=torch.int64, device=dev)
    nb_inc, nb_cl = int(L.mvd_mesh_incidence_scratch(nv, nf)), int(L.mvd_mesh_cluster_scratch(nv, nf, 1, cells))
    sc_inc, sc_cl = words(nb_inc), words(nb_cl)
    inc_start, inc, vc, cs = i32(nv + 1), i32(3 * nf), i32(nv), i32(2)

    def incidence():
        hip.check(L.mvd_mesh_incidence(p(f), hip.ptr(vs), hip.ptr(fs), nv, nf, 1, hip.ptr(inc_start), p(inc), hip.ptr(sc_inc), nb_inc, st()))

    def count():
        hip.check(L.mvd_mesh_cluster_count(p(v), hip.ptr(vs), hip.ptr(inc_start), nv, nf, 1, cells, p(vc), hip.ptr(cs), hip.ptr(sc_cl), nb_cl, st()))

    incidence(), count()
    nc = int(cs[1])
    ov, oc = torch.empty(nc, 3, device=dev), (torch.empty(nc, 3, device=dev) if rgb is not None else None)
    size, rank, placed, mapped = i32(nc), i32(nc), i32(nc), i32(nf, 3)
    keep, keep2 = torch.empty(nf, dtype=torch.uint8, device=dev), torch.empty(nf, dtype=torch.uint8, device=dev)

    def emit():
        hip.check(L.mvd_mesh_cluster_emit(p(v), p(rgb), p(f), hip.ptr(vs), hip.ptr(fs), hip.ptr(inc_start), p(inc), p(vc), nv, nf, 1, cells,
                                          hip.SIMPLIFY_QUADRIC, nc, p(ov), p(oc), p(size), p(rank), p(placed), p(mapped), p(keep), hip.ptr(sc_cl),
                                          nb_cl, st()))

    nb_cinc = int(L.mvd_mesh_incidence_scratch(nc, nf))
    sc_cinc, cinc_start, cinc = words(nb_cinc), i32(nc + 1), i32(3 * nf)

    def dedupe():
        hip.check(L.mvd_mesh_incidence(p(mapped), hip.ptr(cs), hip.ptr(fs), nc, nf, 1, hip.ptr(cinc_start), p(cinc), hip.ptr(sc_cinc), nb_cinc, st()))
        hip.check(L.mvd_mesh_cluster_dedupe(p(mapped), p(keep), hip.ptr(cinc_start), p(cinc), nc, nf, p(keep2), st()))

    emit(), dedupe()
    nb_f = int(L.mvd_mesh_filter_scratch(nc, nf))
    sc_f, starts = words(nb_f), i32(2, 2)
    hip.check(L.mvd_mesh_filter_count(p(mapped), p(keep2), hip.ptr(cs), hip.ptr(fs), nc, nf, 1, hip.ptr(starts[0]), hip.ptr(starts[1]), hip.ptr(sc_f),
                                      nb_f, st()))
    nvo, nfo = (int(x) for x in starts.cpu()[:, 1])
    fv, fc, ff, vi, fi = torch.empty(nvo, 3, device=dev), torch.empty(nvo, 3, device=dev), i32(nfo, 3), i32(nvo), i32(nfo)

    def filter_():
        hip.check(L.mvd_mesh_filter_count(p(mapped), p(keep2), hip.ptr(cs), hip.ptr(fs), nc, nf, 1, hip.ptr(starts[0]), hip.ptr(starts[1]),
                                          hip.ptr(sc_f), nb_f, st()))
        hip.check(L.mvd_mesh_filter_emit(p(ov), p(oc), p(mapped), nc, nf, p(fv), p(fc) if oc is not None else None, p(ff), p(vi), p(fi), nvo, nfo,
                                         hip.ptr(sc_f), nb_f, st()))

    def torch_rule():
        torch_mean_clustering(v, f, cells)

    filter_(), torch_rule()
    out, _, _, cl = fusion.simplify_mesh(mesh, cells=cells, return_index=True)
    assert len(out) == nfo and int(out.vertices.shape[0]) == nvo
    topo = fusion.mesh_topology(out)
    used = v[vc >= 0]
    h = float((used.max(0).values.double() - used.min(0).values.double()).max()) / cells
    acc = float(fusion.compare_geometry(v, out, exact=True).accuracy[0]) / h
    tv, tf = torch_mean_clustering(v, f, cells)
    res = dict(metric="mesh_simplify", G=G, data=data, cells=cells, vertices_in=nv, faces_in=nf, clusters=nc, vertices_out=nvo, faces_out=nfo,
               longest_member_list=int(size.max()) if nc else 0, placed_fallback=int((cl.placed == hip.SIMPLIFY_PLACED_FALLBACK).sum()),
               **{k: int(getattr(topo, k)[0]) for k in hip.TOPO_FIELDS}, h=h, accuracy_h=round(acc, 4),
               torch_faces=int(tf.shape[0]), torch_clusters=int(tv.shape[0]))
    for key, fn in (("us_per_incidence", incidence), ("us_per_count", count), ("us_per_emit", emit), ("us_per_dedupe", dedupe),
                    ("us_per_filter", filter_), ("us_per_torch_mean", torch_rule)):
        r = _timed(fn, blocks, block_seconds)
        res.update({key: r["med"], key + "_min": r["min"], key + "_max": r["max"], key.replace("us_per_", "reps_"): r["reps"]})
    walls = []
    for _ in range(max(blocks, 5) + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fusion.simplify_mesh(mesh, cells=cells)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e6)
    walls = walls[1:]
    ours = sum(res[k] for k in ("us_per_incidence", "us_per_count", "us_per_emit", "us_per_dedupe", "us_per_filter"))
    res.update(us_simplify_mesh=round(statistics.median(walls), 1), us_simplify_mesh_min=round(min(walls), 1), us_simplify_mesh_max=round(max(walls), 1),
               us_entries_total=round(ours, 1), torch_over_entries=round(res["us_per_torch_mean"] / ours, 2), blocks=blocks,
               gpu=torch.cuda.get_device_name(0))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--data", nargs="*", default=["sphere", "random"], choices=["sphere", "random"])
    ap.add_argument("--cells", type=int, nargs="*", default=[16, 64])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-seconds", type=float, default=0.2)
    a = ap.parse_args()
    if a.blocks < 3:
        ap.error("--blocks must be >= 3")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_simplify: no GPU visible (there is no CPU path)")
    for G in a.grid:
        for data in a.data:
            for cells in a.cells:
                print(json.dumps(run_one(G, data, cells, a.blocks, a.block_seconds)), flush=True)


if __name__ == "__main__":
    main()
