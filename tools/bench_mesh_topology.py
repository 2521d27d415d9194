#!/usr/bin/env python
"""Mesh topology (include/mvd_hip.h: mvd_mesh_incidence, _label, _component_table, _topology, _filter_count, _filter_emit,
_vertex_normals, _smooth; mvdfusion_amd/fusion.py) on marched meshes, next to the labelling written with torch ops on the GPU.

One workload = (G voxels per side, data).  data "sphere": extract_mesh of the exact signed distance of a sphere of radius 0.6 -- one
closed component, what a clean sample gives; data "random": extract_mesh of integrate_tsdf of 8 views at S = 32 whose depth latent is
0.5 N(0, 1) (tools/bench_tsdf.py's random case: carving on, trunc 3 voxels) -- the object a noisy depth gives, plus its floaters.
Defaults G in {64, 128} x both.  One JSON line per workload:
  vertices, faces, components, floater_faces   floater_faces: the faces outside the component with the most faces
  us_per_incidence      mvd_mesh_incidence (count, scan, fill, sort)
  us_per_components     mvd_mesh_label + mvd_mesh_component_table (union-find, flatten, scan, labels, table)
  us_per_topology       mvd_mesh_topology on the table and labels above
  us_per_filter_count / us_per_filter_emit   keeping the largest component
  us_per_normals        mvd_mesh_vertex_normals
  us_per_smooth_pass    mvd_mesh_smooth with passes = 1, boundary vertices pinned
  us_per_torch_labels   the labels alone with torch ops: min-label propagation over the faces with scatter_reduce(amin) until nothing
                        changes (one host read per round) -- what a user would otherwise write; torch_rounds: the rounds it took
  us_keep_components    the whole host call fusion.keep_components(mesh, largest=1): its launches, allocations and two host reads,
                        wall clock around a synchronise
Every device figure is the median of --blocks blocks between HIP events on torch's stream; a block repeats the call until it lasts
about --block-seconds (min / max give the spread).  All launches of a workload are warmed up before any is timed.

  python tools/bench_mesh_topology.py
  python tools/bench_mesh_topology.py --grid 128 --data random

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


def make_mesh(G, data):
    import torch
    from bench_tsdf import ring_rig
    from mvdfusion_amd import fusion
    if data == "sphere":
        ax = ((torch.arange(G, dtype=torch.float64, device="cuda") + 0.5) * (1.5 / G) - 0.75)
        zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
        return fusion.extract_mesh(((xx ** 2 + yy ** 2 + zz ** 2).sqrt() - 0.6).float())
    V, S = 8, 32
    g = torch.Generator().manual_seed(100 * V + G)
    lat = torch.randn(V, 5, S, S, generator=g)
    lat[:, 4] *= 0.5
    return fusion.extract_mesh(fusion.integrate_tsdf(lat.cuda(), ring_rig(V).to("cuda"), grid=G))


def torch_labels(faces, nv):
    """(label (nv,) = the smallest vertex id of the vertex's component, rounds): min-label propagation to a fixed point."""
    import torch
    f = faces.long()
    flat = f.reshape(-1)
    label = torch.arange(nv, device=faces.device)
    rounds = 0
    while True:
        low = label[f].min(dim=1).values[:, None].expand(-1, 3).reshape(-1)
        new = label.scatter_reduce(0, flat, low, "amin")
        rounds += 1
        if bool((new == label).all()):
            return label, rounds
        label = new


def run_one(G, data, blocks, block_seconds):
    import torch
    from bench_tsdf import _timed
    from mvdfusion_amd import fusion, hip
    L, st = hip.lib(), hip.stream
    mesh = make_mesh(G, data)
    v, f = mesh.vertices, mesh.faces
    nv, nf, dev = int(v.shape[0]), int(f.shape[0]), v.device
    vs, fs = mesh.vertex_start.to(dev), mesh.face_start.to(dev)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    sizes = {k: int(getattr(L, f"mvd_mesh_{k}_scratch")(nv, nf)) for k in ("incidence", "label", "topology", "filter")}
    scratch = {k: (n, torch.empty((n + 7) // 8, dtype=torch.int64, device=dev)) for k, n in sizes.items()}
    inc_start, inc, vc, fc, cs = i32(nv + 1), i32(3 * nf), i32(nv), i32(nf), i32(2)
    totals, flags = i32(1, hip.TOPO_TOTALS), torch.empty(nv, dtype=torch.uint8, device=dev)
    normals, out, tmp = (torch.empty(nv, 3, device=dev) for _ in range(3))
    mesh_args = (hip.ptr(f), hip.ptr(vs), hip.ptr(fs), nv, nf, 1)
    sc = lambda k: (hip.ptr(scratch[k][1]), scratch[k][0])

    def incidence():
        hip.check(L.mvd_mesh_incidence(*mesh_args, hip.ptr(inc_start), hip.ptr(inc), *sc("incidence"), st()))

    def label():
        hip.check(L.mvd_mesh_label(*mesh_args, hip.ptr(vc), hip.ptr(fc), hip.ptr(cs), *sc("label"), st()))

    incidence()
    label()
    ncomp = int(cs[1])
    root, cfaces, cverts = i32(ncomp), i32(ncomp), i32(ncomp)

    def components():
        label()
        hip.check(L.mvd_mesh_component_table(hip.ptr(vc), hip.ptr(fc), nv, nf, ncomp, hip.ptr(root), hip.ptr(cfaces), hip.ptr(cverts), st()))

    def topology():
        hip.check(L.mvd_mesh_topology(*mesh_args, hip.ptr(inc_start), hip.ptr(inc), hip.ptr(vc), hip.ptr(cs), hip.ptr(totals), hip.ptr(flags),
                                      *sc("topology"), st()))

    components()
    topology()
    biggest = int(cfaces.argmax())
    keep = (fc == biggest).to(torch.uint8).contiguous()
    starts = i32(2, 2)

    def filter_count():
        hip.check(L.mvd_mesh_filter_count(hip.ptr(f), hip.ptr(keep), hip.ptr(vs), hip.ptr(fs), nv, nf, 1, hip.ptr(starts[0]), hip.ptr(starts[1]),
                                          *sc("filter"), st()))

    filter_count()
    nvo, nfo = (int(x) for x in starts.cpu()[:, 1])
    ov, oc, of, vi, fi = torch.empty(nvo, 3, device=dev), torch.empty(nvo, 3, device=dev), i32(nfo, 3), i32(nvo), i32(nfo)
    rgb = mesh.rgb

    def filter_emit():
        hip.check(L.mvd_mesh_filter_emit(hip.ptr(v), hip.ptr(rgb), hip.ptr(f), nv, nf, hip.ptr(ov), hip.ptr(oc) if rgb is not None else None,
                                         hip.ptr(of), hip.ptr(vi), hip.ptr(fi), nvo, nfo, *sc("filter"), st()))

    def vertex_normals():
        hip.check(L.mvd_mesh_vertex_normals(hip.ptr(v), hip.ptr(f), hip.ptr(inc_start), hip.ptr(inc), nv, nf, hip.ptr(normals), st()))

    def smooth_pass():
        hip.check(L.mvd_mesh_smooth(hip.ptr(v), hip.ptr(f), hip.ptr(inc_start), hip.ptr(inc), hip.ptr(flags), nv, nf, 1, 0.5, -0.53,
                                    hip.TOPO_FLAG_BOUNDARY, hip.ptr(out), hip.ptr(tmp), st()))

    rounds = [0]

    def torch_rule():
        rounds[0] = torch_labels(f, nv)[1]

    filter_emit(), vertex_normals(), smooth_pass()
    tl, _ = torch_labels(f, nv)
    torch.cuda.synchronize()
    t = totals.cpu()[0].tolist()
    labels_agree = bool((root.long()[vc.long().clamp(min=0)] == tl)[vc >= 0].all())
    res = dict(metric="mesh_topology", G=G, data=data, vertices=nv, faces=nf, floater_faces=nf - int(cfaces.max()) if ncomp else 0,
               kept_vertices=nvo, kept_faces=nfo, longest_list=int((inc_start[1:] - inc_start[:-1]).max()) if nv else 0,
               **dict(zip(hip.TOPO_FIELDS, t)), torch_labels_agree=labels_agree)
    for key, fn in (("us_per_incidence", incidence), ("us_per_components", components), ("us_per_topology", topology),
                    ("us_per_filter_count", filter_count), ("us_per_filter_emit", filter_emit), ("us_per_normals", vertex_normals),
                    ("us_per_smooth_pass", smooth_pass), ("us_per_torch_labels", torch_rule)):
        r = _timed(fn, blocks, block_seconds)
        res.update({key: r["med"], key + "_min": r["min"], key + "_max": r["max"], key.replace("us_per_", "reps_"): r["reps"]})
    walls = []
    for _ in range(max(blocks, 5) + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fusion.keep_components(mesh, largest=1)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e6)
    walls = walls[1:]
    res.update(us_keep_components=round(statistics.median(walls), 1), us_keep_components_min=round(min(walls), 1),
               us_keep_components_max=round(max(walls), 1), torch_rounds=rounds[0],
               torch_over_components=round(res["us_per_torch_labels"] / res["us_per_components"], 1), blocks=blocks, gpu=torch.cuda.get_device_name(0))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--data", nargs="*", default=["sphere", "random"], choices=["sphere", "random"])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-seconds", type=float, default=0.2)
    a = ap.parse_args()
    if a.blocks < 3:
        ap.error("--blocks must be >= 3")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_topology: no GPU visible (there is no CPU path)")
    for G in a.grid:
        for data in a.data:
            print(json.dumps(run_one(G, data, a.blocks, a.block_seconds)), flush=True)


if __name__ == "__main__":
    main()
