#!/usr/bin/env python
"""Volumetric fusion (mvd_tsdf_integrate, mvd_mesh_count, mvd_mesh_emit; mvdfusion_amd/fusion.py) against the integrate rule written with
torch ops on the GPU.

One workload = (G voxels per side, V views, data) at S = 32 on a ring rig (distance 1.5, elevation 30 degrees, V azimuths), the box
0 +- 0.75, trunc 3 voxels, carving on, colour from a random image at up = 1.  data "sphere": the analytic depth of a sphere of radius 0.6
(background latent +1), what a clean sample looks like; data "random": depth latent 0.5 N(0, 1), so the background and silhouette branches
are taken at every depth.  Defaults G in {64, 128} x V in {8, 24} x both.  One JSON line per workload:
  us_per_integrate      mvd_tsdf_integrate (one launch, with colour)
  us_per_mesh_count     mvd_mesh_count on that volume (six launches)
  us_per_mesh_emit      mvd_mesh_emit (two launches) into exact outputs
  us_per_torch_rule     tsdf and weight of the same rule with torch ops in fp32 on the GPU ((voxels, views) temporaries) -- what a user
                        would otherwise write; no colour
  torch_weight_mismatch_share   voxels whose torch weight differs from the kernel's (two fp32 evaluation orders: expected ~1e-4 or less)
Every figure is the median of --blocks blocks between HIP events on torch's stream; a block repeats the call until it lasts about
--block-seconds (min / max give the spread).  All launches of a workload are warmed up before any is timed.  The host call with its
allocations and its one synchronisation is NOT timed here.

  python tools/bench_tsdf.py
  python tools/bench_tsdf.py --grid 128 --views 24 --data sphere

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


def _timed(fn, blocks, block_seconds):
    import torch
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(3, min(5000, int(block_seconds / max(time.perf_counter() - t, 1e-6))))
    times = []
    for _ in range(blocks):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) / reps * 1e3)
    return dict(med=round(statistics.median(times), 2), min=round(min(times), 2), max=round(max(times), 2), reps=reps)


def ring_rig(V):
    import torch
    from mvdfusion_amd.cameras import Cameras, look_at_view_transform
    R, T = look_at_view_transform(1.5, torch.full((V,), 30.0), torch.arange(V, dtype=torch.float32) * (360.0 / V))
    return Cameras(R, T, torch.full((V, 2), 2.1875), torch.zeros(V, 2))


def sphere_latent(rig, S, radius, depth_scale, depth_shift):
    """(V, S, S) depth latent of a sphere at the origin: per pixel centre the nearer ray-sphere root in camera z, background +1."""
    import torch
    R, T, f, p = (t.double() for t in (rig.R, rig.T, rig.focal_length, rig.principal_point))
    lin = torch.linspace(1.0 - 1.0 / S, -1.0 + 1.0 / S, S, dtype=torch.float64)
    yy, xx = torch.meshgrid(lin, lin, indexing="ij")
    xy = torch.stack([xx, yy], dim=-1).reshape(1, S * S, 2)

    def unproject(z):
        xc = torch.cat([(xy - p[:, None, :]) * z / f[:, None, :], torch.full((len(R), S * S, 1), z, dtype=torch.float64)], dim=-1)
        return torch.einsum("npi,nji->npj", xc - T[:, None, :], R)

    p1 = unproject(1.0)
    d = unproject(2.0) - p1
    a, b, c = (d * d).sum(-1), 2.0 * (p1 * d).sum(-1), (p1 * p1).sum(-1) - radius ** 2
    disc = b * b - 4 * a * c
    z = 1.0 + (-b - disc.clamp(min=0).sqrt()) / (2 * a)
    lat = 2.0 * (z - depth_shift) / depth_scale - 1.0
    return torch.where(disc > 0, lat, torch.ones_like(lat)).reshape(-1, S, S).float()


def torch_rule(lat, cams, V, S, G, org, vs, trunc, carve, depth_scale, depth_shift, lo, hi):
    """(tsdf, weight) (G, G, G) of include/mvd_hip.h's view rule, fp32 torch ops on lat's device; cams = Cameras there."""
    import torch
    dev = lat.device
    dn = torch.clip((lat[:, 4] + 1.0) / 2.0, 0.0, 1.0)
    fg = ((dn > lo) & (dn < hi)).reshape(V, S * S)
    zmap = (dn * depth_scale + depth_shift).reshape(V, S * S)
    R, T, f, p = cams.R, cams.T, cams.focal_length, cams.principal_point
    ax = [o + (torch.arange(G, dtype=torch.float32, device=dev) + 0.5) * vs for o in org]
    zz, yy, xx = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    X = torch.stack([xx, yy, zz], dim=-1).reshape(G ** 3, 3)
    c = torch.einsum("pi,nij->pnj", X, R) + T[None]                       # (voxels, views, 3)
    zc = c[..., 2]
    u, w = f[None, :, 0] * c[..., 0] / zc + p[None, :, 0], f[None, :, 1] * c[..., 1] / zc + p[None, :, 1]
    seen = (zc > 0) & (u.abs() <= 1) & (w.abs() <= 1)
    pix = lambda t: torch.nan_to_num(torch.clip((1.0 - t) * (S / 2.0) - 0.5, 0.0, S - 1.0), nan=0.0)
    ix, iy = pix(u), pix(w)
    x0f, y0f = ix.floor(), iy.floor()
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = (x0 + 1).clamp(max=S - 1), (y0 + 1).clamp(max=S - 1)
    wx, wy = ix - x0f, iy - y0f
    view = torch.arange(V, device=dev)[None, :].expand_as(x0)
    tap = lambda m, y, x: m[view, y * S + x]
    nfg = tap(fg, y0, x0).long() + tap(fg, y0, x1) + tap(fg, y1, x0) + tap(fg, y1, x1)
    zs = (tap(zmap, y0, x0) * (1 - wx) + tap(zmap, y0, x1) * wx) * (1 - wy) + (tap(zmap, y1, x0) * (1 - wx) + tap(zmap, y1, x1) * wx) * wy
    sdf = zs - zc
    surface = seen & (nfg == 4) & ~(sdf < -trunc)
    free = seen & (nfg == 0) & bool(carve)
    d = torch.where(surface, (sdf / trunc).clamp(max=1.0), torch.ones_like(sdf))
    obs = surface | free
    weight = obs.sum(1)
    total = torch.where(obs, d, torch.zeros_like(d)).sum(1)
    tsdf = torch.where(weight > 0, total / weight.clamp(min=1), torch.ones_like(total))
    return tsdf.reshape(G, G, G), weight.reshape(G, G, G)


def run_one(G, V, data, S, blocks, block_seconds):
    import ctypes
    import torch
    from mvdfusion_amd import hip
    from mvdfusion_amd.cameras import pack_cameras
    L = hip.lib()
    dev = "cuda"
    ds, dsh, lo, hi, he, carve = 2.0, 0.5, 0.02, 0.98, 0.75, 1
    trunc = 3 * 2 * he / G
    g = torch.Generator().manual_seed(100 * V + G)
    rig = ring_rig(V)
    lat = torch.randn(V, 5, S, S, generator=g)
    if data == "sphere":
        lat[:, 4] = sphere_latent(rig, S, 0.6, ds, dsh)
    else:
        lat[:, 4] *= 0.5
    lat = lat.to(dev)
    rgb = torch.rand(V, 3, S, S, generator=g).to(dev)
    cams = pack_cameras(rig).to(dev)
    tsdf = torch.empty(1, G, G, G, device=dev)
    weight = torch.empty(1, G, G, G, dtype=torch.uint8, device=dev)
    color = torch.empty(1, G, G, G, 3, device=dev)
    cweight = torch.empty(1, G, G, G, dtype=torch.uint8, device=dev)
    nbytes = int(L.mvd_mesh_scratch(1, G))
    scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    starts = torch.zeros(2, 2, dtype=torch.int32, device=dev)
    fill = (ctypes.c_float * 3)(0.5, 0.5, 0.5)

    def integrate():
        hip.check(L.mvd_tsdf_integrate(hip.ptr(lat), hip.ptr(rgb), hip.ptr(cams), hip.ptr(tsdf), hip.ptr(weight), hip.ptr(color),
                                       hip.ptr(cweight), 1, V, S, 1, G, 0.0, 0.0, 0.0, he, trunc, carve, ds, dsh, lo, hi, hip.stream()))

    def count():
        hip.check(L.mvd_mesh_count(hip.ptr(tsdf), hip.ptr(weight), 1, G, hip.ptr(starts[0]), hip.ptr(starts[1]), hip.ptr(scratch), nbytes,
                                   hip.stream()))

    integrate()
    count()
    nv, nf = (int(v) for v in starts.cpu()[:, 1])
    vertices, colors = torch.empty(max(nv, 1), 3, device=dev), torch.empty(max(nv, 1), 3, device=dev)
    faces = torch.empty(max(nf, 1), 3, dtype=torch.int32, device=dev)

    def emit():
        hip.check(L.mvd_mesh_emit(hip.ptr(tsdf), hip.ptr(weight), hip.ptr(color), hip.ptr(cweight), 1, G, 0.0, 0.0, 0.0, he, fill,
                                  hip.ptr(vertices), hip.ptr(colors), hip.ptr(faces), nv, nf, hip.ptr(scratch), nbytes, hip.stream()))

    rig_dev = rig.to(dev)
    org = [torch.tensor(0.0 - he, dtype=torch.float32).item()] * 3
    vs = float(torch.tensor(2.0, dtype=torch.float32) * torch.tensor(he, dtype=torch.float32) / G)
    rule = lambda: torch_rule(lat, rig_dev, V, S, G, org, vs, trunc, carve, ds, dsh, lo, hi)
    emit()
    tt, tw = rule()
    torch.cuda.synchronize()
    mismatch = float((tw != weight[0].long()).float().mean())
    same = tw == weight[0].long()
    tsdf_diff = float((tt - tsdf[0]).abs()[same].max())
    res = dict(metric="tsdf", G=G, V=V, S=S, data=data, voxels=G ** 3, observed_share=round(float((weight > 0).float().mean()), 4),
               vertices=nv, faces=nf, scratch_mib=round(nbytes / 2 ** 20, 1))
    for key, fn in (("us_per_integrate", integrate), ("us_per_mesh_count", count), ("us_per_mesh_emit", emit), ("us_per_torch_rule", rule)):
        t = _timed(fn, blocks, block_seconds)
        res.update({key: t["med"], key + "_min": t["min"], key + "_max": t["max"], key.replace("us_per_", "reps_"): t["reps"]})
    res.update(torch_over_integrate=round(res["us_per_torch_rule"] / res["us_per_integrate"], 1), torch_weight_mismatch_share=mismatch,
               torch_tsdf_max_diff=tsdf_diff, blocks=blocks, gpu=torch.cuda.get_device_name(0))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--views", type=int, nargs="*", default=[8, 24])
    ap.add_argument("--data", nargs="*", default=["sphere", "random"], choices=["sphere", "random"])
    ap.add_argument("--latent", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-seconds", type=float, default=0.2)
    a = ap.parse_args()
    if a.blocks < 3:
        ap.error("--blocks must be >= 3")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf: no GPU visible (there is no CPU path)")
    for G in a.grid:
        for V in a.views:
            for data in a.data:
                print(json.dumps(run_one(G, V, data, a.latent, a.blocks, a.block_seconds)), flush=True)


if __name__ == "__main__":
    main()
