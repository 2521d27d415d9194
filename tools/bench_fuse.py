#!/usr/bin/env python
"""View fusion (mvd_fuse_points + mvd_compact_points, mvdfusion_amd/fusion.py) against the same rule written with torch ops on the GPU.

One workload = (V views, up) at S = 32 on a ring rig (distance 1.5, elevation 30 degrees, V azimuths), depth latent 0.5 N(0, 1), a random
image; defaults V in {8, 16, 24} x up in {1, 8}.  One JSON line per workload:
  us_per_fuse_launch          mvd_fuse_points as fuse_views launches it (stage auto: one of the two forms below, include/mvd_hip.h)
  us_per_fuse_launch_global   ... forced to read global memory
  us_per_fuse_launch_lds      ... forced to stage the depth planes in LDS (absent when they do not fit)
  us_per_compaction           mvd_compact_points (three launches) with min_support = 0, max_conflicts = 255: every foreground point moves
  us_per_torch_rule           the votes of the same rule with torch ops in fp32 on the GPU (gathers over (points, views) temporaries) --
                              what a user would otherwise write; no compaction, no colour
  torch_count_mismatch_share  points whose torch counts differ from the kernel's (two fp32 evaluation orders: expected ~1e-4 or less)
Every figure is the median of --blocks blocks; a block repeats the call until it lasts about --block-seconds and ends with a device
synchronise (min / max give the spread).  All launches of a workload are warmed up before any is timed.

  python tools/bench_fuse.py
  python tools/bench_fuse.py --views 16 --up 8

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
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) / reps * 1e6)
    return dict(med=round(statistics.median(times), 2), min=round(min(times), 2), max=round(max(times), 2), reps=reps)


def ring_rig(V):
    import torch
    from mvdfusion_amd.cameras import Cameras, look_at_view_transform
    R, T = look_at_view_transform(1.5, torch.full((V,), 30.0), torch.arange(V, dtype=torch.float32) * (360.0 / V))
    return Cameras(R, T, torch.full((V, 2), 2.1875), torch.zeros(V, 2))


def torch_rule(lat, cams, lin, V, S, up, depth_scale, depth_shift, lo, hi, tau):
    """(support, conflict) int64 (V * P * P) of include/mvd_hip.h's pair rule, fp32 torch ops on lat's device; cams = Cameras there."""
    import torch
    P = S * up
    dn = torch.clip((lat[:, 4] + 1.0) / 2.0, 0.0, 1.0)
    fg = ((dn > lo) & (dn < hi)).reshape(V, S * S)
    zmap = (dn * depth_scale + depth_shift).reshape(V, S * S)
    R, T, f, p = cams.R, cams.T, cams.focal_length, cams.principal_point
    fine = zmap.reshape(V, S, S).repeat_interleave(up, dim=1).repeat_interleave(up, dim=2).reshape(V, P * P)
    yy, xx = torch.meshgrid(lin, lin, indexing="ij")
    xy = torch.stack([xx, yy], dim=-1).reshape(1, P * P, 2)
    xc = torch.cat([(xy - p[:, None, :]) * fine[..., None] / f[:, None, :], fine[..., None]], dim=-1)
    X = torch.einsum("npi,nji->npj", xc - T[:, None, :], R).reshape(V * P * P, 3)
    c = torch.einsum("pi,nij->pnj", X, R) + T[None]                       # (points, views, 3)
    zc = c[..., 2]
    u, w = f[None, :, 0] * c[..., 0] / zc + p[None, :, 0], f[None, :, 1] * c[..., 1] / zc + p[None, :, 1]
    seen = (zc > 0) & (u.abs() <= 1) & (w.abs() <= 1)
    pix = lambda t: torch.nan_to_num(torch.clip((1.0 - t) * (S / 2.0) - 0.5, 0.0, S - 1.0), nan=0.0)
    ix, iy = pix(u), pix(w)
    x0f, y0f = ix.floor(), iy.floor()
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = (x0 + 1).clamp(max=S - 1), (y0 + 1).clamp(max=S - 1)
    wx, wy = ix - x0f, iy - y0f
    view = torch.arange(V, device=lat.device)[None, :].expand_as(x0)
    tap = lambda m, y, x: m[view, y * S + x]
    all_fg = tap(fg, y0, x0) & tap(fg, y0, x1) & tap(fg, y1, x0) & tap(fg, y1, x1)
    zs = (tap(zmap, y0, x0) * (1 - wx) + tap(zmap, y0, x1) * wx) * (1 - wy) + (tap(zmap, y1, x0) * (1 - wx) + tap(zmap, y1, x1) * wx) * wy
    dz = zc - zs
    own = torch.arange(V, device=lat.device).repeat_interleave(P * P)
    votes = (view != own[:, None]) & seen & all_fg
    return (votes & (dz.abs() <= tau)).sum(1), (votes & (dz < -tau)).sum(1)


def run_one(V, up, S, blocks, block_seconds):
    import torch
    from mvdfusion_amd import hip
    from mvdfusion_amd.cameras import pack_cameras
    L = hip.lib()
    dev = "cuda"
    P = S * up
    n = V * P * P
    g = torch.Generator().manual_seed(100 * V + up)
    lat = torch.randn(V, 5, S, S, generator=g)
    lat[:, 4] *= 0.5
    lat = lat.to(dev)
    rgb = torch.rand(V, 3, P, P, generator=g).to(dev)
    rig = ring_rig(V)
    cams = pack_cameras(rig).to(dev)
    lin = torch.linspace(1.0 - 1.0 / P, -1.0 + 1.0 / P, P, dtype=torch.float32).to(dev)
    ds, dsh, lo, hi, tau = 2.0, 0.5, 0.02, 0.98, 0.05
    xyz, color = torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev)
    sup, con, fl = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(3))
    oxyz, ocolor, osup = torch.empty_like(xyz), torch.empty_like(color), torch.empty_like(sup)
    oidx = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = int(L.mvd_compact_points_scratch(n))
    scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)

    def fuse(stage):
        return L.mvd_fuse_points(hip.ptr(lat), hip.ptr(rgb), hip.ptr(cams), hip.ptr(lin), hip.ptr(xyz), hip.ptr(color), hip.ptr(sup),
                                 hip.ptr(con), hip.ptr(fl), 1, V, S, up, ds, dsh, lo, hi, tau, stage, hip.stream())

    def compact():
        hip.check(L.mvd_compact_points(hip.ptr(xyz), hip.ptr(color), hip.ptr(sup), hip.ptr(con), hip.ptr(fl), n, 0, 255, hip.ptr(oxyz),
                                       hip.ptr(ocolor), hip.ptr(osup), hip.ptr(oidx), hip.ptr(count), hip.ptr(scratch), nbytes, hip.stream()))

    rig_dev = rig.to(dev)
    rule = lambda: torch_rule(lat, rig_dev, lin, V, S, up, ds, dsh, lo, hi, tau)
    lds_fits = fuse(hip.FUSE_STAGE_LDS) == 0
    hip.check(fuse(hip.FUSE_STAGE_GLOBAL))
    torch.cuda.synchronize()
    ref = (sup.clone(), con.clone(), xyz.clone())
    forms = {"global": hip.FUSE_STAGE_GLOBAL}
    if lds_fits:
        forms["lds"] = hip.FUSE_STAGE_LDS
        hip.check(fuse(hip.FUSE_STAGE_LDS))
        torch.cuda.synchronize()
        if not (torch.equal(sup, ref[0]) and torch.equal(con, ref[1]) and torch.equal(xyz, ref[2])):
            raise SystemExit(f"bench_fuse: the two forms of the kernel differ at V={V} up={up}")
    ts, tc = rule()
    mismatch = float(((ts != ref[0].long()) | (tc != ref[1].long())).float().mean())
    res = dict(metric="fuse_views", V=V, S=S, up=up, points=n, lds_bytes=(V * S * S + V * 20) * 4)
    t = {name: _timed(lambda st=st: hip.check(fuse(st)), blocks, block_seconds) for name, st in forms.items()}
    t["auto"] = _timed(lambda: hip.check(fuse(hip.FUSE_STAGE_AUTO)), blocks, block_seconds)
    for name, key in (("auto", "us_per_fuse_launch"), ("global", "us_per_fuse_launch_global"), ("lds", "us_per_fuse_launch_lds")):
        if name in t:
            res.update({key: t[name]["med"], key + "_min": t[name]["min"], key + "_max": t[name]["max"]})
    c = _timed(compact, blocks, block_seconds)
    r = _timed(rule, blocks, block_seconds)
    res.update(us_per_compaction=c["med"], us_per_compaction_min=c["min"], us_per_compaction_max=c["max"], kept_points=int(count.item()),
               us_per_torch_rule=r["med"], us_per_torch_rule_min=r["min"], us_per_torch_rule_max=r["max"],
               torch_over_fuse=round(r["med"] / t["auto"]["med"], 1), torch_count_mismatch_share=mismatch, blocks=blocks,
               reps_fuse=t["auto"]["reps"], reps_torch=r["reps"], gpu=torch.cuda.get_device_name(0))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, nargs="*", default=[8, 16, 24])
    ap.add_argument("--up", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--latent", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-seconds", type=float, default=0.2)
    a = ap.parse_args()
    if a.blocks < 3:
        ap.error("--blocks must be >= 3")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_fuse: no GPU visible (there is no CPU path)")
    for V in a.views:
        for up in a.up:
            print(json.dumps(run_one(V, up, a.latent, a.blocks, a.block_seconds)), flush=True)


if __name__ == "__main__":
    main()
