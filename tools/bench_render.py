#!/usr/bin/env python
"""Point rendering (mvd_render_points, mvdfusion_amd/fusion.py render_points) against the same rule written with torch ops on the GPU.

One workload = (n points, M cameras, radius r) at P = 256: n points uniform on a sphere of radius 0.6 at the world origin, in random
order, seen from a ring rig (distance 1.5, elevation 30 degrees, M azimuths); defaults n in {65 536, 1 048 576} x M in {1, 8} x r in
{0, 1, 2}.  One JSON line per workload:
  us_per_render         one mvd_render_points call: the z-buffer fill, the splat kernel and the resolve kernel
  us_per_splat          the splat kernel alone (mvd_render_points_stages; the z-buffer is refilled, untimed, before every launch)
  us_per_torch_rule     the same rule in torch ops in fp32 on the GPU: projection, int64 keys (depth bits << 32 | point), one
                        scatter_reduce_(amin) over all (point, camera, footprint pixel) candidates, unpacking -- what a user would otherwise write
  us_per_torch_scatter  ... with the keys and pixel indices built once outside the timed region: the z-buffer fill, scatter_reduce_, unpacking
  index_mismatch        pixels whose torch index differs from the kernel's after the timed calls (the same integer minimum: expected 0)
Every figure is the median over --blocks blocks of HIP-event times on torch's current stream, after a warm-up of every launch; a block
is --reps calls between two events (the splat kernel: an event pair around every launch, summed).  min / max give the spread.

  python tools/bench_render.py
  python tools/bench_render.py --points 1048576 --cameras 8 --radius 1

There is no CPU path: without a GPU this exits with an error.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _event_blocks(fn, blocks, reps, before=None):
    """Median / min / max µs per call of fn over `blocks` blocks; with `before`, before() runs untimed in front of every fn()."""
    import torch
    for _ in range(3):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(blocks):
        if before is None:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / reps)
        else:
            pairs = []
            for _ in range(reps):
                before()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                pairs.append((a, b))
            torch.cuda.synchronize()
            times.append(sum(a.elapsed_time(b) for a, b in pairs) * 1e3 / reps)
    return dict(med=round(statistics.median(times), 2), min=round(min(times), 2), max=round(max(times), 2))


def ring_rig(M):
    import torch
    from mvdfusion_amd.cameras import Cameras, look_at_view_transform
    R, T = look_at_view_transform(1.5, torch.full((M,), 30.0), torch.arange(M, dtype=torch.float32) * (360.0 / M))
    return Cameras(R, T, torch.full((M, 2), 2.1875), torch.zeros(M, 2))


def torch_candidates(xyz, cams, P, r, znear):
    """(pix, key): per (point, camera, footprint pixel) the flat pixel of the (M, P, P) image -- M * P * P for a pixel outside it -- and the
    int64 key of include/mvd_hip.h's depth rule, in fp32 and the kernel's operation order."""
    import torch
    n, M = xyz.shape[0], len(cams)
    total = M * P * P
    lo, hi, P2 = -(r + 2.0), P + r + 1.0, 0.5 * P
    ids = torch.arange(n, device=xyz.device)
    pixs, keys = [], []
    for cam in range(M):
        R, T, f, p = cams.R[cam], cams.T[cam], cams.focal_length[cam], cams.principal_point[cam]
        xc = [xyz[:, 0] * R[0, j] + xyz[:, 1] * R[1, j] + xyz[:, 2] * R[2, j] + T[j] for j in range(3)]
        zc = xc[2]
        cx = (1.0 - (f[0] * xc[0] / zc + p[0])) * P2 - 0.5
        cy = (1.0 - (f[1] * xc[1] / zc + p[1])) * P2 - 0.5
        ok = (zc > znear) & (cx >= lo) & (cx <= hi) & (cy >= lo) & (cy <= hi)
        px = torch.where(ok, (cx + 0.5).floor(), torch.zeros_like(cx)).long()
        py = torch.where(ok, (cy + 0.5).floor(), torch.zeros_like(cy)).long()
        key = (zc.view(torch.int32).long() << 32) | ids
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                x, y = px + dx, py + dy
                inside = ok & (x >= 0) & (x < P) & (y >= 0) & (y < P)
                pixs.append(torch.where(inside, (cam * P + y) * P + x, torch.full_like(x, total)))
                keys.append(key)
    return torch.cat(pixs), torch.cat(keys)


def torch_scatter(pix, key, M, P):
    import torch
    empty = torch.iinfo(torch.int64).max
    z = torch.full((M * P * P + 1,), empty, dtype=torch.int64, device=pix.device)
    z.scatter_reduce_(0, pix, key, "amin", include_self=True)
    z = z[:-1]
    return torch.where(z == empty, torch.full_like(z, -1), z & 0xffffffff).reshape(M, P, P)


def run_one(n, M, r, P, blocks, reps):
    import torch
    from mvdfusion_amd import hip
    from mvdfusion_amd.cameras import pack_cameras
    L = hip.lib()
    dev = "cuda"
    g = torch.Generator().manual_seed(1000 * M + r)
    d = torch.randn(n, 3, generator=g)
    xyz = (0.6 * d / d.norm(dim=1, keepdim=True)).to(dev)
    color = torch.rand(n, 3, generator=g).to(dev)
    rig = ring_rig(M)
    cams = pack_cameras(rig).to(dev)
    start = torch.tensor([0, n], dtype=torch.int32).to(dev)
    index = torch.empty(M, P, P, dtype=torch.int32, device=dev)
    depth = torch.empty(M, P, P, device=dev)
    rgb = torch.empty(M, 3, P, P, device=dev)
    nbytes = int(L.mvd_render_points_scratch(M, P))
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    bg = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    znear = 1e-3

    def stages(which):
        hip.check(L.mvd_render_points_stages(hip.ptr(xyz), hip.ptr(color), hip.ptr(start), hip.ptr(cams), n, 1, M, P, r, znear, float("inf"),
                                             bg, hip.ptr(index), hip.ptr(depth), hip.ptr(rgb), hip.ptr(scratch), nbytes, which, hip.stream()))

    def render():
        hip.check(L.mvd_render_points(hip.ptr(xyz), hip.ptr(color), hip.ptr(start), hip.ptr(cams), n, 1, M, P, r, znear, float("inf"), bg,
                                      hip.ptr(index), hip.ptr(depth), hip.ptr(rgb), hip.ptr(scratch), nbytes, hip.stream()))

    rig_dev = rig.to(dev)
    render()
    pix, key = torch_candidates(xyz, rig_dev, P, r, znear)
    want = torch_scatter(pix, key, M, P)
    t_render = _event_blocks(render, blocks, reps)
    t_splat = _event_blocks(lambda: stages(hip.RENDER_SPLAT), blocks, reps, before=lambda: stages(hip.RENDER_FILL))
    render()                                   # compared AFTER the timed calls: hundreds of renders through the same z-buffer
    torch.cuda.synchronize()
    mismatch = int((want != index.long()).sum())
    t_scatter = _event_blocks(lambda: torch_scatter(pix, key, M, P), blocks, max(2, reps // 10))
    del pix, key
    t_rule = _event_blocks(lambda: torch_scatter(*torch_candidates(xyz, rig_dev, P, r, znear), M, P), blocks, max(2, reps // 10))
    res = dict(metric="render_points", points=n, M=M, r=r, P=P, hit_share=round(float((index >= 0).float().mean()), 3),
               index_mismatch=mismatch)
    for name, t in (("us_per_render", t_render), ("us_per_splat", t_splat), ("us_per_torch_scatter", t_scatter), ("us_per_torch_rule", t_rule)):
        res.update({name: t["med"], name + "_min": t["min"], name + "_max": t["max"]})
    res.update(torch_rule_over_render=round(t_rule["med"] / t_render["med"], 1), torch_scatter_over_render=round(t_scatter["med"] / t_render["med"], 1),
               blocks=blocks, reps=reps, lib=os.path.basename(hip.LIB_PATHS[hip.OPERAND_FORMAT]), gpu=torch.cuda.get_device_name(0))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, nargs="*", default=[65536, 1048576])
    ap.add_argument("--cameras", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--radius", type=int, nargs="*", default=[0, 1, 2])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    if a.blocks < 3:
        ap.error("--blocks must be >= 3")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_render: no GPU visible (there is no CPU path)")
    for n in a.points:
        for M in a.cameras:
            for r in a.radius:
                print(json.dumps(run_one(n, M, r, a.size, a.blocks, a.reps)), flush=True)


if __name__ == "__main__":
    main()
