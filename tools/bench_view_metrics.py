#!/usr/bin/env python
"""The view metrics (mvd_image_metrics, mvd_depth_metrics; mvdfusion_amd/view_metrics.py) next to the same rules written in torch ops.

Workloads: --views images of 3 x --size x --size with the 11-tap sigma = 1.5 window and a mask, and --views depth maps of
--depth-size x --depth-size with a validity map, scale-and-shift aligned.  One JSON line per workload:
  us_per_call           one entry call, every output but the SSIM map (what compare_images / compare_depth enqueue)
  us_per_call_map       the image entry with the SSIM map written too
  us_per_call_torch     the header's rule with torch ops on the same device: for the images a grouped fp64 conv2d per pass (horizontal,
                        then vertical) over the five moment maps and masked sums; for depth masked fp64 reductions
  max_abs_diff          max|kernel - torch| of the per-image figures (two fp64 evaluations in different orders; not asserted)
Every figure is the median over --blocks blocks of HIP-event times on torch's current stream, after a warm-up; a block is --reps calls
between two events.  min / max give the spread.  Nothing is asserted.

  python tools/bench_view_metrics.py
  python tools/bench_view_metrics.py --views 8 --size 256 --depth-size 32

There is no CPU path: without a GPU this exits with an error.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_render import _event_blocks   # noqa: E402


def torch_images(a, b, mask, weights, c1, c2):
    """mvd_image_metrics' rule with torch ops: (sq_sum, ssim_sum) per image, fp64."""
    import torch
    import torch.nn.functional as F
    B, C, H, W = a.shape
    n = len(weights)
    x, y = a.double(), b.double()
    d = x - y
    sq = (d * d * mask[:, None]).sum(dim=(1, 2, 3))
    maps = torch.cat([x, y, x * x, x * y, y * y], dim=1)
    w = torch.tensor(weights, dtype=torch.float64, device=a.device)
    G = 5 * C
    h = F.conv2d(maps, w.reshape(1, 1, 1, n).expand(G, 1, 1, n), groups=G)
    e = F.conv2d(h, w.reshape(1, 1, n, 1).expand(G, 1, n, 1), groups=G)
    mx, my, exx, exy, eyy = e.split(C, dim=1)
    sxx, sxy, syy = exx - mx * mx, exy - mx * my, eyy - my * my
    ssim = ((2.0 * mx * my + c1) * (2.0 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
    r = n // 2
    centre = mask[:, None, r:H - r, r:W - r]
    return sq, torch.where(centre != 0, ssim, torch.zeros_like(ssim)).sum(dim=(1, 2, 3))


def torch_depth(pred, target, valid):
    """mvd_depth_metrics' rule (MVD_DEPTH_ALIGN_SCALE_SHIFT) with torch ops: (fit (B, 2), sums (B, 4), counts (B, 5))."""
    import torch
    ok = (valid != 0) & torch.isfinite(pred) & torch.isfinite(target) & (pred > 0) & (target > 0)
    p, t = torch.where(ok, pred, torch.ones_like(pred)).double(), torch.where(ok, target, torch.ones_like(target)).double()
    m = ok.double()
    red = lambda v: (v * m).sum(dim=(1, 2))
    n, Sp, St, Spp, Spt = m.sum(dim=(1, 2)), red(p), red(t), red(p * p), red(p * t)
    det = n * Spp - Sp * Sp
    s, b = (n * Spt - Sp * St) / det, (Spp * St - Sp * Spt) / det
    q = s[:, None, None] * p + b[:, None, None]
    kept = ok & (q > 0)
    q = torch.where(kept, q, torch.ones_like(q))
    tk = torch.where(kept, t, torch.ones_like(t))
    k = kept.double()
    d = q - tk
    l = torch.log(q) - torch.log(tk)
    r = torch.maximum(q / tk, tk / q)
    sums = torch.stack([(v * k).sum(dim=(1, 2)) for v in (d.abs() / tk, d * d / tk, d * d, l * l)], dim=1)
    counts = torch.stack([(kept & (r < th)).sum(dim=(1, 2)) for th in (1.25, 1.5625, 1.953125)] + [kept.sum(dim=(1, 2)), (ok & ~kept).sum(dim=(1, 2))],
                         dim=1)
    return torch.stack([s, b], dim=1), sums, counts


def run_images(B, P, blocks, reps):
    import torch
    from mvdfusion_amd import hip, view_metrics as vm
    L, p = hip.lib(), hip.ptr
    g = torch.Generator().manual_seed(B)
    a = torch.rand(B, 3, P, P, generator=g).cuda()
    b = (a + 0.05 * torch.randn(B, 3, P, P, generator=g).cuda()).clamp(0, 1).contiguous()
    mask = (torch.rand(B, P, P, generator=g) < 0.6).to(torch.uint8).cuda()
    weights = vm.ssim_window(11, 1.5)
    table = (ctypes.c_double * 11)(*weights)
    c1, c2 = 1e-4, 9e-4
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device="cuda")
    i64 = lambda *s: torch.empty(*s, dtype=torch.int64, device="cuda")
    sq, cnt, ss, sc, smap = f64(B), i64(B), f64(B), i64(B), f64(B, 3, P - 10, P - 10)
    nbytes = int(L.mvd_image_metrics_scratch(B, 3, P, P, 11))
    scratch = i64(max(nbytes // 8, 1))

    def call(with_map):
        hip.check(L.mvd_image_metrics(p(a), p(b), p(mask), B, 3, P, P, table, 11, c1, c2, p(sq), p(cnt), p(ss), p(sc),
                                      p(smap) if with_map else None, p(scratch), nbytes, hip.stream()))

    t_call = _event_blocks(lambda: call(False), blocks, reps)
    t_map = _event_blocks(lambda: call(True), blocks, reps)
    ref = {}

    def rule():
        ref["sq"], ref["ssim"] = torch_images(a, b, mask, weights, c1, c2)

    t_torch = _event_blocks(rule, blocks, max(reps // 4, 1))
    call(False)
    torch.cuda.synchronize()
    res = dict(metric="image_metrics", views=B, C=3, H=P, W=P, window=11, scratch_bytes=nbytes,
               max_abs_diff_sq=float((sq - ref["sq"]).abs().max()), max_abs_diff_ssim=float((ss - ref["ssim"]).abs().max()))
    for key, t in (("us_per_call", t_call), ("us_per_call_map", t_map), ("us_per_call_torch", t_torch)):
        res.update({key: t["med"], key + "_min": t["min"], key + "_max": t["max"]})
    res.update(blocks=blocks, reps=reps, lib=os.path.basename(hip.LIB_PATHS[hip.OPERAND_FORMAT]), gpu=torch.cuda.get_device_name(0))
    return res


def run_depth(B, S, blocks, reps):
    import torch
    from mvdfusion_amd import hip
    L, p = hip.lib(), hip.ptr
    g = torch.Generator().manual_seed(1000 + B)
    t = (0.5 + 2.0 * torch.rand(B, S, S, generator=g)).cuda()
    pr = (t * (0.8 + 0.4 * torch.rand(B, S, S, generator=g).cuda()) * 1.3 + 0.05).contiguous()
    valid = (torch.rand(B, S, S, generator=g) < 0.7).to(torch.uint8).cuda()
    fit = torch.empty(B, 2, dtype=torch.float64, device="cuda")
    sums = torch.empty(B, 4, dtype=torch.float64, device="cuda")
    counts = torch.empty(B, 5, dtype=torch.int64, device="cuda")
    nbytes = int(L.mvd_depth_metrics_scratch(B, S, S))
    scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device="cuda")

    def call():
        hip.check(L.mvd_depth_metrics(p(pr), p(t), p(valid), B, S, S, hip.DEPTH_ALIGN_SCALE_SHIFT, None, p(fit), p(sums), p(counts), p(scratch),
                                      nbytes, hip.stream()))

    t_call = _event_blocks(call, blocks, reps)
    ref = {}

    def rule():
        ref["fit"], ref["sums"], ref["counts"] = torch_depth(pr, t, valid)

    t_torch = _event_blocks(rule, blocks, max(reps // 4, 1))
    call()
    torch.cuda.synchronize()
    res = dict(metric="depth_metrics", views=B, H=S, W=S, align="scale_shift", scratch_bytes=nbytes,
               max_abs_diff_fit=float((fit - ref["fit"]).abs().max()), max_abs_diff_sums=float((sums - ref["sums"]).abs().max()),
               counts_equal=bool(torch.equal(counts, ref["counts"])))
    for key, tm in (("us_per_call", t_call), ("us_per_call_torch", t_torch)):
        res.update({key: tm["med"], key + "_min": tm["min"], key + "_max": tm["max"]})
    res.update(blocks=blocks, reps=reps, lib=os.path.basename(hip.LIB_PATHS[hip.OPERAND_FORMAT]), gpu=torch.cuda.get_device_name(0))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--depth-size", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    a = ap.parse_args()
    if a.blocks < 3:
        ap.error("--blocks must be >= 3")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_view_metrics: no GPU visible (there is no CPU path)")
    for B in a.views:
        print(json.dumps(run_images(B, a.size, a.blocks, a.reps)), flush=True)
    for B in a.views:
        print(json.dumps(run_depth(B, a.depth_size, a.blocks, a.reps)), flush=True)


if __name__ == "__main__":
    main()
