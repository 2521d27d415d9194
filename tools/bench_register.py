#!/usr/bin/env python
"""Global registration (mvd_register_score, mvd_register_select, mvdfusion_amd/fusion.py register_geometry): the whole call and its parts at
the defaults, the score against the same sum in torch ops, and what the truncated walk buys.

One workload = n: the bulged ellipsoid of tests/align_f64.py, n source points moved by the inverse of (135 degrees about (0.3, -1, 0.5),
t = (0.2, -0.1, 0.15)) against an independent resampling of n target points, one scene.  No point has an exact partner.
One JSON line per n (defaults 4 096, 65 536, 1 048 576):
  us_register        one fusion.register_geometry call at the defaults, host work and its host reads included
  us_build           MVD_NN_BUILD of the target's grid
  us_score           mvd_register_score of the sample (REGISTER_SAMPLES rows) under the REGISTER_ROTATIONS hypotheses, trunc as the default
  us_score_no_trunc  the same call with trunc2 = 1e30, so that nothing truncates: the same kernel walks until the nearest target is
                     proven -- the difference is what the early stop buys; up to --no-trunc-max target points (a far point walks
                     many shells of empty cells: seconds per call at a million)
  us_score_brute     the same score with MVD_NN_BRUTE, up to --brute-max target points
  us_score_full      mvd_register_score of the FULL source under the REGISTER_CANDIDATES refined transforms
  us_select          mvd_register_select of K from H
  us_refine          the K refinements: K mvd_align_icp calls of refine_iters iterations on the full source (each rebuilds the grid)
  us_icp_iter        us_refine / (K * (refine_iters + 1)): one ICP pass on the same box, for scale
  us_torch_score     the same scoring in torch ops: per chunk of hypotheses, torch.cdist to the target, min, clamp, sum -- in fp32 by
                     the matrix form, so not the same bits -- up to --torch-max target points
  err                |matrix - truth|_max of the registered result -- reported, nothing is asserted
Every time is the median over --blocks blocks of HIP-event times on torch's current stream, after a warm-up of every launch
(tools/bench_nearest.py: _event_blocks); min / max give the spread.

  python tools/bench_register.py
  python tools/bench_register.py --sizes 65536 --blocks 7

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

from bench_align import ellipsoid                         # noqa: E402
from bench_nearest import _event_blocks                   # noqa: E402


def truth_matrix():
    import torch
    a = torch.tensor([0.3, -1.0, 0.5], dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    th = math.radians(135.0)
    M = torch.eye(4, dtype=torch.float64)
    M[:3, :3] = torch.eye(3, dtype=torch.float64) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    M[:3, 3] = torch.tensor([0.2, -0.1, 0.15], dtype=torch.float64)
    return M


def torch_score(sample, target, hyp, trunc2, chunk):
    """sum_i min(min_j |R_h p_i + t_h - q_j|^2, trunc2) per hypothesis: cdist in chunks of hypotheses."""
    import torch
    m = hyp.reshape(-1, 3, 4).float()
    out = []
    for a in range(0, m.shape[0], chunk):
        moved = torch.einsum("hrc,ic->hir", m[a:a + chunk, :, :3], sample) + m[a:a + chunk, None, :, 3]
        d = torch.cdist(moved.reshape(1, -1, 3), target[None]).min(dim=2).values.reshape(moved.shape[0], -1)
        out.append((d * d).clamp(max=trunc2).double().sum(1))
    return torch.cat(out)


def run_one(n, a):
    import torch
    from mvdfusion_amd import fusion, hip
    L = hip.lib()
    T = truth_matrix()
    inv = torch.linalg.inv(T)
    src = (ellipsoid(n, 1).double() @ inv[:3, :3].T + inv[:3, 3]).float().cuda().contiguous()
    tgt = ellipsoid(n, 2).cuda().contiguous()
    H, K, refine = fusion.REGISTER_ROTATIONS, fusion.REGISTER_CANDIDATES, 20
    start = torch.tensor([0, n], dtype=torch.int32).cuda()
    quat = fusion.rotation_grid(H)
    hyp, _, sample, sample_start, trunc2 = fusion._register_inputs(src, start, tgt, start, 1, fusion._quat_matrix(quat), False,
                                                                    fusion.REGISTER_SAMPLES, None)
    m = int(sample.shape[0])
    res = dict(metric="register_geometry", n=n, rotations=H, samples=m, candidates=K, refine_iters=refine, trunc=round(math.sqrt(trunc2), 6),
               method_auto="grid" if int(L.mvd_nearest_points_scratch(n, 1, hip.NN_AUTO, 0)) else "brute")
    reg = fusion.register_geometry(src, tgt)
    torch.cuda.synchronize()
    res["err"] = float((reg.matrix[0].cpu() - T).abs().max())
    res["candidate_score"] = [round(float(v), 6) for v in reg.candidate_score[0].cpu()]
    res["chosen"] = int(reg.chosen[0])
    times = {"us_register": _event_blocks(lambda: fusion.register_geometry(src, tgt), a.blocks, a.block_ms)}

    def scorer(points, pstart, hyps, method):
        nbytes = fusion._register_scratch(int(points.shape[0]), n, 1, int(hyps.shape[1]), method, 0)
        scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device="cuda")
        fusion._register_build(tgt, start, 1, method, 0, scratch, nbytes)
        return lambda t2: fusion._register_score(points, pstart, tgt, start, 1, hyps, t2, method, 0, scratch, nbytes), scratch, nbytes

    score_sample, scratch, nbytes = scorer(sample, sample_start, hyp, hip.NN_AUTO)
    times["us_build"] = _event_blocks(lambda: fusion._register_build(tgt, start, 1, hip.NN_AUTO, 0, scratch, nbytes), a.blocks, a.block_ms)
    times["us_score"] = _event_blocks(lambda: score_sample(trunc2), a.blocks, a.block_ms)
    if n <= a.no_trunc_max:
        times["us_score_no_trunc"] = _event_blocks(lambda: score_sample(1e30), a.blocks, a.block_ms)
    grid_score, _ = score_sample(trunc2)
    if n <= a.brute_max:
        score_brute, _, _ = scorer(sample, sample_start, hyp, hip.NN_BRUTE)
        times["us_score_brute"] = _event_blocks(lambda: score_brute(trunc2), a.blocks, a.block_ms)
        res["brute_mismatch"] = int((score_brute(trunc2)[0].view(torch.int64) != grid_score.view(torch.int64)).sum())
    refined = reg.candidates[:, :, :3, :].reshape(1, K, 12).contiguous()
    score_full, _, _ = scorer(src, start, refined, hip.NN_AUTO)
    times["us_score_full"] = _event_blocks(lambda: score_full(trunc2), a.blocks, a.block_ms)
    qd = quat.cuda()
    cos_half = math.cos(math.radians(30.0) / 2.0)
    times["us_select"] = _event_blocks(lambda: fusion._register_select(grid_score, qd, K, cos_half), a.blocks, a.block_ms)
    top, _ = fusion._register_select(grid_score, qd, K, cos_half)
    starts = [hyp[0, int(h)].reshape(1, 12).clone() for h in top[0].clamp(min=0).tolist()]

    def refine_all():
        for tr in starts:
            fusion._align_icp(src, start, tgt, start, 1, hip.NN_AUTO, 0, refine, 0, float("inf"), tr.clone())

    times["us_refine"] = _event_blocks(refine_all, a.blocks, a.block_ms)
    if n <= a.torch_max:
        times["us_torch_score"] = _event_blocks(lambda: torch_score(sample, tgt, hyp, trunc2, a.torch_chunk), a.blocks, a.block_ms)
        ref = torch_score(sample, tgt, hyp, trunc2, a.torch_chunk)
        res["torch_rel_diff"] = float(((ref - grid_score[0]).abs() / grid_score[0]).max())
    for name, t in times.items():
        res.update({name: t["med"], name + "_min": t["min"], name + "_max": t["max"]})
    res["us_icp_iter"] = round(times["us_refine"]["med"] / (K * (refine + 1)), 2)
    if "us_score_no_trunc" in times:
        res["no_trunc_over_score"] = round(times["us_score_no_trunc"]["med"] / times["us_score"]["med"], 2)
    if "us_torch_score" in times:
        res["torch_over_score"] = round(times["us_torch_score"]["med"] / times["us_score"]["med"], 2)
    res.update(blocks=a.blocks, lib=os.path.basename(hip.LIB_PATHS[hip.OPERAND_FORMAT]), gpu=torch.cuda.get_device_name(0))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="*", default=[4096, 65536, 1048576])
    ap.add_argument("--torch-max", type=int, default=65536)
    ap.add_argument("--torch-chunk", type=int, default=16, help="hypotheses per torch.cdist call")
    ap.add_argument("--no-trunc-max", type=int, default=65536)
    ap.add_argument("--brute-max", type=int, default=65536)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-ms", type=float, default=100.0)
    a = ap.parse_args()
    if a.blocks < 3:
        ap.error("--blocks must be >= 3")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_register: no GPU visible (there is no CPU path)")
    for n in sorted(a.sizes):
        print(json.dumps(run_one(n, a)), flush=True)


if __name__ == "__main__":
    main()
