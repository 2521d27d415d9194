#!/usr/bin/env python
"""Windowed cross-view aggregation (GridAttn keep_top_k_views) against the full one: time per denoising step and per fused launch.

One workload = (V views, top_k) at S = 32, D = 1, full width (model_channels 320), cfg 2.5; top_k = 0 is the full aggregation (no
window).  Two figures per workload, each the median of --blocks blocks of --block repetitions with a device synchronise at the end of
every block (min / max give the spread), as tools/bench_scenes.py measures:
  ms_per_step          one graph replay of the engine (GridAttn + the CFG pair of UNet passes + the DDIM update)
  ms_per_fused_launch  mvd_gridattn_fused_window alone, on the engine's own buffers
One JSON line per workload; windowed lines carry the ratios to the full run of the same V in the same invocation.

  python tools/bench_window.py                      # V in {8, 15} x top_k in {0, 2, 4}, then V = 24 x top_k in {2, 4} (no full run: a
                                                    # point would have 24 rows), each in a fresh child process under --timeout seconds
  python tools/bench_window.py --views 15 --top-k 4 # one workload in this process

There is no CPU path: without a GPU this exits with an error.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def _blocks(fn, blocks, block):
    import torch
    times = []
    for _ in range(blocks):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(block):
            fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) / block * 1e3)
    return statistics.median(times), min(times), max(times)


def run_one(V, top_k, S, D, warmup, blocks, block, cfg_scale=2.5):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_window: no GPU visible (there is no CPU path)")
    from mvdfusion_amd import hip
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.configs import model_config
    from mvdfusion_amd.engine import ddim_step_table
    from mvdfusion_amd.viewfusion_zero_depth_rgb import ViewFusion
    cfg = model_config(320, D=D, S=S)
    if top_k:
        va = cfg["view_attn_config"]
        cfg["view_attn_config"] = dict(va, params=dict(va["params"], keep_top_k_views=True, top_k=top_k))
    t0 = time.time()
    with syn.skip_default_init():
        m = ViewFusion(**cfg)
    syn.fill_module_(m)
    m = m.cuda().eval()
    ga = m.view_attn
    W, R = ga.window, ga.rows_per_point(V)
    log(f"[bench_window] V={V} top_k={top_k} (W={W}): model built in {time.time() - t0:.1f} s")
    inp = syn.make_inputs(V, S, seed=0)
    dn, sn = syn.step_noise(V, S, D, 50, seed=0)
    eng = m.engine(V, S, D, cfg_scale != 1.0)
    eng.set_conditioning(inp["batch_cameras"], inp["input_latents"].cuda(), inp["input_cameras"], inp["clip_v_embed"].cuda())
    st, dd = m.ddim.tables()
    eng.set_schedule(ddim_step_table(st, dd, [49 - i for i in range(50)]), dn, sn)
    eng.x.copy_(inp["x_T"])

    def step():
        if eng.done == eng.n_rows:          # wrap to a fresh sample every 50 steps
            eng.rewind()
            eng.x.copy_(inp["x_T"])
        eng.step(cfg_scale, do_update=True, use_graph=True)

    t0 = time.time()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    log(f"[bench_window] V={V} top_k={top_k}: warm-up ({warmup} steps, incl. tuning + capture) {time.time() - t0:.1f} s")
    s_med, s_min, s_max = _blocks(step, blocks, block)
    if not bool(torch.isfinite(eng.x).all()):
        raise SystemExit(f"bench_window: non-finite latents at V={V} top_k={top_k}")
    # the fused launch alone, on the buffers the step left behind
    ctx, L = eng.ctx, hip.lib()
    nseq = V * S * S * D
    assert ga.fused_supported(V, nseq * R), (V, R)
    stream, vecs = ga.packed_fused(ctx.device)
    feat, in_feat = ctx.ws.get("ga.feat", (V, S, S, 256)), ctx.ws.get("ga.infeat", (1, S, S, 256))
    pool, lin = ctx.ws.planes("ga.pool", nseq, ga.hidden_size), ctx.ws.bufs[("ga.lin", S)]
    eng.rewind()
    prec = 3 if ctx.prec_of("ga") == 3 else 4

    def launch():
        hip.check(L.mvd_gridattn_fused_window(hip.ptr(eng.x), hip.ptr(eng.depth_noise), hip.ptr(eng.steps), hip.ptr(eng.iter), hip.ptr(lin),
                                              hip.ptr(feat), hip.ptr(in_feat), hip.ptr(eng.cams), hip.ptr(eng.in_cam), hip.ptr(stream),
                                              hip.ptr(vecs), hip.ptr(pool), 1, V, 0, V, S, D, float(ga.depth_scale), float(ga.depth_shift),
                                              prec, 0, 0, W, hip.stream()))

    for _ in range(3):
        launch()
    f_med, f_min, f_max = _blocks(launch, blocks, block)
    Vp = 1 << max(R - 1, 0).bit_length()
    return dict(metric="windowed_gridattn", V=V, top_k=top_k, window=W, rows_per_point=R, padded_slots=Vp, S=S, D=D, model_channels=320,
                cfg_scale=cfg_scale, fused_products=prec, ms_per_step=round(s_med, 3), ms_per_step_min=round(s_min, 3),
                ms_per_step_max=round(s_max, 3), ms_per_fused_launch=round(f_med, 4), ms_per_fused_launch_min=round(f_min, 4),
                ms_per_fused_launch_max=round(f_max, 4), blocks=blocks, replays_per_block=block, gpu=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, nargs="*", default=None)
    ap.add_argument("--top-k", type=int, nargs="*", default=None, help="0 = the full aggregation")
    ap.add_argument("--latent", type=int, default=32)
    ap.add_argument("--depth-samples", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--timeout", type=float, default=300.0, help="time limit of one workload's child process (seconds)")
    a = ap.parse_args()
    if a.blocks < 3 or a.block < 1:
        ap.error("--blocks must be >= 3 and --block >= 1")
    if a.views is None and a.top_k is None:
        work = [(V, k) for V in (8, 15) for k in (0, 2, 4)] + [(24, 2), (24, 4)]
    else:
        work = [(V, k) for V in (a.views or [15]) for k in (a.top_k if a.top_k is not None else [0, 2, 4])]
    if len(work) == 1:
        V, k = work[0]
        print(json.dumps(run_one(V, k, a.latent, a.depth_samples, a.warmup, a.blocks, a.block)), flush=True)
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_window: no GPU visible (there is no CPU path)")
    full = {}
    for V, k in work:
        cmd = [sys.executable, os.path.abspath(__file__), "--views", str(V), "--top-k", str(k), "--latent", str(a.latent),
               "--depth-samples", str(a.depth_samples), "--warmup", str(a.warmup), "--blocks", str(a.blocks), "--block", str(a.block)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            log(f"[bench_window] V={V} top_k={k}: exceeded {a.timeout:.0f} s; stopping")
            raise SystemExit(124)
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            log(f"[bench_window] V={V} top_k={k}: exit status {r.returncode}; stopping")
            raise SystemExit(r.returncode if r.returncode > 0 else 1)
        res = json.loads(r.stdout.strip().splitlines()[-1])
        if k == 0:
            full[V] = res
        elif V in full:
            res["step_vs_full"] = round(res["ms_per_step"] / full[V]["ms_per_step"], 3)
            res["fused_launch_vs_full"] = round(res["ms_per_fused_launch"] / full[V]["ms_per_fused_launch"], 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
