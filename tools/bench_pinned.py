#!/usr/bin/env python
"""Pinned views (DDIMSampler.sample(known_latents=...)) against the unpinned step: time per replayed denoising step and per pin launch.

One workload = (V views, K pinned) at S = 32, D = 1, full width (model_channels 320), cfg 2.5; K = 0 is the plain step.  A pinned step is
the engine of the query range [K, V) -- GridAttn query rows and UNet rows for the V - K free views only -- with mvd_pin_views in front.
Two figures per workload, each the median of --blocks blocks of --block repetitions with a device synchronise at the end of every block
(min / max give the spread), as tools/bench_window.py measures:
  ms_per_step        one graph replay of the engine (pin + GridAttn + the CFG pair of UNet passes + the DDIM update)
  us_per_pin_launch  mvd_pin_views alone (mode 1), on the engine's own buffers; K = 0 has none
One JSON line per workload; pinned lines carry the ratio to the plain run of the same V in the same invocation and (V - K) / V next to it.

  python tools/bench_pinned.py                      # V = 8 with K in {0, 2, 4}, then V = 15 with K in {0, 4}
  python tools/bench_pinned.py --views 15 --pinned 0 4

All workloads share one model in one process.  There is no CPU path: without a GPU this exits with an error.
"""
import argparse
import json
import os
import statistics
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


def run_one(m, V, K, S, D, warmup, blocks, block, cfg_scale=2.5):
    import torch
    from mvdfusion_amd import hip
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.engine import ddim_step_table
    inp = syn.make_inputs(V, S, seed=0)
    dn, sn = syn.step_noise(V, S, D, 50, seed=0)
    eng = m.engine(V, S, D, cfg_scale != 1.0, q0=K, Vq=V - K) if K else m.engine(V, S, D, cfg_scale != 1.0)
    eng.set_conditioning(inp["batch_cameras"], inp["input_latents"].cuda(), inp["input_cameras"], inp["clip_v_embed"].cuda())
    st, dd = m.ddim.tables()
    eng.set_schedule(ddim_step_table(st, dd, [49 - i for i in range(50)]), dn, sn)
    eng.x.copy_(inp["x_T"])
    g = torch.Generator().manual_seed(1)
    try:
        if K:
            eng.set_pin(1, torch.randn(K, 5, S, S, generator=g) * 0.7, torch.randn(50, K, 5, S, S, generator=g))

        def step():
            if eng.done == eng.n_rows:          # wrap to a fresh sample every 50 steps
                eng.rewind()
                eng.x.copy_(inp["x_T"])
            eng.step(cfg_scale, do_update=True, use_graph=True)

        t0 = time.time()
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        log(f"[bench_pinned] V={V} K={K}: warm-up ({warmup} steps, incl. tuning + capture) {time.time() - t0:.1f} s")
        s_med, s_min, s_max = _blocks(step, blocks, block)
        if not bool(torch.isfinite(eng.x).all()):
            raise SystemExit(f"bench_pinned: non-finite latents at V={V} K={K}")
        res = dict(metric="pinned_views", V=V, K=K, free_views=V - K, free_share=round((V - K) / V, 3), S=S, D=D, model_channels=320,
                   cfg_scale=cfg_scale, ms_per_step=round(s_med, 3), ms_per_step_min=round(s_min, 3), ms_per_step_max=round(s_max, 3))
        if K:
            eng.rewind()
            L = hip.lib()

            def launch():
                hip.check(L.mvd_pin_views(hip.ptr(eng.x), hip.ptr(eng.x0), hip.ptr(eng.known), hip.ptr(eng.pin_noise), K * 5 * S * S,
                                          hip.ptr(eng.steps), hip.ptr(eng.iter), 1, V, K, S, 1, hip.stream()))

            for _ in range(3):
                launch()
            p_med, p_min, p_max = _blocks(launch, blocks, 10 * block)
            res.update(us_per_pin_launch=round(p_med * 1e3, 2), us_per_pin_launch_min=round(p_min * 1e3, 2),
                       us_per_pin_launch_max=round(p_max * 1e3, 2))
    finally:
        eng.clear_pin()
    res.update(blocks=blocks, replays_per_block=block, gpu=torch.cuda.get_device_name(0))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, nargs="*", default=None)
    ap.add_argument("--pinned", type=int, nargs="*", default=None, help="0 = the plain step")
    ap.add_argument("--latent", type=int, default=32)
    ap.add_argument("--depth-samples", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--block", type=int, default=20)
    a = ap.parse_args()
    if a.blocks < 3 or a.block < 1:
        ap.error("--blocks must be >= 3 and --block >= 1")
    if a.views is None and a.pinned is None:
        work = [(8, 0), (8, 2), (8, 4), (15, 0), (15, 4)]
    else:
        work = [(V, K) for V in (a.views or [8]) for K in (a.pinned if a.pinned is not None else [0, 2, 4])]
    for V, K in work:
        if not 0 <= K < V:
            ap.error(f"--pinned {K} of --views {V}: 0 <= K < V")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pinned: no GPU visible (there is no CPU path)")
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.configs import model_config
    from mvdfusion_amd.viewfusion_zero_depth_rgb import ViewFusion
    t0 = time.time()
    with syn.skip_default_init():
        m = ViewFusion(**model_config(320, D=a.depth_samples, S=a.latent))
    syn.fill_module_(m)
    m = m.cuda().eval()
    log(f"[bench_pinned] model built in {time.time() - t0:.1f} s")
    plain = {}
    for V, K in work:
        res = run_one(m, V, K, a.latent, a.depth_samples, a.warmup, a.blocks, a.block)
        if K == 0:
            plain[V] = res
        elif V in plain:
            res["step_vs_plain"] = round(res["ms_per_step"] / plain[V]["ms_per_step"], 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
