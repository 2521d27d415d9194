#!/usr/bin/env python
"""Scene-batched sampling throughput: N objects denoised together in every DDIM step (DDIMSampler.sample_scenes / StepEngine(scenes=N)).

One workload = (V views, N scenes) at S = 32, D = 1, full width (model_channels 320), cfg 2.5.  A step is one graph replay of the
N-scene engine.  After the warm-up (the first step tunes the GEMMs of the new shapes and captures the graph), the steps are timed as
--blocks blocks of --block graph replays, with a device synchronise at the end of every block; the median block gives the time per
step, min / max the spread.  One JSON line per workload: ms per batched step, scene-steps/s (= N / step time), and -- for N > 1 with
the N = 1 run of the same V in the same invocation -- the per-scene throughput ratio to N = 1.

  python tools/bench_scenes.py                       # every workload, V in {4, 15} x N in {1, 2, 4}, each in a fresh child process
                                                     # under its own time limit (--timeout seconds)
  python tools/bench_scenes.py --views 4 --scenes 2  # one workload in this process

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


def run_one(V, N, S, D, warmup, blocks, block, cfg_scale=2.5):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_scenes: no GPU visible (there is no CPU path)")
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.configs import model_config
    from mvdfusion_amd.engine import ddim_step_table
    from mvdfusion_amd.viewfusion_zero_depth_rgb import ViewFusion
    t0 = time.time()
    with syn.skip_default_init():
        m = ViewFusion(**model_config(320, D=D, S=S))
    syn.fill_module_(m)
    m = m.cuda().eval()
    log(f"[bench_scenes] V={V} N={N}: model built in {time.time() - t0:.1f} s")
    inps = [syn.make_inputs(V, S, seed=s) for s in range(N)]
    noise = [syn.step_noise(V, S, D, 50, seed=s) for s in range(N)]
    eng = m.engine(V, S, D, cfg_scale != 1.0, scenes=N)
    eng.set_conditioning_scenes([(i["batch_cameras"], i["input_latents"].cuda(), i["input_cameras"], i["clip_v_embed"].cuda())
                                 for i in inps])
    st, dd = m.ddim.tables()
    eng.set_schedule(ddim_step_table(st, dd, [49 - i for i in range(50)]), torch.cat([n[0] for n in noise], 1),
                     torch.cat([n[1] for n in noise], 1))
    eng.x.copy_(torch.cat([i["x_T"] for i in inps]))

    def steps(k):
        for _ in range(k):
            if eng.done == eng.n_rows:      # wrap to a fresh sample every 50 steps
                eng.rewind()
                eng.x.copy_(torch.cat([i["x_T"] for i in inps]))
            eng.step(cfg_scale, do_update=True, use_graph=True)

    t0 = time.time()
    steps(warmup)
    torch.cuda.synchronize()
    log(f"[bench_scenes] V={V} N={N}: warm-up ({warmup} steps, incl. tuning + capture) {time.time() - t0:.1f} s")
    times = []
    for _ in range(blocks):
        torch.cuda.synchronize()
        t = time.perf_counter()
        steps(block)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) / block * 1e3)
    if not bool(torch.isfinite(eng.x).all()):
        raise SystemExit(f"bench_scenes: non-finite latents at V={V} N={N}")
    med = statistics.median(times)
    return dict(metric="scene_batched_step", V=V, N=N, S=S, D=D, model_channels=320, cfg_scale=cfg_scale,
                ms_per_step=round(med, 3), ms_per_step_min=round(min(times), 3), ms_per_step_max=round(max(times), 3),
                scene_steps_per_s=round(N * 1e3 / med, 2), blocks=blocks, replays_per_block=block,
                gpu=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, nargs="*", default=[4, 15])
    ap.add_argument("--scenes", type=int, nargs="*", default=[1, 2, 4])
    ap.add_argument("--latent", type=int, default=32)
    ap.add_argument("--depth-samples", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--timeout", type=float, default=300.0, help="time limit of one workload's child process (seconds)")
    a = ap.parse_args()
    if a.blocks < 3 or a.block < 1:
        ap.error("--blocks must be >= 3 and --block >= 1")
    work = [(V, N) for V in a.views for N in a.scenes]
    if len(work) == 1:
        V, N = work[0]
        print(json.dumps(run_one(V, N, a.latent, a.depth_samples, a.warmup, a.blocks, a.block)), flush=True)
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_scenes: no GPU visible (there is no CPU path)")
    base = {}
    for V, N in work:
        cmd = [sys.executable, os.path.abspath(__file__), "--views", str(V), "--scenes", str(N), "--latent", str(a.latent),
               "--depth-samples", str(a.depth_samples), "--warmup", str(a.warmup), "--blocks", str(a.blocks), "--block", str(a.block)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            log(f"[bench_scenes] V={V} N={N}: exceeded {a.timeout:.0f} s; stopping")
            raise SystemExit(124)
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            log(f"[bench_scenes] V={V} N={N}: exit status {r.returncode}; stopping")
            raise SystemExit(r.returncode if r.returncode > 0 else 1)
        res = json.loads(r.stdout.strip().splitlines()[-1])
        if N == 1:
            base[V] = res["scene_steps_per_s"]
        if V in base:
            res["per_scene_vs_n1"] = round(res["scene_steps_per_s"] / base[V], 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
