"""Training-step timing on one GPU (BASELINE.json configs[4] in miniature: fwd + bwd + AdamW on one scene of V views):
the reference's loop ``loss = model(batch, cfg); optimizer.zero_grad(); loss.backward(); optimizer.step()`` on the HIP forward
and the hand-written backward kernels (mvdfusion_amd/backward*.py), full-width SD1.x UNet, synthetic prepared batch.

    python tools/bench_train.py [--views 8] [--depth-samples 3] [--steps 3] [--width 320] [--scenes N]
--scenes N feeds N scenes (own cameras, latents and draws) to every step: model([batch_0 .. batch_N-1], cfg), one batched forward and
backward with a timestep per scene.  Prints one JSON line (not the headline metric: bench.py measures denoising steps/s).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--depth-samples", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--scenes", type=int, default=1, help="scenes per training step (ViewFusion.forward on a list of batches)")
    ap.add_argument("--frozen-unet", action="store_true", help="finetune_unet: false (only the cross-attention / view-aligned parameters train); "
                    "default = configs/mvd_train.yaml:15 finetune_unet: true (all 1 039 M parameters)")
    ap.add_argument("--tuned", default=None, help="tuner cache file (hip.save_tuned / load_tuned): loaded when present, written after the first step -- "
                    "a profiling pass of the same command then launches the same kernels without timing candidates")
    ap.add_argument("--cprofile", default=None, help="write a cProfile summary of the steady steps (host side) to this file")
    a = ap.parse_args()
    from mvdfusion_amd import hip
    if a.tuned and os.path.exists(a.tuned):
        hip.load_tuned(a.tuned)
    from mvdfusion_amd.configs import model_config
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.viewfusion_zero_depth_rgb import ViewFusion
    V, D, S = a.views, a.depth_samples, 32
    cfg = model_config(a.width, D=D, S=S)
    cfg["finetune_unet"] = not a.frozen_unet
    with syn.skip_default_init():
        m = ViewFusion(**cfg)
    syn.fill_module_(m)
    m = m.cuda().train()
    for n, p in m.named_parameters():
        if n.startswith(("vae.", "clip_image_encoder.")):
            p.requires_grad_(False)
    if a.scenes < 1:
        ap.error("--scenes must be >= 1")
    batches = []
    for n in range(a.scenes):
        inp = syn.make_inputs(V, S, seed=n)
        g = torch.Generator().manual_seed(5 + n)
        lat = torch.randn(V, 5, S, S, generator=g).cuda()
        batches.append({"_prepared": (lat, inp["batch_cameras"], inp["input_latents"].cuda(), inp["input_cameras"], inp["clip_v_embed"].cuda())})
    batch = batches[0] if a.scenes == 1 else batches
    opt = m.configure_optimizers(lr=1e-5)
    n_train = sum(p.numel() for p in m.parameters() if p.requires_grad)
    times, losses = [], []
    prof = None
    mark = torch.zeros(1, dtype=torch.int32, device="cuda")      # step delimiter in a kernel trace (tools/trace_summary.py: advance_iter_kernel)
    for i in range(a.steps + 1):
        hip.check(hip.lib().mvd_advance_iter(hip.ptr(mark), hip.stream()))
        torch.cuda.synchronize()
        if a.cprofile and i == 1:
            import cProfile
            prof = cProfile.Profile()
            prof.enable()
        t0 = time.perf_counter()
        loss = m(batch, {})
        opt.zero_grad()
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        losses.append(float(loss.detach()))
        if i == 0 and a.tuned:
            hip.save_tuned(a.tuned)
    hip.check(hip.lib().mvd_advance_iter(hip.ptr(mark), hip.stream()))
    torch.cuda.synchronize()
    if prof is not None:
        import io
        import pstats
        prof.disable()
        buf = io.StringIO()
        st = pstats.Stats(prof, stream=buf)
        st.sort_stats("cumulative").print_stats(60)
        st.sort_stats("tottime").print_stats(45)
        open(a.cprofile, "w").write(f"# {a.steps} steady steps of tools/bench_train.py --views {a.views} --depth-samples {a.depth_samples}\n" + buf.getvalue())
    import statistics
    dt = statistics.median(times[1:])          # (median: a step that meets a new shape tunes it, a host hiccup is 50 ms)
    # algorithmic work of one step (SURVEY.md section 8(d), 2 FLOP per MAC): forward = V UNet passes (cfg 1: no null twin) + GridAttn; the
    # backward is a dgrad and a wgrad per contraction (2 x forward) and re-runs every block's forward once (activation checkpointing at block
    # granularity, like the reference's use_checkpoint=True) => 4 x forward
    f_unet = {1: 225.09e9, 3: 235.81e9}.get(D, 225.09e9) * (a.width / 320.0) ** 2
    T = V * V * S * S * D
    f_fwd = V * f_unet + T * (3516416 + 3072 * V) + V * S * S * D * 393216 + (V + 1) * S * S * 2560
    flops = 4.0 * f_fwd
    flops *= a.scenes
    print(json.dumps({"metric": "training-steps/sec (fwd + bwd + AdamW, " + ("one scene)" if a.scenes == 1 else f"{a.scenes} scenes per step)"),
                      "value": 1.0 / dt, "unit": "steps/s", "s_per_step": dt, "scenes": a.scenes, "scene_steps_per_s": a.scenes / dt,
                      "step_s": [round(t, 4) for t in times[1:]], "first_step_s": times[0],
                      "roofline": {"bound": "mfma", "achieved": flops / dt / 1e12, "peak": 2500.0, "unit": "TFLOP/s", "frac": flops / dt / 2.5e15,
                                   "traffic": None, "algorithmic_tflop_per_step": flops / 1e12,
                                   "note": "whole step (fwd + recompute + dgrad + wgrad) against the dense 16-bit MFMA peak; the step is "
                                           "host- and glue-bound (DESIGN.md section 6c), not a kernel roofline"},
                      "views": V, "depth_samples": D, "latent": S, "model_channels": a.width, "trainable_parameters": n_train,
                      "finetune_unet": not a.frozen_unet,
                      "losses": losses, "peak_mem_GB": torch.cuda.max_memory_allocated() / 2 ** 30,
                      "note": "backward = recompute-per-block + dgrad/wgrad on the split-operand MFMA GEMM (big shapes autotuned on first sight), "
                              "fp32-MFMA self-attention backward; one batched max|w| read per step; no graph capture, fresh allocations; s_per_step = median of the timed steps"}))


if __name__ == "__main__":
    main()
