"""Write tests/golden/sample_overwrite_mc32_v3.npz by running the REAL reference's DDIMSampler(overwrite_x_noisy=True).sample loop
(mvdfusion/sampler.py:109-110,123-124: row 0 becomes the clean input latents before every iteration) -- container-only, like
oracle/make_golden.py, whose helpers and shims this uses; it calls the reference and copies nothing from it.

The loop that runs is the reference's own `sample` (the overwrite lives there, not in denoise_apply): a recorder around denoise_apply keeps
what each iteration returns and ends the loop after the first STEPS iterations with a private exception.  torch's global generator supplies
the reference's draws; they are replayed in the same order for oracle.ref_torch.denoise_step, with the row-0 overwrite restated here, and
the two trajectories are required to agree before anything is written.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_pinned.py
"""
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as G  # noqa: E402  (installs the shims)

O, syn = G.O, G.syn
NAME, MC, V, D, S, STEPS, CFG, SEED, INPUT_SEED = "sample_overwrite_mc32_v3", 32, 3, 1, 32, 3, 2.5, 778, 9
TOL = 5e-5                      # oracle vs reference, as make_golden's sibling fixture sample_prevdepth_mc32_v2


class _Stop(Exception):
    """Ends the reference's sampling loop after STEPS iterations."""


def facade():
    """The ViewFusion members the sampler and apply_model touch (as gold_sample_feed_prev_depth builds them)."""
    from mvdfusion.scheduler import DDPMScheduler
    from mvdfusion.unet import UNetWrapper
    from mvdfusion.view_attn_efficient2 import GridAttn
    from mvdfusion.viewfusion_zero_depth_rgb import ViewFusion

    class Facade(nn.Module):
        embed_time = ViewFusion.embed_time
        apply_model = ViewFusion.apply_model

        def __init__(self):
            super().__init__()
            self.view_attn = GridAttn(in_channels=5, input_size=S, output_dim=768, num_layers=3, z_near_far_scale=0.8, n_pts_per_ray=D)
            w = UNetWrapper.__new__(UNetWrapper)
            nn.Module.__init__(w)
            w.unet_model = G._unet(MC, S)
            w.drop_conditions, w.use_zero_123 = False, True
            self.unet_model = w
            self.scheduler = DDPMScheduler(1000)
            self.cc_projection = nn.Sequential(nn.Linear(796, 768), nn.SiLU(True), nn.Linear(768, 768), nn.SiLU(True), nn.Linear(768, 768))
            self.time_embed_dim = 256
            self.time_embed = nn.Sequential(nn.Linear(256, 256), nn.SiLU(True), nn.Linear(256, 256))
            self.register_buffer("_device", torch.tensor([0.0]), persistent=False)

    m = Facade()
    for name in ("view_attn", "cc_projection", "time_embed"):
        G.fill_ref(getattr(m, name), name + ".")
    return m.eval()


def oracle_trajectory(sd, inp, x_T, dns, sns):
    """STEPS iterations of oracle.ref_torch.denoise_step with row 0 overwritten by the clean input latents before each of them."""
    tab = O.ddpm_tables()
    dd = O.ddim_schedule(tab)
    x, xs, x0s = x_T.clone(), [], []
    for i in range(len(dns)):
        x = x.clone()              # (the previous iteration's result is kept: overwrite a copy)
        x[0] = inp["input_latents"][0]
        with torch.no_grad():
            x, x0 = O.denoise_step(sd, x, G.cam_dict(inp["batch_cameras"]), inp["input_latents"], G.cam_dict(inp["input_cameras"]),
                                   inp["clip_v_embed"], tab, dd, 49 - i, dns[i], sns[i], cfg_scale=CFG, n_pts_per_ray=D,
                                   unet_kw=dict(model_channels=MC, image_size=S))
        xs.append(x)
        x0s.append(x0)
    return torch.stack(xs), torch.stack(x0s)


def main():
    from mvdfusion.sampler import DDIMSampler
    m = facade()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    sampler = DDIMSampler(m, ddim_num_steps=50, ddim_discretize="uniform", ddim_eta=1.0, latent_size=S, z_dim=4, overwrite_x_noisy=True)
    inp = syn.make_inputs(V, S, seed=INPUT_SEED)
    bc, ic = G.ref_cams(inp["batch_cameras"]), G.ref_cams(inp["input_cameras"])
    seen, xs, x0s = [], [], []
    real = sampler.denoise_apply

    def recorder(x, *a, **kw):
        if len(xs) == STEPS:
            raise _Stop
        seen.append(x.clone())
        x_prev, x0 = real(x, *a, **kw)
        xs.append(x_prev.clone())
        x0s.append(x0.clone())
        return x_prev, x0

    sampler.denoise_apply = recorder
    torch.manual_seed(SEED)
    try:
        sampler.sample(bc, inp["input_latents"], ic, inp["clip_v_embed"], unconditional_scale=CFG, depth=True, verbose=False)
    except _Stop:
        pass
    assert len(xs) == STEPS and all(torch.equal(x[0], inp["input_latents"][0]) for x in seen)      # the overwrite really ran
    xs, x0s = torch.stack(xs), torch.stack(x0s)
    # the reference's draws, in its order: x_T, then per iteration the depth noise (inside GridAttn) and the update noise
    torch.manual_seed(SEED)
    x_T = torch.randn(V, 5, S, S)
    dns, sns = [], []
    for _ in range(STEPS):
        dns.append(torch.randn(V, D, S, S))
        sns.append(torch.randn(V, 5, S, S))
    oxs, ox0s = oracle_trajectory(sd, inp, x_T, dns, sns)
    for i in range(STEPS):
        e = max(G.rel_err(oxs[i], xs[i]), G.rel_err(ox0s[i], x0s[i]))
        print(f"  overwrite_x_noisy step {i}: oracle vs reference {e:.2e}")
        assert e < TOL, e
    G.save(NAME, x_T=x_T, depth_noise=torch.stack(dns), step_noise=torch.stack(sns), xs=xs, x0s=x0s)


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    main()
