"""CPU-only tests (`-m "not gpu"`): the oracle against the reference-generated golden vectors and analytic
known answers, the host logic of the product package, and the C-ABI export check (no compute without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT, load_golden, load_spec, model_config, rel_err

from oracle import ref_torch as O
from mvdfusion_amd import synthetic as syn
from mvdfusion_amd import cameras as cam


def cams(c):
    return {"R": c.R, "T": c.T, "f": c.focal_length, "p": c.principal_point}


# ------------------------------------------------------------------------------------------------ oracle vs golden
def test_oracle_schedule_bit_exact():
    gd = load_golden("schedule")
    tab = O.ddpm_tables()
    dd = O.ddim_schedule(tab)
    assert torch.equal(tab["alphas_cumprod"], gd["alphas_cumprod"])
    assert torch.equal(dd["timesteps"], gd["ddim_timesteps"])
    for k in ("alphas", "alphas_prev", "sigmas", "sqrt_one_minus_alphas"):
        assert torch.equal(dd[k], gd["ddim_" + k]), k
    for index in (49, 25, 1, 0):
        xp, x0 = O.ddim_update(gd["x"], gd["eps"], dd, index, gd["noise"] if index > 0 else None)
        assert torch.equal(xp, gd[f"x_prev_{index}"]) and torch.equal(x0, gd[f"x0_{index}"])


@pytest.mark.parametrize("name,V,D,seed,tval", [("gridattn_v4_d1", 4, 1, 0, 981), ("gridattn_v3_d3", 3, 3, 1, 501),
                                                ("gridattn_v15_d1", 15, 1, 3, 741), ("gridattn_v7_d1", 7, 1, 8, 621),
                                                ("gridattn_v5_d3", 5, 3, 9, 161)])
def test_oracle_gridattn_vs_reference(name, V, D, seed, tval):
    gd = load_golden(name)
    sd = {k: v for k, v in syn.det_fill_state_dict(load_spec(32)).items() if k.startswith("view_attn.")}
    inp = syn.make_inputs(V, 32, seed)
    with torch.no_grad():
        out = O.gridattn_forward(sd, "view_attn.", gd["x"], cams(inp["batch_cameras"]), gd["t_embed"],
                                 torch.full((V,), tval, dtype=torch.long), O.ddpm_tables(), gd["depth_noise"],
                                 inp["input_latents"], cams(inp["input_cameras"]), n_pts_per_ray=D)
    assert rel_err(out[:, ::5, ::7, :, ::3], gd["out_strided"]) < 3e-5
    assert abs(float(out.norm()) - float(gd["out_l2"])) / float(gd["out_l2"]) < 1e-5


def test_oracle_gridattn_overwrite_attn_depth_vs_reference():
    """overwrite_attn_depth (view_attn_efficient2.py:418-426; the feed_prev_depth path) of the oracle against the reference's output."""
    gd = load_golden("gridattn_v4_d1_prevdepth")
    V, tval = 4, 301
    sd = {k: v for k, v in syn.det_fill_state_dict(load_spec(32)).items() if k.startswith("view_attn.")}
    inp = syn.make_inputs(V, 32, int(gd["seed"]))
    kw = dict(n_pts_per_ray=1)
    args = (sd, "view_attn.", gd["x"], cams(inp["batch_cameras"]), gd["t_embed"], torch.full((V,), tval, dtype=torch.long), O.ddpm_tables(),
            gd["depth_noise"], inp["input_latents"], cams(inp["input_cameras"]))
    with torch.no_grad():
        out = O.gridattn_forward(*args, overwrite_attn_depth=gd["prev_depth"], **kw)
        plain = O.gridattn_forward(*args, **kw)
    assert rel_err(out[:, ::5, ::7, :, ::3], gd["out_strided"]) < 3e-5
    assert rel_err(plain[:, ::5, ::7, :, ::3], gd["out_strided"]) > 1e-2


@pytest.mark.parametrize("name,mc,V,D,tval", [("unet_mc32_v4_d1", 32, 4, 1, 981), ("unet_mc32_v2_d3", 32, 2, 3, 501),
                                              ("unet_mc64_v2_d1", 64, 2, 1, 21), ("unet_mc320_v2_d3", 320, 2, 3, 501)])
def test_oracle_unet_vs_reference(name, mc, V, D, tval):
    import json
    gd = load_golden(name)
    spec = [(f"unet_model.unet_model.{k}", tuple(s)) for k, s in json.loads(str(gd["spec"]))]
    sd = syn.det_fill_state_dict(spec)
    g = torch.Generator().manual_seed(200 + int(gd["vol_seed"]))
    x = torch.randn(V, 10, 32, 32, generator=g)
    ctx = torch.randn(V, 1, 768, generator=g)
    vol = torch.randn(V, 32, 32, D, 768, generator=g) * 0.5
    with torch.no_grad():
        out = O.unet_forward(sd, "unet_model.unet_model.", x, torch.tensor([tval]), ctx, O.volume_pyramid(vol),
                             model_channels=mc)
    assert rel_err(out, gd["out"]) < 1e-5


def test_oracle_step_vs_reference():
    gd = load_golden("step_mc32_v4_d1")
    sd = syn.det_fill_state_dict(load_spec(32))
    inp = syn.make_inputs(4, 32, seed=7)
    tab = O.ddpm_tables()
    dd = O.ddim_schedule(tab)
    for index in (49, 0):
        with torch.no_grad():
            xp, x0 = O.denoise_step(sd, gd["x"], cams(inp["batch_cameras"]), inp["input_latents"],
                                    cams(inp["input_cameras"]), inp["clip_v_embed"], tab, dd, index,
                                    gd[f"depth_noise_{index}"], gd[f"step_noise_{index}"], cfg_scale=2.5,
                                    unet_kw=dict(model_channels=32))
        assert rel_err(xp, gd[f"x_prev_{index}"]) < 2e-5 and rel_err(x0, gd[f"x0_{index}"]) < 2e-5


# ------------------------------------------------------------------------------------------------ known answers
def test_kat_camera_rig_and_rebasing():
    gd = load_golden("cameras")
    rig = syn.gso_rig()
    assert rel_err(rig.R, gd["R"]) < 1e-6 and rel_err(rig.T, gd["T"]) < 1e-6
    rel = cam.get_relative_camera(rig, [0])
    assert rel_err(rel.R, gd["rel_R"]) < 1e-6 and rel_err(rel.T, gd["rel_T"]) < 1e-6
    # the input camera becomes R = I, T = (0, 0, 1.5)
    assert torch.allclose(rel.R[0], torch.eye(3), atol=1e-6)
    assert torch.allclose(rel.T[0], torch.tensor([0.0, 0.0, 1.5]), atol=1e-6)
    assert rel_err(rel.get_camera_center(), gd["centers"]) < 1e-6
    assert rel_err(cam.pack_cameras(rel)[:, 16:19], gd["centers"]) < 1e-6


def test_kat_project_unproject_roundtrip():
    gd = load_golden("cameras")
    R, T = gd["rel_R"], gd["rel_T"]
    f, p = torch.full((16, 2), 2.1875), torch.zeros(16, 2)
    assert rel_err(O.project_ndc(R, T, f, p, gd["pts"]), gd["ndc"]) < 1e-5
    xy_d = gd["xy_d"]
    w = O.unproject_ndc(R, T, f, p, xy_d[..., :2], xy_d[..., 2])
    assert rel_err(w, gd["unproj"]) < 1e-5
    for i in range(16):   # project(unproject(xy, d)) == (xy, 1/d)
        back = O.project_ndc(R[i:i + 1], T[i:i + 1], f[i:i + 1], p[i:i + 1], w[i])[0]
        assert torch.allclose(back[:, :2], xy_d[i, :, :2], atol=2e-5)
        assert torch.allclose(back[:, 2], 1.0 / xy_d[i, :, 2], atol=2e-5)


def test_kat_hand_computed_camera_conventions():
    """Independent of oracle/shims.py: numbers worked out BY HAND from PyTorch3D's published conventions (row vectors,
    X_view = X_world R + T; NDC projection u = f x/z + p with 1/z as the third component; C = -T R^T;
    look_at_view_transform axes as columns).  Checks the oracle, the product's host camera algebra and the device record."""
    # (1) R = I, T = (0,0,2), f = 2, p = 0:  X = (0.5,-0.25,1) -> X_view = (0.5,-0.25,3) -> ndc = (1/3, -1/6, 1/3)
    R, T = torch.eye(3)[None], torch.tensor([[0.0, 0.0, 2.0]])
    f, p0 = torch.tensor([[2.0, 2.0]]), torch.zeros(1, 2)
    ndc = O.project_ndc(R, T, f, p0, torch.tensor([[0.5, -0.25, 1.0]]))[0, 0]
    assert torch.allclose(ndc, torch.tensor([1.0 / 3.0, -1.0 / 6.0, 1.0 / 3.0]), atol=1e-6)
    w = O.unproject_ndc(R, T, f, p0, torch.tensor([[[1.0 / 3.0, -1.0 / 6.0]]]), torch.tensor([[3.0]]))[0, 0]
    assert torch.allclose(w, torch.tensor([0.5, -0.25, 1.0]), atol=1e-6)
    # principal point shifts NDC additively: p = (0.1, -0.2)
    ndc = O.project_ndc(R, T, f, torch.tensor([[0.1, -0.2]]), torch.tensor([[0.5, -0.25, 1.0]]))[0, 0]
    assert torch.allclose(ndc[:2], torch.tensor([1.0 / 3.0 + 0.1, -1.0 / 6.0 - 0.2]), atol=1e-6)
    # (2) quarter turn about y, row-vector convention: rows of R are the images of the world axes.
    #     X = (1,0,0) -> X R = row 0 = (0,0,-1);  T = (0,0,2)  =>  X_view = (0,0,1);  C = -T R^T = (2,0,0)
    R2 = torch.tensor([[[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]])
    C = O.camera_center(R2, T)[0]
    assert torch.allclose(C, torch.tensor([2.0, 0.0, 0.0]), atol=1e-6)
    assert torch.allclose(cam.Cameras(R2, T, f, p0).get_camera_center()[0], C, atol=1e-6)
    assert torch.allclose(cam.pack_cameras(cam.Cameras(R2, T, f, p0))[0, 16:19], C, atol=1e-6)
    # a point one unit in front of that camera along its optical axis: world (1,0,0) -> view (0,0,1) -> ndc (0,0,1)
    ndc = O.project_ndc(R2, T, f, p0, torch.tensor([[1.0, 0.0, 0.0]]))[0, 0]
    assert torch.allclose(ndc, torch.tensor([0.0, 0.0, 1.0]), atol=1e-6)
    # world (1, 0.5, 0.25): view = 1*(0,0,-1) + 0.5*(0,1,0) + 0.25*(1,0,0) + (0,0,2) = (0.25, 0.5, 1) -> ndc (0.5, 1.0, 1)
    ndc = O.project_ndc(R2, T, f, p0, torch.tensor([[1.0, 0.5, 0.25]]))[0, 0]
    assert torch.allclose(ndc, torch.tensor([0.5, 1.0, 1.0]), atol=1e-6)
    # (3) look_at_view_transform(dist 1.5, elev 0, azim 0, up y): C = (0,0,1.5), z = (0,0,-1), x = up x z = (-1,0,0),
    #     y = z x x = (0,1,0)  =>  R = diag(-1, 1, -1) (axes as columns), T = -R^T C = (0,0,1.5)
    Rl, Tl = cam.look_at_view_transform(1.5, 0.0, 0.0)
    assert torch.allclose(Rl[0], torch.diag(torch.tensor([-1.0, 1.0, -1.0])), atol=1e-6)
    assert torch.allclose(Tl[0], torch.tensor([0.0, 0.0, 1.5]), atol=1e-6)
    # azim 90 deg: C = (1.5,0,0), z = (-1,0,0), x = (0,1,0) x (-1,0,0) = (0,0,1), y = z x x = (0,1,0)
    Rl, Tl = cam.look_at_view_transform(1.5, 0.0, 90.0)
    assert torch.allclose(Rl[0], torch.tensor([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]), atol=1e-6)
    assert torch.allclose(Tl[0], torch.tensor([0.0, 0.0, 1.5]), atol=1e-6)
    # (4) re-basing with center_at_origin=False: R'_i = R_q^T R_i, T'_i = T_i  (hand: R_q = R2 => R'_q = I)
    rel = cam.get_relative_camera(cam.Cameras(torch.cat([R2, torch.eye(3)[None]]), torch.cat([T, T]), f.expand(2, 2), p0.expand(2, 2)), [0])
    assert torch.allclose(rel.R[0], torch.eye(3), atol=1e-6) and torch.allclose(rel.T, torch.cat([T, T]), atol=1e-6)
    assert torch.allclose(rel.R[1], R2[0].t(), atol=1e-6)


def test_kat_timm_head_layout_and_harmonic_order():
    """timm Attention splits qkv(x) as reshape(B, N, 3, heads, hd): channel c of the 3C output is (which = c // C,
    head = (c % C) // hd, d = c % hd); hand-built 2-token example through the oracle's DiT block attention core."""
    import torch.nn.functional as F
    Cc, H = 8, 2
    x = torch.tensor([[[1.0] * Cc, [2.0] * Cc]])                           # (1, 2 tokens, 8)
    Wqkv = torch.zeros(3 * Cc, Cc)
    Wqkv[2 * Cc + 0, 0] = 1.0                                              # v of head 0, d 0 reads channel 0
    Wqkv[2 * Cc + 4, 1] = 3.0                                              # v of head 1, d 0 reads channel 1 (x3)
    qkv = F.linear(x, Wqkv).reshape(1, 2, 3, H, Cc // H).permute(2, 0, 3, 1, 4)
    q, k, v = qkv.unbind(0)
    out = ((q * (Cc // H) ** -0.5) @ k.transpose(-2, -1)).softmax(-1) @ v   # q = k = 0: uniform attention
    out = out.transpose(1, 2).reshape(1, 2, Cc)
    assert torch.allclose(out[0, :, 0], torch.tensor([1.5, 1.5])) and torch.allclose(out[0, :, 4], torch.tensor([4.5, 4.5]))
    # harmonic embedding order: [sin(dim-major, k-minor) | cos | x], omega_k = 0.1 * 2^k
    e = O.harmonic_embedding(torch.tensor([[1.0, 10.0]]))
    assert e.shape == (1, 30)
    assert float(e[0, 0]) == pytest.approx(float(torch.sin(torch.tensor(0.1)))) and \
        float(e[0, 7]) == pytest.approx(float(torch.sin(torch.tensor(1.0)))) and \
        float(e[0, 14 + 6]) == pytest.approx(float(torch.cos(torch.tensor(6.4)))) and float(e[0, 29]) == 10.0


def test_kat_own_view_gather_coordinates():
    """Ray grid is half-pixel inset but grid_sample uses align_corners=True: own-view samples land at
    0.484375 + 0.96875*i pixels (SURVEY trap T4)."""
    S = 32
    lin = torch.linspace(1 - 1 / S, -1 + 1 / S, S)
    ix = ((-lin + 1) / 2) * (S - 1)
    assert torch.allclose(ix, 0.484375 + 0.96875 * torch.arange(S, dtype=torch.float32), atol=1e-5)


def test_kat_harmonic_and_timestep_embedding():
    e = O.harmonic_embedding(torch.tensor([[2.0]]))
    w = 0.1 * 2.0 ** torch.arange(7)
    assert e.shape == (1, 15)
    assert torch.allclose(e[0, :7], torch.sin(2.0 * w)) and torch.allclose(e[0, 7:14], torch.cos(2.0 * w))
    assert float(e[0, 14]) == 2.0
    e6 = O.harmonic_embedding(torch.arange(6, dtype=torch.float32)[None])
    assert e6.shape == (1, 90) and float(e6[0, 1 * 7 + 2]) == pytest.approx(float(torch.sin(torch.tensor(1.0 * 0.4))))
    t = O.timestep_embedding(torch.tensor([981.0]), 320)
    assert float(t[0, 0]) == pytest.approx(float(torch.cos(torch.tensor(981.0)))) and float(t[0, 160]) == pytest.approx(
        float(torch.sin(torch.tensor(981.0))))


def test_kat_ddim_tables():
    tab = O.ddpm_tables()
    dd = O.ddim_schedule(tab)
    assert int(dd["timesteps"][0]) == 1 and int(dd["timesteps"][-1]) == 981
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    assert torch.equal(tab["alphas_cumprod"], torch.cumprod(1 - betas, 0))
    assert float(dd["alphas_prev"][0]) == float(tab["alphas_cumprod"][0])


def test_kat_kvlen1_attention_is_linear():
    """softmax over one key == 1  =>  CrossAttention(x, ctx of length 1) == to_out(to_v(ctx))."""
    g = torch.Generator().manual_seed(0)
    C, H = 64, 8
    sd = {"a.to_q.weight": torch.randn(C, C, generator=g), "a.to_k.weight": torch.randn(C, 768, generator=g),
          "a.to_v.weight": torch.randn(C, 768, generator=g), "a.to_out.0.weight": torch.randn(C, C, generator=g),
          "a.to_out.0.bias": torch.randn(C, generator=g)}
    x, ctx = torch.randn(2, 10, C, generator=g), torch.randn(2, 1, 768, generator=g)
    full = O._cross_attention(sd, "a.", x, ctx, H)
    short = torch.nn.functional.linear(torch.nn.functional.linear(ctx, sd["a.to_v.weight"]), sd["a.to_out.0.weight"],
                                       sd["a.to_out.0.bias"]).expand(-1, 10, -1)
    assert torch.allclose(full, short, atol=1e-4)


def test_kat_normal_equals_mean_plus_std_randn():
    """torch.normal(mean, std) consumes the CPU stream exactly like mean + std*randn (SURVEY trap T2)."""
    mean, std = torch.randn(4, 3, 8, 8), torch.rand(4, 3, 8, 8) + 0.1
    torch.manual_seed(5)
    a = torch.normal(mean, std=std)
    torch.manual_seed(5)
    b = mean + std * torch.randn(4, 3, 8, 8)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ host logic of the product
def test_state_dict_keys_match_reference():
    from mvdfusion_amd.viewfusion_zero_depth_rgb import ViewFusion
    m = ViewFusion(**model_config(32))
    want = dict(load_spec(32))
    have = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("scheduler.")}
    assert have == want
    sched = {k for k in m.state_dict() if k.startswith("scheduler.")}
    assert sched == {"scheduler." + k for k in ("betas", "alphas", "alphas_cumprod", "sqrt_alphas_cumprod",
                                                "sqrt_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod",
                                                "sqrt_recipm1_alphas_cumprod", "posterior_variance",
                                                "posterior_log_variance_clipped")}


def test_product_scheduler_and_sampler_tables():
    from mvdfusion_amd.scheduler import DDPMScheduler
    from mvdfusion_amd.sampler import DDIMSampler
    from mvdfusion_amd.engine import ddim_step_table
    gd = load_golden("schedule")

    class M:
        scheduler = DDPMScheduler(1000)
    s = DDIMSampler(M(), ddim_num_steps=50, ddim_eta=1.0, latent_size=32)
    assert torch.equal(M.scheduler.alphas_cumprod, gd["alphas_cumprod"])
    assert np.array_equal(s.ddim_timesteps, gd["ddim_timesteps"].numpy())
    assert torch.equal(s.ddim_alphas, gd["ddim_alphas"]) and torch.equal(s.ddim_sigmas, gd["ddim_sigmas"])
    assert torch.equal(s.ddim_alphas_prev, gd["ddim_alphas_prev"])
    st, dd = s.tables()
    tab = ddim_step_table(st, dd, [49, 0])
    assert tab.shape == (2, 8) and float(tab[0, 0]) == 981.0 and float(tab[1, 0]) == 1.0
    assert float(tab[0, 7]) == 1.0 and float(tab[1, 7]) == 0.0
    x, eps = gd["x"], gd["eps"]
    torch.manual_seed(77)
    xp, x0 = s.denoise_apply_impl(x, 25, eps)
    assert torch.equal(xp, gd["x_prev_25"]) and torch.equal(x0, gd["x0_25"])


def test_factory_resolves_reference_targets():
    from mvdfusion_amd.load_model import instantiate_from_config, get_obj_from_str
    from mvdfusion_amd.scheduler import DDPMScheduler
    from mvdfusion_amd.unet import UNetModel
    assert get_obj_from_str("mvdfusion.unet.UNetModel") is UNetModel
    s = instantiate_from_config({"target": "mvdfusion.scheduler.DDPMScheduler", "params": {"timesteps": 1000}})
    assert isinstance(s, DDPMScheduler)


def test_zero_edit_drop_in_aliases_and_reference_yaml_configs(tmp_path):
    """north_star: "demo.py and train.py drop in unchanged".  mvdfusion_amd.install_aliases() registers the mirrors under the reference's
    dotted module names, so `from utils.load_model import instantiate_from_config` (demo.py:21, train.py:24) and the yaml `target:`
    strings (utils/load_model.py:10-25) resolve to this package.  In a clean interpreter, with no reference on the path: (1) the aliases
    alone; (2) the yaml-shaped model block of the two shipped configuration families -- sampling (n_pts_per_ray 1, frozen UNet, 15 views,
    configs/mvd_gso.yaml) and training (n_pts_per_ray 3, finetuned UNet, 7 views, configs/mvd_train.yaml), built by
    mvdfusion_amd.configs.model_config with the VAE block of the yaml: EVERY `target:` resolves, and `instantiate_from_config(model)` builds
    the full ViewFusion (weight paths cleared: no checkpoints offline; parameter initialisers skipped for speed) with that n_pts_per_ray /
    finetune_unet."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = r"""
import os, sys, json
sys.path.insert(0, %r)
import torch
torch.nn.Linear.reset_parameters = lambda self: None
torch.nn.modules.conv._ConvNd.reset_parameters = lambda self: None
import mvdfusion_amd
names = mvdfusion_amd.install_aliases()
import importlib
from utils.load_model import instantiate_from_config, get_obj_from_str
assert instantiate_from_config.__module__ == "mvdfusion_amd.load_model"
for ref, mine in mvdfusion_amd.configs.ALIASES.items():
    assert importlib.import_module(ref).__name__ == mine, ref
from mvdfusion.viewfusion_zero_depth_rgb import ViewFusion
from external.sd1.ldm.models.autoencoder import AutoencoderKL
from external.sd1.ldm.modules.encoders.modules import FrozenCLIPImageEmbedder
assert ViewFusion.__module__.startswith("mvdfusion_amd.") and AutoencoderKL.__module__.startswith("mvdfusion_amd.")
out = {"aliases": len(names), "configs": {}}
from mvdfusion_amd.configs import model_config
vae = {"target": "external.sd1.ldm.models.autoencoder.AutoencoderKL",
       "params": {"embed_dim": 4, "monitor": "val/rec_loss", "lossconfig": {"target": "torch.nn.Identity"},
                  "ddconfig": {"double_z": True, "z_channels": 4, "resolution": 256, "in_channels": 3, "out_ch": 3, "ch": 128,
                               "ch_mult": [1, 2, 4, 4], "num_res_blocks": 2, "attn_resolutions": [], "dropout": 0.0}}}
for name, D, finetune, V in (("sampling", 1, False, 15), ("training", 3, True, 7)):
    params = model_config(320, D=D, finetune_unet=finetune, vae_config=vae, clip_path=None, unet_cc_path=None)
    del params["precision"]                                   # (not a yaml key: the package default applies)
    mc = {"target": "mvdfusion.viewfusion_zero_depth_rgb.ViewFusion", "params": params}
    targets = []
    def walk(n):
        if isinstance(n, dict):
            if "target" in n: targets.append(n["target"].strip())
            for v in n.values(): walk(v)
    walk(mc)
    for t in targets:
        cls = get_obj_from_str(t)
        assert t.startswith("torch.") or cls.__module__.startswith("mvdfusion_amd."), (t, cls)
    m = instantiate_from_config(mc)
    assert type(m).__module__ == "mvdfusion_amd.viewfusion_zero_depth_rgb"
    assert m.view_attn.n_pts_per_ray == D
    assert m.finetune_unet == finetune
    assert all(p.requires_grad == m.finetune_unet for n, p in m.unet_model.named_parameters() if ".aligned_attn_" not in n)
    assert m.view_attn.fused_supported(V, V * V * 1024 * m.view_attn.n_pts_per_ray), (name, V)      # the shipped view counts take the fused kernel
    out["configs"][name] = dict(targets=len(targets), views=V, params=sum(p.numel() for p in m.parameters()))
print("ALIASJSON " + json.dumps(out))
""" % root
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    import json
    rec = json.loads(r.stdout[r.stdout.index("ALIASJSON ") + 10:].splitlines()[0])
    assert rec["aliases"] >= 9
    assert set(rec["configs"]) == {"sampling", "training"}, rec
    assert all(c["targets"] == 6 and c["params"] > 1.0e9 for c in rec["configs"].values()), rec


def test_precision_policy_parsing():
    from mvdfusion_amd import hip
    assert hip.parse_precision("f16x4") == ("f16", 4, {})
    assert hip.parse_precision("bf16x3") == ("bf16", 3, {})
    assert hip.parse_precision("f16") == ("f16", 1, {})
    assert hip.parse_precision("f16x4:conv=3,geglu=3") == ("f16", 4, {"conv": 3, "geglu": 3})
    with pytest.raises(ValueError):
        hip.parse_precision("f16x4:nonsense=3")
    with pytest.raises(ValueError):
        hip.parse_precision("f16x4:conv=2")
    for bad in ("fp16x3", "f16x2", "f32", "bf16x", "x3", "f16x3x3", ""):          # a mistyped BASE name must not become "f16, 1 product"
        with pytest.raises(ValueError):
            hip.parse_precision(bad)
    from mvdfusion_amd.viewfusion_zero_depth_rgb import ViewFusion
    m = ViewFusion(**model_config(32, precision="f16x4:conv=3"))
    assert m.precision == 4 and m.precision_policy == {"conv": 3}


def test_param_maxima_registry_replaces_per_pack_synchronisation():
    """hip.register_param_maxima / _pack_scale(like=): max|w| of every parameter from one batched reduction; a packed image of a
    parameter -- or of a transpose / flip / concatenation of parameters (`like=`) -- takes its power-of-two scale from the registry; tensors
    the registry does not know, parameters that died, and same-address tensors of another size fall back to reducing the tensor itself."""
    import gc
    import math
    from mvdfusion_amd import hip
    lin, conv = torch.nn.Linear(24, 40), torch.nn.Conv2d(8, 16, 3)
    with torch.no_grad():
        lin.weight.mul_(37.0)
        conv.weight.mul_(0.01)
    try:
        n = hip.register_param_maxima(list(lin.parameters()) + list(conv.parameters()))
        assert n == 4
        want = lambda t: 2.0 ** (10 - math.floor(math.log2(float(t.detach().abs().max()))))
        assert hip._known_max(lin.weight.detach()) == pytest.approx(float(lin.weight.detach().abs().max()))
        assert hip._pack_scale(lin.weight) == want(lin.weight) and hip._pack_scale(conv.weight) == want(conv.weight)
        wt = lin.weight.detach().t().contiguous()                      # a derived image: not registered itself ...
        assert hip._known_max(wt) is None and hip._pack_scale(wt) == want(lin.weight)      # ... (falls back to its own reduction)
        big = lin.weight.detach() * 100.0
        assert hip._pack_scale(big, like=lin.weight) == want(lin.weight)                   # `like` decides, not the tensor's own values
        assert hip._pack_scale(torch.cat([lin.weight.detach().reshape(-1), conv.weight.detach().reshape(-1)]),
                               like=[lin.weight, conv.weight]) == want(lin.weight)
        assert hip._pack_scale(big, like=[lin.weight, big]) == want(big)                   # one unknown source: reduce the tensor itself
        assert hip._known_max(lin.weight.detach()[:10]) is None                            # same address, other size
        before = hip._known_max(conv.weight.detach())                                      # an in-place update (an optimizer
        with torch.no_grad():                                                              # step) bumps the tensor version: the cached maximum
            conv.weight.mul_(64.0)                                                         # no longer answers, the tensor itself is reduced
        assert before is not None and hip._known_max(conv.weight.detach()) is None
        assert hip._pack_scale(conv.weight) == want(conv.weight)
        ptr = lin.weight.data_ptr()
        del lin
        gc.collect()
        assert hip._PARAM_MAX[ptr][0]() is None                                            # the parameter died: its entry no longer answers
        hip.forget_param_maxima()
        assert not hip._PARAM_MAX
    finally:
        hip.forget_param_maxima()


def test_fused_gridattn_serves_every_shipped_view_count():
    """configs/mvd_gso.yaml:97 (15 views), mvd_train.yaml:90,97 (5, 7): the fused kernel pads the views of a point to a power of two."""
    from mvdfusion_amd.view_attn_efficient2 import GridAttn
    ga = GridAttn(in_channels=5, input_size=32, n_pts_per_ray=1)
    for V in range(1, 17):
        assert ga.fused_supported(V, V * V * 1024), V
    assert not ga.fused_supported(17, 17 * 17 * 1024)
    assert ga.fused_supported(5, 5 * 1 * 1024 * 3)          # one query view of a 5-view job (a view-parallel rank), D = 3


def test_hot_kernels_compile_without_scratch_spills(tmp_path):
    """Every GEMM instantiation the tuner can select (gemm_kernel per block tile, gemm_ws_kernel, conv_patch_kernel: 156 kernels), the split-K
    reduce kernels, the attention kernel (up to 304 unified VGPRs per instantiation), the fused GridAttn kernel (357 - 361) and the
    reduce-and-normalise kernels hold their working sets in registers: a private (scratch) segment would mean spills in the k-loop.  hipcc
    cross-compiles the device code to assembly without a GPU (the GEMM family is one translation unit per kernel family since round 5,
    ~20 s each, compiled in parallel here); the kernel descriptors carry `.amdhsa_private_segment_fixed_size` and
    `.amdhsa_next_free_vgpr`."""
    import shutil
    import subprocess
    from concurrent.futures import ThreadPoolExecutor
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    plan = [("gemm_plain_t%d.hip" % t, 512, 0) for t in range(5)] + [
        ("gemm_ws.hip", 512, 0), ("gemm_patch.hip", 512, 0), ("gemm.hip", 128, 0),
        ("attention.hip", 512, 0), ("gridattn_fused.hip", 512, 0), ("elementwise.hip", 128, 0)]

    def compile_one(item):
        src = item[0]
        out = tmp_path / (src + ".s")
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                            os.path.join(ROOT, "mvdfusion_amd", "csrc", src), "-o", str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return out.read_text()

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        asms = list(ex.map(compile_one, plan))
    seen, gemm_seen, tiers = 0, 0, 0
    for (src, budget, scratch_max), asm in zip(plan, asms):
        for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
            name, body = m.group(1), m.group(2)
            scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
            vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
            assert scratch <= scratch_max, (src, name, scratch)
            assert vgpr <= budget, (src, name, vgpr)
            seen += 1
            gemm_seen += src.startswith(("gemm_plain", "gemm_ws", "gemm_patch"))
            # occupancy tiers the design depends on (csrc/gemm_plain.hpp, launch bounds): the plain loop of the dense 128x128 tile -- the
            # GEGLU / QKV projections -- runs TWO workgroups per CU = 4 wavefronts per SIMD (<= 128 registers; at 129 the step lost 2 %
            # in round 5 before anyone looked); the register-pipelined 64x80 loop three (<= 168)
            t = re.search(r"gemm_kernelILi(\d+)ELi(\d+)ELi\d+ELi\d+ELi(\d)ELi(\d)ELi(\d)E", name)
            if t:
                bm, bn, ns, amode, stages = (int(x) for x in t.groups())
                if (bm, bn, amode, stages) == (128, 128, 0, 2):
                    assert vgpr <= 128, (name, vgpr)
                    tiers += 1
                if (bm, bn, stages) == (64, 80, 3):
                    assert vgpr <= 168, (name, vgpr)
                    tiers += 1
    assert gemm_seen == 5 * 24 + 18 + 18, gemm_seen          # 5 tiles x 4 loops x 3 precisions x {dense, conv}; 3 tiles x 6; 3 tiles x 3 x 2 shares
    assert seen >= 200 and tiers == 3 + 6


def test_product_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mvdfusion_amd.viewfusion_zero_depth_rgb import ViewFusion
    m = ViewFusion(**model_config(32))
    inp = syn.make_inputs(2, 32, 0)
    with pytest.raises(RuntimeError):
        m.apply_model(inp["x_T"], inp["batch_cameras"], inp["input_latents"], inp["input_cameras"], inp["clip_v_embed"],
                      torch.full((2,), 981))


# ------------------------------------------------------------------------------------------------ VAE decode (section 8(f) rank 2)
@pytest.mark.parametrize("name,ch", [("vae_dec_ch32_z8", 32), ("vae_dec_ch128_z8", 128)])
def test_oracle_vae_decode_vs_reference(name, ch):
    """oracle.vae_decode / viewfusion_decode against the REAL AutoencoderKL.decode + ViewFusion.decode (bit-exact where
    generated; 3e-4 here because another host's conv kernels may flip one of the decoder tail's fp16 roundings)."""
    import json
    gd = load_golden(name)
    sd = syn.det_fill_state_dict(json.loads(str(gd["spec"])))
    with torch.no_grad():
        raw = O.vae_decode(sd, "vae.", gd["z"] * 1 / 0.18215, ch=ch)
        img = O.viewfusion_decode(sd, gd["z"], ch=ch)
    assert rel_err(raw, gd["raw"]) < 3e-4
    assert float((img - gd["image"]).abs().max()) < 1e-3
    assert float(img.min()) == 0.0 and float(img.max()) == 1.0          # the clip is exercised


@pytest.mark.parametrize("name,ch", [("vae_enc_ch32_r64", 32), ("vae_enc_ch128_r64", 128)])
def test_oracle_vae_encode_vs_reference(name, ch):
    import json
    gd = load_golden(name)
    sd = syn.det_fill_state_dict(json.loads(str(gd["spec"])))
    with torch.no_grad():
        z = O.viewfusion_encode(sd, gd["x"], ch=ch)
    assert rel_err(z, gd["z"]) < 2e-5


def test_vae_mirror_keys_and_guards():
    """The HIP VAE mirror exposes exactly the reference's keys, is what the yaml target resolves to, and has no CPU path."""
    import json
    from mvdfusion_amd.autoencoder import AutoencoderKL
    from mvdfusion_amd.load_model import get_obj_from_str
    assert get_obj_from_str("external.sd1.ldm.models.autoencoder.AutoencoderKL") is AutoencoderKL
    spec = json.loads(str(load_golden("vae_dec_ch128_z8")["spec"])) + json.loads(str(load_golden("vae_enc_ch128_r64")["spec"]))
    dd = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
              num_res_blocks=2, attn_resolutions=[], dropout=0.0)
    vae = AutoencoderKL(ddconfig=dd, lossconfig=dict(target="torch.nn.Identity"), embed_dim=4, monitor="val/rec_loss")
    mine = {k: tuple(v.shape) for k, v in vae.state_dict().items()}
    ref = {k[len("vae."):]: tuple(s) for k, s in spec}
    assert mine == ref and len(ref) == 248           # encoder.*, quant_conv.*, decoder.*, post_quant_conv.*
    with pytest.raises(RuntimeError):
        vae.decode(torch.zeros(1, 4, 8, 8))
    with pytest.raises(RuntimeError):
        vae.encode(torch.zeros(1, 3, 64, 64))


def test_fused_gridattn_weight_stream_layout():
    """pack_fused_stream: 215 slots of 32 KiB, and a fragment read the way csrc/gridattn_fused.hip does it (row lane & 15,
    16-byte chunk lane >> 4, swizzled) returns W[row, permuted k] for micro-tiles picked across the stream."""
    from mvdfusion_amd import hip
    from mvdfusion_amd import view_attn_efficient2 as va
    ga = va.GridAttn(in_channels=5, input_size=32, output_dim=768, num_layers=3, n_pts_per_ray=1)
    syn.fill_module_(ga, "view_attn.")
    stream, vecs = va.pack_fused_stream(ga)
    assert stream.shape == (215 * 16, 1024) and stream.dtype == torch.int16 and vecs.numel() == 11264

    def read(tile, row, g, scale):
        b = stream[tile].view(torch.float16)
        oh = ((row >> 3) * 1024 + (row & 7) * 128 + ((g ^ ((row >> 1) & 7)) * 16)) // 2
        ol = ((row >> 3) * 1024 + (row & 7) * 128 + (((4 + g) ^ ((row >> 1) & 7)) * 16)) // 2
        return (b[oh:oh + 8].float() + b[ol:ol + 8].float()) * scale

    kperm = lambda ks, g: [32 * ks + (4 * g + j if j < 4 else 16 + 4 * g + j - 4) for j in range(8)]
    misc = 3 * 3328
    # pre layer: slot ks, micro-tile nt
    Wpre = torch.zeros(256, 736)
    Wpre[:, :723] = ga.pre_layer_b[0].weight.detach()
    for ks, nt, row, g in [(0, 0, 0, 0), (22, 15, 9, 3), (7, 5, 14, 1)]:
        got = read(ks * 16 + nt, row, g, float(vecs[misc + 520]))
        assert torch.allclose(got, Wpre[16 * nt + row, kperm(ks, g)], rtol=1e-6, atol=1e-7)
    # block 1, head 3: qkv micro-tile mt = 6 ks + t6 -> rows {q, k, v} x {0, 1}; then proj k-step 3
    blk = ga.aggregation_transformer.layer_list[1]
    base = (23 + 64) * 16 + 3 * 64            # slots before block 1, then 3 heads x 4 slots x 16 micro-tiles
    for ks, t6, row, g in [(0, 0, 1, 0), (5, 3, 7, 2), (7, 5, 15, 3)]:
        wrow = [96, 112, 256 + 96, 256 + 112, 512 + 96, 512 + 112][t6] + row
        got = read(base + 6 * ks + t6, row, g, float(vecs[misc + 521 + 4]))
        assert torch.allclose(got, blk.attn.qkv.weight.detach()[wrow, kperm(ks, g)], rtol=1e-6, atol=1e-7)
    got = read(base + 48 + 11, 4, 2, float(vecs[misc + 522 + 4]))
    assert torch.allclose(got, blk.attn.proj.weight.detach()[16 * 11 + 4, kperm(3, 2)], rtol=1e-6, atol=1e-7)
    # block 1, MLP chunk 5: fc1 (32 micro-tiles: 4 ks + ... ) then fc2 k-steps 10, 11
    mb = (23 + 64) * 16 + 8 * 64 + 5 * 64
    got = read(mb + 4 * 6 + 2, 3, 1, float(vecs[misc + 523 + 4]))          # ks 6, chunk tile 2 -> hidden rows 64*5 + 32 ..
    assert torch.allclose(got, blk.mlp.fc1.weight.detach()[64 * 5 + 32 + 3, kperm(6, 1)], rtol=1e-6, atol=1e-7)
    got = read(mb + 32 + 16 + 9, 12, 0, float(vecs[misc + 524 + 4]))       # u = 1 -> k-step 11, output tile 9
    assert torch.allclose(got, blk.mlp.fc2.weight.detach()[16 * 9 + 12, kperm(11, 0)], rtol=1e-6, atol=1e-7)
    assert torch.equal(vecs[3328 + 1536:3328 + 2304], blk.attn.qkv.bias.detach())


def test_oracle_clip_vs_reference_golden_and_mirror_keys():
    """oracle clip_image_embed against the golden produced by the REAL FrozenCLIPImageEmbedder (encoders/modules.py:402-441; the
    un-vendored `clip` package is the structural restatement of oracle/shims.py), and the product mirror's parameter names =
    the reference's state_dict keys (clip_image_encoder.model.visual.* ...)."""
    import json
    from mvdfusion_amd.encoders import FrozenCLIPImageEmbedder
    gd = load_golden("clip_tiny")
    spec = json.loads(str(gd["spec"]))
    sd = syn.det_fill_state_dict([("clip_image_encoder." + k, tuple(s)) for k, s in spec])
    g = torch.Generator().manual_seed(int(gd["seed"]))
    x = torch.rand(2, 3, 256, 256, generator=g) * 2.0 - 1.0
    with torch.no_grad():
        out = O.clip_image_embed({k: v for k, v in sd.items() if ".visual." in k}, x, heads=2)
    assert rel_err(out, gd["out"]) < 1e-5
    mine = FrozenCLIPImageEmbedder(model="tiny-test")
    assert {k for k, _ in spec} == set(mine.state_dict().keys())
    assert {k: tuple(v.shape) for k, v in mine.state_dict().items()} == {k: tuple(s) for k, s in spec}
    ref_l14 = {k for k, _ in json.loads(str(load_golden("clip_vit_l14")["spec"]))}
    with torch.device("meta"):
        big = FrozenCLIPImageEmbedder(model="ViT-L/14")
    assert ref_l14 == set(big.state_dict().keys())
    with pytest.raises(RuntimeError):
        mine(x)                                   # CPU tensor: the product has no CPU path


def test_zero123_checkpoint_remap_matches_reference_loader(tmp_path):
    """load_unet_checkpoint (mirror of utils/load_model.py:26-110 + the param_mapper / remove_keys of mvdfusion/unet.py:70-93,
    viewfusion_zero_depth_rgb.py:69) on a synthetic zero123-shaped checkpoint: the same keys end up with the same values as
    with the REAL loader (golden ckpt_remap_mc32: per-key sums), the 8->10 channel stem / 4->5 channel head are dropped and the
    aligned_attn_* layers keep their initialisation."""
    import json
    from mvdfusion_amd.load_model import load_unet_checkpoint
    from mvdfusion_amd.unet import UNetModel
    from conftest import UNET_PARAMS
    gd = load_golden("ckpt_remap_mc32")
    p = dict(UNET_PARAMS)
    p["model_channels"] = 32
    torch.manual_seed(0)
    net = UNetModel(**p)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    path = str(tmp_path / "zero123.ckpt")
    torch.save(syn.synthetic_zero123_ckpt(net.state_dict()), path)
    res = load_unet_checkpoint(net, path, remove_keys=["input_blocks.0.0.weight", "out.2.weight", "out.2.bias"])
    after = net.state_dict()
    keys = json.loads(str(gd["keys"]))
    sums = gd["sums"].double() if torch.is_tensor(gd["sums"]) else torch.tensor(gd["sums"]).double()
    assert len(keys) == 683
    for k, ref in zip(keys, sums):
        assert abs(float(after[k].double().sum()) - float(ref)) < 1e-9 * max(1.0, abs(float(ref))), k
    untouched = [k for k in after if k not in keys]
    assert all("aligned_attn_" in k or k in ("input_blocks.0.0.weight", "out.2.weight", "out.2.bias") for k in untouched)
    assert all(torch.equal(after[k], before[k]) for k in untouched)
    assert not any("aligned_attn_" not in k and k not in ("input_blocks.0.0.weight", "out.2.weight", "out.2.bias")
                   for k in res.missing_keys)


def test_det_fill_is_stable_and_nonzero():
    a = syn.det_fill("unet_model.unet_model.out.2.weight", (5, 32, 3, 3))
    b = syn.det_fill("unet_model.unet_model.out.2.weight", (5, 32, 3, 3))
    assert torch.equal(a, b) and float(a.abs().min()) > 0
    assert abs(float(syn.det_fill("x.norm1.weight", (64,)).mean()) - 1.0) < 0.1


def test_view_range_partition():
    from mvdfusion_amd.parallel import view_range
    for V in (4, 8, 15):
        for world in (1, 2, 4, 8):
            rs = [view_range(V, r, world) for r in range(world)]
            assert sum(n for _, n in rs) == V
            assert all(rs[i][0] + rs[i][1] == rs[i + 1][0] for i in range(world - 1))


def test_gemm_configuration_table_and_tuner_cache(tmp_path):
    """hip.GEMM_CONFIGS mirrors the library's cfg encoding (include/mvd_hip.h): loop 3 (and 8, 9, 10 above the table) were removed in rounds
    5 / 6 and are not valid for any tile (the library rejects them: tests/test_gpu_ops.py), and a tuner cache written before the removal
    cannot smuggle a removed configuration back in."""
    import json
    from mvdfusion_amd import hip
    assert hip.REMOVED_LOOPS == (3,) and len(hip.GEMM_LOOPS) == 8
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    assert int(re.search(r"#define MVD_GEMM_LOOPS (\d+)", hdr).group(1)) == len(hip.GEMM_LOOPS)
    parts = [hip._cfg_parts(c) for c in hip.GEMM_CONFIGS_CONV]
    assert not [p for p in parts if p[1] in hip.REMOVED_LOOPS]
    assert {p[0] for p in parts if p[1] == hip.WS_LOOP} == {1, 2, 4} and {p[0] for p in parts if p[1] == hip.PATCH_LOOP} == {1, 2, 4}
    assert len(hip.GEMM_CONFIGS_CONV) == 2 * (5 * 4 + 3 + 3)                # two tile orders x (4 loops per tile + ws + patch)
    assert all(c in hip.gemm_configs(hip.EPI_STORE) for c in hip.gemm_configs(hip.EPI_GEGLU))
    assert {hip._cfg_parts(c)[0] for c in hip.gemm_configs(hip.EPI_GEGLU)} == {0, 1}      # the 80-column family serves EPI_STORE only
    assert hip.kernel_symbol(hip.make_cfg(2, hip.WS_LOOP), 3, True) == "gemm_ws_kernel<128, 80, 4, 1, 3, 1>"
    assert hip.kernel_symbol(hip.make_cfg(0, 5), 3, False) == "gemm_kernel<64, 64, 2, 2, 3, 0, 7>"
    path = tmp_path / "tuned.json"
    good, removed = hip.make_cfg(1, 4), hip.make_cfg(1, 10)
    doc = {"version": hip.TUNE_CACHE_VERSION, "cfg_stride": hip.CFG_STRIDE, "operand_format": hip.OPERAND_FORMAT,
           "entries": [[[1, 2, 3], [good, 1]], [[4, 5, 6], [removed, 1]], [[7, 8, 9], [0, 2]]]}
    saved = dict(hip._TUNED)
    try:
        hip._TUNED.clear()
        path.write_text(json.dumps(doc))
        assert hip.load_tuned(str(path)) == 2 and (4, 5, 6) not in hip._TUNED
        doc["version"] = hip.TUNE_CACHE_VERSION - 1                              # a cache of the previous encoding: rejected as a whole
        path.write_text(json.dumps(doc))
        hip._TUNED.clear()
        assert hip.load_tuned(str(path)) == 0 and not hip._TUNED
    finally:
        hip._TUNED.clear()
        hip._TUNED.update(saved)


def test_hip_adamw_is_a_torch_adamw_and_falls_back_off_gpu():
    """mvdfusion_amd.optim.HipAdamW: the class ViewFusion.configure_optimizers returns.  On CPU tensors (or any group its one-launch kernel does
    not cover) the step is torch's own, bit for bit, and the state dict is torch's."""
    from mvdfusion_amd.optim import HipAdamW
    g = torch.Generator().manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(7, 5, generator=g)), torch.nn.Parameter(torch.randn(11, generator=g))]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    a, b = HipAdamW(ps, lr=1e-2), torch.optim.AdamW(qs, lr=1e-2)
    assert isinstance(a, torch.optim.AdamW)
    for step in range(3):
        for p, q in zip(ps, qs):
            gr = torch.randn(p.shape, generator=g)
            p.grad, q.grad = gr.clone(), gr.clone()
        a.step()
        b.step()
    assert all(torch.equal(p, q) for p, q in zip(ps, qs))
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["param_groups"] == sb["param_groups"] and set(sa["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert all(torch.equal(sa["state"][k]["exp_avg_sq"], sb["state"][k]["exp_avg_sq"]) for k in sb["state"])


def test_weight_prefetch_schedule():
    """hip.WeightPrefetcher._build (host logic of mvd_gemm_desc.pf_items): which launch requests which weight."""
    import ctypes
    from mvdfusion_amd import hip
    MB = 1 << 20
    # launch order: (pointer, bytes, role-split kernel?); 0 bytes = an activation as B operand (never prefetched)
    seq = [(0x1000, 1 * MB, False), (0x2000, 4 * MB, True), (0x3000, 2 * MB, False), (0, 0, False), (0x3000, 2 * MB, False),
           (0x5000, 30 * MB, False), (0x6000, 3 * MB, True), (0x7000, 1 * MB, False)]
    pf = hip.WeightPrefetcher("cpu", window=8 * MB, self_min=0)
    pf.seq = list(seq)
    pf._build()
    # host 1 takes launches 2 .. 6: the repeated pointer once, the 30 MB weight not (window), its own successor host's weight yes
    assert pf.shares == {1: (0, 2), 6: (2, 1)}
    assert [(it[0], it[3]) for it in pf.items] == [(0x3000, 2), (0x6000, 6), (0x7000, 7)]
    raw = bytes(pf.table.numpy())
    assert len(raw) == 3 * ctypes.sizeof(hip.PrefetchItem) == 72
    first = hip.PrefetchItem.from_buffer_copy(raw[:24])
    assert first.ptr == 0x3000 and first.bytes == 2 * MB
    # self prefetch: a host whose own weight is at least self_min bytes requests it first, outside the window
    ps = hip.WeightPrefetcher("cpu", window=8 * MB, self_min=4 * MB)
    ps.seq = list(seq)
    ps._build()
    assert ps.shares == {1: (0, 3), 6: (3, 1)} and [(it[0], it[3]) for it in ps.items] == [(0x2000, 1), (0x3000, 2), (0x6000, 6), (0x7000, 7)]


def test_bench_tree_fingerprint_tracks_kernel_sources(tmp_path, monkeypatch):
    """bench.tree_fingerprint() stamps every number that is read back from profiles/ (VERDICT r04 item 7): it must change when a kernel
    source changes and only then."""
    import importlib
    bench = importlib.import_module("bench")
    a = bench.tree_fingerprint()
    assert re.fullmatch(r"[0-9a-f]{16}", a) and bench.tree_fingerprint() == a
    src = os.path.join(ROOT, "mvdfusion_amd", "csrc", "norm.hip")
    text = open(src).read()
    real_open = open

    def fake_open(path, *args, **kw):
        f = real_open(path, *args, **kw)
        if os.path.abspath(str(path)) == os.path.abspath(src) and ("b" in (args[0] if args else kw.get("mode", "r"))):
            import io
            f.close()
            return io.BytesIO(text.encode() + b"\n// edited\n")
        return f
    monkeypatch.setattr("builtins.open", fake_open)
    assert bench.tree_fingerprint() != a


# ------------------------------------------------------------------------------------------------ C ABI
def test_c_abi_library_exports_every_declared_symbol():
    from mvdfusion_amd import hip
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    declared = set(re.findall(r"\b(mvd_[a-z0-9_]+)\s*\(", hdr)) - {"mvd_gemm_desc"}
    assert declared == set(hip.SIGNATURES), declared ^ set(hip.SIGNATURES)
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert hip.lib().mvd_version() == 100
    assert hip.lib().mvd_packed_weight_bytes(320, 2880) == 320 * 2880 * 4
    assert hip.lib().mvd_attn_lpad(1000) == 1024
    assert ctypes.sizeof(hip.GemmDesc) > 0


def test_gemm_descriptor_layout_matches_the_header(tmp_path):
    """struct mvd_gemm_desc crosses the boundary by pointer: the ctypes mirror (hip.GemmDesc) must have the header's field order, offsets
    and size -- gcc compiles the header as plain C and prints offsetof() of every field; a mismatch (a field added on one side only)
    would make the library read garbage without any error."""
    import shutil
    import subprocess
    from mvdfusion_amd import hip
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    fields = [f[0] for f in hip.GemmDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mvd_hip.h"\nint main(void) {\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(mvd_gemm_desc, {f}));\n' for f in fields) +
                   '  printf("sizeof %zu\\n", sizeof(mvd_gemm_desc));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]         # (also: the header is valid C, every mirrored field exists in it)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.strip().splitlines())
    for f in fields:
        assert int(got[f]) == getattr(hip.GemmDesc, f).offset, (f, got[f], getattr(hip.GemmDesc, f).offset)
    assert int(got["sizeof"]) == ctypes.sizeof(hip.GemmDesc)
    # ... and no field of the header is missing from the mirror: count the declarators of the struct body
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    body = hdr[hdr.index("typedef struct mvd_gemm_desc"):hdr.index("} mvd_gemm_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl or decl.startswith("typedef struct"):
            decl = decl.split("{", 1)[-1].strip()
            if not decl:
                continue
        for part in decl.split(","):
            m = re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip())
            if m:
                names.append(m.group(1))
    assert names == fields, (set(names) ^ set(fields))


def test_params_signature_tracks_updates_and_does_not_cancel():
    """hip.params_signature (the guard of every packed-weight / engine / graph cache): per-tensor (pointer, version) pairs, so
    in-place updates, re-allocation and a storage SWAP between two parameters (which a xor / sum fingerprint cancels) all change it;
    `.data` writes are documented as invisible and ViewFusion.load_state_dict / _apply invalidate explicitly."""
    import torch.nn as nn
    from mvdfusion_amd import hip
    m = nn.Sequential(nn.Linear(4, 4), nn.Linear(4, 4))
    s0 = hip.params_signature(m)
    assert hip.params_signature(m) == s0
    with torch.no_grad():
        m[0].weight.add_(1.0)
    s1 = hip.params_signature(m)
    assert s1 != s0
    a, b = m[0].weight, m[1].weight
    m[0].weight, m[1].weight = b, a                       # swap: the multiset of pointers and the version sum are unchanged
    assert hip.params_signature(m) != s1
    m[0].weight, m[1].weight = a, b
    assert hip.params_signature(m) == s1
    m[1].bias = nn.Parameter(m[1].bias.detach().clone())  # re-allocation
    assert hip.params_signature(m) != s1
    from mvdfusion_amd.viewfusion_zero_depth_rgb import ViewFusion
    from conftest import model_config
    vf = ViewFusion(**model_config(32))
    vf._engines["stale"] = object()
    vf.load_state_dict(vf.state_dict(), strict=False)
    assert not vf._engines and vf._packed_sig is None
    vf._engines["stale"] = object()
    vf.float()
    assert not vf._engines


def test_kat_clip_tower_hand_computed():
    """The oracle's restatement of OpenAI clip's VisionTransformer (a package that is NOT in the reference tree) against a hand-computed
    case (conftest.clip_kat_case): class token position, patch raster order x positional embedding, 257 keys, head order, LayerNorms."""
    from conftest import clip_kat_case
    sd, img, want = clip_kat_case()
    with torch.no_grad():
        got = O.clip_encode_image(sd, "visual.", img, heads=2)
    assert rel_err(got, want) < 1e-5, rel_err(got, want)
