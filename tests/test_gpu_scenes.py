"""Batched multi-scene sampling on the GPU: N objects denoised in one step (scene-major views, global view scene*V + v).

  op level    : the *_scenes kernels on N distinct scenes are bit-identical to N single-scene launches
  step level  : one batched CFG step == N separate single-scene engines (same math, different GEMM tiling: 2e-5 relative)
  references  : a golden scene placed in a slot of a batch still meets its single-scene golden bounds (step, trajectory, feed_prev_depth)
  engine      : graph replay == eager bit for bit at N = 2;  public API: ViewFusion.sample_scenes == ViewFusion.sample per scene
"""
import pytest
import torch

from conftest import build_model, load_golden, rel_err, rmse

pytestmark = pytest.mark.gpu


def _tables():
    from mvdfusion_amd.scheduler import make_tables
    from oracle import ref_torch as O
    tab = make_tables()
    return tab, O.ddim_schedule(tab)


def _cond(inp):
    return (inp["batch_cameras"], inp["input_latents"], inp["input_cameras"], inp["clip_v_embed"])


def _own_rig(inp, seed):
    """Give a synthetic scene cameras of its own (synthetic.make_inputs puts every seed on the same GSO rig): a seed-dependent rotation
    of the world about the vertical axis plus a per-camera jitter of the translations, for the target views and the input view; the
    camera half of the CLIP / camera embedding is recomputed to match."""
    import math
    from mvdfusion_amd.cameras import Cameras
    from mvdfusion_amd.synthetic import cam_embed
    g = torch.Generator().manual_seed(500 + seed)
    a = 0.3 + 0.2 * seed
    Q = torch.tensor([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])

    def move(c):
        return Cameras(Q @ c.R, c.T + 0.05 * torch.randn(len(c), 3, generator=g), c.focal_length.clone(), c.principal_point.clone())
    out = dict(inp)
    out["batch_cameras"], out["input_cameras"] = move(inp["batch_cameras"]), move(inp["input_cameras"])
    out["clip_v_embed"] = torch.cat([inp["clip_v_embed"][..., :768], cam_embed(out["input_cameras"], out["batch_cameras"])], -1).contiguous()
    return out


def _assert_cams_differ(*inps):
    """The scenes' packed target cameras and input cameras really differ pairwise (the tests below would not see a scene reading
    another scene's cameras otherwise)."""
    from mvdfusion_amd.cameras import pack_cameras
    for i in range(len(inps)):
        for j in range(i + 1, len(inps)):
            assert not torch.allclose(pack_cameras(inps[i]["batch_cameras"]), pack_cameras(inps[j]["batch_cameras"]), atol=1e-3), (i, j)
            assert not torch.allclose(pack_cameras(inps[i]["input_cameras"]), pack_cameras(inps[j]["input_cameras"]), atol=1e-3), (i, j)


def _ga_inputs(V, D, S, seeds):
    """Per-scene GridAttn inputs of len(seeds) distinct synthetic scenes (own cameras, input view, latents and depth noise) + the shared
    step scalars.  The step table has two rows and the kernels run row 1: the per-step stride of the (steps, N*V, D, S, S) depth noise
    enters every read."""
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.cameras import pack_cameras
    tab, _ = _tables()
    rows = []
    for tval in (501, 381):
        sac = tab["sqrt_alphas_cumprod"][tval]
        dstd = tab["sqrt_one_minus_alphas_cumprod"][tval] / sac / 10.0
        rows.append([float(tval), float(sac), float(dstd), 1, 1, 0, 0, 0])
    steps = torch.tensor(rows, dtype=torch.float32).cuda()
    it = torch.ones(1, dtype=torch.int32, device="cuda")
    scenes, inps = [], []
    for s in seeds:
        inp = _own_rig(syn.make_inputs(V, S, s), s)
        inps.append(inp)
        g = torch.Generator().manual_seed(100 + s)
        scenes.append(dict(x=torch.randn(V, 5, S, S, generator=g).cuda(), dn=torch.randn(2, V, D, S, S, generator=g).cuda(),
                           cams=pack_cameras(inp["batch_cameras"]).cuda(), icam=pack_cameras(inp["input_cameras"]).cuda(),
                           il=(inp["input_latents"] + 0.1 * s).cuda()))
    _assert_cams_differ(*inps)
    c = (torch.randn(1, 256, generator=torch.Generator().manual_seed(17)) * 0.5).cuda()
    return steps, it, c, scenes


def _ga_run(ga, ctx, scenes, steps, it, c, V, S, D, fused):
    """GridAttn over the given scenes in ONE call; returns (pooled planes, token planes or None) as host copies."""
    from mvdfusion_amd import hip
    N = len(scenes)
    cat = lambda k: torch.cat([sc[k] for sc in scenes], 1 if k == "dn" else 0).contiguous()
    vol = torch.zeros(N * V * S * S * D, 768, device="cuda")
    ga.run(ctx, cat("x"), cat("dn"), steps, it, cat("cams"), cat("icam"), cat("il"), c, vol, V, S, D, fused=fused, scenes=N)
    torch.cuda.synchronize()
    nseq = N * V * S * S * D
    pool = ctx.ws.planes("ga.pool", nseq, 256).cpu().clone()
    tok = None if fused else ctx.ws.planes("ga.tokens", nseq * V, hip.TOKEN_LD).cpu().clone()
    return pool, tok, vol.cpu()


@pytest.mark.parametrize("V,D,fused", [(4, 1, True), (5, 3, True), (15, 1, True), (4, 1, False), (15, 1, False)])
def test_gridattn_scenes_bitwise_equal_to_single_scene_launches(V, D, fused):
    """mvd_gridattn_fused_scenes / mvd_gridattn_tokens_scenes on N = 3 distinct scenes == three single-scene launches, bit for bit
    (pooled planes of the fused kernel, token planes of the unfused chain, whose pooled rows come out of GEMMs at another M: 2e-5).
    V = 5 exercises the padding slots.  (V = 16 is the largest view count mvd_gridattn_tokens accepts, as before.)"""
    from mvdfusion_amd.engine import Ctx
    S = 32
    m = build_model(32, D=D)
    ga = m.view_attn
    steps, it, c, scenes = _ga_inputs(V, D, S, (3, 7, 11))
    ctx = Ctx("cuda")
    pool3, tok3, vol3 = _ga_run(ga, ctx, scenes, steps, it, c, V, S, D, fused)
    rows = V * S * S * D
    for n, sc in enumerate(scenes):
        pool1, tok1, vol1 = _ga_run(ga, ctx, [sc], steps, it, c, V, S, D, fused)
        if fused:
            assert torch.equal(pool3[n * rows:(n + 1) * rows], pool1), n
        else:
            assert torch.equal(tok3[n * rows * V:(n + 1) * rows * V], tok1), n
        assert rel_err(vol3[n * rows:(n + 1) * rows], vol1) < 2e-5, n       # (the GEMMs run at another M: tiling may differ)
    assert not torch.equal(pool3[:rows], pool3[rows:2 * rows])               # the scenes really differ


@pytest.mark.parametrize("cfg", [1, 0])
def test_unet_input_scenes_bitwise(cfg):
    from mvdfusion_amd import hip
    N, V, S, cpad = 3, 4, 32, 32
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N * V, 5, S, S, generator=g).cuda()
    il = torch.randn(N, 5, S, S, generator=g).cuda()
    L = hip.lib()
    nb = (2 if cfg else 1) * N * V
    out = torch.full((nb * S * S, 2 * cpad), 7, dtype=torch.int16, device="cuda")
    hip.check(L.mvd_unet_input_scenes(hip.ptr(x), hip.ptr(il), hip.ptr(out), N, V, S, cpad, cfg, hip.stream()))
    rows = V * S * S
    singles = []
    for n in range(N):
        o = torch.full(((2 if cfg else 1) * rows, 2 * cpad), 7, dtype=torch.int16, device="cuda")
        hip.check(L.mvd_unet_input(hip.ptr(x[n * V:(n + 1) * V]), hip.ptr(il[n:n + 1]), hip.ptr(o), V, S, cpad, cfg, hip.stream()))
        singles.append(o)
    torch.cuda.synchronize()
    assert torch.equal(out[:N * rows], torch.cat([o[:rows] for o in singles]))
    if cfg:
        assert torch.equal(out[N * rows:], torch.cat([o[rows:] for o in singles]))
    assert hip.lib().mvd_unet_input_scenes(hip.ptr(x), hip.ptr(il), hip.ptr(out), 0, V, S, cpad, cfg, hip.stream()) != 0


def _single_step(m, inp, dn, sn, index, V, S, D, use_graph=False):
    from mvdfusion_amd.engine import ddim_step_table
    tab, dd = _tables()
    eng = m.engine(V, S, D, True)
    eng.set_conditioning(inp["batch_cameras"], inp["input_latents"].cuda(), inp["input_cameras"], inp["clip_v_embed"].cuda())
    eng.set_schedule(ddim_step_table(tab, dd, [index]), dn.reshape(1, V, D, S, S), sn.reshape(1, V, 5, S, S))
    eng.x.copy_(inp["x_T"])
    eng.step(2.5, do_update=True, use_graph=use_graph)
    torch.cuda.synchronize()
    return eng.x.cpu(), eng.x0.cpu()


def _scene_step(m, inps, dns, sns, index, V, S, D, use_graph=False):
    from mvdfusion_amd.cameras import pack_cameras
    from mvdfusion_amd.engine import ddim_step_table
    tab, dd = _tables()
    N = len(inps)
    eng = m.engine(V, S, D, True, scenes=N)
    eng.set_conditioning_scenes([(i["batch_cameras"], i["input_latents"].cuda(), i["input_cameras"], i["clip_v_embed"].cuda())
                                 for i in inps])
    eng.set_schedule(ddim_step_table(tab, dd, [index]), torch.cat([d.reshape(1, V, D, S, S) for d in dns], 1),
                     torch.cat([s.reshape(1, V, 5, S, S) for s in sns], 1))
    eng.x.copy_(torch.cat([i["x_T"] for i in inps]))
    for n, i in enumerate(inps):       # every scene's cameras in its own slots of the engine's buffers
        assert torch.equal(eng.cams[n * V:(n + 1) * V].cpu(), pack_cameras(i["batch_cameras"]))
        assert torch.equal(eng.in_cam[n:n + 1].cpu(), pack_cameras(i["input_cameras"]))
    eng.step(2.5, do_update=True, use_graph=use_graph)
    torch.cuda.synchronize()
    return eng.x.cpu().view(N, V, 5, S, S), eng.x0.cpu().view(N, V, 5, S, S)


@pytest.mark.parametrize("fused", [None, False])
def test_one_step_equals_separate_engines(fused, monkeypatch):
    from mvdfusion_amd import synthetic as syn
    m = build_model(32)
    if fused is False:        # force the unfused chain (token kernel + GEMMs + view MHA / pooling) for both paths
        monkeypatch.setattr(m.view_attn, "fused_supported", lambda V, T: False)
    V, S, D = 4, 32, 1
    inps = [_own_rig(syn.make_inputs(V, S, seed=s), s) for s in (3, 7, 11)]
    _assert_cams_differ(*inps)
    noise = [syn.step_noise(V, S, D, 2, seed=s) for s in (3, 7, 11)]
    dns, sns = [n[0][:1] for n in noise], [n[1][:1] for n in noise]
    xs, x0s = _scene_step(m, inps, dns, sns, 40, V, S, D)
    for n in range(3):
        x1, x01 = _single_step(m, inps[n], dns[n], sns[n], 40, V, S, D)
        assert rel_err(xs[n], x1) < 2e-5 and rel_err(x0s[n], x01) < 2e-5, (n, rel_err(xs[n], x1), rel_err(x0s[n], x01))
    assert not torch.allclose(xs[0], xs[1])


def test_batched_step_golden_scene_in_slot_1_full_width():
    """step_mc320_v4_d1 (the reference's denoise_apply at full width) in slot 1 of an N = 2 batch, a synthetic scene in slot 0: slot 1
    meets test_denoise_step_vs_reference_golden's bounds."""
    from mvdfusion_amd import synthetic as syn
    gd = load_golden("step_mc320_v4_d1")
    m = build_model(320)
    V, S, D, index = 4, 32, 1, 49
    gold = syn.make_inputs(V, S, seed=7)
    if f"depth_noise_{index}" in gd:
        dn, sn, gold["x_T"] = gd[f"depth_noise_{index}"], gd[f"step_noise_{index}"], gd["x"]
    else:
        torch.manual_seed(int(gd["noise_seed_base"]) + index)
        dn = torch.randn(V, D, S, S)
        sn = torch.randn(V, 5, S, S) if index > 0 else torch.zeros(V, 5, S, S)
    other = _own_rig(syn.make_inputs(V, S, seed=2), 2)        # its own cameras: slot 1 must read the golden's
    _assert_cams_differ(other, gold)
    dn0, sn0 = syn.step_noise(V, S, D, 2, seed=2)
    xs, x0s = _scene_step(m, [other, gold], [dn0[:1], dn], [sn0[:1], sn], index, V, S, D)
    xp, x0 = xs[1], x0s[1]
    assert rmse(xp, gd[f"x_prev_{index}"]) < 1e-4 and rel_err(xp, gd[f"x_prev_{index}"]) < 3e-4
    assert rmse(x0, gd[f"x0_{index}"]) < 2e-3 and rel_err(x0, gd[f"x0_{index}"]) < 3e-4


def _scene_noise_source(noises):
    """noise_source that hands scene k (k-th call) its own draws -- sample_scenes calls it once per scene, in order."""
    calls = []

    def source(V, S, D, total):
        k = len(calls) % len(noises)
        calls.append(k)
        return noises[k]
    return source, calls


def test_sample_scenes_trajectory_vs_golden_and_single_scene():
    from mvdfusion_amd import synthetic as syn
    gd = load_golden("traj_mc32_v4_d1")
    m = build_model(32)
    V, S, D, steps = 4, 32, 1, 5
    seeds = (5, 11)                                    # slot 1: the traj_mc32_v4_d1 scene
    inps = [_own_rig(syn.make_inputs(V, S, seed=5), 5), syn.make_inputs(V, S, seed=11)]
    _assert_cams_differ(*inps)
    noises = [syn.step_noise(V, S, D, 50, seed=s) for s in seeds]
    src, calls = _scene_noise_source(noises)
    m.ddim.noise_source = src
    try:
        x, inter = m.ddim.sample_scenes([_cond(i) for i in inps], unconditional_scale=2.5, return_intermediates=True, verbose=False,
                                        x_T=torch.stack([i["x_T"] for i in inps]).cuda(), num_steps=steps)
        assert calls == [0, 1]
        assert x.shape == (2, V, 5, S, S) and len(inter) == steps
        for i, itm in enumerate(inter):
            assert rmse(itm["xt"][1], gd["xs"][i]) < 1e-3, (i, rmse(itm["xt"][1], gd["xs"][i]))
        for n, inp in enumerate(inps):
            m.ddim.noise_source = lambda *a, n=n: noises[n]
            x1, inter1 = m.ddim.sample(*_cond(inp), unconditional_scale=2.5, depth=True, return_intermediates=True, verbose=False,
                                       x_T=inp["x_T"].cuda(), num_steps=steps)
            for i in range(steps):
                assert rmse(inter[i]["xt"][n], inter1[i]["xt"]) < 1e-4, (n, i)
            assert rmse(x[n], x1) < 1e-4
    finally:
        m.ddim.noise_source = None


def test_sample_scenes_feed_prev_depth_vs_reference_golden():
    from conftest import model_config
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.viewfusion_zero_depth_rgb import ViewFusion
    gd = load_golden("sample_prevdepth_mc32_v2")
    V, S, steps = 2, 32, int(gd["xs"].shape[0])
    cfg = model_config(32)
    cfg["feed_prev_depth"] = True
    with syn.skip_default_init():
        m = ViewFusion(**cfg)
    syn.fill_module_(m)
    m = m.cuda().eval()
    gold = syn.make_inputs(V, S, seed=9)
    dn = torch.zeros(50, V, 1, S, S)
    sn = torch.zeros(50, V, 5, S, S)
    dn[:steps], sn[:steps] = gd["depth_noise"], gd["step_noise"]
    other = _own_rig(syn.make_inputs(V, S, seed=4), 4)
    _assert_cams_differ(gold, other)
    src, calls = _scene_noise_source([(dn, sn), syn.step_noise(V, S, 1, 50, seed=4)])
    m.ddim.noise_source = src
    x, inter = m.ddim.sample_scenes([_cond(gold), _cond(other)], unconditional_scale=2.5, return_intermediates=True, verbose=False,
                                    x_T=torch.stack([gd["x_T"], other["x_T"]]).cuda(), num_steps=steps)
    for i, itm in enumerate(inter):
        assert rmse(itm["xt"][0], gd["xs"][i]) < 2e-4 and rmse(itm["x0"][0], gd["x0s"][i]) < 2e-3, (i, rmse(itm["xt"][0], gd["xs"][i]))


def test_scene_graph_replay_equals_eager():
    from mvdfusion_amd import synthetic as syn
    m = build_model(32)
    V, S, D = 4, 32, 1
    inps = [_own_rig(syn.make_inputs(V, S, seed=s), s) for s in (1, 2)]
    noise = [syn.step_noise(V, S, D, 2, seed=s) for s in (1, 2)]
    dns, sns = [n[0][:1] for n in noise], [n[1][:1] for n in noise]
    xg, x0g = _scene_step(m, inps, dns, sns, 49, V, S, D, use_graph=True)
    xe, x0e = _scene_step(m, inps, dns, sns, 49, V, S, D, use_graph=False)
    xg2, _ = _scene_step(m, inps, dns, sns, 49, V, S, D, use_graph=True)      # replay of the cached graph
    assert torch.equal(xe, xg) and torch.equal(x0e, x0g) and torch.equal(xg, xg2)


def test_viewfusion_sample_scenes_matches_sample_per_scene():
    """The public API on two small batches (HIP VAE encode, stub CLIP, 4 DDIM steps): per-scene return structure and shapes, and each scene
    equal to ViewFusion.sample on the same batch with the same injected noise."""
    from conftest import model_config
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.viewfusion_zero_depth_rgb import ViewFusion
    dd = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2, 4, 4],
              num_res_blocks=2, attn_resolutions=[], dropout=0.0)
    cfg = model_config(32)
    cfg["vae_config"] = dict(target="external.sd1.ldm.models.autoencoder.AutoencoderKL",
                             params=dict(embed_dim=4, ddconfig=dd, lossconfig=dict(target="torch.nn.Identity")))
    with syn.skip_default_init():
        m = ViewFusion(clip_image_encoder=syn.StubClipImageEncoder(), **cfg)
    syn.fill_module_(m)
    m = m.cuda().eval()
    m.ddim._make_schedule(4, 1.0)                      # a 4-step DDIM schedule: the test checks plumbing, not the 50-step sample
    V, S = 3, 32
    rig = syn.gso_rig()
    # each batch on its own rig (translations jittered per camera: prepare_batch's relative cameras differ between the two)
    batches = [dict(images=torch.rand(16, 3, 256, 256, generator=torch.Generator().manual_seed(s)).cuda(), R=rig.R.clone(),
                    T=rig.T + 0.05 * torch.randn(16, 3, generator=torch.Generator().manual_seed(600 + s)),
                    f=rig.focal_length, c=rig.principal_point) for s in (3, 8)]
    tc = dict(input_batch_size=1, train_batch_size=V, random_views=False, cfg_scale=2.5)
    noises = [syn.step_noise(V, S, 1, 4, seed=s) for s in (3, 8)]
    x_T = torch.randn(2, V, 5, S, S, generator=torch.Generator().manual_seed(21)).cuda()
    src, calls = _scene_noise_source(noises)
    m.ddim.noise_source = src
    real_scenes, real_sample = m.ddim.sample_scenes, m.ddim.sample
    m.ddim.sample_scenes = lambda conds, **kw: real_scenes(conds, x_T=x_T, **kw)
    outs = m.sample_scenes(batches, tc, cfg_scale=2.5, return_input=True, depth=True, verbose=False)
    assert calls == [0, 1] and len(outs) == 2
    from mvdfusion_amd.cameras import pack_cameras
    assert not torch.allclose(pack_cameras(outs[0][3]), pack_cameras(outs[1][3]), atol=1e-3)
    for n, (batch, o) in enumerate(zip(batches, outs)):
        assert len(o) == 5
        x, batch_latents, input_latents, batch_cameras, inter = o
        assert x.shape == (V, 5, S, S) and batch_latents.shape == (V, 5, S, S) and input_latents.shape == (1, 5, S, S)
        assert len(batch_cameras) == V and len(inter) == 4 and inter[0]["xt"].shape == (V, 5, S, S)
        m.ddim.noise_source = lambda *a, n=n: noises[n]
        m.ddim.sample = lambda *a, n=n, **kw: real_sample(*a, x_T=x_T[n], **kw)
        x1 = m.sample(batch, tc, cfg_scale=2.5, depth=True, verbose=False)
        assert rmse(x, x1) < 1e-4, (n, rmse(x, x1))
        assert torch.equal(batch_latents, m.prepare_batch(batch, tc)[0])
    xs = m.sample_scenes(batches, tc, cfg_scale=2.5, depth=True, verbose=False)
    assert len(xs) == 2 and all(t.shape == (V, 5, S, S) for t in xs)
