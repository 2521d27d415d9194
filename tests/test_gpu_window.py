"""Windowed cross-view aggregation (GridAttn keep_top_k_views=True) on the GPU.

  references : the REAL reference's windowed frustum (gridattn_topk*: fused x4, unfused x4, fused x3), its denoising steps through engine,
               graph and update (step_*_topk4) and its loss.backward() (train_grads_*_topk2) -- tools/make_golden_window.py;
               W = V meets the FULL-attention golden gridattn_v5_d3 (attention and pooling over a set do not depend on the slot order)
  op level   : a windowed token row is, bit for bit, the full launch's row of the view the slot -> view rule names; scenes, shards
               (q0 / Vq) and per-scene step rows of the *_window kernels equal the single launches they stand for, bit for bit
  model level: gradients_scenes == mean of single-scene steps; sample_scenes == sample per scene

Tolerances are the ones the same operator / step / gradients carry without a window (test_gpu_model.py, test_gpu_vae.py,
test_gpu_train_scenes.py, test_gpu_scenes.py)."""
import pytest
import torch

from conftest import load_golden, model_config, planes_to_float, rel_err, rmse

pytestmark = pytest.mark.gpu

_MODELS = {}


def _window_cfg(top_k, mc=32, D=1):
    cfg = model_config(mc, D=D)
    va = cfg["view_attn_config"]
    cfg["view_attn_config"] = dict(va, params=dict(va["params"], keep_top_k_views=True, top_k=top_k))
    return cfg


def _window_model(top_k, D=1):
    """conftest.build_model with the yaml key set: ViewFusion on cuda:0, deterministic fill (cached)."""
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.viewfusion_zero_depth_rgb import ViewFusion
    key = (top_k, D)
    if key not in _MODELS:
        with syn.skip_default_init():
            m = ViewFusion(**_window_cfg(top_k, D=D))
        syn.fill_module_(m)
        _MODELS[key] = m.cuda().eval()
    return _MODELS[key]


def _tables():
    from mvdfusion_amd.scheduler import make_tables
    return make_tables()


def _step_rows(ts):
    tab = _tables()
    out = []
    for t in ts:
        sac = float(tab["sqrt_alphas_cumprod"][t])
        out.append([float(t), sac, float(tab["sqrt_one_minus_alphas_cumprod"][t]) / sac / 10.0, 1.0, 1.0, 0.0, 0.0, 0.0])
    return out


# ------------------------------------------------------------------------------------------------ against the reference
def _run_gridattn_case(ga, gd, V, D, seed, tval, lattice):
    """fused x4, unfused x4 and fused x3 of one GridAttn forward against a reference fixture (the body of
    test_gpu_model.py::test_gridattn_vs_reference_golden, over the fixture's own lattice)."""
    from mvdfusion_amd import hip
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.cameras import pack_cameras
    from mvdfusion_amd.engine import Ctx
    S = 32
    sy, sx, sc = lattice
    ctx = Ctx("cuda")
    inp = syn.make_inputs(V, S, seed)
    steps = torch.tensor(_step_rows([tval]), dtype=torch.float32).cuda()
    it = torch.zeros(1, dtype=torch.int32, device="cuda")
    vol = torch.zeros(V * S * S * D, 768, device="cuda")
    volp = hip.planes_like(V * S * S * D, 768, "cuda")
    c = gd["t_embed"][:1].contiguous().cuda()
    args = (gd["x"].cuda(), gd["depth_noise"].reshape(1, V, D, S, S).cuda(), steps, it,
            pack_cameras(inp["batch_cameras"]).cuda(), pack_cameras(inp["input_cameras"]).cuda(),
            inp["input_latents"].cuda(), c, vol, V, S, D)
    assert ga.fused_supported(V, V * S * S * D * ga.rows_per_point(V))
    ref_s = gd["out_strided"]
    for fused in (True, False):
        vol.zero_()
        ga.run(ctx, *args, vol_planes=volp, fused=fused)
        out = vol.view(V, S, S, D, 768).cpu()
        e_pl = rel_err(planes_to_float(volp).view(V, S, S, D, 768), out)
        e_max = float((out[:, ::sy, ::sx, :, ::sc] - ref_s).abs().max()) / float(ref_s.abs().max())
        e_std = abs(float(out.std()) - float(gd["out_std"])) / float(gd["out_std"])
        e_l2 = abs(float(out.norm()) - float(gd["out_l2"])) / float(gd["out_l2"])
        print(f"V={V} D={D} W={ga.window} fused={fused}: lattice {e_max:.2e} std {e_std:.2e} l2 {e_l2:.2e} planes {e_pl:.2e}")
        assert e_pl < 2e-5
        assert e_max < 2e-4, fused
        assert e_std < 1e-4 and e_l2 < 1e-4, fused
    ctx3 = Ctx("cuda", prec=hip.PREC_X3)
    vol3 = torch.zeros_like(vol)
    ga.run(ctx3, *args[:8], vol3, *args[9:], vol_planes=volp, fused=True)
    e3 = float((vol3.view(V, S, S, D, 768).cpu()[:, ::sy, ::sx, :, ::sc] - ref_s).abs().max()) / float(ref_s.abs().max())
    print(f"V={V} D={D} W={ga.window} fused x3: lattice {e3:.2e}, vs unfused x4 {rel_err(vol3, vol):.2e}")
    assert e3 < 2e-4
    assert rel_err(vol3, vol) < 2e-5                      # (vol: the unfused chain at four products)


@pytest.mark.parametrize("name,V,D,top_k,seed,tval", [
    ("gridattn_topk4_v8_d1", 8, 1, 4, 12, 21),          # W = 5 -> 8 slots, the window wraps at both ends of the rig
    ("gridattn_topk4_v15_d1", 15, 1, 4, 13, 741),       # the shipped view count: 16 -> 8 slots
    ("gridattn_topk2_v8_d3", 8, 3, 2, 14, 501),         # W = 3 -> 4 slots, training depth samples
    ("gridattn_topk4_v3_d3", 3, 3, 4, 15, 161),         # W > V: repeated views
    ("gridattn_topk4_v24_d1", 24, 1, 4, 16, 381)])      # a rig above the 16 rows of a point
def test_windowed_gridattn_vs_reference_golden(name, V, D, top_k, seed, tval):
    gd = load_golden(name)
    assert int(gd["top_k"]) == top_k and int(gd["seed"]) == seed and int(gd["t"][0]) == tval
    ga = _window_model(top_k, D=D).view_attn
    assert ga.window == 2 * (top_k // 2) + 1
    _run_gridattn_case(ga, gd, V, D, seed, tval, tuple(int(v) for v in gd["lattice"]))


def test_window_covering_the_rig_meets_the_full_attention_golden():
    """V = 5, top_k = 4: W = V, every point sees every view (in rotated order) -- the windowed kernels against the reference's
    FULL-attention output (gridattn_v5_d3, the fixture of test_gridattn_vs_reference_golden), independent of the windowed fixtures."""
    gd = load_golden("gridattn_v5_d3")
    ga = _window_model(4, D=3).view_attn
    assert ga.window == 5
    _run_gridattn_case(ga, gd, 5, 3, 9, 161, (5, 7, 3))


@pytest.mark.parametrize("name,V,top_k", [("step_mc32_v8_d1_topk4", 8, 4), ("step_mc32_v24_d1_topk4", 24, 4)])
def test_windowed_denoise_step_vs_reference_golden(name, V, top_k):
    """DDIMSampler.denoise_apply with the windowed GridAttn through engine, graph and update, at the bounds of
    test_gpu_model.py::test_denoise_step_vs_reference_golden; the captured graph replays the eager step bit for bit."""
    from test_gpu_model import _run_step
    gd = load_golden(name)
    assert int(gd["top_k"]) == top_k
    views = gd["views"]
    m = _window_model(top_k)
    for index in (int(i) for i in gd["indices"]):
        # (graph first: its warm-up step picks the GEMM configurations of these shapes, which the eager step then uses too --
        #  the order of test_gpu_model.py::test_full_size_config3_properties)
        xg, x0g = _run_step(m, gd, V, 1, index, 7, use_graph=True)
        xp, x0 = _run_step(m, gd, V, 1, index, 7, use_graph=False)
        e = (rmse(xp[views], gd[f"x_prev_{index}"]), rel_err(xp[views], gd[f"x_prev_{index}"]),
             rmse(x0[views], gd[f"x0_{index}"]), rel_err(x0[views], gd[f"x0_{index}"]))
        print(f"{name} index {index}: x_prev rmse {e[0]:.2e} rel {e[1]:.2e}; x0 rmse {e[2]:.2e} rel {e[3]:.2e}")
        assert e[0] < 1e-4 and e[1] < 3e-4, index
        assert e[2] < 2e-3 and e[3] < 3e-4, index
        assert torch.equal(xg, xp) and torch.equal(x0g, x0), index


def _train_setup(V=8, top_k=2):
    from test_gpu_vae import _training_setup
    gd = load_golden("train_grads_mc32_v8_d3_topk2")
    assert int(gd["top_k"]) == top_k
    m, batch, tc, draws = _training_setup(gd, mc=32, V=V, view_attn_config=_window_cfg(top_k, D=3)["view_attn_config"])
    assert m.view_attn.window == 3
    return gd, m, batch, tc, draws


def test_windowed_training_gradients_vs_reference_golden():
    """loss.backward() with the windowed GridAttn (V = 8, D = 3, top_k = 2): the loss and ALL 994 parameter gradients against the REAL
    reference's autograd, at the bounds of test_gpu_vae.py::test_training_all_gradients_vs_reference_golden."""
    gd, m, batch, tc, draws = _train_setup()
    loss, grads = m.gradients(batch, tc, noise_source=draws)
    print(f"loss {float(loss):.7f} vs reference {float(gd['loss']):.7f}")
    assert abs(float(loss) - float(gd["loss"])) / float(gd["loss"]) < 1e-4
    names = [str(n) for n in gd["grad_names"]]
    norms, projs = gd["grad_norms"].double(), gd["grad_projs"].double()
    assert len(names) == 994
    missing, bad, worst = [], [], 0.0
    for i, n in enumerate(names):
        if n not in grads:
            missing.append(n)
            continue
        gq = grads[n].detach().double().cpu().flatten()
        r = torch.randn(gq.numel(), generator=torch.Generator().manual_seed(1000 + i)).double()
        nr, pr = float(norms[i]), float(projs[i])
        e_n, e_p = abs(float(gq.norm()) - nr), abs(float((gq * r).sum()) - pr)
        tol = 1e-4 * nr + 2e-8 * gq.numel() ** 0.5
        if e_n > tol or e_p > tol:
            bad.append((n, nr, e_n, e_p))
        if nr > 1e-6:
            worst = max(worst, e_n / nr, e_p / nr)
        if n.startswith(("view_attn.", "time_embed.")):
            print(f"{n:75s} |g| {nr:.3e}  d|g| {e_n:.1e}  dproj {e_p:.1e}")
    print(f"all {len(names)} parameter gradients compared, worst relative deviation {worst:.2e}")
    assert not missing, missing[:10]
    assert not bad, bad[:10]


def test_windowed_gradients_scenes_equal_mean_of_single_scene_steps():
    from test_gpu_train_scenes import _chain, _compare, _scene_batches, _seed_draws
    _, m, batch, tc, _ = _train_setup()
    N, V, S, D = 2, 8, 32, 3
    scenes = _scene_batches(m, batch, tc, N)
    seeds = [41, 58]
    ts = [int(_seed_draws(s)(V, D, S)["t"][0]) for s in seeds]
    assert len(set(ts)) == N, ts
    refs, losses = [], []
    for sc, sd in zip(scenes, seeds):
        l1, g1 = m.gradients(sc, tc, noise_source=_seed_draws(sd))
        losses.append(float(l1))
        refs.append({k: (None if v is None else v.clone()) for k, v in g1.items()})
    lossN, gN = m.gradients_scenes(scenes, tc, noise_source=_chain([_seed_draws(s) for s in seeds]))
    ref_loss = sum(losses) / N
    print(f"timesteps {ts}: loss {float(lossN):.7f} vs mean of single-scene losses {ref_loss:.7f}")
    assert abs(float(lossN) - ref_loss) <= 1e-6 * abs(ref_loss)
    bad, count = _compare(gN, refs, N, "mc32 V=8 D=3 top_k=2 N=2")
    assert count == 994
    assert not bad, bad[:10]


def test_windowed_sample_scenes_matches_sample_per_scene():
    """ViewFusion.sample_scenes of a windowed model (N = 2, own rigs) == ViewFusion.sample per scene under the same noise_source:
    latent RMSE < 1e-4 (test_gpu_scenes.py::test_viewfusion_sample_scenes_matches_sample_per_scene)."""
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.viewfusion_zero_depth_rgb import ViewFusion
    from test_gpu_scenes import _scene_noise_source
    dd = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2, 4, 4],
              num_res_blocks=2, attn_resolutions=[], dropout=0.0)
    cfg = _window_cfg(2)
    cfg["vae_config"] = dict(target="external.sd1.ldm.models.autoencoder.AutoencoderKL",
                             params=dict(embed_dim=4, ddconfig=dd, lossconfig=dict(target="torch.nn.Identity")))
    with syn.skip_default_init():
        m = ViewFusion(clip_image_encoder=syn.StubClipImageEncoder(), **cfg)
    syn.fill_module_(m)
    m = m.cuda().eval()
    assert m.view_attn.window == 3
    m.ddim._make_schedule(4, 1.0)
    V, S = 6, 32
    rig = syn.gso_rig()
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
    outs = m.sample_scenes(batches, tc, cfg_scale=2.5, depth=True, verbose=False)
    assert calls == [0, 1] and len(outs) == 2
    for n, (batch, x) in enumerate(zip(batches, outs)):
        m.ddim.noise_source = lambda *a, n=n: noises[n]
        m.ddim.sample = lambda *a, n=n, **kw: real_sample(*a, x_T=x_T[n], **kw)
        x1 = m.sample(batch, tc, cfg_scale=2.5, depth=True, verbose=False)
        print(f"scene {n}: latent RMSE sample_scenes vs sample {rmse(x, x1):.2e}")
        assert bool(torch.isfinite(x).all()) and rmse(x, x1) < 1e-4, (n, rmse(x, x1))
    assert not torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ op level (C ABI, bit equalities)
@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


def _geo(N, V, S, D, ts, seed=3):
    """Inputs of the *_window kernels for N scenes, every scene on a rig of its own, with a two-row-per-scene-capable step table."""
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.cameras import pack_cameras
    from test_gpu_scenes import _own_rig
    g = torch.Generator().manual_seed(seed)
    inps = [_own_rig(syn.make_inputs(V, S, seed=seed + n), seed + n) for n in range(N)]
    q = dict(x=(torch.randn(N * V, 5, S, S, generator=g) * 0.5).cuda(), dn=torch.randn(1, N * V, D, S, S, generator=g).cuda(),
             cams=torch.cat([pack_cameras(i["batch_cameras"]) for i in inps]).cuda(),
             in_cam=torch.cat([pack_cameras(i["input_cameras"]) for i in inps]).cuda(),
             steps=torch.tensor(_step_rows(ts), dtype=torch.float32).cuda(), feat=torch.randn(N * V, S, S, 256, generator=g).cuda(),
             in_feat=torch.randn(N, S, S, 256, generator=g).cuda(), lin=torch.linspace(1.0 - 1.0 / S, -1.0 + 1.0 / S, S).cuda(),
             it=torch.zeros(1, dtype=torch.int32).cuda())
    if N > 1:
        assert not torch.allclose(q["cams"][:V], q["cams"][V:2 * V], atol=1e-3)
    return q


def _scene(q, n, V):
    sub = dict(q)
    sub.update(x=q["x"][n * V:(n + 1) * V].contiguous(), cams=q["cams"][n * V:(n + 1) * V].contiguous(),
               in_cam=q["in_cam"][n:n + 1].contiguous(), feat=q["feat"][n * V:(n + 1) * V].contiguous(),
               in_feat=q["in_feat"][n:n + 1].contiguous(), dn=q["dn"][:, n * V:(n + 1) * V].contiguous())
    return sub


def _tokens(hip, q, N, V, S, D, window, q0=0, Vq=None, sst=0, steps=None):
    Vq = V if Vq is None else Vq
    T = N * Vq * S * S * D * (window or V)
    tok = hip.planes_like(T, hip.TOKEN_LD, q["x"].device).zero_()
    st = q["steps"] if steps is None else steps
    hip.check(hip.lib().mvd_gridattn_tokens_window(hip.ptr(q["x"]), hip.ptr(q["dn"]), hip.ptr(st), hip.ptr(q["it"]), hip.ptr(q["lin"]),
                                                   hip.ptr(q["feat"]), hip.ptr(q["in_feat"]), hip.ptr(q["cams"]), hip.ptr(q["in_cam"]),
                                                   hip.ptr(tok), N, V, q0, Vq, S, D, 2.0, 0.5, sst, window, hip.stream()))
    torch.cuda.synchronize()
    return tok


def _fused(hip, ga, q, N, V, S, D, window, vecs, q0=0, Vq=None, sst=0, vst=0, steps=None):
    Vq = V if Vq is None else Vq
    stream, _ = ga.packed_fused(torch.device("cuda"))
    pool = hip.planes_like(N * Vq * S * S * D, 256, q["x"].device).zero_()
    st = q["steps"] if steps is None else steps
    hip.check(hip.lib().mvd_gridattn_fused_window(hip.ptr(q["x"]), hip.ptr(q["dn"]), hip.ptr(st), hip.ptr(q["it"]), hip.ptr(q["lin"]),
                                                  hip.ptr(q["feat"]), hip.ptr(q["in_feat"]), hip.ptr(q["cams"]), hip.ptr(q["in_cam"]),
                                                  hip.ptr(stream), hip.ptr(vecs), hip.ptr(pool), N, V, q0, Vq, S, D, 2.0, 0.5, 4, sst, vst,
                                                  window, hip.stream()))
    torch.cuda.synchronize()
    return pool


@pytest.mark.parametrize("V,top_k", [(8, 4), (8, 2), (3, 4), (15, 4)])
def test_windowed_token_rows_are_the_full_launch_rows_the_rule_names(hip, V, top_k):
    """Token row (point, slot j) of the windowed launch == row (point, view (b + j - W/2) mod V) of the all-views launch, bit for bit
    (a token row depends on its point and its reference view only) -- the slot -> view rule, independent of any fixture.
    window = 0 through the new entry point is the existing kernel."""
    from mvdfusion_amd.view_attn_efficient2 import window_view_table
    S, D = 16, 2
    W = 2 * (top_k // 2) + 1
    q = _geo(1, V, S, D, [381])
    full = _tokens(hip, q, 1, V, S, D, 0).view(V, S * S * D, V, -1)
    ref = hip.planes_like(V * S * S * D * V, hip.TOKEN_LD, "cuda").zero_()
    hip.check(hip.lib().mvd_gridattn_tokens_scenes_t(hip.ptr(q["x"]), hip.ptr(q["dn"]), hip.ptr(q["steps"]), hip.ptr(q["it"]), hip.ptr(q["lin"]),
                                                     hip.ptr(q["feat"]), hip.ptr(q["in_feat"]), hip.ptr(q["cams"]), hip.ptr(q["in_cam"]),
                                                     hip.ptr(ref), 1, V, 0, V, S, D, 2.0, 0.5, 0, hip.stream()))
    torch.cuda.synchronize()
    assert torch.equal(full.reshape(ref.shape), ref)
    win = _tokens(hip, q, 1, V, S, D, W).view(V, S * S * D, W, -1)
    table = window_view_table(V, top_k)                     # (W, V)
    for b in range(V):
        assert torch.equal(win[b], full[b][:, table[:, b].cuda()]), b
    assert not torch.equal(full[0][:, 0], full[0][:, 1 % V]) or V == 1


@pytest.mark.parametrize("V,top_k,D", [(8, 4, 1), (5, 2, 2)])
def test_windowed_kernels_scenes_shards_and_step_rows_bitwise(hip, V, top_k, D):
    """mvd_gridattn_tokens_window / mvd_gridattn_fused_window: two scenes on different rigs in one launch == two single-scene launches;
    a shard q0 = 2, Vq = 3 == those rows of the unsharded launch (the window is taken in the WHOLE rig); per-scene step rows (and vector
    tables) == single launches at that row -- all bit for bit."""
    from conftest import build_model
    S, N = 16, 2
    W = 2 * (top_k // 2) + 1
    ga = build_model(32, D=D).view_attn                     # (weights only: the window is an argument of the entry points here)
    q = _geo(N, V, S, D, [999, 10])
    _, vecs1 = ga.packed_fused(torch.device("cuda"))
    nv = vecs1.numel()
    vecs = vecs1.view(1, nv).repeat(N, 1)
    g = torch.Generator().manual_seed(13)
    for bi in range(3):                                    # a distinct adaLN modulation per scene
        vecs[:, bi * 3328:bi * 3328 + 1536] = (0.1 * torch.randn(N, 1536, generator=g)).cuda()
    v0 = vecs[0].contiguous()
    # scenes, shared step row
    tokN, poolN = _tokens(hip, q, N, V, S, D, W), _fused(hip, ga, q, N, V, S, D, W, v0)
    # scenes, a step row (and vector table) per scene
    tokT, poolT = _tokens(hip, q, N, V, S, D, W, sst=1), _fused(hip, ga, q, N, V, S, D, W, vecs, sst=1, vst=nv)
    pt, pp = tokN.shape[0] // N, poolN.shape[0] // N
    for n in range(N):
        sub = _scene(q, n, V)
        assert torch.equal(tokN[n * pt:(n + 1) * pt], _tokens(hip, sub, 1, V, S, D, W)), n
        assert torch.equal(poolN[n * pp:(n + 1) * pp], _fused(hip, ga, sub, 1, V, S, D, W, v0)), n
        row = q["steps"][n:n + 1].contiguous()
        assert torch.equal(tokT[n * pt:(n + 1) * pt], _tokens(hip, sub, 1, V, S, D, W, steps=row)), n
        assert torch.equal(poolT[n * pp:(n + 1) * pp], _fused(hip, ga, sub, 1, V, S, D, W, vecs[n].contiguous(), steps=row)), n
    assert not torch.equal(poolN[:pp], poolN[pp:]) and not torch.equal(tokN[:pt], tokN[pt:])          # the scenes really differ
    assert not torch.equal(poolT[pp:], poolN[pp:])                                                    # and so do scene 1's step rows
    # a view-parallel shard of scene 0
    sub = _scene(q, 0, V)
    q0, Vq = 2, 3
    tok1, pool1 = _tokens(hip, sub, 1, V, S, D, W), _fused(hip, ga, sub, 1, V, S, D, W, v0)
    rt, rp = S * S * D * W, S * S * D
    assert torch.equal(_tokens(hip, sub, 1, V, S, D, W, q0=q0, Vq=Vq), tok1[q0 * rt:(q0 + Vq) * rt])
    assert torch.equal(_fused(hip, ga, sub, 1, V, S, D, W, v0, q0=q0, Vq=Vq), pool1[q0 * rp:(q0 + Vq) * rp])
    # window = 0 through the new entry point is the existing kernel
    ref = hip.planes_like(V * S * S * D, 256, "cuda").zero_()
    stream, _ = ga.packed_fused(torch.device("cuda"))
    hip.check(hip.lib().mvd_gridattn_fused_scenes_t(hip.ptr(sub["x"]), hip.ptr(sub["dn"]), hip.ptr(sub["steps"]), hip.ptr(sub["it"]),
                                                    hip.ptr(sub["lin"]), hip.ptr(sub["feat"]), hip.ptr(sub["in_feat"]), hip.ptr(sub["cams"]),
                                                    hip.ptr(sub["in_cam"]), hip.ptr(stream), hip.ptr(v0), hip.ptr(ref), 1, V, 0, V, S, D, 2.0, 0.5,
                                                    4, 0, 0, hip.stream()))
    torch.cuda.synchronize()
    assert torch.equal(_fused(hip, ga, sub, 1, V, S, D, 0, v0), ref)


@pytest.mark.parametrize("V,top_k", [(8, 4), (3, 4)])
def test_windowed_tokens_backward_scatters_into_the_window_views(hip, V, top_k):
    """mvd_gridattn_tokens_backward_window: the windowed scatter into the reference views == the all-views scatter of the same gradient rows
    placed at the views the rule names (rows of other views zero; W <= V), and two scenes == two single-scene launches -- bit for bit
    (64-bit fixed-point accumulation is order independent); the input-view block, summed in fp32 over a point's rows first, to rounding."""
    from mvdfusion_amd.view_attn_efficient2 import window_view_table
    S, D, N = 16, 2, 2
    W = 2 * (top_k // 2) + 1
    q = _geo(N, V, S, D, [999, 10], seed=7)
    npts = N * V * S * S * D
    dtok = torch.randn(npts * W, 512, generator=torch.Generator().manual_seed(9)).cuda()
    scale = 2.0 ** 30
    L = hip.lib()

    def bwd(qq, d, n_sc, window, sst=0, steps=None):
        acc = torch.zeros(n_sc * V, S, S, 256, dtype=torch.int64, device="cuda")
        acc_in = torch.zeros(n_sc, S, S, 256, dtype=torch.int64, device="cuda")
        st = qq["steps"] if steps is None else steps
        hip.check(L.mvd_gridattn_tokens_backward_window(hip.ptr(qq["x"]), hip.ptr(qq["dn"]), hip.ptr(st), hip.ptr(qq["it"]), hip.ptr(qq["lin"]),
                                                        hip.ptr(qq["cams"]), hip.ptr(qq["in_cam"]), hip.ptr(d), 512, hip.ptr(acc),
                                                        hip.ptr(acc_in), scale, n_sc, V, 0, V, S, D, 2.0, 0.5, sst, window, hip.stream()))
        torch.cuda.synchronize()
        return acc, acc_in

    accN, inN = bwd(q, dtok, N, W, sst=1)
    per = dtok.shape[0] // N
    table = window_view_table(V, top_k)                     # (W, V)
    for n in range(N):
        sub = _scene(q, n, V)
        d1 = dtok[n * per:(n + 1) * per].contiguous()
        a1, b1 = bwd(sub, d1, 1, W, steps=q["steps"][n:n + 1].contiguous())
        assert torch.equal(accN[n * V:(n + 1) * V], a1) and torch.equal(inN[n:n + 1], b1), n
        if W <= V:       # (distinct views per point: the same rows through the all-views kernel, other views' rows zero)
            dfull = torch.zeros(V, S * S * D, V, 512, device="cuda")
            dw = d1.view(V, S * S * D, W, 512)
            for b in range(V):
                dfull[b][:, table[:, b].cuda()] = dw[b]
            a0, b0 = bwd(sub, dfull.reshape(-1, 512).contiguous(), 1, 0, steps=q["steps"][n:n + 1].contiguous())
            assert torch.equal(a0, a1), n
            # the input-view block: the kernel adds a point's rows in fp32 (slot order) before ONE scatter, and the all-views launch adds them
            # in view order with zeros in between -- a reordered fp32 sum of W terms |g| < 6 (N(0, 1) draws), tap weight <= 1: at most
            # W * 2^-24 * 6 W per point, and fewer than 1024 points reach one texel (V * D * 4 = 64 taps per texel on average)
            assert int((b0 - b1).abs().max()) <= 1024 * 6 * W * W * 2.0 ** -24 * scale, n
    assert not torch.equal(accN[:V], accN[V:])
