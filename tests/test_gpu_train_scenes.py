"""Batched multi-scene training step with a timestep per scene, on the GPU: the per-scene kernels against their single-scene launches
(bitwise), and ViewFusion.gradients_scenes / p_losses_scenes / forward(list) against the mean of N single-scene steps -- the N sequential
steps a training loop with scene_batch_size == 1 would take are the oracle.  Every scene gets its own cameras, images, draws and timestep."""
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

V4, S, D = 4, 32, 3


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


def _seed_draws(seed, t_fixed=None):
    """A noise_source of one scene: its own seeded draws (single-scene order), optionally a forced timestep."""
    def draws(V_, D_, S_):
        g = torch.Generator().manual_seed(seed)
        t = torch.randint(0, 1000, (V_,), generator=g)
        t = torch.zeros_like(t) + (t[0] if t_fixed is None else t_fixed)
        return dict(t=t, noise=torch.randn(V_, 5, S_, S_, generator=g), depth_noise=torch.randn(V_, D_, S_, S_, generator=g),
                    drop_rand=torch.rand(V_, generator=g))
    return draws


def _chain(sources):
    """One noise_source for an N-scene step: scene n's source on the n-th call (the per-scene call order of p_losses_scenes)."""
    it = iter(sources)
    return lambda V_, D_, S_: next(it)(V_, D_, S_)


def _scene_batches(m, batch, tc, N):
    """N scenes with their own cameras and images: prepared once (VAE encode) per scene, handed over as `_prepared` dicts."""
    out = []
    for n in range(N):
        g = torch.Generator().manual_seed(500 + n)
        b = dict(batch)
        b["images"] = torch.rand(batch["images"].shape, generator=g).to(batch["images"].device)
        b["T"] = batch["T"] + 0.03 * n * torch.randn(batch["T"].shape, generator=g)
        b["R"] = batch["R"]
        out.append({"_prepared": m.prepare_batch(b, tc)})
    return out


def _setup(mc=32, V=4, **kw):
    from test_gpu_vae import _training_setup
    gd = load_golden("train_grads_mc32_v4_d3" if mc == 32 else "train_grads_mc320_v8_d3")
    m, batch, tc, _ = _training_setup(gd, mc=mc, V=V, **kw)
    return m, batch, tc


def _compare(gN, refs, N, label):
    """Every gradient of the N-scene step against the mean of the single-scene ones: L2 norm and a seeded projection within
    1e-4 |g| + 2e-8 sqrt(n) (the golden tolerance of test_gpu_vae.py)."""
    bad, worst, names = [], 0.0, sorted(refs[0])
    for i, n in enumerate(names):
        if refs[0][n] is None:
            assert gN.get(n) is None, n
            continue
        ref = sum(r[n].double() for r in refs) / N
        got = gN[n].detach().double()
        gq, rq = got.flatten().cpu(), ref.flatten().cpu()
        pr = torch.randn(gq.numel(), generator=torch.Generator().manual_seed(1000 + i)).double()
        nr = float(rq.norm())
        e_n, e_p = abs(float(gq.norm()) - nr), abs(float((gq * pr).sum()) - float((rq * pr).sum()))
        tol = 1e-4 * nr + 2e-8 * gq.numel() ** 0.5
        if e_n > tol or e_p > tol:
            bad.append((n, nr, e_n, e_p))
        if nr > 1e-6:
            worst = max(worst, e_n / nr, e_p / nr, float((gq - rq).norm()) / nr)
    print(f"{label}: {len(names)} gradients vs the mean of {N} single-scene steps, worst relative deviation {worst:.2e}")
    return bad, len(names)


# ----------------------------------------------------------------------------------------------------------- op level
def _geo(N, V, S_, D_, rows, seed=3):
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd import hip as H
    from mvdfusion_amd.cameras import pack_cameras
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N * V, 5, S_, S_, generator=g) * 0.5).cuda()
    dn = torch.randn(1, N * V, D_, S_, S_, generator=g).cuda()
    cams = torch.cat([pack_cameras(syn.make_inputs(V, S_, seed=seed + n)["batch_cameras"]) for n in range(N)]).cuda()
    in_cam = torch.cat([pack_cameras(syn.make_inputs(V, S_, seed=seed + n)["input_cameras"]) for n in range(N)]).cuda()
    steps = torch.tensor(rows, dtype=torch.float32).cuda()
    feat = torch.randn(N * V, S_, S_, 256, generator=g).cuda()
    in_feat = torch.randn(N, S_, S_, 256, generator=g).cuda()
    half = 1.0 / S_
    lin = torch.linspace(1.0 - half, -1.0 + half, S_).cuda()
    return dict(x=x, dn=dn, cams=cams, in_cam=in_cam, steps=steps, feat=feat, in_feat=in_feat, lin=lin,
                it=torch.zeros(1, dtype=torch.int32).cuda())


def _rows(ts):
    from mvdfusion_amd.scheduler import make_tables
    tab = make_tables()
    out = []
    for t in ts:
        sac = float(tab["sqrt_alphas_cumprod"][t])
        out.append([float(t), sac, float(tab["sqrt_one_minus_alphas_cumprod"][t]) / sac / 10.0, 1.0, 1.0, 0.0, 0.0, 0.0])
    return out


def _tokens(hip, q, N, V, S_, D_, sst, steps=None, scenes_api=False):
    T = N * V * S_ * S_ * D_ * V
    tok = hip.planes_like(T, hip.TOKEN_LD, q["x"].device).zero_()
    st = q["steps"] if steps is None else steps
    args = (hip.ptr(q["x"]), hip.ptr(q["dn"]), hip.ptr(st), hip.ptr(q["it"]), hip.ptr(q["lin"]), hip.ptr(q["feat"]), hip.ptr(q["in_feat"]),
            hip.ptr(q["cams"]), hip.ptr(q["in_cam"]), hip.ptr(tok), N, V, 0, V, S_, D_, 2.0, 0.5)
    if scenes_api:
        hip.check(hip.lib().mvd_gridattn_tokens_scenes(*args, hip.stream()))
    else:
        hip.check(hip.lib().mvd_gridattn_tokens_scenes_t(*args, sst, hip.stream()))
    torch.cuda.synchronize()
    return tok


def test_tokens_t_kernel_matches_scenes_kernel_and_single_scene_rows(hip):
    N, V, S_, D_ = 3, 4, 16, 2
    q = _geo(N, V, S_, D_, _rows([999, 10, 500]))
    assert torch.equal(_tokens(hip, q, N, V, S_, D_, 0), _tokens(hip, q, N, V, S_, D_, 0, scenes_api=True))
    tok = _tokens(hip, q, N, V, S_, D_, 1)
    per = tok.shape[0] // N
    for n in range(N):
        sub = {k: v for k, v in q.items()}
        sub.update(x=q["x"][n * V:(n + 1) * V].contiguous(), cams=q["cams"][n * V:(n + 1) * V].contiguous(),
                   in_cam=q["in_cam"][n:n + 1].contiguous(), feat=q["feat"][n * V:(n + 1) * V].contiguous(),
                   in_feat=q["in_feat"][n:n + 1].contiguous(), dn=q["dn"][:, n * V:(n + 1) * V].contiguous())
        one = _tokens(hip, sub, 1, V, S_, D_, 0, steps=q["steps"][n:n + 1].contiguous())
        assert torch.equal(tok[n * per:(n + 1) * per], one), n
    assert not torch.equal(tok[:per], tok[per:2 * per])


def test_tokens_backward_scenes_matches_single_scene_launches(hip):
    N, V, S_, D_ = 3, 4, 16, 2
    q = _geo(N, V, S_, D_, _rows([999, 10, 500]), seed=7)
    T = N * V * S_ * S_ * D_ * V
    dtok = torch.randn(T, 512, generator=torch.Generator().manual_seed(9)).cuda()
    scale = 2.0 ** 30
    L = hip.lib()
    acc = torch.zeros(N * V, S_, S_, 256, dtype=torch.int64, device="cuda")
    acc_in = torch.zeros(N, S_, S_, 256, dtype=torch.int64, device="cuda")
    hip.check(L.mvd_gridattn_tokens_backward_scenes(hip.ptr(q["x"]), hip.ptr(q["dn"]), hip.ptr(q["steps"]), hip.ptr(q["it"]), hip.ptr(q["lin"]),
                                                    hip.ptr(q["cams"]), hip.ptr(q["in_cam"]), hip.ptr(dtok), 512, hip.ptr(acc), hip.ptr(acc_in),
                                                    scale, N, V, 0, V, S_, D_, 2.0, 0.5, 1, hip.stream()))
    per = T // N
    for n in range(N):
        a1 = torch.zeros(V, S_, S_, 256, dtype=torch.int64, device="cuda")
        b1 = torch.zeros(1, S_, S_, 256, dtype=torch.int64, device="cuda")
        x1, dn1 = q["x"][n * V:(n + 1) * V].contiguous(), q["dn"][:, n * V:(n + 1) * V].contiguous()
        c1, i1, st1 = q["cams"][n * V:(n + 1) * V].contiguous(), q["in_cam"][n:n + 1].contiguous(), q["steps"][n:n + 1].contiguous()
        d1 = dtok[n * per:(n + 1) * per].contiguous()
        hip.check(L.mvd_gridattn_tokens_backward(hip.ptr(x1), hip.ptr(dn1), hip.ptr(st1), hip.ptr(q["it"]), hip.ptr(q["lin"]), hip.ptr(c1),
                                                 hip.ptr(i1), hip.ptr(d1), 512, hip.ptr(a1), hip.ptr(b1), scale, V, 0, V, S_, D_, 2.0, 0.5,
                                                 hip.stream()))
        torch.cuda.synchronize()
        assert torch.equal(acc[n * V:(n + 1) * V], a1), n
        assert torch.equal(acc_in[n:n + 1], b1), n


def _fused(hip, m, q, N, V, S_, D_, vecs, sst, vst, steps=None, scenes_api=False):
    ga = m.view_attn
    stream, _ = ga.packed_fused(torch.device("cuda"))
    nseq = N * V * S_ * S_ * D_
    pool = hip.planes_like(nseq, 256, q["x"].device).zero_()
    st = q["steps"] if steps is None else steps
    args = (hip.ptr(q["x"]), hip.ptr(q["dn"]), hip.ptr(st), hip.ptr(q["it"]), hip.ptr(q["lin"]), hip.ptr(q["feat"]), hip.ptr(q["in_feat"]),
            hip.ptr(q["cams"]), hip.ptr(q["in_cam"]), hip.ptr(stream), hip.ptr(vecs), hip.ptr(pool), N, V, 0, V, S_, D_, 2.0, 0.5, 4)
    if scenes_api:
        hip.check(hip.lib().mvd_gridattn_fused_scenes(*args, hip.stream()))
    else:
        hip.check(hip.lib().mvd_gridattn_fused_scenes_t(*args, sst, vst, hip.stream()))
    torch.cuda.synchronize()
    return pool


def test_fused_t_kernel_matches_scenes_kernel_and_single_scene_rows(hip):
    from conftest import build_model
    m = build_model(32, D=2)
    N, V, S_, D_ = 3, 4, 16, 2
    q = _geo(N, V, S_, D_, _rows([999, 10, 500]), seed=11)
    _, vecs1 = m.view_attn.packed_fused(torch.device("cuda"))
    nv = vecs1.numel()
    vecs = vecs1.view(1, nv).repeat(N, 1)
    g = torch.Generator().manual_seed(13)
    for bi in range(3):                                   # a distinct adaLN modulation per scene
        vecs[:, bi * 3328:bi * 3328 + 1536] = (0.1 * torch.randn(N, 1536, generator=g)).cuda()
    v0 = vecs[0].contiguous()
    assert torch.equal(_fused(hip, m, q, N, V, S_, D_, v0, 0, 0), _fused(hip, m, q, N, V, S_, D_, v0, 0, 0, scenes_api=True))
    pool = _fused(hip, m, q, N, V, S_, D_, vecs, 1, nv)
    per = pool.shape[0] // N
    for n in range(N):
        sub = dict(q)
        sub.update(x=q["x"][n * V:(n + 1) * V].contiguous(), cams=q["cams"][n * V:(n + 1) * V].contiguous(),
                   in_cam=q["in_cam"][n:n + 1].contiguous(), feat=q["feat"][n * V:(n + 1) * V].contiguous(),
                   in_feat=q["in_feat"][n:n + 1].contiguous(), dn=q["dn"][:, n * V:(n + 1) * V].contiguous())
        one = _fused(hip, m, sub, 1, V, S_, D_, vecs[n].contiguous(), 0, 0, steps=q["steps"][n:n + 1].contiguous())
        assert torch.equal(pool[n * per:(n + 1) * per], one), n
    assert not torch.equal(pool[:per], pool[per:2 * per])


def test_layernorm_groups_forward_and_backward(hip):
    from mvdfusion_amd import backward as bw
    R, rows_g, C = 3, 200, 256
    g = torch.Generator().manual_seed(5)
    x = torch.randn(R * rows_g, C, generator=g).cuda() * 2 + 0.3
    mod = torch.randn(R, 6 * C, generator=g).cuda() * 0.2
    sc, sh = mod[:, C:2 * C], mod[:, :C]
    y = hip.planes_like(R * rows_g, C, x.device)
    yf = torch.empty(R * rows_g, C, device="cuda")
    hip.layernorm_groups(x, y, sc, sh, R * rows_g, C, rows_g, eps=1e-6, w_plus_one=True, y_f32=yf)
    dy = torch.randn(R * rows_g, C, generator=g).cuda()
    w = (1.0 + sc).contiguous()
    dx, dw, db = bw.layernorm_backward_groups(x, dy, w, 1e-6, R)
    torch.cuda.synchronize()
    for n in range(R):
        sl = slice(n * rows_g, (n + 1) * rows_g)
        y1 = hip.planes_like(rows_g, C, x.device)
        yf1 = torch.empty(rows_g, C, device="cuda")
        hip.layernorm(x[sl].contiguous(), y1, sc[n].contiguous(), sh[n].contiguous(), rows_g, C, eps=1e-6, w_plus_one=True, y_f32=yf1)
        dx1, dw1, db1 = bw.layernorm_backward(x[sl].contiguous(), dy[sl].contiguous(), w[n].contiguous(), 1e-6)
        torch.cuda.synchronize()
        assert torch.equal(yf[sl], yf1) and torch.equal(y[sl], y1), n
        assert torch.equal(dx[sl], dx1), n
        assert torch.allclose(dw[n], dw1, rtol=1e-6, atol=1e-6) and torch.allclose(db[n], db1, rtol=1e-6, atol=1e-6), n


def test_timestep_embedding_scenes_rows(hip):
    from mvdfusion_amd.viewfusion_zero_depth_rgb import _sinusoid_freqs
    steps = torch.tensor(_rows([999, 10, 500]), dtype=torch.float32).cuda()
    it = torch.zeros(1, dtype=torch.int32, device="cuda")
    f = _sinusoid_freqs(256).cuda()
    out = torch.empty(3, 256, device="cuda")
    hip.check(hip.lib().mvd_timestep_embedding_scenes(hip.ptr(steps), hip.ptr(it), hip.ptr(f), hip.ptr(out), 256, 3, 1, hip.stream()))
    for n in range(3):
        one = torch.empty(1, 256, device="cuda")
        hip.check(hip.lib().mvd_timestep_embedding(hip.ptr(steps[n:n + 1].contiguous()), hip.ptr(it), hip.ptr(f), hip.ptr(one), 256,
                                                   hip.stream()))
        torch.cuda.synchronize()
        assert torch.equal(out[n], one[0]), n


# ----------------------------------------------------------------------------------------------------------- model level
@pytest.mark.parametrize("N", [2, 3])
def test_gradients_scenes_equal_mean_of_single_scene_steps(N):
    m, batch, tc = _setup(32, V4)
    scenes = _scene_batches(m, batch, tc, N)
    seeds = [41 + 17 * n for n in range(N)]
    ts = [int(_seed_draws(s)(V4, D, S)["t"][0]) for s in seeds]
    assert len(set(ts)) == N, ts                              # distinct timesteps: a shared-t implementation cannot pass
    refs, losses = [], []
    for sc, sd in zip(scenes, seeds):
        l1, g1 = m.gradients(sc, tc, noise_source=_seed_draws(sd))
        losses.append(float(l1))
        refs.append({k: (None if v is None else v.clone()) for k, v in g1.items()})
    lossN, gN = m.gradients_scenes(scenes, tc, noise_source=_chain([_seed_draws(s) for s in seeds]))
    ref_loss = sum(losses) / N
    print(f"N={N} timesteps {ts}: loss {float(lossN):.7f} vs mean of single-scene losses {ref_loss:.7f}")
    assert abs(float(lossN) - ref_loss) <= 1e-6 * abs(ref_loss)
    assert set(k for k, v in gN.items() if v is not None) == set(k for k, v in refs[0].items() if v is not None)
    bad, count = _compare(gN, refs, N, f"mc32 V=4 D=3 N={N}")
    assert count == 994
    assert not bad, bad[:10]


def test_scenes_step_is_bit_reproducible_and_p_losses_scenes_agrees():
    m, batch, tc = _setup(32, V4)
    scenes = _scene_batches(m, batch, tc, 2)
    src = lambda: _chain([_seed_draws(7), _seed_draws(8)])
    l1, g1 = m.gradients_scenes(scenes, tc, noise_source=src())
    g1 = {k: v.clone() for k, v in g1.items() if v is not None}
    l2, g2 = m.gradients_scenes(scenes, tc, noise_source=src())
    assert torch.equal(l1, l2)
    diff = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert not diff, diff[:10]
    fwd = m.p_losses_scenes(scenes, tc, noise_source=src())
    assert abs(float(fwd) - float(l1)) <= 1e-6 * abs(float(l1))


def test_drop_in_list_forward_backward_adamw_step():
    """loss = model([b0, b1], tc); loss.backward(); opt.step() == accumulating loss_i / N over single-scene steps, then one step."""
    m, batch, tc = _setup(32, V4)
    for p in list(m.vae.parameters()) + list(m.clip_image_encoder.parameters()):
        p.requires_grad_(False)
    scenes = _scene_batches(m, batch, tc, 2)
    seeds = [3, 4]
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    opt = m.configure_optimizers(lr=2e-4)
    m._noise_source = _chain([_seed_draws(s) for s in seeds])
    loss = m(scenes, tc)
    opt.zero_grad()
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    opt.step()
    after = {n: p.detach().clone() for n, p in m.named_parameters()}
    m.load_state_dict(sd0)                                   # the same start, then N sequential single-scene steps accumulating loss_i / N
    opt2 = m.configure_optimizers(lr=2e-4)
    opt2.zero_grad()
    total = 0.0
    for sc, sd in zip(scenes, seeds):
        m._noise_source = _seed_draws(sd)
        li = m(sc, tc)
        (li / 2).backward()
        total += float(li.detach()) / 2
    seq = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    assert set(seq) == set(grads) and len(grads) >= 300
    for n, g in grads.items():                    # .grad after loss.backward(): the accumulated sum within the golden tolerance
        assert float((g - seq[n]).double().norm()) <= 1e-4 * float(seq[n].double().norm()) + 2e-8 * g.numel() ** 0.5, n
    opt2.step()
    m._noise_source = None
    assert abs(float(loss.detach()) - total) <= 1e-6 * abs(total)
    # AdamW's first step moves every element by about lr * sign(g): a gradient component near zero turns a round-off difference into a
    # visible fraction of lr, so the parameters are compared against the step size
    worst = 0.0
    for n, p in m.named_parameters():
        d = float((after[n] - p.detach()).abs().max()) if p.numel() else 0.0
        worst = max(worst, d)
        assert d <= 0.1 * 2e-4, n
    print(f"drop-in: worst parameter difference after one AdamW step {worst:.2e} (lr 2e-4)")
    with pytest.raises(ValueError):
        m([], tc)


def test_full_width_config4_two_scenes_equal_mean_and_reference_anchor():
    """configs[4] shape (mc320, V=8, D=3, finetune_unet) at N=2: the mean equivalence, and with both scenes set to the reference fixture
    every gradient matches train_grads_mc320_v8_d3."""
    from test_gpu_vae import _training_setup
    gd = load_golden("train_grads_mc320_v8_d3")
    m, batch, tc, draws = _training_setup(gd, mc=320, V=8, finetune_unet=True)
    scenes = _scene_batches(m, batch, tc, 2)
    seeds = [21, 22]
    refs, losses = [], []
    for sc, sd in zip(scenes, seeds):
        l1, g1 = m.gradients(sc, tc, noise_source=_seed_draws(sd), only_trainable=True)
        losses.append(float(l1))
        refs.append({k: (None if v is None else v.clone()) for k, v in g1.items()})
        del g1
    lossN, gN = m.gradients_scenes(scenes, tc, noise_source=_chain([_seed_draws(s) for s in seeds]), only_trainable=True)
    assert abs(float(lossN) - sum(losses) / 2) <= 1e-6 * abs(sum(losses) / 2)
    bad, _ = _compare(gN, refs, 2, "configs[4] N=2")
    assert not bad, bad[:10]
    del refs, gN
    # reference anchor: both scenes = the fixture batch and draws
    fixture = {"_prepared": m.prepare_batch(batch, tc)}
    loss, grads = m.gradients_scenes([fixture, fixture], tc, noise_source=_chain([draws, draws]), only_trainable=True)
    assert abs(float(loss) - float(gd["loss"])) / float(gd["loss"]) < 1e-4
    names = [str(n) for n in gd["grad_names"]]
    norms, projs = gd["grad_norms"].double(), gd["grad_projs"].double()
    bad = []
    for i, n in enumerate(names):
        gq = grads[n].detach().double().cpu().flatten()
        r = torch.randn(gq.numel(), generator=torch.Generator().manual_seed(1000 + i)).double()
        nr, pr = float(norms[i]), float(projs[i])
        tol = 1e-4 * nr + 2e-8 * gq.numel() ** 0.5
        if abs(float(gq.norm()) - nr) > tol or abs(float((gq * r).sum()) - pr) > tol:
            bad.append(n)
    assert not bad, bad[:10]
