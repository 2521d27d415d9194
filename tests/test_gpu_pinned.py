"""Pinned views in the DDIM loop (mvd_pin_views; StepEngine.set_pin; DDIMSampler overwrite_x_noisy / known_latents / sample_rig).

  kernel   : mvd_pin_views against the torch expression, row by row, both modes, float4 and scalar form, argument checks
  flag     : DDIMSampler(overwrite_x_noisy=True).sample against three iterations of the REAL reference's loop
             (tests/golden/sample_overwrite_mc32_v3.npz, tools/make_golden_pinned.py)
  general  : sample(known_latents=...) against an emulation that never uses the pin path: the unsharded engine (all rows queries, eager)
             with the test writing the re-noised rows itself before every step
  plumbing : replay == eager, no pin state left in cached engines, the free rows' noise, scenes, window, sample_rig, refusals
"""
import pytest
import torch

from conftest import build_model, load_golden, model_config, rel_err, rmse

pytestmark = pytest.mark.gpu

S, D, CFG = 32, 1, 2.5


def _syn():
    from mvdfusion_amd import synthetic
    return synthetic


def _cond(inp):
    return (inp["batch_cameras"], inp["input_latents"], inp["input_cameras"], inp["clip_v_embed"])


def _table(m):
    from mvdfusion_amd.engine import ddim_step_table
    st, dd = m.ddim.tables()
    return ddim_step_table(st, dd, [49 - i for i in range(50)])


def _known(K, seed):
    """Clean latents at the scale of make_inputs' input latents (VAE latents * 0.18215 have std ~0.7)."""
    return (torch.randn(K, 5, S, S, generator=torch.Generator().manual_seed(seed)) * 0.7).cuda()


# ------------------------------------------------------------------------------------------------ kernel
def _pin_case(Sk, seed=0):
    g = torch.Generator().manual_seed(seed)
    groups, gv, K = 2, 3, 2
    x, x0 = torch.randn(groups * gv, 5, Sk, Sk, generator=g).cuda(), torch.randn(groups * gv, 5, Sk, Sk, generator=g).cuda()
    known = torch.randn(groups * K, 5, Sk, Sk, generator=g).cuda()
    noise = torch.randn(3, groups * K, 5, Sk, Sk, generator=g).cuda()
    steps = (torch.rand(3, 8, generator=g) + 0.1).cuda()          # distinct rows: a wrong table row shows
    it = torch.tensor([1], dtype=torch.int32).cuda()              # ... and iter = 1 tells row 1 from row 0 of table and noise
    return groups, gv, K, x, x0, known, noise, steps, it


def _pin(hip, x, x0, known, noise, steps, it, groups, gv, K, Sk, mode):
    stride = 0 if noise is None else noise[0].numel()
    return hip.lib().mvd_pin_views(hip.ptr(x), hip.ptr(x0), hip.ptr(known), hip.ptr(noise), stride, hip.ptr(steps), hip.ptr(it), groups, gv, K,
                                   Sk, mode, hip.stream())


@pytest.mark.parametrize("Sk", [8, 3])          # S*S % 4 == 0: float4 rows; S = 3: 45 floats per row, the scalar form
def test_pin_views_kernel(Sk):
    from mvdfusion_amd import hip
    groups, gv, K, x, x0, known, noise, steps, it = _pin_case(Sk)
    rows = [g * gv + k for g in range(groups) for k in range(K)]
    free = [r for r in range(groups * gv) if r not in rows]
    # mode 0: the clean rows, bit for bit; x0 and the noise pointer are not needed
    x_a = x.clone()
    hip.check(_pin(hip, x_a, None, known, None, None, None, groups, gv, K, Sk, 0))
    torch.cuda.synchronize()
    assert torch.equal(x_a[rows], known) and torch.equal(x_a[free], x[free])
    x_b, x0_b = x.clone(), x0.clone()
    hip.check(_pin(hip, x_b, x0_b, known, noise, steps, it, groups, gv, K, Sk, 0))
    torch.cuda.synchronize()
    assert torch.equal(x_b, x_a) and torch.equal(x0_b, x0)                 # x0 is written in mode 1 only
    # mode 1: sqrt(ab) known + sqrt(1 - ab) noise of table row / noise row *iter; x0 = known
    x_c, x0_c = x.clone(), x0.clone()
    hip.check(_pin(hip, x_c, x0_c, known, noise, steps, it, groups, gv, K, Sk, 1))
    torch.cuda.synchronize()
    sa, s1 = steps[1, 1], steps[1, 6]
    a, b = sa * known, s1 * noise[1]
    bound = 2.0 ** -23 * (a.abs() + b.abs())                                # fused vs separate rounding of the multiply-add
    err = (x_c[rows] - (a + b)).abs()
    print(f"pin_views S={Sk} mode 1: max err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(x0_c[rows], known)
    assert torch.equal(x_c[free], x[free]) and torch.equal(x0_c[free], x0[free])
    assert not torch.equal(x_c[rows], sa * known + s1 * noise[0])           # (the case tells the noise rows apart)


def test_pin_views_bad_arguments_return_an_error():
    from mvdfusion_amd import hip
    groups, gv, K, x, x0, known, noise, steps, it = _pin_case(8)
    x_in = x.clone()
    L = hip.lib()
    assert _pin(hip, x, x0, known, noise, steps, it, groups, gv, 0, 8, 1) != 0            # K = 0
    assert _pin(hip, x, x0, known, noise, steps, it, groups, gv, gv + 1, 8, 1) != 0       # K > group_views
    assert _pin(hip, None, x0, known, noise, steps, it, groups, gv, K, 8, 1) != 0         # null x
    assert _pin(hip, x, x0, None, noise, steps, it, groups, gv, K, 8, 0) != 0             # null known
    assert _pin(hip, x, x0, known, noise, steps, it, groups, gv, K, 8, 2) != 0            # no such mode
    assert _pin(hip, x, x0, known, None, steps, it, groups, gv, K, 8, 1) != 0             # mode 1 without noise
    assert _pin(hip, x, None, known, noise, steps, it, groups, gv, K, 8, 1) != 0          # mode 1 without x0
    assert _pin(hip, x, x0, known, noise, steps, None, groups, gv, K, 8, 1) != 0          # mode 1 without the counter
    assert _pin(hip, x, x0, known, noise, steps, it, 0, gv, K, 8, 1) != 0                 # no groups
    assert L.mvd_pin_views(hip.ptr(x), hip.ptr(x0), hip.ptr(known), hip.ptr(noise), 5, hip.ptr(steps), hip.ptr(it), groups, gv, K, 8, 1,
                           hip.stream()) != 0                                                # noise rows shorter than the pinned set
    off = x.view(-1)[1:1 + (groups * gv - 1) * 5 * 64].view(groups * gv - 1, 5, 8, 8)      # 4 bytes past a 16-byte boundary
    assert _pin(hip, off, x0, known, noise, steps, it, 1, gv, K, 8, 0) != 0               # float4 rows need 16-byte alignment
    assert b"mvd_pin_views" in L.mvd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, x_in)                                                             # nothing was launched


# ------------------------------------------------------------------------------------------------ the reference's flag
def _flag_sampler(m):
    from mvdfusion_amd.sampler import DDIMSampler
    return DDIMSampler(m, ddim_num_steps=50, ddim_discretize="uniform", ddim_eta=1.0, latent_size=S, z_dim=4, overwrite_x_noisy=True,
                       feed_prev_depth=m.ddim.feed_prev_depth)


@pytest.mark.parametrize("use_graph", [True, False])
def test_overwrite_x_noisy_vs_reference_golden(use_graph):
    """DDIMSampler(overwrite_x_noisy=True).sample (sampler.py:109-110,123-124): the first three iterations of the REAL reference's loop, row 0
    rewritten with the clean input latents inside the captured step; every row is a query row and is updated."""
    syn = _syn()
    gd = load_golden("sample_overwrite_mc32_v3")
    V, steps = 3, int(gd["xs"].shape[0])
    m = build_model(32)
    inp = syn.make_inputs(V, S, seed=9)
    dn, sn = torch.zeros(50, V, D, S, S), torch.zeros(50, V, 5, S, S)
    dn[:steps], sn[:steps] = gd["depth_noise"], gd["step_noise"]
    smp = _flag_sampler(m)
    smp.noise_source = lambda *a: (dn, sn)
    x, inter = smp.sample(*_cond(inp), unconditional_scale=CFG, depth=True, return_intermediates=True, verbose=False, x_T=gd["x_T"].cuda(),
                          num_steps=steps, use_graph=use_graph)
    for i, itm in enumerate(inter):
        print(f"overwrite_x_noisy graph={use_graph} step {i}: rmse xt {rmse(itm['xt'], gd['xs'][i]):.3e} x0 {rmse(itm['x0'], gd['x0s'][i]):.3e}")
    for i, itm in enumerate(inter):
        assert rmse(itm["xt"], gd["xs"][i]) < 2e-4 and rmse(itm["x0"], gd["x0s"][i]) < 2e-3, (i, rmse(itm["xt"], gd["xs"][i]))
    assert torch.equal(x, inter[-1]["xt"])                 # what the reference returns: row 0 is the update of the clean row
    if use_graph:
        # the flag matters: without it a FREE row leaves the fixture's trajectory at the first step (row 0 reaches it through GridAttn only)
        m.ddim.noise_source = lambda *a: (dn, sn)
        try:
            _, off = m.ddim.sample(*_cond(inp), unconditional_scale=CFG, depth=True, return_intermediates=True, verbose=False,
                                   x_T=gd["x_T"].cuda(), num_steps=1)
        finally:
            m.ddim.noise_source = None
        dev = max(rmse(off[0]["xt"][v], gd["xs"][0][v]) for v in range(1, V))
        print(f"flag off: free-row rmse to the fixture at step 0 = {dev:.3e}")
        assert dev > 1e-3, dev


def test_overwrite_x_noisy_scenes_equal_single_scene_runs():
    """sample_scenes of two scenes with the flag: row 0 of EACH scene becomes that scene's own input latents."""
    syn = _syn()
    m = build_model(32)
    V, steps = 3, 3
    inps = [syn.make_inputs(V, S, seed=s) for s in (4, 6)]
    assert not torch.equal(inps[0]["input_latents"], inps[1]["input_latents"])
    noises = [syn.step_noise(V, S, D, 50, seed=s) for s in (4, 6)]
    smp = _flag_sampler(m)
    calls = []

    def src(*a):
        calls.append(len(calls) % 2)
        return noises[calls[-1]]
    smp.noise_source = src
    x, inter = smp.sample_scenes([_cond(i) for i in inps], unconditional_scale=CFG, return_intermediates=True, verbose=False,
                                 x_T=torch.stack([i["x_T"] for i in inps]).cuda(), num_steps=steps)
    assert calls == [0, 1] and x.shape == (2, V, 5, S, S)
    for n, inp in enumerate(inps):
        smp.noise_source = lambda *a, n=n: noises[n]
        x1, inter1 = smp.sample(*_cond(inp), unconditional_scale=CFG, depth=True, return_intermediates=True, verbose=False,
                                x_T=inp["x_T"].cuda(), num_steps=steps)
        for i in range(steps):
            assert rmse(inter[i]["xt"][n], inter1[i]["xt"]) < 1e-4, (n, i, rmse(inter[i]["xt"][n], inter1[i]["xt"]))
        assert rmse(x[n], x1) < 1e-4          # (the bound of test_sample_scenes_trajectory_vs_golden_and_single_scene for this comparison)
    assert all(e.pin is None for e in m._engines.values())


def test_overwrite_x_noisy_with_feed_prev_depth():
    """The flag together with feed_prev_depth (two more graph variants: pin with and without the depth overwrite): replay == eager, and both
    equal the plain engine driven by hand with the test writing row 0 itself before every step."""
    from mvdfusion_amd.sampler import DDIMSampler
    syn = _syn()
    m = build_model(32)
    V, steps = 3, 3
    inp = syn.make_inputs(V, S, seed=12)
    dn, sn = syn.step_noise(V, S, D, 50, seed=12)
    smp = DDIMSampler(m, ddim_num_steps=50, ddim_eta=1.0, latent_size=S, z_dim=4, overwrite_x_noisy=True, feed_prev_depth=True)
    smp.noise_source = lambda *a: (dn, sn)
    kw = dict(unconditional_scale=CFG, depth=True, verbose=False, x_T=inp["x_T"].cuda(), num_steps=steps)
    xg, xe = smp.sample(*_cond(inp), use_graph=True, **kw), smp.sample(*_cond(inp), use_graph=False, **kw)
    eng = m.engine(V, S, D, True)
    eng.set_conditioning(*[t.cuda() if torch.is_tensor(t) else t for t in _cond(inp)])
    eng.set_schedule(_table(m), dn, sn)
    eng.x.copy_(inp["x_T"])
    try:
        for i in range(steps):
            eng.x[0] = inp["input_latents"][0].cuda()
            eng.depth_mode = 1 if i > 0 else 0
            eng.step(CFG, do_update=True, use_graph=False)
    finally:
        eng.depth_mode = 0
    assert torch.equal(xg, xe) and torch.equal(xe, eng.x)
    smp.feed_prev_depth = False
    assert not torch.equal(smp.sample(*_cond(inp), **kw), xg)


# ------------------------------------------------------------------------------------------------ known_latents
def _emulate(m, inp, known, kn, dn, sn, steps, V, K):
    """The pinned run without the pin path: the unsharded engine (q0 = 0: every row a query row and updated), eager, and before every step
    the test itself writes rows [0, K) = sqrt(ab_t) known + sqrt(1 - ab_t) noise with torch.  Returns x after each step."""
    table = _table(m)
    eng = m.engine(V, S, D, True)
    eng.set_conditioning(inp["batch_cameras"], inp["input_latents"].cuda(), inp["input_cameras"], inp["clip_v_embed"].cuda())
    eng.set_schedule(table, dn, sn)
    eng.x.copy_(inp["x_T"])
    eng.depth_mode = 0
    out = []
    for i in range(steps):
        eng.x[:K] = float(table[i, 1]) * known + float(table[i, 6]) * kn[i].cuda()
        eng.step(CFG, do_update=True, use_graph=False)
        torch.cuda.synchronize()
        out.append(eng.x.clone())
    return out


def _pinned_case(V, K, seed, steps=3):
    syn = _syn()
    inp = syn.make_inputs(V, S, seed=seed)
    dn, sn = syn.step_noise(V, S, D, 50, seed=seed)
    known = _known(K, 40 + seed)
    kn = torch.randn(steps, K, 5, S, S, generator=torch.Generator().manual_seed(70 + seed))
    return inp, dn, sn, known, kn


def _pinned_sample(m, inp, dn, sn, known, kn, steps, use_graph=True):
    m.ddim.noise_source = lambda *a: (dn, sn)
    try:
        return m.ddim.sample(*_cond(inp), unconditional_scale=CFG, depth=True, return_intermediates=True, verbose=False,
                             x_T=inp["x_T"].cuda(), num_steps=steps, use_graph=use_graph, known_latents=known, known_noise=kn)
    finally:
        m.ddim.noise_source = None


def test_pinned_sample_vs_independent_emulation():
    """V = 4, K = 2: the free rows of sample(known_latents=...) -- the engine of the query range [K, V) with the in-graph pin -- against the
    emulation on the unsharded engine.  Same math, other GEMM tiling (half the UNet batch): the shard-versus-full bound of
    test_view_shard_equivalence after one step, the project's three-iteration bound after three."""
    m = build_model(32)
    V, K, steps = 4, 2, 3
    inp, dn, sn, known, kn = _pinned_case(V, K, 2)
    x, inter = _pinned_sample(m, inp, dn, sn, known, kn, steps)
    emu = _emulate(m, inp, known, kn, dn, sn, steps, V, K)
    e1, e3 = rel_err(inter[0]["xt"][K:], emu[0][K:]), rmse(x[K:], emu[2][K:])
    print(f"pinned vs emulation V={V} K={K}: one step rel_err {e1:.3e} (bound 2e-5), three steps rmse {e3:.3e} (bound 2e-4)")
    assert e1 < 2e-5, e1
    assert e3 < 2e-4, e3
    assert torch.equal(x[:K], known)                                        # the pinned rows come back exactly
    table = _table(m)
    for i, itm in enumerate(inter):
        assert torch.equal(itm["x0"][:K], known)
        want = float(table[i, 1]) * known + float(table[i, 6]) * kn[i].cuda()
        assert float((itm["xt"][:K] - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max())      # the rows the step saw, at ITS timestep


def test_pinned_windowed_step_vs_emulation():
    """keep_top_k_views with pinned views: the window counts views in the whole rig, so a free row near the prefix still attends to it."""
    from mvdfusion_amd.viewfusion_zero_depth_rgb import ViewFusion
    syn = _syn()
    cfg = model_config(32)
    va = cfg["view_attn_config"]
    cfg["view_attn_config"] = dict(va, params=dict(va["params"], keep_top_k_views=True, top_k=4))
    with syn.skip_default_init():
        m = ViewFusion(**cfg)
    syn.fill_module_(m)
    m = m.cuda().eval()
    V, K = 8, 2
    inp, dn, sn, known, kn = _pinned_case(V, K, 5, steps=1)
    x, inter = _pinned_sample(m, inp, dn, sn, known, kn, 1, use_graph=False)      # (replay == eager is pinned at V = 4)
    emu = _emulate(m, inp, known, kn, dn, sn, 1, V, K)
    e1 = rel_err(inter[0]["xt"][K:], emu[0][K:])
    print(f"windowed pinned vs emulation V={V} top_k=4 K={K}: one step rel_err {e1:.3e} (bound 2e-5)")
    assert e1 < 2e-5, e1
    assert torch.equal(x[:K], known)


def test_pinned_replay_equals_eager_and_leaves_no_pin_behind():
    m = build_model(32)
    V, K, steps = 4, 2, 3
    inp, dn, sn, known, kn = _pinned_case(V, K, 3)

    def plain():
        m.ddim.noise_source = lambda *a: (dn, sn)
        try:
            return m.ddim.sample(*_cond(inp), unconditional_scale=CFG, depth=True, verbose=False, x_T=inp["x_T"].cuda(), num_steps=steps)
        finally:
            m.ddim.noise_source = None

    before = plain()
    xg, ig = _pinned_sample(m, inp, dn, sn, known, kn, steps, use_graph=True)
    xe, ie = _pinned_sample(m, inp, dn, sn, known, kn, steps, use_graph=False)
    xg2, _ = _pinned_sample(m, inp, dn, sn, known, kn, steps, use_graph=True)          # replay of the cached graph
    assert torch.equal(xg, xe) and torch.equal(xg, xg2)
    for a, b in zip(ig, ie):
        assert torch.equal(a["xt"], b["xt"]) and torch.equal(a["x0"], b["x0"])
    # the flag pins on the SAME cached engine a plain sample uses
    smp = _flag_sampler(m)
    smp.noise_source = lambda *a: (dn, sn)
    xf = smp.sample(*_cond(inp), unconditional_scale=CFG, depth=True, verbose=False, x_T=inp["x_T"].cuda(), num_steps=steps)
    assert not torch.equal(xf, before)
    assert all(e.pin is None and e.depth_mode == 0 for e in m._engines.values())
    assert torch.equal(plain(), before)                                     # no pin state leaked into the cached engines


def test_pinned_run_hands_the_free_rows_the_unpinned_noise():
    """x_T, depth noise and update noise keep their full-V shapes and order: the engine of a pinned run holds the tables of the unpinned run,
    from a noise_source (called once, with the whole rig's V) and from torch's generator (the pin noise is drawn last)."""
    syn = _syn()
    m = build_model(32)
    V, K = 4, 2
    inp, dn, sn, known, kn = _pinned_case(V, K, 6, steps=1)
    calls = []

    def src(*a):
        calls.append(a)
        return dn, sn
    plain_eng, pin_eng = m.engine(V, S, D, True), m.engine(V, S, D, True, q0=K, Vq=V - K)
    m.ddim.noise_source = src
    try:
        a = m.ddim.sample(*_cond(inp), unconditional_scale=CFG, depth=True, verbose=False, x_T=inp["x_T"].cuda(), num_steps=1)
        b = m.ddim.sample(*_cond(inp), unconditional_scale=CFG, depth=True, verbose=False, x_T=inp["x_T"].cuda(), num_steps=1,
                          known_latents=None)
        m.ddim.sample(*_cond(inp), unconditional_scale=CFG, depth=True, verbose=False, x_T=inp["x_T"].cuda(), num_steps=1,
                      known_latents=known, known_noise=kn)
    finally:
        m.ddim.noise_source = None
    assert torch.equal(a, b)                                                # known_latents=None is the plain call
    assert calls == [(V, S, D, 50)] * 3
    assert torch.equal(pin_eng.depth_noise, plain_eng.depth_noise) and torch.equal(pin_eng.ddim_noise, plain_eng.ddim_noise)
    assert pin_eng.depth_noise.shape == (50, V, D, S, S) and pin_eng.ddim_noise.shape == (50, V, 5, S, S)
    # torch's device generator: the same seed gives the free rows the same draws; the pin noise comes after them
    torch.manual_seed(17)
    m.ddim.sample(*_cond(inp), unconditional_scale=CFG, depth=True, verbose=False, num_steps=1)
    dn_a, sn_a = plain_eng.depth_noise.clone(), plain_eng.ddim_noise.clone()
    torch.manual_seed(17)
    xT = torch.randn(V, 5, S, S, device="cuda")
    torch.manual_seed(17)
    x, inter = m.ddim.sample(*_cond(inp), unconditional_scale=CFG, depth=True, verbose=False, num_steps=1, known_latents=known,
                             return_intermediates=True)
    assert torch.equal(pin_eng.depth_noise, dn_a) and torch.equal(pin_eng.ddim_noise, sn_a)
    torch.manual_seed(17)
    for shape in ((V, 5, S, S), (50, V, D, S, S), (50, V, 5, S, S)):
        torch.randn(*shape, device="cuda")
    assert torch.equal(pin_eng.pin_noise, torch.randn(50, K, 5, S, S, device="cuda"))
    # ... and the free rows start from rows [K, V) of the same x_T: one eager step of the emulation from it agrees
    emu = _emulate(m, dict(inp, x_T=xT), known, pin_eng.pin_noise[:1].cpu(), dn_a, sn_a, 1, V, K)
    assert rel_err(inter[0]["xt"][K:], emu[0][K:]) < 2e-5


# ------------------------------------------------------------------------------------------------ rigs larger than one step
def test_sample_rig_equals_the_sample_calls_composed_by_hand():
    from mvdfusion_amd.cameras import get_camera_slice
    syn = _syn()
    m = build_model(32)
    M, V, K, steps = 7, 4, 1, 2
    inp = syn.make_inputs(M, S, seed=8)
    noises = {}

    def src(Vc, Sc, Dc, total):          # the c-th call (one per chunk) draws for that chunk's view count
        c = src.n
        src.n += 1
        if (c, Vc) not in noises:
            noises[(c, Vc)] = syn.step_noise(Vc, Sc, Dc, total, seed=100 + c)
        return noises[(c, Vc)]
    kn = {1: torch.randn(steps, K, 5, S, S, generator=torch.Generator().manual_seed(9))}
    xT = inp["x_T"].cuda()
    m.ddim.noise_source = src
    try:
        src.n = 0
        out = m.ddim.sample_rig(*_cond(inp), unconditional_scale=CFG, chunk_views=V, anchors_per_chunk=K, verbose=False, x_T=xT,
                                known_noise=kn, num_steps=steps)
        assert src.n == 2 and sorted(noises) == [(0, 4), (1, 4)]
        src.n = 0
        kw = dict(unconditional_scale=CFG, depth=True, verbose=False, num_steps=steps)
        first = m.ddim.sample(get_camera_slice(inp["batch_cameras"], [0, 1, 2, 3]), inp["input_latents"], inp["input_cameras"],
                              inp["clip_v_embed"][:4], x_T=xT[:4], **kw)
        idx = [3, 4, 5, 6]
        second = m.ddim.sample(get_camera_slice(inp["batch_cameras"], idx), inp["input_latents"], inp["input_cameras"],
                               inp["clip_v_embed"][idx], x_T=xT[idx], known_latents=first[3:4], known_noise=kn[1], **kw)
    finally:
        m.ddim.noise_source = None
    assert out.shape == (M, 5, S, S)
    assert torch.equal(out[:4], first) and torch.equal(out[4:], second[1:])         # rig order; the anchor (view 3) as first generated
    assert torch.equal(second[0], first[3])
    assert all(e.pin is None for e in m._engines.values())


# ------------------------------------------------------------------------------------------------ refusals
def test_pinned_refusals():
    from mvdfusion_amd.parallel import sample_view_parallel
    syn = _syn()
    m = build_model(32)
    V = 3
    inp = syn.make_inputs(V, S, seed=1)
    known = _known(1, 1)
    kw = dict(unconditional_scale=CFG, depth=True, verbose=False, num_steps=1)
    with pytest.raises(ValueError, match="single-scene"):
        m.ddim.sample_scenes([_cond(inp), _cond(inp)], unconditional_scale=CFG, verbose=False, num_steps=1, known_latents=known)
    dn, sn = syn.step_noise(V, S, D, 50, seed=1)
    with pytest.raises(ValueError, match="known_latents"):
        sample_view_parallel(m, *_cond(inp), CFG, inp["x_T"].cuda(), dn, sn, num_steps=1, known_latents=known)
    with pytest.raises(ValueError, match="overwrite_x_noisy"):
        _flag_sampler(m).sample(*_cond(inp), known_latents=known, **kw)
    with pytest.raises(ValueError, match="K = 3"):
        m.ddim.sample(*_cond(inp), known_latents=_known(V, 2), **kw)                 # K >= V: nothing left to generate
    with pytest.raises(ValueError, match="known_latents"):
        m.ddim.sample(*_cond(inp), known_latents=known[:, :4], **kw)                 # 4 channels
    with pytest.raises(ValueError, match="known_latents"):
        m.ddim.sample(*_cond(inp), known_latents=known[0], **kw)                     # no view axis
    with pytest.raises(ValueError, match="known_noise"):
        m.ddim.sample(*_cond(inp), known_latents=known, known_noise=torch.zeros(1, 2, 5, S, S), **kw)
    assert all(e.pin is None for e in m._engines.values())
