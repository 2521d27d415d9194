"""Batched multi-scene sampling, host side (no GPU): the C ABI declarations of the *_scenes entry points, the argument checks that must
fire before any device work, and the per-scene noise order of DDIMSampler.sample_scenes (driven through a stub model and engine)."""
import pytest
import torch


SCENE_ENTRY_POINTS = ("mvd_gridattn_fused_scenes", "mvd_gridattn_tokens_scenes", "mvd_unet_input_scenes")


def test_scene_entry_points_are_declared():
    import os
    import re
    from conftest import ROOT
    from mvdfusion_amd import hip
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    declared = set(re.findall(r"\b(mvd_[a-z0-9_]+)\s*\(", hdr))
    for name in SCENE_ENTRY_POINTS:
        assert name in hip.SIGNATURES, name
        assert name in declared, name
    # each takes the single-scene argument list with `nscene` inserted in front of V
    for name, base in zip(SCENE_ENTRY_POINTS, ("mvd_gridattn_fused", "mvd_gridattn_tokens", "mvd_unet_input")):
        assert len(hip.SIGNATURES[name][1]) == len(hip.SIGNATURES[base][1]) + 1, name


class _StubEngine:
    """Records what the sampler hands the step engine; each step adds 1 to the latents (no device, no library)."""

    def __init__(self, V, S, N):
        self.V, self.S, self.N = V, S, N
        self.x = torch.zeros(N * V, 5, S, S)
        self.x0 = torch.zeros(N * V, 5, S, S)
        self.depth_mode = 0
        self.conds = None
        self.schedule = None
        self.steps = 0

    def set_conditioning(self, *a):
        self.conds = [a]

    def set_conditioning_scenes(self, conds):
        self.conds = list(conds)

    def set_schedule(self, table, dn, sn):
        self.schedule = (table, dn, sn)

    def step(self, cfg_scale, do_update, use_graph=True):
        self.x += 1.0
        self.x0.copy_(self.x * 2.0)
        self.steps += 1


class _StubModel:
    def __init__(self, S):
        from mvdfusion_amd.scheduler import DDPMScheduler

        class _VA:
            n_pts_per_ray = 1
        self.scheduler = DDPMScheduler(timesteps=1000)
        self.view_attn = _VA()
        self._device = torch.zeros(1)
        self.engines = []
        self.S = S

    def engine(self, V, S, D, cfg, q0=0, Vq=None, scenes=1):
        e = _StubEngine(V, S, scenes)
        self.engines.append((dict(V=V, S=S, D=D, cfg=cfg, scenes=scenes), e))
        return e


def _sampler(S=8):
    from mvdfusion_amd.sampler import DDIMSampler
    m = _StubModel(S)
    return m, DDIMSampler(m, ddim_num_steps=50, ddim_discretize="uniform", ddim_eta=1.0, latent_size=S, z_dim=4)


def _cond(V, S, seed):
    from mvdfusion_amd import synthetic as syn
    inp = syn.make_inputs(V, S, seed=seed)
    return (inp["batch_cameras"], inp["input_latents"], inp["input_cameras"], inp["clip_v_embed"])


def test_sample_scenes_rejects_mismatched_scenes_before_device_work():
    m, sam = _sampler(8)
    with pytest.raises(ValueError, match="views"):
        sam.sample_scenes([_cond(4, 8, 1), _cond(3, 8, 2)], unconditional_scale=2.5, verbose=False)
    with pytest.raises(ValueError, match="latent"):
        sam.sample_scenes([_cond(4, 8, 1), _cond(4, 16, 2)], unconditional_scale=2.5, verbose=False)
    with pytest.raises(ValueError):
        sam.sample_scenes([], unconditional_scale=2.5, verbose=False)
    with pytest.raises(ValueError, match="x_T"):
        sam.sample_scenes([_cond(4, 8, 1), _cond(4, 8, 2)], unconditional_scale=2.5, verbose=False, x_T=torch.zeros(4, 5, 8, 8))
    assert not m.engines                          # nothing reached the engine


def test_scenes_with_a_partial_view_range_are_rejected():
    from conftest import model_config
    from mvdfusion_amd.viewfusion_zero_depth_rgb import StepEngine, ViewFusion
    vf = ViewFusion(**model_config(32))           # (CPU module: the checks fire before any device is touched)
    with pytest.raises(ValueError, match="single-scene"):
        vf.engine(4, 32, 1, True, q0=0, Vq=2, scenes=2)
    with pytest.raises(ValueError, match="single-scene"):
        vf.engine(4, 32, 1, True, q0=1, scenes=3)
    with pytest.raises(ValueError):
        vf.engine(4, 32, 1, True, scenes=0)
    with pytest.raises(ValueError, match="single-scene"):
        StepEngine(vf, 4, 32, 1, True, "cpu", 3, q0=2, Vq=2, scenes=2)
    assert not vf._engines


def test_noise_source_called_once_per_scene_in_order_and_stacked_scene_major():
    m, sam = _sampler(8)
    V, S, N, total = 3, 8, 3, 50
    calls = []

    def source(v, s, d, steps):
        k = len(calls)
        calls.append((v, s, d, steps))
        dn = torch.full((steps, v, d, s, s), float(k)) + torch.arange(v).view(1, v, 1, 1, 1) * 0.1
        sn = torch.full((steps, v, 5, s, s), -float(k)) - torch.arange(v).view(1, v, 1, 1, 1) * 0.1
        return dn, sn
    sam.noise_source = source
    conds = [_cond(V, S, 3), _cond(V, S, 7), _cond(V, S, 11)]
    x_T = torch.randn(N, V, 5, S, S)
    x, inter = sam.sample_scenes(conds, unconditional_scale=2.5, return_intermediates=True, verbose=False, x_T=x_T, num_steps=4)
    assert calls == [(V, S, 1, total)] * N
    (spec, eng), = m.engines
    assert spec == dict(V=V, S=S, D=1, cfg=True, scenes=N)
    _, dn, sn = eng.schedule
    assert dn.shape == (total, N * V, 1, S, S) and sn.shape == (total, N * V, 5, S, S)
    for n in range(N):
        for v in range(V):
            g = n * V + v                          # global view index: scene-major
            assert torch.allclose(dn[:, g], torch.full_like(dn[:, g], n + 0.1 * v))
            assert torch.allclose(sn[:, g], torch.full_like(sn[:, g], -n - 0.1 * v))
    # the conditioning goes to the engine in scene order, the initial noise scene-major
    assert len(eng.conds) == N
    for i, c in enumerate(eng.conds):          # each scene's own cameras, input latents and embedding, in scene order
        assert c[0] is conds[i][0] and c[2] is conds[i][2]
        assert torch.equal(c[1], conds[i][1]) and torch.equal(c[3], conds[i][3])
    assert eng.steps == 4 and x.shape == (N, V, 5, S, S) and torch.allclose(x, x_T + 4.0)
    assert len(inter) == 4 and all(it["xt"].shape == (N, V, 5, S, S) and it["x0"].shape == (N, V, 5, S, S) for it in inter)
    assert torch.allclose(inter[1]["x0"], (x_T + 2.0) * 2.0)


def test_sample_scenes_scene_noise_equals_single_scene_noise():
    """A scene of a batched call sees exactly the depth / DDIM noise a single-scene `sample` would give it with the same source."""
    def source_for(seed):
        def source(v, s, d, steps):
            g = torch.Generator().manual_seed(seed)
            return torch.randn(steps, v, d, s, s, generator=g), torch.randn(steps, v, 5, s, s, generator=g)
        return source
    V, S = 2, 8
    conds = [_cond(V, S, 1), _cond(V, S, 2)]
    m1, s1 = _sampler(S)
    s1.noise_source = source_for(5)
    s1.sample(*conds[1], unconditional_scale=2.5, depth=True, verbose=False, x_T=torch.zeros(V, 5, S, S), num_steps=1)
    _, dn1, sn1 = m1.engines[0][1].schedule
    mN, sN = _sampler(S)
    sN.noise_source = source_for(5)               # (the same draws on every call: both scenes get them)
    sN.sample_scenes(conds, unconditional_scale=2.5, verbose=False, x_T=torch.zeros(2, V, 5, S, S), num_steps=1)
    _, dnN, snN = mN.engines[0][1].schedule
    assert torch.equal(dnN[:, V:], dn1) and torch.equal(snN[:, V:], sn1) and torch.equal(dnN[:, :V], dn1)
