"""Host side of pinned views (no GPU): the chunk plan of a rig larger than one step, the overwrite_x_noisy fixture re-derived with the CPU
oracle, the constructor and config surface, and the plumbing of ViewFusion.sample_rig."""
import pytest
import torch

from conftest import load_golden, load_spec, model_config

from mvdfusion_amd.sampler import DDIMSampler, plan_rig_chunks


# ------------------------------------------------------------------------------------------------ plan_rig_chunks
@pytest.mark.parametrize("M,V,K", [(7, 4, 1), (10, 4, 2), (9, 4, 3), (24, 16, 4), (5, 4, 1), (17, 16, 15)])
def test_plan_covers_the_rig_once_in_order(M, V, K):
    chunks = plan_rig_chunks(M, V, K)
    assert chunks[0] == list(range(V))                                   # chunk 0: no anchors
    new = list(chunks[0])
    for c in chunks[1:]:
        anchors, fresh = c[:K], c[K:]
        assert len(c) <= V and len(fresh) >= 1                           # the last chunk may be shorter, never without a new view
        assert anchors == new[-K:]                                       # default anchors: the K most recently generated views
        assert fresh == list(range(len(new), len(new) + len(fresh)))     # the next ungenerated views, in rig order
        new += fresh
    assert new == list(range(M))                                         # every view generated exactly once
    assert all(len(c) == V for c in chunks[:-1])


def test_plan_examples():
    assert plan_rig_chunks(7, 4, 1) == [[0, 1, 2, 3], [3, 4, 5, 6]]
    assert plan_rig_chunks(10, 4, 2) == [[0, 1, 2, 3], [2, 3, 4, 5], [4, 5, 6, 7], [6, 7, 8, 9]]
    assert plan_rig_chunks(9, 4, 2) == [[0, 1, 2, 3], [2, 3, 4, 5], [4, 5, 6, 7], [6, 7, 8]]      # short last chunk
    assert plan_rig_chunks(3, 4, 1) == [[0, 1, 2]] and plan_rig_chunks(4, 4, 7) == [[0, 1, 2, 3]]  # one step holds the rig: K is not used


def test_plan_custom_anchors():
    seen = []

    def first_and_last(c, done, new):
        seen.append((c, list(done), list(new)))
        return [done[0], done[-1]]
    assert plan_rig_chunks(8, 4, 2, first_and_last) == [[0, 1, 2, 3], [0, 3, 4, 5], [0, 5, 6, 7]]
    assert seen == [(1, [0, 1, 2, 3], [4, 5]), (2, [0, 1, 2, 3, 4, 5], [6, 7])]
    for bad in (lambda c, d, n: [d[0]], lambda c, d, n: [d[0], d[0]], lambda c, d, n: [d[0], n[0]]):      # count, repeats, not generated yet
        with pytest.raises(ValueError):
            plan_rig_chunks(8, 4, 2, bad)


@pytest.mark.parametrize("K", [0, -1, 4, 5])
def test_plan_rejects_anchor_counts_that_leave_no_new_view(K):
    with pytest.raises(ValueError):
        plan_rig_chunks(7, 4, K)
    with pytest.raises(ValueError):
        plan_rig_chunks(0, 4, 1)


# ------------------------------------------------------------------------------------------------ the fixture, re-derived
def test_overwrite_fixture_rederived_with_the_oracle():
    """tests/golden/sample_overwrite_mc32_v3.npz (the REAL reference's loop, tools/make_golden_pinned.py) against
    oracle.ref_torch.denoise_step with row 0 overwritten by the clean input latents before every iteration, at the tool's 5e-5."""
    from conftest import rel_err
    from mvdfusion_amd import synthetic as syn
    from oracle import ref_torch as O
    gd = load_golden("sample_overwrite_mc32_v3")
    V, S, steps = 3, 32, int(gd["xs"].shape[0])
    assert steps == 3 and gd["xs"].shape == (3, V, 5, S, S) and gd["depth_noise"].shape == (3, V, 1, S, S)
    sd = syn.det_fill_state_dict(load_spec(32))
    inp = syn.make_inputs(V, S, seed=9)
    tab = O.ddpm_tables()
    dd = O.ddim_schedule(tab)
    cams = lambda c: {"R": c.R, "T": c.T, "f": c.focal_length, "p": c.principal_point}
    x = gd["x_T"].clone()
    nthreads = torch.get_num_threads()
    torch.set_num_threads(min(16, nthreads))
    try:
        for i in range(steps):
            x = x.clone()
            x[0] = inp["input_latents"][0]
            with torch.no_grad():
                x, x0 = O.denoise_step(sd, x, cams(inp["batch_cameras"]), inp["input_latents"], cams(inp["input_cameras"]),
                                       inp["clip_v_embed"], tab, dd, 49 - i, gd["depth_noise"][i], gd["step_noise"][i], cfg_scale=2.5,
                                       unet_kw=dict(model_channels=32, image_size=S))
            e = max(rel_err(x, gd["xs"][i]), rel_err(x0, gd["x0s"][i]))
            assert e < 5e-5, (i, e)
    finally:
        torch.set_num_threads(nthreads)
    # without the overwrite the first iteration already differs: the fixture exercises the branch
    with torch.no_grad():
        y, _ = O.denoise_step(sd, gd["x_T"], cams(inp["batch_cameras"]), inp["input_latents"], cams(inp["input_cameras"]),
                              inp["clip_v_embed"], tab, dd, 49, gd["depth_noise"][0], gd["step_noise"][0], cfg_scale=2.5,
                              unet_kw=dict(model_channels=32, image_size=S))
    assert rel_err(y[1:], gd["xs"][0][1:]) > 1e-3


# ------------------------------------------------------------------------------------------------ constructor / config surface
class _Sched:
    num_timesteps = 1000

    def __init__(self):
        from mvdfusion_amd.scheduler import make_tables
        tab = make_tables()
        self.alphas_cumprod, self.alphas = tab["alphas_cumprod"], tab["alphas"]


class _Model:
    def __init__(self):
        self.scheduler = _Sched()


def test_sampler_constructs_with_overwrite_x_noisy():
    on = DDIMSampler(_Model(), ddim_num_steps=50, ddim_eta=1.0, overwrite_x_noisy=True)
    off = DDIMSampler(_Model(), ddim_num_steps=50, ddim_eta=1.0)
    assert on.overwrite_x_noisy is True and off.overwrite_x_noisy is False
    assert torch.equal(on.ddim_sigmas, off.ddim_sigmas)


def test_config_with_the_yaml_key_set_builds_the_model():
    """The reference's yaml files carry `overwrite_x_noisy` (configs/*.yaml:115); with the key set to true in a copy of the model's config
    dict the drop-in construction still works and the switch reaches the sampler.  Without the key nothing changes."""
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.load_model import instantiate_from_config
    base = model_config(32)
    cfg = dict(base, overwrite_x_noisy=True)
    target = "mvdfusion_amd.viewfusion_zero_depth_rgb.ViewFusion"      # (what the yaml's target resolves to under install_aliases())
    with syn.skip_default_init():
        m = instantiate_from_config({"target": target, "params": cfg})
        m0 = instantiate_from_config({"target": target, "params": base})
    assert m.ddim.overwrite_x_noisy is True and m0.ddim.overwrite_x_noisy is False
    assert "overwrite_x_noisy" not in base


def test_viewfusion_sample_rig_plumbing(monkeypatch):
    """ViewFusion.sample_rig: prepare_batch once for the whole rig, the sampler's sample_rig with its conditioning, the shape of `sample`."""
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd.viewfusion_zero_depth_rgb import ViewFusion
    with syn.skip_default_init():
        m = ViewFusion(**model_config(32))
    M, S = 7, 32
    prepared = tuple(object() for _ in range(5))
    prep_calls, rig_calls = [], []
    sentinel = torch.zeros(M, 5, S, S)

    def prepare_batch(batch, tc):
        prep_calls.append((batch, tc))
        return prepared

    def sample_rig(*a, **kw):
        rig_calls.append((a, kw))
        return sentinel
    monkeypatch.setattr(m, "prepare_batch", prepare_batch)
    monkeypatch.setattr(m.ddim, "sample_rig", sample_rig)
    tc = dict(input_batch_size=1, train_batch_size=M, random_views=False)
    pick = lambda c, done, new: done[:2]
    out = m.sample_rig("batch", tc, 2.5, 4, anchors_per_chunk=2, anchors=pick, depth=True, verbose=False)
    assert out is sentinel and prep_calls == [("batch", tc)]
    (a, kw), = rig_calls
    assert a == (prepared[1], prepared[2], prepared[3], prepared[4])
    assert kw == dict(unconditional_scale=2.5, chunk_views=4, anchors_per_chunk=2, anchors=pick, depth=True, verbose=False)
    full = m.sample_rig("batch", tc, 2.5, 4, return_input=True, depth=True, verbose=False)
    assert full[0] is sentinel and full[1:4] == (prepared[0], prepared[2], prepared[1]) and len(full) == 5
