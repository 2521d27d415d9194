"""Batched multi-scene training step, host side (no GPU): the C ABI of the per-scene-timestep entry points, the argument checks that
fire before any device work, and the per-scene order of the random draws (noise_source once per scene, in order; torch's generator
consumed scene after scene exactly as N single-scene steps consume it)."""
import pytest
import torch

TRAIN_SCENE_ENTRY_POINTS = {          # new symbol -> (the entry point it extends, extra arguments)
    "mvd_gridattn_fused_scenes_t": ("mvd_gridattn_fused_scenes", 2),
    "mvd_gridattn_tokens_scenes_t": ("mvd_gridattn_tokens_scenes", 1),
    "mvd_gridattn_tokens_backward_scenes": ("mvd_gridattn_tokens_backward", 2),
    "mvd_layernorm_groups": ("mvd_layernorm", 2),
    "mvd_layernorm_backward_groups": ("mvd_layernorm_backward", 6),
    "mvd_timestep_embedding_scenes": ("mvd_timestep_embedding", 2),
    "mvd_col_sum_groups": ("mvd_col_sum", 1),
}


def test_train_scene_entry_points_are_declared_and_exported():
    import ctypes
    import os
    import re
    from conftest import ROOT
    from mvdfusion_amd import hip
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    declared = set(re.findall(r"\b(mvd_[a-z0-9_]+)\s*\(", hdr))
    so = ctypes.CDLL(hip.LIB_PATHS[hip.OPERAND_FORMAT])
    for name, (base, extra) in TRAIN_SCENE_ENTRY_POINTS.items():
        assert name in declared, name
        assert name in hip.SIGNATURES, name
        assert len(hip.SIGNATURES[name][1]) == len(hip.SIGNATURES[base][1]) + extra, name
        assert hasattr(so, name), name
    assert "mvd_col_sum_groups_workspace_doubles" in declared


def _prep(V, S):
    return {"_prepared": (torch.zeros(V, 5, S, S), None, torch.zeros(1, 5, S, S), None, torch.zeros(V, 796))}


@pytest.fixture(scope="module")
def vf():
    from conftest import model_config
    from mvdfusion_amd.viewfusion_zero_depth_rgb import ViewFusion
    return ViewFusion(**model_config(32))         # (CPU module: the checks fire before any device is touched)


def test_scene_lists_are_validated_before_device_work(vf):
    with pytest.raises(ValueError, match="at least one scene"):
        vf.p_losses_scenes([], {})
    with pytest.raises(ValueError, match="views"):
        vf.p_losses_scenes([_prep(4, 8), _prep(3, 8)], {})
    with pytest.raises(ValueError, match="share S"):
        vf.p_losses_scenes([_prep(4, 8), _prep(4, 16)], {})
    with pytest.raises(ValueError, match="at least one scene"):
        vf.gradients_scenes([], {})
    with pytest.raises(TypeError):
        vf.gradients_scenes(_prep(4, 8), {})
    assert not vf._engines


def test_per_scene_timesteps_need_a_cfg_free_engine():
    from mvdfusion_amd.viewfusion_zero_depth_rgb import StepEngine
    e = StepEngine.__new__(StepEngine)            # (the checks run before any buffer is touched)
    e.cfg, e.N, e.V, e.S = True, 2, 4, 8
    with pytest.raises(ValueError, match="cfg=False"):
        e.set_schedule_scenes(torch.zeros(2, 8), torch.zeros(1, 8, 1, 8, 8))
    e.cfg = False
    with pytest.raises(ValueError, match="step table"):
        e.set_schedule_scenes(torch.zeros(3, 8), torch.zeros(1, 8, 1, 8, 8))


def test_scene_strides_are_rejected_for_a_single_scene():
    """The per-scene strides only mean something with nscene > 1: the C entry points refuse them for one scene (before any launch)."""
    from mvdfusion_amd import hip
    L = hip.lib()
    nul = None
    assert L.mvd_timestep_embedding_scenes(nul, nul, nul, nul, 256, 1, 1, nul) != 0      # (null pointers fail the check as well)
    buf = torch.zeros(64)
    p = hip.ptr(buf)
    it = torch.zeros(1, dtype=torch.int32)
    assert L.mvd_timestep_embedding_scenes(p, hip.ptr(it), p, p, 8, 1, 1, nul) != 0
    assert L.mvd_timestep_embedding_scenes(p, hip.ptr(it), p, p, 8, 0, 0, nul) != 0
    assert L.mvd_gridattn_tokens_scenes_t(p, p, p, hip.ptr(it), p, p, p, p, p, p, 1, 4, 0, 4, 8, 1, 2.0, 0.5, 1, nul) != 0
    assert L.mvd_gridattn_fused_scenes_t(p, p, p, hip.ptr(it), p, p, p, p, p, p, p, p, 1, 4, 0, 4, 8, 1, 2.0, 0.5, 4, 0, 8, nul) != 0
    assert L.mvd_gridattn_fused_scenes_t(p, p, p, hip.ptr(it), p, p, p, p, p, p, p, p, 2, 4, 0, 4, 8, 1, 2.0, 0.5, 4, 1, 6, nul) != 0
    assert L.mvd_gridattn_tokens_backward_scenes(p, p, p, hip.ptr(it), p, p, p, p, 512, p, p, 1.0, 1, 4, 0, 4, 8, 1, 2.0, 0.5, 1, nul) != 0
    assert L.mvd_layernorm_groups(p, p, nul, p, p, 4, 10, 3, 32, 1e-6, 1, nul) != 0              # 3 does not divide 10


def test_noise_source_called_once_per_scene_in_scene_order(vf):
    calls = []

    def ns(V, D, S):
        k = len(calls)
        calls.append((V, D, S))
        return dict(t=torch.full((V,), 10 * k + 1), noise=torch.full((V, 5, S, S), float(k)), depth_noise=torch.full((V, D, S, S), -float(k)),
                    drop_rand=torch.full((V,), 0.5 + k))
    draws = vf.scene_draws([torch.zeros(4, 5, 8, 8)] * 3, ns)
    D = vf.view_attn.n_pts_per_ray
    assert calls == [(4, D, 8)] * 3
    for k, (t, noise, dn, dr) in enumerate(draws):
        assert int(t[0]) == 10 * k + 1 and float(noise[0, 0, 0, 0]) == k and float(dn.flatten()[0]) == -k and float(dr[0]) == 0.5 + k


def test_generator_draws_equal_sequential_single_scene_draws(vf):
    D = vf.view_attn.n_pts_per_ray
    lat = [torch.zeros(4, 5, 8, 8)] * 3
    torch.manual_seed(123)
    batched = vf.scene_draws(lat)
    torch.manual_seed(123)
    single = [vf._draw(x, D, None) for x in lat]
    for a, b in zip(batched, single):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert len({int(d[0][0]) for d in batched}) > 1 or not torch.equal(batched[0][1], batched[1][1])      # the scenes draw apart
