"""Windowed cross-view aggregation (GridAttn keep_top_k_views), host side (no GPU): the slot -> view rule, construction through the
class surface and the config helpers, the fixtures, the C ABI of the *_window entry points and the argument checks that fire before any
device work."""
import os

import pytest
import torch

from conftest import ROOT, load_golden, load_spec

WINDOW_ENTRY_POINTS = {               # new symbol -> the entry point it extends by `int window`
    "mvd_gridattn_fused_window": "mvd_gridattn_fused_scenes_t",
    "mvd_gridattn_tokens_window": "mvd_gridattn_tokens_scenes_t",
    "mvd_gridattn_tokens_backward_window": "mvd_gridattn_tokens_backward_scenes",
}

FIXTURES = {                          # fixture -> (top_k, V)
    "gridattn_topk4_v8_d1": (4, 8), "gridattn_topk4_v15_d1": (4, 15), "gridattn_topk2_v8_d3": (2, 8), "gridattn_topk4_v3_d3": (4, 3),
    "gridattn_topk4_v24_d1": (4, 24), "step_mc32_v8_d1_topk4": (4, 8), "step_mc32_v24_d1_topk4": (4, 24),
    "train_grads_mc32_v8_d3_topk2": (2, 8),
}


def test_window_view_table_is_the_reference_rule():
    from mvdfusion_amd.view_attn_efficient2 import window_size, window_view_table
    # V = 8, top_k = 4: slot j (row) of query views 0..7 (columns)
    want = torch.tensor([[6, 7, 0, 1, 2, 3, 4, 5],
                         [7, 0, 1, 2, 3, 4, 5, 6],
                         [0, 1, 2, 3, 4, 5, 6, 7],
                         [1, 2, 3, 4, 5, 6, 7, 0],
                         [2, 3, 4, 5, 6, 7, 0, 1]])
    assert torch.equal(window_view_table(8, 4), want)
    assert torch.equal(window_view_table(8, 5), want)                 # top_k = 5: the same window
    # W > V (V = 3, top_k = 4): the modulo repeats views
    assert torch.equal(window_view_table(3, 4), torch.tensor([[1, 2, 0], [2, 0, 1], [0, 1, 2], [1, 2, 0], [2, 0, 1]]))
    assert torch.equal(window_view_table(8, 2), torch.tensor([[7, 0, 1, 2, 3, 4, 5, 6], [0, 1, 2, 3, 4, 5, 6, 7], [1, 2, 3, 4, 5, 6, 7, 0]]))
    assert [window_size(True, k) for k in (2, 3, 4, 5)] == [3, 3, 5, 5]
    assert window_size(False, 4) == 0


def test_gridattn_builds_with_the_window_and_keeps_its_state_dict():
    from mvdfusion_amd.view_attn_efficient2 import GridAttn
    kw = dict(in_channels=5, input_size=32, output_dim=768, num_layers=3, z_near_far_scale=0.8, n_pts_per_ray=1)
    ga = GridAttn(keep_top_k_views=True, top_k=4, **kw)
    assert ga.keep_top_k_views and ga.top_k == 4 and ga.window == 5
    assert ga.rows_per_point(8) == 5 and ga.rows_per_point(24) == 5
    full = GridAttn(**kw)
    assert not full.keep_top_k_views and full.window == 0 and full.rows_per_point(8) == 8
    spec = {k[len("view_attn."):]: s for k, s in load_spec(32) if k.startswith("view_attn.")}
    sd = ga.state_dict()
    assert set(sd) == set(spec) == set(full.state_dict())
    assert all(tuple(sd[k].shape) == spec[k] for k in spec)
    # the fused kernel goes by the rows of a point: 24 views at W = 5 are served, 24 views without a window are not
    assert ga.fused_supported(24, 24 * 1024 * 5) and ga.fused_supported(8, 8 * 1024 * 5) and ga.fused_supported(3, 3 * 1024 * 3 * 5)
    assert not full.fused_supported(24, 24 * 24 * 1024)
    assert full.fused_supported(15, 15 * 15 * 1024)
    assert GridAttn(keep_top_k_views=True, top_k=2, **kw).window == 3


def test_viewfusion_builds_from_a_config_with_the_key_set():
    import mvdfusion_amd.configs as configs
    from mvdfusion_amd.viewfusion_zero_depth_rgb import ViewFusion
    va = configs.model_config(32)["view_attn_config"]
    va = dict(va, params=dict(va["params"], keep_top_k_views=True, top_k=4))
    m = ViewFusion(**configs.model_config(32, view_attn_config=va))
    assert m.view_attn.keep_top_k_views and m.view_attn.window == 5
    assert configs.state_dict_spec(m) == configs.state_dict_spec(ViewFusion(**configs.model_config(32)))      # same parameters, same keys
    assert set(load_spec(32)) <= set(configs.state_dict_spec(m))


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixture_loads_and_records_top_k(name):
    top_k, V = FIXTURES[name]
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    assert os.path.getsize(path) < 1024 * 1024, os.path.getsize(path)
    gd = load_golden(name)
    assert int(gd["top_k"]) == top_k
    if name.startswith("gridattn_"):
        sy, sx, sc = (int(v) for v in gd["lattice"])
        D = gd["depth_noise"].shape[1]
        assert gd["x"].shape == (V, 5, 32, 32) and gd["t_embed"].shape == (V, 256) and gd["depth_noise"].shape == (V, D, 32, 32)
        assert gd["out_strided"].shape == (V, len(range(0, 32, sy)), len(range(0, 32, sx)), D, len(range(0, 768, sc)))
        assert bool(torch.isfinite(gd["out_strided"]).all()) and float(gd["out_std"]) > 0
    elif name.startswith("step_"):
        assert [int(i) for i in gd["indices"]] == [49, 1, 0]
        nv = len(gd["views"])               # the views whose latents are stored: all 8, every third of 24
        assert nv == 8 and int(gd["views"].max()) < V and int(gd["views"].max()) >= V - 3
        assert all(gd[f"x_prev_{i}"].shape == (nv, 5, 32, 32) and gd[f"x0_{i}"].shape == (nv, 5, 32, 32) for i in (49, 1, 0))
    else:
        assert len(gd["grad_names"]) == 994 == len(gd["grad_norms"]) == len(gd["grad_projs"]) and float(gd["loss"]) > 0


def test_window_entry_points_are_declared_and_exported():
    import ctypes
    import re
    from mvdfusion_amd import hip
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    declared = set(re.findall(r"\b(mvd_[a-z0-9_]+)\s*\(", hdr))
    so = ctypes.CDLL(hip.LIB_PATHS[hip.OPERAND_FORMAT])
    for name, base in WINDOW_ENTRY_POINTS.items():
        assert name in declared, name
        assert name in hip.SIGNATURES, name
        assert len(hip.SIGNATURES[name][1]) == len(hip.SIGNATURES[base][1]) + 1, name
        assert hasattr(so, name), name
    assert "(b + j - W/2) mod V" in hdr                    # the slot -> view rule is part of the documented ABI


def test_window_arguments_are_checked_before_any_launch():
    from mvdfusion_amd import hip
    L = hip.lib()
    buf = torch.zeros(64)
    p, it, nul = hip.ptr(buf), hip.ptr(torch.zeros(1, dtype=torch.int32)), None
    tok = lambda V, window: L.mvd_gridattn_tokens_window(p, p, p, it, p, p, p, p, p, p, 1, V, 0, V, 8, 1, 2.0, 0.5, 0, window, nul)
    fus = lambda V, window: L.mvd_gridattn_fused_window(p, p, p, it, p, p, p, p, p, p, p, p, 1, V, 0, V, 8, 1, 2.0, 0.5, 4, 0, 0, window, nul)
    bwd = lambda V, window: L.mvd_gridattn_tokens_backward_window(p, p, p, it, p, p, p, p, 512, p, p, 1.0, 1, V, 0, V, 8, 1, 2.0, 0.5, 0,
                                                                  window, nul)
    for f in (tok, fus, bwd):
        assert f(8, 4) != 0            # a window is odd
        assert f(8, -1) != 0
        assert f(8, 17) != 0           # at most 16 rows per point
        assert f(24, 0) != 0           # no window: the rows of a point are the V views
