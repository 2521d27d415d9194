"""Write the fixtures of the windowed cross-view aggregation (GridAttn keep_top_k_views=True) into tests/golden/ by running the REAL
reference -- container-only, like oracle/make_golden.py, whose helpers and shims this uses; it calls the reference and copies nothing
from it.

The reference classes are built by oracle/make_golden.py with the default constructor (no window); here the reference's GridAttn is swapped,
for the duration of one fixture, for a subclass whose constructor adds keep_top_k_views=True / top_k, and the oracle restatement
(oracle/ref_torch.py: gridattn_forward, which every cross-check of make_golden goes through) for the windowed restatement below -- so each
fixture is still required to agree with an independent restatement of what it records.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_window.py [--only NAME]
"""
import argparse
import contextlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as G  # noqa: E402  (installs the shims)

O = G.O


def window_table(V, top_k):
    """(W, V): slot j of query view b holds reference view (b + j - top_k // 2) mod V."""
    half = top_k // 2
    return (torch.arange(-half, half + 1)[:, None] + torch.arange(V)[None, :]) % V


def windowed_gridattn_forward(top_k):
    """oracle.ref_torch.gridattn_forward over the W window rows of every 3-D point instead of all V views."""

    def forward(sd, pre, noisy_latents, cams, t_embed, t, tables, depth_noise, input_latents, in_cam, n_pts_per_ray=1, depth_scale=2.0,
                depth_shift=0.5, return_tokens=False, overwrite_attn_depth=None):
        V, _, S, _ = noisy_latents.shape
        D = n_pts_per_ray
        sac = tables["sqrt_alphas_cumprod"][t]
        std = tables["sqrt_one_minus_alphas_cumprod"][t] / sac / 10.0
        dch = noisy_latents[:, 4:] / sac[:, None, None, None] if overwrite_attn_depth is None else overwrite_attn_depth
        samples = dch.expand(-1, D, -1, -1) + std[:, None, None, None] * depth_noise
        depth = torch.clip((samples + 1.0) / 2.0, 0.0, 1.0) * depth_scale + depth_shift

        def zemb(x):
            return F.gelu(O._lin(sd, pre + "z_embedder.0", x.permute(0, 2, 3, 1))).permute(0, 3, 1, 2)

        z = O.gridattn_tokens(zemb(noisy_latents), zemb(input_latents), cams, in_cam, depth, S)      # (Vref, Vq, n, 723)
        idx = window_table(V, top_k)                                                                 # (W, Vq)
        z = z[idx, torch.arange(V)[None, :]]                                                         # (W, Vq, n, 723)
        W, n = z.shape[0], z.shape[2]
        x = z.permute(1, 2, 0, 3).reshape(V * n, W, -1)
        if return_tokens:
            return x
        x = F.gelu(O._lin(sd, pre + "pre_layer_b.0", x))
        for li in range(3):
            x = O._dit_block(sd, f"{pre}aggregation_transformer.layer_list.{li}.", x, t_embed[:1])
        w = O._lin(sd, pre + "aggregation_transformer.weight_layer", x).softmax(dim=-2)
        return O._lin(sd, pre + "final_layer_b", (x * w).sum(dim=-2)).reshape(V, S, S, D, -1)

    return forward


@contextlib.contextmanager
def windowed(top_k):
    import mvdfusion.view_attn_efficient2 as RV
    ref_cls, oracle_fn = RV.GridAttn, O.gridattn_forward

    class WindowedGridAttn(ref_cls):
        def __init__(self, *a, **kw):
            kw.update(keep_top_k_views=True, top_k=top_k)
            super().__init__(*a, **kw)

    RV.GridAttn, O.gridattn_forward = WindowedGridAttn, windowed_gridattn_forward(top_k)
    try:
        yield
    finally:
        RV.GridAttn, O.gridattn_forward = ref_cls, oracle_fn


def _add_keys(name, views=None, **extra):
    """Re-save a fixture with extra entries; views: keep only these views of the per-step latents (a 24-view step is 2.7 MB otherwise)."""
    path = os.path.join(G.GOLD, name + ".npz")
    with np.load(path, allow_pickle=False) as f:
        arrs = {k: f[k] for k in f.files}
    if views is not None:
        arrs = {k: (v[views] if k.startswith(("x_prev_", "x0_")) else v) for k, v in arrs.items()}
        arrs["views"] = np.asarray(views, dtype=np.int64)
    arrs.update({k: np.asarray(v) for k, v in extra.items()})
    np.savez_compressed(path, **arrs)
    print(f"  {name}.npz: + {sorted(extra)} ({os.path.getsize(path) / 1024:.0f} KB)")


def gold_gridattn_window(tag, V, D, top_k, seed, t_val, lattice=(5, 7, 3)):
    """One GridAttn forward; stored like the gridattn_* fixtures of make_golden (inputs, strided output lattice, summaries) + top_k and
    the lattice strides (y, x, channel)."""
    with windowed(top_k):
        c = G._gridattn_case(V, D, 32, seed, t_val, tokens=False)
    out = c.pop("out")
    c.pop("tokens_sample")
    sy, sx, sc = lattice
    G.save(tag, out_strided=out[:, ::sy, ::sx, :, ::sc].contiguous(), out_mean=out.mean(), out_std=out.std(), out_l2=out.norm(),
           top_k=np.int64(top_k), lattice=np.asarray(lattice, dtype=np.int64), **c)


def gold_step_window(tag, V, D, top_k, views=None):
    """Three denoise_apply steps (lean: the test re-draws the noise); x_prev / x0 of `views` (default: all V) are stored."""
    with windowed(top_k):
        G.gold_step(32, V, D, tag, indices=(49, 1, 0), lean=True)
    _add_keys(tag, views=list(range(V)) if views is None else views, top_k=np.int64(top_k))


def gold_train_window(tag, V, D, top_k):
    with windowed(top_k):
        G.gold_train_loss(32, V, D, tag.replace("train_grads", "train_loss"), seed=31, grads_tag=tag)
    os.remove(os.path.join(G.GOLD, tag.replace("train_grads", "train_loss") + ".npz"))      # (the loss is in the gradient fixture too)
    _add_keys(tag, top_k=np.int64(top_k))


TARGETS = {
    "gridattn_topk4_v8_d1": lambda: gold_gridattn_window("gridattn_topk4_v8_d1", 8, 1, 4, 12, 21),
    "gridattn_topk4_v15_d1": lambda: gold_gridattn_window("gridattn_topk4_v15_d1", 15, 1, 4, 13, 741),
    "gridattn_topk2_v8_d3": lambda: gold_gridattn_window("gridattn_topk2_v8_d3", 8, 3, 2, 14, 501, lattice=(5, 7, 6)),
    "gridattn_topk4_v3_d3": lambda: gold_gridattn_window("gridattn_topk4_v3_d3", 3, 3, 4, 15, 161),
    "gridattn_topk4_v24_d1": lambda: gold_gridattn_window("gridattn_topk4_v24_d1", 24, 1, 4, 16, 381, lattice=(5, 7, 12)),
    "step_mc32_v8_d1_topk4": lambda: gold_step_window("step_mc32_v8_d1_topk4", 8, 1, 4),
    "step_mc32_v24_d1_topk4": lambda: gold_step_window("step_mc32_v24_d1_topk4", 24, 1, 4, views=list(range(0, 24, 3))),
    "train_grads_mc32_v8_d3_topk2": lambda: gold_train_window("train_grads_mc32_v8_d3_topk2", 8, 3, 2),
}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for name, fn in TARGETS.items():
        if a.only is None or a.only == name:
            print(name)
            fn()
