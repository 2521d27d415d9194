"""ViewFusion facade on the MI355X-native hot path -- mirror of
``mvdfusion.viewfusion_zero_depth_rgb.ViewFusion`` (mvdfusion/viewfusion_zero_depth_rgb.py:19-417).

Drop-in surface kept: constructor kwargs (unknown keys ignored, :41), ``apply_model`` (:282), ``sample`` (:348),
``embed_time`` (:276), ``prepare_batch`` (:165), ``encode``/``decode`` (:157-163), ``forward``/``p_losses`` (:362-397
-- the training loss with a hand-written HIP backward behind torch autograd), ``configure_optimizers`` (:399), ``_print_parameter_count`` (:134),
``.ddim`` (DDIMSampler), ``.scheduler``; state_dict keys ``view_attn.*``, ``unet_model.unet_model.*``,
``cc_projection.{0,2,4}``, ``time_embed.{0,2}``, ``scheduler.*`` (+ ``vae.*`` / ``clip_image_encoder.*`` when those
host-side PyTorch modules are plugged in -- they are outside the hot path).

The per-step work is done by :class:`StepEngine`: static buffers + device-resident step tables, one hipGraph per
(V, S, D, cfg) signature, replayed once per DDIM step.
"""
import math

import torch
import torch.nn as nn

from . import hip
from .cameras import Cameras, get_camera_slice, get_relative_camera, pack_cameras
from .engine import Ctx, ddim_step_table
from .sampler import DDIMSampler
from .scheduler import DDPMScheduler
from .unet import UNetWrapper
from .view_attn_efficient2 import GridAttn

import os

# Weight prefetch inside the graph-replayed step (include/mvd_hip.h: mvd_gemm_desc.pf_items).  MVD_PREFETCH=0 turns it
# off (A/B runs); MVD_PREFETCH_OPTS="window=100663296,max_items=24" overrides hip.WeightPrefetcher's parameters.
PREFETCH_WEIGHTS = os.environ.get("MVD_PREFETCH", "ws")          # "ws" (in-kernel, default) | "0"
PREFETCH_OPTIONS = {k: int(v) for k, v in (kv.split("=") for kv in os.environ.get("MVD_PREFETCH_OPTS", "").split(",") if kv)}


def _sinusoid_freqs(dim, max_period=10000):
    """exp(-ln(max_period) * i / half), computed on the host exactly as the reference does
    (diffusionmodules/util.py:161-164; mvdfusion/embedder.py:124-127)."""
    half = dim // 2
    return torch.exp(-math.log(max_period) * torch.arange(start=0, end=half, dtype=torch.float32) / half)


class StepEngine:
    """One denoising iteration (GridAttn -> CFG-batched UNet -> CFG combine [+ DDIM update]) on static buffers.

    scenes = N independent objects denoised together (same V, S, D, cfg, schedule and weights; own cameras, input view, CLIP embedding
    and noise): every per-view buffer holds N*V views scene-major (global view scene*V + v), the per-scene ones (input latents, input
    camera) N, and the UNet's CFG batch is [N*V conditional rows | N*V null rows].  View-parallel sharding (q0 / Vq) is single-scene only.

    The buffers here go by the rig size V whatever GridAttn's window is; the token / attention arenas that go by the rows of a 3-D point
    (W with model.view_attn.keep_top_k_views, else V) are workspace buffers keyed by their shape (engine.Workspace), allocated by the
    first eager step with the window the model was built with and captured by its graphs."""

    def __init__(self, model, V, S, D, cfg, device, prec, q0=0, Vq=None, policy=None, scenes=1):
        self.m, self.V, self.S, self.D, self.cfg = model, V, S, D, bool(cfg)
        self.q0, self.Vq = q0, (V if Vq is None else Vq)   # query views owned by this rank (view-parallel sharding)
        self.N = N = int(scenes)
        if N < 1 or (N > 1 and (self.q0 != 0 or self.Vq != V)):
            raise ValueError(f"StepEngine(scenes={scenes}, q0={q0}, Vq={Vq}, V={V}): view-parallel sharding is single-scene only")
        NV = N * V
        self.ctx = Ctx(device, prec, policy)
        dev = self.ctx.device
        B = 2 * N * self.Vq if cfg else N * self.Vq
        self.B = B
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.x = z(NV, 5, S, S)                # current latents (NCHW like the reference), updated in place
        self.x0 = z(NV, 5, S, S)
        self.eps = z(NV, 5, S, S)
        self.input_latents = z(N, 5, S, S)
        self.clip_v_embed = z(NV, 796)
        self.cams = z(NV, hip.CAM_RECORD)
        self.in_cam = z(N, hip.CAM_RECORD)
        self.context = z(B, 768)               # rows [NV,2NV) stay zero: the null branch (unet.py:173)
        self.vol = z(B * S * S * D, 768)       # rows of the null branch stay zero (unet.py:190)
        # the same as split planes, inside the level-0 operand buffer of the UNet's view-aligned transformers (zero-initialised)
        self.vol_planes, self.vol_col = model.unet_model.level0_operand(self.ctx, B, S, D)
        self.x_in = torch.zeros(B * S * S, 2 * 32, dtype=torch.int16, device=dev)              # UNet input (split planes)
        self.iter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.steps = z(1, hip.STEP_STRIDE)
        self.steps_nodiv = z(1, hip.STEP_STRIDE)   # the same table with sqrt(alpha_bar) = 1: GridAttn's depth source is used as is
        self.prev = z(NV, 5, S, S)             # channel 4: an explicit overwrite_attn_depth (apply_model(prev_depth=...))
        self.depth_mode = 0                    # GridAttn samples depth around 0: x[:,4] / sqrt(alpha_bar) (the x0-style estimate);
                                               # 1: the previous step's x0 estimate self.x0[:,4] (DDIMSampler feed_prev_depth);
                                               # 2: self.prev[:,4] (view_attn_efficient2.py:418-426)
        self.pin = None                        # pinned views: None, or (mode, K) -- the first K view rows of every scene are rewritten from
                                               # self.known at the start of each step (set_pin; include/mvd_hip.h: mvd_pin_views).
                                               # mode 0: the clean rows (DDIMSampler overwrite_x_noisy); 1: re-noised to the step's timestep
        self.known = z(1, 5, S, S)             # (N*K, 5, S, S) clean latents of the pinned views, scene-major
        self.pin_noise = None                  # mode 1: (rows of the step table, N*K, 5, S, S) standard normal
        self.depth_noise = z(1, NV, D, S, S)
        self.ddim_noise = z(1, NV, 5, S, S)
        self.f256 = _sinusoid_freqs(256).to(dev)
        self.funet = _sinusoid_freqs(model.unet_model.unet_model.model_channels).to(dev)
        self.graphs = {}
        self.prefetchers = {}      # per captured graph: its hip.WeightPrefetcher (None when PREFETCH_WEIGHTS is off)
        # per-sample vectors ("Per-sample vectors"): what a step derives from the conditioning or the schedule alone is computed
        # once per set_conditioning* / set_schedule by the step's own launches (refresh_vectors); the step then copies row `iter` of the
        # tables (mvd_select_step_rows).  MVD_STEP_TABLES=0: every step computes them in place, as before (A/B runs).
        self.step_tables = os.environ.get("MVD_STEP_TABLES", "1") != "0"
        self.iter0 = torch.zeros(1, dtype=torch.int32, device=dev)        # row 0: the tables are built from the top of the step table
        self._tables = None        # {"c", "emb", "bias" (+ scratch)}: one row per row of self.steps
        self._cond_sig = None      # (model signature,) the conditioning vectors / the schedule tables were computed under; None: stale
        self._tab_sig = None
        self._drop_masks = None    # training forward: (clip_mask, volume_mask, concat_mask), each (Vq,) in {0, 1} (unet.py:140-151)
        self.n_rows = 1            # rows of the device step table; the kernels index steps[iter], noise[iter] unchecked
        self.steps_scene_stride = 0      # 0: one timestep for every scene; 1 (set_schedule_scenes, cfg=False): scene n reads step row iter + n
        self.done = 0              # host mirror of the device iteration counter

    # -- host-side inputs ----------------------------------------------------------------------------
    def set_conditioning(self, batch_cameras, input_latents, input_cameras, clip_v_embed):
        self.set_conditioning_scenes([(batch_cameras, input_latents, input_cameras, clip_v_embed)])

    def set_conditioning_scenes(self, conds):
        """conds: one (batch_cameras, input_latents, input_cameras, clip_v_embed) per scene, in scene order."""
        if len(conds) != self.N:
            raise ValueError(f"set_conditioning_scenes: {len(conds)} scenes for a {self.N}-scene engine")
        V, S = self.V, self.S
        for n, (bc, il, ic, ce) in enumerate(conds):
            self.cams[n * V:(n + 1) * V].copy_(pack_cameras(bc).to(self.cams.device))
            self.in_cam[n:n + 1].copy_(pack_cameras(ic).to(self.cams.device))
            self.input_latents[n:n + 1].copy_(il.reshape(1, 5, S, S))
            self.clip_v_embed[n * V:(n + 1) * V].copy_(ce.reshape(V, 796))
        self._cond_sig = None

    @property
    def drop_masks(self):
        return self._drop_masks

    @drop_masks.setter
    def drop_masks(self, masks):
        self._drop_masks = masks
        if masks is not None:      # the masked step scales self.context in place: whatever refresh_vectors left there is gone
            self._cond_sig = None

    def invalidate(self):
        """The weights changed: captured graphs (packed images by address) and the per-sample vectors computed from them are stale."""
        self.graphs.clear()
        self.prefetchers.clear()
        self._cond_sig = self._tab_sig = None

    # -- per-sample vectors ---------------------------------------------------------------------------
    def tables_apply(self):
        """The step may read the per-sample vectors: one shared timestep, no condition dropout, no backward behind it, and a schedule of
        more than one row (a one-row schedule is set anew for every step -- apply_model -- so building its table would cost the step's own
        launches plus the selection: it stays on the in-place path)."""
        return self.step_tables and self.steps_scene_stride == 0 and self._drop_masks is None and not self.ctx.keep_fp32 and \
            int(self.steps.shape[0]) > 1

    def _model_sig(self):
        # hip.params_signature of the whole model as ViewFusion.engine() last saw it: the check that guards the packed weight images
        return (getattr(self.m, "_packed_sig", None),)

    def vector_plan(self):
        """Host mirror of what a graph-replayed step spends on the conditioning / time vectors: (launches in the step, rows of the
        schedule tables or None where none is built).  In place: 2 sinusoids + 5 GEMVs over the time rows, 3 GEMVs over the conditional
        rows, 1 over the CFG batch (16 rows per launch); with the per-sample vectors: the one row selection."""
        if self.tables_apply():
            return 1, int(self.steps.shape[0])
        chunks = lambda rows: -(-rows // 16)
        return 2 + 5 * chunks(self.t_rows) + 3 * chunks(self.N * self.Vq) + chunks(self.B), None

    def vectors_valid(self):
        sig = self._model_sig()
        return self.tables_apply() and self._cond_sig == sig and self._tab_sig == sig

    def refresh_vectors(self):
        """Recompute what is stale: the conditioning vectors (context rows of the conditional branch, xattn.vec) after set_conditioning* /
        a masked step, the schedule tables (ViewFusion time vector c, UNet emb and per-ResBlock bias row per step row) after
        set_schedule, both after a weight change.  Called by step() in front of a graph capture or replay, never inside a capture."""
        m, ctx, L, st = self.m, self.ctx, hip.lib(), hip.stream
        unet = m.unet_model.unet_model
        sig = self._model_sig()
        if self._cond_sig != sig:
            NVq, p = self.N * self.Vq, m.cc_projection
            ctx.context = self.context
            wx, bx, _, nx = unet.xattn_weights()
            c1, c2 = ctx.ws.get("vf.cc1", (NVq, 768)), ctx.ws.get("vf.cc2", (NVq, 768))
            clip = self.clip_v_embed[self.q0:self.q0 + NVq]
            hip.check(L.mvd_cond_vectors(hip.ptr(clip), clip.stride(0), NVq, 796, 768, hip.ptr(p[0].weight), hip.ptr(p[0].bias),
                                         hip.ptr(p[2].weight), hip.ptr(p[2].bias), hip.ptr(p[4].weight), hip.ptr(p[4].bias), hip.ptr(c1),
                                         hip.ptr(c2), hip.ptr(self.context), hip.ptr(wx), hip.ptr(bx), nx, self.B,
                                         hip.ptr(unet.xattn_buffer(ctx)), st()))
            self._cond_sig = sig
        if self._tab_sig != sig:
            n, mc = int(self.steps.shape[0]), unet.model_channels
            we, be, _ = unet.temb_weights()
            ted, nb = 4 * mc, int(we.shape[0])
            T = self._tables
            if T is None:
                e = lambda w: torch.empty(n, w, dtype=torch.float32, device=ctx.device)
                T = self._tables = dict(c=e(256), emb=e(ted), bias=e(nb), tsin=e(256), h=e(256), tsu=e(mc), e1=e(ted))
            t, u = m.time_embed, unet.time_embed
            hip.check(L.mvd_step_table(hip.ptr(self.steps), hip.ptr(self.iter0), n, hip.ptr(self.f256), 256, 256, hip.ptr(t[0].weight),
                                       hip.ptr(t[0].bias), hip.ptr(t[2].weight), hip.ptr(t[2].bias), None, None, 0, hip.ptr(T["tsin"]),
                                       hip.ptr(T["h"]), hip.ptr(T["c"]), None, st()))
            hip.check(L.mvd_step_table(hip.ptr(self.steps), hip.ptr(self.iter0), n, hip.ptr(self.funet), mc, ted, hip.ptr(u[0].weight),
                                       hip.ptr(u[0].bias), hip.ptr(u[2].weight), hip.ptr(u[2].bias), hip.ptr(we), hip.ptr(be), nb,
                                       hip.ptr(T["tsu"]), hip.ptr(T["e1"]), hip.ptr(T["emb"]), hip.ptr(T["bias"]), st()))
            self._tab_sig = sig

    def set_schedule(self, steps_table, depth_noise, ddim_noise):
        self._set_tables(steps_table, depth_noise, ddim_noise, scene_stride=0)

    def set_schedule_scenes(self, steps_table, depth_noise, ddim_noise=None):
        """One training step with a timestep PER SCENE: steps_table (N, STEP_STRIDE) holds scene n's row n, depth_noise (1, N*V, D, S, S).
        Only on cfg=False engines (the training forward; a guided sampling step shares one schedule) and without a DDIM update."""
        if self.cfg:
            raise ValueError("StepEngine.set_schedule_scenes: per-scene timesteps need a cfg=False engine (the training step); "
                             "guided sampling steps share one timestep")
        if tuple(steps_table.shape) != (self.N, hip.STEP_STRIDE):
            raise ValueError(f"StepEngine.set_schedule_scenes: step table {tuple(steps_table.shape)} for {self.N} scenes "
                             f"(expected ({self.N}, {hip.STEP_STRIDE}))")
        if ddim_noise is None:
            ddim_noise = torch.zeros(1, self.N * self.V, 5, self.S, self.S)
        self._set_tables(steps_table, depth_noise, ddim_noise, scene_stride=1 if self.N > 1 else 0)

    def _set_tables(self, steps_table, depth_noise, ddim_noise, scene_stride):
        """Load the step table and noise, then rewind: scene n reads step row iter + n * scene_stride (scene_stride 0: one shared row)."""
        dev = self.ctx.device
        if self.steps.shape != steps_table.shape:
            self.graphs.clear()                # table buffers are re-allocated: captured pointers go stale
            self.prefetchers.clear()
            self.steps = steps_table.to(dev).contiguous()
            self.steps_nodiv = self.steps.clone()
            self.depth_noise = depth_noise.to(dev).contiguous()
            self.ddim_noise = ddim_noise.to(dev).contiguous()
            self._tables = None                # (one row per step row: re-allocated with them)
        else:
            self.steps.copy_(steps_table)
            self.depth_noise.copy_(depth_noise)
            self.ddim_noise.copy_(ddim_noise)
        self.steps_nodiv.copy_(self.steps)
        self.steps_nodiv[:, 1] = 1.0
        self.steps_scene_stride = scene_stride
        self._tab_sig = None
        self.n_rows = int(steps_table.shape[0]) - (self.N - 1) * scene_stride      # the kernels index steps[iter + n * stride] unchecked
        self.rewind()

    def set_pin(self, mode, known, noise=None):
        """Pin the first K = len(known) / N views of every scene (after set_schedule: the noise has one row per step-table row).  The
        buffers are static inputs of the captured graphs: a change of shape re-allocates them and clears the graphs, like _set_tables.
        Engines are cached per signature, so callers reset with clear_pin() in a `finally`."""
        dev = self.ctx.device
        nk = int(known.shape[0])
        K = nk // self.N
        if mode not in (0, 1) or K < 1 or K * self.N != nk or K > self.V or tuple(known.shape[1:]) != (5, self.S, self.S):
            raise ValueError(f"StepEngine.set_pin: mode {mode}, known {tuple(known.shape)} for {self.N} scene(s) of {self.V} views at "
                             f"S = {self.S} (expected (N*K, 5, S, S), 1 <= K <= V)")
        if mode == 1 and (noise is None or tuple(noise.shape) != (int(self.steps.shape[0]), nk, 5, self.S, self.S)):
            raise ValueError(f"StepEngine.set_pin: mode 1 needs noise ({int(self.steps.shape[0])}, {nk}, 5, {self.S}, {self.S}), got "
                             f"{None if noise is None else tuple(noise.shape)}")
        if self.known.shape != known.shape:
            self.graphs.clear()
            self.prefetchers.clear()
            self.known = known.to(dev, torch.float32).contiguous().clone()
        else:
            self.known.copy_(known)
        if mode == 1:
            if self.pin_noise is None or self.pin_noise.shape != noise.shape:
                self.graphs.clear()
                self.prefetchers.clear()
                self.pin_noise = noise.to(dev, torch.float32).contiguous().clone()
            else:
                self.pin_noise.copy_(noise)
        self.pin = (int(mode), K)

    def clear_pin(self):
        self.pin = None

    def rewind(self, it=0):
        """Reset the device iteration counter (and its host mirror) to row `it` of the step table."""
        assert 0 <= it < self.n_rows
        self.iter.fill_(it)
        self.done = it

    def depth_geo(self):
        """(depth source (N*V,5,S,S), step table) GridAttn's kernels read the depth channel and its std from (see depth_mode)."""
        if self.depth_mode == 0:
            return self.x, self.steps
        return (self.x0 if self.depth_mode == 1 else self.prev), self.steps_nodiv

    # -- one iteration -------------------------------------------------------------------------------
    def enqueue(self, cfg_scale, do_update, prefetcher=None):
        m, ctx, L = self.m, self.ctx, hip.lib()
        V, S, D, B, q0, Vq, N = self.V, self.S, self.D, self.B, self.q0, self.Vq, self.N
        NVq = N * Vq                   # conditional rows of the UNet batch (q0 = 0, Vq = V when N > 1)
        ctx.B, ctx.D = B, D
        ctx.begin_step()           # eager warm-up and graph capture walk the same rotating buffers
        st = hip.stream
        sst, R = self.steps_scene_stride, self.t_rows
        if sst and do_update:
            raise ValueError("StepEngine: per-scene timesteps (set_schedule_scenes) are a training step: no DDIM update")
        if self.pin is not None:   # pinned views first: GridAttn and the UNet input below read the rewritten rows
            mode, K = self.pin
            pn = self.pin_noise if mode == 1 else None
            hip.check(L.mvd_pin_views(hip.ptr(self.x), hip.ptr(self.x0), hip.ptr(self.known), hip.ptr(pn), N * K * 5 * S * S,
                                      hip.ptr(self.steps), hip.ptr(self.iter), N, V, K, S, mode, st()))
        # embed_time (:276-279): sinusoid(256) -> Linear -> SiLU -> Linear; only row 0 is used downstream (t[:1]) -- one row per scene
        # when every scene has its own timestep
        unet = m.unet_model.unet_model
        tabs = self.vectors_valid()    # per-sample vectors: this step only picks its row (refresh_vectors computed them)
        c = ctx.ws.get("vf.c", (R, 256))
        if tabs:
            T = self._tables
            emb, bias = unet.time_bias_buffers(ctx, 1)
            hip.check(L.mvd_select_step_rows(hip.ptr(self.iter), int(T["c"].shape[0]), hip.ptr(T["c"]), hip.ptr(c), 256, hip.ptr(T["emb"]),
                                             hip.ptr(emb), emb.shape[1], hip.ptr(T["bias"]), hip.ptr(bias), bias.shape[1], st()))
        else:
            ts = ctx.ws.get("vf.tsin", (R, 256))
            te1 = ctx.ws.get("vf.te1", (R, 256))
            hip.check(L.mvd_timestep_embedding_scenes(hip.ptr(self.steps), hip.ptr(self.iter), hip.ptr(self.f256), hip.ptr(ts), 256, R, sst,
                                                      st()))
            ctx.gemv_rows(m.time_embed[0].weight, m.time_embed[0].bias, ts, te1, act_out=hip.ACT_SILU)
            ctx.gemv_rows(m.time_embed[2].weight, m.time_embed[2].bias, te1, c)
        # view-aligned features (:303-313)
        dsrc, dsteps = self.depth_geo()
        m.view_attn.run(ctx, self.x, self.depth_noise, self.steps, self.iter, self.cams, self.in_cam,
                        self.input_latents, c, self.vol, V, S, D, q0=q0, Vq=Vq, vol_planes=self.vol_planes,
                        vol_planes_col=self.vol_col, depth_src=None if self.depth_mode == 0 else dsrc,
                        depth_steps=None if self.depth_mode == 0 else dsteps, scenes=N, steps_scene_stride=sst)
        # cc_projection (:322)
        if not tabs:
            p = m.cc_projection
            c1 = ctx.ws.get("vf.cc1", (NVq, 768))
            c2 = ctx.ws.get("vf.cc2", (NVq, 768))
            ctx.gemv_rows(p[0].weight, p[0].bias, self.clip_v_embed[q0:q0 + NVq], c1, act_out=hip.ACT_SILU)
            ctx.gemv_rows(p[2].weight, p[2].bias, c1, c2, act_out=hip.ACT_SILU)
            ctx.gemv_rows(p[4].weight, p[4].bias, c2, self.context[:NVq])
        if self.drop_masks is not None:        # UNetWrapper.forward(is_train=True) condition dropout (eager only, never captured)
            clip_m, vol_m, cat_m = self.drop_masks          # (N*Vq,) each, scene-major
            self.context[:NVq] *= clip_m[:, None]
            self.vol.view(B, -1)[:NVq] *= vol_m[:, None]
            vp = self.vol_planes.view(B, S * S * D, -1)
            vp[:NVq, :, 2 * self.vol_col:] *= vol_m.to(torch.int16)[:, None, None]        # x * {0, 1} keeps / zeroes the planes
        ctx.context = self.context
        # UNet on the CFG batch (unet.py:167-196)
        xq, x0q, epsq = self.x[q0:q0 + NVq], self.x0[q0:q0 + NVq], self.eps[q0:q0 + NVq]
        hip.check(L.mvd_unet_input_scenes(hip.ptr(xq), hip.ptr(self.input_latents), hip.ptr(self.x_in), N, Vq, S, 32,
                                          int(self.cfg), st()))
        if self.drop_masks is not None:        # x_concat channels 5..9 of the (rows, [32 hi | 32 lo]) input planes
            xin = self.x_in.view(B, S * S, 64)
            cm = self.drop_masks[2].to(torch.int16)[:, None, None]
            xin[:NVq, :, 5:10] *= cm
            xin[:NVq, :, 37:42] *= cm
        ctx.vol_levels = m.unet_model.volume_pyramid(ctx, self.vol.view(B, S, S, D, 768), B, S, D)
        tsu = None                     # (with the per-sample vectors temb.bias and xattn.vec are filled already)
        if not tabs:
            tsu = ctx.ws.get("vf.tsin_unet", (R, unet.model_channels))
            hip.check(L.mvd_timestep_embedding_scenes(hip.ptr(self.steps), hip.ptr(self.iter), hip.ptr(self.funet), hip.ptr(tsu),
                                                      unet.model_channels, R, sst, st()))
        y = unet.run(ctx, self.x_in, tsu, S)
        hip.check(L.mvd_cfg_ddim_update(hip.ptr(y), 8, hip.ptr(xq), hip.ptr(x0q), hip.ptr(epsq),
                                        hip.ptr(self.ddim_noise[:, q0:q0 + NVq]), N * V * 5 * S * S, hip.ptr(self.steps),
                                        hip.ptr(self.iter), NVq, S, int(self.cfg), float(cfg_scale), int(do_update), st()))
        if do_update:
            hip.check(L.mvd_advance_iter(hip.ptr(self.iter), st()))

    @property
    def t_rows(self):
        """Rows of the time conditioning (vf.tsin / vf.c / temb.emb ...): N with per-scene timesteps, else 1."""
        return self.N if self.steps_scene_stride else 1

    def step(self, cfg_scale, do_update, use_graph=True):
        tabs = self.tables_apply()
        key = (float(cfg_scale), bool(do_update), int(self.depth_mode), self.steps_scene_stride, self.pin, tabs)
        if self.done >= self.n_rows:
            raise IndexError(f"StepEngine.step: iteration {self.done} is past the {self.n_rows}-row step table "
                             "(set_schedule() / rewind() before stepping again)")
        if do_update:
            self.done += 1
        if not use_graph:              # (an eager step reads the per-sample vectors while they are valid, else computes them in place)
            return self.enqueue(cfg_scale, do_update)
        if tabs:                       # a graph is captured and replayed with valid vectors only: it holds no launch that computes them
            self.refresh_vectors()
        g = self.graphs.get(key)
        if g is None:
            # first call runs eagerly (allocates every workspace buffer, packs weights), then capture
            it0 = self.iter.clone()
            x_keep, x0_keep = self.x.clone(), self.x0.clone()      # (x0: the previous step's estimate is an INPUT under feed_prev_depth;
                                                                   #  pinned rows need nothing more: every pass rewrites them from static inputs)
            hip.AUTOTUNE = True            # pick the GEMM kernel configuration per problem shape (cached)
            try:
                self.enqueue(cfg_scale, do_update)
            finally:
                hip.AUTOTUNE = False
                hip.release_tuning_buffers()
            torch.cuda.synchronize()
            # weight prefetch (include/mvd_hip.h: mvd_gemm_desc.pf_items): a second eager pass with the tuned configurations records the
            # step's GEMM launch order; at capture every role-split launch is handed the weights of the launches behind it
            pf = None
            if PREFETCH_WEIGHTS == "ws":
                pf = hip.WeightPrefetcher(self.x.device, **PREFETCH_OPTIONS)
                self.iter.copy_(it0)
                self.x.copy_(x_keep)
                self.x0.copy_(x0_keep)
                with pf.following(record=True):
                    self.enqueue(cfg_scale, do_update)
                torch.cuda.synchronize()
            self.iter.copy_(it0)
            self.x.copy_(x_keep)
            self.x0.copy_(x0_keep)
            g = hip.Graph()
            self.ctx.ws.frozen = True      # capture must not allocate: every buffer exists after the eager step
            try:
                with g:
                    if pf is None:
                        self.enqueue(cfg_scale, do_update)
                    else:
                        with pf.following():
                            self.enqueue(cfg_scale, do_update, prefetcher=pf)
            finally:
                self.ctx.ws.frozen = False
            self.graphs[key] = g
            self.prefetchers[key] = pf
        g.launch()


class _HipTrainingLoss(torch.autograd.Function):
    """Bridges ViewFusion.gradients (forward + hand-written backward kernels) into torch autograd: forward computes the loss AND the
    parameter gradients (the HIP buffers of the step are only valid until the next step), backward scales and returns them."""

    @staticmethod
    def forward(ctx, model, batch, trainer_config, names, *params):
        loss, grads = model.gradients(batch, trainer_config, noise_source=getattr(model, "_noise_source", None), only_trainable=True)
        # (batch: one dict, or a list of them = one multi-scene step: gradients_scenes)
        ctx.grads = [grads.get(n) for n in names]
        ctx.shapes = [p.shape for p in params]
        return loss.clone()

    @staticmethod
    def backward(ctx, grad_out):
        # the gradients are this step's own buffers: scale them in place with multi-tensor launches (994 separate multiplies were 15 ms).
        #  in place is only safe ONCE and only over disjoint buffers: a second backward over the same node (retain_graph=True)
        # must not scale again, and two gradients that overlap without being the same view take the out-of-place path.
        if getattr(ctx, "_scaled", False):
            raise RuntimeError("_HipTrainingLoss.backward ran twice on one node: the step's gradient buffers were already scaled in place "
                               "(call model(batch, cfg) again instead of retain_graph=True)")
        ctx._scaled = True
        live, seen, spans = [], set(), []
        for g in ctx.grads:
            if g is None:
                continue
            key = (g.untyped_storage().data_ptr(), g.storage_offset(), tuple(g.shape), tuple(g.stride()))
            if key in seen:                                      # (a buffer shared by two names is scaled once)
                continue
            seen.add(key)
            live.append(g)
            spans.append((g.data_ptr(), g.data_ptr() + g.numel() * g.element_size()) if g.is_contiguous() else None)
        disjoint = all(sp is not None for sp in spans)
        if disjoint:
            srt = sorted(spans)
            disjoint = all(srt[i][1] <= srt[i + 1][0] for i in range(len(srt) - 1))
        if live and disjoint:
            torch._foreach_mul_(live, grad_out.to(live[0].dtype))
            pick = lambda g: g
        else:                                                     # overlapping / strided views: the safe out-of-place multiply per name
            pick = lambda g: g * grad_out.to(g.dtype)
        outs = [torch.zeros(s, dtype=grad_out.dtype, device=grad_out.device) if g is None else pick(g).reshape(s)
                for g, s in zip(ctx.grads, ctx.shapes)]
        return (None, None, None, None, *outs)


class ViewFusion(nn.Module):
    def __init__(self, view_attn_config, unet_config, ddpm_config, vae_config=None, unet_path="", vae_path="",
                 clip_path="", unet_cc_path="", z_scale_factor=0.18215, vae_max_batch=8, objective="noise",
                 loss_type="l2", embed_camera_pose=True, finetune_projection=False, finetune_unet=False,
                 finetune_cross_attn=True, finetune_view_attn=True, feed_prev_depth=False, drop_conditions=False,
                 vae=None, clip_image_encoder=None, precision=None, reference_eval_dropout=False, overwrite_x_noisy=False, **kwargs):
        super().__init__()
        assert embed_camera_pose, "this build implements the embed_camera_pose=True configuration of configs/*.yaml"
        self.finetune_projection, self.finetune_unet, self.z_scale_factor = finetune_projection, finetune_unet, z_scale_factor
        self.vae_max_batch, self.objective, self.loss_type = vae_max_batch, objective, loss_type
        self.embed_camera_pose, self.finetune_cross_attn, self.finetune_view_attn = \
            embed_camera_pose, finetune_cross_attn, finetune_view_attn
        self.feed_prev_depth, self.drop_conditions = feed_prev_depth, drop_conditions
        # The reference applies the condition dropout whenever cfg_scale == 1 (is_train=True is hard-wired at :322-330 / unet.py:140),
        # i.e. also under model.eval() (validation losses, cfg = 1 sampling).  Default here: only in training mode; True reproduces the
        # reference's eval-mode behaviour bit for bit in distribution (validation curves comparable 1:1).
        self.reference_eval_dropout = bool(reference_eval_dropout)
        # precision = MFMA operand type x number of partial products of the (hi+lo)(hi+lo) operand split:
        # "f16x3" (default, configs.DEFAULT_PRECISION: fp16 hi + lo, lo*lo dropped, ~2^-22), "f16x4" (all 4 products; +5 - 7 % time, no
        # measurable accuracy difference: DESIGN.md section 4), "bf16x3" (~2^-16), "f16" / "bf16" (one product, hi only).  The operand type selects the library
        # flavour and is fixed per process.
        # A policy string "f16x4:conv=3,geglu=3" sets the products per layer class (hip.PREC_KINDS).
        from .configs import DEFAULT_PRECISION
        precision = precision or DEFAULT_PRECISION
        fmt, self.precision, self.precision_policy = hip.parse_precision(precision)
        hip.set_operand_format(fmt)
        self.precision_name = precision

        def params(cfg):
            return dict(cfg.get("params", cfg)) if hasattr(cfg, "get") else dict(cfg)

        self.view_attn = GridAttn(**params(view_attn_config))
        self.unet_model = UNetWrapper(unet_config, unet_path=unet_path or None, drop_conditions=drop_conditions,
                                      drop_scheme="default", finetune_unet=finetune_unet,
                                      finetune_cross_attn=finetune_cross_attn, finetune_view_attn=finetune_view_attn,
                                      use_zero_123=True,
                                      remove_keys=["input_blocks.0.0.weight", "out.2.weight", "out.2.bias"])
        self.scheduler = DDPMScheduler(**params(ddpm_config))
        # VAE: `vae_config` (configs/*.yaml: external.sd1.ldm.models.autoencoder.AutoencoderKL) builds the HIP-backed decode
        # mirror (mvdfusion_amd/autoencoder.py; its encode needs an injected module); an injected `vae` takes precedence.
        if vae is not None:
            self.vae = vae
        elif vae_config is not None:
            from .load_model import instantiate_from_config
            self.vae = instantiate_from_config(vae_config)
            if vae_path:
                sd = torch.load(vae_path, map_location="cpu")
                sd = sd.get("state_dict", sd)
                self.vae.load_state_dict({k.replace("first_stage_model.", ""): v for k, v in sd.items()}, strict=False)
        # CLIP image encoder (viewfusion_zero_depth_rgb.py:103-105: FrozenCLIPImageEmbedder(model=clip_path), frozen): an injected
        # module takes precedence; otherwise `clip_path` (the CLIP model name of configs/*.yaml, e.g. "ViT-L/14") builds the
        # HIP-backed mirror, whose weights come with the checkpoint's clip_image_encoder.* keys.
        if clip_image_encoder is not None:
            self.clip_image_encoder = clip_image_encoder
        elif clip_path:
            from .encoders import FrozenCLIPImageEmbedder
            self.clip_image_encoder = FrozenCLIPImageEmbedder(model=clip_path, precision=precision)
            for prm in self.clip_image_encoder.parameters():
                prm.requires_grad_(False)
        self.cc_projection = nn.Sequential(nn.Linear(768 + 14 * 2, 768), nn.SiLU(True), nn.Linear(768, 768),
                                           nn.SiLU(True), nn.Linear(768, 768))
        nn.init.eye_(list(self.cc_projection.parameters())[0][:768, :768])
        nn.init.zeros_(list(self.cc_projection.parameters())[1])
        self.time_embed_dim = 256
        self.time_embed = nn.Sequential(nn.Linear(256, 256), nn.SiLU(True), nn.Linear(256, 256))
        self.register_buffer("_device", torch.tensor([0.0]), persistent=False)
        self.latent_size = int(self.view_attn.input_size)
        self.ddim = DDIMSampler(self, ddim_num_steps=50, ddim_discretize="uniform", ddim_eta=1.0,
                                latent_size=self.latent_size, z_dim=4, feed_prev_depth=feed_prev_depth,
                                overwrite_x_noisy=overwrite_x_noisy)      # (the sampler's switch, sampler.py:14; reachable from a config here)
        self._engines = {}
        self._packed_sig = None
        assert self.finetune_view_attn is True, "must finetune new view attention layers"

    # ------------------------------------------------------------------------------------------------
    train_autotune_min_flops = 2.0e9      # training step: GEMMs at least this large are autotuned on first sight (None: heuristic tiles only)

    def invalidate_packed(self, keep_engines=False):
        """Drop every packed weight image, captured graph and engine: they are rebuilt from the live fp32 parameters.
        keep_engines: the parameters changed IN PLACE (an optimizer step): the engines' static arenas (activations, split-K slabs,
        statistics slots -- GBs of buffers) stay, only the packed images and the graphs that captured their addresses go."""
        hip.drop_packed_caches(self)
        hip.forget_param_maxima()          # (engine() measures them again before anything is packed for a step)
        if keep_engines:
            for e in self._engines.values():
                e.invalidate()
        else:
            self._engines.clear()

    def load_state_dict(self, state_dict, strict=True, **kw):
        """nn.Module.load_state_dict, then drop every derived packed weight / engine / graph (demo.py:165, train.py:144-153)."""
        r = super().load_state_dict(state_dict, strict=strict, **kw)
        self.invalidate_packed()
        self._packed_sig = None
        return r

    def _apply(self, fn, *a, **kw):
        """.cuda() / .to() / .float(): parameters move, so every derived packed image is stale."""
        r = super()._apply(fn, *a, **kw)
        if "_engines" in self.__dict__:
            self.invalidate_packed()
            self._packed_sig = None
        return r

    def engine(self, V, S, D, cfg, q0=0, Vq=None, scenes=1):
        """The StepEngine of one (V, S, D, cfg, view range, scenes) signature (created on first use, then reused).  scenes = N objects
        denoised together in every step (scene-major buffers, see StepEngine); view-parallel sharding (q0 / Vq) is single-scene only.
        Engines are kept until invalidate_packed(): each distinct N holds its own workspace, graphs and tuned GEMM shapes.
        GridAttn's window (view_attn.keep_top_k_views / top_k) is, like n_pts_per_ray, a construction-time property of the model: an
        engine's GridAttn buffers and captured graphs are sized by the W rows per 3-D point it had when the engine first ran, so
        flipping it on a live model needs invalidate_packed()."""
        if int(scenes) < 1:
            raise ValueError(f"engine(scenes={scenes}): at least one scene")
        if int(scenes) > 1 and (q0 != 0 or (Vq is not None and Vq != V)):
            raise ValueError(f"engine(V={V}, q0={q0}, Vq={Vq}, scenes={scenes}): view-parallel sharding is single-scene only")
        sig = hip.params_signature(self)
        if sig != self._packed_sig:      # an in-place update (optimizer step, fill_) since the weights were packed; load_state_dict /
            if self._packed_sig is not None:      # .cuda() invalidate fully themselves (the device may have changed)
                dev_now = self._device.device
                same_dev = all(e.ctx.device == dev_now for e in self._engines.values())
                self.invalidate_packed(keep_engines=same_dev)
            self._packed_sig = sig
            hip.register_param_maxima(self.parameters())      # one reduction + one host read instead of one per packed weight
        if Vq is not None and Vq <= 0:
            raise ValueError(f"engine(V={V}, q0={q0}, Vq={Vq}): a rank must own at least one query view")
        key = (V, S, D, bool(cfg), q0, Vq) if int(scenes) == 1 else (V, S, D, bool(cfg), q0, Vq, int(scenes))
        e = self._engines.get(key)
        if e is None:
            dev = self._device.device
            if dev.type != "cuda":
                raise RuntimeError("mvdfusion_amd.ViewFusion runs on the GPU only (model.cuda() first); "
                                   "there is no CPU path in the product")
            e = StepEngine(self, V, S, D, cfg, dev, self.precision, q0=q0, Vq=Vq, policy=self.precision_policy, scenes=int(scenes))
            self._engines[key] = e
        return e

    def _print_parameter_count(self):
        va = sum(p.numel() for p in self.view_attn.parameters())
        un = sum(p.numel() for p in self.unet_model.get_trainable_parameters())
        uf = sum(p.numel() for p in self.unet_model.parameters())
        tp = sum(p.numel() for p in self.time_embed.parameters())
        pp = sum(p.numel() for p in self.cc_projection.parameters()) if self.finetune_projection else 0
        print(f"view_attn {va * 1e-6:.2f}M | unet trainable {un * 1e-6:.2f}M / full {uf * 1e-6:.2f}M | "
              f"total trainable {(va + un + tp + pp) * 1e-6:.2f}M / full {(va + uf + tp + pp) * 1e-6:.2f}M")

    @torch.no_grad()
    def encode_clip(self, x):
        return self.clip_image_encoder.encode(x)

    @torch.no_grad()
    def encode(self, x):
        return self.vae.encode(torch.clip(x * 2 - 1.0, -1.0, 1.0)).mode() * self.z_scale_factor

    @torch.no_grad()
    def decode(self, z):
        return torch.clip((self.vae.decode(z * 1 / self.z_scale_factor) + 1.0) / 2.0, 0.0, 1.0).clip(0.0, 1.0)

    def prepare_batch(self, batch, trainer_config, generator=None):
        """viewfusion_zero_depth_rgb.py:165-273 (host-side; needs the plugged-in VAE / CLIP encoders)."""
        images = batch["images"]
        dev = images.device
        Bn, _, H, W = images.shape
        n_in, n_tr = trainer_config["input_batch_size"], trainer_config["train_batch_size"]
        if trainer_config["random_views"]:
            rand = torch.randperm(Bn, generator=generator) if generator is not None else torch.randperm(Bn)
        else:
            rand = torch.linspace(0, Bn - 1, n_in + n_tr).long()
        in_idx, b_idx = rand[:n_in], rand[n_in:n_in + n_tr]
        input_latents = self.encode(images[in_idx])
        batch_latents = self.encode(images[b_idx])
        area = lambda d: torch.nn.functional.interpolate(d, scale_factor=0.125, mode="area")
        in_depth = torch.zeros_like(area(torch.zeros((n_in, 1, H, W), device=dev)))      # input depth forced to 0 (:215)
        input_latents = torch.cat((input_latents, in_depth), dim=1)
        if "depths" in batch:
            b_depth = torch.clip(batch["depths"][b_idx].to(dev) * 2 - 1.0, -1.0, 1.0)
        else:
            b_depth = torch.zeros((n_tr, 1, H, W), device=dev)
        batch_latents = torch.cat((batch_latents, area(b_depth)), dim=1)
        cams = get_relative_camera(Cameras(batch["R"].float().cpu(), batch["T"].float().cpu(),
                                           batch["f"].float().cpu(), batch["c"].float().cpu()), in_idx)
        input_cameras, batch_cameras = get_camera_slice(cams, in_idx), get_camera_slice(cams, b_idx)
        clip_embed = self.encode_clip(images[in_idx]).expand(n_tr, -1, -1)
        from .synthetic import cam_embed
        clip_v_embed = torch.cat((clip_embed, cam_embed(input_cameras, batch_cameras).to(dev)), dim=-1)
        return batch_latents, batch_cameras, input_latents, input_cameras, clip_v_embed

    def embed_time(self, t):
        """(B,) int timesteps -> (B, 256).  Runs the same GEMV kernels as the step engine."""
        dev = self._device.device
        e = torch.cat([torch.cos(t[:, None].float() * self._f256(dev)), torch.sin(t[:, None].float() * self._f256(dev))], -1)
        h = torch.empty(t.shape[0], 256, device=dev)
        out = torch.empty(t.shape[0], 256, device=dev)
        for r in range(0, t.shape[0], 16):
            hip.gemv(self.time_embed[0].weight, self.time_embed[0].bias, e[r:r + 16].contiguous(), h[r:r + 16], act_out=hip.ACT_SILU)
            hip.gemv(self.time_embed[2].weight, self.time_embed[2].bias, h[r:r + 16], out[r:r + 16])
        return out

    def _f256(self, dev):
        if not hasattr(self, "_f256_cache") or self._f256_cache.device != dev:
            self._f256_cache = _sinusoid_freqs(256).to(dev)
        return self._f256_cache[None]

    @torch.no_grad()
    def apply_model(self, noisy_latents, batch_cameras, input_latents, input_cameras, clip_v_embed, t, prev_depth=None,
                    cfg_scale=1.0, depth_noise=None, drop_rand=None):
        """viewfusion_zero_depth_rgb.py:282-345.  ``depth_noise`` (V,D,S,S) optionally injects the N(0,1) draw that
        the reference takes inside GridAttn (view_attn_efficient2.py:431); default: torch's device generator.
        With cfg_scale == 1 the reference calls UNetWrapper.forward(is_train=True): when the model was built with
        drop_conditions=True and is in training mode, the per-view condition dropout of unet.py:109-151 is applied
        (``drop_rand`` (V,) optionally injects its torch.rand draw)."""
        V, _, S, _ = noisy_latents.shape
        if depth_noise is None:
            depth_noise = torch.randn(V, self.view_attn.n_pts_per_ray, S, S, device=noisy_latents.device)
        return self._step_scenes(noisy_latents, [(batch_cameras, input_latents, input_cameras, clip_v_embed)], [int(t[0])],
                                 None if prev_depth is None else [prev_depth], depth_noise, drop_rand, cfg_scale)

    def _step_scenes(self, noisy, conds, ts, prev_depth, depth_noise, drop_rand, cfg_scale=1.0):
        """One denoising step of N scenes on the N-scene engine, without the DDIM update: noisy (N*V, 5, S, S) scene-major, conds one
        (batch_cameras, input_latents, input_cameras, clip_v_embed) per scene, ts one timestep per scene (one in all for a guided step),
        prev_depth None or one (V or 1, 1, S, S) overwrite_attn_depth map per scene, depth_noise (N*V, D, S, S), drop_rand None (drawn
        here when the condition dropout applies) or (N*V,).  Returns eps (N*V, 5, S, S)."""
        N = len(conds)
        NV, _, S, _ = noisy.shape
        V = NV // N
        D = self.view_attn.n_pts_per_ray
        cfg = cfg_scale != 1.0
        eng = self.engine(V, S, D, cfg, scenes=N)
        eng.set_conditioning_scenes(conds)
        rows = []
        for tv in ts:
            sac = self.scheduler.sqrt_alphas_cumprod[tv]
            dstd = self.scheduler.sqrt_one_minus_alphas_cumprod[tv] / sac / 10.0
            rows.append([float(tv), float(sac), float(dstd), 1.0, 1.0, 0.0, 0.0, 0.0])
        table = torch.tensor(rows, dtype=torch.float32)
        if cfg:                                # (a guided step shares one timestep)
            eng.set_schedule(table, depth_noise.reshape(1, NV, D, S, S), torch.zeros(1, NV, 5, S, S))
        else:
            eng.set_schedule_scenes(table, depth_noise.reshape(1, NV, D, S, S))
        eng.x.copy_(noisy)
        eng.depth_mode = 0
        if prev_depth is not None:             # overwrite_attn_depth (:312; view_attn_efficient2.py:418-426)
            for n, pd in enumerate(prev_depth):
                eng.prev[n * V:(n + 1) * V, 4:5].copy_(pd.to(eng.prev.device).expand(V, 1, S, S))
            eng.depth_mode = 2
        eng.drop_masks = None
        if not cfg and self.drop_conditions and (self.training or self.reference_eval_dropout):
            r = torch.rand(NV, device=noisy.device) if drop_rand is None else drop_rand.to(noisy.device).float()
            drop_clip, drop_vol = (r > 0.15) & (r <= 0.2), (r > 0.1) & (r <= 0.15)          # get_drop_scheme 'default' (unet.py:109-117)
            drop_cat, drop_all = (r > 0.05) & (r <= 0.1), r <= 0.05
            eng.drop_masks = tuple(1.0 - (dm | drop_all).float() for dm in (drop_clip, drop_vol, drop_cat))
        self._last_drop_masks = eng.drop_masks
        self._train_engine = eng
        keep = eng.ctx.keep_fp32
        eng.ctx.keep_fp32 = keep or bool(getattr(self, "_train_keep_fp32", False))      # this engine only (never a class-wide switch)
        try:
            eng.step(cfg_scale, do_update=False, use_graph=eng.drop_masks is None and not getattr(self, "_force_eager", False))
        finally:
            eng.ctx.keep_fp32 = keep
            eng.drop_masks = None      # (depth_mode stays: the training backward re-derives the geometry from the same depth source)
        return hip.check_finite(eng.eps.clone(), "ViewFusion.apply_model")

    def sample(self, batch, trainer_config, cfg_scale, return_input=False, depth=False, verbose=True):
        """viewfusion_zero_depth_rgb.py:348-359."""
        batch_latents, batch_cameras, input_latents, input_cameras, clip_v_embed = self.prepare_batch(batch, trainer_config)
        res = self.ddim.sample(batch_cameras, input_latents, input_cameras, clip_v_embed, unconditional_scale=cfg_scale, depth=depth,
                               return_intermediates=return_input, verbose=verbose)
        return (res[0], batch_latents, input_latents, batch_cameras, res[1]) if return_input else res

    def sample_scenes(self, batches, trainer_config, cfg_scale, return_input=False, depth=False, verbose=True):
        """``sample`` for several objects at once: every DDIM step denoises all of them in one batched step (DDIMSampler.sample_scenes;
        the scenes share V, S, cfg_scale and the schedule).  Returns a list with what ``sample`` returns for each batch, in order."""
        prepared = [self.prepare_batch(b, trainer_config) for b in batches]
        conds = [(bc, il, ic, ce) for _, bc, il, ic, ce in prepared]
        res = self.ddim.sample_scenes(conds, unconditional_scale=cfg_scale, depth=depth, return_intermediates=return_input,
                                      verbose=verbose)
        if not return_input:
            return [res[n] for n in range(len(batches))]
        x, inter = res
        out = []
        for n, (batch_latents, batch_cameras, input_latents, _, _) in enumerate(prepared):
            its = [{"t": it["t"], "xt": it["xt"][n], "x0": it["x0"][n]} for it in inter]
            out.append((x[n], batch_latents, input_latents, batch_cameras, its))
        return out

    def sample_rig(self, batch, trainer_config, cfg_scale, chunk_views, anchors_per_chunk=1, anchors=None, return_input=False, depth=False,
                   verbose=True):
        """``sample`` for a rig of M = trainer_config["train_batch_size"] views, more than one step holds: prepare_batch once for the
        whole rig, then DDIMSampler.sample_rig generates it in chunks of ``chunk_views`` views, each later chunk with ``anchors_per_chunk``
        already-generated views held fixed.  Returns what ``sample`` returns (no intermediates: the chunks have their own loops)."""
        batch_latents, batch_cameras, input_latents, input_cameras, clip_v_embed = self.prepare_batch(batch, trainer_config)
        x = self.ddim.sample_rig(batch_cameras, input_latents, input_cameras, clip_v_embed, unconditional_scale=cfg_scale,
                                 chunk_views=chunk_views, anchors_per_chunk=anchors_per_chunk, anchors=anchors, depth=depth, verbose=verbose)
        return (x, batch_latents, input_latents, batch_cameras, []) if return_input else x

    @torch.no_grad()
    def fuse(self, latents, batch_cameras, up=8, decode=True, **kw):
        """The call after ``sample`` / ``sample_scenes`` / ``sample_rig``: the sampled views as one depth-consistent point cloud
        (fusion.fuse_views with this model's depth_scale / depth_shift).  latents (V, 5, S, S) with the batch cameras, or (N, V, 5, S, S)
        with a list of N camera sets.  decode: colour the points from ``self.decode(latents[:, :4])`` (8 S pixels per side, so up <= 8);
        otherwise pass ``rgb=`` or get an uncoloured cloud.  Other keywords: tau, min_support, max_conflicts, foreground."""
        from .fusion import fuse_views
        if decode:
            kw["rgb"] = self._decoded(latents)
        return fuse_views(latents, batch_cameras, up=up, depth_scale=self.view_attn.depth_scale, depth_shift=self.view_attn.depth_shift,
                          **kw)

    def _decoded(self, latents):
        """``self.decode`` of the four image channels of (.., 5, S, S) latents, with their leading dimensions."""
        S = latents.shape[-1]
        flat = latents.reshape(-1, 5, S, S)[:, :4]
        img = torch.cat([self.decode(c) for c in flat.split(self.vae_max_batch)]).float()
        return img.reshape(*latents.shape[:-3], 3, img.shape[-2], img.shape[-1])

    @torch.no_grad()
    def mesh(self, latents, batch_cameras, grid=128, up=8, decode=True, largest=None, min_faces=None, smooth=0, simplify=None, texture=None,
             **kw):
        """The sampled views as a closed triangle mesh with vertex colours: fusion.integrate_tsdf with this model's depth_scale /
        depth_shift, then fusion.extract_mesh.  latents and cameras as ``fuse`` takes them; decode: colour from ``self.decode``
        (8 S pixels per side, so up <= 8), otherwise pass ``rgb=`` or get an uncoloured mesh.  Other keywords: center, half_extent, trunc,
        carve, foreground (integrate_tsdf) and fill (extract_mesh).
        largest, min_faces: when either is given, fusion.keep_components drops the floaters of the extracted mesh; smooth: when > 0,
        fusion.smooth_mesh(iters=smooth) follows; simplify: when given, fusion.simplify_mesh(cells=simplify) comes last, after floater
        removal and smoothing.  With the defaults none is called and the mesh is extract_mesh's own.
        texture: when given, the finished mesh is textured from the same images with ``texels=texture`` (fusion.bake_texture's other
        defaults) and the return value is (mesh, MeshTexture); it needs colour (decode or ``rgb=``)."""
        from .fusion import bake_texture, extract_mesh, integrate_tsdf, keep_components, simplify_mesh, smooth_mesh
        if decode:
            kw["rgb"] = self._decoded(latents)
        if texture is not None and kw.get("rgb") is None:
            raise ValueError("texture: needs images -- decode=True or rgb=")
        fill = {"fill": kw.pop("fill")} if "fill" in kw else {}
        vol = integrate_tsdf(latents, batch_cameras, grid=grid, up=up, depth_scale=self.view_attn.depth_scale,
                             depth_shift=self.view_attn.depth_shift, **kw)
        mesh = extract_mesh(vol, **fill)
        if largest is not None or min_faces is not None:
            mesh = keep_components(mesh, largest=largest, min_faces=min_faces)
        if smooth:
            mesh = smooth_mesh(mesh, iters=smooth)
        if simplify is not None:
            mesh = simplify_mesh(mesh, cells=simplify)
        if texture is not None:
            return mesh, bake_texture(mesh, kw["rgb"], batch_cameras, texels=texture)
        return mesh

    @torch.no_grad()
    def texture(self, mesh, latents, batch_cameras, texels=8, decode=True, **kw):
        """A texture for a mesh of ``self.mesh`` from the sampled views (fusion.bake_texture): every texel of a per-face atlas takes
        its colour from the decoded views that see it.  latents and cameras as ``fuse`` takes them; decode: the images are
        ``self.decode(latents[:, :4])``, otherwise pass ``rgb=``.  Other keywords: depth, size, tolerance, min_cos, power, blend, cull,
        fill, znear.

            mesh = model.mesh(latents, batch_cameras, simplify=64)
            tex = model.texture(mesh, latents, batch_cameras)           # tex.image (3, A, A), tex.views, tex.coverage()
            views = model.render_mesh(mesh, batch_cameras, texture=tex)
            fusion.write_obj("object.obj", mesh, tex)
        """
        from .fusion import bake_texture
        rgb = self._decoded(latents) if decode else kw.pop("rgb", None)
        if rgb is None:
            raise ValueError("texture: needs images -- decode=True or rgb=")
        return bake_texture(mesh, rgb, batch_cameras, texels=texels, **kw)

    @torch.no_grad()
    def render(self, cloud, cameras, size=256, radius=1, **kw):
        """A fused cloud seen from any cameras (fusion.render_points; ``depth_latent`` of the result defaults to this model's depth_scale /
        depth_shift).  cameras: M cameras, or a list of N sets of M for an N-scene cloud.  Other keywords: background, znear, empty_depth.

            cloud = model.fuse(latents, batch_cameras)
            views = model.render(cloud, batch_cameras, size=256)      # views.rgb (V, 3, 256, 256), views.depth, views.index, views.hit
            lat4 = views.depth_latent()                                # the depth the whole rig implies for each view, as a depth channel
        """
        from .fusion import render_points
        out = render_points(cloud, cameras, size=size, radius=radius, **kw)
        out._depth_map = (float(self.view_attn.depth_scale), float(self.view_attn.depth_shift))
        return out

    @torch.no_grad()
    def render_mesh(self, mesh, cameras, size=256, **kw):
        """A mesh of ``self.mesh`` seen from any cameras (fusion.render_mesh; ``depth_latent`` of the result defaults to this model's
        depth_scale / depth_shift).  cameras: M cameras, or a list of N sets of M for an N-scene mesh.  Other keywords: cull, background,
        znear, empty_depth.

            mesh = model.mesh(latents, batch_cameras)
            views = model.render_mesh(mesh, batch_cameras, size=256)   # views.rgb (V, 3, 256, 256), views.depth, views.face, views.normal
            lat4 = views.depth_latent()                                # the depth the surface implies for each view, as a depth channel
            grey = views.shaded()                                      # a headlight image (the way to look at a mesh made with decode=False)
        """
        from .fusion import render_mesh
        out = render_mesh(mesh, cameras, size=size, **kw)
        out._depth_map = (float(self.view_attn.depth_scale), float(self.view_attn.depth_shift))
        return out

    @torch.no_grad()
    def compare(self, latents, target_latents, decode=True, rgb=None, target_rgb=None, foreground=(0.02, 0.98), align="none", **kw):
        """Score sampled views against ground-truth views (view_metrics.compare_images, compare_depth) -> (ImageMetrics or None,
        DepthMetrics), each with the latents' leading dimensions.  latents, target_latents: (.., 5, S, S) of one shape.
        decode: the images are ``self.decode`` of both stacks' four image channels (8 S pixels per side); otherwise pass ``rgb=`` and
        ``target_rgb=`` (.., 3, H, W), or neither to score the depth alone.  The depth maps are the depth channels as ``fuse`` reads
        them -- clamp((lat4 + 1) / 2, 0, 1) * depth_scale + depth_shift with this model's values -- scored where the TARGET's depth channel
        is foreground (``fuse_views``' rule).  Depth at S and images at their own size: nothing is resampled, and the images are
        scored unmasked.  align: as ``compare_depth`` takes it.  Other keywords go to ``compare_images``.

            images, depth = model.compare(latents, batch_latents)      # images.psnr (V,), images.ssim, depth.abs_rel, depth.delta1
        """
        from .view_metrics import compare_depth, compare_images, latent_depth
        if not torch.is_tensor(latents) or not torch.is_tensor(target_latents) or latents.shape != target_latents.shape:
            raise ValueError("compare: latents and target_latents must be tensors of one shape (.., 5, S, S)")
        scale, shift = float(self.view_attn.depth_scale), float(self.view_attn.depth_shift)
        depth, _ = latent_depth(latents, scale, shift, foreground)
        target_depth, valid = latent_depth(target_latents, scale, shift, foreground)
        if decode:
            rgb, target_rgb = self._decoded(latents), self._decoded(target_latents)
        if (rgb is None) != (target_rgb is None):
            raise ValueError("compare: rgb= and target_rgb= go together")
        images = compare_images(rgb, target_rgb, **kw) if rgb is not None else None
        return images, compare_depth(depth, target_depth, valid=valid, align=align)

    @torch.no_grad()
    def p_losses(self, batch, trainer_config, noise_source=None, _aux=None):
        """viewfusion_zero_depth_rgb.py:362-392 -- the training objective's FORWARD pass on the HIP path: prepare_batch, shared
        random timestep, q_sample, apply_model (cfg 1, condition dropout when self.training), MSE against the noise.
        ``noise_source(V, D, S) -> dict(t, noise, depth_noise, drop_rand)`` injects the reference's random draws (parity tests);
        default: torch's device generator in the reference's order.  A ``{"_prepared": prepare_batch output}`` dict skips
        prepare_batch (benches)."""
        return self.p_losses_scenes([batch], trainer_config, noise_source=noise_source, _aux=_aux)

    def _draw(self, batch_latents, D, noise_source):
        """The random draws of one scene's training step, in the reference's order: (t (V,) shared, noise, depth_noise (V, D, S, S),
        drop_rand (V,)).  noise_source(V, D, S) -> dict(t, noise, depth_noise, drop_rand) replaces torch's generator."""
        V, _, S, _ = batch_latents.shape
        dev = batch_latents.device
        if noise_source is not None:
            ns = noise_source(V, D, S)
            return ns["t"].to(dev), ns["noise"].to(dev), ns["depth_noise"].to(dev), ns["drop_rand"].to(dev)
        t = self.scheduler.sample_random_times(V, share_t=True, device=dev)
        noise = torch.randn_like(batch_latents)
        return t, noise, torch.randn(V, D, S, S, device=dev), torch.rand(V, device=dev)

    def scene_draws(self, latents, noise_source=None):
        """The draws of an N-scene training step: scene after scene, each exactly what a single-scene p_losses on that scene draws
        (noise_source called once per scene, in order; torch's generator consumed in the single-scene order).  latents: one (V, 5, S, S)
        tensor per scene.  Returns a list of (t, noise, depth_noise, drop_rand)."""
        D = self.view_attn.n_pts_per_ray
        return [self._draw(bl, D, noise_source) for bl in latents]

    def _prepare_scenes(self, batches, trainer_config):
        """prepare_batch for every scene of a training step, after checking the list: non-empty, the same V and S everywhere."""
        if isinstance(batches, dict) or not isinstance(batches, (list, tuple)):
            raise TypeError("a multi-scene training step takes a list of batch dicts")
        if len(batches) == 0:
            raise ValueError("a multi-scene training step needs at least one scene")
        prepared = [b["_prepared"] if isinstance(b, dict) and "_prepared" in b else self.prepare_batch(b, trainer_config) for b in batches]
        V, _, S, _ = prepared[0][0].shape
        for n, pr in enumerate(prepared):
            Vn, _, Sn, _ = pr[0].shape
            if Vn != V:
                raise ValueError(f"scene {n} has {Vn} views, scene 0 has {V}: the scenes of a training step share V")
            if Sn != S:
                raise ValueError(f"scene {n} has {Sn}x{Sn} latents, scene 0 has {S}x{S}: the scenes of a training step share S")
        return prepared

    @torch.no_grad()
    def p_losses_scenes(self, batches, trainer_config, noise_source=None, _aux=None):
        """p_losses over N scenes in ONE batched step (scene-major views, global view scene*V + v): every scene draws its own timestep,
        noise, depth noise and dropout exactly as a single-scene p_losses on it would (scene_draws), the GEMMs / attention / convolutions
        run once over all N*V images, and the loss is the mean of the N single-scene losses (the MSE over all N*V views)."""
        prepared = self._prepare_scenes(batches, trainer_config)
        V = prepared[0][0].shape[0]
        draws = self.scene_draws([pr[0] for pr in prepared], noise_source)
        dev = prepared[0][0].device
        sa, s1 = self.scheduler.sqrt_alphas_cumprod.to(dev), self.scheduler.sqrt_one_minus_alphas_cumprod.to(dev)
        noisy = torch.cat([sa[t].view(V, 1, 1, 1) * pr[0] + s1[t].view(V, 1, 1, 1) * nz                  # q_sample per scene (:55-64)
                           for pr, (t, nz, _, _) in zip(prepared, draws)])
        ts = [int(t[0]) for t, _, _, _ in draws]
        conds = [(bc, il, ic, ce) for _, bc, il, ic, ce in prepared]
        prev = [pr[2][:, 4:].clone() for pr in prepared] if self.feed_prev_depth else None          # (:377-379)
        force = getattr(self, "_force_eager", False)
        self._train_keep_fp32, self._force_eager = True, True      # the backward reads block inputs from the workspace: every fp32 tensor is
        try:                                                      # written (on the step's engine only: ADVICE r04); no graph is replayed
            if len(prepared) == 1:             # one scene: through the public single-scene step (callers and tests may wrap it)
                (t, _, dn, dr), = draws
                pred = self.apply_model(noisy, *conds[0], t, prev_depth=None if prev is None else prev[0], depth_noise=dn, drop_rand=dr)
            else:
                pred = self._step_scenes(noisy, conds, ts, prev, torch.cat([d[2] for d in draws]), torch.cat([d[3] for d in draws]))
        finally:
            self._train_keep_fp32, self._force_eager = False, force
        if self.objective == "noise":
            target = torch.cat([d[1] for d in draws])
        elif self.objective == "x_start":
            target = torch.cat([pr[0] for pr in prepared])
        else:
            raise AssertionError(f"objective {self.objective} not implemented")
        assert self.loss_type == "l2", "loss_type 'l2' is the only one the reference implements (:86-87)"
        loss = torch.nn.functional.mse_loss(target, pred).mean()
        if _aux is not None:
            _aux.update(pred=pred, target=target)
        return loss

    def _loss(self, batch, trainer_config, noise_source=None, _aux=None):
        """p_losses for one batch dict, p_losses_scenes for a list of them."""
        return self.p_losses_scenes(batch if isinstance(batch, (list, tuple)) else [batch], trainer_config, noise_source=noise_source,
                                    _aux=_aux)

    @torch.no_grad()
    def gradients_scenes(self, batches, trainer_config, noise_source=None, only_trainable=False):
        """`gradients` of an N-scene training step (p_losses_scenes): (loss = the mean of the N single-scene losses, {state_dict key:
        gradient} = the mean of the N single-scene gradients), from one batched forward and backward."""
        if not isinstance(batches, (list, tuple)):
            raise TypeError("gradients_scenes takes a list of batch dicts (gradients takes one)")
        return self.gradients(list(batches), trainer_config, noise_source=noise_source, only_trainable=only_trainable)

    @torch.no_grad()
    def unet_gradients(self, batch, trainer_config, noise_source=None, only_trainable=False):
        """`loss.backward()` (train.py:90-95) through the WHOLE UNet and the per-step vector paths on the HIP backward kernels
        (mvdfusion_amd/backward_unet.py): gradients of every `unet_model.unet_model.*` and `cc_projection.*` parameter, plus the
        gradient w.r.t. the volume features that GridAttn produced (its own backward -- `view_attn.*`, `time_embed.*` -- continues
        from there in `gradients`).  Returns (loss, {state_dict key: gradient}, dvol (V, S, S, D, 768))."""
        from . import backward_blocks as bb
        from . import backward_unet as bu
        unet = self.unet_model.unet_model
        unet._record, self._force_eager = [], True
        try:
            loss, grads, dh = self.head_gradients(batch, trainer_config, noise_source=noise_source)
            record = unet._record
        finally:
            unet._record, self._force_eager = None, False
        V, mc, S, _ = dh.shape                     # (V = all N*V views of an N-scene step)
        D = self.view_attn.n_pts_per_ray
        eng = self._train_engine
        ctx = eng.ctx
        M = V * S * S
        R = eng.t_rows
        emb = ctx.ws.get("temb.emb", (R, unet.model_channels * 4))
        t_sin = ctx.ws.get("vf.tsin_unet", (R, unet.model_channels))
        tape = bb.Tape(dh.device, prec=ctx.prec, workspace=ctx.gemm_ws, only_trainable=only_trainable)
        dh_rows = dh.permute(0, 2, 3, 1).reshape(M, mc).contiguous()
        context = eng.context[:V].clone()
        g, dcontext, dvol = bu.unet_backward(unet, ctx, tape, record, dh_rows, V, S, D, emb, t_sin, context, eng.vol.view(V, S, S, D, -1))
        grads.update({"unet_model.unet_model." + k: v for k, v in g.items()})
        masks = getattr(self, "_last_drop_masks", None)
        if masks is not None:                      # the conditions were multiplied by the keep masks after their producers
            dcontext = dcontext * masks[0][:, None]
            dvol = dvol * masks[1].view(V, 1, 1, 1, 1)
        grads.update({"cc_projection." + k: v for k, v in bu.cc_projection_backward(self.cc_projection, eng.clip_v_embed[:V], dcontext).items()})
        return loss, grads, dvol

    @torch.no_grad()
    def gradients(self, batch, trainer_config, noise_source=None, only_trainable=False):
        """The complete `loss.backward()` of train.py:90-95 on the HIP path: unet_gradients continued through GridAttn
        (mvdfusion_amd/backward_gridattn.py: final layer, softmax-over-V pooling, 3 DiT blocks, pre layer, grid_sample backward,
        z-embedding) and ViewFusion.time_embed.  Returns (loss, {state_dict key: gradient}) for every parameter the loss depends on;
        with only_trainable the weight gradients of frozen parameters (requires_grad False) are skipped (None) -- their dgrad still runs."""
        from . import backward_blocks as bb
        from . import backward_gridattn as bg
        tune = self.train_autotune_min_flops is not None and not hip.AUTOTUNE
        if tune:          # the forward of the training step runs eagerly (condition dropout): its GEMMs and the backward's are tuned here,
            prev_min = hip.AUTOTUNE_MIN_FLOPS
            hip.AUTOTUNE, hip.AUTOTUNE_MIN_FLOPS = True, float(self.train_autotune_min_flops)      # once per shape (cached), big ones only
        try:
            return self._gradients(batch, trainer_config, noise_source, only_trainable)
        finally:
            if tune:
                hip.AUTOTUNE, hip.AUTOTUNE_MIN_FLOPS = False, prev_min
                hip.release_tuning_buffers()

    def _gradients(self, batch, trainer_config, noise_source, only_trainable):
        from . import backward_blocks as bb
        from . import backward_gridattn as bg
        loss, grads, dvol = self.unet_gradients(batch, trainer_config, noise_source=noise_source, only_trainable=only_trainable)
        B, S, _, D, _ = dvol.shape                 # (B = N*V views)
        eng = self._train_engine
        ctx = eng.ctx
        tape = bb.Tape(dvol.device, prec=ctx.prec, workspace=ctx.gemm_ws, only_trainable=only_trainable)
        c = ctx.ws.get("vf.c", (eng.t_rows, 256))
        g, dc = bg.gridattn_backward(self.view_attn, tape, eng, c, dvol.reshape(B * S * S * D, -1).contiguous(), eng.V, S, D)
        grads.update({"view_attn." + k: v for k, v in g.items()})
        t_sin = ctx.ws.get("vf.tsin", (eng.t_rows, 256))
        grads.update({"time_embed." + k: v for k, v in bg.time_embed_backward(self.time_embed, t_sin, dc).items()})
        return loss, grads

    @torch.no_grad()
    def tail_gradients(self, batch, trainer_config, noise_source=None):
        """head_gradients continued through the LAST output block (ResBlock + SpatialTransformer + ViewAlignedFeatureTransformer,
        `output_blocks.11`): every operator kind of the UNet has a backward on the HIP path (mvdfusion_amd/backward_blocks.py).
        Returns (loss, {state_dict key: gradient}, dcat = dL/d(input of that block) (V, 2 mc, S, S))."""
        from . import backward_blocks as bb
        loss, grads, dh = self.head_gradients(batch, trainer_config, noise_source=noise_source)
        unet = self.unet_model.unet_model
        V, mc, S, _ = dh.shape
        D = self.view_attn.n_pts_per_ray
        eng = self.engine(V, S, D, False)
        ctx = eng.ctx
        M = V * S * S
        blk = unet.output_blocks[len(unet.output_blocks) - 1]
        cin = blk[0].channels
        cat, catp = ctx.ws.get("cat", (M, cin)), ctx.ws.planes("catp", M, cin)
        emb = ctx.ws.get("temb.emb", (1, unet.model_channels * 4))
        tape = bb.Tape(dh.device, prec=ctx.prec, workspace=ctx.gemm_ws)
        dh_rows = dh.permute(0, 2, 3, 1).reshape(M, mc).contiguous()
        dcat, g, dcontext, dvol, demb = bb.output_block_backward(tape, ctx, blk, cat, catp, emb, eng.context[:V], eng.vol.view(M * D, -1),
                                                                 dh_rows, V, S, S, D)
        pre = f"unet_model.unet_model.output_blocks.{len(unet.output_blocks) - 1}."
        grads.update({pre + k: v for k, v in g.items()})
        return loss, grads, dcat.view(V, S, S, cin).permute(0, 3, 1, 2).contiguous()

    @torch.no_grad()
    def head_gradients(self, batch, trainer_config, noise_source=None):
        """First slice of train.py:90-95 (`loss.backward()`) on the HIP path: the training forward (p_losses) followed by the
        backward of MSE -> UNet output head (conv3x3 <- SiLU <- GroupNorm32) with the backward kernels of mvdfusion_amd/backward.py.
        Returns (loss, {state_dict key: gradient} for the four head parameters, dL/dh at the head's input (V, mc, S, S) -- where the
        backward currently stops: LayerNorm / attention / GEGLU backward do not exist yet)."""
        from . import backward
        aux = {}
        loss = self._loss(batch, trainer_config, noise_source=noise_source, _aux=aux)
        unet = self.unet_model.unet_model
        pred, target = aux["pred"], aux["target"]
        V, C, S, _ = pred.shape
        h, a = unet._head_saved
        rows = lambda t: t.permute(0, 2, 3, 1).reshape(V * S * S, C).contiguous()
        eng = self._train_engine
        grads, dh = backward.unet_head_backward(unet, h, a, rows(pred), rows(target), V, S, eng.ctx.gemm_ws)
        grads = {"unet_model.unet_model." + k: v for k, v in grads.items()}
        return loss, grads, dh.view(V, S, S, -1).permute(0, 3, 1, 2).contiguous()

    def forward(self, batch, trainer_config):
        """viewfusion_zero_depth_rgb.py:394-397: the training loss.  With autograd enabled and trainable parameters the returned
        scalar carries a graph node whose backward hands the HIP-computed gradients (self.gradients) to the parameters, so the
        reference's loop ``loss = model(batch, cfg); optimizer.zero_grad(); loss.backward(); optimizer.step()`` (train.py:86-95) runs
        unchanged -- under torch's DistributedDataParallel too: the parameters are inputs of that node, so DDP's gradient hooks fire and
        all-reduce over RCCL as usual.  Without autograd (torch.no_grad / eval): the plain loss value.
        ``batch`` may also be a LIST of batch dicts: one multi-scene step (p_losses_scenes / gradients_scenes) whose loss and gradients are
        the means over the scenes -- the reference's scene_batch_size > 1."""
        # (view_attn.t_embedder exists in the reference's module tree but its forward never calls it: those parameters stay outside
        #  the graph, exactly like the reference -- DDP(find_unused_parameters=True) treats them as unused)
        params = [(n, p) for n, p in self.named_parameters() if p.requires_grad and not n.startswith("view_attn.t_embedder.")]
        if not torch.is_grad_enabled() or not params:
            return self._loss(batch, trainer_config, noise_source=getattr(self, "_noise_source", None))
        return _HipTrainingLoss.apply(self, batch, trainer_config, tuple(n for n, _ in params), *[p for _, p in params])

    def configure_optimizers(self, lr=None, verbose=False):
        lr = self.learning_rate if lr is None else lr
        groups = []
        if self.finetune_projection:
            groups.append({"params": self.cc_projection.parameters(), "lr": lr})
        groups.append({"params": self.unet_model.get_trainable_parameters(), "lr": lr})
        groups.append({"params": self.time_embed.parameters(), "lr": lr})
        groups.append({"params": self.view_attn.parameters(), "lr": lr})
        from .optim import HipAdamW
        return HipAdamW(groups, lr=lr)          # a torch.optim.AdamW whose step() is one HIP launch (mvdfusion_amd/optim.py)
