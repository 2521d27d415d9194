"""50-step stochastic DDIM sampler -- mirror of ``mvdfusion.sampler.DDIMSampler`` (mvdfusion/sampler.py:13-147).

``sample`` keeps the reference signature and return values but runs the loop as 50 replays of one captured hipGraph
(GridAttn + CFG-batched UNet + CFG combine + DDIM update + iteration counter all on the device); the per-step scalars
come from a device table built here on the host in float64 -> float32 exactly like sampler.py:25-39.
``denoise_apply`` / ``denoise_apply_impl`` are kept for callers that drive single steps (utils/vis_utils.py:30-35).

Noise: the reference draws on the device generator (torch.normal in GridAttn, randn_like in the update).  Here all noise
of a sample is drawn up-front in the reference's order (depth noise, then update noise, per step) either from torch's
device generator or from ``noise_source`` -- a callable ``(V, S, D, steps) -> (depth_noise, ddim_noise)`` used by the
parity tests to inject host-generated noise (SURVEY.md trap T2).
"""
import numpy as np
import torch

from .engine import ddim_step_table


def make_ddim_timesteps(num_ddim_timesteps, num_ddpm_timesteps):
    """'uniform' discretisation, +1 shift (external/sd1/ldm/modules/diffusionmodules/util.py:46-60)."""
    c = num_ddpm_timesteps // num_ddim_timesteps
    return np.asarray(list(range(0, num_ddpm_timesteps, c))) + 1


def plan_rig_chunks(M, V, K, anchors=None):
    """Chunks of at most V views that cover a rig of M views when one step holds V: chunk 0 is views 0..V-1 from noise, every later
    chunk holds K already-generated views fixed (``DDIMSampler.sample(known_latents=...)``) and generates the next V - K views in rig
    order (the last chunk may be shorter, never without a new view).  Anchors: the K most recently generated views, or
    ``anchors(chunk_index, done, new) -> K distinct indices out of done`` (done / new: rig indices generated so far / by this chunk).
    Returns one list of rig indices per chunk in the order handed to ``sample``: anchors first, then the new views.  M <= V is the one
    chunk 0..M-1, whatever K."""
    M, V, K = int(M), int(V), int(K)
    if M < 1 or V < 1:
        raise ValueError(f"plan_rig_chunks: M = {M} views in chunks of V = {V}")
    if M <= V:
        return [list(range(M))]
    if not 1 <= K < V:
        raise ValueError(f"plan_rig_chunks: K = {K} anchors in chunks of V = {V} views (1 <= K < V: a chunk generates at least one view)")
    chunks, done = [list(range(V))], list(range(V))
    while len(done) < M:
        new = list(range(len(done), min(len(done) + V - K, M)))
        if anchors is None:
            pick = done[-K:]
        else:
            pick = [int(a) for a in anchors(len(chunks), list(done), list(new))]
            if len(pick) != K or len(set(pick)) != K or not set(pick) <= set(done):
                raise ValueError(f"plan_rig_chunks: anchors(chunk {len(chunks)}) returned {pick}: expected {K} distinct views out of "
                                 f"the {len(done)} generated so far")
        chunks.append(pick + new)
        done += new
    return chunks


class DDIMSampler:
    def __init__(self, model, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0.0, latent_size=32,
                 overwrite_x_noisy=False, z_dim=4, feed_prev_depth=False):
        assert ddim_discretize == "uniform"
        self.model = model
        self.ddpm_num_timesteps = model.scheduler.num_timesteps
        self.latent_size, self.eta, self.z_dim = latent_size, ddim_eta, z_dim
        # overwrite_x_noisy (sampler.py:109-110,123-124): before every iteration row 0 becomes the clean input_latents[0]
        self.overwrite_x_noisy, self.feed_prev_depth = bool(overwrite_x_noisy), feed_prev_depth
        self.noise_source = None
        self._make_schedule(ddim_num_steps, ddim_eta)

    def _make_schedule(self, ddim_num_steps, ddim_eta):
        self.ddim_timesteps = make_ddim_timesteps(ddim_num_steps, self.ddpm_num_timesteps)
        ts = torch.from_numpy(self.ddim_timesteps.astype(np.int64))
        ac = self.model.scheduler.alphas_cumprod.detach().cpu()
        a = ac[ts].double()
        a_prev = torch.cat([ac[0:1], ac[ts[:-1]]], 0)
        sig = ddim_eta * torch.sqrt((1 - a_prev) / (1 - a) * (1 - a / a_prev))
        self.ddim_alphas_raw = self.model.scheduler.alphas.detach().cpu()[ts].float()
        self.ddim_sigmas = sig.float()
        self.ddim_alphas = a.float()
        self.ddim_alphas_prev = a_prev.float()
        self.ddim_sqrt_one_minus_alphas = torch.sqrt(1.0 - self.ddim_alphas).float()

    def tables(self):
        sch = self.model.scheduler
        st = {k: getattr(sch, k).detach().cpu() for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")}
        dd = {"timesteps": torch.from_numpy(self.ddim_timesteps.astype(np.int64)), "alphas": self.ddim_alphas,
              "alphas_prev": self.ddim_alphas_prev, "sigmas": self.ddim_sigmas,
              "sqrt_one_minus_alphas": self.ddim_sqrt_one_minus_alphas}
        return st, dd

    @torch.no_grad()
    def denoise_apply_impl(self, x_target_noisy, index, noise_pred, is_step0=False):
        dev = x_target_noisy.device
        a_t = self.ddim_alphas[index].to(dev).view(1, 1, 1, 1)
        a_prev = self.ddim_alphas_prev[index].to(dev).view(1, 1, 1, 1)
        s1m = self.ddim_sqrt_one_minus_alphas[index].to(dev).view(1, 1, 1, 1)
        sigma = self.ddim_sigmas[index].to(dev).view(1, 1, 1, 1)
        pred_x0 = (x_target_noisy - s1m * noise_pred) / a_t.sqrt()
        x_prev = a_prev.sqrt() * pred_x0 + torch.clamp(1.0 - a_prev - sigma ** 2, min=1e-7).sqrt() * noise_pred
        if not is_step0:
            x_prev = x_prev + sigma * torch.randn_like(x_target_noisy)
        return x_prev, pred_x0

    @torch.no_grad()
    def denoise_apply(self, x_target_noisy, batch_cameras, input_latents, input_cameras, clip_embed, time_steps, index,
                      is_step0=False, prev_depth=None, cfg_scale=1.0):
        eps = self.model.apply_model(x_target_noisy, batch_cameras, input_latents, input_cameras, clip_embed, time_steps,
                                     prev_depth=prev_depth if self.feed_prev_depth else None, cfg_scale=cfg_scale)      # (:83-86)
        return self.denoise_apply_impl(x_target_noisy, index, eps, is_step0)

    @torch.no_grad()
    def sample(self, batch_cameras, input_latents, input_cameras, clip_embed, unconditional_scale=1.0, depth=False,
               return_intermediates=False, verbose=True, x_T=None, num_steps=None, use_graph=True, known_latents=None,
               known_noise=None):
        """Returns x_0 (V, 5, S, S) [and the per-step {'t','xt','x0'} list].  ``x_T``/``num_steps`` are extensions:
        inject the initial noise / run only the first ``num_steps`` iterations (parity tests, bench warm-up).  One scene of
        ``sample_scenes``.

        ``known_latents`` (K, 5, S, S), 1 <= K < V, holds the FIRST K views of the rig fixed at these clean latents and generates the other
        V - K: every iteration starts with rows [0, K) re-noised to its timestep (sqrt(ab_t) known + sqrt(1 - ab_t) noise) inside the captured
        step, the pinned views are references of GridAttn only (no query rows, no UNet rows, no update: the engine of the query range
        [K, V)), and the returned rows [0, K) are ``known_latents`` exactly.  ``known_noise`` (steps, K, 5, S, S) injects the pin noise;
        default: torch's device generator, drawn after every draw an unpinned call makes -- x_T, depth and update noise keep their full-V
        shapes and order, so the free rows see the noise of the unpinned run with the same seed / ``noise_source`` (x_T rows [0, K) are
        ignored).  Intermediates carry the pinned rows as the step saw them in 'xt' and ``known_latents`` in 'x0'."""
        res = self._sample([(batch_cameras, input_latents, input_cameras, clip_embed)], unconditional_scale, depth,
                           return_intermediates, None if x_T is None else x_T.reshape(1, *x_T.shape), num_steps, use_graph,
                           known_latents=known_latents, known_noise=known_noise)
        if not return_intermediates:
            return res[0]
        x, inter = res
        return x[0], [{"t": it["t"], "xt": it["xt"][0], "x0": it["x0"][0]} for it in inter]

    @torch.no_grad()
    def sample_rig(self, batch_cameras, input_latents, input_cameras, clip_embed, unconditional_scale=1.0, chunk_views=None,
                   anchors_per_chunk=1, anchors=None, depth=True, verbose=True, x_T=None, known_noise=None, num_steps=None, use_graph=True):
        """A rig of M = len(batch_cameras) views, larger than one step holds, in chunks of ``chunk_views`` (``plan_rig_chunks``): chunk 0
        is a plain ``sample``; every later chunk is a ``sample`` with ``anchors_per_chunk`` already-generated views pinned
        (``known_latents``) -- by default the most recent ones, or what ``anchors(chunk_index, done, new)`` picks.  Cameras and
        ``clip_embed`` (M rows) are sliced per chunk; every chunk keeps full attention between its views.  ``x_T`` (M, 5, S, S) is the
        initial noise in rig order (rows of anchors are not used); ``known_noise``: {chunk index: (steps, K, 5, S, S)} pin noise of the
        later chunks; ``noise_source`` is called once per chunk with that chunk's view count.  Returns (M, 5, S, S) in rig order: every
        view is generated exactly once, anchors are returned as first generated."""
        from .cameras import get_camera_slice
        M = int(clip_embed.shape[0])
        if len(batch_cameras) != M:
            raise ValueError(f"sample_rig: {len(batch_cameras)} cameras for {M} rows of clip_embed")
        chunks = plan_rig_chunks(M, M if chunk_views is None else chunk_views, anchors_per_chunk, anchors)
        out, done = None, set()
        for c, idx in enumerate(chunks):
            K = 0 if c == 0 else int(anchors_per_chunk)
            ti = torch.as_tensor(idx, dtype=torch.long)
            x = self.sample(get_camera_slice(batch_cameras, idx), input_latents, input_cameras, clip_embed[ti.to(clip_embed.device)],
                            unconditional_scale=unconditional_scale, depth=depth, verbose=verbose,
                            x_T=None if x_T is None else x_T[ti.to(x_T.device)], num_steps=num_steps, use_graph=use_graph,
                            known_latents=out[ti[:K].to(out.device)] if K else None,
                            known_noise=None if (known_noise is None or not K) else known_noise.get(c))
            if out is None:
                out = torch.zeros(M, *x.shape[1:], dtype=x.dtype, device=x.device)
            new = idx[K:]
            assert not done & set(new)
            out[ti[K:].to(out.device)] = x[K:]
            done |= set(new)
        assert len(done) == M
        return out

    @torch.no_grad()
    def sample_scenes(self, conds, unconditional_scale, depth=True, return_intermediates=False, verbose=True, x_T=None,
                      num_steps=None, use_graph=True, known_latents=None):
        """``sample`` for N scenes in one batched step: ``conds`` is a list of (batch_cameras, input_latents, input_cameras,
        clip_embed), one per scene, all with the same V and S.  Every step runs GridAttn, the CFG-batched UNet (2 N V images: the
        N V conditional rows scene-major, then the N V null rows) and the update once for all scenes.  Returns x_0 (N, V, 5, S, S)
        [and the per-step {'t','xt','x0'} list with (N, V, 5, S, S) tensors].  ``x_T``: (N, V, 5, S, S) initial noise.
        ``noise_source`` is called once per scene, in scene order, exactly as ``sample`` calls it for that scene alone.
        ``known_latents`` is refused: a pinned run owns the query range [K, V), and query ranges are single-scene."""
        if known_latents is not None:
            raise ValueError("sample_scenes: known_latents pins views through the engine's query range, which is single-scene "
                             "(call sample() per scene)")
        return self._sample(conds, unconditional_scale, depth, return_intermediates, x_T, num_steps, use_graph)

    def _sample(self, conds, unconditional_scale, depth, return_intermediates, x_T, num_steps, use_graph, known_latents=None,
                known_noise=None):
        """The DDIM loop of ``sample`` (one scene) and ``sample_scenes``."""
        assert depth, "MVD-Fusion samples RGB-D latents (depth=True at every call site: demo.py:85-90)"
        m = self.model
        N = len(conds)
        if N < 1:
            raise ValueError("sample_scenes: no scenes")
        V, S, D = int(conds[0][3].shape[0]), self.latent_size, m.view_attn.n_pts_per_ray
        for i, (bc, il, ic, ce) in enumerate(conds):
            if int(ce.shape[0]) != V or len(bc) != V:
                raise ValueError(f"sample_scenes: scene {i} has {int(ce.shape[0])} views, scene 0 has {V} (every scene of a call "
                                 "shares V)")
            if tuple(il.shape[-2:]) != (S, S):
                raise ValueError(f"sample_scenes: scene {i} has {tuple(il.shape[-2:])} latents, the sampler's latent size is {S}")
        if x_T is not None and tuple(x_T.shape) != (N, V, self.z_dim + 1, S, S):
            raise ValueError(f"sample_scenes: x_T {tuple(x_T.shape)}, expected {(N, V, self.z_dim + 1, S, S)}")
        dev = m._device.device
        total = self.ddim_timesteps.shape[0]
        n_run = total if num_steps is None else int(num_steps)
        cfg = unconditional_scale != 1.0
        K = 0
        if known_latents is not None:
            if self.overwrite_x_noisy:
                raise ValueError("sample: known_latents with overwrite_x_noisy=True -- both rewrite row 0 before every iteration")
            if known_latents.dim() != 4 or tuple(known_latents.shape[1:]) != (self.z_dim + 1, S, S):
                raise ValueError(f"sample: known_latents {tuple(known_latents.shape)}, expected (K, {self.z_dim + 1}, {S}, {S})")
            K = int(known_latents.shape[0])
            if not 1 <= K < V:
                raise ValueError(f"sample: known_latents pins K = {K} of V = {V} views (1 <= K < V: at least one view is generated)")
            if known_noise is not None and (known_noise.dim() != 5 or not n_run <= int(known_noise.shape[0]) <= total or
                                            tuple(known_noise.shape[1:]) != (K, self.z_dim + 1, S, S)):
                raise ValueError(f"sample: known_noise {tuple(known_noise.shape)}, expected (steps, {K}, {self.z_dim + 1}, {S}, {S}) with "
                                 f"{n_run} <= steps <= {total}")
        elif known_noise is not None:
            raise ValueError("sample: known_noise without known_latents")
        eng = m.engine(V, S, D, cfg, q0=K, Vq=V - K) if K else m.engine(V, S, D, cfg, scenes=N)
        eng.set_conditioning_scenes([(bc, il.to(dev), ic, ce.to(dev)) for bc, il, ic, ce in conds])
        st, dd = self.tables()
        table = ddim_step_table(st, dd, [total - i - 1 for i in range(total)])
        x_T = torch.randn([N * V, self.z_dim + 1, S, S], device=dev) if x_T is None else x_T.reshape(N * V, self.z_dim + 1, S, S)
        if self.noise_source is not None:
            per = [self.noise_source(V, S, D, total) for _ in range(N)]
            dn = torch.stack([torch.as_tensor(p[0]).reshape(total, V, D, S, S) for p in per], 1).reshape(total, N * V, D, S, S)
            sn = torch.stack([torch.as_tensor(p[1]).reshape(total, V, 5, S, S) for p in per], 1).reshape(total, N * V, 5, S, S)
        else:
            dn = torch.randn(total, N * V, D, S, S, device=dev)
            sn = torch.randn(total, N * V, 5, S, S, device=dev)
        eng.set_schedule(table, dn, sn)
        eng.x.copy_(x_T)
        if K:
            known = known_latents.to(dev, torch.float32)
            pn = torch.zeros(total, K, self.z_dim + 1, S, S, device=dev)
            if known_noise is None:
                pn.copy_(torch.randn(total, K, self.z_dim + 1, S, S, device=dev))      # (after every draw of an unpinned call)
            else:
                pn[:int(known_noise.shape[0])].copy_(known_noise)
        inter = []
        try:
            if K:
                eng.set_pin(1, known, pn)
            elif self.overwrite_x_noisy:       # row 0 of every scene <- that scene's clean input_latents[0]; every row stays a query row
                eng.set_pin(0, torch.stack([il.reshape(-1, self.z_dim + 1, S, S)[0] for _, il, _, _ in conds]).to(dev))
            for i in range(n_run):
                # feed_prev_depth (:135-140): from the second iteration on GridAttn samples depth around the previous step's x0 estimate,
                # which the step engine keeps in eng.x0 (a second captured graph; the first iteration has no estimate yet)
                eng.depth_mode = 1 if (self.feed_prev_depth and i > 0) else 0
                eng.step(unconditional_scale, do_update=True, use_graph=use_graph)
                if return_intermediates:
                    inter.append({"t": int(self.ddim_timesteps[total - i - 1]), "xt": eng.x.clone().view(N, V, 5, S, S),
                                  "x0": eng.x0.clone().view(N, V, 5, S, S)})
        finally:                               # engines are cached per signature: never leak a depth mode or a pin into the next caller
            eng.depth_mode = 0
            if K or self.overwrite_x_noisy:
                eng.clear_pin()
        from . import hip
        out = eng.x.clone()
        if K:
            out[:K].copy_(known)
        out = hip.check_finite(out, "DDIMSampler.sample").view(N, V, 5, S, S)
        return (out, inter) if return_intermediates else out
