"""How good is an image or a depth map: PSNR, SSIM and the depth-error family on the GPU (include/mvd_hip.h: mvd_image_metrics,
mvd_depth_metrics have the rules in full; csrc/view_metrics.hip).

``compare_images`` scores images against ground truth: mean squared error, PSNR and the mean SSIM under an optional mask, every moment
of the SSIM window accumulated in fp64 (on the near-flat images a white-background render mostly is, fp32 moments move the SSIM map by
2.5e-4: the cancellation in E[x^2] - mu^2 is measured against C2 = 9e-4).  ``compare_depth`` scores depth maps: abs-rel, sq-rel, RMSE,
log-RMSE and the three delta accuracies, after no alignment, a least-squares scale or scale and shift per image, or a given fit.
``compare_views`` takes two ``RenderedViews`` / ``RenderedMesh`` (or mappings with rgb / depth / hit) and returns both records, and
``ViewFusion.compare`` binds the model's decoder and depth map.  Every sum is fp64 in a fixed order -- the same bits run to run and for
an image alone or inside a batch -- and nothing synchronises with the host: the records hold tensors on the inputs' device.

``ssim_window`` is THE window table: the kernels take it by value and the test oracle uses the same one, so no ``exp`` of another library
enters.  LPIPS is out of scope (it needs network weights).
"""
import ctypes
import math
from collections.abc import Mapping
from dataclasses import dataclass
from typing import Optional

import torch

from . import hip

ALIGN = {"none": hip.DEPTH_ALIGN_NONE, "scale": hip.DEPTH_ALIGN_SCALE, "scale_shift": hip.DEPTH_ALIGN_SCALE_SHIFT}
MAX_SIDE = 32768                             # the largest H and W of both entries
MAX_PLANES = 65535                           # the most B * C planes (images of compare_depth) of one call


@dataclass
class ImageMetrics:
    """What ``compare_images`` returns: fp64 tensors with the inputs' leading dimensions, on their device."""
    mse: torch.Tensor                        # sq_sum / (count * C); NaN where count == 0
    psnr: torch.Tensor                       # 10 log10(data_range^2 / mse): +inf at mse == 0
    ssim: Optional[torch.Tensor]             # the mean SSIM over channels and counting window positions; NaN without one; None for window=None
    count: torch.Tensor                      # int64: the pixels the mask counts
    ssim_map: Optional[torch.Tensor]         # (.., C, H - window + 1, W - window + 1) fp64 with return_map=True


@dataclass
class DepthMetrics:
    """What ``compare_depth`` returns: fp64 tensors (the counts int64) with the inputs' leading dimensions.  Every ratio is NaN at
    count == 0."""
    abs_rel: torch.Tensor                    # mean |p' - t| / t
    sq_rel: torch.Tensor                     # mean (p' - t)^2 / t
    rmse: torch.Tensor                       # sqrt(mean (p' - t)^2)
    rmse_log: torch.Tensor                   # sqrt(mean (log p' - log t)^2)
    delta1: torch.Tensor                     # the share of pixels with max(p' / t, t / p') < 1.25
    delta2: torch.Tensor                     # ... < 1.25^2
    delta3: torch.Tensor                     # ... < 1.25^3
    scale: torch.Tensor                      # the fit p' = scale * p + shift that was applied
    shift: torch.Tensor
    count: torch.Tensor                      # int64: the pixels scored
    dropped: torch.Tensor                    # int64: valid pixels whose p' was not > 0


def ssim_window(window=11, sigma=1.5):
    """The ``window`` weights of the separable SSIM filter as a tuple of Python floats: exp(-(i - window // 2)^2 / (2 sigma^2)) divided by
    their left-to-right sum; ``sigma=None`` gives the uniform window 1 / window."""
    if isinstance(window, bool) or int(window) != window or window < 3 or window > hip.SSIM_MAX_WINDOW or window % 2 == 0:
        raise ValueError(f"window = {window}: an odd integer in [3, {hip.SSIM_MAX_WINDOW}]")
    window = int(window)
    if sigma is None:
        return tuple(1.0 / window for _ in range(window))
    sigma = float(sigma)
    if not (sigma > 0 and math.isfinite(sigma)):
        raise ValueError(f"sigma = {sigma}: finite and > 0, or None for the uniform window")
    g = [math.exp(-float((i - window // 2) ** 2) / (2.0 * sigma * sigma)) for i in range(window)]
    total = 0.0
    for v in g:
        total += v
    return tuple(v / total for v in g)


def _scratch(nbytes, dev):
    return torch.empty(max((int(nbytes) + 7) // 8, 1), dtype=torch.int64, device=dev)


def _image_metrics(a, b, mask, weights, c1, c2, want_map):
    """The enqueues of mvd_image_metrics.  a, b (B, C, H, W) fp32 contiguous on one GPU, mask (B, H, W) uint8 or None, weights a tuple or
    None -> (sq_sum, count, ssim_sum or None, ssim_count or None, ssim_map or None).  No host synchronisation."""
    L = hip.lib()
    B, C, H, W = a.shape
    dev = a.device
    hip._req(a), hip._req(b)
    if mask is not None:
        hip._req(mask, torch.uint8)
    window = len(weights) if weights is not None else 0
    f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)
    i64 = lambda *shape: torch.empty(*shape, dtype=torch.int64, device=dev)
    sq_sum, count = f64(B), i64(B)
    ssim_sum = f64(B) if window else None
    ssim_count = i64(B) if window else None
    ssim_map = f64(B, C, H - window + 1, W - window + 1) if window and want_map else None
    if B == 0:
        return sq_sum, count, ssim_sum, ssim_count, ssim_map
    nbytes = int(L.mvd_image_metrics_scratch(B, C, H, W, window))
    scratch = _scratch(nbytes, dev)
    table = (ctypes.c_double * window)(*weights) if window else None
    hip.check(L.mvd_image_metrics(hip.ptr(a), hip.ptr(b), hip.ptr(mask), B, C, H, W, table, window, float(c1), float(c2), hip.ptr(sq_sum),
                                  hip.ptr(count), hip.ptr(ssim_sum), hip.ptr(ssim_count), hip.ptr(ssim_map), hip.ptr(scratch), nbytes,
                                  hip.stream()))
    return sq_sum, count, ssim_sum, ssim_count, ssim_map


def _depth_metrics(pred, target, valid, align, fit_in=None):
    """The enqueues of mvd_depth_metrics.  pred, target (B, H, W) fp32 contiguous, valid (B, H, W) uint8 or None, fit_in (B, 2) fp64 with
    align = hip.DEPTH_ALIGN_GIVEN -> (fit (B, 2), sums (B, 4), counts (B, 5)).  No host synchronisation."""
    L = hip.lib()
    B, H, W = pred.shape
    dev = pred.device
    hip._req(pred), hip._req(target)
    if valid is not None:
        hip._req(valid, torch.uint8)
    if fit_in is not None:
        hip._req(fit_in, torch.float64)
    fit = torch.empty(B, 2, dtype=torch.float64, device=dev)
    sums = torch.empty(B, 4, dtype=torch.float64, device=dev)
    counts = torch.empty(B, 5, dtype=torch.int64, device=dev)
    if B == 0:
        return fit, sums, counts
    nbytes = int(L.mvd_depth_metrics_scratch(B, H, W))
    scratch = _scratch(nbytes, dev)
    hip.check(L.mvd_depth_metrics(hip.ptr(pred), hip.ptr(target), hip.ptr(valid), B, H, W, align, hip.ptr(fit_in), hip.ptr(fit), hip.ptr(sums),
                                  hip.ptr(counts), hip.ptr(scratch), nbytes, hip.stream()))
    return fit, sums, counts


def _pair(pred, target, tail, what):
    """The two tensors of one comparison: equal shapes with at least ``tail`` dimensions, on one GPU."""
    if not torch.is_tensor(pred) or not torch.is_tensor(target):
        raise ValueError(f"{what}: pred and target must be tensors")
    if pred.shape != target.shape or pred.dim() < tail:
        raise ValueError(f"{what}: pred of shape {tuple(pred.shape)} and target of shape {tuple(target.shape)}: need equal shapes with at least "
                         f"{tail} dimensions")
    if pred.device != target.device:
        raise ValueError(f"{what}: pred on {pred.device}, target on {target.device}")
    H, W = int(pred.shape[-2]), int(pred.shape[-1])
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"{what}: maps of {H} x {W} pixels, each side must lie in [1, {MAX_SIDE}]")
    return H, W


def _mask_of(mask, lead, H, W, dev, name):
    """``mask`` (lead.., H, W) of any dtype -> (B, H, W) uint8 on dev, non-zero where it counts; None stays None."""
    if mask is None:
        return None
    if not torch.is_tensor(mask) or tuple(mask.shape) != (*lead, H, W):
        got = tuple(mask.shape) if torch.is_tensor(mask) else type(mask).__name__
        raise ValueError(f"{name} of shape {got}: need {(*lead, H, W)}, the images' shape without the channels")
    return (mask != 0).to(dev, torch.uint8).reshape(-1, H, W).contiguous()


def compare_images(pred, target, mask=None, data_range=1.0, window=11, sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """Score images against ground truth (include/mvd_hip.h: mvd_image_metrics) -> ImageMetrics.

    pred, target : (.., C, H, W) tensors of one shape on one GPU; H and W are independent.  They are read as fp32.
    mask         : (.., H, W), non-zero = the pixel counts, or None for every pixel.  SSIM counts the window positions whose CENTRE
                   pixel the mask counts -- the mask cropped by window // 2 on each side, as the map itself is.
    data_range   : the value range of the images (1.0 for [0, 1]); it sets PSNR's peak and SSIM's c1 = (k1 data_range)^2,
                   c2 = (k2 data_range)^2.
    window, sigma: ``ssim_window(window, sigma)`` is the separable filter, "valid" region only, so H, W >= window; window=None skips
                   SSIM (``ssim`` and ``ssim_map`` are None).
    return_map   : also return the (.., C, H - window + 1, W - window + 1) fp64 SSIM map.
    A pixel that is not finite under the mask makes the image's figures not finite; it is not left out."""
    H, W = _pair(pred, target, 3, "compare_images")
    lead, C = tuple(pred.shape[:-3]), int(pred.shape[-3])
    B = math.prod(lead)
    if C < 1 or B * C > MAX_PLANES:
        raise ValueError(f"compare_images: {B} images of {C} channels: need C >= 1 and at most {MAX_PLANES} planes per call")
    data_range, k1, k2 = float(data_range), float(k1), float(k2)
    if not (data_range > 0 and math.isfinite(data_range)):
        raise ValueError(f"data_range = {data_range}: finite and > 0")
    weights = None
    if window is not None:
        weights = ssim_window(window, sigma)
        if H < window or W < window:
            raise ValueError(f"window = {window}: larger than the images' {H} x {W} pixels (window=None skips SSIM)")
        if not (k1 >= 0 and k2 >= 0 and math.isfinite(k1) and math.isfinite(k2)):
            raise ValueError(f"k1 = {k1}, k2 = {k2}: finite and >= 0")
    elif return_map:
        raise ValueError("return_map=True needs a window")
    dev = pred.device
    m = _mask_of(mask, lead, H, W, dev, "mask")
    a = pred.reshape(B, C, H, W).to(torch.float32).contiguous()
    b = target.reshape(B, C, H, W).to(torch.float32).contiguous()
    sq_sum, count, ssim_sum, ssim_count, ssim_map = _image_metrics(a, b, m, weights, (k1 * data_range) ** 2, (k2 * data_range) ** 2,
                                                                   return_map)
    mse = sq_sum / (count * C)                      # 0 / 0 = NaN at count == 0
    psnr = 10.0 * torch.log10(data_range * data_range / mse)
    ssim = None if weights is None else ssim_sum / (ssim_count * C)
    return ImageMetrics(mse=mse.reshape(lead), psnr=psnr.reshape(lead), ssim=None if ssim is None else ssim.reshape(lead),
                        count=count.reshape(lead), ssim_map=None if ssim_map is None else ssim_map.reshape(*lead, *ssim_map.shape[1:]))


def compare_depth(pred, target, valid=None, align="none"):
    """Score depth maps against ground truth (include/mvd_hip.h: mvd_depth_metrics) -> DepthMetrics.

    pred, target : (.., H, W) tensors of one shape on one GPU, read as fp32.  A pixel is scored when ``valid`` counts it and both depths
                   are finite and > 0, so the renderers' empty depth (+inf) drops out by itself.
    valid        : (.., H, W), non-zero = the pixel counts, or None.
    align        : "none"; "scale" -- pred is multiplied by the least-squares s = sum(p t) / sum(p p) of each image first, what a method
                   with an unknown global scale is granted; "scale_shift" -- the least-squares (s, b) of s p + b = t per image (NaN, and
                   every pixel dropped, when the pixels do not determine it); or a (.., 2) tensor of (scale, shift) per image to apply
                   as given -- one scene-wide scale, say.
    A scored pixel whose aligned depth is not > 0 is dropped and counted in ``dropped``."""
    H, W = _pair(pred, target, 2, "compare_depth")
    lead = tuple(pred.shape[:-2])
    B = math.prod(lead)
    if B > MAX_PLANES:
        raise ValueError(f"compare_depth: {B} maps, at most {MAX_PLANES} per call")
    dev = pred.device
    fit_in = None
    if torch.is_tensor(align):
        if tuple(align.shape) != (*lead, 2):
            raise ValueError(f"align of shape {tuple(align.shape)}: a given fit is {(*lead, 2)}, (scale, shift) per image")
        fit_in, mode = align.to(dev, torch.float64).reshape(B, 2).contiguous(), hip.DEPTH_ALIGN_GIVEN
    elif align in ALIGN:
        mode = ALIGN[align]
    else:
        raise ValueError(f"align = {align!r}: one of {sorted(ALIGN)} or a (.., 2) tensor of (scale, shift)")
    v = _mask_of(valid, lead, H, W, dev, "valid")
    p = pred.reshape(B, H, W).to(torch.float32).contiguous()
    t = target.reshape(B, H, W).to(torch.float32).contiguous()
    fit, sums, counts = _depth_metrics(p, t, v, mode, fit_in)
    n = counts[:, 3]                                # 0 / 0 = NaN at count == 0
    r = lambda x: x.reshape(lead)
    return DepthMetrics(abs_rel=r(sums[:, 0] / n), sq_rel=r(sums[:, 1] / n), rmse=r(torch.sqrt(sums[:, 2] / n)),
                        rmse_log=r(torch.sqrt(sums[:, 3] / n)), delta1=r(counts[:, 0] / n), delta2=r(counts[:, 1] / n),
                        delta3=r(counts[:, 2] / n), scale=r(fit[:, 0]), shift=r(fit[:, 1]), count=r(n), dropped=r(counts[:, 4]))


def _field(views, name, side):
    v = views[name] if isinstance(views, Mapping) else getattr(views, name, None)
    if v is None and name != "rgb":
        raise ValueError(f"compare_views: {side} has no '{name}' (a RenderedViews, a RenderedMesh or a mapping with rgb / depth / hit)")
    return v


def view_masks(pred_hit, target_hit, mask="both"):
    """The two masks of ``compare_views`` from the hit maps: (the images' mask or None, the depth validity).  mask: "both" (hit in both),
    "either", "target", None (every pixel) or a tensor of the hit maps' shape; the depth validity is always pred_hit & target_hit & mask."""
    ph, th = pred_hit != 0, target_hit != 0
    if ph.shape != th.shape:
        raise ValueError(f"compare_views: hit maps of shapes {tuple(ph.shape)} and {tuple(th.shape)}")
    if mask is None:
        m = None
    elif torch.is_tensor(mask):
        if mask.shape != ph.shape:
            raise ValueError(f"mask of shape {tuple(mask.shape)}: need the hit maps' {tuple(ph.shape)}")
        m = mask.to(ph.device) != 0
    elif mask == "both":
        m = ph & th
    elif mask == "either":
        m = ph | th
    elif mask == "target":
        m = th
    else:
        raise ValueError(f"mask = {mask!r}: 'both', 'either', 'target', None or a tensor")
    return m, (ph & th) if m is None else (ph & th & m)


def compare_views(pred, target, mask="both", align="none", **image_kw):
    """Score rendered views against reference views -> (ImageMetrics or None, DepthMetrics).

    pred, target : a ``RenderedViews``, a ``RenderedMesh`` or a mapping with ``rgb`` (.., 3, P, P) or None, ``depth`` (.., P, P) and
                   ``hit`` (.., P, P); the images are scored when both sides have them.
    mask         : which pixels the IMAGE metrics count: "both" -- hit on both sides; "either"; "target"; None -- every pixel, the
                   backgrounds included; or a tensor (.., P, P).  The depth metrics always count pred.hit & target.hit & that mask.
    align        : as ``compare_depth`` takes it.  Other keywords go to ``compare_images``."""
    m, valid = view_masks(_field(pred, "hit", "pred"), _field(target, "hit", "target"), mask)
    a, b = _field(pred, "rgb", "pred"), _field(target, "rgb", "target")
    images = compare_images(a, b, mask=m, **image_kw) if a is not None and b is not None else None
    return images, compare_depth(_field(pred, "depth", "pred"), _field(target, "depth", "target"), valid=valid, align=align)


def latent_depth(latents, depth_scale, depth_shift, foreground=(0.02, 0.98)):
    """(.., 5, S, S) latents -> (metric depth (.., S, S), foreground (.., S, S) bool) as ``fuse_views`` reads the depth channel:
    d = clamp((lat4 + 1) / 2, 0, 1), depth = d * depth_scale + depth_shift, foreground = foreground[0] < d < foreground[1]."""
    if not torch.is_tensor(latents) or latents.dim() < 3 or latents.shape[-3] != 5:
        got = tuple(latents.shape) if torch.is_tensor(latents) else type(latents).__name__
        raise ValueError(f"latents of shape {got}: need (.., 5, S, S)")
    lo, hi = (float(v) for v in foreground)
    if not lo < hi:
        raise ValueError(f"foreground = {foreground}: need lo < hi")
    d = torch.clamp((latents[..., 4, :, :].float() + 1.0) / 2.0, 0.0, 1.0)
    return d * float(depth_scale) + float(depth_shift), (d > lo) & (d < hi)
