"""Test infrastructure of the view-metric entries (include/mvd_hip.h: mvd_image_metrics, mvd_depth_metrics): the case tables and two
oracles.  Importable without a GPU; not collected by pytest.

THE RULES, restated from the header.
  Squared error: count = the pixels the mask counts; sq_sum = the sum over them and all channels of d * d, d = double(a) - double(b).
  SSIM per (image, channel) plane, "valid" region of Ho x Wo = (H - window + 1) x (W - window + 1) positions: the five maps x, y, xx, xy,
    yy in fp64 (exact); each filtered horizontally, taps ascending from 0.0, then vertically the same way; sxx = E[xx] - mx mx, sxy, syy
    likewise; ssim = ((2 mx my + c1) (2 sxy + c2)) / ((mx mx + my my + c1) (sxx + syy + c2)).  A position counts when the mask counts
    its centre pixel; ssim_count = the counting positions, ssim_sum = the sum of ssim over channels and counting positions.
  Depth: a pixel counts when valid, both depths finite and > 0.  Pass 1: n, Sp, St, Spp, Spt; NONE (1, 0); SCALE (Spt / Spp, 0);
    SCALE_SHIFT det = n Spp - Sp Sp, s = (n Spt - Sp St) / det, b = (Spp St - Sp Spt) / det, NaN unless det > 0; GIVEN: as passed.
    Pass 2: q = s p + b; not > 0: dropped; else d = q - t and the sums |d| / t, d d / t, d d, l l with l = log q - log t, the counts of
    r = max(q / t, t / q) below 1.25, 1.5625, 1.953125, the pixels summed.

(a) `ssim_map_a`, `image_a`, `depth_a`: the rules in numpy float64, operation for operation -- every + - * / of numpy rounds once, as the
    library's do, and a filter is a loop of vector multiply-adds in tap order, never a convolution call.  Sums are math.fsum of the terms.
(b) `ssim_map_b`, `depth_b`: independent.  A direct 2-D window -- scipy.signal.correlate2d(.., 'valid') with the outer product of the
    table -- for the moments; math.fsum for every sum; the fit solved in exact rational arithmetic; mpmath for the logs.

Bounds, none taken from what the kernels give (u = 2^-53):
  ssim_map           EQUAL to (a) in bits: the path uses only + - * /.
  a sum of n terms   within n * 2^-52 * sum|term| of fsum, in any order (`sum_bound`): n - 1 additions of relative error u each perturb the
                     result by at most (n - 1) u sum|term| to first order; 2^-52 = 2 u covers the higher orders for every n < 2^26.
                     sq_sum's terms are those of (a) exactly; ssim_sum's are the map values, equal in bits.
  (a) against (b)    on the map (`ssim_ab_bound`), from the term counts: a moment is a sum of window^2 products either way; the separable
                     form rounds each of its 2 window products and 2 window additions, the direct one window^2 of each and the outer
                     product once, so the two differ by at most g = (window^2 + 4 window + 2) u times the largest |map| value in the
                     window -- dE = g M^2 for the second moments, dm = g M for the means, M = max(1, max |x|, max |y|) over the image.
                     Then ds = dE + 2 |m| dm + dm^2 for each of sxx, sxy, syy (|m| the larger mean), and through the quotient
                     A1 A2 / (B1 B2), A1 = 2 mx my + c1, A2 = 2 sxy + c2, B1 = mx mx + my my + c1, B2 = sxx + syy + c2:
                       dA1 = dB1 = 2 (|mx| + |my|) dm + 2 dm^2, dA2 = dB2 = 2 ds,
                       d ssim <= (|A2| dA1 + |A1| dA2) / (B1 B2) + |ssim| (dB1 / B1 + dB2 / B2),
                     doubled for the second order, plus 8 ulp of the value for the formula's own roundings.  At window 11 on [0, 1]
                     images that is ~1e-10 where the variance is small against c2; about 1e-12 was seen.
  depth fit          against the exact rational solution of the same sums (`fit_bound`): the device sums have relative error
                     e1 = n * 2^-52 (positive terms).  SCALE: |ds| <= |s| (2 e1 + 2 u).  SCALE_SHIFT: with e = 2 e1 + 4 u,
                     d det = (n Spp + Sp^2) e, d num_s = (n Spt + Sp St) e, d num_b = (Spp St + Sp Spt) e and
                     |ds| <= 2 (d num_s + |s| d det) / det + ulp(s), |db| alike: (n Spp + Sp^2) / det is the condition number of the
                     2 x 2 system that scales it.
  depth pass 2       against (a) evaluated WITH THE FIT THE KERNEL RETURNED: then q, d, the ratios, the dropped set and the three delta
                     counts are equal exactly (only + - * / and comparisons), no pixel left out, and the first three sums obey
                     `sum_bound`.  The device log is the one operation that cannot be derived here: its largest error against mpmath
                     on these inputs is measured on the GPU (LOG_ULPS_MEASURED, tests/test_gpu_view_metrics.py measures it again and
                     holds it to this figure) and FOUR times that is allowed per logarithm (`log_sum_bound`): the oracle's own log is
                     mpmath's rounded once (0.5 ulp), so device and oracle differ by at most LOG_ULPS_MEASURED + 0.5 <= 4 *
                     LOG_ULPS_MEASURED ulp;  dl = 4 U (ulp(log q) + ulp(log t)) + ulp(l),  d(l l) = 2 |l| dl + dl^2 + ulp(l l).
"""
import fractions
import functools
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from mvdfusion_amd.view_metrics import ssim_window

TILE_W, TILE_H, CHUNK, MAX_WINDOW = 32, 16, 2048, 33      # MVD_SSIM_TILE_W, _TILE_H, MVD_METRIC_CHUNK, MVD_SSIM_MAX_WINDOW
ALIGN_NONE, ALIGN_SCALE, ALIGN_SCALE_SHIFT, ALIGN_GIVEN = 0, 1, 2, 3
THRESHOLDS = (1.25, 1.5625, 1.953125)
C1, C2 = 0.01 ** 2, 0.03 ** 2
U = 2.0 ** -53
LOG_ULPS_MEASURED = 0.62     # the device log's largest error in ulp against mpmath on the depth cases' 16 280 inputs: 0.6178 on an MI355X
LOG_ULPS_ALLOWED = 4.0 * LOG_ULPS_MEASURED


# ------------------------------------------------------------------------------------------------ images
@dataclass
class ImageCase:
    """The arguments of one mvd_image_metrics call as CPU numpy data."""
    a: np.ndarray                       # (B, C, H, W) fp32
    b: np.ndarray
    mask: Optional[np.ndarray]          # (B, H, W) uint8 or None
    weights: Optional[tuple]            # the window table, or None for no SSIM
    c1: float = C1
    c2: float = C2

    @property
    def shape(self):
        return self.a.shape

    @property
    def window(self):
        return len(self.weights) if self.weights is not None else 0


def _images(seed, B, C, H, W):
    rng = np.random.default_rng(seed)
    a = rng.random((B, C, H, W), dtype=np.float32)
    b = np.clip(a + 0.1 * rng.standard_normal((B, C, H, W)).astype(np.float32), 0.0, 1.0).astype(np.float32)
    return a, b


def _random_mask(seed, B, H, W):
    return (np.random.default_rng(seed).random((B, H, W)) < 0.6).astype(np.uint8)


def _sized(seed, Ho, Wo, window, C=1, B=1, sigma=1.5, mask=None):
    H, W = Ho + window - 1, Wo + window - 1
    a, b = _images(seed, B, C, H, W)
    m = _random_mask(seed + 1000, B, H, W) if mask == "random" else mask
    return ImageCase(a, b, m, ssim_window(window, sigma))


def _flat(va, vb, noise=0.0):
    a = np.full((1, 1, 40, 37), va, np.float32)
    b = np.full((1, 1, 40, 37), vb, np.float32)
    if noise:
        a = (a + noise * np.random.default_rng(5).standard_normal(a.shape)).astype(np.float32)
    return ImageCase(a, b, None, ssim_window(11, 1.5))


def _masked(kind):
    a, b = _images(40, 1, 3, 21, 30)
    m = np.zeros((1, 21, 30), np.uint8)
    if kind == "one":
        m[:] = 1
    elif kind == "single":
        m[0, 10, 17] = 1
    elif kind == "border":
        m[0, 2, 28] = 1      # inside the window // 2 = 5 pixels that SSIM crops: counted by the squared error, by no window position
    return ImageCase(a, b, m, ssim_window(11, 1.5))


def _with_nan(under):
    a, b = _images(41, 2, 3, 20, 23)
    m = np.ones((2, 20, 23), np.uint8)
    m[:, 9, 11] = 0
    m[1, 3:6, 2:9] = 0
    a[1, 2, 9, 12 if under else 11] = np.nan      # image 0 stays clean either way; (9, 11) is outside the mask, (9, 12) under it
    return ImageCase(a, b, m, ssim_window(11, 1.5))


def _identical():
    a, _ = _images(42, 1, 3, 19, 26)
    return ImageCase(a, a.copy(), None, ssim_window(11, 1.5))


IMAGE_CASES = {
    # Ho in {1, T - 1, T, T + 1} for TILE_H = 16, Wo likewise for TILE_W = 32, H != W throughout; windows 3, 11, 33 and the uniform one
    "w11_1x31": lambda: _sized(1, 1, 31, 11),
    "w11_15x33_c3": lambda: _sized(2, 15, 33, 11, C=3),
    "w11_16x32_b5_masked": lambda: _sized(3, 16, 32, 11, B=5, mask="random"),
    "w11_17x31_c3_masked": lambda: _sized(4, 17, 31, 11, C=3, mask="random"),
    "w11_17x1": lambda: _sized(5, 17, 1, 11),
    "w3_17x33_c3": lambda: _sized(6, 17, 33, 3, C=3),
    "w3_33x65_tiles": lambda: _sized(7, 33, 65, 3, B=2, mask="random"),      # 3 x 3 tiles and two chunks of 2048 pixels per image
    "w33_15x32": lambda: _sized(8, 15, 32, 33),
    "w33_1x2": lambda: _sized(9, 1, 2, 33, C=3),
    "uniform7_16x31": lambda: _sized(10, 16, 31, 7, sigma=None),
    "no_ssim": lambda: ImageCase(*_images(11, 2, 3, 5, 9), _random_mask(12, 2, 5, 9), None),
    "b0": lambda: ImageCase(np.zeros((0, 3, 12, 14), np.float32), np.zeros((0, 3, 12, 14), np.float32), None, ssim_window(11, 1.5)),
    "mask_zero": lambda: _masked("zero"),
    "mask_one": lambda: _masked("one"),
    "mask_single": lambda: _masked("single"),
    "mask_border": lambda: _masked("border"),
    "identical": _identical,
    "constant": lambda: _flat(0.25, 0.75),
    "near_white": lambda: _flat(0.999, 1.0),
    "near_flat_noise": lambda: _flat(0.7, 0.7, noise=1e-3),      # the image of the fp32-accumulation figure (tests/test_cpu_view_metrics.py)
    "nan_under_mask": lambda: _with_nan(True),
    "nan_outside_mask": lambda: _with_nan(False),
}


@functools.lru_cache(maxsize=None)
def image_case(name):
    return IMAGE_CASES[name]()


def filter_valid(m, w, dtype=np.float64):
    """The separable filter of the rule on the last two axes of m: horizontal then vertical, taps ascending from 0.0, in dtype."""
    n = len(w)
    H, W = m.shape[-2:]
    Ho, Wo = H - n + 1, W - n + 1
    h = np.zeros(m.shape[:-1] + (Wo,), dtype)
    for k in range(n):
        h = h + w[k] * m[..., :, k:k + Wo]
    v = np.zeros(m.shape[:-2] + (Ho, Wo), dtype)
    for k in range(n):
        v = v + w[k] * h[..., k:k + Ho, :]
    return v


def ssim_formula(mx, my, exx, exy, eyy, c1, c2):
    sxx, sxy, syy = exx - mx * mx, exy - mx * my, eyy - my * my
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((2.0 * mx * my + c1) * (2.0 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))


def ssim_map_a(case, dtype=np.float64):
    """(a): the map (B, C, Ho, Wo) by the rule.  dtype=np.float32 forms and accumulates the moments in fp32 instead -- what a user's
    fp32 conv2d does, the figure that tests/test_cpu_view_metrics.py keeps on record."""
    x, y = case.a.astype(dtype), case.b.astype(dtype)
    w = [dtype(v) for v in case.weights]
    with np.errstate(invalid="ignore"):
        e = [filter_valid(m, w, dtype) for m in (x, y, x * x, x * y, y * y)]
        return ssim_formula(*e, dtype(case.c1), dtype(case.c2))


def ssim_map_b(case):
    """(b): the five moments by a direct 2-D window (scipy.signal.correlate2d 'valid' with the outer product of the table)."""
    from scipy.signal import correlate2d
    x, y = case.a.astype(np.float64), case.b.astype(np.float64)
    k2 = np.outer(case.weights, case.weights)
    B, C = x.shape[:2]
    out = []
    for m in (x, y, x * x, x * y, y * y):
        out.append(np.stack([np.stack([correlate2d(m[i, c], k2, mode="valid") for c in range(C)]) for i in range(B)]))
    return ssim_formula(*out, case.c1, case.c2)


def ssim_ab_bound(case, ssim):
    """The derived bound on |(a) - (b)| per map value (module docstring)."""
    n = case.window
    x, y = case.a.astype(np.float64), case.b.astype(np.float64)
    M = max(1.0, float(np.nanmax(np.abs(x))), float(np.nanmax(np.abs(y))))
    g = (n * n + 4 * n + 2) * U
    dE, dm = g * M * M, g * M
    w = list(case.weights)
    mx, my = filter_valid(x, w), filter_valid(y, w)
    exx, exy, eyy = filter_valid(x * x, w), filter_valid(x * y, w), filter_valid(y * y, w)
    sxx, sxy, syy = exx - mx * mx, exy - mx * my, eyy - my * my
    ds = dE + 2.0 * np.maximum(np.abs(mx), np.abs(my)) * dm + dm * dm
    A1, A2 = 2.0 * mx * my + case.c1, 2.0 * sxy + case.c2
    B1, B2 = mx * mx + my * my + case.c1, sxx + syy + case.c2
    dA1 = 2.0 * (np.abs(mx) + np.abs(my)) * dm + 2.0 * dm * dm
    dA2 = 2.0 * ds
    first = (np.abs(A2) * dA1 + np.abs(A1) * dA2) / (B1 * B2) + np.abs(ssim) * (dA1 / B1 + dA2 / B2)
    return 2.0 * first + 8.0 * np.spacing(np.abs(ssim))


def centre_mask(case):
    """(B, Ho, Wo) bool: the window positions that count -- the mask cropped by window // 2 on each side."""
    B, C, H, W = case.shape
    n, h = case.window, case.window // 2
    if case.mask is None:
        return np.ones((B, H - n + 1, W - n + 1), bool)
    return case.mask[:, h:H - h, h:W - h] != 0


def fsum_terms(terms):
    """(fsum, the bound n * 2^-52 * sum|term|) of a flat array of terms; NaN when a term is not finite."""
    terms = np.asarray(terms, np.float64).ravel()
    if not np.all(np.isfinite(terms)):
        return float("nan"), float("nan")
    return math.fsum(terms.tolist()), len(terms) * 2.0 ** -52 * math.fsum(np.abs(terms).tolist())


def image_a(case, ssim_map=None):
    """(a): per image dict(count, sq_sum, sq_bound, ssim_count, ssim_sum, ssim_bound), the sums by fsum with their bounds.  ssim_map: the
    map to take the SSIM terms from (the kernel's, once it is known to equal (a) in bits); (a)'s own by default."""
    B, C, H, W = case.shape
    x, y = case.a.astype(np.float64), case.b.astype(np.float64)
    d = x - y
    with np.errstate(invalid="ignore"):
        dd = d * d
    counted = np.ones((B, H, W), bool) if case.mask is None else case.mask != 0
    rows = []
    if case.window and ssim_map is None and B:
        ssim_map = ssim_map_a(case)
    centres = centre_mask(case) if case.window else None
    for i in range(B):
        s, sb = fsum_terms(dd[i][:, counted[i]])
        row = dict(count=int(counted[i].sum()), sq_sum=s, sq_bound=sb)
        if case.window:
            t, tb = fsum_terms(ssim_map[i][:, centres[i]])
            row.update(ssim_count=int(centres[i].sum()), ssim_sum=t, ssim_bound=tb)
        rows.append(row)
    return rows


# ------------------------------------------------------------------------------------------------ depth
@dataclass
class DepthCase:
    """The arguments of one mvd_depth_metrics call as CPU numpy data."""
    pred: np.ndarray                    # (B, H, W) fp32
    target: np.ndarray
    valid: Optional[np.ndarray]         # (B, H, W) uint8 or None
    align: int
    fit_in: Optional[np.ndarray] = None      # (B, 2) fp64 with ALIGN_GIVEN
    random: bool = False                # a case of random depths: no pixel sits on a delta threshold (tests/test_cpu_view_metrics.py)


def _depths(seed, B, H, W, align, valid=False, **kw):
    rng = np.random.default_rng(seed)
    t = (0.5 + 2.0 * rng.random((B, H, W))).astype(np.float32)
    p = (t * (0.8 + 0.9 * rng.random((B, H, W))) * 1.3 + 0.05).astype(np.float32)
    v = (rng.random((B, H, W)) < 0.7).astype(np.uint8) if valid else None
    return DepthCase(p, t, v, align, random=True, **kw)


def _bad_values():
    c = _depths(23, 2, 7, 11, ALIGN_SCALE, valid=True)
    c.random = False
    c.pred[0, 0, :6] = [np.inf, -1.0, 0.0, np.nan, -np.inf, 1.0]
    c.target[0, 1, :6] = [np.inf, -2.0, 0.0, np.nan, 1.0, -0.0]
    c.valid[0, :2, :6] = 1
    return c


def _one_pixel(align):
    c = _depths(24, 1, 5, 6, align)
    c.random = False
    c.valid = np.zeros((1, 5, 6), np.uint8)
    c.valid[0, 3, 2] = 1
    return c


def _dyadic():
    p = np.full((1, 3, 4), 4.0, np.float32)
    t = np.full((1, 3, 4), 5.0, np.float32)      # t / p = 1.25 exactly: on the strict threshold, not below it
    t[0, 0, 0] = 4.0
    return DepthCase(p, t, None, ALIGN_NONE)


def _negative_fit():
    c = _depths(25, 3, 8, 9, ALIGN_GIVEN, valid=True, fit_in=np.array([[1.0, -2.0], [-0.5, 1.0], [1.25, 0.0]]))
    c.random = False
    return c


def _all_invalid():
    c = _depths(26, 2, 4, 5, ALIGN_SCALE_SHIFT)
    c.random = False
    c.valid = np.zeros((2, 4, 5), np.uint8)
    return c


DEPTH_CASES = {
    "none_b5": lambda: _depths(20, 5, 9, 13, ALIGN_NONE, valid=True),
    "scale_chunks": lambda: _depths(21, 2, 40, 53, ALIGN_SCALE, valid=True),      # 2 120 pixels: two chunks of 2048
    "scale_shift": lambda: _depths(22, 3, 17, 8, ALIGN_SCALE_SHIFT),
    "scale_shift_2048": lambda: _depths(27, 1, 32, 64, ALIGN_SCALE_SHIFT),          # exactly one chunk
    "scale_shift_2049": lambda: _depths(28, 1, 1, 2049, ALIGN_SCALE_SHIFT),         # one pixel into the second
    "given": lambda: _depths(29, 2, 6, 7, ALIGN_GIVEN, fit_in=np.array([[1.1, 0.0], [0.9, 0.125]])),
    "bad_values": _bad_values,
    "all_invalid": _all_invalid,
    "one_pixel_scale_shift": lambda: _one_pixel(ALIGN_SCALE_SHIFT),      # det is exactly 0: the fit is NaN and the pixel is dropped
    "one_pixel_scale": lambda: _one_pixel(ALIGN_SCALE),
    "dyadic_threshold": _dyadic,
    "negative_fit": _negative_fit,
    "b0": lambda: DepthCase(np.zeros((0, 4, 5), np.float32), np.zeros((0, 4, 5), np.float32), None, ALIGN_SCALE),
}


@functools.lru_cache(maxsize=None)
def depth_case(name):
    return DEPTH_CASES[name]()


def counted_pixels(case):
    p, t = case.pred, case.target
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(p) & np.isfinite(t) & (p > 0) & (t > 0)
    return ok if case.valid is None else ok & (case.valid != 0)


def fit_exact(case):
    """(b): per image (s, b, bound_s, bound_b) -- the fit solved in exact rational arithmetic on the exact sums, rounded once, and the
    derived bounds on the device's fit (module docstring).  NaN where the rule says NaN."""
    F = fractions.Fraction
    ok = counted_pixels(case)
    out = []
    for i in range(case.pred.shape[0]):
        if case.align == ALIGN_GIVEN:
            out.append((float(case.fit_in[i, 0]), float(case.fit_in[i, 1]), 0.0, 0.0))
            continue
        p = [F(float(v)) for v in case.pred[i][ok[i]]]
        t = [F(float(v)) for v in case.target[i][ok[i]]]
        n = len(p)
        Sp, St, Spp, Spt = sum(p, F(0)), sum(t, F(0)), sum((v * v for v in p), F(0)), sum((a * b for a, b in zip(p, t)), F(0))
        e1 = n * 2.0 ** -52
        if case.align == ALIGN_NONE:
            out.append((1.0, 0.0, 0.0, 0.0))
        elif case.align == ALIGN_SCALE:
            if n == 0:
                out.append((float("nan"), 0.0, 0.0, 0.0))
            else:
                s = float(Spt / Spp)
                out.append((s, 0.0, abs(s) * (2 * e1 + 2 * U), 0.0))
        else:
            det = n * Spp - Sp * Sp
            if det <= 0:
                out.append((float("nan"), float("nan"), 0.0, 0.0))
                continue
            s, b = float((n * Spt - Sp * St) / det), float((Spp * St - Sp * Spt) / det)
            e = 2 * e1 + 4 * U
            ddet, dns, dnb = float(n * Spp + Sp * Sp) * e, float(n * Spt + Sp * St) * e, float(Spp * St + Sp * Spt) * e
            fd = float(det)
            out.append((s, b, 2 * (dns + abs(s) * ddet) / fd + np.spacing(abs(s)), 2 * (dnb + abs(b) * ddet) / fd + np.spacing(abs(b))))
    return out


def fit_a(case):
    """(a) of pass 1: per image (s, b) -- the four sums by fsum, then the rule's expressions in float64 in the header's order."""
    ok = counted_pixels(case)
    out = []
    for i in range(case.pred.shape[0]):
        if case.align == ALIGN_GIVEN:
            out.append((float(case.fit_in[i, 0]), float(case.fit_in[i, 1])))
            continue
        p, t = case.pred[i][ok[i]].astype(np.float64), case.target[i][ok[i]].astype(np.float64)
        n = float(len(p))
        Sp, St, Spp, Spt = (math.fsum(v.tolist()) for v in (p, t, p * p, p * t))
        s, b = 1.0, 0.0
        if case.align == ALIGN_SCALE:
            s = Spt / Spp if Spp else float("nan")
        if case.align == ALIGN_SCALE_SHIFT:
            det = n * Spp - Sp * Sp
            s, b = ((n * Spt - Sp * St) / det, (Spp * St - Sp * Spt) / det) if det > 0.0 else (float("nan"), float("nan"))
        out.append((s, b))
    return out


@functools.lru_cache(maxsize=1 << 16)
def log_mp(v):
    """The natural logarithm of the float v by mpmath at 60 digits, rounded once to fp64."""
    import mpmath
    with mpmath.workprec(200):
        return float(mpmath.log(mpmath.mpf(v)))


def log_ulps(values, device_logs):
    """The largest error of device_logs against mpmath's logarithm of values, in ulp of the correctly rounded result."""
    import mpmath
    worst = 0.0
    with mpmath.workprec(200):
        for v, got in zip(np.asarray(values, np.float64).tolist(), np.asarray(device_logs, np.float64).tolist()):
            true = mpmath.log(mpmath.mpf(v))
            ulp = float(np.spacing(abs(float(true)))) or 2.0 ** -1074
            worst = max(worst, float(abs(mpmath.mpf(got) - true) / ulp))
    return worst


def depth_a(case, fit):
    """(a) of pass 2 with the fit (B, 2) given: per image dict(q, kept, counts (5,), sums (4,), bounds (4,)).  q = s p + b on the counted
    pixels in their row-major order; kept: which of them are summed; the sums by fsum; the fourth bound is `log_sum_bound`."""
    ok = counted_pixels(case)
    rows = []
    for i in range(case.pred.shape[0]):
        p, t = case.pred[i][ok[i]].astype(np.float64), case.target[i][ok[i]].astype(np.float64)
        s, b = np.float64(fit[i][0]), np.float64(fit[i][1])
        with np.errstate(invalid="ignore"):
            q = s * p + b
            kept = q > 0
        qk, tk = q[kept], t[kept]
        d = qk - tk
        dd = d * d
        r = np.maximum(qk / tk, tk / qk)
        lq, lt = np.array([log_mp(v) for v in qk.tolist()]), np.array([log_mp(v) for v in tk.tolist()])
        l = lq - lt
        ll = l * l
        terms = (np.abs(d) / tk, dd / tk, dd, ll)
        sums, bounds = zip(*(fsum_terms(x) for x in terms)) if len(qk) else ((0.0,) * 4, (0.0,) * 4)
        dl = LOG_ULPS_ALLOWED * (np.spacing(np.abs(lq)) + np.spacing(np.abs(lt))) + np.spacing(np.abs(l))
        dll = 2.0 * np.abs(l) * dl + dl * dl + np.spacing(ll)
        bounds = list(bounds)
        bounds[3] = bounds[3] + math.fsum(dll.tolist()) * (1.0 + len(qk) * 2.0 ** -52)
        counts = [int((r < th).sum()) for th in THRESHOLDS] + [int(kept.sum()), int((~kept).sum())]
        rows.append(dict(q=q, kept=kept, ratio=r, counts=np.array(counts, np.int64), sums=np.array(sums), bounds=np.array(bounds)))
    return rows


def depth_b(case):
    """(b): the whole of mvd_depth_metrics with the exact rational fit -- per image the record of `depth_a` plus fit = (s, b)."""
    fits = fit_exact(case)
    rows = depth_a(case, [(s, b) for s, b, _, _ in fits])
    for row, f in zip(rows, fits):
        row["fit"] = f
    return rows
