"""The view metrics without a GPU: the two oracles of tests/view_metrics_f64.py against each other within the bounds that file derives,
the window table, the analytic cases, the argument checks of mvdfusion_amd/view_metrics.py, the mask modes of compare_views, and the
library's refusals (every check fires before anything is enqueued).

Kept on record: on a near-flat image (40 x 37, 0.7 plus 1e-3 noise against flat 0.7, the 11-tap sigma = 1.5 window) fp32 accumulation of
the five window moments moves the SSIM map by 2.4e-4 against float64 -- the cancellation in E[x^2] - mu^2 is measured against
C2 = 9e-4 -- while the separable and the direct 2-D form in float64 agree to 1.4e-12 on the same image.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import view_metrics_f64 as V
from mvdfusion_amd import view_metrics as vm

SSIM_CASES = [n for n in V.IMAGE_CASES if V.image_case(n).window and V.image_case(n).shape[0]]


def _same_or_nan(a, b, bound):
    with np.errstate(invalid="ignore"):
        return bool(np.all((np.abs(a - b) <= bound) | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------------------------------------ the oracles against each other
@pytest.mark.parametrize("name", SSIM_CASES)
def test_separable_and_direct_ssim_agree_within_the_derived_bound(name):
    case = V.image_case(name)
    a, b = V.ssim_map_a(case), V.ssim_map_b(case)
    bound = V.ssim_ab_bound(case, a)
    B, C, H, W = case.shape
    assert a.shape == b.shape == (B, C, H - case.window + 1, W - case.window + 1)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert _same_or_nan(a, b, bound), float(np.nanmax(np.abs(a - b) - bound))
    # the sums of the two maps: each within its own fsum bound is exact here (fsum), so they differ by at most the sum of the map bounds
    for ra, rb, i in zip(V.image_a(case, a), V.image_a(case, b), range(B)):
        assert ra["count"] == rb["count"] and ra["ssim_count"] == rb["ssim_count"]
        if math.isnan(ra["ssim_sum"]):
            assert math.isnan(rb["ssim_sum"])
            continue
        centres = V.centre_mask(case)[i]
        assert abs(ra["ssim_sum"] - rb["ssim_sum"]) <= float(bound[i][:, centres].sum()) + ra["ssim_bound"]


@pytest.mark.parametrize("name", V.DEPTH_CASES)
def test_depth_fit_in_float64_meets_the_exact_rational_fit(name):
    case = V.depth_case(name)
    for (s, b), (se, be, ds, db) in zip(V.fit_a(case), V.fit_exact(case)):
        for got, want, bound in ((s, se, ds), (b, be, db)):
            assert (math.isnan(got) and math.isnan(want)) or abs(got - want) <= bound, (got, want, bound)
    # pass 2 at (a)'s fit and at the exact one: the same pixels kept wherever the two fits agree in bits; the counts add up either way
    ok = V.counted_pixels(case)
    for i, row in enumerate(V.depth_b(case)):
        assert row["counts"][3] + row["counts"][4] == int(ok[i].sum())
        assert row["counts"][0] <= row["counts"][1] <= row["counts"][2] <= row["counts"][3]


def test_random_depth_cases_have_no_pixel_on_a_delta_threshold():
    names = [n for n in V.DEPTH_CASES if V.depth_case(n).random]
    assert len(names) >= 5
    for name in names:
        case = V.depth_case(name)
        for fit in (V.fit_a(case), [(s, b) for s, b, _, _ in V.fit_exact(case)]):
            for row in V.depth_a(case, fit):
                assert len(row["ratio"]) > 0
                for th in V.THRESHOLDS:
                    assert int((row["ratio"] == th).sum()) == 0, (name, th)


# ------------------------------------------------------------------------------------------------ the window table
@pytest.mark.parametrize("window, sigma", [(3, 1.5), (11, 1.5), (33, 1.5), (33, 5.0), (7, None), (11, None), (33, None)])
def test_window_table_sums_to_one_and_is_symmetric(window, sigma):
    w = vm.ssim_window(window, sigma)
    assert isinstance(w, tuple) and len(w) == window and all(type(v) is float and v > 0 for v in w)
    assert w == w[::-1]
    # the table's own sum (fsum: a left-to-right fp64 sum of 33 equal weights is three ulp off by its own roundings) within one ulp of 1
    assert abs(math.fsum(w) - 1.0) <= 2.0 ** -52
    if sigma is None:
        assert all(v == 1.0 / window for v in w)
    else:
        assert max(w) == w[window // 2] and all(w[i] < w[i + 1] for i in range(window // 2))


# ------------------------------------------------------------------------------------------------ the analytic cases
def test_identical_images_give_exactly_one_everywhere():
    case = V.image_case("identical")
    assert bool(np.all(V.ssim_map_a(case) == 1.0))      # 2 mu mu == mu mu + mu mu and 2 s == s + s in floating point
    row = V.image_a(case)[0]
    assert row["sq_sum"] == 0.0 and row["ssim_sum"] == 3.0 * row["ssim_count"]


@pytest.mark.parametrize("name, va, vb", [("constant", 0.25, 0.75), ("near_white", 0.999, 1.0)])
def test_constant_images_meet_the_closed_form(name, va, vb):
    case = V.image_case(name)
    x, y = float(np.float32(va)), float(np.float32(vb))
    want = (2.0 * x * y + case.c1) / (x * x + y * y + case.c1)      # both variances and the covariance are 0: the second factor is 1
    got = V.ssim_map_a(case)
    assert _same_or_nan(got, np.full_like(got, want), V.ssim_ab_bound(case, got))
    row = V.image_a(case)[0]
    d = x - y
    assert abs(row["sq_sum"] - row["count"] * d * d) <= row["count"] * 2.0 ** -52 * row["sq_sum"]


def test_mask_cases_count_what_the_rule_says():
    for name, count, centres in (("mask_zero", 0, 0), ("mask_one", 21 * 30, 11 * 20), ("mask_single", 1, 1), ("mask_border", 1, 0)):
        row = V.image_a(V.image_case(name))[0]
        assert (row["count"], row["ssim_count"]) == (count, centres), name
    under, outside = V.image_a(V.image_case("nan_under_mask")), V.image_a(V.image_case("nan_outside_mask"))
    assert all(math.isfinite(r["sq_sum"]) and math.isfinite(r["ssim_sum"]) for r in (under[0], outside[0]))      # image 0 is clean
    assert math.isnan(under[1]["sq_sum"]) and math.isnan(under[1]["ssim_sum"])
    assert math.isfinite(outside[1]["sq_sum"]) and math.isnan(outside[1]["ssim_sum"])      # windows of counted centres still hold the pixel


def test_depth_analytic_cases():
    row = V.depth_b(V.depth_case("dyadic_threshold"))[0]
    assert row["counts"].tolist() == [1, 12, 12, 12, 0]      # the eleven pixels with t / p == 1.25 exactly are not below 1.25
    assert row["sums"][0] == pytest.approx(11 * 0.2, abs=1e-15) and row["sums"][2] == 11.0
    assert row["sums"][3] == pytest.approx(11 * math.log(1.25) ** 2, rel=1e-14)
    row = V.depth_b(V.depth_case("one_pixel_scale_shift"))[0]
    assert math.isnan(row["fit"][0]) and math.isnan(row["fit"][1]) and row["counts"].tolist() == [0, 0, 0, 0, 1]
    for row in V.depth_b(V.depth_case("all_invalid")):
        assert row["counts"].tolist() == [0] * 5 and math.isnan(row["fit"][0])
    rows = V.depth_b(V.depth_case("negative_fit"))
    assert all(r["counts"][4] > 0 for r in rows[:2]) and rows[2]["counts"][4] == 0
    case = V.depth_case("bad_values")
    ok = V.counted_pixels(case)
    assert not ok[0, 0, :5].any() and not ok[0, 1, :4].any() and not ok[0, 1, 5]


def test_fp32_moments_move_the_ssim_map_and_float64_moments_do_not():
    case = V.image_case("near_flat_noise")
    a64 = V.ssim_map_a(case)
    a32 = V.ssim_map_a(case, np.float32).astype(np.float64)
    direct = V.ssim_map_b(case)
    moved, agree = float(np.abs(a32 - a64).max()), float(np.abs(direct - a64).max())
    print(f"FP32 MOMENTS near-flat 40 x 37: |fp32 - fp64| {moved:.3e} | |separable - direct| in fp64 {agree:.3e}")
    assert moved > 1e-4                      # measured here: 2.4e-4
    assert agree < 1e-10 and moved > 1e6 * agree


# ------------------------------------------------------------------------------------------------ the host functions' checks
def test_ssim_window_argument_checks():
    for bad in (2, 4, 1, 35, 0, -3, 11.5, True):
        with pytest.raises(ValueError, match="window"):
            vm.ssim_window(bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="sigma"):
            vm.ssim_window(11, bad)


def test_compare_images_argument_checks():
    a = torch.rand(2, 3, 16, 20)
    bad = [
        (dict(pred=a.numpy()), "tensors"),
        (dict(target=a[:, :, :, :19]), "equal shapes"),
        (dict(pred=a[0, 0], target=a[0, 0]), "at least 3"),
        (dict(pred=torch.rand(2, 0, 16, 20), target=torch.rand(2, 0, 16, 20)), "C >= 1"),
        (dict(pred=torch.zeros(65536, 1, 1, 1), target=torch.zeros(65536, 1, 1, 1), window=None), "65535"),
        (dict(pred=torch.zeros(1, 1, 0, 4), target=torch.zeros(1, 1, 0, 4)), r"\[1, 32768\]"),
        (dict(data_range=0.0), "data_range"),
        (dict(data_range=float("nan")), "data_range"),
        (dict(window=4), "window = 4"),
        (dict(window=35), "window = 35"),
        (dict(window=17), "window = 17: larger"),
        (dict(sigma=-1.0), "sigma = -1.0"),
        (dict(k1=-0.01), "k1 = -0.01"),
        (dict(k2=float("inf")), "k2 = inf"),
        (dict(window=None, return_map=True), "return_map"),
        (dict(mask=torch.ones(2, 3, 16, 20)), "mask of shape"),
        (dict(mask=torch.ones(2, 16, 19)), "mask of shape"),
        (dict(mask=[1, 2]), "mask of shape"),
    ]
    for kw, match in bad:
        args = dict(pred=a, target=a)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            vm.compare_images(**args)


def test_compare_depth_argument_checks():
    d = torch.rand(3, 8, 9) + 0.5
    bad = [
        (dict(pred=d.numpy()), "tensors"),
        (dict(target=d[:, :7]), "equal shapes"),
        (dict(pred=d[0, 0], target=d[0, 0]), "at least 2"),
        (dict(align="affine"), "align = 'affine'"),
        (dict(align=torch.ones(3)), "align of shape"),
        (dict(align=torch.ones(2, 2)), "align of shape"),
        (dict(valid=torch.ones(3, 8)), "valid of shape"),
        (dict(pred=torch.zeros(65536, 1, 1), target=torch.zeros(65536, 1, 1)), "65535"),
    ]
    for kw, match in bad:
        args = dict(pred=d, target=d)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            vm.compare_depth(**args)


def test_latent_depth_is_fuse_views_reading_of_the_depth_channel():
    lat = torch.zeros(2, 5, 3, 4)
    lat[:, 4] = torch.tensor([-3.0, -1.0, -0.97, 0.0]).expand(2, 3, 4)
    lat[1, 4, 0] = torch.tensor([0.95, 0.97, 1.0, 2.0])
    depth, fg = vm.latent_depth(lat, 2.0, 0.5)
    assert depth.shape == fg.shape == (2, 3, 4)
    assert depth[0, 0].tolist() == [0.5, 0.5, pytest.approx(0.53), 1.5] and fg[0, 0].tolist() == [False, False, False, True]
    assert fg[1, 0].tolist() == [True, False, False, False] and depth[1, 0, 3] == 2.5
    for bad, match in ((torch.zeros(4, 3, 3), "latents of shape"), (None, "latents of shape")):
        with pytest.raises(ValueError, match=match):
            vm.latent_depth(bad, 2.0, 0.5)
    with pytest.raises(ValueError, match="foreground"):
        vm.latent_depth(lat, 2.0, 0.5, foreground=(0.9, 0.1))


def test_compare_views_mask_modes_on_hand_made_records():
    from mvdfusion_amd import fusion
    ph = torch.tensor([[[1, 1, 0, 0]]], dtype=torch.bool)
    th = torch.tensor([[[1, 0, 1, 0]]], dtype=torch.bool)
    extra = torch.tensor([[[1, 1, 1, 0]]], dtype=torch.uint8)
    want = {"both": ([1, 0, 0, 0], [1, 0, 0, 0]), "either": ([1, 1, 1, 0], [1, 0, 0, 0]), "target": ([1, 0, 1, 0], [1, 0, 0, 0]),
            None: (None, [1, 0, 0, 0])}
    for mode, (m, v) in want.items():
        got_m, got_v = vm.view_masks(ph, th, mode)
        assert (got_m is None) if m is None else got_m[0, 0].int().tolist() == m, mode
        assert got_v[0, 0].int().tolist() == v, mode
    got_m, got_v = vm.view_masks(ph, th, extra)
    assert got_m[0, 0].int().tolist() == [1, 1, 1, 0] and got_v[0, 0].int().tolist() == [1, 0, 0, 0]
    got_m, got_v = vm.view_masks(ph, th, torch.tensor([[[0, 1, 1, 1]]]))
    assert got_v[0, 0].int().tolist() == [0, 0, 0, 0]
    for bad, match in (("pred", "mask = 'pred'"), (torch.ones(1, 1, 3), "mask of shape")):
        with pytest.raises(ValueError, match=match):
            vm.view_masks(ph, th, bad)
    with pytest.raises(ValueError, match="hit maps of shapes"):
        vm.view_masks(ph, th[..., :3], "both")
    # the records compare_views takes: both dataclasses and a mapping; a record without depth or hit is refused before the library is called
    depth = torch.ones(1, 1, 4)
    views = fusion.RenderedViews(rgb=None, depth=depth, index=torch.zeros(1, 1, 4, dtype=torch.int32), hit=ph)
    assert vm._field(views, "hit", "pred") is ph and vm._field(views, "rgb", "pred") is None
    assert vm._field(dict(rgb=None, depth=depth, hit=th), "depth", "target") is depth
    with pytest.raises(ValueError, match="target has no 'depth'"):
        vm.compare_views(views, dict(rgb=None, depth=None, hit=th))
    with pytest.raises(ValueError, match="pred has no 'hit'"):
        vm.compare_views(object(), views)


# ------------------------------------------------------------------------------------------------ the C ABI
ENTRY_POINTS = {"mvd_image_metrics_scratch": 5, "mvd_image_metrics": 19, "mvd_depth_metrics_scratch": 3, "mvd_depth_metrics": 14}


def test_entry_points_are_declared_and_exported():
    from conftest import ROOT
    from mvdfusion_amd import hip
    hdr = open(os.path.join(ROOT, "include", "mvd_hip.h")).read()
    for fmt in ("f16", "bf16"):
        so = ctypes.CDLL(hip.LIB_PATHS[fmt])
        for name, nargs in ENTRY_POINTS.items():
            decl = re.search(rf"\b{name}\(([^;]*)\);", hdr)
            assert decl is not None and name in hip.SIGNATURES, name
            assert len(hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == nargs, name
            assert hasattr(so, name), name
    for macro, value in (("MVD_SSIM_MAX_WINDOW", hip.SSIM_MAX_WINDOW), ("MVD_SSIM_TILE_W", hip.SSIM_TILE_W), ("MVD_SSIM_TILE_H", hip.SSIM_TILE_H),
                         ("MVD_METRIC_CHUNK", hip.METRIC_CHUNK), ("MVD_DEPTH_ALIGN_NONE", hip.DEPTH_ALIGN_NONE),
                         ("MVD_DEPTH_ALIGN_SCALE", hip.DEPTH_ALIGN_SCALE), ("MVD_DEPTH_ALIGN_SCALE_SHIFT", hip.DEPTH_ALIGN_SCALE_SHIFT),
                         ("MVD_DEPTH_ALIGN_GIVEN", hip.DEPTH_ALIGN_GIVEN)):
        assert re.search(rf"#define {macro} {value}\b", hdr), macro
    assert (V.TILE_W, V.TILE_H, V.CHUNK, V.MAX_WINDOW) == (hip.SSIM_TILE_W, hip.SSIM_TILE_H, hip.METRIC_CHUNK, hip.SSIM_MAX_WINDOW)
    assert (V.ALIGN_NONE, V.ALIGN_SCALE, V.ALIGN_SCALE_SHIFT, V.ALIGN_GIVEN) == (0, 1, 2, 3) == tuple(
        getattr(hip, "DEPTH_ALIGN_" + k) for k in ("NONE", "SCALE", "SCALE_SHIFT", "GIVEN"))
    from mvdfusion_amd.csrc.build import SOURCES
    assert "view_metrics.hip" in SOURCES


def test_scratch_sizes_follow_the_plan():
    from mvdfusion_amd import hip
    L = hip.lib()
    for B, C, H, W, window in ((1, 1, 11, 41, 11), (5, 3, 256, 256, 11), (2, 1, 35, 67, 3), (3, 3, 5, 9, 0), (1, 1, 33, 34, 33)):
        chunks = -(-H * W // V.CHUNK)
        tiles = (-(-(H - window + 1) // V.TILE_H)) * (-(-(W - window + 1) // V.TILE_W)) if window else 0
        assert L.mvd_image_metrics_scratch(B, C, H, W, window) == 8 * (2 * B * chunks + (C + 1) * B * tiles)
    for args in ((-1, 1, 8, 8, 3), (1, 0, 8, 8, 3), (1, 1, 0, 8, 0), (1, 1, 8, 32769, 0), (256, 256, 8, 8, 0), (1, 1, 8, 8, 4), (1, 1, 8, 8, 35),
                 (1, 1, 8, 10, 9), (1, 1, 8, 8, 1)):
        assert L.mvd_image_metrics_scratch(*args) == 0, args
    for B, H, W in ((1, 1, 1), (2, 40, 53), (5, 256, 256)):
        chunks = -(-H * W // V.CHUNK)
        assert L.mvd_depth_metrics_scratch(B, H, W) == 8 * (2 * B + 14 * B * chunks)
    for args in ((-1, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 32769)):
        assert L.mvd_depth_metrics_scratch(*args) == 0, args


def test_the_library_refuses_bad_arguments_before_any_launch():
    """Every check fires before anything is enqueued, so the refusals can be exercised without a device (host memory stands in)."""
    from mvdfusion_amd import hip
    L = hip.lib()
    buf = torch.zeros(1 << 16)
    p = hip.ptr(buf)
    w11 = (ctypes.c_double * 11)(*vm.ssim_window(11, 1.5))
    nan_w = (ctypes.c_double * 11)(*([0.1] * 5 + [float("nan")] + [0.1] * 5))
    good = dict(a=p, b=p, mask=None, B=1, C=3, H=20, W=24, weights=w11, window=11, c1=V.C1, c2=V.C2, sq=p, count=p, ssum=p, scount=p, smap=p,
                scratch=p, nbytes=1 << 18)
    bad = [dict(a=None), dict(b=None), dict(B=-1), dict(C=0), dict(B=300, C=300), dict(H=0), dict(W=0), dict(H=32769), dict(window=10),
           dict(window=1), dict(window=35), dict(window=21), dict(H=10), dict(W=10), dict(weights=nan_w), dict(c1=float("nan")),
           dict(c2=float("inf")), dict(scratch=None), dict(nbytes=8), dict(scratch=ctypes.c_void_p(buf.data_ptr() + 4))]
    for kw in bad:
        a = dict(good)
        a.update(kw)
        assert L.mvd_image_metrics(*a.values(), None) != 0, kw
        assert b"mvd_image_metrics:" in L.mvd_last_error(), (kw, L.mvd_last_error())
    assert L.mvd_image_metrics(*dict(good, B=0, a=None, b=None, scratch=None, nbytes=0).values(), None) == 0      # B = 0: a successful no-op
    fit = hip.ptr(torch.zeros(8, dtype=torch.float64))
    good = dict(pred=p, target=p, valid=None, B=2, H=8, W=9, align=V.ALIGN_SCALE, fit_in=None, fit=p, sums=p, counts=p, scratch=p, nbytes=1 << 18)
    bad = [dict(pred=None), dict(target=None), dict(B=-1), dict(B=65536), dict(H=0), dict(W=32769), dict(align=-1), dict(align=4),
           dict(align=V.ALIGN_GIVEN), dict(fit_in=fit), dict(scratch=None), dict(nbytes=16), dict(scratch=ctypes.c_void_p(buf.data_ptr() + 4))]
    for kw in bad:
        a = dict(good)
        a.update(kw)
        assert L.mvd_depth_metrics(*a.values(), None) != 0, kw
        assert b"mvd_depth_metrics:" in L.mvd_last_error(), (kw, L.mvd_last_error())
    assert L.mvd_depth_metrics(*dict(good, B=0, pred=None, target=None, scratch=None, nbytes=0).values(), None) == 0
