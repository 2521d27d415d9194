"""The view-metric entries on the GPU: mvd_image_metrics and mvd_depth_metrics (csrc/view_metrics.hip) through the C ABI against oracle
(a) of tests/view_metrics_f64.py, and the host path (view_metrics.compare_images, compare_depth, compare_views, ViewFusion.compare).

Bounds -- none taken from what the kernels give (tests/view_metrics_f64.py derives them):
  ssim_map                   EQUAL to (a) in bits on every value of every case (NaN exactly where (a) has NaN): only + - * /.
  count, ssim_count          equal.
  sq_sum, ssim_sum           within n * 2^-52 * sum|term| of fsum over (a)'s terms; NaN exactly where (a) has a term that is not finite.
  depth fit                  within `fit_exact`'s bound of the exact rational solution (the 2 x 2 system's condition number); NaN alike.
  depth pass 2               against (a) evaluated with the fit the kernel returned: the five counts equal -- q, the ratios and the dropped
                             set are + - * / and comparisons, no pixel left out; the first three sums within the fsum bound; the log sum
                             within that plus FOUR times the measured error of the device log per logarithm.
  bit equalities             two runs; an image alone against the same image inside a batch of 5; each NULL-output subset against the full
                             call; MVD_DEPTH_ALIGN_GIVEN with the fit a call returned against that call.
  refusals                   non-zero, the entry's name in mvd_last_error(), every sentinel-filled buffer untouched.

The device log: `test_device_log_error_is_the_measured_one` measures the largest error of the fp64 logarithm against mpmath on every q and
t the depth cases take a logarithm of (torch.log on the device; `test_the_kernel_log_is_the_measured_log` holds the kernel's own log to
the same bits through one-pixel images).  MEASURED on an MI355X: 16 280 inputs in [0.045, 5.75], largest error 0.6178 ulp, 15 700 correctly rounded;
LOG_ULPS_MEASURED = 0.62 records it and the rmse_log bound allows four times that per logarithm.

Cases: tests/view_metrics_f64.py IMAGE_CASES and DEPTH_CASES -- Ho in {1, 15, 16, 17} and Wo in {1, 31, 32, 33} around the 32 x 16 tile
with H != W, 3 x 3 tiles, windows 3, 11, 33 and the uniform one, C in {1, 3}, B in {0, 1, 2, 5}, masks all zero / all one / one pixel /
one pixel in the cropped border / random, identical, constant and near-white images, a NaN under and outside the mask; depth maps of one
chunk, one pixel more, two chunks, every pixel invalid, one valid pixel (det = 0), inf / NaN / negative / zero depths, the dyadic pair on
the strict 1.25 threshold and given fits that drive q <= 0.

Measured on an MI355X: ssim_map bit-equal to (a) on all 22 image cases; the sums use at most 0.24 of their bound (ssim_sum of the
one-pixel mask), the fit at most 0.009, the depth sums at most 0.03; the sphere shifted by one pixel scores PSNR 20.6, SSIM 0.68,
abs_rel 0.012.  The 48 tests take 6.7 s, 4.4 s of them the decoder of the ViewFusion.compare test.
"""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

import view_metrics_f64 as V

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
IMAGE_OUTPUTS = ("sq_sum", "count", "ssim_sum", "ssim_count", "ssim_map")
DEPTH_OUTPUTS = ("fit", "sums", "counts")


@pytest.fixture(scope="module")
def hip():
    from mvdfusion_amd import hip as h
    h.lib()
    return h


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).contiguous().cuda()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(x, y, keys):
    return all(torch.equal(_bits(x[k]), _bits(y[k])) for k in keys)


def _p(hip, t):
    return None if t is None or t.numel() == 0 else hip.ptr(t)


# ------------------------------------------------------------------------------------------------ the image entry
def _image_buffers(hip, case, rows=None):
    B, C, H, W = case.shape if rows is None else (len(rows), *case.shape[1:])
    n = case.window
    f = lambda *s: torch.full(s, SENTINEL, dtype=torch.float64, device="cuda")
    i = lambda *s: torch.full(s, 77, dtype=torch.int64, device="cuda")
    nbytes = int(hip.lib().mvd_image_metrics_scratch(B, C, H, W, n))
    return dict(sq_sum=f(max(B, 1)), count=i(max(B, 1)), ssim_sum=f(max(B, 1)), ssim_count=i(max(B, 1)),
                ssim_map=f(max(B, 1), C, max(H - n + 1, 1), max(W - n + 1, 1)),
                scratch=torch.full((max(nbytes // 8, 1),), 0x1234, dtype=torch.int64, device="cuda"), nbytes=nbytes)


def _image_untouched(out):
    return all(bool((out[k] == SENTINEL).all()) for k in ("sq_sum", "ssim_sum", "ssim_map")) and \
        all(bool((out[k] == 77).all()) for k in ("count", "ssim_count")) and bool((out["scratch"] == 0x1234).all())


def _image_call(hip, case, out, rows=None, skip=(), **over):
    """One mvd_image_metrics call on `case` (on the images `rows` of it) into the buffers `out`; returns the entry's return code."""
    sel = slice(None) if rows is None else list(rows)
    a, b = _dev(case.a[sel], torch.float32), _dev(case.b[sel], torch.float32)
    mask = None if case.mask is None else _dev(case.mask[sel], torch.uint8)
    B, C, H, W = a.shape
    n = case.window
    table = (ctypes.c_double * n)(*case.weights) if n else None
    args = dict(a=_p(hip, a), b=_p(hip, b), mask=_p(hip, mask), B=B, C=C, H=H, W=W, weights=table, window=n, c1=case.c1, c2=case.c2)
    args.update({k: None if k in skip else hip.ptr(out[k]) for k in IMAGE_OUTPUTS})
    args.update(scratch=hip.ptr(out["scratch"]), nbytes=out["nbytes"])
    args.update(over)
    rc = hip.lib().mvd_image_metrics(*args.values(), hip.stream())
    torch.cuda.synchronize()
    return rc


def _image_run(hip, case, rows=None, skip=()):
    out = _image_buffers(hip, case, rows)
    hip.check(_image_call(hip, case, out, rows, skip))
    return out


@pytest.mark.parametrize("name", V.IMAGE_CASES)
def test_image_entry_meets_the_rule(hip, name):
    case = V.image_case(name)
    B, C, H, W = case.shape
    out = _image_run(hip, case)
    if B == 0:
        assert _image_untouched(out)
        return
    again = _image_run(hip, case)
    assert _same(out, again, IMAGE_OUTPUTS), "two runs differ"
    got_map = None
    if case.window:
        want_map = V.ssim_map_a(case)
        got_map = out["ssim_map"].cpu().numpy()
        assert np.array_equal(np.isnan(got_map), np.isnan(want_map))
        differ = int((got_map.view(np.int64) != want_map.view(np.int64))[~np.isnan(want_map)].sum())
        assert differ == 0, f"{differ} map values are not (a)'s bits"
    else:
        assert bool((out["ssim_map"] == SENTINEL).all()) and bool((out["ssim_sum"] == SENTINEL).all()) and bool((out["ssim_count"] == 77).all())
    worst = [0.0, 0.0]
    for i, row in enumerate(V.image_a(case, got_map)):
        assert int(out["count"][i]) == row["count"]
        pairs = [(float(out["sq_sum"][i]), row["sq_sum"], row["sq_bound"])]
        if case.window:
            assert int(out["ssim_count"][i]) == row["ssim_count"]
            pairs.append((float(out["ssim_sum"][i]), row["ssim_sum"], row["ssim_bound"]))
        for k, (got, want, bound) in enumerate(pairs):
            if math.isnan(want):
                assert math.isnan(got), (i, k, got)
                continue
            assert abs(got - want) <= bound, (i, k, got, want, bound)
            worst[k] = max(worst[k], abs(got - want) / bound if bound else 0.0)
    print(f"IMAGE {name} {case.shape} window {case.window} | map bit-equal | |sq_sum - fsum| / bound {worst[0]:.3f} | ssim_sum {worst[1]:.3f}")
    if name == "identical":
        assert bool((out["ssim_map"] == 1.0).all()) and float(out["sq_sum"][0]) == 0.0


def test_an_image_alone_is_the_image_inside_a_batch(hip):
    case = V.image_case("w11_16x32_b5_masked")
    full = _image_run(hip, case)
    for i in range(case.shape[0]):
        one = _image_run(hip, case, rows=[i])
        assert all(torch.equal(_bits(one[k][0]), _bits(full[k][i])) for k in IMAGE_OUTPUTS), i
    swapped = _image_run(hip, case, rows=[4, 3, 2, 1, 0])
    assert all(torch.equal(_bits(swapped[k].flip(0)), _bits(full[k])) for k in IMAGE_OUTPUTS)


def test_image_outputs_may_be_null_in_any_subset(hip):
    case = V.image_case("w11_17x31_c3_masked")
    full = _image_run(hip, case)
    for r in range(1, len(IMAGE_OUTPUTS) + 1):
        for skip in itertools.combinations(IMAGE_OUTPUTS, r):
            out = _image_run(hip, case, skip=skip)
            keep = [k for k in IMAGE_OUTPUTS if k not in skip]
            assert _same(out, full, keep), skip
            for k in skip:
                assert bool((out[k] == (77 if out[k].dtype == torch.int64 else SENTINEL)).all()), (skip, k)


def test_image_entry_refuses_and_writes_nothing(hip):
    case = V.image_case("w11_15x33_c3")
    L = hip.lib()
    nan_w = (ctypes.c_double * 11)(*([0.1] * 5 + [float("inf")] + [0.1] * 5))
    bad = [dict(a=None), dict(b=None), dict(B=-1), dict(C=0), dict(B=300, C=300), dict(H=0), dict(W=32769), dict(window=10), dict(window=1),
           dict(window=35), dict(H=10), dict(W=10), dict(weights=nan_w), dict(c1=float("nan")), dict(c2=float("-inf")), dict(scratch=None),
           dict(nbytes=8)]
    for kw in bad:
        out = _image_buffers(hip, case)
        assert _image_call(hip, case, out, **kw) != 0, kw
        assert b"mvd_image_metrics:" in L.mvd_last_error(), (kw, L.mvd_last_error())
        assert _image_untouched(out), kw
    out = _image_buffers(hip, case)
    off = ctypes.c_void_p(out["scratch"].data_ptr() + 4)
    assert _image_call(hip, case, out, scratch=off) != 0 and b"mvd_image_metrics:" in L.mvd_last_error() and _image_untouched(out)


# ------------------------------------------------------------------------------------------------ the depth entry
def _depth_buffers(hip, B, H, W):
    nbytes = int(hip.lib().mvd_depth_metrics_scratch(B, H, W))
    return dict(fit=torch.full((max(B, 1), 2), SENTINEL, dtype=torch.float64, device="cuda"),
                sums=torch.full((max(B, 1), 4), SENTINEL, dtype=torch.float64, device="cuda"),
                counts=torch.full((max(B, 1), 5), 77, dtype=torch.int64, device="cuda"),
                scratch=torch.full((max(nbytes // 8, 1),), 0x1234, dtype=torch.int64, device="cuda"), nbytes=nbytes)


def _depth_untouched(out):
    return bool((out["fit"] == SENTINEL).all()) and bool((out["sums"] == SENTINEL).all()) and bool((out["counts"] == 77).all()) and \
        bool((out["scratch"] == 0x1234).all())


def _depth_call(hip, case, out, rows=None, skip=(), **over):
    sel = slice(None) if rows is None else list(rows)
    pred, target = _dev(case.pred[sel], torch.float32), _dev(case.target[sel], torch.float32)
    valid = None if case.valid is None else _dev(case.valid[sel], torch.uint8)
    fit_in = None if case.fit_in is None else _dev(case.fit_in[sel], torch.float64)
    B, H, W = pred.shape
    args = dict(pred=_p(hip, pred), target=_p(hip, target), valid=_p(hip, valid), B=B, H=H, W=W, align=case.align, fit_in=_p(hip, fit_in))
    args.update({k: None if k in skip else hip.ptr(out[k]) for k in DEPTH_OUTPUTS})
    args.update(scratch=hip.ptr(out["scratch"]), nbytes=out["nbytes"])
    for k, v in over.items():
        args[k] = hip.ptr(v) if torch.is_tensor(v) else v
    rc = hip.lib().mvd_depth_metrics(*args.values(), hip.stream())
    torch.cuda.synchronize()
    return rc


def _depth_run(hip, case, rows=None, skip=(), **over):
    B = case.pred.shape[0] if rows is None else len(rows)
    out = _depth_buffers(hip, B, *case.pred.shape[1:])
    hip.check(_depth_call(hip, case, out, rows, skip, **over))
    return out


@pytest.mark.parametrize("name", V.DEPTH_CASES)
def test_depth_entry_meets_the_rule(hip, name):
    case = V.depth_case(name)
    B = case.pred.shape[0]
    out = _depth_run(hip, case)
    if B == 0:
        assert _depth_untouched(out)
        return
    again = _depth_run(hip, case)
    assert _same(out, again, DEPTH_OUTPUTS), "two runs differ"
    fit = out["fit"].cpu().numpy()
    worst_fit = 0.0
    for i, (s, b, ds, db) in enumerate(V.fit_exact(case)):
        for got, want, bound in ((fit[i, 0], s, ds), (fit[i, 1], b, db)):
            assert (math.isnan(got) and math.isnan(want)) or abs(got - want) <= bound, (i, got, want, bound)
            worst_fit = max(worst_fit, abs(got - want) / bound if bound else 0.0) if not math.isnan(want) else worst_fit
    sums, counts = out["sums"].cpu().numpy(), out["counts"].cpu().numpy()
    worst = np.zeros(4)
    for i, row in enumerate(V.depth_a(case, fit)):
        assert counts[i].tolist() == row["counts"].tolist(), (i, counts[i], row["counts"])
        for k in range(4):
            assert abs(sums[i, k] - row["sums"][k]) <= row["bounds"][k], (i, k, sums[i, k], row["sums"][k], row["bounds"][k])
            if row["bounds"][k]:
                worst[k] = max(worst[k], abs(sums[i, k] - row["sums"][k]) / row["bounds"][k])
    print(f"DEPTH {name} {case.pred.shape} align {case.align} | |fit - exact| / bound {worst_fit:.3f} | counts equal | "
          f"|sum - fsum| / bound {' '.join(f'{v:.3f}' for v in worst)}")
    # the second way in: MVD_DEPTH_ALIGN_GIVEN with the fit this call returned is this call
    given = _depth_run(hip, case, align=V.ALIGN_GIVEN, fit_in=out["fit"].clone())
    assert _same(given, out, DEPTH_OUTPUTS)


def test_a_depth_map_alone_is_the_map_inside_a_batch(hip):
    case = V.depth_case("none_b5")
    full = _depth_run(hip, case)
    scaled = V.DepthCase(case.pred, case.target, case.valid, V.ALIGN_SCALE_SHIFT)
    full_fit = _depth_run(hip, scaled)
    for i in range(5):
        assert all(torch.equal(_bits(_depth_run(hip, case, rows=[i])[k][0]), _bits(full[k][i])) for k in DEPTH_OUTPUTS), i
        assert all(torch.equal(_bits(_depth_run(hip, scaled, rows=[i])[k][0]), _bits(full_fit[k][i])) for k in DEPTH_OUTPUTS), i


def test_depth_outputs_may_be_null_in_any_subset(hip):
    case = V.depth_case("scale_shift")
    full = _depth_run(hip, case)
    for r in range(1, 4):
        for skip in itertools.combinations(DEPTH_OUTPUTS, r):
            out = _depth_run(hip, case, skip=skip)
            assert _same(out, full, [k for k in DEPTH_OUTPUTS if k not in skip]), skip
            for k in skip:
                assert bool((out[k] == (77 if k == "counts" else SENTINEL)).all()), (skip, k)


def test_depth_entry_refuses_and_writes_nothing(hip):
    case = V.depth_case("scale_chunks")
    L = hip.lib()
    some_fit = torch.ones(2, 2, dtype=torch.float64, device="cuda")
    bad = [dict(pred=None), dict(target=None), dict(B=-1), dict(B=65536), dict(H=0), dict(W=32769), dict(align=-1), dict(align=4),
           dict(align=V.ALIGN_GIVEN), dict(fit_in=some_fit), dict(scratch=None), dict(nbytes=16)]
    for kw in bad:
        out = _depth_buffers(hip, *case.pred.shape)
        assert _depth_call(hip, case, out, **kw) != 0, kw
        assert b"mvd_depth_metrics:" in L.mvd_last_error(), (kw, L.mvd_last_error())
        assert _depth_untouched(out), kw


# ------------------------------------------------------------------------------------------------ the device log
def _log_inputs():
    """Every value a depth case takes a logarithm of (q at the exact fit, and t), once."""
    vals = []
    for name in V.DEPTH_CASES:
        case = V.depth_case(name)
        if case.pred.shape[0] == 0:
            continue
        ok = V.counted_pixels(case)
        for i, row in enumerate(V.depth_b(case)):
            vals.append(row["q"][row["kept"]])
            vals.append(case.target[i][ok[i]].astype(np.float64)[row["kept"]])
    return np.unique(np.concatenate(vals))


def test_device_log_error_is_the_measured_one():
    """MEASURED on an MI355X: 16 280 inputs in [0.045, 5.75], largest error 0.6178 ulp, 15 700 correctly rounded."""
    x = _log_inputs()
    got = torch.log(torch.from_numpy(x).cuda()).cpu().numpy()
    worst = V.log_ulps(x, got)
    exact = int((got == np.array([V.log_mp(v) for v in x.tolist()])).sum())
    print(f"LOG {len(x)} inputs in [{x.min():.4g}, {x.max():.4g}] | largest error {worst:.4f} ulp | correctly rounded {exact} of {len(x)}")
    assert len(x) > 5000
    assert worst <= V.LOG_ULPS_MEASURED      # the figure the bounds allow four times of


def test_the_kernel_log_is_the_measured_log(hip):
    """One-pixel images with t = 1 (log 1 = 0 exactly) and the fit (1, 0): the fourth sum is log(q) * log(q) of the kernel's own log."""
    x = _log_inputs()[::7].astype(np.float32)
    case = V.DepthCase(x.reshape(-1, 1, 1), np.ones((len(x), 1, 1), np.float32), None, V.ALIGN_NONE)
    out = _depth_run(hip, case)
    lg = torch.log(torch.from_numpy(x.astype(np.float64)).cuda())
    assert torch.equal(_bits(out["sums"][:, 3]), _bits(lg * lg))
    assert bool((out["counts"][:, 3] == 1).all())


# ------------------------------------------------------------------------------------------------ the host path
def test_compare_images_is_the_abi(hip):
    from mvdfusion_amd import view_metrics as vm
    case = V.image_case("w11_16x32_b5_masked")
    abi = _image_run(hip, case)
    B, C, H, W = case.shape
    a, b, m = _dev(case.a, torch.float32), _dev(case.b, torch.float32), _dev(case.mask, torch.uint8)
    got = vm.compare_images(a, b, mask=m, return_map=True)
    mse = abi["sq_sum"] / (abi["count"] * C)
    assert torch.equal(_bits(got.mse), _bits(mse)) and torch.equal(got.count, abi["count"])
    assert torch.equal(_bits(got.psnr), _bits(10.0 * torch.log10(1.0 / mse)))
    assert torch.equal(_bits(got.ssim), _bits(abi["ssim_sum"] / (abi["ssim_count"] * C)))
    assert torch.equal(_bits(got.ssim_map), _bits(abi["ssim_map"]))
    assert got.mse.dtype == torch.float64 and got.mse.is_cuda and got.mse.shape == (5,)
    assert bool(((got.ssim > 0.5) & (got.ssim < 1.0)).all()) and bool(((got.psnr > 15) & (got.psnr < 30)).all())
    # leading dimensions, any mask dtype, data_range, no window
    a2, b2 = a[:4].reshape(2, 2, C, H, W), b[:4].reshape(2, 2, C, H, W)
    lead = vm.compare_images(a2 * 255.0, b2 * 255.0, mask=m[:4].reshape(2, 2, H, W).bool(), data_range=255.0, window=None)
    assert lead.mse.shape == lead.psnr.shape == lead.count.shape == (2, 2) and lead.ssim is None and lead.ssim_map is None
    assert torch.allclose(lead.psnr.reshape(4), got.psnr[:4], rtol=0, atol=1e-5)
    one = vm.compare_images(a[0], b[0], mask=m[0])
    assert one.mse.shape == () and torch.equal(_bits(one.mse), _bits(got.mse[0])) and torch.equal(_bits(one.ssim), _bits(got.ssim[0]))
    # the analytic ends: identical images, an empty mask, zero images
    same = vm.compare_images(a, a.clone(), return_map=True)
    assert bool((same.mse == 0).all()) and bool(torch.isinf(same.psnr).all()) and bool((same.psnr > 0).all()) and bool((same.ssim == 1.0).all())
    assert bool((same.ssim_map == 1.0).all())
    none = vm.compare_images(a, b, mask=torch.zeros_like(m))
    assert bool(torch.isnan(none.mse).all()) and bool(torch.isnan(none.ssim).all()) and bool((none.count == 0).all())
    empty = vm.compare_images(a[:0], b[:0])
    assert empty.mse.shape == (0,) and empty.ssim.shape == (0,)
    uniform = vm.compare_images(a, b, window=7, sigma=None)
    assert bool(((uniform.ssim > 0) & (uniform.ssim < 1)).all())


def test_compare_depth_is_the_abi(hip):
    from mvdfusion_amd import view_metrics as vm
    case = V.depth_case("scale_chunks")
    abi = _depth_run(hip, case)
    p, t, v = _dev(case.pred, torch.float32), _dev(case.target, torch.float32), _dev(case.valid, torch.uint8)
    got = vm.compare_depth(p, t, valid=v, align="scale")
    n = abi["counts"][:, 3]
    for name, want in (("abs_rel", abi["sums"][:, 0] / n), ("sq_rel", abi["sums"][:, 1] / n), ("rmse", torch.sqrt(abi["sums"][:, 2] / n)),
                       ("rmse_log", torch.sqrt(abi["sums"][:, 3] / n)), ("delta1", abi["counts"][:, 0] / n), ("delta2", abi["counts"][:, 1] / n),
                       ("delta3", abi["counts"][:, 2] / n), ("scale", abi["fit"][:, 0]), ("shift", abi["fit"][:, 1])):
        assert torch.equal(_bits(getattr(got, name)), _bits(want)), name
    assert torch.equal(got.count, n) and torch.equal(got.dropped, abi["counts"][:, 4]) and got.abs_rel.dtype == torch.float64
    assert bool((got.delta1 <= got.delta2).all()) and bool((got.delta2 <= got.delta3).all()) and bool((got.delta3 <= 1).all())
    given = vm.compare_depth(p, t, valid=v.bool(), align=abi["fit"])
    assert torch.equal(_bits(given.abs_rel), _bits(got.abs_rel)) and torch.equal(_bits(given.rmse_log), _bits(got.rmse_log))
    lead = vm.compare_depth(p.reshape(2, 1, 40, 53), t.reshape(2, 1, 40, 53), valid=v.reshape(2, 1, 40, 53), align="scale")
    assert lead.rmse.shape == (2, 1) and torch.equal(_bits(lead.rmse.reshape(2)), _bits(got.rmse))
    same = vm.compare_depth(t, t)
    assert bool((same.abs_rel == 0).all()) and bool((same.rmse_log == 0).all()) and bool((same.delta1 == 1).all())
    nothing = vm.compare_depth(t, t, valid=torch.zeros_like(v), align="scale_shift")
    assert bool(torch.isnan(nothing.abs_rel).all()) and bool(torch.isnan(nothing.scale).all()) and bool((nothing.count == 0).all())
    holes = torch.where(v.bool(), t, torch.full_like(t, float("inf")))      # the renderers' empty depth drops out by itself
    assert torch.equal(_bits(vm.compare_depth(p, holes, align="scale").abs_rel), _bits(got.abs_rel))


def test_compare_views_takes_records_and_mask_modes(hip):
    from mvdfusion_amd import fusion
    from mvdfusion_amd import view_metrics as vm
    g = torch.Generator().manual_seed(3)
    M, P = 2, 24
    rgb_a, rgb_b = torch.rand(M, 3, P, P, generator=g).cuda(), torch.rand(M, 3, P, P, generator=g).cuda()
    depth_a, depth_b = (torch.rand(M, P, P, generator=g) + 0.5).cuda(), (torch.rand(M, P, P, generator=g) + 0.5).cuda()
    hit_a, hit_b = (torch.rand(M, P, P, generator=g) < 0.7).cuda(), (torch.rand(M, P, P, generator=g) < 0.7).cuda()
    inf = torch.full_like(depth_a, float("inf"))
    pred = fusion.RenderedViews(rgb=rgb_a, depth=torch.where(hit_a, depth_a, inf), index=hit_a.int() - 1, hit=hit_a)
    target = dict(rgb=rgb_b, depth=torch.where(hit_b, depth_b, inf), hit=hit_b)
    for mode, m in (("both", hit_a & hit_b), ("either", hit_a | hit_b), ("target", hit_b), (None, None), (hit_a, hit_a)):
        images, depth = vm.compare_views(pred, target, mask=mode, align="scale", window=7)
        want = vm.compare_images(rgb_a, rgb_b, mask=m, window=7)
        assert torch.equal(_bits(images.mse), _bits(want.mse)) and torch.equal(_bits(images.ssim), _bits(want.ssim)), mode
        valid = hit_a & hit_b if m is None else hit_a & hit_b & m
        want_d = vm.compare_depth(depth_a, depth_b, valid=valid, align="scale")
        assert torch.equal(_bits(depth.abs_rel), _bits(want_d.abs_rel)) and torch.equal(depth.count, want_d.count), mode
    images, depth = vm.compare_views(dict(rgb=None, depth=pred.depth, hit=hit_a), target)
    assert images is None and depth.count.shape == (M,)


def test_viewfusion_compare_binds_the_depth_map():
    """On the reduced-width cached model, decode=False: the images as given, the depth channels through the model's own scale and shift."""
    from conftest import build_model
    from mvdfusion_amd import view_metrics as vm
    V_, S = 3, 32
    m = build_model(32)
    g = torch.Generator().manual_seed(11)
    x, y = (0.5 * torch.randn(V_, 5, S, S, generator=g)).cuda(), (0.5 * torch.randn(V_, 5, S, S, generator=g)).cuda()
    img_x, img_y = torch.rand(V_, 3, 8 * S, 8 * S, generator=g).cuda(), torch.rand(V_, 3, 8 * S, 8 * S, generator=g).cuda()
    scale, shift = float(m.view_attn.depth_scale), float(m.view_attn.depth_shift)
    images, depth = m.compare(x, y, decode=False, rgb=img_x, target_rgb=img_y, align="scale")
    want = vm.compare_images(img_x, img_y)
    assert torch.equal(_bits(images.psnr), _bits(want.psnr)) and torch.equal(_bits(images.ssim), _bits(want.ssim)) and images.psnr.shape == (V_,)
    d01 = lambda lat: torch.clamp((lat[:, 4] + 1.0) / 2.0, 0.0, 1.0)
    fg = (d01(y) > 0.02) & (d01(y) < 0.98)
    want_d = vm.compare_depth(d01(x) * scale + shift, d01(y) * scale + shift, valid=fg, align="scale")
    assert torch.equal(_bits(depth.abs_rel), _bits(want_d.abs_rel)) and torch.equal(depth.count, want_d.count)
    assert bool((depth.count == fg.sum(dim=(1, 2))).all()) and bool((depth.count > 0).all())
    images, depth = m.compare(x, x.clone(), decode=False)
    assert images is None and bool((depth.abs_rel == 0).all()) and bool((depth.delta1 == 1).all())
    both = m.compare(torch.stack([x, y]), torch.stack([y, x]), decode=False, rgb=torch.stack([img_x, img_y]), target_rgb=torch.stack([img_y, img_x]))
    assert both[0].ssim.shape == both[1].rmse.shape == (2, V_)
    from test_gpu_fusion import _small_vae
    assert not hasattr(m, "vae")
    m.vae = _small_vae()                      # (the cached test model is built without one)
    try:
        images, again = m.compare(x, y)       # decode=True: the images are the decoder's, 8 S pixels per side
        want = vm.compare_images(m._decoded(x), m._decoded(y))
        assert torch.equal(_bits(images.psnr), _bits(want.psnr)) and torch.equal(_bits(images.ssim), _bits(want.ssim))
        assert torch.equal(_bits(again.abs_rel), _bits(m.compare(x, y, decode=False)[1].abs_rel))
    finally:
        del m.vae
    with pytest.raises(ValueError, match="go together"):
        m.compare(x, y, decode=False, rgb=img_x)
    with pytest.raises(ValueError, match="one shape"):
        m.compare(x, y[:2], decode=False)


# ------------------------------------------------------------------------------------------------ end to end
def test_a_rendered_sphere_against_itself_and_shifted_by_a_pixel():
    """A marched sphere (G = 24, radius 0.45) rendered into three cameras at 48 x 48: against itself every figure is the perfect one;
    against itself rolled by one pixel along x SSIM < 1, PSNR finite and the depth error > 0 on the pixels both hit."""
    from mvdfusion_amd import fusion
    from mvdfusion_amd import synthetic as syn
    from mvdfusion_amd import view_metrics as vm
    from mvdfusion_amd.cameras import get_camera_slice
    G, R, P = 24, 0.45, 48
    sdf = ((fusion.voxel_centres(G).double().norm(dim=1) - R).reshape(G, G, G)).float().cuda()
    mesh = fusion.extract_mesh(sdf)
    cams = get_camera_slice(syn.gso_rig(), [0, 5, 10])      # three of the rig's views: distance 1.5, looking at the origin
    views = fusion.render_mesh(mesh, cams, size=P)
    record = dict(rgb=views.shaded(), depth=views.depth, hit=views.hit)
    share = float(views.hit.float().mean())
    assert 0.02 < share < 0.9, share
    images, depth = vm.compare_views(record, record)
    assert bool((images.mse == 0).all()) and bool((images.psnr == float("inf")).all()) and bool((images.ssim == 1.0).all())
    assert bool((depth.abs_rel == 0).all()) and bool((depth.rmse == 0).all()) and bool((depth.delta1 == 1).all())
    assert bool((depth.count == views.hit.sum(dim=(1, 2))).all()) and bool((depth.dropped == 0).all())
    moved = {k: torch.roll(v, 1, dims=-1) for k, v in record.items()}
    images, depth = vm.compare_views(moved, record, mask=None)
    print(f"E2E sphere {len(mesh)} faces, hit share {share:.3f} | one-pixel shift: psnr {images.psnr.tolist()} ssim {images.ssim.tolist()} "
          f"abs_rel {depth.abs_rel.tolist()} delta1 {depth.delta1.tolist()}")
    assert bool(torch.isfinite(images.psnr).all()) and bool((images.psnr > 5).all())
    assert bool((images.ssim < 1.0).all()) and bool((images.ssim > 0.0).all())
    assert bool((depth.abs_rel > 0).all()) and bool((depth.abs_rel < 0.5).all()) and bool((depth.count < views.hit.sum(dim=(1, 2))).all())
