"""tests/gemm_f64.py has teeth, shown on the CPU: the gather oracle of the convolutions equals float64 F.conv2d, the exact fixtures give what
their docstring says, every mutant of gemm_f64.MUTANTS is rejected by a (case, fixture) of the very lists tests/test_gpu_gemm_f64.py runs,
an fp32 emulation of the split-operand algorithm stays at or below HALF of every bar in both flavours and all three precisions, the
packed-image decoders invert a packer written from the header text, and no case is larger than the limits the suite sets itself."""

import pytest
import torch
import torch.nn.functional as F

import gemm_f64 as G


def _ids(cases):
    return [G.case_id(c) for c in cases]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ sizes
def test_case_sizes():
    L = G.LIMITS
    for M, N, K in G.DENSE_CASES + G.GEGLU_CASES + G.LINEAR_BACKWARD_CASES:
        assert M <= L["rows"] and N <= L["cols"] and K <= L["K"], (M, N, K)
    for c in G.CONV_CASES:
        assert G.conv_M(c) <= L["rows"] and c.Cout <= L["cols"] and c.Cin <= L["K"] and c.tail <= L["K"], c
        assert c.B * c.Hin * c.Win <= L["rows"], c
    for B, H, W, Cin, Cout in G.CONV_BACKWARD_CASES:
        assert B * H * W <= L["rows"] and Cin <= L["cols"] and Cout <= L["cols"]
    for N, K in G.PACK_LINEAR_CASES + G.PACK_CONV_CASES:
        assert N <= L["cols"] and K <= 320
    assert set(G.MUTANTS) == set(_REJECTORS), "every mutant has a rejection scan below"


# ------------------------------------------------------------------------------------------------ the gather oracle against F.conv2d
def _conv2d_f64(fx, c):
    x = fx["x"].double().permute(0, 3, 1, 2)
    w, b = fx["w"].double(), fx["bias"].double()
    if c.upsample:
        y = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, stride=1, padding=1)
    elif c.no_pad_tl:
        y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=c.stride, padding=0)
    else:
        y = F.conv2d(x, w, b, stride=c.stride, padding=1)
    y = y[:, :, :c.Hout, :c.Wout]
    assert tuple(y.shape[2:]) == (c.Hout, c.Wout), (tuple(y.shape), c)
    y = y.permute(0, 2, 3, 1).reshape(G.conv_M(c), c.Cout)
    if c.tail:
        y = y + fx["x2"].double() @ fx["wt"].double().t()
    return y


@pytest.mark.parametrize("c", G.CONV_CASES, ids=_ids(G.CONV_CASES))
def test_gather_oracle_equals_conv2d(c):
    for name in ("plain", "cancel"):
        fx = G.conv_fixture(name, c)
        ref, S = G.conv_ref(fx, c, rounded=False)          # (four-tap form: the composed weights before their one fp32 rounding)
        want = _conv2d_f64(fx, c)
        assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max()), (name, _rel(ref, want))
        assert bool((S + 1e-300 >= ref.abs() * (1 - 1e-12)).all())
    if c.kind == "up4":          # the four-tap statement against the nine-tap one (the composed weights are rounded to fp32 once: 2^-24)
        nine = c._replace(kind="up9")
        fx = G.conv_fixture("plain", c)
        r4, S4 = G.conv_ref(fx, c)
        r9, _ = G.conv_ref(fx, nine)
        assert bool(((r4 - r9).abs() <= 2.0 ** -24 * S4 + 1e-300).all())


# ------------------------------------------------------------------------------------------------ the exact fixtures
@pytest.mark.parametrize("case", G.DENSE_CASES, ids=_ids(G.DENSE_CASES))
def test_dense_geometry_fixture(case):
    M, N, K = case
    fx = G.dense_fixture("geometry", M, N, K)
    assert float(fx["A"].abs().max()) <= 255 and bool((fx["A"] == fx["A"].round()).all())
    assert bool((fx["W"].sum(1) == 1).all()) and bool(((fx["W"] == 0) | (fx["W"] == 1)).all())
    want = fx["A"][:, fx["pi"]].double()
    for layout in G.LAYOUTS:
        ref, _ = G.dense_ref(fx["A"], fx["W"], layout=G.dense_layout(fx, layout, M, N, K))
        assert torch.equal(ref, want)
    for fmt in G.FMTS:          # exact in every precision, both flavours and under every split
        for prec in G.PRECS:
            for sp in G.split_counts(K // 32):
                assert torch.equal(G.emulate(fx["A"], fx["W"], fmt, prec, splits=sp).double(), want), (fmt, prec, sp)


@pytest.mark.parametrize("c", G.CONV_CASES, ids=_ids(G.CONV_CASES))
def test_conv_geometry_fixture(c):
    fx = G.conv_fixture("geometry", c)
    want = G.conv_geometry_expected(c)
    ref, _ = G.conv_ref(fx, c, bias=False)
    assert torch.equal(ref, want)
    assert float(want.abs().max()) <= 255
    if c.B > 1 and c.Cout >= 27:          # the image index is seen, and only the own image's
        m = torch.arange(G.conv_M(c)) // (c.Hout * c.Wout)
        col = want[:, 2::3][:, :9]
        assert bool(((col == 0) | (col == (m + 1)[:, None].double())).all()) and bool((col[:, 4] > 0).any())
    for fmt in G.FMTS:
        for prec in G.PRECS:
            got = _emulate_conv(fx, c, fmt, prec, 3, bias=False, res=False)
            assert torch.equal(got.double(), want), (fmt, prec)


# ------------------------------------------------------------------------------------------------ mutants
def _over(t_true, t_mut, fixture, fmt, prec, nk, splits=1, act=0, composed=False):
    """Is the mutated reference rejected?  exact fixture: any difference; else more than two bars away somewhere."""
    d = (t_mut["ref"] - t_true["ref"]).abs()
    if fixture == "geometry":
        return bool((d > 0).any())
    return bool((d > 2.0 * G.bar(t_true, fmt, prec, nk, splits, act, composed)).any())


def _scan_dense(mutant, fmt="f16", prec=4, splits_of=lambda nk: [1]):
    hits = []
    for case in G.DENSE_CASES:
        M, N, K = case
        for fixture in G.DENSE_FIXTURES:
            fx = G.dense_fixture(fixture, M, N, K)
            for layout in G.LAYOUTS:
                lay = G.dense_layout(fx, layout, M, N, K)
                for epi, rpb in G.dense_epilogue_runs(M, fixture):
                    for sp in splits_of(K // 32):
                        kw = dict(G.epilogue_args(fx, G.EPILOGUES[epi], rpb), layout=lay, fmt=fmt, splits=sp)
                        t, tm = G.dense_terms(fx["A"], fx["W"], **kw), G.dense_terms(fx["A"], fx["W"], mutant=mutant, **kw)
                        if _over(t, tm, fixture, fmt, prec, K // 32, sp, kw["act"]):
                            hits.append((case, fixture, layout, epi, rpb, sp))
                            return hits
    return hits


def _scan_conv(mutant, kinds, fmt="f16", prec=4):
    hits = []
    for c in G.CONV_CASES:
        if c.kind not in kinds:
            continue
        for fixture in G.CONV_FIXTURES:
            fx = G.conv_fixture(fixture, c)
            for bias, res, layout in G.conv_runs(c, fixture):
                kw = dict(bias=bias, res=res, fmt=fmt, layout=G.conv_res_layout(fx, c, layout) if res else None)
                t, tm = G.conv_terms(fx, c, **kw), G.conv_terms(fx, c, mutant=mutant, **kw)
                if _over(t, tm, fixture, fmt, prec, G.conv_K(c) // 32, composed=c.kind == "up4"):
                    hits.append((G.case_id(c), fixture))
                    break
    return hits


def _scan_geglu(mutant):
    for M, N, K in G.GEGLU_CASES:
        fx = G.dense_fixture("plain", M, N, K)
        t = G.dense_terms(fx["A"], fx["W"], bias=fx["bias"], geglu=True)
        tm = G.dense_terms(fx["A"], fx["W"], bias=fx["bias"], geglu=True, mutant=mutant)
        if _over(t, tm, "plain", "f16", 4, K // 32, act=G.ACT_GELU):
            return [(M, N, K)]
    return []


def _scan_planes(mutant):
    for M, N, K in G.PLANES_CASES:
        fx = G.dense_fixture("plain", M, N, K)
        kw = dict(bias=fx["bias"], acc_scale=G.ACC_SCALE_PLANES, scale=1.0)
        t, tm = G.dense_terms(fx["A"], fx["W"], **kw), G.dense_terms(fx["A"], fx["W"], mutant=mutant, **kw)
        if _over(t, tm, "plain", "f16", 4, K // 32):
            return [(M, N, K)]
    return []


def _scan_packed(mutant):
    for N, K in G.PACK_LINEAR_CASES:
        w = torch.randn(N, K, generator=G._gen("pack", N, K))
        words = G.pack_numpy(w, "f16", G.pack_scale(w))
        hi, lo = G.decode_packed(words, N, K, "f16", mutant=mutant)
        if not torch.equal((hi + lo)[:N, :K], sum(G.split_op(w * G.pack_scale(w), "f16"))):
            return [(N, K)]
    return []


_S1 = ("s1", "tail")
_REJECTORS = {
    "swap_h_w": lambda m: _scan_conv(m, ("s1", "s2", "s2nopad", "up9", "tail")),
    "no_pad_tl_ignored": lambda m: _scan_conv(m, ("s2nopad",)),
    "stride_tap_origin_0": lambda m: _scan_conv(m, ("s2",)),
    "upsample_halves_before_bounds": lambda m: _scan_conv(m, ("up9",)),
    "image_boundary_leaks": lambda m: _scan_conv(m, ("s1", "s2", "s2nopad", "tail")),
    "patch_row_pitch_w": lambda m: _scan_conv(m, ("s1",)),
    "up4_parity_swapped": lambda m: _scan_conv(m, ("up4",)),
    "drop_last_ktile": lambda m: _scan_dense(m) + _scan_conv(m, ("s1", "tail", "up4")),
    "tail_reads_tap_0": lambda m: _scan_conv(m, ("tail",)),
    "a_hi_only": lambda m: _scan_dense(m, fmt="bf16") and _scan_dense(m),
    "w_hi_only": lambda m: _scan_dense(m, fmt="bf16") and _scan_dense(m),
    "acc_scale_ignored": _scan_planes,
    "window_off_by_32_columns": _scan_dense,
    "res_pitch_is_ldo": lambda m: _scan_dense(m) + _scan_conv(m, _S1),
    "bias_b_row_from_tile_base": _scan_dense,
    "colscale_inside_act": _scan_dense,
    "geglu_halves_swapped": _scan_geglu,
    "short_last_split_reads_stale_slab": lambda m: _scan_dense(m, splits_of=G.split_counts),
    "packed_lane_order_n_major": _scan_packed,
}


@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_mutant_is_rejected(mutant):
    hits = _REJECTORS[mutant](mutant)
    print(f"MUTANT {mutant}: rejected by {hits[:3]}")
    assert hits, f"no (case, fixture) of the suite's lists rejects {mutant}"


def test_geometry_mutants_are_rejected_by_the_exact_fixture_alone():
    """The exact fixture pins the geometry without any tolerance: each geometry mutant changes it on some case."""
    for mutant, kinds in (("swap_h_w", ("s1", "s2", "up9")), ("no_pad_tl_ignored", ("s2nopad",)), ("stride_tap_origin_0", ("s2",)),
                          ("upsample_halves_before_bounds", ("up9",)), ("image_boundary_leaks", ("s1", "s2")), ("patch_row_pitch_w", ("s1",)),
                          ("up4_parity_swapped", ("up4",)), ("tail_reads_tap_0", ("tail",))):
        found = False
        for c in G.CONV_CASES:
            if c.kind in kinds:
                fx = G.conv_fixture("geometry", c)
                found = found or not torch.equal(G.conv_ref(fx, c, bias=False)[0], G.conv_ref(fx, c, bias=False, mutant=mutant)[0])
        assert found, mutant


def test_both_orientations_are_needed():
    """A square case cannot see swap_h_w; each of a transposed pair does."""
    sq = G._cc("s1", 2, 4, 4, 32, 48)
    fx = G.conv_fixture("geometry", sq)
    assert torch.equal(G.conv_ref(fx, sq, bias=False)[0], G.conv_ref(fx, sq, bias=False, mutant="swap_h_w")[0])
    for c in G.CONV_CASES[1:3]:
        fx = G.conv_fixture("geometry", c)
        assert not torch.equal(G.conv_ref(fx, c, bias=False)[0], G.conv_ref(fx, c, bias=False, mutant="swap_h_w")[0])


# ------------------------------------------------------------------------------------------------ the emulation against the bars
def _emulate_conv(fx, c, fmt, prec, splits, bias=True, res=True):
    b = fx["bias"] if bias else None
    if c.kind == "up4":
        parts, row = G.conv_operands(fx, c)
        out = torch.zeros(G.conv_M(c), c.Cout)
        sc = G.conv_scale(fx, c)
        for p in range(4):
            out[row[p]] = G.emulate(parts[p][0], parts[p][1], fmt, prec, scale=sc, splits=splits, bias=b)
        return out
    cols, wmat = G.conv_operands(fx, c)
    return G.emulate(cols, wmat, fmt, prec, scale=G.conv_scale(fx, c), splits=splits, bias=b, res=fx["res"] if res else None)


@pytest.mark.parametrize("fmt", G.FMTS)
@pytest.mark.parametrize("case", G.DENSE_CASES, ids=_ids(G.DENSE_CASES))
def test_emulation_stays_below_half_the_bar_dense(case, fmt):
    M, N, K = case
    nk = K // 32
    worst = {}
    for fixture in G.DENSE_FIXTURES:
        fx = G.dense_fixture(fixture, M, N, K)
        for epi, rpb in G.dense_epilogue_runs(M, fixture):
            e = G.EPILOGUES[epi]
            kw = G.epilogue_args(fx, e, rpb)
            t = G.dense_terms(fx["A"], fx["W"], **kw)
            for prec in G.PRECS:
                for sp in (1, 3):
                    got = G.emulate(fx["A"], fx["W"], fmt, prec, splits=sp, bias=kw.get("bias"), act=kw["act"], colscale=kw.get("colscale"),
                                    res=kw.get("res"), bias_b_rows=fx["bias_b"][torch.arange(M) // rpb] if e.get("bias_b") else None)
                    r = G.worst(got, t["ref"], G.bar(t, fmt, prec, nk, min(sp, nk), kw["act"]))
                    worst[(fixture, prec)] = max(worst.get((fixture, prec), 0.0), r)
    print("EMULATION dense", case, fmt, {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 0.5, worst


@pytest.mark.parametrize("fmt", G.FMTS)
def test_emulation_stays_below_half_the_bar_geglu_and_planes(fmt):
    worst = 0.0
    for M, N, K in G.GEGLU_CASES:
        fx = G.dense_fixture("plain", M, N, K)
        t = G.dense_terms(fx["A"], fx["W"], bias=fx["bias"], geglu=True)
        for prec in G.PRECS:
            worst = max(worst, G.worst(G.emulate_geglu(fx["A"], fx["W"], fmt, prec, fx["bias"]), t["ref"], G.bar(t, fmt, prec, K // 32, 1, G.ACT_GELU)))
    for M, N, K in G.PLANES_CASES:
        fx = G.dense_fixture("plain", M, N, K)
        t = G.dense_terms(fx["A"], fx["W"], bias=fx["bias"], acc_scale=G.ACC_SCALE_PLANES, scale=1.0)
        for prec in G.PRECS:
            got = G.emulate(fx["A"], fx["W"], fmt, prec, acc_scale=G.ACC_SCALE_PLANES, bias=fx["bias"], split_w=False, splits=2)
            worst = max(worst, G.worst(got, t["ref"], G.bar(t, fmt, prec, K // 32, 2)))
    print("EMULATION geglu / planes", fmt, round(worst, 3))
    assert worst <= 0.5


@pytest.mark.parametrize("fmt", G.FMTS)
@pytest.mark.parametrize("c", G.CONV_CASES, ids=_ids(G.CONV_CASES))
def test_emulation_stays_below_half_the_bar_conv(c, fmt):
    nk = G.conv_K(c) // 32
    worst = {}
    for fixture in G.CONV_FIXTURES:
        fx = G.conv_fixture(fixture, c)
        res = fixture != "geometry" and c.kind != "up4"
        t = G.conv_terms(fx, c, bias=fixture != "geometry", res=res)
        for prec in G.PRECS:
            got = _emulate_conv(fx, c, fmt, prec, 3, bias=fixture != "geometry", res=res)
            worst[(fixture, prec)] = G.worst(got, t["ref"], G.bar(t, fmt, prec, nk, min(3, nk), composed=c.kind == "up4"))
    print("EMULATION conv", G.case_id(c), fmt, {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 0.5, worst


def test_bars_are_far_below_the_per_tensor_tolerance_where_it_matters():
    """graded: the per-element bar of the smallest rows is orders of magnitude under what max|err| / max|ref| of the tensor allows."""
    M, N, K = 129, 96, 288
    fx = G.dense_fixture("graded", M, N, K)
    t = G.dense_terms(fx["A"], fx["W"])
    b = G.bar(t, "f16", 4, K // 32)
    per_tensor = 2e-6 * float(t["ref"].abs().max())
    print("BARS", float((b < per_tensor).double().mean()), float((b < per_tensor / 100).double().mean()), float(b.min()) / per_tensor)
    assert float((b < per_tensor).double().mean()) > 0.5                # most elements: the new bar is the tighter one
    assert float((b < per_tensor / 100).double().mean()) > 0.2          # a fifth of them: a hundred times tighter
    assert float(b.min()) < per_tensor * 1e-4


# ------------------------------------------------------------------------------------------------ packed images
@pytest.mark.parametrize("fmt", G.FMTS)
@pytest.mark.parametrize("N,K", G.PACK_LINEAR_CASES)
def test_decoder_inverts_the_numpy_packer(N, K, fmt):
    w = torch.randn(N, K, generator=G._gen("pack", N, K)) * 3.0
    scale = G.pack_scale(w)
    assert 1024 <= float(w.abs().max()) * scale < 2048
    words = G.pack_numpy(w, fmt, scale)
    hi, lo = G.decode_packed(words, N, K, fmt)
    h, l = G.split_op(w * scale, fmt)
    assert torch.equal(hi[:N, :K], h) and torch.equal(lo[:N, :K], l)
    pad = torch.ones_like(hi, dtype=torch.bool)
    pad[:N, :K] = False
    assert bool((hi[pad] == 0).all()) and bool((lo[pad] == 0).all())
    assert bool((((hi + lo)[:N, :K].double() - w.double() * scale).abs() <= G.pack_bar(w, scale, fmt)).all())
    # every word of the image is addressed exactly once by (n, k, plane)
    Np, Kp = (N + 15) // 16 * 16, (K + 31) // 32 * 32
    idx = G._index_grid(Np, Kp)
    both = torch.cat([idx.reshape(-1), idx.reshape(-1) + 512])
    assert both.unique().numel() == 2 * Np * Kp == int(both.max()) + 1


@pytest.mark.parametrize("Cout,Cin", G.PACK_CONV_CASES)
def test_conv_weight_matrix_matches_the_operand_order(Cout, Cin):
    """conv_weight_matrix (the header's K index) is the wmat of conv_operands (the gather's K order) when Cin is whole 32-channel blocks."""
    cin_pad = (Cin + 31) // 32 * 32
    w = torch.randn(Cout, Cin, 3, 3, generator=G._gen("packc", Cout, Cin))
    m = G.conv_weight_matrix(w, cin_pad)
    wp = torch.zeros(Cout, cin_pad, 3, 3)
    wp[:, :Cin] = w
    assert torch.equal(m, G.k_order(wp.reshape(Cout, cin_pad, 9).permute(0, 2, 1).contiguous()))
    assert m.shape[1] == 9 * cin_pad and int((m != 0).sum()) == int((w != 0).sum())


# ------------------------------------------------------------------------------------------------ backward oracles against autograd
def test_backward_oracles_equal_autograd():
    for M, N, K in G.LINEAR_BACKWARD_CASES:
        g = G._gen("lb", M, N, K)
        x, w, dy = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((M, K), (N, K), (M, N)))
        x.requires_grad_(), w.requires_grad_()
        (F.linear(x, w) * dy).sum().backward()
        r = G.linear_backward_ref(x, w, dy)
        assert _rel(r["dx"][0], x.grad) < 1e-12 and _rel(r["dW"][0], w.grad) < 1e-12 and _rel(r["db"][0], dy.sum(0)) < 1e-12
    for B, H, W, Cin, Cout in G.CONV_BACKWARD_CASES:
        g = G._gen("cb", B, H, W, Cin, Cout)
        x = torch.randn(B, H, W, Cin, generator=g, dtype=torch.float64, requires_grad=True)
        w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
        dy = torch.randn(B * H * W, Cout, generator=g, dtype=torch.float64)
        y = F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1).reshape(-1, Cout)
        (y * dy).sum().backward()
        r = G.conv3x3_backward_ref(x, w, dy, B, H, W)
        assert _rel(r["dx"][0], x.grad.reshape(-1, Cin)) < 1e-12 and _rel(r["dW"][0], w.grad) < 1e-12
        assert bool((r["dx"][1] >= r["dx"][0].abs() * (1 - 1e-12)).all())
