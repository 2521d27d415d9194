"""FLOAT64 statements of the normalisation / reduction family (csrc/norm.hip) and of the small backward kernels of the training step
(csrc/backward.hip outside attention), the fixtures the GPU tests feed to them, the bars they apply and the case lists they run
(tests/test_gpu_norm_f64.py; tests/test_cpu_norm_f64.py proves on the CPU that references, fixtures and bars have teeth).  CPU only:
plain float64 tensor arithmetic written from the formulas -- no F.group_norm, no autograd in here.

Every reference takes `mutant=`: one realistic way of being wrong (MUTANTS below).  The CPU file shows that each mutant is rejected by
at least one case of the very lists the GPU file parametrises over, i.e. that a kernel with that bug could not pass.

Conditioning.  kappa = (mean^2 + var) / (var + eps) per (image, group) or per row: how much larger E[x^2] is than the variance it is
subtracted down to.  gn_kappa / ln_kappa compute it in float64 from the fp32 values of a fixture; the CPU file checks what each claims.

GroupNorm fixtures (x (B, HW, C) fp32; gamma = +-(1 + 0.3 N(0, 1)), beta = +-(0.3 + 0.3 |N(0, 1)|): every group then has outputs of both
signs, so that max|ref| of a group behind the SiLU is not the ~0.28 of an all-negative group, and a group of zero variance -- whose
output is beta alone while the kernel's rounding is relative to gamma -- does not meet a beta of ~0):
  plain       : 2 N(0, 1) + 0.5 as tests/test_gpu_ops.py                                                   kappa ~ 1.06
  offset8/64  : N(0, 1) + (+-8 | +-64), the sign alternating by group                                      kappa ~ 65 | 4097
  chan_offset : N(0, 1) + a constant per channel drawn from N(0, 4^2): the group variance is mostly channel means
                (groups of n < 512 elements: the offsets 8 | 64 | 4 shrink by (n / 512)^2, gn_offset -- the rounding errors of so few
                terms do not average, and the float32 emulation of the algorithm itself then passes half of the bar's kappa term.
                The ONE-PASS forward only: the GroupNorm backward runs the same fixtures at the full offsets, gn_fixture(full=True))
  tiny        : 1e-4 N(0, 1): var = 1e-8 << eps -- eps must sit INSIDE the square root
  big         : 1e3 N(0, 1) + 1.3e3 at (1, 1024, 1280): sum x^2 of a group = 40960 * 2.69e6 = 1.1e11, a fifth of the 5.5e11 a slot holds
  const       : plain, but every element of group 0 of image 0 is 3.7: var = 0, the clamp of a negative variance, no NaN / inf
  outlier     : N(0, 1) with one element of 1e3 per (image, group)
LayerNorm fixtures (x (rows, C)): plain (3 N(0, 1) + 1), offset64 (N(0, 1) +- 64 by row, at every width: the two-pass
kernels show no kappa growth), tiny, const (row 0 is 3.7 everywhere).
Softmax fixtures take the scale, so that the logits AFTER scaling are what the name says: diffuse (2 N(0, 1)), one_hot (one logit 1e4
above N(0, 1)), equal (all logits of a row equal: 1 / cols).
Elementwise kernels: VALUE_GRID mixed into 2.5 N(0, 1) (every other element).
Column sums: N(0, 1) plus the cancelling pair +-1e6 in one column (an fp32 accumulator would lose that column's sum).
"""
import functools
import math
import zlib

import torch

import attention_f64 as A

U24 = 2.0 ** -24          # unit roundoff of fp32
MUTANTS = ("eps_outside_sqrt", "var_n_minus_1", "per_channel_stats", "batch_shared_stats", "silu_grad_no_z_term", "no_gamma_in_ds_db",
           "ignore_w_plus_one", "group_row_by_block", "drop_last_row_of_split", "scale_after_max", "inv_n_of_32_groups",
           "param_sum_skips_last_image", "dw_drops_group_last_row")

VALUE_GRID = [s * v for v in (0.0, 1e-8, 0.5, 5.0, 9.0, 30.0, 88.0, 100.0, 1e4) for s in (1.0, -1.0)]
ACT_GELU, ACT_SILU = 1, 2          # MVD_ACT_GELU, MVD_ACT_SILU


def _f64(t):
    return t.detach().double().cpu()


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def f32(v):
    """The value a C float argument carries (scale, eps): the kernels compute with that, not with the Python double."""
    return float(torch.tensor(v, dtype=torch.float32))


def sigmoid(z):
    return 1.0 / (1.0 + torch.exp(-z))


def silu(z):
    return z * sigmoid(z)


def silu_grad(z, mutant=None):
    s = sigmoid(z)
    return s if mutant == "silu_grad_no_z_term" else s * (1.0 + z * (1.0 - s))


def gelu(z):
    return z * 0.5 * torch.special.erfc(-z / math.sqrt(2.0))


def gelu_grad(z):
    return 0.5 * torch.special.erfc(-z / math.sqrt(2.0)) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


# ------------------------------------------------------------------------------------------------ the acceptance rule
def worst(got, ref, bar, groups):
    """got, ref: tensors whose leading `groups` entries (after reshape) are the comparison groups; bar (groups,) ABSOLUTE bound of a
    group.  -> the worst  max|got - ref| / bar  over the groups; a value that is not finite counts as an infinite error."""
    err = (_f64(got) - _f64(ref)).abs().reshape(groups, -1)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return float((err.amax(1) / _f64(bar).reshape(groups).clamp_min(1e-300)).max())          # (a bar of 0 demands the exact value)


def group_max(ref, groups):
    return _f64(ref).abs().reshape(groups, -1).amax(1)


# ------------------------------------------------------------------------------------------------ GroupNorm
def by_group(t, G):
    """(B, HW, C) -> one row per (image, group): (B*G, HW * C/G)"""
    B, HW, C = t.shape
    return t.reshape(B, HW, G, C // G).permute(0, 2, 1, 3).reshape(B * G, HW * (C // G))


def gn_moments(x, G, eps, mutant=None):
    """x (B, HW, C) -> mean, rstd (B, 1, C) float64 (per channel of its group)"""
    B, HW, C = x.shape
    x = _f64(x)
    xg = x.reshape(B, HW, G, C // G)
    dims = (1, 3)
    if mutant == "per_channel_stats":
        dims = (1,)
    if mutant == "batch_shared_stats":
        dims = (0, 1, 3)
    n = 1
    for d in dims:
        n *= xg.shape[d]
    mean = xg.mean(dims, keepdim=True)
    var = ((xg - mean) ** 2).sum(dims, keepdim=True) / (n - 1 if mutant == "var_n_minus_1" and n > 1 else n)
    rstd = 1.0 / (var.sqrt() + eps) if mutant == "eps_outside_sqrt" else 1.0 / (var + eps).sqrt()
    full = lambda t: t.expand(B, 1, G, C // G).reshape(B, 1, C)
    return full(mean), full(rstd)


def gn_kappa(x, G, eps):
    """(B*G,): (mean^2 + var) / (var + eps) of every (image, group)"""
    xg = by_group(_f64(x), G)
    mean = xg.mean(1)
    var = ((xg - mean[:, None]) ** 2).mean(1)
    return (mean * mean + var) / (var + eps)


def gn_forward(x, gamma, beta, G, eps, silu_flag=False, round_f16=False, mutant=None):
    """act(GroupNorm(x) * gamma + beta), x (B, HW, C): `silu` bit 0 of the C ABI = silu_flag, bit 1 = round_f16 (the normalised value is
    rounded to fp16 before the activation)."""
    mean, rstd = gn_moments(x, G, f32(eps), mutant)
    y = (_f64(x) - mean) * rstd * _f64(gamma) + _f64(beta)
    if round_f16:
        y = y.float().half().double()
    return silu(y) if silu_flag else y


def gn_backward(x, dy, gamma, beta, G, eps, silu_flag=False, mutant=None, with_abs=False):
    """-> dx (B, HW, C), dgamma (C,), dbeta (C,) of y = act(xhat * gamma + beta); with_abs: also sum |dz xhat| and sum |dz| per channel,
    the magnitudes the two parameter sums are accurate to (fp64 accumulation of terms that carry an fp32 rounding each)."""
    B, HW, C = x.shape
    cg = C // G
    mean, rstd = gn_moments(x, G, f32(eps))
    gm, bt = _f64(gamma), _f64(beta)
    xh = (_f64(x) - mean) * rstd
    dz = _f64(dy) * (silu_grad(xh * gm + bt, mutant) if silu_flag else 1.0)
    s1, s2 = dz.sum(1), (dz * xh).sum(1)                                         # (B, C)
    gw = torch.ones_like(gm) if mutant == "no_gamma_in_ds_db" else gm
    grp = lambda t: t.reshape(B, G, cg).sum(2, keepdim=True).expand(B, G, cg).reshape(B, 1, C)
    ds, db = grp(s2 * gw), grp(s1 * gw)
    n = HW * (C // 32 if mutant == "inv_n_of_32_groups" else cg)
    dx = rstd * (gm * dz - (xh * ds + db) / n)
    nb = B - 1 if mutant == "param_sum_skips_last_image" and B > 1 else B
    if with_abs:          # (..., sum |dz xhat|, sum |dz|, and what a shift of xhat moves dbeta by: |gamma| max|silu''| sum |dy|)
        shift_b = 0.5 * gm.abs() * _f64(dy).abs().sum((0, 1)) if silu_flag else torch.zeros_like(gm)
        return dx, s2[:nb].sum(0), s1[:nb].sum(0), (dz * xh).abs().sum((0, 1)), dz.abs().sum((0, 1)), shift_b
    return dx, s2[:nb].sum(0), s1[:nb].sum(0)


def gn_params(C):
    g = _gen("gn_params", C)
    sign = lambda: torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    return sign() * (1.0 + 0.3 * torch.randn(C, generator=g)), sign() * (0.3 + 0.3 * torch.randn(C, generator=g).abs())


@functools.lru_cache(maxsize=None)
def gn_fixture(name, B, HW, C, G, full=False):
    """-> x (B, HW, C) fp32 -- built once, shared, never modified.  full: the offsets at 8 | 64 | 4 sigma whatever the group size (the
    backward, whose moments are fp64: no kappa growth to make room for)"""
    g = _gen("gn", name, B, HW, C, G)
    z = torch.randn(B, HW, C, generator=g)
    cg = C // G
    if name in ("plain", "const"):
        x = z * 2 + 0.5
        if name == "const":
            x[0, :, :cg] = 3.7
    elif name in ("offset8", "offset64"):
        sign = torch.where(torch.arange(C) // cg % 2 == 0, 1.0, -1.0)
        x = z + sign * gn_offset(name, 512 if full else HW * cg)
    elif name == "chan_offset":
        x = z + gn_offset("offset4", 512 if full else HW * cg) * torch.randn(C, generator=g)
    elif name == "tiny":
        x = z * 1e-4
    elif name == "big":
        x = z * 1e3 + 1.3e3
    elif name == "outlier":
        x = by_group(z, G).clone()
        x[torch.arange(B * G), torch.randint(0, HW * cg, (B * G,), generator=g)] = 1e3
        x = x.reshape(B, G, HW, cg).permute(0, 2, 1, 3).reshape(B, HW, C).contiguous()
    else:
        raise KeyError(name)
    return x


def gn_offset(name, n):
    """|group mean| / sigma of offset8 / offset64 for a group of n elements: 8 | 64, made milder by (n / 512)^2 below 512 elements."""
    return float(name[6:]) * min(1.0, n / 512.0) ** 2


def gn_dy(B, HW, C):
    return torch.randn(B, HW, C, generator=_gen("gn_dy", B, HW, C))


def gn_accum_len(HW, C):
    """The longest per-thread fp32 accumulation of gn_stats_kernel: ceil(rows of a chunk / TY)."""
    rows = HW // gn_chunks(HW)
    return -(-rows // gn_ty(C))


def gn_chunks(HW):
    c = max(1, min(128, HW // 8))
    while HW % c:
        c -= 1
    return c


def gn_ty(C):
    tx = min(C // 4, 256)
    return 1 if C > 640 else min(256 // tx, 4)


def producer_accum_len(path, cg):
    """The longest sequential fp32 accumulation behind a statistics slot, read from the producers: "slab" (concat_stats_kernel,
    splitk_reduce_stats_kernel): 4 rows per thread, the 4 row quarters of the 16-row slab, then the cg columns of the group in column
    order: cg + 6 additions; "tile" (the GEMM tile epilogue, gemm_device.hpp): the rows of the wave tile in row order -- up to 64 over
    the tile shapes -- then the group's columns: 64 + cg - 1; "fused" (concat_gn_kernel, splitk_gn_kernel: a few elements per thread,
    everything else in fp64) and a slot written from float64: 1."""
    return {"slab": cg + 6, "tile": 64 + cg - 1, "fused": 1, "written": 1}[path]


def gn_forward_bar(kappa, ref_max, pl, R=1):
    """ABSOLUTE bound per (image, group) of every forward GroupNorm path:  (PL + 3e-6 + c 2^-24 kappa) max|ref_g|.

    PL + 3e-6 is the project's bar (tests/test_gpu_ops.py::test_groupnorm).  The kappa term is derived: all forward paths form
    var = E[x^2] - mean^2 from fp32 partial sums.  Each x^2 is rounded to 2^-24 relative, so sum x^2 and with it E[x^2] carry <= 2^-24
    relative = 2^-24 (mean^2 + var) absolute; divided by var + eps that is 2^-24 kappa relative in var + eps and half of it in rstd.  The
    fp32 mean in the folded shift beta - mean * a adds 2^-24 |mean| rstd = 2^-24 sqrt(kappa) <= 2^-24 kappa / 2 for kappa >= 4.  c = 1.
    R is the longest sequential fp32 accumulation of the path (gn_accum_len for gn_stats_kernel: <= 8 at the 8-rows-per-workgroup
    geometry the kernel was laid out for).  A sequential fp32 sum of R terms of one sign adds up to (R - 1) 2^-24 relative on top of
    the rounding of the terms; where the geometry degenerates (a prime HW: ONE chunk, R = HW / TY) the bound of that path is
    c = (R + 1) / 2 -- half of the worst case R + 1 roundings, as the emulation's 0.5 is of the bar.  R <= 16, twice the laid-out
    length, keeps c = 1 (the emulation of (1, 37, 64), R = 10, stays under 0.1 of it); (1, 1021, 128), R = 256, is the one case list
    entry beyond: there the emulation reaches 2.6 x the c = 1 bar on offset64, i.e. the ALGORITHM leaves c = 1, and 0.02 of c = 128.5."""
    c = 1.0 if R <= 16 else (R + 1) / 2.0
    return (pl + 3e-6 + c * U24 * kappa) * ref_max


def gn_slot_quantum(x, gamma, G, eps):
    """ABSOLUTE term per (image, group) of every path behind a statistics SLOT:  2^-25 / n * rstd * max|gamma_g|.  The slot holds
    llrint(sum * 2^24): the sum is resolved to 2^-25, the mean to 2^-25 / n, and (x - mean) rstd gamma moves by that times rstd gamma.
    Negligible (< 1e-8) unless the group has a handful of elements AND no variance -- HW = 1 with one channel per group: there
    rstd = eps^-0.5 = 316 and the term is 1e-5 |gamma|, above the rest of the bar."""
    B, HW, C = x.shape
    xg = by_group(_f64(x), G)
    var = ((xg - xg.mean(1, keepdim=True)) ** 2).mean(1)
    gmax = _f64(gamma).abs().reshape(G, C // G).amax(1).repeat(B)
    return 2.0 ** -25 / xg.shape[1] / (var + f32(eps)).sqrt() * gmax


PARAM_FLOOR = 4.0 * U24


def gn_param_bar(ref, kappa_g, G, abs_terms, abs_shift=None):
    """ABSOLUTE bound per CHANNEL of dgamma / dbeta:  stable_bar(5e-6, kappa_g, max|ref| of the channel's group)  plus a rounding floor
    4 * 2^-24 * sum |terms| of the channel (abs_terms).  The kernels add fp32-rounded terms in fp64: a term dz * xhat carries the
    roundings of x - mean, * rstd, of dz and of the stored partial sum -- four of 2^-24 -- so the sum is off by that share of the sum of
    MAGNITUDES whatever the terms cancel to; in a group of one or two channels max|ref_g| can cancel to nearly nothing and the floor is
    then the whole bar (a group of 3.7s: both are 0 and the kernel must return exactly 0).  abs_shift: the group's mean rounded to fp32
    moves EVERY xhat of the group by the same 2^-24 sqrt(kappa): dgamma by that times sum dz (abs_shift = sum |dz|), and behind the SiLU
    dbeta too, through z = xhat gamma + beta and |silu''| <= 1/2 (abs_shift = |gamma| sum |dy| / 2; without SiLU dz = dy and nothing)."""
    C = ref.numel()
    per = lambda t: _f64(t).reshape(G, 1).expand(G, C // G).reshape(C)
    bar = per(stable_bar(5e-6, kappa_g, group_max(ref, G))) + PARAM_FLOOR * _f64(abs_terms)
    return bar if abs_shift is None else bar + U24 * per(kappa_g.sqrt()) * _f64(abs_shift)


def ln_dw_bar(x, dy, dw_ref, eps, rows_per_group):
    """ABSOLUTE bound per element of dw (ngroups, C):  stable_bar(5e-6, worst kappa of the group's rows, max|dw_g|)  plus the floor
    sum_r |dy_rc| (4 * 2^-24 |xhat_rc| + 2^-23 sqrt(kappa_r)):  dw_c = sum_r dy_rc xhat_rc in fp64 over fp32 terms; xhat_rc carries its
    own roundings (relative) and the row's fp32 mean (ABSOLUTE 2^-23 sqrt(kappa_r), as in stable_bar), each weighted by |dy_rc|.  For a
    constant row the reference is 0 and only the second part is left."""
    rows, C = x.shape
    ng = rows // rows_per_group
    mean, rstd = ln_moments(x, eps)
    kap = ln_kappa(x, eps)
    xh = ((_f64(x) - mean) * rstd).abs()
    floor = (_f64(dy).abs() * (PARAM_FLOOR * xh + 2.0 * U24 * kap.sqrt()[:, None])).reshape(ng, rows_per_group, C).sum(1)
    base = stable_bar(5e-6, kap.reshape(ng, rows_per_group).amax(1), group_max(dw_ref, ng))
    return base[:, None] + floor


def stable_bar(base, kappa, ref_max):
    """GroupNorm backward, LayerNorm forward / backward:  (base + 2^-23 sqrt(kappa)) max|ref| of the group / row.  These paths take the
    variance in fp64 (gn_moments_kernel) or in two passes (ln_kernel, ln_bwd_kernel); only the mean rounded to fp32 enters xhat:
    |mean| 2^-24 rstd = 2^-24 sqrt(kappa) per element, twice for the mean's own accumulation."""
    return (base + 2.0 * U24 * kappa.sqrt()) * ref_max


# B, HW, C, groups                                            the branch it reaches
GN_SHAPES = [
    (1, 16, 32, 32),        # cg = 1
    (2, 64, 320, 32),       # TX = 80: idle threads
    (1, 36, 96, 32),        # chunks = 4 of 9 rows
    (1, 37, 64, 32),        # prime HW: one chunk
    (1, 1021, 128, 32),     # prime HW: 256-term fp32 partials
    (3, 8, 640, 32),        # either side of the TY rule ...
    (1, 8, 672, 32),
    (2, 16, 2560, 32),      # largest C
    (1, 4096, 32, 32),      # 128 chunks
    (1, 16, 128, 64),       # groups != 32
    (1, 16, 64, 8),
]
GN_FIXTURES = ("plain", "offset8", "offset64", "chan_offset", "tiny", "const", "outlier")
GN_BIG = (1, 1024, 1280, 32)
GN_F16_CASE = ((2, 64, 320, 32), "plain")
GN_EPS = 1e-5


def gn_cases():
    """(shape, fixture) of mvd_groupnorm_nhwc; each runs with SiLU off and on."""
    return [(s, fx) for s in GN_SHAPES for fx in GN_FIXTURES] + [(GN_BIG, "big")]


# leg 1 of mvd_groupnorm_from_stats (statistics written by the test): B, HW, C (32 groups)
GN_STATS_SHAPES = [
    (1, 1024, 320),         # row-chunk kernel
    (1, 1024, 352),         # just outside it ...
    (2, 1008, 320),
    (1, 100, 96),           # TX = 24, TY = 10, ragged last block, cg = 3 straddling a float4
    (2, 16, 32),            # cg = 1
    (2, 16, 64),            # cg = 2
    (1, 64, 1920),          # TX = 240, two column slabs
    (1, 16, 2560),          # largest C
    (1, 1, 32),             # single row
]
GN_STATS_FIXTURES = ("plain", "offset64", "const", "outlier")


def gn_stats_cases():
    return [(s + (32,), fx) for s in GN_STATS_SHAPES for fx in GN_STATS_FIXTURES]


def gn_fixed_point_stats(x, G):
    """The producers' slot written from float64: llrint(sum * 2^24), llrint(sum of squares * 2^24) per (image, group) -> int64 (B, G, 2)"""
    B = x.shape[0]
    xg = by_group(_f64(x), G)
    return torch.stack([xg.sum(1), (xg * xg).sum(1)], 1).mul(2.0 ** 24).round().to(torch.int64).reshape(B, G, 2)


GN_BWD_SHAPES = [(1, 16, 32, 32), (2, 64, 320, 32), (1, 37, 64, 32), (3, 8, 1280, 32), (1, 1024, 64, 32), (1, 16, 128, 64), (1, 16, 64, 8)]
GN_BWD_FIXTURES = ("plain", "offset64", "chan_offset", "const", "outlier")


def gn_bwd_cases():
    return [(s, fx) for s in GN_BWD_SHAPES for fx in GN_BWD_FIXTURES]


# ------------------------------------------------------------------------------------------------ LayerNorm
def _group_rows(rows, rows_per_group, mutant=None):
    r = torch.arange(rows)
    if mutant == "group_row_by_block":
        r = r // 4 * 4
    return r // rows_per_group


def ln_moments(x, eps):
    x = _f64(x)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    return mean, 1.0 / (var + f32(eps)).sqrt()


def ln_kappa(x, eps):
    x = _f64(x)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    return (mean * mean + var) / (var + eps)


def ln_forward(x, w, b, eps, w_plus_one=False, rows_per_group=None, mutant=None):
    """x (rows, C); w, b: None, (C,) or one row per row group (ngroups, C) -> (rows, C)"""
    rows = x.shape[0]
    mean, rstd = ln_moments(x, eps)
    y = (_f64(x) - mean) * rstd
    pick = _group_rows(rows, rows_per_group or rows, mutant)
    if w is not None:
        wf = _f64(w).reshape(-1, x.shape[1])[pick]
        y = y * (wf + 1.0 if w_plus_one and mutant != "ignore_w_plus_one" else wf)
    if b is not None:
        y = y + _f64(b).reshape(-1, x.shape[1])[pick]
    return y


def ln_backward(x, dy, w, eps, rows_per_group=None, mutant=None):
    """Backward of y = xhat * w + b with w None, (C,) or (ngroups, C):  dx (rows, C), dw, db (ngroups, C) = per row group the column
    sums of dy * xhat and of dy."""
    rows, C = x.shape
    rpg = rows_per_group or rows
    mean, rstd = ln_moments(x, eps)
    xh = (_f64(x) - mean) * rstd
    d = _f64(dy)
    dz = d if w is None else d * _f64(w).reshape(-1, C)[_group_rows(rows, rpg, mutant)]
    dx = rstd * (dz - dz.mean(1, keepdim=True) - xh * (dz * xh).mean(1, keepdim=True))
    keep = torch.ones(rpg, 1, dtype=torch.float64)
    if mutant == "dw_drops_group_last_row" and rpg > 1:
        keep[-1] = 0.0
    return dx, ((d * xh).reshape(rows // rpg, rpg, C) * keep).sum(1), (d.reshape(rows // rpg, rpg, C) * keep).sum(1)


@functools.lru_cache(maxsize=None)
def ln_fixture(name, rows, C):
    g = _gen("ln", name, rows, C)
    z = torch.randn(rows, C, generator=g)
    if name in ("plain", "const"):
        x = z * 3 + 1
        if name == "const":
            x[0] = 3.7
    elif name == "offset64":
        x = z + torch.where(torch.arange(rows) % 2 == 0, 64.0, -64.0)[:, None]
    elif name == "tiny":
        x = z * 1e-4
    else:
        raise KeyError(name)
    return x


def ln_modulation(ngroups, C):
    """(ngroups, 6 C): adaLN's modulation tensor, one row per row group (scene)"""
    return torch.randn(ngroups, 6 * C, generator=_gen("ln_modulation", ngroups, C))


def ln_params(ngroups, C, ld_mult=6):
    """w, b as the column slices [C, 2C) and [3C, 4C) of ln_modulation (adaLN's chunk(6): row stride 6 C); ld_mult = 1: plain contiguous
    (ngroups, C) tensors."""
    if ld_mult == 1:          # |w| near 1 as in gn_params: a row of 4 elements then has max|ref| ~ max|w|, what the bar assumes; b ~ N(0, 1)
        g = _gen("ln_params", ngroups, C)
        sign = torch.where(torch.rand(ngroups, C, generator=g) < 0.5, -1.0, 1.0)
        return sign * (1.0 + 0.3 * torch.randn(ngroups, C, generator=g)), torch.randn(ngroups, C, generator=g)
    mod = ln_modulation(ngroups, C)
    return mod[:, C:2 * C], mod[:, 3 * C:4 * C]


LN_FIXTURES = ("plain", "offset64", "tiny", "const")
LN_ROWS = (1, 5, 37)
LN_PLANES_C = (32, 256, 288, 512, 544, 1280)       # split planes + fp32 output: MAXV changes at 256 and 512
LN_F32_C = (4, 36, 260)                            # fp32 output only
LN_GROUPS = [(3, 5), (7, 2)]                       # rows_per_group, ngroups: a 4-row block of the kernel straddles groups
LN_GROUPS_C = (32, 288)
LN_EPS = 1e-5
LN_BWD_C = (1, 63, 65, 320, 1280, 1283)


def ln_cases():
    """(rows, C, rows_per_group or 0, w_plus_one)"""
    out = [(r, C, 0, wp1) for r in LN_ROWS for C in LN_PLANES_C + LN_F32_C for wp1 in (False, True)]
    return out + [(rpg * ng, C, rpg, True) for rpg, ng in LN_GROUPS for C in LN_GROUPS_C]


def ln_bwd_cases():
    """(rows, C, rows_per_group or 0)"""
    return [(r, C, 0) for r in LN_ROWS for C in LN_BWD_C] + [(rpg * ng, C, rpg) for rpg, ng in LN_GROUPS for C in (63, 320)]


# ------------------------------------------------------------------------------------------------ softmax
def softmax_rows(x, scale, out_scale=1.0, mutant=None):
    """out_scale * softmax(scale * x[r, :]) -- x (rows, cols) (the caller slices a wider matrix)"""
    x, s = _f64(x), f32(scale)
    if mutant == "scale_after_max":
        e = ((x - x.amax(1, keepdim=True)) * s).exp()
    else:
        z = x * s
        e = (z - z.amax(1, keepdim=True)).exp()
    return out_scale * e / e.sum(1, keepdim=True)


SOFTMAX_SHAPES = [(1, 32, 32), (5, 4096, 4096), (7, 96, 128), (9, 1024, 1024)]        # rows, cols, ldx
SOFTMAX_FIXTURES = ("diffuse", "one_hot", "equal")
SOFTMAX_SCALES = (1.0, 0.05, 40.0, -1.0)      # (the negative one: the maximum has to be taken of the SCALED logits)
SOFTMAX_OUT_SCALE = 1024.0


@functools.lru_cache(maxsize=None)
def softmax_fixture(name, rows, cols, ldx, scale):
    """-> x (rows, ldx) fp32; the columns [cols, ldx) hold 3e4 (part of no row's softmax)"""
    g = _gen("softmax", name, rows, cols, ldx, scale)
    if name == "diffuse":
        z = 2.0 * torch.randn(rows, cols, generator=g)
    elif name == "one_hot":
        z = torch.randn(rows, cols, generator=g)
        z[torch.arange(rows), torch.randint(0, cols, (rows,), generator=g)] += 1e4
    elif name == "equal":
        z = (3.0 * torch.randn(rows, 1, generator=g)).expand(rows, cols)
    else:
        raise KeyError(name)
    x = torch.full((rows, ldx), 3e4)
    x[:, :cols] = z / scale
    return x


def softmax_cases():
    return [(s, fx, sc) for s in SOFTMAX_SHAPES for fx in SOFTMAX_FIXTURES for sc in SOFTMAX_SCALES]


# ------------------------------------------------------------------------------------------------ column sums
def col_sum_splits(rows):
    return max(1, min(64, rows // 256))


def col_sum(x, ngroups=1, mutant=None):
    """x (ngroups * rows, cols) -> (ngroups, cols): the column sums of each row group"""
    x = _f64(x)
    rows = x.shape[0] // ngroups
    xg = x.reshape(ngroups, rows, -1).clone()
    if mutant == "drop_last_row_of_split":
        splits = col_sum_splits(rows)
        per = -(-rows // splits)
        for k in range(splits):
            if k * per < rows:
                xg[:, min(rows, (k + 1) * per) - 1] = 0.0
    return xg.sum(1)


def col_sum_bar(x, ref, ngroups=1):
    """ABSOLUTE bound per column:  2^-23 |ref| + 2^-45 sum |x|.  The kernels accumulate in fp64 in a fixed order and round ONCE to fp32:
    2^-24 |ref| (2^-23 leaves room for the float64 reference's own last bit after that rounding); the fp64 accumulation of n terms is
    off by at most n 2^-53 sum |x|, and 2^-45 is that with a margin of 2^8 over the n <= 2^8 * 64 = 16384 rows a launch of 64 splits
    spends per column at the largest row count tested."""
    ax = _f64(x).abs().reshape(ngroups, -1, x.shape[-1]).sum(1)
    return 2.0 ** -23 * _f64(ref).abs() + 2.0 ** -45 * ax


def pow2_scale(x):
    """{s, 1/s}: the power of two s that brings max|x| into [1024, 2048); 1 when the maximum is 0"""
    m = float(_f64(x).abs().max())
    if m == 0.0 or not math.isfinite(m):
        return 1.0, 1.0
    s = 2.0 ** (10 - (math.frexp(m)[1] - 1))
    return s, 1.0 / s


COL_SUM_ROWS = (1, 7, 255, 256, 257, 513, 16385)
COL_SUM_COLS = (1, 31, 33, 320)
COL_SUM_GROUPS = [(3, 300), (2, 520)]            # ngroups, rows per group


@functools.lru_cache(maxsize=None)
def col_sum_fixture(rows, cols, ld=None):
    """-> x (rows, ld) fp32; the sums run over the columns [0, cols).  N(0, 1), and in column cols // 2 the pair +1e6 / -1e6 in the first
    and the last row (rows >= 2)."""
    ld = ld or cols
    x = torch.randn(rows, ld, generator=_gen("col_sum", rows, cols, ld))
    if rows >= 2:
        x[0, cols // 2], x[rows - 1, cols // 2] = 1e6, -1e6
    return x


# ------------------------------------------------------------------------------------------------ elementwise kernels
def value_grid(rows, cols, tag=""):
    """2.5 N(0, 1) with VALUE_GRID cycled through every other element (stride 7 through the grid, so that neighbouring columns -- the
    a and g halves of a GEGLU row -- meet in changing pairs)"""
    x = 2.5 * torch.randn(rows * cols, generator=_gen("grid", rows, cols, tag))
    idx = torch.arange(0, rows * cols, 2)
    x[idx] = torch.tensor(VALUE_GRID)[(idx // 2 * 7) % len(VALUE_GRID)]
    return x.reshape(rows, cols)


def act_forward(x, act):
    return gelu(_f64(x)) if act == ACT_GELU else silu(_f64(x))


def act_backward(dy, x, act, mutant=None):
    return _f64(dy) * (gelu_grad(_f64(x)) if act == ACT_GELU else silu_grad(_f64(x), mutant))


def geglu_backward(h, dy):
    """y = a * gelu(g), [a | g] = h (rows, 2 * half) -> dh (rows, 2 * half) and the FLOOR of each element's bar: the factor in front of
    the activation term: |dy| min(|g|, 1) for the a half (dy * g * Phi(g): |dy| as the issue has it, and relative to g where g is tiny)
    and |dy a| for the g half (dy * a * gelu'(g): a multiplies the incoming gradient of the gate before gelu' does)."""
    h, d = _f64(h), _f64(dy)
    half = d.shape[1]
    a, g = h[:, :half], h[:, half:]
    return torch.cat([d * gelu(g), d * a * gelu_grad(g)], 1), torch.cat([d.abs() * g.abs().clamp_max(1.0), (d * a).abs()], 1)


def elementwise_bar(ref, floor, tol=3e-6):
    """ABSOLUTE bound per ELEMENT: tol max(|ref|, floor).  The project's 2e-6 / 3e-6 bars (tests/test_gpu_backward.py) applied to every
    element instead of the tensor's maximum.  floor: |dy| for dy act'(x) (the issue's max(|ref|, |dy| * 1)); min(|x|, 1) for the
    forward act(x) = x gate(x), which has no dy; GEGLU: see geglu_backward.  Gate and derivative are O(1) quantities evaluated to ~2^-23
    ABSOLUTE (1 + erf cancels for negative arguments), so where they are tiny the error is relative to their factor, not to the result."""
    return tol * torch.maximum(_f64(ref).abs(), _f64(floor))


ELEMENTWISE_SHAPES = [(1, 1), (3, 7), (37, 50)]
GEGLU_BIG = (1025, 1024)         # rows, half: 1 049 600 elements, one more than 4096 workgroups of 256 threads take in one pass
ACT_BIG = (2049, 1024)           # 2 098 176 elements (act_backward), 524 544 float4 columns (act_planes): past 8192 x 256 / past one pass


# ------------------------------------------------------------------------------------------------ per-pixel cross-attention backward
def pixel_xattn_backward(q, k, v, dout, P, D, H, d):
    """Backward of attention_f64.pixel_cross_attention.  -> (dq (P, C), dk, dv (P*D, C)) and their scales per (pixel, head) (P*H,):
    the magnitudes the kernel's roundings are relative to -- dS_j = P_j (dP_j - delta) is a DIFFERENCE of numbers of size max|dP| (it
    is ~0 where one key wins), so dq is accurate relative to d^-0.5 max|dP| max|k|, dk to d^-0.5 max|dP| max|q|, dv to max|dout|."""
    qh = _f64(q).reshape(P, 1, H, d).permute(0, 2, 1, 3)                              # (P, H, 1, d)
    doh = _f64(dout).reshape(P, 1, H, d).permute(0, 2, 1, 3)
    kh, vh = (_f64(t).reshape(P, D, H, d).permute(0, 2, 1, 3) for t in (k, v))         # (P, H, D, d)
    sc = d ** -0.5
    p = A._softmax(qh @ kh.transpose(-1, -2) * sc)                                     # (P, H, 1, D)
    dp = doh @ vh.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True)) * sc
    dq = (ds @ kh).permute(0, 2, 1, 3).reshape(P, H * d)
    dk = (ds.transpose(-1, -2) @ qh).permute(0, 2, 1, 3).reshape(P * D, H * d)
    dv = (p.transpose(-1, -2) @ doh).permute(0, 2, 1, 3).reshape(P * D, H * d)
    amax = lambda t: t.abs().amax((-1, -2)).reshape(P * H)
    dpm = amax(dp) * sc
    return (dq, dk, dv), (dpm * amax(kh), dpm * amax(qh), amax(doh))


def pixel_by_head(t, P, D, H, d):
    """(P*D, H*d) -> one row per (pixel, head): (P*H, D*d)"""
    return t.reshape(P, D, H, d).permute(0, 2, 1, 3).reshape(P * H, D * d)


PIXEL_BWD_CASES = [(5, 1, 3, 8), (7, 3, 1, 40), (2, 5, 5, 68), (3, 8, 2, 160)]      # P, D, heads, dhead
PIXEL_BWD_FIXTURES = {"diffuse": "diffuse", "one_hot": "large"}                      # -> attention_f64.pixel_fixture


def pixel_bwd_fixture(name, P, D, H, d):
    q, k, v = A.pixel_fixture(PIXEL_BWD_FIXTURES[name], P, D, H, d)
    return q, k, v, torch.randn(P, H * d, generator=_gen("pixel_dout", name, P, D, H, d))
