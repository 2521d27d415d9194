"""FLOAT64 statements of the GEMM family (csrc/gemm.hip, gemm_device.hpp, gemm_plain*.hip, gemm_patch.hip, gemm_ws.hip: mvd_gemm and the
weight packers), the fixtures the GPU tests feed to it, the PER-ELEMENT bars they apply, the case lists they run and the mutants that prove
the suite has teeth (tests/test_gpu_gemm_f64.py runs the kernels; tests/test_cpu_gemm_f64.py shows on the CPU that oracles, fixtures and
bars reject every mutant and that an fp32 emulation of the split-operand algorithm stays below half of every bar).  CPU only, float64
tensor arithmetic written from the formulas of include/mvd_hip.h: no F.linear, no F.conv2d, no autograd in here.

What an oracle returns.  (ref, S): the float64 result from the fp32 tensors the kernel gets, and per output element the sum of the magnitudes
of everything added into it -- sum_k |a_mk| |w_nk| |acc_scale| + |bias| + |bias_b| carried through the activation (times its Lipschitz
constant ACT_LIP) and |colscale|, plus |res|.  `*_terms` return a dict that also holds F, the weight of the absolute floor (below).

Fixtures (seeded by name and shape; DENSE_FIXTURES / CONV_FIXTURES):
  plain     N(0, 1) activations, N(0, 1) / sqrt(K) weights, N(0, 1) bias / residual / column scale: as tests/test_gpu_ops.py.
  graded    plain, row m of A times 2^-(m % 11) (a conv: pixel row m of the NHWC image) and weight row n times 2^-(n % 13): every output
            element has its own magnitude, over 22 binades -- a per-tensor bar sees one element in a hundred.  Bias, residual and the
            per-view bias follow the grading (a kernel's error in a small element must not hide behind an O(1) addend's S).
  cancel    A = |N(0, 1)| + 3, the sign of W alternates along k: |ref| << S.  The bar is on S, which the oracle knows and |ref| hides.
  geometry  EXACT in every precision and both flavours (integers of magnitude <= 255 are exact in 8 significant bits; one-hot weights):
            dense -- A holds integers in [-255, 255], row n of W is 1 at k = pi(n) (pi = a seeded permutation of the K columns, continued
            periodically when N > K): out[m, n] == A[m, pi(n)] bit for bit under every cfg and every split count;
            convolution -- input channels 0, 1, 2 hold y + 1, x + 1, b + 1 of their pixel and every other channel 77; output channel
            3 * tap + j (tap = ky * 3 + kx, j < 3, channel < 27) is 1 at (input channel j, tap) and 0 elsewhere: the output is the
            coordinate + 1 of the pixel that tap reads, or 0 in the zero padding (the image index + 1 of channel 2 must never be a
            neighbour image's).  Output channels from 27 on are zero rows -- or, with a centre-tap tail, 1 at tail channel (n - 27) % 3,
            the tail operand holding (m % 251) + 1, (m % 13) + 1, 5.  Pins the taps, both padding conventions, the stride offset, the
            >> 1 of the upsample, the image boundary, the m -> (b, oy, ox) split and the four-tap form's row mapping.
Layouts (LAYOUTS): `packed` -- A (M, K) with 128 spare rows of +-3e4 behind it, every pitch equal to the width; `window` -- A is columns
[32, 32 + K) of a (M + 128, K + 64) buffer whose other columns and spare rows hold +-3e4, and res / out / bias_b have the pitches N + 4,
N + 8, N + 12.

Bars -- per element, never per tensor:      bar = (e_op + e_acc * 2^-24) * S + floor      (bar(), e_op(), e_acc())
  e_op   the operand contract of include/mvd_hip.h ("Operand range"; MVD_PREC_*).  An operand is stored as hi = rn16(x), lo = rn16(x - hi)
         (csrc/common.hpp: split_op16).  |x - hi| <= u |x| with u = 2^-11 (fp16: 11 significant bits) / 2^-8 (bf16: 8), x - hi is exact in
         fp32, and the rounding of lo leaves u |lo| <= u^2 |x|: 2^-22 / 2^-16 per operand with hi + lo (x3, x4), u with hi alone (x1).  A
         product of two operands carries both: e_op = 2 e + e^2.  x3 drops lo * lo, |lo_a lo_w| <= u^2 |a w|: + u^2.  The four-tap
         weights are composed in float64 and rounded once to fp32 before the split: + 2^-24.
  e_acc  fp32 roundings on the longest chain an element passes, counted from the code: every k-tile issues one MFMA 16x16x32 per partial
         product into the element's accumulator (gemm_plain.hpp: mfma_tile -- lo*lo, lo*hi, hi*lo, hi*hi: 4 / 3 / 1 per k-tile), and one
         instruction is one rounding of the accumulator (its 32 products are exact in fp32 and summed inside the instruction; the
         emulation of tests/test_cpu_gemm_f64.py takes the same single rounding): products * nk.  The split-K reduce adds the slabs in slice order: + splits - 1.  The epilogue:
         acc_scale, bias, bias_b, colscale, res: one rounding each, + 5; an activation + ACT_ROUNDINGS = 8 (csrc/common.hpp: the erf fit
         is good to 9.5e-8 = 1.6 * 2^-24 absolute, times |z| / 2; exp, the division and the products of SiLU / QuickGELU: under 6).  Every
         rounding is relative to a partial sum <= S, hence the product with S.
  floor  the absolute resolution the header documents (fp16 flavour): 2^-25 per activation element, 2^-25 / pack scale per weight
         element: floor = 2^-25 * F, F = (sum_k |w_nk| + sum_k |a_mk| / scale) |acc_scale| carried through the activation and the column
         scale like S.  Zero in the bf16 flavour (fp32's exponent range).  The fixtures keep every operand in fp16's range; graded rows
         of 2^-10 and weight rows 2^-12 below the largest have low parts in the subnormal range, where this term is what the contract gives.
  Behind an activation the bar of the pre-activation is multiplied by ACT_LIP = 1.13 (sup |gelu'| = 1.129, sup |silu'| = 1.0998, QuickGELU
  is silu(1.702 z) / 1.702: the same) -- by carrying S and F through it.  GEGLU: out = v gelu(g): S = S_v |gelu(g)| + |v| ACT_LIP S_g (+ the
  second-order product at the largest e_op, 2^-6).  A planes output adds PL |ref| (tests/test_gpu_ops.py: PL) and, fp16, 2^-24 absolute.
  The per-tensor TOL[prec] of tests/test_gpu_ops.py holds on top of all this, unchanged.

Mutants (MUTANTS): one realistic bug each, applied to the ORACLE; a (case, fixture) rejects a mutant when the mutated reference is more than
TWO bars from the true one (a kernel with that bug, itself within one bar of the mutated value, could then not pass), or differs at all on an
exact fixture.
"""
import collections
import functools
import math
import zlib

import torch

U24 = 2.0 ** -24
FMTS = ("f16", "bf16")
PRECS = (4, 3, 1)
ACT_NONE, ACT_GELU, ACT_SILU, ACT_QUICKGELU = 0, 1, 2, 3
ACT_LIP = 1.13
ACT_ROUNDINGS = 8
MFMA_ROUNDINGS = 1         # a 16x16x32 MFMA: 32 exact products and the accumulator, rounded once
LIMITS = dict(rows=384, cols=336, K=288)
SPARE_A_ROWS = 128
JUNK = 3.0e4

MUTANTS = ("swap_h_w", "no_pad_tl_ignored", "stride_tap_origin_0", "upsample_halves_before_bounds", "image_boundary_leaks",
           "patch_row_pitch_w", "up4_parity_swapped",
           "drop_last_ktile", "tail_reads_tap_0", "a_hi_only", "w_hi_only", "acc_scale_ignored", "window_off_by_32_columns",
           "res_pitch_is_ldo", "bias_b_row_from_tile_base", "colscale_inside_act", "geglu_halves_swapped",
           "short_last_split_reads_stale_slab", "packed_lane_order_n_major")

# ------------------------------------------------------------------------------------------------ case lists
# tiles are 64 / 128 rows by 64 / 80 / 128 / 160 columns, k-tiles 32 wide, LDS rings of up to 4 or 8 k-tiles, tiles dealt over 8 XCDs
DENSE_CASES = [(1, 16, 32), (17, 20, 32), (63, 48, 64), (65, 80, 96),
               (129, 96, 288),       # nk = 9: one past the longest ring
               (130, 176, 224),      # nk = 7, N past 160
               (257, 336, 160),      # 3 x 3 tiles of 128 x 128: the XCD remainder branch
               (37, 4, 160)]
GEGLU_CASES = [(17, 64, 32), (65, 96, 96), (129, 96, 288), (130, 192, 224)]          # N % 32 == 0 (value | gate halves of N / 2)
PLANES_CASES = [c for c in DENSE_CASES if c[1] % 16 == 0]                            # MVD_B_PLANES needs N % 16 == 0
ACC_SCALE_PLANES = 0.375
LAYOUTS = ("packed", "window")
DENSE_FIXTURES = ("plain", "graded", "cancel", "geometry")
CONV_FIXTURES = ("plain", "graded", "cancel", "geometry")


def rows_per_batch_list(M):
    return sorted({1, min(5, M), M})


def split_counts(nk):
    """1, 2, 3, nk, nk + 3 (clamped by the library to nk); 3 against nk = 7 leaves a short last slice."""
    return sorted({1, 2, 3, nk, nk + 3})


ConvCase = collections.namedtuple("ConvCase", "kind B Hin Win Cin Cout Hout Wout stride upsample no_pad_tl tail")


def _cc(kind, B, H, W, Cin, Cout, Ho=None, Wo=None, stride=1, upsample=0, no_pad_tl=0, tail=0):
    return ConvCase(kind, B, H, W, Cin, Cout, H if Ho is None else Ho, W if Wo is None else Wo, stride, upsample, no_pad_tl, tail)


CONV_CASES = [
    _cc("s1", 1, 1, 1, 32, 16), _cc("s1", 2, 3, 5, 32, 48), _cc("s1", 2, 5, 3, 32, 48), _cc("s1", 3, 2, 6, 64, 80),
    _cc("s1", 1, 16, 8, 32, 80), _cc("s1", 1, 8, 16, 32, 80),          # H * W = 128: the input-patch kernel serves both orientations
    _cc("s1", 4, 4, 8, 32, 80), _cc("s1", 4, 8, 4, 32, 80),            # four images per tile
    _cc("s1", 1, 2, 64, 32, 80),
    _cc("s1", 5, 4, 4, 32, 16),                                        # the tile runs past the last image
    _cc("s2", 2, 6, 10, 32, 48, 3, 5, stride=2), _cc("s2", 1, 5, 7, 32, 48, 3, 4, stride=2), _cc("s2", 2, 4, 2, 32, 48, 2, 1, stride=2),
    _cc("s2nopad", 2, 6, 10, 32, 48, 3, 5, stride=2, no_pad_tl=1), _cc("s2nopad", 1, 5, 7, 32, 48, 2, 3, stride=2, no_pad_tl=1),
    _cc("up9", 2, 3, 5, 32, 48, 6, 10, upsample=1), _cc("up9", 1, 1, 1, 32, 48, 2, 2, upsample=1),
    _cc("up4", 3, 6, 2, 32, 48, 12, 4, upsample=1),                    # the transpose of the non-square case of tests/test_gpu_up4.py
    _cc("tail", 2, 3, 5, 32, 48, tail=64), _cc("tail", 1, 16, 8, 32, 80, tail=96),
]
LINEAR_BACKWARD_CASES = [(65, 20, 96), (130, 5, 32)]                                  # (M, N, K)
CONV_BACKWARD_CASES = [(2, 3, 5, 32, 48), (1, 8, 16, 64, 5)]                          # (B, H, W, Cin, Cout)
PACK_LINEAR_CASES = [(1, 1), (17, 33), (48, 96), (5, 320)]                            # (N, K)
PACK_CONV_CASES = [(5, 10), (48, 64)]                                                 # (Cout, Cin)


def case_id(c):
    if isinstance(c, ConvCase):
        return f"{c.kind}-{c.B}x{c.Hin}x{c.Win}x{c.Cin}-{c.Cout}" + (f"-t{c.tail}" if c.tail else "")
    return "-".join(str(x) for x in c)


def conv_M(c):
    return c.B * c.Hout * c.Wout


def conv_K(c):
    return (4 if c.kind == "up4" else 9) * c.Cin + c.tail


# the store-epilogue variants every dense (case, fixture, layout, prec) runs: together every option of MVD_EPI_STORE
EPILOGUES = collections.OrderedDict([
    ("bias", dict(bias=True)),
    ("none", dict()),
    ("bias_res", dict(bias=True, res=True)),
    ("bb_res_gate_quick", dict(bias=True, bias_b=True, res=True, colscale=True, act=ACT_QUICKGELU)),
    ("silu_gate", dict(bias=True, act=ACT_SILU, colscale=True)),
    ("gelu_res", dict(bias=True, act=ACT_GELU, res=True)),
    ("bb", dict(bias_b=True)),
])


def dense_epilogue_runs(M, fixture):
    """(epilogue name, rows_per_batch) of every launch a dense (case, fixture, layout, prec) makes: the exact fixture runs bare (an fp32
    addend would round), the others every entry of EPILOGUES, the per-view bias at every rows_per_batch."""
    if fixture == "geometry":
        return [("none", 0)]
    return [(name, rpb) for name, e in EPILOGUES.items() for rpb in (rows_per_batch_list(M) if e.get("bias_b") else [0])]


def conv_runs(c, fixture):
    """(bias, res, layout) of the launches of a convolution (case, fixture, prec); the four-tap form takes no residual (the header refuses it)."""
    if fixture == "geometry":
        return [(False, False, "packed")]
    return [(True, False, "packed")] if c.kind == "up4" else [(True, True, "window"), (True, False, "packed")]


# ------------------------------------------------------------------------------------------------ small helpers
def _f64(t):
    return t.detach().double().cpu()


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def round_op(x, fmt):
    """rn16(x): the hi plane of an operand (fp32 -> fp16 / bf16, round to nearest even) as fp32."""
    return x.float().to(torch.float16 if fmt == "f16" else torch.bfloat16).float()


def split_op(x, fmt):
    """(hi, lo) of csrc/common.hpp: split_op16, as fp32 tensors."""
    x = x.float()
    hi = round_op(x, fmt)
    return hi, round_op(x - hi, fmt)


def pack_scale(w):
    """hip._pack_scale: the power of two that brings max|w| to [1024, 2048)."""
    mx = float(w.abs().max())
    if not (mx > 0.0) or not math.isfinite(mx):
        return 1.0
    return 2.0 ** (10 - math.floor(math.log2(mx)))


def gelu(z):
    return z * 0.5 * torch.special.erfc(-z / math.sqrt(2.0))


def act_f64(z, act):
    if act == ACT_GELU:
        return gelu(z)
    if act == ACT_SILU:
        return z / (1.0 + torch.exp(-z))
    if act == ACT_QUICKGELU:
        return z / (1.0 + torch.exp(-1.702 * z))
    return z


def _junk(shape, *key):
    return (torch.randint(0, 2, shape, generator=_gen("junk", *key)).float() * 2.0 - 1.0) * JUNK


# ------------------------------------------------------------------------------------------------ fixtures
def _grade(n, mod):
    return torch.pow(2.0, -(torch.arange(n) % mod).float())


@functools.lru_cache(maxsize=None)
def dense_fixture(name, M, N, K):
    """-> dict of fp32 tensors: A (M, K), W (N, K), bias (N), bias_b (M, N) (row r serves rows_per_batch rows), res (M, N), colscale (N)."""
    g = _gen("dense", name, M, N, K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    fx = dict(bias=torch.randn(N, generator=g), bias_b=torch.randn(M, N, generator=g), res=torch.randn(M, N, generator=g),
              colscale=torch.randn(N, generator=g))
    if name == "graded":
        gm, gn = _grade(M, 11), _grade(N, 13)
        A, W = A * gm[:, None], W * gn[:, None]
        fx["bias"] = fx["bias"] * gn * gm.min()
        fx["bias_b"] = fx["bias_b"] * gn[None, :] * gm.min()
        fx["res"] = fx["res"] * gm[:, None] * gn[None, :]
    elif name == "cancel":
        A = A.abs() + 3.0
        W = W.abs() * (1.0 - 2.0 * (torch.arange(K) % 2).float())[None, :]
    elif name == "geometry":
        A = torch.randint(-255, 256, (M, K), generator=g).float()
        pi = torch.randperm(K, generator=g)[torch.arange(N) % K]
        W = torch.zeros(N, K)
        W[torch.arange(N), pi] = 1.0
        fx["pi"] = pi
    else:
        assert name == "plain", name
    fx.update(A=A.contiguous(), W=W.contiguous())
    return fx


def dense_layout(fx, layout, M, N, K):
    """The buffers a run hands to the kernel (fp32; the A buffer is what the test converts to split planes): A_buf with a_col0, lda and
    SPARE_A_ROWS rows of +-3e4 behind M; res_buf (M + 4 rows, pitch ldr), bias_b_buf (M + 1 rows, pitch ldbb), and the out pitch ldo."""
    win = layout == "window"
    col0 = 32 if win else 0
    lda = K + 64 if win else K
    A_buf = _junk((M + SPARE_A_ROWS, lda), "A", M, N, K)
    A_buf[:M, col0:col0 + K] = fx["A"]
    ldr, ldo, ldbb = (N + 4, N + 8, N + 12) if win else (N, N, N)
    res_buf = _junk((M + 4, ldr), "res", M, N, K)
    res_buf[:M, :N] = fx["res"]
    bb_buf = _junk((M + 1, ldbb), "bb", M, N, K)
    bb_buf[:M, :N] = fx["bias_b"]
    return dict(A_buf=A_buf, a_col0=col0, lda=lda, res_buf=res_buf, ldr=ldr, bias_b_buf=bb_buf, ldbb=ldbb, ldo=ldo)


@functools.lru_cache(maxsize=None)
def conv_fixture(name, c):
    """-> x (B, Hin, Win, Cin) fp32 NHWC, w (Cout, Cin, 3, 3), bias (Cout), res (M, Cout); with a tail: x2 (M, tail), wt (Cout, tail)."""
    g = _gen("conv", name, tuple(c))
    M = conv_M(c)
    x = torch.randn(c.B, c.Hin, c.Win, c.Cin, generator=g)
    w = torch.randn(c.Cout, c.Cin, 3, 3, generator=g) / math.sqrt(9 * c.Cin)
    bias, res = torch.randn(c.Cout, generator=g), torch.randn(M, c.Cout, generator=g)
    x2 = torch.randn(M, c.tail, generator=g) if c.tail else None
    wt = torch.randn(c.Cout, c.tail, generator=g) / math.sqrt(9 * c.Cin) if c.tail else None
    if name == "graded":
        gp, gn, go = _grade(c.B * c.Hin * c.Win, 11), _grade(c.Cout, 13), _grade(M, 11)
        x = x * gp.view(c.B, c.Hin, c.Win, 1)
        w = w * gn.view(-1, 1, 1, 1)
        bias, res = bias * gn * gp.min(), res * go[:, None] * gn[None, :]
        if c.tail:
            x2, wt = x2 * go[:, None], wt * gn[:, None]
    elif name == "cancel":
        x = x.abs() + 3.0
        sign = 1.0 - 2.0 * (torch.arange(c.Cin) % 2).float()
        w = w.abs() * sign.view(1, -1, 1, 1)
        if c.tail:
            x2, wt = x2.abs() + 3.0, wt.abs() * (1.0 - 2.0 * (torch.arange(c.tail) % 2).float())[None, :]
    elif name == "geometry":
        x = torch.full((c.B, c.Hin, c.Win, c.Cin), 77.0)
        x[..., 0] = (torch.arange(c.Hin).float() + 1.0).view(1, -1, 1)
        x[..., 1] = (torch.arange(c.Win).float() + 1.0).view(1, 1, -1)
        x[..., 2] = (torch.arange(c.B).float() + 1.0).view(-1, 1, 1)
        w = torch.zeros(c.Cout, c.Cin, 3, 3)
        for n in range(min(c.Cout, 27)):
            tap, j = divmod(n, 3)
            w[n, j, tap // 3, tap % 3] = 1.0
        if c.tail:
            m = torch.arange(M)
            x2 = torch.full((M, c.tail), 5.0)
            x2[:, 0], x2[:, 1] = (m % 251).float() + 1.0, (m % 13).float() + 1.0
            wt = torch.zeros(c.Cout, c.tail)
            for n in range(27, c.Cout):
                wt[n, (n - 27) % 3] = 1.0
    else:
        assert name == "plain", name
    return dict(x=x.contiguous(), w=w.contiguous(), bias=bias, res=res, x2=x2, wt=wt)


def conv_geometry_expected(c):
    """What the docstring of the geometry fixture says, written as plain loops over (b, oy, ox, channel): (M, Cout) float64."""
    M = conv_M(c)
    out = torch.zeros(M, c.Cout, dtype=torch.float64)
    for b in range(c.B):
        for oy in range(c.Hout):
            for ox in range(c.Wout):
                m = (b * c.Hout + oy) * c.Wout + ox
                for n in range(min(c.Cout, 27)):
                    tap, j = divmod(n, 3)
                    ky, kx = divmod(tap, 3)
                    if c.upsample:
                        uy, ux = oy + ky - 1, ox + kx - 1
                        inside = 0 <= uy < 2 * c.Hin and 0 <= ux < 2 * c.Win
                        iy, ix = uy // 2, ux // 2
                    else:
                        off = 0 if c.no_pad_tl else 1
                        iy, ix = oy * c.stride + ky - off, ox * c.stride + kx - off
                        inside = 0 <= iy < c.Hin and 0 <= ix < c.Win
                    if inside:
                        out[m, n] = (iy + 1, ix + 1, b + 1)[j]
                if c.tail:
                    for n in range(27, c.Cout):
                        out[m, n] = ((m % 251) + 1, (m % 13) + 1, 5)[(n - 27) % 3]
    return out


# ------------------------------------------------------------------------------------------------ bars
def e_op(fmt, prec, composed=False):
    u = 2.0 ** -11 if fmt == "f16" else 2.0 ** -8
    e = u if prec == 1 else u * u
    total = 2.0 * e + e * e
    if prec == 3:
        total += u * u
    if composed:
        total += U24
    return total


def n_products(prec):
    return {4: 4, 3: 3, 1: 1}[prec]


def e_acc(prec, nk, splits=1, act=ACT_NONE):
    """fp32 roundings on the longest chain, in units of 2^-24 (derivation: module docstring)."""
    return MFMA_ROUNDINGS * n_products(prec) * nk + max(splits - 1, 0) + 5 + (ACT_ROUNDINGS if act else 0)


def bar(t, fmt, prec, nk, splits=1, act=ACT_NONE, composed=False, planes_out=False, PL=0.0):
    """t: the dict of *_terms -> the per-element absolute bar (float64, shape of ref)."""
    b = (e_op(fmt, prec, composed) + e_acc(prec, nk, splits, act) * U24) * t["S"]
    if fmt == "f16":
        b = b + 2.0 ** -25 * t["F"]
    if planes_out:
        b = b + PL * t["ref"].abs() + (U24 if fmt == "f16" else 0.0)
    return b


def worst(got, ref, b):
    """max over the elements of |got - ref| / bar; a non-finite value counts as infinite; a bar of 0 demands the exact value."""
    err = (_f64(got) - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    r = torch.where(err == 0.0, torch.zeros_like(err), err / b.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------ dense oracle
def dense_terms(A, W, *, bias=None, bias_b=None, rows_per_batch=0, act=ACT_NONE, colscale=None, res=None, acc_scale=1.0, scale=None,
                geglu=False, splits=1, mutant=None, fmt="f16", layout=None, tile_m=64):
    """out[m, n] = res[m, n] + colscale[n] * act(acc_scale * sum_k A[m, k] W[n, k] + bias[n] + bias_b[m // rows_per_batch, n])  (MVD_EPI_STORE) or,
    geglu, out[m, j] = (acc_v + bias[j]) * gelu(acc_g + bias[N / 2 + j]) with value rows [0, N / 2) and gate rows [N / 2, N) of W  (MVD_EPI_GEGLU).
    A (M, K), W (N, K): the fp32 tensors the kernel gets; scale: the pack scale of W (None: from max|W|; 1 for an activation operand).
    layout (dense_layout): A, res and bias_b are read THROUGH the buffers and pitches (A / res / bias_b arguments are then ignored except
    as switches).  splits: the split count requested (only the split mutant looks at it).  -> dict(ref, S, F), float64."""
    if layout is not None and layout["A_buf"] is not None:
        M, K = A.shape
        c0 = layout["a_col0"] + (32 if mutant == "window_off_by_32_columns" and layout["lda"] > K else 0)
        A = layout["A_buf"][:M, c0:c0 + K]
    M, K = A.shape
    N = W.shape[0]
    scale = pack_scale(W) if scale is None else scale
    if mutant == "a_hi_only":
        A = round_op(A, fmt)
    if mutant == "w_hi_only":
        W = round_op(W * scale, fmt) / scale
    A, W = _f64(A), _f64(W)
    if mutant == "acc_scale_ignored":
        acc_scale = 1.0
    Ak, Wk = A, W
    if mutant == "drop_last_ktile":
        Ak, Wk = A[:, :max(K - 32, 0)], W[:, :max(K - 32, 0)]
    acc = Ak @ Wk.t()
    if mutant == "short_last_split_reads_stale_slab" and splits > 1:
        nk = (K + 31) // 32
        sp = min(splits, nk)
        kps = -(-nk // sp)
        extra = kps * (-(-nk // kps)) - nk          # k-tiles the short last slice runs past the end of K: it meets k-tile 0's operands again
        if extra > 0:
            acc = acc + extra * (A[:, :32] @ W[:, :32].t())
    acc = acc * acc_scale
    S = (A.abs() @ W.abs().t()) * abs(acc_scale)
    F = (W.abs().sum(1)[None, :] + A.abs().sum(1)[:, None] / scale) * abs(acc_scale)
    if bias is not None:
        acc, S = acc + _f64(bias)[None, :], S + _f64(bias).abs()[None, :]
    if geglu:
        h = N // 2
        v, gt, Sv, Sg, Fv, Fg = acc[:, :h], acc[:, h:], S[:, :h], S[:, h:], F[:, :h], F[:, h:]
        if mutant == "geglu_halves_swapped":
            v, gt = gt, v
        gg = gelu(gt)
        return dict(ref=v * gg, S=Sv * gg.abs() + v.abs() * ACT_LIP * Sg + 2.0 ** -6 * Sv * ACT_LIP * Sg, F=Fv * gg.abs() + v.abs() * ACT_LIP * Fg)
    if bias_b is not None:
        rows = torch.arange(M)
        if mutant == "bias_b_row_from_tile_base":
            rows = rows // tile_m * tile_m
        rows = rows // rows_per_batch
        if layout is not None:
            bb = layout["bias_b_buf"].reshape(-1)[(rows[:, None] * layout["ldbb"] + torch.arange(N)[None, :])]
        else:
            bb = bias_b[rows]
        acc, S = acc + _f64(bb), S + _f64(bb).abs()
    if act:
        if mutant == "colscale_inside_act" and colscale is not None:
            acc = act_f64(acc * _f64(colscale)[None, :], act)
            colscale = None
        else:
            acc = act_f64(acc, act)
        S, F = S * ACT_LIP, F * ACT_LIP
    if colscale is not None:
        cs = _f64(colscale)[None, :]
        acc, S, F = acc * cs, S * cs.abs(), F * cs.abs()
    if res is not None:
        if layout is not None:
            ldr = layout["ldo"] if mutant == "res_pitch_is_ldo" else layout["ldr"]
            flat = layout["res_buf"].reshape(-1)
            idx = (torch.arange(M)[:, None] * ldr + torch.arange(N)[None, :]) % flat.numel()
            r = _f64(flat[idx])
        else:
            r = _f64(res)
        acc, S = acc + r, S + r.abs()
    return dict(ref=acc, S=S, F=F)


def dense_ref(A, W, **kw):
    t = dense_terms(A, W, **kw)
    return t["ref"], t["S"]


def epilogue_args(fx, epi, rows_per_batch=0):
    """The keyword arguments of dense_terms for one entry of EPILOGUES."""
    kw = dict(act=epi.get("act", ACT_NONE))
    if epi.get("bias"):
        kw["bias"] = fx["bias"]
    if epi.get("bias_b"):
        kw["bias_b"], kw["rows_per_batch"] = fx["bias_b"], rows_per_batch
    if epi.get("colscale"):
        kw["colscale"] = fx["colscale"]
    if epi.get("res"):
        kw["res"] = fx["res"]
    return kw


# ------------------------------------------------------------------------------------------------ convolution oracle
def conv_taps(c, mutant=None):
    """The gather table of a nine-tap convolution: (M, 9) int64, the pixel row (b * Hin + iy) * Win + ix of the NHWC input that tap ky * 3 + kx
    of output pixel m = (b * Hout + oy) * Wout + ox reads, -1 in the zero padding.  pad 1 (no_pad_tl: none on the top / left edge, zeros past
    the bottom / right); upsample: the input is nearest-2x upsampled first, the padding is that of the UPSAMPLED image."""
    M = conv_M(c)
    tab = torch.full((M, 9), -1, dtype=torch.int64)
    for b in range(c.B):
        for oy in range(c.Hout):
            for ox in range(c.Wout):
                m = (b * c.Hout + oy) * c.Wout + ox
                if mutant == "swap_h_w":          # the m -> (oy, ox) split divides by the height
                    rem = oy * c.Wout + ox
                    oy_, ox_ = rem // c.Hout, rem % c.Hout
                else:
                    oy_, ox_ = oy, ox
                for ky in range(3):
                    for kx in range(3):
                        if c.upsample:
                            uy, ux = oy_ + ky - 1, ox_ + kx - 1
                            if mutant == "upsample_halves_before_bounds":      # halves first (C division: -1 / 2 == 0), then tests the low-resolution bounds
                                iy, ix = int(uy / 2), int(ux / 2)
                                inside = 0 <= iy < c.Hin and 0 <= ix < c.Win
                            else:
                                inside = 0 <= uy < c.Hout and 0 <= ux < c.Wout
                                iy, ix = uy >> 1, ux >> 1
                        else:
                            off = 0 if (c.no_pad_tl and mutant != "no_pad_tl_ignored") else 1
                            if mutant == "stride_tap_origin_0" and c.stride == 2:
                                off = 0
                            iy, ix = oy_ * c.stride + ky - off, ox_ * c.stride + kx - off
                            if mutant == "patch_row_pitch_w" and c.stride == 1 and not c.no_pad_tl:
                                # the halo patch (Hin + 2) x (Win + 2) addressed with a row pitch of Win: slot (oy + ky) * Win + ox + kx
                                slot = (oy_ + ky) * c.Win + ox_ + kx
                                iy, ix = slot // (c.Win + 2) - 1, slot % (c.Win + 2) - 1
                            inside = 0 <= iy < c.Hin and 0 <= ix < c.Win
                            if mutant == "image_boundary_leaks":               # the row test on the flattened (image, row) index
                                inside = 0 <= b * c.Hin + iy < c.B * c.Hin and 0 <= ix < c.Win
                        if inside:
                            tab[m, ky * 3 + kx] = (b * c.Hin + iy) * c.Win + ix
    return tab


def up4_taps(c, mutant=None):
    """Four-tap form (mvd_gemm_desc.tap_mode MVD_TAPS_UP4): for parity par = 2a + c and low-resolution pixel mq = (b, i, j): tap dy * 2 + dx
    reads row i - 1 + a + dy, column j - 1 + c + dx; the result is row (b, 2i + a, 2j + c) of the output.  -> (src (4, Mq, 4), out_row (4, Mq))."""
    Mq = c.B * c.Hin * c.Win
    src = torch.full((4, Mq, 4), -1, dtype=torch.int64)
    row = torch.zeros(4, Mq, dtype=torch.int64)
    for par in range(4):
        a, cc = par >> 1, par & 1
        if mutant == "up4_parity_swapped":
            a, cc = cc, a
        for b in range(c.B):
            for i in range(c.Hin):
                for j in range(c.Win):
                    mq = (b * c.Hin + i) * c.Win + j
                    row[par, mq] = (b * c.Hout + 2 * i + (par >> 1)) * c.Wout + 2 * j + (par & 1)
                    for dy in range(2):
                        for dx in range(2):
                            iy, ix = i - 1 + a + dy, j - 1 + cc + dx
                            if 0 <= iy < c.Hin and 0 <= ix < c.Win:
                                src[par, mq, dy * 2 + dx] = (b * c.Hin + iy) * c.Win + ix
    return src, row


def up4_weights(w, rounded=True):
    """(4, Cout, Cin, 4) float64: the 3x3 taps that land on one low-resolution pixel, summed -- row weights a = 0: w[0], w[1] + w[2];
    a = 1: w[0] + w[1], w[2]; columns alike (include/mvd_hip.h: MVD_TAPS_UP4) -- rounded once to fp32 as the packer does (rounded=False: the exact sums)."""
    w = _f64(w)
    groups = (((0,), (1, 2)), ((0, 1), (2,)))
    out = torch.zeros(4, w.shape[0], w.shape[1], 4, dtype=torch.float64)
    for a in range(2):
        for cc in range(2):
            for dy in range(2):
                for dx in range(2):
                    for ky in groups[a][dy]:
                        for kx in groups[cc][dx]:
                            out[2 * a + cc, :, :, dy * 2 + dx] += w[:, :, ky, kx]
    return out.float().double() if rounded else out


def gather_cols(x_rows, tab):
    """x_rows (pixels, C), tab (M, T) -> (M, T, C): the gathered taps, zeros where tab is -1."""
    g = x_rows[tab.clamp_min(0)]
    return g * (tab >= 0).to(g.dtype)[..., None]


def k_order(cols):
    """(M, T, C) -> (M, T * C) in the packed K order ((c / 32) * T + tap) * 32 + c % 32: the taps of one 32-channel block are consecutive k-tiles."""
    M, T, C = cols.shape
    return cols.reshape(M, T, C // 32, 32).permute(0, 2, 1, 3).reshape(M, T * C)


def conv_operands(fx, c, mutant=None, rounded=True):
    """The convolution as the matrix product the kernel runs: (cols (M, K), wmat (Cout, K)) fp32 in packed K order; a tail's columns behind.
    Four-tap form: lists of four (cols, wmat) and the output rows."""
    x_rows = fx["x"].reshape(-1, c.Cin)
    if c.kind == "up4":
        src, row = up4_taps(c, mutant)
        wq = up4_weights(fx["w"], rounded)
        wq = wq.float() if rounded else wq
        return [(k_order(gather_cols(x_rows, src[p])), k_order(wq[p].permute(0, 2, 1).contiguous())) for p in range(4)], row
    cols = k_order(gather_cols(x_rows, conv_taps(c, mutant)))
    wmat = k_order(fx["w"].reshape(c.Cout, c.Cin, 9).permute(0, 2, 1).contiguous())
    if c.tail:
        x2 = fx["x2"]
        if mutant == "tail_reads_tap_0":          # the tail operand read at the pixel of tap 0 (oy - 1, ox - 1) instead of the centre
            t0 = conv_taps(c)[:, 0:1]
            x2 = gather_cols(x2, t0)[:, 0, :]
        cols, wmat = torch.cat([cols, x2], 1), torch.cat([wmat, fx["wt"]], 1)
    return cols, wmat


def conv_scale(fx, c):
    if c.kind == "up4":
        return pack_scale(up4_weights(fx["w"]))
    return min(pack_scale(fx["w"]), pack_scale(fx["wt"])) if c.tail else pack_scale(fx["w"])


def conv_terms(fx, c, *, bias=True, res=False, act=ACT_NONE, mutant=None, fmt="f16", splits=1, layout=None, rounded=True):
    """3x3 convolution (stride, upsample, no_pad_tl, centre-tap tail, four-tap form) + the store epilogue -> dict(ref, S, F) (M, Cout)."""
    kw = dict(bias=fx["bias"] if bias else None, act=act, mutant=mutant, fmt=fmt, splits=splits, scale=conv_scale(fx, c))
    if c.kind == "up4":
        assert not res
        parts, row = conv_operands(fx, c, mutant, rounded)
        M = conv_M(c)
        out = {k: torch.zeros(M, c.Cout, dtype=torch.float64) for k in ("ref", "S", "F")}
        for p in range(4):
            t = dense_terms(parts[p][0], parts[p][1], **kw)
            for k in out:
                out[k][row[p]] = t[k]
        return out
    cols, wmat = conv_operands(fx, c, mutant)
    return dense_terms(cols, wmat, res=fx["res"] if res else None, layout=layout, **kw)


def conv_ref(fx, c, **kw):
    t = conv_terms(fx, c, **kw)
    return t["ref"], t["S"]


def conv_res_layout(fx, c, layout):
    """res / out pitches of a convolution run: window -> Cout + 4, Cout + 8 (A is the image: no column window)."""
    M, N = conv_M(c), c.Cout
    ldr, ldo = (N + 4, N + 8) if layout == "window" else (N, (N + 3) // 4 * 4)
    res_buf = _junk((M + 4, ldr), "cres", tuple(c))
    res_buf[:M, :N] = fx["res"]
    return dict(a_col0=0, lda=0, A_buf=None, res_buf=res_buf, ldr=ldr, ldo=ldo)


# ------------------------------------------------------------------------------------------------ backward oracles
def linear_backward_ref(x, w, dy):
    """y = x W^T + b: dx = dy W, dW = dy^T x, db = sum_m dy -- each with its S.  x (M, K), w (N, K), dy (M, N)."""
    x, w, dy = _f64(x), _f64(w), _f64(dy)
    return dict(dx=(dy @ w, dy.abs() @ w.abs()), dW=(dy.t() @ x, dy.abs().t() @ x.abs()), db=(dy.sum(0), dy.abs().sum(0)))


def conv3x3_backward_ref(x, w, dy, B, H, W):
    """y = conv3x3(x), stride 1, pad 1, channels-last.  x (B, H, W, Cin), w (Cout, Cin, 3, 3), dy (B*H*W, Cout).  With the gather table T of
    the forward (y[m] = sum_tap x[T[m, tap]] w[:, :, tap]):  dW[:, :, tap] = sum_m dy[m]^T x[T[m, tap]],  dx[p] = sum_{(m, tap): T[m, tap] = p}
    dy[m] w[:, :, tap],  db = sum_m dy."""
    Cout, Cin = w.shape[0], w.shape[1]
    c = _cc("s1", B, H, W, Cin, Cout)
    tab = conv_taps(c)
    x_rows, w9, dy = _f64(x).reshape(-1, Cin), _f64(w).reshape(Cout, Cin, 9), _f64(dy)
    cols = gather_cols(x_rows, tab)                                   # (M, 9, Cin)
    dW = torch.einsum("mo,mtc->oct", dy, cols)
    dW_S = torch.einsum("mo,mtc->oct", dy.abs(), cols.abs())
    dx = torch.zeros_like(x_rows)
    dx_S = torch.zeros_like(x_rows)
    for tap in range(9):
        ok = tab[:, tap] >= 0
        dx.index_add_(0, tab[ok, tap], dy[ok] @ w9[:, :, tap])
        dx_S.index_add_(0, tab[ok, tap], dy[ok].abs() @ w9[:, :, tap].abs())
    return dict(dx=(dx, dx_S), dW=(dW.reshape(Cout, Cin, 3, 3), dW_S.reshape(Cout, Cin, 3, 3)), db=(dy.sum(0), dy.abs().sum(0)))


# ------------------------------------------------------------------------------------------------ packed weight images
def _op_bits_to_float(bits, fmt):
    bits = bits.to(torch.int16)
    if fmt == "bf16":
        return (bits.to(torch.int32) << 16).view(torch.float32)
    return bits.view(torch.float16).float()


def _float_to_op_bits(x, fmt):
    if fmt == "bf16":
        return x.float().to(torch.bfloat16).view(torch.int16)
    return x.float().to(torch.float16).view(torch.int16)


def packed_index(n, k, Np, mutant=None):
    """Position (in 16-bit words) of element (n, k) of the hi image; the lo image is 512 words behind.  include/mvd_hip.h, "Weight packing":
    [K / 32][N / 16] micro-tiles of 2 KiB = [hi image | lo image]; inside a 1 KiB image lane l = (n & 15) + 16 * ((k & 31) >> 3) owns the 8
    elements k & 7 = 0..7 at byte 16 l."""
    mt = (k // 32) * (Np // 16) + n // 16
    lane = (n & 15) + 16 * ((k & 31) >> 3)
    if mutant == "packed_lane_order_n_major":
        lane = (n & 15) * 4 + ((k & 31) >> 3)
    return mt * 1024 + lane * 8 + (k & 7)


def _index_grid(Np, Kp, mutant=None):
    n = torch.arange(Np)[:, None].expand(Np, Kp)
    k = torch.arange(Kp)[None, :].expand(Np, Kp)
    return packed_index(n, k, Np, mutant)


def decode_packed(words, N, K, fmt, mutant=None):
    """words: the packed image as int16 (mvd_packed_weight_bytes / 2 of them) -> (hi, lo) fp32 (Np, Kp), Np = ceil16(N), Kp = ceil32(K)."""
    Np, Kp = (N + 15) // 16 * 16, (K + 31) // 32 * 32
    words = words.cpu().view(torch.int16).reshape(-1)
    assert words.numel() == 2 * Np * Kp, (words.numel(), Np, Kp)
    idx = _index_grid(Np, Kp, mutant)
    return _op_bits_to_float(words[idx], fmt), _op_bits_to_float(words[idx + 512], fmt)


def conv_k_index(ci, tap):
    """Packed K index of input channel ci at tap ky * 3 + kx: ((ci / 32) * 9 + tap) * 32 + ci % 32."""
    return ((ci // 32) * 9 + tap) * 32 + ci % 32


def conv_weight_matrix(w, cin_pad):
    """(Cout, Cin, 3, 3) -> the (Cout, 9 * cin_pad) matrix whose packed image mvd_pack_conv3x3_weight writes (zeros in the padded channels)."""
    Cout, Cin = w.shape[0], w.shape[1]
    m = torch.zeros(Cout, 9 * cin_pad, dtype=w.dtype)
    for ci in range(Cin):
        for tap in range(9):
            m[:, conv_k_index(ci, tap)] = w[:, ci, tap // 3, tap % 3]
    return m


def pack_numpy(w, fmt, scale):
    """The packer written from the header text, element by element: w (N, K) fp32 -> int16 words of the image (zero padded)."""
    import numpy as np
    N, K = w.shape
    Np, Kp = (N + 15) // 16 * 16, (K + 31) // 32 * 32
    hi, lo = split_op(w * scale, fmt)
    hb, lb = _float_to_op_bits(hi, fmt).numpy(), _float_to_op_bits(lo, fmt).numpy()
    out = np.zeros(2 * Np * Kp, dtype=np.int16)
    for n in range(N):
        for k in range(K):
            p = int(packed_index(n, k, Np))
            out[p], out[p + 512] = hb[n, k], lb[n, k]
    return torch.from_numpy(out)


def pack_bar(w, scale, fmt):
    """|hi + lo - w * scale| per element: the operand contract -- 2^-22 (fp16) / 2^-16 (bf16) relative, fp16: 2^-25 absolute below the normal range."""
    ws = _f64(w).abs() * scale
    return ws * (2.0 ** -22 if fmt == "f16" else 2.0 ** -16) + (2.0 ** -25 if fmt == "f16" else 0.0)


# ------------------------------------------------------------------------------------------------ fp32 emulation of the algorithm
def emulate(A, W, fmt, prec, *, scale=None, acc_scale=1.0, splits=1, bias=None, bias_b_rows=None, act=ACT_NONE, colscale=None, res=None,
            split_w=True):
    """The split-operand product as the kernels run it, in fp32 on the CPU: operands hi / lo in the flavour's type (weights times the pack
    scale first; split_w False: W is an activation operand), per k-tile of 32 the partial products lo*lo, lo*hi, hi*lo, hi*hi (x3: without
    lo*lo; x1: hi*hi) each added to the fp32 accumulator with ONE rounding, k-tiles in order, the slabs of a split summed in slice order,
    then the epilogue in fp32.  A (M, K), W (N, K), K % 32 == 0; bias_b_rows: the (M, N) per-row values.  -> (M, N) fp32."""
    M, K = A.shape
    assert K % 32 == 0
    scale = (pack_scale(W) if scale is None else scale) if split_w else 1.0
    ah, al = split_op(A, fmt)
    wh, wl = split_op(W * scale, fmt)
    terms = {4: ((al, wl), (al, wh), (ah, wl), (ah, wh)), 3: ((al, wh), (ah, wl), (ah, wh)), 1: ((ah, wh),)}[prec]
    nk = K // 32
    sp = max(1, min(splits, nk))
    kps = -(-nk // sp)
    total = None
    for s0 in range(0, nk, kps):
        acc = torch.zeros(M, W.shape[0], dtype=torch.float32)
        for kt in range(s0, min(s0 + kps, nk)):
            ks = slice(32 * kt, 32 * kt + 32)
            for a, w in terms:
                acc = (acc.double() + a[:, ks].double() @ w[:, ks].double().t()).float()
        total = acc if total is None else total + acc
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    z = total * f(acc_scale / scale if split_w else acc_scale)
    if bias is not None:
        z = z + bias.float()[None, :]
    if bias_b_rows is not None:
        z = z + bias_b_rows.float()
    if act:
        z = act_f64(z, act).float() if act != ACT_GELU else (z * 0.5 * (1.0 + torch.erf(z * f(1.0 / math.sqrt(2.0))))).float()
    if colscale is not None:
        z = z * colscale.float()[None, :]
    if res is not None:
        z = z + res.float()
    return z


def emulate_geglu(A, W, fmt, prec, bias, splits=1):
    h = emulate(A, W, fmt, prec, splits=splits, bias=bias)
    n = W.shape[0] // 2
    g = h[:, n:]
    return h[:, :n] * (g * 0.5 * (1.0 + torch.erf(g * torch.tensor(1.0 / math.sqrt(2.0)))))
