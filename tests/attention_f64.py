"""FLOAT64 statements of the attention family of include/mvd_hip.h, the fixtures the GPU tests feed to it and the acceptance rule they
apply (tests/test_gpu_attention_f64.py; tests/test_cpu_attention_f64.py proves on the CPU that fixtures and rule have teeth).

  self_attention        : mvd_attention.  Per (batch, head):  softmax(q k^T / sqrt(dhead)) v  over the keys [0, Lkeys) of the sequence;
                          token-major (B*L, heads*dhead) rows, head-major channels.
  pixel_cross_attention : mvd_pixel_cross_attn.  One query token per pixel against its own D context tokens.
  view_mha              : mvd_view_mha.  timm Attention core over the V rows of a sequence, qkv rows laid out [3][heads][dhead].
  view_pool             : mvd_view_pool.  logits w.x_v + b, softmax over the V rows, weighted sum of the rows.

Every oracle returns (out, scale): scale is max|v| over the values that take part, per GROUP -- (batch, head) for self-attention, the
pixel or sequence for the others.  accept() divides a group's largest error by tol * scale of that group: the project's existing bars
(tests/test_gpu_ops.py: 2 TOL[prec] + PL for mvd_attention, PL + 2e-6 for the fp32 kernels), applied per group instead of against the
largest magnitude of the whole tensor, where a wrong head or a wrong row of small magnitude can hide.

Fixtures (seeded, fp32 tensors; the oracles read exactly these values):
  diffuse   : q, k, v ~ 1.5 N(0, 1) as in tests/test_gpu_ops.py -- every key contributes to every query.
  one_hot   : unit-norm keys, q_i = 24 sqrt(d) k_pi(i) + 0.3 N(0, 1) with pi = perm[arange(L) % Lk]: the logit of key pi(i) leads by
              about 24 (1 - cos) nats, so out_i = v_pi(i) and every key slot of every 64-key tile is the answer of some query: a wrong
              key slot, tile or head costs O(|v|).  The masked keys [Lk, L) are COPIES of keys that win (with other values): letting
              one of them in halves the winner's weight.
  sentinel  : small logits (q, k ~ 0.5 N(0, 1)) and values of about +-3e4 (the top of the fp16 range) in the masked rows [Lk, L): one
              masked key that takes part moves every query by ~ 3e4 / Lk.
  large     : the fp32 kernels only.  All keys of a group are multiples a_j u of one unit vector, the query is +-sqrt(d) u: the logits
              are +-a_j with a_j spread over [-250, 250] in steps of >= 30 -- one key wins by >= 30 nats (so the rounding of a logit
              cannot show) and logits beyond +-100 overflow an fp32 exp that forgot to subtract the maximum.
"""
import functools
import math
import zlib

import torch

ONE_HOT_LEAD = 24.0
SENTINEL_VALUE = 3.0e4
LARGE_SPAN = 250.0

# B, heads, L, Lkeys (0 = L), dhead[, True: also in the three- and one-product precisions] -- the one-tile-per-wavefront kernel
ONE_TILE_CASES = [
    (1, 8, 4, 0, 4, True),         # one query quad, one key tile, 16 padded channels (tail MFMA step only)
    (2, 8, 20, 17, 12, True),      # L < 64, partly filled last channel tile, batch stride b*L != b*Lpad
    (1, 8, 64, 1, 20, False),      # a single key
    (2, 8, 68, 64, 32, False),     # Lkeys on a tile edge with L behind it
    (2, 8, 68, 65, 36, True),      # second key tile holding one key; 48 padded channels (32 + 16)
    (1, 3, 132, 129, 32, False),   # grid of 9 workgroups: remainder branch of the XCD block order
    (1, 5, 196, 0, 32, False),     # grid of 15, three key tiles: both LDS buffers
    (2, 8, 132, 129, 52, False),   # 64 padded channels, partly filled
    (1, 8, 260, 257, 64, True),    # CLIP's shape
    (1, 1, 132, 130, 64, False),   # one head
    (2, 8, 68, 65, 68, False),     # 80 padded channels, one LDS buffer
    (1, 8, 132, 129, 80, False),
    (1, 8, 68, 66, 148, True),     # 160 padded channels, partly filled last channel tile
    (1, 3, 132, 0, 160, False),
]
# two query tiles per wavefront: ceil(Lpad / 128) * heads * B >= 512
TWO_TILE_CASES = [
    (64, 8, 20, 17, 4),            # Lpad 64 under a 128-row block: waves 2 and 3 wholly behind Lpad
    (32, 8, 132, 129, 40),         # Lpad 192
    (22, 8, 260, 257, 64),         # CLIP from 11 images upwards, Lpad 320
    (57, 3, 260, 257, 80),         # grid of 513: remainder branch; one LDS buffer
]


def dpad(d):
    return (d + 15) // 16 * 16


def lpad(L):
    return (L + 63) // 64 * 64


def fixtures_for(L, Lkeys):
    """The fixtures a self-attention case runs: the masked ones where a key limit is at work, else the diffuse one."""
    return ("one_hot", "sentinel") if 0 < Lkeys < L else ("diffuse",)


def _f64(t):
    return t.detach().double().cpu()


def _softmax(s):
    e = (s - s.amax(-1, keepdim=True)).exp()
    return e / e.sum(-1, keepdim=True)


# ------------------------------------------------------------------------------------------------ oracles
def heads_first(x, B, H, L, d):
    """token-major (B*L, H*d) -> (B, H, L, d)"""
    return x.reshape(B, L, H, d).permute(0, 2, 1, 3)


def by_head(x, B, H, L, d):
    """token-major (B*L, H*d) -> one group per (batch, head): (B*H, L, d)"""
    return heads_first(x, B, H, L, d).reshape(B * H, L, d)


def by_rows(x, groups):
    """(groups*r, C) -> (groups, r, C)"""
    return x.reshape(groups, -1, x.shape[-1])


def self_attention(q, k, v, B, H, L, d, Lkeys=0):
    """q, k, v (B*L, H*d) -> out (B*L, H*d) float64, scale (B*H,) = max|v| over the keys [0, Lkeys) of the (batch, head)."""
    Lk = Lkeys or L
    assert 0 < Lk <= L
    q, k, v = (heads_first(_f64(t), B, H, L, d) for t in (q, k, v))
    k, v = k[:, :, :Lk], v[:, :, :Lk]
    p = _softmax(q @ k.transpose(-1, -2) / math.sqrt(d))
    out = (p @ v).permute(0, 2, 1, 3).reshape(B * L, H * d)
    return out, v.abs().amax((-1, -2)).reshape(B * H)


def pixel_cross_attention(q, k, v, P, D, H, d):
    """q (P, H*d), k / v (P*D, H*d) -> out (P, H*d) float64, scale (P,) = max|v| of the pixel's context tokens."""
    q = _f64(q).reshape(P, 1, H, d).permute(0, 2, 1, 3)
    k, v = (_f64(t).reshape(P, D, H, d).permute(0, 2, 1, 3) for t in (k, v))
    p = _softmax(q @ k.transpose(-1, -2) / math.sqrt(d))
    return (p @ v).permute(0, 2, 1, 3).reshape(P, H * d), v.abs().amax((1, 2, 3))


def view_mha(qkv, Nseq, V, H, d):
    """qkv (Nseq*V, 3*H*d), row layout [3][H][d] -> out (Nseq*V, H*d) float64, scale (Nseq,) = max|v| of the sequence."""
    q, k, v = _f64(qkv).reshape(Nseq, V, 3, H, d).permute(2, 0, 3, 1, 4).unbind(0)      # (Nseq, H, V, d) each
    p = _softmax(q @ k.transpose(-1, -2) / math.sqrt(d))
    return (p @ v).permute(0, 2, 1, 3).reshape(Nseq * V, H * d), v.abs().amax((1, 2, 3))


def view_pool(x, w, b, Nseq, V, C):
    """x (Nseq*V, C), w (C,), b (1,) -> out (Nseq, C) float64, scale (Nseq,) = max|x| of the sequence."""
    x = _f64(x).reshape(Nseq, V, C)
    p = _softmax((x @ _f64(w).reshape(C) + _f64(b).reshape(())))       # (Nseq, V)
    return (p[:, :, None] * x).sum(1), x.abs().amax((1, 2))


def accept(got, ref, scale, tol):
    """got, ref (groups, ...); scale (groups,).  The worst |got - ref| / (tol * scale) of every group: a case passes while none
    exceeds 1.  A value that is not finite counts as an infinite error."""
    err = (_f64(got) - _f64(ref)).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return err.reshape(err.shape[0], -1).amax(1) / (tol * _f64(scale))


# ------------------------------------------------------------------------------------------------ self-attention fixtures
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _token_major(x):
    """(B, H, L, d) -> (B*L, H*d)"""
    B, H, L, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * L, H * d).contiguous()


def diffuse(B, H, L, d, Lkeys=0, seed=0):
    g = _gen("diffuse", B, H, L, d, seed)
    return tuple(torch.randn(B * L, H * d, generator=g) * 1.5 for _ in range(3))


def one_hot(B, H, L, d, Lkeys=0, seed=0):
    Lk = Lkeys or L
    g = _gen("one_hot", B, H, L, d, Lk, seed)
    # narrow heads: of a few draws keep, per (batch, head), the key set whose two closest keys are furthest apart (24 (1 - cos) nats lead)
    tries = 16 if d < 16 else 1
    k = torch.randn(tries, B, H, Lk, d, generator=g)
    k = k / k.norm(dim=-1, keepdim=True)
    if tries > 1:
        coh = (k @ k.transpose(-1, -2) - 2.0 * torch.eye(Lk)).amax((-1, -2))          # (tries, B, H)
        k = torch.gather(k, 0, coh.argmin(0)[None, :, :, None, None].expand(1, B, H, Lk, d))
    k = k[0]
    perm = torch.argsort(torch.rand(B, H, Lk, generator=g), dim=-1)
    pi = torch.gather(perm, -1, (torch.arange(L) % Lk).expand(B, H, L))                 # the key query i looks at
    q = ONE_HOT_LEAD * math.sqrt(d) * torch.gather(k, 2, pi[..., None].expand(B, H, L, d)) + 0.3 * torch.randn(B, H, L, d, generator=g)
    if L > Lk:     # masked keys: copies of the keys the first queries look at
        k = torch.cat([k, torch.gather(k, 2, pi[:, :, :L - Lk, None].expand(B, H, L - Lk, d))], 2)
    v = torch.randn(B, H, L, d, generator=g) * 1.5
    return _token_major(q), _token_major(k), _token_major(v)


def sentinel(B, H, L, d, Lkeys=0, seed=0):
    Lk = Lkeys or L
    g = _gen("sentinel", B, H, L, d, Lk, seed)
    q, k = (torch.randn(B, H, L, d, generator=g) * 0.5 for _ in range(2))
    v = torch.randn(B, H, L, d, generator=g) * 1.5
    sign = torch.where(torch.rand(B, H, L - Lk, d, generator=g) < 0.5, -1.0, 1.0)
    v[:, :, Lk:] = sign * SENTINEL_VALUE * (0.75 + 0.25 * torch.rand(B, H, L - Lk, d, generator=g))
    return _token_major(q), _token_major(k), _token_major(v)


FIXTURES = {"diffuse": diffuse, "one_hot": one_hot, "sentinel": sentinel}


@functools.lru_cache(maxsize=None)
def self_case(name, B, H, L, Lkeys, d):
    """(q, k, v, float64 reference, scale) of one fixture of one case -- built once, shared by the tests, never modified."""
    q, k, v = FIXTURES[name](B, H, L, d, Lkeys)
    ref, scale = self_attention(q, k, v, B, H, L, d, Lkeys)
    return q, k, v, ref, scale


# ------------------------------------------------------------------------------------------------ fixtures of the fp32 kernels
def _large_logits(groups, n, g):
    """(groups, n) logits: a permutation of n values spread over [-LARGE_SPAN, LARGE_SPAN] (n = 1: the largest alone)."""
    a = torch.linspace(-LARGE_SPAN, LARGE_SPAN, n) if n > 1 else torch.tensor([LARGE_SPAN])
    return a[torch.argsort(torch.rand(groups, n, generator=g), dim=-1)]


def _unit(shape, g):
    u = torch.randn(*shape, generator=g, dtype=torch.float64)
    return u / u.norm(dim=-1, keepdim=True)


def pixel_fixture(name, P, D, H, d, seed=0):
    """-> q (P, H*d), k, v (P*D, H*d)"""
    g = _gen("pixel", name, P, D, H, d, seed)
    C = H * d
    v = torch.randn(P * D, C, generator=g) * 1.5
    if name == "diffuse":
        return torch.randn(P, C, generator=g) * 1.5, torch.randn(P * D, C, generator=g) * 1.5, v
    u = _unit((P, 1, H, d), g)
    a = _large_logits(P * H, D, g).reshape(P, H, D).permute(0, 2, 1)                    # (P, D, H)
    s = torch.where(torch.rand(P, 1, H, 1, generator=g) < 0.5, -1.0, 1.0).double()      # -1: the SMALLEST a wins
    q = (s * math.sqrt(d) * u).reshape(P, C)
    k = (a[..., None].double() * u).reshape(P * D, C)
    return q.float(), k.float(), v


def view_mha_fixture(name, Nseq, V, H, d, seed=0):
    """-> qkv (Nseq*V, 3*H*d)"""
    g = _gen("view_mha", name, Nseq, V, H, d, seed)
    if name == "diffuse":
        return torch.randn(Nseq * V, 3 * H * d, generator=g)
    u = _unit((Nseq, 1, H, d), g)
    a = _large_logits(Nseq * H, V, g).reshape(Nseq, H, V).permute(0, 2, 1)              # (Nseq, V, H)
    s = torch.where(torch.rand(Nseq, V, H, 1, generator=g) < 0.5, -1.0, 1.0).double()   # per query view
    q = s * math.sqrt(d) * u
    k = a[..., None].double() * u
    v = torch.randn(Nseq, V, H, d, generator=g, dtype=torch.float64) * 1.5
    return torch.stack([q, k, v], 2).reshape(Nseq * V, 3 * H * d).float()


def view_pool_fixture(name, Nseq, V, C, seed=0):
    """-> x (Nseq*V, C), w (1, C), b (1,)"""
    g = _gen("view_pool", name, Nseq, V, C, seed)
    x = torch.randn(Nseq, V, C, generator=g, dtype=torch.float64)
    if name == "diffuse":
        return x.reshape(Nseq * V, C).float(), torch.randn(1, C, generator=g) * 0.2, torch.randn(1, generator=g)
    w = torch.randn(C, generator=g, dtype=torch.float64) * 0.5
    a = _large_logits(Nseq, V, g).double()
    x = x - (x @ w)[..., None] * w / (w @ w) + a[..., None] * w / (w @ w)              # w.x_v = a_v, the rest of x_v is orthogonal to w
    return x.reshape(Nseq * V, C).float(), w.reshape(1, C).float(), torch.tensor([LARGE_SPAN / 2])


# one case per value of each axis, the others at their smallest
PIXEL_CASES = [(1, 1, 8, 4), (5, 1, 8, 4), (301, 1, 8, 4), (1, 2, 8, 4), (1, 8, 8, 4), (1, 1, 8, 40), (1, 1, 1, 32), (5, 2, 2, 80),
               (5, 8, 1, 160)]                                                           # P, D, heads, dhead
VIEW_MHA_FAST_CASES = [(1, 2), (1, 3), (1, 4), (1, 8), (5, 2), (501, 2), (501, 8)]        # Nseq, V   (heads 8, dhead 32)
VIEW_MHA_GENERIC_CASES = [(5, 1, 8, 32), (5, 5, 8, 32), (5, 16, 8, 32), (5, 1, 4, 8), (5, 5, 1, 32), (5, 16, 2, 48)]      # Nseq, V, heads, dhead
VIEW_MHA_GRID_STRIDE_CASE = (4100, 16, 32, 1)         # 2 099 200 work items: one more pass than 8192 workgroups of 256 threads
VIEW_POOL_CASES = [(1, 1, 32), (1, 1, 96), (1, 1, 256), (1, 1, 512), (1, 3, 32), (1, 16, 32), (5, 1, 32), (501, 1, 32), (501, 16, 96),
                   (5, 3, 512)]                                                          # Nseq, V, C
