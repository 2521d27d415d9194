"""Float64 reference of the texture bake and lookup (mvd_texture_bake, mvd_texture_sample: include/mvd_hip.h) -- TEST INFRASTRUCTURE.

The rule of the header is written once, with torch ops on the CPU, and evaluated in a `dtype`: float64 is the reference, float32 the
"fp32 oracle" whose own error against float64 sizes the margins and the bounds -- the pattern of tests/raster_f64.py, whose Case (with
M = V and P = Pd), rigs and meshes this file reuses.  The fp32 evaluation is elementwise in the header's operation order (one rounding
per operation).  The layout (`owner`, `corners`) is written here from the header's text, independently of mvdfusion_amd/fusion.py.

The per-view part of the rule is a chain of comparisons, and float64 may sit too close to one for any fp32 evaluation to be held to
its side.  Per case, with err(q) = max|q_fp32 - q_f64| over the (texel, view) pairs of faces with usable ids and normal whose float64
zc is above znear (the rest of the chain is never reached otherwise), a pair is NEAR
  znear    |zc - znear| < MARGIN err(zc);
  pixel    cx + 0.5 or cy + 0.5 within MARGIN err(cx, cy) of an integer -- the rounding boundaries of the depth pixel, which include the
           image border at -0.5 and Pd - 0.5;
  depth    |zc - (d + tol)| < MARGIN (err(zc) + err(d + tol)), d the float64 pair's depth pixel (only where it is finite);
  cosine   |cosv - min_cos| < MARGIN err(cosv),
and a test FAILS CLEARLY when float64 fails it and the pair is not near it (the depth test also needs the pixel not to be near: another
pixel holds another depth).  A pair is AMBIGUOUS when it is near a test and fails none clearly.  The largest weight is a decision too
-- `best`, and the colour under MVD_TEX_BEST: a texel whose two largest float64 weights are less than MARGIN err(wt) apart but not equal
in both evaluations is ambiguous as well.  A texel with an ambiguous pair is left out of the value comparison; at most MAX_EXCLUDED of a
case's owned texels may be, asserted by `reference` before anything is compared.  A case over the cap gets another seed, not a larger cap.

Bounds on the kept texels: views and best EQUAL float64's; max|texture - f64| <= MARGIN max|fp32 oracle - f64| over those texels (two
fp32 evaluations of the same formulas).  Nothing is taken from the kernel.
"""
import functools
from dataclasses import dataclass
from typing import Optional

import torch

import raster_f64 as R
from gridattn_f64 import MARGIN, MAX_EXCLUDED, make_rig

MEAN, BEST = 0, 1
NEAREST, BILINEAR = 0, 1
FILL = (0.125, 0.375, 0.625)


# ------------------------------------------------------------------------------------------------ the layout, from the header's text
def cells_per_row(nface_max):
    cells = (nface_max + 1) // 2
    C = 1
    while C * C < cells:
        C += 1
    return C


def owner(i, j, T):
    """(half, chart i, chart j) of cell-local texel (i, j), or None -- plain Python, for the brute-force layout test."""
    K = T + 3
    if i <= T and j <= T and i + j <= T + 1:
        return 0, i, j
    mi, mj = K - 1 - i, K - 1 - j
    if mi <= T and mj <= T and mi + mj <= T + 1:
        return 1, mi, mj
    return None


def corners(l, T, C):
    """The texel coordinates (x, y) of the corners a, b, c of local face l."""
    K, c = T + 3, l >> 1
    ox, oy = (c % C) * K, (c // C) * K
    if l & 1:
        return (ox + K - 1, oy + K - 1), (ox + K - 1 - T, oy + K - 1), (ox + K - 1, oy + K - 1 - T)
    return (ox, oy), (ox + T, oy), (ox, oy + T)


def chart_map(T, C):
    """Per texel of the (A, A) atlas: local face l (-1: of no chart), chart indices i, j -- the tensor form of `owner`."""
    K = T + 3
    A = C * K
    y, x = torch.meshgrid(torch.arange(A), torch.arange(A), indexing="ij")
    l = torch.full((A, A), -1, dtype=torch.long)
    ci, cj = torch.zeros(A, A, dtype=torch.long), torch.zeros(A, A, dtype=torch.long)
    for yy in range(K):
        for xx in range(K):
            o = owner(xx, yy, T)
            if o is None:
                continue
            m = (x % K == xx) & (y % K == yy)
            l[m] = (2 * ((y // K) * C + x // K) + o[0])[m]
            ci[m], cj[m] = o[1], o[2]
    return l, ci, cj


# ------------------------------------------------------------------------------------------------ cases
@dataclass
class BakeCase:
    mesh: R.Case                      # vertices, colors, faces, the two start tables, cams (nscene * V), M = V, P = Pd, cull, znear
    rgb: torch.Tensor                 # (nscene * V, 3, H, H) fp32
    depth: torch.Tensor               # (nscene * V, Pd, Pd) fp32, +inf where empty
    texels: int
    tol: float = 0.05
    min_cos: float = 0.1
    power: int = 2
    blend: int = MEAN
    side: Optional[int] = None        # None: the smallest atlas

    @property
    def V(self):
        return self.mesh.M

    @property
    def H(self):
        return int(self.rgb.shape[-1])

    @property
    def Pd(self):
        return int(self.depth.shape[-1])

    @property
    def C(self):
        if self.side is not None:
            return self.side // (self.texels + 3)
        fs = self.mesh.face_start.clamp(0, self.mesh.nface)
        return cells_per_row(int((fs[1:] - fs[:-1]).max()) if self.mesh.nscene else 0)

    @property
    def A(self):
        return self.C * (self.texels + 3)


def rendered_depth(mesh):
    """The float64 rasteriser's depth of the mesh in its own cameras at P = Pd, rounded to fp32 (+inf where empty)."""
    return R.render(mesh).depth.float()


def smooth_images(n, H, g):
    """(n, 3, H, H) fp32 in [0, 1]: a few random low-frequency waves per channel -- bilinear lookups see real gradients."""
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, dtype=torch.float64), torch.linspace(0, 1, H, dtype=torch.float64), indexing="ij")
    k = torch.rand(n, 3, 3, 3, generator=g, dtype=torch.float64) * 12.0          # (image, channel, wave, (kx, ky, phase))
    img = sum(torch.sin(k[..., w, 0, None, None] * xx + k[..., w, 1, None, None] * yy + k[..., w, 2, None, None]) for w in range(3))
    return (0.5 + img / 6.0).float()


def make_bake(mesh, H, texels, g, **kw):
    return BakeCase(mesh=mesh, rgb=smooth_images(mesh.nscene * mesh.M, H, g), depth=rendered_depth(mesh), texels=texels, **kw)


def sphere_case(texels=4, H=32, **kw):
    """raster_f64's sphere_cull1 (2 616 faces, 3 views, Pd = 48) with images of H != Pd pixels."""
    mesh = R.make_case("sphere_cull1")
    return make_bake(mesh, H, texels, torch.Generator().manual_seed(7300), **kw)


# ------------------------------------------------------------------------------------------------ the rule
@dataclass
class Pairs:
    """Per owned texel (K) and view (K, V), in dtype."""
    scene: torch.Tensor               # (K,) long
    y: torch.Tensor
    x: torch.Tensor
    face: torch.Tensor                # (K,) long: the global face row
    ids_ok: torch.Tensor              # (K,) bool
    normal_ok: torch.Tensor           # (K,) bool (False where ids are not)
    fallback: torch.Tensor            # (K, 3): the colour without a contributing view
    zc: torch.Tensor                  # (K, V)
    cx: torch.Tensor
    cy: torch.Tensor
    d: torch.Tensor                   # the depth pixel's value (+inf where the pixel is outside)
    dtol: torch.Tensor                # d + tol
    cosv: torch.Tensor
    wt: torch.Tensor
    col: torch.Tensor                 # (K, V, 3)
    tests: torch.Tensor               # (K, V, 4) bool: znear and finite, pixel inside, depth, cosine -- each on its own
    contributes: torch.Tensor         # (K, V) bool


def _c(v, dtype):
    return torch.tensor(v, dtype=torch.float32).to(dtype)          # the kernel receives its scalars as C floats


def taps(u, w, S, dtype):
    """pixel_taps of fusion_common.hpp: (idx (.., 4) long, wx, wy)."""
    S2, Sm1 = 0.5 * S, float(S - 1)
    ix = ((1.0 - u) * S2 - 0.5).clamp(0.0, Sm1)
    iy = ((1.0 - w) * S2 - 0.5).clamp(0.0, Sm1)
    ix, iy = torch.nan_to_num(ix, nan=0.0), torch.nan_to_num(iy, nan=0.0)
    x0f, y0f = ix.floor(), iy.floor()
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = (x0 + 1).clamp(max=S - 1), (y0 + 1).clamp(max=S - 1)
    return torch.stack([y0 * S + x0, y0 * S + x1, y1 * S + x0, y1 * S + x1], dim=-1), ix - x0f, iy - y0f


def mix(z, wx, wy):
    """bilinear_mix of fusion_common.hpp on z (.., 4)."""
    return (z[..., 0] * (1.0 - wx) + z[..., 1] * wx) * (1.0 - wy) + (z[..., 2] * (1.0 - wx) + z[..., 3] * wx) * wy


def pairs(case, dtype=torch.float64):
    m, T, C, A, V, Pd, H = case.mesh, case.texels, case.C, case.A, case.V, case.Pd, case.H
    l, ci, cj = chart_map(T, C)
    fs = m.face_start.clamp(0, m.nface)
    vs = m.vertex_start.clamp(0, m.nvert)
    own = torch.stack([(l >= 0) & (l < fs[s + 1] - fs[s]) for s in range(m.nscene)])                 # (nscene, A, A)
    scene, y, x = torch.nonzero(own, as_tuple=True)
    face = l[y, x] + fs[scene]
    ids = m.faces[face]
    ids_ok = ((ids >= vs[scene][:, None]) & (ids < vs[scene + 1][:, None])).all(1)
    ids = torch.where(ids_ok[:, None], ids, torch.zeros_like(ids)).clamp(0, max(m.nvert - 1, 0))
    fT = float(T)
    bb, bc = ci[y, x].to(dtype) / fT, cj[y, x].to(dtype) / fT
    ba = (1.0 - bb) - bc
    P3 = m.vertices.to(dtype)[ids]                                                                  # (K, 3 vertices, 3)
    X = (ba[:, None] * P3[:, 0] + bb[:, None] * P3[:, 1]) + bc[:, None] * P3[:, 2]
    fill = torch.tensor(FILL, dtype=torch.float32).to(dtype)
    if m.colors is not None:
        c3 = m.colors.to(dtype)[ids]
        fallback = (ba[:, None] * c3[:, 0] + bb[:, None] * c3[:, 1]) + bc[:, None] * c3[:, 2]
        fallback = torch.where(ids_ok[:, None], fallback, fill.expand_as(fallback))
    else:
        fallback = fill.expand(X.shape[0], 3).clone()
    e1, e2 = P3[:, 1] - P3[:, 0], P3[:, 2] - P3[:, 0]
    n = torch.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], dim=1)
    nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    normal_ok = ids_ok & torch.isfinite(nn) & (nn > 0)
    cam = scene[:, None] * V + torch.arange(V)[None]                                                 # (K, V)
    Rm, Tv = m.cams.R.to(dtype)[cam], m.cams.T.to(dtype)[cam]
    f, p = m.cams.focal_length.to(dtype)[cam], m.cams.principal_point.to(dtype)[cam]
    Xv = X[:, None]
    xc = [Xv[..., 0] * Rm[..., 0, j] + Xv[..., 1] * Rm[..., 1, j] + Xv[..., 2] * Rm[..., 2, j] + Tv[..., j] for j in range(3)]
    zc = xc[2]
    u, w = f[..., 0] * xc[0] / zc + p[..., 0], f[..., 1] * xc[1] / zc + p[..., 1]
    t_z = (zc > _c(m.znear, dtype)) & torch.isfinite(u) & torch.isfinite(w)
    Pd2 = 0.5 * Pd
    cx, cy = (1.0 - u) * Pd2 - 0.5, (1.0 - w) * Pd2 - 0.5
    t_pix = (cx >= -0.5) & (cx <= Pd - 0.5) & (cy >= -0.5) & (cy <= Pd - 0.5)
    dx = torch.nan_to_num((cx + 0.5).floor(), nan=0.0).clamp(0, Pd - 1).long()
    dy = torch.nan_to_num((cy + 0.5).floor(), nan=0.0).clamp(0, Pd - 1).long()
    d = case.depth.to(dtype)[cam, dy, dx]
    d = torch.where(t_pix, d, torch.full_like(d, float("inf")))
    dtol = d + _c(case.tol, dtype)
    t_d = torch.isfinite(d) & (zc <= dtol)
    nv = n[:, None]
    nc = [nv[..., 0] * Rm[..., 0, j] + nv[..., 1] * Rm[..., 1, j] + nv[..., 2] * Rm[..., 2, j] for j in range(3)]
    dot = (nc[0] * xc[0] + nc[1] * xc[1]) + nc[2] * xc[2]
    length = ((xc[0] * xc[0] + xc[1] * xc[1]) + xc[2] * xc[2]).sqrt()
    cosv = -dot / (nn.sqrt()[:, None] * length)
    if not m.cull:
        cosv = cosv.abs()
    t_cos = cosv > _c(case.min_cos, dtype)
    wt = torch.ones_like(cosv)
    for _ in range(case.power):
        wt = wt * cosv
    idx, wx, wy = taps(u, w, H, dtype)
    img = case.rgb.to(dtype).reshape(m.nscene * V, 3, H * H)
    z = torch.stack([img[cam[..., None], ch, idx] for ch in range(3)], dim=-2)                       # (K, V, 3, 4)
    col = mix(z, wx[..., None], wy[..., None])
    tests = torch.stack([t_z, t_pix, t_d, t_cos], dim=-1)
    return Pairs(scene=scene, y=y, x=x, face=face, ids_ok=ids_ok, normal_ok=normal_ok, fallback=fallback, zc=zc, cx=cx, cy=cy, d=d,
                 dtol=dtol, cosv=cosv, wt=wt, col=col, tests=tests, contributes=tests.all(-1) & normal_ok[:, None])


@dataclass
class Baked:
    texture: torch.Tensor             # (nscene, 3, A, A) in dtype
    views: torch.Tensor               # (nscene, A, A) long
    best: torch.Tensor                # (nscene, A, A) long, 255 without a view
    owned: torch.Tensor               # (nscene, A, A) bool


def blend(case, q, dtype):
    """The blend over the views in ascending order -> per owned texel (colour (K, 3), views (K,), best (K,))."""
    K, V = q.zc.shape
    sw, sc = torch.zeros(K, dtype=dtype), torch.zeros(K, 3, dtype=dtype)
    bw, bcol = torch.full((K,), -1.0, dtype=dtype), torch.zeros(K, 3, dtype=dtype)
    best, views = torch.full((K,), 255, dtype=torch.long), torch.zeros(K, dtype=torch.long)
    for v in range(V):
        on = q.contributes[:, v]
        wt = torch.where(on, q.wt[:, v], torch.zeros_like(sw))
        col = torch.where(on[:, None], q.col[:, v], torch.zeros_like(sc))
        sw = torch.where(on, sw + wt, sw)
        sc = torch.where(on[:, None], sc + wt[:, None] * col, sc)
        up = on & (wt > bw)
        bw, best = torch.where(up, wt, bw), torch.where(up, torch.full_like(best, v), best)
        bcol = torch.where(up[:, None], col, bcol)
        views = views + on.long()
    seen = views > 0
    value = bcol if case.blend == BEST else sc / torch.where(seen, sw, torch.ones_like(sw))[:, None]
    return torch.where(seen[:, None], value, q.fallback), views, best


def compose(case, q, colour, views, best, dtype):
    n, A = case.mesh.nscene, case.A
    fill = torch.tensor(FILL, dtype=torch.float32).to(dtype)
    tex = fill.reshape(1, 3, 1, 1).expand(n, 3, A, A).clone()
    vw, bs, own = torch.zeros(n, A, A, dtype=torch.long), torch.full((n, A, A), 255, dtype=torch.long), torch.zeros(n, A, A, dtype=torch.bool)
    tex[q.scene, :, q.y, q.x] = colour
    vw[q.scene, q.y, q.x], bs[q.scene, q.y, q.x], own[q.scene, q.y, q.x] = views, best, True
    return Baked(texture=tex, views=vw, best=bs, owned=own)


def bake(case, dtype=torch.float64):
    """The rule of include/mvd_hip.h evaluated in dtype -> Baked."""
    q = pairs(case, dtype)
    return compose(case, q, *blend(case, q, dtype), dtype)


# ------------------------------------------------------------------------------------------------ the exclusion rule and the bounds
@dataclass
class Ref:
    case: BakeCase
    baked: Baked                      # float64
    o32: Baked                        # the fp32 oracle
    bad: torch.Tensor                 # (nscene, A, A) bool: the texels left out
    sets_differ: int                  # kept owned texels on whose contributing set the two evaluations disagree (reported; 0 expected)
    oracle_err: float                 # max|fp32 oracle - f64| of the texture over the kept texels
    bound: float


def _err(a32, a64, mask):
    e = (a32.double() - a64).abs()[mask]
    e = e[torch.isfinite(e)]
    return float(e.max()) if e.numel() else 0.0


def ambiguous(case, q64, q32):
    """(K,) bool per owned texel -- module docstring."""
    znear = float(_c(case.mesh.znear, torch.float64))
    live = q64.normal_ok[:, None] & (q64.zc > znear) & torch.isfinite(q64.cx) & torch.isfinite(q64.cy)
    m_z = MARGIN * _err(q32.zc, q64.zc, q64.normal_ok[:, None].expand_as(live))
    m_c = MARGIN * max(_err(q32.cx, q64.cx, live), _err(q32.cy, q64.cy, live))
    inside = live & q64.tests[..., 1] & torch.isfinite(q64.d)
    m_cos = MARGIN * _err(q32.cosv, q64.cosv, live)
    near_z = (q64.zc - znear).abs() < m_z
    frac = lambda t: ((t + 0.5) - (t + 0.5).round()).abs()
    near_pix = (frac(q64.cx) < m_c) | (frac(q64.cy) < m_c)
    m_d = m_z + MARGIN * _err(q32.dtol, q64.dtol, inside & ~near_pix & torch.isfinite(q32.dtol))          # (the same pixel in both)
    near_d = torch.isfinite(q64.d) & ((q64.zc - q64.dtol).abs() < m_d)
    near_cos = (q64.cosv - float(_c(case.min_cos, torch.float64))).abs() < m_cos
    near = torch.stack([near_z, near_pix, near_d, near_cos], dim=-1)
    clear_fail = ~q64.tests & ~near
    clear_fail[..., 2] &= ~near_pix
    amb = near.any(-1) & ~clear_fail.any(-1) & q64.normal_ok[:, None]
    amb |= q64.normal_ok[:, None] & ~torch.isfinite(q64.zc)
    bad = amb.any(1)
    # the largest weight
    m_w = MARGIN * _err(q32.wt, q64.wt, q64.contributes)
    w = torch.where(q64.contributes, q64.wt, torch.full_like(q64.wt, float("-inf")))
    if w.shape[1] > 1:
        top = w.topk(2, dim=1).values
        tie32 = torch.where(q32.contributes, q32.wt.double(), torch.full_like(w, float("-inf"))).topk(2, dim=1).values
        exact = (top[:, 0] == top[:, 1]) & (tie32[:, 0] == tie32[:, 1])
        bad |= torch.isfinite(top[:, 1]) & ((top[:, 0] - top[:, 1]) < m_w) & ~exact
    return bad


def reference(case):
    q64, q32 = pairs(case), pairs(case, torch.float32)
    bad_k = ambiguous(case, q64, q32)
    owned = int(q64.scene.numel())
    share = float(bad_k.sum()) / max(owned, 1)
    assert share <= MAX_EXCLUDED, f"{share:.2%} of the owned texels are undecidable (cap {MAX_EXCLUDED:.0%}): choose another seed"
    b64 = compose(case, q64, *blend(case, q64, torch.float64), torch.float64)
    b32 = compose(case, q32, *blend(case, q32, torch.float32), torch.float32)
    bad = torch.zeros_like(b64.owned)
    bad[q64.scene, q64.y, q64.x] = bad_k
    differ = int(((q64.contributes != q32.contributes).any(1) & ~bad_k).sum())
    keep = (~bad)[:, None].expand_as(b64.texture)
    err = _err(b32.texture, b64.texture, keep)
    return Ref(case=case, baked=b64, o32=b32, bad=bad, sets_differ=differ, oracle_err=err, bound=MARGIN * err)


# ------------------------------------------------------------------------------------------------ the lookup
def sample(face, bary, face_start, nface, M, texture, T, filter, background, dtype=torch.float64):
    """mvd_texture_sample in dtype: face (ncam, P, P) long, bary (ncam, 3, P, P) fp32 as the rasteriser wrote them, texture (nscene, 3,
    A, A) fp32 -> (rgb (ncam, 3, P, P) in dtype, near (ncam, P, P) bool: MVD_TEX_NEAREST pixels closer than 1e-3 texels to a rounding
    boundary -- the inputs are fp32 numbers shared by both evaluations and t is three products and two sums of small integers, so its
    own error is a few 2^-23 A, far below that)."""
    ncam, P = face.shape[0], face.shape[-1]
    A = int(texture.shape[-1])
    K = T + 3
    C = A // K
    fs = face_start.clamp(0, nface)
    scene = torch.arange(ncam)[:, None, None].expand_as(face) // M
    l = face - fs[scene]
    ok = (face >= fs[scene]) & (face < fs[scene + 1]) & (l < 2 * C * C)
    l = torch.where(ok, l, torch.zeros_like(l))
    cell, up = l // 2, (l % 2).bool()
    ox, oy = (cell % C) * K, (cell // C) * K
    lo = lambda o, da, db, dc: torch.stack([o + da, o + db, o + dc])
    cxs = torch.where(up[None], lo(ox, K - 1, K - 1 - T, K - 1), lo(ox, 0, T, 0)).to(dtype)
    cys = torch.where(up[None], lo(oy, K - 1, K - 1, K - 1 - T), lo(oy, 0, 0, T)).to(dtype)
    b = bary.to(dtype).permute(1, 0, 2, 3)
    tx = ((b[0] * cxs[0] + b[1] * cxs[1]) + b[2] * cxs[2]).clamp(0.0, float(A - 1))
    ty = ((b[0] * cys[0] + b[1] * cys[1]) + b[2] * cys[2]).clamp(0.0, float(A - 1))
    tex = texture.to(dtype).reshape(-1, 3, A * A)
    gather = lambda idx: torch.stack([tex[scene, ch, idx] for ch in range(3)], dim=1)               # (ncam, 3, P, P)
    near = torch.zeros_like(ok)
    if filter == NEAREST:
        x, y = (tx + 0.5).floor().long().clamp(max=A - 1), (ty + 0.5).floor().long().clamp(max=A - 1)
        out = gather(y * A + x)
        frac = lambda t: ((t + 0.5) - (t + 0.5).round()).abs()
        near = ok & ((frac(tx) < 1e-3) | (frac(ty) < 1e-3))
    else:
        x0f, y0f = tx.floor(), ty.floor()
        x0, y0 = x0f.long(), y0f.long()
        x1, y1 = (x0 + 1).clamp(max=A - 1), (y0 + 1).clamp(max=A - 1)
        wx, wy = (tx - x0f)[:, None], (ty - y0f)[:, None]
        zero = torch.zeros((), dtype=dtype)
        z = [gather(y0 * A + x0), torch.where(wx != 0, gather(y0 * A + x1), zero), torch.where(wy != 0, gather(y1 * A + x0), zero),
             torch.where((wx != 0) & (wy != 0), gather(y1 * A + x1), zero)]
        out = mix(torch.stack(z, dim=-1), wx, wy)
    bg = torch.tensor(background, dtype=torch.float32).to(dtype).reshape(1, 3, 1, 1)
    return torch.where(ok[:, None], out, bg.expand_as(out)), near


# ------------------------------------------------------------------------------------------------ analytic scenes
def quad(z, half=0.5):
    """Two triangles of the square [-half, half]^2 at world z, wound so that the normal points to -z (at the unit camera), each with its
    right angle at corner a: the hypotenuse b-c, across which a chart's gutter texels extrapolate, is the shared diagonal."""
    v = torch.tensor([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]], dtype=torch.float64)
    return v, torch.tensor([[1, 0, 2], [3, 2, 0]])


@functools.lru_cache(maxsize=None)
def refs(name):
    """The Ref of a named parity case -- computed once, shared read-only; the cap is asserted here, before anything is compared."""
    return reference(CASES[name]())


def _small(nf, texels, V, seed, **kw):
    """The nf faces of the icosahedron that face view 0 most, seen by V general cameras; images of 32 pixels, depth of 48."""
    def make():
        k = dict(kw)
        g = torch.Generator().manual_seed(seed)
        v, f = R.icosahedron()
        cams = make_rig(V, True, seed % 7)[0]
        centre = -(cams.T[0].double() @ cams.R[0].double().T)                      # C R = -T
        f = f[torch.argsort(-(v[f].mean(1) @ centre), stable=True)[:nf]]           # the faces that look at view 0 first
        mesh = R.Case(vertices=v.float(), colors=torch.rand(12, 3, generator=g) if k.pop("colors", True) else None, faces=f,
                      vertex_start=torch.tensor([0, 12]), face_start=torch.tensor([0, nf]), cams=cams, nscene=1, M=V, P=48,
                      cull=k.pop("cull", 1))
        return make_bake(mesh, 32, texels, g, **k)
    return make


def _three_scenes():
    """The icosahedron's first 5 faces, an empty scene, its 20 faces: three rigs, one atlas side."""
    g = torch.Generator().manual_seed(7400)
    v, f = R.icosahedron()
    vertices = torch.cat([v, v * 0.5, v * 0.9]).float()
    faces = torch.cat([f[:5], f + 24])
    mesh = R.Case(vertices=vertices, colors=torch.rand(36, 3, generator=g), faces=faces, vertex_start=torch.tensor([0, 12, 24, 36]),
                  face_start=torch.tensor([0, 5, 5, 25]), cams=R.cat_cameras([make_rig(3, True, 11 + s)[0] for s in range(3)]), nscene=3, M=3,
                  P=48, cull=1)
    return make_bake(mesh, 32, 2, g)


def _broken_faces():
    """The sphere at cull 0 plus: faces with ids -1 and nv, a face on a NaN vertex, a zero-area face; view 2 placed behind the mesh
    (camera z <= znear for every texel: its T moved through the object)."""
    g = torch.Generator().manual_seed(7500)
    v, f = R.sphere_mesh(12)
    n = v.shape[0]
    vertices = torch.cat([v, torch.tensor([[0.1, float("nan"), 0.2]], dtype=torch.float64)]).float()
    extra = torch.tensor([[3, n + 1, 7], [-1, 2, 6], [4, n, 9], [5, 5, 8]])
    faces = torch.cat([f[:30], extra[:2], f[30:], extra[2:]])
    cams = make_rig(3, True, 2)[0]
    Tv = cams.T.clone()
    Tv[2, 2] = -Tv[2, 2]
    cams = type(cams)(cams.R, Tv, cams.focal_length, cams.principal_point)
    mesh = R.Case(vertices=vertices, colors=torch.rand(n + 1, 3, generator=g), faces=faces, vertex_start=torch.tensor([0, n + 1]),
                  face_start=torch.tensor([0, faces.shape[0]]), cams=cams, nscene=1, M=3, P=48, cull=0)
    return make_bake(mesh, 32, 2, g, power=0)


# the parity cases of tests/test_gpu_texture.py
CASES = {
    "nf0": _small(0, 2, 1, 7101),
    "nf1_t1": _small(1, 1, 1, 7102),
    "nf2_t8": _small(2, 8, 3, 7103, blend=BEST),
    "nf3_t2_nocolor": _small(3, 2, 3, 7104, colors=False, power=0),
    "nf5_t8_cull0": _small(5, 8, 3, 7105, cull=0),
    "sphere_t1": lambda: sphere_case(texels=1),
    "sphere_t2_best_wide": lambda: sphere_case(texels=2, blend=BEST, side=39 * 5),
    "sphere_t8": lambda: sphere_case(texels=8),
    "three_scenes_empty_middle": _three_scenes,
    "broken_faces_view_behind": _broken_faces,
}


def unit_rig_front_back():
    """View 0: raster_f64's unit camera (camera z = world z + 2).  View 1: the same camera turned half round the y axis -- it looks at
    the origin from the other side: xc = (-x, y, 2 - z)."""
    c = R.unit_camera()
    back = torch.diag(torch.tensor([-1.0, 1.0, -1.0]))[None]
    return type(c)(torch.cat([c.R, back]), torch.cat([c.T, c.T]), torch.cat([c.focal_length] * 2), torch.cat([c.principal_point] * 2))


def two_quads_case(texels=4, blend=MEAN, Pd=48, H=16):
    """A quad of half side 0.6 at z = 0 facing view 0 and, behind it at z = 0.5, one of half side 0.4875 facing view 1: view 0 sees only
    the front quad (the rear one lies 0.5 behind the depth it holds there, far beyond tol), view 1 only the rear one.  The rear quad's
    border projects to pixel coordinates 15.7 and 31.3 of view 1, so every texel of it -- the border and the gutter too -- falls into a
    pixel the quad covers.  cull 0, images constant per view: view 0 red, view 1 green."""
    v0, f0 = quad(0.0, 0.6)
    v1, f1 = quad(0.5, 0.4875)
    mesh = R.Case(vertices=torch.cat([v0, v1]).float(), colors=None, faces=torch.cat([f0, f1[:, [0, 2, 1]] + 4]), vertex_start=torch.tensor([0, 8]),
                  face_start=torch.tensor([0, 4]), cams=unit_rig_front_back(), nscene=1, M=2, P=Pd, cull=0)
    rgb = torch.zeros(2, 3, H, H)
    rgb[0, 0], rgb[1, 1] = 1.0, 1.0
    return BakeCase(mesh=mesh, rgb=rgb, depth=rendered_depth(mesh), texels=texels, blend=blend)


# ------------------------------------------------------------------------------------------------ end to end: detail that vertices lose
E2E = dict(G=24, P=64, V=3, cells=6, texels=8, k=25.0, rig_seed=4)


def e2e_fine():
    """The exact sphere marched at G = 24 (10 296 faces, vertices 0.06 apart: two pixels of the P = 64 views) with a colour wave of
    length 2 pi / 25 = 0.25 per axis -- finer than the 0.2 cells of simplify(cells=6), whose vertices cannot carry it; a chart of
    texels = 8 has texels of 0.025, below a pixel."""
    v, f = R.sphere_mesh(E2E["G"])
    k = E2E["k"]
    col = torch.stack([0.5 + 0.5 * torch.sin(k * v[:, 0] + 1.0), 0.5 + 0.5 * torch.sin(k * v[:, 1] + 2.0), 0.5 + 0.5 * torch.sin(k * v[:, 2])], dim=1)
    return R.Case(vertices=v.float(), colors=col.float(), faces=f, vertex_start=torch.tensor([0, v.shape[0]]),
                  face_start=torch.tensor([0, f.shape[0]]), cams=make_rig(E2E["V"], True, E2E["rig_seed"])[0], nscene=1, M=E2E["V"], P=E2E["P"],
                  cull=1)


def e2e_errors(src_rgb, src_hit, face, bary, vertex_rgb, face_start, nface, texture, views, texels):
    """(mse of the textured render, mse of the vertex-colour render, pixels compared) against the source views, over the pixels both
    meshes hit and whose four texture taps were all seen.  The lookup is this file's, in float64, on CPU tensors."""
    V = face.shape[0]
    tex_rgb, _ = sample(face, bary, face_start, nface, V, texture, texels, BILINEAR, (0.0, 0.0, 0.0))
    seen = (views > 0).float()[:, None].expand(-1, 3, -1, -1)
    all_seen, _ = sample(face, bary, face_start, nface, V, seen, texels, BILINEAR, (0.0, 0.0, 0.0))
    m = src_hit & (face >= 0) & (all_seen[:, 0] == 1.0)
    m3 = m[:, None].expand_as(tex_rgb)
    mse = lambda img: float(((img.double() - src_rgb.double())[m3] ** 2).mean())
    return mse(tex_rgb), mse(vertex_rgb), int(m.sum())


def e2e_oracle():
    """The float64 chain alone: simplify_f64 -> raster_f64 -> bake -> sample."""
    import numpy as np
    import meshtopo_f64 as M
    import simplify_f64 as S
    fine = e2e_fine()
    src = R.render(fine)
    out = S.simplify(M.make(fine.vertices.numpy(), fine.faces.numpy().astype(np.int32), rgb=fine.colors.numpy()), E2E["cells"])["out"]
    cv, cf = torch.from_numpy(out.vertices), torch.from_numpy(out.faces).long()
    coarse = R.Case(vertices=cv, colors=torch.from_numpy(out.rgb), faces=cf, vertex_start=torch.tensor([0, cv.shape[0]]),
                    face_start=torch.tensor([0, cf.shape[0]]), cams=fine.cams, nscene=1, M=fine.M, P=fine.P, cull=1)
    img = R.render(coarse)
    b = bake(BakeCase(mesh=coarse, rgb=src.rgb.float(), depth=img.depth.float(), texels=E2E["texels"]))
    return e2e_errors(src.rgb, src.hit, img.face, img.bary.float(), img.rgb, coarse.face_start, coarse.nface, b.texture.float(), b.views,
                      E2E["texels"])
