"""Float64 reference of the volumetric fusion (mvd_tsdf_integrate, mvd_mesh_count, mvd_mesh_emit: include/mvd_hip.h) -- TEST INFRASTRUCTURE.

The header's rules written once with torch / numpy ops on the CPU and evaluated in a `dtype`: float64 is the reference, float32 the "fp32
oracle" whose own error against float64 sizes every bound of tests/test_gpu_tsdf.py -- the pattern of tests/fusion_f64.py, whose rigs,
sphere_case, MARGIN, Z_EXCLUDE and MAX_EXCLUDED are used here.

integrate().  The FOREGROUND bits are fp32 decisions in both evaluations (fusion_f64.foreground); the box and trunc are the fp32 values the
kernel receives.  A (voxel, view) pair is undecidable where float64 sits within MARGIN x the oracle's own error of one of the rule's
comparisons:
  |zc| < Z_EXCLUDE x rig distance                  the projection is ill-conditioned, and zc > 0 is decided here
  ||u| - 1| < m_n  or  ||w| - 1| < m_n             the seen test
  ix or iy within m_n S / 2 of an integer          the choice of the four taps: the bilinear VALUE is continuous there, but "all four taps
                                                   foreground / background" is decided on the chosen taps (seen pairs only)
  |sdf + trunc| < m_z                              hidden or observed (pairs that reach it: seen, four foreground taps)
  |sdf - trunc| < m_z                              for COLOUR only: whether the observation contributes a colour sample
with m_n = MARGIN max|ndc_fp32 - ndc_f64| and m_z = MARGIN max|sdf_fp32 - sdf_f64| over the case's well-conditioned pairs, as in
fusion_f64.undecidable.  A voxel is compared when all its pairs are decidable (colour: also the colour condition); at most MAX_EXCLUDED of
a case's pairs may be left out.

march().  Marching tetrahedra written from the header's text, vectorised over cells with numpy, NOT from the kernel: the winding of every
(tetrahedron, inside pattern) is found geometrically on the unit cell (the normal of the edge midpoints against the direction from the
inside corners to the outside ones), where the kernel uses the parity of a permutation.  The signs are inputs (the caller's fp32 volume),
so faces and ids are exact in every dtype; positions and colours are evaluated in `dtype`.
"""
import itertools
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import fusion_f64 as F
from oracle import ref_torch as O

MARGIN = F.MARGIN
Z_EXCLUDE = F.Z_EXCLUDE
MAX_EXCLUDED = F.MAX_EXCLUDED


@dataclass
class TCase:
    """The arguments of one mvd_tsdf_integrate launch: a fusion_f64.Case (lat, cams, V, S, up, nscene, depth map, lo, hi) plus the volume."""
    views: F.Case
    G: int
    half_extent: float = 0.75
    center: tuple = (0.0, 0.0, 0.0)
    trunc: Optional[float] = None
    carve: int = 1
    rgb: Optional[torch.Tensor] = None        # (nscene * V, 3, P, P) fp32 or None

    def __post_init__(self):
        if self.trunc is None:
            self.trunc = 3 * 2 * self.half_extent / self.G


# the parity cases of tests/test_gpu_tsdf.py: name -> (V, S, up, G, general rig, seed, scenes, carve, colour)
CASES = {
    "v3_s8_g5": (3, 8, 1, 5, True, 0, 1, 1, False),
    "v5_s12_g9_up2_rgb": (5, 12, 2, 9, True, 1, 1, 1, True),
    "gso_v4_s8_g33_nocarve": (4, 8, 1, 33, False, 2, 1, 0, False),
    "two_scenes_g9": (3, 8, 1, 9, True, 3, 2, 1, True),
    "v1_s8_g9": (1, 8, 1, 9, True, 4, 1, 1, False),
}


def make_case(name):
    """Depth latent 0.5 N(0, 1) as fusion_f64.make_case (foreground, background and silhouette taps all occur), a rig per scene, a random
    image where the case has colour."""
    V, S, up, G, general, seed, N, carve, colour = CASES[name]
    g = torch.Generator().manual_seed(9300 + seed)
    lat = torch.randn(N * V, 5, S, S, generator=g)
    lat[:, 4] *= 0.5
    views = F.Case(lat=lat, cams=F.cat_cameras([F.G.make_rig(V, general, seed + 17 * n)[0] for n in range(N)]), V=V, S=S, up=up, nscene=N)
    rgb = torch.rand(N * V, 3, S * up, S * up, generator=g) if colour else None
    return TCase(views=views, G=G, carve=carve, rgb=rgb)


def f32(x, dtype):
    """A C float argument of the kernel, as a dtype scalar."""
    return torch.tensor(x, dtype=torch.float32).to(dtype)


def voxel_axes(G, center, half_extent, dtype):
    """Three (G,) tensors: the voxel centres along x, y, z -- (c - half_extent) + (i + 0.5) * (2 * half_extent / G), as the header writes it."""
    he = f32(half_extent, dtype)
    vs = 2 * he / G
    idx = torch.arange(G, dtype=dtype)
    return [(f32(c, dtype) - he) + (idx + 0.5) * vs for c in center]


@dataclass
class Vol:
    tsdf: torch.Tensor            # (N, G, G, G) dtype
    weight: torch.Tensor          # (N, G, G, G) int64
    color: Optional[torch.Tensor]     # (N, G, G, G, 3) dtype or None
    cweight: Optional[torch.Tensor]
    zc: torch.Tensor              # (N * G^3, V) per (voxel, view of its scene)
    u: torch.Tensor
    w: torch.Tensor
    ix: torch.Tensor
    iy: torch.Tensor
    sdf: torch.Tensor
    seen: torch.Tensor            # bool
    fg4: torch.Tensor             # bool: seen and four foreground taps (the pair reaches the sdf comparisons)


def _lookup(u, w, S):
    pix = lambda c: torch.nan_to_num(torch.clip((1.0 - c) * S / 2.0 - 0.5, 0.0, S - 1.0), nan=0.0, posinf=0.0, neginf=0.0)
    ix, iy = pix(u), pix(w)
    x0f, y0f = ix.floor(), iy.floor()
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = (x0 + 1).clamp(max=S - 1), (y0 + 1).clamp(max=S - 1)
    return ix, iy, (y0 * S + x0, y0 * S + x1, y1 * S + x0, y1 * S + x1), ix - x0f, iy - y0f


def _mix(z, wx, wy):
    return (z[0] * (1 - wx) + z[1] * wx) * (1 - wy) + (z[2] * (1 - wx) + z[3] * wx) * wy


def integrate(case, dtype=torch.float64):
    c = case.views
    V, S, P, G, N = c.V, c.S, c.P, case.G, c.nscene
    xs, ys, zs_ = voxel_axes(G, case.center, case.half_extent, dtype)
    kk, jj, ii = torch.meshgrid(torch.arange(G), torch.arange(G), torch.arange(G), indexing="ij")
    X = torch.stack([xs[ii], ys[jj], zs_[kk]], dim=-1).reshape(G ** 3, 3)
    zmap_all, fg_all = F.metric_depth(c, dtype), F.foreground(c)
    trunc = f32(case.trunc, dtype)
    out = {k: [] for k in ("tsdf", "weight", "color", "cweight", "zc", "u", "w", "ix", "iy", "sdf", "seen", "fg4")}
    for n in range(N):
        sl = slice(n * V, (n + 1) * V)
        R, T = c.cams.R[sl].to(dtype), c.cams.T[sl].to(dtype)
        f, p = c.cams.focal_length[sl].to(dtype), c.cams.principal_point[sl].to(dtype)
        ndc = O.project_ndc(R, T, f, p, X)
        u, w = ndc[..., 0].T, ndc[..., 1].T                                   # (voxels, V)
        zc = (torch.einsum("pi,nij->npj", X, R) + T[:, None, :])[..., 2].T
        seen = (zc > 0) & (u.abs() <= 1) & (w.abs() <= 1)
        ix, iy, taps, wx, wy = _lookup(u, w, S)
        view = torch.arange(V)[None, :].expand_as(ix)
        zflat, fgflat = zmap_all[sl].reshape(V, S * S), fg_all[sl].reshape(V, S * S)
        fgs = [fgflat[view, t] for t in taps]
        nfg = sum(m.long() for m in fgs)
        sdf = _mix([zflat[view, t] for t in taps], wx, wy) - zc
        fg4 = seen & (nfg == 4)
        obs_s = fg4 & ~(sdf < -trunc)
        obs_b = seen & (nfg == 0) & bool(case.carve)
        d = torch.where(obs_s, torch.minimum(torch.ones_like(sdf), sdf / trunc), torch.ones_like(sdf))
        obs = obs_s | obs_b
        total = torch.zeros(G ** 3, dtype=dtype)
        for v in range(V):                                                    # in view order, as the kernel sums
            total = total + torch.where(obs[:, v], d[:, v], torch.zeros_like(total))
        weight = obs.sum(1)
        out["tsdf"].append(torch.where(weight > 0, total / weight.clamp(min=1).to(dtype), torch.ones_like(total)).reshape(G, G, G))
        out["weight"].append(weight.reshape(G, G, G))
        if case.rgb is not None:
            img = case.rgb[sl].to(dtype).reshape(V, 3, P * P)
            _, _, ctaps, cwx, cwy = _lookup(u, w, P)
            cobs = obs_s & (sdf.abs() <= trunc)
            csum = torch.zeros(G ** 3, 3, dtype=dtype)
            for ch in range(3):
                smp = _mix([img[:, ch][view, t] for t in ctaps], cwx, cwy)
                acc = torch.zeros(G ** 3, dtype=dtype)
                for v in range(V):
                    acc = acc + torch.where(cobs[:, v], smp[:, v], torch.zeros_like(acc))
                csum[:, ch] = acc
            cw = cobs.sum(1)
            out["color"].append(torch.where(cw[:, None] > 0, csum / cw.clamp(min=1).to(dtype)[:, None], torch.zeros_like(csum)).reshape(G, G, G, 3))
            out["cweight"].append(cw.reshape(G, G, G))
        for k, t in (("zc", zc), ("u", u), ("w", w), ("ix", ix), ("iy", iy), ("sdf", sdf), ("seen", seen), ("fg4", fg4)):
            out[k].append(t)
    stack = lambda k: torch.stack(out[k]) if out[k] else None
    return Vol(tsdf=stack("tsdf"), weight=stack("weight"), color=stack("color"), cweight=stack("cweight"),
               **{k: torch.cat(out[k]) for k in ("zc", "u", "w", "ix", "iy", "sdf", "seen", "fg4")})


def undecidable(case, ref, o32):
    """(bad (voxels, V) bool for tsdf / weight, bad_colour likewise for colour / cweight, m_z, m_n) from the float64 reference and the
    fp32 oracle (module docstring); asserts the cap on both."""
    c = case.views
    lim = Z_EXCLUDE * c.distance
    trunc = float(torch.tensor(case.trunc, dtype=torch.float32))
    well = ref.zc.abs() >= lim
    near = well & (ref.u.abs() <= 2) & (ref.w.abs() <= 2)
    m_n = m_z = 0.0
    if bool(near.any()):
        m_n = MARGIN * float(torch.maximum((o32.u.double() - ref.u).abs(), (o32.w.double() - ref.w).abs())[near].max())
    if bool((well & ref.fg4).any()):
        m_z = MARGIN * float((o32.sdf.double() - ref.sdf).abs()[well & ref.fg4].max())
    bad = ref.zc.abs() < lim
    bad |= ((ref.u.abs() - 1).abs() < m_n) | ((ref.w.abs() - 1).abs() < m_n)
    m_p = m_n * c.S / 2
    at_tap = lambda t: ((t - t.round()).abs() < m_p) & (t > 0.5) & (t < c.S - 1.5)      # (floor is constant near the clamped ends)
    bad |= ref.seen & (at_tap(ref.ix) | at_tap(ref.iy))
    bad |= ref.fg4 & ((ref.sdf + trunc).abs() < m_z)
    bad_colour = bad | (ref.fg4 & ((ref.sdf - trunc).abs() < m_z))
    share = float(bad_colour.sum()) / bad.numel()
    assert share <= MAX_EXCLUDED, f"{share:.2%} of the (voxel, view) pairs are undecidable (cap {MAX_EXCLUDED:.0%})"
    return bad, bad_colour, m_z, m_n


def compared(bad, case):
    """(N, G, G, G) bool: the voxels all of whose pairs are decidable."""
    G = case.G
    return (~bad.any(1)).reshape(case.views.nscene, G, G, G)


# ------------------------------------------------------------------------------------------------ marching tetrahedra
DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))          # (dx, dy, dz), the header's order


def _tets():
    """The six Kuhn tetrahedra: per axis permutation in lexicographic order, the four corners as (dx, dy, dz) offsets."""
    out = []
    for perm in sorted(itertools.permutations(range(3))):          # x = 0, y = 1, z = 2
        c = np.zeros(3, dtype=np.int64)
        corners = [c.copy()]
        for ax in perm:
            c[ax] += 1
            corners.append(c.copy())
        out.append(np.stack(corners))
    return out


def _templates():
    """For every (tetrahedron q, inside pattern): the wound polygon as a list of corner pairs (lower corner index, upper corner index),
    found on the unit cell from edge midpoints."""
    out = {}
    for q, corners in enumerate(_tets()):
        cf = corners.astype(np.float64)
        for pattern in range(1, 15):
            ins = [k for k in range(4) if (pattern >> k) & 1]
            outs = [k for k in range(4) if not (pattern >> k) & 1]
            if len(ins) == 2:
                p, r2 = ins
                r, t = outs
                poly = [(p, r), (p, t), (r2, t), (r2, r)]
            else:
                lone, rest = (ins[0], outs) if len(ins) == 1 else (outs[0], ins)
                poly = [(lone, x) for x in rest]
            mid = [0.5 * (cf[a] + cf[b]) for a, b in poly]
            normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
            outward = cf[outs].mean(0) - cf[ins].mean(0)
            s = float(normal @ outward)
            assert abs(s) > 1e-9
            if s < 0:
                poly = poly[::-1]
            out[(q, pattern)] = [(min(a, b), max(a, b)) for a, b in poly]
    return out


@dataclass
class Mesh:
    vertices: torch.Tensor        # (n, 3) dtype
    colors: Optional[torch.Tensor]
    faces: torch.Tensor           # (m, 3) int64
    vertex_start: torch.Tensor    # (N + 1,) int64
    face_start: torch.Tensor


def march(tsdf, weight=None, color=None, cweight=None, center=(0.0, 0.0, 0.0), half_extent=0.75, fill=(0.5, 0.5, 0.5),
          dtype=torch.float64):
    """tsdf (N, G, G, G) fp32 (the volume as the kernel gets it), weight (N, G, G, G) or None = all observed."""
    N, G = tsdf.shape[0], tsdf.shape[1]
    val = tsdf.to(dtype)
    obs = np.ones((N, G, G, G), dtype=bool) if weight is None else (weight > 0).numpy()
    ins = obs & (tsdf < 0).numpy()
    # edges: (N, G, G, G, 7) in (scene, k, j, i, direction) order
    carry = np.zeros((N, G, G, G, 7), dtype=bool)
    for d, (dx, dy, dz) in enumerate(DIRS):
        lo = (slice(None), slice(0, G - dz), slice(0, G - dy), slice(0, G - dx))
        hi = (slice(None), slice(dz, G), slice(dy, G), slice(dx, G))
        carry[lo + (d,)] = obs[lo] & obs[hi] & (ins[lo] != ins[hi])
    ids = np.where(carry, np.cumsum(carry.reshape(-1)).reshape(carry.shape) - 1, -1)
    vertex_start = np.concatenate([[0], np.cumsum(carry.reshape(N, -1).sum(1))])
    # vertices
    n_, k_, j_, i_, d_ = np.nonzero(carry)
    off = np.array(DIRS)[d_]
    k2, j2, i2 = k_ + off[:, 2], j_ + off[:, 1], i_ + off[:, 0]
    first = torch.from_numpy(ins[n_, k_, j_, i_])
    axes = voxel_axes(G, center, half_extent, dtype)
    lo_x = torch.stack([axes[0][i_], axes[1][j_], axes[2][k_]], dim=1)
    hi_x = torch.stack([axes[0][i2], axes[1][j2], axes[2][k2]], dim=1)
    lo_d, hi_d = val[n_, k_, j_, i_], val[n_, k2, j2, i2]
    da, db = torch.where(first, lo_d, hi_d), torch.where(first, hi_d, lo_d)
    xa, xb = torch.where(first[:, None], lo_x, hi_x), torch.where(first[:, None], hi_x, lo_x)
    t = da / (da - db)
    vertices = xa + t[:, None] * (xb - xa)
    colors = None
    if color is not None:
        col = color.to(dtype)
        has = (cweight > 0)
        lo_c, hi_c = col[n_, k_, j_, i_], col[n_, k2, j2, i2]
        lo_h, hi_h = has[n_, k_, j_, i_], has[n_, k2, j2, i2]
        ca, cb = torch.where(first[:, None], lo_c, hi_c), torch.where(first[:, None], hi_c, lo_c)
        ha, hb = torch.where(first, lo_h, hi_h)[:, None], torch.where(first, hi_h, lo_h)[:, None]
        fillc = torch.stack([f32(v, dtype) for v in fill])[None, :].expand_as(ca)
        colors = torch.where(ha & hb, ca + t[:, None] * (cb - ca), torch.where(ha, ca, torch.where(hb, cb, fillc)))
    # faces
    tets, templates = _tets(), _templates()
    dir_of = {d: n for n, d in enumerate(DIRS)}
    C = G - 1
    cell = lambda a, dz, dy, dx: a[:, dz:dz + C, dy:dy + C, dx:dx + C]
    cell_no = np.arange(N * C ** 3).reshape(N, C, C, C)
    faces, keys = [], []
    for q, corners in enumerate(tets):
        cobs = np.stack([cell(obs, c[2], c[1], c[0]) for c in corners])
        cins = np.stack([cell(ins, c[2], c[1], c[0]) for c in corners])
        allobs = cobs.all(0)
        pattern = sum(cins[k].astype(np.int64) << k for k in range(4))
        for pat in range(1, 15):
            sel = allobs & (pattern == pat)
            if not sel.any():
                continue
            poly = []
            for a, b in templates[(q, pat)]:
                lo_c, d = corners[a], dir_of[tuple(int(x) for x in corners[b] - corners[a])]
                poly.append(cell(ids[..., d], lo_c[2], lo_c[1], lo_c[0])[sel])
            poly = np.stack(poly, axis=1)                                     # (cells, 3 or 4) wound ids
            assert (poly >= 0).all()
            rot = np.argmin(poly, axis=1)
            m = poly.shape[1]
            poly = np.take_along_axis(poly, (rot[:, None] + np.arange(m)[None, :]) % m, axis=1)
            cn = cell_no[sel]
            faces.append(poly[:, :3])
            keys.append(np.stack([cn, np.full_like(cn, q), np.zeros_like(cn)], axis=1))
            if m == 4:
                faces.append(poly[:, [0, 2, 3]])
                keys.append(np.stack([cn, np.full_like(cn, q), np.ones_like(cn)], axis=1))
    if faces:
        faces, keys = np.concatenate(faces), np.concatenate(keys)
        order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
        faces, keys = faces[order], keys[order]
        per_scene = np.bincount(keys[:, 0] // C ** 3, minlength=N)
    else:
        faces, per_scene = np.zeros((0, 3), dtype=np.int64), np.zeros(N, dtype=np.int64)
    face_start = np.concatenate([[0], np.cumsum(per_scene)])
    return Mesh(vertices=vertices, colors=colors, faces=torch.from_numpy(faces.astype(np.int64)),
                vertex_start=torch.from_numpy(vertex_start.astype(np.int64)), face_start=torch.from_numpy(face_start.astype(np.int64)))


# ------------------------------------------------------------------------------------------------ volumes for the marching tests
def sphere_volume(G=24, half_extent=0.75, radius=F.SPHERE_R, N=1):
    """The exact signed distance |X| - radius at the voxel centres, fp32 (N, G, G, G)."""
    ax = voxel_axes(G, (0.0, 0.0, 0.0), half_extent, torch.float64)
    zz, yy, xx = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return ((xx ** 2 + yy ** 2 + zz ** 2).sqrt() - radius).float()[None].repeat(N, 1, 1, 1)


def smooth_volume(G, seed, N=1):
    """A random smooth field with sign changes: a few low-frequency cosines, fp32 (N, G, G, G) in about [-1, 1]."""
    g = torch.Generator().manual_seed(9400 + seed)
    ax = torch.linspace(-1.0, 1.0, G, dtype=torch.float64)
    zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
    out = []
    for _ in range(N):
        f = torch.zeros(G, G, G, dtype=torch.float64)
        for _ in range(4):
            k = torch.rand(3, generator=g, dtype=torch.float64) * 5.0
            ph = torch.rand(1, generator=g, dtype=torch.float64) * 6.28
            f += torch.cos(k[0] * xx + k[1] * yy + k[2] * zz + ph) * (0.3 + 0.2 * float(torch.rand(1, generator=g)))
        out.append(f)
    return torch.stack(out).float()


def boundary_edges(faces):
    """Directed edges of `faces` (m, 3) whose reverse does not occur, as an (e, 2) int64 array, and whether any directed edge repeats."""
    f = faces.numpy()
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    nv = int(e.max()) + 1 if len(e) else 1
    key, rev = e[:, 0] * nv + e[:, 1], e[:, 1] * nv + e[:, 0]
    repeated = len(np.unique(key)) != len(key)
    return e[~np.isin(key, rev)], repeated
