"""Float64 reference of the view-fusion kernels (mvd_fuse_points, mvd_compact_points: include/mvd_hip.h) -- TEST INFRASTRUCTURE.

The rule of the header is written once, with torch ops on the CPU, and evaluated in a `dtype`: float64 is the reference, float32 the
"fp32 oracle" whose own error against float64 sizes the bounds of tests/test_gpu_fusion.py -- the pattern of tests/gridattn_f64.py, whose
rigs (make_rig) and exclusion constants are used here.  Geometry: oracle/ref_torch.unproject_ndc / project_ndc (camera-space z is the
third component of the same X R + T, taken before the division).

The FOREGROUND bits are computed in fp32 in both evaluations: the kernel decides lo < dn < hi on its fp32 dn = clamp((lat + 1) / 2, 0, 1)
(one addition and an exact halving of the fp32 input: the same bits in torch), and a mask is an input of the vote, not a result with an
error bar.

Undecidable pairs.  A vote is a chain of comparisons; a (point, other view) pair is left out where float64 sits too close to one of them
for any fp32 evaluation to be held to its side:
  |zc| < Z_EXCLUDE x rig distance            the projection is ill-conditioned (gridattn_f64.Z_EXCLUDE), and zc > 0 is decided here
  ||u| - 1| < m_n  or  ||w| - 1| < m_n       the seen test
  ||dz| - tau| < m_z                         the support / conflict / occlusion test (pairs that reach it: seen, four foreground taps)
with m_n = MARGIN max|ndc_fp32 - ndc_f64| and m_z = MARGIN max|dz_fp32 - dz_f64| over the case's well-conditioned pairs: |zc| above the
limit, and for the NDC margin |u|, |w| <= 2 (the comparison is with 1: a projection far outside the image is decided, its larger absolute
error says nothing about the margin needed at the border), for the dz margin seen with four foreground taps in float64.  MARGIN = 4 as in
gridattn_f64: kernel and oracle are two fp32 evaluation orders of the same formulas.  A point is compared when all its pairs are decidable;
at most MAX_EXCLUDED of a case's pairs may be left out, asserted by `undecidable` before anything else.
"""
import math
from dataclasses import dataclass

import torch

import gridattn_f64 as G
from mvdfusion_amd.cameras import Cameras, get_camera_slice, pack_cameras
from oracle import ref_torch as O

MARGIN = G.MARGIN
Z_EXCLUDE = G.Z_EXCLUDE
MAX_EXCLUDED = G.MAX_EXCLUDED

# the parity cases: name -> (V, S, up, general rig, seed, scenes)
CASES = {
    "general_v3_s8": (3, 8, 1, True, 0, 1),
    "general_v3_s8_up2": (3, 8, 2, True, 1, 1),
    "general_v5_s12": (5, 12, 1, True, 2, 1),
    "gso_v4_s8_up4": (4, 8, 4, False, 3, 1),
    "two_scenes_v3_s8": (3, 8, 1, True, 4, 2),
    "general_v1_s8": (1, 8, 2, True, 5, 1),
}
NAMED = ("general_v3_s8", "general_v3_s8_up2", "general_v5_s12", "gso_v4_s8_up4")


@dataclass
class Case:
    """The arguments of one mvd_fuse_points launch as fp32 CPU tensors."""
    lat: torch.Tensor             # (nscene * V, 5, S, S)
    cams: Cameras                 # nscene * V
    V: int
    S: int
    up: int
    nscene: int = 1
    depth_scale: float = 2.0
    depth_shift: float = 0.5
    lo: float = 0.02
    hi: float = 0.98
    tau: float = 0.05
    distance: float = G.RIG_DISTANCE

    @property
    def P(self):
        return self.S * self.up

    @property
    def npts(self):
        return self.nscene * self.V * self.P * self.P

    def packed(self):
        return pack_cameras(self.cams)


def cat_cameras(cs):
    return Cameras(*(torch.cat([getattr(c, k) for c in cs]) for k in ("R", "T", "focal_length", "principal_point")))


def make_case(name):
    """Depth latent 0.5 N(0, 1) (about 94 % foreground at lo, hi = 0.02, 0.98: foreground and background taps both occur), the other
    channels N(0, 1); a rig per scene."""
    V, S, up, general, seed, N = CASES[name]
    g = torch.Generator().manual_seed(9100 + seed)
    lat = torch.randn(N * V, 5, S, S, generator=g)
    lat[:, 4] *= 0.5
    return Case(lat=lat, cams=cat_cameras([G.make_rig(V, general, seed + 17 * n)[0] for n in range(N)]), V=V, S=S, up=up, nscene=N)


def ndc_lin(P):
    """The host table of mvd_fuse_points: pixel-centre NDC coordinates of a P-pixel axis, GridAttn's grid_lin convention."""
    return torch.linspace(1.0 - 1.0 / P, -1.0 + 1.0 / P, P, dtype=torch.float32)


@dataclass
class Ref:
    xyz: torch.Tensor             # (npts, 3) dtype
    fg: torch.Tensor              # (npts,) bool (fp32 decision)
    support: torch.Tensor         # (npts,) int64
    conflict: torch.Tensor
    other: torch.Tensor           # (npts, V) bool: v != the point's own view
    zc: torch.Tensor              # (npts, V) dtype, per (point, view of the point's rig)
    dz: torch.Tensor
    u: torch.Tensor
    w: torch.Tensor
    votes: torch.Tensor           # (npts, V) bool: the pair reached the dz comparison (other, seen, four foreground taps)


def depth01_f32(lat):
    return torch.clip((lat[:, 4].float() + 1.0) / 2.0, 0.0, 1.0)


def metric_depth(case, dtype):
    """(nscene * V, S, S) metric depth of every latent pixel in dtype."""
    return torch.clip((case.lat[:, 4].to(dtype) + 1.0) / 2.0, 0.0, 1.0) * case.depth_scale + case.depth_shift


def foreground(case):
    """(nscene * V, S, S) bool, decided on the fp32 value against the fp32 thresholds the kernel receives."""
    dn = depth01_f32(case.lat)
    return (dn > torch.tensor(case.lo, dtype=torch.float32)) & (dn < torch.tensor(case.hi, dtype=torch.float32))


def reference(case, dtype=torch.float64):
    V, S, up, P = case.V, case.S, case.up, case.P
    lin = ndc_lin(P).to(dtype)
    yy, xx = torch.meshgrid(lin, lin, indexing="ij")
    xy = torch.stack([xx, yy], dim=-1).reshape(1, P * P, 2).expand(V, -1, -1)
    zmap_all, fg_all = metric_depth(case, dtype), foreground(case)
    tau = torch.tensor(case.tau, dtype=torch.float32).to(dtype)              # the kernel receives tau as a C float
    out = {k: [] for k in ("xyz", "fg", "support", "conflict", "other", "zc", "dz", "u", "w", "votes")}
    for n in range(case.nscene):
        sl = slice(n * V, (n + 1) * V)
        R, T = case.cams.R[sl].to(dtype), case.cams.T[sl].to(dtype)
        f, p = case.cams.focal_length[sl].to(dtype), case.cams.principal_point[sl].to(dtype)
        zmap, fg = zmap_all[sl], fg_all[sl]
        fine = lambda t: t.repeat_interleave(up, dim=1).repeat_interleave(up, dim=2).reshape(V, P * P)
        X = O.unproject_ndc(R, T, f, p, xy, fine(zmap)).reshape(V * P * P, 3)                   # own points, (view, Y, X) order
        ndc = O.project_ndc(R, T, f, p, X)                                                      # (V views, points, (u, w, 1/z))
        u, w = ndc[..., 0].T, ndc[..., 1].T                                                     # (points, V)
        zc = (torch.einsum("pi,nij->npj", X, R) + T[:, None, :])[..., 2].T
        seen = (zc > 0) & (u.abs() <= 1) & (w.abs() <= 1)
        pix = lambda c: torch.nan_to_num(torch.clip((1.0 - c) * S / 2.0 - 0.5, 0.0, S - 1.0), nan=0.0, posinf=0.0, neginf=0.0)
        ix, iy = pix(u), pix(w)
        x0f, y0f = ix.floor(), iy.floor()
        x0, y0 = x0f.long(), y0f.long()
        x1, y1 = (x0 + 1).clamp(max=S - 1), (y0 + 1).clamp(max=S - 1)
        wx, wy = ix - x0f, iy - y0f
        view = torch.arange(V)[None, :].expand_as(x0)
        zflat, fgflat = zmap.reshape(V, S * S), fg.reshape(V, S * S)
        tap = lambda m, y, x: m[view, y * S + x]
        z00, z01, z10, z11 = tap(zflat, y0, x0), tap(zflat, y0, x1), tap(zflat, y1, x0), tap(zflat, y1, x1)
        all_fg = tap(fgflat, y0, x0) & tap(fgflat, y0, x1) & tap(fgflat, y1, x0) & tap(fgflat, y1, x1)
        zs = (z00 * (1 - wx) + z01 * wx) * (1 - wy) + (z10 * (1 - wx) + z11 * wx) * wy
        dz = zc - zs
        own = torch.arange(V).repeat_interleave(P * P)
        other = view != own[:, None]
        votes = other & seen & all_fg
        out["xyz"].append(X)
        out["fg"].append(fine(fg).reshape(-1))
        out["support"].append((votes & (dz.abs() <= tau)).sum(1))
        out["conflict"].append((votes & (dz < -tau)).sum(1))
        for k, t in (("other", other), ("zc", zc), ("dz", dz), ("u", u), ("w", w), ("votes", votes)):
            out[k].append(t)
    return Ref(**{k: torch.cat(v) for k, v in out.items()})


def undecidable(case, ref, o32):
    """(bad (npts, V) bool, m_z, m_n) from the float64 reference `ref` and the fp32 oracle `o32` (module docstring); asserts the cap."""
    lim = Z_EXCLUDE * case.distance
    well = ref.other & (ref.zc.abs() >= lim)
    tau = float(torch.tensor(case.tau, dtype=torch.float32))
    near = well & (ref.u.abs() <= 2) & (ref.w.abs() <= 2)
    m_n = m_z = 0.0
    if bool(near.any()):
        m_n = MARGIN * float(torch.maximum((o32.u.double() - ref.u).abs(), (o32.w.double() - ref.w).abs())[near].max())
    if bool((well & ref.votes).any()):
        m_z = MARGIN * float((o32.dz.double() - ref.dz).abs()[well & ref.votes].max())
    bad = ref.zc.abs() < lim
    bad |= ((ref.u.abs() - 1).abs() < m_n) | ((ref.w.abs() - 1).abs() < m_n)
    bad |= ref.votes & ((ref.dz.abs() - tau).abs() < m_z)
    bad &= ref.other
    share = float(bad.sum()) / max(1, int(ref.other.sum()))
    assert share <= MAX_EXCLUDED, f"{share:.2%} of the (point, view) pairs are undecidable (cap {MAX_EXCLUDED:.0%})"
    return bad, m_z, m_n


def compared_points(bad):
    return ~bad.any(1)


# ------------------------------------------------------------------------------------------------ the sphere
SPHERE_R = 0.6


def sphere_case(V=8, S=32, pull_view=None, pull=0.3):
    """A sphere of radius 0.6 at the world origin seen from V views of the GSO rig: per view the analytic ray-sphere depth in float64
    (the nearer root, in camera z), background latent = +1.  pull_view: that view's foreground moved `pull` towards its camera."""
    cams = G.make_rig(V, False)[0]
    case = Case(lat=torch.zeros(V, 5, S, S), cams=cams, V=V, S=S, up=1)
    R, T, f, p = (t.double() for t in (cams.R, cams.T, cams.focal_length, cams.principal_point))
    lin = ndc_lin(S).double()
    yy, xx = torch.meshgrid(lin, lin, indexing="ij")
    xy = torch.stack([xx, yy], dim=-1).reshape(1, S * S, 2).expand(V, -1, -1)
    ones = torch.ones(V, S * S, dtype=torch.float64)
    p1 = O.unproject_ndc(R, T, f, p, xy, ones)                    # the point of the ray at camera z = 1 ...
    d = O.unproject_ndc(R, T, f, p, xy, 2.0 * ones) - p1          # ... and its step per unit of z: X(z) = p1 + (z - 1) d
    a, b, c = (d * d).sum(-1), 2.0 * (p1 * d).sum(-1), (p1 * p1).sum(-1) - SPHERE_R ** 2
    disc = b * b - 4 * a * c
    hit = disc > 0
    z = 1.0 + (-b - disc.clamp(min=0).sqrt()) / (2 * a)
    if pull_view is not None:
        z[pull_view] -= pull
    lat = 2.0 * (z - case.depth_shift) / case.depth_scale - 1.0
    case.lat[:, 4] = torch.where(hit, lat, torch.ones_like(lat)).reshape(V, S, S).float()
    return case


def kept(ref, min_support=1, max_conflicts=0):
    return ref.fg & (ref.support >= min_support) & (ref.conflict <= max_conflicts)
