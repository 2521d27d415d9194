"""Float64 reference of the point renderer (mvd_render_points: include/mvd_hip.h) -- TEST INFRASTRUCTURE.

The rule of the header is written once, with torch ops on the CPU, and evaluated in a `dtype`: float64 is the reference, float32 the
"fp32 oracle" whose own error against float64 sizes the margins -- the pattern of tests/fusion_f64.py.  Rigs and the exclusion constants are
gridattn_f64's.  Geometry: oracle/ref_torch.project_ndc (camera-space z is the third component of the same X R + T).

Which pixel a point lands on and which of two points is nearer are comparisons; float64 may sit too close to one for any fp32 evaluation
to be held to its side.  With
  m_p = MARGIN max|c_fp32 - c_f64| over cx, cy of the pairs with |zc| >= Z_EXCLUDE x rig distance whose centre lies within r + 2 pixels of
        the image (a projection far outside is decided; its larger absolute error says nothing about the margin needed inside),
  m_z = MARGIN max|zc_fp32 - zc_f64| over the pairs with |zc| >= Z_EXCLUDE x rig distance,
a (point, camera) pair is AMBIGUOUS when |zc| is below the Z_EXCLUDE limit, zc is within m_z of znear, or cx + 0.5 or cy + 0.5 lies within
m_p of an integer (its centre pixel cannot be held to one side); every other pair is decidable: it is dropped, or draws the footprint the
float64 evaluation gives.  A PIXEL is left out of the comparison when
  - among the decidable points covering it, the nearest and the nearest point with OTHER fp32 inputs are less than 2 m_z apart in float64
    (points with identical fp32 inputs are decided by the index rule, and are compared), or
  - an ambiguous point's footprint, grown by one pixel, covers it and that point's depth is below the decidable minimum plus 2 m_z (it
    could be the winner).
At most MAX_EXCLUDED of a case's nscene * M * P^2 pixels may be left out, asserted by `excluded_pixels` before anything is compared; a case
that does not meet the cap gets another seed, not a larger cap.
"""
import functools
from dataclasses import dataclass
from typing import Optional

import torch

from gridattn_f64 import MARGIN, MAX_EXCLUDED, RIG_DISTANCE, Z_EXCLUDE, make_rig
from mvdfusion_amd.cameras import Cameras, pack_cameras
from oracle import ref_torch as O

CUBE = 1.4          # points are uniform in a cube of this side around the world origin

# the parity cases: name -> (points per scene, P, M, r, general rig, seed)
CASES = {
    "sub_wavefront_r0": ((75,), 16, 2, 0, True, 0),
    "sub_wavefront_r2": ((75,), 16, 2, 2, True, 0),
    "main_r0": ((4096,), 32, 3, 0, True, 1),
    "main_r1": ((4096,), 32, 3, 1, True, 1),
    "main_r4": ((4096,), 32, 3, 4, True, 1),
    "gso_r1": ((4096,), 32, 4, 1, False, 2),
    "two_scenes_r1": ((1500, 2596), 32, 3, 1, True, 3),
    "empty_first_scene_r1": ((0, 300), 16, 2, 1, True, 4),
}


@dataclass
class Case:
    """The arguments of one mvd_render_points call as CPU tensors."""
    xyz: torch.Tensor             # (n, 3) fp32
    color: Optional[torch.Tensor]  # (n, 3) fp32 or None
    scene: torch.Tensor           # (n,) int64, sorted
    cams: Cameras                 # nscene * M
    nscene: int
    M: int
    P: int
    r: int
    znear: float = 1e-3
    distance: float = RIG_DISTANCE

    @property
    def n(self):
        return int(self.xyz.shape[0])

    @property
    def pixels(self):
        return self.nscene * self.M * self.P * self.P

    def scene_start(self):
        return torch.searchsorted(self.scene, torch.arange(self.nscene + 1)).to(torch.int32)

    def packed(self):
        return pack_cameras(self.cams)


def cat_cameras(cs):
    return Cameras(*(torch.cat([getattr(c, k) for c in cs]) for k in ("R", "T", "focal_length", "principal_point")))


def make_case(name):
    counts, P, M, r, general, seed = CASES[name]
    g = torch.Generator().manual_seed(9300 + seed)
    n = sum(counts)
    xyz = (torch.rand(n, 3, generator=g) - 0.5) * CUBE
    color = torch.rand(n, 3, generator=g)
    scene = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
    cams = cat_cameras([make_rig(M, general, seed + 17 * s)[0] for s in range(len(counts))])
    return Case(xyz=xyz, color=color, scene=scene, cams=cams, nscene=len(counts), M=M, P=P, r=r)


def duplicated(case):
    """Every point twice: xyz concatenated with itself (the second copy has the higher index and must lose every tie)."""
    two = lambda t: torch.cat([t, t])
    assert case.nscene == 1
    return Case(xyz=two(case.xyz), color=two(case.color), scene=two(case.scene), cams=case.cams, nscene=1, M=case.M, P=case.P, r=case.r,
                znear=case.znear, distance=case.distance)


# ------------------------------------------------------------------------------------------------ the rule
@dataclass
class Proj:
    """Per (point, camera of the point's scene): (n, M) tensors in dtype."""
    zc: torch.Tensor
    cx: torch.Tensor
    cy: torch.Tensor


def project(case, dtype=torch.float64):
    n, M, P = case.n, case.M, case.P
    zc, cx, cy = (torch.zeros(n, M, dtype=dtype) for _ in range(3))
    X = case.xyz.to(dtype)
    for s in range(case.nscene):
        pts = torch.nonzero(case.scene == s).reshape(-1)
        if pts.numel() == 0:
            continue
        sl = slice(s * M, (s + 1) * M)
        R, T = case.cams.R[sl].to(dtype), case.cams.T[sl].to(dtype)
        f, p = case.cams.focal_length[sl].to(dtype), case.cams.principal_point[sl].to(dtype)
        ndc = O.project_ndc(R, T, f, p, X[pts])                                          # (M, points, (u, w, 1/z))
        zc[pts] = (torch.einsum("pi,nij->npj", X[pts], R) + T[:, None, :])[..., 2].T
        cx[pts] = ((1.0 - ndc[..., 0]) * P / 2.0 - 0.5).T
        cy[pts] = ((1.0 - ndc[..., 1]) * P / 2.0 - 0.5).T
    return Proj(zc, cx, cy)


def _znear(case, dtype):
    return torch.tensor(case.znear, dtype=torch.float32).to(dtype)          # the kernel receives znear as a C float


def _centres(proj, r, P):
    """Centre pixels (long) of the pairs whose centre is finite and near enough to the image to cover a pixel at radius r; `ok` marks them."""
    lo, hi = -(r + 2.0), P + r + 1.0
    ok = (proj.cx >= lo) & (proj.cx <= hi) & (proj.cy >= lo) & (proj.cy <= hi)          # (a NaN compares false)
    px = torch.where(ok, (proj.cx + 0.5).floor(), torch.zeros_like(proj.cx)).long()
    py = torch.where(ok, (proj.cy + 0.5).floor(), torch.zeros_like(proj.cy)).long()
    return px, py, ok


def _splat(case, pts, cam, px, py, r):
    """Footprints of radius r of the points `pts` (long) around centres (px, py) in camera `cam` (long, global): (point, flat pixel of the
    (nscene * M, P, P) image) of every covered pixel."""
    P = case.P
    ii, pix = [], []
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            x, y = px + dx, py + dy
            m = (x >= 0) & (x < P) & (y >= 0) & (y < P)
            ii.append(pts[m])
            pix.append((cam[m] * P + y[m]) * P + x[m])
    return torch.cat(ii), torch.cat(pix)


def _pairs(case, mask):
    """(point, global camera, column) of the (n, M) bool mask's pairs."""
    pts, col = torch.nonzero(mask, as_tuple=True)
    return pts, case.scene[pts] * case.M + col, col


def _amin(total, pix, val, fill):
    out = torch.full((total,), fill, dtype=val.dtype)
    return out.scatter_reduce_(0, pix, val, "amin", include_self=True)


@dataclass
class Image:
    index: torch.Tensor           # (nscene * M, P, P) int64, -1 where empty
    depth: torch.Tensor           # dtype; +inf where empty
    hit: torch.Tensor


def _nearest(case, proj, draws):
    """The depth rule over the drawing pairs `draws` ((n, M) bool): per pixel the minimum of (zc, point position), lexicographic."""
    P, total = case.P, case.pixels
    px, py, ok = _centres(proj, case.r, P)
    pts, cam, col = _pairs(case, draws & ok)
    ii, pix = _splat(case, pts, cam, px[pts, col], py[pts, col], case.r)
    z = proj.zc[ii, cam_col(case, pix, ii)]
    zmin = _amin(total, pix, z, float("inf"))
    first = z == zmin[pix]                                                   # the candidates at the pixel's minimum depth: the first wins
    index = _amin(total, pix[first], ii[first], case.n)
    hit = index < case.n
    index = torch.where(hit, index, torch.full_like(index, -1))
    shape = (case.nscene * case.M, P, P)
    return Image(index.reshape(shape), zmin.reshape(shape), hit.reshape(shape))


def cam_col(case, pix, ii):
    """Column (camera inside the point's scene) of flat pixels `pix` covered by points `ii`."""
    return pix // (case.P * case.P) - case.scene[ii] * case.M


def render(case, dtype=torch.float64):
    """The rule of include/mvd_hip.h evaluated in dtype: (Image, Proj)."""
    proj = project(case, dtype)
    return _nearest(case, proj, proj.zc > _znear(case, dtype)), proj


def colours(case, image, background):
    """(nscene * M, 3, P, P): color[index], or the background."""
    idx = image.index.clamp(min=0)
    rgb = case.color[idx].permute(0, 3, 1, 2)
    bg = torch.tensor(background, dtype=torch.float32).reshape(1, 3, 1, 1)
    return torch.where(image.hit[:, None], rgb, bg.expand_as(rgb))


# ------------------------------------------------------------------------------------------------ the exclusion rule
@dataclass
class Margins:
    m_p: float
    m_z: float
    oracle_z: float               # max|zc_fp32 - zc_f64| over the well-conditioned pairs
    max_z: float                  # max|zc_f64| over them


def margins(case, ref, o32):
    """From the float64 projection `ref` and the fp32 oracle's `o32` (module docstring)."""
    r, P = case.r, case.P
    well = ref.zc.abs() >= Z_EXCLUDE * case.distance
    near = well & (ref.cx >= -(r + 2.0)) & (ref.cx <= P - 1 + r + 2.0) & (ref.cy >= -(r + 2.0)) & (ref.cy <= P - 1 + r + 2.0)
    m_p = oz = mz = 0.0
    if bool(near.any()):
        m_p = MARGIN * float(torch.maximum((o32.cx.double() - ref.cx).abs(), (o32.cy.double() - ref.cy).abs())[near].max())
    if bool(well.any()):
        oz, mz = float((o32.zc.double() - ref.zc).abs()[well].max()), float(ref.zc.abs()[well].max())
    return Margins(m_p=m_p, m_z=MARGIN * oz, oracle_z=oz, max_z=mz)


def depth_bound(m):
    """max|kernel depth - f64| on compared pixels: two fp32 evaluation orders of the same formulas, plus one rounding of the result (the
    xyz bound of tests/test_gpu_fusion.py)."""
    return MARGIN * m.oracle_z + 2.0 ** -23 * m.max_z


def excluded_pixels(case, ref, o32):
    """((nscene * M, P, P) bool of the pixels left out, Margins) from the float64 projection and the fp32 oracle's; asserts the cap."""
    P, r, total = case.P, case.r, case.pixels
    m = margins(case, ref, o32)
    znear = float(_znear(case, torch.float64))
    near_int = lambda c: ((c + 0.5) - (c + 0.5).round()).abs() < m.m_p
    ambiguous = (ref.zc.abs() < Z_EXCLUDE * case.distance) | ((ref.zc - znear).abs() < m.m_z) | near_int(ref.cx) | near_int(ref.cy)
    ambiguous |= ~(torch.isfinite(ref.cx) & torch.isfinite(ref.cy) & torch.isfinite(ref.zc))
    draws = ~ambiguous & (ref.zc > znear)
    px, py, ok = _centres(ref, r + 1, P)

    # decidable points: the nearest per pixel, and the nearest among points with other fp32 inputs than the winner's
    pts, cam, col = _pairs(case, draws & ok)
    ii, pix = _splat(case, pts, cam, px[pts, col], py[pts, col], r)
    z = ref.zc[ii, cam_col(case, pix, ii)]
    zmin = _amin(total, pix, z, float("inf"))
    group = torch.unique(case.xyz, dim=0, return_inverse=True)[1]          # points with identical fp32 inputs share a group
    first = z == zmin[pix]
    winner = _amin(total, pix[first], ii[first], case.n)
    wgroup = torch.where(winner < case.n, group[winner.clamp(max=case.n - 1)], torch.full_like(winner, -1))
    other = group[ii] != wgroup[pix]
    zsecond = _amin(total, pix[other], z[other], float("inf"))
    bad = (zsecond - zmin) < 2 * m.m_z                                        # (inf - inf is NaN: compares false)

    # ambiguous points: wherever the footprint grown by one pixel reaches and the point could be the winner
    lost = ~torch.isfinite(ref.cx + ref.cy)                                   # (ambiguous) no centre at all: its whole camera is left out
    pts, cam, col = _pairs(case, ambiguous & ok)
    ii, pix = _splat(case, pts, cam, px[pts, col], py[pts, col], r + 1)
    zamb = _amin(total, pix, ref.zc[ii, cam_col(case, pix, ii)], float("inf"))
    bad |= zamb < zmin + 2 * m.m_z
    bad = bad.reshape(case.nscene * case.M, P, P)
    for _, c, _ in zip(*_pairs(case, lost)):
        bad[int(c)] = True
    share = float(bad.sum()) / total
    assert share <= MAX_EXCLUDED, f"{share:.2%} of the pixels are undecidable (cap {MAX_EXCLUDED:.0%}): choose another seed"
    return bad, m


@functools.lru_cache(maxsize=None)
def refs(name):
    """(case, float64 Image, float64 Proj, excluded pixels, Margins) of a parity case -- computed once, shared read-only; the cap is
    asserted here."""
    case = make_case(name)
    image, ref = render(case)
    bad, m = excluded_pixels(case, ref, project(case, torch.float32))
    return case, image, ref, bad, m


# ------------------------------------------------------------------------------------------------ the hand-computed camera
def unit_camera():
    """R = I, T = (0, 0, 2), focal 1, principal point 0: camera z = world z + 2, u = x / zc, w = y / zc."""
    return Cameras(torch.eye(3)[None], torch.tensor([[0.0, 0.0, 2.0]]), torch.ones(1, 2), torch.zeros(1, 2))


def unit_case(points, P=8, r=0, znear=1e-3):
    xyz = torch.tensor(points, dtype=torch.float32).reshape(-1, 3)
    n = xyz.shape[0]
    return Case(xyz=xyz, color=torch.arange(n * 3, dtype=torch.float32).reshape(n, 3) / 10.0, scene=torch.zeros(n, dtype=torch.long),
                cams=unit_camera(), nscene=1, M=1, P=P, r=r, znear=znear)


# ------------------------------------------------------------------------------------------------ the rule as integer minima
def torch_rule(xyz, starts, cams, M, P, r, znear):
    """The header's rule with torch ops on xyz's device, in fp32 and in the kernel's operation order (elementwise, one rounding per
    operation), as 64-bit integer minima: int64 keys (bits(zc) << 32 | i) and one scatter_reduce_(amin).  starts: nscene + 1 host ints;
    cams: Cameras of nscene * M on the device.  Returns index (nscene * M, P, P) int64."""
    dev, total = xyz.device, (len(starts) - 1) * M * P * P
    pixs, keys = [], []
    lo, hi, P2 = -(r + 2.0), P + r + 1.0, 0.5 * P
    for cam in range((len(starts) - 1) * M):
        s0, s1 = starts[cam // M], starts[cam // M + 1]
        if s1 == s0:
            continue
        X, R, T, f, p = xyz[s0:s1], cams.R[cam], cams.T[cam], cams.focal_length[cam], cams.principal_point[cam]
        xc = [X[:, 0] * R[0, j] + X[:, 1] * R[1, j] + X[:, 2] * R[2, j] + T[j] for j in range(3)]
        zc = xc[2]
        cx = (1.0 - (f[0] * xc[0] / zc + p[0])) * P2 - 0.5
        cy = (1.0 - (f[1] * xc[1] / zc + p[1])) * P2 - 0.5
        ok = (zc > znear) & (cx >= lo) & (cx <= hi) & (cy >= lo) & (cy <= hi)
        px = torch.where(ok, (cx + 0.5).floor(), torch.zeros_like(cx)).long()
        py = torch.where(ok, (cy + 0.5).floor(), torch.zeros_like(cy)).long()
        key = (zc.view(torch.int32).long() << 32) | torch.arange(s0, s1, device=dev)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                x, y = px + dx, py + dy
                inside = ok & (x >= 0) & (x < P) & (y >= 0) & (y < P)
                pixs.append(torch.where(inside, (cam * P + y) * P + x, torch.full_like(x, total)))      # outside: a cell past the image
                keys.append(key)
    empty = torch.iinfo(torch.int64).max
    z = torch.full((total + 1,), empty, dtype=torch.int64, device=dev)
    if pixs:
        z.scatter_reduce_(0, torch.cat(pixs), torch.cat(keys), "amin", include_self=True)
    z = z[:total]
    return torch.where(z == empty, torch.full_like(z, -1), z & 0xffffffff).reshape(-1, P, P)
