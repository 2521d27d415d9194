"""Float64 reference of the mesh rasteriser (mvd_render_mesh: include/mvd_hip.h) -- TEST INFRASTRUCTURE.

The rule of the header is written once, with torch ops on the CPU, and evaluated in a `dtype`: float64 is the reference, float32 the
"fp32 oracle" whose own error against float64 sizes the margins and the bounds -- the pattern of tests/render_f64.py.  The fp32 evaluation
is elementwise in the header's operation order (one rounding per operation).  Rigs are gridattn_f64's general ones: no vertex projects
onto a pixel centre.  Meshes: an icosahedron, hand-placed triangles, and tsdf_f64.march of an exact sphere SDF.

Which side of the image a face is seen from is a property of the INPUTS and is decided once, geometrically and in float64: the face is
front when (b - a) x (c - a) . (a - C) < 0 in world space, C the camera centre.  The header derives a sign of area2 from that; nothing
here uses the derivation.

The rule is a chain of comparisons, and float64 may sit too close to one for any fp32 evaluation to be held to its side.  With, per
(face, camera) pair, m_e = MARGIN max|e_fp32 - e_f64| over the pair's three edge functions at the pixels of its bounding box grown by one
pixel and over area2 (an edge function at a vertex), and per case m_z = MARGIN max|z_fp32 - z_f64| over the vertices' camera z and the
interpolated depths of the decided candidates, a pair is
  dropped    an id out of range, a non-finite coordinate, area2 == 0 in both evaluations, a vertex with zc <= znear - m_z, or (cull) a
             back face with |area2| >= m_e;
  ambiguous  not dropped, and a vertex zc within m_z of znear or |area2| < m_e;
  drawn      otherwise.
At a pixel a pair that is not dropped is out when sign(area2) e_i < -m_e for some edge, decided when it is drawn, every
sign(area2) e_i > m_e and z > znear + m_z, and undecided otherwise.  A PIXEL is left out of the comparison when
  - an undecided candidate's depth is below the decided minimum plus 2 m_z (it could be the winner), or
  - the two nearest decided candidates that are not the same face (the same three vertex ids) are less than 2 m_z apart.
At most MAX_EXCLUDED of a case's nscene * M * P^2 pixels may be left out, asserted by `refs` before anything is compared; a case that does
not meet the cap gets another seed, not a larger cap.
"""
import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import tsdf_f64 as T
from gridattn_f64 import MARGIN, MAX_EXCLUDED, make_rig
from mvdfusion_amd.cameras import Cameras, pack_cameras


@dataclass
class Case:
    """The arguments of one mvd_render_mesh call as CPU tensors."""
    vertices: torch.Tensor            # (n, 3) fp32
    colors: Optional[torch.Tensor]    # (n, 3) fp32 or None
    faces: torch.Tensor               # (m, 3) int64 global ids (a test may put ids outside the scene's range here)
    vertex_start: torch.Tensor        # (nscene + 1,) int64
    face_start: torch.Tensor          # (nscene + 1,) int64
    cams: Cameras                     # nscene * M
    nscene: int
    M: int
    P: int
    cull: int
    znear: float = 1e-3

    @property
    def nface(self):
        return int(self.faces.shape[0])

    @property
    def nvert(self):
        return int(self.vertices.shape[0])

    @property
    def pixels(self):
        return self.nscene * self.M * self.P * self.P

    def packed(self):
        return pack_cameras(self.cams)


def cat_cameras(cs):
    return Cameras(*(torch.cat([getattr(c, k) for c in cs]) for k in ("R", "T", "focal_length", "principal_point")))


# ------------------------------------------------------------------------------------------------ meshes
SPHERE_R = 0.6


def icosahedron(radius=SPHERE_R):
    """(12, 3) float64 vertices and (20, 3) int64 faces wound with the normal out of the solid."""
    phi = (1.0 + 5.0 ** 0.5) / 2.0
    v = []
    for s1 in (-1.0, 1.0):
        for s2 in (-1.0, 1.0):
            v += [(0.0, s1, s2 * phi), (s1, s2 * phi, 0.0), (s2 * phi, 0.0, s1)]
    v = np.array(v)
    d = np.linalg.norm(v[:, None] - v[None], axis=-1)
    edge = d[d > 0].min()
    near = np.abs(d - edge) < 1e-9
    faces = []
    for i in range(12):
        for j in range(i + 1, 12):
            for k in range(j + 1, 12):
                if near[i, j] and near[j, k] and near[i, k]:
                    n = np.cross(v[j] - v[i], v[k] - v[i])
                    faces.append((i, j, k) if n @ (v[i] + v[j] + v[k]) > 0 else (i, k, j))
    assert len(faces) == 20
    return torch.from_numpy(v / np.linalg.norm(v[0]) * radius), torch.tensor(faces, dtype=torch.long)


@functools.lru_cache(maxsize=None)
def sphere_mesh(G):
    """tsdf_f64.march of the exact sphere SDF at G^3 voxels: (vertices float64, faces int64), closed and wound outward."""
    m = T.march(T.sphere_volume(G=G, radius=SPHERE_R))
    return m.vertices, m.faces


def unproject(cams, j, px, py, z, P):
    """World point (float64) that camera j of `cams` sees at pixel coordinates (px, py) and camera z -- the inverse of the header's
    projection."""
    R, Tv, f, p = cams.R[j].double(), cams.T[j].double(), cams.focal_length[j].double(), cams.principal_point[j].double()
    px, py, z = (torch.as_tensor(t, dtype=torch.float64) for t in (px, py, z))
    u, w = 1.0 - 2.0 * (px + 0.5) / P, 1.0 - 2.0 * (py + 0.5) / P
    xc = torch.stack([(u - p[0]) * z / f[0], (w - p[1]) * z / f[1], z], dim=-1)
    return (xc - Tv) @ torch.linalg.inv(R)          # (R is orthonormal only to fp32 rounding: the inverse, not the transpose)


def _one_scene(vertices, faces, colors, cams, M, P, cull, znear=1e-3):
    n, m = vertices.shape[0], faces.shape[0]
    return Case(vertices=vertices.float(), colors=colors, faces=faces, vertex_start=torch.tensor([0, n]), face_start=torch.tensor([0, m]),
                cams=cams, nscene=1, M=M, P=P, cull=cull, znear=znear)


def _case_icosahedron(g):
    v, f = icosahedron()
    return _one_scene(v, f, torch.rand(12, 3, generator=g), make_rig(2, True, 0)[0], M=2, P=16, cull=1)


def _case_big_and_small(g):
    """One triangle with its three vertices outside the 32 x 32 image, covering it, slanted in depth; in front of part of it 70 small ones of
    either winding, four of them with a bounding box of more than 64 pixels (the wavefront path), the rest below it."""
    P, cams = 32, make_rig(1, True, 5)[0]
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    tri = [unproject(cams, 0, [-47.3, 91.6, 13.2], [-25.7, -14.4, 117.9], [1.8, 2.2, 2.0], P)]
    for k in range(70):
        size = 6.0 + 3.0 * float(rnd(1)) if k % 18 == 5 else 0.8 + 1.7 * float(rnd(1))
        centre = torch.tensor([3.0, 3.0], dtype=torch.float64) + rnd(2) * torch.tensor([16.0, 25.0], dtype=torch.float64)
        ang = float(rnd(1)) * 6.28 + torch.tensor([0.0, 2.1, 4.2], dtype=torch.float64) + 0.5 * rnd(3)
        if k % 2:
            ang = ang.flip(0)
        tri.append(unproject(cams, 0, centre[0] + size * torch.cos(ang), centre[1] + size * torch.sin(ang), 1.2 + 0.4 * rnd(3), P))
    v = torch.cat(tri)
    return _one_scene(v, torch.arange(v.shape[0]).reshape(-1, 3), torch.rand(v.shape[0], 3, generator=g), cams, M=1, P=P, cull=0)


def _case_sphere(cull):
    def make(g):
        v, f = sphere_mesh(12)
        return _one_scene(v, f, torch.rand(v.shape[0], 3, generator=g), make_rig(3, True, 1)[0], M=3, P=48, cull=cull)
    return make


def _case_two_scenes(g):
    """Scene 0: five loose vertices and no face; scene 1: the icosahedron.  A rig each."""
    v, f = icosahedron()
    loose = (torch.rand(5, 3, generator=g, dtype=torch.float64) - 0.5) * 0.8
    vertices = torch.cat([loose, v])
    return Case(vertices=vertices.float(), colors=torch.rand(17, 3, generator=g), faces=f + 5, vertex_start=torch.tensor([0, 5, 17]),
                face_start=torch.tensor([0, 0, 20]), cams=cat_cameras([make_rig(2, True, 3 + 17 * s)[0] for s in range(2)]), nscene=2, M=2,
                P=16, cull=1)


def _case_drop_rules(g):
    """The sphere with znear inside it: the faces of the near cap lie in front of znear, a ring of faces straddles it (dropped whole), and
    the back of the sphere shows through the hole (cull 0).  Appended: ten zero-area faces, a face with a NaN vertex, a face with an id past
    the vertices and one with a negative id."""
    v, f = sphere_mesh(12)
    n = v.shape[0]
    vertices = torch.cat([v, torch.tensor([[0.1, float("nan"), 0.2]], dtype=torch.float64)])
    pick = torch.randint(0, n, (10, 2), generator=g)
    zero = torch.stack([pick[:, 0], pick[:, 0], pick[:, 1]], dim=1)
    zero[5:] = torch.stack([pick[5:, 0], pick[5:, 1], pick[5:, 1]], dim=1)
    zero[9] = pick[9, 0]
    extra = torch.tensor([[3, n, 7], [4, 9, n + 1], [-1, 2, 6]])
    faces = torch.cat([f[:40], zero[:5], f[40:], zero[5:], extra])
    return _one_scene(vertices, faces, torch.rand(n + 1, 3, generator=g), make_rig(2, True, 2)[0], M=2, P=32, cull=0, znear=1.0)


# the parity cases of tests/test_gpu_raster.py
CASES = {
    "icosahedron": _case_icosahedron,
    "big_and_small": _case_big_and_small,
    "sphere_cull0": _case_sphere(0),
    "sphere_cull1": _case_sphere(1),
    "two_scenes_empty_first": _case_two_scenes,
    "drop_rules": _case_drop_rules,
}


def make_case(name):
    return CASES[name](torch.Generator().manual_seed(9500 + list(CASES).index(name)))


def duplicated(case):
    """The face list twice: the second copy has the higher ids and must lose every tie."""
    assert case.nscene == 1
    return Case(vertices=case.vertices, colors=case.colors, faces=torch.cat([case.faces, case.faces]), vertex_start=case.vertex_start,
                face_start=torch.tensor([0, 2 * case.nface]), cams=case.cams, nscene=1, M=case.M, P=case.P, cull=case.cull, znear=case.znear)


def only_faces(case, keep):
    """The case with only the faces `keep` (sorted ids): a new face list in ascending id order, face_start recounted per scene."""
    start = torch.searchsorted(keep, case.face_start)
    return Case(vertices=case.vertices, colors=case.colors, faces=case.faces[keep], vertex_start=case.vertex_start, face_start=start,
                cams=case.cams, nscene=case.nscene, M=case.M, P=case.P, cull=case.cull, znear=case.znear)


# ------------------------------------------------------------------------------------------------ the rule: per (face, camera) pair
@dataclass
class Setup:
    """Per (face, camera of the face's scene): (m, M[, 3]) tensors; coordinates in dtype."""
    px: torch.Tensor              # (m, M, 3) pixel coordinates of the vertices a, b, c
    py: torch.Tensor
    zc: torch.Tensor              # (m, M, 3)
    area2: torch.Tensor           # (m, M)
    ids_ok: torch.Tensor          # (m,) bool
    front: torch.Tensor           # (m, M) bool: float64, geometric
    normal: torch.Tensor          # (m, M, 3) unit, camera space, normal_z <= 0 (0 where the world normal vanishes)
    cam: torch.Tensor             # (m, M) long: the global camera


def _znear(case, dtype):
    return torch.tensor(case.znear, dtype=torch.float32).to(dtype)          # the kernel receives znear as a C float


def face_scene(case):
    return torch.searchsorted(case.face_start, torch.arange(case.nface), right=True) - 1


def setup(case, dtype=torch.float64):
    m, M, P = case.nface, case.M, case.P
    scene = face_scene(case).clamp(0, case.nscene - 1)
    v0, v1 = case.vertex_start[scene].clamp(0, case.nvert), case.vertex_start[scene + 1].clamp(0, case.nvert)
    ids_ok = ((case.faces >= v0[:, None]) & (case.faces < v1[:, None])).all(1)
    ids = torch.where(ids_ok[:, None], case.faces, torch.zeros_like(case.faces))
    cam = scene[:, None] * M + torch.arange(M)[None, :]                                   # (m, M)
    X = case.vertices.to(dtype)[ids]                                                       # (m, 3 vertices, 3)
    R, Tv = case.cams.R.to(dtype)[cam], case.cams.T.to(dtype)[cam]                          # (m, M, 3, 3), (m, M, 3)
    f, p = case.cams.focal_length.to(dtype)[cam], case.cams.principal_point.to(dtype)[cam]
    Xv = X[:, None]                                                                        # (m, 1, 3 vertices, 3)
    xc = [Xv[..., 0] * R[..., 0, j, None] + Xv[..., 1] * R[..., 1, j, None] + Xv[..., 2] * R[..., 2, j, None] + Tv[..., j, None]
          for j in range(3)]                                                               # (m, M, 3 vertices) each, the kernel's order
    zc = xc[2]
    u = f[..., 0, None] * xc[0] / zc + p[..., 0, None]
    w = f[..., 1, None] * xc[1] / zc + p[..., 1, None]
    P2 = 0.5 * P
    px, py = (1.0 - u) * P2 - 0.5, (1.0 - w) * P2 - 0.5
    area2 = (px[..., 1] - px[..., 0]) * (py[..., 2] - py[..., 0]) - (py[..., 1] - py[..., 0]) * (px[..., 2] - px[..., 0])
    # front: float64, world space, whatever dtype
    X64, R64, T64 = case.vertices.double()[ids], case.cams.R.double()[cam], case.cams.T.double()[cam]
    n64 = torch.linalg.cross(X64[:, 1] - X64[:, 0], X64[:, 2] - X64[:, 0])                 # (m, 3)
    C = -torch.einsum("fmj,fmij->fmi", T64, R64)                                           # C R = -T with R orthonormal: C = -T R^T
    front = ((X64[:, None, 0] - C) * n64[:, None]).sum(-1) < 0
    # the unit normal in the header's order
    nw = torch.linalg.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
    big = nw.abs().amax(1, keepdim=True)
    ok = (big > 0) & torch.isfinite(big)
    nw = nw / torch.where(ok, big, torch.ones_like(big))
    nwv = nw[:, None]
    n = torch.stack([nwv[..., 0] * R[..., 0, j] + nwv[..., 1] * R[..., 1, j] + nwv[..., 2] * R[..., 2, j] for j in range(3)], dim=-1)
    length = ((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]).sqrt()
    sg = torch.where(n[..., 2] > 0, -torch.ones_like(length), torch.ones_like(length))
    n = torch.where(ok[:, None], (n / length[..., None]) * sg[..., None], torch.zeros_like(n))
    return Setup(px=px, py=py, zc=zc, area2=area2, ids_ok=ids_ok, front=front, normal=n, cam=cam)


def finite(s):
    return torch.isfinite(s.px).all(-1) & torch.isfinite(s.py).all(-1)


def draws(case, s, dtype):
    """(m, M) bool: the header's drop rules in dtype (cull: the float64 geometric side)."""
    d = s.ids_ok[:, None] & (s.zc > _znear(case, dtype)).all(-1) & finite(s) & torch.isfinite(s.area2) & (s.area2 != 0)
    return d & s.front if case.cull else d


# ------------------------------------------------------------------------------------------------ candidates and their evaluation
@dataclass
class Cand:
    """The (pair, pixel) candidates: 1-D long tensors."""
    face: torch.Tensor
    col: torch.Tensor             # camera inside the face's scene
    x: torch.Tensor
    y: torch.Tensor
    pix: torch.Tensor             # flat pixel of the (nscene * M, P, P) image


def candidates(case, s64, pairs):
    """Every pixel of the float64 bounding box, grown by one pixel and clipped to the image, of the pairs `pairs` ((m, M) bool)."""
    P = case.P
    face, col = torch.nonzero(pairs, as_tuple=True)
    px, py = s64.px[face, col], s64.py[face, col]
    x0 = (px.amin(-1).ceil() - 1).clamp(0, P - 1).long()
    x1 = (px.amax(-1).floor() + 1).clamp(0, P - 1).long()
    y0 = (py.amin(-1).ceil() - 1).clamp(0, P - 1).long()
    y1 = (py.amax(-1).floor() + 1).clamp(0, P - 1).long()
    inside = (px.amax(-1) >= -1) & (px.amin(-1) <= P) & (py.amax(-1) >= -1) & (py.amin(-1) <= P)
    w, h = (x1 - x0 + 1) * inside, (y1 - y0 + 1) * inside
    n = w * h
    k = torch.repeat_interleave(torch.arange(face.numel()), n)
    local = torch.arange(int(n.sum())) - (n.cumsum(0) - n)[k]
    x, y = x0[k] + local % w[k].clamp(min=1), y0[k] + local // w[k].clamp(min=1)
    face, col = face[k], col[k]
    return Cand(face=face, col=col, x=x, y=y, pix=(s64.cam[face, col] * P + y) * P + x)


@dataclass
class Eval:
    e: torch.Tensor               # (K, 3): e_a, e_b, e_c times sign(area2)
    in_box: torch.Tensor          # (K,) bool: inside [ceil(min), floor(max)] of the dtype's own coordinates
    z: torch.Tensor               # (K,)
    b: torch.Tensor               # (K, 3)


def evaluate(case, s, c, dtype):
    """Coverage, depth and barycentrics of the candidates in dtype, in the header's order."""
    px, py, zc, area2 = s.px[c.face, c.col], s.py[c.face, c.col], s.zc[c.face, c.col], s.area2[c.face, c.col]
    x, y = c.x.to(dtype), c.y.to(dtype)
    e = []
    for i, j in ((1, 2), (2, 0), (0, 1)):
        e.append((px[:, i] - x) * (py[:, j] - y) - (py[:, i] - y) * (px[:, j] - x))
    e = torch.stack(e, dim=1)
    sg = torch.where(area2 > 0, torch.ones_like(area2), -torch.ones_like(area2))
    q = (e / area2[:, None]) / zc
    iz = (q[:, 0] + q[:, 1]) + q[:, 2]
    z = 1.0 / iz
    in_box = (x >= px.amin(-1).ceil()) & (x <= px.amax(-1).floor()) & (y >= py.amin(-1).ceil()) & (y <= py.amax(-1).floor())
    return Eval(e=e * sg[:, None], in_box=in_box, z=z, b=q * z[:, None])


def _amin(total, pix, val, fill):
    out = torch.full((total,), fill, dtype=val.dtype)
    return out.scatter_reduce_(0, pix, val, "amin", include_self=True)


@dataclass
class Image:
    """(nscene * M, [3,] P, P) in dtype; face int64, -1 where empty."""
    face: torch.Tensor
    hit: torch.Tensor
    depth: torch.Tensor           # +inf where empty
    bary: torch.Tensor
    normal: torch.Tensor
    rgb: Optional[torch.Tensor]   # the background is the caller's: 0 here where empty


def compose(case, s, c, ev, drawn, dtype):
    """The depth rule over the candidates `drawn` ((K,) bool): per pixel the minimum of (z, face id), lexicographic; then the outputs."""
    P, total = case.P, case.pixels
    k = torch.nonzero(drawn).reshape(-1)
    pix, z, face = c.pix[k], ev.z[k], c.face[k]
    zmin = _amin(total, pix, z, float("inf"))
    first = z == zmin[pix]
    winner = _amin(total, pix[first], face[first], case.nface)
    hit = winner < case.nface
    sel = first & (face == winner[pix])                                        # one candidate per hit pixel
    ks, ps = k[sel], pix[sel]
    assert ps.numel() == int(hit.sum()) and ps.unique().numel() == ps.numel()
    ncam = case.nscene * case.M
    cam, rem = ps // (P * P), ps % (P * P)
    bary, normal = torch.zeros(ncam, 3, P * P, dtype=dtype), torch.zeros(ncam, 3, P * P, dtype=dtype)
    bary[cam, :, rem] = ev.b[ks]
    normal[cam, :, rem] = s.normal[c.face[ks], c.col[ks]]
    rgb = None
    if case.colors is not None:
        col = case.colors.to(dtype)[case.faces[c.face[ks]].clamp(0, case.nvert - 1)]          # (hits, 3 vertices, 3 channels)
        b = ev.b[ks]
        rgb = torch.zeros(ncam, 3, P * P, dtype=dtype)
        rgb[cam, :, rem] = (b[:, 0, None] * col[:, 0] + b[:, 1, None] * col[:, 1]) + b[:, 2, None] * col[:, 2]
        rgb = rgb.reshape(ncam, 3, P, P)
    shape = (ncam, P, P)
    return Image(face=torch.where(hit, winner, torch.full_like(winner, -1)).reshape(shape), hit=hit.reshape(shape), depth=zmin.reshape(shape),
                 bary=bary.reshape(ncam, 3, P, P), normal=normal.reshape(ncam, 3, P, P), rgb=rgb)


def _drawn(case, s, c, ev, dtype):
    zn = _znear(case, dtype)
    return draws(case, s, dtype)[c.face, c.col] & (ev.e >= 0).all(1) & ev.in_box & torch.isfinite(ev.z) & (ev.z > zn)


def render(case, dtype=torch.float64):
    """The rule of include/mvd_hip.h evaluated in dtype -> Image."""
    s = setup(case, dtype)
    s64 = s if dtype == torch.float64 else setup(case)
    c = candidates(case, s64, draws(case, s, dtype) & finite(s64))
    ev = evaluate(case, s, c, dtype)
    return compose(case, s, c, ev, _drawn(case, s, c, ev, dtype), dtype)


# ------------------------------------------------------------------------------------------------ the exclusion rule and the bounds
@dataclass
class Ref:
    case: Case
    image: Image                  # float64
    o32: Image                    # the fp32 oracle
    bad: torch.Tensor             # (nscene * M, P, P) bool: the pixels left out
    m_z: float
    bounds: dict                  # depth / bary / normal / rgb -> (fp32 oracle's max error on the compared hit pixels, bound)


def _max_err(a, b, mask):
    m = mask if a.dim() == mask.dim() else mask[:, None].expand_as(a)
    return (float((a.double() - b).abs()[m].max()), float(b.abs()[m].max())) if bool(m.any()) else (0.0, 0.0)


def excluded_pixels(case, s64, s32, c, e64, e32):
    """((nscene * M, P, P) bool of the pixels left out, m_z) -- module docstring."""
    total, znear = case.pixels, float(_znear(case, torch.float64))
    m, M = case.nface, case.M
    pair = c.face * M + c.col
    # m_e per pair: the edge functions over the grown box, and area2
    err = (e32.e.double() - e64.e).abs().amax(1)
    err = torch.where(torch.isfinite(err), err, torch.zeros_like(err))
    m_e = torch.zeros(m * M, dtype=torch.float64).scatter_reduce_(0, pair, err, "amax", include_self=True).reshape(m, M)
    a_err = (s32.area2.double() - s64.area2).abs()
    m_e = MARGIN * torch.maximum(m_e, torch.where(torch.isfinite(a_err), a_err, torch.zeros_like(a_err)))
    usable = s64.ids_ok[:, None] & finite(s64) & torch.isfinite(s64.area2)
    z_err = (s32.zc.double() - s64.zc).abs()[usable]
    m_zv = MARGIN * float(z_err.max()) if z_err.numel() else 0.0
    dropped = ~usable | ((s64.area2 == 0) & (s32.area2 == 0)) | (s64.zc <= znear - m_zv).any(-1)
    if case.cull:
        dropped |= ~s64.front & (s64.area2.abs() >= m_e)
    amb_pair = ~dropped & (((s64.zc - znear).abs() < m_zv).any(-1) | (s64.area2.abs() < m_e))
    me = m_e[c.face, c.col][:, None]
    out = dropped[c.face, c.col] | (e64.e < -me).any(1)
    inside = ~out & ~amb_pair[c.face, c.col] & (e64.e > me).all(1) & torch.isfinite(e64.z)
    zi_err = (e32.z.double() - e64.z).abs()[inside]
    m_z = max(m_zv, MARGIN * float(zi_err.max()) if zi_err.numel() else 0.0)
    decided = inside & (e64.z > znear + m_z)
    undecided = ~out & ~decided
    zmin = _amin(total, c.pix[decided], e64.z[decided], float("inf"))
    zu = torch.nan_to_num(e64.z[undecided], nan=float("-inf"))
    bad = _amin(total, c.pix[undecided], zu, float("inf")) < zmin + 2 * m_z
    # the two nearest decided candidates of different faces
    group = torch.unique(case.faces, dim=0, return_inverse=True)[1]
    kd = torch.nonzero(decided).reshape(-1)
    pix, z, face = c.pix[kd], e64.z[kd], c.face[kd]
    first = z == zmin[pix]
    winner = _amin(total, pix[first], face[first], m)
    wgroup = torch.where(winner < m, group[winner.clamp(max=max(m - 1, 0))], torch.full_like(winner, -1)) if m else winner
    other = group[face] != wgroup[pix]
    bad |= (_amin(total, pix[other], z[other], float("inf")) - zmin) < 2 * m_z          # (inf - inf is NaN: compares false)
    return bad.reshape(case.nscene * M, case.P, case.P), m_z


@functools.lru_cache(maxsize=None)
def refs(name):
    """The Ref of a parity case -- computed once, shared read-only; the cap is asserted here, before anything is compared."""
    return reference(make_case(name))


def reference(case):
    s64, s32 = setup(case), setup(case, torch.float32)
    possible = s64.ids_ok[:, None] & finite(s64) & torch.isfinite(s64.area2)
    possible = possible.expand(case.nface, case.M)
    c = candidates(case, s64, possible)
    e64, e32 = evaluate(case, s64, c, torch.float64), evaluate(case, s32, c, torch.float32)
    bad, m_z = excluded_pixels(case, s64, s32, c, e64, e32)
    share = float(bad.sum()) / case.pixels
    assert share <= MAX_EXCLUDED, f"{share:.2%} of the pixels are undecidable (cap {MAX_EXCLUDED:.0%}): choose another seed"
    image = compose(case, s64, c, e64, _drawn(case, s64, c, e64, torch.float64), torch.float64)
    o32 = compose(case, s32, c, e32, _drawn(case, s32, c, e32, torch.float32), torch.float32)
    both = ~bad & image.hit & (o32.face == image.face)
    bounds = {}
    for k in ("depth", "bary", "normal", "rgb"):
        if getattr(image, k) is None:
            continue
        err, mx = _max_err(getattr(o32, k), getattr(image, k), both)
        bounds[k] = (err, MARGIN * err + 2.0 ** -23 * mx)
    return Ref(case=case, image=image, o32=o32, bad=bad, m_z=m_z, bounds=bounds)


# ------------------------------------------------------------------------------------------------ the hand-computed camera
def unit_camera():
    """R = I, T = (0, 0, 2), focal 1, principal point 0: camera z = world z + 2, u = x / zc, w = y / zc; px = (1 - u) P / 2 - 0.5."""
    return Cameras(torch.eye(3)[None], torch.tensor([[0.0, 0.0, 2.0]]), torch.ones(1, 2), torch.zeros(1, 2))


def unit_case(vertices, faces, colors=None, P=8, cull=0, znear=1e-3, cams=None):
    v = torch.as_tensor(vertices, dtype=torch.float64).reshape(-1, 3)
    return _one_scene(v, torch.as_tensor(faces, dtype=torch.long).reshape(-1, 3), colors, unit_camera() if cams is None else cams, M=1, P=P,
                      cull=cull, znear=znear)
