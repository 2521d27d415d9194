"""Sampled RGB-D views -> one depth-consistent coloured point cloud (include/mvd_hip.h: mvd_fuse_points, mvd_compact_points).

The sampler returns (V, 5, S, S) latents whose channel 4 is a depth map per view.  ``fuse_views`` unprojects every view's depth through its
camera, lets every other view of the rig vote on each point (support: that view's depth map agrees within tau; conflict: the point floats
in front of the surface that view sees), keeps the foreground points with enough support and few enough conflicts and returns them as one
cloud, coloured from the decoded images when given.  ``ViewFusion.fuse`` is the same call with the model's own depth map and decoder;
``write_ply`` saves a cloud.  Both kernels run on torch's current stream; the only host synchronisation is the read of the point count.

``render_points`` goes the other way (include/mvd_hip.h: mvd_render_points): a cloud splatted into any cameras with a z-buffer -- a novel
view, the depth map the rig as a whole implies for a view, and the map of which point each pixel shows.  It synchronises nothing.

``integrate_tsdf`` is the volumetric form of the fusion (include/mvd_hip.h: mvd_tsdf_integrate): every view's depth map integrated into a
truncated signed distance volume, and ``extract_mesh`` (mvd_mesh_count, mvd_mesh_emit) turns a volume into a closed indexed triangle mesh
with vertex colours by marching tetrahedra.  ``ViewFusion.mesh`` is both with the model's own depth map and decoder; ``write_ply`` saves a
mesh too.  The only host synchronisation is the read of the vertex and face counts.

``render_mesh`` brings a mesh back into images (include/mvd_hip.h: mvd_render_mesh): a triangle rasteriser with the point renderer's 64-bit
z-buffer -- a hole-free novel view, the depth map the surface implies for a camera, perspective-correct barycentrics, face normals and
the map of which face each pixel shows.  ``ViewFusion.render_mesh`` binds the model's depth map.  It synchronises nothing.

``nearest_points`` measures that geometry (include/mvd_hip.h: mvd_nearest_points): the exact nearest point of one cloud for every point
of another, by brute force or through a uniform grid, the same bits either way.  ``compare_geometry`` reduces the two directions to
accuracy, completeness, Chamfer distance and precision / recall / F-score per scene, and ``sample_mesh`` turns a mesh into the
deterministic surface samples both take.  ``nearest_points`` synchronises nothing; ``compare_geometry`` reads the scene offsets once.
Nothing of the model is bound here, so there is no ``ViewFusion`` method.

``knn_points`` is the same search returning the k nearest instead of one (include/mvd_hip.h: mvd_knn_points), in ascending (distance,
row) order, and ``estimate_normals`` turns such neighbour lists into a unit normal and a surface variation per point
(mvd_point_normals: centre, covariance and a 3 x 3 Jacobi in fp64).  ``sample_normals`` gives surface samples the exact normals of
their faces; ``write_ply`` saves normals with a cloud.  None of them synchronises.

``align_geometry`` puts two geometries into one frame first (include/mvd_hip.h: mvd_align_icp): point-to-point ICP on that search, the
target's grid built once, every iteration an apply, a query, a deterministic reduction of the matched pairs to moment sums and a
closed-form similarity solve, all enqueued without a host synchronisation.  ``fit_similarity`` is the closed form alone for known
pairs; both return an ``Alignment`` whose ``apply`` moves a cloud, surface samples or a mesh, so that
``compare_geometry(al.apply(cloud), scan)`` measures the reconstruction and not the misalignment.  No ``ViewFusion`` method either.
``align_to_surface`` is the point-to-plane form of that loop (mvd_plane_icp) on the normals of the target -- what converges on a dense
smooth surface, where point-to-point slides -- and ``fit_plane_step`` its one linearised step for known pairs.

``mesh_components``, ``mesh_topology``, ``filter_mesh``, ``keep_components``, ``vertex_normals`` and ``smooth_mesh`` work on the mesh
itself (include/mvd_hip.h: the mesh topology section): connected components by a lock-free union-find, a report of boundary,
non-manifold and misoriented edges with the Euler characteristic, a face filter that rebases ids -- together the floater remover --,
area-weighted vertex normals for ``write_ply``, and Taubin smoothing.  All of them rest on one deterministic vertex -> face incidence
table built on the device; each reads back at most one small table of counts.  ``ViewFusion.mesh`` forwards ``largest``, ``min_faces``
and ``smooth``.

``winding_number`` says whether a point lies inside a mesh (include/mvd_hip.h: mvd_winding_number): the generalized winding number, which
stays meaningful on the open and non-manifold meshes the steps above can leave.  ``signed_distance`` signs ``nearest_on_mesh`` with it,
``voxelize_mesh`` turns a mesh back into an occupancy volume over ``integrate_tsdf``'s box, and ``volume_iou`` is the volumetric
intersection over union beside Chamfer and F-score.  None of them synchronises; nothing of the model is bound, so no ``ViewFusion`` method.

``bake_texture`` gives a mesh the colour detail of the views (include/mvd_hip.h: mvd_texture_bake): a closed-form atlas with one chart
per face, every texel coloured from the views that see it.  ``render_mesh(texture=...)`` and ``sample_texture`` bring it back into
images (mvd_texture_sample), ``write_obj`` saves mesh and texture as OBJ + MTL + PNG, and ``ViewFusion.texture`` binds the decoder.
None of them synchronises beyond the mesh's own host tables.

How good a rendered or sampled image or depth map is -- PSNR, SSIM, abs-rel, the delta accuracies -- is measured in
``mvdfusion_amd/view_metrics.py`` (include/mvd_hip.h: mvd_image_metrics, mvd_depth_metrics): ``compare_images``, ``compare_depth``,
``compare_views`` on the ``RenderedViews`` / ``RenderedMesh`` records of this module, and ``ViewFusion.compare``.
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import hip
from .cameras import Cameras, _as_cameras, pack_cameras

DEPTH_SCALE, DEPTH_SHIFT = 2.0, 0.5          # GridAttn's defaults (view_attn_efficient2.py): metric depth = dn * scale + shift
TAU_FRACTION = 0.025                         # default tau = TAU_FRACTION * depth_scale


@dataclass
class PointCloud:
    """The kept points, in point order (scene, view, Y, X); every field is a tensor on the latents' device."""
    xyz: torch.Tensor                        # (n, 3) fp32 world coordinates
    rgb: Optional[torch.Tensor]              # (n, 3) fp32 in [0, 1], or None without colour
    support: torch.Tensor                    # (n,) uint8: other views whose depth map agrees with the point
    scene: torch.Tensor                      # (n,) int64
    view: torch.Tensor                       # (n,) int64: the view the point was unprojected from
    pixel: torch.Tensor                      # (n, 2) int64: (Y, X) on that view's P x P grid
    index: torch.Tensor                      # (n,) int32: ((scene * V + view) * P + Y) * P + X, as the kernel wrote it

    def __len__(self):
        return int(self.xyz.shape[0])


def _ndc_lin(P, device):
    return torch.linspace(1.0 - 1.0 / P, -1.0 + 1.0 / P, P, dtype=torch.float32).to(device)


def _scratch(nbytes, dev):
    return torch.empty((int(nbytes) + 7) // 8, dtype=torch.int64, device=dev)


def _p(t):
    """The pointer the library takes for ``t``: NULL for None and for an empty tensor."""
    return hip.ptr(t) if t is not None and t.numel() else None


def _run(lat, rgb, cams, N, V, S, up, depth_scale, depth_shift, lo, hi, tau, min_support, max_conflicts):
    """The two launches.  lat (N*V, 5, S, S), rgb (N*V, 3, P, P) or None, cams (N*V, CAM_RECORD), all fp32 on one GPU.  Returns
    (xyz, rgb or None, support, index) cut to the kept points -- one host read, of the count."""
    L = hip.lib()
    dev, P = lat.device, S * up
    npts = N * V * P * P
    hip._req(lat), hip._req(cams)
    if rgb is not None:
        hip._req(rgb)
    u8 = lambda *shape: torch.empty(*shape, dtype=torch.uint8, device=dev)
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    xyz, support, conflict, flags = f32(npts, 3), u8(npts), u8(npts), u8(npts)
    color = f32(npts, 3) if rgb is not None else None
    lin = _ndc_lin(P, dev)
    hip.check(L.mvd_fuse_points(hip.ptr(lat), hip.ptr(rgb), hip.ptr(cams), hip.ptr(lin), hip.ptr(xyz), hip.ptr(color), hip.ptr(support),
                                hip.ptr(conflict), hip.ptr(flags), N, V, S, up, float(depth_scale), float(depth_shift), float(lo),
                                float(hi), float(tau), hip.FUSE_STAGE_AUTO, hip.stream()))
    out_xyz, out_support = f32(npts, 3), u8(npts)
    out_color = f32(npts, 3) if rgb is not None else None
    out_index = torch.empty(npts, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = int(L.mvd_compact_points_scratch(npts))
    scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    hip.check(L.mvd_compact_points(hip.ptr(xyz), hip.ptr(color), hip.ptr(support), hip.ptr(conflict), hip.ptr(flags), npts,
                                   int(min_support), int(max_conflicts), hip.ptr(out_xyz), hip.ptr(out_color), hip.ptr(out_support),
                                   hip.ptr(out_index), hip.ptr(count), hip.ptr(scratch), nbytes, hip.stream()))
    n = int(count.item())
    return out_xyz[:n], None if out_color is None else out_color[:n], out_support[:n], out_index[:n]


def _cat_cameras(cs):
    cs = [_as_cameras(c) for c in cs]
    return Cameras(*(torch.cat([getattr(c, k) for c in cs]) for k in ("R", "T", "focal_length", "principal_point")))


def _check_views(latents, cameras, rgb, up, foreground):
    """The argument conventions shared by ``fuse_views`` and ``integrate_tsdf``: (V, 5, S, S) latents with one camera set or (N, V, 5, S, S)
    with a list of N.  Returns (latents (N, V, 5, S, S), camera sets, rgb with a scene dimension or None, single, (N, V, S, up, P), (lo, hi))."""
    if not torch.is_tensor(latents) or latents.dim() not in (4, 5):
        raise ValueError("latents must be a (V, 5, S, S) or (N, V, 5, S, S) tensor")
    single = latents.dim() == 4
    if single:
        if isinstance(cameras, (list, tuple)):
            raise ValueError("(V, 5, S, S) latents take one camera set, not a list")
        latents, cameras = latents[None], [cameras]
        rgb = None if rgb is None else rgb[None]
    elif not isinstance(cameras, (list, tuple)) or len(cameras) != latents.shape[0]:
        raise ValueError(f"(N, V, 5, S, S) latents take a list of N = {latents.shape[0]} camera sets")
    N, V, C, S, S2 = latents.shape
    if C != 5 or S != S2 or S < 2:
        raise ValueError(f"latents of shape {tuple(latents.shape)}: need 5 channels and a square map of at least 2 x 2")
    if not 1 <= V <= 255:
        raise ValueError(f"V = {V} views outside [1, 255]")
    if int(up) != up or up < 1:
        raise ValueError(f"up = {up}: an integer >= 1")
    up = int(up)
    P = S * up
    if N * V * P * P >= 2 ** 31:
        raise ValueError(f"{N * V * P * P} points: the point index is 31 bits")
    lo, hi = (float(v) for v in foreground)
    if not lo < hi:
        raise ValueError(f"foreground = {foreground}: need lo < hi")
    return latents, cameras, rgb, single, (N, V, S, up, P), (lo, hi)


def _pack_views(latents, cameras, rgb, N, V, S, up, P):
    """The checked views as the kernels take them: (lat (N*V, 5, S, S) fp32, camera records on its device, rgb (N*V, 3, P, P) or None) --
    an image wider than P is area-resized, a narrower one refused."""
    cams = _cat_cameras(cameras)
    if len(cams) != N * V:
        raise ValueError(f"{len(cams)} cameras for {N} x {V} views")
    dev = latents.device
    if rgb is not None:
        if rgb.dim() != 5 or tuple(rgb.shape[:3]) != (N, V, 3) or rgb.shape[3] != rgb.shape[4]:
            raise ValueError(f"rgb of shape {tuple(rgb.shape)} does not go with latents of shape {tuple(latents.shape)}")
        H = rgb.shape[-1]
        if H < P:
            raise ValueError(f"rgb is {H} pixels wide, the output grid {P} (S = {S}, up = {up}): choose up <= {H // S}")
        rgb = rgb.reshape(N * V, 3, H, H).to(dev, torch.float32)
        if H > P:
            rgb = torch.nn.functional.interpolate(rgb, size=(P, P), mode="area")
        rgb = rgb.contiguous()
    lat = latents.reshape(N * V, 5, S, S).float().contiguous()
    return lat, pack_cameras(cams).to(dev), rgb


def fuse_views(latents, cameras, rgb=None, up=1, tau=None, min_support=1, max_conflicts=0, foreground=(0.02, 0.98),
               depth_scale=DEPTH_SCALE, depth_shift=DEPTH_SHIFT):
    """Fuse sampled views into a PointCloud.

    latents : (V, 5, S, S) with ``cameras`` the V batch cameras, or (N, V, 5, S, S) with a list of N camera sets (what ``sample_scenes``
              returns); channel 4 is the depth map in [-1, 1].
    rgb     : (.., 3, H, H) in [0, 1] with the latents' leading dimensions, or None.  The output grid has P = S * up pixels per side; an
              image with H > P is resized to P with F.interpolate(mode="area"), H < P is refused (choose a smaller ``up``).
    up      : integer >= 1.  A fine pixel takes the depth of the latent pixel it lies in and its own ray.
    tau     : depth agreement in the units of depth_scale; default 0.025 * depth_scale.
    A point is kept when it is foreground (foreground[0] < normalised depth < foreground[1]), at least ``min_support`` other views agree
    with it and at most ``max_conflicts`` see their own surface behind it.

    The defaults (tau, min_support, max_conflicts, foreground) are INTERFACE defaults: no trained checkpoint was available when this
    was written, so nobody has tuned them on real samples -- expect to.  depth_scale / depth_shift must be those of the model that made
    the latents (``ViewFusion.fuse`` passes its own)."""
    latents, cameras, rgb, single, (N, V, S, up, P), (lo, hi) = _check_views(latents, cameras, rgb, up, foreground)
    tau = TAU_FRACTION * float(depth_scale) if tau is None else float(tau)
    if not tau >= 0:
        raise ValueError(f"tau = {tau}: >= 0")
    if not (0 <= int(min_support) <= 255 and 0 <= int(max_conflicts) <= 255):
        raise ValueError("min_support and max_conflicts are counts in [0, 255]")
    lat, cams, rgb = _pack_views(latents, cameras, rgb, N, V, S, up, P)
    xyz, color, support, index = _run(lat, rgb, cams, N, V, S, up, depth_scale, depth_shift, lo, hi, tau, min_support,
                                      max_conflicts)
    i = index.long()
    return PointCloud(xyz=xyz, rgb=color, support=support, scene=i // (V * P * P), view=(i // (P * P)) % V,
                      pixel=torch.stack([(i // P) % P, i % P], dim=1), index=index)


def _depth_latent(depth, hit, scale, shift):
    """clamp(2 (z - shift) / scale - 1, -1, 1) with empty pixels at +1: the one formula behind ``depth_latent`` of both renderers."""
    lat = torch.clamp(2.0 * (depth - float(shift)) / float(scale) - 1.0, -1.0, 1.0)
    return torch.where(hit, lat, torch.ones_like(lat))


@dataclass
class RenderedViews:
    """What ``render_points`` returns; the leading scene dimension is present only when a list of camera sets was passed."""
    rgb: Optional[torch.Tensor]              # (.., M, 3, P, P) fp32: the colour of the nearest point, or the background; None without colour
    depth: torch.Tensor                      # (.., M, P, P) fp32: its camera-space z, or empty_depth
    index: torch.Tensor                      # (.., M, P, P) int32: its position in the cloud, or -1
    hit: torch.Tensor                        # (.., M, P, P) bool: index >= 0

    _depth_map = (DEPTH_SCALE, DEPTH_SHIFT)  # depth_latent's defaults (not a field; ViewFusion.render binds the model's own per instance)

    def depth_latent(self, depth_scale=None, depth_shift=None):
        """The depth map in the model's depth-channel convention, clamp(2 (z - shift) / scale - 1, -1, 1) with empty pixels at +1: the
        inverse of ``fuse_views``' map z = clamp((lat + 1) / 2, 0, 1) * scale + shift.  Defaults: DEPTH_SCALE, DEPTH_SHIFT."""
        scale = self._depth_map[0] if depth_scale is None else depth_scale
        shift = self._depth_map[1] if depth_shift is None else depth_shift
        return _depth_latent(self.depth, self.hit, scale, shift)


def _render(xyz, color, scene_start, cams, N, M, P, radius, znear, empty_depth, background):
    """The three enqueues of mvd_render_points.  xyz (n, 3), color (n, 3) or None, scene_start (N + 1) int32, cams (N*M, CAM_RECORD), all
    contiguous on one GPU.  Returns (rgb or None, depth, index) of shapes (N*M, [3,] P, P).  No host synchronisation."""
    import ctypes
    L = hip.lib()
    dev, n = xyz.device, int(xyz.shape[0])
    hip._req(xyz), hip._req(cams), hip._req(scene_start, torch.int32)
    if color is not None:
        hip._req(color)
    index = torch.empty(N * M, P, P, dtype=torch.int32, device=dev)
    depth = torch.empty(N * M, P, P, dtype=torch.float32, device=dev)
    rgb = torch.empty(N * M, 3, P, P, dtype=torch.float32, device=dev) if color is not None else None
    nbytes = int(L.mvd_render_points_scratch(N * M, P))
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    bg = (ctypes.c_float * 3)(*background)
    hip.check(L.mvd_render_points(hip.ptr(xyz), hip.ptr(color), hip.ptr(scene_start), hip.ptr(cams), n, N, M, P, radius, float(znear),
                                  float(empty_depth), bg, hip.ptr(index), hip.ptr(depth), hip.ptr(rgb), hip.ptr(scratch), nbytes, hip.stream()))
    return rgb, depth, index


def render_points(cloud, cameras, size=256, radius=1, background=(1.0, 1.0, 1.0), znear=1e-3, empty_depth=float("inf")):
    """Render a cloud into cameras by z-buffered point splatting (include/mvd_hip.h: mvd_render_points) -> RenderedViews.

    cloud   : a PointCloud, or an (n, 3) tensor (one scene, no colour).
    cameras : M cameras (anything with .R .T .focal_length .principal_point): every point is drawn into each of them, and the cloud must
              be one scene's.  Or a list of N sets of M cameras each: scene s of the cloud goes into set s (``cloud.scene`` < N), and
              the outputs get a leading dimension N.
    size    : P, the output side in pixels.  radius: a point covers the (2 radius + 1)^2 pixels around its centre pixel,
              0 <= radius <= hip.SPLAT_MAX_RADIUS.  Per pixel the nearest point with camera z > znear wins (ties: the first in the cloud).
    background, empty_depth : what a pixel no point covers holds in rgb / depth.
    Nothing is read back from the device, so ``cloud.scene`` < N is checked only for a cloud in host memory; on the GPU a point of a
    scene >= N is drawn nowhere."""
    if isinstance(cloud, PointCloud):
        xyz, color, scene = cloud.xyz, cloud.rgb, cloud.scene
    elif torch.is_tensor(cloud):
        xyz, color, scene = cloud, None, None
    else:
        raise ValueError("cloud must be a PointCloud or an (n, 3) tensor")
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"cloud: xyz of shape {tuple(xyz.shape)}, need (n, 3)")
    n = int(xyz.shape[0])
    if n > 2 ** 31 - 1:
        raise ValueError(f"cloud: {n} points, the point index is 31 bits")
    if color is not None and tuple(color.shape) != (n, 3):
        raise ValueError(f"cloud: rgb of shape {tuple(color.shape)} for {n} points")
    if scene is not None and tuple(scene.shape) != (n,):
        raise ValueError(f"cloud: scene of shape {tuple(scene.shape)} for {n} points")
    if int(size) != size or size < 1:
        raise ValueError(f"size = {size}: an integer >= 1")
    if int(radius) != radius or not 0 <= radius <= hip.SPLAT_MAX_RADIUS:
        raise ValueError(f"radius = {radius}: an integer in [0, {hip.SPLAT_MAX_RADIUS}]")
    P, radius, znear = int(size), int(radius), float(znear)
    if not znear >= 0:
        raise ValueError(f"znear = {znear}: >= 0")
    background = tuple(float(v) for v in background)
    if len(background) != 3:
        raise ValueError(f"background = {background}: three floats")
    single = not isinstance(cameras, (list, tuple))
    sets = [_as_cameras(c) for c in ([cameras] if single else cameras)]
    N = len(sets)
    if N < 1:
        raise ValueError("cameras: an empty list")
    M = len(sets[0])
    if M < 1 or any(len(c) != M for c in sets):
        raise ValueError(f"cameras: every scene needs the same number M >= 1 of cameras, got {[len(c) for c in sets]}")
    if N * M > 65535:
        raise ValueError(f"cameras: {N} x {M} cameras, at most 65535 per call")
    if N * M * P * P >= 2 ** 31:
        raise ValueError(f"size = {P}: {N * M * P * P} pixels for {N} x {M} cameras, the pixel index is 31 bits")
    if scene is None and N != 1:
        raise ValueError(f"cameras: a list of {N} camera sets needs a PointCloud (an (n, 3) tensor is one scene)")
    if scene is not None and n and scene.device.type == "cpu" and not 0 <= int(scene.min()) <= int(scene.max()) < N:
        raise ValueError(f"cameras: {N} camera set(s) for a cloud with scenes {int(scene.min())} .. {int(scene.max())}")
    dev = xyz.device
    xyz = xyz.float().contiguous()
    color = None if color is None else color.to(dev, torch.float32).contiguous()
    if scene is None or n == 0:
        scene_start = torch.tensor([0] + [n] * N, dtype=torch.int32).to(dev)
    else:      # offsets of the sorted scene ids, on the device: a scene id >= N leaves its points past the last range, drawn nowhere
        bounds = torch.arange(N + 1, dtype=scene.dtype, device=scene.device)
        scene_start = torch.searchsorted(scene.contiguous(), bounds).to(dev, torch.int32)
    cams = Cameras(*(torch.cat([getattr(c, k) for c in sets]) for k in ("R", "T", "focal_length", "principal_point")))
    rgb, depth, index = _render(xyz, color, scene_start, pack_cameras(cams).to(dev).contiguous(), N, M, P, radius, znear, empty_depth, background)
    lead = (M,) if single else (N, M)
    index = index.reshape(*lead, P, P)
    return RenderedViews(rgb=None if rgb is None else rgb.reshape(*lead, 3, P, P), depth=depth.reshape(*lead, P, P), index=index,
                         hit=index >= 0)


@dataclass
class TSDFVolume:
    """What ``integrate_tsdf`` returns.  The arrays are (G, G, G) in z, y, x order for (V, 5, S, S) latents and (N, G, G, G) for a list of
    scenes, on the latents' device; voxel (k, j, i) has its centre at center - half_extent + (index + 0.5) * 2 * half_extent / G per axis."""
    tsdf: torch.Tensor                       # fp32: the mean truncated signed distance in units of trunc, <= 1; 1 where weight == 0
    weight: torch.Tensor                     # uint8: the views that observed the voxel
    rgb: Optional[torch.Tensor]              # (.., 3) fp32: the mean colour sample, 0 where cweight == 0; None without colour
    cweight: Optional[torch.Tensor]          # uint8: the views that contributed a colour sample
    center: tuple
    half_extent: float
    trunc: float


@dataclass
class TriangleMesh:
    """What ``extract_mesh`` returns: an indexed triangle mesh, scene after scene.  ``faces`` holds GLOBAL vertex ids; scene s owns the
    vertices [vertex_start[s], vertex_start[s + 1]) and the faces [face_start[s], face_start[s + 1]).  vertices, faces and rgb live on the
    volume's device, the two offset tables on the host (they are what the host read to allocate the rest)."""
    vertices: torch.Tensor                   # (n, 3) fp32 world coordinates
    faces: torch.Tensor                      # (m, 3) int32, wound so that the normal points out of the surface
    rgb: Optional[torch.Tensor]              # (n, 3) fp32, or None without colour
    vertex_start: torch.Tensor               # (N + 1,) int32, host
    face_start: torch.Tensor                 # (N + 1,) int32, host

    def __len__(self):
        return int(self.faces.shape[0])

    def scene(self, s):
        """The sub-mesh of scene s, its faces rebased to its own vertices."""
        N = int(self.vertex_start.numel()) - 1
        if not 0 <= s < N:
            raise ValueError(f"scene {s} of a mesh of {N} scene(s)")
        v0, v1, f0, f1 = (int(t[i]) for t in (self.vertex_start, self.face_start) for i in (s, s + 1))
        return TriangleMesh(vertices=self.vertices[v0:v1], faces=self.faces[f0:f1] - v0, rgb=None if self.rgb is None else self.rgb[v0:v1],
                            vertex_start=torch.tensor([0, v1 - v0], dtype=torch.int32), face_start=torch.tensor([0, f1 - f0], dtype=torch.int32))


def _check_box(grid, center, half_extent, N):
    if int(grid) != grid or not 2 <= grid <= 256:
        raise ValueError(f"grid = {grid}: an integer in [2, 256]")
    G = int(grid)
    if 7 * N * G ** 3 >= 2 ** 31 or 12 * N * (G - 1) ** 3 >= 2 ** 31:
        raise ValueError(f"grid = {G} for {N} scene(s): the edge and face indices are 31 bits (7 N G^3 and 12 N (G - 1)^3 < 2^31)")
    center = tuple(float(v) for v in center)
    if len(center) != 3:
        raise ValueError(f"center = {center}: three floats")
    half_extent = float(half_extent)
    if not half_extent > 0:
        raise ValueError(f"half_extent = {half_extent}: > 0")
    return G, center, half_extent


def _integrate(lat, rgb, cams, N, V, S, up, G, center, half_extent, trunc, carve, depth_scale, depth_shift, lo, hi):
    """The launch of mvd_tsdf_integrate.  lat (N*V, 5, S, S), rgb (N*V, 3, P, P) or None, cams (N*V, CAM_RECORD), all fp32 on one GPU.
    Returns (tsdf, weight, color or None, cweight or None) with a leading scene dimension.  No host synchronisation."""
    dev = lat.device
    hip._req(lat), hip._req(cams)
    tsdf = torch.empty(N, G, G, G, dtype=torch.float32, device=dev)
    weight = torch.empty(N, G, G, G, dtype=torch.uint8, device=dev)
    color = cweight = None
    if rgb is not None:
        hip._req(rgb)
        color = torch.empty(N, G, G, G, 3, dtype=torch.float32, device=dev)
        cweight = torch.empty(N, G, G, G, dtype=torch.uint8, device=dev)
    hip.check(hip.lib().mvd_tsdf_integrate(hip.ptr(lat), hip.ptr(rgb), hip.ptr(cams), hip.ptr(tsdf), hip.ptr(weight), hip.ptr(color),
                                           hip.ptr(cweight), N, V, S, up, G, *center, half_extent, trunc, int(carve),
                                           float(depth_scale), float(depth_shift), lo, hi, hip.stream()))
    return tsdf, weight, color, cweight


def integrate_tsdf(latents, cameras, rgb=None, grid=128, center=(0, 0, 0), half_extent=0.75, trunc=None, carve=True,
                   foreground=(0.02, 0.98), up=1, depth_scale=DEPTH_SCALE, depth_shift=DEPTH_SHIFT):
    """Integrate sampled views into a TSDFVolume (include/mvd_hip.h: mvd_tsdf_integrate has the rule in full).

    latents, cameras, rgb, up, foreground : as ``fuse_views`` takes them.  ``up`` only sets the side P = S * up of the colour images.
    grid        : G, voxels per side, 2 .. 256; center, half_extent: the world box center +- half_extent, the same for every scene.
    trunc       : the truncation distance in the units of depth_scale; default 3 voxels, 3 * 2 * half_extent / grid.
    Per voxel centre and view: the view's depth map is looked up where the voxel projects.  On foreground, sdf = surface depth - voxel
    depth: the voxel is skipped when sdf < -trunc (hidden), else it observes min(1, sdf / trunc), and samples the colour when
    |sdf| <= trunc.  On background it observes 1 (free space) when ``carve``, nothing otherwise; at a silhouette nothing.

    half_extent, trunc, carve and foreground are INTERFACE defaults: no trained checkpoint was available when this was written, so nobody
    has tuned them on real samples -- expect to (half_extent = 0.75 merely holds the unit-radius-ish objects of the GSO rig at distance
    1.5).  depth_scale / depth_shift must be those of the model that made the latents (``ViewFusion.mesh`` passes its own)."""
    latents, cameras, rgb, single, (N, V, S, up, P), (lo, hi) = _check_views(latents, cameras, rgb, up, foreground)
    G, center, half_extent = _check_box(grid, center, half_extent, N)
    trunc = 3 * 2 * half_extent / G if trunc is None else float(trunc)
    if not trunc > 0:
        raise ValueError(f"trunc = {trunc}: > 0")
    lat, cams, rgb = _pack_views(latents, cameras, rgb, N, V, S, up, P)
    tsdf, weight, color, cweight = _integrate(lat, rgb, cams, N, V, S, up, G, center, half_extent, trunc, bool(carve), depth_scale,
                                              depth_shift, lo, hi)
    cut = (lambda t: None if t is None else t[0]) if single else (lambda t: t)
    return TSDFVolume(tsdf=cut(tsdf), weight=cut(weight), rgb=cut(color), cweight=cut(cweight), center=center, half_extent=half_extent,
                      trunc=trunc)


def _march(tsdf, weight, color, cweight, N, G, center, half_extent, fill):
    """mvd_mesh_count, the host read of the 2 (N + 1) offsets, mvd_mesh_emit into exact outputs.  tsdf (N, G, G, G) on a GPU; weight None =
    every voxel observed.  Returns (vertices, colors or None, faces, vertex_start, face_start), the last two on the host."""
    import ctypes
    L = hip.lib()
    dev = tsdf.device
    tsdf = hip._req(tsdf.float().contiguous())
    weight = torch.ones(tsdf.shape, dtype=torch.uint8, device=dev) if weight is None else hip._req(weight.to(dev).contiguous(), torch.uint8)
    if color is not None:
        color, cweight = hip._req(color.to(dev, torch.float32).contiguous()), hip._req(cweight.to(dev).contiguous(), torch.uint8)
    nbytes = int(L.mvd_mesh_scratch(N, G))
    scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    starts = torch.empty(2, N + 1, dtype=torch.int32, device=dev)
    hip.check(L.mvd_mesh_count(hip.ptr(tsdf), hip.ptr(weight), N, G, hip.ptr(starts[0]), hip.ptr(starts[1]), hip.ptr(scratch), nbytes,
                               hip.stream()))
    starts = starts.cpu()                                          # the one host synchronisation
    nvert, nface = int(starts[0, N]), int(starts[1, N])
    vertices = torch.empty(nvert, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(nface, 3, dtype=torch.int32, device=dev)
    colors = torch.empty(nvert, 3, dtype=torch.float32, device=dev) if color is not None else None
    hip.check(L.mvd_mesh_emit(hip.ptr(tsdf), hip.ptr(weight), hip.ptr(color), hip.ptr(cweight), N, G, *center, half_extent,
                              (ctypes.c_float * 3)(*fill), _p(vertices), _p(colors), _p(faces), nvert, nface, hip.ptr(scratch), nbytes,
                              hip.stream()))
    return vertices, colors, faces, starts[0].clone(), starts[1].clone()


def extract_mesh(volume, fill=(0.5, 0.5, 0.5)):
    """A TSDFVolume -> TriangleMesh by marching tetrahedra (include/mvd_hip.h: mvd_mesh_count, mvd_mesh_emit): closed wherever the volume
    is observed, every triangle wound with its normal out of the surface, vertices and faces in a fixed order (the same bits run to run).

    volume : a TSDFVolume, or a bare (G, G, G) / (N, G, G, G) tensor of signed distances (negative inside): every voxel observed, no
             colour, the box of ``integrate_tsdf``'s defaults (center 0, half_extent 0.75).
    fill   : the colour of a vertex neither of whose voxels has a colour sample -- an INTERFACE default like those of ``integrate_tsdf``,
             tuned by nobody."""
    if isinstance(volume, TSDFVolume):
        tsdf, weight, color, cweight = volume.tsdf, volume.weight, volume.rgb, volume.cweight
        center, half_extent = volume.center, volume.half_extent
    elif torch.is_tensor(volume):
        tsdf, weight, color, cweight, center, half_extent = volume, None, None, None, (0.0, 0.0, 0.0), 0.75
    else:
        raise ValueError("volume must be a TSDFVolume or a (G, G, G) / (N, G, G, G) tensor")
    if tsdf.dim() not in (3, 4) or len(set(tsdf.shape[-3:])) != 1:
        raise ValueError(f"volume: tsdf of shape {tuple(tsdf.shape)}, need (G, G, G) or (N, G, G, G)")
    lead = tuple(tsdf.shape[:-3])
    N = lead[0] if lead else 1
    if N < 1:
        raise ValueError("volume: no scene")
    G, center, half_extent = _check_box(tsdf.shape[-1], center, half_extent, N)
    if weight is not None and tuple(weight.shape) != tuple(tsdf.shape):
        raise ValueError(f"volume: weight of shape {tuple(weight.shape)} for tsdf of shape {tuple(tsdf.shape)}")
    if (color is None) != (cweight is None):
        raise ValueError("volume: rgb and cweight go together")
    if color is not None and (tuple(color.shape) != tuple(tsdf.shape) + (3,) or tuple(cweight.shape) != tuple(tsdf.shape)):
        raise ValueError(f"volume: rgb of shape {tuple(color.shape)}, cweight of shape {tuple(cweight.shape)} for tsdf of shape {tuple(tsdf.shape)}")
    fill = tuple(float(v) for v in fill)
    if len(fill) != 3:
        raise ValueError(f"fill = {fill}: three floats")
    if tsdf.dim() == 3:
        tsdf, weight, color, cweight = (None if t is None else t[None] for t in (tsdf, weight, color, cweight))
    vertices, colors, faces, vertex_start, face_start = _march(tsdf, weight, color, cweight, N, G, center, half_extent, fill)
    return TriangleMesh(vertices=vertices, faces=faces, rgb=colors, vertex_start=vertex_start, face_start=face_start)


@dataclass
class RenderedMesh:
    """What ``render_mesh`` returns; the leading scene dimension is present only when a list of camera sets was passed."""
    rgb: Optional[torch.Tensor]              # (.., M, 3, P, P) fp32: the vertex colours interpolated perspective-correctly, or the background;
    #                                          None for a mesh without colour
    depth: torch.Tensor                      # (.., M, P, P) fp32: camera-space z of the surface, or empty_depth
    face: torch.Tensor                       # (.., M, P, P) int32: the face the pixel shows (its row in mesh.faces), or -1
    bary: torch.Tensor                       # (.., M, 3, P, P) fp32: perspective-correct barycentrics of that face's three vertices, or 0
    normal: torch.Tensor                     # (.., M, 3, P, P) fp32: the face's unit normal in camera space turned to normal_z <= 0, or 0
    hit: torch.Tensor                        # (.., M, P, P) bool: face >= 0

    _depth_map = (DEPTH_SCALE, DEPTH_SHIFT)  # depth_latent's defaults (not a field; ViewFusion.render_mesh binds the model's own per instance)

    def depth_latent(self, depth_scale=None, depth_shift=None):
        """The depth map in the model's depth-channel convention, exactly as ``RenderedViews.depth_latent`` forms it."""
        scale = self._depth_map[0] if depth_scale is None else depth_scale
        shift = self._depth_map[1] if depth_shift is None else depth_shift
        return _depth_latent(self.depth, self.hit, scale, shift)

    def shaded(self, background=(1.0, 1.0, 1.0)):
        """(.., M, 3, P, P): clamp(-normal_z, 0, 1) as grey where hit, the background elsewhere -- a headlight image, the way to look
        at a mesh without colour."""
        grey = torch.clamp(-self.normal[..., 2:3, :, :], 0.0, 1.0).expand(*self.normal.shape)
        bg = torch.tensor([float(v) for v in background], dtype=grey.dtype, device=grey.device).reshape(3, 1, 1).expand_as(grey)
        return torch.where(self.hit.unsqueeze(-3), grey, bg)


def _raster(vertices, colors, faces, vertex_start, face_start, cams, N, M, P, cull, znear, empty_depth, background):
    """The three enqueues of mvd_render_mesh.  vertices (n, 3), colors (n, 3) or None, faces (m, 3) int32, vertex_start / face_start
    (N + 1) int32, cams (N*M, CAM_RECORD), all contiguous on one GPU.  Returns (rgb or None, depth, face, bary, normal) of shapes
    (N*M, [3,] P, P).  No host synchronisation."""
    import ctypes
    L = hip.lib()
    dev, nvert, nface = vertices.device, int(vertices.shape[0]), int(faces.shape[0])
    hip._req(vertices), hip._req(cams), hip._req(faces, torch.int32), hip._req(vertex_start, torch.int32), hip._req(face_start, torch.int32)
    if colors is not None:
        hip._req(colors)
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    face = torch.empty(N * M, P, P, dtype=torch.int32, device=dev)
    depth, bary, normal = f32(N * M, P, P), f32(N * M, 3, P, P), f32(N * M, 3, P, P)
    rgb = f32(N * M, 3, P, P) if colors is not None else None
    nbytes = int(L.mvd_render_mesh_scratch(N * M, P))
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    bg = (ctypes.c_float * 3)(*background)
    if colors is not None and nvert == 0:
        colors = f32(1, 3)                   # (an empty mesh with colour: the library pairs a non-NULL colors with rgb; nothing reads it)
    hip.check(L.mvd_render_mesh(_p(vertices), hip.ptr(colors), _p(faces), hip.ptr(vertex_start), hip.ptr(face_start),
                                hip.ptr(cams), nvert, nface, N, M, P, int(cull), float(znear), float(empty_depth), bg, hip.ptr(face),
                                hip.ptr(depth), hip.ptr(bary), hip.ptr(normal), hip.ptr(rgb), hip.ptr(scratch), nbytes, hip.stream()))
    return rgb, depth, face, bary, normal


def _check_mesh(mesh):
    """The mesh checks of ``render_mesh`` -> (vertices, faces, rgb or None, scene count)."""
    if not isinstance(mesh, TriangleMesh):
        raise ValueError("mesh must be a TriangleMesh")
    vertices, faces, colors = mesh.vertices, mesh.faces, mesh.rgb
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"mesh: vertices of shape {tuple(vertices.shape)}, need (n, 3)")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"mesh: faces of shape {tuple(faces.shape)} and dtype {faces.dtype}, need (m, 3) int32")
    nvert, nface = int(vertices.shape[0]), int(faces.shape[0])
    if nface > 2 ** 31 - 1 or nvert > 2 ** 31 - 1:
        raise ValueError(f"mesh: {nface} faces of {nvert} vertices, the face and vertex indices are 31 bits")
    if colors is not None and tuple(colors.shape) != (nvert, 3):
        raise ValueError(f"mesh: rgb of shape {tuple(colors.shape)} for {nvert} vertices")
    scenes = int(mesh.vertex_start.numel()) - 1
    if scenes < 1 or mesh.vertex_start.dim() != 1 or tuple(mesh.face_start.shape) != (scenes + 1,):
        raise ValueError(f"mesh: vertex_start of shape {tuple(mesh.vertex_start.shape)}, face_start of shape {tuple(mesh.face_start.shape)}: "
                         "need (N + 1,) each, N >= 1")
    return vertices, faces, colors, scenes


def render_mesh(mesh, cameras, size=256, cull=True, background=(1.0, 1.0, 1.0), znear=1e-3, empty_depth=float("inf"), texture=None,
                filter="bilinear"):
    """Render a TriangleMesh into cameras by z-buffered rasterisation (include/mvd_hip.h: mvd_render_mesh has the rule) -> RenderedMesh.

    mesh    : a TriangleMesh of one or several scenes (what ``extract_mesh`` returns).
    cameras : M cameras (anything with .R .T .focal_length .principal_point): the mesh must be one scene's.  Or a list of N sets of M
              cameras each, N the mesh's scene count: scene s goes into set s, and the outputs get a leading dimension N.
    size    : P, the output side in pixels.  Per pixel centre the nearest face covering it with camera z > znear wins (ties: the lowest
              face id); depth, colour and barycentrics are interpolated perspective-correctly.
    cull    : drop back faces -- ``extract_mesh`` winds every triangle with its normal out of the surface.  A face with a vertex at or
              behind znear is dropped whole (no near-plane clipping).
    background, empty_depth : what a pixel no face covers holds in rgb / depth.
    texture : a MeshTexture of this mesh (``bake_texture``): rgb is then looked up in it through the face and the barycentrics of every
              pixel (mvd_texture_sample) with ``filter`` "bilinear" or "nearest", and the mesh need not carry colour.  With the default
              None the call is what it always was.
    Nothing is read back from the device; the mesh's two offset tables are copied to it."""
    vertices, faces, colors, scenes = _check_mesh(mesh)
    if texture is not None:
        _check_texture(texture, scenes, filter)
        colors = None
    if int(size) != size or size < 1:
        raise ValueError(f"size = {size}: an integer >= 1")
    P, znear = int(size), float(znear)
    if not znear >= 0:
        raise ValueError(f"znear = {znear}: >= 0")
    if cull not in (True, False, 0, 1):
        raise ValueError(f"cull = {cull}: True or False")
    background = tuple(float(v) for v in background)
    if len(background) != 3:
        raise ValueError(f"background = {background}: three floats")
    single = not isinstance(cameras, (list, tuple))
    sets = [_as_cameras(c) for c in ([cameras] if single else cameras)]
    N = len(sets)
    if N < 1:
        raise ValueError("cameras: an empty list")
    M = len(sets[0])
    if M < 1 or any(len(c) != M for c in sets):
        raise ValueError(f"cameras: every scene needs the same number M >= 1 of cameras, got {[len(c) for c in sets]}")
    if N != scenes:
        raise ValueError(f"cameras: {N} camera set(s) for a mesh of {scenes} scene(s)" + (" (pass a list of sets)" if single else ""))
    if N * M > 65535:
        raise ValueError(f"cameras: {N} x {M} cameras, at most 65535 per call")
    if N * M * P * P >= 2 ** 31:
        raise ValueError(f"size = {P}: {N * M * P * P} pixels for {N} x {M} cameras, the pixel index is 31 bits")
    dev = vertices.device
    vertices = vertices.float().contiguous()
    faces = faces.to(dev).contiguous()
    colors = None if colors is None else colors.to(dev, torch.float32).contiguous()
    vertex_start, face_start = (t.to(torch.int32).to(dev).contiguous() for t in (mesh.vertex_start, mesh.face_start))
    cams = Cameras(*(torch.cat([getattr(c, k) for c in sets]) for k in ("R", "T", "focal_length", "principal_point")))
    rgb, depth, face, bary, normal = _raster(vertices, colors, faces, vertex_start, face_start, pack_cameras(cams).to(dev).contiguous(), N, M,
                                             P, bool(cull), znear, empty_depth, background)
    if texture is not None:
        rgb = _sample(face, bary, face_start, texture, int(faces.shape[0]), N, M, P, TEX_FILTERS[filter], background)
    lead = (M,) if single else (N, M)
    face = face.reshape(*lead, P, P)
    return RenderedMesh(rgb=None if rgb is None else rgb.reshape(*lead, 3, P, P), depth=depth.reshape(*lead, P, P), face=face,
                        bary=bary.reshape(*lead, 3, P, P), normal=normal.reshape(*lead, 3, P, P), hit=face >= 0)


@dataclass
class NearestPoints:
    """What ``nearest_points`` returns, per query point."""
    index: torch.Tensor                      # (nq,) int32: the row of the nearest target, or -1 without one
    dist2: torch.Tensor                      # (nq,) fp32: the squared distance to it, or +inf

    @property
    def dist(self):
        return torch.sqrt(self.dist2)

    @property
    def hit(self):
        return self.index >= 0


@dataclass
class SurfaceSamples:
    """What ``sample_mesh`` returns: points on a mesh's surface, scene after scene; every field is a tensor on the mesh's device."""
    xyz: torch.Tensor                        # (n, 3) fp32 world coordinates
    rgb: Optional[torch.Tensor]              # (n, 3) fp32: the vertex colours mixed like xyz, or None without colour
    scene: torch.Tensor                      # (n,) int64, sorted
    face: torch.Tensor                       # (n,) int32: the row of mesh.faces the sample lies in
    bary: torch.Tensor                       # (n, 3) fp32: its barycentrics on that face's three vertices

    def __len__(self):
        return int(self.xyz.shape[0])


NN_METHODS = {"auto": hip.NN_AUTO, "brute": hip.NN_BRUTE, "grid": hip.NN_GRID}
COMPARE_SAMPLES = 65536                      # compare_geometry's default samples per scene of a mesh
_R2 = 1.32471795724474602596                 # the plastic constant: x^3 = x + 1


def sample_mesh(mesh, n):
    """``n`` points per scene on the surface of a TriangleMesh, by area and deterministically (no random numbers) -> SurfaceSamples.

    Sample k of a scene falls in the face whose interval of the scene's cumulative face area contains (k + 0.5) / n of the scene's
    area: a face of area a gets n a / A samples to within one.  Inside the face it sits at the k-th point of the R2 sequence (Roberts'
    additive recurrence on the plastic constant g: (0.5 + k / g, 0.5 + k / g^2) mod 1, formed in float64), folded into the triangle
    ((r1, r2) -> (1 - r1, 1 - r2) where r1 + r2 > 1) and read as the barycentrics (1 - r1 - r2, r1, r2) of the face's vertices.  xyz and
    rgb are that mix of the vertices and vertex colours.  Areas and the cumulative sum are float64; plain torch ops on the mesh's device
    (CPU tensors too).  A scene without faces, or whose area is zero or not finite, contributes no samples."""
    if not isinstance(mesh, TriangleMesh):
        raise ValueError("mesh must be a TriangleMesh")
    if isinstance(n, bool) or int(n) != n or not 1 <= n <= 2 ** 31 - 1:
        raise ValueError(f"n = {n}: an integer in [1, 2^31 - 1]")
    n = int(n)
    vertices, faces = mesh.vertices, mesh.faces
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"mesh: vertices of shape {tuple(vertices.shape)}, faces of shape {tuple(faces.shape)}, need (n, 3) and (m, 3)")
    if mesh.rgb is not None and tuple(mesh.rgb.shape) != tuple(vertices.shape):
        raise ValueError(f"mesh: rgb of shape {tuple(mesh.rgb.shape)} for {vertices.shape[0]} vertices")
    dev = vertices.device
    start = [int(v) for v in mesh.face_start.tolist()]
    if len(start) < 2 or start[0] < 0 or start[-1] > faces.shape[0] or any(a > b for a, b in zip(start, start[1:])):
        raise ValueError(f"mesh: face_start = {start} for {faces.shape[0]} faces")
    v64, f = vertices.double(), faces.long()
    tri = v64[f]                                                                         # (m, 3 vertices, 3)
    area = 0.5 * torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).norm(dim=1)
    k = torch.arange(n, dtype=torch.float64, device=dev)
    r1, r2 = torch.remainder(0.5 + k / _R2, 1.0), torch.remainder(0.5 + k / (_R2 * _R2), 1.0)
    fold = r1 + r2 > 1.0
    r1, r2 = torch.where(fold, 1.0 - r1, r1), torch.where(fold, 1.0 - r2, r2)
    b12 = torch.stack([r1, r2], dim=1).float()
    b0 = (1.0 - b12[:, 0].double() - b12[:, 1].double()).clamp(min=0.0).float()
    bary1 = torch.cat([b0[:, None], b12], dim=1)                                         # (n, 3): the same for every scene
    face, scene = [], []
    for s_, (f0, f1) in enumerate(zip(start, start[1:])):
        if f1 == f0:
            continue
        cs = torch.cumsum(area[f0:f1], dim=0)
        total = float(cs[-1])
        if not 0.0 < total < float("inf"):
            continue
        at = torch.searchsorted(cs, (k + 0.5) / n * cs[-1], right=True).clamp(max=f1 - f0 - 1)
        face.append(at + f0)
        scene.append(torch.full((n,), s_, dtype=torch.int64, device=dev))
    if face:
        face, scene = torch.cat(face), torch.cat(scene)
    else:
        face, scene = torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev)
    bary = bary1.repeat(face.shape[0] // n, 1)
    mix = lambda values: (bary.double()[:, :, None] * values.double()[f[face]]).sum(1).float()
    return SurfaceSamples(xyz=mix(vertices), rgb=None if mesh.rgb is None else mix(mesh.rgb.to(dev)), scene=scene, face=face.to(torch.int32),
                          bary=bary)


def _nearest(query, query_start, target, target_start, N, method, grid):
    """The enqueues of mvd_nearest_points.  query (nq, 3), target (nt, 3) fp32, query_start / target_start (N + 1) int32, all contiguous
    on one GPU.  Returns (index (nq,) int32, dist2 (nq,) fp32).  No host synchronisation."""
    L = hip.lib()
    dev, nq, nt = query.device, int(query.shape[0]), int(target.shape[0])
    hip._req(query), hip._req(target), hip._req(query_start, torch.int32), hip._req(target_start, torch.int32)
    index = torch.empty(nq, dtype=torch.int32, device=dev)
    dist2 = torch.empty(nq, dtype=torch.float32, device=dev)
    nbytes = int(L.mvd_nearest_points_scratch(nt, N, method, grid))
    scratch = _scratch(nbytes, dev)
    hip.check(L.mvd_nearest_points(_p(query), hip.ptr(query_start), _p(target), hip.ptr(target_start), nq, nt, N, method, grid, _p(index),
                                   _p(dist2), _p(scratch), nbytes, hip.stream()))
    return index, dist2


def _points_of(side, name, scenes):
    """(xyz (n, 3), sorted scene ids (n,) or None for one scene) of an argument of ``nearest_points``, checked."""
    if isinstance(side, TriangleMesh):
        raise ValueError(f"{name}: a TriangleMesh has no points to search -- pass sample_mesh(mesh, n), or use nearest_on_mesh for the "
                         f"distance to its triangles")
    if torch.is_tensor(side):
        xyz, scene = side, None
    elif hasattr(side, "xyz") and hasattr(side, "scene"):
        xyz, scene = side.xyz, side.scene
    else:
        raise ValueError(f"{name} must be an (n, 3) tensor, a PointCloud or SurfaceSamples")
    if not torch.is_tensor(xyz) or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{name}: xyz of shape {tuple(xyz.shape) if torch.is_tensor(xyz) else None}, need (n, 3)")
    n = int(xyz.shape[0])
    if n > 2 ** 31 - 1:
        raise ValueError(f"{name}: {n} points, the point index is 31 bits")
    if scene is not None and tuple(scene.shape) != (n,):
        raise ValueError(f"{name}: scene of shape {tuple(scene.shape)} for {n} points")
    if scene is not None and n and scene.device.type == "cpu" and not 0 <= int(scene.min()) <= int(scene.max()) < scenes:
        raise ValueError(f"{name}: scenes {int(scene.min())} .. {int(scene.max())} with scenes = {scenes}")
    return xyz, scene


def _scene_start(scene, n, N, dev):
    """(N + 1,) int32 offsets of sorted scene ids, formed on the device (``render_points`` does the same); one scene without ids."""
    if scene is None or n == 0:
        return torch.tensor([0] + [n] * N, dtype=torch.int32).to(dev)
    bounds = torch.arange(N + 1, dtype=scene.dtype, device=scene.device)
    return torch.searchsorted(scene.contiguous(), bounds).to(dev, torch.int32)


def _check_nn(scenes, method, grid):
    if isinstance(scenes, bool) or int(scenes) != scenes or not 1 <= scenes <= 65535:
        raise ValueError(f"scenes = {scenes}: an integer in [1, 65535]")
    if method not in NN_METHODS:
        raise ValueError(f"method = {method!r}: one of {sorted(NN_METHODS)}")
    if grid is not None and (isinstance(grid, bool) or int(grid) != grid or not 1 <= grid <= hip.NN_MAX_GRID):
        raise ValueError(f"grid = {grid}: None or an integer in [1, {hip.NN_MAX_GRID}]")
    return int(scenes), NN_METHODS[method], 0 if grid is None else int(grid)


def nearest_points(query, target, scenes=1, method="auto", grid=None):
    """For every point of ``query`` the exact nearest point of ``target`` (include/mvd_hip.h: mvd_nearest_points has the rule)
    -> NearestPoints.

    query, target : an (n, 3) tensor (one scene, scene 0), or anything with ``.xyz`` and a sorted ``.scene`` -- a PointCloud, or the
              SurfaceSamples of ``sample_mesh``.  A point searches the target points of its own scene only.  A TriangleMesh is refused.
    scenes  : N, the number of scenes both sides are split into (scene ids < N).
    method  : "brute" (every pair), "grid" (a uniform grid over the targets of each scene) or "auto" (the library chooses from the
              sizes).  All three return the same bits: the minimum squared distance in fp32, between equal minima the lowest row.
    grid    : cells per axis for "grid", 1 .. hip.NN_MAX_GRID; None leaves it to the library.
    ``index`` is a row of ``target`` (-1, with ``dist2`` = +inf, for a query without a candidate: no target in its scene, or a
    non-finite coordinate).  Nothing is read back from the device, so scene ids < N are checked only for ids in host memory; on the
    GPU a point of a scene >= N finds nothing and is found by nothing."""
    N, method, grid = _check_nn(scenes, method, grid)
    q, q_scene = _points_of(query, "query", N)
    t, t_scene = _points_of(target, "target", N)
    dev = q.device
    q, t = q.float().contiguous(), t.to(dev, torch.float32).contiguous()
    index, dist2 = _nearest(q, _scene_start(q_scene, int(q.shape[0]), N, dev), t, _scene_start(t_scene, int(t.shape[0]), N, dev), N, method, grid)
    return NearestPoints(index=index, dist2=dist2)


@dataclass
class NearestOnMesh:
    """What ``nearest_on_mesh`` returns, per query point: the closest point of the mesh's triangles."""
    face: torch.Tensor                       # (nq,) int32: the row of mesh.faces the closest point lies in, or -1 without one
    dist2: torch.Tensor                      # (nq,) fp32: the squared distance to it (formed in fp64, rounded once), or +inf
    point: torch.Tensor                      # (nq, 3) fp32: the closest point; NaN without one
    bary: torch.Tensor                       # (nq, 3) fp32: its barycentrics on that face's three vertices; 0 without one
    region: torch.Tensor                     # (nq,) int32: 0..2 a vertex of the face, 3..5 an edge (AB, BC, CA), 6 its interior; -1
    normal: torch.Tensor                     # (nq, 3) fp32: the face's unit normal (the winding decides the side); 0 for a degenerate face

    @property
    def dist(self):
        return torch.sqrt(self.dist2)

    @property
    def hit(self):
        return self.face >= 0

    def rgb(self, mesh):
        """(nq, 3) fp32: the vertex colours of ``mesh`` mixed by ``bary`` (float64, rounded once); NaN where nothing was found."""
        if not isinstance(mesh, TriangleMesh) or mesh.rgb is None:
            raise ValueError("rgb(mesh): a TriangleMesh with vertex colours")
        dev = self.face.device
        ids = mesh.faces.to(dev).long()[self.face.long().clamp(min=0)]                       # (nq, 3)
        mixed = (self.bary.double()[:, :, None] * mesh.rgb.to(dev).double()[ids]).sum(1).float()
        return torch.where(self.hit[:, None], mixed, torch.full_like(mixed, float("nan")))


def _mesh_arrays(mesh, N, dev):
    """(vertices (nv, 3) fp32, faces (nf, 3) int32, face_start (N + 1) int32) of a TriangleMesh, contiguous on ``dev``.  A mesh of fewer
    scenes than N has its remaining scenes empty; one of more is refused."""
    if not isinstance(mesh, TriangleMesh):
        raise ValueError("mesh must be a TriangleMesh")
    vertices, faces = mesh.vertices, mesh.faces
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"mesh: vertices of shape {tuple(vertices.shape)}, faces of shape {tuple(faces.shape)}, need (n, 3) and (m, 3)")
    start = [int(v) for v in mesh.face_start.tolist()]
    if len(start) < 2 or start[0] < 0 or start[-1] > faces.shape[0] or any(a > b for a, b in zip(start, start[1:])):
        raise ValueError(f"mesh: face_start = {start} for {faces.shape[0]} faces")
    if len(start) - 1 > N:
        raise ValueError(f"mesh: a mesh of {len(start) - 1} scenes with scenes = {N}")
    start = start + [start[-1]] * (N + 1 - len(start))
    return (vertices.to(dev, torch.float32).contiguous(), faces.to(dev, torch.int32).contiguous(),
            torch.tensor(start, dtype=torch.int32).to(dev))


def _nearest_on_mesh(query, query_start, vertices, faces, face_start, N, method, grid):
    """The enqueues of mvd_nearest_on_mesh, every output asked for -> NearestOnMesh.  No host synchronisation."""
    L = hip.lib()
    dev, nq, nv, nf = query.device, int(query.shape[0]), int(vertices.shape[0]), int(faces.shape[0])
    hip._req(query), hip._req(vertices), hip._req(faces, torch.int32), hip._req(query_start, torch.int32), hip._req(face_start, torch.int32)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    out = NearestOnMesh(face=i32(nq), dist2=f32(nq), point=f32(nq, 3), bary=f32(nq, 3), region=i32(nq), normal=f32(nq, 3))
    nbytes = int(L.mvd_nearest_on_mesh_scratch(nf, N, method, grid))
    scratch = _scratch(nbytes, dev)
    hip.check(L.mvd_nearest_on_mesh(_p(query), hip.ptr(query_start), _p(vertices), _p(faces), hip.ptr(face_start), nq, nv, nf, N, method, grid,
                                    _p(out.face), _p(out.dist2), _p(out.point), _p(out.bary), _p(out.region), _p(out.normal), _p(scratch),
                                    nbytes, hip.stream()))
    return out


def nearest_on_mesh(query, mesh, scenes=1, method="auto", grid=None):
    """For every point of ``query`` the exact closest point of the TRIANGLES of ``mesh`` (include/mvd_hip.h: mvd_nearest_on_mesh has the
    rule) -> NearestOnMesh.  Where ``nearest_points(query, sample_mesh(mesh, n))`` gives the distance to the nearest sample -- an upper
    bound with a floor of the sample spacing -- this is the distance to the surface: 0 for a point on it.

    query   : what ``nearest_points`` takes: an (n, 3) tensor (scene 0) or anything with ``.xyz`` and a sorted ``.scene``.
    mesh    : a TriangleMesh; a point searches the faces of its own scene only.  Its host ``face_start`` goes to the device.  A mesh of
              more scenes than ``scenes`` is refused.
    scenes, method, grid : as for ``nearest_points``; all three methods return the same bits.
    A face with an id outside the vertices or a non-finite coordinate is no candidate; a degenerate face (collinear or coincident
    vertices) is searched as its three segments and has a zero ``normal``.  Nothing is read back from the device."""
    N, method, grid = _check_nn(scenes, method, grid)
    q, q_scene = _points_of(query, "query", N)
    dev = q.device
    vertices, faces, face_start = _mesh_arrays(mesh, N, dev)
    q = q.float().contiguous()
    return _nearest_on_mesh(q, _scene_start(q_scene, int(q.shape[0]), N, dev), vertices, faces, face_start, N, method, grid)


WINDING_BETA = 2.0                           # Barill et al.'s accuracy parameter of the far field: an INTERFACE default, not swept here
WINDING_METHODS = {"auto": hip.WIND_AUTO, "exact": hip.WIND_EXACT, "cells": hip.WIND_CELLS}


@dataclass
class WindingNumber:
    """What ``winding_number`` returns, per query point."""
    value: torch.Tensor                      # (nq,) fp64: the generalized winding number; NaN for a non-finite query or one of no scene
    inside: torch.Tensor                     # (nq,) bool: value >= 0.5
    scene: torch.Tensor                      # (nq,) int64: the scene each query was tested against


@dataclass
class SignedDistance:
    """What ``signed_distance`` returns, per query point."""
    nearest: NearestOnMesh                   # ``nearest_on_mesh`` of the same query
    inside: torch.Tensor                     # (nq,) bool: ``winding_number`` of the same query
    distance: torch.Tensor                   # (nq,) fp32: sqrt(nearest.dist2), negated where inside


@dataclass
class OccupancyVolume:
    """What ``voxelize_mesh`` returns: ``occupied`` is (N, G, G, G) bool in z, y, x order over the box center +- half_extent; voxel
    (k, j, i) has its centre where ``TSDFVolume`` puts it, center - half_extent + (index + 0.5) * 2 * half_extent / G per axis."""
    occupied: torch.Tensor
    center: tuple
    half_extent: float


@dataclass
class VolumeIoU:
    """What ``volume_iou`` returns, per scene."""
    intersection: torch.Tensor               # (N,) int64: voxels both sides occupy
    union: torch.Tensor                      # (N,) int64: voxels either side occupies
    iou: torch.Tensor                        # (N,) fp64: intersection / union, NaN where union == 0


def _check_winding(scenes, method, cells, beta):
    if isinstance(scenes, bool) or int(scenes) != scenes or not 1 <= scenes <= 65535:
        raise ValueError(f"scenes = {scenes}: an integer in [1, 65535]")
    if method not in WINDING_METHODS:
        raise ValueError(f"method = {method!r}: one of {sorted(WINDING_METHODS)}")
    if cells is not None and (isinstance(cells, bool) or int(cells) != cells or not 1 <= cells <= hip.WIND_MAX_CELLS):
        raise ValueError(f"cells = {cells}: None or an integer in [1, {hip.WIND_MAX_CELLS}]")
    if cells is not None and int(scenes) * int(cells) ** 3 > hip.WIND_MAX_TABLE:
        raise ValueError(f"cells = {cells} for {scenes} scene(s): scenes * cells^3 <= 2^28")
    if isinstance(beta, bool) or not float(beta) >= 0.0:
        raise ValueError(f"beta = {beta}: >= 0 or inf")
    return int(scenes), WINDING_METHODS[method], 0 if cells is None else int(cells), float(beta)


def _winding(query, query_start, vertices, faces, face_start, N, method, cells, beta):
    """The enqueues of mvd_winding_number, both outputs -> (value (nq,) fp64, inside (nq,) uint8).  No host synchronisation."""
    L = hip.lib()
    dev, nq, nv, nf = query.device, int(query.shape[0]), int(vertices.shape[0]), int(faces.shape[0])
    hip._req(query), hip._req(vertices), hip._req(faces, torch.int32), hip._req(query_start, torch.int32), hip._req(face_start, torch.int32)
    value = torch.empty(nq, dtype=torch.float64, device=dev)
    inside = torch.empty(nq, dtype=torch.uint8, device=dev)
    nbytes = int(L.mvd_winding_scratch(nf, N, method, cells))
    scratch = _scratch(nbytes, dev)
    hip.check(L.mvd_winding_number(_p(query), hip.ptr(query_start), _p(vertices), _p(faces), hip.ptr(face_start), nq, nv, nf, N, method, cells,
                                   beta, _p(value), _p(inside), _p(scratch), nbytes, hip.stream()))
    return value, inside


def winding_number(query, mesh, scenes=1, method="auto", cells=None, beta=WINDING_BETA):
    """The generalized winding number of ``mesh`` at every point of ``query`` (include/mvd_hip.h: mvd_winding_number has the rule)
    -> WindingNumber.  1 inside a closed mesh whose normals point out (``extract_mesh`` winds them so), 0 outside, and a smooth value in
    between near the holes of an open or non-manifold mesh -- where a ray-parity test has no answer; ``inside`` is ``value >= 0.5``.

    query   : what ``nearest_points`` takes: an (n, 3) tensor (scene 0) or anything with ``.xyz`` and a sorted ``.scene``.
    mesh    : a TriangleMesh; a point sees the faces of its own scene only.  A mesh of more scenes than ``scenes`` is refused.
    method  : "exact" (every face, the sum in face order), "cells" (one level of cells with a dipole far field; near cells are summed
              exactly) or "auto" (the library chooses from the faces per scene).
    cells   : cells per axis for "cells", 1 .. hip.WIND_MAX_CELLS; None leaves it to the library.
    beta    : a cell is far when the query is further from its centre than beta times its radius; inf makes "cells" exact.  The
              default 2 is Barill et al.'s and, like the automatic method and cells, an INTERFACE default (DESIGN.md has the far field's
              error measured: about 2e-2 at beta = 2, 6e-3 at beta = 3, in the winding number).
    A face with an id outside the vertices, a non-finite coordinate or a zero normal contributes nothing.  Nothing is read back."""
    N, method, cells, beta = _check_winding(scenes, method, cells, beta)
    q, q_scene = _points_of(query, "query", N)
    dev = q.device
    vertices, faces, face_start = _mesh_arrays(mesh, N, dev)
    q = q.float().contiguous()
    value, inside = _winding(q, _scene_start(q_scene, int(q.shape[0]), N, dev), vertices, faces, face_start, N, method, cells, beta)
    scene = torch.zeros(int(q.shape[0]), dtype=torch.int64, device=dev) if q_scene is None else q_scene.to(dev, torch.int64)
    return WindingNumber(value=value, inside=inside.bool(), scene=scene)


def signed_distance(query, mesh, scenes=1, method="auto", grid=None, winding="auto", cells=None, beta=WINDING_BETA):
    """The signed distance of every point of ``query`` to ``mesh`` -> SignedDistance: ``nearest_on_mesh`` for the magnitude and
    ``winding_number`` for the sign (negative inside), combined in torch ops.  method, grid go to the search; winding, cells, beta to
    the inside test (its ``method``).  The magnitude is exact; the sign is that of the winding number, whatever holes the mesh has."""
    _check_winding(scenes, winding, cells, beta)
    near = nearest_on_mesh(query, mesh, scenes=scenes, method=method, grid=grid)
    inside = winding_number(query, mesh, scenes=scenes, method=winding, cells=cells, beta=beta).inside
    dist = near.dist
    return SignedDistance(nearest=near, inside=inside, distance=torch.where(inside, -dist, dist))


def _check_voxels(grid, center, half_extent, N):
    if isinstance(grid, bool) or int(grid) != grid or not 1 <= grid <= 1024 or N * int(grid) ** 3 > 2 ** 31 - 1:
        raise ValueError(f"grid = {grid} for {N} scene(s): an integer in [1, 1024] with scenes * grid^3 <= 2^31 - 1")
    center = tuple(float(v) for v in center)
    if len(center) != 3:
        raise ValueError(f"center = {center}: three floats")
    half_extent = float(half_extent)
    if not 0 < half_extent < float("inf"):
        raise ValueError(f"half_extent = {half_extent}: > 0")
    return int(grid), center, half_extent


def voxel_centres(grid, center=(0, 0, 0), half_extent=0.75):
    """(G^3, 3) fp32 on the host: the voxel centres of ``TSDFVolume``'s box in z, y, x order (x fastest), each coordinate formed in fp64
    as center - half_extent + (index + 0.5) * 2 * half_extent / G and rounded once."""
    G, center, half_extent = _check_voxels(grid, center, half_extent, 1)
    idx = torch.arange(G, dtype=torch.float64)
    axis = [c - half_extent + (idx + 0.5) * 2 * half_extent / G for c in center]
    zz, yy, xx = torch.meshgrid(axis[2], axis[1], axis[0], indexing="ij")
    return torch.stack([xx, yy, zz], dim=-1).reshape(-1, 3).float()


def voxelize_mesh(mesh, grid=128, center=(0, 0, 0), half_extent=0.75, method="auto", cells=None, beta=WINDING_BETA):
    """A TriangleMesh -> OccupancyVolume: ``winding_number(...).inside`` at every voxel centre of the box ``integrate_tsdf`` uses, every
    scene of the mesh against the same box.  grid: G voxels per side; method, cells, beta: those of ``winding_number``.  Nothing is
    read back from the device."""
    if not isinstance(mesh, TriangleMesh):
        raise ValueError("mesh must be a TriangleMesh")
    N = int(mesh.face_start.numel()) - 1
    if N < 1:
        raise ValueError("mesh: no scene")
    G, center, half_extent = _check_voxels(grid, center, half_extent, N)
    N, method, cells, beta = _check_winding(N, method, cells, beta)
    dev = mesh.vertices.device
    vertices, faces, face_start = _mesh_arrays(mesh, N, dev)
    q = voxel_centres(G, center, half_extent).to(dev).repeat(N, 1).contiguous()
    q_start = (torch.arange(N + 1, dtype=torch.int64) * G ** 3).to(torch.int32).to(dev)
    _, inside = _winding(q, q_start, vertices, faces, face_start, N, method, cells, beta)
    return OccupancyVolume(occupied=inside.bool().reshape(N, G, G, G), center=center, half_extent=half_extent)


def volume_iou(a, b, grid=128, center=(0, 0, 0), half_extent=0.75, method="auto", cells=None, beta=WINDING_BETA):
    """Volumetric intersection over union of two geometries per scene -> VolumeIoU.  Each side is a TriangleMesh, voxelised by
    ``voxelize_mesh``, or an OccupancyVolume.  A volume fixes the box: a mesh beside it is voxelised into the volume's grid, center and
    half_extent, two volumes must agree on them, and the arguments given here count only between two meshes.  The counts are integer
    sums, so the result is the same bits run to run.  Nothing is read back from the device."""
    sides = (a, b)
    if not all(isinstance(s, (TriangleMesh, OccupancyVolume)) for s in sides):
        raise ValueError("volume_iou: each side is a TriangleMesh or an OccupancyVolume")
    G, center, half_extent = _check_voxels(grid, center, half_extent, 1)
    boxes = [(int(s.occupied.shape[-1]), tuple(float(v) for v in s.center), float(s.half_extent)) for s in sides if isinstance(s, OccupancyVolume)]
    for s in sides:
        if isinstance(s, OccupancyVolume) and (s.occupied.dim() != 4 or len(set(s.occupied.shape[1:])) != 1 or s.occupied.dtype != torch.bool):
            raise ValueError(f"volume_iou: occupied of shape {tuple(s.occupied.shape)} and dtype {s.occupied.dtype}, need (N, G, G, G) bool")
    if boxes:
        if any(box != boxes[0] for box in boxes):
            raise ValueError(f"volume_iou: two volumes of different boxes, {boxes[0]} and {boxes[1]}")
        G, center, half_extent = boxes[0]
    vols = [s if isinstance(s, OccupancyVolume) else voxelize_mesh(s, G, center, half_extent, method, cells, beta) for s in sides]
    x, y = vols[0].occupied, vols[1].occupied.to(vols[0].occupied.device)
    if x.shape != y.shape:
        raise ValueError(f"volume_iou: {x.shape[0]} and {y.shape[0]} scene(s)")
    inter = (x & y).flatten(1).sum(1, dtype=torch.int64)
    union = (x | y).flatten(1).sum(1, dtype=torch.int64)
    iou = torch.where(union > 0, inter.double() / union.clamp(min=1).double(), torch.full_like(inter, float("nan"), dtype=torch.float64))
    return VolumeIoU(intersection=inter, union=union, iou=iou)


@dataclass
class NeighbourPoints:
    """What ``knn_points`` returns, per query point: its k nearest targets in ascending (dist2, row) order."""
    index: torch.Tensor                      # (nq, k) int32: rows of the target, -1 in the slots behind the last neighbour found
    dist2: torch.Tensor                      # (nq, k) fp32: their squared distances, +inf in those slots

    @property
    def dist(self):
        return torch.sqrt(self.dist2)

    @property
    def hit(self):
        return self.index >= 0

    @property
    def count(self):
        """(nq,) int64: the filled slots of every row."""
        return (self.index >= 0).sum(dim=1)


def _knn(query, query_start, target, target_start, N, k, method, grid):
    """The enqueues of mvd_knn_points: ``_nearest`` with (nq, k) outputs.  No host synchronisation."""
    L = hip.lib()
    dev, nq, nt = query.device, int(query.shape[0]), int(target.shape[0])
    hip._req(query), hip._req(target), hip._req(query_start, torch.int32), hip._req(target_start, torch.int32)
    index = torch.empty(nq, k, dtype=torch.int32, device=dev)
    dist2 = torch.empty(nq, k, dtype=torch.float32, device=dev)
    nbytes = int(L.mvd_nearest_points_scratch(nt, N, method, grid))
    scratch = _scratch(nbytes, dev)
    hip.check(L.mvd_knn_points(_p(query), hip.ptr(query_start), _p(target), hip.ptr(target_start), nq, nt, N, k, method, grid, _p(index),
                               _p(dist2), _p(scratch), nbytes, hip.stream()))
    return index, dist2


def _check_k(k, most, what):
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= most:
        raise ValueError(f"k = {k}: an integer in [1, {most}] ({what})")
    return int(k)


def knn_points(query, target, k, scenes=1, method="auto", grid=None):
    """For every point of ``query`` its ``k`` nearest points of ``target`` (include/mvd_hip.h: mvd_knn_points has the rule)
    -> NeighbourPoints.

    query, target, scenes, method, grid : those of ``nearest_points``, with the same checks.
    k       : 1 .. hip.KNN_MAX_K neighbours per query.  k = 1 gives the bits of ``nearest_points`` (as (nq, 1) tensors).
    A row holds the candidates in ascending order of (squared distance in fp32, target row) -- the same bits for every method and from
    run to run -- and -1 / +inf behind the last one when the query's scene holds fewer than k finite targets.
    ``query`` may be ``target``: a point is then its own neighbour at distance 0 and STAYS in its list (slot 0, unless a coincident
    point of a lower row comes first).  There is no exclude flag; ask for k + 1 and drop the first column where that is wanted.
    Nothing is read back from the device."""
    N, method, grid = _check_nn(scenes, method, grid)
    k = _check_k(k, hip.KNN_MAX_K, "hip.KNN_MAX_K")
    q, q_scene = _points_of(query, "query", N)
    t, t_scene = _points_of(target, "target", N)
    dev = q.device
    q, t = q.float().contiguous(), t.to(dev, torch.float32).contiguous()
    index, dist2 = _knn(q, _scene_start(q_scene, int(q.shape[0]), N, dev), t, _scene_start(t_scene, int(t.shape[0]), N, dev), N, k, method, grid)
    return NeighbourPoints(index=index, dist2=dist2)


NORMALS_K = 16                               # estimate_normals' default neighbourhood (an INTERFACE default, see its docstring)


@dataclass
class PointNormals:
    """What ``estimate_normals`` returns, per point."""
    normal: torch.Tensor                     # (n, 3) fp32 unit normals; (0, 0, 0) where the point is not valid
    variation: torch.Tensor                  # (n,) fp32: l0 / (l0 + l1 + l2) of the neighbourhood's covariance, 0 on a plane; NaN where not valid
    valid: torch.Tensor                      # (n,) bool: at least three usable neighbours, neither coincident nor collinear
    neighbours: NeighbourPoints              # the lists the normals were formed from


def _normals(target, index, points, toward):
    """The enqueue of mvd_point_normals.  target (nt, 3) fp32, index (n, k) int32, points / toward (n, 3) fp32 or None, contiguous on
    one GPU.  Returns (normal (n, 3), variation (n,)).  No host synchronisation."""
    L = hip.lib()
    n, k = int(index.shape[0]), int(index.shape[1])
    hip._req(target), hip._req(index, torch.int32)
    if toward is not None:
        hip._req(points), hip._req(toward)
    normal = torch.empty(n, 3, dtype=torch.float32, device=target.device)
    variation = torch.empty(n, dtype=torch.float32, device=target.device)
    hip.check(L.mvd_point_normals(_p(target), int(target.shape[0]), _p(index), n, k, _p(points) if toward is not None else None, _p(toward),
                                  _p(normal), _p(variation), hip.stream()))
    return normal, variation


def estimate_normals(points, k=NORMALS_K, scenes=1, toward=None, neighbours=None, method="auto", grid=None):
    """A unit normal per point of a cloud from its ``k`` nearest neighbours within the cloud (include/mvd_hip.h: mvd_point_normals has
    the rule) -> PointNormals.

    points  : what ``nearest_points`` takes.  Every point's neighbourhood is ``knn_points(points, points, k)``: the point itself and
              its k - 1 nearest others of its scene.
    k       : 3 .. hip.KNN_MAX_K.  The default 16 is an interface default that nobody has tuned: small k follows noise, large k rounds
              edges off; choose it for the data.
    toward  : None -- the sign makes the component of largest magnitude positive (between equal magnitudes the lowest axis), which is
              deterministic and means nothing; or an (N, 3) viewpoint per scene, or an (n, 3) tensor with a viewpoint per point -- the
              normal then faces it (normal . (toward - point) >= 0).  With n == N rows the tensor is read per scene.  There is no
              orientation propagation across the cloud.
    neighbours : a NeighbourPoints of ``points`` against itself to reuse (any k up to hip.NORMALS_MAX_K columns); k, method and grid
              are then unused.
    The normal is the eigenvector of the smallest eigenvalue of the neighbourhood's covariance, all in fp64, rounded to fp32 once;
    ``variation`` is that eigenvalue over the sum of the three.  A point with fewer than three usable neighbours, or whose neighbours
    coincide or are collinear, is not ``valid``: zero normal, NaN variation.  Nothing is read back from the device."""
    N, method, grid = _check_nn(scenes, method, grid)
    x, scene = _points_of(points, "points", N)
    dev, n = x.device, int(x.shape[0])
    x = x.float().contiguous()
    if toward is not None and (not torch.is_tensor(toward) or toward.dim() != 2 or toward.shape[1] != 3 or int(toward.shape[0]) not in (N, n)):
        raise ValueError(f"toward: None, an (N = {N}, 3) or an (n = {n}, 3) tensor")
    if neighbours is None:
        k = _check_k(k, hip.KNN_MAX_K, "hip.KNN_MAX_K")
        if k < 3:
            raise ValueError(f"k = {k}: a normal needs at least 3 neighbours")
        start = _scene_start(scene, n, N, dev)
        neighbours = NeighbourPoints(*_knn(x, start, x, start, N, k, method, grid))
    elif not isinstance(neighbours, NeighbourPoints) or neighbours.index.dim() != 2 or int(neighbours.index.shape[0]) != n or \
            not 1 <= int(neighbours.index.shape[1]) <= hip.NORMALS_MAX_K or neighbours.index.dtype != torch.int32:
        raise ValueError(f"neighbours: a NeighbourPoints with an (n = {n}, k <= {hip.NORMALS_MAX_K}) int32 index")
    if toward is not None:
        toward = toward.to(dev, torch.float32)
        if int(toward.shape[0]) == N:
            toward = toward[scene.to(dev).long()] if scene is not None else toward[:1].expand(n, 3)
        toward = toward.contiguous()
    normal, variation = _normals(x, neighbours.index.to(dev).contiguous(), x, toward)
    return PointNormals(normal=normal, variation=variation, valid=~torch.isnan(variation), neighbours=neighbours)


def sample_normals(mesh, samples):
    """(n, 3) fp32 unit normals of the faces the ``samples`` of ``sample_mesh(mesh, n)`` lie in (``samples.face``): the cross product
    (v1 - v0) x (v2 - v0) in float64 torch ops, divided by its length, so the winding of the mesh decides the side; zero for a face of
    zero or non-finite area.  A mesh target gets exact normals this way, without a search."""
    if not isinstance(mesh, TriangleMesh) or not isinstance(samples, SurfaceSamples):
        raise ValueError("sample_normals(mesh, samples): a TriangleMesh and the SurfaceSamples of sample_mesh")
    face = samples.face.long()
    nf = int(mesh.faces.shape[0])
    if face.numel() and face.device.type == "cpu" and not 0 <= int(face.min()) <= int(face.max()) < nf:
        raise ValueError(f"samples.face: rows {int(face.min())} .. {int(face.max())} of a mesh with {nf} faces")
    tri = mesh.vertices.double()[mesh.faces.long()[face.to(mesh.faces.device)]]          # (n, 3 vertices, 3)
    cross = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    length = cross.norm(dim=1, keepdim=True)
    ok = (length > 0) & torch.isfinite(length)
    return torch.where(ok, cross / torch.where(ok, length, torch.ones_like(length)), torch.zeros_like(cross)).float()


@dataclass
class GeometryDistance:
    """What ``compare_geometry`` returns.  The metrics are (N,) float64 tensors, one value per scene, NaN for a scene with an empty side."""
    a_to_b: NearestPoints                    # for every point of a its nearest point of b (a NearestOnMesh where exact=True met a mesh)
    b_to_a: NearestPoints
    accuracy: torch.Tensor                   # mean distance from a to b
    completeness: torch.Tensor               # mean distance from b to a
    chamfer: torch.Tensor                    # accuracy + completeness
    chamfer_sq: torch.Tensor                 # mean squared distance a to b + mean squared distance b to a
    precision: torch.Tensor                  # the share of a within `threshold` of b
    recall: torch.Tensor                     # the share of b within `threshold` of a
    fscore: torch.Tensor                     # 2 P R / (P + R), 0 when P + R == 0


def geometry_metrics(a_dist2, a_scene, b_dist2, b_scene, scenes, threshold):
    """The arithmetic of ``compare_geometry``: squared nearest distances of the two directions with their sorted scene ids (None: all
    scene 0) -> dict of the seven (N,) float64 metrics of GeometryDistance.  Every scene is reduced on its own slice by torch.sum --
    no float atomics, no index_add_: the same bits run to run.  One host read, of the scene offsets."""
    N = int(scenes)
    dev = a_dist2.device
    starts = torch.stack([_scene_start(a_scene, int(a_dist2.shape[0]), N, dev), _scene_start(b_scene, int(b_dist2.shape[0]), N, dev)]).tolist()
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    rows = {k: [] for k in ("accuracy", "completeness", "chamfer_sq", "precision", "recall")}
    for s in range(N):
        sides = []
        for d2, st in ((a_dist2, starts[0]), (b_dist2, starts[1])):
            part = d2[st[s]:st[s + 1]].double()
            sides.append((part, part.sqrt(), max(st[s + 1] - st[s], 0)))
        if min(c for _, _, c in sides) == 0:
            for k in rows:
                rows[k].append(nan)
            continue
        (a2, a1, na), (b2, b1, nb) = sides
        rows["accuracy"].append(a1.sum() / na)
        rows["completeness"].append(b1.sum() / nb)
        rows["chamfer_sq"].append(a2.sum() / na + b2.sum() / nb)
        rows["precision"].append((a1 <= threshold).sum().double() / na)
        rows["recall"].append((b1 <= threshold).sum().double() / nb)
    out = {k: torch.stack(v) for k, v in rows.items()}
    out["chamfer"] = out["accuracy"] + out["completeness"]
    pr = out["precision"] + out["recall"]
    out["fscore"] = torch.where(pr == 0, torch.zeros_like(pr), 2.0 * out["precision"] * out["recall"] / pr)
    return out


def compare_geometry(a, b, threshold=0.02, scenes=1, samples=None, method="auto", exact=False):
    """Distances between two geometries, scene by scene -> GeometryDistance: accuracy (mean distance from a to b), completeness (from
    b to a), their sum the Chamfer distance, its squared form, and precision / recall / F-score at ``threshold``.  With a the
    reconstruction and b the ground truth these are the usual names; any two clouds, rigs or settings can be compared.

    a, b    : what ``nearest_points`` takes, or a TriangleMesh, which is first turned into ``sample_mesh(mesh, samples)``;
              ``samples`` defaults to COMPARE_SAMPLES = 65536 per scene.
    threshold : in world units, the distance up to which a point counts as matched.  An INTERFACE default: no trained checkpoint was
              available when this was written, so nobody has tuned it on real samples -- expect to.
    scenes, method : as for ``nearest_points``.
    exact   : False -- the distance TO a mesh is the distance to its nearest sample: an upper bound with a floor of about the sample
              spacing, which moves with ``samples``.  True -- the distance to a side that is a TriangleMesh is ``nearest_on_mesh`` to
              its triangles (0 for a point on it, independent of ``samples``), and ``a_to_b`` / ``b_to_a`` are then NearestOnMesh; the
              points taken FROM that side are still its samples.  A side that is not a mesh is searched as before.
    The only host synchronisation is the read of the scene offsets (and, for a mesh, the per-scene areas in ``sample_mesh``)."""
    N, _, _ = _check_nn(scenes, method, None)
    threshold = float(threshold)
    if not threshold >= 0:
        raise ValueError(f"threshold = {threshold}: >= 0")
    if samples is not None and (isinstance(samples, bool) or int(samples) != samples or samples < 1):
        raise ValueError(f"samples = {samples}: None or an integer >= 1")
    sides, meshes = [], []
    for name, side in (("a", a), ("b", b)):
        meshes.append(side if exact and isinstance(side, TriangleMesh) else None)
        if isinstance(side, TriangleMesh):
            if int(side.face_start.numel()) - 1 > N:
                raise ValueError(f"{name}: a mesh of {int(side.face_start.numel()) - 1} scenes with scenes = {N}")
            side = sample_mesh(side, COMPARE_SAMPLES if samples is None else int(samples))
        _points_of(side, name, N)
        sides.append(side)
    to = lambda source, target, mesh: (nearest_points(source, target, scenes=N, method=method) if mesh is None else
                                       nearest_on_mesh(source, mesh, scenes=N, method=method))
    ab = to(sides[0], sides[1], meshes[1])
    ba = to(sides[1], sides[0], meshes[0])
    scene_of = lambda side: None if torch.is_tensor(side) else side.scene
    m = geometry_metrics(ab.dist2, scene_of(sides[0]), ba.dist2, scene_of(sides[1]), N, threshold)
    return GeometryDistance(a_to_b=ab, b_to_a=ba, **m)


# ------------------------------------------------------------------------------------------------ alignment
ALIGN_ITERS = 30                             # align_geometry's default iteration count (an INTERFACE default, see its docstring)


def _align_apply(xyz, start, N, transform):
    """The enqueue of mvd_align_apply: xyz (n, 3) fp32, start (N + 1) int32, transform (N, 12) float64, contiguous on one GPU
    -> moved (n, 3) fp32.  No host synchronisation."""
    L = hip.lib()
    n = int(xyz.shape[0])
    hip._req(xyz), hip._req(start, torch.int32), hip._req(transform, torch.float64)
    out = torch.empty_like(xyz)
    hip.check(L.mvd_align_apply(_p(xyz), hip.ptr(start), n, N, hip.ptr(transform), _p(out), hip.stream()))
    return out


def _ptrs(arrays):
    """``_p`` of each of the fp32 / int32 tensors an entry takes side by side, checked as ``hip._req`` checks one."""
    for t in arrays:
        hip._req(t, torch.float32 if t.is_floating_point() else torch.int32)
    return [_p(t) for t in arrays]


def _fit(entry, scratch_entry, history_width, moved, start, target_args, index, N, flags, max_d2, transform):
    """The enqueues of one fit entry of the library (mvd_align_fit, mvd_plane_fit) on the given pairing: index (n,) int32, or None for
    row i with row i; d2 is formed by the kernel.  target_args: the target-side tensors in the entry's order -- (target,) or (target,
    normals), (nt, 3) fp32.  transform (N, 12) float64 is composed in place unless flags has the entry's NO_STEP.  Returns the history
    row (N, history_width) float64."""
    L = hip.lib()
    dev, n, nt = moved.device, int(moved.shape[0]), int(target_args[0].shape[0])
    hip._req(moved), hip._req(start, torch.int32), hip._req(transform, torch.float64)
    if index is not None:
        hip._req(index, torch.int32)
    row = torch.empty(N, history_width, dtype=torch.float64, device=dev)
    nbytes = int(getattr(L, scratch_entry)(n, 0, N, hip.NN_BRUTE, 0))
    scratch = _scratch(nbytes, dev)
    hip.check(getattr(L, entry)(_p(moved), hip.ptr(start), *_ptrs(target_args), _p(index), None, n, nt, N, flags, max_d2, hip.ptr(transform),
                                hip.ptr(row), hip.ptr(scratch), nbytes, hip.stream()))
    return row


def _icp(entry, scratch_entry, history_width, source, source_start, target_args, target_sizes, N, method, grid, iters, flags, max_d2, transform,
         extra_outputs=()):
    """The enqueues of one ICP entry of the library (mvd_align_icp, mvd_plane_icp, mvd_mesh_icp).  target_args: the target-side tensors
    in the entry's order; target_sizes: their row counts as the entry takes them, the last being the one its scratch entry counts;
    flags: None for an entry without them; extra_outputs: (n, 3) fp32 outputs behind dist2.  transform (N, 12) float64 holds the start
    and is overwritten with the result.  Returns (history (iters + 1, N, history_width) float64, moved (n, 3) fp32, index (n,) int32,
    dist2 (n,) fp32).  No host synchronisation."""
    L = hip.lib()
    dev, nq = source.device, int(source.shape[0])
    hip._req(source), hip._req(source_start, torch.int32), hip._req(transform, torch.float64)
    history = torch.empty(iters + 1, N, history_width, dtype=torch.float64, device=dev)
    moved = torch.empty_like(source)
    index = torch.empty(nq, dtype=torch.int32, device=dev)
    dist2 = torch.empty(nq, dtype=torch.float32, device=dev)
    nbytes = int(getattr(L, scratch_entry)(nq, target_sizes[-1], N, method, grid))
    scratch = _scratch(nbytes, dev)
    hip.check(getattr(L, entry)(_p(source), hip.ptr(source_start), *_ptrs(target_args), nq, *target_sizes, N, method, grid, iters,
                                *(() if flags is None else (flags,)), max_d2, hip.ptr(transform), hip.ptr(history), _p(moved), _p(index),
                                _p(dist2), *_ptrs(extra_outputs), hip.ptr(scratch), nbytes, hip.stream()))
    return history, moved, index, dist2


# The entries by name: what the aligners call (and what a test or a benchmark replaces or times on its own).
def _align_fit(moved, start, target, index, N, flags, max_d2, transform):
    return _fit("mvd_align_fit", "mvd_align_scratch", hip.ALIGN_HISTORY, moved, start, (target,), index, N, flags, max_d2, transform)


def _plane_fit(moved, start, target, normals, index, N, flags, max_d2, transform):
    return _fit("mvd_plane_fit", "mvd_plane_scratch", hip.PLANE_HISTORY, moved, start, (target, normals), index, N, flags, max_d2, transform)


def _align_icp(source, source_start, target, target_start, N, method, grid, iters, flags, max_d2, transform):
    return _icp("mvd_align_icp", "mvd_align_scratch", hip.ALIGN_HISTORY, source, source_start, (target, target_start), (int(target.shape[0]),), N,
                method, grid, iters, flags, max_d2, transform)


def _plane_icp(source, source_start, target, target_start, normals, N, method, grid, iters, max_d2, transform):
    return _icp("mvd_plane_icp", "mvd_plane_scratch", hip.PLANE_HISTORY, source, source_start, (target, target_start, normals),
                (int(target.shape[0]),), N, method, grid, iters, None, max_d2, transform)


def _mesh_icp(source, source_start, vertices, faces, face_start, N, method, grid, iters, max_d2, transform):
    """(history, moved, face, dist2): the loop's point and normal outputs are scratch to the caller."""
    return _icp("mvd_mesh_icp", "mvd_mesh_icp_scratch", hip.PLANE_HISTORY, source, source_start, (vertices, faces, face_start),
                (int(vertices.shape[0]), int(faces.shape[0])), N, method, grid, iters, None, max_d2, transform,
                extra_outputs=(torch.empty_like(source), torch.empty_like(source)))


@dataclass
class Alignment:
    """What ``fit_similarity`` and ``align_geometry`` return: per scene the similarity x -> s R x + t that takes the source into the
    target's frame.  Every field is a tensor on the source's device."""
    matrix: torch.Tensor                     # (N, 4, 4) float64: [[s R, t], [0, 1]]
    rotation: torch.Tensor                   # (N, 3, 3) float64, proper (det = +1)
    translation: torch.Tensor                # (N, 3) float64
    scale: torch.Tensor                      # (N,) float64 (1 exactly when no scale was fitted or given)
    rms: torch.Tensor                        # (iters + 1, N) float64: RMS distance of the accepted pairs BEFORE step k; last row: under
    #                                          the returned transform.  NaN for a scene without an accepted pair
    pairs: torch.Tensor                      # (iters + 1, N) int64: accepted pairs, same rows
    xyz: torch.Tensor                        # (n, 3) fp32: the source points under the returned transform
    nearest: NearestPoints                   # of `xyz` against the target (the final correspondences)

    def apply(self, geometry):
        """``geometry`` with its coordinates moved by this alignment (include/mvd_hip.h: mvd_align_apply has the rule), as the same
        type through ``dataclasses.replace``: an (n, 3) tensor (scene 0; only when the alignment has one scene), a PointCloud,
        SurfaceSamples or a TriangleMesh.  Colours, faces and offsets are the objects they were.  No host synchronisation."""
        import dataclasses
        N = int(self.matrix.shape[0])
        if torch.is_tensor(geometry):
            if N != 1:
                raise ValueError(f"geometry: a bare tensor is scene 0, the alignment has {N} scenes -- pass a PointCloud or SurfaceSamples")
            if geometry.dim() != 2 or geometry.shape[1] != 3:
                raise ValueError(f"geometry: shape {tuple(geometry.shape)}, need (n, 3)")
            xyz, scene, key, start = geometry, None, None, None
        elif isinstance(geometry, TriangleMesh):
            if int(geometry.vertex_start.numel()) - 1 != N:
                raise ValueError(f"geometry: a mesh of {int(geometry.vertex_start.numel()) - 1} scene(s), the alignment has {N}")
            xyz, scene, key, start = geometry.vertices, None, "vertices", geometry.vertex_start
        elif hasattr(geometry, "xyz") and hasattr(geometry, "scene"):
            xyz, scene = _points_of(geometry, "geometry", N)
            key, start = "xyz", None
        else:
            raise ValueError("geometry must be an (n, 3) tensor, a PointCloud, SurfaceSamples or a TriangleMesh")
        dev = xyz.device
        start = _scene_start(scene, int(xyz.shape[0]), N, dev) if start is None else start.to(dev, torch.int32).contiguous()
        moved = _align_apply(xyz.float().contiguous(), start, N, self.matrix[:, :3, :].to(dev, torch.float64).reshape(N, 12).contiguous())
        return moved if key is None else dataclasses.replace(geometry, **{key: moved})


def _alignment(transform, scale, history, xyz, index, dist2):
    N = int(transform.shape[0])
    m34 = transform.reshape(N, 3, 4)
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64, device=transform.device).expand(N, 1, 4)
    return Alignment(matrix=torch.cat([m34, bottom], dim=1), rotation=m34[:, :, :3] / scale[:, None, None], translation=m34[:, :, 3].clone(),
                     scale=scale, rms=history[:, :, 0].clone(), pairs=history[:, :, 1].to(torch.int64), xyz=xyz,
                     nearest=NearestPoints(index=index, dist2=dist2))


def _identity_transform(N, dev):
    return torch.eye(3, 4, dtype=torch.float64, device=dev).reshape(1, 12).repeat(N, 1)


def _fl32_square(v):
    """fl32(fl32(v)^2) as a Python float: the threshold the kernel compares fp32 distances with."""
    import struct
    f32 = lambda x: struct.unpack("f", struct.pack("f", x))[0]
    try:
        return f32(f32(v) * f32(v))
    except OverflowError:
        return float("inf")


def _check_icp(iters, max_distance, scale=False):
    """(iters as an int, max_d2) of the arguments the ICP functions share, checked in the order iters, scale, max_distance."""
    iters = _check_count(iters, "iters", 0, hip.ALIGN_MAX_ITERS)
    if not isinstance(scale, bool):
        raise ValueError(f"scale = {scale!r}: True or False")
    return iters, _max_d2(max_distance)


def _max_d2(max_distance):
    """The gate as the kernel compares it: fl32(max_distance)^2, +inf for None."""
    if max_distance is not None and not float(max_distance) >= 0:
        raise ValueError(f"max_distance = {max_distance}: None or a distance >= 0")
    return float("inf") if max_distance is None else _fl32_square(float(max_distance))


def _check_pairs(pairs, n, nt):
    if pairs is None:
        if n != nt:
            raise ValueError(f"target: {nt} points for {n} of source -- row i goes with row i; give pairs otherwise")
    elif not torch.is_tensor(pairs) or tuple(pairs.shape) != (n,) or pairs.dtype != torch.int32:
        raise ValueError(f"pairs: an ({n},) int32 tensor, one target row (or -1) per source row")


def _given_pairs(moved, start, target, index, nt, N):
    """(index, dist2) of a GIVEN pairing as a search would report it: -1 / +inf for a skipped row."""
    rows = torch.arange(int(moved.shape[0]), dtype=torch.int32, device=moved.device)
    j = rows if index is None else index
    has = (j >= 0) & (j < nt) & (rows >= start[0]) & (rows < start[N])
    d = moved - target[j.long().clamp(0, max(nt - 1, 0))] if nt else torch.full_like(moved, float("nan"))
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]          # (the search's order: every torch op rounds once)
    has = has & (d2 < float("inf"))
    return torch.where(has, j, torch.full_like(j, -1)), torch.where(has, d2, torch.full_like(d2, float("inf")))


def fit_similarity(source, target, scenes=1, scale=True, pairs=None):
    """The similarity (rigid with ``scale=False``) that best takes ``source`` onto ``target`` in the least-squares sense, for KNOWN
    correspondences, in closed form (Horn's quaternion solve; include/mvd_hip.h: mvd_align_fit has the rule) -> Alignment.

    source, target : what ``nearest_points`` takes.  Row i of source goes with row i of target -- both sides then have equal lengths,
              and the target's scene offsets are TAKEN to be the source's: its own scene ids are not looked at (comparing the two
              would be a host read) -- or, with ``pairs`` an (n,) int32 tensor, with row pairs[i] of target; -1 skips the row.  A
              pair with a non-finite coordinate is skipped.
    scenes  : N; every scene gets its own transform from its own rows.
    A scene with fewer than 3 pairs, or whose source points coincide, gets the identity.  ``rms`` and ``pairs`` have one row: under
    the fit.  ``nearest`` holds the given pairing and its squared distances under the fit (-1 / +inf for a skipped row).  Nothing is
    read back from the device."""
    N, _, _ = _check_nn(scenes, "auto", None)
    if not isinstance(scale, bool):
        raise ValueError(f"scale = {scale!r}: True or False")
    s, s_scene = _points_of(source, "source", N)
    t, t_scene = _points_of(target, "target", N)
    dev, n, nt = s.device, int(s.shape[0]), int(t.shape[0])
    _check_pairs(pairs, n, nt)
    s, t = s.float().contiguous(), t.to(dev, torch.float32).contiguous()
    start = _scene_start(s_scene, n, N, dev)
    index = None if pairs is None else pairs.to(dev).contiguous()
    flags = hip.ALIGN_SCALE if scale else 0
    transform = _identity_transform(N, dev)
    first = _align_fit(s, start, t, index, N, flags, float("inf"), transform)
    moved = _align_apply(s, start, N, transform)
    last = _align_fit(moved, start, t, index, N, flags | hip.ALIGN_NO_STEP, float("inf"), transform)
    return _alignment(transform, first[:, 2].clone(), last[None], moved, *_given_pairs(moved, start, t, index, nt, N))


def _centroid_init(s, s_start, t, t_start, N, scale):
    """(N, 12) float64: per scene the map of the source's centroid onto the target's, with ``scale`` also of the RMS radius.  float64
    torch ops on each scene's slice (finite rows only); the identity for a scene with an empty side.  Reads the scene offsets once."""
    starts = torch.stack([s_start, t_start]).tolist()
    dev = s.device
    out = []
    for k in range(N):
        stats = []
        for pts, st in ((s, starts[0]), (t, starts[1])):
            part = pts[st[k]:st[k + 1]].double()
            fin = torch.isfinite(part).all(1, keepdim=True)
            cnt = fin.sum().double()
            c = torch.where(fin, part, torch.zeros_like(part)).sum(0) / cnt
            r2 = torch.where(fin, (part - c) ** 2, torch.zeros_like(part)).sum() / cnt
            stats.append((cnt, c, r2))
        (na, ca, ra), (nb, cb, rb) = stats
        ok = (na > 0) & (nb > 0)
        k_ = torch.sqrt(rb / ra) if scale else torch.ones((), dtype=torch.float64, device=dev)
        ok = ok & torch.isfinite(k_) & (k_ > 0)
        k_ = torch.where(ok, k_, torch.ones_like(k_))
        shift = torch.where(ok, cb - k_ * ca, torch.zeros_like(ca))
        out.append(torch.cat([k_ * torch.eye(3, dtype=torch.float64, device=dev), shift[:, None]], dim=1).reshape(12))
    return torch.stack(out), torch.stack([o[0] for o in out])


def _check_init(init, N, dev):
    """(transform (N, 12) float64 on dev, scale (N,) float64) of a matrix-like ``init``."""
    if isinstance(init, Alignment):
        m, sc = init.matrix, init.scale
        if tuple(m.shape) != (N, 4, 4):
            raise ValueError(f"init: an Alignment of {int(m.shape[0])} scene(s) with scenes = {N}")
        return m[:, :3, :].to(dev, torch.float64).reshape(N, 12).contiguous(), sc.to(dev, torch.float64).clone()
    if not torch.is_tensor(init) or tuple(init.shape) not in ((4, 4), (N, 4, 4)):
        raise ValueError(f"init: None, 'centroid', an Alignment, or a (4, 4) or ({N}, 4, 4) matrix")
    m = init.to(torch.float64)
    if m.device.type == "cpu":
        flat = m.reshape(-1, 4, 4)
        if not bool(torch.isfinite(flat).all()) or not bool((flat[:, 3] == torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)).all()):
            raise ValueError("init: a finite matrix whose last row is (0, 0, 0, 1)")
        if not bool((torch.linalg.det(flat[:, :3, :3]) > 0).all()):
            raise ValueError("init: the 3 x 3 block must have a positive determinant (a similarity, not a reflection)")
    m = m.to(dev).expand(N, 4, 4) if m.dim() == 2 else m.to(dev)
    return m[:, :3, :].reshape(N, 12).contiguous(), torch.linalg.det(m[:, :3, :3]).abs().pow(1.0 / 3.0)


def _start_transform(init, N, dev, centroid):
    """(transform (N, 12) float64 on dev, scale (N,) float64) of the ``init`` argument of the ICP functions.  centroid: a callable that
    gives ``_centroid_init``'s pair; it is called for "centroid" only, the one form that may read the host.  The loop writes its result
    into ``transform``, so it is ALWAYS a fresh tensor: ``_check_init``'s can be a view of the caller's matrix (one scene: the first three
    rows of a (4, 4) float64 matrix are contiguous as they lie)."""
    if init is None:
        return _identity_transform(N, dev), torch.ones(N, dtype=torch.float64, device=dev)
    if isinstance(init, str):
        if init != "centroid":
            raise ValueError(f"init = {init!r}: None, 'centroid', an Alignment, or a (4, 4) or ({N}, 4, 4) matrix")
        return centroid()
    transform, scale0 = _check_init(init, N, dev)
    return transform.clone(), scale0


def align_geometry(source, target, scenes=1, iters=ALIGN_ITERS, scale=False, max_distance=None, init=None, method="auto", grid=None):
    """Point-to-point ICP: ``iters`` times, every source point under the current transform is matched with its exact nearest target
    point (``nearest_points``' bits) and the transform is re-fitted to the accepted pairs in closed form (include/mvd_hip.h:
    mvd_align_icp has the rule) -> Alignment, whose ``rms`` / ``pairs`` history is how a caller sees convergence.

    source, target : what ``nearest_points`` takes; a TriangleMesh is refused with the same message.  The target never moves: its
              grid is built once.
    scenes  : N; every scene is aligned on its own.
    iters   : an integer in [0, 1024], a FIXED count: nothing is read back from the device, so there is no early exit.  0 returns
              ``init`` with its one history row.
    scale   : also fit a uniform scale (a similarity); False keeps it at exactly 1 times that of ``init``.
    max_distance : in world units; a pair is accepted when the point found a target and dist2 <= fl32(max_distance)^2, compared in
              fp32.  None accepts every pair.  With outliers or partial overlap a gate is what keeps the fit honest.
    init    : where to start: None (the identity), an Alignment, an (N, 4, 4) or (4, 4) matrix [[s R, t], [0, 1]] with det > 0 (a matrix
              in host memory is checked: finite, last row (0, 0, 0, 1), det > 0; one on the GPU is NOT, nothing being read back -- a
              reflection or a NaN there is taken as given, and its scale as |det|^(1/3)), or
              "centroid" -- the source's per-scene centroid mapped onto the target's and, with ``scale``, the RMS radii matched
              (float64 torch ops per scene slice; reads the scene offsets once).  ICP converges to the nearest local optimum: it needs
              a start in its basin -- ``register_geometry`` finds one from an arbitrary pose, and its result is a valid ``init``.
              ``init`` is copied, never written into, here and in ``align_to_surface`` and ``align_to_mesh``.
    method, grid : those of ``nearest_points``.
    ``iters`` and ``max_distance`` are INTERFACE defaults: no trained checkpoint or scan was available when this was written, so
    nobody has tuned them on real data -- expect to.  A scene with fewer than 3 accepted pairs keeps its transform.  Apart from
    ``init="centroid"`` nothing synchronises with the host."""
    N, method, grid = _check_nn(scenes, method, grid)
    iters, max_d2 = _check_icp(iters, max_distance, scale)
    s, s_scene = _points_of(source, "source", N)
    t, t_scene = _points_of(target, "target", N)
    dev = s.device
    s, t = s.float().contiguous(), t.to(dev, torch.float32).contiguous()
    s_start, t_start = _scene_start(s_scene, int(s.shape[0]), N, dev), _scene_start(t_scene, int(t.shape[0]), N, dev)
    transform, scale0 = _start_transform(init, N, dev, lambda: _centroid_init(s, s_start, t, t_start, N, scale))
    history, moved, index, dist2 = _align_icp(s, s_start, t, t_start, N, method, grid, iters, hip.ALIGN_SCALE if scale else 0, max_d2, transform)
    return _alignment(transform, scale0 * history[-1, :, 2], history, moved, index, dist2)


@dataclass
class PlaneAlignment(Alignment):
    """What ``fit_plane_step`` and ``align_to_surface`` return: an ``Alignment`` -- ``apply`` and everything that takes one work
    unchanged -- whose ``rms`` is the POINT rms of the accepted pairs, so that it compares with ``align_geometry``'s, plus the two rows
    of the point-to-plane fit."""
    plane_rms: torch.Tensor = None           # (iters + 1, N) float64: RMS distance of the accepted pairs ALONG the target's normals
    rank: torch.Tensor = None                # (iters + 1, N) int64: the directions (of 6) the solve of that row's pairs keeps; 0: no step


def _plane_alignment(transform, scale, history, xyz, index, dist2):
    base = _alignment(transform, scale, history[:, :, [2, 1, 0]], xyz, index, dist2)
    return PlaneAlignment(**{f: getattr(base, f) for f in ("matrix", "rotation", "translation", "scale", "rms", "pairs", "xyz", "nearest")},
                          plane_rms=history[:, :, 0].clone(), rank=history[:, :, 3].to(torch.int64))


def _target_normals(normals, t, t_scene, N, k, method, grid, nt):
    """(nt, 3) fp32 contiguous on the target's device from the ``normals`` argument of the two plane functions."""
    if normals is None:
        start = _scene_start(t_scene, nt, N, t.device)
        index, _ = _knn(t, start, t, start, N, k, method, grid)
        return _normals(t, index, t, None)[0]
    if isinstance(normals, PointNormals):
        normals = normals.normal
    if not torch.is_tensor(normals) or tuple(normals.shape) != (nt, 3):
        raise ValueError(f"normals: None, a PointNormals or an ({nt}, 3) tensor -- one normal per target point")
    return normals.to(t.device, torch.float32).contiguous()


def fit_plane_step(source, target, normals, scenes=1, pairs=None):
    """ONE linearised point-to-plane step for KNOWN correspondences (include/mvd_hip.h: mvd_plane_fit has the rule) -> PlaneAlignment:
    the rigid motion x -> R x + t, R = exp([omega]x), that minimises sum ((p + omega x p + t - q) . n)^2 over the pairs (p, q) with n
    the target's normal at q.  The counterpart of ``fit_similarity``; unlike it this is a step, not a solution -- the error is
    linearised in the rotation, so a large motion takes several.

    source, target, scenes, pairs : as for ``fit_similarity`` (row i with row i, or with row pairs[i]; -1 skips).
    normals : an (nt, 3) tensor or the PointNormals of ``estimate_normals(target)``: one normal per target row.  Their sign does not
              matter; a zero or non-finite normal skips the pair.
    A direction the pairs do not constrain -- sliding along a plane, turning about a sphere's centre -- is left alone (``rank`` < 6), not
    blown up.  A scene with fewer than 3 pairs gets the identity.  ``rms``, ``plane_rms``, ``pairs`` and ``rank`` have one row: under the
    step.  Nothing is read back from the device."""
    N, _, _ = _check_nn(scenes, "auto", None)
    s, s_scene = _points_of(source, "source", N)
    t, t_scene = _points_of(target, "target", N)
    dev, n, nt = s.device, int(s.shape[0]), int(t.shape[0])
    if normals is None:
        raise ValueError("normals: a PointNormals or an (nt, 3) tensor (estimate_normals(target) makes them)")
    _check_pairs(pairs, n, nt)
    s, t = s.float().contiguous(), t.to(dev, torch.float32).contiguous()
    nrm = _target_normals(normals, t, t_scene, N, NORMALS_K, hip.NN_AUTO, 0, nt)
    start = _scene_start(s_scene, n, N, dev)
    index = None if pairs is None else pairs.to(dev).contiguous()
    transform = _identity_transform(N, dev)
    _plane_fit(s, start, t, nrm, index, N, 0, float("inf"), transform)
    moved = _align_apply(s, start, N, transform)
    last = _plane_fit(moved, start, t, nrm, index, N, hip.PLANE_NO_STEP, float("inf"), transform)
    return _plane_alignment(transform, torch.ones(N, dtype=torch.float64, device=dev), last[None], moved,
                            *_given_pairs(moved, start, t, index, nt, N))


def align_to_surface(source, target, normals=None, k=NORMALS_K, scenes=1, iters=ALIGN_ITERS, max_distance=None, init=None, method="auto",
                     grid=None):
    """Point-to-plane ICP: ``align_geometry``'s loop -- the target's grid built once, every iteration an apply, an exact nearest-point
    query and a deterministic reduction, nothing read back -- with the distance ALONG THE TARGET'S NORMAL minimised instead of the
    distance between the points (include/mvd_hip.h: mvd_plane_icp has the rule) -> PlaneAlignment.

    The division of labour: point-to-point has the larger basin -- it pulls matched points together wherever they are -- but on a dense
    smooth surface against an independent resampling of itself it slides slowly, because the nearest sample is never the same surface
    point.  Point-to-plane lets the source slide along the surface freely and converges there in a handful of iterations, but its
    linearisation wants a start within a few degrees.  The recipe is both:
        ``align_to_surface(source, target, init=align_geometry(source, target, iters=5))``.

    source, target, scenes, iters, max_distance, method, grid : those of ``align_geometry``; ``iters`` and ``max_distance`` are the same
              untuned interface defaults.
    normals : one normal per target point: an (nt, 3) tensor, a PointNormals, or None for ``estimate_normals(target, k)`` -- whose sign
              does not matter to the fit.  A target point without a valid normal takes no part.  For a mesh target,
              ``sample_normals`` gives exact ones.
    k       : the neighbourhood of those normals, unused otherwise.
    init    : where to start: None, an Alignment (a PlaneAlignment is one), an (N, 4, 4) or (4, 4) matrix, or "centroid", as for
              ``align_geometry``.  The fit is RIGID: a scale in ``init`` is carried through untouched, none is fitted.
    ``rms`` is the point rms (comparable with ``align_geometry``'s), ``plane_rms`` the rms along the normals, ``rank`` the directions of
    the six that each row's pairs constrain; rows as in ``Alignment``.  Apart from ``init="centroid"`` nothing synchronises with the
    host."""
    N, method, grid = _check_nn(scenes, method, grid)
    iters, max_d2 = _check_icp(iters, max_distance)
    if normals is None:
        k = _check_k(k, hip.KNN_MAX_K, "hip.KNN_MAX_K")
        if k < 3:
            raise ValueError(f"k = {k}: a normal needs at least 3 neighbours")
    s, s_scene = _points_of(source, "source", N)
    t, t_scene = _points_of(target, "target", N)
    dev = s.device
    s, t = s.float().contiguous(), t.to(dev, torch.float32).contiguous()
    s_start, t_start = _scene_start(s_scene, int(s.shape[0]), N, dev), _scene_start(t_scene, int(t.shape[0]), N, dev)
    transform, scale0 = _start_transform(init, N, dev, lambda: _centroid_init(s, s_start, t, t_start, N, False))
    nrm = _target_normals(normals, t, t_scene, N, k, method, grid, int(t.shape[0]))
    history, moved, index, dist2 = _plane_icp(s, s_start, t, t_start, nrm, N, method, grid, iters, max_d2, transform)
    return _plane_alignment(transform, scale0, history, moved, index, dist2)


def align_to_mesh(source, mesh, scenes=1, iters=ALIGN_ITERS, max_distance=None, init=None, method="auto", grid=None):
    """Point-to-plane ICP whose target is the mesh ITSELF (include/mvd_hip.h: mvd_mesh_icp has the rule) -> PlaneAlignment.
    ``align_to_surface(source, sample_mesh(mesh, n), sample_normals(...))`` pairs a source point with the nearest SAMPLE, and its
    residual falls with the sampling density; here the pair is the exact closest point of the triangles with that face's normal, so
    nothing depends on a sampling of the target.  The loop, the fit, the gate and the rank rule are ``align_to_surface``'s.

    source, scenes, iters, max_distance, init, method, grid : as for ``align_to_surface`` (the fit is rigid and carries a scale in
              ``init`` through untouched); ``iters`` and ``max_distance`` are the same untuned interface defaults.
    mesh    : a TriangleMesh of at most ``scenes`` scenes; a degenerate face pairs with nothing (its normal is zero).
    ``nearest`` is the NearestOnMesh of the moved source against the mesh (the final correspondences).  Apart from
    ``init="centroid"`` -- which centres on the mesh's VERTICES -- nothing synchronises with the host."""
    import dataclasses
    N, method, grid = _check_nn(scenes, method, grid)
    iters, max_d2 = _check_icp(iters, max_distance)
    s, s_scene = _points_of(source, "source", N)
    dev = s.device
    s = s.float().contiguous()
    vertices, faces, face_start = _mesh_arrays(mesh, N, dev)
    s_start = _scene_start(s_scene, int(s.shape[0]), N, dev)

    def centroid():
        v_start = [int(v) for v in mesh.vertex_start.tolist()]
        v_start = torch.tensor(v_start + [v_start[-1]] * (N + 1 - len(v_start)), dtype=torch.int32).to(dev)
        return _centroid_init(s, s_start, vertices, v_start, N, False)
    transform, scale0 = _start_transform(init, N, dev, centroid)
    history, moved, face, dist2 = _mesh_icp(s, s_start, vertices, faces, face_start, N, method, grid, iters, max_d2, transform)
    out = _plane_alignment(transform, scale0, history, moved, face, dist2)
    # every field of the final correspondences (the loop keeps face, dist2, point and normal only): the same search once more
    return dataclasses.replace(out, nearest=_nearest_on_mesh(moved, s_start, vertices, faces, face_start, N, method, grid))


# ------------------------------------------------------------------------------------------------ global registration
REGISTER_ROTATIONS = 4096                    # register_geometry's defaults: rotations scored, sample rows per scene, candidates refined.
REGISTER_SAMPLES = 256                       # INTERFACE defaults: the cheapest setting at which the float64 oracle recovers every pose of
REGISTER_CANDIDATES = 4                      # the test table (DESIGN.md has the sweep); nobody has tuned them on real data
_SF_PHI, _SF_PSI = 2.0 ** 0.5, 1.533751168755204288118041      # the two constants of the super-Fibonacci spiral


def rotation_grid(n):
    """(n, 4) float64 unit quaternions (w, x, y, z) that cover the rotations evenly: the super-Fibonacci spiral (Alexa, CVPR 2022).
    With s = i + 1/2 and t = s / n, point i is (sqrt(t) sin a, sqrt(t) cos a, sqrt(1 - t) sin b, sqrt(1 - t) cos b), a = 2 pi s / sqrt(2),
    b = 2 pi s / 1.533751168755204288118041.  Formed in numpy float64 on the host: the same n gives the same bits.  The covering
    radius -- the largest angle from any rotation to the nearest of the grid -- is about 35 degrees at n = 256, 20 at 1 024, 13 at
    4 096."""
    import numpy as np
    if isinstance(n, bool) or not isinstance(n, (int, float)) or int(n) != n or not 1 <= n <= hip.REGISTER_MAX_H:
        raise ValueError(f"rotation_grid: n = {n}: an integer in [1, {hip.REGISTER_MAX_H}]")
    n = int(n)
    s = np.arange(n, dtype=np.float64) + 0.5
    t = s / float(n)
    r, big = np.sqrt(t), np.sqrt(1.0 - t)
    a, b = 2.0 * np.pi * s / _SF_PHI, 2.0 * np.pi * s / _SF_PSI
    return torch.from_numpy(np.stack([r * np.sin(a), r * np.cos(a), big * np.sin(b), big * np.cos(b)], axis=1))


def _quat_matrix(q):
    """(H, 4) unit (w, x, y, z) float64 -> (H, 3, 3), the formula of the solve (include/mvd_hip.h: mvd_align_fit)."""
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=1).reshape(-1, 3, 3)


def _matrix_quat(R):
    """(H, 3, 3) rotations float64 (host) -> (H, 4) unit (w, x, y, z): the dominant eigenvector of the symmetric 4 x 4 form, which has
    no branch at 180 degrees."""
    m = lambda a, b: R[:, a, b]
    K = torch.stack([m(0, 0) + m(1, 1) + m(2, 2), m(2, 1) - m(1, 2), m(0, 2) - m(2, 0), m(1, 0) - m(0, 1),
                     m(2, 1) - m(1, 2), m(0, 0) - m(1, 1) - m(2, 2), m(0, 1) + m(1, 0), m(0, 2) + m(2, 0),
                     m(0, 2) - m(2, 0), m(0, 1) + m(1, 0), m(1, 1) - m(0, 0) - m(2, 2), m(1, 2) + m(2, 1),
                     m(1, 0) - m(0, 1), m(0, 2) + m(2, 0), m(1, 2) + m(2, 1), m(2, 2) - m(0, 0) - m(1, 1)], dim=1).reshape(-1, 4, 4)
    return torch.linalg.eigh(K)[1][:, :, -1].contiguous()


def _check_rotations(rotations):
    """(quat (H, 4), R (H, 3, 3)) float64 in host memory, of a count, an (H, 4) or an (H, 3, 3) tensor."""
    if not torch.is_tensor(rotations):
        q = rotation_grid(rotations)
        return q, _quat_matrix(q)
    if rotations.dim() not in (2, 3) or tuple(rotations.shape[1:]) not in ((4,), (3, 3)) or not 1 <= rotations.shape[0] <= hip.REGISTER_MAX_H:
        raise ValueError(f"rotations: a count, or an (H, 4) or (H, 3, 3) tensor with 1 <= H <= {hip.REGISTER_MAX_H}; got {tuple(rotations.shape)}")
    r = rotations.detach().to("cpu", torch.float64)
    if not bool(torch.isfinite(r).all()):
        raise ValueError("rotations: a non-finite entry")
    if r.dim() == 2:
        norm = r.norm(dim=1, keepdim=True)
        if not bool((norm > 0).all()):
            raise ValueError("rotations: a zero quaternion")
        q = r / norm
        return q, _quat_matrix(q)
    if not bool((torch.linalg.det(r) > 0).all()):
        raise ValueError("rotations: a matrix with a non-positive determinant (rotations, not reflections)")
    return _matrix_quat(r), r


def _register_scratch(n_rows, nt, N, H, method, grid):
    return int(hip.lib().mvd_register_scratch(n_rows, nt, N, H, method, grid))


def _register_build(target, target_start, N, method, grid, scratch, nbytes):
    """MVD_NN_BUILD of mvd_nearest_points_stages into the head of ``scratch``: the grid every following score walks."""
    L = hip.lib()
    nt = int(target.shape[0])
    hip.check(L.mvd_nearest_points_stages(None, hip.ptr(target_start), _p(target), hip.ptr(target_start), 0, nt, N, method, grid, None, None,
                                          _p(scratch), nbytes, hip.NN_BUILD, hip.stream()))


def _register_score(points, start, target, target_start, N, hyp, trunc2, method, grid, scratch, nbytes):
    """The enqueues of mvd_register_score against the grid ``_register_build`` left in ``scratch``: points (n, 3) fp32, hyp (N, H, 12)
    float64 -> (score (N, H) float64, inliers (N, H) int32).  No host synchronisation."""
    L = hip.lib()
    dev, n, nt, H = points.device, int(points.shape[0]), int(target.shape[0]), int(hyp.shape[1])
    hip._req(points), hip._req(target), hip._req(start, torch.int32), hip._req(target_start, torch.int32), hip._req(hyp, torch.float64)
    score = torch.empty(N, H, dtype=torch.float64, device=dev)
    inliers = torch.empty(N, H, dtype=torch.int32, device=dev)
    hip.check(L.mvd_register_score(_p(points), hip.ptr(start), _p(target), hip.ptr(target_start), n, nt, N, H, hip.ptr(hyp), trunc2, method, grid,
                                   hip.ptr(score), hip.ptr(inliers), hip.ptr(scratch), nbytes, hip.stream()))
    return score, inliers


def _register_select(score, quat, K, cos_half):
    """The enqueue of mvd_register_select: score (N, H) float64, quat (H, 4) float64 -> (top (N, K) int32, top_score (N, K) float64)."""
    L = hip.lib()
    N, H = int(score.shape[0]), int(score.shape[1])
    hip._req(score, torch.float64), hip._req(quat, torch.float64)
    top = torch.empty(N, K, dtype=torch.int32, device=score.device)
    top_score = torch.empty(N, K, dtype=torch.float64, device=score.device)
    hip.check(L.mvd_register_select(hip.ptr(score), hip.ptr(quat), N, H, K, cos_half, hip.ptr(top), hip.ptr(top_score), hip.stream()))
    return top, top_score


@dataclass
class Registration(Alignment):
    """What ``register_geometry`` returns: the Alignment of the chosen candidate after its last ICP iterations (``rms`` / ``pairs`` are
    the history of those), and what the choice was made from.  An object with a symmetry shows as two candidates with (nearly) equal
    scores: the data cannot tell them apart, and ``chosen`` is then the lower row."""
    candidates: torch.Tensor                 # (N, K, 4, 4) float64: the K refined transforms
    candidate_score: torch.Tensor            # (N, K) float64: their truncated cost on the full source; +inf for a slot without a candidate
    candidate_inliers: torch.Tensor          # (N, K) int32: source points within `trunc` of the target under each
    chosen: torch.Tensor                     # (N,) int64: the row of `candidates` the result was polished from
    grid_score: torch.Tensor                 # (N, H) float64: the truncated cost of the sample under every rotation of the grid


def _scene_moments(pts, starts, N):
    """Per scene (ok (N,) bool, centroid (N, 3), mean squared radius (N,)) of the finite rows: ``_centroid_init``'s float64 torch ops."""
    ok, cen, r2 = [], [], []
    for k in range(N):
        part = pts[starts[k]:starts[k + 1]].double()
        fin = torch.isfinite(part).all(1, keepdim=True)
        cnt = fin.sum().double()
        c = torch.where(fin, part, torch.zeros_like(part)).sum(0) / cnt
        ok.append(cnt > 0), cen.append(c), r2.append(torch.where(fin, (part - c) ** 2, torch.zeros_like(part)).sum() / cnt)
    return torch.stack(ok), torch.stack(cen), torch.stack(r2)


def _check_count(value, name, lo, hi):
    if isinstance(value, bool) or not isinstance(value, (int, float)) or int(value) != value or not lo <= value <= hi:
        raise ValueError(f"{name} = {value}: an integer in [{lo}, {hi}]")
    return int(value)


def _register_inputs(s, s_start, t, t_start, N, R, scale, samples, trunc):
    """What ``register_geometry`` scores: (hyp (N, H, 12) float64, the scale k of the hypotheses (N,), the sample (m, 3) fp32, its offsets
    (N + 1,) int32, trunc2 as the fp32 value the kernel compares with).  R (H, 3, 3) float64 in host memory.  Reads the scene offsets
    once and, with ``trunc`` None, the target's radii."""
    dev, H = s.device, int(R.shape[0])
    starts = torch.stack([s_start, t_start]).tolist()                       # the host read
    (ok_s, c_s, r_s), (ok_t, c_t, r_t) = _scene_moments(s, starts[0], N), _scene_moments(t, starts[1], N)
    if trunc is None:
        radii = [math.sqrt(v) for v in r_t.tolist() if 0 < v < float("inf")]
        if not radii:
            raise ValueError("trunc = None: no scene of the target has two distinct finite points to take a radius from")
        trunc = 0.1 * min(radii)
    trunc2 = _fl32_square(float(trunc))
    if not 0 < trunc2 < float("inf"):
        raise ValueError(f"trunc = {trunc}: its square is not a positive finite fp32 value")
    # hypotheses: k R_h, t = c_t - k R_h c_s
    k_ = torch.sqrt(r_t / r_s) if scale else torch.ones(N, dtype=torch.float64, device=dev)
    ok = ok_s & ok_t & torch.isfinite(k_) & (k_ > 0)
    k_ = torch.where(ok, k_, torch.ones_like(k_))
    A = k_[:, None, None, None] * R.to(dev)[None]                            # (N, H, 3, 3)
    turned = (A * c_s[:, None, None, :]).sum(-1)                             # (N, H, 3)
    shift = torch.where(ok[:, None, None], c_t[:, None, :] - turned, torch.zeros_like(turned))
    hyp = torch.cat([A, shift[..., None]], dim=-1).reshape(N, H, 12).contiguous()
    # the sample: every step-th row of each scene
    rows, sample_start = [], [0]
    for k in range(N):
        a, b = starts[0][k], starts[0][k + 1]
        rows.append(torch.arange(a, b, max(-(-(b - a) // samples), 1), dtype=torch.int64))
        sample_start.append(sample_start[-1] + int(rows[-1].numel()))
    sample = s[torch.cat(rows).to(dev)].contiguous()
    sample_start = torch.tensor(sample_start, dtype=torch.int32).to(dev)
    return hyp, k_, sample, sample_start, trunc2


def register_geometry(source, target, scenes=1, rotations=REGISTER_ROTATIONS, samples=REGISTER_SAMPLES, candidates=REGISTER_CANDIDATES,
                      separation=30.0, trunc=None, scale=False, refine_iters=20, iters=ALIGN_ITERS, max_distance=None, method="auto",
                      grid=None):
    """Global registration: the start ICP needs, found without one -> Registration, an Alignment (so a valid ``init=`` of
    ``align_geometry``, ``align_to_surface`` and ``align_to_mesh``, with ``.apply``).  A grid of rotations is scored on a sample of the
    source, the best few distinct ones are refined by point-to-point ICP, and the best AFTER refinement is polished (include/mvd_hip.h:
    mvd_register_score and mvd_register_select have the rules).

    source, target : what ``nearest_points`` takes; a TriangleMesh is refused with the same message -- for a mesh target,
              ``align_to_mesh(s, mesh, init=register_geometry(s, sample_mesh(mesh, n)))``.
    scenes  : N; every scene is registered on its own.
    rotations : H, the size of ``rotation_grid`` (at most hip.REGISTER_MAX_H), or the rotations themselves as an (H, 4) tensor of
              (w, x, y, z) quaternions or an (H, 3, 3) tensor of matrices -- a known symmetry group, or the identity alone.
    Hypotheses : per scene and rotation R_h, x -> k R_h x + t with the source's centroid mapped onto the target's and, with ``scale``,
              k the ratio of the RMS radii (else 1): ``init="centroid"`` turned by R_h.  float64 torch ops; they read the scene offsets
              once.  The translation comes from the centroids, so the two sides must show the same part of the object: partial
              overlap is out of scope.
    samples : the grid is scored on every ceil(n / samples)-th row of each scene, counted from the scene's first row.
    trunc   : a sample point costs min(d2, fl32(trunc)^2), d2 its squared distance to the nearest target point, so a point without a
              partner costs a constant instead of dominating the sum.  None: 0.1 x the RMS radius of the target (the smallest over the
              scenes; one more host read).
    candidates, separation : K <= hip.REGISTER_MAX_K rotations are refined: greedily the lowest score, then the lowest among those more
              than ``separation`` degrees from every one taken (0: plain top K).
    refine_iters : ICP iterations (``align_geometry``'s, on the FULL source, with ``scale`` and ``max_distance``) from each candidate.
              The refined candidates are scored on the full source and the lowest is chosen -- after refinement the true basin scores
              about 0, while a flipped basin of a nearly symmetric shape still scores high; before, their scores overlap.
    iters   : further ICP iterations from the chosen candidate; ``rms`` and ``pairs`` are their history.
    max_distance, method, grid : those of ``align_geometry``.
    ``rotations``, ``samples``, ``candidates``, ``separation``, ``trunc``, ``refine_iters`` and ``iters`` are INTERFACE defaults: chosen on a
    synthetic shape (DESIGN.md has the sweep), never tuned on real data -- expect to.  An object with a symmetry has several equally good
    answers; ``candidates`` / ``candidate_score`` show them.  The target's grid is built once for the two scores and once more inside
    each of the K + 1 ICP calls.  After the hypotheses everything is enqueued: no host read."""
    N, method, grid = _check_nn(scenes, method, grid)
    samples = _check_count(samples, "samples", 1, 2 ** 31 - 1)
    K = _check_count(candidates, "candidates", 1, hip.REGISTER_MAX_K)
    refine_iters = _check_count(refine_iters, "refine_iters", 0, hip.ALIGN_MAX_ITERS)
    iters = _check_count(iters, "iters", 0, hip.ALIGN_MAX_ITERS)
    if not isinstance(scale, bool):
        raise ValueError(f"scale = {scale!r}: True or False")
    if isinstance(separation, bool) or not 0 <= float(separation) <= 180:
        raise ValueError(f"separation = {separation}: degrees in [0, 180]")
    if trunc is not None and not 0 < float(trunc) < float("inf"):
        raise ValueError(f"trunc = {trunc}: None or a finite distance > 0")
    max_d2 = _max_d2(max_distance)
    if not torch.is_tensor(rotations):
        _check_count(rotations, "rotations", 1, hip.REGISTER_MAX_H)
    s, s_scene = _points_of(source, "source", N)
    t, t_scene = _points_of(target, "target", N)
    quat, R = _check_rotations(rotations)
    H = int(quat.shape[0])
    dev = s.device
    s, t = s.float().contiguous(), t.to(dev, torch.float32).contiguous()
    n, nt = int(s.shape[0]), int(t.shape[0])
    s_start, t_start = _scene_start(s_scene, n, N, dev), _scene_start(t_scene, nt, N, dev)
    hyp, k_, sample, sample_start, trunc2 = _register_inputs(s, s_start, t, t_start, N, R, scale, samples, trunc)
    nbytes = max(_register_scratch(int(sample.shape[0]), nt, N, H, method, grid), _register_scratch(n, nt, N, K, method, grid))
    scratch = _scratch(nbytes, dev)
    _register_build(t, t_start, N, method, grid, scratch, nbytes)
    grid_score, _ = _register_score(sample, sample_start, t, t_start, N, hyp, trunc2, method, grid, scratch, nbytes)
    cos_half = math.cos(math.radians(float(separation)) / 2.0) if float(separation) > 0 else 2.0
    top, _ = _register_select(grid_score, quat.to(dev).contiguous(), K, cos_half)
    flags = hip.ALIGN_SCALE if scale else 0
    scene_ids = torch.arange(N, device=dev)
    refined, refined_scale = [], []
    for k in range(K):
        tr = hyp[scene_ids, top[:, k].clamp(min=0).long()].clone()           # (a slot without a candidate refines hypothesis 0; it is never chosen)
        history, _, _, _ = _align_icp(s, s_start, t, t_start, N, method, grid, refine_iters, flags, max_d2, tr)
        refined.append(tr), refined_scale.append(k_ * history[-1, :, 2])
    refined, refined_scale = torch.stack(refined, dim=1).contiguous(), torch.stack(refined_scale, dim=1)
    cand_score, cand_inliers = _register_score(s, s_start, t, t_start, N, refined, trunc2, method, grid, scratch, nbytes)
    cand_score = torch.where(top >= 0, cand_score, torch.full_like(cand_score, float("inf")))
    chosen, _ = _register_select(cand_score, torch.zeros(K, 4, dtype=torch.float64, device=dev), 1, 2.0)
    chosen = chosen[:, 0].clamp(min=0).long()
    transform = refined[scene_ids, chosen].clone()
    history, moved, index, dist2 = _align_icp(s, s_start, t, t_start, N, method, grid, iters, flags, max_d2, transform)
    out = _alignment(transform, refined_scale[scene_ids, chosen] * history[-1, :, 2], history, moved, index, dist2)
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64, device=dev).expand(N, K, 1, 4)
    return Registration(**{f: getattr(out, f) for f in out.__dataclass_fields__}, candidates=torch.cat([refined.reshape(N, K, 3, 4), bottom], dim=2),
                        candidate_score=cand_score, candidate_inliers=cand_inliers, chosen=chosen, grid_score=grid_score)


# ------------------------------------------------------------------------------------------------ mesh topology
@dataclass
class MeshComponents:
    """What ``mesh_components`` returns.  Compact ids are the rank of a component's smallest vertex id, so components are numbered scene
    after scene; only components with a face are numbered."""
    vertex_component: torch.Tensor           # (nv,) int32: the compact id, -1 for a vertex no valid face uses
    face_component: torch.Tensor             # (nf,) int32: the compact id, -1 for an invalid face
    component_start: torch.Tensor            # (N + 1,) int32, host: scene s owns the ids [component_start[s], component_start[s + 1])
    root: torch.Tensor                       # (ncomp,) int32: the component's smallest vertex id
    faces: torch.Tensor                      # (ncomp,) int32: its valid faces
    vertices: torch.Tensor                   # (ncomp,) int32: its vertices

    def __len__(self):
        return int(self.root.shape[0])

    def _scene(self):
        """(ncomp,) int64 on the device: the scene of every component."""
        cs = self.component_start.to(self.root.device).long()
        return torch.repeat_interleave(torch.arange(cs.numel() - 1, device=cs.device), cs[1:] - cs[:-1])

    def _rank(self):
        """(ncomp,) int64: a component's position among its scene's components ordered by faces, most first, the lower id first
        between equal counts."""
        n, dev = len(self), self.root.device
        by_faces = torch.sort(-self.faces.long(), stable=True).indices
        order = by_faces[torch.sort(self._scene()[by_faces], stable=True).indices]      # scene after scene, within a scene as above
        pos = torch.arange(n, device=dev) - self.component_start.to(dev).long()[self._scene()[order]]
        return torch.empty(n, dtype=torch.long, device=dev).scatter_(0, order, pos)

    def select(self, keep):
        """(ncomp,) bool per component -> (nf,) bool per face (False for an invalid face)."""
        fc = self.face_component.long()
        if len(self) == 0:
            return torch.zeros_like(fc, dtype=torch.bool)
        return (fc >= 0) & keep[fc.clamp(min=0)]

    def largest(self, k=1):
        """(nf,) bool: the faces of each scene's ``k`` components with the most faces; between equal counts the lower id wins."""
        if int(k) != k or k < 1:
            raise ValueError(f"k = {k}: an integer >= 1")
        return self.select(self._rank() < int(k))


@dataclass
class MeshTopology:
    """What ``mesh_topology`` returns: (N,) int32 host tensors, one value per scene, and the per-vertex bits on the mesh's device."""
    vertices_used: torch.Tensor
    unreferenced: torch.Tensor
    faces_regular: torch.Tensor
    faces_repeated: torch.Tensor
    faces_invalid: torch.Tensor
    edges: torch.Tensor
    boundary_edges: torch.Tensor             # edges with one face
    nonmanifold_edges: torch.Tensor          # edges with more than two faces
    misoriented_edges: torch.Tensor          # edges whose two faces run along them in the same direction
    components: torch.Tensor
    euler: torch.Tensor                      # vertices_used - edges + faces_regular
    vertex_flags: torch.Tensor               # (nv,) uint8: hip.TOPO_FLAG_BOUNDARY, hip.TOPO_FLAG_NONMANIFOLD

    @property
    def closed(self):
        return self.boundary_edges == 0

    @property
    def manifold(self):
        return self.nonmanifold_edges == 0

    @property
    def oriented(self):
        return self.misoriented_edges == 0

    @property
    def watertight(self):
        return self.closed & self.manifold & self.oriented


def _topo_arrays(mesh):
    """(vertices, faces, rgb or None, vertex_start, face_start, N) of a TriangleMesh: contiguous on the device of its vertices, the two
    offset tables as int32 DEVICE tensors."""
    if not isinstance(mesh, TriangleMesh):
        raise ValueError("mesh must be a TriangleMesh")
    vertices, faces, rgb = mesh.vertices, mesh.faces, mesh.rgb
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"mesh: vertices of shape {tuple(vertices.shape)}, faces of shape {tuple(faces.shape)}, need (n, 3) and (m, 3)")
    if rgb is not None and tuple(rgb.shape) != tuple(vertices.shape):
        raise ValueError(f"mesh: rgb of shape {tuple(rgb.shape)} for vertices of shape {tuple(vertices.shape)}")
    starts = []
    for name, table, n in (("vertex_start", mesh.vertex_start, vertices.shape[0]), ("face_start", mesh.face_start, faces.shape[0])):
        start = [int(v) for v in table.tolist()]
        if len(start) < 2 or start[0] < 0 or start[-1] > n or any(a > b for a, b in zip(start, start[1:])):
            raise ValueError(f"mesh: {name} = {start} for {n} rows")
        starts.append(start)
    if len(starts[0]) != len(starts[1]):
        raise ValueError(f"mesh: vertex_start of {len(starts[0]) - 1} scenes, face_start of {len(starts[1]) - 1}")
    dev = vertices.device
    to_dev = lambda s: torch.tensor(s, dtype=torch.int32).to(dev)
    return (vertices.to(dev, torch.float32).contiguous(), faces.to(dev, torch.int32).contiguous(),
            None if rgb is None else rgb.to(dev, torch.float32).contiguous(), to_dev(starts[0]), to_dev(starts[1]), len(starts[0]) - 1)


def _incidence(faces, vertex_start, face_start, nv, N):
    """The enqueues of mvd_mesh_incidence -> (inc_start (nv + 1,), inc (3 nf,)) int32.  No host synchronisation."""
    L = hip.lib()
    dev, nf = faces.device, int(faces.shape[0])
    inc_start = torch.empty(nv + 1, dtype=torch.int32, device=dev)
    inc = torch.empty(3 * nf, dtype=torch.int32, device=dev)
    nbytes = int(L.mvd_mesh_incidence_scratch(nv, nf))
    scratch = _scratch(nbytes, dev)
    hip.check(L.mvd_mesh_incidence(_p(faces), hip.ptr(vertex_start), hip.ptr(face_start), nv, nf, N, hip.ptr(inc_start), _p(inc),
                                   hip.ptr(scratch), nbytes, hip.stream()))
    return inc_start, inc


def _label(faces, vertex_start, face_start, nv, N):
    """The enqueues of mvd_mesh_label -> (vertex_component, face_component, component_start), all on the device.  No host
    synchronisation."""
    L = hip.lib()
    dev, nf = faces.device, int(faces.shape[0])
    vc = torch.empty(nv, dtype=torch.int32, device=dev)
    fc = torch.empty(nf, dtype=torch.int32, device=dev)
    cs = torch.empty(N + 1, dtype=torch.int32, device=dev)
    nbytes = int(L.mvd_mesh_label_scratch(nv, nf))
    scratch = _scratch(nbytes, dev)
    hip.check(L.mvd_mesh_label(_p(faces), hip.ptr(vertex_start), hip.ptr(face_start), nv, nf, N, _p(vc), _p(fc), hip.ptr(cs), hip.ptr(scratch),
                               nbytes, hip.stream()))
    return vc, fc, cs


def _topology(faces, vertex_start, face_start, nv, N, table=None):
    """The enqueues of mvd_mesh_incidence, mvd_mesh_label and mvd_mesh_topology -> (totals (N, hip.TOPO_TOTALS) int32, vertex_flags
    (nv,) uint8, the incidence table), on the device.  No host synchronisation."""
    L = hip.lib()
    dev, nf = faces.device, int(faces.shape[0])
    inc_start, inc = table if table is not None else _incidence(faces, vertex_start, face_start, nv, N)
    vc, _, cs = _label(faces, vertex_start, face_start, nv, N)
    totals = torch.empty(N, hip.TOPO_TOTALS, dtype=torch.int32, device=dev)
    flags = torch.empty(nv, dtype=torch.uint8, device=dev)
    nbytes = int(L.mvd_mesh_topology_scratch(nv, nf))
    scratch = _scratch(nbytes, dev)
    hip.check(L.mvd_mesh_topology(_p(faces), hip.ptr(vertex_start), hip.ptr(face_start), nv, nf, N, hip.ptr(inc_start), _p(inc), _p(vc),
                                  hip.ptr(cs), hip.ptr(totals), _p(flags), hip.ptr(scratch), nbytes, hip.stream()))
    return totals, flags, (inc_start, inc)


def mesh_components(mesh):
    """The connected components of a TriangleMesh (include/mvd_hip.h: mvd_mesh_label has the rule) -> MeshComponents.  Two faces are
    connected when they share a vertex id; a face with an id outside its own scene's vertices is invalid and belongs to nothing.  The
    label of a component is its smallest vertex id, found by a lock-free union-find on the GPU; the result has the same bits run to run,
    and a scene has the same components alone and inside a batch (only the compact ids shift).  One host read: ``component_start``."""
    vertices, faces, _, vs, fs, N = _topo_arrays(mesh)
    L = hip.lib()
    dev, nv, nf = vertices.device, int(vertices.shape[0]), int(faces.shape[0])
    vc, fc, cs = _label(faces, vs, fs, nv, N)
    cs = cs.cpu()                                                  # the one host synchronisation
    ncomp = int(cs[N])
    root, nfaces, nverts = (torch.empty(ncomp, dtype=torch.int32, device=dev) for _ in range(3))
    hip.check(L.mvd_mesh_component_table(_p(vc), _p(fc), nv, nf, ncomp, _p(root), _p(nfaces), _p(nverts), hip.stream()))
    return MeshComponents(vertex_component=vc, face_component=fc, component_start=cs, root=root, faces=nfaces, vertices=nverts)


def mesh_topology(mesh):
    """What a TriangleMesh is (include/mvd_hip.h: mvd_mesh_topology has the rule) -> MeshTopology: per scene the vertices used and
    unreferenced, the faces by class, the edges, those on a boundary (one face), non-manifold (more than two) and misoriented (two
    faces wound alike across them), the components and the Euler characteristic; per vertex whether it lies on a boundary or a
    non-manifold edge.  ``closed``, ``manifold``, ``oriented`` and ``watertight`` (all three) are (N,) bool.  A vertex of valence d
    costs O(d^2): fine for a marched mesh, a limit for a caller's mesh with a huge fan.  One host read: the (N, 11) totals."""
    vertices, faces, _, vs, fs, N = _topo_arrays(mesh)
    totals, flags, _ = _topology(faces, vs, fs, int(vertices.shape[0]), N)
    totals = totals.cpu()                                          # the one host synchronisation
    return MeshTopology(**{name: totals[:, k].clone() for k, name in enumerate(hip.TOPO_FIELDS)}, vertex_flags=flags)


def filter_mesh(mesh, keep_faces, return_index=False):
    """The sub-mesh of the faces with ``keep_faces`` set (include/mvd_hip.h: mvd_mesh_filter_count, mvd_mesh_filter_emit): kept faces
    and the vertices they name stay in their order, ids are rebased, ``rgb`` is carried bit for bit, the offset tables are rewritten;
    an invalid face is never kept.  keep_faces: (nf,) bool or uint8.  With ``return_index`` also the old rows: (mesh, vertex_index,
    face_index), int32 on the device.  One host read: the 2 (N + 1) new offsets."""
    vertices, faces, rgb, vs, fs, N = _topo_arrays(mesh)
    dev, nv, nf = vertices.device, int(vertices.shape[0]), int(faces.shape[0])
    if not torch.is_tensor(keep_faces) or tuple(keep_faces.shape) != (nf,) or keep_faces.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"keep_faces: an ({nf},) bool or uint8 tensor")
    L = hip.lib()
    keep = keep_faces.to(dev).to(torch.uint8).contiguous()
    nbytes = int(L.mvd_mesh_filter_scratch(nv, nf))
    scratch = _scratch(nbytes, dev)
    starts = torch.empty(2, N + 1, dtype=torch.int32, device=dev)
    hip.check(L.mvd_mesh_filter_count(_p(faces), _p(keep), hip.ptr(vs), hip.ptr(fs), nv, nf, N, hip.ptr(starts[0]), hip.ptr(starts[1]),
                                      hip.ptr(scratch), nbytes, hip.stream()))
    starts = starts.cpu()                                          # the one host synchronisation
    nvo, nfo = int(starts[0, N]), int(starts[1, N])
    out_v = torch.empty(nvo, 3, dtype=torch.float32, device=dev)
    out_c = torch.empty(nvo, 3, dtype=torch.float32, device=dev) if rgb is not None else None
    out_f = torch.empty(nfo, 3, dtype=torch.int32, device=dev)
    vi, fi = torch.empty(nvo, dtype=torch.int32, device=dev), torch.empty(nfo, dtype=torch.int32, device=dev)
    hip.check(L.mvd_mesh_filter_emit(_p(vertices), _p(rgb), _p(faces), nv, nf, _p(out_v), _p(out_c), _p(out_f), _p(vi), _p(fi), nvo, nfo,
                                     hip.ptr(scratch), nbytes, hip.stream()))
    out = TriangleMesh(vertices=out_v, faces=out_f, rgb=out_c, vertex_start=starts[0].clone(), face_start=starts[1].clone())
    return (out, vi, fi) if return_index else out


def keep_components(mesh, largest=None, min_faces=None, min_fraction=None, return_index=False):
    """The floater remover: ``mesh_components`` then ``filter_mesh``.  A component survives when it meets EVERY criterion given (at least
    one is required):
    largest      : it is among its scene's ``largest`` components by faces (between equal counts the lower id), an integer >= 1;
    min_faces    : it has at least this many faces;
    min_fraction : it has at least this fraction of its scene's valid faces, in [0, 1].
    Returns what ``filter_mesh`` returns.  Two host reads, one per composed call."""
    if largest is None and min_faces is None and min_fraction is None:
        raise ValueError("keep_components: give at least one of largest, min_faces, min_fraction")
    if largest is not None and (int(largest) != largest or largest < 1):
        raise ValueError(f"largest = {largest}: an integer >= 1")
    if min_faces is not None and (int(min_faces) != min_faces or min_faces < 0):
        raise ValueError(f"min_faces = {min_faces}: an integer >= 0")
    if min_fraction is not None and not 0.0 <= float(min_fraction) <= 1.0:
        raise ValueError(f"min_fraction = {min_fraction}: in [0, 1]")
    comp = mesh_components(mesh)
    keep = torch.ones(len(comp), dtype=torch.bool, device=comp.root.device)
    if len(comp):
        if largest is not None:
            keep &= comp._rank() < int(largest)
        if min_faces is not None:
            keep &= comp.faces >= int(min_faces)
        if min_fraction is not None:
            scene = comp._scene()
            per_scene = torch.zeros(comp.component_start.numel() - 1, dtype=torch.long, device=keep.device).index_add_(0, scene, comp.faces.long())
            keep &= comp.faces.double() >= float(min_fraction) * per_scene[scene].double()
    return filter_mesh(mesh, comp.select(keep), return_index=return_index)


def vertex_normals(mesh):
    """(n, 3) fp32 unit normals per vertex of a TriangleMesh (include/mvd_hip.h: mvd_mesh_vertex_normals): the area-weighted mean of
    the normals of the faces round the vertex -- the fp64 sum of their raw cross products in face order, divided by its length, rounded
    once; zero for a vertex of no regular face or of zero or non-finite total area.  The winding decides the side, as for
    ``sample_normals``.  A plain tensor, not a PointNormals: there is no neighbourhood, so ``variation`` and ``neighbours`` would mean
    nothing.  ``write_ply(path, mesh, vertex_normals(mesh))`` saves them.  Nothing is read back from the device."""
    vertices, faces, _, vs, fs, N = _topo_arrays(mesh)
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    inc_start, inc = _incidence(faces, vs, fs, nv, N)
    normals = torch.empty(nv, 3, dtype=torch.float32, device=vertices.device)
    hip.check(hip.lib().mvd_mesh_vertex_normals(_p(vertices), _p(faces), hip.ptr(inc_start), _p(inc), nv, nf, _p(normals), hip.stream()))
    return normals


def smooth_mesh(mesh, iters=10, lam=0.5, mu=-0.53, pin_boundary=True):
    """Taubin smoothing of a TriangleMesh (include/mvd_hip.h: mvd_mesh_smooth has the rule) -> a TriangleMesh with new vertices and the
    same faces, rgb and offsets.  ``iters`` pairs of umbrella passes, the first of a pair with the factor ``lam`` (it shrinks), the second
    with ``mu`` < -lam (it inflates), 2 * iters passes in all: the staircase of a marched surface goes, the shape does not shrink as it
    would under lam alone.  A vertex moves towards the mean of the other two vertices of every face round it (an interior neighbour counts
    twice, a boundary neighbour once).  pin_boundary: vertices on a boundary edge stay where they are.  A vertex of no regular face, or
    one that would read a non-finite coordinate, stays too.

    iters, lam and mu are INTERFACE defaults: the usual Taubin values (pass band about 0.1), which nobody has tuned on this project's
    meshes -- expect to.  iters in [0, 1000]; lam, mu finite.  The same bits run to run.  Nothing is read back from the device."""
    if int(iters) != iters or not 0 <= iters <= 1000:
        raise ValueError(f"iters = {iters}: an integer in [0, 1000]")
    lam, mu = float(lam), float(mu)
    if not (math.isfinite(lam) and math.isfinite(mu)):
        raise ValueError(f"lam = {lam}, mu = {mu}: finite")
    vertices, faces, rgb, vs, fs, N = _topo_arrays(mesh)
    dev, nv, nf = vertices.device, int(vertices.shape[0]), int(faces.shape[0])
    if pin_boundary:
        _, flags, (inc_start, inc) = _topology(faces, vs, fs, nv, N)
    else:
        flags, (inc_start, inc) = None, _incidence(faces, vs, fs, nv, N)
    out, tmp = torch.empty_like(vertices), torch.empty_like(vertices)
    hip.check(hip.lib().mvd_mesh_smooth(_p(vertices), _p(faces), hip.ptr(inc_start), _p(inc), _p(flags), nv, nf, 2 * int(iters), lam, mu,
                                        hip.TOPO_FLAG_BOUNDARY if pin_boundary else 0, _p(out), _p(tmp), hip.stream()))
    return TriangleMesh(vertices=out, faces=mesh.faces, rgb=mesh.rgb, vertex_start=mesh.vertex_start, face_start=mesh.face_start)


# ------------------------------------------------------------------------------------------------ mesh simplification
SIMPLIFY_CELLS = 64                          # simplify_mesh's default resolution (an INTERFACE default, see its docstring)
SIMPLIFY_PLACEMENTS = {"mean": hip.SIMPLIFY_MEAN, "quadric": hip.SIMPLIFY_QUADRIC}


@dataclass
class MeshClusters:
    """What ``simplify_mesh(..., return_index=True)`` tells about every vertex of its result, int32 on the device."""
    size: torch.Tensor                       # (n,) the input vertices that went into it
    rank: torch.Tensor                       # (n,) the eigenvalues of its quadric above hip.SIMPLIFY_RANK_RATIO of the largest; 0 with placement "mean"
    placed: torch.Tensor                     # (n,) hip.SIMPLIFY_PLACED_MEAN, _QUADRIC, or _FALLBACK: the quadric point was refused, the mean stands

    def __len__(self):
        return int(self.size.shape[0])


def _check_cells(cells, N):
    if isinstance(cells, bool) or int(cells) != cells or not 1 <= cells <= hip.SIMPLIFY_MAX_CELLS:
        raise ValueError(f"cells = {cells}: an integer in [1, {hip.SIMPLIFY_MAX_CELLS}]")
    if N * int(cells) ** 3 > hip.SIMPLIFY_MAX_TABLE:
        raise ValueError(f"cells = {cells} for {N} scenes: scenes * cells^3 beyond 2^28")
    return int(cells)


def _cluster(vertices, rgb, faces, vs, fs, nv, N, cells, placement):
    """The enqueues of mvd_mesh_incidence, mvd_mesh_cluster_count / _emit, mvd_mesh_incidence of the mapped faces and
    mvd_mesh_cluster_dedupe -> a dict of device tensors and the host's cluster_start.  One host read: cluster_start."""
    L = hip.lib()
    dev, nf = vertices.device, int(faces.shape[0])
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    inc_start, inc = _incidence(faces, vs, fs, nv, N)
    vc, cs = i32(nv), i32(N + 1)
    nbytes = int(L.mvd_mesh_cluster_scratch(nv, nf, N, cells))
    scratch = _scratch(nbytes, dev)
    hip.check(L.mvd_mesh_cluster_count(_p(vertices), hip.ptr(vs), hip.ptr(inc_start), nv, nf, N, cells, _p(vc), hip.ptr(cs), hip.ptr(scratch),
                                       nbytes, hip.stream()))
    cs_host = cs.cpu()                                             # the one host synchronisation
    nc = int(cs_host[N])
    out_v = torch.empty(nc, 3, dtype=torch.float32, device=dev)
    out_c = torch.empty(nc, 3, dtype=torch.float32, device=dev) if rgb is not None else None
    size, rank, placed, mapped = i32(nc), i32(nc), i32(nc), i32(nf, 3)
    keep, keep2 = torch.empty(nf, dtype=torch.uint8, device=dev), torch.empty(nf, dtype=torch.uint8, device=dev)
    hip.check(L.mvd_mesh_cluster_emit(_p(vertices), _p(rgb), _p(faces), hip.ptr(vs), hip.ptr(fs), hip.ptr(inc_start), _p(inc), _p(vc), nv, nf, N,
                                      cells, placement, nc, _p(out_v), _p(out_c), _p(size), _p(rank), _p(placed), _p(mapped), _p(keep),
                                      hip.ptr(scratch), nbytes, hip.stream()))
    cinc_start, cinc = _incidence(mapped, cs, fs, nc, N)
    hip.check(L.mvd_mesh_cluster_dedupe(_p(mapped), _p(keep), hip.ptr(cinc_start), _p(cinc), nc, nf, _p(keep2), hip.stream()))
    return dict(vertex_cluster=vc, cluster_start=cs_host, vertices=out_v, rgb=out_c, size=size, rank=rank, placed=placed, mapped_faces=mapped,
                keep=keep, keep_deduped=keep2)


def simplify_mesh(mesh, cells=SIMPLIFY_CELLS, placement="quadric", return_index=False):
    """Vertex clustering of a TriangleMesh (include/mvd_hip.h: the mesh simplification section has every rule) -> a TriangleMesh with
    fewer vertices and faces.  Each scene's box is cut into cubic cells, ``cells`` along its longest axis; the vertices of a cell become
    one vertex with their mean colour; a face survives when its three vertices fall into three cells, and of several faces on the same
    three vertices the first (so a sheet thinner than a cell loses one of its two sides).  A vertex that no face uses, one with a
    non-finite coordinate, and every face that names one, vanish.
    placement: "quadric" puts the vertex where the planes of the faces round its members meet (Lindstrom), as far as they determine it,
    and at the members' mean along the rest, so corners and creases stay where "mean" -- the plain mean of the members -- rounds them
    off; a quadric point outside its own cell falls back to the mean.  On smooth regions the quadric point is no closer to the surface
    than the mean: a UV sphere of radius 0.45 has a worst radius error of 0.0128 / 0.0030 / 0.0011 at cells = 4 / 8 / 16 either way.
    return_index: also (mesh, vertex_cluster, face_index, clusters) -- vertex_cluster (nv,) int32 the output vertex every input vertex
    went to, -1 for none; face_index int32 the input rows of the output faces; clusters a MeshClusters per output vertex.

    ``cells`` = 64 is an INTERFACE default nobody has tuned on this project's meshes -- expect to; an integer in [1, 256] with
    scenes * cells^3 <= 2^28.  NOT promised: clustering preserves neither manifoldness nor closedness --
    ``mesh_topology(simplify_mesh(m))`` is how a caller finds out.  No edge collapse, no target face count, no texture or UV handling, no
    boundary-preserving weights.  The same bits run to run, and for a scene alone or in a batch.  Two host reads: the cluster count and
    the filter's offsets."""
    if placement not in SIMPLIFY_PLACEMENTS:
        raise ValueError(f"placement = {placement!r}: one of {sorted(SIMPLIFY_PLACEMENTS)}")
    if not isinstance(mesh, TriangleMesh):
        raise ValueError("mesh must be a TriangleMesh")
    cells = _check_cells(cells, int(mesh.vertex_start.numel()) - 1)
    vertices, faces, rgb, vs, fs, N = _topo_arrays(mesh)
    nv = int(vertices.shape[0])
    c = _cluster(vertices, rgb, faces, vs, fs, nv, N, cells, SIMPLIFY_PLACEMENTS[placement])
    coarse = TriangleMesh(vertices=c["vertices"], faces=c["mapped_faces"], rgb=c["rgb"], vertex_start=c["cluster_start"], face_start=mesh.face_start)
    out, vi, fi = filter_mesh(coarse, c["keep_deduped"], return_index=True)
    if not return_index:
        return out
    nc = int(c["vertices"].shape[0])
    new_id = torch.full((nc + 1,), -1, dtype=torch.int32, device=vertices.device)      # (the spare row takes the non-members)
    new_id[vi.long()] = torch.arange(vi.numel(), dtype=torch.int32, device=vertices.device)
    vc = c["vertex_cluster"].long()
    vertex_cluster = new_id[torch.where(vc >= 0, vc, torch.full_like(vc, nc))]
    pick = lambda t: t[vi.long()]
    return out, vertex_cluster, fi, MeshClusters(size=pick(c["size"]), rank=pick(c["rank"]), placed=pick(c["placed"]))


def write_ply(path, cloud, normals=None):
    """Binary little-endian PLY: float x y z per vertex, and uchar red green blue (round(255 rgb)) when the cloud has colour.  A
    TriangleMesh is written the same way from its vertices, followed by ``element face`` with ``property list uchar int vertex_indices``.
    ``normals`` -- an (n, 3) tensor or the PointNormals of ``estimate_normals`` -- adds float nx ny nz behind x y z; without it the file
    is what it always was."""
    import numpy as np
    mesh = isinstance(cloud, TriangleMesh)
    pos = cloud.vertices if mesh else cloud.xyz
    n = int(pos.shape[0])
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        normals = normals.normal if isinstance(normals, PointNormals) else normals
        if not torch.is_tensor(normals) or tuple(normals.shape) != (n, 3):
            raise ValueError(f"normals: an ({n}, 3) tensor or a PointNormals")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if cloud.rgb is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    v = np.zeros(n, dtype=np.dtype(fields))
    xyz = pos.detach().cpu().numpy().astype("<f4")
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if normals is not None:
        nrm = normals.detach().cpu().numpy().astype("<f4")
        v["nx"], v["ny"], v["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    if cloud.rgb is not None:
        c = np.rint(np.clip(cloud.rgb.detach().cpu().numpy(), 0.0, 1.0) * 255.0).astype("u1")
        v["red"], v["green"], v["blue"] = c[:, 0], c[:, 1], c[:, 2]
    names = {"<f4": "float", "u1": "uchar"}
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {n}\n" + \
        "".join(f"property {names[t]} {k}\n" for k, t in fields)
    body = v.tobytes()
    if mesh:
        f = np.zeros(len(cloud), dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
        f["n"], f["v"] = 3, cloud.faces.detach().cpu().numpy()
        header += f"element face {len(cloud)}\nproperty list uchar int vertex_indices\n"
        body += f.tobytes()
    with open(path, "wb") as fh:
        fh.write((header + "end_header\n").encode("ascii"))
        fh.write(body)


# ------------------------------------------------------------------------------------------------ texture
TEX_BLENDS = {"mean": hip.TEX_MEAN, "best": hip.TEX_BEST}
TEX_FILTERS = {"nearest": hip.TEX_NEAREST, "bilinear": hip.TEX_BILINEAR}


def atlas_layout(nface_max, texels, scenes=1):
    """(cells per row C, side A) of the atlas for scenes of at most ``nface_max`` faces -- mvd_texture_atlas_side's rule on the host:
    cells of K = texels + 3 texels hold two faces each, C = max(1, ceil(sqrt(ceil(nface_max / 2)))), A = C * K."""
    if int(texels) != texels or not 1 <= texels <= hip.TEX_MAX_TEXELS:
        raise ValueError(f"texels = {texels}: an integer in [1, {hip.TEX_MAX_TEXELS}]")
    cells = (int(nface_max) + 1) // 2
    C = max(1, math.isqrt(cells - 1) + 1 if cells > 0 else 1)
    A = C * (int(texels) + 3)
    if A > hip.TEX_MAX_SIDE or scenes * A * A >= 2 ** 31:
        raise ValueError(f"texels = {texels}: an atlas of {scenes} x {A} x {A} texels for {nface_max} faces per scene; the side is at most "
                         f"{hip.TEX_MAX_SIDE} and the texel index 31 bits -- simplify the mesh or lower texels")
    return C, A


def _chart_of_texel(T, C, dev):
    """Per texel of the (A, A) atlas: (local face l, chart indices i, j, owned) by the header's closed form, with torch ops."""
    K = T + 3
    A = C * K
    y, x = torch.meshgrid(torch.arange(A, device=dev), torch.arange(A, device=dev), indexing="ij")
    i, j, cell = x % K, y % K, (y // K) * C + x // K
    lower = (i <= T) & (j <= T) & (i + j <= T + 1)
    mi, mj = K - 1 - i, K - 1 - j
    upper = (mi <= T) & (mj <= T) & (mi + mj <= T + 1)
    return 2 * cell + upper.long(), torch.where(lower, i, mi), torch.where(lower, j, mj), lower | upper


@dataclass
class MeshTexture:
    """What ``bake_texture`` returns; the leading scene dimension is present only for a list of camera sets.  Texel (x, y) has its centre
    at the integers; local face l of a scene is half l & 1 of cell l >> 1, cell c at column c % cells_per_row, row c // cells_per_row
    of cells ``texels + 3`` texels square (include/mvd_hip.h: the texture section has the layout in full)."""
    image: torch.Tensor                      # (.., 3, A, A) fp32
    views: torch.Tensor                      # (.., A, A) uint8: the views that contributed to the texel
    best: torch.Tensor                       # (.., A, A) uint8: the contributing view of the largest weight, or 255
    texels: int                              # T: texel intervals along a chart's legs
    cells_per_row: int                       # C
    side: int                                # A = C * (T + 3)
    faces: tuple = ()                        # the face count of every scene the texture was baked for

    def _local(self, mesh):
        fs = mesh.face_start.long()
        scene = torch.searchsorted(fs[1:].contiguous(), torch.arange(len(mesh)), right=True).clamp(max=fs.numel() - 2)
        return torch.arange(len(mesh)) - fs[scene]

    def corners(self, mesh):
        """(m, 3, 2) int64: the texel (x, y) of the corners a, b, c of every face of ``mesh``."""
        T, K, C = self.texels, self.texels + 3, self.cells_per_row
        l = self._local(mesh)
        cell, up = l // 2, (l % 2).bool()
        o = torch.stack([(cell % C) * K, (cell // C) * K], dim=1)[:, None]                                   # (m, 1, 2)
        low = torch.tensor([[0, 0], [T, 0], [0, T]])[None]
        return torch.where(up[:, None, None], o + (K - 1) - low, o + low)

    def uv(self, mesh):
        """(m, 3, 2) fp32 in [0, 1]: the OBJ texture coordinates (u right, v UP) of the corners a, b, c of every face."""
        c = self.corners(mesh).float()
        return torch.stack([(c[..., 0] + 0.5) / self.side, 1.0 - (c[..., 1] + 0.5) / self.side], dim=-1)

    def texel_face(self, mesh):
        """(.., A, A) int64: the row in mesh.faces of the face that owns each texel, -1 for none -- the ownership map, built with torch
        ops for inspection and tests (the kernels never need it)."""
        l, _, _, owned = _chart_of_texel(self.texels, self.cells_per_row, "cpu")
        fs = mesh.face_start.long()
        out = [torch.where(owned & (l < fs[s + 1] - fs[s]), l + fs[s], torch.full_like(l, -1)) for s in range(fs.numel() - 1)]
        return out[0] if self.image.dim() == 3 else torch.stack(out)

    def coverage(self):
        """The share of owned texels that at least one view contributed to: a 0-d tensor, or (N,) per scene."""
        T = self.texels
        per_face = (T + 1) * (T + 2) // 2 + T
        owned = torch.tensor([min(n, 2 * self.cells_per_row ** 2) * per_face for n in self.faces], dtype=torch.float32)
        seen = (self.views > 0).flatten(-2).sum(-1).float()
        owned = owned.to(seen.device).reshape(seen.shape)
        return seen / owned.clamp(min=1.0)


def _check_texture(texture, scenes, filter):
    if not isinstance(texture, MeshTexture):
        raise ValueError("texture must be a MeshTexture")
    if filter not in TEX_FILTERS:
        raise ValueError(f"filter = {filter!r}: one of {sorted(TEX_FILTERS)}")
    n = 1 if texture.image.dim() == 3 else int(texture.image.shape[0])
    if texture.image.dim() not in (3, 4) or tuple(texture.image.shape[-3:]) != (3, texture.side, texture.side) or \
            texture.side != texture.cells_per_row * (texture.texels + 3):
        raise ValueError(f"texture: image of shape {tuple(texture.image.shape)} for side {texture.side}, texels {texture.texels}")
    if n != scenes:
        raise ValueError(f"texture: baked for {n} scene(s), the mesh has {scenes}")


def _bake(vertices, colors, faces, vertex_start, face_start, cams, rgb, depth, N, V, texels, A, tol, min_cos, power, cull, blend, znear, fill):
    """The one enqueue of mvd_texture_bake.  Mesh arrays as ``_raster`` takes them, cams (N*V, CAM_RECORD), rgb (N*V, 3, H, H), depth
    (N*V, Pd, Pd), all contiguous on one GPU -> (texture (N, 3, A, A), views (N, A, A), best (N, A, A)).  No host synchronisation."""
    import ctypes
    L = hip.lib()
    dev = vertices.device
    hip._req(vertices), hip._req(cams), hip._req(rgb), hip._req(depth)
    hip._req(faces, torch.int32), hip._req(vertex_start, torch.int32), hip._req(face_start, torch.int32)
    if colors is not None:
        hip._req(colors)
    texture = torch.empty(N, 3, A, A, dtype=torch.float32, device=dev)
    views, best = (torch.empty(N, A, A, dtype=torch.uint8, device=dev) for _ in range(2))
    hip.check(L.mvd_texture_bake(_p(vertices), _p(colors), _p(faces), hip.ptr(vertex_start), hip.ptr(face_start), hip.ptr(cams), hip.ptr(rgb),
                                 hip.ptr(depth), int(vertices.shape[0]), int(faces.shape[0]), N, V, int(rgb.shape[-1]), int(depth.shape[-1]),
                                 texels, A, float(tol), float(min_cos), int(power), int(cull), blend, float(znear),
                                 (ctypes.c_float * 3)(*fill), hip.ptr(texture), hip.ptr(views), hip.ptr(best), hip.stream()))
    return texture, views, best


def _sample(face, bary, face_start, texture, nface, N, M, P, filter, background):
    """The one enqueue of mvd_texture_sample on ``_raster``'s face and bary -> rgb (N*M, 3, P, P)."""
    import ctypes
    L = hip.lib()
    image = texture.image.reshape(N, 3, texture.side, texture.side).to(face.device, torch.float32).contiguous()
    rgb = torch.empty(N * M, 3, P, P, dtype=torch.float32, device=face.device)
    hip._req(bary), hip._req(face, torch.int32), hip._req(face_start, torch.int32)
    hip.check(L.mvd_texture_sample(hip.ptr(face), hip.ptr(bary), hip.ptr(face_start), hip.ptr(image), int(nface), N, M, P, texture.texels,
                                   texture.side, filter, (ctypes.c_float * 3)(*background), hip.ptr(rgb), hip.stream()))
    return rgb


def bake_texture(mesh, rgb, cameras, texels=8, depth=None, size=None, tolerance=None, min_cos=0.1, power=2, blend="mean", cull=True,
                 fill=(0.5, 0.5, 0.5), znear=1e-3):
    """Texture a TriangleMesh from views of it (include/mvd_hip.h: mvd_texture_bake has the rule in full) -> MeshTexture.

    Every face gets a chart of its own in a closed-form atlas -- a right triangle with legs of ``texels`` texel intervals, two to a
    cell -- so simplify first (``simplify_mesh``): the atlas has about (texels + 3)^2 / 2 texels per face.  Every texel takes the world
    point its barycentrics name, projects it into every view and blends the colours of the views that see it.
    rgb, cameras : as ``fuse_views`` takes them -- (V, 3, H, H) in [0, 1] with the V cameras for a one-scene mesh, or (N, V, 3, H, H)
              with a list of N camera sets for an N-scene mesh.  V <= 254.
    depth   : what each view sees of the surface, (.., V, Pd, Pd), empty pixels not finite.  None renders the mesh into the same cameras
              at ``size`` (default H) pixels.  A given depth is taken as it is -- the model's own depth maps, say, which then act as a
              consistency gate.  A view sees a texel when the texel's camera z is at most the depth of the pixel it falls into plus
              ``tolerance`` (default TAU_FRACTION * DEPTH_SCALE, in world units); a texel over an empty depth pixel is not seen.
    min_cos, power, cull : a view contributes where the cosine between the face normal and the direction to the camera exceeds min_cos
              (cull=False: its absolute value), with the weight cosine^power (an integer in [0, 8]; 0 weighs the views equally).
    blend   : "mean" the weighted mean of the contributing views, "best" the colour of the view of the largest weight.
    fill    : what a texel of no face holds; a texel of a face no view contributes to holds the interpolated vertex colours when the
              mesh has colour, else fill.  MeshTexture.views says which.

    tolerance, min_cos and power are INTERFACE defaults: no trained checkpoint was available when this was written, so nobody has tuned
    them on real samples -- expect to.  No seam handling beyond the gutter texel of every chart, no mip-maps, no inpainting of unseen
    texels, no exposure matching.  The same bits run to run, and for a scene alone or in a batch baked at the same side.  No host
    synchronisation: the atlas side comes from the mesh's own host tables."""
    vertices, faces, colors, scenes = _check_mesh(mesh)
    if not torch.is_tensor(rgb) or rgb.dim() not in (4, 5):
        raise ValueError("rgb must be a (V, 3, H, H) or (N, V, 3, H, H) tensor")
    single = rgb.dim() == 4
    if single:
        if isinstance(cameras, (list, tuple)):
            raise ValueError("(V, 3, H, H) images take one camera set, not a list")
        rgb, cameras = rgb[None], [cameras]
        if torch.is_tensor(depth) and depth.dim() == 3:
            depth = depth[None]
    elif not isinstance(cameras, (list, tuple)) or len(cameras) != rgb.shape[0]:
        raise ValueError(f"(N, V, 3, H, H) images take a list of N = {rgb.shape[0]} camera sets")
    N, V, Cn, H, H2 = rgb.shape
    if Cn != 3 or H != H2 or H < 1:
        raise ValueError(f"rgb of shape {tuple(rgb.shape)}: need 3 channels and a square image")
    if not 1 <= V <= hip.TEX_MAX_VIEWS:
        raise ValueError(f"V = {V} views outside [1, {hip.TEX_MAX_VIEWS}]")
    if N != scenes:
        raise ValueError(f"cameras: {N} camera set(s) for a mesh of {scenes} scene(s)" + (" (pass a list of sets)" if single else ""))
    sets = [_as_cameras(c) for c in cameras]
    if any(len(c) != V for c in sets):
        raise ValueError(f"cameras: {[len(c) for c in sets]} cameras for {N} x {V} views")
    if blend not in TEX_BLENDS:
        raise ValueError(f"blend = {blend!r}: one of {sorted(TEX_BLENDS)}")
    if int(power) != power or not 0 <= power <= 8:
        raise ValueError(f"power = {power}: an integer in [0, 8]")
    min_cos, znear = float(min_cos), float(znear)
    if not 0 <= min_cos < 1:
        raise ValueError(f"min_cos = {min_cos} outside [0, 1)")
    if not znear >= 0:
        raise ValueError(f"znear = {znear}: >= 0")
    if cull not in (True, False, 0, 1):
        raise ValueError(f"cull = {cull}: True or False")
    tol = TAU_FRACTION * DEPTH_SCALE if tolerance is None else float(tolerance)
    if not 0 <= tol < math.inf:
        raise ValueError(f"tolerance = {tol}: finite, >= 0")
    fill = tuple(float(v) for v in fill)
    if len(fill) != 3:
        raise ValueError(f"fill = {fill}: three floats")
    counts = tuple(int(n) for n in (mesh.face_start[1:] - mesh.face_start[:-1]))
    C, A = atlas_layout(max(counts), texels, N)
    T = int(texels)
    if depth is not None:
        if not torch.is_tensor(depth) or depth.dim() != 4 or tuple(depth.shape[:2]) != (N, V) or depth.shape[2] != depth.shape[3]:
            raise ValueError(f"depth of shape {tuple(depth.shape) if torch.is_tensor(depth) else depth}: need (.., V, Pd, Pd) with the images' "
                             "leading dimensions")
    Pd = H if size is None else size
    if depth is None and (int(Pd) != Pd or Pd < 1 or N * V * Pd * Pd >= 2 ** 31 or N * V > 65535):
        raise ValueError(f"size = {Pd}: an integer >= 1 with N * V * size^2 < 2^31 and N * V <= 65535")
    dev = vertices.device
    vertices = vertices.float().contiguous()
    faces = faces.to(dev).contiguous()
    colors = None if colors is None else colors.to(dev, torch.float32).contiguous()
    vertex_start, face_start = (t.to(torch.int32).to(dev).contiguous() for t in (mesh.vertex_start, mesh.face_start))
    cams = pack_cameras(_cat_cameras(sets)).to(dev).contiguous()
    if depth is None:
        depth = _raster(vertices, None, faces, vertex_start, face_start, cams, N, V, int(Pd), bool(cull), znear, float("inf"), fill)[1]
    else:
        depth = depth.reshape(N * V, depth.shape[-1], depth.shape[-1]).to(dev, torch.float32).contiguous()
    image = rgb.reshape(N * V, 3, H, H).to(dev, torch.float32).contiguous()
    texture, views, best = _bake(vertices, colors, faces, vertex_start, face_start, cams, image, depth, N, V, T, A, tol, min_cos, int(power),
                                 bool(cull), TEX_BLENDS[blend], znear, fill)
    if single:
        texture, views, best = texture[0], views[0], best[0]
    return MeshTexture(image=texture, views=views, best=best, texels=T, cells_per_row=C, side=A, faces=counts)


def sample_texture(rendered, mesh, texture, filter="bilinear", background=(1.0, 1.0, 1.0)):
    """The RenderedMesh ``rendered`` of ``mesh`` with its rgb looked up in ``texture`` (mvd_texture_sample): what
    ``render_mesh(mesh, cameras, texture=texture)`` returns, for a render that already exists.  No host synchronisation."""
    import dataclasses
    _, faces, _, scenes = _check_mesh(mesh)
    _check_texture(texture, scenes, filter)
    if not isinstance(rendered, RenderedMesh):
        raise ValueError("rendered must be a RenderedMesh")
    background = tuple(float(v) for v in background)
    if len(background) != 3:
        raise ValueError(f"background = {background}: three floats")
    single = rendered.face.dim() == 3
    N = 1 if single else int(rendered.face.shape[0])
    if N != scenes:
        raise ValueError(f"rendered: {N} scene(s), the mesh has {scenes}")
    M, P = int(rendered.face.shape[-3]), int(rendered.face.shape[-1])
    dev = rendered.face.device
    face = rendered.face.reshape(N * M, P, P).contiguous()
    bary = rendered.bary.reshape(N * M, 3, P, P).contiguous()
    rgb = _sample(face, bary, mesh.face_start.to(torch.int32).to(dev).contiguous(), texture, int(faces.shape[0]), N, M, P, TEX_FILTERS[filter],
                  background)
    out = dataclasses.replace(rendered, rgb=rgb.reshape(*rendered.bary.shape))
    if "_depth_map" in vars(rendered):
        out._depth_map = rendered._depth_map
    return out


def _png(image):
    """An (h, w, 3) uint8 array as the bytes of an 8-bit RGB PNG (zlib + struct: no imaging library)."""
    import struct
    import zlib
    h, w = int(image.shape[0]), int(image.shape[1])
    chunk = lambda tag, data: struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    rows = b"".join(b"\x00" + image[y].tobytes() for y in range(h))
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows, 6)) + \
        chunk(b"IEND", b"")


def write_obj(path, mesh, texture, scene=None):
    """A textured mesh as Wavefront OBJ: ``path`` (v, three vt per face, f a/ta b/tb c/tc, 1-based), ``path + ".mtl"`` (map_Kd) and the
    texture as an 8-bit RGB PNG next to it (round(255 clip(image)), row 0 on top).  One scene per file: a mesh of several takes
    ``scene=``."""
    import os
    import numpy as np
    _, _, _, scenes = _check_mesh(mesh)
    _check_texture(texture, scenes, "bilinear")
    if scenes > 1 and scene is None:
        raise ValueError(f"write_obj: a mesh of {scenes} scenes takes scene=")
    s = 0 if scene is None else int(scene)
    if not 0 <= s < scenes:
        raise ValueError(f"scene {scene} of a mesh of {scenes} scene(s)")
    f0 = int(mesh.face_start[s])
    sub = mesh.scene(s)
    uv = texture.uv(mesh)[f0:f0 + len(sub)].reshape(-1, 2).numpy()
    image = texture.image if texture.image.dim() == 3 else texture.image[s]
    pixels = np.rint(np.clip(image.detach().cpu().numpy(), 0.0, 1.0) * 255.0).astype("u1").transpose(1, 2, 0)
    stem = os.path.splitext(os.path.basename(path))[0]
    png, mtl = os.path.splitext(path)[0] + ".png", path + ".mtl"
    with open(png, "wb") as fh:
        fh.write(_png(np.ascontiguousarray(pixels)))
    with open(mtl, "w") as fh:
        fh.write(f"newmtl {stem}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {os.path.basename(png)}\n")
    v = sub.vertices.detach().cpu().numpy()
    f = sub.faces.detach().cpu().numpy().astype("i8") + 1
    lines = [f"mtllib {os.path.basename(mtl)}", f"usemtl {stem}"]
    lines += [f"v {x:.9g} {y:.9g} {z:.9g}" for x, y, z in v]
    lines += [f"vt {a:.9g} {b:.9g}" for a, b in uv]
    lines += [f"f {a}/{3 * k + 1} {b}/{3 * k + 2} {c}/{3 * k + 3}" for k, (a, b, c) in enumerate(f)]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
