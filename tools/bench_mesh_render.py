#!/usr/bin/env python
"""Mesh rendering (mvd_render_mesh, mvdfusion_amd/fusion.py render_mesh) next to what a user had until now: render_points of the same
mesh's vertices at radius 1.

One workload = (mesh, M cameras, cull) at P = 256 from bench_render's ring rig (distance 1.5, elevation 30 degrees, M azimuths).  Meshes:
`sphere` -- extract_mesh of the exact signed distance |X| - 0.6 at G^3 voxels in the default box, G in {64, 128}; `wall` -- 256 triangles
that each cover the whole image from outside it, at 256 depths, nearest last: the wavefront path and nothing else (M = 1, cull off).
One JSON line per workload:
  us_per_render         one mvd_render_mesh call: the z-buffer fill, the raster kernel and the resolve kernel
  us_per_raster         the raster kernel alone (mvd_render_mesh_stages; the z-buffer is refilled, untimed, before every launch)
  us_per_points         one mvd_render_points call on the mesh's vertices (with its colours) at radius 1
  empty_mesh, empty_points   the share of the pixels inside the silhouette -- the pixel's ray meets the sphere; for `wall` every pixel --
                        that each leaves empty
Every figure is the median over --blocks blocks of HIP-event times on torch's current stream, after a warm-up of every launch; a block
is --reps calls between two events (the raster kernel: an event pair around every launch, summed).  min / max give the spread.

  python tools/bench_mesh_render.py
  python tools/bench_mesh_render.py --grid 128 --cameras 8

There is no CPU path: without a GPU this exits with an error.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_render import _event_blocks, ring_rig          # noqa: E402

RADIUS = 0.6


def sphere_mesh(G):
    """extract_mesh of the exact SDF at the voxel centres of the default box (center 0, half_extent 0.75), with position-derived colours."""
    import torch
    from mvdfusion_amd import fusion
    ax = ((torch.arange(G, dtype=torch.float64) + 0.5) * (1.5 / G) - 0.75).cuda()
    zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
    mesh = fusion.extract_mesh(((xx ** 2 + yy ** 2 + zz ** 2).sqrt() - RADIUS).float())
    mesh.rgb = (mesh.vertices / (2 * RADIUS) + 0.5).clamp(0, 1).contiguous()
    return mesh


def wall_mesh(rig, P, count=256):
    """`count` triangles with all vertices outside camera 0's image, each covering it, at camera depths 2.5 down to 1.0."""
    import torch
    from mvdfusion_amd import fusion
    R, T, f, p = rig.R[0].double(), rig.T[0].double(), rig.focal_length[0].double(), rig.principal_point[0].double()
    px = torch.tensor([-1.5 * P, 2.5 * P, 0.5 * P], dtype=torch.float64)
    py = torch.tensor([-0.6 * P, -0.6 * P, 3.4 * P], dtype=torch.float64)
    z = torch.linspace(2.5, 1.0, count, dtype=torch.float64)[:, None].expand(count, 3)
    u, w = 1.0 - 2.0 * (px + 0.5) / P, 1.0 - 2.0 * (py + 0.5) / P
    xc = torch.stack([(u - p[0]) * z / f[0], (w - p[1]) * z / f[1], z], dim=-1).reshape(-1, 3)
    v = ((xc - T) @ torch.linalg.inv(R)).float().cuda()
    n = v.shape[0]
    return fusion.TriangleMesh(vertices=v, faces=torch.arange(n, dtype=torch.int32).reshape(-1, 3).cuda(), rgb=torch.rand(n, 3).cuda(),
                               vertex_start=torch.tensor([0, n], dtype=torch.int32), face_start=torch.tensor([0, n // 3], dtype=torch.int32))


def silhouette(rig, P):
    """(M, P, P) bool: the ray through the pixel centre meets the sphere."""
    import torch
    out = []
    lin = 1.0 - 2.0 * (torch.arange(P, dtype=torch.float64) + 0.5) / P
    w, u = torch.meshgrid(lin, lin, indexing="ij")
    for j in range(len(rig)):
        R, T, f, p = rig.R[j].double(), rig.T[j].double(), rig.focal_length[j].double(), rig.principal_point[j].double()
        d = torch.stack([(u - p[0]) / f[0], (w - p[1]) / f[1], torch.ones_like(u)], dim=-1) @ torch.linalg.inv(R)
        o = -T @ torch.linalg.inv(R)
        b, c = (d * o).sum(-1), (o * o).sum() - RADIUS ** 2
        out.append(b * b - (d * d).sum(-1) * c > 0)
    return torch.stack(out).cuda()


def run_one(name, mesh, rig, P, cull, inside, blocks, reps, extra):
    import torch
    from mvdfusion_amd import hip
    from mvdfusion_amd.cameras import pack_cameras
    L = hip.lib()
    dev, M = "cuda", len(rig)
    nvert, nface = int(mesh.vertices.shape[0]), len(mesh)
    cams = pack_cameras(rig).to(dev)
    vstart, fstart = mesh.vertex_start.to(dev), mesh.face_start.to(dev)
    face = torch.empty(M, P, P, dtype=torch.int32, device=dev)
    depth = torch.empty(M, P, P, device=dev)
    bary, normal, rgb = (torch.empty(M, 3, P, P, device=dev) for _ in range(3))
    nbytes = int(L.mvd_render_mesh_scratch(M, P))
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    bg = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    znear, p = 1e-3, hip.ptr
    args = [p(mesh.vertices), p(mesh.rgb), p(mesh.faces), p(vstart), p(fstart), p(cams), nvert, nface, 1, M, P, int(cull), znear, float("inf"), bg,
            p(face), p(depth), p(bary), p(normal), p(rgb), p(scratch), nbytes]

    def stages(which):
        hip.check(L.mvd_render_mesh_stages(*args, which, hip.stream()))

    def render():
        hip.check(L.mvd_render_mesh(*args, hip.stream()))

    pstart = torch.tensor([0, nvert], dtype=torch.int32).to(dev)
    index, pdepth, prgb = torch.empty(M, P, P, dtype=torch.int32, device=dev), torch.empty(M, P, P, device=dev), torch.empty(M, 3, P, P, device=dev)

    def points():
        hip.check(L.mvd_render_points(p(mesh.vertices), p(mesh.rgb), p(pstart), p(cams), nvert, 1, M, P, 1, znear, float("inf"), bg, p(index),
                                      p(pdepth), p(prgb), p(scratch), nbytes, hip.stream()))

    t_render = _event_blocks(render, blocks, reps)
    t_raster = _event_blocks(lambda: stages(hip.RENDER_SPLAT), blocks, reps, before=lambda: stages(hip.RENDER_FILL))
    t_points = _event_blocks(points, blocks, reps)
    render()
    points()
    torch.cuda.synchronize()
    n_in = max(int(inside.sum()), 1)
    res = dict(metric="render_mesh", mesh=name, faces=nface, vertices=nvert, M=M, P=P, cull=int(cull), **extra,
               hit_share=round(float((face >= 0).float().mean()), 3), empty_mesh=round(int(((face < 0) & inside).sum()) / n_in, 4),
               empty_points=round(int(((index < 0) & inside).sum()) / n_in, 4))
    for key, t in (("us_per_render", t_render), ("us_per_raster", t_raster), ("us_per_points", t_points)):
        res.update({key: t["med"], key + "_min": t["min"], key + "_max": t["max"]})
    res.update(blocks=blocks, reps=reps, lib=os.path.basename(hip.LIB_PATHS[hip.OPERAND_FORMAT]), gpu=torch.cuda.get_device_name(0))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--cameras", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--wall", type=int, default=256, help="triangles of the adversarial mesh (0: skip it)")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    if a.blocks < 3:
        ap.error("--blocks must be >= 3")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_render: no GPU visible (there is no CPU path)")
    P = a.size
    for G in a.grid:
        mesh = sphere_mesh(G)
        for M in a.cameras:
            rig = ring_rig(M)
            inside = silhouette(rig, P)
            for cull in (1, 0):
                print(json.dumps(run_one("sphere", mesh, rig, P, cull, inside, a.blocks, a.reps, dict(G=G))), flush=True)
    if a.wall:
        rig = ring_rig(1)
        everywhere = torch.ones(1, P, P, dtype=torch.bool, device="cuda")
        print(json.dumps(run_one("wall", wall_mesh(rig, P, a.wall), rig, P, 0, everywhere, a.blocks, max(a.reps // 10, 2), {})), flush=True)


if __name__ == "__main__":
    main()
