#!/usr/bin/env python
"""Texturing a mesh from views (mvd_texture_bake, mvd_texture_sample; mvdfusion_amd/fusion.py bake_texture) next to the same rule in
torch ops.

One workload = (mesh, V views, texels) at H = Pd = 256 from bench_render's ring rig.  Meshes: bench_mesh_render's exact sphere at G^3
voxels, G in {64, 128}, as extracted and after simplify_mesh(cells=64).  The views are render_mesh of the mesh itself with its
position-derived vertex colours; the depth maps are the same renders' depth.  One JSON line per workload:
  us_per_bake           one mvd_texture_bake call (all outputs)
  us_per_bake_torch     the header's rule with torch ops on the same device, view after view over the owned texels (MEAN blend)
  side, owned_share     the atlas side A and the share of its A^2 texels that a face owns
  coverage              the share of the owned texels at least one view contributed to
  max_abs_diff          max|kernel - torch| of the texture (two fp32 evaluations; not asserted)
and one line per (mesh, M) for the lookup at P = 256:
  us_per_sample         one mvd_texture_sample call on the rasteriser's face and bary, bilinear
Every figure is the median over --blocks blocks of HIP-event times on torch's current stream, after a warm-up; a block is --reps calls
between two events.  min / max give the spread.  Nothing is asserted.

  python tools/bench_texture.py
  python tools/bench_texture.py --grid 64 --views 8 --texels 8

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

from bench_mesh_render import sphere_mesh          # noqa: E402
from bench_render import _event_blocks, ring_rig   # noqa: E402

FILL = (0.5, 0.5, 0.5)


def torch_bake(mesh, cams, rgb, depth, T, C, tol, min_cos, power, znear):
    """mvd_texture_bake's rule (cull 1, MEAN, one scene) with torch ops: (texture (3, A, A), views (A, A))."""
    import torch
    from mvdfusion_amd import fusion
    dev, A, V, H, Pd = mesh.vertices.device, C * (T + 3), rgb.shape[0], rgb.shape[-1], depth.shape[-1]
    l, ci, cj, owned = fusion._chart_of_texel(T, C, dev)
    own = owned & (l < len(mesh))
    y, x = torch.nonzero(own, as_tuple=True)
    P3 = mesh.vertices[mesh.faces[l[y, x]].long()]
    bb, bc = ci[y, x].float() / T, cj[y, x].float() / T
    ba = (1.0 - bb) - bc
    X = (ba[:, None] * P3[:, 0] + bb[:, None] * P3[:, 1]) + bc[:, None] * P3[:, 2]
    c3 = mesh.rgb[mesh.faces[l[y, x]].long()]
    fallback = (ba[:, None] * c3[:, 0] + bb[:, None] * c3[:, 1]) + bc[:, None] * c3[:, 2]
    n = torch.linalg.cross(P3[:, 1] - P3[:, 0], P3[:, 2] - P3[:, 0])
    nlen = (n * n).sum(1).sqrt()
    sw, sc, views = torch.zeros_like(nlen), torch.zeros_like(X), torch.zeros_like(nlen, dtype=torch.uint8)
    for v in range(V):
        R, Tv, f, p = cams.R[v].to(dev), cams.T[v].to(dev), cams.focal_length[v].to(dev), cams.principal_point[v].to(dev)
        xc = X @ R + Tv
        zc = xc[:, 2]
        u, w = f[0] * xc[:, 0] / zc + p[0], f[1] * xc[:, 1] / zc + p[1]
        cx, cy = (1.0 - u) * (0.5 * Pd) - 0.5, (1.0 - w) * (0.5 * Pd) - 0.5
        ok = (zc > znear) & (cx >= -0.5) & (cx <= Pd - 0.5) & (cy >= -0.5) & (cy <= Pd - 0.5)
        dx, dy = (cx + 0.5).floor().clamp(0, Pd - 1).long(), (cy + 0.5).floor().clamp(0, Pd - 1).long()
        d = depth[v, dy, dx]
        cosv = -((n @ R) * xc).sum(1) / (nlen * xc.norm(dim=1))
        ok &= torch.isfinite(d) & (zc <= d + tol) & (cosv > min_cos)
        wt = cosv ** power if power else torch.ones_like(cosv)
        ix, iy = ((1.0 - u) * (0.5 * H) - 0.5).clamp(0, H - 1), ((1.0 - w) * (0.5 * H) - 0.5).clamp(0, H - 1)
        x0, y0 = ix.floor().long(), iy.floor().long()
        x1, y1, wx, wy = (x0 + 1).clamp(max=H - 1), (y0 + 1).clamp(max=H - 1), (ix - ix.floor())[None], (iy - iy.floor())[None]
        img = rgb[v]
        col = (img[:, y0, x0] * (1 - wx) + img[:, y0, x1] * wx) * (1 - wy) + (img[:, y1, x0] * (1 - wx) + img[:, y1, x1] * wx) * wy
        wt = torch.where(ok, wt, torch.zeros_like(wt))
        sw, sc, views = sw + wt, sc + wt[:, None] * torch.nan_to_num(col.t()), views + ok.to(torch.uint8)
    seen = views > 0
    value = torch.where(seen[:, None], sc / sw.clamp(min=1e-30)[:, None], fallback)
    tex = torch.tensor(FILL, device=dev).reshape(3, 1, 1).expand(3, A, A).clone()
    tex[:, y, x] = value.t()
    out_views = torch.zeros(A, A, dtype=torch.uint8, device=dev)
    out_views[y, x] = views
    return tex, out_views


def run_bake(name, mesh, G, V, T, P, blocks, reps):
    import torch
    from mvdfusion_amd import fusion, hip
    from mvdfusion_amd.cameras import pack_cameras
    L, dev, p = hip.lib(), "cuda", hip.ptr
    rig = ring_rig(V)
    src = fusion.render_mesh(mesh, rig, size=P)
    rgb, depth = src.rgb.contiguous(), src.depth.contiguous()
    C, A = fusion.atlas_layout(len(mesh), T)
    cams = pack_cameras(rig).to(dev)
    vstart, fstart = mesh.vertex_start.to(dev), mesh.face_start.to(dev)
    tex = torch.empty(1, 3, A, A, device=dev)
    views, best = (torch.empty(1, A, A, dtype=torch.uint8, device=dev) for _ in range(2))
    tol, min_cos, power, znear = fusion.TAU_FRACTION * fusion.DEPTH_SCALE, 0.1, 2, 1e-3
    fill = (ctypes.c_float * 3)(*FILL)

    def bake():
        hip.check(L.mvd_texture_bake(p(mesh.vertices), p(mesh.rgb), p(mesh.faces), p(vstart), p(fstart), p(cams), p(rgb), p(depth),
                                     int(mesh.vertices.shape[0]), len(mesh), 1, V, P, P, T, A, tol, min_cos, power, 1, hip.TEX_MEAN, znear, fill,
                                     p(tex), p(views), p(best), hip.stream()))

    t_bake = _event_blocks(bake, blocks, reps)
    ref = {}

    def rule():
        ref["tex"], ref["views"] = torch_bake(mesh, rig, rgb, depth, T, C, tol, min_cos, power, znear)

    t_torch = _event_blocks(rule, 3, 1)
    bake()
    torch.cuda.synchronize()
    per_face = (T + 1) * (T + 2) // 2 + T
    owned = len(mesh) * per_face
    res = dict(metric="texture_bake", mesh=name, G=G, faces=len(mesh), V=V, texels=T, H=P, Pd=P, side=A, owned_share=round(owned / (A * A), 4),
               coverage=round(int((views > 0).sum()) / max(owned, 1), 4), views_agree=round(float((views[0] == ref["views"]).float().mean()), 6),
               max_abs_diff=float((tex[0] - ref["tex"])[:, views[0] == ref["views"]].abs().max()))
    for key, t in (("us_per_bake", t_bake), ("us_per_bake_torch", t_torch)):
        res.update({key: t["med"], key + "_min": t["min"], key + "_max": t["max"]})
    res.update(blocks=blocks, reps=reps, lib=os.path.basename(hip.LIB_PATHS[hip.OPERAND_FORMAT]), gpu=torch.cuda.get_device_name(0))
    return res, fusion.MeshTexture(image=tex[0].clone(), views=views[0].clone(), best=best[0].clone(), texels=T, cells_per_row=C, side=A,
                                   faces=(len(mesh),))


def run_sample(name, mesh, G, texture, M, P, blocks, reps):
    import torch
    from mvdfusion_amd import fusion, hip
    L, dev, p = hip.lib(), "cuda", hip.ptr
    r = fusion.render_mesh(mesh, ring_rig(M), size=P)
    face, bary = r.face.contiguous(), r.bary.contiguous()
    fstart = mesh.face_start.to(dev)
    image = texture.image[None].contiguous()
    rgb = torch.empty(M, 3, P, P, device=dev)
    bg = (ctypes.c_float * 3)(1.0, 1.0, 1.0)

    def sample():
        hip.check(L.mvd_texture_sample(p(face), p(bary), p(fstart), p(image), len(mesh), 1, M, P, texture.texels, texture.side, hip.TEX_BILINEAR, bg,
                                       p(rgb), hip.stream()))

    t = _event_blocks(sample, blocks, reps)
    return dict(metric="texture_sample", mesh=name, G=G, faces=len(mesh), M=M, P=P, texels=texture.texels, side=texture.side,
                hit_share=round(float(r.hit.float().mean()), 3), us_per_sample=t["med"], us_per_sample_min=t["min"], us_per_sample_max=t["max"],
                blocks=blocks, reps=reps, gpu=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--views", type=int, nargs="*", default=[8, 24])
    ap.add_argument("--texels", type=int, nargs="*", default=[4, 8])
    ap.add_argument("--cameras", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if a.blocks < 3:
        ap.error("--blocks must be >= 3")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_texture: no GPU visible (there is no CPU path)")
    from mvdfusion_amd import fusion
    for G in a.grid:
        full = sphere_mesh(G)
        for name, mesh in (("sphere", full), (f"sphere_simplify{a.cells}", fusion.simplify_mesh(full, cells=a.cells))):
            texture = None
            for V in a.views:
                for T in a.texels:
                    res, texture = run_bake(name, mesh, G, V, T, a.size, a.blocks, a.reps)
                    print(json.dumps(res), flush=True)
            for M in a.cameras:
                print(json.dumps(run_sample(name, mesh, G, texture, M, a.size, a.blocks, a.reps * 5)), flush=True)


if __name__ == "__main__":
    main()
