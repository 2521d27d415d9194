// The GridAttn point geometry, shared by the three kernels that walk it (gridattn.hip: tokens_kernel and its backward tokens_bwd_kernel;
// gridattn_fused.hip: g4_fused_kernel): launch arguments (GridGeom) and their host-side check, the decode of a 3-D point index, the depth
// sample -> ray -> world point, the rule that maps a point's reference view slots to views, camera records with PyTorch3D-convention
// unproject / project, Plucker coordinates, and the grid_sample(bilinear, border, align_corners) taps.  The backward scatters with the
// forward's taps and the fused kernel must see the unfused kernel's point bit for bit: both hold because there is one copy, here.
//
// Deliberately NOT shared: the sin / cos of the harmonic embedding.  tokens_kernel (harmonic() in gridattn.hip) calls ocml's sinf / cosf;
// the fused kernel (token_embedding() / sincos_sel in gridattn_fused.hip) has a branch-free Cody-Waite version, because ocml's
// large-argument path drags scratch memory into a kernel that has no register to spare.  The two produce different bits; merging them
// changes the results of one kernel or the resources of the other.
#pragma once
#include "common.hpp"
#include "../../include/mvd_hip.h"

namespace {

// The launch arguments common to the three kernels; filled once per entry point.
struct GridGeom {
  const float *x, *depth_noise, *steps;
  const int* iter;
  const float *grid_lin, *cams, *in_cam;
  int nscene, V, q0, Vq, S, D;      // scenes; views per rig; query views [q0, q0 + Vq) of every rig; S x S pixels; D depth samples per pixel
  float depth_scale, depth_shift;
  int steps_scene_stride, window;   // scene n: step row *iter + n * steps_scene_stride; window: 0 = all V views, else W (odd) rig neighbours
};

// reference view slots (token rows) per 3-D point, and the points of a launch
__host__ __device__ inline int slots_per_point(const GridGeom& g) { return g.window ? g.window : g.V; }
__host__ __device__ inline size_t num_points(const GridGeom& g) { return (size_t)g.nscene * g.Vq * g.S * g.S * g.D; }
// THE window rule: slot j of query view b is view (b + j - W/2) mod V of b's rig (host: the fused kernel's offset table, with b = 0)
__host__ __device__ inline int window_view(int b, int j, int W, int V) { return ((b + j - W / 2) % V + V) % V; }

// The shared arguments, checked on behalf of entry point `fn` before it launches anything (its own arguments it checks itself).
inline int check_geom(const char* fn, const GridGeom& g) {
  MVD_CHECK_ARG(g.x && g.depth_noise && g.steps && g.iter && g.grid_lin && g.cams && g.in_cam, "%s: null pointer", fn);
  MVD_CHECK_ARG(g.nscene >= 1, "%s: nscene=%d (>= 1)", fn, g.nscene);
  MVD_CHECK_ARG(g.steps_scene_stride >= 0 && (g.nscene > 1 || g.steps_scene_stride == 0),
                "%s: steps_scene_stride=%d (>= 0; 0 when nscene = 1)", fn, g.steps_scene_stride);
  MVD_CHECK_ARG(g.window == 0 || (g.window >= 1 && (g.window & 1)), "%s: window=%d (0 = all views, else odd)", fn, g.window);
  MVD_CHECK_ARG(g.V > 0 && slots_per_point(g) <= 16, "%s: %d rows per point outside [1, 16] (V=%d, window=%d)", fn, slots_per_point(g), g.V,
                g.window);
  MVD_CHECK_ARG(g.S > 1 && g.D > 0, "%s: bad shape S=%d, D=%d", fn, g.S, g.D);
  MVD_CHECK_ARG(g.q0 >= 0 && g.Vq > 0 && g.q0 + g.Vq <= g.V, "%s: bad query-view range [%d, %d) of %d", fn, g.q0, g.q0 + g.Vq, g.V);
  MVD_CHECK_ARG((size_t)g.nscene * g.V <= 0x7fffffff, "%s: grid too large", fn);
  return 0;
}

// A 3-D point of the launch: points are ordered (scene, query view, pixel, depth sample), like the token rows.
struct GeomPoint {
  int scene, b, pix, d;   // b: index of the query view inside its scene's rig
  int gv0;                // global index of the scene's view 0
  size_t srow, noise;     // the scene's step row (its own timestep); index of the point's depth noise (which stays at *iter)
};
// the scene of point pt where one wavefront owns the point (so the result is a scalar); the fused kernel takes it from blockIdx.x instead
__device__ __forceinline__ int wave_scene(const GridGeom& g, size_t pt) {
  return __builtin_amdgcn_readfirstlane((int)(pt / ((size_t)g.D * g.S * g.S)) / g.Vq);
}
__device__ __forceinline__ GeomPoint decode_point(const GridGeom& g, size_t pt, int scene) {
  const int SS = g.S * g.S;
  GeomPoint q;
  q.scene = scene;
  q.d = (int)(pt % g.D);
  q.pix = (int)((pt / g.D) % SS);
  q.b = g.q0 + (int)(pt / ((size_t)g.D * SS)) - scene * g.Vq;
  q.gv0 = scene * g.V;
  const int it = g.iter[0];
  q.srow = (size_t)it + (size_t)scene * g.steps_scene_stride;
  q.noise = (((size_t)it * g.nscene * g.V + q.gv0 + q.b) * g.D + q.d) * SS + q.pix;
  return q;
}

// calls f(slot, view) for the reference view slots of a point of query view b: all V views in order, or the window's W neighbours
template <class F>
__device__ __forceinline__ void for_each_slot(const GridGeom& g, int b, F&& f) {
  const int W = slots_per_point(g);
  int vr = g.window ? window_view(b, 0, W, g.V) : 0;
  for (int slot = 0; slot < W; ++slot, vr = vr + 1 == g.V ? 0 : vr + 1) f(slot, vr);
}

struct Cam {
  float R[9], T[3], f[2], p[2], C[3];
};

__device__ __forceinline__ Cam load_cam(const float* rec) {
  Cam c;
#pragma unroll
  for (int i = 0; i < 9; ++i) c.R[i] = rec[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) c.T[i] = rec[9 + i];
  c.f[0] = rec[12];
  c.f[1] = rec[13];
  c.p[0] = rec[14];
  c.p[1] = rec[15];
#pragma unroll
  for (int i = 0; i < 3; ++i) c.C[i] = rec[16 + i];
  return c;
}
// camera of view `view` of the point's rig / of the point's input view
__device__ __forceinline__ Cam view_cam(const GridGeom& g, const GeomPoint& q, int view) {
  return load_cam(g.cams + (size_t)(q.gv0 + view) * MVD_CAM_RECORD);
}
__device__ __forceinline__ Cam input_cam(const GridGeom& g, const GeomPoint& q) { return load_cam(g.in_cam + (size_t)q.scene * MVD_CAM_RECORD); }

// X_world = (X_cam - T) R^T  with X_cam = ((x-px) d / fx, (y-py) d / fy, d)   (pytorch3d unproject_points)
__device__ __forceinline__ void unproject(const Cam& c, float x, float y, float d, float* w) {
  const float xc[3] = {(x - c.p[0]) * d / c.f[0] - c.T[0], (y - c.p[1]) * d / c.f[1] - c.T[1], d - c.T[2]};
#pragma unroll
  for (int j = 0; j < 3; ++j) w[j] = xc[0] * c.R[j * 3 + 0] + xc[1] * c.R[j * 3 + 1] + xc[2] * c.R[j * 3 + 2];
}

// ndc = (fx X/Z + px, fy Y/Z + py) with X_cam = X R + T   (pytorch3d transform_points_ndc)
__device__ __forceinline__ void project(const Cam& c, const float* X, float& u, float& v) {
  float xc[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) xc[j] = X[0] * c.R[0 * 3 + j] + X[1] * c.R[1 * 3 + j] + X[2] * c.R[2 * 3 + j] + c.T[j];
  u = c.f[0] * xc[0] / xc[2] + c.p[0];
  v = c.f[1] * xc[1] / xc[2] + c.p[1];
}

// G1: depth sample and world point of q, seen from its query view's camera cb (view_attn_efficient2.py:419-432, ray_utils.py:175-202,367-369):
// the x0-estimate of the depth channel plus noise, clamped and scaled, along the ray through the pixel.  Returns the depth; X = world
// point, dir = ray direction (unnormalised).
__device__ __forceinline__ float world_point(const GridGeom& g, const GeomPoint& q, const Cam& cb, float* X, float* dir) {
  const int S = g.S, SS = S * S;
  const float sqrt_ac = g.steps[q.srow * MVD_STEP_STRIDE + 1];
  const float dstd = g.steps[q.srow * MVD_STEP_STRIDE + 2];
  const float dch = g.x[((size_t)(q.gv0 + q.b) * 5 + 4) * SS + q.pix] / sqrt_ac;
  const float smp = dch + dstd * g.depth_noise[q.noise];
  const float depth = fminf(fmaxf((smp + 1.0f) / 2.0f, 0.f), 1.f) * g.depth_scale + g.depth_shift;
  const float ndx = g.grid_lin[q.pix % S], ndy = g.grid_lin[q.pix / S];
  float p1[3], p2[3];
  unproject(cb, ndx, ndy, 1.f, p1);
  unproject(cb, ndx, ndy, 2.f, p2);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    dir[j] = p2[j] - p1[j];
    const float org = p1[j] - dir[j];
    X[j] = org + depth * dir[j];
  }
  return depth;
}

// Plucker coordinates (unit direction | C x direction) of the ray with direction (dx, dy, dz) through camera centre C, and the
// direction's norm (view_attn_efficient2.py:344-362).  Named members, not an array: the fused kernel selects among them (pick6) and must
// never index them at run time -- that would put them in scratch memory.
struct Plucker {
  float a, b, c, d, e, f, norm;
};
__device__ __forceinline__ Plucker plucker(float dx, float dy, float dz, const float* C) {
  Plucker r;
  r.norm = sqrtf(dx * dx + dy * dy + dz * dz);
  const float nn = fmaxf(r.norm, 1e-12f);
  r.a = dx / nn;
  r.b = dy / nn;
  r.c = dz / nn;
  r.d = C[1] * r.c - C[2] * r.b;
  r.e = C[2] * r.a - C[0] * r.c;
  r.f = C[0] * r.b - C[1] * r.a;
  return r;
}
// of the ray from camera c's centre to the world point X (norm = the point's distance)
__device__ __forceinline__ Plucker plucker_to(const Cam& c, const float* X) { return plucker(X[0] - c.C[0], X[1] - c.C[1], X[2] - c.C[2], c.C); }

// F.grid_sample(bilinear, padding_mode='border', align_corners=True) at grid (gx, gy) of an S x S map: the four taps' pixel indices
// y * S + x and weights.  A tap beyond the border (weight 0 by construction, but its pixel is outside the map) has pix = -1 for consumers
// that skip it (bilinear4, the backward's scatter4), or with kZeroWeight pixel 0 and weight exactly 0 for the branch-free fused kernel.
struct Taps {
  int pix[4];
  float w[4];
};
template <bool kZeroWeight = false>
__device__ __forceinline__ Taps bilinear_taps(int S, float gx, float gy) {
  float ix = ((gx + 1.f) / 2.f) * (float)(S - 1);
  float iy = ((gy + 1.f) / 2.f) * (float)(S - 1);
  ix = fminf(fmaxf(ix, 0.f), (float)(S - 1));
  iy = fminf(fmaxf(iy, 0.f), (float)(S - 1));
  if (!(ix == ix)) ix = 0.f;  // NaN coordinates (z ~ 0): stay in bounds
  if (!(iy == iy)) iy = 0.f;
  const float x0f = floorf(ix), y0f = floorf(iy);
  const int x0 = (int)x0f, y0 = (int)y0f;
  const int x1 = x0 + 1, y1 = y0 + 1;
  const float wx1 = ix - x0f, wy1 = iy - y0f;
  const float wx0 = (x0f + 1.f) - ix, wy0 = (y0f + 1.f) - iy;
  const int ys[4] = {y0, y0, y1, y1}, xs[4] = {x0, x1, x0, x1};
  const float ws[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};
  Taps t;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool ok = ys[k] < S && xs[k] < S;
    t.pix[k] = ok ? ys[k] * S + xs[k] : (kZeroWeight ? 0 : -1);
    t.w[k] = ok || !kZeroWeight ? ws[k] : 0.f;
  }
  return t;
}
// the taps of world point X in the S x S feature map of camera c (the reference's NDC axes point the other way: grid = -ndc)
template <bool kZeroWeight = false>
__device__ __forceinline__ Taps view_taps(const Cam& c, const float* X, int S) {
  float u, v;
  project(c, X, u, v);
  return bilinear_taps<kZeroWeight>(S, -u, -v);
}

// the bilinear sample of 4 consecutive channels of a channels-last 256-channel map
__device__ __forceinline__ float4 bilinear4(const float* __restrict__ fmap, const Taps& t, int ch) {
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (t.pix[k] < 0) continue;
    const float4 v = *(const float4*)(fmap + (size_t)t.pix[k] * 256 + ch);
    o.x += v.x * t.w[k];
    o.y += v.y * t.w[k];
    o.z += v.z * t.w[k];
    o.w += v.w * t.w[k];
  }
  return o;
}

}  // namespace
