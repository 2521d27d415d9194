// Fusion of sampled RGB-D views into one depth-consistent point cloud (include/mvd_hip.h: mvd_fuse_points, mvd_compact_points).
//
// fuse_kernel: one thread per output point.  A point is pixel (Y, X) of the P x P grid (P = S * up) of view b of a scene; its depth is the
// latent depth of pixel (Y / up, X / up) -- nearest replication -- and its ray goes through the fine pixel's own centre.  The point is
// unprojected through its camera and reprojected into every other view of the rig, whose depth map votes: support (|dz| <= tau), conflict
// (dz < -tau: the point floats in front of the surface that view sees) or nothing (unseen, background under a tap, occluded).  All fp32,
// compiled without contraction; the geometry is gridattn_common.hpp's (Cam, load_cam, unproject) plus the projection below, which also
// returns camera-space z (fusion_common.hpp, shared with tsdf.hip).
//
// Two forms of the same kernel (bit-identical results): the default reads the depth maps from global memory (they are small and stay in
// L1 / L2; a wavefront reprojects into one view at a time, so its lanes hit neighbouring texels); kLds stages the scene's V normalised depth
// planes and camera records in LDS once per workgroup and walks the scene's points in a grid-stride loop.  Measured, the staged form is
// nowhere faster by more than 1 %: it stays selectable (MVD_FUSE_STAGE_LDS) and tested, and auto is the global form.
// A workgroup belongs to one scene (blockIdx.y), so the camera base is uniform.
//
// compact: count_kernel (per-wavefront 64-bit ballot + popcount, per-block count) -> scan_kernel (one workgroup loops over the block
// counts: exclusive offsets in place, total to *count) -> scatter_kernel (same ballots; rank = block offset + earlier wavefronts + popcount
// of the lower lanes).  No atomic decides an order: the output is the masked selection in point order, run to run.
//
// render (mvd_render_points): z-buffered point splatting of a cloud into M cameras per scene.  The z-buffer is filled with ones -> splat_kernel:
// one thread per (point, camera), project_z above, the centre pixel by the fuse kernel's pixel-centre convention, one 64-bit unsigned
// atomicMin of (depth bits << 32 | point position) per covered pixel -> resolve_kernel: one thread per pixel unpacks the winner.  The minimum
// of a set does not depend on the order its members arrive in: the outputs are the same bits run to run.
#include "fusion_common.hpp"

namespace {

constexpr int kFuseThreads = 512;
constexpr size_t kFuseLdsMax = 128 * 1024;            // of the CU's 160 KiB: V = 24, S = 32 is 98 KiB
constexpr int kFusePointsPerThread = 4;               // staged form: a workgroup walks at least this many points per thread

struct FuseArgs {
  const float *lat, *rgb, *cams, *lin;
  float *xyz, *color;
  uint8_t *support, *conflict, *flags;
  int V, S, up, P;
  float depth_scale, depth_shift, lo, hi, tau;
};

template <bool kLds>
__global__ __launch_bounds__(kFuseThreads) void fuse_kernel(FuseArgs a) {
  extern __shared__ float lds[];      // kLds: [V * S * S] depth01 of the scene's views | [V * MVD_CAM_RECORD] camera records
  const int V = a.V, S = a.S, SS = S * S, P = a.P, PP = P * P;
  const int scene = blockIdx.y;
  const float* lat = a.lat + (size_t)scene * V * 5 * SS;
  const float* cams = a.cams + (size_t)scene * V * MVD_CAM_RECORD;
  if (kLds) {
    for (int i = threadIdx.x; i < V * SS; i += kFuseThreads) lds[i] = depth01(lat[((size_t)(i / SS) * 5 + 4) * SS + i % SS]);
    for (int i = threadIdx.x; i < V * MVD_CAM_RECORD; i += kFuseThreads) lds[V * SS + i] = cams[i];
    __syncthreads();
    cams = lds + V * SS;
  }
  const unsigned total = (unsigned)V * PP;   // points of this scene (< 2^31: checked by the entry point, so i + stride fits 32 bits)
  for (unsigned i = blockIdx.x * kFuseThreads + threadIdx.x; i < total; i += gridDim.x * kFuseThreads) {
    const int b = (int)(i / (unsigned)PP), rem = (int)(i % (unsigned)PP), Y = rem / P, X = rem % P;
    const int own = (Y / a.up) * S + X / a.up;
    const float dn = kLds ? lds[b * SS + own] : depth01(lat[((size_t)b * 5 + 4) * SS + own]);
    const bool fg = a.lo < dn && dn < a.hi;
    const float z = dn * a.depth_scale + a.depth_shift;
    float Xw[3];
    unproject(load_cam(cams + (size_t)b * MVD_CAM_RECORD), a.lin[X], a.lin[Y], z, Xw);
    int support = 0, conflict = 0;
    for (int v = 0; v < V; ++v) {
      if (v == b) continue;
      float u, w, zc;
      project_z(load_cam(cams + (size_t)v * MVD_CAM_RECORD), Xw, u, w, zc);
      if (!(zc > 0.f && fabsf(u) <= 1.f && fabsf(w) <= 1.f)) continue;      // unseen (a NaN compares false)
      const PixelTaps t = pixel_taps(u, w, S);
      float zt[4];
      bool all_fg = true;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = kLds ? lds[v * SS + t.idx[k]] : depth01(lat[((size_t)v * 5 + 4) * SS + t.idx[k]]);
        all_fg = all_fg && a.lo < d && d < a.hi;
        zt[k] = d * a.depth_scale + a.depth_shift;
      }
      if (!all_fg) continue;      // view v looks at background or a silhouette there: no vote
      const float zs = bilinear_mix(zt, t);
      const float dz = zc - zs;
      support += fabsf(dz) <= a.tau;
      conflict += dz < -a.tau;
    }
    const size_t pt = (size_t)scene * total + i;
    a.xyz[pt * 3 + 0] = Xw[0];
    a.xyz[pt * 3 + 1] = Xw[1];
    a.xyz[pt * 3 + 2] = Xw[2];
    if (a.rgb) {
      const float* px = a.rgb + ((size_t)(scene * V + b) * 3) * PP + rem;
      a.color[pt * 3 + 0] = px[0];
      a.color[pt * 3 + 1] = px[(size_t)PP];
      a.color[pt * 3 + 2] = px[2 * (size_t)PP];
    }
    a.support[pt] = (uint8_t)support;
    a.conflict[pt] = (uint8_t)conflict;
    a.flags[pt] = fg ? MVD_FUSE_FOREGROUND : 0;
  }
}

// ------------------------------------------------------------------------------------------------ stable compaction
struct CompactArgs {
  const float *xyz, *color;
  const uint8_t *support, *conflict, *flags;
  size_t npts;
  int min_support, max_conflicts;
  float *out_xyz, *out_color;
  uint8_t* out_support;
  int* out_index;
  unsigned *count, *blocks;      // blocks: one word per workgroup of kCompactThreads points (count, then exclusive offset)
  unsigned nblocks;
};

__device__ __forceinline__ bool keep_point(const CompactArgs& a, size_t pt) {
  return pt < a.npts && (a.flags[pt] & MVD_FUSE_FOREGROUND) && (int)a.support[pt] >= a.min_support && (int)a.conflict[pt] <= a.max_conflicts;
}

__global__ __launch_bounds__(kCompactThreads) void count_kernel(CompactArgs a) {
  __shared__ unsigned wave_n[kCompactThreads / 64];
  const size_t pt = (size_t)blockIdx.x * kCompactThreads + threadIdx.x;
  const unsigned long long mask = __ballot(keep_point(a, pt));
  if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = (unsigned)__popcll(mask);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned n = 0;
#pragma unroll
    for (int w = 0; w < kCompactThreads / 64; ++w) n += wave_n[w];
    a.blocks[blockIdx.x] = n;
  }
}

__global__ __launch_bounds__(kCompactThreads) void scatter_kernel(CompactArgs a) {
  __shared__ unsigned wave_n[kCompactThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t pt = (size_t)blockIdx.x * kCompactThreads + threadIdx.x;
  const bool keep = keep_point(a, pt);
  const unsigned long long mask = __ballot(keep);
  if (lane == 0) wave_n[wave] = (unsigned)__popcll(mask);
  __syncthreads();
  if (!keep) return;
  size_t o = a.blocks[blockIdx.x];
#pragma unroll
  for (int w = 0; w < kCompactThreads / 64; ++w)
    if (w < wave) o += wave_n[w];
  o += (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
  for (int j = 0; j < 3; ++j) a.out_xyz[o * 3 + j] = a.xyz[pt * 3 + j];
  if (a.out_color) {
#pragma unroll
    for (int j = 0; j < 3; ++j) a.out_color[o * 3 + j] = a.color[pt * 3 + j];
  }
  a.out_support[o] = a.support[pt];
  a.out_index[o] = (int)pt;
}

// ------------------------------------------------------------------------------------------------ point splatting
constexpr int kSplatThreads = 256;
constexpr unsigned long long kEmptyKey = ~0ull;
// A plain load of the cell in front of each atomic skips it when the stored key is already smaller.  Keys only decrease, so a stale read
// costs an unnecessary atomic and never a wrong result.  Measured (tools/bench_render.py); -DMVD_SPLAT_EARLY_OUT=0
// builds the other form for the comparison.
#ifndef MVD_SPLAT_EARLY_OUT
#define MVD_SPLAT_EARLY_OUT 1
#endif

struct RenderArgs {
  const float *xyz, *color, *cams;
  const int* scene_start;
  unsigned long long* zbuf;
  int* index;
  float *depth, *rgb;
  int n, M, P, radius;
  float znear, empty_depth, bg[3];
};

// blockIdx.y = scene * M + camera: the camera record and the scene's point range are uniform; blockIdx.x walks the range, blocks past it exit
__global__ __launch_bounds__(kSplatThreads) void splat_kernel(RenderArgs a) {
  const int cam = blockIdx.y, scene = cam / a.M, P = a.P, r = a.radius;
  const long long s0 = max(a.scene_start[scene], 0), s1 = min(a.scene_start[scene + 1], a.n);      // (device values: never read past n)
  const long long i = s0 + (long long)blockIdx.x * kSplatThreads + threadIdx.x;
  if (i >= s1) return;
  const float X[3] = {a.xyz[i * 3 + 0], a.xyz[i * 3 + 1], a.xyz[i * 3 + 2]};
  float u, w, zc;
  project_z(load_cam(a.cams + (size_t)cam * MVD_CAM_RECORD), X, u, w, zc);
  if (!(zc > a.znear)) return;                                               // behind the near plane (a NaN compares false)
  const float P2 = 0.5f * (float)P;
  const float cx = (1.f - u) * P2 - 0.5f, cy = (1.f - w) * P2 - 0.5f;          // the fuse kernel's depth lookup, P for S, no clamp
  // a centre further than r + 1 pixels outside covers nothing; the test also drops NaN / inf and keeps the conversion below in range
  const float lo = -(float)(r + 2), hi = (float)(P + r + 1);
  if (!(cx >= lo && cx <= hi && cy >= lo && cy <= hi)) return;
  const int px = (int)floorf(cx + 0.5f), py = (int)floorf(cy + 0.5f);
  const int x0 = max(px - r, 0), x1 = min(px + r, P - 1), y0 = max(py - r, 0), y1 = min(py + r, P - 1);
  const unsigned long long key = ((unsigned long long)__float_as_uint(zc) << 32) | (unsigned long long)(unsigned)i;      // zc > 0: bits order like values
  unsigned long long* z = a.zbuf + (size_t)cam * P * P;
  for (int y = y0; y <= y1; ++y)
    for (int x = x0; x <= x1; ++x) {
      unsigned long long* cell = z + (size_t)y * P + x;
      if (MVD_SPLAT_EARLY_OUT && *cell <= key) continue;
      atomicMin(cell, key);
    }
}

__global__ __launch_bounds__(kSplatThreads) void resolve_kernel(RenderArgs a, unsigned total) {
  const unsigned pix = blockIdx.x * kSplatThreads + threadIdx.x;      // (camera, y, x); total < 2^31
  if (pix >= total) return;
  const unsigned long long key = a.zbuf[pix];
  const unsigned i = (unsigned)(key & 0xffffffffull);
  const bool hit = key != kEmptyKey && i < (unsigned)a.n;      // (i < n always behind the splat kernel; a z-buffer of the caller's is not trusted)
  a.index[pix] = hit ? (int)i : -1;
  a.depth[pix] = hit ? __uint_as_float((unsigned)(key >> 32)) : a.empty_depth;
  if (a.color) {
    const unsigned PP = (unsigned)a.P * a.P, cam = pix / PP, rem = pix % PP;
#pragma unroll
    for (int c = 0; c < 3; ++c) a.rgb[((size_t)cam * 3 + c) * PP + rem] = hit ? a.color[(size_t)i * 3 + c] : a.bg[c];
  }
}

}  // namespace

// the staged form's workgroups per scene: what is resident at once, but at least kFusePointsPerThread points per thread -- staging is
// V * S * S / kFuseThreads loads per thread, a point 4 * (V - 1) gathers
static int fuse_lds_workgroups(size_t scene_pts, size_t lds_bytes, int nscene) {
  const size_t resident = lds_bytes <= 80 * 1024 ? 512 : 256;      // two workgroups per CU while two images fit its 160 KiB, else one
  size_t wgs = resident / nscene;
  const size_t by_work = scene_pts / ((size_t)kFuseThreads * kFusePointsPerThread);
  if (by_work < wgs) wgs = by_work;
  return wgs > 0 ? (int)wgs : 1;
}

extern "C" int mvd_fuse_points(const float* lat, const float* rgb, const float* cams, const float* ndc_lin, float* xyz, float* color,
                               uint8_t* support, uint8_t* conflict, uint8_t* flags, int nscene, int V, int S, int up, float depth_scale,
                               float depth_shift, float lo, float hi, float tau, int stage, mvd_stream_t stream) {
  MVD_CHECK_ARG(lat && cams && ndc_lin && xyz && support && conflict && flags, "mvd_fuse_points: null pointer");
  MVD_CHECK_ARG(!rgb || color, "mvd_fuse_points: rgb without a color output");
  MVD_CHECK_ARG(nscene >= 1 && nscene <= 65535, "mvd_fuse_points: nscene=%d outside [1, 65535]", nscene);
  MVD_CHECK_ARG(V >= 1 && V <= 255, "mvd_fuse_points: V=%d outside [1, 255] (the counts are bytes)", V);
  MVD_CHECK_ARG(S >= 2 && S <= 32768, "mvd_fuse_points: S=%d outside [2, 32768]", S);
  MVD_CHECK_ARG(up >= 1 && up <= 32768, "mvd_fuse_points: up=%d outside [1, 32768]", up);
  MVD_CHECK_ARG(lo < hi, "mvd_fuse_points: foreground range lo=%g >= hi=%g", (double)lo, (double)hi);
  MVD_CHECK_ARG(tau >= 0.f, "mvd_fuse_points: tau=%g (>= 0)", (double)tau);
  MVD_CHECK_ARG(stage >= MVD_FUSE_STAGE_AUTO && stage <= MVD_FUSE_STAGE_LDS, "mvd_fuse_points: stage=%d", stage);
  const unsigned long long P = (unsigned long long)S * up;
  MVD_CHECK_ARG(P <= 46340 && (unsigned long long)nscene * V * P * P <= 0x7fffffffull,
                "mvd_fuse_points: nscene * V * (S * up)^2 points beyond 2^31 - 1 (nscene=%d, V=%d, S=%d, up=%d)", nscene, V, S, up);
  const size_t scene_pts = (size_t)V * P * P;
  const size_t lds_bytes = ((size_t)V * S * S + (size_t)V * MVD_CAM_RECORD) * sizeof(float);
  int wgs = 0;      // auto is the global form: measured, the staged one wins by 1 % at one shape and loses elsewhere
  if (stage == MVD_FUSE_STAGE_LDS) {
    MVD_CHECK_ARG(lds_bytes <= kFuseLdsMax, "mvd_fuse_points: MVD_FUSE_STAGE_LDS needs %zu bytes of LDS (limit %zu)", lds_bytes, kFuseLdsMax);
    wgs = fuse_lds_workgroups(scene_pts, lds_bytes, nscene);
  }
  FuseArgs a{lat, rgb, cams, ndc_lin, xyz, color, support, conflict, flags, V, S, up, (int)P, depth_scale, depth_shift, lo, hi, tau};
  if (wgs > 0) {
    if (lds_bytes > 64 * 1024) {
      static unsigned long long raised = 0;
      const hipError_t e = mvd_raise_dynamic_lds((const void*)fuse_kernel<true>, (int)kFuseLdsMax, &raised);
      MVD_CHECK_ARG(e == hipSuccess, "mvd_fuse_points: hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(fuse_kernel<true>, dim3(wgs, nscene), dim3(kFuseThreads), lds_bytes, (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(fuse_kernel<false>, dim3(cdiv((long)scene_pts, kFuseThreads), nscene), dim3(kFuseThreads), 0, (hipStream_t)stream, a);
  }
  MVD_CHECK_LAUNCH("mvd_fuse_points");
  return 0;
}

extern "C" size_t mvd_compact_points_scratch(size_t npts) { return (npts / kCompactThreads + 1) * sizeof(unsigned); }

extern "C" int mvd_compact_points(const float* xyz, const float* color, const uint8_t* support, const uint8_t* conflict, const uint8_t* flags,
                                  size_t npts, int min_support, int max_conflicts, float* out_xyz, float* out_color, uint8_t* out_support,
                                  int* out_index, unsigned* count, void* scratch, size_t scratch_bytes, mvd_stream_t stream) {
  MVD_CHECK_ARG(xyz && support && conflict && flags && out_xyz && out_support && out_index && count && scratch,
                "mvd_compact_points: null pointer");
  MVD_CHECK_ARG(!out_color == !color, "mvd_compact_points: color and out_color go together");
  MVD_CHECK_ARG(npts >= 1 && npts <= 0x7fffffffull, "mvd_compact_points: npts=%zu outside [1, 2^31 - 1]", npts);
  MVD_CHECK_ARG(min_support >= 0 && max_conflicts >= 0, "mvd_compact_points: min_support=%d, max_conflicts=%d (>= 0)", min_support,
                max_conflicts);
  MVD_CHECK_ARG(scratch_bytes >= mvd_compact_points_scratch(npts) && ((uintptr_t)scratch & 3) == 0,
                "mvd_compact_points: scratch of %zu bytes (needs %zu, 4-byte aligned)", scratch_bytes, mvd_compact_points_scratch(npts));
  const unsigned nblocks = (unsigned)((npts + kCompactThreads - 1) / kCompactThreads);
  CompactArgs a{xyz, color, support, conflict, flags, npts, min_support, max_conflicts, out_xyz, out_color, out_support, out_index, count,
                (unsigned*)scratch, nblocks};
  hipLaunchKernelGGL(count_kernel, dim3(nblocks), dim3(kCompactThreads), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kCompactThreads), 0, (hipStream_t)stream, a.blocks, nblocks, count);
  hipLaunchKernelGGL(scatter_kernel, dim3(nblocks), dim3(kCompactThreads), 0, (hipStream_t)stream, a);
  MVD_CHECK_LAUNCH("mvd_compact_points");
  return 0;
}

extern "C" size_t mvd_render_points_scratch(int ncam, int P) {
  return ncam >= 1 && P >= 1 ? (size_t)ncam * P * P * sizeof(unsigned long long) : 0;
}

extern "C" int mvd_render_points_stages(const float* xyz, const float* color, const int* scene_start, const float* cams, size_t n, int nscene,
                                        int M, int P, int radius, float znear, float empty_depth, const float* background, int* index,
                                        float* depth, float* rgb, void* scratch, size_t scratch_bytes, int stages, mvd_stream_t stream) {
  const char* fn = stages == MVD_RENDER_ALL ? "mvd_render_points" : "mvd_render_points_stages";
  MVD_CHECK_ARG(stages >= 1 && stages <= MVD_RENDER_ALL, "%s: stages=%d outside [1, %d]", fn, stages, MVD_RENDER_ALL);
  MVD_CHECK_ARG(n <= 0x7fffffffull, "%s: n=%zu beyond 2^31 - 1", fn, n);
  MVD_CHECK_ARG(xyz || n == 0, "%s: null xyz with n=%zu", fn, n);
  MVD_CHECK_ARG(scene_start && cams && index && depth && scratch, "%s: null pointer", fn);
  MVD_CHECK_ARG(!color || (rgb && background), "%s: color without an rgb output and a background", fn);
  MVD_CHECK_ARG(nscene >= 1 && M >= 1 && (unsigned long long)nscene * M <= 65535ull, "%s: nscene=%d, M=%d (>= 1, nscene * M <= 65535)", fn,
                nscene, M);
  MVD_CHECK_ARG(P >= 1 && P <= 46340 && (unsigned long long)nscene * M * P * P <= 0x7fffffffull,
                "%s: nscene * M * P^2 pixels outside [1, 2^31 - 1] (nscene=%d, M=%d, P=%d)", fn, nscene, M, P);
  MVD_CHECK_ARG(radius >= 0 && radius <= MVD_SPLAT_MAX_RADIUS, "%s: radius=%d outside [0, %d]", fn, radius, MVD_SPLAT_MAX_RADIUS);
  MVD_CHECK_ARG(znear >= 0.f, "%s: znear=%g (>= 0)", fn, (double)znear);
  const int ncam = nscene * M;
  MVD_CHECK_ARG(scratch_bytes >= mvd_render_points_scratch(ncam, P) && ((uintptr_t)scratch & 7) == 0,
                "%s: scratch of %zu bytes (needs %zu, 8-byte aligned)", fn, scratch_bytes, mvd_render_points_scratch(ncam, P));
  RenderArgs a{xyz, color, cams, scene_start, (unsigned long long*)scratch, index, depth, rgb, (int)n, M, P, radius, znear, empty_depth,
               {0.f, 0.f, 0.f}};
  if (color)
    for (int c = 0; c < 3; ++c) a.bg[c] = background[c];
  const unsigned total = (unsigned)ncam * P * P;
  if (stages & MVD_RENDER_FILL) {
    const hipError_t e = hipMemsetAsync(scratch, 0xff, (size_t)total * sizeof(unsigned long long), (hipStream_t)stream);
    MVD_CHECK_ARG(e == hipSuccess, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
  }
  if ((stages & MVD_RENDER_SPLAT) && n > 0)      // a scene has at most n points: blocks past its range exit
    hipLaunchKernelGGL(splat_kernel, dim3(cdiv((long)n, kSplatThreads), ncam), dim3(kSplatThreads), 0, (hipStream_t)stream, a);
  if (stages & MVD_RENDER_RESOLVE)
    hipLaunchKernelGGL(resolve_kernel, dim3(cdiv((long)total, kSplatThreads)), dim3(kSplatThreads), 0, (hipStream_t)stream, a, total);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int mvd_render_points(const float* xyz, const float* color, const int* scene_start, const float* cams, size_t n, int nscene, int M,
                                 int P, int radius, float znear, float empty_depth, const float* background, int* index, float* depth,
                                 float* rgb, void* scratch, size_t scratch_bytes, mvd_stream_t stream) {
  return mvd_render_points_stages(xyz, color, scene_start, cams, n, nscene, M, P, radius, znear, empty_depth, background, index, depth, rgb,
                                  scratch, scratch_bytes, MVD_RENDER_ALL, stream);
}
