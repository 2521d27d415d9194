// Scoring views against ground truth: squared error, SSIM and the depth-error family (include/mvd_hip.h: mvd_image_metrics and
// mvd_depth_metrics have the rules in full).  Everything is accumulated in fp64 and reduced in a fixed order; no floating-point atomics.
//
// SSIM (vm_ssim_kernel): one workgroup of kVmThreads = 256 per tile of kVmTileW x kVmTileH = 32 x 16 window positions of one (image,
// channel) plane.  The fp32 input tile of both images with its halo -- at most (16 + 32) x (32 + 32) pixels each at window = 33 -- is
// staged in LDS once (2 x 12 KiB).  The five moments x, y, xx, xy, yy are then taken ONE AFTER THE OTHER through a single fp64 plane of
// (16 + 32) x 32 row-filtered values (12 KiB): horizontal pass into the plane, barrier, vertical pass out of it into registers (each
// thread owns two window positions, ten doubles), barrier.  Fifteen fp64 planes of a tile would be 180 KiB; this form is 36.3 KiB of
// static LDS whatever the window, so FOUR workgroups (16 wavefronts, 4 per SIMD) share the 160 KiB of a CU and cover each other's ten
// barriers.  Lanes of a wavefront walk a row of the tile in both passes: consecutive 4-byte and 8-byte LDS words, no bank conflict.
// The window table comes by value in the kernel arguments and is copied to LDS by constant index; no transcendental runs on the device.
// The plane is reused for the workgroup's fixed-order tree sum, whose result goes to the scratch as the tile's partial.
// SQUARED ERROR (vm_sq_kernel) and the DEPTH passes (vm_depth_fit_kernel, vm_depth_err_kernel): one workgroup per chunk of kVmChunk =
// 2048 pixels of one image, thread t takes pixels t, t + 256, ..., the same tree sum, one partial per chunk.
// SECOND STAGE (vm_image_final_kernel, vm_depth_solve_kernel, vm_depth_final_kernel): one workgroup per image sums its partials -- thread
// t takes partials t, t + 256, ... ascending, then the tree.  The order of every sum is a function of (C, H, W, window) alone.
//
// Not tried (the view-metrics section): a vertical slide with the row results in registers; two moment planes in flight to
// halve the barriers; fusing the squared error into the SSIM tiles; packing the 8-bit mask reads.
#include "../../include/mvd_hip.h"
#include "common.hpp"

#include <cstdint>
#include <type_traits>

namespace {

constexpr int kVmThreads = 256;
constexpr int kVmTileW = MVD_SSIM_TILE_W, kVmTileH = MVD_SSIM_TILE_H;
constexpr int kVmMaxWindow = MVD_SSIM_MAX_WINDOW;
constexpr int kVmInW = kVmTileW + kVmMaxWindow - 1, kVmInH = kVmTileH + kVmMaxWindow - 1;      // 64 x 48: the staged tile at window = 33
constexpr int kVmPerThread = kVmTileW * kVmTileH / kVmThreads;                                // 2 window positions per thread
constexpr int kVmChunk = MVD_METRIC_CHUNK;
constexpr int kVmMaxSide = 32768;
constexpr int kVmErrSums = 4, kVmErrCounts = 5, kVmFitSums = 4;

static_assert(kVmTileW == 32 && kVmTileW * kVmTileH % kVmThreads == 0 && kVmChunk % kVmThreads == 0, "the thread maps below assume this");

// ---- the plan: tiles, chunks and where each array of partials sits in the scratch (all of it 8-byte words) ---------------------------
struct VmImagePlan {
  long long Ho, Wo, tiles_x, tiles_y, ntile, nchunk;
  size_t sq_part, cnt_part, ssim_part, scnt_part, words;      // offsets in 8-byte words: (B, nchunk), (B, nchunk), (B*C, ntile), (B, ntile)
};

__host__ __device__ inline long long vm_cdiv(long long a, long long b) { return (a + b - 1) / b; }

// window = 0: no SSIM (no tiles).  false: a limit of mvd_image_metrics is broken.
__host__ inline bool vm_image_plan(long long B, long long C, long long H, long long W, int window, VmImagePlan& p) {
  if (B < 0 || C < 1 || H < 1 || W < 1 || H > kVmMaxSide || W > kVmMaxSide || B * C > 65535) return false;
  if (window && (window < 3 || window > kVmMaxWindow || !(window & 1) || H < window || W < window)) return false;
  p.Ho = window ? H - window + 1 : 0, p.Wo = window ? W - window + 1 : 0;
  p.tiles_x = vm_cdiv(p.Wo, kVmTileW), p.tiles_y = vm_cdiv(p.Ho, kVmTileH), p.ntile = p.tiles_x * p.tiles_y;
  p.nchunk = vm_cdiv(H * W, kVmChunk);
  p.sq_part = 0, p.cnt_part = p.sq_part + (size_t)(B * p.nchunk), p.ssim_part = p.cnt_part + (size_t)(B * p.nchunk);
  p.scnt_part = p.ssim_part + (size_t)(B * C * p.ntile), p.words = p.scnt_part + (size_t)(B * p.ntile);
  return true;
}

struct VmDepthPlan {
  long long nchunk;
  size_t fit, fit_part, n_part, err_part, cnt_part, words;      // (B, 2), (B, nchunk, 4), (B, nchunk), (B, nchunk, 4), (B, nchunk, 5)
};

__host__ inline bool vm_depth_plan(long long B, long long H, long long W, VmDepthPlan& p) {
  if (B < 0 || B > 65535 || H < 1 || W < 1 || H > kVmMaxSide || W > kVmMaxSide) return false;
  p.nchunk = vm_cdiv(H * W, kVmChunk);
  const size_t per = (size_t)(B * p.nchunk);
  p.fit = 0, p.fit_part = p.fit + (size_t)B * 2, p.n_part = p.fit_part + per * kVmFitSums, p.err_part = p.n_part + per;
  p.cnt_part = p.err_part + per * kVmErrSums, p.words = p.cnt_part + per * kVmErrCounts;
  return true;
}

// ---- index arithmetic shared by the kernels and tools/view_metrics_host.hip ---------------------------------------------------------
// Tile `tile` of a plane with Ho x Wo window positions: its first position (r0, c0) and its extent th x tw (the last tiles are cut).
__host__ __device__ inline void vm_tile(long long tile, long long tiles_x, long long Ho, long long Wo, int& r0, int& c0, int& th, int& tw) {
  r0 = (int)(tile / tiles_x) * kVmTileH, c0 = (int)(tile % tiles_x) * kVmTileW;
  th = (int)(Ho - r0 < kVmTileH ? Ho - r0 : kVmTileH), tw = (int)(Wo - c0 < kVmTileW ? Wo - c0 : kVmTileW);
}
// Element i of the staged tile of inw = tw + window - 1 columns: its LDS word and its pixel of the H x W plane.
__host__ __device__ inline void vm_stage(int i, int inw, int r0, int c0, long long W, int& lds, size_t& pixel) {
  const int r = i / inw, c = i - r * inw;
  lds = r * kVmInW + c, pixel = (size_t)(r0 + r) * (size_t)W + (size_t)(c0 + c);
}

// moment m of a pixel pair in fp64: x, y, xx, xy, yy (the products of two fp32 values are exact)
template <int m>
__host__ __device__ __forceinline__ double vm_moment(float xf, float yf) {
  const double x = (double)xf, y = (double)yf;
  return m == 0 ? x : m == 1 ? y : m == 2 ? x * x : m == 3 ? x * y : y * y;
}

// THE formula, in the header's order, from the five filtered moments
__host__ __device__ __forceinline__ double vm_ssim(const double* e, double c1, double c2) {
  const double mx = e[0], my = e[1];
  const double sxx = e[2] - mx * mx, sxy = e[3] - mx * my, syy = e[4] - my * my;
  return ((2.0 * mx * my + c1) * (2.0 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2));
}

// A pixel of the depth metrics counts when both values are finite and > 0 (a NaN compares false).
__host__ __device__ __forceinline__ bool vm_depth_ok(float p, float t) { return p > 0.f && p < INFINITY && t > 0.f && t < INFINITY; }

// The per-image fit from the pass-1 sums {Sp, St, Spp, Spt} and n.
__host__ __device__ inline void vm_solve(int align, long long n, const double* S, double& s, double& b) {
  s = 1.0, b = 0.0;
  if (align == MVD_DEPTH_ALIGN_SCALE) s = S[3] / S[2];
  if (align == MVD_DEPTH_ALIGN_SCALE_SHIFT) {
    const double dn = (double)n, det = dn * S[2] - S[0] * S[0];
    if (det > 0.0) s = (dn * S[3] - S[0] * S[1]) / det, b = (S[2] * S[1] - S[0] * S[3]) / det;
    else s = b = NAN;
  }
}

// ---- the workgroup sums: a tree in LDS, the same pairs in the same order every time ---------------------------------------------------
template <typename T>
__device__ __forceinline__ T vm_block_sum(T v, T* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = kVmThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
    __syncthreads();
  }
  const T out = red[0];
  __syncthreads();
  return out;
}

struct SsimArgs {
  const float *a, *b;
  const unsigned char* mask;
  double *ssim_map, *ssim_part;
  long long* scnt_part;
  long long H, W, Ho, Wo, tiles_x, ntile;
  int C, window;
  double c1, c2;
  double w[kVmMaxWindow];
};

// blockIdx.x = tile, blockIdx.y = plane b * C + c.
__global__ __launch_bounds__(kVmThreads) void vm_ssim_kernel(SsimArgs a) {
  __shared__ float xs[kVmInH * kVmInW], ys[kVmInH * kVmInW];
  __shared__ double plane[kVmInH * kVmTileW];
  __shared__ double wsh[kVmMaxWindow];
  const int tid = threadIdx.x, window = a.window, half = window / 2;
  const size_t pl = blockIdx.y, img = pl / a.C, HW = (size_t)a.H * (size_t)a.W;
  int r0, c0, th, tw;
  vm_tile(blockIdx.x, a.tiles_x, a.Ho, a.Wo, r0, c0, th, tw);
  const int inh = th + window - 1, inw = tw + window - 1;
  const float *pa = a.a + pl * HW, *pb = a.b + pl * HW;
  for (int i = tid; i < inh * inw; i += kVmThreads) {
    int lds;
    size_t pixel;
    vm_stage(i, inw, r0, c0, a.W, lds, pixel);
    xs[lds] = pa[pixel], ys[lds] = pb[pixel];
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < kVmMaxWindow; ++k) wsh[k] = a.w[k];      // (constant indices: the by-value table stays in scalar registers)
  }
  __syncthreads();
  double e[kVmPerThread][5];
  auto pass = [&](auto mc) {
    constexpr int m = decltype(mc)::value;
    for (int i = tid; i < inh * kVmTileW; i += kVmThreads) {      // horizontal: row r of the staged tile, column c of the tile
      const int r = i >> 5, c = i & 31;
      if (c >= tw) continue;
      const float *xr = xs + r * kVmInW + c, *yr = ys + r * kVmInW + c;
      double s = 0.0;
      for (int k = 0; k < window; ++k) s = s + wsh[k] * vm_moment<m>(xr[k], yr[k]);
      plane[i] = s;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kVmPerThread; ++j) {                      // vertical: window position (ro, co) of the tile
      const int i = tid + j * kVmThreads, ro = i >> 5, co = i & 31;
      double s = 0.0;
      if (ro < th && co < tw)
        for (int k = 0; k < window; ++k) s = s + wsh[k] * plane[(ro + k) * kVmTileW + co];
      e[j][m] = s;
    }
    __syncthreads();
  };
  pass(std::integral_constant<int, 0>{}), pass(std::integral_constant<int, 1>{}), pass(std::integral_constant<int, 2>{});
  pass(std::integral_constant<int, 3>{}), pass(std::integral_constant<int, 4>{});
  double sum = 0.0;
  long long n = 0;
#pragma unroll
  for (int j = 0; j < kVmPerThread; ++j) {
    const int i = tid + j * kVmThreads, ro = i >> 5, co = i & 31;
    if (ro >= th || co >= tw) continue;
    const double v = vm_ssim(e[j], a.c1, a.c2);
    if (a.ssim_map) a.ssim_map[(pl * (size_t)a.Ho + (size_t)(r0 + ro)) * (size_t)a.Wo + (size_t)(c0 + co)] = v;
    if (!a.mask || a.mask[img * HW + (size_t)(r0 + ro + half) * (size_t)a.W + (size_t)(c0 + co + half)]) sum = sum + v, ++n;
  }
  sum = vm_block_sum(sum, plane);
  n = vm_block_sum(n, reinterpret_cast<long long*>(plane));
  if (tid == 0) {
    a.ssim_part[pl * (size_t)a.ntile + blockIdx.x] = sum;
    if (pl % a.C == 0) a.scnt_part[img * (size_t)a.ntile + blockIdx.x] = n;
  }
}

// blockIdx.x = chunk, blockIdx.y = image.
__global__ __launch_bounds__(kVmThreads) void vm_sq_kernel(const float* __restrict__ a, const float* __restrict__ b, const unsigned char* __restrict__ mask,
                                                           int C, size_t HW, double* __restrict__ sq_part, long long* __restrict__ cnt_part) {
  __shared__ double red[kVmThreads];
  const size_t img = blockIdx.y;
  double sum = 0.0;
  long long n = 0;
  for (int j = 0; j < kVmChunk / kVmThreads; ++j) {
    const size_t p = (size_t)blockIdx.x * kVmChunk + (size_t)j * kVmThreads + threadIdx.x;
    if (p >= HW || (mask && !mask[img * HW + p])) continue;
    ++n;
    for (int c = 0; c < C; ++c) {
      const size_t at = (img * C + c) * HW + p;
      const double d = (double)a[at] - (double)b[at];
      sum = sum + d * d;
    }
  }
  sum = vm_block_sum(sum, red);
  n = vm_block_sum(n, reinterpret_cast<long long*>(red));
  if (threadIdx.x == 0) sq_part[img * gridDim.x + blockIdx.x] = sum, cnt_part[img * gridDim.x + blockIdx.x] = n;
}

// the sum of part[0 .. n) by one workgroup: thread t takes t, t + 256, ... ascending, then the tree
template <typename T>
__device__ __forceinline__ T vm_sum_parts(const T* part, size_t n, size_t stride, T* red) {
  T s = 0;
  for (size_t i = threadIdx.x; i < n; i += kVmThreads) s = s + part[i * stride];
  return vm_block_sum(s, red);
}

// blockIdx.x = image.
__global__ __launch_bounds__(kVmThreads) void vm_image_final_kernel(const double* sq_part, const long long* cnt_part, const double* ssim_part,
                                                                    const long long* scnt_part, size_t nchunk, size_t ntile, int C, double* sq_sum,
                                                                    long long* count, double* ssim_sum, long long* ssim_count) {
  __shared__ double red[kVmThreads];
  long long* redn = reinterpret_cast<long long*>(red);
  const size_t img = blockIdx.x;
  const double sq = vm_sum_parts(sq_part + img * nchunk, nchunk, 1, red);
  const long long n = vm_sum_parts(cnt_part + img * nchunk, nchunk, 1, redn);
  if (threadIdx.x == 0) {
    if (sq_sum) sq_sum[img] = sq;
    if (count) count[img] = n;
  }
  if (!ntile) return;
  const double ss = vm_sum_parts(ssim_part + img * C * ntile, (size_t)C * ntile, 1, red);
  const long long sn = vm_sum_parts(scnt_part + img * ntile, ntile, 1, redn);
  if (threadIdx.x == 0) {
    if (ssim_sum) ssim_sum[img] = ss;
    if (ssim_count) ssim_count[img] = sn;
  }
}

// pass 1 of the depth metrics: blockIdx.x = chunk, blockIdx.y = image -> {Sp, St, Spp, Spt} and n of the chunk
__global__ __launch_bounds__(kVmThreads) void vm_depth_fit_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                  const unsigned char* __restrict__ valid, size_t HW, double* __restrict__ fit_part,
                                                                  long long* __restrict__ n_part) {
  __shared__ double red[kVmThreads];
  const size_t img = blockIdx.y;
  double S[kVmFitSums] = {0.0, 0.0, 0.0, 0.0};
  long long n = 0;
  for (int j = 0; j < kVmChunk / kVmThreads; ++j) {
    const size_t i = (size_t)blockIdx.x * kVmChunk + (size_t)j * kVmThreads + threadIdx.x;
    if (i >= HW || (valid && !valid[img * HW + i])) continue;
    const float pf = pred[img * HW + i], tf = target[img * HW + i];
    if (!vm_depth_ok(pf, tf)) continue;
    const double p = (double)pf, t = (double)tf;
    ++n, S[0] = S[0] + p, S[1] = S[1] + t, S[2] = S[2] + p * p, S[3] = S[3] + p * t;
  }
  const size_t at = img * gridDim.x + blockIdx.x;
#pragma unroll
  for (int k = 0; k < kVmFitSums; ++k) {
    const double v = vm_block_sum(S[k], red);
    if (threadIdx.x == 0) fit_part[at * kVmFitSums + k] = v;
  }
  n = vm_block_sum(n, reinterpret_cast<long long*>(red));
  if (threadIdx.x == 0) n_part[at] = n;
}

// blockIdx.x = image: the second stage of pass 1 and the solve
__global__ __launch_bounds__(kVmThreads) void vm_depth_solve_kernel(const double* fit_part, const long long* n_part, size_t nchunk, int align,
                                                                    double* fit) {
  __shared__ double red[kVmThreads];
  const size_t img = blockIdx.x;
  double S[kVmFitSums];
#pragma unroll
  for (int k = 0; k < kVmFitSums; ++k) S[k] = vm_sum_parts(fit_part + img * nchunk * kVmFitSums + k, nchunk, kVmFitSums, red);
  const long long n = vm_sum_parts(n_part + img * nchunk, nchunk, 1, reinterpret_cast<long long*>(red));
  if (threadIdx.x == 0) vm_solve(align, n, S, fit[img * 2], fit[img * 2 + 1]);
}

// pass 2: blockIdx.x = chunk, blockIdx.y = image
__global__ __launch_bounds__(kVmThreads) void vm_depth_err_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                  const unsigned char* __restrict__ valid, size_t HW, const double* __restrict__ fit,
                                                                  double* __restrict__ err_part, long long* __restrict__ cnt_part) {
  __shared__ double red[kVmThreads];
  const size_t img = blockIdx.y;
  const double s = fit[img * 2], b = fit[img * 2 + 1];
  double S[kVmErrSums] = {0.0, 0.0, 0.0, 0.0};
  long long N[kVmErrCounts] = {0, 0, 0, 0, 0};      // delta < 1.25, < 1.25^2, < 1.25^3; counted; dropped
  for (int j = 0; j < kVmChunk / kVmThreads; ++j) {
    const size_t i = (size_t)blockIdx.x * kVmChunk + (size_t)j * kVmThreads + threadIdx.x;
    if (i >= HW || (valid && !valid[img * HW + i])) continue;
    const float pf = pred[img * HW + i], tf = target[img * HW + i];
    if (!vm_depth_ok(pf, tf)) continue;
    const double t = (double)tf, q = s * (double)pf + b;
    if (!(q > 0.0)) {
      ++N[4];
      continue;
    }
    const double d = q - t, dd = d * d, l = log(q) - log(t), r = fmax(q / t, t / q);
    S[0] = S[0] + fabs(d) / t, S[1] = S[1] + dd / t, S[2] = S[2] + dd, S[3] = S[3] + l * l;
    N[0] += r < 1.25, N[1] += r < 1.5625, N[2] += r < 1.953125, ++N[3];
  }
  const size_t at = img * gridDim.x + blockIdx.x;
#pragma unroll
  for (int k = 0; k < kVmErrSums; ++k) {
    const double v = vm_block_sum(S[k], red);
    if (threadIdx.x == 0) err_part[at * kVmErrSums + k] = v;
  }
#pragma unroll
  for (int k = 0; k < kVmErrCounts; ++k) {
    const long long v = vm_block_sum(N[k], reinterpret_cast<long long*>(red));
    if (threadIdx.x == 0) cnt_part[at * kVmErrCounts + k] = v;
  }
}

// blockIdx.x = image
__global__ __launch_bounds__(kVmThreads) void vm_depth_final_kernel(const double* err_part, const long long* cnt_part, const double* fit_in,
                                                                    size_t nchunk, double* fit, double* sums, long long* counts) {
  __shared__ double red[kVmThreads];
  const size_t img = blockIdx.x;
#pragma unroll
  for (int k = 0; k < kVmErrSums; ++k) {
    const double v = vm_sum_parts(err_part + img * nchunk * kVmErrSums + k, nchunk, kVmErrSums, red);
    if (threadIdx.x == 0 && sums) sums[img * kVmErrSums + k] = v;
  }
#pragma unroll
  for (int k = 0; k < kVmErrCounts; ++k) {
    const long long v = vm_sum_parts(cnt_part + img * nchunk * kVmErrCounts + k, nchunk, kVmErrCounts, reinterpret_cast<long long*>(red));
    if (threadIdx.x == 0 && counts) counts[img * kVmErrCounts + k] = v;
  }
  if (threadIdx.x == 0 && fit) fit[img * 2] = fit_in[img * 2], fit[img * 2 + 1] = fit_in[img * 2 + 1];
}

}  // namespace

extern "C" size_t mvd_image_metrics_scratch(int B, int C, int H, int W, int window) {
  VmImagePlan p;
  return vm_image_plan(B, C, H, W, window, p) ? p.words * 8 : 0;
}

extern "C" size_t mvd_depth_metrics_scratch(int B, int H, int W) {
  VmDepthPlan p;
  return vm_depth_plan(B, H, W, p) ? p.words * 8 : 0;
}

extern "C" int mvd_image_metrics(const float* a, const float* b, const unsigned char* mask, int B, int C, int H, int W, const double* weights,
                                 int window, double c1, double c2, double* sq_sum, long long* count, double* ssim_sum, long long* ssim_count,
                                 double* ssim_map, void* scratch, size_t scratch_bytes, mvd_stream_t stream) {
  const char* fn = "mvd_image_metrics";
  MVD_CHECK_ARG(B >= 0 && C >= 1 && (long long)B * C <= 65535, "%s: B=%d, C=%d (B >= 0, C >= 1, B * C <= 65535)", fn, B, C);
  MVD_CHECK_ARG(H >= 1 && H <= kVmMaxSide && W >= 1 && W <= kVmMaxSide, "%s: H=%d, W=%d outside [1, %d]", fn, H, W, kVmMaxSide);
  if (!weights) window = 0;
  if (weights) {
    MVD_CHECK_ARG(window >= 3 && window <= kVmMaxWindow && (window & 1), "%s: window=%d (odd, in [3, %d])", fn, window, kVmMaxWindow);
    MVD_CHECK_ARG(H >= window && W >= window, "%s: H=%d, W=%d smaller than window=%d", fn, H, W, window);
    for (int k = 0; k < window; ++k) MVD_CHECK_ARG(fabs(weights[k]) < INFINITY, "%s: weights[%d]=%g is not finite", fn, k, weights[k]);
    MVD_CHECK_ARG(fabs(c1) < INFINITY && fabs(c2) < INFINITY, "%s: c1=%g, c2=%g (finite)", fn, c1, c2);
  }
  VmImagePlan p;
  MVD_CHECK_ARG(vm_image_plan(B, C, H, W, window, p), "%s: no plan for B=%d, C=%d, H=%d, W=%d, window=%d", fn, B, C, H, W, window);
  if (B == 0) return 0;
  MVD_CHECK_ARG(a && b, "%s: null image", fn);
  MVD_CHECK_ARG(scratch && scratch_bytes >= p.words * 8 && ((uintptr_t)scratch & 7) == 0,
                "%s: scratch of %zu bytes at %p (mvd_image_metrics_scratch: %zu bytes, 8-byte aligned)", fn, scratch_bytes, scratch, p.words * 8);
  double* sd = (double*)scratch;
  long long* sl = (long long*)scratch;
  const hipStream_t st = (hipStream_t)stream;
  const size_t HW = (size_t)H * (size_t)W;
  hipLaunchKernelGGL(vm_sq_kernel, dim3((unsigned)p.nchunk, B), dim3(kVmThreads), 0, st, a, b, mask, C, HW, sd + p.sq_part, sl + p.cnt_part);
  MVD_CHECK_LAUNCH(fn);
  if (window) {
    SsimArgs s{a, b, mask, ssim_map, sd + p.ssim_part, sl + p.scnt_part, H, W, p.Ho, p.Wo, p.tiles_x, p.ntile, C, window, c1, c2, {}};
    for (int k = 0; k < kVmMaxWindow; ++k) s.w[k] = k < window ? weights[k] : 0.0;
    hipLaunchKernelGGL(vm_ssim_kernel, dim3((unsigned)p.ntile, B * C), dim3(kVmThreads), 0, st, s);
    MVD_CHECK_LAUNCH(fn);
  }
  hipLaunchKernelGGL(vm_image_final_kernel, dim3(B), dim3(kVmThreads), 0, st, sd + p.sq_part, sl + p.cnt_part, sd + p.ssim_part, sl + p.scnt_part,
                     (size_t)p.nchunk, (size_t)p.ntile, C, sq_sum, count, ssim_sum, ssim_count);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int mvd_depth_metrics(const float* pred, const float* target, const unsigned char* valid, int B, int H, int W, int align,
                                 const double* fit_in, double* fit, double* sums, long long* counts, void* scratch, size_t scratch_bytes,
                                 mvd_stream_t stream) {
  const char* fn = "mvd_depth_metrics";
  MVD_CHECK_ARG(B >= 0 && B <= 65535, "%s: B=%d outside [0, 65535]", fn, B);
  MVD_CHECK_ARG(H >= 1 && H <= kVmMaxSide && W >= 1 && W <= kVmMaxSide, "%s: H=%d, W=%d outside [1, %d]", fn, H, W, kVmMaxSide);
  MVD_CHECK_ARG(align >= MVD_DEPTH_ALIGN_NONE && align <= MVD_DEPTH_ALIGN_GIVEN,
                "%s: align=%d (MVD_DEPTH_ALIGN_NONE, _SCALE, _SCALE_SHIFT or _GIVEN)", fn, align);
  MVD_CHECK_ARG((align == MVD_DEPTH_ALIGN_GIVEN) == (fit_in != nullptr), "%s: fit_in goes with align=MVD_DEPTH_ALIGN_GIVEN and with no other (align=%d)",
                fn, align);
  VmDepthPlan p;
  MVD_CHECK_ARG(vm_depth_plan(B, H, W, p), "%s: no plan for B=%d, H=%d, W=%d", fn, B, H, W);
  if (B == 0) return 0;
  MVD_CHECK_ARG(pred && target, "%s: null depth map", fn);
  MVD_CHECK_ARG(scratch && scratch_bytes >= p.words * 8 && ((uintptr_t)scratch & 7) == 0,
                "%s: scratch of %zu bytes at %p (mvd_depth_metrics_scratch: %zu bytes, 8-byte aligned)", fn, scratch_bytes, scratch, p.words * 8);
  double* sd = (double*)scratch;
  long long* sl = (long long*)scratch;
  const hipStream_t st = (hipStream_t)stream;
  const size_t HW = (size_t)H * (size_t)W;
  const dim3 grid((unsigned)p.nchunk, B);
  const double* use = fit_in;
  if (!fit_in) {
    hipLaunchKernelGGL(vm_depth_fit_kernel, grid, dim3(kVmThreads), 0, st, pred, target, valid, HW, sd + p.fit_part, sl + p.n_part);
    MVD_CHECK_LAUNCH(fn);
    hipLaunchKernelGGL(vm_depth_solve_kernel, dim3(B), dim3(kVmThreads), 0, st, sd + p.fit_part, sl + p.n_part, (size_t)p.nchunk, align, sd + p.fit);
    MVD_CHECK_LAUNCH(fn);
    use = sd + p.fit;
  }
  hipLaunchKernelGGL(vm_depth_err_kernel, grid, dim3(kVmThreads), 0, st, pred, target, valid, HW, use, sd + p.err_part, sl + p.cnt_part);
  MVD_CHECK_LAUNCH(fn);
  hipLaunchKernelGGL(vm_depth_final_kernel, dim3(B), dim3(kVmThreads), 0, st, sd + p.err_part, sl + p.cnt_part, use, (size_t)p.nchunk, fit, sums, counts);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}
