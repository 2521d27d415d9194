// What the kernels behind mvdfusion_amd/fusion.py share (fusion.hip: point fusion and splatting; tsdf.hip: volumetric fusion and meshing):
// the normalised depth, the projection that also returns camera-space z, and the single-workgroup scan of the stream compactions.  One copy,
// so a voxel of the TSDF and a point of the cloud see a view's depth map through the same expressions in the same order.
#pragma once
#include "gridattn_common.hpp"

namespace {

constexpr int kCompactThreads = 256;                  // 4 wavefronts: a block count is at most 256

// the depth channel normalised to [0, 1], the value the foreground test and the metric depth are taken from
__device__ __forceinline__ float depth01(float lat) { return fminf(fmaxf((lat + 1.0f) / 2.0f, 0.f), 1.f); }

// project() of gridattn_common.hpp that also returns camera-space z (the depth the other view's map is compared with)
// ... and the whole camera-space point xc (texture.hip: the viewing direction of a texel); project_z is this with zc = xc[2]
__device__ __forceinline__ void project_xc(const Cam& c, const float* X, float& u, float& w, float* xc) {
#pragma unroll
  for (int j = 0; j < 3; ++j) xc[j] = X[0] * c.R[0 * 3 + j] + X[1] * c.R[1 * 3 + j] + X[2] * c.R[2 * 3 + j] + c.T[j];
  u = c.f[0] * xc[0] / xc[2] + c.p[0];
  w = c.f[1] * xc[1] / xc[2] + c.p[1];
}
__device__ __forceinline__ void project_z(const Cam& c, const float* X, float& u, float& w, float& zc) {
  float xc[3];
  project_xc(c, X, u, w, xc);
  zc = xc[2];
}

// The pixel-centre lookup of NDC (u, w) in an S x S map: geometric pixel centres with a border clamp (NDC +1 is the left / top edge of
// pixel 0), the four taps y * S + x and the weights of the second column / row.
struct PixelTaps {
  int idx[4];
  float wx, wy;
};
__device__ __forceinline__ PixelTaps pixel_taps(float u, float w, int S) {
  const float S2 = 0.5f * (float)S, Sm1 = (float)(S - 1);
  const float ix = fminf(fmaxf((1.f - u) * S2 - 0.5f, 0.f), Sm1), iy = fminf(fmaxf((1.f - w) * S2 - 0.5f, 0.f), Sm1);
  const float x0f = floorf(ix), y0f = floorf(iy);
  const int x0 = (int)x0f, y0 = (int)y0f, x1 = min(x0 + 1, S - 1), y1 = min(y0 + 1, S - 1);
  PixelTaps t;
  t.wx = ix - x0f;
  t.wy = iy - y0f;
  t.idx[0] = y0 * S + x0;
  t.idx[1] = y0 * S + x1;
  t.idx[2] = y1 * S + x0;
  t.idx[3] = y1 * S + x1;
  return t;
}
// the bilinear mix of the four tap values, in THE evaluation order
__device__ __forceinline__ float bilinear_mix(const float* z, const PixelTaps& t) {
  return (z[0] * (1.f - t.wx) + z[1] * t.wx) * (1.f - t.wy) + (z[2] * (1.f - t.wx) + z[3] * t.wx) * t.wy;
}

// one workgroup: exclusive scan of the block counts in place, kCompactThreads at a time with a running carry; the total to *count
__global__ __launch_bounds__(kCompactThreads) void scan_kernel(unsigned* __restrict__ blocks, unsigned nblocks, unsigned* __restrict__ count) {
  __shared__ unsigned wave_n[kCompactThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned carry = 0;
  for (unsigned base = 0; base < nblocks; base += kCompactThreads) {
    const unsigned i = base + threadIdx.x;
    const unsigned v = i < nblocks ? blocks[i] : 0u;
    unsigned incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) wave_n[wave] = incl;
    __syncthreads();
    unsigned before = carry, all = 0;
#pragma unroll
    for (int w = 0; w < kCompactThreads / 64; ++w) {
      if (w < wave) before += wave_n[w];
      all += wave_n[w];
    }
    if (i < nblocks) blocks[i] = before + incl - v;
    carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = carry;
}

}  // namespace
