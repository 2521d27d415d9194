// What the grid searches share (nearest.hip: the nearest and the k nearest POINTS; meshdist.hip: the nearest FACE of a mesh): the
// order-preserving keys of the bounding box, a scene's grid from its box, the cell function, the Chebyshev shell walk with its stop rule,
// and the two chunk levels of the exclusive scan of the cell counts.  One copy, so a point and a face are assigned to cells by the same
// expressions in the same order, and the stop rule of the walk -- with its margins -- is argued once.
//
// The walk is a template over the search's arguments `Args` and over what it keeps per query `Keep`.  Args has query, qstart, tstart,
// box, nq, nt, nscene and g; nn_visit(a, first cell of the scene, ca, cb, t0, t1, qx, qy, qz, keep) is the search's own: it offers what the
// cells [ca, cb] of the scene hold to keep.take(), and keep.worst() is the distance the walk holds against its bound.
#pragma once
#include "fusion_common.hpp"

namespace {

#define NN_HD __host__ __device__ __forceinline__

constexpr int kNNThreads = 256;
constexpr int kChunk = 4096;                          // cell counts one workgroup scans: 16 consecutive words per thread
constexpr float kHFloor = 1e-30f;                     // the positive floor of the cell side
constexpr float kUClamp = 1e9f;                       // a query's position in cell units is clamped to this (towards the box: conservative)

// fp32 -> unsigned that orders like the value (-inf lowest; NaNs at the two ends, and no NaN is ever encoded here)
NN_HD unsigned nn_key(float v) {
#ifdef __HIP_DEVICE_COMPILE__
  const unsigned b = __float_as_uint(v);
#else
  unsigned b;
  __builtin_memcpy(&b, &v, 4);
#endif
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
NN_HD float nn_unkey(unsigned k) {
  const unsigned b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
#ifdef __HIP_DEVICE_COMPILE__
  return __uint_as_float(b);
#else
  float v;
  __builtin_memcpy(&v, &b, 4);
  return v;
#endif
}

NN_HD bool nn_finite(float v) { return fabsf(v) < INFINITY; }      // (a NaN compares false)

NN_HD long long nn_clamp(long long v, long long n) { return v < 0 ? 0 : (v > n ? n : v); }
NN_HD int nn_lo(int a, int b) { return a < b ? a : b; }
NN_HD int nn_hi(int a, int b) { return a > b ? a : b; }

// The scene s with start[s] <= i < start[s + 1] (values clamped to [0, n]), or -1.  At most 16 steps.
NN_HD int nn_find_scene(const int* start, int nscene, long long n, long long i) {
  if (i < nn_clamp(start[0], n)) return -1;
  int lo = 0, hi = nscene;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (nn_clamp(start[mid], n) <= i) lo = mid;
    else hi = mid;
  }
  return i < nn_clamp(start[lo + 1], n) ? lo : -1;
}

// A scene's grid from its box: cubic cells of side h, n[a] cells along axis a.  ok is false for a scene without a finite target.
struct SceneGrid {
  float mn[3], mx[3], h, inv_h;
  int n[3];
  bool ok;
};
NN_HD SceneGrid nn_scene_grid(const unsigned* box, int g) {
  SceneGrid G;
  float ext[3], big = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    G.mn[a] = nn_unkey(box[a]);
    G.mx[a] = nn_unkey(~box[3 + a]);
    ext[a] = fminf(fmaxf(G.mx[a] - G.mn[a], 0.f), 3e38f);      // (a NaN -- the empty box -- gives 0)
    big = fmaxf(big, ext[a]);
  }
  G.ok = G.mn[0] <= G.mx[0] && G.mn[1] <= G.mx[1] && G.mn[2] <= G.mx[2];
  G.h = fmaxf(big / (float)g, kHFloor);
  G.inv_h = 1.0f / G.h;
#pragma unroll
  for (int a = 0; a < 3; ++a) G.n[a] = (int)fminf(fmaxf(floorf(ext[a] * G.inv_h) + 1.f, 1.f), (float)g);      // clamped BEFORE the conversion
  return G;
}
// position along axis a in cell units (not clamped), and the cell: clamped to [0, n - 1] before the conversion, a NaN to 0
NN_HD float nn_units(const SceneGrid& G, int a, float x) { return (x - G.mn[a]) * G.inv_h; }
NN_HD int nn_cell(const SceneGrid& G, int a, float u) { return (int)fminf(fmaxf(floorf(u), 0.f), (float)(G.n[a] - 1)); }
NN_HD long long nn_cell_of(const SceneGrid& G, float x, float y, float z) {
  const int cx = nn_cell(G, 0, nn_units(G, 0, x)), cy = nn_cell(G, 1, nn_units(G, 1, y)), cz = nn_cell(G, 2, nn_units(G, 2, z));
  return ((long long)cz * G.n[1] + cy) * G.n[0] + cx;
}

// One query against the built grid: every candidate that can still matter is offered to `keep`.
template <class Args, class Keep>
NN_HD void nn_walk_grid(const Args& a, long long i, Keep& keep) {
  const int s = nn_find_scene(a.qstart, a.nscene, a.nq, i);
  if (s >= 0) {
    const long long t0 = nn_clamp(a.tstart[s], a.nt), t1 = nn_clamp(a.tstart[s + 1], a.nt);
    const SceneGrid G = nn_scene_grid(a.box + (size_t)s * 6, a.g);
    if (G.ok && t0 < t1) {
      const float q[3] = {a.query[i * 3 + 0], a.query[i * 3 + 1], a.query[i * 3 + 2]};
      const long long cell0 = (long long)s * a.g * a.g * a.g;
      float u[3], out2[3];
      int c[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float uk = nn_units(G, k, q[k]);
        c[k] = nn_cell(G, k, uk);
        u[k] = fminf(fmaxf(uk, -kUClamp), kUClamp);
        // what the query lies outside the box along the axis: every target is inside it, exactly
        const float o = fmaxf(fmaxf(G.mn[k] - q[k], q[k] - G.mx[k]), 0.f) * 0.999f;
        out2[k] = o * o;
      }
      for (int r = 0; r < a.g; ++r) {      // (a host value bounds the loop whatever the data)
        const int z0 = nn_hi(c[2] - r, 0), z1 = nn_lo(c[2] + r, G.n[2] - 1), y0 = nn_hi(c[1] - r, 0), y1 = nn_lo(c[1] + r, G.n[1] - 1);
        const int xa = nn_hi(c[0] - r, 0), xb = nn_lo(c[0] + r, G.n[0] - 1);
        for (int z = z0; z <= z1; ++z)
          for (int y = y0; y <= y1; ++y) {
            const long long row = ((long long)z * G.n[1] + y) * G.n[0];
            // a face of the shell: the whole row, one range; inside (r >= 1): the row's two ends.  One visit site for both, so that
            // what `keep` unrolls is compiled once.
            const bool face = z - c[2] == r || c[2] - z == r || y - c[1] == r || c[1] - y == r;
            for (int part = 0; part < (face ? 1 : 2); ++part) {
              const int x = part == 0 ? c[0] - r : c[0] + r;
              if (!face && (x < 0 || x >= G.n[0])) continue;
              nn_visit(a, cell0, row + (face ? xa : x), row + (face ? xb : x), t0, t1, q[0], q[1], q[2], keep);
            }
          }
        // a lower bound of d2 to any point of an unvisited cell: such a cell lies beyond a face of the visited block along some axis
        float bound = INFINITY;
        bool left = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float others = (out2[(k + 1) % 3] + out2[(k + 2) % 3]);
          if (c[k] + r + 1 < G.n[k]) {      // cells >= c + r + 1: their points sit at >= c + r + 1 cell units
            const float gap = fmaxf(((float)(c[k] + r + 1) - u[k]) - 0.001f, 0.f) * 0.999f * G.h;
            bound = fminf(bound, gap * gap + others);
            left = true;
          }
          if (c[k] - r > 0) {               // cells <= c - r - 1: their points sit below c - r cell units
            const float gap = fmaxf((u[k] - (float)(c[k] - r)) - 0.001f, 0.f) * 0.999f * G.h;
            bound = fminf(bound, gap * gap + others);
            left = true;
          }
        }
        if (!left || keep.worst() < bound * 0.999f) break;
      }
    }
  }
}

// keys only decrease: a stale read costs an unnecessary atomic, never a wrong result (fusion.hip: splat_kernel)
__device__ __forceinline__ void key_min(unsigned* slot, unsigned key) {
  if (*slot <= key) return;
  atomicMin(slot, key);
}

// The two chunk levels of the scan around scan_kernel.  The cell array is padded to whole chunks (and zeroed): no bounds in here.
__global__ __launch_bounds__(kNNThreads) void chunk_sum_kernel(const unsigned* __restrict__ cells, unsigned* __restrict__ blocks) {
  __shared__ unsigned wave_n[kNNThreads / 64];
  const uint4* p = (const uint4*)(cells + (size_t)blockIdx.x * kChunk + threadIdx.x * 16);
  unsigned v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint4 w = p[k];
    v += (w.x + w.y) + (w.z + w.w);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor((int)v, o, 64);
  if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) blocks[blockIdx.x] = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
}

__global__ __launch_bounds__(kNNThreads) void chunk_scan_kernel(unsigned* __restrict__ cells, const unsigned* __restrict__ blocks) {
  __shared__ unsigned wave_n[kNNThreads / 64];
  uint4* p = (uint4*)(cells + (size_t)blockIdx.x * kChunk + threadIdx.x * 16);
  unsigned w[16], mine = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint4 t = p[k];
    w[k * 4 + 0] = t.x, w[k * 4 + 1] = t.y, w[k * 4 + 2] = t.z, w[k * 4 + 3] = t.w;
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) {      // exclusive within the thread
    const unsigned t = w[k];
    w[k] = mine;
    mine += t;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wave_n[wave] = incl;
  __syncthreads();
  unsigned before = blocks[blockIdx.x] + incl - mine;
  for (int k = 0; k < wave; ++k) before += wave_n[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) p[k] = make_uint4(w[k * 4 + 0] + before, w[k * 4 + 1] + before, w[k * 4 + 2] + before, w[k * 4 + 3] + before);
}

static size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace
