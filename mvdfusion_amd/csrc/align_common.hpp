// What the units that move a source by a per-scene transform share (align.hip: the fits and the ICP loops; register.hip: the score of
// pose hypotheses): THE apply rule, the scene of a row, and the number of kAlChunk-row chunks of a scene, from which each unit forms
// first[s] = the chunks of the scenes before s on the device.  One copy of each.
#pragma once
#include "fusion_common.hpp"

namespace {

#define AL_HD __host__ __device__ __forceinline__

constexpr int kAlThreads = 256;
constexpr int kAlChunk = MVD_ALIGN_CHUNK;             // rows one workgroup reduces: kAlChunk / kAlThreads per thread
static_assert(kAlChunk % kAlThreads == 0, "whole rows per thread");

AL_HD long long al_clamp(long long v, long long n) { return v < 0 ? 0 : (v > n ? n : v); }

// The scene s with start[s] <= i < start[s + 1] (values clamped to [0, n]), or -1: mvd_nearest_points' membership rule.
AL_HD int al_find_scene(const int* start, int nscene, long long n, long long i) {
  if (i < al_clamp(start[0], n)) return -1;
  int lo = 0, hi = nscene;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (al_clamp(start[mid], n) <= i) lo = mid;
    else hi = mid;
  }
  return i < al_clamp(start[lo + 1], n) ? lo : -1;
}

// THE apply rule of the header, in its order
AL_HD void al_apply(const double* m, float x, float y, float z, float* out) {
#pragma unroll
  for (int r = 0; r < 3; ++r) out[r] = (float)(((m[r * 4 + 0] * (double)x + m[r * 4 + 1] * (double)y) + m[r * 4 + 2] * (double)z) + m[r * 4 + 3]);
}

// the kAlChunk-row chunks of scene s
AL_HD unsigned al_chunks_of(const int* start, int s, long long n) {
  const long long len = al_clamp(start[s + 1], n) - al_clamp(start[s], n);
  return len > 0 ? (unsigned)((len + kAlChunk - 1) / kAlChunk) : 0u;
}

static size_t al_up16(size_t v) { return (v + 15) & ~(size_t)15; }
static bool al_aligned(const void* p, size_t to) { return ((uintptr_t)p & (to - 1)) == 0; }

}  // namespace
