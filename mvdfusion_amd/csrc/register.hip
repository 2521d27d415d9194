// Global registration: the truncated cost of H pose hypotheses per scene against a target whose grid is already built, and the greedy
// choice of K distinct best (include/mvd_hip.h: mvd_register_score, mvd_register_select have the rules in full).
//
// score_kernel: one workgroup per (scene, hypothesis, chunk of kAlChunk sample rows) -- blockIdx.x finds its (scene, chunk) in first[]
// exactly as accumulate_kernel of align.hip does, blockIdx.y is the hypothesis, whose 12 doubles are uniform over the workgroup.  Thread t
// moves its rows k * 256 + t (k ascending) by al_apply, THE apply rule, and searches the moved point:
//   GRID : nn_walk_grid of nn_grid.hpp, the walk of mvd_nearest_points, over the records mvd_nearest_points_stages(MVD_NN_BUILD) sorted, with
//          RegKeep in place of NNOne.  RegKeep keeps the least d2 by the strict comparison of nn_take -- the value NNOne ends with -- but
//          holds min(best, trunc2) against the walk's bound.  The walk stops after shell r when worst() < bound * 0.999, bound being, with
//          its margins, below the fp32 d2 of every target in a cell not yet visited (the argument of nn_grid.hpp, unchanged).  So when it
//          stops with best <= trunc2, worst() is best and best is the minimum, as in mvd_nearest_points.  When it stops with
//          best > trunc2, worst() is trunc2: every unvisited d2 > trunc2 by the same bound and every visited one >= best > trunc2, so the
//          minimum is > trunc2 too -- the cost is trunc2 and the row no inlier, whatever the walk left unseen.  The cost and the inlier
//          bit are those of the full search; a hypothesis that throws the cloud far from the target ends after its first shell.
//   BRUTE: the targets of the scene staged through LDS in tiles, every row of the chunk against every record, the same strict comparison.
// The costs (double)c are added per thread in row order, the 64 lanes of a wavefront meet in an xor butterfly, the four wavefronts as
// (w0 + w1) + (w2 + w3): the order of MVD_ALIGN_SUMS.  add_kernel: one thread per (scene, hypothesis) adds the chunk sums in ascending
// chunk order.  No float atomics; nothing per row is written.
// select_kernel: one workgroup per scene, K rounds of { argmin of (score, h) over the live hypotheses: per thread over its h = t, t + 256,
// ..., then across the workgroup -- the order is total, so the result does not depend on how it is reduced --; kill the neighbours of the
// winner }.  The live flags are bytes in LDS; the scores are re-read from memory (H doubles, cached) every round.
#include "align_common.hpp"
#include "nn_points.hpp"

namespace {

constexpr int kRgTile = 1024;                         // float4 records per LDS tile of the brute scan (16 KB)
constexpr int kRgRows = kAlChunk / kAlThreads;        // rows per thread
constexpr int kRgMaxH = MVD_REGISTER_MAX_H;
constexpr int kRgMaxK = MVD_REGISTER_MAX_K;

struct RegArgs {
  const float *sample, *target;
  const int *sstart, *tstart;
  const double* hyp;                                  // (nscene, H, 12)
  unsigned* first;                                    // nscene + 1 words: chunks before scene s; [nscene] = all of them
  double* partial;                                    // (nwg, H) chunk sums
  int* ipartial;                                      // (nwg, H) chunk inlier counts
  double* score;
  int* inliers;
  NNArgs nn;                                          // the built grid: sorted, box, cells, nt, nscene, g
  long long ns, nt;
  int nscene, H;
  unsigned nwg;                                       // the launch's workgroups along x: the host bound ceil(ns / kAlChunk) + nscene
  float trunc2;
};

// The moved point of one row as the `query` of the walk: nn_walk_grid reads a.query[i * 3 + 0 .. 2] of its own row i only.
struct RegQuery {
  float x, y, z;
  long long base;                                     // i * 3
  NN_HD float operator[](long long k) const { return k == base ? x : (k == base + 1 ? y : z); }
};
// The arguments of the walk for one row: what nn_walk_grid asks of `Args`
struct RegWalk {
  RegQuery query;
  const int *qstart, *tstart;
  const unsigned* box;
  long long nq, nt;
  int nscene, g;
  const NNArgs* nn;
};
template <class Keep>
NN_HD void nn_visit(const RegWalk& a, long long scene_cell0, long long ca, long long cb, long long t0, long long t1, float qx, float qy, float qz,
                    Keep& keep) {
  nn_visit(*a.nn, scene_cell0, ca, cb, t0, t1, qx, qy, qz, keep);
}

// The least d2 (nn_take's strict comparison: a NaN or an infinite d2 never wins), held against the walk's bound as min(best, trunc2).
struct RegKeep {
  float best, trunc2;
  NN_HD explicit RegKeep(float t2) : best(INFINITY), trunc2(t2) {}
  NN_HD void take(float d2, int) {
    if (d2 < best) best = d2;
  }
  NN_HD float worst() const { return fminf(best, trunc2); }
};

// THE cost rule of the header: c and the inlier bit from the least d2 (+inf when nothing was found; a NaN compares false)
NN_HD void rg_cost(float d2, float trunc2, double& acc, int& cnt) {
  const bool in = d2 <= trunc2;
  acc += (double)(in ? d2 : trunc2);
  cnt += in ? 1 : 0;
}

// first[s] before the scan: the chunks of scene s (align.hip's chunk map, on the sample's offsets)
__global__ __launch_bounds__(kAlThreads) void sample_chunks_kernel(RegArgs a) {
  const int s = blockIdx.x * kAlThreads + threadIdx.x;
  if (s < a.nscene) a.first[s] = al_chunks_of(a.sstart, s, a.ns);
}

template <bool GRID>
__global__ __launch_bounds__(kAlThreads) void score_kernel(RegArgs a) {
  __shared__ float4 tile[GRID ? 1 : kRgTile];
  __shared__ double wave_s[kAlThreads / 64];
  __shared__ int wave_n[kAlThreads / 64];
  const unsigned b = blockIdx.x;
  const int h = blockIdx.y;
  if (b >= a.first[a.nscene]) return;      // (uniform) the bound's slack
  int lo = 0, hi = a.nscene;               // the last scene with first[s] <= b: first[0] = 0, an empty scene owns no chunk
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.first[mid] <= b) lo = mid;
    else hi = mid;
  }
  const long long r0 = al_clamp(a.sstart[lo], a.ns) + (long long)(b - a.first[lo]) * kAlChunk;
  const long long end = al_clamp(a.sstart[lo + 1], a.ns), r1 = r0 + kAlChunk < end ? r0 + kAlChunk : end;
  double m[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) m[k] = a.hyp[((size_t)lo * a.H + h) * 12 + k];      // (uniform)
  double acc = 0.0;
  int cnt = 0;
  if (GRID) {
#pragma unroll 1
    for (int k = 0; k < kRgRows; ++k) {      // (one walk in the code, not kRgRows)
      const long long i = r0 + k * kAlThreads + threadIdx.x;
      if (i >= r1) continue;
      float q[3];
      al_apply(m, a.sample[i * 3 + 0], a.sample[i * 3 + 1], a.sample[i * 3 + 2], q);
      const RegWalk w{RegQuery{q[0], q[1], q[2], i * 3}, a.sstart, a.tstart, a.nn.box, a.ns, a.nt, a.nscene, a.nn.g, &a.nn};
      RegKeep keep(a.trunc2);
      nn_walk_grid(w, i, keep);
      rg_cost(keep.best, a.trunc2, acc, cnt);
    }
  } else {
    float p[kRgRows][3], best[kRgRows];
#pragma unroll
    for (int k = 0; k < kRgRows; ++k) {
      const long long i = r0 + k * kAlThreads + threadIdx.x;
      p[k][0] = p[k][1] = p[k][2] = 0.f, best[k] = INFINITY;
      if (i < r1) al_apply(m, a.sample[i * 3 + 0], a.sample[i * 3 + 1], a.sample[i * 3 + 2], p[k]);
    }
    const long long t0 = al_clamp(a.tstart[lo], a.nt), t1 = al_clamp(a.tstart[lo + 1], a.nt);
    for (long long base = t0; base < t1; base += kRgTile) {      // (uniform)
      const int n = (int)min((long long)kRgTile, t1 - base);
      __syncthreads();      // the previous tile has been read
      for (int k = threadIdx.x; k < n; k += kAlThreads) {
        const long long j = base + k;
        tile[k] = make_float4(a.target[j * 3 + 0], a.target[j * 3 + 1], a.target[j * 3 + 2], 0.f);
      }
      __syncthreads();
      for (int j = 0; j < n; ++j) {
        const float4 r = tile[j];      // (every lane reads the same record: a broadcast)
#pragma unroll
        for (int k = 0; k < kRgRows; ++k) {
          const float d2 = nn_d2(p[k][0], p[k][1], p[k][2], r.x, r.y, r.z);
          if (d2 < best[k]) best[k] = d2;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kRgRows; ++k)
      if (r0 + k * kAlThreads + threadIdx.x < r1) rg_cost(best[k], a.trunc2, acc, cnt);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64), cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) wave_s[threadIdx.x >> 6] = acc, wave_n[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    a.partial[(size_t)b * a.H + h] = (wave_s[0] + wave_s[1]) + (wave_s[2] + wave_s[3]);
    a.ipartial[(size_t)b * a.H + h] = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
  }
}

// One thread per (scene, hypothesis): the chunk sums of the scene in ascending chunk order.
__global__ __launch_bounds__(kAlThreads) void add_kernel(RegArgs a) {
  const int h = blockIdx.x * kAlThreads + threadIdx.x, s = blockIdx.y;
  if (h >= a.H) return;
  const unsigned c0 = min(a.first[s], a.nwg), c1 = min(a.first[s + 1], a.nwg);
  double v = 0.0;
  int n = 0;
  for (unsigned c = c0; c < c1; ++c) v += a.partial[(size_t)c * a.H + h], n += a.ipartial[(size_t)c * a.H + h];
  a.score[(size_t)s * a.H + h] = v;
  a.inliers[(size_t)s * a.H + h] = n;
}

// (score, h) of a candidate, h = -1 for none; `a` comes before `b` in THE order of the header
struct RegBest {
  double s;
  int h;
};
__device__ __forceinline__ bool rg_before(const RegBest& a, const RegBest& b) { return a.h >= 0 && (b.h < 0 || a.s < b.s || (a.s == b.s && a.h < b.h)); }

__global__ __launch_bounds__(kAlThreads) void select_kernel(const double* __restrict__ score, const double* __restrict__ quat, double cos_half, int H,
                                                            int K, int* __restrict__ top, double* __restrict__ top_score) {
  __shared__ unsigned char dead[kRgMaxH];
  __shared__ RegBest wave_b[kAlThreads / 64];
  const int s = blockIdx.x;
  const double* sc = score + (size_t)s * H;
  for (int h = threadIdx.x; h < H; h += kAlThreads) dead[h] = sc[h] != sc[h];      // a NaN score is never taken
  for (int k = 0; k < K; ++k) {      // (uniform)
    RegBest mine{0.0, -1};
    for (int h = threadIdx.x; h < H; h += kAlThreads)      // (a thread reads only the flags it wrote itself)
      if (!dead[h]) {
        const RegBest c{sc[h], h};
        if (rg_before(c, mine)) mine = c;
      }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const RegBest other{__shfl_xor(mine.s, o, 64), __shfl_xor(mine.h, o, 64)};
      if (rg_before(other, mine)) mine = other;
    }
    __syncthreads();      // the previous round's wave_b has been read
    if ((threadIdx.x & 63) == 0) wave_b[threadIdx.x >> 6] = mine;
    __syncthreads();
    RegBest win = wave_b[0];
#pragma unroll
    for (int w = 1; w < kAlThreads / 64; ++w)
      if (rg_before(wave_b[w], win)) win = wave_b[w];
    if (threadIdx.x == 0) {
      top[(size_t)s * K + k] = win.h;
      top_score[(size_t)s * K + k] = win.h >= 0 ? win.s : (double)INFINITY;
    }
    if (win.h < 0) continue;      // (uniform) nothing is left: the remaining rounds write -1 / +inf
    const double q0 = quat[win.h * 4 + 0], q1 = quat[win.h * 4 + 1], q2 = quat[win.h * 4 + 2], q3 = quat[win.h * 4 + 3];
    for (int h = threadIdx.x; h < H; h += kAlThreads) {
      const double dot = ((q0 * quat[h * 4 + 0] + q1 * quat[h * 4 + 1]) + q2 * quat[h * 4 + 2]) + q3 * quat[h * 4 + 3];
      if (fabs(dot) >= cos_half || h == win.h) dead[h] = 1;
    }
  }
}

struct RegPlan {
  unsigned nwg;
  NNLayout nn;
  size_t nn_bytes, off_first, off_partial, off_ipartial, bytes;
};

// false: an argument is out of range
static bool rg_plan(size_t ns, size_t nt, int nscene, int H, int method, int grid, RegPlan& p) {
  p = RegPlan{};
  if (nscene < 1 || nscene > 65535 || ns > 0x7fffffffull || nt > 0x7fffffffull || H < 1 || H > kRgMaxH || method < MVD_NN_AUTO ||
      method > MVD_NN_GRID || grid < 0 || grid > 256)
    return false;
  if (method != MVD_NN_BRUTE && (unsigned long long)nscene * grid * grid * grid > 0x7fffffffull) return false;
  p.nwg = (unsigned)((ns + kAlChunk - 1) / kAlChunk) + (unsigned)nscene;
  if (!nn_points_layout(nt, nscene, method, grid, &p.nn)) return false;
  p.nn_bytes = p.nn.bytes;      // the head of the scratch: the grid as MVD_NN_BUILD leaves it
  p.off_first = al_up16(p.nn_bytes);
  p.off_partial = p.off_first + al_up16((size_t)(nscene + 1) * sizeof(unsigned));
  p.off_ipartial = p.off_partial + al_up16((size_t)p.nwg * H * sizeof(double));
  p.bytes = p.off_ipartial + al_up16((size_t)p.nwg * H * sizeof(int));
  return true;
}

}  // namespace

extern "C" size_t mvd_register_scratch(size_t ns, size_t nt, int nscene, int H, int method, int grid) {
  RegPlan p;
  return rg_plan(ns, nt, nscene, H, method, grid, p) ? p.bytes : 0;
}

extern "C" int mvd_register_score(const float* sample, const int* sample_start, const float* target, const int* target_start, size_t ns,
                                  size_t nt, int nscene, int H, const double* hyp, float trunc2, int method, int grid, double* score,
                                  int* inliers, void* scratch, size_t scratch_bytes, mvd_stream_t stream) {
  const char* fn = "mvd_register_score";
  MVD_CHECK_ARG(method >= MVD_NN_AUTO && method <= MVD_NN_GRID, "%s: method=%d (MVD_NN_AUTO, _BRUTE or _GRID)", fn, method);
  MVD_CHECK_ARG(grid >= 0 && grid <= 256, "%s: grid=%d outside [0, 256]", fn, grid);
  MVD_CHECK_ARG(nscene >= 1 && nscene <= 65535, "%s: nscene=%d outside [1, 65535]", fn, nscene);
  MVD_CHECK_ARG(H >= 1 && H <= kRgMaxH, "%s: H=%d outside [1, %d]", fn, H, kRgMaxH);
  MVD_CHECK_ARG(ns <= 0x7fffffffull && nt <= 0x7fffffffull, "%s: ns=%zu, nt=%zu beyond 2^31 - 1", fn, ns, nt);
  MVD_CHECK_ARG(trunc2 > 0.f && trunc2 < INFINITY, "%s: trunc2=%g (finite and > 0)", fn, (double)trunc2);
  MVD_CHECK_ARG(sample_start && target_start && hyp && score && inliers, "%s: null sample_start, target_start, hyp, score or inliers", fn);
  MVD_CHECK_ARG(sample || ns == 0, "%s: null sample with ns=%zu", fn, ns);
  MVD_CHECK_ARG(target || nt == 0, "%s: null target with nt=%zu", fn, nt);
  MVD_CHECK_ARG(al_aligned(hyp, 8) && al_aligned(score, 8), "%s: hyp or score not 8-byte aligned", fn);
  const uintptr_t low = (uintptr_t)sample | (uintptr_t)sample_start | (uintptr_t)target | (uintptr_t)target_start | (uintptr_t)inliers;
  MVD_CHECK_ARG((low & 3) == 0, "%s: a pointer that is not 4-byte aligned", fn);
  RegPlan p;
  MVD_CHECK_ARG(rg_plan(ns, nt, nscene, H, method, grid, p), "%s: nscene * grid^3 cells beyond 2^31 - 1 (nscene=%d, grid=%d)", fn, nscene, grid);
  MVD_CHECK_ARG(scratch && scratch_bytes >= p.bytes && al_aligned(scratch, 16), "%s: scratch of %zu bytes (needs %zu, 16-byte aligned)", fn,
                scratch_bytes, p.bytes);
  char* base = (char*)scratch;
  RegArgs a{};
  a.sample = sample, a.target = target, a.sstart = sample_start, a.tstart = target_start, a.hyp = hyp;
  a.first = (unsigned*)(base + p.off_first), a.partial = (double*)(base + p.off_partial), a.ipartial = (int*)(base + p.off_ipartial);
  a.score = score, a.inliers = inliers;
  a.ns = (long long)ns, a.nt = (long long)nt, a.nscene = nscene, a.H = H, a.nwg = p.nwg, a.trunc2 = trunc2;
  const bool grid_method = p.nn.method == MVD_NN_GRID;
  a.nn = NNArgs{nullptr, target, sample_start, target_start, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (long long)ns, (long long)nt, nscene, p.nn.g, 0};
  if (grid_method) a.nn.sorted = (Rec*)base, a.nn.box = (unsigned*)(base + p.nn.off_box), a.nn.cells = (unsigned*)(base + p.nn.off_cells);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sample_chunks_kernel, dim3(cdiv(nscene, kAlThreads)), dim3(kAlThreads), 0, st, a);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kCompactThreads), 0, st, a.first, (unsigned)nscene, a.first + nscene);
  const dim3 blocks(p.nwg, (unsigned)H), threads(kAlThreads);
  if (grid_method) hipLaunchKernelGGL(score_kernel<true>, blocks, threads, 0, st, a);
  else hipLaunchKernelGGL(score_kernel<false>, blocks, threads, 0, st, a);
  hipLaunchKernelGGL(add_kernel, dim3(cdiv(H, kAlThreads), (unsigned)nscene), threads, 0, st, a);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int mvd_register_select(const double* score, const double* quat, int nscene, int H, int K, double cos_half, int* top,
                                   double* top_score, mvd_stream_t stream) {
  const char* fn = "mvd_register_select";
  MVD_CHECK_ARG(nscene >= 1 && nscene <= 65535, "%s: nscene=%d outside [1, 65535]", fn, nscene);
  MVD_CHECK_ARG(H >= 1 && H <= kRgMaxH, "%s: H=%d outside [1, %d]", fn, H, kRgMaxH);
  MVD_CHECK_ARG(K >= 1 && K <= kRgMaxK, "%s: K=%d outside [1, %d]", fn, K, kRgMaxK);
  MVD_CHECK_ARG(cos_half == cos_half, "%s: cos_half is a NaN (> 1 for no suppression)", fn);
  MVD_CHECK_ARG(score && quat && top && top_score, "%s: null score, quat, top or top_score", fn);
  MVD_CHECK_ARG(al_aligned(score, 8) && al_aligned(quat, 8) && al_aligned(top_score, 8) && al_aligned(top, 4),
                "%s: score, quat or top_score not 8-byte aligned, or top not 4-byte aligned", fn);
  hipLaunchKernelGGL(select_kernel, dim3((unsigned)nscene), dim3(kAlThreads), 0, (hipStream_t)stream, score, quat, cos_half, H, K, top, top_score);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}
