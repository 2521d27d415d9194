// The exact nearest target point of every query point (include/mvd_hip.h: mvd_nearest_points has the rule in full).
//
// BRUTE: one thread per query; the workgroup walks the scenes its queries belong to and stages each scene's targets through LDS in tiles
// of kTile 16-byte records (x, y, z, j).  Every lane reads the same record at once: a broadcast, no bank conflict.  Targets arrive in
// ascending j, so the strict comparison alone keeps the lowest j between equal minima.
// GRID: box_kernel (the bounding box of every scene's finite targets: order-preserving integer keys under atomicMin, exact in any order)
// -> count_kernel (one integer atomicAdd per finite target into its cell) -> an exclusive scan of the cell counts (two levels: chunk
// sums, scan_kernel of fusion_common.hpp over the chunk sums, chunk scans) -> scatter_kernel (the atomicAdd that hands out a record's
// place turns a cell's begin into its end: afterwards cell c owns the records [cells[c - 1], cells[c])) -> grid_query_kernel, one
// thread per query through nn_query_grid: Chebyshev shells of cells around the query's (clamped) cell, a row of cells along x being ONE
// range of records, until the best distance lies below the lower bound of everything unvisited.
// The per-element pieces (nn_scene_grid, nn_cell, nn_query_grid, nn_find_scene) are host-and-device functions, so that the search can
// be run serially on a CPU against the brute force.
// K NEAREST (mvd_knn_points): the same two searches with another thing kept per query.  The shell walk (nn_walk_grid) and the brute
// scan (nn_brute_scan) are templates over what they keep: NNOne, the single best of mvd_nearest_points, or NNList<K>, the K best in
// ascending (d2, j) order.  K is a compile-time size (1, 2, 4, 8, 16, 32: the smallest that holds k) and the insertion is unrolled, so
// the list stays in registers: a runtime-indexed array would go to scratch memory.  Resource usage of the two K = 32 kernels and why not LDS: DESIGN.md section 6.00000000000000000.
//
// The keys, the grid of a scene, the cell function, the shell walk and the chunk scan live in nn_grid.hpp, which meshdist.hip (the nearest
// FACE of a mesh) includes too: one copy.  The record, the arguments, the distance, the single best and the visit of a range of cells
// live in nn_points.hpp, which register.hip (the truncated cost of a pose hypothesis) includes too; nn_points_layout tells it the plan.
//
// Not tried: sorting the queries by cell, one wavefront per query cell, a hashed grid.
#include "nn_grid.hpp"
#include "nn_points.hpp"

namespace {

constexpr int kTile = 1024;                           // records per LDS tile of the brute kernel (16 KB)
constexpr int kMaxGrid = 256;
// MVD_NN_AUTO: the grid from this many targets per scene upward; automatic grid = sqrt(targets per scene / kGridDivisor)
// (DESIGN.md section 6.000000000000000 has the sweeps both come from)
constexpr long long kGridMinTargets = 1024;
constexpr float kGridDivisor = 16.f;
// the same comparison as a predicate: candidate (d2, j) comes before entry (e2, ej) in the order of the header
NN_HD bool nn_before(float d2, int j, float e2, int ej) { return d2 < e2 || (d2 == e2 && j < ej); }

// The k best in ascending (d2, j) order in the LAST k of K slots, empty slots (+inf, -1) behind the ones found.  The K - k slots in
// front hold (-inf, -1), which no candidate comes before, so the last slot is always the k-th best and nothing depends on k but the
// initial fill and the final write.  Every loop has a compile-time trip count and every subscript is a constant after unrolling (picking
// slot k - 1 with a chain of selects instead is turned back into a runtime subscript by the compiler, and the list leaves the registers).
template <int K>
struct NNList {
  float d[K];
  int j[K];
  NN_HD explicit NNList(int k) {
#pragma unroll
    for (int s = 0; s < K; ++s) d[s] = s < K - k ? -INFINITY : INFINITY, j[s] = -1;
  }
  NN_HD void take(float d2, int id) {
    if (!nn_before(d2, id, d[K - 1], j[K - 1])) return;      // (an infinite or NaN d2 comes before nothing)
    bool here = true;                                        // the candidate comes before the old entry s
#pragma unroll
    for (int s = K - 1; s >= 1; --s) {
      const bool below = nn_before(d2, id, d[s - 1], j[s - 1]);      // ... and before s - 1 too: that entry moves up to s
      d[s] = below ? d[s - 1] : (here ? d2 : d[s]);
      j[s] = below ? j[s - 1] : (here ? id : j[s]);
      here = below;
    }
    if (here) d[0] = d2, j[0] = id;
  }
  NN_HD float worst() const { return d[K - 1]; }      // the k-th best so far, +inf with fewer than k
  NN_HD void write(const NNArgs& a, long long i, int k) const {
#pragma unroll
    for (int s = 0; s < K; ++s)
      if (s >= K - k) a.index[i * k + (s - (K - k))] = j[s], a.dist2[i * k + (s - (K - k))] = d[s];
  }
};

// One query against the built grid.  Writes index[i] and dist2[i].
NN_HD void nn_query_grid(const NNArgs& a, long long i) {
  NNOne one;
  nn_walk_grid(a, i, one);
  a.index[i] = one.bestj;
  a.dist2[i] = one.best;
}

// ---------------------------------------------------------------------------------------------------------------- kernels
// The brute scan of one workgroup: thread t's query (row i, dead past nq) against every target of its scene, offered to `keep`.
template <class Keep>
__device__ __forceinline__ void nn_brute_scan(const NNArgs& a, Rec* tile, int* span, long long i, Keep& keep) {
  const bool live = i < a.nq;
  const int s = live ? nn_find_scene(a.qstart, a.nscene, a.nq, i) : -1;
  if (threadIdx.x == 0) span[0] = a.nscene, span[1] = -1;
  __syncthreads();
  if (s >= 0) atomicMin(&span[0], s), atomicMax(&span[1], s);
  __syncthreads();
  const int s_lo = span[0], s_hi = span[1];      // (uniform: the scenes this workgroup's queries belong to)
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (live) qx = a.query[i * 3 + 0], qy = a.query[i * 3 + 1], qz = a.query[i * 3 + 2];
  for (int sc = s_lo; sc <= s_hi; ++sc) {
    const long long t0 = nn_clamp(a.tstart[sc], a.nt), t1 = nn_clamp(a.tstart[sc + 1], a.nt);
    for (long long base = t0; base < t1; base += kTile) {
      const int m = (int)min((long long)kTile, t1 - base);
      __syncthreads();      // the previous tile has been read
      for (int k = threadIdx.x; k < m; k += kNNThreads) {
        const long long j = base + k;
        tile[k] = Rec{a.target[j * 3 + 0], a.target[j * 3 + 1], a.target[j * 3 + 2], (int)j};
      }
      __syncthreads();
      if (s == sc)
        for (int k = 0; k < m; ++k) {
          const Rec r = tile[k];
          keep.take(nn_d2(qx, qy, qz, r.x, r.y, r.z), r.id);
        }
    }
  }
}

__global__ __launch_bounds__(kNNThreads) void brute_kernel(NNArgs a) {
  __shared__ Rec tile[kTile];
  __shared__ int span[2];
  const long long i = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  NNOne one;
  nn_brute_scan(a, tile, span, i, one);
  if (i < a.nq) a.index[i] = one.bestj, a.dist2[i] = one.best;
}

template <int K>
__global__ __launch_bounds__(kNNThreads) void knn_brute_kernel(NNArgs a) {
  __shared__ Rec tile[kTile];
  __shared__ int span[2];
  const long long i = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  NNList<K> list(a.k);
  nn_brute_scan(a, tile, span, i, list);
  if (i < a.nq) list.write(a, i, a.k);
}

// One thread per target.  A wavefront whose live lanes share one scene reduces its six keys across the lanes first.
__global__ __launch_bounds__(kNNThreads) void box_kernel(NNArgs a) {
  const long long j = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  const int s = j < a.nt ? nn_find_scene(a.tstart, a.nscene, a.nt, j) : -1;
  unsigned key[6] = {~0u, ~0u, ~0u, ~0u, ~0u, ~0u};
  bool in = false;
  if (s >= 0) {
    const float x = a.target[j * 3 + 0], y = a.target[j * 3 + 1], z = a.target[j * 3 + 2];
    if (nn_finite(x) && nn_finite(y) && nn_finite(z)) {
      in = true;
      key[0] = nn_key(x), key[1] = nn_key(y), key[2] = nn_key(z);
      key[3] = ~key[0], key[4] = ~key[1], key[5] = ~key[2];
    }
  }
  const unsigned long long members = __ballot(in);
  if (!members) return;      // (uniform)
  const int s0 = __builtin_amdgcn_readlane(s, __builtin_amdgcn_readfirstlane(__ffsll((long long)members) - 1));
  if (__ballot(in && s != s0) == 0ull) {      // (uniform) one scene: all-ones is the neutral key of the lanes that are out
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      unsigned v = key[k];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o, 64));
      key[k] = v;
    }
    if ((threadIdx.x & 63) == 0)
      for (int k = 0; k < 6; ++k) key_min(a.box + (size_t)s0 * 6 + k, key[k]);
  } else if (in) {
    for (int k = 0; k < 6; ++k) key_min(a.box + (size_t)s * 6 + k, key[k]);
  }
}

// One thread per target: count (scatter = 0) or place (scatter = 1) it in its cell.  A target with a non-finite coordinate is in no cell.
template <int SCATTER>
__global__ __launch_bounds__(kNNThreads) void cell_kernel(NNArgs a) {
  const long long j = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (j >= a.nt) return;
  const int s = nn_find_scene(a.tstart, a.nscene, a.nt, j);
  if (s < 0) return;
  const float x = a.target[j * 3 + 0], y = a.target[j * 3 + 1], z = a.target[j * 3 + 2];
  if (!(nn_finite(x) && nn_finite(y) && nn_finite(z))) return;
  const SceneGrid G = nn_scene_grid(a.box + (size_t)s * 6, a.g);
  if (!G.ok) return;
  unsigned* cell = a.cells + (long long)s * a.g * a.g * a.g + nn_cell_of(G, x, y, z);      // (n[a] <= g: inside the scene's g^3 words)
  const unsigned at = atomicAdd(cell, 1u);
  if (SCATTER && (long long)at < a.nt) a.sorted[at] = Rec{x, y, z, (int)j};
}

__global__ __launch_bounds__(kNNThreads) void grid_query_kernel(NNArgs a) {
  const long long i = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (i < a.nq) nn_query_grid(a, i);
}

template <int K>
__global__ __launch_bounds__(kNNThreads) void knn_grid_kernel(NNArgs a) {
  const long long i = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (i >= a.nq) return;
  NNList<K> list(a.k);
  nn_walk_grid(a, i, list);
  list.write(a, i, a.k);
}

// ---------------------------------------------------------------------------------------------------------------- host
struct NNPlan {
  int method, g;              // resolved: MVD_NN_BRUTE or MVD_NN_GRID; cells per axis
  size_t ncell, chunks;       // nscene * g^3, and the kChunk-word chunks that hold them
  size_t off_box, off_cells, off_blocks, bytes;
};

// false: an argument is out of range (the caller says which)
static bool nn_plan(size_t nt, int nscene, int method, int grid, NNPlan& p) {
  p = NNPlan{};
  if (nscene < 1 || nscene > 65535 || nt > 0x7fffffffull || method < MVD_NN_AUTO || method > MVD_NN_GRID || grid < 0 || grid > kMaxGrid) return false;
  const size_t per = nt / (size_t)nscene;
  p.method = method == MVD_NN_AUTO ? ((long long)per >= kGridMinTargets ? MVD_NN_GRID : MVD_NN_BRUTE) : method;
  if (nt == 0) p.method = MVD_NN_BRUTE;
  if (p.method == MVD_NN_BRUTE) return true;
  int g = grid;
  if (g == 0) {
    g = (int)fminf(fmaxf(floorf(sqrtf((float)per / kGridDivisor) + 0.5f), 1.f), (float)kMaxGrid);
    while (g > 1 && (unsigned long long)nscene * g * g * g > (1ull << 28)) --g;
  }
  if ((unsigned long long)nscene * g * g * g > 0x7fffffffull) return false;
  p.g = g;
  p.ncell = (size_t)nscene * g * g * g;
  p.chunks = (p.ncell + kChunk - 1) / kChunk;
  p.off_box = up16(nt * sizeof(Rec));
  p.off_cells = p.off_box + up16((size_t)nscene * 6 * sizeof(unsigned));
  p.off_blocks = p.off_cells + p.chunks * kChunk * sizeof(unsigned);
  p.bytes = p.off_blocks + up16((p.chunks + 1) * sizeof(unsigned));
  return true;
}

}  // namespace

bool nn_points_layout(size_t nt, int nscene, int method, int grid, NNLayout* out) {
  NNPlan p;
  if (!nn_plan(nt, nscene, method, grid, p)) return false;
  *out = NNLayout{p.method, p.g, p.off_box, p.off_cells, p.bytes};
  return true;
}

extern "C" size_t mvd_nearest_points_scratch(size_t nt, int nscene, int method, int grid) {
  NNPlan p;
  return nn_plan(nt, nscene, method, grid, p) ? p.bytes : 0;
}

namespace {

// The argument checks the two searches share, the plan and the kernel arguments.  Non-zero: refused, with the reason set.
static int nn_prepare(const char* fn, const float* query, const int* query_start, const float* target, const int* target_start, size_t nq,
                      size_t nt, int nscene, int method, int grid, int* index, float* dist2, void* scratch, size_t scratch_bytes, int stages,
                      NNPlan& p, NNArgs& a) {
  MVD_CHECK_ARG(stages >= 1 && stages <= MVD_NN_ALL, "%s: stages=%d outside [1, %d]", fn, stages, MVD_NN_ALL);
  MVD_CHECK_ARG(method >= MVD_NN_AUTO && method <= MVD_NN_GRID, "%s: method=%d (MVD_NN_AUTO, _BRUTE or _GRID)", fn, method);
  MVD_CHECK_ARG(grid >= 0 && grid <= kMaxGrid, "%s: grid=%d outside [0, %d]", fn, grid, kMaxGrid);
  MVD_CHECK_ARG(nscene >= 1 && nscene <= 65535, "%s: nscene=%d outside [1, 65535]", fn, nscene);
  MVD_CHECK_ARG(nq <= 0x7fffffffull && nt <= 0x7fffffffull, "%s: nq=%zu, nt=%zu beyond 2^31 - 1", fn, nq, nt);
  MVD_CHECK_ARG(query_start && target_start, "%s: null query_start or target_start", fn);
  MVD_CHECK_ARG((query && index && dist2) || nq == 0, "%s: null query, index or dist2 with nq=%zu", fn, nq);
  MVD_CHECK_ARG(target || nt == 0, "%s: null target with nt=%zu", fn, nt);
  MVD_CHECK_ARG(nn_plan(nt, nscene, method, grid, p), "%s: nscene * grid^3 cells beyond 2^31 - 1 (nscene=%d, grid=%d)", fn, nscene, grid);
  MVD_CHECK_ARG(p.bytes == 0 || (scratch && scratch_bytes >= p.bytes && ((uintptr_t)scratch & 15) == 0),
                "%s: scratch of %zu bytes (needs %zu, 16-byte aligned)", fn, scratch_bytes, p.bytes);
  char* base = (char*)scratch;
  a = NNArgs{query, target, query_start, target_start, index, dist2, nullptr, nullptr, nullptr, nullptr, (long long)nq, (long long)nt, nscene, p.g, 0};
  if (p.method == MVD_NN_GRID) {
    a.sorted = (Rec*)base;
    a.box = (unsigned*)(base + p.off_box);
    a.cells = (unsigned*)(base + p.off_cells);
    a.blocks = (unsigned*)(base + p.off_blocks);
  }
  return 0;
}

// MVD_NN_BUILD of MVD_NN_GRID: box, count, scan, scatter
static int nn_build(const char* fn, const NNArgs& a, const NNPlan& p, hipStream_t st) {
  hipError_t e = hipMemsetAsync(a.box, 0xff, (size_t)a.nscene * 6 * sizeof(unsigned), st);
  if (e == hipSuccess) e = hipMemsetAsync(a.cells, 0, p.chunks * kChunk * sizeof(unsigned), st);
  MVD_CHECK_ARG(e == hipSuccess, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
  const dim3 per_target(cdiv((long)a.nt, kNNThreads)), threads(kNNThreads);
  hipLaunchKernelGGL(box_kernel, per_target, threads, 0, st, a);
  hipLaunchKernelGGL(cell_kernel<0>, per_target, threads, 0, st, a);
  hipLaunchKernelGGL(chunk_sum_kernel, dim3((unsigned)p.chunks), threads, 0, st, a.cells, a.blocks);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kCompactThreads), 0, st, a.blocks, (unsigned)p.chunks, a.blocks + p.chunks);
  hipLaunchKernelGGL(chunk_scan_kernel, dim3((unsigned)p.chunks), threads, 0, st, a.cells, a.blocks);
  hipLaunchKernelGGL(cell_kernel<1>, per_target, threads, 0, st, a);
  return 0;
}

template <int K>
static void knn_launch(bool grid, const NNArgs& a, hipStream_t st) {
  const dim3 blocks(cdiv((long)a.nq, kNNThreads)), threads(kNNThreads);
  if (grid) hipLaunchKernelGGL(knn_grid_kernel<K>, blocks, threads, 0, st, a);
  else hipLaunchKernelGGL(knn_brute_kernel<K>, blocks, threads, 0, st, a);
}

}  // namespace

extern "C" int mvd_nearest_points_stages(const float* query, const int* query_start, const float* target, const int* target_start, size_t nq,
                                         size_t nt, int nscene, int method, int grid, int* index, float* dist2, void* scratch,
                                         size_t scratch_bytes, int stages, mvd_stream_t stream) {
  const char* fn = stages == MVD_NN_ALL ? "mvd_nearest_points" : "mvd_nearest_points_stages";
  NNPlan p;
  NNArgs a;
  if (const int rc = nn_prepare(fn, query, query_start, target, target_start, nq, nt, nscene, method, grid, index, dist2, scratch, scratch_bytes,
                                stages, p, a))
    return rc;
  const hipStream_t st = (hipStream_t)stream;
  if (p.method == MVD_NN_GRID) {
    if (stages & MVD_NN_BUILD)
      if (const int rc = nn_build(fn, a, p, st)) return rc;
    if ((stages & MVD_NN_QUERY) && nq > 0) hipLaunchKernelGGL(grid_query_kernel, dim3(cdiv((long)nq, kNNThreads)), dim3(kNNThreads), 0, st, a);
  } else if ((stages & MVD_NN_QUERY) && nq > 0) {
    hipLaunchKernelGGL(brute_kernel, dim3(cdiv((long)nq, kNNThreads)), dim3(kNNThreads), 0, st, a);
  }
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int mvd_knn_points_stages(const float* query, const int* query_start, const float* target, const int* target_start, size_t nq,
                                     size_t nt, int nscene, int k, int method, int grid, int* index, float* dist2, void* scratch,
                                     size_t scratch_bytes, int stages, mvd_stream_t stream) {
  const char* fn = stages == MVD_NN_ALL ? "mvd_knn_points" : "mvd_knn_points_stages";
  MVD_CHECK_ARG(k >= 1 && k <= MVD_KNN_MAX_K, "%s: k=%d outside [1, %d]", fn, k, MVD_KNN_MAX_K);
  const uintptr_t low = (uintptr_t)query | (uintptr_t)query_start | (uintptr_t)target | (uintptr_t)target_start | (uintptr_t)index | (uintptr_t)dist2;
  MVD_CHECK_ARG((low & 3) == 0, "%s: a pointer that is not 4-byte aligned", fn);
  NNPlan p;
  NNArgs a;
  if (const int rc = nn_prepare(fn, query, query_start, target, target_start, nq, nt, nscene, method, grid, index, dist2, scratch, scratch_bytes,
                                stages, p, a))
    return rc;
  a.k = k;
  const hipStream_t st = (hipStream_t)stream;
  const bool grid_method = p.method == MVD_NN_GRID;
  if (grid_method && (stages & MVD_NN_BUILD))
    if (const int rc = nn_build(fn, a, p, st)) return rc;
  if ((stages & MVD_NN_QUERY) && nq > 0) {
    if (k == 1) knn_launch<1>(grid_method, a, st);
    else if (k == 2) knn_launch<2>(grid_method, a, st);
    else if (k <= 4) knn_launch<4>(grid_method, a, st);
    else if (k <= 8) knn_launch<8>(grid_method, a, st);
    else if (k <= 16) knn_launch<16>(grid_method, a, st);
    else knn_launch<32>(grid_method, a, st);
  }
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int mvd_knn_points(const float* query, const int* query_start, const float* target, const int* target_start, size_t nq, size_t nt,
                              int nscene, int k, int method, int grid, int* index, float* dist2, void* scratch, size_t scratch_bytes,
                              mvd_stream_t stream) {
  return mvd_knn_points_stages(query, query_start, target, target_start, nq, nt, nscene, k, method, grid, index, dist2, scratch, scratch_bytes,
                               MVD_NN_ALL, stream);
}

extern "C" int mvd_nearest_points(const float* query, const int* query_start, const float* target, const int* target_start, size_t nq,
                                  size_t nt, int nscene, int method, int grid, int* index, float* dist2, void* scratch, size_t scratch_bytes,
                                  mvd_stream_t stream) {
  return mvd_nearest_points_stages(query, query_start, target, target_start, nq, nt, nscene, method, grid, index, dist2, scratch, scratch_bytes,
                                   MVD_NN_ALL, stream);
}
