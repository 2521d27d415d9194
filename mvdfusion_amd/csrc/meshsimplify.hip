// Mesh simplification on the device: vertex clustering (Rossignac-Borrel) with Lindstrom's quadric placement (include/mvd_hip.h: "Mesh
// simplification" has every rule in full).
//
// COUNT: box per scene (integer atomicMin on the order-preserving keys of nn_grid.hpp, in LDS first; the upper corner as the minimum of
// the complemented key) -> occupied cells flagged by plain stores of one value into the dense table -> the exclusive scan of nn_grid.hpp ->
// vertex_cluster, cluster_start -> members per cluster (an integer atomic per member) -> the same scan: the begins of the cluster ->
// member lists, which stay in the scratch for the emit call.
// EMIT: fill (an integer atomic hands out the slot: arrival order) -> rank (every member counts the smaller ids of its own list and
// stores itself at that position: O(list) per thread over all members, no thread is quadratic, and the ORDERED list does not depend on
// the arrival order) -> per vertex the quadric of its faces (fp64, incidence-list order) -> per cluster the sums over its ascending
// members, the 3 x 3 Jacobi of jacobi3.hpp, the placement -> per face the cluster ids and `keep`.
//   Every kernel of the emit call first compares its `nc` with the total the count call left in the scratch and returns when they
//   differ, so a call with another nc writes nothing, neither outputs nor scratch.
// DEDUPE: one thread per kept face walks the incidence list (of the mapped faces) of its smallest id; lists ascend by face, so the walk
// ends at the face's own row.
// fp64 throughout, compiled without contraction; integer atomics only.  Every index read back from a table is clamped or range-checked
// before it addresses anything.
#include "jacobi3.hpp"
#include "mesh_common.hpp"

namespace {

constexpr double kMSRankRatio = MVD_SIMPLIFY_RANK_RATIO;
constexpr double kMSSlack = 1.0 / (double)MVD_SIMPLIFY_BOX_SLACK_DIV;

__device__ __forceinline__ bool ms_finite64(double v) { return fabs(v) < (double)INFINITY; }

// A scene's clustering grid from its box of keys: lower corner, cell side and cells per axis, all from the stated fp64 expressions.
struct MSGrid {
  double lo[3], h;
  int n[3];
};
__device__ __forceinline__ MSGrid ms_grid(const unsigned* box, int cells) {
  MSGrid G;
  double ext[3], big = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    G.lo[a] = (double)nn_unkey(box[a]);
    ext[a] = (double)nn_unkey(~box[3 + a]) - G.lo[a];
    big = ext[a] > big ? ext[a] : big;      // (a NaN -- the box of a scene without a member -- leaves 0)
  }
  G.h = big / (double)cells;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double na = 1.0;
    if (G.h > 0.0) na = floor(ext[a] / G.h) + 1.0;
    na = na >= 1.0 ? na : 1.0;                              // clamped BEFORE the conversion, a NaN to 1
    G.n[a] = (int)(na > (double)cells ? (double)cells : na);
  }
  return G;
}
__device__ __forceinline__ int ms_cell(const MSGrid& G, int a, float x) {
  if (!(G.h > 0.0)) return 0;
  double u = floor(((double)x - G.lo[a]) / G.h);
  u = u >= 0.0 ? u : 0.0;                                   // (a NaN to 0)
  const double top = (double)(G.n[a] - 1);
  return (int)(u > top ? top : u);
}

struct MSVerts {
  const float* vertices;
  const int *vstart, *inc_start;
  long long nv, nf;
  int nscene, cells;
};

// Vertex v is a MEMBER: it lies in a scene, its three coordinates are finite and its incidence list is not empty.  -> its scene, x.
__device__ __forceinline__ int ms_member(const MSVerts& m, long long v, float* x) {
  const int s = nn_find_scene(m.vstart, m.nscene, m.nv, v);
  if (s < 0) return -1;
  long long b, e;
  mt_list(m.inc_start, v, m.nf, b, e);
  if (e <= b) return -1;
  x[0] = m.vertices[v * 3 + 0], x[1] = m.vertices[v * 3 + 1], x[2] = m.vertices[v * 3 + 2];
  return (nn_finite(x[0]) && nn_finite(x[1]) && nn_finite(x[2])) ? s : -1;
}

// the member's word in the dense table: scene s, linear cell id (iz n_y + iy) n_x + ix
__device__ __forceinline__ long long ms_word(const MSVerts& m, const unsigned* box, int s, const float* x, int* cell) {
  const MSGrid G = ms_grid(box + (size_t)s * 6, m.cells);
  cell[0] = ms_cell(G, 0, x[0]), cell[1] = ms_cell(G, 1, x[1]), cell[2] = ms_cell(G, 2, x[2]);
  const long long c3 = (long long)m.cells * m.cells * m.cells;
  return (long long)s * c3 + ((long long)cell[2] * G.n[1] + cell[1]) * G.n[0] + cell[0];
}

// ---------------------------------------------------------------------------------------------------------------- count
__global__ __launch_bounds__(kNNThreads) void ms_fill_kernel(unsigned* __restrict__ words, long long n, unsigned value) {
  const long long i = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (i < n) words[i] = value;
}

// The keys of a workgroup whose rows lie in ONE scene (starts are non-decreasing, so the ends decide) are gathered in LDS first and
// reach the scene's box by six atomics; a workgroup across scenes goes to the boxes directly.  A minimum either way: the same box.
__global__ __launch_bounds__(kNNThreads) void ms_bounds_kernel(MSVerts m, unsigned* box) {
  __shared__ unsigned lds[6];
  if (threadIdx.x < 6) lds[threadIdx.x] = 0xffffffffu;
  __syncthreads();
  const long long first = (long long)blockIdx.x * kNNThreads, v = first + threadIdx.x;
  const long long last = first + kNNThreads - 1 < m.nv ? first + kNNThreads - 1 : m.nv - 1;
  const int s0 = nn_find_scene(m.vstart, m.nscene, m.nv, first), s1 = nn_find_scene(m.vstart, m.nscene, m.nv, last);
  const bool uniform = s0 >= 0 && s0 == s1;
  if (v < m.nv) {
    float x[3];
    const int s = ms_member(m, v, x);
    if (s >= 0) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const unsigned k = nn_key(x[a]);
        if (uniform) {
          atomicMin(lds + a, k);
          atomicMin(lds + 3 + a, ~k);
        } else {
          key_min(box + (size_t)s * 6 + a, k);
          key_min(box + (size_t)s * 6 + 3 + a, ~k);
        }
      }
    }
  }
  __syncthreads();
  if (uniform && threadIdx.x < 6 && lds[threadIdx.x] != 0xffffffffu) key_min(box + (size_t)s0 * 6 + threadIdx.x, lds[threadIdx.x]);
}

__global__ __launch_bounds__(kNNThreads) void ms_flag_kernel(MSVerts m, const unsigned* __restrict__ box, unsigned* table) {
  const long long v = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (v >= m.nv) return;
  float x[3];
  int cell[3];
  const int s = ms_member(m, v, x);
  if (s >= 0) table[ms_word(m, box, s, x, cell)] = 1u;      // (plain stores of the same value)
}

__global__ __launch_bounds__(kNNThreads) void ms_assign_kernel(MSVerts m, const unsigned* __restrict__ box, const unsigned* __restrict__ rank,
                                                              int* __restrict__ vertex_cluster, unsigned* sizes) {
  const long long v = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (v >= m.nv) return;
  float x[3];
  int cell[3];
  const int s = ms_member(m, v, x);
  long long c = -1;
  if (s >= 0) {
    c = rank[ms_word(m, box, s, x, cell)];
    if (c >= m.nv) c = -1;                                  // (never: a cluster has a member)
  }
  vertex_cluster[v] = (int)c;
  if (c >= 0) atomicAdd(sizes + c, 1u);
}

// cluster_start[s] = rank[s cells^3] for s = 0 .. nscene; the total also to *nc_word
__global__ __launch_bounds__(kNNThreads) void ms_starts_kernel(const unsigned* __restrict__ rank, long long c3, int nscene, int* __restrict__ cluster_start,
                                                              unsigned* __restrict__ nc_word) {
  const int s = blockIdx.x * kNNThreads + threadIdx.x;
  if (s > nscene) return;
  const unsigned r = rank[(long long)s * c3];
  cluster_start[s] = (int)r;
  if (s == nscene) *nc_word = r;
}

// ---------------------------------------------------------------------------------------------------------------- emit
struct MSLists {
  const unsigned *nc_word, *mstart;      // what the count call left: the cluster count, the begins of the member lists (nc + 1 words)
  long long nc, nv;
};
__device__ __forceinline__ bool ms_same_count(const MSLists& l) { return (long long)*l.nc_word == l.nc; }
__device__ __forceinline__ void ms_members(const MSLists& l, long long c, long long& b, long long& e) {
  b = nn_clamp(l.mstart[c], l.nv), e = nn_clamp(l.mstart[c + 1], l.nv);
  if (e < b) e = b;
}

__global__ __launch_bounds__(kNNThreads) void ms_cursor_kernel(MSLists l, unsigned* __restrict__ cursor) {
  const long long c = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (!ms_same_count(l) || c >= l.nc) return;
  cursor[c] = l.mstart[c];
}

__global__ __launch_bounds__(kNNThreads) void ms_list_fill_kernel(MSLists l, const int* __restrict__ vertex_cluster, unsigned* cursor,
                                                                 int* __restrict__ unsorted) {
  const long long v = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (!ms_same_count(l) || v >= l.nv) return;
  const long long c = vertex_cluster[v];
  if (c < 0 || c >= l.nc) return;
  const long long at = atomicAdd(cursor + c, 1u);
  if (at < l.nv) unsorted[at] = (int)v;
}

// A member's position in its ordered list is the number of smaller ids in the list: O(list) reads, one store.
__global__ __launch_bounds__(kNNThreads) void ms_list_rank_kernel(MSLists l, const int* __restrict__ vertex_cluster, const int* __restrict__ unsorted,
                                                                 int* __restrict__ members) {
  const long long v = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (!ms_same_count(l) || v >= l.nv) return;
  const long long c = vertex_cluster[v];
  if (c < 0 || c >= l.nc) return;
  long long b, e, below = 0;
  ms_members(l, c, b, e);
  for (long long k = b; k < e; ++k) below += unsorted[k] < v ? 1 : 0;
  if (b + below < e) members[b + below] = (int)v;
}

// Per member vertex: A_v = sum w u u^T (xx xy xz yy yz zz) and g_v = sum w (u . a) u over the faces of its list that name only finite
// vertices, in list order -> quad[v * 9 ..].
__global__ __launch_bounds__(kNNThreads) void ms_vertex_quadric_kernel(MSLists l, const float* __restrict__ vertices, const int* __restrict__ faces,
                                                                      const int* __restrict__ inc_start, const int* __restrict__ inc,
                                                                      const int* __restrict__ vertex_cluster, long long nf, double* __restrict__ quad) {
  const long long v = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (!ms_same_count(l) || v >= l.nv) return;
  if (vertex_cluster[v] < 0) return;
  long long b, e;
  mt_list(inc_start, v, nf, b, e);
  double q[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long k = b; k < e; ++k) {
    long long g;
    int c, gid[3];
    if (!mt_entry(inc, faces, k, v, l.nv, nf, g, c, gid)) continue;
    double T[9];
    bool finite = true;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        const float t = vertices[(long long)gid[j] * 3 + x];
        finite = finite && nn_finite(t);
        T[j * 3 + x] = (double)t;
      }
    if (!finite) continue;
    const double ab[3] = {T[3] - T[0], T[4] - T[1], T[5] - T[2]}, ac[3] = {T[6] - T[0], T[7] - T[1], T[8] - T[2]};
    const double n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
    const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    if (!(len > 0.0) || !ms_finite64(len)) continue;
    const double u[3] = {n[0] / len, n[1] / len, n[2] / len}, w = len / 2.0;
    const double wu[3] = {w * u[0], w * u[1], w * u[2]};
    const double d = (u[0] * T[0] + u[1] * T[1]) + u[2] * T[2];
    q[0] += wu[0] * u[0], q[1] += wu[0] * u[1], q[2] += wu[0] * u[2];
    q[3] += wu[1] * u[1], q[4] += wu[1] * u[2], q[5] += wu[2] * u[2];
    q[6] += wu[0] * d, q[7] += wu[1] * d, q[8] += wu[2] * d;
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) quad[v * 9 + j] = q[j];
}

struct MSOut {
  float *vertices, *rgb;
  int *size, *rank, *placed;
};

__global__ __launch_bounds__(kNNThreads) void ms_cluster_kernel(MSLists l, MSVerts m, const float* __restrict__ rgb, const unsigned* __restrict__ box,
                                                               const int* __restrict__ members, const double* __restrict__ quad, int placement,
                                                               MSOut out) {
  const long long c = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (!ms_same_count(l) || c >= l.nc) return;
  long long b, e;
  ms_members(l, c, b, e);
  double sx[3] = {0.0, 0.0, 0.0}, sc[3] = {0.0, 0.0, 0.0}, q[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  long long count = 0, first = -1;
  for (long long k = b; k < e; ++k) {
    const long long v = members[k];
    if (v < 0 || v >= l.nv) continue;
    if (first < 0) first = v;
    ++count;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      sx[a] += (double)m.vertices[v * 3 + a];
      if (rgb) sc[a] += (double)rgb[v * 3 + a];
    }
    if (placement == MVD_SIMPLIFY_QUADRIC) {
#pragma unroll
      for (int j = 0; j < 9; ++j) q[j] += quad[v * 9 + j];
    }
  }
  const double cnt = (double)(count > 0 ? count : 1);
  const double mean[3] = {sx[0] / cnt, sx[1] / cnt, sx[2] / cnt};
  double x[3] = {mean[0], mean[1], mean[2]};
  int rank = 0, placed = MVD_SIMPLIFY_PLACED_MEAN;
  if (placement == MVD_SIMPLIFY_QUADRIC) {
    placed = MVD_SIMPLIFY_PLACED_FALLBACK;
    const double bv[3] = {((q[0] * mean[0] + q[1] * mean[1]) + q[2] * mean[2]) - q[6], ((q[1] * mean[0] + q[3] * mean[1]) + q[4] * mean[2]) - q[7],
                          ((q[2] * mean[0] + q[4] * mean[1]) + q[5] * mean[2]) - q[8]};
    double A[3][3] = {{q[0], q[1], q[2]}, {q[1], q[3], q[4]}, {q[2], q[4], q[5]}}, V[3][3];
    pn_jacobi3(A, V);
    const double lam[3] = {A[0][0], A[1][1], A[2][2]};
    double top = lam[0] > lam[1] ? lam[0] : lam[1];
    top = top > lam[2] ? top : lam[2];
    double y[3] = {mean[0], mean[1], mean[2]};
    if (top > 0.0 && ms_finite64(top)) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (lam[i] > kMSRankRatio * top) {
          ++rank;
          const double t = ((V[0][i] * bv[0] + V[1][i] * bv[1]) + V[2][i] * bv[2]) / lam[i];
#pragma unroll
          for (int a = 0; a < 3; ++a) y[a] = y[a] - t * V[a][i];
        }
    }
    if (rank > 0 && first >= 0 && ms_finite64(y[0]) && ms_finite64(y[1]) && ms_finite64(y[2])) {
      // the cluster's cell, from its first member by the expressions that numbered it
      const int s = nn_find_scene(m.vstart, m.nscene, m.nv, first);
      const MSGrid G = ms_grid(box + (size_t)(s < 0 ? 0 : s) * 6, m.cells);
      const double slack = G.h * kMSSlack;
      bool inside = s >= 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int ia = ms_cell(G, a, m.vertices[first * 3 + a]);
        const double lo = (G.lo[a] + (double)ia * G.h) - slack, hi = (G.lo[a] + (double)(ia + 1) * G.h) + slack;
        inside = inside && y[a] >= lo && y[a] <= hi;
      }
      if (inside) x[0] = y[0], x[1] = y[1], x[2] = y[2], placed = MVD_SIMPLIFY_PLACED_QUADRIC;
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    out.vertices[c * 3 + a] = (float)x[a];
    if (rgb) out.rgb[c * 3 + a] = (float)(sc[a] / cnt);
  }
  out.size[c] = (int)count, out.rank[c] = rank, out.placed[c] = placed;
}

__global__ __launch_bounds__(kNNThreads) void ms_faces_kernel(MSLists l, MTMesh m, const int* __restrict__ vertex_cluster, int* __restrict__ mapped,
                                                             uint8_t* __restrict__ keep) {
  const long long f = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (!ms_same_count(l) || f >= m.nf) return;
  int id[3], s, c[3] = {-1, -1, -1};
  const int cls = mt_face(m, f, id, s);
  if (cls != kInvalid) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      c[k] = vertex_cluster[id[k]];
      if (c[k] < 0 || c[k] >= l.nc) c[k] = -1;
    }
  }
  mapped[f * 3 + 0] = c[0], mapped[f * 3 + 1] = c[1], mapped[f * 3 + 2] = c[2];
  keep[f] = (cls == kRegular && c[0] >= 0 && c[1] >= 0 && c[2] >= 0 && c[0] != c[1] && c[1] != c[2] && c[0] != c[2]) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------- dedupe
__device__ __forceinline__ void ms_sort3(const int* id, int* o) {
  const int lo = nn_lo(id[0], nn_lo(id[1], id[2])), hi = nn_hi(id[0], nn_hi(id[1], id[2]));
  o[0] = lo, o[2] = hi, o[1] = (int)(((long long)id[0] + id[1] + id[2]) - lo - hi);
}

__global__ __launch_bounds__(kNNThreads) void ms_dedupe_kernel(const int* __restrict__ mapped, const uint8_t* __restrict__ keep, const int* __restrict__ inc_start,
                                                              const int* __restrict__ inc, long long nc, long long nf, uint8_t* __restrict__ keep_out) {
  const long long f = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (f >= nf) return;
  uint8_t mine = keep[f] ? 1 : 0;
  if (mine) {
    const int id[3] = {mapped[f * 3 + 0], mapped[f * 3 + 1], mapped[f * 3 + 2]};
    int a[3];
    ms_sort3(id, a);
    if (a[0] >= 0 && a[0] < nc) {
      long long b, e;
      mt_list(inc_start, a[0], nf, b, e);
      for (long long k = b; k < e; ++k) {
        const long long ent = inc[k];
        if (ent < 0 || ent >= 3 * nf) continue;
        const long long g = ent / 3;
        if (g >= f) break;                                  // lists ascend by face: only lower rows can win
        if (!keep[g]) continue;
        const int gid[3] = {mapped[g * 3 + 0], mapped[g * 3 + 1], mapped[g * 3 + 2]};
        int o[3];
        ms_sort3(gid, o);
        if (o[0] == a[0] && o[1] == a[1] && o[2] == a[2]) {
          mine = 0;
          break;
        }
      }
    }
  }
  keep_out[f] = mine;
}

// ---------------------------------------------------------------------------------------------------------------- host
constexpr size_t kMSMaxTable = (size_t)1 << 28;

struct MSPlan {
  size_t table, off_mstart, off_work, off_cursor, off_unsorted, off_members, off_quad, bytes;      // box and the nc word at 0
};
static bool ms_sizes_ok(size_t nv, size_t nf, int nscene, int cells) {
  return mt_sizes_ok(nv, nf) && nscene >= 1 && nscene <= 65535 && cells >= 1 && cells <= MVD_SIMPLIFY_MAX_CELLS &&
         (size_t)nscene * cells * cells * cells <= kMSMaxTable;
}
static MSPlan ms_plan(size_t nv, int nscene, int cells) {
  MSPlan p;
  p.table = (size_t)nscene * cells * cells * cells;
  p.off_mstart = up16(((size_t)nscene * 6 + 1) * sizeof(unsigned));
  p.off_work = p.off_mstart + mt_scan_bytes(nv);
  // the count call's table and the emit call's lists and quadrics share what follows
  p.off_cursor = p.off_work;
  p.off_unsorted = p.off_cursor + up16(nv * sizeof(unsigned));
  p.off_members = p.off_unsorted + up16(nv * sizeof(int));
  p.off_quad = p.off_members + up16(nv * sizeof(int));
  const size_t emit_end = p.off_quad + up16(nv * 9 * sizeof(double)), count_end = p.off_work + mt_scan_bytes(p.table);
  p.bytes = emit_end > count_end ? emit_end : count_end;
  return p;
}

}  // namespace

extern "C" size_t mvd_mesh_cluster_scratch(size_t nv, size_t nf, int nscene, int cells) {
  return ms_sizes_ok(nv, nf, nscene, cells) ? ms_plan(nv, nscene, cells).bytes : 0;
}

extern "C" int mvd_mesh_cluster_count(const float* vertices, const int* vertex_start, const int* inc_start, size_t nv, size_t nf, int nscene, int cells,
                                      int* vertex_cluster, int* cluster_start, void* scratch, size_t scratch_bytes, mvd_stream_t stream) {
  const char* fn = "mvd_mesh_cluster_count";
  MVD_CHECK_ARG(nscene >= 1 && nscene <= 65535, "%s: nscene=%d outside [1, 65535]", fn, nscene);
  MVD_CHECK_ARG(cells >= 1 && cells <= MVD_SIMPLIFY_MAX_CELLS, "%s: cells=%d outside [1, %d]", fn, cells, MVD_SIMPLIFY_MAX_CELLS);
  MVD_CHECK_ARG(mt_sizes_ok(nv, nf), "%s: nv=%zu beyond 2^31 - 1 - %d or nf=%zu beyond (2^31 - 1) / 3", fn, nv, kChunk, nf);
  MVD_CHECK_ARG((size_t)nscene * cells * cells * cells <= kMSMaxTable, "%s: nscene * cells^3 = %d * %d^3 beyond 2^28", fn, nscene, cells);
  MVD_CHECK_ARG(vertex_start && inc_start && cluster_start, "%s: null vertex_start, inc_start or cluster_start", fn);
  MVD_CHECK_ARG((vertices && vertex_cluster) || nv == 0, "%s: null vertices or vertex_cluster with nv=%zu", fn, nv);
  MVD_CHECK_ARG((((uintptr_t)vertices | (uintptr_t)vertex_start | (uintptr_t)inc_start | (uintptr_t)vertex_cluster | (uintptr_t)cluster_start) & 3) == 0,
                "%s: a pointer that is not 4-byte aligned", fn);
  const MSPlan p = ms_plan(nv, nscene, cells);
  MT_TRY(mt_check_scratch(fn, scratch, scratch_bytes, p.bytes));
  const hipStream_t st = (hipStream_t)stream;
  const MSVerts m{vertices, vertex_start, inc_start, (long long)nv, (long long)nf, nscene, cells};
  char* base = (char*)scratch;
  unsigned *box = (unsigned*)base, *nc_word = box + (size_t)nscene * 6, *sizes = (unsigned*)(base + p.off_mstart), *table = (unsigned*)(base + p.off_work);
  hipError_t e = hipMemsetAsync(sizes, 0, mt_chunks(nv) * kChunk * sizeof(unsigned), st);
  if (e == hipSuccess) e = hipMemsetAsync(table, 0, mt_chunks(p.table) * kChunk * sizeof(unsigned), st);
  MVD_CHECK_ARG(e == hipSuccess, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
  const dim3 threads(kNNThreads);
  hipLaunchKernelGGL(ms_fill_kernel, mt_grid((size_t)nscene * 6), threads, 0, st, box, (long long)nscene * 6, 0xffffffffu);
  if (nv > 0) hipLaunchKernelGGL(ms_bounds_kernel, mt_grid(nv), threads, 0, st, m, box);
  if (nv > 0) hipLaunchKernelGGL(ms_flag_kernel, mt_grid(nv), threads, 0, st, m, box, table);
  mt_scan(table, p.table, st);
  if (nv > 0) hipLaunchKernelGGL(ms_assign_kernel, mt_grid(nv), threads, 0, st, m, box, table, vertex_cluster, sizes);
  hipLaunchKernelGGL(ms_starts_kernel, mt_grid((size_t)nscene + 1), threads, 0, st, table, (long long)cells * cells * cells, nscene, cluster_start, nc_word);
  mt_scan(sizes, nv, st);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int mvd_mesh_cluster_emit(const float* vertices, const float* rgb, const int* faces, const int* vertex_start, const int* face_start,
                                     const int* inc_start, const int* inc, const int* vertex_cluster, size_t nv, size_t nf, int nscene, int cells,
                                     int placement, size_t nc, float* out_vertices, float* out_rgb, int* size, int* rank, int* placed,
                                     int* mapped_faces, uint8_t* keep, void* scratch, size_t scratch_bytes, mvd_stream_t stream) {
  const char* fn = "mvd_mesh_cluster_emit";
  MT_TRY(mt_check_mesh(fn, faces, vertex_start, face_start, nv, nf, nscene));
  MVD_CHECK_ARG(cells >= 1 && cells <= MVD_SIMPLIFY_MAX_CELLS, "%s: cells=%d outside [1, %d]", fn, cells, MVD_SIMPLIFY_MAX_CELLS);
  MVD_CHECK_ARG((size_t)nscene * cells * cells * cells <= kMSMaxTable, "%s: nscene * cells^3 = %d * %d^3 beyond 2^28", fn, nscene, cells);
  MVD_CHECK_ARG(placement == MVD_SIMPLIFY_MEAN || placement == MVD_SIMPLIFY_QUADRIC, "%s: placement=%d is neither MVD_SIMPLIFY_MEAN nor _QUADRIC", fn,
                placement);
  MVD_CHECK_ARG(nc <= nv, "%s: nc=%zu > nv=%zu", fn, nc, nv);
  MT_TRY(mt_check_table(fn, inc_start, inc, nf));
  MVD_CHECK_ARG((vertices && vertex_cluster) || nv == 0, "%s: null vertices or vertex_cluster with nv=%zu", fn, nv);
  MVD_CHECK_ARG((out_vertices && size && rank && placed && (out_rgb || !rgb)) || nc == 0, "%s: null cluster output with nc=%zu", fn, nc);
  MVD_CHECK_ARG((mapped_faces && keep) || nf == 0, "%s: null mapped_faces or keep with nf=%zu", fn, nf);
  const uintptr_t low = (uintptr_t)vertices | (uintptr_t)rgb | (uintptr_t)vertex_cluster | (uintptr_t)out_vertices | (uintptr_t)out_rgb | (uintptr_t)size |
                        (uintptr_t)rank | (uintptr_t)placed | (uintptr_t)mapped_faces;
  MVD_CHECK_ARG((low & 3) == 0, "%s: a pointer that is not 4-byte aligned", fn);
  const MSPlan p = ms_plan(nv, nscene, cells);
  MT_TRY(mt_check_scratch(fn, scratch, scratch_bytes, p.bytes));
  const hipStream_t st = (hipStream_t)stream;
  char* base = (char*)scratch;
  const unsigned* box = (const unsigned*)base;
  const MSLists l{box + (size_t)nscene * 6, (const unsigned*)(base + p.off_mstart), (long long)nc, (long long)nv};
  const MSVerts mv{vertices, vertex_start, inc_start, (long long)nv, (long long)nf, nscene, cells};
  const MTMesh m{faces, vertex_start, face_start, (long long)nv, (long long)nf, nscene};
  unsigned* cursor = (unsigned*)(base + p.off_cursor);
  int *unsorted = (int*)(base + p.off_unsorted), *members = (int*)(base + p.off_members);
  double* quad = (double*)(base + p.off_quad);
  const MSOut out{out_vertices, out_rgb, size, rank, placed};
  const dim3 threads(kNNThreads);
  if (nc > 0 && nv > 0) {
    hipLaunchKernelGGL(ms_cursor_kernel, mt_grid(nc), threads, 0, st, l, cursor);
    hipLaunchKernelGGL(ms_list_fill_kernel, mt_grid(nv), threads, 0, st, l, vertex_cluster, cursor, unsorted);
    hipLaunchKernelGGL(ms_list_rank_kernel, mt_grid(nv), threads, 0, st, l, vertex_cluster, unsorted, members);
    if (placement == MVD_SIMPLIFY_QUADRIC)
      hipLaunchKernelGGL(ms_vertex_quadric_kernel, mt_grid(nv), threads, 0, st, l, vertices, faces, inc_start, inc, vertex_cluster, (long long)nf, quad);
    hipLaunchKernelGGL(ms_cluster_kernel, mt_grid(nc), threads, 0, st, l, mv, rgb, box, members, quad, placement, out);
  }
  if (nf > 0) hipLaunchKernelGGL(ms_faces_kernel, mt_grid(nf), threads, 0, st, l, m, vertex_cluster, mapped_faces, keep);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int mvd_mesh_cluster_dedupe(const int* mapped_faces, const uint8_t* keep, const int* inc_start, const int* inc, size_t nc, size_t nf,
                                       uint8_t* keep_out, mvd_stream_t stream) {
  const char* fn = "mvd_mesh_cluster_dedupe";
  MVD_CHECK_ARG(mt_sizes_ok(nc, nf), "%s: nc=%zu beyond 2^31 - 1 - %d or nf=%zu beyond (2^31 - 1) / 3", fn, nc, kChunk, nf);
  MT_TRY(mt_check_table(fn, inc_start, inc, nf));
  MVD_CHECK_ARG((mapped_faces && keep && keep_out) || nf == 0, "%s: null mapped_faces, keep or keep_out with nf=%zu", fn, nf);
  MVD_CHECK_ARG(keep != keep_out || nf == 0, "%s: keep and keep_out must be two buffers", fn);
  MVD_CHECK_ARG(((uintptr_t)mapped_faces & 3) == 0, "%s: a pointer that is not 4-byte aligned", fn);
  if (nf > 0)
    hipLaunchKernelGGL(ms_dedupe_kernel, mt_grid(nf), dim3(kNNThreads), 0, (hipStream_t)stream, mapped_faces, keep, inc_start, inc, (long long)nc,
                       (long long)nf, keep_out);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}
