// Mesh topology on the device (include/mvd_hip.h: "Mesh topology" has every rule in full): the vertex -> face incidence table, connected
// components, the topology report, the face filter, area-weighted vertex normals and Taubin smoothing.
//
// FACE CLASSES (mt_face): invalid -- an id outside the vertex range of the face's own scene, or a face of no scene; repeated -- two
// equal ids; regular -- the rest.  One function, so every kernel below classifies a face by the same comparisons.
// INCIDENCE: count (one thread per face, atomicAdd per corner) -> the two-level exclusive scan of nn_grid.hpp around scan_kernel ->
// copy of the begins to inc_start -> fill (atomicAdd hands out the slots: arrival order) -> sort (one thread per vertex, insertion sort
// of its list in global memory: the list has no bound but the face count, and the SORTED list does not depend on the arrival order).
// COMPONENTS: lock-free union-find.  parent[v] = v at the start; a hook is atomicCAS(parent + hi, hi, lo) with lo < hi, the path
// halving atomicMin(parent + v, grandparent): parent[v] <= v always and a word only ever decreases.
//   BOUNDS.  mt_find walks strictly downward in vertex ids, so it ends within nv steps whatever the memory holds (what it reads is
//   clamped to [0, v]).  mt_union retries only after a failed CAS, that is after ANOTHER thread lowered parent[hi]; it goes on from that
//   lower value, so max(root a, root b) strictly decreases from one attempt to the next: at most nv attempts.  No thread waits for
//   another one's action, there is no persistent kernel and no host loop.  Both loops also carry the explicit cap nv.
//   The root of a tree is its smallest id (a parent is smaller than its child), and after the hook kernel the trees are the components:
//   the label -- the smallest vertex id of the component -- is unique, so no race can change it.
// REPORT: one thread per face walks, per edge, the incidence list of the endpoint with the shorter list; the lowest (face, edge) user
// owns the edge and adds to the totals.  Totals are integer atomics (LDS first where a workgroup lies in one scene); the vertex bits
// are atomicOr on 32-bit words of the scratch, narrowed to uint8 by the kernel that owns the vertex.  O(valence^2) per vertex.
// FILTER: flag (plain stores of the same value) -> two scans -> starts; the host reads them; emit.
// NORMALS, SMOOTHING: one thread per vertex sums over its list in list order in fp64; no atomics, compiled without contraction.
// Every index read back from a table (inc_start, inc, a rank) is clamped or range-checked before it addresses anything, so a table
// the caller did not build with these entries reads nothing out of bounds.
#include "mesh_common.hpp"

namespace {

constexpr int kMTTotals = MVD_TOPO_TOTALS;
enum { kTUsed = 0, kTUnref, kTRegular, kTRepeated, kTInvalid, kTEdges, kTBoundary, kTNonManifold, kTMisoriented, kTComponents, kTEuler };

// ---------------------------------------------------------------------------------------------------------------- incidence
__global__ __launch_bounds__(kNNThreads) void mt_inc_count_kernel(MTMesh m, unsigned* __restrict__ counts) {
  const long long f = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (f >= m.nf) return;
  int id[3], s;
  if (mt_face(m, f, id, s) != kRegular) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) atomicAdd(counts + id[k], 1u);
}

// words[0 .. n] (n + 1 of them) -> out as int32
__global__ __launch_bounds__(kNNThreads) void mt_copy_kernel(const unsigned* __restrict__ words, int* __restrict__ out, long long n1) {
  const long long i = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (i < n1) out[i] = (int)words[i];
}

__global__ __launch_bounds__(kNNThreads) void mt_inc_fill_kernel(MTMesh m, unsigned* __restrict__ cursor, int* __restrict__ inc) {
  const long long f = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (f >= m.nf) return;
  int id[3], s;
  if (mt_face(m, f, id, s) != kRegular) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const long long at = atomicAdd(cursor + id[k], 1u);
    if (at < 3 * m.nf) inc[at] = (int)(f * 3 + k);      // (always: the scan counted exactly these)
  }
}

// One thread per vertex: its list into ascending order.  Insertion sort in place: at most (e - b)^2 / 2 moves, e - b <= 3 nf.
__global__ __launch_bounds__(kNNThreads) void mt_inc_sort_kernel(const int* __restrict__ inc_start, int* __restrict__ inc, long long nv, long long nf) {
  const long long v = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (v >= nv) return;
  long long b, e;
  mt_list(inc_start, v, nf, b, e);
  for (long long i = b + 1; i < e; ++i) {
    const int x = inc[i];
    long long j = i;
    for (; j > b && inc[j - 1] > x; --j) inc[j] = inc[j - 1];
    inc[j] = x;
  }
}

// ---------------------------------------------------------------------------------------------------------------- components
__device__ __forceinline__ int mt_parent(const int* parent, int v) {      // what a find reads, clamped to [0, v]
  const int p = __atomic_load_n(parent + v, __ATOMIC_RELAXED);
  return p < 0 ? 0 : (p > v ? v : p);
}

// The root above v, halving the path on the way.  Strictly downward: at most nv steps.
__device__ __forceinline__ int mt_find(int* parent, int v, long long nv) {
  for (long long n = 0; n < nv; ++n) {
    const int p = mt_parent(parent, v);
    if (p == v) break;
    const int g = mt_parent(parent, p);
    if (g != p) atomicMin(parent + v, g);      // (v is no root and never becomes one again: only ancestors of v are ever written here)
    v = g;
  }
  return v;
}

__device__ __forceinline__ void mt_union(int* parent, int a, int b, long long nv) {
  for (long long n = 0; n <= nv; ++n) {      // max(a, b) strictly decreases from one attempt to the next
    a = mt_find(parent, a, nv), b = mt_find(parent, b, nv);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicCAS(parent + a, a, b);
    if (old == a) return;
    a = old < 0 ? 0 : (old > a ? a : old);      // another thread hooked a first (old < a): go on from where it points
  }
}

__global__ __launch_bounds__(kNNThreads) void mt_cc_init_kernel(int* __restrict__ parent, uint8_t* __restrict__ used, long long nv) {
  const long long v = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (v < nv) parent[v] = (int)v, used[v] = 0;
}

__global__ __launch_bounds__(kNNThreads) void mt_cc_hook_kernel(MTMesh m, int* parent, uint8_t* used) {
  const long long f = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (f >= m.nf) return;
  int id[3], s;
  if (mt_face(m, f, id, s) == kInvalid) return;
  used[id[0]] = 1, used[id[1]] = 1, used[id[2]] = 1;      // (byte stores of the same value)
  mt_union(parent, id[0], id[1], m.nv);
  mt_union(parent, id[0], id[2], m.nv);
}

// label[v] = the root above v (parent is only read here); flag[v] = v is the root of a component with a face.
__global__ __launch_bounds__(kNNThreads) void mt_cc_flatten_kernel(const int* __restrict__ parent, const uint8_t* __restrict__ used,
                                                                  int* __restrict__ label, unsigned* __restrict__ flag, long long nv) {
  const long long v = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (v >= nv) return;
  int r = (int)v;
  for (long long n = 0; n < nv; ++n) {
    const int p = mt_parent(parent, r);
    if (p == r) break;
    r = p;
  }
  label[v] = r;
  flag[v] = (r == (int)v && used[v]) ? 1u : 0u;
}

__global__ __launch_bounds__(kNNThreads) void mt_cc_vertex_kernel(const int* __restrict__ label, const uint8_t* __restrict__ used,
                                                                 const unsigned* __restrict__ rank, int* __restrict__ vertex_component, long long nv) {
  const long long v = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (v < nv) vertex_component[v] = used[v] ? (int)rank[nn_clamp(label[v], nv)] : -1;
}

__global__ __launch_bounds__(kNNThreads) void mt_cc_face_kernel(MTMesh m, const int* __restrict__ label, const unsigned* __restrict__ rank,
                                                               int* __restrict__ face_component) {
  const long long f = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (f >= m.nf) return;
  int id[3], s;
  face_component[f] = mt_face(m, f, id, s) == kInvalid ? -1 : (int)rank[nn_clamp(label[id[0]], m.nv)];
}

// out[s] = rank[start[s]] for s = 0 .. nscene: what the scenes before s hold (rank is exclusive and has n + 1 words)
__global__ __launch_bounds__(kNNThreads) void mt_starts_kernel(const unsigned* __restrict__ rank, const int* __restrict__ start, long long n, int nscene,
                                                              int* __restrict__ out) {
  const int s = blockIdx.x * kNNThreads + threadIdx.x;
  if (s <= nscene) out[s] = (int)rank[nn_clamp(start[s], n)];
}

__global__ __launch_bounds__(kNNThreads) void mt_table_init_kernel(int* __restrict__ root, int* __restrict__ faces, int* __restrict__ vertices,
                                                                  long long ncomp) {
  const long long c = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (c < ncomp) root[c] = 0x7fffffff, faces[c] = 0, vertices[c] = 0;
}

__global__ __launch_bounds__(kNNThreads) void mt_table_kernel(const int* __restrict__ component, long long n, long long ncomp, int* __restrict__ count,
                                                             int* __restrict__ root) {
  const long long i = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (i >= n) return;
  const long long c = component[i];
  if (c < 0 || c >= ncomp) return;
  atomicAdd(count + c, 1);
  if (root) atomicMin(root + c, (int)i);
}

// ---------------------------------------------------------------------------------------------------------------- report
// Totals of a workgroup: LDS when all its rows lie in one scene (`uniform`), the global table otherwise.
__device__ __forceinline__ void mt_add(int* lds, int* totals, bool uniform, int s, int which) {
  if (uniform) atomicAdd(lds + which, 1);
  else atomicAdd(totals + (long long)s * kMTTotals + which, 1);
}

__device__ __forceinline__ void mt_report_face(const MTMesh& m, long long f, const int* inc_start, const int* inc, int* lds, int* totals,
                                               unsigned* flags, bool uniform) {
  int id[3], s;
  const int cls = mt_face(m, f, id, s);
  if (s < 0) return;
  if (cls != kRegular) return mt_add(lds, totals, uniform, s, cls == kInvalid ? kTInvalid : kTRepeated);
  mt_add(lds, totals, uniform, s, kTRegular);
  for (int e = 0; e < 3; ++e) {
    const int a = id[e], b = id[(e + 1) % 3];
    long long ab, ae, bb, be;
    mt_list(inc_start, a, m.nf, ab, ae);
    mt_list(inc_start, b, m.nf, bb, be);
    const bool walk_b = be - bb < ae - ab;
    const int w = walk_b ? b : a, other = walk_b ? a : b;
    const long long lo = walk_b ? bb : ab, hi = walk_b ? be : ae;
    int users = 0, same = 0;
    long long owner = 3 * m.nf;
    for (long long k = lo; k < hi; ++k) {      // (at most 3 nf entries)
      long long g;
      int c, gid[3];
      if (!mt_entry(inc, m.faces, k, w, m.nv, m.nf, g, c, gid)) continue;
      const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
      int ek;      // the edge of g between w and other: edge j runs from corner j to corner j + 1
      if (gid[c1] == other) ek = c;
      else if (gid[c2] == other) ek = c2;
      else continue;
      ++users;
      same += gid[ek] == a ? 1 : 0;      // g runs along the edge from a to b, as f does
      const long long key = g * 3 + ek;
      owner = key < owner ? key : owner;
    }
    if (owner != f * 3 + e) continue;
    mt_add(lds, totals, uniform, s, kTEdges);
    unsigned bit = 0;
    if (users == 1) mt_add(lds, totals, uniform, s, kTBoundary), bit = MVD_TOPO_FLAG_BOUNDARY;
    if (users > 2) mt_add(lds, totals, uniform, s, kTNonManifold), bit = MVD_TOPO_FLAG_NONMANIFOLD;
    if (users == 2 && same == 2) mt_add(lds, totals, uniform, s, kTMisoriented);
    if (bit) atomicOr(flags + a, bit), atomicOr(flags + b, bit);
  }
}

// rows [first, last] of a workgroup lie in ONE scene (starts are non-decreasing, so the ends decide): that scene, else -1
__device__ __forceinline__ int mt_block_scene(const int* start, int nscene, long long n, long long first) {
  const long long last = first + kNNThreads - 1 < n ? first + kNNThreads - 1 : n - 1;
  const int s0 = nn_find_scene(start, nscene, n, first), s1 = nn_find_scene(start, nscene, n, last);
  return s0 == s1 ? s0 : -1;
}

__device__ __forceinline__ void mt_flush(const int* lds, int* totals, int s) {
  __syncthreads();
  if (s >= 0 && threadIdx.x < kMTTotals && lds[threadIdx.x] != 0) atomicAdd(totals + (long long)s * kMTTotals + threadIdx.x, lds[threadIdx.x]);
}

__global__ __launch_bounds__(kNNThreads) void mt_report_face_kernel(MTMesh m, const int* __restrict__ inc_start, const int* __restrict__ inc,
                                                                   int* totals, unsigned* flags) {
  __shared__ int lds[kMTTotals];
  if (threadIdx.x < kMTTotals) lds[threadIdx.x] = 0;
  __syncthreads();
  const long long first = (long long)blockIdx.x * kNNThreads, f = first + threadIdx.x;
  const int sb = mt_block_scene(m.fstart, m.nscene, m.nf, first);
  if (f < m.nf) mt_report_face(m, f, inc_start, inc, lds, totals, flags, sb >= 0);
  mt_flush(lds, totals, sb);
}

__global__ __launch_bounds__(kNNThreads) void mt_report_vertex_kernel(MTMesh m, const int* __restrict__ vertex_component, const unsigned* __restrict__ flags,
                                                                     int* totals, uint8_t* __restrict__ vertex_flags) {
  __shared__ int lds[kMTTotals];
  if (threadIdx.x < kMTTotals) lds[threadIdx.x] = 0;
  __syncthreads();
  const long long first = (long long)blockIdx.x * kNNThreads, v = first + threadIdx.x;
  const int sb = mt_block_scene(m.vstart, m.nscene, m.nv, first);
  if (v < m.nv) {
    vertex_flags[v] = (uint8_t)(flags[v] & 0xffu);
    const int s = nn_find_scene(m.vstart, m.nscene, m.nv, v);
    if (s >= 0) mt_add(lds, totals, sb >= 0, s, vertex_component[v] >= 0 ? kTUsed : kTUnref);
  }
  mt_flush(lds, totals, sb);
}

__global__ __launch_bounds__(kNNThreads) void mt_report_scene_kernel(const int* __restrict__ component_start, int nscene, int* __restrict__ totals) {
  const int s = blockIdx.x * kNNThreads + threadIdx.x;
  if (s >= nscene) return;
  int* t = totals + (long long)s * kMTTotals;
  t[kTComponents] = component_start[s + 1] - component_start[s];
  t[kTEuler] = t[kTUsed] - t[kTEdges] + t[kTRegular];
}

// ---------------------------------------------------------------------------------------------------------------- filter
__global__ __launch_bounds__(kNNThreads) void mt_filter_flag_kernel(MTMesh m, const uint8_t* __restrict__ keep, unsigned* vflag, unsigned* __restrict__ fflag) {
  const long long f = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (f >= m.nf) return;
  int id[3], s;
  if (!keep[f] || mt_face(m, f, id, s) == kInvalid) return;
  fflag[f] = 1u;
  vflag[id[0]] = 1u, vflag[id[1]] = 1u, vflag[id[2]] = 1u;      // (plain stores of the same value)
}

// rank: exclusive, n + 1 words; row i is kept iff rank[i + 1] != rank[i], and then goes to rank[i]
__global__ __launch_bounds__(kNNThreads) void mt_filter_vertex_kernel(const float* __restrict__ vertices, const float* __restrict__ rgb,
                                                                     const unsigned* __restrict__ vrank, long long nv, long long nvo,
                                                                     float* __restrict__ out_vertices, float* __restrict__ out_rgb,
                                                                     int* __restrict__ vertex_index) {
  const long long v = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (v >= nv) return;
  const long long j = vrank[v];
  if (vrank[v + 1] == vrank[v] || j >= nvo) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    out_vertices[j * 3 + k] = vertices[v * 3 + k];
    if (rgb) out_rgb[j * 3 + k] = rgb[v * 3 + k];
  }
  vertex_index[j] = (int)v;
}

__global__ __launch_bounds__(kNNThreads) void mt_filter_face_kernel(const int* __restrict__ faces, const unsigned* __restrict__ vrank,
                                                                   const unsigned* __restrict__ frank, long long nv, long long nf, long long nfo,
                                                                   int* __restrict__ out_faces, int* __restrict__ face_index) {
  const long long f = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (f >= nf) return;
  const long long j = frank[f];
  if (frank[f + 1] == frank[f] || j >= nfo) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) out_faces[j * 3 + k] = (int)vrank[nn_clamp(faces[f * 3 + k], nv)];
  face_index[j] = (int)f;
}

// ---------------------------------------------------------------------------------------------------------------- normals, smoothing
__global__ __launch_bounds__(kNNThreads) void mt_normals_kernel(const float* __restrict__ vertices, const int* __restrict__ faces,
                                                               const int* __restrict__ inc_start, const int* __restrict__ inc, long long nv, long long nf,
                                                               float* __restrict__ normals) {
  const long long v = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (v >= nv) return;
  long long b, e;
  mt_list(inc_start, v, nf, b, e);
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (long long k = b; k < e; ++k) {
    long long g;
    int c, gid[3];
    if (!mt_entry(inc, faces, k, v, nv, nf, g, c, gid)) continue;
    double T[9];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int x = 0; x < 3; ++x) T[j * 3 + x] = (double)vertices[(long long)gid[j] * 3 + x];
    const double ab[3] = {T[3] - T[0], T[4] - T[1], T[5] - T[2]}, ac[3] = {T[6] - T[0], T[7] - T[1], T[8] - T[2]};
    sx += ab[1] * ac[2] - ab[2] * ac[1];
    sy += ab[2] * ac[0] - ab[0] * ac[2];
    sz += ab[0] * ac[1] - ab[1] * ac[0];
  }
  const double len = sqrt((sx * sx + sy * sy) + sz * sz);
  const bool ok = len > 0.0 && len < (double)INFINITY;
  normals[v * 3 + 0] = ok ? (float)(sx / len) : 0.f;
  normals[v * 3 + 1] = ok ? (float)(sy / len) : 0.f;
  normals[v * 3 + 2] = ok ? (float)(sz / len) : 0.f;
}

__device__ __forceinline__ bool mt_finite64(double v) { return fabs(v) < (double)INFINITY; }

__global__ __launch_bounds__(kNNThreads) void mt_smooth_kernel(const float* __restrict__ src, float* __restrict__ dst, const int* __restrict__ faces,
                                                              const int* __restrict__ inc_start, const int* __restrict__ inc,
                                                              const uint8_t* __restrict__ vertex_flags, long long nv, long long nf, double factor,
                                                              int pin_mask) {
  const long long v = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (v >= nv) return;
  const float x[3] = {src[v * 3 + 0], src[v * 3 + 1], src[v * 3 + 2]};
  float y[3] = {x[0], x[1], x[2]};
  if (!(pin_mask && (vertex_flags[v] & pin_mask))) {
    long long b, e, terms = 0;
    mt_list(inc_start, v, nf, b, e);
    double S[3] = {0.0, 0.0, 0.0};
    for (long long k = b; k < e; ++k) {
      long long g;
      int c, gid[3];
      if (!mt_entry(inc, faces, k, v, nv, nf, g, c, gid)) continue;
      const long long n1 = gid[(c + 1) % 3], n2 = gid[(c + 2) % 3];      // the next corner, then the previous one
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        S[a] += (double)src[n1 * 3 + a];
        S[a] += (double)src[n2 * 3 + a];
      }
      terms += 2;
    }
    // a sum of fp32 values in fp64 cannot overflow, so S is finite exactly when every coordinate read was
    if (terms > 0 && mt_finite64(S[0]) && mt_finite64(S[1]) && mt_finite64(S[2]) && nn_finite(x[0]) && nn_finite(x[1]) && nn_finite(x[2])) {
      const double cnt = (double)terms;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double xa = (double)x[a];
        y[a] = (float)(xa + factor * (S[a] / cnt - xa));
      }
    }
  }
  dst[v * 3 + 0] = y[0], dst[v * 3 + 1] = y[1], dst[v * 3 + 2] = y[2];
}

}  // namespace

extern "C" size_t mvd_mesh_incidence_scratch(size_t nv, size_t nf) { return mt_sizes_ok(nv, nf) ? mt_scan_bytes(nv) : 0; }

extern "C" int mvd_mesh_incidence(const int* faces, const int* vertex_start, const int* face_start, size_t nv, size_t nf, int nscene,
                                  int* inc_start, int* inc, void* scratch, size_t scratch_bytes, mvd_stream_t stream) {
  const char* fn = "mvd_mesh_incidence";
  MT_TRY(mt_check_mesh(fn, faces, vertex_start, face_start, nv, nf, nscene));
  MT_TRY(mt_check_table(fn, inc_start, inc, nf));
  MT_TRY(mt_check_scratch(fn, scratch, scratch_bytes, mt_scan_bytes(nv)));
  const hipStream_t st = (hipStream_t)stream;
  const MTMesh m{faces, vertex_start, face_start, (long long)nv, (long long)nf, nscene};
  unsigned* counts = (unsigned*)scratch;
  const hipError_t e = hipMemsetAsync(counts, 0, mt_chunks(nv) * kChunk * sizeof(unsigned), st);
  MVD_CHECK_ARG(e == hipSuccess, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
  if (nf > 0) hipLaunchKernelGGL(mt_inc_count_kernel, mt_grid(nf), dim3(kNNThreads), 0, st, m, counts);
  mt_scan(counts, nv, st);
  hipLaunchKernelGGL(mt_copy_kernel, mt_grid(nv + 1), dim3(kNNThreads), 0, st, counts, inc_start, (long long)nv + 1);
  if (nf > 0) hipLaunchKernelGGL(mt_inc_fill_kernel, mt_grid(nf), dim3(kNNThreads), 0, st, m, counts, inc);
  if (nv > 0 && nf > 0) hipLaunchKernelGGL(mt_inc_sort_kernel, mt_grid(nv), dim3(kNNThreads), 0, st, inc_start, inc, (long long)nv, (long long)nf);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

namespace {
struct MTLabelPlan {
  size_t off_label, off_rank, off_used, bytes;      // parent at 0
};
static MTLabelPlan mt_label_plan(size_t nv) {
  MTLabelPlan p;
  p.off_label = up16(nv * sizeof(int));
  p.off_rank = p.off_label + up16(nv * sizeof(int));
  p.off_used = p.off_rank + mt_scan_bytes(nv);
  p.bytes = p.off_used + up16(nv);
  return p;
}
}  // namespace

extern "C" size_t mvd_mesh_label_scratch(size_t nv, size_t nf) { return mt_sizes_ok(nv, nf) ? mt_label_plan(nv).bytes : 0; }

extern "C" int mvd_mesh_label(const int* faces, const int* vertex_start, const int* face_start, size_t nv, size_t nf, int nscene,
                              int* vertex_component, int* face_component, int* component_start, void* scratch, size_t scratch_bytes,
                              mvd_stream_t stream) {
  const char* fn = "mvd_mesh_label";
  MT_TRY(mt_check_mesh(fn, faces, vertex_start, face_start, nv, nf, nscene));
  MVD_CHECK_ARG(component_start && (vertex_component || nv == 0) && (face_component || nf == 0), "%s: null output", fn);
  MVD_CHECK_ARG((((uintptr_t)vertex_component | (uintptr_t)face_component | (uintptr_t)component_start) & 3) == 0,
                "%s: an output pointer that is not 4-byte aligned", fn);
  const MTLabelPlan p = mt_label_plan(nv);
  MT_TRY(mt_check_scratch(fn, scratch, scratch_bytes, p.bytes));
  const hipStream_t st = (hipStream_t)stream;
  const MTMesh m{faces, vertex_start, face_start, (long long)nv, (long long)nf, nscene};
  char* base = (char*)scratch;
  int *parent = (int*)base, *label = (int*)(base + p.off_label);
  unsigned* rank = (unsigned*)(base + p.off_rank);
  uint8_t* used = (uint8_t*)(base + p.off_used);
  const hipError_t e = hipMemsetAsync(rank, 0, mt_chunks(nv) * kChunk * sizeof(unsigned), st);
  MVD_CHECK_ARG(e == hipSuccess, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
  const dim3 threads(kNNThreads);
  if (nv > 0) hipLaunchKernelGGL(mt_cc_init_kernel, mt_grid(nv), threads, 0, st, parent, used, (long long)nv);
  if (nf > 0) hipLaunchKernelGGL(mt_cc_hook_kernel, mt_grid(nf), threads, 0, st, m, parent, used);
  if (nv > 0) hipLaunchKernelGGL(mt_cc_flatten_kernel, mt_grid(nv), threads, 0, st, parent, used, label, rank, (long long)nv);
  mt_scan(rank, nv, st);
  if (nv > 0) hipLaunchKernelGGL(mt_cc_vertex_kernel, mt_grid(nv), threads, 0, st, label, used, rank, vertex_component, (long long)nv);
  if (nf > 0) hipLaunchKernelGGL(mt_cc_face_kernel, mt_grid(nf), threads, 0, st, m, label, rank, face_component);
  hipLaunchKernelGGL(mt_starts_kernel, mt_grid((size_t)nscene + 1), threads, 0, st, rank, vertex_start, (long long)nv, nscene, component_start);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int mvd_mesh_component_table(const int* vertex_component, const int* face_component, size_t nv, size_t nf, size_t ncomp, int* root,
                                        int* faces, int* vertices, mvd_stream_t stream) {
  const char* fn = "mvd_mesh_component_table";
  MVD_CHECK_ARG(mt_sizes_ok(nv, nf) && ncomp <= nv, "%s: nv=%zu, nf=%zu out of range or ncomp=%zu > nv", fn, nv, nf, ncomp);
  MVD_CHECK_ARG((vertex_component || nv == 0) && (face_component || nf == 0), "%s: null vertex_component or face_component", fn);
  MVD_CHECK_ARG((root && faces && vertices) || ncomp == 0, "%s: null output with ncomp=%zu", fn, ncomp);
  MVD_CHECK_ARG((((uintptr_t)vertex_component | (uintptr_t)face_component | (uintptr_t)root | (uintptr_t)faces | (uintptr_t)vertices) & 3) == 0,
                "%s: a pointer that is not 4-byte aligned", fn);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 threads(kNNThreads);
  if (ncomp > 0) {
    hipLaunchKernelGGL(mt_table_init_kernel, mt_grid(ncomp), threads, 0, st, root, faces, vertices, (long long)ncomp);
    if (nv > 0) hipLaunchKernelGGL(mt_table_kernel, mt_grid(nv), threads, 0, st, vertex_component, (long long)nv, (long long)ncomp, vertices, root);
    if (nf > 0) hipLaunchKernelGGL(mt_table_kernel, mt_grid(nf), threads, 0, st, face_component, (long long)nf, (long long)ncomp, faces, (int*)nullptr);
  }
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" size_t mvd_mesh_topology_scratch(size_t nv, size_t nf) { return mt_sizes_ok(nv, nf) ? up16(nv * sizeof(unsigned)) + 16 : 0; }

extern "C" int mvd_mesh_topology(const int* faces, const int* vertex_start, const int* face_start, size_t nv, size_t nf, int nscene,
                                 const int* inc_start, const int* inc, const int* vertex_component, const int* component_start, int* totals,
                                 uint8_t* vertex_flags, void* scratch, size_t scratch_bytes, mvd_stream_t stream) {
  const char* fn = "mvd_mesh_topology";
  MT_TRY(mt_check_mesh(fn, faces, vertex_start, face_start, nv, nf, nscene));
  MT_TRY(mt_check_table(fn, inc_start, inc, nf));
  MVD_CHECK_ARG(component_start && (vertex_component || nv == 0), "%s: null vertex_component or component_start", fn);
  MVD_CHECK_ARG(totals && (vertex_flags || nv == 0), "%s: null totals or vertex_flags", fn);
  MVD_CHECK_ARG((((uintptr_t)vertex_component | (uintptr_t)component_start | (uintptr_t)totals) & 3) == 0,
                "%s: a pointer that is not 4-byte aligned", fn);
  MT_TRY(mt_check_scratch(fn, scratch, scratch_bytes, up16(nv * sizeof(unsigned)) + 16));
  const hipStream_t st = (hipStream_t)stream;
  const MTMesh m{faces, vertex_start, face_start, (long long)nv, (long long)nf, nscene};
  unsigned* flags = (unsigned*)scratch;
  hipError_t e = hipMemsetAsync(totals, 0, (size_t)nscene * kMTTotals * sizeof(int), st);
  if (e == hipSuccess && nv > 0) e = hipMemsetAsync(flags, 0, nv * sizeof(unsigned), st);
  MVD_CHECK_ARG(e == hipSuccess, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
  const dim3 threads(kNNThreads);
  if (nf > 0) hipLaunchKernelGGL(mt_report_face_kernel, mt_grid(nf), threads, 0, st, m, inc_start, inc, totals, flags);
  if (nv > 0) hipLaunchKernelGGL(mt_report_vertex_kernel, mt_grid(nv), threads, 0, st, m, vertex_component, flags, totals, vertex_flags);
  hipLaunchKernelGGL(mt_report_scene_kernel, mt_grid((size_t)nscene), threads, 0, st, component_start, nscene, totals);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" size_t mvd_mesh_filter_scratch(size_t nv, size_t nf) { return mt_sizes_ok(nv, nf) ? mt_scan_bytes(nv) + mt_scan_bytes(nf) : 0; }

extern "C" int mvd_mesh_filter_count(const int* faces, const uint8_t* keep, const int* vertex_start, const int* face_start, size_t nv, size_t nf,
                                     int nscene, int* new_vertex_start, int* new_face_start, void* scratch, size_t scratch_bytes,
                                     mvd_stream_t stream) {
  const char* fn = "mvd_mesh_filter_count";
  MT_TRY(mt_check_mesh(fn, faces, vertex_start, face_start, nv, nf, nscene));
  MVD_CHECK_ARG(keep || nf == 0, "%s: null keep with nf=%zu", fn, nf);
  MVD_CHECK_ARG(new_vertex_start && new_face_start && (((uintptr_t)new_vertex_start | (uintptr_t)new_face_start) & 3) == 0,
                "%s: null or misaligned new_vertex_start / new_face_start", fn);
  MT_TRY(mt_check_scratch(fn, scratch, scratch_bytes, mt_scan_bytes(nv) + mt_scan_bytes(nf)));
  const hipStream_t st = (hipStream_t)stream;
  const MTMesh m{faces, vertex_start, face_start, (long long)nv, (long long)nf, nscene};
  unsigned *vrank = (unsigned*)scratch, *frank = (unsigned*)((char*)scratch + mt_scan_bytes(nv));
  hipError_t e = hipMemsetAsync(vrank, 0, mt_chunks(nv) * kChunk * sizeof(unsigned), st);
  if (e == hipSuccess) e = hipMemsetAsync(frank, 0, mt_chunks(nf) * kChunk * sizeof(unsigned), st);
  MVD_CHECK_ARG(e == hipSuccess, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
  const dim3 threads(kNNThreads);
  if (nf > 0) hipLaunchKernelGGL(mt_filter_flag_kernel, mt_grid(nf), threads, 0, st, m, keep, vrank, frank);
  mt_scan(vrank, nv, st);
  mt_scan(frank, nf, st);
  hipLaunchKernelGGL(mt_starts_kernel, mt_grid((size_t)nscene + 1), threads, 0, st, vrank, vertex_start, (long long)nv, nscene, new_vertex_start);
  hipLaunchKernelGGL(mt_starts_kernel, mt_grid((size_t)nscene + 1), threads, 0, st, frank, face_start, (long long)nf, nscene, new_face_start);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int mvd_mesh_filter_emit(const float* vertices, const float* rgb, const int* faces, size_t nv, size_t nf, float* out_vertices,
                                    float* out_rgb, int* out_faces, int* vertex_index, int* face_index, size_t nvo, size_t nfo,
                                    const void* scratch, size_t scratch_bytes, mvd_stream_t stream) {
  const char* fn = "mvd_mesh_filter_emit";
  MVD_CHECK_ARG(mt_sizes_ok(nv, nf) && nvo <= nv && nfo <= nf, "%s: nv=%zu, nf=%zu out of range, or nvo=%zu > nv or nfo=%zu > nf", fn, nv, nf, nvo, nfo);
  MVD_CHECK_ARG((vertices || nv == 0) && (faces || nf == 0), "%s: null vertices or faces", fn);
  MVD_CHECK_ARG((out_vertices && vertex_index && (out_rgb || !rgb)) || nvo == 0, "%s: null vertex output with nvo=%zu", fn, nvo);
  MVD_CHECK_ARG((out_faces && face_index) || nfo == 0, "%s: null face output with nfo=%zu", fn, nfo);
  const uintptr_t low = (uintptr_t)vertices | (uintptr_t)rgb | (uintptr_t)faces | (uintptr_t)out_vertices | (uintptr_t)out_rgb | (uintptr_t)out_faces |
                        (uintptr_t)vertex_index | (uintptr_t)face_index;
  MVD_CHECK_ARG((low & 3) == 0, "%s: a pointer that is not 4-byte aligned", fn);
  MT_TRY(mt_check_scratch(fn, scratch, scratch_bytes, mt_scan_bytes(nv) + mt_scan_bytes(nf)));
  const hipStream_t st = (hipStream_t)stream;
  const unsigned *vrank = (const unsigned*)scratch, *frank = (const unsigned*)((const char*)scratch + mt_scan_bytes(nv));
  const dim3 threads(kNNThreads);
  if (nv > 0 && nvo > 0)
    hipLaunchKernelGGL(mt_filter_vertex_kernel, mt_grid(nv), threads, 0, st, vertices, rgb, vrank, (long long)nv, (long long)nvo, out_vertices, out_rgb,
                       vertex_index);
  if (nf > 0 && nfo > 0)
    hipLaunchKernelGGL(mt_filter_face_kernel, mt_grid(nf), threads, 0, st, faces, vrank, frank, (long long)nv, (long long)nf, (long long)nfo, out_faces,
                       face_index);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int mvd_mesh_vertex_normals(const float* vertices, const int* faces, const int* inc_start, const int* inc, size_t nv, size_t nf,
                                       float* normals, mvd_stream_t stream) {
  const char* fn = "mvd_mesh_vertex_normals";
  MVD_CHECK_ARG(mt_sizes_ok(nv, nf), "%s: nv=%zu beyond 2^31 - 1 - %d or nf=%zu beyond (2^31 - 1) / 3", fn, nv, kChunk, nf);
  MT_TRY(mt_check_table(fn, inc_start, inc, nf));
  MVD_CHECK_ARG(((vertices && normals) || nv == 0) && (faces || nf == 0), "%s: null vertices, faces or normals", fn);
  MVD_CHECK_ARG((((uintptr_t)vertices | (uintptr_t)faces | (uintptr_t)normals) & 3) == 0, "%s: a pointer that is not 4-byte aligned", fn);
  if (nv > 0)
    hipLaunchKernelGGL(mt_normals_kernel, mt_grid(nv), dim3(kNNThreads), 0, (hipStream_t)stream, vertices, faces, inc_start, inc, (long long)nv,
                       (long long)nf, normals);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int mvd_mesh_smooth(const float* vertices, const int* faces, const int* inc_start, const int* inc, const uint8_t* vertex_flags,
                               size_t nv, size_t nf, int passes, double lam, double mu, int pin_mask, float* out, float* tmp,
                               mvd_stream_t stream) {
  const char* fn = "mvd_mesh_smooth";
  MVD_CHECK_ARG(mt_sizes_ok(nv, nf), "%s: nv=%zu beyond 2^31 - 1 - %d or nf=%zu beyond (2^31 - 1) / 3", fn, nv, kChunk, nf);
  MVD_CHECK_ARG(passes >= 0 && passes <= MVD_SMOOTH_MAX_PASSES, "%s: passes=%d outside [0, %d]", fn, passes, MVD_SMOOTH_MAX_PASSES);
  MVD_CHECK_ARG(fabs(lam) < (double)INFINITY && fabs(mu) < (double)INFINITY, "%s: lam=%g or mu=%g is not finite", fn, lam, mu);
  MVD_CHECK_ARG(pin_mask >= 0 && pin_mask <= 255, "%s: pin_mask=%d outside [0, 255]", fn, pin_mask);
  MT_TRY(mt_check_table(fn, inc_start, inc, nf));
  MVD_CHECK_ARG(((vertices && out) || nv == 0) && (faces || nf == 0), "%s: null vertices, faces or out", fn);
  MVD_CHECK_ARG(tmp || passes < 2 || nv == 0, "%s: null tmp with passes=%d", fn, passes);
  MVD_CHECK_ARG(vertex_flags || pin_mask == 0 || nv == 0, "%s: null vertex_flags with pin_mask=%d", fn, pin_mask);
  MVD_CHECK_ARG((out != vertices && tmp != vertices && out != tmp) || nv == 0, "%s: vertices, out and tmp must be three buffers", fn);
  MVD_CHECK_ARG((((uintptr_t)vertices | (uintptr_t)faces | (uintptr_t)out | (uintptr_t)tmp) & 3) == 0, "%s: a pointer that is not 4-byte aligned", fn);
  const hipStream_t st = (hipStream_t)stream;
  if (nv > 0 && passes == 0) {
    const hipError_t e = hipMemcpyAsync(out, vertices, nv * 3 * sizeof(float), hipMemcpyDeviceToDevice, st);
    MVD_CHECK_ARG(e == hipSuccess, "%s: hipMemcpyAsync: %s", fn, hipGetErrorString(e));
  }
  const float* src = vertices;
  for (int k = 0; k < passes && nv > 0; ++k) {
    float* dst = ((passes - 1 - k) & 1) ? tmp : out;      // the last pass writes `out`
    hipLaunchKernelGGL(mt_smooth_kernel, mt_grid(nv), dim3(kNNThreads), 0, st, src, dst, faces, inc_start, inc, vertex_flags, (long long)nv,
                       (long long)nf, (k & 1) ? mu : lam, pin_mask);
    src = dst;
  }
  MVD_CHECK_LAUNCH(fn);
  return 0;
}
