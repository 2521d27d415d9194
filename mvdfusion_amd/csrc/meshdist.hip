// The exact closest point of a triangle mesh for every query point (include/mvd_hip.h: mvd_nearest_on_mesh has the rule in full).
//
// PER PAIR (md_closest): fp64 on exact conversions of the fp32 inputs, + - * / and comparisons only, in the order of the header -- the
// Voronoi regions of the triangle (vertices, then edges, then the interior), or the three segments for a face whose normal is exactly 0.
// The searches keep only (d2, face) per query in the total order of the header; the winner is evaluated once more for the outputs, which
// gives the same bits (the same operations on the same values, no contraction).
// BRUTE: one thread per query; the workgroup walks the scenes its queries belong to and stages each scene's faces through LDS in tiles
// of kMDTile RESOLVED records (nine coordinates, the face row, the candidate flag: 48 bytes).  Every lane reads the same record at once:
// a broadcast, no bank conflict, and the two dependent gathers (face row -> vertex ids -> coordinates) are paid once per workgroup.
// GRID, build: md_bounds_kernel (the bounding box of the vertices of every scene's candidate faces: nn_key under atomicMin) -> count
// (md_cell_kernel<0>: a face is referenced from EVERY cell the axis-aligned box of its three vertices overlaps, found with the cell
// function the queries use; a face whose box spans more than MVD_MESH_SPAN cells along an axis goes to its scene's OVERSIZE list
// instead) -> the two-level exclusive scan of nn_grid.hpp -> fill (md_cell_kernel<1>: face rows, 4 bytes per reference; begins turn
// into ends).  Integer atomics only.  A face outside the oversize list has at most MVD_MESH_SPAN^3 references, so the scratch is a host
// function of (nf, nscene, method, grid) and nothing is read back.  A scene's oversize list lives in the slots of its own face range
// (it cannot hold more faces than the scene has), so it needs no scan.
// GRID, query (md_query_grid): the oversize list of the scene first, every face of it -- which also gives the walk its first bound --
// then nn_walk_grid's Chebyshev shells with its stop rule and margins unchanged.
//   Why the stop rule holds for triangles.  After shell r the visited block is the cells [c - r, c + r] per axis (clipped to the grid).
//   A face that is in no oversize list and has not been offered has no cell of its reference box in that block, so along SOME axis k
//   the whole cell range of its box lies at >= c_k + r + 1 or at <= c_k - r - 1.  The range's ends are the cells of the smallest and the
//   largest vertex coordinate along k, and the cell function is monotone (a subtraction, a product with a positive number, floor and a
//   clamp: each non-decreasing), so EVERY point of the face -- its coordinate along k lies between those two -- sits at >= c_k + r + 1
//   cell units, or below c_k - r, exactly as a target point of such a cell does in nearest.hip.  The bound of the walk is a lower bound of
//   d2 to any such point; its margins (0.1 %, 0.001 cell) cover the fp32 rounding of the cell units as there.  The box of the grid is the
//   box of the candidate faces' vertices, and a triangle lies inside the box of its vertices, so "what the query lies outside the box"
//   holds for every point of every face too.  The walk compares the fp64 best against the fp32 bound exactly (promotion).
//   The order in which faces are met, and how often (a face is met once per cell it is referenced from), cannot matter: the selection is
//   a minimum in a total order.
// Every reference read back from the scratch counts only when it lies in the scene's face range, and every face is re-validated (ids,
// finite coordinates) where it is evaluated, so MVD_NN_QUERY on a scratch it did not build reads nothing out of bounds.
// The per-pair function, the cell assignment and the walk are host-and-device functions: tools/meshdist_host.hip runs them serially on
// a CPU (under the sanitizers) against the brute force.
//
// Chosen: face rows per cell with gathered vertices (4 bytes per reference, three dependent loads per visit) against resolved records
// per reference (48 bytes each, up to 27 per face).  Not tried: the latter; ONE resolved record per face that the references index (two
// dependent loads per visit instead of three); a conservative fp32 bound per face before the fp64 evaluation; skipping a face already
// met in an earlier cell; staging the oversize list through LDS; a BVH.
#include "nn_grid.hpp"

namespace {

constexpr int kMDTile = 512;                          // resolved records per LDS tile of the brute kernel (24 KB)
constexpr int kMDMaxGrid = 256;                       // the largest `grid`: that of mvd_nearest_points (nearest.hip: kMaxGrid)
constexpr int kMDSpan = MVD_MESH_SPAN;
constexpr int kMDRefs = kMDSpan * kMDSpan * kMDSpan;  // the most references a face outside the oversize list has
// MVD_NN_AUTO: the grid from this many faces per scene upward -- an INTERFACE default, not swept.  Automatic grid = sqrt(faces per scene /
// kMDGridDivisor): from ONE sweep (marching-tetrahedra spheres of 74 k and 296 k faces, 65 536
// queries 5 % off the surface), whose best sizes were 24 - 32 and 48.  A cell then holds tens of references: a finer grid sends the
// long faces of such a mesh to the oversize list and makes every query walk more, mostly empty, shells.
constexpr long long kMDGridMinFaces = 1024;
constexpr float kMDGridDivisor = 96.f;

struct MDArgs {
  const float *query, *vertices;
  const int *qstart, *tstart, *faces;                 // tstart: face_start (the names nn_walk_grid uses)
  int* face;
  float *dist2, *point, *bary;
  int* region;
  float* normal;
  unsigned* box;                                      // per scene: keys of min x, y, z, then ~keys of max x, y, z
  unsigned* nover;                                    // per scene: faces in its oversize list
  unsigned* cells;                                    // nscene * g^3 words padded to kChunk: counts -> begins -> ends
  unsigned* blocks;                                   // one word per chunk, and the total behind them
  int* refs;                                          // nref face rows, cell after cell
  int* over;                                          // nf face rows: scene s's oversize list from over[face_start[s]]
  long long nq, nv, nt, nref;                         // nt: nf
  int nscene, g;
};

// ---------------------------------------------------------------------------------------------------------------- per pair
struct MDHit {
  double d2, b[3], c[3];
  int region;
};

NN_HD double md_dot(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// c = b0 A + b1 B + b2 C and d2 = |p - c|^2, in the header's order.  T: the nine coordinates A, B, C.
NN_HD void md_finish(const double* P, const double* T, double b0, double b1, double b2, int region, MDHit& h) {
  h.b[0] = b0, h.b[1] = b1, h.b[2] = b2, h.region = region;
#pragma unroll
  for (int k = 0; k < 3; ++k) h.c[k] = (b0 * T[k] + b1 * T[3 + k]) + b2 * T[6 + k];
  const double dx = P[0] - h.c[0], dy = P[1] - h.c[1], dz = P[2] - h.c[2];
  h.d2 = (dx * dx + dy * dy) + dz * dz;
}

// Segment e of the face (0: A -> B, 1: B -> C, 2: C -> A) as a candidate of the degenerate rule; kept when strictly nearer.
template <int E>
NN_HD void md_segment(const double* P, const double* T, MDHit& best) {
  constexpr int S = E, F = (E + 1) % 3;
  const double se[3] = {T[3 * F + 0] - T[3 * S + 0], T[3 * F + 1] - T[3 * S + 1], T[3 * F + 2] - T[3 * S + 2]};
  const double sp[3] = {P[0] - T[3 * S + 0], P[1] - T[3 * S + 1], P[2] - T[3 * S + 2]};
  const double len2 = md_dot(se, se);
  double t = 0.0;
  if (len2 != 0.0) t = md_dot(sp, se) / len2;      // a segment of zero length is its first end point
  if (!(t > 0.0)) t = 0.0;
  if (t > 1.0) t = 1.0;
  double b[3] = {0.0, 0.0, 0.0};
  b[S] = 1.0 - t, b[F] = t;
  MDHit h;
  md_finish(P, T, b[0], b[1], b[2], t == 0.0 ? S : (t == 1.0 ? F : 3 + E), h);
  if (E == 0 || h.d2 < best.d2) best = h;
}

// THE closest point of the header.  P: the query, T: A, B, C; all finite.
NN_HD void md_closest(const double* P, const double* T, MDHit& h) {
  const double ab[3] = {T[3] - T[0], T[4] - T[1], T[5] - T[2]}, ac[3] = {T[6] - T[0], T[7] - T[1], T[8] - T[2]};
  const double nx = ab[1] * ac[2] - ab[2] * ac[1], ny = ab[2] * ac[0] - ab[0] * ac[2], nz = ab[0] * ac[1] - ab[1] * ac[0];
  bool flat = nx == 0.0 && ny == 0.0 && nz == 0.0;
  if (!flat) {
    const double ap[3] = {P[0] - T[0], P[1] - T[1], P[2] - T[2]};
    const double d1 = md_dot(ab, ap), d2 = md_dot(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) return md_finish(P, T, 1.0, 0.0, 0.0, 0, h);
    const double bp[3] = {P[0] - T[3], P[1] - T[4], P[2] - T[5]};
    const double d3 = md_dot(ab, bp), d4 = md_dot(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) return md_finish(P, T, 0.0, 1.0, 0.0, 1, h);
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
      const double den = d1 - d3, v = den == 0.0 ? 0.0 : d1 / den;
      return md_finish(P, T, 1.0 - v, v, 0.0, 3, h);
    }
    const double cp[3] = {P[0] - T[6], P[1] - T[7], P[2] - T[8]};
    const double d5 = md_dot(ab, cp), d6 = md_dot(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) return md_finish(P, T, 0.0, 0.0, 1.0, 2, h);
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
      const double den = d2 - d6, w = den == 0.0 ? 0.0 : d2 / den;
      return md_finish(P, T, 1.0 - w, 0.0, w, 5, h);
    }
    const double va = d3 * d6 - d5 * d4, e43 = d4 - d3, e56 = d5 - d6;
    if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) {
      const double den = e43 + e56, w = den == 0.0 ? 0.0 : e43 / den;
      return md_finish(P, T, 0.0, 1.0 - w, w, 4, h);
    }
    const double den = (va + vb) + vc;
    if (den != 0.0) {
      const double v = vb / den, w = vc / den;
      return md_finish(P, T, (1.0 - v) - w, v, w, 6, h);
    }
    flat = true;      // (a zero denominator is never divided by: the face is treated as its three segments)
  }
  md_segment<0>(P, T, h);
  md_segment<1>(P, T, h);
  md_segment<2>(P, T, h);
}

// The unit normal of the header: (B - A) x (C - A) / its length in fp64; 0 for a face without one.
NN_HD void md_normal(const double* T, double* n) {
  const double ab[3] = {T[3] - T[0], T[4] - T[1], T[5] - T[2]}, ac[3] = {T[6] - T[0], T[7] - T[1], T[8] - T[2]};
  const double nx = ab[1] * ac[2] - ab[2] * ac[1], ny = ab[2] * ac[0] - ab[0] * ac[2], nz = ab[0] * ac[1] - ab[1] * ac[0];
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);
  const bool ok = len > 0.0 && len < (double)INFINITY;
  n[0] = ok ? nx / len : 0.0, n[1] = ok ? ny / len : 0.0, n[2] = ok ? nz / len : 0.0;
}

// The nine coordinates of face f.  false: not a candidate (an id outside [0, nv), a coordinate that is not finite).
NN_HD bool md_load_face(const MDArgs& a, long long f, float* v) {
  const int i0 = a.faces[f * 3 + 0], i1 = a.faces[f * 3 + 1], i2 = a.faces[f * 3 + 2];
  if (i0 < 0 || i0 >= a.nv || i1 < 0 || i1 >= a.nv || i2 < 0 || i2 >= a.nv) return false;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    v[k] = a.vertices[(long long)i0 * 3 + k], v[3 + k] = a.vertices[(long long)i1 * 3 + k], v[6 + k] = a.vertices[(long long)i2 * 3 + k];
    ok = ok && nn_finite(v[k]) && nn_finite(v[3 + k]) && nn_finite(v[6 + k]);
  }
  return ok;
}

// What a search keeps per query: the minimum of (d2 in fp64, face row).  THE selection rule of the header.
struct MDOne {
  double best = (double)INFINITY;
  int bestf = -1;
  NN_HD void take(double d2, int f) {
    if (d2 < best || (d2 == best && f < bestf)) best = d2, bestf = f;      // (bestf = -1 with best = +inf: an infinite d2 never wins)
  }
  NN_HD double worst() const { return best; }
};

NN_HD void md_offer_coords(const float* v, int f, const double* P, MDOne& keep) {
  double T[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) T[k] = (double)v[k];
  MDHit h;
  md_closest(P, T, h);
  keep.take(h.d2, f);
}

NN_HD void md_offer(const MDArgs& a, long long f, const double* P, MDOne& keep) {
  float v[9];
  if (md_load_face(a, f, v)) md_offer_coords(v, (int)f, P, keep);
}

// The faces referenced from the cells [ca, cb] of a scene against the query (nn_walk_grid's visit).
NN_HD void nn_visit(const MDArgs& a, long long scene_cell0, long long ca, long long cb, long long t0, long long t1, float qx, float qy, float qz,
                    MDOne& keep) {
  const long long first = scene_cell0 + ca, last = scene_cell0 + cb;
  const long long begin = nn_clamp(first > 0 ? (long long)a.cells[first - 1] : 0ll, a.nref), end = nn_clamp((long long)a.cells[last], a.nref);
  const double P[3] = {(double)qx, (double)qy, (double)qz};
  for (long long k = begin; k < end; ++k) {
    const long long f = a.refs[k];
    if (f >= t0 && f < t1) md_offer(a, f, P, keep);
  }
}

// Every output of query i from the winner (or from none).  A NULL output is not written.
NN_HD void md_write(const MDArgs& a, long long i, const float* q, int bestf) {
  const float nan = __builtin_nanf("");
  MDHit h;
  h.d2 = (double)INFINITY, h.region = -1;
  double n[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 3; ++k) h.b[k] = 0.0, h.c[k] = (double)nan;
  float v[9];
  if (bestf >= 0 && bestf < a.nt && md_load_face(a, bestf, v)) {
    double T[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) T[k] = (double)v[k];
    const double P[3] = {(double)q[0], (double)q[1], (double)q[2]};
    md_closest(P, T, h);
    if (a.normal) md_normal(T, n);
  } else {
    bestf = -1;
  }
  if (a.face) a.face[i] = bestf;
  if (a.dist2) a.dist2[i] = (float)h.d2;
  if (a.region) a.region[i] = h.region;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (a.point) a.point[i * 3 + k] = (float)h.c[k];
    if (a.bary) a.bary[i * 3 + k] = (float)h.b[k];
    if (a.normal) a.normal[i * 3 + k] = (float)n[k];
  }
}

// ---------------------------------------------------------------------------------------------------------------- grid: build pieces
// The cells the box of a candidate face overlaps, per axis [lo, hi]; true: the face belongs in the oversize list.
NN_HD bool md_face_cells(const SceneGrid& G, const float* v, int* lo, int* hi) {
  bool over = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float mn = fminf(fminf(v[k], v[3 + k]), v[6 + k]), mx = fmaxf(fmaxf(v[k], v[3 + k]), v[6 + k]);
    lo[k] = nn_cell(G, k, nn_units(G, k, mn)), hi[k] = nn_cell(G, k, nn_units(G, k, mx));
    over = over || hi[k] - lo[k] + 1 > kMDSpan;
  }
  return over;
}

NN_HD unsigned md_add(unsigned* p) {
#ifdef __HIP_DEVICE_COMPILE__
  return atomicAdd(p, 1u);
#else
  return (*p)++;
#endif
}

// Face f counted (FILL = 0; the oversize list is written here) or placed (FILL = 1) in the cells of its scene.
template <int FILL>
NN_HD void md_place_face(const MDArgs& a, long long f) {
  const int s = nn_find_scene(a.tstart, a.nscene, a.nt, f);
  if (s < 0) return;
  float v[9];
  if (!md_load_face(a, f, v)) return;
  const SceneGrid G = nn_scene_grid(a.box + (size_t)s * 6, a.g);
  if (!G.ok) return;
  int lo[3], hi[3];
  if (md_face_cells(G, v, lo, hi)) {
    if (!FILL) {
      const long long t0 = nn_clamp(a.tstart[s], a.nt), t1 = nn_clamp(a.tstart[s + 1], a.nt);
      const long long at = t0 + (long long)md_add(a.nover + s);
      if (at < t1) a.over[at] = (int)f;      // (always: the list holds faces of [t0, t1) only, each once)
    }
    return;
  }
  unsigned* cells = a.cells + (long long)s * a.g * a.g * a.g;      // (n[k] <= g: inside the scene's g^3 words)
  for (int z = lo[2]; z <= hi[2]; ++z)
    for (int y = lo[1]; y <= hi[1]; ++y)
      for (int x = lo[0]; x <= hi[0]; ++x) {
        const unsigned at = md_add(cells + ((long long)z * G.n[1] + y) * G.n[0] + x);
        if (FILL && (long long)at < a.nref) a.refs[at] = (int)f;
      }
}

// One query against the built grid: the scene's oversize list, then the shell walk.
NN_HD void md_query_grid(const MDArgs& a, long long i) {
  const float q[3] = {a.query[i * 3 + 0], a.query[i * 3 + 1], a.query[i * 3 + 2]};
  MDOne one;
  const int s = nn_find_scene(a.qstart, a.nscene, a.nq, i);
  if (s >= 0 && nn_finite(q[0]) && nn_finite(q[1]) && nn_finite(q[2])) {
    const long long t0 = nn_clamp(a.tstart[s], a.nt), t1 = nn_clamp(a.tstart[s + 1], a.nt);
    const long long n = nn_clamp((long long)a.nover[s], t1 - t0);
    const double P[3] = {(double)q[0], (double)q[1], (double)q[2]};
    for (long long k = 0; k < n; ++k) {
      const long long f = a.over[t0 + k];
      if (f >= t0 && f < t1) md_offer(a, f, P, one);
    }
    nn_walk_grid(a, i, one);
  }
  md_write(a, i, q, one.bestf);
}

// ---------------------------------------------------------------------------------------------------------------- kernels
struct alignas(16) TriRec {
  float v[9];
  int id, ok, pad;
};

__global__ __launch_bounds__(kNNThreads) void md_brute_kernel(MDArgs a) {
  __shared__ TriRec tile[kMDTile];
  __shared__ int span[2];
  const long long i = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  const bool live = i < a.nq;
  const int s = live ? nn_find_scene(a.qstart, a.nscene, a.nq, i) : -1;
  if (threadIdx.x == 0) span[0] = a.nscene, span[1] = -1;
  __syncthreads();
  if (s >= 0) atomicMin(&span[0], s), atomicMax(&span[1], s);
  __syncthreads();
  const int s_lo = span[0], s_hi = span[1];      // (uniform: the scenes this workgroup's queries belong to)
  float q[3] = {0.f, 0.f, 0.f};
  if (live) q[0] = a.query[i * 3 + 0], q[1] = a.query[i * 3 + 1], q[2] = a.query[i * 3 + 2];
  const bool searching = s >= 0 && nn_finite(q[0]) && nn_finite(q[1]) && nn_finite(q[2]);
  const double P[3] = {(double)q[0], (double)q[1], (double)q[2]};
  MDOne one;
  for (int sc = s_lo; sc <= s_hi; ++sc) {
    const long long t0 = nn_clamp(a.tstart[sc], a.nt), t1 = nn_clamp(a.tstart[sc + 1], a.nt);
    for (long long base = t0; base < t1; base += kMDTile) {
      const int m = (int)min((long long)kMDTile, t1 - base);
      __syncthreads();      // the previous tile has been read
      for (int k = threadIdx.x; k < m; k += kNNThreads) {
        TriRec r;
#pragma unroll
        for (int c = 0; c < 9; ++c) r.v[c] = 0.f;
        r.ok = md_load_face(a, base + k, r.v) ? 1 : 0, r.id = (int)(base + k), r.pad = 0;
        tile[k] = r;
      }
      __syncthreads();
      if (searching && s == sc)
        for (int k = 0; k < m; ++k) {
          const TriRec r = tile[k];
          if (r.ok) md_offer_coords(r.v, r.id, P, one);
        }
    }
  }
  if (live) md_write(a, i, q, one.bestf);
}

// One thread per face: the box of the vertices of every candidate face of its scene.
__global__ __launch_bounds__(kNNThreads) void md_bounds_kernel(MDArgs a) {
  const long long f = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (f >= a.nt) return;
  const int s = nn_find_scene(a.tstart, a.nscene, a.nt, f);
  if (s < 0) return;
  float v[9];
  if (!md_load_face(a, f, v)) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float mn = fminf(fminf(v[k], v[3 + k]), v[6 + k]), mx = fmaxf(fmaxf(v[k], v[3 + k]), v[6 + k]);
    key_min(a.box + (size_t)s * 6 + k, nn_key(mn));
    key_min(a.box + (size_t)s * 6 + 3 + k, ~nn_key(mx));
  }
}

template <int FILL>
__global__ __launch_bounds__(kNNThreads) void md_cell_kernel(MDArgs a) {
  const long long f = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (f < a.nt) md_place_face<FILL>(a, f);
}

__global__ __launch_bounds__(kNNThreads) void md_grid_kernel(MDArgs a) {
  const long long i = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (i < a.nq) md_query_grid(a, i);
}

// ---------------------------------------------------------------------------------------------------------------- host
struct MDPlan {
  int method, g;              // resolved: MVD_NN_BRUTE or MVD_NN_GRID; cells per axis
  size_t ncell, chunks, nref;
  size_t off_nover, off_cells, off_blocks, off_refs, off_over, bytes;
};

// false: an argument is out of range (the caller says which)
static bool md_plan(size_t nf, int nscene, int method, int grid, MDPlan& p) {
  p = MDPlan{};
  if (nscene < 1 || nscene > 65535 || nf > 0x7fffffffull || method < MVD_NN_AUTO || method > MVD_NN_GRID || grid < 0 || grid > kMDMaxGrid) return false;
  const size_t per = nf / (size_t)nscene;
  p.method = method == MVD_NN_AUTO ? ((long long)per >= kMDGridMinFaces ? MVD_NN_GRID : MVD_NN_BRUTE) : method;
  if (nf == 0) p.method = MVD_NN_BRUTE;
  if (p.method == MVD_NN_BRUTE) return true;
  if (nf * (size_t)kMDRefs > 0x7fffffffull) return false;
  int g = grid;
  if (g == 0) {
    g = (int)fminf(fmaxf(floorf(sqrtf((float)per / kMDGridDivisor) + 0.5f), 1.f), (float)kMDMaxGrid);
    while (g > 1 && (unsigned long long)nscene * g * g * g > (1ull << 28)) --g;
  }
  if ((unsigned long long)nscene * g * g * g > 0x7fffffffull) return false;
  p.g = g;
  p.ncell = (size_t)nscene * g * g * g;
  p.chunks = (p.ncell + kChunk - 1) / kChunk;
  p.nref = nf * (size_t)kMDRefs;
  p.off_nover = up16((size_t)nscene * 6 * sizeof(unsigned));
  p.off_cells = p.off_nover + up16((size_t)nscene * sizeof(unsigned));
  p.off_blocks = p.off_cells + p.chunks * kChunk * sizeof(unsigned);
  p.off_refs = p.off_blocks + up16((p.chunks + 1) * sizeof(unsigned));
  p.off_over = p.off_refs + up16(p.nref * sizeof(int));
  p.bytes = p.off_over + up16(nf * sizeof(int));
  return true;
}

static void md_point_scratch(MDArgs& a, const MDPlan& p, void* scratch) {
  char* base = (char*)scratch;
  a.box = (unsigned*)base;
  a.nover = (unsigned*)(base + p.off_nover);
  a.cells = (unsigned*)(base + p.off_cells);
  a.blocks = (unsigned*)(base + p.off_blocks);
  a.refs = (int*)(base + p.off_refs);
  a.over = (int*)(base + p.off_over);
  a.nref = (long long)p.nref;
  a.g = p.g;
}

}  // namespace

extern "C" size_t mvd_nearest_on_mesh_scratch(size_t nf, int nscene, int method, int grid) {
  MDPlan p;
  return md_plan(nf, nscene, method, grid, p) ? p.bytes : 0;
}

extern "C" int mvd_nearest_on_mesh_stages(const float* query, const int* query_start, const float* vertices, const int* faces,
                                          const int* face_start, size_t nq, size_t nv, size_t nf, int nscene, int method, int grid, int* face,
                                          float* dist2, float* point, float* bary, int* region, float* normal, void* scratch,
                                          size_t scratch_bytes, int stages, mvd_stream_t stream) {
  const char* fn = stages == MVD_NN_ALL ? "mvd_nearest_on_mesh" : "mvd_nearest_on_mesh_stages";
  MVD_CHECK_ARG(stages >= 1 && stages <= MVD_NN_ALL, "%s: stages=%d outside [1, %d]", fn, stages, MVD_NN_ALL);
  MVD_CHECK_ARG(method >= MVD_NN_AUTO && method <= MVD_NN_GRID, "%s: method=%d (MVD_NN_AUTO, _BRUTE or _GRID)", fn, method);
  MVD_CHECK_ARG(grid >= 0 && grid <= kMDMaxGrid, "%s: grid=%d outside [0, %d]", fn, grid, kMDMaxGrid);
  MVD_CHECK_ARG(nscene >= 1 && nscene <= 65535, "%s: nscene=%d outside [1, 65535]", fn, nscene);
  MVD_CHECK_ARG(nq <= 0x7fffffffull && nv <= 0x7fffffffull && nf <= 0x7fffffffull, "%s: nq=%zu, nv=%zu, nf=%zu beyond 2^31 - 1", fn, nq, nv, nf);
  MVD_CHECK_ARG(query_start && face_start, "%s: null query_start or face_start", fn);
  MVD_CHECK_ARG(query || nq == 0, "%s: null query with nq=%zu", fn, nq);
  MVD_CHECK_ARG(faces || nf == 0, "%s: null faces with nf=%zu", fn, nf);
  MVD_CHECK_ARG(vertices || nv == 0, "%s: null vertices with nv=%zu", fn, nv);
  const uintptr_t low = (uintptr_t)query | (uintptr_t)query_start | (uintptr_t)vertices | (uintptr_t)faces | (uintptr_t)face_start |
                        (uintptr_t)face | (uintptr_t)dist2 | (uintptr_t)point | (uintptr_t)bary | (uintptr_t)region | (uintptr_t)normal;
  MVD_CHECK_ARG((low & 3) == 0, "%s: a pointer that is not 4-byte aligned", fn);
  MDPlan p;
  MVD_CHECK_ARG(md_plan(nf, nscene, method, grid, p),
                "%s: MVD_NN_GRID needs nscene * grid^3 <= 2^31 - 1 and nf * %d <= 2^31 - 1 (nscene=%d, grid=%d, nf=%zu)", fn, kMDRefs, nscene,
                grid, nf);
  MVD_CHECK_ARG(p.bytes == 0 || (scratch && scratch_bytes >= p.bytes && ((uintptr_t)scratch & 15) == 0),
                "%s: scratch of %zu bytes (needs %zu, 16-byte aligned)", fn, scratch_bytes, p.bytes);
  MDArgs a{};
  a.query = query, a.vertices = vertices, a.qstart = query_start, a.tstart = face_start, a.faces = faces;
  a.face = face, a.dist2 = dist2, a.point = point, a.bary = bary, a.region = region, a.normal = normal;
  a.nq = (long long)nq, a.nv = (long long)nv, a.nt = (long long)nf, a.nscene = nscene;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 threads(kNNThreads), per_query(cdiv((long)nq, kNNThreads));
  if (p.method == MVD_NN_GRID) {
    md_point_scratch(a, p, scratch);
    if (stages & MVD_NN_BUILD) {
      hipError_t e = hipMemsetAsync(a.box, 0xff, (size_t)nscene * 6 * sizeof(unsigned), st);
      if (e == hipSuccess) e = hipMemsetAsync(a.nover, 0, (size_t)nscene * sizeof(unsigned), st);
      if (e == hipSuccess) e = hipMemsetAsync(a.cells, 0, p.chunks * kChunk * sizeof(unsigned), st);
      MVD_CHECK_ARG(e == hipSuccess, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
      const dim3 per_face(cdiv((long)nf, kNNThreads));
      hipLaunchKernelGGL(md_bounds_kernel, per_face, threads, 0, st, a);
      hipLaunchKernelGGL(md_cell_kernel<0>, per_face, threads, 0, st, a);
      hipLaunchKernelGGL(chunk_sum_kernel, dim3((unsigned)p.chunks), threads, 0, st, a.cells, a.blocks);
      hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kCompactThreads), 0, st, a.blocks, (unsigned)p.chunks, a.blocks + p.chunks);
      hipLaunchKernelGGL(chunk_scan_kernel, dim3((unsigned)p.chunks), threads, 0, st, a.cells, a.blocks);
      hipLaunchKernelGGL(md_cell_kernel<1>, per_face, threads, 0, st, a);
    }
    if ((stages & MVD_NN_QUERY) && nq > 0) hipLaunchKernelGGL(md_grid_kernel, per_query, threads, 0, st, a);
  } else if ((stages & MVD_NN_QUERY) && nq > 0) {
    hipLaunchKernelGGL(md_brute_kernel, per_query, threads, 0, st, a);
  }
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int mvd_nearest_on_mesh(const float* query, const int* query_start, const float* vertices, const int* faces, const int* face_start,
                                   size_t nq, size_t nv, size_t nf, int nscene, int method, int grid, int* face, float* dist2, float* point,
                                   float* bary, int* region, float* normal, void* scratch, size_t scratch_bytes, mvd_stream_t stream) {
  return mvd_nearest_on_mesh_stages(query, query_start, vertices, faces, face_start, nq, nv, nf, nscene, method, grid, face, dist2, point,
                                    bary, region, normal, scratch, scratch_bytes, MVD_NN_ALL, stream);
}
