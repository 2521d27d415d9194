// The generalized winding number of a triangle mesh at every query point (include/mvd_hip.h: mvd_winding_number has the rule in full).
//
// PER PAIR (wn_omega): the signed solid angle of a face seen from the query by Van Oosterom and Strackee's formula, fp64 on exact
// conversions of the fp32 inputs, compiled without contraction, in the order of the header.
// EXACT: one thread per query; the workgroup walks the scenes its queries belong to and stages each scene's faces through LDS in tiles of
// kWFaceTile RESOLVED records (nine coordinates and the candidate flag: 40 bytes), as md_brute_kernel does.  Every lane reads the same
// record at once: a broadcast.  The sum runs in ascending face row, so it does not depend on the launch geometry.
// CELLS, build: wn_bounds_kernel (the box of the vertices of every scene's candidate faces: nn_key under atomicMin) -> assign + count
// (a face belongs to the cell of its centroid; an integer atomic per face) -> the occupied flag per dense cell -> the exclusive scan of
// nn_grid.hpp over the counts (the begins of the member lists) and over the flags (the rank of a cell among the occupied ones) -> the
// member range and the cursor of every occupied cell -> fill (an integer atomic hands out the slot: arrival order) -> rank (every face
// counts the smaller rows of its own list and stores its RESOLVED 36-byte record at that position: the ordered list does not depend on
// the arrival order) -> per occupied cell, one thread, the moments over its ascending members.
// CELLS, query: the occupied-cell records of the scene (centre, dipole, radius, member range: 64 bytes) staged through LDS in tiles of
// kWCellTile and broadcast; a far cell costs one division and one square root, a near cell walks its resolved records from global
// memory: one dependent load per face.
// Integer atomics only; every fp64 sum runs in list order.  Everything read back from the scratch is clamped or range-checked before it
// addresses anything, so MVD_NN_QUERY on a scratch it did not build reads nothing out of bounds.
// The per-pair function, the candidate test, the cell assignment and the moments are host-and-device functions: tools/winding_host.hip
// runs them serially on a CPU (under the sanitizers), cells against exact.
//
// Not tried: a tree or several levels of cells, a quadrupole term, an fp32 pre-test of far faces, more than one thread per cell's
// moments, sorting the queries by cell (DESIGN.md has the section).
#include "mesh_common.hpp"

namespace {

constexpr int kWFaceTile = MVD_WIND_FACE_TILE;        // resolved records per LDS tile of the exact kernel (20 KB)
constexpr int kWCellTile = MVD_WIND_CELL_TILE;        // occupied-cell records per LDS tile of the cells query (8 KB)
constexpr int kWMaxCells = MVD_WIND_MAX_CELLS;
constexpr size_t kWMaxTable = (size_t)1 << 28;        // nscene * cells^3, that of the mesh simplification
// MVD_WIND_AUTO: the cells from this many faces per scene upward; cells = 0: (kWCellsFactor * faces per scene)^(1/4).  INTERFACE
// defaults from a cost model, not from a sweep: a surface occupies ~4 c^2 of its c^3 cells, beta = 2 makes the ~26 cells around a query
// near, and a near face costs about five far cells, so the cost 4 c^2 + 26 * 5 * nf / (4 c^2) is least at c^4 ~ 8 nf.
constexpr long long kWCellsMinFaces = 1024;
constexpr double kWCellsFactor = 8.0;
constexpr double kWFourPi = 4.0 * 3.141592653589793;

struct alignas(8) WCell {
  double p[3], N[3], rho2;
  unsigned begin, end;
};
static_assert(sizeof(WCell) == 64, "an occupied-cell record is 64 bytes");

struct WArgs {
  const float *query, *vertices;
  const int *qstart, *fstart, *faces;
  double* winding;
  unsigned char* inside;
  unsigned* box;                                      // per scene: keys of min x, y, z, then ~keys of max x, y, z
  unsigned* count;                                    // table + 1 words padded to whole chunks: members per cell -> begins
  unsigned* occ;                                      // the same shape: 1 for an occupied cell -> its rank among the occupied cells
  unsigned* cursor;                                   // per occupied cell: the next free slot of its list while it is filled
  int* face_cell;                                     // per face: its word of the dense table, -1 for a face that is no candidate
  int* unsorted;                                      // the member lists in arrival order
  WCell* cell;                                        // per occupied cell, ascending (scene, cell id)
  float* rec;                                         // nine coordinates per member, cell after cell, ascending face row in a cell
  long long nq, nv, nf, c3, table, ncell;             // c3: cells^3; table: nscene * c3; ncell: the most occupied cells, min(table, nf)
  int nscene, cells;
  double bb;                                          // beta * beta
};

// ---------------------------------------------------------------------------------------------------------------- per pair
NN_HD double wn_dot(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// n = (B - A) x (C - A) as md_closest forms it: one subtraction of two products per component
NN_HD void wn_normal(const float* v, double* n) {
  const double ab[3] = {(double)v[3] - (double)v[0], (double)v[4] - (double)v[1], (double)v[5] - (double)v[2]};
  const double ac[3] = {(double)v[6] - (double)v[0], (double)v[7] - (double)v[1], (double)v[8] - (double)v[2]};
  n[0] = ab[1] * ac[2] - ab[2] * ac[1], n[1] = ab[2] * ac[0] - ab[0] * ac[2], n[2] = ab[0] * ac[1] - ab[1] * ac[0];
}

// The nine coordinates of face f.  false: not a candidate (an id outside [0, nv), a coordinate that is not finite, a normal of exactly 0).
NN_HD bool wn_load_face(const WArgs& a, long long f, float* v) {
  const int i0 = a.faces[f * 3 + 0], i1 = a.faces[f * 3 + 1], i2 = a.faces[f * 3 + 2];
  if (i0 < 0 || i0 >= a.nv || i1 < 0 || i1 >= a.nv || i2 < 0 || i2 >= a.nv) return false;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    v[k] = a.vertices[(long long)i0 * 3 + k], v[3 + k] = a.vertices[(long long)i1 * 3 + k], v[6 + k] = a.vertices[(long long)i2 * 3 + k];
    ok = ok && nn_finite(v[k]) && nn_finite(v[3 + k]) && nn_finite(v[6 + k]);
  }
  if (!ok) return false;
  double n[3];
  wn_normal(v, n);
  return !(n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0);
}

// Omega of the header: the signed solid angle of the face v (A, B, C) seen from q.
NN_HD double wn_omega(const double* q, const float* v) {
  const double a[3] = {(double)v[0] - q[0], (double)v[1] - q[1], (double)v[2] - q[2]};
  const double b[3] = {(double)v[3] - q[0], (double)v[4] - q[1], (double)v[5] - q[2]};
  const double c[3] = {(double)v[6] - q[0], (double)v[7] - q[1], (double)v[8] - q[2]};
  const double la = sqrt(wn_dot(a, a)), lb = sqrt(wn_dot(b, b)), lc = sqrt(wn_dot(c, c));
  const double x[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
  const double num = wn_dot(a, x);
  const double den = (((la * lb) * lc + wn_dot(a, b) * lc) + wn_dot(b, c) * la) + wn_dot(c, a) * lb;
  if (num == 0.0) return 0.0;      // the query in the face's plane: no sign of zero to argue about
  return 2.0 * atan2(num, den);
}

// ---------------------------------------------------------------------------------------------------------------- cells: the grid
// A scene's grid from its box of keys, by the fp64 expressions the mesh simplification uses.
struct WGrid {
  double lo[3], h;
  int n[3];
};
NN_HD WGrid wn_grid(const unsigned* box, int cells) {
  WGrid G;
  double ext[3], big = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    G.lo[a] = (double)nn_unkey(box[a]);
    ext[a] = (double)nn_unkey(~box[3 + a]) - G.lo[a];
    big = ext[a] > big ? ext[a] : big;      // (a NaN -- the box of a scene without a candidate -- leaves 0)
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
NN_HD int wn_cell(const WGrid& G, int a, double x) {
  if (!(G.h > 0.0)) return 0;
  double u = floor((x - G.lo[a]) / G.h);
  u = u >= 0.0 ? u : 0.0;                                   // (a NaN to 0)
  const double top = (double)(G.n[a] - 1);
  return (int)(u > top ? top : u);
}
// the centroid g = ((A + B) + C) / 3 per axis
NN_HD void wn_centroid(const float* v, double* g) {
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] = (((double)v[k] + (double)v[3 + k]) + (double)v[6 + k]) / 3.0;
}
// the word of candidate face v of scene s in the dense table: s cells^3 + (iz n_y + iy) n_x + ix
NN_HD long long wn_word(const WArgs& a, int s, const float* v) {
  const WGrid G = wn_grid(a.box + (size_t)s * 6, a.cells);
  double g[3];
  wn_centroid(v, g);
  const int ix = wn_cell(G, 0, g[0]), iy = wn_cell(G, 1, g[1]), iz = wn_cell(G, 2, g[2]);
  return (long long)s * a.c3 + ((long long)iz * G.n[1] + iy) * G.n[0] + ix;
}

// The moments of an occupied cell from its resolved member records rec[b .. e), ascending: p, N and rho2 of the header.
NN_HD void wn_moments(const float* rec, long long b, long long e, WCell& c) {
  double M = 0.0, sg[3] = {0.0, 0.0, 0.0}, sn[3] = {0.0, 0.0, 0.0};
  for (long long k = b; k < e; ++k) {
    const float* v = rec + k * 9;
    double n[3], g[3];
    wn_normal(v, n);
    wn_centroid(v, g);
    const double m = sqrt(wn_dot(n, n));
    M += m;
#pragma unroll
    for (int x = 0; x < 3; ++x) sg[x] += m * g[x], sn[x] += n[x];
  }
#pragma unroll
  for (int x = 0; x < 3; ++x) c.p[x] = sg[x] / M, c.N[x] = 0.5 * sn[x];
  double rho2 = 0.0;
  for (long long k = b; k < e; ++k)
    for (int j = 0; j < 3; ++j) {
      const float* X = rec + k * 9 + j * 3;
      const double d[3] = {(double)X[0] - c.p[0], (double)X[1] - c.p[1], (double)X[2] - c.p[2]};
      const double r = wn_dot(d, d);
      rho2 = r > rho2 ? r : rho2;
    }
  c.rho2 = rho2;
}

// The member range of an occupied-cell record, clamped into the records.
NN_HD void wn_members(const WCell& c, long long nf, long long& b, long long& e) {
  b = nn_clamp((long long)c.begin, nf), e = nn_clamp((long long)c.end, nf);
  if (e < b) e = b;
}

// One cell's contribution to S for the query q.
NN_HD double wn_cell_term(const WArgs& a, const WCell& c, const double* q) {
  const double d[3] = {c.p[0] - q[0], c.p[1] - q[1], c.p[2] - q[2]};
  const double r2 = wn_dot(d, d);
  if (r2 > a.bb * c.rho2) return wn_dot(c.N, d) / (r2 * sqrt(r2));      // FAR: the dipole of the cell
  long long b, e;
  wn_members(c, a.nf, b, e);
  double t = 0.0;
  for (long long k = b; k < e; ++k) t += wn_omega(q, a.rec + k * 9);
  return t;
}

// Both outputs of query i.  `valid`: finite and of a scene.  A NULL output is not written.
NN_HD void wn_write(const WArgs& a, long long i, bool valid, double S) {
  const double w = valid ? S / kWFourPi : (double)__builtin_nanf("");
  if (a.winding) a.winding[i] = w;
  if (a.inside) a.inside[i] = w >= 0.5 ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------- kernels
struct alignas(8) WFaceRec {
  float v[9];
  int ok;
};

// What the two query kernels share: the query, its scene and the scenes of the workgroup.
struct WQuery {
  long long i;
  bool live, valid;
  int s, s_lo, s_hi;
  double q[3];
};
__device__ __forceinline__ WQuery wn_query(const WArgs& a, int* span) {
  WQuery Q;
  Q.i = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  Q.live = Q.i < a.nq;
  Q.s = Q.live ? nn_find_scene(a.qstart, a.nscene, a.nq, Q.i) : -1;
  if (threadIdx.x == 0) span[0] = a.nscene, span[1] = -1;
  __syncthreads();
  if (Q.s >= 0) atomicMin(&span[0], Q.s), atomicMax(&span[1], Q.s);
  __syncthreads();
  Q.s_lo = span[0], Q.s_hi = span[1];      // (uniform: the scenes this workgroup's queries belong to)
  float q[3] = {0.f, 0.f, 0.f};
  if (Q.live) q[0] = a.query[Q.i * 3 + 0], q[1] = a.query[Q.i * 3 + 1], q[2] = a.query[Q.i * 3 + 2];
  Q.valid = Q.s >= 0 && nn_finite(q[0]) && nn_finite(q[1]) && nn_finite(q[2]);
  Q.q[0] = (double)q[0], Q.q[1] = (double)q[1], Q.q[2] = (double)q[2];
  return Q;
}

__global__ __launch_bounds__(kNNThreads) void wn_exact_kernel(WArgs a) {
  __shared__ WFaceRec tile[kWFaceTile];
  __shared__ int span[2];
  const WQuery Q = wn_query(a, span);
  double S = 0.0;
  for (int sc = Q.s_lo; sc <= Q.s_hi; ++sc) {
    const long long t0 = nn_clamp(a.fstart[sc], a.nf), t1 = nn_clamp(a.fstart[sc + 1], a.nf);
    for (long long base = t0; base < t1; base += kWFaceTile) {
      const int m = (int)min((long long)kWFaceTile, t1 - base);
      __syncthreads();      // the previous tile has been read
      for (int k = threadIdx.x; k < m; k += kNNThreads) {
        WFaceRec r;
#pragma unroll
        for (int c = 0; c < 9; ++c) r.v[c] = 0.f;
        r.ok = wn_load_face(a, base + k, r.v) ? 1 : 0;
        tile[k] = r;
      }
      __syncthreads();
      if (Q.valid && Q.s == sc)
        for (int k = 0; k < m; ++k) {
          const WFaceRec r = tile[k];
          if (r.ok) S += wn_omega(Q.q, r.v);
        }
    }
  }
  if (Q.live) wn_write(a, Q.i, Q.valid, S);
}

__global__ __launch_bounds__(kNNThreads) void wn_cells_kernel(WArgs a) {
  __shared__ WCell tile[kWCellTile];
  __shared__ int span[2];
  const WQuery Q = wn_query(a, span);
  double S = 0.0;
  for (int sc = Q.s_lo; sc <= Q.s_hi; ++sc) {
    // the scene's occupied cells: the ranks of its first dense word and of the next scene's
    const long long r0 = nn_clamp((long long)a.occ[(long long)sc * a.c3], a.ncell), r1 = nn_clamp((long long)a.occ[(long long)(sc + 1) * a.c3], a.ncell);
    for (long long base = r0; base < r1; base += kWCellTile) {
      const int m = (int)min((long long)kWCellTile, r1 - base);
      __syncthreads();      // the previous tile has been read
      for (int k = threadIdx.x; k < m; k += kNNThreads) tile[k] = a.cell[base + k];
      __syncthreads();
      if (Q.valid && Q.s == sc)
        for (int k = 0; k < m; ++k) {
          const WCell c = tile[k];
          S += wn_cell_term(a, c, Q.q);
        }
    }
  }
  if (Q.live) wn_write(a, Q.i, Q.valid, S);
}

// One thread per face: the box of the vertices of every candidate face of its scene.
__global__ __launch_bounds__(kNNThreads) void wn_bounds_kernel(WArgs a) {
  const long long f = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (f >= a.nf) return;
  const int s = nn_find_scene(a.fstart, a.nscene, a.nf, f);
  if (s < 0) return;
  float v[9];
  if (!wn_load_face(a, f, v)) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float mn = fminf(fminf(v[k], v[3 + k]), v[6 + k]), mx = fmaxf(fmaxf(v[k], v[3 + k]), v[6 + k]);
    key_min(a.box + (size_t)s * 6 + k, nn_key(mn));
    key_min(a.box + (size_t)s * 6 + 3 + k, ~nn_key(mx));
  }
}

// One thread per face: its word of the dense table (-1: no candidate), counted there.
__global__ __launch_bounds__(kNNThreads) void wn_assign_kernel(WArgs a) {
  const long long f = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (f >= a.nf) return;
  const int s = nn_find_scene(a.fstart, a.nscene, a.nf, f);
  float v[9];
  long long w = -1;
  if (s >= 0 && wn_load_face(a, f, v)) w = wn_word(a, s, v);
  if (w >= a.table) w = -1;                                 // (never: a cell index is clamped into the scene's grid)
  a.face_cell[f] = (int)w;
  if (w >= 0) atomicAdd(a.count + w, 1u);
}

// One thread per dense word, before the scans: the occupied flag.
__global__ __launch_bounds__(kNNThreads) void wn_flag_kernel(WArgs a) {
  const long long w = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (w < a.table) a.occ[w] = a.count[w] ? 1u : 0u;
}

// One thread per dense word, after the scans: the member range and the cursor of every occupied cell.
__global__ __launch_bounds__(kNNThreads) void wn_ranges_kernel(WArgs a) {
  const long long w = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (w >= a.table) return;
  const unsigned b = a.count[w], e = a.count[w + 1];
  if (e <= b) return;
  const long long r = a.occ[w];
  if (r >= a.ncell) return;                                 // (never: an occupied cell has a member, and there are nf members at most)
  a.cursor[r] = b;
  a.cell[r].begin = b, a.cell[r].end = e;
}

// The word and the list of candidate face f as the scratch holds them; false for a face that is in no list.
NN_HD bool wn_list_of(const WArgs& a, long long f, long long& r, long long& b, long long& e) {
  const long long w = a.face_cell[f];
  if (w < 0 || w >= a.table) return false;
  r = a.occ[w];
  b = nn_clamp((long long)a.count[w], a.nf), e = nn_clamp((long long)a.count[w + 1], a.nf);
  return r < a.ncell && b < e;
}

__global__ __launch_bounds__(kNNThreads) void wn_fill_kernel(WArgs a) {
  const long long f = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (f >= a.nf) return;
  long long r, b, e;
  if (!wn_list_of(a, f, r, b, e)) return;
  const long long at = atomicAdd(a.cursor + r, 1u);
  if (at < a.nf) a.unsorted[at] = (int)f;
}

// A member's position in its ordered list is the number of smaller rows in the list: O(list) reads, one resolved record stored.
__global__ __launch_bounds__(kNNThreads) void wn_rank_kernel(WArgs a) {
  const long long f = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (f >= a.nf) return;
  long long r, b, e, below = 0;
  if (!wn_list_of(a, f, r, b, e)) return;
  for (long long k = b; k < e; ++k) below += a.unsorted[k] < f ? 1 : 0;
  float v[9];
  if (b + below >= e || !wn_load_face(a, f, v)) return;
#pragma unroll
  for (int k = 0; k < 9; ++k) a.rec[(b + below) * 9 + k] = v[k];
}

// One thread per occupied cell: its moments.
__global__ __launch_bounds__(kNNThreads) void wn_moment_kernel(WArgs a) {
  const long long r = (long long)blockIdx.x * kNNThreads + threadIdx.x;
  if (r >= nn_clamp((long long)a.occ[a.table], a.ncell)) return;
  WCell c = a.cell[r];
  long long b, e;
  wn_members(c, a.nf, b, e);
  wn_moments(a.rec, b, e, c);
  a.cell[r] = c;
}

// ---------------------------------------------------------------------------------------------------------------- host
struct WPlan {
  int method, cells;          // resolved: MVD_WIND_EXACT or MVD_WIND_CELLS; cells per axis
  size_t table, ncell;
  size_t off_count, off_occ, off_cursor, off_face_cell, off_unsorted, off_cell, off_rec, bytes;      // the boxes at 0
};

static bool wn_sizes_ok(size_t nf, int nscene, int method, int cells) {
  return nscene >= 1 && nscene <= 65535 && nf <= 0x7fffffffull && method >= MVD_WIND_AUTO && method <= MVD_WIND_CELLS && cells >= 0 &&
         cells <= kWMaxCells;
}

// false: an argument is out of range (the caller says which)
static bool wn_plan(size_t nf, int nscene, int method, int cells, WPlan& p) {
  p = WPlan{};
  if (!wn_sizes_ok(nf, nscene, method, cells)) return false;
  const size_t per = nf / (size_t)nscene;
  p.method = method == MVD_WIND_AUTO ? ((long long)per >= kWCellsMinFaces ? MVD_WIND_CELLS : MVD_WIND_EXACT) : method;
  if (nf == 0) p.method = MVD_WIND_EXACT;
  if (p.method == MVD_WIND_EXACT) return true;
  int c = cells;
  if (c == 0) {
    c = (int)fmin(fmax(floor(sqrt(sqrt(kWCellsFactor * (double)per)) + 0.5), 1.0), (double)kWMaxCells);
    while (c > 1 && (size_t)nscene * c * c * c > kWMaxTable) --c;
  }
  if ((size_t)nscene * c * c * c > kWMaxTable) return false;
  p.cells = c;
  p.table = (size_t)nscene * c * c * c;
  p.ncell = p.table < nf ? p.table : nf;
  p.off_count = up16((size_t)nscene * 6 * sizeof(unsigned));
  p.off_occ = p.off_count + mt_scan_bytes(p.table);
  p.off_cursor = p.off_occ + mt_scan_bytes(p.table);
  p.off_face_cell = p.off_cursor + up16(p.ncell * sizeof(unsigned));
  p.off_unsorted = p.off_face_cell + up16(nf * sizeof(int));
  p.off_cell = p.off_unsorted + up16(nf * sizeof(int));
  p.off_rec = p.off_cell + p.ncell * sizeof(WCell);
  p.bytes = p.off_rec + up16(nf * 9 * sizeof(float));
  return true;
}

static void wn_point_scratch(WArgs& a, const WPlan& p, void* scratch) {
  char* base = (char*)scratch;
  a.box = (unsigned*)base;
  a.count = (unsigned*)(base + p.off_count);
  a.occ = (unsigned*)(base + p.off_occ);
  a.cursor = (unsigned*)(base + p.off_cursor);
  a.face_cell = (int*)(base + p.off_face_cell);
  a.unsorted = (int*)(base + p.off_unsorted);
  a.cell = (WCell*)(base + p.off_cell);
  a.rec = (float*)(base + p.off_rec);
  a.cells = p.cells;
  a.c3 = (long long)p.cells * p.cells * p.cells;
  a.table = (long long)p.table, a.ncell = (long long)p.ncell;
}

}  // namespace

extern "C" size_t mvd_winding_scratch(size_t nf, int nscene, int method, int cells) {
  WPlan p;
  return wn_plan(nf, nscene, method, cells, p) ? p.bytes : 0;
}

extern "C" int mvd_winding_number_stages(const float* query, const int* query_start, const float* vertices, const int* faces, const int* face_start,
                                         size_t nq, size_t nv, size_t nf, int nscene, int method, int cells, double beta, double* winding,
                                         unsigned char* inside, void* scratch, size_t scratch_bytes, int stages, mvd_stream_t stream) {
  const char* fn = stages == MVD_NN_ALL ? "mvd_winding_number" : "mvd_winding_number_stages";
  MVD_CHECK_ARG(stages >= 1 && stages <= MVD_NN_ALL, "%s: stages=%d outside [1, %d]", fn, stages, MVD_NN_ALL);
  MVD_CHECK_ARG(method >= MVD_WIND_AUTO && method <= MVD_WIND_CELLS, "%s: method=%d (MVD_WIND_AUTO, _EXACT or _CELLS)", fn, method);
  MVD_CHECK_ARG(cells >= 0 && cells <= kWMaxCells, "%s: cells=%d outside [0, %d]", fn, cells, kWMaxCells);
  MVD_CHECK_ARG(beta >= 0.0, "%s: beta=%g is neither >= 0 nor +inf", fn, beta);      // (a NaN compares false)
  MVD_CHECK_ARG(nscene >= 1 && nscene <= 65535, "%s: nscene=%d outside [1, 65535]", fn, nscene);
  MVD_CHECK_ARG(nq <= 0x7fffffffull && nv <= 0x7fffffffull && nf <= 0x7fffffffull, "%s: nq=%zu, nv=%zu, nf=%zu beyond 2^31 - 1", fn, nq, nv, nf);
  MVD_CHECK_ARG(query_start && face_start, "%s: null query_start or face_start", fn);
  MVD_CHECK_ARG(query || nq == 0, "%s: null query with nq=%zu", fn, nq);
  MVD_CHECK_ARG(faces || nf == 0, "%s: null faces with nf=%zu", fn, nf);
  MVD_CHECK_ARG(vertices || nv == 0, "%s: null vertices with nv=%zu", fn, nv);
  const uintptr_t low = (uintptr_t)query | (uintptr_t)query_start | (uintptr_t)vertices | (uintptr_t)faces | (uintptr_t)face_start;
  MVD_CHECK_ARG((low & 3) == 0 && ((uintptr_t)winding & 7) == 0, "%s: a pointer that is not 4-byte aligned (winding: 8-byte)", fn);
  WPlan p;
  MVD_CHECK_ARG(wn_plan(nf, nscene, method, cells, p), "%s: MVD_WIND_CELLS needs nscene * cells^3 <= 2^28 (nscene=%d, cells=%d)", fn, nscene, cells);
  MVD_CHECK_ARG(p.bytes == 0 || (scratch && scratch_bytes >= p.bytes && ((uintptr_t)scratch & 15) == 0),
                "%s: scratch of %zu bytes (needs %zu, 16-byte aligned)", fn, scratch_bytes, p.bytes);
  WArgs a{};
  a.query = query, a.vertices = vertices, a.qstart = query_start, a.fstart = face_start, a.faces = faces;
  a.winding = winding, a.inside = inside;
  a.nq = (long long)nq, a.nv = (long long)nv, a.nf = (long long)nf, a.nscene = nscene;
  a.bb = beta * beta;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 threads(kNNThreads), per_query(cdiv((long)nq, kNNThreads));
  if (p.method == MVD_WIND_CELLS) {
    wn_point_scratch(a, p, scratch);
    if (stages & MVD_NN_BUILD) {
      hipError_t e = hipMemsetAsync(a.box, 0xff, (size_t)nscene * 6 * sizeof(unsigned), st);
      if (e == hipSuccess) e = hipMemsetAsync(a.count, 0, mt_chunks(p.table) * kChunk * sizeof(unsigned), st);
      if (e == hipSuccess) e = hipMemsetAsync(a.occ, 0, mt_chunks(p.table) * kChunk * sizeof(unsigned), st);
      MVD_CHECK_ARG(e == hipSuccess, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
      const dim3 per_face = mt_grid(nf), per_word = mt_grid(p.table);
      hipLaunchKernelGGL(wn_bounds_kernel, per_face, threads, 0, st, a);
      hipLaunchKernelGGL(wn_assign_kernel, per_face, threads, 0, st, a);
      hipLaunchKernelGGL(wn_flag_kernel, per_word, threads, 0, st, a);
      mt_scan(a.count, p.table, st);
      mt_scan(a.occ, p.table, st);
      hipLaunchKernelGGL(wn_ranges_kernel, per_word, threads, 0, st, a);
      hipLaunchKernelGGL(wn_fill_kernel, per_face, threads, 0, st, a);
      hipLaunchKernelGGL(wn_rank_kernel, per_face, threads, 0, st, a);
      hipLaunchKernelGGL(wn_moment_kernel, mt_grid(p.ncell), threads, 0, st, a);
    }
    if ((stages & MVD_NN_QUERY) && nq > 0) hipLaunchKernelGGL(wn_cells_kernel, per_query, threads, 0, st, a);
  } else if ((stages & MVD_NN_QUERY) && nq > 0) {
    hipLaunchKernelGGL(wn_exact_kernel, per_query, threads, 0, st, a);
  }
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int mvd_winding_number(const float* query, const int* query_start, const float* vertices, const int* faces, const int* face_start,
                                  size_t nq, size_t nv, size_t nf, int nscene, int method, int cells, double beta, double* winding,
                                  unsigned char* inside, void* scratch, size_t scratch_bytes, mvd_stream_t stream) {
  return mvd_winding_number_stages(query, query_start, vertices, faces, face_start, nq, nv, nf, nscene, method, cells, beta, winding, inside,
                                   scratch, scratch_bytes, MVD_NN_ALL, stream);
}
