// What the searches over target POINTS share (nearest.hip: the nearest and the k nearest points; register.hip: the truncated cost of a
// pose hypothesis): the sorted record, the arguments of a search, THE distance, THE selection rule, the single best a query keeps and
// the visit of a range of cells.  One copy, so that a hypothesis is scored with the bits mvd_nearest_points gives.
#pragma once
#include "nn_grid.hpp"

namespace {

struct alignas(16) Rec {
  float x, y, z;
  int id;
};

struct NNArgs {
  const float *query, *target;
  const int *qstart, *tstart;
  int* index;
  float* dist2;
  Rec* sorted;                                        // nt records, cell after cell
  unsigned* box;                                      // per scene: keys of min x, y, z, then ~keys of max x, y, z (both under atomicMin)
  unsigned* cells;                                    // nscene * g^3 words padded to kChunk: counts -> begins -> ends
  unsigned* blocks;                                   // one word per chunk, and the total behind them
  long long nq, nt;
  int nscene, g;
  int k;                                              // mvd_knn_points: neighbours per query (index, dist2 are (nq, k)); unused by the others
};

// THE distance of the header, in its order
NN_HD float nn_d2(float qx, float qy, float qz, float tx, float ty, float tz) {
  const float dx = qx - tx, dy = qy - ty, dz = qz - tz;
  return (dx * dx + dy * dy) + dz * dz;
}
// THE selection rule of the header
NN_HD void nn_take(float d2, int j, float& best, int& bestj) {
  if (d2 < best || (d2 == best && j < bestj)) best = d2, bestj = j;      // (bestj = -1 with best = +inf: an infinite d2 never wins)
}

// What a search keeps per query.  take() offers a candidate; worst() is the distance the shell walk holds against its bound.
struct NNOne {
  float best = INFINITY;
  int bestj = -1;
  NN_HD void take(float d2, int j) { nn_take(d2, j, best, bestj); }
  NN_HD float worst() const { return best; }
};

// The records of the cells [ca, cb] of scene s (local ids, ca <= cb: consecutive cells own consecutive records) against the query.
template <class Keep>
NN_HD void nn_visit(const NNArgs& a, long long scene_cell0, long long ca, long long cb, long long t0, long long t1, float qx, float qy, float qz,
                    Keep& keep) {
  const long long first = scene_cell0 + ca, last = scene_cell0 + cb;
  const long long begin = nn_clamp(first > 0 ? (long long)a.cells[first - 1] : 0ll, a.nt), end = nn_clamp((long long)a.cells[last], a.nt);
  for (long long k = begin; k < end; ++k) {
    const Rec r = a.sorted[k];
    if (r.id >= t0 && r.id < t1) keep.take(nn_d2(qx, qy, qz, r.x, r.y, r.z), r.id);
  }
}

}  // namespace

// The grid of a call as nearest.hip's host code plans it (defined there, beside the constants it comes from): the method MVD_NN_AUTO
// resolves to, the cells per axis, where box and cells lie in the scratch behind the sorted records, and the scratch's size.
// false: an argument is out of range.
struct NNLayout {
  int method, g;
  size_t off_box, off_cells, bytes;
};
bool nn_points_layout(size_t nt, int nscene, int method, int grid, NNLayout* out);
