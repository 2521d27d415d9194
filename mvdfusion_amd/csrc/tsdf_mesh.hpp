// Marching tetrahedra on the TSDF lattice (include/mvd_hip.h: mvd_mesh_count, mvd_mesh_emit): the combinatorics shared by the counting and
// the emitting kernels of tsdf.hip -- lattice edges, the six Kuhn tetrahedra of a cell and the triangles of one tetrahedron.  Plain integer
// functions without any device intrinsic, so a host compiler can run them too.
#pragma once

#ifndef MVD_HD
#ifdef __HIPCC__
#define MVD_HD __host__ __device__ __forceinline__
#else
#define MVD_HD inline
#endif
#endif

namespace {

// A lattice offset is a bit mask: bit 0 = x + 1, bit 1 = y + 1, bit 2 = z + 1.
// The 7 edge directions a corner owns, (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1), as masks: 1 2 4 3 5 6 7.
constexpr int kMeshDirs = 7;
MVD_HD int mesh_dir_mask(int dir) { return (int)((0x7653421u >> (4 * dir)) & 7u); }
MVD_HD int mesh_mask_dir(int mask) { return (int)((0x65423100u >> (4 * mask)) & 7u); }      // the inverse, for masks 1 .. 7

// Tetrahedron q of a cell: the axis permutation (a, b, c) in lexicographic order xyz xzy yxz yzx zxy zyx; corners v0, v0 + e_a,
// v0 + e_a + e_b, v0 + (1,1,1) -- a chain of masks, so every edge of a tetrahedron is a lattice edge owned by its lower corner.
// Four bits per corner, corner 0 lowest.
MVD_HD int tet_corner_mask(int q, int c) {
  const unsigned packed = q == 0 ? 0x7310u : q == 1 ? 0x7510u : q == 2 ? 0x7320u : q == 3 ? 0x7620u : q == 4 ? 0x7540u : 0x7640u;
  return (int)((packed >> (4 * c)) & 7u);
}
// sign of det[c1 - c0, c2 - c0, c3 - c0]: the parity of the permutation
MVD_HD int tet_sign(int q) { return (0x19u >> q) & 1u ? 1 : -1; }      // + - - + + -

// slot of the edge between corners a < b of a tetrahedron: 01 02 03 12 13 23
MVD_HD int tet_edge_slot(int a, int b) { return a == 0 ? b - 1 : a + b; }

MVD_HD int lowest4(unsigned m) { return m & 1u ? 0 : m & 2u ? 1 : m & 4u ? 2 : 3; }
MVD_HD int popcount4(unsigned m) { return (int)((m & 1u) + ((m >> 1) & 1u) + ((m >> 2) & 1u) + ((m >> 3) & 1u)); }

// triangles of a tetrahedron whose four corners are observed: 0, 1 or 2 from its inside mask (bit c = corner c inside)
MVD_HD int tet_triangle_count(unsigned inside) {
  const int n = popcount4(inside);
  return n == 0 || n == 4 ? 0 : n == 2 ? 2 : 1;
}

MVD_HD int pick6(const int* id, int slot) {      // id[slot] without a run-time index
  return slot == 0 ? id[0] : slot == 1 ? id[1] : slot == 2 ? id[2] : slot == 3 ? id[3] : slot == 4 ? id[4] : id[5];
}
MVD_HD int tet_edge_id(const int* id, int a, int b) { return a < b ? pick6(id, tet_edge_slot(a, b)) : pick6(id, tet_edge_slot(b, a)); }

// The triangles of one tetrahedron.  inside: bit c = corner c inside; sign: tet_sign; id[6]: the vertex ids on its edges by slot (only
// the crossing edges are read).  Writes tet_triangle_count(inside) triangles of 3 ids to f and returns the count.
//   The corners are put in the order o = (lone side ascending, other side ascending), the lone side being the inside corners when one or
//   two are inside and the outside corner when three are.  With one corner p alone the triangle (pq, pr, pt) has its normal away from p
//   iff (p, q, r, t) is positively oriented; with p, q against r, t the quad (pr, pt, qt, qr) has its normal towards r, t under the same
//   condition.  The orientation of o is `sign` times the parity of o as a permutation; three inside turns the result around.
//   Every triangle starts at its smallest id; a quad is cut along the diagonal through its smallest id m: with the wound quad rotated to
//   (m, n1, n2, n3) the FIRST triangle is (m, n1, n2), the second (m, n2, n3).
MVD_HD int tet_triangles(unsigned inside, int sign, const int* id, int* f) {
  const int n = popcount4(inside);
  if (n == 0 || n == 4) return 0;
  const unsigned lone = n == 3 ? (~inside & 15u) : inside;
  unsigned a = lone, b = ~lone & 15u;
  const int o0 = lowest4(a);
  a &= a - 1u;
  int o1, o2, o3;
  if (n == 2) {
    o1 = lowest4(a);
    o2 = lowest4(b);
    b &= b - 1u;
  } else {
    o1 = lowest4(b);
    b &= b - 1u;
    o2 = lowest4(b);
    b &= b - 1u;
  }
  o3 = lowest4(b);
  const int inversions = (o0 > o1) + (o0 > o2) + (o0 > o3) + (o1 > o2) + (o1 > o3) + (o2 > o3);
  bool positive = (sign > 0) == ((inversions & 1) == 0);
  if (n == 3) positive = !positive;
  if (n != 2) {
    int t0 = tet_edge_id(id, o0, o1), t1 = tet_edge_id(id, o0, o2), t2 = tet_edge_id(id, o0, o3);
    if (!positive) {
      const int s = t1;
      t1 = t2;
      t2 = s;
    }
    // rotate the smallest id to the front
    if (t1 < t0 && t1 < t2) {
      const int s = t0;
      t0 = t1, t1 = t2, t2 = s;
    } else if (t2 < t0 && t2 < t1) {
      const int s = t0;
      t0 = t2, t2 = t1, t1 = s;
    }
    f[0] = t0, f[1] = t1, f[2] = t2;
    return 1;
  }
  int q0 = tet_edge_id(id, o0, o2), q1 = tet_edge_id(id, o0, o3), q2 = tet_edge_id(id, o1, o3), q3 = tet_edge_id(id, o1, o2);
  if (!positive) {
    const int s = q1;
    q1 = q3;
    q3 = s;
  }
  for (int r = 0; r < 3; ++r)      // at most three rotations bring the smallest id to the front
    if (q0 > q1 || q0 > q2 || q0 > q3) {
      const int s = q0;
      q0 = q1, q1 = q2, q2 = q3, q3 = s;
    }
  f[0] = q0, f[1] = q1, f[2] = q2;
  f[3] = q0, f[4] = q2, f[5] = q3;
  return 2;
}

}  // namespace
