// Aligning one geometry to another: a per-scene similarity transform applied, the matched pairs reduced to nineteen fp64 moment sums,
// the closed-form similarity solve, and the point-to-point ICP loop around mvd_nearest_points_stages (include/mvd_hip.h: mvd_align_icp
// has the rule in full).
//
// apply_kernel: one thread per point, the scene's 12 doubles applied in fp64 in the header's order.
// chunk_count_kernel -> scan_kernel (fusion_common.hpp): first[s] = the number of kChunk-row chunks of the scenes before s, formed on the
// device once per call -- the scene offsets are never read back.  accumulate_kernel: workgroup b finds its (scene, chunk) in first[],
// every thread adds its rows k * 256 + t (k ascending) into 19 doubles, the 64 lanes of a wavefront meet in an xor butterfly (every lane
// ends with the same bits: fp64 addition commutes), the four wavefronts as (w0 + w1) + (w2 + w3).  A row that is not an accepted pair
// adds nothing.  solve_kernel: one workgroup per scene, lane k sums component k of the scene's partials in ascending chunk order (the
// partials staged through LDS by the whole workgroup), lane 0 solves and composes.  No float atomics anywhere: the same bits run to
// run, and for a scene alone and inside a batch, because a chunk is counted from the scene's own first row.
// The per-element pieces (al_apply, al_partner, al_accept, al_add_pair, al_solve, al_finish) are host-and-device functions:
// mvd_align_solve runs the very solve of the kernel on the host, and the pieces can be run serially on a CPU.
//
// POINT TO PLANE (mvd_plane_fit, mvd_plane_icp; the header has the rule): the same chunk map, the same reduction and the same loop with
// another thing summed per pair and another solve.  accumulate_kernel and solve_kernel are templates over the fit -- PointFit: the
// nineteen moments and Horn's solve; PlaneFit: the thirty sums of the linearised point-to-plane error and a 6 x 6 Jacobi with the
// unconstrained directions left out (pl_solve, which mvd_plane_solve runs on the host).
// MESH TARGET (mvd_mesh_icp): the plane loop with mvd_nearest_on_mesh_stages (meshdist.hip) as its search -- the closest point of the
// mesh and its face's normal ARE the pair, so PlaneFit runs with target = point, normals = normal and index == NULL.  No new arithmetic.
//
// Not tried: apply fused into the query's head or the accumulate's tail, a tree over the partials.
#include "align_common.hpp"

namespace {

constexpr int kAlSums = MVD_ALIGN_SUMS;
constexpr int kSolveTile = 128;                       // chunk sums the solve stages through LDS at a time (19 KB)
constexpr int kAlSweeps = 12;                         // cyclic Jacobi sweeps of the 4 x 4 solve (converged after 5 or 6; the rest skip)
constexpr double kAlThetaBig = 1e150;                 // above it theta^2 + 1 == theta^2 in fp64, and theta^2 would overflow near 1.3e154
constexpr int kPlSums = MVD_PLANE_SUMS;
constexpr int kPlSweeps = 16;                         // cyclic Jacobi sweeps of the 6 x 6 solve (converged after 6 or 7; the rest skip)
constexpr double kPlSmallAngle = 1e-4;                // below it the quaternion of the step comes from the series (next term: angle^6 / 645120)

// mvd_nearest_points' distance, in its order
AL_HD float al_d2(const float* p, const float* q) {
  const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// the target row that goes with source row i, or -1
AL_HD long long al_partner(const int* index, long long i, long long nt) {
  const long long j = index ? (long long)index[i] : i;
  return j >= 0 && j < nt ? j : -1;
}
// THE acceptance rule of the header, in fp32 (a NaN compares false)
AL_HD bool al_accept(float d2, float max_d2) { return d2 < INFINITY && d2 <= max_d2; }

// one accepted pair into the nineteen sums: every product of two fp32 values is exact in fp64
AL_HD void al_add_pair(double* s, const float* p, const float* q, float d2) {
  const double px = p[0], py = p[1], pz = p[2], qx = q[0], qy = q[1], qz = q[2];
  s[0] += 1.0;
  s[1] += px, s[2] += py, s[3] += pz;
  s[4] += qx, s[5] += qy, s[6] += qz;
  s[7] += px * qx, s[8] += px * qy, s[9] += px * qz;
  s[10] += py * qx, s[11] += py * qy, s[12] += py * qz;
  s[13] += pz * qx, s[14] += pz * qy, s[15] += pz * qz;
  s[16] += (px * px + py * py) + pz * pz;
  s[17] += (qx * qx + qy * qy) + qz * qz;
  s[18] += (double)d2;
}

// row i of the call: adds its pair, if it is one
AL_HD void al_add_row(double* s, const float* moved, const float* target, const int* index, const float* dist2, long long nt, float max_d2,
                      long long i) {
  const long long j = al_partner(index, i, nt);
  if (j < 0) return;
  const float p[3] = {moved[i * 3 + 0], moved[i * 3 + 1], moved[i * 3 + 2]}, q[3] = {target[j * 3 + 0], target[j * 3 + 1], target[j * 3 + 2]};
  const float d2 = dist2 ? dist2[i] : al_d2(p, q);
  if (al_accept(d2, max_d2)) al_add_pair(s, p, q, d2);
}

AL_HD bool al_finite(double v) { return fabs(v) < (double)INFINITY; }

AL_HD void al_identity(double* step, double* scale) {
#pragma unroll
  for (int k = 0; k < 12; ++k) step[k] = (k % 5 == 0) ? 1.0 : 0.0;
  *scale = 1.0;
}

// Cyclic Jacobi on a symmetric 4 x 4: A -> diagonal, the eigenvectors in the columns of V.
AL_HD void al_jacobi4(double A[4][4], double V[4][4]) {
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kAlSweeps; ++sweep)
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq), at = fabs(theta);
        // tan of the rotation angle, the smaller root: 1 / (|theta| + sqrt(theta^2 + 1)); for a huge theta that is 1 / (2 |theta|)
        double t = at > kAlThetaBig ? 0.5 / at : 1.0 / (at + sqrt(at * at + 1.0));
        if (theta < 0.0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < 4; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - sn * akq, A[k][q] = sn * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - sn * aqk, A[q][k] = sn * apk + c * aqk;
        }
        A[p][q] = A[q][p] = 0.0;
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - sn * vkq, V[k][q] = sn * vkp + c * vkq;
        }
      }
}

// THE solve of the header: the nineteen sums -> the step D (12 doubles, [s R | t]) and its scale.  The identity for what cannot be solved.
AL_HD void al_solve(const double* sums, int flags, double* step, double* scale) {
  al_identity(step, scale);
  const double n = sums[0];
  for (int k = 0; k < kAlSums; ++k)
    if (!al_finite(sums[k])) return;
  if (!(n >= 3.0)) return;
  const double mp[3] = {sums[1] / n, sums[2] / n, sums[3] / n}, mq[3] = {sums[4] / n, sums[5] / n, sums[6] / n};
  double M[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) M[a][b] = sums[7 + a * 3 + b] / n - mp[a] * mq[b];
  const double varp = sums[16] / n - ((mp[0] * mp[0] + mp[1] * mp[1]) + mp[2] * mp[2]);
  if (!(varp > 0.0)) return;
  // Horn's matrix: the unit quaternion (w, x, y, z) that maximises q^T N q is the rotation that takes p onto q
  double N[4][4], V[4][4];
  N[0][0] = (M[0][0] + M[1][1]) + M[2][2];
  N[1][1] = (M[0][0] - M[1][1]) - M[2][2];
  N[2][2] = (M[1][1] - M[0][0]) - M[2][2];
  N[3][3] = (M[2][2] - M[0][0]) - M[1][1];
  N[0][1] = N[1][0] = M[1][2] - M[2][1];
  N[0][2] = N[2][0] = M[2][0] - M[0][2];
  N[0][3] = N[3][0] = M[0][1] - M[1][0];
  N[1][2] = N[2][1] = M[0][1] + M[1][0];
  N[1][3] = N[3][1] = M[2][0] + M[0][2];
  N[2][3] = N[3][2] = M[1][2] + M[2][1];
  al_jacobi4(N, V);
  int best = 0;
  for (int k = 1; k < 4; ++k)
    if (N[k][k] > N[best][best]) best = k;
  double q[4] = {V[0][best], V[1][best], V[2][best], V[3][best]};
  const double len = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
  if (!(len > 0.0) || !al_finite(len)) return;
  const double sign = q[0] < 0.0 ? -1.0 : 1.0;
  for (int k = 0; k < 4; ++k) q[k] = sign * (q[k] / len);
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double R[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)},
                          {2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)},
                          {2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)}};
  double s = 1.0;
  if (flags & MVD_ALIGN_SCALE) {
    double tr = 0.0;
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) tr += R[b][a] * M[a][b];
    s = tr / varp;
    if (!(s > 0.0) || !al_finite(s)) return;      // (a collapsed or mirrored target: no similarity to fit)
  }
  double out[12];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) out[r * 4 + c] = s * R[r][c];
    out[r * 4 + 3] = mq[r] - ((out[r * 4 + 0] * mp[0] + out[r * 4 + 1] * mp[1]) + out[r * 4 + 2] * mp[2]);
  }
  for (int k = 0; k < 12; ++k)
    if (!al_finite(out[k])) return;
  for (int k = 0; k < 12; ++k) step[k] = out[k];
  *scale = s;
}

// A scene's sums -> its history row (rms, pairs, the scale of the steps so far: `before` times this step's) and, unless
// MVD_ALIGN_NO_STEP, m <- D m.
AL_HD void al_finish(const double* sums, int flags, double before, double* m, double* row) {
  const double n = sums[0];
  row[0] = n > 0.0 ? sqrt(sums[18] / n) : __builtin_nan("");
  row[1] = n;
  row[2] = before;
  if (flags & MVD_ALIGN_NO_STEP) return;
  double D[12], s, out[12];
  al_solve(sums, flags, D, &s);
  row[2] = before * s;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 4; ++c) out[r * 4 + c] = (D[r * 4 + 0] * m[0 * 4 + c] + D[r * 4 + 1] * m[1 * 4 + c]) + D[r * 4 + 2] * m[2 * 4 + c];
    out[r * 4 + 3] += D[r * 4 + 3];
  }
  for (int k = 0; k < 12; ++k) m[k] = out[k];
}

// ---------------------------------------------------------------------------------------------------------------- point to plane
// one accepted pair into the thirty sums: p the moved source point, q the target, n its normal
AL_HD void pl_add_pair(double* s, const float* p, const float* q, const float* nrm, float d2) {
  const double px = p[0], py = p[1], pz = p[2], nx = nrm[0], ny = nrm[1], nz = nrm[2];
  const double ex = px - (double)q[0], ey = py - (double)q[1], ez = pz - (double)q[2];
  const double r = (ex * nx + ey * ny) + ez * nz;
  const double a[6] = {py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz};      // (p x n, n): the products are exact
  s[0] += 1.0;
  int at = 1;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) s[at++] += a[i] * a[j];
#pragma unroll
  for (int i = 0; i < 6; ++i) s[22 + i] += a[i] * r;
  s[28] += r * r;
  s[29] += (double)d2;
}

AL_HD bool pl_finitef(float v) { return fabsf(v) < INFINITY; }

// row i of the call: adds its pair, if it is one -- mvd_align_fit's pairs and acceptance, and a finite non-zero normal at the target
AL_HD void pl_add_row(double* s, const float* moved, const float* target, const float* normals, const int* index, const float* dist2, long long nt,
                      float max_d2, long long i) {
  const long long j = al_partner(index, i, nt);
  if (j < 0) return;
  const float p[3] = {moved[i * 3 + 0], moved[i * 3 + 1], moved[i * 3 + 2]}, q[3] = {target[j * 3 + 0], target[j * 3 + 1], target[j * 3 + 2]};
  const float nrm[3] = {normals[j * 3 + 0], normals[j * 3 + 1], normals[j * 3 + 2]};
  const float d2 = dist2 ? dist2[i] : al_d2(p, q);
  if (!al_accept(d2, max_d2)) return;
  if (!(pl_finitef(nrm[0]) && pl_finitef(nrm[1]) && pl_finitef(nrm[2])) || (nrm[0] == 0.f && nrm[1] == 0.f && nrm[2] == 0.f)) return;
  pl_add_pair(s, p, q, nrm, d2);
}

// Cyclic Jacobi on a symmetric 6 x 6 (al_jacobi4's conventions): A -> diagonal, the eigenvectors in the columns of V.
AL_HD void pl_jacobi6(double A[6][6], double V[6][6]) {
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kPlSweeps; ++sweep)
    for (int p = 0; p < 5; ++p)
      for (int q = p + 1; q < 6; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq), at = fabs(theta);
        double t = at > kAlThetaBig ? 0.5 / at : 1.0 / (at + sqrt(at * at + 1.0));
        if (theta < 0.0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < 6; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - sn * akq, A[k][q] = sn * akp + c * akq;
        }
        for (int k = 0; k < 6; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - sn * aqk, A[q][k] = sn * apk + c * aqk;
        }
        A[p][q] = A[q][p] = 0.0;
        for (int k = 0; k < 6; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - sn * vkq, V[k][q] = sn * vkp + c * vkq;
        }
      }
}

// THE solve of the header: the thirty sums -> the rigid step D (12 doubles, [R | t]) and the rank kept.  The identity (rank 0) for what
// cannot be solved.
AL_HD void pl_solve(const double* sums, double* step, int* rank) {
  double one;
  al_identity(step, &one);
  *rank = 0;
  for (int k = 0; k < kPlSums; ++k)
    if (!al_finite(sums[k])) return;
  if (!(sums[0] >= 3.0)) return;
  double H[6][6], V[6][6];
  int at = 1;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) H[i][j] = H[j][i] = sums[at++];
  const double* g = sums + 22;
  pl_jacobi6(H, V);
  double top = H[0][0];
  for (int k = 1; k < 6; ++k) top = fmax(top, H[k][k]);
  if (!(top > 0.0) || !al_finite(top)) return;
  double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int kept = 0;
  for (int i = 0; i < 6; ++i) {
    const double lam = H[i][i];
    if (!(lam > MVD_PLANE_EPS_RANK * top)) continue;      // a direction the data does not constrain is left alone
    double dot = 0.0;
    for (int k = 0; k < 6; ++k) dot += V[k][i] * g[k];
    const double w = dot / lam;
    for (int k = 0; k < 6; ++k) x[k] -= V[k][i] * w;
    ++kept;
  }
  // R = exp([omega]x) through the unit quaternion (cos(angle / 2), omega sin(angle / 2) / angle)
  const double ang2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2], ang = sqrt(ang2);
  double qw, f;
  if (ang < kPlSmallAngle) qw = 1.0 - ang2 / 8.0 + ang2 * ang2 / 384.0, f = 0.5 - ang2 / 48.0 + ang2 * ang2 / 3840.0;
  else qw = cos(0.5 * ang), f = sin(0.5 * ang) / ang;
  double q[4] = {qw, f * x[0], f * x[1], f * x[2]};
  const double len = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
  if (!(len > 0.0) || !al_finite(len)) return;
  for (int k = 0; k < 4; ++k) q[k] = q[k] / len;
  const double w = q[0], a = q[1], b = q[2], c = q[3];
  const double out[12] = {1.0 - 2.0 * (b * b + c * c), 2.0 * (a * b - w * c), 2.0 * (a * c + w * b), x[3],
                          2.0 * (a * b + w * c), 1.0 - 2.0 * (a * a + c * c), 2.0 * (b * c - w * a), x[4],
                          2.0 * (a * c - w * b), 2.0 * (b * c + w * a), 1.0 - 2.0 * (a * a + b * b), x[5]};
  for (int k = 0; k < 12; ++k)
    if (!al_finite(out[k])) return;
  for (int k = 0; k < 12; ++k) step[k] = out[k];
  *rank = kept;
}

// m <- D m in fp64 (al_finish's composition)
AL_HD void al_compose(const double* D, double* m) {
  double out[12];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 4; ++c) out[r * 4 + c] = (D[r * 4 + 0] * m[0 * 4 + c] + D[r * 4 + 1] * m[1 * 4 + c]) + D[r * 4 + 2] * m[2 * 4 + c];
    out[r * 4 + 3] += D[r * 4 + 3];
  }
  for (int k = 0; k < 12; ++k) m[k] = out[k];
}

// A scene's thirty sums -> its history row (plane rms, pairs, point rms, the rank its solve keeps) and, unless MVD_PLANE_NO_STEP, m <- D m.
AL_HD void pl_finish(const double* sums, int flags, double* m, double* row) {
  const double n = sums[0];
  row[0] = n > 0.0 ? sqrt(sums[28] / n) : __builtin_nan("");
  row[1] = n;
  row[2] = n > 0.0 ? sqrt(sums[29] / n) : __builtin_nan("");
  double D[12];
  int rank;
  pl_solve(sums, D, &rank);
  row[3] = (double)rank;
  if (!(flags & MVD_PLANE_NO_STEP)) al_compose(D, m);
}

// ---------------------------------------------------------------------------------------------------------------- kernels
struct FitArgs {
  const float *moved, *target;
  const int *start, *index;
  const float* dist2;
  unsigned* first;                                    // nscene + 1 words: chunks before scene s; [nscene] = all of them
  double* partial;                                    // nwg * kAlSums
  long long n, nt;
  int nscene;
  unsigned nwg;                                       // the launch's workgroups: the host bound ceil(n / kAlChunk) + nscene
  float max_d2;
  const float* normals;                               // PlaneFit: (nt, 3) at the target's rows
};

// What a fit sums per pair and does with a scene's sums.
struct PointFit {
  static constexpr int kSums = kAlSums, kHistory = MVD_ALIGN_HISTORY;
  AL_HD static void add_row(double* s, const FitArgs& a, long long i) { al_add_row(s, a.moved, a.target, a.index, a.dist2, a.nt, a.max_d2, i); }
  AL_HD static void finish(const double* sums, int flags, const double* previous_row, double* m, double* row) {
    al_finish(sums, flags, previous_row ? previous_row[2] : 1.0, m, row);
  }
};
struct PlaneFit {
  static constexpr int kSums = kPlSums, kHistory = MVD_PLANE_HISTORY;
  AL_HD static void add_row(double* s, const FitArgs& a, long long i) {
    pl_add_row(s, a.moved, a.target, a.normals, a.index, a.dist2, a.nt, a.max_d2, i);
  }
  AL_HD static void finish(const double* sums, int flags, const double*, double* m, double* row) { pl_finish(sums, flags, m, row); }
};

__global__ __launch_bounds__(kAlThreads) void apply_kernel(const float* __restrict__ src, const int* __restrict__ start, long long n, int nscene,
                                                           const double* __restrict__ transform, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * kAlThreads + threadIdx.x;
  if (i >= n) return;
  const float x = src[i * 3 + 0], y = src[i * 3 + 1], z = src[i * 3 + 2];
  float r[3] = {x, y, z};
  const int s = al_find_scene(start, nscene, n, i);
  if (s >= 0) al_apply(transform + (size_t)s * 12, x, y, z, r);
  out[i * 3 + 0] = r[0], out[i * 3 + 1] = r[1], out[i * 3 + 2] = r[2];
}

__global__ __launch_bounds__(kAlThreads) void chunk_count_kernel(const int* __restrict__ start, int nscene, long long n, unsigned* __restrict__ first) {
  const int s = blockIdx.x * kAlThreads + threadIdx.x;
  if (s < nscene) first[s] = al_chunks_of(start, s, n);
}

template <class Fit>
__global__ __launch_bounds__(kAlThreads) void accumulate_kernel(FitArgs a) {
  constexpr int kSums = Fit::kSums;
  __shared__ double wave_s[kAlThreads / 64][kSums];
  const unsigned b = blockIdx.x;
  if (b >= a.first[a.nscene]) return;      // (uniform) the bound's slack
  int lo = 0, hi = a.nscene;               // the last scene with first[s] <= b: first[0] = 0, an empty scene owns no chunk
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.first[mid] <= b) lo = mid;
    else hi = mid;
  }
  const long long r0 = al_clamp(a.start[lo], a.n) + (long long)(b - a.first[lo]) * kAlChunk;
  const long long end = al_clamp(a.start[lo + 1], a.n), r1 = r0 + kAlChunk < end ? r0 + kAlChunk : end;
  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
  for (int k = 0; k < kAlChunk / kAlThreads; ++k) {
    const long long i = r0 + k * kAlThreads + threadIdx.x;
    if (i < r1) Fit::add_row(acc, a, i);
  }
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    acc[k] = v;
  }
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < kSums; ++k) wave_s[threadIdx.x >> 6][k] = acc[k];
  __syncthreads();
  if (threadIdx.x < kSums)
    a.partial[(size_t)b * kSums + threadIdx.x] = (wave_s[0][threadIdx.x] + wave_s[1][threadIdx.x]) + (wave_s[2][threadIdx.x] + wave_s[3][threadIdx.x]);
}

// The chunk sums of a scene arrive in LDS kSolveTile chunks at a time, loaded by the whole workgroup (one memory latency per tile,
// not per chunk); lane k then adds component k in ascending chunk order.
template <class Fit>
__global__ __launch_bounds__(kAlThreads) void solve_kernel(FitArgs a, int flags, double* __restrict__ transform, double* __restrict__ history,
                                                           const double* __restrict__ previous) {
  constexpr int kSums = Fit::kSums;
  __shared__ double tile[kSolveTile * kSums];
  __shared__ double sums[kSums];
  const int s = blockIdx.x;
  const unsigned c0 = min(a.first[s], a.nwg), c1 = min(a.first[s + 1], a.nwg);
  double v = 0.0;
  for (unsigned base = c0; base < c1; base += kSolveTile) {      // (uniform)
    const unsigned m = min((unsigned)kSolveTile, c1 - base);
    __syncthreads();      // the previous tile has been added
    for (unsigned e = threadIdx.x; e < m * kSums; e += kAlThreads) tile[e] = a.partial[(size_t)base * kSums + e];
    __syncthreads();
    if (threadIdx.x < kSums)
      for (unsigned j = 0; j < m; ++j) v += tile[j * kSums + threadIdx.x];
  }
  if (threadIdx.x < kSums) sums[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    Fit::finish(sums, flags, previous ? previous + (size_t)s * Fit::kHistory : nullptr, transform + (size_t)s * 12,
                history + (size_t)s * Fit::kHistory);
}

// ---------------------------------------------------------------------------------------------------------------- host
struct AlignPlan {
  unsigned nwg;
  size_t off_partial, off_nn, nn_bytes, bytes;
};

// bytes == 0: an argument is out of range
static AlignPlan al_plan(size_t nq, size_t nt, int nscene, int method, int grid, int sums, bool mesh) {
  AlignPlan p{};
  if (nscene < 1 || nscene > 65535 || nq > 0x7fffffffull || nt > 0x7fffffffull || method < MVD_NN_AUTO || method > MVD_NN_GRID || grid < 0 ||
      grid > 256)
    return p;
  if (method != MVD_NN_BRUTE && (unsigned long long)nscene * grid * grid * grid > 0x7fffffffull) return p;
  // (the limit of mvd_nearest_on_mesh's grid; MVD_NN_AUTO takes the grid at such a size whatever nscene)
  if (mesh && method != MVD_NN_BRUTE && (unsigned long long)nt * MVD_MESH_SPAN * MVD_MESH_SPAN * MVD_MESH_SPAN > 0x7fffffffull) return p;
  p.nwg = (unsigned)((nq + kAlChunk - 1) / kAlChunk) + (unsigned)nscene;
  p.off_partial = al_up16((size_t)(nscene + 1) * sizeof(unsigned));
  p.off_nn = p.off_partial + al_up16((size_t)p.nwg * sums * sizeof(double));
  p.nn_bytes = mesh ? mvd_nearest_on_mesh_scratch(nt, nscene, method, grid) : mvd_nearest_points_scratch(nt, nscene, method, grid);      // (nt: nf)
  p.bytes = p.off_nn + p.nn_bytes;
  return p;
}

static FitArgs al_args(const AlignPlan& p, void* scratch, const float* moved, const int* start, const float* target, const int* index,
                       const float* dist2, size_t n, size_t nt, int nscene, float max_d2, const float* normals) {
  char* base = (char*)scratch;
  return FitArgs{moved, target, start, index, dist2, (unsigned*)base, (double*)(base + p.off_partial), (long long)n, (long long)nt, nscene, p.nwg, max_d2,
                 normals};
}

// first[]: once per call
static void al_launch_map(const FitArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(chunk_count_kernel, dim3(cdiv(a.nscene, kAlThreads)), dim3(kAlThreads), 0, st, a.start, a.nscene, a.n, a.first);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kCompactThreads), 0, st, a.first, (unsigned)a.nscene, a.first + a.nscene);
}

// previous: the history row before this one (its scale is carried on), or NULL for the first
template <class Fit>
static void al_launch_fit(const FitArgs& a, int flags, double* transform, double* history, const double* previous, hipStream_t st) {
  hipLaunchKernelGGL(accumulate_kernel<Fit>, dim3(a.nwg), dim3(kAlThreads), 0, st, a);
  hipLaunchKernelGGL(solve_kernel<Fit>, dim3(a.nscene), dim3(kAlThreads), 0, st, a, flags, transform, history, previous);
}

static void al_launch_apply(const float* src, const int* start, size_t n, int nscene, const double* transform, float* out, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(apply_kernel, dim3(cdiv((long)n, kAlThreads)), dim3(kAlThreads), 0, st, src, start, (long long)n, nscene, transform, out);
}

// One fit of given pairs: mvd_align_fit (normals == NULL) and mvd_plane_fit.  flags_are: the flags the entry takes, in its message's words.
template <class Fit>
static int al_fit(const char* fn, int allowed_flags, const char* flags_are, const float* moved, const int* start, const float* target,
                  const float* normals, const int* index, const float* dist2, size_t n, size_t nt, int nscene, int flags, float max_dist2,
                  double* transform, double* history_row, void* scratch, size_t scratch_bytes, mvd_stream_t stream) {
  MVD_CHECK_ARG(nscene >= 1 && nscene <= 65535, "%s: nscene=%d outside [1, 65535]", fn, nscene);
  MVD_CHECK_ARG(n <= 0x7fffffffull && nt <= 0x7fffffffull, "%s: n=%zu, nt=%zu beyond 2^31 - 1", fn, n, nt);
  MVD_CHECK_ARG((flags & ~allowed_flags) == 0, "%s: flags=%d (%s)", fn, flags, flags_are);
  MVD_CHECK_ARG(max_dist2 >= 0.f, "%s: max_dist2=%g (>= 0, +inf for no gate)", fn, (double)max_dist2);
  MVD_CHECK_ARG(start && transform && history_row && al_aligned(transform, 8) && al_aligned(history_row, 8),
                "%s: null start, null or misaligned transform or history_row", fn);
  MVD_CHECK_ARG(moved || n == 0, "%s: null moved with n=%zu", fn, n);
  if (std::is_same<Fit, PlaneFit>::value) MVD_CHECK_ARG((target && normals) || nt == 0, "%s: null target or normals with nt=%zu", fn, nt);
  else MVD_CHECK_ARG(target || nt == 0, "%s: null target with nt=%zu", fn, nt);
  const AlignPlan p = al_plan(n, 0, nscene, MVD_NN_BRUTE, 0, Fit::kSums, false);
  MVD_CHECK_ARG(scratch && scratch_bytes >= p.bytes && al_aligned(scratch, 16), "%s: scratch of %zu bytes (needs %zu, 16-byte aligned)", fn,
                scratch_bytes, p.bytes);
  const FitArgs a = al_args(p, scratch, moved, start, target, index, dist2, n, nt, nscene, max_dist2, normals);
  al_launch_map(a, (hipStream_t)stream);
  al_launch_fit<Fit>(a, flags, transform, history_row, nullptr, (hipStream_t)stream);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

// What an ICP loop searches: the moved source, the target's arrays, the checks that name them, and the exported search of one against the
// other (BUILD once, QUERY per row).  nn: the search's part of the scratch, placed by al_icp.
struct PointSearch {
  static constexpr bool kMesh = false;
  float* moved;
  const int* source_start;
  const float* target;
  const int* target_start;
  size_t nq, nt;
  int nscene, method, grid, *index;
  float* dist2;
  mvd_stream_t stream;
  void* nn;
  size_t nn_bytes;
  size_t size() const { return nt; }
  int check(const char* fn, const float* source) const {
    MVD_CHECK_ARG(nq <= 0x7fffffffull && nt <= 0x7fffffffull, "%s: nq=%zu, nt=%zu beyond 2^31 - 1", fn, nq, nt);
    MVD_CHECK_ARG(source_start && target_start, "%s: null source_start or target_start", fn);
    MVD_CHECK_ARG((source && moved && index && dist2) || nq == 0, "%s: null source, moved, index or dist2 with nq=%zu", fn, nq);
    return 0;
  }
  void too_large(const char* fn) const { mvd_set_error("%s: nscene * grid^3 cells beyond 2^31 - 1 (nscene=%d, grid=%d)", fn, nscene, grid); }
  int operator()(int stages) const {
    return mvd_nearest_points_stages(moved, source_start, target, target_start, nq, nt, nscene, method, grid, index, dist2, nn, nn_bytes, stages,
                                     stream);
  }
};

struct MeshSearch {
  static constexpr bool kMesh = true;
  float* moved;
  const int* source_start;
  const float* vertices;
  const int *faces, *face_start;
  size_t nq, nv, nf;
  int nscene, method, grid, *face;
  float *dist2, *point, *normal;
  mvd_stream_t stream;
  void* nn;
  size_t nn_bytes;
  size_t size() const { return nf; }
  int check(const char* fn, const float* source) const {
    MVD_CHECK_ARG(nq <= 0x7fffffffull && nv <= 0x7fffffffull && nf <= 0x7fffffffull, "%s: nq=%zu, nv=%zu, nf=%zu beyond 2^31 - 1", fn, nq, nv, nf);
    MVD_CHECK_ARG(source_start && face_start, "%s: null source_start or face_start", fn);
    MVD_CHECK_ARG((source && moved && face && dist2 && point && normal) || nq == 0, "%s: null source, moved, face, dist2, point or normal with nq=%zu",
                  fn, nq);
    MVD_CHECK_ARG(faces || nf == 0, "%s: null faces with nf=%zu", fn, nf);
    MVD_CHECK_ARG(vertices || nv == 0, "%s: null vertices with nv=%zu", fn, nv);
    return 0;
  }
  void too_large(const char* fn) const {
    mvd_set_error("%s: nscene * grid^3 cells or nf * %d references beyond 2^31 - 1 (nscene=%d, grid=%d, nf=%zu)", fn,
                  MVD_MESH_SPAN * MVD_MESH_SPAN * MVD_MESH_SPAN, nscene, grid, nf);
  }
  // (the search checks its own arguments before it enqueues anything, so a refusal of its own has written nothing either)
  int operator()(int stages) const {
    return mvd_nearest_on_mesh_stages(moved, source_start, vertices, faces, face_start, nq, nv, nf, nscene, method, grid, face, dist2, point,
                                      nullptr, nullptr, normal, nn, nn_bytes, stages, stream);
  }
};

static_assert(MVD_PLANE_NO_STEP == MVD_ALIGN_NO_STEP, "the loop marks its last row with one flag for both fits");

// THE loop of mvd_align_icp, mvd_plane_icp and mvd_mesh_icp (the header has the rule), with a fit and a search plugged in.  The entry has
// run s.check() and the null checks of its own arrays; every check, there and here, comes before the first enqueue.  Row i of s.moved is
// fitted to target[index[i]] (index == NULL: target[i]) and, by PlaneFit, the normal there.  flags: MVD_ALIGN_SCALE or 0.
template <class Fit, class Search>
static int al_icp(const char* fn, Search s, const float* source, int iters, int flags, float max_dist2, double* transform, double* history,
                  void* scratch, size_t scratch_bytes, const float* target, const int* index, size_t nt, const float* normals) {
  MVD_CHECK_ARG(s.method >= MVD_NN_AUTO && s.method <= MVD_NN_GRID, "%s: method=%d (MVD_NN_AUTO, _BRUTE or _GRID)", fn, s.method);
  MVD_CHECK_ARG(s.grid >= 0 && s.grid <= 256, "%s: grid=%d outside [0, 256]", fn, s.grid);
  MVD_CHECK_ARG(s.nscene >= 1 && s.nscene <= 65535, "%s: nscene=%d outside [1, 65535]", fn, s.nscene);
  MVD_CHECK_ARG(iters >= 0 && iters <= MVD_ALIGN_MAX_ITERS, "%s: iters=%d outside [0, %d]", fn, iters, MVD_ALIGN_MAX_ITERS);
  MVD_CHECK_ARG((flags & ~MVD_ALIGN_SCALE) == 0, "%s: flags=%d (MVD_ALIGN_SCALE or 0)", fn, flags);
  MVD_CHECK_ARG(max_dist2 >= 0.f, "%s: max_dist2=%g (>= 0, +inf for no gate)", fn, (double)max_dist2);
  MVD_CHECK_ARG(transform && history && al_aligned(transform, 8) && al_aligned(history, 8), "%s: null or misaligned transform or history", fn);
  const AlignPlan p = al_plan(s.nq, s.size(), s.nscene, s.method, s.grid, Fit::kSums, Search::kMesh);
  if (!p.bytes) return s.too_large(fn), -1;
  MVD_CHECK_ARG(scratch && scratch_bytes >= p.bytes && al_aligned(scratch, 16), "%s: scratch of %zu bytes (needs %zu, 16-byte aligned)", fn,
                scratch_bytes, p.bytes);
  const hipStream_t st = (hipStream_t)s.stream;
  s.nn = p.nn_bytes ? (void*)((char*)scratch + p.off_nn) : nullptr, s.nn_bytes = p.nn_bytes;
  const FitArgs a = al_args(p, scratch, s.moved, s.source_start, target, index, s.dist2, s.nq, nt, s.nscene, max_dist2, normals);
  int rc = s(MVD_NN_BUILD);
  if (rc == 0) al_launch_map(a, st);
  const size_t row = (size_t)s.nscene * Fit::kHistory;
  for (int k = 0; k <= iters && rc == 0; ++k) {      // row k: the pairs under the transform before step k; the last row has no step
    al_launch_apply(source, s.source_start, s.nq, s.nscene, transform, s.moved, st);
    rc = s(MVD_NN_QUERY);
    if (rc != 0) break;      // (its argument checks are this function's own, so only a failed enqueue gets here: nothing is fitted to it)
    // (the row before: PointFit carries its scale on, PlaneFit does not look)
    al_launch_fit<Fit>(a, k < iters ? flags : (flags | MVD_ALIGN_NO_STEP), transform, history + (size_t)k * row,
                       k ? history + (size_t)(k - 1) * row : nullptr, st);
  }
  if (rc != 0) {
    char why[400];
    snprintf(why, sizeof(why), "%s", mvd_last_error());
    mvd_set_error("%s: %s", fn, why);
    return rc;
  }
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

}  // namespace

extern "C" size_t mvd_align_scratch(size_t nq, size_t nt, int nscene, int method, int grid) {
  return al_plan(nq, nt, nscene, method, grid, kAlSums, false).bytes;
}

extern "C" int mvd_align_solve(const double* sums, int flags, double* step, double* scale) {
  const char* fn = "mvd_align_solve";
  MVD_CHECK_ARG(sums && step && scale, "%s: null sums, step or scale", fn);
  MVD_CHECK_ARG((flags & ~MVD_ALIGN_SCALE) == 0, "%s: flags=%d (MVD_ALIGN_SCALE or 0)", fn, flags);
  al_solve(sums, flags, step, scale);
  return 0;
}

extern "C" int mvd_align_apply(const float* src, const int* src_start, size_t n, int nscene, const double* transform, float* out,
                               mvd_stream_t stream) {
  const char* fn = "mvd_align_apply";
  MVD_CHECK_ARG(nscene >= 1 && nscene <= 65535, "%s: nscene=%d outside [1, 65535]", fn, nscene);
  MVD_CHECK_ARG(n <= 0x7fffffffull, "%s: n=%zu beyond 2^31 - 1", fn, n);
  MVD_CHECK_ARG(src_start && transform && al_aligned(transform, 8), "%s: null src_start, null or misaligned transform", fn);
  MVD_CHECK_ARG((src && out) || n == 0, "%s: null src or out with n=%zu", fn, n);
  al_launch_apply(src, src_start, n, nscene, transform, out, (hipStream_t)stream);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int mvd_align_fit(const float* moved, const int* start, const float* target, const int* index, const float* dist2, size_t n,
                             size_t nt, int nscene, int flags, float max_dist2, double* transform, double* history_row, void* scratch,
                             size_t scratch_bytes, mvd_stream_t stream) {
  return al_fit<PointFit>("mvd_align_fit", MVD_ALIGN_SCALE | MVD_ALIGN_NO_STEP, "an OR of MVD_ALIGN_SCALE and MVD_ALIGN_NO_STEP", moved, start, target,
                          nullptr, index, dist2, n, nt, nscene, flags, max_dist2, transform, history_row, scratch, scratch_bytes, stream);
}

extern "C" int mvd_align_icp(const float* source, const int* source_start, const float* target, const int* target_start, size_t nq, size_t nt,
                             int nscene, int method, int grid, int iters, int flags, float max_dist2, double* transform, double* history,
                             float* moved, int* index, float* dist2, void* scratch, size_t scratch_bytes, mvd_stream_t stream) {
  const char* fn = "mvd_align_icp";
  const PointSearch search{moved, source_start, target, target_start, nq, nt, nscene, method, grid, index, dist2, stream};
  if (search.check(fn, source) != 0) return -1;
  MVD_CHECK_ARG(target || nt == 0, "%s: null target with nt=%zu", fn, nt);
  return al_icp<PointFit>(fn, search, source, iters, flags, max_dist2, transform, history, scratch, scratch_bytes, target, index, nt, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------- point to plane: entries
extern "C" size_t mvd_plane_scratch(size_t nq, size_t nt, int nscene, int method, int grid) {
  return al_plan(nq, nt, nscene, method, grid, kPlSums, false).bytes;
}

extern "C" int mvd_plane_solve(const double* sums, double* step, int* rank) {
  const char* fn = "mvd_plane_solve";
  MVD_CHECK_ARG(sums && step && rank, "%s: null sums, step or rank", fn);
  pl_solve(sums, step, rank);
  return 0;
}

extern "C" int mvd_plane_fit(const float* moved, const int* start, const float* target, const float* normals, const int* index,
                             const float* dist2, size_t n, size_t nt, int nscene, int flags, float max_dist2, double* transform,
                             double* history_row, void* scratch, size_t scratch_bytes, mvd_stream_t stream) {
  return al_fit<PlaneFit>("mvd_plane_fit", MVD_PLANE_NO_STEP, "MVD_PLANE_NO_STEP or 0", moved, start, target, normals, index, dist2, n, nt, nscene,
                          flags, max_dist2, transform, history_row, scratch, scratch_bytes, stream);
}

extern "C" int mvd_plane_icp(const float* source, const int* source_start, const float* target, const int* target_start, const float* normals,
                             size_t nq, size_t nt, int nscene, int method, int grid, int iters, float max_dist2, double* transform,
                             double* history, float* moved, int* index, float* dist2, void* scratch, size_t scratch_bytes,
                             mvd_stream_t stream) {
  const char* fn = "mvd_plane_icp";
  const PointSearch search{moved, source_start, target, target_start, nq, nt, nscene, method, grid, index, dist2, stream};
  if (search.check(fn, source) != 0) return -1;
  MVD_CHECK_ARG((target && normals) || nt == 0, "%s: null target or normals with nt=%zu", fn, nt);
  return al_icp<PlaneFit>(fn, search, source, iters, 0, max_dist2, transform, history, scratch, scratch_bytes, target, index, nt, normals);
}

// ---------------------------------------------------------------------------------------------------------------- mesh target: entries
extern "C" size_t mvd_mesh_icp_scratch(size_t nq, size_t nf, int nscene, int method, int grid) {
  return al_plan(nq, nf, nscene, method, grid, kPlSums, true).bytes;
}

extern "C" int mvd_mesh_icp(const float* source, const int* source_start, const float* vertices, const int* faces, const int* face_start,
                            size_t nq, size_t nv, size_t nf, int nscene, int method, int grid, int iters, float max_dist2, double* transform,
                            double* history, float* moved, int* face, float* dist2, float* point, float* normal, void* scratch,
                            size_t scratch_bytes, mvd_stream_t stream) {
  const char* fn = "mvd_mesh_icp";
  const MeshSearch search{moved, source_start, vertices, faces, face_start, nq, nv, nf, nscene, method, grid, face, dist2, point, normal, stream};
  if (search.check(fn, source) != 0) return -1;
  // the pairs of the plane fit: row i of moved with row i of point and normal
  return al_icp<PlaneFit>(fn, search, source, iters, 0, max_dist2, transform, history, scratch, scratch_bytes, point, nullptr, nq, normal);
}
