// A normal per point from a list of neighbour rows: centre, covariance and a 3 x 3 cyclic Jacobi in fp64, one thread per point
// (include/mvd_hip.h: mvd_point_normals has the rule in full).
//
// The rows are read twice from global memory (centre, then covariance): k rows of 12 bytes that the neighbouring threads of a cloud
// sorted by position share through the caches; no list is held in registers or LDS.  pn_normal is a host-and-device function, so that
// the rule can be run serially on a CPU.
//
// Not tried: one wavefront per point, single-pass raw moments (they cancel where the rule's centred sums do not), an analytic 3 x 3
// eigen solve.
#include "jacobi3.hpp"

namespace {

constexpr int kPnThreads = 256;

PN_HD bool pn_finite(double v) { return fabs(v) < (double)INFINITY; }      // (a NaN compares false)
PN_HD bool pn_finitef(float v) { return fabsf(v) < INFINITY; }

// a used row's coordinates as doubles; false for a row that is not used
PN_HD bool pn_row(const float* target, long long nt, int j, double* x) {
  if (j < 0 || j >= nt) return false;
  const float a = target[(long long)j * 3 + 0], b = target[(long long)j * 3 + 1], c = target[(long long)j * 3 + 2];
  if (!(pn_finitef(a) && pn_finitef(b) && pn_finitef(c))) return false;
  x[0] = a, x[1] = b, x[2] = c;
  return true;
}

// THE rule of the header for one point: row (k entries) -> out[3], *variation.  p, toward: 3 floats each, or toward == nullptr.
PN_HD void pn_normal(const float* target, long long nt, const int* row, int k, const float* p, const float* toward, float* out, float* variation) {
  out[0] = out[1] = out[2] = 0.f;
  *variation = __builtin_nanf("");
  double sum[3] = {0.0, 0.0, 0.0}, x[3];
  int m = 0;
  for (int e = 0; e < k; ++e)
    if (pn_row(target, nt, row[e], x)) sum[0] += x[0], sum[1] += x[1], sum[2] += x[2], ++m;
  if (m < 3) return;
  const double c[3] = {sum[0] / (double)m, sum[1] / (double)m, sum[2] / (double)m};
  double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
  for (int e = 0; e < k; ++e)
    if (pn_row(target, nt, row[e], x)) {
      const double dx = x[0] - c[0], dy = x[1] - c[1], dz = x[2] - c[2];
      xx += dx * dx, xy += dx * dy, xz += dx * dz, yy += dy * dy, yz += dy * dz, zz += dz * dz;
    }
  if (!(pn_finite(xx) && pn_finite(xy) && pn_finite(xz) && pn_finite(yy) && pn_finite(yz) && pn_finite(zz))) return;
  double A[3][3] = {{xx, xy, xz}, {xy, yy, yz}, {xz, yz, zz}}, V[3][3];
  pn_jacobi3(A, V);
  const double e0 = fmax(A[0][0], 0.0), e1 = fmax(A[1][1], 0.0), e2 = fmax(A[2][2], 0.0);
  if (!(pn_finite(e0) && pn_finite(e1) && pn_finite(e2))) return;
  // the column of the smallest eigenvalue, the lowest between equal ones -- selects, never a runtime subscript
  const bool c1 = e1 < e0, c2 = e2 < (c1 ? e1 : e0);
  double n[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) n[a] = c2 ? V[a][2] : (c1 ? V[a][1] : V[a][0]);
  const double l0 = fmin(e0, fmin(e1, e2)), l2 = fmax(e0, fmax(e1, e2));
  const double l1 = fmax(fmin(e0, e1), fmin(fmax(e0, e1), e2));      // the median
  if (!(l1 > 0.0)) return;
  const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
  if (!(len > 0.0) || !pn_finite(len)) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) n[a] = n[a] / len;
  if (!(pn_finite(n[0]) && pn_finite(n[1]) && pn_finite(n[2]))) return;
  const double a0 = fabs(n[0]), a1 = fabs(n[1]), a2 = fabs(n[2]);
  const double lead = (a0 >= a1 && a0 >= a2) ? n[0] : (a1 >= a2 ? n[1] : n[2]);      // the largest magnitude, the lowest axis between equals
  bool flip = lead < 0.0;
  if (toward) {
    const double tx = (double)toward[0] - (double)p[0], ty = (double)toward[1] - (double)p[1], tz = (double)toward[2] - (double)p[2];
    const double side = (n[0] * tx + n[1] * ty) + n[2] * tz;
    if ((flip ? -side : side) < 0.0) flip = !flip;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) out[a] = (float)(flip ? -n[a] : n[a]);
  *variation = (float)(l0 / ((l0 + l1) + l2));
}

__global__ __launch_bounds__(kPnThreads) void normals_kernel(const float* __restrict__ target, long long nt, const int* __restrict__ index, long long n,
                                                             int k, const float* __restrict__ points, const float* __restrict__ toward,
                                                             float* __restrict__ normal, float* __restrict__ variation) {
  const long long i = (long long)blockIdx.x * kPnThreads + threadIdx.x;
  if (i >= n) return;
  float out[3], var;
  pn_normal(target, nt, index + i * k, k, toward ? points + i * 3 : nullptr, toward ? toward + i * 3 : nullptr, out, &var);
  normal[i * 3 + 0] = out[0], normal[i * 3 + 1] = out[1], normal[i * 3 + 2] = out[2];
  variation[i] = var;
}

}  // namespace

extern "C" int mvd_point_normals(const float* target, size_t nt, const int* index, size_t n, int k, const float* points, const float* toward,
                                 float* normal, float* variation, mvd_stream_t stream) {
  const char* fn = "mvd_point_normals";
  MVD_CHECK_ARG(k >= 1 && k <= MVD_NORMALS_MAX_K, "%s: k=%d outside [1, %d]", fn, k, MVD_NORMALS_MAX_K);
  MVD_CHECK_ARG(nt <= 0x7fffffffull && n <= 0x7fffffffull && n * (size_t)k <= 0x7fffffffull, "%s: nt=%zu, n=%zu, n * k beyond 2^31 - 1", fn, nt, n);
  MVD_CHECK_ARG(target || nt == 0, "%s: null target with nt=%zu", fn, nt);
  MVD_CHECK_ARG((index && normal && variation) || n == 0, "%s: null index, normal or variation with n=%zu", fn, n);
  MVD_CHECK_ARG(!toward || points || n == 0, "%s: toward without points", fn);
  const uintptr_t low = (uintptr_t)target | (uintptr_t)index | (uintptr_t)points | (uintptr_t)toward | (uintptr_t)normal | (uintptr_t)variation;
  MVD_CHECK_ARG((low & 3) == 0, "%s: a pointer that is not 4-byte aligned", fn);
  if (n > 0)
    hipLaunchKernelGGL(normals_kernel, dim3(cdiv((long)n, kPnThreads)), dim3(kPnThreads), 0, (hipStream_t)stream, target, (long long)nt, index,
                       (long long)n, k, points, toward, normal, variation);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}
