// Texturing a mesh from views: the per-face atlas, the bake and the lookup (include/mvd_hip.h: mvd_texture_bake has the rule in full).
//
// ATLAS (tex_owner, tex_corner): closed form, one chart per face, two faces per K x K cell, K = texels + 3.  Neither kernel searches and
// neither reads a texel-to-face table: a texel finds its face, and a face its three corners, by integer arithmetic.
// BAKE: one thread per texel.  A workgroup takes whole cells -- kTexThreads / K^2 of them, at least one, at most kTexMaxCells -- and
// stages the RESOLVED record of their faces in LDS first (three positions, the normal and its length, three colours, the class: 96 bytes
// per face, the way winding.hip stages its records): the (texels + 1)(texels + 2) / 2 + texels texels of a chart then read their face by
// LDS broadcast instead of three dependent global gathers each.  Texel t of the workgroup is (cell t / K^2, row, column): the lanes of
// a wavefront walk rows of K neighbouring texels, which project to neighbouring pixels of one view, so the depth and colour gathers of a
// row share cache lines, and the stores of a row are contiguous.  The camera record is uniform over the workgroup.  The view loop runs
// in ascending view order in every thread: sums in view order, no atomics, no scratch, one enqueue.
// SAMPLE: one thread per pixel of a mvd_render_mesh result.
//
// Not tried (the texture section): staging the projected corners of a chart per view to skip views a whole chart fails;
// one wavefront per chart; tiling the views' images through LDS.
#include "fusion_common.hpp"

namespace {

constexpr int kTexThreads = 256;
constexpr int kTexMaxCells = 16;                      // cells per workgroup at the smallest K = 4 (16 texels each)
constexpr int kTexMaxTexels = MVD_TEX_MAX_TEXELS;
constexpr int kTexMaxSide = MVD_TEX_MAX_SIDE;

enum { kTexOwned = 1, kTexIds = 2, kTexNormal = 4 };  // the class of a staged face: it exists; its ids are in range; its normal is usable

__host__ __device__ __forceinline__ bool tex_finite(float v) { return fabsf(v) < INFINITY; }      // (a NaN compares false)

// Which half of its cell owns cell-local texel (i, j): 0 the lower face, 1 the upper, -1 none.  (ii, jj) are the chart's own indices:
// (i, j) for the lower half, the point reflection (K - 1 - i, K - 1 - j) for the upper.  The two tests exclude each other:
// i + j <= T + 1 and i + j >= T + 3.
__host__ __device__ __forceinline__ int tex_owner(int i, int j, int T, int& ii, int& jj) {
  if (i <= T && j <= T && i + j <= T + 1) {
    ii = i, jj = j;
    return 0;
  }
  ii = T + 2 - i, jj = T + 2 - j;
  return (ii <= T && jj <= T && ii + jj <= T + 1) ? 1 : -1;
}

// The texel coordinates of the three corners of local face l.
__device__ __forceinline__ void tex_corners(int l, int T, int C, float* tx, float* ty) {
  const int K = T + 3, cell = l >> 1, ox = (cell % C) * K, oy = (cell / C) * K;
  if (l & 1) {
    tx[0] = (float)(ox + K - 1), ty[0] = (float)(oy + K - 1);
    tx[1] = (float)(ox + K - 1 - T), ty[1] = (float)(oy + K - 1);
    tx[2] = (float)(ox + K - 1), ty[2] = (float)(oy + K - 1 - T);
  } else {
    tx[0] = (float)ox, ty[0] = (float)oy;
    tx[1] = (float)(ox + T), ty[1] = (float)oy;
    tx[2] = (float)ox, ty[2] = (float)(oy + T);
  }
}

struct alignas(8) TexFaceRec {
  float v[9], n[3], nlen, col[9];
  int cls, pad;
};

struct BakeArgs {
  const float *vertices, *colors, *cams, *rgb, *depth;
  const int *faces, *vertex_start, *face_start;
  float* texture;
  unsigned char *views, *best;
  long long nvert, nface;
  int V, H, Pd, T, C, cells_per_group, cull, blend, power;
  float tol, min_cos, znear, fill[3];
};

__device__ __forceinline__ long long tex_clamp(int v, long long hi) { return min(max((long long)v, 0ll), hi); }

// blockIdx.y = scene, blockIdx.x = a run of cells_per_group cells of its atlas in cell order.
__global__ __launch_bounds__(kTexThreads) void texture_bake_kernel(BakeArgs a) {
  __shared__ TexFaceRec rec[2 * kTexMaxCells];
  const int scene = blockIdx.y, T = a.T, K = T + 3, KK = K * K, C = a.C, CC = C * C, A = C * K;
  const int c0 = blockIdx.x * a.cells_per_group, ncell = min(a.cells_per_group, CC - c0);
  const long long f0 = tex_clamp(a.face_start[scene], a.nface), f1 = tex_clamp(a.face_start[scene + 1], a.nface);
  const long long v0 = tex_clamp(a.vertex_start[scene], a.nvert), v1 = tex_clamp(a.vertex_start[scene + 1], a.nvert);
  for (int k = threadIdx.x; k < 2 * ncell; k += kTexThreads) {
    TexFaceRec r;
#pragma unroll
    for (int c = 0; c < 9; ++c) r.v[c] = 0.f, r.col[c] = 0.f;
    r.n[0] = r.n[1] = r.n[2] = r.nlen = 0.f;
    r.cls = 0, r.pad = 0;
    const long long f = f0 + 2ll * c0 + k;
    if (f < f1) {
      r.cls = kTexOwned;
      const int id[3] = {a.faces[f * 3 + 0], a.faces[f * 3 + 1], a.faces[f * 3 + 2]};
      if (id[0] >= v0 && id[0] < v1 && id[1] >= v0 && id[1] < v1 && id[2] >= v0 && id[2] < v1) {
        r.cls |= kTexIds;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            r.v[c * 3 + j] = a.vertices[(size_t)id[c] * 3 + j];
            if (a.colors) r.col[c * 3 + j] = a.colors[(size_t)id[c] * 3 + j];
          }
        const float e1[3] = {r.v[3] - r.v[0], r.v[4] - r.v[1], r.v[5] - r.v[2]}, e2[3] = {r.v[6] - r.v[0], r.v[7] - r.v[1], r.v[8] - r.v[2]};
        r.n[0] = e1[1] * e2[2] - e1[2] * e2[1];
        r.n[1] = e1[2] * e2[0] - e1[0] * e2[2];
        r.n[2] = e1[0] * e2[1] - e1[1] * e2[0];
        const float nn = (r.n[0] * r.n[0] + r.n[1] * r.n[1]) + r.n[2] * r.n[2];
        if (tex_finite(nn) && nn > 0.f) r.cls |= kTexNormal;
        r.nlen = sqrtf(nn);
      }
    }
    rec[k] = r;
  }
  __syncthreads();
  const size_t AA = (size_t)A * A;
  const float fT = (float)T, Pd2 = 0.5f * (float)a.Pd, Pdm = (float)a.Pd - 0.5f;
  for (int t = threadIdx.x; t < ncell * KK; t += kTexThreads) {
    const int cl = t / KK, rem = t - cl * KK, j = rem / K, i = rem - j * K, cell = c0 + cl;
    const int x = (cell % C) * K + i, y = (cell / C) * K + j;
    int ii, jj;
    const int h = tex_owner(i, j, T, ii, jj);
    float out[3] = {a.fill[0], a.fill[1], a.fill[2]};
    int nviews = 0, bestv = 255;
    const TexFaceRec* r = h >= 0 ? &rec[2 * cl + h] : nullptr;
    if (r && (r->cls & kTexIds)) {
      const float bb = (float)ii / fT, bc = (float)jj / fT, ba = (1.f - bb) - bc;
      if (a.colors) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = (ba * r->col[c] + bb * r->col[3 + c]) + bc * r->col[6 + c];
      }
      if (r->cls & kTexNormal) {
        float X[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) X[c] = (ba * r->v[c] + bb * r->v[3 + c]) + bc * r->v[6 + c];
        const float n[3] = {r->n[0], r->n[1], r->n[2]};
        float sw = 0.f, sc[3] = {0.f, 0.f, 0.f}, bw = -1.f, bcol[3] = {0.f, 0.f, 0.f};
        for (int v = 0; v < a.V; ++v) {
          const size_t cam_id = (size_t)scene * a.V + v;
          const Cam cam = load_cam(a.cams + cam_id * MVD_CAM_RECORD);
          float u, w, xc[3];
          project_xc(cam, X, u, w, xc);
          const float zc = xc[2];
          if (!(zc > a.znear && tex_finite(u) && tex_finite(w))) continue;
          const float cx = (1.f - u) * Pd2 - 0.5f, cy = (1.f - w) * Pd2 - 0.5f;
          if (!(cx >= -0.5f && cx <= Pdm && cy >= -0.5f && cy <= Pdm)) continue;
          const int dx = min((int)floorf(cx + 0.5f), a.Pd - 1), dy = min((int)floorf(cy + 0.5f), a.Pd - 1);      // (>= 0: cx + 0.5 >= 0)
          const float d = a.depth[(cam_id * a.Pd + dy) * a.Pd + dx];
          if (!(tex_finite(d) && zc <= d + a.tol)) continue;
          float nc[3];
#pragma unroll
          for (int q = 0; q < 3; ++q) nc[q] = n[0] * cam.R[0 * 3 + q] + n[1] * cam.R[1 * 3 + q] + n[2] * cam.R[2 * 3 + q];
          const float dot = (nc[0] * xc[0] + nc[1] * xc[1]) + nc[2] * xc[2];
          const float len = sqrtf((xc[0] * xc[0] + xc[1] * xc[1]) + xc[2] * xc[2]);
          float cosv = -dot / (r->nlen * len);
          if (!a.cull) cosv = fabsf(cosv);
          if (!(cosv > a.min_cos)) continue;
          float wt = 1.f;
          for (int p = 0; p < a.power; ++p) wt = wt * cosv;
          const PixelTaps taps = pixel_taps(u, w, a.H);
          float col[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float* img = a.rgb + (cam_id * 3 + c) * (size_t)a.H * a.H;
            const float z[4] = {img[taps.idx[0]], img[taps.idx[1]], img[taps.idx[2]], img[taps.idx[3]]};
            col[c] = bilinear_mix(z, taps);
          }
          ++nviews;
          sw += wt;
#pragma unroll
          for (int c = 0; c < 3; ++c) sc[c] += wt * col[c];
          if (wt > bw) {
            bw = wt, bestv = v;
#pragma unroll
            for (int c = 0; c < 3; ++c) bcol[c] = col[c];
          }
        }
        if (nviews > 0) {
#pragma unroll
          for (int c = 0; c < 3; ++c) out[c] = a.blend == MVD_TEX_BEST ? bcol[c] : sc[c] / sw;
        }
      }
    }
    const size_t o = (size_t)y * A + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) a.texture[((size_t)scene * 3 + c) * AA + o] = out[c];
    if (a.views) a.views[(size_t)scene * AA + o] = (unsigned char)nviews;
    if (a.best) a.best[(size_t)scene * AA + o] = (unsigned char)bestv;
  }
}

struct SampleArgs {
  const int *face_out, *face_start;
  const float *bary, *texture;
  float* rgb;
  long long nface;
  int M, P, T, C, filter;
  float bg[3];
};

// blockIdx.y = camera, blockIdx.x walks its P * P pixels.
__global__ __launch_bounds__(kTexThreads) void texture_sample_kernel(SampleArgs a) {
  const int cam_id = blockIdx.y, scene = cam_id / a.M, PP = a.P * a.P;
  const int rem = blockIdx.x * kTexThreads + threadIdx.x;
  if (rem >= PP) return;
  const int K = a.T + 3, A = a.C * K;
  const size_t AA = (size_t)A * A;
  const long long f0 = tex_clamp(a.face_start[scene], a.nface), f1 = tex_clamp(a.face_start[scene + 1], a.nface);
  const long long f = a.face_out[(size_t)cam_id * PP + rem], l = f - f0;
  float out[3] = {a.bg[0], a.bg[1], a.bg[2]};
  if (f >= f0 && f < f1 && l < 2ll * a.C * a.C) {
    float cx[3], cy[3], b[3];
    tex_corners((int)l, a.T, a.C, cx, cy);
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] = a.bary[((size_t)cam_id * 3 + c) * PP + rem];
    const float Am1 = (float)(A - 1);
    // (the clamp never moves a point of the chart; it keeps barycentrics that no rasteriser made inside the texture)
    const float tx = fminf(fmaxf((b[0] * cx[0] + b[1] * cx[1]) + b[2] * cx[2], 0.f), Am1);
    const float ty = fminf(fmaxf((b[0] * cy[0] + b[1] * cy[1]) + b[2] * cy[2], 0.f), Am1);
    const float* tex = a.texture + (size_t)scene * 3 * AA;
    if (a.filter == MVD_TEX_NEAREST) {
      const int x = min((int)floorf(tx + 0.5f), A - 1), y = min((int)floorf(ty + 0.5f), A - 1);
#pragma unroll
      for (int c = 0; c < 3; ++c) out[c] = tex[c * AA + (size_t)y * A + x];
    } else {
      PixelTaps t;
      const float x0f = floorf(tx), y0f = floorf(ty);
      const int x0 = (int)x0f, y0 = (int)y0f, x1 = min(x0 + 1, A - 1), y1 = min(y0 + 1, A - 1);
      t.wx = tx - x0f, t.wy = ty - y0f;
      t.idx[0] = y0 * A + x0, t.idx[1] = y0 * A + x1, t.idx[2] = y1 * A + x0, t.idx[3] = y1 * A + x1;
      const bool rd[4] = {true, t.wx != 0.f, t.wy != 0.f, t.wx != 0.f && t.wy != 0.f};      // a tap of weight exactly 0 is not read
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float z[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) z[k] = rd[k] ? tex[c * AA + t.idx[k]] : 0.f;
        out[c] = bilinear_mix(z, t);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) a.rgb[((size_t)cam_id * 3 + c) * PP + rem] = out[c];
}

static int tex_cells_per_row(size_t nface_max) {
  const size_t cells = (nface_max + 1) / 2;
  size_t C = (size_t)sqrt((double)cells);
  while (C * C < cells) ++C;
  while (C > 1 && (C - 1) * (C - 1) >= cells) --C;
  return (int)(C < 1 ? 1 : C);
}

// texels and the side A as a pair: A = C * (texels + 3) with C >= 1, inside the limits.  Returns C, or 0.
static int tex_check_side(int nscene, int texels, int A) {
  if (texels < 1 || texels > kTexMaxTexels || nscene < 1 || nscene > 65535 || A < 1 || A > kTexMaxSide) return 0;
  const int K = texels + 3;
  if (A % K) return 0;
  if ((unsigned long long)nscene * A * A >= 0x80000000ull) return 0;
  return A / K;
}

}  // namespace

extern "C" int mvd_texture_atlas_side(size_t nface_max, int texels, int nscene) {
  if (texels < 1 || texels > kTexMaxTexels || nface_max > 0x7fffffffull) return 0;
  const long long A = (long long)tex_cells_per_row(nface_max) * (texels + 3);
  return A <= kTexMaxSide && tex_check_side(nscene, texels, (int)A) ? (int)A : 0;
}

extern "C" int mvd_texture_bake(const float* vertices, const float* colors, const int* faces, const int* vertex_start, const int* face_start,
                                const float* cams, const float* rgb, const float* depth, size_t nvert, size_t nface, int nscene, int V, int H,
                                int Pd, int texels, int A, float tol, float min_cos, int power, int cull, int blend, float znear,
                                const float* fill, float* texture, unsigned char* views, unsigned char* best, mvd_stream_t stream) {
  const char* fn = "mvd_texture_bake";
  MVD_CHECK_ARG(nface <= 0x7fffffffull && nvert <= 0x7fffffffull, "%s: nface=%zu, nvert=%zu beyond 2^31 - 1", fn, nface, nvert);
  MVD_CHECK_ARG((vertices && faces) || nface == 0, "%s: null vertices or faces with nface=%zu", fn, nface);
  MVD_CHECK_ARG(vertex_start && face_start && cams && rgb && depth && fill && texture, "%s: null pointer", fn);
  MVD_CHECK_ARG(nscene >= 1 && nscene <= 65535, "%s: nscene=%d outside [1, 65535]", fn, nscene);
  MVD_CHECK_ARG(V >= 1 && V <= MVD_TEX_MAX_VIEWS, "%s: V=%d outside [1, %d]", fn, V, MVD_TEX_MAX_VIEWS);
  MVD_CHECK_ARG(H >= 1 && H <= 32768 && Pd >= 1 && Pd <= 32768, "%s: H=%d, Pd=%d outside [1, 32768]", fn, H, Pd);
  MVD_CHECK_ARG(texels >= 1 && texels <= kTexMaxTexels, "%s: texels=%d outside [1, %d]", fn, texels, kTexMaxTexels);
  const int C = tex_check_side(nscene, texels, A);
  MVD_CHECK_ARG(C >= 1, "%s: A=%d is no atlas side for texels=%d, nscene=%d (a multiple of texels + 3, <= %d, nscene * A^2 < 2^31)", fn, A,
                texels, nscene, kTexMaxSide);
  MVD_CHECK_ARG(tol >= 0.f && tol < INFINITY, "%s: tol=%g (finite, >= 0)", fn, (double)tol);
  MVD_CHECK_ARG(min_cos >= 0.f && min_cos < 1.f, "%s: min_cos=%g outside [0, 1)", fn, (double)min_cos);
  MVD_CHECK_ARG(power >= 0 && power <= 8, "%s: power=%d outside [0, 8]", fn, power);
  MVD_CHECK_ARG(cull == 0 || cull == 1, "%s: cull=%d (0 or 1)", fn, cull);
  MVD_CHECK_ARG(blend == MVD_TEX_MEAN || blend == MVD_TEX_BEST, "%s: blend=%d (MVD_TEX_MEAN or MVD_TEX_BEST)", fn, blend);
  MVD_CHECK_ARG(znear >= 0.f, "%s: znear=%g (>= 0)", fn, (double)znear);
  const int KK = (texels + 3) * (texels + 3);
  const int per = min(max(kTexThreads / KK, 1), kTexMaxCells);
  BakeArgs a{vertices, colors, cams, rgb, depth, faces, vertex_start, face_start, texture, views, best, (long long)nvert, (long long)nface,
             V, H, Pd, texels, C, per, cull, blend, power, tol, min_cos, znear, {fill[0], fill[1], fill[2]}};
  hipLaunchKernelGGL(texture_bake_kernel, dim3(cdiv((long)C * C, per), nscene), dim3(kTexThreads), 0, (hipStream_t)stream, a);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int mvd_texture_sample(const int* face_out, const float* bary, const int* face_start, const float* texture, size_t nface, int nscene,
                                  int M, int P, int texels, int A, int filter, const float* background, float* rgb, mvd_stream_t stream) {
  const char* fn = "mvd_texture_sample";
  MVD_CHECK_ARG(face_out && bary && face_start && texture && background && rgb, "%s: null pointer", fn);
  MVD_CHECK_ARG(nface <= 0x7fffffffull, "%s: nface=%zu beyond 2^31 - 1", fn, nface);
  MVD_CHECK_ARG(nscene >= 1 && M >= 1 && (unsigned long long)nscene * M <= 65535ull, "%s: nscene=%d, M=%d (>= 1, nscene * M <= 65535)", fn,
                nscene, M);
  MVD_CHECK_ARG(P >= 1 && P <= 46340 && (unsigned long long)nscene * M * P * P <= 0x7fffffffull,
                "%s: nscene * M * P^2 pixels outside [1, 2^31 - 1] (nscene=%d, M=%d, P=%d)", fn, nscene, M, P);
  MVD_CHECK_ARG(texels >= 1 && texels <= kTexMaxTexels, "%s: texels=%d outside [1, %d]", fn, texels, kTexMaxTexels);
  const int C = tex_check_side(nscene, texels, A);
  MVD_CHECK_ARG(C >= 1, "%s: A=%d is no atlas side for texels=%d, nscene=%d (a multiple of texels + 3, <= %d, nscene * A^2 < 2^31)", fn, A,
                texels, nscene, kTexMaxSide);
  MVD_CHECK_ARG(filter == MVD_TEX_NEAREST || filter == MVD_TEX_BILINEAR, "%s: filter=%d (MVD_TEX_NEAREST or MVD_TEX_BILINEAR)", fn, filter);
  SampleArgs a{face_out, face_start, bary, texture, rgb, (long long)nface, M, P, texels, C, filter, {background[0], background[1], background[2]}};
  hipLaunchKernelGGL(texture_sample_kernel, dim3(cdiv((long)P * P, kTexThreads), nscene * M), dim3(kTexThreads), 0, (hipStream_t)stream, a);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}
