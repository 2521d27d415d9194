// Rendering a triangle mesh into cameras: z-buffered rasterisation (include/mvd_hip.h: mvd_render_mesh has the rule in full).
//
// The z-buffer is filled with ones -> raster_kernel: one thread sets up one (face, camera) pair -- the three vertices through project_z
// (fusion_common.hpp), the pixel-centre convention of the point renderer's splat kernel, the drop rules, the bounding box clipped to the
// image.  A thread whose box has at most kThreadBox pixels walks it itself; at the sizes extract_mesh produces a face covers about one pixel
// and this is the whole kernel.  Larger boxes are handed to the wavefront: a ballot collects the flagged lanes, which are taken one at a
// time; the face set-up is broadcast by cross-lane reads and the 64 lanes stride over the box's pixels, so a triangle across the whole
// image costs P^2 / 64 iterations, not P^2 in one lane.  Every covered pixel takes one 64-bit unsigned atomicMin of
// (depth bits << 32 | face id) behind the splat kernel's early-out load -> resolve_kernel: one thread per pixel unpacks the winner and
// evaluates it again through the SAME two device functions (face_setup, pixel_eval), so what it writes belongs to the key that won.
// The minimum of a set does not depend on the order its members arrive in: the outputs are the same bits run to run.
//
// Not tried: LDS tiling, binning, a hierarchical z-buffer.
#include "fusion_common.hpp"

namespace {

constexpr int kRasterThreads = 256;
constexpr int kThreadBox = 64;                        // a clipped bounding box of at most this many pixels is walked by its own thread
constexpr unsigned long long kEmptyKey = ~0ull;

struct MeshArgs {
  const float *vertices, *colors, *cams;
  const int *faces, *vertex_start, *face_start;
  unsigned long long* zbuf;
  int* face_out;
  float *depth, *bary, *normal, *rgb;
  long long nvert, nface;
  int M, P, cull;
  float znear, empty_depth, bg[3];
};

// One (face, camera) pair after projection: pixel coordinates and camera z of the three vertices, area2, and the clipped bounding box.
struct FaceSetup {
  float ax, ay, bx, by, cx, cy, za, zb, zc, area2;
  int x0, y0, w, h;                                   // the box's first pixel, its width and height (>= 1 each when the pair draws)
};

__device__ __forceinline__ bool is_finite(float v) { return fabsf(v) < INFINITY; }      // (a NaN compares false)

// The scene's face and vertex ranges, clamped: never read past the arrays whatever the device tables hold.
struct SceneRange {
  long long f0, f1, v0, v1;
};
__device__ __forceinline__ SceneRange scene_range(const MeshArgs& a, int scene) {
  SceneRange r;
  r.f0 = min(max((long long)a.face_start[scene], 0ll), a.nface);
  r.f1 = min(max((long long)a.face_start[scene + 1], 0ll), a.nface);
  r.v0 = min(max((long long)a.vertex_start[scene], 0ll), a.nvert);
  r.v1 = min(max((long long)a.vertex_start[scene + 1], 0ll), a.nvert);
  return r;
}

// THE drop rules of the header, in its order.  f must lie in [0, nface); ids[] receives the three vertex ids (valid when it returns true).
__device__ __forceinline__ bool face_setup(const MeshArgs& a, const Cam& cam, const SceneRange& r, long long f, FaceSetup& s, int* ids) {
  ids[0] = a.faces[f * 3 + 0];
  ids[1] = a.faces[f * 3 + 1];
  ids[2] = a.faces[f * 3 + 2];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (!(ids[k] >= r.v0 && ids[k] < r.v1)) return false;
  float px[3], py[3], z[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float* v = a.vertices + (size_t)ids[k] * 3;
    const float X[3] = {v[0], v[1], v[2]};
    float u, w;
    project_z(cam, X, u, w, z[k]);
    const float P2 = 0.5f * (float)a.P;
    px[k] = (1.f - u) * P2 - 0.5f;                     // the splat kernel's pixel coordinates: pixel (x, y) has its centre at (x, y)
    py[k] = (1.f - w) * P2 - 0.5f;
  }
  if (!(z[0] > a.znear && z[1] > a.znear && z[2] > a.znear)) return false;          // no near-plane clipping: dropped whole
  if (!(is_finite(px[0]) && is_finite(py[0]) && is_finite(px[1]) && is_finite(py[1]) && is_finite(px[2]) && is_finite(py[2]))) return false;
  s.ax = px[0], s.ay = py[0], s.bx = px[1], s.by = py[1], s.cx = px[2], s.cy = py[2];
  s.za = z[0], s.zb = z[1], s.zc = z[2];
  s.area2 = (s.bx - s.ax) * (s.cy - s.ay) - (s.by - s.ay) * (s.cx - s.ax);
  if (!(is_finite(s.area2) && s.area2 != 0.f)) return false;
  if (a.cull && !(s.area2 < 0.f)) return false;        // front faces have area2 < 0 (header: the derivation)
  // the integer pixels of the bounding box, clipped to the image BEFORE the conversion to int
  const float x0 = fmaxf(ceilf(fminf(fminf(s.ax, s.bx), s.cx)), 0.f), x1 = fminf(floorf(fmaxf(fmaxf(s.ax, s.bx), s.cx)), (float)(a.P - 1));
  const float y0 = fmaxf(ceilf(fminf(fminf(s.ay, s.by), s.cy)), 0.f), y1 = fminf(floorf(fmaxf(fmaxf(s.ay, s.by), s.cy)), (float)(a.P - 1));
  if (!(x0 <= x1 && y0 <= y1)) return false;
  s.x0 = (int)x0, s.y0 = (int)y0, s.w = (int)x1 - s.x0 + 1, s.h = (int)y1 - s.y0 + 1;      // w * h <= P * P < 2^31
  return true;
}

// THE evaluation order of coverage, depth and barycentrics at pixel (x, y).  Returns whether the pixel is drawn; z and b[] are valid then.
__device__ __forceinline__ bool pixel_eval(const FaceSetup& s, float znear, int x, int y, float& z, float* b) {
  const float fx = (float)x, fy = (float)y;
  const float ea = (s.bx - fx) * (s.cy - fy) - (s.by - fy) * (s.cx - fx);
  const float eb = (s.cx - fx) * (s.ay - fy) - (s.cy - fy) * (s.ax - fx);
  const float ec = (s.ax - fx) * (s.by - fy) - (s.ay - fy) * (s.bx - fx);
  const float sg = s.area2 > 0.f ? 1.f : -1.f;
  if (!(ea * sg >= 0.f && eb * sg >= 0.f && ec * sg >= 0.f)) return false;      // edges inclusive, no top-left rule: the z-buffer decides
  const float qa = (ea / s.area2) / s.za, qb = (eb / s.area2) / s.zb, qc = (ec / s.area2) / s.zc;
  const float iz = (qa + qb) + qc;
  z = 1.f / iz;
  b[0] = qa * z, b[1] = qb * z, b[2] = qc * z;
  return is_finite(z) && z > znear;
}

__device__ __forceinline__ void zbuf_min(unsigned long long* cell, unsigned long long key) {
  if (*cell <= key) return;      // keys only decrease: a stale read costs an unnecessary atomic, never a wrong result (fusion.hip: splat_kernel)
  atomicMin(cell, key);
}

__device__ __forceinline__ float lane_f(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
__device__ __forceinline__ int lane_i(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

// blockIdx.y = scene * M + camera: the camera record and the scene's ranges are uniform; blockIdx.x walks the scene's faces, blocks past
// them exit.  No lane leaves before the wavefront loop: the ballot and the cross-lane reads need the whole wavefront.
__global__ __launch_bounds__(kRasterThreads) void raster_kernel(MeshArgs a) {
  const int cam_id = blockIdx.y, scene = cam_id / a.M, P = a.P;
  const SceneRange r = scene_range(a, scene);
  if (r.f0 + (long long)blockIdx.x * kRasterThreads >= r.f1) return;      // (uniform)
  const long long f = r.f0 + (long long)blockIdx.x * kRasterThreads + threadIdx.x;
  const Cam cam = load_cam(a.cams + (size_t)cam_id * MVD_CAM_RECORD);
  unsigned long long* zb = a.zbuf + (size_t)cam_id * P * P;
  FaceSetup s = {};
  int ids[3];
  const bool draws = f < r.f1 && face_setup(a, cam, r, f, s, ids);
  const unsigned fid = (unsigned)f;
  const bool small = s.w * s.h <= kThreadBox;
  if (draws && small) {
    for (int y = s.y0; y < s.y0 + s.h; ++y)
      for (int x = s.x0; x < s.x0 + s.w; ++x) {
        float z, b[3];
        if (pixel_eval(s, a.znear, x, y, z, b)) zbuf_min(zb + (size_t)y * P + x, ((unsigned long long)__float_as_uint(z) << 32) | fid);
      }
  }
  unsigned long long big = __ballot(draws && !small);
  while (big) {      // (uniform: every lane of the wavefront walks the same list)
    const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)big) - 1);
    big &= big - 1;
    FaceSetup t;
    t.ax = lane_f(s.ax, src), t.ay = lane_f(s.ay, src), t.bx = lane_f(s.bx, src), t.by = lane_f(s.by, src);
    t.cx = lane_f(s.cx, src), t.cy = lane_f(s.cy, src), t.za = lane_f(s.za, src), t.zb = lane_f(s.zb, src), t.zc = lane_f(s.zc, src);
    t.area2 = lane_f(s.area2, src);
    t.x0 = lane_i(s.x0, src), t.y0 = lane_i(s.y0, src), t.w = lane_i(s.w, src), t.h = lane_i(s.h, src);
    const unsigned tf = (unsigned)lane_i((int)fid, src);
    for (int p = threadIdx.x & 63; p < t.w * t.h; p += 64) {
      const int x = t.x0 + p % t.w, y = t.y0 + p / t.w;
      float z, b[3];
      if (pixel_eval(t, a.znear, x, y, z, b)) zbuf_min(zb + (size_t)y * P + x, ((unsigned long long)__float_as_uint(z) << 32) | tf);
    }
  }
}

// blockIdx.y = camera (uniform record), blockIdx.x walks its P * P pixels.  A z-buffer of the caller's is not trusted: a winner that is no
// face of the camera's scene, or that does not draw the pixel, reads as empty.
__global__ __launch_bounds__(kRasterThreads) void mesh_resolve_kernel(MeshArgs a) {
  const int cam_id = blockIdx.y, scene = cam_id / a.M, P = a.P, PP = P * P;
  const int rem = blockIdx.x * kRasterThreads + threadIdx.x;
  if (rem >= PP) return;
  const size_t pix = (size_t)cam_id * PP + rem;
  const unsigned long long key = a.zbuf[pix];
  const long long f = (long long)(key & 0xffffffffull);
  const SceneRange r = scene_range(a, scene);
  FaceSetup s;
  int ids[3];
  float z = 0.f, b[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f};
  bool hit = key != kEmptyKey && f >= r.f0 && f < r.f1;
  if (hit) {
    const Cam cam = load_cam(a.cams + (size_t)cam_id * MVD_CAM_RECORD);
    hit = face_setup(a, cam, r, f, s, ids) && pixel_eval(s, a.znear, rem % P, rem / P, z, b);
    if (hit) {
      // the unit normal: (b - a) x (c - a) in world space, divided by its largest component, rotated, normalised, turned to normal_z <= 0
      const float *va = a.vertices + (size_t)ids[0] * 3, *vb = a.vertices + (size_t)ids[1] * 3, *vc = a.vertices + (size_t)ids[2] * 3;
      const float e1[3] = {vb[0] - va[0], vb[1] - va[1], vb[2] - va[2]}, e2[3] = {vc[0] - va[0], vc[1] - va[1], vc[2] - va[2]};
      float nw[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
      const float big = fmaxf(fmaxf(fabsf(nw[0]), fabsf(nw[1])), fabsf(nw[2]));
      if (big > 0.f && is_finite(big)) {
#pragma unroll
        for (int j = 0; j < 3; ++j) nw[j] = nw[j] / big;
#pragma unroll
        for (int j = 0; j < 3; ++j) n[j] = nw[0] * cam.R[0 * 3 + j] + nw[1] * cam.R[1 * 3 + j] + nw[2] * cam.R[2 * 3 + j];
        const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
        const float sg = n[2] > 0.f ? -1.f : 1.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) n[j] = (n[j] / len) * sg;
      }
    }
  }
  a.face_out[pix] = hit ? (int)f : -1;
  a.depth[pix] = hit ? __uint_as_float((unsigned)(key >> 32)) : a.empty_depth;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const size_t o = ((size_t)cam_id * 3 + c) * PP + rem;
    a.bary[o] = hit ? b[c] : 0.f;
    a.normal[o] = hit ? n[c] : 0.f;
  }
  if (a.colors) {
    float col[3] = {a.bg[0], a.bg[1], a.bg[2]};
    if (hit) {
      const float *ca = a.colors + (size_t)ids[0] * 3, *cb = a.colors + (size_t)ids[1] * 3, *cc = a.colors + (size_t)ids[2] * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) col[c] = (b[0] * ca[c] + b[1] * cb[c]) + b[2] * cc[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) a.rgb[((size_t)cam_id * 3 + c) * PP + rem] = col[c];
  }
}

}  // namespace

extern "C" size_t mvd_render_mesh_scratch(int ncam, int P) {
  return ncam >= 1 && P >= 1 ? (size_t)ncam * P * P * sizeof(unsigned long long) : 0;
}

extern "C" int mvd_render_mesh_stages(const float* vertices, const float* colors, const int* faces, const int* vertex_start,
                                      const int* face_start, const float* cams, size_t nvert, size_t nface, int nscene, int M, int P, int cull,
                                      float znear, float empty_depth, const float* background, int* face_out, float* depth, float* bary,
                                      float* normal, float* rgb, void* scratch, size_t scratch_bytes, int stages, mvd_stream_t stream) {
  const char* fn = stages == MVD_RENDER_ALL ? "mvd_render_mesh" : "mvd_render_mesh_stages";
  MVD_CHECK_ARG(stages >= 1 && stages <= MVD_RENDER_ALL, "%s: stages=%d outside [1, %d]", fn, stages, MVD_RENDER_ALL);
  MVD_CHECK_ARG(nface <= 0x7fffffffull && nvert <= 0x7fffffffull, "%s: nface=%zu, nvert=%zu beyond 2^31 - 1", fn, nface, nvert);
  MVD_CHECK_ARG((vertices && faces) || nface == 0, "%s: null vertices or faces with nface=%zu", fn, nface);
  MVD_CHECK_ARG(vertex_start && face_start && cams && face_out && depth && bary && normal && scratch, "%s: null pointer", fn);
  MVD_CHECK_ARG(!colors == !rgb, "%s: colors and rgb go together", fn);
  MVD_CHECK_ARG(!colors || background, "%s: colors without a background", fn);
  MVD_CHECK_ARG(nscene >= 1 && M >= 1 && (unsigned long long)nscene * M <= 65535ull, "%s: nscene=%d, M=%d (>= 1, nscene * M <= 65535)", fn,
                nscene, M);
  MVD_CHECK_ARG(P >= 1 && P <= 46340 && (unsigned long long)nscene * M * P * P <= 0x7fffffffull,
                "%s: nscene * M * P^2 pixels outside [1, 2^31 - 1] (nscene=%d, M=%d, P=%d)", fn, nscene, M, P);
  MVD_CHECK_ARG(cull == 0 || cull == 1, "%s: cull=%d (0 or 1)", fn, cull);
  MVD_CHECK_ARG(znear >= 0.f, "%s: znear=%g (>= 0)", fn, (double)znear);
  const int ncam = nscene * M;
  MVD_CHECK_ARG(scratch_bytes >= mvd_render_mesh_scratch(ncam, P) && ((uintptr_t)scratch & 7) == 0,
                "%s: scratch of %zu bytes (needs %zu, 8-byte aligned)", fn, scratch_bytes, mvd_render_mesh_scratch(ncam, P));
  MeshArgs a{vertices, colors, cams, faces, vertex_start, face_start, (unsigned long long*)scratch, face_out, depth, bary, normal, rgb,
             (long long)nvert, (long long)nface, M, P, cull, znear, empty_depth, {0.f, 0.f, 0.f}};
  if (colors)
    for (int c = 0; c < 3; ++c) a.bg[c] = background[c];
  if (stages & MVD_RENDER_FILL) {
    const hipError_t e = hipMemsetAsync(scratch, 0xff, (size_t)ncam * P * P * sizeof(unsigned long long), (hipStream_t)stream);
    MVD_CHECK_ARG(e == hipSuccess, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
  }
  if ((stages & MVD_RENDER_SPLAT) && nface > 0)      // a scene has at most nface faces: blocks past its range exit
    hipLaunchKernelGGL(raster_kernel, dim3(cdiv((long)nface, kRasterThreads), ncam), dim3(kRasterThreads), 0, (hipStream_t)stream, a);
  if (stages & MVD_RENDER_RESOLVE)
    hipLaunchKernelGGL(mesh_resolve_kernel, dim3(cdiv((long)P * P, kRasterThreads), ncam), dim3(kRasterThreads), 0, (hipStream_t)stream, a);
  MVD_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int mvd_render_mesh(const float* vertices, const float* colors, const int* faces, const int* vertex_start, const int* face_start,
                               const float* cams, size_t nvert, size_t nface, int nscene, int M, int P, int cull, float znear,
                               float empty_depth, const float* background, int* face_out, float* depth, float* bary, float* normal, float* rgb,
                               void* scratch, size_t scratch_bytes, mvd_stream_t stream) {
  return mvd_render_mesh_stages(vertices, colors, faces, vertex_start, face_start, cams, nvert, nface, nscene, M, P, cull, znear, empty_depth,
                                background, face_out, depth, bary, normal, rgb, scratch, scratch_bytes, MVD_RENDER_ALL, stream);
}
