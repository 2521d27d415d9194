// GridAttn front end (mvdfusion/view_attn_efficient2.py:269-370, 413-437): z-embedding of the latents and the fused
// depth-sample -> unproject -> reproject -> bilinear gather -> Plucker/harmonic embedding kernel that writes the token
// matrix consumed by the aggregation transformer's first GEMM, and that kernel's backward (the scatter into the feature maps).
//
// One wavefront per 3-D query point ([scene,] query view b, pixel, depth sample d); it loops over the point's reference view slots -- the
// V views of the rig, or with a window (mvd_gridattn_tokens_window) b's W rig neighbours -- and
// writes one coalesced 736-float row per slot: lanes own 4 feature channels each (float4 gathers from the
// channels-last feature maps, which stay L2/MALL resident: (V+1) x S x S x 256 fp32 = 1 MB per view), and the 210
// sin/cos embedding values are spread over the lanes.
// Where the point lies, which views its slots are and where it falls in them is gridattn_common.hpp (decode_point, world_point,
// for_each_slot, view_taps), shared with the fused kernel; this file is what the two kernels do with a point: embed and store, or scatter.
#include "gridattn_common.hpp"

namespace {

// harmonic embedding value e of a `dim`-vector: layout [sin(dim*7) | cos(dim*7) | x(dim)], index dim_i*7 + k
// (ocml sinf / cosf; the fused kernel has its own branch-free sin / cos -- see gridattn_common.hpp before merging the two)
__device__ __forceinline__ float harmonic(const float* vec, int dim, int e) {
  const int n = dim * 7;
  if (e >= 2 * n) return vec[e - 2 * n];
  const int ee = e < n ? e : e - n;
  const int di = ee / 7, k = ee - di * 7;
  const float w = 0.1f * (float)(1 << k);  // fl(0.1) * 2^k, as torch computes (2.0**arange(7)) * 0.1
  const float a = vec[di] * w;
  return e < n ? sinf(a) : cosf(a);
}
// this lane's two values (e = lane, lane + 64; the second is 0 beyond 105) of the 105-wide embedding [Plucker 90 | depth 15]
__device__ __forceinline__ void embed105(const Plucker& pl, float depth, int lane, float& v0, float& v1) {
  const float p6[6] = {pl.a, pl.b, pl.c, pl.d, pl.e, pl.f}, dp[1] = {depth};
  const int e0 = lane, e1 = lane + 64;
  v0 = e0 < 90 ? harmonic(p6, 6, e0) : harmonic(dp, 1, e0 - 90);
  v1 = e1 >= 105 ? 0.f : e1 < 90 ? harmonic(p6, 6, e1) : harmonic(dp, 1, e1 - 90);
}

__global__ __launch_bounds__(256) void tokens_kernel(GridGeom g, const float* __restrict__ feat, const float* __restrict__ in_feat,
                                                     u16* __restrict__ tok) {
  const int lane = threadIdx.x & 63;
  const int S = g.S, SS = S * S, W = slots_per_point(g);
  const size_t pt = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // one wavefront per point: pt is wave-uniform
  if (pt >= num_points(g)) return;
  const GeomPoint q = decode_point(g, pt, wave_scene(g, pt));
  // ---- G1: depth sample and world point; query-side embedding (same for every reference view)
  const Cam cb = view_cam(g, q, q.b);
  float X[3], dir[3];
  const float depth = world_point(g, q, cb, X, dir);
  float qe0, qe1;
  embed105(plucker(dir[0], dir[1], dir[2], cb.C), depth, lane, qe0, qe1);
  // ---- input-view gather (same for every reference view)  (:320-331)
  const float4 fin = bilinear4(in_feat + (size_t)q.scene * SS * 256, view_taps(input_cam(g, q), X, S), lane * 4);
  // ---- per reference view slot (wave-uniform)
  for_each_slot(g, q.b, [&](int slot, int vr) {
    const Cam cv = view_cam(g, q, vr);
    const float4 fr = bilinear4(feat + (size_t)(q.gv0 + vr) * SS * 256, view_taps(cv, X, S), lane * 4);
    const Plucker rpl = plucker_to(cv, X);
    float re0, re1;
    embed105(rpl, rpl.norm, lane, re0, re1);
    const size_t row = pt * W + slot;
    store_sp4(tok, row, MVD_TOKEN_LD, lane * 4, fr.x, fr.y, fr.z, fr.w);
    store_sp4(tok, row, MVD_TOKEN_LD, 256 + lane * 4, fin.x, fin.y, fin.z, fin.w);
    store_sp1(tok, row, MVD_TOKEN_LD, 512 + lane, re0);
    if (lane + 64 < 105) store_sp1(tok, row, MVD_TOKEN_LD, 512 + lane + 64, re1);
    store_sp1(tok, row, MVD_TOKEN_LD, 617 + lane, qe0);
    if (lane + 64 < 105) store_sp1(tok, row, MVD_TOKEN_LD, 617 + lane + 64, qe1);
    if (lane < MVD_TOKEN_LD - 722) store_sp1(tok, row, MVD_TOKEN_LD, 722 + lane, lane == 0 ? 1.0f : 0.0f);  // mask = 1, zero pad
  });
}

// Linear(5 -> 256) + GELU per pixel; lat (N,5,S,S) NCHW -> feat (N,S,S,256) NHWC; one wave per pixel
__global__ __launch_bounds__(256) void zembed_kernel(const float* __restrict__ lat, const float* __restrict__ w,
                                                     const float* __restrict__ bias, float* __restrict__ feat, int N, int SS) {
  const int lane = threadIdx.x & 63;
  const size_t p = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= (size_t)N * SS) return;
  const int n = (int)(p / SS), pix = (int)(p % SS);
  float in[5];
#pragma unroll
  for (int c = 0; c < 5; ++c) in[c] = lat[((size_t)n * 5 + c) * SS + pix];
  float o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ch = lane * 4 + j;
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < 5; ++c) a += in[c] * w[ch * 5 + c];
    o[j] = gelu_erf(a + bias[ch]);
  }
  *(float4*)(feat + p * 256 + lane * 4) = make_float4(o[0], o[1], o[2], o[3]);
}

// ------------------------------------------------------------------------------------------------ token kernel backward
// Gradient of the token matrix's two gathered blocks w.r.t. the feature maps (F.grid_sample backward w.r.t. its input;
// view_attn_efficient2.py:320-341): dtok (T, ldt) fp32 = dL/d tokens from the first GEMM's dgrad; columns [0, 256) were
// bilinear samples of feat[vr], [256, 512) of in_feat.  Scatter with the forward's taps and weights (the same view_taps of the same
// world_point: gridattn_common.hpp) into 64-bit fixed-point accumulators (value * scale, integer atomics: order independent =>
// bit-reproducible), converted by the caller.
// The sampling positions depend only on data (noisy latents, cameras), never on parameters: no gradient flows there.
__device__ __forceinline__ void scatter4(long long* __restrict__ acc, const Taps& t, int ch, float4 g, float scale) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (t.pix[k] < 0) continue;
    unsigned long long* p = (unsigned long long*)(acc + (size_t)t.pix[k] * 256 + ch);
    const float w = t.w[k] * scale;
    atomicAdd(p + 0, (unsigned long long)(long long)llrintf(g.x * w));
    atomicAdd(p + 1, (unsigned long long)(long long)llrintf(g.y * w));
    atomicAdd(p + 2, (unsigned long long)(long long)llrintf(g.z * w));
    atomicAdd(p + 3, (unsigned long long)(long long)llrintf(g.w * w));
  }
}

__global__ __launch_bounds__(256) void tokens_bwd_kernel(GridGeom g, const float* __restrict__ dtok, int ldt, long long* __restrict__ dfeat,
                                                         long long* __restrict__ din_feat, float scale) {
  const int lane = threadIdx.x & 63;
  const int S = g.S, SS = S * S, W = slots_per_point(g);
  const size_t pt = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pt >= num_points(g)) return;
  const GeomPoint q = decode_point(g, pt, wave_scene(g, pt));
  float X[3], dir[3];
  world_point(g, q, view_cam(g, q, q.b), X, dir);
  float4 gin = make_float4(0.f, 0.f, 0.f, 0.f);
  for_each_slot(g, q.b, [&](int slot, int vr) {      // the forward's slots: row pt * W + slot was gathered from view vr
    const float* row = dtok + (pt * W + slot) * (size_t)ldt;
    const float4 gr = *(const float4*)(row + lane * 4);
    scatter4(dfeat + (size_t)(q.gv0 + vr) * SS * 256, view_taps(view_cam(g, q, vr), X, S), lane * 4, gr, scale);
    const float4 gi = *(const float4*)(row + 256 + lane * 4);     // the input-view block is the same sample in all the point's rows
    gin.x += gi.x; gin.y += gi.y; gin.z += gi.z; gin.w += gi.w;
  });
  scatter4(din_feat + (size_t)q.scene * SS * 256, view_taps(input_cam(g, q), X, S), lane * 4, gin, scale);
}

}  // namespace

extern "C" int mvd_zembed(const float* lat, const float* w, const float* b, float* feat, int N, int S, mvd_stream_t stream) {
  MVD_CHECK_ARG(lat && w && b && feat && N > 0 && S > 0, "mvd_zembed: bad arguments");
  const size_t npix = (size_t)N * S * S;
  hipLaunchKernelGGL(zembed_kernel, dim3(cdiv(npix, 4)), dim3(256), 0, (hipStream_t)stream, lat, w, b, feat, N, S * S);
  MVD_CHECK_LAUNCH("mvd_zembed");
  return 0;
}

extern "C" int mvd_gridattn_tokens_window(const float* x, const float* depth_noise, const float* steps, const int* iter,
                                          const float* grid_lin, const float* feat, const float* in_feat, const float* cams,
                                          const float* in_cam, void* tokens_sp, int nscene, int V, int q0, int Vq, int S, int D,
                                          float depth_scale, float depth_shift, int steps_scene_stride, int window, mvd_stream_t stream) {
  const GridGeom g = {x, depth_noise, steps, iter, grid_lin, cams, in_cam, nscene, V, q0, Vq, S, D, depth_scale, depth_shift, steps_scene_stride, window};
  if (const int e = check_geom("mvd_gridattn_tokens_window", g)) return e;
  MVD_CHECK_ARG(feat && in_feat && tokens_sp, "mvd_gridattn_tokens_window: null pointer");
  const size_t npts = num_points(g);      // one wavefront per point: a point never straddles two scenes
  MVD_CHECK_ARG((npts + 3) / 4 <= 0x7fffffff, "mvd_gridattn_tokens_window: grid too large");
  hipLaunchKernelGGL(tokens_kernel, dim3(cdiv(npts, 4)), dim3(256), 0, (hipStream_t)stream, g, feat, in_feat, (u16*)tokens_sp);
  MVD_CHECK_LAUNCH("mvd_gridattn_tokens_window");
  return 0;
}

extern "C" int mvd_gridattn_tokens_scenes_t(const float* x, const float* depth_noise, const float* steps, const int* iter,
                                            const float* grid_lin, const float* feat, const float* in_feat, const float* cams,
                                            const float* in_cam, void* tokens_sp, int nscene, int V, int q0, int Vq, int S, int D,
                                            float depth_scale, float depth_shift, int steps_scene_stride, mvd_stream_t stream) {
  return mvd_gridattn_tokens_window(x, depth_noise, steps, iter, grid_lin, feat, in_feat, cams, in_cam, tokens_sp, nscene, V, q0, Vq, S, D,
                                    depth_scale, depth_shift, steps_scene_stride, 0, stream);
}

extern "C" int mvd_gridattn_tokens_scenes(const float* x, const float* depth_noise, const float* steps, const int* iter,
                                          const float* grid_lin, const float* feat, const float* in_feat, const float* cams,
                                          const float* in_cam, void* tokens_sp, int nscene, int V, int q0, int Vq, int S, int D,
                                          float depth_scale, float depth_shift, mvd_stream_t stream) {
  return mvd_gridattn_tokens_scenes_t(x, depth_noise, steps, iter, grid_lin, feat, in_feat, cams, in_cam, tokens_sp, nscene, V, q0, Vq, S,
                                      D, depth_scale, depth_shift, 0, stream);
}

extern "C" int mvd_gridattn_tokens(const float* x, const float* depth_noise, const float* steps, const int* iter,
                                   const float* grid_lin, const float* feat, const float* in_feat, const float* cams,
                                   const float* in_cam, void* tokens_sp, int V, int q0, int Vq, int S, int D, float depth_scale,
                                   float depth_shift, mvd_stream_t stream) {
  return mvd_gridattn_tokens_scenes(x, depth_noise, steps, iter, grid_lin, feat, in_feat, cams, in_cam, tokens_sp, 1, V, q0, Vq, S, D,
                                    depth_scale, depth_shift, stream);
}

extern "C" int mvd_gridattn_tokens_backward_window(const float* x, const float* depth_noise, const float* steps, const int* iter,
                                                   const float* grid_lin, const float* cams, const float* in_cam, const float* dtok, int ldt,
                                                   long long* dfeat_acc, long long* din_feat_acc, float scale, int nscene, int V, int q0,
                                                   int Vq, int S, int D, float depth_scale, float depth_shift, int steps_scene_stride,
                                                   int window, mvd_stream_t stream) {
  const GridGeom g = {x, depth_noise, steps, iter, grid_lin, cams, in_cam, nscene, V, q0, Vq, S, D, depth_scale, depth_shift, steps_scene_stride, window};
  if (const int e = check_geom("mvd_gridattn_tokens_backward_window", g)) return e;
  MVD_CHECK_ARG(dtok && dfeat_acc && din_feat_acc, "mvd_gridattn_tokens_backward_window: null pointer");
  MVD_CHECK_ARG(ldt >= 512 && ldt % 4 == 0 && ((uintptr_t)dtok & 15) == 0 && scale > 0.f,
                "mvd_gridattn_tokens_backward_window: bad shape (ldt >= 512, 16-byte aligned dtok, scale > 0)");
  const size_t npts = num_points(g);
  MVD_CHECK_ARG((npts + 3) / 4 <= 0x7fffffff, "mvd_gridattn_tokens_backward_window: grid too large");
  hipLaunchKernelGGL(tokens_bwd_kernel, dim3(cdiv(npts, 4)), dim3(256), 0, (hipStream_t)stream, g, dtok, ldt, dfeat_acc, din_feat_acc, scale);
  MVD_CHECK_LAUNCH("mvd_gridattn_tokens_backward_window");
  return 0;
}

extern "C" int mvd_gridattn_tokens_backward_scenes(const float* x, const float* depth_noise, const float* steps, const int* iter,
                                                   const float* grid_lin, const float* cams, const float* in_cam, const float* dtok, int ldt,
                                                   long long* dfeat_acc, long long* din_feat_acc, float scale, int nscene, int V, int q0,
                                                   int Vq, int S, int D, float depth_scale, float depth_shift, int steps_scene_stride,
                                                   mvd_stream_t stream) {
  return mvd_gridattn_tokens_backward_window(x, depth_noise, steps, iter, grid_lin, cams, in_cam, dtok, ldt, dfeat_acc, din_feat_acc, scale,
                                             nscene, V, q0, Vq, S, D, depth_scale, depth_shift, steps_scene_stride, 0, stream);
}

extern "C" int mvd_gridattn_tokens_backward(const float* x, const float* depth_noise, const float* steps, const int* iter,
                                            const float* grid_lin, const float* cams, const float* in_cam, const float* dtok, int ldt,
                                            long long* dfeat_acc, long long* din_feat_acc, float scale, int V, int q0, int Vq, int S, int D,
                                            float depth_scale, float depth_shift, mvd_stream_t stream) {
  return mvd_gridattn_tokens_backward_scenes(x, depth_noise, steps, iter, grid_lin, cams, in_cam, dtok, ldt, dfeat_acc, din_feat_acc, scale,
                                             1, V, q0, Vq, S, D, depth_scale, depth_shift, 0, stream);
}
