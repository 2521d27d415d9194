// Volumetric fusion of the sampled RGB-D views and mesh extraction (include/mvd_hip.h: mvd_tsdf_integrate, mvd_mesh_count, mvd_mesh_emit).
//
// integrate_kernel: one thread per voxel, x fastest, the scene on blockIdx.y (a workgroup never straddles scenes).  The thread walks the
// scene's V views in order: project_z, the fuse kernel's pixel-centre depth lookup (fusion_common.hpp: one copy of both), one observation
// per view at most, summed in registers -- no atomics, the same bits run to run.  The view index and the camera base are uniform, so the
// camera records come in as scalar loads; the depth planes (V S^2 floats) are read from global memory and stay in L1 / L2 -- a wavefront is
// 64 neighbouring voxels of one row, which project to neighbouring texels.  (The fuse kernel measured its LDS-staged form as no faster.)
//
// mesh: marching tetrahedra (tsdf_mesh.hpp holds the combinatorics).  mvd_mesh_count: edge_count_kernel (one thread per lattice edge,
// 64-bit ballot + popcount per wavefront, a count per block) -> scan_wide_kernel (the single-workgroup carry scan of fusion_common.hpp's
// scan_kernel, eight counts per thread) -> edge_map_kernel (the same ballots: edge -> vertex id or -1) -> cell_count_kernel (one thread
// per cell: its triangles, a count per block) -> scan_wide_kernel ->
// cell_offset_kernel (block offset + in-block exclusive scan: the first face of every cell).  mvd_mesh_emit: vertex_kernel (one thread
// per edge) and face_kernel (one thread per cell) write through those maps.  Blocks are padded per scene (blockIdx.y).  No atomic
// decides an order.
#include "fusion_common.hpp"
#include "tsdf_mesh.hpp"

namespace {

constexpr int kTsdfThreads = 256;
constexpr int kMeshThreads = kCompactThreads;      // 4 wavefronts, as the point compaction's blocks

struct TsdfArgs {
  const float *lat, *rgb, *cams;
  float *tsdf, *color;
  uint8_t *weight, *cweight;
  int V, S, P, G;
  float org[3], vs, trunc;      // org: centre of the box minus half_extent; vs: voxel size
  int carve;
  float depth_scale, depth_shift, lo, hi;
};

// centre of voxel index i along axis ax
__device__ __forceinline__ float voxel_centre(const float* org, float vs, int ax, int i) { return org[ax] + ((float)i + 0.5f) * vs; }

__global__ __launch_bounds__(kTsdfThreads) void integrate_kernel(TsdfArgs a) {
  const int V = a.V, S = a.S, SS = S * S, P = a.P, G = a.G;
  const unsigned GGG = (unsigned)G * G * G;
  const unsigned vox = blockIdx.x * kTsdfThreads + threadIdx.x;
  if (vox >= GGG) return;
  const int scene = blockIdx.y;
  const float* lat = a.lat + (size_t)scene * V * 5 * SS;
  const float* cams = a.cams + (size_t)scene * V * MVD_CAM_RECORD;
  const int i = (int)(vox % (unsigned)G), j = (int)(vox / (unsigned)G % (unsigned)G), k = (int)(vox / ((unsigned)G * G));
  const float X[3] = {voxel_centre(a.org, a.vs, 0, i), voxel_centre(a.org, a.vs, 1, j), voxel_centre(a.org, a.vs, 2, k)};
  float sum = 0.f, csum[3] = {0.f, 0.f, 0.f};
  int n = 0, cn = 0;
  for (int v = 0; v < V; ++v) {
    float u, w, zc;
    project_z(load_cam(cams + (size_t)v * MVD_CAM_RECORD), X, u, w, zc);
    if (!(zc > 0.f && fabsf(u) <= 1.f && fabsf(w) <= 1.f)) continue;      // unseen (a NaN compares false)
    const PixelTaps t = pixel_taps(u, w, S);
    float zt[4];
    int nfg = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float d = depth01(lat[((size_t)v * 5 + 4) * SS + t.idx[q]]);
      nfg += a.lo < d && d < a.hi;
      zt[q] = d * a.depth_scale + a.depth_shift;
    }
    if (nfg == 4) {
      const float sdf = bilinear_mix(zt, t) - zc;
      if (sdf < -a.trunc) continue;      // hidden behind the surface this view sees
      sum += fminf(1.f, sdf / a.trunc);
      ++n;
      if (a.rgb && fabsf(sdf) <= a.trunc) {
        const PixelTaps c = pixel_taps(u, w, P);
        const float* img = a.rgb + ((size_t)(scene * V + v) * 3) * P * P;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          float px[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) px[q] = img[(size_t)ch * P * P + c.idx[q]];
          csum[ch] += bilinear_mix(px, c);
        }
        ++cn;
      }
    } else if (nfg == 0 && a.carve) {      // free space in front of nothing
      sum += 1.f;
      ++n;
    }
  }
  const size_t g = (size_t)scene * GGG + vox;
  a.tsdf[g] = n ? sum / (float)n : 1.f;
  a.weight[g] = (uint8_t)n;
  if (a.rgb) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) a.color[g * 3 + ch] = cn ? csum[ch] / (float)cn : 0.f;
    a.cweight[g] = (uint8_t)cn;
  }
}

// ------------------------------------------------------------------------------------------------ marching tetrahedra
struct MeshArgs {
  const float* tsdf;
  const uint8_t* weight;
  const float* color;
  const uint8_t* cweight;
  int G;
  unsigned GGG, nedge, ncell, nbe, nbc;      // per scene: voxels, edge slots (7 GGG), cells, blocks of edges, blocks of cells
  int* emap;                                 // (nscene, nedge): vertex id or -1
  unsigned *eblocks, *cblocks;               // (nscene, nbe), (nscene, nbc): count, then exclusive offset
  unsigned* celloff;                         // (nscene, ncell): first face of the cell
  int *vertex_start, *face_start;
  float org[3], vs, fill[3];
  float *vertices, *colors;
  int* faces;
  unsigned nvert, nface;
};

__device__ __forceinline__ bool observed(const MeshArgs& a, size_t g) { return a.weight[g] > 0; }
__device__ __forceinline__ bool inside(const MeshArgs& a, size_t g) { return a.weight[g] > 0 && a.tsdf[g] < 0.f; }

// the two ends (voxel numbers inside the scene) of edge slot e of a scene; false when the edge leaves the grid
__device__ __forceinline__ bool edge_ends(const MeshArgs& a, unsigned e, unsigned& v0, unsigned& v1, int* c0, int* c1) {
  const unsigned G = (unsigned)a.G;
  v0 = e / (unsigned)kMeshDirs;
  const int mask = mesh_dir_mask((int)(e % (unsigned)kMeshDirs));
  c0[0] = (int)(v0 % G), c0[1] = (int)(v0 / G % G), c0[2] = (int)(v0 / (G * G));
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) c1[ax] = c0[ax] + ((mask >> ax) & 1);
  v1 = ((unsigned)c1[2] * G + (unsigned)c1[1]) * G + (unsigned)c1[0];
  return c1[0] < a.G && c1[1] < a.G && c1[2] < a.G;
}

// edge slot e of `scene` carries a vertex: both ends observed, exactly one inside
__device__ __forceinline__ bool edge_carries(const MeshArgs& a, int scene, unsigned e) {
  if (e >= a.nedge) return false;
  unsigned v0, v1;
  int c0[3], c1[3];
  if (!edge_ends(a, e, v0, v1, c0, c1)) return false;
  const size_t base = (size_t)scene * a.GGG;
  return observed(a, base + v0) && observed(a, base + v1) && inside(a, base + v0) != inside(a, base + v1);
}

__global__ __launch_bounds__(kMeshThreads) void edge_count_kernel(MeshArgs a) {
  __shared__ unsigned wave_n[kMeshThreads / 64];
  const unsigned long long mask = __ballot(edge_carries(a, blockIdx.y, blockIdx.x * kMeshThreads + threadIdx.x));
  if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = (unsigned)__popcll(mask);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned n = 0;
#pragma unroll
    for (int w = 0; w < kMeshThreads / 64; ++w) n += wave_n[w];
    a.eblocks[(size_t)blockIdx.y * a.nbe + blockIdx.x] = n;
  }
}

__global__ __launch_bounds__(kMeshThreads) void edge_map_kernel(MeshArgs a) {
  __shared__ unsigned wave_n[kMeshThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, scene = blockIdx.y;
  const unsigned e = blockIdx.x * kMeshThreads + threadIdx.x;
  const bool carries = edge_carries(a, scene, e);
  const unsigned long long mask = __ballot(carries);
  if (lane == 0) wave_n[wave] = (unsigned)__popcll(mask);
  __syncthreads();
  unsigned o = a.eblocks[(size_t)scene * a.nbe + blockIdx.x];
  if (blockIdx.x == 0 && threadIdx.x == 0) a.vertex_start[scene] = (int)o;
#pragma unroll
  for (int w = 0; w < kMeshThreads / 64; ++w)
    if (w < wave) o += wave_n[w];
  o += (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
  if (e < a.nedge) a.emap[(size_t)scene * a.nedge + e] = carries ? (int)o : -1;
}

// corner of cell (ck, cj, ci) at lattice offset mask -> voxel number inside the scene
__device__ __forceinline__ unsigned cell_corner(const MeshArgs& a, const int* c, int mask) {
  const unsigned G = (unsigned)a.G;
  return ((unsigned)(c[2] + ((mask >> 2) & 1)) * G + (unsigned)(c[1] + ((mask >> 1) & 1))) * G + (unsigned)(c[0] + (mask & 1));
}

// the cell of a thread and the state of its 8 corners as bit masks over the lattice offsets; false past the scene's cells
__device__ __forceinline__ bool cell_state(const MeshArgs& a, int scene, unsigned cell, int* c, unsigned& obs, unsigned& in) {
  obs = in = 0;
  if (cell >= a.ncell) return false;
  const unsigned G1 = (unsigned)a.G - 1;
  c[0] = (int)(cell % G1), c[1] = (int)(cell / G1 % G1), c[2] = (int)(cell / (G1 * G1));
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const size_t g = (size_t)scene * a.GGG + cell_corner(a, c, m);
    obs |= (unsigned)observed(a, g) << m;
    in |= (unsigned)inside(a, g) << m;
  }
  return true;
}

// the inside mask of tetrahedron q over its corners 0 .. 3; false when a corner is unobserved
__device__ __forceinline__ bool tet_state(int q, unsigned obs, unsigned in, unsigned& inside4) {
  inside4 = 0;
  bool all = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int m = tet_corner_mask(q, k);
    all = all && ((obs >> m) & 1u);
    inside4 |= ((in >> m) & 1u) << k;
  }
  return all;
}

__device__ __forceinline__ unsigned cell_triangles(const MeshArgs& a, int scene, unsigned cell) {
  int c[3];
  unsigned obs, in, n = 0;
  if (!cell_state(a, scene, cell, c, obs, in)) return 0;
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    unsigned inside4;
    if (tet_state(q, obs, in, inside4)) n += (unsigned)tet_triangle_count(inside4);
  }
  return n;
}

// exclusive prefix of v over the workgroup's threads, and the workgroup's total
__device__ __forceinline__ unsigned block_exclusive(unsigned v, unsigned& total) {
  __shared__ unsigned wave_n[kMeshThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wave_n[wave] = incl;
  __syncthreads();
  unsigned before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kMeshThreads / 64; ++w) {
    if (w < wave) before += wave_n[w];
    total += wave_n[w];
  }
  return before + incl - v;
}

// scan_kernel (fusion_common.hpp) with kScanWide consecutive counts per thread: the same single workgroup with a running carry, an eighth of
// the trips.  A 128^3 volume has 57 344 edge blocks; at one count per thread the 224 dependent trips were a quarter of mvd_mesh_count
// (measured).
constexpr int kScanWide = 8;
__global__ __launch_bounds__(kMeshThreads) void scan_wide_kernel(unsigned* __restrict__ blocks, unsigned nblocks, unsigned* __restrict__ count) {
  unsigned carry = 0;
  for (unsigned base = 0; base < nblocks; base += kMeshThreads * kScanWide) {
    const unsigned i0 = base + threadIdx.x * kScanWide;
    unsigned v[kScanWide], sum = 0;
#pragma unroll
    for (int k = 0; k < kScanWide; ++k) {
      v[k] = i0 + k < nblocks ? blocks[i0 + k] : 0u;
      sum += v[k];
    }
    unsigned total;
    unsigned o = carry + block_exclusive(sum, total);
#pragma unroll
    for (int k = 0; k < kScanWide; ++k) {
      if (i0 + k < nblocks) blocks[i0 + k] = o;
      o += v[k];
    }
    carry += total;
    __syncthreads();      // block_exclusive's shared words are rewritten by the next trip
  }
  if (threadIdx.x == 0) *count = carry;
}

__global__ __launch_bounds__(kMeshThreads) void cell_count_kernel(MeshArgs a) {
  unsigned total;
  block_exclusive(cell_triangles(a, blockIdx.y, blockIdx.x * kMeshThreads + threadIdx.x), total);
  if (threadIdx.x == 0) a.cblocks[(size_t)blockIdx.y * a.nbc + blockIdx.x] = total;
}

__global__ __launch_bounds__(kMeshThreads) void cell_offset_kernel(MeshArgs a) {
  const int scene = blockIdx.y;
  const unsigned cell = blockIdx.x * kMeshThreads + threadIdx.x;
  unsigned total;
  const unsigned before = block_exclusive(cell_triangles(a, scene, cell), total);
  const unsigned o = a.cblocks[(size_t)scene * a.nbc + blockIdx.x];
  if (blockIdx.x == 0 && threadIdx.x == 0) a.face_start[scene] = (int)o;
  if (cell < a.ncell) a.celloff[(size_t)scene * a.ncell + cell] = o + before;
}

__global__ __launch_bounds__(kMeshThreads) void vertex_kernel(MeshArgs a) {
  const int scene = blockIdx.y;
  const unsigned e = blockIdx.x * kMeshThreads + threadIdx.x;
  if (e >= a.nedge) return;
  const int id = a.emap[(size_t)scene * a.nedge + e];
  if (id < 0 || (unsigned)id >= a.nvert) return;
  unsigned v0, v1;
  int c0[3], c1[3];
  if (!edge_ends(a, e, v0, v1, c0, c1)) return;      // (a map of the count call never names such an edge)
  const size_t g0 = (size_t)scene * a.GGG + v0, g1 = (size_t)scene * a.GGG + v1;
  const bool first = inside(a, g0);                  // the inside end is a
  const size_t ga = first ? g0 : g1, gb = first ? g1 : g0;
  const float da = a.tsdf[ga], db = a.tsdf[gb];
  const float t = da / (da - db);
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    const float x0 = voxel_centre(a.org, a.vs, ax, c0[ax]), x1 = voxel_centre(a.org, a.vs, ax, c1[ax]);
    const float xa = first ? x0 : x1, xb = first ? x1 : x0;
    a.vertices[(size_t)id * 3 + ax] = xa + t * (xb - xa);
  }
  if (a.colors) {
    const bool ha = a.cweight[ga] > 0, hb = a.cweight[gb] > 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float ca = ha ? a.color[ga * 3 + ch] : 0.f, cb = hb ? a.color[gb * 3 + ch] : 0.f;
      a.colors[(size_t)id * 3 + ch] = ha && hb ? ca + t * (cb - ca) : ha ? ca : hb ? cb : a.fill[ch];
    }
  }
}

__global__ __launch_bounds__(kMeshThreads) void face_kernel(MeshArgs a) {
  const int scene = blockIdx.y;
  const unsigned cell = blockIdx.x * kMeshThreads + threadIdx.x;
  int c[3];
  unsigned obs, in;
  if (!cell_state(a, scene, cell, c, obs, in)) return;
  unsigned o = a.celloff[(size_t)scene * a.ncell + cell];
  const int* emap = a.emap + (size_t)scene * a.nedge;
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    unsigned inside4;
    if (!tet_state(q, obs, in, inside4)) continue;
    const int n = tet_triangle_count(inside4);
    if (n == 0) continue;
    int id[6];
#pragma unroll
    for (int ca = 0; ca < 4; ++ca)
#pragma unroll
      for (int cb = ca + 1; cb < 4; ++cb) {
        const int ma = tet_corner_mask(q, ca), mb = tet_corner_mask(q, cb);
        id[tet_edge_slot(ca, cb)] = emap[(size_t)cell_corner(a, c, ma) * kMeshDirs + mesh_mask_dir(mb ^ ma)];
      }
    int f[6];
    tet_triangles(inside4, tet_sign(q), id, f);
    if ((unsigned long long)o + n <= a.nface) {      // (a scratch of the count call always passes)
#pragma unroll
      for (int k = 0; k < 6; ++k)
        if (k < 3 * n) a.faces[(size_t)o * 3 + k] = f[k];
    }
    o += n;
  }
}

// the shape of a mesh call; false for what the calls refuse
struct MeshShape {
  unsigned GGG, nedge, ncell, nbe, nbc;
  size_t emap, eblocks, cblocks, celloff, words;      // offsets in 4-byte words, and the total
};
bool mesh_shape(int nscene, int G, MeshShape& s) {
  if (G < 2 || G > 256 || nscene < 1 || nscene > 65535) return false;
  const unsigned long long GGG = (unsigned long long)G * G * G, ncell = (unsigned long long)(G - 1) * (G - 1) * (G - 1);
  if (7ull * nscene * GGG >= (1ull << 31) || 12ull * nscene * ncell >= (1ull << 31)) return false;
  s.GGG = (unsigned)GGG;
  s.nedge = (unsigned)(kMeshDirs * GGG);
  s.ncell = (unsigned)ncell;
  s.nbe = (s.nedge + kMeshThreads - 1) / kMeshThreads;
  s.nbc = (s.ncell + kMeshThreads - 1) / kMeshThreads;
  s.emap = 0;
  s.eblocks = s.emap + (size_t)nscene * s.nedge;
  s.cblocks = s.eblocks + (size_t)nscene * s.nbe;
  s.celloff = s.cblocks + (size_t)nscene * s.nbc;
  s.words = s.celloff + (size_t)nscene * s.ncell;
  return true;
}

void mesh_args(MeshArgs& a, const MeshShape& s, int G, void* scratch) {
  unsigned* w = (unsigned*)scratch;
  a.G = G;
  a.GGG = s.GGG, a.nedge = s.nedge, a.ncell = s.ncell, a.nbe = s.nbe, a.nbc = s.nbc;
  a.emap = (int*)(w + s.emap);
  a.eblocks = w + s.eblocks;
  a.cblocks = w + s.cblocks;
  a.celloff = w + s.celloff;
}

}  // namespace

extern "C" int mvd_tsdf_integrate(const float* lat, const float* rgb, const float* cams, float* tsdf, uint8_t* weight, float* color,
                                  uint8_t* cweight, int nscene, int V, int S, int up, int G, float cx, float cy, float cz, float half_extent,
                                  float trunc, int carve, float depth_scale, float depth_shift, float lo, float hi, mvd_stream_t stream) {
  MVD_CHECK_ARG(lat && cams && tsdf && weight, "mvd_tsdf_integrate: null pointer");
  MVD_CHECK_ARG(!rgb || (color && cweight), "mvd_tsdf_integrate: rgb without color and cweight outputs");
  MVD_CHECK_ARG(nscene >= 1 && nscene <= 65535, "mvd_tsdf_integrate: nscene=%d outside [1, 65535]", nscene);
  MVD_CHECK_ARG(V >= 1 && V <= 255, "mvd_tsdf_integrate: V=%d outside [1, 255] (the counts are bytes)", V);
  MVD_CHECK_ARG(S >= 2 && S <= 32768, "mvd_tsdf_integrate: S=%d outside [2, 32768]", S);
  MVD_CHECK_ARG(up >= 1 && (unsigned long long)S * up <= 46340ull, "mvd_tsdf_integrate: up=%d (>= 1, S * up <= 46340)", up);
  MVD_CHECK_ARG(G >= 2 && G <= 256, "mvd_tsdf_integrate: G=%d outside [2, 256]", G);
  MVD_CHECK_ARG(7ull * nscene * G * G * G < (1ull << 31), "mvd_tsdf_integrate: 7 * nscene * G^3 beyond 2^31 - 1 (nscene=%d, G=%d)", nscene, G);
  MVD_CHECK_ARG((unsigned long long)nscene * V * 5 * S * S <= 0x7fffffffull, "mvd_tsdf_integrate: nscene * V * 5 * S^2 beyond 2^31 - 1");
  MVD_CHECK_ARG(trunc > 0.f, "mvd_tsdf_integrate: trunc=%g (> 0)", (double)trunc);
  MVD_CHECK_ARG(half_extent > 0.f, "mvd_tsdf_integrate: half_extent=%g (> 0)", (double)half_extent);
  MVD_CHECK_ARG(lo < hi, "mvd_tsdf_integrate: foreground range lo=%g >= hi=%g", (double)lo, (double)hi);
  TsdfArgs a{lat, rgb, cams, tsdf, color, weight, cweight, V, S, S * up, G, {cx - half_extent, cy - half_extent, cz - half_extent},
             2.f * half_extent / (float)G, trunc, carve, depth_scale, depth_shift, lo, hi};
  hipLaunchKernelGGL(integrate_kernel, dim3(cdiv((long)G * G * G, kTsdfThreads), nscene), dim3(kTsdfThreads), 0, (hipStream_t)stream, a);
  MVD_CHECK_LAUNCH("mvd_tsdf_integrate");
  return 0;
}

extern "C" size_t mvd_mesh_scratch(int nscene, int G) {
  MeshShape s;
  return mesh_shape(nscene, G, s) ? s.words * sizeof(unsigned) : 0;
}

extern "C" int mvd_mesh_count(const float* tsdf, const uint8_t* weight, int nscene, int G, int* vertex_start, int* face_start, void* scratch,
                              size_t scratch_bytes, mvd_stream_t stream) {
  MVD_CHECK_ARG(tsdf && weight && vertex_start && face_start && scratch, "mvd_mesh_count: null pointer");
  MeshShape s;
  MVD_CHECK_ARG(mesh_shape(nscene, G, s),
                "mvd_mesh_count: nscene=%d, G=%d (G in [2, 256], nscene in [1, 65535], 7 * nscene * G^3 and 12 * nscene * (G-1)^3 < 2^31)",
                nscene, G);
  MVD_CHECK_ARG(scratch_bytes >= s.words * sizeof(unsigned) && ((uintptr_t)scratch & 3) == 0,
                "mvd_mesh_count: scratch of %zu bytes (needs %zu, 4-byte aligned)", scratch_bytes, s.words * sizeof(unsigned));
  MeshArgs a{};
  mesh_args(a, s, G, scratch);
  a.tsdf = tsdf, a.weight = weight, a.vertex_start = vertex_start, a.face_start = face_start;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(edge_count_kernel, dim3(s.nbe, nscene), dim3(kMeshThreads), 0, st, a);
  hipLaunchKernelGGL(scan_wide_kernel, dim3(1), dim3(kMeshThreads), 0, st, a.eblocks, (unsigned)nscene * s.nbe, (unsigned*)(vertex_start + nscene));
  hipLaunchKernelGGL(edge_map_kernel, dim3(s.nbe, nscene), dim3(kMeshThreads), 0, st, a);
  hipLaunchKernelGGL(cell_count_kernel, dim3(s.nbc, nscene), dim3(kMeshThreads), 0, st, a);
  hipLaunchKernelGGL(scan_wide_kernel, dim3(1), dim3(kMeshThreads), 0, st, a.cblocks, (unsigned)nscene * s.nbc, (unsigned*)(face_start + nscene));
  hipLaunchKernelGGL(cell_offset_kernel, dim3(s.nbc, nscene), dim3(kMeshThreads), 0, st, a);
  MVD_CHECK_LAUNCH("mvd_mesh_count");
  return 0;
}

extern "C" int mvd_mesh_emit(const float* tsdf, const uint8_t* weight, const float* color, const uint8_t* cweight, int nscene, int G, float cx,
                             float cy, float cz, float half_extent, const float* fill, float* vertices, float* colors, int* faces,
                             size_t nvert, size_t nface, const void* scratch, size_t scratch_bytes, mvd_stream_t stream) {
  MVD_CHECK_ARG(tsdf && weight && scratch, "mvd_mesh_emit: null pointer");
  MVD_CHECK_ARG((vertices || nvert == 0) && (faces || nface == 0), "mvd_mesh_emit: null output for nvert=%zu, nface=%zu", nvert, nface);
  MVD_CHECK_ARG((color && cweight && fill && (colors || nvert == 0)) || (!color && !cweight && !colors),
                "mvd_mesh_emit: color, cweight, fill and colors go together");
  MeshShape s;
  MVD_CHECK_ARG(mesh_shape(nscene, G, s),
                "mvd_mesh_emit: nscene=%d, G=%d (G in [2, 256], nscene in [1, 65535], 7 * nscene * G^3 and 12 * nscene * (G-1)^3 < 2^31)",
                nscene, G);
  MVD_CHECK_ARG(nvert <= (size_t)nscene * s.nedge && nface <= 12ull * nscene * s.ncell, "mvd_mesh_emit: nvert=%zu, nface=%zu beyond the volume's",
                nvert, nface);
  MVD_CHECK_ARG(half_extent > 0.f, "mvd_mesh_emit: half_extent=%g (> 0)", (double)half_extent);
  MVD_CHECK_ARG(scratch_bytes >= s.words * sizeof(unsigned) && ((uintptr_t)scratch & 3) == 0,
                "mvd_mesh_emit: scratch of %zu bytes (needs %zu, 4-byte aligned)", scratch_bytes, s.words * sizeof(unsigned));
  MeshArgs a{};
  mesh_args(a, s, G, const_cast<void*>(scratch));
  a.tsdf = tsdf, a.weight = weight, a.color = color, a.cweight = cweight;
  a.org[0] = cx - half_extent, a.org[1] = cy - half_extent, a.org[2] = cz - half_extent;
  a.vs = 2.f * half_extent / (float)G;
  if (color)
    for (int c = 0; c < 3; ++c) a.fill[c] = fill[c];
  a.vertices = vertices, a.colors = color ? colors : nullptr, a.faces = faces;
  a.nvert = (unsigned)nvert, a.nface = (unsigned)nface;
  const hipStream_t st = (hipStream_t)stream;
  if (nvert > 0) hipLaunchKernelGGL(vertex_kernel, dim3(s.nbe, nscene), dim3(kMeshThreads), 0, st, a);
  if (nface > 0) hipLaunchKernelGGL(face_kernel, dim3(s.nbc, nscene), dim3(kMeshThreads), 0, st, a);
  MVD_CHECK_LAUNCH("mvd_mesh_emit");
  return 0;
}
