// What the mesh units share (meshtopo.hip: incidence, components, report, filter, normals, smoothing; meshsimplify.hip: vertex
// clustering): the face classes, the clamped reads of the incidence table, the scan of nn_grid.hpp as one host call and the argument
// checks.  One copy, so every kernel of both units classifies a face and walks a list by the same comparisons.
#pragma once
#include "nn_grid.hpp"

namespace {

enum { kInvalid = -1, kRegular = 0, kRepeated = 1 };

struct MTMesh {
  const int *faces, *vstart, *fstart;
  long long nv, nf;
  int nscene;
};

// The class of face f, its ids and its scene (-1: of no scene, then invalid).
__device__ __forceinline__ int mt_face(const MTMesh& m, long long f, int* id, int& s) {
  id[0] = m.faces[f * 3 + 0], id[1] = m.faces[f * 3 + 1], id[2] = m.faces[f * 3 + 2];
  s = nn_find_scene(m.fstart, m.nscene, m.nf, f);
  if (s < 0) return kInvalid;
  const long long v0 = nn_clamp(m.vstart[s], m.nv), v1 = nn_clamp(m.vstart[s + 1], m.nv);
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (id[k] < v0 || id[k] >= v1) return kInvalid;
  return (id[0] == id[1] || id[1] == id[2] || id[0] == id[2]) ? kRepeated : kRegular;
}

// The list of vertex v in the incidence table: [b, e) clamped into [0, 3 nf].
__device__ __forceinline__ void mt_list(const int* inc_start, long long v, long long nf, long long& b, long long& e) {
  b = nn_clamp(inc_start[v], 3 * nf), e = nn_clamp(inc_start[v + 1], 3 * nf);
  if (e < b) e = b;
}

// Entry k of the table as (face g, corner c, the three ids of g).  false: not an entry of vertex v (a table these entries did not build).
__device__ __forceinline__ bool mt_entry(const int* inc, const int* faces, long long k, long long v, long long nv, long long nf, long long& g, int& c,
                                         int* gid) {
  const long long ent = inc[k];
  if (ent < 0 || ent >= 3 * nf) return false;
  g = ent / 3, c = (int)(ent - g * 3);
  gid[0] = faces[g * 3 + 0], gid[1] = faces[g * 3 + 1], gid[2] = faces[g * 3 + 2];
  if (gid[c] != v) return false;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (gid[j] < 0 || gid[j] >= nv) return false;
  return true;
}

// ---------------------------------------------------------------------------------------------------------------- host
constexpr size_t kMTMaxFaces = 0x7fffffffull / 3;      // an incidence entry is face * 3 + corner in int32

static size_t mt_chunks(size_t n) { return (n + 1 + kChunk - 1) / kChunk; }      // of a scan over n + 1 words
static size_t mt_scan_bytes(size_t n) { return mt_chunks(n) * kChunk * sizeof(unsigned) + up16((mt_chunks(n) + 1) * sizeof(unsigned)); }
static bool mt_sizes_ok(size_t nv, size_t nf) { return nv <= 0x7fffffffull - kChunk && nf <= kMTMaxFaces; }
static unsigned* mt_scan_blocks(unsigned* words, size_t n) { return words + mt_chunks(n) * kChunk; }

// the exclusive scan in place of n + 1 words padded (and zeroed) to whole chunks; words[n] becomes the total
static void mt_scan(unsigned* words, size_t n, hipStream_t st) {
  const unsigned chunks = (unsigned)mt_chunks(n);
  unsigned* blocks = mt_scan_blocks(words, n);
  hipLaunchKernelGGL(chunk_sum_kernel, dim3(chunks), dim3(kNNThreads), 0, st, words, blocks);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kCompactThreads), 0, st, blocks, chunks, blocks + chunks);
  hipLaunchKernelGGL(chunk_scan_kernel, dim3(chunks), dim3(kNNThreads), 0, st, words, blocks);
}

static dim3 mt_grid(size_t n) { return dim3((unsigned)((n + kNNThreads - 1) / kNNThreads)); }

static int mt_check_mesh(const char* fn, const void* faces, const void* vertex_start, const void* face_start, size_t nv, size_t nf, int nscene) {
  MVD_CHECK_ARG(nscene >= 1 && nscene <= 65535, "%s: nscene=%d outside [1, 65535]", fn, nscene);
  MVD_CHECK_ARG(mt_sizes_ok(nv, nf), "%s: nv=%zu beyond 2^31 - 1 - %d or nf=%zu beyond (2^31 - 1) / 3", fn, nv, kChunk, nf);
  MVD_CHECK_ARG(vertex_start && face_start, "%s: null vertex_start or face_start", fn);
  MVD_CHECK_ARG(faces || nf == 0, "%s: null faces with nf=%zu", fn, nf);
  MVD_CHECK_ARG((((uintptr_t)faces | (uintptr_t)vertex_start | (uintptr_t)face_start) & 3) == 0, "%s: a pointer that is not 4-byte aligned", fn);
  return 0;
}

static int mt_check_scratch(const char* fn, const void* scratch, size_t have, size_t need) {
  MVD_CHECK_ARG(scratch && have >= need && ((uintptr_t)scratch & 15) == 0, "%s: scratch of %zu bytes (needs %zu, 16-byte aligned)", fn, have, need);
  return 0;
}

static int mt_check_table(const char* fn, const void* inc_start, const void* inc, size_t nf) {
  MVD_CHECK_ARG(inc_start && (inc || nf == 0), "%s: null inc_start or inc", fn);
  MVD_CHECK_ARG((((uintptr_t)inc_start | (uintptr_t)inc) & 3) == 0, "%s: an incidence pointer that is not 4-byte aligned", fn);
  return 0;
}

#define MT_TRY(call)              \
  do {                            \
    if (int rc_ = (call)) return rc_; \
  } while (0)

}  // namespace
