// The host-and-device pieces of csrc/meshdist.hip run serially on a CPU, with no GPU: the per-pair rule, the brute force, the cell
// assignment (count, scan, fill, oversize lists) and the shell walk, on a case dumped by tests/meshdist_f64.py, against the oracle's
// face, region and dist2 bits.  Meant to be built with the host sanitizers before the kernels first run on a GPU:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -I include \
//         tools/meshdist_host.hip -o meshdist_host          (the sanitizers on the host pass only; nothing here touches a GPU)
//   python -c "import sys; sys.path.insert(0, 'tests'); import meshdist_f64 as M; M.dump_cases('/tmp/meshdist_cases')"
//   ./meshdist_host /tmp/meshdist_cases/*.bin
//
// File layout (little endian): int32 nq, nv, nf, nscene; query (nq, 3) f32; query_start, face_start (nscene + 1) i32 each; vertices
// (nv, 3) f32; faces (nf, 3) i32; then the oracle's face (nq) i32, region (nq) i32, dist2 (nq) f32.
#include "../mvdfusion_amd/csrc/meshdist.hip"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

void mvd_set_error(const char*, ...) {}

namespace {

template <class T>
bool read_into(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

struct Out {
  std::vector<int> face, region;
  std::vector<float> dist2, point, bary, normal;
  explicit Out(size_t nq) : face(nq, -9), region(nq, -9), dist2(nq, -9.f), point(nq * 3, -9.f), bary(nq * 3, -9.f), normal(nq * 3, -9.f) {}
};

void point_outputs(MDArgs& a, Out& o) {
  a.face = o.face.data(), a.region = o.region.data(), a.dist2 = o.dist2.data(), a.point = o.point.data(), a.bary = o.bary.data();
  a.normal = o.normal.data();
}

// MVD_NN_BRUTE, serially
void run_brute(MDArgs a, Out& o) {
  point_outputs(a, o);
  for (long long i = 0; i < a.nq; ++i) {
    const float q[3] = {a.query[i * 3 + 0], a.query[i * 3 + 1], a.query[i * 3 + 2]};
    MDOne one;
    const int s = nn_find_scene(a.qstart, a.nscene, a.nq, i);
    if (s >= 0 && nn_finite(q[0]) && nn_finite(q[1]) && nn_finite(q[2])) {
      const double P[3] = {(double)q[0], (double)q[1], (double)q[2]};
      for (long long f = nn_clamp(a.tstart[s], a.nt); f < nn_clamp(a.tstart[s + 1], a.nt); ++f) md_offer(a, f, P, one);
    }
    md_write(a, i, q, one.bestf);
  }
}

// MVD_NN_GRID, serially: the build as the kernels do it (box, count, scan, fill), then every query.  The scratch is a vector sized by
// md_plan and pre-filled with a pattern, so a read of a word the build did not write, or a write past the plan, shows.
bool run_grid(MDArgs a, int grid, Out& o, size_t* refs_used, unsigned* oversize) {
  MDPlan p;
  if (!md_plan((size_t)a.nt, a.nscene, MVD_NN_GRID, grid, p)) return false;
  std::vector<unsigned char> scratch(p.bytes, 0xa5);
  md_point_scratch(a, p, scratch.data());
  point_outputs(a, o);
  memset(a.box, 0xff, (size_t)a.nscene * 6 * sizeof(unsigned));
  memset(a.nover, 0, (size_t)a.nscene * sizeof(unsigned));
  memset(a.cells, 0, p.chunks * kChunk * sizeof(unsigned));
  for (long long f = 0; f < a.nt; ++f) {      // md_bounds_kernel
    const int s = nn_find_scene(a.tstart, a.nscene, a.nt, f);
    float v[9];
    if (s < 0 || !md_load_face(a, f, v)) continue;
    for (int k = 0; k < 3; ++k) {
      const float mn = fminf(fminf(v[k], v[3 + k]), v[6 + k]), mx = fmaxf(fmaxf(v[k], v[3 + k]), v[6 + k]);
      unsigned* lo = a.box + (size_t)s * 6 + k;
      unsigned* hi = lo + 3;
      if (nn_key(mn) < *lo) *lo = nn_key(mn);
      if (~nn_key(mx) < *hi) *hi = ~nn_key(mx);
    }
  }
  for (long long f = 0; f < a.nt; ++f) md_place_face<0>(a, f);
  unsigned run = 0;
  for (size_t c = 0; c < p.chunks * kChunk; ++c) {      // the exclusive scan
    const unsigned n = a.cells[c];
    a.cells[c] = run;
    run += n;
  }
  *refs_used = run;
  if ((size_t)run > p.nref) return false;
  for (long long f = 0; f < a.nt; ++f) md_place_face<1>(a, f);
  *oversize = 0;
  for (int s = 0; s < a.nscene; ++s) *oversize += a.nover[s];
  for (long long i = 0; i < a.nq; ++i) md_query_grid(a, i);
  return true;
}

long long differences(const Out& a, const Out& b, size_t nq) {
  long long n = 0;
  for (size_t i = 0; i < nq; ++i) {
    n += a.face[i] != b.face[i] || a.region[i] != b.region[i] || memcmp(&a.dist2[i], &b.dist2[i], 4) != 0;
    n += memcmp(&a.point[i * 3], &b.point[i * 3], 12) != 0 || memcmp(&a.bary[i * 3], &b.bary[i * 3], 12) != 0 ||
         memcmp(&a.normal[i * 3], &b.normal[i * 3], 12) != 0;
  }
  return n;
}

}  // namespace

int main(int argc, char** argv) {
  long long bad = 0;
  for (int k = 1; k < argc; ++k) {
    FILE* f = fopen(argv[k], "rb");
    int head[4];
    if (!f || fread(head, 4, 4, f) != 4) {
      printf("%s: cannot read\n", argv[k]);
      return 2;
    }
    const size_t nq = head[0], nv = head[1], nf = head[2];
    const int nscene = head[3];
    std::vector<float> query, vertices, want_d2;
    std::vector<int> qstart, fstart, faces, want_face, want_region;
    const bool ok = read_into(f, query, nq * 3) && read_into(f, qstart, nscene + 1) && read_into(f, fstart, nscene + 1) &&
                    read_into(f, vertices, nv * 3) && read_into(f, faces, nf * 3) && read_into(f, want_face, nq) &&
                    read_into(f, want_region, nq) && read_into(f, want_d2, nq);
    fclose(f);
    if (!ok) {
      printf("%s: short file\n", argv[k]);
      return 2;
    }
    MDArgs a{};
    a.query = query.data(), a.vertices = vertices.data(), a.qstart = qstart.data(), a.tstart = fstart.data(), a.faces = faces.data();
    a.nq = (long long)nq, a.nv = (long long)nv, a.nt = (long long)nf, a.nscene = nscene;
    Out brute(nq);
    run_brute(a, brute);
    long long oracle = 0;
    for (size_t i = 0; i < nq; ++i)
      oracle += brute.face[i] != want_face[i] || brute.region[i] != want_region[i] || memcmp(&brute.dist2[i], &want_d2[i], 4) != 0;
    printf("%s: nq %zu nf %zu scenes %d | brute against the oracle: %lld mismatches", argv[k], nq, nf, nscene, oracle);
    bad += oracle;
    const int grids[] = {1, 2, 7, 0, 64};
    for (int g : grids) {
      Out grid(nq);
      size_t refs = 0;
      unsigned over = 0;
      if (!run_grid(a, g, grid, &refs, &over)) {
        printf(" | grid %d: PLAN OR REFERENCE BOUND FAILED", g);
        ++bad;
        continue;
      }
      const long long d = differences(brute, grid, nq);
      printf(" | grid %d: %lld differences, %zu references (bound %zu), %u oversize", g, d, refs, nf * (size_t)kMDRefs, over);
      bad += d;
    }
    printf("\n");
  }
  if (bad) printf("FAILED: %lld\n", bad);
  else printf("ok\n");
  return bad ? 1 : 0;
}
