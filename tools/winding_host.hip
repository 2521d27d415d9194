// The host-and-device pieces of csrc/winding.hip run serially on a CPU, with no GPU: the candidate test, the per-pair solid angle, the
// exact sum, the cell build as the kernels do it (box, assign + count, flags, the two scans, ranges, fill, rank, moments) and the cells
// query, on meshes made here (a UV sphere with bad faces mixed in, two scenes), cells against exact.  Meant to be built with the host
// sanitizers before the kernels first run on a GPU:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -I include \
//         tools/winding_host.hip -o winding_host           (the sanitizers on the host pass only; nothing here touches a GPU)
//   ./winding_host
//
// Checked: cells = 1 with beta = +inf gives the bits of the exact sum; every cells with beta = +inf stays within nf * 2^-48 of it (the
// same terms in another grouping); beta = 2 stays within 0.05 (the far field's own error: DESIGN.md has it measured at 2e-2); beta = 0
// gives finite values; every member list ascends, holds candidates of its own cell only, and the lists hold every candidate once.  The
// scratch is a vector sized by wn_plan and pre-filled with a pattern, so a read of a word the build did not write, or a write past the
// plan, shows; the fill runs over the faces in DESCENDING order so that the rank pass has something to sort.
#include "../mvdfusion_amd/csrc/winding.hip"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

void mvd_set_error(const char*, ...) {}

namespace {

struct Mesh {
  std::vector<float> vertices, query;
  std::vector<int> faces, fstart, qstart;
};

// a UV sphere of radius r about (cx, 0, 0), wound outwards, appended to m
void add_sphere(Mesh& m, int nlat, int nlon, float r, float cx) {
  const int v0 = (int)m.vertices.size() / 3;
  auto push = [&](double x, double y, double z) { m.vertices.push_back((float)(x + cx)), m.vertices.push_back((float)y), m.vertices.push_back((float)z); };
  push(0, 0, r);
  for (int i = 1; i < nlat; ++i)
    for (int j = 0; j < nlon; ++j) {
      const double th = M_PI * i / nlat, ph = 2 * M_PI * j / nlon;
      push(r * sin(th) * cos(ph), r * sin(th) * sin(ph), r * cos(th));
    }
  push(0, 0, -r);
  auto ring = [&](int i, int j) { return v0 + 1 + (i - 1) * nlon + (j % nlon); };
  const int south = v0 + 1 + (nlat - 1) * nlon;
  auto face = [&](int a, int b, int c) { m.faces.push_back(a), m.faces.push_back(b), m.faces.push_back(c); };
  for (int i = 0; i < nlat; ++i)
    for (int j = 0; j < nlon; ++j) {
      if (i == 0) face(v0, ring(1, j), ring(1, j + 1));
      else if (i == nlat - 1) face(south, ring(i, j + 1), ring(i, j));
      else face(ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)), face(ring(i, j), ring(i + 1, j + 1), ring(i, j + 1));
    }
}

unsigned lcg(unsigned& s) { return s = s * 1664525u + 1013904223u; }
float uniform(unsigned& s, float lo, float hi) { return lo + (hi - lo) * (float)(lcg(s) >> 8) / 16777216.f; }

Mesh make_mesh() {
  Mesh m;
  m.fstart.push_back(0);
  add_sphere(m, 12, 24, 0.45f, 0.f);
  const int nv = (int)m.vertices.size() / 3;
  const int bad[][3] = {{-1, 0, 1}, {2, 1 << 30, 3}, {3, 3, 3}, {4, 4, 5}};      // ids out of range, a repeated vertex: no candidates
  for (auto& b : bad) m.faces.insert(m.faces.end(), b, b + 3);
  m.fstart.push_back((int)m.faces.size() / 3);
  add_sphere(m, 8, 16, 0.3f, 2.f);
  m.vertices.push_back(NAN), m.vertices.push_back(0.f), m.vertices.push_back(0.f);
  const int last = (int)m.vertices.size() / 3 - 1;
  m.faces.push_back(last), m.faces.push_back(nv), m.faces.push_back(nv + 1);      // a NaN vertex
  m.fstart.push_back((int)m.faces.size() / 3);
  unsigned seed = 12345u;
  m.qstart.push_back(0);
  for (int s = 0; s < 2; ++s) {
    for (int k = 0; k < 150; ++k) {
      m.query.push_back(uniform(seed, -0.7f, 0.7f) + (s ? 2.f : 0.f)), m.query.push_back(uniform(seed, -0.7f, 0.7f)), m.query.push_back(uniform(seed, -0.7f, 0.7f));
    }
    m.qstart.push_back((int)m.query.size() / 3);
  }
  m.query[3] = INFINITY;      // one query that is not finite
  return m;
}

void run_exact(WArgs a, std::vector<double>& w, std::vector<unsigned char>& in) {
  a.winding = w.data(), a.inside = in.data();
  for (long long i = 0; i < a.nq; ++i) {
    const float* qf = a.query + i * 3;
    const int s = nn_find_scene(a.qstart, a.nscene, a.nq, i);
    const bool valid = s >= 0 && nn_finite(qf[0]) && nn_finite(qf[1]) && nn_finite(qf[2]);
    const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
    double S = 0.0;
    if (valid)
      for (long long f = nn_clamp(a.fstart[s], a.nf); f < nn_clamp(a.fstart[s + 1], a.nf); ++f) {
        float v[9];
        if (wn_load_face(a, f, v)) S += wn_omega(q, v);
      }
    wn_write(a, i, valid, S);
  }
}

// the exclusive scan of n + 1 words in place (mt_scan)
void scan(unsigned* words, size_t n) {
  unsigned run = 0;
  for (size_t k = 0; k <= n; ++k) {
    const unsigned t = words[k];
    words[k] = run, run += t;
  }
}

// MVD_WIND_CELLS serially, the build step by step as the kernels do it.  false: a list is not what the header says.
bool run_cells(WArgs a, int cells, double beta, std::vector<double>& w, std::vector<unsigned char>& in, long long* occupied) {
  WPlan p;
  if (!wn_plan((size_t)a.nf, a.nscene, MVD_WIND_CELLS, cells, p)) return false;
  std::vector<unsigned char> scratch(p.bytes, 0xa5);
  wn_point_scratch(a, p, scratch.data());
  a.winding = w.data(), a.inside = in.data(), a.bb = beta * beta;
  memset(a.box, 0xff, (size_t)a.nscene * 6 * sizeof(unsigned));
  memset(a.count, 0, mt_chunks(p.table) * kChunk * sizeof(unsigned));
  memset(a.occ, 0, mt_chunks(p.table) * kChunk * sizeof(unsigned));
  for (long long f = 0; f < a.nf; ++f) {      // wn_bounds_kernel
    const int s = nn_find_scene(a.fstart, a.nscene, a.nf, f);
    float v[9];
    if (s < 0 || !wn_load_face(a, f, v)) continue;
    for (int k = 0; k < 3; ++k) {
      const float mn = fminf(fminf(v[k], v[3 + k]), v[6 + k]), mx = fmaxf(fmaxf(v[k], v[3 + k]), v[6 + k]);
      unsigned* lo = a.box + (size_t)s * 6 + k;
      unsigned* hi = lo + 3;
      if (nn_key(mn) < *lo) *lo = nn_key(mn);
      if (~nn_key(mx) < *hi) *hi = ~nn_key(mx);
    }
  }
  long long candidates = 0;
  for (long long f = 0; f < a.nf; ++f) {      // wn_assign_kernel
    const int s = nn_find_scene(a.fstart, a.nscene, a.nf, f);
    float v[9];
    long long word = -1;
    if (s >= 0 && wn_load_face(a, f, v)) word = wn_word(a, s, v);
    if (word >= a.table) return false;
    a.face_cell[f] = (int)word;
    if (word >= 0) ++a.count[word], ++candidates;
  }
  for (long long k = 0; k < a.table; ++k) a.occ[k] = a.count[k] ? 1u : 0u;      // wn_flag_kernel
  scan(a.count, p.table), scan(a.occ, p.table);
  for (long long k = 0; k < a.table; ++k) {      // wn_ranges_kernel
    const unsigned b = a.count[k], e = a.count[k + 1];
    if (e <= b) continue;
    const long long r = a.occ[k];
    if (r >= a.ncell) return false;
    a.cursor[r] = b, a.cell[r].begin = b, a.cell[r].end = e;
  }
  for (long long f = a.nf - 1; f >= 0; --f) {      // wn_fill_kernel, in another order than the rows
    long long r, b, e;
    if (!wn_list_of(a, f, r, b, e)) continue;
    const long long at = a.cursor[r]++;
    if (at >= a.nf) return false;
    a.unsorted[at] = (int)f;
  }
  for (long long f = 0; f < a.nf; ++f) {      // wn_rank_kernel
    long long r, b, e, below = 0;
    if (!wn_list_of(a, f, r, b, e)) continue;
    for (long long k = b; k < e; ++k) below += a.unsorted[k] < f ? 1 : 0;
    float v[9];
    if (b + below >= e || !wn_load_face(a, f, v)) return false;
    for (int k = 0; k < 9; ++k) a.rec[(b + below) * 9 + k] = v[k];
  }
  *occupied = nn_clamp((long long)a.occ[a.table], a.ncell);
  long long members = 0;
  for (long long r = 0; r < *occupied; ++r) {      // wn_moment_kernel
    WCell c = a.cell[r];
    long long b, e;
    wn_members(c, a.nf, b, e);
    wn_moments(a.rec, b, e, c);
    a.cell[r] = c;
    members += e - b;
    if (!(c.rho2 > 0.0) || !std::isfinite(c.p[0]) || !std::isfinite(c.N[0])) return false;
  }
  if (members != candidates) return false;
  for (long long i = 0; i < a.nq; ++i) {      // wn_cells_kernel
    const float* qf = a.query + i * 3;
    const int s = nn_find_scene(a.qstart, a.nscene, a.nq, i);
    const bool valid = s >= 0 && nn_finite(qf[0]) && nn_finite(qf[1]) && nn_finite(qf[2]);
    const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
    double S = 0.0;
    if (valid) {
      const long long r0 = nn_clamp((long long)a.occ[(long long)s * a.c3], a.ncell), r1 = nn_clamp((long long)a.occ[(long long)(s + 1) * a.c3], a.ncell);
      for (long long r = r0; r < r1; ++r) S += wn_cell_term(a, a.cell[r], q);
    }
    wn_write(a, i, valid, S);
  }
  return true;
}

}  // namespace

int main() {
  const Mesh m = make_mesh();
  WArgs a{};
  a.query = m.query.data(), a.vertices = m.vertices.data(), a.qstart = m.qstart.data(), a.fstart = m.fstart.data(), a.faces = m.faces.data();
  a.nq = (long long)m.query.size() / 3, a.nv = (long long)m.vertices.size() / 3, a.nf = (long long)m.faces.size() / 3, a.nscene = 2;
  std::vector<double> exact(a.nq, -9.0);
  std::vector<unsigned char> exact_in(a.nq, 9);
  run_exact(a, exact, exact_in);
  long long bad = 0, inside = 0;
  for (long long i = 0; i < a.nq; ++i) {
    inside += exact_in[i];
    if (i == 1) bad += !std::isnan(exact[i]) || exact_in[i] != 0;
    else bad += !(fabs(exact[i] - round(exact[i])) < 1e-9);      // closed meshes: an integer
  }
  printf("exact: nq %lld nf %lld | inside %lld | not an integer (or the NaN query wrong) %lld\n", a.nq, a.nf, inside, bad);
  const int grids[] = {1, 2, 7, 0, 64};
  const double betas[] = {INFINITY, 2.0, 0.0};
  for (int g : grids)
    for (double beta : betas) {
      std::vector<double> w(a.nq, -9.0);
      std::vector<unsigned char> in(a.nq, 9);
      long long occupied = 0;
      if (!run_cells(a, g, beta, w, in, &occupied)) {
        printf("cells %d beta %g: PLAN OR LISTS FAILED\n", g, beta);
        ++bad;
        continue;
      }
      double worst = 0.0;
      long long other_bits = 0, flips = 0, wrong = 0;
      for (long long i = 0; i < a.nq; ++i) {
        if (std::isnan(exact[i])) {
          wrong += !std::isnan(w[i]);
          continue;
        }
        worst = fmax(worst, fabs(w[i] - exact[i]));
        other_bits += memcmp(&w[i], &exact[i], 8) != 0;
        flips += in[i] != exact_in[i];
        wrong += !std::isfinite(w[i]);
      }
      const double bound = beta == INFINITY ? (double)a.nf * ldexp(1.0, -48) : (beta == 2.0 ? 0.05 : INFINITY);
      if (worst > bound || wrong || (g == 1 && beta == INFINITY && other_bits) || (beta > 0.0 && flips)) ++bad;
      printf("cells %d beta %g: occupied %lld | largest |w - exact| %.3g (bound %.3g) | other bits %lld | inside flips %lld | not finite %lld\n", g, beta,
             occupied, worst, bound, other_bits, flips, wrong);
    }
  if (bad) printf("FAILED: %lld\n", bad);
  else printf("ok\n");
  return bad ? 1 : 0;
}
