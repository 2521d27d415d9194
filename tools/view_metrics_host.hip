// The host-and-device index arithmetic of csrc/view_metrics.hip run serially on a CPU, with no GPU: the tile plan, the halo addressing of
// the staged tile, the two filter passes through the one fp64 plane, the chunk walk of the pixel-wise sums and the layout of the
// partials in the scratch, on images made here.  Meant to be built with the host sanitizers before the kernels first run on a GPU:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -I include \
//         tools/view_metrics_host.hip -o view_metrics_host           (the sanitizers on the host pass only; nothing here touches a GPU)
//   ./view_metrics_host
//
// Checked, for every shape below (Ho in {1, 15, 16, 17, 33}, Wo in {1, 31, 32, 33, 65}, windows 3, 11, 33, C in {1, 3}, B in {1, 2, 5}):
// every read of an image, of the mask and of the two LDS arrays is inside its array (the arrays are vectors of exactly the kernel's
// sizes, pre-filled with NaN, so a read of a word that was not staged shows in the result as well); the map the tiles produce has the
// bits of a plain double loop over the window; every window position and every pixel is visited exactly once; the scratch is a vector
// of exactly mvd_image_metrics_scratch / mvd_depth_metrics_scratch bytes pre-filled with a pattern, every word of it is written exactly
// once, and the sums of the partials in the second stage's order equal the plain sums within n * 2^-52 * sum|term|.
#include "../mvdfusion_amd/csrc/view_metrics.hip"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

void mvd_set_error(const char*, ...) {}

namespace {

unsigned lcg(unsigned& s) { return s = s * 1664525u + 1013904223u; }
float uniform(unsigned& s) { return (float)(lcg(s) >> 8) / 16777216.f; }

double moment(int m, float x, float y) {
  switch (m) {
    case 0: return vm_moment<0>(x, y);
    case 1: return vm_moment<1>(x, y);
    case 2: return vm_moment<2>(x, y);
    case 3: return vm_moment<3>(x, y);
    default: return vm_moment<4>(x, y);
  }
}

constexpr unsigned long long kPattern = 0xa5a5a5a5a5a5a5a5ull;

struct Scratch {
  std::vector<unsigned long long> words;
  std::vector<int> writes;
  explicit Scratch(size_t n) : words(n, kPattern), writes(n, 0) {}
  void put(size_t at, double v) { memcpy(&words.at(at), &v, 8), ++writes.at(at); }
  void put(size_t at, long long v) { memcpy(&words.at(at), &v, 8), ++writes.at(at); }
  double f(size_t at) const {
    double v;
    memcpy(&v, &words.at(at), 8);
    return v;
  }
  long long n(size_t at) const { return (long long)words.at(at); }
  bool all_once() const {
    for (int w : writes)
      if (w != 1) return false;
    return true;
  }
};

// the second stage's order: thread t takes t, t + 256, ... ascending, then the tree
template <typename T, typename Get>
T second_stage(size_t n, Get get) {
  std::vector<T> red(kVmThreads, T(0));
  for (int t = 0; t < kVmThreads; ++t)
    for (size_t i = t; i < n; i += kVmThreads) red[t] = red[t] + get(i);
  for (int s = kVmThreads / 2; s > 0; s >>= 1)
    for (int t = 0; t < s; ++t) red[t] = red[t] + red[t + s];
  return red[0];
}

int run_image(int B, int C, int H, int W, int window, unsigned seed) {
  VmImagePlan p;
  if (!vm_image_plan(B, C, H, W, window, p) || mvd_image_metrics_scratch(B, C, H, W, window) != p.words * 8) return 1;
  const size_t HW = (size_t)H * W;
  std::vector<float> a((size_t)B * C * HW), b(a.size());
  std::vector<unsigned char> mask((size_t)B * HW);
  for (auto& v : a) v = uniform(seed);
  for (auto& v : b) v = uniform(seed);
  for (auto& v : mask) v = uniform(seed) < 0.6f ? 1 : 0;
  std::vector<double> w(window);
  double total = 0.0;
  for (int k = 0; k < window; ++k) total += (w[k] = exp(-(double)((k - window / 2) * (k - window / 2)) / 4.5));
  for (auto& v : w) v /= total;
  Scratch sc(p.words);
  std::vector<double> map((size_t)B * C * p.Ho * p.Wo, NAN);
  std::vector<int> visits(map.size(), 0);
  int bad = 0;
  const int half = window / 2;
  for (size_t pl = 0; pl < (size_t)B * C; ++pl) {
    const size_t img = pl / C;
    for (long long tile = 0; tile < p.ntile; ++tile) {      // vm_ssim_kernel, one workgroup
      std::vector<float> xs(kVmInH * kVmInW, NAN), ys(kVmInH * kVmInW, NAN);
      std::vector<double> plane(kVmInH * kVmTileW, NAN);
      int r0, c0, th, tw;
      vm_tile(tile, p.tiles_x, p.Ho, p.Wo, r0, c0, th, tw);
      if (th < 1 || tw < 1 || th > kVmTileH || tw > kVmTileW) return 1;
      const int inh = th + window - 1, inw = tw + window - 1;
      for (int i = 0; i < inh * inw; ++i) {
        int lds;
        size_t pixel;
        vm_stage(i, inw, r0, c0, W, lds, pixel);
        if (pixel >= HW) return 1;
        xs.at(lds) = a.at(pl * HW + pixel), ys.at(lds) = b.at(pl * HW + pixel);
      }
      std::vector<double> e((size_t)kVmTileW * kVmTileH * 5, NAN);
      for (int m = 0; m < 5; ++m) {
        for (int i = 0; i < inh * kVmTileW; ++i) {
          const int r = i >> 5, c = i & 31;
          if (c >= tw) continue;
          double s = 0.0;
          for (int k = 0; k < window; ++k) s = s + w[k] * moment(m, xs.at(r * kVmInW + c + k), ys.at(r * kVmInW + c + k));
          plane.at(i) = s;
        }
        for (int i = 0; i < kVmTileW * kVmTileH; ++i) {
          const int ro = i >> 5, co = i & 31;
          if (ro >= th || co >= tw) continue;
          double s = 0.0;
          for (int k = 0; k < window; ++k) s = s + w[k] * plane.at((ro + k) * kVmTileW + co);
          e[(size_t)i * 5 + m] = s;
        }
      }
      double sum = 0.0;
      long long n = 0;
      for (int i = 0; i < kVmTileW * kVmTileH; ++i) {
        const int ro = i >> 5, co = i & 31;
        if (ro >= th || co >= tw) continue;
        const double v = vm_ssim(&e[(size_t)i * 5], 1e-4, 9e-4);
        const size_t at = (pl * (size_t)p.Ho + (size_t)(r0 + ro)) * (size_t)p.Wo + (size_t)(c0 + co);
        map.at(at) = v, ++visits.at(at);
        if (mask.at(img * HW + (size_t)(r0 + ro + half) * W + (size_t)(c0 + co + half))) sum = sum + v, ++n;
      }
      sc.put(p.ssim_part + pl * (size_t)p.ntile + tile, sum);
      if (pl % C == 0) sc.put(p.scnt_part + img * (size_t)p.ntile + tile, n);
    }
  }
  for (size_t img = 0; img < (size_t)B; ++img)      // vm_sq_kernel
    for (long long chunk = 0; chunk < p.nchunk; ++chunk) {
      double sum = 0.0;
      long long n = 0;
      for (int t = 0; t < kVmChunk; ++t) {
        const size_t px = (size_t)chunk * kVmChunk + t;
        if (px >= HW || !mask.at(img * HW + px)) continue;
        ++n;
        for (int c = 0; c < C; ++c) {
          const double d = (double)a.at((img * C + c) * HW + px) - (double)b.at((img * C + c) * HW + px);
          sum = sum + d * d;
        }
      }
      sc.put(p.sq_part + img * (size_t)p.nchunk + chunk, sum), sc.put(p.cnt_part + img * (size_t)p.nchunk + chunk, n);
    }
  if (!sc.all_once()) ++bad, printf("  scratch: a word not written exactly once\n");
  for (int v : visits) bad += v != 1;
  // the plain double loop, the same operations in the same order
  size_t other_bits = 0;
  for (size_t pl = 0; pl < (size_t)B * C; ++pl)
    for (long long r = 0; r < p.Ho; ++r)
      for (long long c = 0; c < p.Wo; ++c) {
        double e[5];
        for (int m = 0; m < 5; ++m) {
          std::vector<double> h(window);
          for (int kr = 0; kr < window; ++kr) {
            double s = 0.0;
            for (int k = 0; k < window; ++k) {
              const size_t at = pl * HW + (size_t)(r + kr) * W + (size_t)(c + k);
              s = s + w[k] * moment(m, a[at], b[at]);
            }
            h[kr] = s;
          }
          double s = 0.0;
          for (int k = 0; k < window; ++k) s = s + w[k] * h[k];
          e[m] = s;
        }
        const double v = vm_ssim(e, 1e-4, 9e-4), got = map[(pl * (size_t)p.Ho + r) * (size_t)p.Wo + c];
        other_bits += memcmp(&v, &got, 8) != 0;
      }
  bad += other_bits != 0;
  // the second stage against plain sums
  for (size_t img = 0; img < (size_t)B; ++img) {
    const double ss = second_stage<double>((size_t)C * p.ntile, [&](size_t i) { return sc.f(p.ssim_part + img * C * (size_t)p.ntile + i); });
    const long long sn = second_stage<long long>((size_t)p.ntile, [&](size_t i) { return sc.n(p.scnt_part + img * (size_t)p.ntile + i); });
    const long long cn = second_stage<long long>((size_t)p.nchunk, [&](size_t i) { return sc.n(p.cnt_part + img * (size_t)p.nchunk + i); });
    double plain = 0.0, mag = 0.0;
    long long pn = 0, pc = 0;
    for (int c = 0; c < C; ++c)
      for (long long r = 0; r < p.Ho; ++r)
        for (long long q = 0; q < p.Wo; ++q)
          if (mask[img * HW + (size_t)(r + half) * W + (size_t)(q + half)]) {
            const double v = map[((img * C + c) * (size_t)p.Ho + r) * (size_t)p.Wo + q];
            plain += v, mag += fabs(v), pn += c == 0;
          }
    for (size_t px = 0; px < HW; ++px) pc += mask[img * HW + px];
    if (sn != pn || cn != pc || !(fabs(ss - plain) <= (double)(C * pn + 1) * ldexp(1.0, -52) * mag)) ++bad;
  }
  printf("image B %d C %d %d x %d window %2d: tiles %lld x %lld, chunks %lld, scratch %zu words | map values with other bits %zu | %s\n", B, C, H, W,
         window, p.tiles_y, p.tiles_x, p.nchunk, p.words, other_bits, bad ? "FAILED" : "ok");
  return bad;
}

int run_depth(int B, int H, int W, int align, unsigned seed) {
  VmDepthPlan p;
  if (!vm_depth_plan(B, H, W, p) || mvd_depth_metrics_scratch(B, H, W) != p.words * 8) return 1;
  const size_t HW = (size_t)H * W;
  std::vector<float> pred((size_t)B * HW), target(pred.size());
  for (auto& v : pred) v = 0.5f + 2.f * uniform(seed);
  for (auto& v : target) v = 0.5f + 2.f * uniform(seed);
  pred[0] = INFINITY, target[HW - 1] = -1.f;
  Scratch sc(p.words);
  int bad = 0;
  std::vector<int> visits(pred.size(), 0);
  for (size_t img = 0; img < (size_t)B; ++img) {
    for (long long chunk = 0; chunk < p.nchunk; ++chunk) {      // vm_depth_fit_kernel
      double S[kVmFitSums] = {0, 0, 0, 0};
      long long n = 0;
      for (int t = 0; t < kVmChunk; ++t) {
        const size_t i = (size_t)chunk * kVmChunk + t;
        if (i >= HW) continue;
        ++visits.at(img * HW + i);
        const float pf = pred.at(img * HW + i), tf = target.at(img * HW + i);
        if (!vm_depth_ok(pf, tf)) continue;
        ++n, S[0] += pf, S[1] += tf, S[2] += (double)pf * pf, S[3] += (double)pf * tf;
      }
      const size_t at = img * (size_t)p.nchunk + chunk;
      for (int k = 0; k < kVmFitSums; ++k) sc.put(p.fit_part + at * kVmFitSums + k, S[k]);
      sc.put(p.n_part + at, n);
    }
    double S[kVmFitSums];      // vm_depth_solve_kernel
    for (int k = 0; k < kVmFitSums; ++k)
      S[k] = second_stage<double>((size_t)p.nchunk, [&](size_t i) { return sc.f(p.fit_part + (img * (size_t)p.nchunk + i) * kVmFitSums + k); });
    const long long n = second_stage<long long>((size_t)p.nchunk, [&](size_t i) { return sc.n(p.n_part + img * (size_t)p.nchunk + i); });
    double s, b;
    vm_solve(align, n, S, s, b);
    sc.put(p.fit + img * 2, s), sc.put(p.fit + img * 2 + 1, b);
    if (!std::isfinite(s) || !std::isfinite(b)) ++bad;
    for (long long chunk = 0; chunk < p.nchunk; ++chunk) {      // vm_depth_err_kernel: the layout of its partials
      const size_t at = img * (size_t)p.nchunk + chunk;
      for (int k = 0; k < kVmErrSums; ++k) sc.put(p.err_part + at * kVmErrSums + k, 0.0);
      for (int k = 0; k < kVmErrCounts; ++k) sc.put(p.cnt_part + at * kVmErrCounts + k, 0ll);
    }
  }
  if (!sc.all_once()) ++bad;
  for (int v : visits) bad += v != 1;
  printf("depth B %d %d x %d align %d: chunks %lld, scratch %zu words | %s\n", B, H, W, align, p.nchunk, p.words, bad ? "FAILED" : "ok");
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  const int shapes[][5] = {{1, 1, 11, 41, 11}, {1, 3, 25, 43, 11}, {5, 1, 26, 42, 11}, {1, 3, 27, 41, 11}, {1, 1, 27, 11, 11}, {1, 3, 19, 35, 3},
                           {2, 1, 35, 67, 3},  {1, 1, 47, 64, 33}, {1, 3, 33, 34, 33}, {1, 1, 65, 97, 33}, {2, 3, 3, 3, 3}};
  unsigned seed = 2024u;
  for (auto& s : shapes) bad += run_image(s[0], s[1], s[2], s[3], s[4], seed++);
  const int depths[][4] = {{1, 1, 3, 1}, {2, 40, 53, 1}, {1, 32, 64, 2}, {1, 1, 2049, 2}, {5, 9, 13, 0}, {3, 64, 97, 2}};
  for (auto& d : depths) bad += run_depth(d[0], d[1], d[2], d[3], seed++);
  VmImagePlan ip;
  VmDepthPlan dp;
  const bool refused = !vm_image_plan(1, 1, 10, 20, 11, ip) && !vm_image_plan(1, 1, 20, 20, 4, ip) && !vm_image_plan(1, 1, 40, 40, 35, ip) &&
                       !vm_image_plan(300, 300, 8, 8, 0, ip) && !vm_image_plan(1, 1, 32769, 8, 0, ip) && !vm_depth_plan(65536, 4, 4, dp) &&
                       !vm_depth_plan(1, 0, 4, dp) && vm_image_plan(0, 3, 12, 14, 11, ip) && ip.words == 0 && vm_image_plan(65535, 1, 32768, 32768, 33, ip);
  if (!refused) ++bad, printf("plans: a limit is not held\n");
  if (bad) printf("FAILED: %d\n", bad);
  else printf("ok\n");
  return bad ? 1 : 0;
}
