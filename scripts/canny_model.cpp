// The device form of the Canny edge stage (videosd_amd/csrc/canny.hip) run on the CPU: the SAME step functions the four kernels loop over
// (videosd_amd/csrc/canny_core.h), tile by tile and pixel by pixel, on buffers of exactly the size the library asks for, compared byte for
// byte with the flood fill behind vsd_canny_host.  Built with the sanitizers, so a wrong index into `parent`, a tile array or the workspace
// is an error here and not an out-of-bounds access on the device.  Launch 2 runs in three pixel orders (raster, reverse, shuffled): the
// result must not depend on the order of the unions.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/canny_model.cpp -o /tmp/canny_model && /tmp/canny_model
//
// Exit status 0 and "canny_model: N cases ok" = clean.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <numeric>

#include "../videosd_amd/csrc/canny_core.h"

namespace {

struct Rng {  // (any noise will do here: the numpy cases of the tests are not restated)
  uint64_t s;
  double uniform() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
  }
  double normal() { return sqrt(-2.0 * log(1.0 - uniform())) * cos(6.283185307179586 * uniform()); }
};

std::vector<unsigned char> noise_frame(int h, int w, uint64_t seed) {
  std::vector<unsigned char> f((size_t)h * w * 3);
  Rng r{seed};
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x)
      for (int c = 0; c < 3; ++c) {
        const double v = 127 + 100 * sin(x / 7.0) * cos(y / 5.0) + 12 * r.normal();
        f[((size_t)y * w + x) * 3 + c] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
      }
  return f;
}

// a 3-pixel band that snakes across the frame at row pitch 8: one long component that crosses every tile border many times
std::vector<unsigned char> serpentine(int h, int w, bool seed) {
  std::vector<unsigned char> g((size_t)h * w, 100);
  std::vector<int> rows;
  for (int y = 4; y < h - 4 - 3; y += 8) rows.push_back(y);
  auto fill = [&](int ya, int yb, int xa, int xb, int v) {
    for (int y = std::max(ya, 0); y < std::min(yb, h); ++y)
      for (int x = std::max(xa, 0); x < std::min(xb, w); ++x) g[(size_t)y * w + x] = (unsigned char)v;
  };
  for (size_t i = 0; i < rows.size(); ++i) {
    fill(rows[i], rows[i] + 3, 4, w - 4, 130);
    if (i + 1 < rows.size()) {
      const int x = i % 2 == 0 ? w - 4 - 3 : 4;
      fill(rows[i], rows[i + 1] + 3, x, x + 3, 130);
    }
  }
  if (seed && !rows.empty()) fill(rows[0], rows[0] + 3, 4, 10, 190);
  std::vector<unsigned char> f((size_t)h * w * 3);
  for (size_t i = 0; i < g.size(); ++i) f[3 * i] = f[3 * i + 1] = f[3 * i + 2] = g[i];
  return f;
}

int g_cases = 0;

bool run_case(const char* name, const std::vector<unsigned char>& frame, int h, int w, int low, int high) {
  const size_t n = (size_t)h * w;
  // exact-size heap blocks: the sanitizer sees every byte past them
  std::unique_ptr<unsigned char[]> rgb(new unsigned char[n * 3]), ref(new unsigned char[n]), got(new unsigned char[n]);
  memcpy(rgb.get(), frame.data(), n * 3);
  if (!canny_host(rgb.get(), h, w, low, high, ref.get())) {
    printf("%s: canny_host refused %d x %d (%d, %d)\n", name, w, h, low, high);
    return false;
  }
  const int64_t ws_bytes = canny_workspace_bytes(h, w);
  bool ok = true;
  size_t n_cand = 0, n_strong = 0, n_edge = 0;
  for (int order = 0; order < 3; ++order) {
    std::unique_ptr<unsigned char[]> ws(new unsigned char[(size_t)ws_bytes]);
    memset(ws.get(), 0xA5, (size_t)ws_bytes);  // (nothing may rely on a zeroed workspace)
    int* parent = (int*)ws.get();
    unsigned char* strong = ws.get() + n * 4;
    unsigned char* flag = strong + n;
    // launch 1
    std::unique_ptr<CannyTile> t(new CannyTile);
    for (int y0 = 0; y0 < h; y0 += CANNY_TH)
      for (int x0 = 0; x0 < w; x0 += CANNY_TW) {
        memset(t.get(), 0xA5, sizeof(CannyTile));
        for (int q = 0; q < CANNY_GRAY_N; ++q) canny_tile_gray(*t, rgb.get(), h, w, x0, y0, q);
        for (int q = 0; q < CANNY_MAG_N; ++q) canny_tile_mag(*t, h, w, x0, y0, q);
        for (int q = 0; q < CANNY_TILE_N; ++q) canny_tile_class(*t, h, w, x0, y0, low, high, q);
        for (int q = 0; q < CANNY_TILE_N; ++q) canny_tile_unite(*t, order == 1 ? CANNY_TILE_N - 1 - q : q);
        for (int q = 0; q < CANNY_TILE_N; ++q) canny_tile_write(*t, h, w, x0, y0, q, parent, strong, flag);
      }
    for (size_t i = 0; i < n; ++i)
      if (parent[i] < -1 || parent[i] > (int)i || (parent[i] >= 0 && parent[parent[i]] != parent[i])) {
        printf("%s: launch 1 left parent[%zu] = %d\n", name, i, parent[i]);
        return false;
      }
    // launch 2
    std::vector<int> idx(n);
    std::iota(idx.begin(), idx.end(), 0);
    if (order == 1) std::reverse(idx.begin(), idx.end());
    if (order == 2) {
      Rng r{12345};
      for (size_t i = n; i > 1; --i) std::swap(idx[i - 1], idx[(size_t)(r.uniform() * i)]);
    }
    for (int i : idx) {
      const int y = i / w, x = i - y * w;
      if (canny_on_tile_border(x, y)) canny_border_unite(parent, h, w, x, y);
    }
    for (size_t i = 0; i < n; ++i)
      if (parent[i] < -1 || parent[i] > (int)i) {
        printf("%s: launch 2 left parent[%zu] = %d\n", name, i, parent[i]);
        return false;
      }
    // launches 3 and 4
    for (int i : idx) canny_mark(parent, strong, flag, i);
    for (size_t i = 0; i < n; ++i) got[i] = canny_is_edge(parent, flag, (int)i) ? 255 : 0;
    if (memcmp(got.get(), ref.get(), n)) {
      size_t bad = 0, first = n;
      for (size_t i = 0; i < n; ++i)
        if (got[i] != ref[i]) {
          ++bad;
          if (first == n) first = i;
        }
      printf("%s (order %d): %zu of %zu pixels differ from the flood fill, first at (%zu, %zu)\n", name, order, bad, n, first % w, first / w);
      ok = false;
    }
    if (order == 0)
      for (size_t i = 0; i < n; ++i) {
        n_cand += parent[i] >= 0;
        n_strong += strong[i];
        n_edge += got[i] != 0;
      }
  }
  printf("%-28s %4d x %-4d (%4d, %4d): %6zu candidates, %5zu strong, %6zu edges  %s\n", name, w, h, low, high, n_cand, n_strong, n_edge, ok ? "ok" : "FAILED");
  ++g_cases;
  return ok;
}

}  // namespace

int main() {
  bool ok = true;
  const int noise_sizes[][2] = {{72, 120}, {64, 64}, {37, 301}, {128, 128}, {16, 32}, {17, 33}, {15, 31}, {48, 97}};
  for (auto& s : noise_sizes)
    for (int k = 0; k < 2; ++k) ok &= run_case("noise", noise_frame(s[0], s[1], 1 + (uint64_t)s[0] * 1000 + s[1]), s[0], s[1], k ? 50 : 100, k ? 150 : 200);
  const int serp_sizes[][2] = {{72, 120}, {40, 520}, {136, 264}, {264, 136}};
  for (auto& s : serp_sizes)
    for (int seed = 0; seed < 2; ++seed) ok &= run_case(seed ? "serpentine, seeded" : "serpentine, no seed", serpentine(s[0], s[1], seed != 0), s[0], s[1], 100, 200);
  const int small[][2] = {{1, 1}, {1, 7}, {7, 1}, {3, 3}, {2, 2}, {1, 33}, {17, 1}};
  for (auto& s : small) {
    ok &= run_case("small", noise_frame(s[0], s[1], 7), s[0], s[1], 100, 200);
    ok &= run_case("small, (0, 0)", noise_frame(s[0], s[1], 8), s[0], s[1], 0, 0);
  }
  ok &= run_case("constant", std::vector<unsigned char>((size_t)40 * 70 * 3, 93), 40, 70, 0, 0);
  ok &= run_case("noise, low == high", noise_frame(64, 64, 3), 64, 64, 120, 120);
  ok &= run_case("noise, (0, 0)", noise_frame(64, 64, 4), 64, 64, 0, 0);
  ok &= run_case("noise, (2040, 2040)", noise_frame(64, 64, 5), 64, 64, 2040, 2040);
  ok &= run_case("binary noise, (0, 0)", [] {
    std::vector<unsigned char> f((size_t)50 * 90 * 3);
    Rng r{99};
    for (size_t i = 0; i < f.size(); i += 3) f[i] = f[i + 1] = f[i + 2] = r.uniform() < 0.5 ? 0 : 255;
    return f;
  }(), 50, 90, 0, 0);
  if (!ok) {
    printf("canny_model: FAILED\n");
    return 1;
  }
  printf("canny_model: %d cases ok\n", g_cases);
  return 0;
}
