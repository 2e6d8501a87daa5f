// THE EDGE CONTRACT of include/vsd.h in executable form: the per-pixel arithmetic, the host flood fill behind vsd_canny_host, and the
// label steps of the device form (csrc/canny.hip).  Plain C++ that also compiles as HIP device code: the kernels are loops over these
// steps with barriers in between, and scripts/canny_model.cpp runs the SAME steps tile by tile on the CPU under the sanitizers and
// compares the result with the flood fill -- a wrong index into `parent` is found there, not on the device.
//
// The device form in four launches (no memset node, no host sync, no cooperative launch, no loop that waits for another workgroup):
//   1. tile:   one workgroup per CANNY_TW x CANNY_TH tile.  Gray values with a 2-pixel apron and magnitudes with a 1-pixel apron in
//              LDS, class per pixel, union-find of the tile's candidates in LDS; parent[i] = global index of the pixel's tile-local
//              root (-1: no candidate), strong[i], flag[i] = 0.
//   2. border: a candidate whose W / NW / N / NE neighbour lies in ANOTHER tile unites its root with that neighbour's: union-find
//              over `parent` with atomic minima, invariant parent[x] <= x.
//   3. mark:   every strong pixel stores 1 to flag[find(i)] (same-value races).
//   4. write:  edge = candidate && flag[find(i)].
// The result is the set of candidates whose component holds a strong one: a function of the input alone, whatever the order of the
// atomics.
#pragma once
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CANNY_HD __host__ __device__ __forceinline__
#else
#define CANNY_HD inline
#endif

// The atomics of the label steps, behind one switch.  Launch 2 reads and lowers words that other workgroups lower in the same launch:
// per-XCD L2s are not coherent and a CU's L1 is never refreshed by another CU's stores, so EVERY access there is an agent-scope relaxed
// atomic.  The tile pass uses the same two on LDS (one workgroup; the scope costs nothing there).  On the host the steps run one after
// the other.
#if defined(__HIP_DEVICE_COMPILE__)
#define CANNY_LOAD(P_) __hip_atomic_load((P_), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define CANNY_FETCH_MIN(P_, V_) __hip_atomic_fetch_min((P_), (V_), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#else
#define CANNY_LOAD(P_) (*(P_))
#define CANNY_FETCH_MIN(P_, V_) canny_host_fetch_min((P_), (V_))
inline int canny_host_fetch_min(int* p, int v) {
  const int old = *p;
  if (v < old) *p = v;
  return old;
}
#endif

constexpr int CANNY_TW = 32, CANNY_TH = 16;  // tile of launch 1
constexpr int CANNY_MAX_MAG = 2040;          // |dx| + |dy| <= 2 * 4 * 255
constexpr int CANNY_MAX_SIDE = 16384;        // (= VSD_RESAMPLE_MAX_SIDE: h * w <= 2^28, every pixel index fits an int)

// ---- per pixel ---------------------------------------------------------------------------------------------------------------------
CANNY_HD int canny_gray(int r, int g, int b) { return (int)(((unsigned)r * 19595u + (unsigned)g * 38470u + (unsigned)b * 7471u + 0x8000u) >> 16); }  // PIL convert("L")

// 3 x 3 Sobel of the gray values a b c / d . f / g h i
CANNY_HD void canny_sobel(int a, int b, int c, int d, int f, int g, int h, int i, int& dx, int& dy) {
  dx = (c + 2 * f + i) - (a + 2 * d + g);
  dy = (g + 2 * h + i) - (a + 2 * b + c);
}

// candidate = above `low` and a maximum along its gradient.  m: this pixel's magnitude; l r u d ul ur dl dr: the neighbours' (0 outside
// the image).  Ranges: x = |dx| <= 1020, so t22 = 13573 x <= 13 844 460 and t67 = t22 + (x << 16) <= 80 691 180; y = |dy| << 15 <=
// 33 423 360: all below 2^31, plain int arithmetic is exact.
CANNY_HD bool canny_candidate(int dx, int dy, int m, int l, int r, int u, int d, int ul, int ur, int dl, int dr, int low) {
  if (m <= low) return false;
  const int x = dx < 0 ? -dx : dx, y = (dy < 0 ? -dy : dy) << 15;
  const int t22 = x * 13573, t67 = t22 + (x << 16);
  if (y < t22) return m > l && m >= r;
  if (y > t67) return m > u && m >= d;
  return (dx ^ dy) < 0 ? (m > ur && m > dl) : (m > ul && m > dr);
}

// ---- union-find over an int array with parent[x] <= x -------------------------------------------------------------------------------
// Terminates by itself: every trip replaces x by a strictly smaller non-negative index (a word that breaks the invariant -- negative,
// or above x -- ends the walk at x instead of being followed), so there are at most x + 1 trips whatever other threads do.
CANNY_HD int canny_find(int* parent, int x) {
  for (;;) {
    const int p = CANNY_LOAD(parent + x);
    if ((unsigned)p >= (unsigned)x) return x;
    x = p;
  }
}
CANNY_HD int canny_find_plain(const int* parent, int x) {  // (behind a kernel boundary: nobody writes `parent` any more)
  for (;;) {
    const int p = parent[x];
    if ((unsigned)p >= (unsigned)x) return x;
    x = p;
  }
}

// Hang the larger root under the smaller.  The minimum fails to do that only when another thread gave `a` a parent `old` < a after
// this thread's find; the word then holds min(old, b), so what is left is to unite old with b.  Terminates by itself: every trip but the
// last replaces the larger of (a, b) by a strictly smaller index and never raises the other, so a + b falls every trip: at most
// a + b + 1 trips whatever other threads do.  Nothing here waits for another thread.
CANNY_HD void canny_unite(int* parent, int a, int b) {
  for (;;) {
    a = canny_find(parent, a);
    b = canny_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = CANNY_FETCH_MIN(parent + a, b);
    if (old == a) return;
    a = old;
  }
}

// ---- launch 1, step by step (q: index of the step's own range; x0, y0: the tile's first pixel) -------------------------------------
struct CannyTile {
  unsigned char g[CANNY_TH + 4][CANNY_TW + 4];   // gray value of pixel (y0 - 2 + r, x0 - 2 + c), coordinates clamped into the image
  unsigned short m[CANNY_TH + 2][CANNY_TW + 2];  // magnitude of pixel (y0 - 1 + r, x0 - 1 + c), 0 outside the image
  unsigned char strong[CANNY_TH][CANNY_TW];
  int lab[CANNY_TH * CANNY_TW];                  // tile-local union-find: q, or -1 where there is no candidate
};
constexpr int CANNY_GRAY_N = (CANNY_TH + 4) * (CANNY_TW + 4), CANNY_MAG_N = (CANNY_TH + 2) * (CANNY_TW + 2), CANNY_TILE_N = CANNY_TH * CANNY_TW;

CANNY_HD void canny_tile_gray(CannyTile& t, const unsigned char* rgb, int h, int w, int x0, int y0, int q) {
  const int r = q / (CANNY_TW + 4), c = q - r * (CANNY_TW + 4);
  int yy = y0 - 2 + r, xx = x0 - 2 + c;
  yy = yy < 0 ? 0 : (yy > h - 1 ? h - 1 : yy);
  xx = xx < 0 ? 0 : (xx > w - 1 ? w - 1 : xx);
  const unsigned char* p = rgb + ((size_t)yy * w + xx) * 3;
  t.g[r][c] = (unsigned char)canny_gray(p[0], p[1], p[2]);
}

// gradient of the pixel whose gray value is t.g[r][c] (1 <= r <= CANNY_TH + 2, 1 <= c <= CANNY_TW + 2)
CANNY_HD void canny_tile_sobel(const CannyTile& t, int r, int c, int& dx, int& dy) {
  canny_sobel(t.g[r - 1][c - 1], t.g[r - 1][c], t.g[r - 1][c + 1], t.g[r][c - 1], t.g[r][c + 1], t.g[r + 1][c - 1], t.g[r + 1][c], t.g[r + 1][c + 1], dx, dy);
}

CANNY_HD void canny_tile_mag(CannyTile& t, int h, int w, int x0, int y0, int q) {
  const int r = q / (CANNY_TW + 2), c = q - r * (CANNY_TW + 2);
  const int yy = y0 - 1 + r, xx = x0 - 1 + c;
  int m = 0;
  if ((unsigned)yy < (unsigned)h && (unsigned)xx < (unsigned)w) {
    int dx, dy;
    canny_tile_sobel(t, r + 1, c + 1, dx, dy);
    m = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
  }
  t.m[r][c] = (unsigned short)m;
}

CANNY_HD void canny_tile_class(CannyTile& t, int h, int w, int x0, int y0, int low, int high, int q) {
  const int ly = q / CANNY_TW, lx = q - ly * CANNY_TW;
  bool cand = false;
  int m = 0;
  if (y0 + ly < h && x0 + lx < w) {
    int dx, dy;
    canny_tile_sobel(t, ly + 2, lx + 2, dx, dy);
    const int r = ly + 1, c = lx + 1;
    m = t.m[r][c];
    cand = canny_candidate(dx, dy, m, t.m[r][c - 1], t.m[r][c + 1], t.m[r - 1][c], t.m[r + 1][c], t.m[r - 1][c - 1], t.m[r - 1][c + 1], t.m[r + 1][c - 1],
                           t.m[r + 1][c + 1], low);
  }
  t.lab[q] = cand ? q : -1;
  t.strong[ly][lx] = (unsigned char)(cand && m > high);
}

// every 8-connected pair of the tile is met once, from the later pixel of the two in raster order
CANNY_HD void canny_tile_unite(CannyTile& t, int q) {
  if (CANNY_LOAD(t.lab + q) < 0) return;  // (the sign of a word never changes: only roots, which are candidates, are ever lowered)
  const int ly = q / CANNY_TW, lx = q - ly * CANNY_TW;
  if (lx > 0 && CANNY_LOAD(t.lab + q - 1) >= 0) canny_unite(t.lab, q, q - 1);
  if (ly > 0) {
    if (lx > 0 && CANNY_LOAD(t.lab + q - CANNY_TW - 1) >= 0) canny_unite(t.lab, q, q - CANNY_TW - 1);
    if (CANNY_LOAD(t.lab + q - CANNY_TW) >= 0) canny_unite(t.lab, q, q - CANNY_TW);
    if (lx < CANNY_TW - 1 && CANNY_LOAD(t.lab + q - CANNY_TW + 1) >= 0) canny_unite(t.lab, q, q - CANNY_TW + 1);
  }
}

// pixels of the tile outside the image write nothing; a root lies inside the image because only candidates are roots
CANNY_HD void canny_tile_write(CannyTile& t, int h, int w, int x0, int y0, int q, int* parent, unsigned char* strong, unsigned char* flag) {
  const int ly = q / CANNY_TW, lx = q - ly * CANNY_TW;
  if (y0 + ly >= h || x0 + lx >= w) return;
  const int i = (y0 + ly) * w + x0 + lx;
  int p = -1;
  if (t.lab[q] >= 0) {
    const int root = canny_find(t.lab, q), ry = root / CANNY_TW, rx = root - ry * CANNY_TW;
    p = (y0 + ry) * w + x0 + rx;  // (<= i: the root is the tile's smallest q of the component, and q orders pixels as i does)
  }
  parent[i] = p;
  strong[i] = t.strong[ly][lx];
  flag[i] = 0;
}

// ---- launches 2 to 4, per pixel i = y * w + x --------------------------------------------------------------------------------------
CANNY_HD bool canny_on_tile_border(int x, int y) {  // has a W / NW / N / NE neighbour in another tile
  const int lx = x % CANNY_TW, ly = y % CANNY_TH;
  return lx == 0 || ly == 0 || lx == CANNY_TW - 1;
}

CANNY_HD void canny_border_unite(int* parent, int h, int w, int x, int y) {
  (void)h;
  const int i = y * w + x, lx = x % CANNY_TW, ly = y % CANNY_TH;
  if (CANNY_LOAD(parent + i) < 0) return;
  if (lx == 0 && x > 0 && CANNY_LOAD(parent + i - 1) >= 0) canny_unite(parent, i, i - 1);
  if (y > 0) {
    if ((lx == 0 || ly == 0) && x > 0 && CANNY_LOAD(parent + i - w - 1) >= 0) canny_unite(parent, i, i - w - 1);
    if (ly == 0 && CANNY_LOAD(parent + i - w) >= 0) canny_unite(parent, i, i - w);
    if ((lx == CANNY_TW - 1 || ly == 0) && x < w - 1 && CANNY_LOAD(parent + i - w + 1) >= 0) canny_unite(parent, i, i - w + 1);
  }
}

CANNY_HD void canny_mark(const int* parent, const unsigned char* strong, unsigned char* flag, int i) {
  if (strong[i]) flag[canny_find_plain(parent, i)] = 1;
}

CANNY_HD bool canny_is_edge(const int* parent, const unsigned char* flag, int i) { return parent[i] >= 0 && flag[canny_find_plain(parent, i)] != 0; }

// workspace of the device form: parent int[h * w] | strong u8[h * w] | flag u8[h * w], rounded up to 256 bytes
inline int64_t canny_workspace_bytes(int h, int w) {
  if (h < 1 || w < 1 || h > CANNY_MAX_SIDE || w > CANNY_MAX_SIDE) return 0;
  return (((int64_t)h * w * 6) + 255) / 256 * 256;
}

inline bool canny_args_ok(int h, int w, int low, int high) {
  return h >= 1 && w >= 1 && h <= CANNY_MAX_SIDE && w <= CANNY_MAX_SIDE && 0 <= low && low <= high && high <= CANNY_MAX_MAG;
}

// ---- the contract as plain host loops: magnitudes, classes, then a stack flood fill from every strong pixel -----------------------
inline bool canny_host(const unsigned char* rgb, int h, int w, int low, int high, unsigned char* edge) {
  if (!rgb || !edge || !canny_args_ok(h, w, low, high)) return false;
  const size_t n = (size_t)h * w;
  std::vector<unsigned char> gray(n), cls(n);  // cls: 0 none, 1 candidate, 2 strong candidate
  std::vector<short> gx(n), gy(n);
  std::vector<int> mag(n);
  for (size_t i = 0; i < n; ++i) gray[i] = (unsigned char)canny_gray(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
  auto G = [&](int y, int x) -> int {
    y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
    x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x);
    return gray[(size_t)y * w + x];
  };
  auto M = [&](int y, int x) -> int { return ((unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w) ? mag[(size_t)y * w + x] : 0; };
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      int dx, dy;
      canny_sobel(G(y - 1, x - 1), G(y - 1, x), G(y - 1, x + 1), G(y, x - 1), G(y, x + 1), G(y + 1, x - 1), G(y + 1, x), G(y + 1, x + 1), dx, dy);
      const size_t i = (size_t)y * w + x;
      gx[i] = (short)dx;
      gy[i] = (short)dy;
      mag[i] = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
    }
  std::vector<int> stack;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const size_t i = (size_t)y * w + x;
      const int m = mag[i];
      const bool cand = canny_candidate(gx[i], gy[i], m, M(y, x - 1), M(y, x + 1), M(y - 1, x), M(y + 1, x), M(y - 1, x - 1), M(y - 1, x + 1), M(y + 1, x - 1),
                                        M(y + 1, x + 1), low);
      cls[i] = cand ? (m > high ? 2 : 1) : 0;
      edge[i] = 0;
      if (cls[i] == 2) stack.push_back((int)i);
    }
  for (int i : stack) edge[i] = 255;
  while (!stack.empty()) {  // every pixel enters the stack at most once (it is marked when pushed)
    const int i = stack.back(), y = i / w, x = i - y * w;
    stack.pop_back();
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int yy = y + dy, xx = x + dx;
        if ((unsigned)yy >= (unsigned)h || (unsigned)xx >= (unsigned)w) continue;
        const int j = yy * w + xx;
        if (cls[j] && !edge[j]) {
          edge[j] = 255;
          stack.push_back(j);
        }
      }
  }
  return true;
}
