// Host check of csrc/ccl.h: the union-find loops of csrc/schools.hip, driven serially on the CPU.
//
// Emulates the three steps of crimac_schools_label -- tiles labelled on their own, tile borders merged, flatten -- with the
// SAME find / unite / neighbour rules (ccl.h), on the shapes and patterns of tests/test_gpu_schools.py, and compares the
// result with a flood fill.  It also checks what no GPU test may provoke: on a corrupt parent array (a cycle) find and
// unite stop at their bound and raise the flag.  Build with the sanitizers and run on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I crimac_classifiers_unet_amd/csrc \
//       tools/exp/ccl_host_check.cpp -o /tmp/ccl_host_check && /tmp/ccl_host_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "ccl.h"

namespace {

struct HostMem {
  int* L;
  int* err;
  long n;
  int load(int i) {
    if (i < 0 || i >= n) { std::fprintf(stderr, "load out of bounds: %d of %ld\n", i, n); std::abort(); }
    return L[i];
  }
  int fetch_min(int i, int v) {
    if (i < 0 || i >= n) { std::fprintf(stderr, "fetch_min out of bounds: %d of %ld\n", i, n); std::abort(); }
    const int old = L[i];
    if (v < old) L[i] = v;
    return old;
  }
  void fail() { *err = 1; }
};

using Mask = std::vector<uint8_t>;

// the kernels' steps, serially; `reverse` walks tiles, border pixels and the flatten backwards (the GPU runs them in any order)
std::vector<int> label_like_the_kernels(const Mask& fg, int R, int P, int conn, bool reverse, int& err) {
  const int W = CCL_TILE_W, H = CCL_TILE_H, tp = (P + W - 1) / W, tr = (R + H - 1) / H;
  std::vector<int> labels((size_t)R * P, -7);
  err = 0;
  for (int tile = 0; tile < tp * tr; ++tile) {                       // label_tiles_kernel
    const int r0 = (tile / tp) * H, p0 = (tile % tp) * W;
    std::vector<int> lab(W * H);
    for (int i = 0; i < W * H; ++i) {
      const int r = r0 + i / W, p = p0 + i % W;
      lab[i] = (r < R && p < P && fg[(size_t)r * P + p]) ? i : -1;
    }
    HostMem m{lab.data(), &err, W * H};
    for (int k = 0; k < W * H; ++k) {
      const int i = reverse ? W * H - 1 - k : k, lr = i / W, lp = i % W;
      if (m.load(i) < 0) continue;
      ccl_back_neighbours(conn, [&](int dr, int dp) {
        const int nr = lr + dr, np = lp + dp;
        if (nr < 0 || np < 0 || np >= W) return;
        const int j = nr * W + np;
        if (m.load(j) >= 0) ccl_unite(m, i, j, W * H);
      });
    }
    for (int i = 0; i < W * H; ++i) {
      const int r = r0 + i / W, p = p0 + i % W;
      if (r >= R || p >= P) continue;
      const int root = lab[i] < 0 ? -1 : ccl_find(m, i, W * H);
      labels[(size_t)r * P + p] = root < 0 ? -1 : (r0 + root / W) * P + p0 + root % W;
    }
  }
  const long n = (long)R * P;
  HostMem g{labels.data(), &err, n};
  for (int k = 0; k < tp * tr; ++k) {                                // merge_borders_kernel
    const int tile = reverse ? tp * tr - 1 - k : k;
    const int r0 = (tile / tp) * H, p0 = (tile % tp) * W;
    for (int t = 0; t < W + H; ++t) {
      const int r = t < W ? r0 : r0 + (t - W), p = t < W ? p0 + t : p0;
      if (r >= R || p >= P || t == W) continue;
      const int i = r * P + p;
      if (g.load(i) < 0) continue;
      ccl_border_neighbours(r, p, conn, [&](int dr, int dp) {
        const int nr = r + dr, np = p + dp;
        if (nr < 0 || nr >= R || np < 0 || np >= P) return;
        const int j = nr * P + np;
        if (g.load(j) >= 0) ccl_unite(g, i, j, n);
      });
    }
  }
  for (long k = 0; k < n; ++k) {                                     // flatten_kernel
    const long i = reverse ? n - 1 - k : k;
    if (labels[i] < 0) continue;
    labels[i] = ccl_find(g, (int)i, n);
  }
  return labels;
}

std::vector<int> flood_fill(const Mask& fg, int R, int P, int conn) {
  std::vector<int> labels((size_t)R * P, -1);
  std::vector<int> stack;
  for (int a = 0; a < R * P; ++a) {
    if (!fg[a] || labels[a] >= 0) continue;
    labels[a] = a;
    stack.push_back(a);
    while (!stack.empty()) {
      const int i = stack.back(), r = i / P, p = i % P;
      stack.pop_back();
      for (int dr = -1; dr <= 1; ++dr)
        for (int dp = -1; dp <= 1; ++dp) {
          if ((!dr && !dp) || (conn == 4 && dr && dp)) continue;
          const int nr = r + dr, np = p + dp;
          if (nr < 0 || nr >= R || np < 0 || np >= P) continue;
          const int j = nr * P + np;
          if (fg[j] && labels[j] < 0) labels[j] = a, stack.push_back(j);
        }
    }
  }
  return labels;
}

// the patterns of tests/test_gpu_schools.py
Mask pattern(const std::string& name, int R, int P) {
  Mask m((size_t)R * P, 0);
  auto at = [&](int r, int p) -> uint8_t& { return m[(size_t)r * P + p]; };
  if (name == "full") m.assign(m.size(), 1);
  if (name == "checker")
    for (int r = 0; r < R; ++r) for (int p = 0; p < P; ++p) at(r, p) = (r + p) % 2 == 0;
  if (name == "serpentine")                                          // even rows full, odd rows one pixel at alternating ends
    for (int r = 0; r < R; ++r) {
      if (r % 2 == 0) for (int p = 0; p < P; ++p) at(r, p) = 1;
      else at(r, (r / 2) % 2 == 0 ? P - 1 : 0) = 1;
    }
  if (name == "spiral") {                                            // a one-pixel path that winds inwards, one gap wide
    auto set = [&](int r, int p) { return r >= 0 && r < R && p >= 0 && p < P && at(r, p); };
    auto open = [&](int r, int p, int dr, int dp) {                  // may the path step from (r, p) to (r + dr, p + dp)?
      const int nr = r + dr, np = p + dp;
      return nr >= 0 && nr < R && np >= 0 && np < P && !at(nr, np) && !set(nr + dr, np + dp);
    };
    int r = 0, p = 0, dr = 0, dp = 1;
    for (long step = 0; step < (long)R * P; ++step) {
      at(r, p) = 1;
      if (!open(r, p, dr, dp)) {
        const int t = dr;
        dr = dp, dp = -t;                                            // turn right
        if (!open(r, p, dr, dp)) break;
      }
      r += dr, p += dp;
    }
  }
  if (name == "combs")                                               // a spine every 24 rows, teeth every third ping, 20 rows long
    for (int r = 0; r < R; ++r) for (int p = 0; p < P; ++p) at(r, p) = (r % 24 == 0) || (p % 3 == 0 && r % 24 <= 20);
  if (name == "random30" || name == "random60") {
    uint64_t s = 0x9e3779b97f4a7c15ull ^ (uint64_t)(R * 131071 + P);
    const unsigned cut = name == "random30" ? 30 : 60;
    for (auto& v : m) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      v = (unsigned)((s >> 33) % 100) < cut;
    }
  }
  return m;
}

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) { std::fprintf(stderr, "FAILED: %s\n", what); ++failures; }
}

}  // namespace

int main() {
  const int shapes[][2] = {{1, 1}, {1, 130}, {67, 1}, {37, 70}, {64, 256}, {129, 257}};
  const char* names[] = {"empty", "full", "checker", "serpentine", "spiral", "combs", "random30", "random60"};
  long cases = 0;
  for (auto& sh : shapes)
    for (const char* name : names)
      for (int conn : {4, 8})
        for (bool reverse : {false, true}) {
          const int R = sh[0], P = sh[1];
          const Mask fg = pattern(name, R, P);
          int err = 0;
          const std::vector<int> got = label_like_the_kernels(fg, R, P, conn, reverse, err);
          const std::vector<int> want = flood_fill(fg, R, P, conn);
          if (err || got != want) {
            std::fprintf(stderr, "FAILED: %s %dx%d connectivity %d reverse %d (err %d)\n", name, R, P, conn, (int)reverse, err);
            ++failures;
          }
          ++cases;
        }
  // the iteration bounds, on arrays no labelling produces: a 2-cycle, a long cycle; find and unite must return and flag
  {
    std::vector<int> L = {0, 2, 1, 3};
    int err = 0;
    HostMem m{L.data(), &err, 4};
    ccl_find(m, 1, 4);
    expect(err == 1, "find on a 2-cycle raises the flag");
    err = 0;
    ccl_unite(m, 3, 1, 4);
    expect(err == 1, "unite into a cycle raises the flag");
    const int n = 1000;
    std::vector<int> ring(n);
    for (int i = 0; i < n; ++i) ring[i] = (i + 1) % n;
    err = 0;
    HostMem r{ring.data(), &err, n};
    ccl_find(r, 5, n);
    expect(err == 1, "find on a ring raises the flag");
    // the longest legal chain: n - 1 links, no flag
    for (int i = 0; i < n; ++i) ring[i] = i ? i - 1 : 0;
    err = 0;
    expect(ccl_find(r, n - 1, n) == 0 && err == 0, "a chain of n - 1 links is walked to its root without the flag");
  }
  std::printf("ccl_host_check: %ld labelling cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
