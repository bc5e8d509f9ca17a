// Union-find for connected-component labelling (csrc/schools.hip), host and device.
//
// The forest lives in an int array L: L[x] is the parent of x, L[x] == x a root, and every link points DOWN
// (L[x] <= x), so the root of a tree is its smallest index -- the component's first pixel in raster order.  Links only
// ever decrease (fetch_min), hence a value read late or stale is still an ancestor of x in x's own component: `find` and
// `unite` stay correct under any interleaving; only the return value of fetch_min decides who linked a root.
//
// `Mem` gives the three accesses, so that the same loops run on LDS, on global memory and in a plain host array
// (tools/exp/ccl_host_check.cpp drives them serially):
//   int load(int i)                  the parent of i (relaxed);
//   int fetch_min(int i, int v)      L[i] = min(L[i], v), returns the value before;
//   void fail()                      raise the error flag of the launch.
//
// EVERY loop is bounded: a chain of links that strictly decrease cannot be longer than the `bound` = number of elements of
// the array, and a `unite` retries only after its root moved down.  A loop that exceeds the bound has met a corrupt array
// (a cycle): it raises the flag and returns, it never spins.
#ifndef CRIMAC_CCL_H_
#define CRIMAC_CCL_H_

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CCL_HD __host__ __device__ inline
#else
#define CCL_HD inline
#endif

// The root of x, after at most `bound` links; on a longer chain: fail(), and the node reached so far.
template <class Mem>
CCL_HD int ccl_find(Mem& m, int x, long bound) {
  for (long it = 0; it <= bound; ++it) {
    const int p = m.load(x);
    if (p == x) return x;
    x = p;
  }
  m.fail();
  return x;
}

// Join the trees of a and b under the smaller root.  At most `bound` rounds (each one moves a root strictly down).
template <class Mem>
CCL_HD void ccl_unite(Mem& m, int a, int b, long bound) {
  for (long it = 0; it <= bound; ++it) {
    a = ccl_find(m, a, bound);
    b = ccl_find(m, b, bound);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = m.fetch_min(b, a);            // b was a root when we looked; link it unless somebody else has
    if (old == b) return;
    b = old;                                      // somebody linked b below: go on from there (old < b)
  }
  m.fail();
}

// ---- the tile geometry of the labelling, shared by the kernels and the host emulation -------------------------------
#define CCL_TILE_W 64          // pings of a tile (the contiguous axis)
#define CCL_TILE_H 16          // rows of a tile

// The neighbours a pixel joins INSIDE its tile (all of them precede it in raster order): left, up, and with
// 8-connectivity up-left and up-right.  visit(dr, dp) is called for each.
template <class F>
CCL_HD void ccl_back_neighbours(int connectivity, F&& visit) {
  visit(0, -1);
  visit(-1, 0);
  if (connectivity == 8) {
    visit(-1, -1);
    visit(-1, 1);
  }
}

// The neighbours of pixel (r, p) that lie in ANOTHER tile and that it is in charge of joining, so that every adjacent pair
// of pixels cut by a tile border is joined by exactly the pixel on the border's lower / right side (or, for an
// anti-diagonal pair cut by a vertical border only, by its upper right pixel, through `down-left`):
//   first row of a tile (r % H == 0): up, and with 8-connectivity up-left, up-right;
//   first column of a tile (p % W == 0): left, and with 8-connectivity up-left, down-left.
template <class F>
CCL_HD void ccl_border_neighbours(int r, int p, int connectivity, F&& visit) {
  const bool top = r % CCL_TILE_H == 0, left = p % CCL_TILE_W == 0;
  if (top) {
    visit(-1, 0);
    if (connectivity == 8) {
      visit(-1, -1);
      visit(-1, 1);
    }
  }
  if (left) {
    visit(0, -1);
    if (connectivity == 8) {
      if (!top) visit(-1, -1);
      visit(1, -1);
    }
  }
}

#endif  // CRIMAC_CCL_H_
