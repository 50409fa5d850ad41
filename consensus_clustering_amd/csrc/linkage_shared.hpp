// The tree builders of the device linkage, each written once: scipy's nn_chain loop and sklearn's
// Prim loop (mst_linkage_core), with the Lance-Williams update in scipy's float64 arithmetic, the
// live-cluster bitmask and the first-minimum row scan with its block reduction.  predict.hip (the
// consensus labels: one workgroup, or G workgroups over index slices) and hclust.hip (the batched
// trees of the hierarchical base clusterer, one workgroup per tree) only say how a workgroup takes
// part, through a scope; every decision of a tree is taken here, so all forms take the same ones.
//
// A scope S has
//   S::T, S::NB      threads of the workgroup; loads per thread in flight per row pass
//   j0, j1           the index slice [j0, j1) its row passes cover
//   tree_argmin      turns the block's (minimum, first index) into the tree's; false: leave at once
//   after_update     orders a Lance-Williams pass before any later scan; false: leave at once
//   writes_out       whether this workgroup writes the merges / edges
//   no_neighbour     reports a tree whose scan found no live finite neighbour
#pragma once

#include <hip/hip_runtime.h>

#include "ccmi_internal.h"

namespace cc_link {

// _hierarchy_distance_update.pxi in float64, every operation rounded separately (no FMA).
// dxi, dyi: the distances of cluster i to the merged x and y; dxy: the merge distance;
// nx, ny, ni: the three sizes (dxy and ni are read by Ward alone).
__device__ __forceinline__ double lw_update(int method, double dxi, double dyi, double dxy, int nx, int ny,
                                            int ni) {
#pragma clang fp contract(off)  // scipy's products and sum rounded separately (no FMA)
  if (method == CC_LINK_COMPLETE) return dxi > dyi ? dxi : dyi;  // fmax(d_xi, d_yi)
  if (method == CC_LINK_WEIGHTED) return 0.5 * (dxi + dyi);
  if (method == CC_LINK_WARD) {
    // t = 1 / (nx + ny + ni); sqrt((ni+nx) t dxi^2 + (ni+ny) t dyi^2 - ni t dxy^2), left to right,
    // on the euclidean (not squared) distances
    const double sx = static_cast<double>(nx), sy = static_cast<double>(ny), si = static_cast<double>(ni);
    const double t = 1.0 / (sx + sy + si);
    const double a = (si + sx) * t * dxi * dxi;
    const double b = (si + sy) * t * dyi * dyi;
    const double c = si * t * dxy * dxy;
    return __dsqrt_rn(a + b - c);
  }
  // average: (size_x * d_xi + size_y * d_yi) / (size_x + size_y)
  const double a = static_cast<double>(nx) * dxi;
  const double b = static_cast<double>(ny) * dyi;
  return (a + b) / static_cast<double>(nx + ny);
}

// Block minimum of (v, i) over T threads: the lower value, ties to the lower index.  The barrier
// before the rv / ri writes also ends every read of an earlier call, so calls may follow each
// other directly.
template <int T>
__device__ __forceinline__ void block_argmin(double& v, int& i, double* rv, int* ri) {
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    if (ov < v || (ov == v && oi < i)) {
      v = ov;
      i = oi;
    }
  }
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    rv[w] = v;
    ri[w] = i;
  }
  __syncthreads();
  v = rv[0];
  i = ri[0];
  for (int k = 1; k < T / 64; ++k)
    if (rv[k] < v || (rv[k] == v && ri[k] < i)) {
      v = rv[k];
      i = ri[k];
    }
}

__device__ __forceinline__ bool live(const unsigned* mask, int i) { return (mask[i >> 5] >> (i & 31)) & 1u; }

// First minimum over live i != x in [j0, j1) of row[i]: thread tid visits i = base + tid + T u in
// increasing order, NB loads in flight per batch.  No live neighbour: (+inf, 0x7fffffff).
template <int T, int NB>
__device__ __forceinline__ void row_argmin(const double* row, int j0, int j1, int x, const unsigned* mask,
                                           double& v, int& bi) {
  constexpr double INF = __builtin_huge_val();
  const int tid = threadIdx.x;
  v = INF;
  bi = 0x7fffffff;
  for (int base = j0; base < j1; base += T * NB) {
    double d[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int i = base + tid + T * u;
      d[u] = i < j1 ? row[i] : INF;
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int i = base + tid + T * u;
      const bool ok = i < j1 && i != x && live(mask, i);
      if (ok && d[u] < v) {
        v = d[u];
        bi = i;
      }
    }
  }
}

// The scope of a workgroup that builds its tree alone: the whole index range, the block's minimum
// is the tree's, a workgroup barrier after an update.  status receives `code` when the tree is
// abandoned (nn_chain only).
template <int T_, int NB_>
struct OneGroup {
  static constexpr int T = T_, NB = NB_;
  static constexpr int j0 = 0;
  int j1;
  int* status;
  int code;
  __device__ bool tree_argmin(double&, int&, double*, int*) { return true; }
  __device__ bool after_update() {
    __syncthreads();
    return true;
  }
  __device__ bool writes_out() const { return true; }
  __device__ void no_neighbour() {
    if (threadIdx.x == 0) *status = code;
  }
};

// scipy.cluster.hierarchy.nn_chain over the symmetric D [n][n] (overwritten): Z [n-1][4] receives
// (x, y, distance, size) per merge in merge order.  mask: [(n + 31) / 32] words in LDS; size,
// chain: [n] ints each, private to the workgroup.  The chain grows from the first live cluster; a
// step's nearest neighbour of the chain top x is the first index of the minimum over live i != x
// of D[x, i], taken only when strictly below D[x, previous] (the previous chain element wins
// ties); mutual neighbours merge, x < y, slot y keeps the union and x dies.  Every thread of every
// workgroup of the tree runs the same control flow: all values a branch depends on are reduced
// ones (or read from memory that a barrier has ordered), identical everywhere.
// Barriers: a write of thread 0 to chain[] / size[] / mask is followed by one before any thread
// reads it, and the reads of size[x], size[y] are followed by one before thread 0 overwrites them;
// chain[len] is read by nobody while thread 0 writes it.
template <typename S>
__device__ __forceinline__ void nn_chain(S& s, double* __restrict__ D, int n, int method, double* __restrict__ Z,
                                         unsigned* mask, int* size, int* chain) {
#pragma clang fp contract(off)  // the Lance-Williams pass: no FMA
  constexpr int T = S::T, NB = S::NB;
  constexpr double INF = __builtin_huge_val();
  __shared__ double rv[T / 64];
  __shared__ int ri[T / 64];
  const int tid = threadIdx.x;
  const size_t nn = static_cast<size_t>(n);
  const int nw = (n + 31) >> 5;
  for (int i = tid; i < n; i += T) size[i] = 1;
  for (int w = tid; w < nw; w += T) mask[w] = (w < nw - 1 || (n & 31) == 0) ? 0xFFFFFFFFu : ((1u << (n & 31)) - 1u);
  __syncthreads();
  int len = 0;  // uniform: every thread runs the same control flow
  for (int k = 0; k < n - 1; ++k) {
    if (len == 0) {  // the first live cluster
      double v = INF;
      int i0 = 0x7fffffff;
      for (int w = tid; w < nw; w += T)
        if (mask[w]) {
          i0 = 32 * w + __builtin_ctz(mask[w]);
          v = 0.0;
          break;
        }
      block_argmin<T>(v, i0, rv, ri);
      if (i0 < 0 || i0 >= n) {  // cannot happen while merges remain; never index with it
        s.no_neighbour();
        return;
      }
      if (tid == 0) chain[0] = i0;
      __syncthreads();
      len = 1;
    }
    int x, y;
    double cur;
    for (;;) {
      x = chain[len - 1];
      y = -1;
      cur = INF;
      if (len > 1) {
        y = chain[len - 2];
        cur = D[x * nn + y];
      }
      double v;
      int bi;
      row_argmin<T, NB>(D + x * nn, s.j0, s.j1, x, mask, v, bi);
      block_argmin<T>(v, bi, rv, ri);
      if (!s.tree_argmin(v, bi, rv, ri)) return;
      if (v < cur) {
        cur = v;
        y = bi;
      }
      // no neighbour: the scan's sentinel (or the -1 of a one-element chain) must never index
      // anything; the tree is reported and abandoned (v, bi and cur are the tree's: every thread
      // of every workgroup holds the same y and leaves here, none is left waiting at a barrier)
      if (y < 0 || y >= n) {
        s.no_neighbour();
        return;
      }
      if (len > 1 && y == chain[len - 2]) break;
      if (tid == 0) chain[len] = y;
      __syncthreads();
      ++len;
    }
    len -= 2;
    if (x > y) {
      const int t = x;
      x = y;
      y = t;
    }
    const int nx = size[x], ny = size[y];
    __syncthreads();  // every thread has read the sizes
    if (tid == 0) {
      if (s.writes_out()) {
        Z[4 * static_cast<size_t>(k) + 0] = x;
        Z[4 * static_cast<size_t>(k) + 1] = y;
        Z[4 * static_cast<size_t>(k) + 2] = cur;
        Z[4 * static_cast<size_t>(k) + 3] = nx + ny;
      }
      size[x] = 0;
      size[y] = nx + ny;
      mask[x >> 5] &= ~(1u << (x & 31));
    }
    __syncthreads();
    const double* rx = D + x * nn;
    double* ry = D + y * nn;
    for (int base = s.j0; base < s.j1; base += T * NB) {
      double dx[NB], dy[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int i = base + tid + T * u;
        dx[u] = i < s.j1 ? rx[i] : 0.0;
        dy[u] = i < s.j1 ? ry[i] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int i = base + tid + T * u;
        if (i < s.j1 && i != y && live(mask, i)) {
          const int ni = method == CC_LINK_WARD ? size[i] : 0;
          const double nd = lw_update(method, dx[u], dy[u], cur, nx, ny, ni);
          ry[i] = nd;
          D[i * nn + y] = nd;
        }
      }
    }
    if (!s.after_update()) return;  // the merged row and column before any later scan
  }
}

// sklearn mst_linkage_core (Prim) over the rows of the symmetric D: out [n-1][3] = (current node,
// new node, distance) per step.  cur: the running minimum distance of every node ([n] float64;
// entry j is only ever touched by the one thread whose passes visit j); tree: in_tree, one bit per
// node, [(n + 31) / 32] words in LDS.  From node 0, each step folds the current node's row into
// cur[] of every node not in the tree and takes the first node of the smallest.
template <typename S>
__device__ __forceinline__ void prim(S& s, const double* __restrict__ D, int n, double* __restrict__ out,
                                     double* __restrict__ cur, unsigned* tree) {
  constexpr int T = S::T, NB = S::NB;
  constexpr double INF = __builtin_huge_val();
  __shared__ double rv[T / 64];
  __shared__ int ri[T / 64];
  const int tid = threadIdx.x;
  const int nw = (n + 31) >> 5;
  for (int i = s.j0 + tid; i < s.j1; i += T) cur[i] = INF;
  for (int w = tid; w < nw; w += T) tree[w] = 0u;
  __syncthreads();
  int node = 0;
  for (int k = 0; k < n - 1; ++k) {
    // every thread is past the previous step's scan (block_argmin's barriers follow it)
    if (tid == 0) tree[node >> 5] |= 1u << (node & 31);
    __syncthreads();
    const double* row = D + static_cast<size_t>(node) * n;
    double v = INF;
    int bi = 0x7fffffff;
    for (int base = s.j0; base < s.j1; base += T * NB) {
      double l[NB], r[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int j = base + tid + T * u;
        l[u] = j < s.j1 ? row[j] : INF;
        r[u] = j < s.j1 ? cur[j] : INF;
      }
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int j = base + tid + T * u;
        if (j < s.j1 && !live(tree, j)) {
          double c = r[u];
          if (l[u] < c) {  // left_value < right_value
            c = l[u];
            cur[j] = c;
          }
          if (c < v) {  // current_distances[j] < new_distance: the first minimum
            v = c;
            bi = j;
          }
        }
      }
    }
    block_argmin<T>(v, bi, rv, ri);
    if (!s.tree_argmin(v, bi, rv, ri)) return;
    const int nxt = (v < INF) ? bi : 0;  // sklearn's new_node starts at 0
    if (tid == 0 && s.writes_out()) {
      out[3 * static_cast<size_t>(k) + 0] = node;
      out[3 * static_cast<size_t>(k) + 1] = nxt;
      out[3 * static_cast<size_t>(k) + 2] = v;
    }
    node = nxt;
  }
}

}  // namespace cc_link
