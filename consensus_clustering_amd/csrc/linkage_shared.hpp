// What the linkage kernels share (predict.hip: the consensus labels' one-workgroup and grid forms;
// hclust.hip: the batched trees of the hierarchical base clusterer): the Lance-Williams update in
// scipy's float64 arithmetic, the live-cluster bitmask, and the first-minimum row scan with its
// block reduction.  One definition, so that the trees of both users take the same decisions.
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

// Block minimum of (v, i) over T threads: the lower value, ties to the lower index.
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

// First minimum over live i != x of row[i]: thread tid visits i = base + tid + T u in increasing
// order, NB loads in flight per batch.  No live neighbour: (+inf, 0x7fffffff).
template <int T, int NB>
__device__ __forceinline__ void row_argmin(const double* row, int n, int x, const unsigned* mask, double& v,
                                           int& bi) {
  constexpr double INF = __builtin_huge_val();
  const int tid = threadIdx.x;
  v = INF;
  bi = 0x7fffffff;
  for (int base = 0; base < n; base += T * NB) {
    double d[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int i = base + tid + T * u;
      d[u] = i < n ? row[i] : INF;
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int i = base + tid + T * u;
      const bool ok = i < n && i != x && live(mask, i);
      if (ok && d[u] < v) {
        v = d[u];
        bi = i;
      }
    }
  }
}

}  // namespace cc_link
