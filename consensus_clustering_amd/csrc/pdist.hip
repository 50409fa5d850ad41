// The distances of the hierarchical base clusterer for the metrics other than euclidean:
// AgglomerativeClustering(metric = manhattan | cosine | correlation) hands its rows to
// scipy.cluster.hierarchy.linkage(X, method, metric), whose distances are pdist(X, metric).
// cc_pdist restates pdist as the full symmetric float64 [n][n] matrix, bit for bit, in the shape
// of hclust.hip's euclid_kernel: only the accumulation and the epilogue differ.
//   cityblock  one accumulator, acc += fabs(u_k - v_k) in increasing k (scipy's distance_impl.h)
//   cosine     scipy's dot product is two accumulators: a0 takes the products of even k, a1 those
//              of odd k, over k < (d & ~1), each in increasing k; then t = a0 + a1, and an odd d
//              adds u_{d-1} v_{d-1} to t last.  The row norms are sqrt(t(u, u)) (norm_kernel).
//              c = t / (norm_i norm_j), clipped to [-1, 1] by magnitude; the distance is 1 - c
//   correlation  is cosine on the rows less their means; the caller centres them (scipy does it
//              with numpy on the float64 copy of X) and calls the cosine kernel
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "ccmi_internal.h"

#pragma clang fp contract(off)  // every product and sum of this file is rounded separately

namespace {

constexpr int PT = 64;  // tile edge
constexpr int PK = 16;  // k slab (even: the parity of k inside a slab is its global parity)
constexpr int PR = 4;   // outputs per thread and side
static_assert(PK % 2 == 0, "the cosine accumulators pair k by parity inside a slab");

// scipy's dot(u, u) of every row, then its square root: norms [n]
template <typename T>
__global__ __launch_bounds__(256) void norm_kernel(const T* __restrict__ X, int n, int d,
                                                   double* __restrict__ norms) {
  const int i = static_cast<int>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const T* u = X + static_cast<int64_t>(i) * d;
  const int de = d & ~1;
  double a0 = 0.0, a1 = 0.0;
  for (int k = 0; k < de; k += 2) {
    const double x0 = static_cast<double>(u[k]), x1 = static_cast<double>(u[k + 1]);
    a0 += x0 * x0;
    a1 += x1 * x1;
  }
  double t = a0 + a1;
  if (d & 1) {
    const double x = static_cast<double>(u[d - 1]);
    t += x * x;
  }
  norms[i] = __dsqrt_rn(t);
}

// 64 x 64 output tiles of the upper triangle (mirrored), 256 threads as 16 x 16, each thread
// 4 x 4 outputs; k slabs of 16 of both row blocks staged in LDS as float64 ([k][row]).
// COSINE: two 4 x 4 accumulator sets (32 float64 a thread); the odd last column stays out of the
// slab loop and is read, after a0 + a1, from the last slab, which is still in LDS.
template <typename T, bool COSINE>
__global__ __launch_bounds__(256) void pdist_kernel(const T* __restrict__ X, int n, int d,
                                                    const double* __restrict__ norms,
                                                    double* __restrict__ D) {
  const int nb = (n + PT - 1) / PT;
  int t = static_cast<int>(blockIdx.x), bi = 0;
  while (t >= nb - bi) {  // blockIdx.x enumerates the upper-triangle tiles row-major
    t -= nb - bi;
    ++bi;
  }
  const int bj = bi + t;
  __shared__ __attribute__((aligned(16))) double sa[PK][PT];
  __shared__ __attribute__((aligned(16))) double sb[PK][PT];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = bi * PT, j0 = bj * PT;
  double acc[PR][PR], acc1[COSINE ? PR : 1][COSINE ? PR : 1];
#pragma unroll
  for (int r = 0; r < PR; ++r)
#pragma unroll
    for (int c = 0; c < PR; ++c) {
      acc[r][c] = 0.0;
      if constexpr (COSINE) acc1[r][c] = 0.0;
    }
  // staging: thread tid loads 4 consecutive k of row tid >> 2, per side (rows past n and k past d
  // read as 0: they reach nothing that is stored, or are never summed)
  const int sr = tid >> 2, sk = 4 * (tid & 3);
  const int dsum = COSINE ? (d & ~1) : d;  // the columns the slab loop sums
  auto load_ab = [&](int k, double (&a)[PR], double (&b)[PR]) {
#pragma unroll
    for (int q = 0; q < PR; q += 2) {
      const double2 av = *reinterpret_cast<const double2*>(&sa[k][PR * ty + q]);
      const double2 bv = *reinterpret_cast<const double2*>(&sb[k][PR * tx + q]);
      a[q] = av.x;
      a[q + 1] = av.y;
      b[q] = bv.x;
      b[q + 1] = bv.y;
    }
  };
  int k0 = 0;
  for (; k0 < d; k0 += PK) {
    double ga[4], gb[4];
    const int gi = i0 + sr, gj = j0 + sr;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int gk = k0 + sk + q;
      ga[q] = (gi < n && gk < d) ? static_cast<double>(X[static_cast<int64_t>(gi) * d + gk]) : 0.0;
      gb[q] = (gj < n && gk < d) ? static_cast<double>(X[static_cast<int64_t>(gj) * d + gk]) : 0.0;
    }
    __syncthreads();  // the previous slab's reads are done
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      sa[sk + q][sr] = ga[q];
      sb[sk + q][sr] = gb[q];
    }
    __syncthreads();
    const int kn = min(PK, dsum - k0);  // <= 0 when the slab holds the odd last column alone
    if constexpr (COSINE) {
      for (int k = 0; k < kn; k += 2) {  // kn is even
        double a[PR], b[PR], a1[PR], b1[PR];
        load_ab(k, a, b);
        load_ab(k + 1, a1, b1);
#pragma unroll
        for (int r = 0; r < PR; ++r)
#pragma unroll
          for (int c = 0; c < PR; ++c) {
            acc[r][c] += a[r] * b[c];
            acc1[r][c] += a1[r] * b1[c];
          }
      }
    } else {
      for (int k = 0; k < kn; ++k) {
        double a[PR], b[PR];
        load_ab(k, a, b);
#pragma unroll
        for (int r = 0; r < PR; ++r)
#pragma unroll
          for (int c = 0; c < PR; ++c) acc[r][c] += __builtin_fabs(a[r] - b[c]);
      }
    }
  }
  double ni[PR] = {}, nj[PR] = {};
  if constexpr (COSINE) {
#pragma unroll
    for (int r = 0; r < PR; ++r)
#pragma unroll
      for (int c = 0; c < PR; ++c) acc[r][c] += acc1[r][c];
    if (d & 1) {  // column d - 1 lies in the last slab staged (k0 - PK <= d - 1 < k0)
      double a[PR], b[PR];
      load_ab((d - 1) - (k0 - PK), a, b);
#pragma unroll
      for (int r = 0; r < PR; ++r)
#pragma unroll
        for (int c = 0; c < PR; ++c) acc[r][c] += a[r] * b[c];
    }
#pragma unroll
    for (int q = 0; q < PR; ++q) {
      const int i = i0 + PR * ty + q, j = j0 + PR * tx + q;
      ni[q] = i < n ? norms[i] : 1.0;
      nj[q] = j < n ? norms[j] : 1.0;
    }
  }
#pragma unroll
  for (int r = 0; r < PR; ++r)
#pragma unroll
    for (int c = 0; c < PR; ++c) {
      const int i = i0 + PR * ty + r, j = j0 + PR * tx + c;
      // a diagonal tile holds both (i, j) and (j, i): each thread stores its own entry alone (the
      // sums and products are commutative term by term, so the two are equal); the others mirror
      if (i < n && j < n) {
        double v = acc[r][c];
        if constexpr (COSINE) {
          double cs = v / (ni[r] * nj[c]);
          if (__builtin_fabs(cs) > 1.0) cs = __builtin_copysign(1.0, cs);
          v = 1.0 - cs;
        }
        if (i == j) v = 0.0;  // squareform's diagonal
        D[static_cast<int64_t>(i) * n + j] = v;
        if (bi != bj) D[static_cast<int64_t>(j) * n + i] = v;
      }
    }
}

int launch_error(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    cc::set_error(std::string(what) + ": " + hipGetErrorString(e));
    return CC_ERR_HIP;
  }
  return CC_OK;
}

template <typename T>
int launch(const T* X, int n, int d, int metric, double* D, double* norms, unsigned tiles, hipStream_t st) {
  if (metric == CC_METRIC_COSINE) {
    hipLaunchKernelGGL((norm_kernel<T>), dim3((n + 255) / 256), dim3(256), 0, st, X, n, d, norms);
    hipLaunchKernelGGL((pdist_kernel<T, true>), dim3(tiles), dim3(256), 0, st, X, n, d, norms, D);
  } else {
    hipLaunchKernelGGL((pdist_kernel<T, false>), dim3(tiles), dim3(256), 0, st, X, n, d, nullptr, D);
  }
  return launch_error("cc_pdist");
}

}  // namespace

extern "C" int cc_pdist(const void* X, int is_f64, int n, int d, int metric, double* D, double* norms,
                        void* stream) {
  if (metric == CC_METRIC_EUCLIDEAN) return cc_euclidean(X, is_f64, n, d, D, stream);
  if (metric != CC_METRIC_CITYBLOCK && metric != CC_METRIC_COSINE) {
    cc::set_error("cc_pdist: unknown metric " + std::to_string(metric));
    return CC_ERR_ARG;
  }
  if (!X || !D || n <= 0 || d <= 0 || (metric == CC_METRIC_COSINE && !norms)) {
    cc::set_error("cc_pdist: bad arguments (the cosine metric needs norms [n])");
    return CC_ERR_ARG;
  }
  const int64_t nb = (n + PT - 1) / PT;
  const int64_t tiles = nb * (nb + 1) / 2;
  if (tiles > 0x7fffffff) {
    cc::set_error("cc_pdist: n too large");
    return CC_ERR_ARG;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (is_f64) return launch(static_cast<const double*>(X), n, d, metric, D, norms, static_cast<unsigned>(tiles), st);
  return launch(static_cast<const float*>(X), n, d, metric, D, norms, static_cast<unsigned>(tiles), st);
}
