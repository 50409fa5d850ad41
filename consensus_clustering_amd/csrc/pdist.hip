// The distances of the hierarchical base clusterer: AgglomerativeClustering(metric = euclidean |
// manhattan | cosine | correlation) hands its rows to scipy.cluster.hierarchy.linkage(X, method,
// metric), whose distances are pdist(X, metric).  Three entry points restate pdist as full
// symmetric float64 matrices with an exact-zero diagonal (squareform's), bit for bit, over one
// tile kernel:
//   cc_euclidean      D [n][n] of the rows X, metric euclidean (a pair's value does not depend on
//                     the resample, so a fit computes it once and cc_hc_gather copies entries)
//   cc_pdist          the same for cityblock and cosine (euclidean goes to cc_euclidean)
//   cc_pdist_batched  feature subsampling: every resample b draws its own columns cols[b] as well
//                     as its own rows idx[b], so a pair's distance depends on the resample:
//                     Db[b] = squareform(pdist(X[idx[b]][:, cols[b]], metric)) for a batch
// The arithmetic, as scipy's distance_impl.h has it, with no FMA:
//   euclidean  one accumulator, acc += (u_k - v_k)^2 in increasing k; sqrt
//   cityblock  one accumulator, acc += fabs(u_k - v_k) in increasing k
//   cosine     scipy's dot product is two accumulators: a0 takes the products of even k, a1 those
//              of odd k, over k < (d & ~1), each in increasing k; then t = a0 + a1, and an odd d
//              adds u_{d-1} v_{d-1} to t last.  The row norms are sqrt(t(u, u)) (row_norm).
//              c = t / (norm_i norm_j), clipped to [-1, 1] by magnitude; the distance is 1 - c
//   correlation  is cosine on the rows less their means.  cc_pdist's caller centres them (scipy
//              does it with numpy on the float64 copy of X) and asks for cosine; cc_pdist_batched
//              centres them itself, in its row pass
// The kernels:
//   norm_kernel  cc_pdist's norms [n] of the rows X
//   rows_kernel  cc_pdist_batched's row pass, one thread per (b, r): the md values of row idx[b][r]
//                at cols[b], as float64, into the compact row Xb[b][r][0..md) of the workspace
//                (scipy's C-contiguous float64 copy).  Correlation then subtracts numpy's mean of
//                the compact row (scipy's X - X.mean(axis=1, keepdims=True)); cosine and
//                correlation write the row's norm
//   tile_kernel  the distances of tree blockIdx.y (one tree, the rows X themselves, for
//                cc_euclidean and cc_pdist; Xb + b m md, norms + b m and Db + b m m for
//                cc_pdist_batched)
//
// numpy's mean of a float64 row a[0..n) is s / n.  The reduction starts from s = 0.0 and hands the
// row to the add loop in pieces of numpy's buffer size (8192 elements, np.getbufsize()'s default):
// s += pw(piece) for each, where pw is the pairwise sum (numpy/_core/src/umath/loops_utils.h.src):
//   n < 8          0.0, then the elements added left to right
//   8 <= n <= 128  eight accumulators r[j] = a[j]; r[j] += a[i + j] for i = 8, 16, ... below
//                  n - n % 8; ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); then the
//                  remaining elements added one by one
//   n > 128        n2 = n / 2 - (n / 2) % 8; pw(a, n2) + pw(a + n2, n - n2)
// The recursion is walked without a call stack: a node is the path from the root (one bit a
// level), its (offset, length) is recomputed from the path, and the left sums that wait for their
// right siblings sit in LDS (one slot a level and thread), so the kernel uses no scratch.
//
// No workgroup talks to another, and nothing is atomic.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "ccmi_internal.h"
#include "launch_error.hpp"

#pragma clang fp contract(off)  // every product and sum of this file is rounded separately

namespace {

constexpr int PT = 64;  // tile edge
constexpr int PK = 16;  // k slab (even: the parity of k inside a slab is its global parity)
constexpr int PR = 4;   // outputs per thread and side
static_assert(PK % 2 == 0, "the cosine accumulators pair k by parity inside a slab");

constexpr int ROW_T = 64;        // rows (threads) per workgroup of the row pass
constexpr int PW_BLOCK = 128;    // numpy's PW_BLOCKSIZE
constexpr int NP_BUFSIZE = 8192;  // numpy's default buffer size: the longest piece one pw() sees
// a node of length L > 128 has children of at most L / 2 + 8, so a piece of 8192 is at most 7
// levels deep; one bit of `path` and one LDS slot a level
constexpr int PW_DEPTH = 8;

// scipy's sqrt(dot(u, u)) of a row u[0..d)
template <typename T>
__device__ __forceinline__ double row_norm(const T* u, int d) {
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
  return __dsqrt_rn(t);
}

template <typename T>
__global__ __launch_bounds__(256) void norm_kernel(const T* __restrict__ X, int n, int d,
                                                   double* __restrict__ norms) {
  const int i = static_cast<int>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  norms[i] = row_norm(X + static_cast<int64_t>(i) * d, d);
}

// numpy's pairwise sum of a block of n <= 128 elements
__device__ __forceinline__ double pw_block(const double* a, int n) {
  if (n < 8) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += a[i];
    return s;
  }
  double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 += a[i + 0];
    r1 += a[i + 1];
    r2 += a[i + 2];
    r3 += a[i + 3];
    r4 += a[i + 4];
    r5 += a[i + 5];
    r6 += a[i + 6];
    r7 += a[i + 7];
  }
  double s = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) s += a[i];
  return s;
}

// numpy's pairwise sum of a[0..n): a post-order walk of the recursion.  `path` holds the turns
// from the root to the current node (bit l set: the right child at level l); wait[l][lane] holds
// the sum of the left child at level l while its right sibling is summed.
__device__ __forceinline__ double pw_sum(const double* a, int n, double (*wait)[ROW_T], int lane) {
  uint32_t path = 0;
  int depth = 0, off = 0, len = n;
  for (;;) {
    while (len > PW_BLOCK && depth < PW_DEPTH) {  // leftmost leaf below the current node
      int n2 = len / 2;
      n2 -= n2 % 8;
      len = n2;
      ++depth;
    }
    double v = pw_block(a + off, len);
    while (depth > 0 && ((path >> (depth - 1)) & 1u)) {  // a right child: left + right, one level up
      --depth;
      path &= ~(1u << depth);
      v = wait[depth][lane] + v;
    }
    if (depth == 0) return v;
    wait[depth - 1][lane] = v;  // a left child: park it and go to the right sibling
    path |= 1u << (depth - 1);
    off = 0;
    len = n;
    for (int l = 0; l < depth; ++l) {
      int n2 = len / 2;
      n2 -= n2 % 8;
      if ((path >> l) & 1u) {
        off += n2;
        len -= n2;
      } else {
        len = n2;
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(ROW_T) void rows_kernel(const T* __restrict__ X, int d,
                                                     const int* __restrict__ idx,
                                                     const int* __restrict__ cols, int m, int md,
                                                     int metric, double* Xb, double* __restrict__ norms) {
  __shared__ double wait[PW_DEPTH][ROW_T];
  const int b = static_cast<int>(blockIdx.y);
  const int r = static_cast<int>(blockIdx.x) * ROW_T + threadIdx.x;
  if (r >= m) return;  // no barrier below
  const size_t br = static_cast<size_t>(b) * m + r;
  const int* cb = cols + static_cast<size_t>(b) * md;
  const T* u = X + static_cast<int64_t>(idx[br]) * d;
  double* row = Xb + br * md;
  for (int k = 0; k < md; ++k) row[k] = static_cast<double>(u[cb[k]]);
  if (metric == CC_METRIC_CORRELATION) {
    double s = 0.0;
    for (int o = 0; o < md; o += NP_BUFSIZE) s += pw_sum(row + o, min(NP_BUFSIZE, md - o), wait, threadIdx.x);
    const double mean = s / static_cast<double>(md);
    for (int k = 0; k < md; ++k) row[k] = row[k] - mean;
  }
  if (metric == CC_METRIC_COSINE || metric == CC_METRIC_CORRELATION) norms[br] = row_norm(row, md);
}

// One 64 x 64 tile of the upper triangle (mirrored) of tree blockIdx.y over its rows [n][d]:
// 256 threads as 16 x 16, each thread 4 x 4 outputs; k slabs of 16 of both row blocks staged in
// LDS as float64 ([k][row]: a thread reads its 4 rows and 4 columns with two 16-B pairs each).
// METRIC is CC_METRIC_EUCLIDEAN, _CITYBLOCK or _COSINE.
// Cosine: two 4 x 4 accumulator sets (32 float64 a thread); the odd last column stays out of the
// slab loop and is read, after a0 + a1, from the last slab, which is still in LDS.
template <typename T, int METRIC>
__global__ __launch_bounds__(256) void tile_kernel(const T* __restrict__ Xall, int n, int d,
                                                   const double* __restrict__ norms_all,
                                                   double* __restrict__ Dall) {
  constexpr bool COSINE = METRIC == CC_METRIC_COSINE;
  const size_t tree = blockIdx.y;
  const T* __restrict__ X = Xall + tree * n * d;
  const double* __restrict__ norms = norms_all + tree * n;
  double* __restrict__ D = Dall + tree * n * n;
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
          for (int c = 0; c < PR; ++c) {
            if constexpr (METRIC == CC_METRIC_EUCLIDEAN) {
              const double df = a[r] - b[c];
              acc[r][c] += df * df;
            } else {
              acc[r][c] += __builtin_fabs(a[r] - b[c]);
            }
          }
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
        if constexpr (METRIC == CC_METRIC_EUCLIDEAN) v = __dsqrt_rn(v);
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

// the upper-triangle tiles of an n x n matrix, a grid's x extent; `what` names the entry point
// and `dim` its argument n
int tile_count(const char* what, const char* dim, int n, unsigned* tiles) {
  const int64_t nb = (n + PT - 1) / PT;
  const int64_t t = nb * (nb + 1) / 2;
  if (t > 0x7fffffff) {
    cc::set_error(std::string(what) + ": " + dim + " too large");
    return CC_ERR_ARG;
  }
  *tiles = static_cast<unsigned>(t);
  return CC_OK;
}

// the tile pass of `trees` trees of n rows each; correlation's rows are centred by now
template <typename T>
void launch_tiles(const T* X, int n, int d, int metric, const double* norms, double* D, unsigned tiles,
                  int trees, hipStream_t st) {
  const dim3 grid(tiles, trees);
  if (metric == CC_METRIC_EUCLIDEAN)
    hipLaunchKernelGGL((tile_kernel<T, CC_METRIC_EUCLIDEAN>), grid, dim3(256), 0, st, X, n, d, norms, D);
  else if (metric == CC_METRIC_CITYBLOCK)
    hipLaunchKernelGGL((tile_kernel<T, CC_METRIC_CITYBLOCK>), grid, dim3(256), 0, st, X, n, d, norms, D);
  else
    hipLaunchKernelGGL((tile_kernel<T, CC_METRIC_COSINE>), grid, dim3(256), 0, st, X, n, d, norms, D);
}

// cc_euclidean and cc_pdist: one tree over the rows X themselves
template <typename T>
int launch(const char* what, const T* X, int n, int d, int metric, double* D, double* norms, unsigned tiles,
           hipStream_t st) {
  if (metric == CC_METRIC_COSINE)
    hipLaunchKernelGGL(norm_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, st, X, n, d, norms);
  launch_tiles(X, n, d, metric, norms, D, tiles, 1, st);
  return launch_error(what);
}

bool known_metric(int metric) {
  return metric == CC_METRIC_EUCLIDEAN || metric == CC_METRIC_CITYBLOCK || metric == CC_METRIC_COSINE ||
         metric == CC_METRIC_CORRELATION;
}

}  // namespace

extern "C" int cc_euclidean(const void* X, int is_f64, int n, int d, double* D, void* stream) {
  if (!X || !D || n <= 0 || d <= 0) {
    cc::set_error("cc_euclidean: bad arguments");
    return CC_ERR_ARG;
  }
  unsigned tiles;
  if (const int rc = tile_count("cc_euclidean", "n", n, &tiles)) return rc;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (is_f64)
    return launch("cc_euclidean", static_cast<const double*>(X), n, d, CC_METRIC_EUCLIDEAN, D, nullptr, tiles, st);
  return launch("cc_euclidean", static_cast<const float*>(X), n, d, CC_METRIC_EUCLIDEAN, D, nullptr, tiles, st);
}

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
  unsigned tiles;
  if (const int rc = tile_count("cc_pdist", "n", n, &tiles)) return rc;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (is_f64) return launch("cc_pdist", static_cast<const double*>(X), n, d, metric, D, norms, tiles, st);
  return launch("cc_pdist", static_cast<const float*>(X), n, d, metric, D, norms, tiles, st);
}

extern "C" size_t cc_pdist_batched_workspace_bytes(int B, int m, int md, int metric) {
  if (B <= 0 || m <= 0 || md <= 0 || !known_metric(metric)) return 0;
  // the compact rows [B][m][md], then the norms [B][m] (read by cosine and correlation alone)
  return sizeof(double) * (static_cast<size_t>(B) * m * md + static_cast<size_t>(B) * m);
}

extern "C" int cc_pdist_batched(const void* X, int is_f64, int n, int d, const int* idx, const int* cols, int B,
                                int m, int md, int metric, double* Db, void* workspace, size_t ws_bytes,
                                void* stream) {
  if (!known_metric(metric)) {
    cc::set_error("cc_pdist_batched: unknown metric " + std::to_string(metric));
    return CC_ERR_ARG;
  }
  if (!X || !idx || !cols || !Db || !workspace || n <= 0 || d <= 0 || B <= 0 || m <= 0 || md <= 0 || md > d ||
      m > n || B > 65535) {
    cc::set_error("cc_pdist_batched: bad arguments (null pointer, a size below 1, md > d, m > n or B > 65535)");
    return CC_ERR_ARG;
  }
  const size_t need = cc_pdist_batched_workspace_bytes(B, m, md, metric);
  if (ws_bytes < need) {
    cc::set_error("cc_pdist_batched: workspace of " + std::to_string(ws_bytes) + " bytes, " +
                  std::to_string(need) + " needed");
    return CC_ERR_ARG;
  }
  unsigned tiles;
  if (const int rc = tile_count("cc_pdist_batched", "m", m, &tiles)) return rc;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  double* Xb = static_cast<double*>(workspace);
  double* norms = Xb + static_cast<size_t>(B) * m * md;
  const dim3 rgrid((m + ROW_T - 1) / ROW_T, B);
  if (is_f64)
    hipLaunchKernelGGL(rows_kernel<double>, rgrid, dim3(ROW_T), 0, st, static_cast<const double*>(X), d, idx,
                       cols, m, md, metric, Xb, norms);
  else
    hipLaunchKernelGGL(rows_kernel<float>, rgrid, dim3(ROW_T), 0, st, static_cast<const float*>(X), d, idx, cols,
                       m, md, metric, Xb, norms);
  launch_tiles(Xb, m, md, metric, norms, Db, tiles, B, st);
  return launch_error("cc_pdist_batched");
}
