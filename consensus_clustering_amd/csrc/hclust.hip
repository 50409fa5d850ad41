// Hierarchical base clusterer: AgglomerativeClustering(linkage = ward | average | complete,
// metric = euclidean) for every resample and every K of a fit (CC.py:282 with the clusterer of
// Monti's paper), on the device.
//
// sklearn hands such an estimator to scipy.cluster.hierarchy.linkage(X, method, 'euclidean') and
// cuts the tree with _hc_cut.  The distances pdist(X, metric) come from pdist.hip, as one full
// symmetric float64 [n][n] a fit or one [m][m] a resample; three kernels restate the rest:
//   gather_kernel   the distances of resample b: D_b[a][c] = Dfull[idx[b][a]][idx[b][c]]
//   nnchain_batched scipy's nn_chain, one workgroup per tree: the loop of linkage_shared.hpp that
//                   predict.hip runs too, here in its one-workgroup scope (workgroups never
//                   communicate)
//   cut_kernel      the K-cluster cut of every tree and K, straight from nn_chain's raw merges
//
// The cut needs no relabelled tree.  nn_chain's merge j joins slots (x_j, y_j), x_j < y_j: slot
// x_j dies and slot y_j keeps the union.  linkage() sorts the merges by distance (stable); the
// K-cluster cut undoes the last K - 1 merges of that order, i.e. keeps the merges of rank
// < m - K.  So slot x gets the link x -> y when the rank of its death merge is < m - K, else
// x -> x; every slot dies at most once, and the root of leaf i under these links names its
// cluster.  The roots are found by pointer jumping (ceil(log2 m) rounds of link[i] =
// link[link[i]]), and a root's id is the number of roots below it, so the ids are [0, K).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "ccmi_internal.h"
#include "launch_error.hpp"
#include "linkage_shared.hpp"

#pragma clang fp contract(off)  // every product and sum of this file is rounded separately

namespace {

__global__ __launch_bounds__(256) void gather_kernel(const double* __restrict__ Dfull, int n,
                                                     const int* __restrict__ idx, int m,
                                                     double* __restrict__ Db) {
  const int b = blockIdx.z, a = blockIdx.y;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= m) return;
  const int* id = idx + static_cast<size_t>(b) * m;
  const double* row = Dfull + static_cast<size_t>(id[a]) * n;
  Db[(static_cast<size_t>(b) * m + a) * m + c] = row[id[c]];
}

// ---- batched nn_chain.  One workgroup of T threads per tree; the live bitmask, the chain and
// the cluster sizes of a tree live in LDS when 8 m bytes fit (every chain step begins with a
// dependent read of the chain top), else in the workspace.
constexpr int NBH = 8;              // loads per thread in flight per row pass
constexpr int HC_T_SMALL = 256;     // threads per tree up to HC_M_SMALL leaves
constexpr int HC_T_LARGE = 1024;    // and above
constexpr int HC_M_SMALL = 1024;
constexpr size_t HC_LDS_STATE_MAX = 48 * 1024;  // chain + sizes in LDS up to this many bytes
constexpr size_t HC_HDR_ALIGN = 256;

// status words of a tree
constexpr int HC_OK = 0;
constexpr int HC_NO_NEIGHBOUR = 1;  // a scan found no live finite neighbour (non-finite distances)

template <int T>
__global__ __launch_bounds__(T) void nnchain_batched_kernel(double* __restrict__ Dall, int m, int method,
                                                            double* __restrict__ Zall, int* __restrict__ status,
                                                            int* __restrict__ state, int state_in_lds) {
  extern __shared__ unsigned hc_lds[];  // live mask [nw], then (state_in_lds) sizes [m], chain [m]
  const size_t b = blockIdx.x, mm = static_cast<size_t>(m);
  const int nw = (m + 31) >> 5;
  int* size = state_in_lds ? reinterpret_cast<int*>(hc_lds + nw) : state + b * 2 * mm;
  if (threadIdx.x == 0) status[b] = HC_OK;
  cc_link::OneGroup<T, NBH> scope{m, status + b, HC_NO_NEIGHBOUR};
  cc_link::nn_chain(scope, Dall + b * mm * mm, m, method, Zall + b * (mm - 1) * 4, hc_lds, size, size + m);
}

// ---- cut: one workgroup per (tree b, K index k).  link[] of the m slots in LDS when 4 m bytes
// fit, else in the workspace; rootmask (one bit per slot) in LDS.
constexpr int CT = 256;
constexpr size_t HC_LDS_LINK_MAX = 48 * 1024;

__global__ __launch_bounds__(CT) void cut_kernel(const double* __restrict__ Zall, const int* __restrict__ rank,
                                                 const int* __restrict__ idx, int m, const int* __restrict__ Ks,
                                                 int nK, int h_begin, uint8_t* __restrict__ labels, int64_t n,
                                                 int64_t ldl, int* __restrict__ links, int link_in_lds) {
  extern __shared__ unsigned cut_lds[];  // rootmask [nw], then (link_in_lds) link [m]
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x, mm = static_cast<size_t>(m);
  const int k = blockIdx.y;
  const int K = Ks[k];
  const int nw = (m + 31) >> 5;
  unsigned* rootmask = cut_lds;
  int* link = link_in_lds ? reinterpret_cast<int*>(cut_lds + nw) : links + (b * nK + k) * mm;
  const double* Z = Zall + b * (mm - 1) * 4;
  const int* rk = rank + b * (mm - 1);
  const int* id = idx + b * mm;
  for (int i = tid; i < m; i += CT) link[i] = i;
  for (int w = tid; w < nw; w += CT) rootmask[w] = 0u;
  __syncthreads();
  const int keep = m - K;  // merges of rank < keep stay merged
  for (int j = tid; j < m - 1; j += CT)
    if (rk[j] < keep) {
      const int x = static_cast<int>(Z[4 * static_cast<size_t>(j) + 0]);
      const int y = static_cast<int>(Z[4 * static_cast<size_t>(j) + 1]);
      if (x >= 0 && x < m && y >= 0 && y < m) link[x] = y;  // every slot dies at most once: no race
    }
  __syncthreads();
  for (int i = tid; i < m; i += CT)
    if (link[i] == i) atomicOr(&rootmask[i >> 5], 1u << (i & 31));
  // pointer jumping in place: whatever link[link[i]] returns is an ancestor of i at least twice
  // as far as link[i] was (or the root), so ceil(log2 m) rounds reach every root
  for (int span = 1; span < m; span <<= 1) {
    __syncthreads();
    for (int i = tid; i < m; i += CT) {
      const int a = link[i];
      const int g = link[a];
      if (g != a) link[i] = g;
    }
  }
  __syncthreads();
  uint8_t* out = labels + static_cast<size_t>(k) * n * ldl + (h_begin + static_cast<int64_t>(b));
  for (int i = tid; i < m; i += CT) {
    const int r = link[i];
    int c = __builtin_popcount(rootmask[r >> 5] & ((1u << (r & 31)) - 1u));
    for (int w = 0; w < (r >> 5); ++w) c += __builtin_popcount(rootmask[w]);
    const int item = id[i];
    if (item >= 0 && item < n) out[static_cast<int64_t>(item) * ldl] = static_cast<uint8_t>(c);
  }
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
size_t mask_words_bytes(int m) { return static_cast<size_t>((m + 31) >> 5) * sizeof(unsigned); }
bool state_in_lds(int m) { return mask_words_bytes(m) + 2 * static_cast<size_t>(m) * sizeof(int) <= HC_LDS_STATE_MAX; }
bool link_in_lds(int m) { return mask_words_bytes(m) + static_cast<size_t>(m) * sizeof(int) <= HC_LDS_LINK_MAX; }
// the live / root bitmask alone must fit the default dynamic LDS
constexpr size_t HC_MASK_LDS_MAX = 60 * 1024;

// workspace: status [B] ints (padded), then per tree the chain state [2 m] ints, then per tree
// and K the links [m] ints (each part present whether or not LDS takes its place: the size does
// not depend on the thresholds)
size_t hc_status_bytes(int B) { return align_up(static_cast<size_t>(B) * sizeof(int), HC_HDR_ALIGN); }
size_t hc_state_bytes(int m, int B) { return align_up(static_cast<size_t>(B) * 2 * m * sizeof(int), HC_HDR_ALIGN); }
size_t hc_links_bytes(int m, int B, int nK) {
  return static_cast<size_t>(B) * static_cast<size_t>(nK) * static_cast<size_t>(m) * sizeof(int);
}

}  // namespace

extern "C" int cc_hc_gather(const double* Dfull, int n, const int* idx, int B, int m, double* Db, void* stream) {
  if (!Dfull || !idx || !Db || n <= 0 || B <= 0 || m <= 0 || B > 65535 || m > 65535) {
    cc::set_error("cc_hc_gather: bad arguments (B and m at most 65535)");
    return CC_ERR_ARG;
  }
  hipLaunchKernelGGL(gather_kernel, dim3((m + 255) / 256, m, B), dim3(256), 0, static_cast<hipStream_t>(stream),
                     Dfull, n, idx, m, Db);
  return launch_error("cc_hc_gather");
}

extern "C" size_t cc_hc_workspace_bytes(int m, int B, int nK) {
  if (m <= 0 || B <= 0 || nK < 0) return 0;
  return hc_status_bytes(B) + hc_state_bytes(m, B) + hc_links_bytes(m, B, nK);
}

extern "C" int cc_hc_nnchain_batched(double* D, int B, int m, int method, double* Z, void* workspace,
                                     size_t ws_bytes, void* stream) {
  if (!D || !Z || B <= 0 || m < 2 || !workspace || ws_bytes < cc_hc_workspace_bytes(m, B, 0) ||
      (method != CC_LINK_AVERAGE && method != CC_LINK_COMPLETE && method != CC_LINK_WEIGHTED &&
       method != CC_LINK_WARD) ||
      mask_words_bytes(m) > HC_MASK_LDS_MAX) {
    cc::set_error("cc_hc_nnchain_batched: bad arguments");
    return CC_ERR_ARG;
  }
  int* status = static_cast<int*>(workspace);
  int* state = reinterpret_cast<int*>(static_cast<char*>(workspace) + hc_status_bytes(B));
  const int in_lds = state_in_lds(m) ? 1 : 0;
  const size_t lds = mask_words_bytes(m) + (in_lds ? 2 * static_cast<size_t>(m) * sizeof(int) : 0);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (m <= HC_M_SMALL)
    hipLaunchKernelGGL(nnchain_batched_kernel<HC_T_SMALL>, dim3(B), dim3(HC_T_SMALL), lds, st, D, m, method, Z,
                       status, state, in_lds);
  else
    hipLaunchKernelGGL(nnchain_batched_kernel<HC_T_LARGE>, dim3(B), dim3(HC_T_LARGE), lds, st, D, m, method, Z,
                       status, state, in_lds);
  return launch_error("cc_hc_nnchain_batched");
}

extern "C" int cc_hc_check(const void* workspace, int B, void* stream) {
  if (!workspace || B <= 0) {
    cc::set_error("cc_hc_check: bad arguments");
    return CC_ERR_ARG;
  }
  hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
  int bad = -1;
  constexpr int CH = 1024;
  int buf[CH];
  for (int b0 = 0; e == hipSuccess && bad < 0 && b0 < B; b0 += CH) {
    const int c = B - b0 < CH ? B - b0 : CH;
    e = hipMemcpy(buf, static_cast<const int*>(workspace) + b0, static_cast<size_t>(c) * sizeof(int),
                  hipMemcpyDeviceToHost);
    for (int i = 0; e == hipSuccess && i < c; ++i)
      if (buf[i] != HC_OK) {
        bad = b0 + i;
        break;
      }
  }
  if (e != hipSuccess) {
    cc::set_error(std::string("cc_hc_check: ") + hipGetErrorString(e));
    return CC_ERR_HIP;
  }
  if (bad >= 0) {
    cc::set_error("cc_hc_nnchain_batched: tree " + std::to_string(bad) +
                  " found no neighbour (non-finite distances?); its merges are invalid");
    return CC_ERR_HIP;
  }
  return CC_OK;
}

extern "C" int cc_hc_cut(const double* Z, const int* rank, const int* idx, int B, int m, const int* Ks, int nK,
                         int h_begin, uint8_t* labels, int64_t n, int64_t ldl, void* workspace, size_t ws_bytes,
                         void* stream) {
  if (!Z || !rank || !idx || !Ks || !labels || B <= 0 || m < 2 || nK <= 0 || nK > 65535 || h_begin < 0 ||
      n < m || ldl < static_cast<int64_t>(h_begin) + B || !workspace ||
      ws_bytes < cc_hc_workspace_bytes(m, B, nK) || mask_words_bytes(m) > HC_MASK_LDS_MAX) {
    cc::set_error("cc_hc_cut: bad arguments");
    return CC_ERR_ARG;
  }
  int* links = reinterpret_cast<int*>(static_cast<char*>(workspace) + hc_status_bytes(B) + hc_state_bytes(m, B));
  const int in_lds = link_in_lds(m) ? 1 : 0;
  const size_t lds = mask_words_bytes(m) + (in_lds ? static_cast<size_t>(m) * sizeof(int) : 0);
  hipLaunchKernelGGL(cut_kernel, dim3(B, nK), dim3(CT), lds, static_cast<hipStream_t>(stream), Z, rank, idx, m, Ks,
                     nK, h_begin, labels, n, ldl, links, in_lds);
  return launch_error("cc_hc_cut");
}
