// PAM (partitioning around medoids; Kaufman & Rousseeuw, R's pam with pamonce = 0) as a base
// clusterer on the device: BUILD and SWAP for every (resample b, K) problem of a batch, from the
// symmetric float64 distances D [B][m][m] with a zero diagonal that the device trees consume
// (cc_hc_gather / cc_pdist_batched).  DESIGN.md K11 states the algorithm; consensus_clustering_amd/
// pam.py is the host form.  All arithmetic is float64, and no sum uses a floating-point atomic:
// the same inputs give the same medoids and a bitwise-equal inertia from run to run.
//
//   build_score_kernel  one wave per candidate row i of a tree: step 0 the row sum, step t >= 1
//                       the gain sum_j max(near[j] - D[i][j], 0) (as -gain, +inf for a medoid),
//                       lanes along j (coalesced), grid (row tiles, trees)
//   build_pick_kernel   one workgroup per tree: first index of the smallest score joins the
//                       chain; near[j] = min(near[j], D[i][j])
//   problem_init_kernel one workgroup per (b, K): the first K of the chain, then refresh()
//   swap_eval_kernel    one thread per candidate h of a still-active problem, the lanes of a wave
//                       on 64 neighbouring h: j is walked grouped by its nearest medoid (perm /
//                       segoff), the same j in every lane, and D[j][h] is read for D[h][j] (D is
//                       symmetric), so a wave reads 512 contiguous bytes of row j and each lane
//                       adds its own sums in the order of j: FastPAM1's shared(h) over all j and
//                       corr(h, i) over the segment of medoid i.  dTD(i, h) = shared(h) +
//                       corr(h, i); the thread keeps the i of its smallest corr
//   swap_apply_kernel   one workgroup per problem: first h of the smallest dTD; when it is < 0
//                       the swap, then refresh(); else the problem is converged
//   labels_kernel       one workgroup per problem: labels by ascending medoid item index into the
//                       uint8 label matrix, the inertia and n_iter
//
// refresh() recomputes near / second / nearest slot of every item from the medoids (K reads of
// a medoid's row per item, coalesced along j) and the grouping of the items by slot (a counting
// sort, stable in j, so the order of every sum is fixed).  Launches are ordered by the stream
// alone; no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "ccmi_internal.h"
#include "launch_error.hpp"

#pragma clang fp contract(off)  // every difference and sum of this file is rounded separately

namespace {

constexpr int PT = 256;      // threads per workgroup
constexpr int PW = PT / 64;  // waves per workgroup = candidate rows per workgroup
constexpr int PAM_KMAX = 127;
constexpr int PAM_MMAX = 65535;
constexpr size_t PAM_ALIGN = 256;

size_t align_up(size_t v) { return (v + PAM_ALIGN - 1) / PAM_ALIGN * PAM_ALIGN; }

// workspace: the active-problems word, per tree the BUILD state, per problem the SWAP state
struct Layout {
  size_t word, score, near0, ismed, chain, med, segoff, nearv, second, nearP, secondP, bestval, slot, perm, besti,
      active, niter, total;
  Layout(int m, int B, int nK, int Kmax) {
    const size_t mm = static_cast<size_t>(m), bb = static_cast<size_t>(B), pp = bb * static_cast<size_t>(nK);
    const size_t kk = static_cast<size_t>(Kmax);
    size_t o = 0;
    auto take = [&o](size_t bytes) {
      const size_t at = o;
      o += align_up(bytes);
      return at;
    };
    word = take(sizeof(int));
    score = take(bb * mm * sizeof(double));
    near0 = take(bb * mm * sizeof(double));
    ismed = take(bb * mm * sizeof(int));
    chain = take(bb * kk * sizeof(int));
    med = take(pp * kk * sizeof(int));
    segoff = take(pp * (kk + 1) * sizeof(int));
    nearv = take(pp * mm * sizeof(double));
    second = take(pp * mm * sizeof(double));
    nearP = take(pp * mm * sizeof(double));
    secondP = take(pp * mm * sizeof(double));
    bestval = take(pp * mm * sizeof(double));
    slot = take(pp * mm * sizeof(int));
    perm = take(pp * mm * sizeof(int));
    besti = take(pp * mm * sizeof(int));
    active = take(pp * sizeof(int));
    niter = take(pp * sizeof(int));
    total = o;
  }
};

// device view of the workspace
struct Ws {
  int* word;
  double *score, *near0;
  int *ismed, *chain, *med, *segoff;
  double *nearv, *second, *nearP, *secondP, *bestval;
  int *slot, *perm, *besti, *active, *niter;
};

Ws view(void* workspace, const Layout& L) {
  char* w = static_cast<char*>(workspace);
  Ws s;
  s.word = reinterpret_cast<int*>(w + L.word);
  s.score = reinterpret_cast<double*>(w + L.score);
  s.near0 = reinterpret_cast<double*>(w + L.near0);
  s.ismed = reinterpret_cast<int*>(w + L.ismed);
  s.chain = reinterpret_cast<int*>(w + L.chain);
  s.med = reinterpret_cast<int*>(w + L.med);
  s.segoff = reinterpret_cast<int*>(w + L.segoff);
  s.nearv = reinterpret_cast<double*>(w + L.nearv);
  s.second = reinterpret_cast<double*>(w + L.second);
  s.nearP = reinterpret_cast<double*>(w + L.nearP);
  s.secondP = reinterpret_cast<double*>(w + L.secondP);
  s.bestval = reinterpret_cast<double*>(w + L.bestval);
  s.slot = reinterpret_cast<int*>(w + L.slot);
  s.perm = reinterpret_cast<int*>(w + L.perm);
  s.besti = reinterpret_cast<int*>(w + L.besti);
  s.active = reinterpret_cast<int*>(w + L.active);
  s.niter = reinterpret_cast<int*>(w + L.niter);
  return s;
}

// K of problem k, kept inside what the workspace was sized for whatever the device array holds
__device__ inline int clamp_K(const int* Ks, int k, int Kmax, int m) {
  const int hi = Kmax < m ? Kmax : m;
  const int K = Ks[k];
  return K < 1 ? 1 : (K > hi ? hi : K);
}

// Butterfly sum over the 64 lanes: a + b is commutative, so every lane ends with the same bits.
__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Smallest (v, key) in lexicographic order over the 64 lanes; every lane ends with it.
__device__ inline void wave_argmin(double& v, int& key) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int ok = __shfl_xor(key, o);
    if (ov < v || (ov == v && ok < key)) {
      v = ov;
      key = ok;
    }
  }
}

// First index of the smallest val[0..m) over the workgroup; every thread returns the same pair.
__device__ inline void block_argmin(const double* __restrict__ val, int m, double* sv, int* si, double& v, int& i) {
  v = INFINITY;
  i = 0x7fffffff;
  for (int j = threadIdx.x; j < m; j += PT) {
    const double x = val[j];
    if (x < v) {  // ascending j in a thread: strict < keeps the first
      v = x;
      i = j;
    }
  }
  wave_argmin(v, i);
  __syncthreads();  // sv / si may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) {
    sv[threadIdx.x >> 6] = v;
    si[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  v = sv[0];
  i = si[0];
#pragma unroll
  for (int w = 1; w < PW; ++w)
    if (sv[w] < v || (sv[w] == v && si[w] < i)) {
      v = sv[w];
      i = si[w];
    }
}

__global__ __launch_bounds__(PT) void build_score_kernel(const double* __restrict__ D, int m, int step,
                                                         const double* __restrict__ near0,
                                                         const int* __restrict__ ismed,
                                                         double* __restrict__ score) {
  const size_t b = blockIdx.y, mm = static_cast<size_t>(m);
  const int i = blockIdx.x * PW + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= m) return;  // the whole wave
  const double* row = D + (b * mm + i) * mm;
  double acc = 0.0;
  bool is_medoid = false;
  if (step == 0) {
#pragma unroll 4
    for (int j = lane; j < m; j += 64) acc += row[j];
  } else {
    is_medoid = ismed[b * mm + i] != 0;
    if (!is_medoid) {
      const double* nr = near0 + b * mm;
#pragma unroll 4
      for (int j = lane; j < m; j += 64) acc += fmax(nr[j] - row[j], 0.0);
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) score[b * mm + i] = step == 0 ? acc : (is_medoid ? INFINITY : -acc);
}

__global__ __launch_bounds__(PT) void build_pick_kernel(const double* __restrict__ D, int m, int step, int Kmax,
                                                        const double* __restrict__ score,
                                                        double* __restrict__ near0, int* __restrict__ ismed,
                                                        int* __restrict__ chain) {
  __shared__ double sv[PW];
  __shared__ int si[PW];
  const size_t b = blockIdx.x, mm = static_cast<size_t>(m);
  double v;
  int i;
  block_argmin(score + b * mm, m, sv, si, v, i);
  if (i < 0 || i >= m) i = 0;  // only when no score is finite (distances that are not finite)
  if (threadIdx.x == 0) {
    chain[b * Kmax + step] = i;
    ismed[b * mm + i] = 1;
  }
  const double* row = D + (b * mm + i) * mm;
  double* nr = near0 + b * mm;
  for (int j = threadIdx.x; j < m; j += PT) nr[j] = step == 0 ? row[j] : fmin(nr[j], row[j]);
}

// near / second / slot of every item of problem p from its medoids (lmed [K] in LDS), then the
// items grouped by slot: segoff [K + 1], perm [m] (ascending j inside a slot) and near / second
// in that order.  A medoid takes its own slot, whatever else lies at distance 0.
__device__ void refresh(const double* __restrict__ Db, int m, int K, size_t p, int Kmax, const Ws& s,
                        const int* lmed, int* lcnt, int* loff) {
  const size_t mm = static_cast<size_t>(m);
  const int tid = threadIdx.x;
  double* nearv = s.nearv + p * mm;
  double* second = s.second + p * mm;
  int* slot = s.slot + p * mm;
  int* perm = s.perm + p * mm;
  for (int i = tid; i <= K; i += PT) lcnt[i] = 0;
  __syncthreads();
  for (int j = tid; j < m; j += PT) {
    double n1 = INFINITY, n2 = INFINITY;
    int sl = 0;
    for (int i = 0; i < K; ++i) {
      const int mi = lmed[i];
      const double d = Db[static_cast<size_t>(mi) * mm + j];
      if (d < n1 || mi == j) {
        n2 = n1;
        n1 = d;
        sl = i;
      } else if (d < n2) {
        n2 = d;
      }
    }
    nearv[j] = n1;
    second[j] = n2;
    slot[j] = sl;
    atomicAdd(&lcnt[sl], 1);  // integer counts: the order of arrival does not show
  }
  __syncthreads();
  if (tid == 0) {
    int o = 0;
    for (int i = 0; i < K; ++i) {
      loff[i] = o;
      o += lcnt[i];
    }
    loff[K] = o;  // = m
  }
  __syncthreads();
  for (int i = tid; i <= K; i += PT) s.segoff[p * (Kmax + 1) + i] = loff[i];
  if (tid < K) {  // one thread per slot walks j upwards: a stable placement
    int c = loff[tid];
    const int end = loff[tid + 1];
    for (int j = 0; j < m && c < end; ++j)
      if (slot[j] == tid) perm[c++] = j;
  }
  __syncthreads();
  double* nearP = s.nearP + p * mm;
  double* secondP = s.secondP + p * mm;
  for (int q = tid; q < m; q += PT) {
    int j = perm[q];
    if (static_cast<unsigned>(j) >= static_cast<unsigned>(m)) j = 0;  // never: keeps the read inside the arrays
    nearP[q] = nearv[j];
    secondP[q] = second[j];
  }
}

__global__ __launch_bounds__(PT) void problem_init_kernel(const double* __restrict__ D, int m,
                                                          const int* __restrict__ Ks, int nK, int Kmax, Ws s) {
  __shared__ int lmed[PAM_KMAX + 1], lcnt[PAM_KMAX + 2], loff[PAM_KMAX + 2];
  const size_t p = blockIdx.x, b = p / nK, mm = static_cast<size_t>(m);
  const int K = clamp_K(Ks, static_cast<int>(p % nK), Kmax, m);
  if (threadIdx.x < K) {
    const int i = s.chain[b * Kmax + threadIdx.x];
    lmed[threadIdx.x] = i;
    s.med[p * Kmax + threadIdx.x] = i;
  }
  if (threadIdx.x == 0) {
    s.active[p] = 1;
    s.niter[p] = 0;
  }
  __syncthreads();
  refresh(D + b * mm * mm, m, K, p, Kmax, s, lmed, lcnt, loff);
}

__global__ __launch_bounds__(PT) void swap_eval_kernel(const double* __restrict__ D, int m,
                                                       const int* __restrict__ Ks, int nK, int Kmax, Ws s) {
  __shared__ int lmed[PAM_KMAX + 1], loff[PAM_KMAX + 2];
  const size_t p = blockIdx.x, b = p / nK, mm = static_cast<size_t>(m);
  if (!s.active[p]) return;  // the whole workgroup
  const int K = clamp_K(Ks, static_cast<int>(p % nK), Kmax, m);
  if (threadIdx.x < K) lmed[threadIdx.x] = s.med[p * Kmax + threadIdx.x];
  if (threadIdx.x <= K) loff[threadIdx.x] = s.segoff[p * (Kmax + 1) + threadIdx.x];
  __syncthreads();
  const int h = blockIdx.y * PT + threadIdx.x;  // one candidate per thread
  if (h >= m) return;                           // no barrier follows
  double* bestval = s.bestval + p * mm;
  int* besti = s.besti + p * mm;
  int sh = s.slot[p * mm + h];
  if (sh < 0 || sh >= K) sh = 0;
  if (lmed[sh] == h) {  // a medoid is no candidate
    bestval[h] = INFINITY;
    besti[h] = 0;
    return;
  }
  // D is symmetric: row h is read as column h, so the lanes of a wave read 64 neighbours of row j
  const double* __restrict__ col = D + b * mm * mm + h;
  const int* __restrict__ perm = s.perm + p * mm;
  const double* __restrict__ nearP = s.nearP + p * mm;
  const double* __restrict__ secondP = s.secondP + p * mm;
  double shared = 0.0, best = INFINITY;
  int best_key = 0x7fffffff, best_i = 0;
  for (int i = 0; i < K; ++i) {
    double c = 0.0;
    const int end = loff[i + 1];
#pragma unroll 8  // independent loads in flight; the sums still run in the order of q
    for (int q = loff[i]; q < end; ++q) {  // q, and what it indexes, is the same in every lane
      int j = perm[q];
      if (static_cast<unsigned>(j) >= static_cast<unsigned>(m)) j = 0;  // never: keeps the read inside D
      const double d = col[static_cast<size_t>(j) * mm];
      const double nr = nearP[q];
      const double s0 = fmin(d - nr, 0.0);
      shared += s0;
      c += (fmin(d, secondP[q]) - nr) - s0;
    }
    const int key = lmed[i];
    if (c < best || (c == best && key < best_key)) {  // a tie goes to the lowest medoid item index
      best = c;
      best_key = key;
      best_i = i;
    }
  }
  bestval[h] = shared + best;
  besti[h] = best_i;
}

__global__ __launch_bounds__(PT) void swap_apply_kernel(const double* __restrict__ D, int m,
                                                        const int* __restrict__ Ks, int nK, int Kmax,
                                                        int max_iter, Ws s) {
  __shared__ int lmed[PAM_KMAX + 1], lcnt[PAM_KMAX + 2], loff[PAM_KMAX + 2];
  __shared__ double sv[PW];
  __shared__ int si[PW];
  const size_t p = blockIdx.x, b = p / nK, mm = static_cast<size_t>(m);
  if (!s.active[p]) return;  // the whole workgroup
  const int K = clamp_K(Ks, static_cast<int>(p % nK), Kmax, m);
  double v;
  int h;
  block_argmin(s.bestval + p * mm, m, sv, si, v, h);
  const int done = s.niter[p];
  __syncthreads();  // every thread has read niter before thread 0 writes it
  if (!(v < 0.0) || h < 0 || h >= m || done >= max_iter) {  // the same in every thread
    if (threadIdx.x == 0) s.active[p] = 0;
    return;
  }
  int i = s.besti[p * mm + h];
  if (i < 0 || i >= K) i = 0;
  if (threadIdx.x == 0) {
    s.med[p * Kmax + i] = h;
    s.niter[p] = done + 1;
    atomicAdd(s.word, 1);  // an integer count of the problems that swapped
  }
  if (threadIdx.x < K) lmed[threadIdx.x] = threadIdx.x == i ? h : s.med[p * Kmax + threadIdx.x];
  __syncthreads();
  refresh(D + b * mm * mm, m, K, p, Kmax, s, lmed, lcnt, loff);
}

__global__ __launch_bounds__(PT) void labels_kernel(const double* __restrict__ D, const int* __restrict__ idx, int m,
                                                    const int* __restrict__ Ks, int nK, int Kmax, int h_begin,
                                                    uint8_t* __restrict__ labels, int64_t n, int64_t ldl,
                                                    double* __restrict__ inertia, int* __restrict__ n_iter,
                                                    int64_t ldo, int* __restrict__ medoids, Ws s) {
  __shared__ int lmed[PAM_KMAX + 1], smed[PAM_KMAX + 1];
  __shared__ double red[PW];
  const size_t p = blockIdx.x, b = p / nK, mm = static_cast<size_t>(m);
  const int k = static_cast<int>(p % nK);
  const int K = clamp_K(Ks, k, Kmax, m);
  const int tid = threadIdx.x;
  if (tid < K) smed[tid] = lmed[tid] = s.med[p * Kmax + tid];
  __syncthreads();
  int r = 0;
  if (tid < K)
    for (int i = 0; i < K; ++i) r += lmed[i] < lmed[tid];
  __syncthreads();
  if (tid < K) smed[r] = lmed[tid];  // the medoids are distinct items: a permutation
  __syncthreads();
  const double* Db = D + b * mm * mm;
  const int* id = idx + b * mm;
  uint8_t* out = labels + static_cast<size_t>(k) * n * ldl + (h_begin + static_cast<int64_t>(b));
  double acc = 0.0;
  for (int j = tid; j < m; j += PT) {
    double n1 = INFINITY;
    int lab = 0;
    bool self = false;
    for (int q = 0; q < K; ++q) {  // ascending item index: strict < keeps the lowest at a tie
      const int mi = smed[q];
      const double d = Db[static_cast<size_t>(mi) * mm + j];
      if (mi == j) {
        n1 = d;
        lab = q;
        self = true;
      } else if (!self && d < n1) {
        n1 = d;
        lab = q;
      }
    }
    acc += n1;
    const int item = id[j];
    if (item >= 0 && item < n) out[static_cast<int64_t>(item) * ldl] = static_cast<uint8_t>(lab);
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double t = red[0];
    for (int w = 1; w < PW; ++w) t += red[w];
    const int64_t at = static_cast<int64_t>(k) * ldo + h_begin + static_cast<int64_t>(b);
    if (inertia) inertia[at] = t;
    if (n_iter) n_iter[at] = s.niter[p];
  }
  if (medoids)
    for (int i = tid; i < Kmax; i += PT) medoids[p * Kmax + i] = i < K ? smed[i] : -1;
}

bool shape_ok(int B, int m, int nK, int Kmax) {
  return B > 0 && B <= 65535 && m >= 1 && m <= PAM_MMAX && nK > 0 && nK <= 65535 && Kmax >= 1 && Kmax <= PAM_KMAX &&
         Kmax <= m && static_cast<size_t>(B) * static_cast<size_t>(nK) <= 0x7fffffffu;
}

}  // namespace

extern "C" size_t cc_pam_workspace_bytes(int m, int B, int nK, int Kmax) {
  if (!shape_ok(B, m, nK, Kmax)) return 0;
  return Layout(m, B, nK, Kmax).total;
}

extern "C" int cc_pam_build(const double* D, int B, int m, const int* Ks, int nK, int Kmax, void* workspace,
                            size_t ws_bytes, void* stream) {
  if (!D || !Ks || !workspace || !shape_ok(B, m, nK, Kmax) || ws_bytes < cc_pam_workspace_bytes(m, B, nK, Kmax)) {
    cc::set_error("cc_pam_build: bad arguments (B <= 65535, 1 <= Kmax <= min(m, 127), m <= 65535)");
    return CC_ERR_ARG;
  }
  const Layout L(m, B, nK, Kmax);
  const Ws s = view(workspace, L);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(s.ismed, 0, static_cast<size_t>(B) * m * sizeof(int), st) != hipSuccess)
    return launch_error("cc_pam_build");
  for (int step = 0; step < Kmax; ++step) {
    hipLaunchKernelGGL(build_score_kernel, dim3((m + PW - 1) / PW, B), dim3(PT), 0, st, D, m, step, s.near0, s.ismed,
                       s.score);
    hipLaunchKernelGGL(build_pick_kernel, dim3(B), dim3(PT), 0, st, D, m, step, Kmax, s.score, s.near0, s.ismed,
                       s.chain);
  }
  hipLaunchKernelGGL(problem_init_kernel, dim3(B * nK), dim3(PT), 0, st, D, m, Ks, nK, Kmax, s);
  return launch_error("cc_pam_build");
}

extern "C" int cc_pam_swap_step(const double* D, int B, int m, const int* Ks, int nK, int Kmax, int max_iter,
                                void* workspace, size_t ws_bytes, void* stream) {
  if (!D || !Ks || !workspace || max_iter < 0 || !shape_ok(B, m, nK, Kmax) ||
      ws_bytes < cc_pam_workspace_bytes(m, B, nK, Kmax)) {
    cc::set_error("cc_pam_swap_step: bad arguments");
    return CC_ERR_ARG;
  }
  const Layout L(m, B, nK, Kmax);
  const Ws s = view(workspace, L);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(s.word, 0, sizeof(int), st) != hipSuccess) return launch_error("cc_pam_swap_step");
  hipLaunchKernelGGL(swap_eval_kernel, dim3(B * nK, (m + PT - 1) / PT), dim3(PT), 0, st, D, m, Ks, nK, Kmax, s);
  hipLaunchKernelGGL(swap_apply_kernel, dim3(B * nK), dim3(PT), 0, st, D, m, Ks, nK, Kmax, max_iter, s);
  return launch_error("cc_pam_swap_step");
}

extern "C" int cc_pam_active(const void* workspace, int* active, void* stream) {
  if (!workspace || !active) {
    cc::set_error("cc_pam_active: bad arguments");
    return CC_ERR_ARG;
  }
  hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
  if (e == hipSuccess) e = hipMemcpy(active, workspace, sizeof(int), hipMemcpyDeviceToHost);  // Layout::word = 0
  if (e != hipSuccess) {
    cc::set_error(std::string("cc_pam_active: ") + hipGetErrorString(e));
    return CC_ERR_HIP;
  }
  return CC_OK;
}

extern "C" int cc_pam_labels(const double* D, const int* idx, int B, int m, const int* Ks, int nK, int Kmax,
                             int h_begin, uint8_t* labels, int64_t n, int64_t ldl, double* inertia, int* n_iter,
                             int64_t ldo, int* medoids, void* workspace, size_t ws_bytes, void* stream) {
  if (!D || !idx || !Ks || !labels || !workspace || !shape_ok(B, m, nK, Kmax) || h_begin < 0 || n < m ||
      ldl < static_cast<int64_t>(h_begin) + B || ((inertia || n_iter) && ldo < static_cast<int64_t>(h_begin) + B) ||
      ws_bytes < cc_pam_workspace_bytes(m, B, nK, Kmax)) {
    cc::set_error("cc_pam_labels: bad arguments");
    return CC_ERR_ARG;
  }
  const Layout L(m, B, nK, Kmax);
  const Ws s = view(workspace, L);
  hipLaunchKernelGGL(labels_kernel, dim3(B * nK), dim3(PT), 0, static_cast<hipStream_t>(stream), D, idx, m, Ks, nK,
                     Kmax, h_begin, labels, n, ldl, inertia, n_iter, ldo, medoids, s);
  return launch_error("cc_pam_labels");
}
