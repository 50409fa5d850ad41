// What the k-means engines share: the one definition of every step in which scikit-learn's
// exact behaviour lives (the k-means++ cumsum order and column bookkeeping, the lowest-index tie
// rule of relocation, _is_same_clustering, the convergence rule, numpy's pairwise sum), plus the
// vector types, the work-item words and a few host helpers.  kmeans.hip (d <= 128, problem state
// as struct-of-arrays in LDS) and kmeans_wide.hip (d > 128, array of structs) differ in how they
// store a problem, so every function here takes the values it needs and references to the few
// fields it updates; none knows which engine calls it.  kmeans_f64.hip and fit.hip use the
// numpy leaf and the host helpers.  Internal: not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "ccmi_internal.h"

namespace cc {
namespace km {

// ---- host helpers -------------------------------------------------------------------------

// k-means++ local trials of sklearn (_kmeans.py:217): 2 + int(log(K)).
inline int local_trials(int K) { return 2 + static_cast<int>(std::log(static_cast<double>(K))); }

// Doubles per (K, init) row of the k-means++ uniform table: the first centre's draw, then
// local_trials(K) uniforms for each further centre.
inline int kpp_row_len(int K) { return 1 + (K - 1) * local_trials(K); }

inline size_t align256(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }

// Records "<where>: <HIP error string>" as the library's last error.
inline int hip_fail(const std::string& where, hipError_t e) {
  set_error(where + ": " + hipGetErrorString(e));
  return CC_ERR_HIP;
}

// CC_OK, or the pending launch error recorded under `fn`.
inline int hip_status(const char* fn) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CC_OK : hip_fail(fn, e);
}

// ---- types, states, item words ------------------------------------------------------------

typedef float v16f __attribute__((ext_vector_type(16)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef short s4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s4 lds_s4;

__device__ __forceinline__ v16f mfma16(const h8& a, const h8& b, const v16f& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// Problem states.  ST_WAIT and ST_FOLLOW belong to the d <= 128 engine's admission and shared
// init-0 seeding (kmeans.hip); the wide engine starts every problem in ST_SEED.
enum { ST_WAIT = 0, ST_SEED = 1, ST_RUN = 2, ST_FINAL = 3, ST_DONE = 4, ST_FOLLOW = 5 };
// Work-item kinds: first k-means++ column, further columns (min with the closest), Lloyd, final E-step.
enum { IK_SEED0 = 0, IK_SEED = 1, IK_RUN = 2, IK_FINAL = 3 };

// Item word 0 = label buffer<<30 | kind<<24 | problem<<16 | K<<8 | slot offset (word 1, the
// seeding columns of an item, is laid out per engine).
__device__ __forceinline__ int iw_off(unsigned w) { return w & 0xFF; }
__device__ __forceinline__ int iw_K(unsigned w) { return (w >> 8) & 0xFF; }
__device__ __forceinline__ int iw_prob(unsigned w) { return (w >> 16) & 0x3F; }
__device__ __forceinline__ int iw_kind(unsigned w) { return (w >> 24) & 3; }
__device__ __forceinline__ int iw_buf(unsigned w) { return (w >> 30) & 1; }

// 16-B LDS-DMA piece (global_load_lds_dwordx4: lane i of the wave writes 16 B at M0 + 16 i),
// issued from inline asm: opaque to the compiler's waitcnt pass, which would otherwise put a
// vmcnt(0) in front of every LDS read it cannot prove disjoint from the DMA.  Untracked VMEM ops
// only make the compiler's own vmcnt waits stricter (the counter drains in order); the caller
// awaits completion explicitly before the barrier that publishes the data.  M0 is set inside
// the asm; no compiler-generated code in these kernels uses M0.  No "memory" clobber: the piece
// writes LDS nothing touches until that barrier and reads immutable rows (a clobber makes the
// compiler drain vmcnt in front of every piece).
__device__ __forceinline__ void dma_piece16(const void* g, const void* lds_dst) {
  const unsigned la = static_cast<unsigned>(reinterpret_cast<uintptr_t>(
      (__attribute__((address_space(3))) const char*)lds_dst));
  asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(__builtin_amdgcn_readfirstlane(la)), "v"(g));
}

// ---- numpy pairwise sum -------------------------------------------------------------------

// numpy pairwise_sum (numpy/_core/src/umath/loops_utils.h.src) of a contiguous array of
// n <= 128 elements, the block below which numpy does not recurse: sequential below 8, else
// eight interleaved partial sums.  `(center_shift ** 2).sum()` over K <= 127 is one such block.
template <class T>
__device__ __forceinline__ T np_pairwise_leaf(const T* a, int n) {
  if (n < 8) {
    T res = 0;
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  }
  T r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i < n - (n % 8); i += 8)
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

// ---- k-means++ ----------------------------------------------------------------------------

// The uniforms that draw the candidates of centre c >= 1 of the fit (K index kidx, init) from
// the table kpp_u [nK][n_init][stride]: entry 0 of a row is the first centre's draw.
__device__ __forceinline__ const double* kpp_uniforms(const double* kpp_u, int kidx, int n_init, int init,
                                                      int stride, int c, int ntr) {
  return kpp_u + (static_cast<size_t>(kidx) * n_init + init) * stride + 1 + static_cast<size_t>(c - 1) * ntr;
}

// k-means++ candidate positions of one centre, one wave: cand[t] =
// searchsorted(cumsum(closest), u[t] * pot) (side='left': #{cumsum < v}), clipped to m - 1, for
// t < ntr.  The cumsum is blocked by RT-row tiles: each lane sums whole tiles sequentially in
// f64 (the in-tile order of the sklearn cumsum), the wave prefix-sums the tile sums, and the
// crossing tile is walked sequentially from its prefix, so the two levels agree exactly.
// `closest` is 16-B aligned and readable up to m rounded up to 4; T = ceil(m / RT), passed in
// because the d <= 128 kernel holds it as a kernel argument (computing it here cost that kernel
// 8 to 24 B/lane of scratch).
template <int RT, int TMAX>
__device__ void kpp_select(const float* closest, int m, int T, const double* u, int ntr, double pot, int* cand,
                           int lane) {
  static_assert(RT % 4 == 0, "tiles are read as float4");
  double rv[TMAX], base[TMAX];
  int tau[TMAX];
  bool found[TMAX];
#pragma unroll
  for (int t = 0; t < TMAX; ++t) {
    rv[t] = (t < ntr) ? u[t] * pot : 0.0;
    base[t] = 0.0;
    tau[t] = T;
    found[t] = false;
  }
  double run = 0.0;
  for (int b = 0; b < T; b += 64) {
    const int j = b + lane;
    double v = 0.0;
    if (j < T) {
      const float* rowp = closest + RT * j;
      const int nr = min(RT, m - RT * j);
      if (nr == RT) {  // a full tile: all its loads in flight, then the same in-order f64 sum
        float4 q[RT / 4];
#pragma unroll
        for (int r4 = 0; r4 < RT / 4; ++r4) q[r4] = *reinterpret_cast<const float4*>(rowp + 4 * r4);
#pragma unroll
        for (int r4 = 0; r4 < RT / 4; ++r4) {
          v += static_cast<double>(q[r4].x);
          v += static_cast<double>(q[r4].y);
          v += static_cast<double>(q[r4].z);
          v += static_cast<double>(q[r4].w);
        }
      } else {
        for (int r = 0; r < nr; r += 4) {
          const float4 q = *reinterpret_cast<const float4*>(rowp + r);  // m, RT multiples of 4 or tail
          v += static_cast<double>(q.x);
          if (r + 1 < nr) v += static_cast<double>(q.y);
          if (r + 2 < nr) v += static_cast<double>(q.z);
          if (r + 3 < nr) v += static_cast<double>(q.w);
        }
      }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double y = __shfl_up(v, o);
      if (lane >= o) v += y;
    }
    const double cum = run + v;
    const int nvalid = min(64, T - b);
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
      if (t >= ntr) continue;
      const int k = __popcll(__ballot(j < T && cum < rv[t]));
      const double prev = __shfl(cum, max(k - 1, 0));
      if (!found[t] && k < nvalid) {
        found[t] = true;
        tau[t] = b + k;
        base[t] = (k == 0) ? run : prev;
      }
    }
    run = __shfl(cum, 63);
  }
  // within the crossing tile: lane t walks its rows
#pragma unroll
  for (int t = 0; t < TMAX; ++t) {
    if (t >= ntr || lane != t) continue;
    int pos = m;
    if (found[t]) {
      const int r0 = RT * tau[t];
      double acc = base[t];
      int k = 0;
      for (; k < RT && r0 + k < m; ++k) {
        acc += static_cast<double>(closest[r0 + k]);
        if (!(acc < rv[t])) break;
      }
      pos = r0 + k;
    }
    cand[t] = min(pos, m - 1);
  }
}

// The decision that closes the sweep of centre c of a seeding problem (_kmeans.py:232-252),
// one thread.  trial_pot[t]: the potential with candidate t (one entry when c = 0, the first
// centre); cs: the column that held the closest distances during the sweep.  The first best
// trial wins; pot is its f32 potential, and its closest distances are the next current column:
// the sweep wrote trial t's to the t-th column other than cs.  The caller stores the three, takes
// the winner's row (cand[best]; the first centre's row is drawn on the host) and moves to c + 1.
// By value: references to the problem's fields cost the d <= 128 kernel scratch.
struct KppDecision {
  int best, cs;
  float pot;
};
__device__ __forceinline__ KppDecision kpp_decide(const double* trial_pot, int ntr, int c, int cs) {
  const int nt = (c == 0) ? 1 : ntr;
  int best = 0;
  float bv = static_cast<float>(trial_pot[0]);
  for (int t = 1; t < nt; ++t) {
    const float v = static_cast<float>(trial_pot[t]);
    if (v < bv) {
      bv = v;
      best = t;
    }
  }
  return {best, (c == 0) ? 0 : ((best < cs) ? best : best + 1), bv};
}

// ---- Lloyd --------------------------------------------------------------------------------

// Workgroup argmax with the lowest index on ties (the engines' order among tied farthest rows):
// every thread brings its own best (value, index); the result is uniform.  red_v / red_i: NW
// entries of LDS.  Ends on a read of them: the caller syncs before their next use.
template <int NW>
__device__ __forceinline__ void wg_argmax_lowest(float bv, int bi, double* red_v, int* red_i, int tid, double& gv,
                                                 int& gi) {
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if ((tid & 63) == 0) {
    red_v[tid >> 6] = bv;
    red_i[tid >> 6] = bi;
  }
  __syncthreads();
  gv = -__builtin_huge_val();
  gi = 0x7fffffff;
  for (int w = 0; w < NW; ++w)
    if (red_v[w] > gv || (red_v[w] == gv && red_i[w] < gi)) {
      gv = red_v[w];
      gi = red_i[w];
    }
}

// Empty-cluster relocation, after the engine has computed dist[r] >= 0, the squared distance of
// each row that can be taken to its centre (< 0: not eligible): the ne empty clusters map[0..ne)
// take the farthest rows in turn, lowest row on ties (_k_means_common.pyx:186-209 with
// argpartition's order made definite).  A taken row moves from its cluster's sum to the empty
// one's, the counts follow, and it leaves the pool (dist = -1).  The whole workgroup calls.
// The problem's sums are rows [row0, row0 + K) of sums [..][dp] and its counts cnt[row0 ..];
// X + idx[r] * dp is row r of the resample.  (row0 is a parameter, not folded into the two
// pointers by the caller: folded, kmeans_kernel<128> took 8 B/lane more scratch.)
template <int NT, int NW>
__device__ __forceinline__ void relocate_farthest(int m, int ne, const int* map, float* dist, const uint8_t* lab,
                                                  const float* X, const int32_t* idx, int dp, int row0, float* sums,
                                                  unsigned* cnt, double* red_v, int* red_i,
                                                  unsigned long long& n_reloc, int tid) {
  static_assert(NT == 64 * NW, "NW waves of 64");
  for (int e = 0; e < ne; ++e) {
    const int c = map[e];
    float bv = -1.f;
    int bi = 0x7fffffff;
    for (int r = tid; r < m; r += NT) {
      const float v = dist[r];
      if (v > bv) {
        bv = v;
        bi = r;
      }
    }
    double gv;
    int gi;
    wg_argmax_lowest<NW>(bv, bi, red_v, red_i, tid, gv, gi);
    const int old = lab[gi];
    const float* x = X + static_cast<size_t>(idx[gi]) * dp;
    for (int d = tid; d < dp; d += NT) {
      sums[static_cast<size_t>(row0 + old) * dp + d] -= x[d];
      sums[static_cast<size_t>(row0 + c) * dp + d] = x[d];
    }
    __syncthreads();
    if (tid == 0) {
      cnt[row0 + c] = 1;
      cnt[row0 + old] -= 1;
      dist[gi] = -1.f;
      n_reloc += 1;
    }
    __syncthreads();
  }
}

// This thread's share of "did any label change": the two label buffers of a problem compared
// 16 B per thread and load (rows past m hold 0xFF in both).
template <int NT>
__device__ __forceinline__ bool labels_differ(const uint8_t* cur_, const uint8_t* old_, int m, int tid) {
  const uint4* cur = reinterpret_cast<const uint4*>(cur_);
  const uint4* old = reinterpret_cast<const uint4*>(old_);
  bool diff = false;
  for (int e = tid; e < (m + 15) / 16; e += NT) {
    const uint4 x = cur[e], y = old[e];
    diff |= (x.x != y.x) | (x.y != y.y) | (x.z != y.z) | (x.w != y.w);
  }
  return diff;
}

// The state of a problem after its Lloyd item (kind IK_RUN) or final E-step (IK_FINAL) of this
// sweep (_kmeans_single_lloyd, _kmeans.py:697-736), one thread.  A Lloyd iteration whose labels
// did not change is strictly converged: its labels and inertia are final (ST_DONE).  Otherwise
// the squared centre shifts (shift [K]) decide between another iteration (ST_RUN) and the final
// E-step (ST_FINAL: tol reached, or max_iter).  iter counts the Lloyd iterations including this
// one (the caller has added it).  The caller takes the item's inertia on ST_DONE.
__device__ __forceinline__ int lloyd_next_state(int kind, bool changed, const float* shift, int K, float tol,
                                                int max_iter, int iter) {
  if (kind != IK_RUN || !changed) return ST_DONE;
  const float tot = np_pairwise_leaf(shift, K);
  return (tot <= tol || iter >= max_iter) ? ST_FINAL : ST_RUN;
}

// ---- best of n_init -----------------------------------------------------------------------

// The fit KMeans.fit keeps among problems [p0, p0 + n_init) (_kmeans.py:1525-1531): a later init
// replaces the best so far when its inertia is lower AND its clustering differs
// (_is_same_clustering: labels_p -> labels_best is not a function).  The whole workgroup calls;
// lab(p) -> the final labels of problem p, inert(p) -> its inertia; map: KMAX + 1 ints of LDS,
// flag: one.  The result is uniform.
template <int NT, int KMAX, class Lab, class Inert>
__device__ __forceinline__ int best_of_inits(int p0, int n_init, int m, Lab lab, Inert inert, int* map, int& flag,
                                             int tid) {
  static_assert(KMAX < NT, "one thread per map entry");
  int best = p0;
  for (int i = 1; i < n_init; ++i) {
    const int p = p0 + i;
    if (!(inert(p) < inert(best))) continue;
    if (tid <= KMAX) map[tid] = -1;
    if (tid == 0) flag = 0;
    __syncthreads();
    const uint8_t* l1 = lab(p);
    const uint8_t* l2 = lab(best);
    for (int r = tid; r < m; r += NT) map[l1[r]] = l2[r];
    __syncthreads();
    bool bad = false;
    for (int r = tid; r < m; r += NT) bad |= (map[l1[r]] != l2[r]);
    if (bad) flag = 1;
    __syncthreads();
    if (flag) best = p;
    __syncthreads();
  }
  return best;
}

// The kept fit's results: its labels scattered to column h of the K's label matrix [n][ldl] (row
// idx[r] of the data), its inertia and iteration count to entry (kidx, h) of the [nK][H] outputs
// (either may be null).  The whole workgroup calls.
template <int NT>
__device__ __forceinline__ void write_fit(const uint8_t* lab, const int32_t* idx, int m, uint8_t* labels_out, int n,
                                          int ldl, int kidx, int h, int H, float inertia, int n_iter,
                                          float* inertia_out, int32_t* niter_out, int tid) {
  uint8_t* out = labels_out + static_cast<size_t>(kidx) * n * ldl + h;
  for (int r = tid; r < m; r += NT) out[static_cast<size_t>(idx[r]) * ldl] = lab[r];
  if (tid == 0) {
    if (inertia_out) inertia_out[static_cast<size_t>(kidx) * H + h] = inertia;
    if (niter_out) niter_out[static_cast<size_t>(kidx) * H + h] = n_iter;
  }
}

}  // namespace km
}  // namespace cc
