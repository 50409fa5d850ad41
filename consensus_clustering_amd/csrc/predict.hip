// Manhattan distances between the rows of the consensus matrix, for the consensus labels.
//
// The reference's consensus labels (consensus_clustering_parallelised.py:292-314,
// `_get_consensus_labels`) run AgglomerativeClustering(affinity='manhattan') on the rows of C;
// sklearn hands that to scipy.cluster.hierarchy.linkage(C, metric='cityblock'), whose pdist
// sums |u_k - v_k| over k in float64, sequentially (scipy/spatial/src/distance_impl.h).  This
// kernel produces the same float64 values (same terms, same order), so the host linkage over
// them is the reference's linkage.
//
// Tiling: 64 x 64 output tiles of the upper triangle (the lower one is mirrored), 256 threads
// as 16 x 16, each thread 4 x 4 pairs; 32-wide k slabs of both row blocks staged in LDS as
// float32, [k][row] so that a thread reads its 4 rows and 4 columns with two 16-B reads.
#include <tuple>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>

#include "ccmi_internal.h"
#include "linkage_shared.hpp"

namespace {

// 128 x 128 output tiles of the upper triangle, 256 threads as 16 x 16, each thread an 8 x 8
// block of float64 accumulators (rows 8 ty + r, columns 8 tx + c); k slabs of 16 staged in LDS
// as float (two float4 reads per side and k serve 64 accumulators), the next slab's global loads
// in flight under the current slab's arithmetic.  Every output is still one sequential sum over
// k in increasing order, so the values are those of the scalar loop.
constexpr int TB = 128;  // output tile edge
constexpr int KS = 16;   // k slab
constexpr int RB = 8;    // accumulators per thread and side

__global__ __launch_bounds__(256) void manhattan_kernel(const float* __restrict__ C, int n, int d,
                                                        double* __restrict__ D) {
  // blockIdx.x enumerates the upper-triangle tiles row-major
  const int nb = (n + TB - 1) / TB;
  int t = static_cast<int>(blockIdx.x), bi = 0;
  while (t >= nb - bi) {
    t -= nb - bi;
    ++bi;
  }
  const int bj = bi + t;
  __shared__ __attribute__((aligned(16))) double sa[KS][TB];  // staged as float64: no conversions in the k loop
  __shared__ __attribute__((aligned(16))) double sb[KS][TB];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = bi * TB, j0 = bj * TB;
  double acc[RB][RB];
#pragma unroll
  for (int r = 0; r < RB; ++r)
#pragma unroll
    for (int c = 0; c < RB; ++c) acc[r][c] = 0.0;
  // staging: thread tid loads 4 consecutive k of row (tid >> 2) and of row (tid >> 2) + 64, per side
  const int sr = tid >> 2, sk = 4 * (tid & 3);
  float4 ga[2], gb[2];
  auto load = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = sr + 64 * h, gk = k0 + sk;
      const int gi = i0 + r, gj = j0 + r;
      float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
      if (gk + 3 < d) {
        if (gi < n) va = *reinterpret_cast<const float4*>(C + static_cast<int64_t>(gi) * d + gk);
        if (gj < n) vb = *reinterpret_cast<const float4*>(C + static_cast<int64_t>(gj) * d + gk);
      } else {  // the tail of k (or a row of d not a multiple of 4: scalar, unaligned-safe)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float a = (gi < n && gk + q < d) ? C[static_cast<int64_t>(gi) * d + gk + q] : 0.f;
          const float b = (gj < n && gk + q < d) ? C[static_cast<int64_t>(gj) * d + gk + q] : 0.f;
          (&va.x)[q] = a;
          (&vb.x)[q] = b;
        }
      }
      ga[h] = va;
      gb[h] = vb;
    }
  };
  const bool vec = (d & 3) == 0;  // 16-B aligned rows
  auto load_any = [&](int k0) __attribute__((always_inline)) {
    if (vec) {
      load(k0);
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int r = sr + 64 * h, gk = k0 + sk;
        const int gi = i0 + r, gj = j0 + r;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          (&ga[h].x)[q] = (gi < n && gk + q < d) ? C[static_cast<int64_t>(gi) * d + gk + q] : 0.f;
          (&gb[h].x)[q] = (gj < n && gk + q < d) ? C[static_cast<int64_t>(gj) * d + gk + q] : 0.f;
        }
      }
    }
  };
  load_any(0);
  for (int k0 = 0; k0 < d; k0 += KS) {
    __syncthreads();  // the previous slab's reads are done
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        sa[sk + q][sr + 64 * h] = static_cast<double>((&ga[h].x)[q]);
        sb[sk + q][sr + 64 * h] = static_cast<double>((&gb[h].x)[q]);
      }
    __syncthreads();
    if (k0 + KS < d) load_any(k0 + KS);  // in flight under this slab
    const int kn = min(KS, d - k0);
    for (int k = 0; k < kn; ++k) {
      double a[RB], b[RB];
#pragma unroll
      for (int q = 0; q < RB; q += 2) {
        const double2 av = *reinterpret_cast<const double2*>(&sa[k][RB * ty + q]);
        const double2 bv = *reinterpret_cast<const double2*>(&sb[k][RB * tx + q]);
        a[q] = av.x;
        a[q + 1] = av.y;
        b[q] = bv.x;
        b[q + 1] = bv.y;
      }
#pragma unroll
      for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int c = 0; c < RB; ++c) acc[r][c] += fabs(a[r] - b[c]);
    }
  }
#pragma unroll
  for (int r = 0; r < RB; ++r)
#pragma unroll
    for (int c = 0; c < RB; ++c) {
      const int i = i0 + RB * ty + r, j = j0 + RB * tx + c;
      if (i < n && j < n) {
        D[static_cast<int64_t>(i) * n + j] = acc[r][c];
        D[static_cast<int64_t>(j) * n + i] = acc[r][c];
      }
    }
}

}  // namespace

extern "C" int cc_manhattan(const float* C, int n, int d, double* D, void* stream) {
  if (!C || !D || n <= 0 || d <= 0) {
    cc::set_error("cc_manhattan: bad arguments");
    return CC_ERR_ARG;
  }
  const int64_t nb = (n + TB - 1) / TB;
  const int64_t tiles = nb * (nb + 1) / 2;
  if (tiles > 0x7fffffff) {
    cc::set_error("cc_manhattan: n too large");
    return CC_ERR_ARG;
  }
  hipLaunchKernelGGL(manhattan_kernel, dim3(static_cast<unsigned>(tiles)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), C, n, d, D);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    cc::set_error(std::string("cc_manhattan: ") + hipGetErrorString(e));
    return CC_ERR_HIP;
  }
  return CC_OK;
}

// ---- Agglomerative linkage on the device: scipy.cluster.hierarchy.nn_chain
// (scipy/cluster/_hierarchy.pyx, the algorithm linkage() runs for 'complete', 'average' and
// 'weighted'), the tree AgglomerativeClustering cuts (CC.py:306-312 -> sklearn linkage_tree ->
// hierarchy.linkage).  The loop itself, with scipy's sequence of decisions, is cc_link::nn_chain
// (linkage_shared.hpp); the kernels here only give it a scope.  Every step is a scan or an
// update over n entries; the full symmetric n x n float64 matrix stays in HBM (20 GB at
// n = 50k).  Z is written in merge order, unsorted; the host sorts it by distance (stable) and
// relabels, as linkage() does after nn_chain.
//
// The live set is a bitmask in LDS (n / 8 bytes), and every row pass issues its loads in batches
// of NB per thread before any compare (branch-free: dead and diagonal entries read as +inf), so
// a scan is a few HBM round trips instead of one per element and thread.
//
// Single linkage: sklearn's own path (linkage_tree -> _hierarchical_fast.mst_linkage_core, Prim's
// MST-LINKAGE-CORE, for a non-precomputed metric such as the reference's 'manhattan'), which is
// cc_link::prim over D's rows (the cityblock values of DistanceMetric64 are cc_manhattan's, same
// terms and order).
namespace {

constexpr int LT = 1024;  // threads of the one workgroup of a G = 0 run
constexpr int NB = 8;     // loads per thread in flight per row pass

// error word of the workspace header (bits, so that neither report hides the other)
constexpr unsigned LINK_ERR_BARRIER = 1u;       // a grid barrier timed out
constexpr unsigned LINK_ERR_NO_NEIGHBOUR = 2u;  // an nn_chain scan found no live finite neighbour

// One workgroup, one tree: size and chain in the workspace, the live / in-tree bits in LDS.
__global__ __launch_bounds__(LT) void nnchain_group_kernel(double* __restrict__ D, int n, int method,
                                                           double* __restrict__ Z, int* __restrict__ size,
                                                           int* __restrict__ chain, int* __restrict__ err) {
  extern __shared__ unsigned mask[];  // live clusters, one bit each
  cc_link::OneGroup<LT, NB> scope{n, err, static_cast<int>(LINK_ERR_NO_NEIGHBOUR)};
  cc_link::nn_chain(scope, D, n, method, Z, mask, size, chain);
}

__global__ __launch_bounds__(LT) void mst_group_kernel(const double* __restrict__ D, int n, double* __restrict__ out,
                                                       double* __restrict__ cur) {
  extern __shared__ unsigned tree[];  // in_tree, one bit per node
  cc_link::OneGroup<LT, NB> scope{n, nullptr, 0};
  cc_link::prim(scope, D, n, out, cur, tree);
}

// ---- Grid forms: the same loops on G co-resident workgroups.  Workgroup g owns the index slice
// [n g / G, n (g + 1) / G): it scans its slice of a row, updates its slice of a merged row and
// its slice's entries of the merged column, and keeps the running minima of its slice (Prim).
// Each workgroup keeps a replica of the whole live / in-tree bitmask in LDS and private copies of
// the chain and the cluster sizes, and every workgroup takes every decision itself from the same
// data, so the control flow is identical on all of them.  Per step the slices' (minimum, first
// index) pairs go through a grid barrier and every workgroup reduces them in slice order (strict
// <: the lowest index wins ties, as the scan of one workgroup does).  nn_chain needs a second
// barrier after each Lance-Williams update (a later scan of another slice reads the merged
// column).  The barrier is a counter and a generation word in the workspace, with agent-scope
// release / acquire fences (buffer_wbl2 / buffer_inv on gfx950, so the D writes of one XCD are
// seen by the others); a workgroup that waits for more than ~2^27 polls sets an error bit and
// every workgroup leaves (cc_linkage_check reports it).  The workgroups are made co-resident,
// not assumed so: G is capped by the occupancy query of the kernel at its dynamic LDS, and the
// grid forms are started with hipLaunchCooperativeKernel, which the runtime starts only when all
// G workgroups can run at once; if it refuses, the one-workgroup form runs instead (nothing has
// been written by then).
constexpr int LG = 256;    // threads of a grid-form workgroup
constexpr int GMAX = 128;  // workgroups of a grid form (all co-resident: one per CU at most)
constexpr int NBG = 8;     // loads per thread in flight per slice pass
constexpr size_t GHDR = 256;  // workspace header: barrier count, generation, error

struct GridWs {
  unsigned* bar;    // [0] arrivals, [1] generation, [2] error (LINK_ERR_* bits)
  double* pv;       // [2][GMAX] slice minima (double-buffered by barrier parity)
  int* pi;          // [2][GMAX] their indices
};

__device__ __forceinline__ GridWs grid_ws(void* ws) {
  char* b = static_cast<char*>(ws);
  GridWs g;
  g.bar = reinterpret_cast<unsigned*>(b);
  g.pv = reinterpret_cast<double*>(b + GHDR);
  g.pi = reinterpret_cast<int*>(b + GHDR + 2 * GMAX * sizeof(double));
  return g;
}
constexpr size_t grid_ws_bytes() { return GHDR + 2 * GMAX * (sizeof(double) + sizeof(int)); }

// Grid barrier.  FULL: every thread's global writes are complete and written back before the
// arrival and every thread reads after the acquire (agent-scope fences: the D updates of
// nn_chain cross XCDs).  Light (FULL = false): only the slice minima cross, and they are written
// and read with agent-scope atomics, so the arrival only has to follow their completion (no
// cache write-back or invalidation).  Returns false when the wait timed out or another workgroup
// reported an error (the caller returns at once).
template <bool FULL>
__device__ bool grid_sync(const GridWs& gw, unsigned& gen) {
  __shared__ int s_ok;
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's stores and atomics have completed
  __syncthreads();
  if (threadIdx.x == 0) {
    int ok = 1;
    const unsigned want = gen + 1;
    if constexpr (FULL) __threadfence();  // release (writes back this XCD's L2)
    // arrival and generation at agent scope (the slice minima of the light form are agent-scope
    // atomics; these order them against the arrival and the generation word).  The arrival is
    // acquire-release: the last arriver's fetch_add reads every earlier arrival (a release
    // sequence on bar[0]), so its generation store below carries their writes to the waiters.
    if (__hip_atomic_fetch_add(&gw.bar[0], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
      __hip_atomic_store(&gw.bar[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_s_waitcnt(0x0F70);  // the reset is done before the release
      if constexpr (FULL) __threadfence();
      __hip_atomic_store(&gw.bar[1], want, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      unsigned polls = 0;
      while (__hip_atomic_load(&gw.bar[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != want) {
        __builtin_amdgcn_s_sleep(2);
        if ((++polls & 1023u) == 0) {
          // an error of another workgroup (it has left), or this wait has lasted too long; the
          // bit is or-ed in, so a no-neighbour report that a late waiter meets here is kept
          if (__hip_atomic_load(&gw.bar[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u || polls > (1u << 27)) {
            __hip_atomic_fetch_or(&gw.bar[2], LINK_ERR_BARRIER, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ok = 0;
            break;
          }
        }
      }
      // acquire: nothing after this reads before the generation word was seen
      if (ok) (void)__hip_atomic_load(&gw.bar[1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
    }
    if constexpr (FULL) __threadfence();  // acquire (invalidates this CU's L1 and this XCD's L2)
    s_ok = ok;
  }
  __syncthreads();
  ++gen;
  return s_ok != 0;
}

// Publish this workgroup's slice minimum, pass the barrier, and reduce every slice's in slice
// order (the same result on every workgroup).  Returns false on a barrier error.
__device__ bool grid_argmin(const GridWs& gw, unsigned& gen, double& v, int& i, double* rv, int* ri) {
  const int par = gen & 1;
  if (threadIdx.x == 0) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(gw.pv) + par * GMAX + blockIdx.x,
                       static_cast<unsigned long long>(__double_as_longlong(v)), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(gw.pi + par * GMAX + blockIdx.x, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!grid_sync<false>(gw, gen)) return false;
  constexpr double INF = __builtin_huge_val();
  v = INF;
  i = 0x7fffffff;
  if (threadIdx.x < static_cast<int>(gridDim.x)) {  // slice order = index order
    v = __longlong_as_double(static_cast<long long>(__hip_atomic_load(
        reinterpret_cast<unsigned long long*>(gw.pv) + par * GMAX + threadIdx.x, __ATOMIC_RELAXED,
        __HIP_MEMORY_SCOPE_AGENT)));
    i = __hip_atomic_load(gw.pi + par * GMAX + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  cc_link::block_argmin<LG>(v, i, rv, ri);
  return true;
}

// The scope of workgroup blockIdx.x of gridDim.x over one tree (linkage_shared.hpp).
struct GridScope {
  static constexpr int T = LG, NB = NBG;
  GridWs gw;
  unsigned gen = 0;
  int j0, j1;
  __device__ GridScope(void* ws, int n)
      : gw(grid_ws(ws)),
        j0(static_cast<int>(static_cast<int64_t>(n) * blockIdx.x / gridDim.x)),
        j1(static_cast<int>(static_cast<int64_t>(n) * (blockIdx.x + 1) / gridDim.x)) {}
  __device__ bool tree_argmin(double& v, int& i, double* rv, int* ri) { return grid_argmin(gw, gen, v, i, rv, ri); }
  __device__ bool after_update() { return grid_sync<true>(gw, gen); }
  __device__ bool writes_out() const { return blockIdx.x == 0; }
  // every workgroup takes this decision from the same reduced values and leaves; one reports it
  __device__ void no_neighbour() {
    if (blockIdx.x == 0 && threadIdx.x == 0)
      __hip_atomic_fetch_or(&gw.bar[2], LINK_ERR_NO_NEIGHBOUR, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

__global__ __launch_bounds__(LG) void nnchain_grid_kernel(double* __restrict__ D, int n, int method,
                                                          double* __restrict__ Z, int* __restrict__ sizes,
                                                          int* __restrict__ chains, void* ws) {
  extern __shared__ unsigned mask[];  // live clusters, one bit each (a replica per workgroup)
  GridScope scope(ws, n);
  const size_t own = static_cast<size_t>(blockIdx.x) * static_cast<size_t>(n);  // private copies: no sharing
  cc_link::nn_chain(scope, D, n, method, Z, mask, sizes + own, chains + own);
}

// each workgroup keeps the running minima of its slice
__global__ __launch_bounds__(LG) void mst_grid_kernel(const double* __restrict__ D, int n, double* __restrict__ out,
                                                      double* __restrict__ cur, void* ws) {
  extern __shared__ unsigned tree[];  // in_tree, one bit per node (a replica per workgroup)
  GridScope scope(ws, n);
  cc_link::prim(scope, D, n, out, cur, tree);
}

size_t mask_bytes(int n) { return static_cast<size_t>((n + 31) >> 5) * sizeof(unsigned); }

// the dynamic LDS of the bitmask (up to the 160 KiB of a CU, less the static part)
constexpr size_t MASK_LDS_MAX = 160 * 1024 - 1024;

// Workgroups of the grid forms for n (CCMI_LINK_G overrides; 0 = one workgroup): about 1536
// entries per slice (six loads per thread), at most GMAX and at most what the kernel's occupancy
// at its dynamic LDS keeps resident on all CUs at once.
template <typename Kern>
int link_groups(int n, Kern kernel) {
  const char* e = std::getenv("CCMI_LINK_G");
  int cus = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    cus = 1;
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kernel), LG,
                                                   mask_bytes(n)) != hipSuccess)
    per_cu = 0;
  (void)hipGetLastError();
  const int cap = std::min(GMAX, per_cu * cus);
  if (cap <= 0) return 0;
  if (e && e[0]) return std::min(std::max(0, std::atoi(e)), cap);
  return std::max(1, std::min(cap, n / 1536));
}

// Start a grid form cooperatively (all G workgroups co-resident, or the launch fails); without
// cooperative-launch support a plain launch of the occupancy-capped G.
template <typename... KArgs, typename... Args>
hipError_t launch_grid(void (*kernel)(KArgs...), int G, size_t lds, hipStream_t st, Args... args) {
  int dev = 0, coop = 0;
  if (hipGetDevice(&dev) == hipSuccess &&
      hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, dev) == hipSuccess && coop) {
    std::tuple<KArgs...> a(args...);  // the kernel's own parameter types
    void* argv[sizeof...(KArgs)];
    std::apply([&argv](auto&... x) {
      int k = 0;
      ((argv[k++] = static_cast<void*>(&x)), ...);
    }, a);
    return hipLaunchCooperativeKernel(reinterpret_cast<const void*>(kernel), dim3(G), dim3(LG), argv,
                                      static_cast<unsigned>(lds), st);
  }
  hipLaunchKernelGGL(kernel, dim3(G), dim3(LG), lds, st, static_cast<KArgs>(args)...);
  return hipGetLastError();
}

// Both forms: the barrier header (zeroed at every launch, so cc_linkage_check never reads the
// error word of an earlier call), then the sizes and chains ([G][n] each, or [n] at G = 0) or the
// running minima.
size_t nnchain_ws(int n, int G) {
  return grid_ws_bytes() + 2 * static_cast<size_t>(G > 0 ? G : 1) * static_cast<size_t>(n) * sizeof(int);
}
size_t mst_ws(int n, int) { return grid_ws_bytes() + static_cast<size_t>(n) * sizeof(double); }

// What cc_linkage_nnchain and cc_linkage_mst do around their kernels: refuse bad arguments, zero
// the header, try the cooperative grid launch (G > 0), fall back to one workgroup, report.
// grid() returns the launch's error; one() launches.
template <typename Grid, typename One>
int run_linkage(const char* what, bool args_ok, void* workspace, int G, hipStream_t st, Grid grid, One one) {
  if (!args_ok) {
    cc::set_error(std::string(what) + ": bad arguments");
    return CC_ERR_ARG;
  }
  hipError_t e = hipMemsetAsync(workspace, 0, GHDR, st);
  if (e != hipSuccess) {
    cc::set_error(std::string(what) + ": " + hipGetErrorString(e));
    return CC_ERR_HIP;
  }
  e = hipErrorNotReady;
  if (G > 0) {
    e = grid();
    if (e != hipSuccess) (void)hipGetLastError();  // refused before any workgroup ran
  }
  if (e != hipSuccess) {
    one();
    e = hipGetLastError();
  }
  if (e != hipSuccess) {
    cc::set_error(std::string(what) + ": " + hipGetErrorString(e));
    return CC_ERR_HIP;
  }
  return CC_OK;
}

}  // namespace

extern "C" size_t cc_linkage_workspace_bytes(int n) {
  return n > 0 ? nnchain_ws(n, link_groups(n, nnchain_grid_kernel)) : 0;
}

extern "C" int cc_linkage_nnchain(double* D, int n, int method, double* Z, void* workspace, size_t ws_bytes,
                                  void* stream) {
  const int G = n > 0 ? link_groups(n, nnchain_grid_kernel) : 0;
  const bool args_ok = D && Z && n >= 2 && workspace && ws_bytes >= nnchain_ws(n, G) &&
                       (method == CC_LINK_AVERAGE || method == CC_LINK_COMPLETE || method == CC_LINK_WEIGHTED ||
                        method == CC_LINK_WARD) &&
                       mask_bytes(n) <= MASK_LDS_MAX;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  char* const ws = static_cast<char*>(workspace);
  return run_linkage(
      "cc_linkage_nnchain", args_ok, workspace, G, st,
      [&] {
        int* sizes = reinterpret_cast<int*>(ws + grid_ws_bytes());
        return launch_grid(nnchain_grid_kernel, G, mask_bytes(n), st, D, n, method, Z, sizes,
                           sizes + static_cast<size_t>(G) * n, workspace);
      },
      [&] {
        int* sizes = reinterpret_cast<int*>(ws + grid_ws_bytes());
        int* err = reinterpret_cast<int*>(ws) + 2;  // GridWs::bar[2]
        hipLaunchKernelGGL(nnchain_group_kernel, dim3(1), dim3(LT), mask_bytes(n), st, D, n, method, Z, sizes,
                           sizes + n, err);
      });
}

extern "C" size_t cc_linkage_mst_workspace_bytes(int n) { return n > 0 ? mst_ws(n, link_groups(n, mst_grid_kernel)) : 0; }

extern "C" int cc_linkage_mst(const double* D, int n, double* out, void* workspace, size_t ws_bytes, void* stream) {
  const int G = n > 0 ? link_groups(n, mst_grid_kernel) : 0;
  const bool args_ok = D && out && n >= 2 && workspace && ws_bytes >= mst_ws(n, G) && mask_bytes(n) <= MASK_LDS_MAX;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  char* const ws = static_cast<char*>(workspace);
  return run_linkage(
      "cc_linkage_mst", args_ok, workspace, G, st,
      [&] {
        return launch_grid(mst_grid_kernel, G, mask_bytes(n), st, D, n, out,
                           reinterpret_cast<double*>(ws + grid_ws_bytes()), workspace);
      },
      [&] {
        hipLaunchKernelGGL(mst_group_kernel, dim3(1), dim3(LT), mask_bytes(n), st, D, n, out,
                           reinterpret_cast<double*>(ws + grid_ws_bytes()));
      });
}

extern "C" int cc_linkage_check(const void* workspace, size_t ws_bytes, void* stream) {
  if (!workspace || ws_bytes < GHDR) {
    cc::set_error("cc_linkage_check: bad arguments");
    return CC_ERR_ARG;
  }
  unsigned err = 0;
  hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
  if (e == hipSuccess) e = hipMemcpy(&err, static_cast<const char*>(workspace) + 2 * sizeof(unsigned), sizeof(err), hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    cc::set_error(std::string("cc_linkage_check: ") + hipGetErrorString(e));
    return CC_ERR_HIP;
  }
  if (err & LINK_ERR_NO_NEIGHBOUR) {
    cc::set_error("cc_linkage_nnchain: the tree found no neighbour (non-finite distances?); its merges are invalid");
    return CC_ERR_HIP;
  }
  if (err) {
    cc::set_error("cc_linkage: a grid barrier timed out (workgroups not co-resident?)");
    return CC_ERR_HIP;
  }
  return CC_OK;
}
