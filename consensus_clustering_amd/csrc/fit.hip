// One-call k-means of a consensus fit (cc_kmeans_fit) and the shared row preparation
// (cc_prepare_rows).
//
// cc_kmeans_fit replaces the whole per-(K, h) `clusterer.fit_predict(X[indices])` loop of the
// reference (consensus_clustering_parallelised.py:282, KMeans(n_init=3) per CC.py:88-90 and
// :212-214) for resamples [h_begin, h_end): it prepares the MFMA row image, replays the
// k-means++ RandomState streams (cc_kpp_tables), asks cc_kmeans_launch_plan what to launch in the
// caller's workspace and makes those calls (cc_kmeans_batched, cc_kmeans_wide or cc_kmeans_f64,
// by row width and precision).  The separate entry points stay the advanced API; the Python host
// walks the same plan with them and gives the same results.  cc_kmeans_launch_plan is the one
// place that turns a fit into engine calls (feature padding, units per resample, concurrent
// seeders, K values per call, the grid or batch that fits a byte budget): host arithmetic only.
//
// cc_prepare_rows: sklearn centres each resample by its own mean (_kmeans.py:1479-1481); the
// f32 engines centre once by the column means of all rows (distances are translation
// invariant), zero-pad to dpad, take squared row norms and the operand scale 2^e with
// max|X| 2^e <= 2^14, and split the rows into the f16 hi/lo image.  Every reduction has a fixed
// order, so the row image is reproducible run to run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "kmeans_shared.hpp"

extern "C" int cc_kpp_tables(const int32_t* Ks, int nK, int n_init, uint32_t seed, int m,
                             int weight_f64, double* kpp_u, int kpp_stride, int32_t* kpp_pos);

namespace {

using cc::km::align256;
using cc::km::hip_status;
using cc::km::kpp_row_len;

constexpr int RB = 256;  // rows per column-sum block

// partial column sums of rows [RB b, RB b + RB) in float64, rows in order
__global__ void colsum_kernel(const float* __restrict__ X, int n, int d, double* __restrict__ part) {
  const int b = blockIdx.x;
  for (int k = threadIdx.x; k < d; k += blockDim.x) {
    double s = 0.0;
    const int r1 = min(n, RB * (b + 1));
    for (int r = RB * b; r < r1; ++r) s += static_cast<double>(X[static_cast<size_t>(r) * d + k]);
    part[static_cast<size_t>(b) * d + k] = s;
  }
}

// column means: the block partials summed in block order
__global__ void colmean_kernel(const double* __restrict__ part, int nb, int n, int d, float* __restrict__ mean) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= d) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += part[static_cast<size_t>(b) * d + k];
  mean[k] = static_cast<float>(s / n);
}

// centred, zero-padded rows, squared norms (sequential fma over the features) and per-block
// max |x| (order-free).  A NaN or an infinity among the centred values (a non-finite input, or
// inf - inf against an infinite column mean) makes the block's maximum +inf, which
// cc_prepare_rows refuses: for device-resident X and the C ABI this is the only guard.
__global__ void centre_kernel(const float* __restrict__ X, int n, int d, int dpad, const float* __restrict__ mean,
                              float* __restrict__ Xd, float* __restrict__ xnorm, float* __restrict__ amax_part) {
  __shared__ float red[256];
  constexpr float INF = __builtin_huge_valf();
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  float am = 0.f;
  if (r < n) {
    float q = 0.f;
    for (int k = 0; k < dpad; ++k) {
      const float v = k < d ? X[static_cast<size_t>(r) * d + k] - mean[k] : 0.f;
      Xd[static_cast<size_t>(r) * dpad + k] = v;
      q = fmaf(v, v, q);
      am = fmaxf(am, isfinite(v) ? fabsf(v) : INF);  // fmaxf alone drops a NaN operand
    }
    xnorm[r] = q;
  }
  red[threadIdx.x] = am;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) amax_part[blockIdx.x] = red[0];
}

// ---- the rules by which a fit becomes engine launches: each defined here, once ---------------

// feature padding: 32 / 64 / 128 for the on-chip engine (cc_kmeans_batched), a multiple of 32
// for the wide-row engine (cc_kmeans_wide, d > 128)
int dpad_for(int d) {
  for (int p : {32, 64, 128})
    if (d <= p) return p;
  return (d + 31) / 32 * 32;
}

// scratch of cc_prepare_rows: column partials, means, per-block maxima
size_t prep_scratch_bytes(int n, int d) {
  const size_t nb = (static_cast<size_t>(n) + RB - 1) / RB, nr = (static_cast<size_t>(n) + 255) / 256;
  return align256(nb * d * 8) + align256(static_cast<size_t>(d) * 4) + align256(nr * 4);
}

// units per resample: enough to fill every CU of the persistent grid with a balanced last round,
// as few as possible (bigger units pack their sweeps better)
int choose_subsets(int nh, int n_groups, int cus) {
  int best = 1;
  double best_eff = -1.0;
  for (int s = 1; s <= std::max(1, n_groups); ++s) {
    const long long units = static_cast<long long>(nh) * s;
    const long long rounds = (units + cus - 1) / cus;
    const double eff = units >= cus ? static_cast<double>(units) / (static_cast<double>(cus) * rounds)
                                    : static_cast<double>(units) / cus;
    if (eff >= 0.85) return s;
    if (eff > best_eff + 1e-9) {
      best = s;
      best_eff = eff;
    }
  }
  return best;
}

// Problems of a unit that may seed (k-means++) concurrently.  Each seeding problem keeps
// closest-distance columns of m rows in the workspace (7 x m f32 per slot), so the cap shrinks
// with m (<= ~110 MB of columns per workgroup).  Measured (k-means launch, round 3, with the
// workspace budget not binding): C3 m = 40k: 12 / 16 / 20 / 24 / 32 -> 1679 / 1670 / 1656 /
// 1645 / 1647 ms; C5 m = 160k: 6 / 8 / 12 / 16 / 20 / 24 / 32 -> 281 / 283 / 276 / 276 / 275 /
// 273 / 273 ms; C2 m = 8k: 12 / 20 / 32 -> 88.2 / 87.5 / 87.0 ms.  (Round 1 measured 6 best at
// C5: there the larger caps passed the 8 GB budget and halved the grid.)
int default_seedmax(int m) { return std::max(2, std::min(24, 4000000 / std::max(m, 1))); }

// the unit table of a batched call: cc_kmeans_plan for the call's n_sub (deterministic, so the
// planner and whoever launches get the same table); returns nU > 0 or cc_kmeans_plan's error
int plan_units(const int32_t* Ks, int nK, int n_init, int n_sub, std::vector<int32_t>& units) {
  const int cap = std::max(n_sub, nK) + 1;
  units.assign(static_cast<size_t>(cap) * CC_KM_USTRIDE, 0);
  const int nU = cc_kmeans_plan(Ks, nK, n_init, n_sub, units.data(), cap);
  return nU ? nU : CC_ERR_ARG;
}

int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  return cus;
}

}  // namespace

extern "C" int cc_kmeans_dpad(int d) {
  if (d > 0) return dpad_for(d);
  cc::set_error("cc_kmeans_dpad: X must have at least one feature");
  return CC_ERR_ARG;
}

// e with max|X| 2^e <= 2^14, so the f16 hi/lo operand pair stays in range
extern "C" int cc_scale_exponent(float amax, int* e) {
  if (!e || !std::isfinite(amax)) {
    cc::set_error(e ? "cc_scale_exponent: X contains non-finite values" : "cc_scale_exponent: bad arguments");
    return CC_ERR_ARG;
  }
  *e = amax == 0.f ? 0
                  : std::max(-62, std::min(62, 14 - static_cast<int>(std::ceil(std::log2(static_cast<double>(amax))))));
  return CC_OK;
}

// Pure host arithmetic (no HIP call): the one place that decides what is launched for a fit.
extern "C" int cc_kmeans_launch_plan(int d, int m, int nh, const int32_t* Ks, int nK, int n_init, int precision,
                                     int cus, size_t budget, size_t budget_hard, int n_sub, int seedmax, int grid,
                                     cc_km_call* calls, int max_calls) {
  if (d <= 0 || m <= 0 || nh <= 0 || !Ks || nK <= 0 || n_init <= 0 || cus <= 0 || n_sub < 0 || seedmax < 0 ||
      grid < 0 || !calls || max_calls < 0 || (precision != CC_KM_FAST && precision != CC_KM_F64)) {
    cc::set_error("cc_kmeans_launch_plan: bad arguments");
    return CC_ERR_ARG;
  }
  budget = std::min(budget, budget_hard);
  int nc = 0;
  const auto emit = [&](int engine, int k0, int nk, int par, int ns, int sm, size_t ws) {
    if (nc >= max_calls) {
      cc::set_error("cc_kmeans_launch_plan: more than max_calls engine calls");
      return false;
    }
    calls[nc++] = cc_km_call{engine, k0, nk, par, ns, sm, static_cast<uint64_t>(ws)};
    return true;
  };
  if (precision == CC_KM_F64) {
    for (int k0 = 0; k0 < nK; k0 += 64) {  // 64 K values per call: NKMAX of kmeans_f64.hip
      const int nk = std::min(64, nK - k0);
      const auto per = [&](int g) { return cc_kmeans_f64_workspace_bytes(m, d, Ks + k0, nk, g, nh); };
      const int g0 = grid ? grid : static_cast<int>(std::min<long long>(4LL * cus, static_cast<long long>(nh) * nk));
      // Never more than budget_hard.  Below it the grid keeps two resident workgroups per CU (the
      // kernel's occupancy) even when their scratch exceeds the budget: with one per CU the
      // float64 fit runs ~1.25x longer (profiles/r04/f64_budget_r4ak.txt).  A caller who must not
      // exceed the budget passes budget_hard = budget, and the floor vanishes.
      const size_t cap = std::min(std::max(budget, per(std::min(g0, 2 * cus))), budget_hard);
      int lo = 1, hi = g0;  // the largest grid that fits (per is non-decreasing in g), else 1
      while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (per(mid) <= cap) lo = mid;
        else hi = mid - 1;
      }
      if (!emit(CC_KM_ENGINE_F64, k0, nk, lo, 0, 0, per(lo))) return CC_ERR_ARG;
    }
    return nc;
  }
  const int dpad = dpad_for(d);
  if (dpad <= 128) {
    const int ns = n_sub ? n_sub : choose_subsets(nh, nK, cus);
    std::vector<int32_t> units;
    const int nU = plan_units(Ks, nK, n_init, ns, units);
    if (nU < 0) return nU;
    int pmax = 0;
    for (int u = 0; u < nU; ++u) pmax = std::max(pmax, static_cast<int>(units[static_cast<size_t>(u) * CC_KM_USTRIDE]));
    const int sm = std::max(1, std::min({seedmax ? seedmax : default_seedmax(m), 32, pmax}));
    const auto per = [&](int g) { return cc_kmeans_workspace_bytes(m, dpad, units.data(), nU, sm, g); };
    int g = static_cast<int>(std::min<long long>(cus, static_cast<long long>(nh) * nU));
    while (g > 1 && per(g) > budget) g /= 2;
    return emit(CC_KM_ENGINE_BATCHED, 0, nK, g, ns, sm, per(g)) ? nc : CC_ERR_ARG;
  }
  // wide rows: each call takes the K values cc_kmeans_wide_chunk deals it (a K that fits no call
  // alone is that function's error, which names K and n_init) and runs the resamples in equal
  // batches sized to the budget, so every batch has one round-count tail
  for (int k0 = 0, nk; k0 < nK; k0 += nk) {
    nk = cc_kmeans_wide_chunk(m, dpad, Ks + k0, nK - k0, n_init);
    if (nk <= 0) return nk ? nk : CC_ERR_ARG;
    const size_t w1 = cc_kmeans_wide_workspace_bytes(m, dpad, Ks + k0, nk, n_init, 1);
    if (w1 == 0) return CC_ERR_ARG;
    const size_t per = cc_kmeans_wide_workspace_bytes(m, dpad, Ks + k0, nk, n_init, 2) - w1;
    const size_t fixed = w1 - per;  // what a call needs besides its resamples
    const size_t fit = budget > fixed ? (budget - fixed) / per : 0;
    const long long cap = static_cast<long long>(std::max<size_t>(1, std::min<size_t>(nh, fit)));
    const long long rounds = (nh + cap - 1) / cap;
    const int batch = static_cast<int>((nh + rounds - 1) / rounds);
    if (!emit(CC_KM_ENGINE_WIDE, k0, nk, batch, 0, 0, w1 + per * (batch - 1))) return CC_ERR_ARG;
  }
  return nc;
}

namespace {

// What cc_kmeans_fit carves from its workspace ahead of the engines' share, and the engine calls
// planned for the rest of it.
struct FitPlan {
  int dpad = 0, stride = 1, nU = 0;
  std::vector<int32_t> units;  // the batched call's unit table
  std::vector<cc_km_call> calls;
  size_t rows_bytes = 0;    // Xd, xnorm, Xhl, prep scratch (f32 engines)
  size_t tables_bytes = 0;  // units, kpp_u, kpp_pos, stats
};

// ws_bytes = SIZE_MAX: the plan of the workspace query
int make_plan(int n, int d, int m, int nh, const int32_t* Ks, int nK, int n_init, int precision, size_t ws_bytes,
              FitPlan& P) {
  const int cus = device_cus();
  if (cus <= 0) {
    cc::set_error("cc_kmeans_fit: no HIP device");
    return CC_ERR_HIP;
  }
  P.calls.resize(static_cast<size_t>(nK));  // no engine takes less than one K per call
  int nc = 0;
  const auto plan = [&](size_t room) {
    nc = cc_kmeans_launch_plan(d, m, nh, Ks, nK, n_init, precision, cus, room, room, 0, 0, 0, P.calls.data(), nK);
    return std::min(nc, 0);
  };
  // which engine runs, and the batched call's n_sub, do not depend on the room: plan without a
  // limit for the sizes, then for what they leave of ws_bytes
  if (const int rc = plan(SIZE_MAX)) return rc;
  P.dpad = dpad_for(d);
  for (int k = 0; k < nK; ++k) P.stride = std::max(P.stride, kpp_row_len(Ks[k]));
  if (precision == CC_KM_FAST)
    P.rows_bytes = align256(static_cast<size_t>(n) * P.dpad * 4) + align256(static_cast<size_t>(n) * 4) +
                   align256(static_cast<size_t>(n) * 2 * P.dpad * 2) + prep_scratch_bytes(n, d);
  if (P.calls[0].engine == CC_KM_ENGINE_BATCHED && (P.nU = plan_units(Ks, nK, n_init, P.calls[0].n_sub, P.units)) < 0)
    return P.nU;
  P.tables_bytes = align256(static_cast<size_t>(std::max(P.nU, 1)) * CC_KM_USTRIDE * 4) +
                   align256(static_cast<size_t>(nK) * n_init * P.stride * 8) +
                   align256(static_cast<size_t>(nK) * n_init * 4) + align256(128 * 8);
  const size_t pre = P.tables_bytes + P.rows_bytes, room = ws_bytes > pre ? ws_bytes - pre : 0;
  if (ws_bytes != SIZE_MAX)
    if (const int rc = plan(room)) return rc;
  P.calls.resize(static_cast<size_t>(nc));
  for (const cc_km_call& c : P.calls)
    if (ws_bytes < pre || c.ws_bytes > room) {
      cc::set_error("cc_kmeans_fit: workspace too small");
      return CC_ERR_ARG;
    }
  return CC_OK;
}

}  // namespace

extern "C" size_t cc_prepare_rows_scratch_bytes(int n, int d) {
  if (n <= 0 || d <= 0) return 0;
  return prep_scratch_bytes(n, d);
}

extern "C" int cc_prepare_rows(const float* X, int n, int d, int dpad, float* Xd, float* xnorm, uint16_t* Xhl,
                               int* scale_exp, void* scratch, size_t scratch_bytes, void* stream) {
  if (!X || !Xd || !xnorm || !Xhl || !scale_exp || !scratch || n <= 0 || d <= 0 || dpad < d ||
      scratch_bytes < prep_scratch_bytes(n, d)) {
    cc::set_error("cc_prepare_rows: bad arguments");
    return CC_ERR_ARG;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int nb = (n + RB - 1) / RB, nr = (n + 255) / 256;
  char* s = static_cast<char*>(scratch);
  double* part = reinterpret_cast<double*>(s);
  float* mean = reinterpret_cast<float*>(s + align256(static_cast<size_t>(nb) * d * 8));
  float* amax = reinterpret_cast<float*>(s + align256(static_cast<size_t>(nb) * d * 8) + align256(static_cast<size_t>(d) * 4));
  hipLaunchKernelGGL(colsum_kernel, dim3(nb), dim3(std::min(256, (d + 63) / 64 * 64)), 0, st, X, n, d, part);
  hipLaunchKernelGGL(colmean_kernel, dim3((d + 255) / 256), dim3(256), 0, st, part, nb, n, d, mean);
  hipLaunchKernelGGL(centre_kernel, dim3(nr), dim3(256), 0, st, X, n, d, dpad, mean, Xd, xnorm, amax);
  int rc = hip_status("cc_prepare_rows");
  if (rc) return rc;
  std::vector<float> am(static_cast<size_t>(nr));
  if (hipMemcpyAsync(am.data(), amax, sizeof(float) * nr, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    cc::set_error("cc_prepare_rows: reading max|X| failed");
    return CC_ERR_HIP;
  }
  float mx = 0.f;
  for (float v : am) mx = (std::isnan(v) || std::isnan(mx)) ? NAN : std::max(mx, v);
  if (cc_scale_exponent(mx, scale_exp)) {
    cc::set_error("cc_prepare_rows: X contains non-finite values");
    return CC_ERR_ARG;
  }
  return cc_split_f16(Xd, n, dpad, *scale_exp, Xhl, stream);
}

extern "C" size_t cc_kmeans_fit_workspace_bytes(int n, int d, int m, int nh, const int32_t* Ks, int nK,
                                                int n_init, int precision) {
  if (n <= 0 || d <= 0 || m <= 0 || m > n || nh <= 0 || !Ks || nK <= 0 || n_init <= 0 ||
      (precision != CC_KM_FAST && precision != CC_KM_F64))
    return 0;
  FitPlan P;
  if (make_plan(n, d, m, nh, Ks, nK, n_init, precision, SIZE_MAX, P)) return 0;
  size_t engine = 0;
  for (const cc_km_call& c : P.calls) {
    // the query's one constant: a wide call gets room for at most 128 resamples at once (in less
    // than its full batch cc_kmeans_fit runs more, smaller batches)
    const int b = std::min(c.par, 128);
    engine = std::max<size_t>(engine, c.engine == CC_KM_ENGINE_WIDE
                                          ? cc_kmeans_wide_workspace_bytes(m, P.dpad, Ks + c.k0, c.nk, n_init, b)
                                          : c.ws_bytes);
  }
  return P.rows_bytes + P.tables_bytes + align256(engine);
}

extern "C" int cc_kmeans_fit(const void* X, int n, int d, const int32_t* idx_hm, int H, int m, int h_begin,
                             int h_end, const int32_t* Ks, int nK, int n_init, int max_iter, double tol_rel,
                             uint32_t seed, int precision, uint8_t* labels_nh, int ldl, void* inertia,
                             int32_t* n_iter, void* workspace, size_t ws_bytes, void* stream) {
  if (!X || !idx_hm || !Ks || !labels_nh || !workspace || n <= 0 || d <= 0 || m <= 0 || m > n || H <= 0 ||
      h_begin < 0 || h_end > H || h_end < h_begin || nK <= 0 || n_init <= 0 || max_iter <= 0 ||
      ldl < H || (precision != CC_KM_FAST && precision != CC_KM_F64)) {
    cc::set_error("cc_kmeans_fit: bad arguments");
    return CC_ERR_ARG;
  }
  for (int k = 0; k < nK; ++k)
    if (Ks[k] < 1 || Ks[k] > 127 || Ks[k] > m) {
      cc::set_error("cc_kmeans_fit: every K must lie in [1, min(127, m)]");
      return CC_ERR_ARG;
    }
  const int nh = h_end - h_begin;
  if (nh == 0) return CC_OK;
  // the plan for this workspace; an undersized one is rejected here, before anything is carved
  // from it or copied into it
  FitPlan P;
  if (const int rc = make_plan(n, d, m, nh, Ks, nK, n_init, precision, ws_bytes, P)) return rc;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(workspace);
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    char* p = w + off;
    off += align256(bytes);
    return p;
  };
  // host tables -> device (pageable copies, ordered on the stream)
  std::vector<double> u(static_cast<size_t>(nK) * n_init * P.stride);
  std::vector<int32_t> pos(static_cast<size_t>(nK) * n_init);
  int rc = cc_kpp_tables(Ks, nK, n_init, seed, m, precision == CC_KM_F64, u.data(), P.stride, pos.data());
  if (rc) return rc;
  int32_t* units_d = reinterpret_cast<int32_t*>(carve(static_cast<size_t>(std::max(P.nU, 1)) * CC_KM_USTRIDE * 4));
  double* u_d = reinterpret_cast<double*>(carve(u.size() * 8));
  int32_t* pos_d = reinterpret_cast<int32_t*>(carve(pos.size() * 4));
  unsigned long long* stats = reinterpret_cast<unsigned long long*>(carve(128 * 8));
  if (hipMemcpyAsync(u_d, u.data(), u.size() * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(pos_d, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(stats, 0, 128 * 8, st) != hipSuccess ||
      (P.nU > 0 && hipMemcpyAsync(units_d, P.units.data(), static_cast<size_t>(P.nU) * CC_KM_USTRIDE * 4,
                                  hipMemcpyHostToDevice, st) != hipSuccess)) {
    cc::set_error("cc_kmeans_fit: table upload failed");
    return CC_ERR_HIP;
  }
  float *Xd = nullptr, *xnorm = nullptr;
  uint16_t* Xhl = nullptr;
  int e = 0;
  if (precision == CC_KM_FAST) {  // float32 engines: the row image
    Xd = reinterpret_cast<float*>(carve(static_cast<size_t>(n) * P.dpad * 4));
    xnorm = reinterpret_cast<float*>(carve(static_cast<size_t>(n) * 4));
    Xhl = reinterpret_cast<uint16_t*>(carve(static_cast<size_t>(n) * 2 * P.dpad * 2));
    void* scratch = carve(prep_scratch_bytes(n, d));
    rc = cc_prepare_rows(static_cast<const float*>(X), n, d, P.dpad, Xd, xnorm, Xhl, &e, scratch,
                         prep_scratch_bytes(n, d), stream);
    if (rc) return rc;
  }
  // one launch per planned call, each on its own K values: rows k0.. of the k-means++ tables
  // (same stride) and of the outputs
  for (const cc_km_call& c : P.calls) {
    const int32_t* Kc = Ks + c.k0;
    const double* uc = u_d + static_cast<size_t>(c.k0) * n_init * P.stride;
    const int32_t* pc = pos_d + c.k0 * n_init;
    uint8_t* lab = labels_nh + static_cast<size_t>(c.k0) * n * ldl;
    const size_t ko = static_cast<size_t>(c.k0) * H;
    float* in32 = inertia ? static_cast<float*>(inertia) + ko : nullptr;
    int32_t* nit = n_iter ? n_iter + ko : nullptr;
    switch (c.engine) {
      case CC_KM_ENGINE_BATCHED:
        rc = cc_kmeans_batched(Xd, Xhl, xnorm, n, d, P.dpad, e, idx_hm, H, m, h_begin, h_end, units_d,
                               P.units.data(), P.nU, n_init, max_iter, tol_rel, uc, P.stride, pc, lab, ldl, in32,
                               nit, stats, w + off, ws_bytes - off, c.par, c.seedmax, stream);
        break;
      case CC_KM_ENGINE_WIDE:
        rc = cc_kmeans_wide(Xd, Xhl, xnorm, n, d, P.dpad, e, idx_hm, H, m, h_begin, h_end, Kc, c.nk, n_init,
                            max_iter, tol_rel, uc, P.stride, pc, lab, ldl, in32, nit, stats, w + off,
                            ws_bytes - off, c.par, stream);
        break;
      default:
        rc = cc_kmeans_f64(static_cast<const double*>(X), n, d, idx_hm, H, m, h_begin, h_end, Kc, c.nk, n_init,
                           max_iter, tol_rel, uc, P.stride, pc, lab, ldl,
                           inertia ? static_cast<double*>(inertia) + ko : nullptr, nit, w + off, ws_bytes - off,
                           c.par, stream);
    }
    if (rc) return rc;
  }
  return CC_OK;
}
