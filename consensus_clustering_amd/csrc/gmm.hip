// K12: batched EM for the diagonal Gaussian mixture base clusterer (gmm.py).
//
// A batch is B resamples x nK values of K = B * nK problems over the compact float64 rows
// Xb [B][m][md] (cc_gmm_gather).  One EM iteration of every active problem is three launches,
// ordered by the stream:
//   gmm_estep   (row chunks x problems) one wave per 16-row tile: the weighted log probabilities
//               as one float64 MFMA GEMM of the row image [x, x^2] (inner length 2 md) against
//               [-2 mu prec ; prec], the row logsumexp (scipy's: the maxima leave the sum), the
//               responsibilities resp [m][Kp] and the tile's sum of the row log-norms
//   gmm_decide  one wave per problem: the lower bound from the tile sums, n_iter, converged / max_iter
//   gmm_mstep   one workgroup per problem: resp^T [x, x^2, 1] (inner length m) on the float64 matrix
//               cores, one wave per 16-component x 16-column tile, then the parameters and the
//               E-step's operand image from the sums
// sklearn runs E, M, then the test; the test reads the E-step's bound alone, so deciding before the
// M-step changes nothing but lets one state word gate the next iteration.  The M-step of the
// deciding iteration still runs (gmm_decide leaves `mrun` set for it), as sklearn's does.
//
// Order of every sum (none depends on the grid, the batch or which workgroup ran first; no
// floating-point atomic anywhere):
//   GEMM chains   v_mfma_f64_16x16x4_f64 accumulates the sequential FMA chain over its inner index
//                 (see kmeans_f64.hip): j = 0 .. 2 md - 1 in the E-step, r = 0 .. m - 1 in the M-step
//   logsumexp, lower bound   gmm_shared.hpp: the row tail of the E-step, gmm_decide and gmm_pick,
//                 which the full-covariance kernels (gmm_full.hip) share with this file
//   per component constants   j = 0 .. md - 1 in order; the weight sum c = 0 .. K - 1 in order
//
// cc_gmm_gather and cc_gmm_active, defined here, serve every row-batch clusterer (gmm_full.hip,
// nmf.hip): the gather knows nothing about mixtures, and cc_gmm_active reads only the two header
// words that all three workspaces share (batch_shared.hpp).
#include "gmm_shared.hpp"

namespace {

// the arrays of one problem, in this order: resp [m][Kp], sums [Kp][2 md + 1], W [Kp][2 md],
// cst / ldet / logw [Kp] each, part [ceil(m / 16)]
struct Prob {
  double *resp, *sums, *W, *cst, *ldet, *logw, *part;
  int K, Kp;
};

__host__ __device__ inline size_t prob_doubles(int m, int md, int K) {
  const size_t Kp = pad16(K);
  return static_cast<size_t>(m) * Kp + Kp * (2 * static_cast<size_t>(md) + 1) + Kp * 2 * static_cast<size_t>(md) +
         3 * Kp + static_cast<size_t>((m + 15) / 16);
}

__device__ inline Prob prob(const Args& a, int b, int k) {
  Prob p;
  p.K = a.Ks[k];
  p.Kp = pad16(p.K);
  const size_t Kp = p.Kp, md = a.md;
  p.resp = reinterpret_cast<double*>(a.base + static_cast<size_t>(b) * a.per_b + a.off[k]);
  p.sums = p.resp + static_cast<size_t>(a.m) * Kp;
  p.W = p.sums + Kp * (2 * md + 1);
  p.cst = p.W + Kp * 2 * md;
  p.ldet = p.cst + Kp;
  p.logw = p.ldet + Kp;
  p.part = p.logw + Kp;
  return p;
}

// Xb[b][r][c] = X[idx[b][r]][cols ? cols[b][c] : c]
__global__ __launch_bounds__(GT) void gmm_gather(const double* __restrict__ X, int d, const int* __restrict__ idx,
                                                 const int* __restrict__ cols, int m, int md,
                                                 double* __restrict__ Xb) {
  const int b = blockIdx.y;
  const size_t e = static_cast<size_t>(blockIdx.x) * GT + threadIdx.x;
  if (e >= static_cast<size_t>(m) * md) return;
  const int r = static_cast<int>(e / md), c = static_cast<int>(e % md);
  const int col = cols ? cols[static_cast<size_t>(b) * md + c] : c;
  Xb[static_cast<size_t>(b) * m * md + e] = X[static_cast<size_t>(idx[static_cast<size_t>(b) * m + r]) * d + col];
}

// mode 0: one E-step of the active problems (resp, tile sums); mode 1: the labels of the problems
// whose init won (argmax of the log responsibilities, first index)
template <int MODE>
__global__ __launch_bounds__(GT) void gmm_estep(Args a, const int* __restrict__ idx, uint8_t* __restrict__ labels,
                                                int64_t n, int64_t ldl, int h_begin) {
  extern __shared__ double lds[];
  const int p = blockIdx.y, b = p / a.nK, k = p % a.nK;
  if (MODE == 0 ? !a.st[p].active : !a.st[p].win) return;  // uniform over the workgroup
  const Prob pr = prob(a, b, k);
  const int K = pr.K, Kp = pr.Kp, nct = Kp >> 4, m = a.m, md = a.md, ld = 2 * md;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, q = lane >> 4;
  const int ntile = (m + 15) >> 4;
  double* wl = lds + static_cast<size_t>(wave) * Kp * 16;  // [comp][16 rows] of this wave's tile
  const double* Xb = a.Xb + static_cast<size_t>(b) * m * md;
  const double half_log = md * 1.8378770664093453;  // n_features * log(2 pi)
  const int S = ld >> 2;
  for (int t0 = blockIdx.x * GW; t0 < ntile; t0 += gridDim.x * GW) {  // the same trips for every wave
    const int tile = t0 + wave;
    const bool valid = tile < ntile;
    const int row = tile * 16 + lr;
    const bool rin = valid && row < m;
    const double* xr = Xb + static_cast<size_t>(rin ? row : 0) * md;
    for (int ct = 0; ct < nct; ++ct) {
      f64x4 acc = {0.0, 0.0, 0.0, 0.0};
      const double* wp = pr.W + static_cast<size_t>(ct * 16 + lr) * ld;
      for (int s = 0; s < S; ++s) {
        const int j = 4 * s + q;
        const double av = wp[j];
        const double x = rin ? xr[j < md ? j : j - md] : 0.0;
        acc = mfma(av, j < md ? x : x * x, acc);
      }
      if (ld & 3) {  // the last, partial step of 4
        const int j = 4 * S + q;
        const bool in = j < ld;
        const double av = in ? wp[j] : 0.0;
        const double x = in && rin ? xr[j < md ? j : j - md] : 0.0;
        acc = mfma(av, j < md ? x : x * x, acc);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = ct * 16 + q + 4 * i;
        double v = -INFINITY;
        if (c < K) v = ((-0.5 * (half_log + (pr.cst[c] + acc[i]))) + pr.ldet[c]) + pr.logw[c];
        wl[c * 16 + lr] = v;
      }
    }
    __syncthreads();
    gmm_row_tail<MODE>(wl, K, Kp, m, tile, valid, pr.resp, pr.part, idx + static_cast<size_t>(b) * m, labels,
                       static_cast<size_t>(k) * n * ldl + h_begin + b, n, ldl);
    __syncthreads();
  }
}

// init 1: _initialize from the one-hot resp (weights = nk / m), every problem; init 0: the M-step
// of the problems whose E-step just ran (weights = nk / sum nk)
__global__ __launch_bounds__(GT) void gmm_mstep(Args a, int init, double reg_covar) {
  __shared__ double nk_s[128];
  __shared__ double wsum_s;
  __shared__ int bad_s;
  const int p = blockIdx.x, b = p / a.nK, k = p % a.nK;
  if (!init && !a.st[p].mrun) return;  // uniform over the workgroup
  const Prob pr = prob(a, b, k);
  const int K = pr.K, Kp = pr.Kp, nct = Kp >> 4, m = a.m, md = a.md, ld = 2 * md, nc = 2 * md + 1;
  const int nft = (nc + 15) >> 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, q = lane >> 4;
  const double* Xb = a.Xb + static_cast<size_t>(b) * m * md;
  const int S = m >> 2;
  for (int job = wave; job < nct * nft; job += GW) {
    const int ct = job / nft, ft = job % nft;
    const int j = ft * 16 + lr;
    const int kind = j < md ? 0 : j < ld ? 1 : j == ld ? 2 : 3;  // x, x^2, 1 (the counts), nothing
    const double* xp = Xb + (kind == 0 ? j : kind == 1 ? j - md : 0);
    const double* rp = pr.resp + ct * 16 + lr;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < S; ++s) {
      const size_t r = 4 * s + q;
      const double av = rp[r * Kp];
      const double x = xp[r * md];
      const double bv = kind == 0 ? x : kind == 1 ? x * x : kind == 2 ? 1.0 : 0.0;
      acc = mfma(av, bv, acc);
    }
    if (m & 3) {  // the last, partial step of 4
      const size_t r = 4 * S + q;
      const bool in = r < static_cast<size_t>(m);
      const double av = in ? rp[r * Kp] : 0.0;
      const double x = in ? xp[r * md] : 0.0;
      const double bv = !in ? 0.0 : kind == 0 ? x : kind == 1 ? x * x : kind == 2 ? 1.0 : 0.0;
      acc = mfma(av, bv, acc);
    }
    if (j < nc) {
#pragma unroll
      for (int i = 0; i < 4; ++i) pr.sums[static_cast<size_t>(ct * 16 + q + 4 * i) * nc + j] = acc[i];
    }
  }
  if (tid == 0) bad_s = 0;
  __syncthreads();
  if (tid < 128) nk_s[tid] = tid < K ? pr.sums[static_cast<size_t>(tid) * nc + ld] + 10 * 2.220446049250313e-16 : 0.0;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int c = 0; c < K; ++c) t += nk_s[c];
    wsum_s = init ? static_cast<double>(m) : t;
  }
  __syncthreads();
  for (int e = tid; e < Kp * md; e += GT) {
    const int c = e / md, j = e % md;
    double w1 = 0.0, w2 = 0.0;
    if (c < K) {
      const double nk = nk_s[c];
      const double mean = pr.sums[static_cast<size_t>(c) * nc + j] / nk;
      const double cov = (pr.sums[static_cast<size_t>(c) * nc + md + j] / nk - mean * mean) + reg_covar;
      const double pch = 1.0 / sqrt(cov);
      const double prec = pch * pch;
      w1 = -2.0 * (mean * prec);
      w2 = prec;
    }
    pr.W[static_cast<size_t>(c) * ld + j] = w1;
    pr.W[static_cast<size_t>(c) * ld + md + j] = w2;
  }
  if (tid < Kp) {
    double cs = 0.0, ldt = 0.0, lw = 0.0;
    if (tid < K) {
      const double nk = nk_s[tid];
      bool bad = false;
      for (int j = 0; j < md; ++j) {
        const double mean = pr.sums[static_cast<size_t>(tid) * nc + j] / nk;
        const double cov = (pr.sums[static_cast<size_t>(tid) * nc + md + j] / nk - mean * mean) + reg_covar;
        bad |= !(cov > 0.0);
        const double pch = 1.0 / sqrt(cov);
        cs += (mean * mean) * (pch * pch);
        ldt += log(pch);
      }
      lw = log(nk / wsum_s);
      if (bad) atomicOr(&bad_s, 1);
    }
    pr.cst[tid] = cs;
    pr.ldet[tid] = ldt;
    pr.logw[tid] = lw;
  }
  __syncthreads();
  if (tid == 0 && bad_s) gmm_mark_failed(a.word, a.st[p]);
}

constexpr int MD_MAX = 1 << 20;

// batch_enter for this file's problems
bool enter(Args* a, bool ok, const double* Xb, int m, int md, int B, const int* Ks, int nK, void* ws, size_t ws_bytes,
           const char* error) {
  return batch_enter(a, prob_doubles, MD_MAX, true, ok, Xb, m, md, B, Ks, nK, ws, ws_bytes, error);
}

}  // namespace

extern "C" size_t cc_gmm_workspace_bytes(int m, int md, int B, const int* Ks, int nK) {
  if (!batch_ok(m, md, B, Ks, nK, MD_MAX, true)) return 0;
  return layout<State>(prob_doubles, m, md, B, Ks, nK, nullptr, nullptr);
}

extern "C" int cc_gmm_gather(const double* X, int64_t n, int d, const int* idx, const int* cols, int B, int m, int md,
                             double* Xb, void* stream) {
  if (!X || !idx || !Xb || n < 1 || d < 1 || B < 1 || B > 65535 || m < 1 || md < 1 || (!cols && md != d) ||
      static_cast<size_t>(m) * md > 0x7fffffffull * GT) {
    cc::set_error("cc_gmm_gather: bad arguments (md = d without a column list, B <= 65535)");
    return CC_ERR_ARG;
  }
  const size_t e = static_cast<size_t>(m) * md;
  hipLaunchKernelGGL(gmm_gather, dim3(static_cast<unsigned>((e + GT - 1) / GT), B), dim3(GT), 0,
                     static_cast<hipStream_t>(stream), X, d, idx, cols, m, md, Xb);
  return launch_error("cc_gmm_gather");
}

extern "C" int cc_gmm_start(const double* Xb, const int* idx, int B, int m, int md, const int* Ks, int nK,
                            const uint8_t* init_labels, int64_t n, int64_t ldl, int col_begin, double reg_covar,
                            void* workspace, size_t ws_bytes, void* stream) {
  Args a;
  if (!enter(&a, idx && init_labels && n >= m && columns_ok(col_begin, B, ldl) && reg_covar >= 0.0, Xb, m, md, B, Ks,
             nK, workspace, ws_bytes,
             "cc_gmm_start: bad arguments (1 <= K <= min(m, 127), at most 127 values of K, B * nK <= 65535)"))
    return CC_ERR_ARG;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(workspace, 0, HEADER, st) != hipSuccess) return launch_error("cc_gmm_start");
  const int chunks = (m + GT - 1) / GT;
  hipLaunchKernelGGL(gmm_onehot<Args>, dim3(chunks < 64 ? chunks : 64, B * nK), dim3(GT), 0, st, a, idx, init_labels, n, ldl,
                     col_begin);
  hipLaunchKernelGGL(gmm_mstep, dim3(B * nK), dim3(GT), 0, st, a, 1, reg_covar);
  return launch_error("cc_gmm_start");
}

extern "C" int cc_gmm_em_step(const double* Xb, int B, int m, int md, const int* Ks, int nK, double tol,
                              double reg_covar, int max_iter, void* workspace, size_t ws_bytes, void* stream) {
  Args a;
  if (!enter(&a, tol >= 0.0 && reg_covar >= 0.0 && max_iter >= 1, Xb, m, md, B, Ks, nK, workspace, ws_bytes,
             "cc_gmm_em_step: bad arguments"))
    return CC_ERR_ARG;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(a.word, 0, sizeof(int), st) != hipSuccess) return launch_error("cc_gmm_em_step");
  hipLaunchKernelGGL(gmm_estep<0>, row_grid(m, B, nK), dim3(GT), tile_lds(Ks, nK), st, a,
                     static_cast<const int*>(nullptr), static_cast<uint8_t*>(nullptr), static_cast<int64_t>(0),
                     static_cast<int64_t>(0), 0);
  hipLaunchKernelGGL(gmm_decide<Args>, dim3((B * nK + GW - 1) / GW), dim3(GT), 0, st, a, tol, max_iter);
  hipLaunchKernelGGL(gmm_mstep, dim3(B * nK), dim3(GT), 0, st, a, 0, reg_covar);
  return launch_error("cc_gmm_em_step");
}

extern "C" int cc_gmm_active(const void* workspace, int* active, int* failed, void* stream) {
  if (!workspace || !active) {
    cc::set_error("cc_gmm_active: bad arguments");
    return CC_ERR_ARG;
  }
  int word[2] = {0, 0};
  hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
  if (e == hipSuccess) e = hipMemcpy(word, workspace, sizeof(word), hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    cc::set_error(std::string("cc_gmm_active: ") + hipGetErrorString(e));
    return CC_ERR_HIP;
  }
  *active = word[0];
  if (failed) *failed = word[1];
  return CC_OK;
}

extern "C" int cc_gmm_finish(const double* Xb, const int* idx, int B, int m, int md, const int* Ks, int nK,
                             int keep_best, int h_begin, uint8_t* labels, int64_t n, int64_t ldl, double* lower_bound,
                             int* n_iter, uint8_t* converged, int64_t ldo, void* workspace, size_t ws_bytes,
                             void* stream) {
  Args a;
  if (!enter(&a, idx && labels && n >= m && columns_ok(h_begin, B, ldl) &&
                 (!(lower_bound || n_iter || converged) || columns_ok(h_begin, B, ldo)),
             Xb, m, md, B, Ks, nK, workspace, ws_bytes, "cc_gmm_finish: bad arguments"))
    return CC_ERR_ARG;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(gmm_pick<Args>, dim3((B * nK + GT - 1) / GT), dim3(GT), 0, st, a, keep_best, h_begin, lower_bound,
                     n_iter, converged, ldo);
  hipLaunchKernelGGL(gmm_estep<1>, row_grid(m, B, nK), dim3(GT), tile_lds(Ks, nK), st, a, idx, labels, n, ldl,
                     h_begin);
  return launch_error("cc_gmm_finish");
}
