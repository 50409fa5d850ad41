// K13: batched EM for the full-covariance Gaussian mixture base clusterer (gmm.py FullGMM,
// DESIGN.md K13).
//
// The batch, the rows Xb [B][m][md] (cc_gmm_gather) and the workspace header are the batch frame's
// (batch_shared.hpp), so cc_gmm_active reads this workspace too; the per-problem State is
// gmm.hip's (gmm_shared.hpp).  One EM
// iteration of every active problem is five launches, ordered by the stream:
//   gmmf_estep   (row chunks x problems) a workgroup owns 4 * tpw 16-row tiles.  Per component c it
//                stages the precision factor P_c (upper triangular, [md][md]) and mu_c P_c in LDS
//                once and every wave multiplies its tiles by it on the float64 matrix cores:
//                Y = X_tile P_c, then sum_j (y_j - (mu_c P_c)_j)^2, the weighted log probability.
//                Only the column tiles' rows 0 .. 16 (jt + 1) - 1 are staged and multiplied: the
//                blocks below the diagonal are zero, and adding their products is exact for
//                finite rows.  Then the shared row tail: logsumexp, resp, tile sums (or labels).
//   gmm_decide   the shared kernel: the lower bound, n_iter, converged / max_iter
//   gmmf_means   one workgroup per problem: resp^T [x, 1] (inner length m) on the matrix cores, one
//                wave per 16-component x 16-column tile, then nk, the means and the log weights
//   gmmf_cov     one wave per (problem, component, 16 x 16 tile of the LOWER triangle): the chain of
//                A = resp[r, c] * (x[r, i] - mu_c[i]) against B = x[r, j] - mu_c[j] over the rows,
//                divided by nk, reg_covar added on the diagonal.  This is sklearn's
//                dot(resp_c * diff.T, diff) in its operand order; that matrix is symmetric only up
//                to rounding and LAPACK reads its lower triangle, so the lower triangle is what
//                the device computes.  Centred two-pass form: no sum(r x x^T) - nk mu mu^T.
//   gmmf_factor  one workgroup per (problem, component), in LDS: the Cholesky factor L of the lower
//                triangle, Z = L^-1 by forward substitution against the identity, P = Z^T into
//                the upper triangle of the same matrix, then mu_c P_c and sum_j log P_jj.  A
//                pivot that is not > 0 (NaN included) marks the problem failed.
// The decision is made before the M-step and the M-step of the deciding iteration still runs, as
// in gmm.hip.
//
// Order of every sum (none depends on the grid, the batch, tpw or which workgroup ran first; no
// floating-point atomic anywhere):
//   GEMM chains   v_mfma_f64_16x16x4_f64 accumulates the sequential FMA chain over its inner
//                 index: i = 0 .. min(16 (jt + 1), md) - 1 for column tile jt of the E-step,
//                 r = 0 .. m - 1 in gmmf_means and gmmf_cov
//   row squares   per row, lane q = 0..3 adds (y_j - (mu P)_j)^2 for its columns j = q, q + 4, ..
//                 below md in order, then (q0 + q1) + (q2 + q3)
//   logsumexp, lower bound   gmm_shared.hpp
//   Cholesky      right-looking, columns j = 0 .. md - 1: element (i, k) loses l_ij l_kj for
//                 j = 0 .. k - 1 in order, then is divided by l_kk
//   substitution  z_i = (e_i - sum_k l_ik z_k) / l_ii, the terms leave in the order k = b .. i - 1
//   mu P, log det, weight sum   i = 0 .. j in order; j = 0 .. md - 1 in order; c = 0 .. K - 1 in order
//
// Limits (batch_ok): 1 <= K <= min(m, 127), 1 <= md <= 128, and gmm.hip's on m, B and the problem
// count.  The largest LDS stages: the E-step's 72 KiB block triangle of P_c at md = 128 next to
// 4 * tpw * Kp * 128 bytes of log probabilities (at most 137 KiB), the factor's 131 KiB at md = 128;
// gfx950 lets a workgroup declare 160 KiB once the kernel's dynamic limit is raised.
#include "gmm_shared.hpp"

namespace {

constexpr int GMMF_MDMAX = 128;
constexpr size_t LDS_DEFAULT = 64 * 1024, LDS_MAX = 160 * 1024;

// the arrays of one problem, in this order: resp [m][Kp], sums [Kp][md + 1], mu [Kp][md],
// P [K][md][md] (the covariances' lower triangles between gmmf_cov and gmmf_factor, then the
// precision factors), muP [Kp][md], ldet / logw / nk [Kp] each, part [ceil(m / 16)]
struct Prob {
  double *resp, *sums, *mu, *P, *muP, *ldet, *logw, *nk, *part;
  int K, Kp;
};

__host__ __device__ inline size_t prob_doubles(int m, int md, int K) {
  const size_t Kp = pad16(K), d = md;
  return static_cast<size_t>(m) * Kp + Kp * (d + 1) + Kp * d + static_cast<size_t>(K) * d * d + Kp * d + 3 * Kp +
         static_cast<size_t>((m + 15) / 16);
}

__device__ inline Prob prob(const Args& a, int b, int k) {
  Prob p;
  p.K = a.Ks[k];
  p.Kp = pad16(p.K);
  const size_t Kp = p.Kp, md = a.md;
  p.resp = reinterpret_cast<double*>(a.base + static_cast<size_t>(b) * a.per_b + a.off[k]);
  p.sums = p.resp + static_cast<size_t>(a.m) * Kp;
  p.mu = p.sums + Kp * (md + 1);
  p.P = p.mu + Kp * md;
  p.muP = p.P + static_cast<size_t>(p.K) * md * md;
  p.ldet = p.muP + Kp * md;
  p.logw = p.ldet + Kp;
  p.nk = p.logw + Kp;
  p.part = p.nk + Kp;
  return p;
}

// doubles before column tile jt in the staged block triangle: tile jt holds rows 0 .. 16 (jt + 1) - 1
__host__ __device__ inline int tri_off(int jt) { return 128 * jt * (jt + 1); }

// mode 0: one E-step of the active problems (resp, tile sums); mode 1: the labels of the problems
// whose init won.  NJT: column tiles the accumulators cover, md <= 16 NJT.
template <int NJT, int MODE>
__global__ __launch_bounds__(GT) void gmmf_estep(Args a, int tpw, const int* __restrict__ idx,
                                                 uint8_t* __restrict__ labels, int64_t n, int64_t ldl, int h_begin) {
  extern __shared__ double lds[];
  const int p = blockIdx.y, b = p / a.nK, k = p % a.nK;
  if (MODE == 0 ? !a.st[p].active : !a.st[p].win) return;  // uniform over the workgroup
  const Prob pr = prob(a, b, k);
  const int K = pr.K, Kp = pr.Kp, m = a.m, md = a.md, njt = (md + 15) >> 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, q = lane >> 4;
  const int ntile = (m + 15) >> 4;
  double* Ps = lds;                  // the block triangle of P_c
  double* mus = Ps + tri_off(njt);   // (mu_c P_c)[16 njt], zero from md on
  double* wl0 = mus + 16 * njt;      // [4 tpw tiles][Kp][16 rows]
  const int tile0 = blockIdx.x * (GW * tpw);
  const double* Xb = a.Xb + static_cast<size_t>(b) * m * md;
  const double half_log = md * 1.8378770664093453;  // n_features * log(2 pi)
  const int S = (md + 3) >> 2;
  for (int c = 0; c < K; ++c) {
    __syncthreads();  // the waves are done with the component before
    const double* Pg = pr.P + static_cast<size_t>(c) * md * md;
    for (int jt = 0; jt < njt; ++jt) {
      const int rows = 16 * (jt + 1) < md ? 16 * (jt + 1) : md;
      double* dst = Ps + tri_off(jt);
      for (int e = tid; e < rows * 16; e += GT) {
        const int j = jt * 16 + (e & 15);
        dst[e] = j < md ? Pg[static_cast<size_t>(e >> 4) * md + j] : 0.0;
      }
    }
    for (int e = tid; e < 16 * njt; e += GT) mus[e] = e < md ? pr.muP[static_cast<size_t>(c) * md + e] : 0.0;
    __syncthreads();
    const double ldet = pr.ldet[c], logw = pr.logw[c];
    for (int t = 0; t < tpw; ++t) {
      const int tl = t * GW + wave, tile = tile0 + tl;
      if (tile >= ntile) break;  // uniform over the wave; no barrier below
      const int row = tile * 16 + lr;
      const bool rin = row < m;
      const double* xr = Xb + static_cast<size_t>(rin ? row : 0) * md;
      f64x4 acc[NJT];
#pragma unroll
      for (int jt = 0; jt < NJT; ++jt) acc[jt] = f64x4{0.0, 0.0, 0.0, 0.0};
      for (int s = 0; s < S; ++s) {
        const int i = 4 * s + q;
        const bool in = i < md;  // false only in the last, partial step of 4
        const double x = in && rin ? xr[i] : 0.0;
        const int j0 = s >> 2;  // the first column tile whose rows reach i
#pragma unroll
        for (int jt = 0; jt < NJT; ++jt) {
          if (jt >= j0 && jt < njt) {
            const double av = in ? Ps[tri_off(jt) + i * 16 + lr] : 0.0;
            acc[jt] = mfma(av, x, acc[jt]);
          }
        }
      }
      // acc[jt][i] = Y[row lr][column jt * 16 + q + 4 i]
      double ss = 0.0;
#pragma unroll
      for (int jt = 0; jt < NJT; ++jt) {
        if (jt < njt) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int j = jt * 16 + q + 4 * i;
            if (j < md) {
              const double y = acc[jt][i] - mus[j];
              ss += y * y;
            }
          }
        }
      }
      ss += __shfl_xor(ss, 16);
      ss += __shfl_xor(ss, 32);
      if (q == 0) wl0[(static_cast<size_t>(tl) * Kp + c) * 16 + lr] = ((-0.5 * (half_log + ss)) + ldet) + logw;
    }
  }
  for (int t = 0; t < tpw; ++t) {
    const int tl = t * GW + wave;
    for (int c = K + q; c < Kp; c += 4) wl0[(static_cast<size_t>(tl) * Kp + c) * 16 + lr] = -INFINITY;
  }
  __syncthreads();
  for (int t = 0; t < tpw; ++t) {
    const int tl = t * GW + wave, tile = tile0 + tl;
    if (tile >= ntile) break;  // uniform over the wave; the tail has no barrier
    gmm_row_tail<MODE>(wl0 + static_cast<size_t>(tl) * Kp * 16, K, Kp, m, tile, true, pr.resp, pr.part,
                       idx + static_cast<size_t>(b) * m, labels, static_cast<size_t>(k) * n * ldl + h_begin + b, n,
                       ldl);
  }
}

// gating of the M-step kernels: init 1 = _initialize, every problem; init 0 = the problems whose
// E-step just ran.  A problem that has failed is left alone.
__device__ inline bool mstep_runs(const State& s, int init) { return (init || s.mrun) && !s.failed; }

// nk, the means and the log weights: init 1 weights = nk / m, init 0 weights = nk / sum nk
__global__ __launch_bounds__(GT) void gmmf_means(Args a, int init) {
  __shared__ double nk_s[128];
  __shared__ double wsum_s;
  const int p = blockIdx.x, b = p / a.nK, k = p % a.nK;
  if (!mstep_runs(a.st[p], init)) return;  // uniform over the workgroup
  const Prob pr = prob(a, b, k);
  const int K = pr.K, Kp = pr.Kp, nct = Kp >> 4, m = a.m, md = a.md, nc = md + 1;
  const int nft = (nc + 15) >> 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, q = lane >> 4;
  const double* Xb = a.Xb + static_cast<size_t>(b) * m * md;
  const int S = m >> 2;
  for (int job = wave; job < nct * nft; job += GW) {
    const int ct = job / nft, ft = job % nft;
    const int j = ft * 16 + lr;
    const int kind = j < md ? 0 : j == md ? 2 : 3;  // x, 1 (the counts), nothing
    const double* xp = Xb + (kind == 0 ? j : 0);
    const double* rp = pr.resp + ct * 16 + lr;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < S; ++s) {
      const size_t r = 4 * s + q;
      const double av = rp[r * Kp];
      const double x = xp[r * md];
      acc = mfma(av, kind == 0 ? x : kind == 2 ? 1.0 : 0.0, acc);
    }
    if (m & 3) {  // the last, partial step of 4
      const size_t r = 4 * S + q;
      const bool in = r < static_cast<size_t>(m);
      const double av = in ? rp[r * Kp] : 0.0;
      const double x = in ? xp[r * md] : 0.0;
      acc = mfma(av, !in ? 0.0 : kind == 0 ? x : kind == 2 ? 1.0 : 0.0, acc);
    }
    if (j < nc) {
#pragma unroll
      for (int i = 0; i < 4; ++i) pr.sums[static_cast<size_t>(ct * 16 + q + 4 * i) * nc + j] = acc[i];
    }
  }
  __syncthreads();
  if (tid < 128) nk_s[tid] = tid < K ? pr.sums[static_cast<size_t>(tid) * nc + md] + 10 * 2.220446049250313e-16 : 0.0;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int c = 0; c < K; ++c) t += nk_s[c];
    wsum_s = init ? static_cast<double>(m) : t;
  }
  __syncthreads();
  for (int e = tid; e < Kp * md; e += GT) {
    const int c = e / md, j = e % md;
    pr.mu[e] = c < K ? pr.sums[static_cast<size_t>(c) * nc + j] / nk_s[c] : 0.0;
  }
  if (tid < Kp) {
    pr.nk[tid] = tid < K ? nk_s[tid] : 0.0;
    pr.logw[tid] = tid < K ? log(nk_s[tid] / wsum_s) : 0.0;
  }
}

// the lower triangle of every component's covariance; jobs: the most (component, tile) pairs of a problem
__global__ __launch_bounds__(GT) void gmmf_cov(Args a, int init, double reg_covar) {
  const int p = blockIdx.y, b = p / a.nK, k = p % a.nK;
  if (!mstep_runs(a.st[p], init)) return;
  const Prob pr = prob(a, b, k);
  const int K = pr.K, Kp = pr.Kp, m = a.m, md = a.md, njt = (md + 15) >> 4, ntri = njt * (njt + 1) / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, q = lane >> 4;
  const int job = blockIdx.x * GW + wave;
  if (job >= K * ntri) return;  // no barrier in this kernel
  const int c = job / ntri, tri = job % ntri;
  int it = 0;
  while ((it + 1) * (it + 2) / 2 <= tri) ++it;
  const int jt = tri - it * (it + 1) / 2;  // jt <= it
  const int i = it * 16 + lr, j = jt * 16 + lr;
  const bool iin = i < md, jin = j < md;
  const double* Xb = a.Xb + static_cast<size_t>(b) * m * md;
  const double* mu = pr.mu + static_cast<size_t>(c) * md;
  const double mui = iin ? mu[i] : 0.0, muj = jin ? mu[j] : 0.0;
  const double* xi = Xb + (iin ? i : 0);
  const double* xj = Xb + (jin ? j : 0);
  const double* rp = pr.resp + c;
  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  const int S = m >> 2;
  for (int s = 0; s < S; ++s) {
    const size_t r = 4 * s + q;
    const double w = rp[r * Kp];
    const double av = iin ? w * (xi[r * md] - mui) : 0.0;
    const double bv = jin ? xj[r * md] - muj : 0.0;
    acc = mfma(av, bv, acc);
  }
  if (m & 3) {  // the last, partial step of 4
    const size_t r = 4 * S + q;
    const bool in = r < static_cast<size_t>(m);
    const double w = in ? rp[r * Kp] : 0.0;
    const double av = in && iin ? w * (xi[r * md] - mui) : 0.0;
    const double bv = in && jin ? xj[r * md] - muj : 0.0;
    acc = mfma(av, bv, acc);
  }
  const double nk = pr.nk[c];
  double* C = pr.P + static_cast<size_t>(c) * md * md;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int gi = it * 16 + q + 4 * e;  // acc[e] = C[gi][j]
    if (gi < md && j <= gi) {
      double v = acc[e] / nk;
      if (gi == j) v += reg_covar;
      C[static_cast<size_t>(gi) * md + j] = v;
    }
  }
}

// P_c, mu_c P_c and the log determinant from the covariance's lower triangle; grid.x: the most components
__global__ __launch_bounds__(GT) void gmmf_factor(Args a, int init) {
  extern __shared__ double lds[];
  const int p = blockIdx.y, b = p / a.nK, k = p % a.nK, c = blockIdx.x;
  if (!mstep_runs(a.st[p], init)) return;  // uniform over the workgroup
  const Prob pr = prob(a, b, k);
  if (c >= pr.K) return;
  const int md = a.md, ld = md | 1;  // an odd row length: a column walks all LDS banks
  const int tid = threadIdx.x;
  double* A = lds;           // [md][ld]: L in the lower triangle, then P above the diagonal
  double* pd = A + md * ld;  // the diagonal of P
  double* mu_s = pd + md;
  double* G = pr.P + static_cast<size_t>(c) * md * md;
  for (int e = tid; e < md * md; e += GT) {
    const int i = e / md, j = e % md;
    A[i * ld + j] = j <= i ? G[e] : 0.0;
  }
  for (int e = tid; e < md; e += GT) mu_s[e] = pr.mu[static_cast<size_t>(c) * md + e];
  __syncthreads();
  const int ti = tid >> 4, tk = tid & 15;
  for (int j = 0; j < md; ++j) {
    const double d = A[j * ld + j];  // every thread reads the same pivot
    if (!(d > 0.0)) {                // NaN included: sklearn's "ill-defined empirical covariance"
      if (tid == 0) gmm_mark_failed(a.word, a.st[p]);
      return;
    }
    const double ljj = sqrt(d);
    __syncthreads();
    for (int i = j + 1 + tid; i < md; i += GT) A[i * ld + j] = A[i * ld + j] / ljj;
    if (tid == 0) A[j * ld + j] = ljj;
    __syncthreads();
    for (int i = j + 1 + ti; i < md; i += 16) {
      const double lij = A[i * ld + j];
      for (int kk = j + 1 + tk; kk <= i; kk += 16) A[i * ld + kk] = A[i * ld + kk] - lij * A[kk * ld + j];
    }
    __syncthreads();
  }
  // column bb of Z = L^-1 is row bb of P; the lower triangle and the diagonal are only read here
  for (int bb = tid; bb < md; bb += GT) {
    double pdb = 0.0;
    for (int i = bb; i < md; ++i) {
      double t = i == bb ? 1.0 : 0.0;
      for (int kk = bb; kk < i; ++kk) t = t - A[i * ld + kk] * (kk == bb ? pdb : A[bb * ld + kk]);
      const double z = t / A[i * ld + i];
      if (i == bb)
        pdb = z;
      else
        A[bb * ld + i] = z;
    }
    pd[bb] = pdb;
  }
  __syncthreads();
  for (int j = tid; j < md; j += GT) {
    double t = 0.0;
    for (int i = 0; i <= j; ++i) t += mu_s[i] * (i == j ? pd[j] : A[i * ld + j]);
    pr.muP[static_cast<size_t>(c) * md + j] = t;
  }
  if (tid == 0) {
    double t = 0.0;
    for (int j = 0; j < md; ++j) t += log(pd[j]);
    pr.ldet[c] = t;
  }
  for (int e = tid; e < md * md; e += GT) {
    const int i = e / md, j = e % md;
    G[e] = i < j ? A[i * ld + j] : i == j ? pd[i] : 0.0;
  }
}

// batch_enter for this file's problems
bool enter(Args* a, bool ok, const double* Xb, int m, int md, int B, const int* Ks, int nK, void* ws, size_t ws_bytes,
           const char* error) {
  return batch_enter(a, prob_doubles, GMMF_MDMAX, true, ok, Xb, m, md, B, Ks, nK, ws, ws_bytes, error);
}

int max_k(const int* Ks, int nK) {
  int v = 0;
  for (int k = 0; k < nK; ++k) v = Ks[k] > v ? Ks[k] : v;
  return v;
}

size_t estep_lds(int md, int Kp, int tpw) {
  const int njt = (md + 15) / 16;
  return (static_cast<size_t>(tri_off(njt)) + 16 * njt + static_cast<size_t>(GW) * tpw * Kp * 16) * sizeof(double);
}

// tiles per wave: the most of 4, 2, 1 that leaves room for a second workgroup's LDS on the CU's
// share (64 KiB), else the most that fits at all; the results do not depend on it
int estep_tpw(int md, int Kp) {
  for (int tpw = 4; tpw >= 1; tpw >>= 1)
    if (estep_lds(md, Kp, tpw) <= LDS_DEFAULT) return tpw;
  for (int tpw = 4; tpw > 1; tpw >>= 1)
    if (estep_lds(md, Kp, tpw) <= LDS_MAX) return tpw;
  return 1;
}

template <class Kern>
int allow_lds(Kern kernel, size_t bytes, const char* what) {
  if (bytes <= LDS_DEFAULT) return CC_OK;
  if (bytes > LDS_MAX ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          static_cast<int>(bytes)) != hipSuccess) {
    (void)hipGetLastError();
    cc::set_error(std::string(what) + ": the kernel's dynamic LDS limit could not be raised");
    return CC_ERR_HIP;
  }
  return CC_OK;
}

template <int NJT, int MODE>
int launch_estep_n(const Args& a, int tpw, size_t lds, hipStream_t st, const int* idx, uint8_t* labels, int64_t n,
                   int64_t ldl, int h_begin, const char* what) {
  const int rc = allow_lds(gmmf_estep<NJT, MODE>, lds, what);
  if (rc != CC_OK) return rc;
  const int ntile = (a.m + 15) / 16, per = GW * tpw;
  hipLaunchKernelGGL((gmmf_estep<NJT, MODE>), dim3((ntile + per - 1) / per, a.B * a.nK), dim3(GT), lds, st, a, tpw, idx,
                     labels, n, ldl, h_begin);
  return CC_OK;
}

template <int MODE>
int launch_estep(const Args& a, const int* Ks, int nK, hipStream_t st, const int* idx, uint8_t* labels, int64_t n,
                 int64_t ldl, int h_begin, const char* what) {
  const int Kp = max_kp(Ks, nK), tpw = estep_tpw(a.md, Kp), njt = (a.md + 15) / 16;
  const size_t lds = estep_lds(a.md, Kp, tpw);
  if (njt <= 1) return launch_estep_n<1, MODE>(a, tpw, lds, st, idx, labels, n, ldl, h_begin, what);
  if (njt <= 2) return launch_estep_n<2, MODE>(a, tpw, lds, st, idx, labels, n, ldl, h_begin, what);
  if (njt <= 4) return launch_estep_n<4, MODE>(a, tpw, lds, st, idx, labels, n, ldl, h_begin, what);
  return launch_estep_n<8, MODE>(a, tpw, lds, st, idx, labels, n, ldl, h_begin, what);
}

// the M-step of every problem that runs one: means, covariances, factors
int launch_mstep(const Args& a, const int* Ks, int nK, int init, double reg_covar, hipStream_t st, const char* what) {
  const int md = a.md, njt = (md + 15) / 16, ntri = njt * (njt + 1) / 2, Kmax = max_k(Ks, nK);
  const size_t lds = (static_cast<size_t>(md) * (md | 1) + 2 * md) * sizeof(double);
  const int rc = allow_lds(gmmf_factor, lds, what);
  if (rc != CC_OK) return rc;
  hipLaunchKernelGGL(gmmf_means, dim3(a.B * a.nK), dim3(GT), 0, st, a, init);
  hipLaunchKernelGGL(gmmf_cov, dim3((Kmax * ntri + GW - 1) / GW, a.B * a.nK), dim3(GT), 0, st, a, init, reg_covar);
  hipLaunchKernelGGL(gmmf_factor, dim3(Kmax, a.B * a.nK), dim3(GT), lds, st, a, init);
  return CC_OK;
}

}  // namespace

extern "C" size_t cc_gmm_full_workspace_bytes(int m, int md, int B, const int* Ks, int nK) {
  if (!batch_ok(m, md, B, Ks, nK, GMMF_MDMAX, true)) return 0;
  return layout<State>(prob_doubles, m, md, B, Ks, nK, nullptr, nullptr);
}

extern "C" int cc_gmm_full_start(const double* Xb, const int* idx, int B, int m, int md, const int* Ks, int nK,
                                 const uint8_t* init_labels, int64_t n, int64_t ldl, int col_begin, double reg_covar,
                                 void* workspace, size_t ws_bytes, void* stream) {
  Args a;
  if (!enter(&a, idx && init_labels && n >= m && columns_ok(col_begin, B, ldl) && reg_covar >= 0.0, Xb, m, md, B, Ks,
             nK, workspace, ws_bytes,
             "cc_gmm_full_start: bad arguments (1 <= K <= min(m, 127), md <= 128, at most 127 values of K, "
             "B * nK <= 65535)"))
    return CC_ERR_ARG;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(workspace, 0, HEADER, st) != hipSuccess) return launch_error("cc_gmm_full_start");
  const int chunks = (m + GT - 1) / GT;
  hipLaunchKernelGGL(gmm_onehot<Args>, dim3(chunks < 64 ? chunks : 64, B * nK), dim3(GT), 0, st, a, idx, init_labels, n,
                     ldl, col_begin);
  const int rc = launch_mstep(a, Ks, nK, 1, reg_covar, st, "cc_gmm_full_start");
  return rc != CC_OK ? rc : launch_error("cc_gmm_full_start");
}

extern "C" int cc_gmm_full_em_step(const double* Xb, int B, int m, int md, const int* Ks, int nK, double tol,
                                   double reg_covar, int max_iter, void* workspace, size_t ws_bytes, void* stream) {
  Args a;
  if (!enter(&a, tol >= 0.0 && reg_covar >= 0.0 && max_iter >= 1, Xb, m, md, B, Ks, nK, workspace, ws_bytes,
             "cc_gmm_full_em_step: bad arguments"))
    return CC_ERR_ARG;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(a.word, 0, sizeof(int), st) != hipSuccess) return launch_error("cc_gmm_full_em_step");
  int rc = launch_estep<0>(a, Ks, nK, st, nullptr, nullptr, 0, 0, 0, "cc_gmm_full_em_step");
  if (rc != CC_OK) return rc;
  hipLaunchKernelGGL(gmm_decide<Args>, dim3((B * nK + GW - 1) / GW), dim3(GT), 0, st, a, tol, max_iter);
  rc = launch_mstep(a, Ks, nK, 0, reg_covar, st, "cc_gmm_full_em_step");
  return rc != CC_OK ? rc : launch_error("cc_gmm_full_em_step");
}

extern "C" int cc_gmm_full_finish(const double* Xb, const int* idx, int B, int m, int md, const int* Ks, int nK,
                                  int keep_best, int h_begin, uint8_t* labels, int64_t n, int64_t ldl,
                                  double* lower_bound, int* n_iter, uint8_t* converged, int64_t ldo, void* workspace,
                                  size_t ws_bytes, void* stream) {
  Args a;
  if (!enter(&a, idx && labels && n >= m && columns_ok(h_begin, B, ldl) &&
                 (!(lower_bound || n_iter || converged) || columns_ok(h_begin, B, ldo)),
             Xb, m, md, B, Ks, nK, workspace, ws_bytes, "cc_gmm_full_finish: bad arguments"))
    return CC_ERR_ARG;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(gmm_pick<Args>, dim3((B * nK + GT - 1) / GT), dim3(GT), 0, st, a, keep_best, h_begin, lower_bound,
                     n_iter, converged, ldo);
  const int rc = launch_estep<1>(a, Ks, nK, st, idx, labels, n, ldl, h_begin, "cc_gmm_full_finish");
  return rc != CC_OK ? rc : launch_error("cc_gmm_full_finish");
}
