// What the diagonal (gmm.hip, K12) and the full-covariance (gmm_full.hip, K13) mixture kernels
// share on top of the batch frame (batch_shared.hpp): the per-problem State, the one-hot start, the
// row tail of the E-step from the weighted log probabilities of a 16-row tile onward, and the
// decide and pick kernels.
//
// A translation unit that includes this file defines, in its own unnamed namespace,
//   struct Prob { double *resp, *part; int K, Kp; ... };   // the arrays of one problem
//   __device__ Prob prob(const Args& a, int b, int k);
// The kernels below find it when they are instantiated.
//
// Order of the sums made here (none depends on the grid, the batch or which workgroup ran first;
// no floating-point atomic anywhere):
//   logsumexp     per row, lane q = 0..3 adds its components q, q + 4, .. in order, then (q0 + q1) +
//                 (q2 + q3)
//   lower bound   per 16-row tile rows 0..15 in order; per problem sum_parts (batch_shared.hpp)
#pragma once

#include "batch_shared.hpp"

namespace {

struct State {
  double prev, lower, best;  // the bound before and after the last E-step; the best init's so far
  int n_iter, active, converged, failed, win, mrun;
};

using Args = BatchArgs<State>;

// the one-hot responsibilities of every problem from the init labels, and the state reset
template <class A>
__global__ __launch_bounds__(GT) void gmm_onehot(A a, const int* __restrict__ idx, const uint8_t* __restrict__ lab,
                                                 int64_t n, int64_t ldl, int col_begin) {
  const int p = blockIdx.y, b = p / a.nK, k = p % a.nK;
  const auto pr = prob(a, b, k);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    State& s = a.st[p];
    s.prev = s.lower = -INFINITY;
    s.n_iter = 0;
    s.active = 1;
    s.converged = s.failed = s.win = s.mrun = 0;
  }
  const uint8_t* L = lab + static_cast<size_t>(k) * n * ldl + col_begin + b;
  for (int r = blockIdx.x * GT + threadIdx.x; r < a.m; r += gridDim.x * GT) {
    const int item = idx[static_cast<size_t>(b) * a.m + r];
    const int l = item >= 0 && item < n ? L[static_cast<int64_t>(item) * ldl] : 0xFF;
    double* row = pr.resp + static_cast<size_t>(r) * pr.Kp;
    for (int c = 0; c < pr.Kp; ++c) row[c] = c == l ? 1.0 : 0.0;
  }
}

// The row tail of one wave's 16-row tile.  wl [Kp][16] holds the weighted log probabilities of the
// tile (component c, row lr at wl[c * 16 + lr]; -inf for c >= K), written before the caller's
// barrier.  MODE 0: scipy's logsumexp of every row, the responsibilities resp [m][Kp] and the
// tile's sum of the row log-norms part[tile]; MODE 1: the label of every row (argmax of the log
// responsibilities, first index) at labels[lab0 + item * ldl] with item = idxb[row].  valid: the
// tile exists (tile * 16 < m).  The whole wave calls it.
template <int MODE>
__device__ inline void gmm_row_tail(const double* wl, int K, int Kp, int m, int tile, bool valid, double* resp,
                                    double* part, const int* __restrict__ idxb, uint8_t* __restrict__ labels,
                                    size_t lab0, int64_t n, int64_t ldl) {
  const int lane = threadIdx.x & 63, lr = lane & 15, q = lane >> 4;
  const int nct = Kp >> 4;
  const int row = tile * 16 + lr;
  const bool rin = valid && row < m;
  // row lr, components q, q + 4, ..
  double mx = -INFINITY;
  for (int c = q; c < Kp; c += 4) mx = fmax(mx, wl[c * 16 + lr]);
  mx = fmax(mx, __shfl_xor(mx, 16));
  mx = fmax(mx, __shfl_xor(mx, 32));
  double sum = 0.0;
  int cnt = 0;
  for (int c = q; c < Kp; c += 4) {
    const double v = wl[c * 16 + lr];
    if (v == mx)
      ++cnt;
    else
      sum += exp(v - mx);
  }
  cnt += __shfl_xor(cnt, 16);
  cnt += __shfl_xor(cnt, 32);
  sum += __shfl_xor(sum, 16);
  sum += __shfl_xor(sum, 32);
  if (sum != 0.0) sum = sum / cnt;
  const double ln = (log1p(sum) + log(static_cast<double>(cnt))) + mx;
  if (MODE == 0) {
    // component ct * 16 + lr, rows q, q + 4, ..: 128-byte pieces of resp
    for (int i = 0; i < 4; ++i) {
      const int rl = q + 4 * i;
      const double lnr = __shfl(ln, rl);
      const int grow = tile * 16 + rl;
      for (int ct = 0; ct < nct; ++ct) {
        const int c = ct * 16 + lr;
        const double r = exp(wl[c * 16 + rl] - lnr);
        if (valid && grow < m) resp[static_cast<size_t>(grow) * Kp + c] = c < K ? r : 0.0;
      }
    }
    double t = 0.0;
    for (int r = 0; r < 16; ++r) {
      const double v = __shfl(ln, r);
      if (tile * 16 + r < m) t += v;
    }
    if (valid && lane == 0) part[tile] = t;
  } else {
    double best = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = q; c < K; c += 4) {
      const double v = wl[c * 16 + lr] - ln;
      if (v > best) {
        best = v;
        bi = c;
      }
    }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const double b2 = __shfl_xor(best, o);
      const int i2 = __shfl_xor(bi, o);
      if (b2 > best || (b2 == best && i2 < bi)) {
        best = b2;
        bi = i2;
      }
    }
    if (bi == 0x7fffffff) bi = 0;
    if (rin && q == 0) {
      const int item = idxb[row];
      if (item >= 0 && item < n) labels[lab0 + static_cast<int64_t>(item) * ldl] = static_cast<uint8_t>(bi);
    }
  }
}

// one wave per problem: the bound of the E-step just run, and what it decides
template <class A>
__global__ __launch_bounds__(GT) void gmm_decide(A a, double tol, int max_iter) {
  const int p = blockIdx.x * GW + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= a.B * a.nK) return;
  State& s = a.st[p];
  if (!s.active) {
    if (lane == 0) s.mrun = 0;
    return;
  }
  const auto pr = prob(a, p / a.nK, p % a.nK);
  const double t = sum_parts(pr.part, (a.m + 15) >> 4);
  if (lane == 0) {
    const double lower = t / a.m;
    const double change = lower - s.prev;
    s.lower = s.prev = lower;
    s.n_iter += 1;
    s.mrun = 1;
    if (fabs(change) < tol) {
      s.converged = 1;
      s.active = 0;
    } else if (s.n_iter >= max_iter) {
      s.active = 0;
    } else {
      atomicAdd(a.word, 1);
    }
  }
}

// which problems this init wins, and their scalar outputs
template <class A>
__global__ __launch_bounds__(GT) void gmm_pick(A a, int keep_best, int h_begin, double* lower_bound, int* n_iter,
                                               uint8_t* converged, int64_t ldo) {
  const int p = blockIdx.x * GT + threadIdx.x;
  if (p >= a.B * a.nK) return;
  State& s = a.st[p];
  const bool win = !keep_best || s.lower > s.best || s.best == -INFINITY;
  s.win = win;
  if (!win) return;
  s.best = s.lower;
  put_scalars(a, p, h_begin, ldo, lower_bound, s.lower, n_iter, converged);
}

// the problem failed (sklearn's "ill-defined empirical covariance"): the batch is refused
__device__ inline void gmm_mark_failed(int* word, State& s) {
  if (!s.failed) atomicAdd(word + 1, 1);
  s.failed = 1;
  s.active = 0;
}

}  // namespace
