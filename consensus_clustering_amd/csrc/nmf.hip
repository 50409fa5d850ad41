// K14: batched multiplicative updates for the NMF base clusterer (nmf.py).
//
// A batch is B resamples x nK values of K = B * nK problems over the compact float64 rows
// Xb [B][m][md], X ~ W H with W [m][Kp] and H [Kp][md], Kp = K rounded up to 16 and
// the padding kept at 0.  One iteration of every active problem is two launches, ordered by the
// stream:
//   nmf_wstep   (row chunks x problems) one wave per 16-row tile: X H^T (inner length md) and
//               W (H H^T) (inner length K) of the tile, then W *= (X H^T) / (W (H H^T))
//   nmf_hstep   one workgroup per problem: W^T W and W^T X (inner length m), then per 16-column slab
//               (W^T W) H (inner length K) and H *= (W^T X) / ((W^T W) H), then H H^T (inner length
//               md) for the next W step and for the label rule
// At an iteration that is a multiple of 10 (tol > 0), and at max_iter, two more:
//   nmf_resid   (row chunks x problems) one wave per 16-row tile: the tile's sum of (X - W H)^2
//   nmf_decide  one wave per problem: the error from the tile sums and sklearn's stopping test
// Every contraction runs on v_mfma_f64_16x16x4_f64.  A denominator equal to 0 becomes float32's
// epsilon; each update is a division, then a multiplication (two roundings, contract off).
// sklearn's multi_dot picks W^T (W H) where md is very small; this file always forms (W^T W) H.
//
// Order of every sum (none depends on the grid, the batch or which workgroup ran first; no
// floating-point atomic anywhere):
//   GEMM chains   v_mfma_f64_16x16x4_f64 accumulates the sequential FMA chain over its inner index
//                 (see kmeans_f64.hip): j = 0 .. md - 1 for X H^T and H H^T, k = 0 .. K - 1 (then
//                 zero padding up to a multiple of 4) for W (H H^T), (W^T W) H and W H,
//                 r = 0 .. m - 1 for W^T X and W^T W, uncut
//   mean of X     thread t of 256 adds the elements t, t + 256, .. of the resample's [m][md] rows in
//                 order, then a halving tree over the 256 sums in LDS
//   error         per 16-row tile lane (q, c) adds, for the column slabs in order, its rows q, q + 4,
//                 q + 8, q + 12 at column c, then a butterfly over the 64 lanes; per problem lane l
//                 adds tiles l, l + 64, .. in order, then a butterfly over the 64 lanes
//
// The batch frame is batch_shared.hpp's: the arguments, the workspace layout and header, the row
// grid and the tile sums.  cc_gmm_gather (gmm.hip) fills Xb, and cc_gmm_active reads the two header
// words of this workspace as of the mixtures': both serve every row-batch clusterer under the
// names they got first.
#include "batch_shared.hpp"

namespace {

constexpr double NMF_EPS = 1.1920928955078125e-07;  // np.finfo(np.float32).eps

struct NState {
  double err0, prev, err, best;  // the error at init, at the last test, the last computed; the best init's
  int n_iter, active, converged, win;
};

using Args = BatchArgs<NState>;

// the arrays of one problem, in this order: W [m][Kp], H [Kp][md], HHt [Kp][Kp], WtW [Kp][Kp],
// num [Kp][md] (W^T X), part [ceil(m / 16)]
struct Prob {
  double *W, *H, *HHt, *WtW, *num, *part;
  int K, Kp;
};

__host__ __device__ inline size_t prob_doubles(int m, int md, int K) {
  const size_t Kp = pad16(K);
  return static_cast<size_t>(m) * Kp + 2 * Kp * static_cast<size_t>(md) + 2 * Kp * Kp +
         static_cast<size_t>((m + 15) / 16);
}

__device__ inline Prob prob(const Args& a, int b, int k) {
  Prob p;
  p.K = a.Ks[k];
  p.Kp = pad16(p.K);
  const size_t Kp = p.Kp, md = a.md;
  p.W = reinterpret_cast<double*>(a.base + static_cast<size_t>(b) * a.per_b + a.off[k]);
  p.H = p.W + static_cast<size_t>(a.m) * Kp;
  p.HHt = p.H + Kp * md;
  p.WtW = p.HHt + Kp * Kp;
  p.num = p.WtW + Kp * Kp;
  p.part = p.num + Kp * md;
  return p;
}

// H H^T [Kp][Kp] of one problem, one wave per 16 x 16 tile; the whole workgroup calls it
__device__ inline void hht_tiles(const Prob& pr, int md) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, q = lane >> 4;
  const int Kp = pr.Kp, nct = Kp >> 4, S = md >> 2;
  for (int job = wave; job < nct * nct; job += GW) {
    const int c1 = job / nct, c2 = job % nct;
    const double* ap = pr.H + static_cast<size_t>(c1 * 16 + lr) * md;
    const double* bp = pr.H + static_cast<size_t>(c2 * 16 + lr) * md;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < S; ++s) acc = mfma(ap[4 * s + q], bp[4 * s + q], acc);
    if (md & 3) {  // the last, partial step of 4
      const int j = 4 * S + q;
      const bool in = j < md;
      acc = mfma(in ? ap[j] : 0.0, in ? bp[j] : 0.0, acc);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) pr.HHt[static_cast<size_t>(c1 * 16 + q + 4 * i) * Kp + c2 * 16 + lr] = acc[i];
  }
}

// one init of every problem: avg = sqrt(mean(X) / K), W = avg |N_W|, H = avg |N_H| (the normals
// [m][K] and [K][md] per K, concatenated, shared by the resamples), H H^T and the state
__global__ __launch_bounds__(GT) void nmf_init(Args a, const double* __restrict__ NW, const double* __restrict__ NH) {
  __shared__ double red[GT];
  const int p = blockIdx.x, b = p / a.nK, k = p % a.nK, tid = threadIdx.x;
  const Prob pr = prob(a, b, k);
  const int K = pr.K, Kp = pr.Kp, m = a.m, md = a.md;
  const size_t cnt = static_cast<size_t>(m) * md;
  const double* Xb = a.Xb + static_cast<size_t>(b) * cnt;
  double t = 0.0;
  for (size_t e = tid; e < cnt; e += GT) t += Xb[e];
  red[tid] = t;
  __syncthreads();
  for (int o = GT / 2; o >= 1; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const double avg = sqrt((red[0] / static_cast<double>(cnt)) / K);
  size_t kw = 0;  // the components before this K
  for (int i = 0; i < k; ++i) kw += a.Ks[i];
  const double* nw = NW + kw * m;
  const double* nh = NH + kw * md;
  for (size_t e = tid; e < static_cast<size_t>(m) * Kp; e += GT) {
    const size_t r = e / Kp;
    const int c = static_cast<int>(e % Kp);
    pr.W[e] = c < K ? avg * nw[r * K + c] : 0.0;
  }
  for (size_t e = tid; e < static_cast<size_t>(Kp) * md; e += GT) pr.H[e] = e < static_cast<size_t>(K) * md ? avg * nh[e] : 0.0;
  if (tid == 0) {
    NState& s = a.st[p];
    s.err0 = s.prev = s.err = 0.0;
    s.n_iter = 0;
    s.active = 1;
    s.converged = s.win = 0;
  }
  __syncthreads();
  hht_tiles(pr, md);
}

// W *= (X H^T) / (W (H H^T)) of the active problems, one wave per 16-row tile
__global__ __launch_bounds__(GT) void nmf_wstep(Args a) {
  extern __shared__ double lds[];
  const int p = blockIdx.y, b = p / a.nK, k = p % a.nK;
  if (!a.st[p].active) return;  // uniform over the workgroup
  const Prob pr = prob(a, b, k);
  const int K = pr.K, Kp = pr.Kp, nct = Kp >> 4, m = a.m, md = a.md;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, q = lane >> 4;
  const int ntile = (m + 15) >> 4;
  double* wt = lds + static_cast<size_t>(wave) * Kp * 16;  // [comp][16 rows]: this wave's tile of the old W
  const double* Xb = a.Xb + static_cast<size_t>(b) * m * md;
  const int S = md >> 2, SK = (K + 3) >> 2;
  for (int t0 = blockIdx.x * GW; t0 < ntile; t0 += gridDim.x * GW) {  // the same trips for every wave
    const int tile = t0 + wave;
    const bool valid = tile < ntile;
    for (int e = lane; e < 16 * Kp; e += 64) {
      const int r = e / Kp, c = e % Kp;
      const int row = tile * 16 + r;
      wt[c * 16 + r] = valid && row < m ? pr.W[static_cast<size_t>(row) * Kp + c] : 0.0;
    }
    __syncthreads();
    const int row = tile * 16 + lr;
    const bool rin = valid && row < m;
    const double* xr = Xb + static_cast<size_t>(rin ? row : 0) * md;
    for (int ct = 0; ct < nct; ++ct) {
      // rows of the tile x components ct * 16 .. + 15: acc[i] is row q + 4 i, component lr
      f64x4 num = {0.0, 0.0, 0.0, 0.0}, den = {0.0, 0.0, 0.0, 0.0};
      const double* hp = pr.H + static_cast<size_t>(ct * 16 + lr) * md;
      for (int s = 0; s < S; ++s) {
        const int j = 4 * s + q;
        num = mfma(rin ? xr[j] : 0.0, hp[j], num);
      }
      if (md & 3) {  // the last, partial step of 4
        const int j = 4 * S + q;
        const bool in = j < md;
        num = mfma(in && rin ? xr[j] : 0.0, in ? hp[j] : 0.0, num);
      }
      const double* gp = pr.HHt + ct * 16 + lr;
      for (int s = 0; s < SK; ++s) {
        const int kk = 4 * s + q;  // below Kp: the padding of the old W and of H H^T is 0
        den = mfma(wt[kk * 16 + lr], gp[static_cast<size_t>(kk) * Kp], den);
      }
      const int c = ct * 16 + lr;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int rl = q + 4 * i, grow = tile * 16 + rl;
        double d = den[i];
        if (d == 0.0) d = NMF_EPS;
        const double delta = num[i] / d;
        if (valid && grow < m && c < K) pr.W[static_cast<size_t>(grow) * Kp + c] = wt[c * 16 + rl] * delta;
      }
    }
    __syncthreads();
  }
}

// W^T W, W^T X, H *= (W^T X) / ((W^T W) H), H H^T and the iteration count of the active problems
__global__ __launch_bounds__(GT) void nmf_hstep(Args a) {
  extern __shared__ double lds[];
  const int p = blockIdx.x, b = p / a.nK, k = p % a.nK;
  if (!a.st[p].active) return;  // uniform over the workgroup
  const Prob pr = prob(a, b, k);
  const int K = pr.K, Kp = pr.Kp, nct = Kp >> 4, m = a.m, md = a.md;
  const int nft = (md + 15) >> 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, q = lane >> 4;
  const double* Xb = a.Xb + static_cast<size_t>(b) * m * md;
  const int S = m >> 2, SK = (K + 3) >> 2;
  // jobs 0 .. nct * nct - 1: the tiles of W^T W; then the tiles of W^T X.  acc[i] is component
  // ct * 16 + q + 4 i, column (or second component) lr of its tile
  for (int job = wave; job < nct * (nct + nft); job += GW) {
    const bool ww = job < nct * nct;
    const int ct = ww ? job / nct : (job - nct * nct) / nft;
    const int ot = ww ? job % nct : (job - nct * nct) % nft;
    const int j = ot * 16 + lr;
    const bool jin = ww || j < md;
    const double* ap = pr.W + ct * 16 + lr;
    const double* bp = ww ? pr.W + j : Xb + (jin ? j : 0);
    const size_t ldb = ww ? Kp : md;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < S; ++s) {
      const size_t r = 4 * s + q;
      const double bv = bp[r * ldb];
      acc = mfma(ap[r * Kp], jin ? bv : 0.0, acc);
    }
    if (m & 3) {  // the last, partial step of 4
      const size_t r = 4 * S + q;
      const bool in = r < static_cast<size_t>(m);
      acc = mfma(in ? ap[r * Kp] : 0.0, in && jin ? bp[r * ldb] : 0.0, acc);
    }
    if (jin) {
      double* out = ww ? pr.WtW : pr.num;
#pragma unroll
      for (int i = 0; i < 4; ++i) out[static_cast<size_t>(ct * 16 + q + 4 * i) * ldb + j] = acc[i];
    }
  }
  __syncthreads();
  double* ht = lds + static_cast<size_t>(wave) * Kp * 16;  // [comp][16 columns]: this wave's slab of the old H
  for (int f0 = 0; f0 < nft; f0 += GW) {  // the same trips for every wave
    const int ft = f0 + wave;
    const int j = ft * 16 + lr;
    const bool jin = ft < nft && j < md;
    for (int e = lane; e < 16 * Kp; e += 64) {
      const int c = e >> 4;
      ht[e] = jin ? pr.H[static_cast<size_t>(c) * md + j] : 0.0;  // e & 15 == lr
    }
    __syncthreads();
    for (int ct = 0; ct < nct; ++ct) {
      f64x4 den = {0.0, 0.0, 0.0, 0.0};
      const double* gp = pr.WtW + static_cast<size_t>(ct * 16 + lr) * Kp;
      for (int s = 0; s < SK; ++s) {
        const int kk = 4 * s + q;  // below Kp: the padding of W^T W and of the old H is 0
        den = mfma(gp[kk], ht[kk * 16 + lr], den);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = ct * 16 + q + 4 * i;
        double d = den[i];
        if (d == 0.0) d = NMF_EPS;
        if (jin && c < K) {
          const double delta = pr.num[static_cast<size_t>(c) * md + j] / d;
          pr.H[static_cast<size_t>(c) * md + j] = ht[c * 16 + lr] * delta;
        }
      }
    }
    __syncthreads();
  }
  hht_tiles(pr, md);
  if (tid == 0) a.st[p].n_iter += 1;
}

// the sum of (X - W H)^2 over every 16-row tile of the active problems (all: of every problem)
__global__ __launch_bounds__(GT) void nmf_resid(Args a, int all) {
  const int p = blockIdx.y, b = p / a.nK, k = p % a.nK;
  if (!all && !a.st[p].active) return;  // uniform over the workgroup
  const Prob pr = prob(a, b, k);
  const int K = pr.K, Kp = pr.Kp, m = a.m, md = a.md;
  const int nft = (md + 15) >> 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, q = lane >> 4;
  const int ntile = (m + 15) >> 4;
  const double* Xb = a.Xb + static_cast<size_t>(b) * m * md;
  const int SK = (K + 3) >> 2;
  for (int tile = blockIdx.x * GW + wave; tile < ntile; tile += gridDim.x * GW) {
    const int row = tile * 16 + lr;
    const bool rin = row < m;
    const double* wp = pr.W + static_cast<size_t>(rin ? row : 0) * Kp;
    double sum = 0.0;
    for (int ft = 0; ft < nft; ++ft) {
      const int j = ft * 16 + lr;
      const bool jin = j < md;
      const double* hp = pr.H + (jin ? j : 0);
      f64x4 acc = {0.0, 0.0, 0.0, 0.0};
      for (int s = 0; s < SK; ++s) {
        const int kk = 4 * s + q;  // below Kp: the padding of W and of H is 0
        const double wv = wp[kk], hv = hp[static_cast<size_t>(kk) * md];
        acc = mfma(rin ? wv : 0.0, jin ? hv : 0.0, acc);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int grow = tile * 16 + q + 4 * i;
        if (grow < m && jin) {
          const double dd = Xb[static_cast<size_t>(grow) * md + j] - acc[i];
          sum += dd * dd;
        }
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) pr.part[tile] = sum;
  }
}

// one wave per problem.  init: the error at init.  Otherwise, for a problem still active: at an
// iteration that is a multiple of 10 (tol > 0) sklearn's test on the error, then max_iter; the
// problems that go on are counted in the header word
__global__ __launch_bounds__(GT) void nmf_decide(Args a, int init, double tol, int max_iter) {
  const int p = blockIdx.x * GW + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= a.B * a.nK) return;
  NState& s = a.st[p];
  if (!s.active) return;
  const Prob pr = prob(a, p / a.nK, p % a.nK);
  const double err = sqrt(sum_parts(pr.part, (a.m + 15) >> 4));
  if (lane != 0) return;
  s.err = err;
  if (init) {
    s.err0 = s.prev = err;
  } else if (tol > 0.0 && s.n_iter % 10 == 0) {
    const double gain = (s.prev - err) / s.err0;
    if (gain < tol) {  // false for a NaN ratio, as in sklearn
      s.converged = 1;
      s.active = 0;
    } else {
      s.prev = err;
    }
  }
  if (s.active && !init && s.n_iter >= max_iter) s.active = 0;
  if (s.active) atomicAdd(a.word, 1);
}

// one wave per problem: the final error, whether this init wins, and the winners' scalar outputs
__global__ __launch_bounds__(GT) void nmf_pick(Args a, int keep_best, int h_begin, double* reconstruction_err,
                                               int* n_iter, uint8_t* converged, int64_t ldo) {
  const int p = blockIdx.x * GW + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= a.B * a.nK) return;
  NState& s = a.st[p];
  const Prob pr = prob(a, p / a.nK, p % a.nK);
  const double err = sqrt(sum_parts(pr.part, (a.m + 15) >> 4));
  if (lane != 0) return;
  s.err = err;
  const bool win = !keep_best || err < s.best;
  s.win = win;
  if (!win) return;
  s.best = err;
  put_scalars(a, p, h_begin, ldo, reconstruction_err, err, n_iter, converged);
}

// the labels of the problems whose init won: argmax_k W[r][k] sqrt((H H^T)[k][k]), first index
__global__ __launch_bounds__(GT) void nmf_label(Args a, const int* __restrict__ idx, uint8_t* __restrict__ labels,
                                                int64_t n, int64_t ldl, int h_begin) {
  __shared__ double norm[128];
  const int p = blockIdx.y, b = p / a.nK, k = p % a.nK;
  if (!a.st[p].win) return;  // uniform over the workgroup
  const Prob pr = prob(a, b, k);
  const int K = pr.K, Kp = pr.Kp;
  if (threadIdx.x < 128) norm[threadIdx.x] = threadIdx.x < K ? sqrt(pr.HHt[static_cast<size_t>(threadIdx.x) * (Kp + 1)]) : 0.0;
  __syncthreads();
  uint8_t* L = labels + static_cast<size_t>(k) * n * ldl + h_begin + b;
  for (int r = blockIdx.x * GT + threadIdx.x; r < a.m; r += gridDim.x * GT) {
    const double* wp = pr.W + static_cast<size_t>(r) * Kp;
    double best = -INFINITY;
    int bi = 0;
    for (int c = 0; c < K; ++c) {
      const double v = wp[c] * norm[c];
      if (v > best) {
        best = v;
        bi = c;
      }
    }
    const int item = idx[static_cast<size_t>(b) * a.m + r];
    if (item >= 0 && item < n) L[static_cast<int64_t>(item) * ldl] = static_cast<uint8_t>(bi);
  }
}

constexpr int MD_MAX = 1 << 20;

// batch_enter for this file's problems; K may exceed m and md
bool enter(Args* a, bool ok, const double* Xb, int m, int md, int B, const int* Ks, int nK, void* ws, size_t ws_bytes,
           const char* error) {
  return batch_enter(a, prob_doubles, MD_MAX, false, ok, Xb, m, md, B, Ks, nK, ws, ws_bytes, error);
}

}  // namespace

extern "C" size_t cc_nmf_workspace_bytes(int m, int md, int B, const int* Ks, int nK) {
  if (!batch_ok(m, md, B, Ks, nK, MD_MAX, false)) return 0;
  return layout<NState>(prob_doubles, m, md, B, Ks, nK, nullptr, nullptr);
}

extern "C" int cc_nmf_start(const double* Xb, int B, int m, int md, const int* Ks, int nK, const double* normals_w,
                            const double* normals_h, void* workspace, size_t ws_bytes, void* stream) {
  Args a;
  if (!enter(&a, normals_w && normals_h, Xb, m, md, B, Ks, nK, workspace, ws_bytes,
             "cc_nmf_start: bad arguments (1 <= K <= 127, at most 127 values of K, B * nK <= 65535)"))
    return CC_ERR_ARG;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(workspace, 0, HEADER, st) != hipSuccess) return launch_error("cc_nmf_start");
  hipLaunchKernelGGL(nmf_init, dim3(B * nK), dim3(GT), 0, st, a, normals_w, normals_h);
  hipLaunchKernelGGL(nmf_resid, row_grid(m, B, nK), dim3(GT), 0, st, a, 1);
  hipLaunchKernelGGL(nmf_decide, dim3((B * nK + GW - 1) / GW), dim3(GT), 0, st, a, 1, 0.0, 0);
  return launch_error("cc_nmf_start");
}

extern "C" int cc_nmf_steps(const double* Xb, int B, int m, int md, const int* Ks, int nK, int first, int count,
                            double tol, int max_iter, void* workspace, size_t ws_bytes, void* stream) {
  Args a;
  if (!enter(&a, first >= 1 && count >= 0 && tol >= 0.0 && max_iter >= 1, Xb, m, md, B, Ks, nK, workspace, ws_bytes,
             "cc_nmf_steps: bad arguments"))
    return CC_ERR_ARG;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t lds = tile_lds(Ks, nK);
  for (int it = first; it < first + count && it <= max_iter; ++it) {
    hipLaunchKernelGGL(nmf_wstep, row_grid(m, B, nK), dim3(GT), lds, st, a);
    hipLaunchKernelGGL(nmf_hstep, dim3(B * nK), dim3(GT), lds, st, a);
    if ((tol > 0.0 && it % 10 == 0) || it == max_iter) {
      if (hipMemsetAsync(a.word, 0, sizeof(int), st) != hipSuccess) return launch_error("cc_nmf_steps");
      hipLaunchKernelGGL(nmf_resid, row_grid(m, B, nK), dim3(GT), 0, st, a, 0);
      hipLaunchKernelGGL(nmf_decide, dim3((B * nK + GW - 1) / GW), dim3(GT), 0, st, a, 0, tol, max_iter);
    }
  }
  return launch_error("cc_nmf_steps");
}

extern "C" int cc_nmf_finish(const double* Xb, const int* idx, int B, int m, int md, const int* Ks, int nK,
                             int keep_best, int h_begin, uint8_t* labels, int64_t n, int64_t ldl,
                             double* reconstruction_err, int* n_iter, uint8_t* converged, int64_t ldo, void* workspace,
                             size_t ws_bytes, void* stream) {
  Args a;
  if (!enter(&a, idx && labels && n >= 1 && columns_ok(h_begin, B, ldl) &&
                 (!(reconstruction_err || n_iter || converged) || columns_ok(h_begin, B, ldo)),
             Xb, m, md, B, Ks, nK, workspace, ws_bytes, "cc_nmf_finish: bad arguments"))
    return CC_ERR_ARG;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(nmf_resid, row_grid(m, B, nK), dim3(GT), 0, st, a, 1);
  hipLaunchKernelGGL(nmf_pick, dim3((B * nK + GW - 1) / GW), dim3(GT), 0, st, a, keep_best, h_begin, reconstruction_err,
                     n_iter, converged, ldo);
  const int chunks = (m + GT - 1) / GT;
  hipLaunchKernelGGL(nmf_label, dim3(chunks < 64 ? chunks : 64, B * nK), dim3(GT), 0, st, a, idx, labels, n, ldl,
                     h_begin);
  return launch_error("cc_nmf_finish");
}
