// The batch frame of the row-batch clusterers (gmm.hip K12, gmm_full.hip K13, nmf.hip K14): a batch
// is B resamples x nK values of K = B * nK problems over the compact float64 rows Xb [B][m][md]
// (cc_gmm_gather).  This file knows nothing about what a problem computes.
//
// The workspace of a batch: a 256-byte header, whose word[0] counts the problems still active and
// word[1] those that failed (cc_gmm_active reads these two words alone, so it serves every such
// workspace), the per-problem states S [B * nK], then per resample the arrays of every K.
//
// Order of the sum made here (it does not depend on the grid, the batch or which workgroup ran
// first; no floating-point atomic anywhere):
//   sum_parts     per problem lane l adds tiles l, l + 64, .. in order, then a butterfly over the
//                 64 lanes
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "ccmi_internal.h"
#include "launch_error.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int GT = 256;  // threads of a workgroup
constexpr int GW = GT / 64;
constexpr int BATCH_KMAX = 127;
constexpr int BATCH_NKMAX = 127;
constexpr int ROW_CHUNKS = 128;  // most workgroups along the rows of one problem
constexpr size_t HEADER = 256;   // word[0]: problems still active, word[1]: problems that failed

using f64x4 = __attribute__((ext_vector_type(4))) double;

template <class S>
struct BatchArgs {
  int m, md, B, nK;
  int Ks[BATCH_NKMAX];
  unsigned long long off[BATCH_NKMAX];  // bytes from a resample's block to the arrays of K index k
  unsigned long long per_b;             // bytes of one resample's block
  int* word;
  S* st;
  char* base;
  const double* Xb;
};

__host__ __device__ inline int pad16(int K) { return (K + 15) & ~15; }
__host__ __device__ inline size_t up256(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

__device__ inline f64x4 mfma(double a, double b, f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// the sum of a problem's tile sums; the whole wave calls it and every lane gets the result
__device__ inline double sum_parts(const double* part, int ntile) {
  const int lane = threadIdx.x & 63;
  double t = 0.0;
  for (int i = lane; i < ntile; i += 64) t += part[i];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o);
  return t;
}

// the scalar outputs [nK][ldo] of problem p = b * nK + k at [k, h_begin + b], each where it is asked
// for: v, and n_iter and converged of the problem's state
template <class S>
__device__ inline void put_scalars(const BatchArgs<S>& a, int p, int h_begin, int64_t ldo, double* value, double v,
                                   int* n_iter, uint8_t* converged) {
  const S& s = a.st[p];
  const int64_t at = static_cast<int64_t>(p % a.nK) * ldo + h_begin + p / a.nK;
  if (value) value[at] = v;
  if (n_iter) n_iter[at] = s.n_iter;
  if (converged) converged[at] = static_cast<uint8_t>(s.converged);
}

// the bounds of a batch: m, md <= md_max, B, the values of K (k_le_m: none above m) and the problem count
bool batch_ok(int m, int md, int B, const int* Ks, int nK, int md_max, bool k_le_m) {
  if (!Ks || m < 1 || m > (1 << 24) || md < 1 || md > md_max || B < 1 || B > 65535 || nK < 1 || nK > BATCH_NKMAX)
    return false;
  for (int k = 0; k < nK; ++k)
    if (Ks[k] < 1 || Ks[k] > BATCH_KMAX || (k_le_m && Ks[k] > m)) return false;
  return static_cast<size_t>(B) * nK <= 65535;  // the problems are a grid's y extent
}

// the workspace: header, the states, then per resample the arrays of every K, where problem
// (m, md, K) takes doubles(m, md, K) doubles
template <class S, class F>
size_t layout(F doubles, int m, int md, int B, const int* Ks, int nK, void* ws, BatchArgs<S>* a) {
  const size_t states = up256(static_cast<size_t>(B) * nK * sizeof(S));
  size_t per_b = 0;
  for (int k = 0; k < nK; ++k) {
    if (a) {
      a->Ks[k] = Ks[k];
      a->off[k] = per_b;
    }
    per_b += up256(8 * doubles(m, md, Ks[k]));
  }
  if (a) {
    a->m = m;
    a->md = md;
    a->B = B;
    a->nK = nK;
    a->per_b = per_b;
    a->word = static_cast<int*>(ws);
    a->st = reinterpret_cast<S*>(static_cast<char*>(ws) + HEADER);
    a->base = static_cast<char*>(ws) + HEADER + states;
    a->Xb = nullptr;
  }
  return HEADER + states + static_cast<size_t>(B) * per_b;
}

// How every entry point that takes a workspace begins: false, with `error` set, unless `ok` (the
// entry's own argument tests), the pointers, the shape and the workspace size hold; else the
// arguments over the workspace and Xb.
template <class S, class F>
bool batch_enter(BatchArgs<S>* a, F doubles, int md_max, bool k_le_m, bool ok, const double* Xb, int m, int md, int B,
                 const int* Ks, int nK, void* ws, size_t ws_bytes, const char* error) {
  if (!ok || !Xb || !ws || !batch_ok(m, md, B, Ks, nK, md_max, k_le_m) ||
      ws_bytes < layout<S>(doubles, m, md, B, Ks, nK, nullptr, nullptr)) {
    cc::set_error(error);
    return false;
  }
  layout(doubles, m, md, B, Ks, nK, ws, a);
  a->Xb = Xb;
  return true;
}

// the columns [begin, begin + B) lie in a row of ld
bool columns_ok(int begin, int B, int64_t ld) { return begin >= 0 && ld >= static_cast<int64_t>(begin) + B; }

int max_kp(const int* Ks, int nK) {
  int v = 0;
  for (int k = 0; k < nK; ++k) v = pad16(Ks[k]) > v ? pad16(Ks[k]) : v;
  return v;
}

// (row chunks x problems): one wave per 16-row tile, at most ROW_CHUNKS workgroups along the rows
dim3 row_grid(int m, int B, int nK) {
  const int ntile = (m + 15) / 16, chunks = (ntile + GW - 1) / GW;
  return dim3(chunks < ROW_CHUNKS ? chunks : ROW_CHUNKS, B * nK);
}

// LDS of a workgroup whose every wave holds a [Kp][16] tile of doubles, Kp the largest of the batch
size_t tile_lds(const int* Ks, int nK) { return static_cast<size_t>(GW) * max_kp(Ks, nK) * 16 * sizeof(double); }

}  // namespace
