// Pairwise agreement of label columns on gfx950: the four contingency sums behind the adjusted
// Rand and Jaccard indices of every pair (column of group A, column of group B), from the labels
// alone (Ben-Hur, Elisseeff & Guyon 2002: how well two resamples agree on the items both drew).
//
// Formulation.  A label column holds one byte per item: a cluster in [0, K) or "absent".  For the
// columns u (cluster count KA) and v (KB), N[a][b] = #{items with u = a and v = b}, and
//   s0 = sum_ab N[a][b]          s2 = sum_ab N[a][b]^2
//   r2 = sum_a (sum_b N[a][b])^2  c2 = sum_b (sum_a N[a][b])^2
// are sklearn's pair_confusion_matrix of the shared items (C11 = s2 - s0, C01 = c2 - s2,
// C10 = r2 - s2, C00 = s0^2 - C01 - C10 - s2).  With the virtual columns (h, c), c in [0, KP),
// KP the power of two >= max(KA, KB) + 1 (at least 4), channel c < K the one-hot [label == c],
// channel K the membership flag [label present] and the rest 0, the Gram matrix G = OA^T OB,
// contracted over the ITEMS, holds in the KP x KP block of a pair (h1, h2): N in its K x K corner,
// N's row sums in channel KB of B, its column sums in channel KA of A, and s0 at (KA, KB).  It is
// an int8 GEMM with a 0/1 operand on v_mfma_i32_32x32x32_i8, int32 accumulators: exact counts
// (N <= n < 2^31).  The four sums are squares of accumulator elements, added by class in uint64
// (every sum <= s0^2 < 2^62): no second pass over the labels, no floating point.
//
// The item dimension is NOT split across workgroups: the sums are sums of squares of the fully
// contracted counts, and squares are not additive, so one workgroup contracts all n items of
// its tile.
//
// Layout.  The MFMA operand wants 16 consecutive items of one column per lane and the label
// matrices are item-major, so transpose_kernel first writes the columns resample-major into the
// caller's workspace: [H rounded up to 128][n rounded up to 128] bytes, labels >= K, items >= n
// and columns >= H as 0x7F (absent; K <= 127 leaves the value free, and with every byte < 0x80
// the one-hot expansion's byte compare cannot carry between bytes).  The one-hot operand never
// exists in HBM: per super-step of 128 items each of the 512 threads expands the 128 label bytes
// of ONE virtual column of the tile (A side or B side) to 128 one-hot bytes in registers and
// writes them to LDS in MFMA fragment order; the 8 waves (2 x 4, each 128 x 64 outputs) read the
// fragments with ds_read_b128 and issue 32 MFMAs each.
//
// Tiles.  An output tile is 256 x 256 virtual columns; 256 is a multiple of every KP, so a
// pair's block never straddles tiles: one workgroup owns its pairs completely and their sums leave
// with plain stores (no global atomics: bitwise reproducible).  Symmetric mode (A with itself)
// runs the tiles bi <= bj, numbered row-major; an off-diagonal tile also stores the mirrored pair
// with r2 and c2 exchanged.  Otherwise all nbA x nbB tiles run, row-major.
//
// Epilogue.  The operand LDS becomes a table [256 / KP][256 / KP][4] uint64 (128 KiB at KP = 4).
// The four rows (v & 3) of an accumulator register group lie in one pair block, so a thread adds
// them in registers first: X over the rows a < KA and Y for the row a = KA, then at most two LDS
// adds per group, to s2 / c2 (its column b < KB) or r2 / s0 (b = KB).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "ccmi_internal.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int T = CC_TILE;            // 256 virtual columns per tile side
constexpr int NT = 512;               // threads per workgroup (8 waves)
constexpr int KC = 4;                 // 32-item chunks per super-step
constexpr int ITEMS = 32 * KC;        // items per super-step; the workspace rows are padded to it
constexpr int FRAG = 1024;            // one 32x32x32 i8 operand fragment: 64 lanes x 16 B
constexpr int SIDE = 8 * KC * FRAG;   // 8 blocks of 32 virtual columns x 4 chunks = 32 KiB
constexpr int BUF = 2 * SIDE;         // A side + B side
constexpr int LDS_BYTES = 2 * BUF;    // double buffered = 128 KiB
constexpr int HPADA = 128;            // workspace columns are padded to a multiple of 128
constexpr uint32_t ABSENT = 0x7Fu;    // "absent" in the workspace
constexpr int TR = 64;                // transposition tile: 64 items x 64 columns

static_assert((T / 4) * (T / 4) * 4 * 8 <= LDS_BYTES, "the pair table of KP = 4 fits the operand LDS");
static_assert(HPADA % TR == 0 && ITEMS % TR == 0, "the transposition grid covers the workspace exactly");

__host__ __device__ constexpr int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// Row-major number t of the upper triangle (bi <= bj) of nb x nb tiles -> (bi, bj); the same
// numbering as the co-association tiles (coassoc.hip).
__device__ __forceinline__ void tile_coords(int64_t t, int nb, int& bi, int& bj) {
  auto start = [nb](int64_t b) -> int64_t { return b * nb - b * (b - 1) / 2; };
  double a = 2.0 * nb + 1.0;
  int r = static_cast<int>(floor((a - sqrt(a * a - 8.0 * static_cast<double>(t))) * 0.5));
  r = r < 0 ? 0 : (r > nb - 1 ? nb - 1 : r);
  while (r > 0 && start(r) > t) --r;
  while (r + 1 < nb && start(r + 1) <= t) ++r;
  bi = r;
  bj = static_cast<int>(r + (t - start(r)));
}

// src: [n][ld] label bytes (H columns used) -> dst: [Hws][npad], Hws = H rounded up to 128 and
// npad = n rounded up to 128, with everything that is not a label in [0, K) written as ABSENT.
// One 64 x 64 tile per workgroup of 256 threads through LDS: byte reads along the columns (ld
// may be any value, e.g. 1 for a partition), dword writes along the items.
__global__ __launch_bounds__(256) void transpose_kernel(const uint8_t* __restrict__ src, int64_t ld, int H, int K,
                                                        int n, uint8_t* __restrict__ dst, int64_t npad) {
  __shared__ uint8_t tile[TR][TR + 4];  // [column][item], rows 68 B: dword-aligned
  const int tid = threadIdx.x;
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * TR;
  const int h0 = blockIdx.y * TR;
  const int hc = tid & 63, ir = tid >> 6;
#pragma unroll
  for (int r = 0; r < TR / 4; ++r) {
    const int il = ir + 4 * r;
    const int64_t i = i0 + il;
    const int h = h0 + hc;
    uint32_t v = ABSENT;
    if (i < n && h < H) {
      v = src[i * ld + h];
      v = v < static_cast<uint32_t>(K) ? v : ABSENT;
    }
    tile[hc][il] = static_cast<uint8_t>(v);
  }
  __syncthreads();
  const int q = tid & 15, hr = tid >> 4;  // dword q of column hr + 16 r
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int hl = hr + 16 * r;
    const uint32_t v = *reinterpret_cast<const uint32_t*>(&tile[hl][4 * q]);
    *reinterpret_cast<uint32_t*>(dst + (h0 + hl) * npad + i0 + 4 * q) = v;
  }
}

// One 32-item chunk of a thread's virtual column into its fragment at dst: the two 16-B halves
// (items 0-15 and 16-31 of the chunk) lie 512 B apart (lanes 0-31 and 32-63 of the fragment).
__device__ __forceinline__ void store_chunk(char* dst, const uint32_t* o) {
#pragma unroll
  for (int g = 0; g < 2; ++g)
    *reinterpret_cast<uint4*>(dst + g * 512) = make_uint4(o[g * 4 + 0], o[g * 4 + 1], o[g * 4 + 2], o[g * 4 + 3]);
}

// The channel of a virtual column as three masks: with label bytes w (all < 0x80),
// t = (w ^ cmp) + 0x7F7F7F7F has bit 7 of a byte set where the label differs from cmp, and
// ((t >> 7) & keep) ^ flip is [label == c] for a cluster channel (cmp = c), [label != ABSENT]
// for the membership channel (cmp = ABSENT) and 0 for the padding channels.
struct Channel {
  uint32_t cmp, keep, flip;
};

__device__ __forceinline__ Channel channel_of(int c, int K) {
  Channel ch;
  ch.cmp = (c < K ? static_cast<uint32_t>(c) : ABSENT) * 0x01010101u;
  ch.keep = c <= K ? 0x01010101u : 0u;
  ch.flip = c < K ? 0x01010101u : 0u;
  return ch;
}

__device__ __forceinline__ void expand_chunk(const uint32_t* w, const Channel& ch, uint32_t (&o)[8]) {
#pragma unroll
  for (int q = 0; q < 8; ++q) o[q] = ((((w[q] ^ ch.cmp) + 0x7F7F7F7Fu) >> 7) & ch.keep) ^ ch.flip;
}

__device__ __forceinline__ void load_chunk(const uint8_t* p, uint32_t* w) {
  const uint4 v0 = reinterpret_cast<const uint4*>(p)[0];
  const uint4 v1 = reinterpret_cast<const uint4*>(p)[1];
  w[0] = v0.x; w[1] = v0.y; w[2] = v0.z; w[3] = v0.w;
  w[4] = v1.x; w[5] = v1.y; w[6] = v1.z; w[7] = v1.w;
}

// LtA / LtB: the transposed columns of the two groups (LtB == LtA in symmetric mode), rows of
// npad bytes.  sums: [HA][HB][4] uint64.
template <int KP>
__global__ __launch_bounds__(NT, 1) void agreement_kernel(
    const uint8_t* __restrict__ LtA, const uint8_t* __restrict__ LtB, int64_t npad, int HA, int KA, int HB, int KB,
    int symmetric, int nbA, int nbB, int64_t tile_begin, unsigned long long* __restrict__ sums) {
  __shared__ __attribute__((aligned(16))) char lds[LDS_BYTES];
  constexpr int LOG = (KP == 4) ? 2 : (KP == 8) ? 3 : (KP == 16) ? 4 : (KP == 32) ? 5 : (KP == 64) ? 6 : 7;
  static_assert((1 << LOG) == KP, "KP = 4 .. 128, a power of two");
  constexpr int PT = T / KP;  // columns (pairs) per tile side

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 2;  // 0..1 : 128-row half
  const int wc = wave & 3;   // 0..3 : 64-col quarter
  // XCD-aware tile order (as coassoc.hip): blocks b and b + 8 share an XCD, so XCD x gets a
  // contiguous tile range and its CUs share the A-side columns through that XCD's L2.
  const int nblk = static_cast<int>(gridDim.x), bx = static_cast<int>(blockIdx.x);
  const int xq = nblk >> 3, xr = nblk & 7, xcd = bx & 7;
  const int64_t t = tile_begin + xcd * xq + (xcd < xr ? xcd : xr) + (bx >> 3);
  int bi, bj;
  if (symmetric) {
    tile_coords(t, nbA, bi, bj);
  } else {
    bi = static_cast<int>(t / nbB);
    bj = static_cast<int>(t - static_cast<int64_t>(bi) * nbB);
  }

  // Expansion role: one virtual column per thread.  side 0 = tile rows (A), side 1 = tile cols (B).
  // Column h = vcol / KP lies inside the workspace: the workspace holds H rounded up to 128
  // columns and a tile side covers 256 / KP <= 64 of them.
  const int side = tid >> 8;
  const int erow = tid & 255;
  const int vcol = (side ? bj : bi) * T + erow;
  const Channel ch = channel_of(vcol & (KP - 1), side ? KB : KA);
  const uint8_t* rowp = (side ? LtB : LtA) + static_cast<int64_t>(vcol >> LOG) * npad;
  const int erb = erow >> 5, er = erow & 31;
  char* const wbase = lds + side * SIDE + erb * KC * FRAG + er * 16;

  const int nsteps = static_cast<int>(npad / ITEMS);
  v16i acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = v16i{};

  // w: the label bytes of the step after the one being contracted.  Chunk kc of it is expanded
  // in the shadow of chunk kc's MFMAs, and its registers are then reloaded with the same chunk
  // one step further on, so every load has a whole super-step to land.
  uint32_t w[8 * KC];
#pragma unroll
  for (int kc = 0; kc < KC; ++kc) load_chunk(rowp + 32 * kc, w + 8 * kc);
#pragma unroll
  for (int kc = 0; kc < KC; ++kc) {
    uint32_t oc[8];
    expand_chunk(w + 8 * kc, ch, oc);
    store_chunk(wbase + kc * FRAG, oc);
  }
  {
    const uint8_t* p1 = rowp + static_cast<int64_t>(nsteps > 1 ? 1 : 0) * ITEMS;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) load_chunk(p1 + 32 * kc, w + 8 * kc);
  }
  __syncthreads();

  for (int s = 0; s < nsteps; ++s) {
    const char* rb = lds + (s & 1) * BUF;
    char* wb = wbase + ((s + 1) & 1) * BUF;
    // clamped at the end: the last steps re-read the last step's labels, and their one-hot
    // lands in the buffer nobody reads
    const uint8_t* pn = rowp + static_cast<int64_t>((s + 2) < nsteps ? s + 2 : nsteps - 1) * ITEMS;
    v4i a[2][4], b[2][2];
    auto frags = [&](int kc, v4i (&fa)[4], v4i (&fb)[2]) __attribute__((always_inline)) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        fa[mi] = *reinterpret_cast<const v4i*>(rb + ((wr * 4 + mi) * KC + kc) * FRAG + lane * 16);
#pragma unroll
      for (int nj = 0; nj < 2; ++nj)
        fb[nj] = *reinterpret_cast<const v4i*>(rb + SIDE + ((wc * 2 + nj) * KC + kc) * FRAG + lane * 16);
    };
    frags(0, a[0], b[0]);
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      const int cb = kc & 1;
      if (kc + 1 < KC) frags(kc + 1, a[cb ^ 1], b[cb ^ 1]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int nj = 0; nj < 2; ++nj)
          acc[mi][nj] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[cb][mi], b[cb][nj], acc[mi][nj], 0, 0, 0);
      uint32_t oc[8];
      expand_chunk(w + 8 * kc, ch, oc);
      store_chunk(wb + kc * FRAG, oc);
      // compiler barrier: a load moved above the expansion it follows lands in other registers
      // and is copied into w at the end of the step, behind a wait for every load of the step
      asm volatile("" ::: "memory");
      load_chunk(pn + 32 * kc, w + 8 * kc);
      // issue order: each MFMA followed by a few expansion VALU ops, which then execute in
      // that MFMA's shadow instead of after the whole MFMA block
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);  // 5 VALU (one one-hot dword)
      }
      __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);  // the 2 LDS stores
      __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);  // the 2 label loads
    }
    __syncthreads();
  }

  // ---- epilogue: squares by class into the pair table, then plain stores -------------------
  // (the loop's last barrier has passed: nobody reads the operand buffers any more)
  unsigned long long* tab = reinterpret_cast<unsigned long long*>(lds);  // [PT][PT][4] = s0, s2, r2, c2
  for (int e = tid; e < PT * PT * 2; e += NT) reinterpret_cast<uint4*>(lds)[e] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  const int hi = lane >> 5;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int row0 = wr * 128 + mi * 32 + 8 * g + 4 * hi;  // rows row0 .. row0 + 3: one pair
      const int a0 = row0 & (KP - 1);
      if (a0 > KA) continue;  // padding channels of A
#pragma unroll
      for (int nj = 0; nj < 2; ++nj) {
        const int col = wc * 64 + nj * 32 + (lane & 31);
        const int bch = col & (KP - 1);
        if (bch > KB) continue;  // a padding channel of B
        const bool bsum = bch == KB;  // N's row sums: X -> r2, Y -> s0 (not squared)
        unsigned long long X = 0, Y = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned long long v = static_cast<uint32_t>(acc[mi][nj][4 * g + q]);
          const unsigned long long sq = v * v;
          if (a0 + q < KA) X += sq;
          if (a0 + q == KA) Y = bsum ? v : sq;
        }
        unsigned long long* const tp = tab + (static_cast<int64_t>(row0 >> LOG) * PT + (col >> LOG)) * 4;
        if (X) atomicAdd(tp + (bsum ? 2 : 1), X);
        if (Y) atomicAdd(tp + (bsum ? 0 : 3), Y);
      }
    }
  __syncthreads();
  for (int e = tid; e < PT * PT; e += NT) {
    const int p1 = e / PT, p2 = e - p1 * PT;
    const int h1 = bi * PT + p1, h2 = bj * PT + p2;
    if (h1 >= HA || h2 >= HB) continue;
    const unsigned long long s0 = tab[e * 4 + 0], s2 = tab[e * 4 + 1], r2 = tab[e * 4 + 2], c2 = tab[e * 4 + 3];
    unsigned long long* o = sums + (static_cast<int64_t>(h1) * HB + h2) * 4;
    o[0] = s0; o[1] = s2; o[2] = r2; o[3] = c2;
    if (symmetric && bi != bj) {  // the mirrored pair: u and v exchanged
      unsigned long long* m = sums + (static_cast<int64_t>(h2) * HB + h1) * 4;
      m[0] = s0; m[1] = s2; m[2] = c2; m[3] = r2;
    }
  }
}

int channels_padded(int KA, int KB) {
  int kp = 4;
  while (kp < (KA > KB ? KA : KB) + 1) kp <<= 1;
  return kp;
}

bool k_ok(int K) { return K >= 1 && K <= 127; }

int refuse(const char* what) {
  cc::set_error(std::string("cc_agreement_sums: ") + what);
  return CC_ERR_ARG;
}

}  // namespace

extern "C" size_t cc_agreement_workspace_bytes(int n, int HA, int HB) {
  if (n < 1 || HA < 1 || HB < 0) return 0;
  return static_cast<size_t>((round_up(HA, HPADA) + round_up(HB, HPADA)) * round_up(n, ITEMS));
}

extern "C" int64_t cc_agreement_num_tiles(int HA, int HB, int KA, int KB, int symmetric) {
  if (symmetric) {
    HB = HA;
    KB = KA;
  }
  if (HA < 1 || HB < 1 || !k_ok(KA) || !k_ok(KB)) return 0;
  const int kp = channels_padded(KA, KB);
  const int64_t nbA = (static_cast<int64_t>(HA) * kp + T - 1) / T, nbB = (static_cast<int64_t>(HB) * kp + T - 1) / T;
  return symmetric ? nbA * (nbA + 1) / 2 : nbA * nbB;
}

extern "C" int cc_agreement_sums(const int8_t* A_nh, int ldA, int HA, int KA, const int8_t* B_nh, int ldB, int HB,
                                 int KB, int n, int64_t tile_begin, int64_t tile_end, int64_t* sums,
                                 void* workspace, size_t ws_bytes, void* stream) {
  const int symmetric = B_nh == nullptr;
  if (symmetric) {
    ldB = ldA;
    HB = HA;
    KB = KA;
  }
  if (!A_nh || !sums || !workspace) return refuse("A_nh, sums and workspace are required");
  if (!k_ok(KA) || !k_ok(KB)) return refuse("K must be in [1, 127]");
  if (HA < 1 || HB < 1 || n < 1) return refuse("H and n must be at least 1");
  if (ldA < HA || ldB < HB) return refuse("the row stride must hold the H columns");
  if (reinterpret_cast<uintptr_t>(sums) & 7) return refuse("sums must be 8-B aligned");
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return refuse("workspace must be 16-B aligned");
  const int64_t nt = cc_agreement_num_tiles(HA, HB, KA, KB, symmetric);
  if (tile_begin < 0 || tile_end < tile_begin || tile_end > nt) return refuse("tile range outside [0, num_tiles]");
  if (ws_bytes < cc_agreement_workspace_bytes(n, HA, symmetric ? 0 : HB))
    return refuse("workspace smaller than cc_agreement_workspace_bytes(n, HA, HB)");
  const int64_t ntl = tile_end - tile_begin;
  if (ntl == 0) return CC_OK;
  if (ntl > 0x7fffffff) return refuse("too many tiles for one launch");

  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t npad = round_up(n, ITEMS);
  const int64_t hwsA = round_up(HA, HPADA), hwsB = round_up(HB, HPADA);
  if (npad / TR > 0x7fffffff || hwsA / TR > 65535 || hwsB / TR > 65535) return refuse("n or H too large for one launch");
  uint8_t* LtA = static_cast<uint8_t*>(workspace);
  uint8_t* LtB = symmetric ? LtA : LtA + hwsA * npad;
  hipLaunchKernelGGL(transpose_kernel, dim3(static_cast<unsigned>(npad / TR), static_cast<unsigned>(hwsA / TR)),
                     dim3(256), 0, st, reinterpret_cast<const uint8_t*>(A_nh), static_cast<int64_t>(ldA), HA, KA, n, LtA,
                     npad);
  if (!symmetric)
    hipLaunchKernelGGL(transpose_kernel, dim3(static_cast<unsigned>(npad / TR), static_cast<unsigned>(hwsB / TR)),
                       dim3(256), 0, st, reinterpret_cast<const uint8_t*>(B_nh), static_cast<int64_t>(ldB), HB, KB, n,
                       LtB, npad);
  const int kp = channels_padded(KA, KB);
  const int nbA = static_cast<int>((static_cast<int64_t>(HA) * kp + T - 1) / T);
  const int nbB = static_cast<int>((static_cast<int64_t>(HB) * kp + T - 1) / T);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(sums);
  switch (kp) {
#define CC_AG(k) case k: hipLaunchKernelGGL((agreement_kernel<k>), dim3(static_cast<unsigned>(ntl)), dim3(NT), 0, st, \
                                            LtA, LtB, npad, HA, KA, HB, KB, symmetric, nbA, nbB, tile_begin, out); break;
    CC_AG(4) CC_AG(8) CC_AG(16) CC_AG(32) CC_AG(64)
    default: CC_AG(128)
#undef CC_AG
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    cc::set_error(std::string("cc_agreement_sums: ") + hipGetErrorString(e));
    return CC_ERR_HIP;
  }
  return CC_OK;
}
