/*
 * ccmi.h — C ABI of the MI355X-native consensus-clustering engine (libccmi.so).
 *
 * Plain C: pointers, sizes and a hipStream_t passed as void*.  No C++ or torch
 * types cross this boundary.  Every entry point returns 0 on success and a
 * negative code on error; the message is available from cc_last_error() on the
 * calling thread.  Device pointers are caller-owned (the Python host passes
 * torch-ROCm tensors' data_ptr()); the library allocates nothing on the device.
 * Launches are asynchronous on the given stream and safe to capture in a graph.
 *
 * Each entry point replaces a piece of the reference's hot path
 * (/root/reference/consensus_clustering_parallelised.py, "CC.py" below):
 *
 *   cc_resample_indices   CC.py:216-241  _get_subsampling_indices (numpy RandomState replay)
 *   cc_resample_device    the same on the device (n <= 65536), straight into HBM
 *   cc_resample_device_wide  the same for any n, without simulating the shuffle
 *   cc_scatter_labels     CC.py:260-262, :284-285  indicator / one-hot row placement
 *   cc_copy_label_columns CC.py:185-195 (the parallel paths' shared M) -> multi-GPU label exchange
 *   cc_cosample           CC.py:264  I = S^T S            (int8 MFMA, upper-triangle tiles)
 *   cc_coassoc            CC.py:287-290 + :338-344  M += L^T L fused with the 20-bin histogram
 *   cc_consensus          CC.py:372-373  C = f32(M) / f32(I + 1e-6), diag 1
 *   cc_item_consensus     (no reference code) item / cluster consensus sums of C by cluster
 *   cc_agreement_sums     (no reference code) contingency sums of every pair of label columns:
 *                         the adjusted Rand / Jaccard agreement of the resamples (int8 MFMA)
 *   cc_kmeans_plan        packing of the (K, init) problems of one resample into units
 *   cc_split_f16          f16 hi/lo operand image of the rows for the k-means MFMAs
 *   cc_kmeans_batched     CC.py:282 clusterer.fit_predict for every (h, K) at once
 *   cc_kmeans_wide        the same for wide rows (d > 128), as distance/centre GEMM rounds
 *                         (sklearn KMeans: k-means++ init, Lloyd, best of n_init)
 *   cc_kmeans_f64         the same at float64 for float64 input
 *   cc_kmeans_f64_cols    cc_kmeans_f64 with every resample on its own columns (feature subsampling)
 *   cc_kmeans_launch_plan which of the three above a fit launches, how often and how large
 *   cc_kmeans_fit         CC.py:282 in one call (makes the calls of cc_kmeans_launch_plan)
 *   cc_euclidean, cc_hc_gather, cc_hc_nnchain_batched, cc_hc_cut
 *                         CC.py:282 for AgglomerativeClustering (ward / average / complete,
 *                         euclidean): one tree per resample, cut at every K
 *   cc_pdist              the distances of the same trees for metric = manhattan / cosine /
 *                         correlation (average and complete linkage): scipy's pdist, bit for bit
 *   cc_pdist_batched      the same distances per resample when each resample also draws its own
 *                         columns (feature subsampling): pdist(X[idx[b]][:, cols[b]], metric)
 *   cc_pam_build, cc_pam_swap_step, cc_pam_active, cc_pam_labels
 *                         CC.py:282 for the PAM (k-medoids) base clusterer: BUILD and SWAP of
 *                         every (resample, K) problem over the same [B][m][m] distances
 *   cc_gmm_gather, cc_gmm_start, cc_gmm_em_step, cc_gmm_active, cc_gmm_finish
 *                         CC.py:282 for the GMM base clusterer (diagonal Gaussian mixture, sklearn's
 *                         GaussianMixture(covariance_type='diag') in float64): batched EM of every
 *                         (resample, K) problem from a k-means initialisation, best of n_init
 *   cc_gmm_full_start, cc_gmm_full_em_step, cc_gmm_full_finish
 *                         the same for FullGMM (full covariances, sklearn's default
 *                         covariance_type='full'): weighted covariances, batched Cholesky and
 *                         triangular inverse, the E-step against the precision factor
 *   cc_nmf_start, cc_nmf_steps, cc_nmf_finish
 *                         CC.py:282 for the NMF base clusterer (sklearn's NMF(init='random',
 *                         solver='mu') in float64): batched multiplicative updates of every
 *                         (resample, K) problem, best of n_init
 */
#ifndef CCMI_H
#define CCMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CC_OK 0
#define CC_ERR_ARG (-1)
#define CC_ERR_HIP (-2)
#define CC_ERR_UNSUPPORTED (-3)

/* Tile edge of the upper-triangle tiling used by cc_cosample / cc_coassoc. */
#define CC_TILE 256
/* Number of consensus-histogram bins (CC.py:316 bins=20). */
#define CC_NBINS 20

const char* cc_version(void);
const char* cc_last_error(void);
/* SHA-256 prefix (16 hex digits) of the sources and flags this library was built from
 * (the .hip, .cpp and .h files of csrc, include/ccmi.h and the csrc Makefile); the Python host
 * refuses a library whose id does not match the sources next to it. */
const char* cc_build_id(void);

/* ---- host-side helpers (native, no device) ------------------------------ */

/* Resample indices of CC.py:231-239 for h in [h_begin, h_end):
 * out[(h-h_begin)*m + r] = numpy.random.RandomState(seed + h).permutation(n)[r], r < m
 * (RandomState.choice(n, m, replace=False) == permutation(n)[:m]).  MT19937
 * init_genrand + legacy random_interval rejection sampling, bit-identical to
 * numpy 1.17+ legacy RandomState.  Runs on n_threads host threads (<=0: all). */
int cc_resample_indices(uint32_t seed, int h_begin, int h_end, int n, int m, int32_t* out,
                        int n_threads);

/* Raw doubles of numpy.random.RandomState(seed).random_sample(count). */
int cc_random_sample(uint32_t seed, int64_t count, double* out);

/* Number of tiles of the CC_TILE upper-triangle tiling for n samples. */
int64_t cc_num_tiles(int n);

/* ---- device kernels ----------------------------------------------------- */

/* cc_resample_indices on the device (CC.py:231-239): out [h_end-h_begin][m] int32 in device
 * memory, bit-identical to numpy.random.RandomState(seed + h).permutation(n)[:m].  One
 * workgroup per resample (Fisher-Yates over a uint16 array in LDS), so 1 <= n <=
 * cc_resample_device_max_n() (65536); larger n stays on the host replay. */
int cc_resample_device_max_n(void);
int cc_resample_device(uint32_t seed, int h_begin, int h_end, int n, int m, int32_t* out,
                       void* stream);

/* The same draws for any n (no 65536 limit): RandomState(seed + h).permutation(n)[:m] resolved
 * from the shuffle's swap partners (the draws on one lane per resample, a counting sort of the
 * steps by partner, then each output value as the end of a short chain of later writers), so no
 * step of the shuffle is simulated.  workspace: device, ws_bytes >= the bytes for one resample;
 * resamples run in batches that fit (cc_resample_device_wide_workspace_bytes(n, nh) for nh at
 * once).  Asynchronous on `stream`; out as cc_resample_device. */
int cc_resample_device_wide(uint32_t seed, int h_begin, int h_end, int n, int m, int32_t* out,
                            void* workspace, size_t ws_bytes, void* stream);
size_t cc_resample_device_wide_workspace_bytes(int n, int nh);

/* labels_nh[idx[h][r] * ldl + h] = labels_hm ? labels_hm[h*m + r] : 0 for h < H, r < m.
 * labels_nh must be pre-filled with 0xFF (= not sampled).  (CC.py:260-262, :284-285)
 * An entry of idx_hm outside [0, n) addresses no row: it is skipped, nothing is written for it
 * and the call still returns CC_OK.  Only the low byte of a label is stored.  H = 0 or m = 0
 * writes nothing (CC_OK); ldl < H, n <= 0, a negative H or m, or a NULL idx_hm / labels_nh is
 * CC_ERR_ARG.  Asynchronous on `stream`. */
int cc_scatter_labels(const int32_t* idx_hm, const int32_t* labels_hm, int H, int m, int n,
                      int8_t* labels_nh, int ldl, void* stream);

/* dst[r*ld_dst + col_dst + j] = src[r*ld_src + col_src + j] for r < rows, j < width (bytes).
 * Moves a window of resample columns between sample-major label matrices ([rows][ld] uint8):
 * the multi-GPU exchange packs a rank's own columns [h0, h1) into a contiguous block before an
 * all-gather and places each rank's block at its columns afterwards.  It replaces the
 * reference's shared in-place M of its parallel paths (CC.py:185-195): labels, not n x n
 * counts, cross the links.  Asynchronous on `stream`. */
int cc_copy_label_columns(const uint8_t* src, int64_t ld_src, int col_src, uint8_t* dst,
                          int64_t ld_dst, int col_dst, int64_t rows, int width, void* stream);

/* Co-sampling counts I_ij = #{h : i and j both sampled} for the tiles
 * [tile_begin, tile_end) of the upper-triangle tiling (CC.py:264).
 * labels_nh: [n][ldl] int8, 0xFF = not sampled; Hpad (multiple of 128, <= ldl) columns used;
 *            16-B aligned, like I_tiles and bin_table below (device allocations are).
 * I_tiles:   [tile_end - tile_begin][CC_TILE*CC_TILE] uint16, accumulator order (device-private).
 * I_full:    optional [n][n] int32 (both triangles), may be NULL. */
int cc_cosample(const int8_t* labels_nh, int n, int ldl, int Hpad, int64_t tile_begin,
                int64_t tile_end, uint16_t* I_tiles, int32_t* I_full, void* stream);

/* Co-association counts M_ij = #{h : label_h(i) == label_h(j) >= 0} for the same
 * tiles, fused with the numpy-exact 20-bin histogram of C = f32(M)/f32(I+1e-6)
 * over the strict upper triangle i < j (CC.py:287-290, :338-344).
 * edges: 21 float32 bin edges (numpy's), device.  bin_counts: [20] uint64, device,
 * accumulated into (not cleared).  M_full: optional [n][n] int32, may be NULL.
 * bin_table: optional cc_bin_table output with table_rows >= Hpad + 1 rows (binning without
 * a division; identical bins), NULL for the division path.  K <= 127. */
int cc_coassoc(const int8_t* labels_nh, int n, int ldl, int Hpad, int K, int64_t tile_begin,
               int64_t tile_end, const uint16_t* I_tiles, const float* edges,
               unsigned long long* bin_counts, int32_t* M_full, const uint16_t* bin_table,
               int table_rows, void* stream);

/* Item consensus sums (Monti's item / cluster consensus without the n x n matrix):
 * S[i*Kc + c] += sum over j != i with cl[j] == c of C_ij * 2^40 (exact integers), for the pairs
 * covered by tiles [tile_begin, tile_end). S is accumulated into: the caller zeroes it.
 * C_ij = f32(M_ij) / f32(I_ij + 1e-6) as cc_consensus computes it; C_ij * 2^40 is an integer
 * for Hpad <= 65535, and the int64 sums are exact for n <= 2^22, so disjoint tile ranges (and
 * ranks) add to the same S in any order.
 * I_tiles: as written by cc_cosample for the same tile range.
 * cl: [n] int32 device, the cluster of each item; an id outside [0, Kc) means "no cluster" (the
 *     item adds to no column, its own row is still filled).  S: [n][Kc] int64 device, 8-B aligned.
 * K, Kc in [1, 127]. */
int cc_item_consensus(const int8_t* labels_nh, int n, int ldl, int Hpad, int K,
                      int64_t tile_begin, int64_t tile_end, const uint16_t* I_tiles,
                      const int32_t* cl, int Kc, int64_t* S, void* stream);

/* Pairwise agreement of label columns (Ben-Hur et al. 2002; the sums behind the adjusted Rand and
 * Jaccard indices): for every column h1 of group A and h2 of group B, with N[a][b] = #{items i
 * with A[i][h1] = a and B[i][h2] = b} over the items present in both,
 *   sums[h1][h2] = { s0 = sum N, s2 = sum N^2, r2 = sum_a (sum_b N)^2, c2 = sum_b (sum_a N)^2 },
 * exact integers (sklearn's pair_confusion_matrix: C11 = s2 - s0, C01 = c2 - s2, C10 = r2 - s2,
 * C00 = s0^2 - C01 - C10 - s2).
 * A_nh: [n][ldA] int8 device, HA columns used, labels in [0, KA); any other byte (0xFF) = absent.
 * B_nh: [n][ldB] likewise (HB columns, KB), or NULL: A with itself (ldB, HB, KB ignored; sums is
 *       [HA][HA][4]; only the tiles of the upper triangle run and each stores its mirror too).
 * Tiles: cc_agreement_num_tiles(HA, HB, KA, KB, symmetric) tiles of 256 x 256 virtual columns; a
 *       call fills the pairs of [tile_begin, tile_end) with plain stores (the caller zeroes sums;
 *       disjoint ranges fill disjoint pairs; an empty range launches nothing).
 * sums: [HA][HB][4] int64 device, 8-B aligned.  workspace: device, 16-B aligned,
 *       ws_bytes >= cc_agreement_workspace_bytes(n, HA, HB) (HB = 0 for A with itself): the columns
 *       transposed, written by every call.  KA, KB in [1, 127]; HA, HB, n >= 1.  No atomics on
 *       global memory and no floating point: the output is bitwise reproducible. */
size_t cc_agreement_workspace_bytes(int n, int HA, int HB);
int64_t cc_agreement_num_tiles(int HA, int HB, int KA, int KB, int symmetric);
int cc_agreement_sums(const int8_t* A_nh, int ldA, int HA, int KA, const int8_t* B_nh, int ldB, int HB,
                      int KB, int n, int64_t tile_begin, int64_t tile_end, int64_t* sums,
                      void* workspace, size_t ws_bytes, void* stream);

/* Bin thresholds per co-sampling count i in [0, rows): row i = 21 uint16 T[b] =
 * min{m : bin(f32(m) / f32(i + 1e-6)) >= b} (T[0] = 0, T[20] = 0xFFFF; i + 1 if no m <= i
 * reaches b), so bin = #{b in 1..19 : m >= T[b]} (numpy.histogram semantics, CC.py:338-344).
 * table: device, table_bytes >= cc_bin_table_bytes(rows).  After the rows * 21 uint16 (padded
 * to 16 B) it holds, when rows is small enough for cc_coassoc to stage them on chip, the
 * threshold pairs T[g] | T[g+1] << 16 (rows * 20 uint32) and the bins themselves for every
 * (m <= i) pair (one byte at i (i + 1) / 2 + m, padded to 16 B). */
int cc_bin_table(int rows, const float* edges, uint16_t* table, size_t table_bytes, void* stream);

/* Bytes of the cc_bin_table buffer for `rows` rows (0 when rows is out of range). */
size_t cc_bin_table_bytes(int rows);

/* Largest table (rows) cc_coassoc can stage on chip. */
int cc_bin_table_max_rows(void);

/* Largest row count for each staged form: 0 = uint16 thresholds (= cc_bin_table_max_rows),
 * 1 = threshold pairs, 2 = the bin triangle.  cc_coassoc stages the most compact form that fits. */
int cc_bin_table_form_rows(int form);

/* Self-test of the division-free binning: for EVERY pair of counts (m <= i < rows), compare
 * the table forms cc_coassoc uses (threshold table + reciprocal estimate computed per
 * element, and with the staged per-row reciprocal; the threshold pairs and the bin triangle
 * when the table holds them) against the direct numpy-exact bin of f32(m) / f32(i + 1e-6).
 * mismatches: device [4] uint64, accumulated into. */
int cc_bin_selftest(int rows, const float* edges, const uint16_t* table,
                    unsigned long long* mismatches, void* stream);

/* C = f32(M) / f32(f64(I) + 1e-6) with C_ii = 1 (CC.py:372-373), [n][n]. */
int cc_consensus(const int32_t* M, const int32_t* I, int n, float* C, void* stream);

/* Manhattan distances between the rows of C [n][d] float32: D [n][n] float64,
 * D_ij = sum_k |f64(C_ik) - f64(C_jk)| summed sequentially over k (scipy pdist 'cityblock'
 * order), for the consensus labels of CC.py:292-314 (AgglomerativeClustering on the rows of C
 * under the manhattan metric). */
int cc_manhattan(const float* C, int n, int d, double* D, void* stream);

/* Agglomerative linkage of the consensus labels (CC.py:306-312: AgglomerativeClustering ->
 * sklearn linkage_tree -> scipy.cluster.hierarchy.linkage -> _hierarchy.nn_chain) on the device:
 * D [n][n] float64 symmetric (e.g. from cc_manhattan) is overwritten; Z [n-1][4] float64 receives
 * (x, y, distance, size) per merge in nn_chain's merge order, before linkage()'s stable sort by
 * distance and relabelling (done by the caller).  Runs on G co-resident workgroups joined by
 * grid barriers (G from n; CCMI_LINK_G overrides, 0 = one workgroup); workspace of
 * cc_linkage_workspace_bytes(n) bytes; call cc_linkage_check after it.  A scan that finds no
 * live finite neighbour (non-finite distances) indexes nothing: the tree is abandoned, Z is
 * invalid and cc_linkage_check reports it. */
#define CC_LINK_AVERAGE 0
#define CC_LINK_COMPLETE 1
#define CC_LINK_WEIGHTED 2
/* Ward on euclidean (not squared) distances, scipy's _ward update:
 * t = 1 / (nx + ny + ni); sqrt((ni+nx) t dxi^2 + (ni+ny) t dyi^2 - ni t dxy^2). */
#define CC_LINK_WARD 3
size_t cc_linkage_workspace_bytes(int n);
int cc_linkage_nnchain(double* D, int n, int method, double* Z, void* workspace, size_t ws_bytes,
                       void* stream);

/* Single linkage of the consensus labels: sklearn's path for linkage='single' with the
 * reference's 'manhattan' affinity (CC.py:306-312 -> linkage_tree ->
 * _hierarchical_fast.mst_linkage_core, Prim's MST-LINKAGE-CORE) on the device, over the rows of
 * D [n][n] float64 (read only; cc_manhattan's values are DistanceMetric64 cityblock's).
 * out [n-1][3] float64 = (current node, new node, distance) per Prim step; the caller sorts the
 * edges by distance (stable) and labels them (_single_linkage_label).  G co-resident workgroups
 * as cc_linkage_nnchain; workspace of cc_linkage_mst_workspace_bytes(n) bytes; call
 * cc_linkage_check after it. */
size_t cc_linkage_mst_workspace_bytes(int n);
int cc_linkage_mst(const double* D, int n, double* out, void* workspace, size_t ws_bytes, void* stream);

/* After cc_linkage_nnchain / cc_linkage_mst on `stream` with this workspace: synchronises the
 * stream and returns CC_ERR_HIP if cc_linkage_nnchain found no neighbour (message "... found no
 * neighbour ...") or a grid barrier of the linkage timed out (the output is then invalid), else
 * CC_OK. */
int cc_linkage_check(const void* workspace, size_t ws_bytes, void* stream);

/* Hierarchical base clusterer (CC.py:282 with AgglomerativeClustering(linkage = ward | average |
 * complete, metric = euclidean), which is scipy.cluster.hierarchy.linkage(X[idx[h]], method,
 * 'euclidean') cut by _hc_cut): one tree per resample serves every K.
 *
 * cc_euclidean: D [n][n] float64 = squareform(pdist(X, 'euclidean')) bit for bit: sqrt of the
 * float64 sum over k, in increasing k, of (u_k - v_k)^2 with no FMA; symmetric, zero diagonal.
 * X [n][d] float32 (is_f64 = 0; converted exactly) or float64 (is_f64 = 1). */
int cc_euclidean(const void* X, int is_f64, int n, int d, double* D, void* stream);

/* The same matrix for the base clusterer's other metrics (AgglomerativeClustering(linkage =
 * average | complete, metric = manhattan | cosine | correlation) -> scipy linkage(X, method,
 * metric)): D [n][n] float64 = squareform(pdist(X, metric)) bit for bit, symmetric, exact-zero
 * diagonal; X as for cc_euclidean.
 *   CC_METRIC_EUCLIDEAN  cc_euclidean (the same tile kernel, as for every metric here)
 *   CC_METRIC_CITYBLOCK  the float64 sum over k, in increasing k, of |u_k - v_k|
 *   CC_METRIC_COSINE     1 - c, c = t(u, v) / (norm_u norm_v) with |c| > 1 clipped to +-1, where
 *                        t is scipy's two-accumulator dot product: the products of even k and of
 *                        odd k < (d & ~1) summed apart, in increasing k, then added, then the
 *                        product of an odd last column added; norm_u = sqrt(t(u, u)), written to
 *                        norms [n] (device, float64) by a pre-kernel.  A zero row gives NaN.
 * pdist's 'correlation' is CC_METRIC_COSINE on the float64 rows less their means
 * (X - X.mean(axis=1, keepdims=True) in numpy, whose mean is a pairwise sum): the caller centres.
 * norms may be NULL for the other metrics.  An unknown metric returns CC_ERR_ARG. */
#define CC_METRIC_EUCLIDEAN 0
#define CC_METRIC_CITYBLOCK 1
#define CC_METRIC_COSINE 2
int cc_pdist(const void* X, int is_f64, int n, int d, int metric, double* D, double* norms, void* stream);

/* Feature subsampling: the distances of B resamples that each draw their own rows AND columns.
 * Db [B][m][m] float64: Db[b] = squareform(pdist(X[idx[b]][:, cols[b]], metric)) bit for bit,
 * symmetric, exact-zero diagonal.  X [n][d] as for cc_euclidean; idx [B][m] int32 in [0, n);
 * cols [B][md] int32 in [0, d), ascending (their order is the summation order); all on the device.
 * The caller checks both ranges: an entry outside them is read out of bounds.
 * metric: CC_METRIC_EUCLIDEAN, _CITYBLOCK, _COSINE, or CC_METRIC_CORRELATION, which this entry
 * point alone accepts: a row pass writes each resample's compact float64 rows [B][m][md] into
 * the workspace, for correlation less numpy's mean of the compact row (s / md, s numpy's pairwise
 * sum), and for cosine and correlation scipy's norms [B][m] behind them (a norm of 0 marks a row
 * without distances); the tile kernel of cc_pdist / cc_euclidean then runs once per tree.
 * CC_ERR_ARG: a null pointer, a size below 1, md > d, m > n, B > 65535, an unknown metric, or
 * fewer workspace bytes than cc_pdist_batched_workspace_bytes (0 for arguments it refuses). */
#define CC_METRIC_CORRELATION 3
size_t cc_pdist_batched_workspace_bytes(int B, int m, int md, int metric);
int cc_pdist_batched(const void* X, int is_f64, int n, int d, const int* idx, const int* cols, int B, int m,
                     int md, int metric, double* Db, void* workspace, size_t ws_bytes, void* stream);

/* Db [B][m][m]: Db[b][a][c] = Dfull[idx[b][a]][idx[b][c]] for B resamples (idx [B][m] int32,
 * values in [0, n)). */
int cc_hc_gather(const double* Dfull, int n, const int* idx, int B, int m, double* Db, void* stream);

/* Workspace of cc_hc_nnchain_batched (nK = 0) or of cc_hc_cut for B trees of m leaves and nK
 * values of K; a workspace sized for nK serves both calls. */
size_t cc_hc_workspace_bytes(int m, int B, int nK);

/* scipy's nn_chain on B trees at once, one workgroup per tree (no communication between
 * workgroups): D [B][m][m] float64 symmetric, overwritten; Z [B][m-1][4] float64 receives each
 * tree's (x, y, distance, size) per merge in merge order (x < y: slot x dies, slot y keeps the
 * union), as cc_linkage_nnchain writes them.  method: CC_LINK_*.  The workspace begins with one
 * status word per tree: a tree whose scan finds no neighbour (non-finite distances) stops there
 * and sets its word; cc_hc_check reports it. */
int cc_hc_nnchain_batched(double* D, int B, int m, int method, double* Z, void* workspace, size_t ws_bytes,
                          void* stream);

/* After cc_hc_nnchain_batched on `stream`: synchronises the stream and returns CC_ERR_HIP when a
 * tree's status word is set (its Z is invalid), else CC_OK. */
int cc_hc_check(const void* workspace, int B, void* stream);

/* The K-cluster cuts of B trees: for tree b (resample h_begin + b), K index k and leaf r,
 * labels[k][idx[b][r]][h_begin + b] = cluster id in [0, Ks[k]), every id used (numbering: the
 * clusters' surviving slots in increasing order).  Z [B][m-1][4] raw merges; rank [B][m-1] int32:
 * the position of each merge in the stable sort of its tree's merges by distance; idx [B][m]
 * int32; Ks [nK] int32 on the device, 1 <= Ks[k] <= m; labels uint8 [nK][n][ldl]. */
int cc_hc_cut(const double* Z, const int* rank, const int* idx, int B, int m, const int* Ks, int nK,
              int h_begin, uint8_t* labels, int64_t n, int64_t ldl, void* workspace, size_t ws_bytes,
              void* stream);

/* PAM (partitioning around medoids; Kaufman & Rousseeuw's BUILD and SWAP, R's pam with
 * pamonce = 0) for the nK values Ks of K on each of B trees' distances D [B][m][m] (float64,
 * symmetric, zero diagonal, finite; read only), the batch cc_hc_gather or cc_pdist_batched makes.
 * Problem (b, k) has Ks[k] medoids.  Ks [nK] int32 on the device, 1 <= Ks[k] <= Kmax; a value
 * outside is read as the nearest bound.  Limits: B <= 65535, m <= 65535, 1 <= Kmax <= min(m, 127).
 * All arithmetic is float64 and no sum uses a floating-point atomic: the same inputs give the same
 * medoids and bitwise the same inertia on every run.  A decision between two candidates whose
 * sums differ by less than about m * 2^-52 of the sums may fall differently than in another
 * conforming implementation, which adds in another order; on integer-valued distances every sum
 * is exact and the tie rules below decide.
 *
 * cc_pam_workspace_bytes: the workspace of the calls below (0 for arguments they refuse).  One
 * workspace carries a batch from cc_pam_build through cc_pam_swap_step to cc_pam_labels. */
size_t cc_pam_workspace_bytes(int m, int B, int nK, int Kmax);

/* BUILD: medoid 0 of a tree is the first index of the smallest row sum; step t = 1 .. Kmax - 1
 * adds the first index of the largest gain sum_j max(near[j] - D[i][j], 0) over the non-medoids
 * (near[j]: the distance of j to its nearest medoid so far).  The chain is greedy, so problem
 * (b, k) starts from the first Ks[k] medoids of tree b's chain.  Two launches a step, ordered by
 * the stream, then one that sets up every problem's state (near, second, nearest slot, the items
 * grouped by slot, n_iter = 0).  Asynchronous on `stream`. */
int cc_pam_build(const double* D, int B, int m, const int* Ks, int nK, int Kmax, void* workspace, size_t ws_bytes,
                 void* stream);

/* One SWAP iteration of every problem that is still active (after cc_pam_build every problem
 * is): over all pairs of a medoid i and a non-medoid h, dTD(i, h) = sum_j of
 * min(D[h][j], second[j]) - near[j] where i is j's nearest medoid, else min(D[h][j] - near[j], 0);
 * the smallest is taken, a tie to the lowest h, then to the medoid with the lowest item index.
 * When it is < 0 and the problem has made fewer than max_iter swaps, h replaces i and the state
 * is refreshed; else the problem is converged and later calls leave it alone.  The number of
 * problems that swapped is left in the workspace for cc_pam_active.  Asynchronous on `stream`. */
int cc_pam_swap_step(const double* D, int B, int m, const int* Ks, int nK, int Kmax, int max_iter, void* workspace,
                     size_t ws_bytes, void* stream);

/* Synchronises `stream` and stores in *active (host) how many problems the last
 * cc_pam_swap_step swapped: 0 = every problem is converged. */
int cc_pam_active(const void* workspace, int* active, void* stream);

/* The results of the batch: for tree b (resample h_begin + b), K index k and item r,
 * labels[k][idx[b][r]][h_begin + b] = the rank, by ascending item index, of r's nearest medoid (a
 * tie in distance goes to the lowest item index; a medoid labels itself); labels uint8
 * [nK][n][ldl], idx [B][m] int32 as for cc_hc_cut.  inertia [nK][ldo] float64 and n_iter [nK][ldo]
 * int32 (either may be NULL) receive at [k][h_begin + b] the total deviation sum_j near[j] and the
 * number of swaps made; medoids (NULL or [B][nK][Kmax] int32) the medoid items r in ascending
 * order, -1 behind the first Ks[k]. */
int cc_pam_labels(const double* D, const int* idx, int B, int m, const int* Ks, int nK, int Kmax, int h_begin,
                  uint8_t* labels, int64_t n, int64_t ldl, double* inertia, int* n_iter, int64_t ldo, int* medoids,
                  void* workspace, size_t ws_bytes, void* stream);

/* GMM: EM for the mixture of Ks[k] Gaussians with diagonal covariances (sklearn 1.7's
 * GaussianMixture(covariance_type='diag') in float64, restated in gmm.py) on each of B resamples'
 * rows Xb [B][m][md] (float64, finite, the batch cc_gmm_gather makes).  Problem (b, k) has Ks[k]
 * components.  Ks [nK] int32 on the HOST (it sizes the workspace), 1 <= Ks[k] <= min(m, 127),
 * nK <= 127, B * nK <= 65535, md >= 1.  All arithmetic is float64, both contractions run on the
 * float64 matrix cores and no sum uses a floating-point atomic or depends on the grid or the
 * batch: the same inputs give bitwise the same lower bound on every run and under every batching.
 * Another conforming implementation adds in another order, so its lower bound differs by about
 * m * 2^-52 relative and a decision (converged, the winning init, a row's component) may fall
 * differently where its margin is that small.
 *
 * cc_gmm_workspace_bytes: the workspace of the calls below (0 for arguments they refuse); it holds
 * per problem the responsibilities (8 m Kp bytes, Kp = Ks[k] rounded up to 16), the M-step sums,
 * the E-step's operand image and the 16-row tile sums.  One workspace carries a batch through
 * every init: cc_gmm_start, cc_gmm_em_step until cc_gmm_active reads 0, cc_gmm_finish. */
size_t cc_gmm_workspace_bytes(int m, int md, int B, const int* Ks, int nK);

/* Xb[b][r][c] = X[idx[b][r]][cols ? cols[b][c] : c]: the rows of B resamples under their own
 * columns.  X [n][d] float64; idx [B][m] int32 and cols (NULL = all columns, md = d; else [B][md]
 * int32) on the device, read as given: the caller checks their ranges.  It serves every row-batch
 * clusterer (GMM, FullGMM, NMF) under the name it got first. */
int cc_gmm_gather(const double* X, int64_t n, int d, const int* idx, const int* cols, int B, int m, int md,
                  double* Xb, void* stream);

/* Start one init of every problem: the one-hot responsibilities from the init labels
 * init_labels uint8 [nK][n][ldl], read at [k][idx[b][r]][col_begin + b] (a label outside
 * [0, Ks[k]) gives the row to no component), then sklearn's _initialize (the M-step with
 * weights = counts / m) and the problem's state: n_iter 0, previous bound -inf, active.  The best
 * bound of earlier inits is kept.  Asynchronous on `stream`. */
int cc_gmm_start(const double* Xb, const int* idx, int B, int m, int md, const int* Ks, int nK,
                 const uint8_t* init_labels, int64_t n, int64_t ldl, int col_begin, double reg_covar,
                 void* workspace, size_t ws_bytes, void* stream);

/* One EM iteration of every problem that is still active: the E-step (log probabilities as one
 * GEMM of [x, x^2] against [-2 mean prec ; prec], scipy's logsumexp per row, the lower bound = the
 * mean of the row log-norms), the M-step (resp^T [x, x^2, 1]; weights divided by their sum;
 * variances avg_x2 - mean^2 + reg_covar), and the decision: converged when
 * |bound - previous| < tol, stopped unconverged at max_iter iterations.  A finished problem is
 * left alone by later calls.  A variance that is not positive marks the problem failed.  The
 * number of problems still active is left in the workspace for cc_gmm_active. */
int cc_gmm_em_step(const double* Xb, int B, int m, int md, const int* Ks, int nK, double tol, double reg_covar,
                   int max_iter, void* workspace, size_t ws_bytes, void* stream);

/* Synchronises `stream` and stores in *active (host) how many problems the last cc_gmm_em_step
 * left active (0 = every problem is finished) and in *failed (host, may be NULL) how many
 * problems of the batch have failed since cc_gmm_start.  It reads only the two header words that
 * the workspaces of every row-batch clusterer share (cc_gmm_workspace_bytes,
 * cc_gmm_full_workspace_bytes, cc_nmf_workspace_bytes), so it serves all three: after
 * cc_gmm_full_em_step and cc_nmf_steps as after cc_gmm_em_step. */
int cc_gmm_active(const void* workspace, int* active, int* failed, void* stream);

/* The results of one init: with keep_best = 0 (the first init) of every problem, else of the
 * problems whose lower bound is strictly larger than the best of the inits before.  For those,
 * a final E-step under the init's parameters gives labels[k][idx[b][r]][h_begin + b] = the
 * component of the largest log responsibility (first index on ties); labels uint8 [nK][n][ldl].
 * lower_bound [nK][ldo] float64, n_iter [nK][ldo] int32 and converged [nK][ldo] uint8 (each may be
 * NULL) receive the init's values at [k][h_begin + b]. */
int cc_gmm_finish(const double* Xb, const int* idx, int B, int m, int md, const int* Ks, int nK, int keep_best,
                  int h_begin, uint8_t* labels, int64_t n, int64_t ldl, double* lower_bound, int* n_iter,
                  uint8_t* converged, int64_t ldo, void* workspace, size_t ws_bytes, void* stream);

/* FullGMM: the same EM for full covariances (sklearn 1.7's GaussianMixture(covariance_type='full')
 * in float64, restated in gmm.py's FullGMM).  The batch, the rows (cc_gmm_gather), Ks, the
 * workspace header and the sequence of calls are the diagonal model's, with the limits
 * 1 <= Ks[k] <= min(m, 127), nK <= 127, B * nK <= 65535 and 1 <= md <= 128.  The M-step is the
 * means (resp^T [x, 1]), the lower triangle of every component's weighted covariance of the
 * centred rows (sklearn's dot(resp_c * diff.T, diff) / nk_c with reg_covar on the diagonal), and
 * per component its Cholesky factor L, the precision factor P = L^-T, mu P and the log
 * determinant; the E-step is sum_j ((x P)_j - (mu P)_j)^2 on the float64 matrix cores.  Every sum
 * has a fixed order (csrc/gmm_full.hip), none depends on the grid or the batch, and there is no
 * floating-point atomic.  A pivot of the factorisation that is not positive marks the problem
 * failed.
 *
 * cc_gmm_full_workspace_bytes: the workspace of the three calls below (0 for arguments they
 * refuse); per problem the responsibilities (8 m Kp bytes), the M-step sums and the means
 * (8 Kp (2 md + 1)), the factors (8 K md md), mu P (8 Kp md), three constants per component and
 * the 16-row tile sums.  cc_gmm_active reads this workspace as it reads cc_gmm_start's. */
size_t cc_gmm_full_workspace_bytes(int m, int md, int B, const int* Ks, int nK);

/* cc_gmm_start for full covariances: the one-hot responsibilities, sklearn's _initialize and the
 * state.  Arguments as cc_gmm_start's. */
int cc_gmm_full_start(const double* Xb, const int* idx, int B, int m, int md, const int* Ks, int nK,
                      const uint8_t* init_labels, int64_t n, int64_t ldl, int col_begin, double reg_covar,
                      void* workspace, size_t ws_bytes, void* stream);

/* cc_gmm_em_step for full covariances: one E-step, the decision and the M-step of every problem
 * still active.  Arguments as cc_gmm_em_step's; cc_gmm_active then reads the counts. */
int cc_gmm_full_em_step(const double* Xb, int B, int m, int md, const int* Ks, int nK, double tol, double reg_covar,
                        int max_iter, void* workspace, size_t ws_bytes, void* stream);

/* cc_gmm_finish for full covariances: which problems this init wins, their scalar outputs and
 * the labels of a final E-step.  Arguments as cc_gmm_finish's. */
int cc_gmm_full_finish(const double* Xb, const int* idx, int B, int m, int md, const int* Ks, int nK, int keep_best,
                       int h_begin, uint8_t* labels, int64_t n, int64_t ldl, double* lower_bound, int* n_iter,
                       uint8_t* converged, int64_t ldo, void* workspace, size_t ws_bytes, void* stream);

/* NMF: X ~ W H by multiplicative updates under the Frobenius loss (sklearn 1.7's NMF(init='random',
 * solver='mu', beta_loss='frobenius') without regularisation in float64, restated in nmf.py) on
 * each of B resamples' rows Xb [B][m][md] (float64, finite, non-negative, the batch cc_gmm_gather
 * makes).  Problem (b, k) has Ks[k] components; the limits are m >= 1, md >= 1, 1 <= Ks[k] <= 127
 * (K may exceed m and md), nK <= 127 and B * nK <= 65535.  Every contraction runs on the float64
 * matrix cores in a fixed order (csrc/nmf.hip); no sum depends on the grid or the batch and there
 * is no floating-point atomic, so a problem's results do not depend on the batch it ran in.  The
 * device always forms (W^T W) H where sklearn's multi_dot may pick W^T (W H).
 *
 * cc_nmf_workspace_bytes: the workspace of the calls below (0 for arguments they refuse); per
 * problem, with Kp = K rounded up to 16, W (8 m Kp bytes), H and W^T X (8 Kp md each), H H^T and
 * W^T W (8 Kp Kp each), the 16-row tile sums of the error and the 48-byte state.  The workspace
 * keeps each problem's best error across the inits of one batch, so one workspace serves every
 * init: cc_nmf_start, cc_nmf_steps until cc_gmm_active reads 0, cc_nmf_finish. */
size_t cc_nmf_workspace_bytes(int m, int md, int B, const int* Ks, int nK);

/* Starts one init of every problem: avg_b = sqrt(mean(Xb[b]) / K) from a fixed-order mean,
 * W = avg |N_W|, H = avg |N_H| and the error at init.  normals_w holds |N_W| [m][K] for every K of
 * Ks, concatenated, normals_h |N_H| [K][md] likewise (float64, device); all B resamples share
 * them.  Every problem is active afterwards. */
int cc_nmf_start(const double* Xb, int B, int m, int md, const int* Ks, int nK, const double* normals_w,
                 const double* normals_h, void* workspace, size_t ws_bytes, void* stream);

/* Enqueues the iterations first .. first + count - 1 (1-based since cc_nmf_start, cut at max_iter)
 * of every problem still active; an inactive problem costs no work.  After an iteration that is a
 * multiple of 10 (when tol > 0) the error is evaluated and a problem stops, converged, when
 * (previous error - error) / error at init < tol; after iteration max_iter every problem stops.
 * After such an iteration the number of problems still active is left in the workspace for
 * cc_gmm_active, which reads this workspace as it reads cc_gmm_start's (no problem fails). */
int cc_nmf_steps(const double* Xb, int B, int m, int md, const int* Ks, int nK, int first, int count, double tol,
                 int max_iter, void* workspace, size_t ws_bytes, void* stream);

/* The results of one init: the final error sqrt(sum (X - W H)^2) of every problem; with
 * keep_best = 0 (the first init) every problem wins, else those whose error is strictly smaller
 * than the best of the inits before.  For the winners labels[k][idx[b][r]][h_begin + b] =
 * argmax_c W[r][c] sqrt(sum_j H[c][j]^2) (first index on ties); labels uint8 [nK][n][ldl].
 * reconstruction_err [nK][ldo] float64, n_iter [nK][ldo] int32 and converged [nK][ldo] uint8 (each
 * may be NULL) receive the init's values at [k][h_begin + b]. */
int cc_nmf_finish(const double* Xb, const int* idx, int B, int m, int md, const int* Ks, int nK, int keep_best,
                  int h_begin, uint8_t* labels, int64_t n, int64_t ldl, double* reconstruction_err, int* n_iter,
                  uint8_t* converged, int64_t ldo, void* workspace, size_t ws_bytes, void* stream);

/* Batched k-means for every (resample h, K, init) problem, replacing the per-(K, h)
 * clusterer.fit_predict(X[indices]) of CC.py:282 for the default clusterer
 * (sklearn KMeans: k-means++ init with 2+floor(ln K) local trials, Lloyd with strict
 * and tol convergence, empty-cluster relocation, best of n_init;
 * sklearn/cluster/_kmeans.py:174-262, :624-752, :1427-1556).
 *
 * Work is split into UNITS = (resample, subset of the (K, init) problems); a persistent
 * grid of workgroups pulls units from an atomic counter and runs each unit's fits as one
 * problem engine (every sweep streams the resample's rows once for up to 256 centroid
 * slots, packed round-robin from the unit's seeding and Lloyd problems).
 * Within a unit the init-0 problems with the same number of local trials share one
 * k-means++ chain: every fit replays RandomState(seed), so init 0 of K' chooses exactly the
 * first K' centres that init 0 of a larger K of that trial class chooses on the same
 * resample.  Only the largest such K seeds; the others start Lloyd from a prefix of its
 * centres (results are unchanged; CCMI_KM_SHARE_SEED=0 in the environment at launch makes
 * every problem seed on its own, for A/B runs).
 * Unit descriptor u (int32, CC_KM_USTRIDE entries): [0] = P (<= CC_KM_PMAX, the n_init
 * runs of one K consecutive), then per problem p: [1+4p] = K, [2+4p] = kidx (index into
 * Ks), [3+4p] = init, [4+4p] = local trials. */
#define CC_KM_PMAX 64
#define CC_KM_USTRIDE (1 + 4 * CC_KM_PMAX)

/* Pack the (K, n_init) groups of Ks[0..nK) into at least n_sub units (balanced by a K^2
 * cost proxy, largest K first); returns the unit count (> 0) or a negative error.
 * units must hold max_units * CC_KM_USTRIDE int32. */
int cc_kmeans_plan(const int32_t* Ks, int nK, int n_init, int n_sub, int32_t* units, int max_units);

/* Workspace bytes of a cc_kmeans_batched launch with `grid` workgroups. */
size_t cc_kmeans_workspace_bytes(int m, int dpad, const int32_t* units_host, int nU, int seedmax,
                                 int grid);

/* f16 hi/lo image of the rows for the MFMA operands: Xhl[r][0][d] = f16(X[r][d] * 2^e),
 * Xhl[r][1][d] = f16(X[r][d] * 2^e - hi), e in [-62, 62] (host-chosen so that
 * max|X| * 2^e <= 2^14).  X [n][dpad] f32, Xhl [n][2][dpad] uint16. */
int cc_split_f16(const float* X, int n, int dpad, int scale_exp, uint16_t* Xhl, void* stream);

/*  X         [n][dpad] float32, mean-centred, zero-padded from dreal to dpad in {32,64,128}
 *  Xhl       cc_split_f16 image of X with the same scale_exp
 *  xnorm     [n] float32 squared row norms of X
 *  idx_hm    [H][m] int32 resample rows; this launch runs resamples [h_begin, h_end)
 *  units     device copy of the plan; units_host the same array on the host
 *  kpp_u     [nK][n_init][kpp_stride] float64: the RandomState(seed) doubles of each
 *            (K, init) k-means++ run (entry 0: the first-centre draw, consumed on the host)
 *  kpp_pos   [nK][n_init] int32 first-centre positions in resample order
 *  labels_nh [nK][n][ldl] uint8 output (pre-filled 0xFF); labels_nh[k][idx[h][r]][h]
 *  inertia   optional [nK][H] float32; n_iter optional [nK][H] int32
 *  stats     optional [8] uint64 accumulated: {Lloyd row x centroid distance products,
 *            seeding row x candidate distance products, Lloyd M-step row updates
 *            (rows x running problems), empty-cluster relocations, sweeps,
 *            32-slot column tiles x row tiles swept}
 *  grid      workgroups (<= units; one per CU is the intended size)
 *  seedmax   problems of a unit seeding concurrently (1..32)
 *  All pointers except units_host are device pointers; X, Xhl and workspace 16-B aligned
 *  (device allocations are; CC_ERR_ARG otherwise). */
int cc_kmeans_batched(const float* X, const uint16_t* Xhl, const float* xnorm, int n, int dreal,
                      int dpad, int scale_exp, const int32_t* idx_hm, int H, int m, int h_begin,
                      int h_end, const int32_t* units, const int32_t* units_host, int nU,
                      int n_init, int max_iter, double tol_rel, const double* kpp_u,
                      int kpp_stride, const int32_t* kpp_pos, uint8_t* labels_nh, int ldl,
                      float* inertia, int32_t* n_iter, unsigned long long* stats,
                      void* workspace, size_t ws_bytes, int grid, int seedmax, void* stream);

/* Wide rows (d > 128; BASELINE config 4, n = 5k x d = 20k): the same fits, decisions and
 * outputs as cc_kmeans_batched (CC.py:282 for the default clusterer), organised as ROUNDS
 * over a batch of `batch` resamples: per round a distance-GEMM launch fused with the
 * E-step, a centre-sum GEMM launch and a per-resample bookkeeping launch, until every
 * problem is done.  The call is synchronous with respect to the host (it reads one counter
 * per round to stop).  Ks [nK] host array (nK * n_init <= CC_KM_PMAX per call); dpad any
 * multiple of 32 >= dreal; other arguments as cc_kmeans_batched; stats[4] counts
 * resample-rounds and stats[5] 256-slot column tiles x rounds. */
size_t cc_kmeans_wide_workspace_bytes(int m, int dpad, const int32_t* Ks, int nK, int n_init,
                                      int batch);
/* How to split a K list over cc_kmeans_wide calls: the number (>= 1) of leading values of
 * Ks [nK] that one call takes, the most that keep nK * n_init <= CC_KM_PMAX and fit the
 * engine's centroid capacity (8 column tiles of 256 slots; a K takes n_init * (K rounded up to
 * 4) of them and one tile is kept as packing slack).  Call it again on the rest.  Negative (an error naming K and n_init) when
 * Ks[0] fits no call on its own. */
int cc_kmeans_wide_chunk(int m, int dpad, const int32_t* Ks, int nK, int n_init);

int cc_kmeans_wide(const float* X, const uint16_t* Xhl, const float* xnorm, int n, int dreal,
                   int dpad, int scale_exp, const int32_t* idx_hm, int H, int m, int h_begin,
                   int h_end, const int32_t* Ks, int nK, int n_init, int max_iter,
                   double tol_rel, const double* kpp_u, int kpp_stride, const int32_t* kpp_pos,
                   uint8_t* labels_nh, int ldl, float* inertia, int32_t* n_iter,
                   unsigned long long* stats, void* workspace, size_t ws_bytes, int batch,
                   void* stream);

/* Float64 k-means for float64 input (the reference's clusterer at the reference's precision,
 * CC.py:282 with float64 X; sklearn/cluster/_kmeans.py restated in float64, see
 * csrc/kmeans_f64.hip).  Same fits, outputs and k-means++ tables as cc_kmeans_batched; X is
 * the raw [n][d] float64 input (the kernel centres each resample by its own mean, as
 * KMeans.fit does).  Ks [nK] is a host array (nK <= 64); one persistent workgroup per
 * (resample, K) unit (or pair of K's); inertia is float64 here.  Workspace from
 * cc_kmeans_f64_workspace_bytes(m, d, Ks, nK, grid, nh): grid workgroup areas and min(grid, nh)
 * per-resample slots for nh = h_end - h_begin (resamples beyond grid run in further launches on
 * the same stream).  X 8-B and workspace 16-B aligned. */
size_t cc_kmeans_f64_workspace_bytes(int m, int d, const int32_t* Ks, int nK, int grid, int nh);

int cc_kmeans_f64(const double* X, int n, int d, const int32_t* idx_hm, int H, int m, int h_begin,
                  int h_end, const int32_t* Ks, int nK, int n_init, int max_iter, double tol_rel,
                  const double* kpp_u, int kpp_stride, const int32_t* kpp_pos, uint8_t* labels_nh,
                  int ldl, double* inertia, int32_t* n_iter, void* workspace, size_t ws_bytes,
                  int grid, void* stream);

/* cc_kmeans_f64 under feature subsampling: resample h is fitted on its own md columns of X,
 * ascontiguousarray(X[idx[h]][:, cols[h]]) to sklearn, bit for bit what cc_kmeans_f64 gives on that
 * materialised matrix.  cols_hmd is a device int32 [H][md] (4-B aligned): row h holds the ascending
 * columns of resample h, every entry in [0, d) (the caller checks the entries: they are read as
 * given); 1 <= md <= d, and d stays the row stride of X.  Only the per-resample setup gathers; the
 * engine runs at row width md, so workspace and launch planning take md where they take d:
 * cc_kmeans_f64_workspace_bytes(m, md, ...) and cc_kmeans_launch_plan(md, ...).  Every other
 * argument is cc_kmeans_f64's, which keeps its prototype and passes no column list. */
int cc_kmeans_f64_cols(const double* X, int n, int d, const int32_t* cols_hmd, int md,
                       const int32_t* idx_hm, int H, int m, int h_begin, int h_end, const int32_t* Ks,
                       int nK, int n_init, int max_iter, double tol_rel, const double* kpp_u,
                       int kpp_stride, const int32_t* kpp_pos, uint8_t* labels_nh, int ldl,
                       double* inertia, int32_t* n_iter, void* workspace, size_t ws_bytes, int grid,
                       void* stream);

/* ---- one-call k-means (the advanced entry points above, planned internally) ----------- */

#define CC_KM_FAST 0 /* float32 input: f16 hi/lo MFMA engines (cc_kmeans_batched / _wide) */
#define CC_KM_F64 1  /* float64 input: cc_kmeans_f64 */

/* k-means++ tables of cc_kmeans_batched for Ks[0..nK) (host): sklearn KMeans(random_state=seed)
 * replays RandomState(seed) for every K; per init it draws the first centre with
 * choice(m, p=w/sum(w)) (_kmeans.py:225; unit weights, float32 unless weight_f64) and then
 * (K-1)*(2+floor(ln K)) uniforms (:243).  kpp_u [nK][n_init][kpp_stride], kpp_pos [nK][n_init]. */
int cc_kpp_tables(const int32_t* Ks, int nK, int n_init, uint32_t seed, int m, int weight_f64,
                  double* kpp_u, int kpp_stride, int32_t* kpp_pos);

/* Row image of the float32 engines from raw rows X [n][d] float32 (device): column means
 * (float64, fixed order), centred rows zero-padded to dpad (Xd [n][dpad]), squared norms
 * (xnorm [n]), the scale exponent (returned in *scale_exp; synchronises the stream) and the
 * cc_split_f16 image (Xhl [n][2][dpad]).  scratch: device, cc_prepare_rows_scratch_bytes. */
size_t cc_prepare_rows_scratch_bytes(int n, int d);
int cc_prepare_rows(const float* X, int n, int d, int dpad, float* Xd, float* xnorm, uint16_t* Xhl,
                    int* scale_exp, void* scratch, size_t scratch_bytes, void* stream);

/* Feature padding of the float32 engines' row image: 32 / 64 / 128 (cc_kmeans_batched), else the
 * next multiple of 32 (cc_kmeans_wide).  Negative for d <= 0. */
int cc_kmeans_dpad(int d);

/* *e = the operand scale exponent of cc_split_f16 for max|X| = amax: the largest e in [-62, 62]
 * with amax * 2^e <= 2^14 (0 for amax = 0).  CC_ERR_ARG when amax is not finite. */
int cc_scale_exponent(float amax, int* e);

/* One engine call of a fit, as cc_kmeans_launch_plan plans it. */
#define CC_KM_ENGINE_BATCHED 0 /* cc_kmeans_batched */
#define CC_KM_ENGINE_WIDE 1    /* cc_kmeans_wide */
#define CC_KM_ENGINE_F64 2     /* cc_kmeans_f64 */
typedef struct {
  int32_t engine;    /* CC_KM_ENGINE_* */
  int32_t k0, nk;    /* the call fits Ks[k0 .. k0 + nk) */
  int32_t par;       /* batched, f64: `grid` workgroups; wide: `batch` resamples at once */
  int32_t n_sub;     /* batched: units come from cc_kmeans_plan(Ks, nK, n_init, n_sub, ...); else 0 */
  int32_t seedmax;   /* batched: concurrent seeders; else 0 */
  uint64_t ws_bytes; /* engine workspace of the call */
} cc_km_call;

/* What is launched for the k-means of nh resamples of m rows with d features: the engine calls
 * in order, written to calls[0 .. max_calls) (nK entries always suffice).  Returns their number
 * (> 0) or a negative error.  Host arithmetic only: it touches no device, so the caller supplies
 * the CU count and the byte budgets.
 *  precision    CC_KM_FAST: one cc_kmeans_batched call (d <= 128) or the cc_kmeans_wide calls
 *               that cc_kmeans_wide_chunk deals; CC_KM_F64: cc_kmeans_f64 calls of <= 64 K values
 *  budget       engine workspace to stay within where the fit loses no speed by it; clipped to
 *  budget_hard  the bytes never to exceed.  The batched grid starts at min(cus, units) and halves
 *               until it fits the budget; a wide call runs the resamples in equal batches that
 *               fit the budget; an f64 call takes the largest grid <= min(4 cus, nh * nk) that
 *               fits max(budget, the bytes of two workgroups per CU) and budget_hard.  No rule
 *               goes below one workgroup or one resample: compare ws_bytes with what you have.
 *  n_sub, seedmax, grid  overrides (0: none) of the units per resample and the concurrent seeders
 *               of the batched call (seedmax is still capped at 32 and the largest unit) and of
 *               the f64 starting grid */
int cc_kmeans_launch_plan(int d, int m, int nh, const int32_t* Ks, int nK, int n_init, int precision,
                          int cus, size_t budget, size_t budget_hard, int n_sub, int seedmax, int grid,
                          cc_km_call* calls, int max_calls);

/* Every (resample h in [h_begin, h_end), K, init) k-means fit of a consensus fit in one call:
 * the loop of clusterer.fit_predict(X[indices]) at CC.py:282 for the default KMeans(n_init)
 * clusterer.  Builds the k-means++ tables and the row image and makes the calls of
 * cc_kmeans_launch_plan for this device and the workspace that is left (budget = budget_hard):
 * cc_kmeans_batched (d <= 128), cc_kmeans_wide (d > 128) or cc_kmeans_f64.
 *  X        device [n][d] raw rows: float32 (CC_KM_FAST) or float64 (CC_KM_F64)
 *  idx_hm   device [H][m] int32 resample rows (rows outside [h_begin, h_end) are not read)
 *  Ks       host [nK], 1 <= K <= min(127, m)
 *  labels_nh device [nK][n][ldl] uint8, pre-filled 0xFF; labels_nh[k][idx[h][r]][h]
 *  inertia  optional device [nK][H] (float32 for CC_KM_FAST, float64 for CC_KM_F64)
 *  n_iter   optional device [nK][H] int32
 *  workspace device, ws_bytes >= cc_kmeans_fit_workspace_bytes(...) (less is fine for the
 *           persistent grid, which shrinks to fit; too little for one workgroup is an error)
 * Synchronous with respect to the host (it reads max|X| and, for wide rows, a counter per
 * round).  Results are identical to driving the advanced entry points with the same inputs. */
size_t cc_kmeans_fit_workspace_bytes(int n, int d, int m, int nh, const int32_t* Ks, int nK,
                                     int n_init, int precision);
int cc_kmeans_fit(const void* X, int n, int d, const int32_t* idx_hm, int H, int m, int h_begin,
                  int h_end, const int32_t* Ks, int nK, int n_init, int max_iter, double tol_rel,
                  uint32_t seed, int precision, uint8_t* labels_nh, int ldl, void* inertia,
                  int32_t* n_iter, void* workspace, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CCMI_H */
