/*
 * lspcg.h -- C ABI of the MI355X-native PCG hot path (liblspcg_hip.so, gfx950).
 *
 * This is the drop-in boundary for the reference's native solver and GNN kernels.
 * Every entry point names the reference interface it replaces:
 *
 *   pymathprim.linalg.PreconditionedConjugateGradient(A, device, preconditioner, dtype)
 *       (unvendored; call sites neural_cg/utils/validate.py:73,79-80,110,116-117,145,151-156)
 *       -> lspcg_solver_create / lspcg_solver_set_spai / lspcg_solver_solve
 *   scipy csr_matvec inside the PCG (validate.py:102, 182)      -> lspcg_spmv
 *   neural_cg/utils/validate.py:22-51 to_csr_cpu
 *       + neural_cg/data.py:134-170 (make_bsr_from_coo_inds, apply_dbc_masking)
 *                                                                -> lspcg_assemble
 *   csr_matrix(spai.T) (validate.py:176)                         -> lspcg_mat_transpose
 *   A.diagonal() (validate.py:243, 280)                          -> lspcg_mat_diagonal
 *   csr @ diags(rsqrt_diag) (scaled_workspace.py:210-211)        -> lspcg_mat_scale_columns
 *   neural_cg/nn/gnns.py:77-97 NodeEdgeProcessing.forward
 *       (+ basic_layers.py:73-109 FeedForward, :145-225 MPLayer) -> lspcg_gnn_forward
 *   neural_cg/nn/basic_layers.py:112-142 GraphSpmv.forward        -> lspcg_graph_spmv
 *   neural_cg/nn/basic_layers.py:228-261 AATPE.forward            -> lspcg_graph_aatpe
 *       (edge lists prepared once by lspcg_graph_create)
 *   neural_cg/utils/optim.py:4-12 create_optimizer (torch.optim.SGD / Adam / AdamW) + Lightning's
 *       gradient_clip_val (clip_grad_norm_, config/trainer.yaml)  -> lspcg_optim_step
 *
 * Conventions: plain pointers and sizes only.  Vector arguments of compute calls are
 * DEVICE pointers; matrix/weight uploads accept host or device pointers.  All work is
 * issued on the context's stream.  Every call returns LSPCG_OK (0), LSPCG_NOT_CONVERGED
 * (1, solve only) or a negative error code; lspcg_last_error() describes the last error
 * of the calling thread.
 */
#ifndef LSPCG_H_
#define LSPCG_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSPCG_OK 0
#define LSPCG_NOT_CONVERGED 1
#define LSPCG_ERR_ARG (-1)
#define LSPCG_ERR_HIP (-2)
#define LSPCG_ERR_UNSUPPORTED (-3)
#define LSPCG_ERR_FORMAT (-4)
#define LSPCG_ERR_BREAKDOWN (-5) /* incomplete factorization hit a non-positive pivot */
#define LSPCG_ERR_SINGULAR (-6)  /* a given triangular factor has a zero diagonal entry */

#define LSPCG_F32 0
#define LSPCG_F64 1

/* preconditioner kinds (pymathprim names: none / diagonal / ext_spai / ext_spai_scaled) */
#define LSPCG_PRECOND_NONE 0
#define LSPCG_PRECOND_DIAGONAL 1
#define LSPCG_PRECOND_EXT_SPAI 2
#define LSPCG_PRECOND_EXT_SPAI_SCALED 3
/* IC(0) of A, applied by two sync-free triangular solves (pymathprim "ic") */
#define LSPCG_PRECOND_IC 4

/* dot-product summation order of the PCG loop (lspcg_solver_set_dot_order) */
#define LSPCG_DOT_COMPENSATED 0 /* default: compensated (Dot2) dots in a fixed tree, ~correctly rounded */
#define LSPCG_DOT_OPENBLAS 1    /* parity mode: numpy's ddot as recorded (OpenBLAS 0.3.29 SkylakeX) */

typedef struct lspcg_ctx lspcg_ctx;
typedef struct lspcg_mat lspcg_mat;
typedef struct lspcg_solver lspcg_solver;
typedef struct lspcg_gnn lspcg_gnn;
typedef struct lspcg_graph lspcg_graph;

const char* lspcg_last_error(void);
int lspcg_version(void);
/* provenance: hash of the sources, headers, compiler flags and arch this library was built from
 * (learningsparsepreconditioner4gpu_amd/_build.py tree_hash) */
const char* lspcg_build_id(void);

/* ---- context: one per GPU per host thread; stream NULL = the default (null) stream ---- */
int lspcg_ctx_create(int device, void* stream, lspcg_ctx** out);
int lspcg_ctx_destroy(lspcg_ctx* ctx);
int lspcg_ctx_synchronize(lspcg_ctx* ctx);

/* ---- sparse matrices (device copies owned by the handle) ---- */
/* scalar CSR, n x n, int32 indptr[n+1] / indices[nnz], vals[nnz] of dtype */
int lspcg_mat_create_csr(lspcg_ctx* ctx, int64_t n, int64_t nnz, const int32_t* indptr,
                         const int32_t* indices, const void* vals, int dtype, lspcg_mat** out);
/* block CSR, nb x nb blocks of bs x bs (bs in {1,3}), vals[nnzb][bs][bs] row-major */
int lspcg_mat_create_bsr(lspcg_ctx* ctx, int64_t nb, int64_t nnzb, int bs, const int32_t* indptr,
                         const int32_t* indices, const void* vals, int dtype, lspcg_mat** out);
int lspcg_mat_destroy(lspcg_mat* A);
/* n = scalar rows, nnzb = stored blocks (= scalar nnz when bs == 1) */
int lspcg_mat_info(const lspcg_mat* A, int64_t* n, int64_t* nnzb, int* bs, int* dtype);
/* copy the handle's arrays out (host or device destinations; NULL skips an array) */
int lspcg_mat_copy_out(const lspcg_mat* A, int32_t* indptr, int32_t* indices, void* vals);
/* New values for an existing matrix of the same pattern (a time step or a sample on a fixed mesh:
 * the reference's is_fixed_topology datasets): vals (host or device, of `dtype` = A's dtype)
 * overwrites A's nnzb*bs*bs values in A's stored order.  indptr / indices (host or device, either
 * may be NULL = not checked) are compared with A's on the device first; a difference returns
 * LSPCG_ERR_FORMAT and nothing is written.  A dtype other than A's is LSPCG_ERR_ARG.  The copy a
 * lspcg_mat_prepare_spmv attached is refilled in place -- same kind, same permutation when it was
 * analysed on P A P^T -- and lspcg_spmv keeps scipy's bits on the new values.  No solve may be
 * running on A; a solver created on A must see lspcg_solver_update_matrix before its next solve. */
int lspcg_mat_set_values(lspcg_mat* A, const int32_t* indptr, const int32_t* indices, const void* vals,
                         int dtype);
/* explicit transpose (sorted), replaces csr_matrix(spai.T) of validate.py:176 */
int lspcg_mat_transpose(const lspcg_mat* A, lspcg_mat** out);
/* d[i] = A[i,i] (0 where absent), device pointer of the matrix dtype, length n */
int lspcg_mat_diagonal(const lspcg_mat* A, void* d);
/* A <- A diag(d): column scaling, d device pointer of the matrix dtype, length n */
int lspcg_mat_scale_columns(lspcg_mat* A, const void* d);
/* The solver's reordering analysis on its own (DESIGN.md §2 "Reordering"): perm (device int32,
 * one entry per block row) <- the reverse Cuthill-McKee order of A's block graph, new row i' = old row
 * perm[i'] (isolated rows -- empty or diagonal-only -- last, each component from a pseudo-peripheral
 * node, children by (row length, index)); *applied = 0 and perm untouched when the graph is left in
 * its order (more than 256 non-trivial components, a row longer than 1024 blocks, or a row whose
 * columns are not strictly increasing).  Mean |col -
 * row| before / after (either pointer may be NULL). */
int lspcg_mat_rcm(const lspcg_mat* A, int32_t* perm, int* applied, double* mean_offset_before,
                  double* mean_offset_after);

/* ---- the GNN's input sample of a matrix on the device (neural_cg/data.py:218-336 make_data) ----
 * A: scalar CSR or BSR 3x3, fp32 or fp64, rows sorted (what lspcg_mat_diagonal requires).  Below
 * E = nnzb, b = block size, nb = block rows, v = a stored value widened to double. */
#define LSPCG_NORM_NONE 0
#define LSPCG_NORM_MEAN 1
#define LSPCG_NORM_FROB 2
#define LSPCG_NORM_L1 3
#define LSPCG_REDUCE_DISABLE 0
#define LSPCG_REDUCE_SUM 1
#define LSPCG_REDUCE_MEAN 2
#define LSPCG_REDUCE_MAX 3
#define LSPCG_REDUCE_MIN 4
typedef struct lspcg_sample_desc {
  int normalize;             /* LSPCG_NORM_*   (make_data's normalize_matrix) */
  int mask_as_node_feature;  /* 0 / 1 */
  int edge_reduce;           /* LSPCG_REDUCE_* (use_edge_features_as_node_feature) */
  int node_in;               /* columns of node_features (0: none) */
} lspcg_sample_desc;

/* edge_index (device int64 [2][nnzb]) <- the block COO of A in stored (row-major) order */
int lspcg_mat_edge_index(const lspcg_mat* A, int64_t* edge_index);

/* make_data of A's block graph; every pointer is a device pointer, the work is issued on ctx's
 * stream and nothing synchronises except an allocation on first use.
 *   scale (one DEVICE double, read from there by the later passes): none 1; mean
 *     1 / (sum|v| / double(E b b)); frob 1 / sqrt(sum v^2), both sums compensated in a fixed order
 *     (chunks of 4096 values, then one workgroup) that depends on neither grid nor device, without
 *     floating-point atomics: the same bits on every call; l1 (b = 1 only, LSPCG_ERR_UNSUPPORTED for
 *     b = 3) 1 / (max_i sum_j |v_ij| + 1e-7), each row a sequential sum in stored order (scipy's).
 *   edge_attr[e][b*a+c] = float(scale * v) (also the sample's matrix_values);
 *   diagonal = float(A_ii * scale) (0 where no diagonal is stored), inv_diag = float(1 / (A_ii *
 *     scale + 1e-7)), rsqrt_diag = float(1 / sqrt(A_ii * scale + 1e-7)): [nb*b] each, given together
 *     or all NULL; every value computed in double and rounded once.
 *   x[nb][F_in] = [node_features (node_in columns) | mask (b columns, when the flag is set; NULL
 *     mask = ones; mask_dtype LSPCG_F32 / LSPCG_F64, [nb*b]) | reduce (b*b columns, when enabled)],
 *     F_in = node_in + flag*b + (reduce ? b*b : 0).  The reduce is PyG's scatter(edge_attr,
 *     edge_index[1]): for node j over the edges with block column j in ascending edge order --
 *     sum: sequential fp32 adds from 0.0f; mean: that sum / max(count, 1) in fp32; max / min over
 *     those edges; 0 for a node without incoming edges; no atomics.  The edges grouped by
 *     destination are built at the first reducing call and stay attached to A (the pattern cannot
 *     change under lspcg_mat_set_values / lspcg_assemble_into).
 * LSPCG_ERR_ARG before any launch: E = 0 or nb = 0, an unknown code, node_in > 0 with NULL
 * node_features, F_in = 0. */
int lspcg_mat_sample(lspcg_ctx* ctx, lspcg_mat* A, const lspcg_sample_desc* desc, const void* mask,
                     int mask_dtype, const float* node_features, float* x, float* edge_attr,
                     float* diagonal, float* inv_diag, float* rsqrt_diag, double* scale);

/* ---- kernels ---- */
/* y = A x (scipy csr_matvec bit pattern: per-row sequential sum in index order).  x and y must not
 * overlap.  After a reordering lspcg_mat_prepare_spmv (lspcg_mat_spmv_reorder_info) the call gathers x
 * into a scratch vector owned by A, so calls on one matrix must run on one stream at a time. */
int lspcg_spmv(lspcg_ctx* ctx, const lspcg_mat* A, const void* x, void* y);
/* analysis step (cf. rocSPARSE csrmv_analysis): attach a SELL-64 copy of a scalar CSR matrix, or
 * the BSELL-64 block copy of a BSR 3x3 (one column per block, block values in 16-B lane chunks), with the
 * same values and dtype and 16-bit column offsets where they fit, that lspcg_spmv then uses -- the
 * results keep the same bits.  *kind (nullable) = the column storage: 1 (SELL-DIA: a sorted scalar
 * CSR whose 64-row slices have <= 16 distinct row-relative offsets col - row, one value slot per
 * offset and a lane mask per slot, no column array), 16 (16-bit offsets from the slice's first row), 17
 * (SELL-64J: lanes sorted by row length, each 4-entry group stored for its active lanes only), 18
 * (SELL-64X: SELL-64J reading x from an LDS copy of each 256-row tile's blocks), 32 (int32
 * columns), or 0 when the matrix stays on the CSR / BSR kernel (irregular row lengths).  A numbering
 * far from banded (the solver's rule: mean |col - row| > 4 n^(2/3), n >= 16384, env LSPCG_REORDER) is
 * analysed on P A P^T, P the device reverse Cuthill-McKee permutation, every row's entries in their
 * original order; lspcg_spmv then gathers x into that numbering and scatters y back (same bits).
 * lspcg_mat_scale_columns drops it. */
int lspcg_mat_prepare_spmv(lspcg_mat* A, int* kind);
/* the analysis step's reordering (lspcg_mat_prepare_spmv): *applied = 1 when the SpMV runs on
 * P A P^T; mean |col - row| before / after (either pointer may be NULL).  Replaces nothing in the
 * reference (its SpMV is scipy's, on the caller's numbering). */
int lspcg_mat_spmv_reorder_info(const lspcg_mat* A, int* applied, double* mean_offset_before,
                                double* mean_offset_after);
/* average device ms of one SpMV launch, HIP events on the ctx stream.  flush_bytes == 0:
 * reps back-to-back launches (warm caches); > 0: before every launch a read of a flush_bytes
 * buffer evicts the 256 MiB Infinity Cache (cold); the launch time is (reps x (flush + SpMV)
 * - reps x flush) / reps, i.e. the in-stream duration without per-event overhead. */
int lspcg_spmv_timed(lspcg_ctx* ctx, const lspcg_mat* A, const void* x, void* y, int reps,
                     int64_t flush_bytes, double* avg_ms);
/* diagnostics: time SpMV launch configuration `variant` (fp64 scalar CSR; see csrc/lspcg_core.hip
 * kSpmvVariants) exactly like lspcg_spmv_timed; variant < 0 returns the number of variants */
int lspcg_spmv_variant_timed(lspcg_ctx* ctx, const lspcg_mat* A, int variant, const void* x, void* y,
                             int reps, int64_t flush_bytes, double* avg_ms);
/* diagnostics: the same timing for the SELL-64 kernel the PCG loop uses (csrc/lspcg_sell.hpp) on a
 * SELL copy of A built inside the call (fp64 scalar CSR).  flags bit 0: store the values as fp32
 * (lossless only when every value is fp32-representable); bit 1: 16-bit column offsets where they
 * fit; bit 3: SELL-DIA where it fits (tried before bit 1); bit 4 (with bit 1): SELL-64J (view kind
 * 17) where 16-bit offsets fit, SELL-64 would store more than 1.15 x nnz slots and no row has more
 * than 64 entries; bit 5 (with bit 4, without bit 2): SELL-64X (kind 18) on top of it from
 * LSPCG_SELLX_MIN_N rows (default 262144) where every 256-row tile reads <= 256 x blocks; bit 2
 * (experiment): gather x from an interleaved (x, x) pair array with one 16-B load per entry, the cost
 * model of a fused update evaluated in the gather.  No padding limit applies.  y = A x, same bits as
 * lspcg_spmv */
int lspcg_spmv_sell_timed(lspcg_ctx* ctx, const lspcg_mat* A, int flags, const void* x, void* y,
                          int reps, int64_t flush_bytes, double* avg_ms);
/* calibration: the same cold / warm timing for a plain streaming read of `bytes` (16-B loads, 8
 * workgroups per CU): the achievable bandwidth an SpMV of that many bytes is compared against */
int lspcg_read_timed(lspcg_ctx* ctx, int64_t bytes, int reps, int64_t flush_bytes, double* avg_ms);
/* ---- baseline preconditioners (pymathprim "ic" / "ainv", infer.py:310-321; algorithms and
 * operation order: oracle/precond.py; scalar CSR, sorted rows, stored diagonal) ---- */
/* IC(0): *L = lower-triangular factor with the pattern of tril(A), A ~ L L^T */
int lspcg_ic0(const lspcg_mat* A, lspcg_mat** L, double* t_ms);
/* AINV(0): *L = Z D^{-1/2} (Z unit upper, pattern triu(A)) so that L L^T = Z D^{-1} Z^T ~ A^{-1};
 * use it as an ext_spai factor with epsilon = 0 */
int lspcg_ainv0(const lspcg_mat* A, lspcg_mat** L, double* t_ms);
/* x = T^{-1} b, T triangular (lower != 0: diagonal stored last in each row; else first), in the
 * arithmetic of scipy's spsolve_triangular on csc(T) -- the reference's IC apply
 * (validate.py:359-365): column-scaled unit solve, updates in SuperLU's column order, diagonal
 * scaling after; one sync-free launch over the level-ordered rows; b, x device vectors of T's
 * dtype */
int lspcg_trsv(const lspcg_mat* T, int lower, const void* b, void* x);
/* compensated, deterministic dot product of two device vectors; result to host */
int lspcg_dot(lspcg_ctx* ctx, int64_t n, int dtype, const void* x, const void* y, double* out);

/* ---- PCG solver (pymathprim.linalg.PreconditionedConjugateGradient) ---- */
int lspcg_solver_create(lspcg_ctx* ctx, const lspcg_mat* A, int precond, lspcg_solver** out);
/* ext_spai=(L, eps): builds Lᵀ (and diag(A) for the scaled variant) on device.
 * t_prec_ms (nullable) receives the device time of that setup. L must outlive solves. */
int lspcg_solver_set_spai(lspcg_solver* s, const lspcg_mat* L, double epsilon, double* t_prec_ms);
/* LSPCG_PRECOND_IC solvers: IC(0) factorization of A on the device (pymathprim "ic" setup;
 * the reference's scipy twin is validate.py:344-429); t_prec_ms = setup time */
int lspcg_solver_set_ic(lspcg_solver* s, double* t_prec_ms);
/* LSPCG_PRECOND_IC solvers: install a given lower-triangular factor L (scalar CSR of the solver's
 * size and dtype, sorted rows, diagonal stored last) and apply M^-1 = L^-T L^-1 -- the
 * reference's IncompleteCholeskyPreconditioner(L) of get_pcg_iter_time_scipy_ichol
 * (validate.py:344-419, which takes an external L).  L is copied. */
int lspcg_solver_set_ic_factor(lspcg_solver* s, const lspcg_mat* L, double* t_prec_ms);
/* The values of the solver's A handle changed in place (lspcg_mat_set_values, lspcg_assemble_into),
 * the pattern did not.  Drains the solver's stream and redoes what depends on values: P A P^T through
 * the kept permutation; the fp32 copy of the values, or the switch to or from it when their
 * fp32-exactness changed; the SELL / BSELL value arrays, in place; d for LSPCG_PRECOND_DIAGONAL and
 * _EXT_SPAI_SCALED.  Kept: the reverse Cuthill-McKee analysis, the SELL pattern, the split
 * reductions' geometry, the vectors, stream and events.  LSPCG_PRECOND_IC with the factor computed
 * here (lspcg_solver_set_ic): a numeric-only IC(0) into the existing factor, its transpose and the
 * triangular solves' scaled values; the levels, padded orders and counter words are kept.  A given
 * factor (lspcg_solver_set_ic_factor) and an installed ext_spai L are left alone: install the new L
 * with lspcg_solver_set_spai.  The results are those of a solver created on the new values, bit for
 * bit.  t_ms (nullable) = device time of the update; *graphs_kept (nullable) = 1 when the captured
 * iteration graphs of lspcg_solver_solve and lspcg_solver_solve_multi survived, which they do exactly
 * when no view moved or changed its storage type (0 across a change of fp32-exactness).  A call that
 * returns an error has dropped the graphs (views may have moved before the failing step), and the
 * successful call after it reports 0.
 * LSPCG_ERR_BREAKDOWN from the numeric IC(0) (a non-positive pivot) leaves no usable factor: every
 * solve returns LSPCG_ERR_BREAKDOWN until another lspcg_solver_update_matrix succeeds. */
int lspcg_solver_update_matrix(lspcg_solver* s, double* t_ms, int* graphs_kept);
/* Solve A x = b from x (x0, in/out).  Semantics of scipy.sparse.linalg.cg (iterative.py
 * 359-418): atol = rtol*||b||, ||r|| checked at the top of each iteration, iters = number
 * of completed iterations, max_iter <= 0 means n.  res_hist (host, nullable, length
 * max_iter+2) receives ||r_k|| for k = 0..iters.  t_solve_ms = device time of the solve.
 * Returns LSPCG_OK when converged, LSPCG_NOT_CONVERGED when max_iter was reached.
 * Scalar systems with n <= LSPCG_SMALL_N (env read at solver creation; default 3072, 0 = off;
 * at most 3 rows per thread of 1024 and 3 vectors in 60 KiB of LDS: 2560 in fp64; IC excluded)
 * run the whole loop in one single-workgroup launch -- same bits as the multi-kernel schedule. */
int lspcg_solver_solve(lspcg_solver* s, const void* b, void* x, double rtol, int64_t max_iter,
                       int64_t* iters, double* res_hist, double* t_solve_ms);
/* lspcg_solver_solve that also records the loop's scalars: coef (host, nullable, 2*(max_iter+1)
 * doubles) receives the `iters` pairs coef[2k] = rho_k = r_k.z_k, coef[2k+1] = pi_k = p_k.q_k -- the
 * rounded values the recurrence itself divides for alpha_k, stored by the thread that commits
 * iteration k, in every schedule, preconditioner kind, dtype and dot order.  They are the Lanczos
 * coefficients of M^-1 A (lspcg_cg_lanczos).  A solve stopped by a non-finite residual reports
 * max_iter iterations and NaN for the pairs it did not complete.  coef == NULL is
 * lspcg_solver_solve: the same launches, the same bits in x, iters and res_hist. */
int lspcg_solver_solve_coef(lspcg_solver* s, const void* b, void* x, double rtol, int64_t max_iter,
                            int64_t* iters, double* res_hist, double* t_solve_ms, double* coef);
/* Solve A X = B for nrhs = 1..8 right-hand sides of the one system in one lockstep loop (heat time
 * steps on a fixed mesh, load cases, a repeated sample).  B, X: device arrays
 * [n][nrhs], row-major and contiguous, of the solver's dtype; X holds x0 on entry and the
 * solutions on return.  Column j comes out as lspcg_solver_solve returns it for (B[:,j], X[:,j])
 * alone on this solver: scipy cg's recurrence with the column's own scalars, top-of-loop test,
 * count, history and status (count, status and history equal; iterate within the compensated
 * dots' rounding).  A zero column is done at the init, a column with a non-finite residual stops
 * alone, and a finished column is frozen while the others run.  The columns share every launch
 * and every load of A, L and Lᵀ: the vectors are stored interleaved [n][Kp], Kp = 2, 4 or 8.
 * iters[j], status[j] (LSPCG_OK / LSPCG_NOT_CONVERGED) and res_hist[j] (host arrays of max_iter + 2
 * entries; res_hist or any entry may be NULL) describe column j as lspcg_batch_solve reports its
 * systems; max_iter <= 0 means n.  Returns LSPCG_OK when every column converged,
 * LSPCG_NOT_CONVERGED when any reached max_iter.
 * LSPCG_ERR_ARG: nrhs outside 1..8.  LSPCG_ERR_UNSUPPORTED (the message names the reason): any
 * preconditioner but LSPCG_PRECOND_EXT_SPAI / _EXT_SPAI_SCALED, block size 3, the OpenBLAS dot
 * order, a reordered solver, or iteration views (lspcg_solver_views) other than SELL-DIA (1) and
 * SELL-64 with 16- or 32-bit columns (16, 32).  nrhs == 1 is lspcg_solver_solve. */
int lspcg_solver_solve_multi(lspcg_solver* s, int nrhs, const void* B, void* X, double rtol, int64_t max_iter,
                             int64_t* iters, int32_t* status, double* const* res_hist, double* t_solve_ms);
/* Measurement only (bench.py): `iters` iterations of the split ext_spai schedule from x0 = 0,
 * each of the five launches bracketed by HIP events on the solver stream (no graph, no
 * convergence stop); kernel_ms[0..4] = mean device time of KA (t = Lᵀr), KB (z = Lt + εr, ρ),
 * UP (p, x), KC (q = Ap, π), UR (r); *nk = 5.  LSPCG_ERR_UNSUPPORTED for other schedules. */
int lspcg_solver_time_kernels(lspcg_solver* s, const void* b, int64_t iters, double* kernel_ms, int* nk);
/* Summation order of every dot / norm of the loop (scipy cg's np.dot / np.linalg.norm,
 * iterative.py:398-418).  LSPCG_DOT_COMPENSATED (default): split / one-workgroup schedules,
 * ~correctly rounded.  LSPCG_DOT_OPENBLAS: parity mode, fp64 only -- each dot is recomputed in
 * the order of numpy's cblas_ddot in the container that recorded the reference's trajectories
 * (OpenBLAS 0.3.29 SkylakeX kernel, split over `threads` (1..16) OpenBLAS threads when n > 10000;
 * restated in oracle/openblas_ddot.c) by one extra single-workgroup launch after each reducing
 * launch, on the last-arriver multi-kernel schedule: the solve then reproduces the reference's
 * recorded count, ||r_k|| history and x bit for bit.  Measurement: DESIGN.md §3. */
int lspcg_solver_set_dot_order(lspcg_solver* s, int order, int threads);
/* Bandwidth-reducing analysis step (no reference counterpart; cf. scipy's reverse_cuthill_mckee
 * before a solve): a solver whose A is numbered far from banded (mean |col - row| > 4 n^(2/3),
 * n above the one-workgroup bound) runs the loop on P A Pᵀ, P Lᵀ Pᵀ, P L Pᵀ with P a reverse
 * Cuthill-McKee permutation, every row's entries kept in their original order -- the same row
 * sums bit for bit -- with b / x permuted on the device around the loop.  Environment
 * LSPCG_REORDER = 0 (never) / 1 (always) / auto.  Not for IC, batches or the OpenBLAS dot order
 * (which switches a reordered solver back).  *applied = 1 if the solver runs permuted;
 * mean |col - row| before / after (either pointer may be NULL). */
/* The iteration views the solver built for A (0), L (1), Lᵀ (2): col_kind[w] = 0 (staged CSR kernel),
 * 1 (SELL-DIA: no column array), 16 / 32 (SELL-64 with 16-bit / int32 columns), 8 (SELL-64C: one-byte
 * codes into per-slice dictionaries of <= 64 row-relative offsets, 16-bit columns for slices with
 * more; unstructured orderings, LSPCG_SELLC=0 turns it off), 17 (SELL-64J: unstructured meshes, each
 * slice's rows sorted by length, no padded slots), 18 (SELL-64X: SELL-64J reading x through the row
 * tile's LDS-staged blocks); value_bytes[w] = 8 (fp64), 4 (fp64 matrix stored exactly as fp32),
 * 0 (no view).  Same bits in every case. */
int lspcg_solver_views(const lspcg_solver* s, int* col_kind, int* value_bytes);
int lspcg_solver_reorder_info(const lspcg_solver* s, int* applied, double* mean_offset_before,
                              double* mean_offset_after);
int lspcg_solver_destroy(lspcg_solver* s);

/* ---- batched lockstep PCG over independent systems (infer.py:278-331 solves its samples one
 * after another, each a get_pcg_iter_time / get_cg_iter_time call, validate.py:54-160; this solves
 * a window of them with every launch covering all systems -- DESIGN.md §6).  Each system keeps
 * scipy cg's recurrence, its own scalars, top-of-loop test and iteration count: the result per
 * system is what lspcg_solver_solve returns for it alone with the same preconditioner kind (count,
 * status and history equal; iterate within the compensated dots' rounding, same bits in practice).
 * A[k], L[k]: nsys >= 1 matrices of one dtype and block size (L[k] the ext_spai factor of A[k]);
 * the handles must outlive the batch only until the create call returns (their entries are copied
 * into a block-diagonal system whose per-system row ranges are padded to whole 256-row workgroup
 * tiles; padding rows are empty, stay 0 in every vector and get d = 1 where a kind divides by
 * diag(A)).
 * Windows whose systems all fit the one-workgroup solve (n <= 2560 in fp64) run it with one
 * workgroup per system in one launch; others run the phases in lockstep: five launches per
 * iteration (KA, KB, UP, KC, UR) for the two ext_spai kinds, three (UP, KC, UR -- UR also reduces
 * the next iteration's dots per system) for none / diagonal.
 * LSPCG_ERR_UNSUPPORTED when a SELL view cannot be built (irregular rows): solve one by one.
 *
 * lspcg_batch_create_precond: precond is LSPCG_PRECOND_NONE, _DIAGONAL, _EXT_SPAI or
 * _EXT_SPAI_SCALED; LSPCG_PRECOND_IC returns LSPCG_ERR_UNSUPPORTED (triangular solves do not fit
 * the tile-per-workgroup scheme).  L is required for the two ext_spai kinds (L[k] of A[k]'s size)
 * and must be NULL for none / diagonal, where epsilon is ignored.  lspcg_batch_create is the
 * LSPCG_PRECOND_EXT_SPAI case. */
typedef struct lspcg_batch lspcg_batch;
int lspcg_batch_create(lspcg_ctx* ctx, int nsys, const lspcg_mat* const* A, const lspcg_mat* const* L,
                       double epsilon, lspcg_batch** out);
int lspcg_batch_create_precond(lspcg_ctx* ctx, int nsys, const lspcg_mat* const* A, const lspcg_mat* const* L,
                               int precond, double epsilon, lspcg_batch** out);
/* b[k], x[k]: device vectors of system k (x in: x0, out: solution).  max_iter <= 0: each
 * system's own n.  iters[k], status[k] (LSPCG_OK converged / LSPCG_NOT_CONVERGED) per system;
 * res_hist (nullable): per-system host arrays of length max_iter_k + 2 (or NULL entries);
 * t_solve_ms = device time of the whole batch.  Returns LSPCG_OK when every system converged. */
int lspcg_batch_solve(lspcg_batch* bt, const void* const* b, void* const* x, double rtol, int64_t max_iter,
                      int64_t* iters, int32_t* status, double* const* res_hist, double* t_solve_ms);
/* lspcg_batch_solve that also records every system's (rho_k, pi_k) pairs as lspcg_solver_solve_coef
 * does: coef (nullable) holds per-system host arrays of 2*(max_iter_k+1) doubles (or NULL entries). */
int lspcg_batch_solve_coef(lspcg_batch* bt, const void* const* b, void* const* x, double rtol, int64_t max_iter,
                           int64_t* iters, int32_t* status, double* const* res_hist, double* t_solve_ms,
                           double* const* coef);
/* New values of A and / or L on a live batch, same patterns (the next window of an is_fixed_topology
 * folder, the next time step on fixed meshes).  A, L: arrays of nsys handles; either array may be
 * NULL (those values stay) and any entry may be NULL (that system's matrix stays); L must be NULL
 * for none / diagonal batches.  epsilon replaces the batch's (ignored for none / diagonal).  The
 * handles are read during the call only.
 * Checked on the host before any launch: a given matrix of another dtype, or L given to a batch that
 * takes none, is LSPCG_ERR_ARG; another block size, size or entry count is LSPCG_ERR_FORMAT.  Then
 * ONE launch compares every given rowptr / colind with the system's slice of the block-diagonal
 * copy and one flag is read back: any difference in any system is LSPCG_ERR_FORMAT and nothing has
 * been written -- not the systems before the offending one, not any L -- so the batch still solves
 * its old systems, bit for bit.
 * After the checks one launch copies all given values into the block-diagonal copies in place, the
 * batch's stream is drained, and what depends on values is redone on the internal solver: for a new A
 * what lspcg_solver_update_matrix redoes (the fp32 copy of the values or the switch to or from it,
 * the SELL / BSELL value arrays in place, d for LSPCG_PRECOND_DIAGONAL and _EXT_SPAI_SCALED, 1 on
 * padding rows), for a new L or epsilon what lspcg_solver_set_spai redoes (L^T and the views of L
 * and L^T, in place).  Kept: the block-diagonal patterns, the SELL patterns, the tile maps, tickets,
 * partials, states, stream and events, the one-workgroup / lockstep and sums / tickets decisions.
 * The results are those of a batch created on the resulting matrices, bit for bit.
 * t_ms (nullable) = device time of the update, checks included; *graphs_kept (nullable) = 1 when the
 * captured iteration graphs of lspcg_batch_solve survived, which they do exactly when no view moved
 * or changed its storage type and epsilon is the same (0 across a change of the concatenated
 * values' fp32-exactness, or of epsilon).  A call that fails after its checks (an allocation, a HIP
 * error) has dropped the graphs; solves return that error until an update succeeds, and that update
 * reports graphs_kept = 0. */
int lspcg_batch_update(lspcg_batch* bt, const lspcg_mat* const* A, const lspcg_mat* const* L,
                       double epsilon, double* t_ms, int* graphs_kept);
/* The iteration views of the batch's block-diagonal A (0), L (1), L^T (2), as lspcg_solver_views
 * reports a solver's: col_kind[w], value_bytes[w]. */
int lspcg_batch_views(const lspcg_batch* bt, int* col_kind, int* value_bytes);
int lspcg_batch_destroy(lspcg_batch* bt);

/* ---- spectrum of the preconditioned system from the PCG scalars (host only: no device call) ----
 * CG is Lanczos on M^-1 A: with alpha_k = rho_k/pi_k and beta_k = rho_k/rho_{k-1}, the m recorded
 * pairs give the m x m tridiagonal T_m whose extreme eigenvalues (Ritz values) converge to those of
 * M^-1 A as the solve converges (Golub & Van Loan, Matrix Computations, sec. 11.3; Saad, Iterative
 * Methods for Sparse Linear Systems, sec. 6.7; PETSc's KSPComputeExtremeSingularValues on its CG).
 * lspcg_cg_lanczos: diag[0] = pi_0/rho_0, diag[k] = pi_k/rho_k + (rho_k/rho_{k-1}) pi_{k-1}/rho_{k-1},
 * off[k] = sqrt(rho_{k+1}/rho_k) pi_k/rho_k for k < m-1 (diag: m doubles, off: m-1, may be NULL for
 * m == 1).  LSPCG_ERR_ARG for m < 1, a NULL array, or a rho / pi that is not positive and finite (a
 * breakdown, or an operator that is not SPD): never a silent NaN. */
int lspcg_cg_lanczos(int64_t m, const double* coef, double* diag, double* off);
/* Smallest and largest eigenvalue of the symmetric tridiagonal (diag[m], off[m-1]): Sturm-count
 * bisection of the Gershgorin interval in double, down to adjacent doubles.  LSPCG_ERR_ARG for
 * m < 1, a NULL array or a non-finite entry. */
int lspcg_tridiag_extremes(int64_t m, const double* diag, const double* off, double* lmin, double* lmax);

/* ---- CSR assembly with Dirichlet masking (to_csr_cpu on device) ----
 * edge_index: device int64 [2,E] (row-major sorted, duplicate free -- checked);
 * blocks: device [E,bs,bs] of in_dtype; mask: device [nb*bs] of mask_dtype or NULL.
 * out_block = 0: scalar CSR exactly as to_csr_cpu (zeros dropped, sorted);
 * out_block = 1: BSR (bs x bs blocks, masking applied, zeros kept) for the block kernels. */
int lspcg_assemble(lspcg_ctx* ctx, int64_t nb, int64_t E, int bs, const int64_t* edge_index,
                   const void* blocks, int in_dtype, const void* mask, int mask_dtype,
                   int out_dtype, int out_block, lspcg_mat** out);
/* lspcg_assemble into an existing handle A (its dtype is the output dtype): the same masking and
 * the same zero dropping, and the values are written only if the resulting rowptr / colind equal
 * A's.  Otherwise -- another mask, a block value that became exactly 0 (scalar output drops it),
 * another size -- LSPCG_ERR_FORMAT, and A is left bit for bit as it was.  No host copy of the
 * pattern: the count pass's row pointer and the fill pass's columns land in scratch arrays that
 * are compared with A's on the device, with one flag read.  A lspcg_mat_prepare_spmv copy is
 * refilled as by lspcg_mat_set_values; the same rules for running solves and solvers apply. */
int lspcg_assemble_into(lspcg_ctx* ctx, int64_t nb, int64_t E, int bs, const int64_t* edge_index,
                        const void* blocks, int in_dtype, const void* mask, int mask_dtype,
                        int out_block, lspcg_mat* A);

/* ---- GNN (NodeEdgeProcessing, F = hidden = 16, FeedForward num_layers = 2) ---- */
typedef struct lspcg_gnn_desc {
  int node_in;        /* node input features (x.shape[1]) */
  int edge_in;        /* edge input features (edge_attr.shape[1]) */
  int hidden;         /* node_features = edge_features = MLP hidden channels (16) */
  int mlp_layers;     /* FeedForward num_layers (2 -> three Linear layers) */
  int num_mp_layers;  /* MPLayer count (4) */
  int edge_out;       /* block_size * block_size */
  int node_residual;  /* gnn.yaml node_residual */
  int edge_residual;  /* gnn.yaml edge_residual */
} lspcg_gnn_desc;

/* weights: packed fp32 blob in the order documented in learningsparsepreconditioner4gpu_amd/nn.py
 * (pack_weights); host or device pointer.  The MLP products run as fp32-accurate split-f16 GEMMs
 * (raw edge features of any magnitude are scaled per edge inside); weights whose LayerNorm-fed MLPs
 * bound their hidden activations at 2^15 or more -- past f16's range -- select the fp32-MFMA
 * kernels instead (environment LSPCG_GNN_F32=1 forces them).  Any weights run. */
int lspcg_gnn_create(lspcg_ctx* ctx, const lspcg_gnn_desc* desc, const float* weights,
                     int64_t nweights, lspcg_gnn** out);
/* Structure analysis of a graph (its CSC by destination), like a sparse library's analysis step:
 * lspcg_gnn_forward reuses it while it is called with the same (edge_index pointer, N, E) -- the
 * reference runs `repeat` forwards of one sample (infer.py:290-293) -- and rebuilds it for any
 * other graph.  Call it again after changing edge_index's contents in place. */
int lspcg_gnn_set_graph(lspcg_gnn* g, int64_t N, int64_t E, const int64_t* edge_index);
/* x [N,node_in], edge_index device int64 [2,E], edge_attr [E,edge_in] -> out [E,edge_out]
 * (all fp32 device).  Message aggregation order is deterministic. */
int lspcg_gnn_forward(lspcg_gnn* g, int64_t N, int64_t E, const float* x, const int64_t* edge_index,
                      const float* edge_attr, float* out);
/* Which kernels lspcg_gnn_create chose: *f32 = 1 for the fp32-MFMA ones, 0 for the split-f16 GEMMs;
 * *hidden_bound (may be NULL) = the weights' hidden-activation bound that decided it (2^15). */
int lspcg_gnn_precision(const lspcg_gnn* g, int* f32, double* hidden_bound);
/* New weights for an existing handle (same layout and count as lspcg_gnn_create; host or device
 * pointer): re-emits the fragments and re-decides f32 / hidden_bound exactly as lspcg_gnn_create
 * does, and keeps the workspace and the analysed graph -- an optimizer step costs no re-analysis. */
int lspcg_gnn_set_weights(lspcg_gnn* g, const float* weights, int64_t nweights);
/* Gradient of every parameter for grad_out = d loss / d out [E,edge_out]: grad_weights receives
 * nweights floats in the layout of the weight blob (overwritten, not accumulated).  x, edge_index,
 * edge_attr as for lspcg_gnn_forward; all device pointers.  Uses the analysed graph (either path),
 * recomputes the forward in plain fp32 whatever kernels the inference forward runs, keeps its
 * per-layer states in the handle's workspace ((2L+1) N + (L+4) E rows of 64 B, grown on first use),
 * and sums in a fixed order without floating-point atomics: the same inputs give the same bits. */
int lspcg_gnn_backward(lspcg_gnn* g, int64_t N, int64_t E, const float* x, const int64_t* edge_index,
                       const float* edge_attr, const float* grad_out, float* grad_weights);
int lspcg_gnn_destroy(lspcg_gnn* g);

/* ---- block SpMV over an edge list (GraphSpmv / AATPE, basic_layers.py:112-142, 228-261) ----
 * edge_index: device int64 [2,E], any order, duplicates summed (PyG scatter-add semantics);
 * N nodes of bs (1 or 3) components.  Values [E,bs,bs], x / y / mask / diag [N*bs], all of
 * `dtype`, device pointers; mask and diag nullable. */
int lspcg_graph_create(lspcg_ctx* ctx, int64_t N, int64_t E, int bs, const int64_t* edge_index, lspcg_graph** out);
int lspcg_graph_destroy(lspcg_graph* g);
/* GraphSpmv(use_transpose).forward: y = A x (transpose = 0: block (ei[0], ei[1]) multiplies
 * x[ei[1]], summed at ei[0]) or y = Aᵀ x (transpose = 1), then y *= mask */
int lspcg_graph_spmv(lspcg_graph* g, const void* vals, int dtype, int transpose, const void* x, const void* mask,
                     void* y);
/* AATPE(epsilon).forward: t = (mask ⊙ Aᵀx) ⊙ diag ; y = mask ⊙ (A t) + (ε x) ⊙ diag
 * (t: caller-provided [N*bs] scratch that receives AᵀX, the reference's AT_x) */
int lspcg_graph_aatpe(lspcg_graph* g, const void* vals, int dtype, double epsilon, const void* x, const void* mask,
                      const void* diag, void* t, void* y);
/* ---- the training objective and its gradient on the same handle ----
 * Both calls below keep scratch in the handle (the ends of every edge in the caller's order; six
 * N*bs vectors and the reduction partials of spai_loss), allocated on first use and freed by
 * lspcg_graph_destroy: calls on ONE graph handle must run on one stream at a time.  No
 * floating-point atomics anywhere: the same inputs give the same bits.
 *
 * Gradient of one GraphSpmv with respect to its values (what torch autograd derives from PyG's
 * propagate in basic_layers.py:126-142, there an [E,b,b] message tensor scatter-added with
 * atomics): for y = mask ⊙ (A x) and gy = mask ⊙ (upstream gradient), already masked by the caller,
 *   transpose = 0: dvals_e = gy_I ⊗ x_J        transpose = 1 (y = mask ⊙ (Aᵀ x)): dvals_e = x_I ⊗ gy_J
 * with e = (I, J) = (edge_index[0][e], edge_index[1][e]); dvals [E,bs,bs] in the caller's edge
 * order, duplicated edges each receive their own gradient.  (The gradient with respect to x is
 * lspcg_graph_spmv with the opposite transpose flag applied to gy.) */
int lspcg_graph_spmv_grad_vals(lspcg_graph* g, int dtype, int transpose, const void* gy, const void* x, void* dvals);
/* The reference's training / validation step after the GNN (workspace.py:96-112 _shared_step,
 * scaled_workspace.py:98-104 with diag = inv_diag): d = AATPE(epsilon)(r, edge_index, L, mask[, diag]),
 * then the loss of loss.py on q = mask ⊙ (A d):
 *   kind 0  RelativeL2Loss_ANorm (loss.py:168-188, sqr_out = True, config/loss.yaml's default):
 *           (1/B) Σ_g ‖q_g − r_g‖² / (‖r_g‖² + loss_eps) over the graphs ptr[g] .. ptr[g+1] (nodes)
 *   kind 1  L2Loss_ANorm (loss.py:190-203): the mean of (q − r)² over all N*bs elements
 * and, when dLvals is not NULL, its gradient with respect to the values of L in the caller's edge
 * order (dLvals [E,bs,bs]; what loss.backward() leaves in boo_entry.grad):
 *   gq = 2 (q − r) w_g ; gy = m ⊙ (Aᵀ (m ⊙ gq)) ; gtm = m ⊙ (Lᵀ gy) [⊙ diag] ; dL_e = gy_I ⊗ t_J + r_I ⊗ gtm_J
 * Lvals / Avals [E,bs,bs], r / mask / diag [N*bs] of `dtype` (mask, diag nullable); ptr: host or
 * device int64 [B+1], non-decreasing from 0 to N (a device ptr is copied back, which synchronises;
 * boundaries equal to the previous call's are not uploaded again); loss_out: one device double.
 * The per-graph sums are accumulated in double for both dtypes over fixed chunks of 2048 scalar
 * rows split at graph boundaries, then per graph over the chunk partials: the order depends on
 * neither the grid nor the device.  N = 0 gives loss 0 and launches nothing that indexes; E = 0
 * with N > 0 is the chain with L = A = 0 (q = 0). */
int lspcg_graph_spai_loss(lspcg_graph* g, const void* Lvals, const void* Avals, int dtype, double epsilon,
                          const void* r, const void* mask, const void* diag, const int64_t* ptr, int64_t B, int kind,
                          double loss_eps, double* loss_out, void* dLvals);

/* ---- P1 operators of a tetrahedral mesh, assembled on the device into a live matrix ----
 * (the reference's pymathprim.geometry laplacian / lumped_mass as datagen/heat_tetmesh.py:17-56 and
 * datagen/heat.py use them, and the linear-elastic block stiffness of datagen/elast_twist.py)
 *
 * lspcg_fem_create is the analysis, once per connectivity, all on the device.  nodes [N,3] fp64 and
 * tets [T,4] int32, each a host or a device pointer (copied into the handle).
 *   Pattern: the sorted unique (row, col) of the 16 vertex pairs of every tet plus (i, i) of every
 *     vertex (an unused vertex owns a stored 0 diagonal): int32 indptr / indices, columns sorted, for
 *     the scalar operator (n = N) and for the 3x3 block operator (nb = N) alike.
 *   Gather map: per stored entry its contributions (tet, 4 a + b) in ascending tet order, within a
 *     tet in ascending 4 a + b (one stable radix sort of 64-bit keys gives pattern and map at once).
 *   Checks, one launch and one flag read back before anything else is built: a vertex index outside
 *     0..N-1, a tet that repeats a vertex, a tet whose determinant is zero or not finite ->
 *     LSPCG_ERR_FORMAT, the message names the first such tet, no handle is returned.  16 T + N, or
 *     9 x the entry count, at or above 2^31 -> LSPCG_ERR_ARG.  N = 0 or T = 0 is legal (T = 0: the
 *     diagonal entries only; N = 0: the empty matrix).
 * Arithmetic, the same for every call below: per tet the expressions of a cofactor P1 element in
 * double -- edge vectors a, b, c from vertex 0, det = (a0 (b×c)0 + a1 (b×c)1) + a2 (b×c)2,
 * g1..g3 = b×c, c×a, a×b divided by det, g0 = -((g1 + g2) + g3), vol = |det| / 6 (either
 * orientation) -- and every stored value is the left-to-right sum of its contributions in gather-map
 * order, the mass term of a diagonal entry added last, rounded once to the matrix dtype on the store.
 * No floating-point atomics: the bits depend on neither the grid nor earlier calls, and the result
 * is symmetric bit for bit (blocks: out[(i,j)][p][q] == out[(j,i)][q][p]).
 * The values are produced in scratch of the handle and handed to lspcg_mat_set_values with the
 * handle's pattern: `out` must be a matrix of that pattern (block size 1 for heat, 3 for elasticity,
 * fp32 or fp64), anything else returns LSPCG_ERR_FORMAT and nothing is written; a prepare_spmv copy
 * is refilled, a solver on `out` needs lspcg_solver_update_matrix, exactly as after set_values.
 * Calls on ONE fem handle must run on one stream at a time (the scratch is the handle's: the values
 * of one assembly and, from the first heat call on, 17 doubles per tet of element matrices). */
typedef struct lspcg_fem lspcg_fem;
int lspcg_fem_create(lspcg_ctx* ctx, int64_t N, int64_t T, const double* nodes, const int32_t* tets, lspcg_fem** out);
int lspcg_fem_destroy(lspcg_fem* f);
/* moved vertices on the same connectivity (host or device [N,3] fp64); the determinant check runs
 * again, and on LSPCG_ERR_FORMAT the old coordinates stay */
int lspcg_fem_set_nodes(lspcg_fem* f, const double* nodes);
int lspcg_fem_info(const lspcg_fem* f, int64_t* N, int64_t* T, int64_t* nnz);
/* copy the pattern out (host or device destinations, N+1 and nnz int32; NULL skips an array) */
int lspcg_fem_pattern(const lspcg_fem* f, int32_t* indptr, int32_t* indices);
/* m_i = Σ_{t ∋ i} vol_t / 4 in ascending tet order; m: device fp64 [N] */
int lspcg_fem_lumped_mass(lspcg_fem* f, double* m);
/* A = K(κ) + diag(ρ ⊙ m): K_ab = ((g_a0 g_b0 + g_a1 g_b1) + g_a2 g_b2) · w, w = vol (kappa NULL) or
 * vol · κ_t (kappa: device fp64 [T]); the diagonal's last term is ρ_i · m_i with ρ = density (device
 * fp64 [N]) or, density NULL, density_scalar for every vertex (0: the bare Laplacian). */
int lspcg_fem_heat(lspcg_fem* f, const double* kappa, const double* density, double density_scalar, lspcg_mat* out);
/* Block (a,b)[i][j] += (λ (g_a,i g_b,j) + μ (g_a,j g_b,i + δ_ij g_a·g_b)) · vol with, per tet,
 * λ = (E ν) / ((1 + ν)(1 − 2 ν)) and μ = E / (2 (1 + ν)) (young, poisson: device fp64 [T]);
 * mass_coef · m_i is added last on the three diagonal entries of block (i, i).  Row-major blocks. */
int lspcg_fem_elasticity(lspcg_fem* f, const double* young, const double* poisson, double mass_coef, lspcg_mat* out);

/* ---- gradient clipping + optimizer step over a flat fp32 blob (neural_cg/utils/optim.py
 * create_optimizer: torch.optim.SGD / Adam / AdamW; Lightning's gradient_clip_val =
 * torch.nn.utils.clip_grad_norm_, config/trainer.yaml) ----
 * One launch of one workgroup on the context's stream; no state is kept and nothing synchronises.
 * All pointers are DEVICE pointers.  With g = coef * (float(grad_scale) * grad) and
 * coef = min(1, clip_norm / (‖float(grad_scale) * grad‖ + 1e-6)) (1 when clip_norm <= 0), the update
 * is torch.optim's non-capturable single-tensor one (no amsgrad / maximize / nesterov / dampening):
 *   ADAMW  w *= 1 - lr wd ; m += (1-β1)(g - m) ; v = β2 v + (1-β2) g² ;
 *          w -= lr/(1-β1^step) · m / (sqrt(v)/sqrt(1-β2^step) + eps)
 *   ADAM   the same with g += wd w in place of the decoupled decay
 *   SGD    g += wd w ; momentum != 0: m = g (step 1) or momentum m + g, g = m ; w -= lr g
 * evaluated in double and rounded once per stored fp32 value.  m, v: n floats each, zero before
 * step 1; v may be NULL for SGD, m too for SGD without momentum.  stats (4 doubles, may be NULL)
 * receives ‖float(grad_scale) * grad‖ before clipping, coef, ‖w‖ before and ‖w‖ after the step.
 * The norms are fixed-shape sums in double without floating-point atomics: the same inputs give the
 * same bits, whatever the pointers' alignment.  Non-finite gradients propagate as in torch.  n = 0
 * touches no array and still writes stats.  Sized for parameter counts up to a few 10^5. */
#define LSPCG_OPT_SGD 0
#define LSPCG_OPT_ADAM 1
#define LSPCG_OPT_ADAMW 2
typedef struct {
  int kind; /* LSPCG_OPT_SGD / _ADAM / _ADAMW */
  double beta1, beta2, eps, weight_decay, momentum;
  double clip_norm;  /* <= 0: no clipping */
  double grad_scale; /* multiplies grad first (1 / accumulate_grad_batches) */
} lspcg_optim_desc;
int lspcg_optim_step(lspcg_ctx* ctx, const lspcg_optim_desc* desc, int64_t n, int64_t step, double lr, float* w,
                     const float* grad, float* m, float* v, double* stats);

/* ---- one system row-partitioned over ranks (NOT in the reference,
 * whose systems each fit one process -- it replaces no reference interface).  The host driver
 * (learningsparsepreconditioner4gpu_amd/dist_pcg.py) owns the halo all-to-alls, the all-gathers
 * of dot partials (torch.distributed: RCCL over xGMI) and scipy cg's scalar recurrence
 * (iterative.py:359-418, as restated at validate.py:163-201); these calls enqueue the rank-local
 * device phases on the context's stream.  A, L, LT: the rank's rows of the global matrices as
 * square n_ext x n_ext scalar CSR over its extended vector [n_own own rows | halo] (rows >= n_own
 * empty; L and LT may both be NULL for plain CG).  send_idx (host or device, n_send entries):
 * own-row indices packed for the other ranks, grouped by destination.  red: a device buffer of
 * 64 x 2 x 2 doubles receiving per-group compensated (sum, correction) pairs of the launch's dots
 * (zeroed by the call; the host sums every rank's groups). */
typedef struct lspcg_part lspcg_part;
int lspcg_part_create(lspcg_ctx* ctx, const lspcg_mat* A, const lspcg_mat* L, const lspcg_mat* LT, int64_t n_own,
                      const int32_t* send_idx, int64_t n_send, lspcg_part** out);
int lspcg_part_destroy(lspcg_part* p);
/* sendbuf[k] = v[send_idx[k]] */
int lspcg_part_pack(lspcg_part* p, const void* v, void* sendbuf);
/* red <- groups of a·a, b·b over the own rows */
int lspcg_part_norms(lspcg_part* p, const void* a, const void* b, double* red);
/* t[i] = (LT r)_i, i < n_own */
int lspcg_part_lt(lspcg_part* p, const void* r_ext, void* t_ext);
/* z = L t + eps r ; red <- groups of r·z, r·r */
int lspcg_part_l(lspcg_part* p, const void* t_ext, const void* r, double eps, void* z, double* red);
/* q = A p ; red <- groups of p·q */
int lspcg_part_a(lspcg_part* p, const void* p_ext, void* q, double* red);
/* p = z (first != 0) or p*beta + z */
int lspcg_part_update_p(lspcg_part* p, const void* z, void* p_ext, double beta, int first);
/* x += alpha p ; r -= alpha q */
int lspcg_part_update_xr(lspcg_part* p, double alpha, const void* p_ext, const void* q, void* x, void* r_ext);
/* Device-side scalar recurrence (no host round trip per iteration; dist_pcg.DistributedPCG):
 * the part's device state holds scipy cg's scalars (rtol, atol, ‖r‖², ρ, ρ_prev, π, α, β, the
 * iteration count and a done code: 1 converged, 2 max_iter, 3 non-finite, 4 ‖b‖ = 0).
 * state_init: reset it (hist: device buffer of max_iter + 2 doubles receiving ‖r_k‖, or NULL).
 * scalars: one single-thread launch summing the all-gathered [world][64][nd][2] group pairs
 * rank-major and applying phase 0 init (nd 2: ‖r_0‖², ‖b‖²), 1 after part_l (nd 2: ρ, ‖r_k‖²;
 * then the top-of-loop test and β), 2 the same for plain CG (no gathered data), 3 after part_a
 * (nd 1: π; α), 4 plain CG after part_norms of r (nd 2: ‖r_{k+1}‖²).  update_p_dev /
 * update_xr_dev: update_p / update_xr with β, α from the state, skipped once done (update_xr_dev
 * also advances the iteration).  status: the iteration count and done code (synchronises). */
int lspcg_part_state_init(lspcg_part* p, double rtol, int64_t max_iter, double* hist);
int lspcg_part_scalars(lspcg_part* p, const double* gathered, int world, int phase);
int lspcg_part_update_p_dev(lspcg_part* p, const void* z, void* p_ext);
int lspcg_part_update_xr_dev(lspcg_part* p, const void* p_ext, const void* q, void* x, void* r_ext);
int lspcg_part_status(lspcg_part* p, int64_t* iter, int* done);
/* The SpMV phases (lt / l / a) of this part store and reduce own rows [r0, n_own) only (default 0):
 * dist_pcg keeps one part for the interior rows (every column owned: computed while the halo
 * exchange is in flight) and one with r0 = the first boundary row (after it). */
int lspcg_part_set_rows(lspcg_part* p, int64_t r0);
/* lspcg_part_status plus the state's ‖r_k‖² and atol: the host sizes the next chunk of enqueued
 * iterations from the residual's decay (as lspcg_solver_solve does), so few iterations are enqueued
 * past convergence -- each would still run its halo exchanges and all-gathers. */
int lspcg_part_progress(lspcg_part* p, int64_t* iter, int* done, double* rr, double* atol);

#ifdef __cplusplus
}
#endif

#endif /* LSPCG_H_ */
