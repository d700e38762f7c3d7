/* libcgps -- C ABI of the MI355X (gfx950) block-tridiagonal cyclic-reduction library.
 *
 * The reference (cunningham-lab/cyclic-gps) has no FFI: its boundary for this
 * path is the Python module cyclic_gps/cyclic_reduction.py.  Each entry point
 * below is what a ctypes binding for one function of that module calls; the
 * function it replaces is cited as file:line (relative to the reference root).
 * The Python mirror of the module lives in cyclic-gps_amd/cyclic_gps/.
 *
 * Conventions
 *   - All data pointers are DEVICE pointers (hipMalloc / torch CUDA tensors),
 *     C-contiguous, batch-major: Rs[N][d][d], Os[N-1][d][d], vectors [N][d].
 *     O_i is the LOWER off-diagonal block J[i+1][i].
 *   - Alignment.  The kernels read and write blocks and vectors 16 bytes at a
 *     time, so every ARRAY OF BLOCKS OR VECTORS of the factorisation, solve,
 *     sampling, inverse, batch and sharding entry points (Rs, Os, x, y, xcrr,
 *     Dp, Fp, Gp, Dk .. On, Sd, So, w, mean, O_left, records, record_out) and
 *     every array of d x d blocks of the LEG assembly and prediction entry
 *     points (Rs, Os, K_Rs, gRs, gOs, term, ip_cov_diag, ip_cov_offdiag,
 *     out_cov) starts on a 16-byte boundary.  Every workspace starts on a
 *     256-byte boundary (hipMalloc and torch give that).  An array or a
 *     workspace off its boundary is CGPS_ERR_ARG, with the argument's name in
 *     cgps_last_error(), before anything is launched.  Every other pointer
 *     (time stamps, G, scalars, offsets, out2, info, patterns, weights ...)
 *     must be aligned to its element size, as C asks of any pointer; the entry
 *     points named above check that too, the element-wise LEG entry points
 *     (log-likelihood forms, perturbation, observations, leave-one-out, the
 *     filter and its adjoint, cgps_normal_fill) take it on trust.
 *     Packed arrays of odd-sized blocks keep rows off the boundary inside the
 *     array (row 1 of 3 x 3 doubles starts at byte 72): that is the kernels'
 *     business; the rule is about the pointer handed in.
 *   - The library never allocates, frees or synchronises: the caller passes a
 *     scratch buffer of cgps_workspace_bytes() bytes, a HIP stream (hipStream_t
 *     as void*; NULL = default stream), and every call is asynchronous.
 *   - dtype: CGPS_F32 / CGPS_F64.  1 <= d <= 8.
 *   - Return value: CGPS_OK, or an error code; cgps_last_error() gives a
 *     thread-local message.
 *   - Non-positive-definite blocks are reported through the device word
 *     `info` (like torch.linalg.cholesky_ex): 0 = fine, otherwise 1 + the
 *     smallest original block-row index whose pivot was not positive.  The
 *     library zeroes it at the start of the call.
 *   - Factor storage ("packed factor"): the reference's decomp = (ms, Ds, Fs, Gs)
 *     (cyclic_reduction.py:287-309) with the per-level tensors concatenated in
 *     level order: Dp[sum ceil(m_l/2)] = Dp[N], Fp[sum floor(m_l/2)],
 *     Gp[sum floor((m_l-1)/2)], m_0 = N, m_{l+1} = floor(m_l/2).  Allocate N
 *     blocks for each.  cgps_level_layout() returns the sizes and offsets.
 *     A vector in "CRR layout" (halfsolve output, cyclic_reduction.py:312-338)
 *     uses the Dp offsets: [N][d].
 */
#ifndef CGPS_H
#define CGPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGPS_VERSION 320

enum { CGPS_F32 = 0, CGPS_F64 = 1 };

enum {
  CGPS_OK = 0,
  CGPS_ERR_ARG = 1,        /* bad argument (null pointer, N < 1, workspace too small ...) */
  CGPS_ERR_HIP = 2,        /* HIP runtime error at launch */
  CGPS_ERR_UNSUPPORTED = 3 /* d or dtype outside the compiled range */
};

/* which operation a workspace is sized for */
enum {
  CGPS_OP_MAHAL_LOGDET = 0,
  CGPS_OP_DECOMPOSE = 1,
  CGPS_OP_HALFSOLVE = 2,
  CGPS_OP_BACKSOLVE = 3,
  CGPS_OP_SOLVE = 4,
  CGPS_OP_LOGDET_FACTOR = 5,
  CGPS_OP_INVERSE_BLOCKS = 6,
  CGPS_OP_MAHAL_LOGDET_LEVELWISE = 7,
  CGPS_OP_DECOMPOSE_SOLVE = 8
};

#define CGPS_MAX_LEVELS 64

int cgps_version(void);
const char* cgps_last_error(void);

/* Level sizes and packed-factor offsets for N block rows (host-side arithmetic only).
 * ms[l] = rows at level l (ms[nlevels-1] == 1); offD/offF/offG[l] = first block of
 * level l in Dp/Fp/Gp; arrays must hold CGPS_MAX_LEVELS entries (offsets: +1 for the total). */
int cgps_level_layout(int64_t N, int* nlevels, int64_t* ms, int64_t* offD, int64_t* offF, int64_t* offG);

int cgps_workspace_bytes(int64_t N, int d, int dtype, int op, size_t* bytes);

/* mahal_and_det(Rs, Os, x) -> (x^T J^-1 x, log|J|)        cyclic_reduction.py:380-438
 * out2[0] = mahal, out2[1] = logdet (device doubles, accumulated in fp64 for both dtypes).
 * When a block is not positive definite (info != 0) cgps_mahal_logdet and cgps_finish_records
 * write NaN to both, so a caller that never reads info cannot take a wrong number for a result. */
int cgps_mahal_logdet(const void* Rs, const void* Os, const void* x, int64_t N, int d, int dtype,
                      void* ws, size_t ws_bytes, double* out2, int* info, void* stream);
/* same result, one kernel launch per reduction level (simple form, kept as cross-check) */
int cgps_mahal_logdet_levelwise(const void* Rs, const void* Os, const void* x, int64_t N, int d, int dtype,
                                void* ws, size_t ws_bytes, double* out2, int* info, void* stream);

/* decompose_step(Rs, Os) -> (n, D, F, G), (R', O')           cyclic_reduction.py:203-259
 * Dk[ceil(n/2)], Fk[n/2], Gk[(n-1)/2], Rn[n/2], On[n/2-1]; n >= 2. */
int cgps_decompose_step(const void* Rs, const void* Os, int64_t n, int d, int dtype,
                        void* Dk, void* Fk, void* Gk, void* Rn, void* On, int* info, void* stream);

/* decompose(Rs, Os) -> packed factor                          cyclic_reduction.py:287-309 */
int cgps_decompose(const void* Rs, const void* Os, int64_t N, int d, int dtype,
                   void* Dp, void* Fp, void* Gp, void* ws, size_t ws_bytes, int* info, void* stream);

/* Right-hand sides: the reference's einsums carry a trailing "..." (cyclic_reduction.py:52-57,
 * 76-84), so halfsolve / backhalfsolve / solve take y[N][d] or Y[N][d][m].  nrhs = m (1 for a plain
 * vector); all vectors are [N][d][nrhs], C-contiguous.  For nrhs > 1 the factor is read once per
 * sweep and per panel of up to eight columns (csrc/cgps_solve_tile_m.h) instead of once per column;
 * size the workspace with cgps_solve_workspace_bytes(). */
int cgps_solve_workspace_bytes(int64_t N, int d, int dtype, int op, int nrhs, size_t* bytes);

/* halfsolve(decomp, y) -> L^-1 T y in CRR layout              cyclic_reduction.py:312-338
 * mahal_out (optional, device double) receives ||L^-1 T y||^2 = mahal(decomp, y), :461-467
 * (summed over all nrhs columns, like the reference's torch.sum). */
int cgps_halfsolve(const void* Dp, const void* Fp, const void* Gp, int64_t N, int d, int dtype, int nrhs,
                   const void* y, void* xcrr, void* ws, size_t ws_bytes, double* mahal_out, void* stream);

/* backhalfsolve(decomp, ycrr) -> T^T L^-T ycrr, natural order  cyclic_reduction.py:341-377 */
int cgps_backsolve(const void* Dp, const void* Fp, const void* Gp, int64_t N, int d, int dtype, int nrhs,
                   const void* ycrr, void* x, void* ws, size_t ws_bytes, void* stream);

/* solve(decomp, y) -> J^-1 y                                   cyclic_reduction.py:441-444 */
int cgps_solve(const void* Dp, const void* Fp, const void* Gp, int64_t N, int d, int dtype, int nrhs,
               const void* y, void* x, void* ws, size_t ws_bytes, void* stream);

/* decompose(Rs, Os) AND solve(decomp, y) in one call, for callers that factor and solve together
 * (compute_insample_posterior, models.py:288-292; the backward of mahal_and_det): the factor comes out as from
 * cgps_decompose, xcrr[N][d] = halfsolve(decomp, y) in CRR layout, x[N][d] = J^-1 y.  The forward substitution of
 * y rides along in the first pass of the factorisation, so the forward sweep proper starts three levels down and
 * never reads the factor blocks of those levels (7/8 of the factor): the factor is read once, not twice.
 * Workspace: cgps_workspace_bytes(N, d, dtype, CGPS_OP_DECOMPOSE_SOLVE). */
int cgps_decompose_solve(const void* Rs, const void* Os, const void* y, int64_t N, int d, int dtype,
                         void* Dp, void* Fp, void* Gp, void* xcrr, void* x, void* ws, size_t ws_bytes, int* info,
                         void* stream);

/* det(decomp) -> log|J| = 2 sum log diag(D)                    cyclic_reduction.py:447-458 */
int cgps_logdet_factor(const void* Dp, int64_t N, int d, int dtype,
                       void* ws, size_t ws_bytes, double* out, void* stream);

/* inverse_blocks(decomp) -> diag and lower off-diag blocks of J^-1   cyclic_reduction.py:470-503
 * Sd[N][d][d], So[N-1][d][d]. */
int cgps_inverse_blocks(const void* Dp, const void* Fp, const void* Gp, int64_t N, int d, int dtype,
                        void* Sd, void* So, void* ws, size_t ws_bytes, void* stream);

/* ---- sampling (an addition to the reference's surface: LEGFamily.sample_from_prior, models.py:243-252, is a stub) ----
 * Counter-based standard normals: out[rows][cols], element (r, s) a pure function of (seed, stream_id, r, s) --
 * Philox4x32-10 and Box-Muller, specified in csrc/cgps_rng.h.  Column s of row r does not depend on cols: the first
 * c columns of a wider array are bitwise those of a c-column array.  stream_id: a caller-chosen word that separates
 * independent arrays drawn under one seed. */
int cgps_normal_fill(void* out, int64_t rows, int64_t cols, int dtype, uint64_t seed, uint32_t stream_id, void* stream);

/* Samples from N(mean, J^-1) off a stored factor: x[:, :, s] = mean + H^T eps[:, :, s], H = L^-1 T (cgps_halfsolve),
 * H^T = cgps_backsolve, J^-1 = H^T H.  eps[N][d][nrhs] is BY DEFINITION what
 * cgps_normal_fill(rows = N d in CRR order, cols = nrhs, seed, stream_id) writes, but it is never in memory: the lane
 * that eliminates a block row makes its panel of eps in registers (csrc/cgps_sample_tile.h), and the last pass adds
 * mean[N][d] (NULL: zero) in its store to x[N][d][nrhs].  Sample s therefore depends on (seed, stream_id, s) alone,
 * not on nrhs.  Launches: one per pass of the sweep for up to 1024 samples (all eight-column chunks of a pass in one
 * launch), each further 1024 samples the same passes again on the same workspace.  1 <= d <= 8, any N, nrhs >= 1.
 * Workspace: cgps_sample_workspace_bytes(). */
int cgps_sample_workspace_bytes(int64_t N, int d, int dtype, int64_t nrhs, size_t* bytes);
int cgps_sample(const void* Dp, const void* Fp, const void* Gp, int64_t N, int d, int dtype, int64_t nrhs,
                const void* mean, uint64_t seed, uint32_t stream_id, void* x, void* ws, size_t ws_bytes, void* stream);

/* Adjoint of mahal_and_det in the blocks (what autograd computes through cyclic_reduction.py:380-438
 * for LEGFamily.training_step, models.py:374-381).  Given Sd/So = inverse_blocks(decomp),
 * w[N][d] = solve(decomp, x) and the two upstream gradients gm, gl (DEVICE scalars of the blocks'
 * dtype: d loss / d mahal, d loss / d logdet), overwrites in place
 *   Sd[i] <- gl Sd[i] - gm w_i w_i^T            (= d loss / d Rs[i])
 *   So[i] <- 2 (gl So[i] - gm w_i+1 w_i^T)      (= d loss / d Os[i])
 * d loss / d x = 2 gm w is the caller's.  No workspace. */
int cgps_mahal_logdet_adjoint(void* Sd, void* So, const void* w, int64_t N, int d, int dtype,
                              const void* gm, const void* gl, void* stream);

/* ---- many independent systems at once -------------------------------------------------------------
 * cgps_mahal_logdet for B block-tridiagonal systems in ONE launch, each with values of its own (one series under many
 * parameter sets, a mixture, blocks modified after the assembly: what a loop of mahal_and_det calls computes).
 * System b is rows offsets[b] .. offsets[b+1]-1 of the concatenated Rs[R][d][d] and x[R][d] (NULL: the
 * log-determinants alone, out2[b][0] = 0); offsets[B+1] is int64 DEVICE memory, non-decreasing, offsets[0] >= 0.
 * Its coupling blocks start at block offsets[b] - (os_packed ? b : 0) of Os:
 *   os_packed = 0: Os[R-1][d][d], the layout of the concatenated system; the entry between two systems is NEVER read,
 *                  whatever it holds;
 *   os_packed = 1: Os[B][n-1][d][d], the dense layout of B systems of n rows each.
 * out2[b] = {x_b^T J_b^-1 x_b, log|J_b|} (device doubles); info[b]: 0, or 1 + a row of the system (local index) near
 * a block that is not positive definite -- that system's two values are NaN then and every other system is
 * unaffected.  One workgroup per system, sums in a fixed order: a system's values do not depend on its place in the
 * batch.  A system with n_b < 1 or n_b > max_rows is skipped (nothing of its slot is written: the caller reduces a
 * long one with cgps_mahal_logdet).  No workspace.
 * CGPS_ERR_ARG: a null pointer (x excepted) or B < 0; CGPS_ERR_UNSUPPORTED: d outside 1..8, a bad dtype, and the
 * block sizes this kernel is not built for (d = 8, fp64 d = 6: reduce each system with cgps_mahal_logdet); B = 0
 * returns CGPS_OK and launches nothing. */
int cgps_mahal_logdet_batch(const void* Rs, const void* Os, const void* x, const int64_t* offsets, int64_t B,
                            int os_packed, int d, int dtype, int64_t max_rows, double* out2, int* info, void* stream);

/* cgps_mahal_logdet_adjoint for B systems with upstream gradients of their own.  Sd[N][d][d], So[N-1][d][d] and
 * w[N][d] are inverse_blocks / solve of the block-diagonal CONCATENATION of the systems (coupling blocks between
 * systems zero); seg[N] (DEVICE int32) names the system of each row, non-decreasing, values outside 0 .. B-1 are
 * clamped; gm[B], gl[B] (DEVICE arrays of the blocks' dtype): d loss / d mahal_b, d loss / d logdet_b.  In place:
 *   Sd[i] <- gl[s] Sd[i] - gm[s] w_i w_i^T,  s = seg[i]
 *   So[i] <- 2 (gl[s] So[i] - gm[s] w_i+1 w_i^T)  when rows i and i+1 belong to one system, 0 otherwise.
 * No workspace. */
int cgps_mahal_logdet_adjoint_seg(void* Sd, void* So, const void* w, const int* seg, int64_t N, int64_t B, int d,
                                  int dtype, const void* gm, const void* gl, void* stream);

/* ---- operand assembly for LEG models (the caller's step right before the path) ---------------
 * Blocks of the PEG prior precision from the time stamps and the generator G
 * (models.py:181-239: E_i = exp(-1/2 (t_{i+1}-t_i) G), two d x d solves per gap):
 * ts[N] (same dtype as the blocks), G[d][d]  ->  Rs[N][d][d], Os[N-1][d][d].
 * info: 0, or 1 + the index of a row next to a gap whose systems are not positive definite
 * (zero-length gap, NaN).  No workspace. */
int cgps_peg_precision(const void* ts, const void* G, int64_t N, int d, int dtype,
                       void* Rs, void* Os, int* info, void* stream);

/* cgps_mahal_logdet of a LEG system WITHOUT materialising its blocks (the assembly fused into the first pass of the
 * reduction; replaces cgps_peg_precision + cgps_mahal_logdet of models.py:349-367 when no factor is kept):
 *     J = PEG precision(ts, G) + blockdiag(A),   out2 = {v^T J^-1 v, log|J|}
 * ts[N], G[d][d], A[d][d] (added to EVERY diagonal block; NULL: nothing added -- the prior precision itself),
 * v[N][d] (NULL: zeros, out2[0] = 0).  Every lane assembles the block rows it eliminates in registers from the time
 * stamps: nothing but ts and v is read from HBM.  One launch at any N.  Workspace, out2 and info as for
 * cgps_mahal_logdet (cgps_workspace_bytes(N, d, dtype, CGPS_OP_MAHAL_LOGDET)); info also reports a singular gap
 * (zero length).  CGPS_ERR_UNSUPPORTED for d = 8 and fp64 d = 6 (their first pass shares a block row between lanes):
 * assemble with cgps_peg_precision and call cgps_mahal_logdet there. */
int cgps_leg_mahal_logdet(const void* ts, const void* G, const void* A, const void* v, int64_t N, int d, int dtype,
                          void* ws, size_t ws_bytes, double* out2, int* info, void* stream);

/* Both reductions of a LEG log-likelihood (models.py:349-367) in ONE launch, side by side:
 *   out4[0..1] = {v^T K^-1 v, log|K|},  K = PEG precision(ts, G) + blockdiag(A)      (posterior precision, info2[0])
 *   out4[2..3] = {0, log|PEG precision(ts, G)|}                                       (prior precision,     info2[1])
 * Workspace: twice cgps_workspace_bytes(N, d, dtype, CGPS_OP_MAHAL_LOGDET), each half rounded up to 256 bytes. */
int cgps_leg_mahal_logdet_pair(const void* ts, const void* G, const void* A, const void* v, int64_t N, int d, int dtype,
                               void* ws, size_t ws_bytes, double* out4, int* info2, void* stream);

/* cgps_leg_mahal_logdet_pair for a series whose rows do not all observe the same channels (or anything at all):
 * row i adds entry pattern[i] of a table of diagonal terms instead of the one A,
 *   K = PEG precision(ts, G) + blockdiag(A_table[pattern[i]]).
 * A_table[P][d][d], 1 <= P <= 256 (an all-zero entry for a row that observes nothing); pattern[N]: DEVICE bytes, a
 * byte >= P reads entry P - 1 (no byte value reads outside the table); v[N][d] (NULL: zeros) is the caller's
 * right-hand side, built with the same per-row pattern.  The prior-precision half (out4[2..3]) adds nothing and reads
 * no pattern.  out4, info2, workspace and error codes: those of cgps_leg_mahal_logdet_pair; null pointers and P
 * outside 1..256 are CGPS_ERR_ARG before anything is launched. */
int cgps_leg_mahal_logdet_pair_obs(const void* ts, const void* G, const void* A_table, int P,
                                   const unsigned char* pattern, const void* v, int64_t N, int d, int dtype,
                                   void* ws, size_t ws_bytes, double* out4, int* info2, void* stream);

/* cgps_leg_mahal_logdet_pair for a series whose rows each have a diagonal term of their own (per-observation noise
 * variances): row i adds a weighted sum of Kb basis blocks shared by all rows,
 *   K = PEG precision(ts, G) + blockdiag(sum_k weights[i][k] basis[k]).
 * basis[Kb][d][d], 1 <= Kb <= 64; weights[N][Kb] in the dtype of the call (DEVICE memory); v[N][d] (NULL: zeros) is
 * the caller's right-hand side.  The d x d terms are formed in registers and never written.  The prior-precision half
 * (out4[2..3]) adds nothing and reads neither basis nor weights.  out4, info2, workspace and error codes: those of
 * cgps_leg_mahal_logdet_pair; null pointers, N < 1 and Kb outside 1..64 are CGPS_ERR_ARG before anything is
 * launched. */
int cgps_leg_mahal_logdet_pair_w(const void* ts, const void* G, const void* basis, int Kb, const void* weights,
                                 const void* v, int64_t N, int d, int dtype, void* ws, size_t ws_bytes, double* out4,
                                 int* info2, void* stream);

/* Adjoint of cgps_peg_precision in G and in the time gaps (training through the assembly; what
 * autograd computes through models.py:181-239 for LEGFamily.training_step, models.py:374-381).
 * gRs[N][d][d], gOs[N-1][d][d]: d loss / d Rs, d loss / d Os.  One lane per time gap, 64 gaps per
 * workgroup; gG_partial[ceil((N-1)/64)][d][d] receives each workgroup's share of d loss / d G
 * (the caller adds them up: a few d x d blocks, deterministic order); gtau[N-1] (may be NULL)
 * receives d loss / d (t_{i+1} - t_i).  N >= 2.  No workspace. */
int cgps_peg_precision_adjoint(const void* ts, const void* G, int64_t N, int d, int dtype,
                               const void* gRs, const void* gOs, void* gG_partial, void* gtau, void* stream);

/* Many independent LEG series in ONE launch (the batch dimension of the reference's time_series_dataset,
 * data_utils.py:61-75, which LEGFamily.training_step squeezes away, models.py:374-381).  Series b is rows
 * offsets[b] .. offsets[b+1]-1 of the concatenated ts[sum n_b], v[sum n_b][d] (NULL: zeros) and q[sum n_b]
 * (NULL: zeros); offsets[B+1] is int64 DEVICE memory.  Per series, in fp64:
 *   out4[b][0..1] = {v_b^T K_b^-1 v_b, log|K_b|},  K_b = PEG precision(ts_b, G) + blockdiag(A)    (info2[2b])
 *   out4[b][2]    = log|PEG precision(ts_b, G)|                                                  (info2[2b+1])
 *   out4[b][3]    = sum of q over the series' rows (summed in a fixed order)
 * i.e. the two reductions of models.py:349-367 and the observation term for each series alone.  info: 0 or
 * 1 + a row of the series (local index) near a block that is not positive definite (a zero-length gap
 * included); that system's entries are NaN, every other series is unaffected.  The time stamps of different
 * series are independent (they may overlap or decrease from one series to the next).  One workgroup per
 * series and system; a series of more than max_rows rows is skipped (nothing written).  No workspace.
 * CGPS_ERR_UNSUPPORTED for d = 8 and fp64 d = 6, as cgps_leg_mahal_logdet. */
int cgps_leg_loglik_batch(const void* ts, const int64_t* offsets, int64_t B, const void* G, const void* A,
                          const void* v, const void* q, int d, int dtype, int64_t max_rows, double* out4,
                          int* info2, void* stream);

/* cgps_leg_loglik_batch for series whose rows do not all observe the same channels (or anything at all: padding,
 * held-out windows): row i of the CONCATENATED batch adds entry pattern[i] of a table of diagonal terms instead of
 * the one A,
 *   K_b = PEG precision(ts_b, G) + blockdiag(A_table[pattern[offsets[b] + r]]),  r = 0 .. n_b - 1.
 * A_table[P][d][d], 1 <= P <= 256 (an all-zero entry for a row that observes nothing); pattern[sum n_b]: DEVICE bytes,
 * a byte >= P reads entry P - 1 (no byte value reads outside the table); v and q are the caller's, built with the same
 * per-row pattern (q carries the rows' observation constants).  The prior-precision system (out4[b][2]) adds nothing,
 * reads neither table nor pattern, and its value is that of cgps_leg_loglik_batch bit for bit.  out4, info2, max_rows
 * and error codes: those of cgps_leg_loglik_batch; a null A_table or pattern with B > 0 and P outside 1..256 are
 * CGPS_ERR_ARG before anything is launched; B = 0 returns CGPS_OK.  No workspace. */
int cgps_leg_loglik_batch_obs(const void* ts, const int64_t* offsets, int64_t B, const void* G, const void* A_table,
                              int P, const unsigned char* pattern, const void* v, const void* q, int d, int dtype,
                              int64_t max_rows, double* out4, int* info2, void* stream);

/* cgps_leg_loglik_batch for series whose rows each have a diagonal term of their own (per-observation noise variances,
 * many series at once): row i of the CONCATENATED batch adds a weighted sum of Kb basis blocks shared by all rows,
 *   K_b = PEG precision(ts_b, G) + blockdiag(sum_k weights[offsets[b] + r][k] basis[k]),  r = 0 .. n_b - 1.
 * basis[Kb][d][d], 1 <= Kb <= 64; weights[sum n_b][Kb] in the dtype of the call (DEVICE memory); v and q are the
 * caller's, built with the same per-row terms (q carries the rows' observation constants).  The d x d terms are formed
 * in registers and never written.  The prior-precision system (out4[b][2]) adds nothing, reads neither basis nor
 * weights, and its value is that of cgps_leg_loglik_batch bit for bit.  out4, info2, max_rows and error codes: those of
 * cgps_leg_loglik_batch; a null basis or weights with B > 0 and Kb outside 1..64 are CGPS_ERR_ARG before anything is
 * launched; B = 0 returns CGPS_OK.  No workspace. */
int cgps_leg_loglik_batch_w(const void* ts, const int64_t* offsets, int64_t B, const void* G, const void* basis, int Kb,
                            const void* weights, const void* v, const void* q, int d, int dtype, int64_t max_rows,
                            double* out4, int* info2, void* stream);

/* cgps_peg_precision of several series concatenated (models.py:181-239 for each): cut[N-1] (device bytes),
 * cut[g] != 0 when rows g and g+1 belong to different series.  Such a gap is never evaluated, its coupling
 * block Os[g] is 0 and it adds nothing to Rs[g] or Rs[g+1]: the blocks of a block-diagonal system of
 * independent series.  Otherwise as cgps_peg_precision (which this leaves unchanged). */
int cgps_peg_precision_seg(const void* ts, const void* G, const unsigned char* cut, int64_t N, int d, int dtype,
                           void* Rs, void* Os, int* info, void* stream);

/* Adjoint of cgps_peg_precision_seg: as cgps_peg_precision_adjoint; a gap between two series contributes
 * nothing to gG_partial and gets gtau = 0. */
int cgps_peg_precision_adjoint_seg(const void* ts, const void* G, const unsigned char* cut, int64_t N, int d,
                                   int dtype, const void* gRs, const void* gOs, void* gG_partial, void* gtau,
                                   void* stream);

/* cgps_leg_loglik_batch for M models over the same batch of series, in ONE launch (several starts of a fit, a
 * population of chains, a grid of length scales, the components of a mixture).  ts[R], offsets[B+1] (int64 DEVICE
 * memory, offsets[B] = R) describe the batch once; model k brings G[k], A[k] of G[M][d][d], A[M][d][d] (A NULL: no
 * diagonal term), v[k] of v[M][R][d] (NULL: zeros) and q[k] of q[M][R] (NULL: zeros).  Grid (B, 2, M): the workgroup of
 * (series b, system, model k) does for (G[k], A[k], v[k], q[k]) what cgps_leg_loglik_batch does for its one model, and
 *   out4[k][b][0..3], info2[k][b][0..1]
 * are that call's out4[b], info2[b] bit for bit; every workgroup owns its slot (no records, counters or atomics on
 * floating-point values).  A series of more than max_rows rows is skipped for every model (nothing written).
 * M outside 1..65535, B < 0, R < 0 or a null ts, offsets, G, out4 or info2 with B > 0: CGPS_ERR_ARG before anything is
 * launched; B = 0 returns CGPS_OK; CGPS_ERR_UNSUPPORTED for d = 8 and fp64 d = 6.  No workspace. */
int cgps_leg_loglik_models(const void* ts, const int64_t* offsets, int64_t B, int64_t R, int64_t M, const void* G,
                           const void* A, const void* v, const void* q, int d, int dtype, int64_t max_rows,
                           double* out4, int* info2, void* stream);

/* cgps_leg_loglik_models for rows that do not all observe the same channels: cgps_leg_loglik_batch_obs for M models in
 * ONE launch, grid (B, 2, M).  The mask belongs to the data: pattern[R] (DEVICE bytes, a byte >= P reads entry P - 1)
 * describes the batch once and is read by every model; model k brings its own table, A_table[k] of A_table[M][P][d][d],
 * 1 <= P <= 256, next to G[k], v[k] and q[k] (v and q built by the caller with the same per-row pattern).
 *   out4[k][b][0..3], info2[k][b][0..1]
 * are what cgps_leg_loglik_batch_obs returns in out4[b], info2[b] for (G[k], A_table[k], pattern, v[k], q[k]), bit for
 * bit; the prior-precision system (out4[k][b][2]) reads neither table nor pattern.  Every workgroup owns its slot (no
 * records, counters or atomics on floating-point values); a series of more than max_rows rows is skipped for every
 * model.  M outside 1..65535, B < 0, R < 0, P outside 1..256 or a null ts, offsets, G, A_table, pattern, out4 or info2
 * with B > 0: CGPS_ERR_ARG before anything is launched; B = 0 returns CGPS_OK; CGPS_ERR_UNSUPPORTED for d = 8 and fp64
 * d = 6.  No workspace. */
int cgps_leg_loglik_models_obs(const void* ts, const int64_t* offsets, int64_t B, int64_t R, int64_t M, const void* G,
                               const void* A_table, int P, const unsigned char* pattern, const void* v, const void* q,
                               int d, int dtype, int64_t max_rows, double* out4, int* info2, void* stream);

/* cgps_leg_loglik_models for rows with a diagonal term of their own (per-observation noise variances):
 * cgps_leg_loglik_batch_w for M models in ONE launch, grid (B, 2, M).  The weights are the entries of each model's own
 * inverse noise covariance, so both operands are per model: basis[k] of basis[M][Kb][d][d], 1 <= Kb <= 64, and
 * weights[k] of weights[M][R][Kb] (DEVICE memory, the dtype of the call).
 *   out4[k][b][0..3], info2[k][b][0..1]
 * are what cgps_leg_loglik_batch_w returns in out4[b], info2[b] for (G[k], basis[k], weights[k], v[k], q[k]), bit for
 * bit; the prior-precision system reads neither basis nor weights.  Slots, max_rows, error codes: those of
 * cgps_leg_loglik_models_obs with Kb outside 1..64 and a null basis or weights in the place of P, A_table and
 * pattern.  No workspace. */
int cgps_leg_loglik_models_w(const void* ts, const int64_t* offsets, int64_t B, int64_t R, int64_t M, const void* G,
                             const void* basis, int Kb, const void* weights, const void* v, const void* q, int d,
                             int dtype, int64_t max_rows, double* out4, int* info2, void* stream);

/* cgps_peg_precision_seg of the same R rows under M generators G[M][d][d]: the blocks of the block-diagonal system
 * "model 0's batch, then model 1's batch, ...", Rs[M R][d][d] and Os[M R - 1][d][d].  ts[R] and cut[R-1] (NULL: one
 * series) are read by every model and not tiled in memory; rows k R .. (k+1) R - 1 use G[k] and equal what
 * cgps_peg_precision_seg writes for (ts, G[k], cut) bit for bit.  The coupling block between two models, Os[k R - 1],
 * is written as zeros and nothing is evaluated for it.  info: 0 or 1 + a row of the concatenated system next to a
 * singular gap.  M outside 1..65535, R < 1 or a null pointer: CGPS_ERR_ARG before anything is launched;
 * CGPS_ERR_UNSUPPORTED for d = 8 and fp64 d = 6 (the block sizes cgps_leg_loglik_models is not built for). */
int cgps_peg_precision_models(const void* ts, const void* G, const unsigned char* cut, int64_t R, int64_t M, int d,
                              int dtype, void* Rs, void* Os, int* info, void* stream);

/* Adjoint of cgps_peg_precision_models.  gRs[M R][d][d], gOs[M R - 1][d][d] (the entries k R - 1 between two models
 * are never read).  No workgroup straddles two models: gG_partial[M][ceil((R-1)/64)][d][d] holds model k's shares
 * (the caller adds them per model), gtau[M][R-1] (may be NULL) model k's d loss / d (t_{i+1} - t_i); a cut gap gets
 * gtau = 0 and adds nothing.  Slice k equals cgps_peg_precision_adjoint_seg on that model's slices bit for bit.
 * R >= 2, as cgps_peg_precision_adjoint_seg wants N >= 2; errors as cgps_peg_precision_models. */
int cgps_peg_precision_adjoint_models(const void* ts, const void* G, const unsigned char* cut, int64_t R, int64_t M,
                                      int d, int dtype, const void* gRs, const void* gOs, void* gG_partial,
                                      void* gtau, void* stream);

/* Blocks of the POSTERIOR precision of several series concatenated, written once: what cgps_peg_precision_seg writes,
 * with every row's observation term added to its diagonal block as the last operation before the store,
 *   K_Rs[i] = Rs[i] + term_i,   Os and info exactly those of cgps_peg_precision_seg.
 * source = CGPS_ROWS_PLAIN:    term_i = term[d][d] for every row (entries and rows are not read);
 *          CGPS_ROWS_TABLE:    term_i = term[min(rows[i], entries - 1)], term[entries][d][d], 1 <= entries <= 256,
 *                              rows = pattern[N] DEVICE bytes (no byte value reads outside the table);
 *          CGPS_ROWS_WEIGHTED: term_i = sum_k w[i][k] term[k], term = basis[entries][d][d], 1 <= entries <= 64,
 *                              rows = w[N][entries] in the dtype of the call (DEVICE memory); the sum over k is formed in
 *                              registers (fused multiply-adds from k = 0 up) and added to the block once.
 * Plain and table results are Rs + term_i with one rounded addition per element.  cut may be NULL: one series.
 * A null pointer, N < 1, an unknown source or entries outside its range: CGPS_ERR_ARG before anything is launched;
 * d outside 1..8 or an unknown dtype: CGPS_ERR_UNSUPPORTED. */
enum { CGPS_ROWS_PLAIN = 0, CGPS_ROWS_TABLE = 1, CGPS_ROWS_WEIGHTED = 2 };
int cgps_leg_posterior_blocks_seg(const void* ts, const void* G, const unsigned char* cut, int64_t N, int d, int dtype,
                                  int source, const void* term, int entries, const void* rows, void* K_Rs, void* Os,
                                  int* info, void* stream);

/* cgps_leg_posterior_blocks_seg of the same R rows under M models: the blocks of the block-diagonal POSTERIOR system
 * "model 0's batch, then model 1's batch, ...", K_Rs[M R][d][d] and Os[M R - 1][d][d], written once in ONE launch
 * (grid (ceil(R / 64), M)).  It is to cgps_leg_posterior_blocks_seg what cgps_peg_precision_models is to
 * cgps_peg_precision_seg.  ts[R], cut[R-1] (NULL: one series) and, for the table source, the pattern bytes rows[R]
 * belong to the data: they are read by every model and not tiled in memory.  Model k uses G[k] of G[M][d][d] and
 * source = CGPS_ROWS_PLAIN:    term[k] of term[M][d][d];
 *          CGPS_ROWS_TABLE:    term[k] of term[M][entries][d][d], 1 <= entries <= 256, rows = pattern[R] shared;
 *          CGPS_ROWS_WEIGHTED: term[k] of basis[M][entries][d][d], 1 <= entries <= 64, and rows[k] of w[M][R][entries]
 *                              (the weights are the entries of each model's own inverse noise covariance).
 * Rows k R .. (k+1) R - 1 of K_Rs and the same R - 1 entries of Os equal what cgps_leg_posterior_blocks_seg writes for
 * (ts, G[k], cut, source, term[k], rows or rows[k]) bit for bit.  The coupling block between two models, Os[k R - 1], is
 * written as zeros and nothing is evaluated for it.  info: 0 or 1 + a row of the concatenated system next to a singular
 * gap.  Built for every d in 1..8 in both precisions, as cgps_leg_posterior_blocks_seg is (not the restricted set of
 * cgps_peg_precision_models).  A null pointer, R < 1, M outside 1..65535, an unknown source or entries outside its
 * range: CGPS_ERR_ARG before anything is launched; d outside 1..8 or an unknown dtype: CGPS_ERR_UNSUPPORTED. */
int cgps_leg_posterior_blocks_models(const void* ts, const void* G, const unsigned char* cut, int64_t R, int64_t M, int d,
                                     int dtype, int source, const void* term, int entries, const void* rows, void* K_Rs,
                                     void* Os, int* info, void* stream);

/* Prediction glue of LEG models, the step AFTER the path (reference models.py:455-514 intercast with
 * forecast :394-408, interpolate :410-452 and gaussian_stitch model_utils.py:64-107, which the reference
 * runs as a Python loop over the targets): posterior mean and covariance of the latent at p target
 * times from the in-sample posterior.  ts[n] sorted; target_ts[p]; G[d][d]; ip_mean[n][d];
 * ip_cov_diag[n][d][d]; ip_cov_offdiag[n-1][d][d] = Cov(z_{i+1}, z_i) (what cgps_inverse_blocks leaves
 * in So)  ->  out_mean[p][d], out_cov[p][d][d].  One lane per target; no workspace, no info word (the
 * systems solved are positive definite whenever ts is strictly increasing). */
int cgps_leg_intercast(const void* ts, int64_t n, const void* target_ts, int64_t p, const void* G, int d, int dtype,
                       const void* ip_mean, const void* ip_cov_diag, const void* ip_cov_offdiag,
                       void* out_mean, void* out_cov, void* stream);

/* cgps_leg_intercast for B series concatenated, all targets of all series in one launch.  ts, ip_mean[R][d],
 * ip_cov_diag[R][d][d] and ip_cov_offdiag[R-1][d][d] are those of the concatenated batch (what cgps_inverse_blocks
 * leaves for the block-diagonal system cgps_peg_precision_seg assembles); series b is rows row_offsets[b] ..
 * row_offsets[b+1]-1 and its targets are target_ts[target_offsets[b] .. target_offsets[b+1]-1] (a series may have
 * none).  Both offset arrays are int64 DEVICE memory of B + 1 entries; P = target_offsets[B] is the total number of
 * targets and sizes the grid.  One lane per target: it finds its series by binary search in target_offsets and then
 * does what cgps_leg_intercast does for that series alone (same branches, same arithmetic, bit for bit); it never reads
 * a row of another series nor the off-diagonal block of a cut gap, whatever they hold.  out_mean[P][d],
 * out_cov[P][d][d].  B < 0, P < 0 or a null pointer with B > 0 and P > 0: CGPS_ERR_ARG; B = 0 or P = 0: CGPS_OK,
 * nothing launched; d outside 1..8 or an unknown dtype: CGPS_ERR_UNSUPPORTED.  No workspace, no info word. */
int cgps_leg_intercast_seg(const void* ts, const int64_t* row_offsets, const void* target_ts,
                           const int64_t* target_offsets, int64_t B, int64_t P, const void* G, int d, int dtype,
                           const void* ip_mean, const void* ip_cov_diag, const void* ip_cov_offdiag,
                           void* out_mean, void* out_cov, void* stream);

/* cgps_leg_intercast_seg under M models, all targets of all series of all models in ONE launch, grid
 * (ceil(P / 64), M).  ts[R], row_offsets[B+1], target_ts[P] and target_offsets[B+1] describe the batch and its targets
 * once and are shared by the models (R = row_offsets[B]); model k brings G[k] of G[M][d][d] and its slices of the
 * posterior of the concatenated system "model 0's batch, then model 1's batch, ...": rows k R .. (k+1) R - 1 of
 * ip_mean[M R][d] and ip_cov_diag[M R][d][d], the R - 1 entries from k R of ip_cov_offdiag[M R - 1][d][d], and gets
 * out_mean[k] of out_mean[M][P][d], out_cov[k] of out_cov[M][P][d][d].  Slice k equals cgps_leg_intercast_seg on model
 * k's slices bit for bit; no lane reads a row of another model or series, nor the off-diagonal entry of a cut gap or of
 * the boundary between two models, whatever they hold.  Errors: those of cgps_leg_intercast_seg, and M outside 1..65535:
 * CGPS_ERR_ARG; B = 0 or P = 0: CGPS_OK, nothing launched.  No workspace, no info word. */
int cgps_leg_intercast_models(const void* ts, const int64_t* row_offsets, const void* target_ts,
                              const int64_t* target_offsets, int64_t B, int64_t P, int64_t M, const void* G, int d,
                              int dtype, const void* ip_mean, const void* ip_cov_diag, const void* ip_cov_offdiag,
                              void* out_mean, void* out_cov, void* stream);

/* Perturb and solve: the right-hand sides of draws from the posterior (or prior) of B concatenated LEG series.
 * K = J_prior + blockdiag(B^T Li_i B) (cgps_leg_posterior_blocks_seg; cgps_peg_precision_seg for the prior) is a sum of
 * local positive semi-definite pieces, so noise w ~ N(0, K) is a sum of local pieces, and  x = K^-1 (v + w)  is a draw
 * from N(K^-1 v, K^-1).  This call writes out[R][d][nrhs] = v + w; the caller solves (cgps_solve on K's factor).
 * Series b is rows row_offsets[b] .. row_offsets[b+1]-1 (local rows r = 0 .. n_b - 1) and has the caller's number
 * k_b = series_ids[b], 0 <= k_b < 2^24; n_b max(d, obs) < 2^40.  Both arrays are int64 DEVICE memory (B + 1 and B
 * entries); the caller checks the two ranges.  With E_r = exp(-1/2 (t_{r+1} - t_r) G), I - E_r E_r^T = L_r L_r^T
 * (evaluated as the assembly evaluates it, never across a series boundary) and u_r = L_r^-T eps_{r+1}:
 *     w_r = (r == 0 ? eps_0 : u_{r-1}) - (r + 1 < n_b ? E_r^T u_r : 0) + H_r eps'_r
 * eps_r[i], column s  = element (k_b 2^40 + r d + i, s) of cgps_normal_fill's generator, key seed, stream word stream_id;
 * eps'_r[c], column s = element (k_b 2^40 + r obs + c, s), stream word stream_id + 1.
 * H_r [d][obs] with H_r H_r^T = B^T Li_r B comes from
 *   hsource = CGPS_H_NONE:  nothing (the prior; hterm, entries, obs and rows are not read);
 *             CGPS_H_PLAIN: hterm[d][obs] for every row;
 *             CGPS_H_TABLE: hterm[min(rows[i], entries - 1)] of hterm[entries][d][obs], rows = pattern bytes [R],
 *                           1 <= entries <= 256;
 *             CGPS_H_ROWS:  hterm[i] of hterm[R][d][obs].
 * v[R][d] may be NULL (zero).  A row's values depend only on (seed, stream_id, k_b, r, the series' time stamps and
 * H_r, v_r, the column): not on the series' position, the rest of the batch, nrhs or the launch geometry, bit for bit.
 * info: 0, or 1 + a row of the concatenated batch next to a singular (zero-length) gap.  One lane per row; no
 * workspace.  Built for every d in 1..8 in both precisions, 1 <= obs <= 8.  B < 0, R < 0, nrhs < 1, a null pointer, an
 * unknown hsource, obs or entries outside their ranges: CGPS_ERR_ARG before anything is launched; B = 0 or R = 0:
 * CGPS_OK, nothing launched; d outside 1..8 or an unknown dtype: CGPS_ERR_UNSUPPORTED. */
enum { CGPS_H_NONE = 0, CGPS_H_PLAIN = 1, CGPS_H_TABLE = 2, CGPS_H_ROWS = 3 };
int cgps_leg_perturbation_seg(const void* ts, int64_t R, const void* G, int d, int dtype, const int64_t* row_offsets,
                              const int64_t* series_ids, int64_t B, int hsource, const void* hterm, int entries, int obs,
                              const unsigned char* rows, const void* v, int64_t nrhs, uint64_t seed, uint32_t stream_id,
                              void* out, int* info, void* stream);

/* cgps_leg_perturbation_seg for the same R rows under M models: the right-hand sides v + w of the block-diagonal system
 * "model 0's batch, then model 1's batch, ..." (cgps_leg_posterior_blocks_models' system), out[M R][d][nrhs], in ONE
 * launch with the model as a grid axis (grid (ceil(R / 64), column chunks, M)).  ts[R], row_offsets[B+1], series_ids[B]
 * and the pattern bytes rows[R] of the table source belong to the data and are shared.  Model k brings G[k] of
 * G[M][d][d], v[k] of v[M][R][d] (v may be NULL: zero, the prior), its factors hterm[k] of hterm[M][d][obs] (CGPS_H_PLAIN),
 * hterm[M][entries][d][obs] (CGPS_H_TABLE) or hterm[M][R][d][obs] (CGPS_H_ROWS; CGPS_H_NONE: nothing) and its own
 * stream word stream_ids[k]: int64 DEVICE memory [M], every value in 0 .. 2^32 - 4 (the caller checks the range; the
 * words stream_ids[k], + 1 and + 2 are the model's: cgps_leg_observations takes the third).  Rows k R .. (k+1) R - 1 of
 * out equal, bit for bit, what cgps_leg_perturbation_seg writes for (ts, G[k], ..., hterm[k], v[k], seed,
 * stream_ids[k]), whatever M, the other models, nrhs or the launch geometry are.  info: 0, or 1 + a row of the
 * concatenated system next to a singular gap.  B < 0, R < 0, M outside 1..65535, nrhs < 1, a null pointer, an unknown
 * hsource, obs or entries outside their ranges: CGPS_ERR_ARG before anything is launched; B = 0 or R = 0: CGPS_OK,
 * nothing launched; d outside 1..8 or an unknown dtype: CGPS_ERR_UNSUPPORTED.  Built for every d in 1..8, both
 * precisions, all four sources.  No workspace. */
int cgps_leg_perturbation_models(const void* ts, int64_t R, int64_t M, const void* G, int d, int dtype,
                                 const int64_t* row_offsets, const int64_t* series_ids, int64_t B, int hsource,
                                 const void* hterm, int entries, int obs, const unsigned char* rows, const void* v,
                                 int64_t nrhs, uint64_t seed, const int64_t* stream_ids, void* out, int* info,
                                 void* stream);

/* Replicated observations: data sets drawn from the observation model given latent paths, for B concatenated series
 * under M models in one launch, one lane per (row, model), grid (ceil(R / 64), column chunks, M):
 *     x[k][i][c][s] = sum_j Bmat[k][c][j] z[k][i][j][s] + sum_c' T[c][c'] eps''[c'][s],   T T^T = LLT[k] + diag(s_i)
 * (T lower, factored in registers by the row's lane), z[M R][d][nrhs], Bmat[M][obs][d], LLT[M][obs][obs],
 * x[M R][obs][nrhs].  s_i[c] = noise_var[i][c] where bit c of pattern[i] is set and 0 elsewhere; noise_var[R][obs] is
 * never read at an unobserved entry; pattern == NULL: every entry is observed; noise_var == NULL: all zeros.  The
 * pattern only selects variances: every row and channel gets a value, observed or not.  eps''[c'], column s, is element
 * (series_ids[b] 2^40 + r obs + c', s) of cgps_normal_fill's generator, key seed, stream word stream_ids[k] + 2 (the
 * two words below it are those of cgps_leg_perturbation_models' draw of the same model), r the row's index inside its
 * series b (row_offsets[B+1], series_ids[B], stream_ids[M]: int64 DEVICE memory, ranges as there).  A value depends
 * only on (seed, stream_ids[k], the series' id, r, the row's operands, the column): not on the series' place in the
 * batch, on M, nrhs or the launch geometry, bit for bit.  info: 0, or 1 + a row k R + i whose T has a pivot that is not
 * positive.  B < 0, R < 0, M outside 1..65535, nrhs < 1 or a null pointer: CGPS_ERR_ARG; B = 0 or R = 0: CGPS_OK,
 * nothing launched; d or obs outside 1..8 or an unknown dtype: CGPS_ERR_UNSUPPORTED.  No workspace. */
int cgps_leg_observations(const void* z, const uint8_t* pattern, const void* noise_var, const int64_t* row_offsets,
                          const int64_t* series_ids, int64_t B, int64_t R, int64_t M, const void* Bmat, const void* LLT,
                          int d, int obs, int dtype, int64_t nrhs, uint64_t seed, const int64_t* stream_ids, void* x,
                          int* info, void* stream);

/* Leave-one-out predictives of B concatenated LEG series under M models, from the posterior of the latent
 * (cgps_decompose_solve + cgps_inverse_blocks of cgps_leg_posterior_blocks_seg / _models' system): one lane per
 * (row, model), grid (ceil(R / 256), M), then one workgroup per (model, series) for the scores, in the same call.
 * xs[R][obs], pattern[R] (bit c set: channel c of the row is observed; NULL: everything is), noise_var[R][obs] (extra
 * variances s of the observed entries; NULL: none) and row_offsets[B+1] (int64 DEVICE memory, row_offsets[B] = R)
 * describe the data once and are shared by the models; xs and noise_var are never read at an unobserved entry.  Model k
 * brings Bmat[k] of Bmat[M][obs][d], LLT[k] of LLT[M][obs][obs] (Lambda Lambda^T + 1e-9 I) and rows k R .. (k+1) R - 1
 * of ip_mean[M R][d] and ip_cov_diag[M R][d][d].  With m = diag(pattern bits), W = m (LLT + diag(s)) m + (I - m),
 * Li = m W^-1 m, x~ = xs where observed and 0 elsewhere, and (mu, S) the row's posterior:
 *     g = Li m (x~ - Bmat mu),   P = Li - Li (Bmat S Bmat^T) Li
 * (the row's block of the precision of all observed entries, and of that precision times the data), and
 *   leave = 0 (entry), per observed (row, c): out_var = 1 / P[c][c], out_mean = x_c - g_c / P[c][c],
 *       out_logpdf = -1/2 g_c^2 / P[c][c] + 1/2 log P[c][c] - 1/2 log 2 pi;  out_mean, out_var, out_logpdf [M][R][obs];
 *   leave = 1 (row), o the row's k observed channels: out_var = cov = (P[o][o])^-1 scattered into [M][R][obs][obs],
 *       out_mean = x_o - cov g_o [M][R][obs], out_logpdf = -1/2 g_o^T cov g_o + 1/2 log|P[o][o]| - k/2 log 2 pi [M][R].
 * An unobserved entry gets mean = var = NaN (row mode: its row and column of cov) and logpdf 0; a row that observes
 * nothing has logpdf 0.  out_score[M][B] (double): the sum of series b's log densities under model k, added in a fixed
 * order that depends on the series' own rows only (no atomics): a score does not depend on the series' place in the
 * batch.  A pivot of W or of P[o][o], or a P[c][c], that is not positive and finite fails the row: its outputs are NaN
 * (its series' score too) and info holds 1 + the smallest failing k R + i, else 0.  Built for every d in 1..8 and
 * obs in 1..8 in both precisions.  B < 0, R < 0, M outside 1..65535, leave outside {0, 1} or a null pointer with work
 * to do: CGPS_ERR_ARG; d or obs outside 1..8 or an unknown dtype: CGPS_ERR_UNSUPPORTED; B = 0 or R = 0: CGPS_OK,
 * nothing launched.  No workspace. */
int cgps_leg_loo(const void* xs, const uint8_t* pattern, const void* noise_var, const int64_t* row_offsets, int64_t B,
                 int64_t R, int64_t M, const void* Bmat, const void* LLT, int d, int obs, int dtype, const void* ip_mean,
                 const void* ip_cov_diag, int leave, void* out_mean, void* out_var, void* out_logpdf, double* out_score,
                 int* info, void* stream);

/* One-step-ahead predictives and filtered states of B concatenated LEG series under M models: one lane per
 * (series, model) walks the series' rows, grid (ceil(B / 64), M); the work is serial in a series' rows.  A launch of one
 * lane per (row, model) first leaves exp(-1/2 gap G) of the gap before every row in the row's slot of z_cov, where the
 * walking lane reads it before it stores the row's z_cov over it.
 * ts[R], xs[R][obs], pattern[R], noise_var[R][obs] and row_offsets[B+1] describe the data as for cgps_leg_loo and are
 * shared by the models; model k brings G[k] of G[M][d][d], Bmat[k] of Bmat[M][obs][d] and LLT[k] of LLT[M][obs][obs]
 * (Lambda Lambda^T + 1e-9 I).  t0[B], m0[M][B][d], P0[M][B][d][d]: the state N(m0, P0) of every (model, series) at the
 * time t0[b] <= the series' first time stamp, from which the series continues; all three NULL: the prior N(0, I) at the
 * first row.  With E = exp(-1/2 gap G), (m^-, P^-) = (E m, I + E (P - I) E^T) the state carried to row i, o the row's k
 * observed channels, e = x_o - Bmat_o m^- and S = (Bmat P^- Bmat^T + LLT + diag(s))[o][o] = T T^T:
 *   pred_mean[M][R][obs] = Bmat m^-,  pred_cov[M][R][obs][obs] = Bmat P^- Bmat^T + LLT + diag(s on o)  (ALL channels),
 *   logpdf[M][R] = -1/2 |T^-1 e|^2 - sum log T_cc - k/2 log 2 pi  (0 for a row that observes nothing),
 *   z_mean[M][R][d], z_cov[M][R][d][d] = the state after the row:  m^- + K e,  P^- - K S K^T,  K = P^- Bmat_o^T S^-1,
 *   loglik[M][B] (double) = the sum of the series' logpdf in row order,  m_end[M][B][d], P_end[M][B][d][d] = the state
 *   after the series' last row (that of t0 for a series without rows).
 * A gap that is negative or not finite, a pivot of S that is not positive, or a result that is not finite fails the
 * row: it and all later rows of that series under that model are NaN, so are loglik, m_end and P_end of that (model,
 * series), and info holds 1 + the smallest failing k R + i, else 0; other series and models are untouched.  Built for
 * every d in 1..8 and obs in 1..8 in both precisions.  B < 0, R < 0, M outside 1..65535, some but not all of t0, m0,
 * P0, or a null pointer with work to do: CGPS_ERR_ARG; d or obs outside 1..8 or an unknown dtype:
 * CGPS_ERR_UNSUPPORTED; B = 0 or R = 0: CGPS_OK, nothing launched.  No workspace. */
int cgps_leg_filter(const void* ts, const void* xs, const uint8_t* pattern, const void* noise_var,
                    const int64_t* row_offsets, int64_t B, int64_t R, int64_t M, const void* G, const void* Bmat,
                    const void* LLT, int d, int obs, int dtype, const void* t0, const void* m0, const void* P0,
                    void* pred_mean, void* pred_cov, void* logpdf, void* z_mean, void* z_cov, double* loglik, void* m_end,
                    void* P_end, int* info, void* stream);

/* cgps_leg_filter in time-parallel form: the same arguments, results and failures, for series whose length, not
 * whose number, is the work.  Every series is cut into chunks of at most chunk_rows rows that never straddle a series:
 * chunk_offsets[n_chunks+1] are the chunks' row offsets (chunk c holds rows chunk_offsets[c] .. chunk_offsets[c+1]-1,
 * series after series), chunk_series[n_chunks] the series of every chunk and series_chunks[B+1] the first chunk of
 * every series; all three are device arrays.  One lane per (chunk, model) composes the rows of its chunk into one
 * element of the filter's recursion, a scan over the elements with groups of `fanout` (levels of a tree, one launch
 * per level up and down; an element that starts a series is selected, never multiplied into) gives every chunk the
 * state it starts from, and the kernels of cgps_leg_filter then run over the chunks as if they were series.  The first
 * chunk of every series is cgps_leg_filter's own arithmetic, bit for bit; later rows agree with it to rounding.
 * loglik is the sum of the chunks' sums, added in chunk order.  A failing row fails as in cgps_leg_filter: the rows
 * before it are finite, it and the later rows of its series under that model are NaN, info holds 1 + the smallest
 * failing k R + i.  (A row whose S is not positive definite may fail the series from the start of its chunk on.)
 * ws / ws_bytes: caller-owned device memory of at least cgps_leg_filter_scan_workspace_bytes(n_chunks, M, d, dtype,
 * fanout) bytes, 256-byte aligned; z_cov is used as scratch before it is written.  The argument errors of
 * cgps_leg_filter, and CGPS_ERR_ARG for chunk_rows < 1, fanout < 2, a chunk count that does not fit (fewer than B or
 * than ceil(R / chunk_rows), more than R), a null or too small workspace. */
int cgps_leg_filter_scan_workspace_bytes(int64_t n_chunks, int64_t M, int d, int dtype, int64_t fanout, size_t* bytes);
int cgps_leg_filter_scan(const void* ts, const void* xs, const uint8_t* pattern, const void* noise_var,
                         const int64_t* row_offsets, int64_t B, int64_t R, int64_t M, const void* G, const void* Bmat,
                         const void* LLT, int d, int obs, int dtype, const void* t0, const void* m0, const void* P0,
                         const int64_t* chunk_offsets, const int64_t* chunk_series, const int64_t* series_chunks,
                         int64_t n_chunks, int64_t chunk_rows, int64_t fanout, void* ws, size_t ws_bytes,
                         void* pred_mean, void* pred_cov, void* logpdf, void* z_mean, void* z_cov, double* loglik,
                         void* m_end, void* P_end, int* info, void* stream);

/* Gradients through cgps_leg_filter: the reverse walk of its recursion.  The data arguments, G, Bmat, LLT, d, obs and
 * dtype are the forward's.  gap[R] replaces ts and t0: the time from the previous row of the series to row i, from the
 * start state to a series' first row, and 0 at a first row without a start state.  z_mean[M][R][d], z_cov[M][R][d][d]:
 * what the forward (serial or time-parallel) stored; m0[M][B][d], P0[M][B][d][d]: the start states, or both NULL.
 * The cotangents of the forward's per-row results, each may be NULL (zero): g_mean[M][R][obs], g_cov[M][R][obs][obs]
 * (its symmetric part is used), g_logpdf[M][R], g_z_mean[M][R][d], g_z_cov[M][R][d][d] (symmetric part).  The caller
 * adds the cotangent of loglik to g_logpdf of the series' rows and those of m_end, P_end to g_z_mean, g_z_cov of its
 * last row.  Three launches: one lane per (row, model) evaluates exp(-1/2 gap G) into the workspace; one lane per
 * (series, model), grid (ceil(B / 64), M), walks the series' rows from last to first, recomputes every row from the
 * state saved before it and stores the adjoint of the exponential over it; one lane per (row, model) takes that
 * through the Frechet derivative of the exponential.  Results:
 *   g_xs[M][R][obs], g_noise_var[M][R][obs]   per model (the caller sums over the models); exactly 0 at unobserved
 *                                             entries, whatever xs and noise_var hold there,
 *   g_Bmat[M][B][obs][d], g_LLT[M][B][obs][obs], g_m0[M][B][d], g_P0[M][B][d][d]   per (model, series); g_LLT and g_P0
 *                                             are symmetric; the caller sums g_Bmat and g_LLT over the series,
 *   g_G_partial[M][ceil(R / 64)][d][d]        sums over the rows of one workgroup in a fixed order (the caller adds them),
 *   g_gap[M][R]                               the gradient in gap, which the caller scatters to ts and t0.
 * A (model, series) whose forward failed (NaN in its last z_mean, z_cov) gets NaN in its rows of g_xs, g_noise_var
 * and g_gap, in its g_Bmat, g_LLT, g_m0, g_P0 and so in its model's g_G_partial; other series are untouched.
 * The entry is also called over CHUNKS of the series as if they were series (the time-parallel backward):
 * row_offsets = the chunks' offsets, B = their number, m0 / P0 = the saved state of the row before every chunk, gap
 * unchanged; g_m0, g_P0 are then the adjoints of those saved states and the caller links the chunks of a series.
 * ws / ws_bytes: caller-owned device memory of at least cgps_leg_filter_adjoint_workspace_bytes(R, B, M, d, obs, dtype)
 * bytes.  CGPS_ERR_ARG, before anything is launched: a null required pointer, one of m0, P0 without the other, B < 0,
 * R < 0, M outside 1..65535, d or obs outside 1..8, a workspace that is too small; an unknown dtype:
 * CGPS_ERR_UNSUPPORTED; B = 0 or R = 0: CGPS_OK, nothing launched. */
int cgps_leg_filter_adjoint_workspace_bytes(int64_t R, int64_t B, int64_t M, int d, int obs, int dtype, size_t* bytes);
int cgps_leg_filter_adjoint(const void* xs, const uint8_t* pattern, const void* noise_var, const int64_t* row_offsets,
                            int64_t B, int64_t R, int64_t M, const void* G, const void* Bmat, const void* LLT, int d,
                            int obs, int dtype, const void* gap, const void* z_mean, const void* z_cov, const void* m0,
                            const void* P0, const void* g_mean, const void* g_cov, const void* g_logpdf,
                            const void* g_z_mean, const void* g_z_cov, void* ws, size_t ws_bytes, void* g_xs,
                            void* g_noise_var, void* g_Bmat, void* g_LLT, void* g_m0, void* g_P0, void* g_G_partial,
                            void* g_gap, void* stream);

/* ---- time-axis sharding (one shard per GPU / rank) -----------------------------------------
 * The reference has no distributed code; this is the multi-GPU form BASELINE.json asks for.
 * A shard is n_loc consecutive block rows: Rs[n_loc], Os[n_loc-1] (couplings INSIDE the shard),
 * x[n_loc], plus O_left = J[first row of the shard, last row of the previous shard] (NULL for the
 * first shard).  cgps_shard_reduce eliminates every row of the shard but its last one and leaves
 *   record_out  : cgps_record_elems() elements = that last row (R, y), its new coupling to the
 *                 previous shard's last row, and the additive update it owes that row;
 *   partial_out : 4 doubles {sum of squares, sum of log pivots, 1 + first failing LOCAL row or 0, 0}.
 * The caller gathers the P records and partials in shard order (ONE all-gather over RCCL; the
 * library itself never communicates) and every rank calls cgps_finish_records, which reduces
 * the P-row boundary system and writes out2 = {mahal, logdet} and info (1 + a failing row --
 * local to the shard that saw it -- or 0).  record_stride_bytes / partial_stride_bytes are the
 * distances between consecutive shards' records / partials (record stride: a multiple of 16 bytes,
 * records 16-byte aligned), so both can be read in place from
 * the receive buffer of an all-gather of [record | partial] messages (record_out and
 * partial_out of cgps_shard_reduce may point straight into the send buffer; partial_out must
 * be 8-byte aligned).  P <= 1024 (256 for fp32 d = 8 and fp64 d = 7; 64 for fp64 d = 6 and d = 8).  Built for every block size
 * 1 <= d <= 8 in both precisions.  A rank may send several records (its rows cut into consecutive sub-shards,
 * each reduced by its own cgps_shard_reduce with O_left = the coupling to the previous sub-shard's last row):
 * cgps_finish_records simply takes all of them in row order.
 * Workspace of cgps_shard_reduce: cgps_workspace_bytes(n_loc, d, dtype, CGPS_OP_MAHAL_LOGDET). */
int cgps_record_elems(int d, int dtype, int64_t* elems);
int cgps_shard_reduce(const void* Rs, const void* Os, const void* x, const void* O_left, int64_t n_loc, int d,
                      int dtype, void* ws, size_t ws_bytes, void* record_out, double* partial_out, void* stream);
int cgps_finish_records(const void* records, size_t record_stride_bytes, const double* partials,
                        size_t partial_stride_bytes, int64_t P, int64_t rows_per_shard, int64_t N_total, int d,
                        int dtype, double* out2, int* info, void* stream);

/* The small systems a sharded SOLVE needs from the gathered records (cyclic_gps/sharded.py), one launch each:
 * cgps_boundary_solve: x at every shard's last row, xsep[P][d] -- the P-row block-tridiagonal system of the shards' last
 *   rows (R_w = Rs_w + dRa_{w+1}, y_w = ys_w + dya_{w+1}, J[w+1, w] = Cs_{w+1}) solved by block Cholesky; P <= 64;
 *   info: 0 or 1 + the first row whose pivot block is not positive definite.
 * cgps_boundary_recursions: what the rest of the system leaves on rank's two ends, out = [Pa (d*d) | pa (d) | dR (d*d) | dy (d)]:
 *   (Pa, pa) = diagonal block and right-hand side of the PREVIOUS shard's last row once every row left of it has been
 *   eliminated (zeros for rank 0), (dR, dy) = what eliminating every row right of rank's last row adds to that row. */
int cgps_boundary_solve(const void* records, size_t record_stride_bytes, int64_t P, int d, int dtype, void* xsep,
                        int* info, void* stream);
int cgps_boundary_recursions(const void* records, size_t record_stride_bytes, int64_t P, int64_t rank, int d, int dtype,
                             void* out, int* info, void* stream);

/* The one-launch forms of cgps_mahal_logdet / cgps_shard_reduce hand records from workgroup to workgroup inside the
 * launch through arrival counters in the library's own device memory.  Every completed launch leaves them at zero;
 * a launch that did NOT complete (a GPU fault in another kernel of the process, a killed context that was revived)
 * can leave a count half-way.  cgps_reset_counters enqueues a memset of all of them on `stream` (current device).
 * Call it with no library call in flight on that device.  Never needed in normal operation. */
int cgps_reset_counters(void* stream);

/* Measurement hook (bench.py): the next cgps_mahal_logdet call on this host thread
 * records `start` right before and `stop` right after its dominant kernel (the one
 * that streams Rs/Os/x from HBM) on the call's stream, then the hook clears itself.
 * start/stop are hipEvent_t created with timing enabled; nothing synchronises. */
int cgps_profile_next_call(void* start_event, void* stop_event);

#ifdef __cplusplus
}
#endif
#endif /* CGPS_H */
