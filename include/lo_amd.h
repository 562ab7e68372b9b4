/* lo_amd.h -- C ABI of liblo_amd.so: MI355X (gfx950) kernels for linear_operator's
 * iterative solve / logdet hot path.
 *
 * The reference (cornellius-gp/linear_operator) is pure Python and has no FFI; the seams this
 * library sits behind are the reference's own plug-in points:
 *   - linear_operator.utils.linear_cg          (linear_operator/utils/linear_cg.py:98-109, looked up
 *                                                at call time in operators/_linear_operator.py:796)
 *   - LinearOperator._matmul                    (operators/_linear_operator.py:169-190)
 *   - AddedDiagLinearOperator._preconditioner   (operators/added_diag_linear_operator.py:95-142)
 *   - PivotedCholesky.forward                   (functions/_pivoted_cholesky.py:14-105)
 *   - lanczos_tridiag / lanczos_tridiag_to_diag (utils/lanczos.py:9-189), StochasticLQ.to_dense
 *                                                (utils/stochastic_lq.py:45-82)
 * Each entry point below cites the reference interface it replaces.  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - all tensors are DEVICE pointers, fp32 (`float`), row-major contiguous, in the reference's
 *     layouts: vectors [B, N, c] with the column index c innermost; matrices [B, rows, cols];
 *     permutations int64 [B, N].  B is the flattened batch (product of the reference's *batch dims).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are asynchronous
 *     unless stated; the library never allocates device memory: the caller provides workspaces
 *     whose sizes come from the matching *_workspace_bytes query (host side: torch.empty).
 *   - return value: 0 = ok, <0 = LO_ERR_* (bad arguments, launch failure).  Numerical conditions
 *     (NaN in a matvec, non-convergence) are reported through lo_cg_info, and are mapped by the
 *     host shim to the reference's RuntimeError / NumericalWarning (linear_cg.py:199-200,337-347).
 *   - pointers are borrowed for the duration of the call only (asynchronous calls: until the
 *     stream has drained); inputs are never written (reference: linear_cg.py:182-190 allocates).
 */
#ifndef LO_AMD_H
#define LO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LO_OK 0
#define LO_ERR_BADARG (-1)
#define LO_ERR_LAUNCH (-2)
#define LO_ERR_WORKSPACE (-3)
#define LO_ERR_UNSUPPORTED (-4)

/* operator kinds: the `_matmul`s that feed CG */
#define LO_OP_LOWRANK_DIAG 0 /* AddedDiag(Root/LowRankRoot(C), Diag(d)):  y = C (C^T v) + d o v       */
#define LO_OP_DENSE_DIAG 1   /* AddedDiag(Dense(K), Diag(d)):             y = K v + d o v             */
#define LO_OP_KRON_DIAG 2    /* AddedDiag(Kron(K1,K2), Diag(d)):          y = (K1 (x) K2) v + d o v   */
#define LO_OP_CALLBACK 3     /* opaque closure (the reference's matmul_closure argument)              */
#define LO_OP_SUM 4          /* SumLinearOperator / PsdSum of up to LO_MAX_TERMS structured terms (+ one diagonal):
                              *   y = sum_i A_i v + d o v   (sum_linear_operator.py:47-51)              */
#define LO_MAX_TERMS 4
#define LO_OP_SKI_DIAG 5      /* AddedDiag(Interpolated(Toeplitz(t), W_l, W_r), Diag(d)):  y = W_l T W_r^T v + d o v
                               * (interpolated_linear_operator.py:192-219 over toeplitz_linear_operator.py:42-53)      */
#define LO_OP_TOEPLITZ_DIAG 6 /* AddedDiag(Toeplitz(t), Diag(d)):          y = T v + d o v   (T symmetric, N == M)  */
#define LO_TOEPLITZ_MAX_M 16384 /* grid sizes the native Toeplitz product takes (larger: LO_ERR_UNSUPPORTED)         */
#define LO_OP_HADAMARD_DIAG 7 /* AddedDiag(Mul(Root(F), Root(G)), Diag(d)):  y = (F F^T o G G^T) v + d o v
                               * (mul_linear_operator.py:54-80); A0 = F [B, N, p], R = p, A1 = G [B, N, q], n2 = q     */
#define LO_HADAMARD_MAX_RANK 128 /* p, q the native Hadamard kernels take (larger: LO_ERR_UNSUPPORTED); any column count */
#define LO_OP_MASKED 8 /* AddedDiag(Masked(base, mask, mask), Diag(d)):  y = S (base) S^T v + d o v, S the selected rows
                        * (masked_linear_operator.py:52-60); `mask` below, N = M, B = base->B                          */

/* diagonal storage */
#define LO_DIAG_NONE 0  /* no diagonal term (plain Root / Dense / Kron operator)                    */
#define LO_DIAG_FULL 1  /* DiagLinearOperator._diag [B, N]         (diag_linear_operator.py:25)      */
#define LO_DIAG_CONST 2 /* ConstantDiagLinearOperator.diag_values [B] (diag_linear_operator.py:313)  */

#define LO_OP_SKI_GRID_DIAG 9 /* AddedDiag(Interpolated(Kron(Toeplitz(t_1), .., Toeplitz(t_D)), W_l, W_r), Diag(d)), D = 2 or 3:
                               *   y = W_l (T_1 (x) .. (x) T_D) W_r^T v + d o v   (SKI on a 2-D / 3-D grid)             */
#define LO_SKI_GRID_MAX_AXIS 1024 /* grid points per axis the native grid product takes (larger: LO_ERR_UNSUPPORTED)    */
#define LO_KRON_EIG_MAX_SMALL 16  /* task-factor sizes n2 the fused kernel of lo_kron_eig_apply_f32 takes                */
#define LO_KRON_EIG_MAX_COLS 256  /* right-hand-side columns it takes (more: LO_ERR_UNSUPPORTED, the caller composes)    */
#define LO_SKI_GRID_MAX_M 4194304 /* grid points in all, 2^22 (larger: LO_ERR_UNSUPPORTED)                              */

#define LO_OP_TOEPLITZ_KRON_DIAG 10 /* AddedDiag(Kron(Toeplitz(t_1), .., Toeplitz(t_D)), Diag(d)), D = 2 or 3:
                                    *   y = (T_1 (x) .. (x) T_D) v + d o v   (a GP on a regular 2-D / 3-D grid)         */

#define LO_OP_KERNEL_DIAG 11 /* AddedDiag(Kernel(X, X, family, lengthscale, outputscale), Diag(d)):  y = K(X, X) v + d o v with
                              *   K_ij = outputscale^2 g(|(x_i - x_j) / lengthscale|) formed tile by tile from X, never stored
                              * (kernel_linear_operator.py:379-383 evaluates covar_func densely)                           */
#define LO_KERNEL_MAX_DIM 32 /* input dimensions D the on-the-fly kernels take (larger: LO_ERR_UNSUPPORTED)                 */
#define LO_KERNEL_RBF 0      /* g(r) = exp(-r^2 / 2)                                    */
#define LO_KERNEL_MATERN12 1 /* g(r) = exp(-r)                                          */
#define LO_KERNEL_MATERN32 2 /* g(r) = (1 + sqrt(3) r) exp(-sqrt(3) r)                  */
#define LO_KERNEL_MATERN52 3 /* g(r) = (1 + sqrt(5) r + 5 r^2 / 3) exp(-sqrt(5) r)      */
#define LO_OP_KERNEL_SUM_DIAG 12 /* AddedDiag(Kernel_1(X, X) + .. + Kernel_T(X, X), Diag(d)) over ONE point tensor X:
                                  *   y = (sum_t K_t(X, X)) v + d o v, every K_t formed tile by tile in the same pass      */
#define LO_KERNEL_MAX_TERMS 4    /* kernel terms T one LO_OP_KERNEL_SUM_DIAG descriptor / lo_kernel_sum_* call fuses      */
#define LO_OP_KERNEL_KRON_DIAG 13 /* AddedDiag(Kron(Kernel(X, X), Bt), Diag(d)), the multitask (coregionalisation) covariance:
                                   *   y[(i,t)] = sum_j theta_D g(r_ij) sum_s Bt[t,s] v[(j,s)] + d o v, index i T + t (data
                                   * index slowest, kronecker_product_linear_operator.py:34-45); K never stored            */
#define LO_KERNEL_KRON_MAX_TASKS 8 /* tasks T (Bt is T x T) the kind and lo_kernel_kron_mv_f32 take (more: LO_ERR_UNSUPPORTED) */
#define LO_OP_KERNEL_GRAD_DIAG 14 /* AddedDiag(GradKernel(X, X), Diag(d)): the covariance of the values AND the D partial
                                   * derivatives of a GP at n points (a GP with derivative observations), D + 1 outputs per
                                   * input, index i (D + 1) + a (data index slowest, a = 0 the value, a = 1 .. D the
                                   * derivative in coordinate a - 1); the n (D + 1) x n (D + 1) matrix is never stored    */
#define LO_KERNEL_GRAD_MAX_DIM 16 /* input dimensions D the kind and lo_kernel_grad_* take (more: LO_ERR_UNSUPPORTED)      */
#define LO_OP_KERNEL_TASK_DIAG 15 /* AddedDiag(TaskKernel(X, X), Diag(d)), the task-indexed ("Hadamard") multitask covariance:
                                   * every observation carries its own task id t_i in the LAST column of X [B, N, D + 1]:
                                   *   y[i] = sum_j theta_D g(r_ij) Bt[t_i, t_j] v[j] + d o v, r over columns 0 .. D - 1;
                                   * tasks need not be observed at the same points; K never stored                        */
#define LO_KERNEL_TASK_MAX_TASKS 8 /* tasks T (Bt is T x T) the kind and lo_kernel_task_* take (more: LO_ERR_UNSUPPORTED)   */
#define LO_OP_SKI_SUM_DIAG 16   /* AddedDiag(SumBatch(Interpolated(Toeplitz(t_p), W_l,p, W_r,p)), Diag(d)):
                                 *   y = sum_{p < P} W_l,p T_p W_r,p^T v + d o v,  P 1-D grids of M points over the same N rows */
#define LO_OP_KERNEL_LMC_DIAG 17 /* AddedDiag(Kron(Kernel_0(X, X), B_0) + .. + Kron(Kernel_{Q-1}(X, X), B_{Q-1}), Diag(d)), the linear
                                  * model of coregionalisation over ONE point tensor, index i T + t (data index slowest):
                                  *   y[(i,t)] = sum_q theta_q[D] sum_j g_{f_q}(r_q,ij) sum_s B_q[t,s] v[(j,s)] + d o v,
                                  *   r_q,ij^2 = sum_k (theta_q[k] (x_i[k] - x_j[k]))^2; no K_q and no product is ever stored;
                                  * Q in 1 .. LO_KERNEL_MAX_TERMS, T in 1 .. LO_KERNEL_KRON_MAX_TASKS, D <= LO_KERNEL_MAX_DIM */
#define LO_OP_KERNEL_PARAM_DIAG 18 /* AddedDiag(ParamKernel(X, X), Diag(d)): the matrix-free families with a shape parameter,
                                    *   y = K(X, X) v + d o v, K_ij = theta[D] g(x_i, x_j) formed tile by tile, never stored   */
#define LO_KERNEL_RQ 16       /* g = (1 + r^2 / (2 alpha))^(-alpha), r as for LO_KERNEL_RBF                                */
#define LO_KERNEL_PERIODIC 17 /* g = exp(-2 sum_k (sin(pi (x_i[k] - x_j[k]) / p_k) / l_k)^2)                               */
#define LO_KERNEL_PARAM_MAX_DIM 32 /* input dimensions D the kind and lo_kernel_param_* take (more: LO_ERR_UNSUPPORTED)     */
#define LO_OP_KERNEL_SM_DIAG 19 /* AddedDiag(SM(X, X), Diag(d)): the matrix-free spectral mixture kernel, y = K(X, X) v + d o v,
                                 *   K_ij = sum_q w_q exp(-2 pi^2 sum_k (sigma_qk tau_k)^2) prod_k cos(2 pi mu_qk tau_k),
                                 *   tau = x_i - x_j, formed tile by tile, never stored                                       */
#define LO_KERNEL_SM_MAX_DIM 16 /* input dimensions D the kind and lo_kernel_sm_* take (more: LO_ERR_UNSUPPORTED)            */
#define LO_KERNEL_SM_MAX_MIX 16 /* mixtures Q the kind and lo_kernel_sm_* take (more: LO_ERR_UNSUPPORTED)                    */
#define LO_SKI_SUM_MAX_TERMS 64 /* terms P one LO_OP_SKI_SUM_DIAG descriptor / lo_interp_sum_f32 call takes (more: LO_ERR_UNSUPPORTED) */

struct lo_interp_desc;
struct lo_mask_desc;
struct lo_grid_desc;

/* Operator descriptor ("op-tree lowering" of an AddedDiag/Sum tree). */
typedef struct lo_op_desc {
  int32_t kind;      /* LO_OP_*                                                                    */
  int32_t diag_mode; /* LO_DIAG_*                                                                  */
  int64_t B;         /* batch members                                                              */
  int64_t N;         /* matrix size (rows == cols)                                                 */
  int64_t R;         /* LOWRANK: root rank R (C is [B,N,R]);  KRON: n1;  DENSE: unused             */
  int64_t n2;        /* KRON: n2 (N == n1*n2); others unused                                       */
  const float* A0;   /* LOWRANK: C [B,N,R];  DENSE: K [B,N,N];  KRON: K1 [B,n1,n1]                 */
  const float* A1;   /* KRON: K2 [B,n2,n2]; others NULL                                            */
  const float* d;    /* diagonal, layout per diag_mode (NULL if LO_DIAG_NONE)                      */
  int32_t nterms;    /* SUM: number of terms (2 .. LO_MAX_TERMS); others 0                         */
  int32_t reserved;
  union {
    const struct lo_op_desc* terms; /* SUM: HOST array of nterms descriptors of kind LOWRANK / DENSE / KRON with
                      * diag_mode LO_DIAG_NONE and the same B, N (summed left to right, like the reference's
                      * Python sum()); the SUM's own (diag_mode, d) is the one diagonal of the tree */
    const struct lo_interp_desc* interp; /* SKI (ABI 16): HOST pointer to the two interpolation matrices      */
    const struct lo_mask_desc* mask;     /* MASKED (ABI 21): HOST pointer to the base descriptor and the index list */
    const struct lo_grid_desc* grid;     /* TOEPLITZ_KRON (ABI 24): HOST pointer to the grid shape                  */
    const float* task;                   /* KERNEL_KRON (ABI 29), KERNEL_TASK (ABI 34): DEVICE pointer to Bt [B, T, T], used
                                          * exactly as given; KERNEL_LMC (ABI 38): Bt [B, Q, T, T]                     */
  };
  /* ABI 16 kinds.  TOEPLITZ: A0 = first column t [B, M] of the symmetric Toeplitz matrix, R = M = N.
   * SKI: A0 = t [B, M], R = M (grid size), n2 = J (interpolation points per row), `interp` as below.
   * (The kinds reuse the existing fields: the size and layout of lo_op_desc are those of ABI 15.)
   * ABI 17 kind.  HADAMARD: A0 = F [B, N, p], R = p, A1 = G [B, N, q], n2 = q (same layout again).  Lowered for
   * lo_matvec_f32, the streaming CG, Lanczos, fp32 MINRES and the fp32 pivoted Cholesky; fp64 entry points return
   * LO_ERR_UNSUPPORTED; not a term kind of LO_OP_SUM.
   * ABI 21 kind.  MASKED: `mask` as below, N = mask->M, B = mask->base->B; its own (diag_mode, d) with d of length M is
   * the diagonal OUTSIDE the mask, the base's own diagonal the one inside (same layout again).  Lowered for
   * lo_matvec_f32, the streaming CG, Lanczos and fp32 MINRES; lo_pivoted_cholesky_f32 and the fp64 entry points return
   * LO_ERR_UNSUPPORTED; not a term kind of LO_OP_SUM.
   * ABI 23 kind.  SKI_GRID: A0 = the first columns of the D Toeplitz factors concatenated per member
   * [B, M_1 + .. + M_D], R = M = M_1 * .. * M_D (grid points, grid index g = (g_1 M_2 + g_2) M_3 + g_3), n2 = J,
   * `interp` as for SKI with the grid shape in its grid_ndim / grid_m (same layout again).  Lowered for lo_matvec_f32,
   * the streaming CG, Lanczos, fp32 MINRES and the fp32 pivoted Cholesky; the fp64 entry points, the resident / fused
   * engines and the solve sessions return LO_ERR_UNSUPPORTED; not a term kind of LO_OP_SUM, not a base kind of
   * LO_OP_MASKED.
   * ABI 24 kind.  TOEPLITZ_KRON: the base of SKI_GRID on its own.  A0 = the first columns of the D Toeplitz factors
   * concatenated per member [B, M_1 + .. + M_D], N = R = M_1 * .. * M_D (same grid index), `grid` as below (same layout
   * again); shape limits LO_SKI_GRID_MAX_AXIS / LO_SKI_GRID_MAX_M.  Lowered for lo_matvec_f32, the streaming CG,
   * Lanczos, fp32 MINRES and the fp32 pivoted Cholesky (diagonal prod_k t_k[0], row[j] = prod_k t_k[|i_k - j_k|]); the
   * fp64 entry points, the resident / fused engines and the solve sessions return LO_ERR_UNSUPPORTED; not a term kind of
   * LO_OP_SUM, not a base kind of LO_OP_MASKED.
   * ABI 26 kind.  KERNEL: A0 = X [B, N, D], R = D <= LO_KERNEL_MAX_DIM, A1 = theta [B, D + 1] = the D INVERSE lengthscales,
   * then outputscale^2 (a shared lengthscale is replicated by the host), n2 = the family code LO_KERNEL_* (same layout
   * again).  Lowered for lo_matvec_f32, the streaming CG, Lanczos, fp32 MINRES and the fp32 pivoted Cholesky (constant
   * diagonal theta[D], row[j] = theta[D] g(r_ij)); the fp64 entry points, the resident / fused engines and the solve
   * sessions return LO_ERR_UNSUPPORTED; a term kind of LO_OP_SUM from ABI 28 on; not a base kind of LO_OP_MASKED.
   * ABI 28 kind.  KERNEL_SUM: A0 = X [B, N, D], R = D <= LO_KERNEL_MAX_DIM, A1 = theta [B, T, D + 1] (per term the D inverse
   * lengthscales, then outputscale^2), nterms = T in 1 .. LO_KERNEL_MAX_TERMS (`terms` unused), n2 = the T family codes, four
   * bits per term, term 0 lowest (same layout again).  Lowered for lo_matvec_f32, the streaming CG, Lanczos, fp32 MINRES
   * and the fp32 pivoted Cholesky (diagonal sum_t theta[t][D], row[j] = sum_t theta[t][D] g_t(r_t,ij) in term order); the
   * fp64 entry points, the resident / fused engines and the solve sessions return LO_ERR_UNSUPPORTED; not a base kind of
   * LO_OP_MASKED.
   * ABI 28: KERNEL and KERNEL_SUM are term kinds of LO_OP_SUM next to LOWRANK / DENSE / KRON for lo_matvec_f32, the
   * streaming CG, Lanczos, fp32 MINRES and the fp32 pivoted Cholesky (operators over different point tensors, a kernel
   * plus a low-rank root); a sum that holds one is refused by the fp64 entry points and as the base of LO_OP_MASKED.
   * ABI 29 kind.  KERNEL_KRON: A0 = X [B, n, D], R = D <= LO_KERNEL_MAX_DIM, A1 = theta [B, D + 1] exactly as for KERNEL,
   * n2 = one family code LO_KERNEL_*, nterms = T in 1 .. LO_KERNEL_KRON_MAX_TASKS, N = n T, `task` = Bt [B, T, T] on the
   * DEVICE (same layout again: `task` is one more member of the union).  Bt is used as given, symmetric or not.  Lowered
   * for lo_matvec_f32, the streaming CG, Lanczos, fp32 MINRES and the fp32 pivoted Cholesky (diagonal theta[D] Bt[t,t],
   * row (p, tau): row[j T + s] = (theta[D] g(r_pj)) Bt[tau, s]); the fp64 entry points, the resident / fused engines and
   * the solve sessions return LO_ERR_UNSUPPORTED; not a term kind of LO_OP_SUM, not a base kind of LO_OP_MASKED.
   * LO_ERR_BADARG: a null A0 / A1 / task, R < 1, a family outside 0 .. 3, T < 1, N % T != 0.
   * ABI 30 kind.  KERNEL_GRAD: A0 = X [B, n, D], R = D <= LO_KERNEL_GRAD_MAX_DIM, A1 = theta [B, D + 1] exactly as for
   * KERNEL, n2 = the family code (LO_KERNEL_RBF only), N = n (D + 1), nterms = 0, no new member.  With t_k = theta[k],
   * u_k = t_k (x_i[k] - x_j[k]), e = exp(-|u|^2 / 2), the block of the pair (i, j) is (a, b = 1 .. D)
   *   K[0,0] = os2 e,  K[0,b] = os2 t_b u_b e,  K[a,0] = -os2 t_a u_a e,  K[a,b] = os2 t_a t_b (delta_ab - u_a u_b) e
   * Lowered for lo_matvec_f32, the streaming CG, Lanczos, fp32 MINRES and the fp32 pivoted Cholesky (diagonal os2 for
   * a = 0, os2 t_a^2 else); the fp64 entry points, the resident / fused engines and the solve sessions return
   * LO_ERR_UNSUPPORTED; not a term kind of LO_OP_SUM, not a base kind of LO_OP_MASKED.
   * LO_ERR_BADARG: a null A0 / A1, R < 1, N % (R + 1) != 0, a family outside 0 .. 3; LO_ERR_UNSUPPORTED: D > 16, a
   * family other than RBF.
   * ABI 34 kind.  KERNEL_TASK: A0 = X [B, N, D + 1], the D coordinates and then the task id of the observation (an integer
   * 0 .. T - 1 stored as a float), R = D (the coordinates: 1 <= D <= LO_KERNEL_MAX_DIM - 1), A1 = theta [B, D + 1] exactly
   * as for KERNEL, n2 = one family code LO_KERNEL_*, nterms = T in 1 .. LO_KERNEL_TASK_MAX_TASKS, `task` = Bt [B, T, T] on
   * the DEVICE (same layout again, no new member), used as given, symmetric or not:
   *   K_ij = theta[D] g(r_ij) Bt[t_i, t_j],  r_ij^2 = sum_{k < D} (theta[k] (x_i[k] - x_j[k]))^2
   * An id is rounded to the nearest integer and clamped into [0, T - 1] (NaN reads as 0): no id indexes outside Bt; ids
   * outside the range are the caller's error.  Lowered for lo_matvec_f32, the streaming CG, Lanczos, fp32 MINRES and the
   * fp32 pivoted Cholesky (diagonal theta[D] Bt[t_i, t_i], row of pivot p: row[j] = (theta[D] g(r_pj)) Bt[t_p, t_j]); the
   * fp64 entry points, the resident / fused engines and the solve sessions return LO_ERR_UNSUPPORTED; not a term kind of
   * LO_OP_SUM, not a base kind of LO_OP_MASKED.
   * LO_ERR_BADARG: a null A0 / A1 / task, R < 1, a family outside 0 .. 3, T < 1; LO_ERR_UNSUPPORTED: R + 1 >
   * LO_KERNEL_MAX_DIM, T > LO_KERNEL_TASK_MAX_TASKS.
   * ABI 37 kind.  SKI_SUM, the additive KISS-GP model (one 1-D grid per input dimension, summed): A0 = t [B, P, M], the
   * first columns of the P Toeplitz terms, R = M <= LO_TOEPLITZ_MAX_M, n2 = J, nterms = P in 1 .. LO_SKI_SUM_MAX_TERMS
   * (`terms` unused), N the rows, `interp` a lo_interp_desc whose four arrays are [B, P, N, J], the term index second --
   * exactly the tensors the base operator holds for its batch (*batch, P) -- with grid_ndim = 0 and right_plan NULL or
   * the copy lo_interp_plan_build makes for (B P, N, J, M) (same layout again, no new member).  The kind's own
   * (diag_mode, d) has d of [B, N] or [B].  An index outside [0, M) contributes nothing and is never dereferenced.
   * Terms are summed in ascending order after each term's own sum over j; with P = 1 the product and the pivoted
   * Cholesky rows have the bits of LO_OP_SKI_DIAG on the same arrays.  Lowered for lo_matvec_f32, the streaming CG,
   * Lanczos, fp32 MINRES and the fp32 pivoted Cholesky (row of pivot q: row[i] = sum_p of the SKI row of term p; the
   * diagonal is the EXACT one, sum_p sum_a sum_b t_p[|li[p,i,a] - ri[p,i,b]|] lv[p,i,a] rv[p,i,b], which is what the
   * reference's SumBatch._diagonal gives its pivot search -- not the approximate one of LO_OP_SKI_DIAG); the fp64 entry
   * points, the resident / fused engines and the solve sessions return LO_ERR_UNSUPPORTED; not a term kind of
   * LO_OP_SUM, not a base kind of LO_OP_MASKED or of lo_block_mv_f32.
   * LO_ERR_BADARG: a null A0 / interp / array in it, P < 1, J < 1, M < 1; LO_ERR_UNSUPPORTED: P > LO_SKI_SUM_MAX_TERMS,
   * M > LO_TOEPLITZ_MAX_M, B P > 65535, N J or M beyond the 32-bit limits of the interpolation kernels;
   * LO_ERR_WORKSPACE: a short workspace.  All before any launch.
   * ABI 38 kind.  KERNEL_LMC, the linear model of coregionalisation: A0 = X [B, n, D], R = D <= LO_KERNEL_MAX_DIM,
   * A1 = theta [B, Q, D + 1] exactly as for KERNEL_SUM (per term the D inverse lengthscales, then outputscale^2),
   * nterms = T in 1 .. LO_KERNEL_KRON_MAX_TASKS, N = n T, `task` = Bt [B, Q, T, T] on the DEVICE, every B_q used as
   * given, symmetric or not; n2 = the Q family codes, four bits per term, term 0 lowest as for KERNEL_SUM, and Q itself,
   * 1 .. LO_KERNEL_MAX_TERMS, in bits 16 .. 19 (same layout again, no new member).  Lowered for lo_matvec_f32, the
   * streaming CG, Lanczos, fp32 MINRES and the fp32 pivoted Cholesky (diagonal sum_q theta_q[D] B_q[t,t], row (p, tau):
   * row[j T + s] = sum_q (theta_q[D] g_q(r_q,pj)) B_q[tau, s], both in term order); the fp64 entry points, the resident /
   * fused engines and the solve sessions return LO_ERR_UNSUPPORTED; not a term kind of LO_OP_SUM, not a base kind of
   * LO_OP_MASKED.
   * LO_ERR_BADARG: a null A0 / A1 / task, R < 1, Q < 1, T < 1, N % T != 0, a family nibble outside 0 .. 3 (or set beyond
   * the Q terms), set bits of n2 above bit 19; LO_ERR_UNSUPPORTED: Q > LO_KERNEL_MAX_TERMS, T >
   * LO_KERNEL_KRON_MAX_TASKS, D > LO_KERNEL_MAX_DIM, sizes beyond the 32-bit limits of the sweep (B > 65535, n or n T >
   * 0x7ffffe00, T c > 0x7fffffff); LO_ERR_WORKSPACE: a short workspace.  All before any launch.
   * ABI 39 kind.  KERNEL_PARAM: A0 = X [B, N, D], R = D <= LO_KERNEL_PARAM_MAX_DIM, n2 = the family code LO_KERNEL_RQ or
   * LO_KERNEL_PERIODIC (the codes 0 .. 3 belong to KERNEL and are refused here, as 16 and 17 are refused there),
   * A1 = theta [B, 2 D + 2], one layout for both families (same layout of lo_op_desc again, no new member):
   *   theta[0 .. D)            the D INVERSE lengthscales (a shared one replicated by the host)
   *   theta[D]                 outputscale^2
   *   theta[D + 1]             alpha (RQ; PERIODIC ignores it, the host writes 0)
   *   theta[D + 2 .. 2 D + 2)  the D INVERSE periods (PERIODIC, a shared one replicated; RQ ignores them)
   * Lowered for lo_matvec_f32, the streaming CG, Lanczos, fp32 MINRES and the fp32 pivoted Cholesky (constant diagonal
   * theta[D], row of pivot p: row[j] = theta[D] g(x_p, x_j)); a term kind of LO_OP_SUM next to KERNEL (its own plan, its
   * own row source: periodic + RBF + noise is one LO_OP_SUM); the fp64 entry points, the resident / fused engines and the
   * solve sessions return LO_ERR_UNSUPPORTED; not a base kind of LO_OP_MASKED (nor a term of a masked sum); not grouped
   * into KERNEL_SUM.  LO_ERR_BADARG: a null A0 / A1, R < 1, a family other than 16 / 17; LO_ERR_UNSUPPORTED: D >
   * LO_KERNEL_PARAM_MAX_DIM, B > 65535, N > 0x7ffffe00; LO_ERR_WORKSPACE: a short workspace.  All before any launch.
   * ABI 40 kind.  KERNEL_SM: A0 = X [B, N, D], R = D <= LO_KERNEL_SM_MAX_DIM, n2 = the number of mixtures Q in 1 ..
   * LO_KERNEL_SM_MAX_MIX, A1 = theta [B, Q, 2 D + 1], per mixture the RAW values (no inverses, no outputscale):
   *   theta[q][0]                  the weight w_q
   *   theta[q][1 .. D + 1)         the D means mu_q (frequencies; the sign of a mean does not change K)
   *   theta[q][D + 1 .. 2 D + 1)   the D scales sigma_q
   * Lowered for lo_matvec_f32, the streaming CG, Lanczos, fp32 MINRES and the fp32 pivoted Cholesky (constant diagonal
   * sum_q w_q added in ascending q, row of pivot p: row[j] = K(x_p, x_j)); a term kind of LO_OP_SUM next to KERNEL and
   * KERNEL_PARAM (SM + RBF + noise is one LO_OP_SUM); the fp64 entry points, the resident / fused engines and the solve
   * sessions return LO_ERR_UNSUPPORTED; not a base kind of LO_OP_MASKED (nor a term of a masked sum); not grouped into
   * KERNEL_SUM.  LO_ERR_BADARG: a null A0 / A1, R < 1, Q < 1; LO_ERR_UNSUPPORTED: D > LO_KERNEL_SM_MAX_DIM, Q >
   * LO_KERNEL_SM_MAX_MIX, B > 65535, N > 0x7ffffe00; LO_ERR_WORKSPACE: a short workspace.  All before any launch.     */
} lo_op_desc;

/* The grid shape of an LO_OP_TOEPLITZ_KRON_DIAG descriptor (host struct). */
struct lo_grid_desc { /* (a plain struct tag, as lo_mask_desc) */
  int32_t ndim;      /* D: 2 or 3 */
  int32_t reserved;
  int64_t m[3];      /* M_1 .. M_D (m[2] unused when D == 2), each <= LO_SKI_GRID_MAX_AXIS */
};

/* The base operator and the selected rows of an LO_OP_MASKED descriptor (masked_linear_operator.py:17-35 with
 * row_mask == col_mask): y = S (base) S^T v + d o v, S selecting the rows idx of the base.  base: HOST descriptor of
 * kind LOWRANK_DIAG, DENSE_DIAG, KRON_DIAG or SUM with any diagonal mode of its own (CALLBACK, MASKED, SKI, SKI_GRID,
 * TOEPLITZ, TOEPLITZ_KRON, HADAMARD, KERNEL: LO_ERR_UNSUPPORTED).  idx: DEVICE pointer, int64 [M], strictly increasing, one list for all members; an
 * entry outside [0, base->N) contributes nothing and is never dereferenced (the convention of lo_interp_desc).      */
struct lo_mask_desc { /* (a plain struct tag: C callers write `struct lo_mask_desc`) */
  const struct lo_op_desc* base;
  const int64_t* idx; /* [M] */
  int64_t M;
};

/* The interpolation matrices of an LO_OP_SKI_DIAG descriptor (interpolated_linear_operator.py:43-92): row n of W_l
 * holds left_vals[b, n, :] at grid points left_idx[b, n, :] (int64, exactly as the operator stores them), W_r likewise.
 * The right side may share the left side's pointers.  Index entries outside [0, M) contribute nothing (the kernels
 * never read out of bounds).  Device pointers in a host struct.
 * right_plan: NULL, or the grid-major copy of W_r that lo_interp_plan_build made from right_idx (same B, N, J, M) and
 * the caller keeps across calls; with NULL every matvec plan (one per lo_matvec_f32 / solve call) builds its own.  */
typedef struct lo_interp_desc {
  const int64_t* left_idx;   /* [B, N, J] */
  const float* left_vals;    /* [B, N, J] */
  const int64_t* right_idx;  /* [B, N, J] */
  const float* right_vals;   /* [B, N, J] */
  const void* right_plan;    /* optional, see above */
  /* ABI 23, LO_OP_SKI_GRID_DIAG only (LO_OP_SKI_DIAG ignores them; 0 = the ABI-16 meaning, a 1-D grid): the grid shape */
  int32_t grid_ndim;         /* D: 2 or 3 */
  int32_t grid_reserved;
  int64_t grid_m[3];         /* M_1 .. M_D (grid_m[2] unused when D == 2), each <= LO_SKI_GRID_MAX_AXIS */
} lo_interp_desc;

/* Callbacks for LO_OP_CALLBACK and for a user preconditioner closure.
 * v, y: device pointers [B, N, c] fp32 contiguous.  Must enqueue on `stream`.  Return 0 on success. */
typedef int (*lo_matvec_cb)(void* user, const float* v, float* y, int64_t B, int64_t N, int64_t c, void* stream);

/* Pivoted-Cholesky/QR Woodbury preconditioner  P = L L^T + D  (added_diag_linear_operator.py:95-184)
 * in the form the reference caches it: z = r/d - Q (Q^T r)   (non-constant diag, :140)
 *                                     z = (r - Q Q^T r)/sigma (constant diag, :137-139)          */
typedef struct lo_precond_desc {
  int32_t k;             /* rank of Q (<= 256)                                                    */
  int32_t ldq;           /* row stride of Q in floats: k, or the zero-padded stride (4 * pow2) that   *
                          * lo_precond_build_f32 emits (no staging copy in that case)               */
  int32_t constant_diag; /* 1: `dinv` holds 1/sigma per member [B]; 0: `dinv` holds 1/d [B,N]      */
  int32_t reserved;
  const float* Q;        /* [B, N, ldq]  (_q_cache; for constant diag it carries the 1/sqrt(sigma)  *
                          * factor so that z = r*dinv - Q (Q^T r) in both cases)                    */
  const float* dinv;     /* reciprocal noise                                                       */
  /* Optional ROOT FORM of the same preconditioner (lo_precond_root_form_f32), valid when the operator is
   * LO_OP_LOWRANK_DIAG and the factor L is the pivoted Cholesky factor of ITS root C: every column of L lies in the
   * column space of C (L = C M), hence  P^-1 r = (r - C F (C^T (r o dinv))) o dinv  with the R x R matrix
   * F = M (I + M^T E M)^-1 M^T, E = C^T D^-1 C.  The operator-resident CG kernels then need no second tall matrix and
   * one group all-reduce per iteration.  NULL = not available (Q is used).                                        */
  const float* F;        /* [B, rf_ld, rf_ld], zero padded, symmetric                               */
  const float* EF;       /* [B, rf_ld, rf_ld] = E F                                                 */
  const float* E;        /* [B, rf_ld, rf_ld] = C^T D^-1 C                                          */
  int32_t rf_ld;         /* row stride of F / EF / E = padded root rank (8, 16 or 32); 0 = absent   */
  int32_t generation;    /* (was reserved2) optional: a number the host changes whenever it rebuilds this cache; part of
                          * the key under which lo_cg_solve_f32 remembers that a solve missed the stop rule in its
                          * result-only pass, so that an ADDRESS the allocator recycles does not inherit the memo.  0 = none.
                          * Results are bit-reproducible per cache state (form of the cache x memo), not across them.      */
  /* Optional KRONECKER ROOT FORM of the same preconditioner (lo_precond_kron_root_f32), valid when the operator is
   * LO_OP_KRON_DIAG with a constant diagonal and L is the pivoted Cholesky factor of K1 (x) K2 with k <= 16 pivots.
   * Row pi of K1 (x) K2 is the Kronecker product of row pi / n2 of K1 and row pi % n2 of K2, and every column of L
   * is a combination of the pivot rows (L = KP M, KP[(i1, i2), m] = kron_a[i1][m] * kron_b[i2][m]), hence
   *   P^-1 r = (r - KP F KP^T (r o dinv)) o dinv,   F = (KP[pivots, :] + KP^T D^-1 KP)^-1  (k x k).
   * The single-column CG iteration of large N (csrc/lo_precond_fused.hip) then forms the rows of KP on the fly from
   * 16 (n1 + n2) floats per member instead of streaming the 16 N floats of Q.  NULL = not available (Q is used).  */
  const float* kron_a;   /* [B, n1, 16]: kron_a[i1][m] = K1[pi_m / n2, i1], columns >= k zero       */
  const float* kron_b;   /* [B, n2, 16]: kron_b[i2][m] = K2[pi_m % n2, i2]                          */
  const float* kron_F;   /* [B, 16, 16], symmetric, zero padded                                     */
  /* Optional R-SPACE FORM next to the root form (lo_precond_root_form_rs_f32; round 5, ABI 11): the fp64 matrices
   * E = C^T D^-1 C | F E | E F E | G2 = C^T C | F | E F, [B, 6, rf_ld, rf_ld], zero padded.  With A P^-1 = I + C (I - F - E F) C^T D^-1
   * every vector of linear_cg (linear_cg.py:245-332) is a combination of the right-hand side and the columns of C, so
   * the iterations of a single-column, result-only solve run on R + 1 coordinates (csrc/lo_rspace.hip): the rows of C
   * are touched twice per solve and a member costs one group all-reduce.  The Gram matrices have to be fp64-accurate
   * (tests/proto/proto_rspace.py); D^-1 is `dinv` as stored (FULL) / 1.0 / (double)sigma (CONST).  NULL = not available. */
  const double* RS;
  /* Optional DIAGONAL FORM of the R-space iteration (lo_precond_eigform_f32; round 5, ABI 13): fp64 [B, 6, rf_ld, rf_ld] =
   * TinT | E^+ | TuT | G2 = C^T C | Tin | {row 0: lam, row 1: status, sweeps, sweeps, rank}.  In the basis that diagonalises the
   * preconditioned member on span(C) (two Jacobi eigendecompositions per member, csrc/lo_eigform.hip) linear_cg is the
   * CG of a diagonal matrix: one reduction of three values per iteration and no R x R product on the dependent chain
   * (k_cg_rspace<.., true>).  Worth building when the cache serves more than one solve (it costs two R x R
   * eigendecompositions per member); same iterates as the RS form to fp64 rounding (tests/proto/proto_eigform.py).
   * NULL = not available (the RS form is used).  Needs RS. */
  const double* RSD;
} lo_precond_desc;

/* Batch-sharded solves (one process per GPU, SURVEY.md section 8(e) "option A"): the reference's stopping rule is the
 * mean residual over the WHOLE batch (linear_cg.py:302-308).  When the batch is split over ranks the engine hands the
 * local statistics to this hook at every stopping-rule evaluation; the hook all-reduces (SUM) the three values in
 * place over the ranks (8-byte-class collective: torch.distributed / RCCL on the host side) and every rank takes the
 * same decision.  vals = {sum of residual norms, number of (member, column) pairs, abort request (NaN seen)}.
 * All ranks call it the same number of times (once per iteration from the first possible stop on).  Returns 0 on success. */
typedef int (*lo_stop_reduce_cb)(void* user, double* vals /* [3], in/out */);

/* linear_cg arguments that are scalars in the reference signature (linear_cg.py:98-109). */
typedef struct lo_cg_params {
  int64_t c;                /* number of right-hand-side columns                                  */
  int32_t n_tridiag;        /* tridiagonalise the first n_tridiag columns (0 = none)              */
  int32_t max_iter;         /* n_iter (already min'ed with N if terminate_cg_by_size, :170)        */
  int32_t max_tridiag_iter; /* n_tridiag_iter = min(max_tridiag_iter, N) (:171)                    */
  int32_t floor_max_iter;   /* the caller's ORIGINAL max_iter for the stop-rule floors min(10, max_iter-1) and
                             * min(n_tridiag_iter, max_iter-1) (:303-305), which the reference evaluates with the
                             * unclipped value; 0 = same as max_iter                                */
  float tolerance;          /* settings.cg_tolerance (:150-151)                                    */
  float eps;                /* 1e-10 (:104)                                                        */
  float stop_updating_after;/* 1e-10 (:105)                                                        */
  float pad;
  lo_stop_reduce_cb stop_reduce; /* NULL: the stopping rule sees this call's batch only (single process, or
                                  * "option B": per-shard rule); else the batch-global rule over all ranks */
  void* stop_reduce_user;
} lo_cg_params;

/* What the reference reports through its warning text / exception (host-readable after the call). */
typedef struct lo_cg_info {
  int32_t iterations;        /* loop bodies executed (k+1 of linear_cg.py:343)                     */
  int32_t matvecs;           /* operator applications actually executed                            */
  int32_t tolerance_reached; /* linear_cg.py:307                                                   */
  int32_t nan_detected;      /* linear_cg.py:199-200                                               */
  int32_t skipped;           /* all columns converged before the first iteration (:207-208)        */
  int32_t last_tridiag_iter; /* t_mat is valid on [0..last_tridiag_iter]^2 (:353)                  */
  float mean_residual;       /* residual_norm.mean() at exit (:343)                                */
  float reserved;
} lo_cg_info;

/* ---- library ------------------------------------------------------------------------------- */
/* ABI version (40; bumped on any signature change) and the gfx arch string the code objects target. */
int lo_abi_version(void);
const char* lo_target_arch(void);

/* ---- structured matvecs: LinearOperator._matmul for the hot-path operator classes ----------- */
/* y[B,N,c] = A v.  Replaces AddedDiagLinearOperator._matmul (added_diag_linear_operator.py:72-76)
 * over RootLinearOperator._matmul (root_linear_operator.py:68-72), DenseLinearOperator._matmul
 * (dense_linear_operator.py:60-64), KroneckerProductLinearOperator._matmul
 * (kronecker_product_linear_operator.py:272-284), Diag/ConstantDiag (diag_linear_operator.py:203-230). */
size_t lo_matvec_workspace_bytes(const lo_op_desc* op, int64_t c);
int lo_matvec_f32(const lo_op_desc* op, const float* v, float* y, int64_t c, void* ws, size_t ws_bytes, void* stream);

/* ---- linear_cg (linear_operator/utils/linear_cg.py:98-359) ----------------------------------- */
/* Solves A X = rhs for all B members and c columns with the reference's modified preconditioned CG
 * (column normalisation, masked alpha/beta, batch-global stopping rule, CG-coefficient tridiagonals).
 *   op        structured operator, or kind LO_OP_CALLBACK with (matvec, matvec_user)
 *   pre       NULL | Woodbury-QR preconditioner;  precond_cb non-NULL = opaque preconditioner closure
 *   rhs       [B,N,c]      x0  [B,N,c] or NULL (zeros)        x  [B,N,c] out
 *   t_mat     [n_tridiag, B, T, T] out, T = max_tridiag_iter, zero-filled by the call; the caller crops
 *             to [: last_tridiag_iter+1]^2 (linear_cg.py:353-357)
 * SYNCHRONOUS for the caller's purposes: returns with `info` filled and x / t_mat complete on `stream`.  When the solve
 * ends inside the resident launches, the status block arrives through pinned host memory (a ticket the control kernel
 * writes last) and the call returns without a hipStreamSynchronize: work the caller queued on `stream` BEFORE the call
 * is complete, but the stream's tail event may not have retired yet -- order later work by the stream, not by the
 * host.  Otherwise polls the device stop flag between launch chunks.
 * Resident single-column solve (k_cg_rspace3; lo_cg_session_solve_f32 too): when the call returns, `info` is FINAL and x
 * is complete IN STREAM ORDER -- work on `stream`, or on a stream that waits for it, sees all of x; a reader that
 * bypasses stream order (a host read of mapped memory, another stream without an event) does not.  This has always
 * been so: the ticket was written by one workgroup of the last group behind its own x pass while the group's other
 * workgroups could still be storing x.  The kernel now sends it in front of that pass (nothing the ticket reports
 * depends on x); with peer buffers installed (lo_peer_gather_set) it still leaves behind the pass.            */
size_t lo_cg_workspace_bytes(const lo_op_desc* op, const lo_precond_desc* pre, const lo_cg_params* prm);
int lo_cg_solve_f32(const lo_op_desc* op, lo_matvec_cb matvec, void* matvec_user, const lo_precond_desc* pre,
                    lo_matvec_cb precond_cb, void* precond_user, const lo_cg_params* prm, const float* rhs,
                    const float* x0, float* x, float* t_mat, void* ws, size_t ws_bytes, lo_cg_info* info,
                    void* stream);

/* ---- prototype: the gather of SURVEY 8(e) as peer writes (round 6) ------------------------------------------------ */
/* north_star: "independent batch elements shard across the 8 GPUs of one node with an RCCL all-gather over xGMI at the
 * end".  Instead of a collective kernel that has to share the CUs with the spin-waiting resident groups, the x pass of the
 * resident single-column solve (k_cg_rspace3) can store every solution value into up to seven more buffers: the IPC-mapped
 * gather buffers of the peers, bufs[p] [B_total, N] fp32, this rank's members starting at `member_offset`.  The pointers
 * are process-wide and stay installed until replaced (n = 0 removes them); only the diagonal-form resident solve honours
 * them.  Emulated on one GPU with local buffers by tools/mb_peer_gather.py; no reference counterpart.                 */
int lo_peer_gather_set(float* const* bufs, int n, long long member_offset);

/* ---- engine selection of lo_cg_solve_f32 as a PURE function ------------------------------------------------------ */
/* Which kernels lo_cg_solve_f32 will run for these arguments: decided from the shapes, the null-ness of the pointers in
 * `pre`, the parameters and the number of compute units -- no device memory is read and nothing is launched, so the
 * selection matrix is testable on a machine without a GPU (tests/test_host_api.py holds the table).  lo_cg_solve_f32
 * executes exactly this plan; what is left to run time are the fall-backs after an occupancy query refuses a kernel
 * (next engine down) or a group hand-off times out (streaming engine).
 *   cus  compute units to plan for; <= 0: the current device (LO_OC_RESERVE_CUS applied)                             */
#define LO_ENGINE_NONE 0          /* no serial resident columns                                                 */
#define LO_ENGINE_RESIDENT_GEN1 1 /* (k_cg_onchip of rounds 1 - 5: removed in round 6, never reported any more)          */
#define LO_ENGINE_RESIDENT_GEN2 2 /* k_cg_onchip4 (four rows per thread, Q form, columns one after the other)    */
#define LO_ENGINE_RESIDENT_ROOT 3 /* k_cg_onchip5 (root-form preconditioner, one all-reduce per iteration)       */
#define LO_STREAM_PRE_NONE 0       /* unpreconditioned update                                                    */
#define LO_STREAM_PRE_TWO_PASS 1   /* Q^T r, then z = r/d - Q u (two passes over Q)                              */
#define LO_STREAM_PRE_CLOSURE 2    /* opaque preconditioner closure                                              */
#define LO_STREAM_PRE_FUSED_Q 3    /* k_precond_fused: one pass over Q, r / x / p updates fused                  */
#define LO_STREAM_PRE_FUSED_KRON 4 /* k_precond_fused_kron: Kronecker root form, no Q traffic                    */
#define LO_STREAM_PRE_FUSED_COLS 5 /* k_cg_step_cols: up to 32 columns, the whole step behind the product (alpha, r / x,
                                    * Q form of the preconditioner, beta, p, control step) in one launch              */
#define LO_STREAM_NOPRE_FUSED_COLS 6 /* the same launch without a preconditioner (z = r)                              */
typedef struct lo_cg_plan {
  int32_t resident;             /* 1: the iterations up to the first possible stop run in operator-resident launches */
  int32_t resident_iterations;  /* how many (first_stop_iteration + 1), 0 if not resident                            */
  int32_t lockstep_cols;        /* columns [0, lockstep_cols) advance 16 at a time on k_cg_lockstep                  */
  int32_t lockstep_group;       /* workgroups per member of that kernel                                              */
  int32_t serial_engine;        /* LO_ENGINE_*: the kernel of the columns [lockstep_cols, c)                         */
  int32_t serial_group;         /* workgroups per member of that kernel                                              */
  int32_t lean;                 /* 1: result-only first pass (state written by a repeat only if CG has to continue)  */
  int32_t needs_q;              /* 1: `pre` carries the root form only and no resident kernel takes the solve:
                                 * lo_cg_solve_f32 returns LO_ERR_UNSUPPORTED, the caller builds the Q form          */
  int32_t streaming_precond;    /* LO_STREAM_PRE_*: the preconditioner step of iterations beyond the resident ones
                                 * (all iterations when resident == 0)                                               */
  int32_t poll_chunk;           /* streaming iterations enqueued between two reads of the control block              */
  int32_t first_stop_iteration; /* min(10, max_iter-1), raised to min(max_tridiag_iter, max_iter-1) with tridiagonals
                                 * (linear_cg.py:302-308)                                                            */
  int32_t streaming_iterations; /* lo_cg_last_executed: streaming iterations enqueued after the resident phase (all of
                                 * them when resident == 0); 0 in a plan                                              */
  int32_t rspace;              /* round 5 (needs lo_precond_desc.RS): the result-only first pass runs the iterations on
                                 * R + 1 coordinates (csrc/lo_rspace.hip): 2 = the single column inside the resident
                                 * launch of `serial_engine` (one all-reduce per member), 1 = ALL columns in three
                                 * streaming launches (k_rs_part / k_rs_iter / k_rs_apply) -- lockstep_cols /
                                 * serial_engine then name the engines of the repeat with the state                  */
  int32_t rspace_diag;          /* lo_cg_last_executed: 1 = the rspace == 2 launch ran the diagonal form (RSD)           */
} lo_cg_plan;
int lo_cg_plan_f32(const lo_op_desc* op, const lo_precond_desc* pre, int has_precond_cb, int has_x0,
                   const lo_cg_params* prm, int cus, lo_cg_plan* plan);
/* The plan as the calling thread's last successful lo_cg_solve_f32 EXECUTED it (after run-time fall-backs, with
 * `streaming_iterations` and `rspace_diag` filled in): the GPU tests compare it with lo_cg_plan_f32.          */
int lo_cg_last_executed(lo_cg_plan* plan);

/* ---- fused end-to-end solve: ONE resident launch ------------------------------------------------- */
/* A.solve(rhs) of AddedDiag(LowRankRoot(C), Diag | ConstantDiag) end to end, the operator read from HBM once:
 *   PivotedCholesky.forward   (functions/_pivoted_cholesky.py:14-105; `rank` pivots of C C^T)
 *   -> AddedDiagLinearOperator._init_cache (operators/added_diag_linear_operator.py:144-184; in ROOT FORM, see
 *      lo_precond_desc.F / EF: L = C M is never written to memory)
 *   -> linear_cg              (utils/linear_cg.py:98-359; the iterations of the reference's floor, :302-308)
 * per member inside one kernel (csrc/lo_solve_fused_impl.h).  The two BATCH-GLOBAL decisions of the reference cannot
 * be taken inside (members are in flight at different times); they are checked after the launch and reported in
 * `info->status`:
 *   LO_FUSED_OK          x holds the reference's result (every member took all `rank` pivots on its own error and the
 *                        stopping rule held at the floor) -- also when nan_detected / skipped are set
 *   LO_FUSED_EARLY_STOP  some member's own pivot error reached error_tol (or NaN) before `rank` pivots: the shared
 *                        pivot count (_pivoted_cholesky.py:57) needs the three-launch path
 *   LO_FUSED_CONTINUE    the tolerance was not met at the floor: CG has to continue (three-launch path)
 *   LO_FUSED_TIMEOUT     a group exchange timed out (co-residency lost)
 * In the last three cases x is NOT valid and the caller redoes the solve with lo_pivoted_cholesky_f32 +
 * lo_precond_root_form_f32 / lo_precond_build_f32 + lo_cg_solve_f32.
 *   op       LO_OP_LOWRANK_DIAG, R in {8, 16, 32}, 256 <= N <= 16384, diag FULL or CONST
 *   rank     pivots (settings.max_preconditioner_size, 1..16), error_tol = settings.preconditioner_tolerance
 *   prm      as lo_cg_solve_f32 (n_tridiag == 0, no stop_reduce, c <= 8)
 *   x        [B, N, c] out
 *   F, EF, E [B, R, R] out, dinv [B, N] | [B] out, logdet_p [B] out: the root-form preconditioner for later solves
 *            (any may be NULL); swaps [B, rank] int32 out: position exchanged with position m at pivot m -- the
 *            reference's permutation is the identity with these exchanges applied in order (lo_solve_fused_perm)
 * SYNCHRONOUS (one read-back of the status block).  lo_solve_fused_supported: 1 if the shape is taken.            */
#define LO_FUSED_OK 0
#define LO_FUSED_EARLY_STOP 1
#define LO_FUSED_CONTINUE 2
#define LO_FUSED_TIMEOUT 3
typedef struct lo_fused_info {
  int32_t status;            /* LO_FUSED_*                                                         */
  int32_t iterations;        /* as lo_cg_info                                                      */
  int32_t matvecs;
  int32_t tolerance_reached;
  int32_t nan_detected;
  int32_t skipped;
  int32_t rank;              /* pivots taken (= rank when status is LO_FUSED_OK)                   */
  float mean_residual;
} lo_fused_info;
int lo_solve_fused_supported(const lo_op_desc* op, int32_t rank, const lo_cg_params* prm);
size_t lo_solve_fused_workspace_bytes(const lo_op_desc* op, int32_t rank, const lo_cg_params* prm);
int lo_solve_fused_f32(const lo_op_desc* op, int32_t rank, float error_tol, const lo_cg_params* prm, const float* rhs,
                       float* x, float* F, float* EF, float* E, float* dinv, float* logdet_p, int32_t* swaps,
                       void* ws, size_t ws_bytes, lo_fused_info* info, void* stream);
int lo_solve_fused_perm(const int32_t* swaps, int64_t B, int64_t N, int32_t rank, int64_t* perm, void* stream);

/* Development / test switch: 0 forces the streaming (multi-kernel) engine, 1 (default) allows the operator-resident
 * fast path (csrc/lo_cg_onchip.hip) for low-rank + Woodbury-preconditioned single-column solves.  Same results
 * up to summation order. */
int lo_cg_set_onchip(int enable);

/* ---- the gate of the resident kernels (round 5, ABI 12) ------------------------------------------ */
/* The resident kernels need every workgroup of a group co-resident.  When a group exchange times out (another
 * kernel -- RCCL's, another process' -- holds part of the CUs) the call is redone on the streaming engines and the
 * next `backoff` entry-point calls (lo_cg_solve_f32 / lo_pivoted_cholesky_f32) skip the resident kernels; then they
 * are tried again.  Timeouts right after a re-arm double the cool-down (16 .. 4096 calls), a clean resident solve
 * resets it.  (Rounds 2 - 4 latched the resident kernels off for the life of the process.)
 * lo_resident_inject_timeouts(n): the next n resident CG launches are treated as timed out (tests, bench --inject). */
typedef struct lo_resident_status {
  int32_t user_disabled;  /* lo_cg_set_onchip(0)                                                   */
  int32_t timeouts;       /* hand-off timeouts since the library was loaded                        */
  int32_t cooldown;       /* entry-point calls still to be served by the streaming engines         */
  int32_t backoff;        /* length of the next cool-down                                          */
  int32_t rearms;         /* cool-downs that ended (resident kernels tried again)                  */
  int32_t fused_timeouts; /* of `timeouts`: inside lo_solve_fused_f32                              */
} lo_resident_status;
int lo_resident_status_get(lo_resident_status* out);
int lo_resident_inject_timeouts(int32_t n);
/* The headline solve (one column, diagonal R-space form: k_cg_rspace3) keeps what its workgroups share -- error word,
 * member and close counters, exchange and close granules -- in ONE buffer per device that the library allocates and zeroes
 * on first use; launches are told apart by a host-assigned tag base and epoch, so no clearing launch runs in front of a
 * solve.  The buffer is cleared again when a counter would wrap and after any launch the host did not see closing clean.
 * Test / debug access for the current device: force_clear != 0 makes the next such launch clear the buffer first;
 * set_next_tag / set_next_epoch >= 0 replace the counters (to reach the wrap-around); out (or NULL) receives
 * {next tag base, next epoch, clears so far, launches so far}.                                                        */
int lo_resident_handoff_debug(int32_t force_clear, int64_t set_next_tag, int64_t set_next_epoch, uint32_t* out);
/* The order in which k_cg_rspace3 walks the members of a batch is UNSPECIFIED: x, `info` and every record are the same
 * bit for bit in any order.  The library uses the freedom: a solve on the operator (C, B, N, padded rank) of the
 * previous solve on the library's buffer, when that one closed clean, walks the members from B - 1 down, so that it
 * starts with what the previous solve left in the memory-side cache; every other solve walks from 0 up (ABI 32).
 * Test / debug access for the current device: mode -1 leaves the rule as it is, 0 automatic (the rule above), 1 always
 * from 0 up, 2 always from B - 1 down (forced modes hold for launches on the caller's workspace too, e.g. under
 * LO_OC_DEBUG); out (or NULL) receives {direction of the last launch: 0 up, 1 down; launches that walked down so far}. */
int lo_resident_order_debug(int32_t mode, uint32_t* out);
/* The ordered start of k_cg_rspace3 (ABI 35).  The dispatcher hands an XCD its workgroups in order and fills the first
 * slot of every compute unit before the second, so the groups of an XCD enter in two waves -- the lower and the upper
 * half of their local indices -- about 4 us apart.  In a launch of six rounds or more (rounds = members / groups,
 * rounded up) every workgroup of a group with a first member waits, at the kernel's entry and before it requests
 * anything, (the group's index inside its wave) x 200 ticks of the 100 MHz clock, provided no group of the layout would
 * wait more than three steps (groups of 8 workgroups or more on a whole device).  Groups that share compute units then
 * stay out of phase round after round.  The wait reads the clock and nothing else, never exceeds 800 ticks (8 us), and
 * enters no result.
 * Test / debug access for the current device: mode -1 leaves the rule as it is, 0 automatic (the rule above), 1 never,
 * 2 delta = 200 whatever the rounds and the layout, 3 delta_ticks (0 .. 800) -- forced modes hold for launches on the
 * caller's workspace too; out (or NULL) receives {mode in force; delta the last launch used, 0 = it did not wait; the
 * groups it was laid out in; launches that waited so far}.
 * lo_resident_start_delay evaluates the rule without a device: the ticks group `grp` of a launch of B members in
 * `ngroups` groups (a multiple of 8) waits under (mode, delta_ticks) as above, or -1 for arguments out of range.      */
int lo_resident_start_debug(int32_t mode, int32_t delta_ticks, uint32_t* out);
int lo_resident_start_delay(int32_t mode, int32_t delta_ticks, int64_t B, int32_t ngroups, int32_t grp);

/* ---- solve sessions: the headline solve without its per-call set-up (ABI 20) ---------------------------------------- */
/* A preconditioner cache serves many solves of one operator; what lo_cg_solve_f32 does before and after its one launch
 * for the headline plan (validation, the LO_* switches, the engine selection, the workspace carve) does not depend on the
 * right-hand side.  A session holds all of it: created once per (operator, cache, parameters), it takes one
 * right-hand side per call.
 *   create   copies the three structs; LO_ERR_UNSUPPORTED unless the plan is the single column inside ONE launch of
 *            k_cg_rspace3 on the library's hand-off buffer: lo_cg_plan.rspace == 2 and lean, c == 1, no tridiagonals,
 *            no x0, no callbacks, no stop_reduce, pre->RSD present, R and pre->ldq already padded, no debug or A/B
 *            switch set.  `workspace` (lo_cg_session_workspace_bytes: a control block and a few scalars per member, no
 *            N-vector) belongs to the session until it is destroyed; the tensors the structs point to must stay alive.
 *   solve    x [B,N,1] = A^-1 rhs as lo_cg_solve_f32 computes it, bit for bit; fills `info` and `executed` (what
 *            lo_cg_last_executed would report, which it also updates).  Returns LO_ERR_UNSUPPORTED -- the caller then
 *            runs lo_cg_solve_f32 with the same arguments on the same thread, where all of that logic lives -- when a
 *            LO_* switch or lo_cg_set_onchip differs from creation, during a cool-down, after a lost or injected
 *            hand-off time-out (counted once), for a right-hand side the diagonal form hands to the dense one, when the
 *            stop rule does not hold at the floor, on NaN, and under stream capture.  That rerun counts as the same
 *            entry-point call of a cool-down.  One solve at a time per session; synchronisation as lo_cg_solve_f32.
 *   destroy  frees the host state (NULL is allowed).  lo_cg_session_debug_live: sessions alive in this process.      */
struct lo_cg_session;
size_t lo_cg_session_workspace_bytes(const lo_op_desc* op, const lo_cg_params* prm);
int lo_cg_session_create_f32(const lo_op_desc* op, const lo_precond_desc* pre, const lo_cg_params* prm, void* workspace,
                             size_t workspace_bytes, struct lo_cg_session** out);
int lo_cg_session_solve_f32(struct lo_cg_session* s, const float* rhs, float* x, lo_cg_info* info, lo_cg_plan* executed,
                            void* stream);
void lo_cg_session_destroy(struct lo_cg_session* s);
int lo_cg_session_debug_live(void);

/* ---- PivotedCholesky.forward (linear_operator/functions/_pivoted_cholesky.py:14-105) ---------- */
/* Greedy partial pivoted Cholesky of the NON-diagonal part of `op` (op->d is ignored, as
 * added_diag_linear_operator.py:125 calls self._linear_op.pivoted_cholesky).
 *   L_rows  [B, max_rank, N] out (row m = column m of L; the host returns L_rows[:, :m].mT.contiguous())
 *   perm    [B, N] int64 out (full permutation; first m entries are the pivots)
 *   rank_out host int: number of pivots m taken (shared by the whole batch, :57)
 * SYNCHRONOUS (reads m back).                                                                      */
size_t lo_pivoted_cholesky_workspace_bytes(const lo_op_desc* op, int32_t max_rank);
int lo_pivoted_cholesky_f32(const lo_op_desc* op, int32_t max_rank, float error_tol, float* L_rows, int64_t* perm,
                            int32_t* rank_out, void* ws, size_t ws_bytes, void* stream);
/* The same for an operator that does not lower to a descriptor: the generic row fetch of the reference
 * (`matrix[..., pi_m, :]`, _pivoted_cholesky.py:81 -> LinearOperator.__getitem__ tensor-index branch,
 * operators/_linear_operator.py:2882-2902) stays a callback, everything else runs in the same kernels.
 *   diag    [B, N] device: matrix._diagonal() (:39)
 *   row_cb  fetches, for the pivots piv [B] (int64, DEVICE pointer), the rows K[b, piv[b], :] into rows [B, N];
 *           must enqueue on `stream` and must not synchronise; called once per pivot.  Returns 0 on success. */
typedef int (*lo_rowfetch_cb)(void* user, const int64_t* piv, float* rows, int64_t B, int64_t N, void* stream);
size_t lo_pivoted_cholesky_cb_workspace_bytes(int64_t B, int64_t N, int32_t max_rank);
int lo_pivoted_cholesky_cb_f32(int64_t B, int64_t N, const float* diag, lo_rowfetch_cb row_cb, void* row_user,
                               int32_t max_rank, float error_tol, float* L_rows, int64_t* perm, int32_t* rank_out,
                               void* ws, size_t ws_bytes, void* stream);

/* The same in float64 (round 4): PivotedCholesky.forward is dtype-generic in the reference.  Same streaming engine and
 * operation order; the descriptor's A0 / A1 are read as `const double*` (kinds LOWRANK / DENSE / KRON / SUM of those; d is
 * ignored), L_rows [B, max_rank, N] double.  No operator-resident fast path.                                          */
typedef int (*lo_rowfetch_cb_f64)(void* user, const int64_t* piv, double* rows, int64_t B, int64_t N, void* stream);
size_t lo_pivoted_cholesky_f64_workspace_bytes(const lo_op_desc* op, int32_t max_rank);
int lo_pivoted_cholesky_f64(const lo_op_desc* op, int32_t max_rank, double error_tol, double* L_rows, int64_t* perm,
                            int32_t* rank_out, void* ws, size_t ws_bytes, void* stream);
size_t lo_pivoted_cholesky_cb_f64_workspace_bytes(int64_t B, int64_t N, int32_t max_rank);
int lo_pivoted_cholesky_cb_f64(int64_t B, int64_t N, const double* diag, lo_rowfetch_cb_f64 row_cb, void* row_user,
                               int32_t max_rank, double error_tol, double* L_rows, int64_t* perm, int32_t* rank_out,
                               void* ws, size_t ws_bytes, void* stream);

/* ---- AddedDiagLinearOperator._init_cache* (added_diag_linear_operator.py:144-184) ------------- */
/* From L [B,N,k] and the diagonal builds Q [B,N,k] (the reference's _q_cache, up to the sign/rotation
 * freedom of a thin QR, which Q Q^T is invariant to), dinv and logdet_p [B].
 * Gram matrix + Cholesky + triangular solve in fp64, rounded once to fp32.            */
size_t lo_precond_build_workspace_bytes(int64_t B, int64_t N, int32_t k);
int lo_precond_build_f32(const float* L, const float* d, int32_t diag_mode, int64_t B, int64_t N, int32_t k, float* Q,
                         float* dinv, float* logdet_p, void* ws, size_t ws_bytes, void* stream);
/* Same with an explicit layout of L: element (member b, row i, column a) = L[b*ld_member + i*ld_row + a*ld_col].
 * (N*k, k, 1) is the reference's [B,N,k]; (max_rank*N, 1, N) consumes the L_rows that
 * lo_pivoted_cholesky_f32 writes without the transposed copy of _pivoted_cholesky.py:105.          */
int lo_precond_build_strided_f32(const float* L, int64_t ld_member, int64_t ld_row, int64_t ld_col, const float* d,
                                 int32_t diag_mode, int64_t B, int64_t N, int32_t k, float* Q, float* dinv,
                                 float* logdet_p, void* ws, size_t ws_bytes, void* stream);
/* Root form of the pivoted-Cholesky preconditioner of a low-rank operator (see lo_precond_desc): from the root
 * C [B, N, R] (R <= 32), the diagonal, the factor L (strided like lo_precond_build_strided_f32, k columns = pivots
 * taken) and the permutation of lo_pivoted_cholesky_f32 (first k entries = pivots) computes, in fp64,
 *   E = C^T D^-1 C,  M (L = C M: the recurrence of _pivoted_cholesky.py:77-92 on the pivot rows),
 *   F = M (I + M^T E M)^-1 M^T,  EF,  logdet P = logdet(I + M^T E M) + sum log d  (== the value of the Q form)
 * and writes F, EF, E as fp32 [B, rf_ld, rf_ld] (rf_ld = 8, 16 or 32 >= R), dinv ([B, N] FULL / [B] CONST), logdet_p [B]. */
size_t lo_precond_root_form_workspace_bytes(int64_t B, int64_t N, int32_t R);
int lo_precond_root_form_f32(const float* C, int32_t R, const float* d, int32_t diag_mode, const float* L,
                             int64_t ld_member, int64_t ld_row, int64_t ld_col, const int64_t* perm, int64_t B,
                             int64_t N, int32_t k, int32_t rf_ld, float* F, float* EF, float* E, float* dinv,
                             float* logdet_p, void* ws, size_t ws_bytes, void* stream);
/* The same with the R-SPACE FORM (lo_precond_desc.RS) as a fifth output: RS fp64 [B, 6, rf_ld, rf_ld] = E | F E | E F E | C^T C | F | E F.
 * E and C^T C are accumulated on the fp64 matrix cores from exact fp32 x fp32 products (the fp32 F / EF / E written next
 * to them are the roundings of the same fp64 matrices).  Needs R % 4 == 0 and a 16-byte aligned C: LO_ERR_UNSUPPORTED
 * otherwise (the caller uses lo_precond_root_form_f32).  Workspace: lo_precond_root_form_rs_workspace_bytes.          */
size_t lo_precond_root_form_rs_workspace_bytes(int64_t B, int64_t N, int32_t R);
int lo_precond_root_form_rs_f32(const float* C, int32_t R, const float* d, int32_t diag_mode, const float* L,
                                int64_t ld_member, int64_t ld_row, int64_t ld_col, const int64_t* perm, int64_t B,
                                int64_t N, int32_t k, int32_t rf_ld, float* F, float* EF, float* E, float* dinv,
                                float* logdet_p, double* RS, void* ws, size_t ws_bytes, void* stream);
/* The DIAGONAL FORM (lo_precond_desc.RSD) from the R-space form RS [B, 6, rf_ld, rf_ld] of a root of rank R (even,
 * <= rf_ld <= 32): RSD [B, 6, rf_ld, rf_ld].  One workgroup per member, fp64, two cyclic Jacobi eigendecompositions in LDS.
 * RSD[b][5][1][0] = 1.0 when the form is usable; -1.0 (an eigenvalue of the preconditioned member is not positive) or -2.0
 * ((s_max / s_min) (1 + s_max^2) of E's kept directions exceeds 1e9: the change of basis V S^-1 would cost more than 1e-7
 * of a solution that is a difference of large terms) otherwise -- the caller keeps the RS form, which stays in the
 * coordinates of C.  Replaces nothing in the reference: it is a cached re-expression of
 * added_diag_linear_operator.py:119-137's closure for linear_cg.py:245-332. */
int lo_precond_eigform_f32(const double* RS, int64_t B, int32_t R, int32_t rf_ld, double* RSD, void* stream);
/* Kronecker root form of the pivoted-Cholesky preconditioner (see lo_precond_desc.kron_*): op = LO_OP_KRON_DIAG with
 * LO_DIAG_CONST, L / perm as lo_precond_root_form_f32 (k <= 16 pivots).  Gathers the pivot rows of the two factors
 * (kron_a [B, n1, 16], kron_b [B, n2, 16]), forms E = KP^T KP / sigma as the Hadamard product of the two small Gram
 * matrices and runs the fp64 algebra of the root form: F [B, 16, 16].  kappa [B]: the factor by which the fp32 rounding
 * of KP^T (r / d) is amplified in P^-1 r, sqrt(sum_m (F E F)_mm E_mm) -- a few units for well separated pivots, large
 * when the pivot rows are nearly dependent (the caller then keeps the Q form).                                     */
size_t lo_precond_kron_root_workspace_bytes(int64_t B);
int lo_precond_kron_root_f32(const lo_op_desc* op, const float* L, int64_t ld_member, int64_t ld_row, int64_t ld_col,
                             const int64_t* perm, int32_t k, float* kron_a, float* kron_b, float* kron_F,
                             float* kappa, void* ws, size_t ws_bytes, void* stream);
/* z = P^{-1} r  (precondition_closure, added_diag_linear_operator.py:135-140) */
size_t lo_precond_apply_workspace_bytes(int64_t B, int64_t N, int32_t k, int64_t c);
int lo_precond_apply_f32(const lo_precond_desc* pre, const float* r, float* z, int64_t B, int64_t N, int64_t c, void* ws,
                         size_t ws_bytes, void* stream);

/* ---- lanczos_tridiag (linear_operator/utils/lanczos.py:9-164) --------------------------------- */
/*   init_vecs [B,N,P];  q_mat [max_iter, B, N, P] out;  t_mat [max_iter, max_iter, B, P] out (reference
 *   storage order, :69-77; the host permutes/crops as :151-161);  iters_out = k+1 (:151). SYNCHRONOUS. */
size_t lo_lanczos_workspace_bytes(const lo_op_desc* op, int64_t P, int32_t max_iter);
int lo_lanczos_tridiag_f32(const lo_op_desc* op, lo_matvec_cb matvec, void* matvec_user, const float* init_vecs,
                           int64_t P, int32_t max_iter, float tol, float* q_mat, float* t_mat, int32_t* iters_out,
                           void* ws, size_t ws_bytes, void* stream);
/* q_mat [k, B, N, P] (first k of the stored vectors, working order) -> [P, B, N, k], the layout lanczos.py:154
 * returns (permute(-1, batch, -2, 0).contiguous()).  Since round 4 the host mirror returns the permuted VIEW and the
 * consumers on the path read the native layout (lo_root_from_lanczos_native_f32): this copy is made on request only.  LO_ERR_UNSUPPORTED when k * 32 * (P + 1) floats exceed 64 KiB
 * of LDS (the host then permutes with torch).                                                       */
int lo_lanczos_permute_f32(const float* q_in, int32_t k, int64_t B, int64_t N, int64_t P, float* q_out, void* stream);
/* Epilogue of RootDecomposition.forward (functions/_root_decomposition.py:73-85) for PB = probes x batch members:
 * qv = q evecs, root = qv o sqrt(evals), inverse = qv / sqrt(evals); q, qv, root, inverse [PB, N, k], evecs
 * [PB, k, k], evals [PB, k]; any of the three outputs may be NULL.  k <= 32, else LO_ERR_UNSUPPORTED.      */
int lo_root_from_lanczos_f32(const float* q, const float* evecs, const float* evals, int64_t PB, int64_t N, int32_t k,
                             float* qv, float* root, float* inverse, void* stream);

/* The same epilogue on the basis in the layout lo_lanczos_tridiag_f32 WRITES it: q_native [k, B, N, P] (the first k stored
 * vectors) with evecs [P, B, k, k], evals [P, B, k]; outputs [P, B, N, k].  The [P, B, N, k] copy of lanczos.py:154 is
 * then never made.  LO_ERR_UNSUPPORTED: k > 32 or P (k k + 1 + k + (256 / P) k) floats beyond 64 KiB of LDS.           */
int lo_root_from_lanczos_native_f32(const float* q_native, const float* evecs, const float* evals, int64_t B, int64_t N,
                                    int64_t P, int32_t k, float* qv, float* root, float* inverse, void* stream);

/* ---- host glue of InvQuadLogdet as kernels (csrc/lo_probes.hip; round 4, ABI 10) ----------------------------- */
/* Probe vectors of InvQuadLogdet.forward (functions/_inv_quad_logdet.py:91-110) for the preconditioner P = L L^T + D of an
 * AddedDiagLinearOperator: z = L e1 + sqrt(d) o e2 (a draw from N(0, P): zero_mean_mvn_samples of the PsdSum,
 * sum_linear_operator.py:88-91), the column norms (:108), z / norm (:109) written into the FIRST P columns of the
 * right-hand-side block rhs_out [B, N, P + q], the q inv_quad columns copied behind them (the torch.cat of :131).
 *   L          element (b, n, j) at L[b * l_sb + n * l_sn + j * l_sk]  (any layout / broadcast batch), k <= 32 columns
 *   d          [B, N] (LO_DIAG_FULL) or [B] (LO_DIAG_CONST);  e1 [B, k, P], e2 [B, N, P] standard normal draws
 *   norms      [B, P] out;  ws: lo_probe_vectors_workspace_bytes.  P, q <= 64.  Asynchronous on `stream`.          */
size_t lo_probe_vectors_workspace_bytes(int64_t B, int64_t N, int64_t P);
int lo_probe_vectors_f32(const float* L, int64_t l_sb, int64_t l_sn, int64_t l_sk, int32_t k, const float* d,
                         int32_t diag_mode, const float* e1, const float* e2, const float* inv_quad_rhs, int64_t q,
                         int64_t B, int64_t N, int64_t P, float* rhs_out, float* norms, void* ws, size_t ws_bytes,
                         void* stream);
/* Element-wise part of InvQuadLogdet.backward (:183-213) in one pass.  solves [B, N, P + q]; pp [B, N, ldp] = the
 * preconditioner applied to the NORMALISED probes (first P columns read); norms [B, P]; g_ld [B] logdet grad;
 * g_iq [B, q] inv_quad grad (or NULL when q = 0); coef = 1 / P.  Outputs: left, right [B, N, P + q] (the factors of
 * linear_op._bilinear_derivative: [probe part | inv_quad part]) and pre_left, pre_right [B, N, P] (the factors of the
 * preconditioner's bilinear derivative, :211-213).                                                                  */
int lo_iql_backward_factors_f32(const float* solves, const float* pp, int64_t ldp, const float* norms, const float* g_ld,
                                const float* g_iq, float coef, int64_t B, int64_t N, int64_t P, int64_t q, float* left,
                                float* right, float* pre_left, float* pre_right, void* stream);

/* ---- lanczos_tridiag_to_diag + StochasticLQ.to_dense (lanczos.py:167-189, stochastic_lq.py:45-82) */
/* t_mat [M, T, T] (M = P*B tridiagonals, only the three diagonals are read) ->
 *   evals [M, T], evecs [M, T, T] (column j = eigenvector j; negative eigenvalues -> 1 and their
 *   eigenvector columns zeroed, lanczos.py:185-187).  evecs may be NULL.
 * If logdet != NULL (size B): logdet[b] = (n / P) * sum_p sum_i evecs[p,b,0,i]^2 log(evals[p,b,i]).
 * One thread per tridiagonal, implicit-shift QL in fp64; T <= 32 (the reference itself switches algorithm
 * at T >= 32, lanczos.py:179).                                                                      */
size_t lo_tridiag_eigh_slq_workspace_bytes(int64_t P, int64_t B);
int lo_tridiag_eigh_slq_f32(const float* t_mat, int64_t P, int64_t B, int32_t T, int64_t n, float* evals, float* evecs,
                            float* logdet, void* ws, size_t ws_bytes, void* stream);

/* ---- backward passes: `_bilinear_derivative` contractions -------------------------------- */
/* U = left_vecs [B,N,D], V = right_vecs [B,N,D] (fp32, contiguous); derivative of sum_d u_d^T K v_d w.r.t. the
 * tensor representing K.
 *   dense: out [B,N,N] = U V^T                               (dense_linear_operator.py:69-71)
 *   diag : out [B,N] = sum_d U o V; constant != 0: out [B] = sum_{n,d} U o V (ws: B*N floats)
 *                                                            (diag_linear_operator.py:37-45, :337-344)
 *   root : out [B,N,R] = U (V^T C) + V (U^T C) for K = C C^T, C [B,N,R]
 *          (autograd of root._matmul(root._t_matmul(v)), _linear_operator.py:336-393, root_linear_operator.py:68-72) */
int lo_bilinear_dense_f32(const float* U, const float* V, int64_t B, int64_t N, int64_t D, float* out, void* stream);
int lo_bilinear_diag_f32(const float* U, const float* V, int64_t B, int64_t N, int64_t D, int32_t constant, float* out,
                         void* ws, size_t ws_bytes, void* stream);
size_t lo_bilinear_root_workspace_bytes(int64_t B, int64_t N, int64_t R, int64_t D);
/* rowdot (optional, [B,N]): sum_d U o V of the same rows, i.e. the Diag derivative of an AddedDiag(Root, Diag)
 * operator, produced in the same pass (NULL: not wanted).                                                          */
int lo_bilinear_root_f32(const float* C, const float* U, const float* V, int64_t B, int64_t N, int64_t R, int64_t D,
                         float* out, float* rowdot, void* ws, size_t ws_bytes, void* stream);

/*   kron : dK1 [B,n1,n1] = sum_d U_d K2 V_d^T, dK2 [B,n2,n2] = sum_d U_d^T K1 V_d with U_d, V_d the [n1,n2] views of
 *          the columns (autograd of the Kronecker matvec, kronecker_product_linear_operator.py:34-45)            */
size_t lo_bilinear_kron_workspace_bytes(int64_t B, int64_t n1, int64_t n2, int64_t D);
int lo_bilinear_kron_f32(const float* K1, const float* K2, const float* U, const float* V, int64_t B, int64_t n1,
                         int64_t n2, int64_t D, float* dK1, float* dK2, void* ws, size_t ws_bytes, void* stream);
/* out [B,N,R] += U [B,N,D] T [B,D,R] in one pass over `out` (ABI 15): the N-sized product of the pull-back through the
 * pivoted Cholesky of a root, bar R = G2 (L11^-1 Rm) -- what PivotedCholesky.backward obtains by autograd
 * (functions/_pivoted_cholesky.py:107-147) -- accumulated onto the gradient the operator's bilinear derivative left in
 * `out`.  R in {8, 16, 32}, D <= 32; LO_ERR_UNSUPPORTED otherwise (the caller takes the library product).            */
int lo_root_apply_add_f32(const float* U, const float* T, int64_t B, int64_t N, int64_t D, int64_t R, float* out,
                          void* stream);

/* ---- shifted MINRES: the reference's second iterative solver -------------------------- */
/* Replaces linear_operator.utils.minres.minres (utils/minres.py:10-207; update block :210-282): solutions of
 * (value * K + shift_q I) x_q = rhs for all shifts at once, optional preconditioner (Woodbury descriptor or closure).
 * It is what contour_integral_quad (utils/contour_integral_quad.py:137-144) and sqrt_inv_matmul call.
 *   rhs [B,N,c]; shifts [n_shifts] or [n_shifts, B] (shifts_per_member); x [n_shifts, B, N, c].
 * Stop rule (:178-183): every 10th iteration, mean over shifts / members / columns of ||update|| / ||solution|| <
 * tolerance; the loop body runs at most max_iter + 2 times (:134; max_iter already min'ed with N + 1, :60).        */
typedef struct lo_minres_params {
  int64_t c;
  int32_t n_shifts;
  int32_t max_iter;
  int32_t has_value;          /* 0: value = None (:66-68)                                                          */
  int32_t shifts_per_member;  /* 0: shifts [n_shifts]; 1: shifts [n_shifts, B]                                     */
  float value;
  float tolerance;            /* settings.minres_tolerance                                                          */
  float eps;                  /* 1e-25 (:13)                                                                        */
  float pad;
} lo_minres_params;

typedef struct lo_minres_info {
  int32_t iterations;
  int32_t matvecs;
  int32_t converged;
  float conv;                 /* last evaluated mean relative update norm                                           */
} lo_minres_info;

size_t lo_minres_workspace_bytes(const lo_op_desc* op, const lo_precond_desc* pre, const lo_minres_params* prm);
int lo_minres_f32(const lo_op_desc* op, lo_matvec_cb matvec, void* matvec_user, const lo_precond_desc* pre,
                  lo_matvec_cb precond_cb, void* precond_user, const lo_minres_params* prm, const float* rhs,
                  const float* shifts, float* x, void* ws, size_t ws_bytes, lo_minres_info* info, void* stream);

/* ---- linear_cg in fp64 (linear_operator/utils/linear_cg.py:98-359 with float64 operands) ---------------------- */
/* north_star's path is fp32; this entry exists so that the reference's own fp64 recipes run unmodified (every case of
 * its test/utils/test_linear_cg.py:27-160 builds float64 operands).  Plain streaming formulation, same masking,
 * stopping rule and CG-coefficient tridiagonals as lo_cg_solve_f32.
 *   A         [B, N, N] dense fp64 operator (+ diag [B, N] or NULL), or NULL with (matvec, matvec_user): the closure
 *             is called once per product on [B, N, c] device buffers, must enqueue on `stream`
 *   precond_cb  opaque preconditioner closure or NULL (identity)
 *   rhs, x0 (or NULL), x  [B, N, c];  t_mat [n_tridiag, B, T, T] out, T = max_tridiag_iter, zero-filled by the call
 * SYNCHRONOUS (one control read-back per iteration).  No batch-global stop hook over ranks.                        */
typedef int (*lo_matvec_cb_f64)(void* user, const double* v, double* y, int64_t B, int64_t N, int64_t c, void* stream);
typedef struct lo_cg_params_f64 {
  int64_t c;
  int32_t n_tridiag, max_iter, max_tridiag_iter, floor_max_iter; /* as lo_cg_params */
  double tolerance, eps, stop_updating_after;
} lo_cg_params_f64;
typedef struct lo_cg_info_f64 {
  int32_t iterations, matvecs, tolerance_reached, nan_detected, skipped, last_tridiag_iter; /* as lo_cg_info */
  double mean_residual;
} lo_cg_info_f64;
size_t lo_cg_f64_workspace_bytes(int64_t B, int64_t N, const lo_cg_params_f64* prm);
int lo_cg_solve_f64(const double* A, const double* diag, lo_matvec_cb_f64 matvec, void* matvec_user,
                    lo_matvec_cb_f64 precond_cb, void* precond_user, const lo_cg_params_f64* prm, int64_t B, int64_t N,
                    const double* rhs, const double* x0, double* x, double* t_mat, void* ws, size_t ws_bytes,
                    lo_cg_info_f64* info, void* stream);

/* ---- shifted MINRES in fp64 (linear_operator/utils/minres.py:10-282 with float64 operands) ---------------------- */
/* As lo_cg_solve_f64: the reference's own test/utils/test_minres.py:17-80 builds float64 operands.  Same recurrences
 * and stop test as lo_minres_f32 (every 10th iteration: mean ||update|| / ||solution|| < tolerance).
 *   A / diag / matvec / precond_cb  as lo_cg_solve_f64
 *   rhs [B, N, c];  shifts [Q] (or [Q, B] with shifts_per_member);  x [Q, B, N, c] out (scaled back, zero columns 0) */
typedef struct lo_minres_params_f64 {
  int64_t c;
  int32_t n_shifts, max_iter, has_value, shifts_per_member; /* as lo_minres_params */
  double value, tolerance, eps;
} lo_minres_params_f64;
typedef struct lo_minres_info_f64 {
  int32_t iterations, matvecs, converged, pad;
  double conv;
} lo_minres_info_f64;
size_t lo_minres_f64_workspace_bytes(int64_t B, int64_t N, const lo_minres_params_f64* prm);
int lo_minres_f64(const double* A, const double* diag, lo_matvec_cb_f64 matvec, void* matvec_user,
                  lo_matvec_cb_f64 precond_cb, void* precond_user, const lo_minres_params_f64* prm, int64_t B, int64_t N,
                  const double* rhs, const double* shifts, double* x, void* ws, size_t ws_bytes,
                  lo_minres_info_f64* info, void* stream);

/* lanczos_tridiag (utils/lanczos.py:9-164) with float64 operands: the reference is dtype-generic and its
 * root_decomposition / Lanczos callers may hand it doubles.  Streaming formulation (csrc/lo_lanczos_f64.hip).
 *   A [B,N,N] (+ diag [B,N]) or matvec   the operator, as lo_cg_solve_f64
 *   init_vecs [B,N,P]                     start block (normalised per column inside, :81)
 *   q_mat [max_iter,B,N,P], t_mat [max_iter,max_iter,B,P]   working order, as lo_lanczos_tridiag_f32; the first
 *   *iters_out vectors / rows+columns are the result (:151)
 * Reads two integers back per step (the reference's re-orthogonalisation and stopping tests), so it synchronises.  */
size_t lo_lanczos_f64_workspace_bytes(int64_t B, int64_t N, int64_t P, int32_t max_iter);
int lo_lanczos_tridiag_f64(const double* A, const double* diag, lo_matvec_cb_f64 matvec, void* matvec_user,
                           const double* init_vecs, int64_t B, int64_t N, int64_t P, int32_t max_iter, double tol,
                           double* q_mat, double* t_mat, int32_t* iters_out, void* ws, size_t ws_bytes, void* stream);

/* ---- float64 structured operators (ABI 22; csrc/lo_matvec_f64.hip) -------------------------------------------------
 * y [B, N, c] = A v for a descriptor whose A0 / A1 / d point to DOUBLES (the convention of lo_pivoted_cholesky_f64; the
 * size and layout of lo_op_desc are unchanged, and nothing in the struct records the element type: the caller keeps
 * float64 descriptors away from the fp32 entry points).
 *   kinds     LO_OP_LOWRANK_DIAG, LO_OP_DENSE_DIAG, LO_OP_KRON_DIAG, (ABI 31) LO_OP_KERNEL_DIAG with A0 = X [B, N, D],
 *             A1 = theta [B, D + 1] as doubles, R = D, n2 = the family, and LO_OP_SUM of up to LO_MAX_TERMS of those in
 *             any order (summed left to right, the sum's own diagonal added last); every other kind -- the sum-, Kron-
 *             and gradient-kernel kinds included: LO_ERR_UNSUPPORTED
 *   diagonal  LO_DIAG_NONE / FULL / CONST;  any N, R, n1, n2, c >= 1, 1 <= B <= 65535;  y must not alias v (LO_ERR_BADARG)
 *   kernel    a null A0 / A1, R < 1 or a family outside LO_KERNEL_RBF .. LO_KERNEL_MATERN52: LO_ERR_BADARG;
 *             R > LO_KERNEL_MAX_DIM: LO_ERR_UNSUPPORTED; both, and a workspace that is too small, before any launch of the
 *             call, whatever the term's position in a sum
 * Plain launches, fixed-order sums, no float64 atomics: the same inputs give the same bits, and a member's result does
 * not depend on the batch around it, nor on the alignment of the operands (row chunks, tiles and the thread layout are
 * functions of the member's own shape).  EXCEPTION: for the kernel kind the order of the partial sums follows
 * ko_shape(B, M, N) exactly as in lo_kernel_mv_f32 (few row blocks: the columns j are split over workgroups), so a
 * member's bits may depend on B; two calls on the same inputs still give equal bits.
 *   low-rank   C^T v as per-workgroup partials in the workspace added in chunk order, then a second pass over C
 *   dense      the kernel of lo_cg_solve_f64;  Kronecker: two small-GEMM passes, the [n1, n2, c] intermediate in the
 *              workspace
 * Asynchronous on `stream`.  Replaces the same `_matmul`s as lo_matvec_f32 for float64 operands.                    */
size_t lo_matvec_f64_workspace_bytes(const lo_op_desc* op, int64_t c);
int lo_matvec_f64(const lo_op_desc* op, const double* v, double* y, int64_t c, void* ws, size_t ws_bytes, void* stream);

/* Library-side callbacks for the `matvec` / `precond_cb` arguments of lo_cg_solve_f64, lo_minres_f64 and
 * lo_lanczos_tridiag_f64: the host passes these exported functions themselves with a context struct as `user`, and the
 * solver runs a lowered operator / the Woodbury preconditioner with no call into the host language per product.  The
 * structs and what they point to must stay alive for the solver call; the workspaces belong to the call.
 *   lo_matvec_desc_cb_f64   y = A v by lo_matvec_f64; ws of lo_matvec_f64_workspace_bytes(op, c).  op->B, op->N must equal
 *                           the solver's B, N.
 *   lo_precond_desc_cb_f64  the precondition_closure of added_diag_linear_operator.py:135-140 from the cached pair
 *                           (Q [B, N, k], noise):  z = r / d - Q (Q^T r)  (LO_DIAG_FULL, noise [B, N])
 *                                                  z = (r - Q Q^T r) / sigma  (LO_DIAG_CONST, noise [B])
 *                           -- the low-rank kernels of lo_matvec_f64 with another epilogue; ws of
 *                           lo_precond_f64_workspace_bytes(B, N, k, c).  z must not alias r.                          */
struct lo_f64_op_ctx { /* (plain struct tags, as lo_mask_desc: C callers write `struct lo_f64_op_ctx`) */
  const lo_op_desc* op;
  void* ws;
  size_t ws_bytes;
};
struct lo_f64_precond_ctx {
  const double* Q;     /* [B, N, k] */
  const double* noise; /* [B, N] (LO_DIAG_FULL) or [B] (LO_DIAG_CONST) */
  int32_t diag_mode;
  int32_t k;
  void* ws;
  size_t ws_bytes;
};
int lo_matvec_desc_cb_f64(void* user, const double* v, double* y, int64_t B, int64_t N, int64_t c, void* stream);
int lo_precond_desc_cb_f64(void* user, const double* r, double* z, int64_t B, int64_t N, int64_t c, void* stream);
size_t lo_precond_f64_workspace_bytes(int64_t B, int64_t N, int32_t k, int64_t c);

/* ---- Toeplitz / interpolation building blocks (ABI 16; csrc/lo_ski.hip) ------------------------------------------
 * Symmetric Toeplitz T = toeplitz(t), t [B, M]; interpolation W [B, N, M] stored as idx int64 [B, N, J] and vals fp32
 * [B, N, J] (utils/interpolation.py, utils/toeplitz.py).  Vectors [B, rows, c], c innermost.  Deterministic: the same
 * inputs give bitwise the same outputs (no float atomics; W^T v runs as a segmented gather over a grid-major copy of
 * W built with an integer counting sort, entries of one grid point in ascending (n, j) order).
 *   lo_interp_f32          y [B, N, c] = W u,  u [B, M, c]                               (left_interp)
 *   lo_interp_t_f32        out [B, M, c] = W^T v,  v [B, N, c]                           (left_t_interp)
 *   lo_interp_plan_build   the grid-major copy of W (lo_interp_plan_bytes bytes, device memory the caller keeps) that
 *                          lo_interp_t_planned_f32 and lo_interp_desc.right_plan reuse: W^T v without the per-call build.
 *                          Cost of the build: linear in B N J, plus sum over grid points of count^2 / 64 (the rank sort
 *                          that fixes the order of a grid point's entries, a wave per point): a grid point that
 *                          receives k entries costs k^2 comparisons, so heavily repeated inputs make the build slow.
 *   lo_toeplitz_mv_f32     y [B, M, c] = T u                                             (sym_toeplitz_matmul)
 *   lo_toeplitz_bilinear_f32  g [B, M]: g_k = sum_s u_s^T (dT/dt_k) v_s, u, v [B, M, S]
 *                          (sym_toeplitz_derivative_quadratic_form)
 *   lo_interp_values_grad_f32  g [B, N, J]: g[n, j] = sum_s lv[n, s] R[idx[n, j], s],  lv [B, N, S], R [B, M, S]
 *                          (the gather-dot of InterpolatedLinearOperator._bilinear_derivative)
 * M <= LO_TOEPLITZ_MAX_M for the Toeplitz product and the lag correlation, else LO_ERR_UNSUPPORTED.               */
int lo_interp_f32(const int64_t* idx, const float* vals, int64_t B, int64_t N, int64_t J, int64_t M, const float* u,
                  int64_t c, float* y, void* stream);
size_t lo_interp_t_workspace_bytes(int64_t B, int64_t N, int64_t J, int64_t M);
int lo_interp_t_f32(const int64_t* idx, const float* vals, int64_t B, int64_t N, int64_t J, int64_t M, const float* v,
                    int64_t c, float* out, void* ws, size_t ws_bytes, void* stream);
size_t lo_interp_plan_bytes(int64_t B, int64_t N, int64_t J, int64_t M);
int lo_interp_plan_build(const int64_t* idx, int64_t B, int64_t N, int64_t J, int64_t M, void* plan, size_t plan_bytes,
                         void* stream);
int lo_interp_t_planned_f32(const void* plan, const float* vals, int64_t B, int64_t N, int64_t J, int64_t M,
                            const float* v, int64_t c, float* out, void* stream);
size_t lo_toeplitz_workspace_bytes(int64_t B, int64_t M, int64_t c);
int lo_toeplitz_mv_f32(const float* t, int64_t B, int64_t M, const float* u, int64_t c, float* y, void* ws,
                       size_t ws_bytes, void* stream);
int lo_toeplitz_bilinear_f32(const float* u, const float* v, int64_t B, int64_t M, int64_t S, float* g, void* ws,
                             size_t ws_bytes, void* stream);
int lo_interp_values_grad_f32(const int64_t* idx, int64_t B, int64_t N, int64_t J, int64_t M, const float* lv,
                              const float* R, int64_t S, float* g, void* stream);

/* ---- additive SKI building blocks (ABI 37; csrc/lo_ski_sum.hip) --------------------------------------------------------
 * The two kernels LO_OP_SKI_SUM_DIAG adds to the ones above, over P terms per member (arrays [B, P, N, J], grid
 * member g = b P + p).  Fixed-order sums (j ascending within a term, terms ascending), no float atomics: the same inputs
 * give the same bits; P = 1 gives the bits of lo_interp_f32 / lo_interp_t_planned_f32.  Index entries outside [0, M)
 * contribute nothing.  LO_ERR_BADARG: null pointers, sizes below 1, a diag_mode other than LO_DIAG_* or one without d / v;
 * LO_ERR_UNSUPPORTED: P > LO_SKI_SUM_MAX_TERMS, B P > 65535.                                                               */
/* y [B, N, c] = sum_{p<P} W_p u_p (+ d o v when dd_mode != LO_DIAG_NONE);  idx / vals [B, P, N, J], u [B, P, M, c] */
int lo_interp_sum_f32(const int64_t* idx, const float* vals, int64_t B, int64_t P, int64_t N, int64_t J, int64_t M,
                      const float* u, int64_t c, const float* d, int32_t diag_mode, const float* v, float* y, void* stream);
/* out [B, P, M, c] = W_p^T v for every p from ONE v [B, N, c] (no [P, N, c] copy of v); plan as lo_interp_plan_build(B*P) */
int lo_interp_t_bcast_planned_f32(const void* plan, const float* vals, int64_t B, int64_t P, int64_t N, int64_t J,
                                  int64_t M, const float* v, int64_t c, float* out, void* stream);

/* ---- SKI on a 2-D / 3-D grid (ABI 23; csrc/lo_ski_grid.hip) -------------------------------------------------------
 * The grid product y = (T_1 (x) .. (x) T_D) u of D = ndim in {2, 3} symmetric Toeplitz factors, one axis per pass and no
 * M_k x M_k matrix anywhere (kronecker_product_linear_operator.py:272-284 over toeplitz_linear_operator.py:42-53).
 *   t   [B, M_1 + .. + M_D]: the factors' first columns, concatenated per member;  m [ndim]: HOST array M_1 .. M_D
 *   u   [B, M_1, .., M_D, c] row-major, columns fastest (= [B, M, c] with the grid index g = (g_1 M_2 + g_2) M_3 + g_3)
 *   y   the same shape; must not alias u.  ws: one grid vector (the _workspace_bytes query).
 * Fixed-order sums (ascending along every axis), no float atomics: the same inputs give the same bits.
 * LO_ERR_UNSUPPORTED: ndim outside {2, 3}, an axis beyond LO_SKI_GRID_MAX_AXIS, M beyond LO_SKI_GRID_MAX_M;
 * LO_ERR_BADARG: null pointers, non-positive sizes.  The kind LO_OP_SKI_GRID_DIAG wraps it between W_r^T and W_l. */
size_t lo_toeplitz_kron_workspace_bytes(const int64_t* m, int ndim, int64_t B, int64_t c);
int lo_toeplitz_kron_mv_f32(const float* t, const int64_t* m, int ndim, int64_t B, const float* u, int64_t c, float* y,
                            void* ws, size_t ws_bytes, void* stream);
/* Gradients of sum_s u_s^T (T_1 (x) .. (x) T_D) v_s with respect to the factors' first columns (ABI 24):
 *   g [B, M_1 + .. + M_D], g_k[b, l] = sum_s u_s^T (dK / dt_k[l]) v_s;  t, m as above;  u, v [B, M, S].
 * With W_k = v with every factor but T_k applied, viewed as [lines = B * outer, M_k, inner], inner = (prod_{j > k} M_j) S:
 *   g_k[b, l] = sum_{lines of b} sum_s sum_i (u[i, s] W_k[i + l, s] + [l > 0] u[i + l, s] W_k[i, s]).
 * The partial products are single-axis passes of the grid product, shared between the axes and, the factors being
 * symmetric, applied to u where that saves one (2 passes for D = 2, 4 for D = 3); an axis lag-correlation kernel writes
 * one partial [M_k] per (member, chunk of lines) and a second kernel adds the partials in ascending order.
 * Deterministic (fixed-order sums, no float atomics).  LO_ERR_UNSUPPORTED outside the shape limits of
 * lo_toeplitz_kron_mv_f32; LO_ERR_BADARG: null pointers, non-positive sizes.  ws: the _workspace_bytes query (0: a shape
 * that is not taken).  (sym_toeplitz_derivative_quadratic_form per axis; the reference obtains these by autograd of
 * KroneckerProductLinearOperator._matmul.)                                                                           */
size_t lo_toeplitz_kron_bilinear_workspace_bytes(const int64_t* m, int ndim, int64_t B, int64_t S);
int lo_toeplitz_kron_bilinear_f32(const float* t, const int64_t* m, int ndim, int64_t B, const float* u, const float* v,
                                  int64_t S, float* g, void* ws, size_t ws_bytes, void* stream);

/* ---- eigenbasis apply of a sum of two Kronecker products (ABI 25; csrc/lo_kron_eigsolve.hip) ----------------------------
 * y = scale o ((M1 (x) S2^T) z): with Z_col the [n1, n2] view of a column of z (row index i1 n2 + i2, as everywhere),
 *   Y_col = scale o (M1 (Z_col S2)).    M1 [B, n1, n1], S2 [B, n2, n2], scale [B, n1 n2] or NULL, z, y [B, n1 n2, c].
 * The closed-form solve of A (x) B + C (x) D (sum_kronecker_linear_operator.py:42-66) is two calls,
 *   (P_1^T, P_2, w) and (P_1, P_2^T, NULL),   w = 1 / (lambda_1 (x) lambda_2 + 1),
 * with P_i, lambda_i from the per-factor generalised eigenproblems (set-up is the caller's).
 *   n2 <= LO_KRON_EIG_MAX_SMALL   ONE fused launch for any n1 >= 1 and c <= LO_KRON_EIG_MAX_COLS: Z S2 is formed while the
 *                                 slab of Z is staged to LDS, M1 is streamed once per 8 of the n2 c columns, scale rides in
 *                                 the epilogue; more columns: LO_ERR_UNSUPPORTED (the caller composes)
 *   n2 >  LO_KRON_EIG_MAX_SMALL   S2 transposed into ws, the Kronecker matvec engines of lo_matvec_f32, one scale kernel:
 *                                 every shape the Kronecker matvec takes
 * (LO_KRON_EIG_NO_FUSED in the environment sends every shape to the second route: measurement aid.)
 * Fixed-order sums, no float atomics.  y must not alias z.  LO_ERR_BADARG: null pointers, non-positive sizes.
 * ws: the _workspace_bytes query (0: a shape that is not taken).                                                       */
size_t lo_kron_eig_apply_workspace_bytes(int64_t B, int64_t n1, int64_t n2, int64_t c);
int lo_kron_eig_apply_f32(const float* M1, const float* S2, const float* scale, const float* z, float* y, int64_t B,
                          int64_t n1, int64_t n2, int64_t c, void* ws, size_t ws_bytes, void* stream);

/* ---- Hadamard product of two roots (ABI 17; csrc/lo_hadamard.hip) -------------------------------------------------
 * K = (F F^T) o (G G^T), F [B, N, p], G [B, N, q], p, q <= LO_HADAMARD_MAX_RANK; U, V [B, N, S], S columns innermost.
 *   lo_hadamard_bilinear_f32   dF [B, N, p], dG [B, N, q]: the derivatives of sum_s u_s^T K v_s with respect to F and G
 *                              (mul_linear_operator.py:91-126 summed over both roots):
 *                                dF[n] = sum_s u[n,s] M^v_s G[n] + v[n,s] M^u_s G[n],  M^v_s = F^T diag(v_s) G
 *                                dG[n] = sum_s u[n,s] M^v_s^T F[n] + v[n,s] M^u_s^T F[n]
 * Deterministic (fixed-order sums, no float atomics).  The workspace comes from the _workspace_bytes query (0: shapes
 * outside what the kernels take).                                                                                      */
size_t lo_hadamard_bilinear_workspace_bytes(int64_t B, int64_t N, int64_t p, int64_t q, int64_t S);
int lo_hadamard_bilinear_f32(const float* F, const float* G, const float* U, const float* V, int64_t B, int64_t N,
                             int64_t p, int64_t q, int64_t S, float* dF, float* dG, void* ws, size_t ws_bytes,
                             void* stream);

/* ---- matrix-free kernel operator (ABI 26, 27; csrc/lo_kernel_op.hip) -------------------------------------------------
 * K(x1, x2)_ij = theta[D] g(r_ij), r_ij^2 = sum_d (theta[d] (x1[i, d] - x2[j, d]))^2 by direct differences, g one of
 * LO_KERNEL_*; x1 [B, M, D], x2 [B, N, D], theta [B, D + 1] = D inverse lengthscales, then outputscale^2.  K is never in
 * memory: a workgroup owns 256 rows (scaled once, kept in registers with their accumulators) and streams tiles of the
 * scaled x2 and of v through LDS (kernel_linear_operator.py:379-383 evaluates covar_func densely before the product).
 *   lo_kernel_mv_f32        y [B, M, c] = K v for v [B, N, c]; + d o v (d, diag_mode as in lo_op_desc) only when M == N
 *                           and diag_mode != LO_DIAG_NONE.  The kind LO_OP_KERNEL_DIAG runs the same kernel with x1 = x2.
 *                           Few rows (B M small): the columns j are split over workgroups, the partials go to ws and a
 *                           second kernel adds them in ascending order.
 *   lo_kernel_bilinear_f32  g_theta [B, D + 1] = d / d theta of sum_ij (sum_s U[i, s] V[j, s]) K_ij, U [B, M, t],
 *                           V [B, N, t]: for d < D  sum_ij W_ij theta[D] (g'(r) / r) (theta[d] delta_d)^2 / theta[d], last
 *                           entry sum_ij W_ij g(r).  A pair with r = 0 adds nothing to the first D entries for every
 *                           family (no division by r).  One partial per workgroup, added in ascending order.
 *   lo_kernel_points_grad_f32 (ABI 27)  g_x1 [B, M, D] = d / d x1 of the same sum with x2 held fixed:
 *                           g_x1[i, d] = theta[D] theta[d] sum_j W_ij (g'(r_ij) / r_ij) theta[d] (x1[i, d] - x2[j, d]).
 *                           A thread owns a row i and sums over j in the product's order (tile, then running); a pair
 *                           with r = 0 adds nothing.  The x2 side is the same call with the roles swapped (x1 <-> x2,
 *                           U <-> V, M <-> N); when x1 and x2 are one tensor the caller adds the two.  Few rows: the
 *                           columns j are split as in the product, partials [js, B, M, D] in ws, added in ascending order.
 * Fixed-order sums, no float atomics: the same inputs give the same bits.  LO_ERR_BADARG: null pointers, non-positive
 * sizes, an unknown family; LO_ERR_UNSUPPORTED: D > LO_KERNEL_MAX_DIM; LO_ERR_WORKSPACE (before any launch): ws smaller
 * than the _workspace_bytes query (0: arguments that are not taken).  y must not alias v.                               */
size_t lo_kernel_mv_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t c);
int lo_kernel_mv_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B, int64_t M,
                     int64_t N, int64_t D, const float* v, int64_t c, const float* d, int32_t diag_mode, float* y,
                     void* ws, size_t ws_bytes, void* stream);
size_t lo_kernel_bilinear_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t);
int lo_kernel_bilinear_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B, int64_t M,
                           int64_t N, int64_t D, const float* U, const float* V, int64_t t, float* g_theta, void* ws,
                           size_t ws_bytes, void* stream);
size_t lo_kernel_points_grad_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t);
int lo_kernel_points_grad_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B, int64_t M,
                              int64_t N, int64_t D, const float* U, const float* V, int64_t t, float* g_x1, void* ws,
                              size_t ws_bytes, void* stream);

/* ---- the same operator in float64 (ABI 31; csrc/lo_kernel_op_f64.hip) --------------------------------------------------
 * The three entry points above with `double` in place of `float`: same formulas, same argument meanings, same error
 * codes in the same order of precedence (lo_kernel_mv_f64 checks the aliasing it forbids: y == v is LO_ERR_BADARG),
 * LO_ERR_WORKSPACE before any launch, sizers of their own.  K is never in memory.  The sweeps keep the structure of the fp32
 * kernels (256 rows per workgroup, x2 scaled while staged in LDS tiles of 128, r^2 by direct differences in ascending k, a
 * tile's sum on its own and then added to the running one, the column split of few-row shapes with an ascending reduce);
 * exp and sqrt are the device math library's, there is no hardware double-precision exponential.  The Matern families
 * take r = sqrt(min(r^2, 1e300)), so every family stays finite (and is 0) when r^2 overflows.  A pair with r^2 <= 1e-30
 * adds nothing to the Matern-1/2 lengthscale and points sums; g'(r) / r of the other families is finite at 0.
 * Fixed-order sums, no atomics: the same inputs give the same bits.  The kind LO_OP_KERNEL_DIAG of lo_matvec_f64 runs
 * lo_kernel_mv_f64's kernel with x1 = x2.                                                                               */
size_t lo_kernel_mv_f64_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t c);
int lo_kernel_mv_f64(const double* x1, const double* x2, const double* theta, int32_t family, int64_t B, int64_t M,
                     int64_t N, int64_t D, const double* v, int64_t c, const double* d, int32_t diag_mode, double* y,
                     void* ws, size_t ws_bytes, void* stream);
size_t lo_kernel_bilinear_f64_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t);
int lo_kernel_bilinear_f64(const double* x1, const double* x2, const double* theta, int32_t family, int64_t B, int64_t M,
                           int64_t N, int64_t D, const double* U, const double* V, int64_t t, double* g_theta, void* ws,
                           size_t ws_bytes, void* stream);
size_t lo_kernel_points_grad_f64_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t);
int lo_kernel_points_grad_f64(const double* x1, const double* x2, const double* theta, int32_t family, int64_t B,
                              int64_t M, int64_t N, int64_t D, const double* U, const double* V, int64_t t, double* g_x1,
                              void* ws, size_t ws_bytes, void* stream);

/* ---- sums of matrix-free kernel operators over the same points (ABI 28; csrc/lo_kernel_sum.hip) ------------------------
 * K_ij = sum_t theta[t][D] g_{f_t}(r_t,ij), r_t,ij^2 = sum_d (theta[t][d] (x1[i, d] - x2[j, d]))^2 for T terms,
 * 1 <= T <= LO_KERNEL_MAX_TERMS; theta [B, T, D + 1], `families` a HOST array of T codes LO_KERNEL_* (terms may mix
 * families).  One pass over the pairs for all terms: the tile of x2 is staged scaled once per term, the tile of v once;
 * the T kernel values of a pair are added before its column FMAs run.  The term loop runs outside sub-tiles of 8 pairs,
 * so a term's family is switched on once per 8 pairs.  Launch shape, column splits and the sums' order as in the
 * single-term kernels above; every argument and error code as there, plus LO_ERR_BADARG for T outside the range or a
 * null `families`.
 *   lo_kernel_sum_mv_f32           y [B, M, c] = K v (+ d o v when M == N), the kind LO_OP_KERNEL_SUM_DIAG with x1 = x2.
 *                                  Fused for T > 1 and c > 4; narrower right-hand sides run the single-term kernel once
 *                                  per term inside the call, added in term order (measured faster: DESIGN.md 6m); the
 *                                  workspace then holds one more [B, M, c] vector
 *   lo_kernel_sum_bilinear_f32     g_theta [B, T, D + 1]: every term's d / d theta of sum_ij W_ij K_ij, W_ij formed once per
 *                                  pair; one sweep (two when 16 < D and T > 2: a thread holds the running sums of 2 terms)
 *   lo_kernel_sum_points_grad_f32  g_x1 [B, M, D], the gradient of the points summed over the terms, one sweep           */
size_t lo_kernel_sum_mv_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, int64_t c);
int lo_kernel_sum_mv_f32(const float* x1, const float* x2, const float* theta, const int32_t* families, int64_t T,
                         int64_t B, int64_t M, int64_t N, int64_t D, const float* v, int64_t c, const float* d,
                         int32_t diag_mode, float* y, void* ws, size_t ws_bytes, void* stream);
size_t lo_kernel_sum_bilinear_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, int64_t t);
int lo_kernel_sum_bilinear_f32(const float* x1, const float* x2, const float* theta, const int32_t* families, int64_t T,
                               int64_t B, int64_t M, int64_t N, int64_t D, const float* U, const float* V, int64_t t,
                               float* g_theta, void* ws, size_t ws_bytes, void* stream);
size_t lo_kernel_sum_points_grad_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, int64_t t);
int lo_kernel_sum_points_grad_f32(const float* x1, const float* x2, const float* theta, const int32_t* families, int64_t T,
                                  int64_t B, int64_t M, int64_t N, int64_t D, const float* U, const float* V, int64_t t,
                                  float* g_x1, void* ws, size_t ws_bytes, void* stream);

/* ---- matrix-free multitask operator Kernel(X, X) (x) Bt (ABI 29; csrc/lo_kernel_kron.hip) -------------------------------
 * y [B, n T, c] = (K(X, X) (x) Bt) v (+ d o v), row and column index i T + t:
 *   y[(i,t), col] = sum_j theta[D] g(r_ij) sum_s Bt[t,s] v[(j,s), col] + d[(i,t)] v[(i,t), col]
 * x [B, n, D], theta [B, D + 1] and `family` as for lo_kernel_mv_f32, task = Bt [B, T, T] (not required symmetric),
 * v [B, n T, c], d per diag_mode over the n T rows.  One sweep of the pairs carries up to 32 of the T c "wide" columns;
 * Bt is applied while the tile of v is staged.  Launch shape, splits of the points j and the order of the sums as in
 * lo_kernel_mv_f32: fixed-order sums, no atomics, two calls give equal bits.
 * LO_ERR_BADARG: a null pointer, a non-positive size, family outside 0 .. 3, T < 1, an unknown diag_mode or one without d;
 * LO_ERR_UNSUPPORTED: D > LO_KERNEL_MAX_DIM, T > LO_KERNEL_KRON_MAX_TASKS; LO_ERR_WORKSPACE before any launch.           */
size_t lo_kernel_kron_mv_workspace_bytes(int64_t B, int64_t n, int64_t D, int64_t T, int64_t c);
int lo_kernel_kron_mv_f32(const float* x, const float* theta, const float* task, int32_t family, int64_t B, int64_t n,
                          int64_t D, int64_t T, const float* v, int64_t c, const float* d, int32_t diag_mode, float* y,
                          void* ws, size_t ws_bytes, void* stream);

/* ---- matrix-free LMC operator sum_q Kernel_q(X, X) (x) B_q (ABI 38; csrc/lo_kernel_lmc.hip) ----------------------------
 * y [B, n T, c] = (sum_{q < Q} K_q(X, X) (x) B_q) v (+ d o v), row and column index i T + t:
 *   y[(i,t), col] = sum_q theta_q[D] sum_j g_{f_q}(r_q,ij) sum_s B_q[t,s] v[(j,s), col] + d[(i,t)] v[(i,t), col]
 * x [B, n, D], theta [B, Q, D + 1] as for lo_kernel_sum_mv_f32, task = Bt [B, Q, T, T] (not required symmetric),
 * `families` = the Q codes LO_KERNEL_* packed four bits per term, term 0 lowest (the low 16 bits of the kind's n2),
 * v [B, n T, c], d per diag_mode over the n T rows.  One pass over the pairs forms all Q kernel values; every B_q v is
 * formed while the tile of v is staged; a sweep carries up to 16 of the T c "wide" columns (8 for Q > 2).  Launch shape,
 * splits of the points j and the order of the sums as in lo_kernel_kron_mv_f32: fixed-order sums, no atomics, two calls
 * give equal bits.  The sizer: 256 bytes, plus js copies of [B, n T, c] floats when the points are split; 0 for what the
 * entry point refuses.
 * LO_ERR_BADARG: a null pointer, a non-positive size, Q < 1, T < 1, a family code outside 0 .. 3 or set beyond the Q
 * terms, an unknown diag_mode or one without d; LO_ERR_UNSUPPORTED: Q > LO_KERNEL_MAX_TERMS, T >
 * LO_KERNEL_KRON_MAX_TASKS, D > LO_KERNEL_MAX_DIM, sizes beyond the 32-bit limits; LO_ERR_WORKSPACE before any launch.  */
size_t lo_kernel_lmc_mv_workspace_bytes(int64_t B, int64_t n, int64_t D, int64_t Q, int64_t T, int64_t c);
int lo_kernel_lmc_mv_f32(const float* x, const float* theta, const float* task, int32_t families, int64_t B, int64_t n,
                         int64_t D, int64_t Q, int64_t T, const float* v, int64_t c, const float* d, int32_t diag_mode,
                         float* y, void* ws, size_t ws_bytes, void* stream);

/* ---- matrix-free derivative GP: the RBF gradient kernel (ABI 30; csrc/lo_kernel_grad.hip) ------------------------------
 * y [B, M (D + 1), c] = K(x1, x2) v (+ d o v) for the block matrix of LO_OP_KERNEL_GRAD_DIAG, rows i (D + 1) + a over
 * the M points of x1 [B, M, D], columns j (D + 1) + b over the N points of x2 [B, N, D] (M, N count POINTS; rectangular
 * x1 != x2 is the prediction case), theta [B, D + 1] and `family` as for lo_kernel_mv_f32, v [B, N (D + 1), c].  With
 * w[j,0] = v[j,0], w[j,b] = t_b v[j,b] (applied while the tile of v is staged) and s = w[j,0] + sum_b u_b w[j,b]:
 *   y[i,0] = os2 sum_j e s,   y[i,a] = os2 t_a sum_j e (w[j,a] - u_a s)
 * so a pair costs D FMAs for s and 2 D + 1 for the accumulators per column; nothing of size D^2 is formed.  d per
 * diag_mode over the M (D + 1) rows, allowed only when M == N.  Launch shape, splits of the points j and the order of
 * the sums as in lo_kernel_mv_f32: fixed-order sums, no atomics, two calls give equal bits.
 * lo_kernel_grad_bilinear_f32: g_theta [B, D + 1] = d / d theta of S = sum_s U[:, s]^T K(x1, x2) V[:, s], U [B, M (D + 1),
 * t], V [B, N (D + 1), t], in the meaning lo_kernel_bilinear_f32 gives its output (inverse lengthscales, then os2).
 * LO_ERR_BADARG: a null pointer, a non-positive size, family outside 0 .. 3, an unknown diag_mode, one without d or one
 * with M != N; LO_ERR_UNSUPPORTED: D > LO_KERNEL_GRAD_MAX_DIM, a family other than LO_KERNEL_RBF; LO_ERR_WORKSPACE before
 * any launch.                                                                                                          */
size_t lo_kernel_grad_mv_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t c);
int lo_kernel_grad_mv_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B, int64_t M,
                          int64_t N, int64_t D, const float* v, int64_t c, const float* d, int32_t diag_mode, float* y,
                          void* ws, size_t ws_bytes, void* stream);
size_t lo_kernel_grad_bilinear_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t);
int lo_kernel_grad_bilinear_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B, int64_t M,
                                int64_t N, int64_t D, const float* U, const float* V, int64_t t, float* g_theta, void* ws,
                                size_t ws_bytes, void* stream);

/* ---- matrix-free task-indexed multitask operator (ABI 34; csrc/lo_kernel_task.hip) --------------------------------------
 * K(x1, x2)_ij = theta[D] g(r_ij) Bt[t_i, t_j] for x1 [B, M, D + 1], x2 [B, N, D + 1]: columns 0 .. D - 1 the coordinates,
 * column D the task id (rounded to nearest, clamped into [0, T - 1]); theta [B, D + 1] and `family` as for
 * lo_kernel_mv_f32, task = Bt [B, T, T] (not required symmetric).  D counts the COORDINATES; rectangular x1 != x2 is the
 * prediction case.  The sweeps are those of lo_kernel_mv_f32 / lo_kernel_bilinear_f32 / lo_kernel_points_grad_f32 (256
 * rows per workgroup, x2 scaled while staged in LDS tiles of 128 together with its task ids, r^2 by direct differences,
 * a tile's sums on their own and then added to the running ones, the column split of few-row shapes with an ascending
 * reduce); Bt sits in LDS transposed and a pair reads one word of it.  Fixed-order sums, no atomics: two calls give
 * equal bits.
 *   lo_kernel_task_mv_f32           y [B, M, c] = K(x1, x2) v (+ d o v when M == N), v [B, N, c], d per diag_mode; the kind
 *                                   LO_OP_KERNEL_TASK_DIAG with x1 = x2
 *   lo_kernel_task_bilinear_f32     for W_ij = sum_s U[i, s] V[j, s], U [B, M, t], V [B, N, t]: g_theta [B, D + 1] =
 *                                   d / d theta of sum_ij W_ij K_ij in the meaning lo_kernel_bilinear_f32 gives it, and
 *                                   g_task [B, T, T], g_task[a, b] = theta[D] sum_{i: t_i = a} sum_{j: t_j = b} W_ij g(r_ij)
 *                                   = d / d Bt[a, b] (not symmetrised; exact zeros for a task without a point)
 *   lo_kernel_task_points_grad_f32  g_x1 [B, M, D + 1] = d / d x1 of the same sum, the task column written as 0.  The x2
 *                                   side is the same call with x1 / x2 and U / V swapped and Bt transposed by the caller
 * LO_ERR_BADARG: a null pointer, a non-positive size, family outside 0 .. 3, T < 1, an unknown diag_mode or (M == N) one
 * without d; LO_ERR_UNSUPPORTED: D + 1 > LO_KERNEL_MAX_DIM, T > LO_KERNEL_TASK_MAX_TASKS; LO_ERR_WORKSPACE before any
 * launch.  The sizers return 0 for arguments the call would refuse.                                                    */
size_t lo_kernel_task_mv_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, int64_t c);
int lo_kernel_task_mv_f32(const float* x1, const float* x2, const float* theta, const float* task, int32_t family,
                          int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, const float* v, int64_t c, const float* d,
                          int32_t diag_mode, float* y, void* ws, size_t ws_bytes, void* stream);
size_t lo_kernel_task_bilinear_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, int64_t t);
int lo_kernel_task_bilinear_f32(const float* x1, const float* x2, const float* theta, const float* task, int32_t family,
                                int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, const float* U, const float* V,
                                int64_t t, float* g_theta, float* g_task, void* ws, size_t ws_bytes, void* stream);
size_t lo_kernel_task_points_grad_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, int64_t t);
int lo_kernel_task_points_grad_f32(const float* x1, const float* x2, const float* theta, const float* task, int32_t family,
                                   int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, const float* U, const float* V,
                                   int64_t t, float* g_x1, void* ws, size_t ws_bytes, void* stream);

/* ---- matrix-free kernels with a shape parameter: rational quadratic and periodic (ABI 39; csrc/lo_kernel_param.hip) ----
 * K(x1, x2)_ij = theta[D] g(x1_i, x2_j) for x1 [B, M, D], x2 [B, N, D], `family` LO_KERNEL_RQ or LO_KERNEL_PERIODIC and
 * theta [B, 2 D + 2] as LO_OP_KERNEL_PARAM_DIAG lays it out (t = inverse lengthscales, os2, alpha, nu = inverse periods):
 *   RQ        q = r^2 / (2 alpha), r^2 = sum_k (t_k x1_i[k] - t_k x2_j[k])^2,  g = (1 + q)^(-alpha)
 *   PERIODIC  phi_k = nu_k x1_i[k] - nu_k x2_j[k],  g = exp(-2 sum_k (t_k sin(pi phi_k))^2)
 * The points are scaled first and then differenced.  The sweeps are those of lo_kernel_mv_f32 / lo_kernel_bilinear_f32 /
 * lo_kernel_points_grad_f32 (256 rows per workgroup, x2 scaled while staged in LDS tiles of 128, a tile's sums on their own
 * and then added to the running ones, the column split of few-row shapes with an ascending reduce).  Fixed-order sums, no
 * atomics: two calls give equal bits.  Rectangular x1 != x2 is the prediction case.
 *   lo_kernel_param_mv_f32           y [B, M, c] = K(x1, x2) v (+ d o v when M == N), v [B, N, c], d per diag_mode; the kind
 *                                    LO_OP_KERNEL_PARAM_DIAG with x1 = x2
 *   lo_kernel_param_bilinear_f32     for W_ij = sum_s U[i, s] V[j, s], U [B, M, t], V [B, N, t]: g_theta [B, 2 D + 2] =
 *                                    d / d theta of sum_ij W_ij K_ij for every entry of theta; the entries the family does
 *                                    not read (RQ: the inverse periods; PERIODIC: alpha) are written as 0
 *   lo_kernel_param_points_grad_f32  g_x1 [B, M, D] = d / d x1 of the same sum, x2 held fixed.  The x2 side is the same
 *                                    call with x1 / x2 and U / V swapped
 * LO_ERR_BADARG: a null pointer, a size < 1, a family other than 16 / 17, an unknown diag_mode, (M == N) a mode without
 * d, (M != N) any mode but LO_DIAG_NONE; LO_ERR_UNSUPPORTED: D > LO_KERNEL_PARAM_MAX_DIM, B > 65535, M or N >
 * 0x7ffffe00, c or t > 0x7fffffff; LO_ERR_WORKSPACE: a short workspace.  In this order, all before any launch.  The
 * sizers return 0 for arguments the call would refuse.                                                                */
size_t lo_kernel_param_mv_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t c);
int lo_kernel_param_mv_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B, int64_t M,
                           int64_t N, int64_t D, const float* v, int64_t c, const float* d, int32_t diag_mode, float* y,
                           void* ws, size_t ws_bytes, void* stream);
size_t lo_kernel_param_bilinear_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t);
int lo_kernel_param_bilinear_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B,
                                 int64_t M, int64_t N, int64_t D, const float* U, const float* V, int64_t t,
                                 float* g_theta, void* ws, size_t ws_bytes, void* stream);
size_t lo_kernel_param_points_grad_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t);
int lo_kernel_param_points_grad_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B,
                                    int64_t M, int64_t N, int64_t D, const float* U, const float* V, int64_t t,
                                    float* g_x1, void* ws, size_t ws_bytes, void* stream);

/* ---- matrix-free spectral mixture kernel (ABI 40; csrc/lo_kernel_sm.hip) -------------------------------------------------
 * K(x1, x2)_ij = sum_{q < Q} w_q E_q prod_k cos(2 pi mu_qk tau_k), E_q = exp(-2 pi^2 sum_k (sigma_qk tau_k)^2), tau = x1_i -
 * x2_j, for x1 [B, M, D], x2 [B, N, D] and theta [B, Q, 2 D + 1] as LO_OP_KERNEL_SM_DIAG lays it out.  The points are
 * differenced FIRST and then multiplied by mu or sigma (the phase error is |mu tau| eps, not |mu x| eps); |tau| is used
 * throughout, so K(x, y) and K(y, x) have equal bits; the cosine is taken in revolutions after fract.  The sweeps are those
 * of lo_kernel_param_*: 256 rows per workgroup, x2 staged in LDS tiles of 128, a tile's sums on their own and then added
 * to the running ones, the column split of few-row shapes with an ascending reduce.  Fixed-order sums, no atomics: two
 * calls give equal bits.  Rectangular x1 != x2 is the prediction case.
 *   lo_kernel_sm_mv_f32           y [B, M, c] = K(x1, x2) v (+ d o v when M == N), v [B, N, c], d per diag_mode; the kind
 *                                 LO_OP_KERNEL_SM_DIAG with x1 = x2
 *   lo_kernel_sm_bilinear_f32     for W_ij = sum_s U[i, s] V[j, s], U [B, M, t], V [B, N, t]: g_theta [B, Q, 2 D + 1] =
 *                                 d / d theta of sum_ij W_ij K_ij, in theta's own layout.  With c_k, s_k the cosine and sine
 *                                 of 2 pi mu_qk tau_k: d/dw_q = E_q prod c, d/dsigma_qk = -4 pi^2 sigma_qk tau_k^2 w_q E_q
 *                                 prod c, d/dmu_qk = -2 pi tau_k s_k w_q E_q prod_{l != k} c_l (no division by a cosine)
 *   lo_kernel_sm_points_grad_f32  g_x1 [B, M, D] = d / d x1 of the same sum, x2 held fixed.  The x2 side is the same call
 *                                 with x1 / x2 and U / V swapped
 * Q stands where `family` stands in lo_kernel_param_*; the sizers take it as well.
 * LO_ERR_BADARG: a null pointer, a size < 1, Q < 1, an unknown diag_mode, (M == N) a mode without d, (M != N) any mode but
 * LO_DIAG_NONE; LO_ERR_UNSUPPORTED: D > LO_KERNEL_SM_MAX_DIM, Q > LO_KERNEL_SM_MAX_MIX, B > 65535, M or N > 0x7ffffe00,
 * c or t > 0x7fffffff; LO_ERR_WORKSPACE: a short workspace.  In this order, all before any launch.  The sizers return 0
 * for arguments the call would refuse.                                                                                */
size_t lo_kernel_sm_mv_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t Q, int64_t c);
int lo_kernel_sm_mv_f32(const float* x1, const float* x2, const float* theta, int32_t Q, int64_t B, int64_t M, int64_t N,
                        int64_t D, const float* v, int64_t c, const float* d, int32_t diag_mode, float* y, void* ws,
                        size_t ws_bytes, void* stream);
size_t lo_kernel_sm_bilinear_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t Q, int64_t t);
int lo_kernel_sm_bilinear_f32(const float* x1, const float* x2, const float* theta, int32_t Q, int64_t B, int64_t M,
                              int64_t N, int64_t D, const float* U, const float* V, int64_t t, float* g_theta, void* ws,
                              size_t ws_bytes, void* stream);
size_t lo_kernel_sm_points_grad_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t Q, int64_t t);
int lo_kernel_sm_points_grad_f32(const float* x1, const float* x2, const float* theta, int32_t Q, int64_t B, int64_t M,
                                 int64_t N, int64_t D, const float* U, const float* V, int64_t t, float* g_x1, void* ws,
                                 size_t ws_bytes, void* stream);

/* ---- exact small-N path: batched Cholesky and triangular solves (ABI 18; csrc/lo_chol.hip) -------------------------
 * fp32, contiguous row-major, N <= 1024 (larger: LO_ERR_UNSUPPORTED), stream-ordered; fixed-order sums, no atomics: a
 * member's result does not depend on the batch around it and repeats bit for bit.
 *   lo_cholesky_f32        A [B, N, N] (lower triangle read) -> L [B, N, N] with A = L L^T, strict upper triangle
 *                          zeroed; info [B] int32: 0, or the 1-based order of the first leading minor whose pivot is
 *                          not > 0 (NaN included; that member's L is unspecified, the others are untouched);
 *                          logdet [B] double = 2 sum log L_ii, or NULL.
 *   lo_tri_solve_f32       out [B, N, c] = M^-1 rhs, M = T or T^T (transpose) of the lower (upper = 0: the lower
 *                          triangle of T is read) or upper factor T [B, N, N]; sumsq [B, c] = sum_i out_ic^2, or NULL.
 *   lo_cholesky_solve_f32  out = (T T^T)^-1 rhs for a lower factor, (T^T T)^-1 rhs for an upper one, one launch.
 * out may alias rhs.                                                                                                  */
size_t lo_cholesky_workspace_bytes(int64_t B, int64_t N);
int lo_cholesky_f32(const float* A, float* L, int32_t* info, double* logdet, int64_t B, int64_t N, void* ws,
                    size_t ws_bytes, void* stream);
int lo_tri_solve_f32(const float* T, const float* rhs, float* out, float* sumsq, int64_t B, int64_t N, int64_t c,
                     int32_t upper, int32_t transpose, void* stream);
int lo_cholesky_solve_f32(const float* T, const float* rhs, float* out, int64_t B, int64_t N, int64_t c, int32_t upper,
                          void* stream);

/* ---- the same path in fp64 (ABI 33; csrc/lo_chol_f64.hip) ------------------------------------------------------------
 * Argument order, refusals, info / logdet / sumsq semantics and determinism as the fp32 calls above; every operand and
 * every sum is float64 (sumsq included), the panel update runs on v_mfma_f64_16x16x4_f64.  N <= 1024; the sizer returns 0
 * for a shape the factorisation refuses.  out may alias rhs.                                                         */
size_t lo_cholesky_f64_workspace_bytes(int64_t B, int64_t N);
int lo_cholesky_f64(const double* A, double* L, int32_t* info, double* logdet, int64_t B, int64_t N, void* ws,
                    size_t ws_bytes, void* stream);
int lo_tri_solve_f64(const double* T, const double* rhs, double* out, double* sumsq, int64_t B, int64_t N, int64_t c,
                     int32_t upper, int32_t transpose, void* stream);
int lo_cholesky_solve_f64(const double* T, const double* rhs, double* out, int64_t B, int64_t N, int64_t c,
                          int32_t upper, void* stream);

/* ---- batched symmetric eigendecomposition in fp64 (ABI 36; csrc/lo_eigh_f64.hip) ---------------------------------------
 * A [B, N, N] contiguous row-major, ONLY THE LOWER TRIANGLE IS READ (the default UPLO of torch.linalg.eigh); A is not
 * modified.  evals [B, N] ascending; evecs [B, N, N] row-major, column j the unit eigenvector of evals[j]; with
 * want_vectors = 0 evecs may be NULL and no vector work is done (the eigenvalues are the same bits either way).
 * info [B] int32: 0, or > 0 when the member's input holds a non-finite value (1) or its iteration did not converge
 * within 30 N sweeps (2); such a member's evals (and evecs) are filled with NaN on the device, the other members are
 * untouched.  One workgroup per member: Householder tridiagonalisation, implicit-shift QL, back-transformation; the
 * member is scaled by a power of two first.  Stream-ordered, fixed-order sums, no atomics: a member's result does not
 * depend on the batch around it and repeats bit for bit.
 * Before any launch: LO_ERR_BADARG for a null A / evals / info, want_vectors with a null evecs, N < 1, B < 0;
 * LO_ERR_UNSUPPORTED for N > LO_EIGH_MAX_N; LO_ERR_WORKSPACE for a short or null workspace; B == 0 is a success that
 * launches nothing.  The sizer returns 0 for what the call refuses.                                                   */
#define LO_EIGH_MAX_N 1024
size_t lo_eigh_f64_workspace_bytes(int64_t B, int64_t N, int32_t want_vectors);
int lo_eigh_f64(const double* A, double* evals, double* evecs, int32_t* info, int64_t B, int64_t N, int32_t want_vectors,
                void* ws, size_t ws_bytes, void* stream);

/* ---- masked operators (ABI 21; csrc/lo_masked.hip) ---------------------------------------------------------------------
 * The kind LO_OP_MASKED is served by lo_matvec_f32 and the solvers above.  lo_mask_expand_f32 is its first step alone:
 * u [B, N0, c] = S^T v for v [B, M, c] (zero rows where the mask is false), one coalesced write of u; idx as in
 * lo_mask_desc.  The operator's derivative expands both vector blocks with it before the base's own contraction.   */
size_t lo_mask_expand_workspace_bytes(int64_t N0);
int lo_mask_expand_f32(const int64_t* idx, int64_t M, int64_t N0, const float* v, float* u, int64_t B, int64_t c,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- block operators over a batch of members (ABI 19; csrc/lo_block.hip) ---------------------------------------------
 * `base` describes B = G * T members of size n x n, the block index fastest (member g * T + t); kind LO_OP_DENSE_DIAG
 * or LO_OP_LOWRANK_DIAG with any diagonal mode (the + d o v term serves Block(AddedDiag(base, Diag))); other kinds
 * return LO_ERR_UNSUPPORTED (the caller composes the product from the base operator's own), B % T != 0 LO_ERR_BADARG.
 * The vectors are read and written in the layout of the block operator, c columns innermost, any c, n, T >= 1:
 *   LO_BLOCK_DIAG         BlockDiagLinearOperator: the plain batched product (lo_matvec_f32 of the same arguments)
 *   LO_BLOCK_INTERLEAVED  BlockInterleavedLinearOperator: no transposed copy of the vectors is made
 *   LO_BLOCK_SUM          SumBatchLinearOperator: the sum over t runs inside the workgroup that owns the output rows,
 *                         no [T, n, c] intermediate
 * Plain launches, fixed-order sums, no float atomics: results repeat bit for bit.  y must not alias v.                 */
#define LO_BLOCK_DIAG 0        /* v, y: [G, T*n, c], row t*n + i belongs to block t       */
#define LO_BLOCK_INTERLEAVED 1 /* v, y: [G, n*T, c], row i*T + t belongs to block t       */
#define LO_BLOCK_SUM 2         /* v, y: [G, n, c];  y = sum_t A_{g,t} v_g                 */
size_t lo_block_mv_workspace_bytes(const lo_op_desc* base, int32_t layout, int64_t T, int64_t c);
int lo_block_mv_f32(const lo_op_desc* base, int32_t layout, int64_t T, const float* v, float* y, int64_t c,
                    void* ws, size_t ws_bytes, void* stream);

/* ---- measurement aid (no reference counterpart) ------------------------------------------------ */
/* Opt-in HIP-event timing of every kernel launch of the library, recorded on the launch stream.
 * lo_prof_report writes "name count total_ms" lines into buf (returns the byte count) and resets.
 * bench.py uses it for the live per-kernel duration behind its roofline line.                     */
int lo_prof_enable(int on);
int lo_prof_report(char* buf, size_t buflen);
/* a = b + s c over n floats (n % 4 == 0): the achievable HBM rate of the box (3 x 4 n bytes per launch), reported by
 * bench.py beside the 8 TB/s spec peak; lo_hbm_copy_f32: a = b (2 x 4 n bytes), the figure the MI355X guide quotes as
 * "achievable" (6.29 TB/s).  Grid sized to the arrays, four 16-byte requests in flight per thread, non-temporal.     */
int lo_hbm_triad_f32(float* a, const float* b, const float* c, float s, size_t n, void* stream);
int lo_hbm_copy_f32(float* a, const float* b, size_t n, void* stream);
/* sweep aid for tools/mb_stream.py: mode 0 triad / 1 copy / 2 read-only; unroll 1, 2, 4, 8; nt 0 / 1               */
int lo_hbm_stream_dev(int mode, int unroll, int nt, float* a, const float* b, const float* c, float s, size_t n,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LO_AMD_H */
