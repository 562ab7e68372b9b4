// lo_internal.h -- shared declarations of liblo_amd's translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/lo_amd.h"

namespace lo {

constexpr int kThreads = 256;  // 4 wave64 per workgroup everywhere (vector / skinny kernels)
constexpr int kMaxCols = 256;  // a workgroup's thread->column map needs c <= 256
constexpr int kMaxRank = 256;  // padded root rank (floats per row) of a skinny operand

#define LO_HIP_CHECK(expr)                                                                  \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess) {                                                                 \
      fprintf(stderr, "liblo_amd: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return LO_ERR_LAUNCH;                                                                 \
    }                                                                                       \
  } while (0)

#define LO_LAUNCH_CHECK() LO_HIP_CHECK(hipGetLastError())

// opt-in event timing of a launch (lo_prof.hip)
extern bool g_prof_on;
void prof_start(const char* name, hipStream_t st);
void prof_stop(hipStream_t st);
#define LO_PROF_BEGIN(name, st) \
  do {                          \
    if (lo::g_prof_on) lo::prof_start(name, st); \
  } while (0)
#define LO_PROF_END(st)                 \
  do {                                  \
    if (lo::g_prof_on) lo::prof_stop(st); \
  } while (0)

// host-side intervals of an entry point (steady_clock), reported by lo_prof_report as "host:<name>" lines next to the
// event scopes.  lo_prof_enable(2) turns them on WITHOUT the event scopes, whose two hipEventRecord calls per launch would
// sit inside the intervals (tools/mb_step_gap.py).
extern bool g_prof_host;
void prof_host(const char* name, double us);

// Row split of one batch member over S workgroups (rows multiple of 4 except the tail).
struct Split {
  int S;
  int rows;
};
// (max_split: 256 unless a caller's kernels hold the partials of a member in a fixed-size buffer)
Split choose_split(int64_t B, int64_t N, int min_rows, int max_split = 256);

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Bump allocator over the caller's workspace.  Over no workspace (base == nullptr) it MEASURES: take() returns nullptr and
// only `off` advances, so the function that lays a workspace out is also the one that sizes it.  `tail`: bytes kept free
// behind the takes, what the entry point's sizer adds to its layout -- a workspace smaller than the reported size is not ok.
struct Arena {
  char* base;
  size_t cap, off;
  bool ok;
  Arena(void* p, size_t bytes, size_t tail = 0)
      : base((char*)p), cap(bytes >= tail ? bytes - tail : 0), off(0), ok(!p || bytes >= tail) {}
  bool measuring() const { return !base; }
  template <typename T>
  T* take(size_t n) {
    off = align_up(off, 256);
    size_t bytes = n * sizeof(T);
    T* r = (T*)(base ? base + off : nullptr);
    off += bytes;
    if (base && off > cap) ok = false;
    return r;
  }
};
// the body of a sizer: what `layout` takes from a measuring arena, plus the entry point's tail
template <typename F>
size_t measured(size_t tail, F layout) {
  Arena ar(nullptr, 0);
  layout(ar);
  return ar.off + tail;
}

// floats per row of a rank-R factor (C, Q) as the skinny kernels read it: 4 * (R / 4 rounded up to a power of two)
inline int padded_rank(int64_t R) {
  int64_t rq = (R + 3) / 4, p = 1;
  while (p < rq) p <<= 1;
  return (int)(4 * p);
}

// ---------------------------------------------------------------------------------------------
// device control block of one CG solve (lives in the workspace; host polls it)
struct CgCtrl {
  int stop;               // sticky: every kernel of the solve exits at once when set
  int iterations;         // loop bodies executed
  int tol_reached;
  int nan_detected;
  int skipped;
  int last_tridiag_iter;
  int tri_disabled;       // update_tridiag == False (linear_cg.py:326-327)
  float mean_resid;
  int oc_err;             // operator-resident kernels: a group exchange timed out (host falls back to streaming)
  int oc_next;            // operator-resident kernels: shared counter of the dynamic member hand-out
  int oc_next_ls;         // the same for the column-lockstep kernel (both may run in one solve)
  int pf_next;            // the same for the fused preconditioner apply of the streaming loop
  int rs_redo;            // diagonal form of the R-space iteration: a member's right-hand side lies (almost) inside span(C) --
                          // the host repeats the launch with the dense form (lo_rspace.hip)
};

// fused-update arguments of the skinny tn kernels (VMODE 1: p-update, VMODE 2: r/x-update; see lo_skinny.hip)
struct TnFuse {
  // VMODE 1
  const float* z;
  const float* beta;  // [B, ldv]
  int first;
  // VMODE 2
  const float* Ap;
  const float* p;
  float* x;
  const float* pAp_part;  // [B, S_dot, ldv]
  int S_dot;
  const float* rz;        // [B, ldv]
  const int* has_conv;    // [B, ldv]
  float eps;
  float* alpha_out;       // [B, ldv]
  float* rr_part;         // [B, S, ldv]
};

// matrix-core versions for 8 < c <= 32 (lo_skinny_mfma.hip); tpart layout [B,S,R4,c]
bool skinny_mfma_ok(int R4, int64_t c);
int skinny_tn_mfma(int vmode, const float* A, int R4, float* v, int64_t c, float* tpart, int64_t B, int64_t N, Split sp,
                   const TnFuse& f, const int* stop, hipStream_t st);
int skinny_nn_mfma(const float* A, int R4, const float* tpart, const float* dd, int dd_mode, float sgn, const float* v,
                   int64_t c, float* y, float* dot_part, int64_t B, int64_t N, Split sp, const int* stop,
                   hipStream_t st);

// ---- skinny operand kernels (lo_skinny.hip): A [B,N,lda] with R4 = 4*RQ padded columns --------
// tpart[B,S,R4,c] = A[rows_s]^T v[rows_s]
int skinny_tn(const float* A, int lda, int R4, const float* v, int64_t c, float* tpart, int64_t B, int64_t N, Split sp,
              const int* stop, hipStream_t st);
// y = sgn * A (sum_s tpart) + dd o v ; optional dot_part[B,S,c] = sum_rows v o y
int skinny_nn(const float* A, int lda, int R4, const float* tpart, const float* dd, int dd_mode, float sgn,
              const float* v, int64_t c, float* y, float* dot_part, int64_t B, int64_t N, Split sp, const int* stop,
              hipStream_t st);
// fused CG variants of skinny_tn (see lo_skinny.hip): the input vector is built on the fly
//   pupdate: p = z + beta p (first: p = z), written back, then tpart = A^T p
//   rupdate: masked alpha from pAp partials; r -= alpha Ap (written back); x += alpha p; rr_part = sum r^2; tpart = A^T r
int skinny_tn_pupdate(const float* A, int lda, int R4, float* p, const float* z, const float* beta, int first, int64_t c,
                      float* tpart, int64_t B, int64_t N, Split sp, const int* stop, hipStream_t st);
int skinny_tn_rupdate(const float* A, int lda, int R4, float* r, const float* Ap, const float* p, float* x,
                      const float* pAp_part, int S_dot, const float* rz, const int* has_conv, float eps,
                      float* alpha_out, float* rr_part, int64_t c, float* tpart, int64_t B, int64_t N, Split sp,
                      const int* stop, hipStream_t st);
// copy rows [B,N,R] -> zero padded [B,N,R4]
int pad_rows(const float* src, int R, float* dst, int R4, int64_t rows, hipStream_t st);

// ---- vector kernels (lo_vec.hip): vectors [B,N,c] ------------------------------------------------
int vec_dot_part(const float* a, const float* b, int64_t c, float* part, int64_t B, int64_t N, Split sp, const int* stop,
                 hipStream_t st);
// y = dd o v added onto y (dense / kron matvec epilogue): y += dd o v
int vec_add_diag(const float* dd, int dd_mode, const float* v, float* y, int64_t c, int64_t B, int64_t N, Split sp,
                 const int* stop, hipStream_t st);

// ---- operator matvec plan (lo_matvec.hip) ----------------------------------------------------
// A kind is a state struct, a plan function and a run function.  The plan function validates the descriptor, takes the
// kind's buffers from the arena in a fixed order and fills the state; on a measuring arena it makes the same takes and
// launches nothing, which is how the workspace is sized (matvec_plan_bytes).
struct MatvecPlan;
// low-rank, dense, Kronecker, sum: planned and run in lo_matvec.hip
struct LowrankPlan {
  const float* Apad;  // padded copy of C when R % 4 != 0 (else op.A0)
  int lda, R4;
  float* tpart;       // [B,S,R4,c]
  bool mv_resident;   // shape the one-pass resident matvec takes (lo_lowrank_mv.hip); else the two-pass kernels
};
struct DensePlan {
  float* part;  // split-K partials of the dense matvec (small batches) or nullptr
};
struct KronPlan {
  float* tmp;  // [B,N,c], twice that on the matrix-core route of c > 1 columns
};
struct SumPlan {
  float* ytmp;  // [B,N,c]: a term beyond the first is computed into it before it is added onto y (terms: MatvecPlan::sub)
};

// ---- SKI / Toeplitz (lo_ski.hip) ------------------------------------------------------------------------------------
// LO_OP_SKI_DIAG, LO_OP_TOEPLITZ_DIAG (lo_ski.hip) and LO_OP_SKI_GRID_DIAG (lo_ski_grid.hip) share one state: the
// interpolation matrices (with the grid shape of the grid kind), the grid-major copy of W_r, the grid-sized
// intermediates u = W_r^T v and T u, and the split-k partials of the 1-D Toeplitz product (nullptr for the grid kind)
struct CsrBufs {
  int* ptr;  // [B, M+1] offsets of the grid points' entries
  int* cur;  // [B, M+1] fill cursors of the build
  int* tmp;  // [B, N*J] entry ids by grid point, unsorted
  int* ids;  // [B, N*J] the same in ascending order within a grid point
};
struct SkiPlan {
  lo_interp_desc w;
  CsrBufs csr;
  float *u, *t;  // [B, M, c]
  float* tz_part;
};
int ski_plan(MatvecPlan* pl, Arena* ar, hipStream_t st);
int ski_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st);
// LO_OK, or why the descriptor of that kind is refused: what the plan function and the pivoted Cholesky (which validates
// without a plan) both check; each adds the bounds of its own kernels.  One per kind, next to the kind's plan function.
int toeplitz_desc_check(const lo_op_desc* op);
int ski_desc_check(const lo_op_desc* op);
inline bool interp_ptrs_ok(const lo_interp_desc* w) {
  return w && w->left_idx && w->left_vals && w->right_idx && w->right_vals;
}
// the interpolation kernels and the grid-major copy of W, shared with the grid kind (lo_ski_grid.hip)
bool interp_shape_ok(int64_t B, int64_t N, int64_t J, int64_t M);
int interp_gather(const int64_t* idx, const float* vals, int64_t B, int64_t N, int64_t J, int64_t M, const float* u,
                  int64_t c, const float* dd, int dd_mode, const float* v, float* y, const int* stop, hipStream_t st);
int interp_scatter(const int* ptr, const int* ids, const float* vals, int64_t B, int64_t N, int64_t J, int64_t M,
                   const float* v, int64_t c, float* out, const int* stop, hipStream_t st);
// the one layout of the grid-major copy; csr_bytes measures it, csr_build fills it (a measuring arena: takes only),
// csr_view finds the buffers of a copy built earlier into `plan`
void csr_layout(Arena& ar, int64_t B, int64_t N, int64_t J, int64_t M, CsrBufs* b);
size_t csr_bytes(int64_t B, int64_t N, int64_t J, int64_t M);
int csr_build(const int64_t* idx, int64_t B, int64_t N, int64_t J, int64_t M, Arena* ar, CsrBufs* b, hipStream_t st);
CsrBufs csr_view(const void* plan, int64_t B, int64_t N, int64_t J, int64_t M);
// the part of the plan the SKI kinds share: u, t and the copy of W_r (built here, or the caller's right_plan)
int ski_interp_plan(MatvecPlan* pl, int64_t M, Arena* ar, hipStream_t st);

// ---- additive SKI, a sum of P 1-D terms over the same rows (lo_ski_sum.hip): LO_OP_SKI_SUM_DIAG, on SkiPlan ---------
// The state of the SKI kind over the G = B * P grid members (member g = b * P + p): u, t [G, M, c], the copy of W_r and
// the split-k partials of G Toeplitz products.
int ski_sum_plan(MatvecPlan* pl, Arena* ar, hipStream_t st);
int ski_sum_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st);
int ski_sum_desc_check(const lo_op_desc* op);
// interp_scatter with member g of W reading v[g / vdiv] (v [B / vdiv, N, c])
int interp_scatter_bcast(const int* ptr, const int* ids, const float* vals, int64_t B, int vdiv, int64_t N, int64_t J,
                         int64_t M, const float* v, int64_t c, float* out, const int* stop, hipStream_t st);
// the 1-D Toeplitz product of lo_ski.hip and the floats of its split-k partials `part`
size_t toeplitz_part_floats(int64_t B, int64_t M, int64_t c);
int toeplitz_mv(const float* t, int64_t B, int64_t M, const float* u, int64_t c, const float* dd, int dd_mode,
                const float* v, float* y, float* part, const int* stop, hipStream_t st);

// ---- SKI on a 2-D / 3-D grid (lo_ski_grid.hip): LO_OP_SKI_GRID_DIAG, on SkiPlan ---------------------------------------
int ski_grid_plan(MatvecPlan* pl, Arena* ar, hipStream_t st);
int ski_grid_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st);
int ski_grid_desc_check(const lo_op_desc* op);

// ---- Kronecker product of 2 / 3 symmetric Toeplitz factors (lo_ski_grid.hip): LO_OP_TOEPLITZ_KRON_DIAG -----------------
struct ToeplitzKronPlan {
  lo_grid_desc g;   // a copy of the host struct op.grid
  float* tmp;       // [B, M, c]: the grid vector between the passes (the last pass writes y)
  bool epilogue;    // the diagonal term as a kernel of its own behind the passes (A/B switch; default: in the last pass)
};
int toeplitz_kron_plan(MatvecPlan* pl, Arena* ar, hipStream_t st);
int toeplitz_kron_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st);
int toeplitz_kron_desc_check(const lo_op_desc* op);

// ---- Hadamard product of two roots (lo_hadamard.hip) ---------------------------------------------------------------
struct HadamardPlan {
  float *part, *m;  // the contraction partials and the reduced M_t of every column (lo_hadamard.hip)
};
int hadamard_plan(MatvecPlan* pl, Arena* ar, hipStream_t st);
int hadamard_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st);
int hadamard_desc_check(const lo_op_desc* op);

// ---- matrix-free kernel operator (lo_kernel_op.hip): LO_OP_KERNEL_DIAG ------------------------------------------------
struct KernelOpPlan {
  float* part;  // [js, B, N, c] partial products when the columns j of a member are split over js workgroups, else nullptr
  float* ytmp;  // LO_OP_KERNEL_SUM_DIAG on its per-term route: [B, N, c], a term beyond the first before it is added onto y
};
int kernel_op_plan(MatvecPlan* pl, Arena* ar, hipStream_t st);
int kernel_op_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st);
int kernel_desc_check(const lo_op_desc* op);

// ---- sum of matrix-free kernel operators over the same points (lo_kernel_sum.hip): LO_OP_KERNEL_SUM_DIAG, on KernelOpPlan
int kernel_sum_plan(MatvecPlan* pl, Arena* ar, hipStream_t st);
int kernel_sum_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st);
int kernel_sum_desc_check(const lo_op_desc* op);

// ---- matrix-free multitask operator Kernel(X, X) (x) Bt (lo_kernel_kron.hip): LO_OP_KERNEL_KRON_DIAG -------------------
struct KernelKronPlan {
  float* part;  // [js, B, n, T c] partial products when the points j of a member are split over js workgroups, else nullptr
};
int kernel_kron_plan(MatvecPlan* pl, Arena* ar, hipStream_t st);
int kernel_kron_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st);
int kernel_kron_desc_check(const lo_op_desc* op);

// ---- matrix-free LMC operator sum_q Kernel_q(X, X) (x) B_q (lo_kernel_lmc.hip): LO_OP_KERNEL_LMC_DIAG, on KernelKronPlan
int kernel_lmc_plan(MatvecPlan* pl, Arena* ar, hipStream_t st);
int kernel_lmc_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st);
int kernel_lmc_desc_check(const lo_op_desc* op);

// ---- matrix-free RBF gradient kernel, D + 1 outputs per input (lo_kernel_grad.hip): LO_OP_KERNEL_GRAD_DIAG -------------
struct KernelGradPlan {
  float* part;  // [js, B, n, (D + 1) c] partial products when the points j of a member are split over js workgroups, else nullptr
};
int kernel_grad_plan(MatvecPlan* pl, Arena* ar, hipStream_t st);
int kernel_grad_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st);
int kernel_grad_desc_check(const lo_op_desc* op);

// ---- matrix-free task-indexed multitask operator (lo_kernel_task.hip): LO_OP_KERNEL_TASK_DIAG ----------------------------
struct KernelTaskPlan {
  float* part;  // [js, B, N, c] partial products when the columns j of a member are split over js workgroups, else nullptr
};
int kernel_task_plan(MatvecPlan* pl, Arena* ar, hipStream_t st);
int kernel_task_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st);
int kernel_task_desc_check(const lo_op_desc* op);

// ---- matrix-free kernels with a shape parameter, RQ and periodic (lo_kernel_param.hip): LO_OP_KERNEL_PARAM_DIAG, on
// KernelOpPlan (its `part`)
int kernel_param_plan(MatvecPlan* pl, Arena* ar, hipStream_t st);
int kernel_param_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st);
int kernel_param_desc_check(const lo_op_desc* op);

// ---- matrix-free spectral mixture kernel (lo_kernel_sm.hip): LO_OP_KERNEL_SM_DIAG, on KernelOpPlan (its `part`)
int kernel_sm_plan(MatvecPlan* pl, Arena* ar, hipStream_t st);
int kernel_sm_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st);
int kernel_sm_desc_check(const lo_op_desc* op);

// ---- masked operator (lo_masked.hip) ---------------------------------------------------------------------------------
struct MaskedPlan {      // (the base's plan is MatvecPlan::sub[0])
  const int64_t* idx;    // [M]
  int64_t N0;
  int* inv;              // [N0], -1 where masked out
  float *u, *w;          // [B, N0, c]: u = S^T v and the base's result (w == nullptr on the dense route)
  bool dense;
};
int masked_plan(MatvecPlan* pl, Arena* ar, hipStream_t st);
int masked_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st);

// ---- the plan and its dispatch (lo_matvec.hip) -----------------------------------------------------------------------
// Partials per (member, column) the kind's matvec writes into dot_part.  The one source: the plan functions store it in
// MatvecPlan::S_dot and the solvers size their partial buffers by it before the plan is laid out.
int matvec_S_dot(const lo_op_desc* op, int64_t c, Split sp);
struct MatvecPlan {
  lo_op_desc op;
  int64_t c;
  Split sp;    // row split used by the skinny kernels / dot partials
  int S_dot;   // number of partials per (b,col) the plan writes into dot_part
  lo_matvec_cb cb;
  void* cb_user;
  // LO_OP_SUM: one sub-plan per term; LO_OP_MASKED: the base's plan.  Host heap, released by matvec_plan_free; a
  // measuring pass keeps none.
  int nterms;
  MatvecPlan* sub;
  union {  // the state of op.kind
    LowrankPlan lr;
    DensePlan dense;
    KronPlan kron;
    SumPlan sum;
    SkiPlan ski;
    ToeplitzKronPlan tk;
    HadamardPlan hd;
    KernelOpPlan ko;
    KernelKronPlan kk;
    KernelGradPlan kg;
    KernelTaskPlan kt;
    MaskedPlan mask;
  };
};
void matvec_plan_free(MatvecPlan* pl);
// releases a plan's sub-plans on every exit path of the function that owns it
struct PlanGuard {
  MatvecPlan* p;
  explicit PlanGuard(MatvecPlan* q) : p(q) {
    p->sub = nullptr;
    p->nterms = 0;
  }
  ~PlanGuard() { matvec_plan_free(p); }
};
// y += a (elementwise, n floats)
int vec_axpy1(float* y, const float* a, size_t n, const int* stop, hipStream_t st);
// clears `bytes` at p (16-byte aligned) with one kernel launch (control blocks / hand-off granules of a resident launch)
int zero_span(void* p, size_t bytes, hipStream_t st);
// Lays the plan of `op` out in the arena: validates, takes the buffers, stages what the kernels need (the padded copy
// of C, the grid-major copy of W_r, the inverse map of a mask).  A failed call holds no sub-plans.  On a measuring
// arena nothing is launched or kept and the return code only says whether the descriptor is valid: ar->off is the
// size.  A caller that lays out more than the plan calls it in both modes, with a scratch plan when it measures.
int matvec_plan_init(MatvecPlan* pl, const lo_op_desc* op, lo_matvec_cb cb, void* cb_user, int64_t c, Split sp,
                     Arena* ar, hipStream_t st);
// what matvec_plan_init takes from an empty arena, plus kPlanTail
constexpr size_t kPlanTail = 256;  // every size reported for a plan alone ends with it: never zero bytes to allocate
size_t matvec_plan_bytes(const lo_op_desc* op, int64_t c, Split sp);
// y = A v (+ optional dot partials sum_rows v o y, S_dot per (b,col))
int matvec_run(const MatvecPlan* pl, const float* v, float* y, float* dot_part, const int* stop, hipStream_t st);
// true if the plan can fuse the CG search-direction update into its first pass (low-rank operators)
bool matvec_can_fuse_pupdate(const MatvecPlan* pl);
// p = z + beta p (first: p = z); y = A p; dot partials
int matvec_run_pupdate(const MatvecPlan* pl, float* p, const float* z, const float* beta, int first, float* y,
                       float* dot_part, const int* stop, hipStream_t st);
// kinds a sum may hold and a mask may cover directly: the plain structured operators
inline bool plain_term_kind(int kind) {
  return kind == LO_OP_LOWRANK_DIAG || kind == LO_OP_DENSE_DIAG || kind == LO_OP_KRON_DIAG;
}
// the matrix-free kernel kinds: terms of a sum next to the plain ones (fp32 engines only; not under a mask)
inline bool kernel_term_kind(int kind) {
  return kind == LO_OP_KERNEL_DIAG || kind == LO_OP_KERNEL_SUM_DIAG || kind == LO_OP_KERNEL_PARAM_DIAG ||
         kind == LO_OP_KERNEL_SM_DIAG;
}

// ---- the Q-form Woodbury apply z = dinv o r - Q (Q^T r) as a plan (lo_skinny.hip): staged and run
// through these two functions by the streaming CG and MINRES engines and by lo_precond_apply_f32 ----------------------
struct PrecondPlan {
  const float* Qp;  // Q with R4 floats per row: the caller's (ldq == R4) or the padded copy; nullptr: root form only
  int R4;           // padded_rank(k)
  float* upart;     // [B,S,R4,c] partials of Q^T r
  const float* dinv;
  int dinv_mode;
  int64_t B, N, c;
  Split sp;
};
// Takes upart, then (Q given, ldq != R4) the padded copy of Q, and pads; ldq must then be k, else LO_ERR_BADARG.  On a
// measuring arena it makes the same takes and nothing else: the return code only says whether the descriptor is valid.
int precond_plan_init(PrecondPlan* pp, const lo_precond_desc* pre, int64_t B, int64_t N, int64_t c, Split sp, Arena* ar,
                      hipStream_t st);
// z = dinv o r - Qp (Qp^T r); optional dot_part[B,S,c] = sum_rows r o z
int precond_plan_run(const PrecondPlan* pp, const float* r, float* z, float* dot_part, const int* stop, hipStream_t st);
// The descriptor the solver sizers lay out when they are given none: a closure preconditioner may be used with the
// workspace, which needs z (CG) / the q vectors (MINRES) and no more staging than the smallest Q form.
inline lo_precond_desc worst_case_precond() { return lo_precond_desc{/*k*/ 4, /*ldq*/ 4}; }

// dense / kron kernels
int dense_matvec(const float* K, const float* d, int dd_mode, const float* v, float* y, float* dot_part, int64_t B,
                 int64_t N, int64_t c, int rows_per_wg, float* ypart, const int* stop, hipStream_t st);
int dense_rows_per_wg(int64_t B, int64_t N);
// number of dot partials per (member, column) the dense matvec writes for this shape (VALU vs MFMA tiling)
int dense_S_dot(int64_t B, int64_t N, int64_t c);
bool dense_mfma_ok(int64_t N, int64_t c);
int dense_mfma_tiles(int64_t N);
// ypart: dense_mfma_slices(B, N, c) * B * N * c floats for the split-K partials of small batches, or nullptr (no split)
int dense_mfma_slices(int64_t B, int64_t N, int64_t c);
int dense_matvec_mfma(const float* K, const float* d, int dd_mode, const float* v, float* y, float* dot_part, int64_t B,
                      int64_t N, int64_t c, float* ypart, const int* stop, hipStream_t st);
int kron_matvec(const float* K1, const float* K2, const float* v, float* tmp, float* y, int64_t B, int n1, int n2,
                int64_t c, const int* stop, hipStream_t st);
// matrix-core engine (c == 1, factors multiples of 128): diagonal term and CG dot partials fused in the epilogue
int kron_bilinear(const float* K1, const float* K2, const float* U, const float* V, float* tmp, float* dK1, float* dK2,
                  int64_t B, int n1, int n2, int64_t D, hipStream_t st);
bool kron_mfma_ok(int n1, int n2, int64_t c);
bool kron_mfma_cols_ok(int n1, int n2, int64_t c);  // c > 1 on the matrix-core engine (columns moved to the front)
int kron_matvec_mfma_cols(const float* K1, const float* K2, const float* diag, int diag_mode, const float* v,
                          float* buf_a, float* buf_b, float* y, int64_t B, int n1, int n2, int64_t c, const int* stop,
                          hipStream_t st);
int kron_S_dot(int n1, int n2, int64_t c, int S_default);
int kron_matvec_mfma(const float* K1, const float* K2, const float* diag, int diag_mode, const float* v, float* tmp,
                     float* y, float* dot_part, int64_t B, int n1, int n2, const int* stop, hipStream_t st);

// ---- one-pass operator-resident matvec of low-rank + diagonal members (lo_lowrank_mv.hip) ------------------------
// y = C (C^T v) + d o v with C read from HBM once (rows wait in registers for the group all-reduce of t = C^T v).
// R4 = padded rank 8 / 16 / 32, c <= 4 columns, N <= 32768.  LO_ERR_UNSUPPORTED: the caller runs the two-pass kernels.
bool lowrank_mv_eligible(int R4, int64_t N, int64_t c);
int lowrank_mv_run(const float* C, int R4, const float* d, int d_mode, const float* v, float* y, int64_t B, int64_t N,
                   int64_t c, const int* stop, hipStream_t st);

// ---- operator-resident CG (lo_cg_onchip.hip) -----------------------------------------------------
// The LO_* switches of the CG driver and of the resident launch helpers.
struct CgSwitches {
  bool no_lockstep, gw8, keep_state, no_rspace_cols, no_rspace, no_wrec, no_kron_root;  // engine selection (cg_plan)
  bool no_fused_ctrl;     // the fused apply / column step leave the control step to k_cg_scal / k_cg_ctrl
  bool oc_test_fallback;  // the resident kernels start with the error word set, as if a hand-off had timed out
  bool rs_no_diag;        // no diagonal form of the R-space iteration (rspace_launch reads it too)
  bool clear_handoff;     // the headline solve on the caller's workspace behind a clearing launch, as every other plan
  int sc_test_fallback;   // the error word set behind the fused column step of iteration k (-1: never)
  bool operator==(const CgSwitches& o) const {
    return no_lockstep == o.no_lockstep && gw8 == o.gw8 && keep_state == o.keep_state && no_rspace_cols == o.no_rspace_cols &&
           no_rspace == o.no_rspace && no_wrec == o.no_wrec && no_kron_root == o.no_kron_root &&
           no_fused_ctrl == o.no_fused_ctrl && oc_test_fallback == o.oc_test_fallback && rs_no_diag == o.rs_no_diag &&
           clear_handoff == o.clear_handoff && sc_test_fallback == o.sc_test_fallback;
  }
};
// Every one of them, taken in ONE pass over the process environment (a getenv per switch walked it some twenty times per
// solve).  cg_env() is the one reader: inside an EnvScope -- the CG entry points open one -- it returns the pass made when
// the scope opened, so a call reads the environment once; outside, every cg_env() is a pass of its own.  The general
// path therefore still sees a switch flipped between two calls (bench.py and the tests do that), and a solve session
// compares the call's pass with the one it was created under.
struct CgEnv {
  CgSwitches sw;
  bool ls_debug, oc_debug, sc_debug;  // LO_LS_DEBUG / LO_OC_DEBUG / LO_SC_DEBUG (CgDebug)
  int ls_member, oc_member;
  bool no_l2_handoff;                 // LO_OC_NO_L2_HANDOFF (onchip_l2_handoff_allowed)
  bool has_reserve; int reserve_cus;  // LO_OC_RESERVE_CUS (onchip_num_workgroups)
  bool no_resident_order;             // LO_NO_RESIDENT_ORDER (ResidentLaunch)
  bool operator==(const CgEnv& o) const {
    return sw == o.sw && ls_debug == o.ls_debug && oc_debug == o.oc_debug && sc_debug == o.sc_debug &&
           ls_member == o.ls_member && oc_member == o.oc_member && no_l2_handoff == o.no_l2_handoff &&
           has_reserve == o.has_reserve && reserve_cus == o.reserve_cus && no_resident_order == o.no_resident_order;
  }
};
CgEnv cg_env();
struct EnvScope {
  EnvScope();
  ~EnvScope();
  EnvScope(const EnvScope&) = delete;
  EnvScope& operator=(const EnvScope&) = delete;
};
struct OnchipArgs;
size_t onchip_gbuf_bytes(int ngroups);
// fp64 Gram partials of a root on the fp64 matrix cores (lo_rspace.hip): E = C^T diag(dinv) C (dinv_full != nullptr) and C^T C
void rs_gram64_launch(const float* C, const float* dinv_full, int64_t B, int64_t N, int R, Split sp, double* gpartE,
                      double* gpart2, hipStream_t st);
int onchip_num_workgroups();
int onchip_l2_handoff_allowed();  // same-XCD plain-store hand-off: verified architectures only (lo_cg_onchip.hip)
bool onchip4_eligible(int RC, int RK, int64_t N, int64_t c);  // lo_cg_onchip4.hip
int onchip4_group_size(int64_t N);
int onchip5_group_size(int64_t N);
// Kernels whose workgroups wait for each other need ALL of them resident: two such kernels on two streams of one
// process would each take part of the CUs and spin until the hand-off timeout.  Construct a ResidentLaunch right before
// such a launch (same scope): if the previous resident kernel of this process went to a DIFFERENT stream, the new stream
// is made to wait for everything submitted to that stream so far; host threads are serialised for the duration of the
// launch call.  No cost when all solves use one stream.
struct ResidentLaunch {
  explicit ResidentLaunch(hipStream_t st);
  ~ResidentLaunch();
  ResidentLaunch(const ResidentLaunch&) = delete;
  ResidentLaunch& operator=(const ResidentLaunch&) = delete;
};
struct ResidentLock {  // the same lock without a launch (host state that resident launches read under it)
  ResidentLock();
  ~ResidentLock();
  ResidentLock(const ResidentLock&) = delete;
  ResidentLock& operator=(const ResidentLock&) = delete;
};
extern bool g_onchip_disabled;  // lo_cg_set_onchip(0): streaming engines only (tests compare the two)
extern int g_onchip_fused_timeouts;  // group exchanges of the fused solve that timed out in this process
// A REAL hand-off timeout (co-residency lost: another process / kernel holds part of the CUs) sends the next calls to
// the streaming engines for a cool-down (16 calls, doubling up to 4096 while the timeouts repeat), after which the
// resident kernels are tried again; lo_cg_set_onchip(1) ends a cool-down at once (lo_cg.hip, lo_resident_status).
// The injected timeout of LO_OC_TEST_FALLBACK does not start a cool-down; lo_resident_inject_timeouts does.
void onchip_note_timeout();
bool resident_off();            // user switch or cool-down: no resident kernel for this call
void resident_tick();           // entry points: one call of the cool-down served
void resident_note_ok();        // a resident solve completed: the next cool-down is short again
bool resident_take_injection(); // lo_resident_inject_timeouts: treat this resident launch as timed out
// Pinned host landing zone for the small status read-backs of the synchronous entry points (a device-to-host copy into
// pageable memory is staged through an internal buffer and costs tens of microseconds more): one 256-byte block per
// host thread, allocated on first use; nullptr if pinned memory is unavailable (callers then copy to their stack).
void* pinned_status_block();
// hipOccupancyMaxActiveBlocksPerMultiprocessor costs microseconds per call and its answer for a given kernel, block
// size and dynamic LDS size never changes within a process: asked once per call site (one site per instantiation)
#define LO_OCCUPANCY_CACHED(out_int, kernel, tpb, dyn_lds)                                                   \
  ([&]() -> hipError_t {                                                                                     \
    static int cached = -1;                                                                                  \
    static hipError_t cached_err = hipSuccess;                                                               \
    if (cached < 0) {                                                                                        \
      int v = 0;                                                                                             \
      cached_err = hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, kernel, tpb, dyn_lds);                   \
      cached = (cached_err == hipSuccess) ? v : 0;                                                           \
    }                                                                                                        \
    (out_int) = cached;                                                                                      \
    return cached_err;                                                                                       \
  }())

// ---- fp64 helpers (lo_cg_f64.hip), shared by the fp64 CG and MINRES engines ---------------------------------------
// out1[b, j] = sum_i a[b, i, j] b1[b, i, j] (and out2 from (a2, b2) when a2 != nullptr)
int f64_dots(const double* a, const double* b1, double* out1, const double* a2, const double* b2, double* out2,
             int64_t B, int64_t N, int64_t c, hipStream_t st);
int f64_dense_mv(const double* A, const double* d, const double* v, double* y, int64_t B, int64_t N, int64_t c,
                 hipStream_t st);
// the same kernel with the diagonal as (d, LO_DIAG_*) and, accumulate != 0, the product added onto y (lo_matvec_f64.hip)
int f64_dense_mv_ex(const double* A, const double* d, int dmode, int accumulate, const double* v, double* y, int64_t B,
                    int64_t N, int64_t c, hipStream_t st);
int f64_copy(const double* a, double* o, size_t total, hipStream_t st);
// the float64 matrix-free kernel product (lo_kernel_op_f64.hip) for lo_matvec_f64: the check of an LO_OP_KERNEL_DIAG
// descriptor whose A0 / A1 point to doubles, the one layout of the product's workspace (the partials [js, B, M, c] of a
// split member, else nullptr) and the product itself on validated arguments ([y +] K v + d o v)
int kernel_desc_check_f64(const lo_op_desc* op, int64_t c);
double* kernel_mv_layout_f64(Arena& ar, int64_t B, int64_t M, int64_t N, int64_t c);
int kernel_mv_run_f64(const double* x1, const double* x2, const double* theta, int family, int64_t B, int64_t M,
                      int64_t N, int64_t D, const double* v, int64_t c, const double* d, int dmode, int accumulate,
                      double* y, double* part, hipStream_t st);

// ---- single-pass Woodbury apply fused with the CG r / x update (lo_precond_fused.hip) --------------
bool precond_fused_eligible(int64_t B, int64_t N, int64_t c, int ldq, int S);
bool precond_fused_kron_eligible(int64_t n1, int64_t n2);  // factor sizes the Kronecker root-form kernel takes
size_t precond_fused_gbuf_bytes();
// the iteration's control step folded into the fused apply (single column, no tridiagonal, k >= 1)
struct PfCtrl {
  int on;
  const int* rhs_is_zero;  // [B]
  float* rz;               // [B] residual_inner_prod out
  float* beta;             // [B]
  float* resid_norm;       // [B]
  int* has_conv;           // [B]
  float stop_after, tol;
  int kfloor;              // min(10, max_iter - 1)
  int* done;               // base of one zeroed counter per launch of the solve
  unsigned long long* gran; // [B] tagged residual norms of the current launch (zeroed once per solve)
  CgCtrl* ctrl;
};
// Kronecker root form of the preconditioner (lo_precond_desc.kron_*): rows of "Q" formed on the fly (nullptr = Q form)
struct PfKron {
  const float* a;
  const float* b;
  const float* F;
  int n1, n2;
};
// (also writes the next iteration's p = z + beta p; z itself is not stored)
int precond_fused_rupdate(const float* Q, const float* dinv, int dinv_mode, float* r, const float* Ap, float* p,
                          float* x, float* z, const float* pAp_part, int S_dot, const float* rz, const int* has_conv,
                          float eps, float* alpha_out, float* rr_part, float* rz_part, int S, int64_t B, int64_t N,
                          unsigned long long* gbuf, int* err, int* next_member, int launch, const int* iter_ptr,
                          int max_launch, const int* stop, int ncu, const PfCtrl* cf, const PfKron* kr,
                          hipStream_t st);

// ---- the whole post-product step of a streaming CG iteration for up to 32 columns (lo_cg_step_cols.hip) ----------
// the iteration's control step (cg_scal_body + cg_ctrl_body of lo_cg.hip) folded into that launch
struct ScCtrl {
  int on;
  const int* rhs_is_zero;  // [B, c]
  float* beta;             // [B, c]
  float* resid_norm;       // [B, c]
  float stop_after, tol;
  int max_iter;            // the value the stop-rule floors are taken from
  int n_tridiag, n_tridiag_iter, T;
  float* t_mat;            // [n_tridiag, B, T, T]
  float* prev_ar;          // [B, n_tridiag]
  float* prev_beta;
  int check_nan_first;
  int* done;               // base of one zeroed counter per launch of the solve
  unsigned long long* gran; // [3, B] tagged per-member aggregates of the current launch (zeroed once per solve)
  CgCtrl* ctrl;
};
bool cg_step_cols_eligible(int64_t B, int64_t N, int64_t c, int ldq);  // ldq = 0: no preconditioner
size_t cg_step_cols_gbuf_bytes();
int cg_step_cols_group(int64_t N);
bool cg_step_cols_worthwhile(int64_t B, int64_t N, int64_t c, bool has_pre);
int cg_step_cols(const float* Q, int ldq, const float* dinv, int dinv_mode, float* r, const float* Ap, float* p, float* x,
                 int64_t c, const float* pAp_part, int S_dot, float* rz, int* has_conv, float eps, float* alpha_out,
                 float* rr_part, float* rz_part, int S, int64_t B, int64_t N, unsigned long long* gbuf, int* err,
                 int* next_member, int launch, int max_launch, const int* stop, int ncu, const ScCtrl* cf,
                 long long* dbg, hipStream_t st);

// ---- operator-resident pivoted Cholesky (lo_pivchol_onchip.hip) ----------------------------------
bool pc_onchip_eligible(const lo_op_desc* op, int max_rank);
size_t pc_onchip_workspace_bytes(const lo_op_desc* op, int max_rank);
// returns LO_ERR_LAUNCH when the group exchange timed out (caller falls back to the streaming engine)
int pc_onchip_run(const lo_op_desc* op, int rank, int max_rank, float tol, float* L_rows, long long* perm,
                  int32_t* rank_out, void* ws, size_t ws_bytes, hipStream_t st);

// the same for operators whose rows are fetched (dense, Kronecker of two dense factors): k_pc_onchip_rows
bool pc_onchip_rows_eligible(const lo_op_desc* op, int max_rank);
size_t pc_onchip_rows_workspace_bytes(const lo_op_desc* op, int max_rank);
int pc_onchip_rows_run(const lo_op_desc* op, int rank, int max_rank, float tol, float* L_rows, long long* perm,
                       int32_t* rank_out, void* ws, size_t ws_bytes, hipStream_t st);

}  // namespace lo
