// lo_matvec.hip -- operator descriptor -> kernel sequence ("op-tree lowering" target), and the public
// lo_matvec_f32 entry point (LinearOperator._matmul of the hot-path classes, lo_amd.h).
#include <algorithm>

#include "lo_internal.h"

namespace lo {

// ---- low-rank + diagonal: y = C (C^T v) + d o v ------------------------------------------------------------------------
static int lowrank_plan(MatvecPlan* pl, Arena* ar, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  LowrankPlan& k = pl->lr;
  if (!op.A0 || op.R < 1) return LO_ERR_BADARG;
  const int R4 = padded_rank(op.R);
  if (R4 > kMaxRank) return LO_ERR_UNSUPPORTED;
  k.R4 = k.lda = R4;
  float* pad = R4 != op.R ? ar->take<float>((size_t)op.B * op.N * R4) : nullptr;
  k.tpart = ar->take<float>((size_t)op.B * pl->sp.S * R4 * pl->c);
  if (ar->measuring()) return LO_OK;
  if (!ar->ok) return LO_ERR_WORKSPACE;
  k.Apad = op.A0;
  if (pad) {
    const int rc = pad_rows(op.A0, (int)op.R, pad, R4, op.B * op.N, st);
    if (rc) return rc;
    k.Apad = pad;
  }
  k.mv_resident = lowrank_mv_eligible(R4, op.N, pl->c);
  return LO_OK;
}

// one pass over C with the rows resident between t = C^T v and y = C t + d o v (lo_lowrank_mv.hip); the fused dot
// partials of the CG iteration and shapes it does not take run the two streaming passes
static int lowrank_run(const MatvecPlan* pl, const float* v, float* y, float* dot_part, const int* stop,
                       hipStream_t st) {
  const lo_op_desc& op = pl->op;
  const LowrankPlan& k = pl->lr;
  if (k.mv_resident && !dot_part) {
    const int rc = lowrank_mv_run(k.Apad, k.R4, op.d, op.diag_mode, v, y, op.B, op.N, pl->c, stop, st);
    if (rc != LO_ERR_UNSUPPORTED) return rc;
  }
  const int rc = skinny_tn(k.Apad, k.lda, k.R4, v, pl->c, k.tpart, op.B, op.N, pl->sp, stop, st);
  if (rc) return rc;
  return skinny_nn(k.Apad, k.lda, k.R4, k.tpart, op.d, op.diag_mode, 1.0f, v, pl->c, y, dot_part, op.B, op.N, pl->sp,
                   stop, st);
}

// ---- dense + diagonal -----------------------------------------------------------------------------------------------------
static int dense_plan(MatvecPlan* pl, Arena* ar, hipStream_t) {
  const lo_op_desc& op = pl->op;
  if (!op.A0) return LO_ERR_BADARG;
  const int ks = dense_mfma_slices(op.B, op.N, pl->c);
  if (ks > 1) pl->dense.part = ar->take<float>((size_t)ks * op.B * op.N * pl->c);
  return LO_OK;
}

static int dense_run(const MatvecPlan* pl, const float* v, float* y, float* dot_part, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  return dense_matvec(op.A0, op.d, op.diag_mode, v, y, dot_part, op.B, op.N, pl->c, dense_rows_per_wg(op.B, op.N),
                      pl->dense.part, stop, st);
}

// ---- Kronecker product of two dense factors + diagonal ---------------------------------------------------------------------
static int kron_plan(MatvecPlan* pl, Arena* ar, hipStream_t) {
  const lo_op_desc& op = pl->op;
  if (!op.A0 || !op.A1 || op.R * op.n2 != op.N) return LO_ERR_BADARG;
  const bool cols = kron_mfma_cols_ok((int)op.R, (int)op.n2, pl->c);
  pl->kron.tmp = ar->take<float>((size_t)op.B * op.N * pl->c * (cols ? 2 : 1));
  return LO_OK;
}

// (the matrix-core route of one column writes the dot partials in its epilogue: kron_fuses_dot)
static bool kron_fuses_dot(const MatvecPlan* pl) { return kron_mfma_ok((int)pl->op.R, (int)pl->op.n2, pl->c); }

static int kron_run(const MatvecPlan* pl, const float* v, float* y, float* dot_part, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  const int n1 = (int)op.R, n2 = (int)op.n2;
  float* tmp = pl->kron.tmp;
  if (kron_fuses_dot(pl))
    return kron_matvec_mfma(op.A0, op.A1, op.d, op.diag_mode, v, tmp, y, dot_part, op.B, n1, n2, stop, st);
  if (kron_mfma_cols_ok(n1, n2, pl->c))  // (the diagonal rides on the way back of the columns)
    return kron_matvec_mfma_cols(op.A0, op.A1, op.d, op.diag_mode, v, tmp, tmp + (size_t)op.B * op.N * pl->c, y, op.B,
                                 n1, n2, pl->c, stop, st);
  const int rc = kron_matvec(op.A0, op.A1, v, tmp, y, op.B, n1, n2, pl->c, stop, st);
  if (rc) return rc;
  return vec_add_diag(op.d, op.diag_mode, v, y, pl->c, op.B, op.N, pl->sp, stop, st);
}

// ---- sum of plain terms + one diagonal --------------------------------------------------------------------------------------
// sum(op._matmul(rhs) for op in linear_ops), left to right (sum_linear_operator.py:47-51)
static int sum_plan(MatvecPlan* pl, Arena* ar, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  if (op.nterms < 2 || op.nterms > LO_MAX_TERMS || !op.terms) return LO_ERR_BADARG;
  for (int i = 0; i < op.nterms; ++i) {
    const lo_op_desc& t = op.terms[i];
    if (!(plain_term_kind(t.kind) || kernel_term_kind(t.kind)) || t.diag_mode != LO_DIAG_NONE || t.B != op.B || t.N != op.N) return LO_ERR_BADARG;
  }
  pl->sum.ytmp = ar->take<float>((size_t)op.B * op.N * pl->c);
  MatvecPlan scratch;  // (a measuring pass keeps no sub-plans)
  if (!ar->measuring()) {
    pl->sub = new MatvecPlan[op.nterms]();
    pl->nterms = op.nterms;
  }
  for (int i = 0; i < op.nterms; ++i) {
    lo_op_desc t = op.terms[i];
    if (i == 0) {  // the tree's one diagonal rides on the first term's epilogue
      t.diag_mode = op.diag_mode;
      t.d = op.d;
    }
    const int rc = matvec_plan_init(pl->sub ? &pl->sub[i] : &scratch, &t, nullptr, nullptr, pl->c, pl->sp, ar, st);
    if (rc) return rc;
  }
  return LO_OK;
}

static int sum_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st) {
  int rc = matvec_run(&pl->sub[0], v, y, nullptr, stop, st);
  for (int i = 1; i < pl->nterms && !rc; ++i) {
    rc = matvec_run(&pl->sub[i], v, pl->sum.ytmp, nullptr, stop, st);
    if (!rc) rc = vec_axpy1(y, pl->sum.ytmp, (size_t)pl->op.B * pl->op.N * pl->c, stop, st);
  }
  return rc;
}

// ---- the plan of any kind -------------------------------------------------------------------------------------------------
// (the dense and Kronecker kernels write one partial per tile of their own; every other kind one per row block)
int matvec_S_dot(const lo_op_desc* op, int64_t c, Split sp) {
  if (op->kind == LO_OP_DENSE_DIAG) return dense_S_dot(op->B, op->N, c);
  if (op->kind == LO_OP_KRON_DIAG) return kron_S_dot((int)op->R, (int)op->n2, c, sp.S);
  return sp.S;
}

int matvec_plan_init(MatvecPlan* pl, const lo_op_desc* op, lo_matvec_cb cb, void* cb_user, int64_t c, Split sp,
                     Arena* ar, hipStream_t st) {
  *pl = MatvecPlan();
  pl->op = *op;
  pl->c = c;
  pl->sp = sp;
  pl->cb = cb;
  pl->cb_user = cb_user;
  if (op->B < 1 || op->N < 1 || c < 1) return LO_ERR_BADARG;
  if (op->diag_mode != LO_DIAG_NONE && !op->d) return LO_ERR_BADARG;
  pl->S_dot = matvec_S_dot(op, c, sp);
  int rc = LO_ERR_BADARG;
  switch (op->kind) {
    case LO_OP_LOWRANK_DIAG: rc = lowrank_plan(pl, ar, st); break;
    case LO_OP_DENSE_DIAG: rc = dense_plan(pl, ar, st); break;
    case LO_OP_KRON_DIAG: rc = kron_plan(pl, ar, st); break;
    case LO_OP_SKI_DIAG:
    case LO_OP_TOEPLITZ_DIAG: rc = ski_plan(pl, ar, st); break;
    case LO_OP_SKI_GRID_DIAG: rc = ski_grid_plan(pl, ar, st); break;
    case LO_OP_SKI_SUM_DIAG: rc = ski_sum_plan(pl, ar, st); break;
    case LO_OP_TOEPLITZ_KRON_DIAG: rc = toeplitz_kron_plan(pl, ar, st); break;
    case LO_OP_HADAMARD_DIAG: rc = hadamard_plan(pl, ar, st); break;
    case LO_OP_KERNEL_DIAG: rc = kernel_op_plan(pl, ar, st); break;
    case LO_OP_KERNEL_SUM_DIAG: rc = kernel_sum_plan(pl, ar, st); break;
    case LO_OP_KERNEL_KRON_DIAG: rc = kernel_kron_plan(pl, ar, st); break;
    case LO_OP_KERNEL_LMC_DIAG: rc = kernel_lmc_plan(pl, ar, st); break;
    case LO_OP_KERNEL_GRAD_DIAG: rc = kernel_grad_plan(pl, ar, st); break;
    case LO_OP_KERNEL_TASK_DIAG: rc = kernel_task_plan(pl, ar, st); break;
    case LO_OP_KERNEL_PARAM_DIAG: rc = kernel_param_plan(pl, ar, st); break;
    case LO_OP_KERNEL_SM_DIAG: rc = kernel_sm_plan(pl, ar, st); break;
    case LO_OP_MASKED: rc = masked_plan(pl, ar, st); break;
    case LO_OP_CALLBACK: rc = cb ? LO_OK : LO_ERR_BADARG; break;
    case LO_OP_SUM: rc = sum_plan(pl, ar, st); break;
  }
  if (!rc && !ar->ok) rc = LO_ERR_WORKSPACE;
  if (rc) matvec_plan_free(pl);
  return rc;
}

size_t matvec_plan_bytes(const lo_op_desc* op, int64_t c, Split sp) {
  MatvecPlan scratch;  // (an invalid descriptor: what it took before it was refused)
  return measured(kPlanTail, [&](Arena& ar) { matvec_plan_init(&scratch, op, nullptr, nullptr, c, sp, &ar, nullptr); });
}

void matvec_plan_free(MatvecPlan* pl) {
  if (pl->sub) {
    for (int i = 0; i < pl->nterms; ++i) matvec_plan_free(&pl->sub[i]);
    delete[] pl->sub;
    pl->sub = nullptr;
  }
}

int matvec_run(const MatvecPlan* pl, const float* v, float* y, float* dot_part, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  bool fused = false;  // the kind's own kernels write dot_part
  int rc = LO_ERR_BADARG;
  switch (op.kind) {
    case LO_OP_LOWRANK_DIAG: fused = true; rc = lowrank_run(pl, v, y, dot_part, stop, st); break;
    case LO_OP_DENSE_DIAG: fused = true; rc = dense_run(pl, v, y, dot_part, stop, st); break;
    case LO_OP_KRON_DIAG: fused = kron_fuses_dot(pl); rc = kron_run(pl, v, y, dot_part, stop, st); break;
    case LO_OP_SKI_DIAG:  // W_l T W_r^T v + d o v: segmented gather over the grid-major W_r, Toeplitz product, gather
    case LO_OP_TOEPLITZ_DIAG: rc = ski_matvec_run(pl, v, y, stop, st); break;
    case LO_OP_SKI_GRID_DIAG:  // W_l (T_1 (x) .. (x) T_D) W_r^T v + d o v: the same with one pass per grid axis
      rc = ski_grid_matvec_run(pl, v, y, stop, st); break;
    case LO_OP_SKI_SUM_DIAG:  // sum_p W_l,p T_p W_r,p^T v + d o v: the SKI passes over B P grid members, one summing gather
      rc = ski_sum_matvec_run(pl, v, y, stop, st); break;
    case LO_OP_TOEPLITZ_KRON_DIAG:  // (T_1 (x) .. (x) T_D) v + d o v: one pass per grid axis, the diagonal in the last
      rc = toeplitz_kron_matvec_run(pl, v, y, stop, st); break;
    case LO_OP_HADAMARD_DIAG:  // (F F^T o G G^T) v + d o v: contraction M_t = F^T diag(v_t) G, expansion rowdot(F, G M_t^T)
      rc = hadamard_matvec_run(pl, v, y, stop, st); break;
    case LO_OP_KERNEL_DIAG:  // K(X, X) v + d o v, K formed tile by tile from X (lo_kernel_op.hip)
      rc = kernel_op_matvec_run(pl, v, y, stop, st); break;
    case LO_OP_KERNEL_SUM_DIAG:  // (sum_t K_t(X, X)) v + d o v in one pass over the pairs (lo_kernel_sum.hip)
      rc = kernel_sum_matvec_run(pl, v, y, stop, st); break;
    case LO_OP_KERNEL_KRON_DIAG:  // (K(X, X) (x) Bt) v + d o v, Bt applied while the tile of v is staged (lo_kernel_kron.hip)
      rc = kernel_kron_matvec_run(pl, v, y, stop, st); break;
    case LO_OP_KERNEL_LMC_DIAG:  // (sum_q K_q(X, X) (x) B_q) v + d o v, every B_q v formed while the tile of v is staged (lo_kernel_lmc.hip)
      rc = kernel_lmc_matvec_run(pl, v, y, stop, st); break;
    case LO_OP_KERNEL_GRAD_DIAG:  // the RBF gradient kernel's blocks formed pair by pair, D + 1 outputs per point (lo_kernel_grad.hip)
      rc = kernel_grad_matvec_run(pl, v, y, stop, st); break;
    case LO_OP_KERNEL_TASK_DIAG:  // K_ij = os2 g(r_ij) Bt[t_i, t_j], the task ids staged with the points (lo_kernel_task.hip)
      rc = kernel_task_matvec_run(pl, v, y, stop, st); break;
    case LO_OP_KERNEL_PARAM_DIAG:  // K_ij = os2 g(x_i, x_j), g rational quadratic or periodic (lo_kernel_param.hip)
      rc = kernel_param_matvec_run(pl, v, y, stop, st); break;
    case LO_OP_KERNEL_SM_DIAG:  // K_ij = sum_q w_q E_q(tau) prod_k cos(2 pi mu_qk tau_k), the spectral mixture (lo_kernel_sm.hip)
      rc = kernel_sm_matvec_run(pl, v, y, stop, st); break;
    case LO_OP_MASKED:  // S (base) S^T v + d o v: expand, the base's product (or the selected rows of a dense base), gather
      rc = masked_matvec_run(pl, v, y, stop, st); break;
    case LO_OP_CALLBACK: rc = pl->cb(pl->cb_user, v, y, op.B, op.N, pl->c, (void*)st) ? LO_ERR_LAUNCH : LO_OK; break;
    case LO_OP_SUM: rc = sum_run(pl, v, y, stop, st); break;
  }
  // the shared epilogue: the dot partials of a kind whose kernels do not write them
  if (!rc && dot_part && !fused) rc = vec_dot_part(v, y, pl->c, dot_part, op.B, op.N, pl->sp, stop, st);
  return rc;
}

bool matvec_can_fuse_pupdate(const MatvecPlan* pl) { return pl->op.kind == LO_OP_LOWRANK_DIAG; }

int matvec_run_pupdate(const MatvecPlan* pl, float* p, const float* z, const float* beta, int first, float* y,
                       float* dot_part, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  if (op.kind != LO_OP_LOWRANK_DIAG) return LO_ERR_BADARG;
  const LowrankPlan& k = pl->lr;
  int rc = skinny_tn_pupdate(k.Apad, k.lda, k.R4, p, z, beta, first, pl->c, k.tpart, op.B, op.N, pl->sp, stop, st);
  if (rc) return rc;
  return skinny_nn(k.Apad, k.lda, k.R4, k.tpart, op.d, op.diag_mode, 1.0f, p, pl->c, y, dot_part, op.B, op.N, pl->sp,
                   stop, st);
}

}  // namespace lo

using namespace lo;

extern "C" {

int lo_abi_version(void) { return 40; }
const char* lo_target_arch(void) { return "gfx950"; }

size_t lo_matvec_workspace_bytes(const lo_op_desc* op, int64_t c) {
  if (!op) return 0;
  Split sp = choose_split(op->B, op->N, 256);
  return matvec_plan_bytes(op, c, sp);
}

int lo_matvec_f32(const lo_op_desc* op, const float* v, float* y, int64_t c, void* ws, size_t ws_bytes, void* stream) {
  if (!op || !v || !y || op->kind == LO_OP_CALLBACK) return LO_ERR_BADARG;
  hipStream_t st = (hipStream_t)stream;
  Split sp = choose_split(op->B, op->N, 256);
  if (op->kind == LO_OP_LOWRANK_DIAG) resident_tick();  // (an entry point that may run a resident kernel: serves the cool-down)
  // A plan may launch while it is built (the padded copy of C, the copy of W_r, a mask's inverse map): the measuring
  // pass validates the descriptor, and a short workspace is refused before anything is launched, for every kind.
  MatvecPlan pl;
  Arena need(nullptr, 0);
  int rc = matvec_plan_init(&pl, op, nullptr, nullptr, c, sp, &need, st);
  if (rc) return rc;
  if (!ws || ws_bytes < need.off + kPlanTail) return LO_ERR_WORKSPACE;
  Arena ar(ws, ws_bytes);
  rc = matvec_plan_init(&pl, op, nullptr, nullptr, c, sp, &ar, st);
  if (rc) return rc;
  rc = matvec_run(&pl, v, y, nullptr, nullptr, st);
  matvec_plan_free(&pl);
  return rc;
}

}  // extern "C"
