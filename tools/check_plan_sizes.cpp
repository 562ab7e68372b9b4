// check_plan_sizes.cpp -- host-only walk of the matvec plan layer's sizing paths for a sanitizer build.
//
// The descriptor table of tests/matvec_plan_cases.py (every kind, one and three columns) and one refused descriptor per
// kind go through lo_matvec_workspace_bytes, lo_cg_workspace_bytes, lo_minres_workspace_bytes and
// lo_lanczos_workspace_bytes.  The sizing passes run the plan functions on a measuring arena: they must read no device
// pointer (the ones here are dummy addresses), keep no sub-plan (a leak report) and touch nothing out of bounds.  No GPU.
// The solver sizers are also walked with Woodbury preconditioners (the padded copy of Q taken and not taken, the root
// form alone), and the sizers of the other entry points with shapes of tests/workspace_cases.py, the five float64 sizers
// (csrc/lo_*_f64.hip) among them.  The compile-time
// pickers of the matrix-free kernel family (csrc/lo_kernel_shape.h) are held to what the switches they replaced chose.
// Last, refused descriptors of every kind go through lo_pivoted_cholesky_f32 / _f64 and lo_matvec_f32, which share one
// descriptor check per kind (the *_desc_check functions of csrc/lo_internal.h): the return codes are pinned.
//
//   cd linear_operator_amd/csrc && mkdir -p build_asan
//   for f in *.hip; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -Xarch_host -fsanitize=address,undefined \
//       -c $f -o build_asan/${f%.hip}.o; done
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -c ../../tools/check_plan_sizes.cpp -o build_asan/check_plan_sizes.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined build_asan/*.o -o build_asan/check_plan_sizes \
//       && build_asan/check_plan_sizes
// (the program is compiled to an object of its own: on one line with the objects, hipcc reads them as HIP source)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/lo_amd.h"
#include "../linear_operator_amd/csrc/lo_kernel_shape.h"

static const float* F(uintptr_t a) { return reinterpret_cast<const float*>(a); }
static const int64_t* I(uintptr_t a) { return reinterpret_cast<const int64_t*>(a); }

static lo_op_desc desc(int kind, int64_t B, int64_t N, int64_t R, int64_t n2, bool a1, int diag_mode) {
  lo_op_desc d;
  memset(&d, 0, sizeof(d));
  d.kind = kind; d.diag_mode = diag_mode; d.B = B; d.N = N; d.R = R; d.n2 = n2;
  d.A0 = F(0x10000);
  d.A1 = a1 ? F(0x20000) : nullptr;
  d.d = diag_mode != LO_DIAG_NONE ? F(0x30000) : nullptr;
  return d;
}

struct Entry {
  const char* name;
  lo_op_desc op;
  bool valid;
};

static int walk(const std::vector<Entry>& table) {
  int bad = 0;
  for (const Entry& e : table) {
    for (int64_t c : {1, 3}) {
      lo_cg_params cg;
      memset(&cg, 0, sizeof(cg));
      cg.c = c; cg.max_iter = 5; cg.max_tridiag_iter = 20; cg.tolerance = 1e-4f; cg.eps = 1e-10f;
      lo_minres_params mr;
      memset(&mr, 0, sizeof(mr));
      mr.c = c; mr.n_shifts = 2; mr.max_iter = 3;
      const size_t mv = lo_matvec_workspace_bytes(&e.op, c);
      const size_t a = lo_cg_workspace_bytes(&e.op, nullptr, &cg);
      const size_t b = lo_minres_workspace_bytes(&e.op, nullptr, &mr);
      const size_t l = lo_lanczos_workspace_bytes(&e.op, c, 4);
      printf("%-22s c=%lld matvec %zu cg %zu minres %zu lanczos %zu\n", e.name, (long long)c, mv, a, b, l);
      if (!e.valid && mv > 256) {
        printf("  a refused descriptor took buffers\n");
        ++bad;
      }
      if (mv < 256 || a < mv || b < mv || l < mv) {
        printf("  a size does not cover the plan\n");
        ++bad;
      }
    }
  }
  return bad;
}

// lo_precond_apply_workspace_bytes and the CG / MINRES sizers over the same descriptors: PrecondPlan on a measuring arena
static int walk_precond(const lo_op_desc& op) {
  int bad = 0;
  const int64_t shapes[2][3] = {{1, 37, 1}, {3, 300, 3}};
  for (const auto& sh : shapes)
    for (int k : {4, 5, 8, 33}) {
      int R4 = 4;
      while (R4 < k) R4 *= 2;
      const size_t got = lo_precond_apply_workspace_bytes(sh[0], sh[1], k, sh[2]);
      const size_t copy = k != R4 ? sizeof(float) * sh[0] * sh[1] * R4 : 0, upart = sizeof(float) * sh[0] * R4 * sh[2];
      printf("precond_apply B=%lld N=%lld k=%d c=%lld: %zu\n", (long long)sh[0], (long long)sh[1], k, (long long)sh[2], got);
      if (got < copy + upart || got > copy + upart * 256 + 2048) {  // (at most 256 row blocks, two alignments, the tail)
        printf("  the size does not match the plan's takes\n");
        ++bad;
      }
    }
  lo_cg_params cg;
  memset(&cg, 0, sizeof(cg));
  cg.c = 3; cg.max_iter = 5; cg.max_tridiag_iter = 20; cg.tolerance = 1e-4f; cg.eps = 1e-10f;
  lo_minres_params mr;
  memset(&mr, 0, sizeof(mr));
  mr.c = 3; mr.n_shifts = 2; mr.max_iter = 3;
  lo_precond_desc pre;
  memset(&pre, 0, sizeof(pre));
  pre.k = 5; pre.dinv = F(0x80000);
  const size_t none_cg = lo_cg_workspace_bytes(&op, nullptr, &cg), none_mr = lo_minres_workspace_bytes(&op, nullptr, &mr);
  const size_t copy = sizeof(float) * op.B * op.N * 8;
  pre.ldq = 8; pre.Q = F(0x90000);  // rows padded already: upart only
  const size_t a8 = lo_cg_workspace_bytes(&op, &pre, &cg), b8 = lo_minres_workspace_bytes(&op, &pre, &mr);
  pre.ldq = 5;                      // unpadded rows: the copy as well
  const size_t a5 = lo_cg_workspace_bytes(&op, &pre, &cg), b5 = lo_minres_workspace_bytes(&op, &pre, &mr);
  pre.Q = nullptr; pre.F = pre.EF = F(0xa0000); pre.rf_ld = 8;  // root form only: no copy
  const size_t ar = lo_cg_workspace_bytes(&op, &pre, &cg);
  printf("woodbury k=5: cg %zu / %zu / root only %zu (none %zu), minres %zu / %zu (none %zu)\n", a8, a5, ar, none_cg, b8, b5,
         none_mr);
  if (a5 < a8 + copy || b5 < b8 + copy || ar >= a8 + copy) {
    printf("  the padded copy of Q is not counted where it is taken\n");
    ++bad;
  }
  return bad;
}

// the sizers of the entry points that lay their own workspace out (rows of tests/workspace_cases.py; 0 = refused)
static int walk_entries() {
  const size_t got[] = {
      lo_precond_build_workspace_bytes(2, 37, 5),           lo_precond_build_workspace_bytes(3, 300, 33),
      lo_precond_root_form_workspace_bytes(2, 37, 5),       lo_precond_root_form_rs_workspace_bytes(2, 37, 8),
      lo_precond_kron_root_workspace_bytes(3),              lo_bilinear_root_workspace_bytes(2, 37, 5, 3),
      lo_bilinear_kron_workspace_bytes(2, 3, 5, 3),         lo_probe_vectors_workspace_bytes(3, 300, 4),
      lo_hadamard_bilinear_workspace_bytes(2, 37, 3, 2, 1), lo_cholesky_workspace_bytes(2, 37),
      lo_tridiag_eigh_slq_workspace_bytes(3, 2)};
  int bad = 0;
  for (size_t g : got) {
    printf("entry sizer: %zu\n", g);
    if (g < 256) ++bad;
  }
  if (lo_hadamard_bilinear_workspace_bytes(2, 37, 0, 2, 1) != 0 || lo_cholesky_workspace_bytes(2, 1025) != 0) {
    printf("  a refused shape was sized\n");
    ++bad;
  }
  return bad;
}

// The float64 sizers over F64_SHAPES of tests/workspace_cases.py: each covers the plain sum of its buffers and, with at most
// 41 takes aligned to 256 bytes and the tail of 1024, no more than that plus 12 KiB; one refused or degenerate argument
// set each.  lo_matvec_f64_workspace_bytes reads the descriptor only (dummy pointers), a sum takes its largest term.
static int walk_f64() {
  int bad = 0;
  auto held = [&](const char* what, size_t got, size_t needed) {
    printf("%s: %zu (buffers %zu)\n", what, got, needed);
    if (got < needed || got > needed + 12288) {
      printf("  the size does not match the layout's takes\n");
      ++bad;
    }
  };
  const int64_t shapes[3][3] = {{1, 1, 1}, {3, 37, 3}, {2, 300, 17}};
  for (const auto& sh : shapes) {
    const size_t B = sh[0], N = sh[1], c = sh[2], V = 8 * B * N * c, S = 8 * B * c;
    lo_cg_params_f64 cg;
    memset(&cg, 0, sizeof(cg));
    cg.c = c; cg.max_iter = 20; cg.max_tridiag_iter = 20;
    held("cg_f64", lo_cg_f64_workspace_bytes(B, N, &cg), 40 + 6 * V + 10 * S + 2 * 4 * B * c);
    for (int Q : {1, 3}) {
      lo_minres_params_f64 mr;
      memset(&mr, 0, sizeof(mr));
      mr.c = c; mr.n_shifts = Q; mr.max_iter = 20;
      held("minres_f64", lo_minres_f64_workspace_bytes(B, N, &mr), 24 + (6 + 3 * Q) * V + (6 + 11 * Q) * S + 4 * B * c);
    }
    for (int m : {1, 20}) held("lanczos_f64", lo_lanczos_f64_workspace_bytes(B, N, c, m), 2 * V + (m + 2) * S + 16);
    for (int k : {4, 33}) held("precond_f64", lo_precond_f64_workspace_bytes(B, N, k, c), k * S * ((N + 255) / 256 + 1));
    lo_op_desc lr = desc(LO_OP_LOWRANK_DIAG, B, N, 5, 0, false, LO_DIAG_FULL);
    lo_op_desc dn = desc(LO_OP_DENSE_DIAG, B, N, 0, 0, false, LO_DIAG_FULL);
    lo_op_desc kr = desc(LO_OP_KRON_DIAG, B, N, 1, N, true, LO_DIAG_CONST);
    lo_op_desc terms[3] = {lr, dn, kr};
    for (lo_op_desc& t : terms) { t.diag_mode = LO_DIAG_NONE; t.d = nullptr; }
    lo_op_desc sum = desc(LO_OP_SUM, B, N, 0, 0, false, LO_DIAG_FULL);
    sum.A0 = nullptr; sum.nterms = 3; sum.terms = terms;
    const size_t need_lr = 5 * S * ((N + 255) / 256 + 1), need_kr = V;
    held("matvec_f64 lowrank", lo_matvec_f64_workspace_bytes(&lr, c), need_lr);
    held("matvec_f64 dense", lo_matvec_f64_workspace_bytes(&dn, c), 0);
    held("matvec_f64 kron", lo_matvec_f64_workspace_bytes(&kr, c), need_kr);
    held("matvec_f64 sum", lo_matvec_f64_workspace_bytes(&sum, c), need_lr > need_kr ? need_lr : need_kr);
    sum.nterms = 1;  // refused: no size
    if (lo_matvec_f64_workspace_bytes(&sum, c) != 0 || lo_matvec_f64_workspace_bytes(&lr, 0) != 0 ||
        lo_matvec_f64_workspace_bytes(nullptr, c) != 0 || lo_precond_f64_workspace_bytes(B, N, 0, c) != 0) {
      printf("  a refused float64 argument set was sized\n");
      ++bad;
    }
  }
  // degenerate arguments the solver sizers take as they come (their entry points refuse): the tail alone, no read
  lo_cg_params_f64 cg0;
  memset(&cg0, 0, sizeof(cg0));
  lo_minres_params_f64 mr0;
  memset(&mr0, 0, sizeof(mr0));
  held("cg_f64 B=0", lo_cg_f64_workspace_bytes(0, 37, &cg0), 40);
  held("minres_f64 c=0", lo_minres_f64_workspace_bytes(3, 37, &mr0), 24);
  held("lanczos_f64 N=0", lo_lanczos_f64_workspace_bytes(3, 0, 3, 20), 8 * (20 + 2) * 9 + 16);
  return bad;
}

// The compile-time pickers of csrc/lo_kernel_shape.h, which choose a kernel instantiation of the matrix-free kernel family
// from run-time values: for every value of a list, one below, one between (where there is one) and one above, the constant
// that ko_pick hands on must be the one the `switch` it replaced chose -- the matching `case`, else the `default:` arm.
// The expectations are written out.
template <class Seq>
static int picked(Seq seq, int v) {
  int got = -1;
  lo::ko_pick(seq, v, [&](auto c) { got = c(); });
  return got;
}

static int walk_pickers() {
  using namespace lo;
  struct Pick {
    const char* list;
    int v, got, want;
  };
  const Pick picks[] = {
      // family: case RBF / MATERN12 / MATERN32, default MATERN52
      {"families", -1, picked(ko_families{}, -1), 3}, {"families", 0, picked(ko_families{}, 0), 0},
      {"families", 1, picked(ko_families{}, 1), 1},   {"families", 2, picked(ko_families{}, 2), 2},
      {"families", 3, picked(ko_families{}, 3), 3},   {"families", 4, picked(ko_families{}, 4), 3},
      // padded dimension: case 4 / 8 / 16, default 32
      {"dims", 3, picked(ko_dims{}, 3), 32},   {"dims", 4, picked(ko_dims{}, 4), 4},    {"dims", 6, picked(ko_dims{}, 6), 32},
      {"dims", 8, picked(ko_dims{}, 8), 8},    {"dims", 12, picked(ko_dims{}, 12), 32}, {"dims", 16, picked(ko_dims{}, 16), 16},
      {"dims", 24, picked(ko_dims{}, 24), 32}, {"dims", 32, picked(ko_dims{}, 32), 32}, {"dims", 33, picked(ko_dims{}, 33), 32},
      // columns of the single-term and task products: case 1 / 4, default 16
      {"cols", 0, picked(ko_cols{}, 0), 16},   {"cols", 1, picked(ko_cols{}, 1), 1},   {"cols", 2, picked(ko_cols{}, 2), 16},
      {"cols", 4, picked(ko_cols{}, 4), 4},    {"cols", 8, picked(ko_cols{}, 8), 16},  {"cols", 16, picked(ko_cols{}, 16), 16},
      {"cols", 17, picked(ko_cols{}, 17), 16},
      // wide columns of the Kronecker product: case 4 / 16, default 32
      {"kron cols", 3, picked(kk_cols{}, 3), 32},   {"kron cols", 4, picked(kk_cols{}, 4), 4},
      {"kron cols", 8, picked(kk_cols{}, 8), 32},   {"kron cols", 16, picked(kk_cols{}, 16), 16},
      {"kron cols", 24, picked(kk_cols{}, 24), 32}, {"kron cols", 32, picked(kk_cols{}, 32), 32},
      {"kron cols", 33, picked(kk_cols{}, 33), 32},
      // float64 columns: CC == 1, CC == 4, else 8 below DP 32 (at DP 32 the old code launched nothing for a third value,
      // which ko64_col_chunk never yields there: the list ends at 4)
      {"f64 cols", 0, picked(ko64_cols<16>{}, 0), 8},   {"f64 cols", 1, picked(ko64_cols<16>{}, 1), 1},
      {"f64 cols", 2, picked(ko64_cols<16>{}, 2), 8},   {"f64 cols", 4, picked(ko64_cols<16>{}, 4), 4},
      {"f64 cols", 6, picked(ko64_cols<16>{}, 6), 8},   {"f64 cols", 8, picked(ko64_cols<16>{}, 8), 8},
      {"f64 cols", 9, picked(ko64_cols<16>{}, 9), 8},   {"f64 cols DP 32", 1, picked(ko64_cols<32>{}, 1), 1},
      {"f64 cols DP 32", 4, picked(ko64_cols<32>{}, 4), 4},
      // gradient kernel, padded dimension: case 4 / 8, default 16
      {"grad dims", 3, picked(kg_dims{}, 3), 16},   {"grad dims", 4, picked(kg_dims{}, 4), 4},
      {"grad dims", 6, picked(kg_dims{}, 6), 16},   {"grad dims", 8, picked(kg_dims{}, 8), 8},
      {"grad dims", 12, picked(kg_dims{}, 12), 16}, {"grad dims", 16, picked(kg_dims{}, 16), 16},
      {"grad dims", 32, picked(kg_dims{}, 32), 16},
      // gradient kernel, columns: CC == 4 at DP 4, CC == 2 up to DP 8, else 1
      {"grad cols DP 4", 0, picked(kg_cols<4>{}, 0), 1},   {"grad cols DP 4", 1, picked(kg_cols<4>{}, 1), 1},
      {"grad cols DP 4", 2, picked(kg_cols<4>{}, 2), 2},   {"grad cols DP 4", 3, picked(kg_cols<4>{}, 3), 1},
      {"grad cols DP 4", 4, picked(kg_cols<4>{}, 4), 4},   {"grad cols DP 4", 5, picked(kg_cols<4>{}, 5), 1},
      {"grad cols DP 8", 0, picked(kg_cols<8>{}, 0), 1},   {"grad cols DP 8", 1, picked(kg_cols<8>{}, 1), 1},
      {"grad cols DP 8", 2, picked(kg_cols<8>{}, 2), 2},   {"grad cols DP 8", 4, picked(kg_cols<8>{}, 4), 1},
      {"grad cols DP 16", 1, picked(kg_cols<16>{}, 1), 1}, {"grad cols DP 16", 2, picked(kg_cols<16>{}, 2), 1},
  };
  int bad = 0;
  for (const Pick& p : picks)
    if (p.got != p.want) {
      printf("picker %s: %d chose %d, the switch chose %d\n", p.list, p.v, p.got, p.want);
      ++bad;
    }
  // the chunk functions yield members of their lists only, so the `default:` arm is never an unlisted width
  for (int64_t c = 1; c <= 40; ++c) {
    for (int DP : {4, 8, 16, 32}) {
      if (picked(ko_cols{}, ko_col_chunk(c)) != ko_col_chunk(c) || picked(kk_cols{}, kk_col_chunk(c)) != kk_col_chunk(c)) ++bad;
      const int c64 = ko64_col_chunk(c, DP);
      if ((DP == 32 ? picked(ko64_cols<32>{}, c64) : picked(ko64_cols<16>{}, c64)) != c64) ++bad;
      const int cg = kg_col_chunk(DP, c);
      if (DP <= 16 && (DP == 4 ? picked(kg_cols<4>{}, cg) : DP == 8 ? picked(kg_cols<8>{}, cg) : picked(kg_cols<16>{}, cg)) != cg)
        ++bad;
    }
  }
  // the dispatcher hands the three constants on together
  int seen[3] = {-1, -1, -1};
  ko_dispatch(LO_KERNEL_MATERN32, 8, kk_cols{}, 16, [&](auto f, auto p, auto c) {
    seen[0] = f();
    seen[1] = p();
    seen[2] = c();
  });
  if (seen[0] != LO_KERNEL_MATERN32 || seen[1] != 8 || seen[2] != 16) ++bad;
  printf("pickers: %zu choices checked, %d wrong\n", sizeof(picks) / sizeof(picks[0]), bad);
  return bad;
}

// The return codes of refused descriptors at the entry points that share the kinds' *_desc_check functions: the pivoted
// Cholesky (both precisions), which validates without a plan, and lo_matvec_f32, whose measuring pass runs the plan
// function.  Every entry returns before anything touches the device: from the descriptor check, or -- the rows marked
// "taken", the descriptors one side accepts and the other refuses -- at the empty workspace (LO_ERR_WORKSPACE, -3), which
// every entry tests before its first launch.  A "taken" row must be of a kind that no resident engine takes (SKI, kernel,
// a sum: pc_onchip_eligible and pc_onchip_rows_eligible are false), never low-rank, dense or Kronecker.  `want`: the codes of the sources before the checks were shared (ABI 37).
struct Refused {
  const char* name;
  lo_op_desc op;
  int want[3];  // lo_pivoted_cholesky_f32, lo_pivoted_cholesky_f64, lo_matvec_f32
};

static int walk_refused(const std::vector<Refused>& table) {
  int bad = 0;
  static char ws[256];  // a non-null workspace of no bytes
  int64_t perm[1];
  int32_t rank = 0;
  float Lf[1], v[1] = {0}, y[1];
  double Ld[1];
  for (const Refused& r : table) {
    const int got[3] = {lo_pivoted_cholesky_f32(&r.op, 4, 1e-3f, Lf, perm, &rank, ws, 0, nullptr),
                        lo_pivoted_cholesky_f64(&r.op, 4, 1e-3, Ld, perm, &rank, ws, 0, nullptr),
                        lo_matvec_f32(&r.op, v, y, 1, nullptr, 0, nullptr)};
    printf("refused %-34s pivchol_f32 %d pivchol_f64 %d matvec %d\n", r.name, got[0], got[1], got[2]);
    for (int k = 0; k < 3; ++k)
      if (got[k] != r.want[k] || got[k] == LO_OK) {
        printf("  entry %d returned %d, expected %d\n", k, got[k], r.want[k]);
        ++bad;
      }
  }
  return bad;
}

int main() {
  std::vector<Entry> t;
  t.push_back({"lowrank_r5", desc(LO_OP_LOWRANK_DIAG, 2, 300, 5, 0, false, LO_DIAG_FULL), true});
  t.push_back({"lowrank_r8", desc(LO_OP_LOWRANK_DIAG, 2, 300, 8, 0, false, LO_DIAG_CONST), true});
  t.push_back({"dense_splitk", desc(LO_OP_DENSE_DIAG, 1, 1024, 0, 0, false, LO_DIAG_FULL), true});
  t.push_back({"dense_plain", desc(LO_OP_DENSE_DIAG, 2, 100, 0, 0, false, LO_DIAG_FULL), true});
  t.push_back({"kron_3x5", desc(LO_OP_KRON_DIAG, 2, 15, 3, 5, true, LO_DIAG_FULL), true});
  t.push_back({"kron_128", desc(LO_OP_KRON_DIAG, 1, 16384, 128, 128, true, LO_DIAG_FULL), true});
  t.push_back({"toeplitz_33", desc(LO_OP_TOEPLITZ_DIAG, 2, 33, 33, 0, false, LO_DIAG_FULL), true});

  lo_interp_desc w, wp, g2, g3;
  memset(&w, 0, sizeof(w));
  w.left_idx = w.right_idx = I(0x40000);
  w.left_vals = w.right_vals = F(0x50000);
  wp = g2 = g3 = w;
  wp.right_plan = F(0x60000);
  g2.grid_ndim = 2; g2.grid_m[0] = 5; g2.grid_m[1] = 7;
  g3.grid_ndim = 3; g3.grid_m[0] = 3; g3.grid_m[1] = 4; g3.grid_m[2] = 5;
  lo_op_desc ski = desc(LO_OP_SKI_DIAG, 2, 50, 20, 4, false, LO_DIAG_FULL), ski_p = ski;
  ski.interp = &w;
  ski_p.interp = &wp;
  lo_op_desc grid2 = desc(LO_OP_SKI_GRID_DIAG, 2, 50, 35, 4, false, LO_DIAG_FULL);
  grid2.interp = &g2;
  lo_op_desc grid3 = desc(LO_OP_SKI_GRID_DIAG, 2, 50, 60, 8, false, LO_DIAG_FULL);
  grid3.interp = &g3;
  t.push_back({"ski", ski, true});
  t.push_back({"ski_plan", ski_p, true});
  t.push_back({"ski_grid_2d", grid2, true});
  t.push_back({"ski_grid_3d", grid3, true});
  t.push_back({"hadamard", desc(LO_OP_HADAMARD_DIAG, 2, 70, 3, 2, true, LO_DIAG_FULL), true});

  lo_op_desc terms2[2] = {desc(LO_OP_LOWRANK_DIAG, 2, 80, 5, 0, false, LO_DIAG_NONE),
                          desc(LO_OP_DENSE_DIAG, 2, 80, 0, 0, false, LO_DIAG_NONE)};
  lo_op_desc terms3[3] = {terms2[0], terms2[1], desc(LO_OP_KRON_DIAG, 2, 80, 8, 10, true, LO_DIAG_NONE)};
  lo_op_desc sum2 = desc(LO_OP_SUM, 2, 80, 0, 0, false, LO_DIAG_FULL), sum3 = sum2;
  sum2.A0 = sum3.A0 = nullptr;
  sum2.nterms = 2; sum2.terms = terms2;
  sum3.nterms = 3; sum3.terms = terms3;
  lo_op_desc base_dense = desc(LO_OP_DENSE_DIAG, 2, 90, 0, 0, false, LO_DIAG_FULL);
  lo_op_desc base_kron = desc(LO_OP_KRON_DIAG, 2, 42, 6, 7, true, LO_DIAG_NONE);
  lo_mask_desc md = {&base_dense, I(0x70000), 61}, mk = {&base_kron, I(0x70000), 29}, ms = {&sum2, I(0x70000), 57};
  lo_op_desc m_dense = desc(LO_OP_MASKED, 2, 61, 0, 0, false, LO_DIAG_FULL);
  m_dense.A0 = nullptr;
  lo_op_desc m_kron = m_dense, m_sum = m_dense;
  m_dense.mask = &md;
  m_kron.N = 29; m_kron.mask = &mk;
  m_sum.N = 57; m_sum.mask = &ms;
  t.push_back({"masked_dense", m_dense, true});
  t.push_back({"masked_kron", m_kron, true});
  t.push_back({"masked_sum", m_sum, true});
  t.push_back({"sum3", sum3, true});

  // one refused descriptor per kind (and a sum whose LATER term is refused: the earlier terms' plans must not stay)
  auto refuse = [&](const char* name, lo_op_desc d) { t.push_back({name, d, false}); };
  lo_op_desc x = t[0].op; x.R = 0; refuse("bad lowrank", x);
  x = t[3].op; x.A0 = nullptr; refuse("bad dense", x);
  x = t[4].op; x.n2 = 4; refuse("bad kron", x);
  x = t[6].op; x.R = 32; refuse("bad toeplitz", x);
  x = ski; x.interp = nullptr; refuse("bad ski", x);
  x = grid2; x.R = 34; refuse("bad ski grid", x);
  x = t[11].op; x.n2 = 0; refuse("bad hadamard", x);
  x = m_dense; x.N = 5; refuse("bad masked", x);
  const lo_op_desc had = t[11].op;  // (a copy: the table grows)
  lo_mask_desc mh = {&had, I(0x70000), 61};
  x = m_dense; x.mask = &mh; refuse("masked over hadamard", x);
  x = sum3; x.nterms = 1; refuse("bad sum", x);
  lo_op_desc x_cb = desc(LO_OP_CALLBACK, 2, 64, 0, 0, false, LO_DIAG_NONE); refuse("callback without one", x_cb);
  int bad = walk(t);

  lo_op_desc late[3] = {terms3[0], terms3[1], terms3[2]};
  late[2].n2 = 9;  // 8 * 9 != 80: refused after the first two terms were planned
  lo_op_desc sum_late = sum3;
  sum_late.terms = late;
  bad += walk({{"sum, bad last term", sum_late, true}});  // (its first terms do take buffers)
  bad += walk_precond(t[0].op) + walk_entries() + walk_f64() + walk_pickers();

  // ---- refused descriptors through the pivoted Cholesky and the product: per kind a missing pointer, an out-of-range
  // family or grid axis, M != R, and the fp32 kinds at the float64 entry (its UNSUPPORTED comes before the check)
  const int BA = LO_ERR_BADARG, UN = LO_ERR_UNSUPPORTED, WS = LO_ERR_WORKSPACE;
  std::vector<Refused> r;
  auto with = [](lo_op_desc d, auto edit) { edit(d); return d; };
  const lo_op_desc tz = t[6].op;
  r.push_back({"hadamard, no G", with(had, [](lo_op_desc& d) { d.A1 = nullptr; }), {BA, UN, BA}});
  r.push_back({"hadamard, q = 0", with(had, [](lo_op_desc& d) { d.n2 = 0; }), {BA, UN, BA}});
  r.push_back({"toeplitz, no column", with(tz, [](lo_op_desc& d) { d.A0 = nullptr; }), {BA, UN, BA}});
  r.push_back({"toeplitz, M != N", with(tz, [](lo_op_desc& d) { d.R = 32; }), {BA, UN, BA}});
  r.push_back({"toeplitz, M != N beyond the bound", with(tz, [](lo_op_desc& d) { d.R = LO_TOEPLITZ_MAX_M + 1; }), {BA, UN, UN}});
  lo_interp_desc w_nolv = w, g_axis = g2, g_ndim = g2, g_nori = g3;
  w_nolv.left_vals = nullptr;
  g_axis.grid_m[1] = LO_SKI_GRID_MAX_AXIS + 1;
  g_ndim.grid_ndim = 4;
  g_nori.right_idx = nullptr;
  r.push_back({"ski, no interp", with(ski, [](lo_op_desc& d) { d.interp = nullptr; }), {BA, UN, BA}});
  r.push_back({"ski, no left values", with(ski, [&](lo_op_desc& d) { d.interp = &w_nolv; }), {BA, UN, BA}});
  r.push_back({"ski, no column", with(ski, [](lo_op_desc& d) { d.A0 = nullptr; }), {BA, UN, BA}});
  r.push_back({"ski, J = 0", with(ski, [](lo_op_desc& d) { d.n2 = 0; }), {BA, UN, BA}});
  r.push_back({"ski, M = 0", with(ski, [](lo_op_desc& d) { d.R = 0; }), {BA, UN, BA}});
  // the two sides differ: the product bounds M (before it looks at J), the pivoted Cholesky reads single entries
  r.push_back({"ski, M beyond the bound, J = 0",
               with(ski, [](lo_op_desc& d) { d.R = LO_TOEPLITZ_MAX_M + 1; d.n2 = 0; }), {BA, UN, UN}});
  r.push_back({"ski, M beyond the bound (taken)", with(ski, [](lo_op_desc& d) { d.R = LO_TOEPLITZ_MAX_M + 1; }), {WS, UN, UN}});
  r.push_back({"ski, M at the bound (taken)", with(ski, [](lo_op_desc& d) { d.R = LO_TOEPLITZ_MAX_M; }), {WS, UN, WS}});
  r.push_back({"ski grid, no right indices", with(grid3, [&](lo_op_desc& d) { d.interp = &g_nori; }), {BA, UN, BA}});
  r.push_back({"ski grid, axis beyond the bound", with(grid2, [&](lo_op_desc& d) { d.interp = &g_axis; }), {UN, UN, UN}});
  r.push_back({"ski grid, four axes", with(grid2, [&](lo_op_desc& d) { d.interp = &g_ndim; }), {UN, UN, UN}});
  r.push_back({"ski grid, M != R", with(grid2, [](lo_op_desc& d) { d.R = 34; }), {BA, UN, BA}});
  r.push_back({"ski grid, J = 0", with(grid2, [](lo_op_desc& d) { d.n2 = 0; }), {BA, UN, BA}});
  r.push_back({"ski grid, J = 0, four axes", with(grid2, [&](lo_op_desc& d) { d.n2 = 0; d.interp = &g_ndim; }), {BA, UN, UN}});
  lo_grid_desc gd = {2, 0, {5, 7, 0}}, gd_axis = {2, 0, {5, LO_SKI_GRID_MAX_AXIS + 1, 0}}, gd_ndim = {1, 0, {35, 0, 0}};
  lo_op_desc tk = desc(LO_OP_TOEPLITZ_KRON_DIAG, 2, 35, 35, 0, false, LO_DIAG_FULL);
  tk.grid = &gd;
  r.push_back({"toeplitz kron, no grid", with(tk, [](lo_op_desc& d) { d.grid = nullptr; }), {BA, UN, BA}});
  r.push_back({"toeplitz kron, no columns", with(tk, [](lo_op_desc& d) { d.A0 = nullptr; }), {BA, UN, BA}});
  r.push_back({"toeplitz kron, axis beyond the bound", with(tk, [&](lo_op_desc& d) { d.grid = &gd_axis; }), {UN, UN, UN}});
  r.push_back({"toeplitz kron, one axis", with(tk, [&](lo_op_desc& d) { d.grid = &gd_ndim; }), {UN, UN, UN}});
  r.push_back({"toeplitz kron, M != R", with(tk, [](lo_op_desc& d) { d.R = 34; }), {BA, UN, BA}});
  r.push_back({"toeplitz kron, M != N", with(tk, [](lo_op_desc& d) { d.N = 36; }), {BA, UN, BA}});
  const lo_op_desc ko = desc(LO_OP_KERNEL_DIAG, 2, 100, 3, LO_KERNEL_MATERN32, true, LO_DIAG_FULL);
  r.push_back({"kernel, no theta", with(ko, [](lo_op_desc& d) { d.A1 = nullptr; }), {BA, UN, BA}});
  r.push_back({"kernel, family 4", with(ko, [](lo_op_desc& d) { d.n2 = 4; }), {BA, UN, BA}});
  r.push_back({"kernel, family -1", with(ko, [](lo_op_desc& d) { d.n2 = -1; }), {BA, UN, BA}});
  r.push_back({"kernel, D = 0", with(ko, [](lo_op_desc& d) { d.R = 0; }), {BA, UN, BA}});
  r.push_back({"kernel, D beyond the bound", with(ko, [](lo_op_desc& d) { d.R = LO_KERNEL_MAX_DIM + 1; }), {UN, UN, UN}});
  // the two sides differ: the product's launch bounds the batch, the pivoted Cholesky's does not
  r.push_back({"kernel, B = 65536 (taken)", with(ko, [](lo_op_desc& d) { d.B = 65536; }), {WS, UN, UN}});
  r.push_back({"kernel, B = 65535 (taken)", with(ko, [](lo_op_desc& d) { d.B = 65535; }), {WS, UN, WS}});
  lo_op_desc ks = ko, kk = ko, kg = ko, kt = ko;
  ks.kind = LO_OP_KERNEL_SUM_DIAG; ks.nterms = 3; ks.n2 = 0x210;
  kk.kind = LO_OP_KERNEL_KRON_DIAG; kk.nterms = 4; kk.task = F(0xb0000);
  kg.kind = LO_OP_KERNEL_GRAD_DIAG; kg.n2 = LO_KERNEL_RBF;
  kt.kind = LO_OP_KERNEL_TASK_DIAG; kt.nterms = 4; kt.task = F(0xb0000);
  r.push_back({"kernel sum, no points", with(ks, [](lo_op_desc& d) { d.A0 = nullptr; }), {BA, UN, BA}});
  r.push_back({"kernel sum, family 4 in term 1", with(ks, [](lo_op_desc& d) { d.n2 = 0x240; }), {BA, UN, BA}});
  r.push_back({"kernel sum, D beyond the bound", with(ks, [](lo_op_desc& d) { d.R = LO_KERNEL_MAX_DIM + 1; }), {UN, UN, UN}});
  r.push_back({"kernel kron, no task matrix", with(kk, [](lo_op_desc& d) { d.task = nullptr; }), {BA, UN, BA}});
  r.push_back({"kernel kron, family 4", with(kk, [](lo_op_desc& d) { d.n2 = 4; }), {BA, UN, BA}});
  r.push_back({"kernel kron, N % T != 0", with(kk, [](lo_op_desc& d) { d.nterms = 3; }), {BA, UN, BA}});
  r.push_back({"kernel grad, no theta", with(kg, [](lo_op_desc& d) { d.A1 = nullptr; }), {BA, UN, BA}});
  r.push_back({"kernel grad, Matern", with(kg, [](lo_op_desc& d) { d.n2 = LO_KERNEL_MATERN52; }), {UN, UN, UN}});
  r.push_back({"kernel grad, N % (D + 1) != 0", with(kg, [](lo_op_desc& d) { d.R = 2; }), {BA, UN, BA}});
  r.push_back({"kernel task, no task matrix", with(kt, [](lo_op_desc& d) { d.task = nullptr; }), {BA, UN, BA}});
  r.push_back({"kernel task, family 4", with(kt, [](lo_op_desc& d) { d.n2 = 4; }), {BA, UN, BA}});
  r.push_back({"kernel task, T beyond the bound",
               with(kt, [](lo_op_desc& d) { d.nterms = LO_KERNEL_TASK_MAX_TASKS + 1; }), {UN, UN, UN}});
  lo_op_desc ss = ski;
  ss.kind = LO_OP_SKI_SUM_DIAG; ss.nterms = 2;
  r.push_back({"ski sum, no interp", with(ss, [](lo_op_desc& d) { d.interp = nullptr; }), {BA, UN, BA}});
  r.push_back({"ski sum, no terms", with(ss, [](lo_op_desc& d) { d.nterms = 0; }), {BA, UN, BA}});
  r.push_back({"ski sum, M beyond the bound", with(ss, [](lo_op_desc& d) { d.R = LO_TOEPLITZ_MAX_M + 1; }), {UN, UN, UN}});
  // sums: a kernel term is validated as the kind on its own is, and refused by the float64 entry
  lo_op_desc kterm = with(ko, [](lo_op_desc& d) { d.N = 80; d.diag_mode = LO_DIAG_NONE; d.d = nullptr; });
  lo_op_desc kbad = with(kterm, [](lo_op_desc& d) { d.n2 = 7; });
  lo_op_desc sk_terms[2] = {terms2[0], kbad}, sk64_terms[2] = {terms2[0], kterm}, sh_terms[2] = {terms2[0], had};
  r.push_back({"sum, kernel term of family 7", with(sum2, [&](lo_op_desc& d) { d.terms = sk_terms; }), {BA, UN, BA}});
  r.push_back({"sum, kernel term (taken by fp32)", with(sum2, [&](lo_op_desc& d) { d.terms = sk64_terms; }), {WS, UN, WS}});
  r.push_back({"sum, Hadamard term", with(sum2, [&](lo_op_desc& d) { d.terms = sh_terms; }), {BA, BA, BA}});
  r.push_back({"sum, one term", with(sum2, [](lo_op_desc& d) { d.nterms = 1; }), {BA, BA, BA}});
  r.push_back({"masked", m_dense, {UN, UN, WS}});
  r.push_back({"callback", x_cb, {UN, UN, BA}});
  r.push_back({"dense, N beyond 32 bits", with(base_dense, [](lo_op_desc& d) { d.N = 0x7ffffff1; }), {UN, UN, WS}});
  bad += walk_refused(r);
  printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
