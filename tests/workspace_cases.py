"""Small shapes for the workspace sizers of the entry points that are not solvers: the Woodbury apply, the
preconditioner builds, the bilinear forms, the probe vectors, the blocked Cholesky and the SLQ eigensolver.  Shared by
tests/test_workspace_bytes_cpu.py (sizes only, no device call), tools/record_workspace_bytes.py (which wrote
tests/golden/workspace_bytes.json) and tests/test_gpu_workspace.py.  Not a test module.

A row is (arguments of the sizer, needed): `needed` is the plain sum of the buffers the entry point provably uses, with
every row split counted as one block (the library never splits into fewer), and 0 for a shape the sizer refuses.  Only
lo_hadamard_bilinear_workspace_bytes and lo_cholesky_workspace_bytes refuse a shape; the other sizers report a size for
whatever they are given and their entry points do the refusing.

F64_CASES: the float64 solvers and the float64 Woodbury apply, rows of the same form.  They are a table of their own
because their entry points take a workspace without the sizer's tail (a behaviour kept as it is), so the walk of
tests/test_gpu_workspace.py, which expects one byte less than the reported size to be refused, does not apply to them."""
import ctypes

from linear_operator_amd import _hip


def padded_rank(k):
    """Floats per row of a rank-k factor as the skinny kernels read it (csrc/lo_internal.h)."""
    p = 1
    while p < (k + 3) // 4:
        p *= 2
    return 4 * p


def _apply(B, N, k, c):
    R4 = padded_rank(k)  # u = Q^T r partials, and the padded copy of Q when its rows are not R4 floats already
    return (B, N, k, c), 4 * B * R4 * c + (4 * B * N * R4 if k != R4 else 0)


def _build(B, N, k):  # Gram partials and M^-1 in fp64, the log d partials, 1 / sqrt(d) per row
    return (B, N, k), 8 * B * k * k + 8 * B + 8 * B * k * k + 4 * B * N


def _root_form(B, N, R):
    return (B, N, R), 8 * B * R * R + 8 * B + 4 * B * N


def _root_form_rs(B, N, R):  # two Gram matrices: C^T D^-1 C and C^T C
    return (B, N, R), 2 * 8 * B * R * R + 8 * B + 4 * B * N


def _kron_root(B):  # a 16 x 16 Gram matrix in fp64, log d, three 16 x 16 fp32 blocks, logdet and 1 / sigma
    return (B,), 8 * B * 256 + 8 * B + 4 * B * 768 + 4 * B * 2


def _hadamard(B, N, p, q, S):  # M_t and its transpose for the 2 S columns, and at least as much again for the partials
    return (B, N, p, q, S), 3 * 4 * B * 2 * S * p * q


APPLY_SHAPES = ((1, 37, 1), (3, 300, 3))
APPLY_RANKS = (4, 5, 8, 33)

CASES = {
    "lo_precond_apply_workspace_bytes": [_apply(B, N, k, c) for (B, N, c) in APPLY_SHAPES for k in APPLY_RANKS],
    "lo_precond_build_workspace_bytes": [_build(2, 37, 5), _build(3, 300, 33), _build(1, 1024, 16)],
    "lo_precond_root_form_workspace_bytes": [_root_form(2, 37, 5), _root_form(3, 300, 32)],
    "lo_precond_root_form_rs_workspace_bytes": [_root_form_rs(2, 37, 8), _root_form_rs(3, 300, 32)],
    "lo_precond_kron_root_workspace_bytes": [_kron_root(1), _kron_root(3)],
    # t = C^T [U V] partials [B, S, 2 D, R]
    "lo_bilinear_root_workspace_bytes": [((2, 37, 5, 3), 4 * 2 * 2 * 3 * 5), ((3, 300, 8, 4), 4 * 3 * 2 * 4 * 8)],
    # the intermediate [B, n1, n2, D]
    "lo_bilinear_kron_workspace_bytes": [((2, 3, 5, 3), 4 * 2 * 15 * 3), ((1, 128, 128, 2), 4 * 128 * 128 * 2)],
    # squared-norm partials [B, blocks of 256 rows, P]
    "lo_probe_vectors_workspace_bytes": [((2, 37, 3), 4 * 2 * 3), ((3, 300, 4), 4 * 3 * 2 * 4)],
    "lo_hadamard_bilinear_workspace_bytes": [_hadamard(2, 37, 3, 2, 1), _hadamard(2, 70, 3, 2, 3),
                                             ((2, 37, 0, 2, 1), 0)],
    # the factor's working copy and the fp64 row sums
    "lo_cholesky_workspace_bytes": [((2, 37), 4 * 2 * 37 * 37 + 8 * 2 * 37), ((1, 64), 4 * 64 * 64 + 8 * 64),
                                    ((2, 1025), 0)],
    # the fail flag and one fp64 term per (probe, member)
    "lo_tridiag_eigh_slq_workspace_bytes": [((3, 2), 4 + 8 * 6), ((1, 1), 4 + 8)],
}


F64_SHAPES = ((1, 1, 1), (3, 37, 3), (2, 300, 17))  # (B, N, c)


def _cg_f64(B, N, c):  # the control block (8 ints and a double), six vectors, ten scalars and two flags per column
    prm = _hip.CgParamsF64(c=c, max_iter=20, max_tridiag_iter=20)
    return (B, N, prm), 40 + 8 * (6 * B * N * c + 10 * B * c) + 4 * 2 * B * c


def _minres_f64(B, N, c, Q):
    # the control block (4 ints and a double), six vectors and three per shift, six scalars and a flag per column, the
    # nine Givens scalars and two squared norms per shift and column
    prm = _hip.MinresParamsF64(c=c, n_shifts=Q, max_iter=20)
    return (B, N, prm), 24 + 8 * ((6 + 3 * Q) * B * N * c + 6 * B * c + 11 * Q * B * c) + 4 * B * c


def _lanczos_f64(B, N, P, max_iter):  # r and the product, the coefficients of every step, two norms, four flag words
    return (B, N, P, max_iter), 8 * (2 * B * N * P + B * P * max_iter + 2 * B * P) + 4 * 4


def _precond_f64(B, N, k, c):  # the partials of Q^T r, one block per chunk of 256 rows, and their sum
    return (B, N, k, c), 8 * B * k * c * ((N + 255) // 256 + 1)


F64_CASES = {
    "lo_cg_f64_workspace_bytes": [_cg_f64(*s) for s in F64_SHAPES],
    "lo_minres_f64_workspace_bytes": [_minres_f64(*s, Q) for s in F64_SHAPES for Q in (1, 3)],
    "lo_lanczos_f64_workspace_bytes": [_lanczos_f64(*s, m) for s in F64_SHAPES for m in (1, 20)],
    "lo_precond_f64_workspace_bytes": [_precond_f64(B, N, k, c) for (B, N, c) in F64_SHAPES for k in (4, 33)],
}


def _show(a):
    """An argument in a key: a parameter struct as its non-zero fields."""
    if isinstance(a, ctypes.Structure):
        return "{" + " ".join(f"{n}={getattr(a, n)}" for n, _ in a._fields_ if getattr(a, n)) + "}"
    return str(a)


def key(fn, args):
    return fn + "(" + ",".join(_show(a) for a in args) + ")"


def sizes(lib):
    """{key: bytes} over both tables."""
    return {key(fn, args): int(getattr(lib, fn)(*args)) for table in (CASES, F64_CASES) for fn, rows in table.items()
            for args, _ in rows}
