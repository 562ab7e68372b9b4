"""KroneckerProductLinearOperator K1 (x) ... (x) KP -- `_matmul`, `_diagonal`, `_get_indices` only
(reference: operators/kronecker_product_linear_operator.py:20-45, 62-96, 188-216, 272-284).  Two dense factors
lower to the batched-GEMM kernel pair in csrc/lo_kron.hip; products of more dense factors are regrouped into two
dense groups (`_two_groups`) and lower the same way.  A product of 2 or 3 symmetric Toeplitz factors (the covariance of
a GP on a regular 2-D / 3-D grid) lowers to LO_OP_TOEPLITZ_KRON_DIAG (csrc/lo_ski_grid.hip), and the gradients with
respect to the factors' columns come from lo_toeplitz_kron_bilinear_f32 or, outside its limits, from the same closed
form in torch.

Multitask covariance, matrix-free.  Kron(KernelLinearOperator(X, X), Dense(Bt)) with a native kernel factor over one
points tensor and a float32 device task factor Bt [*b, T, T], T <= LO_KERNEL_KRON_MAX_TASKS (`_kernel_kron_refusal`),
lowers to LO_OP_KERNEL_KRON_DIAG (csrc/lo_kernel_kron.hip): CG, Lanczos, MINRES and the pivoted Cholesky run on the
device without a Python call per product and without K (x) Bt or K in memory.  `_matmul` itself goes to the fused
product only for the (T, columns) cells of `_NATIVE_MATMUL_KERNEL_KRON`; elsewhere it keeps the per-factor composition,
whose kernel factor is matrix-free already.  `_bilinear_derivative` composes the kernel factor's native derivatives
with one on-the-fly product for Bt; no autograd, nothing of size n^2.  The matrix-free route to a solve is the explicit
AddedDiagLinearOperator(kron, DiagLinearOperator(d)), or KroneckerProductAddedDiag with a general diagonal: `+` and
`add_diagonal` are routed as before, so a constant or Kronecker-structured diagonal keeps the reference's
eigendecomposition forms (which take the dense n x n data kernel).

`+ Diag` / `add_diagonal` build the
KroneckerProductAddedDiagLinearOperator like the reference (:98-145): eigendecomposition closed forms for a
constant diagonal, the CG path otherwise (an explicit AddedDiagLinearOperator(kron, diag) is always the CG path)."""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import Tensor

from .. import kernels as K
from .. import settings
from ..utils.broadcasting import _matmul_broadcast_shape
from ..utils.toeplitz import sym_toeplitz_derivative_quadratic_form, sym_toeplitz_matmul
from ._linear_operator import LinearOperator
from .dense_linear_operator import DenseLinearOperator, to_linear_operator
from .diag_linear_operator import DiagLinearOperator
from .kernel_linear_operator import KernelLinearOperator
from .toeplitz_linear_operator import ToeplitzLinearOperator

# Which products of a Kronecker product of Toeplitz factors `_matmul` hands to the kernels, by (axes, one column / more
# columns): True only where tools/mb_toeplitz_kron.py measured the native product at least as fast as the per-factor
# composition `_matmul` otherwise runs (DESIGN.md section 6j holds both times of every cell).  A cell that is absent
# keeps the composition; the descriptor still serves CG, Lanczos, MINRES and the pivoted Cholesky, where it replaces a
# Python call per product.  Measured (native / composition, microseconds; 1 column, 17 columns):
#   2-D  1 x 128 (x) 128            19 /   236      24 /  3885
#   2-D  16 x 64 (x) 64             17 /   118      34 /  1883
#   3-D  1 x 32 (x) 32 (x) 32       21 /  2382      31 / 40654
_NATIVE_MATMUL_TOEPLITZ: dict = {(2, 1): True, (2, 2): True, (3, 1): True, (3, 2): True}


# Which products of Kron(Kernel, Dense(Bt)) `_matmul` hands to the fused kernel lo_kernel_kron_mv_f32, by (T, one column /
# more columns): True only where tools/mb_kernel_kron.py measured it at least as fast, beyond the spread of the rounds, as
# the per-factor composition (`_kron_matmul`: lo_kernel_mv_f32 with T c columns, then Bt) at BOTH measured shapes.  An
# absent cell keeps the composition; the descriptor lowers always.  Measured on the MI355X (fused / composition,
# microseconds; 1 x 16384, D 4 and 8 x 4096, D 16):
#   T 2   1 column  145 /  161,  203 /  224     17 columns   754 /  795 (ranges overlap),   681 /  940
#   T 4   1 column  143 /  160,  205 /  229     17 columns  1358 / 1314,                   1120 / 1534
#   T 8   1 column  290 /  262,  306 /  314     17 columns  3146 / 2347,                   2264 / 2703
# T = 3 was not measured and takes the side its two neighbours share.
_NATIVE_MATMUL_KERNEL_KRON: dict = {(2, 1): True, (3, 1): True, (4, 1): True}


def _kron_diag(*ops) -> Tensor:
    lead = ops[0]._diagonal()
    if len(ops) == 1:
        return lead
    trail = _kron_diag(*ops[1:])
    d = lead.unsqueeze(-2) * trail.unsqueeze(-1)
    return d.mT.reshape(*d.shape[:-2], -1)


def _kron_matmul(ops, kp_shape, rhs):
    """Per factor: view [n_i, -1], multiply, transposing reshape (reference :34-45) -- ATen fallback path."""
    out_shape = _matmul_broadcast_shape(kp_shape, rhs.shape)
    batch = out_shape[:-2]
    res = rhs.expand(*batch, *rhs.shape[-2:])
    ncols = rhs.size(-1)
    for op in ops:
        res = res.reshape(*batch, op.size(-1), -1)
        f = op._matmul(res)
        res = f.view(*batch, op.size(-2), -1, ncols).transpose(-3, -2).reshape(*batch, -1, ncols)
    return res


def _dense_kron(ts):
    res = ts[0]
    for nxt in ts[1:]:
        res = (res.unsqueeze(-1).unsqueeze(-3) * nxt.unsqueeze(-2).unsqueeze(-4)).reshape(
            *torch.broadcast_shapes(res.shape[:-2], nxt.shape[:-2]), res.shape[-2] * nxt.shape[-2],
            res.shape[-1] * nxt.shape[-1])
    return res


def _group_pullback(dG: Tensor, ts):
    """Gradients of the factors of G = T_1 (x) .. (x) T_p from dG: dT_i[a, b] = sum over the other factors' indices of
    dG[(.., a, ..), (.., b, ..)] prod_{j != i} T_j[r_j, c_j]."""
    if len(ts) == 1:
        return [dG]
    p = len(ts)
    sizes = [t.shape[-1] for t in ts]
    dG = dG.reshape(*dG.shape[:-2], *sizes, *sizes)
    rows, cols = "abcdefgh"[:p], "ijklmnop"[:p]
    out = []
    for i in range(p):
        others = ",".join(f"...{rows[j]}{cols[j]}" for j in range(p) if j != i)
        expr = f"...{rows}{cols},{others}->...{rows[i]}{cols[i]}"
        out.append(torch.einsum(expr, dG, *[ts[j] for j in range(p) if j != i]))
    return out


def _toeplitz_kron_bilinear_torch(cols, u: Tensor, v: Tensor):
    """The column gradients of sum_s u_s^T (T_1 (x) .. (x) T_D) v_s in torch, any number of factors: cols[k]
    [*batch, M_k], u, v [*batch, N, S] of one batch shape.  Returns [g_k [*batch, M_k]]."""
    batch, (N, S) = u.shape[:-2], u.shape[-2:]
    sizes = [int(t.shape[-1]) for t in cols]

    def axis_view(x, k):  # [*batch, outer, M_k, inner]
        outer = math.prod(sizes[:k])
        return x.reshape(*batch, outer, sizes[k], N // (outer * sizes[k]) * S)

    grads = []
    for k in range(len(cols)):
        w = v
        for j in range(len(cols)):
            if j != k:
                w = sym_toeplitz_matmul(cols[j].unsqueeze(-2), axis_view(w, j).contiguous()).reshape(*batch, N, S)
        g = sym_toeplitz_derivative_quadratic_form(axis_view(u, k).contiguous(), axis_view(w, k).contiguous())
        grads.append(g.sum(-2))
    return grads


class KroneckerProductLinearOperator(LinearOperator):
    def __init__(self, *linear_ops):
        try:
            linear_ops = tuple(to_linear_operator(op) for op in linear_ops)
        except TypeError:
            raise RuntimeError("KroneckerProductLinearOperator is intended to wrap lazy tensors.")
        try:
            batch = torch.broadcast_shapes(*(op.batch_shape for op in linear_ops))
        except RuntimeError:
            raise RuntimeError(
                "Batch shapes of LinearOperators "
                f"({', '.join([str(tuple(op.shape)) for op in linear_ops])}) "
                "are incompatible for a Kronecker product."
            )
        if len(batch):
            linear_ops = tuple(op._expand_batch(batch) if op.batch_shape != batch else op for op in linear_ops)
        super().__init__(*linear_ops)
        self.linear_ops = linear_ops

    # ---- lowering: the kernels take TWO dense factors.  A product of more factors is regrouped as
    #      (K_1 (x) .. (x) K_j) (x) (K_j+1 (x) .. (x) K_m) with the split that balances the two sides, the groups formed
    #      densely (they are small: the whole point of the structure is n_i << N); gradients are pulled back to the
    #      individual factors by contracting the group's gradient with the other factors of the group.
    _kMaxGroup = 2048  # largest side of a regrouped factor (B x n^2 floats are materialised)

    def _two_groups(self):
        """(A, B, j): dense group tensors and the split index, or None when the product does not lower."""
        ops = self.linear_ops
        if len(ops) < 2 or not all(isinstance(op, DenseLinearOperator) for op in ops):
            return None
        ts = [op.tensor for op in ops]
        if not all(t.is_cuda and t.dtype == ts[0].dtype and t.shape[-1] == t.shape[-2] for t in ts):
            return None
        if ts[0].dtype != torch.float32 and not (ts[0].dtype == torch.float64 and len(ts) == 2):
            return None  # (float64: two dense factors, for lo_matvec_f64 and the float64 solvers)
        if len(ts) == 2:
            return ts[0], ts[1], 1
        sizes = [t.shape[-1] for t in ts]
        best = None
        for j in range(1, len(ts)):
            na, nb = math.prod(sizes[:j]), math.prod(sizes[j:])
            if best is None or max(na, nb) < best[0]:
                best = (max(na, nb), j)
        if best[0] > self._kMaxGroup:
            return None
        j = best[1]
        # the regrouped dense factors are memoised per operator object, keyed on the factor tensors' storage AND version
        # counters: an in-place update of a factor (optimizer step on a reused operator) rebuilds the groups instead of
        # silently multiplying with stale ones
        key = tuple((t.data_ptr(), t._version, tuple(t.shape)) if not t.is_inference() else None for t in ts)
        cache = getattr(self, "_groups_cache", None)
        if cache is None or None in key or cache[0] != key:
            with torch.no_grad():
                cache = (key, (_dense_kron(ts[:j]), _dense_kron(ts[j:]), j))
            self._groups_cache = cache
        return cache[1]

    def _toeplitz_columns(self):
        """The factors' first columns when every factor is a symmetric Toeplitz operator, else None."""
        if len(self.linear_ops) < 2 or not all(isinstance(op, ToeplitzLinearOperator) for op in self.linear_ops):
            return None
        return [op.column for op in self.linear_ops]

    def _toeplitz_native(self, cols) -> bool:
        """Whether the kernels of csrc/lo_ski_grid.hip take these columns: 2 or 3 fp32 HIP columns within the limits."""
        return (all(t.is_cuda and t.dtype == torch.float32 for t in cols)
                and K.ski_grid_shape_ok(tuple(int(t.shape[-1]) for t in cols)))

    def _kernel_kron_refusal(self, check_device: bool = True) -> Optional[str]:
        """None when this product is the matrix-free multitask operator the kind LO_OP_KERNEL_KRON_DIAG takes, else the
        reason it is not.  `check_device=False` leaves out the on-the-device conditions, as KernelLinearOperator's
        `_native_refusal` does (the rest of the gate can then be asked on any machine)."""
        ops = self.linear_ops
        if len(ops) != 2:
            return f"{len(ops)} factors"
        kern, task = ops
        if not isinstance(kern, KernelLinearOperator):
            return "the first factor is not a KernelLinearOperator"
        why = kern._native_refusal(check_device)
        if why is not None:
            return f"kernel factor: {why}"
        if not kern._same_points():
            return "kernel factor over two different point tensors"
        if not isinstance(task, DenseLinearOperator):
            return "the task factor is not a DenseLinearOperator"
        Bt = task.tensor
        if Bt.dim() < 2 or Bt.shape[-1] != Bt.shape[-2]:
            return f"task factor of shape {tuple(Bt.shape)}"
        if Bt.shape[-1] > K._hip.LO_KERNEL_KRON_MAX_TASKS:
            return f"T = {Bt.shape[-1]} beyond LO_KERNEL_KRON_MAX_TASKS"
        if Bt.dtype != torch.float32:
            return "task factor not float32"
        if check_device and not Bt.is_cuda:
            return "task factor not on the device"
        return None

    def _kernel_kron_descriptor(self, bs):
        kern, task = self.linear_ops
        X = kern.x1.detach()
        X = X if X.shape[:-2] == bs else X.expand(*bs, *X.shape[-2:])
        Bt = task.tensor.detach()
        Bt = Bt if Bt.shape[:-2] == bs else Bt.expand(*bs, *Bt.shape[-2:])
        theta = K.kernel_theta(kern.tensor_params["lengthscale"], kern.tensor_params["outputscale"], bs, X.shape[-1])
        return K.kernel_kron_diag_descriptor(X, theta, kern.covar_func.native_family, Bt)

    def _kernel_descriptor(self, batch_shape=None):
        if self._kernel_kron_refusal() is None:
            return self._kernel_kron_descriptor(torch.Size(self.batch_shape if batch_shape is None else batch_shape))
        cols = self._toeplitz_columns()
        if cols is not None:
            if not self._toeplitz_native(cols):
                return None
            bs = torch.Size(batch_shape) if batch_shape is not None else self.batch_shape
            return K.toeplitz_kron_diag_descriptor([t.expand(*bs, t.shape[-1]) for t in cols], None)
        groups = self._two_groups()
        if groups is None:
            return None
        k1, k2, _ = groups
        bs = torch.Size(batch_shape) if batch_shape is not None else self.batch_shape
        k1 = k1.expand(*bs, *k1.shape[-2:])
        k2 = k2.expand(*bs, *k2.shape[-2:])
        return K.kron_diag_descriptor(k1, k2, None, dtype=k1.dtype)

    def _bilinear_derivative(self, left_vecs: Tensor, right_vecs: Tensor):
        """(dK1, dK2) = (sum_d U_d K2 V_d^T, sum_d U_d^T K1 V_d): the reference's generic autograd version
        (_linear_operator.py:336-393) applied to the Kronecker matvec (:34-45); two dense factors on this path."""
        cols = self._toeplitz_columns()
        if cols is not None:
            return self._toeplitz_bilinear_derivative(cols, left_vecs, right_vecs)
        if (len(self.linear_ops) == 2 and isinstance(self.linear_ops[0], KernelLinearOperator)
                and isinstance(self.linear_ops[1], DenseLinearOperator)):
            return self._kernel_kron_bilinear_derivative(left_vecs, right_vecs)
        groups = self._two_groups()
        if groups is None:
            return super()._bilinear_derivative(left_vecs, right_vecs)
        k1, k2, j = groups
        d1, d2 = K.bilinear_kron(k1, k2, left_vecs, right_vecs)
        ts = [op.tensor for op in self.linear_ops]
        grads = _group_pullback(d1, ts[:j]) + _group_pullback(d2, ts[j:])
        return tuple(g if tuple(g.shape) == tuple(t.shape) else g.sum_to_size(*t.shape) for g, t in zip(grads, ts))

    def _kernel_kron_bilinear_derivative(self, left_vecs: Tensor, right_vecs: Tensor):
        """Kron(Kernel, Dense(Bt)), row index i T + t, by composition -- no autograd of the product, nothing of size
        n^2.  With U3 = U viewed as [*b, m, T s] and VB3 the same view of V with Bt applied to the task index of every row,
        sum_col u^T (K (x) Bt) v = sum_col' U3^T K VB3: the kernel factor's own derivative (lo_kernel_bilinear_f32 and
        lo_kernel_points_grad_f32 on the native path).  dBt[tau, s] = sum_{i, col} U[(i, tau), col] (K V3)[(i, s), col]:
        one product of the kernel factor with T s columns (lo_kernel_mv_f32) and a contraction."""
        kern, task = self.linear_ops
        if left_vecs.ndimension() == 1:
            left_vecs, right_vecs = left_vecs.unsqueeze(-1), right_vecs.unsqueeze(-1)
        Bt = task.tensor
        T, S = Bt.shape[-1], left_vecs.shape[-1]
        m, n = kern.shape[-2:]
        bs = torch.broadcast_shapes(self.batch_shape, left_vecs.shape[:-2], right_vecs.shape[:-2])
        U4 = left_vecs.detach().expand(*bs, m * T, S).reshape(*bs, m, T, S)
        V4 = right_vecs.detach().expand(*bs, n * T, S).reshape(*bs, n, T, S)
        VB4 = torch.einsum("...ts,...jsc->...jtc", Bt.detach(), V4)
        g_kern = kern._bilinear_derivative(U4.reshape(*bs, m, T * S), VB4.reshape(*bs, n, T * S))
        g_task = None
        if Bt.requires_grad:
            KV4 = kern._matmul(V4.reshape(*bs, n, T * S)).reshape(*bs, m, T, S)
            g_task = torch.einsum("...itc,...isc->...ts", U4, KV4)
            g_task = g_task if tuple(g_task.shape) == tuple(Bt.shape) else g_task.sum_to_size(*Bt.shape)
        return tuple(g_kern) + (g_task,)

    def _toeplitz_bilinear_derivative(self, cols, left_vecs: Tensor, right_vecs: Tensor):
        """One gradient per factor column.  With W_k = v with every factor but T_k applied, u and W_k viewed as
        [*batch, outer, M_k, inner] (inner = (prod_{j > k} M_j) S):
            g_k[l] = sum_{outer} sum_s sum_i (u[i, s] W_k[i + l, s] + [l > 0] u[i + l, s] W_k[i, s])
        -- the Toeplitz lag correlation along axis k, summed over the lines of the other axes (the reference obtains the
        same by autograd of `_matmul`).  Native for 2 or 3 fp32 HIP columns within the kernel's limits; CPU, float64, more
        factors and larger grids take the same formula in torch."""
        if left_vecs.ndimension() == 1:
            left_vecs, right_vecs = left_vecs.unsqueeze(-1), right_vecs.unsqueeze(-1)
        batch = torch.broadcast_shapes(self.batch_shape, left_vecs.shape[:-2], right_vecs.shape[:-2])
        sizes = [int(t.shape[-1]) for t in cols]
        N, S = math.prod(sizes), left_vecs.shape[-1]
        u = left_vecs.expand(*batch, N, S)
        v = right_vecs.expand(*batch, N, S)
        ecols = [t.detach().expand(*batch, t.shape[-1]) for t in cols]
        if (self._toeplitz_native(cols) and u.is_cuda and u.dtype == torch.float32 and v.is_cuda
                and v.dtype == torch.float32):
            grads = K.toeplitz_kron_bilinear([t.reshape(-1, t.shape[-1]) for t in ecols], u.reshape(-1, N, S),
                                             v.reshape(-1, N, S))
            grads = [g.reshape(*batch, g.shape[-1]) for g in grads]
        else:
            grads = _toeplitz_kron_bilinear_torch(ecols, u, v)
        return tuple(g if tuple(g.shape) == tuple(t.shape) else g.sum_to_size(*t.shape) for g, t in zip(grads, cols))

    def __add__(self, other):  # reference :98-114
        from .diag_linear_operator import ConstantDiagLinearOperator, DiagLinearOperator
        from .kronecker_product_added_diag_linear_operator import KroneckerProductAddedDiagLinearOperator

        if isinstance(other, (KroneckerProductDiagLinearOperator, ConstantDiagLinearOperator)):
            return KroneckerProductAddedDiagLinearOperator(self, other)
        if isinstance(other, DiagLinearOperator):
            return self.add_diagonal(other._diagonal())
        if (isinstance(other, KroneckerProductLinearOperator) and len(other.linear_ops) == len(self.linear_ops)
                and all(a.shape[-2:] == b.shape[-2:] and a.shape[-1] == a.shape[-2]
                        for a, b in zip(self.linear_ops, other.linear_ops))):
            from .sum_kronecker_linear_operator import SumKroneckerLinearOperator

            return SumKroneckerLinearOperator(self, other)  # reference :107-111: the eigenbasis closed forms
        return super().__add__(other)

    def add_diagonal(self, diag: Tensor):  # reference :116-145
        from .diag_linear_operator import ConstantDiagLinearOperator, DiagLinearOperator
        from .kronecker_product_added_diag_linear_operator import KroneckerProductAddedDiagLinearOperator

        if not self.is_square:
            raise RuntimeError("add_diag only defined for square matrices")
        diag_shape = diag.shape
        if len(diag_shape) == 0:  # scalar tensor = constant diagonal
            diag_tensor = ConstantDiagLinearOperator(diag.unsqueeze(-1), diag_shape=self.shape[-1])
        elif diag_shape[-1] == 1:
            diag_tensor = ConstantDiagLinearOperator(diag, diag_shape=self.shape[-1])
        else:
            try:
                expanded_diag = diag.expand(self.shape[:-1])
            except RuntimeError:
                raise RuntimeError(
                    "add_diag for LinearOperator of size {} received invalid diagonal of size {}.".format(
                        self.shape, diag_shape
                    )
                )
            diag_tensor = DiagLinearOperator(expanded_diag)
        return KroneckerProductAddedDiagLinearOperator(self, diag_tensor)

    def diagonalization(self, method=None):  # reference :147-152
        return super().diagonalization(method="symeig" if method is None else method)

    def _symeig(self, eigenvectors: bool = False, return_evals_as_lazy: bool = False, symeig_dtype_evals: bool = False):
        """Per-factor eigendecompositions (reference :338-360): evals = Kronecker product of the factors' eigenvalues
        [*batch, N], evecs = Kronecker product of the factors' eigenvector matrices.  `symeig_dtype_evals` keeps the
        eigenvalues in `settings._linalg_dtype_symeig` (the closed-form solve shifts and inverts them there, like
        the reference's fp64 solve, kronecker_product_added_diag_linear_operator.py:147-161)."""
        from ..functions import _eigh

        evals, evecs = None, []
        for op in self.linear_ops:
            dense = op.to_dense()
            ev, q = _eigh.eigh(dense.to(dtype=settings._linalg_dtype_symeig.value()))
            ev = ev.clamp_min(0.0)
            if not symeig_dtype_evals:
                ev = ev.to(dtype=dense.dtype)
            evals = ev if evals is None else (evals.unsqueeze(-1) * ev.unsqueeze(-2)).reshape(*ev.shape[:-1], -1)
            evecs.append(DenseLinearOperator(q.to(dtype=dense.dtype)))
        return evals, (KroneckerProductLinearOperator(*evecs) if eigenvectors else None)

    def _diagonal(self) -> Tensor:
        return _kron_diag(*self.linear_ops)

    def _expand_batch(self, batch_shape):
        return self.__class__(*[op._expand_batch(batch_shape) for op in self.linear_ops])

    def _get_indices(self, row_index, col_index, *batch_indices) -> Tensor:  # reference :198-216
        row_factor, col_factor = self.size(-2), self.size(-1)
        res = None
        for op in self.linear_ops:
            nr, nc = op.size(-2), op.size(-1)
            row_factor //= nr
            col_factor //= nc
            sub = op._get_indices(
                torch.div(row_index, row_factor, rounding_mode="floor").fmod(nr),
                torch.div(col_index, col_factor, rounding_mode="floor").fmod(nc),
                *batch_indices,
            )
            res = sub if res is None else (sub * res)
        return res

    def _matmul(self, rhs: Tensor) -> Tensor:  # reference :272-284
        is_vec = rhs.ndimension() == 1
        if is_vec:
            rhs = rhs.unsqueeze(-1)
        if rhs.is_cuda and rhs.dtype == torch.float32 and self._kernel_kron_refusal() is None:
            T = self.linear_ops[1].shape[-1]
            if _NATIVE_MATMUL_KERNEL_KRON.get((T, 1 if rhs.shape[-1] == 1 else 2), False):
                bs = torch.broadcast_shapes(self.batch_shape, rhs.shape[:-2])
                desc = self._kernel_kron_descriptor(bs)
                res = K.kernel_kron_mv(desc.A0, desc.A1, desc.task, desc.n2,
                                       rhs.detach().expand(*bs, *rhs.shape[-2:]).reshape(-1, *rhs.shape[-2:]))
                res = res.reshape(*bs, *res.shape[-2:])
            else:  # (the per-factor composition; its kernel factor is matrix-free)
                res = _kron_matmul(self.linear_ops, self.shape, rhs.contiguous())
            return res.squeeze(-1) if is_vec else res
        desc = None
        if K.native_matmul_candidate(self, rhs) and (
                self._toeplitz_columns() is None
                or _NATIVE_MATMUL_TOEPLITZ.get((len(self.linear_ops), 1 if rhs.shape[-1] == 1 else 2), False)):
            desc = self._kernel_descriptor(torch.broadcast_shapes(self.batch_shape, rhs.shape[:-2]))
        if K.native_matmul(desc, rhs):
            res = K.matvec(desc, rhs.expand(*desc.batch_shape, *rhs.shape[-2:]))
        else:
            res = _kron_matmul(self.linear_ops, self.shape, rhs.contiguous())
        return res.squeeze(-1) if is_vec else res

    def _t_matmul(self, rhs):
        return self.mT._matmul(rhs)

    def _size(self) -> torch.Size:
        rows = 1
        cols = 1
        for op in self.linear_ops:
            rows *= op.size(-2)
            cols *= op.size(-1)
        return torch.Size((*self.linear_ops[0].batch_shape, rows, cols))

    def _transpose_nonbatch(self):
        return self.__class__(*(op._transpose_nonbatch() for op in self.linear_ops))

    def to_dense(self) -> Tensor:
        res = self.linear_ops[0].to_dense()
        for op in self.linear_ops[1:]:
            nxt = op.to_dense()
            res = (res.unsqueeze(-1).unsqueeze(-3) * nxt.unsqueeze(-2).unsqueeze(-4)).reshape(
                *res.shape[:-2], res.shape[-2] * nxt.shape[-2], res.shape[-1] * nxt.shape[-1])
        return res


class KroneckerProductDiagLinearOperator(DiagLinearOperator):
    """D_1 (x) .. (x) D_P of diagonal operators (reference :436-541): a diagonal whose N = prod n_i entries are never
    stored as leaves -- the representation is the factors' own tensors, so gradients reach the factors."""

    def __init__(self, *linear_ops):
        if not all(isinstance(op, DiagLinearOperator) for op in linear_ops):
            raise RuntimeError("Components of KroneckerProductDiagLinearOperator must be DiagLinearOperator.")
        LinearOperator.__init__(self, *linear_ops)
        self.linear_ops = linear_ops

    @property
    def _diag(self) -> Tensor:
        return _kron_diag(*self.linear_ops)

    def _size(self) -> torch.Size:
        shapes = [op._diag.shape for op in self.linear_ops]
        n = math.prod(sh[-1] for sh in shapes)
        return torch.Size((*torch.broadcast_shapes(*(sh[:-1] for sh in shapes)), n, n))

    def _expand_batch(self, batch_shape):
        return self.__class__(*[op._expand_batch(batch_shape) for op in self.linear_ops])

    def _mul_constant(self, other):  # (the product structure is not kept: one plain diagonal)
        return DiagLinearOperator(self._diag * other[..., None])

    def _bilinear_derivative(self, left_vecs: Tensor, right_vecs: Tensor):
        """sum_cols u o v is the gradient of the full diagonal [*batch, N]; factor i receives its contraction with the
        other factors' diagonals, handed to the factor's own rule (full / constant diagonal)."""
        g = K.bilinear_diag(left_vecs, right_vecs, self.batch_shape)
        diags = [op._diag for op in self.linear_ops]
        p = len(diags)
        g = g.reshape(*g.shape[:-1], *(dg.shape[-1] for dg in diags))
        idx = "abcdefgh"[:p]
        out = []
        for i, op in enumerate(self.linear_ops):
            if p == 1:
                gi = g
            else:
                others = ",".join(f"...{idx[j]}" for j in range(p) if j != i)
                gi = torch.einsum(f"...{idx},{others}->...{idx[i]}", g, *[diags[j] for j in range(p) if j != i])
            leaf = op.representation()[0]
            if leaf.shape[-1] == 1 and op._diag.shape[-1] != 1:  # constant factor: d(sigma) = sum of its diagonal's
                gi = gi.sum(-1, keepdim=True)
            out.append(gi if tuple(gi.shape) == tuple(leaf.shape) else gi.sum_to_size(*leaf.shape))
        return tuple(out)

    def abs(self):
        return self.__class__(*[op.abs() for op in self.linear_ops])

    def sqrt(self):
        return self.__class__(*[op.sqrt() for op in self.linear_ops])

    def inverse(self):
        return self.__class__(*[op.inverse() for op in self.linear_ops])

    def exp(self):
        raise NotImplementedError(f"torch.exp({self.__class__.__name__}) is not implemented.")

    def log(self):
        raise NotImplementedError(f"torch.log({self.__class__.__name__}) is not implemented.")


__all__ = ["KroneckerProductLinearOperator", "KroneckerProductDiagLinearOperator"]
