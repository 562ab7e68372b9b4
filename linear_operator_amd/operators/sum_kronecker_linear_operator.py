"""SumKroneckerLinearOperator: A_1 (x) .. (x) A_m + C_1 (x) .. (x) C_m, the covariance of a multitask GP with
Kronecker-structured noise K_data (x) K_task + Sigma_data (x) Sigma_task (reference:
operators/sum_kronecker_linear_operator.py:14-119; what `KroneckerProductLinearOperator.__add__` builds for two
Kronecker products of one factor layout, kronecker_product_linear_operator.py:107-111).

No CG and no stochastic logdet: closed forms on per-factor decompositions.  ONE formulation (the reference's
`_sum_formulation` with R = L_C^-T as the inverse root of C; any R with R R^T = C^-1 serves).  Per factor pair (A, C),
in `settings._linalg_dtype_symeig`, ATen plumbing like `KroneckerProductAddedDiagLinearOperator._symmetrized_eig`:
    C = L_C L_C^T,    At = L_C^-1 A L_C^-T = Q Lambda Q^T  (Lambda clamped at 0),    P = L_C^-T Q
so that P^T C P = I and P^T A P = Lambda, and with P = P_1 (x) .. (x) P_m, lambda = lambda_1 (x) .. (x) lambda_m:
    (A + C)^-1 = P diag(1 / (lambda + 1)) P^T                                                      (:42-66)
    logdet     = sum log1p(lambda) + sum_i (N / n_i) logdet C_i                                    (:68-73)
    root       = (P_1^-T (x) .. (x) P_m^-T) diag((lambda + 1)^1/2),   P_i^-T = L_Ci Q_i            (:75-84)
    inverse root = P diag((lambda + 1)^-1/2)                                                       (:86-95)
Two dense fp32 factors on the device take the native route: `_solve` is two calls of lo_kron_eig_apply_f32
(csrc/lo_kron_eigsolve.hip), (P_1^T, P_2, w) and (P_1, P_2^T, NULL) with w = 1 / (lambda + 1) -- both transposes of
the small matrices are kept from the set-up, so one kernel shape serves both halves.  More factors are regrouped into
two dense groups (`KroneckerProductLinearOperator._two_groups`); where that is not possible, and for float64 operators
and CPU tensors, P, w and P^T are applied through `KroneckerProductLinearOperator._matmul`.  The derivative of
`solve` / `inv_quad` is the inherited sum rule: the Kronecker bilinear kernels, once per term.  `_logdet` is
differentiable through the factors' Cholesky and eigh.  The roots are lazy `MatmulLinearOperator`s: the N x N factor is
never formed."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import kernels as K
from .. import settings
from .dense_linear_operator import DenseLinearOperator
from .diag_linear_operator import DiagLinearOperator
from .kronecker_product_linear_operator import KroneckerProductLinearOperator
from .sum_linear_operator import SumLinearOperator


def _kron_vec(vecs):
    """lambda_1 (x) .. (x) lambda_m for vectors [*batch, n_i] -> [*batch, N], the first factor slowest."""
    res = vecs[0]
    for v in vecs[1:]:
        res = (res.unsqueeze(-1) * v.unsqueeze(-2)).reshape(*res.shape[:-1], -1)
    return res


def sum_kron_factor_setup(a: Tensor, c: Tensor):
    """One factor pair in the dtype of the inputs: (P [*b, n, n], lambda [*b, n] clamped at 0, L_C [*b, n, n], Q) with
    P^T c P = I and P^T a P = diag(lambda).  Differentiable (Cholesky, triangular solves, eigh).  (Called in the symeig
    dtype, float64 unless `settings.linalg_dtypes` says otherwise: the batched float32 Cholesky of INTEGRATION.md
    section 5d is not on this path by default.)"""
    from ..functions import _eigh

    L = torch.linalg.cholesky(c)
    half = torch.linalg.solve_triangular(L, a, upper=False)  # L^-1 a
    at = torch.linalg.solve_triangular(L, half.mT, upper=False)  # L^-1 a^T L^-T
    ev, q = _eigh.eigh(0.5 * (at + at.mT))
    p = torch.linalg.solve_triangular(L.mT, q, upper=True)  # L^-T Q
    return p, ev.clamp_min(0.0), L, q


class SumKroneckerLinearOperator(SumLinearOperator):
    _has_closed_form_solve = True  # functions/_solve._solve: the eigenbasis form at every size

    def __init__(self, *linear_ops, **kwargs):
        if len(linear_ops) != 2 or not all(isinstance(op, KroneckerProductLinearOperator) for op in linear_ops):
            raise RuntimeError("SumKroneckerLinearOperator takes exactly two KroneckerProductLinearOperators")
        first, second = linear_ops
        if len(first.linear_ops) != len(second.linear_ops):
            raise RuntimeError(
                f"SumKroneckerLinearOperator: {len(first.linear_ops)} factors against {len(second.linear_ops)}")
        for a, c in zip(first.linear_ops, second.linear_ops):
            if a.shape[-2:] != c.shape[-2:] or a.shape[-1] != a.shape[-2]:
                raise RuntimeError("SumKroneckerLinearOperator: the factors of both products must be square and of "
                                   f"equal shapes, got {tuple(a.shape)} and {tuple(c.shape)}")
        super().__init__(*linear_ops, **kwargs)
        self._eig_cache = None

    # ------------------------------------------------------------------ set-up
    def _factor_setup(self, detach: bool):
        """Per factor pair (P, lambda, L_C, Q) in the symeig dtype."""
        dt = settings._linalg_dtype_symeig.value()
        out = []
        for a_op, c_op in zip(self.linear_ops[0].linear_ops, self.linear_ops[1].linear_ops):
            a, c = a_op.to_dense(), c_op.to_dense()
            if detach:
                a, c = a.detach(), c.detach()
            out.append(sum_kron_factor_setup(a.to(dt), c.to(dt)))
        return out

    def _setup(self):
        """The detached set-up of the solve, cached on the object: (mats, mats_t, w, P, P^T) -- the two matrices of
        the native route with their transposes (None when the operator does not take it), w = 1 / (lambda + 1)
        [*batch, N] and the Kronecker operators P, P^T of the composition, all in the operator's dtype."""
        if self._eig_cache is None:
            with torch.no_grad():
                parts = self._factor_setup(detach=True)
                w = (_kron_vec([ev for _, ev, _, _ in parts]) + 1.0).reciprocal().to(self.dtype)
                ps = [p.to(self.dtype).contiguous() for p, _, _, _ in parts]
                p_op = KroneckerProductLinearOperator(*ps)
                pt_op = KroneckerProductLinearOperator(*[p.mT.contiguous() for p in ps])
                mats = mats_t = None
                if self.dtype == torch.float32 and all(p.is_cuda for p in ps):
                    groups = p_op._two_groups()  # (two factors: the factors themselves)
                    if groups is not None:
                        mats = (groups[0].contiguous(), groups[1].contiguous())
                        mats_t = (mats[0].mT.contiguous(), mats[1].mT.contiguous())
            self._eig_cache = (mats, mats_t, w, p_op, pt_op)
        return self._eig_cache

    # ------------------------------------------------------------------ solve
    def _solve(self, rhs: Tensor, preconditioner=None, num_tridiag: int = 0):
        is_vec = rhs.dim() == 1
        if is_vec:
            rhs = rhs.unsqueeze(-1)
        mats, mats_t, w, p_op, pt_op = self._setup()
        res = None
        if mats is not None and rhs.is_cuda and rhs.dtype == torch.float32:
            half = K.kron_eig_apply(mats_t[0], mats[1], w, rhs)  # w o (P^T rhs)
            if half is not None:
                res = K.kron_eig_apply(mats[0], mats_t[1], None, half)  # P (..)
        if res is None:
            res = p_op._matmul(w.unsqueeze(-1) * pt_op._matmul(rhs))
        return res.squeeze(-1) if is_vec else res

    def _solve_preconditioner(self):
        return None

    def _preconditioner(self):  # (solves and the logdet are closed forms: nothing to precondition)
        return None, None, None

    # ------------------------------------------------------------------ logdet / inv_quad_logdet
    def _logdet(self) -> Tensor:
        """Differentiable through the factors' Cholesky and eigh, in the symeig dtype."""
        parts = self._factor_setup(detach=False)
        N = self.size(-1)
        res = torch.log1p(_kron_vec([ev for _, ev, _, _ in parts])).sum(-1)
        for _, _, L, _ in parts:
            n = L.shape[-1]
            res = res + (N // n) * 2.0 * L.diagonal(dim1=-2, dim2=-1).log().sum(-1)
        return res.to(self.dtype)

    def inv_quad_logdet(self, inv_quad_rhs=None, logdet: bool = False, reduce_inv_quad: bool = True):  # :97-119
        inv_quad_term = logdet_term = None
        if inv_quad_rhs is not None:
            solve = self.solve(inv_quad_rhs)
            inv_quad_term = (inv_quad_rhs * solve).sum(-2)
            if inv_quad_term.numel() and reduce_inv_quad:
                inv_quad_term = inv_quad_term.sum(-1)
        if logdet:
            logdet_term = self._logdet()
        return inv_quad_term, logdet_term

    # ------------------------------------------------------------------ lazy roots (:75-95)
    def _eig_root(self, power: float):
        from .matmul_linear_operator import MatmulLinearOperator

        with torch.no_grad():
            parts = self._factor_setup(detach=True)
            scale = (_kron_vec([ev for _, ev, _, _ in parts]) + 1.0).pow(power).to(self.dtype)
            if power > 0:  # P^-T = L_C Q
                mats = [(L @ q).to(self.dtype) for _, _, L, q in parts]
            else:
                mats = [p.to(self.dtype) for p, _, _, _ in parts]
        basis = KroneckerProductLinearOperator(*[DenseLinearOperator(m.contiguous()) for m in mats])
        return MatmulLinearOperator(basis, DiagLinearOperator(scale))

    def _root_decomposition(self):
        return self._eig_root(0.5)

    def _root_inv_decomposition(self, initial_vectors=None, test_vectors=None):
        return self._eig_root(-0.5)

    def _choose_root_method(self) -> str:
        # the closed forms hold at every size: the exact branch of small operators (dense Cholesky of N x N) is not needed
        return "lanczos"  # (the name of the branch that calls `_root_decomposition`, reference :2190-2199)

    # ------------------------------------------------------------------ what leaves the class
    def _mul_constant(self, other):  # (a scaled Kronecker product is not one: a plain sum of the scaled terms)
        return SumLinearOperator(*(op._mul_constant(other) for op in self.linear_ops))


__all__ = ["SumKroneckerLinearOperator", "sum_kron_factor_setup"]
