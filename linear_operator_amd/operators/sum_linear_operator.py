"""SumLinearOperator / PsdSumLinearOperator (reference: operators/sum_linear_operator.py:16-116,
operators/psd_sum_linear_operator.py:10-18)."""
from __future__ import annotations

import torch
from torch import Tensor

from ._linear_operator import LinearOperator
from .dense_linear_operator import to_linear_operator


def _common_shape(shapes):
    """torch.broadcast_shapes, with the usual case (all terms already have one shape) answered without it: the torch
    helper costs ~15 us per call and the solve path builds several sums per call (detach, representation trees)."""
    first = shapes[0]
    if all(s == first for s in shapes[1:]):
        return torch.Size(first)
    return torch.broadcast_shapes(*shapes)


def _flatten_terms(ops):
    """The terms of a sum with nested sums flattened, left to right (AddedDiag is a sum of its operator and its diagonal)."""
    flat = []
    for op in ops:
        if isinstance(op, SumLinearOperator):
            flat.extend(_flatten_terms(op.linear_ops))
        else:
            flat.append(op)
    return flat


def _kernel_groups(ops, check_device: bool = True):
    """Partition the (flattened, diagonal-free) terms `ops` for the lowering: native KernelLinearOperators over the SAME
    points tensor (x1 and x2 one tensor, and that tensor shared across the operators) form a group of up to
    LO_KERNEL_MAX_TERMS -- one pass of csrc/lo_kernel_sum.hip; a larger group splits into several.  Returns the items in
    the order of their first member: a list of operators for a group (one member: that operator lowers on its own), the
    operator itself for anything else.  `check_device=False` leaves the float32-on-the-device condition out of the gate."""
    from .. import _hip
    from .kernel_linear_operator import KernelLinearOperator, _same_tensor

    items, open_groups = [], []
    for op in ops:
        if (isinstance(op, KernelLinearOperator) and op._native_refusal(check_device) is None and op._same_points()):
            for grp in open_groups:
                if len(grp) < _hip.LO_KERNEL_MAX_TERMS and _same_tensor(grp[0].x1, op.x1):
                    grp.append(op)
                    break
            else:
                grp = [op]
                open_groups.append(grp)
                items.append(grp)
        else:
            items.append(op)
    return items


def _term_descriptor(op, batch_shape):
    """The descriptor of one operator as a term of a lowering: its `_kernel_descriptor`, or -- a float64
    KernelLinearOperator, whose own `_kernel_descriptor()` stays None -- its `_kernel_descriptor_f64`."""
    desc = op._kernel_descriptor(batch_shape)
    if desc is None and hasattr(op, "_kernel_descriptor_f64"):
        desc = op._kernel_descriptor_f64(batch_shape)
    return desc


def _kernel_group_pair(ops):
    """The operators themselves when ALL of `ops` (two or more, at most LO_KERNEL_MAX_TERMS) are native
    KernelLinearOperators over one (x1, x2) pair -- square or rectangular: one fused product or derivative serves the whole
    sum.  Else None."""
    from .. import _hip
    from .kernel_linear_operator import KernelLinearOperator, _same_tensor

    if not 2 <= len(ops) <= _hip.LO_KERNEL_MAX_TERMS:
        return None
    first = ops[0]
    for op in ops:
        if not (isinstance(op, KernelLinearOperator) and op._is_native() and _same_tensor(op.x1, first.x1)
                and _same_tensor(op.x2, first.x2)):
            return None
    return list(ops)


def _group_theta(group, batch_shape):
    from .. import kernels as K

    return K.kernel_sum_theta([op.tensor_params["lengthscale"] for op in group],
                              [op.tensor_params["outputscale"] for op in group], batch_shape, group[0].x1.shape[-1])


def _group_families(group):
    return [op.covar_func.native_family for op in group]


def _group_descriptor(group, batch_shape):
    """The descriptor of one item of _kernel_groups that is a group."""
    from .. import kernels as K

    if len(group) == 1:
        return group[0]._kernel_descriptor(batch_shape)
    X = group[0].x1.detach()
    X = X if X.shape[:-2] == batch_shape else X.expand(*batch_shape, *X.shape[-2:])
    return K.kernel_sum_diag_descriptor(X, _group_theta(group, batch_shape), _group_families(group))


def _lmc_terms(ops, check_device: bool = True):
    """The terms themselves when ALL of `ops` (the flattened, diagonal-free terms of a sum) are 2 .. LO_KERNEL_MAX_TERMS
    matrix-free multitask products Kron(Kernel_q(X, X), Dense(B_q)) (`_kernel_kron_refusal`) whose kernel factors are over
    the SAME points tensor, with one T and one batch: the linear model of coregionalisation, one pass of
    csrc/lo_kernel_lmc.hip.  Else None.  `check_device=False` leaves the on-the-device conditions out of the gate."""
    from .. import _hip
    from .kernel_linear_operator import _same_tensor
    from .kronecker_product_linear_operator import KroneckerProductLinearOperator

    if not 2 <= len(ops) <= _hip.LO_KERNEL_MAX_TERMS:
        return None
    for op in ops:
        if not isinstance(op, KroneckerProductLinearOperator) or op._kernel_kron_refusal(check_device) is not None:
            return None
    kern0, task0 = ops[0].linear_ops
    for op in ops[1:]:
        kern, task = op.linear_ops
        if not (_same_tensor(kern.x1, kern0.x1) and task.shape[-1] == task0.shape[-1]
                and op.batch_shape == ops[0].batch_shape):
            return None
    return list(ops)


def _lmc_descriptor(terms, batch_shape):
    """The diagonal-free LO_OP_KERNEL_LMC_DIAG descriptor of the terms of _lmc_terms at `batch_shape`."""
    from .. import kernels as K

    kerns = [op.linear_ops[0] for op in terms]
    X = kerns[0].x1.detach()
    X = X if X.shape[:-2] == batch_shape else X.expand(*batch_shape, *X.shape[-2:])
    Bt = torch.stack([op.linear_ops[1].tensor.detach().expand(*batch_shape, *op.linear_ops[1].shape[-2:])
                      for op in terms], -3)
    return K.kernel_lmc_diag_descriptor(X, _group_theta(kerns, batch_shape), _group_families(kerns), Bt)


class SumLinearOperator(LinearOperator):
    def __init__(self, *linear_ops, **kwargs):
        try:
            linear_ops = tuple(to_linear_operator(lt) for lt in linear_ops)
        except TypeError:
            raise TypeError("All arguments of a SumLinearOperator should be LinearOperators or Tensors")
        batch_shape = _common_shape([lt.batch_shape for lt in linear_ops])
        linear_ops = tuple(lt._expand_batch(batch_shape) if lt.batch_shape != batch_shape else lt for lt in linear_ops)
        super().__init__(*linear_ops, **kwargs)
        self.linear_ops = linear_ops

    def _kernel_descriptor(self, batch_shape=None):
        """Lowering of the sum (reference `_matmul` :47-51, `_diagonal` :31-32): one structured term + at most one
        diagonal lowers like AddedDiag; 2 .. LO_MAX_TERMS structured terms (nested sums flattened, left to right)
        + at most one diagonal lower to an LO_OP_SUM descriptor -- matvec, CG, Lanczos, MINRES and the pivoted
        Cholesky then run on the device without per-term Python calls.  Native KernelLinearOperators over the same points
        tensor count as ONE term (_kernel_groups): LO_OP_KERNEL_SUM_DIAG, the descriptor itself when they are the whole
        sum apart from the diagonal; a rational-quadratic or periodic KernelLinearOperator (LO_OP_KERNEL_PARAM_DIAG) and a
        spectral-mixture one (LO_OP_KERNEL_SM_DIAG) are terms of their own.  2 .. LO_KERNEL_MAX_TERMS matrix-free multitask products Kron(Kernel_q, Dense(B_q)) over
        one points tensor (_lmc_terms) that are the whole sum apart from the diagonal lower to LO_OP_KERNEL_LMC_DIAG."""
        from .. import kernels as K
        from .diag_linear_operator import DiagLinearOperator

        batch_shape = torch.Size(self.batch_shape if batch_shape is None else batch_shape)
        flat = _flatten_terms(self.linear_ops)
        diags = [op for op in flat if isinstance(op, DiagLinearOperator)]
        others = [op for op in flat if not isinstance(op, DiagLinearOperator)]
        if len(diags) > 1 or not others:
            return None
        if len(others) == 1:
            return _attach_diag(others[0], diags[0] if diags else None, batch_shape)
        lmc = _lmc_terms(others)
        if lmc is not None:
            desc = _lmc_descriptor(lmc, batch_shape)
            return None if desc is None else _sum_with_diag(desc, diags[0] if diags else None, batch_shape)
        items = _kernel_groups(others)
        if len(items) > K._hip.LO_MAX_TERMS:
            return None
        terms = []
        for item in items:
            desc = _group_descriptor(item, batch_shape) if isinstance(item, list) else _term_descriptor(item, batch_shape)
            if desc is None or desc.diag_mode != 0 or desc.kind not in (
                    K._hip.LO_OP_LOWRANK_DIAG, K._hip.LO_OP_DENSE_DIAG, K._hip.LO_OP_KRON_DIAG, K._hip.LO_OP_KERNEL_DIAG,
                    K._hip.LO_OP_KERNEL_SUM_DIAG, K._hip.LO_OP_KERNEL_PARAM_DIAG, K._hip.LO_OP_KERNEL_SM_DIAG):
                return None  # (a sum's terms: low-rank / dense / Kronecker / kernel; SKI and Toeplitz terms take the closure)
            terms.append(desc)
        if len(terms) == 1:  # the kernel group is the whole sum
            return _sum_with_diag(terms[0], diags[0] if diags else None, batch_shape)
        if len({(t.B, t.N, t.dtype) for t in terms}) != 1:
            return None
        return _sum_with_diag(K.sum_descriptor(terms, dtype=terms[0].dtype), diags[0] if diags else None, batch_shape)

    def _diagonal(self) -> Tensor:
        return sum(op._diagonal() for op in self.linear_ops)

    def _expand_batch(self, batch_shape):
        return self.__class__(*[op._expand_batch(batch_shape) for op in self.linear_ops])

    def _get_indices(self, row_index, col_index, *batch_indices) -> Tensor:
        return sum(op._get_indices(row_index, col_index, *batch_indices) for op in self.linear_ops)

    def _matmul(self, rhs: Tensor) -> Tensor:  # reference :47-51
        from .. import kernels as K

        if K.native_matmul_candidate(self, rhs):
            desc = self._kernel_descriptor(torch.broadcast_shapes(self.batch_shape, rhs.shape[:-2]))
            if K.native_matmul(desc, rhs):
                return K.matvec(desc, rhs.expand(*desc.batch_shape, *rhs.shape[-2:]))
            if desc is None and rhs.dtype == torch.float32:  # e.g. the prediction product K(x*, X) alpha
                group = _kernel_group_pair(self.linear_ops)
                if group is not None:
                    return _group_matmul(group, rhs)
        return sum(op._matmul(rhs) for op in self.linear_ops)

    def _bilinear_derivative(self, left_vecs: Tensor, right_vecs: Tensor):  # reference :59-62
        if left_vecs.is_cuda and left_vecs.dtype == torch.float32:
            group = _kernel_group_pair(self.linear_ops)
            if group is not None:
                return _group_bilinear_derivative(group, left_vecs, right_vecs)
        return tuple(var for op in self.linear_ops for var in op._bilinear_derivative(left_vecs, right_vecs))

    def _t_matmul(self, rhs):
        if rhs.dim() >= 2 and rhs.is_cuda and rhs.dtype == torch.float32:
            group = _kernel_group_pair(self.linear_ops)
            if group is not None:
                return _group_matmul([op._transpose_nonbatch() for op in group], rhs)
        return sum(op._t_matmul(rhs) for op in self.linear_ops)

    def _mul_constant(self, other):  # c (A + B) = c A + c B, each term scaled its own way
        return type(self)(*(op._mul_constant(other) for op in self.linear_ops))

    def _size(self) -> torch.Size:
        return _common_shape([op.shape for op in self.linear_ops])

    def _transpose_nonbatch(self):
        return self.__class__(*[op.mT for op in self.linear_ops])

    def to_dense(self) -> Tensor:
        return sum(op.to_dense() for op in self.linear_ops).contiguous()

    def __add__(self, other):  # reference :88-116
        from .added_diag_linear_operator import AddedDiagLinearOperator
        from .diag_linear_operator import DiagLinearOperator

        if isinstance(other, DiagLinearOperator):
            return AddedDiagLinearOperator(self, other)
        if isinstance(other, SumLinearOperator):
            return SumLinearOperator(*(list(self.linear_ops) + list(other.linear_ops)))
        if isinstance(other, LinearOperator):
            return SumLinearOperator(*(list(self.linear_ops) + [other]))
        if isinstance(other, Tensor):
            shape = torch.broadcast_shapes(self.shape, other.shape)
            new_self = self if shape == self.shape else self._expand_batch(shape[:-2])
            return SumLinearOperator(*(list(new_self.linear_ops) + [to_linear_operator(other.expand(shape))]))
        raise AttributeError("other must be a LinearOperator")


class PsdSumLinearOperator(SumLinearOperator):
    """A sum of positive semi-definite terms: samples add (reference psd_sum_linear_operator.py:15-18)."""

    def zero_mean_mvn_samples(self, num_samples: int) -> Tensor:
        return sum(op.zero_mean_mvn_samples(num_samples) for op in self.linear_ops)


def _group_operands(group, bs):
    """(x1 [B, M, D], x2 [B, N, D], theta [B, T, D + 1], families) of a group of _kernel_group_pair at the batch `bs`."""
    first = group[0]
    M, D = first.x1.shape[-2:]
    N = first.x2.shape[-2]
    x1 = first.x1.detach().expand(*bs, M, D).reshape(-1, M, D)
    x2 = x1 if first._same_points() else first.x2.detach().expand(*bs, N, D).reshape(-1, N, D)
    return x1, x2, _group_theta(group, bs), _group_families(group)


def _group_matmul(group, rhs: Tensor) -> Tensor:
    """(sum_t K_t(x1, x2)) rhs in one pass (lo_kernel_sum_mv_f32); x1 / x2 rectangular or not."""
    from .. import kernels as K

    M = group[0].x1.shape[-2]
    N, c = rhs.shape[-2:]
    bs = torch.broadcast_shapes(group[0].batch_shape, rhs.shape[:-2])
    x1, x2, theta, fams = _group_operands(group, bs)
    y = K.kernel_sum_mv(x1, x2, theta, fams, rhs.detach().expand(*bs, N, c).reshape(-1, N, c))
    return y.reshape(*bs, M, c)


def _group_bilinear_derivative(group, left_vecs: Tensor, right_vecs: Tensor):
    """The derivatives of sum_s u_s^T (sum_t K_t) v_s in the order of SumLinearOperator._bilinear_derivative -- per
    operator (x1, x2, parameters in sorted order): every term's theta gradient from ONE lo_kernel_sum_bilinear_f32 call,
    mapped to lengthscale / outputscale as KernelLinearOperator._bilinear_derivative_native does; the points' gradient,
    summed over the terms, from one lo_kernel_sum_points_grad_f32 call per side, placed in the first operator's slot
    (the operators share the leaf: autograd adds the slots).  Where the fused sweep was measured slower than the
    single-term kernels (K.kernel_sum_fused_bilinear / _points_grad) the same quantities come from one single-term call
    per term.  covar_func is never called."""
    from .. import kernels as K

    if left_vecs.dim() == 1:
        left_vecs, right_vecs = left_vecs.unsqueeze(-1), right_vecs.unsqueeze(-1)
    first = group[0]
    M, D = first.x1.shape[-2:]
    N, t = right_vecs.shape[-2:]
    bs = torch.broadcast_shapes(first.batch_shape, left_vecs.shape[:-2], right_vecs.shape[:-2])
    names = [list(op._differentiable_kwargs) for op in group]
    params = [(op.tensor_params["lengthscale"], op.tensor_params["outputscale"]) for op in group]
    need_theta = any(p.requires_grad for pair in params for p in pair)
    need_x1 = any(op.x1.requires_grad for op in group)
    need_x2 = any(op.x2.requires_grad for op in group)
    outs = [{"x1": None, "x2": None, "lengthscale": None, "outputscale": None} for _ in group]
    if need_theta or need_x1 or need_x2:
        x1, x2, theta, fams = _group_operands(group, bs)
        U = left_vecs.detach().expand(*bs, M, t).reshape(-1, M, t)
        V = right_vecs.detach().expand(*bs, N, t).reshape(-1, N, t)
        T = len(group)

        def points_grad(a, b, left, right):
            if K.kernel_sum_fused_points_grad(D, T):
                return K.kernel_sum_points_grad(a, b, theta, fams, left, right)
            return sum(K.kernel_points_grad(a, b, theta[:, k], fams[k], left, right) for k in range(T))

        if need_theta:
            if K.kernel_sum_fused_bilinear(D, T):
                g = K.kernel_sum_bilinear(x1, x2, theta, fams, U, V)  # [B, T, D + 1]
            else:
                g = torch.stack([K.kernel_bilinear(x1, x2, theta[:, k], fams[k], U, V) for k in range(T)], 1)
            for k, (ls, os_) in enumerate(params):
                if ls.requires_grad:  # theta_d = 1 / l_d: d / d l_d = -theta_d^2 d / d theta_d; a shared l sums over d
                    d_ls = (-(theta[:, k, :D] ** 2) * g[:, k, :D]).reshape(*bs, 1, D)
                    if ls.shape[-1] == 1 and D > 1:
                        d_ls = d_ls.sum(-1, keepdim=True)
                    outs[k]["lengthscale"] = d_ls.sum_to_size(ls.shape)
                if os_.requires_grad:  # theta_D = os^2: d / d os = 2 os d / d theta_D
                    outs[k]["outputscale"] = (2.0 * torch.broadcast_to(os_.detach(), tuple(bs))
                                              * g[:, k, D].reshape(tuple(bs))).sum_to_size(os_.shape)
        # each side with the other held fixed, summed over the terms; the x2 side is the x1 side of the transposed problem
        if need_x1:
            slot = next(k for k, op in enumerate(group) if op.x1.requires_grad)
            outs[slot]["x1"] = points_grad(x1, x2, U, V).reshape(*bs, M, D).sum_to_size(
                group[slot].x1.shape)
        if need_x2:
            slot = next(k for k, op in enumerate(group) if op.x2.requires_grad)
            outs[slot]["x2"] = points_grad(x2, x1, V, U).reshape(*bs, N, D).sum_to_size(
                group[slot].x2.shape)
    return tuple(var for out, nm in zip(outs, names) for var in (out["x1"], out["x2"], *(out[n] for n in nm)))


def _attach_diag(base_op, diag_op, batch_shape):
    """Descriptor of `base_op (+ diag_op)` expanded to batch_shape, or None."""
    desc = _term_descriptor(base_op, batch_shape)
    if desc is None or desc.diag_mode != 0:
        return None
    return _sum_with_diag(desc, diag_op, batch_shape)


def _sum_with_diag(desc, diag_op, batch_shape):
    """Attach a (Constant)DiagLinearOperator to a diagonal-free descriptor, or None if its tensor cannot be used."""
    from .diag_linear_operator import ConstantDiagLinearOperator

    if diag_op is None:
        return desc
    from .. import kernels as K

    if isinstance(diag_op, ConstantDiagLinearOperator):
        vals = diag_op.diag_values
        if not (vals.is_cuda and vals.dtype == desc.dtype):
            return None
        return K._with_diag(desc, vals.expand(*batch_shape, 1)[..., 0], True)
    d = diag_op._diag
    if not (d.is_cuda and d.dtype == desc.dtype):
        return None
    return K._with_diag(desc, d.expand(*batch_shape, d.shape[-1]), False)


__all__ = ["SumLinearOperator", "PsdSumLinearOperator"]
