"""AddedDiagLinearOperator `A + D` with the pivoted-Cholesky / Woodbury preconditioner
(reference: linear_operator/operators/added_diag_linear_operator.py:21-209).

  _matmul          y = A v + d o v in ONE fused kernel (reference :72-76 is addcmul over A._matmul)
  _preconditioner  (:95-142) pivoted Cholesky of the non-diagonal part on the device (csrc/lo_pivchol.hip), then the
                   cached form (Q, 1/d, log|P|) from csrc/lo_precond.hip instead of torch.linalg.qr (:144-184);
                   returns the same triple (closure, PsdSum(Root(L), D), logdet_p).  The closure object carries the
                   device preconditioner so that linear_cg applies it natively inside the CG loop.
"""
from __future__ import annotations

import warnings
from typing import Callable, Optional

import torch
from torch import Tensor

from .. import kernels as K
from .. import settings
from ..utils.warnings import NumericalWarning
from .diag_linear_operator import DiagLinearOperator
from .root_linear_operator import RootLinearOperator
from .sum_linear_operator import PsdSumLinearOperator, SumLinearOperator, _attach_diag


class WoodburyPreconditionClosure:
    """precondition_closure (reference :135-140): z = r / d - Q (Q^T r)  (or (r - Q Q^T r) / sigma)."""

    def __init__(self, woodbury: K.WoodburyPreconditioner, batch_shape):
        self.woodbury = woodbury
        self.batch_shape = torch.Size(batch_shape)

    def __call__(self, tensor: Tensor) -> Tensor:
        is_vec = tensor.dim() == 1
        t = tensor.unsqueeze(-1) if is_vec else tensor
        t = t.expand(*self.batch_shape, *t.shape[-2:]) if t.shape[:-2] != self.batch_shape else t
        z = K.precond_apply(self.woodbury, t)
        return z.squeeze(-1) if is_vec else z


class DensePreconditionClosure:
    """The same closure for float64 operators, evaluated as the reference does (two GEMMs and an elementwise scaling on
    the device, :135-140): Q [*batch, N, k] and the noise are float64 tensors; `woodbury` is None.  The float64
    `linear_cg` recognises the class and applies it natively (`native_operands`); float32 preconditioners of rank > 128
    take the same class and are called back per iteration."""

    woodbury = None

    def __init__(self, q, noise, constant_diag):
        self.q, self.constant_diag = q, bool(constant_diag)
        self.noise = noise.unsqueeze(-1)  # [*batch, N | 1, 1]

    def native_operands(self):
        """(Q, noise [*batch, N | 1], constant_diag): what `linear_cg` hands to K.cg_solve_f64(precond=...), which then
        applies this closure inside the library (lo_precond_desc_cb_f64) instead of calling it back per iteration."""
        return self.q, self.noise[..., 0], self.constant_diag

    def __call__(self, tensor: Tensor) -> Tensor:
        is_vec = tensor.dim() == 1
        t = tensor.unsqueeze(-1) if is_vec else tensor
        qqt = self.q @ (self.q.mT @ t)
        z = (t - qqt) / self.noise if self.constant_diag else t / self.noise - qqt
        return z.squeeze(-1) if is_vec else z


def _rebuild_full_preconditioner(owner):
    """The full (L, Q) preconditioner of `owner` for a root-form-only one that has to grow a Q (ensure_q)."""
    closure = owner._preconditioner()[0]
    if closure is None:
        raise K._hip.HipExtensionError("the preconditioner could not be rebuilt (NaN in the pivoted Cholesky factor)")
    return closure.woodbury


class LazyWoodburyPreconditionClosure:
    """What `_solve_preconditioner` hands to `_solve` when the operator qualifies for the ONE-LAUNCH end-to-end solve
    (csrc/lo_solve_fused_impl.h): the same closure as `_preconditioner()[0]`, but nothing is factorised yet.
    `utils.linear_cg` recognises it (attribute `lazy_fused`) and, when its `matmul_closure` is the `_matmul` of the very
    operator this closure belongs to, runs pivoted Cholesky -> root-form preconditioner -> CG in one resident kernel and
    hands the root form back through `adopt` (memoised for later solves with the same tensors).  Any other use --
    calling it, asking for `.woodbury`, a CG call the fused kernel does not take -- materialises the ordinary
    preconditioner first, so the object is a drop-in for the reference's closure (added_diag_linear_operator.py:135-140).
    """

    lazy_fused = True

    def __init__(self, owner, desc, rank, tol, memo_key, memo_tensors):
        self._owner, self.desc, self.rank, self.tol = owner, desc, int(rank), float(tol)
        self._memo_key, self._memo_tensors = memo_key, memo_tensors
        self.batch_shape = torch.Size(owner.batch_shape)
        self._real = None
        self._done = False

    @property
    def pending(self) -> bool:
        return not self._done

    def owns(self, matmul_closure, batch_shape) -> bool:
        """True if `matmul_closure` is the (unpatched) bound `_matmul` of the operator this closure belongs to and the
        right-hand side carries the operator's own batch shape: the stored descriptor is the closure's lowering."""
        return (getattr(matmul_closure, "__self__", None) is self._owner
                and getattr(matmul_closure, "__func__", None) is type(self._owner)._matmul
                and batch_shape == self.batch_shape)

    def same_operator(self, desc) -> bool:
        """True if `desc` (lowered from linear_cg's matmul_closure) is this closure's operator: same tensors."""
        mine = self.desc
        return (desc is not None and desc.kind == mine.kind and desc.diag_mode == mine.diag_mode
                and desc.A0 is not None and desc.d is not None and (desc.B, desc.N, desc.R) == (mine.B, mine.N, mine.R)
                and desc.A0.data_ptr() == mine.A0.data_ptr() and desc.d.data_ptr() == mine.d.data_ptr())

    def materialize(self):
        """The ordinary closure (three-launch build through `_preconditioner`), or None (NaN in the factor: the
        reference continues without a preconditioner, :126-131)."""
        if not self._done:
            self._real, self._done = self._owner._preconditioner()[0], True
        return self._real

    def adopt(self, woodbury):
        """Root-form preconditioner the fused solve built on the way: becomes this closure's preconditioner and is
        memoised under the operator's tensors for later solves (a later call that needs Q or L rebuilds in full)."""
        # (the rebuild hook references the OPERATOR, not this closure: closure -> woodbury -> hook -> closure would be a
        # reference cycle, and the device tensors of every solve would wait for the cyclic collector -- the caching
        # allocator then has to hipMalloc fresh blocks: + 130 us per solve of 64 members)
        owner = self._owner
        woodbury.rebuild = lambda: _rebuild_full_preconditioner(owner)
        self._real = WoodburyPreconditionClosure(woodbury, self.batch_shape)
        self._done = True
        if PRECONDITIONER_MEMO_SIZE > 0 and self._memo_key is not None:
            _rootform_memo.insert(0, (self._memo_key, self._memo_tensors, woodbury))
            del _rootform_memo[PRECONDITIONER_MEMO_SIZE:]

    @property
    def woodbury(self):
        real = self.materialize()
        return None if real is None else real.woodbury

    def __call__(self, tensor: Tensor) -> Tensor:
        real = self.materialize()
        return tensor.clone() if real is None else real(tensor)


# Memo of the last preconditioners, keyed on the operator's tensors (address, version counter, layout) and the settings
# that shape the factorisation.  The reference caches the preconditioner on the operator OBJECT, but its autograd
# Functions rebuild the operator from its tensors (functions/_solve.py:40), so a solve followed by a logdet, or the
# solve inside Solve.backward, each factorise again; here those calls hit the memo.  The entry keeps the tensors alive
# (so an address cannot be reused by other data) and any in-place update bumps the version counter.
PRECONDITIONER_MEMO_SIZE = 2
_LAZY_Q = object()  # AddedDiagLinearOperator._q_cache of a root-form preconditioner whose Q has not been asked for
_precond_memo: "list[tuple]" = []
# root-form-only preconditioners the fused end-to-end solve produced (no L, no Q): enough for later SOLVES with the
# same tensors; `_preconditioner()` (probe sampling, logdet terms) ignores them and builds in full
_rootform_memo: "list[tuple]" = []


def _memo_key(tensors, extra):
    """None when a tensor cannot be keyed (inference tensors do not track a version counter): the memo is skipped.
    Writes through `.data` do not bump the version counter -- call clear_preconditioner_memo() after such updates."""
    if any(t.is_inference() for t in tensors):
        return None
    # a preconditioner built under distributed.global_stopping_rule carries the rank ALL shards agreed on (a collective
    # ran while it was built): it must not be confused with one built outside the context or under another group, and
    # every rank has to take the same hit / miss decision -- no memo at all inside the context
    from .. import distributed

    if distributed.active_stop_reduce() is not None:
        return None
    return tuple((t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride()), t.dtype) for t in tensors) + extra


def clear_preconditioner_memo():
    """Drop the memoised preconditioners (and the references to the tensors they were built from)."""
    _precond_memo.clear()
    _rootform_memo.clear()


class AddedDiagLinearOperator(SumLinearOperator):
    def __init__(self, *linear_ops, preconditioner_override: Optional[Callable] = None):
        linear_ops = list(linear_ops)
        super().__init__(*linear_ops, preconditioner_override=preconditioner_override)
        if len(linear_ops) > 2:
            raise RuntimeError("An AddedDiagLinearOperator can only have two components")
        a, b = self.linear_ops
        if isinstance(a, DiagLinearOperator) and isinstance(b, DiagLinearOperator):
            raise RuntimeError(
                "Trying to lazily add two DiagLinearOperators. Create a single DiagLinearOperator instead."
            )
        elif isinstance(a, DiagLinearOperator):
            self._diag_tensor, self._linear_op = a, b
        elif isinstance(b, DiagLinearOperator):
            self._diag_tensor, self._linear_op = b, a
        else:
            raise RuntimeError(
                "One of the LinearOperators input to AddedDiagLinearOperator must be a DiagLinearOperator!"
            )
        self.preconditioner_override = preconditioner_override
        # caches (reference :63-70); they live on the rebuilt, detached operator, not on the user's object
        self._constant_diag = None
        self._noise = None
        self._piv_chol_self = None
        self._piv_chol_perm = None
        self._precond_lt = None
        self._precond_logdet_cache = None
        self._q_cache = None
        self._woodbury = None

    def _kernel_descriptor(self, batch_shape=None):
        return _attach_diag(self._linear_op, self._diag_tensor,
                            torch.Size(self.batch_shape if batch_shape is None else batch_shape))

    def _matmul(self, rhs: Tensor) -> Tensor:
        if K.native_matmul_candidate(self, rhs):
            desc = self._kernel_descriptor(torch.broadcast_shapes(self.batch_shape, rhs.shape[:-2]))
            if K.native_matmul(desc, rhs):
                return K.matvec(desc, rhs.expand(*desc.batch_shape, *rhs.shape[-2:]))
        return torch.addcmul(self._linear_op._matmul(rhs), self._diag_tensor._diag.unsqueeze(-1), rhs)

    def _bilinear_derivative(self, left_vecs: Tensor, right_vecs: Tensor):
        """Sum rule (reference sum_linear_operator.py:59-62).  For a dense root plus a full diagonal both derivatives
        -- U (V^T C) + V (U^T C) and sum_d U o V -- come out of ONE pass over the factors (csrc/lo_bilinear.hip)."""
        root_op, diag_op = self._linear_op, self._diag_tensor
        r = root_op._dense_root() if isinstance(root_op, RootLinearOperator) else None
        fused = (r is not None and type(diag_op) is DiagLinearOperator and r.requires_grad
                 and diag_op._diag.requires_grad and left_vecs.is_cuda and left_vecs.dtype == torch.float32)
        if not fused:
            return super()._bilinear_derivative(left_vecs, right_vecs)
        d_root, d_diag = K.bilinear_root(r, left_vecs, right_vecs, with_rowdot=True)
        d_root = d_root if tuple(d_root.shape) == tuple(r.shape) else d_root.sum_to_size(*r.shape)
        dshape = diag_op._diag.shape
        d_diag = d_diag if tuple(d_diag.shape) == tuple(dshape) else d_diag.sum_to_size(*dshape)
        grads = {id(root_op): (d_root,), id(diag_op): (d_diag,)}
        return tuple(g for op in self.linear_ops for g in grads[id(op)])

    def add_diagonal(self, diag: Tensor):
        return self.__class__(self._linear_op, self._diag_tensor.add_diagonal(diag))

    def __add__(self, other):
        if isinstance(other, DiagLinearOperator):
            return self.__class__(self._linear_op, self._diag_tensor + other)
        return self.__class__(self._linear_op + other, self._diag_tensor)

    # ------------------------------------------------------------------ preconditioner (reference :95-184)
    def _precond_memo_key(self):
        tensors = self.representation()
        return tensors, _memo_key(tensors, (settings.max_preconditioner_size.value(),
                                            settings.preconditioner_tolerance.value(), type(self._linear_op),
                                            type(self._diag_tensor)))

    def _solve_preconditioner(self):
        """`_preconditioner()[0]` (reference _linear_operator.py:805), deferred when the solve can run as ONE resident
        launch (LazyWoodburyPreconditionClosure): low-rank root of 8 / 16 / 32 columns plus a diagonal, fp32 on the
        device, nothing memoised for these tensors yet, no batch-global stopping rule over ranks."""
        if (self.preconditioner_override is not None or self._q_cache is not None
                or settings.max_preconditioner_size.value() == 0
                or self.size(-1) < settings.min_preconditioning_size.value()):
            return super()._solve_preconditioner()
        from .. import distributed

        if distributed.active_stop_reduce() is not None or self.device.type != "cuda" or self.dtype != torch.float32:
            return super()._solve_preconditioner()
        tensors, key = self._precond_memo_key()
        if key is not None:
            if any(entry[0] == key for entry in _precond_memo):
                return super()._solve_preconditioner()
            for entry in _rootform_memo:
                if entry[0] == key:
                    return WoodburyPreconditionClosure(entry[2], self.batch_shape)
        desc = self._kernel_descriptor()
        rank = min(settings.max_preconditioner_size.value(), self.size(-1))
        if (desc is None or desc.dtype != torch.float32
                or not K.solve_fused_supported(desc, 1, rank, settings.max_cg_iterations.value())):
            return super()._solve_preconditioner()
        return LazyWoodburyPreconditionClosure(self, desc, rank, settings.preconditioner_tolerance.value(), key, tensors)

    def _preconditioner(self):
        if self.preconditioner_override is not None:
            return self.preconditioner_override(self)
        if settings.max_preconditioner_size.value() == 0 or self.size(-1) < settings.min_preconditioning_size.value():
            return None, None, None
        if self._q_cache is None:
            max_iter = settings.max_preconditioner_size.value()
            tensors, key = self._precond_memo_key()
            for entry in (_precond_memo if key is not None else ()):
                if entry[0] == key:
                    (self._piv_chol_self, self._piv_chol_perm, self._woodbury, self._q_cache,
                     self._precond_logdet_cache, self._constant_diag, self._noise) = entry[2]
                    self._precond_lt = PsdSumLinearOperator(RootLinearOperator(self._piv_chol_self), self._diag_tensor)
                    break
        if self._q_cache is None:
            self._piv_chol_self = self._pivoted_cholesky_factor(max_iter)  # :125
            # :126-131 `torch.any(torch.isnan(L))` as one reduction pass: amax propagates NaN, so the maximum is NaN
            # exactly when some entry is (no boolean tensor of L's size in between).  The constant-diagonal test of
            # _init_cache (:146-150) is evaluated with it: ONE read-back for the two flags instead of two drains of the
            # stream in a row
            L = self._piv_chol_self
            has_nan, constant = False, None
            if L.numel():
                nan_t = torch.isnan(L.amax())
                n = L.shape[-2]
                noise = self._diag_tensor._diagonal().expand(*L.shape[:-2], n)
                if L.is_cuda and not (noise.stride(-1) == 0 or n == 1):
                    both = torch.stack((nan_t, (noise == noise[..., :1]).all())).tolist()
                    has_nan, constant = bool(both[0]), bool(both[1])
                else:
                    has_nan = bool(nan_t.item())
            if has_nan:
                warnings.warn(
                    "NaNs encountered in preconditioner computation. Attempting to continue without preconditioning.",
                    NumericalWarning,
                )
                return None, None, None
            self._init_cache(constant)
            if PRECONDITIONER_MEMO_SIZE > 0 and key is not None:
                _precond_memo.insert(0, (key, tensors, (self._piv_chol_self, self._piv_chol_perm, self._woodbury,
                                                        self._q_cache, self._precond_logdet_cache, self._constant_diag,
                                                        self._noise)))
                del _precond_memo[PRECONDITIONER_MEMO_SIZE:]
        if self._woodbury is None:  # float64: z = r / d - Q (Q^T r) or (r - Q Q^T r) / sigma with library GEMMs (:135-140)
            closure = DensePreconditionClosure(self._q_cache, self._noise, self._constant_diag)
        else:
            closure = WoodburyPreconditionClosure(self._woodbury, self.batch_shape)
        closure.piv_chol, closure.piv_perm = self._piv_chol_self, getattr(self, "_piv_chol_perm", None)
        return closure, self._precond_lt, self._precond_logdet_cache

    def _pivoted_cholesky_factor(self, max_iter):
        """self._linear_op.pivoted_cholesky(rank=max_iter) (:125); when the operator lowers to a kernel descriptor
        the factor stays in the [B, m, N] row layout the HIP kernels write (a strided [.., N, m] view): the
        preconditioner build reads it in place and the transposed copy of _pivoted_cholesky.py:105 is skipped."""
        desc = self._linear_op._kernel_descriptor()
        if (desc is None or desc.diag_mode != 0 or desc.kind == K._hip.LO_OP_MASKED or self.device.type != "cuda"
                or self.dtype != torch.float32 or desc.dtype != torch.float32):
            # (a masked operator: the generic row access, as PivotedCholesky.forward; float64: the row-callback route)
            L, perm = self._linear_op.pivoted_cholesky(rank=max_iter, return_pivots=True)
            from .. import distributed

            m_global = distributed.global_max_int(L.shape[-1])  # (shared rank over all shards, as on the lowered path)
            if m_global > L.shape[-1]:
                L, perm = self._linear_op.pivoted_cholesky(rank=m_global, error_tol=0.0, return_pivots=True)
            self._piv_chol_perm = perm  # (the backward pass of the preconditioner terms needs the pivots here too)
            # detached: the rest of the cache is built by kernels outside autograd and the factor's derivative is
            # chained by hand (functions/_inv_quad_logdet._add_preconditioner_terms), exactly as on the lowered path
            return L.detach()
        tol = settings.preconditioner_tolerance.value()
        rank = min(max_iter, self.size(-1))
        L, perm = K.pivoted_cholesky(desc, rank, float(tol), contiguous=False)
        # batch-sharded runs under distributed.global_stopping_rule: the reference takes pivots while ANY member's
        # error exceeds the tolerance (_pivoted_cholesky.py:57), i.e. the largest rank any shard takes on its own; a
        # shard that stopped earlier continues to that rank (tolerance 0 never stops before the rank bound)
        from .. import distributed

        m_global = distributed.global_max_int(L.shape[-1])
        if m_global > L.shape[-1]:
            L, perm = K.pivoted_cholesky(desc, m_global, 0.0, contiguous=False)
        self._piv_chol_perm = perm  # needed by the backward pass of the preconditioner terms
        return L

    def _init_cache(self, constant_diag=None):
        """`constant_diag`: the value of the constant-diagonal test when the caller has already evaluated it."""
        L = self._piv_chol_self
        batch_shape = L.shape[:-2]
        n = L.shape[-2]
        noise = self._diag_tensor._diagonal().expand(*batch_shape, n)
        # constant-diagonal test on VALUES, as the reference does (:146-150), not on the operator type
        first = noise[..., :1]
        if noise.stride(-1) == 0 or n == 1:
            # a ConstantDiagLinearOperator (homoskedastic noise): the diagonal is an expanded [*batch, 1] tensor, constant
            # by construction -- no comparison kernel and no read-back
            self._constant_diag = True
        elif constant_diag is not None:
            self._constant_diag = bool(constant_diag)
        else:
            self._constant_diag = bool(torch.equal(noise, first.expand_as(noise)))
        self._noise = first if self._constant_diag else noise
        if L.is_cuda and (L.dtype == torch.float64 or (L.dtype == torch.float32 and L.shape[-1] > 128)):
            # float32 preconditioners of rank > 128 (settings.max_preconditioner_size is unbounded in the reference; the
            # kernels of lo_precond.hip stop at 128) take the same route: the reference's own thin QR, the apply as two
            # library GEMMs called back by lo_cg_solve_f32 per iteration.
            # float64 operators (round 4): the factor comes from the float64 instantiation of the pivoted-Cholesky
            # kernels; the thin QR of _init_cache* is the LAPACK call the reference itself makes (:161-184), on the
            # device, and the apply is two library GEMMs -- not a performance path (no Woodbury descriptor: linear_cg in
            # float64 takes the closure)
            # Built OUTSIDE autograd from the detached noise, like the float32 cache the kernels build: the derivatives of
            # logdet P and of the probes' term are chained by hand (functions/_inv_quad_logdet._add_preconditioner_terms).
            # A graph-carrying logdet in the memo below would be shared by later calls on the same tensors -- missing when
            # a solve filled the memo under no_grad, freed after the first backward otherwise.
            self._woodbury = None
            k = L.shape[-1]
            with torch.no_grad():
                L, noise, first = L.detach(), noise.detach(), first.detach()
                self._noise = first if self._constant_diag else noise
                eye = torch.eye(k, dtype=L.dtype, device=L.device).expand(*batch_shape, k, k)
                if self._constant_diag:
                    sig = first.unsqueeze(-1)  # [*batch, 1, 1]
                    Q, Rm = torch.linalg.qr(torch.cat((L, sig.sqrt() * eye), dim=-2))
                    self._q_cache = Q[..., :n, :]
                    logdet = Rm.diagonal(dim1=-1, dim2=-2).abs().log().sum(-1).mul(2) + (n - k) * sig[..., 0, 0].log()
                else:
                    sq = noise.unsqueeze(-1).sqrt()
                    Q, Rm = torch.linalg.qr(torch.cat((L / sq, eye), dim=-2))
                    self._q_cache = Q[..., :n, :] / sq
                    logdet = Rm.diagonal(dim1=-1, dim2=-2).abs().log().sum(-1).mul(2) + noise.log().sum(-1)
            self._precond_logdet_cache = logdet.view(*batch_shape) if len(batch_shape) else logdet.squeeze()
            self._precond_lt = PsdSumLinearOperator(RootLinearOperator(L), self._diag_tensor)  # :159
            return
        if not (L.is_cuda and L.dtype == torch.float32):
            raise K._hip.HipExtensionError("the preconditioner cache is built by liblo_amd: fp32 / fp64 HIP tensors only")
        d_arg = first[..., 0].contiguous() if self._constant_diag else noise.contiguous()
        # for a low-rank root the kernels also get the root form of the preconditioner (F = M (I + M^T E M)^-1 M^T with
        # L = C M): the operator-resident CG then needs one all-reduce per iteration and no second tall matrix
        root = self._linear_op._dense_root() if isinstance(self._linear_op, RootLinearOperator) else None
        perm = getattr(self, "_piv_chol_perm", None)
        if root is not None and perm is not None and root.is_cuda and root.dtype == torch.float32 and root.shape[-1] <= 32:
            root = root.detach().expand(*batch_shape, *root.shape[-2:])
            # (root form + fp64 Gram matrices only: everything a first solve / inv_quad_logdet launches -- the resident
            #  kernels and the R-space passes -- works from them; the generic Q of the reference's cache, 0.2 ms at the cfg3
            #  shape, is built when something asks for it: WoodburyPreconditioner.ensure_q -- the streaming engine, the
            #  stand-alone preconditioner apply, MINRES, the diagonal's logdet gradient)
            self._woodbury = K.precond_build(L, d_arg.to(torch.float32), self._constant_diag, root=root, perm=perm,
                                             need_q=False)
        else:
            # a Kronecker operator (two dense groups) with a constant diagonal also gets the Kronecker root form: the
            # single-column CG of large N then forms the rows of the preconditioner's tall matrix on the fly
            kron = None
            if self._constant_diag and perm is not None:
                base = self._linear_op._kernel_descriptor()
                if (base is not None and base.kind == K._hip.LO_OP_KRON_DIAG and base.diag_mode == K._hip.LO_DIAG_NONE
                        and base.dtype == torch.float32 and tuple(base.batch_shape) == tuple(batch_shape)):
                    kron = K._with_diag(base, d_arg.to(torch.float32), True)
            self._woodbury = K.precond_build(L, d_arg.to(torch.float32), self._constant_diag, perm=perm, kron=kron)
        # (`_q_cache is not None` = "the cache is built", as in the reference :63-70; the tensor itself is only read on the
        #  dense float64 / wide-rank route above, a root-form preconditioner carries its Q lazily)
        self._q_cache = (_LAZY_Q if self._woodbury.Q is None else
                         self._woodbury.Q[..., : self._woodbury.k].reshape(*batch_shape, n, self._woodbury.k))
        logdet = self._woodbury.logdet
        self._precond_logdet_cache = logdet.view(*batch_shape) if len(batch_shape) else logdet.squeeze()  # :172,:184
        self._precond_lt = PsdSumLinearOperator(RootLinearOperator(L), self._diag_tensor)  # :159

    def evaluate_kernel(self):
        rebuilt = self.representation_tree()(*self.representation())
        return rebuilt._linear_op + rebuilt._diag_tensor


__all__ = ["AddedDiagLinearOperator", "WoodburyPreconditionClosure", "LazyWoodburyPreconditionClosure"]
