"""The descriptor table of the matvec plan layer (csrc/lo_matvec.hip): one small operator per kind and per route of a
kind, shared by tests/test_matvec_plan_cpu.py (sizes only: the tensors stay on the CPU and are never read) and
tests/test_gpu_matvec_plan.py (products and solves).  Every operator is positive definite, so the same table serves the
solvers.  Not a test module."""
import ctypes as C
import math

import torch

from linear_operator_amd import _hip
from linear_operator_amd.kernels import OperatorDescriptor

COLS = (1, 3)
# the solver calls of the table: a short CG, MINRES with two shifts, four Lanczos steps
CG_MAX_ITER, MINRES_SHIFTS, MINRES_MAX_ITER, LANCZOS_ITERS = 5, 2, 3, 4
SOLVER_CASES = ("lowrank_r5", "masked_dense", "ski")

CASES = (
    "lowrank_r5", "lowrank_r8", "dense_splitk", "dense_plain", "kron_3x5", "kron_128", "toeplitz_33", "ski", "ski_plan",
    "ski_grid_2d", "ski_grid_3d", "hadamard", "masked_dense", "masked_kron", "masked_sum", "sum3",
)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def _psd(g, B, n):
    a = _randn(g, B, n, n)
    return a @ a.mT / n + 0.5 * torch.eye(n)


def _toeplitz_column(B, m, scale):
    k = torch.arange(m, dtype=torch.float32)
    ell = scale * (1.0 + 0.25 * torch.arange(B, dtype=torch.float32))[:, None]
    return torch.exp(-((k / ell) ** 2)).contiguous()


def _toeplitz_dense(col):
    m = col.shape[-1]
    i = torch.arange(m)
    return col[:, (i[:, None] - i[None, :]).abs()]


def _interp(g, B, N, J, M):
    idx = torch.randint(0, M, (B, N, J), generator=g, dtype=torch.int64)
    vals = torch.rand(B, N, J, generator=g, dtype=torch.float32) + 0.1
    return idx, vals / vals.sum(-1, keepdim=True)


def _interp_dense(idx, vals, M):
    B, N, J = idx.shape
    W = torch.zeros(B, N, M, dtype=torch.float64)
    return W.scatter_add_(-1, idx, vals.double())


class Case:
    """desc: the OperatorDescriptor; dense: the operator as a float64 matrix [B, N, N] (None where `apply` is given);
    apply(v64): the float64 product for an operator too large to write out; need(c): bytes of the buffers the kind
    provably takes for a c-column product (the lower bound of the reported workspace size)."""

    def __init__(self, desc, dense=None, apply=None, need=None, keep=()):
        self.desc, self.dense, self._apply, self.need, self.keep = desc, dense, apply, need, keep

    def product(self, v):
        v64 = v.double()
        return self._apply(v64) if self._apply is not None else self.dense.to(v.device) @ v64


def _desc(kind, B, N, dev, d=None, const=False, **kw):
    t = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()}
    desc = OperatorDescriptor(kind, B, N, **t)
    if d is not None:
        desc.d, desc.diag_mode = d.to(dev).contiguous(), (_hip.LO_DIAG_CONST if const else _hip.LO_DIAG_FULL)
    return desc


def _diag_dense(d, N, const):
    return torch.diag_embed(d.double().expand(-1, N) if const else d.double())


def _f4(n):
    return 4 * n


def build(name, dev="cpu"):
    g = _gen(1000 + CASES.index(name))
    if name in ("lowrank_r5", "lowrank_r8"):
        B, N, R = 2, 300, (5 if name == "lowrank_r5" else 8)
        const = name == "lowrank_r8"
        Cr = _randn(g, B, N, R) / math.sqrt(R)
        d = torch.rand(B, 1 if const else N, generator=g) + 0.5
        dense = Cr.double() @ Cr.double().mT + _diag_dense(d, N, const)
        # t = C^T v partials (at least one row block) and, R % 4 != 0, the padded copy of C
        return Case(_desc(_hip.LO_OP_LOWRANK_DIAG, B, N, dev, d, const, A0=Cr, R=R), dense,
                    need=lambda c: _f4(B * 8 * c) + (_f4(B * N * 8) if R == 5 else 0))
    if name in ("dense_splitk", "dense_plain"):
        B, N = (1, 1024) if name == "dense_splitk" else (2, 100)
        K = _psd(g, B, N)
        d = torch.rand(B, N, generator=g) + 0.5
        # the split-K route (c >= 2, N >= 1024, a small batch) holds at least two slices of partial products
        return Case(_desc(_hip.LO_OP_DENSE_DIAG, B, N, dev, d, A0=K), K.double() + _diag_dense(d, N, False),
                    need=lambda c: _f4(2 * B * N * c) if (name == "dense_splitk" and c >= 2) else 0)
    if name in ("kron_3x5", "kron_128"):
        B, n1, n2 = (2, 3, 5) if name == "kron_3x5" else (1, 128, 128)
        N = n1 * n2
        K1, K2 = _psd(g, B, n1), _psd(g, B, n2)
        d = torch.rand(B, N, generator=g) + 0.5
        desc = _desc(_hip.LO_OP_KRON_DIAG, B, N, dev, d, A0=K1, A1=K2, R=n1, n2=n2)

        def apply(v):  # (K1 (x) K2) v through the factors: the 16384 x 16384 matrix is not written out
            k1, k2, dd = K1.double().to(v.device), K2.double().to(v.device), d.double().to(v.device)
            x = v.reshape(B, n1, n2, -1)
            return torch.einsum("bij,bkl,bjlc->bikc", k1, k2, x).reshape(v.shape) + dd[..., None] * v

        cols = name == "kron_128"  # more than one column on the matrix cores: two column-major copies
        return Case(desc, apply=apply, need=lambda c: _f4(B * N * c) * (2 if cols and c > 1 else 1))
    if name == "toeplitz_33":
        B, M = 2, 33
        col = _toeplitz_column(B, M, 3.0)
        d = torch.rand(B, M, generator=g) + 0.5
        return Case(_desc(_hip.LO_OP_TOEPLITZ_DIAG, B, M, dev, d, A0=col, R=M),
                    _toeplitz_dense(col).double() + _diag_dense(d, M, False), need=lambda c: _f4(B * M * c))
    if name in ("ski", "ski_plan", "ski_grid_2d", "ski_grid_3d"):
        grid = {"ski_grid_2d": (5, 7), "ski_grid_3d": (3, 4, 5)}.get(name, ())
        B, N, J = 2, 50, (4 if not grid else 2 ** len(grid))
        M = math.prod(grid) if grid else 20
        li, lv = _interp(g, B, N, J, M)
        d = torch.rand(B, N, generator=g) + 0.5
        if grid:
            cols = [_toeplitz_column(B, m, 2.0 + k) for k, m in enumerate(grid)]
            col = torch.cat(cols, -1).contiguous()
            T = _toeplitz_dense(cols[0]).double()
            for t in cols[1:]:
                Tk = _toeplitz_dense(t).double()
                T = torch.einsum("bij,bkl->bikjl", T, Tk).reshape(B, T.shape[1] * Tk.shape[1], -1)
            kind = _hip.LO_OP_SKI_GRID_DIAG
        else:
            col = _toeplitz_column(B, M, 4.0)
            T = _toeplitz_dense(col).double()
            kind = _hip.LO_OP_SKI_DIAG
        W = _interp_dense(li, lv, M)
        desc = _desc(kind, B, N, dev, d, A0=col, R=M, n2=J, grid=grid)
        li, lv = li.to(dev), lv.to(dev)
        desc.interp = (li, lv, li, lv)
        csr = 2 * _f4(B * (M + 1)) + 2 * _f4(B * N * J)  # the grid-major copy of W_r: two offset and two id arrays
        if name == "ski_plan":
            if torch.device(dev).type == "cuda":
                from linear_operator_amd import kernels as K

                desc.interp_plan = K.interp_plan_build(li, M)
            else:  # (sizes only: a non-null address)
                desc.interp_plan = torch.zeros(64, dtype=torch.uint8)
            csr = 0
        # u = W_r^T v and T u on the grid, the copy of W_r, and (1-D grid) at least one slice of Toeplitz partials
        return Case(desc, W @ T @ W.mT + _diag_dense(d, N, False),
                    need=lambda c: (2 if grid else 3) * _f4(B * M * c) + csr)
    if name == "hadamard":
        B, N, p, q = 2, 70, 3, 2
        F, G = _randn(g, B, N, p), _randn(g, B, N, q)
        d = torch.rand(B, N, generator=g) + 0.5
        dense = (F.double() @ F.double().mT) * (G.double() @ G.double().mT) + _diag_dense(d, N, False)
        # the reduced M_t = F^T diag(v_t) G of every column, and at least as much again for the partials
        return Case(_desc(_hip.LO_OP_HADAMARD_DIAG, B, N, dev, d, A0=F, A1=G, R=p, n2=q), dense,
                    need=lambda c: 2 * _f4(B * c * p * q))
    if name.startswith("masked_"):
        base_name = {"masked_dense": "dense_base", "masked_kron": "kron_base", "masked_sum": "sum_base"}[name]
        base = _build_base(base_name, g, dev)
        B, N0 = base.desc.B, base.desc.N
        keep = torch.rand(N0, generator=g) < 0.7
        keep[0] = True
        idx = torch.nonzero(keep).squeeze(-1)
        M = idx.numel()
        d = torch.rand(B, M, generator=g) + 0.5
        desc = _desc(_hip.LO_OP_MASKED, B, M, dev, d)
        desc.mask = (base.desc, idx.to(dev))
        dense = base.dense[:, idx][:, :, idx] + _diag_dense(d, M, False)
        # the inverse map, the expanded vector and (every route but the dense one at c <= 4 columns) the base's result
        two = name != "masked_dense"
        return Case(desc, dense, need=lambda c: 4 * N0 + _f4(B * N0 * c) * (2 if two else 1) + base.need(c))
    if name == "sum3":
        return _build_base("sum3", g, dev)
    raise KeyError(name)


def _build_base(name, g, dev):
    if name == "dense_base":
        B, N = 2, 90
        K = _psd(g, B, N)
        d = torch.rand(B, N, generator=g) + 0.5
        return Case(_desc(_hip.LO_OP_DENSE_DIAG, B, N, dev, d, A0=K), K.double() + _diag_dense(d, N, False),
                    need=lambda c: 0)
    if name == "kron_base":
        B, n1, n2 = 2, 6, 7
        K1, K2 = _psd(g, B, n1), _psd(g, B, n2)
        dense = torch.einsum("bij,bkl->bikjl", K1.double(), K2.double()).reshape(B, n1 * n2, n1 * n2)
        return Case(_desc(_hip.LO_OP_KRON_DIAG, B, n1 * n2, dev, A0=K1, A1=K2, R=n1, n2=n2), dense,
                    need=lambda c: _f4(B * n1 * n2 * c))
    B, N, R = 2, 80, 5
    Cr, K = _randn(g, B, N, R) / math.sqrt(R), _psd(g, B, N)
    terms = [_desc(_hip.LO_OP_LOWRANK_DIAG, B, N, dev, A0=Cr, R=R), _desc(_hip.LO_OP_DENSE_DIAG, B, N, dev, A0=K)]
    dense = Cr.double() @ Cr.double().mT + K.double()
    if name == "sum3":
        n1, n2 = 8, 10
        K1, K2 = _psd(g, B, n1), _psd(g, B, n2)
        terms.append(_desc(_hip.LO_OP_KRON_DIAG, B, N, dev, A0=K1, A1=K2, R=n1, n2=n2))
        dense = dense + torch.einsum("bij,bkl->bikjl", K1.double(), K2.double()).reshape(B, N, N)
    d = torch.rand(B, N, generator=g) + 0.5
    desc = _desc(_hip.LO_OP_SUM, B, N, dev, d, terms=tuple(terms))
    # the buffer a term beyond the first is computed into, the rank-5 root's padded copy and (at least one row block of)
    # its partials, the Kronecker term's intermediate
    return Case(desc, dense + _diag_dense(d, N, False),
                need=lambda c: _f4(B * N * c) + _f4(B * N * 8) + _f4(B * 8 * c) + (_f4(B * N * c) if name == "sum3" else 0))


def cg_params(c):
    prm = _hip.CgParams()
    prm.c, prm.n_tridiag, prm.max_iter, prm.max_tridiag_iter, prm.floor_max_iter = c, 0, CG_MAX_ITER, 20, 0
    prm.tolerance, prm.eps, prm.stop_updating_after = 1e-4, 1e-10, 1e-10
    return prm


def minres_params(c):
    prm = _hip.MinresParams()
    prm.c, prm.n_shifts, prm.max_iter, prm.has_value, prm.value = c, MINRES_SHIFTS, MINRES_MAX_ITER, 0, 1.0
    prm.shifts_per_member, prm.tolerance, prm.eps = 0, 1e-4, 1e-25
    return prm


def sizes(lib, desc, c):
    """The four reported workspace sizes of a c-column product / solve on `desc`."""
    s = desc.c_struct()
    cg, mr = cg_params(c), minres_params(c)
    return {
        "lo_matvec_workspace_bytes": int(lib.lo_matvec_workspace_bytes(C.byref(s), c)),
        "lo_cg_workspace_bytes": int(lib.lo_cg_workspace_bytes(C.byref(s), None, C.byref(cg))),
        "lo_minres_workspace_bytes": int(lib.lo_minres_workspace_bytes(C.byref(s), None, C.byref(mr))),
        "lo_lanczos_workspace_bytes": int(lib.lo_lanczos_workspace_bytes(C.byref(s), c, LANCZOS_ITERS)),
    }
