"""The workspaces of the entry points beside the matvec plan, on the device (the sibling of test_gpu_matvec_plan.py):
every entry point that is sized by its own layout function runs on exactly the bytes its sizer reports, gives the same
bits on twice as many, and refuses one byte less before it writes anything.  The Woodbury apply (PrecondPlan) is checked
at k = 5, where it takes a padded copy of Q, and at k = 8, where it does not, on its own and inside CG and MINRES.

kernels.py allocates every workspace through _hip.workspace(bytes the sizer reported): the tests replace that one
function to scale the allocation, pre-filled so that a write shows."""
import ctypes

import numpy as np
import pytest
import torch

import workspace_cases as wc
from conftest import max_rel_err_cols
from linear_operator_amd import _hip as H
from linear_operator_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LO_ERR_BADARG, LO_ERR_WORKSPACE = -1, -3
B, N = 2, 37  # (the row splits have a tail)
COLS = (1, 3)
FILL = 0x5A


class Workspaces:
    """Stands in for _hip.workspace: `scale` times the bytes asked for plus `delta`, pre-filled; keeps what it gave."""

    def __init__(self, scale=1, delta=0):
        self.scale, self.delta, self.given = scale, delta, []

    def __call__(self, nbytes, device):
        ws = torch.full((int(nbytes) * self.scale + self.delta,), FILL, dtype=torch.uint8, device=device)
        self.given.append((int(nbytes), ws))
        return ws

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((ws == FILL).all()) for _, ws in self.given)


def with_workspaces(monkeypatch, fn, scale=1, delta=0):
    w = Workspaces(scale, delta)
    monkeypatch.setattr(H, "workspace", w)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        monkeypatch.undo()
    return out, w


def tensors(out):
    if torch.is_tensor(out):
        return [out]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in tensors(o)]
    return []


def exact_doubled_short(monkeypatch, fn, sizer_bytes=None, launches_nothing=True):
    """fn on exactly the reported bytes; the same bits on twice as many; one byte short: refused, and (every entry point
    but the solvers, which stage their operands while they lay the workspace out) with the workspace untouched."""
    out, w = with_workspaces(monkeypatch, fn)
    assert w.given, "the call took no workspace"
    if sizer_bytes is not None:
        assert [n for n, _ in w.given] == [sizer_bytes] * len(w.given)
    out2, _ = with_workspaces(monkeypatch, fn, scale=2)
    a, b = tensors(out), tensors(out2)
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)), "the workspace size changed the result"
    short = Workspaces(delta=-1)
    monkeypatch.setattr(H, "workspace", short)
    try:
        with pytest.raises(H.HipExtensionError, match="workspace too small"):
            fn()
    finally:
        monkeypatch.undo()
    assert not launches_nothing or short.untouched(), "a short workspace: nothing may be launched"
    return out


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(seed, *shape):
    return torch.randn(*shape, generator=gen(seed)).to(DEV)


_pre = {}


def woodbury(k, width=None):
    """A rank-k Woodbury preconditioner of the shared shape with a full diagonal; `width`: floats per row of Q (the build
    writes padded_rank(k); k gives the unpadded rows the apply has to copy; anything else is a refused descriptor)."""
    if k not in _pre:
        L = randn(40 + k, B, N, k) / k ** 0.5
        d = torch.rand(B, N, generator=gen(50 + k)).to(DEV) + 0.5
        _pre[k] = K.precond_build(L, d, constant_diag=False)
    pre = _pre[k]
    if width is None or width == pre.Q.shape[-1]:
        return pre
    Q = pre.Q[..., :width].contiguous() if width < pre.Q.shape[-1] else torch.nn.functional.pad(
        pre.Q, (0, width - pre.Q.shape[-1]))
    return K.WoodburyPreconditioner(Q, pre.dinv, k, False)


def apply_raw(pre, r, z, ws, nbytes):
    s = pre.c_struct()
    rc = H.load().lo_precond_apply_f32(ctypes.byref(s), H.ptr(r), H.ptr(z), B, N, r.shape[-1], H.ptr(ws), nbytes,
                                       H.stream_ptr(r.device))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("c", COLS)
@pytest.mark.parametrize("k,width", [(5, 5), (8, 8)])
def test_precond_apply_exact_doubled_short_and_value(k, width, c):
    lib = H.load()
    pre = woodbury(k, width)
    r = randn(60 + c, B, N, c)
    need = lib.lo_precond_apply_workspace_bytes(B, N, k, c)
    copy = 4 * B * N * wc.padded_rank(k)
    assert (need >= copy) == (k == 5), "the padded copy is counted exactly where it is taken"
    ws = torch.full((2 * need,), FILL, dtype=torch.uint8, device=DEV)
    z = torch.full_like(r, 7.0)
    assert apply_raw(pre, r, z, ws, need - 1) == LO_ERR_WORKSPACE
    assert bool((z == 7.0).all()) and bool((ws == FILL).all()), "a short workspace: nothing may be launched"
    assert apply_raw(pre, r, z, ws, need) == 0
    z2 = torch.full_like(r, 7.0)
    assert apply_raw(pre, r, z2, ws, 2 * need) == 0
    assert torch.equal(z, z2)
    Q, r64 = pre.Q[..., :k].double().cpu().numpy(), r.double().cpu().numpy()
    ref = r64 * pre.dinv.double().cpu().numpy()[..., None] - Q @ (np.swapaxes(Q, -1, -2) @ r64)
    assert max_rel_err_cols(z.cpu().numpy(), ref) < 1e-5  # (test_gpu_parity: precond_apply against fp64)


_op = {}


def lowrank_operator():
    """Rank-5 root + diagonal at the shared shape, with the rank-5 Woodbury preconditioner on unpadded rows of Q."""
    if not _op:
        Cr = randn(70, B, N, 5) / 5 ** 0.5
        d = torch.rand(B, N, generator=gen(71)).to(DEV) + 0.5
        _op["desc"] = K.lowrank_diag_descriptor(Cr, d)
        _op["dense"] = (Cr.double() @ Cr.double().mT + torch.diag_embed(d.double())).cpu().numpy()
    return _op["desc"], _op["dense"]


@pytest.mark.parametrize("c", COLS)
def test_cg_with_a_woodbury_preconditioner_exact_doubled_short(monkeypatch, c):
    desc, dense = lowrank_operator()
    pre, rhs = woodbury(5, 5), randn(80 + c, B, N, c)

    def solve():
        res = K.cg_solve(desc, rhs, precond=pre, tolerance=1e-5, max_iter=30)
        return res.x, torch.tensor(res.iterations)

    x, _ = exact_doubled_short(monkeypatch, solve, launches_nothing=False)
    assert max_rel_err_cols(x.cpu().numpy(), np.linalg.solve(dense, rhs.double().cpu().numpy())) < 1e-4


@pytest.mark.parametrize("c", COLS)
def test_minres_with_a_woodbury_preconditioner_exact_doubled_short(monkeypatch, c):
    desc, dense = lowrank_operator()
    pre, rhs = woodbury(5, 5), randn(90 + c, B, N, c)
    shifts = torch.tensor([0.0, 0.5], device=DEV)

    def solve():
        res = K.minres_solve(desc, rhs, shifts, precond=pre, max_iter=30)
        return res.x

    x = exact_doubled_short(monkeypatch, solve, launches_nothing=False)
    # (shift 0 is the plain solve whatever the preconditioner; test_gpu_api: MINRES solves at 5e-4)
    assert max_rel_err_cols(x[0].cpu().numpy(), np.linalg.solve(dense, rhs.double().cpu().numpy())) < 5e-4


def test_a_row_stride_that_is_neither_k_nor_the_padded_rank_is_refused():
    desc, _ = lowrank_operator()
    bad, r = woodbury(5, 6), randn(99, B, N, 1)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    assert apply_raw(bad, r, torch.empty_like(r), ws, ws.numel()) == LO_ERR_BADARG
    with pytest.raises(H.HipExtensionError, match="bad argument"):
        K.cg_solve(desc, r, precond=bad, tolerance=1e-5, max_iter=30)
    with pytest.raises(H.HipExtensionError, match="bad argument"):
        K.minres_solve(desc, r, torch.tensor([0.5], device=DEV), precond=bad, max_iter=5)


# ---- the other entry points, each at its smallest shape of tests/workspace_cases.py -----------------------------------
def _first(fn):
    return wc.CASES[fn][0][0]


def _sizer(fn):
    return int(getattr(H.load(), fn)(*_first(fn)))


def _spd(seed, b, n):
    a = randn(seed, b, n, n)
    return a @ a.mT / n + 0.5 * torch.eye(n, device=DEV)


def _build():
    b, n, k = _first("lo_precond_build_workspace_bytes")
    L, d = randn(1, b, n, k), torch.rand(b, n, generator=gen(2)).to(DEV) + 0.5
    return lambda: (lambda p: (p.Q, p.dinv, p.logdet))(K.precond_build(L, d, False))


def _root_form(rs):
    fn = "lo_precond_root_form_rs_workspace_bytes" if rs else "lo_precond_root_form_workspace_bytes"
    b, n, R = _first(fn)  # (R % 4 == 0 takes the R-space entry point, any other rank the plain one)
    Cr = randn(3, b, n, R) / R ** 0.5
    d = torch.rand(b, n, generator=gen(4)).to(DEV) + 0.5
    L, perm = K.pivoted_cholesky(K.lowrank_diag_descriptor(Cr, None), min(R, 4))

    def run():
        p = K.precond_build(L, d, False, root=Cr, perm=perm, need_q=False)
        assert (p.RS is not None) == rs
        return (p.F, p.EF, p.E, p.dinv, p.logdet) + ((p.RS,) if rs else ())

    return run


def _kron_root():
    (b,) = _first("lo_precond_kron_root_workspace_bytes")
    K1, K2 = _spd(5, b, 3), _spd(6, b, 5)
    sig = torch.rand(b, generator=gen(7)).to(DEV) + 0.5
    desc = K.kron_diag_descriptor(K1, K2, sig, const_diag=True)
    L, perm = K.pivoted_cholesky(desc.without_diag(), 4)
    L3 = L.reshape(b, 15, -1)
    return lambda: K._kron_root(H.load(), desc, perm, L3, L3.shape[-1], DEV)[0]


def _bilinear_root():
    b, n, R, D = _first("lo_bilinear_root_workspace_bytes")
    Cr, U, V = randn(8, b, n, R), randn(9, b, n, D), randn(10, b, n, D)
    return lambda: K.bilinear_root(Cr, U, V, with_rowdot=True)


def _bilinear_kron():
    b, n1, n2, D = _first("lo_bilinear_kron_workspace_bytes")
    K1, K2, U, V = _spd(11, b, n1), _spd(12, b, n2), randn(13, b, n1 * n2, D), randn(14, b, n1 * n2, D)
    return lambda: K.bilinear_kron(K1, K2, U, V)


def _probes():
    b, n, P = _first("lo_probe_vectors_workspace_bytes")
    L, d = randn(15, b, n, 5), torch.rand(b, n, generator=gen(16)).to(DEV) + 0.5
    e1, e2 = randn(17, b, 5, P), randn(18, b, n, P)
    return lambda: K.probe_vectors(L, d, e1, e2, None, (b,))


def _hadamard():
    b, n, p, q, S = _first("lo_hadamard_bilinear_workspace_bytes")
    F, G, U, V = randn(19, b, n, p), randn(20, b, n, q), randn(21, b, n, S), randn(22, b, n, S)
    return lambda: K.bilinear_hadamard(F, G, U, V)


def _cholesky():
    b, n = _first("lo_cholesky_workspace_bytes")
    A = _spd(23, b, n)
    return lambda: K.cholesky(A, want_logdet=True)


def _eigh():
    P, b = _first("lo_tridiag_eigh_slq_workspace_bytes")
    T = 6
    off = torch.rand(P, b, T - 1, generator=gen(24)) * 0.3
    t = torch.diag_embed(torch.rand(P, b, T, generator=gen(25)) + 1.0) + torch.diag_embed(off, 1) + torch.diag_embed(off, -1)
    t = t.to(DEV)
    return lambda: K.tridiag_eigh_slq(t, 37, want_evecs=True)


def _bilinear_diag_constant():  # (no sizer: kernels.py gives a float per row and 256 bytes)
    U, V = randn(26, B, N, 3), randn(27, B, N, 3)
    return lambda: K.bilinear_diag(U, V, (B,), constant=True)


ENTRY_POINTS = {
    "lo_precond_build_workspace_bytes": _build,
    "lo_precond_root_form_workspace_bytes": lambda: _root_form(False),
    "lo_precond_root_form_rs_workspace_bytes": lambda: _root_form(True),
    "lo_precond_kron_root_workspace_bytes": _kron_root,
    "lo_bilinear_root_workspace_bytes": _bilinear_root,
    "lo_bilinear_kron_workspace_bytes": _bilinear_kron,
    "lo_probe_vectors_workspace_bytes": _probes,
    "lo_hadamard_bilinear_workspace_bytes": _hadamard,
    "lo_cholesky_workspace_bytes": _cholesky,
    "lo_tridiag_eigh_slq_workspace_bytes": _eigh,
}


def test_every_sizer_of_the_table_has_its_entry_point_here():
    assert set(ENTRY_POINTS) | {"lo_precond_apply_workspace_bytes"} == set(wc.CASES)


@pytest.mark.parametrize("fn", sorted(ENTRY_POINTS))
def test_entry_point_exact_doubled_short(monkeypatch, fn):
    run = ENTRY_POINTS[fn]()  # (operands built on default workspaces; only `run` is measured)
    exact_doubled_short(monkeypatch, run, sizer_bytes=_sizer(fn))


def test_bilinear_diag_constant_takes_its_row_buffer_from_the_workspace(monkeypatch):
    run = _bilinear_diag_constant()
    out, w = with_workspaces(monkeypatch, run)
    out2, _ = with_workspaces(monkeypatch, run, scale=2)
    assert torch.equal(out, out2)
    U, V = randn(26, B, N, 3), randn(27, B, N, 3)
    assert torch.allclose(out.double(), (U.double() * V.double()).sum((-1, -2)).reshape(B, 1), rtol=1e-5, atol=1e-4)
    short = Workspaces(delta=-(256 + 1))  # (one byte less than a float per row)
    monkeypatch.setattr(H, "workspace", short)
    try:
        with pytest.raises(H.HipExtensionError, match="workspace too small"):
            run()
    finally:
        monkeypatch.undo()
    assert short.untouched()
