"""Float64 structured operators on the device (ABI 22, csrc/lo_matvec_f64.hip): lo_matvec_f64 against float64 numpy
under a derived componentwise bound, the refusals of the fp32 consumers, the library-side preconditioner apply, the
three float64 solvers with a descriptor against the reference golden g34 (tests/golden/make_golden_f64.py), and the
operator API, which must not wrap a single Python closure for the product or the preconditioner.

Bound of the products (derived, not tuned): |y - y_np| <= 2 gamma_K (|A| |v|), gamma_K = K u / (1 - K u), u = 2^-53, K the
longest chain of additions and multiplications feeding one output (N + R + 2 low-rank, N + 1 dense, n1 + n2 + 2
Kronecker, the sum of the terms' K for a sum); the factor 2 because the numpy product carries the same bound."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import cases
from conftest import load_golden, rel_err
from make_golden_f64 import CASES, CG, LANCZOS_STEPS, MINRES_SHIFTS, MINRES_TOL, build, f64_inputs
from oracle import lo_oracle as orc

pytestmark = pytest.mark.gpu

from linear_operator_amd import _hip, kernels as K  # noqa: E402

U = 2.0 ** -53
MODES = ("none", "full", "const")
COLS = (1, 3, 17)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.detach().cpu().numpy()


def gamma(k):
    return k * U / (1 - k * U)


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def diag_of(mode, B, N, seed):
    """(numpy diagonal broadcastable to [B, N] or None, builder arguments (d tensor, const_diag))."""
    if mode == "none":
        return None, (None, False)
    if mode == "full":
        d = rng(seed).random((B, N)) + 0.5
        return d, (dev(d), False)
    d = rng(seed).random((B, 1)) + 0.5
    return d, (dev(d[:, 0]), True)


def check_product(desc_of, ref, absref, kchain, B, N, seed):
    """desc_of(d, const, members) -> descriptor of the members `members` (a slice); ref(d, v) / absref(|d|, |v|) the numpy
    product and its |A| |v|.  Every diagonal mode and column count: the bound, two calls bit for bit, and member 0
    computed alone bit for bit equal to member 0 inside the batch."""
    for mode in MODES:
        d, (dt, const) = diag_of(mode, B, N, seed)
        desc = desc_of(dt, const, slice(None))
        one = desc_of(None if dt is None else dt[:1].contiguous(), const, slice(0, 1))
        assert desc.dtype == torch.float64
        for c in COLS:
            v = rng(seed + c).standard_normal((B, N, c))
            y = K.matvec(desc, dev(v))
            assert y.dtype == torch.float64 and tuple(y.shape) == (B, N, c)
            dz = np.zeros((B, 1)) if d is None else d
            want, mag = ref(dz, v), absref(np.abs(dz), np.abs(v))
            err = np.abs(host(y) - want)
            assert np.all(err <= 2 * gamma(kchain) * mag), (mode, c, float((err / np.maximum(mag, 1e-300)).max()))
            assert torch.equal(y, K.matvec(desc, dev(v))), "two calls differ"
            assert torch.equal(K.matvec(one, dev(v[:1])), y[:1]), ("member alone differs from member in batch", mode, c)


def part(t, members):
    return t[members].contiguous()


@pytest.mark.parametrize("B,N,R", [(1, 1, 1), (3, 257, 6), (2, 300, 33), (1, 2049, 16)])
def test_lowrank_product_against_numpy(B, N, R):
    Cn = rng(10 + N).standard_normal((B, N, R)) / np.sqrt(R)
    Ct = dev(Cn)
    check_product(lambda d, const, m: K.lowrank_diag_descriptor(part(Ct, m), d, const, dtype=torch.float64),
                  lambda d, v: Cn @ (Cn.swapaxes(-1, -2) @ v) + d[..., None] * v,
                  lambda d, v: np.abs(Cn) @ (np.abs(Cn).swapaxes(-1, -2) @ v) + d[..., None] * v,
                  N + R + 2, B, N, 100 + N)
    # the same values 8 bytes off a 16-byte boundary: the order of the sums, and so every bit, is that of the aligned copy
    buf = torch.empty(Ct.numel() + 1, dtype=torch.float64, device="cuda")
    shifted = buf[1:].view(B, N, R).copy_(Ct)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 8 and Ct.data_ptr() % 16 == 0
    v = dev(rng(5).standard_normal((B, N, 3)))
    assert torch.equal(K.matvec(K.lowrank_diag_descriptor(shifted, None, dtype=torch.float64), v),
                       K.matvec(K.lowrank_diag_descriptor(Ct, None, dtype=torch.float64), v))


@pytest.mark.parametrize("N", [1, 63, 260])
def test_dense_product_against_numpy(N):
    B = 2
    Kn = rng(20 + N).standard_normal((B, N, N)) / np.sqrt(N)
    Kt = dev(Kn)
    check_product(lambda d, const, m: K.dense_diag_descriptor(part(Kt, m), d, const, dtype=torch.float64),
                  lambda d, v: Kn @ v + d[..., None] * v, lambda d, v: np.abs(Kn) @ v + d[..., None] * v,
                  N + 1, B, N, 200 + N)


@pytest.mark.parametrize("n1,n2", [(1, 7), (5, 7), (16, 24), (17, 33)])
def test_kronecker_product_against_numpy(n1, n2):
    B, N = 2, n1 * n2
    A1, A2 = rng(30 + n1).standard_normal((B, n1, n1)), rng(31 + n2).standard_normal((B, n2, n2))
    t1, t2 = dev(A1), dev(A2)
    check_product(lambda d, const, m: K.kron_diag_descriptor(part(t1, m), part(t2, m), d, const, dtype=torch.float64),
                  lambda d, v: orc.matvec_kron(A1, A2, v) + d[..., None] * v,
                  lambda d, v: orc.matvec_kron(np.abs(A1), np.abs(A2), v) + d[..., None] * v,
                  n1 + n2 + 2, B, N, 300 + N)


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1)])
def test_sum_product_against_numpy_in_both_term_orders(order):
    B, n1, n2, R = 2, 15, 20, 5
    N = n1 * n2
    Cn = rng(41).standard_normal((B, N, R)) / np.sqrt(R)
    Kn = rng(42).standard_normal((B, N, N)) / np.sqrt(N)
    A1, A2 = rng(43).standard_normal((B, n1, n1)), rng(44).standard_normal((B, n2, n2))
    f64 = dict(dtype=torch.float64)
    Ct, Kt, t1, t2 = dev(Cn), dev(Kn), dev(A1), dev(A2)

    def terms(m):
        return [K.lowrank_diag_descriptor(part(Ct, m), None, **f64), K.dense_diag_descriptor(part(Kt, m), None, **f64),
                K.kron_diag_descriptor(part(t1, m), part(t2, m), None, **f64)]

    prods = [lambda v: Cn @ (Cn.swapaxes(-1, -2) @ v), lambda v: Kn @ v, lambda v: orc.matvec_kron(A1, A2, v)]
    mags = [lambda v: np.abs(Cn) @ (np.abs(Cn).swapaxes(-1, -2) @ v), lambda v: np.abs(Kn) @ v,
            lambda v: orc.matvec_kron(np.abs(A1), np.abs(A2), v)]

    def ref(fs):
        def f(d, v):
            acc = fs[order[0]](v)
            for i in order[1:]:
                acc = acc + fs[i](v)
            return acc + d[..., None] * v
        return f

    check_product(lambda d, const, m: K.sum_descriptor([terms(m)[i] for i in order], d, const, **f64), ref(prods),
                  ref(mags), (N + R + 2) + (N + 1) + (n1 + n2 + 2), B, N, 400)


def test_refusals_launch_nothing():
    lib = _hip.load()
    v = torch.zeros(1, 4, 1, dtype=torch.float64, device="cuda")
    y = torch.empty_like(v)
    ws = _hip.workspace(4096, v.device)
    _hip.prof_enable(True)
    try:
        _hip.prof_report()
        for kind in (_hip.LO_OP_TOEPLITZ_DIAG, _hip.LO_OP_SKI_DIAG, _hip.LO_OP_HADAMARD_DIAG, _hip.LO_OP_MASKED,
                     _hip.LO_OP_CALLBACK):
            s = _hip.OpDesc()
            s.kind, s.diag_mode, s.B, s.N, s.R, s.n2, s.A0 = kind, 0, 1, 4, 4, 1, v.data_ptr()
            rc = lib.lo_matvec_f64(C.byref(s), _hip.ptr(v), _hip.ptr(y), 1, _hip.ptr(ws), ws.numel(), _hip.stream_ptr(v.device))
            assert rc == _hip.LO_ERR_UNSUPPORTED, kind
        Cd = torch.randn(2, 512, 16, dtype=torch.float64, device="cuda")
        desc = K.lowrank_diag_descriptor(Cd, torch.rand(2, 512, dtype=torch.float64, device="cuda") + 0.5,
                                         dtype=torch.float64)
        rhs32 = torch.randn(2, 512, 1, device="cuda")
        assert not K.solve_fused_supported(desc, 1, 15)
        assert K.masked_descriptor(desc, torch.arange(8, device="cuda")) is None
        assert K.block_matvec(desc, _hip.LO_BLOCK_DIAG, 2, rhs32.reshape(1, 1024, 1)) is None
        prm = K._cg_params(1, 0, 100, 20, 1.0, 1e-10, 1e-10, 0)
        for call in (lambda: K.pivoted_cholesky(desc, 15), lambda: K.solve_fused(desc, rhs32, 15),
                     lambda: K._CgSession(lib, desc, None, prm, rhs32.device), lambda: K.cg_solve(desc, rhs32),
                     lambda: K.lanczos_tridiag(desc, rhs32, 8), lambda: K.matvec(desc, rhs32),
                     lambda: K.minres_solve(desc, rhs32, torch.zeros(1, device="cuda"))):
            with pytest.raises(_hip.HipExtensionError):
                call()
        torch.cuda.synchronize()
        assert _hip.prof_report() == {}, "a refusal launched a kernel"
    finally:
        _hip.prof_enable(False)


@pytest.mark.parametrize("constant", [False, True])
def test_preconditioner_apply_against_the_dense_closure(constant):
    from linear_operator_amd.operators.added_diag_linear_operator import DensePreconditionClosure

    B, N, k = 2, 300, 15
    Qn = np.linalg.qr(rng(50).standard_normal((B, N, k)))[0]
    noise = rng(51).random((B, 1 if constant else N)) + 0.5
    Q, nz = dev(Qn), dev(noise)
    closure = DensePreconditionClosure(Q, nz, constant)
    for c in (1, 5):
        r = rng(52 + c).standard_normal((B, N, c))
        z = K.precond_apply_f64(Q, nz, constant, dev(r))
        qq = np.abs(Qn) @ (np.abs(Qn).swapaxes(-1, -2) @ np.abs(r))
        mag = (np.abs(r) + qq) / noise[..., None] if constant else np.abs(r) / noise[..., None] + qq
        err = np.abs(host(z) - host(closure(dev(r))))
        assert np.all(err <= 2 * gamma(N + k + 2) * mag), (constant, c, float((err / mag).max()))
        assert torch.equal(z, K.precond_apply_f64(Q, nz, constant, dev(r)))


def descriptor(case, t):
    f64 = dict(dtype=torch.float64)
    if case == "lowrank":
        return K.lowrank_diag_descriptor(t["C"], t["d"], **f64)
    if case == "kron":
        return K.kron_diag_descriptor(t["K1"], t["K2"], t["sigma2"][:, 0], True, **f64)
    return K.sum_descriptor([K.lowrank_diag_descriptor(t["C"], None, **f64), K.dense_diag_descriptor(t["K"], None, **f64)],
                            t["d"], **f64)


def operator(case, t):
    import linear_operator_amd.operators as ops

    base, diag = build(ops, case, t)
    return ops.AddedDiagLinearOperator(base, diag)


@pytest.mark.parametrize("case", CASES)
def test_cg_with_a_descriptor_and_the_native_preconditioner_against_g34(case):
    from linear_operator_amd.operators.added_diag_linear_operator import DensePreconditionClosure

    g = load_golden("g34_fp64_structured")
    t = {k: dev(v) for k, v in f64_inputs(case).items()}
    Q, noise, constant = dev(g[f"Q_{case}"]), dev(g[f"noise_{case}"]), bool(g[f"constant_{case}"])
    kw = dict(n_tridiag=CG["n_tridiag"], max_iter=CG["max_iter"], max_tridiag_iter=CG["max_tridiag_iter"],
              tolerance=CG["tolerance"])
    res = K.cg_solve_f64(None, None, t["rhs"], desc=descriptor(case, t), precond=(Q, noise, constant), **kw)
    assert res.iterations == int(g[f"matvecs_{case}"]) - 1 and res.matvecs == int(g[f"matvecs_{case}"])
    assert rel_err(host(res.x), g[f"x_{case}"]) < 1e-9
    assert res.t_mat.shape == g[f"t_{case}"].shape and rel_err(host(res.t_mat), g[f"t_{case}"]) < 1e-7
    A = operator(case, t)
    py = K.cg_solve_f64(None, None, t["rhs"], matvec_closure=lambda v: A._matmul(v),
                        precond_closure=DensePreconditionClosure(Q, noise, constant), **kw)
    assert py.iterations == res.iterations and rel_err(host(res.x), host(py.x)) < 1e-9


def test_minres_and_lanczos_with_a_descriptor_against_g34():
    g = load_golden("g34_fp64_structured")
    t = {k: dev(v) for k, v in f64_inputs("kron").items()}
    A = operator("kron", t)
    res = K.minres_solve_f64(None, t["rhs"], dev(MINRES_SHIFTS), desc=descriptor("kron", t), tolerance=MINRES_TOL,
                             max_iter=301)
    assert tuple(res.x.shape) == g["x_minres"].shape and rel_err(host(res.x), g["x_minres"]) < 1e-9
    py = K.minres_solve_f64(None, t["rhs"], dev(MINRES_SHIFTS), matvec_closure=lambda v: A._matmul(v),
                            tolerance=MINRES_TOL, max_iter=301)
    assert py.iterations == res.iterations and rel_err(host(res.x), host(py.x)) < 1e-9
    t = {k: dev(v) for k, v in f64_inputs("lowrank").items()}
    A = operator("lowrank", t)
    q, tl = K.lanczos_tridiag_f64(None, None, t["init"], LANCZOS_STEPS, desc=descriptor("lowrank", t))
    assert tuple(tl.shape) == g["lanczos_t"].shape
    assert np.allclose(host(tl), g["lanczos_t"], rtol=1e-9, atol=1e-12) and np.allclose(host(q[0]), g["lanczos_q0"], atol=1e-9)
    qp, tp = K.lanczos_tridiag_f64(None, None, t["init"], LANCZOS_STEPS, matvec_closure=lambda v: A._matmul(v))
    assert tp.shape == tl.shape and rel_err(host(tl), host(tp)) < 1e-9


@pytest.fixture
def wraps(monkeypatch):
    """Counts the Python closures handed to the library as callbacks (kernels._wrap_closure, a pass-through)."""
    count = [0]
    real = K._wrap_closure

    def counting(*a, **kw):
        count[0] += 1
        return real(*a, **kw)

    monkeypatch.setattr(K, "_wrap_closure", counting)
    return count


def api_calls(monkeypatch, lowered):
    """A.solve, inv_quad_logdet with injected probes and sqrt_inv_matmul of the float64 AddedDiag(LowRankRoot, Diag) of g34
    (N 600), and the solve of a Kronecker + full diagonal operator (KroneckerProductAddedDiagLinearOperator without a
    closed form: on CG), through the operator API.  lowered=False: `_lower_f64` and `_native_precond_f64` answer None in
    the three solver front ends, i.e. the product and the preconditioner go back to the called-back closures of the
    parent commit.  Returns the results and the iteration counts of every float64 CG / MINRES call made on the way."""
    import importlib

    import linear_operator_amd as lo
    import linear_operator_amd.operators as ops

    iterations = []
    with monkeypatch.context() as mp:
        if not lowered:
            for name in ("linear_cg", "minres", "lanczos"):
                mod = importlib.import_module("linear_operator_amd.utils." + name)
                mp.setattr(mod, "_lower_f64", lambda *a, **kw: None)
                if hasattr(mod, "_native_precond_f64"):
                    mp.setattr(mod, "_native_precond_f64", lambda *a, **kw: None)
        for name in ("cg_solve_f64", "minres_solve_f64"):
            def recording(*a, _real=getattr(K, name), **kw):
                res = _real(*a, **kw)
                iterations.append(res.iterations)
                return res
            mp.setattr(K, name, recording)

        class Probed(ops.AddedDiagLinearOperator):
            _probes = None

            def _probe_vectors_and_norms(self):
                return self._probes

        t = {k: dev(v) for k, v in f64_inputs("lowrank").items()}
        tk = {k: dev(v) for k, v in f64_inputs("kron").items()}
        dk = dev(rng(60).random((2, 300)) + 0.5)
        Zn, nrm = cases.probes(3403, 2, 600, 4, dtype=np.float64)
        out = {}
        with lo.settings.max_cholesky_size(0), lo.settings.min_preconditioning_size(100), \
                lo.settings.cg_tolerance(CG["tolerance"]), lo.settings.max_cg_iterations(CG["max_iter"]), \
                warnings.catch_warnings():
            warnings.simplefilter("ignore")
            A = operator("lowrank", t)
            out["solve"] = A.solve(t["rhs"])
            Ap = Probed(*build(ops, "lowrank", t))
            Ap._probes = (dev(Zn), dev(nrm))
            out["inv_quad"], out["logdet"] = Ap.inv_quad_logdet(t["rhs"], logdet=True)
            out["sqrt_inv_matmul"] = A.sqrt_inv_matmul(t["rhs"])
            Ak = ops.KroneckerProductLinearOperator(ops.DenseLinearOperator(tk["K1"]), ops.DenseLinearOperator(tk["K2"])
                                                    ).add_diagonal(dk)
            assert isinstance(Ak, ops.KroneckerProductAddedDiagLinearOperator)
            out["kron_solve"] = Ak.solve(tk["rhs"])
    return out, iterations, (A, Ak, t, tk, dk)


def test_float64_operators_solve_without_a_python_closure(wraps, monkeypatch):
    """The operator API end to end.  No Python closure is wrapped for the product or the preconditioner (fails on the
    parent commit: two wraps per solve), and every result equals the same call on the closure route -- the parent's --
    with equal iteration counts and within the float64 bar of 1e-9: a product or a preconditioner that were subtly wrong
    would change the iterates.  The low-rank solve also meets the reference's golden g34 as far as two CG runs stopped
    at different iterations can agree (the golden run carries tridiagonals, which move its stop)."""
    from linear_operator_amd.operators.added_diag_linear_operator import clear_preconditioner_memo

    clear_preconditioner_memo()
    g = load_golden("g34_fp64_structured")
    native, it_native, (A, Ak, t, tk, dk) = api_calls(monkeypatch, lowered=True)
    assert wraps[0] == 0, f"{wraps[0]} Python closures were wrapped on the lowered route"
    assert len(it_native) >= 4 and all(v.dtype == torch.float64 for v in native.values())
    clear_preconditioner_memo()  # (the closure route builds its own preconditioner, as the parent commit would)
    closure, it_closure, _ = api_calls(monkeypatch, lowered=False)
    assert wraps[0] >= 2 * 3, "the comparison route did not go through Python closures"
    assert it_native == it_closure, (it_native, it_closure)
    for key in native:
        err = rel_err(host(native[key]), host(closure[key]))
        print(key, err)
        assert native[key].shape == closure[key].shape and err < 1e-9, (key, err)
    # sanity against the dense matrix and the reference (CG stopped at cg_tolerance: no tighter than that)
    assert rel_err(host(native["solve"]), g["x_lowrank"]) < 10 * CG["tolerance"]
    dense = host(A.to_dense())
    rhs = host(t["rhs"])
    assert np.allclose(host(native["inv_quad"]), (rhs * np.linalg.solve(dense, rhs)).sum((-2, -1)), rtol=1e-6)
    w, V = np.linalg.eigh(dense)
    want = (V * w[..., None, :] ** -0.5) @ (V.swapaxes(-1, -2) @ rhs)
    assert rel_err(host(native["sqrt_inv_matmul"]), want) < 1e-3
    assert rel_err(host(native["kron_solve"]), np.linalg.solve(host(Ak.to_dense()), host(tk["rhs"]))) < 1e-3
    # torch.matmul of the operators, whichever way the routing table sends it
    Cn, dn, K1n, K2n, dkn = (host(a) for a in (t["C"], t["d"], tk["K1"], tk["K2"], dk))
    for op, kchain, prod in ((A, 600 + 8 + 2, lambda C_, d_, v: C_ @ (C_.swapaxes(-1, -2) @ v) + d_[..., None] * v),
                             (Ak, 12 + 25 + 2, None)):
        for c in (1, 3):
            v = rng(70 + c).standard_normal((2, op.shape[-1], c))
            y = torch.matmul(op, dev(v))
            assert y.dtype == torch.float64
            if prod is not None:
                want, mag = prod(Cn, dn, v), prod(np.abs(Cn), dn, np.abs(v))
            else:
                want = orc.matvec_kron(K1n, K2n, v) + dkn[..., None] * v
                mag = orc.matvec_kron(np.abs(K1n), np.abs(K2n), np.abs(v)) + dkn[..., None] * np.abs(v)
            assert np.all(np.abs(host(y) - want) <= 2 * gamma(kchain) * mag), (type(op).__name__, c)
    clear_preconditioner_memo()


def test_user_closures_are_still_called_once_per_product():
    from linear_operator_amd.utils import linear_cg

    M = cases.spd_test_matrix(3431, 60)
    b = cases.randn(3432, 2, 60, 3)
    _, _, info = orc.linear_cg(lambda v: M @ v, b, max_iter=60, tolerance=1e-8)
    Md, calls = dev(M), [0]

    def closure(v):
        calls[0] += 1
        return Md @ v

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x = linear_cg(closure, dev(b), max_iter=60, tolerance=1e-8)
    assert calls[0] == info.matvecs and x.dtype == torch.float64


# ---- the operand path the three float64 solvers share (kernels._f64_operands, csrc/lo_f64_solver.h) --------------------
# B = 2 so that a member index exists, N = 5, two columns, two shifts, five steps.  References: the oracle's restatement
# of each solver on the same numpy operands, computed once, under the float64 bar of this file (1e-9).
SOLVERS = ("cg", "minres", "lanczos")
OB, ON, OC, OSTEPS = 2, 5, 2, 5


class Operand:
    """A + diag(d), SPD and well conditioned, with right-hand sides; `dense_desc(with_diag)`: the float64 descriptor."""

    def __init__(self):
        M = rng(81).standard_normal((OB, ON, ON))
        self.A = M @ M.swapaxes(-1, -2) / ON + np.eye(ON)
        self.d = rng(82).random((OB, ON)) + 0.5
        self.rhs = rng(83).standard_normal((OB, ON, OC))
        self.shifts = np.array([0.25, 1.5])
        self.At, self.dt, self.rhst, self.sht = dev(self.A), dev(self.d), dev(self.rhs), dev(self.shifts)
        self.want = {}

    def dense_desc(self, with_diag):
        return K.dense_diag_descriptor(self.At, self.dt if with_diag else None, dtype=torch.float64)

    def full(self, with_diag):
        return self.At + torch.diag_embed(self.dt) if with_diag else self.At

    def reference(self, solver):
        if solver not in self.want:
            Ad = self.A + np.einsum("bi,ij->bij", self.d, np.eye(ON))
            if solver == "cg":
                x, _, info = orc.linear_cg(lambda v: Ad @ v, self.rhs, max_iter=OSTEPS, max_tridiag_iter=OSTEPS,
                                            tolerance=1e-12)
                self.want[solver] = ((x,), info.matvecs)
            elif solver == "minres":
                x, info = orc.minres(lambda v: self.A @ v, self.rhs, shifts=self.shifts, max_iter=OSTEPS)
                self.want[solver] = ((x,), info.iterations)
            else:
                self.want[solver] = (orc.lanczos_tridiag(lambda v: Ad @ v, OSTEPS, self.rhs), None)
        return self.want[solver]


@pytest.fixture(scope="module")
def opd():
    return Operand()


def run_solver(o, solver, **operand):
    """(output tensors, the count of products (CG) or iterations (MINRES) or None) of one solver call.  `operand`: A= (and diag=), desc= or matvec_closure=
    (and precond_closure=); CG and Lanczos solve with A + diag(d), MINRES (no diagonal argument) with A."""
    A, diag = operand.pop("A", None), operand.pop("diag", None)
    if solver == "cg":
        res = K.cg_solve_f64(A, diag, o.rhst, max_iter=OSTEPS, max_tridiag_iter=OSTEPS, tolerance=1e-12, **operand)
        return (res.x,), res.matvecs
    if solver == "minres":
        res = K.minres_solve_f64(A, o.rhst, o.sht, max_iter=OSTEPS, **operand)
        return (res.x,), res.iterations
    return K.lanczos_tridiag_f64(A, diag, o.rhst, OSTEPS, **operand), None


def dense_operand(o, solver):
    return dict(A=o.At) if solver == "minres" else dict(A=o.At, diag=o.dt)


def assert_right(o, solver, got):
    outs, count = got
    want, want_count = o.reference(solver)
    assert count == want_count
    for a, b in zip(outs, want):
        err = rel_err(host(a), b)
        print(solver, "against the oracle", err)
        assert a.dtype == torch.float64 and tuple(a.shape) == b.shape and err < 1e-9, (solver, err)


class ClosureFailure(Exception):
    pass


@pytest.mark.parametrize("solver,which", [(s, "matvec_closure") for s in SOLVERS] +
                         [(s, "precond_closure") for s in ("cg", "minres")])
def test_an_exception_inside_a_closure_surfaces_as_itself(opd, solver, which):
    raised = ClosureFailure(f"{which} of {solver}, member 1")

    def failing(v):
        raise raised

    full = opd.full(solver != "minres")
    operand = dict(matvec_closure=failing) if which == "matvec_closure" else dict(
        matvec_closure=lambda v: full @ v, precond_closure=failing)
    with pytest.raises(ClosureFailure) as caught:
        run_solver(opd, solver, **operand)
    assert caught.value is raised and str(caught.value) == f"{which} of {solver}, member 1"
    # the device and the library are as they were: the ordinary routes give the right answer
    assert_right(opd, solver, run_solver(opd, solver, **dense_operand(opd, solver)))
    closure = dict(matvec_closure=lambda v: full @ v)
    if solver != "lanczos":
        closure["precond_closure"] = lambda v: v.clone()
    assert_right(opd, solver, run_solver(opd, solver, **closure))


@pytest.mark.parametrize("solver", SOLVERS)
def test_dense_tensor_and_dense_descriptor_give_the_same_bits(opd, solver):
    """Both routes end in k64_dense_mv with the same launch (f64_dense_mv_ex), so an operand wired to the wrong slot of
    the shared helper -- the diagonal dropped, the descriptor's context in the preconditioner's place -- shows as a
    different bit.  Bit-equal on the parent commit too (profiles/r16/README.md)."""
    dense = run_solver(opd, solver, **dense_operand(opd, solver))
    desc = run_solver(opd, solver, desc=opd.dense_desc(solver != "minres"))
    assert_right(opd, solver, dense)
    assert dense[1] == desc[1]
    for a, b in zip(dense[0], desc[0]):
        assert torch.equal(a, b), (solver, float((a - b).abs().max()))


@pytest.mark.parametrize("solver", SOLVERS)
def test_the_wrappers_refuse_a_missing_or_mismatched_operator_in_the_same_words(opd, solver):
    with pytest.raises(ValueError, match="^need a dense fp64 operator or a matvec closure$"):
        run_solver(opd, solver)
    other = K.dense_diag_descriptor(dev(np.ones((3, 4, 4))), None, dtype=torch.float64)
    with pytest.raises(RuntimeError, match=r"^the right-hand side \(batch 2, N 5\) does not match operator batch 3, N 4$"):
        run_solver(opd, solver, desc=other)
