"""The `_bilinear_derivative` contraction kernels (csrc/lo_bilinear.hip: dense, diag, constant diag, root;
`kron_bilinear` of csrc/lo_kron.hip) and the SLQ eigensolver (csrc/lo_eig.hip) on the MI355X, driven directly at the
shapes where their host-side selection rules change branch, against the fp64 oracle under the componentwise bounds
gamma_K * mag of tests/bilinear_cases.py (derived there from the kernels' rounding chains and checked without a GPU in
tests/test_bilinear_cases_cpu.py).  Every product is also run twice (same bits) and with member 0 alone (same bits as
inside the batch); dense and diag write between NaN guard bands; the refusals launch nothing.  The largest
err / bound of every case is printed (pytest -s)."""
import numpy as np
import pytest
import torch

import bilinear_cases as E

from linear_operator_amd import _hip
from linear_operator_amd import kernels as K

pytestmark = pytest.mark.gpu
GUARD = 1024  # sentinel floats before and after a guarded buffer


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def ids(table):
    return ["x".join(str(x) for x in case) for case, _ in table]


def within(name, case, got, ref, mag, k):
    ratio = E.err_over_bound(host(got).reshape(ref.shape), ref, mag, k)
    print(f"{name} {case} K={k}: err / bound {ratio:.3f}")
    return ratio <= 1.0


# ---- products --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,route", E.DENSE_CASES, ids=ids(E.DENSE_CASES))
def test_dense(case, route):
    B, N, D = case
    U, V, ref, mag = E.dense_inputs(case)
    Ud, Vd = dev(U), dev(V)
    out = K.bilinear_dense(Ud, Vd)
    assert out.shape == (B, N, N) and out.dtype == torch.float32
    assert within(f"dense [{route}]", case, out, ref, mag, E.dense_K(*case))
    assert same_bits(out, K.bilinear_dense(Ud, Vd))
    assert same_bits(out[:1], K.bilinear_dense(Ud[:1], Vd[:1]))


@pytest.mark.parametrize("constant", [False, True], ids=["full", "constant"])
@pytest.mark.parametrize("case,route", E.DIAG_CASES, ids=ids(E.DIAG_CASES))
def test_diag(case, route, constant):
    B, N, D = case
    U, V, refs = E.diag_inputs(case)
    ref, mag = refs[constant]
    Ud, Vd = dev(U), dev(V)
    out = K.bilinear_diag(Ud, Vd, constant=constant)
    assert out.shape == ((B, 1) if constant else (B, N)) and out.dtype == torch.float32
    assert within(f"diag{' constant' if constant else ''} [{route}]", case, out, ref, mag, E.diag_K(*case, constant))
    assert same_bits(out, K.bilinear_diag(Ud, Vd, constant=constant))
    assert same_bits(out[:1], K.bilinear_diag(Ud[:1], Vd[:1], constant=constant))


@pytest.mark.parametrize("with_rowdot", [False, True], ids=["plain", "rowdot"])
@pytest.mark.parametrize("case,route", E.ROOT_CASES, ids=ids(E.ROOT_CASES))
def test_root(case, route, with_rowdot):
    B, N, R, D = case
    Cm, U, V, ref, mag, rd, rd_mag = E.root_inputs(case)
    k_out, k_dot = E.root_K(*case)
    Cd, Ud, Vd = dev(Cm), dev(U), dev(V)

    def run(b=slice(None)):
        res = K.bilinear_root(Cd[b], Ud[b], Vd[b], with_rowdot=with_rowdot)
        return res if with_rowdot else (res, None)

    out, dot = run()
    assert out.shape == (B, N, R) and out.dtype == torch.float32
    assert within(f"root [{route}]", case, out, ref, mag, k_out)
    if with_rowdot:
        assert dot.shape == (B, N) and dot.dtype == torch.float32
        assert within("root rowdot", case, dot, rd, rd_mag, k_dot)
    out2, dot2 = run()
    assert same_bits(out, out2) and (not with_rowdot or same_bits(dot, dot2))
    solo, solo_dot = run(slice(0, 1))
    alone, batch = E.root_facts(1, N, R, D), E.root_facts(B, N, R, D)
    if (alone["S"], alone["rows"], alone["launches"]) == (batch["S"], batch["rows"], batch["launches"]):
        assert same_bits(out[:1], solo) and (not with_rowdot or same_bits(dot[:1], solo_dot))
    else:
        # choose_split and `tiles` look at B: alone, the member is cut into other slices (another summation order) or
        # walked by other workgroups, and the library does not promise the batch's bits -- the bound holds either way
        assert within("root, member 0 alone", case, solo, ref[:1], mag[:1], E.root_K(1, N, R, D)[0])
        if with_rowdot:
            assert within("root rowdot, member 0 alone", case, solo_dot, rd[:1], rd_mag[:1], E.root_K(1, N, R, D)[1])


@pytest.mark.parametrize("case,route", E.KRON_CASES, ids=ids(E.KRON_CASES))
def test_kron(case, route):
    B, n1, n2, D = case
    K1, K2, U, V, ref, mag, swapped = E.kron_inputs(case)
    k1, k2 = E.kron_K(*case)
    args = [dev(t) for t in (K1, K2, U, V)]
    d1, d2 = K.bilinear_kron(*args)
    assert d1.shape == (B, n1, n1) and d2.shape == (B, n2, n2) and d1.dtype == d2.dtype == torch.float32
    print(f"kron [{route}]")
    assert within("kron dK1", case, d1, ref[0], mag[0], k1)
    assert within("kron dK2", case, d2, ref[1], mag[1], k2)
    # orientation: the factors are not symmetric, so the same result must MISS the bound around the oracle evaluated
    # with the other factor transposed (a 1 x 1 factor has no orientation)
    if n2 > 1:
        assert not within("kron dK1 against the oracle with K2^T", case, d1, swapped[0], mag[0], k1)
    if n1 > 1:
        assert not within("kron dK2 against the oracle with K1^T", case, d2, swapped[1], mag[1], k2)
    e1, e2 = K.bilinear_kron(*args)
    assert same_bits(d1, e1) and same_bits(d2, e2)
    s1, s2 = K.bilinear_kron(*[t[:1] for t in args])
    assert same_bits(d1[:1], s1) and same_bits(d2[:1], s2)


@pytest.mark.parametrize("case,route", E.SLQ_CASES, ids=ids(E.SLQ_CASES))
def test_slq(case, route):
    P, B, T, kind = case
    t = dev(E.slq_matrices(case))

    def run(tm, want_evecs=True):
        return K.tridiag_eigh_slq(tm, E.SLQ_N, want_evecs=want_evecs, want_logdet=True)

    evals, evecs, logdet = run(t)
    assert evals.shape == (P, B, T) and evecs.shape == (P, B, T, T) and logdet.shape == (B,)
    ratios = E.slq_check(case, host(evals), host(evecs), host(logdet))  # (asserts dtypes and the exact masked entries)
    print(f"slq [{route}]: err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(ratios.items())))
    assert set(ratios) == {"evals", "recon", "orth", "logdet"} and max(ratios.values()) <= 1.0, ratios
    # the instantiation without the eigenvector matrix
    ev0, none, ld0 = run(t, want_evecs=False)
    assert none is None
    assert max(E.slq_check(case, host(ev0), None, host(ld0)).values()) <= 1.0
    for a, b in zip((evals, evecs, logdet), run(t)):
        assert same_bits(a, b)
    # member 0 alone: its tridiagonals sit on other threads, P of them instead of P B
    s_evals, s_evecs, s_logdet = run(t[:, :1].contiguous())
    assert same_bits(evals[:, :1], s_evals) and same_bits(evecs[:, :1], s_evecs) and same_bits(logdet[:1], s_logdet)


# ---- guard bands: dense and diag outputs have no padding -------------------------------------------------------------
def guarded(n):
    """(buffer, its middle n floats): NaN everywhere, the output included."""
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, n):
    sentinel = bits(torch.full((GUARD,), float("nan"), dtype=torch.float32, device="cuda"))
    return torch.equal(bits(buf[:GUARD]), sentinel) and torch.equal(bits(buf[GUARD + n:]), sentinel)


@pytest.mark.parametrize("case,route", E.DENSE_CASES, ids=ids(E.DENSE_CASES))
def test_dense_writes_every_output_and_nothing_else(case, route):
    """A first pass that accumulated instead of overwriting would leave NaN in the output; an edge tile that ignored
    N would write into the band behind it."""
    B, N, D = case
    U, V, ref, mag = E.dense_inputs(case)
    n = B * N * N
    buf, out = guarded(n)
    K._launch("lo_bilinear_dense_f32", buf.device, dev(U), dev(V), B, N, D, out)
    torch.cuda.synchronize()
    assert guards_intact(buf, n), "the dense contraction wrote outside its output"
    assert bool(torch.isfinite(out).all())
    assert within("dense between guards", case, out, ref, mag, E.dense_K(*case))


@pytest.mark.parametrize("constant", [False, True], ids=["full", "constant"])
@pytest.mark.parametrize("case,route", E.DIAG_CASES, ids=ids(E.DIAG_CASES))
def test_diag_writes_every_output_and_nothing_else(case, route, constant):
    B, N, D = case
    U, V, refs = E.diag_inputs(case)
    ref, mag = refs[constant]
    n = B if constant else B * N
    buf, out = guarded(n)
    wbuf, ws = guarded(B * N)  # the row sums of the constant mode: B N floats of workspace, not one more
    K._launch("lo_bilinear_diag_f32", buf.device, dev(U), dev(V), B, N, D, 1 if constant else 0, out,
              ws if constant else None, 4 * B * N if constant else 0)
    torch.cuda.synchronize()
    assert guards_intact(buf, n), "the diag contraction wrote outside its output"
    assert guards_intact(wbuf, B * N), "the diag contraction wrote outside its workspace"
    assert bool(torch.isfinite(out).all())
    if constant:
        assert bool(torch.isfinite(ws).all())
    else:
        assert bool(torch.isnan(ws).all()), "the full mode has no workspace"
    assert within("diag between guards", case, out, ref, mag, E.diag_K(*case, constant))


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    def z(*shape):
        return torch.zeros(*shape, dtype=torch.float32, device="cuda")

    refused = (
        ("diag, D = 8193", lambda: K.bilinear_diag(z(1, 1, 8193), z(1, 1, 8193))),
        ("constant diag, D = 8193", lambda: K.bilinear_diag(z(1, 1, 8193), z(1, 1, 8193), constant=True)),
        ("dense, B = 65536", lambda: K.bilinear_dense(z(65536, 1, 1), z(65536, 1, 1))),
        ("kron, B D = 65552", lambda: K.bilinear_kron(z(3856, 1, 1), z(3856, 1, 1), z(3856, 1, 17), z(3856, 1, 17))),
        ("slq, T = 33", lambda: K.tridiag_eigh_slq(z(1, 1, 33, 33), E.SLQ_N, want_evecs=True)),
    )
    _hip.load()
    _hip.prof_enable(True)
    try:
        _hip.prof_report()
        for name, call in refused:
            with pytest.raises(_hip.HipExtensionError):
                call()
            torch.cuda.synchronize()
            assert _hip.prof_report() == {}, f"{name}: a refusal launched a kernel"
    finally:
        _hip.prof_enable(False)


# ---- what the bound sees that a max-norm comparison does not ---------------------------------------------------------
def test_dense_bound_sees_a_lost_pass():
    """The device result of (2, 65, 130) meets the bound; the same product contracted over the first 64 columns only --
    computed on the host from the reference, what losing the second and third pass would give -- misses it."""
    case = (2, 65, 130)
    U, V, ref, mag = E.dense_inputs(case)
    k = E.dense_K(*case)
    assert within("dense", case, K.bilinear_dense(dev(U), dev(V)), ref, mag, k)
    lost = E.orc.bilinear_derivative_dense(U[..., :64].astype(np.float64), V[..., :64].astype(np.float64))
    ratio = E.err_over_bound(lost, ref, mag, k)
    print(f"dense {case} with the first pass only: err / bound {ratio:.3e}")
    assert ratio > 1e3
