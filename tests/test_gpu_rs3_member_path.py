"""k_cg_rspace3 forms the last iteration's residual norm off the member's serial path (csrc/lo_rspace3.hip):
only workgroup 0 of a group evaluates it, and for a member that is not the group's final one the owning wave does so at
the top of the NEXT member, from what it left in LDS, in front of the barrier that hands the matrices over.  The group
exchange polls up to 9 granules of a thread in one round.

A group takes member `grp` first and then the members it draws: a member is deferred exactly when its group goes on to
another one, so a batch exercises the deferred path only when it has more members than the launch has groups (two
workgroups per CU on 256 CUs: 512 / GW groups).  Shapes:

  (3, 8192, 32)    every member is a group's final one
  (9, 8192, 32)    nine groups with one member each (on a smaller device: a deferred member, then a final one)
  (64, 4096, 16)   four workgroups per member
  (65, 1000, 8)    one workgroup per member, ragged
  (33, 16384, 32)  sixteen workgroups per member, two poll rounds of nine; one group takes a deferred member, then a final one
  (67, 8192, 32)   eight workgroups per member, one poll round of nine; three deferred members
  (130, 4096, 16)  four workgroups per member; two deferred members
  (515, 1000, 8)   one workgroup per member (no exchange), ragged; three deferred members

For each: x meets the fp64 Woodbury solution; 20 solves repeat bit for bit; a batch of copies of ONE system gives every
member the same x, the x of a three-copy batch (final path only); and the same batch of DIFFERENT systems solved on a
quarter of the device (LO_OC_RESERVE_CUS: a quarter of the groups, so other members -- and more of them -- are deferred)
returns the same x and the same mean residual, bit for bit.
"""
import numpy as np
import pytest
import torch

import cases
import test_gpu_early_ticket as et

from linear_operator_amd import kernels as K  # noqa: E402

gpu = pytest.mark.gpu

SHAPES = [(3, 8192, 32), (9, 8192, 32), (64, 4096, 16), (65, 1000, 8), (33, 16384, 32),
          (67, 8192, 32), (130, 4096, 16), (515, 1000, 8)]
N_REPEAT = 20

_form_on_second_use = et._form_on_second_use  # (autouse: the diagonal form on second use, switches restored)


class Copies(et.Case):
    """B copies of one system (its operator, diagonal and right-hand side), on the diagonal form."""

    def __init__(self, seed, B, N, R):
        self.shape = (B, N, R)
        C1, d1, r1 = cases.lowrank_diag(seed, 1, N, R, 1)
        self.C, self.d = np.repeat(C1, B, 0), np.repeat(d1, B, 0)
        self.desc = K.lowrank_diag_descriptor(et.dev(self.C), et.dev(self.d))
        L, perm = K.pivoted_cholesky(self.desc, 15)
        self.pre = K.precond_build(L, et.dev(self.d), constant_diag=False, root=self.desc.A0, perm=perm)
        self.rhs = et.dev(np.repeat(r1, B, 0))
        self.solve(self.rhs)
        self.solve(self.rhs)
        assert torch.is_tensor(self.pre.RSD)
        rsd = self.pre.RSD.reshape(B, -1)
        assert torch.equal(rsd, rsd[:1].expand_as(rsd)), "the copies' diagonal forms differ: the test cannot tell paths apart"
        self.res, _ = self.solve_owned(self.rhs)
        torch.cuda.synchronize()


_cases, _copies = {}, {}


def case(shape):
    if shape not in _cases:
        _cases[shape] = et.Case(9300 + SHAPES.index(shape), *shape)
    return _cases[shape]


def copies(B, N, R):
    """One system per (N, R), whatever the number of copies."""
    if (B, N, R) not in _copies:
        _copies[(B, N, R)] = Copies(9400 + N + R, B, N, R)
    return _copies[(B, N, R)]


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_x_meets_the_closed_form(shape):
    cs = case(shape)
    ex = et.woodbury(cs.C, cs.d, cs.rhs_host[0])
    err = float(((cs.refs[0].x.double() - ex).norm(dim=-2) / ex.norm(dim=-2)).max())
    print(f"{shape}: max relative error against fp64 Woodbury {err:.3e}")
    assert err < 1e-4, err  # (the bound of tests/test_gpu_eigform.py for this engine)


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_twenty_solves_repeat_bit_for_bit(shape):
    cs = case(shape)
    first = cs.refs[0]
    for i in range(N_REPEAT):
        res, cleared = cs.solve_owned(cs.rhs[0])
        assert cleared == 0, f"solve {i} cleared the buffer"
        assert torch.equal(res.x, first.x), f"solve {i} differs"
        assert res.mean_residual == first.mean_residual and res.iterations == first.iterations, f"solve {i}"


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_a_member_s_result_does_not_depend_on_its_path(shape):
    B, N, R = shape
    many, three = copies(B, N, R), copies(3, N, R)
    x = many.res.x
    assert torch.equal(x, x[:1].expand_as(x)), "copies of one system got different solutions"
    assert torch.equal(x[0], three.res.x[0]), "the solution differs from the three-copy batch (final path only)"
    assert many.res.iterations == three.res.iterations
    assert many.res.tolerance_reached == three.res.tolerance_reached and not many.res.nan_detected
    # (cg_solve exposes no per-member residual or state, only the fp32 mean of the norms -- and that mean cannot be compared
    #  between the two batches: the kernels that build a cache's diagonal form are chosen by the batch size, the forms
    #  differ in their last bits, and the norm, a difference of much larger fp64 terms, follows them.  The members'
    #  records are checked through the mean of ONE cache on two grids below.)
    res, _ = many.solve_owned(many.rhs)
    assert torch.equal(res.x, x) and res.mean_residual == many.res.mean_residual


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_the_records_do_not_depend_on_which_members_are_deferred(shape, monkeypatch):
    """One cache, one right-hand side, two grids: with 192 of 256 CUs' worth of slots reserved a launch has a quarter of
    the groups, so (64, 4096, 16) and (33, 16384, 32) defer half and three quarters of their members, the shapes beyond
    the issue's defer most, and a deferred norm meets the matrices of a DIFFERENT system in LDS if it is formed too late.
    The members' norms reach the caller as their fp32 mean, summed in the order of the members: equal bit for bit."""
    cs = case(shape)
    full = cs.refs[0]
    monkeypatch.setenv("LO_OC_RESERVE_CUS", "192")
    for i in range(3):
        res, _ = cs.solve_owned(cs.rhs[0])
        assert torch.equal(res.x, full.x), f"solve {i}: x depends on the grid"
        assert res.mean_residual == full.mean_residual, (i, res.mean_residual, full.mean_residual)
        assert res.iterations == full.iterations and res.tolerance_reached == full.tolerance_reached
    monkeypatch.delenv("LO_OC_RESERVE_CUS")
    res, _ = cs.solve_owned(cs.rhs[0])
    assert torch.equal(res.x, full.x) and res.mean_residual == full.mean_residual
