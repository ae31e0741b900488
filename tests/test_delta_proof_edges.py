"""The difference-array kernels at the edges of their exactness proof, on the CPU emulator (tests/delta_edges.py).

wt_delta.h trusts a window's integer sum when emax - emin <= R = 29 - ceil(lg N) and hands every other window to the general
kernel.  The cases put windows at span R (must stay on the exact route, nothing refused, bits equal to the sequential f64
sum, which there equals the exact sum) and at R + 1 (must be refused; bits equal to the sequential sum, which for a power of
two N >= 8 is NOT the exact sum -- so a kernel that accepted the window would be caught, and the test asserts that the two
differ).  512-bp windows (delta_T=64); ppt=4, T=64 puts a general plan under them that can patch single windows.

Routes, from the emulator's info: a refused window usually takes its neighbour with it (the window index is generous: a
window also reads the run next to it), so counts of refused windows are bounded, not fixed -- except where every window
must be refused."""
import numpy as np
import pytest

import delta_edges as DE
from emu import emu
from helpers import assert_runs_equal

W_EMU = 512
SPECS = DE.specs(device=False)


def _tol(op):
    return 1e-12 if op in DE.VAR_OPS else 0.0


def _check_route(case, info, what):
    r = case.route
    if r == "exact":
        assert info["delta"] == 1 and info["delta_bad"] == 0 and info["patched"] == 0, what
        assert info["W"] == case.W and info["n_windows"] == case.n_windows, what
    elif r == "patched":
        assert info["delta"] == 1 and info["delta_bad"] >= 1 and info["patched"] >= 1, what
    elif r == "fallback":
        assert info["delta"] == 0 and info["delta_bad"] >= 1 and info["patched"] == 0, what
    elif r == "refused":
        assert info["delta_bad"] >= 1, what
    elif r == "near":
        assert info["delta"] == 1 and info["patched"] == info["delta_bad"], what
    else:
        assert r == "off" and info["delta"] == 0 and info["delta_bad"] == 0, what
    if case.all_bad:
        assert info["delta_bad"] == case.n_windows, what
    if case.redo == "none":
        assert info["delta_redo"] == 0, what
    elif case.redo == "some":
        assert info["delta_redo"] >= 1, what


def _check_references(case, oracle):
    """the case is what it claims to be, and the plain references agree with the compiled one"""
    assert len(case.expected("sum")[0]) == case.n_runs, case.name
    if case.finite:
        exact = DE.sequential_is_exact(case)
        if case.sensitive:
            assert not all(exact), "%s: the sequential sum equals the exact sum everywhere -- the case is not sensitive" % case.name
        if case.sensitive_rn:
            assert not all(DE.sequential_is_rounded_exact(case)), "%s: the sequential sum is the exact sum rounded once -- a trusted integer sum would not show" % case.name
        if case.route == "exact":
            assert all(exact), "%s: a sequential sum rounds inside the bound" % case.name
    d = case.t.as_dict()
    for op in case.ops:
        for strict in ((0, 1) if op in ("sum", "mean") else (0,)):
            assert_runs_equal(case.expected(op, strict), oracle.reduce(d, op, flags=strict), _tol(op), "%s %s strict %d: plain reference vs oracle" % (case.name, op, strict))


@pytest.mark.parametrize("spec", SPECS, ids=[s[0] for s in SPECS])
def test_emu_delta_proof_edge(oracle, spec):
    _, fn, kw = spec
    case = fn(W=W_EMU, **kw)
    _check_references(case, oracle)
    for op in case.ops:
        for strict in ((0, 1) if op in ("sum", "mean") else (0,)):
            got, info = emu.reduce(case.t, op, flags=strict, delta_T=64, ppt=4, T=64)
            what = "%s %s strict %d %s" % (case.name, op, strict, info)
            _check_route(case, info, what)
            assert_runs_equal(got, case.expected(op, strict), _tol(op), what)


SPEC5 = DE.specs(device=False, only=("speculative",))


@pytest.mark.parametrize("delta_T", [64, 128])
@pytest.mark.parametrize("spec", SPEC5, ids=[s[0] for s in SPEC5])
def test_emu_delta_speculative_unit_any_wave_order(spec, delta_T):
    """Case 5: every window is narrow in itself, so neither the unit the workgroup guessed nor the order its wavefronts run in may
    show in the result (one and two wavefronts per workgroup)."""
    _, fn, kw = spec
    case = fn(W=8 * delta_T, **kw)
    for op in case.ops:
        exp = case.expected(op)
        assert len(exp[0]) == case.n_runs
        for order in ("forward", "reverse", "shuffle:3"):
            got, info = emu.reduce(case.t, op, delta_T=delta_T, ppt=4, T=64, wave_order=order)
            what = "%s %s T %d %s %s" % (case.name, op, delta_T, order, info)
            _check_route(case, info, what)
            assert_runs_equal(got, exp, 0.0, what)


def test_the_bound_is_what_the_cases_assume():
    """R = 29 - ceil(lg N) at both sides of every power of two the cases use, and N * 2^(R + 24) <= 2^53 < N * 2^(R + 25)"""
    for n, r in ((1, 29), (2, 28), (3, 27), (4, 27), (5, 26), (8, 26), (9, 25), (64, 23), (65, 22), (128, 22), (129, 21), (1100, 18)):
        assert DE.max_span(n) == r
    for n in (1, 2, 4, 8, 64, 128, 1024):
        assert n * 2 ** (DE.max_span(n) + 24) == 2 ** 53
    for n in range(1, 1200):
        assert n * 2 ** (DE.max_span(n) + 24) <= 2 ** 53 < n * 2 ** (DE.max_span(n) + 25)
