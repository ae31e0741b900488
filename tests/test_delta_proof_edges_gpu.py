"""The difference-array kernels at the edges of their exactness proof, on a real MI355X (tests/delta_edges.py; the emulator's
half is tests/test_delta_proof_edges.py).

Span R = 29 - ceil(lg N): exact route, nothing refused, Sum / Mean bit for bit the sequential f64 sum.  Span R + 1: the window
is refused and its values are the general kernel's -- bit for bit the sequential sum again, which for a power of two N >= 8
differs from the exact sum the kernel would have returned had it accepted the window.  Var / StdDev / CV: 1e-12 relative to
the exact rational value, coordinates bit for bit.  Every case at 2048-bp windows (WTAMD_DELTA_T=256); cases 1, 3 and 7
also at the default plan (8192-bp windows, 1024 lanes: 1100 tracks are two chunks there, five at 256 lanes).

Routes, from TrackSet.stats(): kernel == 1 and patched_windows == 0 (exact), patched_windows >= 1 (few windows refused),
kernel == 0 (so many refused that the general kernel redid the input)."""
import pytest

import delta_edges as DE
from helpers import assert_runs_equal

pytestmark = pytest.mark.gpu

PLANS = {"T256": ("256", 2048), "default": (None, 8192)}
SPECS = [("T256",) + s for s in DE.specs(device=True)] + \
        [("default",) + s for s in DE.specs(device=True, only=("span_edge", "through_base", "chunked"))]


@pytest.fixture(scope="module")
def engine():
    import torch
    assert torch.cuda.is_available()
    from wiggletools_amd import engine as E
    return E


def _tol(op):
    return 1e-12 if op in DE.VAR_OPS else 0.0


def _check_route(case, st, what):
    r = case.route
    if r == "exact":
        assert st["kernel"] == 1 and st["patched_windows"] == 0, what
        assert st["window_bp"] == case.W and st["n_windows"] == case.n_windows, what
    elif r == "patched":
        assert st["kernel"] == 1 and st["patched_windows"] >= 1, what
    elif r == "fallback":
        assert st["kernel"] == 0 and st["patched_windows"] == 0, what
    elif r == "refused":
        assert st["kernel"] == 0 or st["patched_windows"] >= 1, what
    elif r == "near":
        assert st["kernel"] == 1, what
    else:
        assert r == "off" and st["kernel"] == 0 and st["patched_windows"] == 0, what


@pytest.mark.parametrize("spec", SPECS, ids=["%s-%s" % (s[0], s[1]) for s in SPECS])
def test_gpu_delta_proof_edge(oracle, engine, spec, monkeypatch):
    plan, _, fn, kw = spec
    T, W = PLANS[plan]
    monkeypatch.setenv("WTAMD_DELTA_MIN_TRACKS", "1")
    if T is None:
        monkeypatch.delenv("WTAMD_DELTA_T", raising=False)
    else:
        monkeypatch.setenv("WTAMD_DELTA_T", T)
    case = fn(W=W, **kw)
    assert len(case.expected("sum")[0]) == case.n_runs
    if case.sensitive:
        assert not all(DE.sequential_is_exact(case)), "%s: not sensitive" % case.name
    if case.sensitive_rn:
        assert not all(DE.sequential_is_rounded_exact(case)), "%s: not sensitive to a trusted integer sum" % case.name
    d = case.t.as_dict()
    ts = engine.TrackSet.from_runlists(case.t)
    try:
        for op in case.ops:
            for strict in ((0, 1) if op in ("sum", "mean") else (0,)):
                exp = case.expected(op, strict)
                assert_runs_equal(exp, oracle.reduce(d, op, flags=strict), _tol(op), "%s %s: plain reference vs oracle" % (case.name, op))
                got = ts.reduce_host(op, flags=strict)
                st = ts.stats()
                what = "%s %s %s strict %d %s" % (plan, case.name, op, strict, st)
                print("ROUTE %s %s %s strict %d: kernel %d patched_windows %d window_bp %d n_windows %d" %
                      (plan, case.name, op, strict, st["kernel"], st["patched_windows"], st["window_bp"], st["n_windows"]))
                _check_route(case, st, what)
                assert_runs_equal(got, exp, _tol(op), what)
    finally:
        ts.close()
