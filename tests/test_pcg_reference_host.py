"""The reference conjugate-gradient solve of tests/pcg_reference.py on its own (no GPU): on synthetic SPD systems of 192 and 1536 unknowns with a 15 %
essential set and Jacobi scaling it reaches the direct solution, its chooser keeps its conditions, and the special cases give the counts and flags the
GPU tests (tests/test_gpu_pcg_reference.py) ask of the solver."""
import numpy as np
import pytest

import pcg_reference as R

_cache = {}


def _system(n):
    if n not in _cache:
        A, ess, b = R.spd_system(n, seed=11 + n)
        ld, f64 = R.dense_apply(A)
        _cache[n] = dict(A=A, ess=ess, b=b, ld=ld, f64=f64, dinv=R.jacobi_dinv(A, ess))
    return _cache[n]


def _history(n, jacobi):
    key = ("h", n, jacobi)
    if key not in _cache:
        s = _system(n)
        _cache[key] = R.History(s["ld"], s["b"], apply64=s["f64"], ess=s["ess"], dinv=s["dinv"] if jacobi else None)
    return _cache[key]


@pytest.mark.parametrize("n", [192, 1536])
@pytest.mark.parametrize("jacobi", [False, True], ids=["identity", "jacobi"])
def test_reference_reaches_the_direct_solution(n, jacobi):
    """driven to rel_tol = 1e-12 the reference agrees with np.linalg.solve on the free rows: within 1e-12 cond(A_ff) |x| of it, as a relative
    reduction of the (preconditioned) residual by 1e-12 allows, and the essential entries stay exactly 0"""
    s = _system(n)
    f = ~s["ess"]
    Aff = s["A"][np.ix_(f, f)]
    want = np.linalg.solve(Aff, s["b"][f])
    got = R.pcg(s["ld"], s["b"], 1e-12, 0.0, 20 * n, ess=s["ess"], dinv=s["dinv"] if jacobi else None)
    assert got["flag"] == R.CONVERGED and got["indefinite"] == 0
    x = np.asarray(got["x"][-1], np.float64)
    assert np.all(x[s["ess"]] == 0.0)
    err = np.abs(x[f] - want).max() / np.abs(want).max()
    bound = 1e-12 * np.linalg.cond(Aff)
    print("n = %d, %s: %d iterations, max |x - direct| / max |x| = %.3e (bound %.3e)" % (n, "jacobi" if jacobi else "identity", got["iters"], err, bound))
    assert err <= bound
    assert got["bn"][-1] <= 1e-24 * got["bn"][0] < got["bn"][-2]


@pytest.mark.parametrize("n", [192, 1536])
@pytest.mark.parametrize("jacobi", [False, True], ids=["identity", "jacobi"])
def test_chooser_conditions_hold_for_its_pick(n, jacobi):
    h = _history(n, jacobi)
    for prefer in (None, 1, 4, 5, 8):
        k, rel = h.choose(prefer)
        print(("prefer %s: " % prefer) + h.describe(k) + ", rel_tol %.6e" % rel)
        assert 1 <= k <= R.K_MAX
        assert h.bn[k] <= 0.8 * h.bn[:k].min()
        assert h.sens_bn[k] <= 1e-6
        assert h.tol_x(k) == max(100.0 * h.sens_x[k], 1e-13) and h.tol_x(k) <= 0.01 * h.step[k] / h.xmax[k]
        thr = rel * rel * float(h.bn[0])
        assert float(h.bn[k]) <= thr / 1.11 and thr * 1.11 <= float(h.bn[:k].min())      # the threshold clears both neighbours by 11 %
        # the reference itself, run with that rel_tol, stops at k - in long double and in permuted float64 alike
        s = _system(n)
        for kw in (dict(), dict(dtype=np.float64, perm_seed=5)):
            got = R.pcg(s["f64"] if kw else s["ld"], s["b"], rel, 0.0, 200, ess=s["ess"], dinv=s["dinv"] if jacobi else None, **kw)
            assert (got["iters"], got["flag"]) == (k, R.CONVERGED)
    # the figures of the construction: the sensitivity of x_k stays far below the steps up to k = 20
    assert h.sens_x[:21].max() < 1e-12 and (h.step[1:21] / h.xmax[1:21]).min() > 1e-4


def test_inadmissible_iterations_are_refused():
    """an iteration whose (r, z) rose is never picked, whatever is preferred"""
    h = _history(192, False)
    rose = [k for k in range(1, h.n + 1) if h.bn[k] > h.bn[:k].min()]
    adm = h.admissible()
    assert not set(rose) & set(adm)
    for k in rose[:3]:
        assert h.choose(k)[0] != k


@pytest.mark.parametrize("jacobi", [False, True], ids=["identity", "jacobi"])
def test_special_cases(jacobi):
    s = _system(192)
    kw = dict(ess=s["ess"], dinv=s["dinv"] if jacobi else None)
    h = _history(192, jacobi)
    # b = 0: no iteration, converged, x = 0 (and the reported reduction is 0: (r0, z0) = 0)
    z = R.pcg(s["ld"], np.zeros(192), 1e-8, 0.0, 50, **kw)
    assert (z["iters"], z["flag"]) == (0, R.CONVERGED) and not np.any(z["x"][-1]) and z["bn"] == [0]
    z = R.pcg(s["ld"], np.zeros(192), 0.0, 0.0, 50, **kw)
    assert (z["iters"], z["flag"]) == (0, R.CONVERGED)
    # a cap of m: m iterations, MAX_ITER, the m-th iterate of the uncapped run
    for m in (1, 3, 4, 5, 8):
        c = R.pcg(s["ld"], s["b"], 0.0, 0.0, m, **kw)
        assert (c["iters"], c["flag"]) == (m, R.MAX_ITER) and len(c["x"]) == m + 1
        assert np.array_equal(c["x"][m], h.x[m]) and c["bn"][m] == h.bn[m]
    # abs_tol governs: rel_tol = 0 and abs_tol^2 = the threshold of the centred stop give the count of the rel_tol stop
    k, rel = h.choose()
    a = R.pcg(s["ld"], s["b"], 0.0, np.sqrt(h.threshold(k)), 200, **kw)
    r = R.pcg(s["ld"], s["b"], rel, 0.0, 200, **kw)
    assert (a["iters"], a["flag"]) == (r["iters"], r["flag"]) == (k, R.CONVERGED)
    assert np.array_equal(a["x"][-1], r["x"][-1])
    # a stop exactly at the cap counts as converged
    c = R.pcg(s["ld"], s["b"], rel, 0.0, k, **kw)
    assert (c["iters"], c["flag"]) == (k, R.CONVERGED)


def test_dense_preconditioner_and_weights():
    """a dense M^-1 equal to diag(dinv) gives the iterates of the vector form; weights that double every addend double (r, z) and leave x alone"""
    s = _system(192)
    a = R.pcg(s["ld"], s["b"], 0.0, 0.0, 10, ess=s["ess"], dinv=s["dinv"])
    b = R.pcg(s["ld"], s["b"], 0.0, 0.0, 10, ess=s["ess"], Minv=np.diag(s["dinv"]))
    c = R.pcg(s["ld"], s["b"], 0.0, 0.0, 10, ess=s["ess"], dinv=s["dinv"], weight=np.full(192, 2.0))
    for k in range(11):
        assert np.abs(a["x"][k] - b["x"][k]).max() <= 1e-17 * max(np.abs(a["x"][k]).max(), 1) and np.array_equal(a["x"][k], c["x"][k])
        assert c["bn"][k] == 2 * a["bn"][k]
