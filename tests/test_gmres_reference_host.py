"""GMRES without a GPU: the numpy reference the GPU tests compare with (tests/gmres_reference.py) against an independent least-squares minimiser, the
small algebra of the scalar kernel through exa_gmres_column_probe (the shared header gmres_small.hpp, compiled for the host), and the options
Solvers.Krylov.solver = "GMRES" / gmres_kdim."""
import ctypes as C
import os

import numpy as np
import pytest

import gmres_reference as G
import pcg_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "refdata")
EPS = np.finfo(np.float64).eps

SYSTEMS = [(192, 1), (375, 2)]


def _system(n, seed, jacobi):
    A, ess, b = G.nonsymmetric_system(n, seed)
    assert np.linalg.norm(A - A.T) / np.linalg.norm(A) > 0.05
    weight = np.random.default_rng(seed + 31).uniform(0.5, 1.0, n)
    dinv = R.jacobi_dinv(A, ess) if jacobi else None
    return A, ess, b, weight, dinv


@pytest.mark.parametrize("jacobi", [False, True], ids=["identity", "jacobi"])
@pytest.mark.parametrize("n,seed", SYSTEMS)
def test_iterates_minimise_the_preconditioned_residual(n, seed, jacobi):
    """iterate k of the unrestarted run is argmin |M^-1 (b - A x)|_W over x in the Krylov space K_k(M^-1 A, M^-1 b), for k <= 12: the space is built
    explicitly, one QR per added vector, and the minimiser comes from numpy's lstsq.  Tolerance: 100 eps cond of the projected matrix, of max |x_k|."""
    A, ess, b, weight, dinv = _system(n, seed, jacobi)
    ld, _ = R.dense_apply(A)
    ref = G.gmres(ld, b, 0.0, 0.0, 12, 30, weight=weight, ess=ess, dinv=dinv)
    assert ref["iters"] == 12 and ref["flag"] == G.MAX_ITER and ref["restarts"] == 0
    B = A if dinv is None else dinv[:, None] * A
    r0 = b if dinv is None else dinv * b
    sw = np.sqrt(weight)
    Q = (r0 / np.linalg.norm(r0))[:, None]
    for k in range(1, 13):
        P = sw[:, None] * (B @ Q)
        z = np.linalg.lstsq(P, sw * r0, rcond=None)[0]
        xk = Q @ z
        cond = np.linalg.cond(P)
        dev = np.abs(np.asarray(ref["x"][k], np.float64) - xk).max() / np.abs(xk).max()
        res = np.linalg.norm(sw * (r0 - B @ xk))
        print("n %d %s k %2d: cond %.2e, |x_k - minimiser| %.2e of max |x_k| (tolerance %.2e), residual %.6e against %.6e"
              % (n, "jacobi" if jacobi else "identity", k, cond, dev, 100 * EPS * cond, float(ref["res"][k]), res))
        assert dev <= 100 * EPS * cond
        assert abs(float(ref["res"][k]) - res) <= 100 * EPS * cond * res
        Q, _ = np.linalg.qr(np.column_stack([Q, B @ Q[:, -1]]))


@pytest.mark.parametrize("n,seed", SYSTEMS)
def test_restarted_equals_chained_unrestarted(n, seed):
    """GMRES(5) at k = 5, 10, 15 is three fresh five-step solves chained on the residual; restarts are counted; histories do not increase"""
    A, ess, b, weight, dinv = _system(n, seed, True)
    ld, _ = R.dense_apply(A)
    kw = dict(weight=weight, ess=ess, dinv=dinv)
    run = G.gmres(ld, b, 0.0, 0.0, 15, 5, **kw)
    assert run["iters"] == 15 and run["restarts"] == 2
    x = np.zeros(n, np.longdouble)
    bl = np.where(ess, 0.0, b).astype(np.longdouble)
    for c in range(3):
        part = G.gmres(ld, bl - np.where(ess, 0, ld(x)), 0.0, 0.0, 5, 30, **kw)
        x = x + part["x"][5]
        dev = float(np.abs(x - run["x"][5 * (c + 1)]).max() / np.abs(x).max())
        print("n %d cycle %d: chained against restarted %.2e of max |x|" % (n, c, dev))
        assert dev <= R.X_FLOOR
    for kdim in (5, 20, 30):
        res = np.array(G.gmres(ld, b, 0.0, 0.0, 25, kdim, **kw)["res"], np.float64)
        assert np.all(res[1:] <= res[:-1] * (1 + 1e-12)), kdim
    assert G.gmres(ld, b, 0.0, 0.0, 5, 5, **kw)["restarts"] == 0 and G.gmres(ld, b, 0.0, 0.0, 6, 5, **kw)["restarts"] == 1
    z = G.gmres(ld, np.zeros(n), 1e-8, 0.0, 10, 5, **kw)
    assert z["iters"] == 0 and z["flag"] == G.CONVERGED and not z["x"][0].any()
    assert G.gmres(ld, b, 0.0, 0.0, 0, 5, **kw)["flag"] == G.MAX_ITER


@pytest.mark.parametrize("jacobi", [False, True], ids=["identity", "jacobi"])
@pytest.mark.parametrize("n,seed", SYSTEMS)
def test_chooser_finds_stops(n, seed, jacobi):
    """the chooser of pcg_reference on the squared residual norms: a centred stop exists under every Krylov dimension the GPU tests use, one after the
    second restart of GMRES(5) among them; the sensitivities leave the floor of tol_x in charge"""
    A, ess, b, weight, dinv = _system(n, seed, jacobi)
    ld, f64 = R.dense_apply(A)
    for kdim in (5, 20, 30):
        h = G.History(ld, b, kdim, apply64=f64, weight=weight, ess=ess, dinv=dinv)
        adm = h.admissible()
        print("n %d %s kdim %d: %d admissible stops of 25 %s; largest sensitivity: residual %.2e, x %.2e" % (n, "jacobi" if jacobi else "identity", kdim, len(adm), adm, h.sens_red.max(), h.sens_x.max()))
        assert adm
        k, rel = h.choose()
        assert h.bn[k] <= G.GAP * h.bn[:k].min() and h.tol_x(k) <= G.STEP_FRACTION * h.step[k] / h.xmax[k]
        stop = G.gmres(ld, b, rel, 0.0, 200, kdim, weight=weight, ess=ess, dinv=dinv)
        assert stop["iters"] == k and stop["flag"] == G.CONVERGED and stop["restarts"] == h.restarts(k)
        if kdim == 5:
            assert any(11 <= a <= 15 for a in adm)


# ---------------------------------------------------------------------------------------------------------------- the shared small algebra
def _hessenberg(seed, m=7):
    rng = np.random.default_rng(seed)
    H = np.triu(rng.standard_normal((m + 1, m)), -1)
    # scaled to cond <= 100: a dominant diagonal of the leading square block plus the random rest
    H[:m, :m] += 4.0 * np.eye(m)
    return H


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_column_probe_against_lstsq(seed):
    import exaconstit_amd.lib as L
    m = 7
    H = _hessenberg(seed, m)
    cond = np.linalg.cond(H)
    assert cond <= 100.0, cond
    beta = 1.7
    out = L.gmres_column_probe(H, beta)
    e1 = np.zeros(m + 1); e1[0] = beta
    for i in range(m):
        yi, res, _, _ = np.linalg.lstsq(H[:i + 2, :i + 1], e1[:i + 2], rcond=None)
        want = np.sqrt(res[0])
        assert abs(out["resid"][i] - want) <= 100 * EPS * cond * beta, (i, out["resid"][i], want)
    y = np.linalg.lstsq(H, e1, rcond=None)[0]
    print("seed %d: cond %.2f, |y - lstsq| %.2e, tolerance %.2e" % (seed, cond, np.abs(out["y"] - y).max(), 100 * EPS * cond * np.abs(y).max()))
    assert out["ok"] and np.abs(out["y"] - y).max() <= 100 * EPS * cond * np.abs(y).max()
    assert np.all(out["flags"] == 0)
    # with the bound between the last two residuals the last column converges
    fin = np.sqrt(out["resid"][-1] * out["resid"][-2])
    assert list(L.gmres_column_probe(H, beta, fin)["flags"][-2:]) == [0, G.CONVERGED]


def test_column_probe_zero_subdiagonal():
    """h_i+1,i = 0: no division anywhere.  An invariant subspace that holds the solution gives resid 0 and CONVERGED; a zero column gives BREAKDOWN,
    a zero pivot and y_i = 0"""
    import exaconstit_amd.lib as L
    H = _hessenberg(5, 3)
    H[3, 2] = 0.0                                  # the Krylov space is exhausted at the third column
    out = L.gmres_column_probe(H, 2.0, 1e-12)
    y = np.linalg.solve(H[:3, :3], np.array([2.0, 0.0, 0.0]))
    assert out["resid"][2] == 0.0 and out["flags"][2] == G.CONVERGED and out["ok"]
    assert np.abs(out["y"] - y).max() <= 100 * EPS * np.linalg.cond(H[:3, :3]) * np.abs(y).max()
    Z = np.zeros((3, 2)); Z[0, 0] = 1.0; Z[1, 0] = 1.0   # second column entirely zero: h_21 = 0 and a zero pivot
    with np.errstate(all="raise"):
        out = L.gmres_column_probe(Z, 1.0, 1e-12)
    assert out["flags"][1] == G.BREAKDOWN and not out["ok"] and out["y"][1] == 0.0 and np.all(np.isfinite(out["y"])) and np.all(np.isfinite(out["resid"]))
    with pytest.raises(ValueError):
        L.gmres_column_probe(np.zeros((102, 101)), 1.0)


# ---------------------------------------------------------------------------------------------------------------- options
def _query(tmp_path, edit):
    import exaconstit_amd.lib as L
    txt = open(os.path.join(REF, "voce_pa.toml")).read()
    for fl in ("props_cp_voce.txt", "state_cp_voce.txt", "voce_quats.ori", "grains.txt", "custom_dt.txt"):
        txt = txt.replace('"%s"' % fl, '"%s"' % os.path.join(REF, fl))
    assert 'solver = "PCG"' in txt
    f = tmp_path / "opt.toml"
    f.write_text(edit(txt))
    out = np.zeros(20); err = C.create_string_buffer(512)
    return L.exa_options_query(str(f).encode(), out.ctypes.data_as(C.POINTER(C.c_double)), err, 512), err.value.decode()


def test_options_gmres(tmp_path):
    rc, msg = _query(tmp_path, lambda t: t.replace('solver = "PCG"', 'solver = "GMRES"\n        gmres_kdim = 20'))
    assert rc == 0, msg
    rc, msg = _query(tmp_path, lambda t: t.replace('solver = "PCG"', 'gmres_kdim = 50'))      # no solver key: the reference's default
    assert rc == 0, msg
    rc, msg = _query(tmp_path, lambda t: t)
    assert rc == 0, msg
    for bad in ("0", "2.5", "101", '"x"', "-3", "true"):
        rc, msg = _query(tmp_path, lambda t: t.replace('solver = "PCG"', 'solver = "GMRES"\n        gmres_kdim = %s' % bad))
        assert rc == -1 and "gmres_kdim" in msg, (bad, msg)
    rc, msg = _query(tmp_path, lambda t: t.replace('solver = "PCG"', 'solver = "PCG"\n        gmres_kdim = 20'))
    assert rc == -1 and "gmres_kdim" in msg and "PCG" in msg
    # the refusals that were there stay, and the one of GMRES names the key that lifts it
    rc, msg = _query(tmp_path, lambda t: t.replace('solver = "PCG"', 'solver = "GMRES"'))
    assert rc == -1 and "PCG" in msg and "gmres_kdim" in msg
    rc, msg = _query(tmp_path, lambda t: t.replace('solver = "PCG"', 'solver = "MINRES"\n        gmres_kdim = 20'))
    assert rc == -1 and "not built" in msg
    rc, msg = _query(tmp_path, lambda t: t.replace('solver = "PCG"', 'solver = "MINRES"'))
    assert rc == -1 and "not built" in msg
