"""Reference restarted GMRES for the tests of GMRESSolver (host/krylov.hip; tests/test_gmres_reference_host.py, tests/test_gpu_gmres.py): plain numpy,
in the style of tests/pcg_reference.py, whose constants it reuses.

gmres() is a transcription of MFEM's GMRESSolver::Mult with iterative_mode = false - preconditioner on the left, r = M^-1 b, beta = |r|,
final = max(rel beta, abs), Arnoldi with plane rotations in the overflow-safe form, stop when |s_i+1| <= final, x += V y at a stop and at the end of a
cycle of kdim columns, then r = M^-1 (b - A x) - in np.longdouble, with weighted dot products and an essential mask.  As in the solver under test the
iteration cap returns the iterate of the columns done so far without another residual evaluation, h_i+1,i = 0 is convergence when the residual says
so and a breakdown otherwise, and nothing divides by zero.  It keeps the residual norm and the iterate of every Arnoldi step.

The same function in float64 with the addends of every dot product permuted, in both orthogonalisation orders (modified Gram-Schmidt and classical
Gram-Schmidt with a second pass), is an equally valid evaluation of the same method; how far those runs move from the long-double one at iteration k
is the reference's own SENSITIVITY there, and every tolerance of the GPU tests is X_FACTOR times it, with the floor X_FLOOR of max |x_k|.

History.choose() is the chooser of pcg_reference.History on the squares of the residual norms: resid_k^2 <= GAP min of the earlier squares, the
threshold their geometric mean, tol_x at most STEP_FRACTION of the step."""
import numpy as np

import pcg_reference as R
from pcg_reference import CONVERGED, MAX_ITER, BREAKDOWN, K_MAX, GAP, X_FACTOR, X_FLOOR, STEP_FRACTION  # noqa: F401

ORDERS = ("mgs", "cgs2")


def _rotation(dx, dy, T):
    """GeneratePlaneRotation: the quotient taken is the one of magnitude <= 1; a column that is zero from the diagonal down gets the swap, so that
    the residual stays what it was"""
    if dy == 0:
        return (T(0), T(1)) if dx == 0 else (T(1), T(0))
    if abs(dy) > abs(dx):
        t = dx / dy
        sn = T(1) / np.sqrt(T(1) + t * t)
        return t * sn, sn
    t = dy / dx
    cs = T(1) / np.sqrt(T(1) + t * t)
    return cs, t * cs


def _back_substitute(H, s, k, T):
    y = np.zeros(k, T)
    for i in range(k - 1, -1, -1):
        t = s[i] - np.sum(H[i, i + 1:k] * y[i + 1:k], dtype=T)
        y[i] = T(0) if H[i, i] == 0 else t / H[i, i]
    if not np.all(np.isfinite(y.astype(np.float64))):
        y[:] = 0
    return y


def gmres(apply, b, rel_tol, abs_tol, max_iter, kdim, weight=None, ess=None, dinv=None, Minv=None, dtype=np.longdouble, perm_seed=None, order="cgs2"):
    """x = A^-1 b from x = 0 by GMRES(kdim), left-preconditioned.  Arguments as pcg_reference.pcg; order: "mgs", "cgs2" (a second pass always) or
    "cgs1" (one pass).  Returns dict(res: [beta0, resid_1, ...] one entry per iterate, x: [x_0 = 0, x_1, ...], iters, flag, restarts, beta0)."""
    T = dtype
    n = len(b)
    w = np.ones(n, T) if weight is None else np.asarray(weight, T)
    free = np.ones(n, bool) if ess is None else ~np.asarray(ess, bool)
    perm = None if perm_seed is None else np.random.default_rng(perm_seed).permutation(n)
    dv = None if dinv is None else np.asarray(dinv, T)
    Mi = None if Minv is None else np.asarray(Minv, T)

    def dot(a, c):
        t = w * a * c
        return np.sum(t if perm is None else t[perm], dtype=T)

    def act(d):
        y = np.asarray(apply(np.where(free, d, T(0))), T)
        return np.where(free, y, T(0))

    def prec(r):
        return r.copy() if dv is None and Mi is None else (dv * r if Mi is None else Mi @ r)

    bm = np.where(free, np.asarray(b, T), T(0))
    x = np.zeros(n, T)
    r = prec(bm)
    beta = np.sqrt(dot(r, r))
    out = dict(res=[beta], x=[x.copy()], iters=0, flag=MAX_ITER, restarts=0, beta0=beta)
    if not np.isfinite(float(beta)):
        out["flag"] = BREAKDOWN
        return out
    final = max(T(rel_tol) * beta, T(abs_tol))
    if beta <= final:
        out["flag"] = CONVERGED
        return out
    j = 0
    while True:
        V = [r / beta]
        s = np.zeros(kdim + 1, T); s[0] = beta
        H = np.zeros((kdim + 1, kdim), T)
        cs = np.zeros(kdim, T); sn = np.zeros(kdim, T)
        x0 = x.copy()
        for i in range(kdim):
            if j >= max_iter:
                out["flag"] = MAX_ITER
                return out
            wv = prec(act(V[i]))
            if order == "mgs":
                for k in range(i + 1):
                    H[k, i] = dot(wv, V[k])
                    wv = wv - H[k, i] * V[k]
            else:
                for _ in range(2 if order == "cgs2" else 1):
                    c = [dot(wv, V[k]) for k in range(i + 1)]
                    for k in range(i + 1):
                        wv = wv - c[k] * V[k]
                        H[k, i] += c[k]
            hn = np.sqrt(dot(wv, wv))
            H[i + 1, i] = hn
            for k in range(i):
                H[k, i], H[k + 1, i] = cs[k] * H[k, i] + sn[k] * H[k + 1, i], -sn[k] * H[k, i] + cs[k] * H[k + 1, i]
            cs[i], sn[i] = _rotation(H[i, i], H[i + 1, i], T)
            H[i, i], H[i + 1, i] = cs[i] * H[i, i] + sn[i] * H[i + 1, i], -sn[i] * H[i, i] + cs[i] * H[i + 1, i]
            s[i], s[i + 1] = cs[i] * s[i] + sn[i] * s[i + 1], -sn[i] * s[i] + cs[i] * s[i + 1]
            resid = abs(s[i + 1])
            j += 1
            y = _back_substitute(H, s, i + 1, T)
            x = x0.copy()
            for k in range(i + 1):
                x = x + y[k] * V[k]
            out["res"].append(resid); out["x"].append(x.copy()); out["iters"] = j
            if not (np.isfinite(float(resid)) and np.isfinite(float(hn))):
                out["flag"] = BREAKDOWN
                return out
            if resid <= final:
                out["flag"] = CONVERGED
                return out
            if hn == 0:
                out["flag"] = BREAKDOWN
                return out
            if j >= max_iter:
                out["flag"] = MAX_ITER
                return out
            V.append(wv / hn)
        r = prec(bm - act(x))
        beta = np.sqrt(dot(r, r))
        out["restarts"] += 1
        if not np.isfinite(float(beta)):
            out["flag"] = BREAKDOWN
            return out
        if beta <= final:
            out["flag"] = CONVERGED
            return out


class History(R.History):
    """the capped reference run of one system under GMRES(kdim) (rel_tol = abs_tol = 0, max_iter = kmax) in long double, and its sensitivity from
    float64 runs with permuted dot products in both orthogonalisation orders (or the orders named).  bn holds the SQUARES of the residual norms, so the chooser, the
    thresholds and rel_tol(k) of pcg_reference.History apply as they stand: resid_k <= rel beta0 is resid_k^2 <= rel^2 beta0^2."""

    def __init__(self, apply, b, kdim, kmax=K_MAX, seeds=(1, 2, 3), apply64=None, orders=ORDERS, **kw):
        """orders: the orthogonalisation orders of the float64 reruns - ORDERS for every solver mode with a stable order; ("cgs1",) for the reduction
        a one-pass solve reports (see tests/test_gpu_gmres.py::test_every_orthogonalisation)"""
        self.kmax, self.kdim, self.orders = kmax, kdim, tuple(orders)
        ref = gmres(apply, b, 0.0, 0.0, kmax, kdim, **kw)
        self.res = np.array(ref["res"], np.longdouble)
        self.bn = self.res * self.res
        self.x = ref["x"]
        self.n = len(self.bn) - 1
        self.xmax = np.array([float(np.abs(x).max()) for x in self.x])
        self.step = np.array([0.0] + [float(np.abs(self.x[k] - self.x[k - 1]).max()) for k in range(1, self.n + 1)])
        self.red = self.res / self.res[0] if self.res[0] > 0 else np.zeros(self.n + 1, np.longdouble)
        self.sens_bn = np.zeros(self.n + 1); self.sens_x = np.zeros(self.n + 1); self.sens_red = np.zeros(self.n + 1)
        for order in self.orders:
            for sd in seeds:
                alt = gmres(apply if apply64 is None else apply64, b, 0.0, 0.0, kmax, kdim, dtype=np.float64, perm_seed=sd, order=order, **kw)
                assert len(alt["res"]) - 1 == self.n, "the float64 run ended at another iterate than the long-double run: %d against %d" % (len(alt["res"]) - 1, self.n)
                for k in range(self.n + 1):
                    a = np.longdouble(alt["res"][k])
                    if self.bn[k] != 0:
                        self.sens_bn[k] = max(self.sens_bn[k], float(abs(a * a - self.bn[k]) / self.bn[k]))
                    if self.red[k] != 0:
                        self.sens_red[k] = max(self.sens_red[k], float(abs(a / np.longdouble(alt["res"][0]) - self.red[k]) / self.red[k]))
                    if self.xmax[k] > 0:
                        self.sens_x[k] = max(self.sens_x[k], float(np.abs(np.asarray(alt["x"][k], np.longdouble) - self.x[k]).max()) / self.xmax[k])

    def restarts(self, k):
        """restarts a solve that ends at iterate k >= 1 has taken"""
        return (k - 1) // self.kdim if k >= 1 else 0


def nonsymmetric_system(n, seed, skew=0.07):
    """pcg_reference.spd_system plus a skew-symmetric part of relative size `skew` (Frobenius), essential rows and columns zero"""
    A, ess, b = R.spd_system(n, seed)
    rng = np.random.default_rng(seed + 7919)
    S = rng.standard_normal((n, n)); S = S - S.T
    S[ess, :] = 0.0; S[:, ess] = 0.0
    return A + S * (skew * np.linalg.norm(A) / np.linalg.norm(S)), ess, b
