"""Reference conjugate-gradient solve for the tests of host/krylov.hip (tests/test_pcg_reference_host.py, tests/test_gpu_pcg_reference.py): plain numpy.

pcg() is a transcription of MFEM's CGSolver::Mult with iterative_mode = false - the order of operations, the stopping test
(r, z) <= max(rel^2 (r0, z0), abs^2) after every update and the iteration cap that oracle/driver_port.hpp::cg_solve and the host loop of
PCGSolver::SolveMultigrid follow as well - in np.longdouble, with weighted dot products and an essential mask.  It keeps the history of (r, z) and
every iterate.  The same function in float64 with the addends of every dot product permuted is a second, equally valid evaluation of the same
recurrence; how far it moves away from the long-double run at iteration k is the reference's own SENSITIVITY there, and every tolerance of the
GPU tests is a multiple of it (never a fixed number on x: by k = 40 a 192-unknown system has lost orthogonality and the sensitivity of x_k has
grown to 1e-6).

choose() picks a stopping iteration whose threshold sits well inside a gap of the (r, z) history, so that a solver that is right must stop exactly
there, and at which an iterate off by one step stands out by a factor of a hundred over the tolerance."""
import numpy as np

CONVERGED, MAX_ITER, BREAKDOWN = 1, 2, -1      # values of the solver's flag (pcg_slots.hpp)
K_MAX = 25                                      # no stop later than this: the recurrence is still well conditioned (see above)
GAP = 0.8                                       # bn[k] <= GAP min(bn[:k]): the geometric-mean threshold clears both neighbours by >= 11 %
SENS_BN_MAX = 1e-6                              # relative sensitivity of bn[k] allowed
X_FACTOR, X_FLOOR = 100.0, 1e-13                # tol_x = max(X_FACTOR sensitivity of x_k, X_FLOOR) of max |x_k| ...
STEP_FRACTION = 0.01                            # ... and at most this part of max |x_k - x_(k-1)|


def pcg(apply, b, rel_tol, abs_tol, max_iter, weight=None, ess=None, dinv=None, Minv=None, dtype=np.longdouble, perm_seed=None):
    """x = A^-1 b from x = 0 by preconditioned conjugate gradients, MFEM's CGSolver::Mult.

    apply: callable d -> A d (any float array in, anything convertible out); b: right-hand side; weight: one weight per entry of the dot products
    (None: ones); ess: boolean mask of essential entries - zeroed in b, in the input and in the output of every action (None: none);
    dinv: diagonal preconditioner z = dinv r, Minv: dense preconditioner z = Minv r (neither: the identity); dtype: the arithmetic;
    perm_seed: the addends of every dot product are summed in this permutation (None: as they stand).
    Returns dict(bn: [(r0, z0), (r1, z1), ...] one entry per iterate, x: [x_0 = 0, x_1, ...], iters, flag, indefinite)."""
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

    rel, ab = T(rel_tol), T(abs_tol)
    x = np.zeros(n, T)
    r = np.where(free, np.asarray(b, T), T(0))
    z = prec(r)
    d = z.copy()
    nom0 = nom = dot(d, r)
    out = dict(bn=[nom0], x=[x.copy()], iters=0, flag=MAX_ITER, indefinite=0)
    if nom < 0:                                   # the preconditioner is not positive definite
        out["flag"] = BREAKDOWN
        return out
    r0 = max(nom * rel * rel, ab * ab)
    if nom <= r0:
        out["flag"] = CONVERGED
        return out
    z = act(d)
    den = dot(z, d)
    if den <= 0:
        if dot(d, d) > 0:
            out["indefinite"] += 1
        if den == 0:
            out["flag"] = BREAKDOWN
            return out
    i = 1
    while True:
        alpha = nom / den
        x = x + alpha * d
        r = r - alpha * z
        z = prec(r)
        betanom = dot(r, z)
        out["bn"].append(betanom); out["x"].append(x.copy()); out["iters"] = i
        if betanom < 0:
            out["flag"] = MAX_ITER
            break
        if betanom <= r0:
            out["flag"] = CONVERGED
            break
        i += 1
        if i > max_iter:
            out["flag"] = MAX_ITER
            break
        beta = betanom / nom
        d = z + beta * d
        z = act(d)
        den = dot(d, z)
        if den <= 0:
            if dot(d, d) > 0:
                out["indefinite"] += 1
            if den == 0:
                out["flag"] = BREAKDOWN
                break
        nom = betanom
    return out


class History:
    """the capped reference run of one system (rel_tol = abs_tol = 0, max_iter = kmax) in long double, and its sensitivity from `seeds` float64 runs
    with permuted dot products: per iterate k the largest deviation of (r_k, z_k), of sqrt((r_k, z_k) / (r0, z0)) and of x_k among them"""

    def __init__(self, apply, b, kmax=K_MAX, seeds=(1, 2, 3), apply64=None, **kw):
        self.kmax = kmax
        ref = pcg(apply, b, 0.0, 0.0, kmax, **kw)
        self.bn = np.array(ref["bn"], np.longdouble)
        self.x = ref["x"]
        self.n = len(self.bn) - 1                 # iterates available (kmax unless (r, z) reached 0 or a breakdown came first)
        self.xmax = np.array([float(np.abs(x).max()) for x in self.x])
        self.step = np.array([0.0] + [float(np.abs(self.x[k] - self.x[k - 1]).max()) for k in range(1, self.n + 1)])
        self.red = np.sqrt(np.maximum(self.bn, 0) / self.bn[0]) if self.bn[0] > 0 else np.zeros(self.n + 1, np.longdouble)
        self.sens_bn = np.zeros(self.n + 1); self.sens_x = np.zeros(self.n + 1); self.sens_red = np.zeros(self.n + 1)
        for sd in seeds:
            alt = pcg(apply if apply64 is None else apply64, b, 0.0, 0.0, kmax, dtype=np.float64, perm_seed=sd, **kw)
            m = min(self.n, len(alt["bn"]) - 1)
            assert m == self.n, "the float64 run ended at another iterate than the long-double run: %d against %d" % (len(alt["bn"]) - 1, self.n)
            for k in range(self.n + 1):
                a = np.longdouble(alt["bn"][k])
                if self.bn[k] != 0:
                    self.sens_bn[k] = max(self.sens_bn[k], float(abs(a - self.bn[k]) / abs(self.bn[k])))
                if self.red[k] != 0:
                    self.sens_red[k] = max(self.sens_red[k], float(abs(np.sqrt(max(a, 0) / np.longdouble(alt["bn"][0])) - self.red[k]) / self.red[k]))
                if self.xmax[k] > 0:
                    self.sens_x[k] = max(self.sens_x[k], float(np.abs(np.asarray(alt["x"][k], np.longdouble) - self.x[k]).max()) / self.xmax[k])

    def tol_x(self, k):
        """tolerance on x_k, relative to max |x_k|"""
        return max(X_FACTOR * self.sens_x[k], X_FLOOR)

    def tol_red(self, k):
        """tolerance on the reported reduction at iterate k, relative"""
        return X_FACTOR * self.sens_red[k]

    def x_ok(self, k):
        """an iterate off by one step can never hide inside tol_x(k)"""
        return k >= 1 and self.xmax[k] > 0 and self.tol_x(k) <= STEP_FRACTION * self.step[k] / self.xmax[k]

    def conditions(self, k):
        """the three conditions of a threshold-centred stop at k, as (gap, sensitivity of bn, tolerance against step)"""
        return (bool(1 <= k <= min(self.n, K_MAX) and self.bn[k] <= GAP * self.bn[:k].min()), bool(k <= self.n and self.sens_bn[k] <= SENS_BN_MAX), bool(k <= self.n and self.x_ok(k)))

    def admissible(self):
        return [k for k in range(1, min(self.n, K_MAX) + 1) if all(self.conditions(k))]

    def threshold(self, k):
        """geometric mean of bn[k] and min(bn[:k])"""
        return float(np.sqrt(self.bn[k] * self.bn[:k].min()))

    def rel_tol(self, k):
        """the rel_tol whose threshold rel^2 (r0, z0) is threshold(k)"""
        return float(np.sqrt(np.sqrt(self.bn[k] * self.bn[:k].min()) / self.bn[0]))

    def choose(self, prefer=None):
        """(k, rel_tol): the admissible stopping iteration nearest to `prefer` (None: the last one) - the later one of two equally near"""
        adm = self.admissible()
        assert adm, "no admissible stopping iteration up to %d: choose another right-hand side" % K_MAX
        k = adm[-1] if prefer is None else min(adm, key=lambda j: (abs(j - prefer), -j))
        return k, self.rel_tol(k)

    def describe(self, k):
        return ("k = %d, (r, z) %.6e against min before %.6e (threshold %.6e), sensitivity: (r, z) %.2e, reduction %.2e, x %.2e; tol_x %.2e of max |x_k|, step %.2e of max |x_k|"
                % (k, float(self.bn[k]), float(self.bn[:k].min()) if k else float("nan"), self.threshold(k) if k else float("nan"), self.sens_bn[k], self.sens_red[k], self.sens_x[k],
                   self.tol_x(k), self.step[k] / self.xmax[k] if self.xmax[k] > 0 else float("nan")))


def spd_system(n, seed, ess_fraction=0.15, cond=50.0):
    """a random symmetric positive definite matrix with the rows and columns of a random essential set zeroed (as the masked operator K_uu has them),
    its mask and a right-hand side with zero essential entries"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.exp(rng.uniform(0.0, np.log(cond), n))
    s = np.exp(rng.uniform(-0.5, 0.5, n))       # a diagonal scaling for the Jacobi preconditioner to undo
    A = (Q * lam) @ Q.T
    A = 0.5 * (A + A.T) * s[:, None] * s[None, :]
    ess = rng.uniform(size=n) < ess_fraction
    A[ess, :] = 0.0; A[:, ess] = 0.0
    b = rng.standard_normal(n); b[ess] = 0.0
    return A, ess, b


def jacobi_dinv(A, ess):
    """1 / diag on free rows, 1 on essential rows"""
    d = np.diag(A).copy()
    d[ess] = 1.0
    return 1.0 / d


def dense_apply(A):
    """the action of a dense matrix in long double and in float64"""
    Al = np.asarray(A, np.longdouble); A64 = np.asarray(A, np.float64)
    return (lambda d: Al @ d), (lambda d: A64 @ d)
