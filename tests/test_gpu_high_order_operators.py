"""The run-time-order kernels of gen_kernels.hip (orders 3 ... 6: k_pa_apply_stage1, k_pa_diag_gen, k_assemble_ea_rt, k_ea_apply_rt, k_eds,
k_residual_bbar, and the shape table read from global memory by k_jacobians, k_grad_calc, k_residual_apply ...) against the oracle on inputs
that can fail: a smoothly warped mesh (every adj(J) entry non-zero, det J varying), a tangent whose asymmetry is 30 % of its scale, seeded
random sigma, x and y0 (the += contract), dt != 1, E = 125 (two 64-element blocks, the second partial), a 10 % mask on the L-vector.
tests/test_high_order_inputs_host.py asserts on the oracle alone that each index slip these inputs are meant to catch moves the result by
at least 1e-6.  Bound: rel-L2 < 1e-12, the project's bound for the same comparisons at p <= 2 (test_gpu_parity.py) and on the reference's
own inputs (test_gpu_reference_unit_tests.py).  The oracle side is computed once per (p, N, integrator) and shared.

The partial-assembly action applies C, the assembled matrices apply C^T (column j holds B^T C B_j, the mat-vec sums over rows); the oracle
does the same.  The PA cases therefore also assert that the GPU action is NOT the assembled action of the same C (> 1e-3 away; the
assembled action of C is the oracle's PA action of C^T, an identity the host module asserts to 1e-13).

Refusals found at p >= 3 (return code EXA_ERR_UNSUPPORTED and the reason in exa_last_error asserted; the composition the driver runs
instead - restrict -> E-vector action -> transposed add, action route "generic_evector" - is checked in their place):
  * exa_grad_apply_lvec under partial assembly: the fused L-vector PA action is built for p = 1 and p = 2;
  * exa_grad_apply_lvec in deterministic mode, both assemblies: the fused action is ordered for p = 1 full integration only;
  * exa_residual_lvec: the fused residual is built for p = 1 full integration and p = 2;
  * exa_set_quadrature_layout(EXA_QLAYOUT_EB64): the element-blocked layout is built for p = 1 full integration and p = 2.
Not refused: the p = 6 element matrices of one element padded to a 64-lane block (0.54 GB).

Every test prints its measured rel-L2; EXA_WRITE_RECORDS=1 keeps the lines in profiles/high_order_checks.txt."""
import ctypes as C
import os

import numpy as np
import pytest

import hipref
from hipref import ptr, rel_l2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "high_order_checks.txt")
TOL = 1e-12
ORDERS = [3, 4, 5, 6]
EA_MESH = {3: 5, 4: 2, 5: 2, 6: 1}          # the oracle assembles these in 0.5 ... 4 s; p = 6: one element, 1029 x 1029
L_PA, L_EA, L_FULL, L_BBAR = 0, 1, 0, 1     # EXA_ASSEMBLY_PA / _EA, EXA_INTEG_FULL / _BBAR of include/exaconstit_hip.h (_open compares them with the library's)


class _Check:
    """the measured lines of one test: printed at once (a failing assertion must not swallow them), asserted, kept by record()"""

    def __init__(self, key):
        self.key, self.lines = key, []

    def say(self, text):
        print(text)
        self.lines.append(text)

    def close(self, what, got, ref, tol=TOL, onto=None):
        """`onto`: the vector the result was added to.  Its entries are O(1) and can outweigh the increment (a residual of this mesh is
        2e-3 of it, so a residual wrong by 1e-10 would pass a comparison of the sums), so the increment is compared as well, to the same
        bound.  The bound still holds for it: the oracle adds every point's contribution into y (fem_port.hpp, element_vector), rounding
        at the magnitude of y0 once per point, a random walk of 0.4 x 1.1e-16 x sqrt(Q) = 8e-16 at Q = 343, which is 4e-13 of a
        2e-3 increment; the kernels add a register sum once."""
        err = rel_l2(got, ref)
        if onto is None:
            self.say(f"{what}: rel-L2 {err:.3e} (< {tol:.0e})")
            assert err < tol, what
            return
        inc = rel_l2(got - onto, ref - onto)
        self.say(f"{what}: rel-L2 {err:.3e}, of the increment {inc:.3e} (< {tol:.0e})")
        assert err < tol and inc < tol, what

    def apart(self, what, got, ref, least):
        err = rel_l2(got, ref)
        self.say(f"{what}: rel-L2 {err:.3e} (> {least:.0e})")
        assert err > least, what

    def record(self):
        """profiles/pcg_checks.txt's convention: with EXA_WRITE_RECORDS=1 the lines replace the block '[key]' of the record file"""
        if os.environ.get("EXA_WRITE_RECORDS") != "1":
            return
        blocks, cur = {}, None
        if os.path.exists(RECORD):
            for ln in open(RECORD).read().splitlines():
                if ln.startswith("[") and ln.endswith("]"):
                    cur = ln[1:-1]; blocks[cur] = []
                elif cur is not None:
                    blocks[cur].append(ln)
        blocks[self.key] = list(self.lines)
        os.makedirs(os.path.dirname(RECORD), exist_ok=True)
        with open(RECORD, "w") as f:
            for k in sorted(blocks):
                f.write("[%s]\n%s\n" % (k, "\n".join(blocks[k])))


_refs = {}


def _ref(orc, p, N, what):
    """one oracle result per (p, N, what), computed on first use and left unchanged"""
    key = (p, N, what)
    if key not in _refs:
        inp = hipref.ho_inputs(orc, p, N)
        o = hipref.HighOrderOracle(orc, inp)
        if what in ("ea", "ea_bbar"):
            val = o.ea(bbar=what == "ea_bbar")
        elif what in ("ea_action", "ea_bbar_action"):
            val = o.ea_mult(_ref(orc, p, N, what[:-7]))
        elif what in ("ea_diag", "ea_bbar_diag"):
            val = o.ea_diag(_ref(orc, p, N, what[:-5]))
        else:
            val = {"residual": o.residual, "residual_bbar_dense": lambda: o.residual_bbar(dense=True), "residual_bbar_pa": lambda: o.residual_bbar(dense=False),
                   "pa_action": o.pa_action, "pa_diag": o.pa_diag,
                   "pa_action_of_Ct": lambda: o.pa_action(Cm=hipref.transpose_points(inp["Cm"], 6))}[what]()
        val.setflags(write=False)
        _refs[key] = val
    return _refs[key]


def _props(orc):
    return np.loadtxt(orc.REFDATA + "/props_cp_voce.txt").ravel()


def _open(orc, p, N, assembly, integ=0):
    """context + device, shape table checked, Jacobians of the warped mesh on the device (the oracle's: exa_jacobians has its own test)"""
    import exaconstit_amd.lib as L
    assert (L.EXA_ASSEMBLY_PA, L.EXA_ASSEMBLY_EA, L.EXA_INTEG_FULL, L.EXA_INTEG_BBAR) == (L_PA, L_EA, L_FULL, L_BBAR)
    inp = hipref.ho_inputs(orc, p, N)
    ctx = L.Context(L.EXA_FCC_VOCE, _props(orc), 298.0, p, inp["E"], assembly=assembly, integ=integ)
    assert (ctx.n, ctx.Q) == (inp["n"], inp["Q"])
    dev = hipref.Dev()
    return L, ctx, dev, inp, _up(dev, inp["J"])


def _up(dev, a):
    return dev.up(np.array(a))        # (a writable copy: the cached inputs are read-only)


def _refused(L, ctx, rc, *words):
    assert rc == L.EXA_ERR_UNSUPPORTED
    msg = L.exa_last_error(ctx.h).decode()
    for w in words:
        assert w in msg, msg
    return msg


@pytest.mark.parametrize("p", ORDERS)
def test_geometry_from_the_global_shape_table(oracle, p):
    """exa_jacobians, exa_grad_calc of a random E-vector field, exa_vol_avg of a random 6-component field; E = 125"""
    orc = oracle
    chk = _Check(f"geometry p={p} N=5")
    L, ctx, dev, inp, d_Jref = _open(orc, p, 5, L_PA)
    E, Q, n, P = inp["E"], inp["Q"], inp["n"], inp["P"]
    G, W = ctx.shape_table()
    chk.close("shape table G", G, inp["rve"]["G"]); chk.close("weights W", W, inp["rve"]["W"])
    d_xe = _up(dev, inp["xe"]); d_J = dev.zeros(9 * P)
    ctx.check(L.exa_jacobians(ctx.h, ptr(d_xe), ptr(d_J), None))
    chk.close("exa_jacobians", d_J.cpu().numpy(), inp["J"])
    grad = np.zeros(9 * P)
    orc.lib().orc_grad_calc(Q, E, n, orc._p(inp["J"]), orc._p(inp["rve"]["G"]), orc._p(inp["field"]), orc._p(grad))
    d_f = _up(dev, inp["field"]); d_g = dev.zeros(9 * P)
    ctx.check(L.exa_grad_calc(ctx.h, ptr(d_Jref), ptr(d_f), ptr(d_g), None))
    chk.close("exa_grad_calc", d_g.cpu().numpy(), grad)
    avg = np.zeros(6); orc.lib().orc_vol_avg(Q, E, 6, orc._p(inp["rve"]["W"]), orc._p(inp["J"]), orc._p(inp["qf"]), orc._p(avg), 1)
    out = np.zeros(7); d_qf = _up(dev, inp["qf"])
    ctx.check(L.exa_vol_avg(ctx.h, ptr(d_Jref), ptr(d_qf), 6, 1, out.ctypes.data_as(C.POINTER(C.c_double)), None))
    chk.close("exa_vol_avg", out[:6], avg)
    vol = float(np.dot(np.tile(inp["rve"]["W"], E), np.linalg.det(inp["J"].reshape(-1, 3, 3))))
    chk.close("exa_vol_avg volume", out[6:], [vol])
    # the element-blocked layout is refused at these orders
    msg = _refused(L, ctx, L.exa_set_quadrature_layout(ctx.h, L.EXA_QLAYOUT_EB64), "element-blocked layout")
    chk.say(f"refused: {msg}")
    ctx.close(); chk.record()


@pytest.mark.parametrize("p", ORDERS)
def test_plain_residual(oracle, p):
    """exa_residual_setup + exa_residual_apply onto a random y0 against the dense AssembleElementVector; E = 125"""
    orc = oracle
    chk = _Check(f"plain residual p={p} N=5")
    L, ctx, dev, inp, d_J = _open(orc, p, 5, L_PA)
    d_sig = _up(dev, inp["sig"]); d_y = _up(dev, inp["y0"])
    ctx.check(L.exa_residual_setup(ctx.h, ptr(d_J), ptr(d_sig), None))
    ctx.check(L.exa_residual_apply(ctx.h, ptr(d_y), None))
    chk.close("residual onto y0 vs orc_element_vector", d_y.cpu().numpy(), _ref(orc, p, 5, "residual"), onto=inp["y0"])
    # the fused L-vector residual is refused at these orders
    d_conn = dev.up(inp["rve"]["conn"]); ctx.check(L.exa_set_connectivity(ctx.h, ptr(d_conn), inp["NN"]))
    d_yL = dev.zeros(3 * inp["NN"])
    msg = _refused(L, ctx, L.exa_residual_lvec(ctx.h, ptr(d_J), ptr(d_sig), ptr(d_yL), None), "exa_residual_lvec", "p = 1")
    chk.say(f"refused: {msg}")
    assert not d_yL.cpu().numpy().any()
    ctx.close(); chk.record()


@pytest.mark.parametrize("p", ORDERS)
def test_bbar_residual(oracle, p):
    """B-bar residual (k_eds + k_residual_bbar) onto y0 against the dense B-bar element vector and against the oracle's AddMultPA; E = 125"""
    orc = oracle
    chk = _Check(f"B-bar residual p={p} N=5")
    L, ctx, dev, inp, d_J = _open(orc, p, 5, L_EA, L_BBAR)
    d_sig = _up(dev, inp["sig"]); d_y = _up(dev, inp["y0"])
    ctx.check(L.exa_residual_setup(ctx.h, ptr(d_J), ptr(d_sig), None))
    ctx.check(L.exa_residual_apply(ctx.h, ptr(d_y), None))
    y = d_y.cpu().numpy()
    chk.close("B-bar residual onto y0 vs orc_element_vector_bbar", y, _ref(orc, p, 5, "residual_bbar_dense"), onto=inp["y0"])
    chk.close("B-bar residual onto y0 vs orc_add_mult_pa_bbar", y, _ref(orc, p, 5, "residual_bbar_pa"), onto=inp["y0"])
    chk.apart("B-bar residual vs the plain one", y - inp["y0"], _ref(orc, p, 5, "residual") - inp["y0"], 1e-3)
    ctx.close(); chk.record()


@pytest.mark.parametrize("p", ORDERS)
def test_pa_gradient_action_and_diagonal(oracle, p):
    """exa_grad_setup, exa_grad_apply onto y0, exa_grad_diagonal against TransformMatGradTo4D -> AssembleGradPA -> AddMultGradPA and
    AssembleGradDiagonalPA; the action must be that of C, not the assembled matrices' C^T; E = 125"""
    orc = oracle
    chk = _Check(f"PA action and diagonal p={p} N=5")
    L, ctx, dev, inp, d_J = _open(orc, p, 5, L_PA)
    nE = 3 * inp["n"] * inp["E"]
    d_C = _up(dev, inp["Cm"]); d_x = _up(dev, inp["x_e"]); d_y = _up(dev, inp["y0"]); d_d = dev.zeros(nE)
    ctx.check(L.exa_grad_setup(ctx.h, inp["dt"], ptr(d_J), ptr(d_C), None))
    ctx.check(L.exa_grad_apply(ctx.h, ptr(d_x), ptr(d_y), None))
    ctx.check(L.exa_grad_diagonal(ctx.h, ptr(d_d), None))
    y = d_y.cpu().numpy()
    chk.close("PA action onto y0 vs orc_add_mult_grad_pa", y, _ref(orc, p, 5, "pa_action"), onto=inp["y0"])
    chk.close("PA diagonal vs orc_assemble_grad_diag_pa", d_d.cpu().numpy(), _ref(orc, p, 5, "pa_diag"))
    chk.apart("PA action vs the assembled action of the same C", y - inp["y0"], _ref(orc, p, 5, "pa_action_of_Ct") - inp["y0"], 1e-3)
    ctx.close(); chk.record()


@pytest.mark.parametrize("integ", [L_FULL, L_BBAR], ids=["plain", "bbar"])
@pytest.mark.parametrize("p", ORDERS)
def test_element_matrices_action_and_diagonal(oracle, p, integ):
    """k_assemble_ea_rt / k_ea_apply_rt: exa_grad_get_ea, exa_grad_apply onto y0 and exa_grad_diagonal against the oracle's dense matrices.
    p = 6 runs on one element: padded to a 64-lane block its 1029 x 1029 matrix takes 0.54 GB on the device, which the library accepts."""
    orc = oracle
    N = EA_MESH[p]
    what = "ea_bbar" if integ else "ea"
    chk = _Check(f"EA {'B-bar' if integ else 'plain'} p={p} N={N}")
    L, ctx, dev, inp, d_J = _open(orc, p, N, L_EA, integ)
    n, E = inp["n"], inp["E"]; nE = 3 * n * E
    if integ:      # B-bar needs the element-average gradients the residual set-up leaves behind
        d_s0 = _up(dev, inp["sig"])
        ctx.check(L.exa_residual_setup(ctx.h, ptr(d_J), ptr(d_s0), None))
    d_C = _up(dev, inp["Cm"]); d_x = _up(dev, inp["x_e"]); d_y = _up(dev, inp["y0"]); d_d = dev.zeros(nE); d_em = dev.zeros(9 * n * n * E)
    ctx.check(L.exa_grad_setup(ctx.h, inp["dt"], ptr(d_J), ptr(d_C), None))
    ctx.check(L.exa_grad_get_ea(ctx.h, ptr(d_em), None))
    ctx.check(L.exa_grad_apply(ctx.h, ptr(d_x), ptr(d_y), None))
    ctx.check(L.exa_grad_diagonal(ctx.h, ptr(d_d), None))
    chk.close("element matrices vs orc_assemble_ea" + ("_bbar" if integ else ""), d_em.cpu().numpy(), _ref(orc, p, N, what))
    chk.close("EA action onto y0 vs orc_ea_mult", d_y.cpu().numpy(), _ref(orc, p, N, what + "_action"), onto=inp["y0"])
    chk.close("EA diagonal vs orc_ea_diag", d_d.cpu().numpy(), _ref(orc, p, N, what + "_diag"))
    ctx.close(); chk.record()


@pytest.mark.parametrize("p,N,assembly", [(3, 5, L_EA), (3, 5, L_PA), (4, 2, L_EA)], ids=["p3-N5-EA", "p3-N5-PA", "p4-N2-EA"])
def test_lvector_forms(oracle, p, N, assembly):
    """exa_restrict, exa_restrict_transpose_add (atomic and ordered), exa_grad_apply_lvec with and without the mask - or, where the fused
    action is refused, the refusal and the composition restrict -> E-vector action -> transposed add - against l_to_e / e_to_l around
    the oracle's element action"""
    orc = oracle
    chk = _Check(f"L-vector forms p={p} N={N} {'EA' if assembly else 'PA'}")
    L, ctx, dev, inp, d_J = _open(orc, p, N, assembly)
    rve, n, E, NN = inp["rve"], inp["n"], inp["E"], inp["NN"]; nE = 3 * n * E
    o = hipref.HighOrderOracle(orc, inp)
    zero = np.zeros(nE)
    d_conn = dev.up(rve["conn"]); ctx.check(L.exa_set_connectivity(ctx.h, ptr(d_conn), NN))
    d_C = _up(dev, inp["Cm"])
    ctx.check(L.exa_grad_setup(ctx.h, inp["dt"], ptr(d_J), ptr(d_C), None))
    # E <-> L
    d_xL = _up(dev, inp["xL"]); d_e = dev.zeros(nE)
    ctx.check(L.exa_restrict(ctx.h, ptr(d_xL), ptr(d_e), None))
    assert np.array_equal(d_e.cpu().numpy(), hipref.l_to_e(rve, inp["xL"]))
    chk.say("exa_restrict: equal to l_to_e")
    d_ev = _up(dev, inp["x_e"])
    sums = hipref.e_to_l(rve, inp["x_e"])                     # np.add.at visits the elements in ascending order, as the ordered kernel does
    d_yL = _up(dev, inp["yL0"])
    ctx.check(L.exa_restrict_transpose_add(ctx.h, ptr(d_ev), ptr(d_yL), None))
    chk.close("exa_restrict_transpose_add (atomic) onto yL0", d_yL.cpu().numpy(), inp["yL0"] + sums, onto=inp["yL0"])
    ctx.check(L.exa_set_deterministic(ctx.h, 1))
    det = []
    for _ in range(2):
        d_yL = _up(dev, inp["yL0"])
        ctx.check(L.exa_restrict_transpose_add(ctx.h, ptr(d_ev), ptr(d_yL), None))
        det.append(d_yL.cpu().numpy())
    chk.close("exa_restrict_transpose_add (ordered) onto yL0", det[0], inp["yL0"] + sums, onto=inp["yL0"])
    assert np.array_equal(det[0], det[1]) and np.array_equal(det[0], inp["yL0"] + sums)
    chk.say("exa_restrict_transpose_add (ordered): bit-identical on a second call and equal to the ascending-element sum")
    # the fused action is refused in deterministic mode at these orders, whatever the assembly
    d_out = dev.zeros(3 * NN)
    msg = _refused(L, ctx, L.exa_grad_apply_lvec(ctx.h, ptr(d_xL), ptr(d_out), None, None), "deterministic mode", "p = 1")
    chk.say(f"refused: {msg}")
    ctx.check(L.exa_set_deterministic(ctx.h, 0))
    d_mask = _up(dev, inp["mask"])
    for mask in (inp["mask"], None):
        tag = "masked" if mask is not None else "unmasked"
        xin = inp["xL"] if mask is None else np.where(mask, 0.0, inp["xL"])
        xe_in = hipref.l_to_e(rve, xin)
        if assembly == L_EA:
            ye = o.ea_mult(_ref(orc, p, N, "ea"), x=xe_in, y0=zero)
        else:
            ye = o.pa_action(x=xe_in, y0=zero)
        yL_ref = inp["yL0"] + hipref.e_to_l(rve, ye)
        d_yL = _up(dev, inp["yL0"])
        rc = L.exa_grad_apply_lvec(ctx.h, ptr(d_xL), ptr(d_yL), ptr(d_mask) if mask is not None else None, None)
        if assembly == L_EA:
            ctx.check(rc)
            chk.close(f"exa_grad_apply_lvec ({tag}) onto yL0", d_yL.cpu().numpy(), yL_ref, onto=inp["yL0"])
        else:
            msg = _refused(L, ctx, rc, "fused L-vector partial-assembly action", "exa_restrict + exa_grad_apply")
            chk.say(f"refused ({tag}): {msg}")
            assert np.array_equal(d_yL.cpu().numpy(), inp["yL0"])      # nothing written
        # the composition the driver runs at these orders: restrict -> E-vector action -> transposed add, atomic and ordered
        d_xin = _up(dev, xin)
        for ordered in (0, 1):
            ctx.check(L.exa_set_deterministic(ctx.h, ordered))
            d_xe = dev.zeros(nE); d_ye = dev.zeros(nE); d_yL = _up(dev, inp["yL0"])
            ctx.check(L.exa_restrict(ctx.h, ptr(d_xin), ptr(d_xe), None))
            ctx.check(L.exa_grad_apply(ctx.h, ptr(d_xe), ptr(d_ye), None))
            ctx.check(L.exa_restrict_transpose_add(ctx.h, ptr(d_ye), ptr(d_yL), None))
            chk.close(f"restrict -> exa_grad_apply -> transposed add ({tag}, {'ordered' if ordered else 'atomic'})", d_yL.cpu().numpy(), yL_ref, onto=inp["yL0"])
        ctx.check(L.exa_set_deterministic(ctx.h, 0))
    ctx.close(); chk.record()


def test_model_setup_p3_matches_oracle(oracle):
    """the fused constitutive launch at 64 nodes / 64 points per element: three steps elastic -> plastic, FCC Voce, on the warped 2^3
    mesh, with the bounds of test_model_setup_p2_matches_oracle (stress 1e-9, tangent 1e-7)"""
    import exaconstit_amd.lib as L
    orc = oracle
    chk = _Check("constitutive launch p=3 N=2")
    p, N = 3, 2
    inp = hipref.ho_inputs(orc, p, N)
    rve, E, Q, n, P = inp["rve"], inp["E"], inp["Q"], inp["n"], inp["P"]
    props = _props(orc)
    dev = hipref.Dev()
    ctx = L.Context(L.EXA_FCC_VOCE, props, 298.0, p, E)
    quats = hipref.random_quats(E)
    d_state0 = dev.zeros(28 * P)
    d_quats_keep = dev.up(quats.ravel())   # must outlive the asynchronous launch
    ctx.check(L.exa_init_state(ctx.h, ptr(d_state0), ptr(d_quats_keep), None))
    sv0 = d_state0.cpu().numpy().copy(); s0 = np.zeros(6 * P)
    v = hipref.velocity_field(rve, scale=2.0); vel_e = hipref.l_to_e(rve, v); x = np.array(rve["X"])
    for dt in (0.2, 0.3, 0.5):
        x = x + v * dt
        xe = hipref.l_to_e(rve, x)
        J = np.zeros(9 * P); orc.lib().orc_jacobians(p, E, orc._p(xe), orc._p(J))
        s1 = np.zeros(6 * P); sv1 = np.zeros(28 * P); cm = np.zeros(36 * P)
        nf = orc.lib().orc_model_setup(0, 0, orc._p(props), len(props), Q, E, n, 28, C.c_double(dt), C.c_double(298.0), orc._p(J), orc._p(rve["G"]),
                                       orc._p(vel_e), orc._p(s0), orc._p(sv0), orc._p(s1), orc._p(sv1), orc._p(cm), None, 1, 0, 0)
        assert nf == 0
        d = [dev.up(a) for a in (J, vel_e, s0, sv0)]; o = [dev.zeros(6 * P), dev.zeros(28 * P), dev.zeros(36 * P)]
        ctx.check(L.exa_model_setup(ctx.h, dt, *[ptr(t) for t in d], *[ptr(t) for t in o], None))
        assert ctx.check(L.exa_model_status(ctx.h, None)) == 0
        chk.close(f"dt={dt}: stress", o[0].cpu().numpy(), s1, 1e-9)
        chk.close(f"dt={dt}: tangent", o[2].cpu().numpy(), cm, 1e-7)
        s0, sv0 = s1, sv1
    ctx.close(); chk.record()
