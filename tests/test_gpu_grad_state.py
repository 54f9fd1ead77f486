"""Transitions of the library's gradient data (include/exaconstit_hip.h): which record sets exist after which set-up, who builds the missing
ones, and which calls are refused.  The forms themselves are pinned to the oracle in test_gpu_parity.py; here two contexts that got the same
inputs are compared with each other.

Bounds: the diagonal and the E-vector action read the 46-double records without atomics, and those records come from the same kernel on the
same inputs whether exa_grad_setup writes them or the first consumer does: same bits.  Two forms of the L-vector action (atomic scatter)
agree to rel-L2 < 1e-13, the bound of test_gpu_parity.py::test_compact_tangent_form.
"""
import numpy as np
import pytest

import hipref
from hipref import rel_l2, ptr

pytestmark = pytest.mark.gpu

DT = 0.5
FORMS_BOUND = 1e-13
_cache = {}


def _ctx(L, t, form, assembly=0, matrix_free=False):
    ctx = L.Context(0, t["props"], 298.0, 1, t["E"], assembly=assembly)
    ctx.check(L.exa_set_quadrature_layout(ctx.h, t["layout"])); ctx.check(L.exa_set_connectivity(ctx.h, ptr(t["conn"]), t["NN"]))
    if matrix_free: ctx.check(L.exa_set_ea_matrix_free(ctx.h, 1))
    ctx.check(L.exa_set_tangent_form(ctx.h, form))
    return ctx


def _tangents(orc, layout):
    """One exa_model_setup_lvec launch (model 0, dt = 0.5) on the distorted 5^3 mesh: E = 125, two 64-element blocks, the second partial.
    Computed once per layout and left unchanged."""
    if layout in _cache: return _cache[layout]
    import torch
    import exaconstit_amd.lib as L
    dev = hipref.Dev()
    rve = hipref.make_rve(orc, 5, distort=0.15)
    E, NN = rve["E"], rve["NN"]
    t = dict(dev=dev, rve=rve, E=E, NN=NN, n=rve["n"], layout=layout, props=np.loadtxt(orc.REFDATA + "/props_cp_voce.txt").ravel(),
             conn=torch.from_numpy(rve["conn"].astype(np.int32)).to(dev.dev))
    ctx = _ctx(L, t, L.EXA_TANGENT_FULL)
    sz = lambda w: int(L.exa_qf_size(ctx.h, w))
    t["sz"] = {w: sz(w) for w in (6, 9, 28, 36)}
    v = hipref.velocity_field(rve, scale=2.0)
    t["v"] = dev.up(v); t["x"] = dev.up(rve["X"] + DT * v)
    t["sv0"] = dev.zeros(sz(28)); t["s0"] = dev.zeros(sz(6))
    d_q = dev.up(hipref.random_quats(E).ravel())
    ctx.check(L.exa_init_state(ctx.h, ptr(t["sv0"]), ptr(d_q), None))
    t["cm"] = dev.zeros(sz(36)); t["J"] = dev.zeros(sz(9)); s1 = dev.zeros(sz(6)); sv1 = dev.zeros(sz(28))
    ctx.check(L.exa_model_setup_lvec(ctx.h, DT, ptr(t["x"]), ptr(t["v"]), ptr(t["s0"]), ptr(t["sv0"]), ptr(s1), ptr(sv1), ptr(t["cm"]), ptr(t["J"]), None))
    assert ctx.check(L.exa_model_status(ctx.h, None)) == 0
    ctx.close()
    rng = np.random.default_rng(2)
    t["xl"] = dev.up(rng.standard_normal(3 * NN)); t["xe"] = dev.up(rng.standard_normal(3 * t["n"] * E))
    t["mask"] = torch.zeros(3 * NN, dtype=torch.uint8, device=dev.dev)
    _cache[layout] = t
    return t


def _lvec(L, ctx, t, coords):
    ctx.check(L.exa_grad_set_coords(ctx.h, ptr(t["x"]) if coords else None))
    y = t["dev"].zeros(3 * t["NN"]); ctx.check(L.exa_grad_apply_lvec(ctx.h, ptr(t["xl"]), ptr(y), ptr(t["mask"]), None))
    return y.cpu().numpy()


def _diag(L, ctx, t):
    d = t["dev"].zeros(3 * t["n"] * t["E"]); ctx.check(L.exa_grad_diagonal(ctx.h, ptr(d), None))
    return d.cpu().numpy()


def _evec(L, ctx, t):
    y = t["dev"].zeros(3 * t["n"] * t["E"]); ctx.check(L.exa_grad_apply(ctx.h, ptr(t["xe"]), ptr(y), None))
    return y.cpu().numpy()


CALLS = {"diag": _diag, "evec": _evec, "lvec": lambda L, c, t: _lvec(L, c, t, False), "lvec_coords": lambda L, c, t: _lvec(L, c, t, True)}
ORDERS = {"diagonal_first": ("diag", "evec", "lvec", "lvec_coords"), "lvec_coords_first": ("lvec_coords", "diag", "evec", "lvec")}


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("layout", [0, 1], ids=["aos", "eb64"])
def test_records_built_on_demand(oracle, layout, order):
    """A set-up in compact form writes the compact records alone; the diagonal, the E-vector action and the L-vector action without coordinates get the
    46-double records from the first of them that runs, built from the arrays of the set-up: same results as a context in the full form, in either
    call order, and again after a second set-up with other data (a pending mark or a remembered input that is not renewed would show there)."""
    import exaconstit_amd.lib as L
    t = _tangents(oracle, layout)
    a = _ctx(L, t, L.EXA_TANGENT_FULL); b = _ctx(L, t, L.EXA_TANGENT_DEV5_BULK)
    dt2, scale = 0.2, 1.7
    cm2 = t["cm"] * scale
    first = None
    for dt, cm in ((DT, t["cm"]), (dt2, cm2)):
        for c in (a, b): c.check(L.exa_grad_setup(c.h, dt, ptr(t["J"]), ptr(cm), None))
        ra = {k: CALLS[k](L, a, t) for k in ORDERS["diagonal_first"]}
        rb = {k: CALLS[k](L, b, t) for k in ORDERS[order]}
        for k in ("diag", "evec"):
            print(layout, order, dt, k, "rel_l2", rel_l2(rb[k], ra[k]), "equal bits", np.array_equal(rb[k], ra[k]))
            assert np.linalg.norm(ra[k]) > 0 and np.array_equal(rb[k], ra[k]), (k, dt)
        for k in ("lvec", "lvec_coords"):
            print(layout, order, dt, k, "rel_l2", rel_l2(rb[k], ra[k]))
            assert np.linalg.norm(ra[k]) > 0 and rel_l2(rb[k], ra[k]) < FORMS_BOUND, (k, dt)
        if first is None: first = ra
        else:      # the action is linear in dt C: the second set-up's data, not the first's
            for k in ra: assert rel_l2(ra[k], (dt2 * scale / DT) * first[k]) < FORMS_BOUND, k
    a.close(); b.close()


def _refused(L, ctx, rc):
    """EXA_ERR_STATE, with a message of this call's own"""
    return rc == L.EXA_ERR_STATE and L.exa_last_error(ctx.h) not in (b"", SENTINEL)


SENTINEL = b"exa_set_quadrature_layout: bad argument"


def _mark(L, ctx):
    assert L.exa_set_quadrature_layout(ctx.h, 5) == L.EXA_ERR_ARG and L.exa_last_error(ctx.h) == SENTINEL


def test_records_of_the_constitutive_launch(oracle):
    """After exa_model_setup_lvec_records the gradient data are the compact records alone: the consumers of the 46-double records and of the element
    matrices refuse, the L-vector action needs the coordinates and then equals the action of a context set up from the tangent field."""
    import exaconstit_amd.lib as L
    t = _tangents(oracle, L.EXA_QLAYOUT_EB64)
    dev, sz = t["dev"], t["sz"]
    nE = 3 * t["n"] * t["E"]

    def records(ctx):
        s1 = dev.zeros(sz[6]); sv1 = dev.zeros(sz[28]); J = dev.zeros(sz[9])
        ctx.check(L.exa_model_setup_lvec_records(ctx.h, DT, ptr(t["x"]), ptr(t["v"]), ptr(t["s0"]), ptr(t["sv0"]), ptr(s1), ptr(sv1), ptr(J), None))
        assert ctx.check(L.exa_model_status(ctx.h, None)) == 0

    r = _ctx(L, t, L.EXA_TANGENT_DEV5_BULK)
    records(r)
    y = dev.zeros(3 * t["NN"]); ye = dev.zeros(nE)
    _mark(L, r); assert _refused(L, r, L.exa_grad_apply(r.h, ptr(t["xe"]), ptr(ye), None))
    _mark(L, r); assert _refused(L, r, L.exa_grad_diagonal(r.h, ptr(ye), None))
    _mark(L, r); assert _refused(L, r, L.exa_grad_apply_lvec(r.h, ptr(t["xl"]), ptr(y), ptr(t["mask"]), None))      # no coordinates named
    assert not y.any() and not ye.any()
    s = _ctx(L, t, L.EXA_TANGENT_DEV5_BULK)
    s.check(L.exa_grad_setup(s.h, DT, ptr(t["J"]), ptr(t["cm"]), None))
    yr, ys = _lvec(L, r, t, True), _lvec(L, s, t, True)
    print("records of the launch against records of the set-up: rel_l2", rel_l2(yr, ys))
    assert np.linalg.norm(ys) > 0 and rel_l2(yr, ys) < FORMS_BOUND
    r.check(L.exa_grad_setup(r.h, DT, ptr(t["J"]), ptr(t["cm"]), None))      # the full records again
    assert np.array_equal(_evec(L, r, t), _evec(L, s, t))
    r.close(); s.close()
    # element assembly, matrix-free: no element matrices to hand out either
    m = _ctx(L, t, L.EXA_TANGENT_DEV5_BULK, assembly=L.EXA_ASSEMBLY_EA, matrix_free=True)
    records(m)
    emat = dev.zeros(9 * t["n"] * t["n"] * t["E"])
    _mark(L, m); assert _refused(L, m, L.exa_grad_get_ea(m.h, ptr(emat), None))
    m.close()


def test_forgetting(oracle):
    """exa_set_tangent_form, when it drops compact records of another shape, and exa_set_quadrature_layout forget the gradient data: the next action is
    refused until exa_grad_setup.  (Selecting a compact form on a context that holds no compact records drops nothing: the action stays legal.)"""
    import exaconstit_amd.lib as L
    t = _tangents(oracle, L.EXA_QLAYOUT_EB64)
    dev = t["dev"]
    c = _ctx(L, t, L.EXA_TANGENT_DEV5_BULK)
    setup = lambda: c.check(L.exa_grad_setup(c.h, DT, ptr(t["J"]), ptr(t["cm"]), None))
    apply = lambda: L.exa_grad_apply_lvec(c.h, ptr(t["xl"]), ptr(dev.zeros(3 * t["NN"])), ptr(t["mask"]), None)
    setup(); c.check(L.exa_grad_set_coords(c.h, ptr(t["x"])))
    assert apply() == L.EXA_OK
    c.check(L.exa_set_tangent_form(c.h, L.EXA_TANGENT_DEV5_BULK)); assert apply() == L.EXA_OK      # same form: nothing dropped
    c.check(L.exa_set_tangent_form(c.h, L.EXA_TANGENT_FULL))
    _mark(L, c); assert _refused(L, c, apply()) and _refused(L, c, L.exa_grad_diagonal(c.h, ptr(dev.zeros(3 * t["n"] * t["E"])), None))
    setup(); y_full = _lvec(L, c, t, True)
    c.check(L.exa_set_tangent_form(c.h, L.EXA_TANGENT_DEV5_BULK)); assert apply() == L.EXA_OK      # no compact records to drop
    setup(); assert rel_l2(_lvec(L, c, t, True), y_full) < FORMS_BOUND
    c.check(L.exa_set_quadrature_layout(c.h, L.EXA_QLAYOUT_EB64))
    _mark(L, c); assert _refused(L, c, apply())
    setup(); assert rel_l2(_lvec(L, c, t, True), y_full) < FORMS_BOUND
    c.close()
