"""Host side of tests/test_gpu_high_order_operators.py (oracle only, no GPU): the inputs those tests feed the run-time-order kernels
(p = 3 ... 6) must be able to fail.  Asserted here, on the oracle alone:
  * the warped meshes (hipref.warp_nodes) are valid and distorted: det J > 0, det J max/min >= 1.03, and every point has an off-diagonal
    Jacobian entry of at least 5 % of its largest entry, for every (p, N) the GPU module uses;
  * every index slip the reference's own unit-test inputs hide moves the oracle's output by rel-L2 >= 1e-6, a million times the GPU bound:
    C -> C^T (partial-assembly action, and assembled matrices + action), J -> J^T per point (action, diagonal, residual), two shear
    components of sigma swapped, a normal and a shear component swapped, B-bar against plain (residual and matrices), element-average
    gradients with unit weights instead of W;
  * the identity the flavour check of the GPU module rests on: the oracle's assembled action of C is its partial-assembly action of C^T
    (the assembled matrices hold B^T C B by columns and the mat-vec sums over rows), to 1e-13 at p = 3, 4, 5.
Every test prints what it measured."""
import numpy as np
import pytest

import hipref
from hipref import rel_l2

MESHES = [(3, 5), (4, 5), (5, 5), (6, 5), (3, 2), (4, 2), (5, 2), (6, 1), (5, 1), (5, 3), (6, 3)]       # every (p, N) of the GPU module and of this one
DISCRIMINATE = 1e-6


def _swap(sig, a, b):
    s = np.array(sig).reshape(-1, 6)
    s[:, [a, b]] = s[:, [b, a]]
    return s.ravel()


@pytest.mark.parametrize("p,N", MESHES)
def test_warped_mesh_is_valid_and_distorted(oracle, p, N):
    inp = hipref.ho_inputs(oracle, p, N)
    J = inp["J"].reshape(-1, 3, 3)
    det = np.linalg.det(J)
    amax = np.abs(J).max(axis=(1, 2))
    off = np.abs(J * (1.0 - np.eye(3))).max(axis=(1, 2))
    print(f"p={p} N={N}: det J min/mean {det.min() / det.mean():.4f} max/mean {det.max() / det.mean():.4f} max/min {det.max() / det.min():.4f}, "
          f"smallest off-diagonal share {np.min(off / amax):.3f}")
    assert det.min() > 0
    assert det.max() / det.min() >= 1.03
    assert np.all(off >= 0.05 * amax)


@pytest.mark.parametrize("p,N", [(3, 5), (4, 5), (5, 3), (6, 3)])
def test_point_data_mutations_move_the_oracle(oracle, p, N):
    """the mutations of the point data, on the mesh of the GPU cases at p = 3, 4 and on 27 elements of it above (a dozen references each)"""
    inp = hipref.ho_inputs(oracle, p, N)
    ref = hipref.HighOrderOracle(oracle, inp)
    zero = np.zeros(3 * inp["n"] * inp["E"])
    CmT = hipref.transpose_points(inp["Cm"], 6)
    JT = hipref.transpose_points(inp["J"], 3)
    y = ref.pa_action(y0=zero)
    d = ref.pa_diag()
    r = ref.residual(y0=zero)
    rb = ref.residual_bbar() - inp["y0"]
    eds_unit = ref.eds(W=np.ones(inp["Q"]))
    moved = {
        "C -> C^T, PA action": rel_l2(ref.pa_action(Cm=CmT, y0=zero), y),
        "J -> J^T, PA action": rel_l2(ref.pa_action(J=JT, y0=zero), y),
        "J -> J^T, PA diagonal": rel_l2(ref.pa_diag(J=JT), d),
        "J -> J^T, residual": rel_l2(ref.residual(J=JT, y0=zero), r),
        "sigma shear 3 <-> 4, residual": rel_l2(ref.residual(sig=_swap(inp["sig"], 3, 4), y0=zero), r),
        "sigma shear 4 <-> 5, residual": rel_l2(ref.residual(sig=_swap(inp["sig"], 4, 5), y0=zero), r),
        "sigma normal 0 <-> shear 3, residual": rel_l2(ref.residual(sig=_swap(inp["sig"], 0, 3), y0=zero), r),
        "sigma normal 0 <-> 1, residual": rel_l2(ref.residual(sig=_swap(inp["sig"], 0, 1), y0=zero), r),
        "sigma shear 3 <-> 4, B-bar residual": rel_l2(ref.residual_bbar(sig=_swap(inp["sig"], 3, 4)) - inp["y0"], rb),
        "B-bar vs plain, residual": rel_l2(r, rb),
        "eDS with unit weights": rel_l2(eds_unit, inp["eDS"]),
        "eDS with unit weights, B-bar residual": rel_l2(ref.residual_bbar(eDS=eds_unit) - inp["y0"], rb),
    }
    for k, v in moved.items():
        print(f"p={p} N={N}: {k}: {v:.3e}")
    for k, v in moved.items():
        assert v >= DISCRIMINATE, k
    # the two statements of the B-bar residual agree with each other
    assert rel_l2(ref.residual_bbar(dense=False), ref.residual_bbar(dense=True)) < 1e-13


@pytest.mark.parametrize("p,N", [(3, 2), (4, 2), (5, 1)])
def test_assembled_action_is_the_transposed_tangent_action(oracle, p, N):
    """oracle EA(C) == oracle PA(C^T) <= 1e-13; EA(C) against PA(C), EA(C) against EA(C^T) and B-bar against plain matrices all move"""
    inp = hipref.ho_inputs(oracle, p, N)      # (one element at p = 5: its 648 x 648 matrix takes a third of a second, eight take 2.7 s)
    ref = hipref.HighOrderOracle(oracle, inp)
    zero = np.zeros(3 * inp["n"] * inp["E"])
    CmT = hipref.transpose_points(inp["Cm"], 6)
    emat = ref.ea()
    y_ea = ref.ea_mult(emat, y0=zero)
    ident = rel_l2(y_ea, ref.pa_action(Cm=CmT, y0=zero))
    flav = rel_l2(y_ea, ref.pa_action(y0=zero))
    ematT = ref.ea(Cm=CmT)
    mat = rel_l2(ematT, emat)
    act = rel_l2(ref.ea_mult(ematT, y0=zero), y_ea)
    bbar = rel_l2(ref.ea(bbar=True), emat)
    print(f"p={p} N={N}: EA(C) vs PA(C^T) {ident:.3e}; EA(C) vs PA(C) {flav:.3e}; EA(C^T) vs EA(C) matrices {mat:.3e} action {act:.3e}; "
          f"B-bar vs plain matrices {bbar:.3e}")
    assert ident <= 1e-13
    assert min(flav, mat, act, bbar) >= DISCRIMINATE
    # the matrices of C^T are the transposed matrices of C
    nd = 3 * inp["n"]
    assert rel_l2(ematT.reshape(inp["E"], nd, nd).transpose(0, 2, 1), emat.reshape(inp["E"], nd, nd)) <= 1e-13
