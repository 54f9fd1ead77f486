"""Host side of the element-field cases of tests/test_gpu_element_fields.py (oracle and numpy only, no GPU): the reference those cases
compare exa_element_fields with (tests/fieldref.py) must be right, precise enough, and able to fail.  Asserted here, on the reference alone:
  * p = 2 ... 6: the nodes of the oracle's mesh sit on the Gauss-Lobatto positions (roots of P_p' and the end points) to 1e-14, numbered the
    same way in every element; the numpy interpolant's derivative is the oracle's gradient table to 1e-12, its weights the oracle's to 1e-15,
    and its shape values sum to 1 to 1e-14;
  * det J > 0 at every point of every input of the GPU cases, the curved p = 2 tetrahedra included;
  * the float64 reference agrees with the same reference in np.longdouble to a tenth of the GPU bound (fieldref.gpu_bounds turns a larger
    figure into that case's bound);
  * every slip the p = 1 and p = 2 hexahedron cases cannot see moves the reference by >= 1e-6 of column scale: the point weight taken from the
    point with x and z exchanged, equispaced in place of Gauss-Lobatto nodes (p >= 3; exactly 0 at p = 2, where the two coincide),
    tetrahedron weights exchanged between weight classes, an element's point data taken from its neighbour in the block;
  * straight-sided tetrahedra: the volume-weighted centroid is the mean of the four vertices and the volume is tet_mesh_util.tet_volumes.
Every test prints what it measured; EXA_WRITE_RECORDS=1 keeps the lines in profiles/element_field_checks.txt."""
import numpy as np
import pytest

import fieldref as F
import hipref
import tet_mesh_util as T

HEX_CASES = [(3, 5), (4, 2), (5, 2), (6, 2)]                   # the (p, N) of the GPU module
DISCRIMINATE = 1e-6


@pytest.fixture(scope="module")
def L():
    import exaconstit_amd.lib as lib
    return lib


@pytest.fixture(scope="module")
def tet_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("fieldref")


@pytest.mark.parametrize("p", [2, 3, 4, 5, 6])
def test_numpy_tables_are_the_oracle_element(oracle, p):
    ck = F.Check(f"host tables p={p}")
    N = 2
    ijk, dist = F.node_lattice(oracle, N, p)
    ck.say(f"p={p}: largest distance of a mesh node from its Gauss-Lobatto position {dist:.2e} (<= 1e-14)")
    assert dist <= 1e-14
    assert np.all(ijk == ijk[:1])                                # the same numbering in every element
    n = (p + 1) ** 3
    assert len({tuple(r) for r in ijk[0]}) == n                  # every lattice position once
    assert np.array_equal(ijk[0][:8], [[0, 0, 0], [p, 0, 0], [p, p, 0], [0, p, 0], [0, 0, p], [p, 0, p], [p, p, p], [0, p, p]])   # vertices first
    Nv, G, W = F.hex_tables(oracle, N, p)
    rve = hipref.make_rve(oracle, N, p=p)
    dG = np.abs(G - rve["G"].reshape(n, 3, n)).max()
    dW = np.abs(W - rve["W"]).max()
    one = np.abs(Nv.sum(0) - 1).max()
    ck.say(f"p={p}: numpy gradient table vs the oracle's {dG:.2e} (<= 1e-12), weights {dW:.2e} (<= 1e-15), |sum_a N_a - 1| {one:.2e} (<= 1e-14)")
    assert dG <= 1e-12 and dW <= 1e-15 and one <= 1e-14
    ck.record()


@pytest.mark.parametrize("p,N", HEX_CASES)
def test_hexahedron_reference_is_precise_and_can_fail(oracle, p, N):
    ck = F.Check(f"host hexahedra p={p} N={N}")
    c = F.hex_case(oracle, p, N)
    cl = F.hex_case(oracle, p, N, np.longdouble)
    E, Q, np1 = c["E"], c["Q"], p + 1
    w = F.point_weights(c["J"], c["W"])
    det = w / c["W"]
    ck.say(f"p={p} N={N}: E = {E}, Q = {Q}, det J min/max {det.min() / det.max():.4f}, smallest |averaged quaternion| {np.linalg.norm(np.einsum('eq,eqk->ek', w, c['SV'][:, :, 9:13]) / w.sum(1)[:, None], axis=1).min():.3f}")
    assert det.min() > 0
    prec = F.column_errors(c["ref"], cl["ref"])
    ck.say(f"p={p} N={N}: float64 vs longdouble reference, worst column {prec[:31].max():.2e} (<= 1e-14), elastic strain {prec[31:].max():.2e} (<= 1e-13)")
    assert np.all(prec <= F.BASE_BOUND / 10)
    ref = c["ref"]
    # the point weight taken from the point with the x and z indices exchanged
    moved = F.column_errors(F.element_fields_numpy(c["J"], c["S"], c["SV"], c["W"], c["xq"], w=w[:, F.transpose_points(np1)]), ref)
    ck.say(f"p={p} N={N}: weight of the x <-> z transposed point: averaged columns move by {moved[F.AVERAGED].min():.2e} ... {moved[F.AVERAGED].max():.2e}")
    assert moved[F.AVERAGED].min() >= DISCRIMINATE
    # the point at which the geometry is interpolated decoded with x and z exchanged (what a swapped qx, qz in the kernel does)
    moved = F.column_errors(F.element_fields_numpy(c["J"], c["S"], c["SV"], c["W"], c["xq"][:, F.transpose_points(np1)]), ref)
    ck.say(f"p={p} N={N}: geometry interpolated at the x <-> z transposed point: centroid moves by {moved[F.CENTROID].min():.2e} ... {moved[F.CENTROID].max():.2e}")
    assert moved[F.CENTROID].min() >= DISCRIMINATE
    # equispaced nodes in the one-dimensional basis
    Neq, _, _ = F.hex_tables(oracle, N, p, nodes=F.equispaced_nodes(p))
    moved = F.column_errors(F.element_fields_numpy(c["J"], c["S"], c["SV"], c["W"], np.einsum("ean,nq->eqa", c["xe"], Neq)), ref)
    ck.say(f"p={p} N={N}: equispaced in place of Gauss-Lobatto nodes: centroid moves by {moved[F.CENTROID].min():.2e} ... {moved[F.CENTROID].max():.2e}")
    assert moved[F.CENTROID].min() >= DISCRIMINATE
    # an element's point data taken from its neighbour in the block
    moved = F.column_errors(F.element_fields_numpy(c["J"], np.roll(c["S"], 1, 0), np.roll(c["SV"], 1, 0), c["W"], c["xq"]), ref)
    ck.say(f"p={p} N={N}: point data of the neighbouring element: averaged columns move by {moved[F.AVERAGED].min():.2e} ... {moved[F.AVERAGED].max():.2e}")
    assert moved[F.AVERAGED].min() >= DISCRIMINATE
    ck.record()


def test_equispaced_nodes_are_invisible_at_p2(oracle):
    """the reason the p = 3 ... 6 cases exist: at p = 2 the Gauss-Lobatto nodes are 0, 1/2, 1, so a reference (or a kernel) built on equispaced
    nodes gives the same bits there"""
    ck = F.Check("host equispaced p=2")
    assert np.array_equal(F.lobatto_nodes(2), F.equispaced_nodes(2))
    Nl, _, _ = F.hex_tables(oracle, 3, 2)
    Ne, _, _ = F.hex_tables(oracle, 3, 2, nodes=F.equispaced_nodes(2))
    inp = hipref.ho_inputs(oracle, 2, 3)
    xe = inp["xe"].reshape(inp["E"], 3, inp["n"])
    moved = np.abs(np.einsum("ean,nq->eqa", xe, Nl) - np.einsum("ean,nq->eqa", xe, Ne)).max()
    ck.say(f"p=2: equispaced in place of Gauss-Lobatto nodes moves the interpolated geometry by {moved:.1e} (exactly 0)")
    assert moved == 0.0
    for p in (3, 4, 5, 6):
        assert np.abs(F.lobatto_nodes(p) - F.equispaced_nodes(p)).max() > 0.02
    ck.record()


@pytest.mark.parametrize("p,warped", [(1, False), (2, False), (2, True)])
def test_tetrahedron_reference_is_precise_and_can_fail(L, tet_dir, p, warped):
    ck = F.Check(f"host tetrahedra p={p}{' warped' if warped else ''}")
    c = F.tet_case(L, tet_dir, p, warped)
    cl = F.tet_case(L, tet_dir, p, warped, np.longdouble)
    E, Q, n = c["E"], c["Q"], c["n"]
    assert (E, Q, n) == (162, 5 if p == 1 else 14, 4 if p == 1 else 10)
    conn = c["conn"].reshape(E, n)
    Xn = c["X"].reshape(3, c["NN"]).T
    w = F.point_weights(c["J"], c["W"])
    det = w / c["W"]
    spread = (det.max(1) / det.min(1)).max()
    ck.say(f"tet p={p} warped={warped}: E = {E}, Q = {Q}, det J min {det.min():.3e} max {det.max():.3e}, largest max/min inside an element {spread:.6f}")
    assert det.min() > 0
    if warped:                                                   # det J varies inside an element: one det J per element would show
        flat = F.column_errors(F.element_fields_numpy(c["J"], c["S"], c["SV"], c["W"], c["xq"], w=c["W"][None, :] * det[:, :1]), c["ref"])
        ck.say(f"tet p={p} warped={warped}: det J of point 0 at every point: averaged columns move by {flat[F.AVERAGED].min():.2e} ... {flat[F.AVERAGED].max():.2e}, volume by {flat[0]:.2e}")
        assert flat[F.AVERAGED].min() >= DISCRIMINATE and flat[0] >= DISCRIMINATE
    prec = F.column_errors(c["ref"], cl["ref"])
    ck.say(f"tet p={p} warped={warped}: float64 vs longdouble reference, worst column {prec[:31].max():.2e} (<= 1e-14), elastic strain {prec[31:].max():.2e} (<= 1e-13)")
    assert np.all(prec <= F.BASE_BOUND / 10)
    ref = c["ref"]
    # two weights of different weight classes exchanged (p = 1: the negative centroid weight and a vertex-side one; p = 2: one pair per two classes)
    for a, b in ([(0, 1)] if p == 1 else [(0, 6), (6, 10), (0, 10)]):
        assert c["W"][a] != c["W"][b]
        Wx = np.array(c["W"]); Wx[[a, b]] = Wx[[b, a]]
        moved = F.column_errors(F.element_fields_numpy(c["J"], c["S"], c["SV"], Wx, c["xq"]), ref)
        ck.say(f"tet p={p} warped={warped}: weights {a} <-> {b} exchanged: averaged columns move by {moved[F.AVERAGED].min():.2e} ... {moved[F.AVERAGED].max():.2e}")
        assert moved[F.AVERAGED].min() >= DISCRIMINATE
    moved = F.column_errors(F.element_fields_numpy(c["J"], np.roll(c["S"], 1, 0), np.roll(c["SV"], 1, 0), c["W"], c["xq"]), ref)
    ck.say(f"tet p={p} warped={warped}: point data of the neighbouring element: averaged columns move by {moved[F.AVERAGED].min():.2e} ... {moved[F.AVERAGED].max():.2e}")
    assert moved[F.AVERAGED].min() >= DISCRIMINATE
    # a row of the neighbouring element would also show in the volume and the centroid
    vol = T.tet_volumes(Xn, conn[:, :4].astype(np.int64))
    assert np.abs(np.roll(vol, 1) - vol).max() >= 1e-3 * vol.max()
    if not warped:
        if p == 2:                                               # the reader puts the edge nodes at the edge midpoints, in this order
            edges = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
            mid = np.stack([0.5 * (Xn[conn[:, i]] + Xn[conn[:, j]]) for i, j in edges], 1)
            assert np.abs(Xn[conn[:, 4:]] - mid).max() <= 1e-15
        dv = np.abs(ref[:, 0] - vol).max() / vol.max()
        dc = np.abs(ref[:, 1:4] - c["vertex_mean"]).max()
        ck.say(f"tet p={p}: reference volume vs tet_volumes {dv:.2e} (<= 1e-13), volume-weighted centroid vs mean of the vertices {dc:.2e} (<= 1e-13)")
        assert dv <= 1e-13 and dc <= 1e-13
        assert abs(vol.sum() - 1.0) <= 1e-13
    ck.record()
