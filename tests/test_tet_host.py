"""Tetrahedra on the host: reference-element tables, mesh readers and the option checks - no GPU needed."""
import ctypes as C
import itertools
import math
import os

import numpy as np
import pytest

import tet_mesh_util as T


@pytest.fixture(scope="module")
def L():
    import exaconstit_amd.lib as lib
    return lib


@pytest.mark.parametrize("p,n,Q", [(1, 4, 5), (2, 10, 14)])
def test_tet_tables(L, p, n, Q):
    G, W, N = L.ref_elem_tables(L.EXA_GEOM_TET, p)
    assert G.size == n * 3 * Q and W.size == Q and N.size == n * Q
    assert abs(W.sum() - 1.0 / 6.0) < 1e-15
    if p == 1:
        assert W.min() < 0   # the Strang-Fix rule the reference runs keeps its negative centroid weight
    # quadrature points from the shape values of the vertices' coordinates (x = N_1 + edge terms ..., exact for the linear map)
    Nq = N.reshape(Q, n)
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], float)
    nodes = verts if p == 1 else np.vstack([verts] + [(verts[i] + verts[j]) / 2 for i, j in itertools.combinations(range(4), 2)])
    xq = Nq @ nodes
    for a, b, c in itertools.product(range(2 * p + 2), repeat=3):
        if a + b + c > 2 * p + 1:
            continue
        exact = math.factorial(a) * math.factorial(b) * math.factorial(c) / math.factorial(a + b + c + 3)
        got = np.sum(W * xq[:, 0] ** a * xq[:, 1] ** b * xq[:, 2] ** c)
        assert abs(got - exact) < 1e-14, (a, b, c)
    assert np.abs(Nq.sum(axis=1) - 1).max() < 1e-14                   # partition of unity
    Gq = G.reshape(Q, 3, n)
    assert np.abs(Gq.sum(axis=2)).max() < 1e-14                       # sum_a grad N_a = 0
    # nodal: N_a evaluated at the nodes through the exact quadratic (or linear) interpolation of the basis
    Gr, Wr, Nr = T.ref_tables_numpy(p)
    assert np.abs(G - Gr).max() < 1e-14 and np.abs(W - Wr).max() < 1e-15 and np.abs(N - Nr).max() < 1e-14
    # nodality: the basis reproduces x, y, z and, at p = 2, x^2 exactly at the points (x = sum_a N_a x_a)
    for k in range(3):
        assert np.abs(Nq @ nodes[:, k] - xq[:, k]).max() < 1e-15
    if p == 2:
        assert np.abs(Nq @ nodes[:, 0] ** 2 - xq[:, 0] ** 2).max() < 1e-14
        assert np.abs(Nq @ (nodes[:, 0] * nodes[:, 1]) - xq[:, 0] * xq[:, 1]).max() < 1e-14


@pytest.mark.parametrize("p", [1, 2, 3])
def test_hex_tables_unchanged(L, oracle, p):
    G, W, N = L.ref_elem_tables(L.EXA_GEOM_HEX, p)
    orc = oracle
    n = (p + 1) ** 3
    Gr, Wr = np.zeros(n * 3 * n), np.zeros(n)
    orc.lib().orc_ref_elem(p, orc._p(Gr), orc._p(Wr))
    assert np.abs(G - Gr).max() < 1e-13 and np.abs(W - Wr).max() < 1e-15   # (the oracle builds its tables on its own)
    assert np.abs(N.reshape(n, n).sum(axis=1) - 1).max() < 1e-13


def test_tables_refuse_bad_orders(L):
    assert L.exa_ref_elem_tables(L.EXA_GEOM_TET, 3, None, None, None) == L.EXA_ERR_ARG
    assert L.exa_ref_elem_tables(7, 1, None, None, None) == L.EXA_ERR_ARG


def test_bbar_tet_context_refused_before_device(L):
    props = np.loadtxt(os.path.join(T.REFDATA, "props_cp_voce.txt")).ravel()
    cfg = L.ExaConfig(L.EXA_FCC_VOCE, len(props), props.ctypes.data_as(C.POINTER(C.c_double)), 298.0, 1, 10, L.EXA_ASSEMBLY_EA, L.EXA_INTEG_BBAR, -1)
    err = C.c_int(0)
    assert not L.exa_create_geom(C.byref(cfg), L.EXA_GEOM_TET, C.byref(err))
    assert err.value == L.EXA_ERR_UNSUPPORTED
    cfg.integ = L.EXA_INTEG_FULL; cfg.order = 3
    assert not L.exa_create_geom(C.byref(cfg), L.EXA_GEOM_TET, C.byref(err))
    assert err.value == L.EXA_ERR_UNSUPPORTED


def _query(L, path, order=1, nranks=1, rank=0):
    info = (C.c_int64 * 8)(); err = C.create_string_buffer(512)
    rc = L._lib.exa_mesh_partition_query_order(path.encode(), rank, nranks, order, info, None, None, None, None, None, None, None, err, 512)
    return rc, list(info), err.value.decode()


@pytest.mark.parametrize("fmt", ["mfem", "mfem_nodes", "gmsh"])
def test_tet_reader(L, tmp_path, fmt):
    m = T.kuhn_cube(3, perturb=0.2, shuffle=True, seed=3)
    path = str(tmp_path / ("m.msh" if fmt == "gmsh" else "m.mesh"))
    (T.write_gmsh if fmt == "gmsh" else T.write_mfem)(path, m, **({"nodes_gf": True} if fmt == "mfem_nodes" else {}))
    rc, info, err = _query(L, path)
    assert rc == 0, err
    assert info[0] == 162 and info[1] == 64 and info[7] == 4
    rc, info, err = _query(L, path, order=2)
    assert rc == 0, err
    assert info[7] == 10 and info[1] == 64 + len({tuple(sorted(e)) for t in m["tets"] for e in itertools.combinations(t, 2)})
    rc, info, err = _query(L, path, nranks=3, rank=1)
    assert rc == 0, err
    assert 0 < info[0] < 162


def test_tet_reader_errors(L, tmp_path):
    m = T.kuhn_cube(2, seed=1)
    # inverted element
    bad = dict(m); bad["tets"] = m["tets"].copy(); bad["tets"][5, [2, 3]] = bad["tets"][5, [3, 2]]
    rc, _, err = _query(L, T.write_mfem(str(tmp_path / "inv.mesh"), bad))
    assert rc != 0 and "tetrahedron 5" in err and "volume" in err
    # mixed hexahedra and tetrahedra
    path = T.write_mfem(str(tmp_path / "mix.mesh"), m)
    txt = open(path).read().replace("1 4 ", "1 5 0 1 2 3 ", 1)
    open(path, "w").write(txt)
    rc, _, err = _query(L, path)
    assert rc != 0 and "mixes" in err
    # second-order Gmsh tetrahedron
    path = T.write_gmsh(str(tmp_path / "o2.msh"), m)
    lines = open(path).read().split("\n")
    k = next(i for i, s in enumerate(lines) if s.split()[1:2] == ["4"])
    parts = lines[k].split(); parts[1] = "11"; lines[k] = " ".join(parts + parts[-6:])
    open(path, "w").write("\n".join(lines))
    rc, _, err = _query(L, path)
    assert rc != 0 and "second-order" in err
    # p_refinement = 3 on tetrahedra
    rc, _, err = _query(L, T.write_mfem(str(tmp_path / "ok.mesh"), m), order=3)
    assert rc != 0 and "p_refinement = 1 or 2" in err


def test_kuhn_util_volumes():
    m = T.kuhn_cube(4, perturb=0.25, shuffle=True, seed=2)
    v = T.tet_volumes(m["X"], m["tets"])
    assert v.min() > 0 and abs(v.sum() - 1.0) < 1e-13
    assert sorted(set(m["tri_attr"].tolist())) == [1, 2, 3, 4, 5, 6] and len(m["tris"]) == 6 * 2 * 16
