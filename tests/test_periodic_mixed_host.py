"""Mixed stress / velocity-gradient loading of a periodic cell, host side (no GPU): the [BCs] periodic_free mask with its refusals,
and the tables Partition::make_periodic(mixed) adds - top-face node lists, control nodes, offset codes, weights."""
import ctypes as C
import os
from collections import defaultdict

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "refdata")
VGRAD = "[[-4.0e-4, 0.0, 0.0], [0.0, -4.0e-4, 0.0], [0.0, 0.0, 1.0e-3]]"
UNIAXIAL = "[[1, 0, 0], [0, 1, 0], [0, 0, 0]]"


def _query(tmp_path, text):
    import exaconstit_amd.lib as L
    for fl in ("props_cp_voce.txt", "state_cp_voce.txt", "voce_quats.ori", "grains.txt", "custom_dt.txt"):
        text = text.replace('"%s"' % fl, '"%s"' % os.path.join(REF, fl))
    f = tmp_path / "case.toml"
    f.write_text(text)
    out = np.zeros(20); err = C.create_string_buffer(512)
    rc = L.exa_options_query(str(f).encode(), out.ctypes.data_as(C.POINTER(C.c_double)), err, 512)
    return rc, err.value.decode(), str(f), out


def _text(free=UNIAXIAL, periodic=True, extra=""):
    """voce_ea_cs.toml (generated mesh) with its [BCs] keys replaced by the periodic ones (the pattern of tests/test_periodic_host.py)"""
    keep, in_bcs = [], False
    for line in open(os.path.join(REF, "voce_ea_cs.toml")).read().splitlines():
        s = line.strip()
        if s.startswith("["):
            in_bcs = s == "[BCs]"
            keep.append(line)
            if in_bcs:
                keep.append("    periodic = %s\n    essential_vel_grad = %s\n" % ("true" if periodic else "false", VGRAD)
                            + ("    periodic_free = %s\n" % free if free is not None else "") + extra)
            continue
        if not in_bcs:
            keep.append(line)
    return "\n".join(keep) + "\n"


def test_valid_masks_parse(tmp_path):
    import exaconstit_amd.lib as L
    rc, msg, path, _ = _query(tmp_path, _text())
    assert rc == 0, msg
    pf = L.options_periodic_free(path)
    assert pf["mixed"] and np.array_equal(pf["free"], np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0]], bool))
    b = L.options_bcs(path)
    assert b["periodic"] and b["vel_grad"][0, 2, 2] == 1.0e-3 and b["vel_grad"][0, 0, 0] == -4.0e-4      # the guess stays in the gradient
    # booleans; one of an off-diagonal pair (simple shear with a free normal would be [[0,0,0],[0,1,0],[0,0,0]])
    rc, msg, path, _ = _query(tmp_path, _text(free="[[false, true, false], [false, true, false], [false, false, false]]"))
    assert rc == 0, msg
    assert np.array_equal(L.options_periodic_free(path)["free"], np.array([[0, 1, 0], [0, 1, 0], [0, 0, 0]], bool))
    # an all-zero mask is the fully prescribed periodic run
    rc, msg, path, _ = _query(tmp_path, _text(free="[[0, 0, 0], [0, 0, 0], [0, 0, 0]]"))
    assert rc == 0, msg
    assert not L.options_periodic_free(path)["mixed"]
    # jacobi stays legal
    rc, msg, _, _ = _query(tmp_path, _text().replace("[Solvers.Krylov]", '[Solvers.Krylov]\n        preconditioner = "jacobi"'))
    assert rc == 0, msg


def test_refusals(tmp_path):
    rc, msg, _, _ = _query(tmp_path, _text(free="[[1, 1, 0], [1, 0, 0], [0, 0, 0]]"))
    assert rc == -1 and "off-diagonal pair" in msg and "rotation" in msg
    rc, msg, _, _ = _query(tmp_path, _text(free="[[0, 0, 1], [0, 0, 0], [1, 0, 0]]"))
    assert rc == -1 and "off-diagonal pair" in msg
    rc, msg, _, _ = _query(tmp_path, _text(free="[[1, 1, 1], [1, 1, 1], [1, 1, 1]]"))
    assert rc == -1 and "all nine entries are free" in msg
    rc, msg, _, _ = _query(tmp_path, _text(periodic=False).replace("    essential_vel_grad = %s\n" % VGRAD, "    essential_ids = [1]\n    essential_comps = [3]\n    essential_vals = [0.0, 0.0, 0.0]\n"))
    assert rc == -1 and "periodic_free needs BCs.periodic = true" in msg
    txt = _text()
    rc, msg, _, _ = _query(tmp_path, txt.replace("[Solvers.Krylov]", '[Solvers.Krylov]\n        preconditioner = "multigrid"').replace("ref_ser = 1", "ref_ser = 0"))
    assert rc == -1 and "periodic" in msg and "multigrid" in msg
    for bad in ("[[1, 0, 0], [0, 1, 0]]", "[[1, 0], [0, 1], [0, 0]]", "[1, 0, 0, 0, 1, 0, 0, 0, 0]", "[[2, 0, 0], [0, 1, 0], [0, 0, 0]]",
                '[["x", 0, 0], [0, 1, 0], [0, 0, 0]]', "1", "[[0.5, 0, 0], [0, 1, 0], [0, 0, 0]]"):
        rc, msg, _, _ = _query(tmp_path, _text(free=bad))
        assert rc == -1 and "3 x 3 array of 0 / 1" in msg, (bad, msg)


def test_a_file_without_the_key_reads_as_before(tmp_path):
    import exaconstit_amd.lib as L
    rc, msg, path, with_zero = _query(tmp_path, _text(free="[[0, 0, 0], [0, 0, 0], [0, 0, 0]]"))
    assert rc == 0, msg
    rc, msg, path, without = _query(tmp_path, _text(free=None))
    assert rc == 0, msg
    assert np.array_equal(with_zero, without)
    pf = L.options_periodic_free(path)
    assert not pf["mixed"] and not pf["free"].any()
    b = L.options_bcs(path)
    assert b["periodic"] and b["vel_grad"].shape == (1, 3, 3)
    for name in ("voce_pa.toml", "voce_full_cyclic.toml", "voce_ea_cs.toml"):
        pf = L.options_periodic_free(os.path.join(REF, name))
        assert not pf["mixed"] and not pf["free"].any()
        assert not L.options_bcs(os.path.join(REF, name))["periodic"]
    # the plain periodic partition is what it was: the corners are a group of eight again
    import exaconstit_amd.lib as L2
    assert L2.partition_periodic(4, 0, 1)["group_sizes"] == {2: 27, 4: 9, 8: 1}


GRIDS = [(6, 5, 4), (4, 4, 4)]
RANKS = [1, 2, 3, 4, 8]


def _grid_index(N, rank, nranks, order):
    """global grid index (3,) of every local node of a rank, from the partition's own node numbering"""
    import exaconstit_amd.lib as L
    gid = np.asarray(L.partition_nodes(N, rank, nranks, order)[0], dtype=np.int64)
    M = [n * order + 1 for n in N]
    return np.stack([gid % M[0], (gid // M[0]) % M[1], gid // (M[0] * M[1])], axis=1)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("nranks", RANKS)
@pytest.mark.parametrize("N", GRIDS)
def test_mixed_partition_tables(N, nranks, order):
    import exaconstit_amd.lib as L
    M = [n * order for n in N]
    face_union = [set() for _ in range(3)]
    ctrl_holders = [0, 0, 0, 0]
    wsum = defaultdict(float)      # reduced unknown -> sum of the weights of its copies
    for r in range(nranks):
        t = L.partition_periodic_mixed(N, r, nranks, order)
        plain = L.partition_periodic(N, r, nranks, order)
        gi = _grid_index(N, r, nranks, order)
        assert gi.shape == (t["NN"], 3)
        top = gi == np.array(M)
        corner = np.all((gi == 0) | top, axis=1)
        # every top-face node of this rank is in its list of that direction exactly once, nothing else is
        for d in range(3):
            lst = t["faces"][d]
            assert len(set(lst.tolist())) == len(lst)
            assert sorted(lst.tolist()) == np.nonzero(top[:, d])[0].tolist()
            for g in lst:
                face_union[d].add(tuple(np.delete(gi[g], d)))
        # offset codes: the grid-index test, bit 3 on the corners; one entry per node that sits on any top face
        code = top[:, 0] * 1 + top[:, 1] * 2 + top[:, 2] * 4
        assert sorted(t["img_nodes"].tolist()) == np.nonzero(code)[0].tolist()
        assert np.array_equal(t["img_code"] & 7, code[t["img_nodes"]])
        assert np.array_equal((t["img_code"] & 8) != 0, corner[t["img_nodes"]])
        # control nodes: c_0 at the origin, c_d one period along d
        want = [(0, 0, 0), (M[0], 0, 0), (0, M[1], 0), (0, 0, M[2])]
        for k in range(4):
            hit = np.nonzero(np.all(gi == np.array(want[k]), axis=1))[0]
            assert t["ctrl"][k] == (hit[0] if len(hit) else -1)
            ctrl_holders[k] += len(hit)
        # the corners are in no group and in no exchange list; everything else is the plain periodic partition
        assert not np.any(corner[t["nbr_dofs"] % t["NN"]])
        assert np.array_equal(t["canon"], plain["canon"])
        assert np.array_equal(t["weight"][~corner], plain["weight"][~corner])
        assert t["groups"] == len(plain["groups"]) - (1 if any(corner[g[0]] for g in plain["groups"]) else 0)
        for g in range(t["NN"]):
            if corner[g]:
                k = [i for i in range(4) if tuple(gi[g]) == want[i]]
                wsum[("c0",) if not k or k[0] == 0 else ("H", k[0])] += t["weight"][g]
            else:
                wsum[("node", int(t["canon"][g]))] += t["weight"][g]
    for d in range(3):
        others = [M[e] + 1 for e in range(3) if e != d]
        assert len(face_union[d]) == others[0] * others[1]      # the whole (N p + 1)^2 grid face
    assert ctrl_holders == [1, 1, 1, 1]
    # every reduced unknown counts once in a dot product: the group values, the pinned corner value, the three control nodes (three entries each)
    assert len(wsum) == M[0] * M[1] * M[2] - 1 + 1 + 3
    assert all(abs(v - 1.0) < 1e-14 for v in wsum.values()), {k: v for k, v in wsum.items() if abs(v - 1.0) >= 1e-14}
