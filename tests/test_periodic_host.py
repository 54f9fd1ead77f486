"""Periodic boundary conditions, host side (no GPU): the [BCs] periodic = true option with its refusals, and the periodic view of the block
decomposition (Partition::make_periodic): canonical ids, weights, neighbour lists and the table of local groups."""
import ctypes as C
import os
from collections import Counter, defaultdict

import numpy as np
import pytest

import partition_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "refdata")
VGRAD = "[[1.0e-3, 2.0e-4, -1.0e-4], [-3.0e-4, -5.0e-4, 4.0e-4], [5.0e-4, -2.0e-4, -5.0e-4]]"


def _query(tmp_path, text):
    import exaconstit_amd.lib as L
    for fl in ("props_cp_voce.txt", "state_cp_voce.txt", "voce_quats.ori", "grains.txt", "custom_dt.txt"):
        text = text.replace('"%s"' % fl, '"%s"' % os.path.join(REF, fl))
    f = tmp_path / "case.toml"
    f.write_text(text)
    out = np.zeros(20); err = C.create_string_buffer(512)
    rc = L.exa_options_query(str(f).encode(), out.ctypes.data_as(C.POINTER(C.c_double)), err, 512)
    return rc, err.value.decode(), str(f)


def _periodic_text(vgrad=VGRAD, extra=""):
    """voce_ea_cs.toml (generated mesh, velocity-gradient faces) with its [BCs] keys replaced by periodic = true"""
    keep, in_bcs = [], False
    for line in open(os.path.join(REF, "voce_ea_cs.toml")).read().splitlines():
        s = line.strip()
        if s.startswith("["):
            in_bcs = s == "[BCs]"
            keep.append(line)
            if in_bcs:
                keep.append("    periodic = true\n    essential_vel_grad = %s\n%s" % (vgrad, extra))
            continue
        if not in_bcs:
            keep.append(line)
    return "\n".join(keep) + "\n"


def test_periodic_option_parses(tmp_path):
    import exaconstit_amd.lib as L
    rc, msg, path = _query(tmp_path, _periodic_text())
    assert rc == 0, msg
    b = L.options_bcs(path)
    assert b["periodic"] is True and b["vel_grad"].shape == (1, 3, 3)
    assert b["vel_grad"][0, 0, 1] == 2.0e-4 and b["vel_grad"][0, 2, 0] == 5.0e-4      # row by row, non-symmetric
    # empty id arrays are "absent"; vgrad_origin is honoured as before
    rc, msg, path = _query(tmp_path, _periodic_text(extra="    essential_ids = []\n    essential_comps = []\n    essential_vals = []\n    vgrad_origin = [0.5, 0.5, 0.5]\n"))
    assert rc == 0, msg
    # one 3 x 3 per update step with changing_ess_bcs
    rc, msg, path = _query(tmp_path, _periodic_text(vgrad="[%s, %s]" % (VGRAD, VGRAD.replace("1.0e-3", "-1.0e-3")),
                                                    extra="    changing_ess_bcs = true\n    update_steps = [1, 4]\n"))
    assert rc == 0, msg
    b = L.options_bcs(path)
    assert b["periodic"] and b["vel_grad"].shape == (2, 3, 3) and b["vel_grad"][1, 0, 0] == -1.0e-3
    # a file without the key is not periodic
    assert L.options_bcs(os.path.join(REF, "voce_ea_cs.toml"))["periodic"] is False


def test_periodic_option_refusals(tmp_path):
    txt = _periodic_text()
    rc, msg, _ = _query(tmp_path, txt.replace("    essential_vel_grad = %s\n" % VGRAD, ""))
    assert rc == -1 and "BCs.periodic = true needs the macroscopic velocity gradient" in msg
    rc, msg, _ = _query(tmp_path, _periodic_text(vgrad="[[1.0e-3, 0.0, 0.0], [0.0, 0.0, 0.0]]"))
    assert rc == -1 and "3 x 3" in msg
    rc, msg, _ = _query(tmp_path, _periodic_text(extra="    essential_ids = [1, 2]\n    essential_comps = [3, 1]\n"))
    assert rc == -1 and "cannot be both periodic and prescribed" in msg
    rc, msg, _ = _query(tmp_path, _periodic_text(extra="    essential_vals = [0.0, 0.0, 0.0]\n"))
    assert rc == -1 and "cannot be both periodic and prescribed" in msg
    rc, msg, _ = _query(tmp_path, _periodic_text(extra="    changing_ess_bcs = true\n    update_steps = [1, 4]\n"))
    assert rc == -1 and "one 3 x 3 array per update step" in msg
    # file meshes need node matching
    other = txt.replace('type = "auto"', 'type = "other"').replace('floc = "../../data/cube-hex-ro.mesh"', 'floc = "%s"' % os.path.join(REF, "cube5_nodes.mesh")).replace("ref_ser = 1", "ref_ser = 0")
    assert other != txt
    rc, msg, _ = _query(tmp_path, other)
    assert rc == -1 and "periodic" in msg and 'Mesh.type = "auto"' in msg and "node matching" in msg
    # multigrid
    assert "[Solvers.Krylov]" in txt
    rc, msg, _ = _query(tmp_path, txt.replace("[Solvers.Krylov]", '[Solvers.Krylov]\n        preconditioner = "multigrid"').replace("ref_ser = 1", "ref_ser = 0"))
    assert rc == -1 and "periodic" in msg and "multigrid" in msg
    rc, msg, _ = _query(tmp_path, txt.replace("[Solvers.Krylov]", '[Solvers.Krylov]\n        preconditioner = "jacobi"'))
    assert rc == 0, msg


def test_non_periodic_files_are_read_as_before(tmp_path):
    """the reference option files return what test_host_logic.py expects, and the message of a missing essential_ids is unchanged"""
    import exaconstit_amd.lib as L

    def q(name):
        out = np.zeros(20); err = C.create_string_buffer(512)
        return L.exa_options_query(os.path.join(REF, name).encode(), out.ctypes.data_as(C.POINTER(C.c_double)), err, 512), out
    rc, o = q("voce_pa.toml")
    assert rc == 0 and o[0] == 298 and o[1] == 17 and o[7] == 40 and o[13] == 1000 and o[19] == 1
    rc, o = q("voce_full_cyclic.toml")
    assert rc == 0 and o[7] == 70 and o[19] == 5
    assert L.options_bcs(os.path.join(REF, "voce_full_cyclic.toml"))["periodic"] is False
    txt = open(os.path.join(REF, "voce_ea_cs.toml")).read()
    rc, msg, _ = _query(tmp_path, txt.replace("essential_ids", "unused_ids"))
    assert rc == -1 and msg == "BCs.essential_ids / essential_comps are required"
    rc, msg, _ = _query(tmp_path, txt.replace("[BCs]", "[BCs]\n    periodic = false"))
    assert rc == 0, msg


GRIDS = [(6, 5, 4), (4, 4, 4)]
RANKS = [1, 2, 3, 4, 8]


def _canon_of_gid(gid, N, p):
    M = [n * p for n in N]
    i = gid % (M[0] + 1); j = (gid // (M[0] + 1)) % (M[1] + 1); k = gid // ((M[0] + 1) * (M[1] + 1))
    return (i % M[0]) + (M[0] + 1) * ((j % M[1]) + (M[1] + 1) * (k % M[2]))


@pytest.mark.parametrize("N", GRIDS)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("nranks", RANKS)
def test_periodic_partition(N, order, nranks):
    import exaconstit_amd.lib as L
    p = order
    parts = [L.partition_periodic(N, r, nranks, order) for r in range(nranks)]
    gids = [L.partition_nodes(N, r, nranks, order)[0] for r in range(nranks)]
    M = [n * p for n in N]
    # canonical id = global node index with index N p mapped to 0 in every direction
    for r in range(nranks):
        assert parts[r]["NN"] == len(gids[r])
        assert np.array_equal(parts[r]["canon"], _canon_of_gid(gids[r], N, p))
    # weights: every canonical id counts once over all its (rank, local node) holders
    wsum, holders = defaultdict(float), defaultdict(list)
    for r in range(nranks):
        for g, (c, w) in enumerate(zip(parts[r]["canon"].tolist(), parts[r]["weight"].tolist())):
            wsum[c] += w
            holders[c].append((r, g))
    assert len(wsum) == M[0] * M[1] * M[2]
    assert all(abs(v - 1.0) < 1e-14 for v in wsum.values())
    for c, h in holders.items():
        for (r, g) in h:
            assert parts[r]["weight"][g] == 1.0 / len(h)
    # group sizes over the whole mesh: distinct nodes per canonical id = face interiors 2, edges 4, corners 8
    nodes_of = defaultdict(set)
    for r in range(nranks):
        for c, g in zip(parts[r]["canon"].tolist(), gids[r].tolist()):
            nodes_of[c].add(g)
    sizes = Counter(len(v) for v in nodes_of.values())
    faces = (M[0] - 1) * (M[1] - 1) + (M[1] - 1) * (M[2] - 1) + (M[0] - 1) * (M[2] - 1)
    edges = (M[0] - 1) + (M[1] - 1) + (M[2] - 1)
    assert sizes == Counter({1: (M[0] - 1) * (M[1] - 1) * (M[2] - 1), 2: faces, 4: edges, 8: 1})
    # local group table: exactly the canonical ids with >= 2 local images, members ascending (representative first), ordered by size then id
    for r in range(nranks):
        local = defaultdict(list)
        for g, c in enumerate(parts[r]["canon"].tolist()):
            local[c].append(g)
        want = sorted((len(v), c, v) for c, v in local.items() if len(v) >= 2)
        got = [(len(m), int(parts[r]["canon"][m[0]]), m.tolist()) for m in parts[r]["groups"]]
        assert got == want
        assert parts[r]["group_sizes"] == {s: sum(1 for w in want if w[0] == s) for s in (2, 4, 8)}
        for m in parts[r]["groups"]:
            assert len(set(parts[r]["canon"][m].tolist())) == 1
    if nranks == 1:
        assert parts[0]["group_sizes"] == {2: faces, 4: edges, 8: 1} and not parts[0]["nbrs"]
    # neighbour lists: one entry per pair of ranks, at most 26, symmetric, equal length, the same canonical dofs in the same order on both
    # sides (component by component, ascending canonical id), a rank's entry for an id is its representative
    for r in range(nranks):
        P = parts[r]
        ranks = [r2 for (r2, _) in P["nbrs"]]
        assert len(ranks) == len(set(ranks)) and r not in ranks and len(ranks) <= 26
        rep = {}
        for g, c in enumerate(P["canon"].tolist()):
            rep.setdefault(c, g)
        for (r2, dofs) in P["nbrs"]:
            Q = parts[r2]
            back = [d for (rr, d) in Q["nbrs"] if rr == r]
            assert len(back) == 1 and len(back[0]) == len(dofs)
            mine = [(int(P["canon"][d % P["NN"]]), d // P["NN"]) for d in dofs]
            theirs = [(int(Q["canon"][d % Q["NN"]]), d // Q["NN"]) for d in back[0]]
            assert mine == theirs
            assert mine == sorted(mine, key=lambda t: (t[1], t[0])) and len(set(mine)) == len(mine)
            assert all(rep[c] == d % P["NN"] for (c, _), d in zip(mine, dofs))
            # ... and it is every canonical id the two ranks both hold
            common = set(P["canon"].tolist()) & set(Q["canon"].tolist())
            assert {c for (c, k) in mine if k == 0} == common and len(mine) == 3 * len(common)
    # coverage: every canonical id with more than one holder is reachable through the local groups and the neighbour lists
    for c, h in holders.items():
        if len(h) < 2:
            continue
        hr = sorted({r for (r, _) in h})
        for r in hr:
            P = parts[r]
            nloc = sum(1 for (rr, _) in h if rr == r)
            if nloc >= 2:
                assert any(int(P["canon"][m[0]]) == c and len(m) == nloc for m in P["groups"])
            for r2 in hr:
                if r2 != r:
                    dofs = [d for (rr, d) in P["nbrs"] if rr == r2][0]
                    assert c in set(P["canon"][dofs[:len(dofs) // 3]].tolist())


@pytest.mark.parametrize("nranks,order", [(1, 1), (2, 1), (3, 1), (8, 1), (4, 2)])
def test_non_periodic_partition_unchanged(nranks, order):
    """the plain decomposition is what it was - weights 1 / ranks holding the node, neighbour lists without wrap-around relations - also after
    a periodic query, which differs from it on the box surface only"""
    import exaconstit_amd.lib as L
    N = (6, 5, 4)
    per = [L.partition_periodic(N, r, nranks, order) for r in range(nranks)]
    parts = [pu.query(N, r, nranks, order) for r in range(nranks)]
    nn_glob = (N[0] * order + 1) * (N[1] * order + 1) * (N[2] * order + 1)
    count = np.zeros(nn_glob)
    for q in parts:
        np.add.at(count, pu.global_node_ids(q, N), 1.0)
    for r, q in enumerate(parts):
        g = pu.global_node_ids(q, N)
        assert np.array_equal(q["weight"], 1.0 / count[g])
        surf = np.any((np.abs(q["X"]) < 1e-12) | (np.abs(q["X"] - 1.0) < 1e-12), axis=0)
        assert np.array_equal(per[r]["weight"][~surf], q["weight"][~surf]) and np.all(per[r]["weight"][surf] < q["weight"][surf])
        pg, rc = q["pg"], (r % q["pg"][0], (r // q["pg"][0]) % q["pg"][1], r // (q["pg"][0] * q["pg"][1]))
        want = []
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    o = (dx, dy, dz)
                    r2 = [rc[d] + o[d] for d in range(3)]
                    if o != (0, 0, 0) and all(0 <= r2[d] < pg[d] for d in range(3)):
                        want.append(r2[0] + pg[0] * (r2[1] + pg[1] * r2[2]))
        assert [rr for (rr, _) in q["nbrs"]] == want                 # no wrap-around neighbours
        for (r2, dofs) in q["nbrs"]:                                 # shared nodes are the same nodes
            assert set(g[dofs % q["NN"]].tolist()) <= set(pu.global_node_ids(parts[r2], N).tolist())
