"""What a live driver reports about its route equals what the host-only query (exa_operator_routes_query, csrc/host/routes.hpp) predicts for the same
facts and environment: the action route of mesh_info, the overlap flag of comm_details, record launches exactly when the row says records, and a
slip-rate launch after reading a slip-rate component exactly when the row says the record launches leave a lean state.  One step at 2^3 elements."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

import test_gpu_tetrahedra as TT
import tet_mesh_util as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "refdata")
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import route_table as RT   # noqa: E402


@pytest.fixture(autouse=True)
def _plain_environment(monkeypatch):
    for k in RT.VARIABLES + RT.RETIRED:
        monkeypatch.delenv(k, raising=False)


def _check(L, d, f):
    """the driver d has taken a step; f: its facts apart from the partition's, which comm_details supplies"""
    cd = d.comm_details()
    f = f[:7] + [int(cd["boundary_block_elements"] > 0), int(cd["neighbours"] > 0), 0]
    row = RT.query(L, f, {k: os.environ[k] for k in RT.VARIABLES if k in os.environ})
    assert L.ACTION_ROUTES.index(d.mesh_info()["action_route"]) == row["action_route"], row
    dg = d.diagnostics()
    # (the two counters are those of the element-blocked p = 1 record launches, exa_model_record_launches; the p = 2 record launches show in the
    #  slip-rate launch below, which only a record launch can make necessary)
    assert (dg["record_policy_launches"] + dg["record_generic_launches"] > 0) == bool(row["records_setup"] and row["fast_p1"] and row["qlayout_eb64"]), (dg, row)
    # (a record launch leaves a lean state when the switch is on and the layout is element-blocked: exa_get_lean_state)
    lean = bool(row["lean_state"] and row["records_setup"] and row["qlayout_eb64"])
    d.qf_component(0, 14)
    assert (d.diagnostics()["slip_rate_launches"] > 0) == lean, (d.diagnostics(), row)
    return cd, row


CASES = {"hex_p1_pa": dict(order=1, assembly=0, bbar=False), "hex_p1_ea": dict(order=1, assembly=1, bbar=False), "hex_p2_pa": dict(order=2, assembly=0, bbar=False),
         "hex_p2_ea_bbar": dict(order=2, assembly=1, bbar=True), "hex_p1_pa_deterministic": dict(order=1, assembly=0, bbar=False)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_synthetic_driver_reports_the_predicted_route(monkeypatch, case):
    import exaconstit_amd.lib as L
    if case.endswith("deterministic"):
        monkeypatch.setenv("EXA_DETERMINISTIC", "1")
    c = CASES[case]; N = 2
    props = np.loadtxt(os.path.join(REF, "props_cp_voce.txt")).ravel()
    q = np.random.default_rng(7).standard_normal((N ** 3, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    d = L.Driver.synthetic(N, props, q.ravel(), np.array([0.005]), **c)
    assert d.step(1)
    cd, row = _check(L, d, RT.facts("hex", c["order"], int(c["bbar"]), c["assembly"], 0, "one"))
    assert cd["halo_overlap"] == bool(row["overlap_wish"]) and not cd["halo_overlap"]
    d.close()


def test_tetrahedral_driver_reports_the_predicted_route(tmp_path):
    import exaconstit_amd.lib as L
    mesh = T.write_mfem(str(tmp_path / "k.mesh"), T.kuhn_cube(2, perturb=0.2, shuffle=True, seed=3))
    d = TT._steps(L, TT._toml(tmp_path, "tet1", mesh=mesh, p=1), 1, tmp_path)
    cd, row = _check(L, d, RT.facts("tet", 1, 0, 0, 0, "one"))
    assert row["action_route"] == 1 and cd["halo_overlap"] == bool(row["overlap_wish"])
    d.close()


@pytest.mark.parametrize("overlap", ["default", "off"])
def test_two_ranks_agree_on_the_predicted_overlap(tmp_path, monkeypatch, overlap):
    """4 x 2 x 2 elements on two loopback ranks: the flag every rank reports is the agreement of the ranks' predicted wishes"""
    import exaconstit_amd.lib as L
    if overlap == "off":
        monkeypatch.setenv("EXA_HALO_OVERLAP", "off")
    path = TT._toml(tmp_path, "two", N=4)
    txt = open(path).read()
    assert "ncuts = [4, 4, 4]" in txt
    with open(path, "w") as fh:
        fh.write(txt.replace("ncuts = [4, 4, 4]", "ncuts = [4, 2, 2]"))
    gid = (C.c_ubyte * 128)()
    assert L.exa_loopback_group_create(2, gid) == 0
    drivers = [None, None]; errors = []

    def work(r):
        try:
            drivers[r] = L.Driver.from_toml(path, out_dir=str(tmp_path), rank=r, nranks=2, uid=gid, write_files=False)
            assert drivers[r].step(1)
        except BaseException as e:   # noqa: BLE001
            errors.append((r, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    assert all(not t.is_alive() for t in th), "a rank hung"
    assert not errors, errors
    got = [_check(L, d, RT.facts("hex", 1, 0, 0, 0, "several")) for d in drivers]   # (the query sets the environment: one thread)
    for d in drivers:
        d.close()
    L.exa_loopback_group_destroy(gid)
    agreed = all(row["overlap_wish"] for _, row in got)
    assert agreed == (overlap == "default")
    for cd, _ in got:
        assert cd["boundary_block_elements"] > 0 and cd["halo_overlap"] == agreed
