"""Comm (host/comm.hip) on its own, through Driver.comm_probe: the all-reduces and the halo sum of every transport a one-GPU box can run, without
a solve around them.
  * eight in-process loopback ranks on the generated 2 x 2 x 2 mesh at p = 1: one element per rank, seven neighbours each, the centre node held by
    all eight ranks (it lies in several segments of every rank);
  * two processes over the shared-device transport: reductions on and across its 32-double pieces, one halo sum;
  * one rank with EXA_FORCE_RCCL=1: the RCCL calls on a one-rank communicator.
Inputs are small integers (tests/partition_util.py), so every sum is exact in any order and the results are compared with equality."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import partition_util as pu

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N = (2, 2, 2)
REDUCE_SIZES = (1, 32, 33, 70)
PROBE_SIZES = (32, 33, 70)     # what the probe mode of tests/rccl_worker.py reduces
NUMPY_OP = (np.sum, np.min, np.max)


def _loopback_probe(nranks, body):
    """body(driver, rank) on `nranks` loopback drivers of the 2 x 2 x 2 mesh, one host thread each; returns the list of its results"""
    import exaconstit_amd.lib as L
    props = np.loadtxt(os.path.join(HERE, "golden", "refdata", "props_cp_voce.txt")).ravel()
    quats = np.tile([1.0, 0.0, 0.0, 0.0], 8)
    gid = (C.c_ubyte * 128)()
    assert L.exa_loopback_group_create(nranks, gid) == 0
    out, drivers, errors = [None] * nranks, [None] * nranks, []

    def work(r):
        try:
            drivers[r] = L.Driver.synthetic(2, props, quats, np.array([0.005]), rank=r, nranks=nranks, uid=gid)
            out[r] = body(drivers[r], r)
        except Exception as e:   # noqa: BLE001
            errors.append((r, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    assert not errors, errors
    assert all(not t.is_alive() for t in th), "a rank hung"
    for d in drivers:
        d.close()
    L.exa_loopback_group_destroy(gid)
    return out


def _halo(d, r):
    gid = pu.probe_node_ids(d.nodal_field("coords_ref"), N)
    return d.comm_info(), d.comm_details()["neighbours"], gid, d.comm_probe(3, pu.probe_halo_input(r, gid))


@pytest.mark.parametrize("env", [{}, {"EXA_DETERMINISTIC": "1"}, {"EXA_LOOPBACK_SYNC": "1"}], ids=["default", "deterministic", "loopback_sync"])
def test_loopback_halo_sum_eight_ranks(monkeypatch, env):
    """Case A: the halo sum gives, at every local node, the sum over the ranks that hold it - in one atomic unpack pass (default), segment by segment
    (EXA_DETERMINISTIC=1) and with the host-synchronous exchange (EXA_LOOPBACK_SYNC=1)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    res = _loopback_probe(8, _halo)
    centre = 1 + 3 * (1 + 3 * 1)
    for r, (info, nbrs, gid, got) in enumerate(res):
        assert info == (8, "loopback") and nbrs == 7 and gid.size == 8 and centre in gid
        assert np.array_equal(got, pu.probe_halo_expected(N, 8, gid)), f"rank {r}"


def test_loopback_reductions_eight_ranks():
    """Case B: sum, min and max over the eight ranks, n in REDUCE_SIZES"""
    res = _loopback_probe(8, lambda d, r: {(n, what): d.comm_probe(what, pu.probe_reduce_input(r, n)) for n in REDUCE_SIZES for what in (0, 1, 2)})
    for n in REDUCE_SIZES:
        rows = np.array([pu.probe_reduce_input(r, n) for r in range(8)])
        for what in (0, 1, 2):
            for r in range(8):
                assert np.array_equal(res[r][(n, what)], NUMPY_OP[what](rows, axis=0)), f"n = {n}, op {what}, rank {r}"


def _probe_worker(tmp_path, tag, nproc, env_extra=None, port=29581):
    out = os.path.join(str(tmp_path), tag)
    env = dict(os.environ); env.update(env_extra or {}); env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    args = [os.path.join(HERE, "rccl_worker.py"), "probe", out]
    cmd = [sys.executable] + args if nproc == 1 else [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
                                                      "--master-addr", "127.0.0.1", "--master-port", str(port)] + args
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return [json.load(open(f"{out}.{k}.json")) for k in range(nproc)]


def test_two_processes_probe(tmp_path):
    """Case C: two processes.  On a one-GPU box they share the device and talk through the shared-device transport, whose reductions pass through
    32-double slots piece by piece: n = 32, 33 and 70 are one piece, two and three.  With two GPUs the same launch runs over RCCL."""
    import torch
    res = _probe_worker(tmp_path, "two", 2)
    for r, d in enumerate(res):
        assert d["world"] == 2 and d["comm_ranks"] == 2 and d["transport"] == ("rccl" if torch.cuda.device_count() >= 2 else "ipc")
        for n in PROBE_SIZES:
            rows = np.array([pu.probe_reduce_input(k, n) for k in range(2)])
            for what in (0, 1, 2):
                assert np.array_equal(np.array(d["reductions"][f"{n}:{what}"]), NUMPY_OP[what](rows, axis=0)), f"n = {n}, op {what}, rank {r}"
        gid = np.array(d["gid"])
        assert gid.size == 18 and np.array_equal(np.array(d["halo"]), pu.probe_halo_expected(N, 2, gid)), f"rank {r}"


def test_forced_rccl_probe_one_rank(tmp_path):
    """Case D: EXA_FORCE_RCCL=1 on one rank - the sum of 33 doubles over the one-rank communicator returns its input; kind 1 (rccl), one rank"""
    d = _probe_worker(tmp_path, "forced", 1, {"EXA_FORCE_RCCL": "1"})[0]
    assert d["transport"] == "rccl" and d["comm_ranks"] == 1 and d["world"] == 1
    assert np.array_equal(np.array(d["reductions"]["33:0"]), pu.probe_reduce_input(0, 33))
