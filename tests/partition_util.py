"""Python view of the driver's block decomposition (exa_partition_query) for the CPU tests."""
import ctypes as C

import numpy as np


def query(N, rank, nranks, order=1):
    import exaconstit_amd.lib as L
    Nc = (C.c_int * 3)(*N)
    info = (C.c_int64 * 8)()
    info[7] = order
    L.exa_partition_query(Nc, rank, nranks, info, None, None, None, None, None, None, None)
    E, NN, nnb, shared, n = info[0], info[1], info[2], info[6], info[7]
    conn = np.zeros(n * E, np.int32); X = np.zeros(3 * NN); gid = np.zeros(E, np.int64); w = np.zeros(NN)
    nr = np.zeros(max(nnb, 1), np.int32); nc = np.zeros(max(nnb, 1), np.int32); nd = np.zeros(max(shared, 1), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    info[7] = order
    L.exa_partition_query(Nc, rank, nranks, info, vp(conn), vp(X), vp(gid), vp(w), vp(nr), vp(nc), vp(nd))
    nbrs = []
    off = 0
    for i in range(nnb):
        nbrs.append((int(nr[i]), nd[off:off + nc[i]].copy()))
        off += nc[i]
    return dict(E=E, NN=NN, pg=(info[3], info[4], info[5]), conn=conn.reshape(E, n), order=order, X=X.reshape(3, NN), gid=gid, weight=w, nbrs=nbrs)


def global_node_ids(part, N):
    """global lexicographic node id of every local node, from its coordinates on the unit cube"""
    X = part["X"]
    p = part.get("order", 1)
    i = np.rint(X[0] * N[0] * p).astype(np.int64); j = np.rint(X[1] * N[1] * p).astype(np.int64); k = np.rint(X[2] * N[2] * p).astype(np.int64)
    return i + (N[0] * p + 1) * (j + (N[1] * p + 1) * k)


# ---- inputs and expected values of the transport probe (Driver.comm_probe; tests/test_gpu_comm.py and the probe mode of tests/rccl_worker.py) ----
def probe_reduce_input(rank, n):
    """integer-valued doubles that differ by rank and position: their sums, minima and maxima over the ranks are exact in any order"""
    i = np.arange(n)
    return ((7 * rank + 3 * i) % 11 - 5 + rank).astype(np.float64)


def probe_node_ids(coords_ref, N):
    """global lexicographic node id of a p = 1 driver's local nodes, from Driver.nodal_field("coords_ref") on the unit cube"""
    return global_node_ids(dict(X=np.asarray(coords_ref).T), N)


def probe_halo_input(rank, gid):
    """L-vector (dof = node + local nodes * component) of small integers that depend on the rank, the global node id and the component"""
    return np.concatenate([(rank + 1) * (gid + 1) + 100 * c for c in range(3)]).astype(np.float64)


def probe_halo_expected(N, nranks, gid):
    """the halo sum of probe_halo_input at the nodes `gid`: at every node the sum over the ranks that hold it (block decomposition of exa_partition_query)"""
    tot = np.zeros((3, (N[0] + 1) * (N[1] + 1) * (N[2] + 1)))
    for r in range(nranks):
        g = global_node_ids(query(N, r, nranks), N)
        tot[:, g] += probe_halo_input(r, g).reshape(3, -1)
    return tot[:, gid].ravel()
