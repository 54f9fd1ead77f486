"""Wall time of a small solve on eight in-process loopback ranks (one host thread each, one device): the generated 32^3 mesh, 16^3 elements per rank, FCC
Voce, two time steps of the full Newton / PCG loop.  Every PCG iteration runs one halo exchange and one host-synchronous all-reduce through the loopback
group, so the line shows what the host code of the transport (host/comm.hip) costs; it is NOT a performance path (bench.py --gpus N is).
Prints one JSON line: build id, seconds for the two steps (slowest rank), PCG iterations, iterations per second.
    python scripts/comm_loopback_bench.py [--root CHECKOUT] [--n 32]"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--n", type=int, default=32)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import numpy as np
    import exaconstit_amd.lib as L
    import hipref
    nranks = 8
    props = np.loadtxt(os.path.join(root, "tests", "golden", "refdata", "props_cp_voce.txt")).ravel()
    quats = hipref.random_quats(a.n ** 3).ravel()
    dts = np.array([0.005, 0.195])
    gid = (C.c_ubyte * 128)()
    assert L.exa_loopback_group_create(nranks, gid) == 0
    res, errors = [None] * nranks, []
    start = threading.Barrier(nranks)

    def work(r):
        try:
            d = L.Driver.synthetic(a.n, props, quats, dts, rank=r, nranks=nranks, uid=gid)
            start.wait()
            t0 = time.perf_counter()
            for ti in (1, 2):
                assert d.step(ti), (r, ti)
            dt = time.perf_counter() - t0
            res[r] = (dt, int(sum(d.stats()[1])), d.comm_details()["halo_overlap"])
            d.close()
        except Exception as e:   # noqa: BLE001
            errors.append((r, repr(e)))
            start.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
    [t.start() for t in th]
    [t.join(timeout=300) for t in th]
    L.exa_loopback_group_destroy(gid)
    if errors or any(r is None for r in res):
        print(json.dumps(dict(ok=False, errors=errors)))
        return 1
    sec = max(r[0] for r in res)
    print(json.dumps(dict(ok=True, build_id=L.exa_build_id().decode(), ranks=nranks, n=a.n, seconds=round(sec, 4), pcg_iters=res[0][1],
                          pcg_iters_per_s=round(res[0][1] / sec, 1), halo_overlap=res[0][2])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
