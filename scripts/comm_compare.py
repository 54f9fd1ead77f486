"""One small multi-rank run into a given directory: the case two builds of the library are compared on (same files, same checkpoint, same kernels) when
the host code of the transports (host/comm.hip) changes.
  loopback (default): voce_pa on the golden mesh, 5 steps, eight in-process loopback ranks (one host thread each), EXA_DETERMINISTIC=1, rank 0 writes the
                      output files, every rank takes part in the checkpoint after the last step
  --forced-rccl:      the same case on one rank with EXA_FORCE_RCCL=1, EXA_HALO_SELFTEST=1 and EXA_HALO_OVERLAP=on: the rank exchanges a face with itself
                      over RCCL on the communication stream, between the all-reduces of the PCG
  --root: the checkout whose package is loaded (default: the one this script lies in); the case files come from the same checkout
Two runs are the same when `diff -r -x time -x '*.toml'` of their directories is empty (time_solve.* hold wall times, the .toml names its checkout) -
and, each under `rocprofv3 --kernel-trace --stats` in a run of its own, when kernel names and call counts agree.
Prints one JSON line: build id, ranks, transport, average stress of the last step, Newton and Krylov counts.
    python scripts/comm_compare.py OUT_DIR [--forced-rccl] [--root CHECKOUT]"""
import argparse
import ctypes as C
import json
import os
import sys
import threading

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSTEPS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--forced-rccl", action="store_true")
    ap.add_argument("--root", default=HERE)
    a = ap.parse_args()
    if a.forced_rccl:
        os.environ.update(EXA_FORCE_RCCL="1", EXA_HALO_SELFTEST="1", EXA_HALO_OVERLAP="on")
    else:
        os.environ["EXA_DETERMINISTIC"] = "1"
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import exaconstit_amd.lib as L
    from test_gpu_driver import _variant_toml
    out = os.path.abspath(a.out_dir)
    os.makedirs(out, exist_ok=True)
    toml = _variant_toml(out, "voce_pa.toml", [], "case")
    nranks = 1 if a.forced_rccl else 8
    gid = (C.c_ubyte * 128)()
    if nranks > 1:
        assert L.exa_loopback_group_create(nranks, gid) == 0
    res, errors = [None] * nranks, []

    def work(r):
        try:
            d = L.Driver.from_toml(toml, out_dir=out, rank=r, nranks=nranks, uid=gid if nranks > 1 else None, write_files=(r == 0), restart="")
            for ti in range(1, NSTEPS + 1):
                assert d.step(ti), (r, ti)
            d.save_checkpoint(os.path.join(out, "final.ckpt"))
            newton, krylov, _ = d.stats()
            res[r] = dict(comm=d.comm_info(), avg_stress=d.avgs(0, 6)[-1].tolist(), newton=[int(x) for x in newton], krylov=[int(x) for x in krylov])
            d.close()
        except Exception as e:   # noqa: BLE001
            errors.append((r, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
    [t.start() for t in th]
    [t.join(timeout=600) for t in th]
    if nranks > 1:
        L.exa_loopback_group_destroy(gid)
    ok = not errors and all(r is not None and r == res[0] for r in res)
    print(json.dumps(dict(build_id=L.exa_build_id().decode(), library=L.LIB_PATH, ranks=nranks, ok=ok, errors=errors, rank0=res[0],
                          files=sum(len(f) for _, _, f in os.walk(out)))))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
