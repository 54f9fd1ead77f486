"""Worker of tests/test_gpu_rccl.py: runs a regression case on the stand-alone driver with the RCCL transport and writes the averaged
stresses and solver history as JSON.  world = 1: EXA_FORCE_RCCL=1 makes the one-rank communicator run every RCCL call (comm init,
all-reduce, grouped send/recv with an empty neighbour list).  world > 1 (torchrun, one rank per GPU): the real multi-rank path.
Usage: python rccl_worker.py <case.toml> <nsteps> <out.json> [jacobi]
       python rccl_worker.py probe <out prefix>      the transport on its own (tests/test_gpu_comm.py): every rank runs Driver.comm_probe on the generated
                                                     2 x 2 x 2 mesh - all-reduces of PROBE_SIZES doubles, one halo sum - and writes <out prefix>.<rank>.json"""
import ctypes as C
import json
import os
import sys

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PROBE_SIZES = (32, 33, 70)     # on and across the 32-double pieces long reductions take through the shared-device transport


def run_probe(L, rank, world, uid, out):
    import numpy as np
    import partition_util as pu
    N = (2, 2, 2)
    props = np.loadtxt(os.path.join(ROOT, "tests", "golden", "refdata", "props_cp_voce.txt")).ravel()
    quats = np.tile([1.0, 0.0, 0.0, 0.0], 8)
    d = L.Driver.synthetic(2, props, quats, np.array([0.005]), rank=rank, nranks=world, uid=uid)
    comm_ranks, transport = d.comm_info()
    red = {f"{n}:{what}": d.comm_probe(what, pu.probe_reduce_input(rank, n)).tolist() for n in PROBE_SIZES for what in (0, 1, 2)}
    gid = pu.probe_node_ids(d.nodal_field("coords_ref"), N)
    halo = d.comm_probe(3, pu.probe_halo_input(rank, gid))
    with open(f"{out}.{rank}.json", "w") as f:
        json.dump(dict(world=world, comm_ranks=comm_ranks, transport=transport, reductions=red, gid=gid.tolist(), halo=halo.tolist()), f)
    d.close()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def main():
    probe = sys.argv[1] == "probe"
    toml, nsteps, out = (None, 0, sys.argv[2]) if probe else (sys.argv[1], int(sys.argv[2]), sys.argv[3])
    jacobi = len(sys.argv) > 4 and sys.argv[4] == "jacobi"
    import torch
    import exaconstit_amd.lib as L
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1")); local = int(os.environ.get("LOCAL_RANK", "0"))
    ndev = torch.cuda.device_count()
    shared = world > ndev                 # more ranks than devices: RCCL (and torch's nccl backend) refuse two ranks on one device
    torch.cuda.set_device(local % ndev)
    uid = None
    if world > 1:
        import torch.distributed as dist
        if shared:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        buf = (C.c_ubyte * 128)()
        if rank == 0:
            assert L.exa_comm_unique_id(buf, world) == 0      # a RCCL id, or the id of the shared-device inter-process transport
        t = torch.tensor(list(buf), dtype=torch.uint8, device="cpu" if shared else "cuda")
        dist.broadcast(t, 0)
        uid = (C.c_ubyte * 128)(*t.cpu().tolist())
    if probe:
        return run_probe(L, rank, world, uid, out)
    d = L.Driver.from_toml(toml, out_dir=os.path.dirname(out), rank=rank, nranks=world, uid=uid, jacobi=jacobi, write_files=False)
    ok = True
    for ti in range(1, nsteps + 1):
        ok = ok and d.step(ti)
    s = d.avgs(0, 6)
    newton, krylov, calls = d.stats()
    comm_ranks, transport = d.comm_info()
    if rank == 0:
        with open(out, "w") as f:
            json.dump(dict(ok=bool(ok), world=world, comm_ranks=comm_ranks, transport=transport, forced=bool(os.environ.get("EXA_FORCE_RCCL")), avg_stress=s.tolist(), comm=d.comm_details(),
                           newton=[int(x) for x in newton], krylov=[int(x) for x in krylov]), f)
    d.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
