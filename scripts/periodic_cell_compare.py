"""One small periodic run into a given directory: the case two builds of the library are compared on (same files, same tangent rows, same checkpoint,
same kernels) when the host code of the periodic cell (host/periodic.hip, host/mixed_loading.hpp, the step code of host/driver.hip) changes.
  the case:  generated 4^3 hexahedral mesh, p = 1, Voce FCC, one grain per element, EXA_DETERMINISTIC=1, periodic with the uniaxial free mask of
             tests/test_gpu_periodic_mixed.py (xx and yy free), 4 steps, the prescribed L changes at step 3 (PeriodicBCChange and the swap of the
             affine part in MixedStepStart), Visualizations.macro_tangent on (a row per step), one checkpoint after the last step
  --ranks:   1 (every image group local: sizes 2, 4, 8), 2 (local groups and cross-rank images), 8 (no local group: the fluctuation route and the
             owner-bits pass do the work); in-process loopback ranks, one host thread each.  File output is on for every rank (the tangent evaluation
             behind Visualizations.macro_tangent is collective and runs where file output is on); the library lets rank 0 write
  --no-mask: every entry of L prescribed (plain periodic conditions)
  --root:    the checkout whose package is loaded (default: the one this script lies in)
Two runs are the same when `diff -r -x time -x 'time_solve*' -x '*.toml'` of their directories is empty - and, each under `rocprofv3 --kernel-trace --stats`
in a run of its own, when kernel names and call counts agree.  Prints one JSON line: build id, ranks, average stress of the last step, Newton and Krylov counts.
    python scripts/periodic_cell_compare.py OUT_DIR [--root CHECKOUT] [--ranks 1|2|8] [--no-mask]"""
import argparse
import ctypes as C
import json
import os
import sys
import threading

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSTEPS, N = 4, 4
L1 = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0e-3]]
L2 = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 5.0e-4]]
FREE_XY = [[1, 0, 0], [0, 1, 0], [0, 0, 0]]


def _mat(m):
    return "[" + ", ".join("[" + ", ".join(repr(x) for x in row) + "]" for row in m) + "]"


def write_case(out, ref, mask):
    gfile = os.path.join(out, "grains.txt")
    with open(gfile, "w") as fh:
        fh.write("".join("%d\n" % (e + 1) for e in range(N ** 3)))
    bcs = "    periodic = true\n    changing_ess_bcs = true\n    update_steps = [1, 3]\n    essential_vel_grad = [%s, %s]\n" % (_mat(L1), _mat(L2))
    if mask:
        bcs += "    periodic_free = %s\n" % _mat(FREE_XY)
    txt = f'''Version = "0.6.0"
[Properties]
    temperature = 298
    [Properties.Matl_Props]
        floc = "{ref}/props_cp_voce.txt"
        num_props = 17
    [Properties.State_Vars]
        floc = "{ref}/state_cp_voce.txt"
        num_vars = 24
    [Properties.Grain]
        ori_state_var_loc = 9
        ori_stride = 4
        ori_type = "quat"
        num_grains = 500
        ori_floc = "{ref}/voce_quats.ori"
        grain_floc = "{gfile}"
[BCs]
{bcs}[Model]
    mech_type = "exacmech"
    cp = true
    [Model.ExaCMech]
        xtal_type = "fcc"
        slip_type = "powervoce"
[Time]
    [Time.Custom]
        nsteps = 40
        floc = "{ref}/custom_dt.txt"
[Visualizations]
    steps = 1
    avg_stress_fname = "avg_stress.txt"
    macro_tangent = true
    macro_tangent_rel_tol = 1e-11
[Solvers]
    assembly = "PA"
    integ_model = "FULL"
    rtmodel = "GPU"
    [Solvers.NR]
        iter = 50
        rel_tol = 1e-10
        abs_tol = 1e-14
        nl_solver = "NR"
    [Solvers.Krylov]
        iter = 20000
        rel_tol = 1e-12
        abs_tol = 1e-30
        solver = "PCG"
[Mesh]
    type = "auto"
    ref_ser = 0
    p_refinement = 1
    [Mesh.Auto]
        length = [1.0, 1.0, 1.0]
        ncuts = [{N}, {N}, {N}]
'''
    path = os.path.join(out, "case.toml")
    with open(path, "w") as fh:
        fh.write(txt)
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--ranks", type=int, default=1, choices=(1, 2, 8))
    ap.add_argument("--no-mask", action="store_true")
    a = ap.parse_args()
    os.environ["EXA_DETERMINISTIC"] = "1"
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import exaconstit_amd.lib as L
    out = os.path.abspath(a.out_dir)
    os.makedirs(out, exist_ok=True)
    toml = write_case(out, os.path.join(root, "tests", "golden", "refdata"), not a.no_mask)
    nranks = a.ranks
    gid = (C.c_ubyte * 128)()
    if nranks > 1:
        assert L.exa_loopback_group_create(nranks, gid) == 0
    res, errors = [None] * nranks, []

    def work(r):
        try:
            d = L.Driver.from_toml(toml, out_dir=out, rank=r, nranks=nranks, uid=gid if nranks > 1 else None, write_files=True, restart="")
            for ti in range(1, NSTEPS + 1):
                assert d.step(ti), (r, ti)
            d.save_checkpoint(os.path.join(out, "final.ckpt"))
            newton, krylov, _ = d.stats()
            mi = d.macro_info()
            res[r] = dict(avg_stress=d.avgs(0, 6)[-1].tolist(), newton=[int(x) for x in newton], krylov=[int(x) for x in krylov],
                          vel_grad=[float(x) for x in mi["vel_grad"].ravel()], groups=d.periodic_info()["groups"] if r == 0 else None)
            d.close()
        except Exception as e:   # noqa: BLE001
            errors.append((r, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
    [t.start() for t in th]
    [t.join(timeout=600) for t in th]
    if nranks > 1:
        L.exa_loopback_group_destroy(gid)
    groups = res[0].pop("groups") if res[0] else None
    for r in res[1:]:
        if r:
            r.pop("groups")
    ok = not errors and all(r is not None and r == res[0] for r in res)
    print(json.dumps(dict(build_id=L.exa_build_id().decode(), library=L.LIB_PATH, ranks=nranks, mask=not a.no_mask, ok=ok, errors=errors, rank0=res[0],
                          groups_rank0=groups, files=sorted(f for _, _, fs in os.walk(out) for f in fs))))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
