#!/usr/bin/env python
"""Tetrahedron rates: Kuhn-split N^3 cubes (6 tetrahedra per cell) at p = 1 and 2, the Voce FCC case of tests/golden/refdata,
constitutive point updates/s, PCG iterations/s and the Krylov action per launch - the fused tetrahedron kernel (default) against the table-driven
route (EXA_TET_ACTION=generic) - with the fraction of the 8 TB/s HBM peak on each route's byte model.

    python scripts/tet_rates.py --sizes 32 64 --out profiles/tet_rates.json

The fused action's time per launch is measured by exa_driver_bench_pcg (back-to-back exa_grad_apply_lvec launches).  The table-driven route has
no such hook (its action is restriction + point stage + element contraction + transpose restriction); its per-launch time is the PCG loop time per
iteration minus the vector work, which both routes share: t_generic_action = t_pcg,generic - (t_pcg,fused - t_action,fused).
"""
import argparse
import itertools
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0


def kuhn_mesh_file(path, N):
    """Vectorised Kuhn split (the layout of tests/tet_mesh_util.kuhn_cube, unperturbed) written as MFEM mesh v1.0; returns (E, NV)."""
    import tet_mesh_util as T
    n1 = N + 1
    g = np.arange(n1)
    X = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).transpose(2, 1, 0, 3).reshape(-1, 3).astype(float) / N
    k, j, i = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    i, j, k = i.ravel(), j.ravel(), k.ravel()
    base = i + n1 * (j + n1 * k)
    step = np.array([1, n1, n1 * n1])
    g5 = T.refdata_grains()
    grain = g5[(i * 5 // N) + 5 * ((j * 5 // N) + 5 * (k * 5 // N))]
    tets, attr = [], []
    for perm in itertools.permutations(range(3)):
        o1 = step[perm[0]]; o2 = o1 + step[perm[1]]; o3 = o2 + step[perm[2]]
        t = np.stack([base, base + o1, base + o2, base + o3], axis=1)
        a = X[t[0, 1]] - X[t[0, 0]]; b = X[t[0, 2]] - X[t[0, 0]]; c = X[t[0, 3]] - X[t[0, 0]]
        if np.dot(a, np.cross(b, c)) < 0:
            t = t[:, [0, 1, 3, 2]]
        tets.append(t); attr.append(grain)
    tets = np.concatenate(tets); attr = np.concatenate(attr)
    # boundary triangles: each boundary cell face split along its min-corner -> max-corner diagonal (the one the Kuhn tetrahedra share)
    tris, tattr = [], []
    u, w = np.meshgrid(np.arange(N), np.arange(N), indexing="ij"); u, w = u.ravel(), w.ravel()
    for d, (lo_id, hi_id) in ((2, (1, 4)), (0, (2, 5)), (1, (3, 6))):
        a1, a2 = [x for x in range(3) if x != d]
        for side, fid in ((0, lo_id), (N, hi_id)):
            c = np.zeros((u.size, 3), int); c[:, a1] = u; c[:, a2] = w; c[:, d] = side
            v0 = c[:, 0] + n1 * (c[:, 1] + n1 * c[:, 2])
            va, vb, vd = v0 + step[a1], v0 + step[a2], v0 + step[a1] + step[a2]
            tris += [np.stack([v0, va, vd], 1), np.stack([v0, vb, vd], 1)]; tattr += [np.full(u.size, fid)] * 2
    tris = np.concatenate(tris); tattr = np.concatenate(tattr)
    with open(path, "w") as f:
        f.write("MFEM mesh v1.0\n\ndimension\n3\n\nelements\n%d\n" % len(tets))
        np.savetxt(f, np.column_stack([attr, np.full(len(tets), 4), tets]), fmt="%d")
        f.write("\nboundary\n%d\n" % len(tris))
        np.savetxt(f, np.column_stack([tattr, np.full(len(tris), 2), tris]), fmt="%d")
        f.write("\nvertices\n%d\n3\n" % len(X))
        np.savetxt(f, X, fmt="%.17g")
    return len(tets), len(X)


def options(path, mesh, p):
    ref = os.path.join(ROOT, "tests", "golden", "refdata")
    txt = open(os.path.join(ref, "voce_pa.toml")).read()
    for fl in ("props_cp_voce.txt", "state_cp_voce.txt", "voce_quats.ori", "grains.txt", "custom_dt.txt"):
        txt = txt.replace('"%s"' % fl, '"%s"' % os.path.join(ref, fl))
    txt = txt.replace('type = "auto"', 'type = "other"').replace('floc = "../../data/cube-hex-ro.mesh"', 'floc = "%s"' % mesh)
    txt = txt.replace("ref_ser = 1", "ref_ser = 0").replace("prefinement = 1", "p_refinement = %d" % p)
    with open(path, "w") as f:
        f.write(txt)
    return path


def byte_models(E, NN, p):
    """Bytes per launch of the action, lower bounds: every stream read once, the L-vectors (x read, y read + written) once per node.
    p = 1 fused: 18 record pairs + the nodal coordinates (J^-1 recomputed); the stored-J^-1 form reads 5 pairs more per element."""
    n, Q = (4, 5) if p == 1 else (10, 14)
    vec = 3 * 8 * NN * 3
    fused = E * (18 * 16 + 4 * n) + vec + 3 * 8 * NN if p == 1 else E * (Q * 23 * 16 + 4 * n) + vec   # p = 1: Cbar record + coordinates
    ev = 3 * n * 8 * E
    generic = (E * 4 * n + 3 * 8 * NN + ev) + (ev + E * Q * 23 * 16 + 9 * 8 * Q * E) + (9 * 8 * Q * E + ev + ev) + (E * 4 * n + ev + 2 * 3 * 8 * NN)
    return fused, generic


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--orders", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import exaconstit_amd.lib as L
    tmp = tempfile.mkdtemp(prefix="tet_rates_")
    dts = np.loadtxt(os.path.join(ROOT, "tests", "golden", "refdata", "custom_dt.txt"))[:3]
    rows = []
    for N in args.sizes:
        mesh = os.path.join(tmp, "kuhn%d.mesh" % N)
        t0 = time.time(); E, NV = kuhn_mesh_file(mesh, N); t_mesh = time.time() - t0
        for p in args.orders:
            res = {}
            for route in ("fused", "generic") + (("fused_stored",) if p == 1 else ()):
                os.environ.pop("EXA_TET_ACTION", None); os.environ.pop("EXA_TET_APPLY_GEO", None)
                if route == "generic":
                    os.environ["EXA_TET_ACTION"] = "generic"
                elif route == "fused_stored":      # p = 1: J^-1 read from the element record instead of recomputed from the coordinates
                    os.environ["EXA_TET_APPLY_GEO"] = "off"
                t0 = time.time()
                d = L.Driver.from_toml(options(os.path.join(tmp, "o.toml"), mesh, p), out_dir=tmp, write_files=False)
                info = d.mesh_info()
                d.bench_prepare(dts)
                t_setup = time.time() - t0
                m = d.bench_model(args.steps)
                pc = d.bench_pcg(args.iters)
                d.close()
                P = info["elements"] * info["qpts_per_elem"]
                res[route] = {"route": info["action_route"], "model_qpt_per_s": P * args.steps / (m["loop_ms"] * 1e-3),
                              "model_kernel_ms": m["kernel_ms"] / args.steps, "pcg_it_per_s": pc["iters"] / (pc["pcg_ms"] * 1e-3),
                              "pcg_ms_per_it": pc["pcg_ms"] / pc["iters"], "fused_action_ms": pc["apply_ms"] / args.iters, "setup_s": t_setup}
                info_keep = info
            os.environ.pop("EXA_TET_ACTION", None); os.environ.pop("EXA_TET_APPLY_GEO", None)
            fb, gb = byte_models(info_keep["elements"], info_keep["nodes"], p)
            t_f = res["fused"]["fused_action_ms"]
            t_g = res["generic"]["pcg_ms_per_it"] - (res["fused"]["pcg_ms_per_it"] - t_f)
            row = {"N": N, "p": p, "elements": info_keep["elements"], "nodes": info_keep["nodes"], "qpts_per_elem": info_keep["qpts_per_elem"],
                   "mesh_write_s": t_mesh, "fused": res["fused"], "generic": res["generic"],
                   "action_ms": {"fused": t_f, "generic": t_g},
                   "action_bytes": {"fused": fb, "generic": gb},
                   "hbm_fraction": {"fused": fb / (t_f * 1e-3) / (HBM_PEAK_GBS * 1e9), "generic": gb / (t_g * 1e-3) / (HBM_PEAK_GBS * 1e9) if t_g > 0 else None},
                   "action_speedup": t_g / t_f if t_f > 0 else None}
            if "fused_stored" in res:
                row["fused_stored"] = res["fused_stored"]
                row["action_ms"]["fused_stored"] = res["fused_stored"]["fused_action_ms"]
                row["action_bytes"]["fused_stored"] = fb + 5 * 16 * info_keep["elements"] - 3 * 8 * info_keep["nodes"]
                row["hbm_fraction"]["fused_stored"] = row["action_bytes"]["fused_stored"] / (row["action_ms"]["fused_stored"] * 1e-3) / (HBM_PEAK_GBS * 1e9)
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = {"kernel_build_id": L.exa_kernel_build_id().decode(), "build_id": L.exa_build_id().decode(), "steps": args.steps, "iters": args.iters,
           "hbm_peak_gbs": HBM_PEAK_GBS, "rows": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"summary": [(r["N"], r["p"], round(r["action_ms"]["fused"], 4), round(r["action_ms"]["generic"], 4)) for r in rows]}))


if __name__ == "__main__":
    main()
