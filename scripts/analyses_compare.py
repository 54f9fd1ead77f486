"""One options-file run with every in-situ analysis on, into a given directory: the case two builds of the library are compared on (same files, same
checkpoints, same kernels) when the host code around the analyses changes.
  case: voce_full_cyclic on 5^3 elements (the _cyclic_toml recipe of tests/test_gpu_fatigue.py: 16 steps, the load reversed at steps 5 and 13),
        EXA_DETERMINISTIC=1, Visualizations.steps = 8, fatigue_cycle_steps = 8, ParaView, light-up, per-grain averages, texture, lattice curvature,
        slip activity and the additional averages on, [Checkpoint] every 8 steps
  --root: the checkout whose package is loaded (default: the one this script lies in); the case files come from the same checkout
Two runs are the same when `diff -r -x time -x '*.toml'` of their directories is empty (the .ckpt files are in it; time/ holds wall times, the
.toml names its checkout) - and, each under `rocprofv3 --kernel-trace --stats` in a run of its own, when kernel names and call counts agree.
Prints one JSON line: build id, steps run, Driver.diagnostics().
    python scripts/analyses_compare.py OUT_DIR [--root CHECKOUT]"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALL_ON = ["paraview = true", "steps = 8", "light_up = true", "light_up_hkl = [[1,1,1],[2,0,0],[2,2,0]]", "light_up_dist_tol_deg = 15.0",
          "grain_avgs = true", "texture = true", "lattice_curvature = true", "lattice_curvature_burgers = 2.5e-7",
          "fatigue = true", "fatigue_sigma_y = 0.2", "fatigue_cycle_steps = 8", "additional_avgs = true"]
CHECKPOINT = "[Checkpoint]\n    write = true\n    steps = 8\n    keep = 4\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--root", default=HERE)
    a = ap.parse_args()
    os.environ["EXA_DETERMINISTIC"] = "1"
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import exaconstit_amd.lib as L
    import test_gpu_fatigue as F
    out = os.path.abspath(a.out_dir)
    os.makedirs(out, exist_ok=True)
    d = L.Driver.from_toml(F._cyclic_toml(out, "all_on", ALL_ON, CHECKPOINT), out_dir=out)
    n = d.run()
    diag = d.diagnostics()
    d.close()
    print(json.dumps(dict(build_id=L.exa_build_id().decode(), library=L.LIB_PATH, steps=n, diagnostics=diag, files=sum(len(f) for _, _, f in os.walk(out)))))
    return 0 if n == 16 else 1


if __name__ == "__main__":
    sys.exit(main())
