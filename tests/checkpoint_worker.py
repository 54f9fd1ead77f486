"""Second half of an interrupted run in a process of its own (tests/test_gpu_checkpoint.py): nothing of the writer survives in memory.
usage: checkpoint_worker.py <options.toml> <out_dir> <checkpoint to load> <last step> <checkpoint to write at the end>"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    toml, out_dir, ckpt, last, final = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5]
    import exaconstit_amd.lib as L
    d = L.Driver.from_toml(toml, out_dir=out_dir, restart=ckpt)
    first = L.checkpoint_info(ckpt)["steps_done"] + 1
    for ti in range(first, last + 1):
        if not d.step(ti):
            raise SystemExit("Newton failed at step %d" % ti)
    d.save_checkpoint(final)
    newton, krylov, calls = d.stats()
    print("STATS", " ".join(str(int(v)) for v in newton), "|", " ".join(str(int(v)) for v in krylov))
    d.close()


if __name__ == "__main__":
    main()
