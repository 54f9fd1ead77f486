"""Per-grain averages, host side: the Visualizations.grain_avgs options (exa_options_query_grains) and that the existing queries ignore them,
the grain_avgs file writer (exa_grain_avgs_write) round trip, and the reduction plan of exa_grain_sums (exa_grain_plan) replayed in numpy the
way the kernel walks it.  No GPU."""
import os
import shutil

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDATA = os.path.join(ROOT, "tests", "golden", "refdata")


def _stage(tmp_path, vis_lines, name="voce_pa.toml"):
    for f in os.listdir(REFDATA):
        if f.endswith((".txt", ".ori", ".mesh")):
            shutil.copy(os.path.join(REFDATA, f), str(tmp_path))
    t = open(os.path.join(REFDATA, "voce_pa.toml")).read()
    a, b = t.index("[Visualizations]"), t.index("[Solvers]")
    t = t[:a] + "[Visualizations]\n" + "".join("    %s\n" % x for x in vis_lines) + t[b:]
    path = os.path.join(str(tmp_path), name)
    open(path, "w").write(t)
    return path


def test_grain_options_defaults(tmp_path):
    import exaconstit_amd.lib as L
    assert L.options_grains(_stage(tmp_path, ["paraview = false"])) == dict(enabled=False, fname="grain_avgs")
    assert L.options_grains(_stage(tmp_path, ["grain_avgs = true"])) == dict(enabled=True, fname="grain_avgs")
    assert L.options_grains(_stage(tmp_path, ["grain_avgs = false", 'grain_avgs_fname = "g"'])) == dict(enabled=False, fname="g")
    assert L.options_grains(_stage(tmp_path, ["grain_avgs = true", 'grain_avgs_fname = "per_grain.x"'])) == dict(enabled=True, fname="per_grain.x")


@pytest.mark.parametrize("name", sorted(f for f in os.listdir(REFDATA) if f.endswith(".toml")))
def test_golden_option_files_leave_grains_off(name):
    import exaconstit_amd.lib as L
    assert L.options_grains(os.path.join(REFDATA, name)) == dict(enabled=False, fname="grain_avgs")


@pytest.mark.parametrize("line,msg", [
    ("grain_avgs = 1", "true or false"),
    ('grain_avgs = "true"', "true or false"),
    ("grain_avgs = [true]", "true or false"),
    ('grain_avgs_fname = ""', "grain_avgs_fname"),
    ('grain_avgs_fname = "out/grains"', "grain_avgs_fname"),
    ("grain_avgs_fname = 3", "grain_avgs_fname"),
])
def test_grain_options_refused(tmp_path, line, msg):
    import exaconstit_amd.lib as L
    with pytest.raises(RuntimeError, match=msg):
        L.options_grains(_stage(tmp_path, ["grain_avgs = true", line] if not line.startswith("grain_avgs =") else [line]))


def test_existing_queries_unchanged_by_grain_keys(tmp_path):
    import ctypes as C

    import exaconstit_amd.lib as L
    base = ["paraview = true", "steps = 3", "light_up = true", "light_up_hkl = [[1, 1, 1]]", 'floc = "vis/out"']
    d0, d1 = tmp_path / "a", tmp_path / "b"
    d0.mkdir()
    d1.mkdir()
    p0 = _stage(d0, base)
    p1 = _stage(d1, base + ["grain_avgs = true", 'grain_avgs_fname = "gr"'])

    def q20(p):
        out = np.zeros(20)
        err = C.create_string_buffer(512)
        assert L.exa_options_query(p.encode(), out.ctypes.data_as(C.POINTER(C.c_double)), err, 512) == 0, err.value
        return out
    assert np.array_equal(q20(p0), q20(p1))
    assert L.options_vis(p0) == L.options_vis(p1)
    assert L.options_lightup(p0) == L.options_lightup(p1)
    assert L.options_grains(p0)["enabled"] is False and L.options_grains(p1) == dict(enabled=True, fname="gr")


def test_writer_round_trip(tmp_path):
    import exaconstit_amd.lib as L
    rng = np.random.default_rng(3)
    n = 57
    ids = np.sort(rng.choice(np.arange(1, 10000), n, replace=False)).astype(np.int32)
    vals = rng.standard_normal((n, L.EXA_GRAIN_NVALS)) * 10.0 ** rng.uniform(-300, 300, (n, L.EXA_GRAIN_NVALS))
    vals[:, 0] = rng.integers(1, 2 ** 40, n)                                     # the element count, written as an integer
    vals[0, 5] = 0.0
    vals[1, 6] = -0.0
    vals[2, 7] = 5e-324                                                          # subnormal
    path = str(tmp_path / "grain_avgs_000003.txt")
    L.write_grain_avgs(path, ids, vals)
    lines = open(path).read().splitlines()
    assert len(lines) == n + 1
    head = lines[0].split()
    assert head[0] == "#" and len(head) == 47                                   # '#' and the 46 column names
    assert head[1:5] == ["grain_id", "n_elements", "volume", "volume_fraction"] and head[-3:] == ["misori_mean_deg", "misori_max_deg", "rotation_deg"]
    assert head.count("shear_rate_12") == 1 and head[-7:-3] == ["quat_0", "quat_1", "quat_2", "quat_3"]
    assert all(len(x.split()) == 46 for x in lines[1:])
    assert all(x.split()[1].isdigit() for x in lines[1:])
    got = L.read_grain_avgs(path)
    assert np.array_equal(got["grain_id"], ids)
    assert np.array_equal(got["n_elements"], vals[:, 0].astype(np.int64))
    for k, (c0, m) in L.GRAIN_COLUMNS.items():
        if k == "n_elements":
            continue
        ref = vals[:, c0] if m == 1 else vals[:, c0:c0 + m]
        assert np.array_equal(got[k], ref), k                                    # 17 significant digits: every double round-trips
    # no rows: the header alone
    L.write_grain_avgs(str(tmp_path / "empty.txt"), np.zeros(0, np.int32), np.zeros((0, L.EXA_GRAIN_NVALS)))
    assert len(open(str(tmp_path / "empty.txt")).read().splitlines()) == 1
    with pytest.raises(RuntimeError):
        L.write_grain_avgs(str(tmp_path / "no" / "such" / "dir.txt"), ids, vals)


# ---- the plan of exa_grain_sums --------------------------------------------------------------------------------------------------------

def _plan(attr):
    import ctypes as C

    import exaconstit_amd.lib as L
    attr = np.ascontiguousarray(attr, dtype=np.int32)
    ln, wk = C.c_int64(), C.c_int64()
    ip = C.POINTER(C.c_int32)
    assert L.exa_grain_plan(len(attr), attr.ctypes.data_as(ip), None, 0, C.byref(ln), C.byref(wk)) == 0
    plan = np.zeros(ln.value, np.int32)
    assert L.exa_grain_plan(len(attr), attr.ctypes.data_as(ip), plan.ctypes.data_as(ip), ln.value - 1, None, None) != 0   # too small
    assert L.exa_grain_plan(len(attr), attr.ctypes.data_as(ip), plan.ctypes.data_as(ip), ln.value, None, None) == 0
    return plan, wk.value


def _replay(plan, vals, G):
    """what the kernel does with the plan: level 0 on the rows in sorted order, then the boundary partials level by level; every segment is
    written exactly once"""
    Lv = int(plan[0])
    assert plan[1] <= G
    n = [int(x) for x in plan[2:2 + Lv]]
    o = 2 + Lv
    order = plan[o:o + (n[0] if Lv else 0)]
    o += n[0] if Lv else 0
    K = vals.shape[1]
    out = np.zeros((G, K))
    written = np.zeros(G, int)
    src = vals[order] if Lv else None
    items_total = 0
    for lev in range(Lv):
        seg = plan[o:o + n[lev]]
        o += n[lev]
        nch = (n[lev] + 63) // 64
        slots = plan[o:o + 2 * nch]
        o += 2 * nch
        nxt = n[lev + 1] if lev + 1 < Lv else 0
        items_total += nxt
        items = np.full((nxt, K), np.nan)
        assert np.all(np.diff(seg) >= 0)                                         # items stay sorted by segment
        for c in range(nch):
            a, b = 64 * c, min(n[lev], 64 * c + 64)
            r0 = a
            for r in range(a + 1, b + 1):
                if r == b or seg[r] != seg[r0]:
                    val = src[r0:r].sum(0)
                    slot = slots[2 * c] if r0 == a else -1
                    if slot < 0 and r == b:
                        slot = slots[2 * c + 1]
                    if slot >= 0:
                        items[slot] = val
                    else:
                        out[seg[r0]] = val                                 # the items carry the grain row itself
                        written[seg[r0]] += 1
                    r0 = r
        assert not np.isnan(items).any()                                         # every item slot filled once
        src = items
    assert o == len(plan)
    return out, written, items_total


@pytest.mark.parametrize("case", ["one_grain", "per_element", "mixed", "tiny", "edges"])
def test_plan_replay(case):
    rng = np.random.default_rng(len(case))
    if case == "one_grain":
        attr = np.full(300000, 7)                                                # 4 levels
    elif case == "per_element":
        attr = rng.permutation(20000) + 1
    elif case == "mixed":
        sizes = np.concatenate([[6000], rng.integers(1, 400, 200), np.ones(50, int)])
        ids = rng.choice(np.arange(1, 3 * len(sizes)), len(sizes), replace=False)   # non-contiguous, unused ids
        attr = rng.permutation(np.repeat(ids, sizes))
    elif case == "tiny":
        attr = np.array([3])
    else:
        attr = np.repeat([2, 1, 5, 4], [64, 1, 127, 64])                         # segments ending and starting on chunk edges
    E = len(attr)
    G = int(attr.max())
    plan, work = _plan(attr)
    assert plan[1] == G
    vals = rng.standard_normal((E, 3))
    vals[:, 0] = 1.0
    out, written, items = _replay(plan, vals, G)
    assert work == 39 * items
    present = np.unique(attr)
    assert np.all(written[present - 1] == 1) and written.sum() == len(present)
    ref = np.zeros((G, 3))
    np.add.at(ref, attr - 1, vals)
    assert np.array_equal(out[:, 0], ref[:, 0])                                  # element counts exactly
    assert np.allclose(out, ref, rtol=1e-12, atol=1e-12 * np.abs(vals).sum())
    order = plan[2 + plan[0]:2 + plan[0] + E]
    assert np.array_equal(order, np.argsort(attr, kind="stable"))               # sorted by grain, stable in element index


def test_plan_refuses_bad_ids():
    import ctypes as C

    import exaconstit_amd.lib as L
    a = np.array([1, 0, 2], np.int32)
    assert L.exa_grain_plan(3, a.ctypes.data_as(C.POINTER(C.c_int32)), None, 0, None, None) != 0
    n = C.c_int64()
    assert L.exa_grain_plan(0, None, None, 0, C.byref(n), None) == 0 and n.value == 2      # no elements: no levels
