"""Checkpoint files without a GPU: the documented format against an independent numpy writer, the refusals that need no device,
the [Checkpoint] option table and the local -> global node map the field sections are addressed by."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import partition_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "refdata")
MASK = (1 << 64) - 1


def _sum64(b):
    return int(np.frombuffer(b, "<u8").sum(dtype=np.uint64))


def write_checkpoint(path, hdr, sections):
    """Writer that follows DESIGN 4.10 and nothing else: 256-byte header, 48-byte table entries, sections at multiples of 64 bytes."""
    names = list(sections)
    blobs = []
    for n in names:
        b = np.ascontiguousarray(sections[n]).tobytes()
        blobs.append(b + b"\0" * (-len(b) % 8))
    off = 256 + 48 * len(names)
    table = b""
    offs = []
    for n, b in zip(names, blobs):
        off = (off + 63) // 64 * 64
        offs.append(off)
        table += n.encode().ljust(24, b"\0") + struct.pack("<QQQ", off, len(b), _sum64(b))
        off += len(b)
    h = bytearray(256)
    h[0:8] = b"EXACKPT\0"
    for key, fmt, o in (("version", "<I", 8), ("header_bytes", "<I", 12), ("elements", "<q", 16), ("nodes", "<q", 24), ("qpts_per_elem", "<i", 32), ("geometry", "<i", 36),
                        ("order", "<i", 40), ("model", "<i", 44), ("nprops", "<i", 48), ("nstatev", "<i", 52), ("props_hash", "<Q", 56), ("grain_hash", "<Q", 64),
                        ("conn_hash", "<Q", 72), ("steps_done", "<q", 80), ("time", "<d", 88), ("dt_class", "<d", 96), ("last_dt", "<d", 104), ("bc_index", "<i", 112),
                        ("nranks", "<i", 116), ("flags", "<I", 120), ("nsections", "<i", 124), ("model_calls", "<q", 128), ("newton_cap", "<i", 136),
                        ("newton_cap2", "<i", 140), ("writer", "<I", 144)):
        struct.pack_into(fmt, h, o, hdr[key])
    struct.pack_into("<Q", h, 248, _sum64(bytes(h[:248])))
    with open(path, "wb") as f:
        f.write(bytes(h) + table)
        for o, b in zip(offs, blobs):
            if b:                     # (an empty section holds no bytes: the file is not extended to its offset)
                f.seek(o)
                f.write(b)
    return dict(zip(names, zip(offs, [len(b) for b in blobs])))


def _example(seed=3):
    rng = np.random.default_rng(seed)
    E, Q, NN, steps = 12, 8, 36, 3
    hdr = dict(version=1, header_bytes=256, elements=E, nodes=NN, qpts_per_elem=Q, geometry=0, order=1, model=2, nprops=17, nstatev=28, props_hash=0x0123456789abcdef,
               grain_hash=MASK - 5, conn_hash=77, steps_done=steps, time=0.35, dt_class=0.15, last_dt=0.1, bc_index=0, nranks=4, flags=3, nsections=0, model_calls=19,
               newton_cap=5, newton_cap2=0, writer=0x48415845)
    sec = {"avg_stress": rng.standard_normal((steps, 6)), "solver_stats": rng.integers(0, 50, (steps, 4)).astype(np.int32),   # 48 bytes: a whole number of words
           "pvd_cycles": np.array([[0, 0.0], [2, 0.2]]), "lattice_strains": np.zeros(0), "lattice_volumes": np.zeros(0), "auto_dt": np.zeros(0),
           "x_beg": rng.standard_normal((NN, 3)), "v_sol": rng.standard_normal((NN, 3)), "stress0": rng.standard_normal((E, Q, 6)),
           "matVars0": rng.standard_normal((E, Q, 28))}
    hdr["nsections"] = len(sec)
    return hdr, sec


def test_numpy_written_file_reads_back(tmp_path):
    import exaconstit_amd.lib as L
    hdr, sec = _example()
    p = str(tmp_path / "a.ckpt")
    where = write_checkpoint(p, hdr, sec)
    info = L.checkpoint_info(p)
    for k in L.CHECKPOINT_INFO_KEYS:
        assert info[k] == hdr[{"elements": "elements", "nodes": "nodes"}.get(k, k)], k
    assert (info["time"], info["dt_class"], info["last_dt"]) == (0.35, 0.15, 0.1)
    assert (info["props_hash"], info["grain_hash"], info["conn_hash"]) == (hdr["props_hash"], hdr["grain_hash"], hdr["conn_hash"])
    assert info["cycle0_saved"] and info["texture0_written"]
    assert list(info["sections"]) == list(sec)
    for n, (off, nb) in where.items():
        assert info["sections"][n][:2] == (off, nb) and off % 64 == 0
    r = L.read_checkpoint(p)
    for k, v in hdr.items():
        assert r["header"][k] == v, k
    for n, a in sec.items():
        assert r[n].shape == (a.shape if a.size else r[n].shape) and np.array_equal(r[n].ravel(), a.ravel()), n
        assert r[n].dtype == a.dtype
    assert r["stress0"].shape == (12, 8, 6) and r["matVars0"].shape == (12, 8, 28) and r["x_beg"].shape == (36, 3) and r["solver_stats"].shape == (3, 4)


def test_empty_trailing_section_after_a_short_one(tmp_path):
    """x_beg_copies with one entry (40 bytes, not a multiple of the 64-byte section alignment) followed by an empty v_sol_copies whose offset lies
    beyond the last byte of the file: an empty section holds no bytes wherever its offset points, so the file is complete."""
    import exaconstit_amd.lib as L
    hdr, sec = _example()
    entry = np.array([[1 + (4 << 32), 17, 0, 0, 0]], np.int64)
    entry[0, 2:] = np.array([0.25, -1.5, 3.0]).view(np.int64)
    sec["x_beg_copies"] = entry
    sec["v_sol_copies"] = np.zeros((0, 5), np.int64)
    hdr["nsections"] = len(sec)
    p = str(tmp_path / "c.ckpt")
    where = write_checkpoint(p, hdr, sec)
    assert where["v_sol_copies"][0] > os.path.getsize(p) and where["v_sol_copies"][1] == 0 and where["x_beg_copies"][1] == 40
    info = L.checkpoint_info(p)
    assert info["sections"]["x_beg_copies"][:2] == where["x_beg_copies"] and info["sections"]["v_sol_copies"][1] == 0
    for copy in (True, False):
        r = L.read_checkpoint(p, copy=copy)
        assert np.array_equal(r["x_beg_copies"], entry) and r["v_sol_copies"].shape == (0, 5)
        assert np.array_equal(r["matVars0"], sec["matVars0"]) and np.array_equal(r["solver_stats"], sec["solver_stats"])
    raw = open(p, "rb").read()
    open(p, "wb").write(raw[:-1])                                        # ... while a byte missing from the short one is a truncation
    with pytest.raises(RuntimeError, match="truncated.*x_beg_copies"):
        L.checkpoint_info(p)
    with pytest.raises(ValueError, match="truncated.*x_beg_copies"):
        L.read_checkpoint(p)


def test_refusals_without_a_gpu(tmp_path):
    import exaconstit_amd.lib as L
    hdr, sec = _example()
    good = str(tmp_path / "good.ckpt")
    where = write_checkpoint(good, hdr, sec)
    raw = open(good, "rb").read()

    def both(data, *words):
        p = str(tmp_path / "bad.ckpt")
        open(p, "wb").write(data)
        for fn, exc in ((L.checkpoint_info, RuntimeError), (L.read_checkpoint, ValueError)):
            with pytest.raises(exc) as e:
                fn(p)
            for w in words:
                assert w in str(e.value), (fn.__name__, str(e.value))

    both(b"NOTACKPT" + raw[8:], "wrong magic")
    both(raw[:5], "wrong magic")
    v2 = bytearray(raw); struct.pack_into("<I", v2, 8, 2); struct.pack_into("<Q", v2, 248, _sum64(bytes(v2[:248])))
    both(bytes(v2), "unsupported format version 2")
    both(raw[:100], "truncated")
    both(raw[:256 + 48 * 3], "truncated", "section table")
    hb = bytearray(raw); hb[90] ^= 0x10                      # a bit of `time`
    both(bytes(hb), "checksum mismatch in the header")
    # cut at every section boundary and one byte short of every section's end: the first incomplete section is named
    order = sorted((o, nb, n) for n, (o, nb) in where.items() if nb)
    for i, (o, nb, n) in enumerate(order):
        both(raw[:o + nb - 1], "truncated", "section '%s'" % n)
        both(raw[:o], "truncated", "section '%s'" % n)
    # one flipped bit in a field section: the numpy reader recomputes every checksum and names the section (the library does so when it loads:
    # tests/test_gpu_checkpoint.py); the header query does not read the sections
    for n in ("x_beg", "v_sol", "stress0", "matVars0", "avg_stress"):
        o, nb = where[n]
        fb = bytearray(raw); fb[o + nb // 2] ^= 0x01
        p = str(tmp_path / "flip.ckpt"); open(p, "wb").write(bytes(fb))
        with pytest.raises(ValueError, match="checksum mismatch in section '%s'" % n):
            L.read_checkpoint(p)
        assert L.checkpoint_info(p)["steps_done"] == 3
    with pytest.raises(RuntimeError, match="cannot open"):
        L.checkpoint_info(str(tmp_path / "missing.ckpt"))


def _toml(tmp_path, name, extra="", replace=()):
    text = open(os.path.join(REF, name)).read()
    for fl in ("props_cp_voce.txt", "state_cp_voce.txt", "voce_quats.ori", "grains.txt", "custom_dt.txt"):
        text = text.replace('"%s"' % fl, '"%s"' % os.path.join(REF, fl))
    for a, b in replace:
        assert a in text
        text = text.replace(a, b)
    p = tmp_path / ("case_%d.toml" % len(list(tmp_path.iterdir())))
    p.write_text(text + "\n" + extra)
    return str(p)


def test_checkpoint_options(tmp_path):
    import exaconstit_amd.lib as L
    plain = os.path.join(REF, "voce_pa.toml")
    assert L.options_checkpoint(plain) == dict(write=False, steps=1, keep=2, floc="checkpoint", restart_from="")
    t = _toml(tmp_path, "voce_pa.toml", '[Checkpoint]\nwrite = true\nsteps = 5\nfloc = "ck"\nkeep = 3\nrestart_from = "old/ck_000010.ckpt"\n')
    assert L.options_checkpoint(t) == dict(write=True, steps=5, keep=3, floc="ck", restart_from="old/ck_000010.ckpt")
    assert L.options_checkpoint(_toml(tmp_path, "voce_pa.toml", "[Checkpoint]\nwrite = true\n")) == dict(write=True, steps=1, keep=2, floc="checkpoint", restart_from="")
    # the table changes nothing else: the general query returns what it returns for the file without it
    q0, q1 = np.zeros(20), np.zeros(20)
    err = C.create_string_buffer(512)
    dp = C.POINTER(C.c_double)
    assert L.exa_options_query(_toml(tmp_path, "voce_pa.toml").encode(), q0.ctypes.data_as(dp), err, 512) == 0
    assert L.exa_options_query(t.encode(), q1.ctypes.data_as(dp), err, 512) == 0
    assert np.array_equal(q0, q1)
    ref = np.zeros(20)
    assert L.exa_options_query(plain.encode(), ref.ctypes.data_as(dp), err, 512) == 0 and np.array_equal(ref, q0)
    assert ref[1] == 17 and ref[7] == 40 and ref[17] == 5
    for body, key in (('write = "yes"', "Checkpoint.write"), ("write = 1", "Checkpoint.write"), ("steps = 0", "Checkpoint.steps"), ("steps = 2.5", "Checkpoint.steps"),
                      ('steps = "3"', "Checkpoint.steps"), ("keep = 0", "Checkpoint.keep"), ("keep = true", "Checkpoint.keep"), ('floc = "a/b"', "Checkpoint.floc"),
                      ('floc = ""', "Checkpoint.floc"), ("floc = 3", "Checkpoint.floc"), ('restart_from = ""', "Checkpoint.restart_from"),
                      ("restart_from = 7", "Checkpoint.restart_from")):
        with pytest.raises(RuntimeError) as e:
            L.options_checkpoint(_toml(tmp_path, "voce_pa.toml", "[Checkpoint]\n" + body + "\n"))
        assert key in str(e.value), (body, str(e.value))


@pytest.mark.parametrize("nranks,order", [(1, 1), (2, 1), (3, 1), (4, 1), (8, 1), (1, 2), (4, 2)])
def test_node_map_of_block_decomposition(nranks, order):
    """Every global node is held by at least one rank, ranks agree on the coordinates of the nodes they share, and the numbering is the node grid's."""
    import exaconstit_amd.lib as L
    N = (6, 5, 4)
    nn_glob = (N[0] * order + 1) * (N[1] * order + 1) * (N[2] * order + 1)
    seen = np.zeros(nn_glob, np.int64)
    X = np.full((3, nn_glob), np.nan)
    for r in range(nranks):
        part = pu.query(N, r, nranks, order)
        gid, ng = L.partition_nodes(N, r, nranks, order)
        assert ng == nn_glob and gid.shape == (part["NN"],)
        assert len(set(gid.tolist())) == part["NN"] and gid.min() >= 0 and gid.max() < nn_glob
        assert np.array_equal(gid, pu.global_node_ids(part, N))
        held = seen[gid] > 0
        assert np.array_equal(X[:, gid[held]], part["X"][:, held])          # shared nodes: the same coordinates, bit for bit
        X[:, gid] = part["X"]
        seen[gid] += 1
    assert seen.min() >= 1
    w = np.zeros(nn_glob)
    for r in range(nranks):
        part = pu.query(N, r, nranks, order)
        gid, _ = L.partition_nodes(N, r, nranks, order)
        np.add.at(w, gid, part["weight"])
    assert np.allclose(w, 1.0)                                               # weight = 1 / (ranks holding the node), by the same numbering


@pytest.mark.parametrize("mesh,order", [("cube5_shuffled.mesh", 1), ("cube5_shuffled.mesh", 2), ("cube5_nodes.mesh", 3)])
@pytest.mark.parametrize("nranks", [1, 2, 4])
def test_node_map_of_file_mesh(mesh, order, nranks):
    import exaconstit_amd.lib as L
    path = os.path.join(REF, mesh)
    g1, ng = L.partition_nodes(None, 0, 1, order, mesh=path)
    assert np.array_equal(g1, np.arange(ng))                                 # one rank: the reader's numbering
    X1 = _mesh_X(L, path, 0, 1, order)
    seen = np.zeros(ng, np.int64)
    for r in range(nranks):
        gid, ng2 = L.partition_nodes(None, r, nranks, order, mesh=path)
        assert ng2 == ng and len(set(gid.tolist())) == len(gid)
        assert np.array_equal(_mesh_X(L, path, r, nranks, order), X1[:, gid])   # a rank's node IS the global node of that number
        seen[gid] += 1
    assert seen.min() >= 1


def _mesh_X(L, path, rank, nranks, order):
    info = (C.c_int64 * 8)()
    err = C.create_string_buffer(512)
    assert L.exa_mesh_partition_query_order(path.encode(), rank, nranks, order, info, None, None, None, None, None, None, None, err, 512) == 0, err.value
    X = np.zeros(3 * info[1])
    assert L.exa_mesh_partition_query_order(path.encode(), rank, nranks, order, info, None, X.ctypes.data_as(C.c_void_p), None, None, None, None, None, err, 512) == 0
    return X.reshape(3, info[1])
