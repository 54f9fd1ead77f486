#!/usr/bin/env python
"""Table of the operator's route decision (csrc/host/routes.hpp) through exa_operator_routes_query: host code, no GPU.

Rows "routes|<facts>|<environment>|<one digit per field of ROUTE_FIELDS>": {hex p = 1, 2, 3; tet p = 1, 2} x {full, B-bar (hex)} x {PA, EA} x
{one rank; several ranks with boundary blocks and neighbours; the same over RCCL; the same, periodic}, under nothing set, every value
scripts/check_switches.sh lists for a variable the operator reads (and the remaining operator variables), and the interacting pairs.
Rows "caps|<slip family>|<environment>|<CAP_FIELDS, blank-separated>": the cap fields depend on the slip family and the two cap variables only.

    python scripts/route_table.py [--root CHECKOUT] [OUT_FILE]      (default: the checkout this script lies in; standard output)

tests/test_host_logic.py regenerates the rows and compares them with tests/operator_routes_table.txt, which was recorded from the commit before
routes.hpp existed (profiles/operator_routes.txt)."""
import argparse
import contextlib
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every variable the operator reads
VARIABLES = ["EXA_TET_ACTION", "EXA_DETERMINISTIC", "EXA_NEWTON_CAP", "EXA_TAIL_RESUME", "EXA_EA_ASSEMBLED", "EXA_TET_APPLY_GEO", "EXA_TANGENT_FORM",
             "EXA_APPLY_GEO", "EXA_P2_PREPASS", "EXA_TANGENT_RECORDS", "EXA_QLAYOUT", "EXA_JAC_FIELD", "EXA_LEAN_STATE", "EXA_HALO_OVERLAP", "EXA_NFEV_LOG",
             "EXA_MODEL_TIMES"]
RETIRED = ["EXA_UNFUSED_SETUP", "EXA_TAIL_COST"]
# order of exa_operator_routes_query's output (include/exaconstit_driver.h)
FIELDS = ["fast_p1", "lvec_grad", "lvec_resid", "compact_tangent", "records_setup", "geo_resid", "tet_fused", "tet_geo", "overlap_wish", "cap_auto", "qlayout_eb64",
          "lean_state", "ea_matrix_free", "det", "det_unfused", "grad_set_coords", "newton_cap", "newton_cap2", "tail_resume", "tail_cost_tenths", "action_route",
          "nfev_log", "model_times"]
CAP_FIELDS = ["cap_auto", "newton_cap", "newton_cap2", "tail_resume", "tail_cost_tenths"]
ROUTE_FIELDS = [f for f in FIELDS if f not in CAP_FIELDS]

SINGLE = [{}] + [{k: v} for k, v in (
    # the values of scripts/check_switches.sh for variables the operator reads ...
    ("EXA_QLAYOUT", "aos"), ("EXA_APPLY_GEO", "off"), ("EXA_TANGENT_FORM", "full"), ("EXA_EA_ASSEMBLED", "1"), ("EXA_NEWTON_CAP", "auto"), ("EXA_NEWTON_CAP", "off"),
    ("EXA_DETERMINISTIC", "1"), ("EXA_TANGENT_RECORDS", "off"), ("EXA_HALO_OVERLAP", "off"), ("EXA_TAIL_RESUME", "off"), ("EXA_NEWTON_CAP", "4,7"), ("EXA_JAC_FIELD", "on"),
    ("EXA_P2_PREPASS", "off"),
    # ... and the operator variables it does not sweep
    ("EXA_TET_ACTION", "generic"), ("EXA_TET_APPLY_GEO", "off"), ("EXA_LEAN_STATE", "off"), ("EXA_HALO_OVERLAP", "on"), ("EXA_HALO_OVERLAP", "0"), ("EXA_NFEV_LOG", "1"),
    ("EXA_MODEL_TIMES", "1"))]
PAIRS = [{"EXA_DETERMINISTIC": "1", "EXA_EA_ASSEMBLED": "1"}, {"EXA_QLAYOUT": "aos", "EXA_TANGENT_RECORDS": "off"}, {"EXA_QLAYOUT": "aos", "EXA_P2_PREPASS": "off"},
         {"EXA_EA_ASSEMBLED": "1", "EXA_TET_ACTION": "generic"}, {"EXA_APPLY_GEO": "off", "EXA_TANGENT_FORM": "full"}, {"EXA_NEWTON_CAP": "4,7", "EXA_TAIL_RESUME": "off"}]
CAP_ENVS = [{}, {"EXA_NEWTON_CAP": "auto"}, {"EXA_NEWTON_CAP": "off"}, {"EXA_NEWTON_CAP": "4"}, {"EXA_NEWTON_CAP": "4,7"}, {"EXA_TAIL_RESUME": "off"},
            {"EXA_NEWTON_CAP": "4,7", "EXA_TAIL_RESUME": "off"}, {"EXA_NEWTON_CAP": "auto", "EXA_TAIL_RESUME": "off"}]
# (several ranks, RCCL, boundary blocks, neighbours, periodic)
RANKS = {"one": (0, 0, 0, 0, 0), "several": (1, 0, 1, 1, 0), "rccl": (1, 1, 1, 1, 0), "periodic": (1, 0, 1, 1, 1)}
MESHES = [("hex", 1, 0), ("hex", 1, 1), ("hex", 2, 0), ("hex", 2, 1), ("hex", 3, 0), ("hex", 3, 1), ("tet", 1, 0), ("tet", 2, 0)]
SLIP = ["voce", "voce_nl", "kmdd"]


def facts(geom="hex", order=1, bbar=0, ea=0, slip=0, ranks="one"):
    return [1 if geom == "tet" else 0, order, bbar, ea, slip] + list(RANKS[ranks])


@contextlib.contextmanager
def environment(env, extra=None):
    """exactly env (+ extra) of the operator's and the retired variables set while the body runs; the process's own values afterwards"""
    saved = {k: os.environ.pop(k) for k in VARIABLES + RETIRED if k in os.environ}
    try:
        os.environ.update(env)
        os.environ.update(extra or {})
        yield
    finally:
        for k in VARIABLES + RETIRED:
            os.environ.pop(k, None)
        os.environ.update(saved)


def query(L, f, env=None, extra=None):
    """the query's fields by name for the facts f under env"""
    fa = (C.c_int * len(f))(*f); out = (C.c_int * len(FIELDS))()
    with environment(env or {}, extra):
        n = L.exa_operator_routes_query(fa, len(f), out, len(FIELDS))
    assert n == len(FIELDS), (n, f, env)
    return dict(zip(FIELDS, out))


def env_key(env):
    return " ".join("%s=%s" % kv for kv in sorted(env.items())) or "-"


def table(L, extra=None):
    """the rows as text lines; extra: variables set on top of every row's environment"""
    rows = []
    for geom, order, bbar in MESHES:
        for ea in (0, 1):
            for ranks in RANKS:
                for env in SINGLE + PAIRS:
                    r = query(L, facts(geom, order, bbar, ea, 0, ranks), env, extra)
                    assert all(0 <= r[k] <= 9 for k in ROUTE_FIELDS)
                    rows.append("routes|%s%d %s %s %s|%s|%s" % (geom, order, "bbar" if bbar else "full", "EA" if ea else "PA", ranks, env_key(env),
                                                                 "".join(str(r[k]) for k in ROUTE_FIELDS)))
    for slip in range(3):
        for env in CAP_ENVS:
            r = query(L, facts(slip=slip), env, extra)
            rows.append("caps|%s|%s|%s" % (SLIP[slip], env_key(env), " ".join(str(r[k]) for k in CAP_FIELDS)))
    return rows


def parse(lines):
    """{ (kind, facts, environment): { field: value } } of table lines"""
    out = {}
    for ln in lines:
        kind, f, env, vals = ln.rstrip("\n").split("|")
        names = ROUTE_FIELDS if kind == "routes" else CAP_FIELDS
        v = [int(c) for c in vals] if kind == "routes" else [int(x) for x in vals.split()]
        assert len(v) == len(names), ln
        out[(kind, f, env)] = dict(zip(names, v))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--root", default=HERE)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import exaconstit_amd.lib as L
    text = "\n".join(table(L)) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
