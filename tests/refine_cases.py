"""What the refinement's CPU and GPU tests share: the fixtures' settings with the counts measured for them, the restatement
driven by the CPU oracle (computed once a session and left unchanged), and the loader of a tool's module."""
import importlib.util
import os
import sys

import numpy as np

from conftest import ROOT, case_kwargs, case_positions
import refine_reference as rr

# (fixture, method or None for the fixture's, poses, iterations, (trans A, rot rad, nm extents), max_halvings,
#  K, accepted, halvings, frozen, evaluations)
TABLE = [
    ("1ppe", None, 24, 8, (1.0, 0.1, 0.5), 3, 12, 125, 54, 8, 2268),
    ("1ppe", None, 24, 12, (8.0, 1.0, 0.5), 2, 12, 75, 48, 24, 1788),
    ("1k4c", None, 8, 4, (1.0, 0.1, 0.5), 3, 12, 22, 10, 0, 392),
    ("2uuy", None, 8, 4, (1.0, 0.1, 0.5), 3, 52, 31, 1, 0, 1672),
    ("2uuy", None, 8, 8, (4.0, 0.5, 2.0), 1, 52, 55, 6, 1, 3232),
    ("1azp", None, 12, 6, (1.0, 0.1, 0.5), 3, 52, 72, 0, 0, 3756),
    ("1azp", None, 12, 10, (4.0, 0.5, 2.0), 1, 52, 118, 1, 1, 6252),
    ("1azp", "pydock", 12, 6, (1.0, 0.1, 0.5), 3, 52, 72, 0, 0, 3756),
]
MIN_GAP = 1e-5
TABLE_IDS = ["%s-%s-%dit-%g" % (r[0], r[1] or "own", r[3], r[4][0]) for r in TABLE]


def oracle_refinement(orc, table, row, cache={}):
    """The restatement driven by the oracle for one row of TABLE, computed once a session (the GPU tests share it)."""
    if row not in cache:
        name, method, n, iterations, steps, max_halvings = row[:6]
        own, rec, lig, kw = case_kwargs(name, orc, table)
        cpu = orc.Scorer(method or own, rec, lig, **kw)
        poses = np.ascontiguousarray(case_positions(name, orc)[:n])
        threads = min(8, os.cpu_count() or 1)
        cache[row] = (poses, rr.refine(orc.q_mul, lambda rows: cpu.energy_rows_mt(rows, threads), poses, poses.shape[1], iterations,
                                       max_halvings, *steps))
    return cache[row]


def tool_module(name):
    """lightdock-rust_amd/<name>.py as the module lightdock_rust_amd.<name>, its directory on sys.path while it loads."""
    tools = os.path.join(ROOT, "lightdock-rust_amd")
    spec = importlib.util.spec_from_file_location("lightdock_rust_amd." + name, os.path.join(tools, name + ".py"))
    sys.path.insert(0, tools)
    try:
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.pop(0)
    return mod
