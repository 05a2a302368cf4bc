#!/usr/bin/env python3
"""The kernel dispatch sequence of ``em_gbdt_fit``, one tiny fit per branch of its plan table (``FitPlan`` in
csrc/gbdt.hip), for comparing two builds of the driver: a host-side change must leave it equal line for line.

    rocprofv3 --kernel-trace --output-format csv -d A -o run -- python tools/gbdt_launch_trace.py run
    EUROM_NATIVE_LIB=<other build> rocprofv3 --kernel-trace --output-format csv -d B -o run -- \
        python tools/gbdt_launch_trace.py run
    python tools/gbdt_launch_trace.py compare A B [KERNEL ...]

``run`` fits the cases in one process (each printed with a hash of its six tree arrays) and puts a marker -- three
one-block ``gbdt_init_margin`` launches -- in front of each.  ``compare`` reads the two traces, keeps the ``gbdt_``
kernels in dispatch order as (name without its parameter list, grid, workgroup, LDS bytes), splits them at the
markers and prints the dispatch count per case and "identical" or the first difference; exit status 1 if any case
differs.  The trace's LDS bytes are the kernel's static LDS rounded up to 512 (the launch's dynamic LDS is not in
it): for a KERNEL named after the two directories, whose device code changed between the builds, that column is
left out of the comparison and its (A, B) values are printed instead."""
from __future__ import annotations

import csv
import functools
import glob
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

# (label, case of tests/_gbdt_fit_cases.py, driver, watch sets, eval_metric, rounds_per_call)
CASES = [
    *[(f"std-logistic 2 sets {d}", "std-logistic", d, 2, None, None) for d in ("default", "separate")],
    ("std-softprob", "std-softprob", "default", 0, None, None),
    ("softprob merror 2 sets", "std-softprob", "default", 2, "merror", None),
    ("std-logistic 5 sets", "std-logistic", "default", 5, None, None),
    ("quant-mixed-logistic", "quant-mixed-logistic", "default", 0, None, None),
    ("quant-cont-logistic", "quant-cont-logistic", "default", 0, None, None),
    ("depth-1", "depth-1", "default", 0, None, None),
    ("depth-9", "depth-9", "default", 0, None, None),
    ("rows-257", "rows-257", "default", 0, None, None),
    ("rows-8448", "rows-8448", "default", 0, None, None),
    ("sub-0.8-rounds7 rounds_per_call 3", "sub-0.8-rounds7", "default", 0, None, 3),
]
TREE_ARRAYS = ("status", "feat", "sbin", "leaf", "gain", "cover")


def run():
    import numpy as np
    import torch

    import _gbdt_fit_cases as K
    import _gbdt_watch_data as D
    from euromillioner_amd.models import gbdt as G
    from euromillioner_amd.models import gbdt_hip
    from euromillioner_amd.ops import _native as N

    dev = torch.device("cuda", torch.cuda.current_device())
    mark = torch.empty(1, dtype=torch.float32, device=dev)
    whole_fit = gbdt_hip.fit
    for label, case, driver, n_sets, metric, per_call in CASES:
        dn, objective, kw = K.CASES[case]
        X, Y, _ = K.data(dn)
        evals = None
        if n_sets:  # the standard problems are the `train` set of the watch data
            sets = D.problem(objective)
            assert sets["train"][0] is X or np.array_equal(sets["train"][0], X)
            evals = D.watch(sets, n_sets)
        g = G.GBDT(objective=objective, backend="hip", **dict(kw, **({"eval_metric": metric} if metric else {})))
        g.separate_launches = driver == "separate"
        for _ in range(3):
            N.call("em_gbdt_init_margin", mark.data_ptr(), 1, 0.0, N.stream_handle(dev))
        gbdt_hip.fit = functools.partial(whole_fit, rounds_per_call=per_call) if per_call else whole_fit
        try:
            g.fit(X, Y, evals=evals)
        finally:
            gbdt_hip.fit = whole_fit
        assert g.backend_used == "hip"
        h = hashlib.sha256(b"".join(np.ascontiguousarray(getattr(g.trees, k)).tobytes() for k in TREE_ARRAYS))
        print(json.dumps({"case": label, "trees": g.trees.n_trees, "trees_sha16": h.hexdigest()[:16]}), flush=True)
    torch.cuda.synchronize()


def dispatches(trace_dir):
    """[(name, grid, workgroup, lds)] of the gbdt_ kernels of a rocprofv3 kernel trace, in dispatch order."""
    paths = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if len(paths) != 1:
        raise SystemExit(f"{trace_dir}: expected one *kernel_trace.csv, found {paths}")
    rows = list(csv.DictReader(open(paths[0])))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    dims = lambda r, stem: tuple(int(r[k]) for k in sorted(r) if k.startswith(stem))  # noqa: E731
    # (the kernel's name with its template arguments, without the parameter list: a build that drops a kernel
    # parameter still compares)
    return [(m.group(0), dims(r, "Grid_Size"), dims(r, "Workgroup_Size"), int(r["LDS_Block_Size"]))
            for r in rows for m in [re.search(r"gbdt_\w+(<[^>]*>)?", r["Kernel_Name"])] if m]


def per_case(seq):
    """The sequence split at the markers (three consecutive one-block gbdt_init_margin dispatches)."""
    def is_mark(d):
        return "gbdt_init_margin" in d[0] and d[1] == d[2]

    out, i = [], 0
    while i < len(seq):
        if i + 2 < len(seq) and all(is_mark(seq[i + k]) for k in range(3)):
            out.append([])
            i += 3
            continue
        if not out:
            raise SystemExit("trace does not start with a marker")
        out[-1].append(seq[i])
        i += 1
    return out


def compare(dir_a, dir_b, lds_changed=()):
    sa, sb = dispatches(dir_a), dispatches(dir_b)
    if lds_changed:
        pairs = sorted({(x[0], x[3], y[3]) for x, y in zip(sa, sb) if x[0] == y[0] and x[0] in lds_changed})
        print("static LDS not compared (A, B):", ", ".join(f"{k} ({la}, {lb})" for k, la, lb in pairs))
        sa, sb = ([d[:3] + (None,) if d[0] in lds_changed else d for d in s] for s in (sa, sb))
    a, b = per_case(sa), per_case(sb)
    bad = len(a) != len(CASES) or len(b) != len(CASES)
    if bad:
        print(f"cases: {len(a)} and {len(b)} traced, {len(CASES)} expected")
    total = 0
    for (label, *_), da, db in zip(CASES, a, b):
        first = next((i for i, (x, y) in enumerate(zip(da, db)) if x != y), None)
        if first is None and len(da) != len(db):
            first = min(len(da), len(db))
        total += len(da)
        if first is None:
            print(f"{label}: {len(da)} dispatches, identical")
        else:
            bad = True
            print(f"{label}: {len(da)} vs {len(db)} dispatches, first difference at {first}: "
                  f"{da[first] if first < len(da) else None} vs {db[first] if first < len(db) else None}")
    print(f"total: {total} dispatches in {len(a)} cases, {'DIFFERENT' if bad else 'identical'}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4:]))
    else:
        raise SystemExit(__doc__)
