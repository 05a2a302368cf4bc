#!/usr/bin/env python3
"""TreeSHAP contribution benchmark (csrc/gbdt_shap.hip), 1xMI355X.

    python tools/gbdt_shap_bench.py [reference|synthetic] [--out profiles/r9/gbdt_shap_bench.jsonl]

Two shapes, one JSON line each (appended to --out):
  * ``reference``: the reference configuration (500 rounds x 62 boosters, depth 3, gamma 1) fitted on the
    reference-sized draw history, its validation rows scored;
  * ``synthetic``: 50 rounds x 62 boosters on the 262 145-draw synthetic set, its 183k training rows scored.
Per shape: the kernel-only time of em_gbdt_shap (device events around warm back-to-back launches over all row
chunks, >= --window seconds), the wall time of ``predict_contribs`` (binning, launches, device-to-host copy of the
[n, 62, F+1] result), the numpy path on the same box (on at most --numpy-rows rows: its rows/s is what compares),
the kernel's VALU-issue bound from the instruction count of its per-leaf blocks, and the largest
|kernel - numpy| on the rows both scored.  No threshold: there is no earlier implementation to compare with.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# VALU instructions of one leaf with d distinct path features in gbdt_shap<3> (`hipcc -S` of csrc/gbdt_shap.hip,
# the v_* instructions of the block of each `case d`), per lane = per row
VALU_PER_LEAF = {1: 7, 2: 22, 3: 51}
# full-rate VALU issue: 256 CUs x 4 SIMDs, one wave64 instruction per 2 cycles per SIMD, 2.4 GHz
LANE_OPS_PER_S = 256 * 4 * 2.4e9 / 2 * 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", nargs="?", default=None, choices=[None, "reference", "synthetic"])
    ap.add_argument("--window", type=float, default=0.5, help="seconds of kernel launches per timed window")
    ap.add_argument("--numpy-rows", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gbdt_shap_bench measures on the GPU"
    from euromillioner_amd import config as C
    from euromillioner_amd.data.draws import DrawSet
    from euromillioner_amd.models import gbdt_explain as E
    from euromillioner_amd.models import gbdt_hip as H
    from euromillioner_amd.models.gbdt import GBDT
    from euromillioner_amd.ops import _native as N
    from euromillioner_amd.pipeline import gbdt_dataset

    cfg = C.RunConfig()
    ok = True
    for name, n_draws, rounds, train_rows in (("reference", None, 500, False), ("synthetic", 262145, 50, True)):
        if a.case and a.case != name:
            continue
        ds = DrawSet.synthetic(n=n_draws, seed=0, planted=0.5)
        X, Y, _ = gbdt_dataset(ds, cfg)
        m = int(0.7 * len(X))
        g = GBDT.from_params(cfg.gbdt_params(), nround=rounds, backend="hip").fit(X[:m], Y[:m])
        Xs = X[:m] if train_rows else X[m:]
        n, F, T = len(Xs), X.shape[1], g.n_tasks

        # ---- the launches predict_contribs makes, on resident bins: kernel-only time
        cuts, dtrees, _ = H._explain_plan(g, need_lds=True)
        tables = H._shap_tables(g, dtrees, F)
        dev = dtrees[0].device
        chunk = max(256, H.SHAP_CHUNK_BYTES // (T * (F + 1) * 4) // 256 * 256)
        d_bins = torch.from_numpy(H._bins_for(g, Xs, cuts, F)).to(dev)
        d_out = torch.empty((T, min(chunk, n), F + 1), dtype=torch.float32, device=dev)
        bias = torch.empty(T, dtype=torch.float32, device=dev)
        stream = N.stream_handle(dev)

        def launch_all():
            for r0 in range(0, n, chunk):
                r1 = min(n, r0 + chunk)
                N.call("em_gbdt_shap", d_bins[r0:r1].data_ptr(), r1 - r0, F, T, g.trees.max_depth, g.trees.n_trees, 0,
                       g.trees.n_trees, float(g.base_margin), *(t.data_ptr() for t in tables), bias.data_ptr(),
                       d_out.data_ptr(), stream)

        def timed(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                launch_all()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / reps

        timed(2)  # warm-up
        reps = max(3, int(np.ceil(a.window / timed(2))))
        ks = [timed(reps) for _ in range(5)]
        med = float(np.median(ks))

        # ---- end to end, and the numpy path on a slice of the same rows
        g.predict_contribs(Xs[:256])
        t0 = time.perf_counter()
        dev_phi = g.predict_contribs(Xs)
        e2e = time.perf_counter() - t0
        nn = min(n, a.numpy_rows)
        t0 = time.perf_counter()
        np_phi = E.contribs_numpy(g, Xs[:nn])
        np_s = time.perf_counter() - t0
        diff = float(np.abs(dev_phi[:nn].astype(np.float64) - np_phi).max())
        add = float(np.abs(dev_phi[:nn].astype(np.float64).sum(axis=2) - g.predict_margin(Xs[:nn], backend="numpy")).max())

        # ---- VALU-issue bound: every row runs every leaf block of its task's trees
        paths = E.build_paths(g.trees.status, g.trees.feat, g.trees.sbin, g.trees.leaf, g.trees.cover, g.trees.max_depth)
        hist = np.bincount(paths.d, minlength=4)
        valu_per_row = float(sum(VALU_PER_LEAF[d] * int(hist[d]) for d in (1, 2, 3)))  # all 62 tasks of one row
        bound = n * valu_per_row / LANE_OPS_PER_S
        out = {"metric": "TreeSHAP contributions (em_gbdt_shap)", "case": name, "rows": n, "features": F, "tasks": T,
               "rounds": rounds, "trees": g.trees.n_trees, "leaves": int(len(paths.d)),
               "leaves_by_path_features": hist.tolist(), "chunk_rows": chunk, "launches_per_window": reps,
               "kernel_s_median": med, "kernel_s_min_max": [min(ks), max(ks)], "kernel_rows_per_s": n / med,
               "predict_contribs_s": e2e, "predict_contribs_rows_per_s": n / e2e,
               "numpy_rows": nn, "numpy_s": np_s, "numpy_rows_per_s": nn / np_s,
               "kernel_over_numpy_rows_per_s": (n / med) / (nn / np_s),
               "valu_per_row": valu_per_row, "valu_issue_bound_s": bound, "share_of_valu_issue_bound": bound / med,
               "max_abs_kernel_minus_numpy": diff, "max_abs_sum_minus_margin": add}
        ok = ok and diff < 1e-4 and add < 1e-4
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a", encoding="utf-8") as f:
                f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
