#!/usr/bin/env python3
"""Out-of-bag evaluation benchmark (700k rows x 100 trees x depth 8 on the synthetic planted set, 1xMI355X).

    python tools/rf_oob_bench.py [--rows 700000] [--trees 100] [--depth 8] [--windows 7] [--launches 100]

Times, on the training rows and trees of one device fit:

* ``em_rf_oob_predict`` and ``em_rf_predict`` (the yardstick: the existing kernel, same rows, same trees, both
  with their tree-image pass ``rf_predict_prepare``), kernel-only: device events around windows of
  ``--launches`` back-to-back launches into preallocated buffers, after a warm-up, the two entry points
  alternating window by window; per-launch medians and the min / max over the windows;
* ``em_rf_oob_metrics`` the same way;
* ``RandomForest.oob_score`` end to end from host arrays (uploads, both kernels, the partials' download), host
  clock around a call that ends in the download.

Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=700_000)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--subset", default="sqrt")
    ap.add_argument("--planted", type=float, default=0.9)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=3, help="end-to-end oob_score calls")
    a = ap.parse_args()
    from euromillioner_amd.data.draws import mask_bits
    from euromillioner_amd.data.synthetic import generate_draws
    from euromillioner_amd.models.forest import RandomForest, n_candidates
    from euromillioner_amd.ops import _native as N
    from euromillioner_amd.ops import forest as K

    if not torch.cuda.is_available():
        raise SystemExit("rf_oob_bench needs a GPU: a timing taken anywhere else says nothing about it")
    nums, _ = generate_draws(a.rows + 1, seed=0, planted=a.planted, native=True)
    m = mask_bits(nums)
    dev = torch.device("cuda")
    md = torch.from_numpy(m.view(np.int64)).to(dev)
    X, Y = md[:a.rows].reshape(-1, 1).contiguous(), md[1:a.rows + 1].contiguous()
    k = n_candidates(a.subset, 62)
    seed = 0
    feat, value, gain, cover = K.fit(X, Y, 62, 0, a.trees, a.depth, k, 1, True, seed, return_device=True)
    n, T = a.rows, a.trees
    out = torch.empty(n, 64, dtype=torch.float32, device=dev)
    out_p = torch.empty(n, 64, dtype=torch.float32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    nb = N.lib().em_rf_predict_scratch(1, T, a.depth)
    prep = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev) if nb > 0 else None
    pp = prep.data_ptr() if prep is not None else None
    part = torch.empty(N.query("em_rf_oob_metrics_words", n), dtype=torch.int64, device=dev)
    st = N.stream_handle(dev)

    def run_oob():
        N.call("em_rf_oob_predict", X.data_ptr(), 1, n, feat.data_ptr(), value.data_ptr(), T, a.depth, seed, 0,
               out.data_ptr(), 64, cnt.data_ptr(), pp, st)

    def run_predict():
        N.call("em_rf_predict", X.data_ptr(), 1, n, feat.data_ptr(), value.data_ptr(), T, a.depth, 0, out_p.data_ptr(),
               64, pp, st)

    def run_metrics():
        N.call("em_rf_oob_metrics", out.data_ptr(), 64, cnt.data_ptr(), Y.data_ptr(), n, part.data_ptr(), st)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.launches  # ms per launch

    for fn in (run_oob, run_predict, run_metrics):  # warm-up: code objects, LDS attribute, clocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {"oob": [], "predict": [], "metrics": []}
    for _ in range(a.windows):  # alternating, so drift and neighbours hit both alike
        ms["oob"].append(window(run_oob))
        ms["predict"].append(window(run_predict))
        ms["metrics"].append(window(run_metrics))

    def stat(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}

    rf = RandomForest(T, a.depth, 1, a.subset, True, seed, "cuda")
    rf.F, rf.k, rf.n_train, rf.tree_start = 62, k, n, 0
    rf.feat, rf.value, rf.gain, rf.cover = (t.cpu().numpy() for t in (feat, value, gain, cover))
    Xh, Yh = m[:n].reshape(-1, 1).copy(), m[1:n + 1].copy()
    e2e = []
    score = None
    for _ in range(1 + a.repeat):  # (the first call is dropped)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        score = rf.oob_score(Xh, Yh)
        e2e.append(time.perf_counter() - t0)
    res = {"metric": "random forest out-of-bag evaluation", "rows": n, "trees": T, "max_depth": a.depth,
           "k_features": k, "windows": a.windows, "launches_per_window": a.launches,
           "em_rf_oob_predict": stat(ms["oob"]), "em_rf_predict": stat(ms["predict"]),
           "em_rf_oob_metrics": stat(ms["metrics"]),
           "oob_over_predict": statistics.median(ms["oob"]) / statistics.median(ms["predict"]),
           "oob_score_end_to_end_s": min(e2e[1:]) if len(e2e) > 1 else e2e[0], "oob_score_first_call_s": e2e[0],
           "oob": score, "importances_top": [[int(f), float(rf.feature_importances("gain")[f])]
                                             for f in np.argsort(-rf.feature_importances("gain"), kind="stable")[:5]]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
