#!/usr/bin/env python3
"""Forest TreeSHAP benchmark (csrc/forest_shap.hip) on the README forest, 1xMI355X.

    python tools/rf_shap_bench.py [--out profiles/r11/rf_shap_bench.jsonl]

100 trees of depth 8 over F = 62 fitted on 700k synthetic planted draws; the 300k validation rows are explained.
One JSON line (appended to --out):

* ``em_rf_shap`` kernel-only over all the validation rows: device events around windows of warm back-to-back
  passes (one pass = every row chunk once, into one resident output buffer; the full output would be 4.7 GB);
* ``RandomForest.predict_contribs`` end to end from host rows (uploads, launches, the 15.6 KB per row copy back);
* the numpy path on ``--numpy-rows`` rows (its rows/s is what compares) and the largest |kernel - numpy| there;
* the alternative that exists without this kernel, alternated window by window on the same ``--ab-rows`` rows:
  the forest recast as 62 x T single-output trees (``TreeArrays.from_arrays``, status 1 / 2, ``sbin`` 0, bits as
  bins, leaves / T) through ``em_gbdt_shap``, kernel-only the same way, and the largest difference of the two
  results; then the same pair through the public calls ``RandomForest.predict_contribs`` and
  ``GBDT.predict_contribs`` end to end from host rows.  No ratio is asserted.

``--kernel-only`` stops after the kernel windows (``rocprofv3`` runs; A/B of a side library built by
``tools/build_variant.sh`` with ``FILE=csrc/forest_shap.hip ... -DRS_WAVES=n``, run under ``EUROM_NATIVE_LIB`` with
``--label``); ``--occupancy-probe`` adds the kernel at 10, 5 and 2 waves per CU.
"""
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


def recast_gbdt(rf, leaves):
    """The forest as a 62-task GBDT of T rounds: tree 62 t + o is tree t with the scalar leaves value[:, o] / T."""
    from euromillioner_amd.models.gbdt import GBDT, TreeArrays

    T, NN = rf.feat.shape
    status1 = np.where(rf.feat >= 0, 1, 0).astype(np.int8)
    status1[leaves] = 2
    reach = status1 > 0  # (splits below an unreachable node do not occur in a fitted forest)
    status = np.repeat(np.where(reach, status1, 0).astype(np.int8), 62, axis=0)
    feat = np.repeat(np.maximum(rf.feat, 0).astype(np.int32), 62, axis=0)
    leaf = (rf.value[:, :, :62].astype(np.float64) / T).transpose(0, 2, 1).reshape(T * 62, NN)
    cover = np.repeat(rf.cover.astype(np.float64), 62, axis=0)
    tr = TreeArrays.from_arrays(rf.max_depth, status, feat, np.zeros_like(feat), np.ascontiguousarray(leaf),
                                np.zeros_like(cover), cover)
    tr.split_value = np.where(status == 1, 0.5, 0.0)  # bit 0 < 0.5 goes left, bit 1 right
    g = GBDT(objective="reg:squarederror", max_depth=rf.max_depth, nround=T, base_score=0.0, backend="hip")
    g.trees, g.n_tasks, g.num_feature, g.backend_used = tr, 62, rf.F, "hip"
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-rows", type=int, default=700_000)
    ap.add_argument("--rows", type=int, default=300_000, help="validation rows explained")
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--planted", type=float, default=0.9)
    ap.add_argument("--chunk-rows", type=int, default=16384)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--passes", type=int, default=1, help="passes over all rows per timed window")
    ap.add_argument("--ab-rows", type=int, default=16384, help="rows of the alternated comparison with the recast GBDT")
    ap.add_argument("--ab-windows", type=int, default=3)
    ap.add_argument("--numpy-rows", type=int, default=128)
    ap.add_argument("--kernel-only", action="store_true",
                    help="only the em_rf_shap windows (for rocprofv3 runs and A/B builds: no numpy path, no recast GBDT)")
    ap.add_argument("--label", default=None, help="'variant' key of the output line (A/B builds, EUROM_NATIVE_LIB)")
    ap.add_argument("--occupancy-probe", action="store_true",
                    help="with --kernel-only: the same forest declared over 124 and 248 features (two and four row "
                         "words, the added ones zero), which changes nothing but the LDS per wave and so the waves a "
                         "CU holds: floor(160 KiB / (260 F bytes)) = 10, 5 and 2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rf_shap_bench needs a GPU: a timing taken anywhere else says nothing about it")
    from euromillioner_amd.data.draws import mask_bits
    from euromillioner_amd.data.synthetic import generate_draws
    from euromillioner_amd.models import forest_explain as E
    from euromillioner_amd.models import gbdt_hip as H
    from euromillioner_amd.models.forest import RandomForest, n_candidates, unpack_bits
    from euromillioner_amd.ops import _native as N
    from euromillioner_amd.ops import forest as K

    total = a.train_rows + a.rows
    nums, _ = generate_draws(total + 1, seed=0, planted=a.planted, native=True)
    m = mask_bits(nums)
    dev = torch.device("cuda")
    md = torch.from_numpy(m.view(np.int64)).to(dev)
    Xd, Yd = md[:total].reshape(-1, 1).contiguous(), md[1:total + 1].contiguous()
    k = n_candidates("sqrt", 62)
    rf = RandomForest(a.trees, a.depth, 1, "sqrt", True, 0, "cuda")
    rf.F, rf.k, rf.n_train = 62, k, a.train_rows
    rf.feat, rf.value, rf.gain, rf.cover = K.fit(Xd[:a.train_rows], Yd[:a.train_rows], 62, 0, a.trees, a.depth, k, 1,
                                                 True, 0)
    Xv = Xd[a.train_rows:total].contiguous()
    Xh = m[a.train_rows:total].reshape(-1, 1).copy()
    n = a.rows
    tables = rf._shap_tables()
    paths = E.paths_of(rf)
    chunk = min(a.chunk_rows, n)
    buf = torch.empty(chunk, 62, 63, dtype=torch.float32, device=dev)

    def one_pass(rows=n):
        for r0 in range(0, rows, chunk):
            r1 = min(rows, r0 + chunk)
            K.shap(Xv[r0:r1], tables, out=buf[:r1 - r0])

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    one_pass(min(n, chunk))  # warm-up: code object, LDS attribute, clocks
    torch.cuda.synchronize()
    ks = [timed(one_pass, a.passes) for _ in range(a.windows)]
    med = statistics.median(ks)
    def emit(res):
        if a.label:
            res = {"variant": a.label, **res}
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a", encoding="utf-8") as f:
                f.write(line + "\n")

    if a.kernel_only:
        res = {"metric": "forest TreeSHAP contributions (em_rf_shap), kernel only", "rows": n,
               "leaves": int(len(paths.d)), "chunk_rows": chunk, "kernel_s_median": med,
               "kernel_s_min_max": [min(ks), max(ks)], "kernel_rows_per_s": n / med}
        if a.occupancy_probe:
            probe = {}
            for Fp in (62, 124, 248):
                W = (Fp + 63) // 64
                tp = K.ShapTables(tables.T, tables.L, tables.max_depth, Fp, tables.pd, tables.pf, tables.pz,
                                  tables.pval, tables.bias)
                Xp = torch.zeros(chunk, W, dtype=torch.int64, device=dev)
                Xp[:, 0] = Xv[:chunk, 0]
                bp = torch.empty(chunk, 62, Fp + 1, dtype=torch.float32, device=dev)
                K.shap(Xp, tp, out=bp)
                torch.cuda.synchronize()
                same = bool(torch.equal(bp[:, :, :62], buf_first)) if Fp > 62 else None
                if Fp == 62:
                    buf_first = bp[:, :, :62].clone()
                ts = [timed(lambda: K.shap(Xp, tp, out=bp), 1) for _ in range(max(3, a.windows))]
                probe[str(Fp)] = {"lds_bytes_per_wave": 260 * Fp, "waves_per_cu_by_lds": (160 * 1024) // (260 * Fp),
                                  "rows": chunk, "kernel_s_median": statistics.median(ts),
                                  "kernel_s_min_max": [min(ts), max(ts)], "features_equal_to_F62": same}
                del bp
            res["occupancy_probe"] = probe
        emit(res)
        return 0

    # ---- end to end from host rows, and the numpy path on a slice of them
    rf.predict_contribs(Xh[:256])
    t0 = time.perf_counter()
    e2e_rows = min(n, 2 * chunk)  # (the host result of all 300k rows would be 4.7 GB)
    dev_phi = rf.predict_contribs(Xh[:e2e_rows], chunk_rows=chunk)
    e2e = time.perf_counter() - t0
    nn = min(n, a.numpy_rows)
    t0 = time.perf_counter()
    np_phi = E.contribs_numpy(rf, Xh[:nn])
    np_s = time.perf_counter() - t0
    diff = float(np.abs(dev_phi[:nn].astype(np.float64) - np_phi).max())
    add = float(np.abs(dev_phi[:nn].astype(np.float64).sum(axis=2) - rf.predict_proba(Xh[:nn])).max())

    # ---- the recast GBDT on the same rows, alternated
    ab = min(n, a.ab_rows, chunk)
    g = recast_gbdt(rf, E.leaf_mask(rf.feat))
    cuts, dtrees, _ = H._explain_plan(g, need_lds=True)
    gt = H._shap_tables(g, dtrees, 62)
    bins = torch.from_numpy(np.ascontiguousarray(unpack_bits(Xh[:ab], 62).astype(np.uint8))).to(dev)
    g_out = torch.empty(62, ab, 63, dtype=torch.float32, device=dev)
    g_bias = torch.empty(62, dtype=torch.float32, device=dev)
    st = N.stream_handle(dev)

    def run_gbdt():
        N.call("em_gbdt_shap", bins.data_ptr(), ab, 62, 62, a.depth, g.trees.n_trees, 0, g.trees.n_trees, 0.0,
               *(t.data_ptr() for t in gt), g_bias.data_ptr(), g_out.data_ptr(), st)

    def run_rf():
        K.shap(Xv[:ab], tables, out=buf[:ab])

    run_gbdt(), run_rf()
    torch.cuda.synchronize()
    ab_diff = float((g_out.permute(1, 0, 2) - buf[:ab]).abs().max())
    ab_rf, ab_gb = [], []
    for _ in range(a.ab_windows):
        ab_rf.append(timed(run_rf, 1))
        ab_gb.append(timed(run_gbdt, 1))
    # ---- the same comparison through the public calls, end to end from host rows (binning / upload, launches,
    # the copy back of the [ab, 62, 63] result), each after one warm call
    Xf = unpack_bits(Xh[:ab], 62).astype(np.float64)
    g.predict_contribs(Xf[:256], backend="hip")
    pub_rf, pub_gb = [], []
    for _ in range(a.ab_windows):
        t0 = time.perf_counter()
        rp = rf.predict_contribs(Xh[:ab], backend="hip", chunk_rows=ab)
        pub_rf.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        gp = g.predict_contribs(Xf, backend="hip", chunk_rows=ab)
        pub_gb.append(time.perf_counter() - t0)
    pub_diff = float(np.abs(gp - rp).max())
    hist = np.bincount(paths.d, minlength=a.depth + 1)
    res = {"metric": "forest TreeSHAP contributions (em_rf_shap)", "rows": n, "train_rows": a.train_rows,
           "trees": a.trees, "max_depth": a.depth, "features": 62, "leaves": int(len(paths.d)),
           "leaves_by_path_features": hist.tolist(), "chunk_rows": chunk, "windows": a.windows,
           "passes_per_window": a.passes, "kernel_s_median": med, "kernel_s_min_max": [min(ks), max(ks)],
           "kernel_rows_per_s": n / med, "predict_contribs_rows": e2e_rows, "predict_contribs_s": e2e,
           "predict_contribs_rows_per_s": e2e_rows / e2e, "numpy_rows": nn, "numpy_s": np_s,
           "numpy_rows_per_s": nn / np_s, "kernel_over_numpy_rows_per_s": (n / med) / (nn / np_s),
           "max_abs_kernel_minus_numpy": diff, "max_abs_sum_minus_proba": add,
           "ab_rows": ab, "ab_em_rf_shap_s": {"median": statistics.median(ab_rf), "min": min(ab_rf), "max": max(ab_rf)},
           "ab_recast_em_gbdt_shap_s": {"median": statistics.median(ab_gb), "min": min(ab_gb), "max": max(ab_gb)},
           "recast_gbdt_over_rf_shap": statistics.median(ab_gb) / statistics.median(ab_rf),
           "max_abs_rf_shap_minus_recast_gbdt": ab_diff,
           "ab_rf_predict_contribs_s": {"median": statistics.median(pub_rf), "min": min(pub_rf), "max": max(pub_rf)},
           "ab_recast_gbdt_predict_contribs_s": {"median": statistics.median(pub_gb), "min": min(pub_gb),
                                                 "max": max(pub_gb)},
           "recast_gbdt_over_rf_predict_contribs": statistics.median(pub_gb) / statistics.median(pub_rf),
           "max_abs_predict_contribs_difference": pub_diff}
    emit(res)
    return 0 if diff < 1e-4 and add < 1e-4 and ab_diff < 1e-4 and pub_diff < 1e-4 else 1


if __name__ == "__main__":
    sys.exit(main())
