#!/usr/bin/env python3
"""Count-table kernels (csrc/draw_counts.hip) against the same results from PyTorch ops, 1xMI355X.

    python tools/count_table_bench.py [--log2-draws 24,28] [--lags 1] [--windows 5] [--launches 10]
                                      [--out profiles/r16/count_table_bench.jsonl]

For every size, on device-generated draws (``generate_masks``, planted 0.9):

* ``em_pair_counts`` (lag 1) over all samples, device events around windows of ``--launches`` back-to-back launches
  after a warm-up; per-launch median and min / max over the windows;
* the same counts from PyTorch ops: 0/1 float32 bit matrices of a chunk of source and target masks and one matmul
  per chunk (exact: a chunk's counts stay below 2^24), summed in int64.  Kernel and PyTorch windows alternate;
* ``em_count_logits`` over all samples into one reused buffer of at most 2^24 rows (a pass is several launches at
  2^28), and the PyTorch form: the 0/1 float32 lag window times the table plus the prior, chunked the same way;
* each kernel as a share of the streaming rate: 8 bytes per sample for the counts, 264 for the logits (8 read,
  256 written), against a device-to-device copy of 1 GiB timed in the same command (bytes read + written).

The outputs of both sides are compared before anything is timed (counts exactly; the logits of the PyTorch form,
whose additions run in another order, within 1e-4).  One JSON line per size, printed and appended to ``--out``.
These are records, not pass criteria.  Note that 2^24 masks (128 MiB) fit in the 256 MiB Infinity Cache."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-draws", default="24,28")
    ap.add_argument("--lags", type=int, default=1)
    ap.add_argument("--planted", type=float, default=0.9)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--torch-passes", type=int, default=1, help="PyTorch passes per window (they are slow)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from euromillioner_amd.data.device_gen import generate_masks
    from euromillioner_amd.models.count_table import CountTable
    from euromillioner_amd.ops import draw_counts as DC

    if not torch.cuda.is_available():
        raise SystemExit("count_table_bench needs a GPU: a timing taken anywhere else says nothing about it")
    dev = torch.device("cuda")
    lags = a.lags
    shifts = torch.arange(62, dtype=torch.int64, device=dev)

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def alternate(kernel, torch_form):
        """Per-call ms of both, their windows alternating after a warm-up of each."""
        for _ in range(3):
            kernel()
        torch_form()
        torch.cuda.synchronize()
        k, t = [], []
        for _ in range(a.windows):
            k.append(window(kernel, a.launches))
            t.append(window(torch_form, a.torch_passes))
        return ({"median_ms": statistics.median(k), "min_ms": min(k), "max_ms": max(k)},
                {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)})

    # streaming yardstick: a 1 GiB device-to-device copy (reads + writes 2 GiB)
    src = torch.empty(1 << 28, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    torch.cuda.synchronize()
    copy_ms = statistics.median(window(lambda: dst.copy_(src), 10) for _ in range(a.windows))
    stream_gbs = 2 * src.numel() * 4 / (copy_ms * 1e-3) / 1e9
    del src, dst

    rows = []
    for lg2 in [int(v) for v in a.log2_draws.split(",") if v]:
        n = 1 << lg2
        masks = generate_masks(n, seed=0, planted=a.planted, device=dev)
        S = n - lags  # samples
        chunk = min(S, 1 << 20)
        out_c = torch.empty(64, 64, dtype=torch.int64, device=dev)

        def counts_kernel():
            DC.pair_counts(masks, 1, 0, n - 1, out=out_c)

        keep = {}

        def bits_of(m):
            return ((m[:, None] >> shifts[None, :]) & 1).to(torch.float32)

        def counts_torch():
            C = torch.zeros(62, 62, dtype=torch.int64, device=dev)
            for c0 in range(0, n - 1, chunk):
                c1 = min(n - 1, c0 + chunk)
                C += (bits_of(masks[c0:c1]).T @ bits_of(masks[c0 + 1:c1 + 1])).to(torch.int64)
            keep["C"] = C

        counts_kernel()
        counts_torch()
        if not torch.equal(out_c[:62, :62], keep["C"]) or bool(out_c[62:].any()) or bool(out_c[:, 62:].any()):
            raise SystemExit(f"2^{lg2}: em_pair_counts differs from the PyTorch counts")
        ck, ct = alternate(counts_kernel, counts_torch)

        model = CountTable(lags, 1.0, "cuda").fit_draw_masks(masks, 0, S)
        table, prior = model._device_weights(dev)
        rows_per = min(S, 1 << 24)
        buf = torch.empty(rows_per, 64, dtype=torch.float32, device=dev)
        W = table[:, :62, :].reshape(lags * 62, 64).contiguous()

        def logits_kernel():
            for c0 in range(0, S, rows_per):
                DC.count_logits(masks, min(rows_per, S - c0), table, prior, offset=c0, out=buf)

        lchunk = min(S, 1 << 21)
        tbuf = torch.empty(lchunk, 64, dtype=torch.float32, device=dev)

        def logits_torch_chunk(c0, c1):
            X = torch.cat([bits_of(masks[c0 + k:c1 + k]) for k in range(lags - 1, -1, -1)], dim=1)  # k = 1 first
            return torch.addmm(prior, X, W, out=tbuf[:c1 - c0])

        def logits_torch():
            for c0 in range(0, S, lchunk):
                logits_torch_chunk(c0, min(S, c0 + lchunk))

        DC.count_logits(masks, min(lchunk, S), table, prior, offset=0, out=buf)
        ref = logits_torch_chunk(0, min(lchunk, S))
        err = float((buf[:ref.shape[0], :62] - ref[:, :62]).abs().max())
        if not err <= 1e-4:
            raise SystemExit(f"2^{lg2}: em_count_logits differs from the PyTorch logits by {err}")
        lk, lt = alternate(logits_kernel, logits_torch)

        row = {"metric": "count-table kernels vs PyTorch ops", "log2_draws": lg2, "draws": n, "lags": lags,
               "planted": a.planted, "windows": a.windows, "launches_per_window": a.launches,
               "torch_passes_per_window": a.torch_passes, "copy_1gib_ms": copy_ms, "stream_gb_per_s": stream_gbs,
               "em_pair_counts": ck, "torch_pair_counts": ct,
               "pair_counts_gsamples_per_s": (n - 1) / (ck["median_ms"] * 1e-3) / 1e9,
               "pair_counts_share_of_stream": 8 * (n - 1) / (ck["median_ms"] * 1e-3) / 1e9 / stream_gbs,
               "pair_counts_torch_over_kernel": ct["median_ms"] / ck["median_ms"],
               "em_count_logits": lk, "torch_count_logits": lt, "logits_max_abs_diff_vs_torch": err,
               "count_logits_gsamples_per_s": S / (lk["median_ms"] * 1e-3) / 1e9,
               "count_logits_share_of_stream": 264 * S / (lk["median_ms"] * 1e-3) / 1e9 / stream_gbs,
               "count_logits_torch_over_kernel": lt["median_ms"] / lk["median_ms"]}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del masks, buf, tbuf
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a", encoding="utf-8") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
