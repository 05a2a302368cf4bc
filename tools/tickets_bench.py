#!/usr/bin/env python3
"""Ticket sampling + prize-tier back-test benchmark (csrc/tickets.hip), 1xMI355X.

    python tools/tickets_bench.py [--rows 1048576] [--tickets 16] [--rounds 5] [--out profiles/r8/tickets_bench.jsonl]

On the logits of a briefly trained FusedSmallMLP, in ONE command:
  * kernel-only time of em_draw_tickets (scored, no ticket output), device events around enough back-to-back
    launches for a >= 0.5 s window, warm;
  * the same work as a plain PyTorch formulation on the same GPU (uniform -> Gumbel -> topk -> scatter to masks
    -> popcount -> tier counts), at the largest N <= --tickets whose [B, N, 62] temporaries fit;
  * the two alternated for --rounds rounds: per-round ratio and its spread;
  * end-to-end model.backtest() rows/s (logits() + kernel + partial sums on the host);
  * the kernel's scored output against the numpy specification on the first 4096 rows of the timed input.
Prints one JSON line (and appends it to --out).  There is no CPU path: without a GPU this fails.
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

# VALU instructions of one ticket's path through draw_tickets_kernel (T != 0, scored): `hipcc -S` of
# csrc/tickets.hip summed by tools/isa_stats.py --blocks over the blocks a sampling lane runs
VALU_PER_TICKET = 3056
# full-rate VALU issue: 256 CUs x 4 SIMDs, one wave64 instruction per 2 cycles per SIMD, 2.4 GHz
LANE_OPS_PER_S = 256 * 4 * 2.4e9 / 2 * 64


def _popcount64(x: torch.Tensor) -> torch.Tensor:
    x = x - ((x >> 1) & 0x5555555555555555)
    x = (x & 0x3333333333333333) + ((x >> 2) & 0x3333333333333333)
    x = (x + (x >> 4)) & 0x0F0F0F0F0F0F0F0F
    return (x * 0x0101010101010101) >> 56 & 0xFF


def torch_backtest(logits, masks, B, n, T, offset, rank_lut):
    """The baseline: the same sampling and scoring written in PyTorch ops (torch's own RNG)."""
    u = torch.rand(B, n, 62, device=logits.device).clamp_min_(2.0 ** -24)
    key = logits[:B, None, :62] / T - torch.log(-torch.log(u))
    im = key[..., :50].topk(5, dim=-1).indices
    ist = key[..., 50:].topk(2, dim=-1).indices + 50
    one = torch.ones((), dtype=torch.int64, device=logits.device)
    tk = (one << im).sum(-1) | (one << ist).sum(-1)
    hit = tk & masks[offset + 1:offset + 1 + B, None]
    cell = _popcount64(hit & ((1 << 50) - 1)) * 3 + _popcount64(hit >> 50)
    hist = torch.bincount(cell.reshape(-1), minlength=18)
    best = torch.bincount(rank_lut[cell].amin(1) - 1, minlength=14)
    return hist, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--tickets", type=int, default=16)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of kernel launches per timed window")
    ap.add_argument("--train-steps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tickets_bench measures on the GPU"
    from euromillioner_amd import tickets as TK
    from euromillioner_amd.data.device_gen import generate_masks
    from euromillioner_amd.models.mlp import FusedSmallMLP
    from euromillioner_amd.ops import _native as N
    from euromillioner_amd.ops import tickets as OT

    dev = torch.device("cuda")
    B, n, T, seed = a.rows, a.tickets, a.temperature, 7
    n_train = 1 << 20
    masks = generate_masks(n_train + B + 1, seed=0, planted=0.8, device=dev)
    model = FusedSmallMLP(dev, lr=3e-3)
    for s in range(a.train_steps):
        model.step(masks, 1 << 16, offset=(s * (1 << 16)) % (n_train - (1 << 16)))
    off = n_train
    logits = model.logits(masks, B, offset=off)
    torch.cuda.synchronize()

    part = torch.zeros(OT.ticket_blocks(B, n), 32, dtype=torch.int32, device=dev)
    stream = N.stream_handle(dev)

    def launch():
        N.call("em_draw_tickets", logits.data_ptr(), logits.stride(0), masks.data_ptr(), None, B, off, 0, n, float(T),
               seed, None, None, part.data_ptr(), stream)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    # ---- correctness on a slice of the timed input
    nv = min(4096, B)
    r = OT.draw_tickets(logits, nv, n, T, seed, masks=masks, offset=off)
    z = logits[:nv].cpu().numpy()
    k = TK.ticket_uniform_bits(seed, np.arange(off, off + nv), n)
    k64 = TK.keys_from_bits(z, k, T, np.float64)
    tol = 16.0 * float(np.abs(TK.keys_from_bits(z, k, T, np.float32).astype(np.float64) - k64).max())
    srt_m, srt_s = -np.sort(-k64[..., :50], -1), -np.sort(-k64[..., 50:], -1)
    near = ((srt_m[..., 4] - srt_m[..., 5]) < 2 * tol) | ((srt_s[..., 1] - srt_s[..., 2]) < 2 * tol)
    got = r["tickets"].cpu().numpy().view(np.uint64)
    spec = TK.tickets_from_keys(k64)
    targets = masks[off + 1:off + 1 + nv].cpu().numpy().view(np.uint64)
    hist, best = OT.sum_partials(r["partials"])
    h_own, b_own = TK.score_tickets_py(got, targets)
    h_spec, b_spec = TK.score_tickets_py(spec, targets)
    check = {"rows": nv, "near_pairs": int(near.sum()), "differ_outside_near": int(((got != spec) & ~near).sum()),
             "scored_equals_own_tickets": bool(np.array_equal(hist, h_own) and np.array_equal(best, b_own)),
             "hist_l1_vs_spec": int(np.abs(hist - h_spec).sum()), "best_l1_vs_spec": int(np.abs(best - b_spec).sum())}
    ok = (check["differ_outside_near"] == 0 and check["scored_equals_own_tickets"]
          and check["hist_l1_vs_spec"] <= 2 * check["near_pairs"] and check["best_l1_vs_spec"] <= 2 * check["near_pairs"])

    # ---- baseline size: the largest N <= n whose temporaries (about 6 [B, N, 62] fp32 tensors) fit in free HBM
    rank_lut = torch.from_numpy(TK.TIER_RANK.reshape(-1).copy()).to(dev)
    free = torch.cuda.mem_get_info()[0]
    nb = n
    while nb > 1 and 6 * B * nb * 62 * 4 > 0.8 * free:
        nb //= 2

    # ---- warm-up and calibration
    for _ in range(3):
        launch()
        torch_backtest(logits, masks, B, nb, T, off, rank_lut)
    t1 = timed(launch, 3)
    reps = max(3, int(np.ceil(a.window / t1)))
    tb1 = timed(lambda: torch_backtest(logits, masks, B, nb, T, off, rank_lut), 1)
    reps_b = max(1, int(np.ceil(a.window / tb1)))
    model.backtest(masks, B, n, T, seed, offset=off)

    rounds = []
    for _ in range(a.rounds):
        tk_s = timed(launch, reps)
        tb_s = timed(lambda: torch_backtest(logits, masks, B, nb, T, off, rank_lut), reps_b)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e2e_reps = 3
        for _ in range(e2e_reps):
            res = model.backtest(masks, B, n, T, seed, offset=off)  # ends in a device-to-host copy of the sums
        e2e = (time.perf_counter() - t0) / e2e_reps
        rounds.append({"kernel_s": tk_s, "kernel_tickets_per_s": B * n / tk_s, "torch_s": tb_s,
                       "torch_tickets_per_s": B * nb / tb_s, "ratio_per_ticket": (tb_s / (B * nb)) / (tk_s / (B * n)),
                       "backtest_rows_per_s": B / e2e})
    ratios = [r_["ratio_per_ticket"] for r_ in rounds]
    ks = [r_["kernel_s"] for r_ in rounds]
    med = float(np.median(ks))
    out = {"metric": "ticket sampling + prize-tier scoring (em_draw_tickets)", "rows": B, "tickets_per_row": n,
           "temperature": T, "kernel_launches_per_window": reps, "torch_tickets_per_row": nb,
           "kernel_s_median": med, "kernel_tickets_per_s_median": B * n / med,
           "kernel_s_min_max": [min(ks), max(ks)],
           "ratio_torch_over_kernel_per_ticket": {"min": min(ratios), "median": float(np.median(ratios)),
                                                  "max": max(ratios)},
           "faster_every_round": bool(min(ratios) > 1.0),
           "backtest_rows_per_s_median": float(np.median([r_["backtest_rows_per_s"] for r_ in rounds])),
           "valu_per_ticket": VALU_PER_TICKET,
           "share_of_valu_issue_bound": (B * n / med) / (LANE_OPS_PER_S / VALU_PER_TICKET),
           "spec_check": check, "spec_check_ok": bool(ok), "backtest_best": res["best"].tolist(), "rounds": rounds}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")
    return 0 if ok and out["faster_every_round"] else 1


if __name__ == "__main__":
    sys.exit(main())
