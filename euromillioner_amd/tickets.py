"""Tickets sampled from a model's scores, and their prize tiers: the specification (pure numpy, no GPU).

``euromillioner predict`` prints the arg-max ticket and every validation metric scores that one pick.  This
module defines (a) how N tickets are *sampled* from a 62-wide score row and (b) how tickets are *scored*
against the draw that followed.  ``csrc/tickets.hip`` reproduces it on the GPU (tests/test_tickets_gpu.py),
the same way ``csrc/datagen.hip`` reproduces ``data/device_gen.generate_masks_py``.

**Sampling.**  A ticket is 5 of the 50 main numbers and 2 of the 12 stars, drawn without replacement from
the Plackett-Luce distribution with weights ``exp(score / T)``, by Gumbel top-k: add independent Gumbel noise
to ``score / T`` and keep the top 5 / top 2.  For row id ``r`` (a 64-bit global sample index), ticket ``t``
(0 <= t < N <= 64) and output ``o`` (0..61), everything mod 2^64::

    s  = mix64(seed ^ ((r * 64 + t + 1) * 0xD1B54A32D192ED03))     # mix64 / GOLDEN: splitmix64, as datagen.hip
    for j in 0..30:  s += GOLDEN; x = mix64(s)
                     k[2j] = x >> 41;  k[2j+1] = (x >> 9) & 0x7FFFFF   # two 23-bit draws per 64-bit word
    u[o]   = (2 k[o] + 1) * 2^-24           # exact in fp32, never 0 or 1
    G[o]   = -log(-log(u[o]))
    key[o] = score[o] * (1 / T) + G[o]
    ticket = stable_top5(key[0:50]) | stable_top2(key[50:62])      # uint64 mask, layout of em_rows_to_masks

"Stable": the earlier index wins a tie, as ``metrics.draw_metrics`` and ``topk_mask`` in ``csrc/draw_topk.h``.
``T == 0`` is greedy: ``key = score`` (no noise, no scaling), so all N tickets are the arg-max pick.

**Scores.**  MLPs use their logits under both losses.  Under ``softmax`` the weights ``exp(logit)`` are the
group's probabilities up to a constant; under ``bce`` ``exp(logit) = p / (1 - p)``: the weights are the
*odds* of each output, not its probability.  Tree models have probabilities only: ``log_scores(p)``.

**Scoring.**  A ticket against a draw gives (m, s) = (main hits, star hits); ``TIER_RANK[m, s]`` is its prize
tier 1..13, or 14 for no prize.  A back-test counts tickets per (m, s) cell (``hist``) and draws by the best
rank among their N tickets (``best``); ``uniform_expectation`` gives both under uniformly random tickets, to
be read next to the counts the way ``trivial_acc`` is read next to ``acc``.
"""
from __future__ import annotations

import math

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
TICKET_SALT = 0xD1B54A32D192ED03
MAX_TICKETS = 64
MAIN_BITS = (1 << 50) - 1
NO_PRIZE = 14

# prize tier of (m main hits, s star hits) at [m, s]; 14 = no prize.  csrc/tickets.hip mirrors it (tier_rank).
TIER_RANK = np.array([[14, 14, 14],
                      [14, 14, 11],
                      [13, 12, 8],
                      [10, 9, 6],
                      [7, 5, 4],
                      [3, 2, 1]], dtype=np.int64)
TIER_RANK.setflags(write=False)
TIER_NAMES = ("5+2", "5+1", "5+0", "4+2", "4+1", "3+2", "4+0", "2+2", "3+1", "3+0", "1+2", "2+1", "2+0", "none")


def _mix64(z: np.ndarray) -> np.ndarray:
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def check_n_t(n: int, temperature: float) -> None:
    if not 1 <= int(n) <= MAX_TICKETS:
        raise ValueError(f"n_tickets={n}: must be in 1..{MAX_TICKETS}")
    if not (temperature >= 0 and math.isfinite(temperature)):
        raise ValueError(f"temperature={temperature}: must be finite and >= 0 (0 = greedy)")


def ticket_uniform_bits(seed: int, row_ids, n: int) -> np.ndarray:
    """The 23-bit draws ``k`` [B, n, 62] (uint32) of rows ``row_ids`` (64-bit global sample indices)."""
    if not 1 <= int(n) <= MAX_TICKETS:
        raise ValueError(f"n_tickets={n}: must be in 1..{MAX_TICKETS}")
    r = np.array([int(x) & M64 for x in np.asarray(row_ids, dtype=object).reshape(-1)], dtype=np.uint64)
    t = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        s = _mix64(np.uint64(int(seed) & M64) ^ ((r[:, None] * np.uint64(64) + t[None, :] + np.uint64(1))
                                                 * np.uint64(TICKET_SALT)))
        k = np.empty((len(r), n, 62), dtype=np.uint32)
        for j in range(31):
            s = s + np.uint64(GOLDEN)
            x = _mix64(s)
            k[:, :, 2 * j] = (x >> np.uint64(41)).astype(np.uint32)
            k[:, :, 2 * j + 1] = ((x >> np.uint64(9)) & np.uint64(0x7FFFFF)).astype(np.uint32)
    return k


def uniforms(k: np.ndarray, dtype=np.float64) -> np.ndarray:
    """u = (2k + 1) 2^-24: inside (0, 1) and exactly representable in fp32."""
    return (2 * k.astype(np.int64) + 1).astype(dtype) * dtype(2.0 ** -24)


def keys_from_bits(scores: np.ndarray, k: np.ndarray, temperature: float, dtype=np.float64) -> np.ndarray:
    """key [B, n, 62] of the formula above evaluated in ``dtype`` (fp64: the specification; fp32: the error
    scale of the formula itself, which the tests' tolerances are multiples of)."""
    z = np.asarray(scores)[:, None, :62].astype(dtype)
    if temperature == 0:
        return np.broadcast_to(z, k.shape).copy()
    u = uniforms(k, dtype)
    g = -np.log(-np.log(u))
    return z * (dtype(1.0) / dtype(temperature)) + g


def _topk_bits(key: np.ndarray, k: int, shift: int) -> np.ndarray:
    idx = np.argsort(-key, axis=-1, kind="stable")[..., :k]  # earlier index wins a tie
    return np.bitwise_or.reduce(np.uint64(1) << (idx.astype(np.uint64) + np.uint64(shift)), axis=-1)


def tickets_from_keys(keys: np.ndarray) -> np.ndarray:
    """keys [..., >= 62] -> uint64 masks [...]: stable top-5 of the mains | stable top-2 of the stars."""
    keys = np.asarray(keys)
    return _topk_bits(keys[..., :50], 5, 0) | _topk_bits(keys[..., 50:62], 2, 50)


def sample_tickets_py(scores, row_ids, n: int, temperature: float = 1.0, seed: int = 0):
    """(tickets uint64 [B, n], keys fp64 [B, n, 62]) for score rows [B, >= 62] with global row ids [B]."""
    check_n_t(n, temperature)
    scores = np.asarray(scores)
    if scores.ndim != 2 or scores.shape[1] < 62:
        raise ValueError("scores must be [B, >= 62]")
    k = ticket_uniform_bits(seed, row_ids, n)
    if k.shape[0] != scores.shape[0]:
        raise ValueError("one row id per score row")
    keys = keys_from_bits(scores, k, temperature)
    return tickets_from_keys(keys), keys


def log_scores(p) -> np.ndarray:
    """Scores of a model that outputs probabilities (RF, GBDT): log(max(p, 1e-12))."""
    return np.log(np.maximum(np.asarray(p, dtype=np.float64), 1e-12))


def ticket_numbers(ticket: int) -> tuple[list[int], list[int]]:
    """uint64 mask -> (main numbers 1..50 ascending, stars 1..12 ascending)."""
    t = int(ticket)
    return [i + 1 for i in range(50) if (t >> i) & 1], [i + 1 for i in range(12) if (t >> (50 + i)) & 1]


def _popcount(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64)
    c = np.zeros(x.shape, dtype=np.int64)
    for b in range(62):
        c += ((x >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    return c


def hits(tickets, targets) -> tuple[np.ndarray, np.ndarray]:
    """(m, s) [B, n]: main and star hits of tickets [B, n] against target masks [B]."""
    tk = np.asarray(tickets).astype(np.uint64)
    tg = np.asarray(targets).astype(np.uint64).reshape(-1)
    both = tk & tg[:, None]
    return _popcount(both & np.uint64(MAIN_BITS)), _popcount(both >> np.uint64(50))


def score_tickets_py(tickets, targets) -> tuple[np.ndarray, np.ndarray]:
    """(hist [6, 3] int64: tickets per (m, s) cell; best [14] int64: draws by the best rank of their tickets)."""
    m, s = hits(tickets, targets)
    hist = np.zeros((6, 3), dtype=np.int64)
    np.add.at(hist, (m.reshape(-1), s.reshape(-1)), 1)
    best = np.zeros(14, dtype=np.int64)
    if m.size:
        np.add.at(best, TIER_RANK[m, s].min(axis=1) - 1, 1)
    return hist, best


def uniform_expectation(n_tickets: int) -> dict:
    """Uniformly random play: ``hist`` [6, 3] = probability of each (m, s) cell per ticket (hypergeometric:
    C(5,m) C(45,5-m) / C(50,5) x C(2,s) C(10,2-s) / C(12,2); jackpot 1 / 139 838 160), ``rank`` [14] = the same
    by prize tier, ``best`` [14] = probability per draw that the best of ``n_tickets`` i.i.d. uniform tickets
    has that rank.  Multiply by the ticket / draw count for expected counts."""
    if n_tickets < 1:
        raise ValueError("n_tickets >= 1")
    c = math.comb
    pm = [c(5, m) * c(45, 5 - m) / c(50, 5) for m in range(6)]
    ps = [c(2, s) * c(10, 2 - s) / c(12, 2) for s in range(3)]
    hist = np.outer(pm, ps)
    rank = np.zeros(14, dtype=np.float64)
    np.add.at(rank, TIER_RANK.reshape(-1) - 1, hist.reshape(-1))
    # P(best >= r) = P(no ticket better than r)^n; ranks 1..14 in order of worth
    better = np.concatenate([[0.0], np.cumsum(rank)])  # better[r] = P(one ticket's rank <= r), better[14] = 1
    none_better = (1.0 - better) ** n_tickets
    none_better[-1] = 0.0
    best = none_better[:-1] - none_better[1:]
    return {"hist": hist, "rank": rank, "best": best}


def tier_counts(hist) -> np.ndarray:
    """hist [6, 3] -> tickets per prize tier [14] (rank 14 = the five no-prize cells)."""
    out = np.zeros(14, dtype=np.asarray(hist).dtype)
    np.add.at(out, TIER_RANK.reshape(-1) - 1, np.asarray(hist).reshape(-1))
    return out
