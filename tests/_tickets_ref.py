"""Comparison rules for sampled tickets (tests/test_tickets_cpu.py, tests/test_tickets_gpu.py) against the fp64
specification euromillioner_amd.tickets.  Nothing in this module touches the GPU.

* keys: an fp32 implementation may differ from the fp64 keys by ``tol`` = 16 x the largest error of the SAME
  formula evaluated in numpy fp32 (``key_tol``), per element;
* tickets: equal to the stable top-k of the implementation's OWN keys exactly; equal to the fp64 picks outside
  the *near* set: (row, ticket) pairs whose fp64 5th/6th main gap or 2nd/3rd star gap is below 2 tol.  At most
  ``NEAR_SHARE`` of the pairs may be near (a condition on the inputs, not a measurement of the kernel).
"""
from __future__ import annotations

import numpy as np

from euromillioner_amd import tickets as TK

NEAR_SHARE = 2e-3
TOL_FACTOR = 16.0


def key_tol(scores: np.ndarray, k: np.ndarray, temperature: float) -> tuple[float, np.ndarray]:
    """(tol, fp64 keys) for these scores [B, >= 62] (fp32 values) and bits k [B, n, 62]."""
    k64 = TK.keys_from_bits(scores, k, temperature, np.float64)
    k32 = TK.keys_from_bits(np.asarray(scores, dtype=np.float32), k, temperature, np.float32)
    assert k32.dtype == np.float32
    return TOL_FACTOR * float(np.abs(k32.astype(np.float64) - k64).max()), k64


def near_set(keys64: np.ndarray, tol: float) -> np.ndarray:
    """[B, n] bool: the pick is undecided within 2 tol."""
    m = -np.sort(-keys64[..., :50], axis=-1)
    s = -np.sort(-keys64[..., 50:62], axis=-1)
    return ((m[..., 4] - m[..., 5]) < 2 * tol) | ((s[..., 1] - s[..., 2]) < 2 * tol)


def check_keys(got: np.ndarray, keys64: np.ndarray, tol: float) -> float:
    """got [B, n, >= 62] (fp32) within tol of the fp64 keys, element by element; returns the largest error."""
    err = np.abs(np.asarray(got, dtype=np.float64)[..., :62] - keys64)
    mx = float(err.max()) if err.size else 0.0
    assert not np.isnan(err).any() and mx <= tol, {"max_err": mx, "tol": tol}
    if got.shape[-1] > 62:
        assert not np.asarray(got)[..., 62:].any(), "pad columns must be 0"
    return mx


def check_own_keys(tickets: np.ndarray, got_keys: np.ndarray) -> None:
    """tickets == stable top-5 | top-2 of the implementation's own keys, exactly, with no exclusions."""
    tk = np.asarray(tickets).astype(np.uint64)
    want = TK.tickets_from_keys(np.asarray(got_keys, dtype=np.float64))
    bad = tk != want
    assert not bad.any(), {"mismatches": int(bad.sum()), "of": tk.size, "first": np.argwhere(bad)[:3].tolist()}
    m, s = TK.hits(tk, np.full(tk.shape[0], (1 << 62) - 1, dtype=np.uint64))
    assert (m == 5).all() and (s == 2).all(), "every ticket has 5 main and 2 star bits"
    assert not (tk >> np.uint64(62)).any()


def check_vs_spec(tickets: np.ndarray, keys64: np.ndarray, tol: float) -> dict:
    """tickets equal the fp64 picks outside the near set.  Returns the near / pair counts: the caller sums them
    over the launches of one logit source and asserts the share with ``check_near_share`` (a single launch may
    hold as few as one pair)."""
    tk = np.asarray(tickets).astype(np.uint64)
    want = TK.tickets_from_keys(keys64)
    near = near_set(keys64, tol)
    stats = {"near": int(near.sum()), "pairs": near.size, "differ": int((tk != want).sum()), "tol": tol}
    bad = (tk != want) & ~near
    assert not bad.any(), (stats, np.argwhere(bad)[:3].tolist())
    return stats


def check_near_share(near: int, pairs: int) -> None:
    """A condition on the inputs, not a measurement: with more near pairs the ticket comparison checks too little."""
    assert near <= NEAR_SHARE * pairs, {"near": near, "pairs": pairs, "cap": NEAR_SHARE}


def check_counts_vs_spec(hist, best, tickets64: np.ndarray, targets: np.ndarray, keys64: np.ndarray, tol: float) -> dict:
    """Back-test integers against the spec's: identical when no pair is near; each near ticket may move one
    count from one hist cell to another, each row holding a near ticket one count between two best ranks."""
    near = near_set(keys64, tol)
    h, b = TK.score_tickets_py(tickets64, targets)
    stats = {"near": int(near.sum()), "pairs": near.size, "hist_l1": int(np.abs(np.asarray(hist) - h).sum()),
             "best_l1": int(np.abs(np.asarray(best) - b).sum())}
    assert near.sum() <= NEAR_SHARE * near.size, stats
    assert int(np.asarray(hist).sum()) == near.size and int(np.asarray(best).sum()) == near.shape[0], stats
    assert stats["hist_l1"] <= 2 * int(near.sum()), stats
    assert stats["best_l1"] <= 2 * int(near.any(1).sum()), stats
    return stats


# ------------------------------------------------------------------------------------------------ mutated specs
def mutated_keys(scores, k: np.ndarray, temperature: float, mutation: str, dtype=np.float32) -> np.ndarray:
    """Deliberately wrong implementations of the key formula (for the checks of the rules themselves)."""
    if mutation == "swap_hi_lo":  # the two 23-bit draws of every 64-bit word trade places
        k = k.reshape(k.shape[0], k.shape[1], 31, 2)[..., ::-1].reshape(k.shape)
    elif mutation == "ignore_t":  # every ticket of a row uses ticket 0's stream
        k = np.broadcast_to(k[:, :1], k.shape)
    else:
        raise ValueError(mutation)
    return TK.keys_from_bits(np.asarray(scores, dtype=dtype), k, temperature, dtype)


def unstable_tickets(keys: np.ndarray) -> np.ndarray:
    """top-k in which the LATER index wins a tie."""
    keys = np.asarray(keys, dtype=np.float64)[..., :62]

    def top(a, kk, shift):
        n = a.shape[-1]
        idx = np.argsort(-a[..., ::-1], axis=-1, kind="stable")[..., :kk]
        idx = (n - 1 - idx).astype(np.uint64)
        return np.bitwise_or.reduce(np.uint64(1) << (idx + np.uint64(shift)), axis=-1)

    return top(keys[..., :50], 5, 0) | top(keys[..., 50:], 2, 50)
