"""Transition-count baseline: the smoothed first-order table "number a in a draw -> number b in a later draw".

In the planted generator (``data/synthetic.py``) each sorted position of draw t votes through a fixed permutation
for a number of draw t + 1, so this table is the sufficient statistic of the whole planted signal: it is the floor
a learned model (MLP, forest, GBDT) has to beat, where ``trivial_acc`` only says how sparse the targets are.

This module is the specification (numpy) and the model.  ``csrc/draw_counts.hip`` (``ops.draw_counts``) reproduces
:func:`pair_counts_np` exactly and :func:`logits_np` bit for bit on device masks.

Masks are the 8-byte feature masks every draw kernel reads: bit n-1 main number n, bit 49+s star s, bits 62-63
ignored.  ``lags`` in 1..4, in ``GemmMLPTrainer``'s convention: sample i reads draws i .. i+lags-1 and its target is
draw i+lags.  The logits are grouped-softmax scores (main numbers over columns 0-49, stars over 50-61), which is
what ``draw_metrics(loss="softmax")`` and ``draw_tickets`` consume.
"""
from __future__ import annotations

import zipfile

import numpy as np

NF = 62
MAX_LAGS = 4
_DRAW_BITS = np.uint64((1 << NF) - 1)
_CKPT_KEYS = ("counts", "S", "T", "N", "alpha", "lags", "table", "prior")


# ---------------------------------------------------------------------------------------------
# specification
# ---------------------------------------------------------------------------------------------
def _as_masks(masks) -> np.ndarray:
    m = np.asarray(masks)
    if m.ndim != 1 or m.dtype not in (np.dtype(np.uint64), np.dtype(np.int64)):
        raise ValueError("masks must be a 1-D uint64 / int64 array of feature masks")
    return m.view(np.uint64)


def _bits(m: np.ndarray) -> np.ndarray:
    """[len(m), 64] int64 of 0 / 1: column j = bit j, columns 62-63 zero."""
    return (((m & _DRAW_BITS)[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.int64)


def bit_counts_np(masks, a: int, b: int) -> np.ndarray:
    """int64 [64]: masks in ``[a, b)`` with bit j set (62-63 zero), the numpy form of ``ops.tree_inputs.bit_counts``
    on the 62 draw bits."""
    m = _as_masks(masks)
    out = np.zeros(64, dtype=np.int64)
    for c0 in range(int(a), int(b), 1 << 18):
        out += _bits(m[c0:min(int(b), c0 + (1 << 18))]).sum(0)
    return out


def pair_counts_np(masks, lag: int, first: int, count: int) -> np.ndarray:
    """int64 [64, 64]: ``C[a, b]`` = number of t in ``[first, first + count)`` with bit a of ``masks[t]`` and bit b
    of ``masks[t + lag]`` both set.  ``lag`` in 0..4; rows and columns 62-63 are zero."""
    m = _as_masks(masks)
    lag, first, count = int(lag), int(first), int(count)
    if not 0 <= lag <= MAX_LAGS:
        raise ValueError(f"lag must be in 0..{MAX_LAGS}, got {lag}")
    if count < 1 or first < 0 or first + count + lag > len(m):
        raise ValueError(f"samples [{first}, {first + count}) + lag {lag} exceed the {len(m)} masks")
    C = np.zeros((64, 64), dtype=np.int64)
    for c0 in range(first, first + count, 1 << 16):
        c1 = min(first + count, c0 + (1 << 16))
        # (float64 products of 0 / 1 over at most 2^16 rows are exact integers)
        C += (_bits(m[c0:c1]).astype(np.float64).T @ _bits(m[c0 + lag:c1 + lag]).astype(np.float64)).astype(np.int64)
    return C


def weights_from_counts(C, S, T, N, alpha: float) -> tuple[np.ndarray, np.ndarray]:
    """(table float32 [lags, 64, 64], prior float32 [64]), computed in fp64 and cast once:

        prior[b]       = log((T[b] + alpha) / (N + 2 alpha))
        table[k-1,a,b] = log(((C[k-1,a,b] + alpha) / (S[k-1,a] + 2 alpha)) / ((T[b] + alpha) / (N + 2 alpha)))

    ``C`` [lags, 64, 64] pairs the draw k steps before the target with the target, ``S`` [lags, 64] are the source
    bit counts, ``T`` [64] the target bit counts, ``N`` the number of samples.  Rows and columns 62-63 of ``table``
    and ``prior[62:]`` are exactly 0."""
    C, S, T = np.asarray(C, dtype=np.float64), np.asarray(S, dtype=np.float64), np.asarray(T, dtype=np.float64)
    alpha, N = float(alpha), float(N)
    if not alpha > 0:
        raise ValueError(f"alpha must be > 0, got {alpha}")
    if C.ndim != 3 or C.shape[1:] != (64, 64) or S.shape != (C.shape[0], 64) or T.shape != (64,):
        raise ValueError("C [lags, 64, 64], S [lags, 64], T [64]")
    pb = (T + alpha) / (N + 2 * alpha)
    prior = np.log(pb)
    table = np.log(((C + alpha) / (S[:, :, None] + 2 * alpha)) / pb[None, None, :])
    prior[NF:] = 0.0
    table[:, NF:, :] = 0.0
    table[:, :, NF:] = 0.0
    return table.astype(np.float32), prior.astype(np.float32)


def logits_np(masks, idx, table, prior) -> np.ndarray:
    """float32 [B, 64] scores of samples ``idx``.  The order of the fp32 additions is part of the specification:
    ``acc = prior[b]``; for k = 1..lags, for each set bit a of ``masks[i + lags - k]`` (bits 62-63 ignored) in
    ascending a: ``acc = fl32(acc + table[k-1][a][b])``.  Columns 62-63 are 0."""
    m = _as_masks(masks)
    table, prior = np.asarray(table), np.asarray(prior)
    if table.dtype != np.float32 or prior.dtype != np.float32:
        raise ValueError("table and prior must be float32")
    lags = table.shape[0]
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    if len(idx) and (idx.min() < 0 or idx.max() + lags > len(m)):
        raise ValueError("sample index outside the masks")
    acc = np.broadcast_to(prior[None, :], (len(idx), 64)).astype(np.float32)
    for k in range(1, lags + 1):
        src = m[idx + (lags - k)] & _DRAW_BITS
        for a in range(NF):
            rows = np.nonzero((src >> np.uint64(a)) & np.uint64(1))[0]
            if len(rows):
                acc[rows] = acc[rows] + table[k - 1, a][None, :]  # float32 + float32: one rounding each
    acc[:, NF:] = 0.0
    return acc


# ---------------------------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------------------------
class CountTable:
    """The count-table model.  ``device``: "auto" (a GPU when there is one), "cuda" or "cpu"."""

    group = None  # single-process (ops.tickets.backtest_model asks)

    def __init__(self, lags: int = 1, alpha: float = 1.0, device: str = "auto"):
        if not 1 <= int(lags) <= MAX_LAGS:
            raise ValueError(f"lags must be in 1..{MAX_LAGS}, got {lags}")
        if not float(alpha) > 0:
            raise ValueError(f"alpha must be > 0, got {alpha}")
        if device not in ("auto", "cuda", "cpu"):
            raise ValueError("device must be auto, cuda or cpu")
        self.lags, self.alpha, self.device = int(lags), float(alpha), device
        self.counts = self.S = self.T = self.table = self.prior = None
        self.N = 0
        self.backend_used: str | None = None
        self._dev = None  # (table, prior) on the GPU

    # ------------------------------------------------------------------ fit
    def _use_gpu(self) -> bool:
        if self.device == "cpu":
            return False
        import torch

        if self.device == "cuda" and not torch.cuda.is_available():
            raise RuntimeError("CountTable(device='cuda') needs a GPU")
        return torch.cuda.is_available()

    def _window(self, n: int, first: int, count: int | None) -> tuple[int, int]:
        first = int(first)
        count = n - self.lags - first if count is None else int(count)
        if count < 1 or first < 0 or first + count + self.lags > n:
            raise ValueError(f"samples [{first}, {first + count}) with {self.lags} lag(s) and a target exceed {n} draws")
        return first, count

    def _finish(self, C, S, T, count: int, backend: str) -> "CountTable":
        self.counts, self.S, self.T, self.N = C, S, T, int(count)
        self.table, self.prior = weights_from_counts(C, S, T, count, self.alpha)
        self.backend_used, self._dev = backend, None
        return self

    def fit_masks_np(self, masks, first: int = 0, count: int | None = None) -> "CountTable":
        """Fit on samples ``[first, first + count)`` of host masks through the numpy specification."""
        m = _as_masks(masks)
        first, count = self._window(len(m), first, count)
        L = self.lags
        C = np.stack([pair_counts_np(m, k, first + L - k, count) for k in range(1, L + 1)])
        S = np.stack([bit_counts_np(m, first + L - k, first + L - k + count) for k in range(1, L + 1)])
        return self._finish(C, S, bit_counts_np(m, first + L, first + L + count), count, "numpy")

    def fit_draw_masks(self, masks, first: int = 0, count: int | None = None) -> "CountTable":
        """Fit on samples ``[first, first + count)`` of device masks: ``lags`` launches of ``pair_counts`` on shifted
        windows, the bit counts from ``ops.tree_inputs.bit_counts``, the weights on the host."""
        from ..ops import draw_counts as DC
        from ..ops import tree_inputs as TI

        n = TI._check_masks(masks)
        first, count = self._window(n, first, count)
        L = self.lags
        C = np.stack([DC.pair_counts(masks, k, first + L - k, count).cpu().numpy() for k in range(1, L + 1)])
        S = np.stack([TI.bit_counts(masks, first + L - k, first + L - k + count) for k in range(1, L + 1)])
        T = TI.bit_counts(masks, first + L, first + L + count)
        S[:, NF:] = 0  # (bit_counts counts all 64 bits; the model ignores 62-63)
        T[NF:] = 0
        return self._finish(C, S, T, count, "hip")

    def fit(self, numbers) -> "CountTable":
        """Fit on every sample of host draw rows [N, 8]: on the GPU when there is one, else the specification."""
        from ..data.draws import mask_bits

        if self._use_gpu():
            from .mlp import FusedSmallMLP

            return self.fit_draw_masks(FusedSmallMLP.prepare(np.asarray(numbers)))
        return self.fit_masks_np(mask_bits(np.asarray(numbers)))

    # ------------------------------------------------------------------ score (GPU)
    def _fitted(self) -> None:
        if self.table is None:
            raise ValueError("the count table is not fitted")

    def _device_weights(self, device):
        import torch

        self._fitted()
        if self._dev is None or self._dev[0].device != device:
            self._dev = (torch.from_numpy(self.table).to(device), torch.from_numpy(self.prior).to(device))
        return self._dev

    def _tmasks(self, masks):
        """Masks as the loss / metric / ticket kernels see them: their target masks[i + 1] is draw i + lags."""
        return masks[self.lags - 1:] if self.lags > 1 else masks

    def logits(self, masks, B: int, offset: int = 0, sidx=None):
        """float32 [B, 64] device logits of samples ``offset + s`` (or ``sidx[s]``) of device masks."""
        from ..ops import draw_counts as DC

        table, prior = self._device_weights(masks.device)
        return DC.count_logits(masks, B, table, prior, offset=offset, sidx=sidx)

    def evaluate(self, masks, B: int, offset: int = 0, sidx=None, chunk: int = 1 << 22) -> dict:
        """The ``METRIC_NAMES`` dict of ``FusedSmallMLP.evaluate``: each sample scored against draw i + lags."""
        from ..ops import fused_mlp as FM

        tot = np.zeros(8, dtype=np.float64)
        done = 0
        while done < B:
            b = min(chunk, B - done)
            o = offset + done if sidx is None else 0
            si = None if sidx is None else sidx[done:done + b]
            lg = self.logits(masks, b, o, si)
            tot += FM.draw_metrics(lg, self._tmasks(masks), b, loss="softmax", offset=o,
                                   sidx=si).double().sum(0).cpu().numpy()
            done += b
        cnt = max(tot[7], 1.0)
        out = {k: float(tot[i] / cnt) for i, k in enumerate(FM.METRIC_NAMES[:-1])}
        out["count"] = int(tot[7])
        return out

    def tickets(self, masks, B: int, n_tickets: int, temperature: float = 1.0, seed: int = 0, offset: int = 0,
                sidx=None, row_base: int = 0):
        """``n_tickets`` tickets per sample, sampled from the logits (``ops.tickets.draw_tickets``): int64 [B, n]."""
        from ..ops import tickets as OT

        lg = self.logits(masks, B, offset=offset, sidx=sidx)
        return OT.draw_tickets(lg, B, n_tickets, temperature, seed, offset=offset, sidx=sidx,
                               row_base=row_base)["tickets"]

    def backtest(self, masks, B: int, n_tickets: int, temperature: float = 1.0, seed: int = 0, offset: int = 0,
                 sidx=None, chunk: int = 1 << 20) -> dict:
        """Prize-tier counts of ``n_tickets`` sampled tickets on each of B samples (``ops.tickets.backtest_model``);
        sample i is scored against draw i + lags."""
        from ..ops import tickets as OT

        return OT.backtest_model(self, masks, B, n_tickets, temperature, seed, offset=offset, sidx=sidx, chunk=chunk,
                                 target_masks=self._tmasks(masks))

    # ------------------------------------------------------------------ score (numpy)
    def logits_np(self, masks, idx) -> np.ndarray:
        self._fitted()
        return logits_np(masks, idx, self.table, self.prior)

    def evaluate_np(self, masks, first: int, count: int, chunk: int = 1 << 16) -> dict:
        """:meth:`evaluate` through the numpy specification and ``metrics.draw_metrics``."""
        from ..metrics import draw_metrics

        m = _as_masks(masks)
        keys = ("loss", "acc", "acc_thr", "hits_main", "hits_star", "exact", "trivial_acc")
        tot = np.zeros(len(keys), dtype=np.float64)
        for a in range(first, first + count, chunk):
            b = min(first + count, a + chunk)
            r = draw_metrics(self.logits_np(m, np.arange(a, b)), _bits(m[a + self.lags:b + self.lags]), "softmax")
            tot += np.array([r[k] for k in keys]) * (b - a)
        out = {k: float(tot[i] / max(count, 1)) for i, k in enumerate(keys)}
        out["count"] = int(count)
        return out

    # ------------------------------------------------------------------ state
    def save(self, path: str) -> None:
        """``.cnt``: an ``np.savez`` archive of the counts, the fit's constants and the float32 weights themselves, so
        a re-loaded model scores bit-identically."""
        self._fitted()
        with open(path, "wb") as f:
            np.savez(f, counts=self.counts.astype(np.int64), S=self.S.astype(np.int64), T=self.T.astype(np.int64),
                     N=np.int64(self.N), alpha=np.float64(self.alpha), lags=np.int64(self.lags),
                     table=self.table.astype(np.float32), prior=self.prior.astype(np.float32))

    @classmethod
    def load(cls, path: str, device: str = "auto") -> "CountTable":
        try:
            with open(path, "rb") as f, np.load(f, allow_pickle=False) as z:
                missing = [k for k in _CKPT_KEYS if k not in z.files]
                if missing:
                    raise ValueError(f"{path}: not a count-table checkpoint (no {', '.join(missing)})")
                d = {k: z[k] for k in z.files}  # (a pickled member raises here: allow_pickle=False)
        except zipfile.BadZipFile as e:
            raise ValueError(f"{path}: not a count-table checkpoint ({e})") from e
        lags = int(d["lags"])
        m = cls(lags, float(d["alpha"]), device)
        if (d["table"].shape != (lags, 64, 64) or d["prior"].shape != (64,) or d["table"].dtype != np.float32
                or d["prior"].dtype != np.float32 or d["counts"].shape != (lags, 64, 64)):
            raise ValueError(f"{path}: count-table arrays of the wrong shape or type")
        m.counts, m.S, m.T, m.N = d["counts"], d["S"], d["T"], int(d["N"])
        m.table, m.prior = np.ascontiguousarray(d["table"]), np.ascontiguousarray(d["prior"])
        m.backend_used = "loaded"
        return m
