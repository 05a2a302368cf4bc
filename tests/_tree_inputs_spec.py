"""Host specifications of ``csrc/tree_inputs.hip``, written from the definitions (``data.draws.lag_features``,
``models.forest.pack_bits``, ``multi_hot`` + ``apply_bins``) and shared by the CPU and the GPU tests."""
import numpy as np

from euromillioner_amd.models.forest import pack_bits

M62 = np.uint64((1 << 62) - 1)


def unpack(masks) -> np.ndarray:
    """uint64 / int64 masks [n] -> 0/1 int64 [n, 62] (bits 62-63 dropped)."""
    m = np.asarray(masks).view(np.uint64).reshape(-1)
    return ((m[:, None] >> np.arange(62, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.int64)


def lag_rows_spec(masks, lags: int, first: int, S: int):
    """(X uint64 [S, W], Y uint64 [S]): sample s = the bits of draws first+s .. first+s+lags-1, oldest first,
    concatenated and packed; its target is draw first+s+lags without bits 62-63."""
    m = np.asarray(masks).view(np.uint64).reshape(-1)
    bits = unpack(m)
    X = np.concatenate([bits[first + k:first + k + S] for k in range(lags)], axis=1)
    return pack_bits(X), (m[first + lags:first + lags + S] & M62).copy()


def random_masks(n: int, seed: int) -> np.ndarray:
    """int64 [n]: all 64 bits random (bits 62-63 must be ignored), with hand-set neighbours that carry only
    bit 0 and only bit 61: a shift that leaks between lag fields moves exactly these."""
    g = np.random.default_rng(seed)
    m = g.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, size=n, dtype=np.uint64)
    for i, v in ((1, 1), (2, 1 << 61), (3, 1), (n - 2, 1 << 61), (n - 1, 1)):
        if 0 <= i < n:
            m[i] = np.uint64(v)
    return m.view(np.int64)
