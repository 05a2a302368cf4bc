"""Inputs shared by the CPU and the GPU tests of the count-table baseline."""
import numpy as np

FULL = (1 << 64) - 1


def case_masks(n: int, seed: int) -> np.ndarray:
    """int64 [n] arbitrary masks: a third dense (all 64 bits random, so bits 62-63 are often set), a third
    draw-like (5 of the 50 main bits + 2 of the 12 star bits, some with stray bits 62-63), a third sparse, and
    hand-set empty and full masks where they fit."""
    g = np.random.default_rng(seed)
    m = g.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, size=n, dtype=np.uint64)
    kind = g.integers(0, 3, size=n)
    for i in np.nonzero(kind == 1)[0]:
        v = sum(1 << int(b) for b in g.choice(50, 5, replace=False)) | sum(1 << (50 + int(b)) for b in g.choice(12, 2, replace=False))
        m[i] = np.uint64(v | (int(g.integers(0, 4)) << 62))
    for i in np.nonzero(kind == 2)[0]:
        m[i] = np.bitwise_or.reduce(np.uint64(1) << g.integers(0, 64, size=int(g.integers(0, 4)), dtype=np.uint64),
                                    initial=np.uint64(0))
    for i, v in ((0, FULL), (1, 0), (2, 3 << 62), (n - 1, FULL), (n - 2, 0), (n // 2, (1 << 62) - 1)):
        if 0 <= i < n:
            m[i] = np.uint64(v)
    return m.view(np.int64)


def valid_masks(n: int, seed: int, planted: float = 0.0) -> np.ndarray:
    """int64 [n] masks of valid synthetic draws."""
    from euromillioner_amd.data.draws import mask_bits
    from euromillioner_amd.data.synthetic import generate_draws

    out = generate_draws(n, seed=seed, planted=planted)
    return mask_bits(out[0] if isinstance(out, tuple) else out).view(np.int64)


def random_table(lags: int, seed: int):
    """(table float32 [lags, 64, 64], prior float32 [64]) with entries up to +-30 and every mantissa bit in use, so
    the order of the fp32 additions shows; rows / columns 62-63 zero, as ``weights_from_counts`` leaves them."""
    g = np.random.default_rng(seed)
    table = g.uniform(-30, 30, size=(lags, 64, 64)).astype(np.float32)
    table *= g.choice(np.array([1.0, 1e-3, 1e-6], dtype=np.float32), size=table.shape)  # mixed magnitudes
    prior = g.uniform(-5, 0, size=64).astype(np.float32)
    table[:, 62:, :] = 0
    table[:, :, 62:] = 0
    prior[62:] = 0
    return table, prior
