"""Exact-integer GEMM checks: operands, guarded buffers, fp64 reference and comparison rules.

No GPU code of its own: everything here is plain torch on whatever device the tensors live on, so
``test_gemm_exact_cpu.py`` can run the checkers against a numpy stand-in "kernel" and its mutations, and
``test_gemm_exact_gpu.py`` can hold ``csrc/gemm.hip`` / ``csrc/gemm_f32.hip`` to them.

Why integers.  With ``|A| <= 3`` and ``|B| <= 5`` every product is an integer of magnitude ``<= 15`` and every
partial sum over ``K <= 2560`` terms an integer of magnitude ``<= 15 * K = 38400 < 2^24``: exactly representable
in fp32 *in any summation order*, so an fp32-accumulating kernel must reproduce the fp64 reference bit for
bit (bf16 outputs: after ONE round-to-nearest-even of that exact value).  No operand is zero, so a dropped,
duplicated or misplaced term always changes the sum.  ``colpart`` rows add 128 such values:
``128 * 38400 < 2^23``, still exact.

Comparison rules (:func:`check_exact`, :func:`check_close`):

* ``none`` / ``relu`` epilogues, relu act', ``alpha`` in {1, 0.5, 2}, ``beta`` in {0, 1, -0.5} with integer
  ``C_old`` and integer bias: ``torch.equal`` -- no tolerance.  (Halves of integers below 2^23 are exact too.)
* sigmoid / tanh (activation or act'): the pre-activation is still an exact integer, the reference is
  ``act(integer)`` in fp64, and the bound is elementwise and derived, not measured, for pre-activations kept
  to ``|x| <= 16``:

  - fp32 outputs: ``|out - ref| <= 2^-19 * |ref|``.  ``__expf(x)`` is ``exp2(x * log2 e)``; the rounding of
    ``x * log2 e`` (magnitude < 32, so half an ulp is ``<= 2^-20`` absolute) moves the exponential by at most
    ``2^-20 * ln 2`` relative; after that come at most four further operations (exp2, the add, the
    reciprocal / the library ``tanhf``, the product with act' or alpha) that are each correctly rounded
    (``2^-24``) or documented to 2 ulp (``2^-22``): ``2^-20 + 4 * 2^-22 = 2^-19``.
  - bf16 outputs: one more round-to-nearest-even, half a bf16 ulp ``= 2^-8 * 2^e <= 2^-8 * |ref|``.  Where the
    fp32 error flips the rounding, ``ref`` lies within ``2^-18 * 2^e`` of a midpoint ``2^e (1 + (2k + 1) 2^-8)``,
    so the error ``2^-8 * 2^e + 2^-18 * 2^e`` is still below ``2^-8 * |ref| >= 2^-8 * 2^e (1 + 2^-8)``.
"""
from __future__ import annotations

import torch

SUM_LIMIT = 1 << 24
A_MOD, B_MOD = 6, 10  # |A| <= 3, |B| <= 5
K_MAX = 2560

SENTINEL = {torch.float32: -559038737,  # 0xDEADBEEF
            torch.int32: 0x5A5A5A5A,
            torch.bfloat16: -16657}      # 0xBEEF
_INT_VIEW = {torch.float32: torch.int32, torch.int32: torch.int32, torch.bfloat16: torch.int16}


class GemmMismatch(AssertionError):
    pass


def round8(n: int) -> int:
    return (n + 7) // 8 * 8


# ------------------------------------------------------------------------------------------- operands
def _map_nonzero(v: torch.Tensor, mod: int) -> torch.Tensor:
    """0 .. mod-1  ->  {-mod/2 .. -1, 1 .. mod/2}"""
    half = mod // 2
    return torch.where(v < half, v - half, v - half + 1)


def int_operand(rows: int, cols: int, a: int, b: int, mod: int, device="cpu",
                dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Asymmetric, nowhere-zero integer matrix: ``(a * r + b * c) % mod`` mapped onto
    ``{-mod/2 .. -1, 1 .. mod/2}`` (``mod`` 6: the A side, ``|v| <= 3``; ``mod`` 10: the B side, ``|v| <= 5``)."""
    assert mod in (A_MOD, B_MOD), mod
    r = torch.arange(rows, dtype=torch.int64, device=device)[:, None]
    c = torch.arange(cols, dtype=torch.int64, device=device)[None, :]
    v = _map_nonzero((a * r + b * c) % mod, mod)
    assert rows * cols == 0 or (int(v.abs().min()) >= 1 and int(v.abs().max()) <= mod // 2)
    return v.to(dtype)


def rand_int_operand(rows: int, cols: int, mod: int, seed: int, device="cpu",
                     dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Seeded random variant of :func:`int_operand` (same value range, nowhere zero)."""
    assert mod in (A_MOD, B_MOD), mod
    g = torch.Generator().manual_seed(seed)
    v = _map_nonzero(torch.randint(0, mod, (rows, cols), generator=g, dtype=torch.int64), mod)
    assert rows * cols == 0 or (int(v.abs().min()) >= 1 and int(v.abs().max()) <= mod // 2)
    return v.to(device=device, dtype=dtype)


def rand_ints(shape, lo: int, hi: int, seed: int, device="cpu", dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Seeded integers in [lo, hi] (integer bias, integer ``C_old``, +-1 masks)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int64).to(device=device, dtype=dtype)


# ------------------------------------------------------------------------------------ guarded buffers
def _fill_poison(buf: torch.Tensor, poison: str):
    if poison == "nan":
        assert buf.dtype.is_floating_point
        buf.fill_(float("nan"))
    elif poison == "sentinel":
        buf.view(_INT_VIEW[buf.dtype]).fill_(SENTINEL[buf.dtype])
    else:
        raise ValueError(poison)


def _untouched_checker(buf: torch.Tensor, region: tuple, name: str):
    """Closure comparing everything of ``buf`` outside ``region`` (an index tuple) bitwise with its state now."""
    iv = buf.view(_INT_VIEW[buf.dtype])
    init = iv.clone()

    def check_untouched():
        cur = iv.clone()
        cur[region] = init[region]
        if not torch.equal(cur, init):
            bad = (cur != init).nonzero()
            raise GemmMismatch(f"{name}: {bad.shape[0]} element(s) outside the view were written, first at "
                               f"buffer index {tuple(bad[0].tolist())} (view = {region})")

    return check_untouched


def guarded(t: torch.Tensor, pad_cols: int = 8, guard_rows: int = 2, poison: str = "nan", col_off: int = 0,
            name: str = "buffer"):
    """Place the 2-D ``t`` as a view inside a larger allocation whose every other byte is poison.

    Row stride ``round8(cols) + pad_cols`` (``pad_cols`` a multiple of 8 for bf16, of 4 for fp32, so rows stay
    16-byte aligned), ``guard_rows`` extra rows above and below, the view at column ``col_off`` of its rows.
    ``poison``: ``"nan"`` (operands, masks) or ``"sentinel"`` (outputs: a fixed bit pattern).  Returns
    ``(view, check_untouched)``; ``check_untouched()`` raises :class:`GemmMismatch` if any byte of the
    surround differs from its state at this call."""
    assert t.dim() == 2
    rows, cols = t.shape
    assert pad_cols % (4 if t.dtype == torch.float32 else 8) == 0, pad_cols
    stride = round8(cols) + pad_cols
    assert 0 <= col_off and col_off + cols <= stride
    buf = torch.empty(rows + 2 * guard_rows, stride, dtype=t.dtype, device=t.device)
    _fill_poison(buf, poison)
    region = (slice(guard_rows, guard_rows + rows), slice(col_off, col_off + cols))
    view = buf[region]
    view.copy_(t)
    assert view.stride() == (stride, 1) or rows * cols == 0 or cols == 1 or rows == 1
    return view, _untouched_checker(buf, region, name)


def guarded_flat(t: torch.Tensor, guard: int = 64, poison: str = "sentinel", name: str = "buffer"):
    """A contiguous tensor (bias, ``colpart``, ``bits``, a workspace) inside a flat allocation with ``guard``
    poisoned elements before and after it.  ``guard`` is a multiple of 4 (the view stays 16-byte aligned)."""
    assert guard % 4 == 0 and t.is_contiguous()
    n = t.numel()
    buf = torch.empty(n + 2 * guard, dtype=t.dtype, device=t.device)
    _fill_poison(buf, poison)
    region = (slice(guard, guard + n),)
    view = buf[region].view(t.shape)
    view.copy_(t)
    return view, _untouched_checker(buf, region, name)


def nan_like(rows: int, cols: int, dtype: torch.dtype, device="cpu") -> torch.Tensor:
    """Output prefill for ``beta == 0``: NaN everywhere, so an unwritten element, or a read of ``C``, shows."""
    return torch.full((rows, cols), float("nan"), dtype=dtype, device=device)


def sentinel_like(shape, dtype: torch.dtype, device="cpu") -> torch.Tensor:
    t = torch.empty(tuple(shape), dtype=dtype, device=device)
    _fill_poison(t, "sentinel")
    return t


# -------------------------------------------------------------------------------------------- reference
ACT = {"none": lambda x: x, "relu": torch.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}
DACT = {"relu": lambda y: (y > 0).to(torch.float64), "sigmoid": lambda y: y * (1 - y), "tanh": lambda y: 1 - y * y}


def reference(a_mk: torch.Tensor, b_kn: torch.Tensor, alpha: float = 1.0, beta: float = 0.0,
              c_old: torch.Tensor | None = None, bias: torch.Tensor | None = None, act: str = "none",
              dact: str | None = None, mask: torch.Tensor | None = None, k_max: int = K_MAX) -> torch.Tensor:
    """fp64 ``act(alpha * A B + bias) * act'(mask) + beta * C_old`` of the logical ``A [M, K]``, ``B [K, N]``.
    Asserts the exact-integer bound: integer operands, ``K <= 2560`` and every ``sum_k |A| |B|`` (the largest
    partial sum of any order) below 2^24.  (``k_max``: the one caller whose API imposes a longer reduction
    says so; ``15 * K < 2^24`` is asserted either way.)"""
    A, B = a_mk.to(torch.float64), b_kn.to(torch.float64)
    K = A.shape[1]
    assert B.shape[0] == K and K <= k_max, K
    assert torch.equal(A, A.round()) and torch.equal(B, B.round()), "operands must be integers"
    assert float(A.abs().max()) * float(B.abs().max()) * K <= 15 * K < SUM_LIMIT
    if K:
        assert float((A.abs() @ B.abs()).max()) < SUM_LIMIT
    x = alpha * (A @ B)
    if bias is not None:
        x = x + bias.to(torch.float64)[None, : x.shape[1]]
    x = ACT[act](x)
    if dact is not None:
        x = x * DACT[dact](mask.to(torch.float64))
    if beta != 0.0:
        x = x + beta * c_old.to(torch.float64)
    return x


def colpart_ref(ref: torch.Tensor, rows: int = 128) -> torch.Tensor:
    """fp32 ``[ceil(M / rows), N]``: column sums of the (pre-rounding) epilogue values per ``rows`` output rows."""
    M, N = ref.shape
    P = -(-M // rows)
    pad = torch.zeros(P * rows, N, dtype=torch.float64, device=ref.device)
    pad[:M] = ref
    s = pad.view(P, rows, N).sum(1)
    assert float(s.abs().max()) < SUM_LIMIT
    return s.float()


def pack_bits(positive: torch.Tensor) -> torch.Tensor:
    """bool ``[M, N]`` -> int32 ``[M / 32, N]``: bit ``m % 32`` of word ``[m // 32, n]``."""
    M, N = positive.shape
    assert M % 32 == 0
    w = positive.view(M // 32, 32, N).to(torch.int64)
    sh = torch.arange(32, dtype=torch.int64, device=positive.device)[None, :, None]
    v = (w << sh).sum(1)
    return torch.where(v >= (1 << 31), v - (1 << 32), v).to(torch.int32)


def unpack_bits(bits: torch.Tensor) -> torch.Tensor:
    """Inverse of :func:`pack_bits`: int32 ``[M / 32, N]`` -> bool ``[M, N]``."""
    P, N = bits.shape
    sh = torch.arange(32, dtype=torch.int64, device=bits.device)[None, :, None]
    return (((bits.to(torch.int64)[:, None, :] >> sh) & 1) != 0).reshape(P * 32, N)


# ------------------------------------------------------------------------------------------ comparison
def expected(ref: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fp32 outputs: ``ref.float()``; bf16 outputs: ``ref.float().bfloat16()`` (one RNE of an exact value)."""
    e = ref.float()
    assert torch.equal(e.double(), ref), "the reference must be exact in fp32 (exact rule only)"
    return e if dtype == torch.float32 else e.to(dtype)


def _first_bad(got: torch.Tensor, want: torch.Tensor):
    bad = ~(got == want)
    idx = tuple(bad.nonzero()[0].tolist())
    return int(bad.sum()), idx


def check_exact(out: torch.Tensor, ref: torch.Tensor, what: str = "out"):
    """``torch.equal(out, expected(ref))`` -- no tolerance; names the first offending element."""
    want = expected(ref, out.dtype)
    if out.shape != want.shape:
        raise GemmMismatch(f"{what}: shape {tuple(out.shape)} != {tuple(want.shape)}")
    if not torch.equal(out, want):
        n, idx = _first_bad(out, want)
        raise GemmMismatch(f"{what}: {n} element(s) differ, first at {idx}: got {out[idx].item()!r}, "
                           f"want {want[idx].item()!r}")


def check_colpart(colpart: torch.Tensor, ref: torch.Tensor, rows: int = 128, what: str = "colpart"):
    """``colpart[: ceil(M / rows) * N]`` equals the exact integer column sums of ``ref`` per ``rows`` rows."""
    want = colpart_ref(ref, rows)
    got = colpart.reshape(-1)[: want.numel()].view(want.shape)
    if not torch.equal(got, want):
        n, idx = _first_bad(got, want)
        raise GemmMismatch(f"{what}: {n} partial(s) differ, first at {idx}: got {got[idx].item()!r}, "
                           f"want {want[idx].item()!r}")


def check_bits(bits: torch.Tensor, ref: torch.Tensor, what: str = "bits"):
    """``bits`` equals the packed ``ref > 0``."""
    want = pack_bits(ref > 0)
    if bits.shape != want.shape or not torch.equal(bits, want):
        n, idx = _first_bad(bits, want)
        raise GemmMismatch(f"{what}: {n} word(s) differ, first at {idx}: got {bits[idx].item():#x}, "
                           f"want {want[idx].item():#x}")


REL_F32, REL_BF16 = 2.0 ** -19, 2.0 ** -8


def check_close(out: torch.Tensor, ref: torch.Tensor, what: str = "out"):
    """sigmoid / tanh only: ``|out - ref| <= 2^-19 |ref|`` (fp32) or ``2^-8 |ref|`` (bf16), elementwise (the
    derivation is in the module docstring)."""
    rel = REL_F32 if out.dtype == torch.float32 else REL_BF16
    if out.shape != ref.shape:
        raise GemmMismatch(f"{what}: shape {tuple(out.shape)} != {tuple(ref.shape)}")
    err = (out.double() - ref).abs()
    ok = err <= rel * ref.abs()  # NaN fails
    if not bool(ok.all()):
        idx = tuple((~ok).nonzero()[0].tolist())
        raise GemmMismatch(f"{what}: {int((~ok).sum())} element(s) off the derived bound {rel:g} |ref|, first at "
                           f"{idx}: got {out[idx].item()!r}, want {ref[idx].item()!r}")
