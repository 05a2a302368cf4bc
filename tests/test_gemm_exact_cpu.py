"""The exact-integer GEMM helpers (``_gemm_exact.py``) are themselves checked (no GPU): the reference against a
numpy int64 matmul, and a numpy stand-in "kernel" run through the checkers unmutated (must pass) and with one
mutation per way a GEMM kernel can be wrong (each must be rejected)."""
import numpy as np
import pytest
import torch

import _gemm_exact as GX

M, N, K = 128, 96, 136  # one colpart row, three 32-column blocks, a K with a 64-tile tail


def _operands():
    a = GX.int_operand(M, K, 1, 5, GX.A_MOD, dtype=torch.float32)
    b = GX.rand_int_operand(K, N, GX.B_MOD, seed=7, dtype=torch.float32)
    bias = GX.rand_ints((N,), -400, 400, seed=1)  # outputs past 256: bf16 has to round
    return a, b, bias


def _rne_bits(x32: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def _trunc_bits(x32: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _outside(view: torch.Tensor, offset: int) -> torch.Tensor:
    """One element of the allocation around ``view``, ``offset`` elements from the view's first."""
    return view.as_strided((1,), (1,), view.storage_offset() + offset)


def _standin(a, b, bias, out, colpart, bits, mutate=None):
    """relu(A B + bias) in int64 numpy -> out (fp32 or bf16 view), colpart [M / 128 * N], bits [M / 32, N]."""
    A = a.numpy().astype(np.int64)
    B = b.numpy().astype(np.int64)
    acc = A @ B
    if mutate == "drop_last_k":
        acc[5] -= A[5, K - 1] * B[K - 1]
    x = np.maximum(acc + bias.numpy().astype(np.int64)[None, :], 0)
    if mutate == "off_by_one":
        x[77, 41] += 1
    if mutate == "block_transposed":
        x[32:64, 64:96] = x[32:64, 64:96].T.copy()
    rows = 127 if mutate == "colpart_127" else 128
    colpart.copy_(torch.from_numpy(x[:rows].sum(0).astype(np.float32)))
    w = (x > 0).reshape(M // 32, 32, N).astype(np.uint64)
    words = (w << np.arange(32, dtype=np.uint64)[None, :, None]).sum(1).astype(np.uint32)
    if mutate == "bit_flip":
        words[2, 17] ^= np.uint32(1 << 9)
    bits.copy_(torch.from_numpy(words.view(np.int32)))
    x32 = x.astype(np.float32)
    if out.dtype == torch.float32:
        out.copy_(torch.from_numpy(x32))
    else:
        enc = _trunc_bits(x32) if mutate == "truncate" else _rne_bits(x32)
        out.copy_(torch.from_numpy(enc.view(np.int16)).view(torch.bfloat16))
    if mutate == "pad_column":
        _outside(out, N).copy_(torch.ones(1, dtype=out.dtype))  # right of row 0's last column
    if mutate == "guard_row":
        _outside(out, -out.stride(0)).copy_(torch.ones(1, dtype=out.dtype))  # the row above the view


def _run_and_check(dtype, mutate=None):
    a, b, bias = _operands()
    out, out_ok = GX.guarded(GX.nan_like(M, N, dtype), poison="sentinel", name="out")
    colpart, cp_ok = GX.guarded_flat(GX.sentinel_like((N,), torch.float32), name="colpart")
    bits, bits_ok = GX.guarded_flat(GX.sentinel_like((M // 32, N), torch.int32), name="bits")
    _standin(a, b, bias, out, colpart, bits, mutate)
    ref = GX.reference(a, b, bias=bias, act="relu")
    GX.check_exact(out, ref)
    GX.check_colpart(colpart, ref)
    GX.check_bits(bits, ref)
    for ok in (out_ok, cp_ok, bits_ok):
        ok()


def test_int_operand_values_and_range():
    for mod in (GX.A_MOD, GX.B_MOD):
        v = GX.int_operand(13, 17, 1, 3, mod, dtype=torch.float32)
        assert sorted(set(v.flatten().tolist())) == [float(x) for x in range(-mod // 2, mod // 2 + 1) if x]
        assert not torch.equal(v[:13, :13], v[:13, :13].t())  # asymmetric: a transposed operand shows
        assert v[2, 5].item() == {6: ((2 + 15) % 6), 10: ((2 + 15) % 10)}[mod] - mod // 2 + ((2 + 15) % mod >= mod // 2)
        r = GX.rand_int_operand(40, 50, mod, seed=3, dtype=torch.float32)
        assert torch.equal(r, GX.rand_int_operand(40, 50, mod, seed=3, dtype=torch.float32))
        assert float(r.abs().min()) == 1 and float(r.abs().max()) == mod // 2
    assert torch.equal(GX.int_operand(9, 9, 1, 1, 6).float(), GX.int_operand(9, 9, 1, 1, 6, dtype=torch.float32))


def test_reference_matches_numpy_int64():
    a, b, bias = _operands()
    want = a.numpy().astype(np.int64) @ b.numpy().astype(np.int64)
    assert np.array_equal(GX.reference(a, b).numpy(), want.astype(np.float64))
    c_old = GX.rand_ints((M, N), -9, 9, seed=2)
    got = GX.reference(a, b, alpha=0.5, beta=-0.5, c_old=c_old, bias=bias, act="relu")
    w2 = np.maximum(0.5 * want + bias.numpy()[None, :], 0) - 0.5 * c_old.numpy()
    assert np.array_equal(got.numpy(), w2)
    mask = GX.rand_ints((M, N), -2, 2, seed=3)
    got = GX.reference(a, b, alpha=2.0, dact="relu", mask=mask)
    assert np.array_equal(got.numpy(), 2.0 * want * (mask.numpy() > 0))
    assert np.array_equal(GX.colpart_ref(GX.reference(a, b)).numpy(), want.sum(0, keepdims=True).astype(np.float32))


def test_reference_refuses_inexact_operands():
    a, b, _ = _operands()
    with pytest.raises(AssertionError):
        GX.reference(a + 0.5, b)
    with pytest.raises(AssertionError):
        GX.reference(a * 1000, b * 1000)  # partial sums past 2^24
    with pytest.raises(AssertionError):
        GX.reference(torch.ones(1, GX.K_MAX + 1), torch.ones(GX.K_MAX + 1, 1))


def test_bits_roundtrip():
    p = GX.rand_ints((64, 5), 0, 1, seed=4).bool()
    w = GX.pack_bits(p)
    assert w.dtype == torch.int32 and w.shape == (2, 5)
    assert torch.equal(GX.unpack_bits(w), p)
    one = torch.zeros(32, 1, dtype=torch.bool)
    one[31, 0] = True
    assert GX.pack_bits(one).item() == -(1 << 31)


def test_guarded_layout():
    t = GX.int_operand(5, 13, 1, 1, 6)
    v, ok = GX.guarded(t, pad_cols=16, guard_rows=3)
    assert v.stride() == (32, 1) and v.data_ptr() % 16 == 0 and torch.equal(v, t)
    assert v.storage_offset() == 3 * 32
    assert torch.isnan(_outside(v, 13).float()).all() and torch.isnan(_outside(v, -1).float()).all()
    ok()
    v.fill_(0)  # writes inside the view are not the surround's business
    ok()
    v4, _ = GX.guarded(t, col_off=4)
    assert v4.data_ptr() % 16 == 8 and v4.stride(0) == 24
    f, okf = GX.guarded(GX.nan_like(3, 5, torch.float32), pad_cols=4, poison="sentinel")
    assert f.stride(0) == 12 and _outside(f, 5).view(torch.int32).item() == GX.SENTINEL[torch.float32]
    okf()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_standin_passes(dtype):
    _run_and_check(dtype)


MUTATIONS = ["off_by_one", "drop_last_k", "block_transposed", "pad_column", "guard_row", "colpart_127", "bit_flip"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mutate", MUTATIONS)
def test_mutation_rejected(mutate, dtype):
    with pytest.raises(GX.GemmMismatch):
        _run_and_check(dtype, mutate)


def test_truncation_instead_of_rne_rejected():
    with pytest.raises(GX.GemmMismatch):
        _run_and_check(torch.bfloat16, "truncate")


def test_unwritten_output_rejected():
    a, b, bias = _operands()
    out = GX.nan_like(M, N, torch.float32)
    ref = GX.reference(a, b)
    out.copy_(ref.float())
    GX.check_exact(out, ref)
    out[3, 3] = float("nan")  # the prefill of an element the kernel skipped
    with pytest.raises(GX.GemmMismatch):
        GX.check_exact(out, ref)


def test_check_close_bounds():
    x = torch.arange(-16, 17, dtype=torch.float64)[None, :]
    ref = torch.sigmoid(x)
    GX.check_close(ref.float(), ref)
    GX.check_close(ref.float().bfloat16(), ref)
    with pytest.raises(GX.GemmMismatch):
        GX.check_close((ref * (1 + 2.0 ** -18)).float(), ref)
    with pytest.raises(GX.GemmMismatch):
        GX.check_close((ref.float() * (1 + 2.0 ** -7)).bfloat16(), ref)
    nan = ref.float().clone()
    nan[0, 0] = float("nan")
    with pytest.raises(GX.GemmMismatch):
        GX.check_close(nan, ref)
