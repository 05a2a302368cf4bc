"""What the native bf16 GEMM entries refuse, in one table.

``test_gemm_exact_gpu.py`` pins what each path computes; this file pins what ``em_gemm_bf16`` and
``em_gemm_bf16_splitk`` turn away.  The entries are called directly (``ops/linear.gemm``'s own checks would
intercept most cases).  A refused call returns ``EM_ERR_ARG`` before any launch, so every output buffer
(``C`` bf16 / fp32, ``ct``, ``colpart``, ``bits``) must keep its poison pattern bit for bit.  ``M = 0`` and
``N = 0`` are accepted and touch nothing either.  All shapes fit the 256 x 256 buffers, whatever the verdict.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

EM_ERR_ARG = -1
NONE, RELU, SIGMOID = 0, 1, 2
DIM = 256
POISON16, POISON32 = 0x7A5C, 0x7A5C7A5C


@pytest.fixture(scope="module")
def bufs():
    def poisoned(dtype, value):
        return torch.full((DIM, DIM), value, dtype=dtype, device="cuda")

    b = {
        "a": torch.ones(DIM, DIM, dtype=torch.bfloat16, device="cuda"),
        "b": torch.ones(DIM, DIM, dtype=torch.bfloat16, device="cuda"),
        "mask": torch.ones(DIM, DIM, dtype=torch.bfloat16, device="cuda"),
        "c16": poisoned(torch.int16, POISON16),
        "c32": poisoned(torch.int32, POISON32),
        "ct": poisoned(torch.int16, POISON16),
        "colpart": poisoned(torch.int32, POISON32),
        "bits": poisoned(torch.int32, POISON32),
    }
    torch.cuda.synchronize()
    return b


def _untouched(bufs):
    torch.cuda.synchronize()
    for name, value in (("c16", POISON16), ("c32", POISON32), ("ct", POISON16), ("colpart", POISON32),
                        ("bits", POISON32)):
        assert bool((bufs[name] == value).all()), f"{name} was written"


def _gemm(bufs, M=128, N=128, K=64, *, a="a", a_off=0, lda=DIM, a_kc=1, b="b", b_kc=1, c="c16", act=NONE, mask=None,
          dact=0, ct=None, colpart=None, colpart_off=0, bits=None):
    """``em_gemm_bf16`` on the module's buffers (``None`` = null pointer); ``c`` picks the bf16 or fp32 output."""
    from euromillioner_amd.ops import _native as NV
    from euromillioner_amd.ops import linear  # noqa: F401  (registers the signatures)

    def p(name, off=0):
        return bufs[name].data_ptr() + off if name else None

    return NV.query("em_gemm_bf16", p(a, a_off), lda, a_kc, p(b), DIM, b_kc, p(c), DIM, int(c == "c16"), M, N, K,
                    None, act, p(mask), DIM if mask else 0, dact, 1.0, 0.0, p(ct), DIM if ct else 0,
                    p(colpart, colpart_off), p(bits), NV.stream_handle(bufs["a"].device))


REFUSED = {
    "null_a": dict(a=None),
    "null_b": dict(b=None),
    "null_c": dict(c=None),
    "negative_m": dict(M=-1),
    "act_4": dict(act=4),
    "mask_dact_0": dict(mask="mask", dact=0),
    "mask_dact_4": dict(mask="mask", dact=4),
    "dact_without_mask_or_bits": dict(dact=RELU),
    "lda_not_multiple_of_8": dict(lda=252),
    "a_offset_2_bytes": dict(a_off=2),
    "bits_fp32_out": dict(M=256, N=256, act=RELU, c="c32", bits="bits"),
    "bits_m_48": dict(M=48, N=256, act=RELU, bits="bits"),
    "bits_act_sigmoid": dict(M=256, N=256, act=SIGMOID, bits="bits"),
    "bits_with_mask_and_dact": dict(M=256, N=256, mask="mask", dact=RELU, bits="bits"),
    "colpart_offset_2_bytes": dict(M=256, N=256, colpart="colpart", colpart_off=2),
    "ct_not_a_256_shape": dict(M=128, N=128, K=64, ct="ct"),
    "colpart_not_a_256_shape": dict(M=128, N=128, K=64, colpart="colpart"),
    "ct_b_mn": dict(M=256, N=256, K=64, b_kc=0, ct="ct"),
    "ct_fp32_out": dict(M=256, N=256, K=256, c="c32", ct="ct"),
    "act_with_dact_k64": dict(M=256, N=256, K=64, act=RELU, mask="mask", dact=RELU),
    "act_with_dact_tile256": dict(M=256, N=256, K=256, act=RELU, mask="mask", dact=RELU),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refused(bufs, case):
    assert _gemm(bufs, **REFUSED[case]) == EM_ERR_ARG
    _untouched(bufs)


@pytest.mark.parametrize("m,n", [(0, 256), (256, 0)])
def test_empty_output_is_a_noop(bufs, m, n):
    assert _gemm(bufs, M=m, N=n, K=64, ct="ct", colpart="colpart") == 0
    _untouched(bufs)


@pytest.mark.parametrize("splits,kstep", [(2, 96), (2, 64), (0, 64)], ids=["kstep_96", "slices_short_of_k", "splits_0"])
def test_splitk_refused(bufs, splits, kstep):
    """K = 256: a ``kstep`` that is no multiple of 64, ``splits * kstep < K``, and no slice at all."""
    from euromillioner_amd.ops import _native as NV
    from euromillioner_amd.ops import linear  # noqa: F401

    rc = NV.query("em_gemm_bf16_splitk", bufs["a"].data_ptr(), DIM, 0, bufs["b"].data_ptr(), DIM, 0,
                  bufs["c32"].data_ptr(), 64, 0, 64, 64, 256, 1.0, splits, kstep, 64 * 64,
                  NV.stream_handle(bufs["a"].device))
    assert rc == EM_ERR_ARG
    _untouched(bufs)
