"""Every GEMM kernel of ``csrc/gemm.hip`` / ``csrc/gemm_f32.hip`` against an fp64 reference, bit for bit.

Operands are small nowhere-zero integers, so every fp32 partial sum is an exact integer in any order and the
result must EQUAL the reference (``_gemm_exact.py``; bf16 outputs after one round-to-nearest-even).  Operands,
masks, bias, outputs, ``ct``, ``colpart``, ``bits`` and workspaces live inside larger allocations whose surround
is NaN (inputs) or a sentinel (outputs): a tail that reads past K or the last row, a wrong leading dimension,
or a store outside ``[M, N]`` fails the test.  Only sigmoid / tanh use a bound, the derived one.

Groups (one named test or more each):
  a. any-layout 128-tile ``gemm_kernel<A_KC, B_KC>``      test_any_layout_*
  b. split-K on that kernel (``linear_wgrad(split_k=s)``)  test_splitk_*
  c. 256-tile ``gemm256_pp16_kernel``                       test_tile256_*
  d. ``gemm_k64_kernel``                                    test_k64_*
  e. ``wgrad_skinny_kernel``                                test_skinny_*
  f. ``em_gemm_f32``                                        test_f32_*
  g. transpose / colsum / rowsum / colpart_reduce           test_small_*
and the dispatch rule for bf16 outputs that are not 16-byte aligned: test_unaligned_bf16_*.
"""
import pytest
import torch

import _gemm_exact as GX

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]


def _ops(M, N, K, seed):
    """Logical A [M, K] (|A| <= 3) and B [K, N] (|B| <= 5), fp32 integers: one structured, one random side."""
    if seed % 2:
        return (GX.rand_int_operand(M, K, GX.A_MOD, seed, DEV, F32), GX.int_operand(K, N, 3, 1, GX.B_MOD, DEV, F32))
    return (GX.int_operand(M, K, 1, 5, GX.A_MOD, DEV, F32), GX.rand_int_operand(K, N, GX.B_MOD, seed, DEV, F32))


def _alpha16(K):
    """Power of two that keeps |alpha * sum| <= 15 (sigmoid / tanh cases; scaling by it is exact)."""
    a = 1.0
    while a * K > 1.0:
        a /= 2
    return a


def _mask_values(M, N, dact, seed):
    """Saved-activation values for act': integers around zero (relu), bf16-exact fractions (sigmoid / tanh)."""
    if dact == "relu":
        return GX.rand_ints((M, N), -2, 2, seed, DEV)
    if dact == "sigmoid":
        return GX.rand_ints((M, N), 1, 63, seed, DEV) / 64
    return GX.rand_ints((M, N), -31, 31, seed, DEV) / 32


def _bf16_case(M, N, K, a_kc, b_kc, out_dtype, *, alpha=1.0, beta=0.0, bias=0, act="none", dact=None,
               act_src="mask", ct=False, colpart=False, wbits=False, seed=0, close=False, col_off=0):
    """One ``LIN.gemm`` launch with everything guarded, then every output against the reference."""
    from euromillioner_amd.ops import linear as LIN

    A, B = _ops(M, N, K, seed)
    oks = []

    def keep(pair):
        oks.append(pair[1])
        return pair[0]

    a = keep(GX.guarded((A if a_kc else A.t().contiguous()).to(BF), pad_cols=8, name="a"))
    b = keep(GX.guarded((B.t().contiguous() if b_kc else B).to(BF), pad_cols=16, guard_rows=1, name="b"))
    bias_v = bias_t = mask_t = bits_t = mask_ref = c_old = ct_t = cp_t = None
    if bias:
        bias_v = GX.rand_ints((N,), -bias, bias, seed + 1, DEV)
        bias_t = keep(GX.guarded_flat(bias_v, poison="nan", name="bias"))
    if dact and act_src == "bits":
        on = GX.rand_ints((M, N), 0, 1, seed + 2, DEV).bool()
        bits_t = keep(GX.guarded_flat(GX.pack_bits(on), name="bits"))
        mask_ref = on.double()
    elif dact:
        mask_ref = _mask_values(M, N, dact, seed + 2)
        mask_t = keep(GX.guarded(mask_ref.to(BF), pad_cols=24, guard_rows=3, name="mask"))
    if wbits:
        bits_t = keep(GX.guarded_flat(GX.sentinel_like((M // 32, N), torch.int32, DEV), name="bits"))
    if beta != 0.0:
        c_old = GX.rand_ints((M, N), -9, 9, seed + 3, DEV, out_dtype)
        out = keep(GX.guarded(c_old, poison="sentinel", name="out"))
    else:
        out = keep(GX.guarded(GX.nan_like(M, N, out_dtype, DEV), poison="sentinel", col_off=col_off, name="out"))
    if ct:
        ct_t = keep(GX.guarded(GX.nan_like(N, M, BF, DEV), poison="sentinel", pad_cols=16, name="ct"))
    if colpart:
        cp_t = keep(GX.guarded_flat(GX.sentinel_like(((M // 128) * N,), F32, DEV), name="colpart"))
    LIN.gemm(a, a_kc, b, b_kc, out, M, N, K, bias=bias_t, act=act, dact_src=mask_t, dact=dact or "relu", alpha=alpha,
             beta=beta, ct=ct_t, colpart=cp_t, bits=bits_t)
    torch.cuda.synchronize()
    ref = GX.reference(A, B, alpha=alpha, beta=beta, c_old=c_old, bias=bias_v, act=act, dact=dact, mask=mask_ref)
    what = f"M={M} N={N} K={K} a_kc={a_kc} b_kc={b_kc} {out_dtype} act={act} dact={dact}/{act_src}"
    chk = GX.check_close if close else GX.check_exact
    chk(out, ref, "out " + what)
    if ct:
        chk(ct_t, ref.t(), "ct " + what)
    if colpart:
        GX.check_colpart(cp_t, ref, what="colpart " + what)
    if wbits:
        GX.check_bits(bits_t, ref, "bits " + what)
    for ok in oks:
        ok()


# ------------------------------------------------------------------------ a. any-layout 128-tile kernel
ANY_MN = [(1, 1), (1, 129), (127, 1), (127, 129), (129, 127), (129, 129), (385, 257)]  # 385 x 257: 4 x 3 = 12 tiles
ANY_K = [1, 7, 8, 63, 64, 65, 72, 136]


def _any_epilogue(e, dtype):
    kind = e % 4
    if kind == 0:
        return {}
    if kind == 1:
        return dict(bias=300, act="relu")  # sums + bias past 256: bf16 outputs have to round
    if kind == 2:
        return dict(dact="relu")
    if dtype == F32:
        return [dict(alpha=0.5, beta=-0.5), dict(alpha=2.0, beta=1.0)][e // 4 % 2]
    return dict(alpha=2.0, bias=300)  # (the bf16 store takes no beta)


@pytest.mark.parametrize("K", ANY_K)
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
def test_any_layout_shapes_and_epilogues(a_kc, b_kc, K):
    """gemm_kernel<A_KC, B_KC>: every layout x K edge (1, 7, 8, around and past one 64-tile) x M, N edges (1, one
    tile +- 1, 12 tiles for xcd_remap), fp32 and bf16 outputs; the epilogue (plain / bias + relu / relu act' /
    alpha + beta) rotates over the shapes so each meets every layout, dtype and K."""
    ki = ANY_K.index(K)
    for i, (M, N) in enumerate(ANY_MN):
        for d, dtype in enumerate((F32, BF)):
            _bf16_case(M, N, K, a_kc, b_kc, dtype, seed=10 * ki + i, **_any_epilogue(i + ki + 2 * d, dtype))


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
def test_any_layout_sigmoid_tanh_derived_bound(a_kc, b_kc):
    """One sigmoid and one tanh case of each kind (activation, act'), fp32 and bf16 outputs, |pre-activation|
    <= 16 (K = 8 and alpha, K = 136 and alpha): the derived elementwise bound of _gemm_exact, not a measured one."""
    for M, N, K in [(129, 127, 8), (127, 129, 136)]:
        al = _alpha16(K)
        for dtype in (F32, BF):
            _bf16_case(M, N, K, a_kc, b_kc, dtype, alpha=al, bias=1, act="sigmoid", close=True, seed=3)
            _bf16_case(M, N, K, a_kc, b_kc, dtype, alpha=al, bias=1, act="tanh", close=True, seed=4)
            _bf16_case(M, N, K, a_kc, b_kc, dtype, alpha=al, dact="sigmoid", close=True, seed=5)
            _bf16_case(M, N, K, a_kc, b_kc, dtype, alpha=al, dact="tanh", close=True, seed=6)


@pytest.mark.parametrize("K", [64, 192])
def test_any_layout_takes_fp32_act_on_256_shapes(K):
    """256-tile-shaped calls that must fall back to the any-layout kernel: fp32 output with act / act'."""
    for M, N in [(256, 256), (512, 256)]:
        _bf16_case(M, N, K, True, True, F32, bias=300, act="relu", seed=K)
        _bf16_case(M, N, K, True, True, F32, dact="relu", seed=K + 1)
        _bf16_case(M, N, K, True, False, F32, dact="relu", alpha=0.5, beta=1.0, seed=K + 2)


# -------------------------------------------------------------------------- b. split-K on that kernel
@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("M", [128, 200, 448])
def test_splitk_wgrad_exact(M, s):
    """linear_wgrad(split_k=s) -> em_gemm_bf16_splitk: reduction M = 128 (whole slices), 200 (last slice 72
    rows: ragged inside a K-tile), 448 with s = 3 (192 + 192 + 64: a short last slice); with and without beta."""
    from euromillioner_amd.ops import linear as LIN

    Nn, K = 70, 130
    P, Q = _ops(Nn, K, M, 7 * M + s)  # P = dz^T [Nn, M], Q = x [M, K]
    dz, dz_ok = GX.guarded(P.t().contiguous().to(BF), pad_cols=8, name="dz")
    x, x_ok = GX.guarded(Q.to(BF), pad_cols=16, name="x")
    for alpha, beta in [(1.0, 0.0), (0.5, 1.0), (2.0, -0.5)]:
        c_old = GX.rand_ints((Nn, K), -9, 9, M + s, DEV, F32) if beta else None
        out, out_ok = GX.guarded(c_old if beta else GX.nan_like(Nn, K, F32, DEV), pad_cols=4, poison="sentinel",
                                 name="out")
        LIN.linear_wgrad(dz, x, out=out, alpha=alpha, beta=beta, split_k=s)
        torch.cuda.synchronize()
        GX.check_exact(out, GX.reference(P, Q, alpha=alpha, beta=beta, c_old=c_old), f"M={M} s={s} beta={beta}")
        for ok in (dz_ok, x_ok, out_ok):
            ok()


# ----------------------------------------------------------------------------------- c. 256-tile kernel
T256_MN = [(256, 256), (512, 256), (256, 512)]


@pytest.mark.parametrize("K", [192, 320])
@pytest.mark.parametrize("M,N", T256_MN)
def test_tile256_nt_epilogues(M, N, K):
    """gemm256_pp16_kernel, both operands K-contiguous: fp32 + alpha / beta; bf16 plain and bias + relu writing
    ``bits``; relu act' from a mask and from ``bits``; with ``ct`` and ``colpart``; 3 and 5 K-tiles."""
    _bf16_case(M, N, K, True, True, F32, seed=1)
    _bf16_case(M, N, K, True, True, F32, alpha=0.5, beta=-0.5, seed=2)
    _bf16_case(M, N, K, True, True, BF, seed=3)
    _bf16_case(M, N, K, True, True, BF, ct=True, colpart=True, alpha=2.0, seed=4)
    _bf16_case(M, N, K, True, True, BF, bias=300, act="relu", wbits=True, seed=5)
    _bf16_case(M, N, K, True, True, BF, bias=300, act="relu", wbits=True, ct=True, colpart=True, seed=6)
    _bf16_case(M, N, K, True, True, BF, bias=300, act="relu", ct=True, seed=7)
    _bf16_case(M, N, K, True, True, BF, dact="relu", seed=8)
    _bf16_case(M, N, K, True, True, BF, dact="relu", ct=True, colpart=True, seed=9)
    _bf16_case(M, N, K, True, True, BF, dact="relu", act_src="bits", seed=10)
    _bf16_case(M, N, K, True, True, BF, dact="relu", act_src="bits", ct=True, colpart=True, seed=11)


@pytest.mark.parametrize("K", [192, 320])
@pytest.mark.parametrize("M,N", T256_MN)
def test_tile256_mn_operands(M, N, K):
    """The other layouts g_dispatch accepts: B MN-contiguous (dgrad form: bf16 out, none or act', ``colpart``,
    ``bits``) and both MN-contiguous (wgrad form: fp32 out, alpha / beta)."""
    _bf16_case(M, N, K, True, False, BF, seed=1)
    _bf16_case(M, N, K, True, False, BF, colpart=True, seed=2)
    _bf16_case(M, N, K, True, False, BF, dact="relu", seed=3)
    _bf16_case(M, N, K, True, False, BF, dact="relu", colpart=True, alpha=0.5, seed=4)
    _bf16_case(M, N, K, True, False, BF, dact="relu", act_src="bits", colpart=True, seed=5)
    _bf16_case(M, N, K, False, False, F32, seed=6)
    _bf16_case(M, N, K, False, False, F32, alpha=2.0, beta=1.0, seed=7)


@pytest.mark.parametrize("K", [64, 128])
def test_tile256_fp32_output_at_k64_k128(K):
    """K = 64 / 128 with an fp32 output also lands on the 256-tile kernel (1 and 2 K-tiles: its prologue paths)."""
    for M, N in T256_MN:
        _bf16_case(M, N, K, True, True, F32, seed=K)
        _bf16_case(M, N, K, True, True, F32, alpha=0.5, beta=1.0, seed=K + 1)
        _bf16_case(M, N, K, False, False, F32, beta=-0.5, seed=K + 2)
    _bf16_case(256, 256, K, True, False, BF, dact="relu", seed=K + 3)  # (B MN-contiguous is never the K64 kernel)


def test_tile256_sigmoid_tanh_derived_bound():
    al = _alpha16(192)
    _bf16_case(256, 256, 192, True, True, BF, alpha=al, bias=1, act="sigmoid", ct=True, close=True, seed=1)
    _bf16_case(256, 256, 192, True, True, BF, alpha=al, bias=1, act="tanh", close=True, seed=2)
    _bf16_case(256, 256, 192, True, True, BF, alpha=al, dact="sigmoid", close=True, seed=3)
    _bf16_case(256, 256, 192, True, False, BF, alpha=al, dact="tanh", close=True, seed=4)


# -------------------------------------------------------------------------------------- d. K64 kernel
@pytest.mark.parametrize("K", [64, 128])
@pytest.mark.parametrize("M,N", T256_MN)
def test_k64_epilogues(M, N, K):
    """gemm_k64_kernel (NT, bf16 out, K = 64 / 128): none and relu forward (relu writing ``bits``), relu act' from
    a mask (the 68 KB LDS variant) and from ``bits`` (the slim one); each with and without ``ct`` + ``colpart``;
    operands, mask and output are padded views."""
    for extra in (dict(), dict(ct=True, colpart=True), dict(ct=True), dict(colpart=True)):
        _bf16_case(M, N, K, True, True, BF, alpha=2.0, seed=1, **extra)
        _bf16_case(M, N, K, True, True, BF, bias=300, act="relu", wbits=True, seed=2, **extra)
        _bf16_case(M, N, K, True, True, BF, dact="relu", seed=3, **extra)
        _bf16_case(M, N, K, True, True, BF, dact="relu", act_src="bits", seed=4, **extra)
    _bf16_case(M, N, K, True, True, BF, bias=300, act="relu", seed=5)  # relu without bits


def test_k64_sigmoid_tanh_derived_bound():
    for K in (64, 128):
        al = _alpha16(K)
        _bf16_case(256, 256, K, True, True, BF, alpha=al, bias=1, act="sigmoid", ct=True, close=True, seed=1)
        _bf16_case(256, 256, K, True, True, BF, alpha=al, bias=1, act="tanh", close=True, seed=2)
        _bf16_case(256, 256, K, True, True, BF, alpha=al, dact="sigmoid", close=True, seed=3)
        _bf16_case(256, 256, K, True, True, BF, alpha=al, dact="tanh", ct=True, close=True, seed=4)


# ------------------------------------------------------------------------------------ e. skinny wgrad
def _skinny_case(K, W, J, trans, splits, kstep, alpha, beta, seed):
    from euromillioner_amd.ops import _native as NV

    Pt, Q = _ops(J, W, K, seed)  # Pt = P^T [J, K], Q [K, W]
    full = torch.full((K, 64), float("nan"), dtype=BF, device=DEV)  # P pad columns J .. 63 are NaN
    full[:, :J] = Pt.t().to(BF)
    pbuf, p_ok = GX.guarded(full, pad_cols=8, name="P")
    q, q_ok = GX.guarded(Q.to(BF), pad_cols=16, name="Q")
    shape = (W, J) if trans else (J, W)
    c_old = GX.rand_ints(shape, -9, 9, seed + 1, DEV, F32) if beta else None
    c, c_ok = GX.guarded(c_old if beta else GX.nan_like(*shape, F32, DEV), pad_cols=4, poison="sentinel", name="C")
    part, part_ok = GX.guarded_flat(GX.sentinel_like((splits * 64 * W,), F32, DEV), name="part")
    NV.call("em_wgrad_skinny", pbuf.data_ptr(), pbuf.stride(0), q.data_ptr(), q.stride(0), K, J, W, c.data_ptr(),
            c.stride(0), int(trans), float(alpha), float(beta), part.data_ptr(), splits, kstep,
            NV.stream_handle(c.device))
    torch.cuda.synchronize()
    ref = GX.reference(Pt, Q, alpha=alpha)
    if trans:
        ref = ref.t()
    if beta:
        ref = ref + beta * c_old.double()
    GX.check_exact(c, ref, f"K={K} W={W} J={J} trans={trans} splits={splits} kstep={kstep}")
    for ok in (p_ok, q_ok, c_ok, part_ok):
        ok()


@pytest.mark.parametrize("K,splits,kstep", [(64, 1, 64), (192, 1, 192), (512, 1, 512), (448, 2, 256)])
def test_skinny_wgrad_ring_tiles_per_slice(K, splits, kstep):
    """wgrad_skinny_kernel through em_wgrad_skinny with chosen splits / kstep.  64-row K-tiles per slice:
    K = 64 -> 1 (no second stage), K = 192 -> 3 (the first stage(t + 2): the ring's third slot), K = 512 -> 8
    (the ring wraps: stage(t + 2) into the slot of tile t - 1 and the vmcnt(12) steady-state wait, five times),
    K = 448 with kstep 256 -> slices of 4 and 3 tiles.  W = 256 / 512 (1 and 2 column blocks), J = 64 / 62 / 1
    with NaN in P's pad columns J .. 63, both ``trans`` values, alpha / beta; ``part`` and C guarded."""
    from euromillioner_amd.ops import linear as LIN  # noqa: F401  (registers em_wgrad_skinny's signature)

    i = 0
    for W in (256, 512):
        for J in (64, 62, 1):
            for trans in (False, True):
                alpha, beta = [(1.0, 0.0), (0.5, 1.0), (2.0, -0.5)][i % 3]
                _skinny_case(K, W, J, trans, splits, kstep, alpha, beta, seed=K + i)
                i += 1


@pytest.mark.parametrize("trans", [False, True])
def test_skinny_wgrad_through_linear_wgrad(trans):
    """The wrapper's own split arithmetic at the smallest shape ``_skinny_ok`` admits: batch 4096, 62 x 256 ->
    ``_wgrad_skinny`` picks 64 slices of one 64-row tile.  (The batch is the reduction and the API's minimum is
    4096, past the helpers' default K <= 2560: 15 * 4096 < 2^24 still holds and is asserted.)"""
    from euromillioner_amd.ops import linear as LIN

    Bn, J, W = 4096, 62, 256
    Pt, Q = _ops(J, W, Bn, 11)
    narrow, n_ok = GX.guarded(Pt.t().contiguous().to(BF), pad_cols=8, name="narrow")  # columns 62, 63: NaN poison
    wide, w_ok = GX.guarded(Q.to(BF), pad_cols=16, name="wide")
    dz, x = (wide, narrow) if trans else (narrow, wide)
    shape = (W, J) if trans else (J, W)
    c_old = GX.rand_ints(shape, -9, 9, 5, DEV, F32)
    out, out_ok = GX.guarded(c_old, pad_cols=8, poison="sentinel", name="out")
    assert LIN._skinny_ok(dz, x, out)
    LIN.linear_wgrad(dz, x, out=out, alpha=0.5, beta=-0.5)
    torch.cuda.synchronize()
    ref = GX.reference(Pt, Q, alpha=0.5, k_max=Bn)
    ref = (ref.t() if trans else ref) - 0.5 * c_old.double()
    GX.check_exact(out, ref, f"linear_wgrad skinny trans={trans}")
    for ok in (n_ok, w_ok, out_ok):
        ok()


# ---------------------------------------------------------------------------------------- f. fp32 GEMM
def _f32_case(M, N, K, a_kc, b_kc, *, guard=True, alpha=1.0, beta=0.0, bias=0, act="none", dact=None, splits=1,
              colpart=False, seed=0, close=False):
    from euromillioner_amd.ops import linear_f32 as LF

    A, B = _ops(M, N, K, seed)
    oks = []

    def place(t, name, pad=4, poison="nan"):
        if not guard:
            return t.contiguous()
        v, ok = GX.guarded(t, pad_cols=pad, poison=poison, name=name)
        oks.append(ok)
        return v

    a = place(A if a_kc else A.t().contiguous(), "a")
    b = place(B.t().contiguous() if b_kc else B, "b", pad=8)
    bias_v = bias_t = mask_ref = mask_t = c_old = cp_t = None
    if bias:
        bias_v = GX.rand_ints((N,), -bias, bias, seed + 1, DEV)
        bias_t, ok = GX.guarded_flat(bias_v, poison="nan", name="bias")
        oks.append(ok)
    if dact:
        mask_ref = _mask_values(M, N, dact, seed + 2)
        mask_t = place(mask_ref, "dact_src", pad=12)
    if beta != 0.0:
        c_old = GX.rand_ints((M, N), -9, 9, seed + 3, DEV, F32)
    out = place(c_old.clone() if beta != 0.0 else GX.nan_like(M, N, F32, DEV), "out", poison="sentinel")
    if colpart:
        cp_t, ok = GX.guarded_flat(GX.sentinel_like((-(-M // 128) * N,), F32, DEV), name="colpart")
        oks.append(ok)
    LF.gemm_f32(a, a_kc, b, b_kc, out, M, N, K, bias=bias_t, act=act, dact_src=mask_t, dact=dact or "relu",
                alpha=alpha, beta=beta, splits=splits, colpart=cp_t)
    torch.cuda.synchronize()
    ref = GX.reference(A, B, alpha=alpha, beta=beta, c_old=c_old, bias=bias_v, act=act, dact=dact, mask=mask_ref)
    what = f"f32 M={M} N={N} K={K} a_kc={a_kc} b_kc={b_kc} guard={guard} act={act} dact={dact} splits={splits}"
    (GX.check_close if close else GX.check_exact)(out, ref, "out " + what)
    if colpart:
        GX.check_colpart(cp_t, ref, what="colpart " + what)
    for ok in oks:
        ok()


F32_MN = [(1, 1), (1, 129), (127, 1), (127, 129), (129, 127), (129, 129)]
F32_K = [1, 5, 15, 16, 17, 40]


def _f32_epilogue(e):
    return [dict(), dict(bias=300, act="relu"), dict(dact="relu"), dict(alpha=0.5, beta=-0.5),
            dict(colpart=True), dict(colpart=True, alpha=2.0, beta=1.0, dact="relu")][e % 6]


@pytest.mark.parametrize("K", F32_K)
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
def test_f32_shapes_and_epilogues(a_kc, b_kc, K):
    """em_gemm_f32: every layout x K edge (1, 5, around one 16-tile, 40) x M, N in {1, 127, 129}, twice: as padded
    views with NaN pads (16-byte aligned rows: f_load's vector branch and its tails) and as contiguous operands
    (odd K / odd M, N: rows not 16-byte aligned, f_load's scalar branch).  The epilogue (plain, bias + relu,
    relu act', alpha + beta, colpart, colpart + act' + beta) rotates over the shapes."""
    ki = F32_K.index(K)
    for i, (M, N) in enumerate(F32_MN):
        for g, guard in enumerate((True, False)):
            _f32_case(M, N, K, a_kc, b_kc, guard=guard, seed=10 * ki + i, **_f32_epilogue(i + ki + 3 * g))


@pytest.mark.parametrize("splits", [2, 3])
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
def test_f32_splitk(a_kc, b_kc, splits):
    """gridDim.y K-slices with K no multiple of ``splits`` (slices start off the 16-byte grid)."""
    for M, N, K in [(127, 129, 5), (129, 127, 17), (1, 129, 40), (129, 1, 1)]:
        if K % splits == 0:
            continue
        for guard in (True, False):
            _f32_case(M, N, K, a_kc, b_kc, guard=guard, splits=splits, seed=K)
            _f32_case(M, N, K, a_kc, b_kc, guard=guard, splits=splits, alpha=0.5, beta=1.0, seed=K + 1)


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
def test_f32_sigmoid_tanh_derived_bound(a_kc, b_kc):
    for M, N, K in [(129, 127, 5), (127, 129, 40)]:
        al = _alpha16(K)
        _f32_case(M, N, K, a_kc, b_kc, alpha=al, bias=1, act="sigmoid", close=True, seed=1)
        _f32_case(M, N, K, a_kc, b_kc, alpha=al, bias=1, act="tanh", close=True, seed=2)
        _f32_case(M, N, K, a_kc, b_kc, alpha=al, dact="sigmoid", close=True, seed=3)
        _f32_case(M, N, K, a_kc, b_kc, alpha=al, dact="tanh", close=True, seed=4)


# -------------------------------------------------------------------------------------- g. small kernels
@pytest.mark.parametrize("R", [63, 64, 65])
def test_small_transpose_exact(R):
    from euromillioner_amd.ops import linear as LIN

    for C in (1, 63, 64, 65, 130):
        src = GX.rand_int_operand(R, C, GX.B_MOD, R + C, DEV, BF)
        x, x_ok = GX.guarded(src, pad_cols=8, name="x")
        out, out_ok = GX.guarded(GX.nan_like(C, R, BF, DEV), pad_cols=16, poison="sentinel", name="out")
        LIN.transpose(x, out)
        torch.cuda.synchronize()
        assert torch.equal(out, src.t()), (R, C)
        x_ok()
        out_ok()


@pytest.mark.parametrize("M", [1, 511, 512, 513, 1025])
def test_small_colsum_exact(M):
    """colsum_partial_kernel's CS_ROWS = 512 row chunks (511 / 512 / 513) and its 512-column groups (tail N)."""
    from euromillioner_amd.ops import linear as LIN

    for N in (7, 64, 523):
        src = GX.rand_int_operand(M, N, GX.B_MOD, M + N, DEV, BF)
        x, x_ok = GX.guarded(src, pad_cols=8, name="x")
        want = src.double().sum(0)
        ws, ws_ok = GX.guarded_flat(GX.sentinel_like((max(1, (M + 511) // 512 * N),), F32, DEV), name="ws")
        out, out_ok = GX.guarded_flat(GX.nan_like(1, N, F32, DEV).view(N), name="out")
        LIN.colsum(x, out=out, ws=ws)
        old = GX.rand_ints((N,), -9, 9, N, DEV)
        acc, acc_ok = GX.guarded_flat(old, name="acc")
        LIN.colsum(x, out=acc, accumulate=True, scale=0.5, ws=ws)
        torch.cuda.synchronize()
        assert torch.equal(out.double(), want), (M, N)
        assert torch.equal(acc.double(), old.double() + 0.5 * want), (M, N)
        for ok in (x_ok, ws_ok, out_ok, acc_ok):
            ok()


@pytest.mark.parametrize("C", [1, 7, 8, 511, 512, 513, 1031])
def test_small_rowsum_exact(C):
    from euromillioner_amd.ops import linear as LIN

    for R in (1, 5, 9):
        src = GX.rand_int_operand(R, C, GX.B_MOD, R + C, DEV, BF)
        x, x_ok = GX.guarded(src, pad_cols=8, name="x")
        want = src.double().sum(1)
        out, out_ok = GX.guarded_flat(GX.nan_like(1, R, F32, DEV).view(R), name="out")
        LIN.rowsum(x, out=out)
        old = GX.rand_ints((R,), -9, 9, C, DEV)
        acc, acc_ok = GX.guarded_flat(old, name="acc")
        LIN.rowsum(x, out=acc, accumulate=True, scale=2.0)
        torch.cuda.synchronize()
        assert torch.equal(out.double(), want), (R, C)
        assert torch.equal(acc.double(), old.double() + 2.0 * want), (R, C)
        for ok in (x_ok, out_ok, acc_ok):
            ok()


@pytest.mark.parametrize("parts", [1, 15, 16, 17, 127, 128, 129, 300])
def test_small_colpart_reduce_exact(parts):
    """colsum_final_kernel: 16 groups (15 / 16 / 17 parts), its 8-deep unrolled loop (from 113 parts on) and the
    64-column blocks (N = 1, 64, 65)."""
    from euromillioner_amd.ops import linear as LIN

    for N in (1, 64, 65):
        src = GX.rand_ints((parts, N), -1000, 1000, parts + N, DEV)
        part, part_ok = GX.guarded_flat(src, poison="nan", name="part")
        want = src.double().sum(0)
        out, out_ok = GX.guarded_flat(GX.nan_like(1, N, F32, DEV).view(N), name="out")
        LIN.colpart_reduce(part, parts, N, out)
        old = GX.rand_ints((N,), -9, 9, N, DEV)
        acc, acc_ok = GX.guarded_flat(old, name="acc")
        LIN.colpart_reduce(part, parts, N, acc, accumulate=True, scale=0.5)
        torch.cuda.synchronize()
        assert torch.equal(out.double(), want), (parts, N)
        assert torch.equal(acc.double(), old.double() + 0.5 * want), (parts, N)
        for ok in (part_ok, out_ok, acc_ok):
            ok()


# ------------------------------------------------------------ bf16 outputs that are not 16-byte aligned
@pytest.mark.parametrize("K", [64, 192])
def test_unaligned_bf16_output_takes_the_scalar_epilogue(K):
    """A bf16 output view at a column offset of 4 elements (8 bytes) on a 256-tile shape: the 256-tile and K64
    epilogues store 16-byte vectors, so gemm_impl routes the call to the any-layout kernel -- exact result,
    surround untouched.  Likewise an act' mask at such an offset."""
    from euromillioner_amd.ops import linear as LIN

    _bf16_case(256, 256, K, True, True, BF, col_off=4, seed=K)
    _bf16_case(256, 256, K, True, True, BF, bias=300, act="relu", col_off=4, seed=K + 1)
    _bf16_case(256, 256, K, True, False, BF, col_off=4, seed=K + 2)
    # the mask misaligned, the output aligned
    M = N = 256
    A, B = _ops(M, N, K, K + 3)
    a, b = LIN.aligned(A.to(BF)), LIN.aligned(B.t().contiguous().to(BF))
    mask_ref = _mask_values(M, N, "relu", 9)
    mask, mask_ok = GX.guarded(mask_ref.to(BF), pad_cols=8, col_off=4, name="mask")
    out, out_ok = GX.guarded(GX.nan_like(M, N, BF, DEV), poison="sentinel", name="out")
    assert mask.data_ptr() % 16 == 8 and out.data_ptr() % 16 == 0
    LIN.gemm(a, True, b, True, out, M, N, K, dact_src=mask, dact="relu")
    torch.cuda.synchronize()
    GX.check_exact(out, GX.reference(A, B, dact="relu", mask=mask_ref), "misaligned mask")
    mask_ok()
    out_ok()


@pytest.mark.parametrize("K", [64, 192])
def test_unaligned_bf16_output_with_colpart_is_refused(K):
    """The same view with ``colpart`` (256-tile / K64 only) raises and leaves output and colpart bit-identical."""
    from euromillioner_amd.ops import linear as LIN

    M = N = 256
    A, B = _ops(M, N, K, 1)
    a, b = LIN.aligned(A.to(BF)), LIN.aligned(B.t().contiguous().to(BF))
    out, out_ok = GX.guarded(GX.nan_like(M, N, BF, DEV), poison="sentinel", col_off=4, name="out")
    cp, cp_ok = GX.guarded_flat(GX.sentinel_like((M // 128 * N,), F32, DEV), name="colpart")
    out0, cp0 = out.view(torch.int16).clone(), cp.view(torch.int32).clone()
    with pytest.raises(ValueError):
        LIN.gemm(a, True, b, True, out, M, N, K, colpart=cp)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), out0) and torch.equal(cp.view(torch.int32), cp0)
    out_ok()
    cp_ok()
