"""``csrc/adam.hip`` (K6) against the fp64 reference of ``_adam_ref.py``, without going through the train kernel:
the slab sums exactly (integer slabs, power-of-two scale) on the vector and the scalar path at every loop edge,
slab sum + Adam within the derived bounds in modes 0 / 1 / 2 and with ``pre``, the flat Adam on every loop path
with its bf16 shadow, the fp32 -> bf16 cast on a directed vector and past the grid, and what the entries refuse.

Buffer discipline: slab rows ``>= nslab`` and columns ``P..stride-1`` are NaN, ``loss_slabs`` entries ``>= nslab``
are NaN, and every output lies in front of a sentinel guard that must survive each launch.
"""
import numpy as np
import pytest
import torch

import _adam_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = {1: 0x5C, 2: 0x7A5C, 4: 0x7A5C7A5C}
IVIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
P_TOTAL, SLAB_STRIDE = 16448, 16640
IMG_B2 = 54528 - 256
POOL_SHIFT = 7919  # step k of a case reads the integer pool from k * POOL_SHIFT


@pytest.fixture(autouse=True)
def _no_launch_after_a_gpu_error():
    """A HIP error ends the session: nothing more is launched on a device that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, not continuing: {e}", returncode=3)


def _fm():
    from euromillioner_amd.ops import fused_mlp as FM

    return FM


class Guarded:
    """``n`` elements followed by a sentinel guard; ``t`` is the view the kernels get."""

    def __init__(self, n, dtype, init=None, poison=True):
        self.n = n
        self.buf = torch.zeros(n + GUARD, dtype=dtype, device="cuda")
        self.iv = self.buf.view(IVIEW[self.buf.element_size()])
        self.sent = SENT[self.buf.element_size()]
        if poison:
            self.iv[:] = self.sent
        self.iv[n:] = self.sent
        self.t = self.buf[:n]
        if init is not None:
            self.t.copy_(torch.as_tensor(init).to(dtype))

    def intact(self):
        return bool((self.iv[self.n:] == self.sent).all())

    def poisoned(self):
        return bool((self.iv[:self.n] == self.sent).all())

    def np(self):
        return self.t.cpu().numpy()

    def bits(self):
        return self.iv[:self.n].clone()


def _all_intact(*gs):
    torch.cuda.synchronize()
    for i, g in enumerate(gs):
        assert g is None or g.intact(), f"guard of buffer {i} was written"


@pytest.fixture(scope="module")
def pool():
    """One pool of nowhere-zero integers in [-4095, 4095] (fp32), on the host and on the GPU, shared by every
    exact case and left unchanged."""
    return _make_pool()


def _make_pool():
    host = R.int_slabs(1, 513 * P_TOTAL + 4 * POOL_SHIFT, seed=1)[0]
    return host, torch.from_numpy(host).cuda()


def _pool_vals(pool, nslab, P, k=0):
    host, dev = pool
    o = k * POOL_SHIFT
    return host[o:o + nslab * P].reshape(nslab, P), dev[o:o + nslab * P].view(nslab, P)


def _make_slabs(nslab, P, stride, offset=0):
    """[nslab + 2, stride] view, all NaN, ``offset`` floats into its allocation (0: 16-B aligned)."""
    rows = nslab + 2
    flat = torch.full((rows * stride + 8,), float("nan"), device="cuda")
    view = flat[offset:offset + rows * stride].view(rows, stride)
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 * offset) % 16
    return view


def _path(P, stride, slabs):
    return "vector" if P % 64 == 0 and stride % 4 == 0 and slabs.data_ptr() % 16 == 0 else "scalar"


def _hp(wd):
    return torch.from_numpy(R.hp_f32(wd=wd)).cuda()


def _state(t):
    return Guarded(2, torch.int32, init=[t, 0])


def _loss(nslab, seed=0):
    """integer loss partials with a NaN tail, and their exact sum"""
    rng = np.random.default_rng(seed)
    vals = rng.integers(1, 64, size=nslab).astype(np.float32)
    t = torch.full((nslab + 5,), float("nan"), device="cuda")
    t[:nslab] = torch.from_numpy(vals).cuda()
    return t, float(vals.astype(np.float64).sum())


LOSS_SCALE = 2.0 ** -7

# ---------------------------------------------------------------- a. slab sums, exact (mode 1)

VEC_SHAPES = [(64, 64), (64, 68), (64, 16640), (128, 128), (128, 132), (128, 16640), (16448, 16448), (16448, 16452),
              (16448, 16640)]
VEC_NSLAB = [1, 2, 15, 16, 17, 239, 240, 241, 242, 243, 244, 245, 255, 256, 257, 272, 511, 512, 513]
# (P, stride, offset in floats of the slab view)
SCALAR_SHAPES = [(1, 1, 0), (63, 63, 0), (65, 68, 0), (100, 104, 0), (128, 130, 0), (128, 132, 1)]
SCALAR_NSLAB = [1, 15, 16, 17, 111, 112, 113, 127, 128, 129, 240, 256, 257]
POW2_SCALE = 2.0 ** -10


def _mode1(slabs, nslab, P, scale, loss=None):
    """One mode-1 launch into poisoned, guarded buffers; params / m / v / state must come back untouched."""
    FM = _fm()
    params, m, v, grad_io = (Guarded(P, torch.float32) for _ in range(4))
    state = Guarded(2, torch.int32)
    loss_out = Guarded(1, torch.float32)
    FM.adam_slab(slabs, nslab, scale, params.t, m.t, v.t, _hp(0.0), state.t, mode=1, grad_io=grad_io.t,
                 loss_slabs=loss, loss_out=loss_out.t if loss is not None else None, loss_scale=LOSS_SCALE)
    _all_intact(params, m, v, grad_io, state, loss_out)
    for g in (params, m, v, state):
        assert g.poisoned(), "mode 1 wrote params / m / v / state"
    return grad_io.np(), loss_out


def _slab_exact_case(pool, P, stride, nslab, offset, path):
    host, dev = _pool_vals(pool, nslab, P)
    slabs = _make_slabs(nslab, P, stride, offset)
    slabs[:nslab, :P] = dev
    assert _path(P, stride, slabs) == path
    got, _ = _mode1(slabs, nslab, P, POW2_SCALE)
    assert R.slab_exact(got, host, nslab, P, POW2_SCALE), (
        f"{int((got.astype(np.float64) != R.slab_sum(host, nslab, P, POW2_SCALE)).sum())} of {P} sums differ")
    return got


@pytest.mark.parametrize("nslab", VEC_NSLAB)
@pytest.mark.parametrize("P,stride", VEC_SHAPES)
def test_slab_sum_exact_vector(pool, P, stride, nslab):
    _slab_exact_case(pool, P, stride, nslab, 0, "vector")


@pytest.mark.parametrize("nslab", SCALAR_NSLAB)
@pytest.mark.parametrize("P,stride,offset", SCALAR_SHAPES)
def test_slab_sum_exact_scalar(pool, P, stride, offset, nslab):
    _slab_exact_case(pool, P, stride, nslab, offset, "scalar")


@pytest.mark.parametrize("nslab", [17, 241, 257])
def test_slab_sum_paths_agree(pool, nslab):
    a = _slab_exact_case(pool, 128, 132, nslab, 0, "vector")
    b = _slab_exact_case(pool, 128, 132, nslab, 1, "scalar")
    c = _slab_exact_case(pool, 128, 130, nslab, 0, "scalar")
    assert np.array_equal(a, b) and np.array_equal(a, c)


@pytest.mark.parametrize("offset,path", [(0, "vector"), (1, "scalar")])
def test_slab_sum_float_within_gamma_bound(offset, path):
    nslab, P, stride, scale = 257, 128, 132, 1.0 / 3.0
    x = np.random.default_rng(17).standard_normal((nslab, P)).astype(np.float32)
    slabs = _make_slabs(nslab, P, stride, offset)
    slabs[:nslab, :P] = torch.from_numpy(x).cuda()
    assert _path(P, stride, slabs) == path
    got, _ = _mode1(slabs, nslab, P, scale)
    ratio = np.abs(got.astype(np.float64) - R.slab_sum(x, nslab, P, scale)) / (2 * R.slab_sum_bound(x, nslab, P, scale))
    print(f"ADAMRATIO slab_float {path} {ratio.max():.4f}")
    assert ratio.max() <= 1.0


# ---------------------------------------------------------------- b. slab sum + Adam

class SlabRun:
    """Guarded optimizer state of ``P`` parameters from the reference inputs of step ``t0 + 1``."""

    def __init__(self, P, wd, t0=0, seed=0, img=False):
        _, w, m, v = R.adam_inputs(P, t0 + 1, seed=seed)
        self.P, self.wd = P, wd
        self.params, self.m, self.v = (Guarded(P, torch.float32, init=x) for x in (w, m, v))
        self.state = _state(t0)
        self.hp = _hp(wd)
        self.loss_out = Guarded(1, torch.float32)
        self.img = Guarded(54528, torch.uint8) if img else None
        if img:
            self.img.iv[:self.img.n] = 0xAB

    def guards(self):
        _all_intact(self.params, self.m, self.v, self.state, self.loss_out, self.img)

    def host(self):
        return self.params.np(), self.m.np(), self.v.np()

    def bits(self):
        return [g.bits() for g in (self.params, self.m, self.v, self.state)]


def _check_step(run, before, gsum, t, scale, tag, where=None):
    ref = R.adam_step(gsum, *before, R.hp_f32(wd=run.wd), t, scale)
    r = R.ratios(*run.host(), ref, where)
    print(f"ADAMRATIO {tag} w {r['w']:.4f} m {r['m']:.4f} v {r['v']:.4f}")
    assert max(r.values()) <= 1.0, (tag, t, r)
    return ref


def _slab_adam_case(pool, P, stride, nslab, wd, scale, pre=False, offset=0, steps=3):
    FM = _fm()
    slabs = _make_slabs(nslab, P, stride, offset)
    path = _path(P, stride, slabs)
    run = SlabRun(P, wd, seed=nslab)
    for k in range(steps):
        t = k + 1
        host, dev = _pool_vals(pool, nslab, P, k)
        slabs[:nslab, :P] = dev
        loss, loss_sum = _loss(nslab, seed=k)
        before = run.host()
        if pre:
            run.state.t[0] = t  # what the train kernel's advance_step does
        FM.adam_slab(slabs, nslab, scale, run.params.t, run.m.t, run.v.t, run.hp, run.state.t, mode=0,
                     loss_slabs=loss, loss_out=run.loss_out.t, loss_scale=LOSS_SCALE, pre=pre)
        run.guards()
        _check_step(run, before, R.slab_sum(host, nslab, P, 1.0), t, scale, f"slab_{path}")
        assert run.state.np().tolist() == [t, 0]
        assert float(run.loss_out.np()[0]) == loss_sum * LOSS_SCALE


ADAM_SHAPES = [(128, 132, n) for n in (1, 240, 241, 242, 243, 244, 257)] + [(16448, 16640, 256)] + [
    (100, 104, n) for n in (1, 113, 129)]


@pytest.mark.parametrize("scale", [POW2_SCALE, 1.0 / 3.0], ids=["pow2", "third"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("P,stride,nslab", ADAM_SHAPES)
def test_slab_adam_three_steps(pool, P, stride, nslab, wd, scale):
    _slab_adam_case(pool, P, stride, nslab, wd, scale)


@pytest.mark.parametrize("P,stride,nslab", [(128, 132, 241), (128, 132, 17), (16448, 16640, 256), (100, 104, 113)])
def test_slab_adam_pre_reads_the_counter_as_is(pool, P, stride, nslab):
    _slab_adam_case(pool, P, stride, nslab, 0.01, 1.0 / 3.0, pre=True)


@pytest.mark.parametrize("P", [100, 128, 16448])
@pytest.mark.parametrize("t0", [0, 49])
def test_adam_mode2_from_grad_io(P, t0):
    FM = _fm()
    run = SlabRun(P, 0.01, t0=t0, seed=P + t0)
    for k in range(3):
        t = t0 + k + 1
        g = R.adam_inputs(P, 1, seed=1000 + k)[0]
        grad_io = Guarded(P, torch.float32, init=g)
        before = run.host()
        FM.adam_slab(None, 0, 1.0, run.params.t, run.m.t, run.v.t, run.hp, run.state.t, mode=2, grad_io=grad_io.t)
        run.guards()
        _all_intact(grad_io)
        assert np.array_equal(grad_io.np(), g)
        _check_step(run, before, g, t, 1.0, "mode2_scalar")
        assert run.state.np().tolist() == [t, 0]
        assert run.loss_out.poisoned()


@pytest.mark.parametrize("P,stride,nslab,offset", [(128, 132, 241, 0), (16448, 16640, 256, 0), (100, 104, 113, 0),
                                                   (128, 132, 129, 1)])
@pytest.mark.parametrize("scale", [POW2_SCALE, 1.0 / 3.0], ids=["pow2", "third"])
def test_mode0_equals_mode1_then_mode2_bit_for_bit(pool, P, stride, nslab, offset, scale):
    FM = _fm()
    host, dev = _pool_vals(pool, nslab, P)
    slabs = _make_slabs(nslab, P, stride, offset)
    slabs[:nslab, :P] = dev
    loss, loss_sum = _loss(nslab)
    a, b = SlabRun(P, 0.01, t0=1, seed=3), SlabRun(P, 0.01, t0=1, seed=3)
    grad_io = Guarded(P, torch.float32)
    FM.adam_slab(slabs, nslab, scale, a.params.t, a.m.t, a.v.t, a.hp, a.state.t, mode=0, loss_slabs=loss,
                 loss_out=a.loss_out.t, loss_scale=LOSS_SCALE)
    FM.adam_slab(slabs, nslab, scale, b.params.t, b.m.t, b.v.t, b.hp, b.state.t, mode=1, grad_io=grad_io.t,
                 loss_slabs=loss, loss_out=b.loss_out.t, loss_scale=LOSS_SCALE)
    torch.cuda.synchronize()
    assert b.state.np().tolist() == [1, 0] and float(b.loss_out.np()[0]) == loss_sum * LOSS_SCALE
    FM.adam_slab(slabs, nslab, scale, b.params.t, b.m.t, b.v.t, b.hp, b.state.t, mode=2, grad_io=grad_io.t)
    a.guards(), b.guards(), _all_intact(grad_io)
    for name, x, y in zip(("params", "m", "v", "state"), a.bits(), b.bits()):
        assert torch.equal(x, y), f"{name}: {int((x != y).sum())} words differ between mode 0 and mode 1 -> 2"
    assert a.state.np().tolist() == [2, 0] and float(a.loss_out.np()[0]) == loss_sum * LOSS_SCALE


@pytest.mark.parametrize("P,stride,offset", [(128, 132, 0), (128, 132, 1)], ids=["vector", "scalar"])
@pytest.mark.parametrize("mode", [0, 1])
def test_loss_pointers_are_optional(pool, P, stride, offset, mode):
    FM = _fm()
    nslab = 65
    host, dev = _pool_vals(pool, nslab, P)
    slabs = _make_slabs(nslab, P, stride, offset)
    slabs[:nslab, :P] = dev
    loss, loss_sum = _loss(nslab)
    results = []
    for use_slabs, use_out in ((True, True), (True, False), (False, True), (False, False)):
        run = SlabRun(P, 0.0, t0=1, seed=5)
        grad_io = Guarded(P, torch.float32)
        FM.adam_slab(slabs, nslab, POW2_SCALE, run.params.t, run.m.t, run.v.t, run.hp, run.state.t, mode=mode,
                     grad_io=grad_io.t if mode else None, loss_slabs=loss if use_slabs else None,
                     loss_out=run.loss_out.t if use_out else None, loss_scale=LOSS_SCALE)
        run.guards(), _all_intact(grad_io)
        if use_slabs and use_out:
            assert float(run.loss_out.np()[0]) == loss_sum * LOSS_SCALE
        else:
            assert run.loss_out.poisoned()
        results.append(run.bits() + [grad_io.bits()])
    for other in results[1:]:
        assert all(torch.equal(x, y) for x, y in zip(results[0], other))


@pytest.mark.parametrize("with_img", [True, False])
def test_pad_slots_and_weight_image(pool, with_img):
    FM = _fm()
    P, stride, nslab, scale = P_TOTAL, SLAB_STRIDE, 9, 1.0 / 3.0
    assert FM.P_TOTAL == P and FM.SLAB_STRIDE == stride and FM.IMG_BYTES == 54528
    pad = FM.pad_mask().numpy() == 0
    assert pad.sum() == 128 + 2 * 128 + 2
    host, dev = _pool_vals(pool, nslab, P)
    slabs = _make_slabs(nslab, P, stride)
    slabs[:nslab, :P] = dev
    run = SlabRun(P, 0.01, t0=1, seed=8, img=with_img)
    padt = torch.from_numpy(pad).cuda()
    run.params.t[padt], run.m.t[padt], run.v.t[padt] = 123.0, -3.0, 7.0  # garbage in the pad slots
    before = run.host()
    FM.adam_slab(slabs, nslab, scale, run.params.t, run.m.t, run.v.t, run.hp, run.state.t, mode=0,
                 img=run.img.t if with_img else None)
    run.guards()
    assert run.state.np().tolist() == [2, 0]
    gsum = R.slab_sum(host, nslab, P, 1.0)
    if not with_img:  # pad slots are parameters like any other
        _check_step(run, before, gsum, 2, scale, "slab_vector")
        return
    _check_step(run, before, gsum, 2, scale, "slab_vector", where=~pad)
    for x in run.host():
        assert np.all(x[pad] == 0)
    packed = Guarded(54528, torch.uint8)
    packed.iv[:packed.n] = 0xAB
    FM.pack(run.params.t, packed.t)
    _all_intact(packed)
    assert torch.equal(run.img.t, packed.t), f"{int((run.img.t != packed.t).sum())} image bytes differ from pack()"
    b2 = run.img.t[IMG_B2:IMG_B2 + 256].view(torch.float32).cpu().numpy()
    assert b2[52] == np.float32(-1.0e30) and b2[53] == np.float32(-1.0e30)  # out_phys(62), out_phys(63)
    assert np.array_equal(b2[:52], run.params.np()[P - 64:P - 12])


GRAPH_SHAPES = [(128, 132, 241), (16448, 16640, 256), (100, 104, 113)]


def _graph_replay_case(pool, P, stride, nslab):
    """One linear hipGraph of a single mode-0 launch, captured once and replayed three times, against three
    eager launches."""
    FM = _fm()
    host, dev = _pool_vals(pool, nslab, P)
    slabs = _make_slabs(nslab, P, stride)
    slabs[:nslab, :P] = dev
    loss, loss_sum = _loss(nslab)
    a, b = SlabRun(P, 0.01, seed=4), SlabRun(P, 0.01, seed=4)

    def launch(run):
        FM.adam_slab(slabs, nslab, 1.0 / 3.0, run.params.t, run.m.t, run.v.t, run.hp, run.state.t, mode=0,
                     loss_slabs=loss, loss_out=run.loss_out.t, loss_scale=LOSS_SCALE)

    for _ in range(3):
        launch(a)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(gr, stream=s):
            launch(b)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert b.state.np().tolist() == [0, 0]  # capture runs nothing
    for _ in range(3):
        gr.replay()
    a.guards(), b.guards()
    for name, x, y in zip(("params", "m", "v", "state"), a.bits(), b.bits()):
        assert torch.equal(x, y), f"{name}: {int((x != y).sum())} words differ between eager and replay"
    assert b.state.np().tolist() == [3, 0] and float(b.loss_out.np()[0]) == loss_sum * LOSS_SCALE


def test_graph_replay_equals_eager():
    """Runs in a process of its own (this file as a script): capturing needs a side stream, and the streams a
    process has used decide which hardware queue a later one gets, which the co-scheduling tests of this suite
    (``test_xgmi_proxy_gpu.py``) are sensitive to."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:]
    for P, stride, nslab in GRAPH_SHAPES:
        assert f"graph replay ok P={P} stride={stride} nslab={nslab}" in p.stdout


# ---------------------------------------------------------------- c. flat Adam, every loop path

# n = k * 1024 * C + r with C the CU count: tails only (k = 0), around the unrolled main loop, main + tails
FLAT_LENGTHS = [(0, r) for r in (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 1027)] + [
    (3, 3), (3, 4), (4, 0), (4, 1), (4, 4), (4, 5), (6, 7), (8, 3)]


def _flat_case(k, r, bf16_grad, scale, wd, t0=0):
    from euromillioner_amd.ops import _native as N

    FM = _fm()
    n = k * 1024 * N.cu_count() + r
    tag = f"flat_{'main' if k >= 4 or (k, r) == (3, 4) else 'tail'}_{'bf16g' if bf16_grad else 'f32g'}"
    print(f"flat Adam over n = {n} ({N.cu_count()} CUs)")
    a, b = SlabRun(n, wd, t0=t0, seed=r + k), SlabRun(n, wd, t0=t0, seed=r + k)
    shadow = Guarded(n, torch.bfloat16)
    for j in range(3):
        t = t0 + j + 1
        g = torch.from_numpy(R.adam_inputs(n, 1, seed=50 + j)[0]).cuda()
        if bf16_grad:
            g = g.bfloat16()
        before = a.host()
        FM.adam_flat(a.params.t, g, a.m.t, a.v.t, a.hp, a.state.t, grad_scale=scale, shadow=shadow.t)
        FM.adam_flat(b.params.t, g, b.m.t, b.v.t, b.hp, b.state.t, grad_scale=scale, shadow=None)
        a.guards(), b.guards(), _all_intact(shadow)
        _check_step(a, before, g.float().cpu().numpy(), t, scale, tag)
        assert a.state.np().tolist() == [t, 0]
        w = a.params.np()
        assert R.bf16_bits_match(shadow.t.view(torch.int16).cpu().numpy(), w), "shadow != RNE bf16 of params"
        assert torch.equal(shadow.t, a.params.t.bfloat16())
        for name, x, y in zip(("params", "m", "v", "state"), a.bits(), b.bits()):
            assert torch.equal(x, y), f"{name} depends on the shadow pointer"


@pytest.mark.parametrize("bf16_grad", [False, True], ids=["f32g", "bf16g"])
@pytest.mark.parametrize("k,r", FLAT_LENGTHS, ids=[f"{k}C+{r}" for k, r in FLAT_LENGTHS])
def test_adam_flat_every_loop_path(k, r, bf16_grad):
    # (scale, wd) paired, not crossed: the pairing rotates from one length to the next, and the two gradient
    # types of a length take complementary pairs
    pairs = [(1.0, 0.0), (1.0 / 3.0, 0.01), (1.0, 0.01), (1.0 / 3.0, 0.0)]
    scale, wd = pairs[(FLAT_LENGTHS.index((k, r)) % 4) ^ int(bf16_grad)]
    _flat_case(k, r, bf16_grad, scale, wd)


@pytest.mark.parametrize("bf16_grad", [False, True], ids=["f32g", "bf16g"])
def test_adam_flat_from_step_50(bf16_grad):
    _flat_case(4, 5, bf16_grad, 1.0 / 3.0, 0.01, t0=49)


# ---------------------------------------------------------------- d. cast

def _cast_case(x_np):
    FM = _fm()
    n = x_np.size
    src = torch.from_numpy(x_np.copy()).cuda()
    dst = Guarded(n, torch.bfloat16)
    FM.cast_bf16(src, dst.t)
    _all_intact(dst)
    got = dst.t.view(torch.int16).cpu().numpy()
    want = R.bf16_rne_bits(x_np)
    nan = R.bf16_is_nan(want)
    assert np.array_equal(R.bf16_is_nan(got), nan), "NaN positions differ"
    bad = np.flatnonzero((got.view(np.uint16) != want) & ~nan)
    assert bad.size == 0, [(hex(int(x_np.view(np.uint32)[i])), hex(int(got.view(np.uint16)[i])), hex(int(want[i])))
                           for i in bad[:8]]


def test_cast_directed_vector_path():
    bits = R.cast_directed_bits()
    assert bits.size % 4 == 0
    for shift in range(4):  # every value passes through every element of a 4-wide group
        _cast_case(np.roll(bits, shift).view(np.float32))


@pytest.mark.parametrize("extra", [1, 2, 3])
def test_cast_directed_scalar_tail(extra):
    bits = R.cast_directed_bits()
    for i in range(0, bits.size, extra):  # one 4-wide group, then each value in turn in the scalar tail
        _cast_case(np.concatenate([bits[:4], bits[i:i + extra]]).view(np.float32))


def test_cast_grid_stride():
    n = 8192 * 1024 + 1027
    g = torch.Generator(device="cuda").manual_seed(3)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)
    _cast_case(bits.cpu().numpy().view(np.float32))


# ---------------------------------------------------------------- e. refusals

@pytest.fixture(scope="module")
def refusal_bufs():
    P = P_TOTAL
    b = {name: Guarded(P, torch.float32) for name in ("params", "m", "v", "grad_io")}
    b["small"] = {name: Guarded(128, torch.float32) for name in ("params", "m", "v", "grad_io")}
    b["state"] = Guarded(2, torch.int32)
    b["loss_out"] = Guarded(1, torch.float32)
    b["img"] = Guarded(54528, torch.uint8)
    b["shadow"] = Guarded(4096, torch.bfloat16)
    b["slabs"] = torch.ones(4, SLAB_STRIDE, device="cuda")
    b["slabs_small"] = torch.ones(4, 132, device="cuda")
    b["slabs_narrow"] = torch.ones(4, 64, device="cuda")
    b["loss_slabs"] = torch.ones(4, device="cuda")
    b["hp"] = _hp(0.0)
    torch.cuda.synchronize()
    return b


def _untouched(b):
    torch.cuda.synchronize()
    for name in ("params", "m", "v", "grad_io", "state", "loss_out", "img", "shadow"):
        assert b[name].poisoned() and b[name].intact(), f"{name} was written"
    for name, g in b["small"].items():
        assert g.poisoned() and g.intact(), f"small {name} was written"


SLAB_REFUSED = {
    "mode_3": dict(mode=3),
    "mode_3_pre": dict(mode=3, pre=True),
    "nslab_0_mode_0": dict(mode=0, nslab=0),
    "nslab_0_mode_1": dict(mode=1, nslab=0),
    "stride_below_p_mode_0": dict(mode=0, slabs="slabs_narrow", small=True),
    "stride_below_p_mode_1": dict(mode=1, slabs="slabs_narrow", small=True),
    "mode_1_without_grad_io": dict(mode=1, grad_io=False),
    "mode_2_without_grad_io": dict(mode=2, grad_io=False),
    "img_with_p_128": dict(mode=0, slabs="slabs_small", small=True, img=True),
}


@pytest.mark.parametrize("case", sorted(SLAB_REFUSED))
def test_adam_slab_refused(refusal_bufs, case):
    FM = _fm()
    b = refusal_bufs
    c = dict(mode=0, nslab=4, slabs="slabs", small=False, grad_io=True, img=False, pre=False)
    c.update(SLAB_REFUSED[case])
    s = b["small"] if c["small"] else b
    with pytest.raises(ValueError):
        FM.adam_slab(b[c["slabs"]], c["nslab"], 1.0, s["params"].t, s["m"].t, s["v"].t, b["hp"], b["state"].t,
                     mode=c["mode"], grad_io=s["grad_io"].t if c["grad_io"] else None,
                     img=b["img"].t if c["img"] else None, loss_slabs=b["loss_slabs"], loss_out=b["loss_out"].t,
                     pre=c["pre"])
    _untouched(b)


def test_adam_flat_bf16g_refuses_a_misaligned_gradient(refusal_bufs):
    FM = _fm()
    b = refusal_bufs
    n = 4096
    grad = torch.ones(n + 8, dtype=torch.bfloat16, device="cuda")[1:1 + n]
    assert grad.data_ptr() % 8 == 2
    with pytest.raises(ValueError):
        FM.adam_flat(b["params"].t[:n], grad, b["m"].t[:n], b["v"].t[:n], b["hp"], b["state"].t, shadow=b["shadow"].t)
    _untouched(b)


@pytest.mark.parametrize("which", ["src", "dst"])
def test_cast_refuses_misaligned_pointers(refusal_bufs, which):
    FM = _fm()
    b = refusal_bufs
    n = 1024
    src = torch.ones(n + 8, device="cuda")
    src = src[1:1 + n] if which == "src" else src[:n]
    dst = b["shadow"].t[1:1 + n] if which == "dst" else b["shadow"].t[:n]
    assert (src.data_ptr() % 16 == 4) == (which == "src") and (dst.data_ptr() % 8 == 2) == (which == "dst")
    with pytest.raises(ValueError):
        FM.cast_bf16(src, dst)
    _untouched(b)


if __name__ == "__main__":  # the child process of test_graph_replay_equals_eager
    _pool = _make_pool()
    for _shape in GRAPH_SHAPES:
        _graph_replay_case(_pool, *_shape)
        print("graph replay ok P=%d stride=%d nslab=%d" % _shape)
