"""The small row, gather and reduction ops of the training step, each against a float64 restatement of the same operation.

The references are plain PyTorch in float64, built from the SAME rounded inputs the kernel reads (a bf16 input is upcast, not regenerated).
Every comparison is element by element; the bounds are derived from the arithmetic, not tuned.  With u = 2^-24 (f32 unit roundoff):

* a chain of k f32 roundings:                     |err| <= k u |ref|
* a sum of n terms accumulated in f32, any order: |err| <= (n + 2) u sum |term_i|   (the + 2 absorbs the rounding of each term's product)
* a bf16 result adds the rounding of the f32 value to bf16: half a bf16 ulp taken at |ref| + (f32 bound), which is at most the
  one bf16 ulp of |ref| that the bar allows.

The one measured bound is the Highway gate's (device expf / tanhf): see HIGHWAY_MEASURED.  Kernels whose output ops.py allocates with
torch.empty are also launched directly (_raw) onto NaN-filled buffers, so that an element the kernel never writes is seen."""
import contextlib
import math

import pytest
import torch

from row_refs import check as _check, half_ulp_bf16 as _half_ulp_bf16, tol as _tol  # noqa: F401  (shared with test_row_ops_gpu.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTS = [F32, BF16]
U = 2.0 ** -24 * (1 + 2.0 ** -20)  # u, with room for the second-order terms ((1 + u)^k - 1 = k u + O(u^2))


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def _ops():
    from case_rg_amd import config, ops
    config.set_dropout(False)
    return ops


def _code(dt):
    return 0 if dt == F32 else 1


def _ev(dt):
    return 4 if dt == F32 else 8


def _rand(*shape, dt=F32, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dt)


def _misaligned(t):
    """A contiguous copy of ``t`` that does not start on a 16-byte boundary (one element into a fresh allocation)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 != 0
    return out


def _nan(*shape, dt=F32, mis=False):
    t = torch.full(shape, float("nan"), dtype=dt, device=DEV)
    return _misaligned(t) if mis else t


def _raw(name, *args):
    """The C entry point itself, on the current stream; tensors are passed as their addresses."""
    from case_rg_amd import _abi, ops
    _abi.call(name, *[ops._ptr(a) if torch.is_tensor(a) else a for a in args], ops._stream())


@contextlib.contextmanager
def _counting():
    """Counts the C-ABI calls made inside the block, by name."""
    from case_rg_amd import _abi
    calls, raw = {}, _abi.call

    def counting(name, *a):
        calls[name] = calls.get(name, 0) + 1
        return raw(name, *a)

    _abi.call = counting
    try:
        yield calls
    finally:
        _abi.call = raw


def _chain(ref, k, dt):
    return _tol(ref, k * U * ref.abs(), dt)


def _sum(ref, n, absum, dt):
    return _tol(ref, (n + 2) * U * absum, dt)


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert torch.equal(_bits(got.contiguous()), _bits(want.contiguous())), "%s: %d elements differ in bits" % (
        what, int((_bits(got.contiguous()) != _bits(want.contiguous())).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. cast
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 1027])
def test_cast_all_four_directions(n):
    ops = _ops()
    x = _rand(n, seed=n)
    want = x.cpu().to(BF16).to(DEV)  # round to nearest even, computed on the host
    _same_bits(ops.cast(x, BF16), want, "f32 -> bf16")
    assert torch.equal(ops.cast(want, F32), want.float()), "bf16 -> f32 is exact"
    for dt, src in ((F32, x), (BF16, want)):  # the same-dtype kernels: ops.cast returns its argument, so they are launched directly
        out = _nan(n, dt=dt)
        _raw("case_cast", src, out, n, _code(dt), _code(dt))
        _same_bits(out, src, "%s -> %s" % (dt, dt))


def test_cast_rounds_special_values_as_torch_does():
    ops = _ops()
    big = torch.finfo(F32).max
    x = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, big, -big, 1.0, -2.5], dtype=F32, device=DEV)
    want_bits = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x3F80, 0x3F82, 0x7F80, 0xFF80, 0x3F80, 0xC020]
    got = ops.cast(x, BF16)
    assert [b & 0xFFFF for b in got.view(torch.int16).tolist()] == want_bits
    _same_bits(got, x.cpu().to(BF16).to(DEV), "f32 -> bf16 special values")
    nan = ops.cast(torch.tensor([float("nan"), 1.0, -float("nan")], device=DEV), BF16)
    assert torch.isnan(nan).tolist() == [True, False, True]
    back = ops.cast(torch.tensor([float("nan"), float("inf"), -0.0], dtype=BF16, device=DEV), F32)
    assert torch.isnan(back[0]) and back[1] == float("inf") and back[2] == 0 and math.copysign(1, back[2].item()) == -1


@pytest.mark.parametrize("src,dst", [(F32, BF16), (BF16, F32)])
def test_cast_to_backward_returns_the_source_dtype(src, dst):
    ops = _ops()
    x = _rand(5, 13, dt=src, seed=1).requires_grad_()
    y = ops.cast_to(x, dst)
    assert y.dtype == dst and ops.cast_to(x, src) is x
    g = _rand(5, 13, dt=dst, seed=2)
    y.backward(g)
    assert x.grad.dtype == src
    _same_bits(x.grad, g.cpu().to(src).to(DEV), "cast_to gradient")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. add
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n,mis", [(64, None), (63, None), (64, "a"), (64, "b"), (64, "out")])
def test_add_vector_and_scalar_branches(dt, n, mis):
    _ops()
    a, b = _rand(n, dt=dt, seed=1), _rand(n, dt=dt, seed=2)
    ref = a.double() + b.double()
    a_, b_ = (_misaligned(a) if mis == "a" else a), (_misaligned(b) if mis == "b" else b)
    out = _nan(n, dt=dt, mis=mis == "out")
    _raw("case_add", a_, b_, out, n, _code(dt))
    _check(out, ref, _chain(ref, 1, dt), "add n=%d misaligned=%s" % (n, mis))


@pytest.mark.parametrize("dt", DTS)
def test_add_through_autograd(dt):
    ops = _ops()
    a, b = _rand(3, 21, dt=dt, seed=1).requires_grad_(), _misaligned(_rand(3, 21, dt=dt, seed=2)).requires_grad_()
    y = ops.add(a, b)
    ref = a.detach().double() + b.detach().double()
    _check(y, ref, _chain(ref, 1, dt), "ops.add")
    g = _rand(3, 21, dt=dt, seed=3)
    y.backward(g)
    assert torch.equal(a.grad, g) and torch.equal(b.grad, g)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. add_n
# ---------------------------------------------------------------------------------------------------------------------------------
def _grid_values(n, seed, dt):
    """k / 32 with integer |k| <= 255: exact in bf16, and any sum of eight of them is exact in f32."""
    k = torch.randint(-255, 256, (n,), generator=torch.Generator().manual_seed(seed))
    return (k.double() / 32).to(DEV).to(dt)


@pytest.mark.parametrize("dt", DTS)
def test_add_n_rounds_once(dt):
    ops = _ops()
    n = 4096
    srcs = [_grid_values(n, 100 + j, dt) for j in range(8)]
    assert all(torch.equal(s.double(), _grid_values(n, 100 + j, torch.float64)) for j, s in enumerate(srcs))
    for count in range(2, 9):
        want = sum(s.double() for s in srcs[:count]).to(dt)  # the float64 sum is exact; ONE rounding to the output type
        _same_bits(ops.add_n(srcs[:count]), want, "add_n of %d" % count)


@pytest.mark.parametrize("dt", DTS)
def test_add_n_rejects_what_it_does_not_take(dt):
    from case_rg_amd import _abi
    _ops()
    ev = _ev(dt)
    srcs = [_rand(8 * ev, dt=dt, seed=j) for j in range(9)]
    for count, n in ((1, 8 * ev), (9, 8 * ev), (3, 8 * ev - 1)):
        out = _nan(8 * ev, dt=dt)
        arr = (_abi.ptr * count)(*[s.data_ptr() for s in srcs[:count]])
        with pytest.raises(RuntimeError, match="case_add_n"):
            _raw("case_add_n", arr, count, out, n, _code(dt))
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), "count %d, n %d: nothing may be launched" % (count, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. fanout with gradients that do not start on a 16-byte boundary
# ---------------------------------------------------------------------------------------------------------------------------------
class _GradientIs(torch.autograd.Function):
    """Identity whose backward hands on exactly the tensor object it was given."""

    @staticmethod
    def forward(ctx, x, grad):
        ctx.grad = grad
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.grad, None


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("which", ["one", "all"])
def test_fanout_takes_misaligned_gradients(dt, which):
    ops = _ops()
    n, shape = 4, (6, 64)
    x = _rand(*shape, dt=dt, seed=1).requires_grad_()
    grads = [_rand(*shape, dt=dt, seed=10 + i) for i in range(n)]
    given = [_misaligned(g) if (which == "all" or i == 2) else g for i, g in enumerate(grads)]
    outs = ops.fanout(x, n)
    sum(_GradientIs.apply(o, g).float().sum() for o, g in zip(outs, given)).backward()
    ref = sum(g.double() for g in grads)
    # plain adds round every partial sum to the gradient's type: n - 1 roundings (unit 2^-8 for bf16's 8 significant bits) of partial sums
    # no larger than sum |g_i|; the one-pass kernel rounds once
    absum = sum(g.double().abs() for g in grads)
    bound = (n - 1) * (2.0 ** -8 if dt == BF16 else U) * absum
    _check(x.grad, ref, bound, "fan-out gradient, %s misaligned" % which)


@pytest.mark.parametrize("dt", DTS)
def test_fanout_under_a_concatenation_along_rows(dt):
    """torch.cat's backward hands each input a slice of the incoming gradient: contiguous, but at an odd storage offset when the rows
    before it do not fill a multiple of 16 bytes."""
    ops = _ops()
    x = _rand(8, 3, dt=dt, seed=1).requires_grad_()
    head = _rand(1, 3, dt=dt, seed=2)
    ws = [_rand(9, 3, dt=dt, seed=3 + i) for i in range(3)]
    outs = ops.fanout(x, 3)
    sum((torch.cat([head, o], dim=0) * w).float().sum() for o, w in zip(outs, ws)).backward()
    ref = sum(w[1:].double() for w in ws)
    absum = sum(w[1:].double().abs() for w in ws)
    _check(x.grad, ref, 2 * (2.0 ** -8 if dt == BF16 else U) * absum, "fan-out gradient under torch.cat")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. colsum
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_colsum_every_tiling(dt):
    ops = _ops()
    for rows in (1, 31, 33, 200):
        for cols in (1, 63, 64, 65, 100, 264):
            x = _rand(rows, cols, dt=dt, seed=rows * 1000 + cols)
            ref, absum = x.double().sum(0), x.double().abs().sum(0)
            _check(ops._colsum(x), ref, _sum(ref, rows, absum, F32), "colsum %d x %d" % (rows, cols))
    for rows, cols in ((33, 64), (200, 264)):  # the 16-byte kernel's shape at an address it cannot take
        x = _misaligned(_rand(rows, cols, dt=dt, seed=7))
        ref, absum = x.double().sum(0), x.double().abs().sum(0)
        _check(ops._colsum(x), ref, _sum(ref, rows, absum, F32), "colsum misaligned %d x %d" % (rows, cols))
    for rows, cols in ((33, 65), (200, 264)):  # out= : the sums are ADDED onto what it holds
        x, out = _rand(rows, cols, dt=dt, seed=8), _rand(cols, seed=9, scale=3.0)
        ref, absum = x.double().sum(0) + out.double(), x.double().abs().sum(0) + out.double().abs()
        got = ops._colsum(x, out=out)
        assert got is out
        _check(got, ref, _sum(ref, rows + 1, absum, F32), "colsum onto out %d x %d" % (rows, cols))


@pytest.mark.parametrize("dt", DTS)
def test_colsum_is_the_bias_gradient_of_a_frozen_linear(dt):
    ops = _ops()
    M, K, N = 33, 24, 40
    x, w, b = _rand(M, K, dt=dt, seed=1), _rand(N, K, seed=2), _rand(N, seed=3).requires_grad_()
    g = _rand(M, N, dt=dt, seed=4)
    with _counting() as calls:
        ops.linear(x, w.requires_grad_(False), b).backward(g)
    assert calls.get("case_colsum", 0) == 1 and w.grad is None
    ref, absum = g.double().sum(0), g.double().abs().sum(0)
    _check(b.grad, ref, _sum(ref, M, absum, F32), "linear bias gradient")


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. row dot (Linear with one output feature)
# ---------------------------------------------------------------------------------------------------------------------------------
def _rowdot_case(ops, dt, xshape, with_b=True, x_grad=True, seed=0):
    C = xshape[-1]
    rows = math.prod(xshape[:-1])
    x = _rand(*xshape, dt=dt, seed=seed + 1).requires_grad_(x_grad)
    w = _rand(1, C, seed=seed + 2).requires_grad_()
    b = _rand(1, seed=seed + 3).requires_grad_() if with_b else None
    with _counting() as calls:
        y = ops.linear(x, w, b, out_dtype=None if dt == F32 else F32)
    assert calls == {"case_rowdot_fwd": 1}, calls
    assert y.dtype == F32 and tuple(y.shape) == tuple(xshape[:-1]) + (1,)
    what = "row dot %s %s" % (tuple(xshape), dt)
    x64, w64 = x.detach().double().reshape(rows, C), w.detach().double()
    b64 = b.detach().double() if with_b else torch.zeros(1, dtype=torch.float64, device=DEV)
    ref = (x64 * w64).sum(1, keepdim=True) + b64
    absum = (x64 * w64).abs().sum(1, keepdim=True) + b64.abs()
    _check(y.reshape(rows, 1), ref, _sum(ref, C + 1, absum, F32), what + " y")
    g = _rand(rows, 1, seed=seed + 4)
    with _counting() as calls:
        y.backward(g.view(y.shape))
    assert calls.get("case_rowdot_bwd", 0) == 1
    g64 = g.double()
    if x_grad:
        assert x.grad.dtype == dt
        _check(x.grad.reshape(rows, C), g64 * w64, _chain(g64 * w64, 1, dt), what + " dx")
    else:
        assert x.grad is None
    ref = (g64 * x64).sum(0, keepdim=True)
    assert w.grad.shape == w.shape and w.grad.dtype == F32
    _check(w.grad, ref, _sum(ref, rows, (g64 * x64).abs().sum(0, keepdim=True), F32), what + " dw")
    if with_b:
        _check(b.grad, g64.sum(0), _sum(g64.sum(0), rows, g64.abs().sum(0), F32), what + " db")


@pytest.mark.parametrize("dt", DTS)
def test_rowdot_forward_and_gradients(dt):
    ops = _ops()
    for rows in (1, 5, 130):
        for C in (1, 63, 64, 65, 512):
            _rowdot_case(ops, dt, (rows, C), seed=rows + C)
    _rowdot_case(ops, dt, (2, 65, 63), seed=5)
    _rowdot_case(ops, dt, (130, 65), with_b=False, seed=6)  # null db
    _rowdot_case(ops, dt, (130, 65), x_grad=False, seed=7)  # null dx


@pytest.mark.parametrize("dt", DTS)
def test_rowdot_backward_writes_every_element_of_dx(dt):
    _ops()
    rows, C = 130, 65
    x, w, g = _rand(rows, C, dt=dt, seed=1), _rand(C, seed=2), _rand(rows, seed=3)
    dx, dw, db = _nan(rows, C, dt=dt), torch.zeros(C, device=DEV), torch.zeros(1, device=DEV)
    _raw("case_rowdot_bwd", g, x, w, dx, dw, db, rows, C, _code(dt))
    ref = g.double()[:, None] * w.double()[None, :]
    _check(dx, ref, _chain(ref, 1, dt), "row dot dx onto NaN")
    terms = g.double()[:, None] * x.double()
    _check(dw, terms.sum(0), _sum(terms.sum(0), rows, terms.abs().sum(0), F32), "row dot dw")
    _check(db, g.double().sum(0, keepdim=True), _sum(g.double().sum(0, keepdim=True), rows, g.double().abs().sum(0, keepdim=True), F32), "row dot db")


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. scale_cols
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_scale_cols_forward_and_raw_backward(dt):
    ops = _ops()
    for rows in (1, 5, 130):  # 130 rows: five row splits, the last one ragged
        for C in (1, 63, 64, 65, 512):
            x, w, g = _rand(rows, C, dt=dt, seed=rows + C), _rand(C, seed=2), _rand(rows, C, dt=dt, seed=3)
            what = "scale_cols %d x %d" % (rows, C)
            ref = x.double() * w.double()
            _check(ops.scale_cols(x, w), ref, _chain(ref, 1, dt), what + " y")
            dx, dw = _nan(rows, C, dt=dt), torch.zeros(C, device=DEV)
            _raw("case_scale_cols_bwd", g, x, w, dx, dw, rows, C, _code(dt))
            ref = g.double() * w.double()
            _check(dx, ref, _chain(ref, 1, dt), what + " dx onto NaN")
            terms = g.double() * x.double()
            _check(dw, terms.sum(0), _sum(terms.sum(0), rows, terms.abs().sum(0), F32), what + " dw")


@pytest.mark.parametrize("dt", DTS)
def test_scale_cols_through_autograd(dt):
    ops = _ops()
    x, w, g = _rand(2, 65, 63, dt=dt, seed=1).requires_grad_(), _rand(63, seed=2).requires_grad_(), _rand(2, 65, 63, dt=dt, seed=3)
    ops.scale_cols(x, w).backward(g)
    ref = g.double() * w.detach().double()
    _check(x.grad, ref, _chain(ref, 1, dt), "scale_cols dx")
    terms = (g.double() * x.detach().double()).reshape(130, 63)
    _check(w.grad, terms.sum(0), _sum(terms.sum(0), 130, terms.abs().sum(0), F32), "scale_cols dw")


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. scale_add_rows
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", [7, 24, 512])
def test_scale_add_rows(dt, H):
    ops = _ops()
    L = 5
    pe = _rand(L + 3, H, seed=9)  # more rows than L: only the first L are used, and the row index wraps at L
    scale = math.sqrt(H)
    s64 = float(torch.tensor(scale, dtype=F32))  # the C ABI takes the factor as a float
    for shape in ((3, L, H), (2, 3, L, H)):
        x = _rand(*shape, dt=dt, seed=len(shape)).requires_grad_()
        y = ops.scale_add_rows(x, pe, scale)
        a, b = x.detach().double() * s64, pe.double()[:L].expand(shape)
        _check(y, a + b, _sum(a + b, 2, a.abs() + b.abs(), dt), "scale_add_rows %s" % (shape,))
        g = _rand(*shape, dt=dt, seed=11)
        y.backward(g)
        _check(x.grad, g.double() * s64, _chain(g.double() * s64, 1, dt), "scale_add_rows backward %s" % (shape,))


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. highway_gate
# ---------------------------------------------------------------------------------------------------------------------------------
# The normal-range bound is MEASURED (it depends on the device's expf and tanhf): 4 x the largest |got - ref| / (1 + |l|) of the forward and
# 4 x the largest |got - ref| / (|dy| (1 + |l|)) of the three gradients, over the shapes of test_highway_gate, as recorded on the MI355X in
# profiles/small_ops_parity.json -- and never looser than the bar of test_ops_gpu.py (1e-3 for f32, 3e-2 for bf16).
HIGHWAY_MEASURED = {F32: {"fwd": 1.034e-07, "bwd": 1.132e-07}, BF16: {"fwd": 2.365e-03, "bwd": 3.123e-03}}
HIGHWAY_BAR = {F32: 1e-3, BF16: 3e-2}


def _highway_bound(dt, which):
    return min(4 * HIGHWAY_MEASURED[dt][which], HIGHWAY_BAR[dt])


def _highway_ref(gnl, dy):
    cols = gnl.shape[-1] // 3
    g, n, l = gnl.double().split(cols, dim=-1)
    t, f = torch.sigmoid(g), torch.tanh(n)
    y = t * f + (1 - t) * l
    d = torch.cat([dy.double() * (f - l) * t * (1 - t), dy.double() * t * (1 - f * f), dy.double() * (1 - t)], dim=-1)
    return y, d, l


def highway_errors(dt):
    """(largest normalised forward error, largest normalised gradient error) over the shapes of the test; also what the profile records."""
    ops = _ops()
    worst_f = worst_b = 0.0
    for rows in (1, 37):
        for cols in (1, 50, 512):
            gnl = _rand(rows, 3 * cols, dt=dt, seed=rows + cols)
            gnl[:, 2 * cols:] *= 2
            gnl.requires_grad_()
            dy = _rand(rows, cols, dt=dt, seed=3)
            dy = torch.where(dy == 0, torch.ones_like(dy), dy)
            y = ops.highway_gate(gnl)
            y.backward(dy)
            yr, dr, l = _highway_ref(gnl.detach(), dy)
            assert torch.isfinite(y).all() and torch.isfinite(gnl.grad).all()
            worst_f = max(worst_f, ((y.double() - yr).abs() / (1 + l.abs())).max().item())
            norm = (dy.double().abs() * (1 + l.abs())).repeat(1, 3)
            worst_b = max(worst_b, ((gnl.grad.double() - dr).abs() / norm).max().item())
    return worst_f, worst_b


@pytest.mark.parametrize("dt", DTS)
def test_highway_gate(dt):
    fwd, bwd = highway_errors(dt)
    print("highway_gate %s: forward %.3e, gradients %.3e" % (dt, fwd, bwd))
    assert fwd <= _highway_bound(dt, "fwd"), (fwd, _highway_bound(dt, "fwd"))
    assert bwd <= _highway_bound(dt, "bwd"), (bwd, _highway_bound(dt, "bwd"))


@pytest.mark.parametrize("dt", DTS)
def test_highway_gate_saturates_to_the_exact_limits(dt):
    ops = _ops()
    rows, cols = 4, 50
    sg = torch.where(_rand(rows, cols, seed=1) > 0, 1.0, -1.0)
    sn = torch.where(_rand(rows, cols, seed=2) > 0, 1.0, -1.0)
    l = _rand(rows, cols, dt=dt, seed=3).float()
    gnl = torch.cat([100 * sg, 50 * sn, l], dim=-1).to(dt).requires_grad_()
    dy = _rand(rows, cols, dt=dt, seed=4)
    y = ops.highway_gate(gnl)
    y.backward(dy)
    assert torch.isfinite(y).all() and torch.isfinite(gnl.grad).all()
    assert torch.equal(y.float(), torch.where(sg > 0, sn, l)), "t = 1 gives tanh(n) = +-1, t = 0 gives l"
    dg, dn, dl = gnl.grad.float().split(cols, dim=-1)
    assert (dg == 0).all() and (dn == 0).all()
    assert torch.equal(dl, torch.where(sg > 0, torch.zeros_like(l), dy.float()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. max_over_p
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_max_over_p_lowest_index_wins(dt):
    ops = _ops()
    for B in (1, 3):
        for P in (1, 2, 5):
            for Lq, Lk in ((1, 1), (7, 11), (25, 41)):
                inner = Lq * Lk
                k = torch.randint(-8, 9, (B, P, inner), generator=torch.Generator().manual_seed(B * 100 + P * 10 + Lq))
                x = (k.float() / 4).to(DEV).to(dt)  # quantised: ties are the rule
                x[0, :, 0] = 0.5  # a column of equal values
                x[B - 1, :, inner - 1] = float("-inf")  # nothing finite: index 0, value -inf
                what = "max_over_p B=%d P=%d inner=%d" % (B, P, inner)
                top = x.amax(1, keepdim=True)
                ar = torch.arange(P, device=DEV).view(1, P, 1).expand(B, P, inner)
                want_idx = torch.where(x == top, ar, torch.full_like(ar, P)).amin(1)
                assert want_idx[0, 0] == 0 and want_idx[B - 1, inner - 1] == 0
                out, arg = _nan(B, inner, dt=dt), torch.full((B, inner), -7, dtype=torch.int32, device=DEV)
                _raw("case_max_over_p_fwd", x, out, arg, B, P, inner, _code(dt))
                _same_bits(out, top.reshape(B, inner), what + " value")
                assert torch.equal(arg.long(), want_idx), what + " index"
                g = _rand(B, inner, dt=dt, seed=5)
                g = torch.where(g == 0, torch.ones_like(g), g)
                dx = _nan(B, P, inner, dt=dt)
                _raw("case_max_over_p_bwd", g, arg, dx, B, P, inner, _code(dt))
                want_dx = torch.where(ar == want_idx[:, None, :], g[:, None, :].expand(B, P, inner), torch.zeros_like(x))
                _same_bits(dx, want_dx, what + " dx")
                xs = x.view(B, P, Lq, Lk).clone().requires_grad_()  # and through the autograd shell
                y = ops.max_over_p(xs)
                assert tuple(y.shape) == (B, 1, Lq, Lk)
                _same_bits(y.detach().reshape(B, inner), top.reshape(B, inner), what + " ops value")
                y.backward(g.view(B, 1, Lq, Lk))
                _same_bits(xs.grad.reshape(B, P, inner), want_dx, what + " ops dx")


# ---------------------------------------------------------------------------------------------------------------------------------
# 11. embed_pos
# ---------------------------------------------------------------------------------------------------------------------------------
def _embed_ref(ids, table, pe):
    V, H = table.shape
    L = ids.shape[-1]
    s64 = float(torch.tensor(math.sqrt(H), dtype=F32))
    clamped = torch.where((ids < 0) | (ids >= V), torch.zeros_like(ids), ids)
    pos = (torch.arange(ids.numel(), device=ids.device) % L).view(ids.shape)
    a, b = table.double()[clamped] * s64, pe.double()[pos]
    return a + b, a.abs() + b.abs()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H,mis", [(8, False), (512, False), (7, False), (20, False), (8, True)])
def test_embed_pos_forward(dt, H, mis):
    """H = 8 / 512: the vector kernel; 7 / 20, and 8 with a misaligned position table: the scalar one."""
    ops = _ops()
    V, L = 11, 5
    ids = torch.randint(0, V, (3, 2, L), generator=torch.Generator().manual_seed(H)).to(DEV)
    ids[0, 0, 1], ids[1, 1, 4], ids[2, 0, 0] = -1, V, 0  # out-of-range ids read row 0
    table, pe = _rand(V, H, seed=1), _rand(L + 4, H, seed=2)
    pe = _misaligned(pe) if mis else pe
    y = ops.embed_pos(ids, table, pe, dtype=dt)
    assert y.dtype == dt and tuple(y.shape) == (3, 2, L, H)
    ref, absum = _embed_ref(ids, table, pe)
    _check(y, ref, _sum(ref, 2, absum, dt), "embed_pos H=%d" % H)
    _same_bits(y[0, 0, 1], ops.embed_pos(torch.zeros(1, 2, dtype=torch.long, device=DEV), table, pe, dtype=dt)[0, 1], "id -1 reads row 0")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", [8, 20])
def test_embed_pos_backward_with_duplicate_ids(dt, H):
    ops = _ops()
    V, L = 11, 5
    ids = torch.randint(0, V, (60, L), generator=torch.Generator().manual_seed(3)).to(DEV)  # 300 rows over 11 ids
    ids[0, 0], ids[1, 1], ids[2, 2] = -1, V, 0
    table, pe = _rand(V, H, seed=1).requires_grad_(), _rand(L, H, seed=2)
    y = ops.embed_pos(ids, table, pe, dtype=dt)
    g = _rand(60, L, H, dt=dt, seed=4)
    y.backward(g)
    s64 = float(torch.tensor(math.sqrt(H), dtype=F32))
    flat, terms = ids.reshape(-1), g.double().reshape(-1, H) * s64
    live = ((flat > 0) & (flat < V)).double()[:, None]
    idx = flat.clamp(0, V - 1)
    ref = torch.zeros(V, H, dtype=torch.float64, device=DEV).index_add_(0, idx, terms * live)
    absum = torch.zeros_like(ref).index_add_(0, idx, terms.abs() * live)
    cnt = torch.zeros(V, 1, dtype=torch.float64, device=DEV).index_add_(0, idx, live)
    assert table.grad.dtype == F32 and (table.grad[0] == 0).all(), "the padding row and out-of-range ids get no gradient"
    _check(table.grad, ref, _sum(ref, cnt, absum, F32), "embed_pos d_table H=%d" % H)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", [512, 20])
def test_embed_pos_backward_regenerates_the_forward_dropout_mask(dt, H):
    """The forward is the vector kernel at H = 512 and the scalar one at H = 20; the backward is always the scalar kernel."""
    from case_rg_amd import config, ops
    config.set_dropout(True)
    config.manual_seed(5)
    try:
        V, L = 65, 16
        ids = torch.arange(1, V, device=DEV).view(4, L)  # every id once
        table = (1 + _rand(V, H, seed=1).abs()).requires_grad_()
        pe = _rand(L, H, seed=2).abs()  # nothing kept is zero
        y = ops.embed_pos(ids, table, pe, p_drop=config.drop_p(0.3, True), dtype=dt)
        kept = y != 0
        assert 0.6 < kept.float().mean().item() < 0.8
        y.backward(torch.ones_like(y))
        assert torch.equal(table.grad[1:].view(4, L, H) != 0, kept), "backward must regenerate the same mask"
        assert (table.grad[0] == 0).all()
    finally:
        config.set_dropout(False)


# ---------------------------------------------------------------------------------------------------------------------------------
# 12. masked_mean: short sequences, misaligned operands, a sequence without a valid position
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("mis", [False, True])
def test_masked_mean_short_and_empty_sequences(dt, L, mis):
    """Aligned: the vector kernels (H = 64), where L < 4 leaves waves without a row; misaligned: the scalar kernels."""
    ops = _ops()
    n, H = 4, 64
    x = _rand(n, L, H, dt=dt, seed=L)
    x = _misaligned(x) if mis else x
    valid = torch.ones(n, L, dtype=torch.bool, device=DEV)
    valid[2] = False  # no valid position at all
    valid[3, L - 1:] = L == 1
    y = ops.masked_mean(x, valid)
    cnt = valid.sum(1, keepdim=True).double()
    live = [0, 1, 3]
    terms = x.double() * valid[:, :, None]
    ref, absum = terms.sum(1) / cnt, terms.abs().sum(1) / cnt
    assert torch.isnan(y[2]).all(), "0 / 0 in every channel, as the reference computes it"
    _check(y[live], ref[live], _sum(ref[live], cnt[live], absum[live], dt), "masked mean L=%d" % L)
    g = _rand(n, H, dt=dt, seed=7)
    g = _misaligned(g) if mis else g
    dx = _nan(n, L, H, dt=dt, mis=mis)
    _raw("case_masked_mean_bwd", g, valid.view(torch.uint8), dx, n, L, H, _code(dt))
    assert (dx[2] == 0).all() and torch.isfinite(dx).all(), "an empty sequence gets an exact, finite zero"
    ref = (g.double()[:, None, :] / cnt[:, :, None]) * valid[:, :, None]
    assert (dx[~valid] == 0).all()
    _check(dx[live], ref[live], _chain(ref[live], 1, dt), "masked mean dx L=%d" % L)


# ---------------------------------------------------------------------------------------------------------------------------------
# 13. concat5 and mask_rows at addresses the 16-byte kernels cannot take
# ---------------------------------------------------------------------------------------------------------------------------------
def _place(t, mis):
    return _misaligned(t) if mis else t


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", [8, 20])
def test_concat5_scalar_and_vector_forms(dt, H):
    _ops()
    rows = 5
    e, a1, a2 = (_rand(rows, H, dt=dt, seed=s) for s in (1, 2, 3))
    d_out = _rand(rows, 5 * H, dt=dt, seed=4)
    valid = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device=DEV)
    v64, zero = valid.double()[:, None], torch.zeros((), dtype=torch.float64, device=DEV)
    e64, x1, x2, g = e.double(), a1.double(), a2.double(), d_out.double()
    ref = torch.where(v64 != 0, torch.cat([e64, x1, x2, e64 * x1, e64 * x2], dim=1), zero)
    g0, g1, g2, g3, g4 = g.split(H, dim=1)
    refs = [torch.where(v64 != 0, r, zero) for r in (g0 + g3 * x1 + g4 * x2, g1 + g3 * e64, g2 + g4 * e64)]
    absums = [(g0.abs() + (g3 * x1).abs() + (g4 * x2).abs()), (g1.abs() + (g3 * e64).abs()), (g2.abs() + (g4 * e64).abs())]
    outs, grads = {}, {}
    for form in ("aligned", "inputs", "outputs"):
        mi, mo = form == "inputs", form == "outputs"
        out = _nan(rows, 5 * H, dt=dt, mis=mo)
        _raw("case_concat5_fwd", _place(e, mi), _place(a1, mi), _place(a2, mi), valid, out, rows, H, _code(dt))
        assert (out[valid == 0] == 0).all(), "invalid rows are exact zeros in all five blocks"
        _same_bits(out[:, :3 * H], ref[:, :3 * H].to(dt), "concat5 %s: the three copies" % form)
        _check(out, ref, _chain(ref, 1, dt), "concat5 forward, %s" % form)
        outs[form] = out.clone()
        ds = [_nan(rows, H, dt=dt, mis=mo) for _ in range(3)]
        _raw("case_concat5_bwd", _place(d_out, mi), _place(e, mi), _place(a1, mi), _place(a2, mi), valid, ds[0], ds[1], ds[2], rows, H, _code(dt))
        for name, d, r, s, n in zip(("de", "da1", "da2"), ds, refs, absums, (3, 2, 2)):
            assert (d[valid == 0] == 0).all(), "invalid rows are exact zeros in " + name
            _check(d, r, _sum(r, n, s * v64, dt), "concat5 %s, %s" % (name, form))
        grads[form] = [d.clone() for d in ds]
    for form in ("inputs", "outputs"):
        _same_bits(outs[form], outs["aligned"], "concat5 forward: %s against aligned" % form)
        for d, a in zip(grads[form], grads["aligned"]):
            _same_bits(d, a, "concat5 backward: %s against aligned" % form)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", [8, 20])
def test_mask_rows_scalar_and_vector_forms(dt, H):
    ops = _ops()
    rows = 5
    x = _rand(rows, H, dt=dt, seed=1)
    valid = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device=DEV)
    want = torch.where(valid[:, None] != 0, x, torch.zeros_like(x))
    for mi, mo in ((False, False), (True, False), (False, True), (True, True)):
        y = _nan(rows, H, dt=dt, mis=mo)
        _raw("case_mask_rows", _place(x, mi), valid, y, rows, H, _code(dt))
        _same_bits(y, want, "mask_rows out of place, misaligned in=%s out=%s" % (mi, mo))
    xm = _misaligned(x)  # in place at a misaligned address: the scalar form touches the invalid rows only
    assert ops.mask_rows(xm, valid.bool(), in_place=True) is xm
    _same_bits(xm, want, "mask_rows in place, misaligned")
    xg = _misaligned(x).requires_grad_()
    g = _misaligned(_rand(rows, H, dt=dt, seed=2))
    y = ops.mask_rows(xg, valid.bool())
    _same_bits(y.detach(), want, "ops.mask_rows")
    y.backward(g)
    _same_bits(xg.grad, torch.where(valid[:, None] != 0, g, torch.zeros_like(g)), "ops.mask_rows gradient")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("offset", [0, 7])
def test_dropout_scalar_and_vector_forms_draw_the_same_mask(dt, offset):
    """case_dropout hashes element PAIRS: the 16-byte kernel takes a pair from one hash when its first counter is even and falls back to the
    per-element definition when it is odd (offset 7); the scalar kernel (misaligned operands, or n not a multiple of the vector) always
    uses the per-element definition.  All of them must keep the same elements."""
    _ops()
    n, p, seed = 1024, 0.3, 123
    x = _rand(n, dt=dt, seed=1)
    x = torch.where(x == 0, torch.ones_like(x), x)
    p64 = float(torch.tensor(p, dtype=F32))
    ref = x.double() / (1 - p64)  # 1 - p, 1 / (1 - p) and the product: three f32 roundings
    ys = []
    for mi, mo in ((False, False), (True, False), (False, True)):
        y = _nan(n, dt=dt, mis=mo)
        _raw("case_dropout", _place(x, mi), y, n, p, seed, offset, None, _code(dt))
        kept = y != 0
        assert 0.6 < kept.float().mean().item() < 0.8
        _check(y, ref * kept, _chain(ref, 3, dt) * kept, "dropout values, misaligned in=%s out=%s" % (mi, mo))
        ys.append(y)
    _same_bits(ys[1], ys[0], "dropout: scalar form (misaligned input) against the vector form")
    _same_bits(ys[2], ys[0], "dropout: scalar form (misaligned output) against the vector form")
    tail = _nan(n - 1, dt=dt)  # n - 1 elements: the scalar form by size; same counters, so the same mask on the common part
    _raw("case_dropout", x, tail, n - 1, p, seed, offset, None, _code(dt))
    _same_bits(tail, ys[0][:n - 1], "dropout: scalar form (odd size) against the vector form")


# ---------------------------------------------------------------------------------------------------------------------------------
# 14. copy_scatter, atomic and sorted
# ---------------------------------------------------------------------------------------------------------------------------------
def _scatter_case(ops, src, V, T, seed, what):
    B, S = src.shape
    w = _rand(B, T, S, seed=seed)
    w[w.abs() < 0.3] = 0  # exact zeros are skipped by both forms
    w.requires_grad_()
    base = _rand(B, T, V, seed=seed + 1).requires_grad_()
    ok = ((src >= 0) & (src < V))[:, None, :].expand(B, T, S)
    idx = src.clamp(0, V - 1)[:, None, :].expand(B, T, S).contiguous()
    w64 = torch.where(ok, w.detach().double(), torch.zeros((), dtype=torch.float64, device=DEV))
    ref = base.detach().double().scatter_add(2, idx, w64)
    absum = base.detach().double().abs().scatter_add(2, idx, w64.abs())
    cnt = torch.zeros(B, T, V, dtype=torch.float64, device=DEV).scatter_add(2, idx, ok.double()) + 1  # + the base
    tol = _sum(ref, cnt, absum, F32)
    d = ops.copy_scatter(src, w, V, base)
    _check(d, ref, tol, what + " atomic")
    assert ops.SortedSource.fits(src, V)
    ss = ops.SortedSource(src, V)
    d1 = ops.copy_scatter(ss, w, V, base)
    d2 = ops.copy_scatter(ss, w, V, base)
    _check(d1, ref, tol, what + " sorted")
    _same_bits(d1.detach(), d2.detach(), what + " sorted, two launches")
    g = _rand(B, T, V, seed=seed + 2)
    want_dw = torch.where(ok, g.gather(2, idx), torch.zeros_like(w))
    for dist in (d, d1):
        w.grad = base.grad = None
        dist.backward(g)
        _same_bits(w.grad, want_dw, what + " dw")
        _same_bits(base.grad, g, what + " dbase")
    d_w = _nan(B, T, S)
    _raw("case_copy_scatter_bwd", src, g, d_w, B, T, S, V)
    _same_bits(d_w, want_dw, what + " dw onto NaN")


def test_copy_scatter_atomic_and_sorted():
    ops = _ops()
    V, T = 9, 3
    tokens = torch.tensor([2, 5, V - 1, -1, V])  # three distinct tokens: their runs straddle the 256-key chunks; -1 and V are dropped
    for S in (1, 255, 256, 257, 600):
        pick = torch.randint(0, 5, (2, S), generator=torch.Generator().manual_seed(S))
        _scatter_case(ops, tokens[pick].to(DEV), V, T, seed=S, what="copy_scatter S=%d" % S)


def test_copy_scatter_at_the_key_packing_limit():
    ops = _ops()
    V = ops.SortedSource.MAX_V
    assert V == 131071
    src = torch.tensor([[7, V - 1, -1, V, V - 1]], device=DEV)  # token V - 1 at the last position: the largest valid key
    _scatter_case(ops, src, V, 2, seed=1, what="copy_scatter V=%d" % V)


# ---------------------------------------------------------------------------------------------------------------------------------
# 15. nll_rows
# ---------------------------------------------------------------------------------------------------------------------------------
def test_nll_rows_targets_at_and_beyond_the_edges():
    ops = _ops()
    rows, V = 300, 13
    dist = torch.softmax(_rand(rows, V, seed=1), -1)
    tgt = torch.randint(1, V, (rows,), generator=torch.Generator().manual_seed(2)).to(DEV)
    tgt[0], tgt[1], tgt[2], tgt[3], tgt[299] = 0, -1, V, V - 1, V - 1
    dist[7, tgt[7]] = 0.0  # probability exactly 0 at the target: -log(1e-8)
    dist.requires_grad_()
    y = ops.nll_rows(dist, tgt)
    live = (tgt > 0) & (tgt < V)
    eps = float(torch.tensor(1e-8, dtype=F32))
    p = dist.detach().double().gather(1, tgt.clamp(0, V - 1)[:, None])[:, 0] + eps
    ref = torch.where(live, -p.log(), torch.zeros_like(p))
    # the f32 sum p + eps is one rounding of the argument, which moves the logarithm by at most u / (1 - u) < 2 u; the device logf is
    # documented to 2 ulp (HIP math API), and an f32 ulp is at most 2 u |ref|
    _check(y, ref, 2 * U + 4 * U * ref.abs(), "nll rows")
    assert (y[:3] == 0).all() and abs(y[7].item() + math.log(eps)) <= 4 * U * abs(math.log(eps))
    g = _rand(rows, seed=3)
    y.backward(g)
    want = torch.zeros(rows, V, dtype=torch.float64, device=DEV)
    want[live, tgt[live]] = (-g.double() / p)[live]
    hit = torch.zeros(rows, V, dtype=torch.bool, device=DEV)
    hit[live, tgt[live]] = True
    assert (dist.grad[~hit] == 0).all(), "the gradient lives at the target column only"
    _check(dist.grad, want, _chain(want, 2, F32), "nll d_dist")


# ---------------------------------------------------------------------------------------------------------------------------------
# 16. row_argmax
# ---------------------------------------------------------------------------------------------------------------------------------
def _argmax_rows(cols):
    """One row per tie stage, where ``cols`` has room for it: equal maxima in one thread's stride (3, 259 and 44, 300: 256 apart), in two
    lanes of a wave (5, 9), in two waves (44, 200); a lone maximum at the last column; a row of -inf; a row of equal values."""
    rows = []
    for pair in ((3, 259), (44, 300), (5, 9), (44, 200), (cols - 1, cols - 1)):
        if max(pair) < cols:
            r = torch.rand(cols, generator=torch.Generator().manual_seed(sum(pair)))
            r[list(pair)] = 2.0
            rows.append(r)
    rows.append(torch.full((cols,), float("-inf")))
    rows.append(torch.full((cols,), 0.25))
    return torch.stack(rows).to(DEV)


def _lowest_argmax(x):
    cols = x.shape[1]
    ar = torch.arange(cols, device=x.device).expand_as(x)
    return torch.where(x == x.amax(1, keepdim=True), ar, torch.full_like(ar, cols)).amin(1)


@pytest.mark.parametrize("cols", [1, 255, 256, 257, 1000])
def test_row_argmax_ties_at_every_stage(cols):
    ops = _ops()
    x = _argmax_rows(cols)
    idx, val = ops.row_argmax(x)
    want = _lowest_argmax(x)
    assert idx.dtype == torch.int64 and idx.tolist() == want.tolist()
    assert torch.equal(val, x.amax(1))
    assert idx[-2] == 0 and val[-2] == float("-inf") and idx[-1] == 0
    # a leading dimension larger than the row: what sits in the padding is larger than every element and must not win
    rows, ld = x.shape[0], cols + 3
    padded = torch.full((rows, ld), 9.0, device=DEV)
    padded[:, :cols] = x
    idx2, val2 = torch.full((rows,), -1, dtype=torch.int64, device=DEV), _nan(rows)
    _raw("case_row_argmax", padded, idx2, val2, rows, cols, ld)
    assert idx2.tolist() == want.tolist() and torch.equal(val2, x.amax(1))


# ---------------------------------------------------------------------------------------------------------------------------------
# 17. autograd glue
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_split_rows_and_split_param_rows_equal_slicing(dt):
    ops = _ops()
    groups = [(0, 2, 3), (6, 1, 4), (10, 3, 2)]
    x = _rand(16, 5, dt=dt, seed=1).requires_grad_()
    xr = x.detach().clone().requires_grad_()
    ws = [_rand(N, L, 5, dt=dt, seed=2 + i) for i, (_, N, L) in enumerate(groups)]
    for used in ((0, 1, 2), (1,), (0, 2)):  # an output nobody uses gets no gradient: its rows are zeros
        x.grad = xr.grad = None
        parts = ops.split_rows(x, groups)
        assert all(p.data_ptr() == x.data_ptr() + r0 * 5 * x.element_size() and tuple(p.shape) == (N, L, 5) for p, (r0, N, L) in zip(parts, groups))
        sum((parts[i] * ws[i]).sum() for i in used).backward()
        sum((xr[groups[i][0]:groups[i][0] + groups[i][1] * groups[i][2]].view(groups[i][1], groups[i][2], 5) * ws[i]).sum() for i in used).backward()
        _same_bits(x.grad, xr.grad, "split_rows gradient, outputs %s used" % (used,))
    w = _rand(9, 4, seed=5).requires_grad_()
    wr = w.detach().clone().requires_grad_()
    g0, g1 = _rand(3, 4, seed=6), _rand(6, 4, seed=7)
    for used in ((0, 1), (0,), (1,)):
        w.grad = wr.grad = None
        a, b = ops.split_param_rows(w, 3)
        assert torch.equal(a, w[:3]) and torch.equal(b, w[3:])
        sum(((a, b)[i] * (g0, g1)[i]).sum() for i in used).backward()
        sum(((wr[:3], wr[3:])[i] * (g0, g1)[i]).sum() for i in used).backward()
        _same_bits(w.grad, wr.grad, "split_param_rows gradient, outputs %s used" % (used,))
    with torch.no_grad():
        a, b = ops.split_param_rows(w, 3)
        assert a.data_ptr() == w.data_ptr() and tuple(b.shape) == (6, 4)


def _close(got, want, tol, what):
    """The bar of test_ops_gpu.py's test_attention: relative to the largest element of the reference."""
    got, want = got.float(), want.float()
    scale = want.abs().max().item() + 1e-6
    err = (got - want).abs().max().item()
    assert err <= tol * scale, "%s: max err %.3e vs scale %.3e (tol %.1e)" % (what, err, scale, tol)


def test_attention_groups_equals_attention_per_group():
    ops = _ops()
    heads, d = 8, 64
    E, W = heads * d, 3 * heads * d
    if not ops.attention_groups_supported(BF16, heads, d, W, True):
        pytest.skip("the grouped fused attention is not built for bf16, 8 heads of 64 with gradients")
    groups = [(0, 2, 40), (80, 3, 24)]  # two geometries: the pointer, lse and delta offsets of the second group are all non-zero
    rows = sum(N * L for _, N, L in groups)
    qkv = _rand(rows, W, dt=BF16, seed=1, scale=0.5).requires_grad_()
    valids = [torch.ones(N, L, dtype=torch.bool, device=DEV) for _, N, L in groups]
    valids[0][1, 25:] = False
    valids[1][0, 23:] = False
    valids[1][2, 10:] = False
    dO = _rand(rows, E, dt=BF16, seed=2)
    O = ops.attention_groups(qkv, groups, valids, heads, d)
    assert tuple(O.shape) == (rows, E) and O.dtype == BF16
    O.backward(dO)
    assert torch.isfinite(O).all() and torch.isfinite(qkv.grad).all()
    for (r0, N, L), valid in zip(groups, valids):
        c = qkv.detach()[r0:r0 + N * L].clone().view(N, L, W).requires_grad_()
        o = ops.attention(c, c, c, 0, E, 2 * E, heads, d, key_valid=valid)
        o.backward(dO[r0:r0 + N * L].view(N, L, E))
        _close(O.detach()[r0:r0 + N * L].view(N, L, E), o.detach(), 3e-2, "attention_groups O, group at row %d" % r0)
        _close(qkv.grad[r0:r0 + N * L].view(N, L, W), c.grad, 2 * 3e-2, "attention_groups dqkv, group at row %d" % r0)
