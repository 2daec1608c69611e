"""The MFMA GEMM family (csrc/gemm.hip, gemm_impl.inc, gemm8w.inc, gemm_small.inc) on operands for which every product and every partial
sum is exact in f32 (tests/exact_inputs.py; pinned on the CPU by test_exact_inputs_cpu.py): integers in [-15, 15], K * 225 < 2^24.  The
result then does not depend on the summation order, the tiling, the split or the order of the f32 atomics, so there is no tolerance:

* an f32 output equals the float64 restatement in every bit,
* a bf16 output has the bits of ref.to(f32).to(bf16): ONE rounding to nearest even (common.h, f32x2_to_bf16x2).  With K >= 256 more than a
  quarter of the outputs round and at least twenty are exact ties, so a truncating store or another tie rule cannot pass.

Every C is prefilled with NaN (an element the kernel never writes is seen), operand padding is NaN (an element outside the extent that
reaches an accumulator is seen), and every call asserts the tiling case_gemm_tile_for reports for it: no case quietly runs elsewhere."""
import pytest
import torch

import exact_inputs as X
import exact_ledger as L
from exact_ledger import ledger  # noqa: F401  (autouse fixture)
from test_small_ops_gpu import _counting, _nan
from test_small_ops_gpu import _same_bits as _same_bits_raw

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
DTYPES = [(F32, F32), (BF16, BF16), (BF16, F32)]
DT_IDS = ["f32-f32", "bf16-bf16", "bf16-f32"]


def _same_bits(got, want, what):
    _same_bits_raw(got, want, what)
    L.record(got.numel())


def _ops():
    from case_rg_amd import config, ops
    config.set_dropout(False)
    return ops


def _want(ref, dt):
    """float64 reference -> the only bits the kernel may store."""
    f = ref.to(F32)
    assert torch.equal(f.to(F64), ref), "the reference itself is not exact in f32"
    return f if dt == F32 else f.to(BF16)


def _lds(layout, M, N, K):
    ak, bk = X.LAYOUTS[layout]
    return (M if ak else K), (N if bk else K)


def _block(t, dt, pad, mis):
    """``t`` [R, C] as a column block of a NaN-filled [R, C + pad] buffer that starts ``mis`` elements into its allocation:
    -> (tensor whose data pointer is the block's first element, leading dimension, the whole buffer)."""
    R, C = t.shape
    ld = C + pad
    buf = torch.full((mis + R * ld,), float("nan"), dtype=dt, device=DEV)
    view = buf[mis:].view(R, ld)
    view[:, :C] = t.to(DEV).to(dt)
    return buf[mis:], ld, view


def _gemm(ops, tile, layout, a, b, c, M, N, K, lda=None, ldb=None, ldc=None, runs_on=None, **kw):
    ak, bk = X.LAYOUTS[layout]
    la, lb = _lds(layout, M, N, K)
    ops.TILE_TRACE, ops.GEMM_TILE = [], tile
    try:
        ops.gemm(a, b, c, M, N, K, lda or la, ldb or lb, ldc or N, a_kmajor=ak, b_kmajor=bk, **kw)
        trace = ops.TILE_TRACE
    finally:
        ops.GEMM_TILE, ops.TILE_TRACE = 0, None
    torch.cuda.synchronize()
    assert trace == [runs_on or tile], "asked for the %d tiling, case_gemm_tile_for reports %s" % (tile, trace)
    return c


def _operands(layout, M, N, K, in_dt):
    a, b = X.gemm_operands(layout, M, N, K, X.gemm_seed(M, N, K))
    ref = X.gemm_product(layout, a.to(DEV), b.to(DEV))  # float64 on the device: integers, exact in any order
    return a.to(DEV).to(in_dt), b.to(DEV).to(in_dt), ref


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the 128x128 tiling
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dt,out_dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("layout", ["nt", "nn", "tn", "tt"])
def test_tile128_layouts_edges_and_k_tails(layout, in_dt, out_dt):
    """Edge tiles in both extents, K tails of the 64- (bf16) and 32-element (f32) K tile, the scalar-load path (K % 8 != 0), 1 and 3 K
    tiles; then the same contents one element into their allocations and with ld > extent for A, B and C."""
    ops = _ops()
    for (M, N, K) in X.GEMM_SHAPES[128]:
        a, b, ref = _operands(layout, M, N, K, in_dt)
        want = _want(ref, out_dt)
        c = _gemm(ops, 128, layout, a, b, _nan(M, N, dt=out_dt), M, N, K)
        _same_bits(c, want, "128 tiling %s %s" % (layout, (M, N, K)))
        (pa, lda, _), (pb, ldb, _) = _block(a, in_dt, 3, 1), _block(b, in_dt, 5, 1)
        pc, ldc, cview = _block(torch.full((M, N), float("nan")), out_dt, 7, 1)
        _gemm(ops, 128, layout, pa, pb, pc, M, N, K, lda, ldb, ldc)
        _same_bits(cview[:, :N], want, "128 tiling %s %s misaligned, padded" % (layout, (M, N, K)))
        assert torch.isnan(cview[:, N:].float()).all(), "columns outside the C block were written"


@pytest.mark.parametrize("in_dt", [F32, BF16], ids=["f32", "bf16"])
def test_tile128_two_level_batch_strides_of_the_attention_scores(in_dt):
    """S[n, h] = alpha Q[n, :, h] K[n, :, h]^T with the heads addressed in place inside packed projections (batch1 = 2 items, batch2 = 3
    heads, Lq 5, Lk 7, d 4), as AttentionFn._probabilities issues it."""
    ops = _ops()
    n, h, Lq, Lk, d = 2, 3, 5, 7, 4
    E = h * d
    q, kv = X.ints((n, Lq, E), 41).to(DEV), X.ints((n, Lk, 2 * E), 42).to(DEV)
    for alpha in (1.0, 0.5, 0.25):
        S = _nan(n, h, Lq, Lk + 3)
        ops.TILE_TRACE = []
        try:
            ops.gemm(q.to(in_dt), kv.to(in_dt), S, Lq, Lk, d, E, 2 * E, Lk + 3, b_off=E, batch1=n, batch2=h, sa=(Lq * E, d),
                     sb=(Lk * 2 * E, d), sc=(h * Lq * (Lk + 3), Lq * (Lk + 3)), alpha=alpha)
            assert ops.TILE_TRACE == [128]
        finally:
            ops.TILE_TRACE = None
        qh = q.reshape(n, Lq, h, d).transpose(1, 2)
        kh = kv[..., E:].reshape(n, Lk, h, d).transpose(1, 2)
        _same_bits(S[..., :Lk], _want(alpha * (qh @ kh.transpose(-1, -2)), F32), "batched scores alpha=%s" % alpha)
        assert torch.isnan(S[..., Lk:]).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. the 256x256 and the 64x64 tilings
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dt", [BF16, F32], ids=["bf16-bf16", "bf16-f32"])
@pytest.mark.parametrize("layout", ["nt", "nn", "tn"])
@pytest.mark.parametrize("tile", [256, 64])
def test_dma_tilings_layouts_and_k_tile_counts(tile, layout, out_dt):
    """256: 1 .. 5 K tiles (pipeline prologue and tail) and several output tiles; 64: 1, 3 and 10 K tiles resident in LDS."""
    ops = _ops()
    for (M, N, K) in X.GEMM_SHAPES[tile]:
        a, b, ref = _operands(layout, M, N, K, BF16)
        c = _gemm(ops, tile, layout, a, b, _nan(M, N, dt=out_dt), M, N, K)
        _same_bits(c, _want(ref, out_dt), "%d tiling %s %s" % (tile, layout, (M, N, K)))


def test_tile256_persistent_loop():
    """320 output tiles on 256 CUs: workgroups walk several tiles (the cross-tile prefetch)."""
    ops = _ops()
    M, N, K = X.GEMM_PERSISTENT
    a, b, ref = _operands("nt", M, N, K, BF16)
    c = _gemm(ops, 256, "nt", a, b, _nan(M, N, dt=BF16), M, N, K)
    _same_bits(c, _want(ref, BF16), "persistent 256 tiling")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. epilogues
# ---------------------------------------------------------------------------------------------------------------------------------
def _keep_mask(ops, M, N, seed, offset):
    """The keep mask of the dropout site (p = 0.5, seed, offset) over M * N elements, from case_dropout on ones: the GEMM epilogue's counter
    for element (row, col) is offset + row * N + col."""
    y = ops._dropout_raw(torch.ones(M * N, device=DEV), 0.5, seed, offset)
    assert set(y.unique().tolist()) == {0.0, 2.0}, "p = 0.5: the scale is exactly 2"
    return (y != 0).view(M, N)


@pytest.mark.parametrize("tile,in_dt,out_dt", [(128,) + p for p in DTYPES] + [(t,) + p for t in (256, 64) for p in DTYPES[1:]],
                         ids=["128-" + i for i in DT_IDS] + ["%d-%s" % (t, i) for t in (256, 64) for i in DT_IDS[1:]])
def test_epilogues_in_the_documented_order(tile, in_dt, out_dt):
    """alpha * acc + bias -> RELU -> MUL_DRELU -> DROPOUT -> + RESIDUAL, each word (and the combinations the model issues) bit for bit."""
    ops = _ops()
    from case_rg_amd import _abi as A
    M, N, K = X.GEMM_EPILOGUE_SHAPE[tile]
    a, b, acc = _operands("nt", M, N, K, in_dt)
    bias_c, bias_r = X.ints((N,), 51).to(DEV), X.ints((M,), 52).to(DEV)
    res, sg = X.ints((M, N), 53).to(DEV), X.signs((M, N), 54).to(DEV)
    assert (sg > 0).any() and (sg == 0).any() and (sg < 0).any()
    bc32, br32 = bias_c.float(), bias_r.float()
    ld_aux = N + 8  # aux with its own leading dimension
    res_p, sg_p = [_block(t, in_dt, 8, 0) for t in (res, sg)]

    def run(epi, want, what, **kw):
        c = _gemm(ops, tile, "nt", a, b, _nan(M, N, dt=out_dt), M, N, K, epilogue=epi, **kw)
        _same_bits(c, _want(want, out_dt), "%d tiling, %s" % (tile, what))

    run(A.EPI_BIAS_COL, X.epilogue(acc, bias_col=bias_c)[0], "BIAS_COL", bias_col=bc32)
    run(A.EPI_BIAS_ROW, X.epilogue(acc, bias_row=bias_r)[0], "BIAS_ROW", bias_row=br32)
    run(A.EPI_BIAS_COL | A.EPI_BIAS_ROW, X.epilogue(acc, bias_col=bias_c, bias_row=bias_r)[0], "BIAS_COL | BIAS_ROW", bias_col=bc32, bias_row=br32)
    # RELU: the ABI saves a pre-activation for GELU only (include/case_hip.h; the ReLU backward reads the activation itself): aux_out stays untouched
    saved = _nan(M, N, dt=in_dt)
    run(A.EPI_BIAS_COL | A.EPI_RELU, X.epilogue(acc, bias_col=bias_c, relu=True)[0], "BIAS_COL | RELU", bias_col=bc32, aux_out=saved, ld_aux=N)
    assert torch.isnan(saved.float()).all(), "RELU wrote aux_out on the %d tiling: only GELU saves its pre-activation" % tile
    assert (X.epilogue(acc, bias_col=bias_c)[0] < 0).any()
    run(A.EPI_MUL_DRELU, X.epilogue(acc, drelu_aux=sg)[0], "MUL_DRELU", aux=sg_p[0], ld_aux=ld_aux)
    run(A.EPI_BIAS_COL | A.EPI_RESIDUAL, X.epilogue(acc, bias_col=bias_c, residual=res)[0], "BIAS_COL | RESIDUAL", bias_col=bc32, aux=res_p[0], ld_aux=ld_aux)
    for alpha in (0.5, 0.25):
        if out_dt == F32:
            run(A.EPI_BIAS_COL, X.epilogue(acc, alpha=alpha, bias_col=bias_c)[0], "alpha %s" % alpha, bias_col=bc32, alpha=alpha)
    seed, offset = 1234, 77
    keep = _keep_mask(ops, M, N, seed, offset)
    assert 0.45 < keep.double().mean().item() < 0.55
    run(A.EPI_BIAS_COL | A.EPI_RESIDUAL, X.epilogue(acc, bias_col=bias_c, keep=keep, residual=res)[0], "BIAS_COL | DROPOUT | RESIDUAL",
        bias_col=bc32, aux=res_p[0], ld_aux=ld_aux, drop=(0.5, seed, offset))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. split-K with f32 atomics
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tn", "nt"])
@pytest.mark.parametrize("tile,in_dt", [(128, F32), (128, BF16), (256, BF16), (64, BF16)], ids=["128-f32", "128-bf16", "256", "64"])
def test_split_k_atomics_are_exact_whatever_the_order(tile, in_dt, layout):
    """K = 64 * 11 cut unevenly into 3 and 4 splits; the column bias arrives once, not once per split; C is accumulated into.  The 256
    tiling takes the bare ATOMIC epilogue only (gemm.hip, prepare): with a bias the call runs on the 128 tiling, which is asserted."""
    ops = _ops()
    from case_rg_amd import _abi as A
    K = X.GEMM_SPLIT_K
    M, N = {128: (200, 136), 256: (256, 512), 64: (128, 192)}[tile]
    a, b, ref = _operands(layout, M, N, K, in_dt)
    bias = X.ints((N,), 61).to(DEV)
    assert (bias != 0).sum() > N // 2
    base = X.ints((M, N), 62).to(DEV)
    for split in (3, 4):
        c = _gemm(ops, tile, layout, a, b, torch.zeros(M, N, device=DEV), M, N, K, split_k=split, epilogue=A.EPI_ATOMIC)
        _same_bits(c, _want(ref, F32), "%d tiling split_k=%d %s" % (tile, split, layout))
        c = _gemm(ops, tile, layout, a, b, torch.zeros(M, N, device=DEV), M, N, K, split_k=split, epilogue=A.EPI_ATOMIC | A.EPI_BIAS_COL,
                  bias_col=bias.float(), runs_on=128 if tile == 256 else tile)
        _same_bits(c, _want(ref + bias[None, :], F32), "%d tiling split_k=%d with bias_col %s" % (tile, split, layout))
    c = _gemm(ops, tile, layout, a, b, base.float().clone(), M, N, K, split_k=4, epilogue=A.EPI_ATOMIC)
    _same_bits(c, _want(ref + base, F32), "%d tiling split_k=4 onto a C that holds integers" % tile)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. weight-gradient forms
# ---------------------------------------------------------------------------------------------------------------------------------
def test_weight_gradient_with_the_bias_gradient_and_its_fallback():
    """rowsum_out: dW = dY^T X and the bias gradient (column sums of dY) -- inside the launch where the 256 tiling takes the call
    (case_gemm_dw_bias), by case_colsum + case_gemm where it does not."""
    ops = _ops()
    from case_rg_amd import _abi as A
    ran = set()
    shapes = ((64 * 24, 512, 256, 3), (64 * 40, 768, 512, 5), (64 * 7, 256, 256, 1), (64 * 9, 320, 256, 2))
    # every shape under the cost model; the interior ones once more with the 256 tiling asked for, so that the fused form runs whatever the model picks
    for (Mtok, N, K, split), force in [(s, 0) for s in shapes] + [(s, 256) for s in shapes if s[1] % 256 == 0]:
        g, x = X.ints((Mtok, N), 71).to(DEV), X.ints((Mtok, K), 72).to(DEV)
        dw, db = torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
        ops.TILE_TRACE, ops.GEMM_TILE = [], force
        try:
            with _counting() as calls:
                ops.gemm(g.to(BF16), x.to(BF16), dw, N, K, Mtok, N, K, K, a_kmajor=True, b_kmajor=True, split_k=split, epilogue=A.EPI_ATOMIC,
                         rowsum_out=db)
            tile = ops.TILE_TRACE[0]
        finally:
            ops.TILE_TRACE, ops.GEMM_TILE = None, 0
        torch.cuda.synchronize()
        fused = tile == 256
        assert calls == ({"case_gemm_dw_bias": 1} if fused else {"case_colsum": 1, "case_gemm": 1}), (calls, tile)
        assert fused or not force, "asked for the 256 tiling on an interior problem and left the fused form"
        assert not fused or N % 256 == 0
        ran.add(fused)
        _same_bits(dw, _want(g.t() @ x, F32), "dW N=%d K=%d tokens=%d (fused %s)" % (N, K, Mtok, fused))
        _same_bits(db, _want(g.sum(0), F32), "bias gradient N=%d (fused %s)" % (N, fused))
    assert ran == {True, False}, "both the fused form and the fallback must have run"


@pytest.mark.parametrize("bias", [True, False], ids=["rowsum", "plain"])
@pytest.mark.parametrize("split", [8, 13])
def test_weight_gradient_through_split_slabs(split, bias):
    """case_gemm_dw_slabs: one f32 slab per split and an ordered reduction; C is accumulated into."""
    ops = _ops()
    from case_rg_amd import _abi as A
    N, K, Mtok = X.GEMM_SLAB
    g, x, ref = _operands("tn", N, K, Mtok, BF16)
    base = X.ints((N, K), 81).to(DEV)
    dw, db = base.float().clone(), (torch.zeros(N, device=DEV) if bias else None)
    ops.GEMM_TILE = 256
    try:
        with _counting() as calls:
            ops.gemm(g, x, dw, N, K, Mtok, N, K, K, a_kmajor=True, b_kmajor=True, split_k=split, epilogue=A.EPI_ATOMIC, rowsum_out=db)
    finally:
        ops.GEMM_TILE = 0
    torch.cuda.synchronize()
    assert calls == {"case_gemm_dw_slabs": 1}, calls
    _same_bits(dw, _want(ref + base, F32), "slab dW split %d" % split)
    if bias:
        _same_bits(db, _want(g.double().sum(0), F32), "bias gradient beside the slabs")


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. autograd shells
# ---------------------------------------------------------------------------------------------------------------------------------
def _r(t, dt):
    """What a tensor of dtype ``dt`` holds of the float64 value ``t`` (one rounding where dt is bf16), back in float64."""
    return _want(t, dt).to(F64)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,K,N", [(136, 72, 40), (256, 320, 256)])
def test_linear_with_bias_and_residual_forward_and_every_gradient(dt, M, K, N):
    ops = _ops()
    x, w, b, r, dy = [X.ints(s, 90 + i).to(DEV) for i, s in enumerate(((M, K), (N, K), (N,), (M, N)))] + [X.ints((M, N), 95, bound=3).to(DEV)]
    xt, rt = x.to(dt).requires_grad_(), r.to(dt).requires_grad_()
    wt, bt = w.float().requires_grad_(), b.float().requires_grad_()
    with _counting() as calls:
        y = ops.linear(xt, wt, bt, residual=rt)
    assert calls.get("case_gemm") == 1, calls
    _same_bits(y, _want(x @ w.t() + b + r, dt), "linear forward")
    y.backward(dy.to(dt))
    _same_bits(xt.grad, _want(dy @ w, dt), "linear dX")
    _same_bits(wt.grad, _want(dy.t() @ x, F32), "linear dW")
    _same_bits(bt.grad, _want(dy.sum(0), F32), "linear db")
    _same_bits(rt.grad, dy.to(dt), "linear d residual")


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("res_is_x", [False, True], ids=["residual", "residual-is-x"])
def test_ffn_relu_with_residual_forward_and_every_gradient(dt, res_is_x):
    """The float64 reference rounds the inner activation (and its gradient) to bf16 where the op stores them in bf16."""
    ops = _ops()
    M, K, F_ = 72, 24, 40
    x, w1, b1, w2, b2, r = [X.ints(s, 100 + i).to(DEV) for i, s in enumerate(((M, K), (F_, K), (F_,), (K, F_), (K,), (M, K)))]
    dy = X.ints((M, K), 107, bound=3).to(DEV)
    xt = x.to(dt).requires_grad_()
    rt = xt if res_is_x else r.to(dt).requires_grad_()
    ps = [t.float().requires_grad_() for t in (w1, b1, w2, b2)]
    y = ops.ffn(xt, ps[0], ps[1], ps[2], ps[3], "relu", residual=rt)
    a = _r((x @ w1.t() + b1).clamp_min(0), dt)
    rr = x if res_is_x else r
    _same_bits(y, _want(a @ w2.t() + b2 + rr, dt), "ffn forward")
    y.backward(dy.to(dt))
    dz = _r(torch.where(a > 0, dy @ w2, torch.zeros_like(a)), dt)
    assert (a > 0).any() and (a == 0).any()
    _same_bits(ps[2].grad, _want(dy.t() @ a, F32), "ffn dW2")
    _same_bits(ps[3].grad, _want(dy.sum(0), F32), "ffn db2")
    _same_bits(ps[0].grad, _want(dz.t() @ x, F32), "ffn dW1")
    _same_bits(ps[1].grad, _want(dz.sum(0), F32), "ffn db1")
    if res_is_x:
        _same_bits(xt.grad, _want(dz @ w1 + dy, dt), "ffn dX with the residual gradient in the epilogue")
    else:
        _same_bits(xt.grad, _want(dz @ w1, dt), "ffn dX")
        _same_bits(rt.grad, dy.to(dt), "ffn d residual")


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_linear_skinny_on_integer_operands(dt):
    ops = _ops()
    rows, widths, nout = 33, (96, 40, 8, 24), 8
    xs = [X.ints((rows, 1, w), 110 + i).to(DEV) for i, w in enumerate(widths)]
    W, b = X.ints((nout, sum(widths)), 115).to(DEV), X.ints((nout,), 116).to(DEV)
    with torch.no_grad():
        assert ops.linear_skinny_supported([x.to(dt) for x in xs], W.float())
        with _counting() as calls:
            y = ops.linear_skinny([x.to(dt) for x in xs], W.float(), b.float())
    assert calls == {"case_linear_skinny": 1}
    _same_bits(y, _want(torch.cat(xs, -1) @ W.t() + b, F32), "linear_skinny")


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_bmm_kn_with_a_row_bias_and_f32_output(dt):
    ops = _ops()
    n, M, K, N = 3, 37, 24, 21
    a, b, bias = X.ints((n, M, K), 120).to(DEV), X.ints((n, K, N), 121).to(DEV), X.ints((n, M), 122).to(DEV)
    dc = X.ints((n, M, N), 123, bound=3).to(DEV)
    at, bt = a.to(dt).requires_grad_(), b.to(dt).requires_grad_()
    c = ops.bmm(at, bt, b_is_kn=True, bias_row=bias.float(), out_dtype=F32)
    _same_bits(c, _want(a @ b + bias[..., None], F32), "bmm forward")
    c.backward(dc.float())
    _same_bits(at.grad, _want(dc @ b.transpose(1, 2), dt), "bmm dA")
    _same_bits(bt.grad, _want(a.transpose(1, 2) @ dc, dt), "bmm dB")
