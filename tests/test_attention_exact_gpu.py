"""The attention family (csrc/attention.hip, attention_wide.inc, attn64.hip, attn_scores.hip, attn_mqa.hip) and the GEMM + softmax + GEMM
path on operands whose softmax is exact (tests/exact_inputs.py; pinned on the CPU by test_exact_inputs_cpu.py): a score is 0 inside the
query's class and -2^20 outside, so every probability is exactly 1/n with n a power of two, V is integers, and O is the exact class mean.

* forward: the bits of the float64 mean rounded ONCE to bf16 (f32 on the f32 path) -- whatever the tile, chunk, split or merge order;
* backward, case A (V constant inside every class): dQ = dK = 0 in every element, dV exact;
* backward, case B (Q = 0, the uniform softmax, V varying): dK = 0, dV exact, dQ within 2^-7 * scale * sum_j |dS_ref[i, j]| |k_j| plus half
  a bf16 ulp (two bf16 roundings of dS -- P and dS itself -- each doubled);
* causal rows whose visible class size is no power of two (at most 10 % of a case): 2^-8 * sum_j p_j |v_j| plus half a bf16 ulp.

key_valid is ragged in every case: one item full, one cut mid-tile, one with a single valid key, one with none (exact zeros).  Each test
asserts the C entry points that ran."""
import math
import os

import pytest
import torch

import exact_inputs as X
import exact_ledger as L
from exact_ledger import ledger  # noqa: F401  (autouse fixture)
from test_small_ops_gpu import _check, _counting, _half_ulp_bf16, _nan, _raw
from test_small_ops_gpu import _same_bits as _same_bits_raw

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64


@pytest.fixture
def ops():
    from case_rg_amd import config, ops
    config.set_dropout(False)
    mode = ops.ATTENTION_MODE
    yield ops
    ops.ATTENTION_MODE = mode


def _same_bits(got, want, what):
    _same_bits_raw(got, want, what)
    L.record(got.numel())


def _zero(t, what):
    assert int(torch.count_nonzero(t)) == 0 and not torch.isnan(t.float()).any(), "%s: %d elements are not zero" % (what, int(torch.count_nonzero(t)))
    L.record(t.numel())


def _once(ref, dt):
    """float64 -> the stored dtype in ONE rounding to nearest even (through f32, which holds every reference built here exactly, or -- for
    the f32 path's alpha = 1/sqrt(d) products -- takes the one rounding itself)."""
    return ref.to(F32) if dt == F32 else X.round_bf16(ref)


def _bounded(got, ref, f32_err, what, reason):
    tol = f32_err + (_half_ulp_bf16(ref.abs() + f32_err) if got.dtype == BF16 else 0.0)
    _check(got, ref, tol, what)
    L.record(0, got.numel(), reason)


def _rows(case, mask):
    """[N, h, Lq] -> [N, Lq, h d] (a row mask spread over the head's columns)."""
    return mask.to(DEV)[..., None].expand(case.N, case.h, case.Lq, case.d).transpose(1, 2).reshape(case.N, case.Lq, case.h * case.d)


def _sources(case, dt, grad):
    """The projections as the op takes them: one packed [N, L, 3E] tensor for self-attention, q [N, Lq, E] and K | V [N, Lk, 2E] otherwise."""
    E = case.h * case.d
    if case.Lq == case.Lk:
        qkv = torch.cat([case.q, case.k, case.v], -1).to(DEV).to(dt).requires_grad_(grad)
        return (qkv, qkv, qkv, 0, E, 2 * E), (qkv,)
    q = case.q.to(DEV).to(dt).requires_grad_(grad)
    kv = torch.cat([case.k, case.v], -1).to(DEV).to(dt).requires_grad_(grad)
    return (q, kv, kv, 0, 0, E), (q, kv)


def _grads(case, leaves):
    E = case.h * case.d
    if len(leaves) == 1:
        g = leaves[0].grad
        return g[..., :E], g[..., E:2 * E], g[..., 2 * E:]
    return leaves[0].grad, leaves[1].grad[..., :E], leaves[1].grad[..., E:]


def _check_forward(case, o, what):
    ref = case.output(DEV)
    marked = _rows(case, case.marked)
    if not case.marked.any():
        _same_bits(o, _once(ref, o.dtype), what + ": O")
        return ref
    free = ~marked
    _same_bits(o[free], _once(ref[free], o.dtype), what + ": O on the rows whose visible class size is a power of two")
    absv = case.merge(case.probabilities(DEV) @ case.heads(case.v.to(DEV)).abs())
    _bounded(o[marked], ref[marked], 2.0 ** -8 * absv[marked], what + ": O on the marked rows",
             "causal rows whose visible class size is no power of two: 1/n is not exact, each probability may round to bf16 once")
    return ref


def _attend(ops, case, dt, want_calls, backward=True, seed=5):
    """ops.attention forward (and backward for the modes that define one) on ``case``; asserts the entry points."""
    srcs, leaves = _sources(case, dt, backward)
    valid = case.key_valid.to(DEV)
    what = "%s N=%d h=%d Lq=%d Lk=%d d=%d%s %s" % (case.mode, case.N, case.h, case.Lq, case.Lk, case.d, " causal" if case.causal else "", dt)
    assert all(t.data_ptr() % 16 == 0 for t in leaves) and valid.data_ptr() % 4 == 0  # (no misalignment keeps a case off the resident kernels)
    with _counting() as calls:
        o = ops.attention(*srcs, case.h, case.d, key_valid=valid, causal=case.causal)
    for name, n in want_calls.items():
        assert calls.get(name, 0) == n, "%s: expected %d x %s, the op made %s" % (what, n, name, calls)
    o_ref = _check_forward(case, o.detach(), what)
    none = [i for i, n in enumerate(case.lengths) if n == 0]
    assert none and int(torch.count_nonzero(o.detach()[none])) == 0, "an item without a valid key gives exact zeros"
    if not backward:
        return o, calls
    scale = float(torch.tensor(1.0 / math.sqrt(case.d), dtype=F32))  # what the kernels multiply by: the f32 value of 1 / sqrt(d)
    dO = X.grad_output(case, seed).to(DEV)
    with _counting() as bcalls:
        o.backward(dO.to(dt))
    fused = calls.get("case_attention_fwd", 0) + calls.get("case_attention_fwd_splitkv", 0) > 0
    assert (bcalls.get("case_attention_bwd", 0) == 1) == fused, "%s: backward made %s" % (what, bcalls)
    dq, dk, dv = _grads(case, leaves)
    # The fused backward reads its own bf16 O for delta = rowsum(dO * O) (equal to the reference on every row with a nonzero dO: asserted
    # above); the softmax backward of the unfused path sums P * dP.  In a causal case dO is zero on the marked rows (exact_inputs.grad_output),
    # so they add exactly nothing and every assertion below holds for the whole tensors: dV = P^T dO over the unmarked rows sees every key
    # each of them may and may not look at.
    assert not dO[_rows(case, case.marked)].any()
    rq, rk, rv, bq = case.backward(dO, scale, o_read=o.detach().double() if fused else None, device=DEV)
    _same_bits(dv, _once(rv, dt), what + ": dV")
    if case.mode == "class_const":
        _zero(dq, what + ": dQ (case A)")
        _zero(dk, what + ": dK (case A)")
    if case.mode == "uniform":
        _zero(dk, what + ": dK (case B)")
        if dt == F32:
            _same_bits(dq, _once(rq, dt), what + ": dQ (case B, f32)")
        else:
            _bounded(dq, rq, 2.0 ** -7 * bq, what + ": dQ (case B)", "case B: dS is rounded to bf16 twice (P and dS itself), each doubled")
    return o, calls


def _resident(case):
    """Whether attn64.hip takes the case.  The choice is made inside case_attention_fwd / case_attention_bwd and is not reported through the
    ABI, so it is INFERRED here from the rule those entry points apply (fa64::fwd_ok: head_dim 64, not causal, 288 < Lk <= 384, Lk % 4 == 0,
    Lq <= 384; the single-pass backward: also Lq > 256) and from the things that would switch it off, which are asserted: the A/B switches
    CASE_ATTN_RESIDENT / CASE_ATTN_RESIDENT_BWD are not "0"; the operands are 16-byte aligned and key_valid 4-byte aligned because
    _sources and _attend pass fresh allocations (checked in _attend)."""
    for switch in ("CASE_ATTN_RESIDENT", "CASE_ATTN_RESIDENT_BWD"):
        assert not os.environ.get(switch, "").startswith("0"), "%s switches the resident kernels off: these cases would run attention.hip" % switch
    return case.d == 64 and not case.causal and 288 < case.Lk <= 384 and case.Lk % 4 == 0 and case.Lq <= 384


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. case_attention_fwd / case_attention_bwd at every built head size
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["classes", "class_const", "uniform"])
@pytest.mark.parametrize("shape", X.FUSED_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("d", X.FUSED_D)
def test_fused_forward_and_backward_at_every_head_size(ops, d, shape, mode):
    from case_rg_amd import _abi as A
    assert A.lib.case_attention_supported(d)
    ops.ATTENTION_MODE = "fused"
    case = X.attn(*shape, d, mode=mode)
    backward = bool(A.lib.case_attention_bwd_supported(d)) and mode != "classes"
    _attend(ops, case, BF16, {"case_attention_fwd": 1}, backward=backward)


def test_every_built_head_size_is_covered():
    from case_rg_amd import _abi as A
    assert [d for d in range(1, 1025) if A.lib.case_attention_supported(d)] == list(X.FUSED_D)


@pytest.mark.parametrize("mode", ["classes", "class_const"])
@pytest.mark.parametrize("d", X.CAUSAL_D)
def test_fused_causal(ops, d, mode):
    ops.ATTENTION_MODE = "fused"
    case = X.attn(*X.CAUSAL_SHAPE, d, causal=True, mode=mode)
    assert case.marked.any(), "the case has rows for the bound as well"
    _attend(ops, case, BF16, {"case_attention_fwd": 1})  # "classes": dV exact; "class_const": dV exact, dQ = dK = 0


@pytest.mark.parametrize("mode", ["classes", "class_const", "uniform"])
def test_flash_kernels_at_head_dim_64_beyond_the_resident_range(ops, mode):
    """(4, 3, 130, 292) at head_dim 64 runs the resident kernel; Lk = 520 keeps the flash-style forward and backward of attention.hip covered."""
    ops.ATTENTION_MODE = "fused"
    assert _resident(X.attn(*X.FUSED_SHAPES[1], 64)) and not _resident(X.attn(*X.FLASH_64, 64))
    _attend(ops, X.attn(*X.FLASH_64, 64, mode=mode), BF16, {"case_attention_fwd": 1}, backward=mode != "classes")


def test_forward_writes_every_element_of_a_nan_filled_output(ops):
    """The raw entry point onto NaN-filled O and LSE (the op allocates with torch.empty): flash, resident and wide head sizes."""
    for shape, d in ((X.FUSED_SHAPES[0], 32), (X.FUSED_SHAPES[1], 64), (X.FLASH_64, 64), (X.FUSED_SHAPES[1], 320)):
        case = X.attn(*shape, d)
        E = case.h * d
        q, kv = case.q.to(DEV).to(BF16), torch.cat([case.k, case.v], -1).to(DEV).to(BF16)
        valid = case.key_valid.to(DEV).to(torch.uint8)
        ad = ops._attn_desc(case.N, case.h, case.Lq, case.Lk, d, q, kv, kv, False, 1.0 / math.sqrt(d), None)
        O, lse = _nan(case.N, case.Lq, E, dt=BF16), _nan(case.N, case.h, case.Lq)
        _raw("case_attention_fwd", ad, q, kv, ops._ptr(kv, E), valid, O, lse)
        _check_forward(case, O, "raw forward %s d=%d" % (shape, d))
        seen = (case.probabilities(DEV) > 0).any(-1)
        assert torch.isfinite(lse[seen]).all(), "LSE of a row with a visible key"


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the resident head_dim-64 kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["classes", "class_const", "uniform"])
@pytest.mark.parametrize("shape", X.RESIDENT_SELF + X.RESIDENT_CROSS, ids=lambda s: "x".join(map(str, s)))
def test_resident_kernels(ops, shape, mode):
    """Self-attention at L 292 and 384; separate query and memory tensors at (1, 384) and (257, 292): the single-pass backward takes
    Lq > 256, the others run the flash-style backward on the resident forward's output."""
    ops.ATTENTION_MODE = "fused"
    case = X.attn(*shape, 64, mode=mode)
    assert _resident(case)
    _attend(ops, case, BF16, {"case_attention_fwd": 1}, backward=mode != "classes")


def test_resident_kernels_with_more_items_than_workgroups(ops):
    """40 x 8 = 320 (item, head) pairs on 256 persistent workgroups: the DMA stream crosses item boundaries.  With this many items some
    query's only class member inside a 96-key chunk is key 27 or 31 of the chunk -- the score the forward's chunk maximum used to leave
    out (register 15 of the first key tile), which gave 334 NaN rows of 102 400 here."""
    ops.ATTENTION_MODE = "fused"
    case = X.attn(*X.RESIDENT_MANY, 64, mode="class_const")
    assert _resident(case) and case.N * case.h > 256
    _attend(ops, case, BF16, {"case_attention_fwd": 1})


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. split-KV
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["classes", "class_const", "uniform"])
def test_split_kv_forward_and_the_backward_behind_it(ops, mode):
    """Lk 3840 in four chunks of 960 keys: the class of 2048 keys spans every seam, the cut item has no valid key in the last chunk."""
    ops.ATTENTION_MODE = "fused"
    N, h, Lq, Lk = X.SPLIT_KV
    case = X.attn(N, h, Lq, Lk, 64, mode=mode)
    splits = ops._kv_splits(N, h, Lq, Lk, False)
    assert splits > 1
    chunk = -(-Lk // splits)
    assert 0 < case.lengths[1] <= Lk - chunk, "one item has no valid key in the last chunk"
    if mode != "uniform":
        big = (case.key_class[0, 0] == 0).nonzero().flatten()
        assert len(big) == 2048 and len(set((big // chunk).tolist())) == splits, "the class of 2048 keys has members in every chunk"
    _attend(ops, case, BF16, {"case_attention_fwd_splitkv": 1, "case_attention_fwd": 0}, backward=mode != "classes")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the decode step
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,h,Lk", X.DECODE)
def test_decode_step(ops, N, h, Lk):
    case = X.attn(N, h, 1, Lk, 64)
    assert N * h >= ops.DECODE_MIN_PAIRS
    with torch.no_grad():
        _attend(ops, case, BF16, {"case_attention_decode": 1, "case_attention_fwd": 0}, backward=False)


@pytest.mark.parametrize("t", X.DECODE_APPEND_T)
def test_decode_step_with_the_cache_append(ops, t):
    """The K | V columns of position t come from qkv and are written into the cache by the launch: the returned attention is exact, the
    appended row has the bits of the qkv columns, every other cache row is untouched."""
    N, h, T = X.DECODE_APPEND
    d, E = 64, h * 64
    case = X.attn(N, h, 1, T, d, lengths=X.decode_append_lengths(N, t))
    kv = torch.cat([case.k, case.v], -1).to(DEV).to(BF16)
    qkv = torch.cat([case.q.to(DEV).to(BF16), kv[:, t:t + 1]], -1).contiguous()
    cache = kv.clone()
    cache[:, t] = float("nan")
    before = cache.clone()
    with torch.no_grad():
        assert ops.decode_append_supported(qkv, cache, h, d)
        with _counting() as calls:
            o = ops.attention_decode_append(qkv, cache, t, h, d, key_valid=case.key_valid.to(DEV))
    assert calls == {"case_attention_decode_append": 1}
    _check_forward(case, o, "decode append t=%d" % t)
    _same_bits(cache[:, t], qkv[:, 0, E:], "the appended cache row")
    rest = [i for i in range(T) if i != t]
    _same_bits(cache[:, rest], before[:, rest], "the other cache rows")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. K17: the score kernels and the row-complete product
# ---------------------------------------------------------------------------------------------------------------------------------
def _scores_launch(ops, case):
    from case_rg_amd import _abi as A
    E = case.h * case.d
    q, kv = case.q.to(DEV).to(BF16), torch.cat([case.k, case.v], -1).to(DEV).to(BF16)
    ad = ops._attn_desc(case.N, case.h, case.Lq, case.Lk, case.d, q, kv, kv, False, 1.0 / math.sqrt(case.d), None)
    assert A.lib.case_attention_scores_supported(ad)
    P = _nan(case.N, case.h, case.Lq, case.Lk, dt=BF16)
    _raw("case_attention_scores_fwd", ad, q, kv, case.key_valid.to(DEV).to(torch.uint8), P, None)
    return ad, kv, P


@pytest.mark.parametrize("d,Lk", X.SCORES)
def test_scores_forward_writes_exactly_one_over_n_or_zero(ops, d, Lk):
    case = X.attn(4, 2, 40, Lk, d)
    _, _, P = _scores_launch(ops, case)
    _same_bits(P, X.round_bf16(case.probabilities(DEV)), "K17 P d=%d Lk=%d" % (d, Lk))


@pytest.mark.parametrize("mode", ["class_const", "uniform"])
@pytest.mark.parametrize("d,Lk", X.SCORES)
def test_scores_backward(ops, d, Lk, mode):
    """dS = P (g - rowsum(g P)), g = dO V^T.  Case A: exactly zero.  Case B: dS within the two-rounding bound of case B."""
    case = X.attn(4, 2, 40, Lk, d, mode=mode)
    ad, kv, P = _scores_launch(ops, case)
    Pref = case.probabilities(DEV)
    _same_bits(P, X.round_bf16(Pref), "K17 P")
    dO = X.grad_output(case, 5).to(DEV)
    dS = _nan(case.N, case.h, case.Lq, case.Lk, dt=BF16)
    _raw("case_attention_scores_bwd", ad, dO.to(BF16), ops._ptr(kv, case.h * d), P, dS)
    g = case.heads(dO) @ case.heads(case.v.to(DEV)).transpose(-1, -2)
    ref = Pref * (g - (g * Pref).sum(-1, keepdim=True))
    if mode == "class_const":
        assert ref.abs().max() == 0
        _zero(dS, "K17 dS (case A)")
    else:
        assert ref.abs().max() > 0
        _bounded(dS, ref, 2.0 ** -7 * ref.abs(), "K17 dS (case B)", "case B: dS is rounded to bf16 (P and dS itself), each doubled")


@pytest.mark.parametrize("alpha", [1.0, 0.5, 0.25])
@pytest.mark.parametrize("N,heads,La,Lb,transposed", [(3, 2, 200, 256, False), (3, 2, 192, 136, True)])
def test_attention_product_on_integer_operands(ops, N, heads, La, Lb, transposed, alpha):
    """case_attention_product (head_dim 320) as a GEMM: c = alpha A b, A = mat or mat^T, packed strided operands, exact."""
    d, E = 320, heads * 320
    mat = X.ints((N, heads, La, Lb), 131).to(DEV)
    M, Kc = (Lb, La) if transposed else (La, Lb)
    assert X.gemm_exact_k(Kc)
    b_src = X.ints((N, Kc, 3 * E), 132).to(DEV)
    out = _nan(N, M, 2 * E, dt=BF16)
    b_off, c_off = 2 * E, E
    with _counting() as calls:
        assert ops.AttentionFn._product(mat.to(BF16), b_src.to(BF16), b_off, out, c_off, heads, d, M, Kc, transposed, alpha)
    assert calls == {"case_attention_product": 1}
    A64 = mat.transpose(-1, -2) if transposed else mat
    B64 = b_src[:, :, b_off:b_off + E].reshape(N, Kc, heads, d).permute(0, 2, 1, 3)
    want = (alpha * (A64 @ B64)).permute(0, 2, 1, 3).reshape(N, M, E)
    _same_bits(out[:, :, c_off:c_off + E], X.round_bf16(want), "product transposed=%s alpha=%s" % (transposed, alpha))
    assert torch.isnan(out[:, :, :c_off].float()).all() and torch.isnan(out[:, :, c_off + E:].float()).all(), "neighbouring columns were written"


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. MQA decode on the raw memory rows
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S", X.MQA)
def test_mqa_decode(ops, B, S):
    from case_rg_amd import _abi as A
    case, qp, qc = X.mqa_case(B, S, seed=B * 10007 + S)
    splits = A.lib.case_attention_decode_mqa_splits(B, S)
    assert splits > 1 or S < 8000, "the (1, 8200) case must take the split path: %d ranges" % splits
    with _counting() as calls:
        out = ops.attention_decode_mqa(qp.to(DEV).to(BF16), case.k.to(DEV).to(BF16), case.key_valid.to(DEV))
    assert calls == {"case_attention_decode_mqa": 1}
    ref, _ = X.mqa_output(case, qc, DEV)
    _same_bits(out, X.round_bf16(ref), "MQA decode B=%d S=%d" % (B, S))


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the unfused path: GEMM + case_softmax_* + GEMM
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("N,h,Lq,Lk,d,causal,mode", [s + (m,) for s in X.UNFUSED for m in ("classes", "class_const", "uniform") if not (s[5] and m == "uniform")])
def test_unfused_path(ops, N, h, Lq, Lk, d, causal, mode, dt):
    """In f32 everything is the float64 value rounded once (alpha = 1/sqrt(d) is no power of two at d 20), dQ of case B included.  Case B
    is defined without the causal mask."""
    ops.ATTENTION_MODE = "unfused"
    # Case B on this path: the bf16 form stores dP = dO V^T as bf16 before the softmax backward, and |dP| <= 3 * |V| * d.  With |V| <= 4
    # and d = 20 that is 240 < 2^8, so dP is exact in bf16 and the only roundings left are the two of dS the bound allows (at |V| <= 127 a
    # rounded dP would enter dS = P (dP - delta) through a cancellation the bound does not cover).  In f32 the same operands keep dS
    # = (dP - mean) / n within 8 + 14 bits and its products with the 2^10 codes within 24, so dQ is exact up to the one rounding by alpha.
    case = X.attn(N, h, Lq, Lk, d, causal=causal, mode=mode, v_bound=4 if mode == "uniform" else X.V_BOUND)
    _attend(ops, case, dt, {"case_softmax_fwd": 1, "case_attention_fwd": 0, "case_attention_scores_fwd": 0}, backward=causal or mode != "classes")
