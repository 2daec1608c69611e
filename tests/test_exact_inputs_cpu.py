"""Pins tests/exact_inputs.py on the CPU: for every committed case the reference alone is exact -- the same operation accumulated in f32 in
three shuffled orders (and cut into partial sums, as split-K and split-KV do) equals the float64 restatement in every bit -- and every cap
the GPU tests rely on holds: K * 225 < 2^24, enough bf16 outputs that round (and enough exact ties), at most 10 % marked causal rows."""
import math

import pytest
import torch

import exact_inputs as X

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
ORDERS = (11, 12, 13)


def _gemm_cases():
    out = []
    for tile, shapes in X.GEMM_SHAPES.items():
        for shape in shapes:
            out += [(layout,) + shape for layout in (("nt", "nn", "tn", "tt") if tile == 128 else ("nt", "nn", "tn"))]
    out += [("nt",) + X.GEMM_PERSISTENT, ("tn",) + X.GEMM_SLAB]
    out += [(layout, M, N, X.GEMM_SPLIT_K) for layout in ("tn", "nt") for (M, N) in ((256, 512), (128, 192), (200, 136))]
    out += [("nt",) + s for s in X.GEMM_EPILOGUE_SHAPE.values()]
    return sorted(set(out))


@pytest.mark.parametrize("layout,M,N,K", _gemm_cases())
def test_gemm_reference_is_exact_in_f32_in_any_order(layout, M, N, K):
    assert X.gemm_exact_k(K)
    a, b = X.gemm_operands(layout, M, N, K, X.gemm_seed(M, N, K))
    for t in (a, b):
        assert t.abs().max() <= 15 and ((t == 0).any() or t.numel() < 8)
        assert torch.equal(t.to(BF16).to(F64), t), "operands are exact in bf16"
    ref = X.gemm_product(layout, a, b)
    assert ref.abs().max() < 2 ** 24
    for i, seed in enumerate(ORDERS):
        got = X.shuffled_f32_gemm(layout, a, b, seed, splits=(1, 3, 4)[i])
        assert torch.equal(got.to(F64), ref), "f32 accumulation in order %d differs from float64" % seed
    for alpha in (0.5, 0.25):  # the epilogue's scalings, biases and residual stay exact too
        bias, res = X.ints((N,), 3), X.ints((M, N), 4)
        want, _ = X.epilogue(ref, alpha=alpha, bias_col=bias, residual=res)
        got = (torch.tensor(alpha, dtype=F32) * ref.float() + bias.float()[None, :]) + res.float()
        assert torch.equal(got.to(F64), want)


@pytest.mark.parametrize("layout,M,N,K", [c for c in _gemm_cases() if c[3] >= 256 and c[1:] not in (X.GEMM_PERSISTENT, X.GEMM_SLAB)])
def test_gemm_bf16_outputs_round_and_tie(layout, M, N, K):
    """With K >= 256 most outputs need more than the 8 bits of a bf16 significand: a store that truncated, or rounded ties away from
    even, cannot pass."""
    a, b = X.gemm_operands(layout, M, N, K, X.gemm_seed(M, N, K))
    share, ties = X.bf16_inexact_and_ties(X.gemm_product(layout, a, b))
    assert share >= 0.25, share
    assert ties >= 20, ties


def test_round_bf16_is_to_nearest_even():
    x = torch.tensor([257.0, 259.0, 258.0, -257.0, 1025.0, 3.0], dtype=F64)  # ties: 257 -> 256 (even), 259 -> 260; 1025 rounds down
    assert X.round_bf16(x).tolist() == [256.0, 260.0, 258.0, -256.0, 1024.0, 3.0]
    with pytest.raises(AssertionError):
        X.round_bf16(torch.tensor([1.0 + 2.0 ** -30], dtype=F64))


def test_lengths_and_parts():
    assert X.pow2_parts(292) == [256, 32, 4] and X.pow2_parts(0) == [] and X.pow2_parts(1) == [1]
    for Lk in (5, 8, 37, 70, 72, 129, 200, 292, 320, 376, 384, 520, 1000, 3840, 8200):
        n = X.cut_length(Lk)
        assert 0 < n < Lk and len(X.pow2_parts(n)) <= 4 and (Lk < 16 or n % 2 == 1), (Lk, n)
    assert X.ragged_lengths(72) == [72, 45, 1, 0]


def _slices(case, step=4):
    """The case cut into groups of ``step`` items (bounds the memory of the f32 replays)."""
    for lo in range(0, case.N, step):
        hi = min(case.N, lo + step)
        c = X.AttnCase()
        c.__dict__.update(case.__dict__)
        c.N = hi - lo
        for name in ("q", "k", "v", "key_valid", "key_class", "query_class", "marked"):
            setattr(c, name, getattr(case, name)[lo:hi])
        yield c


def _id(case):
    args, kw = case
    return "-".join(str(a) for a in args) + "".join("-%s" % (v[0] if isinstance(v, list) else v) for v in kw.values())


@pytest.mark.parametrize("case", X.all_attention_cases(), ids=_id)
def test_attention_reference_is_exact_in_f32_in_any_order(case):
    args, kw = case
    whole = X.attn(*args, **kw)
    d, scale = whole.d, 1.0 / math.sqrt(whole.d)
    assert whole.marked.any(-1).any(-1).sum() == 0 or whole.causal
    if whole.causal:
        share = whole.marked.double().mean().item()
        assert share <= 0.10, "marked rows: %.3f" % share
    if "lengths" not in kw:
        assert whole.lengths[:4] == X.ragged_lengths(whole.Lk)
    assert 0 in whole.lengths and 1 in whole.lengths and max(whole.lengths) > 0
    for c in _slices(whole):
        for t, bound in ((c.q, X.CODE), (c.k, X.CODE), (c.v, X.V_BOUND)):
            assert t.abs().max() <= bound and torch.equal(t.to(BF16).to(F64), t)
        P = c.probabilities()
        s = X.scores(c)
        inside = P > 0
        assert (s[inside] == 0).all(), "a key of the query's class scores exactly 0"
        vis = c.key_valid[:, None, None, :].expand_as(s) & ~inside & (c.query_class[..., None] >= 0)
        if c.causal:
            vis = vis & torch.ones(c.Lq, c.Lk, dtype=torch.bool).tril()
        if c.mode != "uniform":
            assert (s[vis] <= -2.0 ** 20).all(), "every other visible key scores -2^20 or less"
            assert math.exp(-2.0 ** 20 / math.sqrt(512)) == 0.0
        else:
            assert not vis.any() and (c.q == 0).all() and (c.k != 0).any()
        n = inside.sum(-1)
        free = ~c.marked
        assert ((n & (n - 1)) == 0)[free].all(), "the visible class size is a power of two on every unmarked row"
        assert (n[c.query_class < 0] == 0).all() and (n[c.query_class >= 0] > 0).all()
        O = c.output()
        vh = c.heads(c.v).float()
        for seed in ORDERS:
            p32 = X.softmax_f32(c, scale, seed)
            assert torch.equal(p32.to(F64)[free], P[free]), "f32 online softmax in order %d" % seed
            perm = torch.randperm(c.Lk, generator=torch.Generator().manual_seed(seed))
            acc = torch.zeros(c.N, c.h, c.Lq, d)
            for idx in perm.chunk(min(4, c.Lk)):
                acc = acc + p32[..., idx] @ vh[:, :, idx, :]
            assert torch.equal(acc.to(F64)[free], c.heads(O)[free]), "f32 P V in order %d" % seed
        assert torch.equal(c.heads(O).float().to(F64)[free], c.heads(O)[free])
        if c.Lq == 1:
            continue
        # backward: dV exact in any order; case A: dS = 0; case B: dK = 0
        dO = X.grad_output(c, 5)
        assert not c.heads(dO)[c.marked].any() and c.heads(dO)[free].any(), "dO is zero on the marked rows only"
        o_read = c.merge(torch.where(free[..., None], c.heads(O), torch.zeros_like(c.heads(O))))  # (a marked row's O meets dO = 0)
        dQ, dK, dV, _ = c.backward(dO, scale, o_read=X.round_bf16(o_read).to(F64))
        gh = c.heads(dO).float()
        p32 = X.softmax_f32(c, scale, 3)  # marked rows: not exact, and multiplied by dO = 0
        perm = torch.randperm(c.Lq, generator=torch.Generator().manual_seed(3))
        acc = torch.zeros(c.N, c.h, c.Lk, d)
        for idx in perm.chunk(min(3, c.Lq)):
            acc = acc + p32.transpose(-1, -2)[..., idx] @ gh[:, :, idx, :]
        assert torch.equal(acc.to(F64), c.heads(dV)), "f32 P^T dO"
        if c.causal:  # dV feels the mask: a query that also saw the keys behind it would spread its dO over another class size
            c2 = X.AttnCase()
            c2.__dict__.update(c.__dict__)
            c2.causal = False
            assert not torch.equal(c2.backward(dO, scale)[2], dV)
        if c.mode == "class_const":
            assert torch.equal(X.round_bf16(o_read).to(F64), o_read), "case A: O is the class constant, exact in bf16"
            assert dQ.abs().max() == 0 and dK.abs().max() == 0
        if c.mode == "uniform":
            assert dK.abs().max() == 0 and dQ.abs().max() > 0


def test_recomputed_probability_rounds_to_the_exact_one():
    """A backward kernel that recomputes P = exp(S - lse) gets exp(-log n): within 1e-7 of 1/n, and exactly 1/n once rounded to bf16."""
    n = torch.arange(1, 4097, dtype=F32)
    n = n[(n.int() & (n.int() - 1)) == 0]
    for p in (torch.exp(-torch.log(n)), torch.exp2(-torch.log2(n)), torch.exp2(-(torch.log(n) * 1.4426950408889634))):
        assert ((p - 1 / n).abs() <= 1e-7).all()
        assert torch.equal(p.to(BF16).float(), 1 / n)


@pytest.mark.parametrize("B,S", X.MQA)
def test_mqa_reference_is_exact(B, S):
    c, qp, qc = X.mqa_case(B, S, seed=B * 10007 + S)
    assert torch.equal(c.k.to(BF16).to(F64), c.k) and torch.equal(qp.to(BF16).to(F64), qp) and c.k is c.v
    out, P = X.mqa_output(c, qc)
    s = qp.reshape(B, 8, 512) @ c.k[:, :, :].transpose(-1, -2)
    assert (s[P > 0] == 0).all()
    other = c.key_valid[:, None, :].expand_as(s) & ~(P > 0)
    assert (s[other] <= -2.0 ** 20).all()
    n = (P > 0).sum(-1)
    assert ((n & (n - 1)) == 0).all()
    for seed in ORDERS:
        perm = torch.randperm(S, generator=torch.Generator().manual_seed(seed))
        acc = torch.zeros(B, 8, 512)
        for idx in perm.chunk(min(5, S)):
            acc = acc + P.float()[..., idx] @ c.k.float()[:, idx, :]
        assert torch.equal(acc.reshape(B, -1).to(F64), out)
