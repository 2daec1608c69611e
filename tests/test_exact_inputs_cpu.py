"""Pins tests/exact_inputs.py on the CPU: for every committed case the reference alone is exact -- the same operation accumulated in f32 in
three shuffled orders (and cut into partial sums, as split-K and split-KV do) equals the float64 restatement in every bit -- and every cap
the GPU tests rely on holds: K * 225 < 2^24, enough bf16 outputs that round (and enough exact ties), at most 10 % marked causal rows.
For K8 every restated product (A1, B1, A2, B2 with the bf16 roundings in between) is pinned the same way; for K16 the integer stages, the
pre-activations whose GELU is exact, the f32 LayerNorm restatement against the 0.1 % cap, eps_phi and the reach of the permutations."""
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


# ---------------------------------------------------------------------------------------------------------------------------------
# K8 (tests/test_interaction_exact_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def _shuffled_f32(a, b, seed, splits=3):
    """a [.., M, K] @ b [.., K, N] accumulated in f32 with K permuted and cut into partial sums."""
    K = a.shape[-1]
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(seed))
    out = torch.zeros(a.shape[:-1] + (b.shape[-1],), dtype=F32)
    for idx in perm.chunk(max(1, min(splits, K))):
        out = out + a.float()[..., idx] @ b.float()[..., idx, :]
    return out


def _k8_id(case):
    args, kw = case
    return "B%d-P%d-nq%d-Lp%d" % args + "".join("-%s%s" % (k, v) for k, v in kw.items())


@pytest.mark.parametrize("case", X.all_k8_cases(), ids=_k8_id)
def test_interaction_restatement_is_exact_in_f32_in_any_order(case):
    args, kw = case
    c = X.k8(*args, **kw)
    Eq, Ep, qv, pv = c.pairs()
    w = c.w.reshape(-1)
    w1, w2, w3 = w[:512], w[512:1024], w[1024:]
    for t in (Eq, Ep, w, Eq * w3 + w2):
        assert torch.equal(t.to(BF16).to(F64), t), "operands, and w3 Eq + w2 as the kernel holds it in LDS, are exact in bf16"
    assert (w3[c.code] == X.K8_W3).all() and w3.count_nonzero() == len(c.code) and w1.count_nonzero() == 1 and w2.count_nonzero() == 1
    assert all(d // 64 == c.gk for d in c.code) and len({c.gk, c.m1 // 64, c.m2 // 64}) == 3
    payload = torch.ones(512, dtype=torch.bool)
    payload[c.code + [c.m1, c.m2]] = False
    assert Eq[..., payload].abs().max() <= c.v_bound and Ep[..., payload].abs().max() <= c.v_bound
    # the masks: scattered padding (holes inside the 32-row chunks of every ordinary passage), a two-row passage, a dead query
    assert (pv.sum(-1) == 2).any() and (qv.sum(-1) == 0).any() and c.q_marked.any() and c.p_marked.any()
    full = pv.sum(-1) > 2
    holes = (~pv[full]).reshape(int(full.sum()), -1, 32)
    assert (holes.any(-1) & ~holes.all(-1)).any(-1).all(), "every ordinary passage has holes inside a 32-row chunk"
    pos = torch.arange(c.Lp)
    assert ((torch.where(pv[full], c.Lp, pos).min(-1).values) < (torch.where(pv[full], pos, -1).max(-1).values)).all(), "the padding is no tail"
    r = X.interaction_restated(Eq, Ep, qv, pv, c.w)
    raw = r["raw"]
    live = pv[:, :, None] & qv[:, None, :]
    U = raw["U"]
    assert ((U[live] % 2.0 ** 20) == 0).all() and U[live].min() >= -2.0 ** 22, "a score is a multiple of 2^20: exp of a difference is 1 or 0"
    for name in ("A", "Bt"):
        P = raw[name]
        nz = P[P > 0]
        n = (1.0 / nz).round().long()
        assert torch.equal(1.0 / n.to(F64), nz) and ((n & (n - 1)) == 0).all(), "every probability is 1 / 2^k"
        assert torch.equal(P.to(BF16).to(F64), P)
    assert (raw["A"].sum(-1)[live.any(-1)] == 1).all() and (raw["Bt"].sum(-1)[live.any(1)] == 1).all()
    # w1 / w2 act: a marked query column is out of every softmax over j, a marked passage row out of every softmax over i
    qm, pm = [t.reshape(c.B, -1, t.shape[-1]) for t in (c.q_marked, c.p_marked)]
    qm = (qm.expand(c.B, c.P, 64) if c.nq != c.P else qm).reshape(-1, 64)
    assert (raw["A"].transpose(1, 2)[qm] == 0).all() and (raw["Bt"].transpose(1, 2)[pm.reshape(-1, c.Lp)] == 0).all()
    assert (raw["A"][pm.reshape(-1, c.Lp) & pv].sum(-1)[qv.any(-1)[:, None].expand(-1, c.Lp)[pm.reshape(-1, c.Lp) & pv]] == 1).all()
    A, Bt = r["A"], r["Bt"]
    A1, B1 = X.bf16_f64(raw["A1"]), X.bf16_f64(raw["B1"])
    for i, seed in enumerate(ORDERS):
        for name, a, b in (("A1", A, Eq), ("B1", Bt, Ep), ("A2", A, B1), ("B2", Bt, A1)):
            got = _shuffled_f32(a, b, seed, splits=(1, 3, 4)[i])
            assert torch.equal(got.to(F64), raw[name]), "%s accumulated in f32 in order %d differs from float64" % (name, seed)
    for name in ("EpA1", "EpA2", "EqB1", "EqB2"):
        assert torch.equal(raw[name].float().to(F64), raw[name]), "a product of two bf16 values is exact in f32"
    # enough outputs that round (on the rows that hold anything), and exact ties
    rows_p, rows_q = (pv & qv.any(-1)[:, None]), (qv & pv.any(-1)[:, None])
    share = {k: X.bf16_inexact_and_ties(raw[k][rows_p if k in ("A1", "A2", "EpA1", "EpA2") else rows_q]) for k in raw if k not in ("U", "A", "Bt")}
    if c.v_bound == X.V_BOUND and not kw.get("orphan"):
        assert share["A1"][0] >= 0.15 and share["B1"][0] >= 0.10 and min(share[k][0] for k in ("EpA1", "EpA2", "EqB1", "EqB2")) >= 0.5, share
        assert share["A1"][1] >= 20 and share["B1"][1] >= 20 and share["EpA1"][1] >= 20, share
    else:
        assert min(share[k][0] for k in ("EpA1", "EpA2", "EqB1", "EqB2")) >= 0.05, share
    if kw.get("orphan"):
        assert (raw["A"] == 1.0 / 32).any() and (raw["Bt"] == 1.0 / 64).any() and share["A2"][0] > 0 and share["B2"][0] > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# K16 (tests/test_encoder_chain_exact_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def _bits16(t):
    return t.to(F32).to(BF16).view(torch.int16)


@pytest.mark.parametrize("kind", ["A", "Ap"])
def test_chain_family_a_is_exact_and_its_layer_norm_restatement_holds(kind):
    lay = X.chain_layer(kind)
    M = 2048
    ctx, s = X.chain_tokens(M, 100, "zero"), X.chain_tokens(M, 101, "small")
    for t in (ctx, s, lay["Wo"], lay["g2"], lay["be2"]):
        assert torch.equal(t.to(BF16).to(F64), t)
    assert not lay["W1"].any() and not lay["b1"].any() and not lay["b2"].any() and lay["W2"].any()
    assert (lay["g2"] == 0).any() and (lay["g2"] < 0).any() and (lay["be2"] < 0).any() and lay["bo"].any()
    assert len(torch.unique(ctx, dim=0)) > M * 0.6 and len(torch.unique(s, dim=0)) == M, "a different row per token"
    y = X.chain_y(ctx, s, lay)
    assert y.abs().max() < 2 ** 24 and 512 * 225 + 32 < 2 ** 24
    for i, seed in enumerate(ORDERS):
        got = X.shuffled_f32_gemm("nt", ctx, lay["Wo"], seed, splits=(1, 3, 4)[i]) + lay["bo"].float() + s.float()
        assert torch.equal(got.to(F64), y)
    ref, xhat = X.layer_norm64(y, lay["g2"], lay["be2"], X.CHAIN_EPS2)
    for two_pass in (False, True):
        got = X.layer_norm_f32(y, lay["g2"], lay["be2"], X.CHAIN_EPS2, 3, two_pass).to(BF16)
        flips = (got.view(torch.int16) != _bits16(ref)).double().mean().item()
        assert flips <= 1e-3 / 30, "the f32 restatement stays a factor 30 inside the 0.1 %% cap: %.2e" % flips
        assert ((got.to(F64) - ref).abs() <= X.layer_norm_bound(ref, xhat, lay["g2"], lay["be2"])).all()
    # eps_ln2 and eps_ln1_next differ visibly: on the quiet rows most elements move by more than a bf16 step when they are swapped
    other = X.layer_norm64(y, lay["g2"], lay["be2"], X.CHAIN_EPS1N)[0]
    quiet = torch.arange(M) % 3 == 1
    moved = ((other - ref).abs() > 2.0 ** -7 * ref.abs())[quiet][:, lay["g2"] != 0]
    assert moved.double().mean() > 0.8
    # rows with a large mean: the one-pass restatement itself leaves the bound (out of scope, recorded on the GPU)
    y8 = y + 8.0 * 2048.0
    ref8, xhat8 = X.layer_norm64(y8, lay["g2"], lay["be2"], X.CHAIN_EPS2)
    got8 = X.layer_norm_f32(y8, lay["g2"], lay["be2"], X.CHAIN_EPS2, 3).to(BF16)
    assert ((got8.to(F64) - ref8).abs() > 2.0 ** -20 * (xhat8 * lay["g2"]).abs()).any()


@pytest.mark.parametrize("kind", ["B1", "B3"])
def test_chain_family_b_pre_activations_have_an_exact_gelu(kind):
    lay = X.chain_layer(kind)
    assert not lay["g2"].any() and torch.equal(lay["be2"].to(BF16).to(F64), lay["be2"]) and lay["be2"].any()
    pre = lay["W1"] @ lay["be2"] + lay["b1"]
    assert torch.equal(pre, lay["target"]) and ((pre == 0) | (pre >= 8) | (pre <= -20)).all() and not (pre == -8).any()
    for i, seed in enumerate(ORDERS):
        got = X.shuffled_f32_gemm("nt", lay["be2"][None, :], lay["W1"], seed, splits=(1, 3, 4)[i]) + lay["b1"].float()
        assert torch.equal(got[0].to(F64), pre)
    g, _ = X.gelu_f32(pre)
    s2, a, o = X.chain_ffn(lay)
    assert torch.equal(g.to(F64), a) and torch.equal(a.to(BF16).to(F64), a), "gelu_f gives exactly 0, x or -0 (and x is exact in bf16)"
    assert (g[pre < 0] == 0).all() and torch.signbit(g[pre < 0]).all() and (a > 0).sum() > 100 and (a == 0).sum() > 100
    assert ((X.gelu_f32(torch.tensor([-8.0]))[0]) != 0).all(), "-8 is avoided: a tiny non-zero product"
    for i, seed in enumerate(ORDERS):
        got = X.shuffled_f32_gemm("nt", a[None, :], lay["W2"], seed, splits=(1, 3, 4)[i]) + (lay["b2"].float() + s2.float())
        assert torch.equal(got[0].to(F64), o)
    share, ties = X.bf16_inexact_and_ties(o)
    assert o.abs().max() < 2 ** 24 and share >= 0.5 and ties >= 5, (share, ties)
    assert (kind == "B3") == bool(lay["b2"].any())


def test_chain_gelu_grid_and_eps_phi():
    lay = X.chain_layer("B2")
    b1 = lay["b1"]
    assert torch.equal(b1.sort().values, torch.arange(512, dtype=F64) / 32 - 8) and not lay["W1"].any() and not lay["be2"].any() and not lay["b2"].any()
    eps_phi = X.gelu_eps_phi(b1)
    assert 0 < eps_phi <= 2 * 3e-7, "Abramowitz-Stegun 7.1.26 (7.5e-8 on Phi) + the f32 roundings of exp(-x^2 / 2) and 1 - q: %.2e" % eps_phi
    a = X.gelu_f32(b1)[0].to(BF16).to(F64)
    o = lay["W2"] @ a
    assert torch.equal(o.to(BF16).to(F64), o), "+-2^k times a bf16 value is a bf16 value"


@pytest.mark.parametrize("r", X.CHAIN_PERMS)
def test_chain_permutations_reach_every_fragment_of_the_pack(r):
    for w in (X.signed_perm(r, 23, blocks=3), X.chain_layer("Ap")["Wo"], X.chain_layer("B3")["W1"], X.chain_layer("B2")["W2"]):
        blocks = w.shape[0] // 512
        nz = (w != 0).reshape(blocks, 32, 16, 16, 32)          # [slot, feature block, feature, K step, k]
        assert nz.any(-1).any(2).all(), "every (16 features x 32 k) fragment holds a non-zero entry"
        assert ((w != 0).sum(1) == 1).all() and ((w != 0).reshape(blocks, 512, 512).sum(1) == 1).all(), "a permutation per block"
        v = w[w != 0].abs()
        assert torch.equal(torch.exp2(torch.log2(v).round()), v) and v.min() >= 0.5 and v.max() <= 4 and (w < 0).any() and (w > 0).any()
    nxt = X.chain_next(r)
    assert torch.equal((nxt["bqkv"] * 4).round(), nxt["bqkv"] * 4) and nxt["bqkv"].any() and X.CHAIN_EPS2 != X.CHAIN_EPS1N
    s = torch.randn(64, 512, generator=torch.Generator().manual_seed(r)).to(BF16).to(F64)
    ref = s @ nxt["Wqkv"].t() + nxt["bqkv"]
    assert (ref.to(F32).to(F64) == ref).double().mean() >= 0.99, "+-2^k s + b is exact in f32 for all but a tiny s"


def test_chain_geometry():
    assert X.CHAIN_M == (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 257)
    for cus in (128, 120):  # the grid of the large-M cases on 256 / 248 compute units
        for rem, split in ((cus // 4, True), (cus // 2 + cus // 4, False)):
            M = (cus + rem) * 128 - 51
            tiles = (M + 127) // 128
            assert tiles == cus + rem and M % 128 != 0 and (2 * rem <= cus) == split and (M + 63) // 64 > 2 * cus
