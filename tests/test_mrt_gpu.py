"""Minimum-risk training on the MI355X: K29 with row statistics and its backward K41 (``ops.pointer_head_score_grad``) on inputs where
every operation is exact and on random inputs against a float64 restatement; K42 (``ops.sequence_risk``) against the host form
``evaluation.sequence_risk_host``; ``do_mrt`` of a tiny CaSE and a tiny Masque against ``do_score``, ``rouge_l_ids`` and the host form,
its gradients with the fused head against the unfused chain, sampling, the mode switch and the capturing trainer.

Measured maxima go to profiles/mrt_parity.json."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import Calls, head_inputs, scaled_error

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
CAP = 2e-5  # the bar K23's ``gen`` is held to: no bar below is looser
# K41 on random inputs: ten times the larger of the two errors measured on the MI355X against the float64 restatement, max |err| / max |ref|
# per tensor over every V and offset of the test (profiles/mrt_parity.json: the existing unfused f32 chain 5.389e-07, K41 3.669e-07).  Both
# carry the error of __expf and of the f32 divisions in gen and pm.
K41_BAR = min(CAP, 10 * 5.389e-07)
# the fused head against the unfused chain inside a whole do_mrt step: ten times the largest distance measured on the MI355X (the worst
# parameter gradient, tiny Masque in fp32: 1.726e-06; CaSE 9.344e-07; token_probs 1.490e-08, the loss 0).  The weight gradients behind both
# heads are f32 atomic sums, whose order differs from run to run.
STEP_BAR = min(CAP, 10 * 1.726e-06)
# LinearSkinnyFn against float64 torch autograd: every output is a sum of at most 192 f32 products (3 x 64 input columns forward, 130 rows
# in dW), so its rounding error is below 192 x 2^-24 = 1.1e-5 of the sum of the terms' magnitudes; relative to max |ref| per tensor the cap.
SKINNY_BAR = CAP


def _measured(key, value, bar=None):
    """Add one measured maximum to profiles/mrt_parity.json."""
    path = os.path.join(ROOT, "profiles", "mrt_parity.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = {}
    if os.path.exists(path):
        with open(path) as fh:
            data = json.load(fh)
    data[key] = {"measured": float("%.3e" % value), "bar": bar}
    with open(path, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)
        fh.write("\n")


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class _Unfused:
    """CASE_POINTER_SCORE=off for the block."""

    def __enter__(self):
        from case_rg_amd import ops
        self.old, ops.POINTER_SCORE = ops.POINTER_SCORE, "off"

    def __exit__(self, *exc):
        from case_rg_amd import ops
        ops.POINTER_SCORE = self.old


# ---------------------------------------------------------------------------------------------
# 1. K41 on inputs where every operation is exact
# ---------------------------------------------------------------------------------------------
EXACT_V = 1024
TOK_ONCE, TOK_65, TOK_130, TOK_ABSENT = 600, 601, 602, 700


def _exact_source(rows, S, seed):
    """Source ids [rows, S]: background ids in [10, 500) and, where they fit, a token that occurs once, a run of 65 positions (the whole
    row at S = 65: it ends at S), a run of 130 positions that ends at S, id V - 1 once and id 0 once."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(10, 500, (rows, S), generator=g)
    if S >= 200:
        ids[:, 0:65] = TOK_65
        ids[:, S - 130:S] = TOK_130
        ids[:, 66], ids[:, 67], ids[:, 68] = TOK_ONCE, EXACT_V - 1, 0
    elif S == 65:
        ids[:, :] = TOK_65
    elif S >= 63:
        ids[:, 5], ids[:, S - 1], ids[:, 7] = TOK_ONCE, EXACT_V - 1, 0
    else:
        ids[:, 0] = TOK_ONCE
    return ids


def _split(S, nmem):
    base = S // nmem
    return [S - base * (nmem - 1)] + [base] * (nmem - 1)


@pytest.mark.parametrize("pad", [0, -1])
@pytest.mark.parametrize("R,rps,S,nmem", [(1, 1, 1, 1), (3, 1, 63, 2), (3, 1, 64, 3), (5, 5, 65, 4), (130, 5, 200, 3), (130, 1, 200, 1),
                                          (130, 5, 200, 4), (130, 1, 200, 2)])
def test_k41_exact(R, rps, S, nmem, pad):
    """All logits 0 and V = 1024 (gen = 2^-10, stats = (0, V)), equal mixing logits (pm = 1 / (1 + nmem): exact for nmem 1 and 3, one
    rounding for 2 and 4), copy weights that are multiples of 2^-10 and g a power of two (or 0): every element of d_logits, d_mix and
    d_copy_k is one or two correctly rounded f32 operations on exact operands, restated below in numpy f32 operation by operation, and must
    agree bit for bit (the sign of a zero included).  prob is an INPUT of K41: the restatement takes the forward's."""
    from case_rg_amd import ops
    V = EXACT_V
    lens = _split(S, nmem)
    g = torch.Generator().manual_seed(1000 + R + S + nmem)
    src = _exact_source(R // rps, S, 7 + S)
    logits = torch.zeros(R, V, device=DEV)
    mix = torch.zeros(R, 1 + nmem, device=DEV)
    copies = [(torch.randint(0, 8, (R, n), generator=g).float() / 1024).to(DEV) for n in lens]
    cycle = [TOK_ONCE, TOK_65, TOK_130, V - 1, 0, -1, V, TOK_ABSENT]
    targets = torch.tensor([cycle[r % len(cycle)] for r in range(R)], dtype=torch.int64)
    grow = torch.tensor([0.0 if r % 7 == 3 else 2.0 ** ((r % 6) - 3) for r in range(R)])
    sm = ops.SortedSource(src.to(DEV), V)
    with torch.no_grad():
        prob, copy, stats = ops.PointerScoreFn.apply(logits, mix, sm, rps, targets.to(DEV), pad, *copies)
        k29_prob, k29_copy = ops.pointer_head_score(logits, mix, sm, rps, copies, targets.to(DEV), pad)
    assert _same_bits(prob, k29_prob) and _same_bits(copy, k29_copy), "the forward through _stats has K29's bits"
    scored = (targets >= 0) & (targets < V) & (targets != pad if pad >= 0 else torch.ones(R, dtype=torch.bool))
    want_stats = torch.where(scored.unsqueeze(1), torch.tensor([0.0, float(V)]).expand(R, 2), torch.zeros(R, 2))
    assert _same_bits(stats.cpu(), want_stats), "stats = (0, V) on a scored row, (0, 0) elsewhere"

    def launch():
        out = (torch.full((R, V), float("nan"), device=DEV), torch.full((R, 1 + nmem), float("nan"), device=DEV),
               [torch.full((R, n), float("nan"), device=DEV) for n in lens])
        return ops.pointer_head_score_bwd(logits, mix, sm.ids, rps, copies, targets.to(DEV), pad, stats, prob, grow.to(DEV), out=out)

    d_logits, d_mix, d_copies = launch()
    again = launch()
    assert _same_bits(d_logits, again[0]) and _same_bits(d_mix, again[1]) and all(_same_bits(a, b) for a, b in zip(d_copies, again[2]))

    # the restatement
    f32 = np.float32
    pm = f32(1.0) / f32(1 + nmem)
    gen = f32(1.0) / f32(V)
    probs = prob.cpu().numpy()
    cps = [c.cpu().numpy() for c in copies]
    want_l = np.zeros((R, V), dtype=f32)
    want_m = np.zeros((R, 1 + nmem), dtype=f32)
    want_c = [np.zeros((R, n), dtype=f32) for n in lens]
    starts = np.cumsum([0] + lens)
    for r in range(R):
        if not bool(scored[r]):
            continue
        y, gr = int(targets[r]), f32(grow[r])
        hit = src[r // rps].numpy() == y
        coef = (gr * pm) * gen
        onehot = np.zeros(V, dtype=f32)
        onehot[y] = 1.0
        want_l[r] = coef * (onehot - gen)
        want_m[r, 0] = (gr * pm) * (gen - probs[r])
        total = f32(0.0)
        for k in range(nmem):
            hk = hit[starts[k]:starts[k + 1]]
            ck = f32(cps[k][r][hk].astype(np.float64).sum())  # multiples of 2^-10 below 2^14: exact in any order
            total += pm * ck
            want_m[r, 1 + k] = (gr * pm) * (ck - probs[r])
            want_c[k][r] = np.where(hk, gr * pm, f32(0.0))
        if nmem in (1, 3):  # pm is a power of two: the forward itself is exact
            assert probs[r] == pm * gen + total
        run = int(hit.sum())
        assert run == {TOK_ONCE: 0 if S == 65 else 1, TOK_65: 65 if S >= 65 else 0, TOK_130: 130 if S >= 200 else 0, TOK_ABSENT: 0}.get(y, run)
    assert np.array_equal(d_logits.cpu().numpy().view(np.int32), want_l.view(np.int32)), "d_logits"
    assert np.array_equal(d_mix.cpu().numpy().view(np.int32), want_m.view(np.int32)), "d_mix"
    for k in range(nmem):
        assert np.array_equal(d_copies[k].cpu().numpy().view(np.int32), want_c[k].view(np.int32)), "d_copy_%d" % k


# ---------------------------------------------------------------------------------------------
# 2. K41 on random inputs against a float64 autograd restatement
# ---------------------------------------------------------------------------------------------
def _restated_prob(logits, mix, copies, src_rows, targets, pad):
    """prob [R] in the inputs' dtype, differentiable: pm_0 softmax(logits)[y] + sum_k pm_{1+k} sum_{s: id == y} copy_k[s]; 1 at PAD, 0
    outside the vocabulary (neither depends on the inputs)."""
    R, V = logits.shape
    inside = (targets >= 0) & (targets < V)
    skip = targets.eq(pad) if pad >= 0 else torch.zeros_like(inside)
    y = targets.clamp(0, V - 1)
    gen_y = torch.softmax(logits, dim=-1).gather(1, y.unsqueeze(1)).squeeze(1)
    pm = torch.softmax(mix, dim=-1)
    hit = src_rows.eq(y.unsqueeze(1)).to(logits.dtype)
    p, at = pm[:, 0] * gen_y, 0
    for k, c in enumerate(copies):
        p = p + pm[:, 1 + k] * (c * hit[:, at:at + c.shape[1]]).sum(dim=1)
        at += c.shape[1]
    return torch.where(skip, torch.ones_like(p), torch.where(inside, p, torch.zeros_like(p)))


def _unfused_prob(logits, mix, copies, src, targets, pad):
    """The f32 chain ``_score`` runs without K29: masked_softmax, p0 x gen, the sorted scatter, a gather."""
    from case_rg_amd import ops
    R, V = logits.shape
    gen = ops.masked_softmax(logits.clone().view(R, 1, V))  # (a fresh tensor: the chain is the yardstick, the offset row is K41's subject)
    pm = ops.masked_softmax(mix.view(R, 1, -1))
    d1 = pm[:, :, 0:1] * gen
    ptr = torch.cat([pm[:, :, k + 1:k + 2] * c.unsqueeze(1) for k, c in enumerate(copies)], dim=-1)
    d2 = ops.copy_scatter(src, ptr, V)
    inside = (targets >= 0) & (targets < V)
    at = targets.clamp(0, V - 1).reshape(R, 1, 1)
    p = d1.gather(-1, at).reshape(R) + d2.gather(-1, at).reshape(R)
    skip = targets.eq(pad) if pad >= 0 else torch.zeros_like(inside)
    return torch.where(skip, torch.ones_like(p), torch.where(inside, p, torch.zeros_like(p)))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("V", [1, 3, 4, 5, 1023, 1025, 30522])
def test_k41_random_against_float64(V, offset):
    """R = 130 rows (rows_per_source 5), two memories of 17 + 23 positions, a logits base ``offset`` floats behind a 16-byte boundary.
    Both the existing unfused f32 chain and K41 are measured against the f64 restatement, max |err| / max |ref| per tensor; every tensor
    of K41 is held to K41_BAR, the constant above.  The figures of both go to profiles/mrt_parity.json next to it."""
    from case_rg_amd import ops
    R, rps, lens, pad = 130, 5, [17, 23], (0 if V > 5 else -1)
    g = torch.Generator().manual_seed(31 * V + offset)
    flat = torch.zeros(R * V + 4, device=DEV)
    logits = flat[offset:offset + R * V].view(R, V)
    logits.copy_((torch.randn(R, V, generator=g) * 2.0).to(DEV))
    assert logits.is_contiguous() and (logits.data_ptr() % 16) == 4 * offset
    src = torch.randint(0, V, (R // rps, sum(lens)), generator=g)
    mix = torch.randn(R, 1 + len(lens), generator=g).to(DEV)
    # (rows that sum to 0.3 .. 0.9, not to 1: at V = 1 every position holds the target, and with normalised rows a_j - prob would be a pure
    #  cancellation residue of the inputs' own rounding, which no f32 evaluation can be held to)
    copies = [(torch.softmax(torch.randn(R, n, generator=g) * 2.0, dim=-1) * (0.3 + 0.6 * torch.rand(R, 1, generator=g))).to(DEV) for n in lens]
    targets = torch.randint(0, V, (R,), generator=g)
    planted = torch.arange(R) % 3 == 0  # every third row: a token of its own source
    targets[planted] = src[torch.arange(R)[planted] // rps, torch.randint(0, sum(lens), (int(planted.sum()),), generator=g)]
    targets[4], targets[9] = -1, V
    upstream = (torch.randn(R, generator=g) * 2.0).to(DEV)
    targets = targets.to(DEV)
    sm = ops.SortedSource(src.to(DEV), V)
    src_rows = sm.ids.repeat_interleave(rps, dim=0)

    def grads(prob_of, dtype):
        leaves = [t.detach().to(dtype).requires_grad_(True) for t in [logits, mix] + copies]
        p = prob_of(leaves[0], leaves[1], leaves[2:])
        return p.detach(), torch.autograd.grad((p * upstream.to(dtype)).sum(), leaves)

    ref_p, ref = grads(lambda l, m, c: _restated_prob(l, m, c, src_rows, targets, pad), torch.float64)
    k41_p, k41 = grads(lambda l, m, c: ops.pointer_head_score_grad(l, m, sm, rps, c, targets, pad)[0], torch.float32)
    # (the chain takes a logits row at any offset too, but as a fresh contiguous tensor: it is the yardstick, not the subject)
    chain_p, chain = grads(lambda l, m, c: _unfused_prob(l, m, c, sm.expand(rps), targets, pad), torch.float32)
    with torch.no_grad():
        k29_p, k29_c = ops.pointer_head_score(logits, mix, sm, rps, copies, targets, pad)
        fwd_p, fwd_c = ops.pointer_head_score_grad(logits, mix, sm, rps, copies, targets, pad)
    assert _same_bits(k41_p, k29_p) and _same_bits(fwd_p, k29_p) and _same_bits(fwd_c, k29_c), "the forward through _stats has K29's bits"
    names = ["d_logits", "d_mix"] + ["d_copy_%d" % k for k in range(len(lens))]
    worst = {}
    for name, want, got, yard in zip(names, ref, k41, chain):
        e_k41 = scaled_error(name, got.cpu().numpy(), want.cpu().numpy())
        e_chain = scaled_error(name, yard.cpu().numpy(), want.cpu().numpy())
        print("V %d offset %d %s: K41 %.3e, unfused chain %.3e, bar %.3e" % (V, offset, name, e_k41, e_chain, K41_BAR))
        _measured("k41/V%d/offset%d/%s" % (V, offset, name), e_k41, K41_BAR)
        _measured("chain/V%d/offset%d/%s" % (V, offset, name), e_chain, None)
        worst[name] = e_k41
    assert scaled_error("prob", k41_p.cpu().numpy(), ref_p.cpu().numpy()) <= K41_BAR
    assert all(e <= K41_BAR for e in worst.values()), worst


def test_linear_skinny_grad_against_float64_autograd():
    """``ops.linear_skinny_grad`` (the mixing logits of the differentiated scoring pass): the forward has ``ops.linear_skinny``'s bits, and the
    gradients of the three inputs, the weight and the bias agree with torch autograd of Linear(cat(xs)) in float64."""
    from case_rg_amd import ops
    g = torch.Generator().manual_seed(17)
    R, H, nout = 130, 64, 3
    xs = [torch.randn(R, 1, H, generator=g).to(DEV) for _ in range(3)]
    w = (torch.randn(nout, 3 * H, generator=g) * 0.1).to(DEV)
    b = torch.randn(nout, generator=g).to(DEV)
    upstream = torch.randn(R, 1, nout, generator=g).to(DEV)
    with torch.no_grad():
        plain = ops.linear_skinny(xs, w, b)
    leaves = [t.clone().requires_grad_(True) for t in xs + [w, b]]
    assert ops.linear_skinny_supported(leaves[:3], leaves[3], with_grad=True) and not ops.linear_skinny_supported(leaves[:3], leaves[3])
    with Calls() as c:
        y = ops.linear_skinny_grad(leaves[:3], leaves[3], leaves[4])
    assert c.calls == {"case_linear_skinny": 1} and _same_bits(y, plain) and y.requires_grad
    got = torch.autograd.grad((y * upstream).sum(), leaves)
    ref_leaves = [t.double().requires_grad_(True) for t in xs + [w, b]]
    ref_y = torch.nn.functional.linear(torch.cat(ref_leaves[:3], dim=-1), ref_leaves[3], ref_leaves[4])
    want = torch.autograd.grad((ref_y * upstream.double()).sum(), ref_leaves)
    worst = {"y": scaled_error("y", y.detach().cpu().numpy(), ref_y.detach().cpu().numpy())}
    for name, a, r in zip(["d_x0", "d_x1", "d_x2", "d_w", "d_b"], got, want):
        assert a.shape == r.shape and a.dtype == torch.float32
        worst[name] = scaled_error(name, a.cpu().numpy(), r.cpu().numpy())
    for name, e in worst.items():
        print("linear_skinny_grad %s: %.3e (bar %.1e)" % (name, e, SKINNY_BAR))
        _measured("linear_skinny_grad/%s" % name, e, SKINNY_BAR)
    assert all(e <= SKINNY_BAR for e in worst.values()), worst
    # only the inputs: no weight gradient is computed or returned
    only_x = torch.autograd.grad((ops.linear_skinny_grad(leaves[:3], w, b) * upstream).sum(), leaves[:3])
    assert all(_same_bits(a, r) for a, r in zip(only_x, got[:3]))


def test_k41_limits_and_graph_capture():
    """Beyond K29's limits the entry points refuse; inside them forward + backward capture into a graph and replay to the eager bits."""
    from case_rg_amd import ops
    logits, mix, sm, copies, _ = head_inputs(6, 257, [9, 11], seed=5)
    targets = torch.tensor([3, 200, 0, 256, 17, 40], device=DEV)
    upstream = torch.arange(1, 7, device=DEV, dtype=torch.float32)

    def step():
        leaves = [t.detach().requires_grad_(True) for t in [logits, mix] + copies]
        p, _ = ops.pointer_head_score_grad(leaves[0], leaves[1], sm, 1, leaves[2:], targets)
        return [p.detach()] + list(torch.autograd.grad((p * upstream).sum(), leaves))

    eager = step()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            held = step()
    torch.cuda.current_stream().wait_stream(side)
    for t in held:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert all(_same_bits(a, b) for a, b in zip(eager, held))
    with pytest.raises(RuntimeError, match="built for <= 4 memories"):
        five = [torch.rand(2, 2, device=DEV) for _ in range(5)]
        ops.pointer_head_score_bwd(torch.zeros(2, 8, device=DEV), torch.zeros(2, 6, device=DEV), torch.zeros(2, 10, dtype=torch.int64, device=DEV), 1,
                                   five, torch.zeros(2, dtype=torch.int64, device=DEV), 0, torch.zeros(2, 2, device=DEV), torch.zeros(2, device=DEV),
                                   torch.zeros(2, device=DEV))


# ---------------------------------------------------------------------------------------------
# 3. K42 against the host form
# ---------------------------------------------------------------------------------------------
def _risk_inputs(B, N, T, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(B, N, T, generator=g) * 0.999 + 1e-3
    length = torch.randint(1, T + 1, (B, N), generator=g)
    scored = torch.arange(T).view(1, 1, T) < length.unsqueeze(2)  # a PAD tail
    p[~scored] = 1.0
    cost = torch.rand(B, N, generator=g)
    valid = torch.rand(B, N, generator=g) < 0.8
    valid[:, 0] = True
    if B > 2:
        valid[1] = False  # an item without a valid candidate
        p[2, 0, 0] = 1e-35  # below the floor
        p[0, N - 1, 0] = 0.0
    return p.to(DEV), scored.to(DEV), cost.to(DEV), valid.to(DEV)


@pytest.mark.parametrize("B", [1, 130])
@pytest.mark.parametrize("T", [1, 64, 65, 256, 1024])
@pytest.mark.parametrize("N", [1, 2, 63, 64])
def test_k42_against_the_host_form(N, T, B):
    """Every output of the kernel is an f64 value rounded to f32 once, and kernel and host differ by reassociation in f64 only: against
    the host's UNROUNDED f64 values the bound is half an f32 unit, 2^-24 |ref|, plus 1e-12."""
    from case_rg_amd import ops
    from case_rg_amd.evaluation import sequence_risk_host
    p, scored, cost, valid = _risk_inputs(B, N, T, 100 * N + T + B)
    for alpha in (5e-3,) + ((1.0,) if T <= 65 else ()):
        for ok in (valid, None):
            want = sequence_risk_host(p, scored, cost, ok, alpha, rounded=False)
            leaf = p.clone().requires_grad_(True)
            risk, q = ops.sequence_risk(leaf, scored, cost, ok, alpha, want_q=True)
            upstream = torch.linspace(-1.0, 2.0, B, device=DEV)
            (grad,) = torch.autograd.grad((risk * upstream).sum(), leaf)
            risk = risk.detach()
            risk2, q2 = ops.sequence_risk(p, scored, cost, ok, alpha, want_q=True)
            assert _same_bits(risk, risk2) and _same_bits(q, q2), "two launches give equal bits"
            grad_p = torch.autograd.grad(ops.sequence_risk(leaf, scored, cost, ok, alpha).sum(), leaf)[0]
            assert _same_bits(grad, grad_p * upstream.view(-1, 1, 1)), "the backward scales the kept grad_p by the upstream gradient"
            for name, got, ref in (("risk", risk, want["risk"]), ("q", q, want["q"]), ("grad_p", grad_p, want["grad_p"])):
                assert got.dtype == torch.float32 and torch.isfinite(got).all()
                over = (got.detach().double() - ref).abs() - (2.0 ** -24 * ref.abs() + 1e-12)
                assert float(over.max()) <= 0.0, "%s (N %d, T %d, B %d, alpha %g): %.3e over the bound" % (name, N, T, B, alpha, float(over.max()))
            if ok is not None and B > 2:
                assert float(risk[1]) == 0.0 and not q[1].any() and not grad_p[1].any(), "an item without a valid candidate"
                assert float(grad_p[2, 0, 0]) == 0.0 and float(grad_p[0, N - 1, 0]) == 0.0, "no gradient below the floor"
            assert not grad_p[~scored.expand_as(grad_p)].any(), "no gradient on a PAD tail"


def test_k42_special_cases_of_the_cpu_file_and_capture():
    from case_rg_amd import ops
    from case_rg_amd.evaluation import sequence_risk_host
    p = torch.tensor([[[0.5], [0.25]]], device=DEV)
    one = torch.ones(1, 2, 1, dtype=torch.bool, device=DEV)
    cost = torch.tensor([[0.0, 1.0]], device=DEV)
    leaf = p.clone().requires_grad_(True)
    risk, q = ops.sequence_risk(leaf, one, cost, None, 1.0, want_q=True)
    risk.sum().backward()
    assert abs(float(risk.detach()[0]) - 1 / 3) <= 2.0 ** -24 / 3 + 1e-12
    assert torch.allclose(q.cpu(), torch.tensor([[2 / 3, 1 / 3]]), rtol=2.0 ** -23, atol=0)
    assert torch.allclose(leaf.grad.cpu(), torch.tensor([[[-4 / 9], [8 / 9]]]), rtol=2.0 ** -23, atol=0)
    # the special inputs of tests/test_mrt_cpu.py
    p = torch.full((3, 3, 4), 0.5)
    p[0, 1] = 0.25
    p[2, 0, 1] = 1e-35
    scored = torch.ones(3, 3, 4, dtype=torch.bool)
    scored[0, :, 2:] = False
    cost = torch.tensor([[0.0, 1.0, 0.5], [0.2, 0.4, 0.6], [1.0, 0.0, 0.5]])
    valid = torch.tensor([[True, True, False], [False, False, False], [True, True, True]])
    p, scored, cost, valid = p.to(DEV), scored.to(DEV), cost.to(DEV), valid.to(DEV)
    want = sequence_risk_host(p, scored, cost, valid, 1.0, rounded=False)
    static = p.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.sequence_risk(static, scored, cost, valid, 1.0)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            risk, q = ops.sequence_risk(static, scored, cost, valid, 1.0, want_q=True)
            (grad,) = torch.autograd.grad(risk.sum(), static)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    for got, ref in ((risk, want["risk"]), (q, want["q"]), (grad, want["grad_p"])):
        assert float(((got.double() - ref).abs() - (2.0 ** -24 * ref.abs() + 1e-12)).max()) <= 0.0
    assert float(risk[1]) == 0.0 and not grad[1].any() and not grad[0, 2].any() and float(grad[2, 0, 1]) == 0.0


# ---------------------------------------------------------------------------------------------
# 4. the models
# ---------------------------------------------------------------------------------------------
VOCAB = 300


def _model(kind, seed=40):
    from case_rg_amd.CaSE.Model import CaSE
    from case_rg_amd.Masque.Model import Masque
    from case_rg_amd.utils import fill_params, make_vocab
    v2i, i2v = make_vocab(VOCAB)
    m = CaSE(4, 8, i2v, v2i, 64) if kind == "case" else Masque(8, i2v, v2i, 64)
    return fill_params(m, seed).to(DEV)


def _batch(kind, seed=500, B=2):
    from case_rg_amd.utils import synth_batch
    return {k: v.to(DEV) for k, v in synth_batch(B, 3, 24, 12, 8, VOCAB, seed=seed, ragged=True, model=kind).items()}


def _pool(batch, seed=9):
    """Explicit candidates [B, 4, T]: two random answers, a copy of the first (a duplicate) and the reference itself cut by one token."""
    g = torch.Generator().manual_seed(seed)
    B, T = batch["response"].shape
    a = torch.randint(104, VOCAB, (B, 2, T), generator=g)
    a[:, 0, T // 2] = 2  # EOS, then a PAD tail
    a[:, 0, T // 2 + 1:] = 0
    a[:, 1, T - 1] = 2
    cut = batch["response"].cpu().clone()
    cut[:, 1] = 2
    cut[:, 2:] = 0
    return torch.cat([a, a[:, :1], cut.unsqueeze(1)], dim=1).to(DEV)


@pytest.fixture
def fp32():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.float32)
    case_rg_amd.set_dropout(True)  # (on: an MRT step must switch it off by itself)
    case_rg_amd.config.manual_seed(77)
    yield
    case_rg_amd.set_dropout(False)
    case_rg_amd.set_compute_dtype(torch.float32)


def _grads(model, losses):
    model.zero_grad()
    sum(l.mean() for l in losses).backward()
    torch.cuda.synchronize()
    out = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad()
    return out


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_do_mrt_on_an_explicit_pool(fp32, kind):
    from case_rg_amd import evaluation, ops
    from case_rg_amd.evaluation.rouge_ids import model_specials
    m, b = _model(kind).train(), _batch(kind)
    cands = _pool(b)
    with Calls() as c:
        out = m.do_mrt(dict(b), candidates=cands, details=True)
    assert m.training, "the previous mode is restored"
    assert c.count("case_pointer_head_score_stats") > 0 and c.count("case_pointer_head_score") == 0 and c.count("case_sequence_risk") == 1
    assert c.count("case_pointer_head_sample") == 0 and c.count("case_copy_scatter_sorted_fwd") == 0, c.calls
    assert set(out) == {"losses", "risk", "q", "cost", "valid", "candidates", "token_probs"}
    B, T = b["response"].shape
    pool = out["candidates"]
    assert pool.shape == (B, 5, T) and torch.equal(pool[:, :4], cands) and torch.equal(pool[:, 4], b["response"])
    train_losses = m.do_train(dict(b))
    assert [l.shape for l in out["losses"]] == [l.shape for l in train_losses] and out["losses"][-1].shape == (1,)
    # 1. the scores are do_score's
    m.eval()
    with torch.no_grad():
        scored = m.do_score(dict(b), pool)
    m.train()
    assert _same_bits(out["token_probs"], scored["token_probs"]), "token_probs: %.3e" % float(
        (out["token_probs"] - scored["token_probs"]).abs().max())
    # 2. cost, validity, risk and posterior
    specials = model_specials(m.vocab2id)
    f = evaluation.rouge_l_ids(pool, b["response"], specials)["f"][:, :, 0]
    assert _same_bits(out["cost"], 1.0 - f)
    assert float(out["cost"][:, 4].abs().max()) <= 1e-6, "the reference costs nothing"
    assert out["valid"].tolist() == [[True, True, False, True, True]] * B, "the copy of candidate 0 is left out"
    host = evaluation.sequence_risk_host(out["token_probs"].detach(), pool.ne(0), out["cost"], out["valid"], m.mrt["alpha"], rounded=False)
    for key in ("risk", "q"):
        assert float(((out[key].detach().double() - host[key]).abs() - (2.0 ** -24 * host[key].abs() + 1e-12)).max()) <= 0.0, key
    assert _same_bits(out["losses"][-1], out["risk"].mean().reshape(1))
    # 3. every parameter do_train reaches gets a finite gradient
    g_train, g_mrt = _grads(m, train_losses), _grads(m, out["losses"])
    assert set(g_train) <= set(g_mrt) and all(torch.isfinite(g).all() for g in g_mrt.values())
    assert any(float(g.abs().max()) > 0 for n, g in g_mrt.items() if ".decoder.gen." in n)
    # mle_weight adds do_score's loss of the reference row
    with_mle = m.do_mrt(dict(b), candidates=cands, mle_weight=0.5, details=True)
    on = pool[:, 4].ne(0)
    nll = (-torch.log(with_mle["token_probs"][:, 4] + 1e-8) * on).sum() / on.sum()
    assert torch.allclose(with_mle["losses"][-1], with_mle["risk"].mean() + 0.5 * nll, rtol=1e-6, atol=0)
    # without the reference and without dedup
    bare = m.do_mrt(dict(b), candidates=cands, with_reference=False, dedup=False, details=True)
    assert bare["candidates"].shape == (B, 4, T) and bool(bare["valid"].all())
    assert isinstance(m(dict(b, response=b["response"]), method="mrt_train"), list)


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_fused_head_gradients_agree_with_the_unfused_chain(fp32, kind):
    """The same step with K29 + K41 and with the unfused differentiable chain (POINTER_SCORE = "off"): token_probs, the loss and every
    parameter gradient, max |difference| / max |unfused| per tensor, are held to STEP_BAR, the constant above; the measured figures go to
    profiles/mrt_parity.json next to it."""
    from case_rg_amd import ops
    m, b = _model(kind).train(), _batch(kind)
    cands = _pool(b)
    with Calls() as c:
        fused = m.do_mrt(dict(b), candidates=cands, mle_weight=0.25, details=True)
    g_fused = _grads(m, fused["losses"])
    with _Unfused(), Calls() as u:
        assert not ops.pointer_score_grad_supported(ops.SortedSource(b["source_map"], VOCAB), 2)
        plain = m.do_mrt(dict(b), candidates=cands, mle_weight=0.25, details=True)
    g_plain = _grads(m, plain["losses"])
    assert c.count("case_pointer_head_score_bwd") == 0 and u.count("case_pointer_head_score_stats") == 0
    assert u.count("case_copy_scatter_sorted_fwd") > 0
    assert set(g_fused) == set(g_plain)
    e_p = scaled_error("token_probs", fused["token_probs"].detach().cpu().numpy(), plain["token_probs"].detach().cpu().numpy())
    e_l = scaled_error("loss", fused["losses"][-1].detach().cpu().numpy(), plain["losses"][-1].detach().cpu().numpy())
    worst = max(scaled_error(n, g_fused[n].cpu().numpy(), g_plain[n].cpu().numpy()) for n in g_plain if float(g_plain[n].abs().max()) > 0)
    print("%s: token_probs %.3e, loss %.3e, worst parameter gradient %.3e" % (kind, e_p, e_l, worst))
    for key, val in (("token_probs", e_p), ("loss", e_l), ("param_grads", worst)):
        _measured("do_mrt/%s/fused_vs_unfused/%s" % (kind, key), val, STEP_BAR)
    assert e_p <= STEP_BAR and e_l <= STEP_BAR and worst <= STEP_BAR, (e_p, e_l, worst)


def test_k41_runs_in_the_backward_pass(fp32):
    m, b = _model("case").train(), _batch("case")
    out = m.do_mrt(dict(b), candidates=_pool(b))
    with Calls() as c:
        sum(l.mean() for l in out).backward()
    torch.cuda.synchronize()
    assert c.count("case_pointer_head_score_bwd") > 0 and c.count("case_copy_scatter_bwd") == 0, c.calls
    m.zero_grad()


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_bf16_step_is_finite(fp32, kind):
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.bfloat16)
    m, b = _model(kind).train(), _batch(kind)
    losses = m.do_mrt(dict(b), candidates=_pool(b), mle_weight=0.1)
    assert all(torch.isfinite(l).all() for l in losses)
    grads = _grads(m, losses)
    assert grads and all(torch.isfinite(g).all() for g in grads.values())


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_sampled_pool_and_the_mode_switch(fp32, kind):
    m, b = _model(kind), _batch(kind)
    B, N, T = b["query"].shape[0], 3, m.max_target_length
    uniforms = torch.rand(T, B * N, generator=torch.Generator().manual_seed(3)).to(DEV)
    for training in (True, False):
        m.train(training)
        with Calls() as c:
            one = m.do_mrt(dict(b), num_samples=N, uniforms=uniforms, top_k=20, details=True)
        assert c.count("case_pointer_head_sample") + c.count("case_pointer_head_sample_wide") > 0, "the pool is drawn"
        two = m.do_mrt(dict(b), num_samples=N, uniforms=uniforms, top_k=20, details=True)
        assert m.training == training, "the training flag is restored"
        assert one["candidates"].shape[:2] == (B, N + 1) and torch.equal(one["candidates"], two["candidates"])
        assert all(_same_bits(x, y) for x, y in zip(one["losses"], two["losses"])), "fixed uniforms: equal losses"
        assert all(torch.isfinite(l).all() for l in one["losses"]) and one["losses"][-1].requires_grad
        broken = dict(b)
        del broken["source_map"]
        with pytest.raises(KeyError):
            m.do_mrt(broken, num_samples=N)
        assert m.training == training, "... also after an exception raised inside the call"
    m.train()
    m.passage_selection.scorer.eval()  # a submodule held in eval inside a model in train mode keeps its own flag
    free = m.do_mrt(dict(b), num_samples=2)  # the global counter stream
    assert all(torch.isfinite(l).all() for l in free)
    assert m.training and m.response_generation.decoder.training and not m.passage_selection.scorer.training


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_do_score_is_untouched(fp32, kind):
    """``do_score`` under grad still takes the unfused chain (no K29 launch of either kind), and a ``do_mrt`` call in between changes none of
    its bits."""
    m, b = _model(kind).eval(), _batch(kind)
    cands = _pool(b)

    def score():
        m.zero_grad()
        with Calls() as c:
            out = m.do_score(dict(b), cands)
        assert c.scored == 0 and c.count("case_pointer_head_score_stats") == 0 and out["loss"].requires_grad
        with torch.no_grad(), Calls() as c:
            quick = m.do_score(dict(b), cands)
        assert c.scored > 0 and c.count("case_pointer_head_score_stats") == 0
        return [out[k].detach() for k in ("token_probs", "copy_probs", "scores", "loss")] + [quick[k] for k in ("token_probs", "copy_probs", "loss")]

    before = score()
    m.do_mrt(dict(b), candidates=cands)
    assert not m.training
    after = score()
    assert all(_same_bits(x, y) for x, y in zip(before, after))


def test_capturing_trainer_runs_mrt_batches_eagerly(fp32):
    import case_rg_amd
    from case_rg_amd.common.CumulativeTrainer import CumulativeTrainer
    from case_rg_amd.optim import FusedAdam
    m = _model("case").train()
    trainer = CumulativeTrainer(m, None, None, 0, 1, capture=True)
    try:
        opt = FusedAdam(m.parameters(), lr=1e-3)
        m.mrt["num_samples"] = 2
        batch = _batch("case", seed=501)
        batch = {k: v for k, v in batch.items()}
        losses = [trainer.train_batch(0, dict(batch), "mrt_train", opt) for _ in range(4)]
        assert trainer.graphs is not None and not trainer.graphs.graphs and trainer.graphs.replays == 0
        assert not any(sig[0] == "mrt_train" for sig in list(trainer.graphs.graphs) + list(trainer.graphs.seen))
        assert len(losses[0]) == 3 and all(np.isfinite(l).all() for l in losses)
        assert m.training
    finally:
        case_rg_amd.config.set_device_state(None)
