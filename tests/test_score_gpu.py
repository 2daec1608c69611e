"""Teacher-forced answer scoring on the MI355X: the product's ``do_score`` against the fixtures of the reference's own training branch
(tests/golden/score_*.npz, pinned to the CPU oracle by tests/test_score_cpu.py) and against the recorded generation losses of the existing
train fixtures; K29 (``case_pointer_head_score``) against a float64 restatement and against K23's row; the cached decoding step against
the full-prefix pass (``do_sample`` / ``do_beam`` rescored); chunking, several candidates per item, gradients, graph capture, the
trainer's ``evaluate_nll`` and the argument checks.

Measured maxima go to profiles/score_parity.json."""
import json
import math
import os

import numpy as np
import pytest
import torch

import cases
import sample_cases
import score_cases
from helpers import FP32_BAR, Calls, load_golden, record_error, scaled_error, special_ids, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _measured(key, value, bar=None):
    """Add one measured maximum to profiles/score_parity.json."""
    path = os.path.join(ROOT, "profiles", "score_parity.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = {}
    if os.path.exists(path):
        with open(path) as fh:
            data = json.load(fh)
    data[key] = {"measured": float("%.3e" % value), "bar": bar}
    with open(path, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)


def _rel(got, want, floor=0.0):
    """max |got - want| / |want| over the entries with |want| >= floor (element-wise relative error)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    keep = np.abs(want) >= max(floor, 1e-300)
    return float((np.abs(got - want)[keep] / np.abs(want)[keep]).max()) if keep.any() else 0.0


@pytest.fixture(scope="module")
def ns():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.float32)
    case_rg_amd.set_dropout(False)
    return case_rg_amd.namespace()


class _Unfused:
    """CASE_POINTER_SCORE=off for the block."""

    def __enter__(self):
        from case_rg_amd import ops
        self.old, ops.POINTER_SCORE = ops.POINTER_SCORE, "off"

    def __exit__(self, *exc):
        from case_rg_amd import ops
        ops.POINTER_SCORE = self.old


@pytest.fixture(scope="module")
def fixture_models(ns):
    """name -> (golden, model in eval mode, batch, candidates on the device), built once for the module and left unchanged."""
    out = {}
    for name, (kind, _, _, cseed) in score_cases.SCORE_CASES.items():
        golden = load_golden(name)
        m, b = score_cases.build(ns, torch.device("cuda"), name)
        for key in ("query", "passage", "source_map", "response"):
            assert np.array_equal(to_np(b[key]), golden["in_" + key]), key
        cands = score_cases.candidates(b, int(golden["eos"]), cseed)
        assert np.array_equal(cands.numpy(), golden["answers"])
        out[name] = (golden, m.eval(), b, cands.cuda())
    return out


# ---------------------------------------------------------------------------------------------
# 1. the product against the reference's teacher-forced training branch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ["fused", "unfused"])
@pytest.mark.parametrize("name", list(score_cases.SCORE_CASES))
def test_fp32_scores_match_the_reference(fixture_models, name, head):
    golden, m, b, cands = fixture_models[name]
    with torch.no_grad(), Calls() as c:
        if head == "unfused":
            with _Unfused():
                out = m.do_score(dict(b), cands)
        else:
            out = m.do_score(dict(b), cands)
    assert (c.scored > 0) == (head == "fused"), "K29 must run in the fused pass and only there: %s" % c.calls
    assert set(out) == {"rank", "token_probs", "copy_probs", "scores", "loss", "tokens"}
    B, N, T = golden["answers"].shape
    assert out["token_probs"].shape == (B, N, T) and out["copy_probs"].shape == (B, N, T) and out["scores"].shape == (B, N)
    assert out["loss"].shape == (1,) and out["tokens"].dtype == torch.int64 and out["tokens"].dim() == 0
    scored = golden["answers"] != int(golden["pad"])
    p, cp = to_np(out["token_probs"]).astype(np.float64), to_np(out["copy_probs"]).astype(np.float64)
    assert (p[~scored] == 1.0).all() and (cp[~scored] == 0.0).all(), "PAD targets: probability 1, copy part 0"
    assert int(out["tokens"]) == int(golden["tokens"]) == int(scored.sum())
    assert (golden["p"][scored] >= score_cases.P_MIN).all()
    worst = {"token_probs": _rel(p[scored], golden["p"][scored])}
    if "ptr" in golden:
        absent = scored & (golden["occurs"] == 0)
        assert (cp[absent] == 0.0).all(), "a target that is absent from the source has a copy part of exactly 0"
        has = scored & (golden["ptr"] > 0)
        worst["copy_probs"] = _rel(cp[has], golden["ptr"][has])
    else:  # the reference's Masque returns the summed distribution only: p = p0 gen[y] + copy with p0 <= 1 bounds the copy part
        assert (cp[scored] <= p[scored] * (1 + 1e-6)).all() and (cp[scored] >= (p - golden["gen"])[scored] - FP32_BAR * p[scored]).all()
        assert (cp[scored & (golden["occurs"] == 0)] == 0.0).all()
    worst["scores"] = _rel(to_np(out["scores"]), golden["scores"])
    worst["loss"] = _rel(to_np(out["loss"]), [float(golden["loss"])])
    for key, rel in worst.items():
        print("%s [%s] %s: %.3e" % (name, head, key, rel))
        record_error(name, "fp32_" + head, key, rel, FP32_BAR)
        _measured("%s/%s/%s" % (name, head, key), rel, FP32_BAR)
    assert all(rel <= FP32_BAR for rel in worst.values()), worst
    if head == "fused":  # method="score" scores the batch's own response: candidate 0 of every item
        with torch.no_grad():
            own = m(dict(b), method="score")
        T0 = b["response"].shape[1]
        assert own["token_probs"].shape == (B, 1, T0)
        assert _rel(to_np(own["token_probs"][:, 0]), p[:, 0, :T0]) <= FP32_BAR
        assert torch.equal(own["rank"], out["rank"])


# ---------------------------------------------------------------------------------------------
# 2. the existing train fixtures: do_score's loss is do_train's generation loss with dropout off
# ---------------------------------------------------------------------------------------------
TRAIN_FIXTURES = {"case_train": ("case", 141, 142, False), "masque_train": ("masque", 161, 162, False),
                  "prod_case_train": ("case", 211, 212, True), "prod_masque_train": ("masque", 221, 222, True)}


def _train_fixture(ns, name):
    kind, mseed, bseed, prod = TRAIN_FIXTURES[name]
    dev = torch.device("cuda")
    if prod:
        return cases._prod_model(ns, dev, mseed, kind).eval(), cases._prod_batch(dev, bseed, kind)
    return (cases._case_model if kind == "case" else cases._masque_model)(ns, dev, mseed).eval(), cases._batch(dev, bseed, kind)


@pytest.mark.parametrize("name,mode", [(n, "fp32") for n in TRAIN_FIXTURES] + [(n, "bf16_auto") for n in TRAIN_FIXTURES if TRAIN_FIXTURES[n][3]])
def test_loss_equals_the_recorded_generation_loss(name, mode):
    """fp32 at the project's bar; the production-geometry fixtures also in the timed bf16 mode, under the bar tests/test_parity_prod_gpu.py
    applies to the same loss in that mode (the toy fixtures are not replayed in bf16 anywhere)."""
    import case_rg_amd
    from test_parity_prod_gpu import BF16_BARS, _Mode
    bar = FP32_BAR if mode == "fp32" else BF16_BARS[name][0]
    golden = load_golden(name)
    with _Mode(mode) as c:
        m, b = _train_fixture(case_rg_amd.namespace(), name)
        assert np.array_equal(to_np(b["response"]), golden["in_response"])
        with torch.no_grad():
            out = m.do_score(dict(b))
        torch.cuda.synchronize()
    assert c.calls.get("case_pointer_head_score", 0) > 0
    rel = scaled_error(name + "/loss", to_np(out["loss"]), golden["loss_rg"])
    print("%s [%s] loss %.6f, recorded %.6f: %.3e (bar %.0e)" % (name, mode, float(out["loss"][0]), float(golden["loss_rg"][0]), rel, bar))
    record_error(name, mode, "score_loss", rel, bar)
    _measured("%s/%s/loss" % (name, mode), rel, bar)
    assert int(out["tokens"]) == int((golden["in_response"] != 0).sum())
    assert rel <= bar


# ---------------------------------------------------------------------------------------------
# 3. / 4. K29 alone
# ---------------------------------------------------------------------------------------------
def _k29_inputs(R, rps, V, S, nmem, seed):
    """Synthetic head inputs with planted targets.  Ordinary source tokens lie in [5, V // 2); the planted ones above that:
    ``once`` occurs once per source row, ``many`` in a run of min(S // 2, 90) entries that lies on both sides of the boundary between the
    memories, ``absent`` nowhere; id 0 occurs twice and id V - 1 once."""
    from case_rg_amd import ops
    g = torch.Generator().manual_seed(seed)
    K = R // rps
    lens = [S] if nmem == 1 else [S // 4, S - S // 4]
    src = torch.randint(5, V // 2, (K, S), generator=g)
    once, many, absent, common = V // 2 + 1, V // 2 + 2, V // 2 + 3, V // 2 + 4
    run = min(S // 2, 90)
    start = lens[0] - run // 2 if nmem == 2 else 3
    src[:, start:start + run] = many
    src[:, 0] = once
    src[:, 1], src[:, S - 1] = 0, 0
    src[:, 2] = V - 1
    src[:, S - 2] = common
    logits = torch.randn(R, V, generator=g) * 2.0
    mix = torch.randn(R, 1 + nmem, generator=g)
    copies = [torch.softmax(torch.randn(R, n, generator=g) * 2.0, dim=-1) for n in lens]
    special = [once, many, absent, 0, V - 1, V, -3, common]
    dev = torch.device("cuda")
    return (logits.to(dev), mix.to(dev), ops.SortedSource(src.to(dev), V), [c.to(dev) for c in copies], src, lens, special,
            dict(once=1, many=int((src[0] == many).sum())))


def _k29_restated(logits, mix, src, rps, copies, targets, pad):
    """float64 restatement of the rule in include/case_hip.h."""
    lg, mx = to_np(logits).astype(np.float64), to_np(mix).astype(np.float64)
    cs = np.concatenate([to_np(c).astype(np.float64) for c in copies], axis=1)
    bounds = np.cumsum([0] + [c.shape[1] for c in copies])
    src = src.numpy()
    R, V = lg.shape
    prob, ptr = np.zeros(R), np.zeros(R)
    for r in range(R):
        y = int(targets[r])
        if pad >= 0 and y == pad:
            prob[r] = 1.0
            continue
        if y < 0 or y >= V:
            continue
        e = np.exp(lg[r] - lg[r].max())
        pm = np.exp(mx[r] - mx[r].max())
        pm /= pm.sum()
        hit = src[r // rps] == y
        for k in range(len(copies)):
            sl = slice(bounds[k], bounds[k + 1])
            ptr[r] += pm[k + 1] * cs[r, sl][hit[sl]].sum()
        prob[r] = pm[0] * e[y] / e.sum() + ptr[r]
    return prob, ptr


@pytest.mark.parametrize("R,rps", [(3, 1), (8, 1), (8, 2)])
@pytest.mark.parametrize("V", [200, 1031, 30522, 40000])
def test_kernel_matches_the_float64_restatement(V, R, rps):
    """V 1031 leaves rows 4-byte aligned, 30 522 8-byte aligned, 40 000 is beyond what the LDS-row kernels (K23 / K24 / K28) hold; S 1100
    carries a run of 90 equal tokens (more than one wave stride), S 44 one of 22.  Every special target is scored with PAD = 0 and with
    pad = -1 (then id 0 is an ordinary token)."""
    from case_rg_amd import ops
    worst = 0.0
    for S in (44, 1100):
        for nmem in (1, 2):
            logits, mix, sm, copies, src, lens, special, runs = _k29_inputs(R, rps, V, S, nmem, 7 * R + S + nmem)
            assert runs["many"] >= 70 or S == 44
            if nmem == 2:  # the long run spans both memories
                many = special[1]
                assert (src[0, :lens[0]] == many).any() and (src[0, lens[0]:] == many).any()
            for first in range(0, len(special), R):
                ids = [special[(first + i) % len(special)] for i in range(R)]
                targets = torch.tensor(ids, dtype=torch.int64, device="cuda")
                for pad in (0, -1):
                    with Calls() as c:
                        prob, ptr = ops.pointer_head_score(logits, mix, sm, rps, copies, targets, pad=pad)
                        prob2, ptr2 = ops.pointer_head_score(logits, mix, sm, rps, copies, targets, pad=pad)
                    assert c.scored == 2
                    assert torch.equal(prob, prob2) and torch.equal(ptr, ptr2), "two launches differ"
                    want_p, want_c = _k29_restated(logits, mix, src, rps, copies, ids, pad)
                    got_p, got_c = to_np(prob).astype(np.float64), to_np(ptr).astype(np.float64)
                    for r, y in enumerate(ids):
                        if pad >= 0 and y == pad:
                            assert got_p[r] == 1.0 and got_c[r] == 0.0, "a PAD row is not scored"
                        elif y < 0 or y >= V:
                            assert got_p[r] == 0.0 and got_c[r] == 0.0, "an id outside the vocabulary has probability 0"
                        elif y == special[2]:
                            assert got_c[r] == 0.0 and got_p[r] > 0.0, "an absent token has a copy part of exactly 0"
                        else:
                            assert got_c[r] > 0.0
                    worst = max(worst, _rel(got_p, want_p, 1e-6), _rel(got_c, want_c, 1e-6))
    print("K29 vs float64 at V %d, R %d, rows_per_source %d: %.3e" % (V, R, rps, worst))
    record_error("k29_restated", "V%d_R%d_rps%d" % (V, R, rps), "prob_and_copy", worst, FP32_BAR)
    _measured("k29_vs_float64/V%d_R%d_rps%d" % (V, R, rps), worst, FP32_BAR)
    assert worst <= FP32_BAR


@pytest.mark.parametrize("V", [200, 1031, 30522])
def test_kernel_matches_the_greedy_heads_row(V):
    """On the same inputs K29's probability is the entry of K23's distribution row (same exponential, different summation order)."""
    from case_rg_amd import ops
    worst = 0.0
    for S, nmem in ((44, 2), (1100, 2), (1100, 1)):
        logits, mix, sm, copies, src, lens, special, _ = _k29_inputs(8, 1, V, S, nmem, 100 + S + nmem)
        _, dist, _ = ops.pointer_head_decode(logits, mix, sm, copies, want_gen=False, want_dist=True)
        ids = [y for y in special if 0 <= y < V]
        ids = (ids + ids)[:8]
        targets = torch.tensor(ids, dtype=torch.int64, device="cuda")
        prob, _ = ops.pointer_head_score(logits, mix, sm, 1, copies, targets, pad=-1)
        want = to_np(dist.gather(1, targets.unsqueeze(1)).squeeze(1))
        worst = max(worst, _rel(to_np(prob), want, 1e-6))
    print("K29 vs K23 at V %d: %.3e" % (V, worst))
    record_error("k29_vs_k23", "V%d" % V, "prob", worst, FP32_BAR)
    _measured("k29_vs_k23/V%d" % V, worst, FP32_BAR)
    assert worst <= FP32_BAR


# ---------------------------------------------------------------------------------------------
# 5. the cached decoding step against the full-prefix pass
# ---------------------------------------------------------------------------------------------
def _drawn_positions(samples, unk, pad):
    """Where ``sample_probs`` is the probability of the EMITTED token: K28 records the probability of the token it DREW, and the loop emits
    something else at t = 0 (UNK for a drawn EOS), at the last step (EOS is forced) and behind the end (PAD)."""
    keep = samples != pad
    keep[..., -1] = False
    keep[..., 0] &= samples[..., 0] != unk
    return keep


def _beam_costs(token_probs, answers, eos):
    """The cost rule restated in tests/test_beam_cpu.py: a hypothesis of n tokens (up to and including its EOS, or all T) costs
    sum_t -log(p_t + 1e-10) / (n + 1).  -> (cost [B, W], usable [B, W]: no PAD id inside the hypothesis)."""
    B, W, T = answers.shape
    cost, usable = np.zeros((B, W)), np.zeros((B, W), dtype=bool)
    for b in range(B):
        for w in range(W):
            ids = answers[b, w].tolist()
            n = ids.index(eos) + 1 if eos in ids else T
            usable[b, w] = 0 not in ids[:n]
            cost[b, w] = sum(-math.log(token_probs[b, w, t] + 1e-10) for t in range(n)) / (n + 1)
    return cost, usable


@pytest.mark.parametrize("name", ["sample_case", "sample_masque"])
def test_rescoring_reproduces_the_cached_steps_probabilities(ns, name):
    """Toy geometry, fp32: the probabilities the sampled pass recorded step by step (cached K / V, K22, K28) are the full-prefix pass's, and
    the costs of the beam search's finished hypotheses are the rescored ones."""
    m, b = sample_cases.build(ns, torch.device("cuda"), name)
    m.eval()
    _, eos, unk, pad = special_ids(m)
    with torch.no_grad():
        drawn = m.do_sample(dict(b), num_samples=3, seed=5)
        again = m.do_score(dict(b), drawn["samples"])
        beam = m.do_beam(dict(b))
        rescored = m.do_score(dict(b), beam["beam_answers"])
    samples, want = to_np(drawn["samples"]), to_np(drawn["sample_probs"]).astype(np.float64)
    keep = _drawn_positions(samples, unk, pad) & (want >= 1e-4)
    assert keep.sum() >= samples.size // 4, "too few comparable positions: %d" % keep.sum()
    got = to_np(again["token_probs"]).astype(np.float64)
    rel = _rel(got[keep], want[keep])
    print("%s: sampled pass vs rescoring over %d positions: %.3e" % (name, keep.sum(), rel))
    record_error(name, "fp32", "rescored_sample_probs", rel, FP32_BAR)
    _measured("%s/rescored_sample_probs" % name, rel, FP32_BAR)
    assert rel <= FP32_BAR
    scores = to_np(beam["beam_scores"]).astype(np.float64)
    cost, usable = _beam_costs(to_np(rescored["token_probs"]).astype(np.float64), to_np(beam["beam_answers"]), eos)
    fin = np.isfinite(scores) & usable
    assert fin.sum() >= scores.shape[0], "too few finished hypotheses to compare"
    rel_b = _rel(cost[fin], scores[fin])
    print("%s: beam costs vs rescoring over %d hypotheses: %.3e" % (name, fin.sum(), rel_b))
    record_error(name, "fp32", "rescored_beam_scores", rel_b, FP32_BAR)
    _measured("%s/rescored_beam_scores" % name, rel_b, FP32_BAR)
    assert rel_b <= FP32_BAR


def test_rescoring_production_rows_in_bf16():
    """V = 30 522, H = 512, 2 items x 3 samples x 14 steps in the timed bf16 mode: the gap between the cached step's recorded
    probabilities and the full-prefix pass's is MEASURED (ln p per position and the mean -ln p); the one requirement is that everything is
    finite and the mean -ln p over the comparable positions agrees within the bf16 bar of the generation loss."""
    import case_rg_amd
    from test_parity_prod_gpu import BF16_BARS, _Mode
    kind, dev = "case", torch.device("cuda")
    with _Mode("bf16_auto"):
        m = cases._prod_test_model(case_rg_amd.namespace(), dev, 311, kind, cases.PROD_TEST_GAIN[kind]).eval()
        b = cases._prod_test_batch(dev, 312, kind)
        _, eos, unk, pad = special_ids(m)
        with torch.no_grad():
            drawn = m.do_sample(dict(b), num_samples=3, seed=9)
            again = m.do_score(dict(b), drawn["samples"])
        torch.cuda.synchronize()
    samples = to_np(drawn["samples"])
    want, got = to_np(drawn["sample_probs"]).astype(np.float64), to_np(again["token_probs"]).astype(np.float64)
    assert np.isfinite(got).all() and np.isfinite(to_np(again["scores"])).all() and np.isfinite(to_np(again["loss"])).all()
    keep = _drawn_positions(samples, unk, pad)
    assert keep.sum() >= 6
    nll_want, nll_got = -np.log(want[keep] + 1e-8), -np.log(got[keep] + 1e-8)
    gap_ln = float(np.abs(nll_want - nll_got).max())
    rel = abs(nll_want.mean() - nll_got.mean()) / (abs(nll_want.mean()) + 1e-6)
    bar = BF16_BARS["prod_case_train"][0]
    print("production rows, bf16: %d positions, max |ln p gap| %.3e, mean -ln p %.5f (cached) / %.5f (full prefix): %.3e (bar %.0e)" % (
        keep.sum(), gap_ln, nll_want.mean(), nll_got.mean(), rel, bar))
    record_error("score_prod_bf16", "bf16_auto", "mean_nll_cached_vs_full_prefix", rel, bar)
    _measured("prod_bf16/max_abs_ln_p_gap", gap_ln, None)
    _measured("prod_bf16/mean_nll_cached_vs_full_prefix", rel, bar)
    assert rel <= bar


# ---------------------------------------------------------------------------------------------
# 6. / 7. chunking and several candidates per item
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(score_cases.SCORE_CASES))
def test_chunked_head_agrees_with_the_default(fixture_models, name):
    _, m, b, cands = fixture_models[name]
    dec = m.response_generation.decoder
    assert dec.score_chunk_rows == 2048
    with torch.no_grad(), Calls() as c:
        whole = m.do_score(dict(b), cands)
        n_whole = c.scored
        dec.score_chunk_rows = 5
        try:
            parts = m.do_score(dict(b), cands)
        finally:
            dec.score_chunk_rows = 2048
    B, N, T = cands.shape
    assert n_whole == 1 and c.scored - n_whole == B * math.ceil(N * T / 5), c.calls
    for key in ("token_probs", "copy_probs", "scores", "loss"):
        rel = _rel(to_np(parts[key]), to_np(whole[key]), 1e-6)
        _measured("%s/chunk5_vs_default/%s" % (name, key), rel, FP32_BAR)
        assert rel <= FP32_BAR, (key, rel)
    assert int(parts["tokens"]) == int(whole["tokens"])


@pytest.mark.parametrize("name", list(score_cases.SCORE_CASES))
def test_candidates_are_independent_rows(fixture_models, name):
    _, m, b, cands = fixture_models[name]
    with torch.no_grad():
        whole = m.do_score(dict(b), cands)
        singles = [m.do_score(dict(b), cands[:, n].contiguous()) for n in range(cands.shape[1])]
        three_d = m.do_score(dict(b), cands[:, 1:2].contiguous())
    for n, one in enumerate(singles):
        assert one["token_probs"].shape == (cands.shape[0], 1, cands.shape[2]) and one["scores"].shape == (cands.shape[0], 1)
        for key in ("token_probs", "copy_probs", "scores"):
            assert _rel(to_np(one[key][:, 0]), to_np(whole[key][:, n]), 1e-6) <= FP32_BAR, (key, n)
    for key in ("token_probs", "copy_probs", "scores", "loss", "tokens"):
        assert torch.equal(three_d[key], singles[1][key]), "a 2-D answers tensor is the same data as [B, 1, T]: %s" % key
    tokens = sum(int(s["tokens"]) for s in singles)
    merged = sum(float(s["loss"]) * int(s["tokens"]) for s in singles) / tokens
    assert tokens == int(whole["tokens"]) and abs(merged - float(whole["loss"])) <= FP32_BAR * abs(merged)


# ---------------------------------------------------------------------------------------------
# 8. gradients
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(score_cases.SCORE_CASES))
def test_differentiable_pass_reaches_the_parameters(ns, name):
    golden = load_golden(name)
    m, b = score_cases.build(ns, torch.device("cuda"), name)
    m.eval()
    cands = torch.from_numpy(golden["answers"]).cuda()
    with torch.no_grad():
        fused = m.do_score(dict(b), cands)
    m.zero_grad()
    with Calls() as c:
        out = m.do_score(dict(b), cands)
    assert c.scored == 0 and out["loss"].requires_grad
    out["loss"].sum().backward()
    torch.cuda.synchronize()
    grads = {n: p.grad for n, p in m.response_generation.decoder.named_parameters() if p.grad is not None}
    for prefix in ("gen.", "mix.", "attns."):
        hit = [g for n, g in grads.items() if n.startswith(prefix)]
        assert hit and all(torch.isfinite(g).all() for g in hit) and any(float(g.abs().max()) > 0 for g in hit), prefix
    rel = _rel(to_np(out["loss"]), to_np(fused["loss"]))
    _measured("%s/grad_path_loss_vs_fused" % name, rel, FP32_BAR)
    assert rel <= FP32_BAR
    assert _rel(to_np(out["token_probs"]), to_np(fused["token_probs"]), 1e-6) <= FP32_BAR
    m.zero_grad()


# ---------------------------------------------------------------------------------------------
# 9. graph capture
# ---------------------------------------------------------------------------------------------
def test_scoring_pass_replays_from_a_captured_graph(fixture_models):
    _, m, b, cands = fixture_models["score_case"]
    keys = ("token_probs", "copy_probs", "scores", "loss", "tokens", "rank")
    with torch.no_grad():
        eager = {k: v.clone() for k, v in m.do_score(dict(b), cands).items()}
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.do_score(dict(b), cands)  # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        graph, static = torch.cuda.CUDAGraph(), {}
        with torch.cuda.graph(graph), Calls() as c:
            static.update(m.do_score(dict(b), cands))
        assert c.scored == 1
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            for k in keys:
                assert torch.equal(static[k], eager[k]), "the replay differs from the eager pass in %s" % k
        del graph


# ---------------------------------------------------------------------------------------------
# 10. the trainer's corpus NLL
# ---------------------------------------------------------------------------------------------
def test_trainer_evaluate_nll_is_the_token_weighted_merge(ns):
    from case_rg_amd.utils import synth_batch
    m = cases._case_model(ns, torch.device("cuda"), 201)
    data = synth_batch(5, 3, 12, 8, 6, cases.V, seed=203, model="case")
    trainer = ns.CumulativeTrainer(m, None, None, None, 1)
    trainer.model.train()
    got = trainer.evaluate_nll(cases._ListDataset(data), cases._collate, 3)  # batches of 3 and 2 items
    assert trainer.model.training, "the mode must be restored"
    trainer.model.eval()
    total, tokens = 0.0, 0
    with torch.no_grad():
        for lo, hi in ((0, 3), (3, 5)):
            out = trainer.model.do_score({k: v[lo:hi].cuda() for k, v in data.items()})
            total, tokens = total + float(out["loss"]) * int(out["tokens"]), tokens + int(out["tokens"])
    trainer.close()
    assert set(got) == {"nll", "perplexity", "tokens"} and got["tokens"] == tokens == int((data["response"] != 0).sum())
    assert abs(got["nll"] - total / tokens) <= 1e-5 * abs(total / tokens)
    assert abs(got["perplexity"] - math.exp(got["nll"])) <= 1e-9 * got["perplexity"]


# ---------------------------------------------------------------------------------------------
# 11. errors
# ---------------------------------------------------------------------------------------------
def test_argument_checks(fixture_models):
    _, m, b, cands = fixture_models["score_masque"]
    m.train()
    try:
        with pytest.raises(ValueError, match="eval mode"):
            m.do_score(dict(b), cands)
        with pytest.raises(ValueError, match="eval mode"):
            m(dict(b), method="score")
    finally:
        m.eval()
    max_len = m.response_generation.decoder.embedding[1].pe.size(0)
    too_long = torch.ones(cands.shape[0], 1, max_len + 1, dtype=torch.int64, device="cuda")
    with torch.no_grad(), pytest.raises(RuntimeError, match="exceeds max_len %d" % max_len):
        m.do_score(dict(b), too_long)
    with torch.no_grad():  # T' beyond max_target_length is fine: it is bounded by the position table alone
        longer = torch.cat([cands, cands], dim=-1)
        assert longer.shape[-1] > m.max_target_length
        out = m.do_score(dict(b), longer)
    assert out["token_probs"].shape == tuple(longer.shape) and torch.isfinite(out["loss"]).all()
