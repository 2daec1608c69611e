"""Beam search on the MI355X: the product's ``do_beam`` against the fixtures of the reference's own ``Generations.beam``, W = 1 against
greedy decoding, the four beam kernels (K24 - K27) against restatements, production geometry in bf16, and stream capture.

The Python restatement of the selection rule is the one tests/test_beam_cpu.py pins to the reference."""
import math

import numpy as np
import pytest
import torch

import beam_cases
import cases
from helpers import Calls, head_inputs, load_golden, record_error, scaled_error, to_np
from test_beam_cpu import INF, advance, backtrack, beam_search, cut_at_eos, pack, pool_insert, rel_gap

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ns():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.float32)
    case_rg_amd.set_dropout(False)
    return case_rg_amd.namespace()


# ---------------------------------------------------------------------------------------------
# 1. the product against the reference's beam
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", beam_cases.WIDTHS)
@pytest.mark.parametrize("name", list(beam_cases.BEAM_CASES))
def test_fp32_beam_matches_the_reference_beam(ns, name, width):
    golden = load_golden("%s_w%d" % (name, width))
    m, b = beam_cases.build(ns, torch.device("cuda"), name)
    for k in ("query", "passage", "source_map"):
        assert np.array_equal(to_np(b[k]), golden["in_" + k]), k
    m.eval()
    m.beam_width = width
    with torch.no_grad(), Calls() as c:
        out = m(dict(b), method="beam")
        again = m.do_beam(dict(b), width=width)
    assert c.calls.get("case_pointer_head_beam", 0) >= 2 and c.calls.get("case_beam_advance", 0) >= 2, "the beam kernels did not run: %s" % c.calls
    assert set(out) == {"answer", "rank", "beam_score", "beam_answers", "beam_scores"}
    T = beam_cases.T
    assert out["answer"].shape == (beam_cases.ITEMS, T) and out["beam_answers"].shape == (beam_cases.ITEMS, width, T)
    assert out["beam_scores"].shape == (beam_cases.ITEMS, width) and out["beam_score"].shape == (beam_cases.ITEMS,)
    for k in ("answer", "beam_answers", "beam_scores"):
        assert torch.equal(out[k], again[k]), "%s differs between two passes" % k
    assert torch.equal(out["answer"], out["beam_answers"][:, 0]) and torch.equal(out["beam_score"], out["beam_scores"][:, 0])
    got, score = to_np(out["answer"]), to_np(out["beam_score"])
    decisive = golden["gap"] > beam_cases.GAP
    assert decisive.sum() * 2 >= decisive.size
    for i in np.nonzero(decisive)[0]:
        assert np.array_equal(got[i], golden["answer"][i]), "%s w%d item %d: %s != reference %s (gap %.3g)" % (
            name, width, i, got[i], golden["answer"][i], golden["gap"][i])
    rel = scaled_error("%s_w%d/score" % (name, width), score[decisive], golden["score"][decisive])
    record_error("%s_w%d" % (name, width), "fp32", "score", rel, 1e-3)
    assert rel <= 1e-3, "normalised costs: %.2e of their scale" % rel
    # the other retired hypotheses of a decisive item: same costs as the restatement found on the reference, and the same ids wherever
    # an entry's place in the pool is decisive too -- its cost is more than GAP away from both neighbours'.  The last entry of a full
    # pool is left out: the fixture does not record how close the best hypothesis that fell off the pool came to it.
    compared = 0
    for i in np.nonzero(decisive)[0]:
        want_s = golden["beam_scores"][i]
        fin = np.isfinite(want_s)
        assert np.array_equal(np.isfinite(to_np(out["beam_scores"])[i]), fin)
        np.testing.assert_allclose(to_np(out["beam_scores"])[i][fin], want_s[fin], rtol=1e-3)
        n = int(fin.sum())
        for k in range(1, n):
            if k == width - 1 or rel_gap(want_s[k], want_s[k - 1]) <= beam_cases.GAP or (k + 1 < n and rel_gap(want_s[k], want_s[k + 1]) <= beam_cases.GAP):
                continue
            compared += 1
            assert np.array_equal(to_np(out["beam_answers"])[i, k], golden["beam_answers"][i, k]), "%s w%d item %d entry %d: %s != reference %s" % (
                name, width, i, k, to_np(out["beam_answers"])[i, k], golden["beam_answers"][i, k])
    assert compared >= 1, "no pool entry behind the best one was compared"


# ---------------------------------------------------------------------------------------------
# 2. W = 1 is greedy decoding
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", list(beam_cases.BEAM_CASES))
def test_width_one_equals_greedy(ns, name, dtype):
    """K24 at W = 1 returns K23's id and value bit for bit and the rows are the greedy rows, so the ids are equal -- up to and including the
    first EOS, where the beam hypothesis retires and greedy decoding (without early stop) goes on."""
    import case_rg_amd
    from case_rg_amd.common.Constants import EOS_WORD
    case_rg_amd.set_compute_dtype(dtype)
    try:
        m, b = beam_cases.build(ns, torch.device("cuda"), name)
        m.eval()
        eos = m.vocab2id[EOS_WORD]
        with torch.no_grad(), Calls() as c:
            greedy = to_np(m(dict(b), method="test")["answer"])
            out = m.do_beam(dict(b), width=1)
        assert c.calls.get("case_pointer_head_decode", 0) >= beam_cases.T and c.calls.get("case_pointer_head_beam", 0) >= 1, "not the fused heads"
        beam = to_np(out["answer"])
        for i in range(beam.shape[0]):
            want = cut_at_eos(greedy[i], eos)
            assert beam[i, :len(want)].tolist() == want and not beam[i, len(want):].any(), "item %d: beam %s, greedy %s" % (i, beam[i], greedy[i])
        assert np.isfinite(to_np(out["beam_score"])).all()
    finally:
        case_rg_amd.set_compute_dtype(torch.float32)


# ---------------------------------------------------------------------------------------------
# 3. kernel units
# ---------------------------------------------------------------------------------------------
def _head_inputs(R, V, lens, seed):
    """Logits with designed rows: row 0 plain; row 1 has exact ties among its largest logits (tokens the sources do not hold); row 2's
    pointer mass lands on its most probable tokens; row 3 is dominated by copied tokens the generator gives almost nothing."""
    S, free = sum(lens), []

    def design(logits, src, mix):
        order = logits.argsort(dim=1, descending=True)
        free.extend([int(t) for t in order[1].tolist() if t < 1000][:6])  # ids below 1000 are never in ``src``
        logits[1, free] = logits[1].max() + 6.0  # six equal largest logits, far enough above the rest to outweigh any pointer mass ...
        src[2, :40] = order[2, :5].repeat(8)      # the five most probable tokens, eight source positions each
        src[3, :S // 2] = order[3, -3:].repeat(S // 2 // 3 + 1)[:S // 2]
        mix[3, 0] = -4.0
        mix[1, 0] = 4.0  # ... with the generator's share of row 1 near one

    return head_inputs(R, V, lens, seed, src_low=1000, design=design) + (sorted(free),)


def _head_f64(logits, mix, src, copies):
    gen = torch.softmax(logits.double().cpu(), dim=-1)
    pm = torch.softmax(mix.double().cpu(), dim=-1)
    dist = pm[:, :1] * gen
    ptr = torch.cat([pm[:, k + 1:k + 2] * c.double().cpu() for k, c in enumerate(copies)], dim=-1)
    return dist.scatter_add(1, src, ptr)


@pytest.mark.parametrize("width", [1, 4, 8])
def test_pointer_head_topk_against_f64(width):
    from case_rg_amd import ops
    R, V, lens = 6, 30522, [64, 3840]  # S = 3904
    logits, mix, sm, copies, src, tied_ids = _head_inputs(R, V, lens, 7 + width)
    gen, dist, cand_p, cand_id = ops.pointer_head_topk(logits, mix, sm, copies, width, want_gen=True, want_dist=True)
    again = ops.pointer_head_topk(logits, mix, sm, copies, width)
    assert again[0] is None and again[1] is None
    assert torch.equal(again[2], cand_p) and torch.equal(again[3], cand_id), "not deterministic from run to run"
    k_gen, k_dist, k_ids = ops.pointer_head_decode(logits, mix, sm, copies)
    assert torch.equal(dist, k_dist) and torch.equal(gen, k_gen), "the row build differs from K23's"
    assert torch.equal(cand_id[:, 0], k_ids) and torch.equal(cand_p[:, 0], k_dist.gather(1, k_ids[:, None])[:, 0]), "rank 0 is not K23's argmax bit for bit"
    # the candidates are the row's own entries, in the total order (value descending, id ascending)
    assert torch.equal(cand_p, dist.gather(1, cand_id))
    want = _head_f64(logits, mix, src, copies)
    order = np.argsort(-want.numpy(), axis=1, kind="stable")[:, :width + 1]
    for r in range(R):
        w = want[r].numpy()[order[r]]
        # f64 says which neighbours are decisively ordered: K24 works on f32 values whose relative error is ~1e-6 (fast exp, a 30 522-term sum)
        for j in range(width):
            tie = j + 1 <= width and w[j] == w[j + 1] or (j > 0 and w[j] == w[j - 1])
            clear = (j == 0 or w[j - 1] - w[j] > 1e-4 * w[j - 1]) and (w[j] - w[j + 1] > 1e-4 * w[j])
            if tie or clear:
                assert int(cand_id[r, j]) == int(order[r, j]), "row %d rank %d: id %d, f64 %d" % (r, j, int(cand_id[r, j]), int(order[r, j]))
        rel = float(np.abs(to_np(cand_p[r]).astype(np.float64) - want[r].numpy()[to_np(cand_id[r])]).max() / w[0])
        record_error("pointer_head_topk_w%d" % width, "fp32", "row%d" % r, rel, 2e-5)
        assert rel <= 2e-5, "row %d: %.2e of the row's largest probability" % (r, rel)
    if width >= 4:
        tied = cand_id[1, :min(width, 6)].tolist()
        assert tied == tied_ids[:len(tied)] and float(cand_p[1, 0]) == float(cand_p[1, len(tied) - 1]), "the tied row must list its equal entries by ascending id"


def _state_lists(state):
    return (to_np(state.alive).astype(bool), to_np(state.cum).astype(np.float64), to_np(state.len), to_np(state.parent), to_np(state.token))


@pytest.mark.parametrize("width", [1, 2, 4, 8])
def test_beam_advance_and_backtrack_against_the_restatement(width):
    """Several consecutive steps with random candidates: ties (slots that share cum and probabilities), dead slots (step 0, retired
    hypotheses), EOS retirement, the last step; then the back-track of the finished pool."""
    from case_rg_amd import ops
    B, W, T, EOS, V = 9, width, 5, 3, 12
    dev = torch.device("cuda")
    rng = np.random.RandomState(100 + width)
    state = ops.BeamState(B, W, T, dev)
    alive = [[w == 0 for w in range(W)] for _ in range(B)]
    cum = [[0.0] * W for _ in range(B)]
    length = [[1] * W for _ in range(B)]
    history, pools = [[] for _ in range(B)], [[] for _ in range(B)]
    checked = 0
    for t in range(T):
        p = rng.rand(B * W, W).astype(np.float32) * 0.5 + 1e-3
        p = -np.sort(-p, axis=1)
        ids = rng.randint(0, V, size=(B * W, W)).astype(np.int64)  # EOS = 3 turns up about once in twelve candidates
        if W > 1:  # items 0 and 1: every slot offers the same candidates -> exact ties whenever two live slots share a cost (step 1: all of them)
            for b in (0, 1):
                p[b * W:(b + 1) * W] = p[b * W]
                ids[b * W:(b + 1) * W] = ids[b * W]
            p[W:2 * W, :] = p[W, 0]  # item 1: one probability for all candidates
        ops.beam_advance(state, torch.from_numpy(p).to(dev), torch.from_numpy(ids).to(dev), t, EOS)
        g_alive, g_cum, g_len, g_parent, g_token = _state_lists(state)
        for b in range(B):
            if not any(alive[b]):
                assert not g_alive[b].any()
                history[b].append([None] * W)
                continue
            cands = [[(float(p[b * W + w, j]), int(ids[b * W + w, j])) for j in range(W)] for w in range(W)]
            slots, retired, gap = advance(cands, alive[b], cum[b], length[b], t, T, EOS, W)
            history[b].append(slots)
            for key, r in retired:
                pool_insert(pools[b], (key, t, r), W)
            alive[b] = [bool(n and n["alive"]) for n in slots]
            cum[b] = [n["cum"] if n else INF for n in slots]
            length[b] = [n["len"] if n else 0 for n in slots]
            keys = [n["key"] for n in slots if n]
            if 0.0 < min([gap] + [rel_gap(x, y) for x, y in zip(keys, keys[1:])]) < 1e-5:
                continue  # two different keys closer than f32 resolves: not a statement about the rule
            checked += 1
            for w, n in enumerate(slots):
                assert bool(g_alive[b, w]) == alive[b][w], (t, b, w)
                if n is None:
                    assert g_parent[b, w] == w and g_token[b, w] == 0 and np.isinf(g_cum[b, w])
                    continue
                assert g_parent[b, w] == n["parent"] and g_len[b, w] == n["len"], (t, b, w, g_parent[b], [s and s["parent"] for s in slots])
                assert g_token[b, w] == (n["token"] if n["alive"] else 0)
                assert int(state.hist_token[t, b, w]) == n["token"] and int(state.hist_parent[t, b, w]) == n["parent"]
                assert abs(g_cum[b, w] - n["cum"]) <= 1e-5 * max(1.0, abs(n["cum"]))
    assert checked >= B * T // 2 and not to_np(state.alive).any()
    answer, beam_answers, beam_scores = ops.beam_backtrack(state)
    for b in range(B):
        assert len(pools[b]) >= 1
        for k in range(W):
            if k >= len(pools[b]):
                assert np.isinf(float(beam_scores[b, k])) and not beam_answers[b, k].any()
                continue
            key, s, r = pools[b][k]
            assert abs(float(beam_scores[b, k]) - key) <= 1e-5 * max(1.0, abs(key)), (b, k)
            assert beam_answers[b, k].tolist() == backtrack(history[b], s, r, T), (b, k)
        assert torch.equal(answer[b], beam_answers[b, 0])
    assert any(s < T - 1 for pool in pools for _, s, _ in pool) or width == 1, "no hypothesis retired on EOS before the last step"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_beam_gather_is_index_select(dtype):
    from case_rg_amd import ops
    B, W, Tmax, E, L, t = 5, 4, 16, 64, 3, 6
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(5)
    src = [torch.randn(B * W, Tmax, 2 * E, device=dev, generator=g).to(dtype) for _ in range(L)]
    dst = [torch.full_like(s, 7.0) for s in src]
    parent = torch.randint(0, W, (B, W), device=dev, generator=g, dtype=torch.int32)
    valid_src = torch.rand(B * W, Tmax, device=dev, generator=g) > 0.3
    valid_dst = torch.zeros_like(valid_src)
    ops.beam_gather(src, dst, parent, t, valid_src, valid_dst)
    rows = (torch.arange(B, device=dev)[:, None] * W + parent.long()).reshape(-1)
    for s, d in zip(src, dst):
        assert torch.equal(d[:, :t + 1], s.index_select(0, rows)[:, :t + 1]), "copied positions"
        assert (d[:, t + 1:] == 7.0).all(), "positions behind t must stay untouched"
    assert torch.equal(valid_dst[:, :t + 1], valid_src.index_select(0, rows)[:, :t + 1]) and not valid_dst[:, t + 1:].any()
    with pytest.raises(RuntimeError, match="two different"):
        ops.beam_gather(src, src, parent, t)


# ---------------------------------------------------------------------------------------------
# 4. production geometry, bf16
# ---------------------------------------------------------------------------------------------
def _prod(ns, dev, kind="case", items=3, T=16):
    from case_rg_amd.utils import synth_batch
    m = cases._prod_test_model(ns, dev, 311, kind, cases.PROD_TEST_GAIN[kind])
    m.max_target_length = T
    b = synth_batch(items, 10, 384, 64, T, cases.PROD_V, seed=412, model=kind)
    return m.eval(), {k: v.to(dev) for k, v in b.items()}


def _teacher_forced_scores(ns, m, b, kind, answers, bos, eos):
    """cum_cost / length of every answer [B, T] from one teacher-forced pass per prefix length (independent of the cached step)."""
    B, T = answers.shape
    cost, length = np.zeros(B), np.ones(B)
    done = np.zeros(B, dtype=bool)
    prefix = torch.full((B, 1), bos, dtype=torch.long, device=b["query"].device)
    for t in range(T):
        dist = beam_cases.step_dists(ns, m, b, kind, list(range(B)), prefix).double().cpu().numpy()
        for i in range(B):
            if not done[i]:
                cost[i] += -math.log(dist[i, answers[i, t]] + 1e-10)
                length[i] += 1
                done[i] = answers[i, t] == eos
        prefix = torch.cat([prefix, torch.as_tensor(answers[:, t:t + 1], device=prefix.device)], dim=1)
    return cost / length


def test_production_geometry_bf16_fused_against_fallback_and_teacher_forcing():
    """H 512, V 30 522, ten 384-token passages, W = 4, T = 16, bf16.  (a) K24 and the torch.topk fallback feed the same search: the fallback's
    own step distributions are recorded and the restatement replayed over them, which gives the fallback's deciding gaps; the two heads work
    in f32 on the same bf16 logits, so wherever those gaps exceed beam_cases.GAP the fused ids, the fallback's and the replay's are equal;
    (b) each returned score is the length-normalised sum of -log p of an independent teacher-forced pass over the returned ids.

    The bar of (b) is measured: the bf16 teacher-forced scores against the fp32 CPU oracle's on the same ids, times 3 -- and never above
    1.0, the per-token bar on ln(top-1 probability) of the greedy bf16 tests (tests/test_parity_prod_gpu.py), since a score is a mean of
    per-token log probabilities."""
    import types
    import case_rg_amd
    import oracle
    from case_rg_amd import ops
    from case_rg_amd.common.Constants import BOS_WORD, EOS_WORD
    W, T, kind = 4, 16, "case"
    case_rg_amd.set_compute_dtype(torch.bfloat16)
    case_rg_amd.set_dropout(False)
    old = ops.POINTER_HEAD
    try:
        ns = case_rg_amd.namespace()
        ns.act_dtype = torch.bfloat16
        m, b = _prod(ns, torch.device("cuda"), kind, T=T)
        bos, eos = m.vocab2id[BOS_WORD], m.vocab2id[EOS_WORD]
        with torch.no_grad():
            with Calls() as c:
                fused = m.do_beam(dict(b), width=W)
            assert c.calls.get("case_pointer_head_beam", 0) >= 1 and c.calls.get("case_beam_gather", 0) >= 1
            ops.POINTER_HEAD = "off"
            dec, seen = m.response_generation.decoder, []
            head = dec._head

            def recording(*a):
                out = head(*a)
                seen.append(out[2][:, -1].double().cpu().numpy())  # [B * W, V] of this step
                return out

            dec._head = recording
            try:
                with Calls() as c:
                    fallback = m.do_beam(dict(b), width=W)
            finally:
                del dec._head
            assert c.calls.get("case_pointer_head_beam", 0) == 0 and c.calls.get("case_beam_advance", 0) == len(seen) >= 1
            ops.POINTER_HEAD = old
            items = fused["answer"].shape[0]
            res = pack(beam_search(None, items, W, T, bos, eos, slot_fn=lambda t, live: torch.from_numpy(np.stack([seen[t][i * W + w] for i, w in live]))),
                       W, T)
            decisive = res["gap"] > beam_cases.GAP
            record_error("beam_prod_bf16", "bf16", "decisive_items_of_%d" % items, float(decisive.sum()), float(items))
            print("deciding gaps of the fallback's run: %s" % res["gap"])
            assert decisive.any(), "no item of the fallback's run is decisive: the comparison of the ids would be empty"
            for i in np.nonzero(decisive)[0]:
                assert np.array_equal(to_np(fallback["answer"][i]), res["answer"][i]), "item %d: fallback %s, replay %s" % (i, fallback["answer"][i], res["answer"][i])
                assert torch.equal(fused["answer"][i], fallback["answer"][i]), "item %d: fused %s, fallback %s" % (i, fused["answer"][i], fallback["answer"][i])
            tf = _teacher_forced_scores(ns, m, b, kind, to_np(fused["answer"]), bos, eos)
        # the same ids through the fp32 CPU oracle: what bf16 costs on this quantity
        case_rg_amd.set_compute_dtype(torch.float32)
        ons = types.SimpleNamespace(**{k: v for k, v in vars(oracle).items() if not k.startswith("_")})
        om, ob = _prod(ons, torch.device("cpu"), kind, T=T)
        want = _teacher_forced_scores(ons, om, ob, kind, to_np(fused["answer"]), bos, eos)
        measured = float(np.abs(tf - want).max())
        bar = min(3.0 * measured, 1.0)
        got = to_np(fused["beam_score"]).astype(np.float64)
        err = float(np.abs(got - tf).max())
        record_error("beam_prod_bf16", "bf16", "teacher_forced_score_vs_fp32_oracle", measured, 1.0)
        record_error("beam_prod_bf16", "bf16", "beam_score_vs_teacher_forced", err, bar)
        print("beam scores %s\nteacher-forced bf16 %s\nfp32 oracle %s\nmeasured %.3e bar %.3e err %.3e" % (got, tf, want, measured, bar, err))
        assert err <= bar, "returned scores are %.3e away from the teacher-forced ones (bar %.3e = 3 x the measured bf16 error)" % (err, bar)
    finally:
        ops.POINTER_HEAD = old
        case_rg_amd.set_compute_dtype(torch.float32)


# ---------------------------------------------------------------------------------------------
# 5. stream capture
# ---------------------------------------------------------------------------------------------
def test_beam_pass_replays_from_a_captured_graph(ns):
    """A whole beam pass captured with torch.cuda.graph (fixed T steps, no look at device data) replays to the eager pass's ids."""
    from case_rg_amd.utils import fill_params, make_vocab, synth_batch
    V_, T, W = 200, 12, 3
    v2i, i2v = make_vocab(V_)
    model = fill_params(ns.CaSE(4, T, i2v, v2i, 32), 153, gain=3.0).cuda().eval()
    b = {k: v.cuda() for k, v in synth_batch(4, 3, 12, 8, 6, V_, seed=152, model="case").items()}
    dec = model.response_generation.decoder
    with torch.no_grad():
        full = model.do_beam(dict(b), width=W)
        assert 1 <= dec.last_beam_steps <= T
        static_out = {}
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model.do_beam(dict(b), width=W)  # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out.update(model.do_beam(dict(b), width=W))
        assert dec.last_beam_steps == T, "a captured pass runs the fixed T steps"
        graph.replay()
        torch.cuda.synchronize()
        for k in ("answer", "beam_answers", "beam_scores"):
            assert torch.equal(static_out[k], full[k]), "graph replay of the beam pass differs from the eager pass in %s" % k
