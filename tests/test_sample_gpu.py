"""Sampled decoding on the MI355X: the product's ``do_sample`` against the fixtures of the reference's own ``Generations.sample`` loop, K28
(``case_pointer_head_sample``) against the float64 restatement of the draw rule, ties and zeros, the filters' greedy limits, several samples
per item, production geometry against the CPU oracle, and stream capture.

The restatement (tests/golden/sample_cases.py) is the one tests/test_sample_cpu.py pins to the reference."""
import math
import types

import numpy as np
import pytest
import torch

import cases
import sample_cases
from helpers import Calls, head_inputs, load_golden, record_error, scaled_error, special_ids, to_np
from sample_cases import draw, rng_uniform24

pytestmark = pytest.mark.gpu

U_MAX = 1.0 - 2.0 ** -24


@pytest.fixture(scope="module")
def ns():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.float32)
    case_rg_amd.set_dropout(False)
    return case_rg_amd.namespace()


# ---------------------------------------------------------------------------------------------
# 1. the product against the reference's sample loop
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sample_cases.SAMPLE_CASES))
def test_fp32_sample_matches_the_reference_sample(ns, name):
    golden = load_golden(name)
    kind, _, _, seed, (tau, k, pp) = sample_cases.SAMPLE_CASES[name]
    m, b = sample_cases.build(ns, torch.device("cuda"), name)
    for key in ("query", "passage", "source_map"):
        assert np.array_equal(to_np(b[key]), golden["in_" + key]), key
    m.eval()
    m.sampling = dict(num_samples=1, temperature=tau, top_k=k, top_p=pp, seed=seed)
    with torch.no_grad(), Calls() as c:
        out = m(dict(b), method="sample")
        again = m.do_sample(dict(b), temperature=tau, top_k=k, top_p=pp, seed=seed)
    assert c.sampled == 2 * sample_cases.T, "the sampling kernel did not run once per step: %s" % c.calls
    assert set(out) == {"answer", "rank", "samples", "sample_probs", "sample_scores"}
    items, T = sample_cases.ITEMS, sample_cases.T
    assert out["answer"].shape == (items, T) and out["samples"].shape == (items, 1, T) and out["sample_probs"].shape == (items, 1, T)
    assert out["sample_scores"].shape == (items, 1) and torch.equal(out["answer"], out["samples"][:, 0])
    for key in ("answer", "samples", "sample_probs", "sample_scores"):
        assert torch.equal(out[key], again[key]), "%s differs between two passes with the same seed" % key
    got, prob = to_np(out["answer"]), to_np(out["sample_probs"][:, 0]).astype(np.float64)
    steps = sample_cases.decisive_steps(golden["margin"])
    assert (steps == T).sum() * 2 >= items
    eos = int(golden["eos"])
    assert any((golden["drawn"][i, :T - 1] == eos).any() and steps[i] == T for i in range(items)), "no decisive row of the fixture ends early"
    print("%s: margins %s\nproduct %s\nreference %s" % (name, np.array2string(golden["margin"], precision=2), got.tolist(), golden["answer"].tolist()))
    for i, n in enumerate(steps):
        assert np.array_equal(got[i, :n], golden["answer"][i, :n]), "%s item %d: %s != reference %s (decisive for %d steps)" % (
            name, i, got[i], golden["answer"][i], n)
    mask = np.arange(T)[None, :] < steps[:, None]
    rel = scaled_error(name + "/sample_probs", prob[mask], golden["prob"][mask])
    record_error(name, "fp32", "sample_probs", rel, 1e-3)
    assert rel <= 1e-3, "probabilities of the drawn tokens: %.2e of their scale" % rel


@pytest.mark.parametrize("name", ["sample_case", "sample_masque"])
def test_unfused_head_feeds_the_same_draw(ns, name):
    """With the fused head switched off (what an unsorted source map does too) every step draws from the unfused distribution through the
    kernel's ``dist_in`` mode: the ids are the fixture's, and the fused pass's, on every item up to its first non-decisive step, and the
    probabilities of the drawn tokens stay within the 1e-3 bar."""
    from case_rg_amd import ops
    golden = load_golden(name)
    _, _, _, seed, (tau, k, pp) = sample_cases.SAMPLE_CASES[name]
    m, b = sample_cases.build(ns, torch.device("cuda"), name)
    m.eval()
    T = sample_cases.T
    modes, real, old = [], ops.pointer_head_sample, ops.POINTER_HEAD

    def recording(logits, *a, **kw):
        modes.append("fused" if logits is not None else "dist_in" if kw.get("dist_in") is not None else "?")
        return real(logits, *a, **kw)

    ops.pointer_head_sample = recording
    try:
        with torch.no_grad(), Calls() as c:
            fused = m.do_sample(dict(b), temperature=tau, top_k=k, top_p=pp, seed=seed)
            ops.POINTER_HEAD = "off"
            plain = m.do_sample(dict(b), temperature=tau, top_k=k, top_p=pp, seed=seed)
    finally:
        ops.POINTER_HEAD, ops.pointer_head_sample = old, real
    assert modes == ["fused"] * T + ["dist_in"] * T and c.sampled == 2 * T, (modes, c.calls)
    steps = sample_cases.decisive_steps(golden["margin"])
    got, ref = to_np(plain["answer"]), to_np(fused["answer"])
    for i, n in enumerate(steps):
        assert np.array_equal(got[i, :n], golden["answer"][i, :n]) and np.array_equal(got[i, :n], ref[i, :n]), \
            "%s item %d: unfused %s, fused %s, reference %s (decisive for %d steps)" % (name, i, got[i], ref[i], golden["answer"][i], n)
    mask = np.arange(T)[None, :] < steps[:, None]
    rel = scaled_error(name + "/sample_probs_unfused", to_np(plain["sample_probs"][:, 0]).astype(np.float64)[mask], golden["prob"][mask])
    record_error(name, "fp32", "sample_probs_unfused", rel, 1e-3)
    assert rel <= 1e-3, "probabilities of the drawn tokens: %.2e of their scale" % rel


# ---------------------------------------------------------------------------------------------
# 2. / 5. K28 against the float64 restatement: the interval property, in both modes
# ---------------------------------------------------------------------------------------------
def _head_inputs(R, V, lens, seed):
    S = sum(lens)

    def design(logits, src, mix):
        src[0, :S // 2] = src[0, 0]          # one long run of a single token: it crosses the 1024-key chunk of the row build
        src[1, :40] = logits[1].argsort(descending=True)[:5].repeat(8)  # pointer mass on the most probable tokens

    return head_inputs(R, V, lens, seed, design=design)[:4]


def _interval(p, params, u, j, tol):
    """How the kernel's id ``j`` stands against the restatement's draw from the row ``p`` (f64) with the uniform ``u``: "in" with the
    violation of  CDF(j - 1) - tol Z <= u Z <= CDF(j) + tol Z  in units of tol Z (<= 1 passes), or "cut" when j is not in the restatement's
    kept set but tied with its cut within f32 rounding (value within 2e-6, or the first dropped entry with the top-p target within tol of
    the prefix mass)."""
    d = draw(p, *params, u)
    q, Z = d["q"], d["Z"]
    assert q[j] > 0, "an entry without mass was drawn (id %d)" % j
    if not d["kept"][j]:
        assert q[j] >= d["cut"] * (1 - 2e-6) or (j == d["next"] and d["slack"] <= tol), \
            "id %d (q %.9g) is outside the kept set (cut %.9g, slack %.3g) for %s" % (j, q[j], d["cut"], d["slack"], params)
        return "cut", 0.0
    lo, hi, thr = d["cdf"][j] - q[j], d["cdf"][j], u * Z
    return "in", max(lo - thr, thr - hi, 0.0) / (tol * Z)


@pytest.mark.parametrize("R", [3, 8])
@pytest.mark.parametrize("V", [200, 1031, 30522, 36000])
def test_kernel_draws_inside_the_restated_interval(V, R):
    """Explicit uniforms (0 and 1 - 2^-24 among them), S = 1500 source keys, every filter setting: the drawn id j must be kept by the
    restatement (or tied with its cut) and satisfy  CDF(j - 1) - tol <= u Z <= CDF(j) + tol,  tol = 4 (ceil(V / 1024) + 16) 2^-24 Z: four times
    the rounding bound of the issue's tiled f32 scan.  K28's scan is no deeper than that bound allows in any entry's prefix -- 3 adds inside a
    lane's four ids, 7 levels of shuffle scan and exclusive shift, at most ceil(V / 4096) carries over a wave's tiles and at most 16 adds over
    the wave totals, i.e. depth ceil(V / 4096) + 26 <= 4 (ceil(V / 1024) + 16) -- so the formula stands as stated.  ``prob`` is the row's own entry, bit for bit, the fused
    row is K23's bit for bit, and the fused and the ``dist_in`` mode draw the same ids from it."""
    from case_rg_amd import ops
    logits, mix, sm, copies = _head_inputs(R, V, [500, 1000], 11 + R)
    k23_gen, k23_dist, _ = ops.pointer_head_decode(logits, mix, sm, copies)
    rows = to_np(k23_dist).astype(np.float64)
    tol = 4 * (math.ceil(V / 1024) + 16) * 2.0 ** -24
    rs = np.random.RandomState(V + R)
    usets = [np.array(([0.0, U_MAX] * R)[:R]), np.array(([U_MAX, 0.0] * R)[:R]), rs.randint(0, 2 ** 24, R) * 2.0 ** -24, rs.randint(0, 2 ** 24, R) * 2.0 ** -24]
    worst, cuts, n = 0.0, 0, 0
    for params in [(1.0, 0, 1.0), (1.0, 1, 1.0), (1.0, 5, 1.0), (1.0, V, 1.0), (1.0, 0, 0.9), (1.0, 0, 1e-6), (0.7, 50, 0.9), (1.5, 0, 1.0)]:
        for us in usets:
            u = torch.tensor(us, dtype=torch.float32, device="cuda")
            assert np.array_equal(to_np(u).astype(np.float64), us)
            ended = torch.zeros(R, dtype=torch.uint8, device="cuda")
            with Calls() as c:
                gen, dist, ids, prob = ops.pointer_head_sample(logits, mix, sm, copies, ended, False, False, -1, -1, 0, *params, uniforms=u,
                                                               want_gen=True, want_dist=True)
                _, dist2, ids2, prob2 = ops.pointer_head_sample(None, None, None, None, ended, False, False, -1, -1, 0, *params, uniforms=u,
                                                                dist_in=k23_dist, want_dist=True)
            assert c.sampled == 2
            assert torch.equal(dist, k23_dist) and torch.equal(dist2, k23_dist), "the row differs from K23's"
            assert torch.equal(gen, k23_gen)
            assert torch.equal(ids, ids2) and torch.equal(prob, prob2), "fused and dist_in modes disagree for %s: %s vs %s" % (params, ids, ids2)
            assert torch.equal(prob, k23_dist.gather(1, ids[:, None])[:, 0]), "prob is not dist[id] bit for bit"
            assert not ended.any()
            for r in range(R):
                kind, viol = _interval(rows[r], params, float(us[r]), int(ids[r]), tol)
                cuts += kind == "cut"
                n += 1
                worst = max(worst, viol)
                assert viol <= 1.0, "V %d row %d %s u %.9g: id %d misses its interval by %.3g tol" % (V, r, params, us[r], int(ids[r]), viol)
            if params[1] == 1 or params[2] == 1e-6:
                assert torch.equal(ids, k23_dist.argmax(dim=1)), "one kept entry must be the argmax"
    record_error("pointer_head_sample_V%d_R%d" % (V, R), "fp32", "interval_violation_in_tol", worst, 1.0)
    print("V %d R %d: worst interval violation %.3g tol, %d of %d draws on a cut tie" % (V, R, worst, cuts, n))
    assert cuts * 20 <= n, "too many draws fell on a cut tie to call the kept set checked"


def test_loop_conventions_and_the_counter_uniform_in_the_kernel():
    """Rows that put all mass on one token: the kernel's emitted id, ``ended`` and ``prob`` follow the reference's loop; and with rng=(seed,
    offset, None) the uniform of row r is rng_uniform24(seed, offset + r) of the NumPy restatement."""
    from case_rg_amd import ops
    EOS, UNK, PAD, V = 9, 7, 0, 200
    dev = torch.device("cuda")
    d = torch.zeros(4, V, device=dev)
    for r, tok in enumerate([EOS, 3, EOS, 5]):
        d[r, tok] = 1.0
    u = torch.full((4,), 0.5, device=dev)

    def step(ended, first, last):
        e = torch.tensor(ended, dtype=torch.uint8, device=dev)
        with Calls() as c:
            _, _, ids, prob = ops.pointer_head_sample(None, None, None, None, e, first, last, EOS, UNK, PAD, 1.0, 0, 1.0, uniforms=u, dist_in=d)
        assert c.sampled == 1
        return ids.tolist(), e.tolist(), prob.tolist()

    assert step([0, 0, 0, 0], True, False) == ([UNK, 3, UNK, 5], [1, 0, 1, 0], [1.0] * 4)
    assert step([0, 0, 1, 1], False, False) == ([EOS, 3, PAD, PAD], [1, 0, 1, 1], [1.0] * 4)
    assert step([0, 0, 1, 1], False, True) == ([EOS, EOS, PAD, PAD], [1, 0, 1, 1], [1.0] * 4)
    # the counter stream: a row whose CDF is the identity on 1/256 steps tells the uniform's top 8 bits; 4096 rows at an odd offset
    R, seed, offset = 4096, 0x1234567887654321, 1000001
    ramp = torch.full((1, 256), 1.0 / 256, device=dev).expand(R, 256).contiguous()
    ended = torch.zeros(R, dtype=torch.uint8, device=dev)
    _, _, ids, _ = ops.pointer_head_sample(None, None, None, None, ended, False, False, -1, -1, 0, 1.0, 0, 1.0, rng=(seed, offset, None), dist_in=ramp)
    want = np.floor(rng_uniform24(seed, np.arange(R, dtype=np.uint64) + np.uint64(offset)) * 256).astype(np.int64)
    assert np.array_equal(to_np(ids), want), "the kernel's uniforms are not rng_uniform24(seed, offset + row)"


# ---------------------------------------------------------------------------------------------
# 3. ties and zeros
# ---------------------------------------------------------------------------------------------
def test_ties_and_zero_entries():
    from case_rg_amd import ops
    dev = torch.device("cuda")
    R, V = 4096, 1031
    ended = torch.zeros(R, dtype=torch.uint8, device=dev)
    flat = torch.full((R, V), 1.0 / V, device=dev)
    with Calls() as c:
        _, _, ids, prob = ops.pointer_head_sample(None, None, None, None, ended, False, False, -1, -1, 0, 1.0, 5, 1.0, rng=(5, 0, None), dist_in=flat)
    assert c.sampled == 1
    assert sorted(set(ids.tolist())) == [0, 1, 2, 3, 4], "a uniform row with top_k = 5 keeps its five lowest ids: %s" % sorted(set(ids.tolist()))
    assert torch.equal(prob, torch.full((R,), 1.0 / V, device=dev))
    # a row that is zero except three entries (the last id among them): only those are drawn, with their frequencies, the same on every run
    where, p = [7, 500, V - 1], [0.5, 0.3, 0.2]
    sparse = torch.zeros(R, V, device=dev)
    for i, x in zip(where, p):
        sparse[:, i] = x
    with Calls() as c:
        runs = [ops.pointer_head_sample(None, None, None, None, ended, False, False, -1, -1, 0, 1.0, 0, 1.0, rng=(17, 0, None), dist_in=sparse)[2]
                for _ in range(2)]
        filtered = ops.pointer_head_sample(None, None, None, None, ended, False, False, -1, -1, 0, 0.7, 0, 0.99, rng=(17, 0, None), dist_in=sparse)[2]
    assert c.sampled == 3 and torch.equal(runs[0], runs[1]), "not deterministic from run to run"
    counts = np.bincount(to_np(runs[0]), minlength=V)
    assert counts.sum() == R == counts[where].sum(), "an entry without mass was drawn: %s" % np.nonzero(counts)[0]
    assert set(filtered.tolist()) <= set(where)
    for i, x in zip(where, p):
        assert abs(counts[i] - R * x) <= 5 * math.sqrt(R * x * (1 - x)), "id %d drawn %d times of %d at probability %.1f" % (i, counts[i], R, x)
    # ids are the inverse CDF of the restated uniforms wherever u is not within 1e-6 of a boundary
    u = rng_uniform24(17, np.arange(R, dtype=np.uint64))
    want = np.where(u < 0.5, where[0], np.where(u < 0.8, where[1], where[2]))
    clear = (np.abs(u - 0.5) > 1e-6) & (np.abs(u - 0.8) > 1e-6)
    assert np.array_equal(to_np(runs[0])[clear], want[clear])


# ---------------------------------------------------------------------------------------------
# 4. one kept entry is greedy decoding
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["sample_case", "sample_masque"])
def test_one_kept_entry_equals_greedy(ns, name, dtype):
    """top_k = 1, and separately top_p = 1e-6, keep the argmax of the row K23 builds, so the drawn ids are the greedy ids of method="test" up
    to and including the first EOS -- through the loop's conventions: UNK for an EOS at step 0, EOS at the last step."""
    import case_rg_amd
    case_rg_amd.set_compute_dtype(dtype)
    try:
        m, b = sample_cases.build(ns, torch.device("cuda"), name)
        m.eval()
        _, eos, unk, _ = special_ids(m)
        T = sample_cases.T
        with torch.no_grad(), Calls() as c:
            greedy = to_np(m(dict(b), method="test")["answer"])
            outs = [m.do_sample(dict(b), top_k=1, seed=3), m.do_sample(dict(b), top_p=1e-6, seed=4)]
        assert c.calls.get("case_pointer_head_decode", 0) >= T and c.sampled == 2 * T, "not the fused heads: %s" % c.calls
        for out in outs:
            got = to_np(out["answer"])
            for i in range(got.shape[0]):
                want = beam_cut(greedy[i], eos)
                want = [unk if (t == 0 and x == eos) else eos if t == T - 1 else x for t, x in enumerate(want)]
                assert got[i, :len(want)].tolist() == want, "item %d: sampled %s, greedy %s" % (i, got[i], greedy[i])
            assert np.isfinite(to_np(out["sample_scores"])).all()
    finally:
        case_rg_amd.set_compute_dtype(torch.float32)


def beam_cut(ids, eos):
    ids = [int(i) for i in ids]
    return ids[:ids.index(eos) + 1] if eos in ids else ids


# ---------------------------------------------------------------------------------------------
# 6. several samples per item
# ---------------------------------------------------------------------------------------------
def _all_step_dists(ns, m, b, kind, rows, answers):
    """beam_cases.step_dists for every position at once: one teacher-forced pass over ``answers`` int64 [n, T] (rows: the item of each)
    -> f64 [n, T, V], position t = the distribution of token t given BOS and answers[:, :t]."""
    rows = torch.as_tensor(rows, dtype=torch.long, device=answers.device)
    q, p, sm = b["query"][rows], b["passage"][rows], b["source_map"][rows]
    vocab = len(m.vocab2id)
    was_training = m.training
    m.train()
    try:
        with torch.no_grad():
            if kind == "case":
                eq, ep = m.query_encoder(q), m.passage_encoder(p)
                ps = m.passage_selection.action(q, p, encode_query=eq, encode_passage=ep)
                se = m.span_extraction.action(q, p, encode_query=eq, encode_passage=ep, passage_selection_result=ps)
                rg = m.response_generation.action(q, p, ns.build_map(sm, max=vocab), encode_query=eq, encode_passage=ep,
                                                  passage_selection_result=ps, span_extraction_result=se, output=answers)
                dist = rg[2][0] + rg[2][1]
            else:
                eq, ep = m.query_encoder(q)[0][:, :, -1], m.passage_encoder(p)[0][:, :, -1]
                ps = m.passage_selection.action(q, p, encode_query=eq, encode_passage=ep)
                rg = m.response_generation.action(q, p, ns.build_map(sm, max=vocab), encode_query=eq, encode_passage=ep,
                                                  passage_selection_result=ps, output=answers)
                dist = rg[2]
    finally:
        m.train(was_training)
    return dist.double().cpu().numpy()


@pytest.mark.parametrize("name", ["sample_case", "sample_masque"])
def test_several_samples_per_item(ns, name):
    """num_samples = 4: shapes; the rows of an item differ; the pass is, bit for bit, a 16-row pass handed each row's counter uniform; row b N + n
    is the num_samples = 1 pass given that row's uniforms -- exactly, up to the row's first non-decisive step (the margins of the restated draws on the product's own teacher-forced distributions against
    sample_cases.GAP: a pass over 16 rows and one over 4 rows may round a distribution differently); scores are the mean -log of the
    probabilities."""
    kind, N, seed = sample_cases.SAMPLE_CASES[name][0], 4, 29
    m, b = sample_cases.build(ns, torch.device("cuda"), name)
    m.eval()
    _, eos, unk, pad = special_ids(m)
    B, T = sample_cases.ITEMS, sample_cases.T
    R = B * N
    with torch.no_grad(), Calls() as c:
        out = m.do_sample(dict(b), num_samples=N, seed=seed)
    assert c.sampled == T
    assert out["samples"].shape == (B, N, T) and out["sample_probs"].shape == (B, N, T) and out["sample_scores"].shape == (B, N)
    assert out["answer"].shape == (B, T) and torch.equal(out["answer"], out["samples"][:, 0])
    samples, probs = to_np(out["samples"]), to_np(out["sample_probs"]).astype(np.float64)
    assert all(len({tuple(s) for s in samples[i]}) > 1 for i in range(B)), "the samples of an item are all equal: %s" % samples.tolist()
    emitted = samples != pad
    for row, pr in zip(samples.reshape(R, T), probs.reshape(R, T)):  # behind an EOS: PAD with probability 1 (a PAD in front of it is a drawn token)
        if eos in row[:T - 1]:
            end = row.tolist().index(eos)
            assert not row[end + 1:].any() and (pr[end + 1:] == 1.0).all(), (row, pr)
    want_scores = (-np.log(probs) * emitted).sum(-1) / np.maximum(emitted.sum(-1), 1)
    np.testing.assert_allclose(to_np(out["sample_scores"]), want_scores, rtol=1e-5, atol=1e-6)
    u = rng_uniform24(seed, np.arange(T * R, dtype=np.uint64)).reshape(T, R)  # counter t R + b N + n
    # at the same number of rows nothing rounds differently: handing every row the uniform of its counter repeats the pass bit for bit
    with torch.no_grad(), Calls() as c:
        same = m.do_sample(dict(b), num_samples=N, uniforms=torch.tensor(u, dtype=torch.float32, device="cuda"))
    assert c.sampled == T
    for key in ("samples", "sample_probs", "sample_scores"):
        assert torch.equal(same[key], out[key]), "row b N + n at step t does not draw at counter t B N + b N + n: %s differs" % key
    flat = samples.reshape(R, T)
    dists = _all_step_dists(ns, m, b, kind, np.repeat(np.arange(B), N), torch.as_tensor(flat, device="cuda"))
    margin = np.full((R, T), np.inf)
    for r in range(R):
        ended = False
        for t in range(T):
            if ended:
                break
            d = draw(dists[r, t], 1.0, 0, 1.0, float(u[t, r]))
            margin[r, t] = d["margin"]
            ended = d["id"] == eos
    steps = sample_cases.decisive_steps(margin).reshape(B, N)
    assert (steps == T).sum() * 2 >= R, "fewer than half the rows are decisive throughout: %s" % steps
    for n in range(N):
        un = torch.tensor(u.reshape(T, B, N)[:, :, n], dtype=torch.float32, device="cuda")
        with torch.no_grad(), Calls() as c:
            single = m.do_sample(dict(b), uniforms=un)
        assert c.sampled == T
        one = to_np(single["samples"][:, 0])
        for i in range(B):
            k = steps[i, n]
            assert np.array_equal(one[i, :k], samples[i, n, :k]), "item %d sample %d: %s alone, %s among %d (decisive for %d steps)" % (
                i, n, one[i], samples[i, n], N, k)


def test_pass_stops_once_every_row_has_ended(ns):
    """Item 1 of the top-k fixture draws EOS at step 0 (emitted as UNK, ended from step 1).  Alone in its batch, with the fixture's uniforms and
    the end checked every step, the pass stops after that step and fills the rest with PAD at probability 1 -- what the full-length pass emits."""
    name = "sample_case_k5"
    golden = load_golden(name)
    _, _, _, _, (tau, k, pp) = sample_cases.SAMPLE_CASES[name]
    m, b = sample_cases.build(ns, torch.device("cuda"), name)
    m.eval()
    T, item = sample_cases.T, 1
    assert np.isinf(golden["margin"][item, 1:]).all() and golden["margin"][item, 0] > sample_cases.GAP
    one = {key: v[item:item + 1] for key, v in b.items()}
    u = torch.tensor(golden["u"][item][:, None], dtype=torch.float32, device="cuda")
    dec = m.response_generation.decoder
    keep = dec.eos_check_every
    try:
        outs = []
        for every in (1, 1 << 30):
            dec.eos_check_every = every
            with torch.no_grad(), Calls() as c:
                outs.append(m.do_sample(dict(one), temperature=tau, top_k=k, top_p=pp, uniforms=u))
            assert c.sampled == dec.last_sample_steps == (1 if every == 1 else T), (every, c.calls, dec.last_sample_steps)
    finally:
        dec.eos_check_every = keep
    assert to_np(outs[0]["answer"]).tolist() == [golden["answer"][item].tolist()] and to_np(outs[0]["sample_probs"])[0, 0, 1:].tolist() == [1.0] * (T - 1)
    for key in ("samples", "sample_probs", "sample_scores"):
        assert torch.equal(outs[0][key], outs[1][key]), key


# ---------------------------------------------------------------------------------------------
# 7. production-like rows against the CPU oracle
# ---------------------------------------------------------------------------------------------
def test_production_rows_draw_inside_the_oracle_interval(ns):
    """V = 30 522, H = 512, 2 items x 4 samples x 6 steps, fp32: every token the product drew satisfies the interval property against the CPU
    oracle's teacher-forced distribution of its prefix, with tol = the project's 1e-3 parity bar times Z."""
    import oracle
    kind, N, T, seed = "case", 4, 6, 41
    dev = torch.device("cuda")
    m = cases._prod_test_model(ns, dev, 311, kind, cases.PROD_TEST_GAIN[kind]).eval()
    m.max_target_length = T
    b = cases._prod_test_batch(dev, 312, kind)
    _, eos, unk, pad = special_ids(m)
    B = b["query"].shape[0]
    R = B * N
    with torch.no_grad(), Calls() as c:
        out = m.do_sample(dict(b), num_samples=N, seed=seed)
    assert c.sampled == T and B == 2
    samples = to_np(out["samples"])
    u = rng_uniform24(seed, np.arange(T * R, dtype=np.uint64)).reshape(T, B, N)
    ons = types.SimpleNamespace(**{k: v for k, v in vars(oracle).items() if not k.startswith("_")})
    om = cases._prod_test_model(ons, torch.device("cpu"), 311, kind, cases.PROD_TEST_GAIN[kind])
    om.max_target_length = T
    ob = {k: v.cpu() for k, v in b.items()}
    checked, worst = 0, 0.0
    for n in range(N):  # (two rows per oracle pass: its source map is a dense one-hot over the vocabulary)
        dists = _all_step_dists(ons, om, ob, kind, np.arange(B), torch.as_tensor(samples[:, n]))
        for i in range(B):
            ended = False
            for t in range(T):
                if ended:
                    assert samples[i, n, t] == pad
                    continue
                x = int(samples[i, n, t])
                if t == T - 1:
                    assert x == eos  # forced: the drawn id is not visible
                    continue
                if t == 0 and x == unk:  # either UNK itself or an EOS emitted as UNK, which ends the row from step 1
                    ended = samples[i, n, 1] == pad
                    continue
                ended = x == eos
                kindof, viol = _interval(dists[i, t], (1.0, 0, 1.0), float(u[t, i, n]), x, 1e-3)
                checked += 1
                worst = max(worst, viol)
                assert kindof == "in" and viol <= 1.0, "item %d sample %d step %d: id %d misses the oracle's interval by %.3g of the 1e-3 bar" % (i, n, t, x, viol)
                got_p, want_p = float(out["sample_probs"][i, n, t]), dists[i, t, x]
                assert abs(got_p - want_p) <= 1e-3 * dists[i, t].max() + 1e-6, (i, n, t, got_p, want_p)
    record_error("sample_prod_fp32", "fp32", "interval_violation_in_1e-3", worst, 1.0)
    print("production rows: %d draws checked, worst violation %.3g of the bar" % (checked, worst))
    assert checked >= R, "too few draws were visible to check (%d)" % checked


# ---------------------------------------------------------------------------------------------
# 8. stream capture
# ---------------------------------------------------------------------------------------------
def test_sampled_pass_replays_from_a_captured_graph(ns):
    """A sampled pass captured with torch.cuda.graph runs the fixed T steps.  With a device step state installed the counters are
    rng_base + offset + row with rng_base read on the device: replays under two bases give two different sets of samples, each the eager
    pass at that base.  Without a device state seed and offsets are frozen into the graph: a replay repeats its samples."""
    from case_rg_amd import config, stepstate
    from case_rg_amd.utils import fill_params, make_vocab, synth_batch
    V_, T, N = 200, 12, 2
    v2i, i2v = make_vocab(V_)
    model = fill_params(ns.CaSE(4, T, i2v, v2i, 32), 153, gain=3.0).cuda().eval()
    b = {k: v.cuda() for k, v in synth_batch(4, 3, 12, 8, 6, V_, seed=152, model="case").items()}
    dec = model.response_generation.decoder
    keys = ("samples", "sample_probs", "sample_scores")
    keep = config.rng_state()

    def sampled():
        config.manual_seed(77)  # every pass numbers its draws from offset 0
        return model.do_sample(dict(b), num_samples=N, top_k=20, temperature=0.9)

    def captured():
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            sampled()  # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        graph, static = torch.cuda.CUDAGraph(), {}
        config.manual_seed(77)
        with torch.cuda.graph(graph), Calls() as c:
            static.update(model.do_sample(dict(b), num_samples=N, top_k=20, temperature=0.9))
        assert c.sampled == T == dec.last_sample_steps, "a captured pass runs the fixed T steps"
        return graph, static

    try:
        with torch.no_grad():
            # without a device state
            eager = {k: v.clone() for k, v in sampled().items()}
            assert 1 <= dec.last_sample_steps <= T
            graph, static = captured()
            for _ in range(2):
                graph.replay()
                torch.cuda.synchronize()
                for k in keys:
                    assert torch.equal(static[k], eager[k]), "without a device state a replay must repeat the eager pass's %s" % k
            del graph
            # with one
            state = stepstate.StepState("cuda")
            config.set_device_state(state.address, owner=state)
            bases = (1000, 500000)
            eagers = []
            for base in bases:
                state.upload(rng_base=base)
                eagers.append({k: v.clone() for k, v in sampled().items()})
            assert not torch.equal(eagers[0]["samples"], eagers[1]["samples"]), "two counter bases drew the same samples"
            graph, static = captured()
            for base, want in zip(bases, eagers):
                state.upload(rng_base=base)
                graph.replay()
                torch.cuda.synchronize()
                for k in keys:
                    assert torch.equal(static[k], want[k]), "replay at rng_base %d differs from the eager pass at that base in %s" % (base, k)
    finally:
        config.set_device_state(None)
        config.manual_seed(keep[0])
        config.set_rng_state(keep)
