"""BLEU and n-gram overlap on the MI355X: K34 (``case_ngram_counts``) against the ``Counter`` restatement of tests/test_bleu_cpu.py, exactly, at
the 64-bit word boundaries of its match masks, across the 64-token loads of a long reference and over more hypotheses than the device holds
at once; K35 (``case_bleu_scores``) against the f64 restatement; the raw-row functions of ``evaluation.ngram_ids`` against the host form
``evaluation.bleu``; the overlap ratio against the reference-generated fixture; ``consensus(metric="bleu")``, ``do_consensus`` of both task
models, stream capture; the trainer's ``evaluate_bleu`` against ``predict`` + ``to_sentence`` + the host's ``eval_bleu``.

nltk is not available where the fixtures are built, so no BLEU number here comes from running the reference's ``Eval_Bleu.py``; the
restatement is pinned to nltk's published worked example in tests/test_bleu_cpu.py.

Counts are integers and compared exactly.  ``bleu`` (f64) is compared at 1e-12 absolute: about a hundred times the few-ulp difference between
two f64 ``log`` / ``exp`` libraries over five calls on a value in [0, 1].  ``bleu_pair`` at 1.2e-7 absolute: one f32 rounding of a value in
[0, 1] (the project's F_TOL); utilities at 1e-6 relative (f32 sums of at most 64 terms against f64); overlap ratios at 1e-15 (equal small
integers divided).  Measured maxima go to the session's parity ledger (``helpers.record_error``, case "bleu"); profiles/bleu_parity.json
keeps a copy."""
import math

import numpy as np
import pytest
import torch

import cases
import sample_cases
from helpers import Calls, load_golden, record_error, to_np
from test_bleu_cpu import restated_bleu, restated_bp, restated_counts
from test_consensus_cpu import restated_pick

pytestmark = pytest.mark.gpu

F_TOL, D_TOL = 1.2e-7, 1e-12
PAD, BOS, EOS, UNK, FIRST = 0, 1, 2, 3, 4  # the ids of the kernel-level tests
SPECIALS = (BOS, PAD, EOS, UNK)
COUNT_KEYS = ("clip", "clip_any", "hit", "hit_any", "distinct")


@pytest.fixture(scope="module")
def ns():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.float32)
    case_rg_amd.set_dropout(False)
    return case_rg_amd.namespace()


def _note(key, value, tol):
    record_error("bleu", "fp32", key, value, tol)


def _dev(x):
    return torch.as_tensor(x).cuda()


def _packed(lists, T, junk=FIRST + 1):
    """Token lists -> (front-packed int64 [n, T] with garbage behind the length -- an id of the vocabulary, so that reading it would count --,
    lengths int32 [n])."""
    ids = np.full((len(lists), T), junk, dtype=np.int64)
    for i, toks in enumerate(lists):
        ids[i, :len(toks)] = toks
    return ids, np.array([len(t) for t in lists], dtype=np.int32)


def _raw_rows(lists, T):
    """Token lists -> raw decoder-style rows int64 [n, T]: BOS, the tokens, EOS, then ids that must be ignored; a PAD inside the sentence."""
    out = np.zeros((len(lists), T), dtype=np.int64)
    for i, toks in enumerate(lists):
        row = [BOS] + list(toks[:len(toks) // 2]) + [PAD] + list(toks[len(toks) // 2:]) + [EOS, FIRST + 1, FIRST + 2]
        assert len(row) <= T + 3
        row = row[:T]
        out[i, :len(row)] = row
    return out


def want_counts(hyps, refs, max_n=4):
    """The restatement's counts in K34's layout for ONE item: dict of int arrays clip / hit [N, M, 4], clip_any / hit_any / distinct [N, 4];
    orders above ``max_n`` read 0."""
    N, M = len(hyps), len(refs)
    out = dict(clip=np.zeros((N, M, 4), np.int32), hit=np.zeros((N, M, 4), np.int32), clip_any=np.zeros((N, 4), np.int32),
               hit_any=np.zeros((N, 4), np.int32), distinct=np.zeros((N, 4), np.int32))
    for n, h in enumerate(hyps):
        for k in range(1, max_n + 1):
            c = restated_counts(h, refs, k)
            out["clip"][n, :, k - 1], out["hit"][n, :, k - 1] = c["clip"], c["hit"]
            out["clip_any"][n, k - 1], out["hit_any"][n, k - 1], out["distinct"][n, k - 1] = c["clip_any"], c["hit_any"], c["distinct"]
    return out


def run_counts(items, Ta, Tb, max_n=4):
    """items: per item (hypothesis lists, reference lists), the same N and M everywhere -> (K34's dict as numpy, a_len, b_len tensors)."""
    from case_rg_amd import ops
    a, a_len = zip(*[_packed(h, Ta) for h, _ in items])
    b, b_len = zip(*[_packed(r, Tb) for _, r in items])
    a_len, b_len = _dev(np.stack(a_len)), _dev(np.stack(b_len))
    with Calls() as c:
        got = ops.ngram_counts(_dev(np.stack(a)), a_len, _dev(np.stack(b)), b_len, max_n)
    assert c.calls == {"case_ngram_counts": 1}
    assert set(got) == set(COUNT_KEYS) and all(v.dtype == torch.int32 for v in got.values())
    return got, a_len, b_len


def check_counts(got, items, max_n=4, what=""):
    for i, (hyps, refs) in enumerate(items):
        want = want_counts(hyps, refs, max_n)
        for key in COUNT_KEYS:
            g = to_np(got[key][i])
            if not np.array_equal(g, want[key]):
                at = tuple(int(x[0]) for x in np.nonzero(g != want[key]))
                raise AssertionError("%s item %d: %s differs at %s (hypothesis of %d tokens): got %d, restatement %d" % (
                    what, i, key, at, len(hyps[at[0]]), g[at], want[key][at]))


# ---------------------------------------------------------------------------------------------
# 1. K34 at the word boundaries and across the loads of a long reference
# ---------------------------------------------------------------------------------------------
HYP_LENS = (1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 255, 256)
GRAM = (FIRST, FIRST + 1, FIRST + 2, FIRST)  # as  a b c a b c a  it occurs twice in seven positions


def boundary_items(Ta):
    """Three items of the same hypotheses against three references each.  Vocabulary of 6 ids, so that counts exceed 1 and clipping bites.
    Hypotheses: length 0 (every count 0) and what the raw-row functions make of it ([UNK]), every length of HYP_LENS up to ``Ta``, and one
    whose repeated 4-gram straddles positions 61..67 (from Ta = 128 on: the carry into word 1) and 125..131 (Ta = 256: into word 2).
    References: lengths (1, 3, 63), (64, absent, 65) and (130, 3 840, absent); the 130- and the 3 840-token ones hold the 4-gram across
    positions 62..65, the boundary between two 64-token loads."""
    rs = np.random.RandomState(340 + Ta)
    tok = lambda n: (rs.randint(0, 6, n) + FIRST).tolist()  # noqa: E731
    hyps = [[], [UNK]] + [tok(n) for n in HYP_LENS if n <= Ta]
    straddle = tok(min(Ta, 140))
    for at in (61, 125):
        if at + 7 <= len(straddle):
            straddle[at:at + 7] = list(GRAM[:3]) * 2 + [GRAM[0]]
    hyps.append(straddle)
    refs = [[tok(1), tok(3), tok(63)], [tok(64), [], tok(65)], [tok(130), tok(3840), []]]
    for r in refs[2][:2]:
        r[62:66] = GRAM
    return [(hyps, r) for r in refs]


@pytest.mark.parametrize("Ta", [64, 128, 256])
def test_ngram_counts_at_the_word_and_load_boundaries(Ta):
    items = boundary_items(Ta)
    got, _, _ = run_counts(items, Ta, 3840)
    assert got["clip"].shape == (3, len(items[0][0]), 3, 4) and got["distinct"].shape == (3, len(items[0][0]), 4)
    check_counts(got, items, what="Ta %d" % Ta)
    if Ta >= 128:  # (64 positions cannot hold 61..67: nothing is planted there; 128 hold the first copy, 256 both)
        straddle = want_counts(items[2][0][-1:], items[2][1])
        assert straddle["clip"][0, 0, 3] >= 1 and straddle["distinct"][0, 3] < len(items[2][0][-1]) - 3, "the planted 4-gram must repeat and match"
    assert (to_np(got["clip"])[:, :, :, 0] > to_np(got["hit"])[:, :, :, 0]).any(), "clipped counts above 1 must occur"
    assert (to_np(got["clip_any"]) > to_np(got["clip"]).max(axis=2)).any(), "clip_any must not be derivable from clip"


@pytest.mark.parametrize("max_n", [1, 2, 4])
def test_ngram_counts_single_reference_and_lower_orders(max_n):
    """M = 1; the orders above ``max_n`` read 0."""
    hyps = boundary_items(128)[0][0]
    rs = np.random.RandomState(341)
    items = [(hyps, [(rs.randint(0, 6, 65) + FIRST).tolist()])]
    got, _, _ = run_counts(items, 128, 65, max_n)
    check_counts(got, items, max_n, what="max_n %d" % max_n)
    for key in COUNT_KEYS:
        assert not to_np(got[key])[..., max_n:].any() and to_np(got[key])[..., :max_n].any(), key


@pytest.mark.parametrize("BN", [1, 5, 4099])
def test_ngram_counts_grid_tail(BN):
    """B x N hypotheses of up to 16 tokens, four to a workgroup: one, a workgroup and a quarter, and more waves than the device holds at once
    with a partly filled last workgroup.  Items of one hypothesis (and of five), two references each."""
    rs = np.random.RandomState(342 + BN)
    N = 5 if BN == 5 else 1
    tok = lambda n: (rs.randint(0, 6, n) + FIRST).tolist()  # noqa: E731
    items = [([tok(rs.randint(1, 17)) for _ in range(N)], [tok(rs.randint(0, 17)), tok(rs.randint(0, 17))]) for _ in range(BN // N)]
    got, _, _ = run_counts(items, 16, 16)
    check_counts(got, items, what="B x N = %d" % BN)


# ---------------------------------------------------------------------------------------------
# 2. K35 against the f64 restatement
# ---------------------------------------------------------------------------------------------
def noisy_items(count=96, seed=343):
    """Noisy copies: each hypothesis is a prefix of a reference of 12..40 tokens from 50 ids with every token replaced with probability
    0.15; two random distractor references are added (one of them absent in every fifth item).  The last two items have no present
    reference and a one-token hypothesis."""
    rs = np.random.RandomState(seed)
    items = []
    for i in range(count):
        ref = (rs.randint(0, 50, rs.randint(12, 41)) + FIRST).tolist()
        hyp = [int(rs.randint(0, 50)) + FIRST if rs.rand() < 0.15 else t for t in ref[:rs.randint(max(8, len(ref) // 2), len(ref) + 1)]]
        others = [(rs.randint(0, 50, rs.randint(12, 41)) + FIRST).tolist() for _ in range(2)]
        if i % 5 == 0:
            others[0] = []
        refs = [others[0], ref, others[1]]
        items.append(([hyp], [refs[(m + i) % 3] for m in range(3)]))
    items[-2] = (items[-2][0], [[], [], []])
    items[-1] = ([[items[-1][1][0][0] if items[-1][1][0] else FIRST]], items[-1][1])
    return items


@pytest.fixture(scope="module")
def noisy():
    """The items, K34's counts of them and the lengths, computed once and left unchanged."""
    items = noisy_items()
    counts, a_len, b_len = run_counts(items, 40, 40)
    check_counts(counts, items, what="noisy copies")
    return items, counts, a_len, b_len


@pytest.mark.parametrize("smoothing", ["none", "add1"])
@pytest.mark.parametrize("max_n", [4, 2])
def test_bleu_scores_against_the_restatement(noisy, smoothing, max_n):
    from case_rg_amd import ops
    items, counts, a_len, b_len = noisy
    with Calls() as c:
        pair, bleu, bp = ops.bleu_scores(counts, a_len, b_len, max_n, smoothing)
    assert c.calls == {"case_bleu_scores": 1}
    assert pair.dtype == torch.float32 and pair.shape == (len(items), 1, 3) and bleu.dtype == bp.dtype == torch.float64 and bleu.shape == (len(items), 1)
    pair, bleu, bp = to_np(pair).astype(np.float64), bleu.cpu().numpy(), bp.cpu().numpy()
    worst = dict(bleu=0.0, pair=0.0, bp=0.0)
    nonzero = 0
    for i, (hyps, refs) in enumerate(items):
        want = restated_bleu(hyps[0], refs, max_n, smoothing)
        nonzero += want > 0
        assert (want == 0.0) == (bleu[i, 0] == 0.0), "item %d: exactly 0 where the restatement is" % i
        worst["bleu"] = max(worst["bleu"], abs(bleu[i, 0] - want))
        worst["bp"] = max(worst["bp"], abs(bp[i, 0] - restated_bp(len(hyps[0]), [len(r) for r in refs])[0]))
        for m, r in enumerate(refs):
            worst["pair"] = max(worst["pair"], abs(pair[i, 0, m] - restated_bleu(hyps[0], [r], max_n, smoothing)))
    for key, w in worst.items():
        print("bleu_scores(max_n %d, %s): max |%s - restatement| = %.3e" % (max_n, smoothing, key, w))
        _note("scores_%s_n%d_%s" % (key, max_n, smoothing), w, F_TOL if key == "pair" else D_TOL)
    if smoothing == "none":
        assert 2 * nonzero >= len(items), "only %d of %d items have a nonzero BLEU-%d: the inputs prove nothing" % (nonzero, len(items), max_n)
    assert bleu[-2, 0] == 0.0 and bp[-2, 0] == 0.0 and not pair[-2].any(), "no present reference"
    assert worst["bleu"] <= D_TOL and worst["bp"] <= D_TOL and worst["pair"] <= F_TOL, worst


# ---------------------------------------------------------------------------------------------
# 3. raw rows against the host form
# ---------------------------------------------------------------------------------------------
def test_bleu_ids_on_raw_rows_is_the_host_form():
    from case_rg_amd.common.Utils import remove_duplicate
    from case_rg_amd.evaluation import bleu_ids, eval_bleu, eval_bleu_ids, sentence_bleu
    items = noisy_items(24, seed=344)
    rs = np.random.RandomState(345)
    hyps = [h[0] for h, _ in items]
    hyps[0] = []                                                   # an empty answer counts as [UNK]
    hyps[1] = hyps[1][:6] + hyps[1][:6] + hyps[1][:6]              # repeated 6 tokens: remove_duplicate cuts them
    hyps[2] = (rs.randint(0, 3, 30) + FIRST).tolist()
    refs = [r for _, r in items]
    T = 48
    hyp, ref = _dev(_raw_rows(hyps, T)), _dev(np.stack([_raw_rows(r, T) * (np.array([len(x) for x in r])[:, None] > 0) for r in refs]))
    for dedup in (False, True):
        lists = [h if h else [UNK] for h in hyps]
        if dedup:
            lists = [list(h) for h in lists]
            remove_duplicate(lists)
            assert len(lists[1]) < 18, "remove_duplicate must cut the repeated answer"
        for smoothing in ("none", "add1"):
            out = bleu_ids(hyp, ref, SPECIALS, smoothing=smoothing, remove_duplicates=dedup)
            assert set(out) == {"clip", "clip_any", "total", "bleu_pair", "bleu", "bp", "ref_valid"}
            assert to_np(out["ref_valid"]).tolist() == [[len(x) > 0 for x in r] for r in refs]
            assert to_np(out["total"][:, 0]).tolist() == [[max(len(h) - k, 0) for k in range(4)] for h in lists]
            want = np.array([sentence_bleu(h, r, 4, smoothing) for h, r in zip(lists, refs)])
            gap = float(np.abs(out["bleu"][:, 0].cpu().numpy() - want).max())
            _note("raw_rows_bleu_%s%s" % (smoothing, "_dedup" if dedup else ""), gap, D_TOL)
            assert gap <= D_TOL, gap
            pairs = np.array([[sentence_bleu(h, [x], 4, smoothing) for x in r] for h, r in zip(lists, refs)])
            assert float(np.abs(to_np(out["bleu_pair"][:, 0]).astype(np.float64) - pairs).max()) <= F_TOL
        per_item = eval_bleu_ids(hyp, ref, SPECIALS, remove_duplicates=dedup)
        assert per_item.dtype == torch.float64 and per_item.shape == (24,) and per_item.is_cuda
        assert float(per_item[-2]) == 0.0, "an item without a present reference scores 0"
        assert round(float(per_item.mean()), 2) == eval_bleu(lists, refs) > 0.0
    with pytest.raises(TypeError, match="one answer per item"):
        eval_bleu_ids(hyp.unsqueeze(1), ref, SPECIALS)


# ---------------------------------------------------------------------------------------------
# 4. overlap
# ---------------------------------------------------------------------------------------------
def test_ngram_overlap_ids_matches_the_reference_fixture():
    from case_rg_amd.evaluation import ngram_overlap_ids
    g = load_golden("overlap")
    answers = [g["answers"][i, :n].tolist() for i, n in enumerate(g["answer_len"])]
    sources = [g["sources"][i, :n].tolist() for i, n in enumerate(g["source_len"])]
    T, S = 2 + 3 + g["answers"].shape[1], 2 + 3 + g["sources"].shape[1]
    got = ngram_overlap_ids(_dev(_raw_rows(answers, T)), _dev(_raw_rows(sources, S)), SPECIALS)
    assert got.dtype == torch.float64 and got.shape == (24, 1, 4)
    gap = float(np.abs(got[:, 0].cpu().numpy() - g["ratios"]).max())
    _note("overlap_fixture", gap, 1e-15)
    assert gap <= 1e-15, gap
    # an empty answer counts as [UNK]; max_n cuts the orders
    ans = _dev(np.array([[BOS, EOS, 9, 9], [BOS, 9, 8, EOS]], dtype=np.int64))
    src = _dev(np.array([[UNK, 9, 8, 7, EOS], [7, 9, 8, 9, 8]], dtype=np.int64))
    assert ngram_overlap_ids(ans, src, SPECIALS, max_n=2)[:, 0].tolist() == [[1.0, 0.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0]]


def test_ngram_overlap_ids_over_passage_rows_does_not_span_them():
    """source [B, P, L]: every passage compacted on its own.  The answers are cut out of the concatenated passages ACROSS a boundary, so the
    flat form finds n-grams that the row form must not."""
    from case_rg_amd.evaluation import ngram_overlap_ids
    rs = np.random.RandomState(346)
    B, P, L = 6, 3, 40
    passages = [[(rs.randint(0, 30, rs.randint(10, L - 4)) + FIRST).tolist() for _ in range(P)] for _ in range(B)]
    passages[1][2] = []
    answers = [[(p[0][-5:] + p[1][:5]), (rs.randint(0, 30, 12) + FIRST).tolist(), p[0][2:9]] for p in passages]
    src = _dev(np.stack([_raw_rows(p, L) * (np.array([len(x) for x in p])[:, None] > 0) for p in passages]))
    ans = _dev(np.stack([_raw_rows(a, 20) for a in answers]))
    got = ngram_overlap_ids(ans, src, SPECIALS).cpu().numpy()
    flat = ngram_overlap_ids(ans, _dev(_raw_rows([sum(p, []) for p in passages], P * L)), SPECIALS).cpu().numpy()
    assert got.shape == (B, 3, 4)
    for i in range(B):
        for n, a in enumerate(answers[i]):
            for k in range(1, 5):
                c = restated_counts(a, passages[i], k)
                assert got[i, n, k - 1] == (c["hit_any"] / c["distinct"] if c["distinct"] else 0.0), (i, n, k)
                c = restated_counts(a, [sum(passages[i], [])], k)
                assert flat[i, n, k - 1] == c["hit_any"] / c["distinct"]
    assert (flat[0, 0, 1:] > got[0, 0, 1:]).all() and (got[:, 2] == 1.0).all()


# ---------------------------------------------------------------------------------------------
# 5. consensus under BLEU
# ---------------------------------------------------------------------------------------------
def bleu_pick(pool, weights=None, valid=None):
    """``restated_pick`` of tests/test_consensus_cpu.py with the restated add-one BLEU-4 as its pairwise utility: the function looks
    ``evaluation.rouge_l`` up when it is called, so the utility is handed to it there."""
    from case_rg_amd import evaluation
    keep = evaluation.rouge_l
    evaluation.rouge_l = lambda hyp, ref: (restated_bleu(hyp, [ref], 4, "add1"),)
    try:
        return restated_pick(pool, weights, valid)
    finally:
        evaluation.rouge_l = keep


def consensus_pools():
    """9 items x 7 candidates: noisy copies of one sentence per item (so that the utilities are well above 0 and differ), planted exact ties,
    an empty candidate, masks and weights as in the ROUGE-L test."""
    rs = np.random.RandomState(347)
    B, N = 9, 7
    pools = []
    for _ in range(B):
        base = (rs.randint(0, 20, rs.randint(8, 30)) + FIRST).tolist()
        pools.append([[int(rs.randint(0, 20)) + FIRST if rs.rand() < 0.2 else t for t in base[:rs.randint(5, len(base) + 1)]] for _ in range(N)])
    q, z, w5 = [FIRST, FIRST + 1, FIRST + 2, FIRST + 3, FIRST + 4], [100, 101, 102], [200, 201]
    pools[0] = [z, [100, 102], q, q, w5, q, [201]]     # a planted exact tie between 2, 3 and 5, well ahead of the rest
    pools[1] = [w5, z, q, q, q, [100], [200]]          # the same three-fold copy: weights will move the pick to 0
    pools[2][4] = []                                   # an empty candidate counts as [UNK]
    valid = np.ones((B, N), dtype=bool)
    valid[3, [0, 5]] = False
    valid[4] = False                                   # an item without a valid candidate
    valid[0, 6] = False
    weights = rs.uniform(0.1, 1.0, (B, N)).astype(np.float32)
    weights[1] = (50.0, 1e-3, 1.0, 1.0, 1.0, 1e-3, 1e-3)
    return pools, valid, weights


def check_bleu_consensus(res, pools, weights=None, valid=None, tag="", picks=True):
    """``res``: consensus(..., metric="bleu") over ``pools`` (token lists, [UNK] for an empty one).  ``pairwise_bleu`` at F_TOL, utilities at
    1e-6 relative, -inf exactly where invalid, the pick the first maximum of the returned utilities and (``picks``) the restatement's pick.
    The f32 sums of K31 cannot order two candidates differently from the f64 restatement when their utilities are equal (equal rows of the
    matrix sum to equal bits in both) or at least 1e-5 apart (ten times the 1e-6 bound on either); the inputs of the tests that ask for
    identical picks are checked to have no other kind of leading pair."""
    worst_f, worst_u = 0.0, 0.0
    util, index, pf = to_np(res["consensus_utility"]).astype(np.float64), to_np(res["consensus_index"]), to_np(res["pairwise_bleu"]).astype(np.float64)
    for i, pool in enumerate(pools):
        u, at, f = bleu_pick(pool, None if weights is None else weights[i], None if valid is None else valid[i])
        worst_f = max(worst_f, float(np.abs(pf[i] - np.array(f)).max()))
        for n, un in enumerate(u):
            if un == -math.inf:
                assert util[i, n] == -math.inf, "item %d candidate %d is invalid and must read -inf" % (i, n)
            else:
                worst_u = max(worst_u, abs(util[i, n] - un) / max(abs(un), 1e-30))
        assert index[i] == int(np.argmax(util[i])), "item %d: index %d is not the first maximum of %s" % (i, index[i], util[i])
        if picks:
            ranked = sorted((x for x in u if x > -math.inf), reverse=True)
            lead = [x for x in ranked if x < ranked[0]] if ranked else []
            assert not lead or ranked[0] - lead[0] >= 1e-5, "item %d: the inputs leave a leading pair %.3e apart" % (i, ranked[0] - lead[0])
            assert index[i] == at, "item %d: picked %d, the restatement %d (utilities %s)" % (i, index[i], at, u)
    if tag:
        _note(tag + "_pairwise_bleu", worst_f, F_TOL)
        _note(tag + "_utility_rel", worst_u, 1e-6)
    assert worst_f <= F_TOL and worst_u <= 1e-6, (worst_f, worst_u)


def test_consensus_under_bleu_against_the_restatement():
    from case_rg_amd.evaluation import consensus
    pools, valid, weights = consensus_pools()
    B, N, T = len(pools), len(pools[0]), 40
    lists = [[p if p else [UNK] for p in pool] for pool in pools]
    cand = _dev(np.stack([_raw_rows(p, T) for p in pools]))
    with Calls() as c:
        plain = consensus(cand, SPECIALS, metric="bleu")
        masked = consensus(cand, SPECIALS, valid=_dev(valid), metric="bleu")
        weighted = consensus(cand, SPECIALS, valid=_dev(valid), weights=_dev(weights), metric="bleu")
    assert c.count("case_ngram_counts") == 3 and c.count("case_bleu_scores") == 3 and c.count("case_consensus_pick") == 3 and c.count("case_lcs_pairs") == 0
    assert set(plain) == {"answer", "consensus_index", "consensus_utility", "pairwise_bleu"}
    assert plain["pairwise_bleu"].shape == (B, N, N) and plain["pairwise_bleu"].dtype == torch.float32
    check_bleu_consensus(plain, lists, tag="pick_uniform")
    check_bleu_consensus(masked, lists, valid=valid.tolist(), tag="pick_masked")
    check_bleu_consensus(weighted, lists, weights=weights.tolist(), valid=valid.tolist(), tag="pick_weighted")
    u = plain["consensus_utility"]
    assert int(plain["consensus_index"][0]) == 2 and float(u[0, 2]) == float(u[0, 3]) == float(u[0, 5])
    assert int(plain["consensus_index"][1]) == 2 and int(weighted["consensus_index"][1]) == 0, "the weights must move the pick"
    idx = to_np(masked["consensus_index"])
    assert all(valid[i, idx[i]] for i in range(B) if valid[i].any()) and idx[4] == 0
    assert to_np(torch.isinf(masked["consensus_utility"])).tolist() == (~valid).tolist()
    for res in (plain, masked, weighted):
        assert torch.equal(res["answer"], cand[torch.arange(B, device="cuda"), res["consensus_index"]])
    # the self term of add-one BLEU-4 is 1 only from 4 tokens on: a one-token candidate against itself gives (1/2)^(3/4)
    assert abs(float(plain["pairwise_bleu"][0, 6, 6]) - 0.5 ** 0.75) <= F_TOL and abs(float(plain["pairwise_bleu"][0, 2, 2]) - 1.0) <= F_TOL


def test_consensus_under_rouge_l_is_unchanged():
    """``metric="rouge_l"`` and no ``metric`` at all: the same launches, the same keys, the same bits."""
    from case_rg_amd.evaluation import consensus
    pools, valid, weights = consensus_pools()
    cand = _dev(np.stack([_raw_rows(p, 40) for p in pools]))
    with Calls() as c:
        default = consensus(cand, SPECIALS, valid=_dev(valid), weights=_dev(weights))
    with Calls() as named:
        given = consensus(cand, SPECIALS, valid=_dev(valid), weights=_dev(weights), metric="rouge_l")
    assert c.calls == named.calls == {"case_sentence_compact": 1, "case_lcs_pairs": 1, "case_consensus_pick": 1}
    assert list(default) == list(given) == ["answer", "consensus_index", "consensus_utility", "pairwise_f"]
    for key in default:
        assert default[key].dtype == given[key].dtype and torch.equal(default[key], given[key]), key


@pytest.mark.parametrize("name", ["sample_case", "sample_masque"])
def test_do_consensus_under_bleu_over_a_sample_pool(ns, name):
    m, b = sample_cases.build(ns, torch.device("cuda"), name)
    m.eval()
    B, T, N = sample_cases.ITEMS, sample_cases.T, 6
    rows = torch.arange(B, device="cuda")
    with torch.no_grad():
        plain = m.do_sample(dict(b), num_samples=N, seed=7)
        with Calls() as c:
            out = m.do_consensus(dict(b), pool="sample", metric="bleu", seed=7, num_samples=N)
        assert c.count("case_ngram_counts") == 1 and c.count("case_bleu_scores") == 1 and c.count("case_consensus_pick") == 1
        assert c.count("case_lcs_pairs") == 0 and c.sampled == T, c.calls
        assert set(out) == {"rank", "samples", "sample_probs", "sample_scores", "answer", "consensus_index", "consensus_utility", "pairwise_bleu"}
        assert torch.equal(out["samples"], plain["samples"]), "the pool is do_sample's at the same seed"
        assert torch.equal(out["answer"], out["samples"][rows, out["consensus_index"]])
        lists = m.to_sentence(None, out["samples"].reshape(B * N, T))
        check_bleu_consensus(out, [lists[i * N:(i + 1) * N] for i in range(B)], tag=name + "_samples", picks=False)
        # the attribute is the default of the keyword, and of method="consensus"
        m.consensus_metric = "bleu"
        m.sampling = dict(num_samples=1, temperature=1.0, top_k=0, top_p=1.0, seed=7)
        m.consensus_samples = N
        routed = m(dict(b), method="consensus")
        assert torch.equal(routed["pairwise_bleu"], out["pairwise_bleu"]) and torch.equal(routed["answer"], out["answer"])
        with Calls() as c:
            rouge = m.do_consensus(dict(b), metric="rouge_l", seed=7, num_samples=N)
        assert "pairwise_f" in rouge and c.count("case_ngram_counts") == 0 and c.count("case_lcs_pairs") == 1


def test_consensus_under_bleu_replays_from_a_captured_graph():
    """Nothing in consensus(metric="bleu") waits for the host: captured once, the replay on new candidates written into the same buffer is
    the eager call on them."""
    from case_rg_amd.evaluation import consensus
    pools, _, _ = consensus_pools()
    first = _dev(np.stack([_raw_rows(p, 40) for p in pools]))
    second = _dev(np.stack([_raw_rows(p[::-1], 40) for p in pools[::-1]]))
    keys = ("answer", "consensus_index", "consensus_utility", "pairwise_bleu")
    eager = {k: v.clone() for k, v in consensus(second, SPECIALS, metric="bleu").items()}
    buf = first.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        consensus(buf, SPECIALS, metric="bleu")  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph, static = torch.cuda.CUDAGraph(), {}
    with torch.cuda.graph(graph), Calls() as c:
        static.update(consensus(buf, SPECIALS, metric="bleu"))
    assert c.count("case_ngram_counts") == 1 and c.count("case_bleu_scores") == 1 and c.count("case_consensus_pick") == 1
    buf.copy_(second)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(static[k], eager[k]), "the replay differs from the eager call in %s" % k
    assert not torch.equal(eager["pairwise_bleu"], consensus(first, SPECIALS, metric="bleu")["pairwise_bleu"]), "the two candidate sets must differ"
    del graph


# ---------------------------------------------------------------------------------------------
# 6. the trainer's BLEU
# ---------------------------------------------------------------------------------------------
def test_trainer_evaluate_bleu_is_the_host_number(ns):
    """Four items in batches of 3 and 1.  Beside ``response`` the dataset carries ``truths`` [4, 3, T']: the response, an all-PAD row (absent)
    and, for two items, the model's own greedy answer (so that the number is well above 0)."""
    from case_rg_amd.common.Utils import remove_duplicate
    from case_rg_amd.evaluation import eval_bleu
    m, b = sample_cases.build(ns, torch.device("cuda"), "sample_case")
    m.eval()
    data = {k: v.cpu() for k, v in b.items()}
    with torch.no_grad():
        greedy = m(dict(b), method="test")["answer"].cpu()
    truths = torch.zeros(4, 3, max(greedy.shape[1], data["response"].shape[1]), dtype=torch.int64)
    truths[:, 0, :data["response"].shape[1]] = data["response"]
    truths[:2, 2, :greedy.shape[1]] = greedy[:2]
    data["truths"] = truths
    trainer = ns.CumulativeTrainer(m, None, None, None, 1)
    trainer.model.train()
    ds = cases._ListDataset(data)
    for references, dedup in (("response", False), ("truths", False), ("truths", True)):
        got = trainer.evaluate_bleu(ds, cases._collate, 3, method="test", references=references, remove_duplicates=dedup)
        assert trainer.model.training, "the mode must be restored"
        run, ref = [], []
        for batch, out in trainer.predict("test", ds, cases._collate, 3):
            sents = [list(s) for s in m.to_sentence(batch, out["answer"])]
            if dedup:
                remove_duplicate(sents)
            run += sents
            rows = batch[references] if batch[references].dim() == 3 else batch[references].unsqueeze(1)
            for item in rows:
                ref.append([s for s, raw in zip(m.to_sentence(batch, item), item.tolist()) if any(raw)])
        trainer.model.train()
        want = eval_bleu(run, ref)
        print("evaluate_bleu(%s, dedup %s): %s, host %.2f" % (references, dedup, got, want))
        assert set(got) == {"bleu", "items"} and got["items"] == 4
        assert "%.2f" % got["bleu"] == "%.2f" % want
        if references == "truths" and not dedup:
            assert got["bleu"] > 0.0
    trainer.close()
