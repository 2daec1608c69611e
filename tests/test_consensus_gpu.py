"""Consensus answer selection on the MI355X: K30 (``case_lcs_pairs``) against the reference-generated ROUGE-L fixture, at the 64-bit word
boundaries of its match masks and over more hypotheses than the device holds at once; K31 (``case_consensus_pick``) against the pure-Python
restatement of tests/test_consensus_cpu.py; ``do_consensus`` of both task models over sample and beam pools; stream capture; the trainer's
``evaluate_rouge`` against ``predict`` + ``to_sentence`` + the host's ``eval_rouge_l``.

F values are compared at 1.2e-7 absolute: one f32 rounding of a value in [0, 1] (2^-24 = 6e-8 relative to at most 1, twice that as the
bound); LCS lengths and picks exactly; utilities at 1e-6 relative (f32 sums of at most 64 terms against f64).
Measured maxima go to the session's parity ledger (``helpers.record_error``, case "consensus"); profiles/consensus_parity.json keeps a copy."""
import math
import types

import numpy as np
import pytest
import torch

import cases
import sample_cases
from helpers import Calls, load_golden, record_error, to_np
from test_consensus_cpu import restated_pick

pytestmark = pytest.mark.gpu

F_TOL = 1.2e-7
PAD, BOS, EOS, UNK, FIRST = 0, 1, 2, 3, 4  # the ids of the kernel-level tests
SPECIALS = (BOS, PAD, EOS, UNK)


@pytest.fixture(scope="module")
def ns():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.float32)
    case_rg_amd.set_dropout(False)
    return case_rg_amd.namespace()


def _note(key, value, tol):
    record_error("consensus", "fp32", key, value, tol)


def _host():
    from case_rg_amd.evaluation import eval_rouge_l, lcs_length, rouge_l
    return lcs_length, rouge_l, eval_rouge_l


def _host_f(hyp, ref):
    """(lcs, F) of the host for two id lists; an empty side gives (0, 0) as the kernel defines it."""
    lcs_length, rouge_l, _ = _host()
    if len(hyp) == 0 or len(ref) == 0:
        return 0, 0.0
    return lcs_length(hyp, ref), rouge_l(hyp, ref)[0]


def _raw_rows(lists, T):
    """Token lists -> raw decoder-style rows int64 [n, T]: BOS, the tokens, EOS, then ids that must be ignored; a PAD inside the sentence."""
    out = np.zeros((len(lists), T), dtype=np.int64)
    for i, toks in enumerate(lists):
        row = [BOS] + list(toks[:len(toks) // 2]) + [PAD] + list(toks[len(toks) // 2:]) + [EOS, FIRST + 1, FIRST + 2]
        assert len(row) <= T + 3
        row = row[:T]
        out[i, :len(row)] = row
    return out


def _packed(lists, T):
    """Token lists -> (front-packed int64 [n, T] with garbage behind the length, lengths int32 [n])."""
    ids = np.full((len(lists), T), FIRST + 7, dtype=np.int64)
    for i, toks in enumerate(lists):
        ids[i, :len(toks)] = toks
    return ids, np.array([len(t) for t in lists], dtype=np.int32)


def _dev(x):
    return torch.as_tensor(x).cuda()


# ---------------------------------------------------------------------------------------------
# 1. K30 against the reference-generated fixture
# ---------------------------------------------------------------------------------------------
def _fixture_sentences():
    """The hypotheses and ground truths of ``cases.case_rouge_l``, by running that case with a namespace that records what it is given."""
    _, rouge_l, _ = _host()
    seen = {}

    def capture(hyps, refs):
        seen["hyps"], seen["refs"] = hyps, refs
        return 0.0

    cases.case_rouge_l(types.SimpleNamespace(rouge_l=rouge_l, eval_rouge_l=capture), None)
    return seen["hyps"], seen["refs"]


def test_rouge_l_ids_matches_the_reference_fixture():
    from case_rg_amd.evaluation import eval_rouge_l_ids, rouge_l_ids
    golden = load_golden("rouge_l")
    hyps, refs = _fixture_sentences()
    assert len(hyps) == 24 and max(len(r) for r in refs) <= 3
    vocab = {}
    to_ids = lambda s: [vocab.setdefault(w, FIRST + len(vocab)) for w in s.split(" ")]  # noqa: E731
    hyp_ids = [to_ids(h) for h in hyps]
    ref_ids = [[to_ids(t) for t in r] for r in refs]
    T = 2 + 3 + max(max(len(h) for h in hyp_ids), max(len(t) for r in ref_ids for t in r))
    hyp = _dev(_raw_rows(hyp_ids, T))
    cyc = _dev(np.stack([_raw_rows((r + r + r)[:3], T) for r in ref_ids]))  # the fixture's layout: the ground truths repeated to three
    out = rouge_l_ids(hyp, cyc, SPECIALS)
    assert out["lcs"].shape == (24, 1, 3) and out["f"].dtype == torch.float32 and out["ref_valid"].all()
    worst = {}
    for k, key in enumerate(("f", "p", "r")):
        got = to_np(out[key][:, 0].double())
        worst[key] = float(np.abs(got - golden["fpr"][:, :, k]).max())
        print("rouge_l fixture: max |%s - golden| = %.3e" % (key, worst[key]))
        _note("fixture_" + key, worst[key], F_TOL)
    for key, w in worst.items():
        assert w <= F_TOL, "%s differs from the reference's by %.3e" % (key, w)
    # the evaluation script's aggregate, with the ragged ground truths padded by all-PAD rows (absent)
    ragged = np.zeros((24, 3, T), dtype=np.int64)
    for i, r in enumerate(ref_ids):
        ragged[i, :len(r)] = _raw_rows(r, T)
    per_item = eval_rouge_l_ids(hyp, _dev(ragged), SPECIALS)
    assert per_item.dtype == torch.float64 and per_item.shape == (24,) and per_item.is_cuda
    assert round(float(per_item.mean()), 2) == float(golden["rouge_l_f1"][0]) == 33.88
    present = rouge_l_ids(hyp, _dev(ragged), SPECIALS)["ref_valid"]
    assert to_np(present).tolist() == [[k < len(r) for k in range(3)] for r in ref_ids]


def test_empty_hypothesis_is_unk_and_empty_reference_is_absent():
    from case_rg_amd.evaluation import eval_rouge_l_ids, rouge_l_ids
    hyp = _dev(np.array([[BOS, EOS, 9, 9], [PAD, PAD, PAD, PAD], [BOS, 9, 8, EOS]], dtype=np.int64))
    ref = _dev(np.array([[[UNK, 7, EOS, 0], [0, 0, 0, 0]], [[9, EOS, 0, 0], [UNK, EOS, 0, 0]], [[EOS, 9, 8, 0], [BOS, PAD, EOS, 9]]], dtype=np.int64))
    out = rouge_l_ids(hyp, ref, SPECIALS)
    assert to_np(out["ref_valid"]).tolist() == [[True, False], [True, True], [False, False]]
    assert to_np(out["lcs"][:, 0]).tolist() == [[1, 0], [0, 1], [0, 0]]
    _, rouge_l, _ = _host()
    assert abs(float(out["f"][0, 0, 0]) - rouge_l([UNK], [UNK, 7])[0]) <= F_TOL and float(out["p"][0, 0, 0]) == 1.0 and float(out["r"][0, 0, 0]) == 0.5
    best = to_np(eval_rouge_l_ids(hyp, ref, SPECIALS))
    assert abs(best[0] - 100 * rouge_l([UNK], [UNK, 7])[0]) <= 100 * F_TOL and abs(best[1] - 100 * rouge_l([UNK], [UNK])[0]) <= 100 * F_TOL
    assert best[2] == 0.0, "an item without a present reference scores 0"


# ---------------------------------------------------------------------------------------------
# 2. K30 at the word boundaries
# ---------------------------------------------------------------------------------------------
HYP_LENS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256)
REF_LENS = (0, 1, 64, 65, 300)
VOCABS = (1, 2, 12, 1000)


@pytest.fixture(scope="module")
def boundary_pool():
    """Per vocabulary: the hypotheses, the references and the host's (lcs, F) of every pair, computed once."""
    rs = np.random.RandomState(30)
    hyps = [[(rs.randint(0, v, n) + FIRST).tolist() for n in HYP_LENS] for v in VOCABS]
    refs = [[(rs.randint(0, v, n) + FIRST).tolist() for n in REF_LENS] for v in VOCABS]
    want = [[[_host_f(h, r) for r in refs[i]] for h in hyps[i]] for i in range(len(VOCABS))]
    return hyps, refs, want


@pytest.mark.parametrize("Ta", [64, 128, 256])
def test_lcs_pairs_at_the_word_boundaries(boundary_pool, Ta):
    """Every hypothesis length up to ``Ta`` (one, two and four 64-bit words per hypothesis) against every reference length, four vocabularies."""
    from case_rg_amd import ops
    hyps, refs, want = boundary_pool
    keep = [k for k, n in enumerate(HYP_LENS) if n <= Ta]
    a, a_len = zip(*[_packed([hyps[i][k] for k in keep], Ta) for i in range(len(VOCABS))])
    b, b_len = zip(*[_packed(refs[i], max(REF_LENS)) for i in range(len(VOCABS))])
    with Calls() as c:
        lcs, f = ops.lcs_pairs(_dev(np.stack(a)), _dev(np.stack(a_len)), _dev(np.stack(b)), _dev(np.stack(b_len)))
    assert c.count("case_lcs_pairs") == 1 and lcs.shape == (len(VOCABS), len(keep), len(REF_LENS)) and lcs.dtype == torch.int32
    lcs, f = to_np(lcs), to_np(f).astype(np.float64)
    worst = 0.0
    for i, v in enumerate(VOCABS):
        for j, k in enumerate(keep):
            for m, n in enumerate(REF_LENS):
                assert lcs[i, j, m] == want[i][k][m][0], "vocabulary %d, lengths %d x %d: lcs %d, host %d" % (v, HYP_LENS[k], n, lcs[i, j, m], want[i][k][m][0])
                worst = max(worst, abs(f[i, j, m] - want[i][k][m][1]))
    print("Ta %d: max |f - host| = %.3e" % (Ta, worst))
    _note("boundaries_f_Ta%d" % Ta, worst, F_TOL)
    assert worst <= F_TOL


def test_lcs_pairs_carry_id_width_and_a_partly_filled_workgroup():
    from case_rg_amd import ops
    # one word repeated: every step's addition carries through every 64-bit word
    a, a_len = _packed([[FIRST] * 130], 256)
    b, b_len = _packed([[FIRST] * 200], 200)
    lcs, f = ops.lcs_pairs(_dev(a[None]), _dev(a_len[None]), _dev(b[None]), _dev(b_len[None]))
    assert int(lcs[0, 0, 0]) == 130 and abs(float(f[0, 0, 0]) - _host_f([1] * 130, [1] * 200)[1]) <= F_TOL
    # ids are compared on 32 bits: a difference of 2^16 or 2^24 is a difference
    big = 2 ** 31 - 1
    hyp = [[7], [7 + 65536], [7 + 2 ** 24], [7, 7 + 65536, 7 + 2 ** 24, big]]
    ref = [[7], [7 + 65536], [7 + 2 ** 24], [big, big - 65536], [7 + 2 ** 24, 7 + 65536, 7]]
    a, a_len = _packed(hyp, 4)
    b, b_len = _packed(ref, 3)
    lcs, _ = ops.lcs_pairs(_dev(a[None]), _dev(a_len[None]), _dev(b[None]), _dev(b_len[None]))
    assert to_np(lcs[0]).tolist() == [[1, 0, 0, 0, 1], [0, 1, 0, 0, 1], [0, 0, 1, 0, 1], [1, 1, 1, 1, 1]]
    # (B, N) = (3, 5): 15 hypotheses, the fourth workgroup holds three; M = 2 references per item
    rs = np.random.RandomState(35)
    hyps = [[(rs.randint(0, 6, rs.randint(0, 70)) + FIRST).tolist() for _ in range(5)] for _ in range(3)]
    refs = [[(rs.randint(0, 6, rs.randint(0, 90)) + FIRST).tolist() for _ in range(2)] for _ in range(3)]
    a, a_len = zip(*[_packed(h, 70) for h in hyps])
    b, b_len = zip(*[_packed(r, 90) for r in refs])
    lcs, f = ops.lcs_pairs(_dev(np.stack(a)), _dev(np.stack(a_len)), _dev(np.stack(b)), _dev(np.stack(b_len)))
    for i in range(3):
        for n in range(5):
            for m in range(2):
                want = _host_f(hyps[i][n], refs[i][m])
                assert int(lcs[i, n, m]) == want[0] and abs(float(f[i, n, m]) - want[1]) <= F_TOL, (i, n, m)


# ---------------------------------------------------------------------------------------------
# 3. more waves than the device holds at once
# ---------------------------------------------------------------------------------------------
def test_lcs_pairs_self_pool_of_4112_hypotheses():
    from case_rg_amd import ops
    B, N, T = 257, 16, 64
    rs = np.random.RandomState(36)
    ids = rs.randint(0, 9, (B, N, T)) + FIRST
    lens = rs.randint(0, T + 1, (B, N)).astype(np.int32)
    lens[0, :4] = (0, 1, 63, 64)
    a, n = _dev(ids), _dev(lens)
    lcs, f = ops.lcs_pairs(a, n, a, n)
    lcs = to_np(lcs)
    assert np.array_equal(lcs, lcs.transpose(0, 2, 1)), "the LCS length is symmetric"
    assert np.array_equal(lcs[:, np.arange(N), np.arange(N)], lens), "a sequence against itself"
    f = to_np(f).astype(np.float64)
    worst = 0.0
    for _ in range(500):
        i, x, y = rs.randint(0, B), rs.randint(0, N), rs.randint(0, N)
        want = _host_f(ids[i, x, :lens[i, x]].tolist(), ids[i, y, :lens[i, y]].tolist())
        assert lcs[i, x, y] == want[0], (i, x, y, lcs[i, x, y], want[0])
        worst = max(worst, abs(f[i, x, y] - want[1]))
    _note("self_pool_f", worst, F_TOL)
    assert worst <= F_TOL


# ---------------------------------------------------------------------------------------------
# 4. K31 and ``consensus`` against the restatement
# ---------------------------------------------------------------------------------------------
def _check_against_restatement(res, pools, weights=None, valid=None, tag=""):
    """``res``: consensus(...) over ``pools`` (per item N token lists, [UNK] for an empty one).  Pairwise F at F_TOL, utilities at 1e-6
    relative, -inf exactly where invalid; the pick is the first maximum of the returned utilities, and the restatement's pick wherever
    its best utility leads the runner-up by more than 1e-5 (an f32 and an f64 sum may order a closer pair differently: there the pick
    must be one of the close ones)."""
    worst_f, worst_u = 0.0, 0.0
    util, index, pf = to_np(res["consensus_utility"]).astype(np.float64), to_np(res["consensus_index"]), to_np(res["pairwise_f"]).astype(np.float64)
    for i, pool in enumerate(pools):
        w = None if weights is None else weights[i]
        v = None if valid is None else valid[i]
        u, at, f = restated_pick(pool, w, v)
        worst_f = max(worst_f, float(np.abs(pf[i] - np.array(f)).max()))
        for n, un in enumerate(u):
            if un == -math.inf:
                assert util[i, n] == -math.inf, "item %d candidate %d is invalid and must read -inf" % (i, n)
            else:
                worst_u = max(worst_u, abs(util[i, n] - un) / max(abs(un), 1e-30))
        assert index[i] == int(np.argmax(util[i])), "item %d: index %d is not the first maximum of %s" % (i, index[i], util[i])
        ranked = sorted((x for x in u if x > -math.inf), reverse=True)
        if len(ranked) < 2 or ranked[0] - ranked[1] > 1e-5:
            assert index[i] == at, "item %d: picked %d, the restatement %d (utilities %s)" % (i, index[i], at, u)
        else:
            assert u[index[i]] >= ranked[0] - 1e-5 and (v is None or v[index[i]])
    if tag:
        _note(tag + "_pairwise_f", worst_f, F_TOL)
        _note(tag + "_utility_rel", worst_u, 1e-6)
    assert worst_f <= F_TOL and worst_u <= 1e-6, (worst_f, worst_u)


def test_consensus_pick_against_the_restatement():
    from case_rg_amd.evaluation import consensus
    rs = np.random.RandomState(31)
    B, N, T = 9, 7, 40
    pools = [[(rs.randint(0, 8, rs.randint(1, 30)) + FIRST).tolist() for _ in range(N)] for _ in range(B)]
    q, z, w5 = [FIRST, FIRST + 1, FIRST + 2, FIRST + 3], [100, 101, 102], [200, 201]
    pools[0] = [z, [100, 102], q, q, w5, q, [201]]     # a planted exact tie between 2, 3 and 5, well ahead of the rest
    pools[1] = [w5, z, q, q, q, [100], [200]]          # the same three-fold copy: weights will move the pick to 0
    pools[2][4] = []                                   # an empty candidate counts as [UNK]
    valid = np.ones((B, N), dtype=bool)
    valid[3, [0, 5]] = False
    valid[4] = False                                   # an item without a valid candidate
    valid[0, 6] = False
    weights = rs.uniform(0.1, 1.0, (B, N)).astype(np.float32)
    weights[1] = (50.0, 1e-3, 1.0, 1.0, 1.0, 1e-3, 1e-3)
    raw = np.stack([_raw_rows(p, T) for p in pools])
    lists = [[p if p else [UNK] for p in pool] for pool in pools]
    cand = _dev(raw)
    with Calls() as c:
        plain = consensus(cand, SPECIALS)
        masked = consensus(cand, SPECIALS, valid=_dev(valid))
        weighted = consensus(cand, SPECIALS, valid=_dev(valid), weights=_dev(weights))
    assert c.count("case_lcs_pairs") == 3 and c.count("case_consensus_pick") == 3
    assert set(plain) == {"answer", "consensus_index", "consensus_utility", "pairwise_f"}
    assert plain["consensus_index"].dtype == torch.int64 and plain["consensus_utility"].shape == (B, N) and plain["pairwise_f"].shape == (B, N, N)
    _check_against_restatement(plain, lists, tag="pick_uniform")
    _check_against_restatement(masked, lists, valid=valid.tolist(), tag="pick_masked")
    _check_against_restatement(weighted, lists, weights=weights.tolist(), valid=valid.tolist(), tag="pick_weighted")
    # the planted tie: equal bits, the lowest index
    u = plain["consensus_utility"]
    assert int(plain["consensus_index"][0]) == 2 and float(u[0, 2]) == float(u[0, 3]) == float(u[0, 5])
    assert int(plain["consensus_index"][1]) == 2 and int(weighted["consensus_index"][1]) == 0, "the weights must move the pick"
    assert restated_pick(lists[1], weights[1].tolist(), valid[1].tolist())[1] == 0
    # invalid candidates: -inf, never picked; nothing valid: index 0
    idx = to_np(masked["consensus_index"])
    assert all(valid[i, idx[i]] for i in range(B) if valid[i].any()) and idx[4] == 0
    assert torch.isinf(masked["consensus_utility"][4]).all() and (masked["consensus_utility"][4] < 0).all()
    assert to_np(torch.isinf(masked["consensus_utility"])).tolist() == (~valid).tolist()
    # the answer is the raw row of the pick, bit for bit
    for res in (plain, masked, weighted):
        assert torch.equal(res["answer"], cand[torch.arange(B, device="cuda"), res["consensus_index"]])


def test_consensus_pick_on_a_full_wave_and_given_utilities():
    """N = 64 fills the wave; f is handed to K31 directly: the argmax over all 64 lanes, ties to the lowest index, a zero weight sum."""
    from case_rg_amd import ops
    B, N, T = 5, 64, 3
    g = torch.Generator().manual_seed(33)
    f = torch.rand(B, N, N, generator=g)
    f[1] = 0.5                      # every utility equal: index 0
    f[2, 63] = 2.0                  # the last lane wins
    f[3, 40] = 2.0
    f[3, 17] = 2.0                  # two equal rows: the lower index
    cand = torch.arange(B * N * T).view(B, N, T)
    w = torch.rand(B, N, generator=g) + 0.1
    w[4] = 0.0                      # weights that sum to 0: every utility 0, index 0
    util, index, answer = ops.consensus_pick(f.cuda(), w.cuda(), None, cand.cuda())
    want = (f.double() * w.double()[:, None, :]).sum(-1) / w.double().sum(-1, keepdim=True)
    assert to_np(index).tolist() == [int(want[0].argmax()), 0, 63, 17, 0]
    rel = ((util[:4].cpu().double() - want[:4]).abs() / want[:4]).max()
    assert float(rel) <= 1e-6 and (util[4] == 0).all()
    assert torch.equal(answer.cpu(), cand[torch.arange(B), index.cpu()])
    with pytest.raises(ValueError, match="up to 64 candidates"):
        ops.consensus_pick(torch.zeros(1, 65, 65).cuda(), None, None, torch.zeros(1, 65, 2, dtype=torch.int64).cuda())


# ---------------------------------------------------------------------------------------------
# 5. the task models
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sample_case", "sample_masque"])
def test_do_consensus_over_sample_and_beam_pools(ns, name):
    m, b = sample_cases.build(ns, torch.device("cuda"), name)
    m.eval()
    B, T, N = sample_cases.ITEMS, sample_cases.T, 6
    rows = torch.arange(B, device="cuda")
    fields = ("answer", "consensus_index", "consensus_utility", "pairwise_f")
    with torch.no_grad():
        plain = m.do_sample(dict(b), num_samples=N, seed=21)
        greedy = m(dict(b), method="test")
        with Calls() as c:
            out = m.do_consensus(dict(b), num_samples=N, seed=21)
        assert c.count("case_lcs_pairs") == 1 and c.count("case_consensus_pick") == 1 and c.scored == 0 and c.sampled == T, c.calls
        assert set(out) == {"rank", "samples", "sample_probs", "sample_scores"} | set(fields)
        for key in ("samples", "sample_probs", "sample_scores", "rank"):
            assert torch.equal(out[key], plain[key]), "%s differs from do_sample's at the same seed" % key
        assert out["samples"].shape == (B, N, T) and out["consensus_utility"].shape == (B, N) and out["pairwise_f"].shape == (B, N, N)
        assert torch.equal(out["answer"], out["samples"][rows, out["consensus_index"]])
        lists = m.to_sentence(None, out["samples"].reshape(B * N, T))
        pools = [lists[i * N:(i + 1) * N] for i in range(B)]
        _check_against_restatement(out, pools, tag=name + "_samples")
        print("%s: picks %s, utilities %s" % (name, out["consensus_index"].tolist(), np.array2string(to_np(out["consensus_utility"]), precision=3)))
        # forward(method="consensus") = do_consensus with the model's defaults
        m.sampling = dict(num_samples=1, temperature=1.0, top_k=0, top_p=1.0, seed=21)
        m.consensus_samples = N
        routed = m(dict(b), method="consensus")
        for key in fields + ("samples",):
            assert torch.equal(routed[key], out[key]), "method='consensus' differs in %s" % key
        # a posterior over the samples as weights
        length = out["samples"].ne(0).sum(-1).clamp_min(1)
        weights = torch.exp(-length * out["sample_scores"])
        weighted = m.do_consensus(dict(b), num_samples=N, seed=21, weights=weights)
        _check_against_restatement(weighted, pools, weights=to_np(weights).astype(np.float64).tolist())
        # explicit candidates: no decoding, the encode stages give the rank
        with Calls() as c:
            given = m.do_consensus(dict(b), candidates=out["samples"])
        assert c.sampled == 0 and c.count("case_pointer_head_decode") == 0 and c.count("case_consensus_pick") == 1
        assert set(given) == {"rank"} | set(fields) and torch.equal(given["rank"], greedy["rank"])
        for key in fields:
            assert torch.equal(given[key], out[key]), key
        # the beam pool at width 3: empty slots are invalid, the pick is one of beam_answers
        beam = m.do_beam(dict(b), width=3)
        with Calls() as c:
            picked = m.do_consensus(dict(b), pool="beam", width=3)
        assert c.count("case_lcs_pairs") == 1 and c.count("case_consensus_pick") == 1 and c.scored == 0
        assert set(picked) == {"rank", "beam_score", "beam_answers", "beam_scores"} | set(fields)
        assert torch.equal(picked["beam_answers"], beam["beam_answers"]) and torch.equal(picked["beam_scores"], beam["beam_scores"])
        finite = torch.isfinite(picked["beam_scores"])
        assert torch.equal(torch.isinf(picked["consensus_utility"]), ~finite)
        assert finite[rows, picked["consensus_index"]].all()
        assert torch.equal(picked["answer"], picked["beam_answers"][rows, picked["consensus_index"]])
        blists = m.to_sentence(None, picked["beam_answers"].reshape(B * 3, T))
        _check_against_restatement(picked, [blists[i * 3:(i + 1) * 3] for i in range(B)], valid=to_np(finite).tolist())
        # a masked slot: the caller's mask is combined with the pool's
        mask = torch.ones(B, 3, dtype=torch.bool, device="cuda")
        mask[:, 0] = False
        masked = m.do_consensus(dict(b), pool="beam", width=3, valid=mask)
        assert torch.isinf(masked["consensus_utility"][:, 0]).all()
        with pytest.raises(ValueError, match="pools of up to 64"):
            m.do_consensus(dict(b), candidates=torch.zeros(B, 65, T, dtype=torch.int64, device="cuda"))


# ---------------------------------------------------------------------------------------------
# 6. stream capture
# ---------------------------------------------------------------------------------------------
def test_consensus_pass_replays_from_a_captured_graph(ns):
    """With an integer seed nothing in the pass waits for the host: it captures into one graph whose replay is the eager pass, bit for bit."""
    from case_rg_amd.utils import fill_params, make_vocab, synth_batch
    V_, T, N = 200, 12, 4
    v2i, i2v = make_vocab(V_)
    model = fill_params(ns.CaSE(4, T, i2v, v2i, 32), 153, gain=3.0).cuda().eval()
    b = {k: v.cuda() for k, v in synth_batch(4, 3, 12, 8, 6, V_, seed=152, model="case").items()}
    keys = ("answer", "samples", "sample_probs", "sample_scores", "consensus_index", "consensus_utility", "pairwise_f", "rank")

    def run():
        return model.do_consensus(dict(b), num_samples=N, seed=5, top_k=20, temperature=0.9)

    with torch.no_grad():
        eager = {k: v.clone() for k, v in run().items()}
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()  # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        graph, static = torch.cuda.CUDAGraph(), {}
        with torch.cuda.graph(graph), Calls() as c:
            static.update(run())
        assert c.sampled == T and c.count("case_lcs_pairs") == 1 and c.count("case_consensus_pick") == 1
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            for k in keys:
                assert torch.equal(static[k], eager[k]), "the replay differs from the eager pass in %s" % k
        del graph
    assert len({tuple(r) for r in eager["samples"][0].tolist()}) > 1, "the pool of item 0 holds one distinct sample only"


# ---------------------------------------------------------------------------------------------
# 7. the trainer's ROUGE-L
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["test", "consensus"])
def test_trainer_evaluate_rouge_is_the_host_number(ns, method):
    """Four items in batches of 3 and 1.  Beside ``response`` the dataset carries ``truths`` [4, 3, T']: the response, an all-PAD row (absent)
    and, for two items, the model's own greedy answer."""
    _, _, eval_rouge_l = _host()
    m, b = sample_cases.build(ns, torch.device("cuda"), "sample_case")
    m.eval()
    m.sampling = dict(num_samples=1, temperature=1.0, top_k=0, top_p=1.0, seed=9)
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
    for references in ("response", "truths"):
        got = trainer.evaluate_rouge(ds, cases._collate, 3, method=method, references=references)
        assert trainer.model.training, "the mode must be restored"
        run, ref = [], []
        for batch, out in trainer.predict(method, ds, cases._collate, 3):
            run += [" ".join(s) for s in m.to_sentence(batch, out["answer"])]
            rows = batch[references] if batch[references].dim() == 3 else batch[references].unsqueeze(1)
            for item in rows:
                ref.append([" ".join(s) for s, raw in zip(m.to_sentence(batch, item), item.tolist()) if any(raw)])
        trainer.model.train()
        want = eval_rouge_l(run, ref)
        print("evaluate_rouge(%s, %s): %s, host %.2f" % (method, references, got, want))
        assert set(got) == {"rouge_l", "items"} and got["items"] == 4
        assert "%.2f" % got["rouge_l"] == "%.2f" % want
        if references == "truths":
            assert got["rouge_l"] > 0.0
    trainer.close()
