"""TREC ranking metrics, CPU side: the host form ``evaluation.trec`` against worked examples derived by hand, against an independent
restatement (``restated_row`` below: ``sorted`` on (-score, reversed key) and naive ``Fraction`` sums) on seeded random runs, the file
parsers and ``run_lines`` round trip, and the argument checks that need no GPU.  tests/test_rank_gpu.py holds K36 against this restatement.

``pytrec_eval`` is not available where the fixtures are built, so no number here comes from running the reference's ``Eval_Trec.py``; the
pins are the hand-derived values below, which follow trec_eval's definitions as ``evaluation/trec.py`` states them.

WORKED EXAMPLES (L = log2).

q1, graded, with an unretrieved relevant document and a tie resolved by docid.  Run: d1 0.9, d2 0.5, d3 0.5, d4 0.1.  Judgements: d1 0,
d2 1, d3 2, d4 0, d8 -1, d9 3 (d8 and d9 were not retrieved).  Rank order: d1, then the tie at 0.5 with the larger docid first: d3, d2,
then d4.  Grades in rank order 0, 2, 1, 0; num_rel = 3 (d2, d3, d9; d8's negative grade counts as 0).
    map        = (1/3) (1/2 + 2/3) = 7/18
    recall_k   = 2/3 for every k (4 retrieved, all cutoffs >= 5)
    recip_rank = 1/2,  P_1 = 0
    ndcg       = (2 / L(3) + 1 / L(4)) / (3 / L(2) + 2 / L(3) + 1 / L(4)) = (2 / L(3) + 1/2) / (7/2 + 2 / L(3))
  With the tie resolved the other way (d2 before d3) map would still be 7/18, but ndcg's numerator would be 1 / L(3) + 2 / L(4): the test
  checks that the two differ (by (1 / L(3) - 1/2) / (7/2 + 2 / L(3)) = 0.0275).

q2, no relevant document.  Run: d1 1.0, d2 2.0.  Judgements: d1 0, d5 -2.  num_rel = 0: every metric is 0 and the query is counted.

q3, binary, seven retrieved documents d1 .. d7 with scores 7 .. 1, relevant at ranks 1, 6 and 7, num_rel = 3.
    map        = (1/3) (1/1 + 2/6 + 3/7) = (1/3) (74/42) = 37/63
    recall_5   = 1/3,  recall_10 = ... = recall_1000 = 3/3 = 1
    recip_rank = 1,  P_1 = 1
    ndcg       = (1 + 1 / L(7) + 1 / L(8)) / (1 + 1 / L(3) + 1 / L(4)) = (4/3 + 1 / L(7)) / (3/2 + 1 / L(3))

The corpus means over q1, q2, q3:  map = (7/18 + 0 + 37/63) / 3 = (49/126 + 74/126) / 3 = 41/126,  recall_5 = (2/3 + 0 + 1/3) / 3 = 1/3,
recip_rank = 1/2,  P_1 = 1/3."""
import math
import os
import random
from fractions import Fraction

import pytest

CUTOFFS = (5, 10, 15, 20, 30, 100, 200, 500, 1000)
NAMES = ("map", "ndcg") + tuple("recall_%d" % k for k in CUTOFFS) + ("recip_rank", "P_1")
EXACT = tuple(n for n in NAMES if n not in ("map", "ndcg"))
L = math.log2

RUN = {"q1": {"d1": 0.9, "d2": 0.5, "d3": 0.5, "d4": 0.1}, "q2": {"d1": 1.0, "d2": 2.0},
       "q3": {"d%d" % i: float(8 - i) for i in range(1, 8)}, "q4": {"d1": 1.0}}
QREL = {"q1": {"d1": 0, "d2": 1, "d3": 2, "d4": 0, "d8": -1, "d9": 3}, "q2": {"d1": 0, "d5": -2},
        "q3": {"d1": 1, "d2": 0, "d6": 1, "d7": 1}, "q5": {"d1": 1}}


# ---------------------------------------------------------------------------------------------
# the restatement (shared with tests/test_rank_gpu.py)
# ---------------------------------------------------------------------------------------------
def restated_row(scores, keys, rel, valid=None, extra=()):
    """One query: scores, integer tie keys and grades per column, an optional retrieved mask, the grades of judged but unretrieved
    documents -> (order: the columns in rank order, -1 behind the retrieved ones; {metric: f64}; num_rel)."""
    P = len(scores)
    cols = [c for c in range(P) if valid is None or valid[c]]
    canon = lambda x: -math.inf if x != x else float(x)  # noqa: E731
    ranked = sorted(cols, key=lambda c: (-canon(scores[c]), -int(keys[c]), c))
    gains = [max(int(rel[c]), 0) for c in ranked]
    flags = [g >= 1 for g in gains]
    judged = [g for g in gains if g >= 1] + [int(g) for g in extra if g >= 1]
    num_rel, n = len(judged), len(ranked)
    order = ranked + [-1] * (P - n)
    if num_rel == 0:
        return order, {name: 0.0 for name in NAMES}, 0
    out = {"map": float(sum(Fraction(sum(flags[:i]), i) for i in range(1, n + 1) if flags[i - 1]) / num_rel)}
    dcg = sum(g / L(i + 1) for i, g in enumerate(gains, 1))
    idcg = sum(g / L(i + 1) for i, g in enumerate(sorted(judged, reverse=True), 1))
    out["ndcg"] = dcg / idcg
    for k in CUTOFFS:
        out["recall_%d" % k] = float(Fraction(sum(flags[:min(k, n)]), num_rel))
    out["recip_rank"] = float(Fraction(1, flags.index(True) + 1)) if any(flags) else 0.0
    out["P_1"] = 1.0 if flags and flags[0] else 0.0
    return order, out, num_rel


SCORE_VALUES = (-2.5, -1.0, -0.0, 0.0, 0.25, 0.5, 1.0, 3.0)  # a handful, exact in f32: ties are common


def random_row(rs, P, R, keys=True):
    """A seeded query of P slots: (scores, keys (a permutation of distinct integers, or the columns), grades -1 .. 4, extra grades)."""
    scores = [rs.choice(SCORE_VALUES) for _ in range(P)]
    ks = rs.sample(range(-P, 2 * P), P) if keys else list(range(P))
    rel = [rs.choice((-1, 0, 0, 0, 1, 1, 2, 3, 4)) for _ in range(P)]
    extra = [rs.choice((0, 0, 1, 2, 4, -3)) for _ in range(R)]
    return scores, ks, rel, extra


# ---------------------------------------------------------------------------------------------
# 1. worked examples
# ---------------------------------------------------------------------------------------------
def test_host_form_on_the_worked_examples():
    from case_rg_amd.evaluation import rank_metrics
    from case_rg_amd.evaluation.trec import mean_metrics
    got = rank_metrics(RUN, QREL)
    assert set(got) == {"q1", "q2", "q3"}, "the queries present in both"
    assert all(set(v) == set(NAMES) for v in got.values())
    q1, q2, q3 = got["q1"], got["q2"], got["q3"]
    assert q1["map"] == float(Fraction(7, 18)) and q1["recip_rank"] == 0.5 and q1["P_1"] == 0.0
    assert all(q1["recall_%d" % k] == float(Fraction(2, 3)) for k in CUTOFFS)
    want = (2 / L(3) + 0.5) / (3.5 + 2 / L(3))
    other = (1 / L(3) + 2 / L(4)) / (3.5 + 2 / L(3))
    assert abs(q1["ndcg"] - want) <= 1e-15 and abs(want - other) > 0.02, "the tie goes to the larger docid"
    assert all(v == 0.0 for v in q2.values())
    assert q3["map"] == float(Fraction(37, 63)) and q3["recall_5"] == float(Fraction(1, 3)) and q3["recip_rank"] == 1.0 and q3["P_1"] == 1.0
    assert all(q3["recall_%d" % k] == 1.0 for k in CUTOFFS[1:])
    assert abs(q3["ndcg"] - (4 / 3 + 1 / L(7)) / (1.5 + 1 / L(3))) <= 1e-15
    mean = mean_metrics(got)
    assert abs(mean["map"] - float(Fraction(41, 126))) <= 1e-15 and abs(mean["recall_5"] - 1 / 3) <= 1e-15
    assert mean["recip_rank"] == 0.5 and abs(mean["P_1"] - 1 / 3) <= 1e-15


def test_host_form_zero_signs_and_nan():
    """-0.0 and +0.0 tie (the docid decides); NaN ranks as -inf, behind a finite score and level with -inf."""
    from case_rg_amd.evaluation import rank_metrics
    run = {"q": {"a": -0.0, "b": 0.0, "c": float("nan"), "d": -1e30, "e": float("-inf")}}
    # rank order: b, a (tie at zero, larger docid first), d, then e and c level at -inf, larger docid first: e, c
    for docid, rr in (("b", 1.0), ("a", 0.5), ("d", 1 / 3), ("e", 0.25), ("c", 0.2)):
        assert rank_metrics(run, {"q": {docid: 1}})["q"]["recip_rank"] == rr, docid


# ---------------------------------------------------------------------------------------------
# 2. against the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,R", [(1, 0), (4, 3), (10, 0), (37, 7), (1000, 30)])
def test_host_form_against_the_restatement(P, R):
    from case_rg_amd.evaluation import rank_metrics
    rs = random.Random(360 + P)
    width = len(str(3 * P))
    docid = lambda key: "%0*d" % (width, key + P)  # noqa: E731  (zero-padded and non-negative: string order = integer order)
    run, qrel, want = {}, {}, {}
    for q in range(6):
        scores, keys, rel, extra = random_row(rs, P, R)
        if q == 4:
            rel, extra = [min(g, 0) for g in rel], [min(g, 0) for g in extra]  # num_rel == 0
        if q == 5:
            scores = [0.5] * P                                                 # all equal: the keys alone decide
        qid = "q%d" % q
        run[qid] = {docid(k): s for k, s in zip(keys, scores)}
        qrel[qid] = {docid(k): g for k, g in zip(keys, rel)}
        qrel[qid].update({"x%d" % i: g for i, g in enumerate(extra)})
        want[qid] = restated_row(scores, keys, rel, None, extra)[1]
    got = rank_metrics(run, qrel)
    assert any(w["map"] > 0 for w in want.values()) and all(v == 0.0 for v in want["q4"].values())
    for qid in want:
        for name in EXACT:
            assert got[qid][name] == want[qid][name], (qid, name)
        assert abs(got[qid]["map"] - want[qid]["map"]) <= 1e-15 and abs(got[qid]["ndcg"] - want[qid]["ndcg"]) <= 1e-12, qid


# ---------------------------------------------------------------------------------------------
# 3. files
# ---------------------------------------------------------------------------------------------
def test_parsers_and_run_lines_round_trip(tmp_path):
    from case_rg_amd.evaluation import eval_trec_file, parse_qrel, parse_run, rank_metrics, run_lines
    from case_rg_amd.evaluation.trec import mean_metrics
    qids = ["q1", "q2", "q3"]
    pools = [list(RUN[q]) for q in qids]
    scores = [[RUN[q][d] for d in pool] for q, pool in zip(qids, pools)]
    lines = run_lines(qids, pools, scores)
    assert lines[:4] == ["q1 Q0 d1 1 0.9 system", "q1 Q0 d2 2 0.5 system", "q1 Q0 d3 3 0.5 system", "q1 Q0 d4 4 0.1 system"]
    assert lines[4:6] == ["q2 Q0 d2 1 2.0 system", "q2 Q0 d1 2 1.0 system"] and len(lines) == 13
    run = parse_run(lines)
    assert run == {q: RUN[q] for q in qids}
    qrel_lines = ["%s 0 %s %d" % (q, d, g) for q, docs in QREL.items() for d, g in docs.items()]
    assert parse_qrel(qrel_lines + ["", "  "]) == QREL
    # a later duplicate line overwrites an earlier one (the reference's run[qid][pid] = score); the rank column is not read
    dup = parse_run(lines + ["q1 Q0 d4 1 5.0 system"])
    assert dup["q1"]["d4"] == 5.0 and len(dup["q1"]) == 4
    assert rank_metrics(dup, QREL)["q1"]["recip_rank"] == 1 / 3, "d4 (grade 0) now leads: d3 is third"
    run_file, qrel_file = tmp_path / "test.run", tmp_path / "test.qrel"
    run_file.write_text(os.linesep.join(lines) + os.linesep)
    qrel_file.write_text("\n".join(qrel_lines) + "\n")
    got = eval_trec_file(str(run_file), str(qrel_file))
    assert got == mean_metrics(rank_metrics(RUN, QREL)) and set(got) == set(NAMES)
    assert abs(got["map"] - float(Fraction(41, 126))) <= 1e-15


# ---------------------------------------------------------------------------------------------
# 4. the export and the checks that need no GPU
# ---------------------------------------------------------------------------------------------
def test_rank_metrics_export_and_names():
    from case_rg_amd import _abi, ops
    from case_rg_amd.evaluation import trec
    assert ops.RANK_METRICS == NAMES == trec.METRIC_NAMES and ops.RANK_CUTOFFS == CUTOFFS == trec.RECALL_CUTOFFS
    assert _abi.FEAT_RANK_METRICS == 1 << 24 and _abi.lib.case_abi_features() & _abi.FEAT_RANK_METRICS
    assert _abi.lib.case_version() == 600
    assert "case_rank_metrics" in _abi.SIGNATURES and hasattr(_abi.lib, "case_rank_metrics")


def test_rank_metrics_argument_checks():
    import torch
    from case_rg_amd import ops
    from case_rg_amd.evaluation import rank_metrics_ids
    s, r = torch.zeros(2, 5), torch.zeros(2, 5, dtype=torch.int32)
    for bad in (dict(scores=s.double()), dict(rel=r.long()), dict(rel=r[:, :4]), dict(keys=r.long()), dict(valid=r),
                dict(extra_rel=torch.zeros(3, 2, dtype=torch.int32))):
        with pytest.raises(TypeError):
            ops.rank_metrics(**dict(dict(scores=s, rel=r), **bad))
    with pytest.raises(ValueError, match="up to 1024 retrieved"):
        ops.rank_metrics(torch.zeros(1, 1025), torch.zeros(1, 1025, dtype=torch.int32))
    with pytest.raises(ValueError, match="2048 judged"):
        ops.rank_metrics(torch.zeros(1, 1024), torch.zeros(1, 1024, dtype=torch.int32), extra_rel=torch.zeros(1, 1025, dtype=torch.int32))
    with pytest.raises(TypeError, match="labels"):
        rank_metrics_ids(s, torch.zeros(2, 5))
    with pytest.raises(TypeError, match="labels"):
        rank_metrics_ids(s, torch.zeros(3, dtype=torch.int64))


def test_rank_metrics_c_entry_refuses_the_limits_without_a_launch():
    """The C entry checks its arguments before it touches the device: outside the limits it returns an error code (raised by the ctypes
    layer) and launches nothing, so this needs no GPU.  The pointers are never dereferenced."""
    from case_rg_amd import _abi
    p = 4096
    for P, R in ((1025, 0), (1000, 1049), (0, 0)):
        with pytest.raises(RuntimeError, match="case_rank_metrics"):
            _abi.call("case_rank_metrics", p, None, p, None, p if R else None, p, p, p, 2, P, R, None)
    with pytest.raises(RuntimeError, match="case_rank_metrics"):
        _abi.call("case_rank_metrics", p, None, p, None, None, p, p, p, 2, 10, 7, None)  # R > 0 without extra_rel
