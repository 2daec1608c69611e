"""TREC ranking metrics of a run against relevance judgements, on the host: what the reference's ``evaluation/Eval_Trec.py`` asks
``pytrec_eval`` (trec_eval) for -- ``map``, ``ndcg``, ``recall`` -- plus ``recip_rank`` and ``P_1``.  ``rank_ids.py`` beside this file is the
device form over score tensors (K36).

Definitions (trec_eval's).  Each query has a list of retrieved documents; a document has a score, a tie key (here: its docid string) and a
relevance grade.

RANKING.  By score descending; among equal scores the LARGER tie key comes first (trec_eval's "docno descending" rule; the ``rank`` column of
a run file is ignored, as trec_eval ignores it).  ``-0.0`` and ``+0.0`` are equal scores, a NaN score compares as ``-inf``.  Equal (score,
key) pairs, which a caller should not produce, are ordered by ascending column index (device form), so the order is total and reproducible.

RELEVANCE.  A document is relevant when its grade is >= 1; a negative grade counts as 0.  ``num_rel`` is the number of relevant JUDGED
documents of the query, those that were not retrieved included.

METRICS, with i the 1-based rank:
  ``map``         (1 / num_rel) x the sum over the relevant ranks i of (relevant documents in the top i) / i
  ``ndcg``        DCG / IDCG;  DCG = sum_i grade_i / log2(i + 1) over the ranked list, the grade itself as the gain;  IDCG = the same sum over
                  all judged grades >= 1 of the query sorted descending, the unretrieved ones included
  ``recall_k``    (relevant in the top min(k, retrieved)) / num_rel  for k in 5, 10, 15, 20, 30, 100, 200, 500, 1000
  ``recip_rank``  1 / (rank of the first relevant document), 0 if there is none
  ``P_1``         whether the top document is relevant (for the models' single gold passage: selection accuracy)

CONVENTIONS.  Every metric of a query with ``num_rel == 0`` is 0 and the query is still counted; the corpus figure is the plain mean over
queries; every item is its own query.  One deviation: the reference's ``run[qid][pid] = score`` lets a later duplicate line of a run file
overwrite an earlier one; the file form here keeps that, the id-tensor form does not merge items."""
import math
from fractions import Fraction

RECALL_CUTOFFS = (5, 10, 15, 20, 30, 100, 200, 500, 1000)
METRIC_NAMES = ("map", "ndcg") + tuple("recall_%d" % k for k in RECALL_CUTOFFS) + ("recip_rank", "P_1")  # K36's column order


def _score(x):
    x = float(x)
    return -math.inf if x != x else x + 0.0  # (-0.0 + 0.0 is +0.0)


def query_metrics(ranked_grades, judged_grades):
    """``ranked_grades``: the grades of the retrieved documents in rank order; ``judged_grades``: the grades of ALL judged documents of the
    query -> the dict of METRIC_NAMES.  Counts and ratios are exact (``Fraction``, rounded once to f64); DCG and IDCG are f64 sums in rank
    order."""
    gains = [max(int(g), 0) for g in ranked_grades]
    ideal = sorted((int(g) for g in judged_grades if int(g) >= 1), reverse=True)
    num_rel = len(ideal)
    if num_rel == 0:
        return {name: 0.0 for name in METRIC_NAMES}
    seen, ap, first, dcg = 0, Fraction(0), 0, 0.0
    at = {}
    for i, g in enumerate(gains, 1):
        if g >= 1:
            seen += 1
            ap += Fraction(seen, i)
            first = first or i
            dcg += g / math.log2(i + 1)
        at[i] = seen
    idcg = 0.0
    for i, g in enumerate(ideal, 1):
        idcg += g / math.log2(i + 1)
    out = {"map": float(ap / num_rel), "ndcg": dcg / idcg}
    for k in RECALL_CUTOFFS:
        out["recall_%d" % k] = float(Fraction(at.get(min(k, len(gains)), 0), num_rel))
    out["recip_rank"] = float(Fraction(1, first)) if first else 0.0
    out["P_1"] = 1.0 if gains and gains[0] >= 1 else 0.0
    return out


def rank_metrics(run, qrel):
    """run = {qid: {docid: score}}, qrel = {qid: {docid: grade}} (``pytrec_eval``'s shapes) -> {qid: {metric: f64}} for the queries present in
    both; ties in the score are broken on the docid strings."""
    out = {}
    for qid, docs in run.items():
        if qid not in qrel:
            continue
        judged = qrel[qid]
        ranked = sorted(docs.items(), key=lambda d: (_score(d[1]), d[0]), reverse=True)
        out[qid] = query_metrics([judged.get(docid, 0) for docid, _ in ranked], judged.values())
    return out


def parse_run(lines):
    """The six-column run format ``qid Q0 docid rank score system`` -> {qid: {docid: score}}; a later line of the same (qid, docid) overwrites
    an earlier one, as in the reference; the rank column is not read."""
    run = {}
    for line in lines:
        if not line.strip():
            continue
        qid, _, docid, _, score, _ = line.strip().split()
        run.setdefault(qid, {})[docid] = float(score)
    return run


def parse_qrel(lines):
    """The four-column qrel format ``qid 0 docid grade`` -> {qid: {docid: grade}}."""
    qrel = {}
    for line in lines:
        if not line.strip():
            continue
        qid, _, docid, grade = line.strip().split()
        qrel.setdefault(qid, {})[docid] = int(grade)
    return qrel


def mean_metrics(per_query):
    """{qid: {metric: value}} -> {metric: the plain mean over the queries} ({} without a query)."""
    avg = {}
    for res in per_query.values():
        for k, v in res.items():
            avg[k] = avg.get(k, 0.0) + v
    return {k: v / len(per_query) for k, v in avg.items()}


def eval_trec_file(run_file, qrel_file):
    """The reference's ``eval_trec_file``: the mean of every metric over the queries of the two files."""
    with open(run_file) as f:
        run = parse_run(f)
    with open(qrel_file) as f:
        qrel = parse_qrel(f)
    return mean_metrics(rank_metrics(run, qrel))


def run_lines(query_ids, pool_ids, scores, system="system"):
    """The lines the reference's ``save_result`` writes for ``rank``: per item i the documents ``pool_ids[i][j]`` with ``scores[i][j]``,
    sorted by score descending (stable: equal scores keep their pool order), ranks from 1."""
    lines = []
    for qid, pool, row in zip(query_ids, pool_ids, scores):
        docs = sorted(((docid, float(row[j])) for j, docid in enumerate(pool)), key=lambda d: d[1], reverse=True)
        lines += ["%s Q0 %s %d %s %s" % (qid, docid, i, score, system) for i, (docid, score) in enumerate(docs, 1)]
    return lines
