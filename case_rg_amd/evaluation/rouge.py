"""ROUGE-L as the reference's evaluation scripts compute it (host side, like the reference's: evaluation/Rouge.py:65-108 LCS,
:186-206 F-measure, :209-245 sentence-level ROUGE-L, evaluation/Eval_Rouge.py:13-68 max over ground truths, mean, x100, 2 decimals),
and ROUGE-N beside it (``rouge_n``: evaluation/Rouge.py:140-183; ``eval_rouge``: Eval_Rouge.py's three figures).

Used by the acceptance harness (north star: ROUGE-L within 0.2 of the reference on a dev set): tests/test_parity_gpu.py decodes a
synthetic dev set with the HIP path and with the CPU oracle and compares the two scores.  The LCS table is two rolling numpy
rows instead of the reference's dict of (i, j) cells."""
import numpy as np


def lcs_length(x, y):
    """Length of the longest common subsequence of two token sequences."""
    if len(x) == 0 or len(y) == 0:
        return 0
    if len(y) > len(x):
        x, y = y, x
    ids = {}
    a = np.fromiter((ids.setdefault(t, len(ids)) for t in x), dtype=np.int64, count=len(x))
    b = np.fromiter((ids.setdefault(t, len(ids)) for t in y), dtype=np.int64, count=len(y))
    prev = np.zeros(len(b) + 1, dtype=np.int64)
    for tok in a:
        match = prev[:-1] + (b == tok)          # diagonal + 1 where the tokens agree
        cur = np.maximum(prev[1:], match)       # vs the cell above
        cur = np.maximum.accumulate(cur)        # vs the cell to the left (the recurrence is monotone along the row)
        prev = np.concatenate(([0], cur))
    return int(prev[-1])


def rouge_l(hypothesis, reference):
    """(F, P, R) of ROUGE-L between two whitespace-tokenised strings (or token lists), with the reference's F-measure:
    beta = P / (R + 1e-12), F = (1 + beta^2) R P / (R + beta^2 P + 1e-12)."""
    hyp = hypothesis.split(" ") if isinstance(hypothesis, str) else list(hypothesis)
    ref = reference.split(" ") if isinstance(reference, str) else list(reference)
    llcs = lcs_length(hyp, ref)
    r, p = llcs / len(ref), llcs / len(hyp)
    beta = p / (r + 1e-12)
    f = (1 + beta ** 2) * r * p / (r + beta ** 2 * p + 1e-12)
    return f, p, r


def _tokens(text):
    return text.split(" ") if isinstance(text, str) else list(text)


def rouge_n(hypothesis, reference, n=2):
    """(F, P, R) of ROUGE-N between two whitespace-tokenised strings (or token lists) as the reference computes it (evaluation/Rouge.py:140-183):
    a SET measure over the distinct n-grams E of the hypothesis and R of the reference, o = |E & R|, P = o / |E|, R = o / |R| (0.0 where
    the denominator is 0: a sequence shorter than n, an empty list), F = 2.0 * ((P * R) / (P + R + 1e-8)) in this order."""
    if not isinstance(n, int) or n < 1:
        raise ValueError("rouge_n: n must be an integer >= 1 (got %r)" % (n,))
    hyp, ref = _tokens(hypothesis), _tokens(reference)
    evaluated = {tuple(hyp[i:i + n]) for i in range(len(hyp) - n + 1)}
    wanted = {tuple(ref[i:i + n]) for i in range(len(ref) - n + 1)}
    overlap = len(evaluated & wanted)
    p = 0.0 if len(evaluated) == 0 else overlap / len(evaluated)
    r = 0.0 if len(wanted) == 0 else overlap / len(wanted)
    f = 2.0 * ((p * r) / (p + r + 1e-8))
    return f, p, r


def eval_rouge(run, ref):
    """``run``: one hypothesis string per item; ``ref``: a list of ground-truth strings per item (token lists are taken too).  Per item the
    best F x 100 over its ground truths, each metric with its own maximum; the means over the items rounded to 2 decimals ->
    {'ROUGE_1_F1', 'ROUGE_2_F1', 'ROUGE_L_F1'}: the dict of the reference's Eval_Rouge.py eval_rouge, the three ROUGE figures that
    Run_Evaluation.py prints."""
    assert len(run) == len(ref), "the length of predicted span and ground_truths span should be same"
    rouge_1 = rouge_2 = rouge_long = total = 0
    for hyp, truths in zip(run, ref):
        rouge_1 += max(rouge_n(hyp, t, 1)[0] * 100 for t in truths)
        rouge_2 += max(rouge_n(hyp, t, 2)[0] * 100 for t in truths)
        rouge_long += max(rouge_l(hyp, t)[0] * 100 for t in truths)
        total += 1
    return {'ROUGE_1_F1': round(rouge_1 / total, 2), 'ROUGE_2_F1': round(rouge_2 / total, 2), 'ROUGE_L_F1': round(rouge_long / total, 2)}


def eval_rouge_l(run, ref):
    """``run``: one hypothesis string per item; ``ref``: a list of ground-truth strings per item.  Per item the best F over its
    ground truths, x100; the mean over items rounded to 2 decimals (what Run_Evaluation.py prints as ROUGE_L_F1)."""
    assert len(run) == len(ref), "the length of predicted span and ground_truths span should be same"
    total = 0.0
    for hyp, truths in zip(run, ref):
        total += max(rouge_l(hyp, t)[0] * 100 for t in truths)
    return round(total / len(run), 2)
