"""BLEU and n-gram overlap as the reference's evaluation scripts compute them (host side, over token lists): evaluation/Eval_Bleu.py calls
nltk's ``sentence_bleu(references, hypothesis)`` with default arguments per item and prints the mean x 100 rounded to 2 decimals;
evaluation/Eval_Overlap.py prints the share of an answer's distinct n-grams that occur in its passages.  ``ngram_ids.py`` beside this file is
the device form on token ids, as ``rouge_ids.py`` is to ``rouge.py``.

Sentence BLEU, spelled out (nltk.translate.bleu_score, uniform weights over the orders 1 .. max_n):
    clip_k = sum over the distinct k-grams g of the hypothesis of min(count_hyp(g), max over the references of count_ref(g))
    p_k    = clip_k / max(1, la - k + 1)                         (la = the hypothesis length; the modified precision, an exact fraction)
    r      = the reference length closest to la, the shorter one on a tie
    BP     = 1 if la > r, else exp(1 - r / la)
    score  = BP exp(sum_k ln p_k / max_n)
``smoothing="none"``: the score is exactly 0.0 when any clip_k is 0.  (Deviation: nltk substitutes the smallest normal double for such a p_k and
prints a warning, which gives about 1e-78 for one missing order; at the two decimals the reference reports the numbers are identical.)
``smoothing="add1"`` (Lin & Och 2004, nltk's ``SmoothingFunction().method2``): p_k = (clip_k + 1) / (max(1, la - k + 1) + 1) for k >= 2, p_1
unsmoothed, and 0.0 when clip_1 is 0.  No reference, or only empty ones, gives 0.0."""
import math
from collections import Counter
from fractions import Fraction

SMOOTHINGS = ("none", "add1")


def _tokens(s):
    return s.split(" ") if isinstance(s, str) else list(s)


def ngram_counts(tokens, n):
    """Counter of the n-grams (tuples) of a token list."""
    return Counter(tuple(tokens[i:i + n]) for i in range(len(tokens) - n + 1))


def clipped_matches(hyp_tokens, ref_token_lists, n):
    """(clip_n, total_n): the clipped n-gram matches of the hypothesis against the references, and its number of n-grams."""
    hyp = ngram_counts(hyp_tokens, n)
    best = Counter()
    for ref in ref_token_lists:
        for g, c in ngram_counts(ref, n).items():
            if g in hyp and c > best[g]:
                best[g] = c
    return sum(min(c, best[g]) for g, c in hyp.items()), sum(hyp.values())


def modified_precision(hyp_tokens, ref_token_lists, n):
    """nltk's ``modified_precision`` as an exact ``Fraction``: clip_n / max(1, total_n)."""
    clip, total = clipped_matches(_tokens(hyp_tokens), [_tokens(r) for r in ref_token_lists], n)
    return Fraction(clip, max(1, total))


def closest_ref_length(ref_lengths, hyp_len):
    """The reference length closest to ``hyp_len``, the shorter one on a tie."""
    return min(ref_lengths, key=lambda r: (abs(r - hyp_len), r))


def brevity_penalty(closest, hyp_len):
    if hyp_len > closest:
        return 1.0
    return 0.0 if hyp_len == 0 else math.exp(1.0 - closest / hyp_len)


def sentence_bleu(hyp_tokens, ref_token_lists, max_n=4, smoothing="none"):
    """BLEU of one hypothesis (token list or space-joined string) against its references (see the module docstring)."""
    if smoothing not in SMOOTHINGS:
        raise ValueError("sentence_bleu: smoothing must be one of %s, not %r" % (SMOOTHINGS, smoothing))
    if not 1 <= max_n <= 4:
        raise ValueError("sentence_bleu: max_n in 1..4 (got %r)" % (max_n,))
    hyp = _tokens(hyp_tokens)
    refs = [r for r in (_tokens(r) for r in ref_token_lists) if len(r) > 0]
    if len(hyp) == 0 or not refs:
        return 0.0
    s = 0.0
    for k in range(1, max_n + 1):
        num, den = clipped_matches(hyp, refs, k)
        den = max(1, den)
        if smoothing == "add1" and k > 1:
            num, den = num + 1, den + 1
        if num == 0:
            return 0.0
        s += math.log(num / den)
    return brevity_penalty(closest_ref_length([len(r) for r in refs], len(hyp)), len(hyp)) * math.exp(s / max_n)


def eval_bleu(hyps, refs, max_n=4, smoothing="none"):
    """``hyps``: one hypothesis per item; ``refs``: a list of references per item.  The mean sentence BLEU x 100 rounded to 2 decimals (what
    Run_Evaluation.py prints as BLEU)."""
    assert len(hyps) == len(refs), "the length of predicted span and ground_truths span should be same"
    total = 0.0
    for hyp, truths in zip(hyps, refs):
        total += sentence_bleu(hyp, truths, max_n, smoothing)
    return round(total * 100 / len(hyps), 2)


def ngram_overlap(answer_tokens, source_tokens, n):
    """Eval_Overlap's ratio: the share of the answer's distinct n-grams that occur in the source; 0 for an answer without an n-gram."""
    answer = set(ngram_counts(_tokens(answer_tokens), n))
    if not answer:
        return 0.0
    return len(answer & set(ngram_counts(_tokens(source_tokens), n))) / len(answer)
