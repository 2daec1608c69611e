"""METEOR as the reference's evaluation script computes it (host side, over token lists): evaluation/Eval_Meteor.py calls nltk's
``meteor_score(references, hypothesis)`` with default arguments per item and prints the mean x 100 rounded to 2 decimals.  ``meteor_ids.py``
beside this file is the device form on token ids, as ``ngram_ids.py`` is to ``bleu.py``.  nltk's function is a short deterministic alignment
plus a closed-form score; it is spelled out here and needs nothing outside this repository.

The rule, for a hypothesis h[0 .. la) and one reference r[0 .. lb):
    stage 1 (exact)   walk i = la - 1 .. 0; for each i walk the still-unmatched reference positions j from the last to the first; the first j
                      with r[j] == h[i] is matched to i, and both are removed from further matching.
    stage 2 (class)   optional: ``classes`` maps a token to an equivalence class (a stem class, a synonym class or a union of both).  The same
                      double loop over the positions stage 1 left, comparing class keys.  A token without a class (outside the table, or a
                      negative entry) never matches here.  Without a table there is no stage 2.
    chunks            sort the matches by hypothesis position; chunks = 1, plus 1 for every consecutive pair (i, j), (i', j') of that list that
                      is not i' == i + 1 and j' == j + 1.
    score             with m = the number of matches: 0.0 when m == 0; else, in f64 and in exactly this order,
                          P = m / la,  R = m / lb,  fmean = P * R / (alpha * P + (1 - alpha) * R),
                          pen = gamma * pow(chunks / m, beta),  score = (1 - pen) * fmean
                      with nltk's defaults alpha = 0.9, beta = 3.0, gamma = 0.5.
    references        the score of an item is the maximum over its present (non-empty) references, ``best_ref`` the lowest index that
                      reaches it; an item without a present reference, or with an empty hypothesis, scores 0.0.
Read per token, both stages pair the k-th-from-last occurrence in the hypothesis with the k-th-from-last occurrence in the reference; the
device form (K40) walks the reference instead of the hypothesis and finds the same matches.

Deviations from nltk: its stemmer and WordNet stages work on strings and are two stages; here they are ONE caller-provided class table,
which is an equivalence relation (WordNet's test "is the hypothesis word among the lemmas of the reference word's synsets" is not one).  The
project ships no stemmer and no WordNet; ``stem_classes`` builds a table from any callable."""
import math
from numbers import Integral


def _tokens(s):
    return s.split(" ") if isinstance(s, str) else list(s)


def check_params(alpha, beta, gamma, who="meteor"):
    """alpha and gamma in [0, 1], beta >= 0, all finite -> the three as floats; ``ValueError`` otherwise."""
    try:
        alpha, beta, gamma = float(alpha), float(beta), float(gamma)
    except (TypeError, ValueError):
        raise ValueError("%s: alpha, beta and gamma must be numbers (got %r, %r, %r)" % (who, alpha, beta, gamma))
    if not (0.0 <= alpha <= 1.0 and 0.0 <= gamma <= 1.0 and 0.0 <= beta < math.inf):
        raise ValueError("%s: alpha and gamma in [0, 1], beta >= 0 and finite (got %r, %r, %r)" % (who, alpha, beta, gamma))
    return alpha, beta, gamma


def _class_of(classes, token):
    """The class key of a token, None when it has none: ``classes`` is a mapping (``get``) or a sequence indexed by an integer token."""
    if hasattr(classes, "get"):
        c = classes.get(token)
    else:
        if isinstance(token, bool) or not isinstance(token, Integral) or not 0 <= token < len(classes):
            return None
        c = classes[token]
    if c is None:
        return None
    if not isinstance(c, str):
        c = int(c)
        if c < 0:
            return None
    return c


def _stage(hyp_left, ref_left, matches):
    """nltk's ``_match_enums``: ``hyp_left`` / ``ref_left`` are lists of (position, key) in position order; matched pairs leave them."""
    for i in range(len(hyp_left) - 1, -1, -1):
        for j in range(len(ref_left) - 1, -1, -1):
            if hyp_left[i][1] == ref_left[j][1]:
                matches.append((hyp_left[i][0], ref_left[j][0]))
                hyp_left.pop(i)
                ref_left.pop(j)
                break


def meteor_alignment(hyp_tokens, ref_tokens, classes=None):
    """(matches, n_exact): the list of (hypothesis position, reference position) sorted by hypothesis position, and how many of them the
    exact stage made.  ``classes``: None, or a mapping / sequence from token to class for stage 2."""
    hyp, ref = _tokens(hyp_tokens), _tokens(ref_tokens)
    hyp_left, ref_left, matches = list(enumerate(hyp)), list(enumerate(ref)), []
    _stage(hyp_left, ref_left, matches)
    n_exact = len(matches)
    if classes is not None:
        keyed = [[(p, c) for p, c in ((p, _class_of(classes, t)) for p, t in left) if c is not None] for left in (hyp_left, ref_left)]
        _stage(keyed[0], keyed[1], matches)
    return sorted(matches), n_exact


def count_chunks(matches):
    """The number of chunks of an alignment sorted by hypothesis position (0 for an empty one)."""
    if not matches:
        return 0
    chunks = 1
    for (i, j), (i2, j2) in zip(matches, matches[1:]):
        if not (i2 == i + 1 and j2 == j + 1):
            chunks += 1
    return chunks


def meteor_from_counts(m, chunks, la, lb, alpha=0.9, beta=3.0, gamma=0.5):
    """The closed form, in the module docstring's order."""
    if m == 0:
        return 0.0
    P, R = m / la, m / lb
    fmean = P * R / (alpha * P + (1 - alpha) * R)
    pen = gamma * math.pow(chunks / m, beta)
    return (1 - pen) * fmean


def pair_meteor(hyp_tokens, ref_tokens, classes=None, alpha=0.9, beta=3.0, gamma=0.5):
    """dict(matches, exact, chunks, score, alignment) of one hypothesis against one reference."""
    alpha, beta, gamma = check_params(alpha, beta, gamma, "pair_meteor")
    hyp, ref = _tokens(hyp_tokens), _tokens(ref_tokens)
    matches, n_exact = meteor_alignment(hyp, ref, classes)
    chunks = count_chunks(matches)
    return dict(matches=len(matches), exact=n_exact, chunks=chunks, alignment=matches,
                score=meteor_from_counts(len(matches), chunks, len(hyp), len(ref), alpha, beta, gamma))


def best_meteor(hyp_tokens, ref_token_lists, classes=None, alpha=0.9, beta=3.0, gamma=0.5):
    """(score, best_ref): the maximum over the present (non-empty) references and the lowest index that reaches it; (0.0, -1) without one."""
    alpha, beta, gamma = check_params(alpha, beta, gamma, "sentence_meteor")
    hyp = _tokens(hyp_tokens)
    best, at = 0.0, -1
    for k, ref in enumerate(ref_token_lists):
        ref = _tokens(ref)
        if len(ref) == 0:
            continue
        score = pair_meteor(hyp, ref, classes, alpha, beta, gamma)["score"]
        if at < 0 or score > best:
            best, at = score, k
    return best, at


def sentence_meteor(hyp_tokens, ref_token_lists, classes=None, alpha=0.9, beta=3.0, gamma=0.5):
    """METEOR of one hypothesis (token list or space-joined string) against its references (see the module docstring)."""
    return best_meteor(hyp_tokens, ref_token_lists, classes, alpha, beta, gamma)[0]


def eval_meteor(hyps, refs, classes=None, alpha=0.9, beta=3.0, gamma=0.5):
    """``hyps``: one hypothesis per item; ``refs``: a list of references per item.  The mean sentence METEOR x 100 rounded to 2 decimals (what
    Run_Evaluation.py prints as METEOR)."""
    assert len(hyps) == len(refs), "the length of predicted span and ground_truths span should be same"
    total = 0.0
    for hyp, truths in zip(hyps, refs):
        total += sentence_meteor(hyp, truths, classes, alpha, beta, gamma)
    return round(total * 100 / len(hyps), 2)


def stem_classes(id2vocab, stem):
    """id2vocab (a mapping id -> token, or a sequence of tokens) and ``stem`` (any callable token -> string; the project ships none) -> the
    class table int32 [V] that ``meteor_ids`` / ``ops.meteor`` take: ids whose ``stem(token)`` strings are equal share a class (numbered in id
    order), the special tokens and ids without a token get -1."""
    import torch
    from ..common import Constants
    special = {getattr(Constants, n) for n in dir(Constants) if n.endswith("_WORD")}
    items = sorted(id2vocab.items()) if hasattr(id2vocab, "items") else list(enumerate(id2vocab))
    V = (items[-1][0] + 1) if items else 0
    table = torch.full((V,), -1, dtype=torch.int32)
    seen = {}
    for i, token in items:
        if token in special:
            continue
        table[i] = seen.setdefault(stem(token), len(seen))
    return table
