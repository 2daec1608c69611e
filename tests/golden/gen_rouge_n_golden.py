"""Generate the ROUGE-1 / ROUGE-2 fixture from the reference's own evaluation/Rouge.py (build container only).

    python tests/golden/gen_rouge_n_golden.py            # writes tests/golden/rouge_n.npz

Rouge.py needs only ``itertools`` and ``numpy`` and is loaded by path.  Its ``rouge_n`` gives (f, p, r) of every (item, ground truth, order
1..2) and its ``rouge`` the three F values of a pair, on seeded id lists (the ids as decimal strings joined with spaces, as the reference
joins words).  Eval_Rouge.py, which holds the aggregate (per item the best F x 100 over the ground truths, each metric with its own maximum;
the mean over the items; 2 decimals), imports nltk, which is not available where the fixtures are built: its ``cal_rouge`` /
``rouge_max_over_ground_truths`` / ``eval_rouge`` arithmetic is RESTATED in ``aggregate`` below, on the values that Rouge.py's ``rouge``
returns.  Only data is written: the ids, their lengths, the scores and the three aggregates.  No-op when the reference is absent.

Items: 24, ids from a vocabulary of 6 (so that n-grams repeat and a count-based ROUGE-N disagrees with the set-based one), hypotheses of
1 .. 20 ids, 1 .. 3 ground truths of 1 .. 30 ids per item (an absent one: length 0).  Item 0 has a one-token hypothesis, item 1 a ground truth
equal to its hypothesis, item 2 a ground truth over ids that its hypothesis does not use.  ``build`` asserts what the tests rely on; SEED was
picked as the first seed from 430 on for which every assertion holds."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden  # noqa: E402

ITEMS, TRUTHS, FIRST, VOCAB, MAX_HYP, MAX_REF = 24, 3, 4, 6, 20, 30
SEED = 430


def load_reference():
    path = os.path.join(gen_golden.REF, "evaluation", "Rouge.py")
    if not os.path.isfile(path):
        return None
    spec = importlib.util.spec_from_file_location("ref_rouge", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def aggregate(ref, run, truths):
    """Eval_Rouge.py's eval_rouge, restated (see the module docstring): ``run`` strings, ``truths`` lists of strings."""
    rouge_1 = rouge_2 = rouge_l = total = 0
    for pre, ground_truths in zip(run, truths):
        s1, s2, sl = [], [], []
        for ground_truth in ground_truths:
            x = ref.rouge([pre], [ground_truth])
            s1.append(x['rouge_1/f_score'] * 100)
            s2.append(x['rouge_2/f_score'] * 100)
            sl.append(x['rouge_l/f_score'] * 100)
        rouge_1 += max(s1)
        rouge_2 += max(s2)
        rouge_l += max(sl)
        total += 1
    return [round(rouge_1 / total, 2), round(rouge_2 / total, 2), round(rouge_l / total, 2)]


def repeats_a_bigram(toks):
    grams = [tuple(toks[i:i + 2]) for i in range(len(toks) - 1)]
    return len(set(grams)) < len(grams)


def build(ref, seed):
    """-> the arrays of the fixture; AssertionError when ``seed`` does not give what the tests rely on."""
    rs = np.random.RandomState(seed)
    hyp = np.zeros((ITEMS, MAX_HYP), dtype=np.int64)
    refs = np.zeros((ITEMS, TRUTHS, MAX_REF), dtype=np.int64)
    hyp_len = rs.randint(2, MAX_HYP + 1, ITEMS).astype(np.int32)
    ref_len = rs.randint(1, MAX_REF + 1, (ITEMS, TRUTHS)).astype(np.int32)
    present = rs.randint(1, TRUTHS + 1, ITEMS)
    present[:3] = 2
    hyp_len[0] = 1
    for i in range(ITEMS):
        ref_len[i, present[i]:] = 0
        hyp[i, :hyp_len[i]] = rs.randint(0, VOCAB, hyp_len[i]) + FIRST
        for m in range(present[i]):
            refs[i, m, :ref_len[i, m]] = rs.randint(0, VOCAB, ref_len[i, m]) + FIRST
    ref_len[1, 1] = hyp_len[1]                                       # an exact match
    refs[1, 1] = 0
    refs[1, 1, :hyp_len[1]] = hyp[1, :hyp_len[1]]
    hyp[2, :hyp_len[2]] = rs.randint(0, 2, hyp_len[2]) + FIRST      # a disjoint pair: the hypothesis on two ids, the truth on the other four
    refs[2, 0, :ref_len[2, 0]] = rs.randint(2, VOCAB, ref_len[2, 0]) + FIRST
    words = lambda row, n: " ".join(str(t) for t in row[:n])  # noqa: E731
    run = [words(hyp[i], hyp_len[i]) for i in range(ITEMS)]
    truths = [[words(refs[i, m], ref_len[i, m]) for m in range(present[i])] for i in range(ITEMS)]
    scores = np.zeros((ITEMS, TRUTHS, 2, 3), dtype=np.float64)  # (f, p, r) of rouge_n, orders 1 and 2; an absent truth reads 0
    rouge_l = np.zeros((ITEMS, TRUTHS, 3), dtype=np.float64)    # (f, p, r) of the sentence-level ROUGE-L
    for i in range(ITEMS):
        for m, truth in enumerate(truths[i]):
            for n in (1, 2):
                scores[i, m, n - 1] = ref.rouge_n([run[i]], [truth], n)
            x = ref.rouge([run[i]], [truth])
            rouge_l[i, m] = x['rouge_l/f_score'], x['rouge_l/p_score'], x['rouge_l/r_score']
            assert x['rouge_1/f_score'] == scores[i, m, 0, 0] and x['rouge_2/f_score'] == scores[i, m, 1, 0]
    aggregates = np.array(aggregate(ref, run, truths), dtype=np.float64)

    assert sum(repeats_a_bigram(hyp[i, :hyp_len[i]].tolist()) for i in range(ITEMS)) >= 8, "hypotheses with a repeated bigram"
    assert sum(repeats_a_bigram(refs[i, m, :ref_len[i, m]].tolist()) for i in range(ITEMS) for m in range(present[i])) >= 8
    assert hyp_len[0] == 1 and (scores[0, :, 1, 0] == 0).all(), "a one-token hypothesis has no bigram"
    assert (scores[1, 1, :, 1:] == 1).all() and abs(scores[1, 1, 0, 0] - 1) < 1e-8, "the exact match"
    assert (scores[2, 0] == 0).all() and rouge_l[2, 0, 0] == 0, "the disjoint pair"

    def best(f, i):  # the first maximum among the present truths, None unless it is the only one
        row = f[i, :present[i]]
        return int(row.argmax()) if (row == row.max()).sum() == 1 else None

    differ = lambda f, g: [i for i in range(ITEMS) if None not in (best(f, i), best(g, i)) and best(f, i) != best(g, i)]  # noqa: E731
    assert differ(scores[:, :, 0, 0], scores[:, :, 1, 0]), "an item whose best truth differs between ROUGE-1 and ROUGE-2"
    assert differ(scores[:, :, 1, 0], rouge_l[:, :, 0]), "an item whose best truth differs between ROUGE-2 and ROUGE-L"
    return dict(hyp=hyp, hyp_len=hyp_len, refs=refs, ref_len=ref_len, scores=scores, rouge_l=rouge_l, aggregates=aggregates)


def main():
    ref = load_reference()
    if ref is None:
        print("gen_rouge_n_golden: %s not present; fixtures are generated in the build container only" % gen_golden.REF)
        return 0
    data = build(ref, SEED)
    out = os.path.join(HERE, "rouge_n.npz")
    np.savez_compressed(out, **data)
    print("%-32s %8.1f KB; ROUGE_1_F1 / ROUGE_2_F1 / ROUGE_L_F1 %s" % (os.path.basename(out), os.path.getsize(out) / 1024, data["aggregates"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
