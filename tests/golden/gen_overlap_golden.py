"""Generate the n-gram overlap fixture from the reference's own evaluation/Eval_Overlap.py (build container only).

    python tests/golden/gen_overlap_golden.py            # writes tests/golden/overlap.npz

Eval_Overlap.py imports only the standard library.  Its ``ngram`` and ``overlap_ratio`` are called on seeded id lists (the ids as decimal
strings, the words it joins with spaces; orders 2..4 through ``ngram``, order 1 through ``set`` as ``eval_overlap_file`` does).  Only data is
written: the answers, the sources, their lengths and the four ratios per item.  No-op when the reference is absent.

Items: answers of 1 .. 40 ids from a vocabulary of 6 (so that n-grams repeat, and of the 216 3-grams and 1 296 4-grams a source holds a good share but not all), sources of
0 .. 300 ids; item 0 has an answer shorter than every order above 1, item 1 an empty source, item 2 an answer cut out of its source (every
ratio 1)."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden  # noqa: E402

ITEMS, FIRST, VOCAB, MAX_ANSWER, MAX_SOURCE = 24, 4, 6, 40, 300


def main():
    path = os.path.join(gen_golden.REF, "evaluation", "Eval_Overlap.py")
    if not os.path.isfile(path):
        print("gen_overlap_golden: %s not present; fixtures are generated in the build container only" % path)
        return 0
    spec = importlib.util.spec_from_file_location("ref_eval_overlap", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rs = np.random.RandomState(340)
    answers = np.zeros((ITEMS, MAX_ANSWER), dtype=np.int64)
    sources = np.zeros((ITEMS, MAX_SOURCE), dtype=np.int64)
    answer_len = rs.randint(1, MAX_ANSWER + 1, ITEMS).astype(np.int32)
    source_len = rs.randint(20, MAX_SOURCE + 1, ITEMS).astype(np.int32)
    answer_len[0], source_len[1], answer_len[2] = 1, 0, 17
    ratios = np.zeros((ITEMS, 4), dtype=np.float64)
    for i in range(ITEMS):
        sources[i, :source_len[i]] = rs.randint(0, VOCAB, source_len[i]) + FIRST
        answers[i, :answer_len[i]] = rs.randint(0, VOCAB, answer_len[i]) + FIRST
        if i == 2:
            answers[i, :17] = sources[i, 5:22]
        a = [str(t) for t in answers[i, :answer_len[i]]]
        s = [str(t) for t in sources[i, :source_len[i]]]
        ratios[i, 0] = ref.overlap_ratio(set(a), set(s))
        for n in (2, 3, 4):
            ratios[i, n - 1] = ref.overlap_ratio(ref.ngram(a, n), ref.ngram(s, n))
    assert (ratios[2] == 1).all() and (ratios[1] == 0).all() and (ratios[0, 1:] == 0).all()
    assert ((ratios > 0) & (ratios < 1)).sum() >= ITEMS, "the fixture needs ratios strictly between 0 and 1"
    out = os.path.join(HERE, "overlap.npz")
    np.savez_compressed(out, answers=answers, answer_len=answer_len, sources=sources, source_len=source_len, ratios=ratios)
    print("%-32s %8.1f KB; mean ratios %s" % (os.path.basename(out), os.path.getsize(out) / 1024, ratios.mean(0).round(3)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
