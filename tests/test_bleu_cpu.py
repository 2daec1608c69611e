"""BLEU and n-gram overlap, CPU side: the host form ``evaluation.bleu`` against nltk's published worked example, against exact modified
precisions and against an independent restatement (``restated_counts`` / ``restated_bleu`` below: ``collections.Counter``, ``Fraction`` and
``math`` only, in nltk's own order -- ``fsum`` of weight x log precision); the add-one rule and the brevity-penalty tie rule by hand; the
overlap ratio against the reference-generated fixture; the two new exports in the header, the ctypes table and the built library; and the
argument checks that need no GPU.  tests/test_bleu_gpu.py holds the kernels against this restatement.

nltk is not available where the fixtures are built, so no BLEU number here comes from running the reference's ``Eval_Bleu.py``: the pins are
the worked example of nltk's documentation (``hypothesis1`` "It is a guide to action which ensures ..." with its three references), whose
values the restatement reproduces.  tests/golden/overlap.npz does come from the reference's ``Eval_Overlap.py`` (gen_overlap_golden.py)."""
import ctypes
import math
import os
import re
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest

from helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "case_hip.h")

HYP1 = "It is a guide to action which ensures that the military always obeys the commands of the party".split()
REF1 = "It is a guide to action that ensures that the military will forever heed Party commands".split()
REF2 = "It is the guiding principle which guarantees the military forces always being under the command of the Party".split()
REF3 = "It is the practical guide for the army always to heed the directions of the party".split()
CAT = ["the cat is on the mat".split(), "there is a cat on the mat".split()]


# ---------------------------------------------------------------------------------------------
# the restatement (shared with tests/test_bleu_gpu.py)
# ---------------------------------------------------------------------------------------------
def _grams(tokens, k):
    return Counter(tuple(tokens[i:i + k]) for i in range(len(tokens) - k + 1))


def restated_counts(hyp, refs, k):
    """-> dict(clip [M], clip_any, hit [M], hit_any, distinct, total) of order k; an empty reference is absent (it adds nothing anyway)."""
    h = _grams(hyp, k)
    rs = [_grams(r, k) for r in refs]
    return dict(clip=[sum(min(c, r[g]) for g, c in h.items()) for r in rs],
                clip_any=sum(min(c, max([r[g] for r in rs] + [0])) for g, c in h.items()),
                hit=[sum(1 for g in h if r[g] > 0) for r in rs], hit_any=sum(1 for g in h if any(r[g] > 0 for r in rs)),
                distinct=len(h), total=max(len(hyp) - k + 1, 0))


def restated_bp(la, ref_lens):
    """(BP, r): r = the present reference length closest to la, the shorter one on a tie; BP = 1 if la > r else exp(1 - r / la)."""
    present = [n for n in ref_lens if n > 0]
    if not present or la == 0:
        return 0.0, 0
    r = sorted(present, key=lambda n: (abs(n - la), n))[0]
    return (1.0 if la > r else math.exp(1 - Fraction(r, la))), r


def restated_bleu(hyp, refs, max_n=4, smoothing="none"):
    """nltk's sentence_bleu over the present references: exact precisions, ``fsum`` of weight x log, times BP; 0.0 instead of nltk's
    denormal substitute when a precision is 0 (the stated deviation)."""
    refs = [r for r in refs if len(r) > 0]
    bp, _ = restated_bp(len(hyp), [len(r) for r in refs])
    if bp == 0.0:
        return 0.0
    p = []
    for k in range(1, max_n + 1):
        c = restated_counts(hyp, refs, k)
        num, den = c["clip_any"], max(1, c["total"])
        if smoothing == "add1" and k > 1:
            num, den = num + 1, den + 1
        p.append(Fraction(num, den))
    if min(p) == 0:
        return 0.0
    return bp * math.exp(math.fsum(math.log(x) / max_n for x in p))


# ---------------------------------------------------------------------------------------------
# the host form
# ---------------------------------------------------------------------------------------------
def test_host_bleu_on_the_published_worked_example():
    from case_rg_amd.evaluation import eval_bleu, modified_precision, sentence_bleu
    assert abs(sentence_bleu(HYP1, [REF1, REF2, REF3]) - 0.5045666840058485) <= 1e-15
    assert abs(sentence_bleu(HYP1, [REF1]) - 0.41180376356915777) <= 1e-15
    assert abs(restated_bleu(HYP1, [REF1, REF2, REF3]) - 0.5045666840058485) <= 1e-15, "the restatement must reproduce the published value too"
    assert abs(restated_bleu(HYP1, [REF1]) - 0.41180376356915777) <= 1e-15
    assert modified_precision(["the"] * 7, CAT, 1) == Fraction(2, 7)
    assert [modified_precision(HYP1, [REF1, REF2, REF3], n) for n in (1, 2, 3, 4)] == [Fraction(17, 18), Fraction(10, 17), Fraction(7, 16), Fraction(4, 15)]
    assert sentence_bleu(" ".join(HYP1), [" ".join(REF1)]) == sentence_bleu(HYP1, [REF1]), "space-joined strings are token lists"
    assert eval_bleu([HYP1, HYP1], [[REF1, REF2, REF3], [REF1]]) == round((0.5045666840058485 + 0.41180376356915777) * 50, 2) == 45.82
    assert sentence_bleu(HYP1, []) == 0.0 and sentence_bleu(HYP1, [[]]) == 0.0 and sentence_bleu([], [REF1]) == 0.0
    for bad in (dict(max_n=0), dict(max_n=5), dict(smoothing="floor")):
        with pytest.raises(ValueError):
            sentence_bleu(HYP1, [REF1], **bad)


def test_host_bleu_against_the_restatement_on_random_lists():
    """Both are f64 evaluations of the same exact fractions: they differ by the rounding of at most four logarithms (each below 6 in size,
    so 1e-15 absolute), one sum and one exp of a value in [0, 1]: 1e-14 bounds it with room."""
    from case_rg_amd.evaluation import sentence_bleu
    rs = np.random.RandomState(34)
    nonzero = 0
    for case in range(400):
        vocab = (3, 6, 50)[case % 3]
        hyp = rs.randint(0, vocab, rs.randint(0, 30)).tolist()
        refs = [rs.randint(0, vocab, rs.randint(0, 40)).tolist() for _ in range(rs.randint(0, 4))]
        if case % 4 == 0 and refs and len(refs[0]) > 4:
            hyp = refs[0][:rs.randint(4, len(refs[0]) + 1)]
        for max_n in (1, 2, 3, 4):
            for smoothing in ("none", "add1"):
                got, want = sentence_bleu(hyp, refs, max_n, smoothing), restated_bleu(hyp, refs, max_n, smoothing)
                assert abs(got - want) <= 1e-14, (case, hyp, refs, max_n, smoothing, got, want)
                nonzero += want > 0
    assert nonzero > 800


def test_add_one_smoothing_and_the_zero_rules():
    from case_rg_amd.evaluation import sentence_bleu
    hyp, ref = "a b c d".split(), "a b x y".split()
    # clip = 2, 1, 0, 0 of 4, 3, 2, 1: p_1 stays 2/4, the others get (c + 1) / (t + 1); la = r = 4: BP = exp(0) = 1
    want = math.exp((math.log(2 / 4) + math.log(2 / 4) + math.log(1 / 3) + math.log(1 / 2)) / 4)
    assert abs(sentence_bleu(hyp, [ref], smoothing="add1") - want) <= 1e-15
    assert sentence_bleu(hyp, [ref]) == 0.0, "unsmoothed: a missing order gives exactly 0"
    assert abs(sentence_bleu(hyp, [ref], max_n=2) - math.sqrt(2 / 4 * 1 / 3)) <= 1e-15
    assert sentence_bleu("p q r s".split(), [ref], smoothing="add1") == 0.0, "add1 leaves p_1 alone: no unigram match gives 0"
    # a hypothesis shorter than the order: the denominator is max(1, la - k + 1) = 1
    assert abs(sentence_bleu(["a"], [["a"]], smoothing="add1") - math.exp(3 * math.log(1 / 2) / 4)) <= 1e-15
    assert sentence_bleu(["a"], [["a"]]) == 0.0 and sentence_bleu(["a"], [["a"]], max_n=1) == 1.0


def test_brevity_penalty_takes_the_shorter_reference_on_a_tie():
    from case_rg_amd.evaluation import sentence_bleu
    hyp = "a b c d e".split()
    refs = ["a b c d".split(), "a b c d e f".split()]  # lengths 4 and 6 are equally close to 5: r = 4 < la, BP = 1; every precision is 1
    assert sentence_bleu(hyp, refs) == 1.0 == restated_bleu(hyp, refs)
    assert sentence_bleu(hyp, refs[::-1]) == 1.0, "the order of the references does not matter"
    assert abs(sentence_bleu(hyp, refs[1:]) - math.exp(1 - 6 / 5)) <= 1e-15, "with the longer one alone the penalty bites"
    assert restated_bp(5, [6, 0, 4]) == (1.0, 4) and restated_bp(5, [0, 0]) == (0.0, 0) and restated_bp(5, [5])[0] == 1.0


def test_host_overlap_is_the_reference_fixture():
    """tests/golden/overlap.npz: the reference's ``ngram`` / ``overlap_ratio`` on seeded id lists.  Equal small integers divided: exact."""
    from case_rg_amd.evaluation import ngram_overlap
    g = load_golden("overlap")
    assert g["ratios"].shape == (24, 4) and ((g["ratios"] > 0) & (g["ratios"] < 1)).sum() >= 24
    for i in range(24):
        a, s = g["answers"][i, :g["answer_len"][i]].tolist(), g["sources"][i, :g["source_len"][i]].tolist()
        for n in (1, 2, 3, 4):
            assert ngram_overlap(a, s, n) == g["ratios"][i, n - 1], (i, n)
            c = restated_counts(a, [s], n)
            assert (c["hit_any"] / c["distinct"] if c["distinct"] else 0.0) == g["ratios"][i, n - 1], "the restatement's counts give it too"
    assert ngram_overlap([], [1, 2], 1) == 0.0 and ngram_overlap([1], [1, 2], 2) == 0.0
    assert ngram_overlap("x y x y z", "q x y z", 2) == 2 / 3  # distinct bigrams xy, yx, yz: xy and yz occur


# ---------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------
def test_header_table_and_library_carry_the_two_exports():
    from case_rg_amd import _abi
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for name, nargs in (("case_ngram_counts", 16), ("case_bleu_scores", 13)):
        proto = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, text, flags=re.S)
        assert proto, "%s is not declared in include/case_hip.h" % name
        assert len([a for a in proto.group(1).split(",") if a.strip()]) == nargs == len(_abi.SIGNATURES[name])
        assert hasattr(lib, name), "libcase_hip.so does not export %s" % name
    assert _abi.FEAT_NGRAM_COUNTS == 1 << 23 and re.search(r"CASE_FEAT_NGRAM_COUNTS\s*=\s*1u\s*<<\s*23", text)
    assert _abi.lib.case_abi_features() & _abi.FEAT_NGRAM_COUNTS
    assert _abi.lib.case_version() == _abi.ABI_VERSION == 600, "nothing existing changed layout: the generation stays"


def test_exports_validate_before_any_launch():
    """Null pointers, non-positive counts, an order outside 1..4, an unknown smoothing and a hypothesis side beyond 256 positions are refused
    on the host side of the ABI."""
    from case_rg_amd import _abi
    with pytest.raises(RuntimeError, match="case_ngram_counts"):
        _abi.call("case_ngram_counts", *([None] * 9), 1, 1, 1, 8, 8, 4, None)
    buf = (ctypes.c_int64 * 8)()  # never dereferenced: every call below is refused before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    for B, N, M, Ta, Tb, max_n in ((0, 1, 1, 8, 8, 4), (1, 0, 1, 8, 8, 4), (1, 1, 0, 8, 8, 4), (1, 1, 1, 0, 8, 4), (1, 1, 1, 8, 0, 4),
                                   (1, 1, 1, 8, 8, 0), (1, 1, 1, 8, 8, 5), (1, 1, 1, 257, 8, 4), (1 << 20, 1 << 12, 1, 8, 8, 4)):
        with pytest.raises(RuntimeError, match="case_ngram_counts"):
            _abi.call("case_ngram_counts", *([p] * 9), B, N, M, Ta, Tb, max_n, None)
    with pytest.raises(RuntimeError, match="up to 256 positions"):
        _abi.call("case_ngram_counts", *([p] * 9), 1, 1, 1, 257, 8, 4, None)
    with pytest.raises(RuntimeError, match="case_bleu_scores"):
        _abi.call("case_bleu_scores", *([None] * 7), 1, 1, 1, 4, 0, None)
    for B, N, M, max_n, smoothing in ((0, 1, 1, 4, 0), (1, 0, 1, 4, 0), (1, 1, 0, 4, 0), (1, 1, 1, 0, 0), (1, 1, 1, 5, 1), (1, 1, 1, 4, 2), (1, 1, 1, 4, -1)):
        with pytest.raises(RuntimeError, match="case_bleu_scores"):
            _abi.call("case_bleu_scores", *([p] * 7), B, N, M, max_n, smoothing, None)


def test_ops_check_their_arguments_before_the_library_is_called():
    import torch
    from case_rg_amd import ops
    assert ops.ngram_supported(256) and ops.ngram_supported(1, 1) and not ops.ngram_supported(257) and not ops.ngram_supported(64, 5)
    a, n = torch.zeros(2, 3, 8, dtype=torch.int64), torch.ones(2, 3, dtype=torch.int32)
    b, m = torch.zeros(2, 2, 9, dtype=torch.int64), torch.ones(2, 2, dtype=torch.int32)
    with pytest.raises(TypeError, match="int64"):
        ops.ngram_counts(a.int(), n, b, m)
    with pytest.raises(TypeError, match="one batch"):
        ops.ngram_counts(a, n, b[:1], m[:1])
    with pytest.raises(TypeError, match="lengths"):
        ops.ngram_counts(a, n.long(), b, m)
    with pytest.raises(TypeError, match="lengths"):
        ops.ngram_counts(a, n[:, :2], b, m)
    for bad in (0, 5, 2.0):
        with pytest.raises(ValueError, match="max_n"):
            ops.ngram_counts(a, n, b, m, max_n=bad)
    with pytest.raises(ValueError, match="up to 256 positions"):
        ops.ngram_counts(torch.zeros(2, 3, 257, dtype=torch.int64), n, b, m)
    counts = dict(clip=torch.zeros(2, 3, 2, 4, dtype=torch.int32), clip_any=torch.zeros(2, 3, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="smoothing"):
        ops.bleu_scores(counts, n, m, smoothing="add2")
    with pytest.raises(ValueError, match="max_n"):
        ops.bleu_scores(counts, n, m, max_n=7)
    with pytest.raises(TypeError, match="clip"):
        ops.bleu_scores(dict(counts, clip=counts["clip"][:, :, :1]), n, m)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.bleu_scores(counts, n, m)  # everything checked: only now would the library be called


def test_metric_is_checked_early_and_never_reaches_the_decoder():
    """``do_consensus(metric=...)`` is an explicit keyword: an unknown one raises before anything is decoded, and a known one is not handed to
    ``do_sample`` among the sampling arguments."""
    import torch
    import case_rg_amd
    from case_rg_amd import evaluation
    from case_rg_amd.utils import make_vocab
    ns = case_rg_amd.namespace()
    v2i, i2v = make_vocab(200)

    class Reached(Exception):
        pass

    for model in (ns.CaSE(4, 5, i2v, v2i, 32), ns.Masque(5, i2v, v2i, 32)):
        assert model.consensus_metric == "rouge_l"
        model.eval()
        seen = {}

        def do_sample(data, **kw):
            seen.update(kw)
            raise Reached

        model.do_sample = do_sample
        with pytest.raises(ValueError, match="metric must be one of"):
            model.do_consensus({}, metric="nonsense")
        assert not seen, "the metric is checked before the pool is decoded"
        for metric in ("bleu", None):
            seen.clear()
            with pytest.raises(Reached):
                model.do_consensus({}, metric=metric, seed=3)
            assert seen["seed"] == 3 and seen["num_samples"] == 8 and "metric" not in seen
        model.consensus_metric = "nonsense"
        with pytest.raises(ValueError, match="metric must be one of"):
            model.do_consensus({})
    with pytest.raises(ValueError, match="metric must be one of"):
        evaluation.consensus(torch.zeros(2, 4, 8, dtype=torch.int64), (1, 0, 2, 3), metric="meteor")
    with pytest.raises(ValueError, match="up to 256 positions"):
        evaluation.bleu_ids(torch.zeros(2, 257, dtype=torch.int64), torch.zeros(2, 8, dtype=torch.int64), (1, 0, 2, 3))
    with pytest.raises(ValueError, match="smoothing"):
        evaluation.bleu_ids(torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, 8, dtype=torch.int64), (1, 0, 2, 3), smoothing="floor")
