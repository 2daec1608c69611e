"""ROUGE-1 / ROUGE-2, CPU side: the host form ``evaluation.rouge_n`` / ``eval_rouge`` against the reference-generated fixture
(tests/golden/rouge_n.npz, gen_rouge_n_golden.py: the reference's own ``rouge_n`` and ``rouge``) bit for bit, hand-worked cases, the symmetry of
F, the two new exports in the header, the ctypes table and the built library, and every argument check that needs no GPU -- of the exports, of
``ops``, of the ``*_ids`` functions, of the trainer (before a model is called) and of consensus.  tests/test_rouge_n_gpu.py holds the kernels."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "case_hip.h")
SPECIALS = (1, 0, 2, 3)


def fixture_lists():
    """-> (the fixture, hypotheses as id lists [24], ground truths as lists of id lists [24][1..3]: the present ones, which come first)."""
    g = load_golden("rouge_n")
    hyps = [g["hyp"][i, :n].tolist() for i, n in enumerate(g["hyp_len"])]
    truths = [[g["refs"][i, m, :n].tolist() for m, n in enumerate(g["ref_len"][i]) if n > 0] for i in range(len(hyps))]
    return g, hyps, truths


def restated_distinct(tokens, k):
    """The number of distinct k-grams of a token list, by a Python ``set`` (shared with tests/test_rouge_n_gpu.py)."""
    return len({tuple(tokens[i:i + k]) for i in range(len(tokens) - k + 1)})


# ---------------------------------------------------------------------------------------------
# the host form
# ---------------------------------------------------------------------------------------------
def test_fixture_holds_what_the_tests_rely_on():
    g, hyps, truths = fixture_lists()
    assert len(hyps) == 24 and g["scores"].shape == (24, 3, 2, 3) and g["aggregates"].shape == (3,)
    assert set(len(t) for t in truths) == {1, 2, 3} and all((g["ref_len"][i, :len(t)] > 0).all() for i, t in enumerate(truths))
    assert set(np.unique(g["hyp"])) <= set(range(4, 10)) | {0}, "a vocabulary of 6"
    repeated = lambda t: restated_distinct(t, 2) < len(t) - 1  # noqa: E731
    assert sum(map(repeated, hyps)) >= 8 and sum(repeated(t) for ts in truths for t in ts) >= 8
    assert len(hyps[0]) == 1 and truths[1][1] == hyps[1] and not set(hyps[2]) & set(truths[2][0])


def test_host_rouge_n_is_the_reference_bit_for_bit():
    from case_rg_amd.evaluation import rouge_n
    g, hyps, truths = fixture_lists()
    for i, hyp in enumerate(hyps):
        for m, truth in enumerate(truths[i]):
            for n in (1, 2):
                got = rouge_n(hyp, truth, n)
                assert got == tuple(g["scores"][i, m, n - 1]), (i, m, n, got, g["scores"][i, m, n - 1])
                assert all(type(v) is float for v in got)
                words = lambda t: " ".join(str(x) for x in t)  # noqa: E731
                assert rouge_n(words(hyp), words(truth), n) == got, "space-joined strings are token lists"
    assert rouge_n(hyps[3], truths[3][0]) == rouge_n(hyps[3], truths[3][0], 2), "the default order is the reference's: 2"


def test_host_eval_rouge_is_the_reference_aggregate():
    from case_rg_amd.evaluation import eval_rouge, eval_rouge_l
    g, hyps, truths = fixture_lists()
    got = eval_rouge(hyps, truths)
    assert list(got) == ["ROUGE_1_F1", "ROUGE_2_F1", "ROUGE_L_F1"]
    assert [got[k] for k in got] == g["aggregates"].tolist()
    assert got["ROUGE_L_F1"] == eval_rouge_l(hyps, truths), "eval_rouge_l stays what it was"
    # each metric takes its own maximum: somewhere the best ground truth of one is not the best of another
    best = lambda f: [int(np.argmax(f[i, :len(t)])) for i, t in enumerate(truths)]  # noqa: E731
    assert best(g["scores"][:, :, 0, 0]) != best(g["scores"][:, :, 1, 0]) and best(g["scores"][:, :, 1, 0]) != best(g["rouge_l"][:, :, 0])
    with pytest.raises(AssertionError):
        eval_rouge(hyps, truths[:-1])


def test_hand_worked_cases():
    from case_rg_amd.evaluation import rouge_n
    one = 2.0 * (1.0 / (2.0 + 1e-8))
    assert rouge_n("a a a", "a", 1) == (one, 1.0, 1.0), "a set measure: the repeated unigram counts once"
    assert rouge_n("a a a", "a a", 2) == (one, 1.0, 1.0)
    assert rouge_n("a", "a b", 2) == (0.0, 0.0, 0.0), "a one-token hypothesis has no bigram: P = 0, F = 0"
    assert rouge_n("a b", "a", 2) == (0.0, 0.0, 0.0), "a one-token reference has none either: R = 0"
    assert rouge_n(["a", "b"], [], 1) == (0.0, 0.0, 0.0) and rouge_n([], [], 1) == (0.0, 0.0, 0.0), "an empty reference set: |R| = 0, R = 0.0"
    assert rouge_n([], ["a"], 1) == (0.0, 0.0, 0.0)
    # x y x y z against q x y z: E = {xy, yx, yz}, R = {qx, xy, yz}, o = 2
    p = r = 2 / 3
    assert rouge_n("x y x y z", "q x y z", 2) == (2.0 * ((p * r) / (p + r + 1e-8)), p, r)
    assert rouge_n("x y x y z", "q x y z", 1) == (2.0 * ((1.0 * 0.75) / (1.0 + 0.75 + 1e-8)), 1.0, 0.75)
    for bad in (0, -1, 1.0):
        with pytest.raises(ValueError, match="n must be"):
            rouge_n("a", "a", bad)


def test_f_is_symmetric_exactly():
    from case_rg_amd.evaluation import rouge_n
    rs = np.random.RandomState(431)
    nonzero = 0
    for case in range(300):
        x = rs.randint(0, (3, 6, 40)[case % 3], rs.randint(0, 30)).tolist()
        y = rs.randint(0, (3, 6, 40)[case % 3], rs.randint(0, 40)).tolist()
        for n in (1, 2, 3, 4):
            f, p, r = rouge_n(x, y, n)
            g, q, s = rouge_n(y, x, n)
            assert f == g and p == s and r == q, (x, y, n)
            nonzero += f > 0
    assert nonzero > 300


# ---------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------
def test_header_table_and_library_carry_the_two_exports():
    from case_rg_amd import _abi
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for name, nargs in (("case_ngram_distinct", 7), ("case_rouge_n_scores", 14)):
        proto = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, text, flags=re.S)
        assert proto, "%s is not declared in include/case_hip.h" % name
        assert len([a for a in proto.group(1).split(",") if a.strip()]) == nargs == len(_abi.SIGNATURES[name])
        assert hasattr(lib, name), "libcase_hip.so does not export %s" % name
    assert "const int64_t* b, const int32_t* b_len, int32_t* distinct, int64_t rows, int64_t Tb, int32_t max_n" in " ".join(text.split())
    assert _abi.FEAT_ROUGE_N == 1 << 31 and re.search(r"CASE_FEAT_ROUGE_N\s*=\s*1u\s*<<\s*31", text)
    assert re.search(r"CASE_FEAT_ROUGE_N[^\n]*\n?[^\n]*LAST free bit", raw), "the header says that the mask is full"
    assert _abi.lib.case_abi_features() & _abi.FEAT_ROUGE_N
    assert _abi.FEAT_RISK_TRAIN == 1 << 30 and _abi.FEAT_NGRAM_COUNTS == 1 << 23, "the earlier bits stay where they were"
    assert len(_abi.SIGNATURES["case_ngram_counts"]) == 16 and len(_abi.SIGNATURES["case_bleu_scores"]) == 13, "K34 / K35 keep their signatures"
    assert _abi.lib.case_version() == _abi.ABI_VERSION == 600, "nothing existing changed layout: the generation stays"


def test_exports_validate_before_any_launch():
    from case_rg_amd import _abi
    with pytest.raises(RuntimeError, match="case_ngram_distinct"):
        _abi.call("case_ngram_distinct", None, None, None, 1, 8, 4, None)
    buf = (ctypes.c_int64 * 8)()  # never dereferenced: every call below is refused before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    for rows, Tb, max_n in ((0, 8, 4), (1, 0, 4), (1, 8, 0), (1, 8, 5), (1 << 31, 8, 4), (1, 1 << 30, 4)):
        with pytest.raises(RuntimeError, match="case_ngram_distinct"):
            _abi.call("case_ngram_distinct", p, p, p, rows, Tb, max_n, None)
    with pytest.raises(RuntimeError, match="case_rouge_n_scores"):
        _abi.call("case_rouge_n_scores", *([None] * 9), 1, 1, 1, 4, None)
    for B, N, M, max_n in ((0, 1, 1, 4), (1, 0, 1, 4), (1, 1, 0, 4), (1, 1, 1, 0), (1, 1, 1, 5), (1 << 20, 1 << 12, 1, 4)):
        with pytest.raises(RuntimeError, match="case_rouge_n_scores"):
            _abi.call("case_rouge_n_scores", *([p] * 9), B, N, M, max_n, None)


def test_ops_check_their_arguments_before_the_library_is_called():
    from case_rg_amd import ops
    assert ops.rouge_n_supported()
    b, n = torch.zeros(2, 3, 9, dtype=torch.int64), torch.ones(2, 3, dtype=torch.int32)
    with pytest.raises(TypeError, match="int64"):
        ops.ngram_distinct(b.int(), n)
    with pytest.raises(TypeError, match="int64"):
        ops.ngram_distinct(torch.zeros(9, dtype=torch.int64), torch.ones((), dtype=torch.int32))
    with pytest.raises(TypeError, match="b_len"):
        ops.ngram_distinct(b, n.long())
    with pytest.raises(TypeError, match="b_len"):
        ops.ngram_distinct(b, n[:, :2])
    for bad in (0, 5, 2.0, True):
        with pytest.raises(ValueError, match="max_n"):
            ops.ngram_distinct(b, n, max_n=bad)
    with pytest.raises(ValueError, match="at least one row"):
        ops.ngram_distinct(b[:0], n[:0])
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.ngram_distinct(b, n)  # everything checked: only now would the library be called
    hit, e = torch.zeros(2, 3, 2, 4, dtype=torch.int32), torch.zeros(2, 3, 4, dtype=torch.int32)
    d, m = torch.zeros(2, 2, 4, dtype=torch.int32), torch.ones(2, 2, dtype=torch.int32)
    with pytest.raises(TypeError, match="hit must be"):
        ops.rouge_n_scores(hit.long(), e, d, m)
    with pytest.raises(TypeError, match="b_len must be"):
        ops.rouge_n_scores(hit, e, d, m.long())
    with pytest.raises(TypeError, match="ref_distinct must be"):
        ops.rouge_n_scores(hit, e, d[0], m)
    for wrong in (dict(hit=hit[:, :, :1]), dict(e=e[:, :2]), dict(d=d[..., :3]), dict(m=m[:1])):
        args = dict(hit=hit, e=e, d=d, m=m)
        args.update(wrong)
        with pytest.raises(TypeError, match=r"hit \[B, N, M, 4\]"):
            ops.rouge_n_scores(args["hit"], args["e"], args["d"], args["m"])
    for bad in (0, 5, 2.0):
        with pytest.raises(ValueError, match="max_n"):
            ops.rouge_n_scores(hit, e, d, m, max_n=bad)
    with pytest.raises(ValueError, match="at least one item"):
        ops.rouge_n_scores(hit[:0], e[:0], d[:0], m[:0])
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.rouge_n_scores(hit, e, d, m)


def test_ids_functions_check_their_arguments():
    from case_rg_amd import evaluation
    ids = torch.zeros(2, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="up to 256 positions"):
        evaluation.rouge_n_ids(torch.zeros(2, 257, dtype=torch.int64), ids, SPECIALS)
    with pytest.raises(ValueError, match="hypothesis items"):
        evaluation.rouge_n_ids(ids, ids[:1], SPECIALS)
    with pytest.raises(TypeError, match="int64"):
        evaluation.rouge_n_ids(ids.int(), ids, SPECIALS)
    for bad in (0, 5, 2.0):
        with pytest.raises(ValueError, match="max_n"):
            evaluation.rouge_n_ids(ids, ids, SPECIALS, max_n=bad)
    with pytest.raises(TypeError, match="one answer per item"):
        evaluation.eval_rouge_n_ids(ids.unsqueeze(1), ids, SPECIALS)
    for bad in ((0,), (1, 5), (2.0,), ()):
        with pytest.raises(ValueError, match="order"):
            evaluation.eval_rouge_n_ids(ids, ids, SPECIALS, orders=bad)


# ---------------------------------------------------------------------------------------------
# the trainer and consensus
# ---------------------------------------------------------------------------------------------
def test_orders_and_metric_names_are_refused_before_the_model_is_called():
    from case_rg_amd.common.Constants import BOS_WORD, EOS_WORD, PAD_WORD, UNK_WORD
    from case_rg_amd.common.CumulativeTrainer import CumulativeTrainer

    class Reached(Exception):
        pass

    class Stub(torch.nn.Module):
        vocab2id = {PAD_WORD: 0, BOS_WORD: 1, EOS_WORD: 2, UNK_WORD: 3}
        calls = 0

        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def forward(self, data, method):
            Stub.calls += 1
            raise Reached

    class OneItem(torch.utils.data.Dataset):
        def __len__(self):
            return 1

        def __getitem__(self, i):
            return {"response": torch.zeros(4, dtype=torch.int64)}

    collate = lambda items: {"response": torch.stack([x["response"] for x in items])}  # noqa: E731
    trainer = CumulativeTrainer(Stub(), None, None, None, 1)
    trainer.model.train()
    for bad in ((0,), (1, 5), (2.0,), ("1",)):
        with pytest.raises(ValueError, match="orders in 1..4"):
            trainer.evaluate_rouge(OneItem(), collate, 2, orders=bad)
    for bad in (("rouge_1", "rouge_3"), ("rouge_n",), ("ROUGE_1",), ()):
        with pytest.raises(ValueError, match="metrics must name"):
            trainer.evaluate_generation(OneItem(), collate, 2, metrics=bad)
    assert Stub.calls == 0 and trainer.model.training
    assert CumulativeTrainer.GENERATION_METRICS == ("rouge_l", "bleu", "meteor"), "the default tuple stays"
    # good orders and good names do reach the model
    for call in (lambda: trainer.evaluate_rouge(OneItem(), collate, 2, orders=(1, 2)),
                 lambda: trainer.evaluate_generation(OneItem(), collate, 2, metrics=("rouge_1", "rouge_2", "rouge_l"))):
        before = Stub.calls
        with pytest.raises(Reached):
            call()
        assert Stub.calls == before + 1 and trainer.model.training, "the mode is restored"


def test_consensus_takes_the_two_names_through_the_existing_check():
    import case_rg_amd
    from case_rg_amd import evaluation
    from case_rg_amd.evaluation.rouge_ids import CONSENSUS_METRICS
    from case_rg_amd.utils import make_vocab
    assert CONSENSUS_METRICS[:2] == ("rouge_l", "bleu") and set(CONSENSUS_METRICS) == {"rouge_l", "bleu", "rouge_1", "rouge_2"}
    with pytest.raises(ValueError, match="metric must be one of"):
        evaluation.consensus(torch.zeros(2, 4, 8, dtype=torch.int64), SPECIALS, metric="rouge_3")
    with pytest.raises(RuntimeError, match="GPU only"):
        evaluation.consensus(torch.zeros(2, 4, 8, dtype=torch.int64), SPECIALS, metric="rouge_2")
    ns = case_rg_amd.namespace()
    v2i, i2v = make_vocab(200)

    class Reached(Exception):
        pass

    for model in (ns.CaSE(4, 5, i2v, v2i, 32), ns.Masque(5, i2v, v2i, 32)):
        model.eval()
        seen = {}

        def do_sample(data, **kw):
            seen.update(kw)
            raise Reached

        model.do_sample = do_sample
        with pytest.raises(ValueError, match="metric must be one of"):
            model.do_consensus({}, metric="rouge_3")
        assert not seen, "the metric is checked before the pool is decoded"
        for metric in ("rouge_1", "rouge_2"):
            seen.clear()
            with pytest.raises(Reached):
                model.do_consensus({}, metric=metric, seed=3)
            assert seen["seed"] == 3 and "metric" not in seen
