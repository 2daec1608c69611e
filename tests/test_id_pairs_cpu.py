"""The one argument check of the pair ops on token ids (``ops.lcs_pairs``, ``ops.ngram_counts``, ``ops.meteor``) and the one prologue of the
``evaluation.*_ids`` front ends: one table of malformed inputs, every op refusing each entry with the same exception type and its own name
in front, before the library is called.  No GPU needed."""
import pytest
import torch

SPECIALS = (1, 0, 2, 3)  # bos, pad, eos, unk


@pytest.fixture
def no_library(monkeypatch):
    """Any call into the library fails the test: the checks come first."""
    from case_rg_amd import _abi

    def call(name, *args):
        raise AssertionError("%s was called with malformed operands" % name)

    monkeypatch.setattr(_abi, "call", call)


def _good():
    a, n = torch.zeros(2, 3, 8, dtype=torch.int64), torch.ones(2, 3, dtype=torch.int32)
    b, m = torch.zeros(2, 4, 9, dtype=torch.int64), torch.ones(2, 4, dtype=torch.int32)
    return a, n, b, m


# name -> (the malformed (a, a_len, b, b_len) from a well-formed one, the exception, a phrase of its message)
MALFORMED = {
    "int32 ids": (lambda a, n, b, m: (a.int(), n, b, m), TypeError, "int64"),
    "float references": (lambda a, n, b, m: (a, n, b.float(), m), TypeError, "int64"),
    "2-D ids": (lambda a, n, b, m: (a[:, 0], n, b, m), TypeError, "int64"),
    "ids that are no tensor": (lambda a, n, b, m: (a.tolist(), n, b, m), TypeError, "int64"),
    "another batch": (lambda a, n, b, m: (a, n, b[:1], m[:1]), TypeError, "one batch"),
    "a_len of another shape": (lambda a, n, b, m: (a, n[:, :2], b, m), TypeError, "lengths"),
    "b_len of another shape": (lambda a, n, b, m: (a, n, b, m.view(-1)), TypeError, "lengths"),
    "int64 lengths": (lambda a, n, b, m: (a, n.long(), b, m), TypeError, "lengths"),
    "lengths that are no tensor": (lambda a, n, b, m: (a, n, b, m.tolist()), TypeError, "lengths"),
    "Ta = 257": (lambda a, n, b, m: (torch.zeros(2, 3, 257, dtype=torch.int64), n, b, m), ValueError, "up to 256 positions"),
    "lengths on another device": (lambda a, n, b, m: (a, n.to("meta"), b, m), ValueError, "one device"),
    "references on another device": (lambda a, n, b, m: (a, n, b.to("meta"), m.to("meta")), ValueError, "one device"),
    "an empty batch": (lambda a, n, b, m: (a[:0], n[:0], b[:0], m[:0]), ValueError, "at least one"),
    "no reference": (lambda a, n, b, m: (a, n, b[:, :0], m[:, :0]), ValueError, "at least one"),
    "no position": (lambda a, n, b, m: (a[:, :, :0], n, b, m), ValueError, "at least one"),
}
PAIR_OPS = ("lcs_pairs", "ngram_counts", "meteor")


@pytest.mark.parametrize("case", sorted(MALFORMED))
@pytest.mark.parametrize("op", PAIR_OPS)
def test_pair_ops_refuse_malformed_operands_alike(no_library, op, case):
    from case_rg_amd import ops
    spoil, error, phrase = MALFORMED[case]
    with pytest.raises(error, match=phrase) as caught:
        getattr(ops, op)(*spoil(*_good()))
    assert str(caught.value).startswith(op + ": ")


@pytest.mark.parametrize("op", PAIR_OPS)
def test_well_formed_operands_pass_every_check(op):
    """The table spoils one thing at a time: unspoilt, the operands reach the library (which is GPU only), also as non-contiguous views and at
    the limit of 256 positions."""
    from case_rg_amd import ops
    a, n, b, m = _good()
    wide = torch.zeros(2, 3, 512, dtype=torch.int64)
    for operands in ((a, n, b, m), (wide[:, :, ::2], n.t().contiguous().t(), b, m)):
        with pytest.raises(RuntimeError, match="GPU only"):
            getattr(ops, op)(*operands)
    assert ops.LCS_MAX_T == ops.NGRAM_MAX_T == ops.METEOR_MAX_T == 256


@pytest.mark.parametrize("op, name", zip(PAIR_OPS, ("case_lcs_pairs", "case_ngram_counts", "case_meteor")))
def test_the_library_gets_the_five_sizes_in_its_order(monkeypatch, op, name):
    """B, N, M, Ta, Tb as include/case_hip.h declares them (five different numbers here), and outputs of those sizes."""
    from case_rg_amd import _abi, ops
    seen = {}
    monkeypatch.setattr(ops, "_ptr", lambda t, offset_elems=0: t)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(_abi, "call", lambda called, *args: seen.update(name=called, args=args))
    out = getattr(ops, op)(*_good())
    sizes = [x for x in seen["args"] if isinstance(x, int) and not isinstance(x, bool)]
    assert seen["name"] == name and sizes[-5 - (op == "ngram_counts"):][:5] == [2, 3, 4, 8, 9]
    first = out[0] if op == "lcs_pairs" else out["clip" if op == "ngram_counts" else "counts"]
    assert tuple(first.shape[:3]) == (2, 3, 4)
    if op == "meteor":
        monkeypatch.setattr(_abi, "call", lambda called, *args: None)
        assert tuple(ops.meteor(*_good(), want_align=True)["align"].shape) == (2, 3, 4, 8)


def test_max_n_is_an_int_and_no_bool(no_library):
    from case_rg_amd import ops
    a, n, b, m = _good()
    counts = dict(clip=torch.zeros(2, 3, 2, 4, dtype=torch.int32), clip_any=torch.zeros(2, 3, 4, dtype=torch.int32))
    for bad in (True, False, 0, 5, 2.0, None):
        for name, call in (("ngram_counts", lambda: ops.ngram_counts(a, n, b, m, max_n=bad)),
                           ("bleu_scores", lambda: ops.bleu_scores(counts, n, m, max_n=bad)),
                           ("ngram_distinct", lambda: ops.ngram_distinct(b, m, max_n=bad))):
            with pytest.raises(ValueError, match="max_n") as caught:
                call()
            assert str(caught.value).startswith(name + ": ")


def _front_ends():
    from case_rg_amd import evaluation
    return {name: getattr(evaluation, name) for name in ("rouge_l_ids", "bleu_ids", "ngram_overlap_ids", "meteor_ids", "rouge_n_ids")}


# name -> ((hyp, ref), the exception, a phrase of its message)
IDS = torch.zeros(2, 8, dtype=torch.int64)
MALFORMED_ROWS = {
    "another number of items": ((IDS, IDS[:1]), ValueError, "2 .* items, 1 .* items"),
    "T = 257": ((torch.zeros(2, 257, dtype=torch.int64), IDS), ValueError, "up to 256 positions"),
    "float hypotheses": ((IDS.float(), IDS), TypeError, "hyp must be an int64 tensor"),
    "float references": ((IDS, IDS.unsqueeze(1).float()), TypeError, "must be an int64 tensor"),
    "4-D hypotheses": ((IDS.view(2, 2, 2, 2), IDS), TypeError, "hyp must be an int64 tensor"),
}


@pytest.mark.parametrize("case", sorted(MALFORMED_ROWS))
@pytest.mark.parametrize("name", ("rouge_l_ids", "bleu_ids", "ngram_overlap_ids", "meteor_ids", "rouge_n_ids"))
def test_front_ends_refuse_malformed_rows_alike(no_library, name, case):
    (hyp, ref), error, phrase = MALFORMED_ROWS[case]
    with pytest.raises(error, match=phrase) as caught:
        _front_ends()[name](hyp, ref, SPECIALS)
    assert str(caught.value).startswith(name + ": ")


def test_overlap_speaks_of_answers_and_sources(no_library):
    from case_rg_amd.evaluation import ngram_overlap_ids, rouge_l_ids
    with pytest.raises(ValueError, match="2 answer items, 1 source items"):
        ngram_overlap_ids(IDS, IDS[:1], SPECIALS)
    with pytest.raises(ValueError, match="answers of up to 256 positions"):
        ngram_overlap_ids(torch.zeros(2, 257, dtype=torch.int64), IDS, SPECIALS)
    with pytest.raises(TypeError, match="source must be an int64 tensor"):
        ngram_overlap_ids(IDS, IDS.float(), SPECIALS)
    with pytest.raises(ValueError, match="2 hypothesis items, 1 reference items"):
        rouge_l_ids(IDS, IDS[:1], SPECIALS)
    with pytest.raises(TypeError, match="ref must be an int64 tensor"):
        rouge_l_ids(IDS, IDS.float(), SPECIALS)
