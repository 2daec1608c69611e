"""The n-gram ban without a GPU: argument checks of the public surface, the pure-Python restatement of the ban rule (the one the GPU tests
import) against hand-written cases, and the new exports in the header and the ctypes table."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("case_pointer_head_decode_ban", "case_pointer_head_beam_ban", "case_pointer_head_sample_ban", "case_beam_advance_ban",
               "case_ngram_ban", "case_remove_duplicate_ids")


def _model(kind, T):
    from case_rg_amd.CaSE.Model import CaSE
    from case_rg_amd.Masque.Model import Masque
    from case_rg_amd.utils import make_vocab
    v2i, i2v = make_vocab(120)
    return CaSE(4, T, i2v, v2i, 16, enc_layers=1, dec_layers=1, heads=2) if kind == "case" else Masque(T, i2v, v2i, 16, enc_layers=1, dec_layers=1, heads=2)


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_attribute_defaults_to_off_and_bad_values_raise_before_any_work(kind):
    """The checks run before the batch is touched: ``data`` is None here."""
    m = _model(kind, 12).eval()
    assert m.no_repeat_ngram == 0
    for call in (m.do_test, m.do_beam, m.do_sample, m.do_consensus):
        for bad in (-1, 2.5, 3.0, "3", True, [3]):
            with pytest.raises(ValueError, match="no_repeat_ngram"):
                call(None, no_repeat_ngram=bad)
    m.no_repeat_ngram = -2  # None = the attribute
    for method in ("test", "beam", "sample", "consensus"):
        with pytest.raises(ValueError, match="no_repeat_ngram"):
            m(None, method=method)


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_more_than_256_steps_with_the_ban_on_raise(kind):
    m = _model(kind, 257).eval()
    for call in (m.do_test, m.do_beam, m.do_sample, m.do_consensus):
        with pytest.raises(ValueError, match="256"):
            call(None, no_repeat_ngram=3)
    m.no_repeat_ngram = 1
    with pytest.raises(ValueError, match="256"):
        m(None, method="test")


def test_the_checked_parameter():
    from case_rg_amd.common.TransformerSeqEncoderDecoder import no_repeat_ngram_param
    assert no_repeat_ngram_param(0, 1000) == 0  # off: no limit on the pass
    assert no_repeat_ngram_param(3, 256) == 3
    assert no_repeat_ngram_param(300, 24) == 300  # n > max_target_length is legal (and bans nothing)
    with pytest.raises(ValueError):
        no_repeat_ngram_param(1, 257)
    for bad in (-1, 1.0, "1", None, True):
        with pytest.raises(ValueError):
            no_repeat_ngram_param(bad, 24)


def test_restated_rule_on_hand_written_cases():
    from case_rg_amd.common.Utils import banned_tokens as ban
    # n = 1: every token of the history
    assert ban([], 1) == [] and ban([5], 1) == [5] and ban([7, 5, 7, 9], 1) == [5, 7, 9]
    # n = 2: what followed an earlier occurrence of the last token
    assert ban([5], 2) == []                      # t < n
    assert ban([5, 6], 2) == []                   # the suffix [6] occurs at j = 1 only, and j <= t - n = 0
    assert ban([5, 6, 5], 2) == [6]
    assert ban([5, 6, 5, 7, 5], 2) == [6, 7]
    assert ban([5, 5], 2) == [5]                  # the window at j = t - n overlaps the suffix
    # n = 3
    assert ban([1, 2, 3, 1, 2], 3) == [3]
    assert ban([1, 2, 3, 4, 1, 2, 9, 1, 2], 3) == [3, 9]
    assert ban([1, 2, 3, 2, 1], 3) == []
    assert ban([4, 4, 4], 3) == [4]
    assert ban([1, 2], 3) == [] and ban([1, 2, 1], 3) == []
    # a history that holds EOS gets no ban; ids outside the vocabulary are ignored; n > t bans nothing
    assert ban([1, 2, 3, 1, 2], 3, eos=3) == [] and ban([1, 2, 3, 1, 2], 3, eos=8) == [3]
    assert ban([1, 300, 1], 2, vocab_size=200) == [] and ban([1, 300, 1], 2, vocab_size=301) == [300]
    assert ban([300, 2, 300], 2, vocab_size=200) == [2]
    assert ban([1, 2, 3], 30) == [] and ban([1, 2, 3], 0) == []


def test_new_exports_in_the_header_and_the_ctypes_table():
    from case_rg_amd import _abi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "case_hip.h")).read(), flags=re.S)
    for name in NEW_EXPORTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), "%s is not declared" % name
        assert name in _abi.SIGNATURES and hasattr(_abi.lib, name)
    assert "CASE_FEAT_NGRAM_BAN = 1u << 22" in open(os.path.join(ROOT, "include", "case_hip.h")).read()
    assert _abi.FEAT_NGRAM_BAN == 1 << 22 and _abi.lib.case_abi_features() & _abi.FEAT_NGRAM_BAN
    # the existing prototypes keep their argument lists
    assert len(_abi.SIGNATURES["case_pointer_head_decode"]) == 14 and len(_abi.SIGNATURES["case_beam_advance"]) == 18
    assert len(_abi.SIGNATURES["case_pointer_head_beam"]) == 15 and len(_abi.SIGNATURES["case_pointer_head_sample"]) == 28


def test_argument_checks_of_the_new_entry_points_happen_before_any_launch():
    from case_rg_amd import _abi
    with pytest.raises(RuntimeError, match="case_ngram_ban"):
        _abi.call("case_ngram_ban", None, None, None, 0, 0, 0, 0, 0, -1, None)
    with pytest.raises(RuntimeError, match="case_remove_duplicate_ids"):
        _abi.call("case_remove_duplicate_ids", None, None, 0, 0, 3, 0, None)
