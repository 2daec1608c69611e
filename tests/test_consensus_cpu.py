"""Consensus answer selection, CPU side: the two new exports in the header, the ctypes table and the built library; the limits of
``ops.consensus_supported``; a pure-Python restatement of the pick (``restated_pick``: ``evaluation.rouge_l`` over token lists, the self
term, weights, the validity mask and the lowest-index tie rule) on a hand-made pool; and the argument checks that need no GPU.
tests/test_consensus_gpu.py holds the kernels and the models against this restatement."""
import ctypes
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "case_hip.h")


def restated_pick(pool, weights=None, valid=None):
    """pool: N token lists (``to_sentence``'s: an empty answer is already [UNK]) -> (utility [N], index, pairwise F [N][N]).
    utility[n] = sum_m w[m] F(pool[n] as the hypothesis, pool[m] as the reference) / sum_m w[m] over the valid m, the self term included,
    -inf for an invalid n; index = the first maximum (0 when nothing is valid)."""
    from case_rg_amd.evaluation import rouge_l
    N = len(pool)
    weights = [1.0] * N if weights is None else [float(w) for w in weights]
    valid = [True] * N if valid is None else [bool(v) for v in valid]
    f = [[rouge_l(pool[n], pool[m])[0] for m in range(N)] for n in range(N)]
    den = sum(weights[m] for m in range(N) if valid[m])
    utility = [sum(weights[m] * f[n][m] for m in range(N) if valid[m]) / den if valid[n] else -math.inf for n in range(N)]
    index = 0
    for n in range(N):
        if utility[n] > utility[index]:
            index = n
    return utility, index, f


def test_header_table_and_library_carry_the_two_exports():
    from case_rg_amd import _abi
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for name, nargs in (("case_lcs_pairs", 12), ("case_consensus_pick", 11)):
        proto = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, text, flags=re.S)
        assert proto, "%s is not declared in include/case_hip.h" % name
        assert len([a for a in proto.group(1).split(",") if a.strip()]) == nargs == len(_abi.SIGNATURES[name])
        assert hasattr(lib, name), "libcase_hip.so does not export %s" % name
    assert _abi.FEAT_CONSENSUS == 1 << 21 and re.search(r"CASE_FEAT_CONSENSUS\s*=\s*1u\s*<<\s*21", text)
    assert _abi.lib.case_abi_features() & _abi.FEAT_CONSENSUS
    assert _abi.lib.case_version() == _abi.ABI_VERSION == 600, "nothing existing changed layout: the generation stays"


def test_exports_validate_before_any_launch():
    """Null pointers, non-positive counts and a hypothesis side beyond 256 positions are refused on the host side of the ABI."""
    from case_rg_amd import _abi
    with pytest.raises(RuntimeError, match="case_lcs_pairs"):
        _abi.call("case_lcs_pairs", None, None, None, None, None, None, 1, 1, 1, 8, 8, None)
    buf = (ctypes.c_int64 * 8)()  # never dereferenced: every call below is refused before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    for B, N, M, Ta in ((0, 1, 1, 8), (1, 0, 1, 8), (1, 1, 0, 8), (1, 1, 1, 257)):
        with pytest.raises(RuntimeError, match="case_lcs_pairs"):
            _abi.call("case_lcs_pairs", p, p, p, p, p, p, B, N, M, Ta, 8, None)
    with pytest.raises(RuntimeError, match="case_consensus_pick"):
        _abi.call("case_consensus_pick", None, None, None, None, None, None, None, 1, 1, 1, None)
    for B, N, T in ((0, 4, 8), (1, 0, 8), (1, 65, 8), (1, 4, 0)):
        with pytest.raises(RuntimeError, match="case_consensus_pick"):
            _abi.call("case_consensus_pick", p, None, None, p, p, p, p, B, N, T, None)


def test_consensus_supported_at_its_limits():
    from case_rg_amd import ops
    assert ops.consensus_supported(64, 256) and ops.consensus_supported(1, 1)
    assert not ops.consensus_supported(65, 64)
    assert not ops.consensus_supported(8, 257)


def test_restated_pick_on_a_hand_made_pool():
    """Candidate 1 shares the most with the other three; the outlier never wins; weights, the mask and ties act as stated."""
    from case_rg_amd.evaluation import rouge_l
    pool = ["the cat sat on the mat".split(), "the cat sat on a mat".split(), "a cat sat on a mat".split(), "dogs bark".split()]
    utility, index, f = restated_pick(pool)
    assert index == 1, utility
    assert all(f[n][n] == rouge_l(pool[n], pool[n])[0] and abs(f[n][n] - 1.0) < 1e-9 for n in range(4)), "the self term is the F of a full match"
    assert abs(utility[1] - sum(f[1]) / 4) < 1e-15 and utility[3] == min(utility)
    assert f[0][1] == rouge_l(pool[0], pool[1])[0] and abs(f[0][1] - 5 / 6) < 1e-9  # lcs 5 of 6 and 6 tokens
    # the outlier wins once the weight is (almost) all its own
    assert restated_pick(pool, weights=[1e-3, 1e-3, 1e-3, 1.0])[1] == 3
    # an invalid candidate is neither picked nor counted: without 1, candidates 0 and 2 each keep one close neighbour less
    u, i, _ = restated_pick(pool, valid=[True, False, True, True])
    assert u[1] == -math.inf and i in (0, 2) and abs(u[0] - (f[0][0] + f[0][2] + f[0][3]) / 3) < 1e-15
    # exact ties go to the lowest index; nothing valid gives index 0
    assert restated_pick([["x", "y"], ["x", "y"], ["z"]])[1] == 0
    assert restated_pick([["z"], ["x", "y"], ["x", "y"]])[1] == 1
    assert restated_pick(pool, valid=[False] * 4)[1] == 0


def test_do_consensus_is_refused_in_train_mode_and_checks_its_arguments():
    """Eval mode only, and the pool's range, checked before anything is launched (no GPU needed to see it)."""
    import torch
    import case_rg_amd
    from case_rg_amd import evaluation
    from case_rg_amd.utils import make_vocab
    ns = case_rg_amd.namespace()
    v2i, i2v = make_vocab(200)
    for model in (ns.CaSE(4, 5, i2v, v2i, 32), ns.Masque(5, i2v, v2i, 32)):
        assert model.consensus_samples == 8
        model.train()
        with pytest.raises(ValueError, match="eval mode"):
            model.do_consensus({})
        with pytest.raises(ValueError, match="eval mode"):
            model({}, method="consensus")
        model.eval()
        with pytest.raises(ValueError, match="pool must be"):
            model.do_consensus({}, pool="greedy")
    for shape in ((2, 65, 8), (2, 4, 257)):
        with pytest.raises(ValueError, match="pools of up to 64 candidates of up to 256 positions"):
            evaluation.consensus(torch.zeros(shape, dtype=torch.int64), (1, 0, 2, 3))
    with pytest.raises(ValueError, match="up to 256 positions"):
        evaluation.rouge_l_ids(torch.zeros(2, 257, dtype=torch.int64), torch.zeros(2, 8, dtype=torch.int64), (1, 0, 2, 3))
