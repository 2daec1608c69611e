"""The threshold-free ranking figures of the supporting-token stage on the host: ``evaluation.token_rank.token_rank_host`` -- the yardstick
of K45 -- against rows worked by hand, a brute-force count over all (positive, negative) pairs, an exhaustive search over all cuts and
``evaluation.rank_metrics``' ``map``; the ABI entry of ``case_token_rank``; and the ``ValueError``s that are raised before a device is
touched.  Everything except the comparison with ``map`` (f64, 1e-12) is exact: integers and ``Fraction``s."""
import ctypes
import math
import os
import random
import re
from fractions import Fraction

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "case_hip.h")
INTS = ("n_valid", "n_pos", "n_neg", "auc_num2", "best_tp", "best_n", "n_groups")


def host(*args, **kwargs):
    from case_rg_amd.evaluation import token_rank_host
    return token_rank_host(*args, **kwargs)


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def threshold_bits(x):
    return torch.tensor(x, dtype=torch.float32).view(torch.int32).item()


# ---------------------------------------------------------------------------------------------
# 1. rows worked by hand
# ---------------------------------------------------------------------------------------------
def test_a_tie_free_row():
    # order 0.9+ 0.8- 0.7+ 0.6- 0.5-: five groups of one; n_pos 2, n_neg 3
    # ap  = (1 / 2) (1 * 1 / 1 + 1 * 2 / 3) = 5 / 6
    # auc: the first positive beats 3 negatives, the second 2: num2 = 2 * 3 + 2 * 2 = 10, auc = 10 / (2 * 2 * 3) = 5 / 6
    # 2 tp / (n + n_pos) per cut: 2/3, 2/4, 4/5, 4/6, 4/7 -> the third: tp 2, n 3, the score 0.7
    got = host([0.5, 0.9, 0.6, 0.7, 0.8], [0, 1, 0, 1, 0])
    assert {k: got[k] for k in INTS} == dict(n_valid=5, n_pos=2, n_neg=3, auc_num2=10, best_tp=2, best_n=3, n_groups=5)
    assert got["ap"] == Fraction(5, 6) and got["auc"] == Fraction(5, 6) and got["best_f1"] == Fraction(4, 5)
    assert got["best_threshold"] == f32(0.7)


def test_a_row_that_is_one_group():
    # six positions of one score, two positives: one threshold, which takes everything
    # ap = (1 / 2) (2 * 2 / 6) = 1 / 3 = n_pos / n_valid;  num2 = 2 (2 (4 - 4) + 4) = 8, auc = 8 / (2 * 2 * 4) = 1 / 2
    got = host([0.25] * 6, [1, 0, 0, 1, 0, 0])
    assert {k: got[k] for k in INTS} == dict(n_valid=6, n_pos=2, n_neg=4, auc_num2=8, best_tp=2, best_n=6, n_groups=1)
    assert got["ap"] == Fraction(2, 6) and got["auc"] == Fraction(1, 2) and got["best_f1"] == Fraction(4, 8) and got["best_threshold"] == 0.25


def test_a_mixed_tie_at_the_top():
    # groups: 2.0 (2 positives, 1 negative), 1.0 (1 positive), 0.0 (1 negative); n_pos 3, n_neg 2
    # ap  = (1 / 3) (2 * 2 / 3 + 1 * 3 / 4 + 0) = 25 / 36
    # num2 = 2 (2 (2 - 1) + 1) + 1 (2 (2 - 1) + 0) + 0 = 8, auc = 8 / 12 = 2 / 3
    #   (pairs: the two 2.0 positives tie one negative -- 2 halves -- and beat the other -- 2 --, the 1.0 positive loses one and wins one: 4 / 6)
    # cuts: 4 / 6, 6 / 7, 6 / 8 -> the second: tp 3, n 4, the score 1.0
    got = host([2.0, 2.0, 2.0, 1.0, 0.0], [1, 0, 1, 1, 0])
    assert {k: got[k] for k in INTS} == dict(n_valid=5, n_pos=3, n_neg=2, auc_num2=8, best_tp=3, best_n=4, n_groups=3)
    assert got["ap"] == Fraction(25, 36) and got["auc"] == Fraction(2, 3) and got["best_f1"] == Fraction(6, 7) and got["best_threshold"] == 1.0


def test_no_positives_and_all_positives():
    got = host([1.0, 2.0, 3.0], [0, 0, 0])
    assert {k: got[k] for k in INTS} == dict(n_valid=3, n_pos=0, n_neg=3, auc_num2=0, best_tp=0, best_n=0, n_groups=3)
    assert got["ap"] == 0 and got["auc"] is None and got["best_f1"] is None and got["best_threshold"] == math.inf
    # groups 2.0 (2 positives), 1.0 (1): ap = (1 / 3) (2 * 2 / 2 + 1 * 3 / 3) = 1; no negative: no pair; cuts 4 / 5, 6 / 6
    got = host([1.0, 2.0, 2.0], [1, 1, 1])
    assert {k: got[k] for k in INTS} == dict(n_valid=3, n_pos=3, n_neg=0, auc_num2=0, best_tp=3, best_n=3, n_groups=2)
    assert got["ap"] == 1 and got["auc"] is None and got["best_f1"] == 1 and got["best_threshold"] == 1.0


def test_an_all_invalid_row_and_holes():
    got = host([1.0, 2.0], [1, 0], [False, False])
    assert {k: got[k] for k in INTS} == dict(n_valid=0, n_pos=0, n_neg=0, auc_num2=0, best_tp=0, best_n=0, n_groups=0)
    assert got["ap"] == 0 and got["auc"] is None and got["best_threshold"] == math.inf
    # the invalid positions do not exist: the tie-free row above with three more positions struck out
    got = host([0.5, 9.0, 0.9, 0.6, 0.7, 0.7, 0.8, -1.0], [0, 1, 1, 0, 1, 0, 0, 1], [1, 0, 1, 1, 1, 0, 1, 0])
    assert got == host([0.5, 0.9, 0.6, 0.7, 0.8], [0, 1, 0, 1, 0])


def test_both_zeros_are_one_group():
    # groups: 1.0 (1 negative), 0.0 (1 positive, 1 negative): ap = 1 * 1 / 3; num2 = 1 (2 (2 - 2) + 1) = 1, auc = 1 / 4; cuts 0 / 2, 2 / 4
    got = host([0.0, -0.0, 1.0], [1, 0, 0])
    assert {k: got[k] for k in INTS} == dict(n_valid=3, n_pos=1, n_neg=2, auc_num2=1, best_tp=1, best_n=3, n_groups=2)
    assert got["ap"] == Fraction(1, 3) and got["auc"] == Fraction(1, 4) and got["best_f1"] == Fraction(1, 2)
    assert threshold_bits(got["best_threshold"]) == 0, "+0.0, whichever zero the positive carries"
    assert threshold_bits(host([-0.0, -0.0, 1.0], [1, 0, 0])["best_threshold"]) == 0


def test_nan_is_grouped_with_minus_infinity():
    # groups: 0.0 (1 negative), -inf (2 positives): ap = (1 / 2) (2 * 2 / 3) = 2 / 3; both positives lose their pair: auc 0; cuts 0 / 3, 4 / 5
    got = host([math.nan, -math.inf, 0.0], [1, 1, 0])
    assert {k: got[k] for k in INTS} == dict(n_valid=3, n_pos=2, n_neg=1, auc_num2=0, best_tp=2, best_n=3, n_groups=2)
    assert got["ap"] == Fraction(2, 3) and got["auc"] == 0 and got["best_f1"] == Fraction(4, 5) and got["best_threshold"] == -math.inf


def test_a_label_of_exactly_one_half_is_not_positive():
    got = host([3.0, 2.0, 1.0], [0.5, 1.0, 0.5000001])
    assert got["n_pos"] == 2 and got["n_neg"] == 1
    # order: - + +: ap = (1 / 2) (1 / 2 + 2 / 3) = 7 / 12, no positive beats the negative
    assert got["ap"] == Fraction(7, 12) and got["auc"] == 0


def test_shapes_and_containers():
    import numpy as np
    s, l, v = [[0.5, 0.9, 0.6], [1.0, 1.0, 0.0]], [[0, 1, 0], [1, 0, 1]], [[1, 1, 1], [1, 1, 0]]
    rows = host(s, l, v)
    assert isinstance(rows, list) and len(rows) == 2 and rows[0] == host(s[0], l[0], v[0]) and rows[1] == host(s[1], l[1], v[1])
    assert host(torch.tensor(s), torch.tensor(l, dtype=torch.float32), torch.tensor(v, dtype=torch.bool)) == rows
    assert host(np.asarray(s, dtype=np.float32), np.asarray(l), np.asarray(v, dtype=bool)) == rows
    assert host(s, l) == [host(s[0], l[0]), host(s[1], l[1])]
    # scores are f32: two f64 values that round to one f32 are one group
    assert host([1.0, 1.0 + 1e-12], [1, 0])["n_groups"] == 1
    with pytest.raises(ValueError, match="one shape"):
        host([1.0, 2.0], [1])


# ---------------------------------------------------------------------------------------------
# 2. properties on random rows
# ---------------------------------------------------------------------------------------------
def random_row(rng, S, values=None):
    """S positions; ``values`` distinct scores to draw from (None: all distinct), a fifth invalid, a third positive."""
    pool = [rng.uniform(-2, 2) for _ in range(values)] + [0.0, -0.0] if values else None
    scores = [rng.choice(pool) for _ in range(S)] if pool else rng.sample([i / 4 - 30 for i in range(4 * S)], S)
    return scores, [float(rng.random() < 1 / 3) for _ in range(S)], [rng.random() < 0.8 for _ in range(S)]


def tied_rows(seed, n=40):
    rng = random.Random(seed)
    return [random_row(rng, rng.randint(1, 200), values=rng.choice((1, 2, 3, 7, 20))) for _ in range(n)]


def test_auc_num2_counts_the_pairs():
    """2 for every (positive, negative) pair the positive wins, 1 for every tie, by brute force."""
    from case_rg_amd.evaluation.token_rank import canonical_score
    seen = 0
    for scores, labels, valid in tied_rows(451):
        got = host(scores, labels, valid)
        pos = [canonical_score(s) for s, l, v in zip(scores, labels, valid) if v and l > 0.5]
        neg = [canonical_score(s) for s, l, v in zip(scores, labels, valid) if v and not l > 0.5]
        assert got["auc_num2"] == sum(2 * (p > q) + (p == q) for p in pos for q in neg)
        assert (got["n_pos"], got["n_neg"]) == (len(pos), len(neg))
        if pos and neg:
            assert got["auc"] == Fraction(got["auc_num2"], 2 * len(pos) * len(neg))
            seen += 1
        else:
            assert got["auc"] is None
    assert seen >= 20, "the rows prove nothing"


def test_nothing_depends_on_the_position():
    rng = random.Random(452)
    for scores, labels, valid in tied_rows(453):
        order = list(range(len(scores)))
        rng.shuffle(order)
        pick = lambda x: [x[i] for i in order]  # noqa: E731
        assert host(pick(scores), pick(labels), pick(valid)) == host(scores, labels, valid)


def test_the_best_cut_is_the_exhaustive_maximum():
    """Every group end tried, fractions exact, the first (highest score) among equals."""
    from case_rg_amd.evaluation.token_rank import canonical_score
    seen = 0
    for scores, labels, valid in tied_rows(454) + [random_row(random.Random(455 + i), 50) for i in range(10)]:
        got = host(scores, labels, valid)
        kept = sorted(((canonical_score(s), l > 0.5) for s, l, v in zip(scores, labels, valid) if v), key=lambda t: -t[0])
        n_pos = sum(p for _, p in kept)
        if n_pos == 0:
            assert (got["best_tp"], got["best_n"], got["best_threshold"], got["best_f1"]) == (0, 0, math.inf, None)
            continue
        cuts = []
        for n in range(1, len(kept) + 1):
            if n == len(kept) or kept[n][0] != kept[n - 1][0]:  # a group ends here
                cuts.append((Fraction(2 * sum(p for _, p in kept[:n]), n + n_pos), -n, kept[n - 1][0]))
        f1, neg_n, score = max(cuts)
        assert (got["best_f1"], got["best_n"], got["best_threshold"]) == (f1, -neg_n, score) and len(cuts) == got["n_groups"]
        assert got["best_f1"] == Fraction(2 * got["best_tp"], got["best_n"] + n_pos)
        seen += 1
    assert seen >= 30


def test_ap_is_trec_map_on_tie_free_rows():
    from case_rg_amd.evaluation import rank_metrics
    rng = random.Random(456)
    worst, seen = 0.0, 0
    for _ in range(30):
        scores, labels, valid = random_row(rng, rng.randint(1, 150))
        got = host(scores, labels, valid)
        if got["n_pos"] == 0:
            continue
        assert got["n_groups"] == got["n_valid"]
        run = {"q": {"d%04d" % i: s for i, (s, v) in enumerate(zip(scores, valid)) if v}}
        qrel = {"q": {"d%04d" % i: int(l > 0.5) for i, (l, v) in enumerate(zip(labels, valid)) if v}}
        want = rank_metrics(run, qrel)["q"]["map"]
        worst = max(worst, abs(float(got["ap"]) - want))
        seen += 1
    print("ap against rank_metrics' map on %d tie-free rows: max distance %.3e" % (seen, worst))
    assert seen >= 20 and worst <= 1e-12


# ---------------------------------------------------------------------------------------------
# 3. the ABI entry
# ---------------------------------------------------------------------------------------------
def test_abi_table_header_and_library_agree_on_case_token_rank():
    from case_rg_amd import _abi, ops
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    proto = re.search(r"\bint\s+case_token_rank\s*\((.*?)\);", text, flags=re.S).group(1)
    params = [" ".join(a.split()) for a in proto.split(",")]
    assert params == ["const float* scores", "const uint8_t* valid", "const float* labels", "double* stats", "int32_t* counts",
                      "float* threshold", "int64_t B", "int64_t S", "case_stream_t stream"]
    ptr, i64 = ctypes.c_void_p, ctypes.c_int64
    assert _abi.SIGNATURES["case_token_rank"] == [ptr] * 6 + [i64, i64, ptr]
    assert "case_token_rank" in _abi.OPTIONAL and _abi.ABI_VERSION == 600
    assert hasattr(ctypes.CDLL(_abi.LIB_PATH), "case_token_rank"), "libcase_hip.so does not export case_token_rank"
    assert _abi.has("case_token_rank") and ops.token_rank_supported()
    assert _abi.lib.case_token_rank.argtypes == _abi.SIGNATURES["case_token_rank"]
    assert ops.TOKEN_RANK_COUNTS == ("n_valid", "n_pos", "auc_num2", "best_tp", "best_n", "n_groups")


def test_the_c_entry_point_validates_before_any_launch():
    """No device is needed: every call here returns before the launch."""
    from case_rg_amd import _abi
    p = 1 << 20  # (never dereferenced)
    for B, S in ((1, 16385), (1, 0), (-1, 8), (0, 16385)):
        with pytest.raises(RuntimeError, match="case_token_rank"):
            _abi.call("case_token_rank", p, None, p, p, p, p, B, S, None)
    for missing in (0, 2, 3, 4, 5):
        args = [p, None, p, p, p, p]
        args[missing] = None
        with pytest.raises(RuntimeError, match="case_token_rank"):
            _abi.call("case_token_rank", *args, 2, 8, None)
    _abi.call("case_token_rank", None, None, None, None, None, None, 0, 8, None)  # no item: no launch, no error


# ---------------------------------------------------------------------------------------------
# 4. errors that come before a device is touched
# ---------------------------------------------------------------------------------------------
def test_ops_token_rank_raises_before_touching_a_device(monkeypatch):
    from case_rg_amd import _abi, ops
    monkeypatch.setattr(_abi, "call", lambda *a: pytest.fail("a launch was attempted"))
    s, ok = torch.zeros(2, 8), torch.ones(2, 8, dtype=torch.bool)
    with pytest.raises(ValueError, match="on the device"):
        ops.token_rank(s, ok, s)
    with pytest.raises(ValueError, match="on the device"):
        ops.token_rank(s, None, s)
    with pytest.raises(ValueError, match="1 .. 16384 positions"):
        ops.token_rank(torch.zeros(1, 16385), None, torch.zeros(1, 16385))
    with pytest.raises(ValueError, match="scores must be an f32"):
        ops.token_rank(s.double(), ok, s)
    with pytest.raises(ValueError, match="scores must be an f32"):
        ops.token_rank(s[0], ok[0], s[0])
    with pytest.raises(ValueError, match="valid must be bool"):
        ops.token_rank(s, ok[:, :7], s)
    with pytest.raises(ValueError, match="valid must be bool"):
        ops.token_rank(s, s, s)
    with pytest.raises(ValueError, match="labels must be float"):
        ops.token_rank(s, ok, s[:1])
    with pytest.raises(ValueError, match="labels must be float"):
        ops.token_rank(s, ok, ok)


def test_ops_token_rank_names_the_rebuild_where_the_library_lacks_the_symbol(monkeypatch):
    from case_rg_amd import _abi, ops
    monkeypatch.setattr(_abi, "has", lambda name: name != "case_token_rank")
    monkeypatch.setattr(_abi, "call", lambda *a: pytest.fail("a launch was attempted"))
    assert not ops.token_rank_supported()
    s = torch.zeros(2, 8)
    with pytest.raises(RuntimeError, match="lacks K45.*rebuild"):
        ops.token_rank(s, None, s)


def test_do_extract_ranking_without_labels_is_an_error():
    from case_rg_amd.CaSE.Model import CaSE
    from case_rg_amd.utils import make_vocab, synth_batch
    v2i, i2v = make_vocab(400)
    m = CaSE(4, 6, i2v, v2i, 32, enc_layers=1, dec_layers=1, heads=2).eval()
    batch = synth_batch(2, 3, 16, 8, 6, 400, seed=457, model="case")
    with pytest.raises(ValueError, match="ranking=True needs labels"):
        m.do_extract(batch, ranking=True)
    with pytest.raises(ValueError, match="eval mode"):
        m.train().do_extract(batch, labels=batch["token_label"], ranking=True)
