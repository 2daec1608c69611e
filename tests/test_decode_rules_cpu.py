"""The decoding rules (min_length, banned ids, the beam length penalty) without a GPU: the argument checker, the way the task models resolve
their keywords, and the pure-Python / float64 restatements that tests/test_decode_rules_gpu.py holds the kernels against.

The heads and ``ngram_ban_`` have no CPU form, so neither have the rules: there is nothing to run the restatement against here; it is
checked against hand-worked cases instead."""
import math

import numpy as np
import pytest
import torch


# ---------------------------------------------------------------------------------------------
# the restatements (imported by tests/test_decode_rules_gpu.py)
# ---------------------------------------------------------------------------------------------
def restate_rules(row, t, eos, min_length, banned):
    """One row (1-D NumPy array) after the rules of step ``t``: a copy with row[eos] = 0 while t < min_length and row[v] = 0 for every listed v
    inside [0, V).  Nothing else changes."""
    out = np.array(row, copy=True)
    V = out.shape[0]
    if t < min_length and 0 <= eos < V:
        out[eos] = 0.0
    for v in (banned if banned is not None else ()):
        v = int(v)
        if 0 <= v < V:
            out[v] = 0.0
    return out


def item_list(banned, row, rows_per_item):
    """The list of row ``row``: ``banned`` None, [K] (every item) or [items, K] (row r of item r // rows_per_item)."""
    if banned is None:
        return None
    banned = np.asarray(banned)
    return banned if banned.ndim == 1 else banned[row // rows_per_item]


def restate_rows(rows, t, eos, min_length, banned, rows_per_item=1):
    return np.stack([restate_rules(rows[r], t, eos, min_length, item_list(banned, r, rows_per_item)) for r in range(rows.shape[0])])


def ordered_top(row, W):
    """The ids of the W largest entries, the lowest id first among equals (K24's order; W = 1: K23's argmax)."""
    return np.lexsort((np.arange(row.size), -np.asarray(row, dtype=np.float64)))[:W]


def restate_beam(cand_p, cand_id, B, W, T, eos, alpha, zero_is_dead=True):
    """K25 over T steps in float64 and plain Python, from the planted candidates cand_p / cand_id [T, B * W, W] (row b * W + w = slot w of item b):
    candidate (w, j) of a live slot has cost = cum[w] - log(p + 1e-10) and key = cost / (len[w] + 1)^alpha (len counts BOS); a candidate of
    probability 0 is dead; the W smallest keys, stable in (w, j) order, become the new slots; a new slot whose token is ``eos``, and every new
    slot at the last step, retires into the pool (ascending by key, a newcomer behind its equals, the best W kept).
    -> per item: dict(keys, steps, slots: the pool best first, answers: the pool's hypotheses [n, T] with PAD (0) behind the end,
    gaps: the smallest relative distance between two different finite keys that were ever compared)."""
    out = []
    for b in range(B):
        alive, cum, length = [w == 0 for w in range(W)], [0.0] * W, [1] * W
        hist_parent, hist_token, pool, gap = [], [], [], float("inf")
        for t in range(T):
            cands = []
            for w in range(W):
                for j in range(W):
                    p = float(cand_p[t][b * W + w][j])
                    if not alive[w] or (zero_is_dead and p == 0.0):
                        continue
                    cost = cum[w] - math.log(p + 1e-10)
                    cands.append((cost / float(length[w] + 1) ** alpha, w, j, cost))
            order = sorted(range(len(cands)), key=lambda i: cands[i][0])  # stable: (w, j) order among equal keys
            keys = sorted({c[0] for c in cands} | {k for k, _, _ in pool})
            for a, c in zip(keys, keys[1:]):
                gap = min(gap, (c - a) / max(abs(c), 1e-30))
            parents, tokens = list(range(W)), [0] * W
            n_alive, n_cum, n_len = [False] * W, [float("inf")] * W, [0] * W
            for place, i in enumerate(order[:W]):
                key, w, j, cost = cands[i]
                tok = int(cand_id[t][b * W + w][j])
                parents[place], tokens[place] = w, tok
                retire = tok == eos or t == T - 1
                n_alive[place], n_cum[place], n_len[place] = not retire, cost, length[w] + 1
                if retire:
                    at = 0
                    while at < len(pool) and pool[at][0] <= key:
                        at += 1
                    pool.insert(at, (key, t, place))
                    del pool[W:]
            hist_parent.append(parents)
            hist_token.append(tokens)
            alive, cum, length = n_alive, n_cum, n_len
        answers = []
        for key, step, slot in pool:
            toks = [0] * T
            for s in range(step, -1, -1):
                toks[s] = hist_token[s][slot]
                slot = hist_parent[s][slot]
            answers.append(toks)
        out.append(dict(keys=[k for k, _, _ in pool], steps=[s for _, s, _ in pool], slots=[s for _, _, s in pool], answers=answers, gaps=gap))
    return out


def planted_candidates(B, W, T, eos, seed):
    """cand_p f32 / cand_id int64 [T, B * W, W] for ``restate_beam`` and K25: descending probabilities per row with EOS among the ids now and then
    and a probability of exactly 0 in the last place of some rows (a dead candidate)."""
    rng = np.random.RandomState(seed)
    p = np.sort(rng.uniform(0.02, 0.9, size=(T, B * W, W)), axis=-1)[..., ::-1].astype(np.float32)
    ids = rng.randint(5, 60, size=(T, B * W, W)).astype(np.int64)
    ids[rng.uniform(size=ids.shape) < 0.12] = eos
    ids[0, :, 0] = 7  # (no hypothesis ends at the first step through its best candidate)
    p[rng.uniform(size=p.shape[:2]) < 0.3, W - 1] = 0.0
    return np.ascontiguousarray(p), ids


# ---------------------------------------------------------------------------------------------
# the restatements against hand-worked cases
# ---------------------------------------------------------------------------------------------
def test_restated_rules_on_a_small_row():
    row = np.arange(1, 9, dtype=np.float32) / 10
    assert restate_rules(row, 2, 3, 3, None).tolist() == [x if i != 3 else 0.0 for i, x in enumerate(row.tolist())]
    assert np.array_equal(restate_rules(row, 3, 3, 3, None), row), "t = m: EOS is free again"
    assert np.array_equal(restate_rules(row, 0, -1, 5, None), row), "no EOS id: nothing to keep out"
    got = restate_rules(row, 9, 3, 0, [7, 7, -1, 8, 100, 0])
    assert got.tolist() == [0.0] + row[1:7].tolist() + [0.0], "duplicates, -1 and ids >= V are harmless"
    assert restate_rules(row, 0, 3, 1, list(range(8))).tolist() == [0.0] * 8 and ordered_top(np.zeros(8), 1)[0] == 0, "an all-zero row gives id 0"
    rows = np.tile(row, (4, 1))
    per_item = restate_rows(rows, 0, 3, 0, [[1], [2]], rows_per_item=2)
    assert [np.flatnonzero(r == 0).tolist() for r in per_item] == [[1], [1], [2], [2]]
    assert ordered_top(np.asarray([0.5, 0.7, 0.7, 0.1]), 3).tolist() == [1, 2, 0]


def test_restated_beam_on_a_hand_worked_case():
    """W = 2, T = 2, one item.  Step 0: slot 0 offers (a: 0.5, EOS: 0.25).  alpha = 1: keys ln 2 / 2 < ln 4 / 2, so a lives in slot 0 and EOS
    retires from slot 1 with key ln 4 / 2.  Step 1 (last): slot 0 offers (b: 0.5, c: 0.5): both retire with key 2 ln 2 / 3 < ln 4 / 2."""
    eos = 2
    p = np.asarray([[[0.5, 0.25], [0.9, 0.9]], [[0.5, 0.5], [0.9, 0.9]]], dtype=np.float32)
    ids = np.asarray([[[10, eos], [11, 12]], [[20, 21], [22, 23]]], dtype=np.int64)
    (got,) = restate_beam(p, ids, 1, 2, 2, eos, 1.0)
    ln2 = math.log(2.0)
    assert got["answers"] == [[10, 20], [10, 21]] and got["steps"] == [1, 1] and got["slots"] == [0, 1]
    assert np.allclose(got["keys"], [2 * ln2 / 3, 2 * ln2 / 3], rtol=1e-9), "the EOS hypothesis (key ln 4 / 2) fell off the pool of two"
    short = p.copy()
    short[0, 0, 1] = 0.26  # alpha = 0: plain cost, and the short hypothesis (-ln 0.26 = 1.347) beats a b / a c (2 ln 2 = 1.386)
    (flat,) = restate_beam(short, ids, 1, 2, 2, eos, 0.0)
    assert flat["answers"] == [[eos, 0], [10, 20]] and np.allclose(flat["keys"], [-math.log(float(np.float32(0.26))), 2 * ln2], rtol=1e-8)
    (long_,) = restate_beam(p, ids, 1, 2, 2, eos, 2.0)  # alpha = 2: ln 4 / 4 against 2 ln 2 / 9
    assert long_["answers"][0] == [10, 20] and np.allclose(long_["keys"][0], 2 * ln2 / 9, rtol=1e-9)
    dead = p.copy()
    dead[0, 0, 1] = 0.0  # the EOS candidate has probability 0: it never enters a hypothesis
    (got,) = restate_beam(dead, ids, 1, 2, 2, eos, 1.0)
    assert all(eos not in a for a in got["answers"])


def test_planted_candidates_are_decisive_for_every_alpha():
    """The K25 test of the GPU file compares orders exactly: at every alpha every pair of different keys that is ever compared lies >= 1e-4
    apart (relative), far above f32 rounding of a sum of six logarithms and one powf."""
    B, W, T, eos = 3, 4, 6, 2
    p, ids = planted_candidates(B, W, T, eos, seed=BEAM_SEED)
    assert (p == 0).any() and (ids == eos).any()
    firsts = {}
    for alpha in (0.0, 0.6, 1.0, 2.0):
        items = restate_beam(p, ids, B, W, T, eos, alpha)
        assert min(i["gaps"] for i in items) >= 1e-4, "alpha %s: keys %.3g apart" % (alpha, min(i["gaps"] for i in items))
        assert all(len(i["keys"]) == W for i in items), "every pool fills"
        firsts[alpha] = [i["answers"][0] for i in items]
    assert firsts[0.0] != firsts[2.0], "alpha = 0 and alpha = 2 must disagree about a best hypothesis"


BEAM_SEED = 5


# ---------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vocab():
    from case_rg_amd.utils import make_vocab
    return make_vocab(120)


def _check(vocab, min_length=0, banned_ids=None, length_penalty=1.0, B=2, T=8):
    from case_rg_amd.common.TransformerSeqEncoderDecoder import decode_rules_param
    return decode_rules_param(min_length, banned_ids, length_penalty, vocab[0], B, T)


def test_checker_refuses_every_bad_argument(vocab):
    from case_rg_amd.common.Constants import EOS_WORD
    eos = vocab[0][EOS_WORD]
    for bad in (-1, 1.5, "3", True, None):
        with pytest.raises(ValueError, match="min_length"):
            _check(vocab, min_length=bad)
    with pytest.raises(ValueError, match="min_length"):
        _check(vocab, min_length=8, T=8)
    assert _check(vocab, min_length=7, T=8)["min_length"] == 7, "the last position can still hold EOS"
    with pytest.raises(ValueError, match="at most 256"):
        _check(vocab, banned_ids=list(range(100, 357)))
    assert _check(vocab, banned_ids=list(range(100, 356)))["banned"].shape == (256,)
    for shape in ((3, 4), (2, 2, 2), ()):
        with pytest.raises(ValueError, match=r"\[K\] or \[B, K\]"):
            _check(vocab, banned_ids=torch.full(shape, 9, dtype=torch.int64), B=2)
    with pytest.raises(ValueError, match="integers"):
        _check(vocab, banned_ids=[1.5, 2.0])
    for lists in ([5, eos], [[5, 6], [eos, -1]]):
        with pytest.raises(ValueError, match="EOS"):
            _check(vocab, banned_ids=lists)
    for bad in (-0.1, float("inf"), float("nan"), "x", None, True):
        with pytest.raises(ValueError, match="length_penalty"):
            _check(vocab, length_penalty=bad)


def test_checker_returns_the_device_ready_form(vocab):
    from case_rg_amd.common.Constants import EOS_WORD
    off = _check(vocab)
    assert off == dict(min_length=0, banned=None, length_penalty=1.0, eos=vocab[0][EOS_WORD], on=False)
    assert _check(vocab, banned_ids=[])["on"] is False and _check(vocab, length_penalty=0)["on"] is False
    got = _check(vocab, min_length=np.int64(3), banned_ids=[4, 4, -1, 1000], length_penalty=0.6)
    assert got["min_length"] == 3 and got["length_penalty"] == 0.6 and got["on"]
    assert got["banned"].dtype == torch.int32 and got["banned"].tolist() == [4, 4, -1, 1000] and got["banned"].is_contiguous()
    per_item = _check(vocab, banned_ids=torch.tensor([[4, 5, 6], [7, -1, -1]]), B=2)
    assert per_item["banned"].shape == (2, 3) and per_item["banned"].dtype == torch.int32
    assert _check(vocab, banned_ids=[[4, 5]], B=1)["banned"].shape == (1, 2)


def test_row_rules_of_the_ops_layer_check_their_operands():
    from case_rg_amd import ops
    r = ops.row_rules(2, 3, torch.tensor([4, 5], dtype=torch.int32), rows_per_item=4)
    assert r == ops.RowRules(2, 0, 3, r.banned, 4) and r._replace(t=5).t == 5
    assert ops.row_rules(None, 0, torch.zeros(0, dtype=torch.int32)).banned is None and ops.row_rules(None).eos == -1
    with pytest.raises(TypeError):
        ops.row_rules(2, 0, torch.tensor([4, 5]))  # int64
    with pytest.raises(ValueError, match="at most 256"):
        ops.row_rules(2, 0, torch.zeros(257, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.row_rules(2, -1)
    state = ops.BeamState(1, 2, 3, torch.device("cpu"))
    cand = torch.zeros(2, 2), torch.zeros(2, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="flat"):
        ops.beam_advance(state, *cand, 0, 2, length_penalty=0.6)
    with pytest.raises(ValueError, match="length_penalty"):
        ops.beam_advance(state, *cand, 0, 2, length_penalty=-1.0)
    assert ops.RULES_MAX_BANNED == 256


# ---------------------------------------------------------------------------------------------
# the task models: None and defaults resolve to the attributes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["case", "masque"])
def test_models_resolve_keywords_against_their_attributes(kind):
    import case_rg_amd
    from case_rg_amd.common.Constants import EOS_WORD, UNK_WORD
    from case_rg_amd.utils import make_vocab, synth_batch
    ns = case_rg_amd.namespace()
    v2i, i2v = make_vocab(120)
    T = 8
    m = (ns.CaSE(4, T, i2v, v2i, 32) if kind == "case" else ns.Masque(T, i2v, v2i, 32)).eval()
    assert (m.min_length, m.banned_ids, m.length_penalty) == (0, None, 1.0)
    batch = synth_batch(2, 3, 12, 8, 6, 120, seed=3, model=kind)
    seen = []

    def respond(data, **mode):
        seen.append(mode)
        z = torch.zeros(2, T, dtype=torch.int64)
        return (None, None, None, z, z.view(2, 1, T), torch.zeros(2, 1), torch.zeros(2, 1)), torch.zeros(2, 3)

    m._respond = respond
    unk = v2i[UNK_WORD]
    for call in (lambda **kw: m.do_test(batch, **kw), lambda **kw: m.do_beam(batch, **kw), lambda **kw: m.do_sample(batch, seed=7, **kw)):
        del seen[:]
        call()
        call(min_length=None, banned_ids=None)
        m.min_length, m.banned_ids = 3, [unk]
        call()
        call(min_length=2)
        call(min_length=0, banned_ids=[[unk, 9], [10, -1]])
        m.min_length, m.banned_ids = 0, None
        rules = [s["decode_rules"] for s in seen]
        assert rules[0] == rules[1] and not rules[0]["on"] and rules[0]["length_penalty"] == 1.0 and rules[0]["eos"] == v2i[EOS_WORD]
        assert rules[2]["min_length"] == 3 and rules[2]["banned"].tolist() == [unk], "None means the attribute"
        assert rules[3]["min_length"] == 2 and rules[3]["banned"].tolist() == [unk]
        assert rules[4]["min_length"] == 0 and rules[4]["banned"].tolist() == [[unk, 9], [10, -1]]
    del seen[:]
    m.length_penalty = 0.6
    m.do_beam(batch)
    m.do_beam(batch, length_penalty=2)
    m.do_test(batch)
    m.length_penalty = 1.0
    assert [s["decode_rules"]["length_penalty"] for s in seen[:2]] == [0.6, 2.0]
    with pytest.raises(ValueError, match="min_length"):
        m.do_test(batch, min_length=T)
    with pytest.raises(ValueError, match="EOS"):
        m.do_sample(batch, banned_ids=[v2i[EOS_WORD]])
    with pytest.raises(ValueError, match="length_penalty"):
        m.do_beam(batch, length_penalty=-1)
    # do_consensus hands the keywords to its pool
    calls = []
    m.do_sample = lambda data, **kw: calls.append(("sample", kw)) or {"samples": torch.ones(2, 2, T, dtype=torch.int64), "rank": None}
    m.do_beam = lambda data, **kw: calls.append(("beam", kw)) or {"beam_answers": torch.ones(2, 2, T, dtype=torch.int64),
                                                                    "beam_scores": torch.zeros(2, 2), "rank": None}
    for pool, kw in (("sample", dict(min_length=5)), ("beam", dict(min_length=5, banned_ids=[unk], length_penalty=0.6)), ("sample", {})):
        try:
            m.do_consensus(batch, pool=pool, **kw)
        except RuntimeError:  # (the consensus kernels need the device; the pool has been called by then)
            pass
    assert calls[0][0] == "sample" and calls[0][1]["min_length"] == 5 and "banned_ids" not in calls[0][1]
    assert calls[1][0] == "beam" and calls[1][1]["length_penalty"] == 0.6 and calls[1][1]["banned_ids"] == [unk]
    assert not {"min_length", "banned_ids", "length_penalty"} & set(calls[2][1]), "None stays out: the pool takes the attributes"
    with pytest.raises(ValueError, match="length_penalty"):
        m.do_consensus(batch, pool="sample", length_penalty=0.6)
