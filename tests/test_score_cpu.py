"""Teacher-forced scoring, CPU side: the CPU oracle's teacher-forced probabilities (tests/golden/score_cases.py ``forced_probs``, the
route of ``beam_cases.step_dists`` kept at every position) must reproduce the fixtures that the reference's own training branch produced
(tests/golden/gen_score_golden.py), at the oracle bar of tests/test_oracle_vs_golden.py: 2e-5 relative / 2e-6 absolute.  Also here: the
properties the fixtures were searched for, a NumPy restatement of ``do_score``'s reductions on hand-made numbers and on the fixtures, and
the argument check that needs no GPU."""
import types

import numpy as np
import pytest
import torch

import score_cases
from helpers import compare, load_golden


def _oracle_ns():
    import oracle
    return types.SimpleNamespace(**{k: v for k, v in vars(oracle).items() if not k.startswith("_")})


@pytest.fixture(scope="module")
def oracle_probs():
    """name -> (golden, p, ptr | None, gen) of the CPU oracle, computed once for the module."""
    ns, out = _oracle_ns(), {}
    for name, (kind, _, _, cseed) in score_cases.SCORE_CASES.items():
        golden = load_golden(name)
        m, b = score_cases.build(ns, torch.device("cpu"), name)
        for k in ("query", "passage", "source_map", "response"):
            assert np.array_equal(b[k].numpy(), golden["in_" + k]), "regenerated inputs must be the committed inputs"
        cands = score_cases.candidates(b, int(golden["eos"]), cseed)
        assert np.array_equal(cands.numpy(), golden["answers"]), "regenerated candidates must be the committed candidates"
        out[name] = (golden,) + score_cases.forced_all(ns, m, b, kind, cands)
    return out


@pytest.mark.parametrize("name", list(score_cases.SCORE_CASES))
def test_oracle_teacher_forced_probabilities_match_the_reference(name, oracle_probs):
    golden, p, ptr, gen = oracle_probs[name]
    assert tuple(golden["seeds"]) == score_cases.SCORE_CASES[name][1:]
    assert golden["answers"].shape == (score_cases.ITEMS, score_cases.N, score_cases.T)
    compare(name + "/p", p, golden["p"], 2e-5, 2e-6)
    compare(name + "/gen", gen, golden["gen"], 2e-5, 2e-6)
    assert (ptr is not None) == ("ptr" in golden) == (score_cases.SCORE_CASES[name][0] == "case")
    if ptr is not None:
        compare(name + "/ptr", ptr, golden["ptr"], 2e-5, 2e-6)


@pytest.mark.parametrize("name", list(score_cases.SCORE_CASES))
def test_fixture_pins_what_it_was_searched_for(name):
    g = load_golden(name)
    ans, p, pad = g["answers"], g["p"].astype(np.float64), int(g["pad"])
    scored = ans != pad
    assert (p[scored] >= score_cases.P_MIN).all(), "every scored target has p >= 1e-4 under the reference"
    occurs = (g["in_source_map"][:, None, None, :] == ans[..., None]).sum(-1)
    assert np.array_equal(occurs, g["occurs"])
    lower = g["ptr"].astype(np.float64) if "ptr" in g else p - g["gen"]  # p = p0 gen[y] + pointer part, p0 <= 1
    assert (scored & (lower >= 0.5 * p)).any(), "no scored target whose pointer part is at least half of p"
    assert (scored & (occurs >= 2)).any(), "no scored target that occurs twice in its source"
    absent = scored & (occurs == 0)
    assert absent.any(), "no scored target that is absent from its source"
    if "ptr" in g:
        assert (g["ptr"][absent] == 0).all() and (g["ptr"][scored & (occurs > 0)] > 0).all()
    tails = (~scored).any(axis=-1)
    assert tails.any() and not tails.all(), "the candidates need a PAD tail on some and none on others"


@pytest.mark.parametrize("name", list(score_cases.SCORE_CASES))
def test_reductions_of_the_fixture(name):
    g = load_golden(name)
    red = score_cases.reductions(g["p"], g["answers"], int(g["pad"]))
    assert red["tokens"] == int(g["tokens"]) == int((g["answers"] != 0).sum())
    assert np.allclose(red["scores"], g["scores"], rtol=1e-12) and abs(red["loss"] - float(g["loss"])) <= 1e-12
    # by hand: per candidate, then the token-weighted merge
    scored = g["answers"] != int(g["pad"])
    total = 0.0
    for i in range(scored.shape[0]):
        for n in range(scored.shape[1]):
            ps = g["p"][i, n][scored[i, n]].astype(np.float64)
            assert abs(red["scores"][i, n] - np.mean(-np.log(ps))) <= 1e-12
            total += float(np.sum(-np.log(ps + 1e-8)))
    assert abs(red["loss"] - total / red["tokens"]) <= 1e-12


def test_reductions_on_hand_made_numbers():
    p = np.array([[[0.5, 0.25, 0.9], [0.125, 0.0, 0.3]]])
    ans = np.array([[[7, 9, 0], [3, 4, 5]]])
    red = score_cases.reductions(p, ans)
    assert red["tokens"] == 5 and np.array_equal(red["token_probs"][0, 0], [0.5, 0.25, 1.0])
    assert np.isclose(red["scores"][0, 0], (np.log(2) + np.log(4)) / 2)
    assert np.isclose(red["scores"][0, 1], (np.log(8) - np.log(1e-30) - np.log(0.3)) / 3)  # p = 0 is clamped at 1e-30 in the score ...
    want = -(np.log(0.5 + 1e-8) + np.log(0.25 + 1e-8) + np.log(0.125 + 1e-8) + np.log(1e-8) + np.log(0.3 + 1e-8)) / 5
    assert np.isclose(red["loss"], want)  # ... and meets the training loss's 1e-8 epsilon in the loss
    empty = score_cases.reductions(np.ones((1, 1, 2)), np.zeros((1, 1, 2), dtype=np.int64))
    assert empty["tokens"] == 0 and empty["loss"] == 0.0 and empty["scores"][0, 0] == 0.0


def test_do_score_is_refused_in_train_mode():
    """Eval mode only, checked before anything is launched (no GPU needed to see it)."""
    import case_rg_amd
    from case_rg_amd.utils import make_vocab
    ns = case_rg_amd.namespace()
    v2i, i2v = make_vocab(200)
    for model in (ns.CaSE(4, 5, i2v, v2i, 32), ns.Masque(5, i2v, v2i, 32)):
        model.train()
        with pytest.raises(ValueError, match="eval mode"):
            model.do_score({})
        with pytest.raises(ValueError, match="eval mode"):
            model({}, method="score")
