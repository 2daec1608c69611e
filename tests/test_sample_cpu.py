"""Sampled decoding, CPU side: the float64 restatement of the draw rule and of the reference's ``sample`` loop conventions
(tests/golden/sample_cases.py), driven by the CPU oracle's step distributions, must reproduce the fixtures that the reference's own
``Generations.sample`` produced through the same rule (tests/golden/gen_sample_golden.py).  That pins the restatement, which
tests/test_sample_gpu.py then holds the kernel to.  Also here: the rule and the loop on hand-made rows, a statistical screen of the
24-bit counter uniform, and the argument checks of ``do_sample``.

Ids are exact on every item up to its first non-decisive step (a margin at or below sample_cases.GAP in the reference's run); the
recorded probabilities are held to the oracle bar of tests/test_oracle_vs_golden.py, 2e-5."""
import types

import numpy as np
import pytest
import torch

import sample_cases
from helpers import load_golden
from sample_cases import INF, draw, emit


def _oracle_ns():
    import oracle
    return types.SimpleNamespace(**{k: v for k, v in vars(oracle).items() if not k.startswith("_")})


def test_case_table_covers_the_four_required_settings():
    settings = {(v[0], v[4]) for v in sample_cases.SAMPLE_CASES.values()}
    assert ("case", (1.0, 0, 1.0)) in settings and ("masque", (1.0, 0, 1.0)) in settings
    assert any(p[1] == 5 for _, p in settings) and any(p == (0.7, 0, 0.9) for _, p in settings)
    assert (sample_cases.ITEMS, sample_cases.T) == (4, 6)


@pytest.mark.parametrize("name", list(sample_cases.SAMPLE_CASES))
def test_restatement_on_the_oracle_reproduces_the_reference_sample(name):
    import beam_cases
    golden = load_golden(name)
    kind, _, _, seed, params = sample_cases.SAMPLE_CASES[name]
    assert int(golden["seed"]) == seed and tuple(golden["params"]) == tuple(float(x) for x in params)
    ns = _oracle_ns()
    m, b = sample_cases.build(ns, torch.device("cpu"), name)
    for k in ("query", "passage", "source_map"):
        assert np.array_equal(b[k].numpy(), golden["in_" + k]), "regenerated inputs must be the committed inputs"
    assert m.max_target_length == sample_cases.T and len(m.vocab2id) == 200
    u = sample_cases.case_uniforms(seed)
    assert np.array_equal(u, golden["u"]), "the recorded uniforms are rng_uniform24(seed, t * ITEMS + row)"
    got = sample_cases.sample_loop(lambda rows, pre: beam_cases.step_dists(ns, m, b, kind, rows, pre), sample_cases.ITEMS, sample_cases.T,
                                   int(golden["bos"]), int(golden["eos"]), int(golden["unk"]), int(golden["pad"]), params, u)
    steps = sample_cases.decisive_steps(golden["margin"])
    assert (steps == sample_cases.T).sum() * 2 >= steps.size, "the fixture must keep at least half its items decisive through all steps"
    assert any(not np.array_equal(a, g) for a, g in zip(golden["answer"], golden["greedy"])), "no sampled answer differs from the greedy one"
    T, eos, pad = sample_cases.T, int(golden["eos"]), int(golden["pad"])
    early = [i for i in range(steps.size) if (golden["drawn"][i, :T - 1] == eos).any() and steps[i] == T]
    assert early, "no decisive row draws EOS before the last step (a PAD in the answer does not count: a live row may draw it)"
    for i in early:  # behind the drawn EOS: PAD, probability 1, nothing left to decide
        end = int(np.argmax(golden["drawn"][i] == eos))
        assert (golden["answer"][i, end + 1:] == pad).all() and (golden["prob"][i, end + 1:] == 1.0).all() and np.isinf(golden["margin"][i, end + 1:]).all()
    for i, n in enumerate(steps):
        assert np.array_equal(got["answer"][i, :n], golden["answer"][i, :n]), "%s item %d: %s != reference %s (decisive for %d steps)" % (
            name, i, got["answer"][i], golden["answer"][i], n)
        err = np.abs(got["prob"][i, :n] - golden["prob"][i, :n])
        assert (err <= 2e-5 * golden["prob"][i, :n] + 2e-6).all(), "%s item %d: probabilities %s, reference %s" % (name, i, got["prob"][i], golden["prob"][i])


def test_draw_rule_on_hand_made_rows():
    p = np.array([0.125, 0.25, 0.0, 0.25, 0.25, 0.125])  # (dyadic: every boundary is exact)
    # plain inverse CDF in id order: boundaries 0.125, 0.375, 0.375, 0.625, 0.875, 1; an entry without mass is never drawn
    assert [draw(p, 1, 0, 1, u)["id"] for u in (0.0, 0.12, 0.125, 0.37, 0.375, 0.62, 0.625, 0.9, 1 - 2.0 ** -24)] == [0, 0, 1, 1, 3, 3, 4, 5, 5]
    assert draw(p, 1, 0, 1, 0.5)["prob"] == 0.25
    # top-k: the order is q descending, the lower id first among equals -> k = 1 keeps id 1, k = 3 keeps 1, 3, 4, k = 4 adds id 0 (not 5)
    assert {draw(p, 1, 1, 1, u)["id"] for u in np.linspace(0, 0.999, 50)} == {1}
    assert draw(p, 1, 1, 1, 0.5)["margin"] == 0.0  # ids 1 and 3 tie at the cut: the id order decided, not the arithmetic
    assert {draw(p, 1, 3, 1, u)["id"] for u in np.linspace(0, 0.999, 200)} == {1, 3, 4}
    assert np.array_equal(np.nonzero(draw(p, 1, 4, 1, 0.5)["kept"])[0], [0, 1, 3, 4])
    assert draw(p, 1, 3, 1, 0.5)["Z"] == 0.75 and draw(p, 1, 99, 1, 0.5)["kept"].all()
    # top-p: the shortest prefix of the order with mass >= top_p x the kept mass; at least one entry
    assert np.array_equal(np.nonzero(draw(p, 1, 0, 0.5, 0.5)["kept"])[0], [1, 3])       # 0.25 < 0.5 <= 0.5
    assert np.array_equal(np.nonzero(draw(p, 1, 0, 0.51, 0.5)["kept"])[0], [1, 3, 4])   # 0.5 < 0.51 <= 0.75
    assert np.array_equal(np.nonzero(draw(p, 1, 0, 1e-6, 0.5)["kept"])[0], [1])
    assert np.array_equal(np.nonzero(draw(p, 1, 3, 0.6, 0.5)["kept"])[0], [1, 3])        # of the top-3 mass 0.75: 0.25 < 0.45 <= 0.5
    # temperature: q = p^(1 / tau); tau = 1 is p itself, bit for bit
    assert np.array_equal(draw(p, 1, 0, 1, 0.5)["q"], p)
    d = draw(p, 0.5, 0, 1, 0.5)
    assert np.allclose(d["q"], p ** 2) and d["q"][2] == 0 and d["prob"] == p[d["id"]]
    assert draw(p, 0.5, 0, 1, 0.3)["id"] == 1 and draw(p, 2.0, 0, 1, 0.3)["id"] == 1 and draw(p, 2.0, 0, 1, 0.12)["id"] == 0
    # the margin is the distance of u Z to the nearer boundary of the chosen token, relative to Z
    assert draw(p, 1, 0, 1, 0.5)["margin"] == 0.125 and draw(p, 1, 0, 1, 0.0625)["margin"] == 0.0625


def test_loop_conventions_on_hand_made_rows():
    EOS, UNK, PAD, T = 9, 7, 0, 4

    def run(draws):
        e, out = False, []
        for t, x in enumerate(draws):
            tok, e = emit(x, e, t, T, EOS, UNK, PAD)
            out.append(tok)
        return out

    assert run([EOS, 3, 4, 5]) == [UNK, PAD, PAD, PAD]   # EOS at t = 0: UNK is emitted and the row is ended from t = 1 (the reference's quirk)
    assert run([3, EOS, 4, 5]) == [3, EOS, PAD, PAD]     # end in the middle
    assert run([3, 4, 5, 6]) == [3, 4, 5, EOS]           # the last step forces EOS on a live row
    assert run([3, 4, EOS, 6]) == [3, 4, EOS, PAD]
    assert run([3, 4, 5, EOS]) == [3, 4, 5, EOS]

    # and through sample_loop: step distributions that put everything on one token
    def step(rows, prefixes):
        d = torch.zeros(len(rows), 12)
        t = prefixes.shape[1] - 1
        for r in rows:
            d[r, [[EOS, 3, 4, 5], [3, EOS, 4, 5], [3, 4, 5, 6]][r][t]] = 1.0
        return d

    got = sample_cases.sample_loop(step, 3, T, 1, EOS, UNK, PAD, (1.0, 0, 1.0), np.full((3, T), 0.5))
    assert got["answer"].tolist() == [[UNK, PAD, PAD, PAD], [3, EOS, PAD, PAD], [3, 4, 5, EOS]]
    assert got["prob"].tolist() == [[1.0] * 4] * 3 and np.isinf(got["margin"][0, 1:]).all() and np.isfinite(got["margin"][2]).all()


@pytest.mark.parametrize("seed", [123456, 0x9E3779B97F4A7C15])
def test_uniform24_screen(seed):
    """2^20 consecutive counters: mean, a 256-bin chi-square, and the lag correlations inside a site (consecutive rows: lag 1, 2) and
    between consecutive sites (the same row one step later: lag = rows per step, here 4, 256 and 1024).  Every bar is 5 sigma of the
    statistic's sampling noise under independence; csrc/common.h's two-round hash passes, so ``rng_uniform24`` adds no round."""
    n = 1 << 20
    u = sample_cases.rng_uniform24(seed, np.arange(n, dtype=np.uint64))
    assert u.min() >= 0.0 and u.max() < 1.0 and np.array_equal(u, u.astype(np.float32).astype(np.float64))
    assert np.array_equal(u * 2 ** 24, np.floor(u * 2 ** 24)) and len(np.unique(u)) > 0.9 * n  # 24-bit values, not 16-bit ones
    assert abs(u.mean() - 0.5) <= 5 * (1 / 12) ** 0.5 / n ** 0.5, u.mean()
    h = np.bincount((u * 256).astype(np.int64), minlength=256)
    chi = float(((h - n / 256) ** 2 / (n / 256)).sum())
    assert abs(chi - 255) <= 5 * (2 * 255) ** 0.5, chi
    for lag in (1, 2, 4, 256, 1024):
        r = float(np.corrcoef(u[:-lag], u[lag:])[0, 1])
        assert abs(r) <= 5 / n ** 0.5, (lag, r)
    # the hash itself against two values worked out by hand from csrc/common.h (seed 0: h = c C1; h ^= h >> 15; h *= C2; h ^= h >> 13)
    h = (1 * 0x9E3779B1) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x85EBCA77) & 0xFFFFFFFF
    h ^= h >> 13
    assert int(sample_cases.rng_hash(0, 1)) == h and int(sample_cases.rng_hash(0, 0)) == 0


def test_do_sample_argument_checks():
    """Bad arguments are refused before anything is launched (no GPU needed to see it)."""
    import case_rg_amd
    from case_rg_amd.utils import make_vocab
    ns = case_rg_amd.namespace()
    v2i, i2v = make_vocab(200)
    for model in (ns.CaSE(4, 5, i2v, v2i, 32), ns.Masque(5, i2v, v2i, 32)):
        assert model.sampling == dict(num_samples=1, temperature=1.0, top_k=0, top_p=1.0, seed=None)
        for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(num_samples=0)):
            with pytest.raises(ValueError, match=list(bad)[0]):
                model.do_sample({}, **bad)
        model.sampling = dict(num_samples=1, temperature=0.0, top_k=0, top_p=1.0, seed=None)
        with pytest.raises(ValueError, match="temperature"):
            model({}, method="sample")
