"""Answer attribution, host side (no kernel runs): ``evaluation.attribution.copy_attribution_host`` against a hand-worked example and
against an independent per-position loop in f64, its conventions (PAD, out-of-vocabulary and absent targets, the tie rule, the all-zero
run), ``source_segments``, ``summarize`` on worked numbers, and the ``ValueError``s that are raised before anything is launched."""
import numpy as np
import pytest
import torch

from case_rg_amd.evaluation.attribution import attribution_ids, copy_attribution_host, eval_attribution_ids, source_segments, summarize


def loop_attribution(mix, src, copies, targets, seg, pad=0, V=None):
    """The definition, position by position, in Python floats (f64): -> mass [R][G], pos [R], pos_mass [R], count [R]."""
    mix, src, targets = np.asarray(mix, dtype=np.float64), np.asarray(src), np.asarray(targets)
    copies = [np.asarray(c, dtype=np.float64) for c in copies]
    R, G, per = mix.shape[0], len(seg) - 1, mix.shape[0] // src.shape[0]
    mass, pos, pos_mass, count = [[0.0] * G for _ in range(R)], [-1] * R, [0.0] * R, [0] * R
    for r in range(R):
        y = int(targets[r])
        if (pad >= 0 and y == pad) or y < 0 or (V is not None and y >= V):
            continue
        e = np.exp(mix[r] - mix[r].max())
        pm = e / e.sum()
        best = None
        s = 0
        for k, c in enumerate(copies):
            for j in range(c.shape[1]):
                if int(src[r // per, s]) == y:
                    term = float(pm[1 + k] * c[r, j])
                    g = max(i for i in range(G) if seg[i] <= s)
                    mass[r][g] += term
                    count[r] += 1
                    if best is None or term > best:
                        best, pos[r] = term, s
                s += 1
        pos_mass[r] = 0.0 if best is None else best
    return mass, pos, pos_mass, count


def test_hand_worked_example():
    """2 memories (lengths 3 and 4), S = 7, G = 3 with boundaries [0, 2, 5, 7]: the second boundary splits memory 1 (positions 3 .. 6).
    Row 0 has equal mixing logits, pm = (1/3, 1/3, 1/3); row 1 has logits (0, ln 2, 0), pm = (1/4, 1/2, 1/4)."""
    src = torch.tensor([[7, 5, 7, 7, 9, 7, 5]])
    mix = torch.tensor([[0.0, 0.0, 0.0], [0.0, float(np.log(2.0)), 0.0]], dtype=torch.float64)
    c0 = torch.tensor([[0.5, 0.25, 0.25], [0.125, 0.5, 0.375]], dtype=torch.float64)
    c1 = torch.tensor([[0.25, 0.125, 0.5, 0.125], [0.5, 0.25, 0.125, 0.125]], dtype=torch.float64)
    out = copy_attribution_host(mix, src, [c0, c1], torch.tensor([7, 5]), [0, 2, 5, 7])
    # row 0, y = 7 at positions 0, 2, 3, 5: terms 1/3 x (0.5, 0.25, 0.25, 0.5); segments 0 | 1, 1 | 2
    third = 1.0 / 3.0
    assert out["mass"].dtype == torch.float32 and out["pos"].dtype == out["count"].dtype == torch.int32
    want0 = [third * 0.5, third * 0.25 + third * 0.25, third * 0.5]
    assert np.allclose(out["mass"][0].double().numpy(), want0, rtol=1.2e-7, atol=0)
    assert int(out["pos"][0]) == 0 and int(out["count"][0]) == 4  # 0.5 at positions 0 and 5: the lower one
    assert abs(float(out["pos_mass"][0]) - third * 0.5) <= 1.2e-7 * third
    # row 1, y = 5 at positions 1 (memory 0: 1/2 x 0.5) and 6 (memory 1: 1/4 x 0.125)
    assert np.allclose(out["mass"][1].double().numpy(), [0.25, 0.0, 0.03125], rtol=1.2e-7, atol=0)
    assert float(out["mass"][1, 1]) == 0.0
    assert int(out["pos"][1]) == 1 and int(out["count"][1]) == 2 and abs(float(out["pos_mass"][1]) - 0.25) <= 3e-8


@pytest.mark.parametrize("seed", range(6))
def test_random_cases_match_the_loop(seed):
    rng = np.random.RandomState(1000 + seed)
    nmem = 1 + seed % 4
    lens = [int(rng.randint(1, 9)) for _ in range(nmem)]
    S, items, per, V = sum(lens), 1 + seed % 3, 1 + seed % 2, 12
    R = items * per
    G = int(rng.randint(1, min(S, 6) + 1))
    seg = [0] + sorted(rng.choice(np.arange(1, S), size=G - 1, replace=False).tolist()) + [S] if S > 1 else [0, 1]
    src = rng.randint(-1, V + 2, size=(items, S))  # ids outside [0, V) among them
    mix = rng.randn(R, 1 + nmem)
    copies = [rng.rand(R, n) for n in lens]
    targets = rng.randint(0, V, size=R)
    targets[0] = int(src[0, 0]) if 0 < src[0, 0] < V else targets[0]
    out = copy_attribution_host(torch.from_numpy(mix), torch.from_numpy(src), [torch.from_numpy(c) for c in copies],
                                torch.from_numpy(targets), seg, pad=0, V=V)
    mass, pos, pos_mass, count = loop_attribution(mix, src, copies, targets, seg, pad=0, V=V)
    assert out["count"].tolist() == count and out["pos"].tolist() == pos
    want = np.asarray(mass)
    got = out["mass"].double().numpy()
    assert got.shape == (R, len(seg) - 1)
    assert np.array_equal(got == 0.0, want == 0.0), "exactly 0 where the loop's sum is empty"
    assert np.allclose(got, want, rtol=1.2e-7, atol=0) and np.allclose(out["pos_mass"].double().numpy(), pos_mass, rtol=1.2e-7, atol=0)


def test_conventions_for_pad_out_of_vocabulary_and_absent_targets():
    src = torch.tensor([[0, 4, 4, 11, -3, 4]])
    mix = torch.zeros(6, 2, dtype=torch.float64)
    c = torch.full((6, 6), 0.125, dtype=torch.float64)
    targets = torch.tensor([0, 10, -1, 9, 4, 11])  # PAD (it occurs in the source), V, negative, absent, present, >= V but in the source
    out = copy_attribution_host(mix, src, [c], targets, [0, 3, 6], pad=0, V=10)
    for r in (0, 1, 2, 3, 5):
        assert out["mass"][r].tolist() == [0.0, 0.0] and int(out["pos"][r]) == -1 and float(out["pos_mass"][r]) == 0.0 and int(out["count"][r]) == 0
    assert out["mass"][4].tolist() == [0.125, 0.0625] and int(out["pos"][4]) == 1 and int(out["count"][4]) == 3
    # pad = -1: PAD's id is an id like any other; V = None: no upper bound
    free = copy_attribution_host(mix, src, [c], targets, [0, 3, 6], pad=-1, V=None)
    assert int(free["count"][0]) == 1 and int(free["pos"][0]) == 0 and int(free["count"][5]) == 1 and int(free["pos"][5]) == 3
    assert int(free["count"][2]) == 0 and int(free["pos"][2]) == -1  # a negative id is never a token


def test_tie_rule_and_the_all_zero_run():
    src = torch.tensor([[3, 8, 3, 3, 8, 3]])
    mix = torch.zeros(2, 3, dtype=torch.float64)
    c0 = torch.tensor([[0.25, 0.0, 0.5], [0.0, 0.0, 0.0]], dtype=torch.float64)
    c1 = torch.tensor([[0.5, 0.0, 0.5], [0.0, 0.0, 0.0]], dtype=torch.float64)
    out = copy_attribution_host(mix, src, [c0, c1], torch.tensor([3, 8]), [0, 6])
    assert int(out["pos"][0]) == 2, "0.5 at positions 2, 3 and 5: the lowest one"
    assert int(out["count"][0]) == 4 and abs(float(out["pos_mass"][0]) - 0.5 / 3) < 1e-7
    assert int(out["pos"][1]) == 1 and int(out["count"][1]) == 2, "an all-zero run: its lowest position"
    assert float(out["pos_mass"][1]) == 0.0 and out["mass"][1].tolist() == [0.0]


def test_source_segments():
    assert source_segments(4, 3, 5) == [0, 4, 9, 14, 19]
    assert source_segments(64, 10, 384) == [0] + [64 + 384 * p for p in range(11)] and source_segments(64, 10, 384)[-1] == 3904
    assert source_segments(7, 0, 0) == [0, 7]
    with pytest.raises(ValueError):
        source_segments(0, 2, 3)
    with pytest.raises(ValueError):
        source_segments(4, 2, 0)


def test_summarize_on_a_worked_example():
    # one item, three answers of T = 3 over G = 3 segments (the context and P = 2 passages)
    p = torch.tensor([[[0.5, 0.25, 1.0], [0.5, 0.5, 0.0], [1.0, 1.0, 1.0]]])
    scored = torch.tensor([[[True, True, False], [True, True, True], [False, False, False]]])
    mass = torch.zeros(1, 3, 3, 3)
    mass[0, 0, 0] = torch.tensor([0.125, 0.25, 0.0])    # shares: gen 1/4, context 1/4, passage 0 1/2
    mass[0, 0, 1] = torch.tensor([0.0, 0.0, 0.125])     # gen 1/2, passage 1 1/2
    mass[0, 0, 2] = torch.tensor([0.5, 0.5, 0.5])       # PAD: all 0 whatever the masses are
    mass[0, 1, 0] = torch.tensor([0.0, 0.125, 0.125])   # gen 1/2, both passages 1/4
    mass[0, 1, 1] = torch.tensor([0.25, 0.0, 0.0])      # gen 1/2, context 1/2
    out = summarize(p, mass, scored)                    # [0, 1, 2]: p = 0 and no mass: the generator's
    share, support, cited = out["share"], out["support"], out["cited"]
    assert tuple(share.shape) == (1, 3, 3, 4) and tuple(support.shape) == (1, 3, 4) and cited.dtype == torch.int64
    assert share[0, 0, 0].tolist() == [0.25, 0.25, 0.5, 0.0] and share[0, 0, 1].tolist() == [0.5, 0.0, 0.0, 0.5]
    assert share[0, 0, 2].tolist() == [0.0] * 4 and share[0, 1, 2].tolist() == [1.0, 0.0, 0.0, 0.0]
    live = scored & p.gt(0)
    assert torch.allclose(share.sum(-1)[live], torch.ones(int(live.sum())), atol=1e-6, rtol=0)
    assert support[0, 0].tolist() == [0.375, 0.125, 0.25, 0.25]
    assert cited.tolist() == [[0, 0, -1]], "equal support: the lowest index; an empty answer: -1"
    assert support[0, 2].tolist() == [0.0] * 4
    # no passage has support: -1 although the answer is not empty; more mass than p: the generator's share is clamped at 0
    none = summarize(torch.tensor([[0.5, 0.25]]), torch.tensor([[[0.25, 0.0, 0.0], [0.5, 0.0, 0.0]]]), torch.ones(1, 2, dtype=torch.bool))
    assert none["cited"].tolist() == [-1] and none["share"][0, 1].tolist() == [0.0, 2.0, 0.0, 0.0]
    second = summarize(torch.tensor([[0.5]]), torch.tensor([[[0.0, 0.0625, 0.125]]]), torch.ones(1, 1, dtype=torch.bool))
    assert second["cited"].tolist() == [1]
    with pytest.raises(ValueError):
        summarize(p, mass[..., 0], scored)


def test_attribution_columns_on_worked_numbers():
    share = torch.zeros(2, 1, 2, 4)
    share[0, 0] = torch.tensor([[0.5, 0.25, 0.25, 0.0], [0.25, 0.0, 0.5, 0.25]])
    share[1, 0, 0] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    out = dict(cited=torch.tensor([[0], [-1]]), rank=torch.tensor([[2.0, 2.0], [0.5, 1.5]]), share=share,
               answers=torch.tensor([[[5, 6]], [[7, 0]]]))
    cols = attribution_ids(out, torch.tensor([0, 1]))
    assert cols["cited_hit"].tolist() == [1, 0] and cols["rank_agree"].tolist() == [1, 0], "equal ranks: the lowest index; -1 agrees with nothing"
    assert cols["gen_share"].tolist() == [0.75, 1.0] and cols["context_share"].tolist() == [0.25, 0.0]
    assert cols["passage_share"].tolist() == [1.0, 0.0] and cols["tokens"].tolist() == [2, 1]
    assert eval_attribution_ids(out, torch.tensor([0, 1])).tolist() == [1.0, 1.0, 1.75, 0.25, 1.0, 3.0]


def test_bad_segments_are_refused():
    mix, src, c, y = torch.zeros(1, 2), torch.tensor([[1, 2, 3, 4]]), torch.ones(1, 4), torch.tensor([2])
    for seg in ([0, 2, 2, 4], [0, 3, 2, 4], [1, 4], [0, 3], [0], [0, 2, 5]):
        with pytest.raises(ValueError):
            copy_attribution_host(mix, src, [c], y, seg)
    wide_src, wide_c = torch.arange(70).reshape(1, 70), torch.ones(1, 70)
    with pytest.raises(ValueError, match="64 segments"):
        copy_attribution_host(mix, wide_src, [wide_c], y, list(range(66)))
    assert tuple(copy_attribution_host(mix, wide_src, [wide_c], y, list(range(64)) + [70])["mass"].shape) == (1, 64), "64 segments are taken"
    assert tuple(copy_attribution_host(mix, wide_src, [wide_c], y, list(range(66)) + [70], max_segments=None)["mass"].shape) == (1, 66)
    with pytest.raises(ValueError, match="64 segments"):
        copy_attribution_host(mix, wide_src, [wide_c], y, torch.zeros(66, dtype=torch.int32))
    with pytest.raises(TypeError):
        copy_attribution_host(mix, wide_src, [wide_c], y, torch.zeros(5))
    from case_rg_amd import ops
    for seg in ([0, 2, 2, 4], [1, 4], [0, 3], list(range(66))):
        with pytest.raises(ValueError):
            ops.check_segments(seg, 4 if len(seg) < 10 else 65)
    assert ops.check_segments((0, 1, 4), 4) == [0, 1, 4]


def test_do_attribute_is_refused_in_train_mode_and_for_unknown_answers():
    """Checked before anything is launched (no GPU needed to see it)."""
    import case_rg_amd
    from case_rg_amd.utils import make_vocab
    ns = case_rg_amd.namespace()
    v2i, i2v = make_vocab(200)
    for model in (ns.CaSE(4, 5, i2v, v2i, 32), ns.Masque(5, i2v, v2i, 32)):
        model.train()
        with pytest.raises(ValueError, match="eval mode"):
            model.do_attribute({})
        with pytest.raises(ValueError, match="eval mode"):
            model({}, method="attribute")
        model.eval()
        for bad in ("greedy", None, 3, torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64)):
            with pytest.raises(ValueError, match="answers"):
                model.do_attribute({}, answers=bad)
        with pytest.raises(TypeError, match="decoding arguments"):
            model.do_attribute({}, answers="response", width=2)
