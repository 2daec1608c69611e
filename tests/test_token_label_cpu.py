"""The supervision of the supporting-token stage on the host: ``common.Utils.token_label`` against the fixture written from the reference's
own ``CaSEDataset.py token_label`` (tests/golden/gen_token_label_golden.py), against hand-worked rows, and the ``ValueError``s of the
training step that are raised before any launch.

Labels are 0 / 1 and compared exactly.  The reference computes its weights in f32, the host form in f64 with one rounding, so a weight may
differ from the fixture's by the reference's own distance from f64 (``ref_vs_f64``, measured when the fixture was written and capped here
at 2.4e-7: two f32 roundings; 1.12e-7 was measured on this fixture, 7.6e-8 .. 9.1e-8 on earlier draws) plus one f32 rounding of an f64
result (1.2e-7)."""
import math

import numpy as np
import pytest
import torch

from helpers import load_golden

ROUND = 1.2e-7       # one f32 rounding of an f64 result, relative
REF_CAP = 2.4e-7     # the reference's own distance from f64 may not exceed this


@pytest.fixture(scope="module")
def golden():
    return load_golden("token_label")


def golden_cases(golden):
    for i, name in enumerate(golden["names"].tolist()):
        yield name, {k: torch.from_numpy(np.asarray(golden["%s_%d" % (k, i)])) for k in ("passage", "response", "freq", "label", "weight")}


def worst_relative(got, want):
    return float(((got.double() - want.double()).abs() / want.double().abs()).max())


def test_fixture_holds_the_cases_and_the_reference_stays_inside_its_cap(golden):
    names = golden["names"].tolist()
    assert sum(n.startswith("small_") for n in names) == 8 and {"row_1", "row_2", "row_3", "row_5", "all_pad_row", "no_member", "prod"} <= set(names)
    cases = dict(golden_cases(golden))
    assert tuple(cases["small_0"]["passage"].shape) == (1, 3, 17) and cases["small_0"]["response"].shape[1] == 6
    assert tuple(cases["prod"]["passage"].shape) == (1, 10, 384) and cases["prod"]["response"].shape[1] == 80
    assert int(cases["prod"]["freq"].max()) == 2 * 10 ** 6 and cases["prod"]["freq"].numel() >= 3000
    assert cases["all_pad_row"]["passage"].eq(0).all(-1).any() and cases["no_member"]["label"].sum() == 0
    assert 0.0 < float(golden["ref_vs_f64"]) <= REF_CAP, float(golden["ref_vs_f64"])


def test_token_label_is_the_references(golden):
    from case_rg_amd.common.Utils import token_label
    bar = ROUND + float(golden["ref_vs_f64"])
    worst = 0.0
    for name, c in golden_cases(golden):
        label, weight = token_label(c["passage"], c["response"], c["freq"])
        assert label.dtype == weight.dtype == torch.float32 and label.shape == weight.shape == c["passage"].shape
        assert torch.equal(label, c["label"]), name
        assert torch.equal(weight.eq(1.0) | label.bool(), torch.ones_like(label, dtype=torch.bool)), "%s: exactly 1 where the label is 0" % name
        gap = worst_relative(weight, c["weight"])
        print("token_label(%s): max relative distance from the reference %.3e (bar %.3e)" % (name, gap, bar))
        assert gap <= bar, (name, gap, bar)
        worst = max(worst, gap)
    assert worst > 0.0, "an f64 rule that matches an f32 one in every bit proves nothing"


def test_token_label_takes_one_item_as_the_reference_does(golden):
    from case_rg_amd.common.Utils import token_label
    c = dict(golden_cases(golden))["small_3"]
    label, weight = token_label(c["passage"][0], c["response"][0], c["freq"])
    both = token_label(c["passage"], c["response"], c["freq"])
    assert label.shape == (3, 17) and torch.equal(label, both[0][0]) and torch.equal(weight, both[1][0])


def hand(x, y, f, i, g3, g5):
    """The weight of position i of row x by the rule's words."""
    lf = [math.log(f.get(v, 0) + 2) for v in x]
    return (sum(lf) / lf[i] * g3 * g5) ** 0.2


def test_hand_worked_rows():
    from case_rg_amd.common.Utils import token_label
    a, b, c, big = 5, 6, 7, 900
    f = {0: 11, a: 3, b: 0, c: 40}  # b: count 0; big: no entry and beyond the table
    # window `a a b` with both in A: two distinct members, not three
    x, y = [c, a, a, b, c], [a, b]
    label, weight = token_label(torch.tensor([x]), torch.tensor(y), f)
    assert label.tolist() == [[0, 1, 1, 1, 0]]
    want = [1.0, hand(x, y, f, 1, 1, 2), hand(x, y, f, 2, 2, 2), hand(x, y, f, 3, 2, 2), 1.0]
    #            x[0..2] = c a a: g3 1; x[-1..3]: a, b: g5 2   x[1..3] = a a b: g3 2   x[2..4] = a b c: g3 2; x[1..5]: g5 2
    assert np.allclose(weight[0].double().numpy(), want, rtol=ROUND, atol=0), (weight, want)
    # a member at position 0 and at L - 1: the windows read PAD outside the row, and PAD is no member even when the answer is padded
    x, y = [a, c, 0, c, b], [b, a, 0, 0]
    label, weight = token_label(torch.tensor([x]), torch.tensor(y), f)
    assert label.tolist() == [[1, 0, 0, 0, 1]]
    want = [hand(x, y, f, 0, 1, 1), 1.0, 1.0, 1.0, hand(x, y, f, 4, 1, 1)]
    assert np.allclose(weight[0].double().numpy(), want, rtol=ROUND, atol=0), (weight, want)
    # an id beyond the table counts as frequency 0, like an id with count 0; S includes the PAD positions
    x, y = [big, b, 0], [big, b]
    label, weight = token_label(torch.tensor([x]), torch.tensor(y), torch.tensor([11, 0, 0, 0, 0, 3, 0, 40]))
    s = 2 * math.log(2) + math.log(13)
    assert label.tolist() == [[1, 1, 0]]
    assert np.allclose(weight[0].double().numpy(), [(s / math.log(2) * 2 * 2) ** 0.2] * 2 + [1.0], rtol=ROUND, atol=0)
    # five distinct members in one window
    x = [4, 5, 6, 7, 8]
    label, weight = token_label(torch.tensor([x]), torch.tensor(x), {})
    assert label.tolist() == [[1] * 5]
    assert np.allclose(weight[0, 2].item(), (5 * 3 * 5) ** 0.2, rtol=ROUND, atol=0)


def test_dict_and_tensor_tables_agree(golden):
    from case_rg_amd.common.Utils import token_freq_table, token_label
    c = dict(golden_cases(golden))["small_5"]
    table = {v: int(n) for v, n in enumerate(c["freq"].tolist()) if n}
    assert 0 < len(table) <= c["freq"].numel()
    want = token_label(c["passage"], c["response"], c["freq"])
    for form in (table, c["freq"].float(), c["freq"].double(), token_freq_table(table), {v: float(n) for v, n in table.items()}):
        got = token_label(c["passage"], c["response"], form)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert token_freq_table(table).dtype == torch.int64 and token_freq_table({3: 0.5}).dtype == torch.float32
    assert token_freq_table({}).numel() == 0 and token_label(c["passage"], c["response"], {})[1].isfinite().all()


# ---------------------------------------------------------------------------------------------
# the training step's errors: raised before any launch, so a host model is enough
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_and_batch():
    from case_rg_amd.CaSE.Model import CaSE
    from case_rg_amd.utils import make_vocab, synth_batch
    v2i, i2v = make_vocab(400)
    return CaSE(4, 6, i2v, v2i, 32, enc_layers=1, dec_layers=1, heads=2), synth_batch(2, 3, 16, 8, 6, 400, seed=371, model="case")


def test_the_frequency_table_is_a_buffer_outside_the_state_dict(model_and_batch):
    m, _ = model_and_batch
    keys = list(m.state_dict())
    m.set_token_freq({5: 3, 9: 1})
    assert m.token_freq.dtype == torch.int64 and m.token_freq.tolist() == [0, 0, 0, 0, 0, 3, 0, 0, 0, 1]
    assert list(m.state_dict()) == keys and "token_freq" in dict(m.named_buffers())
    assert m.double().token_freq.dtype == torch.int64 and m.float() is m  # (moves with the module: an integer buffer keeps its dtype)
    m.set_token_freq(torch.tensor([1.0, 2.0]))
    assert m.token_freq.dtype == torch.float32 and list(m.state_dict()) == keys
    m.set_token_freq(None)
    assert m.token_freq is None and list(m.state_dict()) == keys


def test_do_train_without_labels_and_without_a_table_names_set_token_freq(model_and_batch):
    m, batch = model_and_batch
    m.set_token_freq(None)
    bare = {k: v for k, v in batch.items() if k not in ("token_label", "token_weight")}
    with pytest.raises(ValueError, match="set_token_freq"):
        m.train()(bare, method="train")
    with pytest.raises(ValueError, match="set_token_freq"):
        m.label_batch(bare)


@pytest.mark.parametrize("only", ["token_label", "token_weight"])
def test_do_train_with_one_of_the_two_keys_is_an_error(model_and_batch, only):
    m, batch = model_and_batch
    half = {k: v for k, v in batch.items() if k not in ("token_label", "token_weight") or k == only}
    with pytest.raises(ValueError, match="token_label.*token_weight|token_weight.*token_label"):
        m.train()(half, method="train")


def test_do_extract_argument_errors_come_before_any_launch(model_and_batch):
    m, batch = model_and_batch
    with pytest.raises(ValueError, match="eval mode"):
        m.train().do_extract(batch)
    with pytest.raises(ValueError, match="eval mode"):
        m(batch, method="extract")
    m.eval()
    with pytest.raises(ValueError, match="select"):
        m.do_extract(batch, select="label")
    for k in (0, 257):
        with pytest.raises(ValueError, match="supporting tokens"):
            m.do_extract(batch, top_k=k)
    m.train()
