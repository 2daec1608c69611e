"""The supporting-token stage on the MI355X: K37 (``case_token_labels``) against the host form ``common.Utils.token_label`` and the fixture of
the reference's own ``token_label``; K38 (``case_token_select``) against a stable descending ``torch.sort`` of the restated keys and exact
counts; the extract-only pass ``do_extract``, the training step without ``token_label`` / ``token_weight`` and the trainer's
``evaluate_extract`` on a tiny CaSE (P 3, L 16) in fp32 and bf16.

Labels, positions and counts are integers and compared exactly.  K37's weights are f64 results rounded once to f32, as the host form's are,
so the two may differ by one f32 rounding: 1.2e-7 relative.  Measured maxima go to the session's parity ledger (``helpers.record_error``,
case "token_label"); profiles/token_label_parity.json keeps a copy."""
import math

import numpy as np
import pytest
import torch

import cases
from helpers import Calls, load_golden, record_error

pytestmark = pytest.mark.gpu

ROUND = 1.2e-7  # one f32 rounding of an f64 result, relative
FIRST = 4


@pytest.fixture(scope="module")
def ns():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.float32)
    case_rg_amd.set_dropout(False)
    return case_rg_amd.namespace()


def relative(got, want):
    return float(((got.double() - want.double()).abs() / want.double().abs()).max())


def label_inputs(B, P, L, T, seed, words=12, f32_table=False):
    """Ragged passages and answers over ``words`` ids (members and repeated members are common), a table that leaves the last two ids out."""
    rs = np.random.RandomState(seed)
    x, y = np.zeros((B, P, L), dtype=np.int64), np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        for p in range(P):
            n = rs.randint((L + 1) // 2, L + 1)
            x[b, p, :n] = rs.randint(0, words, n) + FIRST
        n = rs.randint((T + 1) // 2, T + 1)
        y[b, :n] = rs.randint(0, words, n) + FIRST
    freq = rs.randint(0, 2 * 10 ** 6, FIRST + words - 2)
    freq[FIRST] = 0
    freq = torch.from_numpy(freq.astype(np.float32) if f32_table else freq.astype(np.int64))
    return torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), freq.cuda()


def check_labels(x, y, freq, tag):
    from case_rg_amd import ops
    from case_rg_amd.common.Utils import token_label
    with Calls() as c:
        label, weight = ops.token_labels(x, y, freq)
    assert c.calls == {"case_token_labels": 1}
    want_label, want_weight = token_label(x, y, freq)
    assert label.dtype == weight.dtype == torch.float32 and label.shape == weight.shape == x.shape
    assert torch.equal(label, want_label), "%s: labels differ at %s" % (tag, (label != want_label).nonzero()[:4].tolist())
    assert torch.equal(weight.eq(1.0) | label.bool(), torch.ones_like(label, dtype=torch.bool)), "%s: exactly 1 where the label is 0" % tag
    gap = relative(weight, want_weight)
    print("token_labels(%s): members %d, max relative distance from the host form %.3e" % (tag, int(label.sum()), gap))
    record_error("token_label", "f32", tag, gap, ROUND)
    assert gap <= ROUND, (tag, gap)
    return label, weight


# ---------------------------------------------------------------------------------------------
# 1. K37 against the host form and the fixture
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 384, 1000])
def test_token_labels_against_the_host_form(L):
    members = 0
    for T in (1, 64, 65, 80):
        for B, P in ((1, 1), (7, 3)):
            x, y, freq = label_inputs(B, P, L, T, 372 + 1000 * L + 10 * T + B, words=12 if T < 64 else 90, f32_table=T == 64)
            label, _ = check_labels(x, y, freq, "L%d_T%d_B%dxP%d" % (L, T, B, P))
            members += int(label.sum())
    assert members > 0, "the inputs prove nothing"


def test_token_labels_at_the_limits():
    """L 16384 and T 1024: the flags and the answer fill their LDS arrays."""
    from case_rg_amd import ops
    x, y, freq = label_inputs(1, 2, ops.TOKEN_MAX_L, ops.TOKEN_MAX_T, 373, words=3000)
    label, _ = check_labels(x, y, freq, "L16384_T1024")
    assert 0 < int(label.sum()) < label.numel()
    with Calls() as c:
        with pytest.raises(ValueError, match="up to 16384 tokens"):
            ops.token_labels(torch.ones(1, 1, ops.TOKEN_MAX_L + 1, dtype=torch.int64, device="cuda"), y, freq)
        with pytest.raises(ValueError, match="up to 1024 ids"):
            ops.token_labels(x, torch.ones(1, ops.TOKEN_MAX_T + 1, dtype=torch.int64, device="cuda"), freq)
        with pytest.raises(TypeError, match="freq"):
            ops.token_labels(x, y, freq.int())
    assert c.calls == {}


def test_token_labels_on_the_fixture():
    """The reference's own labels exactly, its weights within its own distance from f64 plus one rounding; the host form as everywhere."""
    golden = load_golden("token_label")
    bar = ROUND + float(golden["ref_vs_f64"])
    for i, name in enumerate(golden["names"].tolist()):
        c = {k: torch.from_numpy(np.asarray(golden["%s_%d" % (k, i)])).cuda() for k in ("passage", "response", "freq", "label", "weight")}
        label, weight = check_labels(c["passage"], c["response"], c["freq"], "fixture_" + name)
        assert torch.equal(label, c["label"]), name
        gap = relative(weight, c["weight"])
        record_error("token_label", "f32", "fixture_%s_vs_reference" % name, gap, bar)
        assert gap <= bar, (name, gap, bar)


def test_token_labels_edge_rows():
    from case_rg_amd import ops
    x, y, freq = label_inputs(3, 3, 21, 7, 374)
    x[0, 1] = 0                                   # an all-PAD row
    y[1] = 0                                      # an empty answer set
    y[2] = torch.tensor([5, 5, 9, 5, 9, 0, 5])    # duplicate answer ids, a PAD between them
    x[2, 0, :6] = torch.tensor([5, 5, 9, 9, 5, 7])
    label, weight = check_labels(x, y, freq, "edge_rows")
    assert not label[0, 1].any() and weight[0, 1].eq(1).all()
    assert not label[1].any() and weight[1].eq(1).all()
    assert label[2, 0, :6].tolist() == [1, 1, 1, 1, 1, 0]
    same = ops.token_labels(x, torch.tensor([[5, 9]]).cuda().expand(3, 2).contiguous(), freq)
    assert torch.equal(same[0][2], label[2]) and torch.equal(same[1][2], weight[2]), "duplicates and PADs in the answer change nothing"
    # ids without an entry: beyond the table, and a table of no entries at all
    empty = ops.token_labels(x, y, freq[:0])
    from case_rg_amd.common.Utils import token_label
    assert torch.equal(empty[0], label) and relative(empty[1], token_label(x, y, {})[1]) <= ROUND


def test_token_labels_is_deterministic_and_replays_from_a_captured_graph():
    from case_rg_amd import ops
    first, second = label_inputs(5, 3, 257, 65, 375, words=40), label_inputs(5, 3, 257, 65, 376, words=40)
    eager = ops.token_labels(*second)
    again = ops.token_labels(*second)
    assert torch.equal(eager[0], again[0]) and torch.equal(eager[1], again[1])
    buf = [t.clone() for t in first]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.token_labels(*buf)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), Calls() as c:
        static = ops.token_labels(*buf)
    assert c.calls == {"case_token_labels": 1}
    for dst, src in zip(buf, second):
        dst.copy_(src)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static[0], eager[0]) and torch.equal(static[1], eager[1])
    assert not torch.equal(eager[0], ops.token_labels(*first)[0]), "the two sets of rows must differ"
    del graph


# ---------------------------------------------------------------------------------------------
# 2. K38 against a stable sort
# ---------------------------------------------------------------------------------------------
SPECIALS = (-0.0, 0.0, math.inf, -math.inf, math.nan, 1.0, -1.0)


def select_rows(S, seed):
    """Six items: 0 random with planted ties (five distinct values, a third invalid), 1 all values equal, 2 the special values, 3 all
    invalid, 4 only three valid positions (K > n_valid wherever K > 3), 5 distinct values."""
    g = torch.Generator().manual_seed(seed)
    values = torch.randint(0, 5, (6, S), generator=g).float() / 4 - 0.5
    values[1] = 0.25
    values[2] = torch.tensor(SPECIALS)[torch.randint(0, len(SPECIALS), (S,), generator=g)]
    values[5] = torch.randn(S, generator=g)
    valid = torch.ones(6, S, dtype=torch.bool)
    valid[0] = torch.rand(S, generator=g) < 2 / 3
    valid[3] = False
    valid[4] = False
    valid[4, torch.randperm(S, generator=g)[:3]] = True
    scores = torch.randn(6, S, generator=g)
    labels = (torch.rand(6, S, generator=g) < 0.3).float()
    return values, valid, scores, labels


def restated_select(values, valid, K, scores=None, labels=None):
    """The order in torch on the host: NaN as -inf and -0.0 as +0.0, a STABLE descending sort (equal keys keep the lower position first),
    the invalid positions struck out, K slots."""
    key = torch.where(torch.isnan(values), torch.full_like(values, -math.inf), values) + 0.0
    order = torch.sort(key, dim=1, descending=True, stable=True).indices
    pos = torch.full((values.shape[0], K), -1, dtype=torch.int32)
    for b in range(values.shape[0]):
        kept = order[b][valid[b][order[b]]][:K]
        pos[b, :kept.numel()] = kept.int()
    if labels is None:
        return pos, None
    s = values if scores is None else scores
    positive, predicted = valid & (labels > 0.5), valid & (s > 0)
    hits = torch.stack([(labels[b][pos[b][pos[b] >= 0].long()] > 0.5).sum() for b in range(values.shape[0])])
    counts = torch.stack([valid.sum(1), positive.sum(1), predicted.sum(1), (positive & predicted).sum(1), hits], 1).int()
    return pos, counts


def check_select(values, valid, K, scores, labels, tag):
    from case_rg_amd import ops
    dev = lambda t: None if t is None else t.cuda()  # noqa: E731
    with Calls() as c:
        got = ops.token_select(dev(values), dev(valid), K, scores=dev(scores), labels=dev(labels))
    assert c.calls == {"case_token_select": 1}
    want_pos, want_counts = restated_select(values, valid, K, scores, labels)
    pos = got["pos"].cpu()
    assert pos.dtype == torch.int32 and pos.shape == (values.shape[0], K)
    assert torch.equal(pos, want_pos), "%s: first difference at %s" % (tag, (pos != want_pos).nonzero()[:1].tolist())
    want_value = torch.where(pos >= 0, values.gather(1, pos.clamp(min=0).long()), torch.zeros(()))
    assert torch.equal(got["value"].cpu().view(torch.int32), want_value.view(torch.int32)), "%s: value is values at pos, 0 behind" % tag
    if labels is None:
        assert set(got) == {"pos", "value"}
    else:
        assert got["counts"].dtype == torch.int32 and torch.equal(got["counts"].cpu(), want_counts), (tag, got["counts"].tolist(), want_counts.tolist())
    return got


@pytest.mark.parametrize("K", [1, 32, 256])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 256, 257, 3840, 16384])
def test_token_select_against_a_stable_sort(S, K):
    values, valid, scores, labels = select_rows(S, 377 + 3 * S + K)
    got = check_select(values, valid, K, scores, labels, "S%d_K%d" % (S, K))
    pos = got["pos"].cpu()
    assert pos[3].eq(-1).all() and got["value"][3].eq(0).all() and got["counts"][3].eq(0).all(), "an all-invalid row selects nothing"
    assert int(pos[4].ge(0).sum()) == min(K, 3, S) and pos[4, min(K, 3, S):].eq(-1).all()
    assert pos[1, :min(K, S)].tolist() == list(range(min(K, S))), "equal values: the lower position first"
    if S >= 63:
        assert int(got["counts"][0, 4]) > 0 or K == 1, "the inputs prove nothing"
    # without labels: the same positions, no counts; the scores default to the values
    check_select(values, valid, K, None, None, "S%d_K%d_plain" % (S, K))
    check_select(values, valid, K, None, labels, "S%d_K%d_own_scores" % (S, K))


def test_token_select_orders_the_special_values():
    values = torch.tensor([[math.nan, -0.0, math.inf, 0.0, -math.inf, -1.0, 1.0, math.nan]])
    got = check_select(values, torch.ones(1, 8, dtype=torch.bool), 8, None, None, "specials")
    assert got["pos"].tolist() == [[2, 6, 1, 3, 5, 0, 4, 7]], "inf, 1, the zeros by position, -1, then NaN and -inf by position"


def test_token_select_limits_raise_before_any_launch():
    from case_rg_amd import _abi, ops
    v = torch.zeros(2, 16385, device="cuda")
    ok = torch.ones(2, 16385, dtype=torch.bool, device="cuda")
    with Calls() as c:
        with pytest.raises(ValueError, match="up to 16384 keys"):
            ops.token_select(v, ok, 4)
        with pytest.raises(ValueError, match="256 selected"):
            ops.token_select(v[:, :100].contiguous(), ok[:, :100].contiguous(), 257)
        with pytest.raises(ValueError, match="k = 1"):
            ops.token_select(v[:, :100].contiguous(), ok[:, :100].contiguous(), 0)
        with pytest.raises(TypeError, match="labels"):
            ops.token_select(v[:, :100].contiguous(), ok[:, :100].contiguous(), 4, scores=v[:, :100].contiguous())
    assert c.calls == {}
    pos, val = torch.zeros(1, 4, dtype=torch.int32, device="cuda"), torch.zeros(1, 4, device="cuda")
    with pytest.raises(Exception, match="case_token_select"):
        _abi.call("case_token_select", v.data_ptr(), None, None, None, pos.data_ptr(), val.data_ptr(), None, 1, 16385, 4,
                  torch.cuda.current_stream().cuda_stream)


def test_token_select_is_deterministic_and_replays_from_a_captured_graph():
    from case_rg_amd import ops
    first, second = [t.cuda() for t in select_rows(3840, 378)], [t.cuda() for t in select_rows(3840, 379)]
    call = lambda t: ops.token_select(t[0], t[1], 32, scores=t[2], labels=t[3])  # noqa: E731
    eager, again = call(second), call(second)
    for k in eager:
        assert torch.equal(eager[k].view(torch.int32), again[k].view(torch.int32)), k
    buf = [t.clone() for t in first]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(buf)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), Calls() as c:
        static = call(buf)
    assert c.calls == {"case_token_select": 1}
    for dst, src in zip(buf, second):
        dst.copy_(src)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(static[k].view(torch.int32), eager[k].view(torch.int32)), "the replay differs from the eager call in %s" % k
    assert not torch.equal(eager["pos"], call(first)["pos"]), "the two sets of rows must differ"
    del graph


def test_token_metrics_ids_names_the_columns():
    from case_rg_amd import ops
    from case_rg_amd.evaluation import eval_token_ids, token_metrics_ids
    values, valid, scores, labels = (t.cuda().reshape(6, 3, 21) for t in select_rows(63, 380))
    got = token_metrics_ids(scores, labels, valid, top_k=8, select=values)
    want_pos, want = restated_select(values.cpu().reshape(6, -1), valid.cpu().reshape(6, -1), 8, scores.cpu().reshape(6, -1), labels.cpu().reshape(6, -1))
    assert set(got) == set(ops.TOKEN_COUNTS) | {"support_pos"} and torch.equal(got["support_pos"].cpu(), want_pos)
    for i, name in enumerate(ops.TOKEN_COUNTS):
        assert got[name].dtype == torch.int64 and torch.equal(got[name].cpu(), want[:, i].long()), name
    total = eval_token_ids(scores, labels, valid, top_k=8, select=values)
    assert total.is_cuda and total.dtype == torch.int64 and torch.equal(total.cpu(), want.long().sum(0))
    own = token_metrics_ids(scores, labels, valid, top_k=8)
    assert torch.equal(own["support_pos"].cpu(), restated_select(scores.cpu().reshape(6, -1), valid.cpu().reshape(6, -1), 8)[0])


# ---------------------------------------------------------------------------------------------
# 3. the model: do_extract, the training step without the two keys, evaluate_extract
# ---------------------------------------------------------------------------------------------
ITEMS, P, L = 4, 3, 16


@pytest.fixture(params=["fp32", "bf16"])
def tiny(request, ns):
    """A tiny CaSE at P 3, L 16 with a frequency table installed, in eval mode, and its batch on the device."""
    import case_rg_amd
    from case_rg_amd.utils import synth_batch
    case_rg_amd.set_compute_dtype(torch.bfloat16 if request.param == "bf16" else torch.float32)
    try:
        m = cases._case_model(ns, torch.device("cuda"), 381, gain=3.0).eval()
        b = {k: v.cuda() for k, v in synth_batch(ITEMS, P, L, 8, 6, cases.V, seed=382, model="case").items()}
        freq = torch.from_numpy(np.random.RandomState(383).randint(0, 10 ** 5, cases.V))
        m.set_token_freq(freq)
        yield m, b, request.param
    finally:
        case_rg_amd.set_compute_dtype(torch.float32)


def _decoder_calls(c):
    return sum(n for name, n in c.calls.items() if name.startswith("case_pointer"))


def test_do_extract_is_the_middle_of_do_test(tiny):
    m, b, mode = tiny
    seen = {}
    hook = m.response_generation.decoder.register_forward_pre_hook(
        lambda mod, args, kwargs: seen.update(prior=kwargs["encode_weights"][1].clone()), with_kwargs=True)
    try:
        with torch.no_grad():
            with Calls() as full:
                test = m.do_test(dict(b))
    finally:
        hook.remove()
    with torch.no_grad():
        rank = m.do_rank(dict(b))["rank"]
        with Calls() as c:
            out = m.do_extract(dict(b))
        routed = m(dict(b), method="extract")
        by_score = m.do_extract(dict(b), top_k=5, select="score")
    K = m.support_top_k
    assert K == 32 and set(out) == {"rank", "token_score", "token_prior", "support_pos", "support_ids", "support_value"}
    assert _decoder_calls(full) > 0 and _decoder_calls(c) == 0 and c.count("case_token_select") == 1
    assert torch.equal(out["rank"], rank) and torch.equal(out["rank"], test["rank"])
    assert out["token_prior"].dtype == torch.float32 and out["token_prior"].shape == (ITEMS, P, L)
    assert torch.equal(out["token_prior"], seen["prior"]), "the prior the decoder receives in do_test (%s)" % mode
    valid = b["passage"].ne(0)
    assert out["token_score"].dtype == torch.float32 and out["token_score"][~valid].eq(-1e6).all() and out["token_score"][valid].abs().max() < 1e6
    for key in out:
        assert torch.equal(out[key], routed[key]), key
    flat = lambda t: t.reshape(ITEMS, -1).cpu()  # noqa: E731
    for got, key, k in ((out, out["token_prior"], K), (by_score, out["token_score"], 5)):
        pos = got["support_pos"].cpu()
        assert pos.dtype == torch.int32 and torch.equal(pos, restated_select(flat(key), flat(valid), k)[0])
        picked = pos >= 0
        assert torch.equal(picked.sum(1), flat(valid).sum(1).clamp(max=k))
        want_ids = torch.where(picked, flat(b["passage"]).gather(1, pos.clamp(min=0).long()), torch.zeros((), dtype=torch.int64))
        assert got["support_ids"].dtype == torch.int64 and torch.equal(got["support_ids"].cpu(), want_ids) and want_ids[picked].ne(0).all()
        assert torch.equal(got["support_value"].cpu(), torch.where(picked, flat(key).gather(1, pos.clamp(min=0).long()), torch.zeros(())))
    assert by_score["support_pos"].shape == (ITEMS, 5)


def test_do_train_without_the_two_keys_is_do_train_on_label_batch(tiny):
    from case_rg_amd.common.Utils import token_label
    m, b, mode = tiny
    bare = {k: v for k, v in b.items() if k not in ("token_label", "token_weight")}
    m.train()
    try:
        with torch.no_grad():
            m(dict(b), method="train")  # (the first pass of a model also fills the cache of bf16 operands: not counted)
            with Calls() as c:
                absent = m(dict(bare), method="train")
            labelled = m.label_batch(bare)
            with Calls() as given:
                present = m(dict(labelled), method="train")
            host = dict(bare)
            host["token_label"], host["token_weight"] = token_label(bare["passage"], bare["response"], m.token_freq)
            on_host = m(host, method="train")
    finally:
        m.eval()
    assert c.count("case_token_labels") == 1 and given.count("case_token_labels") == 0
    assert {k: v for k, v in c.calls.items() if k != "case_token_labels"} == given.calls, "one launch more, nothing else"
    assert set(labelled) == set(bare) | {"token_label", "token_weight"} and "token_label" not in bare
    assert torch.equal(labelled["token_label"], host["token_label"]) and labelled["token_label"].sum() > 0
    for a, p, h in zip(absent, present, on_host):
        assert torch.equal(a, p), (mode, a, p)
        gap = abs(float(a) - float(h)) / abs(float(h))
        record_error("token_label", mode, "do_train_vs_host_labels", gap, 1e-6)
        assert gap <= 1e-6, (mode, float(a), float(h))
    with torch.no_grad():
        assert not torch.equal(absent[1], m.train()(dict(b), method="train")[1]), "the synthetic labels of the batch give another loss"
    m.eval()
    # another answer than the batch's: its non-PAD ids are the answer set
    other = b["passage"][:, 0, 1:4].contiguous()
    relabelled = m.label_batch(bare, response=other)
    assert torch.equal(relabelled["token_label"], token_label(bare["passage"], other, m.token_freq)[0])
    assert relabelled["token_label"][:, 0, 1:4][other.ne(0)].eq(1).all()


def test_a_captured_training_step_labels_its_batch(ns):
    """``CumulativeTrainer(capture=True)`` on batches without the two keys: K37 is part of the recorded step.  Two trainers from the same
    weights on the same four batches, as tests/test_step_graph_gpu.py runs them: one eager throughout, one that records its third step and
    replays it.  Both launch the same kernels on the same numbers; the weight gradients are sums of f32 atomics whose order is free (1e-7
    relative per step), so after four steps of lr 1e-3 the losses are held to 1e-4 relative."""
    from case_rg_amd.optim import FusedAdam
    from case_rg_amd.utils import synth_batch
    freq = torch.from_numpy(np.random.RandomState(383).randint(0, 10 ** 5, cases.V))
    batches = []
    for step in range(4):
        b = synth_batch(2, P, L, 8, 6, cases.V, seed=390 + step, ragged=False, model="case")
        batches.append({k: v.cuda() for k, v in b.items() if k not in ("token_label", "token_weight")})
    losses, replays = {}, {}
    for captured in (False, True):
        model = cases._case_model(ns, torch.device("cuda"), 381).train()
        model.set_token_freq(freq)
        trainer = ns.CumulativeTrainer(model, None, None, 0, 1, capture=True)
        if not captured:
            trainer.graphs = None  # device-state mode without captures: the eager yardstick
        opt = FusedAdam(model.parameters(), lr=1e-3)
        with Calls() as c:
            losses[captured] = [trainer.train_batch(0, dict(b), "train", opt) for b in batches]
        torch.cuda.synchronize()
        replays[captured] = 0 if trainer.graphs is None else trainer.graphs.replays
        assert c.count("case_token_labels") in ((3, 4) if captured else (4,)), "a replay makes no call of its own: %s" % c.calls
        trainer.close()
    assert replays == {False: 0, True: 2}, replays  # (two eager steps, then the third is recorded and replayed)
    print("captured step without the two keys: eager %s, replayed %s" % (losses[False], losses[True]))
    assert np.allclose(losses[False], losses[True], rtol=1e-4, atol=0), (losses[False], losses[True])
    assert len({tuple(l) for l in losses[True]}) == 4, "the batches differ"


def test_trainer_evaluate_extract_is_predict_plus_torch(tiny, ns):
    m, b, mode = tiny
    data = {k: v.cpu() for k, v in b.items()}
    m.support_top_k = 6
    trainer = ns.CumulativeTrainer(m, None, None, None, 1)
    ds = cases._ListDataset(data)
    try:
        for labels in ("token_label", "computed"):
            if labels == "computed":  # the data carries no labels: K37 makes them from the response
                from case_rg_amd.common.Utils import token_label
                ds = cases._ListDataset({k: v for k, v in data.items() if k not in ("token_label", "token_weight")})
                gold_all = token_label(data["passage"], data["response"], m.token_freq.cpu())[0]
            else:
                gold_all = data["token_label"]
            trainer.model.train()
            got = trainer.evaluate_extract(ds, cases._collate, 3, labels="token_label")
            assert trainer.model.training, "the mode must be restored"
            n_valid = n_pos = n_pred = tp = hits = slots = 0
            for batch, out in trainer.predict("extract", ds, cases._collate, 3):
                ids = batch["id"].cpu()
                valid, gold = batch["passage"].ne(0).cpu().reshape(len(ids), -1), gold_all[ids].reshape(len(ids), -1) > 0.5
                predicted = out["token_score"].cpu().reshape(len(ids), -1) > 0
                pos = out["support_pos"].cpu()
                assert pos.shape[1] == 6
                n_valid += int(valid.sum())
                n_pos += int((valid & gold).sum())
                n_pred += int((valid & predicted).sum())
                tp += int((valid & gold & predicted).sum())
                hits += sum(int(gold[i][pos[i][pos[i] >= 0].long()].sum()) for i in range(len(ids)))
                slots += int(valid.sum(1).clamp(max=6).sum())
            ratio = lambda x, y: x / y if y else 0.0  # noqa: E731
            pr, rc = ratio(tp, n_pred), ratio(tp, n_pos)
            want = dict(precision=pr, recall=rc, f1=ratio(2 * pr * rc, pr + rc), precision_at_k=ratio(hits, slots), recall_at_k=ratio(hits, n_pos),
                        items=ITEMS, tokens=n_valid)
            print("evaluate_extract(%s, %s): %s" % (mode, labels, got))
            assert got == want, (got, want)
            assert n_pos > 0 and n_valid > slots > 0
        by_score = trainer.evaluate_extract(ds, cases._collate, 3, top_k=4, select="score")
        assert by_score["precision"] == got["precision"] and by_score["tokens"] == got["tokens"]
    finally:
        m.support_top_k = 32
        m.eval()
        trainer.close()
