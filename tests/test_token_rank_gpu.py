"""Token ranking metrics on the MI355X: K45 (``case_token_rank``) against the exact host form ``evaluation.token_rank_host``, against K38's
counts and K36's ``map``; determinism and graph capture; ``do_extract(ranking=True)`` and ``evaluate_extract(ranking=True)`` on a tiny
CaSE (P 3, L 16) in fp32 and bf16.

Every count (n_valid, n_pos, auc_num2, best_tp, best_n, n_groups) is an integer and compared exactly; ``best_threshold`` is compared in
bits; ``auc`` is one correctly rounded f64 division of exact integers and compared in bits with ``float(Fraction)``.  ``ap`` is a sum of
at most n_pos <= 16384 non-zero terms <= 1, each rounded once, added through a tree (at most 16 own terms, 6 levels in the wave, 16 waves:
<= 40 roundings of partial sums <= n_pos), and divided once: about 5e-15 relative.  It is held to the project's f64 bar, 1e-12, against the
``Fraction``.  Measured maxima go to the session's parity ledger (``helpers.record_error``, case "token_rank");
profiles/token_rank_parity.json keeps a copy."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import cases
from helpers import Calls, record_error

pytestmark = pytest.mark.gpu

AP_BAR = 1e-12
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 16384]
FAMILIES = ("tie_free", "bf16", "three_values", "all_equal", "planted_runs", "specials")
VALIDITY = ("all", "holes", "none")
LABELS = ("random", "no_positive", "all_positive", "one_first", "one_last", "half")
SPECIALS = (-0.0, 0.0, math.inf, -math.inf, math.nan, 1.0, -1.0)


@pytest.fixture(scope="module")
def ns():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.float32)
    case_rg_amd.set_dropout(False)
    return case_rg_amd.namespace()


def instance(S):
    """The padded row length, the threads and the elements per thread of the instance K45 uses for rows of S positions."""
    N = max(64, 1 << (S - 1).bit_length())
    threads = 64 if N <= 256 else (256 if N <= 2048 else 1024)
    return N, threads, N // threads


def score_row(family, S, g):
    if family == "tie_free":
        return torch.randperm(4 * S, generator=g)[:S].float() / 8 - S / 4
    if family == "bf16":
        return torch.randn(S, generator=g).bfloat16().float()
    if family == "three_values":
        return torch.tensor([-1.5, 0.25, 3.0])[torch.randint(0, 3, (S,), generator=g)]
    if family == "all_equal":
        return torch.full((S,), 0.25)
    if family == "specials":
        return torch.tensor(SPECIALS)[torch.randint(0, len(SPECIALS), (S,), generator=g)]
    # planted runs: the sorted row descends by one per rank, a few runs cover whole chunks and more, rank b takes the score of rank b - 1 at every
    # boundary between two threads' chunks (which covers every wave boundary), and the last three ranks are one group (the
    # boundary to the padding, or the end of the row where S is a power of two); the positions are then shuffled
    _, threads, per = instance(S)
    ranked = -torch.arange(S, dtype=torch.float32)
    for start in (0, 64 * per - per - 1, S // 2):
        stop = min(S, start + 3 * per + 2)
        if 0 <= start < stop:
            ranked[start:stop] = ranked[start]
    step = max(per, 2)
    for b in range(step, S, step):
        ranked[b] = ranked[b - 1]
    ranked[max(0, S - 3):] = ranked[max(0, S - 3)]
    return ranked[torch.randperm(S, generator=g)]


def valid_row(kind, S, g):
    if kind == "holes":
        return torch.rand(S, generator=g) < 0.7
    return torch.full((S,), kind == "all", dtype=torch.bool)


def label_row(kind, scores, valid, g):
    S = scores.numel()
    if kind == "random":
        return (torch.rand(S, generator=g) < 0.3).float()
    if kind == "no_positive":
        return torch.zeros(S)
    if kind == "all_positive":
        return torch.ones(S)
    if kind == "half":  # 0.5 is not positive, the next f32 is
        return torch.tensor([0.5, 0.50000006, 0.0])[torch.randint(0, 3, (S,), generator=g)]
    # one positive, first or last in the order among the valid positions (any member of that group)
    labels, at = torch.zeros(S), valid.nonzero().flatten()
    if at.numel():
        key = torch.where(torch.isnan(scores), torch.full_like(scores, -math.inf), scores)[at]
        labels[at[key.argmax() if kind == "one_first" else key.argmin()]] = 1.0
    return labels


def rows(S, B, seed, first=0):
    """B rows that walk through FAMILIES x VALIDITY x LABELS from combination ``first`` on."""
    g = torch.Generator().manual_seed(seed)
    scores, valid, labels, names = [], [], [], []
    for r in range(B):
        c = first + r
        family, validity, label = FAMILIES[c % 6], VALIDITY[(c // 6) % 3], LABELS[(c // 18) % 6]
        scores.append(score_row(family, S, g))
        valid.append(valid_row(validity, S, g))
        labels.append(label_row(label, scores[-1], valid[-1], g))
        names.append("%s/%s/%s" % (family, validity, label))
    return torch.stack(scores), torch.stack(valid), torch.stack(labels), names


def launch(scores, valid, labels):
    """The C entry point on outputs the test fills itself (NaN, -1): every element must be written."""
    from case_rg_amd import _abi
    B, S = scores.shape
    dev = lambda t: None if t is None else t.cuda().contiguous()  # noqa: E731
    s, v, l = dev(scores), dev(valid), dev(labels)
    stats = torch.full((B, 2), math.nan, dtype=torch.float64, device="cuda")
    counts = torch.full((B, 6), -1, dtype=torch.int32, device="cuda")
    threshold = torch.full((B,), math.nan, dtype=torch.float32, device="cuda")
    _abi.call("case_token_rank", s.data_ptr(), None if v is None else v.view(torch.uint8).data_ptr(), l.data_ptr(), stats.data_ptr(),
              counts.data_ptr(), threshold.data_ptr(), B, S, torch.cuda.current_stream().cuda_stream)
    return dict(stats=stats.cpu(), counts=counts.cpu(), threshold=threshold.cpu())


def f32_bits(x):
    return torch.tensor(x, dtype=torch.float32).view(torch.int32).item()


def compare(got, want, names, tag):
    """K45's three outputs (host tensors) against ``token_rank_host``'s rows -> the largest distance of ``ap`` from the Fraction."""
    from case_rg_amd import ops
    worst = 0.0
    assert got["counts"].dtype == torch.int32 and got["stats"].dtype == torch.float64 and got["threshold"].dtype == torch.float32
    for b, (w, name) in enumerate(zip(want, names)):
        where = "%s row %d (%s)" % (tag, b, name)
        assert got["counts"][b].tolist() == [w[k] for k in ops.TOKEN_RANK_COUNTS], (where, got["counts"][b].tolist(), w)
        assert f32_bits(got["threshold"][b].item()) == f32_bits(w["best_threshold"]), (where, got["threshold"][b].item(), w["best_threshold"])
        ap, auc = got["stats"][b].tolist()
        want_auc = 0.0 if w["auc"] is None else float(w["auc"])
        assert auc == want_auc and math.copysign(1.0, auc) == 1.0, (where, auc, want_auc)
        assert ap == ap, where
        gap = float(abs(Fraction(ap) - w["ap"]))
        assert gap <= AP_BAR, (where, ap, float(w["ap"]), gap)
        worst = max(worst, gap)
    return worst


def check(scores, valid, labels, names, tag):
    from case_rg_amd.evaluation import token_rank_host
    got = launch(scores, valid, labels)
    gap = compare(got, token_rank_host(scores, labels, valid), names, tag)
    print("token_rank(%s): %d rows, max |ap - exact| %.3e" % (tag, scores.shape[0], gap))
    record_error("token_rank", "f64", tag, gap, AP_BAR)
    return got


# ---------------------------------------------------------------------------------------------
# 1. parity with the exact host form
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", SIZES)
def test_token_rank_against_the_exact_host_form(S):
    seed = 460 + 7 * S
    s, v, l, names = rows(S, 1, seed, first=S % 108)
    check(s, v, l, names, "S%d_B1" % S)
    groups = pos = 0
    if S <= 1025:  # every combination of family, validity and labels, and 22 more
        s, v, l, names = rows(S, 130, seed + 1)
        got = check(s, v, l, names, "S%d_B130" % S)
        groups, pos = int(got["counts"][:, 5].max()), int(got["counts"][:, 1].sum())
    for i in range(6):  # B = 3: every family under another validity and other labels each time
        s, v, l, names = rows(S, 3, seed + 2 + i, first=(S + 25 * i) % 108)
        got = check(s, v, l, names, "S%d_B3_%d" % (S, i))
        groups, pos = max(groups, int(got["counts"][:, 5].max())), pos + int(got["counts"][:, 1].sum())
    s, v, l, names = rows(S, 3, seed + 8)
    check(s, None, l, names, "S%d_B3_valid_none" % S)
    if S > 2:
        assert groups > S // 2 and pos > 0, "the inputs prove nothing"


def test_token_rank_planted_runs_sit_on_the_boundaries():
    """The planted family does what it says: in the sorted row, equal scores meet across every chunk boundary of the instance."""
    for S in (257, 4097, 16384):
        _, _, per = instance(S)
        ranked = score_row("planted_runs", S, torch.Generator().manual_seed(1)).sort(descending=True).values
        assert all(ranked[b] == ranked[b - 1] for b in range(max(per, 2), S, max(per, 2))) and ranked.unique().numel() > S // 4
    s, v, l, names = rows(16384, 1, 461, first=4)
    assert names == ["planted_runs/all/random"]
    check(s, v, l, names, "S16384_planted")


# ---------------------------------------------------------------------------------------------
# 2. the neighbours: K38's counts, K36's map
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [65, 1024, 3840])
def test_counts_are_k38s(S):
    from case_rg_amd import ops
    s, v, l, _ = (t.cuda() if torch.is_tensor(t) else t for t in rows(S, 36, 462 + S))
    with Calls() as c:
        got = ops.token_rank(s, v, l)
    assert c.calls == {"case_token_rank": 1}
    k38 = ops.token_select(s, v, 1, labels=l)["counts"]
    assert torch.equal(got["counts"][:, :2], k38[:, :2]) and int(k38[:, 1].sum()) > 0


@pytest.mark.parametrize("S", [1, 64, 257, 1024])
def test_ap_is_k36s_map_on_tie_free_rows(S):
    from case_rg_amd import ops
    g = torch.Generator().manual_seed(463 + S)
    B = 12
    s = torch.stack([score_row("tie_free", S, g) for _ in range(B)]).cuda()
    v = (torch.rand(B, S, generator=g) < 0.8).cuda()
    v[0] = True
    l = (torch.rand(B, S, generator=g) < 0.3).float().cuda()
    l[0, 0] = 1.0
    got = ops.token_rank(s, v, l)
    k36 = ops.rank_metrics(s, (l > 0.5).int(), valid=v)
    assert torch.equal(got["counts"][:, 1], k36["num_rel"]) and int(k36["num_rel"].sum()) > 0
    gap = float((got["stats"][:, 0] - k36["metrics"][:, ops.RANK_METRICS.index("map")]).abs().max())
    print("token_rank ap against rank_metrics map, S %d: max distance %.3e" % (S, gap))
    record_error("token_rank", "f64", "S%d_vs_k36_map" % S, gap, AP_BAR)
    assert gap <= AP_BAR


# ---------------------------------------------------------------------------------------------
# 3. the wrapper, determinism, capture
# ---------------------------------------------------------------------------------------------
def test_the_wrapper_and_the_evaluation_module_name_the_columns():
    from case_rg_amd import ops
    from case_rg_amd.evaluation import eval_token_rank_ids, token_rank_host, token_rank_ids
    s, v, l, names = rows(63, 60, 464)
    want = token_rank_host(s, l, v)
    got = ops.token_rank(s.cuda(), v.cuda(), l.cuda().double())  # (labels of any float dtype)
    assert set(got) == {"stats", "counts", "threshold"} and all(t.is_cuda for t in got.values())
    compare({k: t.cpu() for k, t in got.items()}, want, names, "wrapper")
    cube = lambda t: t.cuda().reshape(60, 3, 21)  # noqa: E731
    other = torch.randn(60, 3, 21, device="cuda")
    with Calls() as c:
        by_name = token_rank_ids(other, cube(l), cube(v), select=cube(s))
    assert c.calls == {"case_token_rank": 1}
    assert set(by_name) == set(ops.TOKEN_RANK_COUNTS) | {"n_neg", "ap", "auc", "best_threshold"}
    for i, name in enumerate(ops.TOKEN_RANK_COUNTS):
        assert by_name[name].dtype == torch.int64 and torch.equal(by_name[name], got["counts"][:, i].long()), name
    assert torch.equal(by_name["n_neg"].cpu(), torch.tensor([w["n_neg"] for w in want]))
    assert torch.equal(by_name["ap"], got["stats"][:, 0]) and torch.equal(by_name["auc"], got["stats"][:, 1])
    assert by_name["ap"].dtype == torch.float64 and by_name["best_threshold"].dtype == torch.float32
    assert torch.equal(by_name["best_threshold"].view(torch.int32), got["threshold"].view(torch.int32))
    own = token_rank_ids(cube(s), cube(l), cube(v))
    assert torch.equal(own["auc_num2"], by_name["auc_num2"])
    sums = eval_token_rank_ids(other, cube(l), cube(v), select=cube(s))
    assert sums.is_cuda and sums.dtype == torch.float64 and sums.shape == (8,)
    ints = [sum(w["n_pos"] > 0 for w in want), sum(w["auc"] is not None for w in want), sum(w["auc_num2"] for w in want),
            sum(2 * w["n_pos"] * w["n_neg"] for w in want), sum(w["best_tp"] for w in want), sum(w["best_n"] + w["n_pos"] for w in want)]
    assert sums[2:].tolist() == [float(x) for x in ints] and ints[0] > ints[1] > 0
    assert abs(float(sums[0]) - float(sum(w["ap"] for w in want))) <= 60 * AP_BAR
    assert abs(float(sums[1]) - float(sum(w["auc"] or 0 for w in want))) <= 60 * AP_BAR
    empty = ops.token_rank(s.cuda()[:0], v.cuda()[:0], l.cuda()[:0])
    assert empty["stats"].shape == (0, 2) and empty["counts"].shape == (0, 6) and empty["threshold"].shape == (0,)


def test_token_rank_limits_raise_before_any_launch():
    from case_rg_amd import _abi, ops
    s = torch.zeros(2, 16385, device="cuda")
    with Calls() as c:
        with pytest.raises(ValueError, match="16384 positions"):
            ops.token_rank(s, None, s)
        with pytest.raises(ValueError, match="on the device"):
            ops.token_rank(s[:, :8].contiguous(), None, torch.zeros(2, 8))
        with pytest.raises(ValueError, match="labels must be float"):
            ops.token_rank(s[:, :8].contiguous(), None, torch.zeros(2, 9, device="cuda"))
    assert c.calls == {}
    out = torch.zeros(16, device="cuda", dtype=torch.float64)
    with pytest.raises(Exception, match="case_token_rank"):
        _abi.call("case_token_rank", s.data_ptr(), None, s.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), 1, 16385,
                  torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("S", [200, 3840, 16384])
def test_token_rank_is_deterministic_and_replays_from_a_captured_graph(S):
    from case_rg_amd import ops
    first, second = ([t.cuda() for t in rows(S, 12, 465 + i)[:3]] for i in range(2))
    call = lambda t: ops.token_rank(t[0], t[1], t[2])  # noqa: E731
    eager, again = call(second), call(second)
    bits = lambda t: t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)  # noqa: E731
    for k in eager:
        assert torch.equal(bits(eager[k]), bits(again[k])), k
    buf = [t.clone() for t in first]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(buf)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), Calls() as c:
        static = call(buf)
    assert c.calls == {"case_token_rank": 1}
    for dst, src in zip(buf, second):
        dst.copy_(src)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(bits(static[k]), bits(eager[k])), "the replay differs from the eager call in %s" % k
    assert not torch.equal(eager["counts"], call(first)["counts"]), "the two sets of rows must differ"
    del graph


# ---------------------------------------------------------------------------------------------
# 4. the model: do_extract(ranking=True), evaluate_extract(ranking=True)
# ---------------------------------------------------------------------------------------------
ITEMS, P, L = 4, 3, 16
RANK_KEYS = {"token_ap", "token_auc", "rank_counts", "best_threshold"}


@pytest.fixture(params=["fp32", "bf16"])
def tiny(request, ns):
    """A tiny CaSE at P 3, L 16 in eval mode, and its batch on the device."""
    import case_rg_amd
    from case_rg_amd.utils import synth_batch
    case_rg_amd.set_compute_dtype(torch.bfloat16 if request.param == "bf16" else torch.float32)
    try:
        m = cases._case_model(ns, torch.device("cuda"), 466, gain=3.0).eval()
        b = {k: v.cuda() for k, v in synth_batch(ITEMS, P, L, 8, 6, cases.V, seed=467, model="case").items()}
        m.set_token_freq(torch.from_numpy(np.random.RandomState(468).randint(0, 10 ** 5, cases.V)))
        yield m, b, request.param
    finally:
        case_rg_amd.set_compute_dtype(torch.float32)


def model_outputs(out):
    return dict(stats=torch.stack([out["token_ap"], out["token_auc"]], 1).cpu(), counts=out["rank_counts"].cpu(),
                threshold=out["best_threshold"].cpu())


@pytest.mark.parametrize("select", ["prior", "score"])
def test_do_extract_with_ranking_adds_one_launch_and_four_keys(tiny, select):
    from case_rg_amd.evaluation import token_rank_host
    m, b, mode = tiny
    gold = b["token_label"]
    with torch.no_grad():
        m.do_extract(dict(b))  # (the first pass of a model also fills the cache of bf16 operands: not counted)
        with Calls() as plain:
            base = m.do_extract(dict(b), select=select, labels=gold)
        with Calls() as c:
            out = m.do_extract(dict(b), select=select, labels=gold, ranking=True)
        with pytest.raises(ValueError, match="needs labels"):
            m.do_extract(dict(b), select=select, ranking=True)
    assert set(out) == set(base) | RANK_KEYS and "token_ap" not in base
    assert c.calls == dict(plain.calls, case_token_rank=1) and "case_token_rank" not in plain.calls
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t  # noqa: E731
    for k in base:
        assert base[k].dtype == out[k].dtype and torch.equal(bits(base[k]), bits(out[k])), k
    assert out["token_ap"].dtype == out["token_auc"].dtype == torch.float64 and out["token_ap"].shape == (ITEMS,)
    assert out["rank_counts"].dtype == torch.int32 and out["rank_counts"].shape == (ITEMS, 6) and out["best_threshold"].dtype == torch.float32
    flat = lambda t: t.reshape(ITEMS, -1).cpu()  # noqa: E731
    key = out["token_prior"] if select == "prior" else out["token_score"]
    want = token_rank_host(flat(key), flat(gold), flat(b["passage"].ne(0)))
    gap = compare(model_outputs(out), want, [select] * ITEMS, "do_extract_%s_%s" % (mode, select))
    record_error("token_rank", mode, "do_extract_%s" % select, gap, AP_BAR)
    assert torch.equal(out["rank_counts"][:, :2], out["counts"][:, :2]), "n_valid and n_pos are K38's"
    assert sum(w["n_pos"] for w in want) > 0 and sum(w["n_neg"] for w in want) > 0


def test_trainer_evaluate_extract_with_ranking_is_predict_plus_the_host_form(tiny, ns):
    from case_rg_amd.evaluation import token_rank_host
    m, b, mode = tiny
    data = {k: v.cpu() for k, v in b.items()}
    trainer = ns.CumulativeTrainer(m, None, None, None, 1)
    ds = cases._ListDataset(data)
    base_keys = {"precision", "recall", "f1", "precision_at_k", "recall_at_k", "items", "tokens"}
    try:
        for select in ("prior", "score"):
            base = trainer.evaluate_extract(ds, cases._collate, 3, select=select)
            assert set(base) == base_keys, "the default call returns what it did"
            trainer.model.train()
            with Calls() as c:
                got = trainer.evaluate_extract(ds, cases._collate, 3, select=select, ranking=True)
            assert trainer.model.training, "the mode must be restored"
            assert c.count("case_token_rank") == 2, "two batches (3 items and 1): one launch each"
            assert set(got) == base_keys | {"map", "auc", "auc_stratified", "oracle_f1", "ranked_items", "auc_items"}
            assert {k: got[k] for k in base_keys} == base and all(type(got[k]) is type(base[k]) for k in base_keys)
            want = []
            for batch, out in trainer.predict("extract", ds, cases._collate, 3):
                ids = batch["id"].cpu()
                flat = lambda t: t.reshape(len(ids), -1).cpu()  # noqa: E731
                key = out["token_prior"] if select == "prior" else out["token_score"]
                want += token_rank_host(flat(key), flat(data["token_label"][ids]), flat(batch["passage"].ne(0)))
            assert len(want) == ITEMS
            ranked, both = [w for w in want if w["n_pos"]], [w for w in want if w["auc"] is not None]
            ratio = lambda x, y: x / y if y else 0.0  # noqa: E731
            assert got["ranked_items"] == len(ranked) > 0 and got["auc_items"] == len(both) > 0
            assert got["auc_stratified"] == ratio(sum(w["auc_num2"] for w in want), sum(2 * w["n_pos"] * w["n_neg"] for w in want))
            assert got["oracle_f1"] == ratio(2 * sum(w["best_tp"] for w in want), sum(w["best_n"] + w["n_pos"] for w in want))
            gap = abs(got["map"] - float(sum(w["ap"] for w in ranked) / len(ranked)))
            record_error("token_rank", mode, "evaluate_extract_%s_map" % select, gap, AP_BAR)
            assert gap <= AP_BAR, (got["map"], gap)
            assert abs(got["auc"] - float(sum(w["auc"] for w in both) / len(both))) <= AP_BAR
            print("evaluate_extract(%s, %s, ranking): %s" % (mode, select, got))
        empty = trainer.evaluate_extract(cases._ListDataset({k: v[:0] for k, v in data.items()}), cases._collate, 3, ranking=True)
        assert empty["items"] == 0 and math.isnan(empty["map"]) and math.isnan(empty["oracle_f1"]) and empty["ranked_items"] == 0
    finally:
        m.eval()
        trainer.close()
