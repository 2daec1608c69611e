"""TREC ranking metrics on the MI355X: K36 (``case_rank_metrics``) against the restatement of tests/test_trec_cpu.py (``sorted`` on (-score,
reversed key) and naive ``Fraction`` sums) at the wave, workgroup and padding boundaries of its sorts and up to its limits; that every
output element is written; the limits; determinism; stream capture; the rank-only pass ``do_rank`` of both task models against
``do_test(...)['rank']``; the trainer's ``evaluate_rank`` against ``predict`` + the host form ``evaluation.rank_metrics``.

``pytrec_eval`` is not available where the fixtures are built, so no number here comes from running the reference's ``Eval_Trec.py``; the
restatement is pinned to hand-derived examples in tests/test_trec_cpu.py.

``order`` and ``num_rel`` are integers and compared exactly; ``recall_*``, ``recip_rank`` and ``P_1`` are one f64 division of two small
integers and compared exactly.  ``map`` and ``ndcg`` are compared at 1e-12 absolute (the project's D_TOL), here derived: at most 1024 f64
terms in [0, 1] summed in another order differ by less than 1024 x 1.1e-16 = 1.2e-13, and the device ``log2`` adds a few ulp per term.
Measured maxima go to the session's parity ledger (``helpers.record_error``, case "rank"); profiles/rank_parity.json keeps a copy."""
import math
import random

import pytest
import torch

import cases
import sample_cases
from helpers import Calls, record_error
from test_trec_cpu import EXACT, NAMES, random_row, restated_row

pytestmark = pytest.mark.gpu

D_TOL = 1e-12
SPECIAL_SCORES = (-0.0, 0.0, math.inf, -math.inf, math.nan, 1.0, -1.0)


@pytest.fixture(scope="module")
def ns():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.float32)
    case_rg_amd.set_dropout(False)
    return case_rg_amd.namespace()


def _note(key, value, tol=D_TOL):
    record_error("rank", "f64", key, value, tol)


def make_rows(P, R, seed, with_keys):
    """Five queries of P slots and R judged-but-unretrieved grades: 0 random (ties common, a third of the slots invalid), 1 all scores equal
    (with keys: drawn from four values, so that equal (score, key) pairs fall back on the column), 2 scores from -0.0, +0.0, +-inf, NaN and
    +-1, 3 all slots invalid, 4 no relevant document anywhere.  -> dict of lists per row."""
    rs = random.Random(seed)
    rows = dict(scores=[], keys=[], rel=[], valid=[], extra=[])
    for b in range(5):
        scores, keys, rel, extra = random_row(rs, P, R, with_keys)
        valid = [True] * P
        if b == 0:
            valid = [rs.random() < 2 / 3 for _ in range(P)]
        if b == 1:
            scores = [0.25] * P
            keys = [rs.choice((-7, 0, 3, 2 ** 31 - 1)) for _ in range(P)] if with_keys else keys
        if b == 2:
            scores = [rs.choice(SPECIAL_SCORES) for _ in range(P)]
        if b == 3:
            valid = [False] * P
        if b == 4:
            rel, extra = [min(g, 0) for g in rel], [min(g, 0) for g in extra]
        for name, v in zip(("scores", "keys", "rel", "valid", "extra"), (scores, keys, rel, valid, extra)):
            rows[name].append(v)
    return rows


def to_device(rows, with_keys, R):
    dev = lambda v, dt: torch.tensor(v, dtype=dt).cuda()  # noqa: E731
    return dict(scores=dev(rows["scores"], torch.float32), rel=dev(rows["rel"], torch.int32),
                keys=dev(rows["keys"], torch.int32) if with_keys else None, valid=dev(rows["valid"], torch.bool),
                extra_rel=dev(rows["extra"], torch.int32) if R else None)


def check_against_restatement(got, rows, tag):
    """-> the worst |map| and |ndcg| gaps; everything else must be equal."""
    order, metrics, num_rel = got["order"].cpu().tolist(), got["metrics"].cpu().numpy(), got["num_rel"].cpu().tolist()
    worst = dict(map=0.0, ndcg=0.0)
    for b in range(len(rows["scores"])):
        want_order, want, want_rel = restated_row(rows["scores"][b], rows["keys"][b], rows["rel"][b], rows["valid"][b], rows["extra"][b])
        assert order[b] == want_order, "%s row %d: order differs, first at rank %d" % (
            tag, b, next(i for i, (x, y) in enumerate(zip(order[b], want_order)) if x != y))
        assert num_rel[b] == want_rel, "%s row %d: num_rel %d, restatement %d" % (tag, b, num_rel[b], want_rel)
        for name in EXACT:
            assert metrics[b, NAMES.index(name)] == want[name], "%s row %d: %s %r, restatement %r" % (
                tag, b, name, metrics[b, NAMES.index(name)], want[name])
        for name in worst:
            worst[name] = max(worst[name], abs(metrics[b, NAMES.index(name)] - want[name]))
    return worst


# ---------------------------------------------------------------------------------------------
# 1. K36 against the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 7, "full"])
@pytest.mark.parametrize("P", [1, 10, 63, 64, 65, 256, 257, 1000, 1024])
def test_rank_metrics_against_the_restatement(P, R):
    """R = "full": P + R = 2048.  The tie keys are given for R = 0 and "full" and left to the column index for R = 7."""
    from case_rg_amd import ops
    R = 2048 - P if R == "full" else R
    with_keys = R != 7
    rows = make_rows(P, R, 361 + 7 * P + R, with_keys)
    if not with_keys:
        assert all(k == list(range(P)) for k in rows["keys"])
    with Calls() as c:
        got = ops.rank_metrics(**to_device(rows, with_keys, R))
    assert c.calls == {"case_rank_metrics": 1}
    assert got["order"].dtype == torch.int32 and got["order"].shape == (5, P) and got["num_rel"].dtype == torch.int32
    assert got["metrics"].dtype == torch.float64 and got["metrics"].shape == (5, 13) and got["num_rel"].shape == (5,)
    worst = check_against_restatement(got, rows, "P %d R %d" % (P, R))
    for name, w in worst.items():
        print("rank_metrics(P %d, R %d): max |%s - restatement| = %.3e" % (P, R, name, w))
        _note("%s_p%d_r%d" % (name, P, R), w)
    m = got["metrics"].cpu().numpy()
    assert got["order"][3].eq(-1).all() and not m[3].any(), "an all-invalid row retrieves nothing"
    assert int(got["num_rel"][4]) == 0 and not m[4].any(), "num_rel == 0: every metric is 0"
    if P >= 10:
        assert m[:3, 0].min() > 0 and m[:3, 1].min() > 0 and len(set(m[:3, 0])) == 3, "the inputs prove nothing"
    assert worst["map"] <= D_TOL and worst["ndcg"] <= D_TOL, worst


def test_rank_metrics_ids_labels_and_sums():
    """The id-tensor layer: a gold index int64 [B] and a grade tensor int64 [B, P] of the same content give the same columns; named columns
    are the kernel's; ``eval_rank_ids`` is their column sum.  With one gold slot map == recip_rank."""
    from case_rg_amd import ops
    from case_rg_amd.evaluation import eval_rank_ids, rank_metrics_ids
    g = torch.Generator().manual_seed(362)
    B, P = 6, 10
    scores = torch.randint(0, 4, (B, P), generator=g).float().cuda()
    gold = torch.randint(0, P, (B,), generator=g).cuda()
    grades = torch.zeros(B, P, dtype=torch.int64, device="cuda").scatter_(1, gold.unsqueeze(1), 1)
    a, b = rank_metrics_ids(scores, gold), rank_metrics_ids(scores, grades)
    assert set(a) == set(ops.RANK_METRICS) | {"order", "num_rel"}
    for key in a:
        assert torch.equal(a[key], b[key]), key
    assert torch.equal(a["map"], a["recip_rank"]) and a["map"].dtype == torch.float64 and a["map"].shape == (B,)
    assert a["num_rel"].tolist() == [1] * B and torch.equal(a["recall_5"] + 0, (a["recip_rank"] >= 0.2).double())
    for b_ in range(B):
        want = restated_row(scores[b_].tolist(), list(range(P)), grades[b_].tolist())[1]
        assert all(float(a[name][b_]) == want[name] for name in NAMES), b_
    total = eval_rank_ids(scores, gold)
    assert total.is_cuda and total.dtype == torch.float64 and total.shape == (13,)
    assert torch.equal(total, torch.stack([a[name] for name in ops.RANK_METRICS], 1).sum(0))


# ---------------------------------------------------------------------------------------------
# 2. output buffers, limits, determinism, capture
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,R", [(10, 7), (257, 7), (1024, 1024)])
def test_rank_metrics_writes_every_output_element(P, R):
    """Through the C ABI onto NaN- and -2-filled buffers, keys and valid NULL."""
    from case_rg_amd import _abi
    rows = make_rows(P, R, 363 + P, False)
    t = to_device(rows, False, R)
    B = 5
    order = torch.full((B, P), -2, dtype=torch.int32, device="cuda")
    num_rel = torch.full((B,), -2, dtype=torch.int32, device="cuda")
    metrics = torch.full((B, 13), math.nan, dtype=torch.float64, device="cuda")
    _abi.call("case_rank_metrics", t["scores"].data_ptr(), None, t["rel"].data_ptr(), None, t["extra_rel"].data_ptr(), order.data_ptr(),
              metrics.data_ptr(), num_rel.data_ptr(), B, P, R, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not order.eq(-2).any() and not num_rel.eq(-2).any() and not torch.isnan(metrics).any()
    assert order.sort(1).values.eq(torch.arange(P, dtype=torch.int32, device="cuda")).all(), "without a mask every row is a permutation"
    rows["valid"] = [[True] * P] * B
    check_against_restatement(dict(order=order, metrics=metrics, num_rel=num_rel), rows, "C ABI P %d" % P)


def test_rank_metrics_limits_raise_before_any_launch():
    from case_rg_amd import _abi, ops
    z = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")  # noqa: E731
    with Calls() as c:
        with pytest.raises(ValueError, match="up to 1024 retrieved"):
            ops.rank_metrics(torch.zeros(2, 1025, device="cuda"), z(2, 1025))
        with pytest.raises(ValueError, match="2048 judged"):
            ops.rank_metrics(torch.zeros(2, 1000, device="cuda"), z(2, 1000), extra_rel=z(2, 1049))
    assert c.calls == {}
    # the C entry refuses the same shapes with an error code (raised by the ctypes layer), and launches nothing
    s, r, o, m, n = torch.zeros(1, 1025, device="cuda"), z(1, 1025), z(1, 1025), torch.zeros(1, 13, dtype=torch.float64, device="cuda"), z(1)
    with pytest.raises(Exception, match="case_rank_metrics"):
        _abi.call("case_rank_metrics", s.data_ptr(), None, r.data_ptr(), None, None, o.data_ptr(), m.data_ptr(), n.data_ptr(), 1, 1025, 0,
                  torch.cuda.current_stream().cuda_stream)
    ops.rank_metrics(torch.zeros(2, 1000, device="cuda"), z(2, 1000), extra_rel=z(2, 1048))  # P + R = 2048 is inside


def test_rank_metrics_is_deterministic():
    from case_rg_amd import ops
    t = to_device(make_rows(1000, 7, 364, True), True, 7)
    first, second = ops.rank_metrics(**t), ops.rank_metrics(**t)
    for key in ("order", "metrics", "num_rel"):
        assert torch.equal(first[key], second[key]), key


def test_rank_metrics_replays_from_a_captured_graph():
    """Nothing in the call waits for the host: captured once, the replay on new rows written into the same buffers is the eager call."""
    from case_rg_amd import ops
    P, R = 65, 7
    first, second = to_device(make_rows(P, R, 365, True), True, R), to_device(make_rows(P, R, 366, True), True, R)
    eager = {k: v.clone() for k, v in ops.rank_metrics(**second).items()}
    buf = {k: v.clone() for k, v in first.items()}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.rank_metrics(**buf)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph, static = torch.cuda.CUDAGraph(), {}
    with torch.cuda.graph(graph), Calls() as c:
        static.update(ops.rank_metrics(**buf))
    assert c.calls == {"case_rank_metrics": 1}
    for k in buf:
        buf[k].copy_(second[k])
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(static[k], eager[k]), "the replay differs from the eager call in %s" % k
    assert not torch.equal(eager["order"], ops.rank_metrics(**first)["order"]), "the two sets of rows must differ"
    del graph


# ---------------------------------------------------------------------------------------------
# 3. the rank-only pass
# ---------------------------------------------------------------------------------------------
def _heads(c):
    return sum(n for name, n in c.calls.items() if name.startswith("case_pointer"))


@pytest.mark.parametrize("name", ["sample_case", "sample_masque"])
def test_do_rank_is_do_tests_rank_without_the_decoder(ns, name):
    m, b = sample_cases.build(ns, torch.device("cuda"), name)
    m.eval()
    with torch.no_grad():
        with Calls() as full:
            test = m.do_test(dict(b))
        with Calls() as c:
            out = m.do_rank(dict(b))
        routed = m(dict(b), method="rank")
    assert set(out) == set(routed) == {"rank"} and out["rank"].shape == (sample_cases.ITEMS, 3)
    assert out["rank"].dtype == test["rank"].dtype and torch.equal(out["rank"], test["rank"]) and torch.equal(routed["rank"], test["rank"])
    assert _heads(full) >= sample_cases.T, "the counter must see do_test's head calls: %s" % full.calls
    assert _heads(c) == 0 and sum(c.calls.values()) < sum(full.calls.values()), c.calls
    m.train()
    with pytest.raises(ValueError, match="eval mode"):
        m.do_rank(dict(b))
    with pytest.raises(ValueError, match="eval mode"):
        m(dict(b), method="rank")
    m.eval()


# ---------------------------------------------------------------------------------------------
# 4. the trainer
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sample_case", "sample_masque"])
def test_trainer_evaluate_rank_is_the_host_form(ns, name):
    """Four items in batches of 3 and 1, every item its own query; docids are zero-padded integers, so that string order = integer order.
    First with the column index as the docid; then with ``docno`` tie keys and a ``slots`` mask from the data (one non-gold slot of item
    0 is not retrieved)."""
    from case_rg_amd.evaluation import rank_metrics
    from case_rg_amd.evaluation.trec import mean_metrics
    m, b = sample_cases.build(ns, torch.device("cuda"), name)
    data = {k: v.cpu() for k, v in b.items()}
    B, P = data["passage"].shape[:2]
    gold = data["passage_label"]
    data["docno"] = torch.tensor([[5, 9, 7], [1, 2, 3], [30, 20, 10], [4, 6, 8]])[:B, :P]
    data["slots"] = torch.ones(B, P, dtype=torch.bool)
    data["slots"][0, (int(gold[0]) + 1) % P] = False
    trainer = ns.CumulativeTrainer(m, None, None, None, 1)
    ds = cases._ListDataset(data)
    for keys, valid in ((None, None), ("docno", "slots")):
        trainer.model.train()
        got = trainer.evaluate_rank(ds, cases._collate, 3, keys=keys, valid=valid)
        assert trainer.model.training, "the mode must be restored"
        run, qrel = {}, {}
        for batch, out in trainer.predict("test", ds, cases._collate, 3):
            for i in range(out["rank"].shape[0]):
                qid = "q%d" % int(batch["id"][i])
                docid = lambda j: "%03d" % (int(batch[keys][i, j]) if keys else j)  # noqa: E731, B023
                run[qid] = {docid(j): float(out["rank"][i, j]) for j in range(P) if valid is None or bool(batch[valid][i, j])}
                qrel[qid] = {docid(int(batch["passage_label"][i])): 1}
        assert len(run) == B
        want = mean_metrics(rank_metrics(run, qrel))
        print("evaluate_rank(%s, keys %s): %s" % (name, keys, got))
        assert set(got) == set(NAMES) | {"items"} and got["items"] == B
        for key in EXACT:
            assert got[key] == want[key], (key, got[key], want[key])
        for key in ("map", "ndcg"):
            _note("trainer_%s_%s_%s" % (key, name, keys), abs(got[key] - want[key]))
            assert abs(got[key] - want[key]) <= D_TOL, (key, got[key], want[key])
        assert got["map"] == got["recip_rank"] > 0.0, "one gold passage per item"
        via_test = trainer.evaluate_rank(ds, cases._collate, 3, method="test", keys=keys, valid=valid)
        assert via_test == got, "method='test' carries the same rank"
    trainer.close()
