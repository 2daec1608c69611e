"""One walk over the 24 ways to call a fused decode head on the MI355X: K23 argmax / K24 top-W / K28 draw x the row in LDS / in device memory
x with and without the n-gram ban x with and without the decoding rules, at the smallest shapes that still reach every branch.

Per combination: exactly the tabled entry point runs (tests/test_head_entries_cpu.py::NAMES); the outputs stand against the float64 row of
K23's docstring with the suite's restatements applied to it (the n-gram rule ``Utils.banned_tokens``, ``restate_rows`` / ``ordered_top`` of
tests/test_decode_rules_cpu.py, the draw rule of tests/golden/sample_cases.py) at the bars tests/test_wide_head_gpu.py uses for the same
quantities; the other row form returns the same bits; the history is appended exactly where it should be.

Shapes: two memories of 5 + 3 positions (S = 8); V = 37 (a workspace stride rounded up to 40, unaligned rows); V = 40 for K28 on a ready
distribution (the wide form reads it in place); 3 rows for the argmax and the draw, B = 2 x W = 2 = 4 rows for the top-W; Tmax 6, step 3,
n = 2 with histories [a, w, a] that ban w, the row's winner; the rules keep EOS = 4 out (min_length 5 > t) and ban ids 7 / 9 / 100 / -1:
per item [[7, -1], [9, 100]] with two rows per item for the top-W (stride K), as the one list [7, -1, 9, 100] for the three rows of the
argmax and the draw (stride 0; two lists do not divide three rows).  Every row's first entries are planted in the order winner > the row's
banned id > the other list's id > EOS, so the ban, each rule and the choice of the item's list all change what is returned.

No comparison sits on a near-tie: ``MIN_GAP`` is asserted on the float64 rows before anything is compared."""
import numpy as np
import pytest
import torch

from helpers import Calls, to_np
from sample_cases import draw
from test_decode_rules_cpu import ordered_top, restate_rows
from test_head_entries_cpu import NAMES

pytestmark = pytest.mark.gpu

LENS, S = (5, 3), 8
TMAX, T_STEP, N = 6, 3, 2
EOS, MIN_LENGTH, UNK, PAD = 4, 5, 2, 0
LISTS = np.asarray([[7, -1], [9, 100]], dtype=np.int32)
W = 2
DRAW = (0.7, 5, 0.9)  # temperature, top_k, top_p
UNIFORMS = (0.15, 0.55, 0.9)
GEN_BAR, DIST_BAR = (2e-5, 1e-9), (3e-5, 1e-8)  # (rtol, atol) of tests/test_wide_head_gpu.py for gen and for dist / cand_p / prob
# Two different values of a compared row, and a draw's threshold and the masses around it, lie at least this far apart (relative): thirty
# times the rtol of DIST_BAR, so no id below depends on f32 rounding
MIN_GAP = 1e-3


def _plant(logits):
    """The first four entries of every row, in order: the winner 11 + r, the row's banned id, the other list's id, EOS."""
    R = logits.shape[0]
    top = logits.max(dim=1).values
    for r in range(R):
        mine, other = (7, 9) if (r < 2 if R == 4 else r % 2 == 0) else (9, 7)
        logits[r, 11 + r] = top[r] + 3.0
        logits[r, mine] = top[r] + 2.5
        logits[r, other] = top[r] + 2.25
        logits[r, EOS] = top[r] + 2.0


def _inputs(R, V, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(R, V, generator=g) * 2.0
    src = torch.randint(0, V, (R, S), generator=g)
    src[:, 0] = V - 1
    mix = torch.randn(R, 1 + len(LENS), generator=g)
    mix[:, 0] = 3.0  # (the generator decides the order of the planted entries; the pointer mass still moves every row)
    copies = [torch.softmax(torch.randn(R, n, generator=g) * 2.0, dim=-1) for n in LENS]
    _plant(logits)
    return logits, mix, src, copies


def _float64_row(logits, mix, src, copies):
    """The docstring of K23 in float64: gen = softmax(logits); pm = softmax(mix); dist = pm_0 gen + the pointer mass scattered over the source."""
    x = logits.numpy().astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    gen = e / e.sum(axis=1, keepdims=True)
    m = mix.numpy().astype(np.float64)
    pm = np.exp(m - m.max(axis=1, keepdims=True))
    pm /= pm.sum(axis=1, keepdims=True)
    w = np.concatenate([pm[:, k + 1:k + 2] * c.numpy().astype(np.float64) for k, c in enumerate(copies)], axis=1)
    dist = pm[:, :1] * gen
    for r in range(dist.shape[0]):
        np.add.at(dist[r], src[r].numpy(), w[r])
    return gen, dist


def _history(R):
    h = np.zeros((R, TMAX), dtype=np.int32)
    h[:, 0] = h[:, 2] = 1
    h[:, 1] = 11 + np.arange(R)
    return h


def _rule_lists(R):
    """-> (the lists as ``restate_rows`` and ``ops.row_rules`` take them, rows_per_item)."""
    return (LISTS, 2) if R == 4 else (LISTS.reshape(-1), 1)


def expected_row(base, hist, ban, rules):
    """``base`` [R, V] after the n-gram ban of step T_STEP and then the rules, each where asked for (the same dtype: only zeros are written)."""
    from case_rg_amd.common.Utils import banned_tokens
    R, V = base.shape
    out = np.array(base, copy=True)
    if ban:
        for r in range(R):
            out[r, banned_tokens(hist[r, :T_STEP].tolist(), N, vocab_size=V, eos=EOS)] = 0.0
    if rules:
        lists, rpi = _rule_lists(R)
        out = restate_rows(out, T_STEP, EOS, MIN_LENGTH, lists, rpi)
    return out


def min_gap(rows):
    """The smallest relative distance between two different values of one row, over ``rows``."""
    gap = np.inf
    for row in rows:
        v = np.unique(row)
        v = v[v > 0]
        gap = min(gap, float(((v[1:] - v[:-1]) / v[1:]).min()))
    return gap


def geometry(R, V, seed):
    """The CPU side of one shape: inputs, the float64 rows of the four (ban, rules) variants, and their decisiveness."""
    logits, mix, src, copies = _inputs(R, V, seed)
    gen64, base64 = _float64_row(logits, mix, src, copies)
    hist = _history(R)
    want = {(ban, rules): expected_row(base64, hist, ban, rules) for ban in (False, True) for rules in (False, True)}
    assert base64.argmax(axis=1).tolist() == [11 + r for r in range(R)], "the winner was not planted"
    for (ban, rules), rows in want.items():
        assert min_gap(rows) > MIN_GAP, "ban %s rules %s: two values %.3g apart" % (ban, rules, min_gap(rows))
        assert not ban or (rows[np.arange(R), 11 + np.arange(R)] == 0).all(), "the ban must zero every row's winner"
    tops = {k: [tuple(ordered_top(r, W)) for r in rows] for k, rows in want.items()}
    assert all(len({tops[k][r] for k in tops}) == 4 for r in range(R)), "the ban and the rules must each change every row's first two: %s" % tops
    assert all(tops[(True, False)][r][0] != tops[(True, True)][r][0] for r in range(R)), "behind the ban the rules must change the argmax"
    return dict(R=R, V=V, logits=logits, mix=mix, src=src, copies=copies, gen64=gen64, hist=hist, want=want)


def ready_rows(R, V, seed):
    """A ready f32 distribution [R, V] for K28's ``dist_in`` and what the four variants leave of it (exactly: only zeros are written)."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(R, V, generator=g) * 2.0
    _plant(logits)
    p = torch.softmax(logits, dim=-1)
    hist = _history(R)
    want = {(ban, rules): expected_row(p.numpy(), hist, ban, rules) for ban in (False, True) for rules in (False, True)}
    assert all(min_gap(rows.astype(np.float64)) > MIN_GAP for rows in want.values())
    return dict(R=R, V=V, p=p, hist=hist, want=want)


def expected_draws(rows):
    """The draw rule on float64 rows with UNIFORMS -> (ids, the rows' own probability of them); every draw is decisive."""
    out = [draw(np.asarray(row, dtype=np.float64), *DRAW, u) for row, u in zip(rows, UNIFORMS)]
    assert all(d["margin"] > MIN_GAP for d in out), "a draw within %.3g of a boundary: %s" % (MIN_GAP, [d["margin"] for d in out])
    return [d["id"] for d in out], [d["prob"] for d in out]


def within(got, want, bar):
    """max |got - want| / (atol + rtol |want|): <= 1 is torch.allclose(got, want, rtol, atol)."""
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / (bar[1] + bar[0] * np.abs(want))).max())


def _bits(a):
    return to_np(a).view(np.uint32) if a.is_floating_point() else to_np(a)


def _same(xs, ys):
    return all((x is None and y is None) or np.array_equal(_bits(x), _bits(y)) for x, y in zip(xs, ys))


@pytest.fixture(scope="module")
def shapes():
    from case_rg_amd import ops
    dev = torch.device("cuda")
    out = {}
    for key, R, seed in (("rows3", 3, 3), ("rows4", 4, 9)):  # (seeds whose rows and draws are decisive: what geometry() asserts)
        g = geometry(R, 37, seed)
        g["head"] = (g["logits"].to(dev), g["mix"].to(dev), ops.SortedSource(g["src"].to(dev), g["V"]), [c.to(dev) for c in g["copies"]])
        out[key] = g
    out["ready"] = ready_rows(3, 40, 7)
    out["ready"]["p_dev"] = out["ready"]["p"].to(dev)
    out["uniforms"] = torch.tensor(UNIFORMS, dtype=torch.float32, device=dev)
    return out


def _ban(g, ban, sampler=False):
    """A fresh history on the device and the ``ban=`` of one call (None without a ban)."""
    if not ban:
        return None, None
    h = torch.from_numpy(g["hist"]).cuda()
    return h, ((h, T_STEP, N) if sampler else (h, T_STEP, N, EOS))


def _rules(g, rules):
    from case_rg_amd import ops
    if not rules:
        return None
    lists, rpi = _rule_lists(g["R"])
    return ops.row_rules(EOS, MIN_LENGTH, torch.from_numpy(lists).cuda(), rpi, t=T_STEP)


def _appended(h, g, ban, ids):
    """The history after a call: untouched but for column T_STEP, which holds ``ids`` (None: nothing is appended)."""
    if not ban:
        return
    want = g["hist"].copy()
    if ids is not None:
        want[:, T_STEP] = to_np(ids)
    assert np.array_equal(to_np(h), want), "the history after the call"


def _other(row):
    return "global" if row == "lds" else "lds"


def _routed(calls, name):
    assert calls.count(name) == 1 and sum(calls.count(n) for n in set(NAMES.values())) == 1, "%s expected once: %s" % (name, calls.calls)


COMBOS = sorted(NAMES)


@pytest.mark.parametrize("head,row,ban,rules", COMBOS, ids=["%s-%s-%s-%s" % (h, r, "ban" if b else "noban", "rules" if u else "norules")
                                                               for h, r, b, u in COMBOS])
def test_every_head_call(shapes, head, row, ban, rules):
    from case_rg_amd import ops
    name = NAMES[(head, row, ban, rules)]
    if head == "decode":
        g = shapes["rows3"]
        want = g["want"][(ban, rules)]
        h, b = _ban(g, ban)
        with Calls() as c:
            gen, dist, ids = ops.pointer_head_decode(*g["head"], ban=b, rules=_rules(g, rules), row=row)
        _routed(c, name)
        assert within(to_np(gen), g["gen64"], GEN_BAR) <= 1.0 and within(to_np(dist), want, DIST_BAR) <= 1.0
        assert np.array_equal(to_np(dist) == 0, want == 0), "exactly the restated entries are zeroed"
        assert to_np(ids).tolist() == [int(ordered_top(r, 1)[0]) for r in want]
        _appended(h, g, ban, ids)
        h2, b2 = _ban(g, ban)
        assert _same((gen, dist, ids), ops.pointer_head_decode(*g["head"], ban=b2, rules=_rules(g, rules), row=_other(row))), "LDS and global rows differ"
        assert h is None or np.array_equal(to_np(h), to_np(h2))
    elif head == "beam":
        g = shapes["rows4"]
        want = g["want"][(ban, rules)]
        h, b = _ban(g, ban)
        with Calls() as c:
            gen, dist, cand_p, cand_id = ops.pointer_head_topk(*g["head"], W, want_gen=True, want_dist=True, ban=b, rules=_rules(g, rules), row=row)
        _routed(c, name)
        assert within(to_np(gen), g["gen64"], GEN_BAR) <= 1.0 and within(to_np(dist), want, DIST_BAR) <= 1.0
        assert np.array_equal(to_np(dist) == 0, want == 0), "exactly the restated entries are zeroed"
        top = np.stack([ordered_top(r, W) for r in want])
        assert np.array_equal(to_np(cand_id), top)
        assert within(to_np(cand_p), np.take_along_axis(want, top, axis=1), DIST_BAR) <= 1.0 and _same((cand_p,), (dist.gather(1, cand_id),))
        _appended(h, g, ban, None)  # K24 only reads the history
        h2, b2 = _ban(g, ban)
        again = ops.pointer_head_topk(*g["head"], W, want_gen=True, want_dist=True, ban=b2, rules=_rules(g, rules), row=_other(row))
        assert _same((gen, dist, cand_p, cand_id), again), "LDS and global rows differ"
    else:
        g = shapes["rows3"]
        want = g["want"][(ban, rules)]
        want_ids, want_prob = expected_draws(want)
        u = shapes["uniforms"]

        def sample(source, form):
            """-> (outputs, ended, history, calls) of one K28 call on the built row (source = g) or on the ready distribution."""
            hist, b = _ban(source, ban, sampler=True)
            ended = torch.zeros(3, dtype=torch.uint8, device="cuda")
            lead = source["head"] if "head" in source else (None, None, None, None)
            with Calls() as c:
                out = ops.pointer_head_sample(*lead, ended, False, False, EOS, UNK, PAD, *DRAW, uniforms=u, dist_in=source.get("p_dev"),
                                              want_gen="head" in source, want_dist=True, ban=b, rules=_rules(source, rules), row=form)
            return out, ended, hist, c

        (gen, dist, ids, prob), ended, h, c = sample(g, row)
        _routed(c, name)
        assert within(to_np(gen), g["gen64"], GEN_BAR) <= 1.0 and within(to_np(dist), want, DIST_BAR) <= 1.0
        assert np.array_equal(to_np(dist) == 0, want == 0), "exactly the restated entries are zeroed"
        assert to_np(ids).tolist() == want_ids and within(to_np(prob), np.asarray(want_prob), DIST_BAR) <= 1.0
        assert _same((prob,), (dist.gather(1, ids[:, None])[:, 0],)) and to_np(ended).tolist() == [int(i == EOS) for i in want_ids]
        _appended(h, g, ban, ids)
        other, ended2, h2, _ = sample(g, _other(row))
        assert _same((gen, dist, ids, prob, ended), other + (ended2,)), "LDS and global rows differ"
        # the ready distribution (V = 40: the wide form reads it in place when nothing is to be zeroed): the returned row is exact
        rd = shapes["ready"]
        ready_ids, _ = expected_draws(rd["want"][(ban, rules)])
        before = rd["p_dev"].clone()
        (gen, dist, ids, prob), ended, h, c = sample(rd, row)
        _routed(c, name)
        assert gen is None and np.array_equal(_bits(dist), rd["want"][(ban, rules)].view(np.uint32)) and _same((before,), (rd["p_dev"],))
        assert to_np(ids).tolist() == ready_ids and _same((prob,), (dist.gather(1, ids[:, None])[:, 0],))
        _appended(h, rd, ban, ids)
        other, ended2, _, _ = sample(rd, _other(row))
        assert _same((gen, dist, ids, prob, ended), other + (ended2,)), "LDS and global rows differ on a ready distribution"
