"""The decoding rules on the MI355X: min_length, banned ids and the beam length penalty, held against the restatements of
tests/test_decode_rules_cpu.py (never against the kernels themselves).

1. K23 / K24 / K28 with ``rules=``: the returned row is the rule-off row with exactly the restated entries set to 0.0, bit for bit, and the
   ids / candidates are the argmax / ordered top-W of that row -- LDS and global rows, with and without the n-gram ban.
2. K28's draw from the zeroed row: the interval property of tests/test_wide_head_gpu.py, the loop's conventions.
3. ``ops.row_rules_`` (the unfused head).
4. K25 with the length penalty against the float64 beam search.
5. Whole passes of tiny CaSE and Masque models (the geometry of tests/test_ngram_block_gpu.py).

Every test here uses ``rules=``, ``length_penalty=`` or the new keywords of the task models, none of which exist without the feature."""
import json
import math
import os

import numpy as np
import pytest
import torch

from helpers import Calls, head_inputs, record_error, special_ids, to_np
from sample_cases import draw
from test_decode_rules_cpu import BEAM_SEED, ordered_top, planted_candidates, restate_beam, restate_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U_MAX = 1.0 - 2.0 ** -24
RULE_HEADS = ("case_pointer_head_decode_rules", "case_pointer_head_beam_rules", "case_pointer_head_sample_rules",
              "case_pointer_head_decode_wide_rules", "case_pointer_head_beam_wide_rules", "case_pointer_head_sample_wide_rules")


def _measured(key, value, bar=None):
    """Add one measured maximum to profiles/decode_rules_parity.json."""
    path = os.path.join(ROOT, "profiles", "decode_rules_parity.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = {}
    if os.path.exists(path):
        with open(path) as fh:
            data = json.load(fh)
    data[key] = {"measured": float("%.3e" % value), "bar": bar}
    with open(path, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)


def _bits(a):
    return to_np(a).view(np.uint32) if a.is_floating_point() else to_np(a)


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------
# 1. the heads, bit for bit
# ---------------------------------------------------------------------------------------------
T_STEP, TMAX = 7, 12  # the step of every launch here; min_length = 8 is t = m - 1 (EOS zeroed), min_length = 7 is t = m (EOS free)


def _lens(nmem):
    return {1: (70,), 2: (30, 40), 4: (10, 15, 20, 25)}[nmem]


def _inputs(R, V, nmem):
    """Rows with a planted tie: ids TIE_LO < TIE_HI hold the two bit-equal largest entries (equal logits, no pointer mass on either), so the
    rule-off argmax is TIE_LO and zeroing it must give TIE_HI."""
    lo, hi = 5, V - 2

    def design(logits, src, mix):
        src[(src == lo) | (src == hi)] = 9
        src[:, 0] = V - 1
        src[:, 1] = 0
        mix[:, 0] = 4.0
        top = logits.max(dim=1).values
        logits[:, lo] = top + 8.0
        logits[:, hi] = top + 8.0

    logits, mix, sm, copies, src = head_inputs(R, V, _lens(nmem), 500 + V + 3 * R + nmem, design=design)
    return (logits, mix, sm, copies), lo, hi


def _history(R, V, lo, hi, seed):
    rng = np.random.RandomState(seed)
    words = np.asarray([lo, hi, 0, V - 1])
    h = words[rng.randint(0, 4, size=(R, TMAX))]
    h[0] = lo
    return h.astype(np.int32)


def _lists(R, V, K, per_item, rows_per_item, lo, base, seed):
    """A banned list [K] or [R / rows_per_item, K]: the planted maximum, every row's rule-off runner-ups, duplicates, -1 padding and ids >= V."""
    rng = np.random.RandomState(seed)
    items = R // rows_per_item if per_item else 1
    out = np.full((items, K), -1, dtype=np.int32)
    for i in range(items):
        pool = [lo, lo, V + 3, V] if (i % 2 == 0 or not per_item) else [V + 3]  # odd items keep the planted maximum
        pool += ordered_top(base[(i * rows_per_item) % R], 6)[2:].tolist()
        pool += rng.randint(0, V, size=K).tolist()
        fill = pool[:max(1, (3 * K) // 4)] if K > 1 else pool[:1]
        out[i, :len(fill)] = fill
    if per_item and items > 1:
        assert not np.array_equal(out[0], out[1]), "two neighbouring items must take different lists"
    return out if per_item else out[0]


def _check_heads(head, R, V, lo, hi, forms, combos):
    from case_rg_amd import ops
    dev = torch.device("cuda")
    _, base_t, base_ids = ops.pointer_head_decode(*head, want_gen=False, row=forms[0])
    base = to_np(base_t)
    assert to_np(base_ids).tolist() == [lo] * R and (base[:, lo] == base[:, hi]).all(), "the tie was not planted"
    hist = _history(R, V, lo, hi, V + R)
    u_np = np.random.RandomState(V).randint(0, 2 ** 24, R) * 2.0 ** -24
    u_np[0], u_np[1 % R] = 0.0, U_MAX
    u = torch.tensor(u_np, dtype=torch.float32, device=dev)
    for K, per_item, rpi in combos:
        rows = (R // rpi) * rpi  # whole items
        if rows == 0:
            continue
        sub = (head[0][:rows], head[1][:rows], head[2].select(slice(0, rows)), [c[:rows] for c in head[3]])
        lists = _lists(rows, V, K, per_item, rpi, lo, base, K + rpi)
        banned = torch.from_numpy(lists).to(dev)
        for m in (T_STEP + 1, T_STEP, 0):
            for eos in (lo, hi):
                if m == 0 and eos == hi:
                    continue
                rules = ops.row_rules(eos, m, banned, rpi, t=T_STEP)
                for n in (0, 3):
                    if n:  # the ban alone: today's `_ban` / `_wide` launch, and the same through the `_rules` entry with every rule off
                        h0 = torch.from_numpy(hist[:rows]).to(dev)
                        _, ban_t, ban_ids = ops.pointer_head_decode(*sub, want_gen=False, ban=(h0, T_STEP, n, None), row=forms[0])
                        h1 = torch.from_numpy(hist[:rows]).to(dev)
                        with Calls() as c:
                            _, d1, i1 = ops.pointer_head_decode(*sub, want_gen=False, ban=(h1, T_STEP, n, None), row=forms[0],
                                                                rules=ops.row_rules(eos, 0, None, rpi, t=T_STEP))
                        assert sum(c.count(k) for k in RULE_HEADS) == 1
                        assert _same(d1, ban_t) and _same(i1, ban_ids) and _same(h1, h0), "the ban through the `_rules` entry is not today's ban"
                        start = to_np(ban_t)
                    else:
                        start = base[:rows]
                    want = restate_rows(start, T_STEP, eos, m, lists, rpi)
                    changed = (want != start).any(axis=1)
                    assert n or changed[0], "the rules change nothing in row 0"
                    top8 = [ordered_top(r, 8).tolist() for r in want]
                    want_ids = [r[0] for r in top8]
                    outs = {}
                    for form in forms:
                        def ban():
                            return (torch.from_numpy(hist[:rows]).to(dev), T_STEP, n, None) if n else None
                        what = "V %d rows %d K %d per_item %s rpi %d m %d eos %d n %d %s" % (V, rows, K, per_item, rpi, m, eos, n, form)
                        b1 = ban()
                        with Calls() as c:
                            gen, d, ids = ops.pointer_head_decode(*sub, ban=b1, rules=rules, row=form)
                        assert c.count(RULE_HEADS[3 if form == "global" else 0]) == 1 == sum(c.count(k) for k in RULE_HEADS), c.calls
                        assert np.array_equal(_bits(d), want.view(np.uint32)), "K23 %s: not the restated row" % what
                        assert to_np(ids).tolist() == want_ids, "K23 %s: ids" % what
                        if n:
                            assert to_np(b1[0])[:, T_STEP].tolist() == want_ids, "K23 %s: the appended history" % what
                        again = ops.pointer_head_decode(*sub, ban=ban(), rules=rules, row=form)
                        assert all(_same(x, y) for x, y in zip((gen, d, ids), again)), "K23 %s: two launches differ" % what
                        got = [gen, d, ids]
                        for W in (1, 4, 8):
                            b2 = ban()
                            _, dw, cp, ci = ops.pointer_head_topk(*sub, W, want_dist=True, ban=b2, rules=rules, row=form)
                            assert np.array_equal(_bits(dw), want.view(np.uint32)), "K24 %s W %d: not the restated row" % (what, W)
                            assert to_np(ci).tolist() == [r[:W] for r in top8], "K24 %s W %d: candidates" % (what, W)
                            assert _same(cp, dw.gather(1, ci)) and (not n or np.array_equal(to_np(b2[0]), hist[:rows]))
                            got += [cp, ci]
                        ended = torch.zeros(rows, dtype=torch.uint8, device=dev)
                        b3 = None if not n else ban()[:3]
                        _, ds, si, sp = ops.pointer_head_sample(*sub, ended, False, False, -1, -1, 0, 1.0, 0, 1.0, uniforms=u[:rows], want_dist=True,
                                                                ban=b3, rules=rules, row=form)
                        assert np.array_equal(_bits(ds), want.view(np.uint32)), "K28 %s: not the restated row" % what
                        assert _same(sp, ds.gather(1, si[:, None])[:, 0]) and (to_np(sp) > 0).all(), "K28 %s: prob is not the row's own entry" % what
                        outs[form] = got + [si, sp]
                    if len(forms) == 2:
                        for a, b in zip(outs[forms[0]], outs[forms[1]]):
                            assert _same(a, b), "the LDS and the global row differ (%s)" % what
                    if m > T_STEP and not n:  # the planted tie: with the lower id zeroed (banned or EOS) the higher wins
                        zero_lo = want[:, lo] == 0
                        assert zero_lo[0] and all(want_ids[r] == hi for r in np.flatnonzero(zero_lo & (want[:, hi] != 0)))


COMBOS = [(1, False, 1), (64, True, 1), (256, True, 4), (256, False, 4), (64, True, 4)]


@pytest.mark.parametrize("nmem", [1, 2, 4])
@pytest.mark.parametrize("R", [3, 130])
@pytest.mark.parametrize("V", [150, 1031])
def test_heads_with_rules_equal_the_restated_row_bit_for_bit(V, R, nmem):
    head, lo, hi = _inputs(R, V, nmem)
    _check_heads(head, R, V, lo, hi, ("lds", "global"), COMBOS if R > 3 else COMBOS[:2] + [(64, False, 1)])


def test_heads_with_rules_beyond_the_lds_row():
    V, R = 36001, 4
    head, lo, hi = _inputs(R, V, 2)
    _check_heads(head, R, V, lo, hi, ("global",), [(1, False, 1), (256, True, 4), (64, True, 1)])


def test_a_row_zeroed_entirely_gives_id_zero():
    """Semantics 5: a row whose every entry ends up 0.0 behaves as an all-zero row: id 0, value 0 (K24: ids 0 .. W - 1 at probability 0)."""
    from case_rg_amd import ops
    V, R = 150, 3
    head, lo, hi = _inputs(R, V, 1)
    rules = ops.row_rules(-1, 0, torch.arange(V, dtype=torch.int32, device="cuda"), t=0)
    _, d, ids = ops.pointer_head_decode(*head, want_gen=False, rules=rules)
    _, _, cp, ci = ops.pointer_head_topk(*head, 4, rules=rules)
    assert not d.any() and ids.tolist() == [0] * R and not cp.any() and ci.tolist() == [[0, 1, 2, 3]] * R


# ---------------------------------------------------------------------------------------------
# 2. the sampler
# ---------------------------------------------------------------------------------------------
def _interval(p, params, u, j, tol):
    """tests/test_wide_head_gpu.py::_interval: how the kernel's id ``j`` stands against the restatement's draw from the row ``p`` (f64) with the
    uniform ``u``: "in" with the violation of  CDF(j - 1) - tol Z <= u Z <= CDF(j) + tol Z  in units of tol Z (<= 1 passes), or "cut" when j is
    not in the restatement's kept set but tied with its cut within f32 rounding."""
    d = draw(p, *params, u)
    q, Z = d["q"], d["Z"]
    assert q[j] > 0, "an entry without mass was drawn (id %d)" % j
    if not d["kept"][j]:
        assert q[j] >= d["cut"] * (1 - 2e-6) or (j == d["next"] and d["slack"] <= tol), \
            "id %d (q %.9g) is outside the kept set (cut %.9g, slack %.3g) for %s" % (j, q[j], d["cut"], d["slack"], params)
        return "cut", 0.0
    lo, hi, thr = d["cdf"][j] - q[j], d["cdf"][j], u * Z
    return "in", max(lo - thr, thr - hi, 0.0) / (tol * Z)


@pytest.mark.parametrize("form", ["lds", "global"])
def test_sampler_draws_from_the_zeroed_row(form):
    """The drawn id is never banned and never EOS while t < m, ``prob`` is the row's own entry, and the draw lies inside the restated CDF interval
    of the ZEROED row (tolerance 4 (ceil(V / 1024) + 16) 2^-24 Z, as in tests/test_wide_head_gpu.py); an ended row still returns PAD with
    probability 1 and the forced EOS of the last step still happens.  Filters off, and temperature + top-k + top-p."""
    from case_rg_amd import ops
    V, R, rpi = 1031, 8, 4
    EOS, UNK, PAD = 5, 3, 0  # EOS = the planted maximum of every row
    head, lo, hi = _inputs(R, V, 2)
    logits = head[0].clone()
    logits[:, [lo, hi]] -= 7.0  # (a flatter row: the draw has a choice)
    head = (logits,) + head[1:]
    _, base_t, _ = ops.pointer_head_decode(*head, want_gen=False)
    base = to_np(base_t)
    lists = np.stack([np.concatenate([ordered_top(base[i * rpi], 12)[2:10], [-1, V + 1, hi, hi]]) for i in range(R // rpi)]).astype(np.int32)
    lists[1, -2:] = -1  # item 1 keeps the planted runner-up
    banned = torch.from_numpy(lists).cuda()
    tol = 4 * (math.ceil(V / 1024) + 16) * 2.0 ** -24
    rs = np.random.RandomState(7)
    usets = [np.linspace(0.0, U_MAX, R), rs.randint(0, 2 ** 24, R) * 2.0 ** -24, rs.randint(0, 2 ** 24, R) * 2.0 ** -24]
    worst, cuts, count = 0.0, 0, 0
    for m in (T_STEP + 1, T_STEP):
        rules = ops.row_rules(EOS, m, banned, rpi, t=T_STEP)
        want = restate_rows(base, T_STEP, EOS, m, lists, rpi)
        for params in [(1.0, 0, 1.0), (0.7, 5, 0.9)]:
            for us in usets:
                u = torch.tensor(us, dtype=torch.float32, device="cuda")
                ended = torch.zeros(R, dtype=torch.uint8, device="cuda")
                with Calls() as c:
                    _, dist, ids, prob = ops.pointer_head_sample(*head, ended, False, False, EOS, UNK, PAD, *params, uniforms=u, want_dist=True,
                                                                 rules=rules, row=form)
                    _, dist2, ids2, prob2 = ops.pointer_head_sample(None, None, None, None, torch.zeros_like(ended), False, False, EOS, UNK, PAD,
                                                                    *params, uniforms=u, dist_in=base_t, want_dist=True, rules=rules, row=form)
                assert c.count(RULE_HEADS[5 if form == "global" else 2]) == 2 == sum(c.count(k) for k in RULE_HEADS), c.calls
                assert np.array_equal(_bits(dist), want.view(np.uint32)) and _same(dist, dist2) and _same(ids, ids2) and _same(prob, prob2)
                assert _same(prob, dist.gather(1, ids[:, None])[:, 0]), "prob is not the row's own entry"
                for r in range(R):
                    j = int(ids[r])
                    assert want[r, j] > 0 and j not in lists[r // rpi].tolist() and (j != EOS or m <= T_STEP), "row %d drew a zeroed id %d" % (r, j)
                    kind, viol = _interval(want[r].astype(np.float64), params, float(us[r]), j, tol)
                    cuts += kind == "cut"
                    count += 1
                    worst = max(worst, viol)
                    assert viol <= 1.0, "row %d %s u %.9g: id %d misses its interval by %.3g tol" % (r, params, us[r], j, viol)
                assert to_np(ended).tolist() == [int(int(i) == EOS) for i in ids]
    assert cuts * 10 <= count, "too many draws fell on a cut tie to call the kept set checked"
    _measured("k28_rules/%s/interval_violation_in_tol" % form, worst, 1.0)
    # an ended row is left alone and keeps emitting PAD with probability 1; the last step still forces EOS on the others
    rules = ops.row_rules(EOS, T_STEP + 1, banned, rpi, t=T_STEP)
    want = restate_rows(base, T_STEP, EOS, T_STEP + 1, lists, rpi)
    want[2] = base[2]
    u = torch.full((R,), 0.5, device="cuda")
    for last in (False, True):
        ended = torch.tensor([0, 0, 1] + [0] * (R - 3), dtype=torch.uint8, device="cuda")
        _, dist, ids, prob = ops.pointer_head_sample(*head, ended, False, last, EOS, UNK, PAD, 1.0, 0, 1.0, uniforms=u, want_dist=True, rules=rules,
                                                     row=form)
        assert np.array_equal(_bits(dist), want.view(np.uint32)), "an ended row must be left alone"
        assert int(ids[2]) == PAD and float(prob[2]) == 1.0 and int(ended[2]) == 1
        if last:
            assert ids.tolist() == [EOS, EOS, PAD] + [EOS] * (R - 3), "the forced EOS of the last step"


# ---------------------------------------------------------------------------------------------
# 3. the unfused op
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [203, 2051])
def test_row_rules_on_random_rows(V):
    from case_rg_amd import ops
    R, rpi, K, eos = 12, 3, 64, 17
    g = torch.Generator().manual_seed(V)
    dist = torch.rand(R, V, generator=g)
    dist[5] = 0.0
    dist[5, [3, 40, V - 1]] = torch.tensor([0.5, 0.25, 0.25])  # item 1 (rows 3 .. 5): its list removes every non-zero entry of row 5
    rng = np.random.RandomState(V)
    lists = rng.randint(-1, V + 5, size=(R // rpi, K)).astype(np.int32)
    lists[lists == eos] = -1
    lists[1, :3] = [3, 40, V - 1]
    for banned_np, per in ((lists, rpi), (lists[0], 1), (None, 1)):
        banned = None if banned_np is None else torch.from_numpy(np.ascontiguousarray(banned_np)).cuda()
        for t, m in ((0, 1), (4, 5), (5, 5), (300, 0), (300, 301)):
            got = dist.clone().cuda()
            with Calls() as c:
                out = ops.row_rules_(got, ops.row_rules(eos, m, banned, per, t=t))
            assert out is got and c.count("case_row_rules") == 1
            want = restate_rows(dist.numpy(), t, eos, m, banned_np, per)
            assert np.array_equal(_bits(got), want.view(np.uint32)), "t %d m %d" % (t, m)
            if banned_np is lists:
                assert not got[5].any() and int(ops.row_argmax(got)[0][5]) == 0
    ended = torch.tensor([0, 1] * (R // 2), dtype=torch.uint8, device="cuda")
    got = ops.row_rules_(dist.clone().cuda(), ops.row_rules(eos, 1, torch.from_numpy(lists).cuda(), rpi), ended)
    want = restate_rows(dist.numpy(), 0, eos, 1, lists, rpi)
    want[1::2] = dist.numpy()[1::2]
    assert np.array_equal(_bits(got), want.view(np.uint32)), "rows with ended set must be left alone"
    with pytest.raises(ValueError, match="rows_per_item"):
        ops.row_rules_(dist.clone().cuda(), ops.row_rules(eos, 1, torch.from_numpy(lists).cuda(), 5))


# ---------------------------------------------------------------------------------------------
# 4. K25 with the length penalty
# ---------------------------------------------------------------------------------------------
KEY_BAR = 2e-6  # ten times the worst relative key error measured (1.995e-07, profiles/decode_rules_parity.json); never looser than 1e-5


def _run_beam(p, ids, B, W, T, eos, **kw):
    from case_rg_amd import ops
    state = ops.BeamState(B, W, T, torch.device("cuda"), flat=True)
    for t in range(T):
        ops.beam_advance(state, torch.from_numpy(p[t]).cuda(), torch.from_numpy(ids[t]).cuda(), t, eos, **kw)
    return state


STATE = ("alive", "cum", "len", "parent", "token", "hist_parent", "hist_token", "fin_key", "fin_step", "fin_slot", "flat")


def test_beam_advance_with_a_length_penalty_matches_the_float64_search():
    """B = 3, W = 4, T = 6 on planted candidates whose keys lie >= 1e-4 apart at every alpha (asserted in the CPU file): the finished pool's order,
    steps and slots and the back-tracked answers equal the restatement exactly; the keys agree within f32 rounding (the worst relative
    difference, measured 1.995e-07, is recorded; the bar is ten times that, 2e-6, which is tighter than the 1e-5 cap).  alpha = 1.0 leaves every state tensor bit-equal to the
    ``case_beam_advance_ban`` path, through the Python default, the keyword and the C entry itself."""
    from case_rg_amd import _abi as A
    from case_rg_amd import ops
    B, W, T, eos = 3, 4, 6, 2
    p, ids = planted_candidates(B, W, T, eos, seed=BEAM_SEED)
    worst = 0.0
    for alpha in (0.0, 0.6, 1.0, 2.0):
        want = restate_beam(p, ids, B, W, T, eos, alpha)
        with Calls() as c:
            state = _run_beam(p, ids, B, W, T, eos, length_penalty=alpha)
        assert c.count("case_beam_advance_rules") == (T if alpha != 1.0 else 0) and c.count("case_beam_advance_ban") == (T if alpha == 1.0 else 0)
        answer, beam_answers, beam_scores = ops.beam_backtrack(state)
        for b in range(B):
            n = len(want[b]["keys"])
            assert n == W
            assert to_np(state.fin_step)[b].tolist() == want[b]["steps"] and to_np(state.fin_slot)[b].tolist() == want[b]["slots"], (alpha, b)
            assert to_np(beam_answers)[b].tolist() == want[b]["answers"], "alpha %s item %d" % (alpha, b)
            got, ref = to_np(beam_scores)[b].astype(np.float64), np.asarray(want[b]["keys"])
            assert _same(beam_scores, state.fin_key)
            worst = max(worst, float((np.abs(got - ref) / np.abs(ref)).max()))
        assert torch.equal(answer, beam_answers[:, 0])
    print("K25 with alpha: worst relative key error %.3e" % worst)
    record_error("beam_length_penalty", "fp32", "key_rel", worst, KEY_BAR)
    _measured("k25_alpha/key_rel_vs_float64", worst, KEY_BAR)
    assert worst <= KEY_BAR
    # alpha = 1.0: today's path, bit for bit
    today = _run_beam(p, ids, B, W, T, eos)
    keyword = _run_beam(p, ids, B, W, T, eos, length_penalty=1.0)
    direct = ops.BeamState(B, W, T, torch.device("cuda"), flat=True)
    for t in range(T):
        cp, ci = torch.from_numpy(p[t]).cuda(), torch.from_numpy(ids[t]).cuda()
        s = direct
        A.call("case_beam_advance_rules", cp.data_ptr(), ci.data_ptr(), *[getattr(s, k).data_ptr() for k in STATE[:-1]], t, T, B, W, eos,
               s.flat[t % 2].data_ptr(), s.flat[(t + 1) % 2].data_ptr(), T, 1.0, None)
    for k in STATE:
        assert _same(getattr(today, k), getattr(keyword, k)) and _same(getattr(today, k), getattr(direct, k)), "%s differs at alpha = 1" % k
    with pytest.raises(RuntimeError, match="length penalty"):
        A.call("case_beam_advance_rules", *([None] * 12), 0, T, B, W, eos, None, None, T, -1.0, None)


# ---------------------------------------------------------------------------------------------
# 5. whole passes
# ---------------------------------------------------------------------------------------------
V_, H_, T_, ITEMS, M_ = 200, 32, 24, 4, 5
SEEDS = {"case": (153, 152), "masque": (153, 152)}  # (model seed, batch seed) of tests/test_ngram_block_gpu.py
BEAM_BAR, SAMPLE_BAR = 5e-6, 1.5e-5


@pytest.fixture(scope="module")
def ns():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.float32)
    case_rg_amd.set_dropout(False)
    return case_rg_amd.namespace()


def _build(ns, kind):
    from case_rg_amd.utils import fill_params, make_vocab, synth_batch
    v2i, i2v = make_vocab(V_)
    mseed, bseed = SEEDS[kind]
    model = ns.CaSE(4, T_, i2v, v2i, H_) if kind == "case" else ns.Masque(T_, i2v, v2i, H_)
    model = fill_params(model, mseed, gain=3.0).cuda().eval()
    return model, {k: v.cuda() for k, v in synth_batch(ITEMS, 3, 12, 8, 6, V_, seed=bseed, model=kind).items()}


@pytest.fixture(scope="module")
def fixtures(ns):
    """kind -> (model in eval mode, batch on the device), left unchanged."""
    return {kind: _build(ns, kind) for kind in ("case", "masque")}


class _Unfused:
    def __enter__(self):
        from case_rg_amd import ops
        self.old, ops.POINTER_HEAD = ops.POINTER_HEAD, "off"

    def __exit__(self, *exc):
        from case_rg_amd import ops
        ops.POINTER_HEAD = self.old


def _specials(m):
    from case_rg_amd.common.Constants import CLS_WORD, SEP_WORD
    bos, eos, unk, pad = special_ids(m)
    return eos, unk, pad, [unk, m.vocab2id[CLS_WORD], m.vocab2id[SEP_WORD]]


def _obeys(rows, eos, banned, what):
    rows = np.asarray(rows).reshape(-1, T_)
    assert not (rows[:, :M_] == eos).any(), "%s: EOS among the first %d tokens: %s" % (what, M_, rows[:, :M_ + 1].tolist())
    assert not np.isin(rows, banned).any(), "%s: a banned id was emitted" % what


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["case", "masque"])
def test_greedy_and_sampled_passes_obey_the_rules(ns, kind, dtype):
    import case_rg_amd
    case_rg_amd.set_compute_dtype(dtype)
    try:
        m, b = _build(ns, kind)
        dec = m.response_generation.decoder
        eos, unk, pad, banned = _specials(m)
        with torch.no_grad(), Calls() as c:
            greedy = m.do_test(dict(b), min_length=M_, banned_ids=banned)
            steps = dec.last_greedy_steps
            drawn = m.do_sample(dict(b), num_samples=4, seed=11, min_length=M_, banned_ids=banned)
        assert c.count("case_pointer_head_decode_rules") == steps == T_ and c.count("case_pointer_head_sample_rules") == dec.last_sample_steps >= M_
        _obeys(to_np(greedy["answer"]), eos, banned, "greedy")
        _obeys(to_np(drawn["samples"]), eos, banned, "sampled")
        assert drawn["samples"].shape == (ITEMS, 4, T_)
    finally:
        case_rg_amd.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_greedy_pass_with_rules_equals_the_unfused_pass(fixtures, kind):
    """The answers are the ``CASE_POINTER_HEAD=off`` pass's (``row_rules_`` on the unfused distribution) item by item up to the first position
    where the unfused row's two largest entries are within 1e-5 of each other (relative) -- the decisiveness rule of
    tests/test_wide_head_gpu.py; at most 10 % of the (item, position) pairs may be left out."""
    from case_rg_amd import ops
    m, b = fixtures[kind]
    eos, unk, pad, banned = _specials(m)
    with torch.no_grad():
        fused = to_np(m.do_test(dict(b), min_length=M_, banned_ids=banned)["answer"])
    gaps, real = [], ops.row_argmax

    def recording(x, *a, **kw):
        if tuple(x.shape) == (ITEMS, V_):
            top = torch.topk(x.float(), 2, dim=-1).values
            gaps.append(to_np((top[:, 0] - top[:, 1]) / top[:, 0]))
        return real(x, *a, **kw)

    ops.row_argmax = recording
    try:
        with torch.no_grad(), _Unfused(), Calls() as c:
            plain = to_np(m.do_test(dict(b), min_length=M_, banned_ids=banned)["answer"])
    finally:
        ops.row_argmax = real
    assert c.count("case_row_rules") == T_ == len(gaps) and sum(c.count(k) for k in RULE_HEADS) == 0, c.calls
    _obeys(plain, eos, banned, "unfused greedy")
    gaps = np.stack(gaps, axis=1)
    compared = 0
    for i in range(ITEMS):
        close = np.flatnonzero(gaps[i] < 1e-5)
        n = int(close[0]) if close.size else T_
        compared += n
        assert np.array_equal(fused[i, :n], plain[i, :n]), "%s item %d: fused %s, unfused %s (decisive for %d steps)" % (kind, i, fused[i], plain[i], n)
    share = compared / (ITEMS * T_)
    _measured("%s/greedy_compared_share" % kind, share, 0.9)
    assert share >= 0.9, "only %.0f %% of the (item, position) pairs were decisive" % (100 * share)


def _beam_keys(token_probs, answers, eos, alpha):
    """sum_t -log(p_t + 1e-10) / (n + 1)^alpha over the n tokens up to and including EOS (tests/test_score_gpu.py::_beam_costs with the exponent)."""
    B, W, T = answers.shape
    key, usable = np.zeros((B, W)), np.zeros((B, W), dtype=bool)
    for b in range(B):
        for w in range(W):
            ids = answers[b, w].tolist()
            n = ids.index(eos) + 1 if eos in ids else T
            usable[b, w] = 0 not in ids[:n]
            key[b, w] = sum(-math.log(token_probs[b, w, t] + 1e-10) for t in range(n)) / float(n + 1) ** alpha
    return key, usable


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_beam_pass_with_rules_and_length_penalty(fixtures, kind):
    m, b = fixtures[kind]
    dec = m.response_generation.decoder
    eos, unk, pad, banned = _specials(m)
    for alpha in (1.0, 0.6):
        with torch.no_grad(), Calls() as c:
            beam = m.do_beam(dict(b), width=4, min_length=M_, banned_ids=banned, length_penalty=alpha)
            steps = dec.last_beam_steps
            rescored = m.do_score(dict(b), beam["beam_answers"])
        assert c.count("case_pointer_head_beam_rules") == steps >= M_, c.calls
        assert c.count("case_beam_advance_rules" if alpha != 1.0 else "case_beam_advance_ban") == steps and c.count("case_beam_advance") == 0
        scores = to_np(beam["beam_scores"]).astype(np.float64)
        answers = to_np(beam["beam_answers"])
        fin = np.isfinite(scores)
        assert fin[:, 0].all() and torch.equal(beam["answer"], beam["beam_answers"][:, 0]) and _same(beam["beam_score"], beam["beam_scores"][:, 0])
        _obeys(answers[fin], eos, banned, "beam alpha %s" % alpha)
        # beam_scores x (len + 1)^alpha is the cost do_score's per-token probabilities give
        key, usable = _beam_keys(to_np(rescored["token_probs"]).astype(np.float64), answers, eos, alpha)
        ok = fin & usable
        assert ok.sum() >= ITEMS, "too few finished hypotheses to compare"
        rel = float((np.abs(key - scores)[ok] / np.abs(scores)[ok]).max())
        print("%s alpha %s: beam keys vs rescoring over %d hypotheses: %.3e" % (kind, alpha, ok.sum(), rel))
        record_error("decode_rules_%s" % kind, "fp32", "rescored_beam_scores_alpha_%s" % alpha, rel, BEAM_BAR)
        _measured("%s/rescored_beam_scores_alpha_%s" % (kind, alpha), rel, BEAM_BAR)
        assert rel <= BEAM_BAR


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_length_penalty_decides_between_short_and_long_on_planted_steps(fixtures, kind):
    """alpha = 0 against alpha = 2 through ``do_beam``, on planted items: the step's head is replaced by candidates that offer a continuation at
    0.6 and EOS at 0.3 in every row (EOS at 0.0 while t < min_length, as the rule leaves it), so hypotheses of every length from min_length on
    retire; the decoder's own loop, ``min_length`` and K25 with the exponent then have to reproduce the float64 search: alpha = 0 ranks the
    shortest hypothesis first, alpha = 2 the longest."""
    from case_rg_amd import ops
    m, b = fixtures[kind]
    eos, unk, pad, banned = _specials(m)
    W, steps_seen = 4, []

    def planted_row(t, item):
        # (every probability depends on the step, so no two hypotheses add up the same costs in another order)
        return [0.6 - 0.003 * t, 0.3 + 0.002 * t if t >= M_ else 0.0, 0.05 - 0.001 * item + 0.0007 * t, 0.04 - 0.0005 * t], [110 + t, eos, 120 + item, 150 + t]

    def planted_head(logits, mix_logits, source_map, copies, width, ban=None, rules=None, **kw):
        assert width == W and rules is not None and rules.min_length == M_ and rules.rows_per_item == W and ban is None
        steps_seen.append(rules.t)
        rows = [planted_row(rules.t, r // W) for r in range(logits.shape[0])]
        return (None, None, torch.tensor([p for p, _ in rows], dtype=torch.float32, device=logits.device),
                torch.tensor([i for _, i in rows], dtype=torch.int64, device=logits.device))

    cand = [[planted_row(t, r // W) for r in range(ITEMS * W)] for t in range(T_)]
    p_np = np.asarray([[p for p, _ in step] for step in cand], dtype=np.float32)
    id_np = np.asarray([[i for _, i in step] for step in cand], dtype=np.int64)
    real, best = ops.pointer_head_topk, {}
    ops.pointer_head_topk = planted_head
    try:
        for alpha in (0.0, 2.0):
            del steps_seen[:]
            with torch.no_grad(), Calls() as c:
                beam = m.do_beam(dict(b), width=W, min_length=M_, length_penalty=alpha)
            assert steps_seen == list(range(T_)) and c.count("case_beam_advance_rules") == T_
            want = restate_beam(p_np, id_np, ITEMS, W, T_, eos, alpha)
            assert min(i["gaps"] for i in want) >= 2e-5, "the planted keys are not decisive (a hundred times the f32 key error)"
            got = to_np(beam["beam_answers"])
            for i in range(ITEMS):
                assert got[i].tolist() == want[i]["answers"], "alpha %s item %d" % (alpha, i)
                ref = np.asarray(want[i]["keys"])
                assert float((np.abs(to_np(beam["beam_scores"])[i] - ref) / ref).max()) <= KEY_BAR
            best[alpha] = got[:, 0]
    finally:
        ops.pointer_head_topk = real
    short, long_ = (best[0.0] != 0).sum(axis=1), (best[2.0] != 0).sum(axis=1)
    assert (short == M_ + 1).all() and (long_ == T_).all(), "alpha = 0 must rank the shortest hypothesis first and alpha = 2 the longest: %s %s" % (short, long_)
    assert not np.array_equal(best[0.0], best[2.0])


def _drawn_positions(samples, unk, pad):
    """Where ``sample_probs`` is the probability of the EMITTED token (tests/test_score_gpu.py)."""
    keep = samples != pad
    keep[..., -1] = False
    keep[..., 0] &= samples[..., 0] != unk
    return keep


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_sampled_pass_with_rules_is_rescored(fixtures, kind):
    m, b = fixtures[kind]
    eos, unk, pad, banned = _specials(m)
    with torch.no_grad():
        drawn = m.do_sample(dict(b), num_samples=4, seed=5, min_length=M_, banned_ids=banned)
        again = m.do_score(dict(b), drawn["samples"])
    samples = to_np(drawn["samples"])
    _obeys(samples, eos, banned, "sampled")
    want, got = to_np(drawn["sample_probs"]).astype(np.float64), to_np(again["token_probs"]).astype(np.float64)
    keep = _drawn_positions(samples, unk, pad)
    assert keep.sum() >= samples.size // 4, "too few comparable positions: %d" % keep.sum()
    err = float(np.abs(got - want)[keep].max())
    print("%s: sampled pass with rules vs rescoring over %d positions: %.3e" % (kind, keep.sum(), err))
    record_error("decode_rules_%s" % kind, "fp32", "rescored_sample_probs_abs", err, SAMPLE_BAR)
    _measured("%s/rescored_sample_probs_abs" % kind, err, SAMPLE_BAR)
    assert err <= SAMPLE_BAR


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_consensus_and_per_item_lists(fixtures, kind):
    m, b = fixtures[kind]
    eos, unk, pad, banned = _specials(m)
    with torch.no_grad(), Calls() as c:
        out = m.do_consensus(dict(b), pool="sample", min_length=M_, num_samples=4, seed=9)
    assert c.count("case_pointer_head_sample_rules") >= M_
    pick = to_np(out["answer"])
    assert pick.shape == (ITEMS, T_) and not (pick[:, :M_] == eos).any(), "the consensus pick ends before min_length"
    assert not (to_np(out["samples"])[:, :, :M_] == eos).any()
    with torch.no_grad():
        beam_pool = m.do_consensus(dict(b), pool="beam", width=3, min_length=M_, length_penalty=0.6)
    assert not (to_np(beam_pool["answer"])[:, :M_] == eos).any() and beam_pool["beam_answers"].shape == (ITEMS, 3, T_)
    # one list per item: item 0 loses its own greedy first token, the other items (empty lists) keep their answers bit for bit
    with torch.no_grad():
        plain = to_np(m.do_test(dict(b))["answer"])
        first = int(plain[0, 0])
        assert first != eos
        lists = torch.full((ITEMS, 2), -1, dtype=torch.int64)
        lists[0, 1] = first
        ruled = to_np(m.do_test(dict(b), banned_ids=lists)["answer"])
        beams = to_np(m.do_beam(dict(b), width=2, banned_ids=lists)["beam_answers"])
    assert first not in ruled[0].tolist() and ruled[0, 0] != plain[0, 0], "item 0 emitted its banned id"
    assert np.array_equal(ruled[1:], plain[1:]), "an item with an empty list must keep its answer"
    assert first not in beams[0].reshape(-1).tolist(), "a beam slot of item 0 took its neighbour's list"


def _capture(fn):
    """Warm up on a side stream, capture ``fn`` into one graph, replay twice -> the static outputs."""
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph, static = torch.cuda.CUDAGraph(), {}
    with torch.cuda.graph(graph):
        static.update(fn())
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    return graph, static


def test_captured_passes_with_rules_replay_to_the_eager_passes(fixtures):
    """A greedy and a sampled pass with rules on capture into one hipGraph each (the list as a device tensor: a host list would need a
    host-to-device copy inside the capture) and the replay equals the eager pass."""
    m, b = fixtures["case"]
    eos, unk, pad, banned = _specials(m)
    dev_list = torch.tensor(banned, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        eager = m.do_test(dict(b), min_length=M_, banned_ids=dev_list)["answer"].clone()
        graph, static = _capture(lambda: m.do_test(dict(b), min_length=M_, banned_ids=dev_list))
        assert torch.equal(static["answer"], eager), "hipGraph replay of the greedy pass with rules differs from the eager pass"
        del graph
        keys = ("samples", "sample_probs", "sample_scores")
        sampled = {k: v.clone() for k, v in m.do_sample(dict(b), num_samples=2, seed=5, min_length=M_, banned_ids=dev_list).items()}
        graph, static = _capture(lambda: m.do_sample(dict(b), num_samples=2, seed=5, min_length=M_, banned_ids=dev_list))
        for k in keys:
            assert torch.equal(static[k], sampled[k]), "a replay must repeat the eager pass's %s" % k
        del graph
    _obeys(to_np(eager), eos, banned, "captured greedy")


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_defaults_are_the_calls_without_the_keywords(fixtures, kind):
    """With the new attributes at their defaults, do_test / do_beam / do_sample return the tensors of the same calls with the keywords spelled
    out as 0 / None / 1.0 -- and make the same launches, none of them a `_rules` one."""
    m, b = fixtures[kind]
    assert (m.min_length, m.banned_ids, m.length_penalty) == (0, None, 1.0)
    with torch.no_grad():
        with Calls() as c0:
            default = (m.do_test(dict(b)), m.do_beam(dict(b)), m.do_sample(dict(b), seed=7))
        with Calls() as c1:
            explicit = (m.do_test(dict(b), min_length=0, banned_ids=None), m.do_beam(dict(b), min_length=0, banned_ids=None, length_penalty=1.0),
                        m.do_sample(dict(b), seed=7, min_length=0, banned_ids=None))
    assert c0.calls == c1.calls, "the spelled-out defaults change the launches"
    assert not any(name.endswith("_rules") for name in c1.calls) and c1.count("case_beam_advance") >= 1
    for d, e in zip(default, explicit):
        assert set(d) == set(e)
        for k in d:
            assert torch.equal(d[k], e[k]), k
