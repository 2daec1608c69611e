"""The wide (global-row) forms of K23 / K24 / K28 on the MI355X: the vocabulary row of a workgroup in a device-memory workspace instead of LDS.

1. At every V the LDS forms accept, ``row="global"`` returns the bits of ``row="lds"`` in every output -- which carries everything pinned
   for K23 / K24 / K28 / K32 over to the wide forms.
2. Beyond 36 000 ids: against a float64 NumPy restatement of the row (the docstring of K23), at the bars tests/test_pointer_decode_gpu.py
   uses against the separate launches, with planted winners so that every id comparison is decisive; ties, determinism, the ban.
3. Sampling beyond 36 000 ids: the interval property of tests/test_sample_gpu.py, restated here; the loop conventions.
4. Whole passes of tiny CaSE and Masque models with 36 100 words, and unchanged launches at 30 522."""
import json
import math
import os

import numpy as np
import pytest
import torch

from helpers import Calls, head_inputs, record_error, special_ids, to_np
from sample_cases import draw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U_MAX = 1.0 - 2.0 ** -24
WIDE = ("case_pointer_head_decode_wide", "case_pointer_head_beam_wide", "case_pointer_head_sample_wide")
LDS = ("case_pointer_head_decode", "case_pointer_head_beam", "case_pointer_head_sample", "case_pointer_head_decode_ban",
       "case_pointer_head_beam_ban", "case_pointer_head_sample_ban")


def _measured(key, value, bar=None):
    """Add one measured maximum to profiles/wide_head_parity.json."""
    path = os.path.join(ROOT, "profiles", "wide_head_parity.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = {}
    if os.path.exists(path):
        with open(path) as fh:
            data = json.load(fh)
    data[key] = {"measured": float("%.3e" % value), "bar": bar}
    with open(path, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)


def _same(a, b):
    """torch.equal, and for floats on the bit patterns (so that -0.0 and 0.0 differ)."""
    if a is None or b is None:
        return a is None and b is None
    if a.is_floating_point():
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def _ban(history, n, V, eos):
    from case_rg_amd.common.Utils import banned_tokens
    return banned_tokens(history, n, V, eos)


# ---------------------------------------------------------------------------------------------
# 1. bit equality with the LDS forms
# ---------------------------------------------------------------------------------------------
T_BAN, TMAX = 7, 12


def _lens(nmem, S):
    """S = 1: one position per memory (a source map of a single key at nmem = 1; every memory needs a position).  S = 1100 split over the memories."""
    if S == 1:
        return (1,) * nmem
    return {1: (1100,), 2: (100, 1000), 4: (100, 200, 300, 500)}[nmem]


def _small_inputs(R, V, nmem, S):
    lens = _lens(nmem, S)
    total = sum(lens)
    run_tok = (2 * V) // 3

    def design(logits, src, mix):
        if total < 1100:
            src[:, 0] = torch.tensor([0, V - 1, run_tok] * R)[:R]  # ids 0 and V - 1 among the single keys
            return
        g = torch.Generator().manual_seed(V + R)
        for r in range(R):  # 980 keys sort below the run, so the 90 equal tokens lie at the sorted indices 980 .. 1069: across the 1024-key chunk
            low = torch.randint(0, run_tok, (980,), generator=g)
            low[0] = 0
            high = torch.randint(run_tok + 1, V, (total - 980 - 90,), generator=g)
            high[0] = V - 1
            row = torch.cat([low, torch.full((90,), run_tok), high])
            src[r] = row[torch.randperm(total, generator=g)]  # (the run's positions spread over the memories)

    logits, mix, sm, copies, src = head_inputs(R, V, lens, 1000 + V + 7 * R + nmem, design=design)
    if total >= 1100:
        keys = (to_np(sm.keys).astype(np.int64) & 0xFFFFFFFF) >> 15
        assert (keys[:, 980:1070] == run_tok).all() and (keys[:, 979] != run_tok).all(), "the run does not cross the 1024-key chunk"
        assert (keys[:, 0] == 0).all() and (keys[:, -1] == V - 1).all()
    return logits, mix, sm, copies, run_tok


def _history(R, V, run_tok, seed):
    """int32 [R, TMAX]: T_BAN tokens over four words the rows can emit (the run's token, ids 0 and V - 1 among them), many matching windows."""
    rng = np.random.RandomState(seed)
    words = np.asarray([run_tok, 0, V - 1, min(5, V - 1)])
    h = words[rng.randint(0, 4, size=(R, TMAX))]
    h[0] = run_tok
    h[1 % R] = words[np.arange(TMAX) % 2]
    return h.astype(np.int32)


@pytest.mark.parametrize("S", [1, 1100])
@pytest.mark.parametrize("nmem", [1, 2, 4])
@pytest.mark.parametrize("R", [3, 130])
@pytest.mark.parametrize("V", [150, 1031, 30522, 36000])
def test_global_row_equals_lds_row_bit_for_bit(V, R, nmem, S):
    from case_rg_amd import ops
    logits, mix, sm, copies, run_tok = _small_inputs(R, V, nmem, S)
    head = (logits, mix, sm, copies)
    hist = _history(R, V, run_tok, V + R)
    # K23: no ban, n = 1 and n = 3 at t = 7, the appended history column included
    base = None
    for n in (0, 1, 3):
        outs = []
        for form in ("lds", "global"):
            h = torch.from_numpy(hist).cuda()
            with Calls() as c:
                gen, dist, ids = ops.pointer_head_decode(*head, ban=(h, T_BAN, n, None) if n else None, row=form)
            assert c.count(WIDE[0]) == (form == "global") and sum(c.count(k) for k in LDS) == (form == "lds"), c.calls
            outs.append((gen, dist, ids, h))
        for name, a, b in zip(("gen", "dist", "ids", "hist"), *outs):
            assert _same(a, b), "K23 n %d: %s differs between the LDS and the global row" % (n, name)
        if n == 0:
            base = outs[0]
        else:
            assert torch.equal(outs[1][3][:, T_BAN], outs[1][2].int()) and not _same(outs[1][1], base[1]), "the ban did not change the row"
    # K24
    for W in (1, 4, 8):
        for n in (0, 3):
            outs = []
            for form in ("lds", "global"):
                h = torch.from_numpy(hist).cuda()
                with Calls() as c:
                    outs.append(ops.pointer_head_topk(*head, W, want_gen=True, want_dist=True, ban=(h, T_BAN, n, None) if n else None, row=form))
                assert c.count(WIDE[1]) == (form == "global") and sum(c.count(k) for k in LDS) == (form == "lds"), c.calls
            for name, a, b in zip(("gen", "dist", "cand_p", "cand_id"), *outs):
                assert _same(a, b), "K24 W %d n %d: %s differs" % (W, n, name)
    # K28: explicit uniforms with 0 and 1 - 2^-24
    rs = np.random.RandomState(V + R + nmem)
    us = rs.randint(0, 2 ** 24, R) * 2.0 ** -24
    us[0], us[1] = 0.0, U_MAX
    u = torch.tensor(us, dtype=torch.float32, device="cuda")
    eos, unk, pad = run_tok, 3, 0
    none_ended, one_ended = [0] * R, [0, 0, 1] + [0] * (R - 3)
    settings = [("off", (1.0, 0, 1.0), False, False, none_ended, 0), ("top_k", (1.0, 5, 1.0), False, False, none_ended, 0),
                ("top_p", (1.0, 0, 0.9), False, False, none_ended, 0), ("temperature", (0.7, 0, 1.0), False, False, none_ended, 0),
                ("t_first", (1.0, 0, 1.0), True, False, none_ended, 0), ("t_last", (1.0, 0, 1.0), False, True, one_ended, 0),
                ("ended", (0.7, 5, 0.9), False, False, one_ended, 0), ("ban", (1.0, 0, 1.0), False, False, one_ended, 3)]
    for source in ("fused", "dist_in"):
        for what, params, first, last, ended, n in settings:
            outs = []
            for form in ("lds", "global"):
                e = torch.tensor(ended, dtype=torch.uint8, device="cuda")
                h = torch.from_numpy(hist).cuda()
                kw = dict(uniforms=u, want_dist=True, ban=(h, T_BAN, n) if n else None, row=form)
                with Calls() as c:
                    if source == "fused":
                        gen, dist, ids, prob = ops.pointer_head_sample(*head, e, first, last, eos, unk, pad, *params, want_gen=True, **kw)
                    else:
                        gen, dist, ids, prob = ops.pointer_head_sample(None, None, None, None, e, first, last, eos, unk, pad, *params,
                                                                       dist_in=base[1], **kw)
                assert c.count(WIDE[2]) == (form == "global") and sum(c.count(k) for k in LDS) == (form == "lds"), c.calls
                outs.append((gen, dist, ids, prob, e, h))
            for name, a, b in zip(("gen", "dist", "ids", "prob", "ended", "hist"), *outs):
                assert _same(a, b), "K28 %s %s: %s differs between the LDS and the global row" % (source, what, name)
            if not n:
                assert _same(outs[1][1], base[1]), "K28 %s %s: the row is not K23's" % (source, what)


# ---------------------------------------------------------------------------------------------
# 2. beyond the LDS row: the float64 restatement
# ---------------------------------------------------------------------------------------------
WIDE_LENS, W_MAX = (40, 60), 8


def _planted(V, R):
    """id [R, 8]: the planted winners of every row, the first the argmax: ids 35 999, 36 000 and V - 1 among the winners, distinct in a row."""
    rng = np.random.RandomState(V + R)
    first = [V - 1, 36000, 35999, 17, V // 2]
    out = np.zeros((R, W_MAX), dtype=np.int64)
    for r in range(R):
        rest = [x for x in rng.permutation(V)[:W_MAX + 3].tolist() if x != first[r]][:W_MAX - 1]
        out[r] = [first[r]] + rest
    return out


def _wide_inputs(V, R):
    win = _planted(V, R)

    def design(logits, src, mix):
        src[:, :6] = torch.tensor([35999, 36000, V - 1, 35999, V - 1, 36000])  # pointer mass on both sides of the LDS bound and on the last id
        mix[:, 0] = 3.0  # (the generator's share outweighs any pointer mass: the planted order decides)
        top = logits.max(dim=1).values
        for r in range(R):
            for j in range(W_MAX):
                logits[r, win[r, j]] = top[r] + 5.0 - 0.5 * j

    logits, mix, sm, copies, src = head_inputs(R, V, WIDE_LENS, 77 + V + R, design=design)
    return logits, mix, sm, copies, src, win


def _restate(logits, mix, src, copies, V):
    """The docstring of K23 in float64: gen = softmax(logits); pm = softmax(mix); dist = pm_0 gen + the pointer mass scattered over the source."""
    x = to_np(logits).astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    gen = e / e.sum(axis=1, keepdims=True)
    m = to_np(mix).astype(np.float64)
    pm = np.exp(m - m.max(axis=1, keepdims=True))
    pm /= pm.sum(axis=1, keepdims=True)
    w = np.concatenate([pm[:, k + 1:k + 2] * to_np(c).astype(np.float64) for k, c in enumerate(copies)], axis=1)
    ptr = np.zeros_like(gen)
    ids = src.numpy()
    for r in range(ptr.shape[0]):
        ok = ids[r] < V
        np.add.at(ptr[r], ids[r][ok], w[r][ok])
    return gen, pm[:, :1] * gen + ptr, ptr


def _order(row, W):
    return np.lexsort((np.arange(row.size), -row))[:W]


def _within(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|): <= 1 is torch.allclose(got, want, rtol, atol)."""
    got = np.asarray(got, dtype=np.float64)
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())


@pytest.mark.parametrize("R", [2, 5])
@pytest.mark.parametrize("V", [36001, 50265, 131071])
def test_wide_heads_match_the_float64_restatement(V, R):
    from case_rg_amd import ops
    logits, mix, sm, copies, src, win = _wide_inputs(V, R)
    head = (logits, mix, sm, copies)
    gen64, dist64, ptr64 = _restate(logits, mix, src, copies, V)
    for r in range(R):  # every comparison is decisive, in every row
        top = dist64[r][_order(dist64[r], W_MAX + 1)]
        assert ((top[:-1] - top[1:]) > 1e-3 * top[:-1]).all(), "row %d is not decisive: %s" % (r, top)
        assert _order(dist64[r], 1)[0] == win[r, 0]
    assert all(ptr64[r, t] > 0 for r in range(R) for t in (35999, 36000, V - 1)), "no pointer mass was planted"
    with Calls() as c:
        gen, dist, ids = ops.pointer_head_decode(*head)
        gen2, dist2, ids2 = ops.pointer_head_decode(*head, row="global")
    assert c.count(WIDE[0]) == 2 and sum(c.count(k) for k in LDS) == 0, "row='auto' beyond 36 000 ids must take the wide form: %s" % c.calls
    assert _same(gen, gen2) and _same(dist, dist2) and _same(ids, ids2), "two launches differ"
    eg, ed = _within(to_np(gen), gen64, 2e-5, 1e-9), _within(to_np(dist), dist64, 3e-5, 1e-8)
    print("V %d R %d: gen %.3f of its bar, dist %.3f of its bar" % (V, R, eg, ed))
    record_error("wide_head_V%d_R%d" % (V, R), "fp32", "gen_in_bar(rtol 2e-5, atol 1e-9)", eg, 1.0)
    record_error("wide_head_V%d_R%d" % (V, R), "fp32", "dist_in_bar(rtol 3e-5, atol 1e-8)", ed, 1.0)
    _measured("k23_wide_vs_float64/V%d_R%d/gen_in_bar" % (V, R), eg, 1.0)
    _measured("k23_wide_vs_float64/V%d_R%d/dist_in_bar" % (V, R), ed, 1.0)
    assert eg <= 1.0 and ed <= 1.0
    got = to_np(dist)
    assert to_np(ids).tolist() == [int(_order(dist64[r], 1)[0]) for r in range(R)] == win[:, 0].tolist()
    assert to_np(ids).tolist() == [int(np.argmax(got[r])) for r in range(R)], "ids is not the lowest-index argmax of the returned row"
    # K24
    for W in (1, 4, 8):
        with Calls() as c:
            _, d, cand_p, cand_id = ops.pointer_head_topk(*head, W, want_dist=True)
            again = ops.pointer_head_topk(*head, W, want_dist=True)
        assert c.count(WIDE[1]) == 2 and sum(c.count(k) for k in LDS) == 0
        assert _same(d, dist) and _same(cand_p, again[2]) and _same(cand_id, again[3])
        want = np.stack([_order(dist64[r], W) for r in range(R)])
        assert np.array_equal(to_np(cand_id), want), "K24 W %d: %s, restatement %s" % (W, to_np(cand_id).tolist(), want.tolist())
        p = to_np(cand_p)
        assert (p[:, :-1] > p[:, 1:]).all(), "cand_p is not descending"
        assert _same(cand_p, dist.gather(1, cand_id))
        ep = _within(p, np.take_along_axis(dist64, want, axis=1), 3e-5, 1e-8)
        _measured("k24_wide_vs_float64/V%d_R%d_W%d/cand_p_in_bar" % (V, R, W), ep, 1.0)
        assert ep <= 1.0
    # ties: two bit-equal maximal logits, no pointer mass on either
    lo, hi = 35999, V - 1
    flat = torch.full((R, V), -5.0, device="cuda")
    flat[:, lo] = 9.0
    flat[:, hi] = 9.0
    src2 = torch.full((R, sum(WIDE_LENS)), 3, device="cuda")
    _, d2, i2 = ops.pointer_head_decode(flat, mix, ops.SortedSource(src2, V), copies, want_gen=False)
    _, _, cp2, ci2 = ops.pointer_head_topk(flat, mix, ops.SortedSource(src2, V), copies, 4)
    d2n = to_np(d2)
    assert (d2n[:, lo] == d2n[:, hi]).all() and (d2n[:, lo] > d2n[:, 3]).all(), "the tie was not built"
    assert to_np(i2).tolist() == [lo] * R == [int(np.argmax(d2n[r])) for r in range(R)], "a tie must give the lower id"
    assert to_np(ci2)[:, :3].tolist() == [[lo, hi, 3]] * R
    # the ban: the ban-off row with the restated rule's entries set to 0.0, bit for bit
    t, Tm = 7, 12
    words = np.asarray([int(win[0, 0]), 35999, 36000, V - 1])
    rng = np.random.RandomState(V)
    hist = words[rng.randint(0, 4, size=(R, Tm))].astype(np.int32)
    hist[0] = win[0, 0]
    for n in (1, 3):
        want = got.copy()
        lists = [_ban(hist[r, :t].tolist(), n, V, None) for r in range(R)]
        assert lists[0] == [int(win[0, 0])]
        for r in range(R):
            want[r, lists[r]] = 0.0
        want_ids = [int(np.argmax(row)) for row in want]
        h = torch.from_numpy(hist).cuda()
        _, d, i = ops.pointer_head_decode(*head, want_gen=False, ban=(h, t, n, None))
        assert np.array_equal(to_np(d).view(np.uint32), want.view(np.uint32)), "K23 n %d: not the zeroed row" % n
        assert to_np(i).tolist() == want_ids == to_np(h)[:, t].tolist() and want_ids[0] != win[0, 0]
        h = torch.from_numpy(hist).cuda()
        _, d, cp, ci = ops.pointer_head_topk(*head, 4, want_dist=True, ban=(h, t, n, None))
        assert np.array_equal(to_np(d).view(np.uint32), want.view(np.uint32)) and np.array_equal(to_np(h), hist)
        assert to_np(ci).tolist() == [_order(row.astype(np.float64), 4).tolist() for row in want]
        h = torch.from_numpy(hist).cuda()
        ended = torch.zeros(R, dtype=torch.uint8, device="cuda")
        u = torch.full((R,), 0.5, device="cuda")
        _, d, i, p = ops.pointer_head_sample(*head, ended, False, False, -1, -1, 0, 1.0, 1, 1.0, uniforms=u, want_dist=True, ban=(h, t, n))
        assert np.array_equal(to_np(d).view(np.uint32), want.view(np.uint32)), "K28 n %d: not the zeroed row" % n
        assert to_np(i).tolist() == want_ids == to_np(h)[:, t].tolist()


# ---------------------------------------------------------------------------------------------
# 3. sampling beyond the LDS row
# ---------------------------------------------------------------------------------------------
def _interval(p, params, u, j, tol):
    """tests/test_sample_gpu.py::_interval restated: how the kernel's id ``j`` stands against the restatement's draw from the row ``p`` (f64)
    with the uniform ``u``: "in" with the violation of  CDF(j - 1) - tol Z <= u Z <= CDF(j) + tol Z  in units of tol Z (<= 1 passes), or "cut"
    when j is not in the restatement's kept set but tied with its cut within f32 rounding (value within 2e-6, or the first dropped entry with
    the top-p target within tol of the prefix mass)."""
    d = draw(p, *params, u)
    q, Z = d["q"], d["Z"]
    assert q[j] > 0, "an entry without mass was drawn (id %d)" % j
    if not d["kept"][j]:
        assert q[j] >= d["cut"] * (1 - 2e-6) or (j == d["next"] and d["slack"] <= tol), \
            "id %d (q %.9g) is outside the kept set (cut %.9g, slack %.3g) for %s" % (j, q[j], d["cut"], d["slack"], params)
        return "cut", 0.0
    lo, hi, thr = d["cdf"][j] - q[j], d["cdf"][j], u * Z
    return "in", max(lo - thr, thr - hi, 0.0) / (tol * Z)


def test_wide_sampler_draws_inside_the_restated_interval():
    """V = 50 265, the filter settings of the bit-equality test: the drawn id is kept by the restatement (or tied with its cut) and satisfies
    CDF(j - 1) - tol <= u Z <= CDF(j) + tol with tol = 4 (ceil(V / 1024) + 16) 2^-24 Z, the bound tests/test_sample_gpu.py derives for the
    scan (its depth, ceil(V / 4096) + 26, is the same in the wide form: the same tree).  The fused row is the wide K23's bit for bit, the
    fused and ``dist_in`` modes agree, ``prob`` is the row's own entry, and one kept entry is the wide K23's id."""
    from case_rg_amd import ops
    V, R = 50265, 3
    logits, mix, sm, copies, src, win = _wide_inputs(V, R)
    logits = logits.clone()
    for r in range(R):  # (a flatter row than the planted one: the draw has a choice)
        logits[r, torch.as_tensor(win[r], device="cuda")] -= 3.0
    head = (logits, mix, sm, copies)
    k23_gen, k23_dist, k23_ids = ops.pointer_head_decode(*head)
    rows = to_np(k23_dist).astype(np.float64)
    tol = 4 * (math.ceil(V / 1024) + 16) * 2.0 ** -24
    rs = np.random.RandomState(V)
    usets = [np.array([0.0, U_MAX, 0.5]), np.array([U_MAX, 0.0, 0.25]), rs.randint(0, 2 ** 24, R) * 2.0 ** -24, rs.randint(0, 2 ** 24, R) * 2.0 ** -24]
    worst, cuts, n = 0.0, 0, 0
    for params in [(1.0, 0, 1.0), (1.0, 5, 1.0), (1.0, 0, 0.9), (0.7, 0, 1.0), (0.7, 5, 0.9), (1.0, 1, 1.0)]:
        for us in usets:
            u = torch.tensor(us, dtype=torch.float32, device="cuda")
            ended = torch.zeros(R, dtype=torch.uint8, device="cuda")
            with Calls() as c:
                gen, dist, ids, prob = ops.pointer_head_sample(*head, ended, False, False, -1, -1, 0, *params, uniforms=u, want_gen=True, want_dist=True)
                _, dist2, ids2, prob2 = ops.pointer_head_sample(None, None, None, None, ended, False, False, -1, -1, 0, *params, uniforms=u,
                                                                dist_in=k23_dist, want_dist=True)
            assert c.count(WIDE[2]) == 2 and sum(c.count(k) for k in LDS) == 0, c.calls
            assert _same(dist, k23_dist) and _same(dist2, k23_dist) and _same(gen, k23_gen), "the row differs from the wide K23's"
            assert _same(ids, ids2) and _same(prob, prob2), "fused and dist_in modes disagree for %s" % (params,)
            assert _same(prob, k23_dist.gather(1, ids[:, None])[:, 0]) and not ended.any()
            for r in range(R):
                kind, viol = _interval(rows[r], params, float(us[r]), int(ids[r]), tol)
                cuts += kind == "cut"
                n += 1
                worst = max(worst, viol)
                assert viol <= 1.0, "row %d %s u %.9g: id %d misses its interval by %.3g tol" % (r, params, us[r], int(ids[r]), viol)
            if params[1] == 1:
                assert _same(ids, k23_ids), "top_k = 1 must return the wide K23's id"
    record_error("wide_head_sample_V%d_R%d" % (V, R), "fp32", "interval_violation_in_tol", worst, 1.0)
    _measured("k28_wide/V%d_R%d/interval_violation_in_tol" % (V, R), worst, 1.0)
    print("V %d R %d: worst interval violation %.3g tol, %d of %d draws on a cut tie" % (V, R, worst, cuts, n))
    assert cuts * 20 <= n, "too many draws fell on a cut tie to call the kept set checked"


@pytest.mark.parametrize("V", [50265, 50268])
def test_wide_sampler_follows_the_loop_conventions(V):
    """Rows with all mass on one token (one of them the last id), read where they lie (V = 50 268: aligned rows) and through the workspace."""
    from case_rg_amd import ops
    EOS, UNK, PAD = V - 1, 7, 0
    dev = torch.device("cuda")
    d = torch.zeros(4, V, device=dev)
    for r, tok in enumerate([EOS, 36000, EOS, 35999]):
        d[r, tok] = 1.0
    keep = d.clone()
    u = torch.full((4,), 0.5, device=dev)

    def step(ended, first, last):
        e = torch.tensor(ended, dtype=torch.uint8, device=dev)
        with Calls() as c:
            _, _, ids, prob = ops.pointer_head_sample(None, None, None, None, e, first, last, EOS, UNK, PAD, 1.0, 0, 1.0, uniforms=u, dist_in=d)
        assert c.count(WIDE[2]) == 1 and sum(c.count(k) for k in LDS) == 0
        return ids.tolist(), e.tolist(), prob.tolist()

    assert step([0, 0, 0, 0], True, False) == ([UNK, 36000, UNK, 35999], [1, 0, 1, 0], [1.0] * 4)
    assert step([0, 0, 1, 1], False, False) == ([EOS, 36000, PAD, PAD], [1, 0, 1, 1], [1.0] * 4)
    assert step([0, 0, 1, 1], False, True) == ([EOS, EOS, PAD, PAD], [1, 0, 1, 1], [1.0] * 4)
    assert torch.equal(d, keep), "dist_in was written"


# ---------------------------------------------------------------------------------------------
# 4. whole passes
# ---------------------------------------------------------------------------------------------
V_WIDE, V_LDS, H_, T_, ITEMS = 36100, 30522, 32, 12, 4
PASS_TOL = 10 * 1.5e-6  # the pass-level tolerance of tests/test_ngram_block_gpu.py: ten times what profiles/ngram_parity.json records
BEAM_BAR = 5e-6


@pytest.fixture(scope="module")
def ns():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.float32)
    case_rg_amd.set_dropout(False)
    return case_rg_amd.namespace()


def _build(ns, kind, V):
    from case_rg_amd.utils import fill_params, make_vocab, synth_batch
    v2i, i2v = make_vocab(V)
    model = ns.CaSE(4, T_, i2v, v2i, H_) if kind == "case" else ns.Masque(T_, i2v, v2i, H_)
    model = fill_params(model, 153, gain=3.0).cuda().eval()
    return model, {k: v.cuda() for k, v in synth_batch(ITEMS, 3, 12, 8, 6, V, seed=152, model=kind).items()}


@pytest.fixture(scope="module")
def wide_models(ns):
    """kind -> (model in eval mode, batch on the device) with 36 100 words, built once and left unchanged."""
    return {kind: _build(ns, kind, V_WIDE) for kind in ("case", "masque")}


class _Unfused:
    def __enter__(self):
        from case_rg_amd import ops
        self.old, ops.POINTER_HEAD = ops.POINTER_HEAD, "off"

    def __exit__(self, *exc):
        from case_rg_amd import ops
        ops.POINTER_HEAD = self.old


def _drawn_positions(samples, unk, pad):
    """Where ``sample_probs`` is the probability of the EMITTED token (tests/test_score_gpu.py)."""
    keep = samples != pad
    keep[..., -1] = False
    keep[..., 0] &= samples[..., 0] != unk
    return keep


def _beam_costs(token_probs, answers, eos):
    """tests/test_score_gpu.py::_beam_costs: sum_t -log(p_t + 1e-10) / (n + 1) over the n tokens up to and including EOS."""
    B, W, T = answers.shape
    cost, usable = np.zeros((B, W)), np.zeros((B, W), dtype=bool)
    for b in range(B):
        for w in range(W):
            ids = answers[b, w].tolist()
            n = ids.index(eos) + 1 if eos in ids else T
            usable[b, w] = 0 not in ids[:n]
            cost[b, w] = sum(-math.log(token_probs[b, w, t] + 1e-10) for t in range(n)) / (n + 1)
    return cost, usable


def _no_lds_heads(c):
    return sum(c.count(k) for k in LDS) == 0


class _Fused:
    def __enter__(self):
        pass

    def __exit__(self, *exc):
        pass


@pytest.mark.parametrize("head", ["fused", "unfused"])
@pytest.mark.parametrize("kind", ["case", "masque"])
def test_sampled_pass_beyond_the_lds_row_is_rescored(wide_models, kind, head):
    """``do_sample`` runs with 36 100 words -- through the fused wide K28, and with ``CASE_POINTER_HEAD=off`` through the wide K28 on the unfused
    distribution (``dist_in``) -- and ``do_score`` reproduces the probabilities it recorded."""
    m, b = wide_models[kind]
    dec = m.response_generation.decoder
    _, eos, unk, pad = special_ids(m)
    with torch.no_grad(), Calls() as c:
        with (_Fused() if head == "fused" else _Unfused()):
            drawn = m.do_sample(dict(b), num_samples=2, seed=5)
        steps = dec.last_sample_steps
        again = m.do_score(dict(b), drawn["samples"])
    assert c.count(WIDE[2]) == steps >= 1 and _no_lds_heads(c), "not one wide K28 per step: %s" % c.calls
    if head == "unfused":
        assert c.count("case_copy_scatter_sorted_fwd") >= steps, "the unfused chain did not run: %s" % c.calls
    assert drawn["samples"].shape == (ITEMS, 2, T_)
    samples = to_np(drawn["samples"])
    want, got = to_np(drawn["sample_probs"]).astype(np.float64), to_np(again["token_probs"]).astype(np.float64)
    keep = _drawn_positions(samples, unk, pad)
    assert keep.sum() >= samples.size // 4, "too few comparable positions: %d" % keep.sum()
    err = float(np.abs(got - want)[keep].max())
    print("%s %s: sampled pass vs rescoring over %d positions: %.3e" % (kind, head, keep.sum(), err))
    record_error("wide_%s_V%d" % (kind, V_WIDE), "fp32", "rescored_sample_probs_abs_%s" % head, err, PASS_TOL)
    _measured("%s/%s/rescored_sample_probs_abs" % (kind, head), err, PASS_TOL)
    assert err <= PASS_TOL


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_beam_pass_beyond_the_lds_row_is_rescored(wide_models, kind):
    m, b = wide_models[kind]
    dec = m.response_generation.decoder
    _, eos, unk, pad = special_ids(m)
    with torch.no_grad(), Calls() as c:
        beam = m.do_beam(dict(b), width=4)
        steps = dec.last_beam_steps
        rescored = m.do_score(dict(b), beam["beam_answers"])
    assert c.count(WIDE[1]) == steps >= 1 and _no_lds_heads(c), "not one wide K24 per step: %s" % c.calls
    scores = to_np(beam["beam_scores"]).astype(np.float64)
    cost, usable = _beam_costs(to_np(rescored["token_probs"]).astype(np.float64), to_np(beam["beam_answers"]), eos)
    fin = np.isfinite(scores) & usable
    assert fin.sum() >= scores.shape[0], "too few finished hypotheses to compare"
    rel = float((np.abs(cost - scores)[fin] / np.abs(scores)[fin]).max())
    print("%s: beam costs vs rescoring over %d hypotheses: %.3e" % (kind, fin.sum(), rel))
    record_error("wide_%s_V%d" % (kind, V_WIDE), "fp32", "rescored_beam_scores", rel, BEAM_BAR)
    _measured("%s/rescored_beam_scores" % kind, rel, BEAM_BAR)
    assert rel <= BEAM_BAR


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_greedy_pass_beyond_the_lds_row_equals_the_unfused_pass(wide_models, kind):
    """One wide K23 per step; the answers are the ``CASE_POINTER_HEAD=off`` pass's item by item up to the first position where the unfused
    distribution's two largest entries are within 1e-5 of each other (relative); at least 90 % of the (item, position) pairs are compared."""
    from case_rg_amd import ops
    m, b = wide_models[kind]
    dec = m.response_generation.decoder
    with torch.no_grad(), Calls() as c:
        fused = to_np(m.do_test(dict(b))["answer"])
        steps = dec.last_greedy_steps
    assert c.count(WIDE[0]) == steps == T_ and _no_lds_heads(c), c.calls
    gaps, real = [], ops.row_argmax

    def recording(x, *a, **kw):
        if tuple(x.shape) == (ITEMS, V_WIDE):  # the unfused head's newest position
            top = torch.topk(x.float(), 2, dim=-1).values
            gaps.append(to_np((top[:, 0] - top[:, 1]) / top[:, 0]))
        return real(x, *a, **kw)

    ops.row_argmax = recording
    try:
        with torch.no_grad(), _Unfused(), Calls() as c:
            plain = to_np(m.do_test(dict(b))["answer"])
    finally:
        ops.row_argmax = real
    assert sum(c.count(k) for k in WIDE + LDS) == 0 and len(gaps) == T_, c.calls
    gaps = np.stack(gaps, axis=1)  # [items, T]
    compared = 0
    for i in range(ITEMS):
        close = np.flatnonzero(gaps[i] < 1e-5)
        n = int(close[0]) if close.size else T_
        compared += n
        assert np.array_equal(fused[i, :n], plain[i, :n]), "%s item %d: fused %s, unfused %s (decisive for %d steps)" % (kind, i, fused[i], plain[i], n)
    share = compared / (ITEMS * T_)
    _measured("%s/greedy_compared_share" % kind, share, 0.9)
    assert share >= 0.9, "only %.0f %% of the (item, position) pairs were decisive" % (100 * share)


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_consensus_ban_and_capture_beyond_the_lds_row(wide_models, kind):
    m, b = wide_models[kind]
    dec = m.response_generation.decoder
    _, eos, unk, pad = special_ids(m)
    with torch.no_grad(), Calls() as c:
        out = m.do_consensus(dict(b), pool="sample", num_samples=3, seed=9)
    assert c.count(WIDE[2]) >= 1 and _no_lds_heads(c)
    assert out["answer"].shape == (ITEMS, T_) and out["consensus_index"].shape == (ITEMS,) and out["samples"].shape == (ITEMS, 3, T_)
    # the ban inside the wide K28
    with torch.no_grad(), Calls() as c:
        banned = m.do_sample(dict(b), num_samples=2, seed=5, top_k=3, no_repeat_ngram=3)
    assert c.count(WIDE[2]) == dec.last_sample_steps and _no_lds_heads(c)
    for row in to_np(banned["samples"]).reshape(-1, T_):
        toks = [int(x) for x in row]
        toks = toks[:toks.index(eos)] if eos in toks else toks
        grams = [tuple(toks[i:i + 3]) for i in range(len(toks) - 2)]
        assert len(grams) == len(set(grams)), "a repeated trigram under no_repeat_ngram=3: %s" % toks
    # a captured sampled pass replays to the eager pass's samples
    keys = ("samples", "sample_probs", "sample_scores")
    with torch.no_grad():
        eager = {k: v.clone() for k, v in m.do_sample(dict(b), num_samples=2, seed=5).items()}
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.do_sample(dict(b), num_samples=2, seed=5)  # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        graph, static = torch.cuda.CUDAGraph(), {}
        with torch.cuda.graph(graph), Calls() as c:
            static.update(m.do_sample(dict(b), num_samples=2, seed=5))
        assert c.count(WIDE[2]) == T_ == dec.last_sample_steps, "a captured pass runs the fixed T steps"
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            for k in keys:
                assert torch.equal(static[k], eager[k]), "a replay must repeat the eager pass's %s" % k
        del graph


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_launches_at_30522_words_are_the_lds_forms(ns, kind):
    """With V <= 36 000 every mode makes the launches it made: one LDS head per step, no wide launch, no workspace."""
    m, b = _build(ns, kind, V_LDS)
    dec = m.response_generation.decoder
    with torch.no_grad():
        with Calls() as c:
            m.do_test(dict(b))
        assert c.count("case_pointer_head_decode") == dec.last_greedy_steps == T_ and sum(c.count(k) for k in WIDE + LDS) == T_, c.calls
        with Calls() as c:
            m.do_beam(dict(b), width=4)
        assert c.count("case_pointer_head_beam") == dec.last_beam_steps >= 1 and sum(c.count(k) for k in WIDE + LDS) == dec.last_beam_steps, c.calls
        with Calls() as c:
            m.do_sample(dict(b), num_samples=2, seed=5)
        assert c.sampled == dec.last_sample_steps >= 1 and sum(c.count(k) for k in WIDE + LDS) == dec.last_sample_steps, c.calls
        with Calls() as c:
            m.do_sample(dict(b), num_samples=2, seed=5, no_repeat_ngram=3)
        assert c.count("case_pointer_head_sample_ban") == dec.last_sample_steps and sum(c.count(k) for k in WIDE + LDS) == dec.last_sample_steps, c.calls
