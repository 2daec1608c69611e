"""Answer attribution on the MI355X: K39 (``case_copy_attribution``) bit for bit against a per-position Python loop on inputs where every
operation is exact, against the f64 restatement, K29 and the host form on random inputs, and ``do_attribute`` / ``evaluate_attribution`` on
a tiny CaSE and Masque (P = 3 passages: G = 4 segments) in fp32 and bf16.

Measured maxima go to profiles/attribution_parity.json."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import cases
from helpers import FP32_BAR, Calls, special_ids, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 2e-5  # the bar K23's ``gen`` is held to: the bar below is never looser
# ten times the worst relative distance measured on the MI355X (profiles/attribution_parity.json: 8.115e-07, K39 against the host form on
# the tiny Masque in fp32; against the f64 restatement 2.905e-07, against K29's copy 1.218e-07).  The error is that of __expf and the f32
# division in pm and of the f32 product of a term; the sums themselves are f64.
BAR = min(CAP, 10 * 8.115e-07)


def _measured(key, value, bar=None):
    """Add one measured maximum to profiles/attribution_parity.json."""
    path = os.path.join(ROOT, "profiles", "attribution_parity.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = {}
    if os.path.exists(path):
        with open(path) as fh:
            data = json.load(fh)
    data[key] = {"measured": float("%.3e" % value), "bar": bar}
    with open(path, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)


def _rel(got, want):
    """max |got - want| / |want| over the entries with want > 0; the entries with want == 0 must be exactly 0."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert (got[want == 0] == 0).all(), "exactly 0 where the restatement is 0"
    keep = want > 0
    return float((np.abs(got - want)[keep] / want[keep]).max()) if keep.any() else 0.0


@pytest.fixture(scope="module")
def ns():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.float32)
    case_rg_amd.set_dropout(False)
    return case_rg_amd.namespace()


class _HostForm:
    """CASE_COPY_ATTRIBUTION=off for the block."""

    def __enter__(self):
        from case_rg_amd import ops
        self.old, ops.COPY_ATTRIBUTION = ops.COPY_ATTRIBUTION, "off"

    def __exit__(self, *exc):
        from case_rg_amd import ops
        ops.COPY_ATTRIBUTION = self.old


def restated(mix, src, rps, copies, targets, seg, pad, V):
    """The definition position by position in Python floats (f64) on the same f32 inputs -> mass [R, G], pos, pos_mass, count, and per
    row the f64 terms of the run by position (for the tie allowance)."""
    mix = np.asarray(mix, dtype=np.float64)
    cs = np.concatenate([np.asarray(c, dtype=np.float64) for c in copies], axis=1)
    mem_of = np.concatenate([np.full(np.asarray(c).shape[1], k) for k, c in enumerate(copies)])
    src, seg = np.asarray(src), list(seg)
    R, G = mix.shape[0], len(seg) - 1
    seg_of = np.searchsorted(np.asarray(seg[1:]), np.arange(src.shape[1]), side="right")
    mass, pos, pos_mass, count, terms = np.zeros((R, G)), np.full(R, -1), np.zeros(R), np.zeros(R, dtype=np.int64), [dict() for _ in range(R)]
    for r in range(R):
        y = int(targets[r])
        if (pad >= 0 and y == pad) or y < 0 or y >= V:
            continue
        with np.errstate(under="ignore"):
            e = np.exp(mix[r] - mix[r].max())
        pm = e / e.sum()
        best = None
        for s in np.nonzero(src[r // rps] == y)[0].tolist():
            term = float(pm[1 + mem_of[s]] * cs[r, s])
            mass[r, seg_of[s]] += term
            count[r] += 1
            terms[r][s] = term
            if best is None or term > best:
                best, pos[r] = term, s
        pos_mass[r] = 0.0 if best is None else best
    return mass, pos, pos_mass, count, terms


# ---------------------------------------------------------------------------------------------
# 1. the exact leg: every operation is exact, so the kernel equals the loop in every bit
# ---------------------------------------------------------------------------------------------
RUNS = (130, 65, 64, 63, 2, 1)  # the planted run lengths (0: a token that is absent), largest first so that a small S keeps the long ones


def _boundaries(S, G, rng):
    """G segments of [0, S): one-position segments in front (0 | 1 | 2 ...), the others cut at random; G = 64 is 63 of one position and
    the rest in one."""
    if G == 1:
        return [0, S]
    ones = min(G - 1, 3) if G < 64 else 63
    ones = min(ones, S - 1)
    free = G - 1 - ones
    rest = sorted(rng.choice(np.arange(ones + 1, S), size=free, replace=False).tolist()) if free else []
    return list(range(ones + 1)) + rest + [S]


def _exact_case(R, rps, S, nmem, G, V, tail, seed):
    """-> mix, src [K, S], lens, copies, targets (a cycle of planted and special ids), seg.  pm is exact: equal logits for 1 and 3 memories
    (1/2, 1/4), an -inf logit on the last of 2 and 4 memories ((1/2, 1/2, 0) and four times 1/4 with a last memory whose terms are all 0.0);
    the copy weights are multiples of 2^-10, with a planted pair of equal maxima and an all-zero run in every item."""
    rng = np.random.RandomState(seed)
    K = R // rps
    cuts = sorted(rng.choice(np.arange(1, S), size=nmem - 1, replace=False).tolist()) if nmem > 1 else []
    lens = np.diff([0] + cuts + [S]).tolist()
    low, high = 5, max(6, V // 2)
    src = rng.randint(low, high, size=(K, S))
    planted = []
    for k in range(K):
        free, token = rng.permutation(S).tolist(), V - 1  # V - 1 is the largest id: its run ends at S unless ids outside [0, V) follow
        for n in RUNS:
            if n <= len(free) - (2 if tail == "invalid" and S > 2 else 0):
                at, free = free[:n], free[n:]
                src[k, at] = token
                if k == 0:
                    planted.append((token, n))
                token -= 1
        if tail == "invalid" and S > 2:
            src[k, free[0]], src[k, free[1]] = V, -7  # no tokens: 0xFFFFFFFF keys behind the last run
    mix = np.zeros((R, 1 + nmem), dtype=np.float32)
    if nmem in (2, 4):
        mix[:, nmem] = -np.inf
    weights = rng.randint(0, 1023, size=(R, S)).astype(np.float32) / 1024.0
    targets = np.zeros(R, dtype=np.int64)
    ids = [t for t, _ in planted]
    special = ids + [0, V, V // 2 + 3 if V // 2 + 3 < V - len(RUNS) else V - len(RUNS) - 1, -1, int(src[0, 0])]
    for r in range(R):
        targets[r] = special[r % len(special)] if r < 2 * len(special) else int(src[r // rps, rng.randint(S)])
        at = np.nonzero(src[r // rps] == targets[r])[0]
        if len(at) >= 2 and r % 3 == 0:  # equal maxima: the lower position must win
            weights[r, at[-1]] = weights[r, at[len(at) // 2]] = 1023.0 / 1024.0
        if len(at) >= 1 and r % 5 == 4:  # an all-zero run: its lowest position
            weights[r, at] = 0.0
    copies = np.split(weights, np.cumsum(lens)[:-1], axis=1)
    return mix, src, lens, [np.ascontiguousarray(c) for c in copies], targets, _boundaries(S, G, rng)


def _launch(mix, src, rps, copies, targets, seg, pad, V, seg_tensor=False):
    from case_rg_amd import ops
    dev = torch.device("cuda")
    sm = ops.SortedSource(torch.from_numpy(np.asarray(src)).to(dev), V)
    seg_arg = torch.tensor(seg, dtype=torch.int32, device=dev) if seg_tensor else seg
    args = (torch.from_numpy(mix).to(dev), sm, rps, [torch.from_numpy(c).to(dev) for c in copies], torch.from_numpy(targets).to(dev), seg_arg)
    return ops.copy_attribution(*args, pad=pad), args


EXACT = [  # R, rps, S, nmem, G, V, tail
    (1, 1, 1, 1, 1, 200, "end"), (3, 1, 63, 1, 2, 200, "end"), (3, 1, 64, 2, 11, 200, "end"), (3, 1, 65, 4, 64, 200, "end"),
    (130, 5, 200, 3, 11, 1031, "invalid"), (130, 1, 200, 2, 64, 131071, "end"), (130, 5, 3904, 2, 11, 30522, "end"),
    (3, 1, 3904, 4, 64, 131071, "invalid"), (5, 5, 3904, 1, 1, 30522, "end"), (2, 1, 32768, 4, 11, 131071, "end"),
    (2, 1, 32768, 1, 64, 30522, "invalid"), (10, 5, 65, 3, 2, 131071, "invalid"),
]


@pytest.mark.parametrize("R,rps,S,nmem,G,V,tail", EXACT)
def test_exact_inputs_give_the_loops_bits(R, rps, S, nmem, G, V, tail):
    mix, src, lens, copies, targets, seg = _exact_case(R, rps, S, nmem, G, V, tail, 17 * S + 3 * R + nmem + G)
    assert len(seg) == G + 1 and seg[0] == 0 and seg[-1] == S
    for pad in (0, -1):
        want = restated(mix, src, rps, copies, targets, seg, pad, V)
        got, args = _launch(mix, src, rps, copies, targets, seg, pad, V, seg_tensor=(pad == -1))
        assert got["mass"].dtype == torch.float32 and tuple(got["mass"].shape) == (R, G)
        assert got["pos"].dtype == got["count"].dtype == torch.int32 and got["pos_mass"].dtype == torch.float32
        assert np.array_equal(to_np(got["count"]), want[3]), "count (pad %d)" % pad
        assert np.array_equal(to_np(got["pos"]), want[1]), "pos (pad %d)" % pad
        assert np.array_equal(to_np(got["mass"]), want[0].astype(np.float32)), "mass (pad %d)" % pad
        assert np.array_equal(to_np(got["pos_mass"]), want[2].astype(np.float32)), "pos_mass (pad %d)" % pad
    longest = max(n for n in RUNS if n <= S - (2 if tail == "invalid" and S > 2 else 0))
    assert int(want[3].max()) >= longest, "the case must hold its longest run"
    from case_rg_amd import ops
    again = ops.copy_attribution(*args, pad=-1)
    for key in got:
        assert torch.equal(again[key], got[key]), "two launches differ in %s" % key


def test_exact_targets_at_the_edges_of_the_vocabulary():
    """PAD; -1 with pad = -1; V; V - 1 with V = 131 071 (the largest id the key format takes: its run ends at S)."""
    V, S = 131071, 200
    mix, src, lens, copies, _, seg = _exact_case(8, 1, S, 3, 11, V, "end", 991)
    targets = np.array([0, -1, V, V - 1, V - 1, 0, V + 5, V - 2], dtype=np.int64)
    for k in range(src.shape[0]):  # PAD's id occurs in the source: not scored with pad = 0, an ordinary token with pad = -1
        src[k, np.nonzero(src[k] < V // 2)[0][0]] = 0
    for pad in (0, -1):
        want = restated(mix, src, 1, copies, targets, seg, pad, V)
        got, _ = _launch(mix, src, 1, copies, targets, seg, pad, V)
        for i, key in enumerate(("mass", "pos", "pos_mass", "count")):
            assert np.array_equal(to_np(got[key]).astype(np.float64), np.asarray(want[i], dtype=np.float64)), (key, pad)
        assert int(got["count"][3]) == 130 and int(got["pos"][1]) == -1 and int(got["pos"][2]) == -1
        assert (int(got["count"][0]) == 0) == (pad == 0)


def test_launch_replays_from_a_captured_graph():
    from case_rg_amd import ops
    mix, src, lens, copies, targets, seg = _exact_case(130, 5, 200, 3, 11, 1031, "invalid", 77)
    eager, args = _launch(mix, src, 5, copies, targets, seg, 0, 1031)
    for seg_arg in (seg, torch.tensor(seg, dtype=torch.int32, device="cuda")):
        args = args[:5] + (seg_arg,)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.copy_attribution(*args)  # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        graph, static = torch.cuda.CUDAGraph(), {}
        with torch.cuda.graph(graph):
            static.update(ops.copy_attribution(*args))
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            for key in eager:
                assert torch.equal(static[key], eager[key]), "the replay differs from the eager launch in %s" % key
        del graph


def test_wrapper_argument_checks():
    from case_rg_amd import ops
    mix, src, lens, copies, targets, seg = _exact_case(4, 1, 65, 2, 2, 200, "end", 5)
    _, args = _launch(mix, src, 1, copies, targets, seg, 0, 200)
    mixd, sm, rps, cs, y, _ = args
    for bad in ([0, 65, 65], [0, 70, 65], [1, 65], [0, 64], list(range(66))):
        with pytest.raises(ValueError):
            ops.copy_attribution(mixd, sm, rps, cs, y, bad)
    with pytest.raises(TypeError):
        ops.copy_attribution(mixd, sm, rps, cs, y, torch.tensor(seg, device="cuda"))  # int64
    with pytest.raises(ValueError):
        ops.copy_attribution(mixd, sm, rps, cs, y, torch.zeros(66, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        ops.copy_attribution(mixd, sm.ids, rps, cs, y, seg)
    with pytest.raises(ValueError):
        ops.copy_attribution(mixd, sm, rps, cs[:1], y, seg)
    with pytest.raises(TypeError):
        ops.copy_attribution(mixd, sm, rps, cs, y.int(), seg)
    with pytest.raises(ValueError):
        ops.copy_attribution(mixd, sm, 3, cs, y, seg)
    assert ops.copy_attribution_supported(sm, 2) and not ops.copy_attribution_supported(sm.ids, 2) and not ops.copy_attribution_supported(sm, 5)
    with _HostForm():
        assert not ops.copy_attribution_supported(sm, 2)


# ---------------------------------------------------------------------------------------------
# 2. the random leg: the f64 restatement of the same f32 inputs, K29 and the host form
# ---------------------------------------------------------------------------------------------
def _random_case(R, rps, V, S, nmem, seed):
    """Random mixing logits and softmax copy weights; source ids from a range of S // 6 ids, so a target's run has about six entries, one
    long run (90, or S // 2) across the memories' boundary, and ids outside [0, V)."""
    g = torch.Generator().manual_seed(seed)
    K = R // rps
    lens = [S] if nmem == 1 else [S // 4, S - S // 4]
    src = torch.randint(5, 5 + max(2, S // 6), (K, S), generator=g)
    run = min(S // 2, 90)
    start = lens[0] - run // 2 if nmem == 2 else 3
    src[:, start:start + run] = V - 1
    src[:, 0], src[:, S - 1] = V, -2
    logits = torch.randn(R, V, generator=g) * 2.0
    mix = torch.randn(R, 1 + nmem, generator=g)
    copies = [torch.softmax(torch.randn(R, n, generator=g) * 2.0, dim=-1) for n in lens]
    targets = src[torch.arange(R) // rps, torch.randint(1, S - 1, (R,), generator=g)].clone()
    targets[0], targets[1 % R], targets[2 % R] = V - 1, 0, 4  # the long run, PAD, an absent id
    return logits, mix, src, lens, copies, targets


@pytest.mark.parametrize("R,rps,V,S,nmem,G", [(8, 1, 200, 44, 1, 4), (96, 3, 30522, 1100, 2, 11), (130, 5, 1031, 3904, 2, 11)])
def test_random_inputs_against_float64_k29_and_the_host_form(R, rps, V, S, nmem, G):
    from case_rg_amd import ops
    from case_rg_amd.evaluation.attribution import copy_attribution_host
    logits, mix, src, lens, copies, targets = _random_case(R, rps, V, S, nmem, 11 * R + S)
    seg = _boundaries(S, G, np.random.RandomState(S + G))
    dev = torch.device("cuda")
    sm = ops.SortedSource(src.to(dev), V)
    on_dev = (mix.to(dev), sm, rps, [c.to(dev) for c in copies], targets.to(dev))
    got = ops.copy_attribution(*on_dev, seg, pad=0)
    mass, pos, pos_mass, count, terms = restated(mix.numpy(), src.numpy(), rps, [c.numpy() for c in copies], targets.numpy(), seg, 0, V)
    assert np.array_equal(to_np(got["count"]), count) and count.max() >= 44 // 2 and (count == 0).any()
    got_pos = to_np(got["pos"])
    for r in np.nonzero(got_pos != pos)[0].tolist():  # only where the two candidates are closer than the bar in f64
        a, b = terms[r][int(got_pos[r])], terms[r][int(pos[r])]
        assert abs(a - b) <= BAR * max(a, b), (r, a, b)
    seen = got_pos >= 0
    rows = np.arange(R)[seen] // rps
    assert np.array_equal(src.numpy()[rows, got_pos[seen]], targets.numpy()[seen]), "source_ids[item, pos] == target wherever pos >= 0"
    assert np.array_equal(seen, count > 0)
    worst = {"mass_vs_float64": _rel(to_np(got["mass"]), mass), "pos_mass_vs_float64": _rel(to_np(got["pos_mass"]), pos_mass)}
    _, k29 = ops.pointer_head_score(logits.to(dev), *on_dev, 0)
    total = to_np(got["mass"]).astype(np.float64).sum(axis=1)
    worst["sum_vs_k29_copy"] = _rel(to_np(k29), total)
    host = copy_attribution_host(on_dev[0], sm.ids, on_dev[3], on_dev[4], seg, pad=0, V=V)
    assert torch.equal(host["count"], got["count"]) and host["mass"].dtype == torch.float32 and host["pos"].dtype == torch.int32
    assert np.array_equal(to_np(host["pos"]), pos), "the host form is f64 throughout: the restatement's arg-max"
    worst["mass_vs_host_form"] = _rel(to_np(got["mass"]), to_np(host["mass"]))
    worst["pos_mass_vs_host_form"] = _rel(to_np(got["pos_mass"]), to_np(host["pos_mass"]))
    for key, rel in worst.items():
        print("K39 at R %d, S %d, %d memories, G %d: %s %.3e (bar %.1e)" % (R, S, nmem, G, key, rel, BAR))
        _measured("k39/%s/R%d_S%d" % (key, R, S), rel, BAR)
    assert BAR <= CAP and all(rel <= BAR for rel in worst.values()), worst


# ---------------------------------------------------------------------------------------------
# 3. the models
# ---------------------------------------------------------------------------------------------
ITEMS, P, L, LQ = 4, 3, 16, 8
ATTRIBUTION_KEYS = {"answers", "copy_mass", "copy_pos", "copy_pos_mass", "copy_count", "share", "support", "cited"}
SCORE_KEYS = {"rank", "token_probs", "copy_probs", "scores", "loss", "tokens"}


@contextlib.contextmanager
def _tiny(ns, name):
    """A tiny CaSE or Masque at P 3, L 16 in eval mode, its batch on the device, and two candidates per item: the response and a random
    answer that ends in EOS and PAD, whose first token is absent from the item's source and whose second a passage holds."""
    import case_rg_amd
    from case_rg_amd.utils import synth_batch
    kind, mode = name.split("-")
    case_rg_amd.set_compute_dtype(torch.bfloat16 if mode == "bf16" else torch.float32)
    try:
        build = cases._case_model if kind == "case" else cases._masque_model
        m = build(ns, torch.device("cuda"), 391, gain=3.0).eval()
        cpu = synth_batch(ITEMS, P, L, LQ, 6, cases.V, seed=392, model=kind)
        T = cpu["response"].shape[1]
        g = torch.Generator().manual_seed(393)
        other = torch.randint(5, cases.V, (ITEMS, T), generator=g)
        _, eos, _, _ = special_ids(m)
        other[:, T - 2], other[:, T - 1] = eos, 0
        for i in range(ITEMS):
            other[i, 0] = next(v for v in range(cases.V - 1, 4, -1) if not bool((cpu["source_map"][i] == v).any()))
            other[i, 1] = cpu["passage"][i, 1, 1]
        cands = torch.stack([cpu["response"], other], dim=1)
        yield m, {k: v.cuda() for k, v in cpu.items()}, cands.cuda(), cpu, name
    finally:
        case_rg_amd.set_compute_dtype(torch.float32)


@pytest.fixture(scope="module", params=["case-fp32", "case-bf16", "masque-fp32", "masque-bf16"])
def tiny(request, ns):
    with _tiny(ns, request.param) as built:
        yield built


def _bits_equal(a, b, keys, what):
    for k in keys:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), "%s: %s differs" % (what, k)


def test_do_attribute_scores_as_do_score_and_splits_the_copy_part(tiny):
    m, b, cands, cpu, name = tiny
    with torch.no_grad():
        before = m.do_score(dict(b), cands)
        with Calls() as c:
            out = m.do_attribute(dict(b), answers=cands)
        after = m.do_score(dict(b), cands)
        own = m.do_attribute(dict(b), answers="response")
        routed = m(dict(b), method="attribute")
        ref_own = m.do_score(dict(b))
    assert c.count("case_copy_attribution") == c.scored >= 1, c.calls
    assert set(out) == SCORE_KEYS | ATTRIBUTION_KEYS
    _bits_equal(out, before, SCORE_KEYS, "do_attribute(tensor) vs do_score")
    _bits_equal(after, before, SCORE_KEYS, "do_score before and after do_attribute")
    _bits_equal(own, ref_own, SCORE_KEYS, "do_attribute('response') vs do_score")
    T = cands.shape[-1]
    assert torch.equal(own["answers"], b["response"][:, None]) and torch.equal(out["answers"], cands)
    assert out["copy_mass"].shape == (ITEMS, 2, T, 1 + P) and out["copy_mass"].dtype == torch.float32
    assert out["copy_pos"].shape == out["copy_count"].shape == (ITEMS, 2, T) and out["copy_pos"].dtype == out["copy_count"].dtype == torch.int32
    assert out["share"].shape == (ITEMS, 2, T, 2 + P) and out["support"].shape == (ITEMS, 2, 2 + P)
    assert out["cited"].shape == (ITEMS, 2) and out["cited"].dtype == torch.int64
    test_keys = set(routed)
    assert test_keys == SCORE_KEYS | ATTRIBUTION_KEYS | {"answer"} and routed["answers"].shape[:2] == (ITEMS, 1)
    # the split adds up to K29's pointer part
    rel = _rel(to_np(out["copy_mass"]).astype(np.float64).sum(-1), to_np(out["copy_probs"]))
    print("%s: sum_g copy_mass vs copy_probs %.3e (bar %.1e)" % (name, rel, BAR))
    _measured("%s/copy_mass_sum_vs_copy_probs" % name, rel, BAR)
    assert rel <= BAR
    # the position holds the token; counts are the occurrences in the item's source
    ans, pos, src = to_np(out["answers"]), to_np(out["copy_pos"]), cpu["source_map"].numpy()
    occurs = (src[:, None, None, :] == ans[..., None]).sum(-1) * (ans != 0)
    assert np.array_equal(to_np(out["copy_count"]), occurs)
    assert np.array_equal(pos >= 0, occurs > 0)
    item = np.broadcast_to(np.arange(ITEMS)[:, None, None], pos.shape)
    assert np.array_equal(src[item[pos >= 0], pos[pos >= 0]], ans[pos >= 0])
    seg = np.searchsorted(np.array([LQ + p * L for p in range(P + 1)]), pos, side="right")
    mass = to_np(out["copy_mass"])
    assert (np.take_along_axis(mass, seg[..., None], -1)[..., 0][pos >= 0] >= to_np(out["copy_pos_mass"])[pos >= 0] * (1 - 1e-6)).all()
    # the planted absent token: nothing to copy, all of it generated
    assert (to_np(out["copy_count"])[:, 1, 0] == 0).all() and (pos[:, 1, 0] == -1).all() and (mass[:, 1, 0] == 0).all()
    share = to_np(out["share"])
    assert (share[:, 1, 0, 0] == 1.0).all() and (share[:, 1, 0, 1:] == 0).all()
    assert (to_np(out["copy_count"])[:, 1, 1] >= 1).all() and (mass[:, 1, 1, 1:].sum(-1) > 0).all()
    # shares
    p = to_np(out["token_probs"])
    live = (ans != 0) & (p > 0)
    assert np.abs(share.sum(-1)[live] - 1.0).max() <= 1e-6 and (share[ans == 0] == 0).all()
    from case_rg_amd.evaluation.attribution import summarize
    again = summarize(out["token_probs"], out["copy_mass"], out["answers"].ne(0))
    _bits_equal(out, again, ("share", "support", "cited"), "summarize")
    assert ((to_np(out["cited"]) >= -1) & (to_np(out["cited"]) < P)).all()


def test_host_form_agrees_with_the_kernel(tiny):
    m, b, cands, _, name = tiny
    with torch.no_grad():
        out = m.do_attribute(dict(b), answers=cands)
        with _HostForm(), Calls() as c:
            host = m.do_attribute(dict(b), answers=cands)
    assert c.count("case_copy_attribution") == 0 and c.scored >= 1
    _bits_equal(host, out, SCORE_KEYS | {"copy_pos", "copy_count", "cited", "answers"}, "host form")
    rel = max(_rel(to_np(out["copy_mass"]), to_np(host["copy_mass"])), _rel(to_np(out["copy_pos_mass"]), to_np(host["copy_pos_mass"])))
    print("%s: K39 vs the host form %.3e (bar %.1e)" % (name, rel, BAR))
    _measured("%s/kernel_vs_host_form" % name, rel, BAR)
    assert rel <= BAR


def test_unfused_chain_attributes_with_the_host_form(ns):
    """With grad enabled, or CASE_POINTER_SCORE=off, the scoring pass is the unfused differentiable chain and the attribution is the host
    form on its tensors.  The chain's mixing logits come from the GEMM, the fused pass's from the skinny kernel, so the masses are held to
    the project's fp32 bar (helpers.FP32_BAR, as tests/test_score_gpu.py holds the chain's probabilities), not to K39's."""
    from case_rg_amd import ops
    with _tiny(ns, "case-fp32") as (m, b, cands, _, _):
        with torch.no_grad():
            fused = m.do_attribute(dict(b), answers=cands)
            old, ops.POINTER_SCORE = ops.POINTER_SCORE, "off"
            try:
                with Calls() as c:
                    chain = m.do_attribute(dict(b), answers=cands)
            finally:
                ops.POINTER_SCORE = old
        assert c.scored == 0 and c.count("case_copy_attribution") == 0
        with torch.enable_grad(), Calls() as c:
            grad = m.do_attribute(dict(b), answers=cands)
        assert c.scored == 0 and c.count("case_copy_attribution") == 0 and grad["copy_mass"].requires_grad
        grad["copy_mass"].sum().backward()
        assert m.response_generation.decoder.mix.weight.grad is not None
        m.zero_grad()
        for other in (chain, grad):
            _bits_equal(other, fused, ("copy_pos", "copy_count", "cited", "answers"), "unfused chain")
            rel = _rel(to_np(other["copy_mass"].detach()), to_np(fused["copy_mass"]))
            print("unfused chain vs K39: %.3e (bar %.1e)" % (rel, FP32_BAR))
            assert rel <= FP32_BAR


def test_decoded_pools(tiny):
    m, b, _, _, name = tiny
    _, eos, _, _ = special_ids(m)
    with torch.no_grad():
        test = m.do_test(dict(b))
        out = m.do_attribute(dict(b), answers="test")
        raw = m.do_attribute(dict(b), answers="test", trim_eos=False)
        beam = m.do_attribute(dict(b), answers="beam", width=2)
        sample = m.do_attribute(dict(b), answers="sample", num_samples=3, seed=5)
        plain_sample = m.do_sample(dict(b), num_samples=3, seed=5)
    ends = test["answer"].eq(eos).long()
    trimmed = test["answer"].masked_fill((ends.cumsum(-1) - ends).gt(0), 0)
    assert torch.equal(out["answer"], test["answer"]) and torch.equal(out["rank"], test["rank"])
    assert torch.equal(out["answers"], trimmed[:, None]) and torch.equal(raw["answers"], test["answer"][:, None])
    with torch.no_grad():
        ref = m.do_score(dict(b), trimmed)
    _bits_equal(out, ref, SCORE_KEYS, "do_attribute('test') vs do_score of the trimmed answer")
    T = m.max_target_length
    assert beam["answers"].shape == (ITEMS, 2, T) and beam["cited"].shape == (ITEMS, 2) and {"beam_answers", "beam_scores", "beam_score"} <= set(beam)
    assert sample["answers"].shape == (ITEMS, 3, T) and sample["copy_mass"].shape == (ITEMS, 3, T, 1 + P) and {"samples", "sample_probs"} <= set(sample)
    assert torch.equal(sample["samples"], plain_sample["samples"]), "the pool is do_sample's at the same seed"


def test_evaluate_attribution_is_predict_plus_torch(tiny, ns):
    m, b, _, cpu, name = tiny
    trainer = ns.CumulativeTrainer(m, None, None, None, 1)
    try:
        got = trainer.evaluate_attribution(cases._ListDataset(cpu), cases._collate, 3)  # batches of 3 and 1 items
        assert not trainer.model.training, "the mode must be restored"
        hit = agree = items = tokens = 0
        sums = np.zeros(3)
        with torch.no_grad():
            for lo, hi in ((0, 3), (3, ITEMS)):
                data = {k: v[lo:hi].cuda() for k, v in cpu.items()}
                out = {k: v.cpu() for k, v in trainer.model.do_attribute(data).items() if torch.is_tensor(v)}
                cited, label = out["cited"][:, 0].numpy(), cpu["passage_label"][lo:hi].numpy()
                top = np.array([int(np.flatnonzero(row == row.max())[0]) for row in out["rank"].numpy()])
                scored = (out["answers"][:, 0] != 0).numpy()
                share = out["share"][:, 0].double().numpy() * scored[..., None]
                hit, agree, items, tokens = hit + int((cited == label).sum()), agree + int((cited == top).sum()), items + (hi - lo), tokens + int(scored.sum())
                sums += [share[..., 0].sum(), share[..., 1].sum(), share[..., 2:].sum()]
    finally:
        trainer.close()
    print("evaluate_attribution(%s): %s" % (name, got))
    assert set(got) == {"cited_accuracy", "rank_agreement", "gen_share", "context_share", "passage_share", "items", "tokens"}
    assert got["items"] == items == ITEMS and got["tokens"] == tokens > 0
    assert got["cited_accuracy"] == hit / items and got["rank_agreement"] == agree / items
    for key, want in zip(("gen_share", "context_share", "passage_share"), sums / tokens):
        assert abs(got[key] - want) <= 1e-6, (key, got[key], want)
    assert abs(got["gen_share"] + got["context_share"] + got["passage_share"] - 1.0) <= 1e-5


def test_attribution_pass_replays_from_a_captured_graph(ns):
    with _tiny(ns, "case-bf16") as (m, b, _, _, _), torch.no_grad():
        eager = {k: v.clone() for k, v in m.do_attribute(dict(b), answers="response").items()}
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.do_attribute(dict(b), answers="response")  # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        graph, static = torch.cuda.CUDAGraph(), {}
        with torch.cuda.graph(graph), Calls() as c:
            static.update(m.do_attribute(dict(b), answers="response"))
        assert c.count("case_copy_attribution") == 1
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            for k in eager:
                assert torch.equal(static[k], eager[k]), "the replay differs from the eager pass in %s" % k
        del graph
