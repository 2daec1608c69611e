"""Beam search, CPU side: a plain-Python restatement of the selection rule (the reference's common/Generations.py ``beam``: width,
length-normalised cost, EOS retirement), driven by the CPU oracle's step distributions, must reproduce the fixtures the reference's own
``beam`` produced (tests/golden/gen_beam_golden.py).  That pins the restatement, which tests/test_beam_gpu.py then holds the kernels to.

Ids are exact on decisive items (every deciding comparison of the item has a relative gap above beam_cases.GAP in the reference's run);
costs are held to the oracle bar of tests/test_oracle_vs_golden.py, 2e-5."""
import math

import numpy as np
import pytest
import torch

import beam_cases
from helpers import load_golden

INF = float("inf")


def rel_gap(a, b):
    """|a - b| relative to the larger magnitude; 0 for two equal values (an exact tie is decided by order, not by arithmetic)."""
    if a == b:
        return 0.0
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def top_candidates(row, width):
    """The ``width`` most probable tokens of a distribution row, descending, the lowest id first among equals -> ([(p, id)], gap to the next)."""
    row = np.asarray(row, dtype=np.float64)
    order = np.argsort(-row, kind="stable")[:width + 1]
    gap = rel_gap(row[order[width - 1]], row[order[width]]) if len(order) > width else INF
    return [(float(row[i]), int(i)) for i in order[:width]], gap


def advance(cands, alive, cum, length, t, T, eos, width):
    """One step of the search for one item.  cands[w] = the [(p, id)] of slot w; alive / cum / length per slot.
    -> (slots, retired, gap): ``slots`` = ``width`` dicts (parent, token, cum, len, key, alive; ``None`` for an empty slot) in rank order,
    ``retired`` = [(key, slot)] in rank order, ``gap`` = the relative gap between the last kept and the first dropped key."""
    children = []
    for w in range(width):
        if not alive[w]:
            continue
        for p, tok in cands[w]:
            c = cum[w] + -math.log(p + 1e-10)
            children.append(dict(parent=w, token=tok, cum=c, len=length[w] + 1, key=c / (length[w] + 1)))
    ranked = sorted(children, key=lambda n: n["key"])  # stable over (parent slot, candidate rank)
    gap = rel_gap(ranked[width - 1]["key"], ranked[width]["key"]) if len(ranked) > width else INF
    slots, retired = [], []
    for r in range(width):
        n = ranked[r] if r < len(ranked) else None
        if n is not None:
            n["alive"] = not (n["token"] == eos or t == T - 1)
            if not n["alive"]:
                retired.append((n["key"], r))
        slots.append(n)
    return slots, retired, gap


def pool_insert(pool, entry, width):
    """The finished pool: ascending by key, a newcomer behind its equals, at most ``width`` entries."""
    at = 0
    while at < len(pool) and pool[at][0] <= entry[0]:
        at += 1
    pool.insert(at, entry)
    del pool[width:]


def backtrack(history, step, slot, T):
    """history[s] = the slots of step s; the tokens of the hypothesis that retired as ``slot`` of ``step``, PAD behind them."""
    out = [0] * T
    for s in range(step, -1, -1):
        out[s] = history[s][slot]["token"]
        slot = history[s][slot]["parent"]
    return out


def beam_search(step_fn, items, width, T, bos, eos, slot_fn=None):
    """step_fn(rows, prefixes int64 [n, L]) -> distributions [n, V] (or slot_fn(t, [(item, slot)]) for a caller that keeps the rows of a
    recorded run).  Per item: dict(answers=[[T ids]] best first, scores=[key], gap=the smallest deciding gap, eos_before_last=bool)."""
    alive = [[w == 0 for w in range(width)] for _ in range(items)]
    cum = [[0.0] * width for _ in range(items)]
    length = [[1] * width for _ in range(items)]
    prefix = [[[bos] for _ in range(width)] for _ in range(items)]
    history = [[] for _ in range(items)]
    pools = [[] for _ in range(items)]
    gaps = [INF] * items
    early = [False] * items
    for t in range(T):
        live = [(b, w) for b in range(items) for w in range(width) if alive[b][w]]
        if not live:
            break
        if slot_fn is not None:
            dists = slot_fn(t, live)
        else:
            dists = step_fn([b for b, _ in live], torch.tensor([prefix[b][w] for b, w in live], dtype=torch.long))
        dists = dists.detach().double().cpu().numpy()
        cands = [[None] * width for _ in range(items)]
        for (b, w), row in zip(live, dists):
            cands[b][w], g = top_candidates(row, width)
            gaps[b] = min(gaps[b], g)
        for b in range(items):
            if not any(alive[b]):
                continue
            slots, retired, g = advance(cands[b], alive[b], cum[b], length[b], t, T, eos, width)
            gaps[b] = min(gaps[b], g)
            history[b].append(slots)
            for key, r in retired:
                pool_insert(pools[b], (key, t, r), width)
                early[b] = early[b] or t < T - 1
            prefix[b] = [prefix[b][n["parent"]] + [n["token"]] if n else [bos] for n in slots]
            alive[b] = [bool(n and n["alive"]) for n in slots]
            cum[b] = [n["cum"] if n else INF for n in slots]
            length[b] = [n["len"] if n else 0 for n in slots]
    out = []
    for b in range(items):
        pool = pools[b]
        if len(pool) > 1:
            gaps[b] = min(gaps[b], rel_gap(pool[0][0], pool[1][0]))
        out.append(dict(answers=[backtrack(history[b], s, r, T) for _, s, r in pool], scores=[k for k, _, _ in pool], gap=gaps[b],
                        eos_before_last=early[b]))
    return out


def pack(results, width, T):
    """The restatement's results as the arrays the product returns: answer [B, T], beam_answers [B, W, T], beam_scores [B, W], gap [B]."""
    B = len(results)
    answers = np.zeros((B, width, T), dtype=np.int64)
    scores = np.full((B, width), np.inf, dtype=np.float64)
    for b, r in enumerate(results):
        for k, (a, s) in enumerate(zip(r["answers"], r["scores"])):
            answers[b, k], scores[b, k] = a, s
    return dict(answer=answers[:, 0].copy(), beam_answers=answers, beam_scores=scores, gap=np.array([r["gap"] for r in results]))


def cut_at_eos(ids, eos):
    ids = [int(i) for i in ids]
    return ids[:ids.index(eos) + 1] if eos in ids else ids


# ---------------------------------------------------------------------------------------------
def _oracle_ns():
    import types
    import oracle
    return types.SimpleNamespace(**{k: v for k, v in vars(oracle).items() if not k.startswith("_")})


def test_selection_rule_on_hand_made_candidates():
    """Stable order on exact ties, dead slots, EOS retirement, the last step, the pool's order."""
    W, T, EOS = 2, 3, 9
    cands = [[(0.5, 4), (0.25, EOS)], [(0.5, 7), (0.5, 8)]]
    slots, retired, gap = advance(cands, [True, False], [0.0, 0.0], [1, 1], 0, T, EOS, W)
    assert [(n["parent"], n["token"], n["alive"]) for n in slots] == [(0, 4, True), (0, EOS, False)] and retired == [(-math.log(0.25 + 1e-10) / 2, 1)]
    assert gap == INF  # the dead slot's candidates do not compete
    slots, retired, gap = advance(cands, [True, True], [0.0, 0.0], [1, 1], 0, T, EOS, W)
    assert [(n["parent"], n["token"]) for n in slots] == [(0, 4), (1, 7)] and gap == 0.0  # three equal keys: (slot, rank) order decides
    slots, retired, _ = advance(cands, [True, True], [0.0, 0.0], [1, 1], T - 1, T, EOS, W)
    assert [n["alive"] for n in slots] == [False, False] and [r for _, r in retired] == [0, 1]
    pool = []
    for e in [(2.0, 0, 0), (1.0, 1, 0), (2.0, 1, 1), (1.0, 2, 1)]:
        pool_insert(pool, e, 3)
    assert pool == [(1.0, 1, 0), (1.0, 2, 1), (2.0, 0, 0)]
    assert top_candidates([0.1, 0.4, 0.4, 0.1], 2)[0] == [(0.4, 1), (0.4, 2)]


@pytest.mark.parametrize("width", beam_cases.WIDTHS)
@pytest.mark.parametrize("name", list(beam_cases.BEAM_CASES))
def test_restatement_on_the_oracle_reproduces_the_reference_beam(name, width):
    golden = load_golden("%s_w%d" % (name, width))
    ns = _oracle_ns()
    m, b = beam_cases.build(ns, torch.device("cpu"), name)
    for k in ("query", "passage", "source_map"):
        assert np.array_equal(b[k].numpy(), golden["in_" + k]), "regenerated inputs must be the committed inputs"
    model = beam_cases.BEAM_CASES[name][0]
    bos, eos = int(golden["bos"]), int(golden["eos"])
    got = pack(beam_search(lambda rows, pre: beam_cases.step_dists(ns, m, b, model, rows, pre), beam_cases.ITEMS, width, beam_cases.T, bos, eos),
               width, beam_cases.T)
    decisive = golden["gap"] > beam_cases.GAP
    assert decisive.sum() * 2 >= decisive.size, "the fixture must keep at least half its items decisive"
    for i in np.nonzero(decisive)[0]:
        assert np.array_equal(got["answer"][i], golden["answer"][i]), "%s item %d: %s != reference %s" % (name, i, got["answer"][i], golden["answer"][i])
        assert abs(got["beam_scores"][i, 0] - golden["score"][i]) <= 2e-5 * abs(golden["score"][i]) + 2e-6, \
            "%s item %d: cost %.8f, reference %.8f" % (name, i, got["beam_scores"][i, 0], golden["score"][i])
