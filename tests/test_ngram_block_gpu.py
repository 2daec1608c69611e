"""The n-gram ban (K32) on the MI355X.

Operator level, exact: K23 / K24 / K28 with the ban against the SAME kernels' ban-off distribution row with the entries zeroed that the
pure-Python restatement of the rule lists (``Utils.banned_tokens``, pinned by tests/test_ngram_block_cpu.py) -- ids, candidates,
probabilities and the returned row bit for bit -- and ``ops.ngram_ban_`` on random rows; the flat beam history of K25 against a walk of
``hist_parent`` / ``hist_token``.

Pass level, fp32: greedy, beam and sampled passes of both task models never repeat an n-gram, every emitted token is (within ``tol``) the
best token the ban allows under the teacher-forced distribution of its prefix, ban-off calls are unchanged, and a pass still captures.
``tol`` is measured here: 10 x the largest |cached step - teacher-forced| probability of the same fixtures with the ban off (one f32 row
build against a differently ordered one); the measurement goes to profiles/ngram_parity.json."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import FP32_BAR, Calls, special_ids, to_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ban(history, n, V, eos):
    from case_rg_amd.common.Utils import banned_tokens
    return banned_tokens(history, n, V, eos)


# ---------------------------------------------------------------------------------------------
# 1. the three heads and the stand-alone launch, exact
# ---------------------------------------------------------------------------------------------
R, LENS, TMAX, EOS_ID, W = 5, (8, 36), 24, 7, 4
ALPHABET = (11, 12, 13, 14)  # the histories' words: among the 12 source words and among the most probable tokens of every row


def _inputs(V, seed):
    from case_rg_amd import ops
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(R, V, generator=g) * 2.0
    logits[:, list(ALPHABET)] += 7.0  # the banned candidates are the rows' largest entries: a ban changes the selection
    logits[:, [20, 21, 22]] += 5.0
    logits[0, ALPHABET[0]] = logits[0].max() + 3.0  # rows 0 and 1: the argmax is the word their periodic histories ban (see _histories)
    logits[1, ALPHABET[1]] = logits[1].max() + 3.0
    words = torch.tensor(list(ALPHABET) + [20, 21, 22, 30, 31, V - 1, V - 2, 40])  # 12 source words: pointer runs exist
    src = words[torch.randint(0, 12, (R, sum(LENS)), generator=g)]
    mix = torch.randn(R, 1 + len(LENS), generator=g)
    mix[:2, 0] = 3.0  # (the generator's share of rows 0 and 1 outweighs any pointer mass)
    copies = [torch.softmax(torch.randn(R, n, generator=g) * 2.0, dim=-1) for n in LENS]
    dev = torch.device("cuda")
    return logits.to(dev), mix.to(dev), ops.SortedSource(src.to(dev), V), [c.to(dev) for c in copies]


def _histories(V, t, seed):
    """int32 [R, TMAX]: t tokens over the 4-word alphabet (many windows match): row 0 one word repeated, row 1 two words alternating, the rest
    random; row 3 carries EOS, row 4 an id >= V; garbage behind t."""
    rng = np.random.RandomState(seed)
    h = rng.randint(0, 4, size=(R, TMAX))
    h[0] = 0
    h[1] = np.arange(TMAX) % 2
    h = np.asarray(ALPHABET)[h]
    h[:, t:] = ALPHABET[0]  # must not be read
    if t >= 1:
        h[3, rng.randint(0, t)] = EOS_ID
        h[4, t - 1 if t < 3 else t - 3] = V + 5
    return h.astype(np.int32)


def _zeroed(dist, hist, t, n, V, eos, skip=()):
    out = dist.copy()
    lists = []
    for r in range(R):
        banned = [] if r in skip else _ban(hist[r, :t].tolist(), n, V, eos)
        out[r, banned] = 0.0
        lists.append(banned)
    return out, lists


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("V", [203, 2051])
def test_heads_with_the_ban_equal_the_zeroed_row_bit_for_bit(V, n):
    from case_rg_amd import ops
    logits, mix, sm, copies = _inputs(V, 40 + V)
    _, base, base_ids = ops.pointer_head_decode(logits, mix, sm, copies, want_gen=False, want_dist=True)
    base = to_np(base)
    uniforms = torch.tensor([0.03, 0.31, 0.55, 0.78, 0.97], dtype=torch.float32, device="cuda")
    changed = 0
    for t in sorted({0, 1, n - 1, n, 17}):
        hist = _histories(V, t, 7 * t + n)
        want_row, lists = _zeroed(base, hist, t, n, V, EOS_ID)
        assert lists[3] == [] or t == 0, "the EOS row must not be banned"
        if t >= n:
            assert lists[0] == [ALPHABET[0]] and all(V + 5 not in b for b in lists)
        if t == 17:
            assert ALPHABET[1] in lists[1], "t 17: row 1 is not banned: %s" % lists
        # K23: argmax with the lowest index on ties
        h = torch.from_numpy(hist).cuda()
        with Calls() as c:
            gen, dist, ids = ops.pointer_head_decode(logits, mix, sm, copies, want_gen=True, want_dist=True, ban=(h, t, n, EOS_ID))
        assert c.count("case_pointer_head_decode_ban") == 1 and c.count("case_pointer_head_decode") == 0
        want_ids = [int(np.flatnonzero(row == row.max())[0]) for row in want_row]
        assert to_np(ids).tolist() == want_ids, "K23 t %d: %s, want %s" % (t, to_np(ids).tolist(), want_ids)
        assert _same_bits(to_np(dist), want_row), "K23 t %d: the returned row is not the zeroed row" % t
        got_h = to_np(h)
        assert got_h[:, t].tolist() == want_ids and np.array_equal(np.delete(got_h, t, axis=1), np.delete(hist, t, axis=1)), "K23 t %d: history" % t
        gen0, _, _ = ops.pointer_head_decode(logits, mix, sm, copies, want_gen=True, want_dist=False)
        assert torch.equal(gen, gen0), "gen must be untouched"
        changed += sum(a != b for a, b in zip(want_ids, to_np(base_ids).tolist()))
        # K24: the W largest by (p descending, id ascending)
        h = torch.from_numpy(hist).cuda()
        _, dist, cand_p, cand_id = ops.pointer_head_topk(logits, mix, sm, copies, W, want_dist=True, ban=(h, t, n, EOS_ID))
        order = [np.lexsort((np.arange(V), -row.astype(np.float64)))[:W] for row in want_row]
        assert to_np(cand_id).tolist() == [o.tolist() for o in order], "K24 t %d" % t
        assert _same_bits(to_np(cand_p), np.stack([row[o] for row, o in zip(want_row, order)])) and _same_bits(to_np(dist), want_row)
        assert np.array_equal(to_np(h), hist), "K24 only reads the history"
        # K28: the ban-off kernel fed the zeroed row; row 2 has ended (no ban there)
        want_s, _ = _zeroed(base, hist, t, n, V, EOS_ID, skip=(2,))
        fed = torch.from_numpy(want_s).cuda()
        for temperature, top_k, top_p in ((0.7, 5, 0.9), (1.0, 0, 1.0)):
            draw = (False, False, EOS_ID, 3, 0, temperature, top_k, top_p)
            ended = torch.tensor([0, 0, 1, 0, 0], dtype=torch.uint8, device="cuda")
            e_ref, e_fused, e_in = ended.clone(), ended.clone(), ended.clone()
            _, d_ref, id_ref, p_ref = ops.pointer_head_sample(None, None, None, None, e_ref, *draw, uniforms=uniforms, dist_in=fed, want_dist=True)
            for source, e in (("fused", e_fused), ("dist_in", e_in)):
                h = torch.from_numpy(hist).cuda()
                if source == "fused":
                    head = (logits, mix, sm, copies)
                    kw = {}
                else:
                    head, kw = (None, None, None, None), {"dist_in": torch.from_numpy(base).cuda()}
                with Calls() as c:
                    _, d, ids, p = ops.pointer_head_sample(*head, e, *draw, uniforms=uniforms, want_dist=True, ban=(h, t, n), **kw)
                assert c.count("case_pointer_head_sample_ban") == 1 and c.sampled == 0
                what = "K28 %s t %d tau %s" % (source, t, temperature)
                assert torch.equal(ids, id_ref) and _same_bits(to_np(p), to_np(p_ref)), what
                assert _same_bits(to_np(d), to_np(d_ref)) and _same_bits(to_np(d), want_s) and torch.equal(e, e_ref), what
                assert to_np(h)[:, t].tolist() == to_np(ids).tolist(), what + ": history"
    assert changed >= 3, "the ban changed %d argmaxes (row 0 at t = n and t = 17, row 1 at t = 17 by construction)" % changed


@pytest.mark.parametrize("V", [203, 2051])
def test_ngram_ban_on_random_rows(V):
    from case_rg_amd import ops
    g = torch.Generator().manual_seed(V)
    base = torch.rand(R, V, generator=g)
    ended = torch.tensor([0, 1, 0, 0, 0], dtype=torch.uint8, device="cuda")
    for n in (1, 2, 3):
        for t in sorted({0, 1, n - 1, n, 17}):
            hist = _histories(V, t, 3 * t + n)
            for flags, skip in ((None, ()), (ended, (1,))):
                want, _ = _zeroed(base.numpy(), hist, t, n, V, EOS_ID, skip=skip)
                d = base.clone().cuda()
                out = ops.ngram_ban_(d, torch.from_numpy(hist).cuda(), t, n, eos=EOS_ID, ended=flags)
                assert out.data_ptr() == d.data_ptr() and _same_bits(to_np(d), want), "n %d t %d" % (n, t)
            want, lists = _zeroed(base.numpy(), hist, t, n, V, None)  # no EOS id: row 3 is banned like the others
            d = base.clone().cuda()
            ops.ngram_ban_(d, torch.from_numpy(hist).cuda(), t, n)
            assert _same_bits(to_np(d), want) and (n > 1 or t < 1 or EOS_ID in lists[3]), "no EOS id: n %d t %d" % (n, t)
    with pytest.raises(ValueError):
        ops.ngram_ban_(base.clone().cuda(), torch.zeros(R, TMAX, dtype=torch.int32, device="cuda"), TMAX, 2)
    with pytest.raises(TypeError):
        ops.ngram_ban_(base.clone().cuda(), torch.zeros(R, TMAX, dtype=torch.int64, device="cuda"), 3, 2)


def test_a_history_of_256_tokens_and_a_vocabulary_at_the_lds_limit():
    """t = 256 is the staging bound; V = 36 000 the row bound: the ban must fit beside it without more LDS."""
    from case_rg_amd import ops
    V, T, n = 36000, 257, 3
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(2, V, generator=g)).cuda()
    mix = torch.randn(2, 2, generator=g).cuda()
    src = torch.randint(0, V, (2, 16), generator=g)
    sm = ops.SortedSource(src.cuda(), V)
    copies = [torch.softmax(torch.randn(2, 16, generator=g), dim=-1).cuda()]
    hist = np.random.RandomState(3).randint(V - 3, V, size=(2, T)).astype(np.int32)
    _, base, _ = ops.pointer_head_decode(logits, mix, sm, copies, want_gen=False, want_dist=True)
    h = torch.from_numpy(hist).cuda()
    _, dist, ids = ops.pointer_head_decode(logits, mix, sm, copies, want_gen=False, want_dist=True, ban=(h, 256, n, None))
    want = to_np(base).copy()
    for r in range(2):
        banned = _ban(hist[r, :256].tolist(), n, V, None)
        assert banned
        want[r, banned] = 0.0
    assert _same_bits(to_np(dist), want) and to_np(h)[:, 256].tolist() == to_np(ids).tolist()


# ---------------------------------------------------------------------------------------------
# 2. the flat beam history
# ---------------------------------------------------------------------------------------------
def test_flat_beam_history_is_the_walk_of_the_parents():
    from case_rg_amd import ops
    B, Wb, T, steps, V = 2, 3, 8, 6, 50
    rng = np.random.RandomState(12)
    state = ops.BeamState(B, Wb, T, torch.device("cuda"), flat=True)
    plain = ops.BeamState(B, Wb, T, torch.device("cuda"))
    permuted = 0
    for t in range(steps):
        cand_p = torch.from_numpy(rng.uniform(0.05, 0.9, size=(B * Wb, Wb)).astype(np.float32)).sort(dim=1, descending=True)[0].cuda()
        cand_id = torch.from_numpy(rng.randint(4, V, size=(B * Wb, Wb))).cuda()
        with Calls() as c:
            ops.beam_advance(state, cand_p, cand_id, t, 2)
            ops.beam_advance(plain, cand_p, cand_id, t, 2)
        assert c.count("case_beam_advance_ban") == 1 and c.count("case_beam_advance") == 1
        for k in ("alive", "cum", "len", "parent", "token", "hist_parent", "hist_token", "fin_key", "fin_step", "fin_slot"):
            assert torch.equal(getattr(state, k), getattr(plain, k)), "%s differs with the flat history at step %d" % (k, t)
        hp, ht = to_np(state.hist_parent), to_np(state.hist_token)
        flat = to_np(state.flat_rows(t + 1)).reshape(B, Wb, T)
        for b in range(B):
            for w in range(Wb):
                toks, slot = [], w
                for s in range(t, -1, -1):
                    toks.append(int(ht[s, b, slot]))
                    slot = int(hp[s, b, slot])
                assert flat[b, w, :t + 1].tolist() == toks[::-1], "step %d item %d slot %d: %s, walk %s" % (t, b, w, flat[b, w], toks[::-1])
            parents = hp[t, b].tolist()
            permuted += t > 0 and (parents != sorted(parents) or len(set(parents)) < Wb)
    assert permuted >= 3, "the crafted candidates never permute the slots"
    # a candidate of probability 0 is dead with the flat history: it takes no slot
    state = ops.BeamState(1, 2, 4, torch.device("cuda"), flat=True)
    ops.beam_advance(state, torch.tensor([[0.5, 0.0], [0.0, 0.0]], device="cuda"), torch.tensor([[5, 6], [7, 8]], device="cuda"), 0, 2)
    assert to_np(state.alive).tolist() == [[1, 0]] and to_np(state.token).tolist() == [[5, 0]]


# ---------------------------------------------------------------------------------------------
# 3. whole passes
# ---------------------------------------------------------------------------------------------
V_, H_, T_, ITEMS = 200, 32, 24, 4
# (model seed, batch seed): the ban-off answers of these hold a repeated trigram before EOS, and their ban-off fused and unfused beam passes
# agree exactly (both asserted below)
SEEDS = {"case": (153, 152), "masque": (153, 152)}


@pytest.fixture(scope="module")
def ns():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.float32)
    case_rg_amd.set_dropout(False)
    return case_rg_amd.namespace()


@pytest.fixture(scope="module")
def fixtures(ns):
    """kind -> (model in eval mode, batch on the device), built as in test_greedy_early_stop_and_graph_replay and left unchanged."""
    from case_rg_amd.utils import fill_params, make_vocab, synth_batch
    v2i, i2v = make_vocab(V_)
    out = {}
    for kind, (mseed, bseed) in SEEDS.items():
        model = ns.CaSE(4, T_, i2v, v2i, H_) if kind == "case" else ns.Masque(T_, i2v, v2i, H_)
        model = fill_params(model, mseed, gain=3.0).cuda().eval()
        out[kind] = (model, {k: v.cuda() for k, v in synth_batch(ITEMS, 3, 12, 8, 6, V_, seed=bseed, model=kind).items()})
    return out


class _Unfused:
    def __enter__(self):
        from case_rg_amd import ops
        self.old, ops.POINTER_HEAD = ops.POINTER_HEAD, "off"

    def __exit__(self, *exc):
        from case_rg_amd import ops
        ops.POINTER_HEAD = self.old


def _before_eos(row, eos):
    row = [int(x) for x in row]
    return row[:row.index(eos)] if eos in row else row


def _repeats(tokens, n):
    grams = [tuple(tokens[i:i + n]) for i in range(len(tokens) - n + 1)]
    return len(grams) - len(set(grams))


class _Grabbed(Exception):
    pass


def _teacher_forced(m, b, answers):
    """The decoder's full-prefix training-form path (``_run_prefix`` + ``_head``) in eval mode on dec_ids = [BOS, answers[:, :-1]]:
    answers int64 [B * n, T] (the rows of an item consecutive) -> f64 [B * n, T, V], position t = the distribution behind answers[:, :t]."""
    dec = m.response_generation.decoder
    seen = {}

    def grab(*a, **kw):
        seen["a"], seen["kw"] = a, kw
        raise _Grabbed()

    dec._run = grab
    try:
        with torch.no_grad():
            m.do_test(dict(b))
    except _Grabbed:
        pass
    finally:
        del dec._run
    memories, masks, weights, source_map, BOS = seen["a"][:5]
    feature_of = seen["kw"].get("feature_of")
    B, H = source_map.size(0), dec.hidden_size
    n, T = answers.shape[0] // B, answers.shape[1]
    with torch.no_grad():
        mems = [x.reshape(B, -1, H) for x in memories]
        valid = [x.reshape(B, -1).contiguous() for x in masks]
        weights = [w.reshape(B, -1) for w in weights]
        feat = None if feature_of is None else feature_of(T)
        mems, valid, weights, source_map, feat = dec._per_item(n, mems, valid, weights, dec._sorted(source_map), feat)
        dec_ids = torch.cat([dec._bos(B * n, BOS, answers.device), answers[:, :-1]], dim=-1)
        _, _, dist = dec._head(*dec._run_prefix(dec_ids, mems, valid, weights, feat), feat, source_map)
    return dist.double().cpu().numpy()


def _drawn(samples, unk, pad):
    """Where ``sample_probs`` is the probability of the emitted token (tests/test_score_gpu.py ``_drawn_positions``)."""
    keep = samples != pad
    keep[..., -1] = False
    keep[..., 0] &= samples[..., 0] != unk
    return keep


def _uniforms(rows, seed=31):
    return torch.from_numpy(np.random.RandomState(seed).uniform(0.0, 1.0, size=(T_, rows)).astype(np.float32)).cuda()


@pytest.fixture(scope="module")
def tol(fixtures):
    """10 x the largest |cached step - teacher-forced| probability with the ban OFF: the probabilities a sampled pass recorded for its
    drawn tokens (K28's row entry, the entry K23 and K24 select from) against the teacher-forced pass over the same ids, on both fixtures."""
    worst = {}
    for kind, (m, b) in fixtures.items():
        _, eos, unk, pad = special_ids(m)
        with torch.no_grad():
            drawn = m.do_sample(dict(b), num_samples=3, uniforms=_uniforms(ITEMS * 3))
        samples = to_np(drawn["samples"]).reshape(ITEMS * 3, T_)
        P = _teacher_forced(m, b, torch.from_numpy(samples).cuda())
        keep = _drawn(samples, unk, pad)
        got = to_np(drawn["sample_probs"]).reshape(ITEMS * 3, T_).astype(np.float64)
        want = np.take_along_axis(P, samples[..., None], axis=2)[..., 0]
        worst[kind + "/sample_probs"] = float(np.abs(got - want)[keep].max())
    measured = max(worst.values())
    path = os.path.join(ROOT, "profiles", "ngram_parity.json")
    record = {"what": "largest |cached-step probability - teacher-forced probability| with the ban off (fp32, V 200, hidden 32, T 24, batch 4)",
              "measured": {k: float("%.3e" % v) for k, v in sorted(worst.items())}, "tol": float("%.3e" % (10 * measured)), "tol_rule": "10 x the largest"}
    with open(path, "w") as fh:
        json.dump(record, fh, indent=1, sort_keys=True)
    print("ngram parity: %s -> tol %.3e" % (worst, 10 * measured))
    assert 0.0 < measured <= FP32_BAR, "the ban-off cached step is %.3e from the teacher-forced pass" % measured
    return 10 * measured


def _check_allowed_best(P, rows, n, eos, tol, what):
    """Every emitted token before EOS (EOS itself included) is not banned and is, within tol, the largest entry the ban leaves."""
    V = P.shape[2]
    checked = 0
    for r, row in enumerate(rows):
        row = [int(x) for x in row]
        end = row.index(eos) + 1 if eos in row else len(row)
        for t in range(end):
            banned = _ban(row[:t], n, V, None)
            assert row[t] not in banned, "%s row %d step %d: token %d is banned (%s)" % (what, r, t, row[t], row)
            masked = P[r, t].copy()
            masked[banned] = 0.0
            assert P[r, t, row[t]] >= masked.max() - tol, "%s row %d step %d: p %.6g, best allowed %.6g" % (what, r, t, P[r, t, row[t]], masked.max())
            checked += 1
    return checked


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_ban_off_answers_loop(fixtures, kind):
    """The fixtures exercise the ban: the ban-off greedy, beam and sampled answers repeat trigrams (bigrams) before EOS."""
    m, b = fixtures[kind]
    _, eos, _, _ = special_ids(m)
    with torch.no_grad():
        greedy = to_np(m.do_test(dict(b))["answer"])
        beam = to_np(m.do_beam(dict(b), width=3)["beam_answers"])
        drawn = to_np(m.do_sample(dict(b), num_samples=3, uniforms=_uniforms(ITEMS * 3))["samples"])
    assert sum(_repeats(_before_eos(r, eos), 3) > 0 for r in greedy) >= 1, greedy
    assert sum(_repeats(_before_eos(r, eos), 1) > 0 for r in greedy) >= 1
    assert sum(_repeats(_before_eos(r, eos), 3) > 0 for r in beam.reshape(-1, T_)) >= 1, beam
    assert sum(_repeats(_before_eos(r, eos), 2) > 0 for r in drawn.reshape(-1, T_)) >= 1, drawn


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("kind", ["case", "masque"])
def test_greedy_pass(fixtures, tol, kind, n):
    m, b = fixtures[kind]
    _, eos, _, _ = special_ids(m)
    with torch.no_grad(), Calls() as c:
        out = m.do_test(dict(b), no_repeat_ngram=n)
    assert c.count("case_pointer_head_decode_ban") == T_ and c.count("case_pointer_head_decode") == 0 and c.count("case_ngram_ban") == 0
    answer = to_np(out["answer"])
    for r, row in enumerate(answer):
        assert _repeats(_before_eos(row, eos), n) == 0, "row %d repeats a %d-gram: %s" % (r, n, row)
    P = _teacher_forced(m, b, out["answer"])
    assert _check_allowed_best(P, answer, n, eos, tol, "greedy n %d" % n) >= ITEMS
    m.no_repeat_ngram = n  # the attribute is what model(data, method=...) uses
    try:
        with torch.no_grad():
            assert torch.equal(m(dict(b), method="test")["answer"], out["answer"])
        with _Unfused(), torch.no_grad(), Calls() as c:
            unfused = m(dict(b), method="test")["answer"]
        assert c.count("case_ngram_ban") == T_ and c.count("case_pointer_head_decode_ban") == 0
    finally:
        m.no_repeat_ngram = 0
    for r, row in enumerate(to_np(unfused)):
        assert _repeats(_before_eos(row, eos), n) == 0, "unfused row %d repeats a %d-gram: %s" % (r, n, row)
    assert _check_allowed_best(P if torch.equal(unfused, out["answer"]) else _teacher_forced(m, b, unfused), to_np(unfused), n, eos, tol, "unfused greedy") >= ITEMS


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_beam_pass(fixtures, kind):
    from test_score_gpu import _beam_costs, _rel
    m, b = fixtures[kind]
    _, eos, _, _ = special_ids(m)
    n, width = 3, 3
    with torch.no_grad():
        off_fused = m.do_beam(dict(b), width=width)
        with _Unfused():
            off_unfused = m.do_beam(dict(b), width=width)
    assert torch.equal(off_fused["beam_answers"], off_unfused["beam_answers"]), "ban off: the fused and unfused beams differ on these seeds"
    with torch.no_grad(), Calls() as c:
        out = m.do_beam(dict(b), width=width, no_repeat_ngram=n)
        rescored = m.do_score(dict(b), out["beam_answers"])
    assert c.count("case_pointer_head_beam_ban") >= 2 and c.count("case_beam_advance_ban") == c.count("case_pointer_head_beam_ban")
    assert c.count("case_pointer_head_beam") == 0 and c.count("case_beam_advance") == 0
    answers, scores = to_np(out["beam_answers"]), to_np(out["beam_scores"]).astype(np.float64)
    assert np.isfinite(scores).sum() >= ITEMS
    for i in range(ITEMS):
        for k in range(width):
            if np.isfinite(scores[i, k]):
                assert _repeats(_before_eos(answers[i, k], eos), n) == 0, "item %d entry %d repeats a trigram: %s" % (i, k, answers[i, k])
    cost, usable = _beam_costs(to_np(rescored["token_probs"]).astype(np.float64), answers, eos)
    fin = np.isfinite(scores) & usable
    assert fin.sum() >= ITEMS
    rel = _rel(cost[fin], scores[fin])
    print("%s: banned beam costs vs rescoring over %d hypotheses: %.3e" % (kind, fin.sum(), rel))
    assert rel <= FP32_BAR
    with _Unfused(), torch.no_grad(), Calls() as c:
        unfused = m.do_beam(dict(b), width=width, no_repeat_ngram=n)
    assert c.count("case_ngram_ban") >= 2 and c.count("case_pointer_head_beam_ban") == 0
    assert torch.equal(unfused["beam_answers"], out["beam_answers"]), "fused and unfused beams differ with the ban on"
    # W = 1 is greedy decoding, ban included: equal up to and including the first EOS, where the beam hypothesis retires
    with torch.no_grad():
        one = to_np(m.do_beam(dict(b), width=1, no_repeat_ngram=n)["answer"])
        greedy = to_np(m.do_test(dict(b), no_repeat_ngram=n)["answer"])
    for i in range(ITEMS):
        want = [int(x) for x in greedy[i]]
        want = want[:want.index(eos) + 1] if eos in want else want
        assert one[i, :len(want)].tolist() == want and not one[i, len(want):].any(), "item %d: beam %s, greedy %s" % (i, one[i], greedy[i])


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_sampled_pass(fixtures, tol, kind):
    m, b = fixtures[kind]
    _, eos, unk, pad = special_ids(m)
    n, N = 2, 3
    u = _uniforms(ITEMS * N)
    with torch.no_grad(), Calls() as c:
        out = m.do_sample(dict(b), num_samples=N, uniforms=u, no_repeat_ngram=n)
        again = m.do_sample(dict(b), num_samples=N, uniforms=u, no_repeat_ngram=n)
    assert c.count("case_pointer_head_sample_ban") == 2 * T_ and c.sampled == 0
    for k in ("samples", "sample_probs", "sample_scores"):
        assert torch.equal(out[k], again[k]), "%s differs between two passes" % k
    samples = to_np(out["samples"]).reshape(ITEMS * N, T_)
    for r, row in enumerate(samples):
        assert _repeats(_before_eos(row, eos), n) == 0, "row %d repeats a bigram: %s" % (r, row)
    P = _teacher_forced(m, b, torch.from_numpy(samples).cuda())
    keep = _drawn(samples, unk, pad)
    got = to_np(out["sample_probs"]).reshape(ITEMS * N, T_).astype(np.float64)
    want = np.take_along_axis(P, samples[..., None], axis=2)[..., 0]
    worst = float(np.abs(got - want)[keep].max())
    print("%s: sample_probs with the ban vs teacher-forced: %.3e (tol %.3e)" % (kind, worst, tol))
    assert keep.sum() >= samples.size // 4 and worst <= tol
    with _Unfused(), torch.no_grad(), Calls() as c:
        unfused = m.do_sample(dict(b), num_samples=N, uniforms=u, no_repeat_ngram=n)
    assert c.count("case_pointer_head_sample_ban") == T_
    for r, row in enumerate(to_np(unfused["samples"]).reshape(ITEMS * N, T_)):
        assert _repeats(_before_eos(row, eos), n) == 0, "unfused row %d repeats a bigram: %s" % (r, row)


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_zero_is_the_default_call_bit_for_bit(fixtures, kind):
    m, b = fixtures[kind]
    u = _uniforms(ITEMS * 3)
    with torch.no_grad():
        with Calls() as c0:
            default = (m.do_test(dict(b)), m.do_beam(dict(b), width=3), m.do_sample(dict(b), num_samples=3, uniforms=u))
        with Calls() as c1:
            explicit = (m.do_test(dict(b), no_repeat_ngram=0), m.do_beam(dict(b), width=3, no_repeat_ngram=0),
                        m.do_sample(dict(b), num_samples=3, uniforms=u, no_repeat_ngram=0))
        big = m.do_test(dict(b), no_repeat_ngram=T_ + 1)  # legal, bans nothing
    assert c0.calls == c1.calls, "no_repeat_ngram=0 changes the launches"
    assert not any(name.endswith("_ban") for name in c1.calls)
    for d, e in zip(default, explicit):
        assert set(d) == set(e)
        for k in d:
            assert torch.equal(d[k], e[k]), k
    assert torch.equal(big["answer"], default[0]["answer"])


def test_captured_greedy_pass_with_the_ban_replays_to_the_eager_ids(fixtures):
    m, b = fixtures["case"]
    with torch.no_grad():
        eager = m.do_test(dict(b), no_repeat_ngram=3)["answer"]
        static_out = {}
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.do_test(dict(b), no_repeat_ngram=3)  # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out["answer"] = m.do_test(dict(b), no_repeat_ngram=3)["answer"]
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(static_out["answer"], eager), "hipGraph replay of the banned greedy pass differs from the eager pass"
    del graph


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_consensus_over_a_repeat_free_pool(fixtures, kind):
    m, b = fixtures[kind]
    _, eos, _, _ = special_ids(m)
    with torch.no_grad(), Calls() as c:
        out = m.do_consensus(dict(b), pool="sample", no_repeat_ngram=2, num_samples=4, seed=3)
    assert c.count("case_pointer_head_sample_ban") == T_ and c.sampled == 0
    pool = to_np(out["samples"])
    assert pool.shape == (ITEMS, 4, T_)
    for r, row in enumerate(pool.reshape(-1, T_)):
        assert _repeats(_before_eos(row, eos), 2) == 0, "pool row %d repeats a bigram: %s" % (r, row)
    index = to_np(out["consensus_index"])
    assert np.array_equal(to_np(out["answer"]), pool[np.arange(ITEMS), index])
    with torch.no_grad(), Calls() as c:
        m.do_consensus(dict(b), pool="beam", width=2, no_repeat_ngram=3)
    assert c.count("case_pointer_head_beam_ban") >= 1
