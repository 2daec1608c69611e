"""METEOR on the MI355X: K40 (``case_meteor``) against the host form ``evaluation.meteor`` on compacted rows -- match, exact-match and chunk
counts, the alignment and ``best_ref`` EQUAL -- at the 64-bit word boundaries of its match masks, across the backward 64-token loads of a
long reference and over a partly filled last workgroup; the raw-row functions of ``evaluation.meteor_ids`` against the host form; two launches
and a graph replay bit for bit; the trainer's ``evaluate_meteor`` against ``predict`` + ``to_sentence`` + the host's ``eval_meteor``, and
``evaluate_generation`` against the three single-metric methods from one decoding pass.

nltk is not available where the tests run; the rule is written out in ``evaluation/meteor.py`` and pinned by hand in tests/test_meteor_cpu.py.

Counts, alignments and ``best_ref`` are integers and compared exactly.  ``meteor`` (f64) is compared at 1e-12 absolute, the project's bar for
f64 device scores (three divisions, four products and one ``pow`` on values in [0, 1]: two f64 libraries differ by a few ulp of 1.1e-16).
``meteor_pair`` at 1.2e-7 absolute: one f32 rounding of a value in [0, 1] (the project's F_TOL).  Measured maxima go to the session's parity
ledger (``helpers.record_error``, case "meteor"); profiles/meteor_parity.json keeps a copy."""
import numpy as np
import pytest
import torch

import cases
import sample_cases
from helpers import Calls, record_error, to_np
from test_meteor_cpu import restated_pair

pytestmark = pytest.mark.gpu

F_TOL, D_TOL = 1.2e-7, 1e-12
PAD, BOS, EOS, UNK, FIRST = 0, 1, 2, 3, 4  # the ids of the kernel-level tests
SPECIALS = (BOS, PAD, EOS, UNK)
# The class table of the kernel-level tests, V = 12: the three words of the small vocabulary are FIRST .. FIRST + 2.  FIRST and FIRST + 1 share
# class 0 (so that a pair with an exact partner for one of them must prefer it), FIRST + 2 has a negative entry (no class); 8 ~ 9 and
# 10 ~ 11; ids from 12 on lie outside the table.
TABLE = [-1, -1, -1, -1, 0, 0, -7, 5, 1, 1, 2, 2]
OUT_KEYS = ("counts", "meteor_pair", "meteor", "best_ref")


@pytest.fixture(scope="module")
def ns():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.float32)
    case_rg_amd.set_dropout(False)
    return case_rg_amd.namespace()


def _note(key, value, tol):
    record_error("meteor", "fp32", key, value, tol)


def _dev(x):
    return torch.as_tensor(x).cuda()


def _packed(lists, T, junk=FIRST):
    """Token lists -> (front-packed int64 [n, T] with garbage behind the length -- an id of the vocabulary, so that reading it would match --,
    lengths int32 [n])."""
    ids = np.full((len(lists), T), junk, dtype=np.int64)
    for i, toks in enumerate(lists):
        ids[i, :len(toks)] = toks
    return ids, np.array([len(t) for t in lists], dtype=np.int32)


def _raw_rows(lists, T):
    """Token lists -> raw decoder-style rows int64 [n, T]: BOS, the tokens, EOS, then ids that must be ignored; a PAD inside the sentence."""
    out = np.zeros((len(lists), T), dtype=np.int64)
    for i, toks in enumerate(lists):
        row = [BOS] + list(toks[:len(toks) // 2]) + [PAD] + list(toks[len(toks) // 2:]) + [EOS, FIRST + 1, FIRST + 2]
        assert len(row) <= T + 3
        row = row[:T]
        out[i, :len(row)] = row
    return out


def operands(items, Ta, Tb):
    """items: per item (hypothesis lists, reference lists), the same N and M everywhere -> a, a_len, b, b_len on the device."""
    a, a_len = zip(*[_packed(h, Ta) for h, _ in items])
    b, b_len = zip(*[_packed(r, Tb) for _, r in items])
    return _dev(np.stack(a)), _dev(np.stack(a_len)), _dev(np.stack(b)), _dev(np.stack(b_len))


def run_meteor(items, Ta, Tb, classes=None, want_align=True, **params):
    from case_rg_amd import ops
    table = None if classes is None else _dev(np.array(classes, dtype=np.int32))
    with Calls() as c:
        got = ops.meteor(*operands(items, Ta, Tb), table, want_align=want_align, **params)
    assert c.calls == {"case_meteor": 1}
    assert set(got) == set(OUT_KEYS) | ({"align"} if want_align else set())
    assert got["counts"].dtype == got["best_ref"].dtype == torch.int32 and got["meteor_pair"].dtype == torch.float32 and got["meteor"].dtype == torch.float64
    return got


def host_form(items, Ta, classes=None, **params):
    """The host form of every pair in K40's layout: counts [B, N, M, 3], align [B, N, M, Ta], pair and best scores (f64), best_ref."""
    from case_rg_amd.evaluation import best_meteor, pair_meteor
    B, N, M = len(items), len(items[0][0]), len(items[0][1])
    counts, align = np.zeros((B, N, M, 3), np.int32), np.full((B, N, M, Ta), -1, np.int32)
    pair, best, best_ref = np.zeros((B, N, M)), np.zeros((B, N)), np.full((B, N), -1, np.int32)
    for i, (hyps, refs) in enumerate(items):
        for n, h in enumerate(hyps):
            for m, r in enumerate(refs):
                if not r:
                    continue
                p = pair_meteor(h, r, classes, **params)
                counts[i, n, m] = p["matches"], p["exact"], p["chunks"]
                pair[i, n, m] = p["score"]
                for at, to in p["alignment"]:
                    align[i, n, m, at] = to
            best[i, n], best_ref[i, n] = best_meteor(h, refs, classes, **params)
    return dict(counts=counts, align=align, pair=pair, best=best, best_ref=best_ref)


def check(got, want, what, tag=None):
    """Integers equal; the scores within their tolerances; exactly 0 where the host form is; -> (worst pair, worst best)."""
    for key in ("counts", "best_ref") + (("align",) if "align" in got else ()):
        g = to_np(got[key])
        if not np.array_equal(g, want[key]):
            at = tuple(int(x[0]) for x in np.nonzero(g != want[key]))
            raise AssertionError("%s: %s differs at %s: got %d, the host form %d" % (what, key, at, g[at], want[key][at]))
    pair, best = to_np(got["meteor_pair"]).astype(np.float64), got["meteor"].cpu().numpy()
    assert np.array_equal(pair == 0.0, want["pair"] == 0.0) and np.array_equal(best == 0.0, want["best"] == 0.0), what
    worst = float(np.abs(pair - want["pair"]).max()), float(np.abs(best - want["best"]).max())
    print("%s: max |meteor_pair - host| = %.3e, max |meteor - host| = %.3e" % (what, worst[0], worst[1]))
    if tag:
        _note(tag + "_pair", worst[0], F_TOL)
        _note(tag + "_meteor", worst[1], D_TOL)
    assert worst[0] <= F_TOL and worst[1] <= D_TOL, (what, worst)
    return worst


# ---------------------------------------------------------------------------------------------
# 1. K40 at the word boundaries and across the backward loads of a long reference
# ---------------------------------------------------------------------------------------------
HYP_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256)
REF_SIZES = (1, 63, 64, 65, 129, 200, 1000)


def boundary_items(Ta, Tb, N, M, B, seed):
    """B items of N hypotheses against M references over the three-word vocabulary FIRST .. FIRST + 2 (plus 8 .. 13 sprinkled in for the class
    stage and the ids outside the table), so that every id repeats across the 64-lane words and the loads.  The first reference of an item has
    all Tb tokens, the others a random length; the hypotheses of an item are, in turn: Ta random tokens, the reference itself (its last Ta
    tokens), the reversed reference, Ta equal tokens (against the all-equal reference that item 1 holds, shorter or longer than Ta as Tb
    says), an empty row, and random ones of a random length.  From M = 3 on reference 1 of item 0 is absent, and the last item of a batch
    of more than two has no present reference."""
    rs = np.random.RandomState(seed)

    def tok(n):
        t = rs.randint(0, 3, n) + FIRST
        rare = rs.rand(n) < 0.15
        return np.where(rare, rs.randint(8, 14, n), t).tolist()

    items = []
    for i in range(B):
        refs = [tok(Tb)] + [tok(rs.randint(1, Tb + 1)) for _ in range(M - 1)]
        if i == 1:
            refs[0] = [FIRST] * Tb
        if M >= 3 and i == 0:
            refs[1] = []
        if B > 2 and i == B - 1:
            refs = [[] for _ in range(M)]
        base = refs[0] if refs[0] else tok(Tb)
        kinds = [tok(Ta), base[-Ta:], base[::-1][:Ta], [FIRST] * Ta, [], tok(rs.randint(1, Ta + 1))]
        hyps = [kinds[(i + n) % len(kinds)] for n in range(N)]
        items.append((hyps, refs))
    return items


@pytest.mark.parametrize("Tb", REF_SIZES)
@pytest.mark.parametrize("Ta", HYP_SIZES)
def test_meteor_at_the_word_and_load_boundaries(Ta, Tb):
    """3 hypotheses (N = 1, M = 1: less than one workgroup) and 10 (N = 5, M = 3), each with and without the class table."""
    worst = [0.0, 0.0]
    stage_two = 0
    for N, M, B in ((1, 1, 3), (5, 3, 2)):
        items = boundary_items(Ta, Tb, N, M, B, 4000 + 7 * Ta + Tb + N)
        for classes in (None, TABLE):
            got = run_meteor(items, Ta, Tb, classes)
            assert got["counts"].shape == (B, N, M, 3) and got["align"].shape == (B, N, M, Ta) and got["meteor"].shape == (B, N)
            w = check(got, host_form(items, Ta, classes), "Ta %d Tb %d N %d M %d %s" % (Ta, Tb, N, M, "classes" if classes else "exact"))
            worst = [max(worst[0], w[0]), max(worst[1], w[1])]
            counts = to_np(got["counts"])
            assert (counts[..., 1] <= counts[..., 0]).all() and (counts[..., 2] <= counts[..., 0]).all()
            if classes is None:
                assert (counts[..., 0] == counts[..., 1]).all(), "without a table every match is exact"
            else:
                stage_two += int((counts[..., 0] - counts[..., 1]).sum())
    assert stage_two > 0 or min(Ta, Tb) < 63, "the class stage must match something"
    _note("boundary_Ta%d_Tb%d_pair" % (Ta, Tb), worst[0], F_TOL)
    _note("boundary_Ta%d_Tb%d_meteor" % (Ta, Tb), worst[1], D_TOL)


@pytest.mark.parametrize("hypotheses", [3, 130])
def test_meteor_grid_tail(hypotheses):
    """3 hypotheses in one workgroup of four waves; 130 = 32 workgroups and a half (26 items x 5 candidates, 3 references each)."""
    B, N, M = (3, 1, 3) if hypotheses == 3 else (26, 5, 3)
    items = boundary_items(40, 70, N, M, B, 4100 + hypotheses)
    for classes in (None, TABLE):
        check(run_meteor(items, 40, 70, classes), host_form(items, 40, classes), "%d hypotheses" % hypotheses,
              tag="grid_tail_%d_%s" % (hypotheses, "classes" if classes else "exact"))


# ---------------------------------------------------------------------------------------------
# 2. the hazards, one by one, with the expected values written out
# ---------------------------------------------------------------------------------------------
def test_all_equal_rows_pair_from_the_end_across_the_words():
    """200 equal tokens against 150 and against 260: hypothesis position la - 1 - k meets reference position lb - 1 - k, one chunk; the
    highest set bit must be found across the words, and the chunk must carry from lane 63 into lane 0."""
    hyp = [FIRST] * 200
    items = [([hyp], [[FIRST] * 150, [FIRST] * 260])]
    got = run_meteor(items, 256, 260)
    align = to_np(got["align"])[0, 0]
    assert align[0, :50].tolist() == [-1] * 50 and align[0, 50:200].tolist() == list(range(150)) and (align[0, 200:] == -1).all()
    assert align[1, :200].tolist() == list(range(60, 260)) and (align[1, 200:] == -1).all()
    assert to_np(got["counts"])[0, 0].tolist() == [[150, 150, 1], [200, 200, 1]]
    check(got, host_form(items, 256), "all equal", tag="all_equal")
    assert int(got["best_ref"][0, 0]) == 0, "150 of 200 against 150 tokens beats 200 of 200 against 260 at alpha = 0.9"


def test_identity_and_reversal():
    """The hypothesis equal to the reference: every position, one chunk, (1 - gamma) at any length.  Equal to the reversed reference of
    DISTINCT ids: every position, as many chunks as tokens."""
    rs = np.random.RandomState(4200)
    same = (rs.randint(0, 3, 129) + FIRST).tolist()
    distinct = (rs.permutation(130) + 20).tolist()
    items = [([same, distinct[::-1]], [same, distinct])]
    got = run_meteor(items, 130, 130)
    counts, align = to_np(got["counts"])[0], to_np(got["align"])[0]
    assert counts[0, 0].tolist() == [129, 129, 1] and align[0, 0, :129].tolist() == list(range(129))
    assert counts[1, 1].tolist() == [130, 130, 130] and align[1, 1].tolist() == list(range(129, -1, -1))
    assert abs(float(got["meteor"][0, 0]) - (1 - 0.5 * (1 / 129) ** 3)) <= D_TOL and float(got["meteor"][0, 1]) == 0.5
    assert got["best_ref"][0].tolist() == [0, 1]
    check(got, host_form(items, 130), "identity and reversal", tag="identity")


def test_stage_one_wins_and_tokens_without_a_class_never_match():
    """FIRST ~ FIRST + 1 (class 0).  Against the reference (FIRST + 1, FIRST) the hypothesis (FIRST, 13) takes its exact partner at position 1
    and leaves FIRST + 1 alone; (FIRST, FIRST) takes the exact partner with its LAST token and the class partner with its first.  FIRST + 2
    (a negative entry) and 12 / 13 (outside the table) have no class: they match exactly or not at all."""
    a, b, c = FIRST, FIRST + 1, FIRST + 2
    items = [([[a, 13], [a, a], [c, 12, 7], [c, 13, 7], [9, 11, 7]], [[b, a], [7, c, 13], [10, 8, 7, 7]])]
    got = run_meteor(items, 3, 4, TABLE)
    counts, align = to_np(got["counts"])[0], to_np(got["align"])[0]
    assert counts[0, 0].tolist() == [1, 1, 1] and align[0, 0].tolist() == [1, -1, -1]
    assert counts[1, 0].tolist() == [2, 1, 1] and align[1, 0].tolist() == [0, 1, -1]
    assert counts[2, 1].tolist() == [2, 2, 2] and align[2, 1].tolist() == [1, -1, 0], "12 and 13 lie outside the table and never meet"
    assert counts[3, 1].tolist() == [3, 3, 2] and align[3, 1].tolist() == [1, 2, 0]
    assert counts[4, 2].tolist() == [3, 1, 3] and align[4, 2].tolist() == [1, 0, 3], "9 ~ 8, 11 ~ 10, and 7 takes the LAST 7"
    check(got, host_form(items, 3, TABLE), "stage one wins", tag="stage_one_wins")
    exact = run_meteor(items, 3, 4, None)
    assert to_np(exact["counts"])[0, 1, 0].tolist() == [1, 1, 1] and to_np(exact["counts"])[0, 4, 2].tolist() == [1, 1, 1]


def test_parameters_reach_the_score():
    items = boundary_items(65, 129, 5, 3, 2, 4300)
    for params in (dict(alpha=0.5, beta=1.0, gamma=1.0), dict(alpha=0.0, beta=0.0, gamma=0.25), dict(alpha=1.0, beta=2.5, gamma=0.0)):
        check(run_meteor(items, 65, 129, TABLE, **params), host_form(items, 65, TABLE, **params), str(params),
              tag="params_a%g_b%g_g%g" % (params["alpha"], params["beta"], params["gamma"]))


# ---------------------------------------------------------------------------------------------
# 3. determinism, capture, the optional output
# ---------------------------------------------------------------------------------------------
def test_two_launches_give_equal_bits_and_align_is_optional():
    items = boundary_items(129, 200, 5, 3, 26, 4400)
    first, second, bare = (run_meteor(items, 129, 200, TABLE, want_align=w) for w in (True, True, False))
    for key in OUT_KEYS + ("align",):
        assert torch.equal(first[key], second[key]), key
    for key in OUT_KEYS:
        assert torch.equal(first[key], bare[key]), "want_align=False changes %s" % key
    assert int(first["counts"][..., 0].sum()) > 0 and float(first["meteor"].max()) > 0.0


def test_meteor_ids_replays_from_a_captured_graph():
    """Nothing in ``meteor_ids`` waits for the host: captured once, the replay on new rows written into the same buffers is the eager call."""
    from case_rg_amd.evaluation import meteor_ids
    rs = np.random.RandomState(4500)
    tok = lambda n: (rs.randint(0, 6, n) + FIRST).tolist()  # noqa: E731
    sets = []
    for _ in range(2):
        hyps = [[tok(rs.randint(0, 40)) for _ in range(3)] for _ in range(9)]
        refs = [[tok(rs.randint(1, 60)), [], tok(rs.randint(1, 60))] for _ in range(9)]
        sets.append((_dev(np.stack([_raw_rows(h, 48) for h in hyps])),
                     _dev(np.stack([_raw_rows(r, 64) * (np.array([len(x) for x in r])[:, None] > 0) for r in refs]))))
    table = _dev(np.array(TABLE, dtype=np.int32))
    call = lambda h, r: meteor_ids(h, r, SPECIALS, table, want_align=True)  # noqa: E731
    eager = {k: v.clone() for k, v in call(*sets[1]).items()}
    hyp, ref = sets[0][0].clone(), sets[0][1].clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(hyp, ref)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph, static = torch.cuda.CUDAGraph(), {}
    with torch.cuda.graph(graph), Calls() as c:
        static.update(call(hyp, ref))
    assert c.count("case_meteor") == 1
    hyp.copy_(sets[1][0])
    ref.copy_(sets[1][1])
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(static[k], eager[k]), "the replay differs from the eager call in %s" % k
    assert not torch.equal(eager["meteor"], call(*sets[0])["meteor"]), "the two sets must differ"
    del graph


# ---------------------------------------------------------------------------------------------
# 4. raw rows against the host form
# ---------------------------------------------------------------------------------------------
def test_meteor_ids_on_raw_rows_is_the_host_form():
    from case_rg_amd.common.Utils import remove_duplicate
    from case_rg_amd.evaluation import best_meteor, eval_meteor, eval_meteor_ids, meteor_ids, pair_meteor
    rs = np.random.RandomState(4600)
    tok = lambda n: (rs.randint(0, 10, n) + FIRST).tolist()  # noqa: E731
    refs = [[tok(rs.randint(12, 41)), tok(rs.randint(12, 41)), tok(rs.randint(12, 41))] for _ in range(24)]
    hyps = [[int(rs.randint(0, 10)) + FIRST if rs.rand() < 0.2 else t for t in r[i % 3][:rs.randint(8, len(r[i % 3]) + 1)]] for i, r in enumerate(refs)]
    for i in range(0, 24, 5):
        refs[i][(i + 1) % 3] = []                                  # an absent reference among present ones
    refs[-2] = [[], [], []]                                        # an item without a present reference
    hyps[0] = []                                                   # an empty answer counts as [UNK]
    refs[0][0] = tok(5) + [UNK] + tok(5)
    hyps[1] = hyps[1][:6] + hyps[1][:6] + hyps[1][:6]              # repeated 6 tokens: remove_duplicate cuts them
    T = 48
    hyp, ref = _dev(_raw_rows(hyps, T)), _dev(np.stack([_raw_rows(r, T) * (np.array([len(x) for x in r])[:, None] > 0) for r in refs]))
    table = _dev(np.array(TABLE, dtype=np.int32))
    for dedup in (False, True):
        lists = [h if h else [UNK] for h in hyps]
        if dedup:
            lists = [list(h) for h in lists]
            remove_duplicate(lists)
            assert len(lists[1]) < 18, "remove_duplicate must cut the repeated answer"
        for classes in (None, TABLE):
            out = meteor_ids(hyp, ref, SPECIALS, None if classes is None else table, remove_duplicates=dedup, want_align=True)
            assert set(out) == {"matches", "exact", "chunks", "meteor_pair", "meteor", "best_ref", "ref_valid", "align"}
            assert to_np(out["ref_valid"]).tolist() == [[len(x) > 0 for x in r] for r in refs]
            assert out["align"].shape == (24, 1, 3, T)
            for i, (h, r) in enumerate(zip(lists, refs)):
                score, at = best_meteor(h, r, classes)
                assert int(out["best_ref"][i, 0]) == at and abs(float(out["meteor"][i, 0]) - score) <= D_TOL, i
                for m, x in enumerate(r):
                    p = pair_meteor(h, x, classes) if x else dict(matches=0, exact=0, chunks=0, score=0.0, alignment=[])
                    assert [int(out[k][i, 0, m]) for k in ("matches", "exact", "chunks")] == [p["matches"], p["exact"], p["chunks"]], (i, m)
                    assert abs(float(out["meteor_pair"][i, 0, m]) - p["score"]) <= F_TOL
                    assert [(k, v) for k, v in enumerate(to_np(out["align"][i, 0, m]).tolist()) if v >= 0] == p["alignment"]
                    assert p == restated_pair(h, x, classes), "the restatement agrees on the same lists"
            assert int(out["matches"][0, 0, 0]) == 1, "the empty answer is [UNK] and meets the UNK of its reference"
            per_item = eval_meteor_ids(hyp, ref, SPECIALS, None if classes is None else table, remove_duplicates=dedup)
            assert per_item.dtype == torch.float64 and per_item.shape == (24,) and per_item.is_cuda
            assert float(per_item[-2]) == 0.0 and int(out["best_ref"][-2, 0]) == -1, "an item without a present reference scores 0"
            want = eval_meteor(lists, refs, classes)
            assert round(float(per_item.mean()), 2) == want > 0.0
            _note("raw_rows_%s%s" % ("classes" if classes else "exact", "_dedup" if dedup else ""),
                  float(np.abs(out["meteor"][:, 0].cpu().numpy() - np.array([best_meteor(h, r, classes)[0] for h, r in zip(lists, refs)])).max()), D_TOL)
    with pytest.raises(TypeError, match="one answer per item"):
        eval_meteor_ids(hyp.unsqueeze(1), ref, SPECIALS)


# ---------------------------------------------------------------------------------------------
# 5. the trainer
# ---------------------------------------------------------------------------------------------
def _trainer_data(m, b):
    """Four items.  Beside ``response`` the dataset carries ``truths`` [4, 3, T']: the response, an all-PAD row (absent) and, for two items, the
    model's own greedy answer (so that the numbers are well above 0)."""
    data = {k: v.cpu() for k, v in b.items()}
    with torch.no_grad():
        greedy = m(dict(b), method="test")["answer"].cpu()
    truths = torch.zeros(4, 3, max(greedy.shape[1], data["response"].shape[1]), dtype=torch.int64)
    truths[:, 0, :data["response"].shape[1]] = data["response"]
    truths[:2, 2, :greedy.shape[1]] = greedy[:2]
    data["truths"] = truths
    return data


@pytest.mark.parametrize("name", ["sample_case", "sample_masque"])
def test_trainer_evaluate_meteor_is_the_host_number(ns, name):
    """Batches of 3 and 1.  The class table joins neighbouring ids in pairs, so the class stage has work on the model's own vocabulary."""
    from case_rg_amd.common.Utils import remove_duplicate
    from case_rg_amd.evaluation import eval_meteor
    from case_rg_amd.evaluation.rouge_ids import model_specials
    m, b = sample_cases.build(ns, torch.device("cuda"), name)
    m.eval()
    data = _trainer_data(m, b)
    V = len(m.vocab2id)
    table = (torch.arange(V, dtype=torch.int32) // 2)
    table[list(model_specials(m.vocab2id))] = -1
    trainer = ns.CumulativeTrainer(m, None, None, None, 1)
    trainer.model.train()
    ds = cases._ListDataset(data)
    for references, dedup, classes in (("response", False, None), ("truths", False, None), ("truths", True, None), ("truths", False, table)):
        got = trainer.evaluate_meteor(ds, cases._collate, 3, method="test", references=references, remove_duplicates=dedup,
                                      classes=None if classes is None else classes.cuda())
        assert trainer.model.training, "the mode must be restored"
        run, ref = [], []
        for batch, out in trainer.predict("test", ds, cases._collate, 3):
            sents = [list(s) for s in m.to_sentence(batch, out["answer"])]
            if dedup:
                remove_duplicate(sents)
            run += sents
            rows = batch[references] if batch[references].dim() == 3 else batch[references].unsqueeze(1)
            for item in rows:
                ref.append([s for s, raw in zip(m.to_sentence(batch, item), item.tolist()) if any(raw)])
        trainer.model.train()
        by_word = None if classes is None else {w: int(classes[i]) for w, i in m.vocab2id.items()}
        want = eval_meteor(run, ref, by_word)
        print("evaluate_meteor(%s, dedup %s, classes %s): %s, host %.2f" % (references, dedup, classes is not None, got, want))
        assert set(got) == {"meteor", "items"} and got["items"] == 4
        assert "%.2f" % got["meteor"] == "%.2f" % want
        if references == "truths" and not dedup:
            assert got["meteor"] > 0.0
    trainer.close()


@pytest.mark.parametrize("name", ["sample_case", "sample_masque"])
def test_evaluate_generation_is_the_three_numbers_from_one_pass(ns, name):
    m, b = sample_cases.build(ns, torch.device("cuda"), name)
    m.eval()
    ds = cases._ListDataset(_trainer_data(m, b))
    trainer = ns.CumulativeTrainer(m, None, None, None, 1)
    trainer.model.train()
    forwards = []
    hook = m.register_forward_pre_hook(lambda *a, **k: forwards.append(1))
    try:
        for dedup in (False, True):
            args = dict(method="test", references="truths", remove_duplicates=dedup)
            del forwards[:]
            single = dict(rouge_l=trainer.evaluate_rouge(ds, cases._collate, 3, **args)["rouge_l"],
                          bleu=trainer.evaluate_bleu(ds, cases._collate, 3, **args)["bleu"],
                          meteor=trainer.evaluate_meteor(ds, cases._collate, 3, **args)["meteor"])
            assert len(forwards) == 6, "three methods, two batches each"
            del forwards[:]
            with Calls() as c:
                got = trainer.evaluate_generation(ds, cases._collate, 3, **args)
            assert len(forwards) == 2, "one decoding pass per batch, not one per metric (%d forward calls)" % len(forwards)
            assert c.count("case_lcs_pairs") == c.count("case_ngram_counts") == c.count("case_bleu_scores") == c.count("case_meteor") == 2
            assert trainer.model.training, "the mode must be restored"
            assert got == dict(single, items=4), (got, single)
            assert got["meteor"] > 0.0 and got["rouge_l"] > 0.0
        del forwards[:]
        only = trainer.evaluate_generation(ds, cases._collate, 3, references="truths", remove_duplicates=True, metrics=("meteor",))
        assert only == dict(meteor=single["meteor"], items=4) and len(forwards) == 2
        with pytest.raises(ValueError, match="metrics must name"):
            trainer.evaluate_generation(ds, cases._collate, 3, metrics=("rouge_l", "cider"))
        assert len(forwards) == 2, "an unknown metric is refused before anything is decoded"
    finally:
        hook.remove()
    trainer.close()
