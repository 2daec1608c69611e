"""ROUGE-1 / ROUGE-2 on the MI355X: K43 (``case_ngram_distinct``) against a Python ``set`` restatement, exactly, at every length around its
windows and with k-grams planted across every window seam; K44 (``case_rouge_n_scores``) against the host's arithmetic on counts with zero
denominators, absent references and planted equal F values; ``evaluation.rouge_n_ids`` / ``eval_rouge_n_ids`` against the reference-generated
fixture (tests/golden/rouge_n.npz); the trainer's ``evaluate_rouge(orders=...)`` and ``evaluate_generation`` against ``predict`` +
``to_sentence`` + the host's ``eval_rouge``; ``consensus(metric="rouge_2")``, ``do_consensus`` of both task models, stream capture.

Counts are integers and compared exactly.  ``f`` / ``p`` / ``r`` (f64) at 1e-12 and ``f_pair`` (f32) at 1.2e-7 absolute: the project's bars for
K35 and K40, one f64 evaluation of a value in [0, 1] and one f32 rounding of it.  Utilities at 1e-6 relative (K31's bar: f32 sums of at most 64
terms against f64).

K43 counts a row in windows of 256 positions that start every 253 (one window of 64 / 128 positions when the rows have at most 64 / 128):
window w >= 1 counts the positions from 253 w + 3 on, so the seams lie in front of the positions 256, 509, 762, ..."""
import math

import numpy as np
import pytest
import torch

import cases
import sample_cases
from helpers import Calls, record_error, to_np
from test_consensus_cpu import restated_pick
from test_rouge_n_cpu import fixture_lists, restated_distinct

pytestmark = pytest.mark.gpu

F_TOL, D_TOL = 1.2e-7, 1e-12
PAD, BOS, EOS, UNK, FIRST = 0, 1, 2, 3, 4  # the ids of the kernel-level tests
SPECIALS = (BOS, PAD, EOS, UNK)
SEAMS = (256, 509, 762)  # the first position that the windows 1, 2 and 3 count (Tb > 128)
LENGTHS = (0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129) + tuple(range(250, 261)) + tuple(range(505, 516)) + (1000,)


@pytest.fixture(scope="module")
def ns():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.float32)
    case_rg_amd.set_dropout(False)
    return case_rg_amd.namespace()


def _note(key, value, tol):
    record_error("rouge_n", "fp32", key, value, tol)


def _dev(x):
    return torch.as_tensor(x).cuda()


def _packed(lists, T, junk=FIRST + 1):
    """Token lists -> (front-packed int64 [n, T] with an id of the vocabulary behind the length, so that reading it would count, lengths)."""
    ids = np.full((len(lists), T), junk, dtype=np.int64)
    for i, toks in enumerate(lists):
        ids[i, :len(toks)] = toks
    return ids, np.array([len(t) for t in lists], dtype=np.int32)


def _raw_rows(lists, T):
    """Token lists -> raw decoder-style rows int64 [n, T]: BOS, the tokens with a PAD inside, EOS, then ids that must be ignored; an empty
    list is an all-PAD row (an absent reference)."""
    out = np.zeros((len(lists), T), dtype=np.int64)
    for i, toks in enumerate(lists):
        if len(toks) == 0:
            continue
        row = [BOS] + list(toks[:len(toks) // 2]) + [PAD] + list(toks[len(toks) // 2:]) + [EOS, FIRST + 1, FIRST + 2]
        assert len(row) <= T + 3
        row = row[:T]
        out[i, :len(row)] = row
    return out


def want_distinct(lists, max_n=4):
    return np.array([[restated_distinct(t, k) if k <= max_n else 0 for k in (1, 2, 3, 4)] for t in lists], dtype=np.int32)


def run_distinct(ids, lens, max_n=4):
    """K43 twice: through the ABI into an output pre-filled with -1 (every owned entry must be written) and through ``ops``; equal bits."""
    from case_rg_amd import _abi, ops
    ids, lens = _dev(ids), _dev(lens)
    out = torch.full((ids.shape[0], 4), -1, dtype=torch.int32, device="cuda")
    _abi.call("case_ngram_distinct", ids.data_ptr(), lens.data_ptr(), out.data_ptr(), ids.shape[0], ids.shape[1], max_n,
              torch.cuda.current_stream().cuda_stream)
    with Calls() as c:
        again = ops.ngram_distinct(ids, lens, max_n)
    assert c.calls == {"case_ngram_distinct": 1}
    assert again.dtype == torch.int32 and again.shape == (ids.shape[0], 4)
    assert torch.equal(out, again), "two calls must give the same bits"
    return to_np(out)


def check_distinct(lists, Tb, max_n=4, what=""):
    ids, lens = _packed(lists, Tb)
    got, want = run_distinct(ids, lens, max_n), want_distinct(lists, max_n)
    if not np.array_equal(got, want):
        row, k = (int(x[0]) for x in np.nonzero(got != want))
        raise AssertionError("%s row %d (%d tokens), order %d: got %d, the set has %d" % (what, row, len(lists[row]), k + 1, got[row, k], want[row, k]))
    return got


def _tokens(rs, n, vocab):
    """vocab None: all distinct."""
    return (np.arange(n) + 100).tolist() if vocab is None else (rs.randint(0, vocab, n) + FIRST).tolist()


# ---------------------------------------------------------------------------------------------
# 1. K43 against the set
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tb", [64, 128, 129, 1000])
def test_ngram_distinct_at_every_length_around_the_windows(Tb):
    """Every length of LENGTHS up to Tb with vocabularies of 1, 2, 3 ids and all-distinct ids; Tb 64 and 128 take the one-window kernels."""
    rs = np.random.RandomState(430 + Tb)
    lists = [_tokens(rs, n, vocab) for n in LENGTHS if n <= Tb for vocab in (1, 2, 3, None)]
    got = check_distinct(lists, Tb, what="Tb %d" % Tb)
    assert got.max() == Tb, "the all-distinct row of full length"
    if Tb == 1000:
        assert (got[[i for i, t in enumerate(lists) if len(t) == 1000 and t[0] < 100]][:, 3] <= 81).all(), "3 ids make at most 81 4-grams"


def test_ngram_distinct_on_a_long_row():
    rs = np.random.RandomState(433)
    got = check_distinct([_tokens(rs, 3840, 2), _tokens(rs, 3840, 3), _tokens(rs, 3840, None), _tokens(rs, 3839, 6)], 3840, what="Tb 3840")
    assert got[2].tolist() == [3840, 3839, 3838, 3837] and got[0].tolist() == [2, 4, 8, 16]


def seam_rows():
    """For every seam c of SEAMS, every order k = 2, 3, 4 and every start q with q < c <= q + k - 1 (the k-gram straddles the seam): an
    all-distinct row in which that k-gram occurs once more, (a) only in an EARLIER window (at position 10 + c // 253, window 0) and (b) only
    LATER (300 positions on, a later window).  In (a) the straddling occurrence must drop out, in (b) it must be the one that counts."""
    rows = []
    for c in SEAMS:
        for k in (2, 3, 4):
            for q in range(c - k + 1, c):
                base = (np.arange(1100) + 100).tolist()
                early, late = list(base), list(base)
                at = 10 + c // 253
                early[at:at + k] = base[q:q + k]
                late[q + 300:q + 300 + k] = base[q:q + k]
                rows.append((q + k, early, late))
    return rows


def test_ngram_distinct_across_the_window_seams():
    rows = seam_rows()
    assert len(rows) == 3 * 6
    full = [r for _, early, late in rows for r in (early, late)]
    got = check_distinct(full, 1100, what="seams")
    # a row of 1100 ids with one k-gram doubled holds k ids fewer than 1100 and exactly one k-gram twice
    assert (got[:, 0] <= 1098).all() and (got[:, 0] >= 1096).all()
    # the (a) rows cut right behind the straddling k-gram: the seam is then in the LAST window, which counts fewer than k positions
    check_distinct([early[:end] for end, early, _ in rows], 800, what="cut seams")


@pytest.mark.parametrize("max_n", [1, 2, 3, 4])
def test_ngram_distinct_orders_above_max_n_read_zero(max_n):
    rs = np.random.RandomState(434)
    lists = [_tokens(rs, n, vocab) for n in (0, 1, 3, 4, 64, 129, 257, 600) for vocab in (2, None)]
    for Tb in (64, 128, 600):
        got = check_distinct([t for t in lists if len(t) <= Tb], Tb, max_n, what="max_n %d, Tb %d" % (max_n, Tb))
        assert (got[:, max_n:] == 0).all() and got[:, :max_n].max() > 0


@pytest.mark.parametrize("rows", [1, 3, 130])
def test_ngram_distinct_rows_and_lengths_out_of_range(rows):
    """1, 3 and 130 rows (a part-filled and many workgroups); a length above Tb is Tb, a negative one is 0."""
    rs = np.random.RandomState(435 + rows)
    Tb = 300
    ids = rs.randint(0, 3, (rows, Tb)).astype(np.int64) + FIRST
    lens = rs.randint(0, Tb + 1, rows).astype(np.int32)
    lens[0] = Tb + 7
    if rows > 2:
        lens[1], lens[2] = -3, 2 ** 31 - 1
    got = run_distinct(ids, lens)
    want = want_distinct([ids[i, :min(max(int(n), 0), Tb)].tolist() for i, n in enumerate(lens)])
    assert np.array_equal(got, want), np.nonzero(got != want)


@pytest.mark.parametrize("Ta", [64, 128, 256])
def test_ngram_distinct_is_k34s_distinct_on_rows_that_fit(Ta):
    from case_rg_amd import ops
    rs = np.random.RandomState(436 + Ta)
    lens = [n for n in (0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 255, 256) if n <= Ta]
    a, a_len = _packed([_tokens(rs, n, 3) for n in lens] + [_tokens(rs, n, None) for n in lens], Ta)
    a, a_len = _dev(a).view(2, len(lens), Ta), _dev(a_len).view(2, len(lens))
    b, b_len = _dev(np.full((2, 1, 5), FIRST, dtype=np.int64)), _dev(np.full((2, 1), 5, dtype=np.int32))
    for max_n in (2, 4):
        assert torch.equal(ops.ngram_distinct(a, a_len, max_n), ops.ngram_counts(a, a_len, b, b_len, max_n)["distinct"])


# ---------------------------------------------------------------------------------------------
# 2. K44 against the host's arithmetic
# ---------------------------------------------------------------------------------------------
def host_scores(hit, e, d, b_len, max_n):
    """evaluation.rouge.rouge_n's arithmetic on counts, in its order, and K44's selection rule."""
    B, N, M = hit.shape[:3]
    f_pair = np.zeros((B, N, M, 4))
    f, p, r, best = np.zeros((B, N, 4)), np.zeros((B, N, 4)), np.zeros((B, N, 4)), np.full((B, N, 4), -1, dtype=np.int32)
    for i in range(B):
        for n in range(N):
            for k in range(max_n):
                for m in range(M):
                    if b_len[i, m] <= 0:
                        continue
                    o = int(hit[i, n, m, k])
                    pm = 0.0 if e[i, n, k] == 0 else o / int(e[i, n, k])
                    rm = 0.0 if d[i, m, k] == 0 else o / int(d[i, m, k])
                    fm = 2.0 * ((pm * rm) / (pm + rm + 1e-8))
                    f_pair[i, n, m, k] = fm
                    if best[i, n, k] < 0 or fm > f[i, n, k]:
                        best[i, n, k], f[i, n, k], p[i, n, k], r[i, n, k] = m, fm, pm, rm
    return f_pair, f, p, r, best


@pytest.mark.parametrize("max_n", [4, 2])
def test_rouge_n_scores_against_the_host_arithmetic(max_n):
    from case_rg_amd import ops
    rs = np.random.RandomState(437)
    B, N, M = 6, 3, 4
    e = rs.randint(0, 7, (B, N, 4)).astype(np.int32)              # zero denominators among them
    d = rs.randint(0, 7, (B, M, 4)).astype(np.int32)
    hit = np.minimum(rs.randint(0, 7, (B, N, M, 4)), np.minimum(e[:, :, None], d[:, None])).astype(np.int32)
    b_len = rs.randint(1, 9, (B, M)).astype(np.int32)
    b_len[0, 0] = b_len[1, 3] = b_len[2, :3] = 0                    # absent references, in front and behind
    b_len[3] = 0                                                    # an item without a reference
    d[4, 2], hit[4, :, 2] = d[4, 0], hit[4, :, 0]                   # planted equal F values: the lowest index wins
    d[5, 3], hit[5, :, 3] = d[5, 1], hit[5, :, 1]
    d[0, 1], hit[0, :, 1] = d[0, 0], hit[0, :, 0]                   # equal to an ABSENT reference: the present one wins
    hit[5, :, 0] = np.minimum(hit[5, :, 0], 4)
    e[5, 0], d[5, 0], hit[5, 0, 0] = 4, 4, 4                        # a full match, F = 2 / (2 + 1e-8)
    with Calls() as c:
        got = ops.rouge_n_scores(_dev(hit), _dev(e), _dev(d), _dev(b_len), max_n)
    assert c.calls == {"case_rouge_n_scores": 1}
    assert {k: (v.dtype, tuple(v.shape)) for k, v in got.items()} == dict(
        f_pair=(torch.float32, (B, N, M, 4)), f=(torch.float64, (B, N, 4)), p=(torch.float64, (B, N, 4)), r=(torch.float64, (B, N, 4)),
        best_ref=(torch.int32, (B, N, 4)))
    f_pair, f, p, r, best = host_scores(hit, e, d, b_len, max_n)
    gap_pair = float(np.abs(got["f_pair"].double().cpu().numpy() - f_pair).max())
    gap = max(float(np.abs(got[k].cpu().numpy() - w).max()) for k, w in (("f", f), ("p", p), ("r", r)))
    _note("k44_f_pair_max_n%d" % max_n, gap_pair, F_TOL)
    _note("k44_fpr_max_n%d" % max_n, gap, D_TOL)
    print("K44 max_n %d: f_pair gap %.3e, f / p / r gap %.3e" % (max_n, gap_pair, gap))
    assert gap_pair <= F_TOL and gap <= D_TOL
    assert np.array_equal(to_np(got["best_ref"]), best)
    assert (best[3] == -1).all() and (f[3] == 0).all() and (best[:, :, max_n:] == -1).all()
    assert (best[4, :, :max_n] != 2).all() and (best[5, :, :max_n] != 3).all() and (best[0, :, :max_n] >= 1).all()
    assert (f_pair[4, :, 0] == f_pair[4, :, 2]).all() and f_pair[5, 0, 0, 0] == 2.0 * (1.0 / (2.0 + 1e-8)) and (f > 0).sum() > 10
    again = ops.rouge_n_scores(_dev(hit), _dev(e), _dev(d), _dev(b_len), max_n)
    assert all(torch.equal(got[k], again[k]) for k in got), "two calls must give the same bits"


# ---------------------------------------------------------------------------------------------
# 3. the device form on the reference-generated fixture
# ---------------------------------------------------------------------------------------------
def test_rouge_n_ids_on_the_reference_fixture():
    from case_rg_amd.evaluation import eval_rouge_n_ids, rouge_n, rouge_n_ids
    g, hyps, truths = fixture_lists()
    B, M = len(hyps), 3
    padded = [t + [[]] * (M - len(t)) for t in truths]
    hyp = _dev(_raw_rows(hyps, g["hyp"].shape[1] + 5))
    ref = _dev(np.stack([_raw_rows(t, g["refs"].shape[2] + 5) for t in padded]))
    with Calls() as c:
        got = rouge_n_ids(hyp, ref, SPECIALS)
    assert c.calls == {"case_sentence_compact": 2, "case_ngram_counts": 1, "case_ngram_distinct": 1, "case_rouge_n_scores": 1}
    assert set(got) == {"hit", "hyp_distinct", "ref_distinct", "f_pair", "f", "p", "r", "best_ref", "ref_valid"}
    assert to_np(got["ref_valid"]).tolist() == (g["ref_len"] > 0).tolist()
    want_hit = np.zeros((B, 1, M, 4), dtype=np.int32)
    for i in range(B):
        for m, t in enumerate(truths[i]):
            for k in (1, 2):
                grams = lambda x: {tuple(x[j:j + k]) for j in range(len(x) - k + 1)}  # noqa: E731
                want_hit[i, 0, m, k - 1] = len(grams(hyps[i]) & grams(t))
    assert np.array_equal(to_np(got["hit"]), want_hit)
    assert np.array_equal(to_np(got["hyp_distinct"])[:, 0], want_distinct(hyps, 2))
    assert np.array_equal(to_np(got["ref_distinct"]), np.stack([want_distinct(t, 2) for t in padded]))
    gap_pair = float(np.abs(got["f_pair"][:, 0, :, :2].double().cpu().numpy() - g["scores"][..., 0]).max())
    best = np.array([[int(np.argmax(g["scores"][i, :len(t), k, 0])) for k in (0, 1)] for i, t in enumerate(truths)])
    rows = np.arange(B)[:, None]
    want = g["scores"][rows, best, np.arange(2)[None, :]]  # [B, 2, 3]: (f, p, r) of the best truth per order
    gap = max(float(np.abs(got[key][:, 0, :2].cpu().numpy() - want[..., j]).max()) for j, key in enumerate(("f", "p", "r")))
    _note("fixture_f_pair", gap_pair, F_TOL)
    _note("fixture_fpr", gap, D_TOL)
    print("rouge_n_ids on the fixture: f_pair gap %.3e, f / p / r gap %.3e" % (gap_pair, gap))
    assert gap_pair <= F_TOL and gap <= D_TOL
    assert np.array_equal(to_np(got["best_ref"])[:, 0, :2], best) and (to_np(got["best_ref"])[:, 0, 2:] == -1).all()
    assert (to_np(got["f_pair"])[..., 2:] == 0).all() and (to_np(got["f"])[..., 2:] == 0).all()
    per_item = eval_rouge_n_ids(hyp, ref, SPECIALS)
    assert per_item.dtype == torch.float64 and per_item.shape == (B, 2)
    host = np.array([[max(rouge_n(hyps[i], t, k)[0] * 100 for t in truths[i]) for k in (1, 2)] for i in range(B)])
    gap_mean = float(np.abs(per_item.cpu().numpy().mean(0) - host.mean(0)).max())
    print("eval_rouge_n_ids means %s, host %s" % (per_item.cpu().numpy().mean(0), host.mean(0)))
    assert gap_mean <= 1e-9
    assert [round(float(x), 2) for x in host.mean(0)] == g["aggregates"][:2].tolist()
    only_2 = eval_rouge_n_ids(hyp, ref, SPECIALS, orders=(2,))
    assert only_2.shape == (B, 1) and torch.equal(only_2[:, 0], per_item[:, 1])
    # one ground truth as [B, T']; an empty hypothesis counts as [UNK]; a long reference goes through K43's windows
    long_ref = (np.arange(700) % 5 + FIRST).tolist()
    ans = _dev(np.array([[BOS, EOS, 9, 9], [BOS, FIRST, FIRST + 1, EOS]], dtype=np.int64))
    one = rouge_n_ids(ans, _dev(_raw_rows([[UNK, 9], long_ref], 710)), SPECIALS, max_n=4)
    assert to_np(one["hyp_distinct"])[:, 0].tolist() == [[1, 0, 0, 0], [2, 1, 0, 0]]
    assert to_np(one["ref_distinct"])[:, 0].tolist() == [[2, 1, 0, 0], [5, 5, 5, 5]]
    assert one["p"][:, 0].cpu().numpy().tolist() == [[1.0, 0.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0]]
    assert one["r"][:, 0].cpu().numpy().tolist() == [[0.5, 0.0, 0.0, 0.0], [2 / 5, 1 / 5, 0.0, 0.0]]


# ---------------------------------------------------------------------------------------------
# 4. the trainer
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
def test_trainer_reports_the_three_rouge_figures_of_the_host(ns, name):
    from case_rg_amd.common.Utils import remove_duplicate
    from case_rg_amd.evaluation import eval_rouge
    m, b = sample_cases.build(ns, torch.device("cuda"), name)
    m.eval()
    ds = cases._ListDataset(_trainer_data(m, b))
    trainer = ns.CumulativeTrainer(m, None, None, None, 1)
    trainer.model.train()
    forwards = []
    hook = m.register_forward_pre_hook(lambda *a, **k: forwards.append(1))
    try:
        for references, dedup in (("response", False), ("truths", False), ("truths", True)):
            args = dict(method="test", references=references, remove_duplicates=dedup)
            del forwards[:]
            with Calls() as plain_calls:
                plain = trainer.evaluate_rouge(ds, cases._collate, 3, **args)
            assert len(forwards) == 2 and set(plain) == {"rouge_l", "items"}
            assert not [n for n in plain_calls.calls if "ngram" in n or "rouge_n" in n], "without orders: the launches of before"
            assert plain_calls.count("case_lcs_pairs") == 2
            del forwards[:]
            with Calls() as c:
                got = trainer.evaluate_rouge(ds, cases._collate, 3, orders=(1, 2), **args)
            assert len(forwards) == 2, "one forward call per batch (%d)" % len(forwards)
            assert c.count("case_ngram_counts") == c.count("case_ngram_distinct") == c.count("case_rouge_n_scores") == c.count("case_lcs_pairs") == 2
            del forwards[:]
            both = trainer.evaluate_generation(ds, cases._collate, 3, metrics=("rouge_1", "rouge_2", "rouge_l"), **args)
            assert len(forwards) == 2, "one forward call per batch (%d)" % len(forwards)
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
            want = eval_rouge(run, ref)
            print("evaluate_rouge(%s, dedup %s, orders (1, 2)): %s, host %s" % (references, dedup, got, want))
            assert list(got) == ["rouge_l", "rouge_1", "rouge_2", "items"] and got["items"] == 4
            assert list(both) == ["rouge_1", "rouge_2", "rouge_l", "items"] and both == got
            assert plain == dict(rouge_l=got["rouge_l"], items=4), "without orders: the dict of before"
            for key, name_ in (("rouge_1", "ROUGE_1_F1"), ("rouge_2", "ROUGE_2_F1"), ("rouge_l", "ROUGE_L_F1")):
                assert "%.2f" % got[key] == "%.2f" % want[name_], (key, got, want)
            if references == "truths" and not dedup:
                assert got["rouge_1"] > 0.0 and got["rouge_2"] > 0.0
        del forwards[:]
        with pytest.raises(ValueError, match="orders in 1..4"):
            trainer.evaluate_rouge(ds, cases._collate, 3, orders=(1, 5))
        with pytest.raises(ValueError, match="metrics must name"):
            trainer.evaluate_generation(ds, cases._collate, 3, metrics=("rouge_1", "rouge_3"))
        assert not forwards, "refused before anything is decoded"
        only = trainer.evaluate_generation(ds, cases._collate, 3, references="truths", remove_duplicates=True, metrics="rouge_2")
        assert only == dict(rouge_2=got["rouge_2"], items=4)
    finally:
        hook.remove()
    trainer.close()


# ---------------------------------------------------------------------------------------------
# 5. consensus under ROUGE-2
# ---------------------------------------------------------------------------------------------
def rouge_2_pick(pool, weights=None, valid=None):
    """``restated_pick`` of tests/test_consensus_cpu.py with the host's ROUGE-2 F as its pairwise utility: the function looks
    ``evaluation.rouge_l`` up when it is called, so the utility is handed to it there."""
    from case_rg_amd import evaluation
    keep = evaluation.rouge_l
    evaluation.rouge_l = lambda hyp, ref: evaluation.rouge_n(hyp, ref, 2)
    try:
        return restated_pick(pool, weights, valid)
    finally:
        evaluation.rouge_l = keep


def consensus_pools():
    """9 items x 7 candidates: noisy copies of one sentence per item, planted exact ties, an empty candidate, masks and weights."""
    rs = np.random.RandomState(438)
    B, N = 9, 7
    pools = []
    for _ in range(B):
        base = (rs.randint(0, 20, rs.randint(8, 30)) + FIRST).tolist()
        pools.append([[int(rs.randint(0, 20)) + FIRST if rs.rand() < 0.2 else t for t in base[:rs.randint(5, len(base) + 1)]] for _ in range(N)])
    q, z, w5 = [FIRST, FIRST + 1, FIRST + 2, FIRST + 3, FIRST + 4], [100, 101, 102], [200, 201]
    pools[0] = [z, [100, 102], q, q, w5, q, [201]]     # a planted exact tie between 2, 3 and 5, well ahead of the rest
    pools[1] = [w5, z, q, q, q, [100], [200]]          # the same three-fold copy: weights will move the pick to 0
    pools[2][4] = []                                   # an empty candidate counts as [UNK]
    valid = np.ones((B, N), dtype=bool)
    valid[3, [0, 5]] = False
    valid[4] = False                                   # an item without a valid candidate
    valid[0, 6] = False
    weights = rs.uniform(0.1, 1.0, (B, N)).astype(np.float32)
    weights[1] = (50.0, 1e-3, 1.0, 1.0, 1.0, 1e-3, 1e-3)
    return pools, valid, weights


def check_consensus(res, pools, weights=None, valid=None, tag="", picks=True):
    """``res``: consensus(..., metric="rouge_2") over ``pools`` (token lists, [UNK] for an empty one).  ``pairwise_rouge_2`` bitwise symmetric
    and at F_TOL, utilities at 1e-6 relative, -inf exactly where invalid, the pick the first maximum of the returned utilities and
    (``picks``) the restatement's pick.  As in tests/test_bleu_gpu.py, the f32 sums of K31 cannot order two candidates differently from the
    f64 restatement when their utilities are equal or at least 1e-5 apart; the inputs are checked to have no other kind of leading pair."""
    worst_f, worst_u = 0.0, 0.0
    assert torch.equal(res["pairwise_rouge_2"], res["pairwise_rouge_2"].transpose(1, 2)), "F(h, r) == F(r, h) bit for bit"
    util, index = to_np(res["consensus_utility"]).astype(np.float64), to_np(res["consensus_index"])
    pf = to_np(res["pairwise_rouge_2"]).astype(np.float64)
    for i, pool in enumerate(pools):
        u, at, f = rouge_2_pick(pool, None if weights is None else weights[i], None if valid is None else valid[i])
        worst_f = max(worst_f, float(np.abs(pf[i] - np.array(f)).max()))
        for n, un in enumerate(u):
            if un == -math.inf:
                assert util[i, n] == -math.inf, "item %d candidate %d is invalid and must read -inf" % (i, n)
            else:
                worst_u = max(worst_u, abs(util[i, n] - un) / max(abs(un), 1e-30))
        assert index[i] == int(np.argmax(util[i])), "item %d: index %d is not the first maximum of %s" % (i, index[i], util[i])
        if picks:
            ranked = sorted((x for x in u if x > -math.inf), reverse=True)
            lead = [x for x in ranked if x < ranked[0]] if ranked else []
            assert not lead or ranked[0] - lead[0] >= 1e-5, "item %d: the inputs leave a leading pair %.3e apart" % (i, ranked[0] - lead[0])
            assert index[i] == at, "item %d: picked %d, the restatement %d (utilities %s)" % (i, index[i], at, u)
    if tag:
        _note(tag + "_pairwise_rouge_2", worst_f, F_TOL)
        _note(tag + "_utility_rel", worst_u, 1e-6)
    print("consensus under ROUGE-2 %s: pairwise gap %.3e, utility gap %.3e relative" % (tag, worst_f, worst_u))
    assert worst_f <= F_TOL and worst_u <= 1e-6, (worst_f, worst_u)


def test_consensus_under_rouge_2_against_the_restatement():
    from case_rg_amd.evaluation import consensus
    pools, valid, weights = consensus_pools()
    B, N, T = len(pools), len(pools[0]), 40
    lists = [[p if p else [UNK] for p in pool] for pool in pools]
    cand = _dev(np.stack([_raw_rows(p, T) for p in pools]))
    with Calls() as c:
        plain = consensus(cand, SPECIALS, metric="rouge_2")
        masked = consensus(cand, SPECIALS, valid=_dev(valid), metric="rouge_2")
        weighted = consensus(cand, SPECIALS, valid=_dev(valid), weights=_dev(weights), metric="rouge_2")
    assert c.count("case_ngram_counts") == 3 and c.count("case_rouge_n_scores") == 3 and c.count("case_consensus_pick") == 3
    assert c.count("case_lcs_pairs") == 0 and c.count("case_ngram_distinct") == 0 and c.count("case_bleu_scores") == 0
    assert list(plain) == ["answer", "consensus_index", "consensus_utility", "pairwise_rouge_2"]
    assert plain["pairwise_rouge_2"].shape == (B, N, N) and plain["pairwise_rouge_2"].dtype == torch.float32
    check_consensus(plain, lists, tag="pick_uniform")
    check_consensus(masked, lists, valid=valid.tolist(), tag="pick_masked")
    check_consensus(weighted, lists, weights=weights.tolist(), valid=valid.tolist(), tag="pick_weighted")
    u = plain["consensus_utility"]
    assert int(plain["consensus_index"][0]) == 2 and float(u[0, 2]) == float(u[0, 3]) == float(u[0, 5])
    idx = to_np(masked["consensus_index"])
    assert all(valid[i, idx[i]] for i in range(B) if valid[i].any()) and idx[4] == 0
    for res in (plain, masked, weighted):
        assert torch.equal(res["answer"], cand[torch.arange(B, device="cuda"), res["consensus_index"]])
    # a one-token candidate has no bigram: 0 against everything, itself included; under ROUGE-1 it matches itself
    assert float(plain["pairwise_rouge_2"][0, 6, 6]) == 0.0 and abs(float(plain["pairwise_rouge_2"][0, 2, 2]) - 1.0) <= F_TOL
    first = consensus(cand, SPECIALS, metric="rouge_1")
    assert list(first)[-1] == "pairwise_rouge_1" and abs(float(first["pairwise_rouge_1"][0, 6, 6]) - 1.0) <= F_TOL
    assert torch.equal(first["pairwise_rouge_1"], first["pairwise_rouge_1"].transpose(1, 2))
    # "rouge_l" and "bleu" make the launches they made
    with Calls() as c:
        consensus(cand, SPECIALS)
        consensus(cand, SPECIALS, metric="bleu")
    assert c.calls == {"case_sentence_compact": 2, "case_lcs_pairs": 1, "case_ngram_counts": 1, "case_bleu_scores": 1, "case_consensus_pick": 2}


@pytest.mark.parametrize("name", ["sample_case", "sample_masque"])
def test_do_consensus_under_rouge_2_over_a_sample_pool(ns, name):
    m, b = sample_cases.build(ns, torch.device("cuda"), name)
    m.eval()
    B, T, N = sample_cases.ITEMS, sample_cases.T, 6
    rows = torch.arange(B, device="cuda")
    with torch.no_grad():
        plain = m.do_sample(dict(b), num_samples=N, seed=7)
        with Calls() as c:
            out = m.do_consensus(dict(b), pool="sample", metric="rouge_2", seed=7, num_samples=N)
        assert c.count("case_ngram_counts") == 1 and c.count("case_rouge_n_scores") == 1 and c.count("case_consensus_pick") == 1
        assert c.count("case_lcs_pairs") == 0 and c.count("case_ngram_distinct") == 0 and c.sampled == T, c.calls
        assert set(out) == {"rank", "samples", "sample_probs", "sample_scores", "answer", "consensus_index", "consensus_utility", "pairwise_rouge_2"}
        assert torch.equal(out["samples"], plain["samples"]), "the pool is do_sample's at the same seed"
        assert torch.equal(out["answer"], out["samples"][rows, out["consensus_index"]])
        lists = m.to_sentence(None, out["samples"].reshape(B * N, T))
        check_consensus(out, [lists[i * N:(i + 1) * N] for i in range(B)], tag=name + "_samples", picks=False)
        m.consensus_metric = "rouge_1"
        m.sampling = dict(num_samples=1, temperature=1.0, top_k=0, top_p=1.0, seed=7)
        m.consensus_samples = N
        routed = m(dict(b), method="consensus")
        assert "pairwise_rouge_1" in routed and torch.equal(routed["samples"], out["samples"])


def test_consensus_under_rouge_2_replays_from_a_captured_graph():
    """Nothing in consensus(metric="rouge_2") waits for the host: captured once, the replay on new candidates written into the same buffer is
    the eager call on them."""
    from case_rg_amd.evaluation import consensus
    pools, _, _ = consensus_pools()
    first = _dev(np.stack([_raw_rows(p, 40) for p in pools]))
    second = _dev(np.stack([_raw_rows(p[::-1], 40) for p in pools[::-1]]))
    keys = ("answer", "consensus_index", "consensus_utility", "pairwise_rouge_2")
    eager = {k: v.clone() for k, v in consensus(second, SPECIALS, metric="rouge_2").items()}
    buf = first.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        consensus(buf, SPECIALS, metric="rouge_2")  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph, static = torch.cuda.CUDAGraph(), {}
    with torch.cuda.graph(graph), Calls() as c:
        static.update(consensus(buf, SPECIALS, metric="rouge_2"))
    assert c.count("case_ngram_counts") == 1 and c.count("case_rouge_n_scores") == 1 and c.count("case_consensus_pick") == 1
    buf.copy_(second)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(static[k], eager[k]), "the replay differs from the eager call in %s" % k
    assert not torch.equal(eager["pairwise_rouge_2"], consensus(first, SPECIALS, metric="rouge_2")["pairwise_rouge_2"]), "the two candidate sets must differ"
    del graph
