"""K33, the reference's ``remove_duplicate`` on the device: ``sentence_compact`` + ``remove_duplicate_ids`` against the reference-generated
``sentences`` fixture and against the host ``Utils.remove_duplicate`` (which that fixture pins to the reference) on random rows, and the
``remove_duplicates`` flag of the id-level ROUGE-L against the host metric on the host-deduplicated sentences.  Ids and lengths are
compared exactly; F values at the id-ROUGE tests' bound (one f32 rounding of a value in [0, 1]: 1.2e-7, x 100 on the per-item number)."""
import numpy as np
import pytest
import torch

from helpers import load_golden, to_np

pytestmark = pytest.mark.gpu

F_TOL = 1.2e-7  # tests/test_consensus_gpu.py
PAD, BOS, EOS, UNK, FIRST = 0, 1, 2, 3, 4
SPECIALS = (BOS, PAD, EOS, UNK)


def _host_dedup(lists, n):
    from case_rg_amd.common.Utils import remove_duplicate
    sents = [list(x) for x in lists]
    remove_duplicate(sents, n)
    return sents


def _packed(lists, T, fill):
    ids = np.full((len(lists), T), fill, dtype=np.int64)
    for i, toks in enumerate(lists):
        ids[i, :len(toks)] = toks
    return ids, np.array([len(t) for t in lists], dtype=np.int32)


def test_compact_and_dedup_match_the_reference_fixture():
    from case_rg_amd import ops
    from case_rg_amd.common import Utils
    from case_rg_amd.utils import make_vocab
    import cases
    golden = load_golden("sentences")
    v2i, _ = make_vocab(cases.V)
    bos, eos, pad, unk = v2i["[unused0]"], v2i["[unused1]"], v2i["[PAD]"], v2i["[UNK]"]
    assert int(golden["unk"][0]) == unk
    ids = torch.from_numpy(golden["in_ids"]).cuda()
    kept, count = ops.sentence_compact(ids, bos, pad, eos)
    empty = count.eq(0)  # to_sentence's rule: an empty answer is [UNK]
    kept[:, 0] = torch.where(empty, torch.full_like(kept[:, 0], unk), kept[:, 0])
    count = count.clamp_min(1)
    before = [row[:n] for row, n in zip(kept.tolist(), count.tolist())]
    out, length = Utils.remove_duplicate_ids(kept, count)
    assert out.data_ptr() == kept.data_ptr() and length.data_ptr() == count.data_ptr(), "in place"
    rows, lens = out.tolist(), length.tolist()
    assert any(n < len(b) for n, b in zip(lens, before)), "the fixture cuts nothing"
    for r, (row, n) in enumerate(zip(rows, lens)):
        want = [int(x) for x in golden["deduplicated"][r] if x >= 0]
        assert row[:n] == want, "row %d: %s, the reference %s" % (r, row[:n], want)
        assert all(x == pad for x in row[n:]), "row %d: no PAD behind the new length: %s" % (r, row)
        assert [int(x) for x in golden["sentences"][r] if x >= 0] == before[r]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("T", [1, 3, 4, 64, 65, 256])
def test_random_rows_equal_the_host_remove_duplicate(T, n):
    """512 rows over an alphabet of 6 ids, every length 0 .. T; behind the length the rows hold ids that must not be read."""
    from case_rg_amd import ops
    rng = np.random.RandomState(1000 * n + T)
    lists = []
    for r in range(512):
        L = r % (T + 1) if r < 2 * (T + 1) else int(rng.randint(0, T + 1))
        # half the rows are periodic with a random head, so that long tails repeat and several passes cut
        if r % 2 and L > 4:
            head = rng.randint(FIRST, FIRST + 6, size=int(rng.randint(1, 5))).tolist()
            period = rng.randint(FIRST, FIRST + 6, size=int(rng.randint(1, 4))).tolist()
            lists.append((head + period * L)[:L])
        else:
            lists.append(rng.randint(FIRST, FIRST + 6, size=L).tolist())
    want = _host_dedup(lists, n)
    assert sum(len(w) < len(x) for w, x in zip(want, lists)) >= (8 if T > 4 else 0), "the host cuts too few rows for a test"
    ids, lens = _packed(lists, T, FIRST + 2)
    out, length = ops.remove_duplicate_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), n=n, pad=PAD)
    out, length = to_np(out), to_np(length)
    for r, w in enumerate(want):
        assert length[r] == len(w) and out[r, :len(w)].tolist() == w, "row %d of T %d n %d: %s (%d), host %s" % (r, T, n, out[r], length[r], w)
        assert (out[r, len(w):len(lists[r])] == PAD).all() and (out[r, len(lists[r]):] == FIRST + 2).all(), "row %d: the tail %s" % (r, out[r])


def test_argument_checks():
    from case_rg_amd import ops
    ids = torch.zeros(2, 257, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="256"):
        ops.remove_duplicate_ids(ids, torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="n must"):
        ops.remove_duplicate_ids(ids[:, :8].contiguous(), torch.zeros(2, dtype=torch.int32, device="cuda"), n=0)
    with pytest.raises(TypeError):
        ops.remove_duplicate_ids(ids[:, :8].contiguous(), torch.zeros(2, dtype=torch.int64, device="cuda"))


def test_id_rouge_with_remove_duplicates_is_the_host_number_on_deduplicated_sentences():
    """Hypotheses with looping tails against two references each: per item F x 100 within 1.2e-5 of the host's ROUGE-L on the sentences
    the host ``remove_duplicate`` leaves, the mean equal at the 2 decimals the evaluation prints; flag off: the numbers of the raw sentences,
    bit for bit what the call without the flag returns."""
    from case_rg_amd.evaluation import eval_rouge_l, eval_rouge_l_ids, rouge_l, rouge_l_ids
    rng = np.random.RandomState(77)
    B, T = 24, 40
    hyps, refs = [], []
    for i in range(B):
        body = rng.randint(FIRST, FIRST + 12, size=int(rng.randint(4, 12))).tolist()
        loop = body[-int(rng.randint(1, 4)):] * int(rng.randint(0, 6))
        hyps.append((body + loop)[:T - 3])
        refs.append([(body[:int(rng.randint(2, len(body) + 1))] + rng.randint(FIRST, FIRST + 12, size=3).tolist()),
                     rng.randint(FIRST, FIRST + 12, size=int(rng.randint(3, 10))).tolist()])
    hyps[0] = []  # an empty answer is [UNK], with or without the flag

    def raw(lists):
        out = np.zeros((len(lists), T), dtype=np.int64)
        for i, toks in enumerate(lists):
            row = [BOS] + list(toks) + [EOS, FIRST + 1]
            out[i, :len(row)] = row[:T]
        return out

    hyp = torch.from_numpy(raw(hyps)).cuda()
    ref = torch.from_numpy(np.stack([raw(r) for r in refs])).cuda()
    as_words = lambda toks: " ".join("w%d" % t for t in toks) if toks else "w%d" % UNK  # noqa: E731
    dedup = _host_dedup([h if h else [UNK] for h in hyps], 3)
    assert sum(len(d) < len(h) for d, h in zip(dedup, hyps)) >= 6, "too few hypotheses are cut"
    for flag, sents in ((True, dedup), (False, [h if h else [UNK] for h in hyps])):
        got = to_np(eval_rouge_l_ids(hyp, ref, SPECIALS, remove_duplicates=flag))
        want = np.array([100.0 * max(rouge_l(s, r)[0] for r in rs) for s, rs in zip(sents, refs)])
        worst = float(np.abs(got - want).max())
        print("remove_duplicates=%s: max |per-item F x 100 - host| = %.3e" % (flag, worst))
        assert worst <= 100 * F_TOL
        host = eval_rouge_l([as_words(s) for s in sents], [[as_words(r) for r in rs] for rs in refs])
        assert "%.2f" % round(float(got.mean()), 2) == "%.2f" % host
    off, default = rouge_l_ids(hyp, ref, SPECIALS, remove_duplicates=False), rouge_l_ids(hyp, ref, SPECIALS)
    for k in ("lcs", "f", "p", "r", "ref_valid"):
        assert torch.equal(off[k], default[k]), k
    on = rouge_l_ids(hyp, ref, SPECIALS, remove_duplicates=True)
    assert not torch.equal(on["lcs"], off["lcs"]) or not torch.equal(on["p"], off["p"]), "the flag changes nothing on looping answers"
