"""ROUGE-1 .. ROUGE-4 on token ids, on the device.

``rouge.py`` beside this file has the host form (``rouge_n``: Python sets of token tuples).  Here the ids stay where the decoders left them, as
in ``rouge_ids.py`` and ``ngram_ids.py``: ``ops.sentence_compact`` applies ``to_sentence``'s filter, K34 (``ops.ngram_counts``) gives, per order,
the distinct k-grams of every hypothesis and how many of them occur in every reference, K43 (``ops.ngram_distinct``) the distinct k-grams of
every reference row, whatever its length, and K44 (``ops.rouge_n_scores``) the reference's F / P / R from those three integers.  Nothing is
read back to the host.

Conventions (``rouge_l_ids``'): an EMPTY HYPOTHESIS is the single token UNK; an EMPTY REFERENCE ROW is absent (a ragged number of ground
truths is padded with all-PAD rows).  Limits: hypotheses of at most 256 positions, ids in [0, 2^31); references of any length, at a cost
that grows with the square of the length (K43)."""
import torch

from .. import ops
from .rouge_ids import _id_rows


def rouge_n_ids(hyp, ref, specials, max_n=2, remove_duplicates=False):
    """hyp int64 [B, T] or [B, N, T], ref int64 [B, T'] or [B, M, T'] (raw ids on the device), specials = (bos, pad, eos, unk) ->
    dict(hit int32 [B, N, M, 4], hyp_distinct int32 [B, N, 4], ref_distinct int32 [B, M, 4], f_pair f32 [B, N, M, 4], f / p / r f64
    [B, N, 4], best_ref int32 [B, N, 4], ref_valid bool [B, M]), the order k = 1..4 on the last axis.  ``f_pair[b, n, m, k - 1]`` is
    ``rouge.rouge_n(.., .., k)``'s F of hypothesis n against reference m (f64 rounded once; 0 for an absent reference); ``f`` / ``p`` / ``r``
    are the values against the present reference with the largest F, ``best_ref`` its index (the lowest among equals; -1 and zeros for an
    item without a present reference).  The orders above ``max_n`` read 0 everywhere and ``best_ref`` -1.
    ``remove_duplicates``: the compacted HYPOTHESES go through ``remove_duplicate`` first (K33), as in ``rouge_l_ids``."""
    if not isinstance(max_n, int) or isinstance(max_n, bool) or not 1 <= max_n <= ops.NGRAM_MAX_ORDER:
        raise ValueError("rouge_n_ids: max_n in 1..%d (got %r)" % (ops.NGRAM_MAX_ORDER, max_n))
    a, a_len, b, b_len = _id_rows("rouge_n_ids", hyp, ref, specials, ops.NGRAM_MAX_T, remove_duplicates)
    counts = ops.ngram_counts(a, a_len, b, b_len, max_n)
    ref_distinct = ops.ngram_distinct(b, b_len, max_n)
    out = ops.rouge_n_scores(counts["hit"], counts["distinct"], ref_distinct, b_len, max_n)
    out.update(hit=counts["hit"], hyp_distinct=counts["distinct"], ref_distinct=ref_distinct, ref_valid=b_len.gt(0))
    return out


def check_orders(orders, what):
    """-> the orders as a tuple of ints; ``ValueError`` for one outside 1..4."""
    orders = (orders,) if isinstance(orders, int) else tuple(orders)
    if any(not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= ops.NGRAM_MAX_ORDER for k in orders):
        raise ValueError("%s: orders in 1..%d (got %r)" % (what, ops.NGRAM_MAX_ORDER, orders))
    return orders


def eval_rouge_n_ids(hyp, ref, specials, orders=(1, 2), remove_duplicates=False):
    """hyp int64 [B, T], ref int64 [B, M, T'] (or [B, T']: one ground truth) -> f64 [B, len(orders)] on the device: per item and per order of
    ``orders`` the best F x 100 over its present references (0 for an item without one).  The column means rounded to 2 decimals are
    ``rouge.eval_rouge``'s ROUGE_1_F1 / ROUGE_2_F1 for ``orders=(1, 2)``."""
    if not torch.is_tensor(hyp) or hyp.dim() != 2:
        raise TypeError("eval_rouge_n_ids: hyp must be int64 [B, T], one answer per item")
    orders = check_orders(orders, "eval_rouge_n_ids")
    if not orders:
        raise ValueError("eval_rouge_n_ids: at least one order")
    f = rouge_n_ids(hyp, ref, specials, max(orders), remove_duplicates)["f"][:, 0]
    return torch.stack([f[:, k - 1] for k in orders], dim=1) * 100  # (slices, no index tensor: nothing crosses to the device)
