"""BLEU and n-gram overlap on token ids, on the device.

``bleu.py`` beside this file is the host form (token lists, ``collections.Counter``).  Here the ids stay where the decoders left them, as in
``rouge_ids.py``: ``ops.sentence_compact`` applies ``to_sentence``'s filter, K34 (``ops.ngram_counts``) counts the clipped and the distinct
k-gram matches of every (hypothesis, reference) pair for k = 1..4, and K35 (``ops.bleu_scores``) turns the counts into sentence BLEU.
Nothing is read back to the host.

Conventions (``rouge_l_ids``'): an EMPTY HYPOTHESIS is the single token UNK; an EMPTY REFERENCE ROW is absent (a ragged number of ground
truths is padded with all-PAD rows).  Limits: hypotheses of at most 256 positions, ids in [0, 2^31)."""
import torch

from .. import ops
from .rouge_ids import _id_rows


def _orders(length, max_n):
    """length int32 [B, N] -> int64 [B, N, 4]: the number of k-grams max(length - k + 1, 0) for k <= max_n, 0 above."""
    k = torch.arange(ops.NGRAM_MAX_ORDER, device=length.device)
    total = (length.long().unsqueeze(-1) - k).clamp_min(0)
    return torch.where(k < max_n, total, torch.zeros_like(total))


def bleu_ids(hyp, ref, specials, max_n=4, smoothing="none", remove_duplicates=False):
    """hyp int64 [B, T] or [B, N, T], ref int64 [B, T'] or [B, M, T'] (raw ids on the device), specials = (bos, pad, eos, unk) ->
    dict(clip int32 [B, N, M, 4], clip_any int32 [B, N, 4], total int64 [B, N, 4], bleu_pair f32 [B, N, M], bleu f64 [B, N], bp f64 [B, N],
    ref_valid bool [B, M]).  ``bleu_pair[b, n, m]`` is ``bleu.sentence_bleu`` of hypothesis n against reference m alone, ``bleu[b, n]`` against
    all present references (``bp``: its brevity penalty); ``clip`` / ``clip_any`` are the numerators of the modified precisions of the orders
    1..4 and ``total`` their denominators before max(1, .).  An absent reference reads 0; an item without a present one has ``bleu`` 0.
    ``remove_duplicates``: the compacted HYPOTHESES go through ``remove_duplicate`` first (K33), as in ``rouge_l_ids``."""
    if smoothing not in ops.BLEU_SMOOTHINGS:
        raise ValueError("bleu_ids: smoothing must be 'none' or 'add1', not %r" % (smoothing,))
    a, a_len, b, b_len = _id_rows("bleu_ids", hyp, ref, specials, ops.NGRAM_MAX_T, remove_duplicates)
    counts = ops.ngram_counts(a, a_len, b, b_len, max_n)
    pair, bleu, bp = ops.bleu_scores(counts, a_len, b_len, max_n, smoothing)
    return dict(clip=counts["clip"], clip_any=counts["clip_any"], total=_orders(a_len, max_n), bleu_pair=pair, bleu=bleu, bp=bp,
                ref_valid=b_len.gt(0))


def eval_bleu_ids(hyp, ref, specials, max_n=4, smoothing="none", remove_duplicates=False):
    """hyp int64 [B, T], ref int64 [B, M, T'] (or [B, T']: one ground truth) -> f64 [B] on the device: per item the multi-reference sentence
    BLEU x 100 (0 for an item without a present reference).  Its mean rounded to 2 decimals is ``bleu.eval_bleu``'s number."""
    if hyp.dim() != 2:
        raise TypeError("eval_bleu_ids: hyp must be int64 [B, T], one answer per item")
    return bleu_ids(hyp, ref, specials, max_n, smoothing, remove_duplicates)["bleu"][:, 0] * 100


def ngram_overlap_ids(hyp, source, specials, max_n=4):
    """hyp int64 [B, T] or [B, N, T], source int64 [B, S] or [B, P, L] (raw ids) -> f64 [B, N, 4]: for k = 1..4 the share of the distinct
    k-grams of answer n that occur in the item's source, ``hit_any / distinct`` (0 where the answer has no k-gram, and above ``max_n``).
    Every source row is compacted on its own and k-grams do not span rows.  With one flat row this is Eval_Overlap.py's ratio exactly; with
    the passages as rows [B, P, L] it leaves out the few n-grams that the reference, which concatenates the passages of an item first,
    counts across a passage boundary."""
    a, a_len, b, b_len = _id_rows("ngram_overlap_ids", hyp, source, specials, ops.NGRAM_MAX_T, held=("answer", "answers"),
                                  streamed=("source", "source"))
    counts = ops.ngram_counts(a, a_len, b, b_len, max_n)
    distinct = counts["distinct"].double()
    return torch.where(distinct > 0, counts["hit_any"].double() / distinct.clamp_min(1), torch.zeros_like(distinct))
