"""METEOR on token ids, on the device.

``meteor.py`` beside this file is the host form (token lists, nltk's double loop) and states the rule.  Here the ids stay where the decoders
left them, as in ``rouge_ids.py`` and ``ngram_ids.py``: ``ops.sentence_compact`` applies ``to_sentence``'s filter and K40 (``ops.meteor``)
aligns every (hypothesis, reference) pair, counts matches and chunks and scores them.  Nothing is read back to the host.

Conventions (``rouge_l_ids``'): an EMPTY HYPOTHESIS is the single token UNK; an EMPTY REFERENCE ROW is absent (a ragged number of ground
truths is padded with all-PAD rows); an item without a present reference scores 0.  The comparison is over the models' token ids
(``bleu_ids``' deviation), and the stem / synonym stages are one caller-provided class table (``meteor.stem_classes`` builds one).  Limits:
hypotheses of at most 256 positions, ids in [0, 2^31)."""
from .. import ops
from .rouge_ids import _id_rows


def meteor_ids(hyp, ref, specials, classes=None, alpha=0.9, beta=3.0, gamma=0.5, remove_duplicates=False, want_align=False):
    """hyp int64 [B, T] or [B, N, T], ref int64 [B, T'] or [B, M, T'] (raw ids on the device), specials = (bos, pad, eos, unk) ->
    dict(matches, exact, chunks int32 [B, N, M], meteor_pair f32 [B, N, M], meteor f64 [B, N], best_ref int32 [B, N], ref_valid bool [B, M]
    and, with ``want_align``, align int32 [B, N, M, T]: the matched position of the COMPACTED reference per position of the compacted
    hypothesis, or -1).  ``meteor_pair[b, n, m]`` is ``meteor.sentence_meteor`` of hypothesis n against reference m alone, ``meteor[b, n]``
    against all present references and ``best_ref`` the lowest index that reaches it (-1 without a present reference, where ``meteor`` is
    0).  An absent reference reads 0.  ``classes``: int32 [V] on the ids' device for the second stage (None: exact matches only).
    ``remove_duplicates``: the compacted HYPOTHESES go through ``remove_duplicate`` first (K33), as in ``rouge_l_ids``."""
    a, a_len, b, b_len = _id_rows("meteor_ids", hyp, ref, specials, ops.METEOR_MAX_T, remove_duplicates)
    out = ops.meteor(a, a_len, b, b_len, classes, alpha, beta, gamma, want_align)
    counts = out.pop("counts")
    out.update(matches=counts[..., 0], exact=counts[..., 1], chunks=counts[..., 2], ref_valid=b_len.gt(0))
    return out


def eval_meteor_ids(hyp, ref, specials, classes=None, alpha=0.9, beta=3.0, gamma=0.5, remove_duplicates=False):
    """hyp int64 [B, T], ref int64 [B, M, T'] (or [B, T']: one ground truth) -> f64 [B] on the device: per item the multi-reference sentence
    METEOR x 100 (0 for an item without a present reference).  Its mean rounded to 2 decimals is ``meteor.eval_meteor``'s number."""
    if hyp.dim() != 2:
        raise TypeError("eval_meteor_ids: hyp must be int64 [B, T], one answer per item")
    return meteor_ids(hyp, ref, specials, classes, alpha, beta, gamma, remove_duplicates)["meteor"][:, 0] * 100
