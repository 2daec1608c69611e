"""ROUGE-L on token ids, on the device, and consensus (minimum-Bayes-risk) answer selection over a pool of decoded candidates.

``rouge.py`` beside this file is the host form (token strings, one numpy DP per pair, after a device-to-host copy).  Here the ids stay where
the decoders left them: ``ops.sentence_compact`` applies ``to_sentence``'s filter (drop BOS / PAD, cut at EOS), K30 (``ops.lcs_pairs``) gives
the LCS length and the F value of every (hypothesis, reference) pair, and K31 (``ops.consensus_pick``) picks, per item, the candidate with
the highest expected ROUGE-L against its pool.  Nothing is read back to the host, so a decoding pass followed by any of these still captures
into one graph.

Conventions: an EMPTY HYPOTHESIS is the single token UNK (``to_sentence``'s rule); an EMPTY REFERENCE ROW is absent (a ragged number of
ground truths is padded with all-PAD rows).  Limits: hypotheses of at most 256 positions, ids in [0, 2^31)."""
import torch

from .. import ops


def _compact(ids, bos, pad, eos, unk=None):
    """ids int64 [B, N, T] -> (front-packed ids [B, N, T], lengths int32 [B, N]); with ``unk`` an empty row becomes [UNK]."""
    B, N, T = ids.shape
    kept, count = ops.sentence_compact(ids.reshape(B * N, T), bos, pad, eos)
    if unk is not None:
        empty = count.eq(0)
        kept[:, 0] = torch.where(empty, torch.full_like(kept[:, 0], unk), kept[:, 0])
        count = count.clamp_min(1)
    return kept.view(B, N, T), count.view(B, N)


def _pool(who, ids, what):
    if not torch.is_tensor(ids) or ids.dtype != torch.int64 or ids.dim() not in (2, 3):
        raise TypeError("%s: %s must be an int64 tensor [B, T] or [B, N, T]" % (who, what))
    return ids.unsqueeze(1) if ids.dim() == 2 else ids


def _id_rows(who, hyp, ref, specials, max_t, remove_duplicates=False, held=("hypothesis", "hypotheses"), streamed=("reference", "ref")):
    """The operands of a metric on token ids from raw rows: hyp int64 [B, T] or [B, N, T] and ref int64 [B, T'] or [B, M, T'] of one batch, T <=
    max_t -> (a, a_len, b, b_len), compacted; an empty hypothesis becomes [UNK], and with ``remove_duplicates`` the compacted hypotheses go
    through ``remove_duplicate`` (K33).  ``held`` / ``streamed``: what the messages call the two sides (the latter with the argument's name)."""
    bos, pad, eos, unk = specials
    hyp, ref = _pool(who, hyp, "hyp"), _pool(who, ref, streamed[1])
    if hyp.shape[0] != ref.shape[0]:
        raise ValueError("%s: %d %s items, %d %s items" % (who, hyp.shape[0], held[0], ref.shape[0], streamed[0]))
    if hyp.shape[2] > max_t:
        raise ValueError("%s: %s of up to %d positions (got %d)" % (who, held[1], max_t, hyp.shape[2]))
    a, a_len = _compact(hyp, bos, pad, eos, unk)
    if remove_duplicates:
        ops.remove_duplicate_ids(a.view(-1, a.shape[2]), a_len.view(-1), 3, pad)
    return (a, a_len) + _compact(ref, bos, pad, eos)


def rouge_l_ids(hyp, ref, specials, remove_duplicates=False):
    """hyp int64 [B, T] or [B, N, T], ref int64 [B, T'] or [B, M, T'] (raw ids on the device, as the decoders and the batches hold them),
    specials = (bos, pad, eos, unk) -> dict(lcs int32, f f32, p f64, r f64: all [B, N, M]; ref_valid bool [B, M]).  f / p / r are
    ``rouge.rouge_l``'s of hypothesis n against reference m; an absent reference (``ref_valid`` False) reads 0 everywhere.
    ``remove_duplicates``: the compacted HYPOTHESES (not the references) go through the reference's ``remove_duplicate`` first (K33), as its
    ``save_result`` does before an answer is written or evaluated."""
    a, a_len, b, b_len = _id_rows("rouge_l_ids", hyp, ref, specials, ops.LCS_MAX_T, remove_duplicates)
    lcs, f = ops.lcs_pairs(a, a_len, b, b_len)
    n = lcs.double()
    return dict(lcs=lcs, f=f, p=n / a_len.double().unsqueeze(2), r=n / b_len.clamp_min(1).double().unsqueeze(1), ref_valid=b_len.gt(0))


def eval_rouge_l_ids(hyp, ref, specials, remove_duplicates=False):
    """hyp int64 [B, T], ref int64 [B, M, T'] (or [B, T']: one ground truth) -> f64 [B] on the device: per item the best F x 100 over its
    present references (0 for an item without one).  Its mean rounded to 2 decimals is ``rouge.eval_rouge_l``'s number (F is K30's f32
    rounding of the host's f64 value, so a per-item term is within 1.2e-5 of the host's).  ``remove_duplicates`` as in ``rouge_l_ids``: the number
    for the sentences after ``remove_duplicate``."""
    if hyp.dim() != 2:
        raise TypeError("eval_rouge_l_ids: hyp must be int64 [B, T], one answer per item")
    out = rouge_l_ids(hyp, ref, specials, remove_duplicates)
    f = out["f"][:, 0].double()
    return torch.where(out["ref_valid"], f, torch.zeros_like(f)).max(dim=1)[0] * 100


CONSENSUS_METRICS = ("rouge_l", "bleu", "rouge_1", "rouge_2")
_ROUGE_N_ORDER = {"rouge_1": 1, "rouge_2": 2}


def consensus(candidates, specials, valid=None, weights=None, metric="rouge_l"):
    """candidates int64 [B, N, T] (raw ids: ``do_sample``'s ``samples``, ``do_beam``'s ``beam_answers``), specials = (bos, pad, eos, unk),
    valid bool [B, N] (default: all), weights f32 [B, N] (default: uniform; e.g. a posterior exp(-len x sample_scores)) ->
    dict(answer int64 [B, T] = the raw row of the pick, consensus_index int64 [B], consensus_utility f32 [B, N], pairwise_f f32 [B, N, N]).
    The pick of item b maximises  sum_m w[b, m] F(candidate n as the hypothesis, m as the reference) / sum_m w[b, m]  over the valid
    candidates, the self term included, the lowest index on ties; an invalid candidate reads -inf and is never picked.
    ``metric="bleu"``: the utility F is sentence BLEU-4 with add-one smoothing (K34 + K35 on the pool against itself; unsmoothed sentence BLEU
    is 0 for most short pairs and useless as a utility), and the dict carries ``pairwise_bleu`` f32 [B, N, N] instead of ``pairwise_f``.
    ``metric="rouge_1"`` / ``"rouge_2"``: the utility is the reference's ROUGE-N F (K34 on the pool against itself -- its ``distinct`` is
    both |E| and |R|, a pool row fits K34 -- then K44), and the dict carries ``pairwise_rouge_1`` / ``pairwise_rouge_2`` instead."""
    bos, pad, eos, unk = specials
    if metric not in CONSENSUS_METRICS:
        raise ValueError("consensus: metric must be one of %s, not %r" % (CONSENSUS_METRICS, metric))
    if not torch.is_tensor(candidates) or candidates.dtype != torch.int64 or candidates.dim() != 3:
        raise TypeError("consensus: candidates must be an int64 tensor [B, N, T]")
    N, T = candidates.shape[1:]
    if not ops.consensus_supported(N, T):
        raise ValueError("consensus: pools of up to %d candidates of up to %d positions (got %d x %d)" % (ops.CONSENSUS_MAX_N, ops.LCS_MAX_T, N, T))
    kept, count = _compact(candidates, bos, pad, eos, unk)
    if metric == "bleu":
        f = ops.bleu_scores(ops.ngram_counts(kept, count, kept, count, 4), count, count, 4, "add1")[0]
    elif metric in _ROUGE_N_ORDER:
        order = _ROUGE_N_ORDER[metric]
        counts = ops.ngram_counts(kept, count, kept, count, order)
        f = ops.rouge_n_scores(counts["hit"], counts["distinct"], counts["distinct"], count, order)["f_pair"][..., order - 1].contiguous()
    else:
        _, f = ops.lcs_pairs(kept, count, kept, count)
    weights = None if weights is None else weights.to(device=candidates.device, dtype=torch.float32)
    utility, index, answer = ops.consensus_pick(f, weights, valid, candidates)
    return {"answer": answer, "consensus_index": index, "consensus_utility": utility, "pairwise_" + ("f" if metric == "rouge_l" else metric): f}


def model_specials(vocab2id):
    """(bos, pad, eos, unk) of a task model's vocabulary."""
    from ..common.Constants import BOS_WORD, EOS_WORD, PAD_WORD, UNK_WORD
    return tuple(vocab2id[w] for w in (BOS_WORD, PAD_WORD, EOS_WORD, UNK_WORD))


def consensus_answers(model, data, rank_of, pool="sample", candidates=None, valid=None, weights=None, no_repeat_ngram=None, metric=None,
                      **sampling):
    """``do_consensus`` of the task models (CaSE, Masque): build the pool with the model's own decoders (or take ``candidates``), then
    ``consensus``.  ``rank_of(data)``: the model's passage ranking from its encode stages alone.  ``no_repeat_ngram`` goes to the pool's decoder
    (None: the model's attribute); explicit candidates are taken as they are.  ``metric``: one of ``CONSENSUS_METRICS`` (None: the model's
    ``consensus_metric``), checked before anything is decoded."""
    if model.training:
        raise ValueError("do_consensus runs in eval mode: call model.eval() first")
    metric = model.consensus_metric if metric is None else metric
    if metric not in CONSENSUS_METRICS:
        raise ValueError("do_consensus: metric must be one of %s, not %r" % (CONSENSUS_METRICS, metric))
    if candidates is None and pool in ("sample", "beam"):
        sampling["no_repeat_ngram"] = no_repeat_ngram
    if candidates is not None:
        if sampling:
            raise TypeError("do_consensus: explicit candidates take no decoding arguments (%s)" % ", ".join(sorted(sampling)))
        out, pool_ids = {'rank': rank_of(data)}, candidates.to(data['query'].device)
    elif pool == "sample":
        params = dict(model.sampling, num_samples=model.consensus_samples)
        params.update(sampling)
        out = model.do_sample(data, **params)
        pool_ids = out['samples']
    elif pool == "beam":
        out = model.do_beam(data, **sampling)
        pool_ids = out['beam_answers']
        finite = torch.isfinite(out['beam_scores'])
        valid = finite if valid is None else finite & valid.to(finite.device).bool()
    else:
        raise ValueError("do_consensus: pool must be 'sample' or 'beam' (or give candidates), not %r" % (pool,))
    out.update(consensus(pool_ids, model_specials(model.vocab2id), valid=valid, weights=weights, metric=metric))
    return out
