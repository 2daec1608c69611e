"""CaSE task model on the HIP path (reference: CaSE/Model.py:13-339).

Module-attribute graph, constructor signatures and ``state_dict`` keys follow the reference (the shared encoder is
reachable under 16 prefixes, 1301 keys), so reference checkpoints load with ``strict=True``
and the reference's ``CumulativeTrainer`` / ``Run.py`` drive this class unchanged.  ``enc_layers`` /
``dec_layers`` / ``heads`` expose the counts the reference hard-codes (3 / 4 / 8).
"""
import torch
import torch.nn as nn

from .. import config, ops
from ..common.Constants import BOS_WORD, EOS_WORD, UNK_WORD
from ..common.Interaction import Interaction
from ..common.TransformerSeqEncoderDecoder import PointerDecoderCore, TransformerSeqEncoder, decode_rules_param, no_repeat_ngram_param, sampling_params
from ..common.Utils import to_sentence, token_freq_table
from ..common.heads import block_stack, nll_mean, passage_bce, run_block_pair, run_blocks
from ..evaluation.attribution import attribute_answers
from ..evaluation.risk import MRT_DEFAULTS, minimum_risk_step
from ..evaluation.rouge_ids import consensus_answers


class CaSETransformerSeqDecoder(PointerDecoderCore):
    """Two-memory pointer-generator decoder conditioned on the answer representation (reference :13-125)."""

    def __init__(self, num_memories, num_layers, nhead, tgt_vocab_size, hidden_size, emb_matrix=None):
        super().__init__()
        H = hidden_size
        self._build(num_memories, num_layers, nhead, tgt_vocab_size, H, 2 * H, emb_matrix=emb_matrix)
        self.norm1 = nn.LayerNorm(H)
        self.norm2 = nn.LayerNorm(H)
        self.gen = nn.Sequential(nn.Linear(3 * H, H), nn.Dropout(0.1), nn.Linear(H, tgt_vocab_size, bias=False), nn.Softmax(dim=-1))
        self.mix = nn.Linear(3 * H, num_memories + 1)

    def extend(self, dec_outputs, gen_outputs, memory_weights, source_map):
        """Public form of the mixing step (reference :38-48); ``dec_outputs`` is cat[dec_out, ctx_q, ctx_p]."""
        H = self.hidden_size
        d1, d2 = self._mix(dec_outputs[..., :H], [dec_outputs[..., H:2 * H], dec_outputs[..., 2 * H:]], gen_outputs,
                           memory_weights, source_map)
        return (d1, d2) if self.training else d1 + d2

    def _feature(self, answer_rep, T):
        """LN2(answer_rep) broadcast over the T decoder positions, dropout 0.1 in training (reference :69, :98)."""
        feat = ops.layer_norm(answer_rep, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        return ops.dropout(feat.unsqueeze(1).expand(-1, T, -1).contiguous(), 0.1, self.training)

    def _head_parts(self, dec_in, x, feat):
        dec_out = ops.layer_norm(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        return dec_out, torch.cat([dec_in, dec_out, feat], dim=-1)

    train_returns_pair = True

    @property
    def gen_dropout(self):
        return self.gen[1].p

    def forward(self, encode_memories, BOS, UNK, source_map, groundtruth_index=None, additional_decoder_feature=None,
                encode_weights=None, encode_masks=None, init_decoder_state=None, max_target_length=None, beam_width=None, sampling=None,
                score_index=None, no_repeat_ngram=0, decode_rules=None, segments=None, score_grad_head=False, loss_only=False):
        return self._run(encode_memories, encode_masks, encode_weights, source_map, BOS, groundtruth_index, max_target_length, beam_width, sampling,
                         score_index, feature_of=lambda T: self._feature(additional_decoder_feature, T), no_repeat_ngram=no_repeat_ngram,
                         decode_rules=decode_rules, segments=segments, score_grad_head=score_grad_head, loss_only=loss_only)


class RelevantPassageSelection(nn.Module):
    """Interaction -> 3 query / 5 passage TransformerBlocks -> Linear(H, 1) on [CLS]  (reference :127-163)."""

    def __init__(self, hidden_size, num_heads, query_encoder, passage_encoder):
        super().__init__()
        self.hidden_size = hidden_size
        self.query_encoder = query_encoder
        self.passage_encoder = passage_encoder
        self.num_heads = num_heads
        self.interaction = Interaction(hidden_size)
        self.query_blocks = block_stack(num_heads, hidden_size, 2)
        self.passage_blocks = block_stack(num_heads, hidden_size, 4)
        self.scorer = nn.Linear(hidden_size, 1)

    def action(self, query, passage, encode_query, encode_passage):
        eq, ep = encode_query[0][:, :, -1], encode_passage[0][:, :, -1]
        passage_mask, query_mask = passage.ne(0), query.ne(0)
        g_pq, g_qp = self.interaction(eq, ep, query_mask, passage_mask)
        query_reps, passage_reps = run_block_pair(self.query_blocks, g_pq, query_mask, self.passage_blocks, g_qp, passage_mask)
        cls = passage_reps[:, :, 0].contiguous()
        score = ops.linear(cls, self.scorer.weight, self.scorer.bias, out_dtype=torch.float32).squeeze(-1)
        return score, (query_reps, query_reps[:, :, 0]), (passage_reps, passage_reps[:, :, 0])


class SupportingTokenIdentification(nn.Module):
    """Second Interaction on the selection-stage reps -> 2 + 3 blocks -> per-token logit; reps refined by
    LN(stage1 + stage2)  (reference :165-212)."""

    def __init__(self, max_span_size, hidden_size, num_heads, query_encoder, passage_encoder, passage_selection):
        super().__init__()
        self.hidden_size = hidden_size
        self.num_heads = num_heads
        self.query_encoder = query_encoder
        self.passage_encoder = passage_encoder
        self.max_span_size = max_span_size
        self.passage_selection = passage_selection
        self.interaction = Interaction(hidden_size)
        self.query_blocks = block_stack(num_heads, hidden_size, 1)
        self.passage_blocks = block_stack(num_heads, hidden_size, 2)
        self.norm1 = nn.LayerNorm(hidden_size)
        self.norm2 = nn.LayerNorm(hidden_size)
        self.scorer = nn.Linear(hidden_size, 1)

    def action(self, query, passage, encode_query, encode_passage, passage_selection_result):
        passage_mask, query_mask = passage.ne(0), query.ne(0)
        _, query_rep, passage_rep = passage_selection_result
        g_pq, g_qp = self.interaction(query_rep[0], passage_rep[0], query_mask, passage_mask)
        query_reps, passage_reps = run_block_pair(self.query_blocks, g_pq, query_mask, self.passage_blocks, g_qp, passage_mask)
        token_score = ops.linear(passage_reps, self.scorer.weight, self.scorer.bias, out_dtype=torch.float32).squeeze(-1)
        token_score = token_score.masked_fill(~passage_mask, -1e6).clamp(min=-1e6, max=1e6)
        query_reps = ops.layer_norm(query_rep[0], self.norm1.weight, self.norm1.bias, self.norm1.eps, add=query_reps)
        passage_reps = ops.layer_norm(passage_rep[0], self.norm2.weight, self.norm2.bias, self.norm2.eps, add=passage_reps)
        return token_score, (query_reps, query_reps[:, :, 0]), (passage_reps, passage_reps[:, :, 0])


class ResponseGeneration(nn.Module):
    """Priors over the passage tokens + answer representation + decoder call (reference :214-253)."""

    def __init__(self, BOS, UNK, vocab_size, hidden_size, num_heads, query_encoder, passage_encoder, passage_selection,
                 span_extraction, decoder):
        super().__init__()
        self.hidden_size = hidden_size
        self.vocab_size = vocab_size
        self.num_heads = num_heads
        self.query_encoder = query_encoder
        self.passage_encoder = passage_encoder
        self.passage_selection = passage_selection
        self.span_extraction = span_extraction
        self.BOS = BOS
        self.UNK = UNK
        self.decoder = decoder

    @staticmethod
    def token_prior(passage_score, token_score):
        """sigma(passage) * sigma(token), normalised over all P*Lp tokens of an item (:239-241): [B, P*Lp] f32 scalars (glue).  The decoder
        weighs its copy attention by it, and ``CaSE.do_extract`` returns it."""
        prior = (torch.sigmoid(passage_score).unsqueeze(-1) * torch.sigmoid(token_score)).reshape(token_score.size(0), -1)
        return prior / (1e-8 + prior.sum(dim=-1, keepdim=True))

    def action(self, query, passage, source_map, encode_query, encode_passage, passage_selection_result,
               span_extraction_result, output=None, max_target_length=None, beam_width=None, sampling=None, score_index=None, no_repeat_ngram=0,
               decode_rules=None, segments=None, score_grad_head=False, loss_only=False):
        B = query.size(0)
        passage_score = passage_selection_result[0]
        token_score, query_rep, passage_rep = span_extraction_result
        H = passage_rep[0].size(-1)
        prior = self.token_prior(passage_score, token_score)
        mem = passage_rep[0].reshape(B, -1, H)
        answer_rep = ops.bmm(ops.cast_to(prior.unsqueeze(1), mem.dtype), mem, b_is_kn=True).squeeze(1)  # prior @ reps (:242)
        prior_p = prior.reshape_as(token_score)
        prior_q = torch.ones(B, 1, query_rep[0].size(2), device=prior.device)
        return self.decoder([query_rep[0], passage_rep[0]], self.BOS, self.UNK, source_map,
                            additional_decoder_feature=answer_rep, groundtruth_index=output,
                            max_target_length=max_target_length, encode_masks=[query.ne(0), passage.ne(0)],
                            encode_weights=[prior_q, prior_p], beam_width=beam_width, sampling=sampling, score_index=score_index,
                            no_repeat_ngram=no_repeat_ngram, decode_rules=decode_rules, segments=segments, score_grad_head=score_grad_head,
                            loss_only=loss_only)


class CaSE(nn.Module):
    def __init__(self, max_span_size, max_target_length, id2vocab, vocab2id, hidden_size, enc_layers=3, dec_layers=4, heads=8, early_stop=False):
        super().__init__()
        V = len(vocab2id)
        self.UNK = vocab2id[UNK_WORD]
        self.max_target_length = max_target_length
        self.query_encoder = TransformerSeqEncoder(enc_layers, heads, V, hidden_size)
        self.passage_encoder = self.query_encoder
        self.passage_selection = RelevantPassageSelection(hidden_size, heads, self.query_encoder, self.passage_encoder)
        self.span_extraction = SupportingTokenIdentification(max_span_size, hidden_size, heads, self.query_encoder,
                                                             self.passage_encoder, self.passage_selection)
        self.response_generation = ResponseGeneration(vocab2id[BOS_WORD], vocab2id[UNK_WORD], V, hidden_size, heads,
                                                      self.query_encoder, self.passage_encoder, self.passage_selection,
                                                      self.span_extraction,
                                                      CaSETransformerSeqDecoder(2, dec_layers, heads, V, hidden_size))
        self.id2vocab = id2vocab
        self.vocab_size = len(id2vocab)
        self.vocab2id = vocab2id
        self.beam_width = 4  # do_beam's default width
        self.sampling = dict(num_samples=1, temperature=1.0, top_k=0, top_p=1.0, seed=None)  # forward(data, method='sample') passes these to do_sample
        self.consensus_samples = 8  # do_consensus's default pool: this many samples per item
        self.consensus_metric = "rouge_l"  # do_consensus's default utility: "rouge_l" (K30), "bleu" (K34 + K35, BLEU-4 with add-one smoothing), "rouge_1" / "rouge_2" (K34 + K44)
        # K32: greedy, beam and sampled decoding never emit an n-gram a hypothesis already holds (0 = off; the reference only truncates
        # afterwards, ``remove_duplicate``).  The ``no_repeat_ngram=`` keyword of do_test / do_beam / do_sample / do_consensus overrides it.
        self.no_repeat_ngram = 0
        # Length and token rules of greedy, beam and sampled decoding (README "Length and token rules in decoding"); the keywords of do_test /
        # do_beam / do_sample / do_consensus override them.  min_length: no EOS before that many tokens (0 = off); banned_ids: ids that are never
        # emitted, [K] for every item or [B, K] per item (None = off); length_penalty: beam search ranks by cost / length^alpha (1.0 = the reference).
        self.min_length = 0
        self.banned_ids = None
        self.length_penalty = 1.0
        self.mrt = dict(MRT_DEFAULTS)  # do_mrt's defaults (evaluation.risk): num_samples, alpha, with_reference, dedup, mle_weight, temperature, top_k, top_p
        self.support_top_k = 32  # do_extract's default K: this many supporting tokens per item
        # the per-id frequency table of the token supervision (K37), installed by set_token_freq: it moves with .to() and is no state_dict key
        self.register_buffer("token_freq", None, persistent=False)
        self.response_generation.decoder.beam_eos_id = vocab2id[EOS_WORD]
        if early_stop:  # greedy decoding ends once every answer of the batch has produced EOS (off = the reference's fixed T steps)
            self.response_generation.decoder.eos_id = vocab2id[EOS_WORD]

    def to_sentence(self, data, batch_indices):
        return to_sentence(batch_indices, self.id2vocab)

    def _encode_select(self, data):
        if self.query_encoder is self.passage_encoder:  # one shared encoder (reference :262-263): both inputs in one pass
            eq, ep = self.query_encoder.forward_many([data['query'], data['passage']])
        else:
            eq, ep = self.query_encoder(data['query']), self.passage_encoder(data['passage'])
        return eq, ep, self.passage_selection.action(data['query'], data['passage'], encode_query=eq, encode_passage=ep)

    def _encode_select_extract(self, data):
        eq, ep, ps = self._encode_select(data)
        se = self.span_extraction.action(data['query'], data['passage'], encode_query=eq, encode_passage=ep,
                                         passage_selection_result=ps)
        return eq, ep, ps, se

    def set_token_freq(self, vocab_freq):
        """Install the per-id frequency table of the token supervision: a 1-D tensor of counts (the count of id v at [v]) or the reference's
        ``{id: count}`` dict; None removes it.  With it ``do_train`` and ``evaluate_extract`` label a batch that carries no ``token_label`` /
        ``token_weight`` on the device (K37)."""
        self.token_freq = None if vocab_freq is None else token_freq_table(vocab_freq, next(self.parameters()).device)
        return self

    def _token_labels(self, data, response=None, who="label_batch"):
        if self.token_freq is None:
            raise ValueError("%s: data carries no token_label / token_weight and no frequency table is installed to compute them from: "
                             "call set_token_freq(vocab_freq) first" % who)
        return ops.token_labels(data['passage'], data['response'] if response is None else response, self.token_freq)

    def label_batch(self, data, response=None):
        """A shallow copy of ``data`` with ``token_label`` and ``token_weight`` f32 [B, P, L] computed on the device (K37, ``common.Utils.
        token_label``'s rule) from ``data['passage']``, the table of ``set_token_freq`` and ``response`` int64 [B, T] (default
        ``data['response']``).  Any answer may be given -- a ``do_consensus`` pick, a rescored sample --: its non-PAD ids are the answer set
        as they stand, so the caller strips BOS / EOS where they should not count."""
        out = dict(data)
        out['token_label'], out['token_weight'] = self._token_labels(data, response)
        return out

    def _token_supervision(self, data):
        """(token_label, token_weight) of a training batch: the two entries of ``data``, or K37's where ``data`` carries neither."""
        has_label, has_weight = 'token_label' in data, 'token_weight' in data
        if has_label != has_weight:
            raise ValueError("do_train: data carries %s without %s: give both, or neither (they are then computed on the device, set_token_freq)" % (
                ("token_label", "token_weight") if has_label else ("token_weight", "token_label")))
        if has_label:
            return data['token_label'], data['token_weight']
        return self._token_labels(data, who="do_train")

    @staticmethod
    def _stage_losses(data, ps, se, token_label, token_weight):
        """The passage-selection and token-identification losses of a training batch, from the stages' outputs: what ``do_train`` and
        ``do_mrt`` share."""
        loss_ps = passage_bce(ps[0], data['passage_label'])
        valid = data['passage'].ne(0).float()
        bce = torch.nn.functional.binary_cross_entropy_with_logits(se[0], token_label.detach(), reduction='none')
        loss_se = (valid * bce * token_weight.detach()).sum() / valid.sum()
        return [loss_ps, loss_se]

    def do_train(self, data):
        token_label, token_weight = self._token_supervision(data)
        eq, ep, ps, se = self._encode_select_extract(data)
        loss_ps, loss_se = self._stage_losses(data, ps, se, token_label, token_weight)
        # the decoder's loss-only head: per-row NLL without a [rows, V] distribution where the fused head runs, the dense chain otherwise
        rows = self.response_generation.action(data['query'], data['passage'], data['source_map'], encode_query=eq,
                                               encode_passage=ep, passage_selection_result=ps, span_extraction_result=se,
                                               output=data['response'], loss_only=True)
        return [loss_ps, loss_se, nll_mean(rows, data['response'])]

    def do_mrt(self, data, candidates=None, num_samples=None, alpha=None, with_reference=None, dedup=None, mle_weight=None, details=False,
               **sampling):
        """Minimum-risk training on ROUGE-L (``evaluation.risk``): the expected  1 - ROUGE-L F  of a pool of candidates under the model's
        renormalised posterior  Q_n ~ p(candidate n)^alpha,  instead of the token-level NLL of ``do_train``.  The pool is ``num_samples``
        draws of ``do_sample`` (``**sampling``: ``temperature`` / ``top_k`` / ``top_p`` / ``uniforms`` / ``no_repeat_ngram`` / ``min_length`` /
        ``banned_ids``; drawn under no_grad from the global counter stream) or explicit ``candidates`` int64 [B, N, T]; with ``with_reference``
        ``data['response']`` joins as the last candidate; with ``dedup`` a candidate that repeats an earlier one is left out of the
        posterior.  The pool is scored teacher-forced with grad (K29 with row statistics and K41 where the build has them, the unfused
        chain otherwise).  ``mle_weight`` adds that multiple of the reference's NLL (``do_score``'s ``loss``; needs the reference).  None
        takes the value from ``self.mrt``.  At most 64 candidates (the reference included) of at most 256 positions.
        -> the list ``do_train`` returns with the generation loss replaced by  mean risk + mle_weight x nll_ref;  ``details=True``: a dict
        with that list under ``losses`` plus ``risk`` [B], ``q`` [B, N], ``cost`` [B, N], ``valid`` [B, N], ``candidates`` [B, N, T] (the pool
        as scored) and ``token_probs`` [B, N, T].  LIMIT: an MRT step runs WITHOUT DROPOUT -- the module is switched to eval mode (grad
        enabled) for the call and its previous mode is restored afterwards, also after an exception -- so a trainer that called
        ``model.train()`` drives it unchanged.  Nothing is read back."""
        token_label, token_weight = self._token_supervision(data)
        return minimum_risk_step(self, data, lambda: self._encode_select_extract(data),
                                 lambda enc: self._stage_losses(data, enc[2], enc[3], token_label, token_weight), candidates, num_samples, alpha,
                                 with_reference, dedup, mle_weight, details, **sampling)

    def _respond(self, data, _enc=None, **mode):
        """Encode, select, extract, then the decoder in the mode the keyword names: (the decoder's raw result, rank)."""
        eq, ep, ps, se = self._encode_select_extract(data) if _enc is None else _enc  # (do_attribute encodes once for two passes)
        rg = self.response_generation.action(data['query'], data['passage'], data['source_map'], encode_query=eq,
                                             encode_passage=ep, passage_selection_result=ps, span_extraction_result=se,
                                             output=None, **mode)
        return rg, ps[0]

    def _ngram(self, no_repeat_ngram):
        """The checked n-gram ban of a decoding call: the keyword, or the model's attribute when it is None."""
        return no_repeat_ngram_param(self.no_repeat_ngram if no_repeat_ngram is None else no_repeat_ngram, self.max_target_length)

    def _rules(self, data, min_length=None, banned_ids=None, length_penalty=None):
        """The checked decoding rules of a decoding call: the keywords, or the model's attributes where they are None."""
        return decode_rules_param(self.min_length if min_length is None else min_length, self.banned_ids if banned_ids is None else banned_ids,
                                  self.length_penalty if length_penalty is None else length_penalty, self.vocab2id, data['query'].size(0),
                                  self.max_target_length, device=data['query'].device)

    def do_test(self, data, no_repeat_ngram=None, min_length=None, banned_ids=None, _enc=None):
        """Greedy decoding.  ``no_repeat_ngram`` (None = ``self.no_repeat_ngram``; 0 = off): at every step the tokens that would complete an
        n-gram the answer already holds get probability 0 before the argmax (K32); max_target_length <= 256 with it on.  ``min_length`` /
        ``banned_ids`` (None = the model's attributes): no EOS among the first ``min_length`` tokens, and the listed ids ([K], or [B, K] per item)
        are never emitted -- their entries of the distribution are zeroed before the argmax, nothing is renormalised."""
        rg, rank = self._respond(data, _enc=_enc, max_target_length=self.max_target_length, no_repeat_ngram=self._ngram(no_repeat_ngram),
                                 decode_rules=self._rules(data, min_length, banned_ids))
        return {'answer': rg[3], 'rank': rank}

    do_infer = do_test  # BASELINE.json's wording

    def do_beam(self, data, width=None, no_repeat_ngram=None, min_length=None, banned_ids=None, length_penalty=None, _enc=None):
        """``do_test`` with beam search instead of the greedy argmax (the reference's common/Generations.py ``beam``: ``width`` hypotheses per
        item ranked by length-normalised cost, retired on EOS): the ``do_test`` dict plus ``beam_score`` [B] (the answer's cum_cost / length),
        ``beam_answers`` [B, W, T] and ``beam_scores`` [B, W] (the best W retired hypotheses, best first; +inf where there are fewer).
        ``min_length`` / ``banned_ids`` as in ``do_test``, for every slot of an item; ``length_penalty`` = alpha (None = the attribute; 1.0 = the
        reference) ranks candidates and retired hypotheses by cum_cost / length^alpha, and ``beam_score`` / ``beam_scores`` are those keys."""
        rg, rank = self._respond(data, _enc=_enc, max_target_length=self.max_target_length, beam_width=self.beam_width if width is None else width,
                                 no_repeat_ngram=self._ngram(no_repeat_ngram), decode_rules=self._rules(data, min_length, banned_ids, length_penalty))
        return {'answer': rg[3], 'rank': rank, 'beam_score': rg[5][:, 0], 'beam_answers': rg[4], 'beam_scores': rg[5]}

    def do_sample(self, data, num_samples=1, temperature=1.0, top_k=0, top_p=1.0, seed=None, uniforms=None, no_repeat_ngram=None, min_length=None,
                  banned_ids=None, _enc=None):
        """``do_test`` with every token DRAWN from the model's distribution (the reference's common/Generations.py ``sample`` loop; the draw is
        from the mixed pointer-generator distribution itself after ``temperature`` / ``top_k`` (0 = off) / ``top_p`` (1 = off), not from the
        reference's softmax of it): the ``do_test`` dict plus ``samples`` [B, N, T], ``sample_probs`` [B, N, T] (the model's unfiltered
        probability of each drawn token, 1 behind the end) and ``sample_scores`` [B, N] (mean -log p over the emitted non-PAD tokens);
        ``answer`` = samples[:, 0].  ``seed=None`` draws from the global counter stream (``config.next_rng``: new samples every pass, and on
        every replay of a captured pass when a device step state is installed; without one a replay repeats its samples); an integer seed
        gives a private, reproducible pass and leaves the global stream untouched.  ``uniforms`` f32 [T, B * N] is the kernel's ``uniforms`` override
        handed up one layer, beyond the reference's interface: a caller with a stream of its own (antithetic or common random numbers across
        models, a replayed draw) supplies u of row b N + n at step t as uniforms[t, b N + n]; it replaces ``seed`` and the counter generator.
        ``min_length`` / ``banned_ids`` as in ``do_test``, for every sample of an item, zeroed before the cuts and the draw; ``sample_probs``
        stay the model's own probabilities.  With ``min_length`` >= 1 the UNK-for-EOS convention of the first step can no longer fire."""
        sampling = sampling_params(self.vocab2id, num_samples, temperature, top_k, top_p, seed, uniforms)
        rg, rank = self._respond(data, _enc=_enc, max_target_length=self.max_target_length, sampling=sampling, no_repeat_ngram=self._ngram(no_repeat_ngram),
                                 decode_rules=self._rules(data, min_length, banned_ids))
        return {'answer': rg[3], 'rank': rank, 'samples': rg[4], 'sample_probs': rg[5], 'sample_scores': rg[6]}

    def do_consensus(self, data, pool="sample", candidates=None, valid=None, weights=None, no_repeat_ngram=None, metric=None, min_length=None,
                     banned_ids=None, length_penalty=None, **sampling):
        """Consensus (minimum-Bayes-risk) selection under ROUGE-L (eval mode only): the answer is the candidate of a pool with the highest
        expected ROUGE-L F against the pool, instead of the pool's slot 0.  ``pool="sample"``: ``do_sample`` with ``self.sampling`` overridden
        by ``**sampling`` (``num_samples`` defaults to ``self.consensus_samples``); ``pool="beam"``: ``do_beam`` (``width=`` may be given), the
        pool is ``beam_answers`` and the empty slots (``beam_scores`` = +inf) are invalid; explicit ``candidates`` int64 [B, N, T]: no decoding,
        only the encode stages run for ``rank``.  ``valid`` bool [B, N] and ``weights`` f32 [B, N] (default uniform; e.g. the posterior
        exp(-length x ``sample_scores``)) as in ``evaluation.consensus``.  N <= 64, T <= 256, ids < 2^31; an empty candidate counts as [UNK].
        -> the pool's dict with ``answer`` [B, T] replaced by the pick, plus ``consensus_index`` [B], ``consensus_utility`` [B, N] (-inf where
        invalid) and ``pairwise_f`` [B, N, N].  ``metric`` ("rouge_l", "bleu", "rouge_1" or "rouge_2"; None: ``self.consensus_metric``) chooses the utility; under
        "bleu" (sentence BLEU-4 with add-one smoothing) the matrix is returned as ``pairwise_bleu``.  Nothing is read back: with a sample pool
        at an integer ``seed`` the pass captures into one graph.  ``min_length`` / ``banned_ids`` (and ``length_penalty`` with ``pool="beam"``) go to
        the pool's decoder as ``no_repeat_ngram`` does (None: the model's attributes); explicit candidates take none of them."""
        return consensus_answers(self, data, lambda d: self._encode_select_extract(d)[2][0], pool, candidates, valid, weights,
                                 no_repeat_ngram=no_repeat_ngram, metric=metric, **self._pool_rules(pool, min_length, banned_ids, length_penalty), **sampling)

    @staticmethod
    def _pool_rules(pool, min_length, banned_ids, length_penalty):
        """The rule keywords ``do_consensus`` hands to its pool's decoder (None stays out: the pool's decoder then takes the attributes)."""
        if length_penalty is not None and pool != "beam":
            raise ValueError("do_consensus: length_penalty belongs to pool='beam'")
        given = dict(min_length=min_length, banned_ids=banned_ids, length_penalty=length_penalty)
        return {k: v for k, v in given.items() if v is not None}

    def do_score(self, data, answers=None):
        """What the model thinks of answers that already exist (eval mode only): ``answers`` int64 [B, T'] or [B, N, T'] with PAD (0) at
        the positions that are not scored -- the layout of ``data['response']`` (the default), of ``do_beam``'s ``beam_answers`` and of
        ``do_sample``'s ``samples``; T' is bounded by the decoder's position table, not by ``max_target_length``.  The encoder, selection and
        token-identification stages run once per item as in ``do_test``; the N candidates of an item are extra decoder rows (N x the memory
        footprint).  -> ``rank`` as in ``do_test``; ``token_probs`` f32 [B, N, T'] = p(y_t | y_<t, item) under the mixed pointer-generator
        distribution (1 where y_t is PAD); ``copy_probs`` its pointer part (0 where PAD); ``scores`` [B, N] = the mean over the non-PAD
        targets of -log max(p, 1e-30) (``sample_scores``' convention); ``loss`` [1] = ``do_train``'s generation loss with dropout off
        (sum of -log(p + 1e-8) over the non-PAD targets / their count); ``tokens`` = that count (int64 scalar).  A 2-D ``answers`` gives
        N = 1.  Under no_grad the head is K29 (no vocabulary row is built); with grad enabled the pass is differentiable."""
        if self.training:
            raise ValueError("do_score runs in eval mode: call model.eval() first")
        out, rank = self._respond(data, score_index=data['response'] if answers is None else answers)
        out['rank'] = rank
        return out

    def do_attribute(self, data, answers="test", trim_eos=None, **decode):
        """Where an answer came from (eval mode only): which part of the source every answer token was copied from, and the passage the
        answer cites.  ``answers``: "test" / "beam" / "sample" decode first in that mode (``**decode`` goes to it: ``width``, ``num_samples``,
        ``no_repeat_ngram``, ...) and the pool is ``answer[:, None]`` / ``beam_answers`` / ``samples``; "response" scores ``data['response']``;
        an int64 [B, T'] or [B, N, T'] tensor is scored as given.  The encode stages run once.  ``trim_eos``: the ids behind a row's first
        EOS become PAD before scoring (default: True for a decoded pool -- a fixed-T greedy pass keeps emitting behind EOS --, False
        otherwise).  -> everything ``do_score`` returns for the pool (``rank``, ``token_probs``, ``copy_probs``, ``scores``, ``loss``,
        ``tokens``), the decoded pool's own keys, and ``answers`` int64 [B, N, T'] (what was scored); ``copy_mass`` f32 [B, N, T', 1 + P]:
        the pointer mass of every token from the conversation context (segment 0) and from passage p of the pool (segment 1 + p: column p
        of ``rank``); ``copy_pos`` int32 [B, N, T']: the position, in ``data['source_map']`` coordinates, of the largest single term (-1:
        none), ``copy_pos_mass`` that term, ``copy_count`` int32 the source positions that hold the token; ``share`` f32 [B, N, T', 2 + P]:
        column 0 the generator, clamp(1 - sum_g mass_g / max(p, 1e-30), 0, 1), column 1 + g mass_g / max(p, 1e-30), 0 at PAD; ``support``
        f32 [B, N, 2 + P]: the mean share over the non-PAD positions; ``cited`` int64 [B, N]: the passage with the largest support as a
        pool index (the lowest among equals; -1 for an empty answer or no support).  The split is K39 (``ops.copy_attribution``) behind K29
        on the same operands; more than 63 passages, an unsorted source map, grad enabled or CASE_COPY_ATTRIBUTION=off take the host form.
        Nothing is read back: a pass at fixed arguments captures into one graph."""
        return attribute_answers(self, data, lambda: self._encode_select_extract(data), answers, trim_eos, **decode)

    def do_rank(self, data):
        """The passage ranking alone (eval mode only): the encoders and the selection stage run, the token-identification stage and the
        decoder do not -> {'rank': [B, P]}, the bits of ``do_test(data)['rank']``.  ``evaluation.rank_metrics_ids`` and
        ``CumulativeTrainer.evaluate_rank`` score it."""
        if self.training:
            raise ValueError("do_rank runs in eval mode: call model.eval() first")
        return {'rank': self._encode_select(data)[2][0]}

    def do_extract(self, data, top_k=None, select="prior", labels=None, ranking=False):
        """The supporting tokens alone (eval mode only): the encoders, the selection stage and the token-identification stage run, the
        decoder does not -> ``rank`` [B, P] (the bits of ``do_rank``); ``token_score`` f32 [B, P, L] (the stage's logits, -1e6 at PAD);
        ``token_prior`` f32 [B, P, L] (sigmoid(rank) x sigmoid(token_score) normalised over the item's P L tokens: the weights of the
        decoder's copy attention); and the K best non-PAD tokens of every item, best first (K38: key descending, then the lower position):
        ``support_pos`` int32 [B, K] (flat positions p L + l, -1 behind the item's non-PAD tokens), ``support_ids`` int64 [B, K] (``passage``
        there, PAD where the position is -1), ``support_value`` f32 [B, K] (the key there, 0 where the position is -1).  K = ``top_k``
        (None: ``self.support_top_k``), at most 256; P L <= 16384.  ``select="prior"`` ranks by ``token_prior``, ``"score"`` by
        ``token_score`` alone.  ``labels`` f32 [B, P, L] (e.g. ``token_label``): the same launch also counts, per item, ``counts`` int32
        [B, 5] = n_valid, n_pos, n_pred (token_score > 0), tp, hits (``ops.TOKEN_COUNTS``).  With ``labels`` and ``ranking=True`` one more
        launch (K45, on the key ``select`` names) adds the threshold-free figures of ``evaluation.token_rank``: ``token_ap`` and
        ``token_auc`` f64 [B], ``rank_counts`` int32 [B, 6] (``ops.TOKEN_RANK_COUNTS``) and ``best_threshold`` f32 [B].  Nothing is read
        back."""
        if self.training:
            raise ValueError("do_extract runs in eval mode: call model.eval() first")
        if select not in ("prior", "score"):
            raise ValueError("do_extract: select must be 'prior' or 'score', not %r" % (select,))
        if ranking and labels is None:
            raise ValueError("do_extract: ranking=True needs labels")
        K = int(self.support_top_k if top_k is None else top_k)
        B, P, L = data['passage'].shape
        if not 1 <= K <= ops.TOKEN_MAX_K or P * L > ops.TOKEN_MAX_L:
            raise ValueError("do_extract: 1 .. %d supporting tokens out of up to %d (got top_k %d, P x L = %d)" % (
                ops.TOKEN_MAX_K, ops.TOKEN_MAX_L, K, P * L))
        _, _, ps, se = self._encode_select_extract(data)
        token_score = se[0]
        prior = self.response_generation.token_prior(ps[0], token_score)
        flat_score = token_score.reshape(B, -1)
        key, valid = prior if select == "prior" else flat_score, data['passage'].ne(0).reshape(B, -1)
        picked = ops.token_select(key, valid, K, scores=None if labels is None else flat_score,
                                  labels=None if labels is None else labels.reshape(B, -1).float())
        pos = picked['pos']
        ids = data['passage'].reshape(B, -1).gather(1, pos.clamp(min=0).long()).masked_fill(pos < 0, 0)
        out = {'rank': ps[0], 'token_score': token_score, 'token_prior': prior.reshape_as(token_score), 'support_pos': pos,
               'support_ids': ids, 'support_value': picked['value']}
        if labels is not None:
            out['counts'] = picked['counts']
        if ranking:
            ranked = ops.token_rank(key, valid, labels.reshape(B, -1).float())
            out.update(token_ap=ranked['stats'][:, 0], token_auc=ranked['stats'][:, 1], rank_counts=ranked['counts'],
                       best_threshold=ranked['threshold'])
        return out

    def forward(self, data, method='mle_train'):
        # the reference expands data['source_map'] into a dense one-hot here (Utils.build_map, 15 GB at cfg 2);
        # the ids themselves feed the pointer scatter kernel instead
        if method == 'train':
            return self.do_train(data)
        elif method == 'mrt_train':
            return self.do_mrt(data)
        elif method == 'test':
            return self.do_test(data)
        elif method == 'beam':
            return self.do_beam(data)
        elif method == 'sample':
            return self.do_sample(data, **self.sampling)
        elif method == 'score':
            return self.do_score(data)
        elif method == 'consensus':
            return self.do_consensus(data)
        elif method == 'rank':
            return self.do_rank(data)
        elif method == 'attribute':
            return self.do_attribute(data)
        elif method == 'extract':
            return self.do_extract(data)
