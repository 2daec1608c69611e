"""Masque task model on the HIP path (reference: Masque/Model.py:13-286): CaSE minus supporting-token
identification; two losses (+ a passage-selection-only training mode)."""
import torch
import torch.nn as nn

from .. import ops
from ..common.Constants import BOS_WORD, EOS_WORD, UNK_WORD
from ..common.Interaction import Interaction
from ..common.TransformerSeqEncoderDecoder import PointerDecoderCore, TransformerSeqEncoder, decode_rules_param, no_repeat_ngram_param, sampling_params
from ..common.Utils import to_sentence
from ..common.heads import block_stack, nll_mean, passage_bce, run_block_pair
from ..evaluation.attribution import attribute_answers
from ..evaluation.risk import MRT_DEFAULTS, minimum_risk_step
from ..evaluation.rouge_ids import consensus_answers


class MasqueTransformerSeqDecoder(PointerDecoderCore):
    """Reference :13-119: additive-attention query = decoder state (H wide), gen on cat[dec_in, dec_out], one norm,
    ``extend`` always returns the summed distribution."""

    def __init__(self, num_memories, num_layers, nhead, tgt_vocab_size, hidden_size, emb_matrix=None):
        super().__init__()
        H = hidden_size
        self._build(num_memories, num_layers, nhead, tgt_vocab_size, H, H, emb_matrix=emb_matrix)
        self.norm = nn.LayerNorm(H)
        self.gen = nn.Sequential(nn.Linear(2 * H, H), nn.Linear(H, tgt_vocab_size, bias=False), nn.Softmax(dim=-1))
        self.mix = nn.Linear(3 * H, num_memories + 1)

    def extend(self, dec_outputs, gen_outputs, memory_weights, source_map):
        H = self.hidden_size
        d1, d2 = self._mix(dec_outputs[..., :H], [dec_outputs[..., H:2 * H], dec_outputs[..., 2 * H:]], gen_outputs,
                           memory_weights, source_map)
        return d1 + d2

    def _head_parts(self, dec_in, x, feat):
        dec_out = ops.layer_norm(x, self.norm.weight, self.norm.bias, self.norm.eps)
        return dec_out, torch.cat([dec_in, dec_out], dim=-1)

    def forward(self, encode_memories, BOS, UNK, source_map, encode_masks=None, encode_weights=None,
                groundtruth_index=None, init_decoder_state=None, max_target_length=None, beam_width=None, sampling=None, score_index=None,
                no_repeat_ngram=0, decode_rules=None, segments=None, score_grad_head=False, loss_only=False):
        return self._run(encode_memories, encode_masks, encode_weights, source_map, BOS, groundtruth_index, max_target_length, beam_width, sampling,
                         score_index, no_repeat_ngram=no_repeat_ngram, decode_rules=decode_rules, segments=segments, score_grad_head=score_grad_head,
                         loss_only=loss_only)


class PassageSelection(nn.Module):
    """Reference :121-159 (same network as CaSE's selection stage; returns bare tensors)."""

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

    def action(self, query, passage, encode_query=None, encode_passage=None):
        if encode_query is None:
            encode_query = self.query_encoder(query)[0][:, :, -1]
        if encode_passage is None:
            encode_passage = self.passage_encoder(passage)[0][:, :, -1]
        passage_mask, query_mask = passage.ne(0), query.ne(0)
        g_pq, g_qp = self.interaction(encode_query, encode_passage, query_mask, passage_mask)
        query_reps, passage_reps = run_block_pair(self.query_blocks, g_pq, query_mask, self.passage_blocks, g_qp, passage_mask)
        cls = passage_reps[:, :, 0].contiguous()
        score = ops.linear(cls, self.scorer.weight, self.scorer.bias, out_dtype=torch.float32).squeeze(-1)
        return score, query_reps, passage_reps


class ResponseGeneration(nn.Module):
    """Reference :161-200: passage prior = sigma(passage score) broadcast over its tokens."""

    def __init__(self, BOS, UNK, vocab_size, hidden_size, num_heads, query_encoder, passage_encoder, passage_selection, decoder):
        super().__init__()
        self.hidden_size = hidden_size
        self.vocab_size = vocab_size
        self.num_heads = num_heads
        self.query_encoder = query_encoder
        self.passage_encoder = passage_encoder
        self.passage_selection = passage_selection
        self.BOS = BOS
        self.UNK = UNK
        self.decoder = decoder

    def action(self, query, passage, source_map, encode_query=None, encode_passage=None, passage_selection_result=None,
               output=None, max_target_length=None, beam_width=None, sampling=None, score_index=None, no_repeat_ngram=0, decode_rules=None, segments=None,
               score_grad_head=False, loss_only=False):
        if encode_query is None:
            encode_query = self.query_encoder(query)[0][:, :, -1]
        if encode_passage is None:
            encode_passage = self.passage_encoder(passage)[0][:, :, -1]
        if passage_selection_result is None:
            passage_selection_result = self.passage_selection.action(query, passage, encode_query=encode_query,
                                                                     encode_passage=encode_passage)
        passage_score, query_rep, passage_rep = passage_selection_result
        B = query.size(0)
        prior_q = torch.ones(B, 1, query_rep.size(2), device=passage_score.device)
        prior_p = torch.sigmoid(passage_score).unsqueeze(-1).expand(-1, -1, passage_rep.size(2))
        return self.decoder([query_rep, passage_rep], self.BOS, self.UNK, source_map, groundtruth_index=output,
                            max_target_length=max_target_length, encode_masks=[query.ne(0), passage.ne(0)],
                            encode_weights=[prior_q, prior_p], beam_width=beam_width, sampling=sampling, score_index=score_index,
                            no_repeat_ngram=no_repeat_ngram, decode_rules=decode_rules, segments=segments, score_grad_head=score_grad_head,
                            loss_only=loss_only)


class Masque(nn.Module):
    def __init__(self, max_target_length, id2vocab, vocab2id, hidden_size, enc_layers=3, dec_layers=4, heads=8, early_stop=False):
        super().__init__()
        V = len(vocab2id)
        self.UNK = vocab2id[UNK_WORD]
        self.max_target_length = max_target_length
        self.query_encoder = TransformerSeqEncoder(enc_layers, heads, V, hidden_size)
        self.passage_encoder = self.query_encoder
        self.passage_selection = PassageSelection(hidden_size, heads, self.query_encoder, self.passage_encoder)
        self.response_generation = ResponseGeneration(vocab2id[BOS_WORD], vocab2id[UNK_WORD], V, hidden_size, heads,
                                                      self.query_encoder, self.passage_encoder, self.passage_selection,
                                                      MasqueTransformerSeqDecoder(2, dec_layers, heads, V, hidden_size))
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
        self.response_generation.decoder.beam_eos_id = vocab2id[EOS_WORD]
        if early_stop:  # greedy decoding ends once every answer of the batch has produced EOS (off = the reference's fixed T steps)
            self.response_generation.decoder.eos_id = vocab2id[EOS_WORD]

    def to_sentence(self, data, batch_indices):
        return to_sentence(batch_indices, self.id2vocab)

    def _encode_select(self, data):
        if self.query_encoder is self.passage_encoder:  # one shared encoder (reference :207-208): both inputs in one pass
            oq, op = self.query_encoder.forward_many([data['query'], data['passage']])
            eq, ep = oq[0][:, :, -1], op[0][:, :, -1]
        else:
            eq = self.query_encoder(data['query'])[0][:, :, -1]
            ep = self.passage_encoder(data['passage'])[0][:, :, -1]
        return eq, ep, self.passage_selection.action(data['query'], data['passage'], encode_query=eq, encode_passage=ep)

    def do_train(self, data):
        eq, ep, ps = self._encode_select(data)
        rows = self.response_generation.action(data['query'], data['passage'], data['source_map'], encode_query=eq,
                                               encode_passage=ep, passage_selection_result=ps, output=data['response'], loss_only=True)
        return self._stage_losses(data, ps) + [nll_mean(rows, data['response'])]

    @staticmethod
    def _stage_losses(data, ps):
        """The passage-selection loss of a training batch, from the stage's output: what ``do_train`` and ``do_mrt`` share."""
        return [0.25 * passage_bce(ps[0], data['passage_label'])]

    def do_mrt(self, data, candidates=None, num_samples=None, alpha=None, with_reference=None, dedup=None, mle_weight=None, details=False,
               **sampling):
        """Minimum-risk training on ROUGE-L over a sampled pool or explicit ``candidates`` (see CaSE.do_mrt and ``evaluation.risk``): the list
        ``do_train`` returns with the generation loss replaced by  mean risk + mle_weight x nll_ref;  ``details=True``: a dict with that list
        under ``losses`` plus ``risk``, ``q``, ``cost``, ``valid``, ``candidates`` and ``token_probs``.  The step runs without dropout: the module
        is in eval mode for the call and its previous mode is restored afterwards."""
        return minimum_risk_step(self, data, lambda: self._encode_select(data), lambda enc: self._stage_losses(data, enc[2]), candidates,
                                 num_samples, alpha, with_reference, dedup, mle_weight, details, **sampling)

    def do_ps_train(self, data):
        _, _, ps = self._encode_select(data)
        return [passage_bce(ps[0], data['passage_label'])]

    def _respond(self, data, _enc=None, **mode):
        """Encode, select, then the decoder in the mode the keyword names: (the decoder's raw result, rank)."""
        eq, ep, ps = self._encode_select(data) if _enc is None else _enc  # (do_attribute encodes once for two passes)
        rg = self.response_generation.action(data['query'], data['passage'], data['source_map'], encode_query=eq,
                                             encode_passage=ep, passage_selection_result=ps, output=None, **mode)
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

    do_infer = do_test

    def do_beam(self, data, width=None, no_repeat_ngram=None, min_length=None, banned_ids=None, length_penalty=None, _enc=None):
        """``do_test`` with beam search instead of the greedy argmax (the reference's common/Generations.py ``beam``): the ``do_test`` dict
        plus ``beam_score`` [B], ``beam_answers`` [B, W, T] and ``beam_scores`` [B, W] (see CaSE.do_beam, also for ``min_length`` / ``banned_ids`` /
        ``length_penalty``)."""
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
        ``min_length`` / ``banned_ids`` as in ``do_test`` (see CaSE.do_sample)."""
        sampling = sampling_params(self.vocab2id, num_samples, temperature, top_k, top_p, seed, uniforms)
        rg, rank = self._respond(data, _enc=_enc, max_target_length=self.max_target_length, sampling=sampling, no_repeat_ngram=self._ngram(no_repeat_ngram),
                                 decode_rules=self._rules(data, min_length, banned_ids))
        return {'answer': rg[3], 'rank': rank, 'samples': rg[4], 'sample_probs': rg[5], 'sample_scores': rg[6]}

    def do_consensus(self, data, pool="sample", candidates=None, valid=None, weights=None, no_repeat_ngram=None, metric=None, min_length=None,
                     banned_ids=None, length_penalty=None, **sampling):
        """Consensus (minimum-Bayes-risk) selection under ROUGE-L over a sample pool, a beam pool or explicit ``candidates`` (eval mode only;
        see CaSE.do_consensus): the pool's dict with ``answer`` replaced by the pick, plus ``consensus_index`` [B], ``consensus_utility``
        [B, N] and ``pairwise_f`` [B, N, N] (``metric="bleu"``: ``pairwise_bleu``, ``"rouge_1"`` / ``"rouge_2"``: ``pairwise_rouge_1`` / ``pairwise_rouge_2``; None: ``self.consensus_metric``).  ``min_length`` / ``banned_ids``
        (and ``length_penalty`` with ``pool="beam"``) go to the pool's decoder."""
        return consensus_answers(self, data, lambda d: self._encode_select(d)[2][0], pool, candidates, valid, weights,
                                 no_repeat_ngram=no_repeat_ngram, metric=metric, **self._pool_rules(pool, min_length, banned_ids, length_penalty), **sampling)

    @staticmethod
    def _pool_rules(pool, min_length, banned_ids, length_penalty):
        """The rule keywords ``do_consensus`` hands to its pool's decoder (None stays out: the pool's decoder then takes the attributes)."""
        if length_penalty is not None and pool != "beam":
            raise ValueError("do_consensus: length_penalty belongs to pool='beam'")
        given = dict(min_length=min_length, banned_ids=banned_ids, length_penalty=length_penalty)
        return {k: v for k, v in given.items() if v is not None}

    def do_score(self, data, answers=None):
        """The probability of given answers under the model (eval mode only; see CaSE.do_score): ``answers`` int64 [B, T'] or [B, N, T'],
        PAD (0) = not scored, default ``data['response']`` -> ``rank``, ``token_probs`` / ``copy_probs`` [B, N, T'], ``scores`` [B, N],
        ``loss`` [1] (``do_train``'s generation loss with dropout off) and ``tokens``."""
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
        return attribute_answers(self, data, lambda: self._encode_select(data), answers, trim_eos, **decode)

    def do_rank(self, data):
        """The passage ranking alone (eval mode only; see CaSE.do_rank): the encoders and the selection stage run, the decoder does not
        -> {'rank': [B, P]}, the bits of ``do_test(data)['rank']``."""
        if self.training:
            raise ValueError("do_rank runs in eval mode: call model.eval() first")
        return {'rank': self._encode_select(data)[2][0]}

    def forward(self, data, method='mle_train'):
        if method == 'train':
            return self.do_train(data)
        elif method == 'ps_train':
            return self.do_ps_train(data)
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
