"""Sequence encoder and pointer-generator decoders on the HIP path.

Reference: common/TransformerSeqEncoderDecoder.py:14-45 (encoder), :47-150 (generic decoder);
CaSE/Model.py:13-125 and Masque/Model.py:13-119 hold the two task-specific decoder variants, which share
``PointerDecoderCore`` here.

Differences from the reference that do not change results:
  * the copy distribution is a scatter-add over the source *ids* (kernel K11) instead of a dense bmm with a
    [B, S, V] one-hot map (15-40 GB at the BASELINE sizes); a dense map is still accepted for API compatibility;
  * greedy decoding keeps the reference's step semantics (argmax of the last position, lowest index on ties, fixed
    T steps) but projects each memory's K/V and additive-attention keys once instead of once per step.
"""
import operator
import os

import torch
import torch.nn as nn

from .. import config, ops
from ..evaluation.attribution import copy_attribution_host
from .BilinearAttention import BilinearAttention
from .PositionalEmbedding import PositionalEmbedding
from .TransformerDecoder import TransformerDecoder, TransformerDecoderLayer
from .TransformerEncoder import TransformerEncoder, TransformerEncoderLayer
from .Utils import generate_square_subsequent_mask

MERGED_ENCODE = os.environ.get("CASE_MERGED_ENCODE", "1") != "0"  # A/B switch of TransformerSeqEncoder.forward_many
QUERY_SPLIT = os.environ.get("CASE_QUERY_SPLIT", "1") != "0"  # A/B switch: the greedy step projects x_t alone for the additive-attention query


def _embedding(vocab, width, max_len=1000, emb_matrix=None):
    """Embedding + position pair.  ``emb_matrix`` [V, H]: a pre-trained table, loaded and frozen as the reference's
    ``create_emb_layer`` does (common/Utils.py:250-256: ``non_trainable=True``)."""
    if emb_matrix is not None:
        vocab, width = emb_matrix.shape
    table = nn.Embedding(vocab, width, padding_idx=0)
    if emb_matrix is not None:
        table.load_state_dict({"weight": emb_matrix})
        table.weight.requires_grad = False
    return nn.Sequential(table, PositionalEmbedding(width, dropout=0.1, max_len=max_len))


def _embed(seq, ids, training):
    """Fused gather * sqrt(H) + position (+dropout) through the nn.Sequential(Embedding, PositionalEmbedding) pair."""
    table, pos = seq[0].weight, seq[1]
    if ids.shape[-1] > pos.pe.size(0):
        raise RuntimeError("sequence length %d exceeds max_len %d" % (ids.shape[-1], pos.pe.size(0)))
    return ops.embed_pos(ids, table, pos.pe, p_drop=config.drop_p(pos.p, training))


class TransformerSeqEncoder(nn.Module):
    def __init__(self, num_layers, num_heads, src_vocab_size, hidden_size, emb_matrix=None, norm=None):
        super().__init__()
        self.num_layers, self.num_heads = num_layers, num_heads
        self.embedding = _embedding(src_vocab_size, hidden_size, emb_matrix=emb_matrix)
        layer = TransformerEncoderLayer(hidden_size, nhead=num_heads, dim_feedforward=hidden_size, dropout=0.1, activation='gelu')
        self.enc = TransformerEncoder(layer, num_layers=num_layers, norm=norm)

    def forward(self, batch_numseq_seqlen):
        """ids [B, N, L] -> (out [B, N, 1, L, H], state [B, N, 1, H])."""
        B, N, L = batch_numseq_seqlen.shape
        ids = batch_numseq_seqlen.reshape(B * N, L)
        valid = ids.ne(0)
        x = _embed(self.embedding, ids, self.training)
        y = self.enc.forward_batch_first(x, valid)
        state = ops.masked_mean(y, valid)
        return y.reshape(B, N, L, -1).unsqueeze(2), state.reshape(B, N, -1).unsqueeze(2)


    def forward_many(self, id_tensors):
        """Several inputs through the SAME encoder in one pass (the reference's models share one encoder between query and passages:
        CaSE/Model.py:262-263, Masque/Model.py:207-208): embeddings of all inputs back to back in one [rows, H] buffer, every
        row-local op of every layer launched once, the attention core once per input.  Returns what ``forward`` returns, per input;
        the training path's ~120 launches on the 2048 query rows ride along with the 122 880 passage rows, and the shared
        parameters receive ONE gradient instead of two that autograd adds.  Falls back to separate passes where the grouped attention
        does not apply (f32 parity mode, the inference chain, unfused mode)."""
        dt = config.compute_dtype()
        needs_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if (not MERGED_ENCODE or len(id_tensors) < 2 or not needs_grad or not self.enc.rows_supported(dt, needs_grad)
                or not all(t.is_cuda for t in id_tensors)):
            return [self.forward(t) for t in id_tensors]
        xs, groups, valids, shapes, r0 = [], [], [], [], 0
        for t in id_tensors:
            B, N, L = t.shape
            ids = t.reshape(B * N, L)
            xs.append(_embed(self.embedding, ids, self.training).reshape(B * N * L, -1))
            groups.append((r0, B * N, L))
            valids.append(ids.ne(0))
            shapes.append((B, N, L))
            r0 += B * N * L
        y = self.enc.forward_rows(torch.cat(xs, dim=0), groups, valids)
        outs = []
        for yi, valid, (B, N, L) in zip(ops.split_rows(y, groups), valids, shapes):
            state = ops.masked_mean(yi, valid)
            outs.append((yi.reshape(B, N, L, -1).unsqueeze(2), state.reshape(B, N, -1).unsqueeze(2)))
        return outs


def sampling_params(vocab2id, num_samples=1, temperature=1.0, top_k=0, top_p=1.0, seed=None, uniforms=None):
    """The checked ``sampling`` argument of the pointer decoders (what the task models' ``do_sample`` hands down)."""
    from .Constants import EOS_WORD, PAD_WORD, UNK_WORD
    if int(num_samples) != num_samples or num_samples < 1:
        raise ValueError("do_sample: num_samples must be an integer >= 1, not %r" % (num_samples,))
    if not float(temperature) > 0.0:
        raise ValueError("do_sample: temperature must be > 0, not %r" % (temperature,))
    if int(top_k) != top_k or top_k < 0:
        raise ValueError("do_sample: top_k must be an integer >= 0 (0 = off), not %r" % (top_k,))
    if not 0.0 < float(top_p) <= 1.0:
        raise ValueError("do_sample: top_p must lie in (0, 1] (1 = off), not %r" % (top_p,))
    return dict(num_samples=int(num_samples), temperature=float(temperature), top_k=int(top_k), top_p=float(top_p),
                seed=None if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF, uniforms=uniforms,
                eos=vocab2id[EOS_WORD], unk=vocab2id[UNK_WORD], pad=vocab2id[PAD_WORD])


def no_repeat_ngram_param(n, max_target_length=None):
    """The checked ``no_repeat_ngram`` of the decoders and the task models: an integer >= 0 (0 = off).  With the ban on, a pass is limited to
    ``ops.NGRAM_MAX_T`` steps (K32 stages a row's history in LDS beside the vocabulary row).  n > max_target_length is legal and bans nothing."""
    try:
        n = None if isinstance(n, bool) else operator.index(n)
    except TypeError:
        n = None
    if n is None or n < 0:
        raise ValueError("no_repeat_ngram must be an integer >= 0 (0 = off)")
    if n and max_target_length is not None and max_target_length > ops.NGRAM_MAX_T:
        raise ValueError("no_repeat_ngram: the ban covers passes of up to %d steps (max_target_length %d)" % (ops.NGRAM_MAX_T, max_target_length))
    return n


def decode_rules_param(min_length, banned_ids, length_penalty, vocab2id, B, max_target_length, device=None):
    """The checked decoding rules of the decoders and the task models, in their device-ready form (made once per pass, not per step):
    ``min_length`` an integer in [0, max_target_length - 1] (0 = off: EOS gets probability 0 at the steps t < min_length, and the last position can
    always hold EOS); ``banned_ids`` None (off) or an integer tensor / sequence [K] (every item) or [B, K] (one list per item), K <=
    ``ops.RULES_MAX_BANNED``, entries outside the vocabulary ignored (-1 pads a ragged list), duplicates legal, EOS refused (that is what
    ``min_length`` is for); ``length_penalty`` a finite float >= 0 (1.0 = the reference's cost / length ranking of beam search).
    -> dict(min_length, banned int32 tensor on ``device`` | None, length_penalty, eos); ``on`` says whether a row rule is set.
    A pass that is captured into a graph takes ``banned_ids`` as a device tensor (a host list would need a host-to-device copy inside the
    capture); its EOS check is one read-back, made by every call outside a capture -- the warm-up pass included -- and skipped while the
    stream captures."""
    from .Constants import EOS_WORD
    eos = vocab2id[EOS_WORD]
    try:
        m = None if isinstance(min_length, bool) else operator.index(min_length)
    except TypeError:
        m = None
    if m is None or m < 0:
        raise ValueError("min_length must be an integer >= 0 (0 = off)")
    if max_target_length is not None and m > max_target_length - 1:
        raise ValueError("min_length %d leaves no position for EOS within max_target_length %d" % (m, max_target_length))
    try:
        alpha = None if isinstance(length_penalty, bool) else float(length_penalty)
    except (TypeError, ValueError):
        alpha = None
    if alpha is None or not (alpha >= 0.0) or alpha == float("inf"):
        raise ValueError("length_penalty must be a finite float >= 0 (1.0 = cost / length)")
    banned = None
    if banned_ids is not None:
        try:
            banned = banned_ids.detach() if torch.is_tensor(banned_ids) else torch.as_tensor(banned_ids)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError("banned_ids must be an integer tensor or sequence [K] or [B, K]")
        if banned.numel() == 0 and banned.dim() <= 2:
            banned = None
        else:
            if banned.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
                raise ValueError("banned_ids must hold integers, not %s" % banned.dtype)
            if banned.dim() not in (1, 2) or (banned.dim() == 2 and banned.shape[0] != B):
                raise ValueError("banned_ids must be [K] or [B, K] with the batch's B = %d, not %s" % (B, list(banned.shape)))
            if banned.shape[-1] > ops.RULES_MAX_BANNED:
                raise ValueError("banned_ids: at most %d ids per item (got %d)" % (ops.RULES_MAX_BANNED, banned.shape[-1]))
            # (one read-back for a device tensor; a capturing stream cannot read back, and the warm-up pass a capture needs has made the check)
            if not (banned.is_cuda and torch.cuda.is_current_stream_capturing()) and bool(banned.eq(eos).any()):
                raise ValueError("banned_ids must not hold EOS (%d): use min_length to keep an answer from ending" % eos)
            banned = banned.to(device=device, dtype=torch.int32).contiguous()
    return dict(min_length=m, banned=banned, length_penalty=alpha, eos=eos, on=bool(m or banned is not None))


class _DecodeMode:
    """What differs between the decoding modes of ``PointerDecoderCore._decode``: how a step's head becomes the next ids [R, 1]
    (``fused_step`` from the f32 logits, mixing logits, sorted source map and copy weights [R, len_k]; ``unfused_step`` from the unfused
    ``gen`` / ``dist``), what happens between two steps, when the pass may end early and what it returns.  The rows of one item are
    consecutive: row b * N + n is candidate n (beam slot, sample) of item b."""
    counter = None  # the decoder attribute that receives the number of steps the pass ran: last_greedy_steps / last_beam_steps / last_sample_steps
    ngram = 0  # no_repeat_ngram (K32): 0 = off, the launches of a pass without it
    rules = None  # min_length / banned ids (an ops.RowRules at t = 0): None = off, the launches of a pass without them

    def _set_rules(self, rules, rows_per_item):
        """``rules``: what ``decode_rules_param`` returned (or None).  The pass's RowRules, made once; a step takes ``_rules_at(t)``."""
        if rules is not None and rules["on"]:
            self.rules = ops.row_rules(rules["eos"], rules["min_length"], rules["banned"], rows_per_item)

    def _rules_at(self, t):
        return None if self.rules is None else self.rules._replace(t=t)

    def _banned_copy(self, dist, hist, t, eos, ended=None):
        """The unfused head with the ban or the rules on: a float copy of the newest position's distribution with the banned entries zeroed (K32
        first, then the rules, as the fused heads do)."""
        row = dist[:, -1].detach().to(torch.float32, copy=True)
        if self.ngram:
            ops.ngram_ban_(row, hist, t, self.ngram, eos, ended)
        if self.rules is not None:
            ops.row_rules_(row, self._rules_at(t), ended)
        return row

    def start(self, capturing, self_kvs, hist_valid):
        pass

    def after_step(self, t, self_kvs, hist_valid):
        """Between step ``t`` and step t + 1 (not after the last step): -> the self-attention caches and prefix validity of step t + 1."""
        return self_kvs, hist_valid


class _GreedyMode(_DecodeMode):
    """Argmax of the newest position with the lowest index on ties (the reference's CaSE/Model.py:94-123): K23, or ``row_argmax`` on the
    unfused distribution.  With the decoder's ``eos_id`` set (the EOS-aware early stop) a finished answer is continued with PAD
    (to_sentence stops at EOS anyway) and the pass may end once EVERY answer of the batch has produced EOS; None is the reference's
    behaviour, always max_target_length steps (CaSE/Model.py:94).  K23 writes gen / dist back for the LAST step only (what the caller
    gets): on step T - 1, or on any step when the early stop is armed and the stream is not capturing -- then any step may turn out to be
    the last one.  -> (dec_out, gen, dist of the last step, answer [B, T], PAD behind a short pass)."""
    counter = "last_greedy_steps"

    def __init__(self, decoder, B, T, dev, ngram=0, rules=None):
        self.T, self.V, self.eos, self.ngram = T, decoder.tgt_vocab_size, decoder.eos_id, ngram
        self._set_rules(rules, 1)
        self.hist = torch.zeros(B, T, dtype=torch.int32, device=dev) if ngram else None  # K23 appends its argmax at [:, t]
        self.finished = None if self.eos is None else torch.zeros(B, dtype=torch.bool, device=dev)
        self.picked, self.gen, self.dist = [], None, None

    def start(self, capturing, self_kvs, hist_valid):
        self.any_step_may_be_last = self.finished is not None and not capturing

    def fused_step(self, t, logits, mix_logits, source_map, copies):
        want = t == self.T - 1 or self.any_step_may_be_last
        ban = (self.hist, t, self.ngram, self.eos) if self.ngram else None
        if self.rules is None:
            gen, dist, ids = ops.pointer_head_decode(logits, mix_logits, source_map, copies, want_gen=want, want_dist=want, ban=ban)
        else:
            gen, dist, ids = ops.pointer_head_decode(logits, mix_logits, source_map, copies, want_gen=want, want_dist=want, ban=ban, rules=self._rules_at(t))
        self.gen, self.dist = (gen.view(-1, 1, self.V), dist.view(-1, 1, self.V)) if want else (None, None)
        return self._emit(ids.unsqueeze(1))

    def unfused_step(self, t, gen, dist):
        if self.ngram or self.rules is not None:  # dist is returned as the row after the ban and the rules, as K23 returns it
            row = self._banned_copy(dist, self.hist, t, self.eos)
            ids = ops.row_argmax(row)[0]
            if self.ngram:
                self.hist[:, t] = ids
            self.gen, self.dist = gen, row.unsqueeze(1)
            return self._emit(ids.unsqueeze(1))
        self.gen, self.dist = gen, dist
        return self._emit(ops.row_argmax(dist[:, -1])[0].unsqueeze(1))

    def _emit(self, ids):
        if self.finished is not None:
            ids = ids.masked_fill(self.finished.unsqueeze(1), 0)
            self.finished = self.finished | ids[:, 0].eq(self.eos)
        self.picked.append(ids)
        return ids

    def all_finished(self):
        return self.finished is not None and bool(self.finished.all())

    def result(self, dec_out):
        answer = torch.cat(self.picked, dim=-1)
        if answer.size(1) < self.T:
            answer = torch.nn.functional.pad(answer, (0, self.T - answer.size(1)))
        return dec_out, self.gen, self.dist, answer


class _BeamMode(_DecodeMode):
    """Beam search (the reference's common/Generations.py:112-190, per item on the device).  The W slots of an item are the rows
    b * W + w, and every step is the greedy step on B * W rows followed by K24 (top-W of the mixed distribution; ``torch.topk`` on the
    unfused one), K25 (the per-item merge, EOS / last-step retirement), K26 and, after the last step, K27 (the back-track).  K26 reorders
    the self-attention caches by the chosen parents; a gather cannot run in place, so it writes into a second set of buffers and the two
    sets swap roles every step.  A hypothesis retires on the decoder's ``beam_eos_id`` or at max_target_length; the pass may end once no
    slot is alive.  -> (dec_out of the last step's rows, None, None, answer [B, T], beam_answers [B, W, T], beam_scores [B, W])."""
    counter = "last_beam_steps"

    def __init__(self, decoder, B, W, T, dev, ngram=0, rules=None):
        self.W, self.eos, self.ngram = W, decoder.beam_eos_id, ngram
        self._set_rules(rules, W)
        self.alpha = 1.0 if rules is None else rules["length_penalty"]
        # the flat history: a slot's history is its hypothesis, K25 carries it along.  Any rule selects it too: that form of K25 holds a candidate
        # of probability 0 dead (a zeroed EOS or banned id never enters a hypothesis) and is the one that takes the length penalty
        self.state = ops.BeamState(B, W, T, dev, flat=bool(ngram) or self.rules is not None or self.alpha != 1.0)

    def start(self, capturing, self_kvs, hist_valid):
        spare = [[torch.zeros_like(c) for c in layers] for layers in self_kvs]
        self.live = (self_kvs, hist_valid, [c for layers in self_kvs for c in layers])
        self.spare = (spare, torch.zeros_like(hist_valid), [c for layers in spare for c in layers])

    def fused_step(self, t, logits, mix_logits, source_map, copies):
        ban = (self.state.flat_rows(t), t, self.ngram, self.eos) if self.ngram else None
        if self.rules is None:
            _, _, cand_p, cand_id = ops.pointer_head_topk(logits, mix_logits, source_map, copies, self.W, ban=ban)
        else:
            _, _, cand_p, cand_id = ops.pointer_head_topk(logits, mix_logits, source_map, copies, self.W, ban=ban, rules=self._rules_at(t))
        return self._advance(t, cand_p, cand_id)

    def unfused_step(self, t, gen, dist):
        ruled = self.ngram or self.rules is not None
        row = self._banned_copy(dist, self.state.flat_rows(t) if self.ngram else None, t, self.eos) if ruled else dist[:, -1].detach().float()
        return self._advance(t, *torch.topk(row, self.W, dim=-1))

    def _advance(self, t, cand_p, cand_id):
        if self.alpha == 1.0:
            ops.beam_advance(self.state, cand_p, cand_id, t, self.eos)
        else:
            ops.beam_advance(self.state, cand_p, cand_id, t, self.eos, length_penalty=self.alpha)
        return self.state.token.view(-1, 1)

    def after_step(self, t, self_kvs, hist_valid):
        ops.beam_gather(self.live[2], self.spare[2], self.state.parent, t, self.live[1], self.spare[1])
        self.live, self.spare = self.spare, self.live
        return self.live[:2]

    def all_finished(self):
        return not bool(self.state.alive.any())

    def result(self, dec_out):
        return (dec_out, None, None) + ops.beam_backtrack(self.state)


class _SampleMode(_DecodeMode):
    """Sampled decoding (the reference's common/Generations.py:7-63 ``sample``, with the draw on the device).  The ``num_samples`` draws of
    an item are the rows b * N + n.  K28 (ops.pointer_head_sample) takes K23's place: one launch draws the token of every row after
    temperature / top-k / top-p, applies the loop's conventions (UNK for EOS at step 0, EOS forced at the last step, PAD behind the end)
    and keeps the ``ended`` flags on the device; nothing is read back inside a step.  The unfused distribution feeds the same kernel
    (``dist_in``).

    ``params``: dict(num_samples, temperature, top_k, top_p, eos, unk, pad, seed, uniforms).  ``uniforms`` f32 [T, B * N] overrides the
    RNG.  Otherwise row r of step t draws at counter rng_base + offset + r: with ``seed`` None, (seed, offset, state) is
    ``config.next_rng(B * N)``, taken once per step in step order -- the global counter stream, so with a device step state installed a
    captured pass draws NEW samples on every replay whose ``CaseStepState.rng_base`` has moved, and WITHOUT a device state a replay
    repeats its samples (seed and offsets are frozen into the graph); with an integer ``seed`` the pass is private and reproducible:
    (seed, offset t * B * N, no state).  A short pass is padded with PAD ids of probability 1.
    -> (dec_out of the last step's rows, None, None, answer [B, T], samples [B, N, T], sample_probs [B, N, T], sample_scores [B, N])."""
    counter = "last_sample_steps"

    def __init__(self, B, T, dev, params, ngram=0, rules=None):
        self.B, self.N, self.T, self.R, self.pad = B, int(params["num_samples"]), T, B * int(params["num_samples"]), params["pad"]
        self.ngram = ngram
        self._set_rules(rules, self.N)
        self.hist = torch.zeros(self.R, T, dtype=torch.int32, device=dev) if ngram else None  # K28 appends the emitted id at [:, t]
        self.seed, self.uniforms = params.get("seed"), params.get("uniforms")
        if self.uniforms is not None and tuple(self.uniforms.shape) != (T, self.R):
            raise ValueError("sampled decoding: uniforms must be [max_target_length, batch * num_samples] = [%d, %d]" % (T, self.R))
        self.draw = (params["eos"], params["unk"], params["pad"], params["temperature"], params["top_k"], params["top_p"])
        self.ended = torch.zeros(self.R, dtype=torch.uint8, device=dev)
        self.picked, self.probs = [], []

    def _draw(self, t, *head, **kw):
        u = None if self.uniforms is None else self.uniforms[t]
        rng = None if u is not None else config.next_rng(self.R) if self.seed is None else (int(self.seed), t * self.R, None)
        if self.ngram:  # (K28 applies the ban to either row source, the unfused ``dist_in`` included)
            kw["ban"] = (self.hist, t, self.ngram)
        if self.rules is not None:  # (likewise; a row that has ended is left alone)
            kw["rules"] = self._rules_at(t)
        _, _, tok, p = ops.pointer_head_sample(*head, self.ended, t == 0, t == self.T - 1, *self.draw, rng=rng, uniforms=u, **kw)
        self.picked.append(tok.unsqueeze(1))
        self.probs.append(p.unsqueeze(1))
        return self.picked[-1]

    def fused_step(self, t, logits, mix_logits, source_map, copies):
        return self._draw(t, logits, mix_logits, source_map, copies)

    def unfused_step(self, t, gen, dist):
        return self._draw(t, None, None, None, None, dist_in=dist[:, -1].detach().float())

    def all_finished(self):
        return bool(self.ended.all())

    def result(self, dec_out):
        B, N, T = self.B, self.N, self.T
        samples, sample_probs = torch.cat(self.picked, dim=1), torch.cat(self.probs, dim=1)
        if samples.size(1) < T:  # every row had ended: PAD, probability 1
            samples = torch.nn.functional.pad(samples, (0, T - samples.size(1)))
            sample_probs = torch.nn.functional.pad(sample_probs, (0, T - sample_probs.size(1)), value=1.0)
        emitted = samples.ne(self.pad)
        nll = -torch.log(sample_probs.clamp_min(1e-30)) * emitted
        sample_scores = nll.sum(dim=1) / emitted.sum(dim=1).clamp_min(1)
        samples = samples.view(B, N, T)
        return dec_out, None, None, samples[:, 0].contiguous(), samples, sample_probs.view(B, N, T), sample_scores.view(B, N)


class PointerDecoderCore(nn.Module):
    """Shared machinery of the three pointer-generator decoders: the dispatch of their ``forward``s (``_run``), the teacher-forced and the
    KV-cached passes and the heads.  A decoder adds its modules, ``_head_parts`` and the two settings below."""
    gen_dropout = 0.0  # dropout between the generator's two Linears (training)
    train_returns_pair = False  # the training branch returns (dist1, dist2) instead of their sum

    def _build(self, num_memories, num_layers, nhead, vocab, H, query_width, emb_matrix=None, max_len=1000):
        self.tgt_vocab_size, self.num_layers, self.hidden_size = vocab, num_layers, H
        self.embedding = _embedding(vocab, H, max_len=max_len, emb_matrix=emb_matrix)
        layer = TransformerDecoderLayer(H, nhead=nhead, dim_feedforward=H, dropout=0.1, activation='gelu')
        self.decs = nn.ModuleList([TransformerDecoder(layer, num_layers=num_layers, norm=None) for _ in range(num_memories)])
        self.attns = nn.ModuleList([BilinearAttention(query_width, H, H) for _ in range(num_memories)])
        # EOS-aware early stop of greedy decoding.  None = the reference's behaviour: always max_target_length steps
        # (CaSE/Model.py:94).  With an id, a finished answer is continued with PAD and the loop ends once EVERY answer of the
        # batch has produced EOS -- checked every ``eos_check_every`` steps, so one host sync per 8 tokens, none per token.
        self.eos_id = None
        self.eos_check_every = 8
        self.last_greedy_steps = 0
        self.last_beam_steps = 0
        self.last_sample_steps = 0
        # beam search retires a hypothesis on this id (the task models set it to EOS); None: every hypothesis runs to max_target_length
        self.beam_eos_id = None
        # the head of a scoring pass (``_score``) runs over chunks of at most this many (candidate, position) rows: the f32 logits buffer is
        # score_chunk_rows x V however many candidates are scored
        self.score_chunk_rows = 2048

    # ------------------------------------------------------------------------------------------
    def _sorted(self, source_map):
        """The batch's source map with its (token, position) keys sorted on the device, once per forward: every
        pointer scatter of the batch -- one per training step, one per generated token -- then adds run by run without atomics."""
        if torch.is_tensor(source_map) and source_map.is_cuda and ops.SortedSource.fits(source_map, self.tgt_vocab_size):
            return ops.SortedSource(source_map, self.tgt_vocab_size)
        return source_map

    def _memory_cache(self, mems, absorb=False):
        """Step-invariant projections of the memories (cross-attention K/V per layer, additive-attention keys)."""
        out = []
        for i, m in enumerate(mems):
            fused = absorb and ops.pointer_decode_supported(m) and self.attns[i].hidden_size == m.shape[2]  # K22: e^{2 uh} instead of uh
            out.append(dict(kvs=self.decs[i].project_memory(m, absorb=absorb), uh=None if fused else self.attns[i].project_keys(m),
                            eu=self.attns[i].project_keys_exp(m) if fused else None))
        return out

    def _run_prefix(self, dec_ids, mems, valid, weights, feature):
        """decs[0] -> attns[0] -> decs[1] -> attns[1] (a sequential chain, CaSE/Model.py:74-83)."""
        dec_in = _embed(self.embedding, dec_ids, self.training)
        tgt_valid = dec_ids.ne(0)
        x = dec_in
        ctxs, copies = [], []
        for i, mem in enumerate(mems):
            x = self.decs[i].forward_batch_first(x, mem, tgt_valid, valid[i], causal=True)
            q = x if feature is None else torch.cat([x, feature], dim=-1)
            ctx, p = self.attns[i].attend(q, mem, mem, row_valid=tgt_valid, col_valid=valid[i])
            ctxs.append(ctx)
            if weights is not None:
                p = weights[i].unsqueeze(1) * p
                p = p / (1e-8 + p.sum(dim=-1, keepdim=True))
            copies.append(p)
        return dec_in, x, ctxs, copies

    def _check_length(self, T):
        if T > self.embedding[1].pe.size(0):
            raise RuntimeError("max_target_length %d exceeds max_len %d" % (T, self.embedding[1].pe.size(0)))

    def _cache_setup(self, mems, max_target_length, feat):
        """What a cached decoding pass builds once: the step-invariant memory projections, one empty self-attention cache per layer, the
        prefix validity and the step-invariant halves of the additive-attention queries."""
        B, dev = mems[0].shape[0], mems[0].device
        # the raw-pointer decode kernels (K21 / K22 / K23) have no autograd Function behind them: eval mode AND no_grad (the reference only
        # predicts under no_grad; a caller that differentiates an eval-mode greedy pass keeps the differentiable launches)
        inference = not self.training and not torch.is_grad_enabled()
        cache = self._memory_cache(mems, absorb=inference)
        self_kvs = [dec.new_self_cache(B, max_target_length, mems[0]) for dec in self.decs]
        hist_valid = torch.zeros(B, max_target_length, dtype=torch.bool, device=dev)
        self._check_length(max_target_length)
        # the feature half of the additive-attention query does not change over the steps: projected once per pass (BilinearAttention.split_query)
        splits = [self.attns[i].split_query(feat, self.hidden_size) if (QUERY_SPLIT and inference and feat is not None and cache[i]["eu"] is not None) else None
                  for i in range(len(mems))]
        return inference, cache, self_kvs, hist_valid, splits

    def _cached_layers(self, t, ids, mems, valid, weights, feat, cache, splits, self_kvs, hist_valid):
        """Position ``t`` of every row through the decoder stacks and the additive attentions, against the caches: (dec_in, x, ctxs, copies)."""
        table, pos = self.embedding[0].weight, self.embedding[1]
        tok_valid = ids.ne(0)
        hist_valid[:, t] = tok_valid[:, 0]
        dec_in = ops.embed_pos(ids, table, pos.pe[t:t + 1])  # position t
        x = dec_in
        ctxs, copies = [], []
        for i, mem in enumerate(mems):
            x = self.decs[i].step(x, t, self_kvs[i], hist_valid, cache[i]["kvs"], valid[i])
            q = x if (feat is None or splits[i] is not None) else torch.cat([x, feat], dim=-1)
            if cache[i]["eu"] is not None:  # K22: scores, softmax, prior renormalisation and context in one launch
                ctx, p = self.attns[i].attend_decode(q, mem, tok_valid, valid[i], cache[i]["eu"], None if weights is None else weights[i],
                                                     split=splits[i])
            else:
                ctx, p = self.attns[i].attend(q, mem, mem, row_valid=tok_valid, col_valid=valid[i], uh=cache[i]["uh"])
                if weights is not None:
                    p = weights[i].unsqueeze(1) * p
                    p = p / (1e-8 + p.sum(dim=-1, keepdim=True))
            ctxs.append(ctx)
            copies.append(p)
        return dec_in, x, ctxs, copies

    @staticmethod
    def _per_item(n, mems, valid, weights, source_map, feat, keys=True, unit_too=False):
        """Every item's row ``n`` times in a row (row b * n + k): the memories, masks, copy priors, the feature and the source map of a pass
        whose candidates (beam slots, samples, answers to score) are extra batch rows, so a pass costs n x the memory footprint per item.
        A SortedSource repeats its sorted keys, it does not sort again; ``keys=False`` leaves the source map as it is (K29 reads key row
        r // rows_per_source).  n = 1 launches nothing unless ``unit_too`` (beam search at width 1 repeats)."""
        if n == 1 and not unit_too:
            return mems, valid, weights, source_map, feat
        mems = [m.repeat_interleave(n, dim=0) for m in mems]
        valid = [v.repeat_interleave(n, dim=0) for v in valid]
        weights = None if weights is None else [w.repeat_interleave(n, dim=0) for w in weights]
        if keys:
            source_map = source_map.expand(n) if isinstance(source_map, ops.SortedSource) else source_map.repeat_interleave(n, dim=0)
        return mems, valid, weights, source_map, None if feat is None else feat.repeat_interleave(n, dim=0)

    def _decode(self, mode, mems, valid, weights, source_map, feat, BOS, max_target_length):
        """The KV-cached decoding pass (K13) every mode shares.  Step semantics are the reference's (CaSE/Model.py:94-123): a fixed number
        of steps, PAD tokens in the prefix masked as keys -- but each step computes ONE new position: self-attention K/V of earlier
        positions, the per-layer K/V projections of both memories and the additive-attention keys are cached, so a step streams the caches
        once instead of recomputing the prefix (O(T) instead of O(T^2) decoder work, no per-step projection of the 3840-token passage
        memory).  ``mode`` (a ``_DecodeMode``) turns a step's head into the next ids and owns everything else that differs between greedy,
        beam and sampled decoding.  A pass ends early once ``mode.all_finished()``, read every ``eos_check_every`` steps: one host sync per
        8 tokens, none per token, and none at all in a captured pass, which cannot branch on device data and runs its fixed T steps."""
        R, dev, T = mems[0].shape[0], mems[0].device, max_target_length
        inference, cache, self_kvs, hist_valid, splits = self._cache_setup(mems, T, feat)
        ids = self._bos(R, BOS, dev)
        capturing = torch.cuda.is_current_stream_capturing()
        fused_head = inference and ops.pointer_head_supported(source_map, self.tgt_vocab_size, len(mems))
        mode.start(capturing, self_kvs, hist_valid)
        for t in range(T):
            dec_in, x, ctxs, copies = self._cached_layers(t, ids, mems, valid, weights, feat, cache, splits, self_kvs, hist_valid)
            if fused_head:  # vocabulary softmax, mixing, pointer scatter and the mode's choice in one launch
                dec_out, gen_in = self._head_parts(dec_in, x, feat)
                logits, mix_logits = self._head_logits(dec_out, gen_in, ctxs)
                ids = mode.fused_step(t, logits, mix_logits, source_map, [c.reshape(R, -1) for c in copies])
            else:  # no fused head for this pass (or a differentiated one): the unfused distribution feeds the mode
                dec_out, gen, dist = self._head(dec_in, x, ctxs, copies, feat, source_map)
                ids = mode.unfused_step(t, gen, dist)
            steps = t + 1
            if steps == T:
                break
            self_kvs, hist_valid = mode.after_step(t, self_kvs, hist_valid)
            if not capturing and steps % self.eos_check_every == 0 and mode.all_finished():
                break
        setattr(self, mode.counter, steps)
        return mode.result(dec_out)

    def _score(self, mems, valid, weights, source_map, BOS, answers, pad=0, feature_of=None, segments=None, grad_head=False):
        """Teacher-forced scoring of given answers (eval mode): ``answers`` int64 [B, T'] or [B, N, T'], ``pad`` marking the positions that
        are not scored.  One full-prefix pass over dec_ids = cat[BOS, answers[:, :-1]] (``_run_prefix``, causal), then the head over row
        chunks of at most ``score_chunk_rows`` (candidate, position) rows.  The N candidates of an item are extra batch rows (``_per_item``).
        The sorted source keys are NOT repeated: the rows of an item are consecutive and K29 reads key row r // rows_per_source.
        Under no_grad (and unless CASE_POINTER_SCORE=off) a chunk's head is ``_head_logits`` + K29 (ops.pointer_head_score): one read of the
        logits, no [rows, V] distribution.  With grad enabled it is the unfused differentiable chain of the training branch (``_generate``,
        ``_mix``, a gather), so gradients reach the parameters.  ``grad_head`` (only ``do_mrt`` sets it): with grad enabled and where
        ``ops.pointer_score_grad_supported``, a chunk's head is ``_head_logits`` + K29 with row statistics and K41 in the backward pass
        (ops.pointer_head_score_grad) instead of the chain.  Nothing is read back: the pass captures into one graph.
        -> dict(token_probs [B, N, T'] (1 where PAD), copy_probs [B, N, T'] (the pointer part, 0 where PAD), scores [B, N] (mean over the
        scored targets of -log max(p, 1e-30)), loss [1] (sum of -log(p + 1e-8) over the scored targets / their count), tokens int64 scalar).
        ``segments`` (the G + 1 boundaries of ``evaluation.attribution.source_segments``; None: the launches of a pass without it): every
        chunk also attributes its targets' pointer mass, K39 (ops.copy_attribution) right behind K29 on the same operands, the host form
        (``copy_attribution_host``) on the unfused chain, for an unsorted source map, more than 64 segments or CASE_COPY_ATTRIBUTION=off ->
        also copy_mass f32 [B, N, T', G], copy_pos int32, copy_pos_mass f32 and copy_count int32 [B, N, T']."""
        if self.training:
            raise ValueError("scoring runs in eval mode: call model.eval() first")
        if answers.dim() == 2:
            answers = answers.unsqueeze(1)
        if answers.dim() != 3 or answers.dtype != torch.int64 or answers.size(0) != mems[0].shape[0]:
            raise ValueError("scoring: answers must be int64 [B, T] or [B, N, T] with the batch's B")
        B, N, T = answers.shape
        dev, V, H = mems[0].device, self.tgt_vocab_size, self.hidden_size
        self._check_length(T)
        feat = None if feature_of is None else feature_of(T)
        mems, valid, weights, source_map, feat = self._per_item(N, mems, valid, weights, source_map, feat, keys=False)
        R = B * N
        tgt = answers.reshape(R, T).to(dev)
        dec_ids = torch.cat([self._bos(R, BOS, dev), tgt[:, :-1]], dim=-1)
        dec_in, x, ctxs, copies = self._run_prefix(dec_ids, mems, valid, weights, feat)
        # every (candidate, position) pair is one row of the head; item b owns rows b * per .. (b + 1) * per - 1
        rows, per = R * T, N * T
        dec_in, x = dec_in.reshape(rows, 1, H), x.reshape(rows, 1, H)
        feat = None if feat is None else feat.reshape(rows, 1, -1)
        ctxs = [c.reshape(rows, 1, -1) for c in ctxs]
        copies = [c.reshape(rows, -1) for c in copies]
        flat = tgt.reshape(rows)
        sorted_src = isinstance(source_map, ops.SortedSource)
        fused = sorted_src and ops.pointer_score_supported(source_map, len(mems))
        # the differentiable fused head (K29 with row statistics, K41 in the backward pass): only for a caller that asks (minimum-risk training)
        fused_grad = bool(grad_head) and not fused and torch.is_grad_enabled() and ops.pointer_score_grad_supported(source_map, len(mems))
        head_score = ops.pointer_head_score_grad if fused_grad else ops.pointer_head_score
        limit = max(1, int(self.score_chunk_rows))
        if per <= limit:  # whole items per chunk
            step = limit // per * per
            chunks = [(r0, min(r0 + step, rows)) for r0 in range(0, rows, step)]
        else:  # an item's rows in several chunks: every chunk lies inside one item
            chunks = [(b * per + o, min(b * per + o + limit, (b + 1) * per)) for b in range(B) for o in range(0, per, limit)]
        probs, ptrs, parts = [], [], []
        if segments is not None:
            segments = ops.check_segments(segments, (source_map.ids if sorted_src else source_map).size(1), "scoring", limit=None)
            kernel = sorted_src and len(segments) - 1 <= ops.ATTRIBUTION_MAX_G and ops.copy_attribution_supported(source_map, len(mems))
        for r0, r1 in chunks:
            n = r1 - r0
            dec_out, gen_in = self._head_parts(dec_in[r0:r1], x[r0:r1], None if feat is None else feat[r0:r1])
            cx, cp, y = [c[r0:r1] for c in ctxs], [c[r0:r1] for c in copies], flat[r0:r1]
            b0, b1 = r0 // per, (r1 + per - 1) // per
            if fused or fused_grad:  # K29: (max, sum) over the logits row, logit[y], and the pointer mass of y's run in the item's sorted keys
                logits, mix_logits = self._head_logits(dec_out, gen_in, cx, with_grad=fused_grad)
                p, c = head_score(logits, mix_logits, source_map.select(slice(b0, b1)), n // (b1 - b0), cp, y, pad)
                if segments is not None and kernel:  # K39: the same run of the same keys, kept apart by segment
                    parts.append(ops.copy_attribution(mix_logits, source_map.select(slice(b0, b1)), n // (b1 - b0), cp, y, segments, pad))
                elif segments is not None:
                    parts.append(copy_attribution_host(mix_logits, source_map.ids[b0:b1], cp, y, segments, pad, V, max_segments=None))
            else:  # the differentiable chain: every row a batch row of one position, its item's source beside it
                item = torch.arange(r0, r1, device=dev) // per
                src = source_map.select(item) if sorted_src else source_map.index_select(0, item)
                gen = self._generate(gen_in, 0.0)
                d1, d2 = self._mix(dec_out, cx, gen, [c.unsqueeze(1) for c in cp], src)
                inside = (y >= 0) & (y < V)
                at = y.clamp(0, V - 1).reshape(n, 1, 1)
                c = d2.gather(-1, at).reshape(n)
                p = d1.gather(-1, at).reshape(n) + c
                skip = y.eq(pad) if pad >= 0 else torch.zeros_like(inside)
                p = torch.where(skip, torch.ones_like(p), torch.where(inside, p, torch.zeros_like(p)))
                c = torch.where(skip | ~inside, torch.zeros_like(c), c)
                if segments is not None:  # the host form on the chain's own tensors (the mixing logits are ``_mix``'s)
                    mix_logits = ops.linear(torch.cat([dec_out] + cx, dim=-1), self.mix.weight, self.mix.bias, out_dtype=torch.float32)
                    ids = source_map.ids if sorted_src else source_map
                    parts.append(copy_attribution_host(mix_logits.reshape(n, -1), ids[b0:b1], cp, y, segments, pad, V, max_segments=None))
            probs.append(p)
            ptrs.append(c)
        p, c = torch.cat(probs).view(B, N, T), torch.cat(ptrs).view(B, N, T)
        scored = (answers.to(dev).ne(pad) if pad >= 0 else torch.ones_like(answers, dtype=torch.bool, device=dev))
        count = scored.sum()
        scores = (-torch.log(p.clamp_min(1e-30)) * scored).sum(dim=-1) / scored.sum(dim=-1).clamp_min(1)
        loss = ((-torch.log(p + 1e-8) * scored).sum() / count.clamp_min(1)).reshape(1)
        out = dict(token_probs=p, copy_probs=c, scores=scores, loss=loss, tokens=count)
        if segments is not None:
            whole = {k: torch.cat([part[k] for part in parts]) for k in ("mass", "pos", "pos_mass", "count")}
            out.update(copy_mass=whole["mass"].view(B, N, T, -1), copy_pos=whole["pos"].view(B, N, T),
                       copy_pos_mass=whole["pos_mass"].view(B, N, T), copy_count=whole["count"].view(B, N, T))
        return out

    def _run(self, encode_memories, encode_masks, encode_weights, source_map, BOS, groundtruth_index, max_target_length, beam_width, sampling,
             score_index, feature_of=None, no_repeat_ngram=0, decode_rules=None, segments=None, score_grad_head=False, loss_only=False):
        """What the three ``forward``s share: score / train / beam / sample / greedy.  ``feature_of(T)``: the decoder feature for T positions
        (CaSE's answer representation), or None.  ``no_repeat_ngram`` (K32) and ``decode_rules`` (what ``decode_rules_param`` returned: min_length,
        banned ids, the beam length penalty) apply to the three decoding modes only.  ``loss_only`` (the training branch; ``do_train`` sets it):
        the result is the per-row NLL of ``groundtruth_index``, f32 [B * T] (``_train_nll``), instead of (dec_out, gen, dist, index)."""
        B, dev = source_map.size(0), encode_memories[0].device
        source_map = self._sorted(source_map)
        mems = [m.reshape(B, -1, self.hidden_size) for m in encode_memories]
        valid = [m.reshape(B, -1).contiguous() for m in encode_masks]
        weights = None if encode_weights is None else [w.reshape(B, -1) for w in encode_weights]
        if score_index is not None:
            return self._score(mems, valid, weights, source_map, BOS, score_index, feature_of=feature_of, segments=segments, grad_head=score_grad_head)
        T = groundtruth_index.size(1) if max_target_length is None else max_target_length
        if self.training and groundtruth_index is not None:
            dec_ids = torch.cat([self._bos(B, BOS, dev), groundtruth_index[:, :-1]], dim=-1)
            feat = None if feature_of is None else feature_of(dec_ids.size(1))
            if loss_only:
                return self._train_nll(*self._run_prefix(dec_ids, mems, valid, weights, feat), feat, source_map, groundtruth_index)
            dec_out, gen, dist = self._head(*self._run_prefix(dec_ids, mems, valid, weights, feat), feat, source_map)
            return dec_out, gen, dist, groundtruth_index
        if self.training:
            return None
        feat = None if feature_of is None else feature_of(1)
        ngram = no_repeat_ngram_param(no_repeat_ngram, T)
        if ngram and not ops.ngram_ban_supported():
            raise RuntimeError("no_repeat_ngram: this build of the library lacks the n-gram ban (CASE_FEAT_NGRAM_BAN)")
        rules = decode_rules
        if rules is not None and not (rules["on"] or rules["length_penalty"] != 1.0):
            rules = None  # every rule off: the launches of a pass without the argument
        if rules is not None:
            if not ops.decode_rules_supported():
                raise RuntimeError("min_length / banned_ids / length_penalty: this build of the library lacks the decoding rules (CASE_FEAT_DECODE_RULES)")
            if rules["min_length"] > T - 1:
                raise ValueError("min_length %d leaves no position for EOS within max_target_length %d" % (rules["min_length"], T))
            if rules["banned"] is not None and (rules["banned"].device != dev or (rules["banned"].dim() == 2 and rules["banned"].shape[0] != B)):
                raise ValueError("banned_ids must be on the batch's device and [K] or [B, K] with the batch's B = %d" % B)
        if beam_width:
            W = int(beam_width)
            if not ops.beam_supported(W):
                raise RuntimeError("beam search: width %d is outside what the beam kernels are built for (1 .. 8)" % W)
            mode, n = _BeamMode(self, B, W, T, dev, ngram, rules), W
        elif sampling:
            if not ops.sample_supported(self.tgt_vocab_size):
                raise RuntimeError("sampled decoding: this build of the library cannot draw from a vocabulary of %d (CASE_FEAT_SAMPLE_DECODE, "
                                   "CASE_FEAT_POINTER_HEAD_WIDE)" % self.tgt_vocab_size)
            mode, n = _SampleMode(B, T, dev, sampling, ngram, rules), int(sampling["num_samples"])
        else:
            mode, n = _GreedyMode(self, B, T, dev, ngram, rules), 1
        # beam search repeats its rows at width 1 too
        return self._decode(mode, *self._per_item(n, mems, valid, weights, source_map, feat, unit_too=bool(beam_width)), BOS, T)

    def _head_logits(self, dec_out, gen_in, ctxs, with_grad=False):
        """The vocabulary logits and the mixing logits of one cached step (f32): what K23 / K24 / K28 / K29 take.  ``with_grad``: the
        differentiated scoring pass of minimum-risk training -- the same launches with autograd behind them, so its probabilities carry the
        bits of the no_grad pass."""
        B, V = dec_out.shape[0], self.tgt_vocab_size
        h = ops.linear(gen_in, self.gen[0].weight, self.gen[0].bias)
        logits = ops.linear(h, self.gen[-2].weight, None, out_dtype=torch.float32)
        parts = [dec_out] + ctxs
        if with_grad and ops.linear_skinny_supported(parts, self.mix.weight, with_grad=True):
            mix_logits = ops.linear_skinny_grad(parts, self.mix.weight, self.mix.bias)
        elif ops.linear_skinny_supported(parts, self.mix.weight):  # the 1 + nmem mixing logits straight from the three inputs: no concatenation, no N = 3 GEMM tile
            mix_logits = ops.linear_skinny(parts, self.mix.weight, self.mix.bias)
        else:
            mix_logits = ops.linear(torch.cat(parts, dim=-1), self.mix.weight, self.mix.bias, out_dtype=torch.float32)
        return logits.reshape(B, V), mix_logits.reshape(B, -1)

    def _head(self, dec_in, x, ctxs, copies, feat, source_map):
        """The unfused head: (dec_out, gen, dist)."""
        dec_out, gen_in = self._head_parts(dec_in, x, feat)
        gen = self._generate(gen_in, self.gen_dropout)
        d1, d2 = self._mix(dec_out, ctxs, gen, copies, source_map)
        return dec_out, gen, ((d1, d2) if self.training and self.train_returns_pair else ops.add(d1, d2))

    def _train_nll(self, dec_in, x, ctxs, copies, feat, source_map, target):
        """The training head when only the loss is wanted: -log(p(target) + 1e-8) per (item, position) row, f32 [B * T], 0 where the target
        is PAD.  Where ``ops.train_head_supported`` (CASE_TRAIN_HEAD=auto, a device-sorted source map, <= 4 memories, CASE_POINTER_SCORE not
        off, a library with the loss-form kernels) it is the generator's first Linear -- the SAME dropout site, drawn at the same point of
        the counter stream, as ``_generate`` -- the mixing logits and ``ops.train_head_nll``: no [rows, V] probability tensor exists.
        Otherwise the dense chain of ``_head`` and a gather."""
        V, H = self.tgt_vocab_size, self.hidden_size
        if not ops.train_head_supported(source_map, len(ctxs)):
            _, _, dist = self._head(dec_in, x, ctxs, copies, feat, source_map)
            dist = ops.add(*dist) if isinstance(dist, tuple) else dist
            return ops.nll_rows(dist.reshape(-1, V), target.reshape(-1))
        B, T = target.shape
        dec_out, gen_in = self._head_parts(dec_in, x, feat)
        h = ops.linear(gen_in, self.gen[0].weight, self.gen[0].bias, p_drop=config.drop_p(self.gen_dropout, self.training))
        parts = [dec_out] + ctxs
        if ops.linear_skinny_supported(parts, self.mix.weight, with_grad=True):
            mix_logits = ops.linear_skinny_grad(parts, self.mix.weight, self.mix.bias)
        else:
            mix_logits = ops.linear(torch.cat(parts, dim=-1), self.mix.weight, self.mix.bias, out_dtype=torch.float32)
        return ops.train_head_nll(h.reshape(B * T, H), self.gen[-2].weight, mix_logits.reshape(B * T, -1), source_map, T,
                                  [c.reshape(B * T, -1) for c in copies], target.reshape(-1))

    def _generate(self, gen_in, hidden_drop):
        """gen = softmax(W_v (drop(W_h x + b)))  -- f32 logits and probabilities (K10)."""
        h = ops.linear(gen_in, self.gen[0].weight, self.gen[0].bias, p_drop=config.drop_p(hidden_drop, self.training))
        logits = ops.linear(h, self.gen[-2].weight, None, out_dtype=torch.float32)
        return ops.masked_softmax(logits)

    def _mix(self, dec_out, ctxs, gen, copies, source_map):
        """p = softmax(mix([dec_out, ctx_q, ctx_p])); dist1 = p0 * gen; dist2 = pointer mass scattered to the vocabulary."""
        mix_in = torch.cat([dec_out] + ctxs, dim=-1)
        pm = ops.masked_softmax(ops.linear(mix_in, self.mix.weight, self.mix.bias, out_dtype=torch.float32))
        dist1 = pm[:, :, 0:1] * gen
        ptr = torch.cat([pm[:, :, k + 1:k + 2] * c for k, c in enumerate(copies)], dim=-1)
        return dist1, self._scatter(ptr, source_map, gen.shape[-1])

    @staticmethod
    def _scatter(ptr, source_map, V):
        if isinstance(source_map, ops.SortedSource) or (source_map.dtype == torch.int64 and source_map.dim() == 2):
            return ops.copy_scatter(source_map, ptr, V)
        # dense [B, S, V] one-hot given by an API-compatible caller: recover the ids once, then scatter
        return ops.copy_scatter(source_map.argmax(dim=-1), ptr * source_map.sum(dim=-1).unsqueeze(1), V)

    @staticmethod
    def _bos(batch_size, BOS, device):
        return torch.full((batch_size, 1), BOS, dtype=torch.long, device=device)


class TransformerSeqDecoder(PointerDecoderCore):
    """Generic multi-memory decoder (reference: common/TransformerSeqEncoderDecoder.py:47-150)."""

    def __init__(self, num_memories, num_layers, nhead, tgt_vocab_size, hidden_size, emb_matrix=None):
        super().__init__()
        H = hidden_size
        # the reference's generic decoder builds its position table with max_len = 100 when a pre-trained embedding matrix is given
        # (common/TransformerSeqEncoderDecoder.py:57; 1000 otherwise, :55): ``pe`` is a persistent buffer, so a checkpoint of that
        # configuration only loads strictly into the same shape
        self._build(num_memories, num_layers, nhead, tgt_vocab_size, H, H, emb_matrix=emb_matrix, max_len=100 if emb_matrix is not None else 1000)
        self.norm = nn.LayerNorm(H)
        self.gen = nn.Sequential(nn.Linear(2 * H, H), nn.Linear(H, tgt_vocab_size, bias=False), nn.Softmax(dim=-1))
        self.mix = nn.Linear(H + num_memories * H, num_memories + 1)

    def _head_parts(self, dec_in, x, feat):
        dec_out = ops.layer_norm(x, self.norm.weight, self.norm.bias, self.norm.eps)
        return dec_out, torch.cat([dec_in, dec_out], dim=-1)

    def forward(self, encode_memories, BOS, UNK, source_maps, encode_masks=None, encode_weights=None,
                groundtruth_index=None, init_decoder_state=None, max_target_length=None, beam_width=None, sampling=None, score_index=None,
                no_repeat_ngram=0, decode_rules=None, segments=None, score_grad_head=False, loss_only=False):
        if isinstance(source_maps, (list, tuple)):
            source_maps = torch.cat(source_maps, dim=-2 if source_maps[0].dim() == 3 else -1)
        return self._run(encode_memories, encode_masks, encode_weights, source_maps, BOS, groundtruth_index, max_target_length, beam_width, sampling,
                         score_index, no_repeat_ngram=no_repeat_ngram, decode_rules=decode_rules, segments=segments, score_grad_head=score_grad_head,
                         loss_only=loss_only)
