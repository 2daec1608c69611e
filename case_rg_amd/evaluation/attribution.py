"""Answer attribution: which part of the source every answer token was copied from.

The model's probability of a token y is ``pm_0 gen[y] + sum_k pm_{1+k} sum_{s : src[s] == y} copy_k[s]``: the second part is a sum over
concrete source positions, and every position belongs to the conversation context or to one passage of the pool.  K39
(``ops.copy_attribution``) splits that sum over segments of the source on the device; this module holds what surrounds it:

``copy_attribution_host``  the same four outputs in plain vectorised torch (f64 inside, rounded once; CPU or GPU tensors): the path of an
                           unsorted source map, of a grad-enabled pass and of CASE_COPY_ATTRIBUTION=off, and what the tests compare K39 to;
``source_segments``        the boundaries of the layout ``collate_fn`` builds: the query row, then the P passages in pool order;
``summarize``              per-token shares, per-answer support and the cited passage from the masses and the token probabilities;
``attribution_ids`` / ``eval_attribution_ids``  does the model cite the gold passage?  Per-item columns and their sums, on the device.

Nothing here reads a device tensor back."""
import torch

from .. import ops

MAX_SEGMENTS = 64  # K39's limit, kept by the host form too: one meaning of ``seg_start`` on both paths


def source_segments(Lq, P, L):
    """The segment boundaries of ``data['source_map']`` = cat[query row (Lq), P passages of L tokens]: [0, Lq, Lq + L, ..., Lq + P L].
    Segment 0 is the conversation context, segment 1 + p passage p of the pool."""
    Lq, P, L = int(Lq), int(P), int(L)
    if Lq < 1 or P < 0 or (P and L < 1):
        raise ValueError("source_segments: a query row of at least one token and P >= 0 passages of at least one (got %d, %d, %d)" % (Lq, P, L))
    return [0] + [Lq + p * L for p in range(P + 1)]


def _boundaries(seg_start, S, device, who, max_segments=MAX_SEGMENTS):
    """-> (int64 [G + 1] on ``device``, G).  A Python sequence is checked in full, a tensor by shape and dtype only (it is not read back).
    ``max_segments`` None: no upper limit (a pass whose pool is larger than K39 takes)."""
    limit = float("inf") if max_segments is None else int(max_segments)
    if torch.is_tensor(seg_start):
        if seg_start.dtype not in (torch.int32, torch.int64) or seg_start.dim() != 1:
            raise TypeError("%s: a seg_start tensor must be int32 [G + 1]" % who)
        G = seg_start.numel() - 1
        if not 1 <= G <= limit:
            raise ValueError("%s: 1 .. %s segments (seg_start holds %d boundaries)" % (who, limit, G + 1))
        return seg_start.to(device=device, dtype=torch.int64), G
    seg = ops.check_segments(seg_start, S, who, limit=max_segments)
    G = len(seg) - 1
    return torch.tensor(seg, dtype=torch.int64, device=device), G


def copy_attribution_host(mix_logits, src_ids, copies, targets, seg_start, pad=0, V=None, max_segments=MAX_SEGMENTS):
    """K39's outputs without the kernel.  mix_logits [R, 1 + nmem]; src_ids int64 [I, S] with R a multiple of I (row r reads source row
    r // (R / I)); copies: list of [R, len_k] with sum len_k = S; targets int64 [R]; seg_start as in ``ops.copy_attribution``; ``pad`` -1:
    none; ``V``: ids outside [0, V) are no tokens (None: no upper bound); ``max_segments``: K39's 64, None lifts it -> dict(mass f32 [R, G],
    pos int32 [R], pos_mass f32 [R], count int32 [R]).  The mixing softmax, the terms and the sums are f64 and rounded once; differentiable as torch is."""
    who = "copy_attribution_host"
    if mix_logits.dim() != 2 or mix_logits.shape[1] != len(copies) + 1 or not copies:
        raise ValueError("%s: mix_logits must be [R, 1 + nmem]" % who)
    R = mix_logits.shape[0]
    if src_ids.dim() != 2 or src_ids.dtype != torch.int64 or src_ids.shape[0] < 1 or R % src_ids.shape[0]:
        raise ValueError("%s: src_ids must be int64 [I, S] with the %d rows a multiple of I" % (who, R))
    I, S = src_ids.shape
    if any(c.dim() != 2 or c.shape[0] != R for c in copies) or sum(c.shape[1] for c in copies) != S:
        raise ValueError("%s: every copies[k] must be [R, len_k] with sum len_k = S = %d" % (who, S))
    if targets.dtype != torch.int64 or targets.numel() != R:
        raise TypeError("%s: targets must be int64 [R]" % who)
    dev = mix_logits.device
    seg, G = _boundaries(seg_start, S, dev, who, max_segments)
    y = targets.reshape(R)
    pm = torch.softmax(mix_logits.double(), dim=-1)
    term = torch.cat([pm[:, k + 1:k + 2] * c.double() for k, c in enumerate(copies)], dim=-1)  # [R, S]
    src = src_ids if I == R else src_ids.repeat_interleave(R // I, dim=0)
    live = y.ge(0) if V is None else (y.ge(0) & y.lt(V))
    if pad >= 0:
        live = live & y.ne(pad)
    match = src.eq(y.unsqueeze(1)) & live.unsqueeze(1)
    at = torch.arange(S, device=dev)
    seg_of = torch.bucketize(at, seg[1:], right=True).clamp_(max=G - 1)
    onehot = seg_of.unsqueeze(1).eq(torch.arange(G, device=dev)).double()  # [S, G]
    mass = torch.where(match, term, torch.zeros_like(term)) @ onehot
    count = match.sum(dim=1)
    masked = torch.where(match, term.detach(), torch.full_like(term, float("-inf")))
    best = masked.max(dim=1).values
    first = torch.where(masked.eq(best.unsqueeze(1)) & match, at.unsqueeze(0), torch.full_like(at, S).unsqueeze(0)).min(dim=1).values
    some = count.gt(0)
    pos = torch.where(some, first, torch.full_like(first, -1))
    pos_mass = torch.where(some, term.gather(1, first.clamp(max=S - 1).unsqueeze(1)).squeeze(1), torch.zeros_like(best))
    return dict(mass=mass.float(), pos=pos.int(), pos_mass=pos_mass.float(), count=count.int())


def summarize(token_probs, mass, scored):
    """token_probs f32 [..., T], mass f32 [..., T, G] (segment 0 the context, 1 + p passage p), scored bool [..., T] (False at PAD) ->
    share f32 [..., T, 1 + G]: column 0 the generator, clamp(1 - sum_g mass_g / max(p, 1e-30), 0, 1), column 1 + g mass_g / max(p, 1e-30),
    all 0 where not scored; support f32 [..., 1 + G]: the mean of share over the scored positions (0 for an empty answer); cited int64
    [...]: the passage with the largest support (columns 2 ..) as a pool index, the lowest index among equals, -1 where the answer is empty
    or no passage has support."""
    if mass.dim() != token_probs.dim() + 1 or mass.shape[:-1] != token_probs.shape or scored.shape != token_probs.shape:
        raise ValueError("summarize: token_probs [..., T], mass [..., T, G] and scored [..., T] (got %s, %s, %s)" % (
            tuple(token_probs.shape), tuple(mass.shape), tuple(scored.shape)))
    p = token_probs.float().clamp_min(1e-30).unsqueeze(-1)
    part = mass.float() / p
    gen = (1.0 - part.sum(dim=-1, keepdim=True)).clamp(0.0, 1.0)
    keep = scored.unsqueeze(-1)
    share = torch.cat([gen, part], dim=-1) * keep
    n = scored.sum(dim=-1)
    support = share.sum(dim=-2) / n.clamp_min(1).unsqueeze(-1)
    P = mass.shape[-1] - 1
    if P < 1:
        return dict(share=share, support=support, cited=torch.full_like(n, -1))
    passages = support[..., 2:]
    best = passages.max(dim=-1, keepdim=True).values
    index = torch.arange(P, device=mass.device).expand_as(passages)
    first = torch.where(passages.eq(best), index, torch.full_like(index, P)).min(dim=-1).values
    cited = torch.where(n.gt(0) & best.squeeze(-1).gt(0), first, torch.full_like(first, -1))
    return dict(share=share, support=support, cited=cited)


ANSWER_POOLS = ("test", "beam", "sample", "response")


def attribute_answers(model, data, encode, answers="test", trim_eos=None, **decode):
    """``do_attribute`` of the task models (CaSE, Masque): take or decode the pool, score it teacher-forced with the attribution on
    (``segments=``), then ``summarize``.  ``encode()``: the model's encode stages, run ONCE here and handed to the pool's decoder and to
    the scoring pass (``_enc=``).  The arguments are checked before anything runs."""
    from ..common.Constants import EOS_WORD
    if model.training:
        raise ValueError("do_attribute runs in eval mode: call model.eval() first")
    named = isinstance(answers, str)
    if named and answers not in ANSWER_POOLS:
        raise ValueError("do_attribute: answers must be one of %s or an int64 [B, T'] / [B, N, T'] tensor, not %r" % (ANSWER_POOLS, answers))
    if not named and not (torch.is_tensor(answers) and answers.dtype == torch.int64 and answers.dim() in (2, 3)):
        raise ValueError("do_attribute: answers must be one of %s or an int64 [B, T'] / [B, N, T'] tensor" % (ANSWER_POOLS,))
    decoded = named and answers != "response"
    if decode and not decoded:
        raise TypeError("do_attribute: answers that exist take no decoding arguments (%s)" % ", ".join(sorted(decode)))
    B, P, L = data['passage'].shape
    segments = source_segments(data['query'][0].numel(), P, L)
    if data['source_map'].dim() != 2 or data['source_map'].size(1) != segments[-1]:
        raise ValueError("do_attribute: data['source_map'] must be int64 [B, %d]: the query row, then the %d passages of %d tokens" % (
            segments[-1], P, L))
    enc = encode()
    if decoded:
        out = getattr(model, "do_" + answers)(data, _enc=enc, **decode)
        pool = out['answer'].unsqueeze(1) if answers == "test" else out['beam_answers' if answers == "beam" else 'samples']
    else:
        out = {}
        pool = data['response'] if named else answers.to(data['query'].device)
        pool = pool.unsqueeze(1) if pool.dim() == 2 else pool
    if decoded if trim_eos is None else trim_eos:  # a fixed-T greedy pass keeps emitting behind EOS: those ids are not part of the answer
        ends = pool.eq(model.vocab2id[EOS_WORD]).long()
        pool = pool.masked_fill((ends.cumsum(dim=-1) - ends).gt(0), 0)
    scored, rank = model._respond(data, _enc=enc, score_index=pool, segments=segments)
    out.update(scored)
    out.update(rank=rank, answers=pool, **summarize(scored['token_probs'], scored['copy_mass'], pool.ne(0)))
    return out


ATTRIBUTION_COLUMNS = ("cited_hit", "rank_agree", "gen_share", "context_share", "passage_share", "tokens")


def attribution_ids(out, passage_label, pad=0):
    """``out``: what ``do_attribute`` returned; passage_label int64 [B] (``data['passage_label']``'s form) -> per-item columns from slot 0
    of the pool, in ``ATTRIBUTION_COLUMNS``' order: ``cited_hit`` (cited == passage_label; an item that cites nothing misses) and
    ``rank_agree`` (cited == the passage the selection stage ranks first, the lowest index among equal scores), int64 [B]; ``gen_share``,
    ``context_share`` and ``passage_share`` (all passages), f64 [B]: the SUMS of the shares over the item's scored tokens, so that sums
    over items divided by the sum of ``tokens`` (int64 [B]) are token-weighted averages."""
    cited, rank, share = out['cited'][:, 0], out['rank'], out['share'][:, 0].double()
    if not torch.is_tensor(passage_label) or passage_label.dim() != 1 or passage_label.shape[0] != cited.shape[0]:
        raise TypeError("attribution_ids: passage_label must be int64 [B] with the batch's B = %d" % cited.shape[0])
    P = rank.shape[1]
    index = torch.arange(P, device=rank.device).expand_as(rank)
    top = torch.where(rank.eq(rank.max(dim=1, keepdim=True).values), index, torch.full_like(index, P)).min(dim=1).values
    scored = out['answers'][:, 0].ne(pad)
    sums = (share * scored.unsqueeze(-1)).sum(dim=1)  # [B, 2 + P]
    return dict(cited_hit=cited.eq(passage_label.to(cited.device)).long(), rank_agree=cited.eq(top).long(), gen_share=sums[:, 0],
                context_share=sums[:, 1], passage_share=sums[:, 2:].sum(dim=1), tokens=scored.sum(dim=1))


def eval_attribution_ids(out, passage_label, pad=0):
    """``attribution_ids``' arguments -> f64 [6] on the device: the sums over the items of the columns in ``ATTRIBUTION_COLUMNS``' order."""
    cols = attribution_ids(out, passage_label, pad)
    return torch.stack([cols[name].double().sum() for name in ATTRIBUTION_COLUMNS])
