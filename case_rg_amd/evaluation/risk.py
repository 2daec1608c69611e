"""Minimum-risk training (MRT; Shen et al. 2016, "Minimum Risk Training for Neural Machine Translation") on ROUGE-L: the expected cost of
a pool of candidates under the model's renormalised posterior, its gradient, and the training step of the task models built on it.

THE RULE.  For item b, over the candidates n with ``valid[b, n]`` and the scored positions t of candidate n (its non-PAD targets):

    l_n    = sum_t ln(max(p[n, t], 1e-30))            the candidate's log-probability under the model
    z_n    = alpha l_n                                alpha >= 0 sharpens (large) or flattens (small) the posterior
    Q_n    = exp(z_n - max z) / sum exp(z - max z)    over the valid n; Q_n = 0 where n is invalid
    risk_b = sum_n Q_n c_n                            c = cost[b, n], here 1 - ROUGE-L F against the reference
    dl_n   = alpha Q_n (c_n - risk_b)                 = d risk_b / d l_n
    grad_p[n, t] = dl_n / p[n, t]                     on scored positions with p > 1e-30, 0 elsewhere

An item without a valid candidate has risk 0 and zero gradients.  ``sequence_risk_host`` is this in vectorised f64 torch (CPU or GPU
tensors), ``ops.sequence_risk`` (K42) the device kernel: one wave per item, f64 inside, every output rounded to f32 once.

THE STEP (``minimum_risk_step``: ``do_mrt`` of CaSE and Masque).  Encode once with grad; draw a pool with ``do_sample`` under no_grad (or take
explicit candidates), append the reference; cost = 1 - F from K30 against the reference; duplicates of an earlier candidate are invalid;
score the pool teacher-forced with grad (``_score``; where ``ops.pointer_score_grad_supported`` the head of a chunk is ``_head_logits`` + K29
with row statistics, K41 in the backward pass, so no [rows, V] distribution is built or kept); loss = mean risk + mle_weight x the
reference's NLL.  Nothing is read back to the host.

LIMITS.  MRT steps run without dropout: the sampled pool, its scores and the gradient must come from one model, so the whole step runs
the module in eval mode (grad enabled) and restores the previous mode afterwards.  A pool holds at most 64 candidates (the reference
included) of at most 256 positions.  The cost is ROUGE-L F against ``data['response']`` alone."""
import math

import torch

from .. import ops
from .rouge_ids import model_specials, rouge_l_ids

P_MIN = 1e-30
MRT_MAX_N, MRT_MAX_T = ops.CONSENSUS_MAX_N, ops.LCS_MAX_T
MRT_DEFAULTS = dict(num_samples=8, alpha=5e-3, with_reference=True, dedup=True, mle_weight=0.0, temperature=1.0, top_k=0, top_p=1.0)


def sequence_risk_host(token_probs, scored, cost, valid=None, alpha=5e-3, rounded=True):
    """The rule above in vectorised f64 torch: token_probs [B, N, T], scored bool [B, N, T], cost [B, N], valid bool [B, N] or None (all)
    -> dict(risk [B], q [B, N], grad_p [B, N, T]), f32 (the f64 values rounded once; ``rounded=False``: the f64 values themselves).
    ``risk`` and ``q`` are differentiable in ``token_probs`` as torch is; ``grad_p`` is the closed form, detached."""
    alpha = ops.check_risk_alpha(alpha, "sequence_risk_host")
    if token_probs.dim() != 3 or tuple(scored.shape) != tuple(token_probs.shape) or tuple(cost.shape) != tuple(token_probs.shape[:2]):
        raise ValueError("sequence_risk_host: token_probs / scored [B, N, T] and cost [B, N]")
    p = token_probs.double()
    scored = scored.bool()
    c = cost.detach().double()
    ok = torch.ones_like(c, dtype=torch.bool) if valid is None else valid.bool()
    if tuple(ok.shape) != tuple(c.shape):
        raise ValueError("sequence_risk_host: valid must be [B, N]")
    l = (torch.log(p.clamp_min(P_MIN)) * scored).sum(dim=-1)
    z = torch.where(ok, alpha * l, torch.full_like(l, -math.inf))
    zmax = z.max(dim=1, keepdim=True)[0]
    some = torch.isfinite(zmax)
    e = torch.where(ok & some, torch.exp(z - torch.where(some, zmax, torch.zeros_like(zmax))), torch.zeros_like(z))
    q = e / e.sum(dim=1, keepdim=True).clamp_min(1e-300)
    risk = (q * c).sum(dim=1)
    dl = (alpha * q * (c - risk.unsqueeze(1))).detach()
    pd = p.detach()
    live = scored & (pd > P_MIN)
    grad_p = torch.where(live, dl.unsqueeze(-1) / torch.where(live, pd, torch.ones_like(pd)), torch.zeros_like(pd))
    out = dict(risk=risk, q=q, grad_p=grad_p)
    return {k: v.float() for k, v in out.items()} if rounded else out


def assemble_pool(candidates, reference, pad=0):
    """candidates int64 [B, N, T] or None, reference int64 [B, T'] or None -> int64 [B, N (+ 1), max(T, T')]: the reference joins as the
    LAST candidate, both right-padded with ``pad`` to the common width.  Pure tensor glue (CPU or GPU), nothing is read back."""
    if candidates is None and reference is None:
        raise ValueError("assemble_pool: no candidates and no reference")
    if candidates is not None and (not torch.is_tensor(candidates) or candidates.dtype != torch.int64 or candidates.dim() != 3):
        raise ValueError("do_mrt: candidates must be an int64 tensor [B, N, T]")
    if reference is None:
        return candidates
    if reference.dtype != torch.int64 or reference.dim() != 2:
        raise ValueError("do_mrt: the reference must be an int64 tensor [B, T]")
    ref = reference.unsqueeze(1)
    if candidates is None:
        return ref
    if candidates.shape[0] != ref.shape[0]:
        raise ValueError("do_mrt: %d items of candidates, %d references" % (candidates.shape[0], ref.shape[0]))
    ref = ref.to(candidates.device)
    width = max(candidates.shape[2], ref.shape[2])
    grow = lambda t: torch.nn.functional.pad(t, (0, width - t.shape[2]), value=pad)  # noqa: E731
    return torch.cat([grow(candidates), grow(ref)], dim=1)


def dedup_valid(lcs, length):
    """lcs int [B, N, N] (the LCS length of candidate n against candidate m, K30 on the pool against itself) and length int [B, N] (the
    compacted lengths: lcs[b, n, n]) -> valid bool [B, N]: candidate n is invalid when an earlier VALID m has lcs[n, m] == len_n == len_m,
    i.e. holds the same tokens.  Equality of sentences is transitive, so the first copy of every distinct sentence stays valid and "an
    earlier valid twin" is "any earlier twin": one comparison on [B, N, N], no loop."""
    N = lcs.shape[1]
    ln, lm = length.unsqueeze(2), length.unsqueeze(1)
    same = lcs.eq(ln) & lcs.eq(lm)
    earlier = torch.ones(N, N, dtype=torch.bool, device=lcs.device).tril(-1)  # [n, m]: m < n
    return ~(same & earlier).any(dim=2)


def pool_cost(pool, reference, specials, dedup=True):
    """pool int64 [B, N, T], reference int64 [B, T'] -> (cost f32 [B, N] = 1 - ROUGE-L F of every candidate against the reference (K30),
    valid bool [B, N] (all True without ``dedup``))."""
    f = rouge_l_ids(pool, reference, specials)["f"][:, :, 0]
    cost = 1.0 - f
    if not dedup:
        return cost, torch.ones_like(cost, dtype=torch.bool)
    lcs = rouge_l_ids(pool, pool, specials)["lcs"]
    return cost, dedup_valid(lcs, lcs.diagonal(dim1=1, dim2=2))


def mrt_params(model, candidates, num_samples, alpha, with_reference, dedup, mle_weight, sampling):
    """The checked arguments of a ``do_mrt`` call: the keywords, or ``model.mrt`` where they are None."""
    cfg = dict(MRT_DEFAULTS)
    cfg.update(getattr(model, "mrt", None) or {})
    given = dict(num_samples=num_samples, alpha=alpha, with_reference=with_reference, dedup=dedup, mle_weight=mle_weight)
    cfg.update({k: v for k, v in given.items() if v is not None})
    unknown = set(sampling) - {"temperature", "top_k", "top_p", "uniforms", "no_repeat_ngram", "min_length", "banned_ids"}
    if unknown:
        raise TypeError("do_mrt: unknown arguments %s" % ", ".join(sorted(unknown)))
    draw = {k: cfg[k] for k in ("temperature", "top_k", "top_p")}
    draw.update(sampling)
    cfg["alpha"] = ops.check_risk_alpha(cfg["alpha"], "do_mrt")
    cfg["mle_weight"] = float(cfg["mle_weight"])
    if not math.isfinite(cfg["mle_weight"]):
        raise ValueError("do_mrt: mle_weight must be finite (got %r)" % cfg["mle_weight"])
    cfg["with_reference"], cfg["dedup"] = bool(cfg["with_reference"]), bool(cfg["dedup"])
    if cfg["mle_weight"] != 0.0 and not cfg["with_reference"]:
        raise ValueError("do_mrt: mle_weight needs the reference in the pool (with_reference=True)")
    extra = 1 if cfg["with_reference"] else 0
    if candidates is None:
        cfg["num_samples"] = int(cfg["num_samples"])
        if cfg["num_samples"] < 1 or cfg["num_samples"] + extra > MRT_MAX_N:
            raise ValueError("do_mrt: 1 .. %d candidates per item, the reference included (num_samples %d)" % (MRT_MAX_N, cfg["num_samples"]))
    else:
        if sampling:
            raise TypeError("do_mrt: explicit candidates take no sampling arguments (%s)" % ", ".join(sorted(sampling)))
        if not torch.is_tensor(candidates) or candidates.dtype != torch.int64 or candidates.dim() != 3:
            raise ValueError("do_mrt: candidates must be an int64 tensor [B, N, T]")
        if candidates.shape[1] < 1 or candidates.shape[1] + extra > MRT_MAX_N or not 1 <= candidates.shape[2] <= MRT_MAX_T:
            raise ValueError("do_mrt: 1 .. %d candidates per item, the reference included, of 1 .. %d positions (got %d x %d)" % (
                MRT_MAX_N, MRT_MAX_T, candidates.shape[1], candidates.shape[2]))
    return cfg, draw


def minimum_risk_step(model, data, encode, stage_losses, candidates=None, num_samples=None, alpha=None, with_reference=None, dedup=None,
                      mle_weight=None, details=False, **sampling):
    """``do_mrt`` of the task models (CaSE, Masque).  ``encode()``: the model's encode stages (what ``_respond`` takes as ``_enc``);
    ``stage_losses(enc)``: the non-generation losses ``do_train`` computes from them.  -> the list ``do_train`` returns with the generation
    loss replaced by  mean_b risk_b + mle_weight x nll_ref;  ``details=True``: dict(losses, risk [B], q [B, N], cost [B, N], valid [B, N],
    candidates int64 [B, N, T], token_probs [B, N, T])."""
    cfg, draw = mrt_params(model, candidates, num_samples, alpha, with_reference, dedup, mle_weight, sampling)
    reference = data['response']
    if candidates is not None and candidates.shape[0] != reference.shape[0]:
        raise ValueError("do_mrt: %d items of candidates, a batch of %d" % (candidates.shape[0], reference.shape[0]))
    if cfg["with_reference"] and reference.shape[1] > MRT_MAX_T:
        raise ValueError("do_mrt: candidates of up to %d positions (the reference has %d)" % (MRT_MAX_T, reference.shape[1]))
    specials = model_specials(model.vocab2id)
    pad = specials[1]
    modes = [(mod, mod.training) for mod in model.modules()]  # every module's own flag: a submodule that was held in eval stays there
    model.eval()  # dropout off for the pool, the scores and the gradient alike
    try:
        with torch.enable_grad():
            enc = encode()
            losses = stage_losses(enc)
            with torch.no_grad():
                if candidates is None:
                    candidates = model.do_sample(data, num_samples=cfg["num_samples"], _enc=enc, **draw)['samples']
                pool = assemble_pool(candidates.to(reference.device), reference if cfg["with_reference"] else None, pad)
                if pool.shape[1] > MRT_MAX_N or pool.shape[2] > MRT_MAX_T:
                    raise ValueError("do_mrt: pools of up to %d candidates of up to %d positions (got %d x %d)" % (
                        MRT_MAX_N, MRT_MAX_T, pool.shape[1], pool.shape[2]))
                cost, valid = pool_cost(pool, reference, specials, cfg["dedup"])
            scored_pass, _ = model._respond(data, _enc=enc, score_index=pool, score_grad_head=True)
            p = scored_pass['token_probs']
            scored = pool.ne(pad)
            risk, q = ops.sequence_risk(p, scored, cost, valid, cfg["alpha"], want_q=True)
            loss = risk.mean().reshape(1)
            if cfg["mle_weight"] != 0.0:  # do_score's ``loss`` formula on the reference row (the last candidate)
                on = scored[:, -1]
                nll_ref = (-torch.log(p[:, -1] + 1e-8) * on).sum() / on.sum().clamp_min(1)
                loss = loss + cfg["mle_weight"] * nll_ref
    finally:
        for mod, training in modes:
            mod.training = training
    losses = list(losses) + [loss]
    if not details:
        return losses
    return dict(losses=losses, risk=risk, q=q, cost=cost, valid=valid, candidates=pool, token_probs=p)
