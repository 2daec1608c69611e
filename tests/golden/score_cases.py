"""Teacher-forced scoring parity cases: the case table, the candidate answers, the one teacher-forced route every party takes, and a
plain-NumPy restatement of ``do_score``'s reductions.

``forced_probs`` is ``beam_cases.step_dists``' route (the model in ``train()`` with dropout off in every namespace, the public ``action``
API with ``output`` = the answer) kept at every position instead of the last one.  It runs against

  * the reference            (tests/golden/gen_score_golden.py)            -> tests/golden/score_*.npz
  * the CPU oracle           (tests/test_score_cpu.py)
  * nothing on the GPU: the product is asked through its public ``do_score`` (tests/test_score_gpu.py) and held to the fixtures.

Geometry: the beam cases' (4 items, 3 x 12 passages, V 200), N = 3 candidates per item, T' = 6 -- but the GAIN 1.0 builders.  At the beam
cases' gain 3.0 the generator is peaky (top entry 0.3-0.99), the pointer mass of most rows is below 1e-6 and the batch's own response gets
probabilities down to 1e-18, far below the loss's 1e-8 epsilon: nothing about the pointer path would be pinned.  At gain 1.0 the reference
puts 0.16-0.48 of a row's mass on the pointer path and 0.02-0.09 on the most-copied source token.
"""
import numpy as np
import torch

from beam_cases import ITEMS, T  # noqa: F401  (the beam cases' batch geometry)
from case_rg_amd.utils import synth_batch
from case_rg_amd.utils.synth import FIRST_WORD_ID
from cases import V, _case_model, _masque_model

N = 3
P_MIN = 1e-4             # every scored target of the fixtures has at least this probability under the reference
# name -> (model, model seed, batch seed, candidate seed); searched on the CPU (gen_score_golden.py --search) so that the reference alone
# satisfies the generator's assertions
SCORE_CASES = {"score_case": ("case", 214, 152, 1), "score_masque": ("masque", 7, 11, 1)}


def build(ns, dev, name):
    model, mseed, bseed, _ = SCORE_CASES[name]
    m = (_case_model if model == "case" else _masque_model)(ns, dev, mseed, gain=1.0)
    b = {k: v.to(dev) for k, v in synth_batch(ITEMS, 3, 12, 8, 6, V, seed=bseed, model=model).items()}
    return m, b


def candidates(b, eos, cand_seed):
    """int64 [ITEMS, N, T] from the batch alone.  Per item: 0 = the batch's own response (PAD behind its EOS when it is shorter than T);
    1 = T tokens copied from the source, the most frequent source token first, no PAD; 2 = three ids that do NOT occur in the source, EOS,
    then a PAD tail."""
    src, resp = b["source_map"].cpu().numpy(), b["response"].cpu().numpy()
    out = np.zeros((ITEMS, N, T), dtype=np.int64)
    for i in range(ITEMS):
        rng = np.random.RandomState(1000 * cand_seed + i)
        out[i, 0, :resp.shape[1]] = resp[i, :T]
        tokens = src[i][src[i] != 0]
        ids, counts = np.unique(tokens, return_counts=True)
        out[i, 1, 0] = ids[np.argmax(counts)]
        out[i, 1, 1:] = tokens[rng.randint(0, len(tokens), size=T - 1)]
        absent = np.setdiff1d(np.arange(FIRST_WORD_ID, V), ids)
        out[i, 2, :3] = absent[rng.randint(0, len(absent), size=3)]
        out[i, 2, 3] = eos
    return torch.from_numpy(out)


def forced_probs(ns, m, b, model, answers):
    """answers int64 [B, T] -> (p f32 [B, T], ptr f32 [B, T] | None, gen f32 [B, T]): the probability of every answer token given the tokens
    before it, its pointer part where the model returns the two parts separately (CaSE: ``(dist1, dist2)``), and the generator's own
    probability of it (before mixing)."""
    q, p, sm = b["query"], b["passage"], b["source_map"]
    vocab = len(m.vocab2id)
    was_training = m.training
    m.train()  # (teacher forcing is the training branch of the decoders; dropout is off / patched to identity in every namespace)
    try:
        with torch.no_grad():
            if model == "case":
                eq, ep = m.query_encoder(q), m.passage_encoder(p)
                ps = m.passage_selection.action(q, p, encode_query=eq, encode_passage=ep)
                se = m.span_extraction.action(q, p, encode_query=eq, encode_passage=ep, passage_selection_result=ps)
                rg = m.response_generation.action(q, p, ns.build_map(sm, max=vocab), encode_query=eq, encode_passage=ep,
                                                  passage_selection_result=ps, span_extraction_result=se, output=answers)
                dist, dist2 = rg[2][0] + rg[2][1], rg[2][1]
            else:
                eq, ep = m.query_encoder(q)[0][:, :, -1], m.passage_encoder(p)[0][:, :, -1]
                ps = m.passage_selection.action(q, p, encode_query=eq, encode_passage=ep)
                rg = m.response_generation.action(q, p, ns.build_map(sm, max=vocab), encode_query=eq, encode_passage=ep,
                                                  passage_selection_result=ps, output=answers)
                dist, dist2 = rg[2], None
    finally:
        m.train(was_training)
    at = answers.unsqueeze(-1)
    pick = lambda d: d.float().gather(-1, at).squeeze(-1)  # noqa: E731
    return pick(dist), None if dist2 is None else pick(dist2), pick(rg[1])


def forced_all(ns, m, b, model, cands):
    """One pass per candidate: cands [B, N, T] -> (p, ptr | None, gen), each f32 numpy [B, N, T]."""
    parts = [forced_probs(ns, m, b, model, cands[:, n].contiguous()) for n in range(cands.shape[1])]
    stack = lambda k: None if parts[0][k] is None else np.stack([x[k].cpu().numpy() for x in parts], axis=1)  # noqa: E731
    return stack(0), stack(1), stack(2)


def reductions(p, answers, pad=0):
    """``do_score``'s outputs restated in NumPy (float64) from per-token probabilities p [B, N, T] and the answers [B, N, T]:
    token_probs (1 where PAD), scores [B, N] = mean over the non-PAD targets of -log max(p, 1e-30), loss = sum of -log(p + 1e-8) over all
    non-PAD targets / their count, tokens = that count."""
    p, answers = np.asarray(p, dtype=np.float64), np.asarray(answers)
    scored = answers != pad
    tp = np.where(scored, p, 1.0)
    scores = (-np.log(np.maximum(tp, 1e-30)) * scored).sum(-1) / np.maximum(scored.sum(-1), 1)
    tokens = int(scored.sum())
    loss = float((-np.log(tp + 1e-8) * scored).sum() / max(tokens, 1))
    return dict(token_probs=tp, scores=scores, loss=loss, tokens=tokens)
