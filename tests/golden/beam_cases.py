"""Beam-search parity cases (the builders of tests/golden/cases.py at a batch of ITEMS items).

``step_dists`` is the one way every party gets the next-token distribution of a prefix: a teacher-forced pass through the model's public
``action`` API, the same call ``cases.case_case_test`` uses for its margins.  It runs against

  * the reference            (tests/golden/gen_beam_golden.py: the adapter its own ``Generations.beam`` drives) -> tests/golden/beam_*.npz
  * the CPU oracle           (tests/test_beam_cpu.py: drives the plain-Python restatement of the selection rule)
  * the HIP product          (tests/test_beam_gpu.py: the independent check of the returned scores)

so the three differ in arithmetic only.
"""
import torch

from case_rg_amd.utils import synth_batch
from cases import V, _case_model, _masque_model

ITEMS, T = 4, 6          # T = the max_target_length _case_model / _masque_model build their models with
WIDTHS = (3, 4)
GAP = 1e-3               # an item is decisive when every comparison that decided its search has a relative gap above this
# name -> (model, model seed, batch seed); the seeds were searched on the CPU so that the reference alone satisfies the assertions of
# gen_beam_golden.py (enough decisive items, a beam answer that differs from the greedy one, a hypothesis retired on EOS before the last step)
BEAM_CASES = {"beam_case": ("case", 214, 152), "beam_masque": ("masque", 276, 172)}


def build(ns, dev, name):
    model, mseed, bseed = BEAM_CASES[name]
    m = (_case_model if model == "case" else _masque_model)(ns, dev, mseed, gain=3.0)
    b = {k: v.to(dev) for k, v in synth_batch(ITEMS, 3, 12, 8, 6, V, seed=bseed, model=model).items()}
    return m, b


def step_dists(ns, m, b, model, rows, prefixes):
    """rows: item index of every prefix; prefixes int64 [n, L], BOS first -> the distribution of token L, f32 [n, V]."""
    rows = torch.as_tensor(rows, dtype=torch.long, device=prefixes.device)
    q, p, sm = b["query"][rows], b["passage"][rows], b["source_map"][rows]
    # the teacher-forced input is cat[BOS, output[:, :-1]]: the last column of ``output`` is never read
    output = torch.cat([prefixes[:, 1:], torch.zeros_like(prefixes[:, :1])], dim=1)
    vocab = len(m.vocab2id)  # (the model's own vocabulary: the production-geometry test reuses this function at V = 30 522)
    was_training = m.training
    m.train()  # (teacher forcing is the training branch of the decoders; dropout is off / patched to identity in every namespace)
    try:
        with torch.no_grad():
            if model == "case":
                eq, ep = m.query_encoder(q), m.passage_encoder(p)
                ps = m.passage_selection.action(q, p, encode_query=eq, encode_passage=ep)
                se = m.span_extraction.action(q, p, encode_query=eq, encode_passage=ep, passage_selection_result=ps)
                rg = m.response_generation.action(q, p, ns.build_map(sm, max=vocab), encode_query=eq, encode_passage=ep,
                                                  passage_selection_result=ps, span_extraction_result=se, output=output)
                dist = rg[2][0] + rg[2][1]
            else:
                eq, ep = m.query_encoder(q)[0][:, :, -1], m.passage_encoder(p)[0][:, :, -1]
                ps = m.passage_selection.action(q, p, encode_query=eq, encode_passage=ep)
                rg = m.response_generation.action(q, p, ns.build_map(sm, max=vocab), encode_query=eq, encode_passage=ep,
                                                  passage_selection_result=ps, output=output)
                dist = rg[2]
    finally:
        m.train(was_training)
    return dist[:, -1].float()
