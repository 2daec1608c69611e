"""Generate the beam-search fixtures by running the reference's own ``Generations.beam`` (build container only).

    python tests/golden/gen_beam_golden.py       # writes tests/golden/beam_<model>_w<width>.npz

The reference's ``beam`` drives a model through ``encode / init_decoder_states / decode / generate / to_word /
generation_to_decoder_input``; its CaSE and Masque models decode inside ``forward`` and have none of these, so ``Adapter`` below supplies
them around the reference models: the decoder state is the prefix of ids, the step distribution is the teacher-forced ``action`` call of
``beam_cases.step_dists`` (what ``cases.case_case_test`` uses for its margins), ``to_word`` is the reference's ``topk``.  The reference's
``beam`` returns ids only; the normalised costs and the deciding gaps are recorded by running the plain-Python restatement of
tests/test_beam_cpu.py over the same adapter (same Python-float arithmetic as the reference's ``Node``) and asserting that it returns the
reference's ids.  Only data is written: inputs, answers, costs, gaps.  No-op when the reference is absent.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_golden  # noqa: E402


class Adapter(object):
    def __init__(self, ns, model, kind, bos):
        self.ns, self.model, self.kind, self.bos = ns, model, kind, bos

    def encode(self, data):
        return {"item": data["id"].clone()}  # (every step re-encodes the rows it is given: nothing to carry)

    def init_decoder_states(self, data, encode_outputs):
        return torch.zeros(data["id"].size(0), 0, dtype=torch.long)  # the prefix in front of the token ``decode`` is handed

    def generation_to_decoder_input(self, data, indices):
        return indices

    def decode(self, data, decoder_input, encode_outputs, decode_outputs):
        import beam_cases
        prefix = torch.cat([decode_outputs["state"], decoder_input.reshape(-1, 1)], dim=1)
        dist = beam_cases.step_dists(self.ns, self.model, data, self.kind, range(prefix.size(0)), prefix)
        return {"state": prefix, "dist": dist}

    def generate(self, data, encode_outputs, decode_outputs, softmax=True):
        return decode_outputs["dist"]

    def to_word(self, data, gen_output, k=5, sampling=False):
        return self.ns.topk(gen_output, k)


def run_case(ns, name, width, verbose=True):
    import beam_cases
    import common.Generations as generations
    from test_beam_cpu import beam_search, cut_at_eos, pack
    from case_rg_amd.common.Constants import BOS_WORD, EOS_WORD
    dev = torch.device("cpu")
    m, b = beam_cases.build(ns, dev, name)
    kind = beam_cases.BEAM_CASES[name][0]
    bos, eos = m.vocab2id[BOS_WORD], m.vocab2id[EOS_WORD]
    T, items = beam_cases.T, beam_cases.ITEMS
    adapter = Adapter(ns, m, kind, bos)
    with torch.no_grad():
        ref = generations.beam(adapter, dict(b), m.vocab2id, max_len=T, width=width)
    answer = np.zeros((items, T), dtype=np.int64)
    answer[:, :ref.size(1)] = ref.numpy()
    step = lambda rows, pre: beam_cases.step_dists(ns, m, b, kind, rows, pre)  # noqa: E731
    res = beam_search(step, items, width, T, bos, eos)
    rec = pack(res, width, T)
    greedy = pack(beam_search(step, items, 1, T, bos, eos), 1, T)["answer"]
    decisive = rec["gap"] > beam_cases.GAP
    for i in np.nonzero(decisive)[0]:
        assert np.array_equal(rec["answer"][i], answer[i]), "the restatement and the reference's beam disagree on decisive item %d" % i
    differs = [cut_at_eos(answer[i], eos) != cut_at_eos(greedy[i], eos) for i in range(items)]
    early = [r["eos_before_last"] for r in res]
    if verbose:
        print("%s w%d: gaps %s decisive %d/%d, beam != greedy %s, EOS before the last step %s" % (
            name, width, np.array2string(rec["gap"], precision=2), decisive.sum(), items, differs, early))
    ok = decisive.sum() * 2 >= items and any(differs) and any(early)
    out = {"in_" + k: b[k].numpy() for k in ("query", "passage", "source_map")}
    out.update(answer=answer, score=rec["beam_scores"][:, 0], beam_answers=rec["beam_answers"], beam_scores=rec["beam_scores"], gap=rec["gap"],
               greedy=greedy, eos_before_last=np.array(early), bos=np.int64(bos), eos=np.int64(eos))
    return ok, out


def main():
    if not os.path.isdir(gen_golden.REF):
        print("gen_beam_golden: %s not present; fixtures are generated in the build container only" % gen_golden.REF)
        return 0
    import beam_cases
    ns = gen_golden.reference_namespace()
    torch.manual_seed(0)
    for name in beam_cases.BEAM_CASES:
        for width in beam_cases.WIDTHS:
            ok, out = run_case(ns, name, width)
            assert ok, "%s w%d: needs >= half its items decisive, one beam answer that differs from greedy and one early EOS" % (name, width)
            path = os.path.join(HERE, "%s_w%d.npz" % (name, width))
            np.savez_compressed(path, **out)
            print("%-24s %3d arrays %8.1f KB" % (os.path.basename(path), len(out), os.path.getsize(path) / 1024))
    return 0


if __name__ == "__main__":
    sys.exit(main())
