"""Generate the sampled-decoding fixtures by running the reference's own ``Generations.sample`` (build container only).

    python tests/golden/gen_sample_golden.py            # writes tests/golden/sample_<case>.npz
    python tests/golden/gen_sample_golden.py --search   # prints, per case, the first draw seeds that satisfy the assertions below

The reference's ``sample`` drives a model through the same interface as its ``beam``; ``Adapter`` is gen_beam_golden.py's, with
``to_word(sampling=True)`` applying the restated draw rule (sample_cases.draw) to the distribution ``generate`` stashed -- the product's
deliberate deviation: the reference draws from Categorical(logits = softmax(p)), which is nearly uniform over the vocabulary -- with
u = rng_uniform24(draw seed, t * ITEMS + row).  The loop itself (UNK for EOS at step 0, the forced EOS, PAD behind the end) is the
reference's code.  Only data is written: inputs, answers, the drawn ids, uniforms, margins, probabilities, the greedy answer.  No-op when
the reference is absent.
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
from gen_beam_golden import Adapter  # noqa: E402


class SamplingAdapter(Adapter):
    def __init__(self, ns, model, kind, bos, params, uniforms):
        super().__init__(ns, model, kind, bos)
        self.params, self.uniforms, self.t, self.dist = params, uniforms, 0, None
        self.drawn, self.prob, self.margin = [], [], []

    def generate(self, data, encode_outputs, decode_outputs, softmax=True):
        self.dist = decode_outputs["dist"]
        return self.dist

    def to_word(self, data, gen_output, k=5, sampling=False):
        if not sampling:
            return self.ns.topk(gen_output, k)
        import sample_cases
        rows = self.dist.double().numpy()
        ds = [sample_cases.draw(rows[i], *self.params, float(self.uniforms[i, self.t])) for i in range(rows.shape[0])]
        self.t += 1
        self.drawn.append([d["id"] for d in ds])
        self.prob.append([d["prob"] for d in ds])
        self.margin.append([d["margin"] for d in ds])
        ids = torch.tensor([[d["id"]] for d in ds], dtype=torch.long)
        return torch.tensor([[d["prob"]] for d in ds]), ids  # (the loop rewrites ``ids`` in place: ``drawn`` keeps the draws)


def run_case(ns, name, draw_seed=None, verbose=True):
    import beam_cases
    import sample_cases
    import common.Generations as generations
    from case_rg_amd.common.Constants import BOS_WORD, EOS_WORD, PAD_WORD, UNK_WORD
    kind, _, _, seed, params = sample_cases.SAMPLE_CASES[name]
    seed = seed if draw_seed is None else draw_seed
    m, b = sample_cases.build(ns, torch.device("cpu"), name)
    v2i = m.vocab2id
    bos, eos, unk, pad = v2i[BOS_WORD], v2i[EOS_WORD], v2i[UNK_WORD], v2i[PAD_WORD]
    T, items = sample_cases.T, sample_cases.ITEMS
    u = sample_cases.case_uniforms(seed)
    adapter = SamplingAdapter(ns, m, kind, bos, params, u)
    with torch.no_grad():
        answer = generations.sample(adapter, dict(b), v2i, max_len=T)[0].numpy().astype(np.int64)
        greedy = generations.greedy(Adapter(ns, m, kind, bos), dict(b), v2i, max_len=T).numpy().astype(np.int64)
    assert answer.shape == (items, T) and greedy.shape == (items, T)
    drawn, prob, margin = np.array(adapter.drawn).T, np.array(adapter.prob).T, np.array(adapter.margin).T
    # behind the end of a row its draws decide nothing: probability 1, margin inf (what sample_cases.sample_loop records)
    ended = np.zeros(items, dtype=bool)
    for t in range(T):
        prob[ended, t], margin[ended, t] = 1.0, np.inf
        ended |= drawn[:, t] == eos
    # the restated loop over the same distributions must emit what the reference's loop emitted
    step = lambda rows, pre: beam_cases.step_dists(ns, m, b, kind, rows, pre)  # noqa: E731
    again = sample_cases.sample_loop(step, items, T, bos, eos, unk, pad, params, u)
    assert np.array_equal(again["answer"], answer), "the restated loop and the reference's sample disagree"
    assert np.array_equal(again["prob"], prob) and np.array_equal(again["margin"], margin)
    steps = sample_cases.decisive_steps(margin)
    differs = [not np.array_equal(answer[i], greedy[i]) for i in range(items)]
    # an early end is a *drawn* EOS before the last step (at t = 0 it is emitted as UNK).  A PAD in the answer proves nothing: PAD is an
    # ordinary id that a live row may draw.  The row must also be decisive throughout, so that the fixture pins the end itself.
    early = [bool((drawn[i, :T - 1] == eos).any() and steps[i] == T) for i in range(items)]
    if verbose:
        print("%s seed %d: decisive steps %s, min margins %s, sample != greedy %s, ends before the last step %s" % (
            name, seed, steps, np.array2string(margin.min(axis=1), precision=2), differs, early))
    ok = (steps == T).sum() * 2 >= items and any(differs) and any(early)
    out = {"in_" + k: b[k].numpy() for k in ("query", "passage", "source_map")}
    out.update(answer=answer, drawn=drawn.astype(np.int64), u=u, margin=margin, prob=prob, greedy=greedy, bos=np.int64(bos), eos=np.int64(eos),
               unk=np.int64(unk), pad=np.int64(pad), seed=np.int64(seed), params=np.array(params, dtype=np.float64))
    return ok, out


def main():
    if not os.path.isdir(gen_golden.REF):
        print("gen_sample_golden: %s not present; fixtures are generated in the build container only" % gen_golden.REF)
        return 0
    import sample_cases
    ns = gen_golden.reference_namespace()
    torch.manual_seed(0)
    if "--search" in sys.argv:
        for name in sample_cases.SAMPLE_CASES:
            print(name, [s for s in range(1, 40) if run_case(ns, name, s, verbose=False)[0]][:5])
        return 0
    for name in sample_cases.SAMPLE_CASES:
        ok, out = run_case(ns, name)
        assert ok, "%s: needs >= half its items decisive through all steps, one sampled answer that differs from greedy and one decisive row that draws EOS before the last step" % name
        path = os.path.join(HERE, "%s.npz" % name)
        np.savez_compressed(path, **out)
        print("%-32s %3d arrays %8.1f KB" % (os.path.basename(path), len(out), os.path.getsize(path) / 1024))
    return 0


if __name__ == "__main__":
    sys.exit(main())
