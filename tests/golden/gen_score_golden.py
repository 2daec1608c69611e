"""Generate the scoring fixtures from the reference's own teacher-forced training branch (build container only).

    python tests/golden/gen_score_golden.py            # writes tests/golden/score_<case>.npz
    python tests/golden/gen_score_golden.py --search   # prints, per case, the first (model seed, batch seed, candidate seed) that qualify

One pass per candidate through ``score_cases.forced_probs`` (``m.train()`` in ``gen_golden.reference_namespace()``, whose dropout is the
identity): the probability of every candidate token, its pointer part where the reference returns it (CaSE's ``(dist1, dist2)``) and the
generator's own probability.  Only data is written: inputs, candidates, probabilities and the restated reductions.  No-op when the
reference is absent.
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


def run_case(ns, name, seeds=None, verbose=True):
    import score_cases
    from case_rg_amd.common.Constants import EOS_WORD, PAD_WORD
    if seeds is not None:
        score_cases.SCORE_CASES[name] = (score_cases.SCORE_CASES[name][0],) + tuple(seeds)
    kind, _, _, cseed = score_cases.SCORE_CASES[name]
    m, b = score_cases.build(ns, torch.device("cpu"), name)
    eos, pad = m.vocab2id[EOS_WORD], m.vocab2id[PAD_WORD]
    cands = score_cases.candidates(b, eos, cseed)
    p, ptr, gen = score_cases.forced_all(ns, m, b, kind, cands)
    ans, src = cands.numpy(), b["source_map"].numpy()
    scored = ans != pad
    occurs = (src[:, None, None, :] == ans[..., None]).sum(-1)  # [B, N, T] how often each target occurs in its item's source
    # what the fixture must pin, on the reference alone
    floor_ok = bool((p[scored] >= score_cases.P_MIN).all())
    # the pointer part is at least half of p: read from dist2 where the reference returns it; otherwise from p - gen[y] <= the pointer part
    # (p = p0 gen[y] + pointer part with p0 <= 1)
    lower = ptr if ptr is not None else p - gen
    pointer_ok = bool((scored & (lower >= 0.5 * p)).any())
    twice_ok = bool((scored & (occurs >= 2)).any())
    absent = scored & (occurs == 0)
    absent_ok = bool(absent.any()) and (ptr is None or bool((ptr[absent] == 0).all()))
    tails = [(~scored[i, n]).any() for i in range(ans.shape[0]) for n in range(ans.shape[1])]
    tail_ok = any(tails) and not all(tails)
    ok = floor_ok and pointer_ok and twice_ok and absent_ok and tail_ok
    if verbose:
        print("%s %s: min p %.3e, pointer >= p/2 %s, twice in source %s, absent (copy 0) %s, PAD tail some/not all %s" % (
            name, score_cases.SCORE_CASES[name][1:], p[scored].min(), pointer_ok, twice_ok, absent_ok, tail_ok))
    red = score_cases.reductions(p, ans, pad)
    out = {"in_" + k: b[k].numpy() for k in ("query", "passage", "source_map", "response")}
    out.update(answers=ans, p=p.astype(np.float32), gen=gen.astype(np.float32), occurs=occurs.astype(np.int64), scores=red["scores"],
               loss=np.float64(red["loss"]), tokens=np.int64(red["tokens"]), eos=np.int64(eos), pad=np.int64(pad),
               seeds=np.array(score_cases.SCORE_CASES[name][1:], dtype=np.int64))
    if ptr is not None:
        out["ptr"] = ptr.astype(np.float32)
    return ok, out


def main():
    if not os.path.isdir(gen_golden.REF):
        print("gen_score_golden: %s not present; fixtures are generated in the build container only" % gen_golden.REF)
        return 0
    import score_cases
    ns = gen_golden.reference_namespace()
    torch.manual_seed(0)
    if "--search" in sys.argv:
        for name in score_cases.SCORE_CASES:
            start = score_cases.SCORE_CASES[name][1:3]
            grid = [start + (c,) for c in range(1, 6)] + [(ms, bs, c) for ms in range(1, 12) for bs in range(11, 14) for c in (1, 2)]
            print(name, [s for s in grid if run_case(ns, name, s, verbose=False)[0]][:3])
        return 0
    for name in score_cases.SCORE_CASES:
        ok, out = run_case(ns, name)
        assert ok, ("%s: every scored target needs p >= 1e-4; one needs a pointer part >= p / 2, one must occur twice in its source, one must "
                    "be absent from it (copy exactly 0), and the candidates need a PAD tail on some and none on others" % name)
        path = os.path.join(HERE, "%s.npz" % name)
        np.savez_compressed(path, **out)
        print("%-32s %3d arrays %8.1f KB" % (os.path.basename(path), len(out), os.path.getsize(path) / 1024))
    return 0


if __name__ == "__main__":
    sys.exit(main())
