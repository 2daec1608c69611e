"""The eval modes of the generic ``TransformerSeqDecoder`` on the MI355X.  Its fixture (``cases.case_seq_decoder_generic``) covers the
training branch with dense maps only; greedy, beam, sampled decoding and scoring reach it through the dispatch it shares with the CaSE and
Masque decoders, here at the fixture's shapes with int64 id source maps given as a list, so the sorted, fused path runs."""
import numpy as np
import pytest
import torch

import cases
import sample_cases
from helpers import FP32_BAR, Calls, to_np

pytestmark = pytest.mark.gpu

T, BOS, UNK, EOS, PAD = 6, 1, 100, 2, 0


@pytest.fixture(scope="module")
def ns():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.float32)
    case_rg_amd.set_dropout(False)
    return case_rg_amd.namespace()


def _through_the_sample_loop(greedy):
    """What the sample loop emits for a greedy row, by the restatement tests/test_sample_cpu.py pins to the reference (``sample_cases.emit``):
    UNK for an EOS at step 0, the row up to its first EOS, EOS at the last step, PAD behind."""
    out, ended = [], False
    for t, x in enumerate(int(i) for i in greedy):
        tok, ended = sample_cases.emit(x, ended, t, T, EOS, UNK, PAD)
        out.append(tok)
    return out


def test_eval_modes_agree_with_greedy_fused_and_unfused(ns):
    from case_rg_amd import ops
    dev = torch.device("cuda")
    m = cases._mod(ns.TransformerSeqDecoder(2, 2, cases.HEADS, cases.V, cases.E), 131, dev).eval()
    b = cases.synth_batch(2, 3, 12, 8, 6, cases.V, seed=132)
    mems = [cases._rand(133, 2, 1, 8, cases.E).to(dev), cases._rand(134, 2, 3, 12, cases.E).to(dev)]
    maps = [b["query"].reshape(2, -1).to(dev), b["passage"].reshape(2, -1).to(dev)]
    masks = [b["query"].ne(0).to(dev), b["passage"].ne(0).to(dev)]
    sampling = dict(num_samples=1, temperature=1.0, top_k=1, top_p=1.0, seed=3, uniforms=None, eos=EOS, unk=UNK, pad=PAD)

    def run(**mode):
        return m(mems, BOS, UNK, maps, encode_masks=masks, **mode)

    answers, old = {}, ops.POINTER_HEAD
    try:
        for head in ("auto", "off"):
            ops.POINTER_HEAD = head
            with torch.no_grad(), Calls() as c:
                _, _, dist, greedy = run(max_target_length=T)
                beam = run(max_target_length=T, beam_width=1)[3]
                drawn = run(max_target_length=T, sampling=sampling)[3]
                scored = run(score_index=greedy)
            fused = (c.count("case_pointer_head_decode"), c.count("case_pointer_head_beam"))
            assert fused == ((T, T) if head == "auto" else (0, 0)) and c.sampled == T and m.last_greedy_steps == T, (head, c.calls)
            assert greedy.shape == (2, T) and dist.shape == (2, 1, cases.V)
            assert torch.equal(beam, greedy), "%s: beam_width=1 %s, greedy %s" % (head, beam.tolist(), greedy.tolist())
            want = [_through_the_sample_loop(row) for row in greedy.tolist()]
            assert drawn.tolist() == want, "%s: top_k=1 %s, greedy through the loop's conventions %s" % (head, drawn.tolist(), want)
            # the full-prefix pass against the cached step: p(last token | the tokens before it) is the entry of greedy's last-step row
            last = greedy[:, -1]
            keep = to_np(last.ne(PAD))  # scoring leaves PAD targets out (probability 1)
            assert keep.any(), "every greedy answer ends in PAD: nothing to compare"
            got = to_np(scored["token_probs"][:, 0, -1]).astype(np.float64)[keep]
            ref = to_np(dist[:, 0].gather(1, last.unsqueeze(1)).squeeze(1)).astype(np.float64)[keep]
            rel = float((np.abs(got - ref) / np.abs(ref)).max())
            print("%s: rescored last token vs greedy's row over %d items: %.3e" % (head, keep.sum(), rel))
            assert rel <= FP32_BAR, "%s: %.3e" % (head, rel)
            answers[head] = (greedy, beam, drawn)
    finally:
        ops.POINTER_HEAD = old
    for fused, plain in zip(answers["auto"], answers["off"]):
        assert torch.equal(fused, plain), "fused %s, unfused %s" % (fused.tolist(), plain.tolist())
