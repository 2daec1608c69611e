#!/usr/bin/env python
"""Beam search next to greedy decoding at the cfg 4 decode geometry (bench.py --mode decode: d_model 512, 3 encoder layers, ten 384-token
passages, 64-token answers, vocabulary 30 522, bf16).

    python tools/beam_bench.py [--out profiles/beam_bench.json]

For W in {1, 2, 4, 8} the batch is 256 / W items, so that every cached step runs on B * W = 256 rows -- the row count of the greedy step at
batch 256, which is the yardstick.  Reported per point: answers/s of the whole pass (encode + T cached steps) and the ms of one cached step,
(T-step pass - 1-step pass) / (T - 1) as bench.py's phase split takes it.  The expectation under test: a beam step costs the greedy step at
the same row count plus the three extra launches (K25 merge, K26 cache reorder, K24's top-W tail instead of the argmax).
The launches themselves are timed alone at the same row count ("kernels" in the json, device events over --kernel-iters launches): K23 as
greedy decoding calls it (with and without the gen / dist write-back), K24 and K25 per width, K26 at the first, the middle and the last step.
Stand-alone: bench.py does not call this.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256, help="B * W, the rows of every cached step")
    ap.add_argument("--widths", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--decode-len", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--enc-layers", type=int, default=3)
    ap.add_argument("--passages", type=int, default=10)
    ap.add_argument("--passage-len", type=int, default=384)
    ap.add_argument("--query-len", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_bench.json"))
    return ap.parse_args()


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    a = parse()
    import case_rg_amd
    from case_rg_amd.CaSE.Model import CaSE
    from case_rg_amd.common.CumulativeTrainer import init_params
    from case_rg_amd.common.Utils import init_seed
    from case_rg_amd.utils import make_vocab, synth_batch
    case_rg_amd.set_compute_dtype(torch.bfloat16)
    dev = torch.device("cuda")
    init_seed(123456)
    v2i, i2v = make_vocab(a.vocab)
    model = CaSE(4, a.decode_len, i2v, v2i, a.hidden, enc_layers=a.enc_layers)
    init_params(model)
    model = model.to(dev).eval()
    dec = model.response_generation.decoder
    dec.eos_check_every = 1 << 30  # every pass runs its full length: no look at the device, no early end

    def point(items, width):
        batch = synth_batch(items, a.passages, a.passage_len, a.query_len, 40, a.vocab, seed=123456, ragged=False)
        batch = {k: v.to(dev) for k, v in batch.items()}

        def run():
            with torch.no_grad():
                return model(dict(batch), method="test") if width is None else model.do_beam(dict(batch), width=width)

        T = a.decode_len
        model.max_target_length = T
        full = timed(run, a.warmup, a.steps)
        model.max_target_length = 1
        one = timed(run, a.warmup, a.steps)
        model.max_target_length = T
        return {"decoder": "greedy" if width is None else "beam", "width": width, "items": items, "rows": items * (width or 1),
                "answers_per_s": round(items / full, 2), "ms_per_pass": round(full * 1e3, 2), "ms_one_step_pass": round(one * 1e3, 2),
                "ms_per_cached_step": round((full - one) / (T - 1) * 1e3, 4)}

    def launches(fn):
        """us per launch: device events around --kernel-iters back-to-back launches."""
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.kernel_iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) * 1e3 / a.kernel_iters, 2)

    def kernels():
        from case_rg_amd import ops
        R, V, T = a.rows, a.vocab, a.decode_len
        lens = [a.query_len, a.passages * a.passage_len]
        g = torch.Generator(device="cuda").manual_seed(3)
        logits = torch.randn(R, V, device=dev, generator=g) * 2.0
        mix = torch.randn(R, 1 + len(lens), device=dev, generator=g)
        src = ops.SortedSource(torch.randint(4, V, (R, sum(lens)), device=dev, generator=g), V)
        copies = [torch.softmax(torch.randn(R, n, device=dev, generator=g) * 2.0, dim=-1) for n in lens]
        out = {"rows": R, "iters": a.kernel_iters,
               "K23_us_with_gen_dist": launches(lambda: ops.pointer_head_decode(logits, mix, src, copies)),
               "K23_us_ids_only": launches(lambda: ops.pointer_head_decode(logits, mix, src, copies, want_gen=False, want_dist=False))}
        layers = sum(len(d.layers) for d in dec.decs)
        E = dec.hidden_size
        ka = [torch.randn(R, T, 2 * E, device=dev, generator=g).to(torch.bfloat16) for _ in range(layers)]
        kb = [torch.zeros_like(k) for k in ka]
        va, vb = torch.ones(R, T, dtype=torch.bool, device=dev), torch.zeros(R, T, dtype=torch.bool, device=dev)
        out["K26_layers"] = layers
        for w in a.widths:
            out["K24_us_w%d" % w] = launches(lambda: ops.pointer_head_topk(logits, mix, src, copies, w))
            _, _, cand_p, cand_id = ops.pointer_head_topk(logits, mix, src, copies, w)
            state = ops.BeamState(R // w, w, a.kernel_iters + 16, dev)  # a history long enough for every timed launch to be a middle step
            step = [0]

            def advance():
                ops.beam_advance(state, cand_p, cand_id, step[0], -1)
                step[0] += 1

            out["K25_us_w%d" % w] = launches(advance)
            parent = torch.randint(0, w, (R // w, w), device=dev, generator=g, dtype=torch.int32)
            for t in (0, T // 2 - 1, T - 2):
                out["K26_us_w%d_t%d" % (w, t)] = launches(lambda: ops.beam_gather(ka, kb, parent, t, va, vb))
        return out

    points = [point(a.rows, None)]
    for w in a.widths:
        points.append(point(a.rows // w, w))
    greedy = points[0]["ms_per_cached_step"]
    for p in points[1:]:
        p["step_vs_greedy_step"] = round(p["ms_per_cached_step"] / greedy, 3)
    res = {"what": "beam search vs greedy decoding, CaSE, cfg 4 decode geometry, bf16, eager launches",
           "config": {"rows_per_step": a.rows, "decode_len": a.decode_len, "hidden": a.hidden, "enc_layers": a.enc_layers, "passages": a.passages,
                      "passage_len": a.passage_len, "query_len": a.query_len, "vocab": a.vocab, "timed_passes": a.steps, "warmup": a.warmup},
           "device": torch.cuda.get_device_name(0), "points": points, "kernels": kernels()}
    for p in points:
        print(json.dumps(p))
    print(json.dumps(res["kernels"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
