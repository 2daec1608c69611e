#!/usr/bin/env python
"""Consensus answer selection: K30 + K31 on the device next to the host's ROUGE-L over the same pool, and what the consensus step adds to
a sampled decoding pass.

    python tools/consensus_bench.py [--out profiles/consensus_bench.json]

Kernel ("kernel" in the json): --items x N in {4, 8, 16} candidates x T --length positions, random ids from a --words vocabulary with random
lengths, the pool against itself (items x N^2 LCS problems):
  device   ops.sentence_compact + ops.lcs_pairs (K30) + ops.consensus_pick (K31), device events around --kernel-iters repetitions;
           "k30_k31" leaves the compaction out;
  host     evaluation.rouge.rouge_l over every pair of --host-items items of the same pool (a numpy DP per pair), the host clock, scaled to
           --items items: context, not a competitor -- it also needs the ids on the host first.
Passes ("passes"): ``do_sample`` and ``do_consensus`` at the same N and seed (CaSE, bf16, eager launches, B --batch, T --decode-len), the
host clock around a pass that ends in a synchronise, alternating; "added_ms" is the difference of the medians.
The event windows hold the wrappers' host work too, so they bound a kernel's time from above.  Stand-alone: bench.py does not call this.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
POOLS = (4, 8, 16)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--length", type=int, default=64)
    ap.add_argument("--words", type=int, default=200)
    ap.add_argument("--host-items", type=int, default=4)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--decode-len", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--enc-layers", type=int, default=3)
    ap.add_argument("--passages", type=int, default=10)
    ap.add_argument("--passage-len", type=int, default=384)
    ap.add_argument("--query-len", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-passes", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus_bench.json"))
    return ap.parse_args()


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise SystemExit("tools/consensus_bench.py measures on the GPU; there is none here")
    import case_rg_amd
    from case_rg_amd import evaluation, ops
    dev = torch.device("cuda")
    bos, pad, eos, unk, first = 1, 0, 2, 3, 4

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.kernel_iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / a.kernel_iters)
        return {"median": round(statistics.median(out), 1), "min": round(min(out), 1), "max": round(max(out), 1)}

    def kernel():
        points = []
        g = torch.Generator().manual_seed(7)
        for N in POOLS:
            B, T = a.items, a.length
            ids = torch.randint(first, first + a.words, (B, N, T), generator=g)
            lens = torch.randint(1, T, (B, N), generator=g)
            ids[torch.arange(T)[None, None, :] == lens[..., None]] = eos  # raw rows: the sentence, EOS, ids to be ignored
            cand = ids.to(dev)

            def whole():
                return evaluation.consensus(cand, (bos, pad, eos, unk))

            kept, count = ops.sentence_compact(cand.view(B * N, T), bos, pad, eos)
            kept, count = kept.view(B, N, T), count.view(B, N)

            def kernels():
                _, f = ops.lcs_pairs(kept, count, kept, count)
                return ops.consensus_pick(f, None, None, cand)

            with torch.no_grad():
                us = {"compact_k30_k31": timed(whole), "k30_k31": timed(kernels)}
                picked = whole()["consensus_index"][:a.host_items].tolist()
            rows, n = ids[:a.host_items].tolist(), lens[:a.host_items].tolist()
            t0 = time.perf_counter()
            host_pick = []
            for i in range(a.host_items):
                pool = [rows[i][k][:n[i][k]] for k in range(N)]
                util = [sum(evaluation.rouge_l(h, r)[0] for r in pool) for h in pool]
                host_pick.append(max(range(N), key=lambda k: (util[k], -k)))
            host_s = (time.perf_counter() - t0) * B / a.host_items
            points.append({"items": B, "pool": N, "length": T, "words": a.words, "pairs": B * N * N, "us_per_call": us,
                           "host_rouge_ms_scaled_to_items": round(host_s * 1e3, 1), "host_items_timed": a.host_items,
                           "host_over_device": round(host_s * 1e6 / us["compact_k30_k31"]["median"], 1),
                           "picks_agree_on_the_timed_items": host_pick == picked})
        return {"iters": a.kernel_iters, "repeats": a.repeats, "points": points}

    def passes():
        from case_rg_amd.CaSE.Model import CaSE
        from case_rg_amd.common.CumulativeTrainer import init_params
        from case_rg_amd.common.Utils import init_seed
        from case_rg_amd.utils import make_vocab, synth_batch
        case_rg_amd.set_compute_dtype(torch.bfloat16)
        init_seed(123456)
        v2i, i2v = make_vocab(a.vocab)
        model = CaSE(4, a.decode_len, i2v, v2i, a.hidden, enc_layers=a.enc_layers)
        init_params(model)
        model = model.to(dev).eval()
        model.response_generation.decoder.eos_check_every = 1 << 30
        batch = synth_batch(a.batch, a.passages, a.passage_len, a.query_len, 40, a.vocab, seed=123456, ragged=False)
        batch = {k: v.to(dev) for k, v in batch.items()}
        points = []
        with torch.no_grad():
            for N in POOLS:
                runs = {"sample": lambda: model.do_sample(dict(batch), num_samples=N, seed=11),
                        "consensus": lambda: model.do_consensus(dict(batch), num_samples=N, seed=11)}
                times = {n: [] for n in runs}
                for fn in runs.values():
                    for _ in range(a.warmup):
                        fn()
                torch.cuda.synchronize()
                for _ in range(a.steps):
                    for n, fn in runs.items():
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        times[n].append(time.perf_counter() - t0)
                med = {n: statistics.median(v) * 1e3 for n, v in times.items()}
                points.append({"batch": a.batch, "pool": N, "decode_len": a.decode_len, "sample_ms": round(med["sample"], 2),
                               "consensus_ms": round(med["consensus"], 2), "added_ms": round(med["consensus"] - med["sample"], 2),
                               "ms_min_max": {n: [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)] for n, v in times.items()}})
        return {"points": points}

    res = {"what": "consensus selection: compaction + K30 + K31 vs evaluation.rouge on the host; do_consensus vs do_sample, CaSE, bf16, eager",
           "config": {"batch": a.batch, "decode_len": a.decode_len, "hidden": a.hidden, "enc_layers": a.enc_layers, "passages": a.passages,
                      "passage_len": a.passage_len, "query_len": a.query_len, "vocab": a.vocab, "timed_passes": a.steps, "warmup": a.warmup},
           "device": torch.cuda.get_device_name(0), "kernel": kernel()}
    print(json.dumps(res["kernel"]))
    if not a.skip_passes:
        res["passes"] = passes()
        print(json.dumps(res["passes"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
