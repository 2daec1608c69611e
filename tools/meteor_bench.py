#!/usr/bin/env python
"""METEOR on the device: K40 with and without a class table and with and without the alignment output, next to K34 + K35 (BLEU) on the
same operands and to the host's ``evaluation.meteor`` over the same pools.

    python tools/meteor_bench.py [--out profiles/meteor_bench.json]

Pools: --items x N in {4, 8, 16} candidates x T --length positions, random ids from a --words vocabulary with random lengths, the pool
against itself (one candidate per reference row: items x N^2 pairs), as tools/bleu_bench.py sets them up.  Variants, timed ALTERNATELY (one
window of --kernel-iters calls of each in turn, --repeats rounds; median, min and max of the rounds, microseconds per call, device events):
  k40                ops.meteor on the compacted pool, exact matches only
  k40_classes        ... with a class table that joins neighbouring ids in pairs (the second backward pass runs)
  k40_align          exact matches only, with the alignment output [B, N, N, T]
  k40_classes_align  both
  k34_k35            ops.ngram_counts + ops.bleu_scores (add-one smoothing, max_n 4): the nearest sibling, as context, not a bar
  host               evaluation.meteor.pair_meteor over every pair of --host-items items of the same pool, the host clock, scaled to --items
                     items: context, not a competitor -- it also needs the ids on the host first.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meteor_bench.json"))
    return ap.parse_args()


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise SystemExit("tools/meteor_bench.py measures on the GPU; there is none here")
    from case_rg_amd import evaluation, ops
    dev = torch.device("cuda")
    bos, pad, eos, first = 1, 0, 2, 4

    def timed(variants):
        """{name: fn} -> {name: {median, min, max}} in microseconds per call; the variants take turns inside every round."""
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        out = {n: [] for n in variants}
        for _ in range(a.repeats):
            for n, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.kernel_iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                out[n].append(e0.elapsed_time(e1) * 1e3 / a.kernel_iters)
        return {n: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for n, v in out.items()}

    table = torch.full((first + a.words,), -1, dtype=torch.int32)
    table[first:] = torch.arange(a.words, dtype=torch.int32) // 2
    classes, by_id = table.to(dev), table.tolist()
    points = []
    g = torch.Generator().manual_seed(7)
    for N in POOLS:
        B, T = a.items, a.length
        ids = torch.randint(first, first + a.words, (B, N, T), generator=g)
        lens = torch.randint(1, T, (B, N), generator=g)
        ids[torch.arange(T).view(1, 1, -1) == lens[..., None]] = eos
        kept, count = ops.sentence_compact(ids.to(dev).view(B * N, T), bos, pad, eos)
        kept, count = kept.view(B, N, T), count.view(B, N)
        variants = {"k40": lambda: ops.meteor(kept, count, kept, count),
                    "k40_classes": lambda: ops.meteor(kept, count, kept, count, classes),
                    "k40_align": lambda: ops.meteor(kept, count, kept, count, want_align=True),
                    "k40_classes_align": lambda: ops.meteor(kept, count, kept, count, classes, want_align=True),
                    "k34_k35": lambda: ops.bleu_scores(ops.ngram_counts(kept, count, kept, count, 4), count, count, 4, "add1")}
        with torch.no_grad():
            us = timed(variants)
            got = variants["k40_classes"]()
            pair, counts = got["meteor_pair"][:a.host_items].double().cpu(), got["counts"][:a.host_items].cpu()
        rows, n = ids[:a.host_items].tolist(), lens[:a.host_items].tolist()
        t0 = time.perf_counter()
        host = [[[evaluation.pair_meteor(rows[i][x][:n[i][x]], rows[i][y][:n[i][y]], by_id) for y in range(N)] for x in range(N)]
                for i in range(a.host_items)]
        host_s = (time.perf_counter() - t0) * B / a.host_items
        want = torch.tensor([[[p["score"] for p in row] for row in item] for item in host], dtype=torch.float64)
        want_counts = torch.tensor([[[[p["matches"], p["exact"], p["chunks"]] for p in row] for row in item] for item in host], dtype=torch.int32)
        points.append({"items": B, "pool": N, "length": T, "words": a.words, "pairs": B * N * N, "us_per_call": us,
                       "classes_over_exact": round(us["k40_classes"]["median"] / us["k40"]["median"], 2),
                       "align_over_none": round(us["k40_align"]["median"] / us["k40"]["median"], 2),
                       "k40_over_k34_k35": round(us["k40"]["median"] / us["k34_k35"]["median"], 2),
                       "host_meteor_ms_scaled_to_items": round(host_s * 1e3, 1), "host_items_timed": a.host_items,
                       "host_over_device": round(host_s * 1e6 / us["k40_classes"]["median"], 1),
                       "counts_equal_to_host_on_the_timed_items": bool(torch.equal(counts, want_counts)),
                       "max_abs_diff_to_host_on_the_timed_items": float((pair - want).abs().max())})
    res = {"what": "METEOR on the device: K40 exact / with a class table / with the alignment output, K34 + K35 (BLEU) on the same operands "
                   "and evaluation.meteor on the host as context",
           "device": torch.cuda.get_device_name(0), "iters": a.kernel_iters, "repeats": a.repeats, "points": points}
    print(json.dumps(res["points"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
