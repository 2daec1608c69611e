#!/usr/bin/env python
"""BLEU and n-gram overlap on the device: K34, K34 + K35 and consensus under BLEU next to consensus under ROUGE-L, the overlap of answers
with a long source row, and the host's ``evaluation.bleu`` over the same pools.

    python tools/bleu_bench.py [--out profiles/bleu_bench.json]

Pools ("pools" in the json): --items x N in {4, 8, 16} candidates x T --length positions, random ids from a --words vocabulary with random
lengths, the pool against itself (items x N^2 pairs).  Variants, timed ALTERNATELY (one window of --kernel-iters calls of each in turn,
--repeats rounds; median, min and max of the rounds, microseconds per call, device events):
  k34              ops.ngram_counts on the compacted pool
  k34_k35          ... + ops.bleu_scores (add-one smoothing, max_n 4)
  consensus_bleu   evaluation.consensus(metric="bleu"): compaction + K34 + K35 + K31
  consensus_rouge  evaluation.consensus(metric="rouge_l"): compaction + K30 + K31
  host             evaluation.bleu.sentence_bleu over every pair of --host-items items of the same pool, the host clock, scaled to --items
                   items: context, not a competitor -- it also needs the ids on the host first.
Overlap ("overlap"): ``evaluation.ngram_overlap_ids`` of --items answers of --length positions against one source row of --source-len tokens
each (compaction of both + K34), next to K34 alone on the compacted rows and to the compaction of the source rows alone (K13's
``sentence_compact`` walks a row with one thread), and the host's ``ngram_overlap`` for the four orders on --host-items of them, scaled.
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
    ap.add_argument("--source-len", type=int, default=3840)
    ap.add_argument("--host-items", type=int, default=4)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bleu_bench.json"))
    return ap.parse_args()


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bleu_bench.py measures on the GPU; there is none here")
    from case_rg_amd import evaluation, ops
    dev = torch.device("cuda")
    bos, pad, eos, unk, first = 1, 0, 2, 3, 4
    specials = (bos, pad, eos, unk)

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

    def raw(g, shape):
        """Raw rows: the sentence, EOS, ids to be ignored -> (ids on the host, lengths)."""
        ids = torch.randint(first, first + a.words, shape, generator=g)
        lens = torch.randint(1, shape[-1], shape[:-1], generator=g)
        ids[torch.arange(shape[-1]).view((1,) * (len(shape) - 1) + (-1,)) == lens[..., None]] = eos
        return ids, lens

    def pools():
        points = []
        g = torch.Generator().manual_seed(7)
        for N in POOLS:
            B, T = a.items, a.length
            ids, lens = raw(g, (B, N, T))
            cand = ids.to(dev)
            kept, count = ops.sentence_compact(cand.view(B * N, T), bos, pad, eos)
            kept, count = kept.view(B, N, T), count.view(B, N)
            variants = {"k34": lambda: ops.ngram_counts(kept, count, kept, count, 4),
                        "k34_k35": lambda: ops.bleu_scores(ops.ngram_counts(kept, count, kept, count, 4), count, count, 4, "add1"),
                        "consensus_bleu": lambda: evaluation.consensus(cand, specials, metric="bleu"),
                        "consensus_rouge": lambda: evaluation.consensus(cand, specials, metric="rouge_l")}
            with torch.no_grad():
                us = timed(variants)
                pair = variants["consensus_bleu"]()["pairwise_bleu"][:a.host_items].double().cpu()
            rows, n = ids[:a.host_items].tolist(), lens[:a.host_items].tolist()
            t0 = time.perf_counter()
            host = [[[evaluation.sentence_bleu(rows[i][x][:n[i][x]], [rows[i][y][:n[i][y]]], 4, "add1") for y in range(N)] for x in range(N)]
                    for i in range(a.host_items)]
            host_s = (time.perf_counter() - t0) * B / a.host_items
            points.append({"items": B, "pool": N, "length": T, "words": a.words, "pairs": B * N * N, "us_per_call": us,
                           "bleu_over_rouge_consensus": round(us["consensus_bleu"]["median"] / us["consensus_rouge"]["median"], 2),
                           "host_bleu_ms_scaled_to_items": round(host_s * 1e3, 1), "host_items_timed": a.host_items,
                           "host_over_device": round(host_s * 1e6 / us["k34_k35"]["median"], 1),
                           "max_abs_diff_to_host_on_the_timed_items": float((pair - torch.tensor(host, dtype=torch.float64)).abs().max())})
        return {"iters": a.kernel_iters, "repeats": a.repeats, "points": points}

    def overlap():
        g = torch.Generator().manual_seed(8)
        B = a.items
        ans, _ = raw(g, (B, a.length))
        src = torch.randint(first, first + a.words, (B, a.source_len), generator=g)
        src_len = torch.randint(max(a.source_len - 64, 1), a.source_len, (B,), generator=g)  # nearly full rows: the passages of an item
        src[torch.arange(a.source_len)[None, :] == src_len[:, None]] = eos
        d_ans, d_src = ans.to(dev), src.to(dev)
        with torch.no_grad():
            a_kept, a_len = ops.sentence_compact(d_ans, bos, pad, eos)
            s_kept, s_len = ops.sentence_compact(d_src, bos, pad, eos)
            a_kept, a_len, s_kept, s_len = a_kept.unsqueeze(1), a_len.unsqueeze(1), s_kept.unsqueeze(1), s_len.unsqueeze(1)
            us = timed({"ngram_overlap_ids": lambda: evaluation.ngram_overlap_ids(d_ans, d_src, specials),
                        "k34": lambda: ops.ngram_counts(a_kept, a_len, s_kept, s_len, 4),
                        "compact_source": lambda: ops.sentence_compact(d_src, bos, pad, eos)})
            got = evaluation.ngram_overlap_ids(d_ans, d_src, specials)[:a.host_items, 0].cpu()
        rows_a, rows_s = ans[:a.host_items].tolist(), src[:a.host_items].tolist()
        cut = lambda row: row[:row.index(eos)] if eos in row else row  # noqa: E731
        t0 = time.perf_counter()
        host = [[evaluation.ngram_overlap(cut(x), cut(y), k) for k in (1, 2, 3, 4)] for x, y in zip(rows_a, rows_s)]
        host_s = (time.perf_counter() - t0) * B / a.host_items
        return {"items": B, "answer_length": a.length, "source_len": a.source_len, "words": a.words, "us_per_call": us,
                "host_overlap_ms_scaled_to_items": round(host_s * 1e3, 1), "host_items_timed": a.host_items,
                "equal_to_host_on_the_timed_items": bool(torch.equal(got, torch.tensor(host, dtype=torch.float64)))}

    res = {"what": "BLEU on the device: K34, K34 + K35, consensus under BLEU vs under ROUGE-L, n-gram overlap with a long source row; "
                   "evaluation.bleu on the host as context",
           "device": torch.cuda.get_device_name(0), "pools": pools(), "overlap": overlap()}
    print(json.dumps(res["pools"]))
    print(json.dumps(res["overlap"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
