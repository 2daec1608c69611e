#!/usr/bin/env python
"""ROUGE-N on the device: K43 alone over rows of three lengths, and the whole ``rouge_n_ids`` next to ``rouge_l_ids`` and ``bleu_ids``.

    python tools/rouge_n_bench.py [--out profiles/rouge_n_bench.json] [--bench-line FILE]

The method is tools/bleu_bench.py's: the variants are timed ALTERNATELY (one window of --kernel-iters calls of each in turn, --repeats rounds;
median, min and max of the rounds, microseconds per call, device events).  The event windows hold the wrappers' host work too -- the output
allocations and the ctypes call -- so they bound a kernel's time from above.
  "k43":      ops.ngram_distinct on --rows front-packed rows of Tb = 64, 1 000 and 3 840 ids from a --words vocabulary, every row nearly full
              (the quadratic cost of K43 shows in the two long ones), max_n 4 and max_n 2.
  "metrics":  --items items x N in {4, 8, 16} hypotheses x T --length positions against one reference row each, raw ids:
              rouge_n_ids (compaction of both sides + K34 + K43 + K44, max_n 2), rouge_l_ids (compaction + K30), bleu_ids (compaction + K34 +
              K35); and the host's ``evaluation.rouge_n`` for the orders 1 and 2 over --host-items of the items, scaled: context, not a
              competitor.
These figures are context, not bars, and nothing here is a speed claim.  --bench-line FILE: a json file with bench.py's default line of this
build and of the parent commit's, taken in turn; it is copied into the result under "bench_default".  Stand-alone: bench.py does not call this.
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
ROW_LENGTHS = (64, 1000, 3840)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=768)
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--length", type=int, default=64)
    ap.add_argument("--words", type=int, default=200)
    ap.add_argument("--host-items", type=int, default=4)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--bench-line", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rouge_n_bench.json"))
    return ap.parse_args()


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise SystemExit("tools/rouge_n_bench.py measures on the GPU; there is none here")
    from case_rg_amd import evaluation, ops
    dev = torch.device("cuda")
    bos, pad, eos, unk, first = 1, 0, 2, 3, 4
    specials = (bos, pad, eos, unk)

    def timed(variants, iters):
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
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                out[n].append(e0.elapsed_time(e1) * 1e3 / iters)
        return {n: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for n, v in out.items()}

    def k43():
        points = []
        g = torch.Generator().manual_seed(43)
        for Tb in ROW_LENGTHS:
            ids = torch.randint(first, first + a.words, (a.rows, Tb), generator=g).to(dev)
            lens = torch.randint(max(Tb - 16, 1), Tb + 1, (a.rows,), generator=g).int().to(dev)
            iters = a.kernel_iters if Tb <= 1000 else max(a.kernel_iters // 5, 2)  # (a long row costs its length squared)
            us = timed({"max_n_4": lambda: ops.ngram_distinct(ids, lens, 4), "max_n_2": lambda: ops.ngram_distinct(ids, lens, 2)}, iters)
            row = ids[0, :int(lens[0])].tolist()
            want = [len({tuple(row[i:i + k]) for i in range(len(row) - k + 1)}) for k in (1, 2, 3, 4)]
            points.append({"rows": a.rows, "Tb": Tb, "words": a.words, "iters": iters, "us_per_call": us,
                           "row_0_equals_the_set": ops.ngram_distinct(ids[:1], lens[:1], 4)[0].tolist() == want})
        return {"repeats": a.repeats, "points": points}

    def metrics():
        points = []
        g = torch.Generator().manual_seed(44)
        for N in POOLS:
            B, T = a.items, a.length
            hyp = torch.randint(first, first + a.words, (B, N, T), generator=g)
            ref = torch.randint(first, first + a.words, (B, T), generator=g)
            hyp_len, ref_len = torch.randint(1, T, (B, N), generator=g), torch.randint(1, T, (B,), generator=g)
            hyp[torch.arange(T).view(1, 1, -1) == hyp_len[..., None]] = eos
            ref[torch.arange(T).view(1, -1) == ref_len[..., None]] = eos
            d_hyp, d_ref = hyp.to(dev), ref.to(dev)
            with torch.no_grad():
                us = timed({"rouge_n_ids": lambda: evaluation.rouge_n_ids(d_hyp, d_ref, specials, 2),
                            "rouge_l_ids": lambda: evaluation.rouge_l_ids(d_hyp, d_ref, specials),
                            "bleu_ids": lambda: evaluation.bleu_ids(d_hyp, d_ref, specials)}, a.kernel_iters)
                got = evaluation.rouge_n_ids(d_hyp, d_ref, specials, 2)["f"][:a.host_items, :, :2].cpu()
            t0 = time.perf_counter()
            host = [[[evaluation.rouge_n(hyp[i, n, :hyp_len[i, n]].tolist(), ref[i, :ref_len[i]].tolist(), k)[0] for k in (1, 2)]
                     for n in range(N)] for i in range(a.host_items)]
            host_s = (time.perf_counter() - t0) * B / a.host_items
            points.append({"items": B, "hypotheses": N, "length": T, "words": a.words, "pairs": B * N, "us_per_call": us,
                           "rouge_n_over_rouge_l": round(us["rouge_n_ids"]["median"] / us["rouge_l_ids"]["median"], 2),
                           "rouge_n_over_bleu": round(us["rouge_n_ids"]["median"] / us["bleu_ids"]["median"], 2),
                           "host_rouge_n_ms_scaled_to_items": round(host_s * 1e3, 1), "host_items_timed": a.host_items,
                           "max_abs_diff_to_host_on_the_timed_items": float((got - torch.tensor(host, dtype=torch.float64)).abs().max())})
        return {"iters": a.kernel_iters, "repeats": a.repeats, "points": points}

    res = {"what": "ROUGE-N on the device: K43 over rows of three lengths; rouge_n_ids next to rouge_l_ids and bleu_ids; evaluation.rouge_n on "
                   "the host as context.  Context, not bars.",
           "device": torch.cuda.get_device_name(0), "k43": k43(), "metrics": metrics()}
    if a.bench_line:
        with open(a.bench_line) as fh:
            res["bench_default"] = json.load(fh)
    print(json.dumps(res["k43"]))
    print(json.dumps(res["metrics"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
