#!/usr/bin/env python
"""TREC ranking metrics on the device: K36 next to the host's ``evaluation.trec`` on the same lists, and a rank-only pass next to a greedy
pass.

    python tools/rank_bench.py [--out profiles/rank_bench.json]

Kernel ("kernel" in the json): --items queries x P in {10, 1000} document slots, scores from 32 values (ties are common), tie keys a
permutation, grades 0 .. 4, 7 judged-but-unretrieved grades per query.  Variants, timed ALTERNATELY (one window of --kernel-iters calls of
each in turn, --repeats rounds; median, min and max of the rounds, microseconds per call, device events):
  k36            ops.rank_metrics on prepared f32 / int32 tensors
  rank_ids       evaluation.rank_metrics_ids from int64 grades and keys: the casts + K36 + the column views
  eval_rank_ids  ... + the column sums (what CumulativeTrainer.evaluate_rank runs per batch)
  host           evaluation.rank_metrics over --host-items of the same lists as dicts, the host clock, scaled to --items: context, not a
                 competitor -- it also needs the scores on the host first.
The event windows hold the wrappers' host work too (output allocations, the ctypes call), so they bound the kernel's time from above.
Passes ("passes"): CaSE, bf16, --batch items, ``do_rank`` next to ``do_test`` (--decode-len cached steps), eager, alternating, the host
clock around a pass that ends in a device synchronise; medians of --steps passes.  Stand-alone: bench.py does not call this.
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
DEPTHS = (10, 1000)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--extra", type=int, default=7)
    ap.add_argument("--host-items", type=int, default=16)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--decode-len", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--enc-layers", type=int, default=3)
    ap.add_argument("--passages", type=int, default=10)
    ap.add_argument("--passage-len", type=int, default=384)
    ap.add_argument("--query-len", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-passes", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_bench.json"))
    return ap.parse_args()


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise SystemExit("tools/rank_bench.py measures on the GPU; there is none here")
    import case_rg_amd
    from case_rg_amd import evaluation, ops
    dev = torch.device("cuda")

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

    def kernel():
        points = []
        g = torch.Generator().manual_seed(7)
        B, R = a.items, a.extra
        for P in DEPTHS:
            scores = torch.randint(0, 32, (B, P), generator=g).float() / 8
            keys = torch.stack([torch.randperm(P, generator=g) for _ in range(B)])
            grades = torch.randint(0, 5, (B, P), generator=g) * (torch.rand(B, P, generator=g) < 0.2)
            extra = torch.randint(0, 5, (B, R), generator=g)
            d = {k: v.to(dev) for k, v in dict(scores=scores, keys=keys, grades=grades, extra=extra).items()}
            k32, g32, e32 = d["keys"].int(), d["grades"].int(), d["extra"].int()
            variants = {"k36": lambda: ops.rank_metrics(d["scores"], g32, k32, None, e32),
                        "rank_ids": lambda: evaluation.rank_metrics_ids(d["scores"], d["grades"], d["keys"], None, d["extra"]),
                        "eval_rank_ids": lambda: evaluation.eval_rank_ids(d["scores"], d["grades"], d["keys"], None, d["extra"])}
            us = timed(variants)
            got = variants["rank_ids"]()
            n = min(a.host_items, B)
            docid = lambda k: "%04d" % k  # noqa: E731
            run = {i: {docid(int(k)): float(s) for k, s in zip(keys[i], scores[i])} for i in range(n)}
            qrel = {i: dict({docid(int(k)): int(x) for k, x in zip(keys[i], grades[i])}, **{"x%d" % j: int(x) for j, x in enumerate(extra[i])})
                    for i in range(n)}
            t0 = time.perf_counter()
            host = evaluation.rank_metrics(run, qrel)
            host_s = (time.perf_counter() - t0) * B / n
            gap = max(abs(float(got[name][i]) - host[i][name]) for i in range(n) for name in ops.RANK_METRICS)
            points.append({"items": B, "depth": P, "extra": R, "us_per_call": us, "host_ms_scaled_to_items": round(host_s * 1e3, 2),
                           "host_items_timed": n, "host_over_device": round(host_s * 1e6 / us["k36"]["median"], 1),
                           "max_abs_diff_to_host_on_the_timed_items": gap})
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
        with torch.no_grad():
            runs = {"rank": lambda: model.do_rank(dict(batch)), "test": lambda: model.do_test(dict(batch)),
                    "rank_and_metrics": lambda: evaluation.eval_rank_ids(model.do_rank(dict(batch))["rank"], batch["passage_label"])}
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
            same = bool(torch.equal(runs["rank"]()["rank"], runs["test"]()["rank"]))
        med = {n: statistics.median(v) * 1e3 for n, v in times.items()}
        return {"batch": a.batch, "decode_len": a.decode_len, "do_rank_ms": round(med["rank"], 2), "do_test_ms": round(med["test"], 2),
                "do_rank_and_metrics_ms": round(med["rank_and_metrics"], 2), "test_over_rank": round(med["test"] / med["rank"], 1),
                "rank_equal_bits": same, "ms_min_max": {n: [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)] for n, v in times.items()}}

    res = {"what": "TREC ranking metrics: K36 vs evaluation.trec on the host; do_rank vs do_test, CaSE, bf16, eager",
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
