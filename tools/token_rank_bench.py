#!/usr/bin/env python
"""Token ranking metrics: K45 next to K38 on the same rows and next to a restatement in torch on the device.

    python tools/token_rank_bench.py [--out profiles/token_rank_bench.json]

The method of tools/token_label_bench.py: the variants are timed ALTERNATELY (one window of --kernel-iters calls of each in turn, --repeats
rounds; median, min and max of the rounds, microseconds per call, device events; the windows hold the wrappers' host work too -- output
allocations, the ctypes call -- so they bound a kernel's time from above).
Points: --points items x positions (default 32 x 3840, 256 x 3840, 32 x 16384), a tenth of the positions invalid, a tenth of the labels
positive, for two kinds of scores: "bf16" (normal draws rounded to bf16: many ties) and "f32" (normal draws: none).
  k45         ops.token_rank
  k38_counts  ops.token_select(k = 32) with labels on the same rows: context -- what the stage's fixed-point counts cost -- not a bar
  torch_form  torch.sort + cumsum in f64 on the device, AP and AUC by position in the sorted row: it breaks ties by position instead of
              grouping them and has no best cut, so it restates the tie-free figures only: context, not a bar
Stand-alone: bench.py does not call this.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[32, 3840, 256, 3840, 32, 16384], help="items positions, repeated")
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_rank_bench.json"))
    return ap.parse_args()


def torch_form(scores, valid, labels):
    """AP and AUC of every row by position in a descending sort: equal to K45's on rows without ties."""
    key = torch.where(torch.isnan(scores), torch.full_like(scores, -math.inf), scores).masked_fill(~valid, -math.inf)
    order = key.sort(dim=1, descending=True).indices
    ok = valid.gather(1, order)
    pos = ((labels > 0.5) & valid).gather(1, order).double()
    neg = ok.double() - pos
    tp, n = pos.cumsum(1), ok.double().cumsum(1)
    n_pos, n_neg = pos.sum(1), neg.sum(1)
    ap = (pos * tp / n.clamp(min=1)).sum(1) / n_pos.clamp(min=1)
    auc = (pos * (n_neg[:, None] - neg.cumsum(1))).sum(1) / (n_pos * n_neg).clamp(min=1)
    return ap, auc


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise SystemExit("tools/token_rank_bench.py measures on the GPU; there is none here")
    from case_rg_amd import ops
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

    res = {"what": "token ranking metrics: K45 (AP, AUC, best F1 cut) next to K38's counts and a torch restatement (sort + cumsum, f64)",
           "config": {"kernel_iters": a.kernel_iters, "repeats": a.repeats, "invalid": 0.1, "positive": 0.1},
           "device": torch.cuda.get_device_name(0), "points": []}
    g = torch.Generator().manual_seed(10)
    for B, S in zip(a.points[0::2], a.points[1::2]):
        for kind in ("bf16", "f32"):
            scores = torch.randn(B, S, generator=g)
            scores = (scores.bfloat16().float() if kind == "bf16" else scores).to(dev)
            valid = (torch.rand(B, S, generator=g) < 0.9).to(dev)
            gold = (torch.rand(B, S, generator=g) < 0.1).float().to(dev)
            us = timed({"k45": lambda: ops.token_rank(scores, valid, gold),
                        "k38_counts": lambda: ops.token_select(scores, valid, 32, labels=gold),
                        "torch_form": lambda: torch_form(scores, valid, gold)})
            got, (ap, auc) = ops.token_rank(scores, valid, gold), torch_form(scores, valid, gold)
            point = {"items": B, "positions": S, "scores": kind, "us_per_call": us,
                     "groups_per_item": round(float(got["counts"][:, 5].double().mean()), 1),
                     "torch_form_over_k45": round(us["torch_form"]["median"] / us["k45"]["median"], 2),
                     "k45_over_k38_counts": round(us["k45"]["median"] / us["k38_counts"]["median"], 2)}
            if kind == "f32":  # (the restatement has no tie rule)
                point["max_ap_diff_to_torch_form"] = float((got["stats"][:, 0] - ap).abs().max())
                point["max_auc_diff_to_torch_form"] = float((got["stats"][:, 1] - auc).abs().max())
            res["points"].append(point)
            print(json.dumps(point), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(res, fh, indent=1)
                fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
