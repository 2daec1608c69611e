#!/usr/bin/env python
"""Minimum-risk training: the differentiable score head (K29 with row statistics + K41) next to the unfused chain, the risk kernel
(K42), and a whole ``do_mrt`` step next to ``do_train``.

    python tools/mrt_bench.py [--out profiles/mrt_bench.json]

Head ("head" in the json): --rows x V 30 522 (2048 rows = one default head chunk), S = 64 + 3840 source positions, one source row per
--rows-per-source rows.  Forward AND backward of sum(prob x g) down to the gradients of the logits, the mixing logits and the copy
weights, two variants on the same operands, ALTERNATING inside a round, device events around --iters passes:
  K29+K41  ops.pointer_head_score_grad: the forward reads the logits once and keeps them with two floats per row; the backward reads them
           once more and writes d_logits;
  chain    the launches the unfused differentiable path runs: masked_softmax over the logits, p0 x gen, the sorted scatter, the gather,
           and autograd's backward through them (the dense scatter's gradient included).
Every pass reads a different logits buffer of a ring.  K42 ("risk"): ops.sequence_risk forward + backward at two pool shapes.
Step ("step"): CaSE in bf16, forward + backward of ``do_train`` (dropout on) and of ``do_mrt`` with the fused head and with the unfused
chain (CASE_POINTER_SCORE=off), device events around each step, alternating, and torch's peak allocation of each.  Seven rounds
everywhere: medians with min - max.  These are records, not bars.  Stand-alone: bench.py does not call this.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--rows-per-source", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--answer-len", type=int, default=40)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--enc-layers", type=int, default=3)
    ap.add_argument("--passages", type=int, default=10)
    ap.add_argument("--passage-len", type=int, default=384)
    ap.add_argument("--query-len", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ring", type=int, default=3, help="logits buffers the passes rotate over")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mrt_bench.json"))
    return ap.parse_args()


def summary(v, scale=1.0, digits=1):
    return {"median": round(statistics.median(v) * scale, digits), "min": round(min(v) * scale, digits), "max": round(max(v) * scale, digits)}


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mrt_bench.py measures on the GPU; there is none here")
    import case_rg_amd
    from case_rg_amd import ops
    dev = torch.device("cuda")

    def events(variants, rounds, iters):
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        samples = {n: [] for n in variants}
        for _ in range(rounds):
            for n, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                samples[n].append(e0.elapsed_time(e1) * 1e3 / iters)
        return {n: summary(v) for n, v in samples.items()}

    def head():
        R, V, rps = a.rows, a.vocab, a.rows_per_source
        lens = [a.query_len, a.passages * a.passage_len]
        S = sum(lens)
        g = torch.Generator(device="cuda").manual_seed(3)
        ring = [(torch.randn(R, V, device=dev, generator=g) * 2.0).requires_grad_(True) for _ in range(a.ring)]
        mix = torch.randn(R, 1 + len(lens), device=dev, generator=g).requires_grad_(True)
        src = ops.SortedSource(torch.randint(4, V, (R // rps, S), device=dev, generator=g), V)
        rows = src.select(torch.arange(R, device=dev) // rps)  # the chain scatters per row: its item's keys beside every row
        copies = [torch.softmax(torch.randn(R, n, device=dev, generator=g) * 2.0, dim=-1).requires_grad_(True) for n in lens]
        targets = torch.randint(4, V, (R,), device=dev, generator=g)
        targets[::2] = src.ids[torch.arange(0, R, 2, device=dev) // rps, 7]  # half the targets occur in their source
        upstream = torch.randn(R, device=dev, generator=g)
        turn = [0]

        def fused():
            turn[0] += 1
            logits = ring[turn[0] % a.ring]
            p, _ = ops.pointer_head_score_grad(logits, mix, src, rps, copies, targets, pad=0)
            return p.detach(), torch.autograd.grad((p * upstream).sum(), [logits, mix] + copies)

        def chain():
            turn[0] += 1
            logits = ring[turn[0] % a.ring]
            gen = ops.masked_softmax(logits.view(R, 1, V))
            pm = ops.masked_softmax(mix.view(R, 1, -1))
            d1 = pm[:, :, 0:1] * gen
            ptr = torch.cat([pm[:, :, k + 1:k + 2] * c.unsqueeze(1) for k, c in enumerate(copies)], dim=-1)
            d2 = ops.copy_scatter(rows, ptr, V)
            at = targets.reshape(R, 1, 1)
            p = d1.gather(-1, at).reshape(R) + d2.gather(-1, at).reshape(R)
            return p.detach(), torch.autograd.grad((p * upstream).sum(), [logits, mix] + copies)

        turn[0] = 0
        pf, gf = fused()
        turn[0] = 0
        pc, gc = chain()
        gap = {"prob": float((pf - pc).abs().max() / pc.abs().max())}
        for name, x, y in zip(["d_logits", "d_mix", "d_copy_0", "d_copy_1"], gf, gc):
            gap[name] = float("%.3e" % float((x - y).abs().max() / y.abs().max()))
        del pf, gf, pc, gc
        peak = {}
        for n, fn in (("K29+K41", fused), ("chain", chain)):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            peak[n] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        us = events({"K29+K41": fused, "chain": chain}, a.rounds, a.iters)
        return {"rows": R, "vocab": V, "source_positions": S, "rows_per_source": rps, "iters": a.iters, "rounds": a.rounds, "ring": a.ring,
                "max_rel_gap_fused_vs_chain": gap, "peak_extra_MB_one_pass": peak, "us_per_forward_backward": us,
                "chain_over_fused": round(us["chain"]["median"] / us["K29+K41"]["median"], 2)}

    def risk():
        out = []
        for B, N, T in ((32, 9, 64), (130, 64, 1024)):
            g = torch.Generator(device="cuda").manual_seed(B)
            p = (torch.rand(B, N, T, device=dev, generator=g) * 0.9 + 0.05).requires_grad_(True)
            scored = torch.rand(B, N, T, device=dev, generator=g) < 0.8
            cost = torch.rand(B, N, device=dev, generator=g)

            def k42():
                return torch.autograd.grad(ops.sequence_risk(p, scored, cost, None, 5e-3).mean(), p)

            out.append({"B": B, "N": N, "T": T, "us_per_forward_backward": events({"K42": k42}, a.rounds, 20)["K42"]})
        return out

    def step():
        from case_rg_amd.CaSE.Model import CaSE
        from case_rg_amd.common.CumulativeTrainer import init_params
        from case_rg_amd.common.Utils import init_seed
        from case_rg_amd.utils import make_vocab, synth_batch
        case_rg_amd.set_compute_dtype(torch.bfloat16)
        case_rg_amd.set_dropout(True)
        init_seed(123456)
        v2i, i2v = make_vocab(a.vocab)
        T = a.answer_len
        model = CaSE(4, T, i2v, v2i, a.hidden, enc_layers=a.enc_layers)
        init_params(model)
        model = model.to(dev).train()
        batch = synth_batch(a.batch, a.passages, a.passage_len, a.query_len, T, a.vocab, seed=123456, ragged=False)
        batch = {k: v.to(dev) for k, v in batch.items()}

        def run(method, mode="auto"):
            def fn():
                old, ops.POINTER_SCORE = ops.POINTER_SCORE, mode
                try:
                    losses = model.do_train(dict(batch)) if method == "train" else model.do_mrt(dict(batch), num_samples=a.samples)
                    sum(l.mean() for l in losses).backward()
                finally:
                    ops.POINTER_SCORE = old
                model.zero_grad(set_to_none=True)
            return fn

        runs = {"do_train": run("train"), "do_mrt_fused": run("mrt"), "do_mrt_unfused": run("mrt", "off")}
        times, peak = {n: [] for n in runs}, {}
        for n, fn in runs.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peak[n] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
        for _ in range(a.rounds):
            for n, fn in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[n].append(e0.elapsed_time(e1) * 1e-3)
        rows = a.batch * (a.samples + 1) * T
        return {"ms_per_step_forward_backward": {n: summary(v, 1e3, 2) for n, v in times.items()}, "max_memory_allocated_MB": peak,
                "scored_rows": rows, "score_chunk_rows": model.response_generation.decoder.score_chunk_rows, "rounds": a.rounds}

    res = {"what": "minimum-risk training: K29 + K41 vs the unfused differentiable chain; K42; do_mrt vs do_train, CaSE, bf16, eager",
           "config": {"batch": a.batch, "samples": a.samples, "answer_len": a.answer_len, "hidden": a.hidden, "enc_layers": a.enc_layers,
                      "passages": a.passages, "passage_len": a.passage_len, "query_len": a.query_len, "vocab": a.vocab, "warmup": a.warmup},
           "device": torch.cuda.get_device_name(0), "head": head()}
    print(json.dumps(res["head"]), flush=True)
    res["risk"] = risk()
    print(json.dumps(res["risk"]), flush=True)
    if not a.skip_step:
        res["step"] = step()
        print(json.dumps(res["step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
