#!/usr/bin/env python
"""The wide (global-row) forms of K23 / K24 / K28 next to what they stand beside: the LDS forms where both run, the unfused chain beyond
36 000 ids, and the LDS forms of this build next to another build's.

    python tools/wide_head_bench.py [--parent-lib other/libcase_hip.so] [--out profiles/wide_head_bench.json]

256 rows, S = 64 + 3840 source keys, no gen / dist write-back (what a decoding step asks for).  Every group of variants is timed with device
events around --kernel-iters back-to-back calls, --repeats times, the variants ALTERNATING inside a repeat; reported are the median and the
spread (min, max) in us per call.  The windows hold the wrappers' host work too (the wide wrappers allocate their row workspace inside), so
they bound a kernel's time from above.

(a) "wide_vs_lds": V = 30 522, ``row="global"`` against ``row="lds"``: K23, K24 at W = 4, K28 with the filters off and with temperature 0.7 +
    top-k 50 + top-p 0.9.
(b) "wide_vs_unfused": V = 50 265 and 119 547, the wide forms against the chain the decoder ran there before: masked softmax of the logits
    and of the mixing logits, p0 x gen, the sorted pointer scatter, the sum, then ``row_argmax`` (greedy), ``torch.topk`` (beam) or K28 on
    the finished distribution (``dist_in``, the wide form: sampling had no other path beyond 36 000 ids).
(c) "ab_lds": with --parent-lib, the LDS entry points of that build (A) and of this one (B) by raw C-ABI calls on the same operands,
    alternating: what the shared row code costs the default path.
Stand-alone: bench.py does not call this.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--passages", type=int, default=10)
    ap.add_argument("--passage-len", type=int, default=384)
    ap.add_argument("--query-len", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--wide-vocabs", type=int, nargs="+", default=[50265, 119547])
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parent-lib", default=None, help="another build of libcase_hip.so (the parent commit's): A/B of the LDS launches")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_head_bench.json"))
    return ap.parse_args()


def _stats(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def _time(variants, iters, repeats):
    for fn in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    samples = {n: [] for n in variants}
    for _ in range(repeats):
        for n, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            samples[n].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {n: _stats(v) for n, v in samples.items()}


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise SystemExit("tools/wide_head_bench.py measures on the GPU; there is none here")
    from case_rg_amd import _abi, ops
    dev = torch.device("cuda")
    R, W = a.rows, 4
    lens = [a.query_len, a.passages * a.passage_len]

    def operands(V):
        g = torch.Generator(device="cuda").manual_seed(3)
        logits = torch.randn(R, V, device=dev, generator=g) * 2.0
        mix = torch.randn(R, 1 + len(lens), device=dev, generator=g)
        src = ops.SortedSource(torch.randint(4, V, (R, sum(lens)), device=dev, generator=g), V)
        copies = [torch.softmax(torch.randn(R, n, device=dev, generator=g) * 2.0, dim=-1) for n in lens]
        return logits, mix, src, copies

    ended = torch.zeros(R, dtype=torch.uint8, device=dev)

    def heads(V, head, row):
        def k28(tau, k, p):
            return lambda: ops.pointer_head_sample(*head, ended, False, False, -1, -1, 0, tau, k, p, rng=(1, 0, None), row=row)
        return {"K23": lambda: ops.pointer_head_decode(*head, want_gen=False, want_dist=False, row=row),
                "K24_w4": lambda: ops.pointer_head_topk(*head, W, row=row),
                "K28_filters_off": k28(1.0, 0, 1.0), "K28_t07_k50_p09": k28(0.7, 50, 0.9)}

    res = {"what": "wide (global-row) pointer-generator heads; eager calls, device events, us per call", "device": torch.cuda.get_device_name(0),
           "rows": R, "source_keys": sum(lens), "iters": a.kernel_iters, "repeats": a.repeats}

    # (a) wide against LDS
    V = a.vocab
    head = operands(V)
    variants = {}
    for name in ("K23", "K24_w4", "K28_filters_off", "K28_t07_k50_p09"):
        variants[name + "/lds"] = heads(V, head, "lds")[name]
        variants[name + "/global"] = heads(V, head, "global")[name]
    timed = _time(variants, a.kernel_iters, a.repeats)
    res["wide_vs_lds"] = {"vocab": V, "us_per_call": timed,
                          "global_over_lds": {n: round(timed[n + "/global"]["median"] / timed[n + "/lds"]["median"], 3)
                                              for n in ("K23", "K24_w4", "K28_filters_off", "K28_t07_k50_p09")}}
    print(json.dumps(res["wide_vs_lds"]))

    # (c) the LDS forms of two builds (before (b): the same operands)
    if a.parent_lib:
        other = C.CDLL(os.path.abspath(a.parent_lib))
        names = ("case_pointer_head_decode", "case_pointer_head_beam", "case_pointer_head_sample")
        for lib in (other, _abi.lib):
            for name in names:
                getattr(lib, name).argtypes, getattr(lib, name).restype = _abi.SIGNATURES[name], C.c_int
        lg, mx, cs, ptrs, ln, nm, S = ops._head_operands(*head)
        ids = torch.empty(R, dtype=torch.int64, device=dev)
        prob = torch.empty(R, dtype=torch.float32, device=dev)
        cp, ci = torch.empty(R, W, device=dev), torch.empty(R, W, dtype=torch.int64, device=dev)
        p, stream = ops._ptr, ops._stream
        hd = (p(lg), p(mx), p(head[2].keys), ptrs, ln, nm)

        def raw(lib):
            def k28(tau, k, pp):
                return lambda: lib.case_pointer_head_sample(*hd, None, None, None, p(ids), p(prob), p(ended), None, R, V, S, tau, k, pp, 1, 0, None,
                                                            -1, -1, 0, 0, 0, stream())
            return {"K23": lambda: lib.case_pointer_head_decode(*hd, None, None, p(ids), None, R, V, S, stream()),
                    "K24_w4": lambda: lib.case_pointer_head_beam(*hd, None, None, p(cp), p(ci), R, V, S, W, stream()),
                    "K28_filters_off": k28(1.0, 0, 1.0), "K28_t07_k50_p09": k28(0.7, 50, 0.9)}
        keys = ("K23", "K24_w4", "K28_filters_off", "K28_t07_k50_p09")
        ab = {}
        for k in keys:
            ab["A_parent/" + k] = raw(other)[k]
            ab["B_this/" + k] = raw(_abi.lib)[k]
        for fn in ab.values():
            assert fn() == 0
        timed = _time(ab, a.kernel_iters, a.repeats)
        res["ab_lds"] = {"what": "the LDS launches through the parent build (A) and this build (B), raw C-ABI calls on the same operands, alternating",
                         "vocab": V, "parent_lib": os.path.basename(a.parent_lib), "us_per_call": timed,
                         "B_minus_A_us": {k: round(timed["B_this/" + k]["median"] - timed["A_parent/" + k]["median"], 2) for k in keys},
                         "medians_inside_each_others_range": {
                             k: bool(timed["A_parent/" + k]["min"] <= timed["B_this/" + k]["median"] <= timed["A_parent/" + k]["max"]
                                     and timed["B_this/" + k]["min"] <= timed["A_parent/" + k]["median"] <= timed["B_this/" + k]["max"]) for k in keys}}
        print(json.dumps(res["ab_lds"]))
    del head, variants

    # (b) wide against the unfused chain
    res["wide_vs_unfused"] = []
    for V in a.wide_vocabs:
        head = operands(V)
        logits, mix, src, copies = head

        def chain():
            gen = ops.masked_softmax(logits.view(R, 1, V))
            pm = ops.masked_softmax(mix.view(R, 1, -1))
            ptr = torch.cat([pm[:, :, k + 1:k + 2] * c.view(R, 1, -1) for k, c in enumerate(copies)], dim=-1)
            return ops.add(pm[:, :, 0:1] * gen, ops.copy_scatter(src, ptr, V))

        def draw_unfused(tau, k, p):
            return lambda: ops.pointer_head_sample(None, None, None, None, ended, False, False, -1, -1, 0, tau, k, p, rng=(1, 0, None),
                                                   dist_in=chain()[:, -1].detach().float())

        wide = heads(V, head, "global")
        variants = {"greedy/wide_K23": wide["K23"], "greedy/unfused_chain_row_argmax": lambda: ops.row_argmax(chain()[:, -1]),
                    "beam_w4/wide_K24": wide["K24_w4"], "beam_w4/unfused_chain_topk": lambda: torch.topk(chain()[:, -1].detach().float(), W, dim=-1),
                    "sample_filters_off/wide_K28": wide["K28_filters_off"], "sample_filters_off/unfused_chain_K28_dist_in": draw_unfused(1.0, 0, 1.0),
                    "sample_t07_k50_p09/wide_K28": wide["K28_t07_k50_p09"], "sample_t07_k50_p09/unfused_chain_K28_dist_in": draw_unfused(0.7, 50, 0.9)}
        timed = _time(variants, a.kernel_iters, a.repeats)
        point = {"vocab": V, "us_per_call": timed,
                 "unfused_over_wide": {m: round(timed[m + "/" + u]["median"] / timed[m + "/" + w]["median"], 3)
                                       for m, w, u in (("greedy", "wide_K23", "unfused_chain_row_argmax"), ("beam_w4", "wide_K24", "unfused_chain_topk"),
                                                       ("sample_filters_off", "wide_K28", "unfused_chain_K28_dist_in"),
                                                       ("sample_t07_k50_p09", "wide_K28", "unfused_chain_K28_dist_in"))}}
        print(json.dumps(point))
        res["wide_vs_unfused"].append(point)
        del head, logits, mix, src, copies, variants, wide

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
