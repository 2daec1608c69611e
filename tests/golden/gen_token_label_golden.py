"""Generate the token-supervision fixture from the reference's own CaSE/CaSEDataset.py ``token_label`` (build container only).

    python tests/golden/gen_token_label_golden.py            # writes tests/golden/token_label.npz

CaSEDataset.py opens with ``from common.Utils import *``; ``token_label`` itself needs only ``torch``, so the file is loaded by path with a
stub ``common.Utils`` module in ``sys.modules`` that carries ``torch`` and ``random`` and nothing else (the stub is removed again).  The
reference takes one item at a time: its passages [P, L], the answer WITHOUT padding [T'], a ``{id: count}`` dict.  Only data is written, per
case i: ``passage_i`` int64 [B, P, L], ``response_i`` int64 [B, T] (PAD-padded), ``freq_i`` int64 [F] (the dict as a table), ``label_i`` and
``weight_i`` f32 [B, P, L] (the reference's), and once ``ref_vs_f64``: the worst relative distance of the reference's f32 weights from the
f64 host form (``common.Utils.token_label_f64``) over all cases.  No-op when the reference is absent.

Cases (``names``): eight seeds of P 3, L 17, T 6 with ids from 12 words, so that windows hold repeated members; rows of L = 1, 2, 3, 5; an
item with an all-PAD row; an item whose answer ids never occur; one item at P 10, L 384, T 80 over 3000 words with counts up to 2 x 10^6."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden  # noqa: E402

FIRST = 4  # the first word id (0 = PAD; 1 .. 3 stand for the other specials and are ordinary ids here)


def load_reference():
    path = os.path.join(gen_golden.REF, "CaSE", "CaSEDataset.py")
    if not os.path.isfile(path):
        return None
    import random
    saved = {k: sys.modules.get(k) for k in ("common", "common.Utils")}
    pkg, stub = types.ModuleType("common"), types.ModuleType("common.Utils")
    stub.torch, stub.random = torch, random
    stub.__all__ = ["torch", "random"]
    pkg.Utils = stub
    sys.modules["common"], sys.modules["common.Utils"] = pkg, stub
    try:
        spec = importlib.util.spec_from_file_location("ref_case_dataset", path)
        ref = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ref)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return ref


def rows(rs, B, P, L, words, full=False):
    """Passages of ragged length (PAD behind), ids FIRST .. FIRST + words - 1."""
    x = np.zeros((B, P, L), dtype=np.int64)
    for b in range(B):
        for p in range(P):
            n = L if full else rs.randint(max(1, L // 2), L + 1)
            x[b, p, :n] = rs.randint(0, words, n) + FIRST
    return x


def answers(rs, B, T, words, full=False):
    y = np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        n = T if full else rs.randint(1, T + 1)
        y[b, :n] = rs.randint(0, words, n) + FIRST
    return y


def build_cases():
    rs = np.random.RandomState(370)
    table = lambda words, top: np.concatenate([rs.randint(0, top, FIRST), rs.randint(0, top, words)]).astype(np.int64)  # noqa: E731
    cases = {}
    for seed in range(8):
        cases["small_%d" % seed] = (rows(rs, 1, 3, 17, 12), answers(rs, 1, 6, 12), table(12, 50))
    for L in (1, 2, 3, 5):
        cases["row_%d" % L] = (rows(rs, 2, 2, L, 4, full=True), answers(rs, 2, 3, 4), table(4, 50))
    x = rows(rs, 1, 3, 9, 6)
    x[0, 1] = 0
    cases["all_pad_row"] = (x, answers(rs, 1, 4, 6), table(6, 50))
    cases["no_member"] = (rows(rs, 1, 3, 11, 6), answers(rs, 1, 4, 6) + 100, table(6, 50))
    freq = table(3000, 2 * 10 ** 6 + 1)
    freq[FIRST + 7], freq[FIRST + 8] = 0, 2 * 10 ** 6  # count 0 and the largest count occur
    cases["prod"] = (rows(rs, 1, 10, 384, 3000), answers(rs, 1, 80, 3000, full=True), freq)
    # half of the production answer is copied from the passages, so that members are common there too
    x, y, _ = cases["prod"]
    pool = x[x != 0]
    y[0, ::2] = pool[rs.randint(0, len(pool), len(y[0, ::2]))]
    return cases


def main():
    ref = load_reference()
    if ref is None:
        print("gen_token_label_golden: %s not present; fixtures are generated in the build container only" % gen_golden.REF)
        return 0
    sys.path.insert(0, gen_golden.ROOT)
    from case_rg_amd.common.Utils import token_label_f64
    out, worst, members = {}, 0.0, 0
    cases = build_cases()
    for i, (name, (x, y, freq)) in enumerate(cases.items()):
        table = {v: int(c) for v, c in enumerate(freq) if c or v % 2}  # (a zero count is both a missing entry and an entry of 0)
        label, weight = np.zeros(x.shape, np.float32), np.zeros(x.shape, np.float32)
        for b in range(x.shape[0]):
            answer = torch.from_numpy(y[b][y[b] != 0])
            got = ref.token_label(torch.from_numpy(x[b]), answer, None, table)
            label[b], weight[b] = got[0].numpy(), got[1].numpy()
        want_label, want = token_label_f64(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(freq))
        assert np.array_equal(label, want_label.numpy()), name
        worst = max(worst, float(np.abs(weight.astype(np.float64) / want.numpy() - 1.0).max()))
        members += int(label.sum())
        out.update({"passage_%d" % i: x, "response_%d" % i: y, "freq_%d" % i: freq, "label_%d" % i: label, "weight_%d" % i: weight})
        print("%-12s %-14s members %5d  max weight %.4f" % (name, x.shape, label.sum(), weight.max()))
    assert members > 200 and out["label_%d" % list(cases).index("no_member")].sum() == 0
    path = os.path.join(HERE, "token_label.npz")
    np.savez_compressed(path, names=np.array(list(cases)), ref_vs_f64=np.float64(worst), **out)
    print("%-32s %8.1f KB; reference vs f64 host form: %.3e" % (os.path.basename(path), os.path.getsize(path) / 1024, worst))
    return 0


if __name__ == "__main__":
    sys.exit(main())
