"""Sampled-decoding parity cases: the case table, the NumPy restatement of the counter RNG (csrc/common.h ``rng_hash`` / ``rng_uniform24``), a
float64 restatement of the draw rule (include/case_hip.h, ``case_pointer_head_sample``) and of the reference's ``sample`` loop conventions
(common/Generations.py:47-57).

The same restatement runs against

  * the reference            (tests/golden/gen_sample_golden.py: the adapter its own ``Generations.sample`` drives) -> tests/golden/sample_*.npz
  * the CPU oracle           (tests/test_sample_cpu.py)
  * the HIP product          (tests/test_sample_gpu.py: the kernel's interval property, the self-check on the product's own trajectories)

Every draw comes with its **margin**: the smallest relative distance that decided it -- u Z to the two CDF boundaries of the chosen token
(relative to Z), and the gaps that decided the top-k and top-p cuts.  An item is decisive while all its margins so far exceed ``GAP``.
"""
import numpy as np
import torch

from beam_cases import GAP, ITEMS, T  # noqa: F401  (the beam cases' batch geometry and id-exactness margin)
from beam_cases import build as _beam_build
from beam_cases import BEAM_CASES

INF = float("inf")
# name -> (model, model seed, batch seed, draw seed, (temperature, top_k, top_p)).  Models and batches are the beam cases' (their EOS is
# likely enough to end a row early); the draw seeds were searched on the CPU (gen_sample_golden.py --search) so that the reference alone
# satisfies the generator's assertions: at least half the items decisive through all T steps, one sampled answer that differs from the
# greedy one, one row that ends before the last step -- a row, decisive throughout, that DRAWS EOS at some t < T - 1 (a PAD in the answer
# is no sign of an end: PAD is an ordinary id that a live row may draw).
SAMPLE_CASES = {
    "sample_case": ("case", 214, 152, 21, (1.0, 0, 1.0)),
    "sample_masque": ("masque", 276, 172, 19, (1.0, 0, 1.0)),
    "sample_case_k5": ("case", 214, 152, 1, (1.0, 5, 1.0)),
    "sample_masque_t07_p09": ("masque", 276, 172, 7, (0.7, 0, 0.9)),
}
assert all(BEAM_CASES["beam_" + v[0]][:3] == v[:3] for v in SAMPLE_CASES.values())


def build(ns, dev, name):
    return _beam_build(ns, dev, "beam_" + SAMPLE_CASES[name][0])


# ---- the counter RNG ----------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def rng_hash(seed, counter):
    """csrc/common.h ``rng_hash`` on uint64 counters (scalar or array) -> uint64 array holding the 32-bit hash."""
    c = np.asarray(counter, dtype=np.uint64)
    seed = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    lo, hi = c & _M32, c >> np.uint64(32)
    h = lo ^ (((hi << np.uint64(16)) | (hi >> np.uint64(16))) & _M32) ^ (seed & _M32)
    h = (h * np.uint64(0x9E3779B1)) & _M32
    h = h ^ (h >> np.uint64(15)) ^ (seed >> np.uint64(32))
    h = (h * np.uint64(0x85EBCA77)) & _M32
    return h ^ (h >> np.uint64(13))


def rng_uniform24(seed, counter):
    """``rng_uniform24``: (hash >> 8) 2^-24, exact in float32 and in float64."""
    return (rng_hash(seed, counter) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


# ---- the draw rule ------------------------------------------------------------------------------
def rel_gap(a, b):
    """|a - b| relative to the larger magnitude; two zeros are no comparison at all (neither can be drawn), other equal values are a tie
    that the id order decides, not the arithmetic: 0."""
    if a == b:
        return INF if a == 0 else 0.0
    return abs(a - b) / max(abs(a), abs(b))


def draw(p, temperature, top_k, top_p, u):
    """One draw from the row ``p`` in float64 -> dict(id, prob = p[id], margin, q, kept (bool [V]), cdf ([V], the kept mass up to and
    including each id), Z, cut (the smallest kept q), next (the first id the cuts dropped, -1 if none), slack (how far the top-p target is
    from the nearer prefix mass around its cut, relative to the mass; inf without top-p))."""
    p = np.asarray(p, dtype=np.float64)
    V = p.size
    q = p.copy() if temperature == 1 else np.where(p > 0, np.power(np.maximum(p, 1e-300), 1.0 / temperature), 0.0)
    order = np.argsort(-q, kind="stable")  # q descending, the lower id first among equals
    margin, n, slack = INF, V, INF
    if top_k > 0 and top_k < V:
        n = top_k
        margin = min(margin, rel_gap(q[order[n - 1]], q[order[n]]))
    if top_p < 1:
        c = np.cumsum(q[order[:n]])
        target = top_p * c[-1]
        m = min(max(int(np.searchsorted(c, target, side="left")) + 1, 1), n)  # the shortest prefix whose mass is >= target
        slack = abs(c[m - 1] - target) / c[-1]
        if m > 1:
            slack = min(slack, abs(target - c[m - 2]) / c[-1])
        margin = min(margin, slack)
        if m < V:
            margin = min(margin, rel_gap(q[order[m - 1]], q[order[m]]))
        n = m
    kept = np.zeros(V, dtype=bool)
    kept[order[:n]] = True
    cdf = np.cumsum(np.where(kept, q, 0.0))
    Z = cdf[-1]
    thr = u * Z
    hit = np.nonzero(kept & (q > 0) & (cdf > thr))[0]
    j = int(hit[0]) if hit.size else int(np.nonzero(kept & (q > 0))[0][-1])
    margin = min(margin, (cdf[j] - thr) / Z)
    below = cdf[j] - q[j]
    if below > 0:  # (the lower boundary 0 of the first token with mass is exact: u Z >= 0 in every arithmetic)
        margin = min(margin, (thr - below) / Z)
    return dict(id=j, prob=float(p[j]), margin=float(margin), q=q, kept=kept, cdf=cdf, Z=float(Z), cut=float(q[order[n - 1]]),
                next=int(order[n]) if n < V else -1, slack=float(slack))


def emit(x, ended, t, T, eos, unk, pad):
    """The loop conventions for one row: the drawn id ``x`` and e = "ended before this step" -> (emitted id, ended after this step)."""
    this_end = x == eos
    if t == 0:
        out = unk if this_end else x
    elif t == T - 1:
        out = pad if ended else eos
    else:
        out = pad if ended else x
    return out, bool(ended or this_end)


def sample_loop(step_fn, items, T, bos, eos, unk, pad, params, uniforms):
    """The whole sampled pass.  step_fn(rows, prefixes int64 [n, L]) -> distributions [n, V]; uniforms [items, T].
    -> dict(answer int64 [items, T], prob f64 [items, T] (1 behind the end), margin f64 [items, T] (inf behind the end))."""
    tau, k, pp = params
    prefix = [[bos] for _ in range(items)]
    ended = [False] * items
    answer = np.zeros((items, T), dtype=np.int64)
    prob = np.ones((items, T))
    margin = np.full((items, T), INF)
    for t in range(T):
        dists = step_fn(list(range(items)), torch.tensor(prefix, dtype=torch.long)).detach().double().cpu().numpy()
        for i in range(items):
            d = draw(dists[i], tau, k, pp, float(uniforms[i, t]))
            if not ended[i]:
                prob[i, t], margin[i, t] = d["prob"], d["margin"]
            answer[i, t], ended[i] = emit(d["id"], ended[i], t, T, eos, unk, pad)
            prefix[i].append(int(answer[i, t]))
    return dict(answer=answer, prob=prob, margin=margin)


def decisive_steps(margin):
    """[items] the number of leading steps of each item whose margins all exceed GAP (T for an item that is decisive throughout)."""
    ok = np.asarray(margin) > GAP
    return np.where(ok.all(axis=1), ok.shape[1], np.argmin(ok, axis=1))


def case_uniforms(seed, items=ITEMS, steps=T):
    """u of row ``row`` at step ``t`` = rng_uniform24(seed, t * items + row): the private stream of ``do_sample(seed=...)`` -> [items, steps]."""
    return rng_uniform24(seed, np.arange(steps * items, dtype=np.uint64)).reshape(steps, items).T.copy()
