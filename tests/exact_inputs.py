"""Operands for which the MFMA GEMM and the attention kernels have no rounding to hide behind: every product and every partial sum is
exactly representable in f32, so the result does not depend on the summation order, the tiling, the split or the use of f32 atomics, and a
kernel must equal the float64 restatement in every bit (after ONE round-to-nearest-even where the output is bf16).

Plain torch, no GPU: everything is built on the CPU in float64 (the values are small integers or powers of two, exact in bf16 and f32) and the
callers move it where they need it.  tests/test_exact_inputs_cpu.py pins every claim made here for the seeds the GPU tests use.

GEMM       integers in [-15, 15], an eighth of them 0: |product| <= 225, and K * 225 < 2^24 for every K used.
attention  the first C <= min(d, 8) head dimensions carry a class code: key j of class c has 2^10 at dimension c, query i of class c has
           -2^10 at every code dimension but c.  A score is 0 inside the class and -2^20 outside (exp of it, times any 1/sqrt(d), is 0 in
           f32), so the probabilities are exactly 1/n on the n valid keys of the class.  Class sizes are the powers of two of the binary
           decomposition of the valid length, scattered over the positions by a seeded permutation per (item, head).  V is integers in
           [-127, 127]; O is the exact class mean.
K8         the same class code carried over to the co-attention's rank-1 score (see "K8" below): every entry of A and Bm^T is 1/n or 0,
           and the kernels' bf16 roundings are restated at the points where they round (interaction_restated).
K16        the encoder chain's parameters written so that each stage stands alone (see "K16" below): integers, signed permutations, zeros.
K7 / K22   the additive attention (see "K7 / K22" below): a ternary family whose tanh is 0 or +-1, a mid-range family with the float64
           restatement AND its derived error bound per arithmetic form, the launch rules restated (k7_paths); pinned by
           tests/test_additive_exact_cpu.py."""
import torch

F64 = torch.float64
GEMM_BOUND = 15
CODE = 1024.0  # 2^10
V_BOUND = 127
DO_BOUND = 3


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, seed, bound=GEMM_BOUND, zero_share=0.125):
    """float64 integers in [-bound, bound]; ``zero_share`` of them forced to 0."""
    g = _gen(seed)
    x = torch.randint(-bound, bound + 1, tuple(shape), generator=g)
    z = torch.rand(tuple(shape), generator=g) < zero_share
    return torch.where(z, torch.zeros_like(x), x).to(F64)


def signs(shape, seed):
    """Integers in [-15, 15] with a third each positive, zero and negative (the operand of MUL_DRELU)."""
    g = _gen(seed)
    s = torch.randint(-1, 2, tuple(shape), generator=g)
    return (s * torch.randint(1, GEMM_BOUND + 1, tuple(shape), generator=g)).to(F64)


# ---------------------------------------------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------------------------------------------
LAYOUTS = {"nt": (False, False), "nn": (False, True), "tn": (True, True), "tt": (True, False)}  # name -> (a_kmajor, b_kmajor)


def gemm_exact_k(K):
    return K * GEMM_BOUND * GEMM_BOUND < 2 ** 24


def gemm_operands(layout, M, N, K, seed):
    """(a, b) as stored: A is [M, K] (or [K, M] k-major), B is [N, K] (or [K, N] k-major)."""
    assert gemm_exact_k(K)
    ak, bk = LAYOUTS[layout]
    return ints((K, M) if ak else (M, K), 2 * seed + 1), ints((K, N) if bk else (N, K), 2 * seed + 2)


def gemm_product(layout, a, b):
    """op(A) op(B) of the stored operands, in the dtype they come in."""
    ak, bk = LAYOUTS[layout]
    return (a.t() if ak else a) @ (b if bk else b.t())


def epilogue(acc, alpha=1.0, bias_col=None, bias_row=None, relu=False, drelu_aux=None, keep=None, residual=None):
    """The documented order: alpha * acc + bias -> RELU -> MUL_DRELU -> DROPOUT (p = 0.5: scale 2) -> + RESIDUAL.  Returns (result,
    the value in front of the activation)."""
    v = alpha * acc
    if bias_col is not None:
        v = v + bias_col[None, :]
    if bias_row is not None:
        v = v + bias_row[:, None]
    pre = v
    if relu:
        v = v.clamp_min(0.0)
    if drelu_aux is not None:
        v = torch.where(drelu_aux > 0, v, torch.zeros_like(v))
    if keep is not None:
        v = 2.0 * keep.to(v.dtype) * v
    if residual is not None:
        v = v + residual
    return v, pre


def round_bf16(ref):
    """The ONE rounding a bf16 output is allowed: float64 -> f32 (exact for everything built here) -> bf16, to nearest even."""
    f = ref.to(torch.float32)
    assert torch.equal(f.to(F64), ref), "the reference is not exact in f32"
    return f.to(torch.bfloat16)


def bf16_inexact_and_ties(ref):
    """(share of the elements that are not representable in bf16, number of exact ties between two bf16 neighbours)."""
    low = ref.to(torch.float32).contiguous().view(torch.int32) & 0xFFFF
    return (low != 0).double().mean().item(), int((low == 0x8000).sum())


def shuffled_f32_gemm(layout, a, b, order_seed, splits):
    """The same product accumulated in f32 with the K index permuted and cut into ``splits`` partial sums that are added one after
    another (what split-K with atomics does, in one of its orders)."""
    ak, bk = LAYOUTS[layout]
    A, B = (a.t() if ak else a).float(), (b if bk else b.t()).float()
    K = A.shape[1]
    perm = torch.randperm(K, generator=_gen(order_seed))
    out = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float32)
    for idx in perm.chunk(max(1, min(splits, K))):
        out = out + A[:, idx] @ B[idx, :]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------------
def pow2_parts(n):
    """Binary decomposition, largest first: 292 -> [256, 32, 4]."""
    return [1 << b for b in range(n.bit_length() - 1, -1, -1) if n >> b & 1]


def cut_length(Lk):
    """A valid length strictly inside the memory that ends in the middle of every tile (odd), with at most four powers of two."""
    if Lk < 16:
        return max(1, Lk // 2)
    cut = Lk * 5 // 8
    while bin(cut).count("1") > 2:
        cut &= cut - 1
    return cut | 5


def ragged_lengths(Lk, N=4):
    """One item full, one cut mid-tile, one with a single valid key, one with none; further items repeat the pattern."""
    base = [Lk, cut_length(Lk), 1, 0]
    return [base[i % 4] for i in range(N)]


class AttnCase(object):
    """q [N, Lq, h d], k / v [N, Lk, h d] float64, key_valid [N, Lk] bool, key_class [N, h, Lk] (-1: not a valid key), query_class
    [N, h, Lq] (-1: no visible key: a row of zeros), marked [N, h, Lq] (causal rows whose visible count is no power of two)."""

    def probabilities(self, device="cpu"):
        """P [N, h, Lq, Lk] float64: exactly 1 / n on the n valid, visible keys of the query's class (not exact on marked rows)."""
        kc, qc = self.key_class.to(device), self.query_class.to(device)
        match = (kc[:, :, None, :] == qc[:, :, :, None]) & (qc[:, :, :, None] >= 0)
        if self.causal:
            Lq, Lk = qc.shape[2], kc.shape[2]
            match &= torch.ones(Lq, Lk, dtype=torch.bool, device=device).tril()
        n = match.sum(-1, keepdim=True)
        return match.to(F64) / n.clamp_min(1).to(F64)

    def heads(self, t):
        """[N, L, h d] -> [N, h, L, d]"""
        N, L, _ = t.shape
        return t.reshape(N, L, self.h, self.d).transpose(1, 2)

    def merge(self, t):
        """[N, h, L, d] -> [N, L, h d]"""
        N, h, L, d = t.shape
        return t.transpose(1, 2).reshape(N, L, h * d)

    def output(self, device="cpu"):
        """O [N, Lq, h d] float64 = P V (every sum is an integer over a power of two: exact in float64 and in f32)."""
        return self.merge(self.probabilities(device) @ self.heads(self.v.to(device)))

    def backward(self, dO, scale, o_read=None, device="cpu"):
        """(dQ, dK, dV, |dS| |K| row sums) in float64 for the gradient dO [N, Lq, h d].  ``o_read``: the output the kernel reads for
        delta = rowsum(dO * O) (the fused kernels read their own bf16 result); None = rowsum(P * dP), the softmax backward's form."""
        P = self.probabilities(device)
        qh, kh, vh, gh = [self.heads(t.to(device).to(F64)) for t in (self.q, self.k, self.v, dO)]
        dV = P.transpose(-1, -2) @ gh
        dP = gh @ vh.transpose(-1, -2)
        delta = (P * dP).sum(-1, keepdim=True) if o_read is None else (gh * self.heads(o_read.to(device).to(F64))).sum(-1, keepdim=True)
        dS = P * (dP - delta)
        dQ, dK = scale * (dS @ kh), scale * (dS.transpose(-1, -2) @ qh)
        bound_q = scale * (dS.abs() @ kh.abs())
        return self.merge(dQ), self.merge(dK), self.merge(dV), self.merge(bound_q)


def _ranks(valid_h, g):
    """valid_h [N, h, L] -> rank of every valid position in a seeded permutation of the valid positions of its (item, head)."""
    r = torch.rand(valid_h.shape, generator=g, dtype=F64)
    r = torch.where(valid_h, r, r + 2.0)
    return r.argsort(-1).argsort(-1)


def attention_case(N, h, Lq, Lk, d, seed, lengths=None, causal=False, mode="classes", max_classes=8, v_bound=V_BOUND):
    """``mode``: "classes" (the general case), "class_const" (backward case A: V constant within every class), "uniform" (backward
    case B: Q = 0 and a power-of-two number of valid keys scattered inside the valid prefix: the uniform softmax)."""
    g = _gen(seed)
    lengths = list(ragged_lengths(Lk, N) if lengths is None else lengths)
    assert len(lengths) == N and all(0 <= n <= Lk for n in lengths) and (not causal or Lq == Lk)
    cmax = min(d, max_classes, 8)
    pos = torch.arange(Lk)
    valid = pos[None, :] < torch.tensor(lengths)[:, None]                                   # [N, Lk]
    if mode == "uniform":  # keep the largest power of two of the prefix, scattered
        keep = torch.tensor([0 if n == 0 else 1 << (n.bit_length() - 1) for n in lengths])
        valid = valid & (_ranks(valid[:, None, :], g)[:, 0, :] < keep[:, None])
        counts = keep.tolist()
    else:
        counts = lengths
    valid_h = valid[:, None, :].expand(N, h, Lk)
    rank = _ranks(valid_h, g)
    parts = [[] if mode == "uniform" and n else pow2_parts(n) for n in counts]
    parts = [p if p else ([n] if n else []) for p, n in zip(parts, counts)]
    assert all(len(p) <= cmax for p in parts), "valid lengths %s need more than %d classes" % (counts, cmax)
    ncls = torch.tensor([max(1, len(p)) for p in parts])                                    # [N]
    bounds = torch.full((N, 8), 1 << 40, dtype=torch.int64)
    for n, p in enumerate(parts):
        if p:
            bounds[n, :len(p)] = torch.tensor(p).cumsum(0)
    key_class = (rank[..., None] >= bounds[:, None, None, :]).sum(-1)                       # [N, h, Lk]: class by rank for the valid keys
    noise = torch.randint(0, 1 << 30, (N, h, Lk), generator=g) % ncls[:, None, None]        # masked keys carry a code as well: the mask must count
    key_code = torch.where(valid_h, key_class, noise)
    key_class = torch.where(valid_h, key_class, torch.full_like(key_class, -1))
    if mode == "uniform":  # the codes in K are free (Q = 0): spread them, dQ = scale dS K then sees every code dimension
        key_code = torch.randint(0, cmax, (N, h, Lk), generator=g)
    marked = torch.zeros(N, h, Lq, dtype=torch.bool)
    if causal:
        onehot = key_class[..., None] == torch.arange(8)                                    # [N, h, L, 8]
        cnt = onehot.cumsum(2)                                                              # visible valid keys of each class for query i
        pow2 = (cnt > 0) & ((cnt & (cnt - 1)) == 0)
        pick = torch.rand(N, h, Lq, 8, generator=g, dtype=F64) + 1.0
        best2, best1 = (pick * pow2).max(-1), (pick * (cnt > 0)).max(-1)
        query_class = torch.where(best2.values > 0, best2.indices, best1.indices)
        marked = (best2.values == 0) & (best1.values > 0)
        query_class = torch.where(best1.values > 0, query_class, torch.full_like(query_class, -1))
    else:
        query_class = torch.randint(0, 1 << 30, (N, h, Lq), generator=g) % ncls[:, None, None]
        query_class = torch.where(torch.tensor(counts)[:, None, None] > 0, query_class, torch.full_like(query_class, -1))
    dims = torch.arange(d)
    k = torch.where(key_code[..., None] == dims, CODE, 0.0).to(F64)                        # [N, h, Lk, d]
    if mode == "uniform":
        q = torch.zeros(N, h, Lq, d, dtype=F64)
        query_class = torch.where(query_class >= 0, torch.zeros_like(query_class), query_class)
    else:
        coded = (dims < ncls[:, None, None, None]) & (dims != query_class[..., None]) & (query_class[..., None] >= 0)
        q = torch.where(coded, -CODE, 0.0).to(F64)                                          # [N, h, Lq, d]
    v = ints((N, h, Lk, d), seed + 7919, bound=v_bound, zero_share=0.0)
    if mode == "class_const":
        table = ints((N, h, 8, d), seed + 104729, bound=v_bound, zero_share=0.0)
        v = torch.gather(table, 2, key_code[..., None].expand(N, h, Lk, d))
    c = AttnCase()
    c.N, c.h, c.Lq, c.Lk, c.d, c.causal, c.mode, c.lengths = N, h, Lq, Lk, d, causal, mode, lengths
    c.q, c.k, c.v = c.merge(q), c.merge(k), c.merge(v)
    c.key_valid, c.key_class, c.query_class, c.marked = valid, key_class, query_class, marked
    return c


def grad_output(case, seed):
    """dO [N, Lq, h d]: integers in [-3, 3]; zero on the marked rows of a causal case.  A marked row's probabilities are not exact, but
    with dO = 0 it adds exactly nothing to dV = P^T dO and its dS = P (dP - delta) is exactly 0, so dV is again integers over powers of two
    -- and still sees every key of every unmarked row: a kernel that let a query look past the diagonal gets another P, another dV."""
    g = ints((case.N, case.Lq, case.h * case.d), seed, bound=DO_BOUND, zero_share=0.0)
    return g * case.merge((~case.marked)[..., None].expand(case.N, case.h, case.Lq, case.d).to(F64))


def scores(case):
    """S [N, h, Lq, Lk] float64 = Q K^T without the 1/sqrt(d): exactly 0 inside the class, -2^20 times a positive integer outside."""
    return case.heads(case.q) @ case.heads(case.k).transpose(-1, -2)


def softmax_f32(case, scale, order_seed):
    """The probabilities as a kernel gets them, in f32 and with the keys visited in a shuffled order: online softmax over chunks."""
    s = (scores(case).float() * torch.tensor(scale, dtype=torch.float32))
    allowed = case.key_valid[:, None, None, :].expand_as(s).clone()
    if case.causal:
        allowed &= torch.ones(case.Lq, case.Lk, dtype=torch.bool).tril()
    s = torch.where(allowed, s, torch.full_like(s, float("-inf")))
    perm = torch.randperm(case.Lk, generator=_gen(order_seed))
    m = torch.full(s.shape[:-1], float("-inf"))
    l = torch.zeros(s.shape[:-1])
    for idx in perm.chunk(max(1, min(5, case.Lk))):
        blk = s[..., idx]
        m_new = torch.maximum(m, blk.max(-1).values)
        safe = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
        l = l * torch.exp(torch.where(torch.isinf(m), torch.full_like(m, float("-inf")), m - safe)) + torch.exp(blk - safe[..., None]).sum(-1)
        m = m_new
    safe = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    p = torch.exp(s - safe[..., None]) / l.clamp_min(1e-30)[..., None]
    return torch.where(allowed, p, torch.zeros_like(p))


def mqa_case(B, S, seed, lengths=None, heads=8, width=512):
    """K21's operands: memory [B, S, 512] is key AND value -- the class code in its first 8 columns, integers in [-127, 127] in the rest;
    qp [B, 8 * 512] is the absorbed query, -2^10 on the code columns of the other classes.  Returns (AttnCase with h = 1 holding the
    memory as k and v, qp, query_class [B, heads])."""
    c = attention_case(B, 1, 1, S, width, seed, lengths=lengths)
    mem = c.v.clone()
    mem[:, :, :8] = c.k[:, :, :8]
    c.k = c.v = mem
    g = _gen(seed + 31)
    ncls = torch.tensor([max(1, bin(n).count("1")) for n in c.lengths])
    qc = torch.randint(0, 1 << 30, (B, heads), generator=g) % ncls[:, None]
    cols = torch.arange(width)
    qp = torch.where((cols < ncls[:, None, None]) & (cols != qc[..., None]), -CODE, 0.0).to(F64)  # [B, heads, width]
    return c, qp.reshape(B, heads * width), qc


def mqa_output(c, qc, device="cpu"):
    """[B, heads * 512] float64: per head the mean of the memory rows of the head's class."""
    kc = c.key_class[:, 0, :].to(device)                                                   # [B, S]
    match = (kc[:, None, :] == qc.to(device)[:, :, None]) & (kc[:, None, :] >= 0)          # [B, heads, S]
    P = match.to(F64) / match.sum(-1, keepdim=True).clamp_min(1).to(F64)
    return (P @ c.k.to(device)).reshape(P.shape[0], -1), P


# ---------------------------------------------------------------------------------------------------------------------------------
# the committed cases: the GPU tests take their operands from here, the CPU test proves the claims for exactly these
# ---------------------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = {
    128: [(1, 1, 1), (7, 5, 20), (129, 127, 65), (200, 130, 136), (128, 128, 192)],
    256: [(256, 256, 64 * k) for k in range(1, 6)] + [(512, 768, 128)],
    64: [(64, 64, 64), (128, 192, 640), (320, 64, 192)],
}
GEMM_PERSISTENT = (5120, 4096, 192)
GEMM_SPLIT_K = 64 * 11
GEMM_SLAB = (256, 256, 64 * 64)
GEMM_EPILOGUE_SHAPE = {128: (200, 136, 136), 256: (256, 512, 256), 64: (128, 192, 256)}  # K >= 256 on the DMA tilings: bf16 outputs that round


def gemm_seed(M, N, K):
    return (M * 31 + N) * 17 + K


_CASES = {}


def attn(N, h, Lq, Lk, d, causal=False, mode="classes", lengths=None, v_bound=V_BOUND):
    """The committed case of this geometry (built once per process and shared: treat it as read-only)."""
    key = (N, h, Lq, Lk, d, causal, mode, None if lengths is None else tuple(lengths), v_bound)
    if key not in _CASES:
        seed = (((N * 7 + h) * 1009 + Lq) * 4099 + Lk) * 13 + d + (8 if causal else 0) + {"classes": 0, "class_const": 1, "uniform": 2}[mode]
        _CASES[key] = attention_case(N, h, Lq, Lk, d, seed, lengths=lengths, causal=causal, mode=mode, v_bound=v_bound)
    return _CASES[key]


FUSED_D = (32, 64, 96, 160, 320, 480)
FUSED_SHAPES = [(4, 2, 40, 72), (4, 3, 130, 292)]
CAUSAL_SHAPE, CAUSAL_D = (4, 2, 70, 70), (32, 64, 96)
FLASH_64 = (4, 3, 130, 520)
RESIDENT_SELF = [(4, 2, 292, 292), (4, 2, 384, 384)]
RESIDENT_CROSS = [(4, 2, 1, 384), (4, 2, 257, 292)]
RESIDENT_MANY = (40, 8, 320, 320)
SPLIT_KV = (4, 2, 40, 3840)
DECODE = [(40, 8, 37), (300, 1, 129)]
DECODE_APPEND, DECODE_APPEND_T = (40, 8, 37), (0, 17, 36)   # (N, h, cache length), the positions appended
SCORES = [(d, Lk) for d in (128, 192, 320) for Lk in (8, 200, 376)]   # (head_dim, Lk) of the K17 cases; N 4, h 2, Lq 40
UNFUSED = [(4, 2, 13, 200, 20, False), (4, 2, 5, 5, 4, True)]
MQA = [(3, 1000), (7, 37), (1, 8200)]


def decode_append_lengths(N, t):
    """Valid prefixes for the decode step at position t: one item up to and including t, one cut short (position t is cached but not
    attended: a PAD token), one with a single valid key, one with none."""
    base = [t + 1, cut_length(t + 1), 1, 0]
    return [base[i % 4] for i in range(N)]


def all_attention_cases():
    """Every (args, kwargs) the GPU tests pass to ``attn``."""
    out = []
    for d in FUSED_D:
        for shape in FUSED_SHAPES:
            out += [(shape + (d,), dict(mode=m)) for m in ("classes", "class_const", "uniform")]
    out += [(CAUSAL_SHAPE + (d,), dict(causal=True, mode=m)) for d in CAUSAL_D for m in ("classes", "class_const")]
    for shape in [FLASH_64] + RESIDENT_SELF + RESIDENT_CROSS + [SPLIT_KV]:
        out += [(shape + (64,), dict(mode=m)) for m in ("classes", "class_const", "uniform")]
    out += [(RESIDENT_MANY + (64,), dict(mode="class_const"))]
    out += [((N, h, 1, Lk, 64), {}) for (N, h, Lk) in DECODE]
    out += [(DECODE_APPEND[:2] + (1, DECODE_APPEND[2], 64), dict(lengths=decode_append_lengths(DECODE_APPEND[0], t))) for t in DECODE_APPEND_T]
    out += [((4, 2, 40, Lk, d), dict(mode=m)) for (d, Lk) in SCORES for m in ("classes", "class_const", "uniform")]
    for (N, h, Lq, Lk, d, causal) in UNFUSED:
        out += [((N, h, Lq, Lk, d), dict(causal=causal, mode=m, v_bound=4 if m == "uniform" else V_BOUND))
                for m in (("classes", "class_const") if causal else ("classes", "class_const", "uniform"))]
    return out



# ---------------------------------------------------------------------------------------------------------------------------------
# K8, the dual co-attention (csrc/interaction.hip): U[i, j] = w1 . Eq[j] + w2 . Ep[i] + (w3 o Ep[i]) . Eq[j]
# ---------------------------------------------------------------------------------------------------------------------------------
# A few "code" dimensions inside ONE 64-wide K group carry the class: passage row i of class c has 2^5 at code dimension c, query row j of
# class c has -2^5 at every OTHER code dimension, and w3 = 2^10 there: the score is 0 inside the class and -2^20 outside.  w3 = 0 on every
# other dimension, which holds the payload: integers in [-bound, bound].  w1 = -2^20 on one marker dimension that a few ("marked") query rows
# carry as 1: those columns drop out of the softmax over j; w2 = -2^20 on another marker dimension that a few passage rows carry: those rows
# drop out of the softmax over i.  (A marked passage row keeps its own softmax over j: its scores move together.)  The unmarked valid rows of
# a class are a power of two, so every entry of A and Bm^T is exactly 1 / n or 0; w3 Eq + w2 is 0, -2^15 or -2^20: exact in bf16.
K8_H, K8_LQ = 512, 64
K8_CODE, K8_W3, K8_SOFT = 32.0, 1024.0, -2.0 ** 20
K8_CODE_OFFSETS = (1, 9, 34, 43, 62)          # inside the K group: both lane halves, four different K steps
K8_Q_PARTS, K8_Q_MARKED = (32, 16, 8), 4      # 56 unmarked valid query rows + 4 marked + 4 padded, scattered
K8_P_PARTS = {32: (16, 8, 4), 96: (64, 16, 8), 384: (256, 64, 32), 416: (256, 128, 16), 512: (256, 128, 64)}
K8_P_MARKED = {32: 2, 96: 4, 384: 8, 416: 8, 512: 8}


def k8_dims(gk, ncode=3):
    """(code dimensions, marker of w1, marker of w2): the code in K group gk, the markers three and five groups further."""
    return [64 * gk + o for o in K8_CODE_OFFSETS[:ncode]], 64 * ((gk + 3) % 8) + 21, 64 * ((gk + 5) % 8) + 50


def _k8_side(L, classes, parts, marked, g):
    """(valid [L], class [L], marked [L]): the parts scattered over the L positions; marked and padded rows carry a class of the side too."""
    perm = torch.randperm(L, generator=g)
    cls = torch.tensor(classes)[torch.randint(0, len(classes), (L,), generator=g)]
    valid, mark = torch.zeros(L, dtype=torch.bool), torch.zeros(L, dtype=torch.bool)
    pos = 0
    for c, n in zip(classes, parts):
        cls[perm[pos:pos + n]] = c
        valid[perm[pos:pos + n]] = True
        pos += n
    assert pos + marked <= L
    valid[perm[pos:pos + marked]] = True
    mark[perm[pos:pos + marked]] = True
    return valid, cls, mark


class InteractionCase(object):
    """Eq [B, nq, 64, 512], Ep [B, P, Lp, 512] float64 (exact in bf16), qv [B, nq, 64], pv [B, P, Lp] bool, w [1, 1536] float64."""

    def pairs(self, device="cpu"):
        """The operands expanded per pair: Eq [n, 64, H], Ep [n, Lp, H], qv [n, 64], pv [n, Lp]."""
        B, nq, P = self.B, self.nq, self.P
        Eq = self.Eq.to(device).expand(B, P, K8_LQ, K8_H) if nq != P else self.Eq.to(device)
        qv = self.qv.to(device).expand(B, P, K8_LQ) if nq != P else self.qv.to(device)
        return (Eq.reshape(B * P, K8_LQ, K8_H), self.Ep.to(device).reshape(B * P, self.Lp, K8_H), qv.reshape(B * P, K8_LQ),
                self.pv.to(device).reshape(B * P, self.Lp))


def interaction_case(B, P, nq, Lp, seed, gk=0, v_bound=V_BOUND, q=None, p=None):
    """``q`` / ``p``: (classes, parts, marked) of the ordinary queries / passages (default: three classes on both sides).  Passage P - 1 of
    sample 0 has two valid rows (classes 0 and 1), the first query of the last sample has no valid token (B > 1)."""
    g = _gen(seed)
    q = ((0, 1, 2), K8_Q_PARTS, K8_Q_MARKED) if q is None else q
    p = ((0, 1, 2), K8_P_PARTS[Lp], K8_P_MARKED[Lp]) if p is None else p
    ncode = 1 + max(max(q[0]), max(p[0]))
    code, m1, m2 = k8_dims(gk, ncode)
    code_t = torch.tensor(code)
    c = InteractionCase()
    c.B, c.P, c.nq, c.Lp, c.gk, c.v_bound, c.code, c.m1, c.m2 = B, P, nq, Lp, gk, v_bound, code, m1, m2
    c.Eq = ints((B, nq, K8_LQ, K8_H), seed + 7919, bound=v_bound)
    c.Ep = ints((B, P, Lp, K8_H), seed + 104729, bound=v_bound)
    c.qv, c.pv = torch.zeros(B, nq, K8_LQ, dtype=torch.bool), torch.zeros(B, P, Lp, dtype=torch.bool)
    c.q_marked, c.p_marked = torch.zeros_like(c.qv), torch.zeros_like(c.pv)
    for b in range(B):
        for k in range(nq):
            valid, cls, mark = _k8_side(K8_LQ, q[0], q[1], q[2], g)
            if B > 1 and b == B - 1 and k == 0:
                valid = torch.zeros_like(valid)  # codes, markers and payload stay: only the mask says that these rows do not count
            c.Eq[b, k][:, code_t] = torch.where(cls[:, None] == torch.arange(ncode)[None, :], 0.0, -K8_CODE).to(F64)
            c.Eq[b, k][:, m1] = mark.to(F64)
            c.qv[b, k], c.q_marked[b, k] = valid, mark & valid
        for k in range(P):
            side = ((0, 1), (1, 1), 0) if (b == 0 and k == P - 1) else p
            valid, cls, mark = _k8_side(Lp, side[0], side[1], side[2], g)
            c.Ep[b, k][:, code_t] = torch.where(cls[:, None] == torch.arange(ncode)[None, :], K8_CODE, 0.0).to(F64)
            c.Ep[b, k][:, m2] = mark.to(F64)
            c.pv[b, k], c.p_marked[b, k] = valid, mark
    w = torch.zeros(3 * K8_H, dtype=F64)
    w[m1], w[K8_H + m2] = K8_SOFT, K8_SOFT
    w[2 * K8_H + code_t] = K8_W3
    c.w = w.reshape(1, 3 * K8_H)
    return c


def bf16_f64(x):
    """float64 -> f32 -> bf16 (each to nearest even) -> float64: a bf16 store of an f32 value, restated."""
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def interaction_restated(Eq, Ep, qv, pv, w):
    """The kernels' arithmetic in float64 with their bf16 roundings at the points where they round (operands per pair, any device):
    w3 Eq + w2 once in LDS; A and Bm^T as stored; A1 = A Eq and B1 = Bm^T Ep once (tile_to_lds) -- A2 = A B1, B2 = Bm^T A1 and the four
    elementwise products (mul8) read the ROUNDED values.  Returns the stored values ("A", "Bt", "Gqp", "Gpq": float64 holding bf16 values,
    padded rows 0) and, under "raw", the values in front of each rounding (what must be exact in f32 for the exact cases)."""
    H = K8_H
    w1, w2, w3 = w.reshape(-1)[:H], w.reshape(-1)[H:2 * H], w.reshape(-1)[2 * H:]
    bq = bf16_f64(Eq * w3 + w2)
    U = (Eq @ w1)[:, None, :] + Ep @ bq.transpose(1, 2)                                    # [n, Lp, 64]
    mask = pv[:, :, None] & qv[:, None, :]
    U = torch.where(mask, U, torch.full_like(U, float("-inf")))

    def softmax(u, dim):
        m = u.max(dim, keepdim=True).values
        e = torch.where(mask, torch.exp(u - torch.where(torch.isinf(m), torch.zeros_like(m), m)), torch.zeros_like(u))
        s = e.sum(dim, keepdim=True)
        return e / torch.where(s > 0, s, torch.ones_like(s))

    raw = {"U": U, "A": softmax(U, 2), "Bt": softmax(U, 1).transpose(1, 2)}
    A, Bt = bf16_f64(raw["A"]), bf16_f64(raw["Bt"])
    raw["A1"], raw["B1"] = A @ Eq + 0.0, Bt @ Ep + 0.0                                     # (+ 0.0: a sum of -0 terms is +0 on the MFMA)
    A1, B1 = bf16_f64(raw["A1"]), bf16_f64(raw["B1"])
    raw["A2"], raw["B2"] = A @ B1 + 0.0, Bt @ A1 + 0.0
    A2, B2 = bf16_f64(raw["A2"]), bf16_f64(raw["B2"])
    raw["EpA1"], raw["EpA2"], raw["EqB1"], raw["EqB2"] = Ep * A1, Ep * A2, Eq * B1, Eq * B2
    zero = torch.zeros((), dtype=F64, device=Eq.device)
    Gqp = torch.where(pv[:, :, None], torch.cat([Ep, A1, A2, bf16_f64(raw["EpA1"]), bf16_f64(raw["EpA2"])], -1), zero)
    Gpq = torch.where(qv[:, :, None], torch.cat([Eq, B1, B2, bf16_f64(raw["EqB1"]), bf16_f64(raw["EqB2"])], -1), zero)
    return {"A": A, "Bt": Bt, "Gqp": Gqp, "Gpq": Gpq, "raw": raw}


K8_GEOMETRY = [(3, 3, nq, Lp) for Lp in (32, 96, 384, 416, 512) for nq in (1, 3)]   # (B, P, nq, Lp): nq = 1 is eq_div = P
K8_GROUPS = (3, 3, 1, 96)                                                          # the shape of the eight K-group cases
K8_SMALL_PAYLOAD = [(3, 3, 1, 384), (3, 3, 3, 96)]                                  # |v| <= 15
K8_MANY = (29, 9, 1, 32)                                                           # 261 pairs: more than the 256 CUs
K8_ORPHAN = (3, 3, 1, 96)  # query class 4 and passage class 3 have no counterpart: uniform over ALL unmarked valid rows (32 and 64 of them)
K8_ORPHAN_Q, K8_ORPHAN_P = ((0, 1, 2, 4), (16, 8, 4, 4), 4), ((0, 1, 2, 3), (32, 16, 8, 8), 4)

_K8 = {}


def k8(B, P, nq, Lp, gk=None, v_bound=V_BOUND, orphan=False):
    """The committed K8 case (built once per process: read-only).  gk None: the K group follows from the geometry."""
    gk = (Lp // 32 + nq) % 8 if gk is None else gk
    key = (B, P, nq, Lp, gk, v_bound, orphan)
    if key not in _K8:
        seed = ((((B * 31 + P) * 7 + nq) * 1031 + Lp) * 11 + gk) * 3 + (1 if v_bound == V_BOUND else 0) + (500000 if orphan else 0)
        _K8[key] = interaction_case(B, P, nq, Lp, seed, gk=gk, v_bound=v_bound, q=K8_ORPHAN_Q if orphan else None,
                                    p=K8_ORPHAN_P if orphan else None)
    return _K8[key]


def all_k8_cases():
    """Every (args, kwargs) the GPU tests pass to ``k8``."""
    out = [(s, {}) for s in K8_GEOMETRY]
    out += [(K8_GROUPS, dict(gk=gk)) for gk in range(8)]
    out += [(s, dict(v_bound=GEMM_BOUND)) for s in K8_SMALL_PAYLOAD]
    out += [(K8_MANY, {}), (K8_ORPHAN, dict(orphan=True))]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# K16, the encoder chain (csrc/encoder_chain.hip): y = ctx Wo^T + bo + s; s2 = LN2(y); a = gelu(s2 W1^T + b1); o = a W2^T + b2 + s2;
# s' = LN1'(o); qkv' = s' Wqkv'^T + bqkv'.  The layer's parameters are written so that each stage stands alone.
# ---------------------------------------------------------------------------------------------------------------------------------
CHAIN_E = 512
CHAIN_EPS2, CHAIN_EPS1N = 0.5, 2.0   # clearly different: on the quiet rows (variance 1 to 3) swapping them moves the result by tens of bf16 steps
CHAIN_M = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 257)
CHAIN_GAMMA = (0.0, 0.5, -0.5, 1.0, -1.0, 1.5, 2.0, -0.25)
CHAIN_BETA = (0.0, 0.25, -0.25, 1.0, -1.0, 3.0, 0.0, 0.5)
CHAIN_PERMS = (0, 5, 11)


def pick(n, seed, values):
    return torch.tensor(values, dtype=F64)[torch.randint(0, len(values), (n,), generator=_gen(seed))]


def chain_tokens(M, seed, quiet="small", bound=GEMM_BOUND):
    """[M, 512] integers in [-bound, bound], a different row per token; every third row is "quiet": integers in [-1, 1] ("small") or 0."""
    x = ints((M, CHAIN_E), seed, bound=bound)
    q = torch.arange(M) % 3 == 1
    small = ints((M, CHAIN_E), seed + 1, bound=1, zero_share=0.0) if quiet == "small" else torch.zeros(M, CHAIN_E, dtype=F64)
    return torch.where(q[:, None], small, x)


def signed_perm(r, seed, blocks=1):
    """[512 blocks, 512]: per block of 512 rows a signed permutation times a power of two (2^-1 .. 2^2).  Row n = 16 fb + i of block c has
    its one entry in column 32 ((i + fb + r + c) % 16) + (fb + 3 (r + c)) % 32: every (16 features x 32 k) fragment of the weight pack
    holds exactly one non-zero entry."""
    g = _gen(seed)
    out = []
    for c in range(blocks):
        n = torch.arange(CHAIN_E)
        fb, i = n // 16, n % 16
        col = 32 * ((i + fb + r + c) % 16) + (fb + 3 * (r + c)) % 32
        val = (torch.randint(0, 2, (CHAIN_E,), generator=g) * 2 - 1).to(F64) * 2.0 ** torch.randint(-1, 3, (CHAIN_E,), generator=g).to(F64)
        w = torch.zeros(CHAIN_E, CHAIN_E, dtype=F64)
        w[n, col] = val
        out.append(w)
    return torch.cat(out, 0)


GELU_TARGETS = tuple(range(8, 65)) + tuple(range(-64, -19)) + (0,) * 40   # pre-activations of which gelu_f gives exactly x, -0 or 0


def chain_layer(kind, seed=0):
    """The layer's tensors as float64 (all exact in bf16 / f32).  kind:
    "A"  W1 = 0, b1 = b2 = 0 (a = gelu(0) = 0, o = s2): dense integer Wo, bo in [-2, 2], dyadic g2 / be2 with zeros and negative entries;
    "Ap" as A with Wo a signed permutation;
    "B1" g2 = 0 (s2 = be2 on every token), integer be2 / W1 and b1 such that every pre-activation is a GELU_TARGET; dense integer W2, b2 = 0;
    "B3" as B1 with W1 a signed permutation and b2 != 0;
    "B2" be2 = 0, W1 = 0, b1 a dyadic grid over [-8, 8), W2 a signed permutation, b2 = 0: o[n] = +-2^k bf16(gelu(b1[pi(n)]))."""
    E, z = CHAIN_E, torch.zeros(CHAIN_E, dtype=F64)
    lay = {"kind": kind, "eps2": CHAIN_EPS2}
    lay["Wo"] = signed_perm(3, seed + 1) if kind == "Ap" else ints((E, E), seed + 1)
    lay["bo"] = ints((E,), seed + 2, bound=2)
    if kind in ("A", "Ap"):
        lay["g2"], lay["be2"] = pick(E, seed + 3, CHAIN_GAMMA), pick(E, seed + 4, CHAIN_BETA)
        lay["W1"], lay["b1"], lay["W2"], lay["b2"] = torch.zeros(E, E, dtype=F64), z, ints((E, E), seed + 5), z
    elif kind in ("B1", "B3"):
        lay["g2"], lay["be2"] = z, ints((E,), seed + 4, bound=3)
        lay["W1"] = signed_perm(7, seed + 6) if kind == "B3" else ints((E, E), seed + 6)
        lay["target"] = pick(E, seed + 7, GELU_TARGETS)
        lay["b1"] = lay["target"] - lay["W1"] @ lay["be2"]
        lay["W2"], lay["b2"] = ints((E, E), seed + 5), (ints((E,), seed + 8) if kind == "B3" else z)
    else:
        assert kind == "B2"
        lay["g2"], lay["be2"], lay["W1"] = z, z, torch.zeros(E, E, dtype=F64)
        lay["b1"] = (torch.arange(E, dtype=F64) / 32.0 - 8.0)[torch.randperm(E, generator=_gen(seed + 9))]
        lay["W2"], lay["b2"] = signed_perm(2, seed + 10), z
    return lay


def chain_next(r, seed=0):
    """The next layer's norm1 and in-projection: dyadic g1n / be1n; Wqkv three signed permutations (r in CHAIN_PERMS) or dense integers
    (r None); bqkv multiples of 1/4 in [-2, 2]."""
    nxt = {"r": r, "eps1n": CHAIN_EPS1N, "g1n": pick(CHAIN_E, seed + 21, CHAIN_GAMMA), "be1n": pick(CHAIN_E, seed + 22, CHAIN_BETA)}
    nxt["Wqkv"] = ints((3 * CHAIN_E, CHAIN_E), seed + 23) if r is None else signed_perm(r, seed + 23, blocks=3)
    nxt["bqkv"] = ints((3 * CHAIN_E,), seed + 24, bound=8) / 4.0
    return nxt


def layer_norm64(y, gamma, beta, eps):
    """(LN(y), xhat) in float64 (biased variance, as nn.LayerNorm)."""
    mean = y.mean(-1, keepdim=True)
    var = ((y - mean) ** 2).mean(-1, keepdim=True)
    xhat = (y - mean) / torch.sqrt(var + eps)
    return xhat * gamma + beta, xhat


def layer_norm_bound(ref, xhat, gamma, beta):
    """One bf16 step at a tie plus the f32 evaluation error on the terms in front of their cancellation."""
    return 2.0 ** -8 * ref.abs() + 2.0 ** -20 * ((xhat * gamma).abs() + beta.abs())


def layer_norm_f32(y, gamma, beta, eps, order_seed, two_pass=False):
    """The kernel's f32 LayerNorm restated on the CPU with a shuffled sum: one pass (E[x^2] - mean^2, stages 0 and 2) or two (the head)."""
    x = y.to(torch.float32)
    perm = torch.randperm(x.shape[-1], generator=_gen(order_seed))
    inv = torch.tensor(1.0 / CHAIN_E, dtype=torch.float32)

    def total(t):
        acc = torch.zeros(t.shape[:-1], dtype=torch.float32)
        for idx in perm.chunk(8):
            acc = acc + t[..., idx].sum(-1)
        return acc

    mean = total(x) * inv
    if two_pass:
        var = total((x - mean[..., None]) ** 2) * inv
    else:
        var = (total(x * x) * inv - mean * mean).clamp_min(0.0)
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    return ((x - mean[..., None]) * rstd[..., None]) * gamma.to(torch.float32) + beta.to(torch.float32)


def chain_y(ctx, s, lay):
    dev = ctx.device
    return ctx @ lay["Wo"].to(dev).t() + lay["bo"].to(dev) + s


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / 2.0 ** 0.5))


def gelu_f32(x):
    """common.h's gelu_terms / gelu_f restated in f32 on the CPU (separate multiplies and adds where the kernel has FMAs) -> (gelu, Phi)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    x = x.to(torch.float32)
    z = x.abs() * f(0.70710678118654752)
    t = 1.0 / (f(0.3275911) * z + 1.0)
    e = torch.exp(-z * z)
    p = f(1.061405429) * t + f(-1.453152027)
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = p * t + f(c)
    q = 0.5 * p * t * e
    cdf = torch.where(x >= 0, 1.0 - q, q)
    return x * cdf, cdf


def gelu_eps_phi(grid):
    """max |Phi_f32(x) - Phi_64(x)| over the grid, DOUBLED for the device's v_rcp and v_exp: the Phi term of the GELU bar."""
    phi64 = 0.5 * (1.0 + torch.erf(grid.to(F64) / 2.0 ** 0.5))
    return 2.0 * (gelu_f32(grid)[1].to(F64) - phi64).abs().max().item()


def chain_ffn(lay, rows=1):
    """Families B1 / B3: (s2, a, o) of one token in float64 -- the same for every token, since g2 = 0."""
    s2 = lay["be2"]
    pre = lay["W1"] @ s2 + lay["b1"]
    a = torch.where(pre > 0, pre, torch.zeros_like(pre))
    return s2, a, lay["W2"] @ a + lay["b2"] + s2


# ---------------------------------------------------------------------------------------------------------------------------------
# K7 / K22: the additive attention  s[b,t,j] = sum_h v_h tanh(wq[b,t,h] + uh[b,j,h])  (csrc/attn_pointer.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
# Two operand families.
#   ternary    wq = 10 sw, uh = 10 su with seeded random signs: wq + uh is 0 or +-20, tanh is 0 or +-1 and 1 - tanh^2 is 1 or 0 (to below
#              1e-16); v in {+-1, +-2}, ds integers in [-3, 3].  s, d_wq, d_uh and d_v are integers below 2^24 that depend on every one of
#              b, t, j, h, so the f32 path (tanhf is exact at 0 and at +-20) must give the float64 restatement in every bit, through any
#              summation order and any split with atomics.  10 is exact in bf16 and inside the +-21.4 clamp of the factored form.
#   mid-range  normal operands at scale 1.5 (v at 0.3, ds at 1): the numerics -- the prescale, the factors 4 and 2, the clamp.
# k7_reference is the float64 restatement TOGETHER with its error bound, element by element, per arithmetic form of the kernels.  With
# u = 2^-24 and first-order terms only (every constant carries a factor 1 + 2^-10 for the higher orders):
#   "tanhf"     th = tanhf(fl(w + u)): the rounded sum moves tanh by u |x| (1 - th^2), tanhf itself by EPS_TANHF |th|.
#               1 - th th: two more roundings, |d(1 - th^2)| <= 2 |th| dth + 2 u.
#   "factored"  ws = fl(PS w), us = fl(PS u), PS = fl(2 / ln 2): each prescaled argument is off by ARG = 2 u relative (the constant's rounding
#               and the product's), which moves 2^ws 2^us by the factor (|ws| + |us|) ln 2 ARG = 2 (|w| + |u|) ARG; the two v_exp_f32 add
#               EPS_EXP each:  eta = 2 (|w| + |u|) ARG + 2 EPS_EXP  is the relative error of E = e^{2x} as the kernel has it.
#               r = rcp(fma(ew, eu, 1)): d r / d ln E = -r (1 - r); the fma's rounding and v_rcp_f32 are relative errors of r itself:
#               dr = r (1 - r) eta + r (u + EPS_RCP);  tanh = 1 - 2 r: dth = 2 dr;  1 - tanh^2 = 4 r (1 - r), taken as g r - (g r) r:
#               |d(4 r (1 - r))| <= 4 |1 - 2 r| dr + 8 u r  (three roundings of magnitude <= g r).
#   "exp2x"     the row-wise bf16 kernel: 1 - __fdividef(2, __expf(2 fl(w + u)) + 1).  __expf(y) is v_exp_f32(fl(y log2 e)): relative error
#               |y| ARG + EPS_EXP, and the rounded sum adds 2 u |x|: eta = 6 u |x| + EPS_EXP;  dr = r (1 - r) eta + r (u + EPS_FDIV),
#               dth = 2 dr + u |th| (the final subtraction).
#   "cached"    K22: E = EW eu with eu the kernel's own bf16 input (exact) and EW = __expf(clip(2 w)): eta = |2 w| ARG + EPS_EXP, dr as in
#               "factored" (k22_reference).
# Sums: n terms accumulated in f32 in ANY order (sequential, tree, partial sums added with atomics) err by at most (n + c) u sum |term|; c
# counts the roundings outside the sum (each term's product, the factor v_h or 4 v_h, the final subtraction).  The forward of the factored
# form is vsum - 2 acc with acc = sum v r: 2 (H + 2) u sum |v| (r <= 1 and the v-sum share one bar); its d_v is gsum - 2 dv in the same way.
U32 = 2.0 ** -24 * (1 + 2.0 ** -10)
ULP32 = 2 * U32            # one ulp as a relative error: 2^-23 2^e <= 2^-23 |y|
EPS_EXP = 1 * ULP32        # v_exp_f32: 1 ulp (CDNA4 ISA guide, VOP1 transcendental accuracy)
EPS_RCP = 1 * ULP32        # v_rcp_f32: 1 ulp (same table)
EPS_FDIV = 2 * ULP32       # __fdividef: 2 ulp (HIP math API, single-precision intrinsics; the table is not in the ROCm tree, CUDA's lists the same)
EPS_TANHF = 5 * ULP32      # tanhf: OpenCL 3.0 table 7.4 (tanh <= 5 ulp); the HIP math API table is not in the ROCm tree
ARG32 = 2 * U32
K7_A = 10.0
K7_CLAMP = 21.0            # inputs stay inside |x| <= 21: the factored form's clamp (+-62 / (2 / ln 2) = 21.49) never acts
K7_FORMS = ("tanhf", "factored", "exp2x")


def k7_ternary(B, T, S, H, seed):
    """(wq [B,T,H], uh [B,S,H], v [H], ds [B,T,S]) in float64, all exact in bf16."""
    g = _gen(seed)
    pm = lambda *shape: (torch.randint(0, 2, shape, generator=g) * 2 - 1).to(F64)
    wq, uh = K7_A * pm(B, T, H), K7_A * pm(B, S, H)
    v = pm(H) * torch.randint(1, 3, (H,), generator=g).to(F64)
    ds = torch.randint(-3, 4, (B, T, S), generator=g).to(F64)
    return wq, uh, v, ds


def k7_midrange(B, T, S, H, seed):
    """The same four operands, normal: wq, uh at scale 1.5 (cut at +-K7_CLAMP / 2, so that |wq + uh| <= 21), v at 0.3, ds at 1; rounded to f32
    (the caller rounds uh once more where the kernel reads bf16)."""
    g = _gen(seed)
    rn = lambda scale, *shape: (torch.randn(shape, generator=g) * scale).to(torch.float32).to(F64)
    half = K7_CLAMP / 2
    return rn(1.5, B, T, H).clamp(-half, half), rn(1.5, B, S, H).clamp(-half, half), rn(0.3, H), rn(1.0, B, T, S)


K7_FAMILIES = {"ternary": k7_ternary, "mid": k7_midrange}


def k7_seed(B, T, S, H):
    return (B * 1000003 + T * 10007 + S * 101 + H) % (2 ** 31)


def k7_element(form, w, u, prescale=1.0):
    """(tanh, 1 - tanh^2, bound on the kernel's tanh, bound on the kernel's 1 - tanh^2) of w + u, broadcast, float64."""
    x = (w + u) * prescale
    th = torch.tanh(x)
    r = torch.sigmoid(-2.0 * x)          # 1 / (e^{2x} + 1)
    gp = 4.0 * r * (1.0 - r)             # 1 - tanh^2 without the cancellation
    if form == "tanhf":
        dth = U32 * x.abs() * gp + EPS_TANHF * th.abs()
        return th, gp, dth, 2.0 * th.abs() * dth + 2.0 * U32
    if form == "factored":
        eta = 2.0 * (w.abs() + u.abs()) * ARG32 + 2.0 * EPS_EXP
        dr = r * (1.0 - r) * eta + r * (U32 + EPS_RCP)
        return th, gp, 2.0 * dr, 4.0 * (1.0 - 2.0 * r).abs() * dr + 8.0 * U32 * r
    if form == "exp2x":
        eta = 6.0 * U32 * x.abs() + EPS_EXP
        dr = r * (1.0 - r) * eta + r * (U32 + EPS_FDIV)
        return th, gp, 2.0 * dr + U32 * th.abs(), None
    raise ValueError(form)


def k7_reference(wq, uh, v, ds=None, form="tanhf", prescale=1.0, limit=1 << 22):
    """float64 restatement on the device of the operands, in chunks over the items so that no [b, T, S, H] temporary exceeds ``limit``
    elements (32 MB).  -> {name: (value, bound)} for s and, with ``ds``, d_wq, d_uh, d_v."""
    B, T, H = wq.shape
    S = uh.shape[1]
    assert T * S * H <= 1 << 23, "one item alone is too large for a chunk"
    nb = max(1, limit // (T * S * H))
    c = 2 if form == "factored" else 1
    av, z = v.abs(), lambda *shape: torch.zeros(shape, dtype=F64, device=wq.device)
    s, s_b = z(B, T, S), z(B, T, S)
    if ds is not None:
        d_wq, d_wq_b, d_uh, d_uh_b, d_v, d_v_b, d_v_abs = z(B, T, H), z(B, T, H), z(B, S, H), z(B, S, H), z(H), z(H), z(H)
    for b0 in range(0, B, nb):
        sl = slice(b0, min(B, b0 + nb))
        th, gp, dth, dgp = k7_element(form, wq[sl, :, None, :], uh[sl, None, :, :], prescale)
        s[sl] = (th * v).sum(-1)
        s_b[sl] = (dth * av).sum(-1) + c * (H + 2) * U32 * av.sum()
        if ds is None:
            continue
        g = ds[sl, :, :, None]
        ag = g.abs()
        d_uh[sl] = v * (g * gp).sum(1)
        d_uh_b[sl] = av * ((ag * dgp).sum(1) + (T + 4) * U32 * (ag * gp).sum(1))
        d_wq[sl] = v * (g * gp).sum(2)
        d_wq_b[sl] = av * ((ag * dgp).sum(2) + (S + 4) * U32 * (ag * gp).sum(2))
        d_v += (g * th).sum((0, 1, 2))
        d_v_b += (ag * dth).sum((0, 1, 2))
        d_v_abs += (ag * th.abs()).sum((0, 1, 2)) if c == 1 else ag.sum()
    out = {"s": (s, s_b)}
    if ds is not None:
        out.update(d_wq=(d_wq, d_wq_b), d_uh=(d_uh, d_uh_b), d_v=(d_v, d_v_b + c * (B * T * S + 4) * U32 * d_v_abs))
    return out


def k7_ternary_exact(ref):
    """The ternary family's float64 result is an integer or a half-integer up to the 1e-16 that 1 - tanh(20)^2 leaves: that number itself."""
    exact = torch.round(2.0 * ref) / 2.0
    assert float((ref - exact).abs().max()) < 1e-9 and float(exact.abs().max()) < 2 ** 24
    return exact


def k7_emulate(form, wq, uh, v, ds=None):
    """The kernels' arithmetic in float32 on the host (torch's exp2 / exp / tanh and a true division where the device has v_exp_f32,
    v_rcp_f32 and tanhf; torch's own summation order) -> {name: f32 tensor}: what a correct kernel may return, up to the instructions' own error."""
    f = lambda t: t.to(torch.float32)
    wq, uh, v = f(wq), f(uh), f(v)
    one = torch.tensor(1.0, dtype=torch.float32)
    if form == "factored":
        ps = torch.tensor(2.8853900817779268, dtype=torch.float32)
        ew, eu = torch.exp2((ps * wq).clamp(-62.0, 62.0)), torch.exp2((ps * uh).clamp(-62.0, 62.0))
        r = one / (ew[:, :, None, :] * eu[:, None, :, :] + one)
        out = {"s": v.sum() - 2.0 * (v * r).sum(-1)}
        if ds is not None:
            g = f(ds)[..., None]
            gr = g * r
            q = gr - gr * r
            out.update(d_uh=4.0 * v * q.sum(1), d_wq=4.0 * v * q.sum(2), d_v=g.expand_as(gr).sum((0, 1, 2)) - 2.0 * gr.sum((0, 1, 2)))
        return out
    x = wq[:, :, None, :] + uh[:, None, :, :]
    th = torch.tanh(x) if form == "tanhf" else one - 2.0 / (torch.exp(2.0 * x) + one)
    out = {"s": (v * th).sum(-1)}
    if ds is not None:
        g = f(ds)[..., None]
        q = g * (one - th * th)
        out.update(d_uh=v * q.sum(1), d_wq=v * q.sum(2), d_v=(g * th).sum((0, 1, 2)))
    return out


def k7_form(path, dtype):
    """The arithmetic form the launcher's choice computes with: f32 -> tanhf everywhere; bf16 -> factored (tiled forward, both backward
    sweeps) or exp(2x) with a division (row-wise forward)."""
    if dtype == torch.float32:
        return "tanhf"
    return "exp2x" if path == "rowwise" else "factored"


def k7_paths(B, T, S, H, dtype, aligned=True):
    """The launch rules of case_additive_scores_fwd / _bwd restated: (set of path names, dict of the launchers' figures)."""
    cdiv = lambda a, b: (a + b - 1) // b
    ev = 4 if dtype == torch.float32 else 8
    p, fig = set(), {}
    if T <= 2 and H % ev == 0 and H <= 2 * 64 * ev and aligned:
        nch = 1 if H <= 64 * ev else 2
        wgs = min(cdiv(S, 16), 64)
        p |= {"fwd.rowwise", "fwd.rowwise.T%d" % T, "fwd.rowwise.NCH%d" % nch, "fwd.rowwise.T%d.NCH%d" % (T, nch)}
        if S > 4 * wgs:
            p.add("fwd.rowwise.stride")
        if cdiv(S, 16) > 64 and S > 1024:
            p.add("fwd.rowwise.capped")
        fig.update(fwd="rowwise", nch=nch, wgs=wgs)
    else:
        jb, tchunks = cdiv(S, 64), cdiv(T, 32)
        p.add("fwd.tiled")
        if T <= 2:
            p.add("fwd.fallback.h_mod" if H % ev else "fwd.fallback.h_wide" if H > 2 * 64 * ev else "fwd.fallback.misaligned")
        if tchunks > 1:
            p.add("fwd.tiled.zstride" if jb * B < 512 else "fwd.tiled.loop")
        if H > 64:
            p.add("fwd.tiled.hchunks")
        for name, n, tile in (("h", H, 64), ("j", S, 64), ("t", T, 32)):
            if n % tile:
                p.add("fwd.tiled.ragged_" + name)
        fig.update(fwd="tiled", jb=jb, tchunks=tchunks, gz=tchunks if jb * B < 512 else 1)
    hb, tblocks, j_chunks = cdiv(H, 256), cdiv(T, 8), cdiv(S, 64)
    base = tblocks * hb * B
    sch = min(1 if base >= 2048 else cdiv(2048, base), j_chunks)
    j_per = cdiv(j_chunks, sch) * 64
    sch = cdiv(S, j_per)
    if hb > 1:
        p.add("bwd.hblocks")
    if sch > 1:
        p.add("bwd.wq.split")
        if j_per > 64:
            p.add("bwd.wq.split.multichunk")
        if S % j_per:
            p.add("bwd.wq.split.ragged")
    else:
        p.add("bwd.wq.unsplit")
        p.add("bwd.wq.unsplit.multichunk" if j_chunks > 1 else "bwd.wq.unsplit.onechunk")
    if T > 32:
        p.add("bwd.uh.tstage")
    if S < 16:
        p.add("bwd.uh.s_lt16")
    if S % 16:
        p.add("bwd.uh.ragged_s")
    fig.update(hb=hb, tblocks=tblocks, base_wgs=base, sch=sch, j_per=j_per, last_range=S - (sch - 1) * j_per)
    return p, fig


# (B, T, S, H): the smallest shapes that reach each path (tests/test_additive_exact_cpu.py asserts the reach)
K7_FWD_TILED = [(2, 3, 1, 1), (2, 32, 63, 63), (2, 33, 64, 64), (1, 3, 65, 65), (2, 11, 150, 96), (2, 70, 150, 512), (512, 70, 33, 8)]
K7_FWD_ROWWISE = {  # (B, T, S, H, aligned)
    torch.float32: [(2, 1, 77, 4, True), (2, 2, 1, 256, True), (1, 1, 1030, 260, True), (2, 2, 77, 512, True),
                    (2, 1, 77, 6, True), (2, 2, 77, 516, True), (2, 1, 77, 256, False)],
    torch.bfloat16: [(2, 1, 77, 8, True), (2, 2, 1, 512, True), (1, 1, 1030, 520, True), (2, 2, 77, 1024, True),
                     (2, 1, 77, 1032, True), (2, 2, 77, 512, False)],
}
K7_BWD = [(2, 1, 1, 1), (2, 7, 15, 255), (1, 8, 16, 256), (2, 9, 17, 257), (2, 33, 64, 512), (1, 65, 65, 8),
          (2, 40, 200, 512), (128, 64, 300, 8), (256, 64, 130, 8)]
K7_FWD_PATHS = {"fwd.tiled.zstride", "fwd.tiled.loop", "fwd.tiled.hchunks", "fwd.tiled.ragged_h", "fwd.tiled.ragged_j", "fwd.tiled.ragged_t",
                "fwd.rowwise.T1.NCH1", "fwd.rowwise.T1.NCH2", "fwd.rowwise.T2.NCH1", "fwd.rowwise.T2.NCH2", "fwd.rowwise.stride",
                "fwd.rowwise.capped", "fwd.fallback.h_mod", "fwd.fallback.h_wide", "fwd.fallback.misaligned"}
K7_BWD_PATHS = {"bwd.hblocks", "bwd.wq.split", "bwd.wq.split.multichunk", "bwd.wq.split.ragged", "bwd.wq.unsplit.multichunk",
                "bwd.wq.unsplit.onechunk", "bwd.uh.tstage", "bwd.uh.s_lt16", "bwd.uh.ragged_s"}


# K22 ---------------------------------------------------------------------------------------------------------------------------------
K22_H, K22_CLAMP, K22_MAX_S = 512, 43.0, 28000
TINY32 = 2.0 ** -120       # an f32 exponential that underflows is flushed: absolute, far below every probability compared here


def key_exp_reference(x):
    """case_additive_key_exp in float64 -> (e^{clip(2x, +-43)}, the f32 error of __expf in front of the one rounding to bf16)."""
    y = (2.0 * x.to(F64)).clamp(-K22_CLAMP, K22_CLAMP)
    ref = torch.exp(y)
    return ref, ref * (y.abs() * ARG32 + EPS_EXP)


def k22_depths(S, H=K22_H):
    """The most additions one term passes through in K22's three sums: (score: H / 64 per lane + 6 tree levels over the lanes; softmax sum and
    prior sum: ceil(S / 1024) per thread + 6 levels over the lanes + 6 over the 16 waves' partial sums; context: ceil(S / 16) rows per wave
    + 16 partial sums)."""
    return H // 64 + 6, -(-S // 1024) + 12, -(-S // 16) + 16


def k22_reference(w, eu, v, mem, cv=None, rv=None, prior=None, limit=1 << 22):
    """K22 in float64 from the kernel's own inputs: w [B, H] (the f32 sum wq + wq_add, upcast), eu / mem [B, S, H] (the bf16 tensors, upcast),
    v [H], masks bool, prior [B, S] -> {name: (value, bound)} for s, p, copy (with a prior) and ctx (the bound is the f32 one: the caller adds
    the one rounding to bf16).
    Sums: a term that passes through at most D additions errs by D u sum |term| whatever the order; the depths are the kernel's (a rewrite
    that sums no deeper meets them too): k22_depths.
      s     = sum v - 2 sum_h v_h r_h, r = rcp(fma(EW, eu, 1)): form "cached" above; each lane sums its 8 features, a reduction tree over the
              64 lanes follows (D = 14), for sum v and for sum v r alike, + 2 for the product and the last subtraction:
              2 sum |v_h| dr_h + 3 (D + 2) u sum |v|.
      p_j   = e_j / sum e, e_j = __expf(s_j - m) for ANY m (the softmax does not depend on the shift, so the kernel's maximum need not be the
              reference's): relative error rho_j = ds_j + u |y_j| (the subtraction) + |y_j| ARG + EPS_EXP (__expf); the sum of S positive
              terms (S / 1024 per thread, then trees over lanes and waves) has the p-weighted mean of the rho plus D_S u; 1 / sum, and the
              product: two more.  rel_j = rho_j + sum p rho + (D_S + 4) u.
      copy  = p prior / (1e-8f + sum p prior): rel_j + the (p prior)-weighted mean of the rel + (D_S + 6) u.
      ctx_h = sum_j p_j mem_jh: each of the 16 waves takes every 16th row by FMAs, the 16 partial sums are added in sequence (D_C):
              sum |dp_j| |mem_jh| + (D_C + 2) u sum p_j |mem_jh|.
    Masked positions, an item without a valid position and an invalid target row give exact zeros (bound 0)."""
    B, S, H = eu.shape
    dev = eu.device
    nb = max(1, limit // (S * H))
    av = v.abs()
    d_s, d_sum, d_ctx = k22_depths(S, H)
    s, s_b = torch.empty(B, S, dtype=F64, device=dev), torch.empty(B, S, dtype=F64, device=dev)
    for b0 in range(0, B, nb):
        sl = slice(b0, min(B, b0 + nb))
        y = (2.0 * w[sl, None, :]).clamp(-K22_CLAMP, K22_CLAMP)
        r = 1.0 / (torch.exp(y) * eu[sl] + 1.0)
        dr = r * (1.0 - r) * (y.abs() * ARG32 + EPS_EXP) + r * (U32 + EPS_RCP)
        s[sl] = v.sum() - 2.0 * (v * r).sum(-1)
        s_b[sl] = 2.0 * (av * dr).sum(-1) + 3.0 * (d_s + 2) * U32 * av.sum()
    valid = torch.ones(B, S, dtype=torch.bool, device=dev) if cv is None else cv.clone()
    live = valid.any(-1) if rv is None else valid.any(-1) & rv
    sm = s.masked_fill(~valid, float("-inf"))
    m = torch.where(valid.any(-1), sm.max(-1).values, torch.zeros(B, dtype=F64, device=dev))
    yj = torch.where(valid, s - m[:, None], torch.zeros_like(s))
    e = torch.where(valid, torch.exp(yj), torch.zeros_like(s))
    p = torch.where(live[:, None], e / e.sum(-1, keepdim=True).clamp_min(1e-300), torch.zeros_like(e))
    rho = torch.where(valid, s_b + yj.abs() * (U32 + ARG32) + EPS_EXP, torch.zeros_like(s))
    rel = rho + (p * rho).sum(-1, keepdim=True) + (d_sum + 4) * U32
    p_b = torch.where(p > 0, p * torch.expm1(rel) + TINY32, torch.zeros_like(p))
    out = {"s": (s, s_b), "p": (p, p_b)}
    if prior is not None:
        pw = p * prior
        den = float(torch.tensor(1e-8, dtype=torch.float32)) + pw.sum(-1, keepdim=True)
        crel = rel + (pw * rel).sum(-1, keepdim=True) / den + (d_sum + 6) * U32
        out["copy"] = (pw / den, torch.where(pw > 0, pw / den * torch.expm1(crel) + TINY32, torch.zeros_like(pw)))
    ctx, ctx_b = torch.empty(B, H, dtype=F64, device=dev), torch.empty(B, H, dtype=F64, device=dev)
    for b0 in range(0, B, nb):
        sl = slice(b0, min(B, b0 + nb))
        ctx[sl] = torch.einsum("bs,bsh->bh", p[sl], mem[sl])
        am = mem[sl].abs()
        ctx_b[sl] = torch.einsum("bs,bsh->bh", p_b[sl], am) + (d_ctx + 2) * U32 * torch.einsum("bs,bsh->bh", p[sl], am)
    out["ctx"] = (ctx, ctx_b)
    return out


def k22_emulate(w, eu, v):
    """K22's scores in float32 on the host (torch's exp and a true division for __expf and v_rcp_f32)."""
    w, eu, v = w.to(torch.float32), eu.to(torch.float32), v.to(torch.float32)
    ew = torch.exp((2.0 * w).clamp(-K22_CLAMP, K22_CLAMP))
    return v.sum() - 2.0 * (v / (ew[:, None, :] * eu + 1.0)).sum(-1)


def k22_midrange(B, S, seed, H=K22_H):
    """(wq [B,H], uh [B,S,H], v [H], mem [B,S,H]) float64: wq, uh normal at 1.5 and rounded to f32, v at 0.3, mem normal rounded to bf16."""
    g = _gen(seed)
    rn = lambda scale, *shape: (torch.randn(shape, generator=g) * scale).to(torch.float32).to(F64)
    return rn(1.5, B, H), rn(1.5, B, S, H), rn(0.3, H), rn(1.0, B, S, H).to(torch.bfloat16).to(F64)


def k22_ternary(B, S, n, seed, H=K22_H):
    """An exact K22 case: wq = 10 sw with random signs, v in {+-1, +-2}.  ``n`` rows of every item (a power of two, scattered by a seeded
    permutation) form the best class: uh = 10 sign(v) where sw = sign(v) (tanh(20) = sign(v): the term is |v|), -wq elsewhere (tanh(0) = 0).
    Every other row is the worst: uh = -10 sign(v) where sw = -sign(v) (the term is -|v|), -wq elsewhere.  The class's score is
    sum_{sw = sign v} |v| (about 384), the others' -sum_{sw = -sign v} |v|: apart by sum |v| >= 512, and e^-512 is 0 in f32 and in float64.
    The rows of a class are the same bits, so their scores are; p is exactly 1 / n on the class and exactly 0 elsewhere, and with integer
    memory rows ctx is the exact class mean (one rounding to bf16).  eu = bf16(e^{+-20}) carries a rounding: the class scores move by
    2^-9 sum |v|, all alike.  -> (wq, uh, v, mem, best [B, S] bool), float64."""
    assert n & (n - 1) == 0 and n <= S
    g = _gen(seed)
    pm = lambda *shape: (torch.randint(0, 2, shape, generator=g) * 2 - 1).to(F64)
    sw, sv = pm(B, H), pm(H)
    v = sv * torch.randint(1, 3, (H,), generator=g).to(F64)
    agree = sw == sv
    top = torch.where(agree, sv.expand(B, H), -sw)      # [B, H]
    low = torch.where(~agree, -sv.expand(B, H), -sw)
    best = torch.zeros(B, S, dtype=torch.bool)
    for b in range(B):
        best[b, torch.randperm(S, generator=g)[:n]] = True
    uh = K7_A * torch.where(best[:, :, None], top[:, None, :], low[:, None, :])
    mem = torch.randint(-V_BOUND, V_BOUND + 1, (B, S, H), generator=g).to(F64)
    return K7_A * sw, uh, v, mem, best
