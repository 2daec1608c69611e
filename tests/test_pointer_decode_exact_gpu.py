"""The cached key exponent (additive_key_exp_kernel) and K22 (pointer_attend_decode_kernel) of csrc/attn_pointer.hip through their C entry
points, on NaN-filled outputs, element by element against tests/exact_inputs.py's float64 restatements.

case_additive_key_exp: the reference is exp(clip(2x, +-43)) of the f32 input; the stored bf16 is within half a bf16 ulp of it, taken in front
of the f32 error of __expf (v_exp_f32 of the log2 e-scaled argument: |2x| ARG + EPS_EXP relative, exact_inputs.key_exp_reference) -- the
_tol form of test_small_ops_gpu.py.

case_pointer_attend_decode: the reference starts from the kernel's OWN inputs -- the bf16 e^{2 uh} it was handed, the f32 sum wq + wq_add,
f32 v, the bf16 value rows, the masks and the prior -- so the bound is f32 arithmetic only (k22_reference derives it for the scores, for p
with the softmax's __expf and normalisation, for copy, and for ctx with its ONE rounding to bf16).  The scores are not an output: their
bound is the first term of p's, and p is what shows them (a wrong row or feature moves a score by |v_h|, a probability by a third).  Masked p and copy and a masked item's
ctx are exact zeros.  One ternary family (k22_ternary) has p exactly 1 / n on its best class and 0 elsewhere, and ctx the exact class
mean."""
import pytest
import torch

import exact_inputs as X
import exact_ledger as L
from exact_ledger import ledger  # noqa: F401  (autouse fixture)
from test_small_ops_gpu import _check, _counting, _misaligned, _nan, _raw, _same_bits, _tol

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
H = X.K22_H


def _note(key, got, ref, bound):
    ratio = float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())
    cur = L._CURRENT[0]
    if cur is not None:
        L.note(key, max(ratio, cur.get("figures", {}).get(key, 0.0)))


def _bounded(name, got, ref, tol, what):
    _check(got, ref, tol, "%s: %s" % (what, name))
    _note("%s: max error / bound" % name, got, ref, tol + torch.zeros_like(ref))
    L.record(0, ref.numel(), "f32 arithmetic on the kernel's own inputs (bound derived in exact_inputs.k22_reference / key_exp_reference)")


# ---------------------------------------------------------------------------------------------------------------------------------
# case_additive_key_exp
# ---------------------------------------------------------------------------------------------------------------------------------
def _key_exp_values(n):
    """A dense sweep over [-25, 25] with the special values planted: the clamp edges +-21.5 with their f32 neighbours, +-50, 0 and -0."""
    x = torch.linspace(-25.0, 25.0, n, dtype=F64).to(F32)
    edge = torch.tensor([21.5, -21.5], dtype=F32)
    inf = torch.tensor(float("inf"), dtype=F32)
    special = torch.cat([edge, torch.nextafter(edge, inf), torch.nextafter(edge, -inf), torch.tensor([50.0, -50.0, 0.0, -0.0], dtype=F32)])
    k = min(n, special.numel())
    x[torch.randperm(n, generator=torch.Generator().manual_seed(n))[:k]] = special[:k]
    return x.to(DEV)


@pytest.mark.parametrize("n", [8, 16, 8 * 257, 8 * (2097152 + 5)], ids=lambda n: "n%d" % n)
def test_key_exp_against_float64(n):
    x = _key_exp_values(n)
    if n >= 16:
        assert all(bool((x == val).any()) for val in (21.5, -21.5, 50.0, -50.0, 0.0))
    if n > 8 * 256 * 32 * 256:
        x[-40:] = torch.linspace(-22.0, 22.0, 40, device=DEV)  # the elements of the grid-stride loop's second round
    eu = _nan(n, dt=BF16)
    with _counting() as calls:
        _raw("case_additive_key_exp", x, eu, n)
    assert calls == {"case_additive_key_exp": 1}
    assert not torch.isnan(eu.float()).any(), "an element was never written"
    ref, f32_err = X.key_exp_reference(x)
    _bounded("eu", eu, ref, _tol(ref, f32_err, BF16), "key exp n %d" % n)
    sat, top = x.abs() >= 21.5, torch.exp(torch.tensor(X.K22_CLAMP, dtype=F64, device=DEV))
    assert torch.equal(eu[sat].double(), torch.where(x[sat] > 0, top, 1.0 / top).to(BF16).double()), "clamped arguments give bf16(e^{+-43})"
    eu2 = _nan(n, dt=BF16)
    _raw("case_additive_key_exp", x, eu2, n)
    _same_bits(eu2, eu, "key exp of a second launch")


def test_key_exp_rejects_ragged_sizes_and_misaligned_pointers():
    x, eu = _key_exp_values(24), _nan(24, dt=BF16)
    for n in (0, 7, 12, 23):
        with pytest.raises(RuntimeError, match="bad argument"):
            _raw("case_additive_key_exp", x, eu, n)
    xm, em = _misaligned(x[:16]), _misaligned(_nan(16, dt=BF16))
    for a, b in ((xm, eu), (x, em), (None, eu), (x, None)):
        with pytest.raises(RuntimeError, match="bad argument"):
            _raw("case_additive_key_exp", a, b, 16)
    torch.cuda.synchronize()
    assert torch.isnan(eu.float()).all() and torch.isnan(em.float()).all(), "a rejected call wrote its output"
    L.record(eu.numel() + em.numel())


# ---------------------------------------------------------------------------------------------------------------------------------
# case_pointer_attend_decode
# ---------------------------------------------------------------------------------------------------------------------------------
def _k22(wq, wq_add, eu, v, mem, cv, rv, prior):
    """The C entry on NaN-filled outputs -> (ctx bf16 [B, H], p, copy | None)."""
    B, S = eu.shape[0], eu.shape[1]
    ctx, p = _nan(B, H, dt=BF16), _nan(B, S)
    copy = _nan(B, S) if prior is not None else None
    u8 = lambda m: None if m is None else m.to(torch.uint8).contiguous()
    with _counting() as calls:
        _raw("case_pointer_attend_decode", wq, wq_add, eu, v, mem, u8(cv), u8(rv), prior, ctx, p, copy, B, S, H)
    assert calls == {"case_pointer_attend_decode": 1}
    for name, t in (("ctx", ctx), ("p", p), ("copy", copy)):
        assert t is None or not torch.isnan(t.float()).any(), "%s has elements the kernel never wrote" % name
    return ctx, p, copy


def _masks(kind, B, S, seed):
    """(col_valid, row_valid) of one of the mask patterns."""
    g = torch.Generator().manual_seed(seed)
    if kind == "none":
        return None, None
    cv = torch.rand(B, S, generator=g) < 0.85
    cv[:, 0] = True
    rv = torch.ones(B, dtype=torch.bool)
    if kind == "group":      # the four rows wave 3 takes in its first round: positions 3, 19, 35, 51
        cv[0, 3:min(S, 52):16] = False
    elif kind == "tail":     # the last valid position is the last position, everything else of the last round of four is masked
        cv[:, max(0, S - 8):] = False
        cv[:, S - 1] = True
    elif kind == "dead":     # an item without a valid position and an invalid target row
        cv[1 % B] = False
        rv[2 % B] = False
    return cv.to(DEV), rv.to(DEV)


K22_CASES = [(3, 1, "random", True), (3, 15, "dead", True), (3, 16, "none", False), (3, 17, "tail", True), (3, 63, "group", False),
             (3, 64, "dead", False), (3, 65, "tail", False), (3, 333, "group", True), (3, 333, "none", True), (2, X.K22_MAX_S, "random", True)]


@pytest.mark.parametrize("B,S,masks,with_prior", K22_CASES, ids=lambda c: str(c))
def test_pointer_attend_decode_against_float64_from_its_own_inputs(B, S, masks, with_prior):
    wq, uh, v, mem = X.k22_midrange(B, S, seed=7 * S + B)
    g = torch.Generator().manual_seed(S)
    part = (torch.randn(B, H, generator=g) * 0.8).to(DEV).to(F32)
    wq, v = wq.to(DEV).to(F32), v.to(DEV).to(F32)
    mem = mem.to(DEV).to(BF16)
    uh = uh.to(DEV).to(F32)
    eu = _nan(B, S, H, dt=BF16)
    _raw("case_additive_key_exp", uh, eu, uh.numel())
    cv, rv = _masks(masks, B, S, seed=S + 1)
    prior = torch.rand(B, S, generator=g).to(DEV).to(F32) if with_prior else None
    wq_add = part if S % 2 else None
    w = (wq + wq_add) if wq_add is not None else wq          # the same f32 addition the kernel makes
    ref = X.k22_reference(w.double(), eu.double(), v.double(), mem.double(), cv, rv, None if prior is None else prior.double())
    ctx, p, copy = _k22(wq, wq_add, eu, v, mem, cv, rv, prior)
    what = "B%d S%d %s" % (B, S, masks)
    _bounded("p", p, ref["p"][0], ref["p"][1], what)
    _bounded("ctx", ctx, ref["ctx"][0], _tol(ref["ctx"][0], ref["ctx"][1], BF16), what)
    if with_prior:
        _bounded("copy", copy, ref["copy"][0], ref["copy"][1], what)
    if cv is not None:
        assert int(torch.count_nonzero(p[~cv])) == 0, what + ": a masked position has a probability"
        assert copy is None or int(torch.count_nonzero(copy[~cv])) == 0, what + ": a masked position has a copy weight"
        dead = ~(cv.any(-1) & rv)
        assert masks != "dead" or B < 3 or int(dead.sum()) == 2
        assert int(torch.count_nonzero(p[dead])) == 0 and int(torch.count_nonzero(ctx[dead].float())) == 0, what + ": a masked item is all zero"
    ctx2, p2, copy2 = _k22(wq, wq_add, eu, v, mem, cv, rv, prior)
    _same_bits(p2, p, what + ": p of a second launch")
    _same_bits(ctx2, ctx, what + ": ctx of a second launch")
    if with_prior:
        _same_bits(copy2, copy, what + ": copy of a second launch")


@pytest.mark.parametrize("B,S,n", [(3, 1, 1), (3, 17, 4), (2, 65, 64), (3, 333, 32), (2, 2048, 1024)], ids=lambda c: str(c))
def test_pointer_attend_decode_is_exact_on_the_ternary_family(B, S, n):
    wq, uh, v, mem, best = X.k22_ternary(B, S, n, seed=S)
    wq, uh, v = [t.to(DEV).to(F32).contiguous() for t in (wq, uh, v)]
    mem, best = mem.to(DEV).to(BF16), best.to(DEV)
    eu = _nan(B, S, H, dt=BF16)
    _raw("case_additive_key_exp", uh, eu, uh.numel())
    cv = torch.ones(B, S, dtype=torch.bool, device=DEV)
    cv[0] = best[0] | (torch.arange(S, device=DEV) % 3 == 0)   # masks on rows outside the class only
    ctx, p, _ = _k22(wq, None, eu, v, mem, cv, None, None)
    want_p = best.double() / n
    assert torch.equal(p.double(), want_p), "p is exactly 1 / %d on the best class and 0 elsewhere; %d elements differ" % (n, int((p.double() != want_p).sum()))
    want_ctx = torch.einsum("bs,bsh->bh", want_p, mem.double())
    _same_bits(ctx, X.round_bf16(want_ctx), "ctx is the exact class mean, rounded once")
    L.record(p.numel() + ctx.numel())


def test_pointer_attend_decode_rejects_what_it_was_not_built_for():
    B, S = 2, 16
    wq, uh, v, mem = X.k22_midrange(B, S, seed=3)
    wq, v = wq.to(DEV).to(F32), v.to(DEV).to(F32)
    eu, mem = torch.exp(2 * uh).to(DEV).to(BF16), mem.to(DEV).to(BF16)
    ctx, p, copy = _nan(B, H, dt=BF16), _nan(B, S), _nan(B, S)
    prior = torch.rand(B, S).to(DEV)
    with pytest.raises(RuntimeError, match=r"\(-2\).*built for H"):
        _raw("case_pointer_attend_decode", wq, None, eu, v, mem, None, None, None, ctx, p, None, 1, X.K22_MAX_S + 1, H)  # rejected by its size alone
    with pytest.raises(RuntimeError, match=r"\(-2\).*built for H"):
        _raw("case_pointer_attend_decode", wq, None, eu, v, mem, None, None, None, ctx, p, None, B, S, 256)
    args = [wq, None, eu, v, mem, None, None, prior, ctx, p, copy]
    for i in (0, 2, 3, 4, 8, 9, 10, 7):  # a null operand or output; copy without prior and prior without copy
        with pytest.raises(RuntimeError, match="bad argument"):
            _raw("case_pointer_attend_decode", *(args[:i] + [None] + args[i + 1:]), B, S, H)
    for dims in ((0, S), (B, 0)):
        with pytest.raises(RuntimeError, match="bad argument"):
            _raw("case_pointer_attend_decode", *args, dims[0], dims[1], H)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _raw("case_pointer_attend_decode", _misaligned(wq), None, eu, v, mem, None, None, prior, ctx, p, copy, B, S, H)
    torch.cuda.synchronize()
    assert torch.isnan(ctx.float()).all() and torch.isnan(p).all() and torch.isnan(copy).all(), "a rejected call wrote an output"
    L.record(ctx.numel() + p.numel() + copy.numel())
