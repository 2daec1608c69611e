"""K8, the dual co-attention as two kernels (csrc/interaction.hip: scores_kernel<3|4>, products_kernel), on operands whose softmaxes are
exact (tests/exact_inputs.py, "K8"; pinned on the CPU by test_exact_inputs_cpu.py): a one-hot class code in a few dimensions of one 64-wide
K group with w3 = 2^10 there makes a score 0 inside the pair's class and -2^20 outside, w1 / w2 = -2^20 on a marker dimension take a few
query columns / passage rows out of one softmax each, the unmarked valid rows of a class are a power of two -- so every entry of A and Bm^T
is exactly 1/n or 0, A1 = A Eq and B1 = Bm^T Ep are exact in f32, and with the kernel's bf16 roundings restated at the points where it
rounds (w3 Eq + w2 in LDS, A1 / B1 / A2 / B2 in tile_to_lds, the four products in mul8) EVERY element of A, Bm^T, G_q_p and G_p_q must have
the restatement's bits; padded rows are exact zeros.

The C entry point is called directly on buffers the test owns: NaN-filled, with one guard pair behind the last that must stay NaN.  Padding
is scattered over the rows, one passage has two valid rows, one query has no valid token.  One case with random inputs compares each of the
ten 512-wide output segments on its own."""
import pytest
import torch

import exact_inputs as X
import exact_ledger as L
from exact_ledger import ledger  # noqa: F401  (autouse fixture)
from test_small_ops_gpu import _counting, _nan, _raw
from test_small_ops_gpu import _same_bits as _same_bits_raw

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
H, LQ = X.K8_H, X.K8_LQ
SEGMENTS = ("E", "1", "2", "E o 1", "E o 2")


@pytest.fixture
def ops():
    import case_rg_amd
    from case_rg_amd import ops
    case_rg_amd.set_compute_dtype(BF16)
    case_rg_amd.set_dropout(False)
    yield ops
    ops.INTERACTION_FUSED = "auto"
    case_rg_amd.set_compute_dtype(F32)


def _same_bits(got, want, what):
    _same_bits_raw(got, want, what)
    L.record(got.numel())


def _direct(Eq, Ep, qv, pv, w, nq):
    """case_interaction_fwd itself on NaN-filled outputs with one guard pair behind the last -> (G_p_q, G_q_p, A, Bm^T) per pair."""
    from case_rg_amd import _abi
    B, P, Lp = Ep.shape[0], Ep.shape[1], Ep.shape[2]
    n = B * P
    d = _abi.InteractionDesc()
    d.n, d.Lp, d.Lq, d.H, d.eq_div, d.dtype = n, Lp, LQ, H, (P if nq != P else 1), _abi.BF16
    a, bt = _nan(n + 1, Lp, LQ, dt=BF16), _nan(n + 1, LQ, Lp, dt=BF16)
    gqp, gpq = _nan(n + 1, Lp, 5 * H, dt=BF16), _nan(n + 1, LQ, 5 * H, dt=BF16)
    with _counting() as calls:
        _raw("case_interaction_fwd", d, Eq, Ep, qv.view(torch.uint8), pv.view(torch.uint8), w, a, bt, gqp, gpq)
    torch.cuda.synchronize()
    assert calls == {"case_interaction_fwd": 1}, calls
    for name, t in (("A", a), ("Bm^T", bt), ("G_q_p", gqp), ("G_p_q", gpq)):
        assert torch.isnan(t[n].float()).all(), "%s: the guard pair behind the last one was written" % name
        assert not torch.isnan(t[:n].float()).any(), "%s: an element was never written" % name
    return gpq[:n], gqp[:n], a[:n], bt[:n]


def _operands(case):
    assert case.Eq.shape == (case.B, case.nq, LQ, H)
    return (case.Eq.to(DEV).to(BF16).contiguous(), case.Ep.to(DEV).to(BF16).contiguous(), case.qv.to(DEV).contiguous(),
            case.pv.to(DEV).contiguous(), case.w.reshape(-1).to(DEV).to(F32).contiguous())


def _check_exact(case, got, what):
    gpq, gqp, a, bt = got
    Eq, Ep, qv, pv = case.pairs(DEV)
    r = X.interaction_restated(Eq, Ep, qv, pv, case.w.to(DEV))
    for name, raw in r["raw"].items():
        if name != "U":
            assert torch.equal(raw.to(F32).to(F64), raw), "%s: the restated %s is not exact in f32" % (what, name)
    _same_bits(a, X.round_bf16(r["raw"]["A"]), what + ": A")
    _same_bits(bt, X.round_bf16(r["raw"]["Bt"]), what + ": Bm^T")
    for k, seg in enumerate(SEGMENTS):  # per segment, so that a failure names it
        _same_bits(gqp[..., k * H:(k + 1) * H], X.round_bf16(r["Gqp"][..., k * H:(k + 1) * H]), "%s: G_q_p segment %s" % (what, seg))
        _same_bits(gpq[..., k * H:(k + 1) * H], X.round_bf16(r["Gpq"][..., k * H:(k + 1) * H]), "%s: G_p_q segment %s" % (what, seg))
    assert int(torch.count_nonzero(gqp[~pv])) == 0 and int(torch.count_nonzero(gpq[~qv])) == 0, what + ": padded rows are exact zeros"
    assert int(torch.count_nonzero(a[~pv])) == 0 and int(torch.count_nonzero(bt[~qv])) == 0
    dead = ~qv.any(-1)  # pairs of a query without a valid token
    if case.B > 1:
        assert dead.any()
        assert int(torch.count_nonzero(a[dead])) == 0 and int(torch.count_nonzero(bt[dead])) == 0, what + ": A = Bm^T = 0 without a valid query token"
        g, e, v = gqp[dead], Ep[dead].to(BF16), pv[dead]
        assert torch.equal(g[..., :H][v], e[v]) and int(torch.count_nonzero(g[..., H:][v].float() != 0)) == 0, what + ": G_q_p = [Ep, 0, 0, 0, 0]"
    return r


def _case_id(c):
    args, kw = c
    return "B%d-P%d-nq%d-Lp%d" % args + "".join("-%s%s" % (k, v) for k, v in kw.items())


@pytest.mark.parametrize("case", X.all_k8_cases(), ids=_case_id)
def test_interaction_fwd_is_exact_in_every_output_bit(ops, case):
    args, kw = case
    c = X.k8(*args, **kw)
    Eq, Ep, qv, pv, w = _operands(c)
    got = _direct(Eq, Ep, qv, pv, w, c.nq)
    r = _check_exact(c, got, _case_id(case))
    if args == X.K8_MANY:
        assert c.B * c.P > torch.cuda.get_device_properties(0).multi_processor_count
    if kw.get("orphan"):  # a class without a counterpart: uniform over all 32 unmarked valid query rows / all 64 unmarked valid passage rows
        assert (r["A"] == 1.0 / 32).any() and (r["Bt"] == 1.0 / 64).any()


def test_the_wrapper_makes_the_same_call(ops):
    """ops.interaction_fwd on the operands of one exact case: the bits of the direct call, through one launch of the entry point."""
    c = X.k8(*X.K8_GEOMETRY[5])  # Lp 384, one query per passage
    Eq, Ep, qv, pv, w = _operands(c)
    want = _direct(Eq, Ep, qv, pv, w, c.nq)
    with _counting() as calls:
        gpq, gqp, a, bt = ops.interaction_fwd(Eq, Ep, qv, pv, w.reshape(1, -1))
    assert calls == {"case_interaction_fwd": 1}, calls
    n = c.B * c.P
    for name, g, t in zip(("G_p_q", "G_q_p", "A", "Bm^T"), (gpq, gqp, a, bt), want):
        _same_bits(g.reshape(t.shape), t, "ops.interaction_fwd vs the direct call: " + name)
    assert gqp.shape == (c.B, c.P, c.Lp, 5 * H) and a.shape == (n, c.Lp, LQ)


def _rel(a, b):
    return ((a.double() - b).norm() / b.norm().clamp_min(1e-300)).item()


def test_random_inputs_segment_by_segment(ops):
    """randn inputs (the distribution of test_interaction_fused_gpu.py), one query per passage, ragged masks with holes: each of the ten
    512-wide segments of G_q_p / G_p_q gets a relative L2 of its own against the float64 restatement with the kernel's rounding points, and
    may be at most 1.5 times what the single launches (INTERACTION_FUSED = "off") show for that segment on the same inputs.  No floor."""
    from case_rg_amd.common.Interaction import Interaction
    B, P, Lp = 2, 3, 384
    g = torch.Generator().manual_seed(20)
    Eq = (torch.randn(B, P, LQ, H, generator=g) * 0.7).to(DEV).to(BF16)
    Ep = (torch.randn(B, P, Lp, H, generator=g) * 0.7).to(DEV).to(BF16)
    qv = (torch.rand(B, P, LQ, generator=g) < 0.85).to(DEV)
    pv = (torch.rand(B, P, Lp, generator=g) < 0.85).to(DEV)
    m = Interaction(H).to(DEV)
    with torch.no_grad():
        m.dual_att_linear.weight.copy_(torch.randn(1, 3 * H, generator=g).to(DEV) * 0.05)
    w = m.dual_att_linear.weight.detach().reshape(-1).contiguous()
    gpq, gqp, a, bt = _direct(Eq, Ep, qv, pv, w, P)
    with torch.no_grad():
        ops.INTERACTION_FUSED = "off"
        with _counting() as calls:
            s_pq, s_qp = m(Eq, Ep, qv, pv)
        ops.INTERACTION_FUSED = "auto"
    assert "case_interaction_fwd" not in calls
    n = B * P
    r = X.interaction_restated(Eq.reshape(n, LQ, H).to(F64), Ep.reshape(n, Lp, H).to(F64), qv.reshape(n, LQ), pv.reshape(n, Lp), w.to(F64))
    figures, failures = {}, []
    for side, got, single, ref in (("G_q_p", gqp, s_qp.reshape(n, Lp, 5 * H), r["Gqp"]), ("G_p_q", gpq, s_pq.reshape(n, LQ, 5 * H), r["Gpq"])):
        for k, seg in enumerate(SEGMENTS):
            sl = slice(k * H, (k + 1) * H)
            e_f, e_s = _rel(got[..., sl], ref[..., sl]), _rel(single[..., sl], ref[..., sl])
            figures["%s [%s]" % (side, seg)] = {"fused": e_f, "single_launches": e_s}
            print("%s segment %-6s rel L2: fused %.3e  single launches %.3e" % (side, seg, e_f, e_s))
            if not e_f <= 1.5 * e_s:
                failures.append((side, seg, e_f, e_s))
    figures["A max abs"] = (a.double() - r["A"]).abs().max().item()
    figures["Bm^T max abs"] = (bt.double() - r["Bt"]).abs().max().item()
    L.note("segments", figures)
    L.record(0, gqp.numel() + gpq.numel(), "random inputs: per-segment relative L2 at most 1.5 x the single launches'")
    assert not failures, failures
