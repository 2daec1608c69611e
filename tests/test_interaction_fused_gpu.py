"""K8 as kernels (round 6, csrc/interaction.hip; reference: common/Interaction.py:32-74): case_interaction_fwd -- scores + both masked
softmaxes in one launch, the four products and the two 5H-wide concatenations in a second -- against (a) an f32 restatement of the
reference's formulas on the same bf16 inputs and (b) the single-launch HIP path it replaces, for one query against P passages and for
P against P, ragged masks (a two-token filler passage, a query row range that is all padding), Lp = 32 .. 512, more pairs than CUs."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, LQ = 512, 64


def _reference(Eq, Ep, qv, pv, w):
    """common/Interaction.py:32-74 in f32 (Eq [n, Lq, H], Ep [n, Lp, H] already expanded per pair)."""
    Eq, Ep = Eq.float(), Ep.float()
    w1, w2, w3 = w[0, :H], w[0, H:2 * H], w[0, 2 * H:]
    U = (Eq @ w1)[:, None, :] + (Ep @ w2)[:, :, None] + (Ep * w3) @ Eq.transpose(1, 2)
    mask = pv[:, :, None] & qv[:, None, :]
    U = U.masked_fill(~mask, float("-inf"))
    A = torch.softmax(U, dim=2).nan_to_num(0.0).masked_fill(~mask, 0.0)
    Bm = torch.softmax(U, dim=1).nan_to_num(0.0).masked_fill(~mask, 0.0)
    A1, B1 = A @ Eq, Bm.transpose(1, 2) @ Ep
    A2, B2 = A @ B1, Bm.transpose(1, 2) @ A1
    Gqp = torch.cat([Ep, A1, A2, Ep * A1, Ep * A2], -1).masked_fill(~pv[:, :, None], 0.0)
    Gpq = torch.cat([Eq, B1, B2, Eq * B1, Eq * B2], -1).masked_fill(~qv[:, :, None], 0.0)
    return Gpq, Gqp, A, Bm.transpose(1, 2)


@pytest.fixture
def bf16_mode():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.bfloat16)
    case_rg_amd.set_dropout(False)
    yield
    case_rg_amd.set_compute_dtype(torch.float32)


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-30)).item()


@pytest.mark.parametrize("B,P,nq,Lp", [(2, 3, 1, 384), (2, 3, 3, 384), (1, 2, 1, 512), (3, 1, 1, 32), (30, 10, 1, 96)])
def test_fused_interaction_matches_the_formulas_and_the_single_launches(bf16_mode, B, P, nq, Lp):
    from case_rg_amd import _abi, ops
    from case_rg_amd.common.Interaction import Interaction
    g = torch.Generator().manual_seed(B * 100 + P * 10 + Lp)
    Eq = (torch.randn(B, nq, LQ, H, generator=g) * 0.7).to(DEV).to(torch.bfloat16)
    Ep = (torch.randn(B, P, Lp, H, generator=g) * 0.7).to(DEV).to(torch.bfloat16)
    qlen = torch.randint(LQ // 2, LQ + 1, (B, nq), generator=g)
    plen = torch.randint(max(2, Lp // 2), Lp + 1, (B, P), generator=g)
    plen[0, P - 1] = 2  # a filler passage: [CLS][SEP] + padding
    qv = (torch.arange(LQ)[None, None, :] < qlen[:, :, None]).to(DEV)
    pv = (torch.arange(Lp)[None, None, :] < plen[:, :, None]).to(DEV)
    if B > 1:
        qv[B - 1, 0, :] = False  # a query without a token: every score of its pairs is masked
    m = Interaction(H).to(DEV)
    with torch.no_grad():
        m.dual_att_linear.weight.copy_(torch.randn(1, 3 * H, generator=g).to(DEV) * 0.05)
    calls = {}
    raw = _abi.call

    def counting(name, *a):
        calls[name] = calls.get(name, 0) + 1
        return raw(name, *a)

    with torch.no_grad():
        _abi.call = counting
        try:
            got_pq, got_qp = m(Eq, Ep, qv, pv)
        finally:
            _abi.call = raw
        assert calls.get("case_interaction_fwd", 0) == 1 and "case_concat5_fwd" not in calls and "case_softmax_fwd" not in calls, calls
        gpq_raw, gqp_raw, A, Bt = ops.interaction_fwd(Eq, Ep, qv, pv, m.dual_att_linear.weight)
        ops.INTERACTION_FUSED = "off"
        try:
            want_pq, want_qp = m(Eq, Ep, qv, pv)
        finally:
            ops.INTERACTION_FUSED = "auto"
    n = B * P
    Eqx = (Eq.expand(-1, P, -1, -1) if nq != P else Eq).reshape(n, LQ, H)
    qvx = (qv.expand(-1, P, -1) if nq != P else qv).reshape(n, LQ)
    rpq, rqp, rA, rBt = _reference(Eqx, Ep.reshape(n, Lp, H), qvx, pv.reshape(n, Lp), m.dual_att_linear.weight.detach())
    assert torch.isfinite(got_qp.float()).all() and torch.isfinite(got_pq.float()).all()
    # probabilities: bf16 outputs of f32 softmaxes over bf16-operand scores
    assert (A.float() - rA).abs().max().item() <= 2e-2 and (Bt.float() - rBt).abs().max().item() <= 2e-2
    # exact zeros where the reference has them (masked rows / columns, all-masked queries)
    assert (A.float()[rA == 0] == 0).all() and (Bt.float()[rBt == 0] == 0).all()
    assert (gqp_raw.reshape(n, Lp, 5 * H).float()[~pv.reshape(n, Lp)] == 0).all() and (gpq_raw.reshape(n, LQ, 5 * H).float()[~qvx] == 0).all()
    e_qp, e_pq = _rel(gqp_raw.reshape(n, Lp, -1), rqp), _rel(gpq_raw.reshape(n, LQ, -1), rpq)
    b_qp = _rel(want_qp.reshape(n, Lp, -1), rqp)
    assert e_qp <= max(1e-2, 1.5 * b_qp) and e_pq <= 1e-2, (e_qp, e_pq, b_qp)
    # the module's outputs (max over passages when one query faces P) against the single launches
    assert _rel(got_qp, want_qp) <= 1e-2 and _rel(got_pq, want_pq) <= 1e-2, (_rel(got_qp, want_qp), _rel(got_pq, want_pq))
    print("fused Interaction B%d P%d nq%d Lp%d: rel L2 vs f32 G_q_p %.2e (single launches %.2e), G_p_q %.2e" % (B, P, nq, Lp, e_qp, b_qp, e_pq))


@pytest.mark.parametrize("nq,through_block", [(1, False), (3, False), (1, True)])
def test_fused_interaction_in_training_matches_the_single_launches_and_f32_autograd(bf16_mode, nq, through_block):
    """Training: the same two forward kernels with the explicit backward (ops.InteractionFn) against the autograd-composed single launches
    and against f32 autograd of the reference's formulas -- gradients of Eq, Ep and the rank-1 weight; ``through_block`` sends G_q_p through
    a TransformerBlock(5H -> H), whose LayerNorm<5H> hands its gradient straight to the pieces (concat5_layer_norm_carry)."""
    from case_rg_amd import _abi, ops
    from case_rg_amd.common.Interaction import Interaction
    from case_rg_amd.common.TransformerBlock import TransformerBlock
    B, P, Lp = 2, 3, 128
    g = torch.Generator().manual_seed(7 + nq)
    Eq0 = (torch.randn(B, nq, LQ, H, generator=g) * 0.7).to(DEV).to(torch.bfloat16)
    Ep0 = (torch.randn(B, P, Lp, H, generator=g) * 0.7).to(DEV).to(torch.bfloat16)
    qv = (torch.arange(LQ)[None, None, :] < torch.randint(LQ // 2, LQ + 1, (B, nq, 1), generator=g)).to(DEV)
    pv = (torch.arange(Lp)[None, None, :] < torch.randint(Lp // 2, Lp + 1, (B, P, 1), generator=g)).to(DEV)
    m = Interaction(H).to(DEV)
    with torch.no_grad():
        m.dual_att_linear.weight.copy_(torch.randn(1, 3 * H, generator=g).to(DEV) * 0.05)
    block = TransformerBlock(8, 5 * H, H).to(DEV).train() if through_block else None
    gq = (torch.randn(B, nq if nq == P else 1, LQ, 5 * H, generator=g)).to(DEV).to(torch.bfloat16)
    gp = (torch.randn(B, P, Lp, 5 * H if not through_block else H, generator=g)).to(DEV).to(torch.bfloat16)

    def run(fused):
        ops.INTERACTION_TRAIN = fused
        calls = []
        raw = _abi.call

        def spy(name, *a):
            calls.append(name)
            return raw(name, *a)

        _abi.call = spy
        try:
            Eq, Ep = Eq0.clone().requires_grad_(), Ep0.clone().requires_grad_()
            m.zero_grad()
            if block is not None:
                block.zero_grad()
            G_p_q, G_q_p = m(Eq, Ep, qv, pv)
            out_p = G_q_p if block is None else block(G_q_p, pv)
            ((G_p_q.float() * gq.float()).sum() + (out_p.float() * gp.float()).sum()).backward()
        finally:
            _abi.call = raw
            ops.INTERACTION_TRAIN = True
        assert ("case_interaction_fwd" in calls) == fused
        if fused and block is not None:
            assert "case_layernorm_bwd_concat5" in calls, "the block's LayerNorm<5H> did not take the fused concatenation backward"
        return Eq.grad.float(), Ep.grad.float(), m.dual_att_linear.weight.grad.float().clone()

    fused, single = run(True), run(False)
    for name, a, b in zip(("dEq", "dEp", "dw"), fused, single):
        assert torch.isfinite(a).all()
        # two bf16 computations with independent roundings; through the block (LayerNorm<5H>, head_dim-320 attention, two Linears) the
        # difference of the two forwards (5e-4 on G) is amplified: measured 4.0e-2 on dEp there, 3-7e-3 without the block
        assert _rel(a, b) <= (8e-2 if through_block else 2e-2), "%s: fused training path vs single launches %.3e" % (name, _rel(a, b))
    if block is None:  # f32 autograd of the formulas on the same bf16 inputs
        n = B * P
        Eq, Ep, w = Eq0.float().requires_grad_(), Ep0.float().requires_grad_(), m.dual_att_linear.weight.detach().float().requires_grad_()
        Eqx = (Eq.expand(-1, P, -1, -1) if nq != P else Eq).reshape(n, LQ, H)
        qvx = (qv.expand(-1, P, -1) if nq != P else qv).reshape(n, LQ)
        rpq, rqp, _, _ = _reference(Eqx, Ep.reshape(n, Lp, H), qvx, pv.reshape(n, Lp), w)
        rpq = rpq.reshape(B, P, LQ, 5 * H)
        if nq != P:
            rpq = rpq.max(dim=1, keepdim=True)[0]
        ((rpq * gq.float()).sum() + (rqp.reshape(B, P, Lp, 5 * H) * gp.float()).sum()).backward()
        for name, a, b, s_ in zip(("dEq", "dEp", "dw"), fused, (Eq.grad, Ep.grad, w.grad), single):
            assert _rel(a, b) <= max(2e-2, 1.5 * _rel(s_, b)), "%s vs f32 autograd: fused %.3e, single launches %.3e" % (name, _rel(a, b), _rel(s_, b))
        print("fused Interaction training nq%d: rel L2 vs f32 autograd  dEq %.2e  dEp %.2e  dw %.2e  (single launches %.2e %.2e %.2e)" % (
            (nq,) + tuple(_rel(a, b) for a, b in zip(fused, (Eq.grad, Ep.grad, w.grad))) + tuple(_rel(a, b) for a, b in zip(single, (Eq.grad, Ep.grad, w.grad)))))


def test_f32_keeps_the_single_launches(bf16_mode):
    """The fused kernels have no f32 form: the parity mode runs the single launches."""
    import case_rg_amd
    from case_rg_amd import _abi
    from case_rg_amd.common.Interaction import Interaction
    m = Interaction(H).to(DEV)
    Eq = torch.randn(1, 1, LQ, H, device=DEV)
    Ep = torch.randn(1, 2, 64, H, device=DEV)
    qv, pv = torch.ones(1, 1, LQ, dtype=torch.bool, device=DEV), torch.ones(1, 2, 64, dtype=torch.bool, device=DEV)
    calls = []
    raw = _abi.call

    def spy(name, *a):
        calls.append(name)
        return raw(name, *a)

    case_rg_amd.set_compute_dtype(torch.float32)
    _abi.call = spy
    try:
        with torch.no_grad():
            m(Eq, Ep, qv, pv)
        assert "case_interaction_fwd" not in calls
    finally:
        _abi.call = raw


def test_training_steps_do_not_keep_their_graphs_alive(bf16_mode):
    """The pieces handed to the block's LayerNorm are outputs of the node that saved G_q_p: hung on G_q_p itself they closed a reference
    cycle (every step's activations stayed allocated, and a hipGraph capture after such steps crashed in hipStreamEndCapture on the stale
    AccumulateGrad nodes).  Allocated memory must be flat from step to step."""
    from case_rg_amd.common.Interaction import Interaction
    from case_rg_amd.common.TransformerBlock import TransformerBlock
    m, block = Interaction(H).to(DEV), TransformerBlock(8, 5 * H, H).to(DEV).train()
    Eq0 = torch.randn(2, 1, LQ, H, device=DEV).to(torch.bfloat16)
    Ep0 = torch.randn(2, 3, 128, H, device=DEV).to(torch.bfloat16)
    qv, pv = torch.ones(2, 1, LQ, dtype=torch.bool, device=DEV), torch.ones(2, 3, 128, dtype=torch.bool, device=DEV)
    seen = []
    for step in range(6):
        Eq, Ep = Eq0.clone().requires_grad_(), Ep0.clone().requires_grad_()
        G_p_q, G_q_p = m(Eq, Ep, qv, pv)
        (block(G_q_p, pv).float().sum() + G_p_q.float().sum()).backward()
        m.zero_grad(), block.zero_grad()
        del Eq, Ep, G_p_q, G_q_p
        torch.cuda.synchronize()
        seen.append(torch.cuda.memory_allocated())
    assert seen[5] == seen[3] == seen[2], seen


@pytest.mark.parametrize("grad", [False, True])
def test_query_count_outside_one_or_p_is_refused(bf16_mode, grad):
    """One query per sample or one per passage: nq = 2 against P = 4 raises as the single launches do (the reference's assertion,
    common/Interaction.py:27) instead of indexing the queries as pair / P; nq = 1 and nq = P keep the fused launch."""
    from case_rg_amd import _abi, ops
    from case_rg_amd.common.Interaction import Interaction
    B, P, Lp = 2, 4, 64
    g = torch.Generator().manual_seed(17)
    m = Interaction(H).to(DEV)
    with torch.no_grad():
        m.dual_att_linear.weight.copy_(torch.randn(1, 3 * H, generator=g).to(DEV) * 0.05)
    Ep = (torch.randn(B, P, Lp, H, generator=g) * 0.7).to(DEV).to(torch.bfloat16).requires_grad_(grad)
    pv = torch.ones(B, P, Lp, dtype=torch.bool, device=DEV)

    def run(nq):
        Eq = (torch.randn(B, nq, LQ, H, generator=g) * 0.7).to(DEV).to(torch.bfloat16).requires_grad_(grad)
        qv = torch.ones(B, nq, LQ, dtype=torch.bool, device=DEV)
        calls = {}
        raw = _abi.call

        def counting(name, *a):
            calls[name] = calls.get(name, 0) + 1
            return raw(name, *a)

        _abi.call = counting
        try:
            with torch.set_grad_enabled(grad):
                out = m(Eq, Ep, qv, pv)
                if grad:
                    (out[0].float().sum() + out[1].float().sum()).backward()
        finally:
            _abi.call = raw
        return out, calls, Eq, qv

    for nq in (1, P):
        out, calls, _, _ = run(nq)
        assert calls.get("case_interaction_fwd", 0) == 1, (nq, calls)
        assert out[0].shape == (B, 1 if nq == 1 else P, LQ, 5 * H) and torch.isfinite(out[1].float()).all()
    with pytest.raises(AssertionError):
        run(2)
    Eq = torch.zeros(B, 2, LQ, H, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="2 queries for 4 passages"):
        ops.interaction_fwd(Eq, Ep.detach(), torch.ones(B, 2, LQ, dtype=torch.bool, device=DEV), pv, m.dual_att_linear.weight)
    assert not ops.interaction_supported(Eq, Ep, False)
