"""Differentiable operators of the MI355X path: thin ``torch.autograd.Function`` shells around the C ABI.

PyTorch is used here for device memory (caching allocator), streams and the autograd tape only; every
arithmetic pass over an activation is a kernel of libcase_hip.so launched through ``_abi`` on the current
stream.  There is no eager fallback: tensors must live on a ROCm device.
"""
import collections
import math
import ctypes as C
import os

import torch
from torch.autograd import Function

from . import _abi as A
from . import config, paramcache

_DT = {torch.float32: A.F32, torch.bfloat16: A.BF16}


def _code(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError("case_rg_amd: unsupported activation dtype %s" % t.dtype)


_raw_stream, _cur_device = getattr(torch._C, "_cuda_getCurrentRawStream", None), getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    # the launch stream of every C-ABI call = torch's current stream on the current device.  torch.cuda.current_stream() builds a Stream
    # object behind four layers of Python (9 us per call, ~1900 calls per step: 6 ms of a 29-ms step at the reference's default geometry);
    # the two C accessors it ends in take 0.3 us
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _ptr(t, offset_elems=0):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("case_rg_amd ops run on the GPU only (got a %s tensor); there is no CPU path" % t.device)
    return t.data_ptr() + offset_elems * t.element_size()


def _drop4(drop):
    """A dropout site as the descriptors take it: (p, seed, offset, state) -- ``state`` is None or the address of the CaseStepState whose
    rng_base the kernels add to ``offset`` (config.next_rng); None / a 3-tuple = arguments only."""
    if drop is None:
        return 0.0, 0, 0, None
    return tuple(drop) if len(drop) == 4 else tuple(drop) + (None,)


def _u8(mask):
    """bool mask -> uint8 view (same storage) or None."""
    if mask is None:
        return None
    m = mask.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


# ----------------------------------------------------------------------------------------------
# parameter casting: fp32 master -> compute dtype, kept in paramcache
# ----------------------------------------------------------------------------------------------
def invalidate_param_cache():
    """Forget every copy derived from the parameters (paramcache.rewritten): the code paths that write through ``.data`` and so leave
    ``_version`` where it was -- ``EMA.apply_shadow`` / ``restore``, ``GradSync.broadcast_parameters``, ``init_params`` -- call this."""
    paramcache.rewritten()


def cast_param(p, dtype):
    """fp32 parameter -> operand of the compute dtype.  bf16 copies of nn.Parameters (and of views of them, e.g. the K/V rows of
    ``in_proj_weight``) are kept in paramcache (the rule is there) under the owning Parameter and the view's geometry.  Temporaries
    (``torch.cat`` of weights, test tensors) are never cached: a freed tensor's address can be handed to a new tensor of the same shape."""
    if p.dtype == dtype:
        return p.detach().contiguous()
    base = getattr(p, "_base", None)
    owner = p if isinstance(p, torch.nn.Parameter) else (base if isinstance(base, torch.nn.Parameter) else None)
    if owner is None:
        return cast(p.detach(), dtype)
    owners, tag = (owner,), paramcache.cast_tag(p, dtype)
    hit = paramcache.peek(owners, tag)
    if hit is not None:
        return hit
    if owner is not p and p.is_contiguous() and owner.is_contiguous():  # a view (K/V rows of in_proj_weight ...): slice the whole-parameter copy if one is live
        whole = paramcache.peek(owners, paramcache.cast_tag(owner, dtype))
        if whole is not None:
            return whole.as_strided(p.shape, p.stride(), p.storage_offset() - owner.storage_offset())
    return paramcache.derived(owners, tag, lambda: cast(p.detach(), dtype))


def rowpad_rows(rows, multiple):
    return -(-int(rows) // int(multiple)) * int(multiple)


def rowpad_wanted(p):
    """The row multiple a caller of ``cast_param_rowpad`` has asked for on this parameter (0: none) -- FusedAdam then keeps its persistent
    operand copy of it inside a padded buffer (``new_rowpad_copy``)."""
    return int(getattr(p, "_case_rowpad_multiple", 0))


def new_rowpad_copy(p, dtype, multiple):
    """An UNFILLED operand copy of the 2-D parameter ``p`` [V, K] as the [:V] prefix view of a zero-initialised [Vp, K] buffer, Vp = V rounded
    up to ``multiple``; the view carries the buffer as ``_case_rowpad_buf``.  A writer of the copy (case_cast, the optimizer kernel) touches the
    first V K elements only, so rows [V, Vp) stay zero for the life of the buffer."""
    buf = torch.zeros(rowpad_rows(p.shape[0], multiple), p.shape[1], dtype=dtype, device=p.device)
    low = buf[:p.shape[0]]
    low._case_rowpad_buf = buf
    return low


def cast_param_rowpad(p, dtype, multiple=256):
    """2-D parameter [V, K] -> its operand copy of ``dtype`` with the rows padded to a multiple of ``multiple``: [Vp, K], rows [V, Vp) zero
    (a GEMM over it runs on whole tiles; the columns / reduction terms it adds are exact zeros).  Kept in paramcache under its own tag and
    dropped with every other copy when the parameters are rewritten.  Where the live cast copy of ``p`` (``cast_param``'s entry: FusedAdam
    installs its persistent one after every step) already sits inside such a buffer, that buffer is the answer and nothing is cast.
    The call also leaves the request on the parameter (``_case_rowpad_multiple``, read by ``rowpad_wanted``): that is how FusedAdam learns,
    before its first step, which persistent copy to allocate padded.  Without such a copy (f32 compute, another optimizer) the padded copy
    is rebuilt -- one zero fill and one cast or copy of [Vp, K] -- after every rewrite of the parameter."""
    if not isinstance(p, torch.nn.Parameter) or p.dim() != 2 or not p.is_contiguous():
        raise TypeError("cast_param_rowpad: a contiguous 2-D nn.Parameter")
    p._case_rowpad_multiple = int(multiple)
    tag = ("rowpad", dtype, int(multiple))
    hit = paramcache.peek((p,), tag)
    if hit is not None:
        return hit
    low = paramcache.peek((p,), paramcache.cast_tag(p, dtype))
    buf = getattr(low, "_case_rowpad_buf", None)
    if buf is not None and buf.shape == (rowpad_rows(p.shape[0], multiple), p.shape[1]) and buf.dtype == dtype and buf.device == p.device:
        return paramcache.install((p,), tag, buf)

    def build():
        low = new_rowpad_copy(p, dtype, multiple)
        if p.dtype == dtype:
            low.copy_(p.detach())
        else:
            A.call("case_cast", _ptr(p), _ptr(low), p.numel(), _code(p), _DT[dtype], _stream())
        return low._case_rowpad_buf
    return paramcache.derived((p,), tag, build)


def cast(x, dtype):
    if x.dtype == dtype:
        return x
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    A.call("case_cast", _ptr(x), _ptr(out), x.numel(), _code(x), _DT[dtype], _stream())
    return out


# ----------------------------------------------------------------------------------------------
# K16 fused encoder chain (inference): out-proj + residual -> LN2 -> FFN1 + GELU -> FFN2 + residual -> next LN1 -> next QKV
# ----------------------------------------------------------------------------------------------
# "auto": the chain runs wherever it is built (bf16, d_model = dim_feedforward = 512, no autograd, no dropout); "off": the
# single-launch path (tests replay the same fixtures under both; A/B measurements)
ENCODER_CHAIN = "auto"


def encoder_chain_supported(x, width, ffn_width, needs_grad):
    return (ENCODER_CHAIN == "auto" and x.is_cuda and x.dtype == torch.bfloat16 and width == 512 and ffn_width == 512
            and not needs_grad)


def _chain_pack(mats):
    """Fragment-ordered bf16 pack of (Wo, W1, W2, Wqkv_next) -- any of them None -- kept in paramcache until one of the parameters changes."""
    def build():
        low = [None if m is None else cast_param(m, torch.bfloat16) for m in mats]
        packed = torch.empty(A.lib.case_encoder_chain_packed_bytes() // 2, dtype=torch.bfloat16, device=next(m for m in mats if m is not None).device)
        A.call("case_encoder_chain_pack", _ptr(low[0]), _ptr(low[1]), _ptr(low[2]), _ptr(low[3]), _ptr(packed), _stream())
        return packed

    return paramcache.derived(mats, "chain", build)


def encoder_chain(variant, x_in, resid, layer, next_layer):
    """One launch of the row-local chain (csrc/encoder_chain.hip).  variant "head": x_in = embedding output, ``next_layer``'s norm1 +
    in-projection -> (s, qkv); "full": x_in = ``layer``'s attention output, resid = its normed input -> (s', qkv') for
    ``next_layer``; "tail": the last layer -> its output.  ``layer`` / ``next_layer`` are TransformerEncoderLayer modules."""
    M = x_in.shape[0] * x_in.shape[1]
    dev = x_in.device
    f32 = lambda p: None if p is None else p.detach()
    lay = None if variant == "head" else layer
    nxt = None if variant == "tail" else next_layer
    packed = _chain_pack((None if lay is None else lay.self_attn.out_proj.weight, None if lay is None else lay.linear1.weight,
                          None if lay is None else lay.linear2.weight, None if nxt is None else nxt.self_attn.in_proj_weight))
    d = A.EncoderChainDesc()
    d.rows, d.width, d.variant = M, 512, {"full": 0, "tail": 1, "head": 2}[variant]
    d.eps_ln2 = 0.0 if lay is None else lay.norm2.eps
    d.eps_ln1_next = 0.0 if nxt is None else nxt.norm1.eps
    s_out = torch.empty(x_in.shape, dtype=torch.bfloat16, device=dev)
    qkv = None if nxt is None else torch.empty(x_in.shape[0], x_in.shape[1], 1536, dtype=torch.bfloat16, device=dev)
    x_in = x_in if x_in.is_contiguous() else x_in.contiguous()
    if resid is not None and not resid.is_contiguous():
        resid = resid.contiguous()
    A.call("case_encoder_chain", d, _ptr(x_in), _ptr(resid), _ptr(packed),
           _ptr(None if lay is None else f32(lay.self_attn.out_proj.bias)), _ptr(None if lay is None else f32(lay.linear1.bias)),
           _ptr(None if lay is None else f32(lay.linear2.bias)), _ptr(None if nxt is None else f32(nxt.self_attn.in_proj_bias)),
           _ptr(None if lay is None else f32(lay.norm2.weight)), _ptr(None if lay is None else f32(lay.norm2.bias)),
           _ptr(None if nxt is None else f32(nxt.norm1.weight)), _ptr(None if nxt is None else f32(nxt.norm1.bias)),
           _ptr(s_out), _ptr(qkv), _stream())
    return s_out, qkv


# ----------------------------------------------------------------------------------------------
# raw GEMM launcher
# ----------------------------------------------------------------------------------------------
# Tiling of the GEMM calls issued from here: 0 = case_gemm's cost model, 128 / 256 = CaseGemmDesc.tile (tests and A/B
# measurements run the same model under both tilings).  Host-side configuration: the library itself holds no state.
GEMM_TILE = 0
# Streams the package itself has put work on beside the caller's (common/heads.run_block_pair), by handle.  A backward pass then runs post-accumulate
# hooks on more than one stream: while this is non-empty, parallel.GradSync._on_grad records an event per gradient and the bucket's gather waits for those.
AUX_STREAMS = {}


# Measurement aid (bench.py): when a list, every launch appends the tile edge case_gemm_tile_for() reports for it.
TILE_TRACE = None
# Fewest (sequence, head) pairs for which the one-workgroup-per-pair decode attention kernel is used (below: split-KV forward)
DECODE_MIN_PAIRS = 192
# Bias gradients of the weight-gradient GEMMs inside the same launch (False: always the separate column-sum pass; A/B measurements)
FUSE_BIAS_GRAD = True


def gemm(a, b, c, M, N, K, lda, ldb, ldc, *, a_off=0, b_off=0, c_off=0, a_kmajor=False, b_kmajor=False,
         batch1=1, batch2=1, sa=(0, 0), sb=(0, 0), sc=(0, 0), alpha=1.0, epilogue=0, bias_col=None, bias_row=None,
         aux=None, aux_out=None, ld_aux=0, saux=(0, 0), split_k=1, drop=None, rowsum_out=None):
    """``rowsum_out`` (weight-gradient calls: k-major contiguous A, ATOMIC epilogue): pre-zeroed f32 [M] that also receives
    sum_k op(A)[m, k], the bias gradient -- inside the same launch when the 256x256 tiling takes the call, else by case_colsum."""
    d = A.GemmDesc()
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.ld_aux = M, N, K, lda, ldb, ldc, ld_aux
    d.batch1, d.batch2 = batch1, batch2
    d.sa1, d.sa2 = sa
    d.sb1, d.sb2 = sb
    d.sc1, d.sc2 = sc
    d.saux1, d.saux2 = saux
    d.a_kmajor, d.b_kmajor = int(a_kmajor), int(b_kmajor)
    d.in_dtype, d.out_dtype = _code(a), _code(c)
    d.tile = GEMM_TILE
    if b.dtype != a.dtype:
        raise TypeError("gemm operands differ in dtype: %s vs %s" % (a.dtype, b.dtype))
    for name, t in (("aux", aux), ("aux_out", aux_out)):  # the kernels read / write these with the INPUT element size
        if t is not None and t.dtype != a.dtype:
            raise TypeError("gemm %s must have the operand dtype %s, got %s" % (name, a.dtype, t.dtype))
    for name, t in (("bias_col", bias_col), ("bias_row", bias_row)):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("gemm %s must be float32, got %s" % (name, t.dtype))
    if drop is not None and drop[0] > 0.0:
        epilogue |= A.EPI_DROPOUT
        d.drop_p, d.seed, d.offset, d.state = _drop4(drop)
    d.epilogue, d.split_k, d.alpha = epilogue, split_k, alpha
    if TILE_TRACE is not None:
        TILE_TRACE.append(A.lib.case_gemm_tile_for(d, _ptr(a, a_off), _ptr(b, b_off), _ptr(c, c_off), _ptr(bias_col), _ptr(aux),
                                                   _ptr(aux_out)))
    if rowsum_out is not None:
        if not (a_kmajor and epilogue == A.EPI_ATOMIC and lda == M and batch1 * batch2 == 1 and a_off == 0):
            raise ValueError("rowsum_out needs an unbatched k-major contiguous A and the bare ATOMIC epilogue")
        if FUSE_BIAS_GRAD and a.dtype == torch.bfloat16 and A.lib.case_gemm_tile_for(d, _ptr(a), _ptr(b, b_off), _ptr(c, c_off), None, None, None) == 256:
            if not _dw_slabs(d, a, b, b_off, c, c_off, rowsum_out):
                A.call("case_gemm_dw_bias", d, _ptr(a), _ptr(b, b_off), _ptr(c, c_off), _ptr(rowsum_out), _stream())
            return c
        A.call("case_colsum", _ptr(a), _ptr(rowsum_out), K, M, _code(a), _stream())
    elif (epilogue == A.EPI_ATOMIC and split_k >= DW_SLAB_MIN_SPLIT and a.dtype == torch.bfloat16 and batch1 * batch2 == 1 and a_off == 0
          and A.lib.case_gemm_tile_for(d, _ptr(a), _ptr(b, b_off), _ptr(c, c_off), None, None, None) == 256 and _dw_slabs(d, a, b, b_off, c, c_off, None)):
        return c
    A.call("case_gemm", d, _ptr(a, a_off), _ptr(b, b_off), _ptr(c, c_off), _ptr(bias_col), _ptr(bias_row), _ptr(aux),
           _ptr(aux_out), _stream())
    return c


# split-K weight gradients with at least this many splits (small outputs, long reductions: the 512 x 512 gradients over 122,880
# tokens run 64) go through per-split slabs + an ordered reduction instead of f32 atomics (case_gemm_dw_slabs); 0 switches it off
DW_SLAB_MIN_SPLIT = int(os.environ.get("CASE_DW_SLAB_MIN_SPLIT", "8"))
DW_SLAB_MAX_BYTES = 256 << 20


def _dw_slabs(d, a, b, b_off, c, c_off, rowsum_out):
    """Run the weight-gradient GEMM described by ``d`` through case_gemm_dw_slabs when it qualifies; False = caller takes the atomic path."""
    if DW_SLAB_MIN_SPLIT <= 0 or d.split_k < DW_SLAB_MIN_SPLIT or d.ldc != d.N:
        return False
    need = A.lib.case_gemm_dw_slab_bytes(d)
    if need <= 0 or need > DW_SLAB_MAX_BYTES:
        return False
    ws = torch.empty(need, dtype=torch.uint8, device=c.device)  # stream-ordered: the caching allocator hands it on after the reduce
    A.call("case_gemm_dw_slabs", d, _ptr(a), _ptr(b, b_off), _ptr(c, c_off), _ptr(rowsum_out), _ptr(ws), need, _stream())
    return True


def _split_for(out_rows, out_cols, k_len, elem_bytes):
    """split-K factor for GEMMs with a small output and a long reduction (weight gradients, the vocabulary projection's
    input gradient).  Outputs that the 256x256 persistent tiling takes (bf16, both extents multiples of 256, K of 64) run one
    workgroup per CU: pick the split whose tile count best fills whole rounds of 256 (minus a small cost per extra split).  Everything else runs
    the 128x128 tiling, 512 workgroups resident at once: the smallest split with >= 1024 workgroups and < 8 % of the last
    round wasted.  Splits keep >= 8 K tiles each, or >= 2 when the output has so few tiles that the chip would otherwise sit
    idle (the decoder's 512 x 512 weight gradients: 16 tiles)."""
    k_tiles = max(1, (k_len * elem_bytes + 127) // 128)
    tiles256 = (out_rows // 256) * (out_cols // 256)
    if elem_bytes == 2 and out_rows % 256 == 0 and out_cols % 256 == 0 and k_len % 64 == 0:
        # an output whose 256-tiles fill ONE round of the persistent grid by themselves (the row-padded vocabulary gradient: 120 x 2 tiles
        # over 1280 rows) is not split: a split only adds the zero fill and the atomics
        cus = max(8, (256 - int(A.lib.case_get_reserved_cus())) // 8 * 8)
        if 0.9 * cus <= tiles256 <= cus:
            return 1
    # (one to three 256-tiles cannot fill the chip even at 64 splits -- the reference's default width 256: a 256 x 256 gradient over 16 000
    #  tokens ran as ONE workgroup, 209 us -- so those go to the small tilings below)
    if (elem_bytes == 2 and out_rows % 256 == 0 and out_cols % 256 == 0 and k_len % 64 == 0 and k_tiles >= 64
            and tiles256 * min(64, k_tiles // 8) >= 230):
        tiles = tiles256
        # rounds of the PERSISTENT grid as it is right now: under data parallelism GradSync keeps 8 CUs for RCCL during the backward pass
        # (case_set_reserved_cus), and splits chosen for 256 workgroups then land just past a round of 248 -- 300 x 5 work items = 6.05
        # rounds, 100 x 5 = 2.02: the forced one-rank group paid 3 ms per step for that alone
        cus = max(8, (256 - int(A.lib.case_get_reserved_cus())) // 8 * 8)
        best, best_score = 1, -1.0
        for split in range(1, 65):
            if split > 1 and k_tiles // split < 8:
                break
            wgs = tiles * split
            eff = wgs / float(((wgs + cus - 1) // cus) * cus)
            # every extra split is another pass over C: slab stores + an ordered reduce at the HBM rate for the small outputs (0.4 % of the launch
            # each), f32 atomics at ~1.3 TB/s for the large ones (1.2 %)
            score = eff - (0.012 if tiles >= 64 else 0.004) * split - (0.5 if wgs < 0.9 * cus else 0.0)
            if score > best_score:
                best, best_score = split, score
        return best
    tiles = ((out_rows + 127) // 128) * ((out_cols + 127) // 128)
    if elem_bytes == 2 and out_rows % 64 == 0 and out_cols % 64 == 0 and k_len % 64 == 0 and tiles < 128:
        # small output (the decoder- / query-side weight gradients): the 64x64 tiling holds <= 10 K tiles per workgroup in LDS and
        # wants about one round of workgroups, <= 512 in all (csrc/gemm_small.inc, case_gemm's choice)
        t64 = (out_rows // 64) * (out_cols // 64)
        need = (k_tiles + 9) // 10
        want = max(need, (256 + t64 - 1) // t64)
        split = min(want, k_tiles, max(need, 512 // t64))
        if (k_tiles + split - 1) // split <= 10 and t64 * split <= 512:
            return max(1, split)
    min_k_tiles = 8 if tiles >= 128 else 2
    best, best_eff = 1, 0.0
    for split in range(1, 65):
        if split > 1 and k_tiles // split < min_k_tiles:
            break
        wgs = tiles * split
        eff = wgs / (((wgs + 511) // 512) * 512.0)
        if wgs >= 1024 and eff >= 0.92:
            return split
        if eff > best_eff + 1e-9:
            best, best_eff = split, eff
    return best


class _ZeroArena:
    """Zero-initialised f32 memory for the gradients of one training step, handed out in slices of ONE fill: the backward pass asked
    for ~330 separately zeroed buffers per step (weight / bias gradients that are accumulated with atomics, LayerNorm and embedding
    gradients), each a 4-microsecond fill launch on a GPU-bound step.  The arena of a step is sized by what the previous step took
    (steps are told apart by paramcache.EPOCH); the first step, and anything beyond the estimate, falls back to
    one allocation per request.  Gradients are views of the arena: it is freed when the last of them dies (zero_grad, or GradSync's
    switch to its bucket views)."""
    ENABLED = os.environ.get("CASE_ZERO_ARENA", "1") != "0"
    ALIGN = 64  # floats: every slice starts on a 256-byte boundary

    def __init__(self):
        self.epoch, self.buf, self.pos, self.served, self.want, self.device = -1, None, 0, 0, 0, None

    def take(self, n, device):
        if not self.ENABLED or not torch.device(device).type == "cuda":
            return torch.zeros(n, dtype=torch.float32, device=device)
        if self.epoch != paramcache.EPOCH or self.device != device:
            self.want = self.served if self.device == device else 0
            self.epoch, self.buf, self.pos, self.served, self.device = paramcache.EPOCH, None, 0, 0, device
        step = (n + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.served += step
        if self.buf is None or self.pos + step > self.buf.numel():
            size = self.want - (self.served - step) if self.buf is None else 0  # the rest of the estimate, once
            if size < step:
                return torch.zeros(n, dtype=torch.float32, device=device)
            self.buf, self.pos = torch.zeros(size, dtype=torch.float32, device=device), 0
        out = self.buf[self.pos:self.pos + n]
        self.pos += step
        return out


_ZEROS = _ZeroArena()


def _zeros_like_shapes(device, *shapes):
    """Zero-initialised f32 tensors for atomically accumulated gradients, carved out of ONE slice of the step's zero arena (one fill
    kernel per step instead of one per gradient).  Each tensor starts on a 16-byte boundary."""
    sizes = [int(torch.Size(sh).numel()) for sh in shapes]
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + 3) // 4 * 4
    flat = _ZEROS.take(total, device)
    return [flat[o:o + n].view(sh) for o, n, sh in zip(offs, sizes, shapes)]


def _weight_grad(g2, x2, N, K, out=None, bias_out=None):
    """dW[N, K] = g2[M, N]^T x2[M, K]  (both operands k-major, f32 atomics across K splits); ``out`` is pre-zeroed.
    ``bias_out`` (pre-zeroed f32 [N]) also receives the bias gradient, the column sums of g2 (see ``gemm(rowsum_out=)``)."""
    M = g2.shape[0]
    dw = out if out is not None else _zeros_like_shapes(g2.device, (N, K))[0]
    split = _split_for(N, K, M, g2.element_size())
    gemm(g2, x2, dw, N, K, M, N, K, K, a_kmajor=True, b_kmajor=True, split_k=split, epilogue=A.EPI_ATOMIC, rowsum_out=bias_out)
    return dw


def _colsum(g2, out=None):
    out = out if out is not None else _zeros_like_shapes(g2.device, (g2.shape[1],))[0]
    A.call("case_colsum", _ptr(g2), _ptr(out), g2.shape[0], g2.shape[1], _code(g2), _stream())
    return out


def _dropout_raw(x, p, seed, offset, state=None):
    y = torch.empty_like(x)
    A.call("case_dropout", _ptr(x), _ptr(y), x.numel(), p, seed, offset, state, _code(x), _stream())
    return y


# ----------------------------------------------------------------------------------------------
# Linear:  y = dropout(x W^T + b) + residual
# ----------------------------------------------------------------------------------------------


def _input_grad(g, wc, M, K, N):
    """dX[M, K] = g[M, N] . W[N, K].  A long reduction over few output tiles (the vocabulary projection: N = 30522 onto
    M x 512) leaves most CUs idle in one pass, so it is split along N into f32 partial sums and cast afterwards."""
    tiles = ((M + 127) // 128) * ((K + 127) // 128)
    if g.dtype == torch.bfloat16 and N >= 4096 and tiles < 256:
        split = _split_for(M, K, N, 2)
        if split > 1:
            acc = _zeros_like_shapes(g.device, (M, K))[0]
            gemm(g, wc, acc, M, K, N, N, K, K, b_kmajor=True, split_k=split, epilogue=A.EPI_ATOMIC)
            return cast(acc, g.dtype)
    dx = torch.empty(M, K, dtype=g.dtype, device=g.device)
    gemm(g, wc, dx, M, K, N, N, K, K, b_kmajor=True)
    return dx


LN_TAIL = os.environ.get("CASE_LN_TAIL", "1") != "0"  # A/B switch: "0" keeps Linear / FFN and the LayerNorm behind them separate ops


def _ln_tail_forward(y2, ln):
    """LayerNorm of the rows y2 [M, N] right behind the GEMM that produced them (same kernel as ops.layer_norm)."""
    gamma, beta, eps = ln
    n = torch.empty_like(y2)
    mean = torch.empty(y2.shape[0], dtype=torch.float32, device=y2.device)
    rstd = torch.empty_like(mean)
    g, b = gamma.detach().contiguous(), beta.detach().contiguous()
    A.call("case_layernorm_fwd", _ptr(y2), None, _ptr(g), _ptr(b), _ptr(n), _ptr(mean), _ptr(rstd), y2.shape[0], y2.shape[1], eps,
           _code(y2), _stream())
    return n, g, mean, rstd


def _ln_tail_backward(dn, y2, g, mean, rstd, drop):
    """Backward of LN(y), y = dropout(z) + r: -> (dy, masked dy, d_gamma, d_beta).  dy is the gradient of y (and of the residual r); the masked
    copy -- what the GEMMs of z's Linear read -- comes out of the SAME kernel when it has a dropout (case_layernorm_bwd_dropout) instead of a
    separate pass over dy."""
    R, C = y2.shape
    dn2 = dn.reshape(R, C)
    dn2 = dn2 if dn2.is_contiguous() else dn2.contiguous()
    if dn2.dtype != y2.dtype:
        dn2 = cast(dn2, y2.dtype)
    dy = torch.empty_like(y2)
    dg, db = _zeros_like_shapes(y2.device, (C,), (C,))
    chunk = 512 if y2.dtype == torch.bfloat16 else 256
    if drop is not None and C % chunk == 0 and C // chunk <= 8:
        gm = torch.empty_like(y2)
        A.call("case_layernorm_bwd_dropout", _ptr(dn2), _ptr(y2), _ptr(g), _ptr(mean), _ptr(rstd), _ptr(dy), _ptr(gm), _ptr(dg), _ptr(db), R, C,
               drop[0], drop[1], drop[2], drop[3], _code(y2), _stream())
        return dy, gm, dg, db
    A.call("case_layernorm_bwd", _ptr(dn2), _ptr(y2), None, _ptr(g), _ptr(mean), _ptr(rstd), _ptr(dy), None, _ptr(dg), _ptr(db), R, C,
           _code(y2), _stream())
    return dy, (_dropout_raw(dy, *drop) if drop is not None else dy), dg, db


class LinearFn(Function):
    """y = dropout(x W^T + b) + residual.  With ``carry`` the input is handed back as a second output: a caller that adds x
    to something computed from y (x + out_proj(attention(in_proj(x)))) takes its residual from that output, and both
    gradients of x then arrive here together -- the sum rides in the epilogue of the dX GEMM instead of a separate add."""

    @staticmethod
    def forward(ctx, x, w, b, residual, p_drop, out_dtype, carry=False, ln_g=None, ln_b=None, ln_eps=0.0):
        """``ln_g`` / ``ln_b`` / ``ln_eps``: a LayerNorm applied to the result (its only consumer); the backward then produces the
        LayerNorm's input gradient and its dropout-masked copy in one kernel (_ln_tail_backward)."""
        K, N = x.shape[-1], w.shape[0]
        x2 = x.reshape(-1, K)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        M = x2.shape[0]
        wc = cast_param(w, x2.dtype)
        y = torch.empty(M, N, dtype=out_dtype or x2.dtype, device=x2.device)
        epi, drop, res2 = 0, None, None
        if b is not None:
            epi |= A.EPI_BIAS_COL
        if p_drop > 0.0:
            drop = (p_drop,) + config.next_rng(M * N)
        if residual is not None:
            res2 = residual.reshape(M, N).contiguous()
            epi |= A.EPI_RESIDUAL
        gemm(x2, wc, y, M, N, K, K, K, N, epilogue=epi, bias_col=b, aux=res2, ld_aux=N, drop=drop)
        ctx.meta = (x.shape, b is not None, residual is not None, drop, w.dtype)
        if ln_g is not None:
            n, g_, mean, rstd = _ln_tail_forward(y, (ln_g, ln_b, ln_eps))
            ctx.save_for_backward(x2, wc, y, g_, mean, rstd)
            return n.view(*x.shape[:-1], N)
        ctx.save_for_backward(x2, wc)
        if carry:
            return y.view(*x.shape[:-1], N), x.view_as(x)
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy, d_carry=None):
        xshape, has_b, has_res, drop, _ = ctx.meta
        d_lng = d_lnb = None
        if len(ctx.saved_tensors) == 6:  # a LayerNorm behind the GEMM: dy arrives as the gradient of its output
            x2, wc, y, g_, mean, rstd = ctx.saved_tensors
            M, K = x2.shape
            N = wc.shape[0]
            dy, g, d_lng, d_lnb = _ln_tail_backward(dy, y, g_, mean, rstd, drop)
            d_res = dy.view(*xshape[:-1], N) if has_res else None
        else:
            x2, wc = ctx.saved_tensors
            M, K = x2.shape
            N = wc.shape[0]
            d_res = dy if has_res else None
            g = cast(dy.reshape(M, N), x2.dtype)
            if not g.is_contiguous():
                g = g.contiguous()
            if drop is not None:
                g = _dropout_raw(g, *drop)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            if d_carry is not None and d_carry.dtype == x2.dtype:
                extra = d_carry.reshape(M, K)
                extra = extra if extra.is_contiguous() else extra.contiguous()
                dx = torch.empty(M, K, dtype=x2.dtype, device=x2.device)
                gemm(g, wc, dx, M, K, N, N, K, K, b_kmajor=True, epilogue=A.EPI_RESIDUAL, aux=extra, ld_aux=K)
                dx = dx.view(xshape)
            else:
                dx = _input_grad(g, wc, M, K, N).view(xshape)
                if d_carry is not None:
                    dx = dx + d_carry.to(dx.dtype)
        want_w, want_b = ctx.needs_input_grad[1], has_b and ctx.needs_input_grad[2]
        if want_w and want_b:
            dw, db = _zeros_like_shapes(g.device, (N, K), (N,))
            _weight_grad(g, x2, N, K, out=dw, bias_out=db)
        elif want_w:
            dw = _weight_grad(g, x2, N, K)
        elif want_b:
            db = _colsum(g)
        return dx, dw, db, d_res, None, None, None, d_lng, d_lnb, None


class RowDotFn(Function):
    """Linear with ONE output feature: y[..., 0] = x . w + b (f32 out)."""

    @staticmethod
    def forward(ctx, x, w, b):
        C = x.shape[-1]
        x2 = x.reshape(-1, C)
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        wv = w.detach().reshape(-1).float().contiguous()
        bv = None if b is None else b.detach().reshape(-1).float().contiguous()
        y = torch.empty(x2.shape[0], dtype=torch.float32, device=x2.device)
        A.call("case_rowdot_fwd", _ptr(x2), _ptr(wv), _ptr(bv), _ptr(y), x2.shape[0], C, _code(x2), _stream())
        ctx.save_for_backward(x2, wv)
        ctx.meta = (x.shape, w.shape, b is not None)
        return y.view(*x.shape[:-1], 1)

    @staticmethod
    def backward(ctx, g):
        x2, wv = ctx.saved_tensors
        xshape, wshape, has_b = ctx.meta
        R, C = x2.shape
        g = g.reshape(-1).float().contiguous()
        dx = torch.empty_like(x2) if ctx.needs_input_grad[0] else None
        dw, db = _zeros_like_shapes(x2.device, (C,), (1,))
        db = db if has_b else None
        A.call("case_rowdot_bwd", _ptr(g), _ptr(x2), _ptr(wv), _ptr(dx), _ptr(dw), _ptr(db), R, C, _code(x2), _stream())
        return (None if dx is None else dx.view(xshape)), dw.view(wshape), db


def linear_carry(x, w, b=None):
    """(x W^T + b, x'): x' is x routed through the op so that a later ``+ x'`` merges its gradient into this op's dX GEMM."""
    return LinearFn.apply(x, w, b, None, 0.0, None, True)


def linear(x, w, b=None, residual=None, p_drop=0.0, out_dtype=None, ln=None):
    """``ln`` = (gamma, beta, eps): LayerNorm of the result, as part of this op (the caller must not use the un-normed result)."""
    if ln is not None:
        if LN_TAIL and out_dtype is None:
            return LinearFn.apply(x, w, b, residual, p_drop, None, False, ln[0], ln[1], ln[2])
        return layer_norm(linear(x, w, b, residual, p_drop, out_dtype), ln[0], ln[1], ln[2])
    if w.shape[0] == 1 and residual is None and p_drop == 0.0 and out_dtype in (None, torch.float32) and (
            out_dtype is torch.float32 or x.dtype == torch.float32):
        return RowDotFn.apply(x, w, b)  # single-output heads: a row dot, not an N = 1 GEMM tile
    return LinearFn.apply(x, w, b, residual, p_drop, out_dtype)


# LayerNorm as the prologue of a small projection (case_gemm_ln): the greedy step's LN -> Linear pairs in one launch.  "on": bf16 rows of
# width 512, a multiple of 64 rows, inference; "off" (the default): layer_norm + linear.  MEASURED FLAT (round 5, B = 256, hipGraph replay of
# the whole greedy pass so that host time does not count): 2.232 ms per cached step without, 2.231 ms with -- the 24 LayerNorm launches it
# removes per step (~4 us of GPU time each outside the profiler) are paid back by the prologue, which serialises DMA -> LayerNorm -> MFMA in
# each of the N / 64 column workgroups of a row tile; eagerly it is 0.06 ms SLOWER (more host work per call).  Built, tested, not the default.
LN_GEMM = os.environ.get("CASE_LN_GEMM", "off")


def ln_gemm_supported(x, out_features):
    return (LN_GEMM == "on" and x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] == 512 and (x.numel() // 512) % 64 == 0
            and out_features % 64 == 0 and not torch.is_grad_enabled() and bool(A.lib.case_abi_features() & A.FEAT_GEMM_LN))


def ln_linear(x, ln, w, b=None, act=None, residual=None):
    """(y, xn): xn = LayerNorm(x; ln = (gamma, beta, eps)), y = act(xn W^T + b) (+ residual) -- one launch where case_gemm_ln applies
    (see ln_gemm_supported), layer_norm + linear otherwise.  ``act``: None | "gelu" | "relu".  No autograd (inference)."""
    gamma, beta, eps = ln
    N = w.shape[0]
    if not ln_gemm_supported(x, N):
        xn = layer_norm(x, gamma, beta, eps)
        if act is not None:
            raise RuntimeError("ln_linear: an activation needs case_gemm_ln (check ln_gemm_supported; ops.ffn is the general path)")
        return linear(xn, w, b, residual=residual), xn
    x2 = x.reshape(-1, 512)
    x2 = x2 if x2.is_contiguous() else x2.contiguous()
    M = x2.shape[0]
    wc = cast_param(w, torch.bfloat16)
    y = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    xn = torch.empty_like(x2)
    d = A.GemmDesc()
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.ld_aux = M, N, 512, 512, 512, N, N
    d.batch1 = d.batch2 = 1
    d.in_dtype, d.out_dtype, d.split_k, d.alpha, d.tile = A.BF16, A.BF16, 1, 1.0, 64
    epi = 0
    if b is not None:
        epi |= A.EPI_BIAS_COL
    if act == "gelu":
        epi |= A.EPI_GELU
    elif act == "relu":
        epi |= A.EPI_RELU
    elif act is not None:
        raise ValueError("ln_linear: activation %r" % (act,))
    res2 = None
    if residual is not None:
        res2 = residual.reshape(M, N)
        res2 = res2 if res2.is_contiguous() else res2.contiguous()
        epi |= A.EPI_RESIDUAL
    d.epilogue = epi
    g32, b32 = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
    A.call("case_gemm_ln", d, _ptr(x2), _ptr(g32), _ptr(b32), float(eps), _ptr(xn), _ptr(wc), _ptr(y), _ptr(None if b is None else b.detach()),
           _ptr(res2), _stream())
    return y.view(*x.shape[:-1], N), xn.view(x.shape)


# ----------------------------------------------------------------------------------------------
# Feed-forward pair:  y = dropout_o(W2 dropout_i(act(W1 x + b1)) + b2) + residual
#   common/TransformerEncoder.py:72-75, TransformerDecoder.py:86-88, TransformerBlock.py:28-29
# ----------------------------------------------------------------------------------------------
class FFNFn(Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, act, p_inner, p_out, residual, ln_g=None, ln_b=None, ln_eps=0.0):
        K, F_, N = x.shape[-1], w1.shape[0], w2.shape[0]
        x2 = x.reshape(-1, K)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        M = x2.shape[0]
        w1c, w2c = cast_param(w1, x2.dtype), cast_param(w2, x2.dtype)
        a = torch.empty(M, F_, dtype=x2.dtype, device=x2.device)
        z = torch.empty_like(a) if act == "gelu" else None
        drop_i = drop_o = None
        if p_inner > 0.0:
            drop_i = (p_inner,) + config.next_rng(M * F_)
        if p_out > 0.0:
            drop_o = (p_out,) + config.next_rng(M * N)
        gemm(x2, w1c, a, M, F_, K, K, K, F_, epilogue=A.EPI_BIAS_COL | (A.EPI_GELU if act == "gelu" else A.EPI_RELU),
             bias_col=b1, aux_out=z, ld_aux=F_, drop=drop_i)
        y = torch.empty(M, N, dtype=x2.dtype, device=x2.device)
        res2, epi = None, A.EPI_BIAS_COL
        if residual is not None:
            res2 = residual.reshape(M, N).contiguous()
            epi |= A.EPI_RESIDUAL
        gemm(a, w2c, y, M, N, F_, F_, F_, N, epilogue=epi, bias_col=b2, aux=res2, ld_aux=N, drop=drop_o)
        # y = x + FFN(x): the residual gradient can ride in the epilogue of the dX GEMM instead of a separate add
        ctx.meta = (x.shape, act, drop_i, drop_o, residual is not None, residual is x and N == K)
        if ln_g is not None:  # a LayerNorm behind the pair (the next layer's norm1): see LinearFn
            n, g_, mean, rstd = _ln_tail_forward(y, (ln_g, ln_b, ln_eps))
            ctx.save_for_backward(x2, w1c, w2c, a, z, y, g_, mean, rstd)
            return n.view(*x.shape[:-1], N)
        ctx.save_for_backward(x2, w1c, w2c, a, z)
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        xshape, act, drop_i, drop_o, has_res, res_is_x = ctx.meta
        d_lng = d_lnb = None
        if len(ctx.saved_tensors) == 9:
            x2, w1c, w2c, a, z, y, g_, mean, rstd = ctx.saved_tensors
            M, K = x2.shape
            F_, N = w1c.shape[0], w2c.shape[0]
            g_res, g, d_lng, d_lnb = _ln_tail_backward(dy, y, g_, mean, rstd, drop_o)
            dy = g_res.view(*xshape[:-1], N)
            fuse_res = res_is_x and ctx.needs_input_grad[0]
            d_res = dy if (has_res and not fuse_res) else None
        else:
            x2, w1c, w2c, a, z = ctx.saved_tensors
            M, K = x2.shape
            F_, N = w1c.shape[0], w2c.shape[0]
            g = dy.reshape(M, N)
            if not g.is_contiguous():
                g = g.contiguous()
            fuse_res = res_is_x and ctx.needs_input_grad[0] and g.dtype == x2.dtype
            d_res = dy if (has_res and not fuse_res) else None
            g_res = g  # the incoming gradient before the output dropout mask is applied
            if drop_o is not None:
                g = _dropout_raw(g, *drop_o)
        dw1, db1, dw2, db2 = _zeros_like_shapes(g.device, (F_, K), (F_,), (N, F_), (N,))
        _weight_grad(g, a, N, F_, out=dw2, bias_out=db2)
        # dz = (g W2) * act'(.) * keep_i/(1-p_i): one GEMM with the derivative (and the regenerated mask) in the epilogue
        dz = torch.empty(M, F_, dtype=x2.dtype, device=x2.device)
        if act == "gelu":
            gemm(g, w2c, dz, M, F_, N, N, F_, F_, b_kmajor=True, epilogue=A.EPI_MUL_DGELU, aux=z, ld_aux=F_, drop=drop_i)
        else:
            gemm(g, w2c, dz, M, F_, N, N, F_, F_, b_kmajor=True, epilogue=A.EPI_MUL_DRELU, aux=a, ld_aux=F_, drop=drop_i)
        _weight_grad(dz, x2, F_, K, out=dw1, bias_out=db1)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(M, K, dtype=x2.dtype, device=x2.device)
            if fuse_res:
                gemm(dz, w1c, dx, M, K, F_, F_, K, K, b_kmajor=True, epilogue=A.EPI_RESIDUAL, aux=g_res, ld_aux=N)
            else:
                gemm(dz, w1c, dx, M, K, F_, F_, K, K, b_kmajor=True)
            dx = dx.view(xshape)
        return dx, dw1, db1, dw2, db2, None, None, None, d_res, d_lng, d_lnb, None


def ffn(x, w1, b1, w2, b2, act, p_inner=0.0, p_out=0.0, residual=None, ln=None):
    """``ln`` = (gamma, beta, eps): LayerNorm of the result as part of this op (see ``linear``)."""
    if ln is not None:
        if LN_TAIL:
            return FFNFn.apply(x, w1, b1, w2, b2, act, p_inner, p_out, residual, ln[0], ln[1], ln[2])
        return layer_norm(FFNFn.apply(x, w1, b1, w2, b2, act, p_inner, p_out, residual), ln[0], ln[1], ln[2])
    return FFNFn.apply(x, w1, b1, w2, b2, act, p_inner, p_out, residual)


# ----------------------------------------------------------------------------------------------
# LayerNorm (optionally of a sum)
# ----------------------------------------------------------------------------------------------
class LayerNormFn(Function):
    """LN(x [+ x2]).  With ``carry`` (x2 must be None) x is handed back as a second output for a residual use
    (x + f(LN(x))): both gradients of x then arrive here and are summed inside the backward kernel."""

    @staticmethod
    def forward(ctx, x, x2, gamma, beta, eps, carry=False):
        C = x.shape[-1]
        xa = x.reshape(-1, C)
        xa = xa if xa.is_contiguous() else xa.contiguous()
        xb = None
        if x2 is not None:
            xb = x2.reshape(-1, C)
            xb = xb if xb.is_contiguous() else xb.contiguous()
        R = xa.shape[0]
        y = torch.empty_like(xa)
        mean = torch.empty(R, dtype=torch.float32, device=xa.device)
        rstd = torch.empty_like(mean)
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        A.call("case_layernorm_fwd", _ptr(xa), _ptr(xb), _ptr(g), _ptr(b), _ptr(y), _ptr(mean), _ptr(rstd), R, C, eps,
               _code(xa), _stream())
        ctx.save_for_backward(xa, xb, g, mean, rstd)
        ctx.shape = x.shape
        if carry:
            return y.view(x.shape), x.view_as(x)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy, d_carry=None):
        xa, xb, g, mean, rstd = ctx.saved_tensors
        R, C = xa.shape
        dy2 = dy.reshape(R, C)
        dy2 = dy2 if dy2.is_contiguous() else dy2.contiguous()
        extra = None
        if d_carry is not None:
            extra = d_carry.reshape(R, C).to(xa.dtype)
            extra = extra if extra.is_contiguous() else extra.contiguous()
        dx = torch.empty_like(xa)
        dg, db = _zeros_like_shapes(xa.device, (C,), (C,))
        A.call("case_layernorm_bwd", _ptr(dy2), _ptr(xa), _ptr(xb), _ptr(g), _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(extra),
               _ptr(dg), _ptr(db), R, C, _code(xa), _stream())
        dx = dx.view(ctx.shape)
        return dx, (dx if xb is not None else None), dg, db, None, None


def layer_norm(x, gamma, beta, eps=1e-5, add=None):
    return LayerNormFn.apply(x, add, gamma, beta, eps)


def layer_norm_carry(x, gamma, beta, eps=1e-5):
    """(LN(x), x'): take a later residual ``+ x`` from x' and its gradient is summed inside the LayerNorm backward kernel."""
    return LayerNormFn.apply(x, None, gamma, beta, eps, True)


# ----------------------------------------------------------------------------------------------
# masked softmax over the last dim of a [outer, inner, R, C] view
# ----------------------------------------------------------------------------------------------
def _softmax_desc(outer, inner, R, C, causal, in_dt, out_dt, drop):
    d = A.SoftmaxDesc()
    d.outer, d.inner, d.R, d.C = outer, inner, R, C
    d.causal, d.in_dtype, d.out_dtype = int(causal), in_dt, out_dt
    d.drop_p, d.seed, d.offset, d.state = _drop4(drop)
    return d


class SoftmaxFn(Function):
    @staticmethod
    def forward(ctx, x, col_valid, row_valid, outer, causal, p_drop, out_dtype):
        """x [..., R, C]; col_valid [outer, C] / row_valid [outer, R] uint8 or None; leading dims = outer*inner."""
        R, C = x.shape[-2], x.shape[-1]
        xc = x if x.is_contiguous() else x.contiguous()
        inner = xc.numel() // (outer * R * C)
        odt = out_dtype or xc.dtype
        p = torch.empty(xc.shape, dtype=odt, device=xc.device)
        drop, y = None, p
        if p_drop > 0.0:
            drop = (p_drop,) + config.next_rng(xc.numel())
            y = torch.empty_like(p)
        d = _softmax_desc(outer, inner, R, C, causal, _code(xc), _DT[odt], drop)
        A.call("case_softmax_fwd", d, _ptr(xc), _ptr(col_valid), _ptr(row_valid), _ptr(p), _ptr(y), _stream())
        ctx.save_for_backward(p)
        ctx.meta = (outer, inner, R, C, causal, xc.dtype, odt, drop)
        return y

    @staticmethod
    def backward(ctx, dy):
        (p,) = ctx.saved_tensors
        outer, inner, R, C, causal, idt, odt, drop = ctx.meta
        dyc = cast(dy, odt)
        dyc = dyc if dyc.is_contiguous() else dyc.contiguous()
        dx = torch.empty(p.shape, dtype=idt, device=p.device)
        d = _softmax_desc(outer, inner, R, C, causal, _DT[idt], _DT[odt], drop)
        A.call("case_softmax_bwd", d, _ptr(dyc), _ptr(p), _ptr(dx), _stream())
        return dx, None, None, None, None, None, None


def masked_softmax(x, col_valid=None, row_valid=None, outer=1, causal=False, p_drop=0.0, out_dtype=None):
    return SoftmaxFn.apply(x, _u8(col_valid), _u8(row_valid), outer, causal, p_drop, out_dtype)


# ----------------------------------------------------------------------------------------------
# Multi-head attention core on packed projections (K4 / K5 / K6)
#   S = alpha Q K^T -> masked softmax (+dropout) -> O = P V, heads addressed in place by batch strides.
# ----------------------------------------------------------------------------------------------
def _src_key(t):
    """Identity of a projection tensor passed in several roles (packed QKV): two different tensors can share a base address."""
    return (t.data_ptr(), tuple(t.shape), tuple(t.stride()))


# Which attention path runs:
#   "auto"    per head size, whichever measured faster on MI355X (tools/attn_bench.py, profiles/r02_attn_bench.jsonl):
#             head_dim 32 / 64 / 96 / 160 fused forward + backward; head_dim 320 / 480 (the 5H blocks) fused forward only when no
#             backward will follow (their fused backward recomputes S in three kernels and is slower than four batched GEMMs
#             over saved probabilities), otherwise GEMM + softmax + GEMM
#   "fused"   the fused kernels wherever they are built (32, 64, 96, 160, 320, 480: forward and backward)
#   "unfused" never fused (tests run the production-shape fixtures under both)
ATTENTION_MODE = "auto"
SCORES_FUSED = os.environ.get("CASE_SCORES_FUSED", "1") != "0"  # the GEMM + softmax + GEMM path keeps its scores in the score GEMM's accumulators where K17 covers the shape
_FUSED_TRAINING = (32, 64, 96, 160)   # 32 / 160: hidden 256 (the reference's default), round 5
_FUSED_INFERENCE = (32, 64, 96, 160, 320)
# head_dim 320 in INFERENCE where K17 covers the shape (Lk <= 384): "slab" (default) = the fused flash-style forward (fas_fwd_kernel, f32
# probabilities inside the kernel); "scores" = K17's score kernel + product, what training runs.  A/B at B 256 (the greedy pass's encode
# phase, two runs each on one box, round 5): 194.0 / 195.0 ms with the slab kernel, 190.2 / 191.0 ms with K17 (+1 % answers/s) -- NOT
# taken: K17 rounds the probabilities to bf16 before the product and the passage-selection logits of prod_case_test [bf16_auto] then sit
# 3.08e-2 from the reference against 2.2e-2 with the slab kernel (bar 3e-2): one per cent of throughput does not buy a wider parity bar.
INFER_320 = os.environ.get("CASE_INFER_320", "slab")


def _fused_ok(q_src, k_src, v_src, q_off, k_off, v_off, d, needs_grad=True):
    if ATTENTION_MODE == "unfused" or q_src.dtype != torch.bfloat16 or not A.lib.case_attention_supported(d):
        return False
    if ATTENTION_MODE == "auto":
        if d not in (_FUSED_TRAINING if needs_grad else _FUSED_INFERENCE):
            return False
        if not needs_grad and d == 320 and INFER_320 == "scores" and SCORES_FUSED and k_src.shape[1] <= 384 and k_src.shape[1] % 8 == 0:
            return False
    for t, off in ((q_src, q_off), (k_src, k_off), (v_src, v_off)):
        if t.shape[2] % 8 or off % 8 or t.data_ptr() % 16:
            return False
    return True


def _kv_splits(N, heads, Lq, Lk, causal):
    """Key chunks for the split-KV forward: only when the plain launch would leave most of the 256 CUs idle (few sequences x
    heads x query tiles) and the memory is long enough to cut into chunks of >= 1024 keys."""
    wgs = N * heads * ((Lq + 127) // 128)
    if causal or wgs >= 512 or Lk < 2048:
        return 1
    # chunks of ~1000 keys, 512 .. 1024 workgroups in all (tools/ksplit_sweep.py: 32 x 8 pairs over 3840 keys 0.089 -> 0.065 ms with 4 chunks,
    # 4 x 8 pairs over 20 480 keys best at 16)
    return max(1, min(Lk // 960, (512 + wgs - 1) // wgs * (2 if wgs >= 128 else 1), 64))


def _attn_desc(N, heads, Lq, Lk, d, q_src, k_src, v_src, causal, alpha, drop):
    ad = A.AttnDesc()
    ad.N, ad.heads, ad.Lq, ad.Lk, ad.head_dim = N, heads, Lq, Lk, d
    ad.ldq, ad.ldk, ad.ldv = q_src.shape[2], k_src.shape[2], v_src.shape[2]
    ad.sq, ad.sk, ad.sv = Lq * q_src.shape[2], Lk * k_src.shape[2], Lk * v_src.shape[2]
    ad.ldo, ad.so = heads * d, Lq * heads * d
    ad.causal, ad.scale = int(causal), alpha
    ad.drop_p, ad.seed, ad.offset, ad.state = _drop4(drop)
    return ad


class AttentionFn(Function):
    @staticmethod
    def forward(ctx, q_src, k_src, v_src, q_off, k_off, v_off, heads, d, key_valid, causal, p_drop, add_mask=None):
        """*_src: [N, L, W] contiguous tensors holding the projections at column offset *_off (width heads*d);
        the same tensor may be passed for several roles (packed QKV).  key_valid uint8 [N, Lk] or None.
        bf16 with a built head size runs the fused kernel (no score tensor); otherwise GEMM + softmax + GEMM.
        ``add_mask`` f32 [Lq, Lk]: an ARBITRARY additive attention mask (nn.MultiheadAttention's attn_mask / memory_mask; no caller on the
        CaSE / Masque path uses one): added to the f32 scores between the score GEMM and the softmax -- the GEMM + softmax + GEMM path only."""
        N, Lq, _ = q_src.shape
        Lk = k_src.shape[1]
        dt, dev = q_src.dtype, q_src.device
        E = heads * d
        alpha = 1.0 / math.sqrt(d)
        drop = (p_drop,) + config.next_rng(N * heads * Lq * Lk) if p_drop > 0.0 else None
        O = torch.empty(N, Lq, E, dtype=dt, device=dev)
        fused = add_mask is None and _fused_ok(q_src, k_src, v_src, q_off, k_off, v_off, d, any(ctx.needs_input_grad[:3]))
        if (fused and Lq == 1 and not causal and drop is None and not any(ctx.needs_input_grad[:3]) and N * heads >= DECODE_MIN_PAIRS
                and A.lib.case_attention_decode_supported(d)):
            # greedy decode step: one query per sequence against the cached keys / values -- the streaming kernel (no LSE: nothing
            # to differentiate); few (sequence, head) pairs with a long memory keep the split-KV forward below
            ad = _attn_desc(N, heads, Lq, Lk, d, q_src, k_src, v_src, causal, alpha, None)
            A.call("case_attention_decode", ad, _ptr(q_src, q_off), _ptr(k_src, k_off), _ptr(v_src, v_off), _ptr(key_valid), _ptr(O),
                   _stream())
            ctx.meta = None
            return O
        if fused:
            lse = torch.empty(N, heads, Lq, dtype=torch.float32, device=dev)
            ad = _attn_desc(N, heads, Lq, Lk, d, q_src, k_src, v_src, causal, alpha, drop)
            ksplit = _kv_splits(N, heads, Lq, Lk, causal)
            if ksplit > 1:
                # long memory, few (sequence, head) pairs: cut the key range over workgroups (flash-decoding style merge)
                need = A.i64(0)
                A.call("case_attention_splitkv_workspace", ad, ksplit, need)
                ws = torch.empty(need.value // 4, dtype=torch.float32, device=dev)
                A.call("case_attention_fwd_splitkv", ad, _ptr(q_src, q_off), _ptr(k_src, k_off), _ptr(v_src, v_off), _ptr(key_valid),
                       _ptr(O), _ptr(lse), _ptr(ws), need.value, ksplit, _stream())
            else:
                A.call("case_attention_fwd", ad, _ptr(q_src, q_off), _ptr(k_src, k_off), _ptr(v_src, v_off), _ptr(key_valid), _ptr(O),
                       _ptr(lse), _stream())
            ctx.save_for_backward(q_src, k_src, v_src, key_valid, O, lse)
        else:
            S, Pd = AttentionFn._probabilities(q_src, k_src, q_off, k_off, heads, d, key_valid, causal, drop, alpha, add_mask)
            if not AttentionFn._product(Pd, v_src, v_off, O, 0, heads, d, Lq, Lk, False):
                gemm(Pd, v_src, O, Lq, d, Lk, Lk, v_src.shape[2], E, b_off=v_off, b_kmajor=True, batch1=N, batch2=heads,
                     sa=(heads * Lq * Lk, Lq * Lk), sb=(Lk * v_src.shape[2], d), sc=(Lq * E, d))
            ctx.save_for_backward(q_src, k_src, v_src, key_valid, S, Pd if drop is not None else None)
        ctx.meta = (q_off, k_off, v_off, heads, d, causal, drop, alpha, fused)
        return O

    @staticmethod
    def _grad_buffers(q_src, k_src, v_src, E):
        """One gradient buffer per distinct source tensor (packed projections share one)."""
        bufs = {}
        for src in (q_src, k_src, v_src):
            key = _src_key(src)
            if key not in bufs:
                covered = sum(E for t in (q_src, k_src, v_src) if _src_key(t) == key)
                bufs[key] = torch.empty_like(src) if covered == src.shape[2] else torch.zeros_like(src)
        return bufs

    @staticmethod
    def _fused_backward(ctx, dO):
        q_src, k_src, v_src, key_valid, O, lse = ctx.saved_tensors
        q_off, k_off, v_off, heads, d, causal, drop, alpha, _ = ctx.meta
        N, Lq, _ = q_src.shape
        Lk = k_src.shape[1]
        dO = dO if dO.is_contiguous() else dO.contiguous()
        bufs = AttentionFn._grad_buffers(q_src, k_src, v_src, heads * d)
        gq, gk, gv = bufs[_src_key(q_src)], bufs[_src_key(k_src)], bufs[_src_key(v_src)]
        ad = _attn_desc(N, heads, Lq, Lk, d, q_src, k_src, v_src, causal, alpha, drop)
        delta = torch.empty(A.lib.case_attention_bwd_scratch_floats(ad), dtype=torch.float32, device=dO.device)
        A.call("case_attention_bwd", ad, _ptr(q_src, q_off), _ptr(k_src, k_off), _ptr(v_src, v_off), _ptr(key_valid), _ptr(O), _ptr(lse),
               _ptr(dO), _ptr(delta), _ptr(gq, q_off), _ptr(gk, k_off), _ptr(gv, v_off), _stream())
        out, seen = [], set()
        for src in (q_src, k_src, v_src):
            key = _src_key(src)
            out.append(None if key in seen else bufs[key])
            seen.add(key)
        return (out[0], out[1], out[2]) + (None,) * 9

    @staticmethod
    def _scores_fused(a_src, b_src, a_off, b_off, heads, d, Lq, Lk, causal):
        """K17 covers this product (bf16, head_dim % 64 == 0 and >= 128, Lk <= 384, Lk % 8 == 0, no causal mask, 16-byte aligned slices)."""
        if not SCORES_FUSED or a_src.dtype != torch.bfloat16 or causal or d % 64 or d < 128 or Lk > 384 or Lk % 8:
            return False
        return all(t.shape[2] % 8 == 0 and off % 8 == 0 and t.data_ptr() % 16 == 0 for t, off in ((a_src, a_off), (b_src, b_off)))

    @staticmethod
    def _product(mat, b_src, b_off, out, c_off, heads, d, M, Kc, transposed, alpha=1.0):
        """out[n, row, head, :] = alpha * sum_k A[n, head][row, k] b[n, k, head, :], A = mat [N, heads, La, Lb] or its transpose (K17's
        row-complete product kernel at head_dim 320); False when the shape is outside its scope (the caller runs case_gemm)."""
        if not SCORES_FUSED or mat.dtype != torch.bfloat16:
            return False
        N, _, La, Lb = mat.shape
        pd = A.AttnProductDesc()
        pd.N, pd.heads, pd.M, pd.Kc, pd.head_dim = N, heads, M, Kc, d
        pd.lda, pd.sa_seq, pd.sa_head = Lb, heads * La * Lb, La * Lb
        pd.ldb, pd.sb_seq, pd.sb_head = b_src.shape[2], b_src.shape[1] * b_src.shape[2], d
        pd.ldc, pd.sc_seq, pd.sc_head = out.shape[2], out.shape[1] * out.shape[2], d
        pd.a_transposed, pd.alpha = int(transposed), alpha
        # the library's own shape query, then a mirror of case_attention_product's stride / alignment / 32-bit-offset requirements:
        # outside them the caller runs case_gemm instead of getting a RuntimeError
        if not A.lib.case_attention_product_supported(pd):
            return False
        strides = (pd.lda, pd.ldb, pd.ldc, pd.sa_seq, pd.sa_head, pd.sb_seq, pd.sb_head, pd.sc_seq, pd.sc_head)
        if any(v % 8 for v in strides) or b_off % 8 or c_off % 8 or any(t.data_ptr() % 16 for t in (mat, b_src, out)):
            return False
        a_rows = Kc if transposed else M
        if pd.lda < (M if transposed else Kc) or a_rows * pd.lda * 2 >= 1 << 31 or Kc * pd.ldb * 2 >= 1 << 31 or (M + 127) * pd.ldc * 2 >= 1 << 31:
            return False
        A.call("case_attention_product", pd, _ptr(mat), _ptr(b_src, b_off), _ptr(out, c_off), _stream())
        return True

    @staticmethod
    def _probabilities(q_src, k_src, q_off, k_off, heads, d, key_valid, causal, drop, alpha, add_mask=None):
        """P = softmax(alpha Q K^T | masks) [N, h, Lq, Lk] and its dropped-out copy (same tensor when drop is None).
        The scores are kept in f32 between the GEMM and the softmax: a bf16 score of magnitude 16 carries an absolute error of
        0.06, i.e. 6 % on its probability (measured: 4-5 % L2 error on the block gradients at head_dim 320 / 480 with bf16
        scores against 0.5 % with f32 ones)."""
        N, Lq, _ = q_src.shape
        Lk = k_src.shape[1]
        dt = q_src.dtype
        if add_mask is None and AttentionFn._scores_fused(q_src, k_src, q_off, k_off, heads, d, Lq, Lk, causal):
            # K17: the softmax rides in the score GEMM (a workgroup holds whole rows): no f32 score tensor
            P = torch.empty(N, heads, Lq, Lk, dtype=dt, device=q_src.device)
            Pd = torch.empty_like(P) if drop is not None else P
            ad = _attn_desc(N, heads, Lq, Lk, d, q_src, k_src, k_src, causal, alpha, drop)
            A.call("case_attention_scores_fwd", ad, _ptr(q_src, q_off), _ptr(k_src, k_off), _ptr(key_valid), _ptr(P),
                   _ptr(Pd) if drop is not None else None, _stream())
            return P, Pd
        S = torch.empty(N, heads, Lq, Lk, dtype=torch.float32, device=q_src.device)
        gemm(q_src, k_src, S, Lq, Lk, d, q_src.shape[2], k_src.shape[2], Lk, a_off=q_off, b_off=k_off, batch1=N, batch2=heads,
             sa=(Lq * q_src.shape[2], d), sb=(Lk * k_src.shape[2], d), sc=(heads * Lq * Lk, Lq * Lk), alpha=alpha)
        if add_mask is not None:
            # glue: a broadcast add on the f32 scores (off the CaSE / Masque path); a 3-D mask is torch's per-head form [N * heads, Lq, Lk]
            S.add_(add_mask.to(torch.float32).reshape((1, 1, Lq, Lk) if add_mask.dim() == 2 else (S.shape[0], heads, Lq, Lk)))
        P = S if dt == torch.float32 else torch.empty(N, heads, Lq, Lk, dtype=dt, device=q_src.device)
        Pd = torch.empty_like(P) if drop is not None else P
        sd = _softmax_desc(N, heads, Lq, Lk, causal, A.F32, _DT[dt], drop)
        A.call("case_softmax_fwd", sd, _ptr(S), _ptr(key_valid), None, _ptr(P), _ptr(Pd), _stream())  # f32 mode: in place
        return P, Pd

    @staticmethod
    def backward(ctx, dO):
        q_off, k_off, v_off, heads, d, causal, drop, alpha, fused = ctx.meta
        if fused and A.lib.case_attention_bwd_supported(d):
            return AttentionFn._fused_backward(ctx, dO)
        if fused:
            q_src, k_src, v_src, key_valid, _, _ = ctx.saved_tensors
            P, Pd = AttentionFn._probabilities(q_src, k_src, q_off, k_off, heads, d, key_valid, causal, drop, alpha)
        else:
            q_src, k_src, v_src, key_valid, P, Pd = ctx.saved_tensors
            if Pd is None:
                Pd = P
        N, Lq, Wq = q_src.shape
        Lk, Wk, Wv = k_src.shape[1], k_src.shape[2], v_src.shape[2]
        E = heads * d
        dt, dev = q_src.dtype, q_src.device
        dO = dO if dO.is_contiguous() else dO.contiguous()
        pstr = (heads * Lq * Lk, Lq * Lk)
        # one gradient buffer per distinct source tensor; slices are written in place by the GEMMs
        bufs = {}

        def grad_of(src):
            key = _src_key(src)
            if key not in bufs:
                covered = sum(E for s in (q_src, k_src, v_src) if _src_key(s) == key)
                bufs[key] = (torch.empty_like(src) if covered == src.shape[2] else torch.zeros_like(src))
            return bufs[key]

        gq, gk, gv = grad_of(q_src), grad_of(k_src), grad_of(v_src)
        # dV = Pd^T dO
        if not AttentionFn._product(Pd, dO, 0, gv, v_off, heads, d, Lk, Lq, True):
            gemm(Pd, dO, gv, Lk, d, Lq, Lk, E, Wv, c_off=v_off, a_kmajor=True, b_kmajor=True, batch1=N, batch2=heads,
                 sa=pstr, sb=(Lq * E, d), sc=(Lk * Wv, d))
        dP = torch.empty(N, heads, Lq, Lk, dtype=dt, device=dev)
        if AttentionFn._scores_fused(dO, v_src, 0, v_off, heads, d, Lq, Lk, causal):
            # K17: dS = softmax'(dO V^T) with the row sums in the GEMM's epilogue (dP itself is never written)
            ad = _attn_desc(N, heads, Lq, Lk, d, q_src, k_src, v_src, causal, alpha, drop)
            A.call("case_attention_scores_bwd", ad, _ptr(dO), _ptr(v_src, v_off), _ptr(P), _ptr(dP), _stream())
        else:
            # dP = dO V^T
            gemm(dO, v_src, dP, Lq, Lk, d, E, Wv, Lk, b_off=v_off, batch1=N, batch2=heads, sa=(Lq * E, d), sb=(Lk * Wv, d), sc=pstr)
            # dS = softmax'(dP) in place
            sd = _softmax_desc(N, heads, Lq, Lk, causal, _DT[dt], _DT[dt], drop)
            A.call("case_softmax_bwd", sd, _ptr(dP), _ptr(P), _ptr(dP), _stream())
        # dQ = alpha dS K ; dK = alpha dS^T Q
        if not AttentionFn._product(dP, k_src, k_off, gq, q_off, heads, d, Lq, Lk, False, alpha):
            gemm(dP, k_src, gq, Lq, d, Lk, Lk, Wk, Wq, b_off=k_off, c_off=q_off, b_kmajor=True, batch1=N, batch2=heads,
                 sa=pstr, sb=(Lk * Wk, d), sc=(Lq * Wq, d), alpha=alpha)
        if not AttentionFn._product(dP, q_src, q_off, gk, k_off, heads, d, Lk, Lq, True, alpha):
            gemm(dP, q_src, gk, Lk, d, Lq, Lk, Wq, Wk, b_off=q_off, c_off=k_off, a_kmajor=True, b_kmajor=True, batch1=N,
                 batch2=heads, sa=pstr, sb=(Lq * Wq, d), sc=(Lk * Wk, d), alpha=alpha)
        out, seen = [], set()
        for src in (q_src, k_src, v_src):
            key = _src_key(src)
            out.append(None if key in seen else bufs[key])
            seen.add(key)
        return (out[0], out[1], out[2]) + (None,) * 9


# K21: the greedy step's cross-attention over a long memory on the RAW memory rows with absorbed K / V projections (csrc/attn_mqa.hip).
# "auto": bf16, width 512, 8 heads, memories of >= DECODE_ABSORB_MIN_KEYS keys, inference; "off": the cached K / V projections (K13).
DECODE_ABSORB = os.environ.get("CASE_DECODE_ABSORB", "auto")
DECODE_ABSORB_MIN_KEYS = 1024


def decode_absorb_supported(memory, embed_dim, heads):
    return (DECODE_ABSORB != "off" and torch.is_tensor(memory) and memory.is_cuda and memory.dtype == torch.bfloat16 and memory.dim() == 3
            and embed_dim == 512 and heads == 8 and memory.shape[2] == 512 and memory.shape[1] >= DECODE_ABSORB_MIN_KEYS
            and not torch.is_grad_enabled()  # raw-pointer launches without an autograd Function: inference under no_grad only
            and bool(A.lib.case_abi_features() & A.FEAT_ATTN_DECODE_MQA))


def attention_decode_mqa(qp, memory, key_valid=None):
    """qp [B, 8 * 512] bf16: per head the absorbed query log2(e) / sqrt(d) * Wk_h^T q_h; memory [B, S, 512] bf16 (keys AND values);
    key_valid [B, S] bool -> [B, 8 * 512] bf16, head h's context sum_j p_hj memory_j at columns 512 h .. (no autograd: inference)."""
    B, S, E = memory.shape
    if qp.dtype != torch.bfloat16 or memory.dtype != torch.bfloat16 or E != 512 or qp.numel() != B * 8 * E:
        raise TypeError("attention_decode_mqa: bf16 [B, 8 * 512] queries against a bf16 [B, S, 512] memory")
    qp = qp if qp.is_contiguous() else qp.contiguous()
    memory = memory if memory.is_contiguous() else memory.contiguous()
    out = torch.empty(B, 8 * E, dtype=torch.bfloat16, device=memory.device)
    nsplit = A.lib.case_attention_decode_mqa_splits(B, S)
    need = A.lib.case_attention_decode_mqa_workspace(B, S, nsplit)
    ws = torch.empty(need // 4, dtype=torch.float32, device=memory.device) if need else None
    A.call("case_attention_decode_mqa", _ptr(qp), _ptr(memory), _ptr(_u8(key_valid)), _ptr(out), B, S, 8 * E, nsplit, _ptr(ws), need, _stream())
    return out


# The greedy step's self-attention with the cache append inside the launch (case_attention_decode_append): "auto" / "off" (A/B: the strided
# copy into the cache + case_attention_decode)
DECODE_APPEND = os.environ.get("CASE_DECODE_APPEND", "auto")


def decode_append_supported(qkv, cache, heads, d):
    return (DECODE_APPEND != "off" and qkv.is_cuda and qkv.dtype == torch.bfloat16 and cache.dtype == torch.bfloat16 and qkv.dim() == 3
            and qkv.shape[1] == 1 and qkv.is_contiguous() and cache.is_contiguous() and not torch.is_grad_enabled()
            and qkv.shape[0] * heads >= DECODE_MIN_PAIRS and bool(A.lib.case_abi_features() & A.FEAT_ATTN_DECODE_APPEND)
            and bool(A.lib.case_attention_decode_supported(d)))


def attention_decode_append(qkv, cache, t, heads, d, key_valid=None):
    """qkv [N, 1, 3E] bf16: the packed projections of position ``t``; cache [N, Tmax, 2E] bf16: K | V of the earlier positions.  Writes the K | V
    columns of qkv into cache[:, t] and returns the attention of the query columns over the cache rows ``key_valid`` marks (which must include
    position t when it is to be attended) -> [N, 1, E].  One launch (no autograd: inference)."""
    N, _, W = qkv.shape
    E = heads * d
    if W != 3 * E or cache.shape[0] != N or cache.shape[2] != 2 * E or not 0 <= t < cache.shape[1]:
        raise ValueError("attention_decode_append: qkv %s against a cache %s at position %d" % (tuple(qkv.shape), tuple(cache.shape), t))
    O = torch.empty(N, 1, E, dtype=qkv.dtype, device=qkv.device)
    ad = _attn_desc(N, heads, 1, cache.shape[1], d, qkv, cache, cache, False, 1.0 / math.sqrt(d), None)
    A.call("case_attention_decode_append", ad, _ptr(qkv), _ptr(cache), _ptr(cache, E), _ptr(qkv, E), _ptr(qkv, 2 * E), W, t, _ptr(_u8(key_valid)), _ptr(O),
           _stream())
    return O


def attention(q_src, k_src, v_src, q_off, k_off, v_off, heads, d, key_valid=None, causal=False, p_drop=0.0, add_mask=None):
    return AttentionFn.apply(q_src, k_src, v_src, q_off, k_off, v_off, heads, d, _u8(key_valid), causal, p_drop, add_mask)


class AttentionGroupsFn(Function):
    """Fused self-attention of several sequence GROUPS that live in ONE packed projection buffer: rows [r0, r0 + N L) of qkv [rows, 3E]
    are the N sequences of length L of a group (the shared query / passage encoder runs its row-local work -- LayerNorm, projections,
    feed-forward -- once over the query rows and the passage rows together; only the attention core needs the sequence geometry).
    One launch of the fused kernels per group, reading and writing slices of the shared buffers in place: no split / concat copies."""

    @staticmethod
    def forward(ctx, qkv, heads, d, p_drop, groups, *valids):
        rows, W = qkv.shape
        E = heads * d
        alpha = 1.0 / math.sqrt(d)
        O = torch.empty(rows, E, dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty(sum(N * heads * L for _, N, L in groups), dtype=torch.float32, device=qkv.device)
        drops, lo = [], 0
        for (r0, N, L), valid in zip(groups, valids):
            drop = (p_drop,) + config.next_rng(N * heads * L * L) if p_drop > 0.0 else None
            view = qkv[r0:r0 + N * L].view(N, L, W)
            ad = _attn_desc(N, heads, L, L, d, view, view, view, False, alpha, drop)
            A.call("case_attention_fwd", ad, _ptr(qkv, r0 * W), _ptr(qkv, r0 * W + E), _ptr(qkv, r0 * W + 2 * E), _ptr(valid),
                   _ptr(O, r0 * E), _ptr(lse, lo), _stream())
            drops.append(drop)
            lo += N * heads * L
        ctx.save_for_backward(qkv, O, lse, *valids)
        ctx.meta = (heads, d, groups, drops, alpha)
        return O

    @staticmethod
    def backward(ctx, dO):
        qkv, O, lse = ctx.saved_tensors[:3]
        valids = ctx.saved_tensors[3:]
        heads, d, groups, drops, alpha = ctx.meta
        rows, W = qkv.shape
        E = heads * d
        dO = dO if dO.is_contiguous() else dO.contiguous()
        dqkv = torch.empty_like(qkv)  # the q, k and v slices of every row are written by the kernels
        delta = torch.empty(2 * lse.numel(), dtype=torch.float32, device=lse.device)  # (case_attention_bwd_scratch_floats of each group)
        lo = 0
        for (r0, N, L), valid, drop in zip(groups, valids, drops):
            view = qkv[r0:r0 + N * L].view(N, L, W)
            ad = _attn_desc(N, heads, L, L, d, view, view, view, False, alpha, drop)
            assert A.lib.case_attention_bwd_scratch_floats(ad) <= 2 * N * heads * L
            A.call("case_attention_bwd", ad, _ptr(qkv, r0 * W), _ptr(qkv, r0 * W + E), _ptr(qkv, r0 * W + 2 * E), _ptr(valid),
                   _ptr(O, r0 * E), _ptr(lse, lo), _ptr(dO, r0 * E), _ptr(delta, 2 * lo), _ptr(dqkv, r0 * W), _ptr(dqkv, r0 * W + E),
                   _ptr(dqkv, r0 * W + 2 * E), _stream())
            lo += N * heads * L
        return (dqkv, None, None, None, None) + (None,) * len(valids)


def attention_groups_supported(dtype, heads, d, width, needs_grad):
    """The grouped form exists for the fused kernels only (bf16, a built head size on the training / inference list, packed width 3E)."""
    if ATTENTION_MODE == "unfused" or dtype != torch.bfloat16 or width != 3 * heads * d or width % 8:
        return False
    if not A.lib.case_attention_supported(d) or (needs_grad and not A.lib.case_attention_bwd_supported(d)):
        return False
    return ATTENTION_MODE == "fused" or d in (_FUSED_TRAINING if needs_grad else _FUSED_INFERENCE)


def attention_groups(qkv, groups, valids, heads, d, p_drop=0.0):
    """qkv [rows, 3 heads d] contiguous; groups [(first row, sequences, length)] tiling the rows; valids: per group [N, L] bool or None."""
    assert qkv.dim() == 2 and qkv.is_contiguous() and sum(N * L for _, N, L in groups) == qkv.shape[0]
    return AttentionGroupsFn.apply(qkv, heads, d, p_drop, tuple(groups), *[_u8(v) for v in valids])


class SplitRowsFn(Function):
    """Row ranges of a [rows, C] tensor as separate [N, L, C] views; backward gathers the range gradients into ONE buffer (autograd's
    own slicing would build a zero-filled full-size tensor per range and add them)."""

    @staticmethod
    def forward(ctx, x, groups):
        ctx.groups, ctx.shape = groups, x.shape
        return tuple(x[r0:r0 + N * L].view(N, L, x.shape[1]) for r0, N, L in groups)

    @staticmethod
    def backward(ctx, *grads):
        rows, C = ctx.shape
        like = next(g for g in grads if g is not None)
        parts = [g.reshape(N * L, C) if g is not None else like.new_zeros(N * L, C) for (r0, N, L), g in zip(ctx.groups, grads)]
        return torch.cat(parts, dim=0), None


def split_rows(x, groups):
    return SplitRowsFn.apply(x, tuple(groups))


# ----------------------------------------------------------------------------------------------
# batched matmul for the Interaction chain:  C[n] = A[n] op(B[n])  (+ row / column rank-1 terms)
# ----------------------------------------------------------------------------------------------
class BmmFn(Function):
    @staticmethod
    def forward(ctx, a, b, b_is_kn, bias_row, bias_col_per_batch, out_dtype):
        """a [n, M, K]; b [n, N, K] (b_is_kn=False: C = A B^T) or [n, K, N] (True: C = A B).
        bias_row f32 [n, M] adds to every column; bias_col_per_batch f32 [n, N] is added by a second pass."""
        n, M, K = a.shape
        N = b.shape[2] if b_is_kn else b.shape[1]
        a = a if a.is_contiguous() else a.contiguous()
        b = b if b.is_contiguous() else b.contiguous()
        c = torch.empty(n, M, N, dtype=out_dtype or a.dtype, device=a.device)
        gemm(a, b, c, M, N, K, K, b.shape[2], N, b_kmajor=b_is_kn, batch1=n, sa=(M * K, 0), sb=(b.shape[1] * b.shape[2], 0),
             sc=(M * N, 0), epilogue=A.EPI_BIAS_ROW if bias_row is not None else 0, bias_row=bias_row)
        ctx.save_for_backward(a, b)
        ctx.meta = (b_is_kn, bias_row is not None)
        return c

    @staticmethod
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        b_is_kn, has_row = ctx.meta
        n, M, K = a.shape
        N = dc.shape[2]
        g = cast(dc, a.dtype)
        g = g if g.is_contiguous() else g.contiguous()
        da = torch.empty_like(a)
        db = torch.empty_like(b)
        if b_is_kn:  # C = A B,  B [K, N]:  dA = G B^T (B rows are K, contraction over N -> B is "N_out x Kc" = [K, N]: NT)
            gemm(g, b, da, M, K, N, N, N, K, batch1=n, sa=(M * N, 0), sb=(K * N, 0), sc=(M * K, 0))
            # dB[K, N] = A^T G : A k-major [M(Kc), K], G k-major [M(Kc), N]
            gemm(a, g, db, K, N, M, K, N, N, a_kmajor=True, b_kmajor=True, batch1=n, sa=(M * K, 0), sb=(M * N, 0), sc=(K * N, 0))
        else:  # C = A B^T, B [N, K]: dA = G B (B k-major: [N(Kc), K]) ; dB[N, K] = G^T A
            gemm(g, b, da, M, K, N, N, K, K, b_kmajor=True, batch1=n, sa=(M * N, 0), sb=(N * K, 0), sc=(M * K, 0))
            gemm(g, a, db, N, K, M, N, K, K, a_kmajor=True, b_kmajor=True, batch1=n, sa=(M * N, 0), sb=(M * K, 0), sc=(N * K, 0))
        d_row = dc.float().sum(dim=2) if has_row else None  # [n, M] tiny reduction (glue)
        return da, db, None, d_row, None, None


def bmm(a, b, b_is_kn=False, bias_row=None, out_dtype=None):
    return BmmFn.apply(a, b, b_is_kn, bias_row, None, out_dtype)


# ----------------------------------------------------------------------------------------------
# K1 embedding + position
# ----------------------------------------------------------------------------------------------
class EmbedPosFn(Function):
    @staticmethod
    def forward(ctx, ids, table, pe, seq_len, p_drop, dtype):
        rows, (V, H) = ids.numel(), table.shape
        ids_c = ids.contiguous()
        out = torch.empty(*ids.shape, H, dtype=dtype, device=table.device)
        drop = (p_drop,) + config.next_rng(rows * H) if p_drop > 0.0 else (0.0, 0, 0, None)
        scale = math.sqrt(H)
        A.call("case_embed_pos_fwd", _ptr(ids_c), _ptr(table.detach()), _ptr(pe), _ptr(out), rows, seq_len, H, V, scale, drop[0],
               drop[1], drop[2], drop[3], _DT[dtype], _stream())
        ctx.save_for_backward(ids_c)
        ctx.meta = (V, H, scale, drop)
        return out

    @staticmethod
    def backward(ctx, d_out):
        (ids_c,) = ctx.saved_tensors
        V, H, scale, drop = ctx.meta
        d_out = d_out if d_out.is_contiguous() else d_out.contiguous()
        d_table = _zeros_like_shapes(d_out.device, (V, H))[0]
        A.call("case_embed_pos_bwd", _ptr(ids_c), _ptr(d_out), _ptr(d_table), ids_c.numel(), H, V, scale, drop[0], drop[1],
               drop[2], drop[3], _code(d_out), _stream())
        return None, d_table, None, None, None, None


def embed_pos(ids, table, pe, p_drop=0.0, dtype=None):
    """ids [..., L] -> [..., L, H] = table[ids]*sqrt(H) + pe[position]."""
    return EmbedPosFn.apply(ids, table, pe, ids.shape[-1], p_drop, dtype or config.compute_dtype())


class ScaleAddRowsFn(Function):
    @staticmethod
    def forward(ctx, x, pe, scale):
        L, H = x.shape[-2], x.shape[-1]
        x = x if x.is_contiguous() else x.contiguous()
        y = torch.empty_like(x)
        A.call("case_scale_add_rows", _ptr(x), _ptr(pe), _ptr(y), x.numel() // H, L, H, scale, _code(x), _stream())
        ctx.scale = scale
        return y

    @staticmethod
    def backward(ctx, g):
        H = g.shape[-1]
        g = g if g.is_contiguous() else g.contiguous()
        dx = torch.empty_like(g)
        A.call("case_scale_add_rows", _ptr(g), None, _ptr(dx), g.numel() // H, 1, H, ctx.scale, _code(g), _stream())
        return dx, None, None


def scale_add_rows(x, pe, scale):
    """x [..., L, H] * scale + pe[:L]  (stand-alone PositionalEmbedding)."""
    return ScaleAddRowsFn.apply(x, pe, scale)


class CastFn(Function):
    @staticmethod
    def forward(ctx, x, dtype):
        ctx.src = x.dtype
        return cast(x, dtype)

    @staticmethod
    def backward(ctx, g):
        return cast(g, ctx.src), None


def cast_to(x, dtype):
    """Differentiable dtype conversion (identity when already ``dtype``)."""
    return x if x.dtype == dtype else CastFn.apply(x, dtype)


# ----------------------------------------------------------------------------------------------
# small elementwise ops
# ----------------------------------------------------------------------------------------------
FANOUT = os.environ.get("CASE_FANOUT", "1") != "0"  # A/B switch: "0" leaves the gradient sums to autograd's binary adds


def add_n(tensors):
    """Sum of 2 .. 8 same-shaped tensors in one pass (f32 accumulation, one rounding)."""
    ts = [t if t.is_contiguous() else t.contiguous() for t in tensors]
    out = torch.empty_like(ts[0])
    arr = (A.ptr * len(ts))(*[t.data_ptr() for t in ts])
    A.call("case_add_n", arr, len(ts), _ptr(out), out.numel(), _code(out), _stream())
    return out


class FanOutFn(Function):
    """n aliases of one tensor for n consumers: the backward pass receives the n gradients TOGETHER and sums them in one kernel
    (case_add_n: n + 1 tensor passes) instead of the autograd engine's n - 1 binary adds (3 (n - 1) passes, each intermediate rounded to
    bf16).  Used where a large activation feeds several products: the Interaction tensors (common/Interaction.py:32-63) and the
    memory of a decoder stack (one K / V projection per layer, common/TransformerDecoder.py:76-89)."""

    @staticmethod
    def forward(ctx, x, n):
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        gs = [g for g in grads if g is not None]
        if not gs:
            return None, None
        if len(gs) == 1:
            return gs[0], None
        dt = gs[0].dtype
        ev = 8 if dt == torch.bfloat16 else 4
        # (a contiguous gradient may still start at an odd storage offset -- torch.cat's backward hands out such slices -- and case_add_n
        #  takes 16-byte aligned sources only; a non-contiguous one is copied by add_n into a fresh, aligned allocation)
        if (not gs[0].is_cuda or dt not in (torch.bfloat16, torch.float32) or gs[0].numel() % ev or len(gs) > 8
                or any(g.dtype != dt or g.shape != gs[0].shape for g in gs)
                or any(g.is_contiguous() and g.data_ptr() % 16 for g in gs)):
            total = gs[0]
            for g in gs[1:]:
                total = total + g
            return total, None
        return add_n(gs), None


class SplitParamRowsFn(Function):
    """(w[:k], w[k:]) of a parameter used in two places (the query rows and the key / value rows of a cross-attention's packed
    in-projection, common/TransformerDecoder.py:81 through nn.MultiheadAttention): the two gradients arrive together and are
    concatenated by ONE launch.  Plain slicing costs five per parameter and step: autograd zero-fills a full-size tensor for each
    slice, copies the slice's gradient in, and adds the two."""

    @staticmethod
    def forward(ctx, w, k):
        k = int(k)
        ctx.k, ctx.shape = k, w.shape
        return w[:k], w[k:]

    @staticmethod
    def backward(ctx, g0, g1):
        k, shape = ctx.k, ctx.shape
        ref = g0 if g0 is not None else g1
        if ref is None:
            return None, None
        if g0 is None:
            g0 = torch.zeros((k,) + tuple(shape[1:]), dtype=ref.dtype, device=ref.device)
        if g1 is None:
            g1 = torch.zeros((shape[0] - k,) + tuple(shape[1:]), dtype=ref.dtype, device=ref.device)
        return torch.cat([g0, g1], dim=0), None


def split_param_rows(w, k):
    k = int(k)
    if not (torch.is_grad_enabled() and w.requires_grad):
        return w[:k], w[k:]
    return SplitParamRowsFn.apply(w, k)


def fanout(x, n):
    """``n`` aliases of ``x`` whose gradients are summed in one pass (identity when gradients are off or the switch is)."""
    if n < 2 or not FANOUT or not (torch.is_grad_enabled() and x.requires_grad):
        return (x,) * n
    return FanOutFn.apply(x, n)


class AddFn(Function):
    @staticmethod
    def forward(ctx, a, b):
        a = a if a.is_contiguous() else a.contiguous()
        b = b if b.is_contiguous() else b.contiguous()
        out = torch.empty_like(a)
        A.call("case_add", _ptr(a), _ptr(b), _ptr(out), a.numel(), _code(a), _stream())
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g


def add(a, b):
    return AddFn.apply(a, b)


class DropoutFn(Function):
    @staticmethod
    def forward(ctx, x, p):
        x = x if x.is_contiguous() else x.contiguous()
        ctx.rng = (p,) + config.next_rng(x.numel())
        return _dropout_raw(x, *ctx.rng)

    @staticmethod
    def backward(ctx, g):
        g = g if g.is_contiguous() else g.contiguous()
        return _dropout_raw(g, *ctx.rng), None


def dropout(x, p, training=True):
    p = config.drop_p(p, training)
    return DropoutFn.apply(x, p) if p > 0.0 else x


class MaskRowsFn(Function):
    @staticmethod
    def forward(ctx, x, valid_u8):
        C = x.shape[-1]
        x = x if x.is_contiguous() else x.contiguous()
        y = torch.empty_like(x)
        A.call("case_mask_rows", _ptr(x), _ptr(valid_u8), _ptr(y), x.numel() // C, C, _code(x), _stream())
        ctx.save_for_backward(valid_u8)
        return y

    @staticmethod
    def backward(ctx, g):
        (valid_u8,) = ctx.saved_tensors
        C = g.shape[-1]
        g = g if g.is_contiguous() else g.contiguous()
        dx = torch.empty_like(g)
        A.call("case_mask_rows", _ptr(g), _ptr(valid_u8), _ptr(dx), g.numel() // C, C, _code(g), _stream())
        return dx, None


def mask_rows(x, valid, in_place=False):
    """Zero x[..., r, :] where valid[..., r] is False.  ``in_place`` (the caller owns x and nobody else reads it): without autograd the rows are
    zeroed IN x -- the kernel then touches the invalid rows only (the B = 256 encode phase spent 3.3 ms per pass copying valid rows)."""
    if in_place and not (torch.is_grad_enabled() and x.requires_grad) and x.is_contiguous():
        C = x.shape[-1]
        A.call("case_mask_rows", _ptr(x), _ptr(_u8(valid)), _ptr(x), x.numel() // C, C, _code(x), _stream())
        return x
    # (in training the out-of-place op stays: x is the output of a custom Function -- a view of its workspace -- and autograd refuses an
    #  in-place write to such a tensor)
    return MaskRowsFn.apply(x, _u8(valid))


class ScaleColsFn(Function):
    @staticmethod
    def forward(ctx, x, w):
        C = x.shape[-1]
        x = x if x.is_contiguous() else x.contiguous()
        wc = w.detach().contiguous()
        y = torch.empty_like(x)
        A.call("case_scale_cols", _ptr(x), _ptr(wc), _ptr(y), x.numel() // C, C, _code(x), _stream())
        ctx.save_for_backward(x, wc)
        return y

    @staticmethod
    def backward(ctx, g):
        x, wc = ctx.saved_tensors
        C = x.shape[-1]
        g = g if g.is_contiguous() else g.contiguous()
        dx = torch.empty_like(x)
        dw = _zeros_like_shapes(x.device, (C,))[0]
        A.call("case_scale_cols_bwd", _ptr(g), _ptr(x), _ptr(wc), _ptr(dx), _ptr(dw), x.numel() // C, C, _code(x), _stream())
        return dx, dw


def scale_cols(x, w):
    return ScaleColsFn.apply(x, w)


class MaskedMeanFn(Function):
    @staticmethod
    def forward(ctx, x, valid_u8):
        n, L, H = x.shape
        x = x if x.is_contiguous() else x.contiguous()
        out = torch.empty(n, H, dtype=x.dtype, device=x.device)
        A.call("case_masked_mean_fwd", _ptr(x), _ptr(valid_u8), _ptr(out), n, L, H, _code(x), _stream())
        ctx.save_for_backward(valid_u8)
        ctx.shape = (n, L, H)
        return out

    @staticmethod
    def backward(ctx, g):
        (valid_u8,) = ctx.saved_tensors
        n, L, H = ctx.shape
        g = g if g.is_contiguous() else g.contiguous()
        dx = torch.empty(n, L, H, dtype=g.dtype, device=g.device)
        A.call("case_masked_mean_bwd", _ptr(g), _ptr(valid_u8), _ptr(dx), n, L, H, _code(g), _stream())
        return dx, None


def masked_mean(x, valid):
    return MaskedMeanFn.apply(x, _u8(valid))


class HighwayGateFn(Function):
    @staticmethod
    def forward(ctx, gnl):
        cols = gnl.shape[-1] // 3
        gnl = gnl if gnl.is_contiguous() else gnl.contiguous()
        rows = gnl.numel() // (3 * cols)
        y = torch.empty(*gnl.shape[:-1], cols, dtype=gnl.dtype, device=gnl.device)
        A.call("case_highway_gate_fwd", _ptr(gnl), _ptr(y), rows, cols, _code(gnl), _stream())
        ctx.save_for_backward(gnl)
        return y

    @staticmethod
    def backward(ctx, g):
        (gnl,) = ctx.saved_tensors
        cols = gnl.shape[-1] // 3
        rows = gnl.numel() // (3 * cols)
        g = g if g.is_contiguous() else g.contiguous()
        d = torch.empty_like(gnl)
        A.call("case_highway_gate_bwd", _ptr(g), _ptr(gnl), _ptr(d), rows, cols, _code(gnl), _stream())
        return d


def highway_gate(gnl):
    return HighwayGateFn.apply(gnl)


class Concat5Fn(Function):
    @staticmethod
    def forward(ctx, e, a1, a2, valid_u8):
        H = e.shape[-1]
        e, a1, a2 = (t if t.is_contiguous() else t.contiguous() for t in (e, a1, a2))
        rows = e.numel() // H
        out = torch.empty(*e.shape[:-1], 5 * H, dtype=e.dtype, device=e.device)
        A.call("case_concat5_fwd", _ptr(e), _ptr(a1), _ptr(a2), _ptr(valid_u8), _ptr(out), rows, H, _code(e), _stream())
        ctx.save_for_backward(e, a1, a2, valid_u8)
        return out

    @staticmethod
    def backward(ctx, g):
        e, a1, a2, valid_u8 = ctx.saved_tensors
        H = e.shape[-1]
        g = g if g.is_contiguous() else g.contiguous()
        de, d1, d2 = torch.empty_like(e), torch.empty_like(e), torch.empty_like(e)
        A.call("case_concat5_bwd", _ptr(g), _ptr(e), _ptr(a1), _ptr(a2), _ptr(valid_u8), _ptr(de), _ptr(d1), _ptr(d2),
               e.numel() // H, H, _code(e), _stream())
        return de, d1, d2, None


def concat5(e, a1, a2, valid, shape=None):
    """[e | a1 | a2 | e o a1 | e o a2] with the rows of ``valid`` == 0 zeroed, optionally reshaped.  The result remembers its pieces
    (``_case_concat5``) so that a LayerNorm applied DIRECTLY to it can run the fused backward (concat5_layer_norm_carry)."""
    vu = _u8(valid)
    out = Concat5Fn.apply(e, a1, a2, vu)
    if shape is not None:
        out = out.reshape(shape)
    if out.requires_grad:
        out._case_concat5 = (e, a1, a2, vu)
    return out


CONCAT5_LN = os.environ.get("CASE_CONCAT5_LN", "1") != "0"  # A/B switch


class Concat5LayerNormFn(Function):
    """(LN(G), G') for G = concat5(e, a1, a2): G' carries the block's residual use of G.  The forward is the ordinary LayerNorm over the
    concatenation the caller already formed; the BACKWARD goes from (d LN, d G') straight to (d e, d a1, d a2) in one kernel
    (case_layernorm_bwd_concat5) -- the 5H-wide gradient of G is never written or re-read."""

    @staticmethod
    def forward(ctx, e, a1, a2, valid_u8, G, gamma, beta, eps):
        C = G.shape[-1]
        xa = G.detach().reshape(-1, C)
        R = xa.shape[0]
        y = torch.empty_like(xa)
        mean = torch.empty(R, dtype=torch.float32, device=xa.device)
        rstd = torch.empty_like(mean)
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        A.call("case_layernorm_fwd", _ptr(xa), None, _ptr(g), _ptr(b), _ptr(y), _ptr(mean), _ptr(rstd), R, C, eps, _code(xa), _stream())
        ctx.save_for_backward(xa, g, mean, rstd, valid_u8)
        ctx.shapes = (G.shape, e.shape)
        return y.view(G.shape), G.detach().view_as(G)

    @staticmethod
    def backward(ctx, dy, d_carry):
        xa, g, mean, rstd, valid_u8 = ctx.saved_tensors
        gshape, eshape = ctx.shapes
        R, C = xa.shape
        H = C // 5
        dy2 = dy.reshape(R, C)
        dy2 = dy2 if dy2.is_contiguous() else dy2.contiguous()
        extra = None
        if d_carry is not None:
            extra = d_carry.reshape(R, C).to(xa.dtype)
            extra = extra if extra.is_contiguous() else extra.contiguous()
        de, d1, d2 = (torch.empty(R, H, dtype=xa.dtype, device=xa.device) for _ in range(3))
        dg, db = _zeros_like_shapes(xa.device, (C,), (C,))
        A.call("case_layernorm_bwd_concat5", _ptr(dy2), _ptr(xa), _ptr(g), _ptr(mean), _ptr(rstd), _ptr(extra), _ptr(xa), _ptr(xa), _ptr(xa),
               _ptr(valid_u8), _ptr(de), _ptr(d1), _ptr(d2), _ptr(dg), _ptr(db), R, H, _code(xa), _stream())
        return de.view(eshape), d1.view(eshape), d2.view(eshape), None, None, dg, db, None


def concat5_layer_norm_carry(G, gamma, beta, eps):
    """ops.layer_norm_carry(G, ...) for a G that ops.concat5 made (it carries its pieces as ``_case_concat5``), with the fused backward;
    None when G is not such a tensor or the kernel does not take the shape."""
    src = getattr(G, "_case_concat5", None)
    if (src is None or not CONCAT5_LN or G.dtype != torch.bfloat16 or G.shape[-1] != 2560 or not G.is_contiguous()
            or not (torch.is_grad_enabled() and G.requires_grad)):
        return None
    e, a1, a2, valid_u8 = src
    # G enters DETACHED: the gradient goes to the pieces directly.  (As a differentiable input with a None gradient, autograd still ran the
    # concatenation's own backward on a materialised 5H-wide zero tensor.)
    return Concat5LayerNormFn.apply(e, a1, a2, valid_u8, G.detach(), gamma, beta, eps)


# K8 as kernels (round 6, csrc/interaction.hip): scores + both softmaxes in one launch, the four products + the two concatenations in a
# second -- instead of the 16 single launches of common/Interaction.py.  "auto": bf16, H = 512, Lq = 64, Lp a multiple of 32 up to 512,
# no autograd (the greedy pass's encode phase, evaluation); "off": the single launches.
INTERACTION_FUSED = os.environ.get("CASE_INTERACTION_FUSED", "auto")


def interaction_supported(Eq, Ep, needs_grad):
    if INTERACTION_FUSED == "off" or needs_grad or not (Eq.is_cuda and Eq.dtype == torch.bfloat16 and Ep.dtype == torch.bfloat16):
        return False
    if Eq.shape[1] not in (1, Ep.shape[1]):
        return False  # one query per sample, or one per passage: anything else is refused by the single launches
    if not A.lib.case_abi_features() & A.FEAT_INTERACTION:
        return False
    d = A.InteractionDesc()
    d.n, d.Lp, d.Lq, d.H, d.eq_div, d.dtype = Ep.shape[0] * Ep.shape[1], Ep.shape[2], Eq.shape[2], Ep.shape[3], 1, A.BF16
    return bool(A.lib.case_interaction_supported(d))


def interaction_fwd(Eq, Ep, q_valid, p_valid, w):
    """Eq [B, nq, Lq, H] (nq = 1 or P), Ep [B, P, Lp, H] bf16; masks bool [B, nq, Lq] / [B, P, Lp]; w f32 [1, 3H] ->
    (G_p_q [B, P, Lq, 5H], G_q_p [B, P, Lp, 5H], A [B P, Lp, Lq], Bm^T [B P, Lq, Lp]).  No autograd."""
    B, nq, Lq, H = Eq.shape
    _, P, Lp, _ = Ep.shape
    if nq not in (1, P):
        raise ValueError("interaction_fwd: %d queries for %d passages (one query, or one per passage)" % (nq, P))
    n = B * P
    Eq, Ep = (t if t.is_contiguous() else t.contiguous() for t in (Eq.detach(), Ep.detach()))
    qv, pv = _u8(q_valid), _u8(p_valid)
    wf = w.detach().reshape(-1).float().contiguous()
    d = A.InteractionDesc()
    d.n, d.Lp, d.Lq, d.H, d.eq_div, d.dtype = n, Lp, Lq, H, (P if nq != P else 1), A.BF16
    dev = Ep.device
    a = torch.empty(n, Lp, Lq, dtype=torch.bfloat16, device=dev)
    bt = torch.empty(n, Lq, Lp, dtype=torch.bfloat16, device=dev)
    gqp = torch.empty(B, P, Lp, 5 * H, dtype=torch.bfloat16, device=dev)
    gpq = torch.empty(B, P, Lq, 5 * H, dtype=torch.bfloat16, device=dev)
    A.call("case_interaction_fwd", d, _ptr(Eq), _ptr(Ep), _ptr(qv), _ptr(pv), _ptr(wf), _ptr(a), _ptr(bt), _ptr(gqp), _ptr(gpq), _stream())
    return gpq, gqp, a, bt


INTERACTION_TRAIN = os.environ.get("CASE_INTERACTION_TRAIN", "1") != "0"  # A/B switch: the fused forward + explicit backward in training


class InteractionFn(Function):
    """K8 in TRAINING: the two forward kernels (ops.interaction_fwd) with an explicit backward -- the chain rule of
    common/Interaction.py:32-74 written out on the saved probabilities A / Bm^T and the A1 / B1 columns of the two outputs, as batched
    GEMMs on strided views (nothing is concatenated or copied), with the score gradient formed ONCE (the single-launch forward computes U
    and U^T by two GEMMs and autograd differentiates both).  Outputs: (G_p_q, G_q_p, A1', A2'): A1' / A2' are the [.., H:2H] / [.., 2H:3H]
    columns of G_q_p as tensors of their own, so that the TransformerBlock's fused LayerNorm<5H> + concatenation backward
    (ops.concat5_layer_norm_carry) can hand their gradients -- and Ep's -- over without a 5H-wide gradient tensor."""

    @staticmethod
    def forward(ctx, Eq, Ep, w, q_valid, p_valid):
        ctx.set_materialize_grads(False)  # an output nobody differentiates arrives as None, not as a 5H-wide tensor of zeros
        gpq, gqp, a, bt = interaction_fwd(Eq, Ep, q_valid, p_valid, w)
        H = Ep.shape[-1]
        ctx.save_for_backward(Eq.detach(), Ep.detach(), w.detach(), a, bt, gqp, gpq, _u8(q_valid), _u8(p_valid))
        a1p, a2p = gqp[..., H:2 * H], gqp[..., 2 * H:3 * H]
        return gpq, gqp, a1p, a2p

    @staticmethod
    def backward(ctx, dgpq, dgqp, da1p, da2p):
        Eq, Ep, w, a, bt, gqp, gpq, qv, pv = ctx.saved_tensors
        B, nq, Lq, H = Eq.shape
        _, P, Lp, _ = Ep.shape
        n, dt, dev = B * P, Ep.dtype, Ep.device
        C5 = 5 * H
        Ep3 = Ep.reshape(n, Lp, H)
        Ep3 = Ep3 if Ep3.is_contiguous() else Ep3.contiguous()
        Eqx = (Eq.expand(-1, P, -1, -1) if nq != P else Eq).reshape(n, Lq, H)
        Eqx = Eqx if Eqx.is_contiguous() else Eqx.contiguous()
        qvx = (qv.view(B, nq, Lq).expand(-1, P, -1) if nq != P else qv.view(B, nq, Lq)).reshape(n, Lq).contiguous()
        wf = w.reshape(-1).float().contiguous()
        w1, w2, w3 = wf[:H], wf[H:2 * H], wf[2 * H:]
        st = _stream()

        def bg(x, y, M, N, K, lda, ldb, x_off=0, y_off=0, xk=False, yk=False, sx=None, sy=None, add=None):
            """C[n, M, N] = op(x) op(y) (+ add), batched over the n pairs; strided operands by offset / leading dimension / batch stride."""
            c = torch.empty(n, M, N, dtype=dt, device=dev)
            gemm(x, y, c, M, N, K, lda, ldb, N, a_off=x_off, b_off=y_off, a_kmajor=xk, b_kmajor=yk, batch1=n,
                 sa=(sx if sx is not None else (K * M), 0), sb=(sy if sy is not None else (K * N), 0), sc=(M * N, 0),
                 epilogue=A.EPI_RESIDUAL if add is not None else 0, aux=add, ld_aux=N, saux=(M * N, 0))
            return c

        # ---- gradients of the concatenations ------------------------------------------------------------------------------------------------
        dEp_parts, dEq_parts = [], []
        dA1 = None if da1p is None else cast(da1p, dt).reshape(n, Lp, H)
        dA2 = None if da2p is None else cast(da2p, dt).reshape(n, Lp, H)
        if dgqp is not None:  # G_q_p consumed as a whole (not through the fused LayerNorm + concatenation backward)
            g = cast(dgqp, dt).reshape(n * Lp, C5)
            g = g if g.is_contiguous() else g.contiguous()
            a1c, a2c = gqp.reshape(n * Lp, C5)[:, H:2 * H].contiguous(), gqp.reshape(n * Lp, C5)[:, 2 * H:3 * H].contiguous()
            de, d1, d2 = (torch.empty(n * Lp, H, dtype=dt, device=dev) for _ in range(3))
            A.call("case_concat5_bwd", _ptr(g), _ptr(Ep3), _ptr(a1c), _ptr(a2c), _ptr(pv), _ptr(de), _ptr(d1), _ptr(d2), n * Lp, H, _code(Ep3), st)
            dEp_parts.append(de.view(n, Lp, H))
            dA1 = d1.view(n, Lp, H) if dA1 is None else add_n([dA1, d1.view(n, Lp, H)])
            dA2 = d2.view(n, Lp, H) if dA2 is None else add_n([dA2, d2.view(n, Lp, H)])
        zeros_p = None
        if dA1 is None or dA2 is None:
            zeros_p = torch.zeros(n, Lp, H, dtype=dt, device=dev)
            dA1 = zeros_p if dA1 is None else dA1
            dA2 = zeros_p if dA2 is None else dA2
        dA1 = dA1 if dA1.is_contiguous() else dA1.contiguous()
        dA2 = dA2 if dA2.is_contiguous() else dA2.contiguous()
        if dgpq is not None:
            g = cast(dgpq, dt).reshape(n * Lq, C5)
            g = g if g.is_contiguous() else g.contiguous()
            g2 = gpq.reshape(n * Lq, C5)
            b1c, b2c = g2[:, H:2 * H].contiguous(), g2[:, 2 * H:3 * H].contiguous()
            de, dB1, dB2 = (torch.empty(n * Lq, H, dtype=dt, device=dev) for _ in range(3))
            A.call("case_concat5_bwd", _ptr(g), _ptr(Eqx), _ptr(b1c), _ptr(b2c), _ptr(qvx), _ptr(de), _ptr(dB1), _ptr(dB2), n * Lq, H, _code(Eqx), st)
            dEq_parts.append(de.view(n, Lq, H))
            dB1, dB2 = dB1.view(n, Lq, H), dB2.view(n, Lq, H)
        else:
            dB1 = dB2 = torch.zeros(n, Lq, H, dtype=dt, device=dev)
        # ---- the four products (A1 / B1 are the [H, 2H) columns of the outputs: leading dimension 5H) ----------------------------------------
        #   A2 = A B1:  dA = dA2 B1^T,  dB1 += A^T dA2        B2 = Bm^T A1:  dBm^T = dB2 A1^T,  dA1 += Bm dB2
        dA = bg(dA2, gpq, Lp, Lq, H, H, C5, y_off=H, sy=Lq * C5)
        dB1t = bg(a, dA2, Lq, H, Lp, Lq, H, xk=True, yk=True, add=dB1)
        dA1t = bg(bt, dB2, Lp, H, Lq, Lp, H, xk=True, yk=True, add=dA1)
        dBt = bg(dB2, gqp, Lq, Lp, H, H, C5, y_off=H, sy=Lp * C5)
        #   A1 = A Eq:  dA += dA1 Eq^T,  dEq += A^T dA1       B1 = Bm^T Ep:  dBm^T += dB1 Ep^T,  dEp += Bm dB1
        dA = bg(dA1t, Eqx, Lp, Lq, H, H, H, add=dA)
        dBt = bg(dB1t, Ep3, Lq, Lp, H, H, H, add=dBt)
        dEq_parts.append(bg(a, dA1t, Lq, H, Lp, Lq, H, xk=True, yk=True))
        dEp_parts.append(bg(bt, dB1t, Lp, H, Lq, Lp, H, xk=True, yk=True))
        # ---- the two softmaxes share ONE score matrix ---------------------------------------------------------------------------------------
        dUa = torch.empty(n, Lp, Lq, dtype=torch.float32, device=dev)
        sd = _softmax_desc(n, 1, Lp, Lq, False, A.F32, _DT[dt], None)
        A.call("case_softmax_bwd", sd, _ptr(dA), _ptr(a), _ptr(dUa), st)
        dUb = torch.empty(n, Lq, Lp, dtype=torch.float32, device=dev)
        sd = _softmax_desc(n, 1, Lq, Lp, False, A.F32, _DT[dt], None)
        A.call("case_softmax_bwd", sd, _ptr(dBt), _ptr(bt), _ptr(dUb), st)
        dU32 = dUa + dUb.transpose(1, 2)
        dU = dU32.to(dt)
        # ---- U = (w3 o Ep) Eq^T + w2 . Ep[i] + w1 . Eq[j] -----------------------------------------------------------------------------------
        dEpw = bg(dU, Eqx, Lp, H, Lq, Lq, H, yk=True)
        epw = torch.empty_like(Ep3)
        A.call("case_scale_cols", _ptr(Ep3), _ptr(w3), _ptr(epw), n * Lp, H, _code(Ep3), st)
        dEq_parts.append(bg(dU, epw, Lq, H, Lp, Lq, H, xk=True, yk=True))
        dEp_s = torch.empty_like(Ep3)
        dw1, dw2, dw3 = _zeros_like_shapes(dev, (H,), (H,), (H,))
        A.call("case_scale_cols_bwd", _ptr(dEpw), _ptr(Ep3), _ptr(w3), _ptr(dEp_s), _ptr(dw3), n * Lp, H, _code(Ep3), st)
        dEp_parts.append(dEp_s)
        dap, dcq = dU32.sum(dim=2).reshape(-1).contiguous(), dU32.sum(dim=1).reshape(-1).contiguous()
        dEp_r, dEq_r = torch.empty_like(Ep3), torch.empty_like(Eqx)
        A.call("case_rowdot_bwd", _ptr(dap), _ptr(Ep3), _ptr(w2), _ptr(dEp_r), _ptr(dw2), None, n * Lp, H, _code(Ep3), st)
        A.call("case_rowdot_bwd", _ptr(dcq), _ptr(Eqx), _ptr(w1), _ptr(dEq_r), _ptr(dw1), None, n * Lq, H, _code(Eqx), st)
        dEp_parts.append(dEp_r)
        dEq_parts.append(dEq_r)
        dEp = add_n(dEp_parts).view(Ep.shape)
        dEq = add_n(dEq_parts).view(B, P, Lq, H)
        if nq != P:
            dEq = dEq.float().sum(dim=1, keepdim=True).to(dt)
        dw = torch.cat([dw1, dw2, dw3]).view(w.shape)
        return dEq, dEp, dw, None, None


def interaction_train_supported(Eq, Ep):
    return INTERACTION_TRAIN and interaction_supported(Eq, Ep, False)


class MaxOverPFn(Function):
    @staticmethod
    def forward(ctx, x):
        B, P = x.shape[0], x.shape[1]
        x = x if x.is_contiguous() else x.contiguous()
        inner = x.numel() // (B * P)
        out = torch.empty(B, 1, *x.shape[2:], dtype=x.dtype, device=x.device)
        arg = torch.empty(B * inner, dtype=torch.int32, device=x.device)
        A.call("case_max_over_p_fwd", _ptr(x), _ptr(out), _ptr(arg), B, P, inner, _code(x), _stream())
        ctx.save_for_backward(arg)
        ctx.shape = x.shape
        return out

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        B, P = ctx.shape[0], ctx.shape[1]
        g = g if g.is_contiguous() else g.contiguous()
        dx = torch.empty(ctx.shape, dtype=g.dtype, device=g.device)
        A.call("case_max_over_p_bwd", _ptr(g), _ptr(arg), _ptr(dx), B, P, dx.numel() // (B * P), _code(g), _stream())
        return dx


def max_over_p(x):
    return MaxOverPFn.apply(x)


# ----------------------------------------------------------------------------------------------
# K7 additive attention scores
# ----------------------------------------------------------------------------------------------
class AdditiveScoresFn(Function):
    @staticmethod
    def forward(ctx, wq, uh, v):
        """wq f32 [B, T, H]; uh [B, S, H] (compute dtype); v f32 [H] -> s f32 [B, T, S]."""
        B, T, H = wq.shape
        S = uh.shape[1]
        wq = wq.float().contiguous()
        uh = uh if uh.is_contiguous() else uh.contiguous()
        vv = v.detach().float().contiguous()
        s = torch.empty(B, T, S, dtype=torch.float32, device=wq.device)
        A.call("case_additive_scores_fwd", _ptr(wq), _ptr(uh), _ptr(vv), _ptr(s), B, T, S, H, _code(uh), _stream())
        ctx.save_for_backward(wq, uh, vv)
        return s

    @staticmethod
    def backward(ctx, ds):
        wq, uh, vv = ctx.saved_tensors
        B, T, H = wq.shape
        S = uh.shape[1]
        ds = ds.float().contiguous()
        d_wq = torch.empty_like(wq)
        d_uh = torch.empty(B, S, H, dtype=torch.float32, device=wq.device)
        d_v = _zeros_like_shapes(wq.device, (H,))[0]
        A.call("case_additive_scores_bwd", _ptr(ds), _ptr(wq), _ptr(uh), _ptr(vv), _ptr(d_wq), _ptr(d_uh), _ptr(d_v), B, T, S, H,
               _code(uh), _stream())
        return d_wq, cast(d_uh, uh.dtype), d_v


def additive_scores(wq, uh, v):
    return AdditiveScoresFn.apply(wq, uh, v)


# ----------------------------------------------------------------------------------------------
# K11 pointer scatter / K12 NLL / K13 argmax
# ----------------------------------------------------------------------------------------------
# K22: the greedy step's additive attention (scores + masked softmax + prior renormalisation + context) as one launch over the cached
# e^{2 uh} rows (csrc/attn_pointer.hip).  "auto": bf16 memories of width 512, batches of >= POINTER_FUSED_MIN_BATCH items (one workgroup
# per item: a small batch is faster on the multi-workgroup kernels); "off": scores -> softmax -> cast -> product.
POINTER_FUSED = os.environ.get("CASE_POINTER_FUSED", "auto")
POINTER_FUSED_MIN_BATCH = 96


def pointer_decode_supported(memory):
    return (POINTER_FUSED != "off" and torch.is_tensor(memory) and memory.is_cuda and memory.dtype == torch.bfloat16 and memory.dim() == 3
            and memory.shape[2] == 512 and memory.shape[1] <= 28000 and memory.shape[0] >= POINTER_FUSED_MIN_BATCH
            and not torch.is_grad_enabled()  # (no autograd Function behind K22)
            and bool(A.lib.case_abi_features() & A.FEAT_POINTER_DECODE))


def additive_key_exp(uh):
    """uh f32 [..., H] (the key projection Wk k) -> bf16 e^{2 uh}, the form ops.pointer_attend_decode streams (no autograd)."""
    uh = uh.detach()
    uh = uh if uh.is_contiguous() else uh.contiguous()
    eu = torch.empty(uh.shape, dtype=torch.bfloat16, device=uh.device)
    A.call("case_additive_key_exp", _ptr(uh), _ptr(eu), uh.numel(), _stream())
    return eu


def pointer_attend_decode(wq, eu, v, value, col_valid=None, row_valid=None, prior=None, wq_add=None):
    """wq f32 [B, H] (+ wq_add f32 [B, H]: a step-invariant part of the query projection, added in the kernel); eu / value bf16 [B, S, H]; v f32 [H];
    masks bool; prior f32 [B, S] -> (ctx bf16 [B, H], p f32 [B, S], copy f32 [B, S] | None)."""
    B, S, H = value.shape
    wq = wq.reshape(B, H)
    wq = wq if wq.is_contiguous() else wq.contiguous()
    if wq_add is not None:
        wq_add = wq_add.reshape(B, H)
        if wq_add.dtype != torch.float32 or not wq_add.is_contiguous():
            raise TypeError("pointer_attend_decode: wq_add must be a contiguous f32 [B, H]")
    ctx = torch.empty(B, H, dtype=torch.bfloat16, device=value.device)
    p = torch.empty(B, S, dtype=torch.float32, device=value.device)
    copy = torch.empty_like(p) if prior is not None else None
    if prior is not None:
        prior = prior.reshape(B, S).float()
        prior = prior if prior.is_contiguous() else prior.contiguous()
    A.call("case_pointer_attend_decode", _ptr(wq), _ptr(wq_add), _ptr(eu), _ptr(v), _ptr(value), _ptr(_u8(col_valid)), _ptr(_u8(row_valid)), _ptr(prior),
           _ptr(ctx), _ptr(p), _ptr(copy), B, S, H, _stream())
    return ctx, p, copy


# K23: the greedy step's head (vocabulary softmax, mixing softmax, p0 x gen + pointer scatter, argmax) as one launch with the vocabulary
# row in LDS (V <= 36000) or, in the wide form, in a device-memory workspace (V <= 131071).  "auto": a device-sorted source map, <= 4
# memories, inference; "off": the separate launches.
POINTER_HEAD = os.environ.get("CASE_POINTER_HEAD", "auto")
HEAD_LDS_MAX_V = 36000  # K23 / K24 / K28 with the f32 vocabulary row in LDS
HEAD_WIDE_MAX_V = 131071  # the wide forms with a built row: the SortedSource key format
SAMPLE_WIDE_MAX_V = 1 << 24  # the wide K28 on a ready distribution: 2^24 fixed-point masses below 2^40 cannot overflow a 64-bit sum


def pointer_head_wide_supported():
    return bool(A.lib.case_abi_features() & A.FEAT_POINTER_HEAD_WIDE)


def pointer_head_supported(source_map, V, nmem):
    return (POINTER_HEAD != "off" and isinstance(source_map, SortedSource) and 1 <= nmem <= 4
            and (V <= HEAD_LDS_MAX_V or (V <= HEAD_WIDE_MAX_V and pointer_head_wide_supported()))
            and not torch.is_grad_enabled()  # (no autograd Function behind K23)
            and bool(A.lib.case_abi_features() & A.FEAT_POINTER_HEAD))


def head_row_form(V, row="auto", who="pointer_head"):
    """Where a head launch keeps its vocabulary row: "lds" (the LDS kernels, V <= 36000) or "global" (the wide kernels).  ``row`` = "auto"
    is the LDS form wherever it fits and the wide form above; "lds" beyond 36000 is a ValueError."""
    if row not in ("auto", "lds", "global"):
        raise ValueError("%s: row must be 'auto', 'lds' or 'global' (got %r)" % (who, row))
    if row == "lds" and V > HEAD_LDS_MAX_V:
        raise ValueError("%s: row='lds' holds V <= %d in LDS (V %d)" % (who, HEAD_LDS_MAX_V, V))
    if row == "auto":
        row = "lds" if V <= HEAD_LDS_MAX_V else "global"
    if row == "global" and not pointer_head_wide_supported():
        raise RuntimeError("%s: this build of the library lacks the wide heads (CASE_FEAT_POINTER_HEAD_WIDE)" % who)
    return row


def _row_workspace(rows, V, dev):
    """The wide heads' row workspace f32 [rows, row_stride]: -> (tensor, row_stride), row_stride the next multiple of 4 (the allocator's
    blocks are 16-byte aligned and beyond)."""
    stride = (V + 3) & ~3
    return torch.empty(rows, stride, dtype=torch.float32, device=dev), stride


LINEAR_SKINNY = os.environ.get("CASE_LINEAR_SKINNY", "auto")  # "off": torch.cat + the GEMM path (A/B)


def linear_skinny_supported(xs, w, with_grad=False):
    """``with_grad``: for ``linear_skinny_grad`` (the same forward with autograd behind it); otherwise inference under no_grad only."""
    return (LINEAR_SKINNY != "off" and 1 <= len(xs) <= 4 and 1 <= w.shape[0] <= 8 and (with_grad or not torch.is_grad_enabled())
            and all(x.is_cuda and x.dtype == xs[0].dtype and x.shape[:-1] == xs[0].shape[:-1] for x in xs)
            and xs[0].dtype in (torch.float32, torch.bfloat16) and sum(x.shape[-1] for x in xs) == w.shape[1]
            and bool(A.lib.case_abi_features() & A.FEAT_LINEAR_SKINNY))


def linear_skinny(xs, w, b=None):
    """Linear(sum widths, nout <= 8) on the column-wise concatenation of ``xs`` (1-4 tensors [..., width_k] of one dtype) WITHOUT forming it:
    f32 [..., nout].  Weights and bias are used in f32 as they are (no bf16 copy).  No autograd (inference)."""
    xs = [x if x.is_contiguous() else x.contiguous() for x in xs]
    n = len(xs)
    rows = xs[0].numel() // xs[0].shape[-1]
    ptrs = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
    widths = (C.c_int64 * n)(*[x.shape[-1] for x in xs])
    w32 = w.detach().float().contiguous()
    b32 = None if b is None else b.detach().float().contiguous()
    y = torch.empty(*xs[0].shape[:-1], w.shape[0], dtype=torch.float32, device=xs[0].device)
    A.call("case_linear_skinny", C.cast(ptrs, C.c_void_p), C.cast(widths, C.c_void_p), n, _ptr(w32), _ptr(b32), _ptr(y), rows, w.shape[0], _code(xs[0]),
           _stream())
    return y


class LinearSkinnyFn(Function):
    """``linear_skinny`` with autograd: the forward is the same launch (the same bits as the no_grad pass), the backward the two GEMMs of
    ``LinearFn`` on the concatenated inputs -- dX = g W split by the inputs' widths, dW = g^T cat(xs) with the bias gradient beside it."""

    @staticmethod
    def forward(ctx, w, b, *xs):
        xs = [x if x.is_contiguous() else x.contiguous() for x in xs]
        ctx.save_for_backward(w, *xs)
        ctx.has_b = b is not None
        return linear_skinny(xs, w, b)

    @staticmethod
    def backward(ctx, g):
        w, xs = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        N, K = w.shape
        x2 = torch.cat([x.reshape(-1, x.shape[-1]) for x in xs], dim=-1)
        M = x2.shape[0]
        g2 = cast(g.reshape(M, N).contiguous(), x2.dtype)
        dxs = [None] * len(xs)
        if any(ctx.needs_input_grad[2:]):
            dx = _input_grad(g2, cast_param(w, x2.dtype), M, K, N)
            dxs = [d.reshape(x.shape) for d, x in zip(dx.split([x.shape[-1] for x in xs], dim=-1), xs)]
        dw = db = None
        want_w, want_b = ctx.needs_input_grad[0], ctx.has_b and ctx.needs_input_grad[1]
        if want_w and want_b:
            dw, db = _zeros_like_shapes(g2.device, (N, K), (N,))
            _weight_grad(g2, x2, N, K, out=dw, bias_out=db)
        elif want_w:
            dw = _weight_grad(g2, x2, N, K)
        elif want_b:
            db = _colsum(g2)
        return (dw, db) + tuple(dxs)


def linear_skinny_grad(xs, w, b=None):
    """``linear_skinny`` (same kernel, same bits) as a differentiable op, for a scoring pass that is differentiated."""
    return LinearSkinnyFn.apply(w, b, *xs)


def _head_operands(logits, mix_logits, source_map, copies):
    """What every pointer-head launch takes: contiguous f32 logits and mixing logits, the f32 copy weights (kept alive by the caller until the
    call), their device pointers and lengths as C arrays, the number of memories and the source length S."""
    logits = logits if logits.is_contiguous() else logits.contiguous()
    mix_logits = mix_logits.float().contiguous()
    cs = [c.float().contiguous() for c in copies]
    n = len(cs)
    ptrs = (C.c_void_p * n)(*[c.data_ptr() for c in cs])
    lens = (C.c_int64 * n)(*[c.shape[-1] for c in cs])
    return logits, mix_logits, cs, C.cast(ptrs, C.c_void_p), C.cast(lens, C.c_void_p), n, source_map.keys.shape[1]


ID_MAX_T = 256  # a row of token ids that one wave holds: 4 words of 64 positions (csrc/id_rows.h)
NGRAM_MAX_T = ID_MAX_T  # K32 stages a history in LDS (beside the vocabulary row in the LDS heads); K33 and the n-gram metrics stage rows as long


def _ban_operands(ban, rows, who, own_eos=True):
    """``ban`` = (hist int32 [rows, Tmax] contiguous, t, n, eos | None) -> the history operands of an entry point (K32): hist, Tmax, t, n, eos.
    ``own_eos=False`` (the sampler, whose loop's ``eos`` serves): ``ban`` = (hist, t, n) and no eos operand."""
    (hist, t, n, eos) = ban if own_eos else tuple(ban) + (None,)
    if hist.dtype != torch.int32 or hist.dim() != 2 or hist.shape[0] != rows or not hist.is_contiguous():
        raise TypeError("%s: the history must be a contiguous int32 [%d, Tmax]" % (who, rows))
    if int(n) < 1 or not 0 <= int(t) < hist.shape[1] or int(t) > NGRAM_MAX_T:
        raise ValueError("%s: n >= 1 and 0 <= t < min(Tmax, %d + 1) (got n %r, t %r, Tmax %d)" % (who, NGRAM_MAX_T, n, t, hist.shape[1]))
    return (_ptr(hist), hist.shape[1], int(t), int(n)) + ((-1 if eos is None else int(eos),) if own_eos else ())


# The decoding rules on the mixed distribution row (behind K32, before the argmax / top-W / draw): ``min_length`` zeroes row[eos] while
# t < min_length, ``banned`` zeroes the listed ids at every step.  The limits of both, in one place: a list holds at most RULES_MAX_BANNED ids
# per item; the rules need no history and have no step bound (NGRAM_MAX_T binds a pass only when the n-gram ban is on as well).
RULES_MAX_BANNED = 256
RowRules = collections.namedtuple("RowRules", "eos t min_length banned rows_per_item")
RowRules.__doc__ = """What a head launch takes as ``rules=``: ``eos`` (the id ``min_length`` keeps out; -1: none), ``t`` (the 0-based step = the tokens
a row has emitted), ``min_length`` (0 = off), ``banned`` (None, or a contiguous int32 [K] / [items, K] tensor on the rows' device, K <= 256; entries
outside [0, V) are ignored) and ``rows_per_item`` (rows r of item r // rows_per_item share that item's list).  ``row_rules`` makes one per pass;
``rules._replace(t=t)`` is the step's."""


def decode_rules_supported():
    return bool(A.lib.case_abi_features() & A.FEAT_DECODE_RULES)


def row_rules(eos, min_length=0, banned=None, rows_per_item=1, t=0):
    """The checked ``RowRules`` of a pass (made once, not per step): ``banned`` must already be an int32 tensor [K] or [items, K]."""
    min_length, rows_per_item = int(min_length), int(rows_per_item)
    if min_length < 0 or rows_per_item < 1:
        raise ValueError("row_rules: min_length >= 0 and rows_per_item >= 1 (got %d, %d)" % (min_length, rows_per_item))
    if banned is not None:
        _check_banned(banned, "row_rules")
        if banned.numel() == 0:
            banned = None
    return RowRules(-1 if eos is None else int(eos), int(t), min_length, banned, rows_per_item)


def _check_banned(banned, who):
    """``banned`` is an int32 tensor [K] or [items, K] the kernels can read, K <= RULES_MAX_BANNED -> K."""
    if not torch.is_tensor(banned) or banned.dtype != torch.int32 or banned.dim() not in (1, 2) or not banned.is_contiguous():
        raise TypeError("%s: banned must be a contiguous int32 tensor [K] or [items, K]" % who)
    if banned.shape[-1] > RULES_MAX_BANNED:
        raise ValueError("%s: at most %d banned ids per item (got %d)" % (who, RULES_MAX_BANNED, banned.shape[-1]))
    return banned.shape[-1]


def _rule_operands(rules, rows, who):
    """``rules`` (a ``RowRules``) -> (t, the trailing arguments of a ``_rules`` entry point: eos, min_length, banned, K, item stride, rows_per_item)."""
    if not isinstance(rules, RowRules):
        raise TypeError("%s: rules must be an ops.RowRules (ops.row_rules(...))" % who)
    eos, t, min_length, banned, rpi = rules
    if int(t) < 0 or int(min_length) < 0 or int(rpi) < 1:
        raise ValueError("%s: t >= 0, min_length >= 0 and rows_per_item >= 1 (got %r, %r, %r)" % (who, t, min_length, rpi))
    K = stride = 0
    if banned is not None:
        K = _check_banned(banned, who)
        if banned.dim() == 2:
            if rows % int(rpi) or banned.shape[0] * int(rpi) != rows:
                raise ValueError("%s: %d rows, %d lists, rows_per_item %d" % (who, rows, banned.shape[0], rpi))
            stride = K
    return int(t), (int(eos), int(min_length), _ptr(banned) if K else None, K, stride, int(rpi))


def head_entry(head, row, has_ban, has_rules):
    """The C entry point of a fused head call: ``head`` "decode" (K23) | "beam" (K24) | "sample" (K28), ``row`` "lds" | "global"."""
    return "case_pointer_head_" + head + ("_wide" if row == "global" else "") + ("_rules" if has_rules else "_ban" if has_ban and row == "lds" else "")


def _head_tail(head, row, ban, rules, rows, V, dev, who, own_eos=True, in_place=False):
    """What follows a head's own operands: -> (the entry point's name, its trailing operands up to the stream, the row workspace to keep alive
    until the call returns).  The tail is the workspace and its stride (a global row; NULL, 0 for a row read ``in_place``), the history
    operands (``_ban_operands``; NULL with n = 0 where the entry point takes them and there is no ban) and the rule operands."""
    t, rule = _rule_operands(rules, rows, who) if rules is not None else (0, ())
    if ban is not None:
        hist = _ban_operands(ban, rows, who, own_eos)
        if rules is not None and hist[2] != t:
            raise ValueError("%s: the ban's step %d and the rules' step %d differ" % (who, hist[2], t))
    else:
        hist = (None, 0, t, 0) + ((-1,) if own_eos else ()) if (rules is not None or row == "global") else ()
    ws, stride = _row_workspace(rows, V, dev) if row == "global" and not in_place else (None, 0)
    return head_entry(head, row, ban is not None, rules is not None), ((_ptr(ws), stride) if row == "global" else ()) + hist + rule, ws


def pointer_head_decode(logits, mix_logits, source_map, copies, want_gen=True, want_dist=True, ban=None, row="auto", rules=None):
    """logits f32 [B, V]; mix_logits f32 [B, 1 + nmem]; source_map a SortedSource over the concatenated memories; copies: list of f32
    [B, len_k] pointer weights -> (gen [B, V] | None, dist [B, V] | None, ids [B] int64) (no autograd: inference).
    ``ban`` = (hist int32 [B, Tmax], t, n, eos | None): K32, the n-gram ban before the argmax; the kernel appends ids at hist[:, t].
    ``row``: "auto" | "lds" | "global" (``head_row_form``); both forms return the same bits wherever both run.
    ``rules`` (a ``RowRules``): min_length / banned ids zeroed behind the ban, before the argmax; with rules the ban is optional and, without
    one, nothing is appended anywhere.  A row left all zero returns id 0."""
    B, V = logits.shape
    row = head_row_form(V, row, "pointer_head_decode")
    logits, mix_logits, cs, ptrs, lens, n, S = _head_operands(logits, mix_logits, source_map, copies)
    gen = torch.empty(B, V, dtype=torch.float32, device=logits.device) if want_gen else None
    dist = torch.empty(B, V, dtype=torch.float32, device=logits.device) if want_dist else None
    ids = torch.empty(B, dtype=torch.int64, device=logits.device)
    entry, tail, ws = _head_tail("decode", row, ban, rules, B, V, logits.device, "pointer_head_decode")
    A.call(entry, _ptr(logits), _ptr(mix_logits), _ptr(source_map.keys), ptrs, lens, n, _ptr(gen), _ptr(dist), _ptr(ids), None, B, V, S, *tail, _stream())
    return gen, dist, ids


def beam_supported(width):
    return 1 <= width <= 8 and bool(A.lib.case_abi_features() & A.FEAT_BEAM_DECODE)


def pointer_head_topk(logits, mix_logits, source_map, copies, width, want_gen=False, want_dist=False, ban=None, row="auto", rules=None):
    """K24, ``pointer_head_decode`` with a top-``width`` tail: -> (gen [R, V] | None, dist [R, V] | None, cand_p f32 [R, W], cand_id int64 [R, W]),
    the W largest entries of every row in descending order, the lowest id first among equals (no autograd: inference).  ``ban`` as in
    ``pointer_head_decode``, but the history is only read: row b * W + w is the hypothesis of slot w, which ``beam_advance`` maintains.
    ``row`` and ``rules`` as in ``pointer_head_decode`` (a zeroed entry can still be among the W candidates when fewer than W entries are
    positive: its probability is 0.0, which ``beam_advance`` on a flat-history state treats as dead)."""
    R, V = logits.shape
    row = head_row_form(V, row, "pointer_head_topk")
    logits, mix_logits, cs, ptrs, lens, n, S = _head_operands(logits, mix_logits, source_map, copies)
    gen = torch.empty(R, V, dtype=torch.float32, device=logits.device) if want_gen else None
    dist = torch.empty(R, V, dtype=torch.float32, device=logits.device) if want_dist else None
    cand_p = torch.empty(R, width, dtype=torch.float32, device=logits.device)
    cand_id = torch.empty(R, width, dtype=torch.int64, device=logits.device)
    entry, tail, ws = _head_tail("beam", row, ban, rules, R, V, logits.device, "pointer_head_topk")
    A.call(entry, _ptr(logits), _ptr(mix_logits), _ptr(source_map.keys), ptrs, lens, n, _ptr(gen), _ptr(dist), _ptr(cand_p), _ptr(cand_id), R, V, S, width,
           *tail, _stream())
    return gen, dist, cand_p, cand_id


def sample_supported(V):
    """K28 can draw from a distribution row of V entries: in LDS up to 36000, from device memory (the wide form) beyond."""
    return (V <= HEAD_LDS_MAX_V or (V <= SAMPLE_WIDE_MAX_V and pointer_head_wide_supported())) and bool(A.lib.case_abi_features() & A.FEAT_SAMPLE_DECODE)


def pointer_head_sample(logits, mix_logits, source_map, copies, ended, t_first, t_last, eos, unk, pad, temperature, top_k, top_p, rng=None,
                        uniforms=None, dist_in=None, want_gen=False, want_dist=False, ban=None, row="auto", rules=None):
    """K28, ``pointer_head_decode`` with a draw instead of the argmax: -> (gen [R, V] | None, dist [R, V] | None, ids int64 [R], prob f32 [R]).
    One token per row is drawn from the mixed distribution after temperature, top-k and top-p (the rule: include/case_hip.h); ``ids`` is what
    the reference's ``sample`` loop emits for it (UNK for EOS at the first step, EOS at the last, PAD behind the end) and ``ended`` (uint8 [R])
    is updated in place; ``prob`` is the row's unfiltered probability of the drawn token, 1 for a row that had ended.  The uniform of row r is
    ``uniforms[r]`` (f32 [R]) when given, else the 24-bit counter uniform of ``rng = (seed, offset, state)`` (what ``config.next_rng(R)`` returns)
    at counter ``rng_base + offset + r``.  ``dist_in`` f32 [R, V] with ``logits=None`` draws from a ready distribution instead of building the row
    (``mix_logits`` / ``source_map`` / ``copies`` unused).  ``ban`` = (hist int32 [R, Tmax], t, n): K32, the n-gram ban before pmax, the cuts and
    the draw (either row source; no ban for a row that has ended or whose history holds ``eos``); the kernel appends ``ids`` at hist[:, t].
    ``row`` as in ``pointer_head_decode``; the wide form reads an aligned ``dist_in`` where it lies (V a multiple of 4, no ban, no rules).
    ``rules`` (a ``RowRules``; its ``eos`` is the rule's own, ``eos`` above stays the loop's): min_length / banned ids zeroed behind the ban, before
    pmax, the cuts and the draw, for every row that has not ended.  No autograd (inference)."""
    if not (float(temperature) > 0.0) or int(top_k) < 0 or not (0.0 < float(top_p) <= 1.0):
        raise ValueError("pointer_head_sample: temperature must be > 0, top_k >= 0 and top_p in (0, 1]")
    if (logits is None) == (dist_in is None):
        raise ValueError("pointer_head_sample: give either the logits or dist_in")
    if uniforms is None and rng is None:
        raise ValueError("pointer_head_sample: give rng=(seed, offset, state) or uniforms")
    src = dist_in if logits is None else logits
    if src.dtype != torch.float32 or src.dim() != 2:
        raise TypeError("pointer_head_sample: the row source must be f32 [R, V]")
    R, V = src.shape
    dev = src.device
    row = head_row_form(V, row, "pointer_head_sample")
    src = src if src.is_contiguous() else src.contiguous()
    if ended.dtype != torch.uint8 or tuple(ended.shape) != (R,) or not ended.is_contiguous():
        raise TypeError("pointer_head_sample: ended must be a contiguous uint8 [R]")
    if uniforms is not None:
        if uniforms.dtype != torch.float32 or tuple(uniforms.shape) != (R,):
            raise TypeError("pointer_head_sample: uniforms must be f32 [R]")
        uniforms = uniforms if uniforms.is_contiguous() else uniforms.contiguous()
    seed, offset, state = rng if rng is not None else (0, 0, None)
    gen = torch.empty(R, V, dtype=torch.float32, device=dev) if (want_gen and logits is not None) else None
    dist = torch.empty(R, V, dtype=torch.float32, device=dev) if want_dist else None
    ids = torch.empty(R, dtype=torch.int64, device=dev)
    prob = torch.empty(R, dtype=torch.float32, device=dev)
    tail = (_ptr(gen), _ptr(dist), _ptr(ids), _ptr(prob), _ptr(ended), _ptr(uniforms), R, V)
    draw = (float(temperature), min(int(top_k), 2 ** 31 - 1), float(top_p), int(seed), int(offset), state, int(eos), int(unk), int(pad),
            int(bool(t_first)), int(bool(t_last)))
    in_place = rules is None and logits is None and ban is None and V % 4 == 0 and src.data_ptr() % 16 == 0  # (the wide form alone asks)
    entry, hist, ws = _head_tail("sample", row, ban, rules, R, V, dev, "pointer_head_sample", own_eos=False, in_place=in_place)
    if logits is None:
        A.call(entry, None, None, None, None, None, 0, _ptr(src), *tail, 0, *draw, *hist, _stream())
    else:
        src, mix_logits, cs, ptrs, lens, n, S = _head_operands(src, mix_logits, source_map, copies)
        A.call(entry, _ptr(src), _ptr(mix_logits), _ptr(source_map.keys), ptrs, lens, n, None, *tail, S, *draw, *hist, _stream())
    return gen, dist, ids, prob


# K29: the head of a teacher-forced scoring pass (one probability per row, no vocabulary row).  "auto": a device-sorted source map, <= 4
# memories, no grad; "off": the unfused differentiable chain (masked_softmax, p0 x gen, sorted scatter, add, gather).
POINTER_SCORE = os.environ.get("CASE_POINTER_SCORE", "auto")


def pointer_score_supported(source_map, nmem):
    return (POINTER_SCORE != "off" and isinstance(source_map, SortedSource) and 1 <= nmem <= 4
            and not torch.is_grad_enabled()  # (no autograd Function behind K29)
            and bool(A.lib.case_abi_features() & A.FEAT_POINTER_SCORE))


def pointer_head_score(logits, mix_logits, source_map, rows_per_source, copies, targets, pad=0):
    """K29: logits f32 [R, V]; mix_logits f32 [R, 1 + nmem]; source_map a SortedSource with R / rows_per_source rows (row r reads key row
    r // rows_per_source); copies: list of f32 [R, len_k]; targets int64 [R] -> (prob f32 [R], copy f32 [R]): the mixed pointer-generator
    probability of every row's target and its pointer part.  ``targets == pad`` (pad -1: none) gives (1, 0), an id outside [0, V) (0, 0).
    No autograd (inference)."""
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise TypeError("pointer_head_score: logits must be f32 [R, V]")
    R, V = logits.shape
    rows_per_source = int(rows_per_source)
    keys = source_map.keys
    if rows_per_source < 1 or R % rows_per_source or keys.shape[0] * rows_per_source != R:
        raise ValueError("pointer_head_score: %d rows, %d key rows, rows_per_source %d" % (R, keys.shape[0], rows_per_source))
    if targets.dtype != torch.int64 or targets.numel() != R:
        raise TypeError("pointer_head_score: targets must be int64 [R]")
    if tuple(mix_logits.shape) != (R, len(copies) + 1):
        raise ValueError("pointer_head_score: mix_logits must be [R, 1 + nmem]")
    if any(c.dim() != 2 or c.shape[0] != R for c in copies):
        raise ValueError("pointer_head_score: every copies[k] must be [R, len_k]")
    logits, mix_logits, cs, ptrs, lens, n, S = _head_operands(logits, mix_logits, source_map, copies)
    targets = targets.reshape(R).contiguous()
    prob = torch.empty(R, dtype=torch.float32, device=logits.device)
    copy = torch.empty(R, dtype=torch.float32, device=logits.device)
    A.call("case_pointer_head_score", _ptr(logits), _ptr(mix_logits), _ptr(keys), rows_per_source, ptrs, lens, n, _ptr(targets), int(pad), _ptr(prob),
           _ptr(copy), R, V, S, _stream())
    return prob, copy


# K41: K29 with autograd behind it, for a scoring pass that is differentiated (minimum-risk training).  The forward is K29's kernel with the
# row's (max, sum) kept; the backward is one launch that writes the gradient of the logits, of the mixing logits and of every memory's copy
# weights.  ``pointer_score_supported`` / ``pointer_head_score`` stay the no-grad pair: only a caller that asks for this head gets it.
def pointer_score_grad_supported(source_map, nmem):
    return (POINTER_SCORE != "off" and isinstance(source_map, SortedSource) and 1 <= nmem <= 4
            and bool(A.lib.case_abi_features() & A.FEAT_RISK_TRAIN))


def _copy_pointers(tensors):
    return C.cast((C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors]), C.c_void_p)


def pointer_head_score_bwd(logits, mix_logits, ids, rows_per_source, copies, targets, pad, stats, prob, g, out=None):
    """K41 as a plain launch: contiguous f32 logits [R, V], mix_logits [R, 1 + nmem], copies [R, len_k], stats [R, 2], prob [R] and g [R];
    ids int64 [R / rows_per_source, S] (``SortedSource.ids``); targets int64 [R] -> (d_logits [R, V], d_mix [R, 1 + nmem], [d_copy_k
    [R, len_k]]), every element written.  ``out``: that triple as buffers to write into."""
    R, V = logits.shape
    d_logits, d_mix, d_cs = out if out is not None else (torch.empty_like(logits), torch.empty_like(mix_logits), [torch.empty_like(c) for c in copies])
    for t in [logits, mix_logits, stats, prob, g, d_logits, d_mix] + list(copies) + list(d_cs):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError("pointer_head_score_bwd: contiguous f32 tensors")
    if (ids.dtype != torch.int64 or not ids.is_contiguous() or ids.shape[0] * rows_per_source != R or targets.dtype != torch.int64 or targets.numel() != R
            or tuple(mix_logits.shape) != (R, len(copies) + 1) or tuple(stats.shape) != (R, 2) or prob.numel() != R or g.numel() != R
            or d_logits.shape != logits.shape or d_mix.shape != mix_logits.shape or len(d_cs) != len(copies)
            or any(c.shape != d.shape or c.dim() != 2 or c.shape[0] != R for c, d in zip(copies, d_cs))):
        raise ValueError("pointer_head_score_bwd: shapes do not fit R = %d rows of V = %d" % (R, V))
    lens = C.cast((C.c_int64 * len(copies))(*[c.shape[1] for c in copies]), C.c_void_p)
    A.call("case_pointer_head_score_bwd", _ptr(logits), _ptr(mix_logits), _ptr(ids), int(rows_per_source), _copy_pointers(copies), lens, len(copies),
           _ptr(targets), int(pad), _ptr(stats), _ptr(prob), _ptr(g), _ptr(d_logits), _ptr(d_mix), _copy_pointers(d_cs), R, V, ids.shape[1], _stream())
    return d_logits, d_mix, d_cs


class PointerScoreFn(Function):
    @staticmethod
    def forward(ctx, logits, mix_logits, source_map, rows_per_source, targets, pad, *copies):
        R, V = logits.shape
        mix_dtype = mix_logits.dtype
        logits, mix_logits, cs, ptrs, lens, n, S = _head_operands(logits, mix_logits, source_map, copies)
        prob = torch.empty(R, dtype=torch.float32, device=logits.device)
        copy = torch.empty(R, dtype=torch.float32, device=logits.device)
        stats = torch.empty(R, 2, dtype=torch.float32, device=logits.device)
        A.call("case_pointer_head_score_stats", _ptr(logits), _ptr(mix_logits), _ptr(source_map.keys), rows_per_source, ptrs, lens, n, _ptr(targets),
               pad, _ptr(prob), _ptr(copy), _ptr(stats), R, V, S, _stream())
        ctx.save_for_backward(logits, mix_logits, targets, stats, prob, source_map.ids, *cs)
        ctx.meta = (rows_per_source, pad, [c.dtype for c in copies], mix_dtype)
        ctx.mark_non_differentiable(copy, stats)
        return prob, copy, stats

    @staticmethod
    def backward(ctx, g, _g_copy, _g_stats):
        logits, mix_logits, targets, stats, prob, ids = ctx.saved_tensors[:6]
        cs = list(ctx.saved_tensors[6:])
        rows_per_source, pad, copy_dtypes, mix_dtype = ctx.meta
        R, V = logits.shape
        d_logits, d_mix, d_cs = pointer_head_score_bwd(logits, mix_logits, ids, rows_per_source, cs, targets, pad, stats, prob, g.float().contiguous())
        return (d_logits, d_mix.to(mix_dtype), None, None, None, None) + tuple(d.to(dt) for d, dt in zip(d_cs, copy_dtypes))


def pointer_head_score_grad(logits, mix_logits, source_map, rows_per_source, copies, targets, pad=0):
    """``pointer_head_score`` with autograd (K29 with row statistics forward, K41 backward): the same arguments -> (prob f32 [R], copy f32
    [R]) with K29's bits.  ``prob`` is differentiable in ``logits``, ``mix_logits`` and every ``copies[k]``; ``copy`` is not.  The forward
    keeps the logits, the mixing logits, the copy weights, the targets, the row statistics [R, 2] and prob for the backward pass
    (``PointerScoreFn`` itself also returns the statistics: the row's (max, sum exp(logit - max)), (0, 0) for a row that is not scored)."""
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise TypeError("pointer_head_score_grad: logits must be f32 [R, V]")
    if not isinstance(source_map, SortedSource):
        raise TypeError("pointer_head_score_grad: source_map must be a SortedSource")
    if not bool(A.lib.case_abi_features() & A.FEAT_RISK_TRAIN):
        raise RuntimeError("pointer_head_score_grad: this build of the library lacks K41 (CASE_FEAT_RISK_TRAIN)")
    R, V = logits.shape
    rows_per_source = int(rows_per_source)
    keys = source_map.keys
    if rows_per_source < 1 or R % rows_per_source or keys.shape[0] * rows_per_source != R:
        raise ValueError("pointer_head_score_grad: %d rows, %d key rows, rows_per_source %d" % (R, keys.shape[0], rows_per_source))
    if targets.dtype != torch.int64 or targets.numel() != R:
        raise TypeError("pointer_head_score_grad: targets must be int64 [R]")
    if not 1 <= len(copies) <= 4:
        raise ValueError("pointer_head_score_grad: 1 .. 4 memories (got %d)" % len(copies))
    if tuple(mix_logits.shape) != (R, len(copies) + 1):
        raise ValueError("pointer_head_score_grad: mix_logits must be [R, 1 + nmem]")
    if any(c.dim() != 2 or c.shape[0] != R for c in copies):
        raise ValueError("pointer_head_score_grad: every copies[k] must be [R, len_k]")
    if sum(c.shape[1] for c in copies) != keys.shape[1]:
        raise ValueError("pointer_head_score_grad: the memories hold %d positions, the source map %d" % (sum(c.shape[1] for c in copies), keys.shape[1]))
    prob, copy, _ = PointerScoreFn.apply(logits, mix_logits, source_map, rows_per_source, targets.reshape(R).contiguous(), int(pad), *copies)
    return prob, copy


# The loss-only head of the TRAINING step: generator rows -> per-row NLL of the mixed pointer-generator distribution without any dense
# [rows, V] probability tensor.  "auto": wherever the differentiable score head runs (``pointer_score_grad_supported``) and the library
# exports the loss-form kernels; "dense": the chain masked_softmax, p0 x gen, sorted scatter, add, gather.
TRAIN_HEAD = os.environ.get("CASE_TRAIN_HEAD", "auto")
TRAIN_HEAD_PAD = 256  # the vocabulary rows are padded to the edge of the 8-wave GEMM's tile


def train_head_supported(source_map, nmem):
    return (TRAIN_HEAD != "dense" and pointer_score_grad_supported(source_map, nmem)
            and A.has("case_pointer_head_loss") and A.has("case_pointer_head_loss_bwd"))


def pointer_head_loss(logits, V, mix_logits, source_map, rows_per_source, copies, targets, pad=0):
    """The forward loss kernel as a plain launch: logits f32 [R, ld] (ld >= V; columns [V, ld) are not read), contiguous f32 mix_logits
    [R, 1 + nmem] and copies [R, len_k], targets int64 [R] -> (prob, copy, stats [R, 2], nll) with K29's prob / copy / stats bits."""
    R, ld = logits.shape
    for t in [logits, mix_logits] + list(copies):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError("pointer_head_loss: contiguous f32 tensors")
    if (ld < V or source_map.keys.shape[0] * rows_per_source != R or targets.dtype != torch.int64 or targets.numel() != R
            or tuple(mix_logits.shape) != (R, len(copies) + 1) or any(c.dim() != 2 or c.shape[0] != R for c in copies)):
        raise ValueError("pointer_head_loss: shapes do not fit R = %d rows of V = %d (ld %d)" % (R, V, ld))
    dev = logits.device
    prob, copy, nll = (torch.empty(R, dtype=torch.float32, device=dev) for _ in range(3))
    stats = torch.empty(R, 2, dtype=torch.float32, device=dev)
    lens = C.cast((C.c_int64 * len(copies))(*[c.shape[1] for c in copies]), C.c_void_p)
    A.call("case_pointer_head_loss", _ptr(logits), ld, _ptr(mix_logits), _ptr(source_map.keys), int(rows_per_source), _copy_pointers(copies), lens,
           len(copies), _ptr(targets), int(pad), _ptr(prob), _ptr(copy), _ptr(stats), _ptr(nll), R, V, source_map.keys.shape[1], _stream())
    return prob, copy, stats, nll


def pointer_head_loss_bwd(logits, V, mix_logits, ids, rows_per_source, copies, targets, pad, stats, prob, g_nll, dtype=torch.float32, out=None):
    """The backward loss kernel as a plain launch: the operands of ``pointer_head_loss`` (``ids`` = ``SortedSource.ids``), its stats and prob,
    g_nll f32 [R] -> (d_logits ``dtype`` [R, ld] with columns [V, ld) zero, d_mix f32 [R, 1 + nmem], [d_copy_k f32 [R, len_k]]), every element
    written.  ``out``: that triple as buffers to write into."""
    R, ld = logits.shape
    d_logits, d_mix, d_cs = out if out is not None else (torch.empty(R, ld, dtype=dtype, device=logits.device), torch.empty_like(mix_logits),
                                                         [torch.empty_like(c) for c in copies])
    for t in [logits, mix_logits, stats, prob, g_nll, d_mix] + list(copies) + list(d_cs):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError("pointer_head_loss_bwd: contiguous f32 tensors")
    if (ld < V or ld % 8 or ids.dtype != torch.int64 or not ids.is_contiguous() or ids.shape[0] * rows_per_source != R or targets.dtype != torch.int64
            or targets.numel() != R or tuple(mix_logits.shape) != (R, len(copies) + 1) or tuple(stats.shape) != (R, 2) or prob.numel() != R
            or g_nll.numel() != R or tuple(d_logits.shape) != (R, ld) or not d_logits.is_contiguous() or d_mix.shape != mix_logits.shape
            or len(d_cs) != len(copies) or any(c.shape != d.shape or c.dim() != 2 or c.shape[0] != R for c, d in zip(copies, d_cs))):
        raise ValueError("pointer_head_loss_bwd: shapes do not fit R = %d rows of V = %d (ld %d)" % (R, V, ld))
    lens = C.cast((C.c_int64 * len(copies))(*[c.shape[1] for c in copies]), C.c_void_p)
    A.call("case_pointer_head_loss_bwd", _ptr(logits), ld, _ptr(mix_logits), _ptr(ids), int(rows_per_source), _copy_pointers(copies), lens, len(copies),
           _ptr(targets), int(pad), _ptr(stats), _ptr(prob), _ptr(g_nll), _ptr(d_logits), _code(d_logits), _ptr(d_mix), _copy_pointers(d_cs), R, V,
           ids.shape[1], _stream())
    return d_logits, d_mix, d_cs


class TrainHeadFn(Function):
    """h [R, H] (the generator's hidden rows) -> nll f32 [R].  Forward: the vocabulary GEMM into an f32 [R, Vp] buffer against the row-padded
    operand copy of ``w`` (Vp = V rounded up to 256: the 8-wave tiling takes it; the pad columns come out as exact zeros and are never
    read), then the forward loss kernel.  Backward: the backward loss kernel writes d_logits [R, Vp] in the operand dtype with zero pad
    columns, then dX reduces over Vp and dW is computed as [Vp, H] in one unsplit round of tiles -- no zero fill, no atomics -- and
    returned as its contiguous [:V] prefix.  No host synchronisation."""

    @staticmethod
    def forward(ctx, h, w, mix_logits, source_map, rows_per_source, targets, pad, *copies):
        H, V = h.shape[-1], w.shape[0]
        h2 = h.reshape(-1, H)
        h2 = h2 if h2.is_contiguous() else h2.contiguous()
        R = h2.shape[0]
        wp = cast_param_rowpad(w, h2.dtype, TRAIN_HEAD_PAD)
        Vp = wp.shape[0]
        logits = torch.empty(R, Vp, dtype=torch.float32, device=h2.device)
        gemm(h2, wp, logits, R, Vp, H, H, H, Vp)
        mix32 = mix_logits.reshape(R, -1).float().contiguous()
        cs = [c.reshape(R, -1).float().contiguous() for c in copies]
        targets = targets.reshape(R).contiguous()
        prob, _, stats, nll = pointer_head_loss(logits, V, mix32, source_map, rows_per_source, cs, targets, pad)
        ctx.save_for_backward(h2, wp, logits, mix32, targets, stats, prob, source_map.ids, *cs)
        ctx.meta = (h.shape, V, rows_per_source, pad, mix_logits.shape, mix_logits.dtype, [(c.shape, c.dtype) for c in copies])
        return nll

    @staticmethod
    def backward(ctx, g_nll):
        h2, wp, logits, mix32, targets, stats, prob, ids = ctx.saved_tensors[:8]
        cs = list(ctx.saved_tensors[8:])
        hshape, V, rows_per_source, pad, mix_shape, mix_dtype, copy_meta = ctx.meta
        (R, H), Vp = h2.shape, wp.shape[0]
        d_logits, d_mix, d_cs = pointer_head_loss_bwd(logits, V, mix32, ids, rows_per_source, cs, targets, pad, stats, prob,
                                                      g_nll.reshape(R).float().contiguous(), dtype=h2.dtype)
        dh = _input_grad(d_logits, wp, R, H, Vp).view(hshape) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            if _split_for(Vp, H, R, h2.element_size()) == 1:
                dwp = torch.empty(Vp, H, dtype=torch.float32, device=h2.device)
                gemm(d_logits, h2, dwp, Vp, H, R, Vp, H, H, a_kmajor=True, b_kmajor=True)
            else:
                dwp = _weight_grad(d_logits, h2, Vp, H)
            dw = dwp[:V]
        return (dh, dw, d_mix.view(mix_shape).to(mix_dtype), None, None, None, None) + tuple(d.view(sh).to(dt) for d, (sh, dt) in zip(d_cs, copy_meta))


def train_head_nll(h, w, mix_logits, source_map, rows_per_source, copies, targets, pad=0):
    """The loss-only training head (``TrainHeadFn``): h [R, H] of the compute dtype, w the [V, H] vocabulary projection (an nn.Parameter),
    mix_logits [R, 1 + nmem], source_map a SortedSource with R / rows_per_source rows, copies [R, len_k], targets int64 [R] -> nll f32 [R]
    = -log(p(target) + 1e-8), 0 where target == pad; differentiable in h, w, mix_logits and every copies[k]."""
    if not isinstance(source_map, SortedSource) or not 1 <= len(copies) <= 4:
        raise TypeError("train_head_nll: a SortedSource and 1 .. 4 memories")
    if not (A.has("case_pointer_head_loss") and A.has("case_pointer_head_loss_bwd")):
        raise RuntimeError("train_head_nll: this build of the library lacks case_pointer_head_loss / case_pointer_head_loss_bwd")
    R = h.numel() // h.shape[-1]
    rows_per_source = int(rows_per_source)
    if rows_per_source < 1 or source_map.keys.shape[0] * rows_per_source != R or targets.numel() != R or targets.dtype != torch.int64:
        raise ValueError("train_head_nll: %d rows, %d key rows, rows_per_source %d, %d targets" % (R, source_map.keys.shape[0], rows_per_source,
                                                                                               targets.numel()))
    if sum(c.shape[-1] for c in copies) != source_map.keys.shape[1]:
        raise ValueError("train_head_nll: the memories hold %d positions, the source map %d" % (sum(c.shape[-1] for c in copies), source_map.keys.shape[1]))
    return TrainHeadFn.apply(h, w, mix_logits, source_map, rows_per_source, targets, int(pad), *copies)


# K42: the expected cost of a pool of candidates under the renormalised model posterior (evaluation/risk.py states the rule).
RISK_MAX_N, RISK_MAX_T = 64, 1024


def check_risk_alpha(alpha, who="sequence_risk"):
    alpha = float(alpha)
    if not (alpha >= 0.0 and math.isfinite(alpha)):
        raise ValueError("%s: alpha must be >= 0 and finite (got %r)" % (who, alpha))
    return alpha


class SequenceRiskFn(Function):
    @staticmethod
    def forward(ctx, token_probs, scored, cost, valid, alpha):
        B, N, T = token_probs.shape
        p = token_probs.float().contiguous()
        dev = p.device
        risk = torch.empty(B, dtype=torch.float32, device=dev)
        q = torch.empty(B, N, dtype=torch.float32, device=dev)
        grad_p = torch.empty(B, N, T, dtype=torch.float32, device=dev)
        A.call("case_sequence_risk", _ptr(p), _ptr(_u8(scored)), _ptr(cost), _ptr(_u8(valid)), alpha, _ptr(risk), _ptr(q), _ptr(grad_p), B, N, T,
               _stream())
        ctx.save_for_backward(grad_p)
        ctx.in_dtype = token_probs.dtype
        ctx.mark_non_differentiable(q)
        return risk, q

    @staticmethod
    def backward(ctx, g, _g_q):
        (grad_p,) = ctx.saved_tensors
        return (grad_p * g.float().reshape(-1, 1, 1)).to(ctx.in_dtype), None, None, None, None


def sequence_risk(token_probs, scored, cost, valid=None, alpha=5e-3, want_q=False):
    """K42: token_probs f32 [B, N, T] (the model's probability of every token of N candidates per item), scored bool [B, N, T] (the
    positions that count), cost f32 [B, N], valid bool [B, N] or None (all) -> risk f32 [B] = sum_n Q_n cost_n with Q = softmax over the
    valid n of alpha sum_t ln max(p, 1e-30) (``evaluation.risk``; f64 inside, rounded once).  ``risk`` is differentiable in ``token_probs``:
    the forward keeps grad_p [B, N, T], the backward scales it by the upstream [B] gradient.  ``want_q``: (risk, q f32 [B, N]).  N <= 64,
    T <= 1024; an item without a valid candidate has risk 0 and no gradient."""
    if token_probs.dim() != 3 or not token_probs.is_floating_point():
        raise TypeError("sequence_risk: token_probs must be a float tensor [B, N, T]")
    B, N, T = token_probs.shape
    if scored.dtype not in (torch.bool, torch.uint8) or tuple(scored.shape) != (B, N, T):
        raise TypeError("sequence_risk: scored must be bool [B, N, T]")
    if cost.dim() != 2 or tuple(cost.shape) != (B, N) or not cost.is_floating_point():
        raise TypeError("sequence_risk: cost must be a float tensor [B, N]")
    if valid is not None and (valid.dtype not in (torch.bool, torch.uint8) or tuple(valid.shape) != (B, N)):
        raise TypeError("sequence_risk: valid must be bool [B, N]")
    alpha = check_risk_alpha(alpha)
    if N > RISK_MAX_N or T > RISK_MAX_T:
        raise ValueError("sequence_risk: pools of up to %d candidates of up to %d positions (got %d x %d)" % (RISK_MAX_N, RISK_MAX_T, N, T))
    if not bool(A.lib.case_abi_features() & A.FEAT_RISK_TRAIN):
        raise RuntimeError("sequence_risk: this build of the library lacks K42 (CASE_FEAT_RISK_TRAIN)")
    risk, q = SequenceRiskFn.apply(token_probs, scored.contiguous(), cost.detach().float().contiguous(), valid, alpha)
    return (risk, q) if want_q else risk


# K32: the n-gram ban.  The fused heads apply it behind their row build (``ban=`` above); ``ngram_ban_`` is the same rule as a launch of its own.
def ngram_ban_supported():
    return bool(A.lib.case_abi_features() & A.FEAT_NGRAM_BAN)


def ngram_ban_(dist, hist, t, n, eos=None, ended=None):
    """K32 in place on dist f32 [R, V] (contiguous): at step ``t`` with the histories hist int32 [R, Tmax] (BOS excluded), entry v of row r
    becomes 0.0 when some j <= t - n has hist[r, j : j + n - 1] == hist[r, t - n + 1 : t] and hist[r, j + n - 1] == v.  Nothing else changes
    (no renormalisation).  No ban for t < n, a history that holds ``eos``, or a row with ``ended`` (uint8 [R]) set.  -> dist."""
    if dist.dtype != torch.float32 or dist.dim() != 2 or not dist.is_contiguous():
        raise TypeError("ngram_ban_: dist must be a contiguous f32 [R, V]")
    R, V = dist.shape
    if ended is not None and (ended.dtype != torch.uint8 or tuple(ended.shape) != (R,) or not ended.is_contiguous()):
        raise TypeError("ngram_ban_: ended must be a contiguous uint8 [R]")
    hp, Tmax, t, n, eos = _ban_operands((hist, t, n, eos), R, "ngram_ban_")
    A.call("case_ngram_ban", _ptr(dist), hp, _ptr(ended), R, V, Tmax, t, n, eos, _stream())
    return dist


def row_rules_(dist, rules, ended=None):
    """The decoding rules as a launch of their own (the unfused head), in place on dist f32 [R, V] (contiguous): row[eos] = 0.0 while
    ``rules.t < rules.min_length`` and row[v] = 0.0 for every id v of the row's item's list; nothing else changes (no renormalisation).  A row
    with ``ended`` (uint8 [R]) set is left alone.  -> dist."""
    if dist.dtype != torch.float32 or dist.dim() != 2 or not dist.is_contiguous():
        raise TypeError("row_rules_: dist must be a contiguous f32 [R, V]")
    R, V = dist.shape
    if ended is not None and (ended.dtype != torch.uint8 or tuple(ended.shape) != (R,) or not ended.is_contiguous()):
        raise TypeError("row_rules_: ended must be a contiguous uint8 [R]")
    t, rule = _rule_operands(rules, R, "row_rules_")
    A.call("case_row_rules", _ptr(dist), _ptr(ended), R, V, t, *rule, _stream())
    return dist


def remove_duplicate_ids(out, len, n=3, pad=0):
    """K33: the reference's ``remove_duplicate`` on ``sentence_compact``'s outputs, in place: out int64 [B, T] front-packed ids, len int32 [B].
    Per row, while the length L > n: cut at the largest i in [1, L - n] whose tail out[i:L] holds only tokens of out[:i].  PAD behind the new
    length, ``len`` updated.  T <= 256.  -> (out, len)."""
    if out.dtype != torch.int64 or out.dim() != 2 or not out.is_contiguous():
        raise TypeError("remove_duplicate_ids: out must be a contiguous int64 [B, T]")
    B, T = out.shape
    if len.dtype != torch.int32 or tuple(len.shape) != (B,) or not len.is_contiguous():
        raise TypeError("remove_duplicate_ids: len must be a contiguous int32 [B]")
    if int(n) != n or n < 1:
        raise ValueError("remove_duplicate_ids: n must be an integer >= 1, not %r" % (n,))
    if T > NGRAM_MAX_T:
        raise ValueError("remove_duplicate_ids: rows of up to %d positions (got %d)" % (NGRAM_MAX_T, T))
    A.call("case_remove_duplicate_ids", _ptr(out), _ptr(len), B, T, int(n), int(pad), _stream())
    return out, len


class BeamState(object):
    """The device-side state of one beam-search pass over B items x W slots and at most T steps: what K25 rewrites every step (``parent``,
    ``token``, ``cum``, ``len``, ``alive``), the [T, B, W] history K27 walks back, and the finished pool (best W retired hypotheses per item).
    ``flat=True`` adds the flat history of the n-gram ban (K32): int32 [2, B, W, T], every slot's hypothesis so far; step t reads buffer t % 2
    (``flat_rows(t)``: what K24 takes) and K25 writes buffer (t + 1) % 2."""

    def __init__(self, B, W, T, device, flat=False):
        self.B, self.W, self.T = B, W, T
        self.flat = torch.zeros(2, B, W, T, dtype=torch.int32, device=device) if flat else None
        self.alive = torch.zeros(B, W, dtype=torch.uint8, device=device)
        self.alive[:, 0] = 1  # the root: BOS in slot 0, cost 0, length 1
        self.cum = torch.zeros(B, W, dtype=torch.float32, device=device)
        self.len = torch.ones(B, W, dtype=torch.int32, device=device)
        self.parent = torch.zeros(B, W, dtype=torch.int32, device=device)
        self.token = torch.zeros(B, W, dtype=torch.int64, device=device)
        self.hist_parent = torch.zeros(T, B, W, dtype=torch.int32, device=device)
        self.hist_token = torch.zeros(T, B, W, dtype=torch.int64, device=device)
        self.fin_key = torch.full((B, W), float("inf"), dtype=torch.float32, device=device)
        self.fin_step = torch.full((B, W), -1, dtype=torch.int32, device=device)
        self.fin_slot = torch.zeros(B, W, dtype=torch.int32, device=device)


    def flat_rows(self, t):
        """The hypotheses the rows of step ``t`` continue: int32 [B * W, T], positions 0 .. t - 1 filled."""
        return self.flat[t % 2].view(self.B * self.W, self.T)


def beam_advance(state, cand_p, cand_id, t, eos, length_penalty=1.0):
    """K25: step ``t`` of the search on ``state`` (in place) from the candidates cand_p f32 / cand_id int64 [B * W, W] of the step's rows.  A state
    with the flat history gets it advanced in the same launch (and there a candidate of probability 0, a banned entry, is dead).
    ``length_penalty`` = alpha >= 0: the key of a candidate and of a retiring hypothesis is cost / (len + 1)^alpha; 1.0 is the reference's
    cost / (len + 1), the same launch as without the argument; any other value needs a flat-history state."""
    alpha = float(length_penalty)
    if not (alpha >= 0.0) or alpha == float("inf"):
        raise ValueError("beam_advance: length_penalty must be a finite float >= 0, not %r" % (length_penalty,))
    if alpha != 1.0 and state.flat is None:
        raise ValueError("beam_advance: a length_penalty other than 1.0 needs a BeamState with the flat history (flat=True)")
    B, W = state.B, state.W
    if tuple(cand_p.shape) != (B * W, W) or tuple(cand_id.shape) != (B * W, W) or cand_p.dtype != torch.float32 or cand_id.dtype != torch.int64:
        raise TypeError("beam_advance: candidates must be f32 / int64 [B * W, W]")
    cand_p = cand_p if cand_p.is_contiguous() else cand_p.contiguous()
    cand_id = cand_id if cand_id.is_contiguous() else cand_id.contiguous()
    args = (_ptr(cand_p), _ptr(cand_id), _ptr(state.alive), _ptr(state.cum), _ptr(state.len), _ptr(state.parent), _ptr(state.token),
            _ptr(state.hist_parent), _ptr(state.hist_token), _ptr(state.fin_key), _ptr(state.fin_step), _ptr(state.fin_slot), t, state.T, B, W,
            -1 if eos is None else eos)
    flat = () if state.flat is None else (_ptr(state.flat[t % 2]), _ptr(state.flat[(t + 1) % 2]), state.T) + ((alpha,) if alpha != 1.0 else ())
    A.call("case_beam_advance" + ("" if state.flat is None else "_rules" if alpha != 1.0 else "_ban"), *args, *flat, _stream())


def beam_gather(src, dst, parent, t, valid_src=None, valid_dst=None):
    """K26: dst[l][b * W + w, :t + 1] = src[l][b * W + parent[b, w], :t + 1] for the caches ``src`` / ``dst`` (lists of [B * W, Tmax, 2E] tensors, one
    pair of different buffers per layer) in one launch, and the same for the bool prefix validity [B * W, Tmax] when given."""
    B, W = parent.shape
    n = len(src)
    first = src[0]
    for s, d in zip(src, dst):
        if not (s.is_contiguous() and d.is_contiguous() and s.shape == first.shape == d.shape and s.dtype == first.dtype == d.dtype
                and s.shape[0] == B * W):
            raise TypeError("beam_gather: every cache must be a contiguous [B * W, Tmax, 2E] tensor of one shape and dtype")
    if parent.dtype != torch.int32 or not parent.is_contiguous():
        raise TypeError("beam_gather: parent must be a contiguous int32 [B, W]")
    sp = (C.c_void_p * n)(*[x.data_ptr() for x in src])
    dp = (C.c_void_p * n)(*[x.data_ptr() for x in dst])
    Tmax = first.shape[1]
    A.call("case_beam_gather", C.cast(sp, C.c_void_p), C.cast(dp, C.c_void_p), n, _ptr(parent), _ptr(_u8(valid_src)), _ptr(_u8(valid_dst)), B, W, Tmax,
           first.shape[2] * first.element_size(), t, _stream())


def beam_backtrack(state):
    """K27: -> (answer int64 [B, T], beam_answers int64 [B, W, T] best first, beam_scores f32 [B, W] = cum_cost / length, +inf where empty)."""
    B, W, T = state.B, state.W, state.T
    dev = state.fin_key.device
    answer = torch.empty(B, T, dtype=torch.int64, device=dev)
    beam_answers = torch.empty(B, W, T, dtype=torch.int64, device=dev)
    beam_scores = torch.empty(B, W, dtype=torch.float32, device=dev)
    A.call("case_beam_backtrack", _ptr(state.hist_parent), _ptr(state.hist_token), _ptr(state.fin_key), _ptr(state.fin_step), _ptr(state.fin_slot),
           _ptr(answer), _ptr(beam_answers), _ptr(beam_scores), B, W, T, _stream())
    return answer, beam_answers, beam_scores


class SortedSource(object):
    """A source map [B, S] with its device-sorted (token, position) keys, made once per batch and shared by every
    pointer scatter of that batch (one per training step; one per generated token in greedy decoding)."""
    MAX_S, MAX_V = 32768, 131071

    def __init__(self, ids, V):
        self.ids = ids.contiguous()
        self.V = V
        B, S = self.ids.shape
        self.keys = torch.empty(B, S, dtype=torch.int32, device=ids.device)
        A.call("case_source_sort", _ptr(self.ids), _ptr(self.keys), B, S, V, _stream())

    def expand(self, width):
        """Every row ``width`` times in a row (the rows of one item's beam slots): the sorted keys are repeated, not sorted again."""
        out = object.__new__(SortedSource)
        out.ids, out.V, out.keys = self.ids.repeat_interleave(width, dim=0), self.V, self.keys.repeat_interleave(width, dim=0)
        return out

    def select(self, rows):
        """The rows named by ``rows`` (a slice, or an int64 index tensor with repeats allowed): ids and sorted keys, not sorted again."""
        out = object.__new__(SortedSource)
        if isinstance(rows, slice):
            out.ids, out.V, out.keys = self.ids[rows], self.V, self.keys[rows]
        else:
            out.ids, out.V, out.keys = self.ids.index_select(0, rows), self.V, self.keys.index_select(0, rows)
        return out

    @classmethod
    def fits(cls, ids, V):
        return ids.dtype == torch.int64 and ids.dim() == 2 and ids.size(1) <= cls.MAX_S and V <= cls.MAX_V


class CopyScatterFn(Function):
    @staticmethod
    def forward(ctx, src_ids, w, V, base, keys=None):
        """dist[b, t, src[b, s]] += w[b, t, s] on top of ``base`` (or zeros); with sorted ``keys`` run by run, without atomics."""
        B, T, S = w.shape
        w = w.float().contiguous()
        dist = torch.zeros(B, T, V, dtype=torch.float32, device=w.device) if base is None else base.float().clone()
        if keys is not None:
            A.call("case_copy_scatter_sorted_fwd", _ptr(keys), _ptr(w), _ptr(dist), B, T, S, V, _stream())
        else:
            A.call("case_copy_scatter_fwd", _ptr(src_ids), _ptr(w), _ptr(dist), B, T, S, V, _stream())
        ctx.save_for_backward(src_ids)
        ctx.meta = (B, T, S, V, base is not None)
        return dist

    @staticmethod
    def backward(ctx, g):
        (src_ids,) = ctx.saved_tensors
        B, T, S, V, has_base = ctx.meta
        g = g.float().contiguous()
        d_w = torch.empty(B, T, S, dtype=torch.float32, device=g.device)
        A.call("case_copy_scatter_bwd", _ptr(src_ids), _ptr(g), _ptr(d_w), B, T, S, V, _stream())
        return None, d_w, None, (g if has_base else None), None


def copy_scatter(src_ids, w, V, base=None):
    if isinstance(src_ids, SortedSource):
        if src_ids.V != V:
            raise ValueError("source map was sorted for a vocabulary of %d, scatter asks for %d" % (src_ids.V, V))
        return CopyScatterFn.apply(src_ids.ids, w, V, base, src_ids.keys)
    return CopyScatterFn.apply(src_ids.contiguous(), w, V, base)


class NllGatherFn(Function):
    @staticmethod
    def forward(ctx, dist, target):
        V = dist.shape[-1]
        dist = dist.float().contiguous()
        tgt = target.reshape(-1).contiguous()
        per_row = torch.empty(tgt.numel(), dtype=torch.float32, device=dist.device)
        A.call("case_nll_gather_fwd", _ptr(dist), _ptr(tgt), _ptr(per_row), tgt.numel(), V, _stream())
        ctx.save_for_backward(dist, tgt)
        return per_row

    @staticmethod
    def backward(ctx, g):
        dist, tgt = ctx.saved_tensors
        V = dist.shape[-1]
        g = g.float().contiguous()
        d = torch.zeros_like(dist)
        A.call("case_nll_gather_bwd", _ptr(dist), _ptr(tgt), _ptr(g), _ptr(d), tgt.numel(), V, _stream())
        return d, None


def nll_rows(dist, target):
    """Per-row -log(dist[target] + 1e-8), 0 where target == 0 (ignore_index)."""
    return NllGatherFn.apply(dist, target)


def row_argmax(x):
    """[rows, cols] f32 -> (int64 argmax with lowest-index tie break, max value)."""
    x = x.float()
    x = x if x.is_contiguous() else x.contiguous()
    rows, cols = x.shape
    idx = torch.empty(rows, dtype=torch.int64, device=x.device)
    val = torch.empty(rows, dtype=torch.float32, device=x.device)
    A.call("case_row_argmax", _ptr(x), _ptr(idx), _ptr(val), rows, cols, cols, _stream())
    return idx, val


def sentence_compact(ids, bos, pad, eos):
    """ids int64 [B, T] on the GPU -> (kept ids front-packed [B, T], count int32 [B]): BOS / PAD dropped, cut at the first EOS."""
    ids = ids.contiguous()
    B, T = ids.shape
    out = torch.empty_like(ids)
    n = torch.empty(B, dtype=torch.int32, device=ids.device)
    A.call("case_sentence_compact", _ptr(ids), _ptr(out), _ptr(n), B, T, bos, pad, eos, _stream())
    return out, n


# K30 / K31: ROUGE-L on token ids and the consensus pick over a pool of candidates
CONSENSUS_MAX_N, LCS_MAX_T = 64, ID_MAX_T


def _id_pairs(who, a, a_len, b, b_len, max_t):
    """The operands of K30, K34 and K40, checked: a int64 [B, N, Ta] with a_len int32 [B, N], b int64 [B, M, Tb] with b_len int32 [B, M], on
    one device, nothing empty, Ta <= max_t -> (a, a_len, b, b_len) contiguous and (B, N, M, Ta, Tb)."""
    is_tensor = torch.is_tensor  # (spelt out, no loops: this runs in front of kernels of some 20 us)
    if not (is_tensor(a) and is_tensor(b)) or a.dtype != torch.int64 or b.dtype != torch.int64 or a.dim() != 3 or b.dim() != 3 or \
            a.shape[0] != b.shape[0]:
        raise TypeError("%s: a and b must be int64 [B, N, Ta] and [B, M, Tb] of one batch" % who)
    (B, N, Ta), (M, Tb) = a.shape, b.shape[1:]
    if not (is_tensor(a_len) and is_tensor(b_len)) or a_len.dtype != torch.int32 or b_len.dtype != torch.int32 or a_len.shape != (B, N) or \
            b_len.shape != (B, M):
        raise TypeError("%s: the lengths must be int32 [B, N] and [B, M]" % who)
    if not a.device == a_len.device == b.device == b_len.device:
        raise ValueError("%s: a, a_len, b and b_len must be on one device (got %s, %s, %s, %s)" % (who, a.device, a_len.device, b.device, b_len.device))
    if B < 1 or N < 1 or M < 1 or Ta < 1 or Tb < 1:
        raise ValueError("%s: at least one item, hypothesis, reference and position (got a %s, b %s)" % (who, list(a.shape), list(b.shape)))
    if Ta > max_t:
        raise ValueError("%s: hypotheses of up to %d positions (got %d)" % (who, max_t, Ta))
    return (a.contiguous(), a_len.contiguous(), b.contiguous(), b_len.contiguous()), (B, N, M, Ta, Tb)


def consensus_supported(N, T):
    """A pool of N candidates of T positions: K31 holds a pool in one wave, K30 a hypothesis in 4 x 64 match-mask bits."""
    return 1 <= N <= CONSENSUS_MAX_N and 1 <= T <= LCS_MAX_T and bool(A.lib.case_abi_features() & A.FEAT_CONSENSUS)


def lcs_pairs(a, a_len, b, b_len):
    """K30: a int64 [B, N, Ta] / a_len int32 [B, N] (front-packed hypotheses and their lengths, as ``sentence_compact`` writes them), b int64
    [B, M, Tb] / b_len int32 [B, M] (references) -> (lcs int32 [B, N, M], f f32 [B, N, M]): the LCS length and the ROUGE-L F of every pair
    (evaluation.rouge's, in f64, rounded once).  Ta <= 256; ids must lie in [0, 2^31) (not checked: they are compared on 32 bits)."""
    (a, a_len, b, b_len), (B, N, M, Ta, Tb) = _id_pairs("lcs_pairs", a, a_len, b, b_len, LCS_MAX_T)
    lcs = torch.empty(B, N, M, dtype=torch.int32, device=a.device)
    f = torch.empty(B, N, M, dtype=torch.float32, device=a.device)
    A.call("case_lcs_pairs", _ptr(a), _ptr(a_len), _ptr(b), _ptr(b_len), _ptr(lcs), _ptr(f), B, N, M, Ta, Tb, _stream())
    return lcs, f


def consensus_pick(f, weights, valid, candidates):
    """K31: f f32 [B, N, N] (pairwise utility, candidate n as the hypothesis, m as the reference), weights f32 [B, N] or None (uniform),
    valid bool [B, N] or None (all), candidates int64 [B, N, T] -> (utility f32 [B, N] = the weighted mean of f[b, n, :] over the valid m,
    -inf for an invalid n; index int64 [B] = its argmax, the lowest index on ties, 0 without a valid candidate; answer int64 [B, T] =
    candidates[b, index[b]])."""
    if f.dtype != torch.float32 or f.dim() != 3 or f.shape[1] != f.shape[2]:
        raise TypeError("consensus_pick: f must be f32 [B, N, N]")
    B, N = f.shape[:2]
    if candidates.dtype != torch.int64 or candidates.dim() != 3 or tuple(candidates.shape[:2]) != (B, N):
        raise TypeError("consensus_pick: candidates must be int64 [B, N, T]")
    if N > CONSENSUS_MAX_N:
        raise ValueError("consensus_pick: pools of up to %d candidates (got %d)" % (CONSENSUS_MAX_N, N))
    if weights is not None and (weights.dtype != torch.float32 or tuple(weights.shape) != (B, N)):
        raise TypeError("consensus_pick: weights must be f32 [B, N]")
    if valid is not None and (valid.dtype not in (torch.bool, torch.uint8) or tuple(valid.shape) != (B, N)):
        raise TypeError("consensus_pick: valid must be bool [B, N]")
    T = candidates.shape[2]
    f, candidates = (t if t.is_contiguous() else t.contiguous() for t in (f, candidates))
    weights = None if weights is None else weights.contiguous()
    utility = torch.empty(B, N, dtype=torch.float32, device=f.device)
    index = torch.empty(B, dtype=torch.int64, device=f.device)
    answer = torch.empty(B, T, dtype=torch.int64, device=f.device)
    A.call("case_consensus_pick", _ptr(f), _ptr(weights), _ptr(_u8(valid)), _ptr(candidates), _ptr(utility), _ptr(index), _ptr(answer), B, N, T,
           _stream())
    return utility, index, answer


# K34 / K35: n-gram counts and BLEU on token ids
NGRAM_MAX_ORDER = 4  # (rows of up to NGRAM_MAX_T positions, as K32's histories)
BLEU_SMOOTHINGS = {"none": 0, "add1": 1}


def ngram_supported(Ta, max_n=4):
    """Hypotheses of Ta positions and orders 1 .. max_n: K34 holds a hypothesis in 4 x 64 match-mask bits and counts four orders."""
    return 1 <= Ta <= NGRAM_MAX_T and 1 <= max_n <= NGRAM_MAX_ORDER and bool(A.lib.case_abi_features() & A.FEAT_NGRAM_COUNTS)


def _max_n(what, max_n):
    if not isinstance(max_n, int) or isinstance(max_n, bool) or not 1 <= max_n <= NGRAM_MAX_ORDER:
        raise ValueError("%s: max_n in 1..%d (got %r)" % (what, NGRAM_MAX_ORDER, max_n))


def ngram_counts(a, a_len, b, b_len, max_n=4):
    """K34: a int64 [B, N, Ta] / a_len int32 [B, N] (front-packed hypotheses and their lengths, as ``sentence_compact`` writes them), b int64
    [B, M, Tb] / b_len int32 [B, M] (references; ``b_len`` 0: absent) -> dict of exact int32 counts, the order k = 1..4 on the last axis (0
    above ``max_n``): clip [B, N, M, 4] (clipped k-gram matches against reference m), clip_any [B, N, 4] (against the per-k-gram maximum over
    the present references: multi-reference BLEU's numerator), hit [B, N, M, 4] / hit_any [B, N, 4] (distinct hypothesis k-grams that occur
    in reference m / in any present one), distinct [B, N, 4].  Ta <= 256; ids must lie in [0, 2^31) (not checked: compared on 32 bits)."""
    (a, a_len, b, b_len), (B, N, M, Ta, Tb) = _id_pairs("ngram_counts", a, a_len, b, b_len, NGRAM_MAX_T)
    _max_n("ngram_counts", max_n)
    new = lambda *shape: torch.empty(*shape, NGRAM_MAX_ORDER, dtype=torch.int32, device=a.device)  # noqa: E731
    out = dict(clip=new(B, N, M), clip_any=new(B, N), hit=new(B, N, M), hit_any=new(B, N), distinct=new(B, N))
    A.call("case_ngram_counts", _ptr(a), _ptr(a_len), _ptr(b), _ptr(b_len), _ptr(out["clip"]), _ptr(out["clip_any"]), _ptr(out["hit"]),
           _ptr(out["hit_any"]), _ptr(out["distinct"]), B, N, M, Ta, Tb, max_n, _stream())
    return out


def bleu_scores(counts, a_len, b_len, max_n=4, smoothing="none"):
    """K35: ``counts`` (``ngram_counts``' dict: ``clip`` and ``clip_any`` are read) and the lengths it was given -> (bleu_pair f32 [B, N, M]:
    sentence BLEU of hypothesis n against the single reference m, f64 rounded once; bleu f64 [B, N]: against all present references;
    bp f64 [B, N]: the brevity penalty of ``bleu``).  evaluation.bleu.sentence_bleu's definition; ``smoothing`` "none" or "add1"."""
    if smoothing not in BLEU_SMOOTHINGS:
        raise ValueError("bleu_scores: smoothing must be 'none' or 'add1', not %r" % (smoothing,))
    _max_n("bleu_scores", max_n)
    if a_len.dtype != torch.int32 or b_len.dtype != torch.int32 or a_len.dim() != 2 or b_len.dim() != 2 or a_len.shape[0] != b_len.shape[0]:
        raise TypeError("bleu_scores: the lengths must be int32 [B, N] and [B, M]")
    B, N = a_len.shape
    M = b_len.shape[1]
    clip, clip_any = counts["clip"], counts["clip_any"]
    if clip.dtype != torch.int32 or clip_any.dtype != torch.int32 or tuple(clip.shape) != (B, N, M, NGRAM_MAX_ORDER) or \
            tuple(clip_any.shape) != (B, N, NGRAM_MAX_ORDER):
        raise TypeError("bleu_scores: counts['clip'] / ['clip_any'] must be int32 [B, N, M, 4] / [B, N, 4] for lengths [B, N] and [B, M]")
    clip, clip_any, a_len, b_len = (t if t.is_contiguous() else t.contiguous() for t in (clip, clip_any, a_len, b_len))
    pair = torch.empty(B, N, M, dtype=torch.float32, device=clip.device)
    bleu = torch.empty(B, N, dtype=torch.float64, device=clip.device)
    bp = torch.empty(B, N, dtype=torch.float64, device=clip.device)
    A.call("case_bleu_scores", _ptr(clip), _ptr(clip_any), _ptr(a_len), _ptr(b_len), _ptr(pair), _ptr(bleu), _ptr(bp), B, N, M, max_n,
           BLEU_SMOOTHINGS[smoothing], _stream())
    return pair, bleu, bp


# K43 / K44: the distinct k-grams of rows of any length and ROUGE-N from the counts
def rouge_n_supported():
    return bool(A.lib.case_abi_features() & A.FEAT_ROUGE_N)


def ngram_distinct(b, b_len, max_n=4):
    """K43: b int64 [..., Tb] / b_len int32 [...] (front-packed rows and their lengths, as ``sentence_compact`` writes them; a length is
    clamped to 0 .. Tb) -> distinct int32 [..., 4]: the number of distinct k-grams of every row for k = 1..4 on the last axis (0 above
    ``max_n`` and for a row shorter than k).  Exact; Tb has no limit, the cost of a row grows with the SQUARE of its length (about
    L^2 / 500 token steps).  Ids must lie in [0, 2^31) (not checked: compared on 32 bits)."""
    if not torch.is_tensor(b) or b.dtype != torch.int64 or b.dim() < 2:
        raise TypeError("ngram_distinct: b must be int64 [..., Tb]")
    if not torch.is_tensor(b_len) or b_len.dtype != torch.int32 or tuple(b_len.shape) != tuple(b.shape[:-1]):
        raise TypeError("ngram_distinct: b_len must be int32 %s for b %s" % (list(b.shape[:-1]), list(b.shape)))
    if b_len.device != b.device:
        raise ValueError("ngram_distinct: b is on %s, b_len on %s" % (b.device, b_len.device))
    _max_n("ngram_distinct", max_n)
    Tb = b.shape[-1]
    rows = b_len.numel()
    if rows < 1 or Tb < 1:
        raise ValueError("ngram_distinct: at least one row and one position (got b %s)" % (list(b.shape),))
    if not rouge_n_supported():
        raise RuntimeError("ngram_distinct: this build of the library lacks K43 / K44 (CASE_FEAT_ROUGE_N)")
    b, b_len = (t if t.is_contiguous() else t.contiguous() for t in (b, b_len))
    distinct = torch.empty(*b_len.shape, NGRAM_MAX_ORDER, dtype=torch.int32, device=b.device)
    A.call("case_ngram_distinct", _ptr(b), _ptr(b_len), _ptr(distinct), rows, Tb, max_n, _stream())
    return distinct


def rouge_n_scores(hit, hyp_distinct, ref_distinct, b_len, max_n=4):
    """K44: hit int32 [B, N, M, 4] and hyp_distinct int32 [B, N, 4] (``ngram_counts``' ``hit`` and ``distinct``), ref_distinct int32 [B, M, 4]
    (``ngram_distinct`` of the references), b_len int32 [B, M] (0: the reference is absent) -> dict(f_pair f32 [B, N, M, 4]: the reference's
    ``rouge_n`` F of hypothesis n against reference m for the orders 1..4, f64 rounded once, 0 for an absent reference; f, p, r f64
    [B, N, 4]: the values against the present reference with the largest F, the lowest index among equals; best_ref int32 [B, N, 4]: its
    index, -1 without a present reference, and then f = p = r = 0).  The orders above ``max_n`` read 0 and best_ref -1."""
    _max_n("rouge_n_scores", max_n)
    tensors = (("hit", hit, 4), ("hyp_distinct", hyp_distinct, 3), ("ref_distinct", ref_distinct, 3), ("b_len", b_len, 2))
    for name, t, dim in tensors:
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != dim:
            raise TypeError("rouge_n_scores: %s must be an int32 tensor of %d axes" % (name, dim))
    B, N, M = hit.shape[:3]
    if tuple(hit.shape) != (B, N, M, NGRAM_MAX_ORDER) or tuple(hyp_distinct.shape) != (B, N, NGRAM_MAX_ORDER) or \
            tuple(ref_distinct.shape) != (B, M, NGRAM_MAX_ORDER) or tuple(b_len.shape) != (B, M):
        raise TypeError("rouge_n_scores: hit [B, N, M, 4], hyp_distinct [B, N, 4], ref_distinct [B, M, 4] and b_len [B, M] (got %s, %s, %s, %s)"
                        % tuple(list(t.shape) for _, t, _ in tensors))
    if B < 1 or N < 1 or M < 1:
        raise ValueError("rouge_n_scores: at least one item, one hypothesis and one reference slot (got hit %s)" % (list(hit.shape),))
    if any(t.device != hit.device for _, t, _ in tensors):
        raise ValueError("rouge_n_scores: the four tensors must be on one device")
    if not rouge_n_supported():
        raise RuntimeError("rouge_n_scores: this build of the library lacks K43 / K44 (CASE_FEAT_ROUGE_N)")
    hit, hyp_distinct, ref_distinct, b_len = (t if t.is_contiguous() else t.contiguous() for t in (hit, hyp_distinct, ref_distinct, b_len))
    new = lambda dtype: torch.empty(B, N, NGRAM_MAX_ORDER, dtype=dtype, device=hit.device)  # noqa: E731
    out = dict(f_pair=torch.empty(B, N, M, NGRAM_MAX_ORDER, dtype=torch.float32, device=hit.device), f=new(torch.float64),
               p=new(torch.float64), r=new(torch.float64), best_ref=new(torch.int32))
    A.call("case_rouge_n_scores", _ptr(hit), _ptr(hyp_distinct), _ptr(ref_distinct), _ptr(b_len), _ptr(out["f_pair"]), _ptr(out["f"]),
           _ptr(out["p"]), _ptr(out["r"]), _ptr(out["best_ref"]), B, N, M, max_n, _stream())
    return out


# K40: METEOR on token ids
METEOR_MAX_T = ID_MAX_T


def meteor_supported(Ta):
    """Hypotheses of Ta positions: K40 holds a hypothesis in 4 x 64 match-mask bits."""
    return 1 <= Ta <= METEOR_MAX_T and bool(A.lib.case_abi_features() & A.FEAT_METEOR)


def meteor(a, a_len, b, b_len, classes=None, alpha=0.9, beta=3.0, gamma=0.5, want_align=False):
    """K40: a int64 [B, N, Ta] / a_len int32 [B, N] (front-packed hypotheses and their lengths, as ``sentence_compact`` writes them), b int64
    [B, M, Tb] / b_len int32 [B, M] (references; ``b_len`` 0: absent) -> dict(counts int32 [B, N, M, 3] = (matches, exact matches, chunks) of
    evaluation.meteor's alignment, meteor_pair f32 [B, N, M] = the score of every pair (f64 rounded once), meteor f64 [B, N] = the maximum over
    the present references, best_ref int32 [B, N] = the lowest index that reaches it (-1 without a present reference) and, with
    ``want_align``, align int32 [B, N, M, Ta] = the matched reference position of every hypothesis position or -1).  ``classes``: an int32 [V]
    table id -> equivalence class on the ids' device (a negative entry and an id >= V: no class) for the second stage; None: exact matches
    only.  Ta <= 256; ids must lie in [0, 2^31) (not checked: compared on 32 bits)."""
    (a, a_len, b, b_len), (B, N, M, Ta, Tb) = _id_pairs("meteor", a, a_len, b, b_len, METEOR_MAX_T)
    try:
        alpha, beta, gamma = float(alpha), float(beta), float(gamma)
    except (TypeError, ValueError):
        raise ValueError("meteor: alpha, beta and gamma must be numbers (got %r, %r, %r)" % (alpha, beta, gamma))
    if not (0.0 <= alpha <= 1.0 and 0.0 <= gamma <= 1.0 and 0.0 <= beta < math.inf):
        raise ValueError("meteor: alpha and gamma in [0, 1], beta >= 0 and finite (got %r, %r, %r)" % (alpha, beta, gamma))
    if classes is not None and (not torch.is_tensor(classes) or classes.dtype != torch.int32 or classes.dim() != 1 or classes.numel() == 0
                                or classes.device != a.device):
        raise ValueError("meteor: classes must be a 1-D int32 tensor [V] on the ids' device")
    classes = None if classes is None else classes.contiguous()
    out = dict(counts=torch.empty(B, N, M, 3, dtype=torch.int32, device=a.device),
               meteor_pair=torch.empty(B, N, M, dtype=torch.float32, device=a.device),
               meteor=torch.empty(B, N, dtype=torch.float64, device=a.device), best_ref=torch.empty(B, N, dtype=torch.int32, device=a.device))
    if want_align:
        out["align"] = torch.empty(B, N, M, Ta, dtype=torch.int32, device=a.device)
    A.call("case_meteor", _ptr(a), _ptr(a_len), _ptr(b), _ptr(b_len), _ptr(classes), 0 if classes is None else classes.numel(), alpha, beta,
           gamma, _ptr(out["counts"]), _ptr(out["meteor_pair"]), _ptr(out["meteor"]), _ptr(out["best_ref"]), _ptr(out.get("align")), B, N, M,
           Ta, Tb, _stream())
    return out


# K36: TREC ranking metrics of score rows
RANK_MAX_P, RANK_MAX_JUDGED = 1024, 2048
RANK_CUTOFFS = (5, 10, 15, 20, 30, 100, 200, 500, 1000)
RANK_METRICS = ("map", "ndcg") + tuple("recall_%d" % k for k in RANK_CUTOFFS) + ("recip_rank", "P_1")  # the columns of ``metrics``


def rank_metrics(scores, rel, keys=None, valid=None, extra_rel=None):
    """K36: scores f32 [B, P] (one query per row), rel int32 [B, P] (grades; relevant from 1 on, negative = 0), keys int32 [B, P] or None
    (the column index; the LARGER key comes first among equal scores), valid bool [B, P] or None (all; an invalid slot is not retrieved and
    its ``rel`` is ignored), extra_rel int32 [B, R] or None (grades of judged documents that were not retrieved; <= 0 = padding) ->
    dict(order int32 [B, P]: the columns in rank order, -1 behind the retrieved ones; metrics f64 [B, 13] in the order of ``RANK_METRICS``;
    num_rel int32 [B]).  evaluation.trec's definitions.  P <= 1024, P + R <= 2048."""
    if scores.dtype != torch.float32 or scores.dim() != 2:
        raise TypeError("rank_metrics: scores must be f32 [B, P]")
    B, P = scores.shape
    if rel.dtype != torch.int32 or tuple(rel.shape) != (B, P):
        raise TypeError("rank_metrics: rel must be int32 [B, P]")
    if keys is not None and (keys.dtype != torch.int32 or tuple(keys.shape) != (B, P)):
        raise TypeError("rank_metrics: keys must be int32 [B, P]")
    if valid is not None and (valid.dtype not in (torch.bool, torch.uint8) or tuple(valid.shape) != (B, P)):
        raise TypeError("rank_metrics: valid must be bool [B, P]")
    if extra_rel is not None and (extra_rel.dtype != torch.int32 or extra_rel.dim() != 2 or extra_rel.shape[0] != B):
        raise TypeError("rank_metrics: extra_rel must be int32 [B, R]")
    R = 0 if extra_rel is None else extra_rel.shape[1]
    if B < 1 or P < 1:
        raise ValueError("rank_metrics: at least one query and one document slot (got [%d, %d])" % (B, P))
    if P > RANK_MAX_P or P + R > RANK_MAX_JUDGED:
        raise ValueError("rank_metrics: up to %d retrieved and %d judged documents per query (got %d and %d)" % (
            RANK_MAX_P, RANK_MAX_JUDGED, P, P + R))
    scores, rel = (t if t.is_contiguous() else t.contiguous() for t in (scores, rel))
    keys = None if keys is None else keys.contiguous()
    extra_rel = None if R == 0 else extra_rel.contiguous()
    order = torch.empty(B, P, dtype=torch.int32, device=scores.device)
    metrics = torch.empty(B, len(RANK_METRICS), dtype=torch.float64, device=scores.device)
    num_rel = torch.empty(B, dtype=torch.int32, device=scores.device)
    A.call("case_rank_metrics", _ptr(scores), _ptr(keys), _ptr(rel), _ptr(_u8(valid)), _ptr(extra_rel), _ptr(order), _ptr(metrics),
           _ptr(num_rel), B, P, R, _stream())
    return dict(order=order, metrics=metrics, num_rel=num_rel)


# K37 / K38: the supporting-token stage's supervision and its best tokens
TOKEN_MAX_L, TOKEN_MAX_T, TOKEN_MAX_K = 16384, 1024, 256
TOKEN_COUNTS = ("n_valid", "n_pos", "n_pred", "tp", "hits")  # the columns of ``counts``


def token_labels_supported():
    return bool(A.lib.case_abi_features() & A.FEAT_TOKEN_LABELS)


def token_labels(passage, response, freq, pad=0):
    """K37: passage int64 [B, P, L], response int64 [B, T] (``pad`` where there is no token), freq f32 or int64 [F] (the count of id v at
    freq[v]; 0 for v >= F) -> (label, weight) f32 [B, P, L]: ``common.Utils.token_label``'s rule (the reference's CaSEDataset.py
    token_label), f64 inside and rounded once.  L <= 16384, T <= 1024, ids in [0, 2^31) (not checked: compared on 32 bits)."""
    if passage.dtype != torch.int64 or passage.dim() != 3:
        raise TypeError("token_labels: passage must be int64 [B, P, L]")
    B, P, L = passage.shape
    if response.dtype != torch.int64 or response.dim() != 2 or response.shape[0] != B:
        raise TypeError("token_labels: response must be int64 [B, T] for passage [%d, %d, %d]" % (B, P, L))
    if freq.dtype not in (torch.float32, torch.int64) or freq.dim() != 1:
        raise TypeError("token_labels: freq must be f32 or int64 [F]")
    T = response.shape[1]
    if B < 1 or P < 1 or L < 1 or T < 1:
        raise ValueError("token_labels: at least one item, passage, token and answer slot (got passage %s, response %s)" % (
            tuple(passage.shape), tuple(response.shape)))
    if L > TOKEN_MAX_L or T > TOKEN_MAX_T:
        raise ValueError("token_labels: rows of up to %d tokens and answers of up to %d ids (got %d and %d)" % (TOKEN_MAX_L, TOKEN_MAX_T, L, T))
    if not token_labels_supported():
        raise RuntimeError("token_labels: this build of the library lacks K37 / K38 (CASE_FEAT_TOKEN_LABELS)")
    passage, response, freq = (t if t.is_contiguous() else t.contiguous() for t in (passage, response, freq))
    label = torch.empty(B, P, L, dtype=torch.float32, device=passage.device)
    weight = torch.empty(B, P, L, dtype=torch.float32, device=passage.device)
    A.call("case_token_labels", _ptr(passage), _ptr(response), _ptr(freq) if freq.numel() else None, int(freq.dtype == torch.int64),
           _ptr(label), _ptr(weight), B, P, L, T, freq.numel(), int(pad), _stream())
    return label, weight


def token_select(values, valid, k, scores=None, labels=None):
    """K38: values f32 [B, S] (one item per row), valid bool [B, S] -> dict(pos int32 [B, k]: the positions of the k best valid keys, best
    first -- value descending, NaN as -inf, -0.0 == +0.0, then the LOWER position --, -1 behind the valid ones; value f32 [B, k]: ``values``
    there, 0 where pos is -1).  With ``labels`` f32 [B, S] also counts int32 [B, 5] in ``TOKEN_COUNTS``' order: n_valid, n_pos (valid and
    label > 0.5), n_pred (valid and score > 0; ``scores`` f32 [B, S], default ``values``), tp (both), hits (label > 0.5 among the selected).
    S <= 16384, k <= 256."""
    if values.dtype != torch.float32 or values.dim() != 2:
        raise TypeError("token_select: values must be f32 [B, S]")
    B, S = values.shape
    if valid.dtype not in (torch.bool, torch.uint8) or tuple(valid.shape) != (B, S):
        raise TypeError("token_select: valid must be bool [B, S]")
    for name, t in (("scores", scores), ("labels", labels)):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (B, S)):
            raise TypeError("token_select: %s must be f32 [B, S]" % name)
    if scores is not None and labels is None:
        raise TypeError("token_select: scores are read for the counts only, which need labels")
    k = int(k)
    if B < 1 or S < 1 or k < 1:
        raise ValueError("token_select: at least one item, one position and k = 1 (got [%d, %d], k %d)" % (B, S, k))
    if S > TOKEN_MAX_L or k > TOKEN_MAX_K:
        raise ValueError("token_select: rows of up to %d keys and up to %d selected positions (got %d and %d)" % (TOKEN_MAX_L, TOKEN_MAX_K, S, k))
    if not token_labels_supported():
        raise RuntimeError("token_select: this build of the library lacks K37 / K38 (CASE_FEAT_TOKEN_LABELS)")
    values = values if values.is_contiguous() else values.contiguous()
    scores, labels = (None if t is None else t.contiguous() for t in (scores, labels))
    pos = torch.empty(B, k, dtype=torch.int32, device=values.device)
    val = torch.empty(B, k, dtype=torch.float32, device=values.device)
    counts = None if labels is None else torch.empty(B, len(TOKEN_COUNTS), dtype=torch.int32, device=values.device)
    A.call("case_token_select", _ptr(values), _ptr(_u8(valid)), _ptr(scores), _ptr(labels), _ptr(pos), _ptr(val), _ptr(counts), B, S, k, _stream())
    out = dict(pos=pos, value=val)
    if counts is not None:
        out["counts"] = counts
    return out


# K45: the threshold-free ranking figures of a row of token scores (evaluation/token_rank.py states the definitions)
TOKEN_RANK_COUNTS = ("n_valid", "n_pos", "auc_num2", "best_tp", "best_n", "n_groups")  # the columns of ``counts``
TOKEN_RANK_STATS = ("ap", "auc")  # the columns of ``stats``


def token_rank_supported():
    return A.has("case_token_rank")


def token_rank(scores, valid, labels):
    """K45: scores f32 [B, S] (one item per row), valid bool [B, S] or None (all), labels float [B, S] (positive where > 0.5) ->
    dict(stats f64 [B, 2] = ap, auc; counts int32 [B, 6] in ``TOKEN_RANK_COUNTS``' order; threshold f32 [B] = the score of the best-F1 group,
    +inf where the item has no positive).  Scores compare as K38's key (NaN as -inf, -0.0 == +0.0); every figure is a function of the
    groups of equal key, so none depends on the position of a token.  S <= 16384; ValueError for a longer row, a shape or dtype mismatch or
    tensors off the device.  No autograd, nothing is read back."""
    if not torch.is_tensor(scores) or scores.dtype != torch.float32 or scores.dim() != 2:
        raise ValueError("token_rank: scores must be an f32 [B, S] tensor")
    B, S = scores.shape
    if valid is not None and (not torch.is_tensor(valid) or valid.dtype not in (torch.bool, torch.uint8) or tuple(valid.shape) != (B, S)):
        raise ValueError("token_rank: valid must be bool [%d, %d] or None" % (B, S))
    if not torch.is_tensor(labels) or not labels.is_floating_point() or tuple(labels.shape) != (B, S):
        raise ValueError("token_rank: labels must be float [%d, %d]" % (B, S))
    if S < 1 or S > TOKEN_MAX_L:
        raise ValueError("token_rank: rows of 1 .. %d positions (got %d)" % (TOKEN_MAX_L, S))
    if not token_rank_supported():
        raise RuntimeError("token_rank: this build of the library lacks K45 (case_token_rank) -- rebuild it (make -C case_rg_amd/csrc)")
    for name, t in (("scores", scores), ("valid", valid), ("labels", labels)):
        if t is not None and (t.device.type != "cuda" or t.device != scores.device):
            raise ValueError("token_rank: %s must live on the device (%s; scores on %s)" % (name, t.device, scores.device))
    scores = scores if scores.is_contiguous() else scores.contiguous()
    labels = labels.float().contiguous()
    valid = None if valid is None else valid.contiguous()
    stats = torch.empty(B, len(TOKEN_RANK_STATS), dtype=torch.float64, device=scores.device)
    counts = torch.empty(B, len(TOKEN_RANK_COUNTS), dtype=torch.int32, device=scores.device)
    threshold = torch.empty(B, dtype=torch.float32, device=scores.device)
    if B:
        A.call("case_token_rank", _ptr(scores), _ptr(_u8(valid)), _ptr(labels), _ptr(stats), _ptr(counts), _ptr(threshold), B, S, _stream())
    return dict(stats=stats, counts=counts, threshold=threshold)


# K39: where the pointer mass of a target token comes from (the per-segment split, the best source position, the run length).  "auto": a
# device-sorted source map and <= 4 memories; "off": the host form (evaluation.attribution.copy_attribution_host) wherever a pass attributes.
COPY_ATTRIBUTION = os.environ.get("CASE_COPY_ATTRIBUTION", "auto")
ATTRIBUTION_MAX_G = 64


def copy_attribution_supported(source_map, nmem):
    return (COPY_ATTRIBUTION != "off" and isinstance(source_map, SortedSource) and 1 <= nmem <= 4
            and bool(A.lib.case_abi_features() & A.FEAT_COPY_ATTRIBUTION))


def check_segments(seg_start, S, who="copy_attribution", limit=ATTRIBUTION_MAX_G):
    """A Python sequence of segment boundaries, checked in full: 1 .. ``limit`` segments (None: any number), strictly ascending from 0 to S
    -> list of int."""
    seg = [int(v) for v in seg_start]
    G = len(seg) - 1
    if G < 1 or (limit is not None and G > limit):
        raise ValueError("%s: 1 .. %s segments (seg_start holds %d boundaries)" % (who, limit, len(seg)))
    if seg[0] != 0 or seg[-1] != S or any(a >= b for a, b in zip(seg, seg[1:])):
        raise ValueError("%s: seg_start must ascend strictly from 0 to S = %d (got %r)" % (who, S, seg))
    return seg


def copy_attribution(mix_logits, source_map, rows_per_source, copies, targets, seg_start, pad=0):
    """K39: mix_logits f32 [R, 1 + nmem]; source_map a SortedSource with R / rows_per_source rows (row r reads key row r // rows_per_source);
    copies: list of f32 [R, len_k]; targets int64 [R]; seg_start: the G + 1 boundaries that cut the S source positions into G <= 64 segments,
    a Python sequence (checked in full: strictly ascending from 0 to S) or an int32 device tensor [G + 1] (shape and dtype only: it is not
    read back) -> dict(mass f32 [R, G]: the pointer mass of the row's target from the positions of each segment; pos int32 [R]: the source
    position with the largest single term, the lower one among equals; pos_mass f32 [R]: that term; count int32 [R]: the positions of the
    item's source that hold the target).  ``targets == pad`` (pad -1: none), an id outside [0, V) or absent from the source: 0, -1, 0, 0.
    No autograd (inference)."""
    if mix_logits.dim() != 2 or tuple(mix_logits.shape) != (mix_logits.shape[0], len(copies) + 1):
        raise ValueError("copy_attribution: mix_logits must be [R, 1 + nmem]")
    if not isinstance(source_map, SortedSource):
        raise TypeError("copy_attribution: source_map must be a SortedSource (the host form takes plain ids)")
    R = mix_logits.shape[0]
    rows_per_source = int(rows_per_source)
    keys = source_map.keys
    if rows_per_source < 1 or R % rows_per_source or keys.shape[0] * rows_per_source != R:
        raise ValueError("copy_attribution: %d rows, %d key rows, rows_per_source %d" % (R, keys.shape[0], rows_per_source))
    if targets.dtype != torch.int64 or targets.numel() != R:
        raise TypeError("copy_attribution: targets must be int64 [R]")
    if not 1 <= len(copies) <= 4:
        raise ValueError("copy_attribution: 1 .. 4 memories (got %d)" % len(copies))
    if any(c.dim() != 2 or c.shape[0] != R for c in copies):
        raise ValueError("copy_attribution: every copies[k] must be [R, len_k]")
    S = keys.shape[1]
    if sum(c.shape[1] for c in copies) != S:
        raise ValueError("copy_attribution: the memories hold %d positions, the source map %d" % (sum(c.shape[1] for c in copies), S))
    dev = mix_logits.device
    if torch.is_tensor(seg_start):
        if seg_start.dtype != torch.int32 or seg_start.dim() != 1 or seg_start.device != dev:
            raise TypeError("copy_attribution: a seg_start tensor must be int32 [G + 1] on the rows' device")
        G = seg_start.numel() - 1
        if not 1 <= G <= ATTRIBUTION_MAX_G:
            raise ValueError("copy_attribution: 1 .. %d segments (seg_start holds %d boundaries)" % (ATTRIBUTION_MAX_G, G + 1))
        seg_dev, seg_host = seg_start.contiguous(), None
    else:
        seg = check_segments(seg_start, S)
        G = len(seg) - 1
        seg_dev, seg_host = None, (C.c_int32 * (G + 1))(*seg)
    if not bool(A.lib.case_abi_features() & A.FEAT_COPY_ATTRIBUTION):
        raise RuntimeError("copy_attribution: this build of the library lacks K39 (CASE_FEAT_COPY_ATTRIBUTION)")
    mix_logits = mix_logits.float().contiguous()
    cs = [c.float().contiguous() for c in copies]  # (alive until the call)
    n = len(cs)
    ptrs = C.cast((C.c_void_p * n)(*[c.data_ptr() for c in cs]), C.c_void_p)
    lens = C.cast((C.c_int64 * n)(*[c.shape[1] for c in cs]), C.c_void_p)
    targets = targets.reshape(R).contiguous()
    mass = torch.empty(R, G, dtype=torch.float32, device=dev)
    pos = torch.empty(R, dtype=torch.int32, device=dev)
    pos_mass = torch.empty(R, dtype=torch.float32, device=dev)
    count = torch.empty(R, dtype=torch.int32, device=dev)
    A.call("case_copy_attribution", _ptr(mix_logits), _ptr(keys), rows_per_source, ptrs, lens, n, _ptr(targets), int(pad), _ptr(seg_dev),
           None if seg_host is None else C.cast(seg_host, C.c_void_p), G, _ptr(mass), _ptr(pos), _ptr(pos_mass), _ptr(count), R, source_map.V, S,
           _stream())
    return dict(mass=mass, pos=pos, pos_mass=pos_mass, count=count)
