"""CPU-side checks of the loss-only training head: the two entry points in the header, the ctypes table and the library; their argument
validation before any launch; the row-padded operand copy's host logic on CPU tensors; and the fall-back to the dense chain where the head
is not supported (switches, an unsorted source map, more than 4 memories, a library without the symbols).  No compute is launched."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "case_hip.h")
NAMES = ("case_pointer_head_loss", "case_pointer_head_loss_bwd")


def test_header_table_and_library_carry_the_two_exports():
    from case_rg_amd import _abi
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for name, nargs in zip(NAMES, (18, 21)):
        proto = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, text, flags=re.S)
        assert proto, "%s is not declared in include/case_hip.h" % name
        assert len([a for a in proto.group(1).split(",") if a.strip()]) == nargs == len(_abi.SIGNATURES[name])
        assert hasattr(lib, name) and _abi.has(name), "libcase_hip.so does not export %s" % name
        assert name in _abi.OPTIONAL, "found by symbol lookup: the 32-bit feature mask is full"
    assert not _abi.has("case_no_such_entry_point")
    assert _abi.FEAT_ROUGE_N == 1 << 31 and _abi.FEAT_RISK_TRAIN == 1 << 30, "no existing feature bit moved"
    assert _abi.lib.case_version() == _abi.ABI_VERSION == 600, "purely additive: the generation stays"
    assert len(_abi.SIGNATURES["case_pointer_head_score_stats"]) == 16 and len(_abi.SIGNATURES["case_pointer_head_score_bwd"]) == 19


def test_exports_validate_before_any_launch():
    """Every refusal is matched by the part of its message that names the violated condition, with operands on a 16-byte boundary so that
    no case is turned away by the alignment check in front of the condition it is there for."""
    from case_rg_amd import _abi
    raw = (ctypes.c_char * 160)()  # never dereferenced: every call below is refused before a launch
    base = (ctypes.addressof(raw) + 15) // 16 * 16
    p, off8 = ctypes.c_void_p(base), ctypes.c_void_p(base + 8)
    lens = ctypes.cast((ctypes.c_int64 * 5)(4, 4, 4, 4, 4), ctypes.c_void_p)
    ptrs = ctypes.cast((ctypes.c_void_p * 5)(*[base] * 5), ctypes.c_void_p)

    def fwd(ld, nmem, R, V, S, rps, logits=p, stats=p, nll=p):
        _abi.call("case_pointer_head_loss", logits, ld, p, p, rps, ptrs, lens, nmem, p, 0, p, p, stats, nll, R, V, S, None)

    def bwd(ld, dt, nmem, R, V, S, rps, logits=p, d_logits=p):
        _abi.call("case_pointer_head_loss_bwd", logits, ld, p, p, rps, ptrs, lens, nmem, p, 0, p, p, p, d_logits, dt, p, ptrs, R, V, S, None)

    with pytest.raises(RuntimeError, match="case_pointer_head_loss: bad argument"):
        _abi.call("case_pointer_head_loss", None, 8, None, None, 1, None, None, 1, None, 0, None, None, None, None, 1, 8, 4, None)
    with pytest.raises(RuntimeError, match="case_pointer_head_loss_bwd: bad argument"):
        _abi.call("case_pointer_head_loss_bwd", None, 8, None, None, 1, None, None, 1, None, 0, None, None, None, None, 0, None, None, 1, 8, 4, None)
    for kw in (dict(stats=None), dict(nll=None)):  # both are required
        with pytest.raises(RuntimeError, match="case_pointer_head_loss: bad argument"):
            fwd(8, 1, 1, 8, 4, 1, **kw)
    for args, kw, why in (((4, 1, 1, 8, 4, 1), {}, r"ld_logits >= V floats apart.*got ld 4, V 8"),          # ld below V
                          ((10, 1, 1, 8, 4, 1), {}, r"a multiple of 4.*got ld 10, V 8"),                    # ld no multiple of 4
                          ((8, 1, 1, 8, 4, 1), dict(logits=off8), r"on a 16-byte base"),                    # a base 8 bytes off
                          ((8, 5, 1, 8, 20, 1), {}, r"built for <= 4 memories"),
                          ((131328, 1, 1, 131072, 4, 1), {}, r"V <= 131071"),
                          ((8, 1, 1, 8, 32769, 1), {}, r"S <= 32768"),
                          ((8, 1, 3, 8, 4, 2), {}, r"3 rows are no multiple of rows_per_source 2"),
                          ((8, 1, 1, 8, 5, 1), {}, r"the memories hold 4 positions, the source map 5"),
                          ((8, 1, 0, 8, 4, 1), {}, r"case_pointer_head_loss: bad argument")):                # no rows
        with pytest.raises(RuntimeError, match=why):
            fwd(*args, **kw)
    for args, kw, why in (((4, 0, 1, 1, 8, 4, 1), {}, r"ld_logits >= V elements apart.*got ld 4, V 8"),
                          ((12, 1, 1, 1, 8, 4, 1), {}, r"a multiple of 8.*got ld 12, V 8"),
                          ((8, 1, 1, 1, 8, 4, 1), dict(logits=off8), r"on 16-byte bases"),
                          ((8, 1, 1, 1, 8, 4, 1), dict(d_logits=off8), r"on 16-byte bases"),
                          ((8, 2, 1, 1, 8, 4, 1), {}, r"d_logits is f32 or bf16 \(got dtype 2\)"),
                          ((8, 1, 5, 1, 8, 20, 1), {}, r"built for <= 4 memories"),
                          ((131328, 1, 1, 1, 131072, 4, 1), {}, r"V <= 131071"),
                          ((8, 0, 1, 1, 8, 32769, 1), {}, r"S <= 32768"),
                          ((8, 1, 1, 3, 8, 4, 2), {}, r"3 rows are no multiple of rows_per_source 2"),
                          ((8, 0, 1, 1, 8, 5, 1), {}, r"the memories hold 4 positions, the source map 5"),
                          ((8, 0, 1, 0, 8, 4, 1), {}, r"case_pointer_head_loss_bwd: bad argument")):
        with pytest.raises(RuntimeError, match=why):
            bwd(*args, **kw)


def test_row_padded_copy_on_cpu_tensors():
    """The accessor's host logic, with f32 as the operand dtype so that nothing is launched: geometry, the zero pad, the cache, both kinds
    of rewrite, and the short cut through a live cast copy that already sits inside a padded buffer (FusedAdam's)."""
    from case_rg_amd import ops, paramcache
    assert [ops.rowpad_rows(v, 256) for v in (1, 256, 257, 30522)] == [256, 256, 512, 30720]
    p = torch.nn.Parameter(torch.arange(40, dtype=torch.float32).reshape(10, 4) + 1)
    assert ops.rowpad_wanted(p) == 0
    low = ops.new_rowpad_copy(p, torch.bfloat16, 8)
    buf = low._case_rowpad_buf
    assert low.shape == p.shape and low.is_contiguous() and buf.shape == (16, 4) and low.data_ptr() == buf.data_ptr() and not buf.any()
    wp = ops.cast_param_rowpad(p, torch.float32, 8)
    assert ops.rowpad_wanted(p) == 8
    assert wp.shape == (16, 4) and torch.equal(wp[:10], p.detach()) and not wp[10:].any() and wp.data_ptr() != p.data_ptr()
    assert ops.cast_param_rowpad(p, torch.float32, 8) is wp, "served from the registry while the parameter stands still"
    with torch.no_grad():
        p.add_(1.0)  # an in-place update moves _version
    wp2 = ops.cast_param_rowpad(p, torch.float32, 8)
    assert wp2 is not wp and torch.equal(wp2[:10], p.detach()) and not wp2[10:].any()
    p.data.mul_(2.0)  # a write behind autograd's back: the writer reports it
    ops.invalidate_param_cache()
    wp3 = ops.cast_param_rowpad(p, torch.float32, 8)
    assert wp3 is not wp2 and torch.equal(wp3[:10], p.detach()) and not wp3[10:].any()
    # a live cast copy inside a padded buffer is the answer itself
    low.copy_(p.detach())
    paramcache.install((p,), paramcache.cast_tag(p, torch.bfloat16), low)
    assert ops.cast_param_rowpad(p, torch.bfloat16, 8) is buf and torch.equal(buf[:10], p.detach().to(torch.bfloat16)) and not buf[10:].any()
    with pytest.raises(TypeError, match="2-D"):
        ops.cast_param_rowpad(torch.zeros(10, 4), torch.float32, 8)
    with pytest.raises(TypeError, match="2-D"):
        ops.cast_param_rowpad(torch.nn.Parameter(torch.zeros(10)), torch.float32, 8)
    ops.invalidate_param_cache()


def test_split_k_leaves_the_padded_vocabulary_gradient_whole():
    from case_rg_amd import ops
    assert ops._split_for(30720, 512, 1280, 2) == 1, "240 tiles of 256 x 256 are one round of the persistent grid: no split, no atomics"
    assert ops._split_for(1280, 512, 30720, 2) >= ops.DW_SLAB_MIN_SPLIT, "the padded dX reduction goes to the slab path"
    assert ops._split_for(30522, 512, 1280, 2) <= 2 and ops._split_for(512, 512, 1280, 2) == 4, "the unpadded shapes keep their choice"


def _sorted_source_stub():
    from case_rg_amd import ops
    return object.__new__(ops.SortedSource)  # (its constructor sorts on the device)


def test_gating(monkeypatch):
    from case_rg_amd import _abi, ops
    sm = _sorted_source_stub()
    assert ops.train_head_supported(sm, 2) and ops.train_head_supported(sm, 4)
    assert not ops.train_head_supported(sm, 5), "more than 4 memories"
    assert not ops.train_head_supported(torch.zeros(2, 4, dtype=torch.int64), 2), "an unsorted source map"
    monkeypatch.setattr(ops, "TRAIN_HEAD", "dense")
    assert not ops.train_head_supported(sm, 2)
    monkeypatch.setattr(ops, "TRAIN_HEAD", "auto")
    monkeypatch.setattr(ops, "POINTER_SCORE", "off")
    assert not ops.train_head_supported(sm, 2), "CASE_POINTER_SCORE=off restores the dense chain too"
    monkeypatch.setattr(ops, "POINTER_SCORE", "auto")
    for missing in NAMES:
        monkeypatch.setattr(_abi, "has", lambda name, missing=missing: name != missing)
        assert not ops.train_head_supported(sm, 2), "a build without %s" % missing
        with pytest.raises(RuntimeError, match="lacks"):
            ops.train_head_nll(torch.zeros(2, 4), torch.nn.Parameter(torch.zeros(8, 4)), torch.zeros(2, 2), sm, 1, [torch.zeros(2, 3)],
                               torch.zeros(2, dtype=torch.int64))


def test_decoder_falls_back_to_the_dense_chain_without_the_symbols(monkeypatch):
    """``_train_nll`` of a decoder on a library that lacks the loss-form kernels runs ``_head`` and the gather (stubbed here: nothing is
    launched) and never reaches ``ops.train_head_nll``."""
    from case_rg_amd import _abi, ops
    from case_rg_amd.CaSE.Model import CaSETransformerSeqDecoder
    dec = CaSETransformerSeqDecoder(2, 1, 4, 120, 16).train()
    d1, d2 = torch.full((2, 3, 120), 0.25), torch.full((2, 3, 120), 0.5)
    seen = {}

    def head(*args):
        seen["head"] = True
        return None, None, (d1, d2)

    def nll_rows(dist, target):
        seen["dist"], seen["target"] = dist, target
        return torch.ones(6)

    def fused(*args, **kw):
        raise AssertionError("the fused head ran")

    monkeypatch.setattr(dec, "_head", head)
    monkeypatch.setattr(ops, "add", lambda a, b: a + b)
    monkeypatch.setattr(ops, "nll_rows", nll_rows)
    monkeypatch.setattr(ops, "train_head_nll", fused)
    monkeypatch.setattr(_abi, "has", lambda name: name not in NAMES)
    target = torch.tensor([[5, 6, 0], [7, 0, 0]])
    rows = dec._train_nll(None, None, [None, None], [None, None], None, _sorted_source_stub(), target)
    assert seen["head"] and rows.shape == (6,) and seen["dist"].shape == (6, 120) and bool((seen["dist"] == 0.75).all())
    assert torch.equal(seen["target"], target.reshape(-1))
    from case_rg_amd.common.heads import nll_mean
    assert float(nll_mean(rows, target)) == 2.0, "six rows of 1 over three non-pad targets"
