"""The wide (global-row) forms of K23 / K24 / K28, the part that needs no GPU: the feature bit, what the wrappers admit and the
``row="auto"`` policy at the LDS bound of 36 000 ids."""
import pytest


def test_feature_bit_is_reported():
    from case_rg_amd import _abi
    assert _abi.FEAT_POINTER_HEAD_WIDE == 1 << 25
    assert _abi.lib.case_abi_features() & _abi.FEAT_POINTER_HEAD_WIDE
    for name in ("case_pointer_head_decode_wide", "case_pointer_head_beam_wide", "case_pointer_head_sample_wide"):
        assert name in _abi.SIGNATURES and hasattr(_abi.lib, name)


def test_sampling_is_supported_beyond_the_lds_row():
    from case_rg_amd import ops
    assert ops.sample_supported(36000) and ops.sample_supported(36001) and ops.sample_supported(50265) and ops.sample_supported(119547)
    assert ops.sample_supported(1 << 24) and not ops.sample_supported((1 << 24) + 1), "the bound of the 64-bit histogram sums"


def test_auto_picks_lds_at_36000_and_global_at_36001():
    from case_rg_amd import ops
    assert ops.head_row_form(36000) == "lds" and ops.head_row_form(36001) == "global"
    assert ops.head_row_form(1, "auto") == "lds" and ops.head_row_form(131071, "auto") == "global"
    assert ops.head_row_form(150, "global") == "global" and ops.head_row_form(36000, "lds") == "lds"


def test_lds_beyond_36000_is_a_value_error():
    from case_rg_amd import ops
    with pytest.raises(ValueError, match="lds"):
        ops.head_row_form(36001, "lds")
    with pytest.raises(ValueError):
        ops.head_row_form(150, "shared")


def test_wide_entry_points_validate_before_any_launch():
    """Null operands, a missing or misaligned workspace and a vocabulary beyond the key format are refused on the host side."""
    from case_rg_amd import _abi
    with pytest.raises(RuntimeError, match="case_pointer_head_decode_wide"):
        _abi.call("case_pointer_head_decode_wide", *([None] * 5), 1, *([None] * 4), 1, 10, 1, None, 0, None, 0, 0, 0, -1, None)
    with pytest.raises(RuntimeError, match="case_pointer_head_beam_wide"):
        _abi.call("case_pointer_head_beam_wide", *([None] * 5), 1, *([None] * 4), 1, 10, 1, 4, None, 0, None, 0, 0, 0, -1, None)
    with pytest.raises(RuntimeError, match="case_pointer_head_sample_wide"):
        _abi.call("case_pointer_head_sample_wide", *([None] * 5), 0, *([None] * 7), 1, 10, 0, 1.0, 0, 1.0, 0, 0, None, -1, -1, 0, 0, 0,
                  None, 0, None, 0, 0, 0, None)
    # a ready distribution beyond 2^24 entries: unsupported, whatever else is given (fake non-null addresses: nothing is launched or read)
    fake = 1 << 20
    with pytest.raises(RuntimeError, match="built for V <= 16777216"):
        _abi.call("case_pointer_head_sample_wide", *([None] * 5), 0, fake, None, None, fake, fake, fake, None, 1, (1 << 24) + 1, 0, 1.0, 0, 1.0, 0, 0,
                  None, -1, -1, 0, 0, 0, None, 0, None, 0, 0, 0, None)
    # an unaligned V without a workspace: the copy form needs one
    with pytest.raises(RuntimeError, match="row workspace"):
        _abi.call("case_pointer_head_sample_wide", *([None] * 5), 0, fake, None, None, fake, fake, fake, None, 1, 10, 0, 1.0, 0, 1.0, 0, 0,
                  None, -1, -1, 0, 0, 0, None, 0, None, 0, 0, 0, None)


def test_pointer_head_supported_admits_the_key_format():
    import torch
    from case_rg_amd import ops

    class Stub(ops.SortedSource):
        def __init__(self):
            pass

    with torch.no_grad():
        assert ops.pointer_head_supported(Stub(), 36000, 2) and ops.pointer_head_supported(Stub(), 36001, 2)
        assert ops.pointer_head_supported(Stub(), 131071, 4) and not ops.pointer_head_supported(Stub(), 131072, 2)
        assert not ops.pointer_head_supported(Stub(), 50265, 5)
