"""Bookkeeping of the exact-arithmetic GPU tests (test_gemm_exact_gpu.py, test_attention_exact_gpu.py, test_interaction_exact_gpu.py,
test_encoder_chain_exact_gpu.py, test_additive_exact_gpu.py, test_pointer_decode_exact_gpu.py) and of test_row_ops_gpu.py
(profiles/row_ops_parity.json): per test function the C entry points that ran,
the cases, and the number of elements compared exactly and by a bound.  It is what profiles/exact_parity.json,
profiles/fused_exact_parity.json and profiles/additive_exact_parity.json are made from;
no assertion depends on it.  Nothing is written unless CASE_EXACT_LEDGER names a file."""
import pytest

LEDGER = {}
_CURRENT = [None]


def begin(family, case):
    _CURRENT[0] = LEDGER.setdefault(family, {"entry_points": [], "cases": [], "elements": 0, "exact": 0, "bounded": 0, "bound_reasons": []})
    _CURRENT[0]["cases"].append(case)


def end(entry_points):
    cur, _CURRENT[0] = _CURRENT[0], None
    cur["entry_points"] = sorted(set(cur["entry_points"]) | set(entry_points))
    if len(LEDGER) == 1 and len(cur["cases"]) == 1:
        import atexit
        atexit.register(_dump)


def record(exact, bounded=0, reason=None):
    cur = _CURRENT[0]
    if cur is None:
        return
    cur["elements"] += int(exact) + int(bounded)
    cur["exact"] += int(exact)
    cur["bounded"] += int(bounded)
    if bounded and reason and reason not in cur["bound_reasons"]:
        cur["bound_reasons"].append(reason)


def note(key, value):
    """A measured figure of the current test (LayerNorm flip shares, eps_phi, per-segment errors), kept under "figures"."""
    cur = _CURRENT[0]
    if cur is not None:
        cur.setdefault("figures", {})[key] = value


def _dump():
    """At exit: the ledger as JSON at the path CASE_EXACT_LEDGER names (unset: nothing is written); each test file's process adds its
    families to the file."""
    import json
    import os
    path, merged = os.environ.get("CASE_EXACT_LEDGER"), {}
    if not path:
        return
    if os.path.exists(path):
        with open(path) as fh:
            merged = json.load(fh)
    merged.update(LEDGER)
    with open(path, "w") as fh:
        json.dump(merged, fh, indent=1, sort_keys=True)
        fh.write("\n")


@pytest.fixture(autouse=True)
def ledger(request):
    """Notes the C entry points the test makes (a spy on _abi.call) and opens the test's entry."""
    from case_rg_amd import _abi
    raw, seen = _abi.call, set()

    def spy(name, *a):
        seen.add(name)
        return raw(name, *a)

    _abi.call = spy
    begin(request.node.originalname, request.node.name)
    try:
        yield
    finally:
        _abi.call = raw
        end(seen)
