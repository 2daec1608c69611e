"""The 20 C entry points around the fused decode heads (15 x K23 / K24 / K28, 3 x K25, K32 and the rules as launches of their own), the part
that needs no GPU: which entry point a call is routed to, and what each entry point refuses before any launch.

The refusals are a table of bad-argument calls with the code and the message each one gets.  Codes and messages are literals, recorded from a
build of the commit before the host launch path behind these entry points was unified: they pin the text and, where two arguments are bad at
once, which complaint wins.  No call of the table passes validation (nothing here may reach a launch): operands are nulls, or fake non-null
addresses that are never read; the two arrays the host side does read (the copy pointers and the lengths) are real."""
import ctypes as C

import pytest

ARG, UNSUPPORTED = -1, -2  # CASE_E_ARG, CASE_E_UNSUPPORTED
HEADS = ("decode", "beam", "sample")
FORMS = ("", "_ban", "_wide", "_rules", "_wide_rules")

# ---- the naming function ----------------------------------------------------------------------------------------------------------------------
# (head, row, ban given, rules given) -> entry point, written out from the five-way ladders the three public functions carried
NAMES = {
    ("decode", "lds", False, False): "case_pointer_head_decode",
    ("decode", "lds", True, False): "case_pointer_head_decode_ban",
    ("decode", "lds", False, True): "case_pointer_head_decode_rules",
    ("decode", "lds", True, True): "case_pointer_head_decode_rules",
    ("decode", "global", False, False): "case_pointer_head_decode_wide",
    ("decode", "global", True, False): "case_pointer_head_decode_wide",
    ("decode", "global", False, True): "case_pointer_head_decode_wide_rules",
    ("decode", "global", True, True): "case_pointer_head_decode_wide_rules",
    ("beam", "lds", False, False): "case_pointer_head_beam",
    ("beam", "lds", True, False): "case_pointer_head_beam_ban",
    ("beam", "lds", False, True): "case_pointer_head_beam_rules",
    ("beam", "lds", True, True): "case_pointer_head_beam_rules",
    ("beam", "global", False, False): "case_pointer_head_beam_wide",
    ("beam", "global", True, False): "case_pointer_head_beam_wide",
    ("beam", "global", False, True): "case_pointer_head_beam_wide_rules",
    ("beam", "global", True, True): "case_pointer_head_beam_wide_rules",
    ("sample", "lds", False, False): "case_pointer_head_sample",
    ("sample", "lds", True, False): "case_pointer_head_sample_ban",
    ("sample", "lds", False, True): "case_pointer_head_sample_rules",
    ("sample", "lds", True, True): "case_pointer_head_sample_rules",
    ("sample", "global", False, False): "case_pointer_head_sample_wide",
    ("sample", "global", True, False): "case_pointer_head_sample_wide",
    ("sample", "global", False, True): "case_pointer_head_sample_wide_rules",
    ("sample", "global", True, True): "case_pointer_head_sample_wide_rules",
}


def test_head_entry_names_all_24_combinations():
    from case_rg_amd import _abi, ops
    assert len(NAMES) == 24
    for (head, row, ban, rules), name in NAMES.items():
        assert ops.head_entry(head, row, ban, rules) == name, (head, row, ban, rules)
        assert name in _abi.SIGNATURES and hasattr(_abi.lib, name), name
    assert set(NAMES.values()) == {"case_pointer_head_" + h + f for h in HEADS for f in FORMS}


# ---- the refusals -----------------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20  # a non-null, 16-byte aligned address that nothing reads
COPIES = (C.c_void_p * 2)(FAKE, FAKE)  # read on the host side: the copy pointers and the lengths of two memories, 5 + 3 = S
LENS = (C.c_int64 * 2)(5, 3)

BAD = "{who}: bad argument"
HIST = "{who}: bad history argument"
STEP = "{who}: the n-gram ban stages histories of up to 256 tokens (step 257)"
LDS_V = "{who}: built for <= 4 memories, V <= 36000, S <= 32768 (run the softmax / scatter / argmax launches)"
WIDE_V = "{who}: built for <= 4 memories, V <= 131071, S <= 32768"
SUM = "{who}: the memories hold 8 positions, the source map 9"
WS = "{who}: the row workspace must be 16-byte aligned f32 [rows, row_stride], row_stride >= V and a multiple of 4"
RULE = "{who}: bad rule argument (t >= 0, min_length >= 0, banned [K] with stride 0 or [rows / rows_per_item, K] with stride K)"
MANY = "{who}: at most 256 banned ids per item (got 257)"
WIDTH = "{who}: width %d outside 1 .. min(8, V)"
TEMP = "{who}: temperature must be > 0, top_k >= 0 and top_p in (0, 1]"
EITHER = "{who}: give either the logits or a ready distribution"
DIST_V = "{who}: built for V <= %d"
ADV_W = "{who}: width %d outside 1 .. 8"
PENALTY = "case_beam_advance_rules: the length penalty must be a finite float >= 0"

HEAD_DEFAULTS = dict(
    logits=FAKE, mix=FAKE, keys=FAKE, copies=COPIES, lens=LENS, nmem=2, dist_in=None, gen=None, dist=None, ids=FAKE, top=None, cand_p=FAKE,
    cand_id=FAKE, prob=FAKE, ended=FAKE, uniforms=None, R=3, V=37, S=8, W=2, temperature=1.0, top_k=0, top_p=1.0, seed=0, offset=0, state=None,
    eos=4, unk=1, pad=0, first=0, last=0, ws=FAKE, stride=40, hist=FAKE, Tmax=6, t=3, n=2, ban_eos=-1, rule_eos=4, min_length=5, banned=FAKE, K=2,
    banned_stride=0, rows_per_item=1)
HEAD_POINTERS = ("logits", "mix", "keys", "copies", "lens", "dist_in", "gen", "dist", "ids", "top", "cand_p", "cand_id", "prob", "ended", "uniforms",
                 "state", "ws", "hist", "banned")
NULLS = dict.fromkeys(HEAD_POINTERS)
OWN = {"decode": "ids", "beam": "cand_id", "sample": "prob"}  # an output of the head's own, checked before the shared operands
READY = dict(logits=None, dist_in=FAKE)  # K28 on a ready distribution


def head_args(head, form, over):
    v = dict(HEAD_DEFAULTS, **over)
    a = [v["logits"], v["mix"], v["keys"], v["copies"], v["lens"], v["nmem"]]
    if head == "decode":
        a += [v["gen"], v["dist"], v["ids"], v["top"], v["R"], v["V"], v["S"]]
    elif head == "beam":
        a += [v["gen"], v["dist"], v["cand_p"], v["cand_id"], v["R"], v["V"], v["S"], v["W"]]
    else:
        a += [v["dist_in"], v["gen"], v["dist"], v["ids"], v["prob"], v["ended"], v["uniforms"], v["R"], v["V"], v["S"], v["temperature"], v["top_k"],
              v["top_p"], v["seed"], v["offset"], v["state"], v["eos"], v["unk"], v["pad"], v["first"], v["last"]]
    if "_wide" in form:
        a += [v["ws"], v["stride"]]
    if form:
        a += [v["hist"], v["Tmax"], v["t"], v["n"]] + ([] if head == "sample" else [v["ban_eos"]])  # (the sampler's history uses the loop's eos)
    if form.endswith("_rules"):
        a += [v["rule_eos"], v["min_length"], v["banned"], v["K"], v["banned_stride"], v["rows_per_item"]]
    return a + [None]


LATE_STEP = dict(t=257, Tmax=300)
# form -> (what is wrong, the operands that differ from a valid call, code, message); the same for the three heads
SHARED = {
    "": [
        ("all null", NULLS, ARG, BAD),
        ("V 36001", dict(V=36001), UNSUPPORTED, LDS_V),
        ("V 36001, own output null", dict(V=36001, own=None), ARG, BAD),
        ("keys null", dict(keys=None), ARG, BAD),
        ("five memories", dict(nmem=5), UNSUPPORTED, LDS_V),
        ("lengths do not add up to S", dict(S=9), ARG, SUM),
    ],
    "_ban": [
        ("all null", NULLS, ARG, HIST),
        ("history null", dict(hist=None), ARG, HIST),
        ("n 0", dict(n=0), ARG, HIST),
        ("t == Tmax", dict(t=6), ARG, HIST),
        ("t 257", LATE_STEP, UNSUPPORTED, STEP),
        ("history null, V 36001", dict(hist=None, V=36001), ARG, HIST),
        ("n 0, own output null", dict(n=0, own=None), ARG, HIST),
        ("V 36001", dict(V=36001), UNSUPPORTED, LDS_V),
        ("own output null", dict(own=None), ARG, BAD),
    ],
    "_wide": [
        ("all null", NULLS, ARG, BAD),
        ("V 131072", dict(V=131072, stride=131072), UNSUPPORTED, WIDE_V),
        ("workspace null", dict(ws=None), ARG, WS),
        ("workspace misaligned", dict(ws=FAKE + 4), ARG, WS),
        ("row_stride < V", dict(stride=36), ARG, WS),
        ("row_stride % 4", dict(stride=38), ARG, WS),
        ("t 257", LATE_STEP, UNSUPPORTED, STEP),
        ("n -1", dict(n=-1), ARG, HIST),
        ("n 0 is no ban (t 257 passes), workspace null", dict(n=0, ws=None, **LATE_STEP), ARG, WS),
        ("history null is no ban (t 257 passes), workspace null", dict(hist=None, ws=None, **LATE_STEP), ARG, WS),
        ("workspace null, V 131072", dict(ws=None, V=131072), UNSUPPORTED, WIDE_V),
        ("workspace null, own output null", dict(ws=None, own=None), ARG, BAD),
        ("t 257, own output null", dict(own=None, **LATE_STEP), UNSUPPORTED, STEP),
    ],
    "_rules": [
        ("all null", NULLS, ARG, RULE),
        ("K 257", dict(K=257), UNSUPPORTED, MANY),
        ("banned_stride 1", dict(banned_stride=1), ARG, RULE),
        ("banned_stride K, rows no multiple of rows_per_item", dict(banned_stride=2, rows_per_item=2), ARG, RULE),
        ("min_length -1", dict(min_length=-1), ARG, RULE),
        ("t 257", LATE_STEP, UNSUPPORTED, STEP),
        ("no ban (t 257 passes), V 36001", dict(hist=None, n=0, V=36001, **LATE_STEP), UNSUPPORTED, LDS_V),
        ("K 257, own output null", dict(K=257, own=None), UNSUPPORTED, MANY),
        ("n -1, K 257", dict(n=-1, K=257), ARG, HIST),
        ("V 36001", dict(V=36001), UNSUPPORTED, LDS_V),
        ("own output null", dict(own=None), ARG, BAD),
    ],
    "_wide_rules": [
        ("all null", NULLS, ARG, RULE),
        ("K 257", dict(K=257), UNSUPPORTED, MANY),
        ("banned_stride 1", dict(banned_stride=1), ARG, RULE),
        ("workspace null", dict(ws=None), ARG, WS),
        ("workspace misaligned", dict(ws=FAKE + 4), ARG, WS),
        ("row_stride < V", dict(stride=36), ARG, WS),
        ("row_stride % 4", dict(stride=38), ARG, WS),
        ("V 131072", dict(V=131072, stride=131072), UNSUPPORTED, WIDE_V),
        ("t 257", LATE_STEP, UNSUPPORTED, STEP),
        ("workspace null, K 257", dict(ws=None, K=257), UNSUPPORTED, MANY),
        ("workspace null, own output null", dict(ws=None, own=None), ARG, BAD),
    ],
}
# what K24's width adds: checked behind the candidates' pointers, before the shared operands
BEAM = {
    "": [("W 0", dict(W=0), UNSUPPORTED, WIDTH % 0), ("W 9", dict(W=9), UNSUPPORTED, WIDTH % 9), ("W > V", dict(V=1), UNSUPPORTED, WIDTH % 2),
         ("W 0, cand_p null", dict(W=0, cand_p=None), ARG, BAD), ("W 9, V 36001", dict(W=9, V=36001), UNSUPPORTED, WIDTH % 9)],
    "_ban": [("W 0", dict(W=0), UNSUPPORTED, WIDTH % 0), ("W 9", dict(W=9), UNSUPPORTED, WIDTH % 9),
             ("W 0, history null", dict(W=0, hist=None), ARG, HIST)],
    "_wide": [("W 0", dict(W=0), UNSUPPORTED, WIDTH % 0), ("W 9", dict(W=9), UNSUPPORTED, WIDTH % 9),
              ("W 0, workspace null", dict(W=0, ws=None), UNSUPPORTED, WIDTH % 0)],
    "_rules": [("W 0", dict(W=0), UNSUPPORTED, WIDTH % 0), ("W 9", dict(W=9), UNSUPPORTED, WIDTH % 9),
               ("W 0, K 257", dict(W=0, K=257), UNSUPPORTED, MANY)],
    "_wide_rules": [("W 0", dict(W=0), UNSUPPORTED, WIDTH % 0), ("W 9", dict(W=9), UNSUPPORTED, WIDTH % 9),
                    ("W 9, banned_stride 1", dict(W=9, banned_stride=1), ARG, RULE)],
}
# what K28's draw adds: ids / prob / ended, then the temperature, then "either logits or dist_in", all before the row's operands
DRAW = [
    ("temperature 0", dict(temperature=0.0), ARG, TEMP),
    ("top_p 0", dict(top_p=0.0), ARG, TEMP),
    ("logits and dist_in", dict(dist_in=FAKE), ARG, EITHER),
    ("neither logits nor dist_in", dict(logits=None), ARG, EITHER),
    ("temperature 0, ids null", dict(temperature=0.0, ids=None), ARG, BAD),
    ("logits and dist_in, temperature 0", dict(dist_in=FAKE, temperature=0.0), ARG, TEMP),
    ("logits and dist_in, V beyond the form", dict(dist_in=FAKE, V=1 << 25), ARG, EITHER),
]
SAMPLE = {
    "": DRAW + [("dist_in, V 36001", dict(READY, V=36001), UNSUPPORTED, DIST_V % 36000)],
    "_ban": DRAW + [("dist_in, V 36001", dict(READY, V=36001), UNSUPPORTED, DIST_V % 36000),
                    ("temperature 0, history null", dict(temperature=0.0, hist=None), ARG, HIST)],
    "_wide": DRAW + [("dist_in, V 2^24 + 1", dict(READY, V=(1 << 24) + 1, stride=(1 << 24) + 4), UNSUPPORTED, DIST_V % (1 << 24)),
                     ("dist_in unaligned rows (V 37), workspace null", dict(READY, n=0, ws=None), ARG, WS),
                     ("dist_in misaligned, V 40, workspace null", dict(READY, dist_in=FAKE + 4, V=40, n=0, ws=None), ARG, WS),
                     ("dist_in aligned, V 40, a ban, workspace null", dict(READY, V=40, ws=None), ARG, WS),
                     ("temperature 0, workspace null", dict(temperature=0.0, ws=None), ARG, TEMP)],
    "_rules": DRAW + [("dist_in, V 36001", dict(READY, V=36001), UNSUPPORTED, DIST_V % 36000),
                      ("temperature 0, K 257", dict(temperature=0.0, K=257), UNSUPPORTED, MANY)],
    "_wide_rules": DRAW + [("dist_in, V 2^24 + 1", dict(READY, V=(1 << 24) + 1, stride=(1 << 24) + 4), UNSUPPORTED, DIST_V % (1 << 24)),
                           ("dist_in aligned, V 40, no ban, workspace null: the rules keep it out of place",
                            dict(READY, V=40, hist=None, n=0, ws=None), ARG, WS),
                           ("neither logits nor dist_in, banned_stride 1", dict(logits=None, banned_stride=1), ARG, RULE)],
}

ADVANCE_DEFAULTS = dict(
    cand_p=FAKE, cand_id=FAKE, alive=FAKE, cum=FAKE, len=FAKE, parent=FAKE, token=FAKE, hist_parent=FAKE, hist_token=FAKE, fin_key=FAKE,
    fin_step=FAKE, fin_slot=FAKE, t=3, T=6, B=2, W=2, eos=4, flat_old=FAKE, flat_new=FAKE + 64, Tmax=6, alpha=0.5)
ADVANCE_POINTERS = tuple(ADVANCE_DEFAULTS)[:12]
ADVANCE_NULLS = dict.fromkeys(ADVANCE_POINTERS + ("flat_old", "flat_new"))
BY_BAN = "case_beam_advance_ban"  # alpha == 1 is case_beam_advance_ban's call, and reports as it


def advance_args(form, over):
    v = dict(ADVANCE_DEFAULTS, **over)
    a = [v[k] for k in ADVANCE_POINTERS] + [v["t"], v["T"], v["B"], v["W"], v["eos"]]
    if form:
        a += [v["flat_old"], v["flat_new"], v["Tmax"]]
    if form == "_rules":
        a += [v["alpha"]]
    return a + [None]


ADVANCE = {
    "": [
        ("all null", ADVANCE_NULLS, ARG, BAD),
        ("W 0", dict(W=0), UNSUPPORTED, ADV_W % 0),
        ("W 9", dict(W=9), UNSUPPORTED, ADV_W % 9),
        ("t == T", dict(t=6), ARG, BAD),
        ("B 0", dict(B=0), ARG, BAD),
        ("W 9, cand_p null", dict(W=9, cand_p=None), ARG, BAD),
    ],
    "_ban": [
        ("all null", ADVANCE_NULLS, ARG, BAD),
        ("flat_old null", dict(flat_old=None), ARG, BAD),
        ("flat_new null", dict(flat_new=None), ARG, BAD),
        ("one flat buffer", dict(flat_new=FAKE), ARG, BAD),
        ("t == Tmax", dict(Tmax=3), ARG, BAD),
        ("W 0", dict(W=0), UNSUPPORTED, ADV_W % 0),
        ("W 9", dict(W=9), UNSUPPORTED, ADV_W % 9),
        ("W 9, flat_old null", dict(W=9, flat_old=None), ARG, BAD),
    ],
    "_rules": [
        ("all null", ADVANCE_NULLS, ARG, BAD),
        ("length_penalty -0.5", dict(alpha=-0.5), ARG, PENALTY),
        ("length_penalty inf", dict(alpha=float("inf")), ARG, PENALTY),
        ("length_penalty nan", dict(alpha=float("nan")), ARG, PENALTY),
        ("length_penalty -1, all null", dict(ADVANCE_NULLS, alpha=-1.0), ARG, PENALTY),
        ("length_penalty -1, W 9", dict(alpha=-1.0, W=9), ARG, PENALTY),
        ("length_penalty 1, flat_old null", dict(alpha=1.0, flat_old=None), ARG, BY_BAN + ": bad argument"),
        ("length_penalty 1, all null", dict(ADVANCE_NULLS, alpha=1.0), ARG, BY_BAN + ": bad argument"),
        ("length_penalty 1, W 9", dict(alpha=1.0, W=9), UNSUPPORTED, BY_BAN + ": width 9 outside 1 .. 8"),
        ("flat_old null", dict(flat_old=None), ARG, BAD),
        ("one flat buffer", dict(flat_new=FAKE), ARG, BAD),
        ("W 0", dict(W=0), UNSUPPORTED, ADV_W % 0),
        ("W 9", dict(W=9), UNSUPPORTED, ADV_W % 9),
        ("W 9, flat_new null", dict(W=9, flat_new=None), ARG, BAD),
    ],
}

ROW_DEFAULTS = dict(dist=FAKE, hist=FAKE, ended=None, R=3, V=37, Tmax=6, t=3, n=2, eos=4, min_length=5, banned=FAKE, K=2, banned_stride=0,
                    rows_per_item=1)
NGRAM_BAN = [
    ("all null", dict(dist=None, hist=None), ARG, BAD),
    ("history null", dict(hist=None), ARG, HIST),
    ("n 0", dict(n=0), ARG, HIST),
    ("t == Tmax", dict(t=6), ARG, HIST),
    ("t 257", LATE_STEP, UNSUPPORTED, STEP),
    ("R 0", dict(R=0), ARG, BAD),
    ("dist null, n 0", dict(dist=None, n=0), ARG, BAD),
    ("n 0, t 257", dict(n=0, **LATE_STEP), ARG, HIST),
]
ROW_RULES = [
    ("all null", dict(dist=None, banned=None), ARG, BAD),
    ("K 257", dict(K=257), UNSUPPORTED, MANY),
    ("banned_stride 1", dict(banned_stride=1), ARG, RULE),
    ("banned null", dict(banned=None), ARG, RULE),
    ("t -1", dict(t=-1), ARG, RULE),
    ("rows_per_item 0", dict(rows_per_item=0), ARG, RULE),
    ("dist null, K 257", dict(dist=None, K=257), ARG, BAD),
    ("K 257, banned_stride 1", dict(K=257, banned_stride=1), ARG, RULE),
]


def row_args(name, over):
    v = dict(ROW_DEFAULTS, **over)
    if name == "case_ngram_ban":
        return [v["dist"], v["hist"], v["ended"], v["R"], v["V"], v["Tmax"], v["t"], v["n"], v["eos"], None]
    return [v["dist"], v["ended"], v["R"], v["V"], v["t"], v["eos"], v["min_length"], v["banned"], v["K"], v["banned_stride"], v["rows_per_item"], None]


def refusals():
    """-> [(entry point, what is wrong, the argument list, code, message)] over the 20 entry points."""
    out = []
    for head in HEADS:
        for form in FORMS:
            name = "case_pointer_head_" + head + form
            for what, over, code, msg in SHARED[form] + {"decode": {}, "beam": BEAM, "sample": SAMPLE}[head].get(form, []):
                over = dict(over)
                if "own" in over:
                    over[OWN[head]] = over.pop("own")
                out.append((name, what, head_args(head, form, over), code, msg.format(who=name)))
    for form, rows in ADVANCE.items():
        name = "case_beam_advance" + form
        out += [(name, what, advance_args(form, over), code, msg.format(who=name)) for what, over, code, msg in rows]
    for name, rows in (("case_ngram_ban", NGRAM_BAN), ("case_row_rules", ROW_RULES)):
        out += [(name, what, row_args(name, over), code, msg.format(who=name)) for what, over, code, msg in rows]
    return out


REFUSALS = refusals()


def test_the_table_covers_every_entry_point_and_only_refusals():
    from case_rg_amd import _abi
    names = {r[0] for r in REFUSALS}
    assert names == ({"case_pointer_head_" + h + f for h in HEADS for f in FORMS}
                     | {"case_beam_advance", "case_beam_advance_ban", "case_beam_advance_rules", "case_ngram_ban", "case_row_rules"})
    for name, what, args, code, msg in REFUSALS:
        assert code in (ARG, UNSUPPORTED), (name, what)
        assert len(args) == len(_abi.SIGNATURES[name]), (name, what)


@pytest.mark.parametrize("name,what,args,code,msg", REFUSALS, ids=["%s: %s" % (r[0][5:], r[1]) for r in REFUSALS])
def test_refused_before_any_launch(name, what, args, code, msg):
    from case_rg_amd import _abi
    got = getattr(_abi.lib, name)(*args)
    assert (got, _abi.lib.case_last_error().decode()) == (code, msg)
