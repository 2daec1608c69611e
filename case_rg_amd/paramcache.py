"""The one registry of tensors derived from parameters: bf16 operand casts (ops.cast_param), the encoder chain's fragment packs
(ops._chain_pack), the folded decode projections (MultiheadAttention.absorbed), Highway's packed rows, FusedAdam's bf16 copies.

An entry belongs to a tuple of ``owners`` (nn.Parameters, or None in a fixed position) and a hashable ``tag`` that tells different
copies of the same owners apart; a tag's kind is its first element if it is a tuple, else itself ("cast", "chain", "absorbed",
"highway").  It is served while every owner is the same live object -- held through a weak reference, so a new Parameter at a recycled
``id()`` cannot hit -- and every owner's ``(_version, data_ptr(), device)`` is what it was when the entry was stored: in-place updates
move ``_version``, ``p.data = t`` moves the address.  Writes that move neither (``p.data.copy_()``, a kernel writing through the raw
pointer, ``dist.broadcast(p.data)``) must be followed by ``rewritten()``.  Entries of dead owners go at the next miss.  A stored value
is never None and must never reference its owners strongly (a Parameter, an autograd graph), or the weak references never die."""
import weakref

_entries = {}  # (tag, id of every owner) -> (weak references, stamps, value)
# parameter-rewrite events (``rewritten()`` calls).  stepgraph.StepGraphs compares it to know whether anybody rewrote parameters since
# its last replay; ops._ZeroArena treats each event as a step boundary (an optimizer step is one; a capture and a replay bump it as well)
EPOCH = 0
_nobody = lambda: None  # noqa: E731  (in place of the weak reference where an owner is None)


def cast_tag(t, dtype):
    """Tag of the ``dtype`` copy of ``t`` -- a Parameter or a view of one -- under the owning Parameter: the view's geometry."""
    return ("cast", t.storage_offset(), t.shape, t.stride(), dtype)


def peek(owners, tag):
    """The stored value, or None on a miss."""
    hit = _entries.get((tag, *map(id, owners)))
    if hit is None:
        return None
    for ref, stamp, p in zip(hit[0], hit[1], owners):
        if ref() is not p or (p is not None and stamp != (p._version, p.data_ptr(), p.device)):
            return None
    return hit[2]


def install(owners, tag, value):
    """Store a value made elsewhere as the current copy of ``owners`` under ``tag``."""
    _entries[(tag, *map(id, owners))] = (tuple(_nobody if p is None else weakref.ref(p) for p in owners),
                                                 tuple(None if p is None else (p._version, p.data_ptr(), p.device) for p in owners), value)
    return value


def derived(owners, tag, build):
    """The stored value while every owner stands still; otherwise ``build()``, stored and returned."""
    value = peek(owners, tag)
    if value is None:
        for key in [k for k, (refs, _, _) in _entries.items() if any(r is not _nobody and r() is None for r in refs)]:
            del _entries[key]
        value = install(owners, tag, build())
    return value


def rewritten(keep=()):
    """Parameters were written behind autograd's back: drop every entry, then reinstall ``keep`` -- (parameter, low-precision copy of
    the whole parameter that the writer refreshed in the same pass) pairs -- as they are, without a cast."""
    global EPOCH
    _entries.clear()
    EPOCH += 1
    for p, low in keep:
        install((p,), cast_tag(p, low.dtype), low)


def entries(kind=None):
    """Read-only view for tests: (owners, tag, value) of every entry, or of one kind; a dead owner reads None."""
    for key, (refs, _, value) in list(_entries.items()):
        if kind is None or kind == (key[0][0] if isinstance(key[0], tuple) else key[0]):
            yield tuple(r() for r in refs), key[0], value
