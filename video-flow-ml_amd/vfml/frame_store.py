"""Bookkeeping of the engine's per-frame stores (vfml/network.py: the gates' context parts, the GMA attention planes, the
first-iteration motion features).  No tensors here: slot numbers, keys, and the cache dictionary the entries live in.

The one mechanism (SlotRing): a store is a ring of frame slots handed out round robin, skipping the slots the current
window (`busy`) or the last one (`live`: its launches may still read them) uses.  A slot handed out again takes its old
owner's entry out of the cache the entries live in (the engine's `_feat_cache`: whatever clears that cache forgets the
entries), and the ring's serial marks the entries of a store that has been rebuilt since as stale.  What a store's slots
hold, when it is rebuilt and when `live` is written is the engine's business."""
import itertools
from typing import Any, NamedTuple, Optional

from .hip import SEED_LOAD, SEED_NONE, SEED_STORE       # (vfml_window_seed's modes: all this module takes from the library)

_serials = itertools.count(1)       # one counter for every ring of the process: a serial is never seen twice


class SlotRing:
    def __init__(self, name, slots, cache):
        self.name, self.R, self.cache = name, slots, cache
        self.next, self.owner, self.live, self.serial = 0, [None] * slots, set(), next(_serials)

    def take(self, key, busy=()):
        """The next slot of the ring (not one of `busy` or `live`) for `key`; whoever owned it loses its cache entry - `key`
        itself included, should it own the slot already: the taker puts its entry (again) once the slot is filled."""
        busy = set(busy) | self.live
        for _ in range(self.R):
            s = self.next
            self.next = (s + 1) % self.R
            if s not in busy:
                break
        else:
            raise RuntimeError(f"{self.name} store: every slot is in use by the current window")
        if self.owner[s] is not None:
            self.cache.pop(self.owner[s], None)
        self.owner[s] = key
        return s


def window_base(slots, R, mirrored):
    """The first slot of a window whose centre frames' slots are consecutive in a ring of R slots - straight, or through
    the ring's first `mirrored` slots, which are kept a second time behind it (slot s at R + s) so that a window that wraps
    is consecutive too.  None: they are not (random access), the window's parts have to be gathered."""
    first = slots[0]
    if all(s == first + i or (first + i >= R and s == first + i - R and s < mirrored) for i, s in enumerate(slots)):
        return first
    return None


class FrameContext(NamedTuple):
    """A centre frame's context cache entry (kind "c").  A tuple on purpose: whoever looks for an entry's tensors descends
    tuples, lists and dicts (MOFNetHIP.prefetch_frames)."""
    map: Any                            # the context map, tanh | relu halves
    addends: dict                       # {gate: view of the frame's slot in the gate's store}
    slot: int
    serial: int                         # ... of the context store the slot is in
    att_slot: Optional[int] = None      # with the GMA aggregator: the slot of the frame's attention, and that store's serial
    att_serial: Optional[int] = None


class Iter0Ring(SlotRing):
    """The iteration-zero store's ring: which slot holds which centre frame's first-iteration motion features.  Entries are
    of kind "m", (slot, serial).

    At iteration 0 the flow is zero, so a centre frame's motion features depend on its two correlation pyramids alone -
    on the frame AND its two neighbours in the window.  The key is therefore the cache keys of all three: a window clamped
    at the start of a clip gives frame 0 the neighbours (0, 0), the next one (0, 1) - different entries."""

    def __init__(self, slots, cache):
        super().__init__("iteration-zero", slots, cache)

    @staticmethod
    def entry_key(keys, j, tail=()):
        """Key of frame j (1 <= j <= len(keys) - 2) of a window whose frames have the cache keys `keys`."""
        return ("m", keys[j - 1], keys[j], keys[j + 1]) + tuple(tail)

    def lookup(self, ek):
        ent = self.cache.get(ek)
        if ent is not None and ent[1] == self.serial and self.owner[ent[0]] == ek:
            return ent[0]
        return None

    def forget(self, eks):
        for ek in eks:
            s = self.lookup(ek)
            if s is not None:
                self.owner[s] = None
                del self.cache[ek]

    def plan(self, keys, tail=()):
        """A window's slots: (warm, [(slot, mode)] per centre frame, keys of the entries this window fills).
        warm: every centre but the newest (the last) has an entry - those are loaded (SEED_LOAD) and only the newest is
        computed, and stored unless it has an entry already.  Else every centre is computed and those without an entry are
        stored (SEED_STORE); a key that occurs twice in a window is stored once."""
        M = len(keys) - 2
        if M + 1 > self.R:
            raise ValueError(f"iteration-zero store: {self.R} slots cannot serve {M} centre frames")
        eks = [self.entry_key(keys, j, tail) for j in range(1, M + 1)]
        found = [self.lookup(ek) for ek in eks]
        warm = M >= 2 and all(s is not None for s in found[:-1])
        busy = {s for s in found if s is not None}
        out, new = [], []
        for i, ek in enumerate(eks):
            s = self.lookup(ek)           # (again: an earlier centre of this window may just have taken a slot for this key)
            if s is not None:
                out.append((s, SEED_LOAD if warm and i < M - 1 else SEED_NONE))
            else:
                s = self.take(ek, busy)
                self.cache[ek] = (s, self.serial)
                busy.add(s)
                new.append(ek)
                out.append((s, SEED_STORE))
        return warm, out, new
