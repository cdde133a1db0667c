"""The bookkeeping of the engine's per-frame stores (vfml/frame_store.py): the one slot ring behind the context, attention and
iteration-zero stores, the rule that finds a window's centre slots consecutive, and the iteration-zero ring's plans.  No GPU,
no tensors: slot numbers, keys and a dictionary."""
import collections
import types

import pytest


def _windows(T, nfr):
    from processing.videoflow_processor import VideoFlowProcessor
    me = types.SimpleNamespace(sequence_length=T)
    return [VideoFlowProcessor.window_indices(me, nfr, i) for i in range(nfr)]


# ---------------------------------------------------------------------------------------------- the slot ring
def test_take_hands_out_slots_in_order_and_evicts_the_owner_of_the_slot_it_reuses():
    from vfml.frame_store import SlotRing
    R = 5
    cache = collections.OrderedDict()
    cache[("f", "other kinds stay")] = 1
    ring = SlotRing("context", R, cache)
    for i in range(R):
        assert ring.take(("c", i), ()) == i
        cache[("c", i)] = i
    assert ring.owner == [("c", i) for i in range(R)] and ring.next == 0
    assert ring.take(("c", R), ()) == 0
    assert list(cache) == [("f", "other kinds stay")] + [("c", i) for i in range(1, R)]
    assert ring.owner[0] == ("c", R) and ring.next == 1
    # an owner whose entry is gone already (a cleared cache, an LRU eviction) is no error; an unkeyed taker owns nothing
    cache.clear()
    assert ring.take(None, ()) == 1 and ring.owner[1] is None
    cache[("c", 2)] = 2
    assert ring.take(("c", "x"), ()) == 2 and cache == {}


def test_take_skips_busy_and_live_slots_and_moves_next_past_them():
    from vfml.frame_store import SlotRing
    ring = SlotRing("context", 4, {})
    ring.next, ring.live = 1, {1}
    assert ring.take("k", {2}) == 3
    assert ring.next == 0
    assert ring.live == {1} and ring.owner == [None, None, None, "k"]


def test_take_raises_when_every_slot_is_in_use():
    from vfml.frame_store import Iter0Ring, SlotRing
    cache = {"old": 1}
    ring = SlotRing("attention", 4, cache)
    assert ring.take("old", ()) == 0
    ring.live = {0, 3}
    with pytest.raises(RuntimeError, match="attention store: every slot is in use by the current window"):
        ring.take("k", {1, 2})
    assert ring.owner == ["old", None, None, None] and cache == {"old": 1}         # (nothing taken, nothing evicted)
    with pytest.raises(RuntimeError, match="iteration-zero store"):
        Iter0Ring(3, {}).take("k", {0, 1, 2})


def test_rings_over_one_cache_have_different_serials():
    from vfml.frame_store import Iter0Ring, SlotRing
    cache = {}
    rings = [SlotRing("context", 4, cache), SlotRing("attention", 4, cache), Iter0Ring(8, cache), SlotRing("context", 4, cache)]
    assert len({r.serial for r in rings}) == len(rings)


@pytest.mark.parametrize("slots,mirrored,want", [
    ([3, 4, 5], 2, 3),
    ([10, 11, 0], 2, 10),
    ([11, 0, 1], 2, 11),
    ([11, 0, 1], 1, None),          # (slot 1 is not mirrored)
    ([9, 11, 0], 2, None),
    ([5, 4, 3], 2, None),
])
def test_window_base(slots, mirrored, want):
    from vfml.frame_store import window_base
    assert window_base(slots, 12, mirrored) == want


def test_frame_context_is_a_tuple_with_named_fields():
    """prefetch_frames finds an entry's tensors by descending tuples, lists and dicts."""
    from vfml.frame_store import FrameContext
    ent = FrameContext("map", {"zr1": "view"}, 3, 7)
    assert isinstance(ent, tuple) and ent.att_slot is None and ent.att_serial is None
    ent = ent._replace(att_slot=2, att_serial=9)
    assert tuple(ent) == ("map", {"zr1": "view"}, 3, 7, 2, 9) and (ent.slot, ent.serial) == (3, 7)


# ---------------------------------------------------------------------------------------------- the iteration-zero ring
def test_ring_bookkeeping_of_a_sliding_job_and_its_clip_ends():
    from vfml import hip
    from vfml.frame_store import Iter0Ring
    cache = collections.OrderedDict()
    cache[("f", "other kinds stay")] = 1
    ring = Iter0Ring(8, cache)
    nfr = 2 * ring.R + 3
    wins = _windows(5, nfr)
    assert wins[0] == [0, 0, 0, 1, 2] and wins[1] == [0, 0, 1, 2, 3] and wins[-1] == [nfr - 3, nfr - 2, nfr - 1, nfr - 1, nfr - 1]
    # the key names the neighbours: frame 0 between (0, 0) and between (0, 1) are different entries
    assert Iter0Ring.entry_key(wins[0], 1) != Iter0Ring.entry_key(wins[0], 2)
    assert Iter0Ring.entry_key(wins[0], 2) == Iter0Ring.entry_key(wins[1], 1)
    assert Iter0Ring.entry_key(wins[0], 2) != Iter0Ring.entry_key(wins[0], 2, tail=(3,))
    straddle = 0
    for i, w in enumerate(wins):
        warm, seeds, new = ring.plan(w)
        slots, modes = [s for s, _ in seeds], [m for _, m in seeds]
        assert len(set(slots)) == 3
        if i == 0:
            assert not warm and modes == [hip.SEED_STORE] * 3 and len(new) == 3
        else:            # clamped windows at either end included: the two older centres hit
            assert warm and modes == [hip.SEED_LOAD, hip.SEED_LOAD, hip.SEED_STORE], (i, modes)
            assert new == [Iter0Ring.entry_key(w, 3)]
            assert slots[:2] == prev[1:], i                       # ... in the slots the last window left them in
            straddle += slots != sorted(slots)
        prev = slots
        assert sum(1 for k in cache if k[0] == "m") <= ring.R
    assert straddle >= 2
    assert cache[("f", "other kinds stay")] == 1
    # the same window again: everything is there, nothing is stored twice
    warm, seeds, new = ring.plan(wins[-1])
    assert warm and [m for _, m in seeds] == [hip.SEED_LOAD, hip.SEED_LOAD, hip.SEED_NONE] and new == []
    # a window whose first centre was evicted long ago runs cold and keeps what it still finds
    warm, seeds, new = ring.plan(wins[nfr - 2])
    assert warm
    warm, seeds, new = ring.plan(wins[3])
    assert not warm and [m for _, m in seeds] == [hip.SEED_STORE] * 3
    # a cleared cache forgets every entry; forget() gives up a window's promises
    cache.clear()
    warm, seeds, new = ring.plan(wins[-1])
    assert not warm and len(new) == 3
    ring.forget(new)
    assert not any(k[0] == "m" for k in cache)
    assert not ring.plan(wins[-1])[0]


def test_ring_bookkeeping_repeated_keys_and_sizes():
    from vfml import hip
    from vfml.frame_store import Iter0Ring
    ring = Iter0Ring(8, {})
    # a two-frame clip: centres 0 (0, 0) twice and 0 (0, 1) - one slot per key, stored once
    warm, seeds, new = ring.plan([0, 0, 0, 0, 1])
    assert not warm and seeds[0][0] == seeds[1][0] != seeds[2][0]
    assert [m for _, m in seeds] == [hip.SEED_STORE, hip.SEED_NONE, hip.SEED_STORE] and len(new) == 2
    # the newest centre's key already stored by an older centre of the same window: loaded there, not stored again
    warm, seeds, new = ring.plan([0, 0, 0, 0, 0])
    assert warm and [m for _, m in seeds] == [hip.SEED_LOAD, hip.SEED_LOAD, hip.SEED_NONE] and new == []
    # three-frame windows have one centre: never warm; nine-frame windows have seven
    assert not Iter0Ring(8, {}).plan([0, 1, 2])[0]
    ring = Iter0Ring(8, {})
    assert not ring.plan(list(range(9)))[0]
    warm, seeds, new = ring.plan(list(range(1, 10)))
    assert warm and [m for _, m in seeds] == [hip.SEED_LOAD] * 6 + [hip.SEED_STORE]
    assert len({s for s, _ in seeds}) == 7
    with pytest.raises(ValueError):
        Iter0Ring(4, {}).plan(list(range(9)))
    # another ring over the same cache does not take this one's entries for its own
    cache = {}
    a, b = Iter0Ring(8, cache), Iter0Ring(8, cache)
    a.plan([0, 1, 2, 3, 4])
    assert not b.plan([1, 2, 3, 4, 5])[0]
