"""Every engine's fields on small seeded cases, bit for bit against tests/golden/engine_digests.json, and the kernels three of
them launch against the census recorded there.  The file is recorded by tests/golden/make_engine_digests.py from the tree
BEFORE a change that is meant to leave arithmetic and launch order alone (its docstring says when to record it again); the
cases reach every branch of the update block's launch sequences (vfml/update_block.py and its two callers)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load():
    spec = importlib.util.spec_from_file_location("make_engine_digests", os.path.join(GOLDEN, "make_engine_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLDEN, "engine_digests.json")) as f:
        return mod, json.load(f)


MAKE, RECORDED = _load()


def test_every_case_is_recorded():
    assert sorted(RECORDED["digests"]) == sorted(MAKE.CASES)
    assert sorted(RECORDED["census"]) == sorted(MAKE.CENSUS)
    assert all(RECORDED["digests"][c] for c in MAKE.CASES)


@pytest.mark.parametrize("case", sorted(MAKE.CASES))
def test_fields_are_bit_identical(gpu, case):
    got = MAKE.CASES[case]()
    want = RECORDED["digests"][case]
    differ = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
    print(f"[digests] {case}: {len(want)} tensors, {len(differ)} differ")
    assert not differ, f"{case}: other bits than recorded in {differ}"


@pytest.mark.parametrize("case", sorted(MAKE.CENSUS))
def test_same_kernels_same_number_of_times(gpu, case):
    got = MAKE.CENSUS[case]()
    want = RECORDED["census"][case]
    differ = {v: (got.get(v), want.get(v)) for v in set(got) | set(want) if got.get(v) != want.get(v)}
    print(f"[census] {case}: {sum(sum(s.values()) for s in want.values())} launches recorded")
    assert not differ, f"{case}: (launched, recorded) per kernel variant {differ}"
