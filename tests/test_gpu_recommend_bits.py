"""recommend() returns the bits it returned before its variants shared one driver.

tools/recommend_bits.py runs a fixed case list over the four variants (cosine and MLP head,
each with popularity: the fast path with and without exclusions, k above it, overflowing rows,
widths outside the MFMA kernels, fewer items than k) on seeded CPU inputs and digests each
call's idx, vals and stats.  tests/recommend_bits_parent.json is that script's output on an
MI355X with the recs.py of the commit before the refactor, on the same library (taken twice
there, identical); the driver issues the same launches, so every digest must be the same."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "recommend_bits", os.path.join(os.path.dirname(HERE), "tools", "recommend_bits.py"))
recommend_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recommend_bits)

with open(os.path.join(HERE, "recommend_bits_parent.json")) as _f:
    PARENT = json.load(_f)


@pytest.mark.parametrize("group", recommend_bits.GROUPS)
def test_bits_equal_the_parent_driver(group):
    got = recommend_bits.run([group])
    want = {name for name in PARENT if name.startswith(group + "/")}
    assert got and set(got) == want, sorted(want ^ set(got))
    wrong = [name for name, digest in got.items() if PARENT[name] != digest]
    assert not wrong, f"{len(wrong)} of {len(got)} results differ from the parent driver: {wrong}"
