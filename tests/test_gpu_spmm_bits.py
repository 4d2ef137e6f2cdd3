"""The a1 aggregation family writes the bits its parent build wrote.

tools/spmm_bits.py runs a fixed case list over every form of the neighbour gather (plain,
packed, two relations, dropout; static schedule, heavy-row split by host plan, device plan and
overflowed device plan, group form, row queue) on seeded CPU inputs and digests each output.
tests/spmm_bits_parent.json is that script's output on an MI355X with the build before the
kernels were unified (taken twice there, identical); the reduction order is the project's
reproducibility contract, so every digest must still be the same."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "spmm_bits", os.path.join(os.path.dirname(HERE), "tools", "spmm_bits.py"))
spmm_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(spmm_bits)

with open(os.path.join(HERE, "spmm_bits_parent.json")) as _f:
    PARENT = json.load(_f)
CASES = spmm_bits.cases()
GROUPS = sorted({group for group, _, _ in CASES})


def test_every_case_has_a_parent_digest():
    names = [name for _, name, _ in CASES]
    assert len(set(names)) == len(names)
    assert set(names) == set(PARENT)
    assert GROUPS == ["dropout", "group", "out", "packed", "plain", "queued", "spmm2"]


@pytest.mark.parametrize("group", GROUPS)
def test_bits_equal_the_parent_build(group):
    got = spmm_bits.run([group])
    assert got, group
    wrong = [name for name, digest in got.items() if PARENT[name] != digest]
    assert not wrong, f"{len(wrong)} of {len(got)} outputs differ from the parent build: {wrong[:8]}"
