"""The fused aggregate+project kernels write the bits their parent build wrote.

tools/fused_bits.py runs a fixed case list over the four kernels of csrc/spmm_project.hip and
csrc/spmm_pair_mfma.hip (every template instantiation, the epilogues and accumulate modes,
ragged row counts, the row queue) on seeded CPU inputs and digests each output.
tests/fused_bits_parent.json is that script's output on an MI355X with the libraries of the
build before the kernels shared their gather, tile walk and epilogue (taken twice there,
identical); the refactor changes no summation order, so every digest must still be the same."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "fused_bits", os.path.join(os.path.dirname(HERE), "tools", "fused_bits.py"))
fused_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fused_bits)

with open(os.path.join(HERE, "fused_bits_parent.json")) as _f:
    PARENT = json.load(_f)
GROUPS = sorted({group for group, _, _ in fused_bits.cases()})


@pytest.mark.parametrize("group", GROUPS)
def test_bits_equal_the_parent_build(group):
    got = fused_bits.run([group])
    assert got, group
    wrong = [name for name, digest in got.items() if PARENT[name] != digest]
    assert not wrong, f"{len(wrong)} of {len(got)} outputs differ from the parent build: {wrong[:8]}"
