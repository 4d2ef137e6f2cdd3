"""The GEMM kernels write the bits their parent build wrote.

tools/gemm_bits.py runs a fixed case list over csrc/gemm.hip (every instantiation of the
LDS-DMA kernel the dispatch can pick, both operand pairs with both degree modes, the
compile-time and run-time epilogues, accumulate modes, ragged row and column counts, and the
register-staged general kernel) on seeded CPU inputs and digests everything each call writes.
tests/gemm_bits_parent.json is that script's output on an MI355X with the library of the build
before the two LDS-DMA kernels became one (taken twice there, identical); the merge keeps the
k order, the degree transform of each depth and each instantiation's epilogue, so every digest
must still be the same."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "gemm_bits", os.path.join(os.path.dirname(HERE), "tools", "gemm_bits.py"))
gemm_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gemm_bits)

with open(os.path.join(HERE, "gemm_bits_parent.json")) as _f:
    PARENT = json.load(_f)


@pytest.mark.parametrize("group", gemm_bits.GROUPS)
def test_bits_equal_the_parent_build(group):
    got = gemm_bits.run([group])
    want = {name for name in PARENT if name.startswith(group + "/")}
    assert got and set(got) == want, sorted(want ^ set(got))
    wrong = [name for name, digest in got.items() if PARENT[name] != digest]
    assert not wrong, f"{len(wrong)} of {len(got)} outputs differ from the parent build: {wrong[:8]}"
