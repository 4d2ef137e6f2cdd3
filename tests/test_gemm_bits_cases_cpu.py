"""tools/gemm_bits.py's case list and tests/gemm_bits_parent.json name the same cases, so a
renamed or dropped case cannot pass tests/test_gpu_gemm_bits.py silently.  No GPU: the cases
are listed, not run."""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "gemm_bits", os.path.join(os.path.dirname(HERE), "tools", "gemm_bits.py"))
gemm_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gemm_bits)


def test_every_case_has_a_parent_digest():
    with open(os.path.join(HERE, "gemm_bits_parent.json")) as f:
        parent = json.load(f)
    cases = gemm_bits.cases()
    names = [name for _, name, _ in cases]
    assert len(set(names)) == len(names)
    assert set(names) == set(parent)
    assert all(name.startswith(group + "/") for group, name, _ in cases)
    assert sorted({group for group, _, _ in cases}) == sorted(gemm_bits.GROUPS) == [
        "d16_bn128", "d16_bn64", "d32_bn256", "d32_bn32", "general"]
    assert all(len(d) == 64 and int(d, 16) >= 0 for d in parent.values())
