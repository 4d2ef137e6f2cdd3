"""tools/fused_bits.py's case list and tests/fused_bits_parent.json name the same cases, so a
renamed or dropped case cannot pass tests/test_gpu_fused_bits.py silently.  No GPU: the
cases are listed, not run."""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "fused_bits", os.path.join(os.path.dirname(HERE), "tools", "fused_bits.py"))
fused_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fused_bits)


def test_every_case_has_a_parent_digest():
    with open(os.path.join(HERE, "fused_bits_parent.json")) as f:
        parent = json.load(f)
    cases = fused_bits.cases()
    names = [name for _, name, _ in cases]
    assert len(set(names)) == len(names)
    assert set(names) == set(parent)
    assert all(name.startswith(group + "/") for group, name, _ in cases)
    assert sorted({group for group, _, _ in cases}) == ["pair", "pre", "project2", "queued",
                                                        "ragged", "single"]
    assert all(len(d) == 64 and int(d, 16) >= 0 for d in parent.values())
