"""tools/recommend_bits.py's case list and tests/recommend_bits_parent.json name the same
cases, so a renamed or dropped case cannot pass tests/test_gpu_recommend_bits.py silently.
No GPU: the cases are listed, not run."""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location(
    "recommend_bits", os.path.join(os.path.dirname(HERE), "tools", "recommend_bits.py"))
recommend_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recommend_bits)


def test_every_case_has_a_parent_digest():
    with open(os.path.join(HERE, "recommend_bits_parent.json")) as f:
        parent = json.load(f)
    cases = recommend_bits.cases()
    names = [name for _, name, _ in cases]
    assert len(set(names)) == len(names)
    assert set(names) == set(parent)
    assert all(name.startswith(group + "/") for group, name, _ in cases)
    assert {group for group, _, _ in cases} == {"cos", "mlp", "cos_pop", "mlp_pop"}
    kinds = {"fast", "user_rows", "k_above", "overflow", "few_items"}
    for g in recommend_bits.GROUPS:
        have = {name.split("/")[1] for group, name, _ in cases if group == g}
        assert have == kinds | ({"d102", "d100"} if g.startswith("cos") else set()), g
    assert all(len(d) == 64 and int(d, 16) >= 0 for d in parent.values())
