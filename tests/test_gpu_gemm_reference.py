"""Every GEMM path against the fp64 reference of ops.gemm's contract.

tests/test_gpu_gemm_bits.py pins the bytes of each case of tools/gemm_bits.py to the parent
build; here the same cases, and those of tests/gemm_cases.py that the pinned list does not
reach (the scalar-store epilogue, a second column block, row_epilogue_kernel, the degree modes
in every loader, -inf rows under A2_ZERO_DEG, guard rows past M), are compared with
tests/gemm_reference.py: every tensor a case writes, whole, after every call, to rtol = 1e-4,
atol = 1e-5 inside the written window and bit-exact outside it.  An attention case is compared
call by call with the online form and, at the end, with one softmax over all its relations."""
import pytest
import torch

import gemm_cases
import gemm_reference as ref

pytestmark = pytest.mark.gpu

gemm_bits = gemm_cases.gemm_bits


def _failures(case):
    """What the case got wrong, as strings (empty: all written tensors match)."""
    seen = []

    def keep(j, written):
        torch.cuda.synchronize()
        seen.append([t.cpu() for t in written])

    gemm_bits.run_case(case, after_call=keep)
    steps = ref.reference(case)
    assert len(seen) == len(steps) == len(case.calls)
    bad = []
    for j, (got, want) in enumerate(zip(seen, steps)):
        for t, (what, exp) in zip(got, want.items()):
            err = ref.mismatch(t, exp)
            if err:
                bad.append(f"call {j} {what}: {err}")
    if case.calls[-1].accum == "attn_last":
        for t, (what, exp) in zip(seen[-1], ref.direct_attention(case).items()):
            err = ref.mismatch(t, exp)
            if err:
                bad.append(f"direct softmax {what}: {err}")
    worst = max(ref.error_ratio(t, exp) for got, want in zip(seen, steps)
                for t, exp in zip(got, want.values()))
    return bad, worst


def _run_group(listed, group):
    mine = [(name, describe) for g, name, describe in listed if g == group]
    assert mine
    wrong, ratios = {}, {}
    for name, describe in mine:
        bad, ratios[name] = _failures(describe())
        if bad:
            wrong[name] = bad
    top = max(ratios, key=ratios.get)
    print(f"{group}: {len(mine)} cases, worst error {ratios[top]:.3f} of the tolerance ({top})")
    assert not wrong, (f"{len(wrong)} of {len(mine)} cases differ from the fp64 reference: "
                       + "; ".join(f"{n}: {b[0]}" for n, b in list(wrong.items())[:8]))


@pytest.mark.parametrize("group", gemm_bits.GROUPS)
def test_pinned_cases_match_fp64(group):
    _run_group(gemm_cases.pinned(), group)


@pytest.mark.parametrize("group", gemm_cases.GROUPS_NEW)
def test_new_cases_match_fp64(group):
    _run_group(gemm_cases.new(), group)
