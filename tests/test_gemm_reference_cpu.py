"""The answer key of tests/test_gpu_gemm_reference.py, checked without a GPU: every pinned
and new GEMM case yields a description and an fp64 reference; the online and the direct
attention forms agree; the reference agrees with a plain torch fp32 evaluation; and no l2norm
case sits on the discontinuity of the guarded division."""
import functools

import torch
import torch.nn.functional as F

import gemm_cases
import gemm_reference as ref


@functools.lru_cache(None)
def _all():
    return [(name, describe()) for _, name, describe in gemm_cases.pinned() + gemm_cases.new()]


def test_every_case_has_a_description_and_a_reference():
    pinned, new = gemm_cases.pinned(), gemm_cases.new()
    assert [(g, n) for g, n, _ in pinned] == [(g, n) for g, n, _ in gemm_cases.gemm_bits.cases()]
    assert len(pinned) == 252 and 0 < len(new) <= 200
    names = [n for _, n, _ in pinned + new]
    assert len(set(names)) == len(names)
    assert {g for g, _, _ in new} == set(gemm_cases.GROUPS_NEW)
    assert all(n.startswith(g + "/") for g, n, _ in new)
    for name, case in _all():
        steps = ref.reference(case)
        assert len(steps) == len(case.calls) >= 1, name
        for step in steps:
            assert tuple(step) == case.writes, name
            for exp in step.values():
                assert exp.value.dtype == torch.float64 and exp.value.shape == exp.init.shape
                assert bool(torch.isfinite(exp.value[exp.touched]).all()), name
                assert torch.equal(exp.value[~exp.touched], exp.init[~exp.touched].double()), name


def test_new_cases_have_guards_and_mixed_degrees():
    for _, name, describe in gemm_cases.new():
        case = describe()
        assert case.guard == 1 and case.out_init.shape == (case.m + 1, case.col + case.n + case.pad)
        assert bool((case.out_init[case.m] == gemm_cases.SENTINEL).all()), name
        for t in (case.row_norm_init, case.attn_state_init):
            assert t is None or (t.shape[0] == case.m + 1
                                 and bool((t == gemm_cases.SENTINEL).all())), name
        assert case.m <= 300 and case.n <= 384, name
        for c in case.calls:
            assert c.k1 <= 128 and (c.a2 is None or c.a2.shape[1] <= 128), name
            if c.a2_deg is not None:
                assert bool((c.a2_deg == 0).any()) and bool((c.a2_deg > 0).any()), name
    neginf = [d() for g, _, d in gemm_cases.new() if g == "neginf"]
    assert len(neginf) == 3
    for case in neginf:
        (c,) = case.calls
        assert c.a2_mode == "zero" and bool(torch.isinf(c.a2[c.a2_deg == 0]).all())
        assert bool(torch.isfinite(c.a2[c.a2_deg > 0]).all())


def test_online_and_direct_attention_agree():
    n = 0
    for name, case in _all():
        if case.calls[-1].accum != "attn_last":
            continue
        n += 1
        online, direct = ref.reference(case)[-1], ref.direct_attention(case)
        for what in case.writes:
            assert torch.allclose(online[what].value, direct[what].value, rtol=1e-12, atol=1e-12), \
                (name, what, float((online[what].value - direct[what].value).abs().max()))
    assert n >= 40


def _plain_fp32(c):
    """One store call with torch's own fp32 operators."""
    x = F.linear(c.a1, c.w1)
    if c.a2 is not None:
        a2 = c.a2
        if c.a2_mode == "div":
            a2 = a2 / c.a2_deg.clamp(min=1).float().unsqueeze(1)
        elif c.a2_mode == "zero":
            a2 = a2.masked_fill((c.a2_deg == 0).unsqueeze(1), 0.0)
        x = x + F.linear(a2, c.w2)
    if c.bias is not None:
        x = x + c.bias
    if c.bias_nonempty is not None:
        x = torch.where((c.a2_deg > 0).unsqueeze(1), x + c.bias_nonempty, x)
    if c.relu:
        x = F.relu(x)
    if c.sigmoid:
        x = torch.sigmoid(x)
    norm = torch.linalg.vector_norm(x, dim=1)
    return (F.normalize(x, dim=1) if c.l2norm else x), norm


def test_reference_agrees_with_plain_torch_fp32_on_store_cases():
    n = 0
    for name, case in _all():
        if len(case.calls) != 1 or case.calls[0].accum != "store":
            continue
        n += 1
        (c,) = case.calls
        z, norm = _plain_fp32(c)
        if c.out_div > 0:
            z = z / c.out_div
        want = ref.reference(case)[0]
        got = case.out_init.clone()
        got[:case.m, case.col:case.col + case.n] = z
        assert ref.mismatch(got, want["out"]) is None, (name, ref.mismatch(got, want["out"]))
        if "row_norm" in want:
            rn = case.row_norm_init.clone()
            rn[:case.m] = norm
            assert ref.mismatch(rn, want["row_norm"]) is None, name
    assert n >= 150


def test_l2norm_cases_are_well_conditioned():
    """The guarded division x / (|x| or 1) jumps at |x| = 0, so a row whose norm is a
    rounding error away from zero would compare noise: no reference row may have a norm in
    (0, 1e-3) before the normalisation.  Every pinned and new case satisfies it, so no row is
    exempt from the comparison."""
    checked = 0
    for name, case in _all():
        for c in case.calls:
            if not c.l2norm:
                continue
            checked += 1
            norm = ref.activations(c)[1]
            ill = int(((norm > 0) & (norm < 1e-3)).sum())
            assert ill == 0, (name, ill, float(norm[norm > 0].min()))
    assert checked >= 150


def test_mismatch_reports_each_kind_of_difference():
    init = torch.full((3, 4), gemm_cases.SENTINEL)
    touched = torch.zeros(3, 4, dtype=torch.bool)
    touched[:2, :3] = True
    value = init.double()
    value[:2, :3] = torch.arange(6.0, dtype=torch.float64).reshape(2, 3)
    exp = ref.Expected(value, touched, init)
    good = value.float()
    assert ref.mismatch(good, exp) is None
    assert ref.mismatch(good + touched * 1e-6, exp) is None           # inside atol
    for r, c, v, what in ((1, 2, 5.01, "outside rtol"), (0, 0, float("nan"), "non-finite"),
                          (2, 0, 0.0, "window changed"), (0, 3, 0.0, "window changed")):
        got = good.clone()
        got[r, c] = v
        assert what in ref.mismatch(got, exp), what
    nan_ref = ref.Expected(value.clone(), touched, init)
    nan_ref.value[0, 0] = float("nan")
    assert "outside rtol" in ref.mismatch(good, nan_ref)
