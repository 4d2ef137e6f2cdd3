"""CPU-side checks of the bf16-prefiltered top-k (gnnrec.recs.recommend, csrc/recommend.hip):
the error bound the filter rests on, the algorithm restated in torch (the filtered set
holds the exact top k, and the GPU tests' inputs stay under their candidate cap), and the
Meta kernels' argument checks.  Nothing launches here."""
import numpy as np
import pytest
import torch

import recommend_cases as rc

EPS = rc.EPS


def _unit_bf16(x):
    """Rows normalised in fp32 with the max(norm, 1e-12) guard, rounded to bf16 (nearest even)."""
    x = torch.from_numpy(x)
    n = torch.sqrt((x * x).sum(1, keepdim=True)).clamp_min(1e-12)
    return (x / n).to(torch.bfloat16)


def _approx(hu, hi):
    """a(u, v): bf16 operands, fp32 accumulation."""
    return (_unit_bf16(hu).float() @ _unit_bf16(hi).float().T).numpy()


_cosine64 = rc.cosine64


def test_eps_is_the_documented_constant():
    from gnnrec import recs
    assert recs.REC_EPS == EPS == 2.0 ** -7 + 2.0 ** -11
    assert recs.REC_MAX_D == 2048


@pytest.mark.parametrize("d", [16, 64, 128, 100] + sorted(set(rc.BOUND_DIMS) - {16, 64, 128, 100}))
@pytest.mark.parametrize("kind", ["normal", "relu", "lowrank", "midpoint"])
def test_bound(kind, d):
    """|a - s| <= eps, s the float64 cosine, at every d that
    tests/test_gpu_recommend_kernels.py::test_device_bound runs on the device (the figures of
    both are in profiles/recommend_device_bound.md)."""
    hu, hi = rc.bound_tables(kind, d)
    err = np.abs(_approx(hu, hi) - _cosine64(hu, hi)).max()
    print(f"{kind} d={d} scale=1: max |a - s| = {err:.3e} (eps {EPS:.3e})")
    assert err <= EPS


@pytest.mark.parametrize("d,scale", rc.BOUND_SCALED)
@pytest.mark.parametrize("kind", ["normal", "relu", "lowrank", "midpoint"])
def test_bound_scaled(kind, d, scale):
    """The same with both tables times 2^-20 and 2^20 (exact in fp32, the squares far inside
    the normal range); the reference comes from the scaled tables."""
    hu, hi = rc.bound_tables(kind, d, scale)
    err = np.abs(_approx(hu, hi) - _cosine64(hu, hi)).max()
    print(f"{kind} d={d} scale={scale:g}: max |a - s| = {err:.3e} (eps {EPS:.3e})")
    assert err <= EPS


def _filter_counts(hu, hi, indptr, indices, k, sample):
    """The algorithm in torch: tau = k-th best non-excluded approximate score of the item
    prefix, keep a >= tau - 2 eps.  -> (keep mask with excluded items still in it, counts),
    after checking that the float64 top k of every row is kept."""
    a = _approx(hu, hi)
    s = _cosine64(hu, hi)
    m = min(sample, hi.shape[0])
    keep = np.zeros(a.shape, bool)
    for r in range(a.shape[0]):
        ex = indices[indptr[r]:indptr[r + 1]]
        pre = a[r, :m].copy()
        pre[ex[ex < m]] = -np.inf
        tau = np.sort(pre)[::-1][k - 1] if m >= k else -np.inf
        keep[r] = a[r] >= np.float32(tau) - np.float32(2 * EPS)
        cols = np.setdiff1d(np.arange(a.shape[1]), ex)
        top = cols[np.lexsort((cols, -s[r, cols]))][:k]
        assert keep[r, top].all(), (r, tau)
    return keep, keep.sum(1)


@pytest.mark.parametrize("k", rc.KS)
@pytest.mark.parametrize("d", rc.DIMS)
@pytest.mark.parametrize("kind", rc.KINDS)
def test_filter_keeps_the_top_k_and_fits_the_cap(kind, d, k):
    """The inputs of tests/test_gpu_recommend.py: the exact top k survives the filter and no
    row needs more than the cap those tests run with (they assert that nothing overflows)."""
    hu, hi = rc.tables(kind, d)
    indptr, indices = rc.exclusions()
    _, counts = _filter_counts(hu, hi, indptr, indices, k, rc.SAMPLE)
    print(f"{kind} d={d} k={k}: largest count {counts.max()}, mean {counts.mean():.1f}")
    assert counts.max() <= rc.CAND_CAP


def test_filter_fits_the_cap_wide_rows():
    hu, hi = rc.tables("normal", rc.WIDE_D)
    indptr, indices = rc.exclusions()
    _, counts = _filter_counts(hu, hi, indptr, indices, 10, rc.SAMPLE)
    assert counts.max() <= rc.CAND_CAP


def test_filter_at_200k_items():
    """k = 64, 200k items, a 65536-item prefix: the counts stay in the hundreds."""
    hu, hi = rc.tables("normal", 128, 32, 200_000)
    indptr, indices = rc.exclusions(32, 200_000, 0, 60)
    _, counts = _filter_counts(hu, hi, indptr, indices, 64, 65536)
    print(f"largest count {counts.max()}")
    assert counts.max() <= 1024


# ------------------------------------------- what the device kernel tests lean on
@pytest.mark.parametrize("d", rc.NORMALIZE_DIMS)
def test_normalize_reference_decides_nearly_every_entry(d):
    """rc.normalize_expected: the two admissible bf16 patterns are neighbours or equal, equal
    wherever the quotient is DECIDED away from a rounding midpoint, and equal for more than
    99% of the entries, so the device test pins nearly every output to one value.  (The
    DECIDED entries alone are about 91%: the band of 2 x 2^-12 relative lies in a bf16
    spacing of 2^-8 .. 2^-7 relative.  The bracket of the norm, 2^-20, is what decides.)
    The host restatement itself passes the check it sets for the device."""
    x = rc.normalize_source(d)
    a, b, decided = rc.normalize_expected(x)
    assert (np.abs(a.astype(np.int32) - b.astype(np.int32)) <= 1).all()
    assert (a == b)[decided].all()
    print(f"d={d}: one admissible value for {(a == b).mean():.4%} of the entries, "
          f"{decided.mean():.2%} at least 2^-12 from a midpoint")
    assert (a == b).mean() > 0.99
    got = rc.bf16_bits(rc.unit_bf16(x))
    assert ((got == a) | (got == b)).all()


def test_normalize_reference_midpoint_table():
    hu, _ = rc.tables("midpoint", 100, 37, 1)
    a, b, _ = rc.normalize_expected(hu)
    assert (a == b).mean() > 0.99
    got = rc.bf16_bits(rc.unit_bf16(hu))
    assert ((got == a) | (got == b)).all()


def test_tie_rows_round_to_even():
    """rc.tie_rows: the fp32 norm is 512 exactly, the first quotient an exact midpoint; the
    expected pattern is the even neighbour, which truncation and round-half-up both miss
    for half of the rows."""
    x = rc.tie_rows()
    assert (np.sqrt((x * x).sum(1, dtype=np.float32)) == 512).all()
    q = x[:, 0] / np.float32(512)
    want = rc.bf16_bits(q)
    assert (want & 1 == 0).all()
    lo = q.view(np.uint32) >> 16            # truncation
    assert ((q.view(np.uint32) & 0xFFFF) == 0x8000).all()
    assert (want != lo).sum() == 64 and (want != lo + 1).sum() == 64
    np.testing.assert_array_equal(rc.bf16_bits(rc.unit_bf16(x)), rc.bf16_bits(x / np.float32(512)))


def test_truncating_conversion_breaks_the_bound_and_the_bits():
    """The mutation a device test must catch, tried on the host: bf16 by truncation exceeds
    eps at small d (at d = 16 on the relu and lowrank tables, not on the normal one; from
    d = 128 on it stays under eps everywhere), and misses the admissible patterns of
    normalize_expected at every d."""
    def trunc(x):
        x = np.asarray(x, np.float32)
        ss = (x * x).sum(1, keepdims=True, dtype=np.float32)
        nrm = np.maximum(np.sqrt(ss), np.float32(1e-12))
        return ((x / nrm).view(np.uint32) >> 16).astype(np.uint16)
    hu, hi = rc.bound_tables("lowrank", 16)
    a = rc.bf16_value(trunc(hu)).astype(np.float64) @ rc.bf16_value(trunc(hi)).astype(np.float64).T
    assert np.abs(a - _cosine64(hu, hi)).max() > EPS
    x = rc.normalize_source(32)
    lo, hi_, _ = rc.normalize_expected(x)
    got = trunc(x)
    assert ((got != lo) & (got != hi_)).mean() > 0.25


@pytest.mark.parametrize("d", rc.FILTER_DIMS)
def test_filter_band_is_thin(d):
    """The inputs of test_filter_keeps_exactly_the_expected_set: fewer than 0.1% of a case's
    pairs lie within FILTER_BAND of their row's threshold, where the fp32 accumulation order
    may decide."""
    hu, hi = rc.filter_tables(d)
    a64 = rc.unit_bf16(hu).astype(np.float64) @ rc.unit_bf16(hi).astype(np.float64).T
    for B in rc.FILTER_BS:
        for n in rc.FILTER_NS:
            keep, band = rc.filter_expected(a64[:B, :n], rc.filter_tau(d, B))
            assert band.mean() < rc.FILTER_BAND_SHARE, (B, n, band.sum())
            assert keep[0].all() and (B == 1 or not keep[-1].any())
            assert keep.sum(1).max() <= rc.FILTER_CAP


@pytest.mark.parametrize("name", sorted(rc.FALLBACKS))
def test_fallback_inputs(name):
    """The small cases of test_recommend_other_paths: where the fast path must run without
    overflow (d = 2048), the restated filter keeps every count under the cap."""
    hu, hi, (ip, ix), k, kw, fast = rc.fallback_case(name)
    if fast:
        _, counts = _filter_counts(hu, hi, ip, ix, k, kw.get("sample", rc.SAMPLE))
        assert counts.max() <= rc.CAND_CAP
    else:
        assert hi.shape[0] <= 600 and hu.shape[0] <= 16


# ---------------------------------------------------------------- Meta kernels
def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta")


def _T():
    from gnnrec import _lib
    return _lib.torch_ops()


def test_meta_normalize_rows_bf16():
    T = _T()
    bf = torch.bfloat16
    T.normalize_rows_bf16(_meta(10, 100), None, _meta(10, 128, dtype=bf))
    T.normalize_rows_bf16(_meta(10, 16), _meta(3, dtype=torch.int64), _meta(3, 32, dtype=bf))
    with pytest.raises(ValueError, match="dpad"):
        T.normalize_rows_bf16(_meta(10, 100), None, _meta(10, 100, dtype=bf))
    with pytest.raises(ValueError, match="out must be"):
        T.normalize_rows_bf16(_meta(10, 16), _meta(3, dtype=torch.int64), _meta(10, 32, dtype=bf))
    with pytest.raises(ValueError, match="out must be BFloat16"):
        T.normalize_rows_bf16(_meta(10, 16), None, _meta(10, 32, dtype=torch.float16))
    with pytest.raises(ValueError, match="row_map must be Long"):
        T.normalize_rows_bf16(_meta(10, 16), _meta(3, dtype=torch.int32), _meta(3, 32, dtype=bf))


def test_meta_score_ops():
    T = _T()
    bf, i32 = torch.bfloat16, torch.int32
    u, v = _meta(130, 128, dtype=bf), _meta(5000, 128, dtype=bf)
    T.score_bf16_store(u, v, _meta(130, 5000))
    with pytest.raises(ValueError, match="out must be"):
        T.score_bf16_store(u, v, _meta(130, 4999))
    with pytest.raises(ValueError, match="multiple of 32"):
        T.score_bf16_store(_meta(130, 48, dtype=bf), _meta(5000, 48, dtype=bf), _meta(130, 5000))
    with pytest.raises(ValueError, match="share a dpad"):
        T.score_bf16_store(u, _meta(5000, 64, dtype=bf), _meta(130, 5000))
    with pytest.raises(ValueError, match="users must be BFloat16"):
        T.score_bf16_store(_meta(130, 128), v, _meta(130, 5000))
    tau, cnt, cand = _meta(130), _meta(130, dtype=i32), _meta(130, 1024, dtype=i32)
    T.score_bf16_filter(u, v, tau, cnt, cand)
    with pytest.raises(ValueError, match="tau / counts"):
        T.score_bf16_filter(u, v, _meta(129), cnt, cand)
    with pytest.raises(ValueError, match="cap must be"):
        T.score_bf16_filter(u, v, tau, cnt, _meta(130, 4097, dtype=i32))
    with pytest.raises(ValueError, match="cand_items must be Int"):
        T.score_bf16_filter(u, v, tau, cnt, _meta(130, 1024, dtype=torch.int64))
    with pytest.raises(ValueError, match="counts must be Int"):
        T.score_bf16_filter(u, v, tau, _meta(130, dtype=torch.int64), cand)


def test_meta_candidates_and_mask():
    T = _T()
    i32, i64 = torch.int32, torch.int64
    cnt, cand = _meta(7, dtype=i32), _meta(7, 256, dtype=i32)
    rows = _meta(7, dtype=i64)
    hu, hi = _meta(40, 64), _meta(300, 64)
    ip, ix = _meta(41, dtype=i64), _meta(400, dtype=i32)
    ov, oi = _meta(7, 10), _meta(7, 10, dtype=i64)
    T.topk_candidates_f32(cnt, cand, rows, hu, hi, ip, ix, 10, ov, oi)
    T.topk_candidates_f32(cnt, cand, None, hu, hi, None, None, 10, ov, oi)
    with pytest.raises(ValueError, match="k must be"):
        T.topk_candidates_f32(cnt, cand, rows, hu, hi, ip, ix, 257, _meta(7, 257),
                              _meta(7, 257, dtype=i64))
    with pytest.raises(ValueError, match="multiple of 4"):
        T.topk_candidates_f32(cnt, cand, rows, _meta(40, 63), _meta(300, 63), ip, ix, 10, ov, oi)
    with pytest.raises(ValueError, match="exclude_indptr must be"):
        T.topk_candidates_f32(cnt, cand, rows, hu, hi, _meta(40, dtype=i64), ix, 10, ov, oi)
    with pytest.raises(ValueError, match="exclude_indices must be Int"):
        T.topk_candidates_f32(cnt, cand, rows, hu, hi, ip, _meta(400, dtype=i64), 10, ov, oi)
    with pytest.raises(ValueError, match="out_vals / out_idx"):
        T.topk_candidates_f32(cnt, cand, rows, hu, hi, ip, ix, 10, _meta(7, 9), oi)
    T.mask_excluded_f32(_meta(7, 300), rows, ip, ix)
    with pytest.raises(ValueError, match="user_rows must be"):
        T.mask_excluded_f32(_meta(7, 300), _meta(6, dtype=i64), ip, ix)


def test_cpu_tensors_are_refused():
    T = _T()
    from gnnrec import ops, recs
    with pytest.raises(ValueError, match="HIP device tensor"):
        T.normalize_rows_bf16(torch.zeros(4, 16), None, torch.zeros(4, 32, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="HIP device tensor"):
        T.score_bf16_store(torch.zeros(4, 32, dtype=torch.bfloat16),
                           torch.zeros(4, 32, dtype=torch.bfloat16), torch.zeros(4, 4))
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.normalize_rows_bf16(torch.zeros(4, 16))
    with pytest.raises(ValueError, match="HIP device tensor"):
        recs.recommend(torch.zeros(4, 16), torch.zeros(9, 16), 3)
