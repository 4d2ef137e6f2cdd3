"""Host checks for the popularity-weighted many-user top-k (gnnrec.recs.recommend with
popularity=): the argument checks of every new op on meta tensors, and — for
the very inputs tests/test_gpu_recommend_pop.py uses — the band, the candidate counts, the
overflow case and the gaps its comparisons lean on."""
import functools

import numpy as np
import pytest
import torch

import recommend_cases as rc
import recommend_mlp_cases as mc
import recommend_pop_cases as pc


def test_band_is_the_library_constant():
    from gnnrec import recs
    assert recs.REC_RATING_BAND == pc.RATING_BAND and recs.REC_RATING_SLACK == pc.RATING_SLACK
    eps = recs.REC_EPS
    assert pc.RATING_BAND == np.exp(1 + eps) * (np.expm1(eps) + 2.0 ** -20)


# ---------------------------------------------------------------- the band and the counts
@functools.lru_cache(maxsize=None)
def _cos(kind, d):
    hu, hi = rc.tables(kind, d)
    return pc.approx_and_score(hu, hi)


@functools.lru_cache(maxsize=None)
def _mlp(kind, d):
    hu, hi = rc.tables(kind, d)
    return mc.host_scores(mc.head(d), hu, hi)


@pytest.mark.parametrize("d", [16, 64, 128] + sorted(set(rc.BOUND_DIMS) - {16, 64, 128}))
@pytest.mark.parametrize("kind", ["normal", "relu", "lowrank", "midpoint"])
def test_rating_band(kind, d):
    """|Ra - R| <= delta_u in fp64 for the bound tables, each of the four popularities."""
    hu, hi = rc.bound_tables(kind, d)
    a, S = pc.approx_and_score(hu, hi)
    assert np.abs(a - S).max() <= rc.EPS
    for name in pc.POPS:
        pop, w = pc.popularity(name, hi.shape[0])
        p = pc.p_vector(pop, w)
        R, Z = pc.ratings64(S, p)
        Ra = np.exp(a) / Z[:, None] + p.astype(np.float64)
        delta = pc.RATING_BAND / Z + pc.RATING_SLACK * float(p.max())
        assert (np.abs(Ra - R) <= delta[:, None]).all(), (name, np.abs(Ra - R).max(), delta.min())


@pytest.mark.parametrize("name", pc.POPS)
@pytest.mark.parametrize("d", rc.DIMS)
@pytest.mark.parametrize("kind", rc.KINDS)
def test_candidate_counts_stay_far_under_the_cap(kind, d, name):
    """The cosine head: for every k the GPU file uses no row keeps more than CAND_CAP / 2
    items, with and without exclusions, and the exact top k is always inside the kept set."""
    a, S = _cos(kind, d)
    pop, w = pc.popularity(name)
    p = pc.p_vector(pop, w)
    R, Z = pc.ratings64(S, p)
    Ra = np.exp(a) / Z[:, None] + p.astype(np.float64)
    for excl in (rc.exclusions(), (None, None)):
        for k in rc.KS:
            counts, inside = pc.filter_counts(Ra, R, Z, p, excl[0], excl[1], k, pc.SAMPLE,
                                              pc.POP_SAMPLE, True)
            print(kind, d, name, k, counts.max())
            assert inside and counts.max() <= pc.CAND_CAP // 2 and counts.min() >= k


@pytest.mark.parametrize("name", pc.POPS)
@pytest.mark.parametrize("d", mc.DIMS)
@pytest.mark.parametrize("kind", mc.KINDS)
def test_candidate_counts_stay_far_under_the_cap_mlp(kind, d, name):
    S = _mlp(kind, d)
    pop, w = pc.popularity(name)
    p = pc.p_vector(pop, w)
    R, Z = pc.ratings64(S, p)
    for excl in (rc.exclusions(), (None, None)):
        for k in mc.KS:
            counts, inside = pc.filter_counts(R, R, Z, p, excl[0], excl[1], k, pc.SAMPLE,
                                              pc.POP_SAMPLE, False)
            print(kind, d, name, k, counts.max())
            assert inside and counts.max() <= pc.CAND_CAP // 2 and counts.min() >= k


def test_overflow_case_overflows_without_the_popular_sample():
    o = pc.OVERFLOW
    a, S = _cos(o["kind"], o["d"])
    pop, w = pc.block_popularity()
    p = pc.p_vector(pop, w)
    R, Z = pc.ratings64(S, p)
    Ra = np.exp(a) / Z[:, None] + p.astype(np.float64)
    ip, ix = rc.exclusions()
    without, inside0 = pc.filter_counts(Ra, R, Z, p, ip, ix, o["k"], o["sample"], 0, True)
    with_, inside1 = pc.filter_counts(Ra, R, Z, p, ip, ix, o["k"], o["sample"], pc.POP_SAMPLE,
                                      True)
    print(without.min(), without.max(), with_.max())
    # far from the cap on both sides: fp32 rounding on the device cannot move a row across
    assert without.min() > 2 * o["cand_cap"] and inside0
    assert with_.max() < o["cand_cap"] // 2 and inside1


def test_dominant_k_is_decided_by_popularity():
    """The gap between the k-th and (k + 1)-th largest p exceeds every softmax term, so the k
    most popular items are every user's list, as a set."""
    pop, w = pc.popularity("dominant")
    p = np.sort(pc.p_vector(pop, w).astype(np.float64))[::-1]
    _, S = _cos("normal", pc.EDGE_D)
    soft, _ = pc.ratings64(S, np.zeros(rc.N_ITEMS, np.float32))
    assert p[pc.DOMINANT_K - 1] - p[pc.DOMINANT_K] > 1.05 * soft.max()


def test_mlp_reference_case_has_no_near_ties():
    hu, hi, pop, (ip, ix) = pc.mlp_ref_case()
    s = pc.MLP_REF
    S = mc.host_scores(mc.head(s["d"]), hu, hi)
    R, _ = pc.ratings64(S, pc.p_vector(pop, s["weight"]))
    _, vals = rc.ranked(R, ip, ix, s["k"] + 1)
    assert np.isfinite(vals).all()
    gaps = (vals[:, :-1] - vals[:, 1:]) / np.abs(vals[:, :-1])
    print(gaps.min())
    assert gaps.min() > pc.MLP_REF_GAP


def test_sample_columns():
    p = np.array([0, 5, 1, 7, 7, 0, 3, 9], np.float32)
    np.testing.assert_array_equal(pc.sample_columns(p, 2, 3), [0, 1, 3, 4, 7])
    np.testing.assert_array_equal(pc.sample_columns(p, 2, 0), [0, 1])
    np.testing.assert_array_equal(pc.sample_columns(p, 100, 3), np.arange(8))
    np.testing.assert_array_equal(pc.sample_columns(p, 6, 100), np.arange(8))


# ---------------------------------------------------------------- Meta kernels
def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta")


def _T():
    from gnnrec import _lib
    return _lib.torch_ops()


def test_meta_normalize_and_denominators():
    T = _T()
    T.normalize_rows_f32(_meta(10, 100), None, _meta(10, 104))
    T.normalize_rows_f32(_meta(10, 16), _meta(3, dtype=torch.int64), _meta(3, 16))
    with pytest.raises(ValueError, match="multiple of 4"):
        T.normalize_rows_f32(_meta(10, 102), None, _meta(10, 104))
    with pytest.raises(ValueError, match="multiple of 4"):
        T.normalize_rows_f32(_meta(10, 2052), None, _meta(10, 2056))
    with pytest.raises(ValueError, match="out must be"):
        T.normalize_rows_f32(_meta(10, 100), None, _meta(10, 100))
    with pytest.raises(ValueError, match="out must be Float"):
        T.normalize_rows_f32(_meta(10, 16), None, _meta(10, 16, dtype=torch.bfloat16))
    u, v = _meta(130, 128), _meta(5000, 128)
    T.cos_denominators_f32(u, v, _meta(5, 130), _meta(130))
    with pytest.raises(ValueError, match="parts must hold"):
        T.cos_denominators_f32(u, v, _meta(4, 130), _meta(130))
    with pytest.raises(ValueError, match="Z must be"):
        T.cos_denominators_f32(u, v, _meta(5, 130), _meta(129))
    with pytest.raises(ValueError, match="share a dpad"):
        T.cos_denominators_f32(u, _meta(5000, 64), _meta(5, 130), _meta(130))
    with pytest.raises(ValueError, match="multiple of 8"):
        T.cos_denominators_f32(_meta(130, 12), _meta(5000, 12), _meta(5, 130), _meta(130))
    with pytest.raises(ValueError, match="users must be Float"):
        T.cos_denominators_f32(_meta(130, 128, dtype=torch.bfloat16), v, _meta(5, 130), _meta(130))


def test_meta_rating_rows_and_thresholds():
    T = _T()
    i32, i64 = torch.int32, torch.int64
    T.exp_rowsum_f32(_meta(7, 300), _meta(7))
    with pytest.raises(ValueError, match="Z must be"):
        T.exp_rowsum_f32(_meta(7, 300), _meta(8))
    T.rating_rows_f32(_meta(7, 300), _meta(7), _meta(300))
    with pytest.raises(ValueError, match="p must be"):
        T.rating_rows_f32(_meta(7, 300), _meta(7), _meta(299))
    with pytest.raises(ValueError, match="Z must be"):
        T.rating_rows_f32(_meta(7, 300), _meta(6), _meta(300))
    T.rating_thresholds_f32(_meta(7), _meta(7), _meta(1), _meta(7))
    with pytest.raises(ValueError, match="pmax must be"):
        T.rating_thresholds_f32(_meta(7), _meta(7), _meta(2), _meta(7))
    with pytest.raises(ValueError, match="thr must be"):
        T.rating_thresholds_f32(_meta(7), _meta(7), _meta(1), _meta(6))
    rows, ip, ix = _meta(7, dtype=i64), _meta(41, dtype=i64), _meta(400, dtype=i32)
    T.mask_excluded_mapped_f32(_meta(7, 300), _meta(300, dtype=i32), rows, ip, ix)
    with pytest.raises(ValueError, match="col_ids must be contiguous"):
        T.mask_excluded_mapped_f32(_meta(7, 300), _meta(299, dtype=i32), rows, ip, ix)
    with pytest.raises(ValueError, match="col_ids must be Int"):
        T.mask_excluded_mapped_f32(_meta(7, 300), _meta(300, dtype=i64), rows, ip, ix)
    with pytest.raises(ValueError, match="user_rows must be"):
        T.mask_excluded_mapped_f32(_meta(7, 300), _meta(300, dtype=i32), _meta(6, dtype=i64), ip,
                                   ix)


def test_meta_rating_scorers():
    T = _T()
    bf, i32, i64 = torch.bfloat16, torch.int32, torch.int64
    u, v = _meta(130, 128, dtype=bf), _meta(5000, 128, dtype=bf)
    Z, p = _meta(130), _meta(5000)
    T.score_bf16_store_rating(u, v, Z, p, _meta(130, 5000))
    with pytest.raises(ValueError, match="out must be"):
        T.score_bf16_store_rating(u, v, Z, p, _meta(130, 4999))
    with pytest.raises(ValueError, match="p_col must be"):
        T.score_bf16_store_rating(u, v, Z, _meta(4999), _meta(130, 5000))
    with pytest.raises(ValueError, match="Z must be"):
        T.score_bf16_store_rating(u, v, _meta(131), p, _meta(130, 5000))
    thr, cnt, cand = _meta(130), _meta(130, dtype=i32), _meta(130, 1024, dtype=i32)
    T.score_bf16_filter_rating(u, v, Z, p, thr, cnt, cand)
    with pytest.raises(ValueError, match="thr must be"):
        T.score_bf16_filter_rating(u, v, Z, p, _meta(129), cnt, cand)
    with pytest.raises(ValueError, match="cap must be"):
        T.score_bf16_filter_rating(u, v, Z, p, thr, cnt, _meta(130, 4097, dtype=i32))
    with pytest.raises(ValueError, match="counts must be Int"):
        T.score_bf16_filter_rating(u, v, Z, p, thr, _meta(130, dtype=i64), cand)
    cnt, cand = _meta(7, dtype=i32), _meta(7, 256, dtype=i32)
    rows = _meta(7, dtype=i64)
    hu, hi = _meta(40, 64), _meta(300, 64)
    ip, ix = _meta(41, dtype=i64), _meta(400, dtype=i32)
    ov, oi = _meta(7, 10), _meta(7, 10, dtype=i64)
    T.topk_candidates_rating_f32(cnt, cand, rows, hu, hi, ip, ix, _meta(7), _meta(300), 10, ov, oi)
    T.topk_candidates_rating_f32(cnt, cand, None, hu, hi, None, None, _meta(7), _meta(300), 10,
                                 ov, oi)
    with pytest.raises(ValueError, match="Z must be"):
        T.topk_candidates_rating_f32(cnt, cand, rows, hu, hi, ip, ix, _meta(8), _meta(300), 10,
                                     ov, oi)
    with pytest.raises(ValueError, match="p must be"):
        T.topk_candidates_rating_f32(cnt, cand, rows, hu, hi, ip, ix, _meta(7), _meta(40), 10,
                                     ov, oi)
    with pytest.raises(ValueError, match="k must be"):
        T.topk_candidates_rating_f32(cnt, cand, rows, hu, hi, ip, ix, _meta(7), _meta(300), 257,
                                     _meta(7, 257), _meta(7, 257, dtype=i64))


def test_meta_dense_mlp_rating_ops():
    T = _T()
    i32 = torch.int32
    P, Q = _meta(130, 128), _meta(5000, 128)
    tail = (_meta(32, 128), _meta(32), _meta(32), _meta(1))
    Z, p = _meta(130), _meta(5000)
    assert T.cos_denominator_parts(5000) == 5 and T.cos_denominator_parts(1024) == 1
    assert T.cos_denominator_parts(0) == 0 and T.cos_denominator_parts(1025) == pc.parts(1025)
    T.edge_mlp_dense_denominators_f32(P, Q, *tail, _meta(5, 130))
    with pytest.raises(ValueError, match="parts must be"):
        T.edge_mlp_dense_denominators_f32(P, Q, *tail, _meta(4, 130))
    with pytest.raises(ValueError, match="hidden sizes"):
        T.edge_mlp_dense_denominators_f32(_meta(130, 64), Q, *tail, _meta(5, 130))
    T.fold_partials_f32(_meta(5, 130), Z)
    with pytest.raises(ValueError, match="Z must be"):
        T.fold_partials_f32(_meta(5, 129), Z)
    with pytest.raises(ValueError, match="parts must be"):
        T.fold_partials_f32(_meta(650), Z)
    T.edge_mlp_dense_store_rating_f32(P, Q, *tail, Z, p, _meta(130, 5000))
    with pytest.raises(ValueError, match="p_col must be"):
        T.edge_mlp_dense_store_rating_f32(P, Q, *tail, Z, _meta(130), _meta(130, 5000))
    with pytest.raises(ValueError, match="out must be"):
        T.edge_mlp_dense_store_rating_f32(P, Q, *tail, Z, p, _meta(130, 4999))
    cnt, cand, csc = _meta(130, dtype=i32), _meta(130, 64, dtype=i32), _meta(130, 64)
    T.edge_mlp_dense_filter_rating_f32(P, Q, *tail, Z, p, _meta(130), cnt, cand, csc)
    with pytest.raises(ValueError, match="tau must be"):
        T.edge_mlp_dense_filter_rating_f32(P, Q, *tail, Z, p, _meta(129), cnt, cand, csc)
    with pytest.raises(ValueError, match="cand_scores must be"):
        T.edge_mlp_dense_filter_rating_f32(P, Q, *tail, Z, p, _meta(130), cnt, cand, _meta(130, 63))
    with pytest.raises(ValueError, match="cap must be"):
        T.edge_mlp_dense_filter_rating_f32(P, Q, *tail, Z, p, _meta(130), cnt,
                                       _meta(130, 4097, dtype=i32), _meta(130, 4097))


def test_cpu_tensors_are_refused():
    T = _T()
    from gnnrec import ops
    with pytest.raises(ValueError, match="HIP device tensor"):
        T.normalize_rows_f32(torch.zeros(4, 16), None, torch.zeros(4, 16))
    with pytest.raises(ValueError, match="HIP device tensor"):
        T.cos_denominators_f32(torch.zeros(4, 16), torch.zeros(9, 16), torch.zeros(1, 4),
                           torch.zeros(4))
    with pytest.raises(ValueError, match="HIP device tensor"):
        T.rating_rows_f32(torch.zeros(4, 9), torch.zeros(4), torch.zeros(9))
    with pytest.raises(ValueError, match="HIP device tensor"):
        T.exp_rowsum_f32(torch.zeros(4, 9), torch.zeros(4))
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.normalize_rows_f32(torch.zeros(4, 16))
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.rating_thresholds(torch.zeros(4), torch.zeros(4), torch.zeros(1))
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.edge_mlp_dense_denominators(torch.zeros(4, 128), torch.zeros(9, 128),
                                        torch.zeros(32, 128), torch.zeros(32), torch.zeros(32),
                                        torch.zeros(1))


def test_popularity_is_checked_before_any_launch():
    """Meta tables pass recommend's own checks and launch nothing: a popularity of the wrong
    length, shape, dtype or device is refused first."""
    from gnnrec import recs
    hu, hi = _meta(4, 16), _meta(9, 16)
    for bad in (_meta(8), _meta(9, 2), _meta(3, 3), _meta(9, dtype=torch.float64),
                _meta(9, dtype=torch.int64)):
        with pytest.raises(ValueError, match="popularity"):
            recs.recommend(hu, hi, 3, popularity=bad)
    with pytest.raises(ValueError, match="popularity"):
        recs.recommend(hu, hi, 3, popularity=torch.zeros(9))            # a CPU tensor
    with pytest.raises(ValueError, match="popularity"):
        recs.recommend(hu, hi, 3, popularity=np.zeros(9, np.float32))   # not a tensor
    with pytest.raises(ValueError, match="pop_sample"):
        recs.recommend(hu, hi, 3, popularity=_meta(9), pop_sample=-1)
