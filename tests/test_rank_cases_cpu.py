"""Host checks for the full-ranking evaluation (gnnrec.recs.rank_items / ranks_to_metrics,
DESIGN.md §23): the definition of tests/rank_cases.py against recommend_cases.ranked, the
metrics' restatement on hand-made ranks, the argument checks of the new ops on meta tensors,
and — for the very inputs tests/test_gpu_rank.py uses — the band condition behind its
overflow_rows == 0."""
import functools
import math

import numpy as np
import pytest
import torch

import rank_cases as rk
import recommend_cases as rc


@functools.lru_cache(maxsize=None)
def _case(kind, d):
    hu, hi = rc.tables(kind, d)
    C = rc.cosine64(hu, hi)
    excl = rc.exclusions()
    return C, excl, rk.pairs(C, excl)


def test_eps_is_the_library_value():
    from gnnrec import _lib, recs
    lib = _lib.load()
    for d in (4, 6, 16, 100, 128, 160, 2048):
        assert recs.rank_eps(d) == rk.eps(d) == lib.gnnrec_rank_eps(d)
    assert rk.eps(128) == 544 * 2.0 ** -24 and rk.eps(100) == rk.eps(104)
    assert rk.eps(160) <= 2.0 ** -13          # the width the band condition below was sized for
    assert lib.gnnrec_rank_eps(0) == 0.0


# ---------------------------------------------------------------- the definition
@pytest.mark.parametrize("kind,d", [("normal", 16), ("relu", 16), ("lowrank", 64),
                                    ("midpoint", 128)])
def test_definition_agrees_with_ranked(kind, d):
    """rank(u, g) <= k if and only if ranked's idx[u][rank - 1] == g."""
    C, (ip, ix), (us, gs) = _case(kind, d)
    k = 10
    idx, _ = rc.ranked(C, ip, ix, k)
    r = rk.ranks(C, us, gs, ip, ix)
    for u, g, q in zip(us.tolist(), gs.tolist(), r.tolist()):
        in_list = (idx[u] == g).nonzero()[0]
        if 1 <= q <= k:
            assert idx[u][q - 1] == g
        else:
            assert in_list.size == 0
    # every list entry, without exclusions too
    idx0, _ = rc.ranked(C[:20], None, None, k)
    uu = np.repeat(np.arange(20), k)
    np.testing.assert_array_equal(rk.ranks(C, uu, idx0.reshape(-1)),
                                  np.tile(np.arange(1, k + 1), 20))


def test_pairs_hold_what_the_gpu_tests_need():
    C, (ip, ix), (us, gs) = _case("normal", 16)
    assert us.size == rk.PAIRS_PER_USER * rc.N_USERS
    r = rk.ranks(C, us, gs, ip, ix).reshape(rc.N_USERS, rk.PAIRS_PER_USER)
    assert set(r[:, :5].reshape(-1).tolist()) == set(range(1, 11))       # every position 1..10
    n_ex = np.array([np.unique(ix[ip[u]:ip[u + 1]]).size for u in range(rc.N_USERS)])
    np.testing.assert_array_equal(r[:, 5], rc.N_ITEMS - n_ex)            # the worst-ranked item
    assert ((r[:, 6] == 0) == (n_ex > 0)).all() and (n_ex > 0).sum() > 100  # an excluded item
    np.testing.assert_array_equal(r[:, 7], r[:, 0])                      # a repeated pair


def test_definition_counts_a_duplicated_exclusion_once():
    S = np.array([[0.5, 0.9, 0.9, 0.1, 0.7]])
    ip, ix = rc.csr([[1, 1, 4, 1]])
    np.testing.assert_array_equal(rk.ranks(S, [0, 0, 0, 0, 0], [0, 1, 2, 3, 4], ip, ix),
                                  [2, 0, 1, 3, 0])
    np.testing.assert_array_equal(rk.ranks(S, [0] * 5, [0, 1, 2, 3, 4]), [4, 1, 2, 5, 3])


# ---------------------------------------------------------------- the metrics
def test_metrics_on_hand_made_ranks():
    #        user 0: ranks 1, 3, 3 (a repeated pair), 0 (excluded)   user 1: 12   user 2: 0
    rank = [1, 3, 3, 0, 12, 0]
    users = [0, 0, 0, 0, 1, 2]
    m = rk.metrics(rank, users, (1, 3, 20))
    assert m["unranked"] == 2
    assert m["mrr"] == pytest.approx((1 + 1 / 3 + 1 / 3 + 1 / 12) / 4, rel=1e-15)
    assert m["mean_rank"] == 19 / 4
    assert m["recall@1"] == 1 / 6 and m["recall@3"] == 3 / 6 and m["recall@20"] == 4 / 6
    assert m["hit_rate@1"] == 1 / 3 and m["hit_rate@3"] == 1 / 3 and m["hit_rate@20"] == 2 / 3
    # user 0 has two distinct ranked items {1, 3}; user 1 one; user 2 none (not in the mean)
    d = lambda r: 1.0 / math.log2(1.0 + r)
    assert m["ndcg@1"] == pytest.approx((d(1) / d(1) + 0.0) / 2, rel=1e-15)
    assert m["ndcg@3"] == pytest.approx(((d(1) + d(3)) / (d(1) + d(2)) + 0.0) / 2, rel=1e-15)
    assert m["ndcg@20"] == pytest.approx(((d(1) + d(3)) / (d(1) + d(2)) + d(12) / d(1)) / 2,
                                         rel=1e-15)
    empty = rk.metrics([], [], (10,))
    assert empty["unranked"] == 0 and all(math.isnan(empty[k]) for k in
                                          ("mrr", "mean_rank", "recall@10", "hit_rate@10",
                                           "ndcg@10"))


# ---------------------------------------------------------------- the band condition
@pytest.mark.parametrize("d", rk.DIMS)
@pytest.mark.parametrize("kind", rk.KINDS)
def test_band_stays_under_the_cap(kind, d):
    """No pair of the base cases has CAND_CAP items whose fp64 cosine lies within
    2 (eps(d) + COS_TOL) of its own: the GPU tests assert overflow_rows == 0 on these inputs."""
    C, _, (us, gs) = _case(kind, d)
    worst = int(rk.band_counts(C, us, gs, d).max())
    assert worst < rk.CAND_CAP, worst


# ---------------------------------------------------------------- Meta kernels
def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta")


def _T():
    from gnnrec import _lib
    return _lib.torch_ops()


def test_meta_cos_scores_and_rank_count():
    T = _T()
    i32 = torch.int32
    u, v = _meta(130, 128), _meta(5000, 128)
    T.cos_scores_f32(u, v, _meta(130, 5000))
    with pytest.raises(ValueError, match="out must be"):
        T.cos_scores_f32(u, v, _meta(130, 4999))
    with pytest.raises(ValueError, match="share a dpad"):
        T.cos_scores_f32(u, _meta(5000, 64), _meta(130, 5000))
    thr, parts, ahead = _meta(130), _meta(5, 130, dtype=i32), _meta(130, dtype=i32)
    cnt, band = _meta(130, dtype=i32), _meta(130, 1024, dtype=i32)
    T.rank_count_f32(u, v, thr, parts, ahead, cnt, band)
    with pytest.raises(ValueError, match="parts must hold"):
        T.rank_count_f32(u, v, thr, _meta(4, 130, dtype=i32), ahead, cnt, band)
    with pytest.raises(ValueError, match="parts must be Int"):
        T.rank_count_f32(u, v, thr, _meta(5, 130), ahead, cnt, band)
    with pytest.raises(ValueError, match="thr / ahead / band_counts"):
        T.rank_count_f32(u, v, _meta(129), parts, ahead, cnt, band)
    with pytest.raises(ValueError, match="cap must be"):
        T.rank_count_f32(u, v, thr, parts, ahead, cnt, _meta(130, 4097, dtype=i32))
    with pytest.raises(ValueError, match="band_items must be Int"):
        T.rank_count_f32(u, v, thr, parts, ahead, cnt, _meta(130, 1024, dtype=torch.int64))
    with pytest.raises(ValueError, match="multiple of 8"):
        T.rank_count_f32(_meta(130, 12), _meta(5000, 12), thr, parts, ahead, cnt, band)
    with pytest.raises(ValueError, match="users must be Float"):
        T.rank_count_f32(_meta(130, 128, dtype=torch.bfloat16), v, thr, parts, ahead, cnt, band)


def test_meta_rank_resolve():
    T = _T()
    i32, i64 = torch.int32, torch.int64
    P = 77
    us, gs, thr = _meta(P, dtype=i64), _meta(P, dtype=i64), _meta(P)
    ahead, cnt, band = _meta(P, dtype=i32), _meta(P, dtype=i32), _meta(P, 64, dtype=i32)
    hu, hi, out = _meta(130, 16), _meta(5000, 16), _meta(P, dtype=i64)
    ip, ix = _meta(131, dtype=i64), _meta(900, dtype=i32)
    T.rank_resolve_f32(us, gs, thr, ahead, cnt, band, hu, hi, None, None, out)
    T.rank_resolve_f32(us, gs, thr, ahead, cnt, band, hu, hi, ip, ix, out)
    with pytest.raises(ValueError, match="come together"):
        T.rank_resolve_f32(us, gs, thr, ahead, cnt, band, hu, hi, ip, None, out)
    with pytest.raises(ValueError, match="n_user_rows"):
        T.rank_resolve_f32(us, gs, thr, ahead, cnt, band, hu, hi, _meta(130, dtype=i64), ix, out)
    with pytest.raises(ValueError, match="multiple of 4"):
        T.rank_resolve_f32(us, gs, thr, ahead, cnt, band, _meta(130, 6), _meta(5000, 6), None,
                           None, out)
    with pytest.raises(ValueError, match="rank must be Long"):
        T.rank_resolve_f32(us, gs, thr, ahead, cnt, band, hu, hi, None, None, _meta(P, dtype=i32))
    with pytest.raises(ValueError, match="must be contiguous"):
        T.rank_resolve_f32(us, _meta(P - 1, dtype=i64), thr, ahead, cnt, band, hu, hi, None, None,
                           out)
    with pytest.raises(ValueError, match="users must be Long"):
        T.rank_resolve_f32(_meta(P, dtype=i32), gs, thr, ahead, cnt, band, hu, hi, None, None, out)


def test_cpu_tensors_and_bad_arguments_are_refused_before_any_launch():
    from gnnrec import ops, recs
    T = _T()
    with pytest.raises(ValueError, match="HIP device tensor"):
        T.cos_scores_f32(torch.zeros(4, 16), torch.zeros(9, 16), torch.zeros(4, 9))
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.rank_count(torch.zeros(4, 16), torch.zeros(9, 16), torch.zeros(4),
                       torch.zeros(4, dtype=torch.int32), torch.zeros(4, 8, dtype=torch.int32))
    hu, hi = _meta(4, 16), _meta(9, 16)
    i64 = torch.int64
    with pytest.raises(ValueError, match="HIP device tensor"):
        recs.rank_items(hu, hi, torch.zeros(3, dtype=i64), _meta(3, dtype=i64))
    with pytest.raises(ValueError, match="users must be"):
        recs.rank_items(hu, hi, _meta(3, dtype=torch.int32), _meta(3, dtype=i64))
    with pytest.raises(ValueError, match="3 users for 2 items"):
        recs.rank_items(hu, hi, _meta(3, dtype=i64), _meta(2, dtype=i64))
    with pytest.raises(ValueError, match="cand_cap"):
        recs.rank_items(hu, hi, _meta(3, dtype=i64), _meta(3, dtype=i64), cand_cap=4097)
    with pytest.raises(ValueError, match="batch_size"):
        recs.rank_items(hu, hi, _meta(3, dtype=i64), _meta(3, dtype=i64), batch_size=0)
    with pytest.raises(ValueError, match="one feature size"):
        recs.rank_items(hu, _meta(9, 32), _meta(3, dtype=i64), _meta(3, dtype=i64))
    with pytest.raises(ValueError, match="n_users \\+ 1"):
        recs.rank_items(hu, hi, _meta(3, dtype=i64), _meta(3, dtype=i64),
                        (_meta(4, dtype=i64), _meta(7, dtype=torch.int32)))
    with pytest.raises(ValueError, match="exclude indices"):
        recs.rank_items(hu, hi, _meta(3, dtype=i64), _meta(3, dtype=i64),
                        (_meta(5, dtype=i64), _meta(7, dtype=i64)))
    with pytest.raises(ValueError, match="rank must be"):
        recs.ranks_to_metrics(_meta(3, dtype=torch.int32), _meta(3, dtype=i64))
    with pytest.raises(ValueError, match="HIP device tensor"):
        recs.ranks_to_metrics(torch.zeros(3, dtype=i64), torch.zeros(3, dtype=i64))
