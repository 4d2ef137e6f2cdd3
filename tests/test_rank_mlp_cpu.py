"""Host checks for the full-ranking evaluation of the MLP head (gnnrec.recs.rank_items(head=),
DESIGN.md §24): the argument checks of the new ops on meta tensors, the refusals that come
before any launch, and — for the very inputs tests/test_gpu_rank_mlp.py uses — the exact ties
its tie-rule and rating cases lean on."""
import functools

import numpy as np
import pytest
import torch

import rank_cases as rk
import rank_mlp_cases as rm
import recommend_cases as rc
import recommend_mlp_cases as mc


def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta")


def _T():
    from gnnrec import _lib
    return _lib.torch_ops()


def _tail():
    return _meta(32, 128), _meta(32), _meta(32), _meta(1)


# ---------------------------------------------------------------- Meta kernels
def test_meta_dense_count():
    T = _T()
    i32 = torch.int32
    P, Q, tail = _meta(130, 128), _meta(5000, 128), _tail()
    thr, gid = _meta(130), _meta(130, dtype=i32)
    parts, ahead = _meta(5, 130, dtype=i32), _meta(130, dtype=i32)
    T.edge_mlp_dense_count_f32(P, Q, *tail, thr, gid, parts, ahead)
    T.edge_mlp_dense_count_f32(_meta(0, 128), Q, *tail, _meta(0), _meta(0, dtype=i32),
                               _meta(5, 0, dtype=i32), _meta(0, dtype=i32))
    T.edge_mlp_dense_count_f32(P, _meta(0, 128), *tail, thr, gid, _meta(0, 130, dtype=i32), ahead)
    with pytest.raises(ValueError, match="parts must be a contiguous \\[5, 130\\]"):
        T.edge_mlp_dense_count_f32(P, Q, *tail, thr, gid, _meta(4, 130, dtype=i32), ahead)
    with pytest.raises(ValueError, match="parts must be a contiguous"):
        T.edge_mlp_dense_count_f32(P, Q, *tail, thr, gid, _meta(5, 129, dtype=i32), ahead)
    with pytest.raises(ValueError, match="parts must be a contiguous"):
        T.edge_mlp_dense_count_f32(P, Q, *tail, thr, gid, _meta(650, dtype=i32), ahead)
    with pytest.raises(ValueError, match="parts must be Int"):
        T.edge_mlp_dense_count_f32(P, Q, *tail, thr, gid, _meta(5, 130), ahead)
    with pytest.raises(ValueError, match="ahead must be Int"):
        T.edge_mlp_dense_count_f32(P, Q, *tail, thr, gid, parts, _meta(130, dtype=torch.int64))
    with pytest.raises(ValueError, match="gid must be Int"):
        T.edge_mlp_dense_count_f32(P, Q, *tail, thr, _meta(130, dtype=torch.int64), parts, ahead)
    with pytest.raises(ValueError, match="thr must be Float"):
        T.edge_mlp_dense_count_f32(P, Q, *tail, _meta(130, dtype=torch.float64), gid, parts, ahead)
    with pytest.raises(ValueError, match="thr must be contiguous \\[130\\]"):
        T.edge_mlp_dense_count_f32(P, Q, *tail, _meta(129), gid, parts, ahead)
    with pytest.raises(ValueError, match="gid / ahead"):
        T.edge_mlp_dense_count_f32(P, Q, *tail, thr, _meta(131, dtype=i32), parts, ahead)
    with pytest.raises(ValueError, match="gid / ahead"):
        T.edge_mlp_dense_count_f32(P, Q, *tail, thr, gid, parts, _meta(129, dtype=i32))
    with pytest.raises(ValueError, match="128/32 hidden sizes"):
        T.edge_mlp_dense_count_f32(_meta(130, 64), Q, *tail, thr, gid, parts, ahead)
    with pytest.raises(ValueError, match="128/32 hidden sizes"):
        T.edge_mlp_dense_count_f32(P, Q, _meta(32, 64), *tail[1:], thr, gid, parts, ahead)


def test_meta_dense_count_rating():
    T = _T()
    i32 = torch.int32
    P, Q, tail = _meta(130, 128), _meta(5000, 128), _tail()
    Z, p, s, gid = _meta(130), _meta(5000), _meta(130), _meta(130, dtype=i32)
    parts, ahead = _meta(5, 130, dtype=i32), _meta(130, dtype=i32)
    T.edge_mlp_dense_count_rating_f32(P, Q, *tail, Z, p, s, gid, parts, ahead)
    with pytest.raises(ValueError, match="Z must be contiguous \\[130\\]"):
        T.edge_mlp_dense_count_rating_f32(P, Q, *tail, _meta(129), p, s, gid, parts, ahead)
    with pytest.raises(ValueError, match="p_col must be contiguous \\[5000\\]"):
        T.edge_mlp_dense_count_rating_f32(P, Q, *tail, Z, _meta(4999), s, gid, parts, ahead)
    with pytest.raises(ValueError, match="p_col must be Float"):
        T.edge_mlp_dense_count_rating_f32(P, Q, *tail, Z, _meta(5000, dtype=torch.float64), s, gid,
                                          parts, ahead)
    with pytest.raises(ValueError, match="thr must be contiguous"):
        T.edge_mlp_dense_count_rating_f32(P, Q, *tail, Z, p, _meta(131), gid, parts, ahead)
    with pytest.raises(ValueError, match="parts must be a contiguous \\[5, 130\\]"):
        T.edge_mlp_dense_count_rating_f32(P, Q, *tail, Z, p, s, gid, _meta(6, 130, dtype=i32),
                                          ahead)
    with pytest.raises(ValueError, match="gid must be Int"):
        T.edge_mlp_dense_count_rating_f32(P, Q, *tail, Z, p, s, _meta(130), parts, ahead)
    with pytest.raises(ValueError, match="128/32 hidden sizes"):
        T.edge_mlp_dense_count_rating_f32(P, _meta(5000, 64), *tail, Z, p, s, gid, parts, ahead)


def test_meta_rank_resolve_mlp():
    T = _T()
    i32, i64 = torch.int32, torch.int64
    n = 77
    us, gs, s, ahead = _meta(n, dtype=i64), _meta(n, dtype=i64), _meta(n), _meta(n, dtype=i32)
    P, Q, tail = _meta(n, 128), _meta(5000, 128), _tail()
    ip, ix = _meta(131, dtype=i64), _meta(900, dtype=i32)
    Z, p = _meta(n), _meta(5000)
    rank, vals = _meta(n, dtype=i64), _meta(n)
    T.rank_resolve_mlp_f32(us, gs, s, ahead, 130, P, Q, *tail, None, None, None, None, rank, vals)
    T.rank_resolve_mlp_f32(us, gs, s, ahead, 130, P, Q, *tail, Z, p, ip, ix, rank, vals)
    with pytest.raises(ValueError, match="exclude_indptr and exclude_indices come together"):
        T.rank_resolve_mlp_f32(us, gs, s, ahead, 130, P, Q, *tail, None, None, ip, None, rank, vals)
    with pytest.raises(ValueError, match="Z and p_col come together"):
        T.rank_resolve_mlp_f32(us, gs, s, ahead, 130, P, Q, *tail, Z, None, None, None, rank, vals)
    with pytest.raises(ValueError, match="n_users \\+ 1"):
        T.rank_resolve_mlp_f32(us, gs, s, ahead, 131, P, Q, *tail, None, None, ip, ix, rank, vals)
    with pytest.raises(ValueError, match="one row per pair"):
        T.rank_resolve_mlp_f32(us, gs, s, ahead, 130, _meta(130, 128), Q, *tail, None, None, None,
                               None, rank, vals)
    with pytest.raises(ValueError, match="Z must be contiguous \\[77\\]"):
        T.rank_resolve_mlp_f32(us, gs, s, ahead, 130, P, Q, *tail, _meta(130), p, None, None, rank,
                               vals)
    with pytest.raises(ValueError, match="rank must be Long"):
        T.rank_resolve_mlp_f32(us, gs, s, ahead, 130, P, Q, *tail, None, None, None, None,
                               _meta(n, dtype=i32), vals)
    with pytest.raises(ValueError, match="vals must be contiguous \\[77\\]"):
        T.rank_resolve_mlp_f32(us, gs, s, ahead, 130, P, Q, *tail, None, None, None, None, rank,
                               _meta(n - 1))
    with pytest.raises(ValueError, match="must be contiguous \\[77\\]"):
        T.rank_resolve_mlp_f32(us, _meta(n - 1, dtype=i64), s, ahead, 130, P, Q, *tail, None, None,
                               None, None, rank, vals)
    with pytest.raises(ValueError, match="users must be Long"):
        T.rank_resolve_mlp_f32(_meta(n, dtype=i32), gs, s, ahead, 130, P, Q, *tail, None, None,
                               None, None, rank, vals)
    with pytest.raises(ValueError, match="pairs need users and items"):
        T.rank_resolve_mlp_f32(us, gs, s, ahead, 130, P, _meta(0, 128), *tail, None, None, None,
                               None, rank, vals)
    with pytest.raises(ValueError, match="128/32 hidden sizes"):
        T.rank_resolve_mlp_f32(us, gs, s, ahead, 130, _meta(n, 64), Q, *tail, None, None, None,
                               None, rank, vals)


# ---------------------------------------------------------------- refusals
def test_wrappers_refuse_cpu_tensors():
    from gnnrec import ops
    i32, i64 = torch.int32, torch.int64
    P, Q = torch.zeros(4, 128), torch.zeros(9, 128)
    tail = (torch.zeros(32, 128), torch.zeros(32), torch.zeros(32), torch.zeros(1))
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.edge_mlp_dense_count(P, Q, *tail, torch.zeros(4), torch.zeros(4, dtype=i32))
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.edge_mlp_dense_count_rating(P, Q, *tail, torch.zeros(4), torch.zeros(9), torch.zeros(4),
                                        torch.zeros(4, dtype=i32))
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.rank_resolve_mlp(torch.zeros(4, dtype=i64), torch.zeros(4, dtype=i64), torch.zeros(4),
                             torch.zeros(4, dtype=i32), 6, P, Q, *tail)
    # a device table does not excuse a host operand after it
    with pytest.raises(ValueError, match="gid must be"):
        ops.edge_mlp_dense_count(_meta(4, 128), _meta(9, 128), *_tail(), _meta(4),
                                 _meta(4, dtype=i64))


def test_popularity_without_a_head_is_not_implemented():
    """Refused before anything touches a device: meta and CPU inputs alike get here."""
    from gnnrec import recs
    i64 = torch.int64
    with pytest.raises(NotImplementedError, match="popularity= needs head="):
        recs.rank_items(_meta(4, 16), _meta(9, 16), _meta(3, dtype=i64), _meta(3, dtype=i64),
                        popularity=_meta(9))
    with pytest.raises(NotImplementedError, match="popularity= needs head="):
        recs.rank_items(torch.zeros(4, 16), torch.zeros(9, 16), torch.zeros(3, dtype=i64),
                        torch.zeros(3, dtype=i64), popularity=torch.zeros(9), weight_popularity=0.5)

    class _G:
        ndata = {"popularity": {"item": torch.zeros(9)}}

        def in_csr(self, etype):
            raise AssertionError("the graph's lists are not touched before the refusal")

    with pytest.raises(NotImplementedError, match="popularity= needs head="):
        recs.rank_for_graph(_G(), {"user": torch.zeros(4, 16), "item": torch.zeros(9, 16)},
                            ([0], [1]), use_popularity=True)


def test_rank_for_graph_without_popularity_data():
    from gnnrec import recs

    class _G:
        ndata = {}

    with pytest.raises(KeyError, match="popularity"):
        recs.rank_for_graph(_G(), {"user": torch.zeros(4, 16), "item": torch.zeros(9, 16)},
                            ([0], [1]), use_popularity=True, head=mc.head(16))


def test_head_arguments_are_checked_on_the_host():
    """rank_items(head=) keeps the cosine path's argument checks."""
    from gnnrec import recs
    i64 = torch.int64
    with pytest.raises(ValueError, match="HIP device tensor"):
        recs.rank_items(torch.zeros(4, 16), torch.zeros(9, 16), torch.zeros(3, dtype=i64),
                        torch.zeros(3, dtype=i64), head=mc.head(16))
    with pytest.raises(ValueError, match="3 users for 2 items"):
        recs.rank_items(_meta(4, 16), _meta(9, 16), _meta(3, dtype=i64), _meta(2, dtype=i64),
                        head=mc.head(16))


# ---------------------------------------------------------------- what the GPU tests lean on
@functools.lru_cache(maxsize=None)
def _saturated():
    hu, hi = rc.tables("normal", rm.SATURATED_D)
    S = mc.host_scores(mc.saturated_head(rm.SATURATED_D), hu, hi)
    return S, rk.pairs(S, rc.exclusions())


def test_saturated_pairs_are_tied_on_both_sides():
    """The tie rule is exercised, not merely allowed: most scores are exactly 1.0f, and for most
    pairs some item below the held-out id and some item above it carry exactly its score."""
    S, (us, gs) = _saturated()
    assert (S == 1.0).mean() > 0.99
    assert us.size == rk.PAIRS_PER_USER * rc.N_USERS
    both = rm.tied_both_sides(S, us, gs)
    print(f"saturated pairs tied on both sides: {both.mean():.4f}")
    assert both.mean() >= rm.TIED_BOTH_SIDES_MIN
    # and the ranks of those pairs are decided by ids: dropping the tie rule moves them
    r = rk.ranks(S, us, gs)
    strict = 1 + (S[us] > S[us, gs][:, None]).sum(1)
    assert (r[both] > strict[both]).all()


@pytest.mark.parametrize("weight", rm.POP_WEIGHTS)
def test_popularity_vector_gives_exact_rating_ties(weight):
    """POP_LEVELS distinct popularity values: items of one level whose softmax terms differ by
    less than an ulp of the sum collide (weight 0.5), and so do equal softmax terms (0.0)."""
    hu, hi = rc.tables("normal", 64)
    S = mc.host_scores(mc.head(64), hu, hi)
    pop = rm.popularity()
    assert np.unique(pop).size == rm.POP_LEVELS
    p = (pop * np.float32(weight)).astype(np.float32)
    Z = np.exp(S).sum(1, dtype=np.float64).astype(np.float32)
    R = rm.ratings32(S, Z, p)
    assert R.dtype == np.float32
    tied_rows = sum(np.unique(R[u]).size < R.shape[1] for u in range(R.shape[0]))
    print(f"weight {weight}: {tied_rows} of {R.shape[0]} rows hold an exact R tie")
    assert tied_rows >= R.shape[0] // 2
