"""Host checks for the full-ranking evaluation of the MLP head (gnnrec.recs.rank_items(head=),
DESIGN.md §24): the refusals that come before any launch (the argument checks of its ops on
meta tensors are tests/test_rank_lists_cpu.py's: pairs run as one-slot rows of the list ops),
and — for the very inputs tests/test_gpu_rank_mlp.py uses — the exact ties
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


# ---------------------------------------------------------------- refusals
def test_wrappers_refuse_cpu_tensors():
    """The ops rank_items(head=) runs on: pairs as one-slot rows of the list ops."""
    from gnnrec import ops
    i32, i64 = torch.int32, torch.int64
    P, Q = torch.zeros(4, 128), torch.zeros(9, 128)
    tail = (torch.zeros(32, 128), torch.zeros(32), torch.zeros(32), torch.zeros(1))
    lptr = torch.arange(5)
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.edge_mlp_dense_count_lists(P, Q, *tail, lptr, torch.zeros(4), torch.zeros(4, dtype=i32))
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.edge_mlp_dense_count_lists_rating(P, Q, *tail, torch.zeros(4), torch.zeros(9), lptr,
                                              torch.zeros(4), torch.zeros(4, dtype=i32))
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.rank_resolve_mlp_lists(torch.zeros(4, dtype=i64), lptr, torch.zeros(4),
                                   torch.zeros(4, dtype=i32), torch.zeros(4, dtype=i32), 6, P, Q,
                                   *tail)
    # a device table does not excuse a host operand after it
    with pytest.raises(ValueError, match="gid must be"):
        ops.edge_mlp_dense_count_lists(_meta(4, 128), _meta(9, 128), *_tail(),
                                       _meta(5, dtype=i64), _meta(4), _meta(4, dtype=i64))


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
