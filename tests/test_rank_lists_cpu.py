"""Host checks for the list-shaped full-ranking evaluation (gnnrec.recs.rank_lists / list_pairs
/ rank_lists_for_graph): list_pairs and the row plan against numpy restatements
on CPU tensors, the validation that comes before any launch, the argument checks of the new ops
on meta tensors, the C entries, and — for the very lists tests/test_gpu_rank_lists.py gives the
saturated head — the share of entries whose rank is decided by the id tie rule on both sides."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import rank_lists_cases as rl
import rank_mlp_cases as rm
import recommend_cases as rc
import recommend_mlp_cases as mc

i32, i64 = torch.int32, torch.int64


def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta")


def _T():
    from gnnrec import _lib
    return _lib.torch_ops()


def _tail():
    return _meta(32, 128), _meta(32), _meta(32), _meta(1)


# ---------------------------------------------------------------- list_pairs
def _gt():
    lists = [[4, 2, 4], [], [9], [0, 7, 7, 1], [], [3, 3]]      # unsorted, empty, duplicates
    return rc.csr(lists)


@pytest.mark.parametrize("rows", [None, [3, 0, 5], [1, 4], [4, 2, 1], []])
def test_list_pairs_is_the_restatement(rows):
    """On CPU tensors, without the library: every user, an unsorted subset, empty lists (alone
    and between others), duplicates inside a list."""
    from gnnrec import recs
    ip, ix = _gt()
    want_u, want_g = rl.list_pairs(rows, ip, ix)
    for idx in (torch.from_numpy(ix), torch.from_numpy(ix.astype(np.int64))):
        us, gs = recs.list_pairs(None if rows is None else torch.tensor(rows, dtype=i64),
                                 torch.from_numpy(ip), idx)
        assert us.dtype == i64 and gs.dtype == i64
        np.testing.assert_array_equal(us.numpy(), want_u)
        np.testing.assert_array_equal(gs.numpy(), want_g)
    if rows is None:
        assert want_g.tolist() == [4, 2, 4, 9, 0, 7, 7, 1, 3, 3]
    if rows == [3, 0, 5]:
        assert want_u.tolist() == [3] * 4 + [0] * 3 + [5] * 2


def test_list_pairs_refuses_users_out_of_range():
    from gnnrec import recs
    ip, ix = _gt()
    for bad in ([6], [-1, 2]):
        with pytest.raises(ValueError, match="out of range"):
            recs.list_pairs(torch.tensor(bad, dtype=i64), torch.from_numpy(ip),
                            torch.from_numpy(ix))


# ---------------------------------------------------------------- the row plan
@pytest.mark.parametrize("budget", [rl.BUDGET, 1, 3])
def test_row_plan_covers_every_slot_once_within_the_budget(budget):
    from gnnrec import recs
    B = budget
    cases = [[0, 1, B - 1, B, B + 1, 5 * B], [5 * B], [0, 0], [0], [], [B + 1, 0, 0, B, 1, 0]]
    if B == rl.BUDGET:
        assert tuple(cases[0]) == rl.PLAN_LENGTHS
        cases.append(np.random.default_rng(0).choice(rl.PLAN_LENGTHS, 200).tolist())
    for lens in cases:
        lens = np.asarray(lens, np.int64)
        want_owner, want_lptr = rl.row_plan(lens, B)
        for n_rows in (None, want_owner.size):          # read by the plan, or given
            owner, lptr = recs._list_row_plan(torch.from_numpy(lens), B, n_rows)
            assert owner.dtype == i64 and lptr.dtype == i64
            np.testing.assert_array_equal(owner.numpy(), want_owner)
            np.testing.assert_array_equal(lptr.numpy(), want_lptr)
        owner, lptr = owner.numpy(), lptr.numpy()
        # every slot exactly once, in list order, no row over the budget or empty
        size = np.diff(lptr)
        assert lptr[0] == 0 and lptr[-1] == lens.sum()
        assert ((size >= 1) & (size <= B)).all()
        slot_owner = np.repeat(owner, size)
        np.testing.assert_array_equal(slot_owner, np.repeat(np.arange(lens.size), lens))
        np.testing.assert_array_equal(np.bincount(owner, minlength=lens.size), -(-lens // B))


def test_budget_is_the_kernels():
    from gnnrec import _lib, ops
    assert ops.rank_list_slots() == rl.BUDGET == _lib.load().gnnrec_rank_list_slots()


# ---------------------------------------------------------------- validation before any launch
def test_id_check_on_cpu_tensors():
    """The one read's checks are plain torch: a repeated user, ids out of range in user_rows
    and in a SERVED list only, an indptr that is not one."""
    from gnnrec import recs
    ip, ix = (torch.from_numpy(a) for a in _gt())
    rows = torch.tensor([3, 0, 5], dtype=i64)
    lens, served, E, more = recs._lists_check(rows, ip, ix, 6, 10,
                                              lambda lens, served: [lens.max(), served.sum()])
    assert lens.tolist() == [4, 3, 2] and E == 9 and more == [4, 3]
    assert served.tolist() == [True, False, False, True, False, True]
    with pytest.raises(ValueError, match="repeated user"):
        recs._lists_check(torch.tensor([3, 0, 3], dtype=i64), ip, ix, 6, 10)
    for bad in ([3, 6], [-1, 0]):
        with pytest.raises(ValueError, match="out of range"):
            recs._lists_check(torch.tensor(bad, dtype=i64), ip, ix, 6, 10)
    with pytest.raises(ValueError, match="out of range"):     # user 2's list holds item 9
        recs._lists_check(torch.tensor([2], dtype=i64), ip, ix, 6, 9)
    recs._lists_check(rows, ip, ix, 6, 8)                     # ... and user 2 is not served here
    neg = ix.clone()
    neg[4] = -1                                               # user 3's first entry
    with pytest.raises(ValueError, match="out of range"):
        recs._lists_check(rows, ip, neg, 6, 10)
    with pytest.raises(ValueError, match="not the indptr"):
        recs._lists_check(rows, ip + 1, ix, 6, 10)


def test_arguments_are_checked_on_the_host():
    from gnnrec import recs
    hu, hi = _meta(6, 16), _meta(10, 16)
    ip, ix = _meta(7, dtype=i64), _meta(10, dtype=i32)
    pl = mc.head(16)
    with pytest.raises(ValueError, match="gt_indptr must be int64 \\[n_users \\+ 1 = 7\\]"):
        recs.rank_lists(hu, hi, None, _meta(6, dtype=i64), ix, head=pl)
    with pytest.raises(ValueError, match="gt_indptr must be int64"):
        recs.rank_lists(hu, hi, None, _meta(7, dtype=i32), ix)
    with pytest.raises(ValueError, match="gt_indptr must be int64"):
        recs.rank_lists(torch.zeros(6, 16), torch.zeros(10, 16), None,
                        torch.zeros(8, dtype=i64), torch.zeros(3, dtype=i64))
    with pytest.raises(ValueError, match="gt_indices must be int32 or int64"):
        recs.rank_lists(hu, hi, None, ip, _meta(10), head=pl)
    with pytest.raises(ValueError, match="HIP device tensor"):
        recs.rank_lists(torch.zeros(6, 16), torch.zeros(10, 16), None,
                        torch.zeros(7, dtype=i64), torch.zeros(3, dtype=i64), head=pl)
    with pytest.raises(ValueError, match="user_rows must be torch.int64"):
        recs.rank_lists(hu, hi, _meta(3, dtype=i32), ip, ix, head=pl)
    with pytest.raises(ValueError, match="batch_size must be >= 1"):
        recs.rank_lists(hu, hi, None, ip, ix, head=pl, batch_size=0)
    with pytest.raises(ValueError, match="exclude indptr must have n_users \\+ 1"):
        recs.rank_lists(hu, hi, None, ip, ix, (_meta(6, dtype=i64), _meta(4, dtype=i32)), head=pl)


def test_popularity_without_a_head_is_not_implemented():
    """rank_items' refusal, before anything touches a device or the graph."""
    from gnnrec import recs
    with pytest.raises(NotImplementedError, match="popularity= needs head="):
        recs.rank_lists(_meta(4, 16), _meta(9, 16), None, _meta(5, dtype=i64),
                        _meta(3, dtype=i64), popularity=_meta(9))
    with pytest.raises(NotImplementedError, match="popularity= needs head="):
        recs.rank_lists(torch.zeros(4, 16), torch.zeros(9, 16), torch.zeros(2, dtype=i64),
                        torch.zeros(5, dtype=i64), torch.zeros(3, dtype=i64),
                        popularity=torch.zeros(9), weight_popularity=0.5)

    class _G:
        ndata = {"popularity": {"item": torch.zeros(9)}}

        def in_csr(self, etype):
            raise AssertionError("the graph's lists are not touched before the refusal")

    with pytest.raises(NotImplementedError, match="popularity= needs head="):
        recs.rank_lists_for_graph(_G(), {"user": torch.zeros(4, 16), "item": torch.zeros(9, 16)},
                                  ([0], [1]), use_popularity=True)

    class _Bare:
        ndata = {}

    with pytest.raises(KeyError, match="popularity"):
        recs.rank_lists_for_graph(_Bare(), {"user": torch.zeros(4, 16),
                                            "item": torch.zeros(9, 16)},
                                  ([0], [1]), use_popularity=True, head=mc.head(16))


# ---------------------------------------------------------------- Meta kernels
def test_meta_dense_count_lists():
    T = _T()
    P, Q, tail = _meta(130, 128), _meta(5000, 128), _tail()
    E = 700
    lptr, thr, gid = _meta(131, dtype=i64), _meta(E), _meta(E, dtype=i32)
    parts, ahead = _meta(5, E, dtype=i32), _meta(E, dtype=i32)
    T.edge_mlp_dense_count_lists_f32(P, Q, *tail, lptr, thr, gid, parts, ahead)
    T.edge_mlp_dense_count_lists_f32(_meta(0, 128), Q, *tail, _meta(1, dtype=i64), _meta(0),
                                     _meta(0, dtype=i32), _meta(5, 0, dtype=i32),
                                     _meta(0, dtype=i32))
    T.edge_mlp_dense_count_lists_f32(P, _meta(0, 128), *tail, lptr, thr, gid,
                                     _meta(0, E, dtype=i32), ahead)
    with pytest.raises(ValueError, match="lptr must be contiguous \\[131\\]"):
        T.edge_mlp_dense_count_lists_f32(P, Q, *tail, _meta(130, dtype=i64), thr, gid, parts, ahead)
    with pytest.raises(ValueError, match="lptr must be Long"):
        T.edge_mlp_dense_count_lists_f32(P, Q, *tail, _meta(131, dtype=i32), thr, gid, parts, ahead)
    with pytest.raises(ValueError, match="at most 16 slots a row"):
        T.edge_mlp_dense_count_lists_f32(P, Q, *tail, lptr, _meta(2081), _meta(2081, dtype=i32),
                                         _meta(5, 2081, dtype=i32), _meta(2081, dtype=i32))
    with pytest.raises(ValueError, match="parts must be a contiguous \\[5, 700\\]"):
        T.edge_mlp_dense_count_lists_f32(P, Q, *tail, lptr, thr, gid, _meta(4, E, dtype=i32), ahead)
    with pytest.raises(ValueError, match="parts must be a contiguous"):
        T.edge_mlp_dense_count_lists_f32(P, Q, *tail, lptr, thr, gid, _meta(5, 130, dtype=i32),
                                         ahead)
    with pytest.raises(ValueError, match="parts must be a contiguous"):
        T.edge_mlp_dense_count_lists_f32(P, Q, *tail, lptr, thr, gid, _meta(5 * E, dtype=i32),
                                         ahead)
    with pytest.raises(ValueError, match="parts must be Int"):
        T.edge_mlp_dense_count_lists_f32(P, Q, *tail, lptr, thr, gid, _meta(5, E), ahead)
    with pytest.raises(ValueError, match="ahead must be Int"):
        T.edge_mlp_dense_count_lists_f32(P, Q, *tail, lptr, thr, gid, parts, _meta(E, dtype=i64))
    with pytest.raises(ValueError, match="gid must be Int"):
        T.edge_mlp_dense_count_lists_f32(P, Q, *tail, lptr, thr, _meta(E, dtype=i64), parts, ahead)
    with pytest.raises(ValueError, match="thr must be Float"):
        T.edge_mlp_dense_count_lists_f32(P, Q, *tail, lptr, _meta(E, dtype=torch.float64), gid,
                                         parts, ahead)
    with pytest.raises(ValueError, match="gid / ahead"):
        T.edge_mlp_dense_count_lists_f32(P, Q, *tail, lptr, thr, _meta(E + 1, dtype=i32), parts,
                                         ahead)
    with pytest.raises(ValueError, match="gid / ahead must be contiguous \\[699\\]"):   # E is thr's
        T.edge_mlp_dense_count_lists_f32(P, Q, *tail, lptr, _meta(E - 1), gid, parts, ahead)
    with pytest.raises(ValueError, match="gid / ahead"):
        T.edge_mlp_dense_count_lists_f32(P, Q, *tail, lptr, thr, gid, parts,
                                         _meta(E - 1, dtype=i32))
    with pytest.raises(ValueError, match="128/32 hidden sizes"):
        T.edge_mlp_dense_count_lists_f32(_meta(130, 64), Q, *tail, lptr, thr, gid, parts, ahead)
    with pytest.raises(ValueError, match="128/32 hidden sizes"):
        T.edge_mlp_dense_count_lists_f32(P, Q, _meta(32, 64), *tail[1:], lptr, thr, gid, parts,
                                         ahead)


def test_meta_dense_count_lists_rating():
    T = _T()
    P, Q, tail = _meta(130, 128), _meta(5000, 128), _tail()
    E = 700
    Z, p = _meta(130), _meta(5000)
    lptr, s, gid = _meta(131, dtype=i64), _meta(E), _meta(E, dtype=i32)
    parts, ahead = _meta(5, E, dtype=i32), _meta(E, dtype=i32)
    T.edge_mlp_dense_count_lists_rating_f32(P, Q, *tail, Z, p, lptr, s, gid, parts, ahead)
    with pytest.raises(ValueError, match="Z must be contiguous \\[130\\]"):      # per row, not slot
        T.edge_mlp_dense_count_lists_rating_f32(P, Q, *tail, _meta(E), p, lptr, s, gid, parts,
                                                ahead)
    with pytest.raises(ValueError, match="p_col must be contiguous \\[5000\\]"):
        T.edge_mlp_dense_count_lists_rating_f32(P, Q, *tail, Z, _meta(4999), lptr, s, gid, parts,
                                                ahead)
    with pytest.raises(ValueError, match="p_col must be Float"):
        T.edge_mlp_dense_count_lists_rating_f32(P, Q, *tail, Z, _meta(5000, dtype=torch.float64),
                                                lptr, s, gid, parts, ahead)
    with pytest.raises(ValueError, match="lptr must be contiguous \\[131\\]"):
        T.edge_mlp_dense_count_lists_rating_f32(P, Q, *tail, Z, p, _meta(132, dtype=i64), s, gid,
                                                parts, ahead)
    with pytest.raises(ValueError, match="parts must be a contiguous \\[5, 700\\]"):
        T.edge_mlp_dense_count_lists_rating_f32(P, Q, *tail, Z, p, lptr, s, gid,
                                                _meta(6, E, dtype=i32), ahead)
    with pytest.raises(ValueError, match="gid must be Int"):
        T.edge_mlp_dense_count_lists_rating_f32(P, Q, *tail, Z, p, lptr, s, _meta(E), parts, ahead)
    with pytest.raises(ValueError, match="gid / ahead must be contiguous \\[701\\]"):   # E is s's
        T.edge_mlp_dense_count_lists_rating_f32(P, Q, *tail, Z, p, lptr, _meta(E + 1), gid, parts,
                                                ahead)
    with pytest.raises(ValueError, match="128/32 hidden sizes"):
        T.edge_mlp_dense_count_lists_rating_f32(P, _meta(5000, 64), *tail, Z, p, lptr, s, gid,
                                                parts, ahead)


def test_meta_rank_resolve_mlp_lists():
    T = _T()
    B, E = 40, 77
    ru, lptr = _meta(B, dtype=i64), _meta(B + 1, dtype=i64)
    s, gid, ahead = _meta(E), _meta(E, dtype=i32), _meta(E, dtype=i32)
    P, Q, tail = _meta(B, 128), _meta(5000, 128), _tail()
    ip, ix = _meta(131, dtype=i64), _meta(900, dtype=i32)
    Z, p = _meta(B), _meta(5000)
    rank, vals = _meta(E, dtype=i64), _meta(E)
    T.rank_resolve_mlp_lists_f32(ru, lptr, s, gid, ahead, 130, P, Q, *tail, None, None, None,
                                 None, rank, vals)
    T.rank_resolve_mlp_lists_f32(ru, lptr, s, gid, ahead, 130, P, Q, *tail, Z, p, ip, ix, rank,
                                 vals)
    with pytest.raises(ValueError, match="exclude_indptr and exclude_indices come together"):
        T.rank_resolve_mlp_lists_f32(ru, lptr, s, gid, ahead, 130, P, Q, *tail, None, None, ip,
                                     None, rank, vals)
    with pytest.raises(ValueError, match="Z and p_col come together"):
        T.rank_resolve_mlp_lists_f32(ru, lptr, s, gid, ahead, 130, P, Q, *tail, Z, None, None,
                                     None, rank, vals)
    with pytest.raises(ValueError, match="n_users \\+ 1"):
        T.rank_resolve_mlp_lists_f32(ru, lptr, s, gid, ahead, 131, P, Q, *tail, None, None, ip, ix,
                                     rank, vals)
    with pytest.raises(ValueError, match="one row per list row"):
        T.rank_resolve_mlp_lists_f32(ru, lptr, s, gid, ahead, 130, _meta(E, 128), Q, *tail, None,
                                     None, None, None, rank, vals)
    with pytest.raises(ValueError, match="Z must be contiguous \\[40\\]"):
        T.rank_resolve_mlp_lists_f32(ru, lptr, s, gid, ahead, 130, P, Q, *tail, _meta(E), p, None,
                                     None, rank, vals)
    with pytest.raises(ValueError, match="row_user / lptr"):
        T.rank_resolve_mlp_lists_f32(ru, _meta(B, dtype=i64), s, gid, ahead, 130, P, Q, *tail,
                                     None, None, None, None, rank, vals)
    with pytest.raises(ValueError, match="at most 16 slots a row"):
        T.rank_resolve_mlp_lists_f32(ru, lptr, _meta(641), _meta(641, dtype=i32),
                                     _meta(641, dtype=i32), 130, P, Q, *tail, None, None, None,
                                     None, _meta(641, dtype=i64), _meta(641))
    with pytest.raises(ValueError, match="rank must be Long"):
        T.rank_resolve_mlp_lists_f32(ru, lptr, s, gid, ahead, 130, P, Q, *tail, None, None, None,
                                     None, _meta(E, dtype=i32), vals)
    with pytest.raises(ValueError, match="vals must be contiguous \\[77\\]"):
        T.rank_resolve_mlp_lists_f32(ru, lptr, s, gid, ahead, 130, P, Q, *tail, None, None, None,
                                     None, rank, _meta(E - 1))
    with pytest.raises(ValueError, match="gid must be Int"):
        T.rank_resolve_mlp_lists_f32(ru, lptr, s, _meta(E, dtype=i64), ahead, 130, P, Q, *tail,
                                     None, None, None, None, rank, vals)
    with pytest.raises(ValueError, match="must be contiguous \\[77\\]"):
        T.rank_resolve_mlp_lists_f32(ru, lptr, s, _meta(E - 1, dtype=i32), ahead, 130, P, Q, *tail,
                                     None, None, None, None, rank, vals)
    with pytest.raises(ValueError, match="row_user must be Long"):
        T.rank_resolve_mlp_lists_f32(_meta(B, dtype=i32), lptr, s, gid, ahead, 130, P, Q, *tail,
                                     None, None, None, None, rank, vals)
    with pytest.raises(ValueError, match="entries need users and items"):
        T.rank_resolve_mlp_lists_f32(ru, lptr, s, gid, ahead, 130, P, _meta(0, 128), *tail, None,
                                     None, None, None, rank, vals)
    with pytest.raises(ValueError, match="128/32 hidden sizes"):
        T.rank_resolve_mlp_lists_f32(ru, lptr, s, gid, ahead, 130, _meta(B, 64), Q, *tail, None,
                                     None, None, None, rank, vals)


def test_wrappers_refuse_cpu_tensors():
    from gnnrec import ops
    P, Q = torch.zeros(4, 128), torch.zeros(9, 128)
    tail = (torch.zeros(32, 128), torch.zeros(32), torch.zeros(32), torch.zeros(1))
    lptr, s, gid = torch.zeros(5, dtype=i64), torch.zeros(6), torch.zeros(6, dtype=i32)
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.edge_mlp_dense_count_lists(P, Q, *tail, lptr, s, gid)
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.edge_mlp_dense_count_lists_rating(P, Q, *tail, torch.zeros(4), torch.zeros(9), lptr, s,
                                              gid)
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.rank_resolve_mlp_lists(torch.zeros(4, dtype=i64), lptr, s, gid,
                                   torch.zeros(6, dtype=i32), 6, P, Q, *tail)
    with pytest.raises(ValueError, match="lptr must be"):
        ops.edge_mlp_dense_count_lists(_meta(4, 128), _meta(9, 128), *_tail(),
                                       _meta(5, dtype=i32), _meta(6), _meta(6, dtype=i32))


# ---------------------------------------------------------------- the C entries
def test_c_entries_are_declared_exported_and_validate():
    from gnnrec import _lib
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "gnnrec.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("gnnrec_rank_list_slots", "gnnrec_edge_mlp_dense_count_lists_f32",
                 "gnnrec_edge_mlp_dense_count_lists_rating_f32",
                 "gnnrec_rank_resolve_mlp_lists_f32"):
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    f16 = 16      # an aligned non-null address: validation only, nothing is launched
    # more slots than the rows can hold; negative sizes; nothing to do
    rc_ = lib.gnnrec_edge_mlp_dense_count_lists_f32(f16, 4, f16, 9, f16, f16, f16, f16, f16, 65,
                                                    f16, f16, f16, f16, None)
    assert rc_ != 0 and b"n_slots must be in" in lib.gnnrec_last_error()
    rc_ = lib.gnnrec_edge_mlp_dense_count_lists_f32(f16, 4, f16, 9, f16, f16, f16, f16, None, 5,
                                                    f16, f16, f16, f16, None)
    assert rc_ != 0 and b"null lptr" in lib.gnnrec_last_error()
    rc_ = lib.gnnrec_edge_mlp_dense_count_lists_rating_f32(f16, -1, f16, 9, f16, f16, f16, f16,
                                                           f16, f16, f16, 0, f16, f16, f16, f16,
                                                           None)
    assert rc_ != 0 and b"negative size" in lib.gnnrec_last_error()
    assert lib.gnnrec_edge_mlp_dense_count_lists_f32(f16, 4, f16, 9, f16, f16, f16, f16, None, 0,
                                                     None, None, None, None, None) == 0
    rc_ = lib.gnnrec_rank_resolve_mlp_lists_f32(f16, f16, 3, f16, f16, f16, 5, 4, f16, f16, 9,
                                                f16, f16, f16, f16, f16, None, None, None, f16,
                                                f16, None)
    assert rc_ != 0 and b"Z and p_col come together" in lib.gnnrec_last_error()
    rc_ = lib.gnnrec_rank_resolve_mlp_lists_f32(f16, f16, 3, f16, f16, f16, 49, 4, f16, f16, 9,
                                                f16, f16, f16, f16, None, None, None, None, f16,
                                                f16, None)
    assert rc_ != 0 and b"bad size" in lib.gnnrec_last_error()
    assert lib.gnnrec_rank_resolve_mlp_lists_f32(None, None, 0, None, None, None, 0, 4, None, None,
                                                 9, None, None, None, None, None, None, None,
                                                 None, None, None, None) == 0


# ---------------------------------------------------------------- what the GPU tests lean on
@functools.lru_cache(maxsize=None)
def _saturated():
    hu, hi = rc.tables("normal", rm.SATURATED_D)
    return mc.host_scores(mc.saturated_head(rm.SATURATED_D), hu, hi)


@pytest.mark.parametrize("n_users", rl.COUNT_ROWS)
def test_saturated_list_entries_are_tied_on_both_sides(n_users):
    """The condition tests/test_gpu_rank_lists.py's saturated count case states: for the lists
    it counts (all items), at least TIED_BOTH_SIDES_MIN of the entries have an item with
    exactly their score below their id and one above it, so their count is decided by ids."""
    S = _saturated()[:n_users]
    assert (S == 1.0).mean() > 0.99
    us, gs = rl.list_pairs(None, *rl.kernel_lists(n_users, rc.N_ITEMS))
    both = rm.tied_both_sides(S, us, gs)
    print(f"{n_users} users, {us.size} entries: tied on both sides {both.mean():.4f}")
    assert both.mean() >= rl.TIED_BOTH_SIDES_MIN


def test_kernel_lists_hold_what_the_tests_need():
    for n_users in rl.COUNT_ROWS:
        for n_items in rl.COUNT_ITEMS:
            ip, ix = rl.kernel_lists(n_users, n_items)
            lens = np.diff(ip)
            assert lens[(n_users - 1) // 2] == rl.LONG and set(lens) <= set(rl.LENGTHS) | {rl.LONG}
            assert ix.min() >= 0 and ix.max() < n_items
            for u in range(n_users):
                x = ix[ip[u]:ip[u + 1]]
                if x.size >= 3:
                    assert x[0] == n_items - 1 and x[1] == 0 and np.unique(x).size < x.size
    lens = np.diff(rl.kernel_lists(130, 5000)[0])
    assert set(lens) == set(rl.LENGTHS) | {rl.LONG}            # every length is drawn
