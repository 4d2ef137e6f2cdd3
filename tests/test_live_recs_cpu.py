"""CPU-side checks of the cached lists' update (gnnrec.recs.update_recommendations,
gnnrec_topk_update_f32): the settle rule restated in numpy on the tables the GPU
tests run (tests/live_recs_cases.py) — a settled row IS the exhaustive ranking's, the filter
keeps every dirty item that can enter — the share of rows the rule cannot settle on the small
perturbation, the Meta kernel's argument checks, and the C entry's declaration and binding.
Nothing launches here.

The restatement tests (the first five) pin the RULE on the shared tables, not the code: they
import nothing of the feature and pass without it.  The Meta-kernel, refusal and C-entry tests
below them are the ones that need the feature."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import live_recs_cases as lc
import recommend_cases as rc


@functools.lru_cache(maxsize=None)
def _restated(d, k, n_di, n_du):
    c = lc.grid_case(d, k, n_di, n_du)
    s0 = rc.cosine64(c["hu0"], c["hi0"])
    s1 = lc.refreshed_scores(s0, c["hu1"], c["hi1"], c["du"], c["di"])
    a1 = lc.approx(c["hu1"], c["hi1"])
    return c, s1, a1, lc.rule(s0, s1, a1, c["excl"], k, c["du"], c["di"])


@pytest.mark.parametrize("d,k,n_di,n_du", lc.GRID)
def test_a_settled_row_is_the_exhaustive_ranking(d, k, n_di, n_du):
    c, s1, _a1, (idx, vals, settled, _kept, _und) = _restated(d, k, n_di, n_du)
    want_i, want_v = rc.ranked(s1, *c["excl"], k)
    clean = np.setdiff1d(np.arange(lc.N_USERS), c["du"])
    same = (idx == want_i).all(1) & (vals == want_v).all(1)
    # every settled row equals the exhaustive (score desc, id asc) ranking ...
    assert same[clean][settled[clean]].all()
    # ... so every row whose merged list is NOT that ranking is flagged unsettled
    assert not settled[clean][~same[clean]].any()
    assert not settled[c["du"]].any()      # dirty users are never the merge's business
    if n_di >= lc.SMALL:                   # the case is not vacuous: clean users' lists change
        old_i, _ = rc.ranked(rc.cosine64(c["hu0"], c["hi0"]), *c["excl"], k)
        assert (want_i[clean] != old_i[clean]).any()


@pytest.mark.parametrize("d,k,n_di,n_du", lc.GRID)
def test_the_filter_keeps_every_dirty_item_that_can_enter(d, k, n_di, n_du):
    """K_u (approximate score >= s_last - 2 EPS) holds every dirty eligible item whose
    refreshed score is >= s_last: |a - score| <= EPS."""
    c, s1, a1, (_idx, _vals, _settled, kept, _und) = _restated(d, k, n_di, n_du)
    s0 = rc.cosine64(c["hu0"], c["hi0"])
    _i0, v0 = rc.ranked(s0, *c["excl"], k)
    indptr, indices = c["excl"]
    assert np.abs(a1 - s1).max() <= lc.EPS
    for u in np.setdiff1d(np.arange(lc.N_USERS), c["du"]):
        s_last = v0[u][np.isfinite(v0[u])][-1]
        must = set(c["di"][s1[u, c["di"]] >= s_last].tolist()) - \
            set(indices[indptr[u]:indptr[u + 1]].tolist())
        assert must <= kept[u], (u, must - kept[u])


def test_small_perturbation_leaves_few_rows_unsettled():
    """A CONDITION of the GPU test, not a measurement: with 5 % of the items moved by
    0.05 N(0, 1) (and lists of k <= 10) at most 5 % of the clean rows are unsettled in the
    restatement — half the cap tests/test_gpu_live_recs.py asserts on the device's redo_rows
    for the same tables, and for every other grid case that stays under 5 % here.  (With 129
    of 700 items dirty, or k = 64 and 35 dirty, the rule itself leaves 8 - 22 %: a list's last
    entry is then dirty in about that share of the rows, and whenever its score falls the row
    cannot be settled.  There the GPU test holds the device to the restatement's own count.)"""
    small = [g for g in lc.GRID if g[2] <= lc.SMALL and g[1] <= 10]
    assert {(64, 5, 35), (128, 10, 35)} <= {g[:3] for g in small}
    for d, k, n_di, n_du in small:
        _c, _s1, _a1, (_idx, _vals, settled, _kept, _und) = _restated(d, k, n_di, n_du)
        n_clean = lc.N_USERS - n_du
        share = (n_clean - int(settled.sum())) / n_clean
        print(f"d {d} k {k} dirty items {n_di} users {n_du}: unsettled share {share:.3f}")
        assert share <= lc.UNSETTLED_CPU, (d, k, n_di, n_du, share)
    for d, k, n_di, n_du in lc.GRID:   # what the GPU test adds to the restated count
        und = _restated(d, k, n_di, n_du)[3][4]
        print(f"d {d} k {k} dirty items {n_di}: {int(und.sum())} rows undecided within "
              f"{lc.DECIDE_TOL:g}")


def test_a_leaving_item_is_flagged():
    """A list entry whose refreshed score drops to -1 cannot be replaced from inside the merged
    set: the row must be unsettled."""
    d, k = 64, 10
    hu, hi0 = lc.tables(d)
    excl = lc.exclusions()
    s0 = rc.cosine64(hu, hi0)
    i0, _v0 = rc.ranked(s0, *excl, k)
    u, v = 7, int(i0[7, 3])
    hi1 = hi0.copy()
    hi1[v] = -hu[u]
    di = np.asarray([v], np.int64)
    s1 = lc.refreshed_scores(s0, hu, hi1, np.empty(0, np.int64), di)
    _idx, _vals, settled, _kept, _und = lc.rule(s0, s1, lc.approx(hu, hi1), excl, k,
                                          np.empty(0, np.int64), di)
    assert not settled[u]


# ---------------------------------------------------------------- Meta kernel
def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta")


def _args(n_users=40, n_items=300, d=64, k=10, B=7, cap=246, nd=12):
    i32, i64 = torch.int32, torch.int64
    return dict(rows=_meta(B, dtype=i64), idx=_meta(n_users, k, dtype=i64), vals=_meta(n_users, k),
                item_mark=_meta(n_items, dtype=i32), counts=_meta(B, dtype=i32),
                cand_cols=_meta(B, cap, dtype=i32), dirty_ids=_meta(nd, dtype=i32),
                h_user=_meta(n_users, d), h_item=_meta(n_items, d),
                exclude_indptr=_meta(n_users + 1, dtype=i64),
                exclude_indices=_meta(400, dtype=i32), redo=_meta(n_users, dtype=i32))


def _call(**over):
    from gnnrec import _lib
    a = dict(_args(), **over)
    _lib.torch_ops().topk_update(*a.values())


def test_meta_topk_update_accepts_the_shapes_of_the_update():
    _call()
    _call(exclude_indptr=None, exclude_indices=None)
    a = _args(k=64, cap=192)
    _call(**a)
    a = _args(k=1, cap=255)
    _call(**a)


@pytest.mark.parametrize("name,dtype,match", [
    ("rows", torch.int32, "rows must be Long"),
    ("idx", torch.int32, "idx must be Long"),
    ("vals", torch.float64, "vals must be Float"),
    ("item_mark", torch.int64, "item_mark must be Int"),
    ("counts", torch.int64, "counts must be Int"),
    ("cand_cols", torch.int64, "cand_cols must be Int"),
    ("dirty_ids", torch.int64, "dirty_ids must be Int"),
    ("h_user", torch.float16, "h_user must be Float"),
    ("exclude_indices", torch.int64, "exclude_indices must be Int"),
    ("redo", torch.int64, "redo must be Int"),
])
def test_meta_topk_update_refuses_wrong_dtypes(name, dtype, match):
    a = _args()
    with pytest.raises(ValueError, match=match):
        _call(**{name: torch.empty(a[name].shape, dtype=dtype, device="meta")})


def test_meta_topk_update_refuses_wrong_shapes_and_ranges():
    i32, i64 = torch.int32, torch.int64
    with pytest.raises(ValueError, match="idx / vals"):
        _call(idx=_meta(39, 10, dtype=i64))
    with pytest.raises(ValueError, match="idx / vals"):
        _call(vals=_meta(40, 9))
    with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
        _call(**_args(k=65, cap=100))
    with pytest.raises(ValueError, match="cap must be"):
        _call(**_args(k=10, cap=247))
    with pytest.raises(ValueError, match="cap must be"):
        _call(**_args(k=64, cap=193))
    with pytest.raises(ValueError, match="cand_cols"):
        _call(counts=_meta(6, dtype=i32))
    with pytest.raises(ValueError, match="multiple of 4"):
        _call(**_args(d=6))
    with pytest.raises(ValueError, match="multiple of 4"):
        _call(h_item=_meta(300, 32))
    with pytest.raises(ValueError, match="item_mark must be"):
        _call(item_mark=_meta(299, dtype=i32))
    with pytest.raises(ValueError, match="redo must be"):
        _call(redo=_meta(41, dtype=i32))
    with pytest.raises(ValueError, match="come together"):
        _call(exclude_indices=None)
    with pytest.raises(ValueError, match="exclude_indptr must be"):
        _call(exclude_indptr=_meta(40, dtype=i64))


def test_cpu_tensors_are_refused():
    from gnnrec import recs
    z = torch.zeros
    with pytest.raises(ValueError, match="HIP device tensor"):
        recs.update_recommendations(z(4, 3, dtype=torch.int64), z(4, 3), z(4, 16), z(9, 16),
                                    None, None)


def test_head_and_popularity_are_refused():
    from gnnrec import recs
    m = _meta
    for kw in ({"head": object()}, {"popularity": m(9)}):
        with pytest.raises(ValueError, match="refused"):
            recs.update_recommendations(m(4, 3, dtype=torch.int64), m(4, 3), m(4, 16), m(9, 16),
                                        None, None, **kw)


# ---------------------------------------------------------------- the C entry
def _declared_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "gnnrec.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(gnnrec_[a-z0-9_]+)\s*\(", txt))


def test_header_declares_and_lib_binds_the_entry():
    from gnnrec import _lib
    assert "gnnrec_topk_update_f32" in _declared_symbols()
    assert "gnnrec_topk_update_f32" in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, "gnnrec_topk_update_f32")
    p16 = ctypes.c_void_p(16)
    # refusals before any launch, through gnnrec_last_error
    rc_ = lib.gnnrec_topk_update_f32(p16, 3, p16, p16, 9, 65, p16, 40, p16, p16, 64, p16, 5, p16,
                                     16, p16, 16, 16, None, None, p16, None)
    assert rc_ == _lib.OK + 1 and b"k must be in [1, 64]" in lib.gnnrec_last_error()
    rc_ = lib.gnnrec_topk_update_f32(p16, 3, p16, p16, 9, 10, p16, 40, p16, p16, 247, p16, 5, p16,
                                     16, p16, 16, 16, None, None, p16, None)
    assert rc_ == _lib.OK + 1 and b"cap must be" in lib.gnnrec_last_error()
    rc_ = lib.gnnrec_topk_update_f32(p16, 3, p16, p16, 9, 10, p16, 40, p16, p16, 64, p16, 5, p16,
                                     16, p16, 16, 16, None, None, None, None)
    assert rc_ == _lib.OK + 1 and b"null pointer" in lib.gnnrec_last_error()
    # empty problems succeed without touching memory
    assert lib.gnnrec_topk_update_f32(None, 0, None, None, 9, 10, None, 40, None, None, 64, None,
                                      5, None, 16, None, 16, 16, None, None, None, None) == 0
    assert lib.gnnrec_topk_update_f32(None, 3, None, None, 9, 10, None, 40, None, None, 64, None,
                                      0, None, 16, None, 16, 16, None, None, None, None) == 0
