"""GPU checks of the many-user top-k for the MLP head: the dense scoring kernels of
csrc/heads.hip (store and filter), the scored-candidate ranking of csrc/recommend.hip and
gnnrec.recs.recommend(head=...).  The reference for values and lists is ops.edge_mlp over
the expanded pair list — the per-edge kernel, not the code under test — and
recommend_cases.ranked() of that matrix: every score must carry the same bits, every list
must be the exhaustive ranking.  tests/test_recommend_mlp_cpu.py shows on the host that the
inputs keep every candidate count far under the cap, which the tests here assert as
overflow_rows == 0."""
import functools

import numpy as np
import pytest
import torch

import golden_io
import recommend_cases as rc
import recommend_mlp_cases as mc

pytestmark = pytest.mark.gpu


def _cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@functools.lru_cache(maxsize=None)
def _head(d, saturated=False):
    return (mc.saturated_head(d) if saturated else mc.head(d)).cuda()


def _tail(pl):
    return (pl.hidden_2.weight, pl.hidden_2.bias, pl.output.weight.reshape(-1), pl.output.bias)


def _PQ(pl, hu, hi):
    from gnnrec import ops
    d = hu.shape[1]
    W1 = pl.hidden_1.weight
    return (ops.gemm(_cu(hu), W1[:, :d], bias=pl.hidden_1.bias), ops.gemm(_cu(hi), W1[:, d:]))


def _edge_mlp_matrix(pl, P, Q):
    """score(u, v) for every pair: ops.edge_mlp over the expanded pair list, the definition."""
    from gnnrec import ops
    U, n = P.shape[0], Q.shape[0]
    src = torch.arange(U, device="cuda").repeat_interleave(n)
    dst = torch.arange(n, device="cuda").repeat(U)
    return ops.edge_mlp(src, dst, P, Q, *_tail(pl)).view(U, n)


@functools.lru_cache(maxsize=None)
def _case(kind, d, saturated=False):
    hu, hi = rc.tables(kind, d)
    pl = _head(d, saturated)
    S = _edge_mlp_matrix(pl, *_PQ(pl, hu, hi)).cpu().numpy()
    S.setflags(write=False)
    return hu, hi, S


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _recommend(pl, hu, hi, k, rows=None, excl=None, **kw):
    from gnnrec import recs
    kw.setdefault("sample", rc.SAMPLE)
    kw.setdefault("cand_cap", rc.CAND_CAP)
    ex = None if excl is None else (_cu(excl[0]), _cu(excl[1]))
    idx, vals, stats = recs.recommend(_cu(hu), _cu(hi), k, None if rows is None else _cu(rows),
                                      ex, return_stats=True, head=pl, **kw)
    assert idx.dtype == torch.int64 and vals.dtype == torch.float32 and idx.is_cuda
    return idx.cpu().numpy(), vals.cpu().numpy(), stats


def _assert_exact(idx, vals, S, excl, k, rows=None):
    ip, ix = excl if excl is not None else (None, None)
    ref_i, ref_v = rc.ranked(S if rows is None else S[rows], ip, ix, k, rows)
    np.testing.assert_array_equal(idx, ref_i)
    np.testing.assert_array_equal(_bits(vals), _bits(ref_v))  # bitwise


# ---------------------------------------------------------------- 1. store
@functools.lru_cache(maxsize=None)
def _kernel_case():
    """P, Q of the 130 x 5000 'normal' tables at d = 64 and their edge_mlp matrix."""
    hu, hi = rc.tables("normal", 64)
    pl = _head(64)
    P, Q = _PQ(pl, hu, hi)
    return pl, P, Q, _edge_mlp_matrix(pl, P, Q)


@pytest.mark.parametrize("n_users", mc.STORE_USERS)
def test_store_is_bitwise_edge_mlp(n_users):
    """Every ragged edge of the 32-item tile and of the user group (one below, one above, and
    130 = two groups and two users), against the per-edge kernel's bits; written through a
    row stride wider than the item range, the columns past it untouched."""
    from gnnrec import ops
    pl, P, Q, S = _kernel_case()
    for n_items in mc.STORE_ITEMS:
        ref = S[:n_users, :n_items].cpu().numpy()
        got = ops.edge_mlp_dense_store(P[:n_users], Q[:n_items], *_tail(pl))
        assert tuple(got.shape) == (n_users, n_items)
        np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(ref))
        wide = torch.full((n_users, n_items + 5), -7.0, device="cuda")
        ops.edge_mlp_dense_store(P[:n_users], Q[:n_items], *_tail(pl), out=wide[:, :n_items])
        np.testing.assert_array_equal(_bits(wide[:, :n_items].cpu().numpy()), _bits(ref))
        assert (wide[:, n_items:] == -7.0).all()


# ---------------------------------------------------------------- 2. filter
def _filter_tau(S, seed):
    """Per row the value at a rank drawn from [0, 150) of its sorted scores (so counts spread
    around the small caps); row 0 -inf (keeps everything), the last row +inf (keeps nothing)."""
    rng = np.random.default_rng(seed)
    srt = -np.sort(-S, axis=1)
    rank = rng.integers(0, min(150, S.shape[1]), S.shape[0])
    tau = srt[np.arange(S.shape[0]), rank].astype(np.float32)
    tau[0] = -np.inf
    tau[-1] = np.inf
    return tau


@pytest.mark.parametrize("cap", mc.FILTER_CAPS)
@pytest.mark.parametrize("B,n", [(130, 5000), (65, 257)])
def test_filter_keeps_exactly_the_expected_set(B, n, cap):
    """The kept set is {v : S[u, v] >= tau[u]} — no band: the comparison is on the bits the
    store writes — with each stored score S[u, v] bitwise; counts counts past cap; nothing is
    written past a row's min(count, cap) slots or past the buffers (guard fill).  The last
    user row and the last item are both off a tile boundary."""
    from gnnrec import ops
    pl, P, Q, S = _kernel_case()
    S = S[:B, :n].cpu().numpy()
    tau = _filter_tau(S, [B, n])
    guard = 4096
    ibuf = torch.full((B * cap + guard,), -7, dtype=torch.int32, device="cuda")
    sbuf = torch.full((B * cap + guard,), -7.0, dtype=torch.float32, device="cuda")
    counts = torch.zeros(B, dtype=torch.int32, device="cuda")
    ops.edge_mlp_dense_filter(P[:B], Q[:n], *_tail(pl), _cu(tau), counts,
                              ibuf[:B * cap].view(B, cap), sbuf[:B * cap].view(B, cap))
    torch.cuda.synchronize()
    assert (ibuf[B * cap:] == -7).all() and (sbuf[B * cap:] == -7.0).all()
    keep = S >= tau[:, None]
    cnt = counts.cpu().numpy()
    np.testing.assert_array_equal(cnt, keep.sum(1))
    assert cnt[0] == n and cnt[-1] == 0
    ci = ibuf[:B * cap].view(B, cap).cpu().numpy()
    cs = sbuf[:B * cap].view(B, cap).cpu().numpy()
    for u in range(B):
        m = min(int(cnt[u]), cap)
        ids = ci[u, :m]
        assert np.unique(ids).size == m and keep[u, ids].all(), u
        if cnt[u] <= cap:
            np.testing.assert_array_equal(np.sort(ids), np.nonzero(keep[u])[0])
        np.testing.assert_array_equal(_bits(cs[u, :m]), _bits(S[u, ids]))
        assert (ci[u, m:] == -7).all() and (cs[u, m:] == -7.0).all(), u
    assert (cnt > cap).any() == (n > cap) and (cnt <= cap).any()  # both sides of the cap


# ---------------------------------------------------------------- 3. ranking
def _scored_lists(cap, k, n_users):
    """Hand-made candidate rows: count 0, < k, = cap and > cap, equal scores, an exclusion
    list longer than one staging chunk (2048) whose hits lie in both chunks, and a row whose
    candidates are all excluded.  -> (counts, items, scores, exclusion lists per user)."""
    rng = np.random.default_rng(5)
    n_items = 9000
    counts = np.array([0, 5, cap, cap + 3, 40, 12, 33], np.int32)
    B = counts.size
    items = np.full((B, cap), -7, np.int32)
    scores = np.full((B, cap), -7.0, np.float32)
    for r in range(B):
        m = min(int(counts[r]), cap)
        items[r, :m] = rng.choice(n_items, m, replace=False)       # shuffled slot order
        scores[r, :m] = rng.integers(0, 6, m).astype(np.float32) / 8  # many equal scores
    excl = [rng.choice(n_items, int(rng.integers(0, 30)), replace=False).astype(np.int32)
            for _ in range(n_users)]
    return counts, items, scores, excl


def _ranked_lists(counts, items, scores, excl, users, cap, k):
    idx = np.full((counts.size, k), -9, np.int64)
    vals = np.full((counts.size, k), -9.0, np.float32)
    for r in range(counts.size):
        if counts[r] > cap:
            continue  # left untouched
        it, sc = items[r, :counts[r]], scores[r, :counts[r]]
        ok = ~np.isin(it, excl[users[r]]) if excl is not None else np.ones(it.size, bool)
        it, sc = it[ok], sc[ok]
        order = np.lexsort((it, -sc))[:k]
        idx[r], vals[r] = -1, -np.inf
        idx[r, :order.size] = it[order]
        vals[r, :order.size] = sc[order]
    return idx, vals


@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("with_excl", [False, True])
def test_scored_candidates_ranking(with_rows, with_excl):
    from gnnrec import ops
    cap, k, n_users = 64, 10, 9
    counts, items, scores, excl = _scored_lists(cap, k, n_users)
    B = counts.size
    users = np.array([3, 8, 0, 1, 3, 5, 7], np.int64) if with_rows else np.arange(B)
    # the user of row 4: a list of 3000 ids, its candidates' hits in both staging chunks
    long = np.setdiff1d(np.arange(20000, 23000), items[4]).astype(np.int32)[:2990]
    long = np.concatenate([long[:100], items[4, :3], long[100:2500], items[4, 20:24], long[2500:]])
    assert long.size > 2048 + 400
    excl[int(users[4])] = long
    excl[int(users[5])] = np.concatenate([items[5, :12][::-1], [1, 2]]).astype(np.int32)  # all
    ip, ix = rc.csr(excl)
    out_v = torch.full((B, k), -9.0, device="cuda")
    out_i = torch.full((B, k), -9, dtype=torch.int64, device="cuda")
    ops.topk_scored_candidates(_cu(counts), _cu(items), _cu(scores), k,
                               _cu(users) if with_rows else None,
                               _cu(ip) if with_excl else None, _cu(ix) if with_excl else None,
                               out_v, out_i)
    ref_i, ref_v = _ranked_lists(counts, items, scores, excl if with_excl else None, users, cap, k)
    np.testing.assert_array_equal(out_i.cpu().numpy(), ref_i)
    np.testing.assert_array_equal(_bits(out_v.cpu().numpy()), _bits(ref_v))
    assert (ref_i[0] == -1).all() and (ref_i[3] == -9).all() and (ref_i[1, 5:] == -1).all()
    if with_excl:
        assert (ref_i[5] == -1).all() and np.isneginf(ref_v[5]).all()
        assert not set(ref_i[4].tolist()) & set(long.tolist())
    # equal scores: the lower id first
    full = ref_i[2]
    same = ref_v[2][:-1] == ref_v[2][1:]
    assert same.any() and (full[:-1][same] < full[1:][same]).all()


# ---------------------------------------------------------------- 4. the result
@pytest.mark.parametrize("k", mc.KS)
@pytest.mark.parametrize("d", mc.DIMS)
@pytest.mark.parametrize("kind", mc.KINDS)
def test_recommend_head_is_the_exhaustive_ranking(kind, d, k):
    hu, hi, S = _case(kind, d)
    excl = rc.exclusions()
    idx, vals, stats = _recommend(_head(d), hu, hi, k, excl=excl)
    print(stats)
    assert stats["fast_path"] and stats["overflow_rows"] == 0
    assert k <= stats["candidates_max"] <= rc.CAND_CAP
    assert set(stats) == {"candidates_mean", "candidates_max", "overflow_rows", "sample",
                          "cand_cap", "fast_path"}
    _assert_exact(idx, vals, S, excl, k)


def test_recommend_head_user_rows():
    """A permuted subset with a repeated user, in two batches."""
    hu, hi, S = _case("relu", 128)
    excl = rc.exclusions()
    rows = np.random.default_rng(7).permutation(rc.N_USERS)[:77].astype(np.int64)
    rows[40] = rows[3]
    idx, vals, stats = _recommend(_head(128), hu, hi, 10, rows, excl, batch_size=50)
    assert stats["overflow_rows"] == 0
    _assert_exact(idx, vals, S, excl, 10, rows)
    np.testing.assert_array_equal(idx[40], idx[3])


def test_recommend_head_without_exclusions():
    hu, hi, S = _case("normal", 64)
    idx, vals, stats = _recommend(_head(64), hu, hi, 10)
    assert stats["overflow_rows"] == 0
    _assert_exact(idx, vals, S, None, 10)


@pytest.mark.parametrize("batch_size", [1, 64, 130, 8192])
def test_recommend_head_batch_sizes(batch_size):
    hu, hi, S = _case("lowrank", 16)
    excl = rc.exclusions()
    idx, vals, stats = _recommend(_head(16), hu, hi, 10, excl=excl, batch_size=batch_size)
    assert stats["fast_path"] and stats["overflow_rows"] == 0
    _assert_exact(idx, vals, S, excl, 10)


def test_recommend_head_deterministic():
    hu, hi, _ = _case("relu", 64)
    excl = rc.exclusions()
    a = _recommend(_head(64), hu, hi, 64, excl=excl)
    b = _recommend(_head(64), hu, hi, 64, excl=excl)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(_bits(a[1]), _bits(b[1]))


def test_head_none_is_the_cosine_ranking():
    """head=None: the cosine path, the same tensors as a call without the argument."""
    from gnnrec import recs
    hu, hi = rc.tables("normal", 64)
    a = recs.recommend(_cu(hu), _cu(hi), 10, sample=rc.SAMPLE)
    b = recs.recommend(_cu(hu), _cu(hi), 10, sample=rc.SAMPLE, head=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------- 5. other routes
def test_head_k_above_the_fast_path():
    hu, hi, S = _case("normal", 64)
    excl = rc.exclusions()
    idx, vals, stats = _recommend(_head(64), hu[:20], hi, 300, excl=(excl[0][:21], excl[1]))
    assert not stats["fast_path"]
    _assert_exact(idx, vals, S[:20], excl, 300)


@pytest.mark.parametrize("n_items", [1, 5])
def test_head_items_below_k(n_items):
    hu, hi, S = _case("normal", 16)
    excl = rc.exclusions(16, n_items, 0, n_items, seed=3)
    idx, vals, _ = _recommend(_head(16), hu[:16], hi[:n_items], 10, excl=excl)
    _assert_exact(idx, vals, S[:16, :n_items], excl, 10)
    assert (idx[:, n_items:] == -1).all() and np.isneginf(vals[:, n_items:]).all()


def test_head_sample_below_k_overflows_every_row():
    """A 4-item prefix holds fewer than k items: tau = -inf keeps all 600 items, over a cap of
    256 every row overflows and is recomputed exhaustively."""
    hu, hi, S = _case("normal", 16)
    excl = rc.exclusions(16, 600, 0, 20, seed=3)
    idx, vals, stats = _recommend(_head(16), hu[:16], hi[:600], 10, excl=excl, sample=4,
                                  cand_cap=256)
    assert stats["fast_path"] and stats["overflow_rows"] == 16 and stats["candidates_max"] == 600
    _assert_exact(idx, vals, S[:16, :600], excl, 10)


def test_saturated_head_overflows():
    """Most scores are exactly 1.0f: the k-th best of the prefix is 1.0f, thousands of items
    tie with it, the rows overflow the cap and the exhaustive route ranks the ties by id."""
    hu, hi, S = _case("normal", 16, True)
    assert (S == 1.0).mean() > 0.9 and ((S == 1.0).sum(1) > rc.CAND_CAP).all()
    excl = rc.exclusions()
    idx, vals, stats = _recommend(_head(16, True), hu, hi, 10, excl=excl)
    assert stats["fast_path"] and stats["overflow_rows"] > 0
    assert stats["candidates_max"] > rc.CAND_CAP
    _assert_exact(idx, vals, S, excl, 10)
    assert (vals == 1.0).all()


def test_head_no_users():
    hu, hi, _ = _case("normal", 16)
    idx, vals, stats = _recommend(_head(16), hu, hi, 10, np.zeros(0, np.int64), rc.exclusions())
    assert tuple(idx.shape) == (0, 10) and tuple(vals.shape) == (0, 10)
    assert stats["overflow_rows"] == 0


def test_head_user_with_everything_excluded():
    hu, hi, S = _case("normal", 64)
    ip, ix = rc.exclusions()
    lists = [ix[ip[u]:ip[u + 1]] for u in range(rc.N_USERS)]
    keep3 = np.array([17, 2600, 4999])
    lists[1] = np.setdiff1d(np.arange(rc.N_ITEMS), keep3).astype(np.int32)   # all but 3
    lists[2] = np.arange(rc.N_ITEMS, dtype=np.int32)[::-1]                    # everything
    excl = rc.csr(lists)
    idx, vals, stats = _recommend(_head(64), hu, hi, 10, excl=excl)
    _assert_exact(idx, vals, S, excl, 10)
    assert sorted(idx[1, :3].tolist()) == keep3.tolist() and (idx[1, 3:] == -1).all()
    assert (idx[2] == -1).all() and np.isneginf(vals[2]).all()
    assert stats["overflow_rows"] >= 1  # a -inf threshold keeps every item


# ---------------------------------------------------------------- 6. the reference
def _assert_same_ranking(got, ref, scores, tol, msg):
    """got == ref item for item, except swaps among items whose reference ratings are
    within `tol` relative of each other (tests/test_recs.py's rule, restated)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, msg
    bad = np.nonzero(got != ref)[0]
    if bad.size == 0:
        return
    assert sorted(got[bad].tolist()) == sorted(ref[bad].tolist()), msg
    for j in bad:
        a, b = float(scores[got[j]]), float(scores[ref[j]])
        assert abs(a - b) <= tol * max(abs(a), abs(b)), f"{msg}: rank {j} {got[j]} vs {ref[j]}"


def _lists(users, items, n_users):
    out = [[] for _ in range(n_users)]
    for u, i in zip(np.asarray(users).tolist(), np.asarray(items).tolist()):
        out[u].append(i)
    return out


def _model(pl):
    model = type("M", (), {})()
    model.pred_fn = type("P", (), {})()
    model.pred_fn.layer_nn = pl
    return model


@pytest.mark.parametrize("name", ["recs_nn", "recs_nn_k100"])
def test_recommend_head_matches_reference(name):
    from gnnrec.nn import PredictingLayer
    from gnnrec.recs import create_ground_truth, get_recs
    meta = golden_io.manifest()[name]
    a = golden_io.load(name)
    assert meta["pred"] == "nn" and not meta["use_popularity"]
    pl = PredictingLayer(meta["embed_dim"])
    pl.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in a.items() if k.startswith("w/")})
    pl = pl.cuda().eval()
    bought = _lists(a["bought/u"], a["bought/i"], a["h/user"].shape[0])
    idx, _, stats = _recommend(pl, a["h/user"], a["h/item"], meta["k"], a["user_ids"],
                               rc.csr(bought))
    assert stats["fast_path"]
    h = {"user": _cu(a["h/user"]), "item": _cu(a["h/item"])}
    with torch.no_grad():
        recs = get_recs(None, h, _model(pl), meta["embed_dim"], meta["k"], a["user_ids"].tolist(),
                        create_ground_truth(a["bought/u"], a["bought/i"]), pred="nn", batch_size=7)
    for r, (u, ref, s) in enumerate(zip(a["user_ids"], a["recs"], a["scores"])):
        ref = ref[ref >= 0]
        got = idx[r][idx[r] >= 0]
        _assert_same_ranking(got, ref, s, meta["min_rel_gap_required"], f"user {u}")
        assert not set(got.tolist()) & set(bought[int(u)])
        np.testing.assert_array_equal(got, recs[int(u)])


# ---------------------------------------------------------------- 7. the graph entry
def test_recommend_for_graph_head_equals_get_recs():
    from gnnrec.graph import HeteroGraph
    from gnnrec.recs import create_ground_truth, get_recs, recommend_for_graph
    rng = np.random.default_rng(3)
    n_u, n_i, E = 120, 80, 900
    u, i = rng.integers(0, n_u, E), rng.integers(0, n_i, E)
    edges = {("user", "buys", "item"): (u, i), ("item", "bought-by", "user"): (i, u)}
    g = HeteroGraph({ce: (torch.from_numpy(s), torch.from_numpy(d)) for ce, (s, d) in edges.items()},
                    {"user": n_u, "item": n_i}).to("cuda")
    h = {"user": _cu(rng.standard_normal((n_u, 16)).astype(np.float32)),
         "item": _cu(rng.standard_normal((n_i, 16)).astype(np.float32))}
    pl = _head(16)
    users = [0, 5, 7, 119, 64, 33]
    with torch.no_grad():
        ref = get_recs(g, h, _model(pl), 16, 5, users, create_ground_truth(u, i), pred="nn")
    idx, vals = recommend_for_graph(g, h, 5, users, head=pl)
    for r, user in enumerate(users):
        np.testing.assert_array_equal(idx[r].cpu().numpy(), ref[user])
    idx_all, _ = recommend_for_graph(g, h, 5, head=pl)
    assert tuple(idx_all.shape) == (n_u, 5)
    np.testing.assert_array_equal(idx_all[users].cpu().numpy(), idx.cpu().numpy())


# ---------------------------------------------------------------- 8. refusals
def test_refusals():
    """Each raises before any launch."""
    from gnnrec import ops, recs
    pl, P, Q, _ = _kernel_case()
    tail = _tail(pl)
    B = 4
    buf = torch.zeros(B * 128 + 4, device="cuda")
    skew = buf[1:1 + B * 128].view(B, 128)  # contiguous, 4 bytes off a 16-byte boundary
    assert skew.is_contiguous() and skew.data_ptr() % 16 == 4
    tau = torch.zeros(B, device="cuda")
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    ci = torch.zeros((B, 8), dtype=torch.int32, device="cuda")
    cs = torch.zeros((B, 8), device="cuda")
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.edge_mlp_dense_store(skew, Q[:9], *tail)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.edge_mlp_dense_filter(skew, Q[:9], *tail, tau, cnt, ci, cs)
    bad_w2 = torch.zeros((32, 64), device="cuda")
    with pytest.raises(ValueError, match="128/32 hidden sizes"):
        ops.edge_mlp_dense_store(P[:B], Q[:9], bad_w2, *tail[1:])
    with pytest.raises(ValueError, match="128/32 hidden sizes"):
        ops.edge_mlp_dense_filter(P[:B], Q[:9], bad_w2, *tail[1:], tau, cnt, ci, cs)
    for cap in (0, 4097):
        with pytest.raises(ValueError, match="cap must be"):
            ops.edge_mlp_dense_filter(P[:B], Q[:9], *tail, tau, cnt,
                                      torch.zeros((B, cap), dtype=torch.int32, device="cuda"),
                                      torch.zeros((B, cap), device="cuda"))
        with pytest.raises(ValueError, match="cap must be"):
            ops.topk_scored_candidates(cnt, torch.zeros((B, cap), dtype=torch.int32, device="cuda"),
                                       torch.zeros((B, cap), device="cuda"), 1)
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.edge_mlp_dense_store(P[:B].cpu(), Q[:9], *tail)
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.edge_mlp_dense_filter(P[:B], Q[:9], *tail, tau.cpu(), cnt, ci, cs)
    with pytest.raises(ValueError, match="HIP device tensor"):
        recs.recommend(torch.zeros(4, 64), Q[:9, :64].contiguous(), 3, head=pl)
    assert (cnt == 0).all() and (ci == 0).all()
