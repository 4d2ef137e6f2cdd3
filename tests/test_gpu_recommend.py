"""GPU checks of the bf16-prefiltered exact top-k (gnnrec.recs.recommend and the kernels of
csrc/recommend.hip): the lists and values must be those of an exhaustive ranking of
ops.sddmm_cos scores, bit for bit, whatever the filter kept.  Inputs come from
tests/recommend_cases.py; tests/test_recommend_cpu.py shows on the CPU that they keep every
candidate count under the cap, which the tests here assert as overflow_rows == 0."""
import functools

import numpy as np
import pytest
import torch

import golden_io
import recommend_cases as rc

pytestmark = pytest.mark.gpu


def _cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _scores(hu, hi):
    """score(u, v) for every pair: ops.sddmm_cos, the definition."""
    from gnnrec import ops
    U, n = hu.shape[0], hi.shape[0]
    src = torch.arange(U, device="cuda").repeat_interleave(n)
    dst = torch.arange(n, device="cuda").repeat(U)
    return ops.sddmm_cos(src, dst, _cu(hu), _cu(hi)).view(U, n).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(kind, d):
    hu, hi = rc.tables(kind, d)
    return hu, hi, _scores(hu, hi)


def _recommend(hu, hi, k, rows=None, excl=None, **kw):
    from gnnrec import recs
    kw.setdefault("sample", rc.SAMPLE)
    kw.setdefault("cand_cap", rc.CAND_CAP)
    ex = None if excl is None else (_cu(excl[0]), _cu(excl[1]))
    idx, vals, stats = recs.recommend(_cu(hu), _cu(hi), k, None if rows is None else _cu(rows),
                                      ex, return_stats=True, **kw)
    assert idx.dtype == torch.int64 and vals.dtype == torch.float32 and idx.is_cuda
    return idx.cpu().numpy(), vals.cpu().numpy(), stats


def _assert_exact(idx, vals, S, excl, k, rows=None):
    ip, ix = excl if excl is not None else (None, None)
    ref_i, ref_v = rc.ranked(S if rows is None else S[rows], ip, ix, k, rows)
    np.testing.assert_array_equal(idx, ref_i)
    np.testing.assert_array_equal(vals.view(np.int32), ref_v.view(np.int32))  # bitwise


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("d", [16, 100, 128])
def test_normalize_rows_bf16(d):
    from gnnrec import ops
    rng = np.random.default_rng(d)
    x = rng.standard_normal((37, d)).astype(np.float32) * 3
    x[5] = 0
    rmap = np.array([36, 5, 0, 0, 17, 5, 36], np.int64)
    dpad = (d + 31) // 32 * 32
    x64 = x.astype(np.float64)
    want = x64 / np.maximum(np.linalg.norm(x64, axis=1, keepdims=True), 1e-12)
    for m in (None, rmap):
        out = ops.normalize_rows_bf16(_cu(x), None if m is None else _cu(m))
        w = want if m is None else want[m]
        assert out.dtype == torch.bfloat16 and tuple(out.shape) == (w.shape[0], dpad)
        got = out.float().cpu().numpy().astype(np.float64)
        assert (got[:, d:] == 0).all()
        assert (np.abs(got[:, :d] - w) <= (2.0 ** -8 + 2.0 ** -20) * np.abs(w)).all()
        assert (got[5 if m is None else 1] == 0).all()


@pytest.mark.parametrize("d", [16, 64, 80, 128, 160])
def test_store_mode_matches_bf16_matmul(d):
    """Every ragged edge of the 128 x 128 block tile, the 64 x 64 wave tile and the 32 x 32
    MFMA tile (129: one row or column in a second block tile), in every form of the kernel:
    the slab kernel at dpad 32, 64 and 128, and the one that loads its operands directly at
    dpad 96 (d = 80) and dpad > 128 (d = 160)."""
    from gnnrec import ops
    hu, hi = rc.tables("normal", d, 130, 4097, seed=3)
    ub, vb = ops.normalize_rows_bf16(_cu(hu)), ops.normalize_rows_bf16(_cu(hi))
    uf, vf = ub.float().cpu(), vb.float().cpu()
    for B in (1, 33, 129, 130):
        for n in (1, 31, 129, 1000, 4097):
            got = ops.score_bf16_store(ub[:B].contiguous(), vb[:n].contiguous()).cpu()
            torch.testing.assert_close(got, uf[:B] @ vf[:n].T, rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------- the result
@pytest.mark.parametrize("k", rc.KS)
@pytest.mark.parametrize("d", rc.DIMS)
@pytest.mark.parametrize("kind", rc.KINDS)
def test_recommend_is_the_exhaustive_ranking(kind, d, k):
    hu, hi, S = _case(kind, d)
    excl = rc.exclusions()
    idx, vals, stats = _recommend(hu, hi, k, excl=excl)
    print(stats)
    assert stats["fast_path"] and stats["overflow_rows"] == 0
    assert 0 < stats["candidates_max"] <= rc.CAND_CAP
    _assert_exact(idx, vals, S, excl, k)


@pytest.mark.parametrize("kind,d", [("normal", 16), ("relu", 128)])
def test_recommend_user_rows(kind, d):
    """A permuted subset with a repeated user, in two batches."""
    hu, hi, S = _case(kind, d)
    excl = rc.exclusions()
    rows = np.random.default_rng(7).permutation(rc.N_USERS)[:77].astype(np.int64)
    rows[40] = rows[3]
    idx, vals, stats = _recommend(hu, hi, 10, rows, excl, batch_size=50)
    assert stats["overflow_rows"] == 0
    _assert_exact(idx, vals, S, excl, 10, rows)
    np.testing.assert_array_equal(idx[40], idx[3])


def test_recommend_wide_rows():
    """dpad > 128: the scoring kernel without the register-resident item slab."""
    hu, hi, S = _case("normal", rc.WIDE_D)
    excl = rc.exclusions()
    idx, vals, stats = _recommend(hu, hi, 10, excl=excl)
    assert stats["fast_path"] and stats["overflow_rows"] == 0
    _assert_exact(idx, vals, S, excl, 10)


def test_recommend_without_exclusions():
    hu, hi, S = _case("normal", 64)
    idx, vals, stats = _recommend(hu, hi, 10)
    assert stats["overflow_rows"] == 0
    _assert_exact(idx, vals, S, None, 10)


def test_ties_rank_by_item_id():
    hu, hi = rc.tables("normal", 64)
    hi = hi.copy()
    hi[2500:] = hi[:2500]
    S = _scores(hu, hi)
    np.testing.assert_array_equal(S[:, :2500].view(np.int32), S[:, 2500:].view(np.int32))
    idx, vals, stats = _recommend(hu, hi, 10)
    assert stats["overflow_rows"] == 0
    _assert_exact(idx, vals, S, None, 10)
    assert (idx[:, 0::2] < 2500).all()
    np.testing.assert_array_equal(idx[:, 1::2], idx[:, 0::2] + 2500)


def test_exclusion_extremes():
    hu, hi, S = _case("normal", 64)
    ip, ix = rc.exclusions()
    lists = [ix[ip[u]:ip[u + 1]] for u in range(rc.N_USERS)]
    lists[0] = np.argsort(-S[0], kind="stable")[:50].astype(np.int32)[::-1]  # its whole top 50
    keep3 = np.array([17, 2600, 4999])
    lists[1] = np.setdiff1d(np.arange(rc.N_ITEMS), keep3).astype(np.int32)   # all but 3
    lists[2] = np.arange(rc.N_ITEMS, dtype=np.int32)[::-1]                    # everything
    excl = rc.csr(lists)
    idx, vals, stats = _recommend(hu, hi, 10, excl=excl)
    _assert_exact(idx, vals, S, excl, 10)
    assert not set(idx[0].tolist()) & set(lists[0].tolist())
    assert sorted(idx[1, :3].tolist()) == keep3.tolist() and (idx[1, 3:] == -1).all()
    assert np.isneginf(vals[1, 3:]).all()
    assert (idx[2] == -1).all() and np.isneginf(vals[2]).all()
    assert stats["overflow_rows"] >= 1  # a -inf threshold keeps every item


def _collapsed(d=64):
    rng = np.random.default_rng(11)
    hu = rng.standard_normal((rc.N_USERS, d)).astype(np.float32)
    base = rng.standard_normal(d).astype(np.float32)
    hi = (base + 1e-3 * rng.standard_normal((rc.N_ITEMS, d))).astype(np.float32)
    return hu, hi


def test_collapsed_table_takes_the_fallback():
    hu, hi = _collapsed()
    S = _scores(hu, hi)
    idx, vals, stats = _recommend(hu, hi, 10, excl=rc.exclusions())
    assert stats["overflow_rows"] == rc.N_USERS and stats["candidates_max"] > rc.CAND_CAP
    _assert_exact(idx, vals, S, rc.exclusions(), 10)


@pytest.mark.parametrize("cap", [1, 64, 1024])
def test_filter_never_stores_past_the_cap(cap):
    """Every row overflows: the counters count on, the stores stay inside each row's cap
    slots (a guard region after cand_items, and every stored id a distinct item)."""
    from gnnrec import ops
    hu, hi = _collapsed()
    B, n, guard = rc.N_USERS, rc.N_ITEMS, 4096
    ub, vb = ops.normalize_rows_bf16(_cu(hu)), ops.normalize_rows_bf16(_cu(hi))
    a = ops.score_bf16_store(ub, vb)
    tau = a.max(dim=1).values.contiguous()
    want = (a >= (tau - 2 * torch.tensor(rc.EPS, dtype=torch.float32))[:, None]).sum(1).cpu()
    buf = torch.full((B * cap + guard,), -7, dtype=torch.int32, device="cuda")
    cand = buf[:B * cap].view(B, cap)
    counts = torch.zeros(B, dtype=torch.int32, device="cuda")
    ops.score_bf16_filter(ub, vb, tau, counts, cand)
    torch.cuda.synchronize()
    assert (buf[B * cap:] == -7).all()
    np.testing.assert_array_equal(counts.cpu().numpy(), want.numpy())
    assert (counts > cap).all()
    c = cand.cpu().numpy()
    assert ((c >= 0) & (c < n)).all()
    assert all(np.unique(r).size == cap for r in c)


def test_k_above_the_fast_path():
    hu, hi, S = _case("normal", 64)
    excl = rc.exclusions()
    idx, vals, stats = _recommend(hu[:20], hi, 300, excl=(excl[0][:21], excl[1]))
    assert not stats["fast_path"]
    _assert_exact(idx, vals, S[:20], excl, 300)


def test_deterministic():
    hu, hi, _ = _case("relu", 64)
    excl = rc.exclusions()
    a = _recommend(hu, hi, 64, excl=excl)
    b = _recommend(hu, hi, 64, excl=excl)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.int32), b[1].view(np.int32))


# ---------------------------------------------------------------- the reference
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


@pytest.mark.parametrize("name", ["recs_cos", "recs_cos_k100"])
def test_recommend_matches_reference(name):
    meta = golden_io.manifest()[name]
    a = golden_io.load(name)
    bought = _lists(a["bought/u"], a["bought/i"], a["h/user"].shape[0])
    idx, _, stats = _recommend(a["h/user"], a["h/item"], meta["k"], a["user_ids"],
                               rc.csr(bought))
    assert stats["fast_path"]
    for r, (u, ref, s) in enumerate(zip(a["user_ids"], a["recs"], a["scores"])):
        ref = ref[ref >= 0]
        got = idx[r][idx[r] >= 0]
        _assert_same_ranking(got, ref, s, meta["min_rel_gap_required"], f"user {u}")
        assert not set(got.tolist()) & set(bought[int(u)])


def test_recommend_for_graph_equals_get_recs():
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
    users = [0, 5, 7, 119, 64, 33]
    ref = get_recs(g, h, None, 16, 5, users, create_ground_truth(u, i))
    idx, vals = recommend_for_graph(g, h, 5, users)
    for r, user in enumerate(users):
        np.testing.assert_array_equal(idx[r].cpu().numpy(), ref[user])
    idx_all, _ = recommend_for_graph(g, h, 5)
    assert tuple(idx_all.shape) == (n_u, 5)
    np.testing.assert_array_equal(idx_all[users].cpu().numpy(), idx.cpu().numpy())


@pytest.mark.parametrize("name", sorted(k for k, v in golden_io.manifest().items()
                                        if v["kind"] == "recs"))
@pytest.mark.parametrize("dup", [False, True])
def test_recs_to_metrics_device(name, dup):
    from gnnrec.recs import create_ground_truth, recs_to_metrics, recs_to_metrics_device
    a = golden_io.load(name)
    n_users, n_items = a["h/user"].shape[0], a["h/item"].shape[0]
    gu, gi = a["gt/u"], a["gt/i"]
    if dup:  # the same purchase more than once: recall counts it every time
        gu, gi = np.concatenate([gu, gu[::3], gu[:5]]), np.concatenate([gi, gi[::3], gi[:5]])
    recs = {int(u): r[r >= 0] for u, r in zip(a["user_ids"], a["recs"])}

    class G:
        def num_nodes(self, nt):
            return n_items
    want = recs_to_metrics(recs, create_ground_truth(gu, gi), G())
    if not dup:
        np.testing.assert_allclose(want, a["metrics"], rtol=0, atol=0)
    ip, ix = rc.csr(_lists(gu, gi, n_users))
    got = recs_to_metrics_device(_cu(a["recs"]), _cu(a["user_ids"]), _cu(ip), _cu(ix), n_items)
    assert tuple(got) == tuple(want)
