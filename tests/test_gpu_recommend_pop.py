"""GPU checks of the popularity-weighted many-user top-k (gnnrec.recs.recommend with
popularity=, csrc/recommend_pop.hip, the rating epilogues of csrc/recommend.hip and
csrc/heads.hip): the lists and values are those of an exhaustive ranking of
the device's own rating matrix R = expf(score) / Z + p, bit for bit, whatever the filter
kept; the denominators Z match fp64 within a derived bound and have the same bits for any
batching.  Inputs and bounds come from tests/recommend_pop_cases.py;
tests/test_recommend_pop_cpu.py shows on the host that they keep every candidate count under
half the cap, which the tests here assert as overflow_rows == 0."""
import functools

import numpy as np
import pytest
import torch

import golden_io
import recommend_cases as rc
import recommend_mlp_cases as mc
import recommend_pop_cases as pc

pytestmark = pytest.mark.gpu

HEADS = ("cos", "mlp")
PERM = np.array([0, 2, 4, 6, 1, 3, 5, 7])   # normalize_rows_f32's order inside 8 columns


def _cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _kinds(head):
    return rc.KINDS if head == "cos" else mc.KINDS


def _unpermute(t, d):
    """normalize_rows_f32's table -> the plain [n, d] columns, float64."""
    x = t.cpu().numpy().astype(np.float64)
    out = np.empty_like(x)
    for s in range(0, x.shape[1], 8):
        out[:, s + PERM] = x[:, s:s + 8]
    assert (out[:, d:] == 0).all()
    return out[:, :d]


@functools.lru_cache(maxsize=None)
def _mlp_head(d):
    return mc.head(d).cuda()


@functools.lru_cache(maxsize=None)
def _case(head, kind, d):
    """(hu, hi, S, Z): the device's own score matrix and denominators (numpy)."""
    from gnnrec import ops, recs
    hu, hi = rc.tables(kind, d)
    U, n = hu.shape[0], hi.shape[0]
    if head == "cos":
        src = torch.arange(U, device="cuda").repeat_interleave(n)
        dst = torch.arange(n, device="cuda").repeat(U)
        S = ops.sddmm_cos(src, dst, _cu(hu), _cu(hi)).view(U, n)
        Z = ops.cos_denominators(ops.normalize_rows_f32(_cu(hu)), ops.normalize_rows_f32(_cu(hi)))
    else:
        with torch.no_grad():
            mlp = recs._MlpHead(_mlp_head(d), _cu(hu), _cu(hi))
            P = mlp.P(torch.arange(U, device="cuda"))
            S, Z = mlp.store(P), mlp.denominators(P)
    return hu, hi, S.cpu().numpy(), Z.cpu().numpy()


def _ratings(S, Z, p, rows=None):
    """The exhaustive path's rating matrix: ops.rating_rows_ of the score rows."""
    from gnnrec import ops
    if rows is not None:
        S, Z = S[rows], Z[rows]
    return ops.rating_rows_(_cu(S).clone(), _cu(Z), _cu(p)).cpu().numpy()


def _recommend(head, hu, hi, k, pop, w, rows=None, excl=None, **kw):
    from gnnrec import recs
    kw.setdefault("sample", pc.SAMPLE)
    kw.setdefault("cand_cap", pc.CAND_CAP)
    kw.setdefault("pop_sample", pc.POP_SAMPLE)
    ex = None if excl is None else (_cu(excl[0]), _cu(excl[1]))
    with torch.no_grad():
        idx, vals, stats = recs.recommend(
            _cu(hu), _cu(hi), k, None if rows is None else _cu(rows), ex, return_stats=True,
            head=None if head == "cos" else _mlp_head(hu.shape[1]), popularity=_cu(pop),
            weight_popularity=w, **kw)
    assert idx.dtype == torch.int64 and vals.dtype == torch.float32 and idx.is_cuda
    return idx.cpu().numpy(), vals.cpu().numpy(), stats


def _assert_exact(idx, vals, R, excl, k, rows=None):
    """R: the rating rows of the served users, in order."""
    ip, ix = excl if excl is not None else (None, None)
    ref_i, ref_v = rc.ranked(R, ip, ix, k, rows)
    np.testing.assert_array_equal(idx, ref_i)
    np.testing.assert_array_equal(vals.view(np.int32), ref_v.view(np.int32))  # bitwise


# ---------------------------------------------------------------- 1. denominators
@pytest.mark.parametrize("d", [16, 100, 128, 160])
def test_cos_denominators_against_fp64(d):
    """Z from the MFMA kernel against sum exp in fp64 over the float64 product of the
    device's own fp32-normalised tables: every ragged edge of the 128-user tile, the 32-item
    subtile and the 1024-item partial; d = 100 a short last k-chunk, 160 a second one."""
    from gnnrec import ops
    hu, hi = rc.tables("normal", d)
    un, vn = ops.normalize_rows_f32(_cu(hu)), ops.normalize_rows_f32(_cu(hi))
    assert tuple(un.shape) == (rc.N_USERS, (d + 7) // 8 * 8)
    u64, v64 = _unpermute(un, d), _unpermute(vn, d)
    x64 = hu.astype(np.float64)
    want = x64 / np.maximum(np.linalg.norm(x64, axis=1, keepdims=True), 1e-12)
    assert (np.abs(u64 - want) <= 2.0 ** -20 * np.abs(want)).all()
    worst = 0.0
    for n in pc.Z_ITEMS:
        E = np.exp(u64 @ v64[:n].T)
        for U in pc.Z_USERS:
            Z = ops.cos_denominators(un[:U].contiguous(), vn[:n].contiguous()).cpu().numpy()
            Z64 = E[:U].sum(1)
            rel = np.abs(Z - Z64) / Z64
            worst = max(worst, rel.max() / pc.z_rel_bound("cos", d, n))
            assert (rel <= pc.z_rel_bound("cos", d, n)).all(), (n, U, rel.max())
    print(f"d {d}: largest relative error / bound {worst:.3f}")


def test_mlp_denominators_against_fp64():
    from gnnrec import recs
    d = 64
    hu, hi = rc.tables("normal", d)
    worst = 0.0
    with torch.no_grad():
        for n in pc.Z_ITEMS:
            mlp = recs._MlpHead(_mlp_head(d), _cu(hu), _cu(hi[:n]))
            for U in pc.Z_USERS:
                P = mlp.P(torch.arange(U, device="cuda"))
                Z = mlp.denominators(P).cpu().numpy()
                Z64 = np.exp(mlp.store(P).cpu().numpy().astype(np.float64)).sum(1)
                rel = np.abs(Z - Z64) / Z64
                worst = max(worst, rel.max() / pc.z_rel_bound("mlp", d, n))
                assert (rel <= pc.z_rel_bound("mlp", d, n)).all(), (n, U, rel.max())
    print(f"largest relative error / bound {worst:.3f}")


def test_exp_rowsum_against_fp64():
    """The denominators of the widths the MFMA kernel does not take: 3 block-strides of 256
    columns and a ragged tail; chain 20 adds in a lane, 6 tree levels, 3 wave adds."""
    from gnnrec import ops
    S = np.random.default_rng(4).uniform(-1, 1, (37, 5000)).astype(np.float32)
    for n in (1, 255, 257, 5000):
        Z = ops.exp_rowsum(_cu(S[:, :n])).cpu().numpy()
        Z64 = np.exp(S[:, :n].astype(np.float64)).sum(1)
        assert (np.abs(Z - Z64) <= Z64 * (2.0 ** -22 + 29 * 2.0 ** -24)).all()


# ---------------------------------------------------------------- 2. invariance
@pytest.mark.parametrize("head", HEADS)
def test_denominators_are_invariant(head):
    """The same bits for a user row whatever the batch size, the order or repetition of the
    rows, and the run."""
    from gnnrec import ops, recs
    d = 64
    hu, hi, _, Z0 = _case(head, "normal", d)
    hu_c = _cu(hu)
    with torch.no_grad():
        if head == "cos":
            vn = ops.normalize_rows_f32(_cu(hi))
            zfn = lambda rows: ops.cos_denominators(ops.normalize_rows_f32(hu_c, rows), vn)
        else:
            mlp = recs._MlpHead(_mlp_head(d), hu_c, _cu(hi))
            zfn = lambda rows: mlp.denominators(mlp.P(rows))
        everyone = torch.arange(rc.N_USERS, device="cuda")
        for bs in pc.BATCHES:
            Z = torch.cat([zfn(everyone[b:b + bs]) for b in range(0, rc.N_USERS, bs)])
            np.testing.assert_array_equal(Z.cpu().numpy().view(np.int32), Z0.view(np.int32))
        rows = np.random.default_rng(7).permutation(rc.N_USERS)[:77].astype(np.int64)
        rows[40] = rows[3]
        for _ in range(2):
            Z = zfn(_cu(rows)).cpu().numpy()
            np.testing.assert_array_equal(Z.view(np.int32), Z0[rows].view(np.int32))


# ---------------------------------------------------------------- 3. stored ratings
@pytest.mark.parametrize("name", pc.POPS)
@pytest.mark.parametrize("head", HEADS)
def test_rating_matrix_against_fp64(head, name):
    """The exhaustive path's R against exp(score) / Z64 + p in fp64 (score: the device's own
    bits; Z64: the fp64 sum over them), and the fast path's vals the matrix's entries at the
    returned ids, bitwise.  For the cosine head Z's g is the MFMA product, not the score: the
    two differ by g's accumulation (at most d 2^-24 in nearest rounding, half of the bound's
    d 2^-23 term) plus the rounding of the normalised entries and of the score's own lane sums
    and divide (a few 2^-24 each, under the other half for d >= 16)."""
    d = 64
    hu, hi, S, Z = _case(head, "normal", d)
    pop, w = pc.popularity(name)
    p = pc.p_vector(pop, w)
    R = _ratings(S, Z, p)
    E = np.exp(S.astype(np.float64))
    Z64 = E.sum(1)
    zrel = pc.z_rel_bound(head, d, rc.N_ITEMS)
    assert (np.abs(Z - Z64) <= zrel * Z64).all()
    soft = E / Z64[:, None]
    R64 = soft + p.astype(np.float64)
    err, bound = np.abs(R - R64), pc.r_abs_bound(soft, R64, zrel)
    print(f"{head} {name}: largest error / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    idx, vals, stats = _recommend(head, hu, hi, 10, pop, w, excl=rc.exclusions())
    assert stats["fast_path"] and stats["overflow_rows"] == 0
    np.testing.assert_array_equal(vals.view(np.int32),
                                  np.take_along_axis(R, idx, 1).view(np.int32))


# ---------------------------------------------------------------- 4. the result
@pytest.mark.parametrize("k", rc.KS)
@pytest.mark.parametrize("d", rc.DIMS)
@pytest.mark.parametrize("head,kind", [(h, kd) for h in HEADS for kd in _kinds(h)])
def test_recommend_is_the_exhaustive_ranking(head, kind, d, k):
    hu, hi, S, Z = _case(head, kind, d)
    excl = rc.exclusions()
    for name in pc.POPS:
        pop, w = pc.popularity(name)
        idx, vals, stats = _recommend(head, hu, hi, k, pop, w, excl=excl)
        print(name, stats)
        assert stats["fast_path"] and stats["overflow_rows"] == 0
        assert 0 < stats["candidates_max"] <= pc.CAND_CAP // 2
        assert stats["pop_sample"] == pc.POP_SAMPLE and stats["sample"] == pc.SAMPLE
        _assert_exact(idx, vals, _ratings(S, Z, pc.p_vector(pop, w)), excl, k)


@pytest.mark.parametrize("name", pc.POPS)
@pytest.mark.parametrize("head,kind,d", [("cos", "normal", 16), ("cos", "relu", 128),
                                         ("mlp", "lowrank", 64)])
def test_recommend_rows_batches_and_no_exclusions(head, kind, d, name):
    """Without exclusions; a permuted subset with a repeated user; the four batch sizes."""
    hu, hi, S, Z = _case(head, kind, d)
    pop, w = pc.popularity(name)
    p = pc.p_vector(pop, w)
    R = _ratings(S, Z, p)
    idx, vals, stats = _recommend(head, hu, hi, 10, pop, w)
    assert stats["overflow_rows"] == 0
    _assert_exact(idx, vals, R, None, 10)
    excl = rc.exclusions()
    rows = np.random.default_rng(7).permutation(rc.N_USERS)[:77].astype(np.int64)
    rows[40] = rows[3]
    ref = None
    for bs in pc.BATCHES:
        idx, vals, stats = _recommend(head, hu, hi, 10, pop, w, rows, excl, batch_size=bs)
        assert stats["overflow_rows"] == 0
        if ref is None:
            _assert_exact(idx, vals, R[rows], excl, 10, rows)
            np.testing.assert_array_equal(idx[40], idx[3])
            ref = idx, vals
        np.testing.assert_array_equal(idx, ref[0])
        np.testing.assert_array_equal(vals.view(np.int32), ref[1].view(np.int32))


# ---------------------------------------------------------------- 5. the epilogues alone
def _thresholds(Ra, seed):
    """Per-row thresholds at random quantiles of the row's own ratings; row 0 -inf (keeps
    everything), the last row +inf (nothing)."""
    q = np.random.default_rng(seed).uniform(0.3, 0.999, Ra.shape[0])
    thr = np.array([np.quantile(r, x) for r, x in zip(Ra, q)], np.float32)
    thr[0], thr[-1] = -np.inf, np.inf
    return thr


def _check_kept(counts, cand, keep, cap, guard_ok):
    assert guard_ok
    np.testing.assert_array_equal(counts, keep.sum(1))
    for r in range(keep.shape[0]):
        got = cand[r, :min(counts[r], cap)]
        want = np.nonzero(keep[r])[0]
        assert np.unique(got).size == got.size and np.isin(got, want).all()
        if counts[r] <= cap:
            np.testing.assert_array_equal(np.sort(got), want)


@pytest.mark.parametrize("cap", [1, 64, 4096])
@pytest.mark.parametrize("B,n", [(130, 5000), (65, 257)])
@pytest.mark.parametrize("d", [64, 128, 160])
def test_cos_rating_epilogues(d, B, n, cap):
    """STORE-R is rating() of the plain store's approximate score (against fp64 within the
    rounding of its three operations); FILTER-R keeps exactly the pairs whose stored Ra is >=
    the threshold — the same a and the same rating(), so no band is needed here — counting
    past the cap and storing inside it."""
    from gnnrec import ops
    hu, hi = rc.tables("normal", d)
    pop, w = pc.popularity("dense", n)
    p = pc.p_vector(pop, w)
    ub = ops.normalize_rows_bf16(_cu(hu[:B]))
    vb = ops.normalize_rows_bf16(_cu(hi[:n]))
    Z = ops.cos_denominators(ops.normalize_rows_f32(_cu(hu[:B])),
                             ops.normalize_rows_f32(_cu(hi[:n])))
    a = ops.score_bf16_store(ub, vb).cpu().numpy().astype(np.float64)
    Ra = ops.score_bf16_store_rating(ub, vb, Z, _cu(p)).cpu().numpy()
    soft = np.exp(a) / Z.cpu().numpy().astype(np.float64)[:, None]
    Ra64 = soft + p.astype(np.float64)
    assert (np.abs(Ra - Ra64) <= pc.r_abs_bound(soft, Ra64, 0.0)).all()
    thr = _thresholds(Ra, d + B + cap)
    guard = 4096
    buf = torch.full((B * cap + guard,), -7, dtype=torch.int32, device="cuda")
    cand = buf[:B * cap].view(B, cap)
    counts = torch.zeros(B, dtype=torch.int32, device="cuda")
    ops.score_bf16_filter_rating(ub, vb, Z, _cu(p), _cu(thr), counts, cand)
    torch.cuda.synchronize()
    _check_kept(counts.cpu().numpy(), cand.cpu().numpy(), Ra >= thr[:, None], cap,
                bool((buf[B * cap:] == -7).all()))


@pytest.mark.parametrize("cap", [1, 64, 4096])
@pytest.mark.parametrize("B,n", [(130, 5000), (65, 257)])
def test_mlp_rating_epilogues(B, n, cap):
    """STORE_R is rating() of the dense store's score; FILTER_R keeps exactly the pairs with
    R >= tau, with their R."""
    from gnnrec import ops, recs
    d = 64
    hu, hi = rc.tables("normal", d)
    pop, w = pc.popularity("dense", n)
    p = pc.p_vector(pop, w)
    with torch.no_grad():
        mlp = recs._MlpHead(_mlp_head(d), _cu(hu[:B]), _cu(hi[:n]))
        P = mlp.P(torch.arange(B, device="cuda"))
        Z = mlp.denominators(P)
        S = mlp.store(P)
        R = mlp.store_rating(P, mlp.Q, Z, _cu(p))
        want = ops.rating_rows_(S.clone(), Z, _cu(p))
        np.testing.assert_array_equal(R.cpu().numpy().view(np.int32),
                                      want.cpu().numpy().view(np.int32))
        R = R.cpu().numpy()
        tau = _thresholds(R, B + cap)
        guard = 4096
        buf = torch.full((B * cap + guard,), -7, dtype=torch.int32, device="cuda")
        sbuf = torch.full((B * cap + guard,), -7.0, dtype=torch.float32, device="cuda")
        cand, cand_sc = buf[:B * cap].view(B, cap), sbuf[:B * cap].view(B, cap)
        counts = torch.zeros(B, dtype=torch.int32, device="cuda")
        mlp.filter_rating(P, Z, _cu(p), _cu(tau), counts, cand, cand_sc)
        torch.cuda.synchronize()
    counts, cand, cand_sc = counts.cpu().numpy(), cand.cpu().numpy(), cand_sc.cpu().numpy()
    _check_kept(counts, cand, R >= tau[:, None], cap,
                bool((buf[B * cap:] == -7).all() and (sbuf[B * cap:] == -7).all()))
    for r in range(B):
        m = min(counts[r], cap)
        np.testing.assert_array_equal(cand_sc[r, :m].view(np.int32),
                                      R[r, cand[r, :m]].view(np.int32))


def test_rating_thresholds():
    """tau - 2 delta_u, rounded down (at most one ulp below the fp64 value); -inf stays."""
    from gnnrec import ops
    rng = np.random.default_rng(2)
    tau = rng.uniform(-1e-3, 0.6, 300).astype(np.float32)
    tau[5] = -np.inf
    Z = rng.uniform(1.0, 3e6, 300).astype(np.float32)
    for pmax in (0.0, 0.5, 3.0):
        got = ops.rating_thresholds(_cu(tau), _cu(Z), _cu(np.array([pmax], np.float32)))
        got = got.cpu().numpy()
        want = tau.astype(np.float64) - 2 * (pc.RATING_BAND / Z.astype(np.float64)
                                              + pc.RATING_SLACK * pmax)
        fin = np.isfinite(tau)
        assert got[5] == -np.inf
        assert (got[fin].astype(np.float64) <= want[fin]).all()
        assert (np.nextafter(got[fin], np.float32(np.inf)).astype(np.float64) >= want[fin]).all()


@pytest.mark.parametrize("with_rows", [False, True])
def test_mask_excluded_mapped(with_rows):
    from gnnrec import ops
    rng = np.random.default_rng(5)
    n_users, n_items = 40, 3000
    ip, ix = rc.exclusions(n_users, n_items, 0, 60, seed=8)
    cols = np.sort(np.concatenate([np.arange(200),
                                   200 + rng.choice(n_items - 200, 150, replace=False)]))
    rows = rng.integers(0, n_users, 23).astype(np.int64) if with_rows else None
    n_rows = 23 if with_rows else n_users
    S = rng.standard_normal((n_rows, cols.size)).astype(np.float32)
    want = S.copy()
    for r in range(n_rows):
        u = r if rows is None else rows[r]
        want[r, np.isin(cols, ix[ip[u]:ip[u + 1]])] = -np.inf
    got = _cu(S)
    ops.mask_excluded_mapped(got, _cu(cols.astype(np.int32)),
                             None if rows is None else _cu(rows), _cu(ip), _cu(ix))
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert np.isneginf(want).any()


# ---------------------------------------------------------------- 6. the popular sample
def test_the_sample_must_contain_the_popular_items():
    """Popularity on the items [4000, 5000) only, a 256-item prefix and cap: without the
    popular sample tau comes from ratings near 1 / n and every row keeps every popular item
    and overflows (the lists, recomputed exhaustively, are still right); with it no row
    does."""
    o = pc.OVERFLOW
    hu, hi, S, Z = _case("cos", o["kind"], o["d"])
    pop, w = pc.block_popularity()
    R = _ratings(S, Z, pc.p_vector(pop, w))
    excl = rc.exclusions()
    kw = dict(excl=excl, sample=o["sample"], cand_cap=o["cand_cap"])
    idx0, vals0, st0 = _recommend("cos", hu, hi, o["k"], pop, w, pop_sample=0, **kw)
    assert st0["overflow_rows"] == rc.N_USERS and st0["pop_sample"] == 0
    _assert_exact(idx0, vals0, R, excl, o["k"])
    idx1, vals1, st1 = _recommend("cos", hu, hi, o["k"], pop, w, pop_sample=pc.POP_SAMPLE, **kw)
    print(st0, st1)
    assert st1["overflow_rows"] == 0 and st1["candidates_max"] < o["cand_cap"]
    assert st1["pop_sample"] == pc.POP_SAMPLE
    np.testing.assert_array_equal(idx1, idx0)
    np.testing.assert_array_equal(vals1.view(np.int32), vals0.view(np.int32))


# ---------------------------------------------------------------- 7. edges
@pytest.mark.parametrize("head", HEADS)
def test_dominant_popularity_decides_the_lists(head):
    hu, hi, S, Z = _case(head, "normal", pc.EDGE_D)
    pop, w = pc.popularity("dominant")
    k = pc.DOMINANT_K
    idx, vals, stats = _recommend(head, hu, hi, k, pop, w)
    _assert_exact(idx, vals, _ratings(S, Z, pc.p_vector(pop, w)), None, k)
    top = np.sort(np.argsort(-pc.p_vector(pop, w).astype(np.float64), kind="stable")[:k])
    if head == "cos":   # the CPU file shows the gap for the cosine's softmax terms
        for r in range(rc.N_USERS):
            np.testing.assert_array_equal(np.sort(idx[r]), top)


@pytest.mark.parametrize("head", HEADS)
def test_edge_cases(head):
    from gnnrec import recs
    d = pc.EDGE_D
    hu, hi, S, Z = _case(head, "normal", d)
    pop, w = pc.popularity("dense")
    p = pc.p_vector(pop, w)
    R = _ratings(S, Z, p)
    # n_items < k
    from gnnrec import ops
    hi5 = hi[:5]
    idx, vals, stats = _recommend(head, hu, hi5, 10, pop[:5], w)
    assert (idx[:, 5:] == -1).all() and np.isneginf(vals[:, 5:]).all()
    assert (np.sort(idx[:, :5], axis=1) == np.arange(5)).all()
    # k above cand_cap / 4: the exhaustive path, the same Z
    excl = rc.exclusions()
    idx, vals, stats = _recommend(head, hu[:20], hi, 300, pop, w, excl=(excl[0][:21], excl[1]),
                                  cand_cap=1024)
    assert not stats["fast_path"]
    _assert_exact(idx, vals, R[:20], excl, 300)
    # a user with everything excluded, one with all but three
    ip, ix = excl
    lists = [ix[ip[u]:ip[u + 1]] for u in range(rc.N_USERS)]
    keep3 = np.array([17, 2600, 4999])
    lists[1] = np.setdiff1d(np.arange(rc.N_ITEMS), keep3).astype(np.int32)
    lists[2] = np.arange(rc.N_ITEMS, dtype=np.int32)[::-1]
    ex2 = rc.csr(lists)
    idx, vals, stats = _recommend(head, hu, hi, 10, pop, w, excl=ex2)
    _assert_exact(idx, vals, R, ex2, 10)
    assert sorted(idx[1, :3].tolist()) == keep3.tolist() and (idx[1, 3:] == -1).all()
    assert (idx[2] == -1).all() and np.isneginf(vals[2]).all()
    # no users
    idx, vals, stats = _recommend(head, hu, hi, 10, pop, w, rows=np.zeros(0, np.int64))
    assert idx.shape == (0, 10) and vals.shape == (0, 10)
    # popularity as a column; weight 0 ranks by the score alone (exp / Z is monotone, and on
    # the fast path no two distinct scores of a list collapse: compared with zero popularity)
    a = _recommend(head, hu, hi, 10, pop.reshape(-1, 1), w, excl=excl)
    b = _recommend(head, hu, hi, 10, pop, w, excl=excl)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.int32), b[1].view(np.int32))
    a = _recommend(head, hu, hi, 10, pop, 0.0, excl=excl)
    b = _recommend(head, hu, hi, 10, np.zeros_like(pop), 1.0, excl=excl)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.int32), b[1].view(np.int32))
    _assert_exact(a[0], a[1], _ratings(S, Z, np.zeros_like(p)), excl, 10)


@pytest.mark.parametrize("name", ["d102", "d2052"])
def test_widths_outside_the_mfma_kernel(name):
    """d % 4 != 0 and d > 2048: the exhaustive path, Z summed from the score rows."""
    from gnnrec import ops
    hu, hi, excl, k, kw, fast = rc.fallback_case(name)
    assert fast is False
    pop, w = pc.popularity("dense", hi.shape[0])
    p = pc.p_vector(pop, w)
    idx, vals, stats = _recommend("cos", hu, hi, k, pop, w, excl=excl)
    assert not stats["fast_path"]
    U, n = hu.shape[0], hi.shape[0]
    src = torch.arange(U, device="cuda").repeat_interleave(n)
    dst = torch.arange(n, device="cuda").repeat(U)
    S = ops.sddmm_cos(src, dst, _cu(hu), _cu(hi)).view(U, n)
    Z = ops.exp_rowsum(S)
    Z64 = np.exp(S.cpu().numpy().astype(np.float64)).sum(1)
    assert (np.abs(Z.cpu().numpy() - Z64) <= Z64 * (2.0 ** -22 + 12 * 2.0 ** -24)).all()
    R = ops.rating_rows_(S.clone(), Z, _cu(p)).cpu().numpy()
    _assert_exact(idx, vals, R, excl, k)


# ---------------------------------------------------------------- 8. the reference
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


class _G:
    def __init__(self, n_items, pop):
        self._n = n_items
        self.ndata = {"popularity": {"item": _cu(pop)}}

    def num_nodes(self, nt):
        return self._n


def _lists(users, items, n_users):
    out = [[] for _ in range(n_users)]
    for u, i in zip(np.asarray(users).tolist(), np.asarray(items).tolist()):
        out[u].append(i)
    return out


def test_recommend_matches_the_reference_fixture():
    """recs_cos_pop: the reference's own lists and ratings with use_popularity, weight 0.5."""
    from gnnrec.recs import create_ground_truth, get_recs
    meta = golden_io.manifest()["recs_cos_pop"]
    assert meta["use_popularity"] and meta["pred"] == "cos"
    a = golden_io.load("recs_cos_pop")
    bought = _lists(a["bought/u"], a["bought/i"], a["h/user"].shape[0])
    idx, _, stats = _recommend("cos", a["h/user"], a["h/item"], meta["k"], a["popularity"],
                               meta["weight_popularity"], a["user_ids"], rc.csr(bought))
    assert stats["fast_path"]
    h = {"user": _cu(a["h/user"]), "item": _cu(a["h/item"])}
    old = get_recs(_G(a["h/item"].shape[0], a["popularity"]), h, None, meta["embed_dim"],
                   meta["k"], a["user_ids"].tolist(),
                   create_ground_truth(a["bought/u"], a["bought/i"]), True, True, None, "cos",
                   True, meta["weight_popularity"])
    for r, (u, ref, s) in enumerate(zip(a["user_ids"], a["recs"], a["scores"])):
        ref = ref[ref >= 0]
        got = idx[r][idx[r] >= 0]
        _assert_same_ranking(got, ref, s, meta["min_rel_gap_required"], f"user {u}")
        _assert_same_ranking(old[int(u)], ref, s, meta["min_rel_gap_required"], f"get_recs {u}")
        assert not set(got.tolist()) & set(bought[int(u)])


def test_mlp_head_matches_get_recs():
    """No reference-made fixture for the MLP head with popularity: the unchanged
    get_recs(pred='nn', use_popularity=True), under the same rule with the host's ratings
    (the CPU file shows their gaps above MLP_REF_GAP)."""
    from gnnrec.recs import get_recs
    s = pc.MLP_REF
    hu, hi, pop, (ip, ix) = pc.mlp_ref_case()
    S = mc.host_scores(mc.head(s["d"]), hu, hi)
    R, _ = pc.ratings64(S, pc.p_vector(pop, s["weight"]))
    idx, _, stats = _recommend("mlp", hu, hi, s["k"], pop, s["weight"], excl=(ip, ix))
    model = type("M", (), {})()
    model.pred_fn = type("P", (), {})()
    model.pred_fn.layer_nn = _mlp_head(s["d"])
    bought = {u: ix[ip[u]:ip[u + 1]].tolist() for u in range(s["n_users"])}
    with torch.no_grad():
        old = get_recs(_G(s["n_items"], pop), {"user": _cu(hu), "item": _cu(hi)}, model, s["d"],
                       s["k"], list(range(s["n_users"])), bought, True, True, None, "nn", True,
                       s["weight"])
    ref_i, _ = rc.ranked(R, ip, ix, s["k"])
    for u in range(s["n_users"]):
        _assert_same_ranking(idx[u], ref_i[u], R[u], pc.MLP_REF_GAP, f"user {u}")
        _assert_same_ranking(old[u], ref_i[u], R[u], pc.MLP_REF_GAP, f"get_recs {u}")


# ---------------------------------------------------------------- 9. the graph entry
def test_recommend_for_graph_with_popularity():
    from gnnrec.graph import HeteroGraph
    from gnnrec.recs import recommend, recommend_for_graph
    rng = np.random.default_rng(3)
    n_u, n_i, E = 120, 80, 900
    u, i = rng.integers(0, n_u, E), rng.integers(0, n_i, E)
    edges = {("user", "buys", "item"): (u, i), ("item", "bought-by", "user"): (i, u)}
    g = HeteroGraph({ce: (torch.from_numpy(s), torch.from_numpy(d)) for ce, (s, d) in edges.items()},
                    {"user": n_u, "item": n_i}).to("cuda")
    h = {"user": _cu(rng.standard_normal((n_u, 16)).astype(np.float32)),
         "item": _cu(rng.standard_normal((n_i, 16)).astype(np.float32))}
    users = [0, 5, 7, 119, 64, 33]
    with pytest.raises(KeyError, match="popularity"):
        recommend_for_graph(g, h, 5, users, use_popularity=True, weight_popularity=0.01)
    pop = rng.random((n_i, 1)).astype(np.float32)          # a column, as the reference stores it
    g.nodes["item"].data["popularity"] = _cu(pop)
    ex_ptr, ex_idx = g.in_csr("bought-by")[:2]
    for wgt in (0.01, 0.5):
        idx, vals = recommend_for_graph(g, h, 5, users, use_popularity=True,
                                        weight_popularity=wgt)
        ref_i, ref_v = recommend(h["user"], h["item"], 5, _cu(np.asarray(users, np.int64)),
                                 (ex_ptr.cuda(), ex_idx.cuda()),
                                 popularity=g.ndata["popularity"]["item"], weight_popularity=wgt)
        assert torch.equal(idx, ref_i) and torch.equal(vals, ref_v)
    plain, _ = recommend_for_graph(g, h, 5, users)
    assert not torch.equal(plain, idx)   # weight 0.5 over 80 items changes the lists
