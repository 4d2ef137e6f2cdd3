"""GPU checks of the parts of the bf16-prefiltered top-k (csrc/recommend.hip), each against a
float64 or bit-exact host reference: the error bound the filter rests on, measured on the
device's own approximate scores; normalize_rows_bf16 bit for bit; which items the filter
keeps; mask_excluded and topk_candidates on their own; and the paths of recs.recommend that
tests/test_gpu_recommend.py does not reach.  Inputs and references come from
tests/recommend_cases.py; tests/test_recommend_cpu.py checks on the host every band and share
condition asserted here."""
import functools

import numpy as np
import pytest
import torch

import recommend_cases as rc

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5   # tests/test_gpu_parity.py: what sddmm_cos is held to against fp64
TIE_GAP = 1e-5            # fp64 gap under which two neighbouring ranks may swap


def _cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _scores(hu, hi):
    """ops.sddmm_cos for every pair -> fp32 [U, n]."""
    from gnnrec import ops
    U, n = hu.shape[0], hi.shape[0]
    src = torch.arange(U, device="cuda").repeat_interleave(n)
    dst = torch.arange(n, device="cuda").repeat(U)
    return ops.sddmm_cos(src, dst, _cu(hu), _cu(hi)).view(U, n).cpu().numpy()


def _wide(x, pad, junk=1e30):
    """x as the [:, :d] view of a device table with `pad` more columns, those full of junk."""
    w = torch.full((x.shape[0], x.shape[1] + pad), junk, dtype=torch.float32, device="cuda")
    w[:, :x.shape[1]] = _cu(x)
    return w[:, :x.shape[1]]


def _bits(t):
    """A bf16 device tensor's bit patterns as uint16."""
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


# ---------------------------------------------------------------- 1. the bound
@pytest.mark.parametrize("d,scale", [(d, 1.0) for d in rc.BOUND_DIMS] + list(rc.BOUND_SCALED))
@pytest.mark.parametrize("kind", ["normal", "relu", "lowrank", "midpoint"])
def test_device_bound(kind, d, scale):
    """|a - s| <= eps for the device's a (normalize_rows_bf16, then score_bf16_store) against
    the float64 cosine and against ops.sddmm_cos, the score by definition.  The maxima are
    recorded in profiles/recommend_device_bound.md."""
    from gnnrec import ops
    hu, hi = rc.bound_tables(kind, d, scale)
    a = ops.score_bf16_store(ops.normalize_rows_bf16(_cu(hu)),
                             ops.normalize_rows_bf16(_cu(hi))).cpu().numpy().astype(np.float64)
    e64 = np.abs(a - rc.cosine64(hu, hi)).max()
    e32 = np.abs(a - _scores(hu, hi).astype(np.float64)).max()
    print(f"BOUND {kind} d={d} scale={scale:g}: max|a - s64| = {e64:.3e}, "
          f"max|a - s32| = {e32:.3e} (eps {rc.EPS:.3e})")
    assert e64 <= rc.EPS and e32 <= rc.EPS


# ---------------------------------------------------------------- 2. normalize, exactly
def _assert_normalized(out, x, d):
    """out: normalize_rows_bf16 of rows x [n, d] -> every entry one of the two admissible
    patterns (one where the rounding is decided), the pad exact zeros."""
    dpad = (d + 31) // 32 * 32
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (x.shape[0], dpad)
    got = _bits(out)
    assert (got[:, d:] == 0).all()
    a, b, _ = rc.normalize_expected(x)
    ok = (got[:, :d] == a) | (got[:, :d] == b)
    assert ok.all(), f"{(~ok).sum()} of {ok.size} entries are neither admissible pattern"
    return a, b


@pytest.mark.parametrize("d", rc.NORMALIZE_DIMS)
def test_normalize_rows_bf16_bits(d):
    """Contiguous and strided sources (pad 4: the 16-B path where d % 4 == 0; pad 3: the
    scalar path), a row_map with repeats, 1, 3 and 5 rows (the four-rows-per-block tail), a
    zero row and a row under the 1e-12 guard."""
    from gnnrec import ops
    x = rc.normalize_source(d)
    a, b, _ = rc.normalize_expected(x)
    assert (a == b).mean() > 0.99  # nearly every entry is pinned to one value
    rmap = np.array([36, 5, 0, 0, 17, 6, 5, 36, 6], np.int64)
    for pad in (0, 4, 3):
        src = _cu(x) if pad == 0 else _wide(x, pad)
        _assert_normalized(ops.normalize_rows_bf16(src), x, d)
        out = ops.normalize_rows_bf16(src, _cu(rmap))
        _assert_normalized(out, x[rmap], d)
        assert (_bits(out)[[1, 6]] == 0).all()  # the zero row
        for n in (1, 3, 5):
            _assert_normalized(ops.normalize_rows_bf16(src[:n]), x[:n], d)
            _assert_normalized(ops.normalize_rows_bf16(src, _cu(rmap[:n])), x[rmap[:n]], d)


@pytest.mark.parametrize("d", [100, 128])
def test_normalize_rows_bf16_midpoint_table(d):
    from gnnrec import ops
    hu, _ = rc.tables("midpoint", d, 37, 1)
    a, b = _assert_normalized(ops.normalize_rows_bf16(_cu(hu)), hu, d)
    assert (a == b).mean() > 0.99


@pytest.mark.parametrize("cols", [5, 8])
def test_normalize_rows_bf16_ties_go_to_even(cols):
    """rc.tie_rows: the norm is exactly 512 in any summation order and the first quotient an
    exact midpoint, so the bits are known exactly and the tie rule decides them (cols = 8:
    three zero columns more, the 16-B path)."""
    from gnnrec import ops
    x = np.zeros((128, cols), np.float32)
    x[:, :5] = rc.tie_rows()
    got = _bits(ops.normalize_rows_bf16(_cu(x)))
    np.testing.assert_array_equal(got[:, :cols], rc.bf16_bits(x / np.float32(512)))
    assert (got[:, cols:] == 0).all()


# ---------------------------------------------------------------- 4. the filter's kept set
@pytest.mark.parametrize("d", rc.FILTER_DIMS)
def test_filter_keeps_exactly_the_expected_set(d):
    """No row can overflow (n <= cap): the stored ids are exactly {v : a >= tau_u - 2 eps},
    from the float64 product of the bf16 tables outside a band of 2^-16 round the threshold,
    and from score_bf16_store of the same inputs with no band at all."""
    from gnnrec import ops
    hu, hi = rc.filter_tables(d)
    ub_all, vb_all = ops.normalize_rows_bf16(_cu(hu)), ops.normalize_rows_bf16(_cu(hi))
    a64 = ub_all.float().cpu().numpy().astype(np.float64) @ \
        vb_all.float().cpu().numpy().astype(np.float64).T
    cap, guard = rc.FILTER_CAP, 4096
    for B in rc.FILTER_BS:
        for n in rc.FILTER_NS:
            msg = f"d={d} B={B} n={n}"
            ub, vb = ub_all[:B].contiguous(), vb_all[:n].contiguous()
            tau = rc.filter_tau(d, B)
            keep, band = rc.filter_expected(a64[:B, :n], tau)
            assert band.mean() < rc.FILTER_BAND_SHARE, msg
            buf = torch.full((B * cap + guard,), -7, dtype=torch.int32, device="cuda")
            cand = buf[:B * cap].view(B, cap)
            counts = torch.zeros(B, dtype=torch.int32, device="cuda")
            ops.score_bf16_filter(ub, vb, _cu(tau), counts, cand)
            stored = ops.score_bf16_store(ub, vb).cpu().numpy()
            assert (buf[B * cap:] == -7).all(), msg
            cnt, c = counts.cpu().numpy(), cand.cpu().numpy()
            assert ((cnt >= 0) & (cnt <= n)).all(), msg
            used = np.arange(cap)[None, :] < cnt[:, None]
            assert (c[~used] == -7).all(), msg            # counts[u] == number of stored ids
            assert ((c[used] >= 0) & (c[used] < n)).all(), msg
            got = np.zeros((B, n), bool)
            got[np.nonzero(used)[0], c[used]] = True
            np.testing.assert_array_equal(got.sum(1), cnt, err_msg=msg)  # distinct ids
            wrong = (got != keep) & ~band
            assert not wrong.any(), f"{msg}: rows {np.unique(np.nonzero(wrong)[0])[:8]}"
            thr = tau - np.float32(2 * rc.EPS)
            np.testing.assert_array_equal(got, stored >= thr[:, None], err_msg=msg)
            assert got[0].all() and (B == 1 or not got[-1].any()), msg


# ---------------------------------------------------------------- 5. mask_excluded
def _mask_lists(n_users, n_cols, rng):
    lists = []
    for u in range(n_users):
        kind = u % 5
        if kind == 0:
            x = np.zeros(0, np.int64)
        elif kind == 1:
            x = rng.integers(0, n_cols, 12)
            x = np.concatenate([x, x[:5]])                       # duplicates
        elif kind == 2:
            x = np.concatenate([rng.integers(0, n_cols, 6),
                                [-1, -5, n_cols, n_cols + 7, 2 ** 31 - 1, -2 ** 31]])
            rng.shuffle(x)
        else:
            x = rng.choice(n_cols, int(rng.integers(1, min(n_cols, 40) + 1)), replace=False)
        lists.append(x)
    lists[3] = rng.choice(max(n_cols, 200), 200, replace=n_cols < 200)  # longer than a wave
    return lists


def _check_mask(n_rows, n_cols, pad, rows, seed):
    from gnnrec import ops
    rng = np.random.default_rng(seed)
    n_users = 140
    lists = _mask_lists(n_users, n_cols, rng)
    ip, ix = rc.csr(lists)
    base = rng.standard_normal((n_rows, n_cols + pad)).astype(np.float32)
    want = base.copy()
    for r in range(n_rows):
        u = r if rows is None else int(rows[r])
        for c in lists[u]:
            if 0 <= c < n_cols:
                want[r, c] = -np.inf
    t = _cu(base)
    ops.mask_excluded(t[:, :n_cols], None if rows is None else _cu(rows), _cu(ip), _cu(ix))
    np.testing.assert_array_equal(t.cpu().numpy().view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("rows_given", [False, True])
@pytest.mark.parametrize("n_rows", [1, 4, 5, 130])
def test_mask_excluded(n_rows, rows_given):
    """Bitwise the input with -inf exactly at the listed columns: contiguous rows and a
    strided view whose pad columns stay as they were; empty lists, duplicates, ids outside
    [0, n_cols), a list longer than a wave; user_rows a permutation with repeats."""
    rows = None
    if rows_given:
        rows = np.random.default_rng(n_rows).permutation(140)[:n_rows].astype(np.int64)
        rows[0] = 3                    # the 200-id list
        rows[-1] = rows[n_rows // 2]   # a repeat (n_rows = 1: the row itself)
    for pad in (0, 5):
        _check_mask(n_rows, 300, pad, rows, seed=n_rows + pad)


def test_mask_excluded_one_column():
    _check_mask(5, 1, 0, None, seed=1)
    _check_mask(5, 1, 3, np.array([3, 1, 2, 3, 0], np.int64), seed=2)


# ---------------------------------------------------------------- 6. topk_candidates
def _candidates_reference(hu, hi, counts, cand, cap, k, rows, lists):
    """Per batch row (count in [0, cap]): rc.ranked over the float64 cosines, everything but
    the row's candidates excluded along with the user's list -> (idx, s64 [B, n_items]);
    rows with a count outside [0, cap] get None."""
    n_items = hi.shape[0]
    users = np.arange(len(counts)) if rows is None else rows
    s64 = rc.cosine64(hu[users], hi)
    ref = []
    for b, n in enumerate(counts):
        if n < 0 or n > cap:
            ref.append(None)
            continue
        out = np.union1d(np.setdiff1d(np.arange(n_items), cand[b, :n]), lists[users[b]])
        ip, ix = rc.csr([out])
        ref.append(rc.ranked(s64[b:b + 1], ip, ix, k)[0][0])
    return ref, s64


def _check_candidates(hu, hi, counts, cand, k, rows, lists, pad=4):
    """Run topk_candidates on [:, :d] views of tables `pad` columns wider and check ids,
    values and the rows that must stay unwritten."""
    from gnnrec import ops
    counts = np.asarray(counts, np.int32)
    B, cap = cand.shape
    wu, wi = (_wide(hu, pad), _wide(hi, pad)) if pad else (_cu(hu), _cu(hi))
    out_v = torch.full((B, k), 123.0, dtype=torch.float32, device="cuda")
    out_i = torch.full((B, k), -9, dtype=torch.int64, device="cuda")
    ip, ix = (None, None) if lists is None else rc.csr(lists)
    ops.topk_candidates(_cu(counts), _cu(cand.astype(np.int32)),
                        None if rows is None else _cu(rows), wu, wi, k,
                        None if ip is None else _cu(ip), None if ix is None else _cu(ix),
                        out_v, out_i)
    vals, idx = out_v.cpu().numpy(), out_i.cpu().numpy()
    if lists is None:
        lists = [np.zeros(0, np.int64)] * hu.shape[0]
    ref, s64 = _candidates_reference(hu, hi, counts, cand, cap, k, rows, lists)
    users = np.arange(B) if rows is None else rows
    S32 = _scores(hu[users], hi)
    for b in range(B):
        msg = f"row {b} (count {counts[b]})"
        if ref[b] is None:   # overflowed or negative: the sentinel stays
            assert (idx[b] == -9).all() and (vals[b] == 123.0).all(), msg
            continue
        n_ok = int((ref[b] >= 0).sum())
        assert (idx[b, n_ok:] == -1).all() and np.isneginf(vals[b, n_ok:]).all(), msg
        got, want = idx[b, :n_ok], ref[b][:n_ok]
        assert np.unique(got).size == n_ok, msg
        assert np.isin(got, cand[b, :counts[b]]).all(), msg
        assert not np.isin(got, lists[users[b]]).any(), msg
        for j in np.nonzero(got != want)[0]:  # only a swap among (near-)tied items
            assert abs(s64[b, got[j]] - s64[b, want[j]]) <= TIE_GAP, f"{msg}: rank {j}"
        np.testing.assert_array_equal(vals[b, :n_ok].view(np.int32),
                                      S32[b, got].view(np.int32), err_msg=msg)
        np.testing.assert_allclose(vals[b, :n_ok], s64[b, got], rtol=RTOL, atol=ATOL, err_msg=msg)
    return idx, vals


def _draw_candidates(rng, counts, cap, n_items):
    """cand [B, cap]: row b's first min(count, cap) slots distinct random items; the slots
    past the count hold other valid ids, which a kernel reading too far would rank."""
    cand = rng.integers(0, n_items, (len(counts), cap))
    for b, n in enumerate(counts):
        m = min(max(n, 0), cap)
        cand[b, :m] = rng.choice(n_items, m, replace=False)
    return cand


@pytest.mark.parametrize("rows_given", [False, True])
@pytest.mark.parametrize("d", [4, 64, 68, 128, 132, 256])
def test_topk_candidates(d, rows_given):
    """Each lane-group form on both sides of its limit, strided tables, counts 0, 1, k - 1,
    cap, cap + 1 and -1, a row whose candidates are all excluded."""
    rng = np.random.default_rng([d, rows_given])
    n_users, n_items, cap, k = 20, 600, 64, 10
    hu, hi = rc.tables("normal", d, n_users, n_items, seed=4)
    counts = [0, 1, k - 1, cap, cap + 1, -1, 30, 40, cap, 17, 33, 5]
    rows = None
    if rows_given:
        rows = rng.permutation(n_users)[:len(counts)].astype(np.int64)
        rows[9] = rows[6]  # a repeated user
    cand = _draw_candidates(rng, counts, cap, n_items)
    users = np.arange(len(counts)) if rows is None else rows
    lists = [rng.choice(n_items, int(rng.integers(0, 31)), replace=False) for _ in range(n_users)]
    for b in (3, 6, 8):  # some of the row's own candidates among its user's exclusions
        lists[users[b]] = np.concatenate([lists[users[b]], cand[b, 2:counts[b]:3]])
    lists[users[7]] = np.concatenate([cand[7, :40][::-1], lists[users[7]]])  # all of them
    idx, _ = _check_candidates(hu, hi, counts, cand, k, rows, lists)
    assert (idx[7] == -1).all()
    if not rows_given:
        _check_candidates(hu, hi, counts, cand, k, rows, None, pad=0)  # no exclusion lists


@pytest.mark.parametrize("cap,k", [(1, 1), (64, 64), (4096, 10), (4096, 64)])
def test_topk_candidates_caps(cap, k):
    """k == cap at cap 1 and 64, and the largest cap with a full list: count == cap is
    served, count == cap + 1 is not."""
    rng = np.random.default_rng([cap, k])
    n_users, n_items = 6, 5000
    hu, hi = rc.tables("normal", 64, n_users, n_items, seed=6)
    counts = [cap, cap - 1, cap + 1, cap, min(cap, 10), 0]
    cand = _draw_candidates(rng, counts, cap, n_items)
    lists = [np.zeros(0, np.int64) for _ in range(n_users)]
    lists[3] = np.concatenate([cand[3, ::2], rng.integers(0, n_items, 20)])  # half of a full row
    lists[4] = cand[4, :counts[4]].copy()                                    # all of row 4
    idx, vals = _check_candidates(hu, hi, counts, cand, k, None, lists)
    assert (idx[0] >= 0).all() and (idx[4] == -1).all() and (idx[2] == -9).all()


@pytest.mark.parametrize("length", [2048, 2049, 4097])
def test_topk_candidates_exclusion_chunks(length):
    """Exclusion lists on both sides of the staging chunk (2048 ids): the row's best
    candidate is struck by the list's last id, its second best by the first."""
    rng = np.random.default_rng(length)
    n_users, n_items, cap, k, n = 3, 5000, 64, 10, 30
    hu, hi = rc.tables("normal", 16, n_users, n_items, seed=8)
    counts = [n, n, n]
    cand = _draw_candidates(rng, counts, cap, n_items)
    s64 = rc.cosine64(hu, hi)
    lists = [rng.choice(n_items, 7, replace=False) for _ in range(n_users)]
    u = 1
    best = cand[u, :n][np.argsort(-s64[u, cand[u, :n]])]
    others = rng.choice(np.setdiff1d(np.arange(n_items), cand[u, :n]), length - 2, replace=False)
    mid = [best[2]] if length > 4096 else []   # and one in a middle chunk
    body = np.concatenate([others[:2500], mid, others[2500:]])[:length - 2]
    lists[u] = np.concatenate([[best[1]], body, [best[0]]])
    assert lists[u].size == length
    idx, _ = _check_candidates(hu, hi, counts, cand, k, None, lists)
    assert best[0] not in idx[u] and best[1] not in idx[u]
    assert idx[u, 0] == (best[3] if mid else best[2])


def test_topk_candidates_ties_go_to_the_lower_id():
    """Two candidates with identical item rows, in either order in the list."""
    rng = np.random.default_rng(12)
    n_items, cap, k, n = 600, 64, 10, 40
    hu, hi = rc.tables("normal", 64, 4, n_items, seed=10)
    hi = hi.copy()
    p, q = 77, 431
    hi[p] = hi[q] = 2 * hu[1] + 0.1 * hi[p]   # user 1's best items by far, bit-identical rows
    rows = np.array([1, 1, 1], np.int64)
    cand = _draw_candidates(rng, [n, n, n], cap, n_items)
    for b, (sp, sq) in enumerate([(3, 35), (35, 3), (0, n - 1)]):
        cand[b, :n] = rng.choice(np.setdiff1d(np.arange(n_items), [p, q]), n, replace=False)
        cand[b, sp], cand[b, sq] = p, q
    idx, vals = _check_candidates(hu, hi, [n, n, n], cand, k, rows, None)
    np.testing.assert_array_equal(idx[:, 0], [p, p, p])
    np.testing.assert_array_equal(idx[:, 1], [q, q, q])
    np.testing.assert_array_equal(vals[:, 0].view(np.int32), vals[:, 1].view(np.int32))


# ---------------------------------------------------------------- 7. recommend's other paths
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


@pytest.mark.parametrize("name", sorted(rc.FALLBACKS))
def test_recommend_other_paths(name):
    """d % 4 != 0 (6, 102), d above REC_MAX_D and the boundary d = 2048 on the fast path,
    d = 100 (a multiple of 4 that is none of 32: the fast path, padded to 128), fewer items
    or fewer sampled items than k, a single item: the exhaustive ranking each time."""
    hu, hi, excl, k, kw, fast = rc.fallback_case(name)
    idx, vals, stats = _recommend(hu, hi, k, excl=excl, **kw)
    print(name, stats)
    if fast is not None:
        assert stats["fast_path"] == fast
    if fast:
        assert stats["overflow_rows"] == 0
    if name == "sample_below_k":  # tau = -inf keeps every item: each row is redone
        assert stats["fast_path"] and stats["overflow_rows"] == hu.shape[0]
    _assert_exact(idx, vals, _scores(hu, hi), excl, k)


def test_recommend_empty_inputs():
    hu, hi = rc.tables("normal", 16, 16, 600, seed=2)
    excl = rc.exclusions(16, 600, 0, 20, seed=3)
    idx, vals, _ = _recommend(hu, hi, 10, np.zeros(0, np.int64), excl)
    assert idx.shape == (0, 10) and vals.shape == (0, 10)
    idx, vals, _ = _recommend(hu, hi[:0], 10, excl=rc.csr([[]] * 16))
    assert idx.shape == (16, 10) and (idx == -1).all() and np.isneginf(vals).all()


@functools.lru_cache(maxsize=None)
def _standard():
    hu, hi = rc.tables("normal", 16)
    excl = rc.exclusions()
    return hu, hi, excl, _recommend(hu, hi, 10, excl=excl)


@pytest.mark.parametrize("batch_size", [1, 129])
def test_recommend_batch_size(batch_size):
    """One user per batch, and a last batch of one user: bitwise the default batch."""
    hu, hi, excl, (idx0, vals0, _) = _standard()
    idx, vals, stats = _recommend(hu, hi, 10, excl=excl, batch_size=batch_size)
    assert stats["fast_path"] and stats["overflow_rows"] == 0
    np.testing.assert_array_equal(idx, idx0)
    np.testing.assert_array_equal(vals.view(np.int32), vals0.view(np.int32))
