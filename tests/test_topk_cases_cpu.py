"""The inputs of tests/test_gpu_topk_rows.py are what they claim to be (no GPU): with the
scan loops of csrc/topk.hip restated on the host, every table and list in tests/topk_cases.py
reaches the path it is named for, and the reference itself agrees with a naive sort."""
import numpy as np
import pytest

import topk_cases as tc

# per column count: the float4 scan's (threads making >= 1 and >= 2 trips of the
# four-loads-in-flight loop, most trips of one thread), (threads in the single-float4 loop,
# its trips over all threads), the trips of the scalar tail after them; and for the scalar
# scan (threads with a column, fewest and most columns of a thread).  Literal on purpose: a
# change to the loop structure of topk_rows_kernel means revisiting the column counts.
TRIPS = {
    1: ((0, 0, 0), (0, 0), 1, (1, 0, 1)),
    3: ((0, 0, 0), (0, 0), 3, (3, 0, 1)),
    4: ((0, 0, 0), (1, 1), 0, (4, 0, 1)),
    5: ((0, 0, 0), (1, 1), 1, (5, 0, 1)),
    255: ((0, 0, 0), (63, 63), 3, (255, 0, 1)),
    256: ((0, 0, 0), (64, 64), 0, (256, 1, 1)),
    257: ((0, 0, 0), (64, 64), 1, (256, 1, 2)),
    1023: ((0, 0, 0), (255, 255), 3, (256, 3, 4)),
    1024: ((0, 0, 0), (256, 256), 0, (256, 4, 4)),
    1027: ((0, 0, 0), (256, 256), 3, (256, 4, 5)),
    3072: ((0, 0, 0), (256, 768), 0, (256, 12, 12)),
    3073: ((0, 0, 0), (256, 768), 1, (256, 12, 13)),
    3076: ((1, 0, 1), (255, 765), 0, (256, 12, 13)),    # thread 0 alone enters
    3079: ((1, 0, 1), (255, 765), 3, (256, 12, 13)),
    4092: ((255, 0, 1), (1, 3), 0, (256, 15, 16)),      # all but the last thread
    4096: ((256, 0, 1), (0, 0), 0, (256, 16, 16)),      # every thread once, nothing after
    4097: ((256, 0, 1), (0, 0), 1, (256, 16, 17)),
    7168: ((256, 0, 1), (256, 768), 0, (256, 28, 28)),  # one short of a second trip
    7172: ((256, 1, 2), (255, 765), 0, (256, 28, 29)),  # thread 0 alone makes a second
    7175: ((256, 1, 2), (255, 765), 3, (256, 28, 29)),
    8195: ((256, 256, 2), (0, 0), 3, (256, 32, 33)),    # every thread twice, and the tail
}


def test_column_counts_cover_the_scan_loops():
    assert set(TRIPS) == set(tc.COLS)
    for n in tc.COLS:
        u, s, t = tc.trips(n, True)
        assert 4 * (4 * u.sum() + s.sum()) + t.sum() == n   # every column scanned once
        assert (t <= 1).all() and t.sum() == n % 4
        _, _, sc = tc.trips(n, False)
        assert sc.sum() == n
        got = ((int((u >= 1).sum()), int((u >= 2).sum()), int(u.max())),
               (int((s >= 1).sum()), int(s.sum())), int(t.sum()),
               (int((sc >= 1).sum()), int(sc.min()), int(sc.max())))
        assert got == TRIPS[n], (n, got)
    unrolled = {n: v[0] for n, v in TRIPS.items()}
    assert unrolled[3072] == (0, 0, 0) and unrolled[3076] == (1, 0, 1)    # thread 0 only
    assert unrolled[4096] == (256, 0, 1) and TRIPS[4096][1] == (0, 0)     # all threads once
    assert unrolled[7168] == (256, 0, 1) and unrolled[7172] == (256, 1, 2)  # a second trip
    assert unrolled[8195] == (256, 256, 2)
    # the single-float4 loop after the unrolled one, alone and after it; the tail of 1 and 3
    assert TRIPS[4092][1] == (1, 3) and TRIPS[7168][1] == (256, 768)
    assert {TRIPS[n][2] for n in tc.COLS} == {0, 1, 3}
    # fewer columns than threads, and than the k of some scan case
    assert min(tc.COLS) < min(k for k in tc.SCAN_KS if k > 1) and 255 in tc.COLS


def test_edge_rows_put_winners_at_every_loop_boundary():
    """The `edges` rows of the scan cases: every column next to a boundary of the scan loops
    is among the best 17, so the k = 17 and k = 64 cases lose a winner if one is dropped."""
    assert 17 in tc.SCAN_KS and 64 in tc.SCAN_KS
    for n in tc.COLS:
        s, names = tc.scan_scores(n)
        at = tc.edge_columns(n)
        n4 = n & ~3
        assert at.size <= 17 and {0, n - 1} <= set(at.tolist())
        assert n4 == n or n4 in at                       # the first tail column
        assert n4 == 0 or n4 - 1 in at                   # the last float4 column
        for b in tc.LOOP_BOUNDS:                         # 256 threads x float4 x (3 | 4) trips
            assert b % (4 * tc.THREADS) == 0 and (b >= n or {b - 1, b} <= set(at.tolist()))
        rows = [r for r, name in enumerate(names) if name == "edges"]
        assert len(rows) == 2
        idx, vals = tc.ranked(s, 17)
        for r in rows:
            assert set(idx[r, :at.size].tolist()) == set(at.tolist())
            assert np.unique(vals[r, :at.size]).size == at.size


def test_layouts_select_the_scan_they_are_named_for():
    for n in tc.COLS + tc.INSERT_COLS + tc.EXCL_COLS + (tc.ROW_COLS,):
        for lay in tc.LAYOUTS:
            width, start = tc.geometry(lay, n)
            assert width >= start + n
            big, s0 = tc.embed(np.zeros((2, n), np.float32), lay)
            assert big.shape == (2, width) and s0 == start
            assert (big[:, :start] == tc.FILL).all() and (big[:, start + n:] == tc.FILL).all()
        assert tc.geometry("contig", n) == (n, 0) and tc.is_vec("contig", n) == (n % 4 == 0)
        w, s = tc.geometry("prefix", n)
        assert s == 0 and w % 4 == 0 and n + 4 < w <= n + 8 and tc.is_vec("prefix", n)
        w, s = tc.geometry("odd_ld", n)      # the stride alone rules out float4 loads
        assert s == 0 and w % 4 == 1 and w > n and not tc.is_vec("odd_ld", n)
        w, s = tc.geometry("shifted", n)     # the stride would do: the base does not
        assert s == 1 and w % 4 == 0 and not tc.is_vec("shifted", n)
    # a float4 scan with a ragged end exists, and one with a stride above n_cols
    assert any(n % 4 for n in tc.COLS) and tc.PASS_LAYOUT == "prefix"
    assert all(tc.is_vec(tc.PASS_LAYOUT, n) and n % 4 for n in tc.PASS_COLS)


def test_ks_choose_every_kmax_first_and_later():
    first = {tc.passes(k)[0] for k in tc.KS}
    later = {m for k in tc.KS for m in tc.passes(k)[1:]}
    assert first == {16, 32, 64} and later == {16, 32, 64}
    last = {min(tc.PASS, k - c0) for k in tc.KS for c0 in range(0, k, tc.PASS)}
    assert {1, 16, 17, 32, 33, 64} <= last
    assert [tc.passes(k) for k in (17, 32, 81, 96, 97, 129)] == \
        [[32], [32], [64, 32], [64, 32], [64, 64], [64, 64, 16]]
    assert {tc.passes(k)[0] for k in tc.SCAN_KS} == {16, 32, 64}
    assert {m for k in tc.INSERT_KS for m in tc.passes(k)} == {16, 32, 64}
    assert {m for k in tc.EXCL_KS for m in tc.passes(k)} == {16, 32, 64}


def test_owner_helpers_match_the_restated_loops():
    """owner_vec / owner_scalar against a walk of the loops, thread by thread."""
    for n in (5, 1027, 4097, 8195):
        for vec in (True, False):
            seen = np.full(n, -1)
            for tid in range(tc.THREADS):
                cols, c_tail = [], 0
                if vec:
                    n4 = n & ~3
                    for c0 in range(4 * tid, n4, 4 * tc.THREADS):
                        cols += [c0, c0 + 1, c0 + 2, c0 + 3]
                    c_tail = n4
                cols += list(range(c_tail + tid, n, tc.THREADS))
                assert (seen[cols] == -1).all()
                seen[cols] = tid
            np.testing.assert_array_equal(seen, tc.owner(np.arange(n), n, vec))


@pytest.mark.parametrize("n_cols,layout,k", tc.INSERT_CASES)
def test_one_owner_rows_have_one_owner(n_cols, layout, k):
    """The best one_owner_count columns of a one_owner row are scanned by one thread in the
    layout named; that is all k of them at the widest table, a full KMAX = 16 list at 4096
    columns and a full KMAX = 32 list at 8195."""
    s, names = tc.insert_scores(n_cols, layout, k)
    vec = tc.is_vec(layout, n_cols)
    assert vec == (layout == "prefix")
    m = tc.one_owner_count(k, n_cols, vec)
    assert m == {4096: min(k, 16), 8195: min(k, 32), 25603: k}[n_cols]
    idx, vals = tc.ranked(s, k)
    rows = [r for r, name in enumerate(names) if name == "one_owner"]
    assert len(rows) >= 2
    owners = set()
    for r in rows:
        own = tc.owner(idx[r, :m], n_cols, vec)
        assert (own == own[0]).all(), (r, own)
        owners.add(int(own[0]))
        assert np.unique(vals[r, :m]).size == m and vals[r, m - 1] >= 100.0
        assert m == k or vals[r, m] < 10.0    # the background lies below
        assert (tc.owner(idx[r, :m], n_cols, not vec) != own[0]).any()  # not so in the other
    assert len(owners) == len(rows)
    for r, name in enumerate(names):
        if name == "ascending":
            assert (np.diff(s[r]) > 0).all()
            np.testing.assert_array_equal(idx[r], np.arange(n_cols - 1, n_cols - 1 - k, -1))
        if name == "descending":
            assert (np.diff(s[r]) < 0).all()
            np.testing.assert_array_equal(idx[r], np.arange(k))


def test_score_patterns():
    for n in (1, 5, 257, 4097):
        s, names = tc.scan_scores(n)
        assert s.dtype == np.float32 and np.isfinite(s).all()
        for r, name in enumerate(names):
            if name == "normal":
                assert np.unique(s[r]).size == n
        assert n < 257 or np.unique(s[names.index("ints")]).size <= 80
    s, names = tc.pass_scores(257)
    assert not np.isnan(s).any()
    neg = [r for r, name in enumerate(names) if name == "neg_inf"]
    assert (s[neg[-1]] == -np.inf).all()
    share = np.isneginf(s[neg[0]]).mean()
    assert 0.45 < share < 0.75 and np.isfinite(s[neg[0]]).sum() < 128 <= max(tc.KS) < 257
    assert all(np.isposinf(s[r]).sum() == 3 for r, name in enumerate(names) if name == "pos_inf")
    const = s[names.index("const")]
    assert (const == const[0]).all()


@pytest.mark.parametrize("n_cols", tc.EXCL_COLS)
@pytest.mark.parametrize("k", tc.EXCL_KS)
def test_winners_in_overflow_needs_the_overflow_scan(n_cols, k):
    s, indptr, indices = tc.excl_inputs("winners_in_overflow", n_cols, k)
    idx_all, _ = tc.ranked(s, k)
    cut = [indices[indptr[r]:indptr[r + 1]][:tc.MAX_EXCL] for r in range(s.shape[0])]
    idx, vals = tc.ranked(s, k, indptr, indices)
    idx_cut, vals_cut = tc.ranked(s, k, *tc.csr(cut))
    for r in range(s.shape[0]):
        lst = indices[indptr[r]:indptr[r + 1]]
        assert lst.size == tc.MAX_EXCL + tc.OVERFLOW_FILL + k // 2
        assert np.unique(lst).size == lst.size
        winners = idx_all[r, :k // 2]
        pos = np.array([np.nonzero(lst == w)[0][0] for w in winners])
        assert (pos >= tc.MAX_EXCL).all()
        assert pos[0] == tc.MAX_EXCL and pos[1] == lst.size - 1   # the scan's first and last
        assert pos.max() - pos.min() > winners.size    # spread among the low scorers
        assert not np.isin(winners, idx[r]).any() and np.isin(winners, idx_cut[r]).all()
        assert (idx[r] != idx_cut[r]).any()
        # nothing staged in LDS matters to the answer: the overflow scan alone decides
        assert not np.isin(lst[:tc.MAX_EXCL], idx_all[r, :2 * k]).any()


@pytest.mark.parametrize("group,n_cols,k",
                         [("excl", n, k) for n in tc.EXCL_COLS for k in tc.EXCL_KS] +
                         [("route", tc.ROUTE_COLS, k) for k in tc.ROUTE_KS])
def test_all_but_leaves_min_k_m(group, n_cols, k):
    if group == "route":
        s, indptr, indices = tc.route_inputs("all_but", k)
    else:
        s, indptr, indices = tc.excl_inputs("all_but", n_cols, k)
    idx, vals = tc.ranked(s, k, indptr, indices)
    ms = tc.all_but_ms(k)
    assert set(ms) == {0, 1, k - 1, k, k + 1, tc.PASS} and s.shape[0] >= len(ms)
    for r in range(s.shape[0]):
        m = ms[r % len(ms)]
        assert indptr[r + 1] - indptr[r] == n_cols - m
        assert (idx[r] >= 0).sum() == min(k, m)
        assert (idx[r, min(k, m):] == -1).all() and np.isneginf(vals[r, min(k, m):]).all()
    if k > tc.PASS:   # runs out in the first pass, exactly at its end, and in a later one
        assert {0, 1, tc.PASS, k - 1} <= set(ms) and tc.PASS < k - 1


@pytest.mark.parametrize("n_cols", tc.EXCL_COLS)
def test_exclusion_lists_are_what_they_claim(n_cols):
    for k in tc.EXCL_KS:
        lists = {}
        for b in tc.BUILDERS:
            s, indptr, indices = tc.excl_inputs(b, n_cols, k)
            assert indptr.dtype == np.int64 and indices.dtype == np.int64
            assert indptr.size == tc.EXCL_ROWS + 1 and indptr[-1] == indices.size
            lists[b] = [indices[indptr[r]:indptr[r + 1]] for r in range(tc.EXCL_ROWS)]
        assert all(x.size == 0 for x in lists["empty"])
        assert [x.size for x in lists["odd_and_even_lengths"]] == list(tc.ODD_EVEN_LENGTHS)
        s, indptr, indices = tc.excl_inputs("odd_and_even_lengths", n_cols, k)
        over = lists["odd_and_even_lengths"][-1]      # its last entry: a first-pass winner
        assert over.size == tc.MAX_EXCL + 1 and over[-1] in tc.ranked(s, k)[0][-1, :tc.PASS]
        assert any((np.diff(x) < 0).any() for x in lists["random"])             # unsorted
        assert all(np.unique(x).size < x.size for x in lists["with_duplicates"])
        assert {x.size % 2 for x in lists["with_duplicates"]} == {0, 1}
        s, indptr, indices = tc.excl_inputs("out_of_range", n_cols, k)
        inside = [x[(x >= 0) & (x < n_cols)] for x in lists["out_of_range"]]
        for x in lists["out_of_range"]:
            assert np.isin([-1, -7, n_cols, n_cols + 5], x).all()
        a = tc.ranked(s, k, indptr, indices)
        b = tc.ranked(s, k, *tc.csr(inside))
        np.testing.assert_array_equal(a[0], b[0])
        # the selective lists remove winners of the first pass and, at k = 100, of the second
        for name in ("random", "with_duplicates", "odd_and_even_lengths", "out_of_range"):
            s, indptr, indices = tc.excl_inputs(name, n_cols, k)
            free, _ = tc.ranked(s, k)
            hit = [np.isin(free[r], lists[name][r]) for r in range(tc.EXCL_ROWS)]
            assert all(h.any() for h in hit), name
            if k > tc.PASS:
                assert all(h[tc.PASS:].any() for r, h in enumerate(hit)
                           if lists[name][r].size >= 2), name


def test_row_group_lists_differ_per_row():
    for n in tc.ROW_COUNTS:
        s, indptr, indices = tc.row_inputs(n)
        lens = np.diff(indptr)
        assert s.shape == (n, tc.ROW_COLS) and lens.size == n
        assert (lens == (7 * np.arange(n)) % (tc.ROW_COLS + 1)).all()
        if n > 1:
            assert (lens[1:] != lens[:-1]).all()
            idx, _ = tc.ranked(s, tc.ROW_K, indptr, indices)
            assert np.unique(idx, axis=0).shape[0] >= n - n // 50  # rows tell each other apart
    assert max(tc.ROW_COUNTS) > 256   # more rows than compute units (256 on an MI355X)


def _naive(row, k, excluded=()):
    cand = [(-float(v), c) for c, v in enumerate(row) if c not in set(excluded)]
    best = sorted(cand)[:k]
    idx = [c for _, c in best] + [-1] * (k - len(best))
    vals = [row[c] for _, c in best] + [-np.inf] * (k - len(best))
    return idx, vals


def test_ranked_agrees_with_a_naive_sort():
    inf = np.inf
    rows = np.array([[3, 1, 3, -2, 0, 3, 1, 7],
                     [-inf, 2, -inf, 2, -inf, -inf, 1, -inf],
                     [-inf] * 8,
                     [inf, 0, inf, -1, 5, inf, -inf, 5],
                     [0.5] * 8,
                     [-0.0, 0.0, -0.0, 1, -1, 0.0, 2, -2]], np.float32)
    lists = [[0, 5], [], [1, 0, 1, 9, -1], [2, 2, 7], [7, 0, 3, 4, 5, 6, 1, 2], [6]]
    indptr, indices = tc.csr(lists)
    for k in (1, 3, 8, 11):
        for ex in (None, lists):
            idx, vals = tc.ranked(rows, k) if ex is None else tc.ranked(rows, k, indptr, indices)
            for r in range(rows.shape[0]):
                ni, nv = _naive(rows[r], k, () if ex is None else ex[r])
                assert idx[r].tolist() == ni, (k, r)
                np.testing.assert_array_equal(vals[r], np.asarray(nv, np.float32))
            tau = tc.kth_eligible(rows, k, *(() if ex is None else (indptr, indices)))
            np.testing.assert_array_equal(tau, vals[:, k - 1])
    rng = np.random.default_rng(0)
    s = rng.integers(-3, 3, (4, 40)).astype(np.float32)
    indptr, indices = tc.csr([rng.choice(40, 7) for _ in range(4)])
    idx, vals = tc.ranked(s, 12, indptr, indices)
    for r in range(4):
        ni, nv = _naive(s[r], 12, indices[indptr[r]:indptr[r + 1]].tolist())
        assert idx[r].tolist() == ni
