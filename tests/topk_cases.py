"""Inputs and the definition shared by tests/test_topk_cases_cpu.py and
tests/test_gpu_topk_rows.py: score tables, the ways a device tensor is carved out of an
allocation, exclusion lists, and the named groups of cases the GPU file runs
gnnrec_topk_rows_f32 (csrc/topk.hip) over.  The CPU file checks, with the kernel's loop
conditions restated on the host, that these very inputs reach the paths they are named for.

The order (score desc, column asc) is total, so `ranked` is exact: every comparison in the
GPU file is equality of indices and of the bits of the values.  No NaN appears anywhere."""
import functools

import numpy as np

import recommend_cases as rc

THREADS = 256      # kTopkThreads
MAX_EXCL = 2048    # kMaxExcl: list entries staged in LDS; later ones are scanned in global
PASS = 64          # columns per pass; a pass of <= 16 / <= 32 / <= 64 picks KMAX 16 / 32 / 64
FILL = np.float32(3e38)  # what surrounds a view in its allocation: would win if it were read

COLS = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1027, 3072, 3073, 3076, 3079, 4092, 4096, 4097,
        7168, 7172, 7175, 8195)
KS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 80, 81, 96, 97, 128, 129)
LAYOUTS = ("contig", "prefix", "odd_ld", "shifted")


def ranked(scores, k, indptr=None, indices=None):
    """The definition: per row the k best columns by (score desc, column asc) among those not
    in the row's list, padded with (-1, -inf) -> (idx int64, vals)."""
    return rc.ranked(scores, indptr, indices, k)


def kmax_of_pass(kk):
    return 16 if kk <= 16 else 32 if kk <= 32 else 64


def passes(k):
    """The KMAX of every pass of a call with this k, in order."""
    return [kmax_of_pass(min(PASS, k - c0)) for c0 in range(0, k, PASS)]


# ---------------------------------------------------------------- layouts
def geometry(layout, n_cols):
    """-> (columns of the allocation, first column of the view)."""
    if layout == "contig":
        return n_cols, 0
    if layout == "prefix":    # the next multiple of 4 above n_cols + 4
        return (n_cols + 4) // 4 * 4 + 4, 0
    if layout == "odd_ld":    # = 1 (mod 4), wider than the view
        return n_cols + (1 - n_cols) % 4 + 4, 0
    if layout == "shifted":   # a multiple of 4, the view starts one float in
        return (n_cols + 4) // 4 * 4, 1
    raise KeyError(layout)


def is_vec(layout, n_cols):
    """Whether the launcher picks the float4 scan: a 16-byte aligned base (allocations are)
    and a row stride that is a multiple of 4."""
    width, start = geometry(layout, n_cols)
    return start % 4 == 0 and width % 4 == 0


def embed(scores, layout):
    """-> (allocation [n_rows, width] filled with FILL around the scores, first column)."""
    n_rows, n_cols = scores.shape
    width, start = geometry(layout, n_cols)
    big = np.full((n_rows, width), FILL, np.float32)
    big[:, start:start + n_cols] = scores
    return big, start


# ---------------------------------------------------------------- who scans a column
def owner_vec(c, n_cols):
    c = np.asarray(c)
    n4 = n_cols & ~3
    return np.where(c < n4, (c // 4) % THREADS, (c - n4) % THREADS)


def owner_scalar(c):
    return np.asarray(c) % THREADS


def owner(c, n_cols, vec):
    return owner_vec(c, n_cols) if vec else owner_scalar(c)


def trips(n_cols, vec):
    """The scan's loop conditions restated per thread -> (unrolled, single, scalar) trip
    counts, int arrays [THREADS]: the four-float4 loop, the one-float4 loop after it, and the
    scalar loop (the tail after the float4 loops, or the whole row when not vec)."""
    unrolled = np.zeros(THREADS, np.int64)
    single = np.zeros(THREADS, np.int64)
    scalar = np.zeros(THREADS, np.int64)
    for tid in range(THREADS):
        c_tail = 0
        if vec:
            n4 = n_cols & ~3
            c0 = tid * 4
            while c0 + 3 * THREADS * 4 < n4:
                unrolled[tid] += 1
                c0 += 4 * THREADS * 4
            while c0 < n4:
                single[tid] += 1
                c0 += THREADS * 4
            c_tail = n4
        c = c_tail + tid
        while c < n_cols:
            scalar[tid] += 1
            c += THREADS
    return unrolled, single, scalar


# ---------------------------------------------------------------- score patterns
def _rng(*key):
    return np.random.default_rng([int(x) for x in key])


def normal(n_rows, n_cols, seed):
    """Standard normal, no two entries of a row equal."""
    rng = _rng(1, seed, n_rows, n_cols)
    s = rng.standard_normal((n_rows, n_cols)).astype(np.float32)
    for r in range(n_rows):
        while np.unique(s[r]).size != n_cols:
            s[r] = rng.standard_normal(n_cols).astype(np.float32)
    return s


def ints(n_rows, n_cols, seed):
    return _rng(2, seed, n_rows, n_cols).integers(-40, 40, (n_rows, n_cols)).astype(np.float32)


def const(n_rows, n_cols, seed):
    return np.full((n_rows, n_cols), 1.25, np.float32)


def ascending(n_rows, n_cols, seed):
    """Strictly increasing along the row (halves: exact in fp32): every offer inserts."""
    s = np.arange(n_cols, dtype=np.float64)[None, :] * 0.5 - 100.0 + np.arange(n_rows)[:, None]
    out = s.astype(np.float32)
    assert (out == s).all()
    return out


def descending(n_rows, n_cols, seed):
    return -ascending(n_rows, n_cols, seed)


OWNER_THREADS = (0, 255, 77, 128)  # row r's owner is OWNER_THREADS[r % 4]


def owned_columns(tid, n_cols, vec):
    cols = np.arange(n_cols)
    return cols[owner(cols, n_cols, vec) == tid]


def one_owner_count(k, n_cols, vec):
    """How many of a one_owner row's winners sit with the owner: k, or every column the
    least-endowed owner thread has when that is fewer."""
    return min([k] + [owned_columns(t, n_cols, vec).size for t in OWNER_THREADS])


def one_owner(vec, k):
    """Background `normal`; the largest values of the row, distinct and above the background,
    sit in random order at columns that one thread scans in that layout: one_owner_count of
    them (all k where the thread has k columns, which needs n_cols >= 256 k or so)."""
    def make(n_rows, n_cols, seed):
        s = normal(n_rows, n_cols, seed)
        rng = _rng(3, seed, n_rows, n_cols, k, vec)
        m = one_owner_count(k, n_cols, vec)
        for r in range(n_rows):
            own = owned_columns(OWNER_THREADS[r % 4], n_cols, vec)
            at = rng.choice(own, m, replace=False)
            s[r, at] = 100.0 + rng.permutation(m)
        return s
    return make


def neg_inf(share):
    """`normal` with that share of entries -inf; the last row is -inf throughout."""
    def make(n_rows, n_cols, seed):
        assert n_rows >= 2
        rng = _rng(4, seed, n_rows, n_cols)
        s = normal(n_rows, n_cols, seed)
        s[rng.random((n_rows, n_cols)) < share] = -np.inf
        s[-1] = -np.inf
        return s
    return make


def pos_inf(n_rows, n_cols, seed):
    """`ints` with up to three +inf entries per row."""
    rng = _rng(5, seed, n_rows, n_cols)
    s = ints(n_rows, n_cols, seed)
    for r in range(n_rows):
        s[r, rng.choice(n_cols, min(3, n_cols), replace=False)] = np.inf
    return s


LOOP_BOUNDS = (1024, 3072, 4096, 7168, 8192)  # where a thread's float4 trips begin and end


def edge_columns(n_cols):
    """The columns on either side of every boundary of the scan loops: the row's two ends,
    the last float4 column and the first tail column, and the columns around LOOP_BOUNDS."""
    n4 = n_cols & ~3
    cols = {0, n_cols - 1, n4 - 1, n4}
    for b in LOOP_BOUNDS:
        cols |= {b - 1, b}
    return np.array(sorted(c for c in cols if 0 <= c < n_cols))


def edges(n_rows, n_cols, seed):
    """Background `normal`; the largest values of the row, distinct, sit at edge_columns in
    random order: a scan that drops or mislabels a boundary column loses a winner."""
    s = normal(n_rows, n_cols, seed + 1)
    rng = _rng(13, seed, n_rows, n_cols)
    at = edge_columns(n_cols)
    for r in range(n_rows):
        s[r, at] = 100.0 + rng.permutation(at.size)
    return s


def stack(patterns, n_cols, seed, rows_each=2):
    """Rows of several patterns in one table -> (scores, the pattern's name per row)."""
    parts, names = [], []
    for name, fn in patterns:
        parts.append(fn(rows_each, n_cols, seed))
        names += [name] * rows_each
    return np.vstack(parts), names


# ---------------------------------------------------------------- exclusion lists
def csr(lists):
    """-> (indptr int64, indices int64)."""
    indptr = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=indptr[1:])
    flat = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(0, np.int64)])
    return indptr, flat


def order_of(row):
    """Every column of the row, best first."""
    cols = np.arange(row.size)
    return cols[np.lexsort((cols, -row))]


def _biting(rng, row, k, length):
    """`length` distinct columns, unsorted: one of the row's best min(k, PASS) always, with
    two or more entries one of ranks PASS..k-1 too when k > PASS (so the list removes winners
    of the first pass and of a later one), then about half from the best 2 k and the rest
    from anywhere else."""
    order = order_of(row)
    forced = [order[rng.integers(0, min(k, PASS, row.size))]]
    if k > PASS and length >= 2:
        forced.append(order[rng.integers(PASS, k)])
    forced = np.asarray(forced[:length], np.int64)
    top = np.setdiff1d(order[:2 * k], forced)
    rest = order[2 * k:]
    n_rest = min(rest.size, (length - forced.size) // 2)
    n_top = min(top.size, length - forced.size - n_rest)
    n_rest = length - forced.size - n_top
    out = np.concatenate([forced, rng.choice(top, n_top, replace=False),
                          rng.choice(rest, n_rest, replace=False)])
    assert out.size == length and np.unique(out).size == length
    return rng.permutation(out)


def excl_empty(scores, k, seed):
    return csr([[] for _ in range(scores.shape[0])])


def excl_random(lo, hi):
    def make(scores, k, seed):
        rng = _rng(6, seed, k, *scores.shape)
        n_cols = scores.shape[1]
        return csr([_biting(rng, row, k, min(n_cols, int(rng.integers(lo, hi + 1))))
                    for row in scores])
    return make


def excl_with_duplicates(scores, k, seed):
    """Unsorted lists in which many ids come two or three times; odd and even lengths."""
    rng = _rng(7, seed, k, *scores.shape)
    lists = []
    for r, row in enumerate(scores):
        base = _biting(rng, row, k, min(row.size, 40 + 3 * r))
        again = rng.choice(base, base.size + r % 2)  # total length: even, odd, even, ..
        lists.append(rng.permutation(np.concatenate([base, again])))
    return csr(lists)


ODD_EVEN_LENGTHS = (1, 2, 3, MAX_EXCL - 1, MAX_EXCL, MAX_EXCL + 1)


def excl_odd_and_even_lengths(scores, k, seed):
    """Row r's list has ODD_EVEN_LENGTHS[r % 6] entries: both parities of the odd-even sort,
    and the LDS stage one short of full, full, and one entry over; that one entry, the only
    one left to the global scan, is the best column the list holds."""
    rng = _rng(8, seed, k, *scores.shape)
    assert scores.shape[1] > MAX_EXCL + 1
    lists = []
    for r, row in enumerate(scores):
        lst = _biting(rng, row, k, ODD_EVEN_LENGTHS[r % 6])
        if lst.size > MAX_EXCL:
            rank = np.empty(row.size, np.int64)
            rank[order_of(row)] = np.arange(row.size)
            j = int(np.argmin(rank[lst]))
            lst[[j, MAX_EXCL]] = lst[[MAX_EXCL, j]]
        lists.append(lst)
    return csr(lists)


OUT_OF_RANGE = (-1, -7, 0, 5)  # the last two are added to n_cols


def excl_out_of_range(scores, k, seed):
    """excl_random's lists with -1, -7, n_cols and n_cols + 5 added: they change nothing."""
    n_cols = scores.shape[1]
    rng = _rng(9, seed, k, *scores.shape)
    indptr, flat = excl_random(1, 60)(scores, k, seed)
    extra = np.array([-1, -7, n_cols, n_cols + 5])
    return csr([rng.permutation(np.concatenate([flat[indptr[r]:indptr[r + 1]], extra]))
                for r in range(scores.shape[0])])


def excl_winners_in_overflow(n_fill):
    """The list opens with the row's MAX_EXCL worst columns (they fill the LDS stage); from
    position MAX_EXCL on come the row's best k // 2 columns mixed with n_fill more low
    scorers, the best at position MAX_EXCL itself and the second best last.  Only the global
    scan can remove those winners."""
    def make(scores, k, seed):
        rng = _rng(10, seed, k, *scores.shape)
        lists = []
        for row in scores:
            order = order_of(row)
            assert row.size >= MAX_EXCL + n_fill + 2 * k and k >= 4
            staged = rng.permutation(order[-MAX_EXCL:])
            later = np.concatenate([order[:k // 2],
                                    order[-MAX_EXCL - n_fill:-MAX_EXCL]])
            later = rng.permutation(later)
            # a winner right at position MAX_EXCL and one at the very end: the scan's two ends
            for at, w in ((0, order[0]), (-1, order[1])):
                j = int(np.nonzero(later == w)[0][0])
                later[[at, j]] = later[[j, at]]
            lists.append(np.concatenate([staged, later]))
        return csr(lists)
    return make


def all_but_ms(k):
    """How many columns a row keeps.  With k = 100 the row runs out in the first pass (0, 1),
    exactly at the pass boundary (64) and in the second pass (k - 1); k and k + 1 fill it."""
    return (0, 1, k - 1, k, k + 1, PASS)


def excl_all_but(scores, k, seed):
    """Row r keeps all_but_ms(k)[r % 6] random columns and lists every other one, unsorted."""
    rng = _rng(11, seed, k, *scores.shape)
    n_cols = scores.shape[1]
    lists = []
    for r in range(scores.shape[0]):
        keep = rng.choice(n_cols, all_but_ms(k)[r % 6], replace=False)
        lists.append(rng.permutation(np.setdiff1d(np.arange(n_cols), keep)))
    return csr(lists)


OVERFLOW_FILL = 500
BUILDERS = {
    "empty": excl_empty,
    "random": excl_random(1, 300),
    "with_duplicates": excl_with_duplicates,
    "odd_and_even_lengths": excl_odd_and_even_lengths,
    "out_of_range": excl_out_of_range,
    "winners_in_overflow": excl_winners_in_overflow(OVERFLOW_FILL),
    "all_but": excl_all_but,
}


# ---------------------------------------------------------------- the groups
# A case is (n_cols, layout, k, ...); its inputs come from the *_inputs function of its group,
# cached so that the CPU and GPU files, and every test within one, see the same arrays.
SCAN_KS = (1, 17, 64)
SCAN_CASES = [(n, lay, k) for n in COLS for lay in LAYOUTS for k in SCAN_KS]


@functools.lru_cache(maxsize=None)
def scan_scores(n_cols):
    s, names = stack((("normal", normal), ("ints", ints), ("edges", edges)), n_cols, seed=20)
    s.setflags(write=False)
    return s, names


PASS_COLS = (257, 4097)
PASS_LAYOUT = "prefix"  # the float4 scan with a tail
PASS_CASES = [(n, k) for n in PASS_COLS for k in KS]
NEG_INF_SHARE = 0.6  # at 257 columns fewer than 128 finite scores: -inf columns are returned


@functools.lru_cache(maxsize=None)
def pass_scores(n_cols):
    s, names = stack((("ints", ints), ("const", const), ("neg_inf", neg_inf(NEG_INF_SHARE)),
                      ("pos_inf", pos_inf)), n_cols, seed=21)
    s.setflags(write=False)
    return s, names


# 25603 columns give every thread 100 of them in either scan, so that one thread can hold all
# the winners of a 64-column pass (and of the 33-column pass after it); at 4096 and 8195 a
# thread scans 16 and 32 columns, which fills a KMAX = 16 and a KMAX = 32 list
INSERT_KS = (16, 32, 64, 97)
INSERT_COLS = (4096, 8195, 25603)
INSERT_LAYOUTS = ("prefix", "odd_ld")  # the float4 scan and the scalar scan
INSERT_CASES = [(n, lay, k) for n in INSERT_COLS for lay in INSERT_LAYOUTS for k in INSERT_KS]


@functools.lru_cache(maxsize=None)
def insert_scores(n_cols, layout, k):
    vec = is_vec(layout, n_cols)
    pats = [("one_owner", one_owner(vec, k))]
    if n_cols != INSERT_COLS[-1]:
        pats = [("ascending", ascending), ("descending", descending)] + pats
    s, names = stack(tuple(pats), n_cols, seed=22, rows_each=4 if len(pats) == 1 else 2)
    s.setflags(write=False)
    return s, names


EXCL_KS = (10, 32, 100)
EXCL_COLS = (3079, 4097)
EXCL_LAYOUTS = ("contig", "odd_ld", "prefix")  # the first two scan scalar, prefix by float4
EXCL_ROWS = 6
EXCL_CASES = [(b, n, lay, k) for b in BUILDERS for n in EXCL_COLS for lay in EXCL_LAYOUTS
              for k in EXCL_KS]


@functools.lru_cache(maxsize=None)
def excl_inputs(builder, n_cols, k):
    """-> (scores [EXCL_ROWS, n_cols], indptr, indices): rows 0-2 `normal`, rows 3-5 `ints`."""
    s = np.vstack([normal(3, n_cols, 23), ints(3, n_cols, 23)])
    indptr, indices = BUILDERS[builder](s, k, 23)
    for a in (s, indptr, indices):
        a.setflags(write=False)
    return s, indptr, indices


ROW_COUNTS = (1, 300, 1025)   # 1025: more rows than the device has compute units
ROW_COLS, ROW_K = 257, 17
ROW_LAYOUTS = ("contig", "prefix")
ROW_CASES = [(n, lay) for n in ROW_COUNTS for lay in ROW_LAYOUTS]


@functools.lru_cache(maxsize=None)
def row_inputs(n_rows):
    """`normal` rows; row r lists (7 r) % 258 columns: every length from none to all."""
    s = normal(n_rows, ROW_COLS, 24)
    rng = _rng(12, n_rows)
    indptr, indices = csr([rng.permutation(ROW_COLS)[:(7 * r) % (ROW_COLS + 1)]
                           for r in range(n_rows)])
    for a in (s, indptr, indices):
        a.setflags(write=False)
    return s, indptr, indices


# two routes, one answer: finite scores, contiguous
ROUTE_KS = (10, 100)
ROUTE_COLS = 4096
ROUTE_BUILDERS = ("random", "all_but")
ROUTE_CASES = [(b, k) for b in ROUTE_BUILDERS for k in ROUTE_KS]


@functools.lru_cache(maxsize=None)
def route_inputs(builder, k):
    s = np.vstack([normal(5, ROUTE_COLS, 25), ints(5, ROUTE_COLS, 25)])
    indptr, indices = BUILDERS[builder](s, k, 25)
    for a in (s, indptr, indices):
        a.setflags(write=False)
    return s, indptr, indices


def kth_eligible(scores, k, indptr=None, indices=None):
    """tau: per row the k-th largest score among the columns not listed, -inf with fewer
    than k of them.  A plain sort of the values, independent of `ranked`."""
    out = np.full(scores.shape[0], -np.inf, np.float32)
    for r, row in enumerate(scores):
        keep = np.ones(row.size, bool)
        if indptr is not None:
            ids = indices[indptr[r]:indptr[r + 1]]
            keep[ids[(ids >= 0) & (ids < row.size)]] = False
        v = np.sort(row[keep])[::-1]
        if v.size >= k:
            out[r] = v[k - 1]
    return out
