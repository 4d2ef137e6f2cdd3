"""Inputs and references shared by tests/test_recommend_cpu.py, tests/test_gpu_recommend.py and
tests/test_gpu_recommend_kernels.py: the CPU file checks, with the algorithm restated on the
host, that these very tables keep every row's candidate count under the cap the GPU tests
run with (they assert overflow_rows == 0), and that every band or share condition a GPU test
leans on holds for its inputs."""
import numpy as np

EPS = 2.0 ** -7 + 2.0 ** -11   # |bf16 approximate score - score| (csrc/recommend.hip)
N_USERS, N_ITEMS = 130, 5000
SAMPLE, CAND_CAP = 1024, 1024
DIMS = (16, 64, 128)
WIDE_D = 160  # dpad > 128: the scoring kernel's other form
KINDS = ("normal", "relu", "lowrank", "midpoint")
KS = (1, 10, 64)
KIND_IDS = {"normal": 0, "relu": 1, "lowrank": 2, "midpoint": 3}


def tables(kind, d, n_users=N_USERS, n_items=N_ITEMS, seed=0):
    """(h_user, h_item) fp32: 'normal', 'relu' (ReLU'd normal), 'lowrank' (rank-4 product,
    ReLU'd), 'midpoint' (every entry halfway between two neighbouring bf16 values)."""
    rng = np.random.default_rng([seed, d, KIND_IDS[kind]])
    if kind in ("normal", "relu"):
        hu = rng.standard_normal((n_users, d))
        hi = rng.standard_normal((n_items, d))
    elif kind == "lowrank":
        basis = rng.standard_normal((4, d))
        hu = rng.standard_normal((n_users, 4)) @ basis
        hi = rng.standard_normal((n_items, 4)) @ basis
    elif kind == "midpoint":
        def mid(shape):  # (1 + (2 j + 1) 2^-8) 2^e, signed: 8 bits of significand after the 1
            j = rng.integers(0, 128, shape)
            e = rng.integers(-3, 4, shape)
            sgn = rng.choice([-1.0, 1.0], shape)
            return sgn * (1.0 + (2 * j + 1) * 2.0 ** -8) * 2.0 ** e
        hu, hi = mid((n_users, d)), mid((n_items, d))
    else:
        raise KeyError(kind)
    if kind in ("relu", "lowrank"):
        hu, hi = np.maximum(hu, 0), np.maximum(hi, 0)
    return hu.astype(np.float32), hi.astype(np.float32)


def exclusions(n_users=N_USERS, n_items=N_ITEMS, lo=0, hi=60, seed=1):
    """Per user `lo`..`hi` distinct random items, unsorted -> (indptr int64, indices int32)."""
    rng = np.random.default_rng(seed)
    lists = [rng.choice(n_items, int(rng.integers(lo, hi + 1)), replace=False)
             for _ in range(n_users)]
    return csr(lists)


def csr(lists):
    indptr = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=indptr[1:])
    flat = np.concatenate([np.asarray(x, np.int32) for x in lists] + [np.zeros(0, np.int32)])
    return indptr, flat.astype(np.int32)


def ranked(scores, indptr, indices, k, rows=None):
    """The definition: per row the k best columns by (score desc, column asc) among those
    not in the row's user's exclusion list, padded with (-1, -inf) -> (idx, vals)."""
    n_rows, n_cols = scores.shape
    idx = np.full((n_rows, k), -1, np.int64)
    vals = np.full((n_rows, k), -np.inf, scores.dtype)
    for r in range(n_rows):
        u = r if rows is None else int(rows[r])
        cols = np.arange(n_cols)
        if indptr is not None:
            cols = np.setdiff1d(cols, indices[indptr[u]:indptr[u + 1]])
        order = cols[np.lexsort((cols, -scores[r, cols]))][:k]
        idx[r, :order.size] = order
        vals[r, :order.size] = scores[r, order]
    return idx, vals


# ---------------------------------------------------------------- references
def cosine64(hu, hi):
    """float64 cosine of every (user, item) pair, rows divided by max(norm, 1e-12)."""
    hu, hi = hu.astype(np.float64), hi.astype(np.float64)
    nu = np.maximum(np.linalg.norm(hu, axis=1, keepdims=True), 1e-12)
    ni = np.maximum(np.linalg.norm(hi, axis=1, keepdims=True), 1e-12)
    return (hu / nu) @ (hi / ni).T


def bf16_bits(x):
    """fp32 array -> bf16 bit patterns (uint16), round to nearest even."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    """bf16 bit patterns (uint16) -> their values as fp32."""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def unit_bf16(x):
    """normalize_rows_bf16 restated on the host: fp32 x / max(norm, 1e-12), rounded to bf16
    (nearest even) -> the bf16 values as fp32 [n, d] (no pad columns)."""
    x = np.asarray(x, np.float32)
    nrm = np.maximum(np.sqrt((x * x).sum(1, keepdims=True, dtype=np.float32)), np.float32(1e-12))
    return bf16_value(bf16_bits(x / nrm))


# the device's fp32 norm (any summation order, d <= 2048 terms, a correctly rounded sqrt and
# divide) is within 2^-20 relative of the float64 norm
NORM_SLACK = 2.0 ** -20
DECIDED = 2.0 ** -12      # relative distance from a bf16 rounding midpoint
BOUND_DIMS = (4, 16, 64, 80, 100, 128, 160, 2048)
BOUND_SCALED = tuple((d, s) for d in (16, 128) for s in (2.0 ** -20, 2.0 ** 20))
NORMALIZE_DIMS = (1, 3, 4, 31, 32, 33, 100, 128)


def bound_tables(kind, d, scale=1.0):
    """The tables of the bound tests: 64 x 2000 (64 x 512 at d = 2048), times `scale` (a
    power of two: exact in fp32)."""
    hu, hi = tables(kind, d, 64, 512 if d == 2048 else 2000)
    s = np.float32(scale)
    return hu * s, hi * s


def normalize_expected(x):
    """The two bf16 patterns normalize_rows_bf16 may give per entry, and the entries whose
    rounding is decided.  The exact result is fp32 x / max(norm, 1e-12) rounded to nearest
    even; the norm's last bits depend on the summation order, so the quotient is bracketed
    with norm64 (1 -+ NORM_SLACK) — rounding is monotonic, the device's value lies between
    the two.  -> (a, b uint16 [n, d], decided bool [n, d]): decided where x / norm64 is at
    least DECIDED relative away from the midpoint of its two neighbouring bf16 values (there
    a and b agree)."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    nrm = np.maximum(np.sqrt((x64 * x64).sum(1, keepdims=True)), np.float64(np.float32(1e-12)))
    a = bf16_bits((x64 / (nrm * (1 - NORM_SLACK))).astype(np.float32))
    b = bf16_bits((x64 / (nrm * (1 + NORM_SLACK))).astype(np.float32))
    q = x64 / nrm
    down = np.ascontiguousarray(q, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    mid = (down | np.uint32(0x8000)).view(np.float32).astype(np.float64)
    decided = np.abs(q - mid) >= DECIDED * np.abs(q)
    return a, b, decided


def normalize_source(d, n=37, seed=0):
    """N(0, 9) rows with a zero row (5) and a row of norm 1e-13 (6, under the guard)."""
    rng = np.random.default_rng([seed, d, n])
    x = (rng.standard_normal((n, d)) * 3).astype(np.float32)
    if n > 6:
        x[5] = 0
        x[6] = (x[6].astype(np.float64) / np.linalg.norm(x[6].astype(np.float64)) * 1e-13)
    return x


def tie_rows():
    """Rows whose norm is 512 in fp32 whatever the summation order (integer entries, squares
    summing to 2^18), with first entry a = 257, 259, .. 511: a / 512 lies exactly halfway
    between two bf16 values, so the tie rule alone decides the output.  -> int-valued fp32
    [128, 5]; the expected bits are bf16_bits(x / 512), exact."""
    two = {}
    for e in range(512):
        for f in range(e + 1):
            two.setdefault(e * e + f * f, (e, f))
    rows = []
    for a in range(257, 512, 2):
        rest = (1 << 18) - a * a
        for b in range(int(rest ** 0.5), -1, -1):
            hit = next((two[rest - b * b - c * c] for c in range(b + 1)
                        if rest - b * b - c * c >= 0 and rest - b * b - c * c in two), None)
            if hit is not None:
                c = next(c for c in range(b + 1) if two.get(rest - b * b - c * c) == hit)
                rows.append([a, b, c, hit[0], hit[1]])
                break
    out = np.asarray(rows, np.float32)
    assert out.shape == (128, 5) and ((out.astype(np.int64) ** 2).sum(1) == 1 << 18).all()
    return out


# ---------------------------------------------------------------- the filter's kept set
FILTER_DIMS = (16, 64, 80, 128, 160)
FILTER_BS = (1, 63, 129, 200)
FILTER_NS = (1, 127, 130, 4096)
FILTER_CAP = 4096
FILTER_BAND = 2.0 ** -16   # above the fp32 accumulation error of <= 160 products of |.| <= 1
FILTER_BAND_SHARE = 1e-3


def filter_tables(d):
    return tables("normal", d, max(FILTER_BS), max(FILTER_NS), seed=5)


def filter_tau(d, B):
    """Per-row thresholds uniform in [-0.3, 0.6]: neighbouring rows differ by far more than
    2 eps.  The last row +inf (keeps nothing), row 0 -inf (keeps everything)."""
    tau = np.random.default_rng([9, d, B]).uniform(-0.3, 0.6, B).astype(np.float32)
    tau[-1] = np.inf
    tau[0] = -np.inf
    return tau


def filter_expected(a64, tau):
    """a64: float64 product of the two bf16 tables.  -> (keep, band): keep[u, v] where
    a64 >= float32(tau_u) - float32(2 eps), the kernel's own fp32 threshold; band where the
    pair is within FILTER_BAND of it and may fall either way."""
    thr = (tau.astype(np.float32) - np.float32(2 * EPS)).astype(np.float64)[:, None]
    with np.errstate(invalid="ignore"):
        band = np.abs(a64 - thr) <= FILTER_BAND
    return a64 >= thr, band


# ---------------------------------------------------------------- recommend's other paths
# name -> (d, n_users, n_items, k, kwargs of recommend, fast_path expected or None)
FALLBACKS = {
    "d100": (100, 16, 600, 10, {}, True),    # a multiple of 4: padded to 128, the fast path
    "d102": (102, 16, 600, 10, {}, False),   # d % 4 != 0
    "d6": (6, 16, 600, 10, {}, False),
    "d2052": (2052, 8, 300, 10, {}, False),
    "d2048": (2048, 8, 300, 10, {}, True),
    "items_below_k": (16, 16, 5, 10, {}, None),
    # a -inf threshold keeps all 600 items: over a cap of 256 every row overflows
    "sample_below_k": (16, 16, 600, 10, {"sample": 4, "cand_cap": 256}, None),
    "one_item": (16, 16, 1, 10, {}, None),
}


def fallback_case(name):
    """-> (hu, hi, (indptr, indices), k, kwargs, fast)."""
    d, n_users, n_items, k, kw, fast = FALLBACKS[name]
    hu, hi = tables("normal", d, n_users, n_items, seed=2)
    excl = exclusions(n_users, n_items, 0, min(20, n_items), seed=3)
    return hu, hi, excl, k, kw, fast
