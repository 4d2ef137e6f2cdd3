"""Inputs, bounds and host restatements shared by tests/test_recommend_pop_cpu.py and
tests/test_gpu_recommend_pop.py (popularity-weighted many-user top-k).  Tables,
exclusions and ranked() come from tests/recommend_cases.py, the head from
tests/recommend_mlp_cases.py.  The CPU file shows on the host, for these very inputs, what the
GPU tests lean on: the band |Ra - R| <= delta_u, candidate counts far under the cap the exact
tests run with, the overflow case overflowing (and not, with the popular sample), the gaps of
the lists compared with get_recs."""
import math

import numpy as np

import recommend_cases as rc

SAMPLE = 1024
POP_SAMPLE = 256
CAND_CAP = 2048            # the exact-ranking tests; the host shows no row above CAND_CAP / 2
POPS = ("sparse", "dense", "dominant", "zero")
WEIGHTS = {"sparse": 0.05, "dense": 4e-4, "dominant": 0.5, "zero": 1.0}
POP_IDS = {"sparse": 0, "dense": 1, "dominant": 2, "zero": 3}
BATCHES = (1, 64, 130, 8192)
Z_ITEMS = (1, 31, 33, 257, 5000)
Z_USERS = (1, 63, 65, 130)
PART_ITEMS = 1024          # items per partial sum of a denominator (csrc/recommend_pop.hip)

# the library's band (csrc/recommend.hip, THE RATING BAND): |Ra - R| <= delta_u =
# RATING_BAND / Z_u + RATING_SLACK max(p)
RATING_BAND = math.exp(1.0 + rc.EPS) * (math.expm1(rc.EPS) + 2.0 ** -20)
RATING_SLACK = 2.0 ** -22


def popularity(name, n_items=rc.N_ITEMS, seed=0):
    """-> (popularity fp32 [n_items], weight).  sparse: 5 % of the items non-zero, Zipf(1.5)
    counts over their sum (as the reference builds it); dense, dominant: uniform [0, 1);
    zero."""
    rng = np.random.default_rng([seed, 77, POP_IDS[name], n_items])
    pop = np.zeros(n_items, np.float64)
    if name == "sparse":
        nz = rng.choice(n_items, max(1, n_items // 20), replace=False)
        counts = rng.zipf(1.5, nz.size).astype(np.float64)
        pop[nz] = counts / counts.sum()
    elif name in ("dense", "dominant"):
        pop = rng.random(n_items)
    return pop.astype(np.float32), WEIGHTS[name]


def p_vector(pop, weight):
    """p_v = popularity[v] * weight: one fp32 multiply."""
    return (pop.astype(np.float32) * np.float32(weight)).astype(np.float32)


def block_popularity(n_items=rc.N_ITEMS, lo=4000, seed=3):
    """The overflow case: popularity uniform on [lo, n_items), zero elsewhere; weight 0.5."""
    pop = np.zeros(n_items, np.float32)
    pop[lo:] = np.random.default_rng(seed).random(n_items - lo).astype(np.float32)
    return pop, 0.5


def parts(n_items):
    return (n_items + PART_ITEMS - 1) // PART_ITEMS


# ---------------------------------------------------------------- bounds, derived
# Z against the fp64 sum of exp over g.  Every term is positive, so a sum's relative error is
# at most (the longest chain of additions a term passes through) x 2^-24, plus each term's
# own relative error.
#   expf: within 2 ulp, 2^-22 relative.
#   cosine head: g is an fp32 MFMA dot product of d terms with sum |x_c y_c| <= 1 (unit
#     rows); the MFMA's internal rounding is not documented, so one unit 2^-23 per term (it
#     covers truncation as well as nearest): |g - g64| <= d 2^-23, and exp moves by that
#     relative amount (e^x - 1 <= 1.001 x there).  Chain: 8 subtiles in a lane, 5 tree levels,
#     3 wave adds, parts - 1 folds.
#   MLP head: g is the stored score itself, no term for it.  Chain: 5 tree levels, 32 tiles
#     into the user's sum, parts - 1 folds.
def z_rel_bound(head, d, n_items):
    if head == "cos":
        return 1.001 * d * 2.0 ** -23 + 2.0 ** -22 + (8 + 5 + 3 + parts(n_items)) * 2.0 ** -24
    return 2.0 ** -22 + (5 + 32 + parts(n_items)) * 2.0 ** -24


def r_abs_bound(soft64, R64, zrel):
    """|R_device - R64| for R64 = exp(score) / Z64 + p in fp64 from the device's score, Z64
    the fp64 denominator: expf 2^-22 and the divide 2^-24 relative to the softmax term, the
    relative error of Z times it, and half an ulp (2^-24 relative) of R; 1.01 for the second
    order."""
    return 1.01 * (soft64 * (2.0 ** -22 + 2.0 ** -24 + zrel) + np.abs(R64) * 2.0 ** -24)


# ---------------------------------------------------------------- host restatements
def sample_columns(p, sample, pop_sample):
    """The threshold sample's item ids, ascending: the prefix and the pop_sample items of
    largest p outside it, ties by id."""
    n = p.size
    m = min(sample, n)
    rest = np.arange(m, n)
    extra = rest[np.lexsort((rest, -p[m:].astype(np.float64)))][:min(pop_sample, n - m)]
    return np.concatenate([np.arange(m), np.sort(extra)]).astype(np.int64)


def ratings64(S, p):
    """exp(S) / sum_v exp(S) + p in float64 -> (R, Z)."""
    E = np.exp(S.astype(np.float64))
    Z = E.sum(1)
    return E / Z[:, None] + p.astype(np.float64)[None, :], Z


def filter_counts(Ra, R, Z, p, indptr, indices, k, sample, pop_sample, band):
    """recommend(popularity=)'s filter on the host: tau = the k-th best non-excluded Ra of the
    sample columns, kept = Ra >= tau - 2 delta (delta = 0 without a band: the MLP head, where
    Ra is R).  -> (counts per row, whether every row's exact top k of R is inside its kept
    set)."""
    U, n = R.shape
    cols = sample_columns(p, sample, pop_sample)
    pmax = float(np.abs(p).max()) if p.size else 0.0
    counts = np.zeros(U, np.int64)
    inside = True
    for r in range(U):
        ex = indices[indptr[r]:indptr[r + 1]] if indptr is not None else np.zeros(0, np.int64)
        ok = np.ones(n, bool)
        ok[ex] = False
        pre = Ra[r, cols][ok[cols]]
        tau = np.sort(pre)[::-1][k - 1] if pre.size >= k else -np.inf
        delta = (RATING_BAND / Z[r] + RATING_SLACK * pmax) if band else 0.0
        keep = Ra[r] >= tau - 2 * delta
        counts[r] = keep.sum()
        elig = np.nonzero(ok)[0]
        top = elig[np.lexsort((elig, -R[r, elig]))][:k]
        inside = inside and bool(keep[top].all())
    return counts, inside


def approx_and_score(hu, hi):
    """(a, score) in float64: the product of the two bf16-rounded unit tables, and the
    float64 cosine."""
    a = rc.unit_bf16(hu).astype(np.float64) @ rc.unit_bf16(hi).astype(np.float64).T
    return a, rc.cosine64(hu, hi)


# ---------------------------------------------------------------- other cases
OVERFLOW = dict(kind="normal", d=64, k=10, sample=256, cand_cap=256)
# 'dominant' without exclusions: the k most popular items for every user.  It holds for a k
# whose k-th and (k + 1)-th largest p are further apart than any softmax term can bridge; the
# CPU file checks that for this k.
DOMINANT_K = 10
EDGE_D = 64
# the MLP head against get_recs(pred='nn', use_popularity=True): tables of this seed, for
# which the CPU file shows every list's relative gaps through rank k + 1 above MLP_REF_GAP
# (seeds tried on the host from 0 upwards: seed 0 has a gap of 7.6e-7, seed 1 4.6e-5)
MLP_REF = dict(seed=1, d=16, n_users=40, n_items=300, k=10, weight=2e-3)
MLP_REF_GAP = 1e-5


def mlp_ref_case():
    s = MLP_REF
    hu, hi = rc.tables("normal", s["d"], s["n_users"], s["n_items"], seed=100 + s["seed"])
    pop = np.random.default_rng([s["seed"], 5]).random(s["n_items"]).astype(np.float32)
    excl = rc.exclusions(s["n_users"], s["n_items"], 0, 20, seed=200 + s["seed"])
    return hu, hi, pop, excl
