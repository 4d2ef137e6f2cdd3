"""The load launch of gnnrec_spmm_project_agg_f32 (spmm_project_load_mfma_kernel): the
projection of the kept aggregates on v_mfma_f32_32x32x2_f32, whose k-slot 0 carries the self
row and W_self and k-slot 1 the aggregate and W_neigh, so that every output element runs the
VALU kernel's fmaf chain.

Everything is compared bitwise (torch.equal on the int32 views) against the plain gathering
launch, ops.spmm_project(..., variant="valu") without agg; the load launch reads the aggregate
that a save launch of the same arguments wrote (tests/test_gpu_project_agg.py's method).

Shapes: row counts across the 32-row tile (1, 31, 32, 33, 63, 64, 65), 4099, and BIG = four
tiles for each of 2 x 256 blocks plus one odd row, the smallest count at which 512 blocks draw
their tiles from the row queue (rowq_slot_for: n_dst >= 4 tickets x 32 rows x blocks), so every
block's double buffer wraps and the queue hands out about 2050 tickets; BIG runs under both
schedules and the queued run asserts that the queue was taken.  Rows include empty ones
(bias_nonempty), the first rows of every CSR among them.  Every accumulate mode, bias /
bias_nonempty and ReLU / L2 norm on and off; row strides of 132 and 256 floats for H, agg and
out; poisoned and absent X / indices / edge weights.

Inputs, chosen so that a reordered sum shows: randn tables; a table whose columns are scaled
by powers of two over +-20 binades (the weights' rows by other powers); a table with
subnormals and -0.0 in H, the aggregate and the weights, with rows that are subnormal
throughout (a flushed operand would zero them).  Finite inputs only: what the MFMA does with
NaN payloads is not pinned."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D, N_SRC = 128, 3000
ROWS = [1, 31, 32, 33, 63, 64, 65, 4099]
BIG = 4 * 32 * 2 * 256 + 1
ACCUMS = ["store", "add", "max", "attn_first", "attn", "attn_last"]
FLAGS = list(itertools.product((False, True), repeat=4))  # bias, bias_nonempty, relu, l2


def _bits(t):
    return t.contiguous().view(torch.int32)


def _csr(n_dst, rng):
    """Degrees 0..8; rows 0, 4, 8, ... are empty and rows 1, 5, 9, ... have one edge (their
    sum is a source row's bits).  The one-row CSR's row has three."""
    deg = rng.integers(0, 9, n_dst).astype(np.int64)
    deg[::4] = 0
    deg[1::4] = 1
    if n_dst == 1:
        deg[0] = 3
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ix = rng.integers(0, N_SRC, int(ip[-1])).astype(np.int32)
    return torch.from_numpy(ip).cuda(), torch.from_numpy(ix).cuda()


def _tables(kind, g):
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    t = {"X": r(N_SRC, D), "Ws": r(D, D) / 11, "Wn": r(D, D) / 11, "bias": r(D), "bias_ne": r(D),
         "attn_vec": r(D) / 11}
    if kind == "binades":
        e = torch.randint(-20, 21, (3, D), device="cuda", generator=g).float()
        t["X"] = t["X"] * torch.exp2(e[0])
        t["Ws"] = t["Ws"] * torch.exp2(e[1])  # W[j][k]: input column k scaled
        t["Wn"] = t["Wn"] * torch.exp2(e[2])
        t["hscale"] = torch.exp2(e[0].flip(0))
    if kind == "subnormal":
        def sprinkle(x):
            m = torch.rand(x.shape, device="cuda", generator=g)
            x = torch.where(m < 0.2, x * 1e-40, x)      # subnormal entries
            return torch.where(m > 0.9, -torch.zeros_like(x), x)  # -0.0
        t["X"] = sprinkle(t["X"])
        t["X"][::3] = r(N_SRC, D)[::3] * 1e-40          # source rows subnormal throughout
        t["Ws"], t["Wn"] = sprinkle(t["Ws"]), sprinkle(t["Wn"])
        t["Ws"][::7] = t["Ws"][::7] * 2.0 ** 20         # subnormal x weight: a normal product
        t["sprinkle"] = sprinkle
    return t


def _shape(t, n, rng, g):
    ip, ix = _csr(n, rng)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    H = r(n, D)
    if "hscale" in t:
        H = H * t["hscale"]
    if "sprinkle" in t:
        H = t["sprinkle"](H)
        H[1::4] = r(n, D)[1::4] * 1e-40  # the degree-1 rows: subnormal throughout
    state = torch.stack([r(n), torch.rand(n, device="cuda", generator=g) + 1], 1)
    return ip, ix, H, r(n, D), state


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(11)
    g = torch.Generator(device="cuda").manual_seed(5)
    out = {}
    for kind in ("randn", "binades", "subnormal"):
        t = _tables(kind, g)
        t["csr"] = {n: _shape(t, n, rng, g) for n in (ROWS if kind == "randn" else [65, 4099])}
        out[kind] = t
    out["randn"]["csr"][BIG] = _shape(out["randn"], BIG, rng, g)
    assert all(torch.isfinite(v).all() for t in out.values()
               for v in (t["X"], t["Ws"], t["Wn"]))
    return out


def _strided(x, ld):
    """x's values in a view of row stride ld floats."""
    if ld == D:
        return x.clone()
    v = torch.full((x.shape[0], ld), 7.0, device="cuda")[:, :D]
    v.copy_(x)
    return v


def _sweep(t, n, reduce, accums, flags, ld=(D, D, D), poisoned=False):
    """Plain launch vs save launch + load launch over accums x flags; the failing cases."""
    from gnnrec import ops
    ip, ix, H, out0, state0 = t["csr"][n]
    ldh, lda, ldo = ld
    Hs = _strided(H, ldh)
    bad = []
    agg = None
    for accum, (b, bne, relu, l2) in itertools.product(accums, flags):
        attn = accum.startswith("attn")

        def launch(H_=H, out=None, X=t["X"], indices=ix, **kw):
            st = state0.clone() if attn else None
            o = ops.spmm_project(
                ip, indices, X, H_, t["Ws"], t["Wn"], reduce, None, relu=relu, l2norm=l2,
                accum=accum, out=out0.clone() if out is None else out,
                bias=t["bias"] if b else None, bias_nonempty=t["bias_ne"] if bne else None,
                attn_vec=t["attn_vec"] if attn else None, attn_state=st, variant="valu", **kw)
            return o, st

        def same(a, b_):
            return torch.equal(_bits(a[0]), _bits(b_[0])) and \
                (not attn or torch.equal(_bits(a[1]), _bits(b_[1])))

        plain = launch()
        what = (n, reduce, accum, b, bne, relu, l2, ld)
        if agg is None:  # the aggregate no weight or flag enters: saved once per sweep
            agg = _strided(torch.full((n, D), 3.0, device="cuda"), lda)
            if not same(launch(agg=agg, agg_mode="save"), plain):
                bad.append(("save output",) + what)
        if not same(launch(H_=Hs, out=_strided(out0, ldo), agg=agg, agg_mode="load"), plain):
            bad.append(("load output",) + what)
        if poisoned:
            X_nan = torch.full_like(t["X"], float("nan"))
            ix_bad = torch.full_like(ix, 1 << 30)
            if not same(launch(X=X_nan, indices=ix_bad, agg=agg, agg_mode="load"), plain):
                bad.append(("load output, poisoned sources",) + what)
            if not same(launch(X=None, indices=None, agg=agg, agg_mode="load"), plain):
                bad.append(("load output, sources absent",) + what)
    return bad


@pytest.mark.parametrize("n_dst", ROWS)
def test_load_launch_has_the_plain_launch_bits(data, n_dst):
    """Every accumulate mode x bias x bias_nonempty x ReLU x L2 at every row count."""
    from gnnrec import ops
    with ops.concurrency(0, False):
        bad = _sweep(data["randn"], n_dst, "mean", ACCUMS, FLAGS)
    assert not bad, bad[:10]


@pytest.mark.parametrize("queued", [False, True], ids=["static", "queue"])
def test_many_tiles_per_block_under_both_schedules(data, queued):
    """BIG rows: each block walks several tiles (the double buffer wraps); queued, the blocks
    draw them as tickets."""
    from gnnrec import ops
    flags = [(True, True, True, True), (False, True, False, False), (True, False, False, True)]
    q0, _ = ops.rowq_stats()
    with ops.concurrency(0, queued):
        bad = _sweep(data["randn"], BIG, "mean", ACCUMS, flags)
        torch.cuda.synchronize()
    took = ops.rowq_stats()[0] - q0
    assert not bad, bad[:10]
    if queued:  # 6 x 3 load launches, and as many plain ones, each with its own slot
        assert took >= len(ACCUMS) * len(flags), took
    else:
        assert took == 0, took


@pytest.mark.parametrize("ld", [(132, 132, 132), (256, 132, D), (D, 256, 256)],
                         ids=lambda v: "ld%d_%d_%d" % v)
def test_row_strides_above_the_row_width(data, ld):
    """H, agg and out with rows of 132 and 256 floats."""
    from gnnrec import ops
    flags = [(True, True, True, True), (False, False, False, False)]
    with ops.concurrency(0, False):
        bad = [x for n in (33, 4099)
               for x in _sweep(data["randn"], n, "mean", ["store", "add", "attn"], flags, ld=ld)]
    assert not bad, bad[:10]


def test_load_launch_reads_no_source(data):
    """X and indices poisoned (NaN rows, out-of-range ids), and absent."""
    from gnnrec import ops
    flags = [(True, True, True, True), (False, False, False, False)]
    with ops.concurrency(0, False):
        bad = [x for n in (1, 65, 4099)
               for x in _sweep(data["randn"], n, "mean", ["store", "max"], flags, poisoned=True)]
    assert not bad, bad[:10]


@pytest.mark.parametrize("kind", ["binades", "subnormal"])
@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_inputs_that_show_a_reordered_sum(data, kind, reduce):
    """Columns over +-20 binades; subnormals and -0.0 in H, the aggregate and the weights."""
    from gnnrec import ops
    t = data[kind]
    if kind == "subnormal":  # the inputs are what the docstring says they are
        tiny = torch.finfo(torch.float32).tiny
        H = t["csr"][4099][2]
        for x in (H, t["X"], t["Ws"], t["Wn"]):
            assert ((x != 0) & (x.abs() < tiny)).any() and ((x == 0) & torch.signbit(x)).any()
    with ops.concurrency(0, False):
        bad = [x for n in (65, 4099) for x in _sweep(t, n, reduce, ["store", "add"], FLAGS)]
    assert not bad, bad[:10]
