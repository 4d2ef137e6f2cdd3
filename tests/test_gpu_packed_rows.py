"""Packed rows on the GPU (d = 128): pack_rows equals the host routine byte for byte and
settles packed_ok / the dense-row count; the packed gather is bitwise the dense gather —
sum and mean, with and without accumulate-into-partial, through the heavy-row chunk path,
under the static schedule and the row queue, with `dense`-flagged source rows sharing steps
with packed ones, and through the dense fallback loop of a table whose packed_ok is 0."""
import numpy as np
import pytest
import torch

from packed_rows_cases import DENSE_BIT, relu_table, row_with_nnz, source_table

pytestmark = pytest.mark.gpu

N_SRC, N_DST = 300, 70
DEGREES = (0, 1, 2, 7, 8, 9, 63, 64, 65, 129)  # cross the 8-edge step and the 64-index chunk
HEAVY = 1100                                    # > TILE_SPLIT (512): the chunk kernels run


def _bits(t):
    return t.view(torch.int32)


@pytest.fixture(scope="module")
def src():
    """The 300-row source table (host and device) with every nnz case and flagged rows."""
    x = source_table(np.random.default_rng(0), N_SRC)
    return x, torch.from_numpy(x).cuda()


@pytest.fixture(scope="module")
def csr():
    """70 destination rows: the listed degrees seven times over, one of them ≈1100 edges."""
    g = torch.Generator().manual_seed(5)
    deg = torch.tensor(DEGREES * 7, dtype=torch.int64)[torch.randperm(N_DST, generator=g)]
    deg[17] = HEAVY
    indptr = torch.zeros(N_DST + 1, dtype=torch.int64)
    torch.cumsum(deg, 0, out=indptr[1:])
    indices = torch.randint(0, N_SRC, (int(indptr[-1]),), generator=g, dtype=torch.int32)
    return indptr.cuda(), indices.cuda()


@pytest.fixture
def static_mode():
    from gnnrec import ops
    old = ops.get_concurrency()
    ops.set_concurrency(0, False)
    yield
    ops.set_concurrency(*old)


def test_pack_equals_the_host_routine(src):
    from gnnrec import ops
    x, X = src
    ref, dense = ops.pack_rows_host(x)
    P = ops.pack_rows(X)
    got = P.data.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got, ref)
    assert dense > 40  # every 7th row and the nnz 89 / 128 cases
    assert P.status.tolist() == [0, dense, 0, 0]  # above the default fraction; counters reset
    # a strided view of a wider buffer packs the same rows
    wide = torch.zeros(N_SRC, 160, device="cuda")
    wide[:, :128] = X
    np.testing.assert_array_equal(ops.pack_rows(wide[:, :128]).data.cpu().numpy().view(np.uint32),
                                  ref)


def test_packed_ok_and_dense_count():
    """all-sparse, all-dense, and a table exactly at the chosen fraction (and one row above)."""
    from gnnrec import ops
    rng = np.random.default_rng(1)
    n = 640
    limit = int(ops.PACK_MAX_DENSE_FRAC * n)
    assert limit >= 1
    sparse = relu_table(rng, n, 0.6)
    sparse[(sparse != 0).sum(1) > 88] = 0.0

    def status(x, **kw):
        P = ops.pack_rows(torch.from_numpy(x).cuda(), **kw)
        return P.status.tolist()

    assert status(sparse) == [1, 0, 0, 0]
    assert status(np.ones((n, 128), dtype=np.float32)) == [0, n, 0, 0]
    at = sparse.copy()
    for r in rng.permutation(n)[:limit]:
        at[r] = row_with_nnz(rng, 89)
    assert status(at) == [1, limit, 0, 0]
    over = at.copy()
    over[np.nonzero((at != 0).sum(1) <= 88)[0][0]] = row_with_nnz(rng, 128)
    assert status(over) == [0, limit + 1, 0, 0]
    assert status(over, max_dense_frac=1.0) == [1, limit + 1, 0, 0]
    # the buffers are reused: the counters start from zero again
    P = ops.pack_rows(torch.from_numpy(over).cuda())
    ops.pack_rows(torch.from_numpy(sparse).cuda(), into=P)
    assert P.status.tolist() == [1, 0, 0, 0]


def _packed(X, force_ok=True):
    """X packed with packed_ok = 1 whatever its share of flagged rows, so the packed loop and
    its escape to the dense table run."""
    from gnnrec import ops
    return ops.pack_rows(X, max_dense_frac=1.0 if force_ok else None)


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("split", [512, None])
def test_spmm_packed_bitwise(static_mode, src, csr, reduce, split):
    from gnnrec import ops
    _, X = src
    indptr, indices = csr
    P = _packed(X)
    assert P.status[0].item() == 1 and P.status[1].item() > 0
    ref = ops.spmm(indptr, indices, X, reduce, split=split)
    out = ops.spmm_packed(indptr, indices, P, reduce, split=split)
    assert torch.equal(_bits(ref), _bits(out))
    # accumulate into a partial (a source tile onto the tiles before it)
    base = torch.randn(N_DST, 128, device="cuda")
    o_ref, o = base.clone(), base.clone()
    ops.spmm(indptr, indices, X, reduce, out=o_ref, accumulate=True, split=split)
    ops.spmm_packed(indptr, indices, P, reduce, out=o, accumulate=True, split=split)
    assert torch.equal(_bits(o_ref), _bits(o))


def test_spmm_packed_device_plan(static_mode, src, csr):
    """the heavy-row plan built on the device (the pass's tiles carry their edge count)"""
    from gnnrec import ops
    _, X = src
    indices = csr[1]
    ref = ops.spmm(csr[0], indices, X, "sum", split=512)
    indptr = csr[0].clone()  # no host plan cached on it
    indptr._gnnrec_nnz = indices.numel()
    out = ops.spmm_packed(indptr, indices, _packed(X), "sum", split=512)
    assert torch.equal(_bits(ref), _bits(out))


@pytest.mark.parametrize("accumulate", [False, True])
def test_spmm_packed_row_queue(static_mode, src, accumulate):
    """Enough rows for the launch to take the queue (>= 32 per wave of the grid)."""
    from gnnrec import ops
    _, X = src
    n_dst = 400_000
    g = torch.Generator().manual_seed(7)
    deg = torch.randint(0, 13, (n_dst,), generator=g)
    indptr = torch.zeros(n_dst + 1, dtype=torch.int64)
    torch.cumsum(deg, 0, out=indptr[1:])
    indices = torch.randint(0, N_SRC, (int(indptr[-1]),), generator=g, dtype=torch.int32)
    indptr, indices = indptr.cuda(), indices.cuda()
    P = _packed(X)
    base = torch.randn(n_dst, 128, device="cuda")

    def run(fn, **kw):
        o = base.clone()
        fn(out=o, accumulate=accumulate, split=None, **kw)
        return o
    ref = run(lambda **kw: ops.spmm(indptr, indices, X, "mean", **kw))
    static = run(lambda **kw: ops.spmm_packed(indptr, indices, P, "mean", **kw))
    q0, _ = ops.rowq_stats()
    with ops.concurrency(16, True):
        queued = run(lambda **kw: ops.spmm_packed(indptr, indices, P, "mean", **kw))
    torch.cuda.synchronize()
    assert ops.rowq_stats()[0] > q0  # the launch did take the queue
    assert torch.equal(_bits(ref), _bits(static))
    assert torch.equal(_bits(ref), _bits(queued))


@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_all_dense_table_takes_the_fallback_loop(static_mode, csr, reduce):
    from gnnrec import ops
    indptr, indices = csr
    X = torch.randn(N_SRC, 128, device="cuda")
    P = ops.pack_rows(X)
    assert P.status.tolist() == [0, N_SRC, 0, 0]
    assert not (P.data.cpu().numpy().view(np.uint32)[:, 8:]).any()  # no values were stored
    assert ((P.data.cpu().numpy().view(np.uint32)[:, 5] & DENSE_BIT) != 0).all()
    ref = ops.spmm(indptr, indices, X, reduce, split=512)
    out = ops.spmm_packed(indptr, indices, P, reduce, split=512)
    assert torch.equal(_bits(ref), _bits(out))
    # and the same table through the packed loop: every row escapes to the dense table
    out = ops.spmm_packed(indptr, indices, _packed(X), reduce, split=512)
    assert torch.equal(_bits(ref), _bits(out))


def test_packed_rejects_what_it_does_not_cover(src, csr):
    from gnnrec import ops
    _, X = src
    with pytest.raises(ValueError):
        ops.pack_rows(torch.zeros(8, 64, device="cuda"))
    with pytest.raises(ValueError):
        ops.spmm_packed(csr[0], csr[1], _packed(X), "max")


@pytest.fixture(scope="module")
def small_graph():
    """2000 users x 300 items x 20k edges per direction, a 3-layer d = 128 'mean' model."""
    from gnnrec import nn as gnn
    from gnnrec.graph import HeteroGraph
    rng = np.random.default_rng(0)
    n_u, n_i, E, d = 2000, 300, 20000, 128
    u, i = rng.integers(0, n_u, E), rng.integers(0, n_i, E)
    rels = {("user", "buys", "item"): (u, i), ("item", "bought-by", "user"): (i, u)}
    g = HeteroGraph({ce: (torch.from_numpy(s), torch.from_numpy(t)) for ce, (s, t) in rels.items()},
                    {"user": n_u, "item": n_i}, device="cuda")
    feats = {"user": torch.from_numpy(rng.standard_normal((n_u, d)).astype(np.float32)).cuda(),
             "item": torch.from_numpy(rng.standard_normal((n_i, d)).astype(np.float32)).cuda()}
    torch.manual_seed(0)
    model = gnn.ConvModel(g, 3, {"user": d, "item": d, "hidden": d, "out": d}, True, 0.0, "mean",
                          "cos", "sum", True).cuda().eval()
    return g, feats, model


def _run_pass(g, feats, model, deterministic, packed, monkeypatch):
    from gnnrec.dist import Exchange
    from gnnrec.inference import GraphShard, ShardedFullGraphPass
    monkeypatch.setenv("GNNREC_PACKED_ROWS", "1" if packed else "0")
    sh = GraphShard.from_graph(g, 0, 1, "user", device="cuda", segments=8)
    runner = ShardedFullGraphPass(model, sh, Exchange(), deterministic=deterministic)
    out = runner.run(sh.local_features(feats))
    out = runner.run(sh.local_features(feats))  # the second pass reuses the packed buffers
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}, runner


@pytest.mark.parametrize("deterministic", [True, False])
@pytest.mark.parametrize("dense", [False, True])
def test_pass_packed_equals_dense_bitwise(small_graph, monkeypatch, deterministic, dense):
    import copy
    g, feats, model = small_graph
    if dense:
        # every weight and feature positive: no pre-activation is negative, the ReLU zeroes
        # nothing and every hidden row is flagged — the tables' packed_ok comes out 0
        model = copy.deepcopy(model)
        with torch.no_grad():
            for p in model.parameters():
                p.abs_()
        feats = {k: v.abs() for k, v in feats.items()}
    off, r_off = _run_pass(g, feats, model, deterministic, False, monkeypatch)
    on, r_on = _run_pass(g, feats, model, deterministic, True, monkeypatch)
    assert not r_off.packed and not r_off._pack_pool  # off: nothing is packed
    # the user table is gathered by the source tiles; the item table by a fused launch,
    # which reads dense rows
    assert r_on.packed == {("user", "buys", "item")}
    assert [k[0] for k in r_on._pack_pool] == ["user"]  # one buffer, reused by the layers
    for pk in r_on._pack_pool.values():
        ok, n_dense, *_ = pk.status.tolist()
        assert ok == (0 if dense else 1)
        assert n_dense == (pk.data.shape[0] if dense else 0)
    for nt in off:
        assert torch.equal(_bits(off[nt]), _bits(on[nt])), nt
