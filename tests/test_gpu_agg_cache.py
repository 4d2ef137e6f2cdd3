"""ShardedFullGraphPass keeps the first layer's aggregates of the raw feature tables and
reuses them while the caller's tensors stay the same.

A small bipartite shard (3000 users x 400 items x 150k edges: 50 edges per user row, so the
user side runs the VALU fused launch; d = 128, 4 source tiles).  A runner with the cache is
compared, every layer's tables bitwise, with one without it — on the cold pass, the warm pass,
after weight updates (still a hit), after a feature update (a miss of that relation alone) and
after invalidate_aggregates().  The route is asserted through the runner's records (fused,
agg_hits, agg_saved) and the timer tags, so no case can pass by taking another path."""
import contextlib
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu

N_U, N_I, E, D, SEG = 3000, 400, 150_000, 128, 4
BUYS, BOUGHT = ("user", "buys", "item"), ("item", "bought-by", "user")


class Tags:
    """runner.timers: records the tag of every timed launch."""

    def __init__(self):
        self.tags = []

    @contextlib.contextmanager
    def __call__(self, tag):
        self.tags.append(tag)
        yield


def _setup(agg="mean", rank=0, world=1):
    from gnnrec import nn as gnn
    from gnnrec.synth import GraphMeta, bipartite_shard, node_features
    dev = torch.device("cuda", 0)
    sh = bipartite_shard(N_U, N_I, E, rank, world, dev, segments=SEG)
    feats = {"user": node_features(N_U, D, 0, dev, slice(sh.p_lo, sh.p_hi)),
             "item": torch.zeros((sh.padded_rows("item"), D), device=dev)}
    feats["item"][:N_I] = node_features(N_I, D, 1, dev)
    torch.manual_seed(0)
    model = gnn.ConvModel(GraphMeta(sh.canonical_etypes, ["item", "user"]), 3,
                          {"user": D, "item": D, "hidden": D, "out": D}, True, 0.0, agg, "cos",
                          "sum", True).to(dev).eval()
    return sh, feats, model


def _pass(runner, feats, **kw):
    """One pass -> every layer's tables (cloned: the scratch behind them is reused)."""
    runner.capture, runner.timers = [], Tags()
    runner.run(feats, **kw)
    torch.cuda.synchronize()
    return [{nt: t.clone() for nt, t in layer.items()} for layer in runner.capture]


def _same(a, b):
    assert len(a) == len(b) and len(a) >= 2
    for l, (la, lb) in enumerate(zip(a, b)):
        assert la.keys() == lb.keys()
        for nt in la:
            assert torch.equal(la[nt].view(torch.int32), lb[nt].view(torch.int32)), (l, nt)


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "fast"])
def test_cached_passes_equal_uncached_bitwise(det):
    from gnnrec.inference import ShardedFullGraphPass
    sh, feats, model = _setup()
    plain = ShardedFullGraphPass(model, sh, deterministic=det, cache_aggregates=False)
    kept = ShardedFullGraphPass(model, sh, deterministic=det)
    both, n_tiles = {BUYS, BOUGHT}, SEG

    def check(hits, saved, ref=None):
        ref = _pass(plain, feats) if ref is None else ref
        assert plain.agg_hits == set() and plain.agg_saved == set()
        got = _pass(kept, feats)
        assert kept.agg_hits == hits and kept.agg_saved == saved, (kept.agg_hits, kept.agg_saved)
        # the route: the user side is the VALU fused launch in both layers; a relation that
        # hit ran no aggregation launch in the first layer
        tags = kept.timers.tags
        assert BOUGHT in kept.fused and "spmm_project_mfma" not in tags and "spmm" not in tags
        assert tags.count("project_cached") == (BOUGHT in hits)
        assert tags.count("spmm_project") == 2 - (BOUGHT in hits)
        assert tags.count("spmm_tile") == n_tiles * (2 - (BUYS in hits))
        assert plain.timers.tags.count("spmm_project") == 2
        assert plain.timers.tags.count("spmm_tile") == 2 * n_tiles
        _same(got, ref)
        return ref

    ref0 = check(set(), both)            # 1. cold
    check(both, set(), ref0)             # 2. warm
    with torch.no_grad():                # 3. new weights: the aggregates do not depend on them
        model.layers[0].mods["bought-by"].fc_neigh.weight.add_(0.01)
        model.layers[0].mods["buys"].fc_self.weight.add_(0.01)
        model.user_embed.proj_feats.weight.add_(0.01)
        model.item_embed.proj_feats.bias.add_(0.01)
    ref1 = check(both, set())
    assert not torch.equal(ref1[0]["user"], ref0[0]["user"])
    assert not torch.equal(ref1[0]["item"], ref0[0]["item"])
    feats["item"].add_(1)                # 4. new item features: the item-sourced relation
    ref2 = check({BUYS}, {BOUGHT})
    assert not torch.equal(ref2[0]["user"], ref1[0]["user"])
    check(both, set(), ref2)
    kept.invalidate_aggregates()         # 5.
    check(set(), both, ref2)
    check(both, set(), ref2)
    # a new tensor of the same shape and values is another key
    feats["user"] = feats["user"].clone()
    check({BOUGHT}, {BUYS}, ref2)


def test_switch_off_by_environment(monkeypatch):
    from gnnrec.inference import ShardedFullGraphPass
    sh, feats, model = _setup()
    runner = ShardedFullGraphPass(model, sh, deterministic=True)
    monkeypatch.setenv("GNNREC_AGG_CACHE", "0")
    a, b = _pass(runner, feats), _pass(runner, feats)
    assert runner.agg_hits == set() and runner.agg_saved == set()
    assert "project_cached" not in runner.timers.tags
    monkeypatch.delenv("GNNREC_AGG_CACHE")
    _pass(runner, feats)
    c = _pass(runner, feats)
    assert runner.agg_hits == {BUYS, BOUGHT}
    _same(a, b)
    _same(a, c)


def test_without_embedding_layer():
    """No NodeEmbedding: the first layer gathers the caller's tables as they are."""
    from gnnrec.inference import ShardedFullGraphPass
    sh, feats, model = _setup()
    plain = ShardedFullGraphPass(model, sh, deterministic=True, cache_aggregates=False)
    kept = ShardedFullGraphPass(model, sh, deterministic=True)
    ref = _pass(plain, feats, embedding_layer=False)
    _same(_pass(kept, feats, embedding_layer=False), ref)
    assert kept.agg_saved == {BUYS, BOUGHT}
    _same(_pass(kept, feats, embedding_layer=False), ref)
    assert kept.agg_hits == {BUYS, BOUGHT} and "project_cached" in kept.timers.tags
    # with the embedding applied the same runner must not reuse raw-feature aggregates for a
    # model that cannot fold it: here it folds, and the keys are the same tensors' — a hit
    _same(_pass(kept, feats), _pass(plain, feats))


@pytest.mark.parametrize("embedding_layer", [True, False])
def test_fc_preagg_layer_is_not_cached(embedding_layer):
    """mean_nn: the message is fc_preagg's output, which depends on a weight."""
    from gnnrec.inference import ShardedFullGraphPass
    sh, feats, model = _setup("mean_nn")
    plain = ShardedFullGraphPass(model, sh, deterministic=True, cache_aggregates=False)
    kept = ShardedFullGraphPass(model, sh, deterministic=True)
    ref = _pass(plain, feats, embedding_layer=embedding_layer)
    for _ in range(2):
        _same(_pass(kept, feats, embedding_layer=embedding_layer), ref)
        assert kept.agg_hits == set() and kept.agg_saved == set()
        assert "project_cached" not in kept.timers.tags


# ---- two ranks on one GPU ---------------------------------------------------------------
def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from gnnrec.dist import AsyncEmulatedExchange, RecordingExchange
        from gnnrec.inference import ShardedFullGraphPass
        sh, feats, model = _setup(rank=rank, world=world)
        ex = AsyncEmulatedExchange(delay_us=500)
        rec = RecordingExchange(ex)
        runner = ShardedFullGraphPass(model, sh, rec, deterministic=True, cache_exchanged=True)
        res = []
        for _ in range(3):  # cold, warm, warm
            rec.calls = []
            out = runner.run(feats)
            torch.cuda.synchronize()
            res.append((out["user"].cpu().numpy(), out["item"][:N_I].cpu().numpy(),
                        [c[:2] for c in rec.calls], sorted(runner.agg_hits)))
        q.put((rank, sh.p_lo, sh.p_hi, res))
        ex.close()
    finally:
        dist.destroy_process_group()


def test_two_ranks_warm_passes_skip_the_first_layer_exchange():
    import numpy as np
    import torch.multiprocessing as mp
    from gnnrec.inference import ShardedFullGraphPass
    sh, feats, model = _setup()
    one = ShardedFullGraphPass(model, sh, deterministic=True, cache_aggregates=False).run(feats)
    users, items = one["user"].cpu().numpy(), one["item"][:N_I].cpu().numpy()
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    try:
        for p in procs:
            p.start()
        res = [q.get(timeout=240) for _ in range(2)]
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    for rank, lo, hi, passes in res:
        for k, (u, i, calls, hits) in enumerate(passes):
            assert np.array_equal(u.view(np.int32), users[lo:hi].view(np.int32)), (rank, k)
            assert np.array_equal(i.view(np.int32), items.view(np.int32)), (rank, k)
        cold, warm = passes[0][2], passes[1][2]
        # cold: per layer the partials' all-to-all, then the all-gather of the owners' rows
        assert [c[0] for c in cold] == ["all_to_all", "all_gather"] * 2, cold
        assert passes[0][3] == [] and passes[1][3] == sorted([BUYS, BOUGHT])
        # warm: the first layer's partial exchange is gone, everything else is as before
        assert warm == cold[1:], (warm, cold)
        assert passes[2][2] == warm and passes[2][3] == passes[1][3]
