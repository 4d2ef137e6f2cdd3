"""The first-layer aggregate cache of ShardedFullGraphPass without a GPU: the
pass's orchestration runs on the oracle backend (tests/oracle_ops.py), whose spmm calls are
counted.  Without an embedding layer the first layer gathers the caller's feature tensors, so
its aggregates are kept: a warm pass makes exactly the later layers' spmm calls.  The key is
the source tensor's identity, version, address and layout — never a weight."""
import numpy as np
import pytest
import torch

N_U, N_I, E, D = 300, 40, 4000, 16
BUYS, BOUGHT = ("user", "buys", "item"), ("item", "bought-by", "user")


class CountingOps:
    """oracle_ops with its spmm calls counted."""

    def __init__(self):
        import oracle_ops
        self._o, self.spmm_calls = oracle_ops, 0
        self.gemm, self.add_, self.lstm_aggregate = oracle_ops.gemm, oracle_ops.add_, \
            oracle_ops.lstm_aggregate

    def spmm(self, *a, **kw):
        self.spmm_calls += 1
        return self._o.spmm(*a, **kw)


def _graph():
    from gnnrec.graph import HeteroGraph
    rng = np.random.default_rng(3)
    u, i = rng.integers(0, N_U, E), rng.integers(0, N_I, E)
    return HeteroGraph({BUYS: (torch.from_numpy(u), torch.from_numpy(i)),
                        BOUGHT: (torch.from_numpy(i), torch.from_numpy(u))},
                       {"user": N_U, "item": N_I})


def _model(agg="mean"):
    from gnnrec import nn as gnn
    from gnnrec.synth import GraphMeta
    torch.manual_seed(0)
    return gnn.ConvModel(GraphMeta([BUYS, BOUGHT], ["item", "user"]), 3,
                         {"user": D, "item": D, "hidden": D, "out": D}, True, 0.0, agg, "cos",
                         "sum", True).eval()


def _feats(sh):
    rng = np.random.default_rng(1)
    return sh.local_features({"user": torch.from_numpy(rng.standard_normal((N_U, D)).astype(np.float32)),
                              "item": torch.from_numpy(rng.standard_normal((N_I, D)).astype(np.float32))})


def _runner(model, segments, **kw):
    from gnnrec.inference import GraphShard, ShardedFullGraphPass
    sh = GraphShard.from_graph(_graph(), 0, 1, "user", device="cpu", segments=segments)
    O = CountingOps()
    return sh, O, ShardedFullGraphPass(model, sh, ops_backend=O, deterministic=segments is not None,
                                       **kw)


def _run(runner, O, feats):
    O.spmm_calls = 0
    out = runner.run(feats, embedding_layer=False)
    return {nt: t.clone().numpy() for nt, t in out.items()}, O.spmm_calls


def _eq(a, b):
    return all(np.array_equal(a[nt].view(np.int32), b[nt].view(np.int32)) for nt in a)


# spmm calls of one layer: one per relation, or one per source tile for the tiled relation
@pytest.mark.parametrize("segments,per_layer", [(None, 2), (4, 5)])
def test_warm_pass_makes_only_the_later_layers_spmm_calls(segments, per_layer):
    model = _model()
    sh, O, kept = _runner(model, segments)
    _, P, plain = _runner(model, segments, cache_aggregates=False)
    feats = _feats(sh)
    ref, n_ref = _run(plain, P, feats)
    assert n_ref == 2 * per_layer
    cold, n_cold = _run(kept, O, feats)
    assert n_cold == 2 * per_layer and kept.agg_hits == set() and kept.agg_saved == {BUYS, BOUGHT}
    warm, n_warm = _run(kept, O, feats)
    assert n_warm == per_layer and kept.agg_hits == {BUYS, BOUGHT} and kept.agg_saved == set()
    assert _eq(cold, ref) and _eq(warm, ref)
    assert _run(plain, P, feats)[1] == 2 * per_layer  # cache_aggregates=False: never


def test_key_follows_the_feature_tensors_and_never_a_weight():
    model = _model()
    sh, O, kept = _runner(model, None)
    _, P, plain = _runner(model, None, cache_aggregates=False)
    feats = _feats(sh)
    _run(kept, O, feats)
    # a weight update: still a hit, and the new weights are used
    before = _run(kept, O, feats)[0]
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.01)
    got, n = _run(kept, O, feats)
    assert n == 2 and kept.agg_hits == {BUYS, BOUGHT}
    assert _eq(got, _run(plain, P, feats)[0]) and not _eq(got, before)
    # a version bump of one table: the relation gathering it misses, the other hits
    feats["item"].add_(1)
    got, n = _run(kept, O, feats)
    assert n == 3 and kept.agg_hits == {BUYS} and kept.agg_saved == {BOUGHT}
    assert _eq(got, _run(plain, P, feats)[0])
    assert _run(kept, O, feats)[1] == 2
    # a new tensor of equal shape and values
    feats["user"] = feats["user"].clone()
    got, n = _run(kept, O, feats)
    assert n == 3 and kept.agg_hits == {BOUGHT} and kept.agg_saved == {BUYS}
    assert _eq(got, _run(plain, P, feats)[0])
    # dropped on request
    kept.invalidate_aggregates()
    assert _run(kept, O, feats)[1] == 4 and kept.agg_saved == {BUYS, BOUGHT}
    assert _run(kept, O, feats)[1] == 2


def test_edge_weights_are_part_of_the_key():
    """mean_edge: the relation's weight tensor enters the aggregate, so it enters the key."""
    model = _model("mean_edge")
    sh, O, kept = _runner(model, None)
    feats = _feats(sh)
    if all(rs.weights is None for rs in sh.rels.values()):
        for rs in sh.rels.values():
            rs.weights = torch.ones(rs.local_edges)
    _run(kept, O, feats)
    assert _run(kept, O, feats)[1] == 2
    w = sh.rels[BUYS].weights
    key = kept._agg_cache[BUYS]['key']
    assert key[1] is not None and key[1][0] == id(w) and key[2] == 'mean'
    w.mul_(2)
    assert _run(kept, O, feats)[1] == 3 and kept.agg_saved == {BUYS}


def test_switches(monkeypatch):
    model = _model()
    sh, O, kept = _runner(model, None)
    feats = _feats(sh)
    monkeypatch.setenv("GNNREC_AGG_CACHE", "0")
    assert _run(kept, O, feats)[1] == 4 and _run(kept, O, feats)[1] == 4
    monkeypatch.delenv("GNNREC_AGG_CACHE")
    assert _run(kept, O, feats)[1] == 4 and _run(kept, O, feats)[1] == 2
    # with the embedding layer on, this backend cannot fold it: the first layer gathers
    # embedded tables, which depend on weights — nothing is kept
    O.spmm_calls = 0
    kept.run(feats, embedding_layer=True)
    kept.run(feats, embedding_layer=True)
    assert O.spmm_calls == 8 and kept.agg_hits == set() and kept.agg_saved == set()
