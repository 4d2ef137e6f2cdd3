"""The sharded pass's side stream reads tensors the main stream allocated — a layer's input
tables and the fc_preagg message of a fused launch — and the caller drops them when the layer
returns.  With the side stream running late (side_delay_us holds it before its work) the main
stream's next allocation, the next layer's fc_preagg output, must not land in memory the side
stream has yet to read: the pass with the delay equals the pass without a side stream."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_U, N_I, E, D = 289, 119, 9826, 128  # 34 edges per user row, 83 per item row: both fuse


@pytest.mark.parametrize("agg", ["mean_nn", "mean"])
def test_late_side_stream_reads_its_inputs_intact(agg):
    from gnnrec import nn as gnn
    from gnnrec.graph import HeteroGraph
    from gnnrec.inference import GraphShard, ShardedFullGraphPass
    rng = np.random.default_rng(52)
    u, i = rng.integers(0, N_U, E), rng.integers(0, N_I, E)
    g = HeteroGraph({("user", "buys", "item"): (torch.from_numpy(u), torch.from_numpy(i)),
                     ("item", "bought-by", "user"): (torch.from_numpy(i), torch.from_numpy(u))},
                    {"user": N_U, "item": N_I}, device="cuda")
    feats = {nt: torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).cuda()
             for nt, n in (("user", N_U), ("item", N_I))}
    torch.manual_seed(0)
    model = gnn.ConvModel(g, 3, {"user": D, "item": D, "hidden": D, "out": D}, True, 0.0, agg,
                          "cos", "sum", True).cuda().eval()
    sh = GraphShard.from_graph(g, 0, 1, "user", device="cuda")
    x = sh.local_features(feats)
    ref = ShardedFullGraphPass(model, sh, overlap=False, cache_aggregates=False).run(x)
    ref = {nt: t.clone() for nt, t in ref.items()}
    late = ShardedFullGraphPass(model, sh, cache_aggregates=False)
    assert late.side is not None
    late.side_delay_us = 3000
    for _ in range(3):
        out = late.run(x)
        assert {("user", "buys", "item"), ("item", "bought-by", "user")} <= late.fused
        for nt in ref:
            torch.testing.assert_close(out[nt], ref[nt], rtol=1e-5, atol=1e-6, msg=nt)
