"""GPU tests of training dropout inside the fused nodes (csrc/dropout.hip; reference
ConvLayer.forward src/model.py:140-141 applies dropout_fn to h_neigh and h_self).

Expected values never come from the code under test: they come from the p = 0 path (pinned to
the oracle elsewhere) run on inputs the test multiplies by mask * scale itself, the mask from
the library's host routine (pinned by tests/test_dropout_cpu.py); autograd of that
multiplication gives the expected gradients.  Tolerance: the project's rtol 2e-4, atol 2e-6."""
import copy

import numpy as np
import pytest
import torch

from test_gpu_capture import _close, _loader, _loss
from test_gpu_sampling import DEV, _graph, _model

pytestmark = pytest.mark.gpu

P = (0.1, 0.5, 0.8)
SEED = 0x9E3779B97F4A7C15  # above 2**63: the seed travels as a signed schema int


def _keys(step, n, stream0=0, seed=SEED):
    from gnnrec import ops
    counter = torch.tensor([step], dtype=torch.int64, device=DEV)
    keys = ops.dropout_keys(seed, counter, n, stream0=stream0)
    assert int(counter) == step + 1  # the same launch advanced the device counter
    return keys


def _factor(step, stream, n_rows, d, p, seed=SEED):
    """mask * scale of (seed, step, stream) as a device tensor, from the host routine."""
    from gnnrec import ops
    keep = ops.dropout_mask_host(seed, step, stream, n_rows, d, p)
    return torch.from_numpy(keep.astype(np.float32) * np.float32(ops.dropout_scale(p))).to(DEV)


@pytest.mark.parametrize("p", P)
@pytest.mark.parametrize("d", (6, 20, 64, 128))
def test_device_mask_equals_the_host_mask_bitwise(d, p):
    from gnnrec import ops
    gen = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(301, d, device=DEV, generator=gen)
    keys = _keys(11, 3, stream0=5 << 16)
    for k in range(3):
        f = _factor(11, (5 << 16) + k, 301, d, p)
        want = torch.where(f > 0, x * f, torch.zeros_like(x))
        assert torch.equal(ops.dropout_rows(x, keys, k, p), want)
    # the first n rows only, accumulated into a table: this call's rows are masked, not the table
    base = torch.randn(301, d, device=DEV, generator=gen)
    out = base.clone()
    ops.dropout_rows(x, keys, 1, p, n=37, out=out, accumulate=True)
    f = _factor(11, (5 << 16) + 1, 37, d, p)
    want = base[:37] + torch.where(f > 0, x[:37] * f, torch.zeros(37, d, device=DEV))
    assert torch.equal(out[:37], want)
    assert torch.equal(out[37:], base[37:])
    # two streams, and two steps of one stream, are different masks
    assert not torch.equal(ops.dropout_rows(x, keys, 0, p), ops.dropout_rows(x, keys, 1, p))
    assert not torch.equal(ops.dropout_rows(x, _keys(12, 1, stream0=5 << 16), 0, p),
                           ops.dropout_rows(x, keys, 0, p))


def _block(dense, n_dst=37, n_src=150, seed=3):
    """Destination degrees 0, 1 and 70 (past one 64-edge chunk) among small ones; source
    n_src - 1 has no edge; source 5 is also a destination row.  dense: 20 more edges on every
    row (a mean degree above the lane-group kernel's limit: the wave kernel takes d <= 64)."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 9, n_dst)
    deg[:3] = (0, 1, 70)
    if dense:
        deg[3:] += 20
    ip = np.zeros(n_dst + 1, np.int64)
    ip[1:] = np.cumsum(deg)
    ix = rng.integers(0, n_src - 1, ip[-1]).astype(np.int32)
    ix[ip[2]] = 5
    assert (ix != n_src - 1).all() and (ix < n_dst).any()
    ew = rng.integers(1, 9, ip[-1]).astype(np.float32)
    ipt = torch.from_numpy(ip).to(DEV)
    ipt._gnnrec_nnz = int(ip[-1])
    return ipt, torch.from_numpy(ix).to(DEV), torch.from_numpy(ew).to(DEV)


def _one_relation(ip, ix, ew, d, p, reduce, norm, step, live=None, n_out=16, n_src=150):
    """SageRelFn with dropout inside against SageRelFn at p = 0 on pre-masked inputs."""
    from gnnrec import autograd as ag
    n_dst = ip.numel() - 1
    gen = torch.Generator(device=DEV).manual_seed(d * 7 + step)
    m0 = torch.randn(n_src, d, device=DEV, generator=gen)
    h0 = torch.randn(n_src, d, device=DEV, generator=gen)
    Ws0 = torch.randn(n_out, d, device=DEV, generator=gen) / d ** 0.5
    Wn0 = torch.randn(n_out, d, device=DEV, generator=gen) / d ** 0.5
    R = torch.randn(n_dst, n_out, device=DEV, generator=gen)
    keys = _keys(step, 4, stream0=1 << 16)
    fn = _factor(step, (1 << 16) + 2, n_src, d, p)
    fs = _factor(step, (1 << 16) + 3, n_dst, d, p)
    if live is not None:
        ip = ip.clone()
        ip._gnnrec_nnz = int(ip[-1])
        ip._gnnrec_live = torch.tensor([live], dtype=torch.int64, device=DEV)
    res = []
    for fused in (True, False):
        m, h, Ws, Wn = (t.clone().requires_grad_(True) for t in (m0, h0, Ws0, Wn0))
        if fused:
            z = ag.SageRelFn.apply(m, h, Ws, Wn, ip, ix, ew, reduce, norm, n_dst, None,
                                   (p, keys, 2, 3))
        else:
            z = ag.SageRelFn.apply(m * fn, h[:n_dst] * fs, Ws, Wn, ip, ix, ew, reduce, norm)
        (z * R).sum().backward()
        res.append((z.detach(), m.grad, h.grad, Ws.grad, Wn.grad))
    what = f"d={d} p={p} {reduce} ew={ew is not None} norm={norm}"
    for name, a, b in zip(("z", "g_m", "g_self", "g_Ws", "g_Wn"), *res):
        _close(a, b, f"{name} {what}")
    return res[0]


@pytest.mark.parametrize("p", P)
@pytest.mark.parametrize("d", (6, 20, 64, 128))
def test_one_relation_matches_premasked_inputs(d, p):
    ip, ix, ew = _block(dense=False)
    step = 0
    for reduce in ("mean", "sum"):
        for w in (None, ew):
            for norm in (True, False):
                step += 1
                z, g_m, g_self, _, _ = _one_relation(ip, ix, w, d, p, reduce, norm, step)
                assert torch.count_nonzero(g_m[149]) == 0      # the source no edge refers to
                assert torch.count_nonzero(g_self[37:]) == 0   # rows past the destinations


@pytest.mark.parametrize("d", (20, 64))
def test_one_relation_wave_kernel_at_narrow_rows(d):
    """A mean degree above 16: d <= 64 runs the wave-per-row kernel, not the lane-group one."""
    ip, ix, ew = _block(dense=True)
    assert int(ip[-1]) > 16 * 37
    for step, (reduce, w) in enumerate((("mean", None), ("sum", ew))):
        _one_relation(ip, ix, w, d, 0.5, reduce, True, 40 + step)


def test_static_block_padding_rows_contribute_nothing():
    """A live count below the padded row count (sampling static_shapes): the rows past it
    aggregate nothing; in the transposed gather they get zero gradient, and are left as they
    are under accumulation."""
    from gnnrec import ops
    ip, ix, ew = _block(dense=False)
    z, g_m, g_self, _, _ = _one_relation(ip, ix, None, 64, 0.5, "mean", True, 77, live=30)
    gen = torch.Generator(device=DEV).manual_seed(2)
    X = torch.randn(150, 64, device=DEV, generator=gen)
    keys = _keys(5, 2)
    live = torch.tensor([30], dtype=torch.int64, device=DEV)
    plain = torch.empty(37, 64, device=DEV)
    ops._T().spmm_csr(ip, ix, None, X, ops.REDUCE["sum"], 0, plain, live)
    out = ops.spmm_dropout(ip, ix, X, "sum", keys, 1, 0.5, "out", live=live)
    _close(out, plain * _factor(5, 1, 37, 64, 0.5), "out-side mask, live rows")
    assert torch.count_nonzero(out[30:]) == 0
    acc = torch.ones(37, 64, device=DEV)
    ops.spmm_dropout(ip, ix, X, "sum", keys, 1, 0.5, "out", live=live, out=acc, accumulate=True)
    assert torch.equal(acc[30:], torch.ones(7, 64, device=DEV))
    _close(acc[:30], 1 + out[:30], "accumulated live rows")
    src = ops.spmm_dropout(ip, ix, X, "mean", keys, 0, 0.5, "src", live=live)
    ops._T().spmm_csr(ip, ix, None, X * _factor(5, 0, 150, 64, 0.5), ops.REDUCE["mean"], 0, plain,
                      live)
    _close(src, plain, "source-side mask, live rows")


@pytest.mark.parametrize("n_rows", (300, 3000))
def test_heavy_row_backward_masks_at_the_store(n_rows):
    """The transposed gather as sage_rel_backward issues it (gather_planned: nnz > 2048 builds
    a heavy-row plan; one hub source has more out-edges than the split): chunk partials plus
    combine for the hub, the row kernel for the rest (the lane-group form at 3000 rows), the
    mask applied at the store — storing, and accumulating into a table that already holds
    another relation's gradient, which the mask must not touch."""
    from gnnrec import ops
    rng = np.random.default_rng(n_rows)
    n_dst, d, p = 500, 64, 0.5
    deg = rng.integers(0, 4, n_rows)
    deg[17] = 5000  # the hub: three chunks of 2048 edges
    ip = np.zeros(n_rows + 1, np.int64)
    ip[1:] = np.cumsum(deg)
    nnz = int(ip[-1])
    assert nnz > 2048 and deg[17] > 2048
    ix = torch.from_numpy(rng.integers(0, n_dst, nnz).astype(np.int32)).to(DEV)
    w = torch.from_numpy(rng.random(nnz).astype(np.float32)).to(DEV)
    ip = torch.from_numpy(ip).to(DEV)
    ip._gnnrec_nnz = nnz
    gen = torch.Generator(device=DEV).manual_seed(9)
    G = torch.randn(n_dst, d, device=DEV, generator=gen)
    keys = _keys(3, 2, stream0=2 << 16)
    f = _factor(3, (2 << 16) + 1, n_rows, d, p)
    want = ops.spmm(ip, ix, G, "sum", edge_weight=w) * f
    got = ops.spmm_dropout(ip, ix, G, "sum", keys, 1, p, "out", edge_weight=w)
    _close(got, want, "stored")
    assert float(got[17].abs().max()) > 0
    table = torch.randn(n_rows, d, device=DEV, generator=gen)
    acc = table.clone()
    ops.spmm_dropout(ip, ix, G, "sum", keys, 1, p, "out", edge_weight=w, out=acc, accumulate=True)
    _close(acc, table + want, "accumulated")
    # the source-side mask through the same plan (chunk kernel with the mask in the gather)
    fs = _factor(3, 2 << 16, n_dst, d, p)
    _close(ops.spmm_dropout(ip, ix, G, "mean", keys, 0, p, "src", edge_weight=w),
           ops.spmm(ip, ix, G * fs, "mean", edge_weight=w), "source side")


def test_one_relation_with_a_hub_source():
    """The same through SageRelFn's backward (sage_rel_backward -> gather_planned): the
    transposed block has more than 2048 edges, so a heavy-row plan is built on the device,
    and source 7 feeds every destination row — more out-edges than the split."""
    rng = np.random.default_rng(8)
    n_dst, n_src = 2500, 2600
    ip = torch.arange(0, 2 * n_dst + 1, 2, dtype=torch.int64, device=DEV)
    ip._gnnrec_nnz = 2 * n_dst
    ix = np.empty(2 * n_dst, np.int32)
    ix[0::2] = 7
    ix[1::2] = rng.integers(0, n_src, n_dst)
    ew = torch.from_numpy(rng.integers(1, 9, 2 * n_dst).astype(np.float32)).to(DEV)
    ix = torch.from_numpy(ix).to(DEV)
    assert int((ix == 7).sum()) > 2048
    for step, (reduce, w) in enumerate((("mean", None), ("sum", ew))):
        _, g_m, _, _, _ = _one_relation(ip, ix, w, 64, 0.5, reduce, True, 60 + step, n_src=n_src)
        assert float(g_m[7].abs().max()) > 0


def _set_dropout(model, p):
    from gnnrec import nn as gnn
    for mod in model.modules():
        if isinstance(mod, gnn.ConvLayer):
            mod.dropout_fn.p = p
    return model


def _count_calls(monkeypatch, fn):
    calls = []
    orig = fn.apply

    def apply(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    monkeypatch.setattr(fn, "apply", staticmethod(apply))
    return calls


@pytest.mark.parametrize("hetero", ("sum", "mean"))
def test_two_relations_into_one_type_through_the_layer_node(monkeypatch, hetero):
    """clicks and buys (user -> item) and their reverses in one HeteroSageFn node with
    dropout inside: outputs and every gradient against per-relation p = 0 twins on pre-masked
    tables, summed by the test; the node was taken; the two relations' masks over the table
    they share differ."""
    from gnnrec import autograd as ag
    from gnnrec import ops
    g, _ = _graph(n_u=300, n_i=120, e_b=4000, e_c=3000, min_deg=False)
    torch.manual_seed(3)
    blocks = next(iter(_loader(g, False)))[-1]
    block = blocks[1]
    model = _set_dropout(_model(g, agg="mean_edge", hetero=hetero), 0.5).train()
    layer = model.layers[1]
    p, d, step = 0.5, 16, 21
    gen = torch.Generator(device=DEV).manual_seed(4)
    tabs0 = {nt: torch.randn(block.number_of_src_nodes(nt), d, device=DEV, generator=gen)
             for nt in block.ntypes}
    R = {nt: torch.randn(block.number_of_dst_nodes(nt), 8, device=DEV, generator=gen)
         for nt in block.ntypes}
    streams = layer._drop_streams()
    assert sorted(s for pair in streams.values() for s in pair) == list(range(2 * len(streams)))
    keys = _keys(step, 2 * len(streams), stream0=1 << 16)
    calls = _count_calls(monkeypatch, ag.HeteroSageFn)

    def grads(tabs, outs):
        layer.zero_grad()
        sum((outs[nt] * R[nt]).sum() for nt in outs).backward()
        return ({nt: t.grad.clone() for nt, t in tabs.items()},
                {n: q.grad.clone() for n, q in layer.named_parameters() if q.grad is not None})

    tabs = {nt: t.clone().requires_grad_(True) for nt, t in tabs0.items()}
    layer._drop = (keys, streams)
    try:
        outs = layer(block, tabs)
    finally:
        layer._drop = None
    assert len(calls) == 1, "the layer did not run as one HeteroSageFn node"
    gt, gw = grads(tabs, outs)

    tw = {nt: t.clone().requires_grad_(True) for nt, t in tabs0.items()}
    parts = {}
    for ce in block.canonical_etypes:
        if block.num_edges(ce) == 0:
            continue
        mod, rg = layer.mods[ce[1]], block.rel_graph(ce)
        _pre, weighted, reduce = mod._plan(rg)
        n_dst = block.number_of_dst_nodes(ce[2])
        sn, ss = streams[ce[1]]
        fn = _factor(step, (1 << 16) + sn, tw[ce[0]].shape[0], d, p)
        fs = _factor(step, (1 << 16) + ss, n_dst, d, p)
        z = ag.SageRelFn.apply(tw[ce[0]] * fn, tw[ce[2]][:n_dst] * fs, mod.fc_self.weight,
                               mod.fc_neigh.weight, rg.indptr, rg.indices,
                               mod._edge_weight(rg) if weighted else None, reduce, bool(mod.norm))
        parts.setdefault(ce[2], []).append(z)
    want = {nt: sum(zs) / (len(zs) if hetero == "mean" else 1) for nt, zs in parts.items()}
    assert all(len(zs) == 2 for zs in parts.values())
    et, ew_ = grads(tw, want)
    assert len(calls) == 1
    for nt in want:
        _close(outs[nt], want[nt], f"out {nt}")
        _close(gt[nt], et[nt], f"table gradient {nt}")
    assert gw.keys() == ew_.keys() and gw
    for n in gw:
        _close(gw[n], ew_[n], n)
    # clicks and buys gather the same user table through different masks
    x = tabs0["user"]
    a = ops.dropout_rows(x, keys, streams["clicks"][0], p)
    b = ops.dropout_rows(x, keys, streams["buys"][0], p)
    assert not torch.equal(a == 0, b == 0)


def _batch(g, static=False, seed=3):
    torch.manual_seed(seed)
    return next(iter(_loader(g, static)))


def test_model_runs_its_layers_as_fused_nodes_under_dropout(monkeypatch):
    """ConvModel in training mode with p = 0.5: every layer is one HeteroSageFn node (the
    parent commit bails out to nn.Dropout and per-relation nodes), nn.Dropout is never called,
    and GNNREC_TRAIN_DROPOUT=torch restores that path."""
    from gnnrec import autograd as ag
    g, _ = _graph(n_u=300, n_i=120, e_b=4000, e_c=3000, min_deg=False)
    batch = _batch(g)
    model = _set_dropout(_model(g, agg="mean"), 0.5).train()
    model.train_fold = "0"
    calls = _count_calls(monkeypatch, ag.HeteroSageFn)
    torch_dropout = []
    monkeypatch.setattr(torch.nn.Dropout, "forward",
                        lambda self, x: torch_dropout.append(1) or x)
    loss = _loss(4)(model, batch)
    loss.backward()
    assert torch.isfinite(loss)
    assert len(calls) == len(model.layers) and not torch_dropout
    assert int(model._dropout_counter) == len(model.layers)  # one key derivation per layer call
    monkeypatch.setenv("GNNREC_TRAIN_DROPOUT", "torch")
    _loss(4)(model, batch)
    assert len(calls) == len(model.layers) and torch_dropout


def test_eval_mode_and_p_zero_are_todays_path():
    g, _ = _graph(n_u=300, n_i=120, e_b=4000, e_c=3000, min_deg=False)
    batch = _batch(g)
    base = _model(g, agg="mean")
    dropped = _set_dropout(copy.deepcopy(base), 0.5)
    la = _loss(4)(base.eval(), batch)
    lb = _loss(4)(dropped.eval(), batch)
    assert torch.equal(la, lb)
    with torch.no_grad():
        assert torch.equal(_loss(4)(base, batch), _loss(4)(dropped, batch))
    assert dropped._dropout_counter is None  # no key was derived
    lt = _loss(4)(base.train(), batch)
    assert base._dropout_counter is None and torch.isfinite(lt)


def _train(base, batches, seed, steps=3):
    m = copy.deepcopy(base).train()
    m.dropout_seed = seed
    opt = torch.optim.Adam(m.parameters(), lr=0.01)
    losses = []
    for batch in batches[:steps]:
        loss = _loss(4)(m, batch)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def test_training_is_reproducible_from_the_dropout_seed():
    g, _ = _graph(n_u=300, n_i=120, e_b=4000, e_c=3000, min_deg=False)
    torch.manual_seed(3)
    batches = list(_loader(g, False))[:3]
    base = _set_dropout(_model(g, agg="mean"), 0.5)
    a, b, c = _train(base, batches, 5), _train(base, batches, 5), _train(base, batches, 6)
    assert a == b
    assert a[0] != c[0]


def test_first_layer_fold_is_off_under_dropout():
    """dropout(W_e x + b_e) sits between the NodeEmbedding and the first layer: train_fold
    '1' (what a captured step sets) must not fold — the loss is the unfolded form's."""
    g, _ = _graph(n_u=300, n_i=120, e_b=4000, e_c=3000, min_deg=False)
    batch = _batch(g)
    base = _set_dropout(_model(g, agg="mean", emb=True), 0.5).train()
    losses = {}
    for fold in ("1", "0"):
        m = copy.deepcopy(base)
        m.train_fold = fold
        m.dropout_seed = 9
        losses[fold] = _loss(4)(m, batch).detach()
    _close(losses["1"], losses["0"], "loss with train_fold='1' against the unfolded form")
    # and dropout does change the loss: the comparison above is not vacuous
    m = copy.deepcopy(base)
    m.dropout_seed = 10
    assert not torch.equal(_loss(4)(m, batch).detach(), losses["0"])


def test_captured_step_with_dropout(monkeypatch):
    """CapturedTrainStep over static batches with p = 0.5 against step.eager on the same
    batches from the same seed: warm-up, capture and replays give the eager losses (the keys
    come from a device counter, so every replay draws the masks of its own step), and
    replaying one batch twice gives two different losses."""
    from gnnrec.capture import CapturedTrainStep
    g, _ = _graph(n_u=300, n_i=120, e_b=4000, e_c=3000, min_deg=False)
    torch.manual_seed(7)
    batches = [b for b in list(_loader(g, True))[:6] if b[1].static]
    assert len(batches) == 6
    base = _set_dropout(_model(g, agg="mean"), 0.5).train()
    runs = []
    for captured in (False, True):  # eager first: the captured step reuses a batch's buffers
        m = copy.deepcopy(base)
        m.train_fold = "1"
        m.dropout_seed = 13
        opt = torch.optim.Adam(m.parameters(), lr=0.01, fused=True)
        step = CapturedTrainStep(m, opt, _loss(4), warmup=1)
        losses = [float((step(b) if captured else step.eager(b)).detach()) for b in batches]
        runs.append((losses, step))
    (la, _), (lb, st) = runs
    assert st.captures == 1 and st.replays == len(batches) - 1 and st.eager_steps == 1
    np.testing.assert_allclose(lb, la, rtol=1e-4)
    # the same batch replayed twice, parameters frozen (lr = 0): only the masks change
    m = copy.deepcopy(base)
    m.dropout_seed = 13
    opt = torch.optim.Adam(m.parameters(), lr=0.0, fused=True)
    step = CapturedTrainStep(m, opt, _loss(4), warmup=1)
    torch.manual_seed(7)
    fresh = list(_loader(g, True))[:2]
    step(fresh[0])
    seen = [float(step(fresh[1]).detach())]  # capture, then the first replay
    for _ in range(2):  # the captured batch again: its buffers are the graph's inputs
        step.graph.replay()
        seen.append(float(step.loss))
    assert step.captures == 1 and step.replays == 1
    assert seen[1] != seen[2] and seen[0] != seen[1]
