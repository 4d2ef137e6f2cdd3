"""Training gradients of every layer route against the fp64 reference (tests/train_reference.py,
pinned on the CPU by tests/test_train_reference_cpu.py): per case of tests/train_grad_cases.py
the loss, every score, every parameter's gradient and both feature tables' gradients of one
step through the HIP autograd Functions, once per route the case can take — the one-node
layer, the one-node relation, the two-node form, the first-layer fold, with and without the
blocks' own transposes — each run compared directly with the reference, never with another
run.  Then the LSTM reducer at op level, at hidden 136 and 512.

Tolerance, per tensor T: |got − ref64| <= 1e-4 · |ref64| + a_T, a_T = 1e-5 · max|ref64_T| —
the project's rtol / atol with the atol scaled to the tensor.  For the tensors listed in
train_grad_cases.MEASURED_ATOL a_T is 4 × max|ref32_T − ref64_T| of the reference's own fp32
run on the CPU (never anything derived from the HIP output)."""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

import train_grad_cases as tc
import train_reference as tr

pytestmark = pytest.mark.gpu
DEV = "cuda"

Route = namedtuple("Route", "layer fused fold transposes")
_LINEAR = ("mean", "mean_edge", "mean_nn", "mean_nn_edge")


@functools.lru_cache(maxsize=None)
def _refs(name):
    """(case, data, fp64 run, fp32 run) — computed once per case and left unchanged."""
    case = next(c for c in tc.CASES if c.name == name)
    data = tc.with_parameters(case)
    return case, data, tr.train_step(data), tr.train_step(data, dtype=torch.float32)


def _widths(case):
    return [case.hidden] * (case.blocks - 1) + [case.out]


def _fusable(case, width):
    return case.aggregator in _LINEAR and (not case.norm or width <= 256)


def _routes(case):
    if case.aggregator not in _LINEAR:  # max / LSTM reducers: the switches do not apply
        return [Route(1, 1, 0, True)]
    routes = []
    if case.hetero in ("sum", "mean"):
        routes += [Route(1, 1, 0, True), Route(1, 1, 0, False)]
    routes += [Route(0, 1, 0, True), Route(0, 1, 0, False), Route(0, 0, 0, True)]
    if case.embed and case.aggregator == "mean" and case.hetero in ("sum", "mean") and \
            _fusable(case, _widths(case)[0]):
        routes.append(Route(1, 1, 1, True))
    return routes


def _expected_nodes(case, route):
    """{autograd Function name: must run (True) / must not run (False)} for one route."""
    rel = [_fusable(case, w) and bool(route.fused) for w in _widths(case)]
    node = [r and bool(route.layer) and case.hetero in ("sum", "mean") for r in rel]
    two = any(not r for r in rel)
    return {"HeteroSageFn": any(node),
            "SageRelFn": any(r and not n for r, n in zip(rel, node)),
            "SageProjectFn": two,
            "SpmmFn": two and case.aggregator != "lstm",
            "LstmAggFn": case.aggregator == "lstm",
            "FoldFn": bool(route.fold),
            "CosinePairFn": case.pred == "cos"}


def _record(monkeypatch, ag):
    calls = {}
    for name in ("HeteroSageFn", "SageRelFn", "SageProjectFn", "SpmmFn", "LstmAggFn", "FoldFn",
                 "CosinePairFn", "LinearFn"):
        fn = getattr(ag, name)
        calls[name] = []

        def apply(*a, _orig=fn.apply, _log=calls[name], **k):
            _log.append(a)
            return _orig(*a, **k)
        monkeypatch.setattr(fn, "apply", staticmethod(apply))
    return calls


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _objects(case, data, transposes):
    from gnnrec import sampling
    from gnnrec.graph import Block, PairGraph
    blocks = []
    for b in data["blocks"]:
        blk = Block({nt: torch.arange(n, device=DEV) for nt, n in b["num_src"].items()},
                    b["num_dst"],
                    {ce: (_t(ip, torch.int64), _t(ix, torch.int32), _t(e, torch.int64))
                     for ce, (ip, ix, e) in b["rels"].items()})
        blk.edata["occurrence"] = {ce: _t(data["occurrence"][ce][e], torch.int64)  # CSR order
                                   for ce, (_ip, _ix, e) in b["rels"].items()}
        if transposes:
            sampling._add_transposes(blk)
            assert blk._t
        blocks.append(blk)
    feats = {nt: _t(v, torch.float32).requires_grad_(True) for nt, v in data["feats"].items()}
    blocks[0].srcdata["features"] = feats
    last = data["blocks"][-1]["num_dst"]
    ids = {nt: torch.arange(n, device=DEV) for nt, n in last.items()}
    pos_g = PairGraph({ce: (_t(s, torch.int64), _t(d, torch.int64))
                       for ce, (s, d) in data["pos"].items()}, ids)
    neg_g = PairGraph({ce: (_t(s, torch.int64), _t(d, torch.int64))
                       for ce, (s, d) in data["neg"].items()}, ids)
    if case.grouped:
        neg_g.src_repeats_pos = case.K
    if data["recency"] is not None:
        pos_g.edata["recency"] = {ce: _t(v, torch.int64) for ce, v in data["recency"].items()}
    mask = None if data["mask"] is None else {ce: _t(v, torch.float32)
                                              for ce, v in data["mask"].items()}
    return blocks, feats, pos_g, neg_g, mask


def _step(case, data, model, route):
    """One step on the device -> {tensor name: numpy} (gradients None where not reached)."""
    from gnnrec import nn as gnn
    blocks, feats, pos_g, neg_g, mask = _objects(case, data, route.transposes)
    _, ps, ns = model(blocks, blocks[0].srcdata["features"], pos_g, neg_g, case.embed)
    loss = gnn.max_margin_loss(ps, ns, data["delta"], case.K, data["recency"] is not None,
                               pos_g.edata["recency"] if data["recency"] is not None else None,
                               mask is not None, mask)
    names = [n for n, _ in model.named_parameters()]
    grads = torch.autograd.grad(loss, [p for _, p in model.named_parameters()] +
                                list(feats.values()), allow_unused=True)
    out = {"loss": loss}
    out.update({f"pos {ce[1]}": v for ce, v in ps.items()})
    out.update({f"neg {ce[1]}": v for ce, v in ns.items()})
    out.update({"grad " + n: g for n, g in zip(names, grads)})
    out.update({"grad features " + nt: g for nt, g in zip(feats, grads[len(names):])})
    torch.cuda.synchronize()
    return {k: (None if v is None else v.detach().cpu().numpy()) for k, v in out.items()}


def _reference_tensors(ref):
    out = {"loss": ref["loss"]}
    out.update({f"pos {ce[1]}": v for ce, v in ref["pos"].items()})
    out.update({f"neg {ce[1]}": v for ce, v in ref["neg"].items()})
    out.update({"grad " + n: g for n, g in ref["grads"].items()})
    out.update({"grad features " + nt: g for nt, g in ref["feat_grads"].items()})
    return out


def _compare(got, want64, want32, measured):
    """-> (worst error as a fraction of its tolerance, its tensor, [failure lines])."""
    assert got.keys() == want64.keys()
    worst, where, bad = 0.0, None, []
    for name, ref in want64.items():
        g = got[name]
        if ref is None:  # the case does not reach this parameter
            if g is not None and np.abs(g).max() != 0:
                bad.append(f"{name}: gradient of an unreached parameter is not 0")
            continue
        if g is None:
            bad.append(f"{name}: no gradient")
            continue
        ref = np.asarray(ref, np.float64).reshape(g.shape)
        r32 = np.asarray(want32[name], np.float64).reshape(g.shape)
        scale = np.abs(ref).max()
        e32 = np.abs(r32 - ref).max()
        atol = 4 * e32 if name in measured else 1e-5 * scale
        err = np.abs(g.astype(np.float64) - ref)
        tol = 1e-4 * np.abs(ref) + atol
        if scale == 0:
            ratio = 0.0 if err.max() == 0 else np.inf
        else:
            ratio = float((err / tol).max())
        if not np.isfinite(g).all():
            ratio = np.inf
        if ratio > worst:
            worst, where = ratio, name
        if ratio > 1:
            bad.append(f"{name}: {ratio:.2f} of the tolerance (max error {err.max():.3e}, atol "
                       f"{atol:.3e}, max|ref| {scale:.3e}; the fp32 reference is off by "
                       f"{e32:.3e})")
    return worst, where, bad


@pytest.mark.parametrize("name", [c.name for c in tc.CASES])
def test_training_step_matches_fp64_reference(monkeypatch, name):
    from gnnrec import autograd as ag
    case, data, ref64, ref32 = _refs(name)
    assert ref64["report"].empty() and ref64["hinge_active"] >= 0.1
    want64, want32 = _reference_tensors(ref64), _reference_tensors(ref32)
    model = tc.build_model(case).to(DEV).train()
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    assert sd.keys() == data["sd"].keys() and all(np.array_equal(sd[k], data["sd"][k]) for k in sd)
    calls = _record(monkeypatch, ag)
    failures = []
    for route in _routes(case):
        monkeypatch.setenv("GNNREC_TRAIN_LAYER", str(route.layer))
        monkeypatch.setenv("GNNREC_TRAIN_FUSED", str(route.fused))
        monkeypatch.setenv("GNNREC_TRAIN_FOLD", str(route.fold))
        for log in calls.values():
            log.clear()
        got = _step(case, data, model, route)
        # the route was taken: a silently ignored switch would make two runs the same run
        for fn, must in _expected_nodes(case, route).items():
            assert bool(calls[fn]) == must, (route, fn, len(calls[fn]))
        if case.pred == "cos":
            assert all(a[6] == (case.K if case.grouped else None) for a in calls["CosinePairFn"])
        else:
            assert any(a[4] for a in calls["LinearFn"])  # the MLP head's sigmoid layer
        for a in calls["SageRelFn"]:
            assert (a[10] is not None) == route.transposes, route
        for a in calls["HeteroSageFn"]:
            assert all((rel[8] is not None) == route.transposes for rel in a[0][1]), route
        worst, where, bad = _compare(got, want64, want32, tc.MEASURED_ATOL.get(name, {}))
        print(f"{name} {route}: worst error {worst:.3f} of the tolerance ({where})")
        failures += [f"{route} {line}" for line in bad]
        # rows of source rows that nothing references: exactly 0
        for nt in data["feats"]:
            if np.abs(got["grad features " + nt][-1]).max() != 0:
                failures.append(f"{route} grad features {nt}: unreferenced row is not 0")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", [c.name for c in tc.CASES])
def test_training_step_is_bitwise_repeatable(monkeypatch, name):
    """The same run twice gives the same bits, on every route of the case.

    The max reducer's backward once failed this for every pool_nn / pool_nn_edge case (float
    atomics into source rows that several destinations route to: every gradient upstream of a
    max differed between two runs by up to 3.3e-7 of the tensor's max|value|); it now sums
    per-edge gradients over the source-major CSR (ops._spmm_max_backward, and
    test_spmm_max_backward_routes_to_first_argmax_and_repeats below)."""
    case, data, _ref64, _ref32 = _refs(name)
    model = tc.build_model(case).to(DEV).train()
    failures = []
    for route in _routes(case):
        monkeypatch.setenv("GNNREC_TRAIN_LAYER", str(route.layer))
        monkeypatch.setenv("GNNREC_TRAIN_FUSED", str(route.fused))
        monkeypatch.setenv("GNNREC_TRAIN_FOLD", str(route.fold))
        got, again = _step(case, data, model, route), _step(case, data, model, route)
        for k, v in got.items():
            if v is None and again[k] is None:
                continue
            if v is None or again[k] is None or not np.array_equal(v, again[k]):
                diff = np.abs(v - again[k]).max() / max(np.abs(v).max(), 1e-300)
                failures.append(f"{route} {k}: not bitwise repeatable (max difference "
                                f"{diff:.2e} of max|value|)")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------- the max reducer's backward ---
@pytest.mark.parametrize("d,weighted", [(70, False), (70, True), (384, True)])
def test_spmm_max_backward_routes_to_first_argmax_and_repeats(d, weighted):
    """ops.spmm_backward(reduce='max') against an fp64 scatter to the first arg-max edge (CSR
    order) of every (destination, column): 300 destinations over 20 sources, so nearly every
    source row collects from many destinations — where the atomic form was not repeatable —
    with repeated sources inside rows, in-degree 0 rows and one row of 200 edges; twice, for
    the same bits.  d = 70: a partial column chunk; d = 384: the four-chunk kernel."""
    from gnnrec import ops
    rng = np.random.default_rng(d + weighted)
    n_src, n_dst = 20, 300
    deg = rng.integers(0, 9, n_dst)
    deg[7] = 200
    indptr = np.zeros(n_dst + 1, np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = rng.integers(0, n_src - 1, indptr[-1]).astype(np.int32)  # last source: unused
    X = rng.standard_normal((n_src, d)).astype(np.float32)
    w = rng.integers(1, 9, indices.size).astype(np.float32) if weighted else None
    G = rng.standard_normal((n_dst, d)).astype(np.float32)
    want = {}
    for dtype in (np.float64, np.float32):
        gx = np.zeros((n_src, d), dtype)
        for v in range(n_dst):
            e = np.arange(indptr[v], indptr[v + 1])
            if e.size == 0:
                continue
            wv = w[e][:, None] if weighted else np.ones((e.size, 1), np.float32)
            first = (X[indices[e]] * wv).argmax(0)  # fp32 messages, the first maximum
            np.add.at(gx, (indices[e][first], np.arange(d)), (G[v] * wv[first, 0]).astype(dtype))
        want[dtype] = gx

    def run():
        ip, ix = _t(indptr, torch.int64), _t(indices, torch.int32)
        ew = None if w is None else _t(w, torch.float32)
        x = _t(X, torch.float32)
        y = ops.spmm(ip, ix, x, "max", edge_weight=ew)
        gx = ops.spmm_backward(ip, ix, _t(G, torch.float32), "max", edge_weight=ew, X=x, out=y,
                               n_src=n_src)
        torch.cuda.synchronize()
        return {"grad_X": gx.cpu().numpy()}
    got = run()
    worst, _, bad = _compare(got, {"grad_X": want[np.float64]}, {"grad_X": want[np.float32]}, {})
    print(f"spmm max backward d={d} weighted={weighted}: worst error {worst:.3f} of the tolerance")
    assert not bad, "\n".join(bad)
    assert np.abs(got["grad_X"][-1]).max() == 0
    assert np.array_equal(got["grad_X"], run()["grad_X"])


# ------------------------------------------------------------------ LSTM at op level ---
def _lstm_problem(d):
    rng = np.random.default_rng(d)
    n_dst, n_src = 70, 50
    deg = np.array(([0, 1] + list(range(2, 13))) * 6, np.int64)[:n_dst - 1]
    deg = rng.permutation(np.concatenate([deg, [40]]))
    dst = np.repeat(np.arange(n_dst), deg)
    order = rng.permutation(dst.size)  # edge ids in shuffled order; in-row order = eid order
    dst = dst[order]
    src = rng.integers(0, n_src, dst.size)
    by_dst = np.argsort(dst, kind="stable")
    indptr = np.zeros(n_dst + 1, np.int64)
    np.cumsum(np.bincount(dst, minlength=n_dst), out=indptr[1:])
    indices = src[by_dst].astype(np.int32)
    k = 1.0 / np.sqrt(d)
    u = lambda *shape: rng.uniform(-k, k, shape).astype(np.float32)  # noqa: E731
    X = rng.standard_normal((n_src, d)).astype(np.float32)
    g = rng.standard_normal((n_dst, d)).astype(np.float32)
    return indptr, indices, X, u(4 * d, d), u(4 * d, d), u(4 * d), u(4 * d), g


@pytest.mark.parametrize("d", [136, 512])
def test_lstm_ops_match_fp64_recurrence(d):
    """ops.lstm_aggregate, lstm_aggregate_train and lstm_aggregate_backward against an fp64
    recurrence that walks each destination's edges in CSR order (no LstmPlan): 70 destinations
    of in-degree 0, 1, 2..12 and one of 40.  d = 136: two unit blocks per row tile; d = 512:
    the largest hidden size, 32·513·4 bytes of dynamic LDS per block."""
    from gnnrec import ops
    indptr, indices, X, W_ih, W_hh, b_ih, b_hh, g = _lstm_problem(d)
    names = ("out", "dX", "dW_ih", "dW_hh", "db")
    ref64 = dict(zip(names, tr.lstm_reference(indptr, indices, X, W_ih, W_hh, b_ih, b_hh, g)))
    ref32 = dict(zip(names, tr.lstm_reference(indptr, indices, X, W_ih, W_hh, b_ih, b_hh, g,
                                              dtype=torch.float32)))
    assert set(np.diff(indptr)) >= set(range(13)) | {40}

    def run():
        ip, ix = _t(indptr, torch.int64), _t(indices, torch.int32)
        a = [_t(v, torch.float32) for v in (X, W_ih, W_hh, b_ih, b_hh)]
        out_inf = ops.lstm_aggregate(ip, ix, *a)
        out, state = ops.lstm_aggregate_train(ip, ix, *a)
        grads = ops.lstm_aggregate_backward(ip, ix, a[0], a[1], state, _t(g, torch.float32))
        torch.cuda.synchronize()
        return {"out (inference)": out_inf.cpu().numpy(),
                **{n: v.cpu().numpy() for n, v in zip(names, (out, *grads))}}
    got = run()
    want64 = {"out (inference)": ref64["out"], **ref64}
    want32 = {"out (inference)": ref32["out"], **ref32}
    worst, where, bad = _compare(got, want64, want32, tc.MEASURED_ATOL.get(f"lstm-op-{d}", {}))
    print(f"lstm ops d={d}: worst error {worst:.3f} of the tolerance ({where})")
    assert np.array_equal(got["out"][np.diff(indptr) == 0], np.zeros((int((np.diff(indptr) == 0).sum()), d)))
    again = run()
    bad += [f"{k}: not bitwise repeatable" for k in got if not np.array_equal(got[k], again[k])]
    assert not bad, "\n".join(bad)


def test_lstm_hidden_size_above_the_limit_is_an_error():
    """Hidden sizes above the kernel's limit (512) are refused, not computed."""
    from gnnrec import ops
    d = 520
    ip = torch.tensor([0, 1], dtype=torch.int64, device=DEV)
    ix = torch.zeros(1, dtype=torch.int32, device=DEV)
    z = lambda *s: torch.zeros(s, device=DEV)  # noqa: E731
    with pytest.raises(Exception, match="hidden size"):
        ops.lstm_aggregate(ip, ix, z(1, d), z(4 * d, d), z(4 * d, d), z(4 * d), z(4 * d))
        torch.cuda.synchronize()
