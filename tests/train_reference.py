"""A plain restatement of ONE training step over sampled blocks — TEST INFRASTRUCTURE.

torch on the CPU, `float64` by default: NodeEmbedding, every ConvLayer aggregator (mean,
mean_nn, pool_nn, mean_edge, mean_nn_edge, pool_nn_edge, lstm), the cross-relation
sum / mean / max / attention, the cosine and the MLP head, max_margin_loss — and through
torch.autograd the gradient of every parameter and of block 0's feature tables.  It is the
yardstick of tests/test_gpu_train_grads.py; tests/test_train_reference_cpu.py pins its forward
to oracle/oracle.py (which the goldens pin to the reference model) and its gradients to
central finite differences of its own fp64 loss.  It imports nothing of the product.

The same code runs in `float32` (dtype=torch.float32): that run measures what fp32
arithmetic itself costs on a tensor, the yardstick of the GPU test's measured tolerances.

Semantics restated (oracle/oracle.py cites the reference's lines):
  * edge weights ('occurrence', read through the block's global eids) apply only between
    user / item types; mean = weighted sum / max(in-degree, 1);
  * a block's dst inputs are the dst prefix of its source tables;
  * relations with no edges are skipped (they add no term, and a 'mean' divides by the
    number of ACTIVE relations);
  * z = relu(h_self W_selfᵀ + agg W_neighᵀ), then z / ||z|| with ||z|| == 0 replaced by 1;
  * attention: per dst node a softmax over its active relations of a_T · z_r.

Max reductions.  The neighbour max is a scatter 'amax' over the per-edge candidates, whose
backward splits a tied maximum's gradient evenly among the tied edges.  Two edges from ONE
source tie exactly (same row, same weight), and both halves land on the same source row: the
gradient is per source row, the tie is harmless.  The other exact ties are at 0, after a
ReLU (the pool aggregators' messages are relu(x W_preᵀ), the layer outputs across relations
are relu(..) / norm): whichever tied candidate receives the gradient, it passes relu'(0) = 0
next and carries zero gradient upstream, so the split does not matter either.  Every other
near-tie is reported as fragile (below).

Fragility report.  An fp32 forward may land on the other side of a kink of this function, and
its gradient is then legitimately another one.  `Report` counts, for tau = 1e-5 (the forward
atol of the project: the amount by which a forward value may already differ):
  relu   ReLU pre-activations with |x| < tau (fc_preagg, the layer output, the MLP hidden
         layers, the hinge argument);
  max    max reductions (over neighbours, over relations) whose best and second-best
         DISTINCT candidates differ by less than tau, unless both are 0;
  hinge  hinge arguments within tau of 0.
A case is usable only when all three are 0.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

USER_ITEM = ("user", "item")
TAU = 1e-5
_PREAGG = ("mean_nn", "pool_nn", "mean_nn_edge", "pool_nn_edge")
AGGREGATORS = ("mean", "mean_nn", "pool_nn", "mean_edge", "mean_nn_edge", "pool_nn_edge", "lstm")


class Report:
    """The fragility counts, and the discrete choices of the run (ReLU masks and arg-max
    picks, in call order) so that two runs can be compared decision by decision."""

    def __init__(self, tau: float = TAU):
        self.tau = tau
        self.relu = 0
        self.max = 0
        self.hinge = 0
        self.where: List[str] = []
        self.choices: List[tuple] = []

    def counts(self):
        return {"relu": self.relu, "max": self.max, "hinge": self.hinge}

    def empty(self) -> bool:
        return self.relu == 0 and self.max == 0 and self.hinge == 0

    def _note(self, kind: str, name: str, n: int):
        if n:
            setattr(self, kind, getattr(self, kind) + n)
            self.where.append(f"{kind} {name}: {n}")

    def same_choices(self, other: "Report") -> Optional[str]:
        """None when both runs took the same side of every kink, else the first difference."""
        if len(self.choices) != len(other.choices):
            return "different number of recorded choices"
        for (na, a), (nb, b) in zip(self.choices, other.choices):
            if na != nb or a.shape != b.shape or not np.array_equal(a, b):
                return f"{na}: {int((a != b).sum()) if a.shape == b.shape else 'shape'} differ"
        return None


def _relu(x, rep: Report, name: str):
    v = x.detach()
    rep._note("relu", name, int((v.abs() < rep.tau).sum()))
    rep.choices.append(("relu " + name, (v > 0).numpy()))
    return torch.relu(x)  # relu'(0) = 0


def _neighbour_max(msg, dst, src, w, n_dst: int, rep: Report, name: str):
    """out[v] = max over v's in-edges of msg[e] (0 for no in-edge); see the module docstring
    for the ties.  msg [E, d] per-edge candidates, dst / src int64 [E], w [E] or None."""
    E, d = msg.shape
    out = msg.new_zeros((n_dst, d)).scatter_reduce(0, dst[:, None].expand(E, d), msg, "amax",
                                                   include_self=False)
    # fragility over DISTINCT candidates: the edges of one (dst, src, weight) are one candidate
    v = msg.detach()
    key = np.stack([dst.numpy(), src.numpy(),
                    (w.detach().numpy().astype(np.float64) if w is not None
                     else np.zeros(E))], 1)
    _, keep = np.unique(key, axis=0, return_index=True)
    keep = torch.from_numpy(np.sort(keep))
    cv, cd, cs = v[keep], dst[keep], src[keep]
    C = cv.shape[0]
    ix = cd[:, None].expand(C, d)
    neg = v.new_full((n_dst, d), -np.inf)
    m1 = neg.scatter_reduce(0, ix, cv, "amax", include_self=True)
    pos = torch.arange(C)[:, None].expand(C, d)
    first = torch.full((n_dst, d), C, dtype=torch.int64).scatter_reduce(
        0, ix, torch.where(cv == m1[cd], pos, torch.full_like(pos, C)), "amin", include_self=True)
    m2 = neg.scatter_reduce(0, ix, torch.where(pos == first[cd], torch.full_like(cv, -np.inf), cv),
                            "amax", include_self=True)
    has2 = torch.isfinite(m2)
    fragile = has2 & ((m1 - m2) < rep.tau) & ~((m1 == 0) & (m2 == 0))
    rep._note("max", name, int(fragile.sum()))
    # the arg-max as a SOURCE row (-1: no in-edge; ties at 0 are not a choice: -2)
    pick = torch.where(first < C, cs[first.clamp(max=max(C - 1, 0))] if C else first,
                       torch.full_like(first, -1))
    pick = torch.where(has2 & (m1 == 0) & (m2 == 0), torch.full_like(pick, -2), pick)
    rep.choices.append(("argmax " + name, pick.numpy()))
    return out


def _lstm(indptr, indices, X, W_ih, W_hh, b_ih, b_hh):
    """Per destination nn.LSTM (one layer, h0 = c0 = 0, gates i, f, g, o) over its in-edges
    in CSR order; the final hidden state, 0 for in-degree 0."""
    d = W_hh.shape[1]
    n_dst = indptr.numel() - 1
    deg = indptr[1:] - indptr[:-1]
    h = X.new_zeros((n_dst, d))
    c = X.new_zeros((n_dst, d))
    if indices.numel() == 0:
        return h
    P = X @ W_ih.t() + (b_ih + b_hh)
    for t in range(int(deg.max())):
        act = torch.nonzero(deg > t).reshape(-1)
        gates = P[indices[indptr[act] + t]] + h[act] @ W_hh.t()
        i, f = torch.sigmoid(gates[:, :d]), torch.sigmoid(gates[:, d:2 * d])
        g, o = torch.tanh(gates[:, 2 * d:3 * d]), torch.sigmoid(gates[:, 3 * d:])
        cn = f * c[act] + i * g
        c = c.index_copy(0, act, cn)
        h = h.index_copy(0, act, o * torch.tanh(cn))
    return h


def split_state_dict(sd: Dict[str, object]):
    """state_dict -> (embed {ntype: [W, b]}, layers [{rel: {name: W}, '__attn__': {ntype: a}}],
    pred {name: W}) by ConvModel's parameter names."""
    embed, layers, pred = {}, {}, {}
    for k, v in sd.items():
        p = k.split(".")
        if p[0].endswith("_embed"):
            embed.setdefault(p[0][:-len("_embed")], [None, None])[0 if p[-1] == "weight" else 1] = v
        elif p[0] == "layers" and p[2] == "attn":
            layers.setdefault(int(p[1]), {}).setdefault("__attn__", {})[p[3]] = v
        elif p[0] == "layers":
            layers.setdefault(int(p[1]), {}).setdefault(p[3], {})[".".join(p[4:])] = v
        elif p[0] == "pred_fn":
            pred[".".join(p[1:])] = v
    return embed, [layers[i] for i in sorted(layers)], pred


def _conv_layer(ce, rel, m_in, h_self, w, agg: str, norm: bool, occ, rep: Report, name: str):
    indptr, indices, eids = rel
    n_dst = indptr.numel() - 1
    if agg == "lstm":
        h_n = _lstm(indptr, indices, m_in, w["lstm.weight_ih_l0"], w["lstm.weight_hh_l0"],
                    w["lstm.bias_ih_l0"], w["lstm.bias_hh_l0"])
    else:
        m = _relu(m_in @ w["fc_preagg.weight"].t(), rep, name + " fc_preagg") \
            if agg in _PREAGG else m_in
        deg = indptr[1:] - indptr[:-1]
        dst = torch.repeat_interleave(torch.arange(n_dst), deg)
        ew = None
        if agg.endswith("_edge") and ce[0] in USER_ITEM and ce[2] in USER_ITEM:
            ew = occ[ce][eids]
        msg = m[indices] if ew is None else m[indices] * ew[:, None]
        if agg.startswith("pool"):
            h_n = _neighbour_max(msg, dst, indices, ew, n_dst, rep, name + " neighbours")
        else:
            h_n = msg.new_zeros((n_dst, msg.shape[1])).index_add(0, dst, msg) / \
                deg.clamp(min=1).to(msg.dtype)[:, None]
    z = _relu(h_self @ w["fc_self.weight"].t() + h_n @ w["fc_neigh.weight"].t(), rep,
              name + " output")
    if norm:
        n = z.norm(2, 1, keepdim=True)
        z = z / torch.where(n == 0, torch.ones_like(n), n)
    return z


def _hetero(block, h, lw, agg: str, hetero: str, norm: bool, occ, rep: Report, name: str):
    outs: Dict[str, list] = {}
    for ce, rel in block["rels"].items():
        s, r, d = ce
        if rel[1].numel() == 0 or s not in h or d not in block["num_dst"] or d not in h:
            continue
        outs.setdefault(d, []).append(
            _conv_layer(ce, rel, h[s], h[d][:block["num_dst"][d]], lw[r], agg, norm, occ, rep,
                        f"{name} {r}"))
    res = {}
    for nt, lst in outs.items():
        st = torch.stack(lst, 0)
        if hetero == "sum":
            res[nt] = st.sum(0)
        elif hetero == "mean":
            res[nt] = st.mean(0)
        elif hetero == "max":
            res[nt] = st.amax(0)  # a tie splits evenly; ties are at 0 or reported
            v = st.detach()
            if v.shape[0] > 1:
                top = torch.sort(v, 0, descending=True)[0]
                zero = (top[0] == 0) & (top[1] == 0)
                rep._note("max", f"{name} relations into {nt}",
                          int((((top[0] - top[1]) < rep.tau) & ~zero).sum()))
                pick = torch.where(zero, torch.full_like(v[0], -2, dtype=torch.int64), v.argmax(0))
                rep.choices.append((f"argmax {name} relations into {nt}", pick.numpy()))
        elif hetero == "attention":
            wt = torch.softmax((st * lw["__attn__"][nt]).sum(-1), 0)
            res[nt] = (wt[..., None] * st).sum(0)
        else:
            raise KeyError(hetero)
    return res


def train_step(data: dict, dtype=torch.float64, tau: float = TAU, grad: bool = True) -> dict:
    """One training step on plain data.

    data: {'sd': {name: array} (ConvModel's state_dict), 'blocks': [{'rels': {cetype:
    (indptr, indices, eids)} dst-major CSR over local ids, 'num_dst': {ntype: n}}], 'feats':
    {ntype: [n_src, d_in]} block 0's source features, 'occurrence': {cetype: per GLOBAL eid},
    'pos' / 'neg': {cetype: (src, dst)}, 'K', 'delta', 'recency': {cetype: per positive} or
    None, 'mask': {cetype: per negative} or None, 'aggregator', 'hetero', 'norm', 'embed',
    'pred': 'cos' | 'nn'}.

    -> {'loss', 'pos' / 'neg': {cetype: scores}, 'h': {ntype: final rows}, 'grads': {name:
    gradient or None (not reached)}, 'feat_grads': {ntype: gradient}, 'report': Report,
    'hinge_active': the fraction of hinge terms above 0} as numpy arrays of `dtype`.
    grad=False: the forward alone ('grads' / 'feat_grads' hold None)."""
    rep = Report(tau)
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)  # noqa: E731
    I = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int64)  # noqa: E731
    params = {k: T(v).requires_grad_(True) for k, v in data["sd"].items()}
    feats = {nt: T(v).requires_grad_(True) for nt, v in data["feats"].items()}
    embed, layers, pred = split_state_dict(params)
    occ = {ce: T(v) for ce, v in (data.get("occurrence") or {}).items()}
    blocks = [{"rels": {ce: tuple(I(a) for a in r) for ce, r in b["rels"].items()},
               "num_dst": dict(b["num_dst"])} for b in data["blocks"]]
    h = dict(feats)
    if data["embed"]:
        for nt in h:
            W, b = embed[nt]
            h[nt] = h[nt] @ W.t() + b
    for li, (block, lw) in enumerate(zip(blocks, layers)):
        h = _hetero(block, h, lw, data["aggregator"], data["hetero"], data["norm"], occ, rep,
                    f"layer {li}")
    pos_s, neg_s = {}, {}
    for which, out in ((data["pos"], pos_s), (data["neg"], neg_s)):
        for ce, (s, d) in which.items():
            if ce[0] not in h or ce[2] not in h:
                continue
            s, d = I(s), I(d)
            if data["pred"] == "cos":
                hs = torch.nn.functional.normalize(h[ce[0]], p=2.0, dim=-1, eps=1e-12)
                hd = torch.nn.functional.normalize(h[ce[2]], p=2.0, dim=-1, eps=1e-12)
                out[ce] = (hs[s] * hd[d]).sum(-1, keepdim=True)
            elif ce[0] in USER_ITEM and ce[2] in USER_ITEM:
                x = torch.cat([h[ce[0]][s], h[ce[2]][d]], 1)
                tag = f"head {ce[1]} {'pos' if out is pos_s else 'neg'}"
                x = _relu(x @ pred["layer_nn.hidden_1.weight"].t() +
                          pred["layer_nn.hidden_1.bias"], rep, tag + " hidden_1")
                x = _relu(x @ pred["layer_nn.hidden_2.weight"].t() +
                          pred["layer_nn.hidden_2.bias"], rep, tag + " hidden_2")
                out[ce] = torch.sigmoid(x @ pred["layer_nn.output.weight"].t() +
                                        pred["layer_nn.output.bias"])
    K, terms, active = int(data["K"]), [], []
    for ce in pos_s:
        arg = neg_s[ce].reshape(-1, K) + data["delta"] - pos_s[ce]
        if data.get("mask") is not None:
            arg = arg - T(data["mask"][ce]).reshape(-1, K)
        rep._note("hinge", ce[1], int((arg.detach().abs() <= rep.tau).sum()))
        active.append((arg.detach() > 0).reshape(-1))
        sc = _relu(arg, rep, f"hinge {ce[1]}")
        if data.get("recency") is not None and ce in data["recency"]:
            sc = sc / T(data["recency"][ce])[:, None]
        terms.append(sc.reshape(-1))
    loss = torch.cat(terms).mean()
    names = list(params) + ["feat:" + nt for nt in feats]
    grads = torch.autograd.grad(loss, list(params.values()) + list(feats.values()),
                                allow_unused=True) if grad else [None] * len(names)
    g = {n: (None if t is None else t.numpy()) for n, t in zip(names, grads)}
    return {"loss": loss.detach().numpy(),
            "pos": {ce: v.detach().numpy() for ce, v in pos_s.items()},
            "neg": {ce: v.detach().numpy() for ce, v in neg_s.items()},
            "h": {nt: v.detach().numpy() for nt, v in h.items()},
            "grads": {n: g[n] for n in params},
            "feat_grads": {nt: g["feat:" + nt] for nt in feats},
            "report": rep,
            "hinge_active": float(torch.cat(active).double().mean())}


def loss_only(data: dict, dtype=torch.float64) -> float:
    """The step's loss alone (finite differences perturb `data` and call this)."""
    return float(train_step(data, dtype, grad=False)["loss"])


def lstm_reference(indptr, indices, X, W_ih, W_hh, b_ih, b_hh, g_out, dtype=torch.float64):
    """The LSTM reducer alone, walking each destination's edges in CSR order: -> (out, dX,
    dW_ih, dW_hh, db) for the read-out sum(out * g_out); db is the gradient of b_ih (and of
    b_hh, the same)."""
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype).requires_grad_(True)  # noqa: E731
    X, W_ih, W_hh, b_ih, b_hh = T(X), T(W_ih), T(W_hh), T(b_ih), T(b_hh)
    out = _lstm(torch.as_tensor(np.asarray(indptr), dtype=torch.int64),
                torch.as_tensor(np.asarray(indices), dtype=torch.int64), X, W_ih, W_hh, b_ih, b_hh)
    grads = torch.autograd.grad((out * torch.as_tensor(np.asarray(g_out), dtype=dtype)).sum(),
                                [X, W_ih, W_hh, b_ih])
    return tuple(t.detach().numpy() for t in (out, *grads))
