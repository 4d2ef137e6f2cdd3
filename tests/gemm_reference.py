"""What ops.gemm writes, computed on the CPU in fp64 from a case description.

A description is a tools/gemm_bits.py `Case`: the CPU inputs and keyword arguments of one or
more ops.gemm calls into one output window of a wider table.  Nothing here comes from the
kernels; the contract is written out once more, in whole-matrix torch operations:

    x   = A1 W1^T + T(A2) W2^T        T: rows / max(deg, 1) ("div"); rows with deg == 0
                                      REPLACED by zeros ("zero": a -inf row adds nothing)
    x  += bias;  x += bias_nonempty on rows with deg > 0
    x   = relu(x), then sigmoid(x)
    z   = x / (|x| or 1) with l2norm (row_norm = |x|), else x
    out = z | out + z | max(out, z) | the attention update below;  out /= out_div where > 0

Attention over the calls of a case, score e = attn_vec . z, state (m, s) per row:
    attn_first        out = z, (m, s) = (e, 1)
    attn, attn_last   m' = max(m, e); out = out exp(m - m') + z exp(e - m');
                      s' = s exp(m - m') + exp(e - m');  attn_last: out /= s'
`reference` follows the calls one by one (this online form); `direct_attention` is the same
result as one softmax over all relations.  Everything outside the [m, n] window (pad columns,
guard rows, row_norm / attn_state entries past m) keeps its initial bits.
"""
import dataclasses

import torch

RTOL, ATOL = 1e-4, 1e-5  # the project's fp32 parity tolerance (tests/test_gpu_parity.py)


@dataclasses.dataclass
class Expected:
    """One written tensor, whole: `value` where `touched`, the bits of `init` elsewhere."""
    value: torch.Tensor    # the reference's dtype
    touched: torch.Tensor  # bool
    init: torch.Tensor     # fp32, what the tensor held before the case


def activations(call, dtype=torch.float64):
    """(z, row norm before the normalisation or None) of one call."""
    x = call.a1.to(dtype) @ call.w1.to(dtype).T
    deg = call.a2_deg
    if call.a2 is not None:
        t = call.a2.to(dtype)
        if call.a2_mode == "div":
            t = t / deg.clamp(min=1).to(dtype)[:, None]
        elif call.a2_mode == "zero":
            t = torch.where((deg == 0)[:, None], torch.zeros_like(t), t)
        else:
            assert call.a2_mode is None
        x = x + t @ call.w2.to(dtype).T
    if call.bias is not None:
        x = x + call.bias.to(dtype)
    if call.bias_nonempty is not None:
        x = x + (deg > 0).to(dtype)[:, None] * call.bias_nonempty.to(dtype)
    if call.relu:
        x = x.clamp(min=0)
    if call.sigmoid:
        x = 1 / (1 + torch.exp(-x))
    if not call.l2norm:
        return x, None
    norm = (x * x).sum(1).sqrt()
    return x / torch.where(norm == 0, torch.ones_like(norm), norm)[:, None], norm


def _initial(case, dtype):
    m, n = case.m, case.n
    exp = {"out": Expected(case.out_init.to(dtype, copy=True), torch.zeros(case.out_init.shape, dtype=torch.bool),
                           case.out_init)}
    exp["out"].touched[:m, case.col:case.col + n] = True
    if case.row_norm_init is not None:
        exp["row_norm"] = Expected(case.row_norm_init.to(dtype, copy=True),
                                   torch.zeros(case.row_norm_init.shape, dtype=torch.bool),
                                   case.row_norm_init)
        exp["row_norm"].touched[:m] = True
    if case.attn_state_init is not None:
        exp["attn_state"] = Expected(case.attn_state_init.to(dtype, copy=True),
                                     torch.zeros(case.attn_state_init.shape, dtype=torch.bool),
                                     case.attn_state_init)
        exp["attn_state"].touched[:m] = True
    assert tuple(exp) == tuple(case.writes)
    return exp


def _snapshot(exp):
    return {k: Expected(e.value.clone(), e.touched, e.init) for k, e in exp.items()}


def reference(case, dtype=torch.float64):
    """[{name: Expected} after each call of the case], names in the order of case.writes."""
    m, n = case.m, case.n
    exp = _initial(case, dtype)
    win = exp["out"].value[:m, case.col:case.col + n]  # a view: updated in place
    steps = []
    for call in case.calls:
        z, norm = activations(call, dtype)
        if norm is not None and "row_norm" in exp:
            exp["row_norm"].value[:m] = norm
        if call.accum == "store":
            new = z
        elif call.accum == "add":
            new = win + z
        elif call.accum == "max":
            new = torch.maximum(win, z)
        else:
            e = z @ call.attn_vec.to(dtype)
            st = exp["attn_state"].value
            if call.accum == "attn_first":
                new, m_new, s_new = z, e, torch.ones_like(e)
            else:
                assert call.accum in ("attn", "attn_last")
                m_old, s_old = st[:m, 0].clone(), st[:m, 1].clone()
                m_new = torch.maximum(m_old, e)
                w_old, w_new = torch.exp(m_old - m_new), torch.exp(e - m_new)
                new = win * w_old[:, None] + z * w_new[:, None]
                s_new = s_old * w_old + w_new
                if call.accum == "attn_last":
                    new = new / s_new[:, None]
            st[:m, 0], st[:m, 1] = m_new, s_new
        if call.out_div > 0:
            new = new / call.out_div
        win.copy_(new)
        steps.append(_snapshot(exp))
    return steps


def direct_attention(case, dtype=torch.float64):
    """{name: Expected} after the last call of an attention case, as one softmax over all its
    relations: out = sum_j softmax_j(e_j) z_j, m = max_j e_j, s = sum_j exp(e_j - m)."""
    assert [c.accum for c in case.calls][0] == "attn_first" and case.calls[-1].accum == "attn_last"
    assert all(c.accum == "attn" for c in case.calls[1:-1])
    m, n = case.m, case.n
    exp = _initial(case, dtype)
    zs = torch.stack([activations(c, dtype)[0] for c in case.calls])        # [R, m, n]
    es = torch.stack([z @ c.attn_vec.to(dtype) for z, c in zip(zs, case.calls)])  # [R, m]
    top = es.max(0).values
    out = (torch.softmax(es, 0)[:, :, None] * zs).sum(0)
    if case.calls[-1].out_div > 0:
        out = out / case.calls[-1].out_div
    exp["out"].value[:m, case.col:case.col + n] = out
    exp["attn_state"].value[:m, 0] = top
    exp["attn_state"].value[:m, 1] = torch.exp(es - top).sum(0)
    return exp


def mismatch(got, expected, rtol=RTOL, atol=ATOL):
    """None when the fp32 tensor `got` holds `expected`: finite and within atol + rtol |ref| of
    the reference where the case writes, the initial bits elsewhere.  Otherwise what differs."""
    got = got.detach().cpu()
    if got.shape != expected.init.shape or got.dtype != torch.float32:
        return f"shape/dtype {tuple(got.shape)} {got.dtype}"
    t = expected.touched
    if not torch.equal(got[~t].view(torch.int32), expected.init[~t].view(torch.int32)):
        bad = int((got[~t].view(torch.int32) != expected.init[~t].view(torch.int32)).sum())
        return f"{bad} values outside the written window changed"
    g, ref = got[t].double(), expected.value[t].double()
    if not bool(torch.isfinite(g).all()):
        return f"{int((~torch.isfinite(g)).sum())} non-finite values"
    outside = ~((g - ref).abs() <= atol + rtol * ref.abs())  # a NaN reference is outside too
    if bool(outside.any()):
        i = int(((g - ref).abs() - (atol + rtol * ref.abs())).nan_to_num(nan=float("inf")).argmax())
        return (f"{int(outside.sum())} of {g.numel()} values outside rtol={rtol:g} atol={atol:g}, "
                f"worst got {g[i].item():.9g} want {ref[i].item():.9g}")
    return None


def error_ratio(got, expected, rtol=RTOL, atol=ATOL):
    """max |got - ref| / (atol + rtol |ref|) over the written window (<= 1: inside)."""
    t = expected.touched
    g, ref = got.detach().cpu()[t].double(), expected.value[t].double()
    return float(((g - ref).abs() / (atol + rtol * ref.abs())).max()) if g.numel() else 0.0
