"""gnnrec_spmm_project_agg_f32: the fused aggregate+project launch (VALU kernel, d = 128) that
also saves the rows' aggregates, or takes saved ones instead of gathering.

Everything is compared bitwise (torch.equal on the int32 views) against the plain launch
(gnnrec_spmm_project_f32) of the same arguments:
  1. a save launch writes the plain launch's output,
  2. and its AGG is ops.spmm of the same CSR and reducer (the fused kernels' aggregate has the
     plain aggregation kernel's bits);
  3. a load launch from that AGG writes the plain launch's output,
  4. also with the source table, the indices and the edge weights poisoned (NaN rows,
     out-of-range ids): a load launch reads none of them;
  5. the library refuses a missing or misaligned agg and a row stride below the row width.
Shapes: row counts around the two-rows-per-wave step (odd counts pad a row) and one with many
queue tickets; degrees around the 64-edge index window, and one row just under the heavy-row
split.  Both row schedules, every reducer, weighted and not, every accumulate mode, bias /
bias_nonempty and ReLU / L2 norm on and off."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D, N_SRC = 128, 3000
DEGREES = [0, 1, 63, 64, 65, 130, 2047]  # 2047: just under ops.DEFAULT_SPLIT (2048)
ACCUMS = ["store", "add", "max", "attn_first", "attn", "attn_last"]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _csr(n_dst, rng):
    """The first rows take DEGREES in turn, the rest degrees around 8 (0..16); the CSRs
    shorter than one step of two rows pair a valid row with the padding row, an empty row
    with a full one, and a row past the 64-edge window with short ones."""
    short = {1: [65], 2: [0, 130], 3: [1, 0, 64]}
    deg = np.array(short.get(n_dst) or
                   [DEGREES[r] if r < len(DEGREES) else int(rng.integers(0, 17))
                    for r in range(n_dst)], dtype=np.int64)
    ip = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ix = rng.integers(0, N_SRC, int(ip[-1])).astype(np.int32)
    return torch.from_numpy(ip).cuda(), torch.from_numpy(ix).cuda()


@pytest.fixture(scope="module")
def tables():
    rng = np.random.default_rng(7)
    g = torch.Generator(device="cuda").manual_seed(3)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    t = {"X": r(N_SRC, D), "Ws": r(D, D) / 11, "Wn": r(D, D) / 11, "bias": r(D), "bias_ne": r(D),
         "attn_vec": r(D) / 11, "csr": {}, "ref": {}}
    for n in (0, 1, 2, 3, 17, 4099):
        ip, ix = _csr(n, rng)
        ew = torch.rand(ix.numel(), device="cuda", generator=g) + 0.5
        t["csr"][n] = (ip, ix, ew, r(n, D), r(n, D),
                       torch.stack([r(n), torch.rand(n, device="cuda", generator=g) + 1], 1))
    return t


def _ref(t, n, reduce, weighted):
    """ops.spmm of the shape's CSR, computed once per (shape, reducer, weighted)."""
    from gnnrec import ops
    key = (n, reduce, weighted)
    if key not in t["ref"]:
        ip, ix, ew = t["csr"][n][:3]
        t["ref"][key] = ops.spmm(ip, ix, t["X"], reduce, edge_weight=ew if weighted else None)
    return t["ref"][key]


@pytest.mark.parametrize("queued", [False, True], ids=["static", "queue"])
@pytest.mark.parametrize("n_dst", [1, 2, 3, 17, 4099])
def test_save_and_load_launches_match_the_plain_launch(tables, n_dst, queued):
    import contextlib

    from gnnrec import ops
    t = tables
    ip, ix, ew, H, out0, state0 = t["csr"][n_dst]
    X_nan = torch.full_like(t["X"], float("nan"))
    ix_bad = torch.full_like(ix, 1 << 30)
    ew_nan = torch.full_like(ew, float("nan"))
    bad = []
    with ops.concurrency(0, True) if queued else contextlib.nullcontext():
        for reduce, weighted in itertools.product(("sum", "mean", "max"), (False, True)):
            agg_ref = _ref(t, n_dst, reduce, weighted)
            for accum, (b, bne), (relu, l2) in itertools.product(
                    ACCUMS, itertools.product((False, True), repeat=2),
                    itertools.product((False, True), repeat=2)):
                attn = accum.startswith("attn")

                def launch(X=t["X"], indices=ix, w=ew, **kw):
                    st = state0.clone() if attn else None
                    out = ops.spmm_project(
                        ip, indices, X, H, t["Ws"], t["Wn"], reduce, w if weighted else None,
                        relu=relu, l2norm=l2, accum=accum, out=out0.clone(),
                        bias=t["bias"] if b else None, bias_nonempty=t["bias_ne"] if bne else None,
                        attn_vec=t["attn_vec"] if attn else None, attn_state=st, variant="valu",
                        **kw)
                    return out, st

                def same(a, b_):
                    return torch.equal(_bits(a[0]), _bits(b_[0])) and \
                        (not attn or torch.equal(_bits(a[1]), _bits(b_[1])))

                plain = launch()
                agg = torch.full((n_dst, D), float("nan"), device="cuda")
                what = (reduce, weighted, accum, b, bne, relu, l2)
                if not same(launch(agg=agg, agg_mode="save"), plain):
                    bad.append(("save output",) + what)
                if not torch.equal(_bits(agg), _bits(agg_ref)):
                    bad.append(("saved aggregate",) + what)
                if not same(launch(agg=agg, agg_mode="load"), plain):
                    bad.append(("load output",) + what)
                if not same(launch(X=X_nan, indices=ix_bad, w=ew_nan, agg=agg, agg_mode="load"),
                            plain):
                    bad.append(("load output, poisoned sources",) + what)
    assert not bad, bad[:10]


def test_load_launch_takes_no_source_arguments(tables):
    """indices, X and the edge weights may be absent from a load launch."""
    from gnnrec import ops
    t = tables
    ip, ix, ew, H, _, _ = t["csr"][17]
    plain = ops.spmm_project(ip, ix, t["X"], H, t["Ws"], t["Wn"], "mean", variant="valu")
    agg = torch.empty((17, D), device="cuda")
    ops.spmm_project(ip, ix, t["X"], H, t["Ws"], t["Wn"], "mean", agg=agg, agg_mode="save")
    out = ops.spmm_project(ip, None, None, H, t["Ws"], t["Wn"], "mean", agg=agg, agg_mode="load")
    assert torch.equal(_bits(out), _bits(plain))


def test_empty_problem_launches_nothing(tables):
    from gnnrec import _lib, ops
    t = tables
    ip, ix, _, H, _, _ = t["csr"][0]
    agg = torch.empty((0, D), device="cuda")
    for mode in ("save", "load"):
        out = ops.spmm_project(ip, ix, t["X"], H, t["Ws"], t["Wn"], "mean", agg=agg, agg_mode=mode)
        assert tuple(out.shape) == (0, D)
    # the entry itself: an empty problem is accepted before any pointer is looked at
    lib = _lib.load()
    rc = lib.gnnrec_spmm_project_agg_f32(None, None, None, None, 128, None, 128, None, None, None,
                                         None, 0, 128, _lib.REDUCE_MEAN, 0, _lib.ACC_STORE, 0.0,
                                         None, None, None, 128, None, 128, _lib.AGG_LOAD, None)
    assert rc == _lib.OK


def test_bad_aggregate_arguments_are_refused(tables):
    """The library's own refusals (before anything is launched), through the C entry and,
    for what a tensor can express, through the op."""
    from gnnrec import _lib, ops
    t = tables
    ip, ix, _, H, _, _ = t["csr"][17]
    lib = _lib.load()
    out = torch.empty((17, D), device="cuda")
    WsT, WnT = t["Ws"].t().contiguous(), t["Wn"].t().contiguous()
    room = torch.empty(17 * D + 4, device="cuda")

    def call(agg_ptr, lda, mode):
        P = ctypes.c_void_p
        return lib.gnnrec_spmm_project_agg_f32(
            P(ip.data_ptr()), P(ix.data_ptr()), None, P(t["X"].data_ptr()), D, P(H.data_ptr()), D,
            P(WsT.data_ptr()), P(WnT.data_ptr()), None, None, 17, D, _lib.REDUCE_MEAN, 0,
            _lib.ACC_STORE, 0.0, None, None, P(out.data_ptr()), D,
            None if agg_ptr is None else P(agg_ptr), lda, mode,
            P(torch.cuda.current_stream().cuda_stream))

    def refused(rc, text):
        err = lib.gnnrec_last_error().decode()
        assert rc == 1 and err.startswith("gnnrec_spmm_project_agg_f32:") and text in err, (rc, err)

    for mode in (_lib.AGG_SAVE, _lib.AGG_LOAD):
        refused(call(None, D, mode), "the aggregate mode needs agg")
        refused(call(room.data_ptr() + 4, D, mode), "agg needs 16-B aligned rows")
        refused(call(room.data_ptr(), D - 4, mode), "agg needs 16-B aligned rows of lda >= 128")
    refused(call(room.data_ptr(), D, 7), "unknown aggregate mode 7")
    # through the op: a misaligned view raises the library's message as a ValueError
    skew = room[1:1 + 17 * D].view(17, D)
    with pytest.raises(ValueError, match="agg needs 16-B aligned rows"):
        ops.spmm_project(ip, ix, t["X"], H, t["Ws"], t["Wn"], "mean", agg=skew, agg_mode="save")
    with pytest.raises(ValueError, match="agg and agg_mode go together"):
        ops.spmm_project(ip, ix, t["X"], H, t["Ws"], t["Wn"], "mean", agg_mode="load")
    with pytest.raises(ValueError, match="runs on the valu kernel"):
        ops.spmm_project(ip, ix, t["X"], H, t["Ws"], t["Wn"], "mean", agg=out.clone(),
                         agg_mode="save", variant="mfma")
    torch.cuda.synchronize()
