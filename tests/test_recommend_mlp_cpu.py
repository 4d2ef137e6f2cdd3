"""CPU-side checks of the many-user top-k for the MLP head (gnnrec.recs.recommend(head=...),
the dense kernels of csrc/heads.hip and the scored-candidate ranking of csrc/recommend.hip):
the Meta kernels' argument checks, the refusal of CPU tensors, and — with the head restated
in torch on the host — the conditions tests/test_gpu_recommend_mlp.py leans on for its
inputs.  Nothing launches here."""
import numpy as np
import pytest
import torch

import recommend_cases as rc
import recommend_mlp_cases as mc


def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta")


def _T():
    from gnnrec import _lib
    return _lib.torch_ops()


def _head_meta():
    return _meta(32, 128), _meta(32), _meta(32), _meta(1)


def test_meta_dense_store():
    T = _T()
    P, Q = _meta(130, 128), _meta(5000, 128)
    T.edge_mlp_dense_store_f32(P, Q, *_head_meta(), _meta(130, 5000))
    T.edge_mlp_dense_store_f32(P, Q[:1024], *_head_meta(), _meta(130, 1024))
    with pytest.raises(ValueError, match="out must be"):
        T.edge_mlp_dense_store_f32(P, Q, *_head_meta(), _meta(130, 4999))
    with pytest.raises(ValueError, match="128/32 hidden sizes"):
        T.edge_mlp_dense_store_f32(_meta(130, 64), Q, *_head_meta(), _meta(130, 5000))
    with pytest.raises(ValueError, match="128/32 hidden sizes"):
        T.edge_mlp_dense_store_f32(P, Q, _meta(128, 32), _meta(32), _meta(32), _meta(1),
                                   _meta(130, 5000))
    with pytest.raises(ValueError, match="must be Float"):
        T.edge_mlp_dense_store_f32(P, _meta(5000, 128, dtype=torch.float16), *_head_meta(),
                                   _meta(130, 5000))
    with pytest.raises(ValueError, match="out must be Float"):
        T.edge_mlp_dense_store_f32(P, Q, *_head_meta(), _meta(130, 5000, dtype=torch.float64))


def test_meta_dense_filter():
    T = _T()
    i32 = torch.int32
    P, Q = _meta(130, 128), _meta(5000, 128)
    tau, cnt = _meta(130), _meta(130, dtype=i32)
    ci, cs = _meta(130, 1024, dtype=i32), _meta(130, 1024)
    T.edge_mlp_dense_filter_f32(P, Q, *_head_meta(), tau, cnt, ci, cs)
    with pytest.raises(ValueError, match="tau / counts"):
        T.edge_mlp_dense_filter_f32(P, Q, *_head_meta(), _meta(129), cnt, ci, cs)
    with pytest.raises(ValueError, match="cap must be"):
        T.edge_mlp_dense_filter_f32(P, Q, *_head_meta(), tau, cnt, _meta(130, 4097, dtype=i32),
                                    _meta(130, 4097))
    with pytest.raises(ValueError, match="cap must be"):
        T.edge_mlp_dense_filter_f32(P, Q, *_head_meta(), tau, cnt, _meta(130, 0, dtype=i32),
                                    _meta(130, 0))
    with pytest.raises(ValueError, match="cand_scores must be"):
        T.edge_mlp_dense_filter_f32(P, Q, *_head_meta(), tau, cnt, ci, _meta(130, 512))
    with pytest.raises(ValueError, match="cand_items must be Int"):
        T.edge_mlp_dense_filter_f32(P, Q, *_head_meta(), tau, cnt,
                                    _meta(130, 1024, dtype=torch.int64), cs)
    with pytest.raises(ValueError, match="cand_scores must be Float"):
        T.edge_mlp_dense_filter_f32(P, Q, *_head_meta(), tau, cnt, ci, _meta(130, 1024, dtype=i32))
    with pytest.raises(ValueError, match="128/32 hidden sizes"):
        T.edge_mlp_dense_filter_f32(P, Q, _meta(32, 64), _meta(32), _meta(32), _meta(1), tau, cnt,
                                    ci, cs)


def test_meta_topk_scored_candidates():
    T = _T()
    i32, i64 = torch.int32, torch.int64
    cnt, ci, cs = _meta(7, dtype=i32), _meta(7, 256, dtype=i32), _meta(7, 256)
    rows = _meta(7, dtype=i64)
    ip, ix = _meta(41, dtype=i64), _meta(400, dtype=i32)
    ov, oi = _meta(7, 10), _meta(7, 10, dtype=i64)
    T.topk_scored_candidates_f32(cnt, ci, cs, rows, ip, ix, 10, ov, oi)
    T.topk_scored_candidates_f32(cnt, ci, cs, None, None, None, 10, ov, oi)
    T.topk_scored_candidates_f32(cnt, ci, cs, None, _meta(8, dtype=i64), ix, 10, ov, oi)
    with pytest.raises(ValueError, match="k must be"):
        T.topk_scored_candidates_f32(cnt, ci, cs, rows, ip, ix, 257, _meta(7, 257),
                                     _meta(7, 257, dtype=i64))
    with pytest.raises(ValueError, match="cand_scores must be"):
        T.topk_scored_candidates_f32(cnt, ci, _meta(7, 128), rows, ip, ix, 10, ov, oi)
    with pytest.raises(ValueError, match="come together"):
        T.topk_scored_candidates_f32(cnt, ci, cs, rows, ip, None, 10, ov, oi)
    with pytest.raises(ValueError, match="exclude_indptr must be"):
        T.topk_scored_candidates_f32(cnt, ci, cs, None, _meta(7, dtype=i64), ix, 10, ov, oi)
    with pytest.raises(ValueError, match="exclude_indices must be Int"):
        T.topk_scored_candidates_f32(cnt, ci, cs, rows, ip, _meta(400, dtype=i64), 10, ov, oi)
    with pytest.raises(ValueError, match="user_rows must be"):
        T.topk_scored_candidates_f32(cnt, ci, cs, _meta(6, dtype=i64), ip, ix, 10, ov, oi)
    with pytest.raises(ValueError, match="out_vals / out_idx"):
        T.topk_scored_candidates_f32(cnt, ci, cs, rows, ip, ix, 10, _meta(7, 9), oi)


def test_cpu_tensors_are_refused():
    from gnnrec import ops, recs
    T = _T()
    pl = mc.head(16)
    tail = (pl.hidden_2.weight, pl.hidden_2.bias, pl.output.weight.reshape(-1), pl.output.bias)
    with pytest.raises(ValueError, match="HIP device tensor"):
        recs.recommend(torch.zeros(4, 16), torch.zeros(9, 16), 3, head=pl)
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.edge_mlp_dense_store(torch.zeros(4, 128), torch.zeros(9, 128), *tail)
    with pytest.raises(ValueError, match="HIP device tensor"):
        T.edge_mlp_dense_store_f32(torch.zeros(4, 128), torch.zeros(9, 128),
                                   *[t.detach() for t in tail], torch.zeros(4, 9))
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.edge_mlp_dense_filter(torch.zeros(4, 128), torch.zeros(9, 128), *tail,
                                  torch.zeros(4), torch.zeros(4, dtype=torch.int32),
                                  torch.zeros(4, 8, dtype=torch.int32), torch.zeros(4, 8))
    with pytest.raises(ValueError, match="HIP device tensor"):
        ops.topk_scored_candidates(torch.zeros(4, dtype=torch.int32),
                                   torch.zeros(4, 8, dtype=torch.int32), torch.zeros(4, 8), 3)


def test_head_of_the_wrong_width_is_refused():
    """hidden_1 must be [128, 2 d] for the tables' d: checked before anything launches (meta
    tensors stand in for device tensors)."""
    from gnnrec import recs
    with pytest.raises(ValueError, match="hidden_1 must be"):
        recs.recommend(_meta(4, 16), _meta(9, 16), 3, head=mc.head(32).to("meta"))


@pytest.mark.parametrize("d", mc.DIMS)
@pytest.mark.parametrize("kind", mc.KINDS)
def test_candidate_counts_stay_far_under_the_cap(kind, d):
    """The inputs of test_recommend_head_is_the_exhaustive_ranking: with the head restated on
    the host, every row keeps at most cand_cap / 2 = 512 items (the factor of two is the
    margin for device-versus-host rounding moving a threshold), and no score is exactly 0
    or 1.  Measured on the host with these tables and weights: the largest count is 426
    (normal, d = 16, k = 64); 109 at k = 10; 30 at k = 1."""
    hu, hi = rc.tables(kind, d)
    S = mc.host_scores(mc.head(d), hu, hi)
    assert S.dtype == np.float32 and S.shape == (rc.N_USERS, rc.N_ITEMS)
    assert ((S > 0) & (S < 1)).all()
    ip, ix = rc.exclusions()
    for k in mc.KS:
        counts = mc.filter_counts(S, ip, ix, k, rc.SAMPLE)
        print(f"{kind} d={d} k={k}: largest count {counts.max()}, mean {counts.mean():.1f}")
        assert k <= counts.min() and counts.max() <= rc.CAND_CAP // 2


def test_exact_ties_occur():
    """Why the GPU tests rank the device's own score matrix with the id tie-break instead of
    comparing to a host ranking: distinct items of one row do score the same fp32 value."""
    hu, hi = rc.tables("normal", 16)
    S = mc.host_scores(mc.head(16), hu, hi)
    ties = sum(S.shape[1] - np.unique(row).size for row in S)
    print(f"{ties} repeated values in the {S.shape[0]} x {S.shape[1]} matrix")
    assert ties > 0


def test_saturated_head_saturates():
    """The head of test_saturated_head_overflows: on the host restatement more than cand_cap
    items of every row are within one ulp of 1."""
    hu, hi = rc.tables("normal", 16)
    S = mc.host_scores(mc.saturated_head(16), hu, hi)
    near = (S >= np.nextafter(np.float32(1), np.float32(0))).sum(1)
    print(f"items within one ulp of 1 per row: min {near.min()}, mean {near.mean():.0f}")
    assert near.min() > rc.CAND_CAP
