// torch_sampler.cpp — the sampler and loader ops of TORCH_LIBRARY(gnnrec): the per-layer
// sampler and its relabel (dgl samplers / to_block, src/sampling.py:153-161), the fused
// sample_blocks, the row gathers and the loaders' batch head.  Same conventions as
// torch_ops.cpp: thin validated wrappers of the C ABI, mutated outputs declared in the schema.
#include <algorithm>
#include <map>
#include <utility>
#include <vector>

#include "torch_common.hpp"

namespace {

using namespace gnnrec_torch;

// ---------------------------------------------------------------- a9 sampler / relabel
// the operands both sampling phases take.  excluded_rows flags one byte per destination row
// (the kernels index it by the seed's global id) and only narrows the exclusion: it means
// nothing without the eid mask
void check_sample_operands(const Tensor& indptr, const Tensor& eids, const Tensor& seeds,
                           const optional<Tensor>& excluded,
                           const optional<Tensor>& excluded_rows) {
  dev(indptr, "indptr", at::kLong);
  dev(eids, "eids", at::kLong);
  dev(excluded, "excluded", at::kByte);
  dev(excluded_rows, "excluded_rows", at::kByte);
  dev(seeds, "seeds", at::kLong);
  if (!has(excluded_rows)) return;
  TORCH_CHECK_VALUE(has(excluded), "excluded_rows given without the excluded eid mask");
  TORCH_CHECK_VALUE(excluded_rows->numel() >= indptr.numel() - 1,
                    "excluded_rows must hold one flag per destination row (",
                    indptr.numel() - 1, "), got ", excluded_rows->numel());
}

void sample_count(const Tensor& indptr, const Tensor& eids, const optional<Tensor>& excluded,
                  const Tensor& seeds, int64_t fanout, int64_t seed_key, Tensor& counts,
                  const optional<Tensor>& excluded_rows) {
  const OneDevice one_device_;
  check_sample_operands(indptr, eids, seeds, excluded, excluded_rows);
  dev(counts, "counts", at::kLong);
  TORCH_CHECK_VALUE(counts.numel() >= seeds.numel(), "counts shorter than seeds");
  if (meta(seeds)) return;
  const c10::DeviceGuard g(seeds.device());
  ck(gnnrec_sample_count(p<int64_t>(indptr), p<int64_t>(eids), p<uint8_t>(excluded),
                         p<uint8_t>(excluded_rows), p<int64_t>(seeds), seeds.numel(), fanout,
                         (uint64_t)seed_key, p<int64_t>(counts), stream_of(seeds)),
     "gnnrec_sample_count");
}

void sample_fill(const Tensor& indptr, const Tensor& indices, const Tensor& eids,
                 const optional<Tensor>& excluded, const Tensor& seeds, int64_t fanout,
                 int64_t seed_key, const Tensor& out_indptr, Tensor& out_src, Tensor& out_eid,
                 const optional<Tensor>& excluded_rows) {
  const OneDevice one_device_;
  check_sample_operands(indptr, eids, seeds, excluded, excluded_rows);
  dev(indices, "indices", at::kInt);
  dev(out_indptr, "out_indptr", at::kLong);
  dev(out_src, "out_src", at::kLong);
  dev(out_eid, "out_eid", at::kLong);
  TORCH_CHECK_VALUE(out_indptr.numel() >= seeds.numel() + 1, "out_indptr shorter than seeds + 1");
  if (meta(seeds)) return;
  const c10::DeviceGuard g(seeds.device());
  ck(gnnrec_sample_fill(p<int64_t>(indptr), p<int32_t>(indices), p<int64_t>(eids),
                        p<uint8_t>(excluded), p<uint8_t>(excluded_rows), p<int64_t>(seeds),
                        seeds.numel(), fanout, (uint64_t)seed_key, p<int64_t>(out_indptr),
                        p<int64_t>(out_src), p<int64_t>(out_eid), stream_of(seeds)),
     "gnnrec_sample_fill");
}

void exclusive_scan(const Tensor& x, Tensor& out, Tensor& ws) {
  const OneDevice one_device_;
  dev(out, "out", at::kLong);
  TORCH_CHECK_VALUE(x.is_cuda() || x.is_meta(), "x must be a HIP device tensor");
  TORCH_CHECK_VALUE(x.scalar_type() == at::kLong || x.scalar_type() == at::kInt,
                    "exclusive_scan supports int32/int64");
  TORCH_CHECK_VALUE(x.is_contiguous() && out.numel() == x.numel() + 1,
                    "exclusive_scan: contiguous x [n] and out [n+1]");
  if (meta(x)) return;
  const c10::DeviceGuard g(x.device());
  if (x.scalar_type() == at::kLong)
    ck(gnnrec_exclusive_scan_i64(p<int64_t>(x), x.numel(), p<int64_t>(out), ws.data_ptr(),
                                 stream_of(x)),
       "gnnrec_exclusive_scan_i64");
  else
    ck(gnnrec_exclusive_scan_i32(p<int32_t>(x), x.numel(), p<int64_t>(out), ws.data_ptr(),
                                 stream_of(x)),
       "gnnrec_exclusive_scan_i32");
}

void mark_ids(const Tensor& ids, const Tensor& prefix_pos, Tensor& mark) {
  const OneDevice one_device_;
  dev(ids, "ids", at::kLong);
  dev(prefix_pos, "prefix_pos", at::kLong);
  dev(mark, "mark", at::kInt);
  if (meta(ids)) return;
  const c10::DeviceGuard g(ids.device());
  ck(gnnrec_mark_ids(p<int64_t>(ids), ids.numel(), p<int64_t>(prefix_pos), p<int32_t>(mark),
                     stream_of(ids)),
     "gnnrec_mark_ids");
}

void relabel_ids(const Tensor& ids, const Tensor& prefix_pos, const Tensor& rank, int64_t n_prefix,
                 Tensor& local) {
  const OneDevice one_device_;
  dev(ids, "ids", at::kLong);
  dev(prefix_pos, "prefix_pos", at::kLong);
  dev(rank, "rank", at::kLong);
  dev(local, "local", at::kLong);
  TORCH_CHECK_VALUE(local.numel() >= ids.numel(), "local shorter than ids");
  if (meta(ids)) return;
  const c10::DeviceGuard g(ids.device());
  ck(gnnrec_relabel_ids(p<int64_t>(ids), ids.numel(), p<int64_t>(prefix_pos), p<int64_t>(rank),
                        n_prefix, p<int64_t>(local), stream_of(ids)),
     "gnnrec_relabel_ids");
}

void compact_marked(const Tensor& mark, const Tensor& rank, Tensor& out_ids) {
  const OneDevice one_device_;
  dev(mark, "mark", at::kInt);
  dev(rank, "rank", at::kLong);
  dev(out_ids, "out_ids", at::kLong);
  if (meta(mark)) return;
  const c10::DeviceGuard g(mark.device());
  ck(gnnrec_compact_marked(p<int32_t>(mark), p<int64_t>(rank), mark.numel(), p<int64_t>(out_ids),
                           stream_of(mark)),
     "gnnrec_compact_marked");
}

void set_prefix_pos(const Tensor& prefix, Tensor& prefix_pos) {
  const OneDevice one_device_;
  dev(prefix, "prefix", at::kLong);
  dev(prefix_pos, "prefix_pos", at::kLong);
  if (meta(prefix)) return;
  const c10::DeviceGuard g(prefix.device());
  ck(gnnrec_set_prefix_pos(p<int64_t>(prefix), prefix.numel(), p<int64_t>(prefix_pos),
                           stream_of(prefix)),
     "gnnrec_set_prefix_pos");
}

void clear_prefix_pos(const Tensor& prefix, Tensor& prefix_pos) {
  const OneDevice one_device_;
  dev(prefix, "prefix", at::kLong);
  dev(prefix_pos, "prefix_pos", at::kLong);
  if (meta(prefix)) return;
  const c10::DeviceGuard g(prefix.device());
  ck(gnnrec_clear_prefix_pos(p<int64_t>(prefix), prefix.numel(), p<int64_t>(prefix_pos),
                             stream_of(prefix)),
     "gnnrec_clear_prefix_pos");
}

Tensor exclusive_scan_new(const Tensor& x) {
  const OneDevice one_device_;
  const int64_t n = x.numel();
  Tensor out = at::empty({n + 1}, x.options().dtype(at::kLong));
  Tensor ws = at::empty({std::max<int64_t>(1, (gnnrec_scan_workspace_bytes(n) + 7) / 8)},
                        x.options().dtype(at::kLong));
  exclusive_scan(x, out, ws);
  return out;
}

// the last element of every tensor (a scan's total) in ONE device -> host copy
std::vector<int64_t> read_last(const std::vector<Tensor>& scans) {
  std::vector<Tensor> last;
  for (const Tensor& t : scans) last.push_back(t.narrow(0, t.numel() - 1, 1));
  const Tensor h = at::cat(last).to(at::kCPU);
  return std::vector<int64_t>(h.data_ptr<int64_t>(), h.data_ptr<int64_t>() + h.numel());
}

// The to_block relabel of one node type (the C++ form of ops.Relabeler, gnnrec/ops.py): the
// prefix keeps its positions, the new ids follow in ascending order.  Three phases, so a
// caller can batch the count read-back of several types (read_last of every `rank`) and
// choose whether it comes before finish (an exact node list) or after it (a capacity):
//   begin   set the prefix map, mark the lists' ids, scan the marks -> rank
//   finish  the node list [prefix | tail new ids], every list's local ids
//   reset   the scratch (prefix_pos = -1, mark = 0) restored by touching only what was set
struct Relabel {
  Tensor prefix, prefix_pos, mark;  // the dst ids and the type's scratch (int64 / int32 [n])
  std::vector<Tensor> lists;        // global ids (negative: skipped, local = -1)
  Tensor rank, nodes;

  void begin() {
    set_prefix_pos(prefix, prefix_pos);
    for (const Tensor& ids : lists) mark_ids(ids, prefix_pos, mark);
    rank = exclusive_scan_new(mark);
  }
  // tail: the room for new ids — their exact count, or a capacity of at least that;
  // out[i] (optional): where list i's local ids are written (a fresh tensor otherwise)
  std::vector<Tensor> finish(int64_t tail, std::vector<Tensor> out = {}) {
    const int64_t n_p = prefix.numel();
    const auto i64 = prefix.options().dtype(at::kLong);
    nodes = at::empty({n_p + tail}, i64);
    nodes.narrow(0, 0, n_p).copy_(prefix);
    if (tail) {
      Tensor fresh = nodes.narrow(0, n_p, tail);
      compact_marked(mark, rank, fresh);
    }
    out.resize(lists.size());
    for (size_t i = 0; i < lists.size(); ++i) {
      if (!out[i].defined()) out[i] = at::empty({lists[i].numel()}, i64);
      relabel_ids(lists[i], prefix_pos, rank, n_p, out[i]);
    }
    return out;
  }
  // -> the node list cut to its n_new real new ids
  Tensor reset(int64_t n_new) {
    const int64_t n_p = prefix.numel();
    clear_prefix_pos(prefix, prefix_pos);
    if (n_new) mark.index_fill_(0, nodes.narrow(0, n_p, n_new), 0);
    return nodes.narrow(0, 0, n_p + n_new);
  }
};

// ---------------------------------------------------------------- a9 one sampled layer
// The whole of one block layer of BlockSampler.sample_blocks (gnnrec/sampling.py) issued
// from C++: per relation count -> scan; ONE host read of the sampled edge counts; fills;
// per node type the to_block relabel (prefix map, marks of the new sources, scan); ONE
// host read of the new-source counts; compaction, relabel of every relation's sources,
// scratch reset.  The same kernels in the same order with the same keys as the Python
// form it replaces (bitwise the same blocks), minus ≈ 40 Python-level launches per layer
// (the C2 step's sampler spent 1.5 ms of host time per batch on them).
//   relations r: CSR (indptr, indices int32, eids), optional exclusion mask, source / dst
//   node-type index, fanout (-1 = all), RNG key; node types t: the seeds (dst prefix) and
//   the Relabeler scratch (prefix_pos int64 [n_t] = -1, mark int32 [n_t] = 0, restored on
//   exit).  Returns per relation (out indptr, local src int32, eids), per type the src
//   node ids (prefix first), and the edge counts.
std::tuple<std::vector<Tensor>, std::vector<Tensor>, std::vector<Tensor>, std::vector<Tensor>,
           std::vector<int64_t>>
sample_layer(at::TensorList indptrs, at::TensorList indices, at::TensorList eids,
             const c10::List<optional<Tensor>>& masks,
             const c10::List<optional<Tensor>>& mask_rows, at::IntArrayRef src_type,
             at::IntArrayRef dst_type, at::IntArrayRef fanouts, at::IntArrayRef keys,
             at::TensorList seeds, at::TensorList prefix_pos, at::TensorList marks) {
  const OneDevice one_device_;
  const size_t R = indptrs.size(), NT = seeds.size();
  TORCH_CHECK_VALUE(indices.size() == R && eids.size() == R && masks.size() == R &&
                        mask_rows.size() == R &&
                        src_type.size() == R && dst_type.size() == R && fanouts.size() == R &&
                        keys.size() == R,
                    "sample_layer: one entry per relation in every relation list");
  TORCH_CHECK_VALUE(prefix_pos.size() == NT && marks.size() == NT,
                    "sample_layer: one seed list and one scratch pair per node type");
  for (size_t r = 0; r < R; ++r)
    TORCH_CHECK_VALUE(src_type[r] >= 0 && (size_t)src_type[r] < NT && dst_type[r] >= 0 &&
                          (size_t)dst_type[r] < NT,
                      "sample_layer: node-type index out of range");
  TORCH_CHECK_VALUE(NT > 0, "sample_layer: no node types");
  const c10::DeviceGuard g(seeds[0].device());
  // Bounded fanouts (every relation samples at most fanout >= 0 in-edges per seed): the
  // fills write into capacity-sized buffers (seeds x fanout, unused tail = -1, which the
  // mark / relabel kernels skip) and the new-source scan runs before any size is known,
  // so the layer's edge counts and new-node counts come back in ONE readback.  Unbounded
  // (full-neighbour) layers read the edge counts first to size the fills (two readbacks).
  bool bounded = true;
  for (size_t r = 0; r < R; ++r) bounded = bounded && fanouts[r] >= 0;
  // counts -> out indptr per relation
  std::vector<Tensor> o_ip(R), o_src(R), o_eid(R), src_loc(R), src_nid(NT);
  for (size_t r = 0; r < R; ++r) {
    const Tensor& sd = seeds[dst_type[r]];
    Tensor counts = at::empty({sd.numel()}, sd.options().dtype(at::kLong));
    const optional<Tensor> m = masks.get(r);
    sample_count(indptrs[r], eids[r], m, sd, fanouts[r], keys[r], counts, mask_rows.get(r));
    o_ip[r] = exclusive_scan_new(counts);
  }
  std::vector<int64_t> totals(R, 0);
  if (R && !bounded) totals = read_last(o_ip);  // the unbounded layer's first readback
  for (size_t r = 0; r < R; ++r) {
    const Tensor& sd = seeds[dst_type[r]];
    const int64_t cap = bounded ? sd.numel() * fanouts[r] : totals[r];
    o_src[r] = bounded ? at::full({cap}, -1, sd.options().dtype(at::kLong))
                       : at::empty({cap}, sd.options().dtype(at::kLong));
    o_eid[r] = at::empty({cap}, sd.options().dtype(at::kLong));
    const optional<Tensor> m = masks.get(r);
    sample_fill(indptrs[r], indices[r], eids[r], m, sd, fanouts[r], keys[r], o_ip[r], o_src[r],
                o_eid[r], mask_rows.get(r));
  }
  // relabel: per node type, mark the new sources and scan
  std::vector<Relabel> rel(NT);
  std::vector<Tensor> scans = o_ip;  // (bounded) every count of the layer: edges, then new nodes
  for (size_t t = 0; t < NT; ++t) {
    rel[t] = Relabel{seeds[t], prefix_pos[t], marks[t]};
    for (size_t r = 0; r < R; ++r)
      if ((size_t)src_type[r] == t) rel[t].lists.push_back(o_src[r]);
    rel[t].begin();
    scans.push_back(rel[t].rank);
  }
  // the room for new sources of type t.  Bounded: at most the sampled edges from it and at
  // most the type's nodes, so the local source ids and the fresh nodes are queued before any
  // count is on the host; unbounded: the counts themselves
  std::vector<int64_t> n_new(NT, 0);
  if (bounded) {
    for (size_t t = 0; t < NT; ++t) {
      for (const Tensor& ids : rel[t].lists) n_new[t] += ids.numel();
      n_new[t] = std::min(n_new[t], marks[t].numel());
    }
  } else {  // the layer's second size readback
    n_new = read_last(std::vector<Tensor>(scans.begin() + R, scans.end()));
  }
  for (size_t t = 0; t < NT; ++t) {
    const std::vector<Tensor> loc = rel[t].finish(n_new[t]);
    for (size_t r = 0, i = 0; r < R; ++r)
      if ((size_t)src_type[r] == t) src_loc[r] = loc[i++];
  }
  if (bounded) {  // the layer's one size readback
    const std::vector<int64_t> h = read_last(scans);
    totals.assign(h.begin(), h.begin() + R);
    n_new.assign(h.begin() + R, h.end());
  }
  for (size_t t = 0; t < NT; ++t) src_nid[t] = rel[t].reset(n_new[t]);
  for (size_t r = 0; r < R; ++r) {
    o_eid[r] = o_eid[r].narrow(0, 0, totals[r]);
    src_loc[r] = src_loc[r].narrow(0, 0, totals[r]).to(at::kInt);
  }
  return {o_ip, src_loc, o_eid, src_nid, totals};
}

// ---------------------------------------------------------------- a10 row gathers
// one checked gather out = src[idx] of op's job j; with n_dev (one device int64: a producer's
// count) only the first min(*n_dev, n) rows.  Rows are copied as flat byte runs: within a row
// the elements must be contiguous
gnnrec_gather_job gather_job(const char* op, size_t j, const Tensor& src, const Tensor& idx,
                             const Tensor& out, const int64_t* n_dev) {
  dev(idx, "idx", at::kLong);
  TORCH_CHECK_VALUE(src.is_cuda() || src.is_meta(),
                    "src: expected a device tensor (there is no CPU path)");
  same_dev(src, "src");
  same_dev(out, "out");
  TORCH_CHECK_VALUE(src.dim() >= 1 && out.dim() == src.dim() &&
                        out.scalar_type() == src.scalar_type() && idx.is_contiguous() &&
                        out.size(0) == idx.numel() && out.is_contiguous(),
                    op, ": job ", j, ": out [n, ...] of src's dtype and rank, contiguous idx [n]");
  int64_t inner = 1;
  for (int64_t k = src.dim() - 1; k >= 1; --k) {
    TORCH_CHECK_VALUE(out.size(k) == src.size(k), op, ": row shapes differ");
    TORCH_CHECK_VALUE(src.size(k) <= 1 || src.stride(k) == inner, op,
                      ": src rows must be contiguous (stride ", src.stride(k), " in dim ", k, ")");
    inner *= src.size(k);
  }
  const int64_t es = src.element_size();
  return gnnrec_gather_job{src.data_ptr(), src.stride(0) * es, p<int64_t>(idx), idx.numel(),
                           inner * es, out.data_ptr(), inner * es, n_dev};
}

void gather_rows(const Tensor& src, const Tensor& idx, Tensor& out) {
  const OneDevice one_device_;
  const gnnrec_gather_job j = gather_job("gather_rows", 0, src, idx, out, nullptr);
  if (meta(src)) return;
  const c10::DeviceGuard g(src.device());
  ck(gnnrec_gather_rows(j.src, j.src_ld_bytes, j.idx, j.n, j.row_bytes, j.dst, j.dst_ld_bytes,
                        stream_of(src)),
     "gnnrec_gather_rows");
}

// the inverse: dst[idx[i]] = src[i] (idx strictly ascending; ids outside dst's rows are skipped)
void scatter_rows(const Tensor& src, const Tensor& idx, Tensor& dst) {
  const OneDevice one_device_;
  dev(idx, "idx", at::kLong);
  TORCH_CHECK_VALUE(src.is_cuda() || src.is_meta(),
                    "src: expected a device tensor (there is no CPU path)");
  same_dev(src, "src");
  same_dev(dst, "dst");
  TORCH_CHECK_VALUE(src.dim() >= 1 && dst.dim() == src.dim() &&
                        dst.scalar_type() == src.scalar_type() && idx.is_contiguous() &&
                        src.size(0) == idx.numel() && src.is_contiguous(),
                    "scatter_rows: src [n, ...] contiguous, of dst's dtype and rank, contiguous "
                    "idx [n]");
  int64_t inner = 1;
  for (int64_t k = dst.dim() - 1; k >= 1; --k) {
    TORCH_CHECK_VALUE(dst.size(k) == src.size(k), "scatter_rows: row shapes differ");
    TORCH_CHECK_VALUE(dst.size(k) <= 1 || dst.stride(k) == inner,
                      "scatter_rows: dst rows must be contiguous (stride ", dst.stride(k),
                      " in dim ", k, ")");
    inner *= dst.size(k);
  }
  TORCH_CHECK_VALUE(dst.size(0) <= 1 || dst.stride(0) >= inner,
                    "scatter_rows: dst rows overlap");
  if (meta(src)) return;
  const c10::DeviceGuard g(src.device());
  const int64_t es = src.element_size();
  ck(gnnrec_scatter_rows(src.data_ptr(), inner * es, p<int64_t>(idx), idx.numel(), inner * es,
                         dst.data_ptr(), (dst.size(0) > 1 ? dst.stride(0) : inner) * es,
                         dst.size(0), stream_of(src)),
     "gnnrec_scatter_rows");
}

// several row gathers in one launch (gnnrec_gather_rows_batch): out[j] = src[j][idx[j]]
void gather_rows_batch(at::TensorList src, at::TensorList idx, at::TensorList out,
                       at::TensorList n_dev) {
  const OneDevice one_device_;
  const size_t n = src.size();
  TORCH_CHECK_VALUE(idx.size() == n && out.size() == n && n <= GNNREC_GATHER_MAX_JOBS &&
                        (n_dev.empty() || n_dev.size() == n),
                    "gather_rows_batch: one idx and out (and n_dev, if any) per src, at most ",
                    GNNREC_GATHER_MAX_JOBS, " jobs");
  std::vector<gnnrec_gather_job> jobs(n);
  for (size_t j = 0; j < n; ++j) {
    // n_dev[j] (one device int64, or empty): rows min(*n_dev, n) — a producer's count
    const int64_t* cnt = nullptr;
    if (!n_dev.empty() && n_dev[j].numel() > 0) {
      dev(n_dev[j], "n_dev", at::kLong);
      TORCH_CHECK_VALUE(n_dev[j].numel() == 1, "gather_rows_batch: n_dev entries hold one count");
      cnt = p<int64_t>(n_dev[j]);
    }
    jobs[j] = gather_job("gather_rows_batch", j, src[j], idx[j], out[j], cnt);
  }
  if (n == 0 || meta(src[0])) return;
  const c10::DeviceGuard g(src[0].device());
  ck(gnnrec_gather_rows_batch(jobs.data(), (int)n, stream_of(src[0])), "gnnrec_gather_rows_batch");
}

// ---------------------------------------------------------------- a9 fused sample_blocks
// The one owner of the fused sampler's size layout (include/gnnrec.h, gnnrec_sample_blocks):
// the device `sizes` array holds the node counts [-1..L-1][T] (row -1: the seeds), then the
// edge counts [L][R].  The host record the op returns appends the dump rows [L][T] and holds
// either the actual sizes (dump rows zero) or, at static shapes, the capacities.
struct SampleLayout {
  int64_t L, T, R;
  int64_t node(int64_t s, int64_t t) const { return (s + 1) * T + t; }  // s = -1: the seeds
  int64_t edge(int64_t s, int64_t r) const { return (L + 1) * T + s * R + r; }
  int64_t dump(int64_t s, int64_t t) const { return n_sizes() + s * T + t; }
  int64_t n_sizes() const { return (L + 1) * T + L * R; }
  int64_t n_record() const { return n_sizes() + L * T; }

  // the plan's capacities as a host record (the C ABI's strided arrays read once); a step's
  // seed capacity is the node capacity of the step before it
  std::vector<int64_t> caps(const gnnrec_sample_plan& P, int64_t* ws_bytes) const {
    int64_t seed_cap[GNNREC_SB_MAX_STEPS * GNNREC_SB_MAX_TYPES];
    int64_t edge_cap[GNNREC_SB_MAX_STEPS * GNNREC_SB_MAX_RELS];
    int64_t node_cap[GNNREC_SB_MAX_STEPS * GNNREC_SB_MAX_TYPES];
    int64_t dump_rows[GNNREC_SB_MAX_STEPS * GNNREC_SB_MAX_TYPES];
    ck(gnnrec_sample_blocks_caps(&P, seed_cap, edge_cap, node_cap, dump_rows, ws_bytes),
       "gnnrec_sample_blocks_caps");
    std::vector<int64_t> rec(n_record());
    for (int64_t t = 0; t < T; ++t) rec[node(-1, t)] = seed_cap[t];
    for (int64_t s = 0; s < L; ++s) {
      for (int64_t t = 0; t < T; ++t) {
        rec[node(s, t)] = node_cap[s * GNNREC_SB_MAX_TYPES + t];
        rec[dump(s, t)] = dump_rows[s * GNNREC_SB_MAX_TYPES + t];
      }
      for (int64_t r = 0; r < R; ++r) rec[edge(s, r)] = edge_cap[s * GNNREC_SB_MAX_RELS + r];
    }
    return rec;
  }
};

// Every block of one bounded-fanout BlockSampler.sample_blocks call (gnnrec_sample_blocks:
// 1 + 3L launches, include/gnnrec.h) with ONE host read of the sizes at the end: outputs are
// allocated at their capacities and returned narrowed to the actual sizes.
//   relations r: global in-CSR, src / dst type index, exclusion (eids, COO dst, flag arrays:
//   all four or none); types t: node count, step-0 seeds, scratch (pos int64 [2n], bits int64
//   [2 ceil(n/64)], word_rank int64 [ceil(n/64) + 1]); fanouts / keys flattened [step][r].
//   -> per step s and relation r (flattened [s][r]): out_indptr [n_dst + 1], local src int32,
//   eids; per step and type ([s][t]): the source node ids (seeds first); the size record
//   (SampleLayout); the gathered block data.
// static_shapes: every output at its capacity, the actual sizes left in sizes_out on the
// device and nothing read back; the record holds the capacities.  The block data tables are
// gathered by exact calls only (a static batch's are read lazily, gnnrec/graph.py LazyRows).
std::tuple<std::vector<Tensor>, std::vector<Tensor>, std::vector<Tensor>, std::vector<Tensor>,
           std::vector<int64_t>, std::vector<Tensor>>
sample_blocks(at::TensorList indptrs, at::TensorList indices, at::TensorList eids,
              at::IntArrayRef src_type, at::IntArrayRef dst_type,
              const c10::List<optional<Tensor>>& excl_eids,
              const c10::List<optional<Tensor>>& coo_dst,
              const c10::List<optional<Tensor>>& excl_masks,
              const c10::List<optional<Tensor>>& excl_rows, at::IntArrayRef n_nodes,
              at::TensorList seeds, at::TensorList pos, at::TensorList bits,
              at::TensorList word_rank, at::TensorList marks, at::IntArrayRef fanouts,
              at::IntArrayRef keys, int64_t steps, int64_t stamp, bool static_shapes,
              const optional<Tensor>& sizes_out,
              at::IntArrayRef node_cap_hint, const optional<Tensor>& overflow,
              at::TensorList edge_tables, at::IntArrayRef edge_table_rel,
              at::TensorList node_tables, at::IntArrayRef node_table_type,
              at::TensorList edge_recs) {
  const OneDevice one_device_;
  const size_t R = indptrs.size(), NT = n_nodes.size();
  TORCH_CHECK_VALUE(edge_recs.empty() || edge_recs.size() == R,
                    "sample_blocks: edge_recs holds one packed record array per relation or none");
  TORCH_CHECK_VALUE(indices.size() == R && eids.size() == R && src_type.size() == R &&
                        dst_type.size() == R && excl_eids.size() == R && coo_dst.size() == R &&
                        excl_masks.size() == R && excl_rows.size() == R,
                    "sample_blocks: one entry per relation in every relation list");
  TORCH_CHECK_VALUE(seeds.size() == NT && pos.size() == NT && bits.size() == NT &&
                        word_rank.size() == NT && marks.size() == NT,
                    "sample_blocks: one seed list and one scratch set per node type");
  TORCH_CHECK_VALUE(steps >= 1 && steps <= GNNREC_SB_MAX_STEPS && R <= GNNREC_SB_MAX_RELS &&
                        NT >= 1 && NT <= GNNREC_SB_MAX_TYPES,
                    "sample_blocks: ", steps, " steps, ", R, " relations, ", NT,
                    " types exceed the fused sampler's limits");
  TORCH_CHECK_VALUE((int64_t)fanouts.size() == steps * (int64_t)R &&
                        (int64_t)keys.size() == steps * (int64_t)R,
                    "sample_blocks: fanouts / keys must hold steps x relations entries");
  const SampleLayout lay{steps, (int64_t)NT, (int64_t)R};
  // static: the real counts stay on the device in sizes_out, where they drive the kernels
  // over the blocks; exact: the op reads them itself
  TORCH_CHECK_VALUE(has(sizes_out) == static_shapes,
                    "sample_blocks: sizes_out goes with static_shapes, and only with it");
  TORCH_CHECK_VALUE(!static_shapes || (edge_tables.empty() && node_tables.empty()),
                    "sample_blocks: data tables are gathered by exact calls only");
  TORCH_CHECK_VALUE(edge_table_rel.size() == edge_tables.size() &&
                        node_table_type.size() == node_tables.size(),
                    "sample_blocks: one relation / node type per data table");
  gnnrec_sample_plan P{};
  P.n_rels = (int)R;
  P.n_types = (int)NT;
  P.n_steps = (int)steps;
  P.stamp = (uint32_t)stamp;
  P.static_shapes = static_shapes ? 1 : 0;
  // static capacity hints [step][type] (empty: none) and the overflow flag they may raise
  TORCH_CHECK_VALUE(node_cap_hint.empty() || (int64_t)node_cap_hint.size() == steps * (int64_t)NT,
                    "sample_blocks: node_cap_hint must hold steps x types entries");
  for (int64_t s = 0; s < steps && !node_cap_hint.empty(); ++s)
    for (size_t t = 0; t < NT; ++t) P.node_cap_hint[s][t] = node_cap_hint[s * NT + t];
  if (has(overflow)) {
    dev(overflow, "overflow", at::kLong);
    TORCH_CHECK_VALUE(overflow->numel() >= 1, "sample_blocks: overflow holds one flag");
    P.overflow = p<int64_t>(overflow);
  }
  for (size_t r = 0; r < R; ++r) {
    dev(indptrs[r], "indptr", at::kLong);
    dev(indices[r], "indices", at::kInt);
    dev(eids[r], "eids", at::kLong);
    TORCH_CHECK_VALUE(src_type[r] >= 0 && (size_t)src_type[r] < NT && dst_type[r] >= 0 &&
                          (size_t)dst_type[r] < NT,
                      "sample_blocks: node-type index out of range");
    TORCH_CHECK_VALUE(indptrs[r].numel() == n_nodes[dst_type[r]] + 1 &&
                          eids[r].numel() == indices[r].numel(),
                      "sample_blocks: relation ", r, ": indptr must hold n_dst + 1 entries and "
                      "eids one per index");
    gnnrec_sample_rel& re = P.rel[r];
    re.indptr = p<int64_t>(indptrs[r]);
    re.indices = p<int32_t>(indices[r]);
    re.eids = p<int64_t>(eids[r]);
    if (!edge_recs.empty()) {  // {eid << 32 | src} per CSR edge (HeteroGraph.edge_records)
      dev(edge_recs[r], "edge_recs", at::kLong);
      TORCH_CHECK_VALUE(edge_recs[r].is_contiguous() && edge_recs[r].numel() == eids[r].numel(),
                        "sample_blocks: relation ", r, ": edge_recs must hold one record per edge");
      re.edge_rec = p<uint64_t>(edge_recs[r]);
    }
    re.src_type = (int32_t)src_type[r];
    re.dst_type = (int32_t)dst_type[r];
    const optional<Tensor> xe = excl_eids.get(r), cd = coo_dst.get(r), xm = excl_masks.get(r),
                           xr = excl_rows.get(r);
    TORCH_CHECK_VALUE(has(xe) == has(cd) && has(xe) == has(xm) && has(xe) == has(xr),
                      "sample_blocks: relation ", r,
                      ": exclusion needs the eids, the COO dst and both flag arrays");
    if (has(xe)) {
      dev(xe, "excl_eids", at::kLong);
      dev(cd, "coo_dst", at::kLong);
      dev(xm, "excl_mask", at::kByte);
      dev(xr, "excl_rows", at::kByte);
      TORCH_CHECK_VALUE(xe->is_contiguous() && cd->numel() == eids[r].numel() &&
                            xm->numel() == eids[r].numel() &&
                            xr->numel() == n_nodes[dst_type[r]],
                        "sample_blocks: relation ", r, ": exclusion arrays sized E, E, n_dst");
      re.excl_eids = p<int64_t>(xe);
      re.n_excl = xe->numel();
      re.coo_dst = p<int64_t>(cd);
      re.excl_mask = p<uint8_t>(xm);
      re.excl_rows = p<uint8_t>(xr);
    }
    for (int64_t s = 0; s < steps; ++s) {
      P.fanout[s][r] = fanouts[s * R + r];
      P.key[s][r] = (uint64_t)keys[s * R + r];
    }
  }
  for (size_t t = 0; t < NT; ++t) {
    dev(seeds[t], "seeds", at::kLong);
    dev(pos[t], "pos", at::kLong);
    dev(bits[t], "bits", at::kLong);
    dev(word_rank[t], "word_rank", at::kLong);
    dev(marks[t], "marks", at::kByte);
    const int64_t W = (n_nodes[t] + 63) / 64;
    TORCH_CHECK_VALUE(seeds[t].is_contiguous() && pos[t].numel() == 2 * n_nodes[t] &&
                          bits[t].numel() == 2 * W && word_rank[t].numel() == W + 1 &&
                          marks[t].numel() == 4 * 64 * W,
                      "sample_blocks: type ", t,
                      ": scratch sized 2n, 2 ceil(n/64), ceil(n/64)+1, 256 ceil(n/64) bytes");
    gnnrec_sample_type& ty = P.type[t];
    ty.n_nodes = n_nodes[t];
    ty.seeds = p<int64_t>(seeds[t]);
    ty.n_seeds = seeds[t].numel();
    ty.pos = p<int64_t>(pos[t]);
    ty.bits = p<uint64_t>(bits[t]);
    ty.word_rank = p<int64_t>(word_rank[t]);
    ty.marks = p<uint8_t>(marks[t]);
  }
  int64_t ws_bytes = 0;
  std::vector<int64_t> rec = lay.caps(P, &ws_bytes);  // the capacities, then (exact) the sizes
  const c10::DeviceGuard g(pos[0].device());
  const auto i64 = pos[0].options();
  std::vector<Tensor> o_ip(steps * R), o_src(steps * R), o_eid(steps * R), nodes(steps * NT);
  for (int64_t s = 0; s < steps; ++s) {
    for (size_t r = 0; r < R; ++r) {
      const int64_t ec = rec[lay.edge(s, r)];
      // the seed rows + 1, then (static) the destination type's dump rows
      o_ip[s * R + r] = at::empty(
          {rec[lay.node(s - 1, dst_type[r])] + 1 + rec[lay.dump(s, dst_type[r])]}, i64);
      o_src[s * R + r] = at::empty({ec}, i64.dtype(at::kInt));
      o_eid[s * R + r] = at::empty({ec}, i64);
      P.out_indptr[s][r] = p<int64_t>(o_ip[s * R + r]);
      P.out_src[s][r] = p<int32_t>(o_src[s * R + r]);
      P.out_eid[s][r] = p<int64_t>(o_eid[s * R + r]);
    }
    for (size_t t = 0; t < NT; ++t) {
      // static shapes: a node list also holds the next step's dump rows (the last step: one)
      const int64_t pad = !static_shapes ? 0 : s + 1 < steps ? rec[lay.dump(s + 1, t)] : 1;
      nodes[s * NT + t] = at::empty({rec[lay.node(s, t)] + pad}, i64);
      P.nodes[s][t] = p<int64_t>(nodes[s * NT + t]);
    }
  }
  if (static_shapes) {
    dev(sizes_out, "sizes_out", at::kLong);
    TORCH_CHECK_VALUE(sizes_out->numel() == lay.n_sizes() && sizes_out->is_contiguous(),
                      "sample_blocks: sizes_out must hold ", lay.n_sizes(), " entries");
  }
  Tensor sizes = static_shapes ? *sizes_out : at::empty({lay.n_sizes()}, i64);
  Tensor ws = at::empty({std::max<int64_t>(ws_bytes, 1)}, i64.dtype(at::kByte));
  P.sizes = p<int64_t>(sizes);
  P.workspace = ws.data_ptr();
  ck(gnnrec_sample_blocks(&P, stream_of(pos[0])), "gnnrec_sample_blocks");
  if (static_shapes) return {o_ip, o_src, o_eid, nodes, rec, std::vector<Tensor>{}};
  // the block data (a10): every step's edge data tables at its edge ids, the input block's
  // node tables at its source ids — queued behind the sampler, row counts read on the device,
  // ahead of the one size read below
  std::vector<Tensor> gathered;
  std::vector<int64_t> gathered_n;  // where each one's row count sits in the sizes
  std::vector<gnnrec_gather_job> jobs;
  auto add_job = [&](const Tensor& src, const Tensor& idx, int64_t n_at) {
    TORCH_CHECK_VALUE(src.dim() >= 1, "sample_blocks: data tables have rows");
    std::vector<int64_t> shape(src.sizes().begin(), src.sizes().end());
    shape[0] = idx.numel();
    gathered.push_back(at::empty(shape, src.options()));
    gathered_n.push_back(n_at);
    jobs.push_back(gather_job("sample_blocks", jobs.size(), src, idx, gathered.back(),
                              p<int64_t>(sizes) + n_at));
  };
  for (int64_t s = 0; s < steps; ++s)
    for (size_t j = 0; j < edge_tables.size(); ++j) {
      const int64_t r = edge_table_rel[j];
      TORCH_CHECK_VALUE(r >= 0 && (size_t)r < R, "sample_blocks: edge table relation");
      add_job(edge_tables[j], o_eid[s * R + r], lay.edge(s, r));
    }
  for (size_t j = 0; j < node_tables.size(); ++j) {
    const int64_t t = node_table_type[j];
    TORCH_CHECK_VALUE(t >= 0 && (size_t)t < NT, "sample_blocks: node table type");
    add_job(node_tables[j], nodes[(steps - 1) * NT + t], lay.node(steps - 1, t));
  }
  for (size_t i = 0; i < jobs.size(); i += GNNREC_GATHER_MAX_JOBS)
    ck(gnnrec_gather_rows_batch(jobs.data() + i,
                                (int)std::min<size_t>(GNNREC_GATHER_MAX_JOBS, jobs.size() - i),
                                stream_of(pos[0])),
       "gnnrec_gather_rows_batch");
  const Tensor hs = sizes.to(at::kCPU);  // the call's one size readback
  std::copy_n(hs.data_ptr<int64_t>(), lay.n_sizes(), rec.begin());  // (exact: no dump rows)
  for (int64_t s = 0; s < steps; ++s) {
    for (size_t r = 0; r < R; ++r) {
      const int64_t n_dst = rec[lay.node(s - 1, dst_type[r])], ne = rec[lay.edge(s, r)];
      o_ip[s * R + r] = o_ip[s * R + r].narrow(0, 0, n_dst + 1);
      o_src[s * R + r] = o_src[s * R + r].narrow(0, 0, ne);
      o_eid[s * R + r] = o_eid[s * R + r].narrow(0, 0, ne);
    }
    for (size_t t = 0; t < NT; ++t)
      nodes[s * NT + t] = nodes[s * NT + t].narrow(0, 0, rec[lay.node(s, t)]);
  }
  for (size_t i = 0; i < gathered.size(); ++i)
    gathered[i] = gathered[i].narrow(0, 0, rec[gathered_n[i]]);
  return {o_ip, o_src, o_eid, nodes, rec, gathered};
}

// a11: compact_graphs over id lists at static shapes (gnnrec_compact_ids): per node type the
// sorted distinct ids of its lists in nodes[t] [caps[t]] (-1 past the count), each list
// relabelled to local ids, the per-type counts left on the device — no host read, so a
// loader feeding a captured step keeps every shape fixed.  bits [2 ceil(n/64) +
// GNNREC_COMPACT_SCAN_WS(n)] and word_rank [ceil(n/64) + 1] per type; the bitmaps zero before
// the first call, parity alternating.
std::tuple<std::vector<Tensor>, std::vector<Tensor>, Tensor>
compact_ids(at::TensorList ids, at::IntArrayRef type, at::IntArrayRef n_nodes,
            at::IntArrayRef caps, at::TensorList bits, at::TensorList word_rank,
            at::TensorList marks, int64_t parity) {
  const OneDevice one_device_;
  const size_t L = ids.size(), NT = n_nodes.size();
  TORCH_CHECK_VALUE(type.size() == L && L <= GNNREC_COMPACT_MAX_LISTS && NT >= 1 &&
                        NT <= GNNREC_SB_MAX_TYPES && caps.size() == NT && bits.size() == NT &&
                        word_rank.size() == NT && marks.size() == NT,
                    "compact_ids: at most ", GNNREC_COMPACT_MAX_LISTS, " lists (one type each) "
                    "and 1..", GNNREC_SB_MAX_TYPES, " types (a cap and a scratch pair each)");
  TORCH_CHECK_VALUE(parity == 0 || parity == 1, "compact_ids: parity is 0 or 1");
  gnnrec_compact_type T[GNNREC_SB_MAX_TYPES] = {};
  gnnrec_compact_list Ls[GNNREC_COMPACT_MAX_LISTS] = {};
  const c10::DeviceGuard g(bits[0].device());
  const auto i64 = bits[0].options();
  std::vector<Tensor> nodes(NT), local(L);
  for (size_t t = 0; t < NT; ++t) {
    dev(bits[t], "bits", at::kLong);
    dev(word_rank[t], "word_rank", at::kLong);
    const int64_t W = (n_nodes[t] + 63) / 64;
    dev(marks[t], "marks", at::kByte);
    // bits: the two parity bitmaps, then the scan's workspace
    const int64_t ws = GNNREC_COMPACT_SCAN_WS(n_nodes[t]);
    TORCH_CHECK_VALUE(n_nodes[t] >= 0 && caps[t] >= 0 && bits[t].numel() == 2 * W + ws &&
                          word_rank[t].numel() == W + 1 && marks[t].numel() == 2 * 64 * W,
                      "compact_ids: type ", t, ": scratch sized 2 ceil(n/64) + ", ws,
                      ", ceil(n/64)+1, 128 ceil(n/64) bytes");
    nodes[t] = at::empty({caps[t]}, i64);
    T[t] = gnnrec_compact_type{n_nodes[t], p<uint64_t>(bits[t]), p<int64_t>(word_rank[t]),
                               p<int64_t>(nodes[t]), caps[t], p<uint8_t>(marks[t]),
                               p<uint64_t>(bits[t]) + 2 * W};
  }
  // the lists' local ids are consecutive views of one buffer (lists given one after the
  // other, e.g. an etype's positive then negative sources, come back joined)
  int64_t n_all = 0;
  for (size_t l = 0; l < L; ++l) n_all += ids[l].numel();
  const Tensor local_all = at::empty({n_all}, i64);
  int64_t off = 0;
  for (size_t l = 0; l < L; ++l) {
    dev(ids[l], "ids", at::kLong);
    TORCH_CHECK_VALUE(type[l] >= 0 && (size_t)type[l] < NT && ids[l].is_contiguous(),
                      "compact_ids: list ", l, ": type out of range or ids not contiguous");
    local[l] = local_all.narrow(0, off, ids[l].numel());
    off += ids[l].numel();
    Ls[l] = gnnrec_compact_list{p<int64_t>(ids[l]), ids[l].numel(), (int32_t)type[l],
                                p<int64_t>(local[l])};
  }
  Tensor count = at::empty({(int64_t)NT}, i64);
  ck(gnnrec_compact_ids(Ls, (int)L, T, (int)NT, (int)parity, p<int64_t>(count),
                        stream_of(bits[0])),
     "gnnrec_compact_ids");
  return {nodes, local, count};
}

// a12: many contiguous same-size copies dst[j] <- src[j] in one launch per 64
// (gnnrec_copy_batch: a static batch into a captured step's buffers, gnnrec/capture.py)
void copy_batch(at::TensorList src, at::TensorList dst) {
  const OneDevice one_device_;
  TORCH_CHECK_VALUE(src.size() == dst.size(), "copy_batch: one dst per src");
  std::vector<const void*> sp;
  std::vector<void*> dp;
  std::vector<int64_t> nb;
  for (size_t j = 0; j < src.size(); ++j) {
    TORCH_CHECK_VALUE(src[j].is_cuda() && dst[j].is_cuda(),
                      "copy_batch: device tensors (there is no CPU path)");
    same_dev(src[j], "src");
    same_dev(dst[j], "dst");
    TORCH_CHECK_VALUE(src[j].scalar_type() == dst[j].scalar_type() &&
                          src[j].sizes() == dst[j].sizes() && src[j].is_contiguous() &&
                          dst[j].is_contiguous(),
                      "copy_batch: job ", j, ": contiguous tensors of one dtype and shape");
    sp.push_back(src[j].data_ptr());
    dp.push_back(dst[j].data_ptr());
    nb.push_back(src[j].nbytes());
  }
  if (src.empty()) return;
  const c10::DeviceGuard g(src[0].device());
  for (size_t i = 0; i < sp.size(); i += GNNREC_COPY_MAX_JOBS) {
    const int n = (int)std::min<size_t>(GNNREC_COPY_MAX_JOBS, sp.size() - i);
    ck(gnnrec_copy_batch(sp.data() + i, dp.data() + i, nb.data() + i, n, stream_of(src[0])),
       "gnnrec_copy_batch");
  }
}

// EdgeDataLoader's batch head in one call (gnnrec/sampling.py _iter_batches): the batch's
// positive pairs (find_edges), the uniform negatives (src repeated K times, dst =
// randint(N_dst) from the default generator — the same draws as negative_sampler.Uniform),
// and DGL's compact_graphs([pos, neg]) over both (relabel per node type, ONE size
// readback), returning every pair list in local ids.  The same kernels, generator calls and
// order as the Python form it replaces (bitwise the same pair graphs), issued from C++ with
// the GIL released, so a prefetching loader thread leaves the training thread alone.
//   batch[r]: edge ids of relation r in the batch (empty: not in it); neg_order: the
//   relations in the order their negatives are drawn (the batch's type order)
std::tuple<std::vector<Tensor>, std::vector<Tensor>, std::vector<Tensor>, std::vector<Tensor>,
           std::vector<Tensor>>
edge_batch_pairs(at::TensorList rel_src, at::TensorList rel_dst, at::IntArrayRef src_type,
                 at::IntArrayRef dst_type, at::TensorList batch, at::IntArrayRef neg_order,
                 int64_t K, at::IntArrayRef n_nodes, at::TensorList prefix_pos,
                 at::TensorList marks) {
  const OneDevice one_device_;
  const size_t R = rel_src.size(), NT = n_nodes.size();
  TORCH_CHECK_VALUE(rel_dst.size() == R && src_type.size() == R && dst_type.size() == R &&
                        batch.size() == R && prefix_pos.size() == NT && marks.size() == NT &&
                        NT > 0,
                    "edge_batch_pairs: list lengths");
  for (size_t r = 0; r < R; ++r)
    TORCH_CHECK_VALUE(src_type[r] >= 0 && (size_t)src_type[r] < NT && dst_type[r] >= 0 &&
                          (size_t)dst_type[r] < NT,
                      "edge_batch_pairs: node-type index out of range");
  const c10::DeviceGuard g(prefix_pos[0].device());
  const auto opt = prefix_pos[0].options();  // int64 on the device
  const Tensor empty = at::empty({0}, opt);
  std::vector<Tensor> ps(R, empty), pd(R, empty), ns(R, empty), nd(R, empty);
  for (size_t r = 0; r < R; ++r) {
    if (batch[r].numel() == 0) continue;
    ps[r] = rel_src[r].index_select(0, batch[r]);
    pd[r] = rel_dst[r].index_select(0, batch[r]);
  }
  if (K > 0) {
    for (int64_t r : neg_order) {
      TORCH_CHECK_VALUE(r >= 0 && (size_t)r < R, "edge_batch_pairs: neg_order out of range");
      if (batch[r].numel() == 0) continue;
      ns[r] = ps[r].repeat_interleave(K);
      nd[r] = at::randint(0, n_nodes[dst_type[r]], {ns[r].numel()}, opt);
    }
  }
  // compact_graphs([pos, neg]): per node type the lists in (pos, neg) x relation order
  std::vector<std::vector<Tensor*>> lists(NT);
  for (auto* side : {&ps, &ns})
    for (size_t r = 0; r < R; ++r) {
      lists[src_type[r]].push_back(&(*side)[r]);
      auto& dlist = side == &ps ? pd : nd;
      lists[dst_type[r]].push_back(&dlist[r]);
    }
  // a relation's positive and negative local ids of one side are written into one buffer
  // [positives | negatives]: the cosine backward then joins them as a view, not a cat
  std::map<const Tensor*, Tensor> joined_out;
  for (size_t r = 0; r < R; ++r)
    for (auto side : {std::make_pair(&ps[r], &ns[r]), std::make_pair(&pd[r], &nd[r])}) {
      const int64_t a = side.first->numel(), b = side.second->numel();
      if (a == 0 || b == 0) continue;
      const Tensor buf = at::empty({a + b}, opt);
      joined_out[side.first] = buf.narrow(0, 0, a);
      joined_out[side.second] = buf.narrow(0, a, b);
    }
  std::vector<Relabel> rel(NT);  // no prefix: every id is new
  std::vector<Tensor> scans;
  for (size_t t = 0; t < NT; ++t) {
    rel[t] = Relabel{empty, prefix_pos[t], marks[t]};
    for (const Tensor* ids : lists[t]) rel[t].lists.push_back(*ids);
    rel[t].begin();
    scans.push_back(rel[t].rank);
  }
  const std::vector<int64_t> n_new = read_last(scans);  // the one size readback
  std::vector<Tensor> nodes(NT);
  for (size_t t = 0; t < NT; ++t) {
    std::vector<Tensor> out;
    for (const Tensor* ids : lists[t]) {
      const auto j = joined_out.find(ids);
      out.push_back(j != joined_out.end() ? j->second : Tensor());
    }
    const std::vector<Tensor> loc = rel[t].finish(n_new[t], out);
    for (size_t i = 0; i < loc.size(); ++i) *lists[t][i] = loc[i];  // the entry's local ids
    nodes[t] = rel[t].reset(n_new[t]);
  }
  return {nodes, ps, pd, ns, nd};
}

}  // namespace

// Schemas: mutated outputs are annotated (a!) so functionalisation knows what each op writes.
TORCH_LIBRARY_FRAGMENT(gnnrec, m) {
  m.def("sample_count(Tensor indptr, Tensor eids, Tensor? excluded, Tensor seeds, int fanout, "
        "int seed_key, Tensor(a!) counts, Tensor? excluded_rows=None) -> ()");
  m.def("sample_fill(Tensor indptr, Tensor indices, Tensor eids, Tensor? excluded, Tensor seeds, "
        "int fanout, int seed_key, Tensor out_indptr, Tensor(a!) out_src, Tensor(b!) out_eid, "
        "Tensor? excluded_rows=None) -> ()");
  m.def("exclusive_scan(Tensor x, Tensor(a!) out, Tensor(b!) workspace) -> ()");
  m.def("mark_ids(Tensor ids, Tensor prefix_pos, Tensor(a!) mark) -> ()");
  m.def("relabel_ids(Tensor ids, Tensor prefix_pos, Tensor rank, int n_prefix, "
        "Tensor(a!) local) -> ()");
  m.def("compact_marked(Tensor mark, Tensor rank, Tensor(a!) out_ids) -> ()");
  m.def("set_prefix_pos(Tensor prefix, Tensor(a!) prefix_pos) -> ()");
  m.def("clear_prefix_pos(Tensor prefix, Tensor(a!) prefix_pos) -> ()");
  m.def("gather_rows(Tensor src, Tensor idx, Tensor(a!) out) -> ()");
  m.def("scatter_rows(Tensor src, Tensor idx, Tensor(a!) dst) -> ()");
  m.def("edge_batch_pairs(Tensor[] rel_src, Tensor[] rel_dst, int[] src_type, int[] dst_type, "
        "Tensor[] batch, int[] neg_order, int K, int[] n_nodes, Tensor[] prefix_pos, "
        "Tensor[] marks) -> (Tensor[], Tensor[], Tensor[], Tensor[], Tensor[])");
  m.def("sample_layer(Tensor[] indptrs, Tensor[] indices, Tensor[] eids, Tensor?[] masks, "
        "Tensor?[] mask_rows, int[] src_type, int[] dst_type, int[] fanouts, int[] keys, Tensor[] seeds, "
        "Tensor(a!)[] prefix_pos, Tensor(b!)[] marks) -> "
        "(Tensor[] out_indptr, Tensor[] src_local, Tensor[] eids, Tensor[] src_nid, int[] n_edges)");
  m.def("sample_blocks(Tensor[] indptrs, Tensor[] indices, Tensor[] eids, int[] src_type, "
        "int[] dst_type, Tensor?[] excl_eids, Tensor?[] coo_dst, Tensor?[] excl_masks, "
        "Tensor?[] excl_rows, int[] n_nodes, Tensor[] seeds, Tensor(a!)[] pos, "
        "Tensor(b!)[] bits, Tensor(c!)[] word_rank, Tensor(f!)[] marks, int[] fanouts, "
        "int[] keys, int steps, "
        "int stamp, bool static_shapes, Tensor(d!)? sizes_out, int[] node_cap_hint, "
        "Tensor(e!)? overflow, Tensor[] edge_tables, int[] edge_table_rel, Tensor[] node_tables, "
        "int[] node_table_type, Tensor[] edge_recs) -> (Tensor[] out_indptr, Tensor[] src_local, Tensor[] eids, "
        "Tensor[] src_nid, int[] sizes, Tensor[] data)");
  m.def("gather_rows_batch(Tensor[] src, Tensor[] idx, Tensor(a!)[] out, Tensor[] n_dev) -> ()");
  m.def("copy_batch(Tensor[] src, Tensor(a!)[] dst) -> ()");
  m.def("compact_ids(Tensor[] ids, int[] type, int[] n_nodes, int[] caps, Tensor(a!)[] bits, "
        "Tensor(b!)[] word_rank, Tensor(c!)[] marks, int parity) -> (Tensor[] nodes, "
        "Tensor[] local, Tensor count)");
}

#define GNNREC_SAMPLER_IMPLS(m)                          \
  m.impl("sample_count", &sample_count);                 \
  m.impl("sample_fill", &sample_fill);                   \
  m.impl("exclusive_scan", &exclusive_scan);             \
  m.impl("mark_ids", &mark_ids);                         \
  m.impl("relabel_ids", &relabel_ids);                   \
  m.impl("compact_marked", &compact_marked);             \
  m.impl("set_prefix_pos", &set_prefix_pos);             \
  m.impl("clear_prefix_pos", &clear_prefix_pos);         \
  m.impl("gather_rows", &gather_rows);                   \
  m.impl("scatter_rows", &scatter_rows);                 \
  m.impl("gather_rows_batch", &gather_rows_batch)

// HIP tensors dispatch under the CUDA key in ROCm PyTorch.
TORCH_LIBRARY_IMPL(gnnrec, CUDA, m) {
  GNNREC_SAMPLER_IMPLS(m);
  m.impl("sample_layer", &sample_layer);  // data-dependent sizes: device only, no meta form
  m.impl("edge_batch_pairs", &edge_batch_pairs);
  m.impl("sample_blocks", &sample_blocks);
  m.impl("compact_ids", &compact_ids);
  m.impl("copy_batch", &copy_batch);
}
// Meta / fake tensors and CPU tensors: as in torch_ops.cpp, the same functions stop after
// their checks or refuse in their first operand check.
TORCH_LIBRARY_IMPL(gnnrec, Meta, m) { GNNREC_SAMPLER_IMPLS(m); }
TORCH_LIBRARY_IMPL(gnnrec, CPU, m) { GNNREC_SAMPLER_IMPLS(m); }
