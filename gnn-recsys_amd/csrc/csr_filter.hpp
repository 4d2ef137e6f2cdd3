// What the two stream compactions of a relation share (csr_filter.hip: remove_edges by an
// edge-id list; csr_remove_nodes.hip: remove_nodes by per-type node rank tables): a removed
// bit per id, the kept count per 32-bit word, the packed rank << 32 | word entries that make
// new_id one 8-B probe, and the ballots over a CSR's slots.  Integer kernels only: the same
// bits whichever file launches them.
#pragma once
#include "common.hpp"

namespace gnnrec {
namespace {

constexpr int kFT = 256;  // threads per block: 4 waves = 4 CSR chunks of 64 slots
constexpr size_t kAlign = 256;
inline size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

inline unsigned flat_grid(int64_t n) {
  int64_t b = (n + kFT - 1) / kFT;
  if (b > 256 * 32) b = 256 * 32;
  return (unsigned)(b < 1 ? 1 : b);
}

// byte offsets of the workspace's parts
struct FilterWs {
  size_t mark;     // uint32 [W]  removed bit per old edge id
  size_t wcnt;     // int32 [W]  kept edges per word
  size_t rank;     // int64 [W + 1]  exclusive scan of wcnt, then packed with mark; rank[W] = E'
  size_t ballot;   // uint64 [C]  kept flags of CSR slots 64 c .. 64 c + 63
  size_t ccnt;     // int32 [C]
  size_t cpre;     // int64 [C + 1]
  size_t scan_ws;  // shared by the two scans (W >= C)
  size_t bytes;
};

inline FilterWs carve(int64_t E) {
  const int64_t W = (E + 31) / 32, C = (E + 63) / 64;
  size_t o = 0;
  FilterWs w;
  w.mark = o; o += align_up((size_t)W * 4);
  w.wcnt = o; o += align_up((size_t)W * 4);
  w.rank = o; o += align_up((size_t)(W + 1) * 8);
  w.ballot = o; o += align_up((size_t)C * 8);
  w.ccnt = o; o += align_up((size_t)C * 4);
  w.cpre = o; o += align_up((size_t)(C + 1) * 8);
  w.scan_ws = o; o += align_up((size_t)gnnrec_scan_workspace_bytes(W > 0 ? W : 1));
  w.bytes = o;
  return w;
}

// the workspace's parts as pointers
struct FilterPtrs {
  uint32_t* mark;
  int32_t* wcnt;
  int64_t* rank;
  uint64_t* ballot;
  int32_t* ccnt;
  int64_t* cpre;
  void* scan_ws;
};

inline FilterPtrs filter_ptrs(void* workspace, const FilterWs& o) {
  char* base = static_cast<char*>(workspace);
  return {reinterpret_cast<uint32_t*>(base + o.mark),   reinterpret_cast<int32_t*>(base + o.wcnt),
          reinterpret_cast<int64_t*>(base + o.rank),    reinterpret_cast<uint64_t*>(base + o.ballot),
          reinterpret_cast<int32_t*>(base + o.ccnt),    reinterpret_cast<int64_t*>(base + o.cpre),
          base + o.scan_ws};
}

__global__ __launch_bounds__(kFT) void mark_removed_kernel(const int64_t* __restrict__ rm,
                                                           int64_t R, int64_t E,
                                                           uint32_t* __restrict__ mark,
                                                           int64_t* __restrict__ status) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t R64 = (R + kWave - 1) / kWave * kWave;  // whole waves reach the shuffles
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < R64; i += stride) {
    int w = -2;  // past the list
    uint32_t v = 0;
    if (i < R) {
      const int64_t e = __builtin_nontemporal_load(rm + i);
      if (e < 0 || e >= E) {
        status[1] = 1;  // benign race: every writer stores 1
        w = -1;
      } else {
        w = (int)(e >> 5);
        v = 1u << (e & 31);
      }
    }
    // v |= the bits of lanes below that hold the same word (any such lane's bits belong in
    // that word, so a coincidence outside the run is harmless); the last lane of every run
    // of equal words then holds the run's bits
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int wo = __shfl_up(w, off);
      const uint32_t vo = __shfl_up(v, off);
      if (lane >= off && wo == w) v |= vo;
    }
    const int wn = __shfl_down(w, 1);
    if (w >= 0 && (lane == kWave - 1 || wn != w)) atomicOr(&mark[w], v);
  }
}

__global__ __launch_bounds__(kFT) void word_count_kernel(const uint32_t* __restrict__ mark,
                                                         int64_t E, int64_t W,
                                                         int32_t* __restrict__ wcnt) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < W; w += stride) {
    const int64_t left = E - w * 32;  // >= 1
    const uint32_t valid = left >= 32 ? 0xffffffffu : ((1u << left) - 1u);
    wcnt[w] = __popc(~mark[w] & valid);
  }
}

// rank[w] (< 2^31) and the word's removed bits in one 8-B entry
__global__ __launch_bounds__(kFT) void pack_rank_kernel(const uint32_t* __restrict__ mark,
                                                        int64_t W, int64_t* __restrict__ rank) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < W; w += stride)
    rank[w] = (rank[w] << 32) | (int64_t)mark[w];
}

// x: the packed entry of e's word
__device__ __forceinline__ int64_t new_eid(int64_t x, int64_t e) {
  return (x >> 32) + __popc(~(uint32_t)x & ((1u << (e & 31)) - 1u));
}

// one wave per 64-slot chunk (blockDim = kFT: whole waves, so every lane reaches the ballot)
__global__ __launch_bounds__(kFT) void csr_flags_kernel(const int64_t* __restrict__ eids,
                                                        int64_t E, int64_t C,
                                                        const uint32_t* __restrict__ mark,
                                                        uint64_t* __restrict__ ballot,
                                                        int32_t* __restrict__ ccnt) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave0 = (int64_t)blockIdx.x * (kFT / kWave) + (threadIdx.x >> 6);
  const int64_t wstride = (int64_t)gridDim.x * (kFT / kWave);
  for (int64_t c = wave0; c < C; c += wstride) {
    const int64_t j = c * kWave + lane;
    bool keep = false;
    if (j < E) {
      const int64_t e = __builtin_nontemporal_load(eids + j);
      // (an id outside [0, E) is no edge of the relation: dropped, never probed)
      keep = e >= 0 && e < E && !((mark[e >> 5] >> (e & 31)) & 1u);
    }
    const uint64_t b = __ballot(keep);
    if (lane == 0) {
      ballot[c] = b;
      ccnt[c] = __popcll(b);
    }
  }
}

inline int hip_ck(hipError_t e, const char* what) {
  if (e == hipSuccess) return GNNREC_OK;
  set_error("%s: %s", what, hipGetErrorString(e));
  return GNNREC_EHIP;
}

}  // namespace
}  // namespace gnnrec
