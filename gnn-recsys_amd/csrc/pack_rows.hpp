// Packed rows of a ReLU-sparse [n, 128] fp32 table: 384 B per row instead of 512, lossless.
//
// Row r of a packed table lives at P + 384 * r (16-B aligned), as 96 32-bit words:
//   words 0-3    mask: bit c of the 128-bit mask is set iff the 32-bit pattern of x[r][c] is
//                non-zero (a bit test, not a float compare: -0.0, NaN and denormals are kept)
//   word  4      pre[0..3], one byte each: pre[w] = set bits in the mask words below w
//   word  5      nnz in the low bits, bit 31 the `dense` flag: nnz > 88, the row stores no
//                values and its readers take it from the dense table
//   words 6-7    zero
//   words 8-95   the non-zero values in column order (88 slots), unused slots zero
// Beside the table sit four int32 of status: {packed_ok, dense rows, 2 words the pack
// kernel counts in (zero between launches)}; packed_ok = 1 iff dense rows <= the limit the
// pack was given.  The gathers read a table with packed_ok = 0 through their dense loop.
//
// pack_row_host / unpack_row_host restate the format on the host (tests, C ABI).
#pragma once
#include <cstdint>
#include <cstring>

namespace gnnrec {

constexpr int kPackD = 128;           // columns of a packable table
constexpr int kPackWords = 96;        // 32-bit words per packed row (384 B)
constexpr int kPackHdrWords = 8;      // mask[4], pre, nnz | flag, 2 x zero
constexpr int kPackSlots = kPackWords - kPackHdrWords;  // 88 values
constexpr uint32_t kPackDenseBit = 0x80000000u;
constexpr int kPackStatusWords = 4;   // packed_ok, dense rows, counter, exit counter
// share of `dense` rows up to which a table counts as packed (packed_ok = 1) when the
// caller names none.  A dense row costs its 384 packed bytes and then a dependent 512-B
// read of the dense row.  Measured (tools/probe_packed_gather.py, 500M edges from a 1M-row
// table, dense gather = 1): 0.76 with no such row, 0.78 at 1/64, 0.83 at 1/16, 1.01 at 1/4,
// 1.86 at 1 — linear, crossing the dense gather at 0.23.  Half of that keeps a tenth of
// the dense gather's time as the gain at the limit, above the pack's own cost.
constexpr double kPackMaxDenseFrac = 1.0 / 8;

inline void pack_row_host(const float* x, uint32_t* p) {
  uint32_t bits[kPackD];
  std::memcpy(bits, x, sizeof(bits));
  for (int i = 0; i < kPackWords; ++i) p[i] = 0;
  uint32_t nnz = 0, pre = 0;
  for (int w = 0; w < 4; ++w) {
    pre |= nnz << (8 * w);  // nnz below word 3 is at most 96: fits a byte
    for (int b = 0; b < 32; ++b)
      if (bits[32 * w + b] != 0) {
        p[w] |= 1u << b;
        ++nnz;
      }
  }
  p[4] = pre;
  p[5] = nnz | (nnz > (uint32_t)kPackSlots ? kPackDenseBit : 0u);
  if (nnz > (uint32_t)kPackSlots) return;
  int q = 0;
  for (int c = 0; c < kPackD; ++c)
    if (bits[c] != 0) p[kPackHdrWords + q++] = bits[c];
}

// x = the row p packs; a `dense` row is copied from dense_row (its row of the dense table)
inline void unpack_row_host(const uint32_t* p, const float* dense_row, float* x) {
  if (p[5] & kPackDenseBit) {
    std::memcpy(x, dense_row, kPackD * sizeof(float));
    return;
  }
  uint32_t bits[kPackD];
  int q = 0;
  for (int c = 0; c < kPackD; ++c)
    bits[c] = (p[c >> 5] >> (c & 31)) & 1u ? p[kPackHdrWords + q++] : 0u;
  std::memcpy(x, bits, sizeof(bits));
}

}  // namespace gnnrec
