// k_crc32.hip -- CRC-32 of n variable-length spans of a byte arena (ImmutableDB
// chunk validation: the checksum column of the secondary index, computeCRC in
// System.FS.CRC; parseChunkFile's checkEntries compares it per block).
//
// Spans run from ~800 B to ~90 KB, so one lane per span is out (serial,
// uncoalesced, imbalanced; see the note above arena.hpp's b2b256_staged).  Instead every span
// is cut into tiles of CRC_TILE bytes counted from its start; the host's prefix
// sum of the tile counts (tile_first) maps a workgroup to (span, tile).
//   k_crc32_tiles  one workgroup per tile.  A tile is CRC_ROWS rows of NT * 16
//                  bytes; in each row lane l loads its 16 bytes, so a wave reads
//                  whole consecutive cache lines.  The lane runs its rows
//                  through the raw register (crc32_gf2.hpp), stepping over the
//                  other lanes' bytes with the constant x^(8 * (ROW - 16)), and
//                  is then shifted to the tile's end by the constant
//                  x^(8 * 16 * (NT - 1 - l)); the xor over the workgroup is the
//                  tile's raw(0, .).  The last, shorter tile of a span is
//                  aligned to the span's END: leading zero bytes do not change
//                  raw(0, .), so the bytes in front of the tile are masked to
//                  zero and the same constants serve every tile.
//   k_crc32_merge  one lane per span: Horner over its tiles -- x^(8 * CRC_TILE)
//                  is a constant, the last tile's x^(8 * len) comes from
//                  square-and-multiply over the x^(8 * 2^k) table -- and the
//                  initial value / final xor (crc_finish).
// Every arena byte is read from HBM once; tile results are 4 bytes per 16 KB.
//
// Per-byte step: table-free.  A byte-table walk needs 16-20 LDS look-ups per
// 16 bytes at 64 unrelated indices per wave (bank conflicts serialise them 3-4x)
// and a table fill per workgroup; the shift/xor form is pure VALU with literal
// constants: (s + w) * x^32 as 32 independent (bit ? row : 0) terms, ~3 ops per
// data bit with full ILP, ~26 ops per byte including the row steps.  At 256 CUs
// x 256 lane-ops per clock that is ~6 TB/s of integer rate, the same order as
// the HBM stream, with no LDS traffic beyond the final 4-word reduction (an upper bound by
// instruction count; DESIGN.md section 17 has the measured rate).
#include "kcommon.hpp"
#include "arena.hpp"
#include "crc32_gf2.hpp"

namespace {

constexpr uint32_t CRC_ROW = NT * 16;
constexpr uint32_t CRC_ROWS = 4;
static_assert(CRC_ROW * CRC_ROWS == PRAOS_CRC_TILE, "tile size is part of the ABI (abi.CRC_TILE)");

// x^(8 * 16 * (NT - 1 - l)): lane l's distance to the end of its row
struct LaneShift { uint32_t v[NT]; };
constexpr LaneShift make_lane_shift() {
  LaneShift t{};
  const uint32_t x128 = crc_xpow8(16);
  uint32_t p = CRC_ONE;
  for (int l = NT - 1; l >= 0; l--) { t.v[l] = p; p = crc_mulmod(p, x128); }
  return t;
}
__device__ const LaneShift LANE_SHIFT = make_lane_shift();

// 8 bytes at p (any alignment) of which only those at or after `lo` count; bytes in
// front of lo read as zero and are never loaded (p may lie before the arena).
__device__ __forceinline__ uint64_t ld64_from(const uint8_t* __restrict__ a, int64_t p, int64_t lo) {
  if (p >= lo) return ld64u(a, (uint64_t)p);
  if (p + 8 <= lo) return 0;
  return ld64u(a, (uint64_t)lo) << (8u * (uint32_t)(lo - p));
}

__global__ void __launch_bounds__(NT) k_crc32_tiles(uint32_t n, const uint8_t* __restrict__ arena,
                                                    const uint64_t* __restrict__ off,
                                                    const uint32_t* __restrict__ len,
                                                    const uint32_t* __restrict__ tile_first,
                                                    uint32_t* __restrict__ tile_raw) {
  __shared__ uint32_t s_part[NT / 64];
  const uint32_t tile = blockIdx.x, t = threadIdx.x;
  // span of this tile: the last i with tile_first[i] <= tile (empty spans own no tile)
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (tile_first[mid] <= tile) lo = mid; else hi = mid;
  }
  const uint32_t k = tile - tile_first[lo];
  const uint64_t done = (uint64_t)k * PRAOS_CRC_TILE;
  const uint64_t rest = (uint64_t)len[lo] - done;
  const int64_t start = (int64_t)(off[lo] + done);
  const int64_t end = start + (int64_t)(rest < PRAOS_CRC_TILE ? rest : PRAOS_CRC_TILE);
  const int64_t vstart = end - (int64_t)PRAOS_CRC_TILE;   // < start for a short last tile
  uint64_t w[2 * CRC_ROWS];
#pragma unroll
  for (uint32_t r = 0; r < CRC_ROWS; r++) {
    const int64_t p = vstart + (int64_t)(r * CRC_ROW + 16 * t);
    w[2 * r] = ld64_from(arena, p, start);
    w[2 * r + 1] = ld64_from(arena, p + 8, start);
  }
  constexpr CrcRows ROWSTEP = crc_make_rows(crc_xpow8(CRC_ROW - 16));
  uint32_t s = 0;
#pragma unroll
  for (uint32_t r = 0; r < CRC_ROWS; r++) {
    if (r) s = crc_apply(ROWSTEP, s);
    s = crc_word(s, (uint32_t)w[2 * r]);
    s = crc_word(s, (uint32_t)(w[2 * r] >> 32));
    s = crc_word(s, (uint32_t)w[2 * r + 1]);
    s = crc_word(s, (uint32_t)(w[2 * r + 1] >> 32));
  }
  s = crc_mulmod(s, LANE_SHIFT.v[t]);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s ^= __shfl_xor(s, m);
  if ((t & 63u) == 0) s_part[t >> 6] = s;
  __syncthreads();
  if (t == 0) {
    uint32_t x = 0;
#pragma unroll
    for (uint32_t q = 0; q < NT / 64; q++) x ^= s_part[q];
    tile_raw[tile] = x;
  }
}

__global__ void __launch_bounds__(NT) k_crc32_merge(uint32_t n, const uint32_t* __restrict__ len,
                                                    const uint32_t* __restrict__ tile_first,
                                                    const uint32_t* __restrict__ tile_raw,
                                                    uint32_t* __restrict__ crc) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr CrcRows TILESTEP = crc_make_rows(crc_xpow8(PRAOS_CRC_TILE));
  const uint32_t L = len[i], t0 = tile_first[i], nt = tile_first[i + 1] - t0;
  uint32_t acc = 0;
  for (uint32_t k = 0; k < nt; k++) {
    const uint32_t rest = L - k * PRAOS_CRC_TILE;
    acc = rest >= PRAOS_CRC_TILE ? crc_apply(TILESTEP, acc) : crc_mulmod(acc, crc_xpow8(rest));
    acc ^= tile_raw[t0 + k];
  }
  crc[i] = L ? crc_finish(acc, L) : 0u;
}

}  // namespace

// ---- host launcher: tile_first has n + 1 entries (exclusive prefix sum of the tile counts)
void launch_crc32(hipStream_t stream, uint32_t n, uint32_t ntiles, const uint8_t* arena, const uint64_t* off,
                  const uint32_t* len, const uint32_t* tile_first, uint32_t* tile_raw, uint32_t* crc) {
  if (n == 0) return;
  if (ntiles)
    hipLaunchKernelGGL(k_crc32_tiles, dim3(ntiles), dim3(NT), 0, stream, n, arena, off, len, tile_first, tile_raw);
  hipLaunchKernelGGL(k_crc32_merge, dim3((n + NT - 1) / NT), dim3(NT), 0, stream, n, len, tile_first, tile_raw, crc);
}
