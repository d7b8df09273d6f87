// wire_scan.hpp -- the node-to-node wrapper of a header, as the ChainSync client receives it.
//
//   Shelley-based eras   [eraIndex, #6.24(bytes)]
//       (decodeNS, HardFork/Combinator/Serialisation/Common.hs:451-463: listLen 2, Word8 index;
//        Shelley/Node/Serialisation.hs:110-112: the header wrapped in CBOR-in-CBOR)
//   Byron (era 0)        [0, [[kind, sizeHint], #6.24(bytes)]]
//       (Byron/Node/Serialisation.hs:83-99, ByronNodeToNodeVersion2: kind 0 = EBB, 1 = main header)
//
// wire_unwrap finds the inner header bytes and does nothing else: what the bytes hold is the
// decoders' business (k_decode_praos, k_pbft_decode).  Heads of any width are taken (cborg's
// decodeListLen / decodeWord8 / decodeTag accept non-shortest forms); lists and the byte string
// must be definite; the tag must be 24.  Plain integers only: k_wire.hip includes the file for
// the device and g++ compiles it for the host tests (tests/test_wire_host.py).
// gen_tx_unwrap, below it, is the same for a transaction (k_gentx.hip, tests/test_gentx_host.py),
// wire_block_unwrap for a block (k_blockfetch.hip, tests/test_blockfetch_host.py).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define WIRE_HD __host__ __device__ __forceinline__
#else
#define WIRE_HD inline
#endif

namespace wire_scan {

// praos_hip.h PRAOS_WIRE_*
constexpr uint8_t OK = 0, RANGE = 1, SYNTAX = 2, ERA = 3, TRAILING = 4;
constexpr uint8_t NOT_BYRON = 0xff;

struct Item {
  uint8_t status;
  uint8_t era;          // the wire index (0xff until it is read)
  uint8_t byron_kind;   // 0 EBB, 1 main header, 0xff outside Byron
  uint32_t size_hint;   // Byron only
  uint64_t off;         // inner bytes a[off, off + len)
  uint32_t len;
};

struct Cur {
  const uint8_t* a;
  uint64_t p, end;
};

// one head of major type `want`, any width; false: truncated, another type, indefinite or reserved
WIRE_HD bool head(Cur& c, uint32_t want, uint64_t& arg) {
  if (c.p >= c.end) return false;
  const uint32_t ib = c.a[c.p++];
  if ((ib >> 5) != want) return false;
  const uint32_t ai = ib & 31u;
  if (ai < 24) { arg = ai; return true; }
  if (ai > 27) return false;
  const uint32_t nb = 1u << (ai - 24);
  if (nb > c.end - c.p) return false;
  uint64_t v = 0;
  for (uint32_t k = 0; k < nb; k++) v = (v << 8) | c.a[c.p + k];
  c.p += nb;
  arg = v;
  return true;
}

// the wire item a[pos, pos + len) of an arena of arena_len bytes; n_eras = eras of the block type
WIRE_HD Item wire_unwrap(const uint8_t* a, uint64_t arena_len, uint64_t pos, uint64_t len, uint32_t n_eras) {
  Item r{SYNTAX, 0xff, NOT_BYRON, 0u, 0ull, 0u};
  if (pos > arena_len || len > arena_len - pos) { r.status = RANGE; return r; }
  Cur c{a, pos, pos + len};
  uint64_t v;
  if (!head(c, 4, v) || v != 2) return r;
  if (!head(c, 0, v) || v > 0xff) return r;           // decodeWord8
  r.era = (uint8_t)v;
  if (v >= n_eras) { r.status = ERA; return r; }
  if (v == 0) {
    uint64_t kind, hint;
    if (!head(c, 4, v) || v != 2) return r;
    if (!head(c, 4, v) || v != 2) return r;
    if (!head(c, 0, kind) || kind > 1) return r;
    if (!head(c, 0, hint) || hint > 0xffffffffull) return r;
    r.byron_kind = (uint8_t)kind;
    r.size_hint = (uint32_t)hint;
  }
  if (!head(c, 6, v) || v != 24) return r;
  if (!head(c, 2, v) || v > c.end - c.p) return r;
  r.off = c.p;
  r.len = (uint32_t)v;
  r.status = c.p + v == c.end ? OK : TRAILING;
  return r;
}

// praos_hip.h PRAOS_GTX_BYRON
constexpr uint8_t GTX_BYRON = 6;

// The node-to-node wrapper of a transaction (GenTx), as the TxSubmission server receives it.
//   Shelley-based eras   [eraIndex, #6.24(bytes)]   (decodeNS; Shelley/Ledger/Mempool.hs:186-193)
//   Byron (era 0)        [0, [kind, payload]]       (Byron/Ledger/Mempool.hs encodeByronGenTx:
//                        kind 0 tx, 1 delegation certificate, 2 update proposal, 3 update vote)
// The same rules as wire_unwrap for the heads.  A Byron item is GTX_BYRON with byron_kind set and
// (off, len) its payload: every byte after the kind up to the end of the item, at least one (what
// they hold is not looked at); any other era-0 form is SYNTAX.  size_hint stays 0.
WIRE_HD Item gen_tx_unwrap(const uint8_t* a, uint64_t arena_len, uint64_t pos, uint64_t len, uint32_t n_eras) {
  Item r{SYNTAX, 0xff, NOT_BYRON, 0u, 0ull, 0u};
  if (pos > arena_len || len > arena_len - pos) { r.status = RANGE; return r; }
  Cur c{a, pos, pos + len};
  uint64_t v;
  if (!head(c, 4, v) || v != 2) return r;
  if (!head(c, 0, v) || v > 0xff) return r;           // decodeWord8
  r.era = (uint8_t)v;
  if (v >= n_eras) { r.status = ERA; return r; }
  if (v == 0) {
    uint64_t kind;
    if (!head(c, 4, v) || v != 2) return r;
    if (!head(c, 0, kind) || kind > 3) return r;
    if (c.p >= c.end || c.end - c.p > 0xffffffffull) return r;
    r.byron_kind = (uint8_t)kind;
    r.off = c.p;
    r.len = (uint32_t)(c.end - c.p);
    r.status = GTX_BYRON;
    return r;
  }
  if (!head(c, 6, v) || v != 24) return r;
  if (!head(c, 2, v) || v > c.end - c.p) return r;
  r.off = c.p;
  r.len = (uint32_t)v;
  r.status = c.p + v == c.end ? OK : TRAILING;
  return r;
}

// The node-to-node wrapper of a block, as the BlockFetch client receives it: #6.24(bytes) around
// the stored block [diskTag, ...] (wrapCBORinCBOR (encodeDiskHfcBlock ccfg),
// HardFork/Combinator/Serialisation/SerialiseNodeToNode.hs:113) -- no era list around it.  The
// same rules as wire_unwrap for the tag and the byte string.  Bytes after the byte string are
// TRAILING, whatever it holds.  The inner bytes must start with a definite array head of length 2
// and an unsigned integer, both of any width (SYNTAX otherwise): the disk tag, 0 an EBB, 1 a Byron
// main block, 2.. the Shelley-based eras; a tag above n_eras (7 for the reference's CardanoBlock)
// is ERA.  era = the disk tag (0xff until it is read; a tag above 0xfe reads 0xfe), (off, len) the
// inner bytes of an OK or ERA item (0, 0 otherwise).  byron_kind and size_hint are not used.
WIRE_HD Item wire_block_unwrap(const uint8_t* a, uint64_t arena_len, uint64_t pos, uint64_t len, uint32_t n_eras) {
  Item r{SYNTAX, 0xff, NOT_BYRON, 0u, 0ull, 0u};
  if (pos > arena_len || len > arena_len - pos) { r.status = RANGE; return r; }
  Cur c{a, pos, pos + len};
  uint64_t v;
  if (!head(c, 6, v) || v != 24) return r;
  if (!head(c, 2, v) || v > c.end - c.p || v > 0xffffffffull) return r;
  if (c.p + v != c.end) { r.status = TRAILING; return r; }
  const uint64_t at = c.p;
  uint64_t tag;
  if (!head(c, 4, v) || v != 2 || !head(c, 0, tag)) return r;
  r.off = at;
  r.len = (uint32_t)(c.end - at);
  r.era = tag > 0xfe ? (uint8_t)0xfe : (uint8_t)tag;
  r.status = tag > n_eras ? ERA : OK;
  return r;
}

}  // namespace wire_scan
