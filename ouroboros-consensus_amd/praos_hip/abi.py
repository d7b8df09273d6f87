"""ctypes binding of libpraos_hip.so (include/praos_hip.h).

This is plumbing for tests and bench.py; the product is the C ABI itself.  The
library is the gfx950 HIP build; there is deliberately no CPU fallback: every
call here goes to the GPU, and a missing library raises.
"""
import ctypes
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_PKG), "libpraos_hip.so")
# A/B experiments only: load an alternative in-tree build (same ABI)
LIB_PATH = os.environ.get("PRAOS_HIP_LIB", LIB_PATH)
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_PKG)), "include", "praos_hip.h")

u8p = ctypes.POINTER(ctypes.c_uint8)
u16p = ctypes.POINTER(ctypes.c_uint16)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)
i32p = ctypes.POINTER(ctypes.c_int32)

# bits (PRAOS_BIT_*)
BLK_DECODE = 0x01      # block-integrity result bits (praos_verify_block_integrity)
BLK_KES = 0x02
BLK_BODY_HASH = 0x04
BIT_KES_BEFORE_START = 0x0001
BIT_KES_AFTER_END = 0x0002
BIT_OCERT_SIG = 0x0004
BIT_KES_MERKLE = 0x0008
BIT_KES_LEAF = 0x0010
BIT_COUNTER_MISSING = 0x0020
BIT_COUNTER_TOO_SMALL = 0x0040
BIT_COUNTER_OVER_INC = 0x0080
BIT_VRF_KEY_UNKNOWN = 0x0100
BIT_VRF_KEY_WRONG = 0x0200
BIT_VRF_PROOF = 0x0400
BIT_VRF_OUTPUT = 0x0800
BIT_LEADER = 0x1000
BIT_INPUT = 0x8000
HOST_ONLY = -1
BIT_TP_VRF_NONCE = 0x0400
BIT_TP_VRF_LEADER = 0x0800
# praos_synth_params.corrupt_fields
CORRUPT_OCERT, CORRUPT_KES_SIG, CORRUPT_VRF_PROOF, CORRUPT_VRF_OUT, CORRUPT_BODY = 0x01, 0x02, 0x04, 0x08, 0x10

# verdicts (enum praos_verdict)
V_OK, V_KES_BEFORE_START, V_KES_AFTER_END, V_OCERT_SIG, V_KES_SIG, V_COUNTER_MISSING, \
    V_COUNTER_TOO_SMALL, V_COUNTER_OVER_INC, V_VRF_KEY_UNKNOWN, V_VRF_KEY_WRONG, V_VRF_BAD_PROOF, \
    V_LEADER_TOO_BIG, V_INPUT, V_ENV_BLOCK_NO, V_ENV_SLOT_NO, V_ENV_PREV_HASH, V_ENV_OBSOLETE_NODE, \
    V_ENV_HEADER_SIZE, V_ENV_BLOCK_SIZE = range(19)
V_TPRAOS = 19
V_DOESNT_FIT, V_NOT_REACHED = 25, 255      # praos_validate_candidates (praos_hip.wire)
# TPraos PRTCL predicate failures (PRAOS_TPF_*)
TPF_KES_BEFORE_START, TPF_KES_AFTER_END, TPF_OCERT_SIG, TPF_KES_SIG, TPF_COUNTER_MISSING, \
    TPF_COUNTER_TOO_SMALL, TPF_COUNTER_OVER_INC = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40
TPF_VRF_KEY_UNKNOWN, TPF_VRF_KEY_WRONG, TPF_BAD_NONCE, TPF_BAD_LEADER, TPF_LEADER_TOO_BIG, TPF_NOT_ACTIVE, \
    TPF_GEN_COLD, TPF_GEN_VRF = 0x100, 0x200, 0x400, 0x800, 0x1000, 0x2000, 0x4000, 0x8000


class Params(ctypes.Structure):
    _fields_ = [("slots_per_kes_period", ctypes.c_uint64), ("max_kes_evo", ctypes.c_uint64),
                ("f_is_one", ctypes.c_int32), ("vrf_check_output", ctypes.c_int32),
                ("c_raw", ctypes.c_uint8 * 16)]


class Pool(ctypes.Structure):
    _fields_ = [("hash28", ctypes.c_uint8 * 28), ("vrf_hash32", ctypes.c_uint8 * 32),
                ("sigma_fp", ctypes.c_uint8 * 16)]


class Headers(ctypes.Structure):
    _fields_ = [("n", ctypes.c_size_t), ("slot", u64p), ("cold_vk", u8p), ("vrf_vk", u8p), ("vrf_out", u8p),
                ("vrf_proof", u8p), ("hot_vk", u8p), ("ocert_n", u64p), ("ocert_c0", u64p), ("ocert_sig", u8p),
                ("kes_sig", u8p), ("body_off", u64p), ("body_len", u32p), ("body_bytes", u8p),
                ("body_bytes_len", ctypes.c_size_t)]


class Out(ctypes.Structure):
    _fields_ = [("bits", u16p), ("pool_idx", i32p), ("beta", u8p), ("leader", u8p), ("nonce", u8p)]


class TPHeaders(ctypes.Structure):
    _fields_ = [("h", Headers), ("leader_out", u8p), ("leader_proof", u8p)]


class TPOut(ctypes.Structure):
    _fields_ = [("bits", u16p), ("pool_idx", i32p), ("beta_eta", u8p), ("beta_leader", u8p), ("nonce", u8p)]


class GenDeleg(ctypes.Structure):
    _fields_ = [("genesis_hash28", ctypes.c_uint8 * 28), ("delegate_hash28", ctypes.c_uint8 * 28),
                ("vrf_hash32", ctypes.c_uint8 * 32)]


class Overlay(ctypes.Structure):
    _fields_ = [("d_num", ctypes.c_uint64), ("d_den", ctypes.c_uint64), ("asc_num", ctypes.c_uint64),
                ("asc_den", ctypes.c_uint64), ("epoch_base_slot", ctypes.c_uint64), ("epoch_length", ctypes.c_uint64),
                ("gen_delegs", ctypes.POINTER(GenDeleg)), ("n_gen_delegs", ctypes.c_uint32)]


class Nonce(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint8 * 32), ("neutral", ctypes.c_int32)]


class ChainState(ctypes.Structure):
    _fields_ = [("last_slot_origin", ctypes.c_int32), ("last_slot", ctypes.c_uint64),
                ("counter_hash28", u8p), ("counter", u64p), ("m", ctypes.c_size_t), ("cap", ctypes.c_size_t),
                ("evolving", Nonce), ("candidate", Nonce), ("epoch_nonce", Nonce), ("lab", Nonce),
                ("last_epoch_block", Nonce)]


class EpochInfo(ctypes.Structure):
    _fields_ = [("epoch_base_slot", ctypes.c_uint64), ("epoch_base_no", ctypes.c_uint64),
                ("epoch_length", ctypes.c_uint64), ("stability_window", ctypes.c_uint64)]


class Envelope(ctypes.Structure):
    _fields_ = [("block_no", u64p), ("header_hash", u8p), ("header_size", u32p), ("body_size", u32p),
                ("tip_is_origin", ctypes.c_int32), ("tip_slot", ctypes.c_uint64), ("tip_block_no", ctypes.c_uint64),
                ("tip_hash", ctypes.c_uint8 * 32), ("max_major_pv", ctypes.c_uint64),
                ("lv_prot_major", ctypes.c_uint64), ("max_header_size", ctypes.c_uint64),
                ("max_body_size", ctypes.c_uint64)]


class ReplayStats(ctypes.Structure):
    _fields_ = [("skipped", ctypes.c_uint64), ("headers", ctypes.c_uint64), ("validated", ctypes.c_uint64), ("stop_index", ctypes.c_uint64),
                ("stop_verdict", ctypes.c_uint32), ("epochs", ctypes.c_uint32), ("batches", ctypes.c_uint32),
                ("chunks", ctypes.c_uint32), ("ms_io", ctypes.c_double), ("ms_device", ctypes.c_double),
                ("ms_fold", ctypes.c_double), ("ms_nonce", ctypes.c_double)]


class LedgerView(ctypes.Structure):
    _fields_ = [("first_epoch", ctypes.c_uint64), ("pools", ctypes.c_void_p), ("npools", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("lv_prot_major", ctypes.c_uint64),
                ("max_header_size", ctypes.c_uint64), ("max_body_size", ctypes.c_uint64)]


class Counters(ctypes.Structure):
    _fields_ = [("hash28", u8p), ("counter", u64p), ("m", ctypes.c_size_t)]


class SynthParams(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint64), ("npools", ctypes.c_uint32), ("first_slot", ctypes.c_uint64),
                ("slot_stride", ctypes.c_uint64), ("body_len", ctypes.c_uint32),
                ("corrupt_per_10000", ctypes.c_uint32), ("nkes", ctypes.c_uint32), ("seed", ctypes.c_uint8 * 32),
                ("body_hash", u8p), ("sched_slot", u64p), ("sched_pool", u32p), ("block_no0", ctypes.c_uint64),
                ("link_prev", ctypes.c_int32), ("prev0", u8p), ("header_hash", u8p),
                ("corrupt_fields", ctypes.c_uint32)]


class HeaderBytes(ctypes.Structure):
    _fields_ = [("n", ctypes.c_size_t), ("bytes", u8p), ("bytes_len", ctypes.c_size_t), ("off", u64p),
                ("len", u32p)]


DECODED_FIELDS = (  # name, dtype, record shape (praos_decoded, include/praos_hip.h)
    ("status", np.uint16, ()), ("block_no", np.uint64, ()), ("slot", np.uint64, ()), ("prev_hash", np.uint8, (32,)),
    ("prev_is_genesis", np.uint8, ()), ("cold_vk", np.uint8, (32,)), ("vrf_vk", np.uint8, (32,)),
    ("vrf_out", np.uint8, (64,)), ("vrf_proof", np.uint8, (80,)), ("body_size", np.uint32, ()),
    ("body_hash", np.uint8, (32,)), ("hot_vk", np.uint8, (32,)), ("ocert_n", np.uint64, ()),
    ("ocert_c0", np.uint64, ()), ("ocert_sig", np.uint8, (64,)), ("prot_major", np.uint64, ()),
    ("prot_minor", np.uint64, ()), ("kes_sig", np.uint8, (448,)), ("signed_len", np.uint32, ()),
    ("signed_body", np.uint8, (448,)), ("header_hash", np.uint8, (32,)))
_CT = {np.uint8: u8p, np.uint16: u16p, np.uint32: u32p, np.uint64: u64p}


class Decoded(ctypes.Structure):
    _fields_ = [(name, _CT[dt]) for name, dt, _ in DECODED_FIELDS]


# ImmutableDB chunk validation (praos_crc32 / praos_validate_chunk)
CRC_TILE = (16384,)     # PRAOS_CRC_TILE: the tile size(s) of k_crc32.hip, counted from a span's start
CHUNK_OK, CHUNK_ERR_READ, CHUNK_ERR_CORRUPT, CHUNK_ERR_HASH_MISMATCH, CHUNK_UNSUPPORTED = 0, 1, 2, 3, 4
CHUNK_OUTCOMES = ("OK", "ERR_READ", "ERR_CORRUPT", "ERR_HASH_MISMATCH", "UNSUPPORTED")
CHUNK_ENTRY_SIZE = 56
E_ARG = -2


class Chunk(ctypes.Structure):
    _fields_ = [("bytes", u8p), ("bytes_len", ctypes.c_size_t), ("expected_crc", u32p),
                ("n_expected", ctypes.c_size_t), ("block_off", u64p)]


class ChunkResult(ctypes.Structure):
    _fields_ = [("outcome", ctypes.c_uint32), ("integrity_bits", ctypes.c_uint32), ("blocks", ctypes.c_uint64),
                ("checked", ctypes.c_uint64), ("truncate_at", ctypes.c_uint64), ("rescanned_from", ctypes.c_uint64),
                ("err_slot", ctypes.c_uint64), ("err_hash", ctypes.c_uint8 * 32),
                ("expected_prev", ctypes.c_uint8 * 32), ("actual_prev", ctypes.c_uint8 * 32),
                ("actual_prev_is_genesis", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 7)]


class ChunkOut(ctypes.Structure):
    _fields_ = [("cap", ctypes.c_size_t), ("entries", u8p), ("block_no", u64p), ("prev_hash", u8p),
                ("prev_is_genesis", u8p), ("integrity", ctypes.POINTER(ctypes.c_int8))]


class ChunkCfg(ctypes.Structure):
    _fields_ = [("slots_per_kes_period", ctypes.c_uint64), ("byron_epoch_slots", ctypes.c_uint64),
                ("byron_protocol_magic", ctypes.c_uint32), ("pad_", ctypes.c_uint32)]


# Transaction index of stored blocks (praos_index_block_txs / praos_block_batch_tx_index)
TXI_OK, TXI_DECODE, TXI_SHAPE = 0, 1, 2
TXI_STATS_FIELDS = (  # name, dtype (praos_txi_stats; tx_first has n + 1 entries)
    ("status", np.uint8), ("n_tx", np.uint32), ("txs_size", np.uint64), ("n_out", np.uint64),
    ("ex_steps", np.uint64), ("tx_first", np.uint64))
TXI_ROW_FIELDS = (  # name, dtype, record shape (praos_txi_rows)
    ("block", np.uint32, ()), ("body_off", np.uint64, ()), ("body_len", np.uint32, ()), ("wit_off", np.uint64, ()),
    ("wit_len", np.uint32, ()), ("aux_off", np.uint64, ()), ("aux_len", np.uint32, ()), ("size", np.uint32, ()),
    ("n_out", np.uint32, ()), ("ex_steps", np.uint64, ()), ("is_valid", np.uint8, ()), ("tx_id", np.uint8, (32,)))


class TxiCfg(ctypes.Structure):
    _fields_ = [("byron", ctypes.c_uint32), ("pad_", ctypes.c_uint32)]


class TxiStats(ctypes.Structure):
    _fields_ = [(name, _CT[dt]) for name, dt in TXI_STATS_FIELDS]


class TxiRows(ctypes.Structure):
    _fields_ = [("cap", ctypes.c_size_t), ("n_rows", ctypes.c_size_t)] + [(name, _CT[dt])
                                                                          for name, dt, _ in TXI_ROW_FIELDS]


# Key witnesses of stored blocks' transactions (praos_verify_tx_witnesses / praos_block_batch_tx_witnesses)
TXW_OK, TXW_SHAPE, TXW_SKIPPED = 0, 1, 2
TXW_BLOCK_FIELDS = (  # name, dtype (praos_txw_blocks; tx_first has n + 1 entries)
    ("status", np.uint8), ("n_tx", np.uint32), ("n_wit", np.uint32), ("n_bad", np.uint32), ("n_shape", np.uint32),
    ("tx_first", np.uint64))
TXW_TX_FIELDS = (  # name, dtype, record shape (praos_txw_txs; wit_first has cap + 1 entries)
    ("block", np.uint32, ()), ("status", np.uint8, ()), ("n_vkey", np.uint32, ()), ("n_boot", np.uint32, ()),
    ("n_bad", np.uint32, ()), ("tx_id", np.uint8, (32,)), ("wit_first", np.uint64, ()))
TXW_WIT_FIELDS = (  # name, dtype, record shape (praos_txw_wits)
    ("tx", np.uint32, ()), ("kind", np.uint8, ()), ("key_off", np.uint64, ()), ("sig_off", np.uint64, ()),
    ("ok", np.uint8, ()), ("key_hash", np.uint8, (28,)))


class TxwCfg(ctypes.Structure):
    _fields_ = [("byron", ctypes.c_uint32), ("max_lanes", ctypes.c_uint32)]


class TxwBlocks(ctypes.Structure):
    _fields_ = [(name, _CT[dt]) for name, dt in TXW_BLOCK_FIELDS]


class TxwTxs(ctypes.Structure):
    _fields_ = [("cap", ctypes.c_size_t), ("n_rows", ctypes.c_size_t)] + [(name, _CT[dt])
                                                                          for name, dt, _ in TXW_TX_FIELDS]


class TxwWits(ctypes.Structure):
    _fields_ = [("cap", ctypes.c_size_t), ("n_wits", ctypes.c_size_t)] + [(name, _CT[dt])
                                                                          for name, dt, _ in TXW_WIT_FIELDS]


# TxSubmission transactions: wire GenTxs, each checked once (praos_verify_gen_txs)
GTX_SHAPE, GTX_BYRON, GTX_PER_TX_OVERHEAD, GTX_NO_ROW = 5, 6, 4, 0xFFFFFFFF
GTX_ITEM_FIELDS = (  # name, dtype (praos_gtx_items)
    ("status", np.uint8), ("era", np.uint8), ("row", np.uint32), ("byron_kind", np.uint8),
    ("payload_off", np.uint64), ("payload_len", np.uint32))
GTX_TX_FIELDS = (  # name, dtype, record shape (praos_gtx_txs; wit_first has cap + 1 entries)
    ("item", np.uint32, ()), ("era", np.uint8, ()), ("body_off", np.uint64, ()), ("body_len", np.uint32, ()),
    ("wit_off", np.uint64, ()), ("wit_len", np.uint32, ()), ("aux_off", np.uint64, ()), ("aux_len", np.uint32, ()),
    ("size", np.uint32, ()), ("in_block_size", np.uint32, ()), ("ex_mem", np.uint64, ()), ("ex_steps", np.uint64, ()),
    ("is_valid", np.uint8, ()), ("tx_id", np.uint8, (32,)), ("wstatus", np.uint8, ()), ("n_vkey", np.uint32, ()),
    ("n_boot", np.uint32, ()), ("n_bad", np.uint32, ()), ("wit_first", np.uint64, ()))


class GtxCfg(ctypes.Structure):
    _fields_ = [("n_eras", ctypes.c_uint32), ("dedup", ctypes.c_uint32), ("max_lanes", ctypes.c_uint32),
                ("pad_", ctypes.c_uint32)]


class GtxItems(ctypes.Structure):
    _fields_ = [(name, _CT[dt]) for name, dt in GTX_ITEM_FIELDS]


class GtxTxs(ctypes.Structure):
    _fields_ = [("cap", ctypes.c_size_t), ("n_rows", ctypes.c_size_t)] + [(name, _CT[dt])
                                                                          for name, dt, _ in GTX_TX_FIELDS]


# BlockFetch blocks: wire blocks, each checked once (praos_verify_fetched_blocks)
(BF_OK, BF_WIRE, BF_DECODE, BF_WRONG_BLOCK, BF_INVALID_BODY, BF_TOO_MANY, BF_UNSUPPORTED,
 BF_NOT_REACHED) = 0, 1, 2, 3, 4, 5, 6, 255
BF_RANGE_COMPLETE, BF_RANGE_FAILED, BF_RANGE_TOO_FEW, BF_NO_ROW = 0, 1, 2, 0xFFFFFFFF
SPAN_EQ_VEC, SPAN_EQ_WAVE, SPAN_EQ_TILE = 16, 1024, 4096   # praos_debug_span_equal's geometry
BF_ITEM_FIELDS = (("status", np.uint8), ("tag", np.uint8), ("verdict", np.uint8), ("row", np.uint32))   # praos_bf_items
BF_RANGE_FIELDS = (("stop", np.uint64), ("accepted", np.uint64), ("status", np.uint8))   # praos_bf_range_out
BF_ROW_FIELDS = (  # name, dtype, record shape (praos_bf_rows)
    ("item", np.uint32, ()), ("tag", np.uint8, ()), ("is_ebb", np.uint8, ()), ("slot", np.uint64, ()),
    ("block_no", np.uint64, ()), ("header_hash", np.uint8, (32,)), ("prev_hash", np.uint8, (32,)),
    ("hdr_off", np.uint64, ()), ("hdr_len", np.uint32, ()), ("blk_off", np.uint64, ()), ("blk_len", np.uint32, ()),
    ("body_hash", np.uint8, (32,)), ("bits", np.uint8, ()), ("which", np.uint8, ()))


class BfRanges(ctypes.Structure):
    _fields_ = [("k", ctypes.c_size_t), ("item_first", u64p), ("exp_first", u64p), ("exp_slot", u64p),
                ("exp_hash", u8p)]


class BfCfg(ctypes.Structure):
    _fields_ = [("n_eras", ctypes.c_uint32), ("dedup", ctypes.c_uint32), ("witnesses", ctypes.c_uint32),
                ("max_lanes", ctypes.c_uint32), ("byron_epoch_slots", ctypes.c_uint64)]


class BfItems(ctypes.Structure):
    _fields_ = [(name, _CT[dt]) for name, dt in BF_ITEM_FIELDS]


class BfRangeOut(ctypes.Structure):
    _fields_ = [(name, _CT[dt]) for name, dt in BF_RANGE_FIELDS]


class BfRows(ctypes.Structure):
    _fields_ = [("cap", ctypes.c_size_t), ("n_rows", ctypes.c_size_t)] + [(name, _CT[dt])
                                                                          for name, dt, _ in BF_ROW_FIELDS]


# Byron blocks: further PRAOS_BLK_* bits and the failing body comparisons (PRAOS_BYRON_W_*)
BLK_PBFT_SIG, BLK_PM = 0x08, 0x10
BYRON_W_DLG, BYRON_W_UPD, BYRON_W_NTX, BYRON_W_WIT, BYRON_W_ROOT = 0x01, 0x02, 0x04, 0x08, 0x10

# Byron header validation: PBFT (praos_verify_pbft_headers / praos_pbft_update_chain_dep_state)
PBFT_BIT_DECODE, PBFT_BIT_SIG, PBFT_BIT_NOT_DELEGATE = 0x01, 0x02, 0x04
V_OK, V_INPUT, V_ENV_BLOCK_NO, V_ENV_SLOT_NO, V_ENV_PREV_HASH = 0, 12, 13, 14, 15
V_PBFT_INVALID_SIG, V_PBFT_INVALID_SLOT, V_PBFT_NOT_DELEGATE, V_PBFT_EXCEEDED, V_ENV_EBB_IN_SLOT = 20, 21, 22, 23, 24


class PbftParams(ctypes.Structure):
    _fields_ = [("window_size", ctypes.c_uint64), ("threshold", ctypes.c_uint64), ("epoch_slots", ctypes.c_uint64),
                ("protocol_magic", ctypes.c_uint32), ("pad_", ctypes.c_uint32)]


class PbftOut(ctypes.Structure):
    _fields_ = [("bits", u8p), ("gk_idx", i32p), ("slot", u64p), ("block_no", u64p), ("prev_hash", u8p),
                ("prev_is_genesis", u8p), ("header_hash", u8p), ("delegate_hash", u8p)]


class PbftTip(ctypes.Structure):
    _fields_ = [("origin", ctypes.c_uint8), ("is_ebb", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 6),
                ("slot", ctypes.c_uint64), ("block_no", ctypes.c_uint64), ("hash", ctypes.c_uint8 * 32)]


class PbftStateC(ctypes.Structure):
    _fields_ = [("cap", ctypes.c_uint64), ("n", ctypes.c_uint64), ("slot", u64p), ("genesis_hash", u8p)]


PBFT_OUT_FIELDS = (("bits", np.uint8, ()), ("gk_idx", np.int32, ()), ("slot", np.uint64, ()),
                   ("block_no", np.uint64, ()), ("prev_hash", np.uint8, (32,)), ("prev_is_genesis", np.uint8, ()),
                   ("header_hash", np.uint8, (32,)), ("delegate_hash", np.uint8, (28,)))


# decode status (PRAOS_DEC_*)
DEC_RANGE, DEC_SYNTAX, DEC_SIZE, DEC_UNSUPPORTED, DEC_TRAILING, DEC_NONCANONICAL, DEC_OVERFLOW = \
    0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40
DEC_FAILED = 0x5F
SIGNED_STRIDE = 448
TP_SIGNED_STRIDE = 640

# every entry point declared in include/praos_hip.h: name -> (restype, argtypes)
SIGNATURES = {
    "praos_abi_version": (ctypes.c_int, []),
    "praos_host_register": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    "praos_host_unregister": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "praos_open": (ctypes.c_void_p, [ctypes.c_int]),
    "praos_close": (None, [ctypes.c_void_p]),
    "praos_last_error": (ctypes.c_char_p, [ctypes.c_void_p]),
    "praos_set_epoch": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.POINTER(Pool), ctypes.c_uint32,
                                       ctypes.POINTER(Params)]),
    "praos_verify_headers": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Headers), ctypes.POINTER(Out)]),
    "praos_batch_upload": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.POINTER(Headers)]),
    "praos_batch_run": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "praos_batch_sync": (ctypes.c_int, [ctypes.c_void_p]),
    "praos_batch_download": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Out)]),
    "praos_batch_free": (None, [ctypes.c_void_p, ctypes.c_void_p]),
    "praos_batch_kernel_ms": (ctypes.c_float, [ctypes.c_void_p, ctypes.c_int]),
    "praos_set_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "praos_batch_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, u32p]),
    "praos_batch_wide_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, u32p]),
    "praos_set_vrf_wide": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "praos_batch_dedup_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, u32p]),
    "praos_verify_ocert": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, u8p, u8p, u64p, u64p, u8p, u8p]),
    "praos_verify_kes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, u8p, u32p, u8p, u64p, u32p, u8p,
                                        ctypes.c_size_t, u8p]),
    "praos_verify_vrf": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, u8p, u8p, u8p, u8p, u8p]),
    "praos_check_leader": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, u8p, u8p, ctypes.POINTER(Params), u8p]),
    "praos_apply_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Headers), ctypes.POINTER(Out),
                                         ctypes.POINTER(Counters), u8p, ctypes.POINTER(ctypes.c_size_t)]),
    "praos_update_chain_dep_state": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Headers), u8p, u8p,
                                                    ctypes.POINTER(Out), ctypes.POINTER(EpochInfo),
                                                    ctypes.POINTER(ChainState), u8p, ctypes.POINTER(ctypes.c_size_t),
                                                    ctypes.POINTER(ctypes.c_size_t)]),
    "praos_validate_headers": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Headers), u8p, u8p, ctypes.POINTER(Out),
                                              ctypes.POINTER(Envelope), ctypes.POINTER(EpochInfo),
                                              ctypes.POINTER(ChainState), u8p, ctypes.POINTER(ctypes.c_size_t),
                                              ctypes.POINTER(ctypes.c_size_t)]),
    "praos_state_encode": (ctypes.c_int, [ctypes.POINTER(ChainState), u8p, ctypes.c_size_t,
                                          ctypes.POINTER(ctypes.c_size_t)]),
    "praos_state_decode": (ctypes.c_int, [u8p, ctypes.c_size_t, ctypes.POINTER(ChainState)]),
    "praos_replay_immutable": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(Pool), ctypes.c_uint32,
                                              ctypes.POINTER(Params), ctypes.POINTER(EpochInfo),
                                              ctypes.POINTER(Envelope), ctypes.POINTER(ChainState), ctypes.c_size_t,
                                              u8p, ctypes.c_size_t, ctypes.POINTER(ReplayStats)]),
    "praos_replay_immutable_tpraos": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(Pool),
                                                     ctypes.c_uint32, ctypes.POINTER(Params),
                                                     ctypes.POINTER(EpochInfo), ctypes.POINTER(Nonce),
                                                     ctypes.POINTER(Envelope), ctypes.POINTER(ChainState),
                                                     ctypes.c_size_t, u8p, u16p, ctypes.c_size_t,
                                                     ctypes.POINTER(ReplayStats)]),
    "praos_replay_immutable_views": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(LedgerView),
                                                    ctypes.c_uint32, ctypes.POINTER(Params), ctypes.POINTER(EpochInfo),
                                                    ctypes.POINTER(Envelope), ctypes.POINTER(ChainState),
                                                    ctypes.c_size_t, u8p, ctypes.c_size_t,
                                                    ctypes.POINTER(ReplayStats)]),
    "praos_batch_upload_tpraos_bytes": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.POINTER(HeaderBytes)]),
    "praos_batch_download_tpraos": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(TPOut)]),
    "praos_tpraos_validate_headers_nonces": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(TPHeaders), u8p, u8p,
                                                            ctypes.POINTER(TPOut), ctypes.POINTER(Envelope),
                                                            ctypes.POINTER(EpochInfo), ctypes.POINTER(Nonce),
                                                            ctypes.POINTER(ChainState), ctypes.POINTER(Nonce),
                                                            ctypes.c_uint32, u8p, u8p, u16p,
                                                            ctypes.POINTER(ctypes.c_size_t),
                                                            ctypes.POINTER(ctypes.c_size_t)]),
    "praos_ticked_epoch_nonce": (ctypes.c_int, [ctypes.POINTER(ChainState), ctypes.POINTER(EpochInfo), ctypes.c_uint64,
                                                ctypes.POINTER(Nonce)]),
    "praos_tpraos_ticked_epoch_nonce": (ctypes.c_int, [ctypes.POINTER(ChainState), ctypes.POINTER(EpochInfo),
                                                       ctypes.c_uint64, ctypes.POINTER(Nonce), ctypes.POINTER(Nonce)]),
    "praos_group_open": (ctypes.c_void_p, [i32p, ctypes.c_int]),
    "praos_group_close": (None, [ctypes.c_void_p]),
    "praos_group_size": (ctypes.c_int, [ctypes.c_void_p]),
    "praos_group_ctx": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int]),
    "praos_group_last_error": (ctypes.c_char_p, [ctypes.c_void_p]),
    "praos_group_set_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "praos_group_set_epoch": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.POINTER(Pool), ctypes.c_uint32,
                                             ctypes.POINTER(Params)]),
    "praos_group_verify_headers": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Headers), ctypes.POINTER(Out)]),
    "praos_group_verify_header_bytes": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HeaderBytes),
                                                       ctypes.POINTER(Out), ctypes.POINTER(Decoded)]),
    "praos_group_verify_tpraos_headers": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(TPHeaders),
                                                         ctypes.POINTER(TPOut)]),
    "praos_group_verify_tpraos_header_bytes": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HeaderBytes),
                                                              ctypes.POINTER(TPOut), ctypes.POINTER(Decoded), u8p,
                                                              u8p]),
    "praos_group_set_overlay": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Overlay)]),
    "praos_group_host_register": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    "praos_group_host_unregister": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "praos_group_replay_immutable": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(Pool),
                                                    ctypes.c_uint32, ctypes.POINTER(Params), ctypes.POINTER(EpochInfo),
                                                    ctypes.POINTER(Envelope), ctypes.POINTER(ChainState),
                                                    ctypes.c_size_t, u8p, ctypes.c_size_t,
                                                    ctypes.POINTER(ReplayStats)]),
    "praos_group_replay_immutable_tpraos": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(Pool),
                                                           ctypes.c_uint32, ctypes.POINTER(Params),
                                                           ctypes.POINTER(EpochInfo), ctypes.POINTER(Nonce),
                                                           ctypes.POINTER(Envelope), ctypes.POINTER(ChainState),
                                                           ctypes.c_size_t, u8p, u16p, ctypes.c_size_t,
                                                           ctypes.POINTER(ReplayStats)]),
    "praos_group_verify_block_integrity": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HeaderBytes),
                                                          ctypes.c_uint64, u8p, u8p]),
    "praos_group_replay_immutable_views": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p,
                                                          ctypes.POINTER(LedgerView), ctypes.c_uint32,
                                                          ctypes.POINTER(Params), ctypes.POINTER(EpochInfo),
                                                          ctypes.POINTER(Envelope), ctypes.POINTER(ChainState),
                                                          ctypes.c_size_t, u8p, ctypes.c_size_t,
                                                          ctypes.POINTER(ReplayStats)]),
    "praos_synthesize": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(SynthParams), ctypes.POINTER(Params), u8p,
                                        ctypes.POINTER(Pool), u64p, u8p, u8p, u8p, u8p, u8p, u64p, u64p, u8p, u8p,
                                        u64p, u32p, u8p, u8p]),
    "praos_leader_schedule": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_uint32, u8p, ctypes.POINTER(Params), u8p,
                                             ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, i32p]),
    "praos_verify_tpraos_headers": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(TPHeaders),
                                                   ctypes.POINTER(TPOut)]),
    "praos_set_overlay": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Overlay)]),
    "praos_overlay_classify": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, u64p, i32p]),
    "praos_tpraos_update_chain_dep_state": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(TPHeaders), u8p, u8p,
                                                           ctypes.POINTER(TPOut), ctypes.POINTER(Envelope),
                                                           ctypes.POINTER(EpochInfo), ctypes.POINTER(Nonce),
                                                           ctypes.POINTER(ChainState), u8p, u16p,
                                                           ctypes.POINTER(ctypes.c_size_t),
                                                           ctypes.POINTER(ctypes.c_size_t)]),
    "praos_synthesize_tpraos": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(SynthParams), ctypes.POINTER(Params),
                                               u8p, ctypes.POINTER(Pool), u64p, u8p, u8p, u8p, u8p, u8p, u64p, u64p,
                                               u8p, u8p, u64p, u32p, u8p, u8p, u8p, u8p]),
    "praos_decode_headers": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HeaderBytes), ctypes.POINTER(Decoded)]),
    "praos_verify_header_bytes": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HeaderBytes), ctypes.POINTER(Out),
                                                 ctypes.POINTER(Decoded)]),
    "praos_verify_header_bytes_submit": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HeaderBytes),
                                                        ctypes.POINTER(Out), ctypes.POINTER(Decoded)]),
    "praos_verify_drain": (ctypes.c_int, [ctypes.c_void_p]),
    "praos_verify_tpraos_header_bytes": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HeaderBytes),
                                                        ctypes.POINTER(TPOut), ctypes.POINTER(Decoded), u8p, u8p]),
    "praos_batch_upload_bytes": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.POINTER(HeaderBytes)]),
    "praos_batch_download_decoded": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Decoded)]),
    "praos_batch_decode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "praos_batch_set_nonces": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Nonce), ctypes.c_uint32,
                                              u8p]),
    "praos_validate_headers_nonces": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Headers), u8p, u8p,
                                                     ctypes.POINTER(Out), ctypes.POINTER(Envelope),
                                                     ctypes.POINTER(EpochInfo), ctypes.POINTER(ChainState),
                                                     ctypes.POINTER(Nonce), ctypes.c_uint32, u8p, u8p,
                                                     ctypes.POINTER(ctypes.c_size_t),
                                                     ctypes.POINTER(ctypes.c_size_t)]),
    "praos_verify_block_integrity": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HeaderBytes), ctypes.c_uint64,
                                                    u8p, u8p]),
    "praos_crc32": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HeaderBytes), u32p]),
    "praos_block_batch_crc32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, u32p]),
    "praos_validate_chunk": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Chunk), ctypes.c_uint64,
                                            ctypes.POINTER(ChunkResult), ctypes.POINTER(ChunkOut)]),
    "praos_validate_chunk_cfg": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Chunk), ctypes.POINTER(ChunkCfg),
                                                ctypes.POINTER(ChunkResult), ctypes.POINTER(ChunkOut), u8p]),
    "praos_verify_byron_integrity": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HeaderBytes), ctypes.c_uint64,
                                                    ctypes.c_uint32, u8p, u8p]),
    "praos_byron_key_hash": (ctypes.c_int, [ctypes.c_void_p, u8p, ctypes.c_size_t, u8p]),
    "praos_verify_pbft_headers": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HeaderBytes), u8p,
                                                 ctypes.POINTER(PbftParams), u8p, ctypes.c_uint32,
                                                 ctypes.POINTER(PbftOut)]),
    "praos_pbft_stats": (ctypes.c_int, [ctypes.c_void_p, u32p]),
    "praos_pbft_update_chain_dep_state": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(PbftOut),
                                                         u8p, ctypes.POINTER(PbftParams), u8p, ctypes.c_uint32,
                                                         ctypes.POINTER(PbftTip), ctypes.POINTER(PbftStateC), u8p,
                                                         u64p, ctypes.POINTER(ctypes.c_size_t)]),
    "praos_pbft_state_encode": (ctypes.c_int, [ctypes.POINTER(PbftStateC), u8p, ctypes.c_size_t,
                                               ctypes.POINTER(ctypes.c_size_t)]),
    "praos_pbft_state_decode": (ctypes.c_int, [u8p, ctypes.c_size_t, ctypes.POINTER(PbftStateC)]),
    "praos_index_block_txs": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HeaderBytes), ctypes.POINTER(TxiCfg),
                                             ctypes.POINTER(TxiStats), ctypes.POINTER(TxiRows)]),
    "praos_block_batch_tx_index": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(TxiCfg),
                                                  ctypes.POINTER(TxiStats), ctypes.POINTER(TxiRows)]),
    "praos_verify_tx_witnesses": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HeaderBytes), ctypes.POINTER(TxwCfg),
                                                 ctypes.POINTER(TxwBlocks), ctypes.POINTER(TxwTxs),
                                                 ctypes.POINTER(TxwWits)]),
    "praos_verify_gen_txs": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HeaderBytes), ctypes.POINTER(GtxCfg),
                                            ctypes.POINTER(GtxItems), ctypes.POINTER(GtxTxs), ctypes.POINTER(TxwWits)]),
    "praos_verify_fetched_blocks": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(HeaderBytes),
                                                   ctypes.POINTER(BfRanges), ctypes.POINTER(BfCfg),
                                                   ctypes.POINTER(BfItems), ctypes.POINTER(BfRangeOut),
                                                   ctypes.POINTER(BfRows), ctypes.POINTER(TxwBlocks),
                                                   ctypes.POINTER(TxwTxs), ctypes.POINTER(TxwWits)]),
    "praos_debug_span_equal": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, u8p, ctypes.c_size_t, u64p, u64p, u32p,
                                              u8p]),
    "praos_debug_row_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, u8p, u8p, u8p, ctypes.c_uint32, ctypes.c_int,
                                           u32p, u32p, u32p]),
    "praos_block_batch_tx_witnesses": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(TxwCfg),
                                                      ctypes.POINTER(TxwBlocks), ctypes.POINTER(TxwTxs),
                                                      ctypes.POINTER(TxwWits)]),
    "praos_block_batch_upload": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.POINTER(HeaderBytes)]),
    "praos_block_batch_run": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "praos_block_batch_download": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, u8p, u8p]),
    "praos_debug_fe": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, u8p, u8p, u8p]),
    "praos_debug_sha512": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, u8p, u64p, u32p, u8p, ctypes.c_size_t,
                                          u8p]),
    "praos_debug_blake2b": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, u8p, u8p]),
    "praos_debug_sc_reduce": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, u8p, u8p]),
    "praos_debug_decode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, u8p, u8p, u8p]),
    "praos_debug_scalarmult_base": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, u8p, u8p]),
    "praos_debug_leader": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, u8p, u8p, u8p, i32p]),
    "praos_debug_leader512": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, u8p, u8p, u8p, i32p]),
    "praos_debug_hash_to_curve": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, u8p, u8p, u8p]),
    "praos_debug_fe_multi": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, u8p, u8p]),
    "praos_debug_ge": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, u8p, u8p, u8p]),
    "praos_debug_msm": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, u8p, u8p, u8p,
                                       u8p, u8p, u8p]),
    "praos_debug_hash_bytes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, u8p, ctypes.c_size_t,
                                              u64p, u32p, u8p, u64p, ctypes.c_size_t, u8p]),
    "praos_debug_int": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, u8p, u8p, u8p, u8p]),
    # wire headers (the structs are praos_hip.wire's)
    "praos_unwrap_wire_headers": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    "praos_validate_candidates": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "praos_validate_candidates_tpraos": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                        ctypes.c_void_p]),
    "praos_validate_candidates_pbft": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.c_void_p]),
}

_lib = None


def load():
    """Load libpraos_hip.so (raises if it was not built: there is no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: build it with __graft_entry__.build() "
                               "(make -C ouroboros-consensus_amd/csrc)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def ptr(a, t=u8p):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(t)


OPT_CONCURRENT, OPT_KERNELS, OPT_KEYCACHE, OPT_DEDUP, OPT_PIPELINE, OPT_KES_PAIR, OPT_POOL_KEYS = 1, 2, 3, 4, 5, 6, 7
OPT_KES_NOCACHE = 8
# (praos_set_option, praos_hip.h)


class PraosError(RuntimeError):
    pass


class Context:
    """One praos_ctx (one GPU).  Mirrors the lifetime rules of the C ABI."""

    def __init__(self, device: int = 0):
        self.L = load()
        self.h = self.L.praos_open(device)
        if not self.h:
            raise PraosError(f"praos_open({device}) failed (no HIP device?)")
        self._keep = []

    def close(self):
        if self.h:
            self.L.praos_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def check(self, rc):
        if rc != 0:
            msg = self.L.praos_last_error(self.h)
            raise PraosError(f"praos rc={rc}: {msg.decode() if msg else ''}")

    # ---- epoch ----
    @staticmethod
    def pool_array(pools):
        """pools: list of (hash28: bytes, vrf_hash32: bytes, sigma_fp: int)."""
        if not pools:
            return (Pool * 1)()
        # one buffer of 76-byte records (the struct has no padding), copied in once
        data = b"".join(bytes(h)[:28].ljust(28, b"\0") + bytes(v)[:32].ljust(32, b"\0") + int(s).to_bytes(16, "little")
                        for h, v, s in pools)
        return (Pool * len(pools)).from_buffer_copy(data)

    def set_epoch(self, eta0, pools, params: Params):
        """pools: list of (hash28: bytes, vrf_hash32: bytes, sigma_fp: int)."""
        arr = self.pool_array(pools)
        e = None
        if eta0 is not None:
            eb = np.frombuffer(bytes(eta0), dtype=np.uint8).copy()
            self._keep.append(eb)
            e = ptr(eb)
        self.check(self.L.praos_set_epoch(self.h, e, arr, len(pools), ctypes.byref(params)))
        self._keep.append(arr)

    # ---- headers ----
    @staticmethod
    def headers_struct(H: dict):
        """H: dict of numpy arrays: slot u64[n], cold_vk u8[n,32], vrf_vk, vrf_out[n,64], vrf_proof[n,80],
        hot_vk, ocert_n u64, ocert_c0 u64, ocert_sig[n,64], kes_sig[n,448], body_off u64, body_len u32,
        body_bytes u8[]."""
        s = Headers()
        s.n = len(H["slot"])
        s.slot = ptr(H["slot"], u64p)
        for k in ("cold_vk", "vrf_vk", "vrf_out", "vrf_proof", "hot_vk", "ocert_sig", "kes_sig", "body_bytes"):
            setattr(s, k, ptr(H[k]))
        s.ocert_n = ptr(H["ocert_n"], u64p)
        s.ocert_c0 = ptr(H["ocert_c0"], u64p)
        s.body_off = ptr(H["body_off"], u64p)
        s.body_len = ptr(H["body_len"], u32p)
        s.body_bytes_len = len(H["body_bytes"])
        return s

    @staticmethod
    def alloc_out(n):
        return {"bits": np.zeros(n, np.uint16), "pool_idx": np.zeros(n, np.int32),
                "beta": np.zeros((n, 64), np.uint8), "leader": np.zeros((n, 32), np.uint8),
                "nonce": np.zeros((n, 32), np.uint8)}

    @staticmethod
    def out_struct(o):
        s = Out()
        s.bits = ptr(o["bits"], u16p)
        s.pool_idx = ptr(o["pool_idx"], i32p)
        s.beta = ptr(o["beta"])
        s.leader = ptr(o["leader"])
        s.nonce = ptr(o["nonce"])
        return s

    def verify_headers(self, H, out=None):
        """out: caller-owned output arrays (alloc_out) reused across calls, as a replay loop does."""
        n = len(H["slot"])
        o = self.alloc_out(n) if out is None else out
        hs = self.headers_struct(H)
        os_ = self.out_struct(o)
        self.check(self.L.praos_verify_headers(self.h, ctypes.byref(hs), ctypes.byref(os_)))
        return o

    @staticmethod
    def tp_headers_struct(H):
        th = TPHeaders()
        th.h = Context.headers_struct(H)
        th.leader_out = ptr(H["leader_out"])
        th.leader_proof = ptr(H["leader_proof"])
        return th

    @staticmethod
    def tp_out(n):
        """TPraos output arrays and their praos_tpraos_out struct."""
        o = {"bits": np.zeros(n, np.uint16), "pool_idx": np.zeros(n, np.int32),
             "beta_eta": np.zeros((n, 64), np.uint8), "beta_leader": np.zeros((n, 64), np.uint8),
             "nonce": np.zeros((n, 32), np.uint8)}
        to = TPOut()
        to.bits, to.pool_idx = ptr(o["bits"], u16p), ptr(o["pool_idx"], i32p)
        to.beta_eta, to.beta_leader, to.nonce = ptr(o["beta_eta"]), ptr(o["beta_leader"]), ptr(o["nonce"])
        return o, to

    def verify_tpraos_headers(self, H):
        """H as for verify_headers plus leader_out [n,64] / leader_proof [n,80] (the bheaderL cert)."""
        th = self.tp_headers_struct(H)
        o, to = self.tp_out(len(H["slot"]))
        self.check(self.L.praos_verify_tpraos_headers(self.h, ctypes.byref(th), ctypes.byref(to)))
        return o

    def set_overlay(self, d, f, epoch_base_slot, epoch_length, gen_delegs):
        """TPraos overlay schedule (praos_set_overlay): d, f Fractions; gen_delegs list of
        (genesis_hash28, delegate_hash28, vrf_hash32).  d = None clears everything."""
        if d is None:
            self.check(self.L.praos_set_overlay(self.h, None))
            return
        arr = (GenDeleg * max(1, len(gen_delegs)))()
        for k, (g, dl, v) in enumerate(gen_delegs):
            ctypes.memmove(arr[k].genesis_hash28, bytes(g), 28)
            ctypes.memmove(arr[k].delegate_hash28, bytes(dl), 28)
            ctypes.memmove(arr[k].vrf_hash32, bytes(v), 32)
        ov = Overlay(d.numerator, d.denominator, f.numerator, f.denominator, epoch_base_slot, epoch_length,
                     ctypes.cast(arr, ctypes.POINTER(GenDeleg)), len(gen_delegs))
        self._overlay_keep = arr
        self.check(self.L.praos_set_overlay(self.h, ctypes.byref(ov)))

    def overlay_classify(self, slots):
        s = np.ascontiguousarray(slots, dtype=np.uint64)
        out = np.zeros(len(s), np.int32)
        self.check(self.L.praos_overlay_classify(self.h, len(s), ptr(s, u64p), ptr(out, i32p)))
        return out

    def tpraos_update_chain_dep_state(self, H, crypto, prev_hash, state: dict, epoch_info, prev_is_genesis=None,
                                      extra_entropy=None):
        """praos_tpraos_update_chain_dep_state over TPraos outputs (verify_tpraos_headers);
        state as for update_chain_dep_state (updated in place).  Returns (verdict u8[n],
        failures u16[n], chain_stop, processed)."""
        n = len(H["slot"])
        th = TPHeaders()
        th.h = self.headers_struct(H)
        th.leader_out = ptr(H["leader_out"])
        th.leader_proof = ptr(H["leader_proof"])
        to = TPOut()
        to.bits = ptr(crypto["bits"], u16p)
        to.pool_idx = ptr(crypto["pool_idx"], i32p)
        to.nonce = ptr(crypto["nonce"])
        st, hk, cv = _state_struct(state, len(state.get("counters", {})) + n)
        ei = EpochInfo(*epoch_info)
        ph = np.ascontiguousarray(prev_hash, dtype=np.uint8)
        pg = None if prev_is_genesis is None else np.ascontiguousarray(prev_is_genesis, dtype=np.uint8)
        xe = None
        if extra_entropy is not None:
            xe = Nonce()
            ctypes.memmove(xe.hash, bytes(extra_entropy), 32)
        verdict = np.zeros(n, np.uint8)
        fails = np.zeros(n, np.uint16)
        stop, done = ctypes.c_size_t(0), ctypes.c_size_t(0)
        self.check(self.L.praos_tpraos_update_chain_dep_state(
            self.h, ctypes.byref(th), ptr(ph), ptr(pg) if pg is not None else None, ctypes.byref(to), None,
            ctypes.byref(ei), ctypes.byref(xe) if xe is not None else None, ctypes.byref(st), ptr(verdict),
            ptr(fails, u16p), ctypes.byref(stop), ctypes.byref(done)))
        new = _state_from_struct(st, hk, cv)
        state.clear()
        state.update(new)
        return verdict, fails, int(stop.value), int(done.value)

    def upload(self, H):
        hs = self.headers_struct(H)
        b = self.L.praos_batch_upload(self.h, ctypes.byref(hs))
        if not b:
            self.check(-3)
        return b

    def run(self, b):
        self.check(self.L.praos_batch_run(self.h, b))

    def sync(self):
        self.check(self.L.praos_batch_sync(self.h))

    def set_option(self, opt, value):
        self.check(self.L.praos_set_option(self.h, opt, value))

    def set_vrf_wide(self, min_uses=-1, max_keys=0):
        """Wide tier of the VRF key cache: keys with min_uses uses in a batch (-1 automatic, 0 off),
        at most max_keys of them per batch (0: the default)."""
        self.check(self.L.praos_set_vrf_wide(self.h, min_uses, max_keys))

    def batch_stats(self, b):
        """Key-cache statistics of the last run: dict of cold/vrf/kes entries, hits, misses."""
        out = np.zeros(9, np.uint32)
        self.check(self.L.praos_batch_stats(self.h, b, ptr(out, u32p)))
        w = np.zeros(2, np.uint32)
        self.check(self.L.praos_batch_wide_stats(self.h, b, ptr(w, u32p)))
        return {"cold_keys": int(out[0]), "cold_hits": int(out[1]), "cold_misses": int(out[2]),
                "vrf_keys": int(out[3]), "vrf_hits": int(out[4]), "vrf_misses": int(out[5]),
                "kes_keys": int(out[6]), "kes_hits": int(out[7]), "kes_misses": int(out[8]),
                "vrf_wide_keys": int(w[0]), "vrf_wide_hits": int(w[1])}

    def dedup_stats(self, b):
        """OCert dedup of the last run: distinct OCert tuples verified, headers."""
        out = np.zeros(2, np.uint32)
        self.check(self.L.praos_batch_dedup_stats(self.h, b, ptr(out, u32p)))
        return {"ocert_unique": int(out[0]), "headers": int(out[1])}

    def kernel_ms(self, which):
        return float(self.L.praos_batch_kernel_ms(self.h, which))

    def download(self, b, n, out=None):
        o = self.alloc_out(n) if out is None else out
        os_ = self.out_struct(o)
        self.check(self.L.praos_batch_download(self.h, b, ctypes.byref(os_)))
        return o

    def free(self, b):
        self.L.praos_batch_free(self.h, b)

    # ---- stored header bytes (GPU decode, k_decode.hip) ----
    @staticmethod
    def header_bytes_struct(arena, off, length):
        s = HeaderBytes()
        s.n = len(off)
        s.bytes = ptr(arena)
        s.bytes_len = len(arena)
        s.off = ptr(off, u64p)
        s.len = ptr(length, u32p)
        return s

    @staticmethod
    def alloc_decoded(n, stride=SIGNED_STRIDE):
        D = {name: np.zeros((n,) + (shp if name != "signed_body" else (stride,)), dt)
             for name, dt, shp in DECODED_FIELDS}
        d = Decoded()
        for name, dt, _ in DECODED_FIELDS:
            setattr(d, name, ptr(D[name], _CT[dt]))
        return D, d

    @staticmethod
    def _chunk(arena, off, length):
        return (np.ascontiguousarray(np.frombuffer(arena, np.uint8) if isinstance(arena, (bytes, bytearray))
                                     else arena, dtype=np.uint8),
                np.ascontiguousarray(off, dtype=np.uint64), np.ascontiguousarray(length, dtype=np.uint32))

    def decode_headers(self, arena, off, length):
        """Decode stored Praos headers arena[off[i]:off[i]+len[i]] on the GPU; returns a dict of arrays
        (DECODED_FIELDS)."""
        arena, off, length = self._chunk(arena, off, length)
        hb = self.header_bytes_struct(arena, off, length)
        D, d = self.alloc_decoded(len(off))
        self.check(self.L.praos_decode_headers(self.h, ctypes.byref(hb), ctypes.byref(d)))
        return D

    def verify_header_bytes(self, arena, off, length, decoded=False, out=None):
        """out: caller-owned output arrays (alloc_out) reused across calls."""
        arena, off, length = self._chunk(arena, off, length)
        n = len(off)
        hb = self.header_bytes_struct(arena, off, length)
        o = self.alloc_out(n) if out is None else out
        os_ = self.out_struct(o)
        D, d = self.alloc_decoded(n) if decoded else (None, None)
        self.check(self.L.praos_verify_header_bytes(self.h, ctypes.byref(hb), ctypes.byref(os_),
                                                    ctypes.byref(d) if d is not None else None))
        return (o, D) if decoded else o

    def submit_header_bytes(self, arena, off, length, out, decoded=None):
        """Streaming form of verify_header_bytes (praos_verify_header_bytes_submit): queued, returns
        at once; out (and decoded, an alloc_decoded pair) are written by the third submit after it
        or by drain().  The inputs and outputs stay referenced here until drained."""
        arena, off, length = self._chunk(arena, off, length)
        hb = self.header_bytes_struct(arena, off, length)
        os_ = self.out_struct(out)
        d = decoded[1] if decoded is not None else None
        self.check(self.L.praos_verify_header_bytes_submit(self.h, ctypes.byref(hb), ctypes.byref(os_),
                                                           ctypes.byref(d) if d is not None else None))
        self._inflight = (getattr(self, "_inflight", []) + [(arena, off, length, hb, os_, out, decoded)])[-4:]

    def drain(self):
        """Every submitted call's outputs written (praos_verify_drain)."""
        self.check(self.L.praos_verify_drain(self.h))
        self._inflight = []

    def verify_tpraos_header_bytes(self, arena, off, length, decoded=False):
        """Stored TPraos headers (BHeader = [BHBody, kesSig], Shelley..Alonzo) decoded and
        verified on the GPU (praos_verify_tpraos_header_bytes).  Returns the TPraos outputs
        (bits, pool_idx, beta_eta, beta_leader, nonce); with decoded=True also the decoded
        fields plus leader_out / leader_proof."""
        arena, off, length = self._chunk(arena, off, length)
        n = len(off)
        hb = self.header_bytes_struct(arena, off, length)
        o, to = self.tp_out(n)
        D, d = self.alloc_decoded(n, TP_SIGNED_STRIDE) if decoded else (None, None)
        lo = np.zeros((n, 64), np.uint8) if decoded else None
        lp = np.zeros((n, 80), np.uint8) if decoded else None
        self.check(self.L.praos_verify_tpraos_header_bytes(self.h, ctypes.byref(hb), ctypes.byref(to),
                                                           ctypes.byref(d) if d is not None else None,
                                                           ptr(lo) if decoded else None, ptr(lp) if decoded else None))
        if not decoded:
            return o
        D["leader_out"], D["leader_proof"] = lo, lp
        return o, D

    # ---- stored blocks: verifyBlockIntegrity (k_block.hip) ----
    def verify_block_integrity(self, arena, off, length, slots_per_kes_period):
        """Integrity.hs:14-20 over blocks arena[off[i]:off[i]+len[i]]; returns (result u8[n] of
        PRAOS_BLK_* bits, computed hashTxSeq u8[n,32])."""
        arena, off, length = self._chunk(arena, off, length)
        n = len(off)
        hb = self.header_bytes_struct(arena, off, length)
        res = np.zeros(n, np.uint8)
        bh = np.zeros((n, 32), np.uint8)
        self.check(self.L.praos_verify_block_integrity(self.h, ctypes.byref(hb), slots_per_kes_period, ptr(res),
                                                       ptr(bh)))
        return res, bh

    # ---- stored blocks: the transaction index (k_txindex.hip) ----
    def _tx_index(self, call, n, byron, rows, cap, out=None):
        """call(cfg, stats, rows) -> rc.  rows: True (every row array), False (none) or the names
        wanted; cap: the row capacity (None: sized by a first call without row arrays); out: the
        (stats, rows) dicts of an earlier call with the same n and cap, written again in place."""
        cfg = TxiCfg(1 if byron else 0, 0)
        S = out[0] if out else {name: np.zeros(n + 1 if name == "tx_first" else n, dt)
                                for name, dt in TXI_STATS_FIELDS}
        st = TxiStats()
        for name, dt in TXI_STATS_FIELDS:
            setattr(st, name, ptr(S[name], _CT[dt]))
        names = [f[0] for f in TXI_ROW_FIELDS] if rows is True else list(rows or ())
        rw = TxiRows()
        if cap is None:
            self.check(call(cfg, st, rw))
            cap = int(rw.n_rows)
        R = out[2] if out else {name: np.zeros((cap,) + shp, dt) for name, dt, shp in TXI_ROW_FIELDS
                                if name in names}
        rw = TxiRows()
        rw.cap = cap
        for name, dt, _ in TXI_ROW_FIELDS:
            if name in R:
                setattr(rw, name, ptr(R[name], _CT[dt]))
        rc = call(cfg, st, rw)
        if rc == E_ARG and rw.n_rows > cap:
            msg = self.L.praos_last_error(self.h)
            err = PraosError(f"praos rc={rc}: {msg.decode() if msg else ''}")
            err.needed, err.stats = int(rw.n_rows), S
            raise err
        self.check(rc)
        k = int(rw.n_rows)
        return S, {name: a[:k] for name, a in R.items()}, R

    def index_block_txs(self, arena, off, length, byron=False, rows=True, cap=None):
        """The transaction index of the stored blocks arena[off[i]:off[i]+len[i]]
        (praos_index_block_txs).  Returns (stats, rows): stats = dict of per-block arrays
        (TXI_STATS_FIELDS; tx_first has n + 1 entries), rows = dict of per-transaction arrays
        (TXI_ROW_FIELDS, or the names given in rows; False: none, stats only).  byron: Byron
        blocks and EBBs are indexed too.  cap: capacity of the row arrays (default: sized by a
        first call); a smaller one raises PraosError with .needed and .stats set."""
        arena, off, length = self._chunk(arena, off, length)
        hb = self.header_bytes_struct(arena, off, length)
        return self._tx_index(lambda cfg, st, rw: self.L.praos_index_block_txs(
            self.h, ctypes.byref(hb), ctypes.byref(cfg), ctypes.byref(st), ctypes.byref(rw)),
            len(off), byron, rows, cap)[:2]

    def tx_index_blocks(self, b, n, byron=False, rows=True, cap=None, out=None):
        """index_block_txs over an upload_blocks batch (praos_block_batch_tx_index): no second
        upload.  out: tx_index_buffers(n, cap, rows), written in place (a caller indexing batch
        after batch into its own arrays); then (stats, rows cut to n_rows, the full row arrays)
        is returned."""
        r = self._tx_index(lambda cfg, st, rw: self.L.praos_block_batch_tx_index(
            self.h, b, ctypes.byref(cfg), ctypes.byref(st), ctypes.byref(rw)), n, byron, rows, cap, out)
        return r if out is not None else r[:2]

    def tx_index_buffers(self, n, cap, rows=True):
        """Output arrays for tx_index_blocks(..., cap=cap, out=...): (stats, rows, row arrays)."""
        names = [f[0] for f in TXI_ROW_FIELDS] if rows is True else list(rows or ())
        S = {name: np.zeros(n + 1 if name == "tx_first" else n, dt) for name, dt in TXI_STATS_FIELDS}
        R = {name: np.zeros((cap,) + shp, dt) for name, dt, shp in TXI_ROW_FIELDS if name in names}
        return S, R, R

    # ---- stored blocks: the transactions' key witnesses (k_txwit.hip) ----
    def tx_witness_buffers(self, n, tx_cap, wit_cap, rows=True):
        """Output arrays for verify_tx_witnesses / tx_witnesses_blocks(..., out=...): (blocks, txs,
        wits) dicts of n blocks, tx_cap rows (wit_first: tx_cap + 1) and wit_cap witnesses; rows =
        False: the per-block arrays only."""
        B = {name: np.zeros(n + 1 if name == "tx_first" else n, dt) for name, dt in TXW_BLOCK_FIELDS}
        if not rows:
            return B, {}, {}
        T = {name: np.zeros((tx_cap + 1 if name == "wit_first" else tx_cap,) + shp, dt)
             for name, dt, shp in TXW_TX_FIELDS}
        W = {name: np.zeros((wit_cap,) + shp, dt) for name, dt, shp in TXW_WIT_FIELDS}
        return B, T, W

    def _tx_witnesses(self, call, n, byron, max_lanes, rows, cap, out):
        """call(cfg, blocks, txs, wits) -> rc.  rows: every row and witness array (True) or the
        per-block arrays only; cap: (rows, witnesses) capacities (None: sized by a first call
        without row arrays); out: tx_witness_buffers of the same n, written again in place."""
        cfg = TxwCfg(1 if byron else 0, max_lanes)
        if out is None and rows and cap is None:
            ts, ws = TxwTxs(), TxwWits()
            self.check(call(cfg, None, ts, ws))
            cap = (int(ts.n_rows), int(ws.n_wits))
        B, T, W = out if out is not None else self.tx_witness_buffers(n, *(cap or (0, 0)), rows=rows)
        bs, ts, ws = TxwBlocks(), TxwTxs(), TxwWits()
        for name, dt in TXW_BLOCK_FIELDS:
            setattr(bs, name, ptr(B[name], _CT[dt]))
        if T:
            ts.cap = len(T["block"])
            for name, dt, _ in TXW_TX_FIELDS:
                setattr(ts, name, ptr(T[name], _CT[dt]))
        if W:
            ws.cap = len(W["tx"])
            for name, dt, _ in TXW_WIT_FIELDS:
                setattr(ws, name, ptr(W[name], _CT[dt]))
        rc = call(cfg, bs, ts, ws)
        if rc == E_ARG and (T or W) and (ts.n_rows > ts.cap or ws.n_wits > ws.cap):
            msg = self.L.praos_last_error(self.h)
            err = PraosError(f"praos rc={rc}: {msg.decode() if msg else ''}")
            err.needed, err.blocks = (int(ts.n_rows), int(ws.n_wits)), B
            raise err
        self.check(rc)
        nt, nw = int(ts.n_rows), int(ws.n_wits)
        return (B, {k: a[:nt + 1 if k == "wit_first" else nt] for k, a in T.items()},
                {k: a[:nw] for k, a in W.items()}, (nt, nw))

    def verify_tx_witnesses(self, arena, off, length, byron=False, max_lanes=0, rows=True, cap=None, out=None):
        """Every VKey and bootstrap witness of the stored blocks arena[off[i]:off[i]+len[i]]
        checked over its transaction's txId (praos_verify_tx_witnesses).  Returns (blocks, txs,
        wits, (n_rows, n_wits)): dicts of per-block (TXW_BLOCK_FIELDS), per-transaction
        (TXW_TX_FIELDS) and per-witness (TXW_WIT_FIELDS) arrays; rows=False: the per-block arrays
        only.  cap: (row, witness) capacities (default: sized by a first call); smaller ones raise
        PraosError with .needed and .blocks set.  max_lanes: witnesses per launch (0: default)."""
        arena, off, length = self._chunk(arena, off, length)
        hb = self.header_bytes_struct(arena, off, length)
        return self._tx_witnesses(lambda cfg, bs, ts, ws: self.L.praos_verify_tx_witnesses(
            self.h, ctypes.byref(hb), ctypes.byref(cfg), ctypes.byref(bs) if bs is not None else None,
            ctypes.byref(ts), ctypes.byref(ws)), len(off), byron, max_lanes, rows, cap, out)

    def tx_witnesses_blocks(self, b, n, byron=False, max_lanes=0, rows=True, cap=None, out=None):
        """verify_tx_witnesses over an upload_blocks batch (praos_block_batch_tx_witnesses): no
        second upload."""
        return self._tx_witnesses(lambda cfg, bs, ts, ws: self.L.praos_block_batch_tx_witnesses(
            self.h, b, ctypes.byref(cfg), ctypes.byref(bs) if bs is not None else None, ctypes.byref(ts),
            ctypes.byref(ws)), n, byron, max_lanes, rows, cap, out)

    # ---- TxSubmission: wire transactions, each distinct one checked once (k_gentx.hip) ----
    def gen_tx_buffers(self, n, tx_cap, wit_cap, rows=True):
        """Output arrays for verify_gen_txs(..., out=...): (items, txs, wits) dicts of n items,
        tx_cap rows (wit_first: tx_cap + 1) and wit_cap witnesses; rows=False: the per-item arrays
        only."""
        I = {name: np.zeros(n, dt) for name, dt in GTX_ITEM_FIELDS}
        if not rows:
            return I, {}, {}
        T = {name: np.zeros((tx_cap + 1 if name == "wit_first" else tx_cap,) + shp, dt)
             for name, dt, shp in GTX_TX_FIELDS}
        W = {name: np.zeros((wit_cap,) + shp, dt) for name, dt, shp in TXW_WIT_FIELDS}
        return I, T, W

    def verify_gen_txs(self, arena, off, length, n_eras=7, dedup=True, max_lanes=0, rows=True, cap=None, out=None):
        """The wire transactions arena[off[i]:off[i]+len[i]] (GenTxs in the node-to-node encoding)
        unwrapped, the distinct ones indexed and their key witnesses checked over their txId
        (praos_verify_gen_txs).  Returns (items, txs, wits, (n_rows, n_wits)): dicts of per-item
        (GTX_ITEM_FIELDS), per-distinct-transaction (GTX_TX_FIELDS) and per-witness
        (TXW_WIT_FIELDS, tx = the row) arrays; rows=False: the per-item arrays only.  dedup:
        byte-identical transactions of the same era share a row.  cap: (row, witness) capacities
        (default: sized by a first call); smaller ones raise PraosError with .needed and .items
        set.  max_lanes: witnesses per launch (0: default).  out: gen_tx_buffers of the same n,
        written again in place (a caller verifying batch after batch into its own arrays)."""
        arena, off, length = self._chunk(arena, off, length)
        hb = self.header_bytes_struct(arena, off, length)
        n = len(off)
        cfg = GtxCfg(n_eras, 1 if dedup else 0, max_lanes, 0)

        def call(it, ts, ws):
            return self.L.praos_verify_gen_txs(self.h, ctypes.byref(hb), ctypes.byref(cfg),
                                               ctypes.byref(it) if it is not None else None, ctypes.byref(ts),
                                               ctypes.byref(ws))
        if out is None and rows and cap is None:
            ts, ws = GtxTxs(), TxwWits()
            self.check(call(None, ts, ws))
            cap = (int(ts.n_rows), int(ws.n_wits))
        I, T, W = out if out is not None else self.gen_tx_buffers(n, *(cap or (0, 0)), rows=rows)
        it, ts, ws = GtxItems(), GtxTxs(), TxwWits()
        for name, dt in GTX_ITEM_FIELDS:
            setattr(it, name, ptr(I[name], _CT[dt]))
        if T:
            ts.cap = len(T["item"])
            for name, dt, _ in GTX_TX_FIELDS:
                setattr(ts, name, ptr(T[name], _CT[dt]))
        if W:
            ws.cap = len(W["tx"])
            for name, dt, _ in TXW_WIT_FIELDS:
                setattr(ws, name, ptr(W[name], _CT[dt]))
        rc = call(it, ts, ws)
        if rc == E_ARG and (T or W) and (ts.n_rows > ts.cap or ws.n_wits > ws.cap):
            msg = self.L.praos_last_error(self.h)
            err = PraosError(f"praos rc={rc}: {msg.decode() if msg else ''}")
            err.needed, err.items = (int(ts.n_rows), int(ws.n_wits)), I
            raise err
        self.check(rc)
        nt, nw = int(ts.n_rows), int(ws.n_wits)
        return (I, {k: a[:nt + 1 if k == "wit_first" else nt] for k, a in T.items()},
                {k: a[:nw] for k, a in W.items()}, (nt, nw))

    # ---- BlockFetch: wire blocks, each distinct one checked once (k_blockfetch.hip) ----
    def fetched_block_buffers(self, n, k, row_cap, tx_cap, wit_cap, rows=True):
        """Output arrays for verify_fetched_blocks(..., out=...): (items, ranges, rows, blocks, txs,
        wits) dicts of n items, k ranges, row_cap rows (the witness call's per-block arrays hold a
        row each), tx_cap transactions and wit_cap witnesses; rows=False: the per-item and
        per-range arrays only."""
        I = {name: np.zeros(n, dt) for name, dt in BF_ITEM_FIELDS}
        G = {name: np.zeros(k, dt) for name, dt in BF_RANGE_FIELDS}
        if not rows:
            return I, G, {}, {}, {}, {}
        R = {name: np.zeros((row_cap,) + shp, dt) for name, dt, shp in BF_ROW_FIELDS}
        B, T, W = self.tx_witness_buffers(row_cap, tx_cap, wit_cap)
        return I, G, R, B, T, W

    def verify_fetched_blocks(self, arena, off, length, item_first, exp_first, exp_slot, exp_hash, n_eras=7,
                              byron_epoch_slots=0, dedup=True, witnesses=True, max_lanes=0, rows=True, cap=None,
                              out=None):
        """The wire blocks arena[off[i]:off[i]+len[i]] (blocks in the node-to-node encoding, as the
        BlockFetch client receives them) held against the requested points, the distinct ones
        checked once: blockMatchesHeader and, with witnesses, their transactions' key witnesses
        (praos_verify_fetched_blocks).  item_first / exp_first (k + 1 each): range r holds items
        [item_first[r], item_first[r+1]) and expects the points [exp_first[r], exp_first[r+1]) of
        exp_slot / exp_hash (u8[., 32]).  Returns (items, ranges, rows, blocks, txs, wits, (n_rows,
        n_txs, n_wits)): dicts of per-item (BF_ITEM_FIELDS), per-range (BF_RANGE_FIELDS), per-row
        (BF_ROW_FIELDS) arrays and verify_tx_witnesses' three with "block" meaning row (empty
        without witnesses); rows=False: the per-item and per-range arrays only.  cap: (row,
        transaction, witness) capacities (default: sized by a first call, which costs a whole run
        of the pipeline, witness verifies included: a caller that knows bounds passes cap or
        out); smaller ones raise PraosError with .needed, .items and .ranges set, and the
        per-row witness counts are then not written.  out: fetched_block_buffers of the same n
        and k, written again in place."""
        arena, off, length = self._chunk(arena, off, length)
        hb = self.header_bytes_struct(arena, off, length)
        n = len(off)
        item_first = np.ascontiguousarray(item_first, np.uint64)
        exp_first = np.ascontiguousarray(exp_first, np.uint64)
        exp_slot = np.ascontiguousarray(exp_slot, np.uint64)
        exp_hash = np.ascontiguousarray(exp_hash, np.uint8).reshape(-1, 32)
        k = len(item_first) - 1
        rg = BfRanges(k, ptr(item_first, u64p), ptr(exp_first, u64p), ptr(exp_slot, u64p) if len(exp_slot) else None,
                      ptr(exp_hash) if len(exp_hash) else None)
        cfg = BfCfg(n_eras, 1 if dedup else 0, 1 if witnesses else 0, max_lanes, byron_epoch_slots)

        def call(it, ro, rs, bs, ts, ws):
            ref = lambda x: ctypes.byref(x) if x is not None else None
            return self.L.praos_verify_fetched_blocks(self.h, ctypes.byref(hb), ctypes.byref(rg), ctypes.byref(cfg),
                                                      ref(it), ref(ro), ref(rs), ref(bs), ref(ts), ref(ws))
        if out is None and rows and cap is None:
            rs, ts, ws = BfRows(), TxwTxs(), TxwWits()
            self.check(call(None, None, rs, None, ts, ws))
            cap = (int(rs.n_rows), int(ts.n_rows), int(ws.n_wits))
        I, G, R, B, T, W = out if out is not None else self.fetched_block_buffers(n, k, *(cap or (0, 0, 0)), rows=rows)
        if not witnesses:
            B, T, W = {}, {}, {}
        it, ro, rs, bs, ts, ws = BfItems(), BfRangeOut(), BfRows(), TxwBlocks(), TxwTxs(), TxwWits()
        for name, dt in BF_ITEM_FIELDS:
            setattr(it, name, ptr(I[name], _CT[dt]))
        for name, dt in BF_RANGE_FIELDS:
            setattr(ro, name, ptr(G[name], _CT[dt]))
        if R:
            rs.cap = len(R["item"])
            for name, dt, _ in BF_ROW_FIELDS:
                setattr(rs, name, ptr(R[name], _CT[dt]))
        if B:
            for name, dt in TXW_BLOCK_FIELDS:
                setattr(bs, name, ptr(B[name], _CT[dt]))
        if T:
            ts.cap = len(T["block"])
            for name, dt, _ in TXW_TX_FIELDS:
                setattr(ts, name, ptr(T[name], _CT[dt]))
        if W:
            ws.cap = len(W["tx"])
            for name, dt, _ in TXW_WIT_FIELDS:
                setattr(ws, name, ptr(W[name], _CT[dt]))
        rc = call(it, ro, rs, bs if B else None, ts, ws)
        if rc == E_ARG and (R or T or W) and (rs.n_rows > rs.cap or ts.n_rows > ts.cap or ws.n_wits > ws.cap):
            msg = self.L.praos_last_error(self.h)
            err = PraosError(f"praos rc={rc}: {msg.decode() if msg else ''}")
            err.needed, err.items, err.ranges = (int(rs.n_rows), int(ts.n_rows), int(ws.n_wits)), I, G
            raise err
        self.check(rc)
        nr, nt, nw = int(rs.n_rows), int(ts.n_rows), int(ws.n_wits)
        return (I, G, {k_: a[:nr] for k_, a in R.items()},
                {k_: a[:nr + 1 if k_ == "tx_first" else nr] for k_, a in B.items()},
                {k_: a[:nt + 1 if k_ == "wit_first" else nt] for k_, a in T.items()},
                {k_: a[:nw] for k_, a in W.items()}, (nr, nt, nw))

    # ---- ImmutableDB chunk validation (k_crc32.hip, praos_validate_chunk) ----
    def crc32(self, arena, off, length):
        """CRC-32 (zlib) of arena[off[i]:off[i]+len[i]] on the GPU; returns u32[n]."""
        arena, off, length = self._chunk(arena, off, length)
        hb = self.header_bytes_struct(arena, off, length)
        crc = np.zeros(len(off), np.uint32)
        self.check(self.L.praos_crc32(self.h, ctypes.byref(hb), ptr(crc, u32p)))
        return crc

    def crc32_blocks(self, b, n):
        """CRC-32 of the block spans of an upload_blocks batch (device-resident form)."""
        crc = np.zeros(n, np.uint32)
        self.check(self.L.praos_block_batch_crc32(self.h, b, ptr(crc, u32p)))
        return crc

    def verify_byron_integrity(self, arena, off, length, epoch_slots, protocol_magic):
        """verifyBlockIntegrity of stored Byron blocks and EBBs arena[off[i]:off[i]+len[i]]
        (praos_verify_byron_integrity); returns (result u8[n] of PRAOS_BLK_* bits, which u8[n] of
        BYRON_W_* bits: the failing comparisons of blockMatchesHeader)."""
        arena, off, length = self._chunk(arena, off, length)
        n = len(off)
        hb = self.header_bytes_struct(arena, off, length)
        res = np.zeros(n, np.uint8)
        which = np.zeros(n, np.uint8)
        self.check(self.L.praos_verify_byron_integrity(self.h, ctypes.byref(hb), epoch_slots, protocol_magic,
                                                       ptr(res), ptr(which)))
        return res, which

    # ---- Byron header validation: PBFT (k_pbft.hip, praos_pbft.hip) ----
    def byron_key_hash(self, keys64):
        """hashVerKey of Byron extended public keys: Blake2b-224(SHA3-256(58 40 || xpub64)); keys64
        u8[n, 64] (or bytes) -> u8[n, 28].  Host-only contexts compute it on the host."""
        k = np.ascontiguousarray(np.frombuffer(keys64, np.uint8) if isinstance(keys64, (bytes, bytearray))
                                 else keys64, dtype=np.uint8).reshape(-1, 64)
        out = np.zeros((len(k), 28), np.uint8)
        self.check(self.L.praos_byron_key_hash(self.h, ptr(k), len(k), ptr(out)))
        return out

    @staticmethod
    def pbft_params(window_size, threshold, epoch_slots, protocol_magic):
        return PbftParams(int(window_size), int(threshold), int(epoch_slots), int(protocol_magic), 0)

    @staticmethod
    def _pbft_delegs(delegs):
        """delegs: list of (genesis key hash 28, delegate key hash 28) -> u8[n, 56]"""
        d = np.zeros((len(delegs), 56), np.uint8)
        for k, (g, h) in enumerate(delegs):
            d[k, :28] = np.frombuffer(bytes(g), np.uint8)
            d[k, 28:] = np.frombuffer(bytes(h), np.uint8)
        return d

    @staticmethod
    def _pbft_out(H):
        o = PbftOut()
        for name, dt, _ in PBFT_OUT_FIELDS:
            setattr(o, name, ptr(H[name], i32p if dt is np.int32 else _CT[dt]) if name in H else None)
        return o

    def verify_pbft_headers(self, arena, off, length, is_ebb, params, delegs, delegate_hash=False):
        """The per-header half of Byron header validation (praos_verify_pbft_headers): returns a
        dict of the columns bits, gk_idx, slot, block_no, prev_hash, prev_is_genesis, header_hash
        and, with delegate_hash=True, delegate_hash (hashVerKey of each header's delegate: the
        payload of PBftNotGenesisDelegate; the fold reads gk_idx, not this column)."""
        arena, off, length = self._chunk(arena, off, length)
        n = len(off)
        ebb = np.ascontiguousarray(is_ebb, dtype=np.uint8)
        assert len(ebb) == n
        H = {name: np.zeros((n,) + shp, dt) for name, dt, shp in PBFT_OUT_FIELDS
             if delegate_hash or name != "delegate_hash"}
        hb = self.header_bytes_struct(arena, off, length)
        d = self._pbft_delegs(delegs)
        o = self._pbft_out(H)
        self.check(self.L.praos_verify_pbft_headers(self.h, ctypes.byref(hb), ptr(ebb), ctypes.byref(params), ptr(d),
                                                    len(d), ctypes.byref(o)))
        return H

    def pbft_stats(self):
        """Which kernels the last verify_pbft_headers ran (praos_pbft_stats): dict of cache (bool),
        keys_cached, cached_verifies, uncached_verifies."""
        o = np.zeros(4, np.uint32)
        self.check(self.L.praos_pbft_stats(self.h, ptr(o, u32p)))
        return {"cache": bool(o[0]), "keys_cached": int(o[1]), "cached_verifies": int(o[2]),
                "uncached_verifies": int(o[3])}

    def pbft_update_chain_dep_state(self, H, is_ebb, params, delegs, tip=None, state=()):
        """The sequential half (praos_pbft_update_chain_dep_state) over verify_pbft_headers' columns.
        tip: None (Origin) or (slot, block_no, hash32, is_ebb); state: the window's signers, oldest
        first, as (slot, genesis key hash 28).  Returns (verdict u8[n], aux u64[n], chain_stop,
        tip, state) with tip and state those at chain_stop."""
        n = len(H["bits"])
        ebb = np.ascontiguousarray(is_ebb, dtype=np.uint8)
        d = self._pbft_delegs(delegs)
        o = self._pbft_out(H)
        t = PbftTip()
        t.origin = 1
        if tip is not None:
            t.origin, t.slot, t.block_no, t.is_ebb = 0, int(tip[0]), int(tip[1]), int(bool(tip[3]))
            ctypes.memmove(t.hash, bytes(tip[2]), 32)
        state = list(state)
        cap = max(int(params.window_size), len(state), 1)
        ss = np.zeros(cap, np.uint64)
        sh = np.zeros((cap, 28), np.uint8)
        for k, (s, g) in enumerate(state):
            ss[k] = s
            sh[k] = np.frombuffer(bytes(g), np.uint8)
        st = PbftStateC(cap, len(state), ptr(ss, u64p), ptr(sh))
        verdict = np.zeros(n, np.uint8)
        aux = np.zeros(n, np.uint64)
        stop = ctypes.c_size_t(0)
        self.check(self.L.praos_pbft_update_chain_dep_state(self.h, n, ctypes.byref(o), ptr(ebb), ctypes.byref(params),
                                                            ptr(d), len(d), ctypes.byref(t), ctypes.byref(st),
                                                            ptr(verdict), ptr(aux, u64p), ctypes.byref(stop)))
        new_tip = None if t.origin else (int(t.slot), int(t.block_no), bytes(t.hash), int(t.is_ebb))
        new_state = [(int(ss[k]), bytes(sh[k])) for k in range(int(st.n))]
        return verdict, aux, int(stop.value), new_tip, new_state

    def validate_pbft_headers(self, arena, off, length, is_ebb, params, delegs, tip=None, state=()):
        """Verify, then fold, carrying the state: (columns, verdict, aux, chain_stop, tip, state)."""
        H = self.verify_pbft_headers(arena, off, length, is_ebb, params, delegs)
        v, aux, stop, tip, state = self.pbft_update_chain_dep_state(H, is_ebb, params, delegs, tip, state)
        return H, v, aux, stop, tip, state

    @staticmethod
    def pbft_state_encode(state):
        """encodePBftState of [(slot, genesis key hash 28)] (oldest first) -> bytes"""
        L = load()
        state = list(state)
        cap = max(len(state), 1)
        ss = np.zeros(cap, np.uint64)
        sh = np.zeros((cap, 28), np.uint8)
        for k, (s, g) in enumerate(state):
            ss[k] = s
            sh[k] = np.frombuffer(bytes(g), np.uint8)
        st = PbftStateC(cap, len(state), ptr(ss, u64p), ptr(sh))
        ln = ctypes.c_size_t(0)
        L.praos_pbft_state_encode(ctypes.byref(st), None, 0, ctypes.byref(ln))
        out = np.zeros(max(ln.value, 1), np.uint8)
        if L.praos_pbft_state_encode(ctypes.byref(st), ptr(out), len(out), ctypes.byref(ln)) != 0:
            raise PraosError("praos_pbft_state_encode failed")
        return bytes(out[:ln.value])

    @staticmethod
    def pbft_state_decode(data):
        """decodePBftState -> [(slot, genesis key hash 28)], oldest first"""
        L = load()
        buf = np.frombuffer(bytes(data), np.uint8).copy()
        cap = max(len(buf), 1)                     # every signer takes at least one byte
        ss = np.zeros(cap, np.uint64)
        sh = np.zeros((cap, 28), np.uint8)
        st = PbftStateC(cap, 0, ptr(ss, u64p), ptr(sh))
        if L.praos_pbft_state_decode(ptr(buf) if len(buf) else None, len(buf), ctypes.byref(st)) != 0:
            raise PraosError("praos_pbft_state_decode: not a PBftState")
        return [(int(ss[k]), bytes(sh[k])) for k in range(int(st.n))]

    def validate_chunk(self, chunk, expected_crc=None, block_off=None, slots_per_kes_period=129600, cap=None,
                       byron=None):
        """parseChunkFile over one chunk file's bytes (praos_validate_chunk).  expected_crc: the
        secondary index's checksums in order (None: index missing); block_off: its blockOffsets, a
        hint.  Returns a dict: outcome (CHUNK_*), integrity_bits, blocks, checked, truncate_at,
        rescanned_from, err_slot, err_hash, expected_prev, actual_prev, actual_prev_is_genesis, and
        per yielded block entries (bytes, 56 each), block_no, prev_hash, prev_is_genesis, integrity.
        cap: capacity of the output buffers (default: grown until the blocks fit); a smaller one
        raises PraosError with .needed set.
        byron: None (a Byron item ends the parse with UNSUPPORTED), or (epoch_slots,
        protocol_magic): praos_validate_chunk_cfg decodes and checks Byron blocks and EBBs too, an
        EBB's entry carries its epoch number, and the dict also has is_ebb per yielded block."""
        cfg = None
        if byron is not None:
            cfg = ChunkCfg(slots_per_kes_period, int(byron[0]), int(byron[1]), 0)
            if cfg.byron_epoch_slots == 0:
                raise ValueError("byron epoch_slots must be positive")
        data = np.ascontiguousarray(np.frombuffer(chunk, np.uint8) if isinstance(chunk, (bytes, bytearray))
                                    else chunk, dtype=np.uint8)
        ch = Chunk()
        ch.bytes, ch.bytes_len = ptr(data), len(data)
        ecrc = None if expected_crc is None else np.ascontiguousarray(expected_crc, dtype=np.uint32)
        boff = None if block_off is None else np.ascontiguousarray(block_off, dtype=np.uint64)
        ch.n_expected = 0 if ecrc is None else len(ecrc)
        ch.expected_crc = ptr(ecrc, u32p) if ch.n_expected else None
        if boff is not None and len(boff) != ch.n_expected:
            raise ValueError("block_off must have one offset per expected_crc entry")
        ch.block_off = ptr(boff, u64p) if (boff is not None and ch.n_expected) else None
        grow = cap is None
        cap = max(ch.n_expected, 64) if grow else cap
        while True:
            ent = np.zeros(cap * CHUNK_ENTRY_SIZE, np.uint8)
            bno = np.zeros(cap, np.uint64)
            prev = np.zeros((cap, 32), np.uint8)
            gen = np.zeros(cap, np.uint8)
            integ = np.zeros(cap, np.int8)
            out = ChunkOut()
            out.cap, out.entries, out.block_no, out.prev_hash = cap, ptr(ent), ptr(bno, u64p), ptr(prev)
            out.prev_is_genesis, out.integrity = ptr(gen), ptr(integ, ctypes.POINTER(ctypes.c_int8))
            res = ChunkResult()
            ebb = np.zeros(cap, np.uint8)
            if cfg is None:
                rc = self.L.praos_validate_chunk(self.h, ctypes.byref(ch), slots_per_kes_period, ctypes.byref(res),
                                                 ctypes.byref(out))
            else:
                rc = self.L.praos_validate_chunk_cfg(self.h, ctypes.byref(ch), ctypes.byref(cfg), ctypes.byref(res),
                                                     ctypes.byref(out), ptr(ebb))
            if rc == E_ARG and res.blocks > cap:
                if grow:
                    cap = int(res.blocks)
                    continue
                msg = self.L.praos_last_error(self.h)
                err = PraosError(f"praos rc={rc}: {msg.decode() if msg else ''}")
                err.needed = int(res.blocks)
                raise err
            self.check(rc)
            break
        y = int(res.blocks)
        extra = {} if cfg is None else {"is_ebb": ebb[:y].copy()}
        return {**extra, "outcome": int(res.outcome), "integrity_bits": int(res.integrity_bits), "blocks": y,
                "checked": int(res.checked), "truncate_at": int(res.truncate_at),
                "rescanned_from": int(res.rescanned_from), "err_slot": int(res.err_slot),
                "err_hash": bytes(res.err_hash), "expected_prev": bytes(res.expected_prev),
                "actual_prev": bytes(res.actual_prev), "actual_prev_is_genesis": int(res.actual_prev_is_genesis),
                "entries": ent[:y * CHUNK_ENTRY_SIZE].tobytes(), "block_no": bno[:y].copy(),
                "prev_hash": prev[:y].copy(), "prev_is_genesis": gen[:y].copy(), "integrity": integ[:y].copy()}

    def upload_blocks(self, arena, off, length):
        arena, off, length = self._chunk(arena, off, length)
        hb = self.header_bytes_struct(arena, off, length)
        b = self.L.praos_block_batch_upload(self.h, ctypes.byref(hb))
        if not b:
            raise RuntimeError("praos_block_batch_upload: " + self.L.praos_last_error(self.h).decode())
        return b

    def run_blocks(self, b, slots_per_kes_period):
        self.check(self.L.praos_block_batch_run(self.h, b, slots_per_kes_period))

    def download_blocks(self, b, n):
        res = np.zeros(n, np.uint8)
        bh = np.zeros((n, 32), np.uint8)
        self.check(self.L.praos_block_batch_download(self.h, b, ptr(res), ptr(bh)))
        return res, bh

    def upload_bytes(self, arena, off, length):
        arena, off, length = self._chunk(arena, off, length)
        hb = self.header_bytes_struct(arena, off, length)
        b = self.L.praos_batch_upload_bytes(self.h, ctypes.byref(hb))
        if not b:
            self.check(-3)
        return b

    def host_register(self, arr):
        """Page-locks a numpy array's memory for this context (praos_host_register): uploads
        from it move by direct DMA.  Keep the array alive until host_unregister."""
        self.check(self.L.praos_host_register(self.h, arr.ctypes.data, arr.nbytes))

    def host_unregister(self, arr):
        self.check(self.L.praos_host_unregister(self.h, arr.ctypes.data))

    def upload_tpraos_bytes(self, arena, off, length):
        """Stored TPraos headers (BHeader) as a resident batch (praos_batch_upload_tpraos_bytes);
        every praos_batch_run decodes them on the device and runs the TPraos kernels."""
        arena, off, length = self._chunk(arena, off, length)
        hb = self.header_bytes_struct(arena, off, length)
        b = self.L.praos_batch_upload_tpraos_bytes(self.h, ctypes.byref(hb))
        if not b:
            self.check(-3)
        return b

    def download_tpraos(self, b, n):
        o = {"bits": np.zeros(n, np.uint16), "pool_idx": np.zeros(n, np.int32),
             "beta_eta": np.zeros((n, 64), np.uint8), "beta_leader": np.zeros((n, 64), np.uint8),
             "nonce": np.zeros((n, 32), np.uint8)}
        to = TPOut()
        to.bits, to.pool_idx = ptr(o["bits"], u16p), ptr(o["pool_idx"], i32p)
        to.beta_eta, to.beta_leader, to.nonce = ptr(o["beta_eta"]), ptr(o["beta_leader"]), ptr(o["nonce"])
        self.check(self.L.praos_batch_download_tpraos(self.h, b, ctypes.byref(to)))
        return o

    def batch_decode(self, b):
        self.check(self.L.praos_batch_decode(self.h, b))

    @staticmethod
    def nonce_array(etas):
        arr = (Nonce * max(1, len(etas)))()
        for k, e in enumerate(etas):
            arr[k].neutral = int(e is None)
            if e is not None:
                ctypes.memmove(arr[k].hash, bytes(e), 32)
        return arr

    def set_nonces(self, b, etas, eta_idx):
        """praos_batch_set_nonces: header i of batch b is verified under etas[eta_idx[i]]
        (None = NeutralNonce)."""
        idx = np.ascontiguousarray(eta_idx, dtype=np.uint8)
        self.check(self.L.praos_batch_set_nonces(self.h, b, self.nonce_array(etas), len(etas), ptr(idx)))

    def download_decoded(self, b, n):
        D, d = self.alloc_decoded(n)
        self.check(self.L.praos_batch_download_decoded(self.h, b, ctypes.byref(d)))
        return D

    def update_chain_dep_state(self, H, crypto, prev_hash, state: dict, epoch_info, prev_is_genesis=None,
                               envelope=None, etas=None, eta_idx=None):
        """state: dict(last_slot (None = Origin), counters {hash28: n}, evolving, candidate, epoch_nonce,
        lab, leb) with nonces None (Neutral) or 32 bytes; updated in place.  epoch_info: (base_slot,
        base_no, length, stability_window).  envelope (praos_validate_headers): dict(block_no u64[n],
        header_hash u8[n,32], header_size u32[n], body_size u32[n], tip (None = Origin, or (slot,
        block_no, hash32)), max_major_pv, lv_prot_major, max_header_size, max_body_size); its "tip" is
        updated in place.  etas / eta_idx: the per-header nonces the crypto ran under
        (praos_validate_headers_nonces).  Returns (verdict u8[n], chain_stop, processed)."""
        n = len(H["slot"])
        hs = self.headers_struct(H)
        os_ = self.out_struct(crypto)
        keys = list(state["counters"].keys())
        cap = len(keys) + n
        hk = np.zeros(28 * max(cap, 1), np.uint8)
        cv = np.zeros(max(cap, 1), np.uint64)
        for k, key in enumerate(keys):
            hk[28 * k:28 * k + 28] = np.frombuffer(key, np.uint8)
            cv[k] = state["counters"][key]
        st = ChainState()
        st.last_slot_origin = int(state["last_slot"] is None)
        st.last_slot = state["last_slot"] or 0
        st.counter_hash28, st.counter, st.m, st.cap = ptr(hk), ptr(cv, u64p), len(keys), cap

        def setn(dst, v):
            dst.neutral = int(v is None)
            if v is not None:
                ctypes.memmove(dst.hash, v, 32)

        def getn(src):
            return None if src.neutral else bytes(src.hash)
        for a, b in (("evolving", "evolving"), ("candidate", "candidate"), ("epoch_nonce", "epoch_nonce"),
                     ("lab", "lab"), ("last_epoch_block", "leb")):
            setn(getattr(st, a), state[b])
        ei = EpochInfo(*epoch_info)
        ph = np.ascontiguousarray(prev_hash, dtype=np.uint8)
        pg = None if prev_is_genesis is None else np.ascontiguousarray(prev_is_genesis, dtype=np.uint8)
        verdict = np.zeros(n, np.uint8)
        stop, done = ctypes.c_size_t(0), ctypes.c_size_t(0)
        E = None
        if envelope is not None:
            E = Envelope()
            arrs = {k: np.ascontiguousarray(envelope[k], dtype=dt) for k, dt in
                    (("block_no", np.uint64), ("header_hash", np.uint8), ("header_size", np.uint32),
                     ("body_size", np.uint32))}
            E.block_no, E.header_hash = ptr(arrs["block_no"], u64p), ptr(arrs["header_hash"])
            E.header_size, E.body_size = ptr(arrs["header_size"], u32p), ptr(arrs["body_size"], u32p)
            tip = envelope["tip"]
            E.tip_is_origin = int(tip is None)
            if tip is not None:
                E.tip_slot, E.tip_block_no = tip[0], tip[1]
                ctypes.memmove(E.tip_hash, bytes(tip[2]), 32)
            for k in ("max_major_pv", "lv_prot_major", "max_header_size", "max_body_size"):
                setattr(E, k, envelope[k])
        if etas is not None:
            idx = np.ascontiguousarray(eta_idx, dtype=np.uint8)
            self.check(self.L.praos_validate_headers_nonces(
                self.h, ctypes.byref(hs), ptr(ph), ptr(pg) if pg is not None else None, ctypes.byref(os_),
                ctypes.byref(E) if E is not None else None, ctypes.byref(ei), ctypes.byref(st),
                self.nonce_array(etas), len(etas), ptr(idx), ptr(verdict), ctypes.byref(stop), ctypes.byref(done)))
            if envelope is not None:
                envelope["tip"] = None if E.tip_is_origin else (int(E.tip_slot), int(E.tip_block_no),
                                                                bytes(E.tip_hash))
        elif envelope is None:
            self.check(self.L.praos_update_chain_dep_state(self.h, ctypes.byref(hs), ptr(ph),
                                                           ptr(pg) if pg is not None else None, ctypes.byref(os_),
                                                           ctypes.byref(ei), ctypes.byref(st), ptr(verdict),
                                                           ctypes.byref(stop), ctypes.byref(done)))
        else:
            E = Envelope()
            arrs = {k: np.ascontiguousarray(envelope[k], dtype=dt) for k, dt in
                    (("block_no", np.uint64), ("header_hash", np.uint8), ("header_size", np.uint32),
                     ("body_size", np.uint32))}
            E.block_no, E.header_hash = ptr(arrs["block_no"], u64p), ptr(arrs["header_hash"])
            E.header_size, E.body_size = ptr(arrs["header_size"], u32p), ptr(arrs["body_size"], u32p)
            tip = envelope["tip"]
            E.tip_is_origin = int(tip is None)
            if tip is not None:
                E.tip_slot, E.tip_block_no = tip[0], tip[1]
                ctypes.memmove(E.tip_hash, bytes(tip[2]), 32)
            for k in ("max_major_pv", "lv_prot_major", "max_header_size", "max_body_size"):
                setattr(E, k, envelope[k])
            self.check(self.L.praos_validate_headers(self.h, ctypes.byref(hs), ptr(ph),
                                                     ptr(pg) if pg is not None else None, ctypes.byref(os_),
                                                     ctypes.byref(E), ctypes.byref(ei), ctypes.byref(st),
                                                     ptr(verdict), ctypes.byref(stop), ctypes.byref(done)))
            envelope["tip"] = None if E.tip_is_origin else (int(E.tip_slot), int(E.tip_block_no), bytes(E.tip_hash))
        state["last_slot"] = None if st.last_slot_origin else int(st.last_slot)
        state["counters"] = {bytes(hk[28 * k:28 * k + 28]): int(cv[k]) for k in range(st.m)}
        for a, b in (("evolving", "evolving"), ("candidate", "candidate"), ("epoch_nonce", "epoch_nonce"),
                     ("lab", "lab"), ("last_epoch_block", "leb")):
            state[b] = getn(getattr(st, a))
        return verdict, stop.value, done.value

    def replay_immutable(self, path, pools, params: Params, epoch_info, state: dict, envelope: dict,
                         batch_max=1 << 16, verdicts_cap=0, counter_cap=1 << 16, tpraos=False, extra_entropy=None):
        """praos_replay_immutable over an ImmutableDB directory.  state (chain state dict, as
        update_chain_dep_state) and envelope (limits + "tip") are updated in place.
        Returns (stats dict, verdict u8[verdicts_cap]); tpraos=True (praos_replay_immutable_tpraos,
        extra_entropy None = NeutralNonce) returns (stats, verdict, failures u16[verdicts_cap])."""
        fn = self.L.praos_replay_immutable_tpraos if tpraos else self.L.praos_replay_immutable
        return _replay(fn, self.h, self.check, path, pools, params, epoch_info, state, envelope, batch_max,
                       verdicts_cap, counter_cap, tpraos, extra_entropy)

    def replay_immutable_views(self, path, views, params: Params, epoch_info, state: dict, envelope: dict,
                               batch_max=1 << 16, verdicts_cap=0, counter_cap=1 << 16):
        """praos_replay_immutable_views: views = [(first_epoch, pools, {lv_prot_major, max_header_size,
        max_body_size})] sorted by first_epoch, a ledger view per epoch range; otherwise as
        replay_immutable (envelope's limits are not read)."""
        return _replay_views(self.L.praos_replay_immutable_views, self.h, self.check, path, views, params, epoch_info,
                             state, envelope, batch_max, verdicts_cap, counter_cap)

    def apply_batch(self, H, crypto, counters=None):
        """counters: dict hash28 -> int.  Returns (verdict u8[n], chain_stop, counters_out)."""
        n = len(H["slot"])
        hs = self.headers_struct(H)
        os_ = self.out_struct(crypto)
        verdict = np.zeros(n, np.uint8)
        stop = ctypes.c_size_t(0)
        cs = None
        keys = list(counters.keys()) if counters else []
        hk = np.frombuffer(b"".join(keys), dtype=np.uint8).copy() if keys else np.zeros(28, np.uint8)
        cv = np.array([counters[k] for k in keys], dtype=np.uint64) if keys else np.zeros(1, np.uint64)
        if counters is not None:
            cs = Counters()
            cs.hash28 = ptr(hk)
            cs.counter = ptr(cv, u64p)
            cs.m = len(keys)
        self.check(self.L.praos_apply_batch(self.h, ctypes.byref(hs), ctypes.byref(os_),
                                            ctypes.byref(cs) if cs is not None else None, ptr(verdict),
                                            ctypes.byref(stop)))
        out_counters = {k: int(cv[i]) for i, k in enumerate(keys)}
        return verdict, stop.value, out_counters

    # ---- single primitives ----
    def verify_ocert(self, cold_vk, hot_vk, n_arr, c0_arr, sig):
        n = len(n_arr)
        ok = np.zeros(n, np.uint8)
        self.check(self.L.praos_verify_ocert(self.h, n, ptr(cold_vk), ptr(hot_vk), ptr(n_arr, u64p),
                                             ptr(c0_arr, u64p), ptr(sig), ptr(ok)))
        return ok

    def verify_kes(self, vk, period, sig, msgs):
        n = len(period)
        lens = np.array([len(m) for m in msgs], dtype=np.uint32)
        offs = np.zeros(n, np.uint64)
        if n > 1:
            offs[1:] = np.cumsum(lens[:-1].astype(np.uint64))
        blob = np.frombuffer(b"".join(msgs) + b"\0" * 8, dtype=np.uint8).copy()
        res = np.zeros(n, np.uint8)
        self.check(self.L.praos_verify_kes(self.h, n, ptr(vk), ptr(period, u32p), ptr(sig), ptr(offs, u64p),
                                           ptr(lens, u32p), ptr(blob), len(blob) - 8, ptr(res)))
        return res

    def verify_vrf(self, vk, proof, alpha):
        n = len(vk)
        ok = np.zeros(n, np.uint8)
        beta = np.zeros((n, 64), np.uint8)
        self.check(self.L.praos_verify_vrf(self.h, n, ptr(vk), ptr(proof), ptr(alpha), ptr(ok), ptr(beta)))
        return ok, beta

    def check_leader(self, leader_be, sigma_fp, params: Params):
        n = len(leader_be)
        res = np.zeros(n, np.uint8)
        self.check(self.L.praos_check_leader(self.h, n, ptr(leader_be), ptr(sigma_fp), ctypes.byref(params),
                                             ptr(res)))
        return res

    def leader_schedule(self, seed: bytes, sigma_fp, params: Params, eta0, first_slot, nslots, tpraos=False):
        """First-leader-wins forger per slot (praos_leader_schedule): int32[nslots], -1 = empty slot.
        sigma_fp: per-pool Fixed E34 stake (ints), in forger order."""
        npools = len(sigma_fp)
        sig = np.frombuffer(b"".join(int(x).to_bytes(16, "little") for x in sigma_fp), np.uint8).copy()
        sd = np.frombuffer(bytes(seed), np.uint8).copy()
        e = None if eta0 is None else np.frombuffer(bytes(eta0), np.uint8).copy()
        out = np.zeros(nslots, np.int32)
        self.check(self.L.praos_leader_schedule(self.h, ptr(sd), npools, ptr(sig), ctypes.byref(params), ptr(e),
                                                first_slot, nslots, int(bool(tpraos)), ptr(out, i32p)))
        return out

    def synthesize(self, n, npools, params: Params, eta0, seed: bytes, first_slot=0, slot_stride=20,
                   body_len=397, corrupt_per_10000=0, nkes=0, tpraos=False, body_hash=None, schedule=None,
                   block_no0=0, link=False, prev0=None, corrupt_fields=0):
        """schedule: (slots u64[n], pools u32[n]) from leader_schedule (a leader-valid chain), or None
        (evenly spaced slots, pools by hash: not leader-valid).  link=True chains the headers
        (prevHash = headerHash of the previous header; header 0: prev0, None = GenesisHash) and
        returns the header hashes in H["header_hash"]."""
        sp = SynthParams()
        if link:
            hh_out = np.zeros((n, 32), np.uint8)
            sp.link_prev, sp.header_hash = 1, ptr(hh_out)
            if prev0 is not None:
                p0 = np.frombuffer(bytes(prev0), np.uint8).copy()
                sp.prev0 = ptr(p0)
        if body_hash is not None:   # n*32 hbBodyHash values for the CBOR bodies (body_len=0)
            body_hash = np.ascontiguousarray(body_hash, dtype=np.uint8).reshape(n, 32)
            sp.body_hash = ptr(body_hash)
        if schedule is not None:
            ss = np.ascontiguousarray(schedule[0], dtype=np.uint64)
            sq = np.ascontiguousarray(schedule[1], dtype=np.uint32)
            assert len(ss) == n and len(sq) == n
            sp.sched_slot, sp.sched_pool, sp.block_no0 = ptr(ss, u64p), ptr(sq, u32p), block_no0
        sp.n = n
        sp.npools = npools
        sp.first_slot = first_slot
        sp.slot_stride = slot_stride
        sp.body_len = body_len
        sp.corrupt_per_10000 = corrupt_per_10000
        sp.corrupt_fields = corrupt_fields
        sp.nkes = nkes
        ctypes.memmove(sp.seed, seed, 32)
        bstride = (body_len + 7) & ~7 if body_len else (TP_SIGNED_STRIDE if tpraos else SIGNED_STRIDE)
        H = {"slot": np.zeros(n, np.uint64), "cold_vk": np.zeros((n, 32), np.uint8),
             "vrf_vk": np.zeros((n, 32), np.uint8), "vrf_out": np.zeros((n, 64), np.uint8),
             "vrf_proof": np.zeros((n, 80), np.uint8), "hot_vk": np.zeros((n, 32), np.uint8),
             "ocert_n": np.zeros(n, np.uint64), "ocert_c0": np.zeros(n, np.uint64),
             "ocert_sig": np.zeros((n, 64), np.uint8), "kes_sig": np.zeros((n, 448), np.uint8),
             "body_off": np.zeros(n, np.uint64), "body_len": np.zeros(n, np.uint32),
             "body_bytes": np.zeros(bstride * n + 8, np.uint8)}
        corrupted = np.zeros(n, np.uint8)
        pools = (Pool * npools)()
        e = None
        if eta0 is not None:
            eb = np.frombuffer(bytes(eta0), dtype=np.uint8).copy()
            e = ptr(eb)
        common = (self.h, ctypes.byref(sp), ctypes.byref(params), e, pools, ptr(H["slot"], u64p), ptr(H["cold_vk"]),
                  ptr(H["vrf_vk"]), ptr(H["vrf_out"]), ptr(H["vrf_proof"]), ptr(H["hot_vk"]),
                  ptr(H["ocert_n"], u64p), ptr(H["ocert_c0"], u64p), ptr(H["ocert_sig"]), ptr(H["kes_sig"]),
                  ptr(H["body_off"], u64p), ptr(H["body_len"], u32p), ptr(H["body_bytes"]))
        if tpraos:
            H["leader_out"] = np.zeros((n, 64), np.uint8)
            H["leader_proof"] = np.zeros((n, 80), np.uint8)
            self.check(self.L.praos_synthesize_tpraos(*common, ptr(H["leader_out"]), ptr(H["leader_proof"]),
                                                      ptr(corrupted)))
        else:
            self.check(self.L.praos_synthesize(*common, ptr(corrupted)))
        H["body_bytes"] = H["body_bytes"][:bstride * n]
        if link:
            H["header_hash"] = hh_out
        pool_list = [(bytes(p.hash28), bytes(p.vrf_hash32)) for p in pools]
        return H, pool_list, corrupted

    # ---- self tests ----
    def debug_fe(self, op, a, b=None):
        n = len(a)
        r = np.zeros((n, 32), np.uint8)
        self.check(self.L.praos_debug_fe(self.h, op, n, ptr(a), ptr(b if b is not None else a), ptr(r)))
        return r

    def debug_sha512(self, prefix, msgs):
        n = len(msgs)
        lens = np.array([len(m) for m in msgs], dtype=np.uint32)
        offs = np.zeros(n, np.uint64)
        if n > 1:
            offs[1:] = np.cumsum(lens[:-1].astype(np.uint64))
        blob = np.frombuffer(b"".join(msgs) + b"\0" * 8, dtype=np.uint8).copy()
        out = np.zeros((n, 64), np.uint8)
        self.check(self.L.praos_debug_sha512(self.h, n, ptr(prefix), ptr(offs, u64p), ptr(lens, u32p), ptr(blob),
                                             len(blob) - 8, ptr(out)))
        return out

    def debug_blake2b(self, in64):
        out = np.zeros((len(in64), 32), np.uint8)
        self.check(self.L.praos_debug_blake2b(self.h, len(in64), ptr(in64), ptr(out)))
        return out

    def debug_sc_reduce(self, in64):
        out = np.zeros((len(in64), 32), np.uint8)
        self.check(self.L.praos_debug_sc_reduce(self.h, len(in64), ptr(in64), ptr(out)))
        return out

    def debug_decode(self, in32):
        n = len(in32)
        out = np.zeros((n, 32), np.uint8)
        ok = np.zeros(n, np.uint8)
        self.check(self.L.praos_debug_decode(self.h, n, ptr(in32), ptr(out), ptr(ok)))
        return out, ok

    def debug_scalarmult_base(self, s):
        out = np.zeros((len(s), 32), np.uint8)
        self.check(self.L.praos_debug_scalarmult_base(self.h, len(s), ptr(s), ptr(out)))
        return out

    def debug_leader(self, leader_be, x_raw16):
        n = len(leader_be)
        res = np.zeros(n, np.uint8)
        it = np.zeros(n, np.int32)
        self.check(self.L.praos_debug_leader(self.h, n, ptr(leader_be), ptr(x_raw16), ptr(res), ptr(it, i32p)))
        return res, it

    def debug_leader512(self, leader_be64, x_raw16):
        n = len(leader_be64)
        res = np.zeros(n, np.uint8)
        it = np.zeros(n, np.int32)
        self.check(self.L.praos_debug_leader512(self.h, n, ptr(leader_be64), ptr(x_raw16), ptr(res), ptr(it, i32p)))
        return res, it

    def debug_hash_to_curve(self, pk, alpha):
        out = np.zeros((len(pk), 32), np.uint8)
        self.check(self.L.praos_debug_hash_to_curve(self.h, len(pk), ptr(pk), ptr(alpha), ptr(out)))
        return out

    def debug_fe_multi(self, op, ins):
        """ins (n, 8, 32): a1 b1 .. a4 b4 -> (n, 4, 32); op 0..4 (fe_mul2, fe_sq2, fe_mul3, fe_mul4, fe_sq4), | 8 aliased"""
        ins = np.ascontiguousarray(ins, np.uint8)
        n = len(ins)
        out = np.zeros((n, 4, 32), np.uint8)
        self.check(self.L.praos_debug_fe_multi(self.h, op, n, ptr(ins), ptr(out)))
        return out

    def debug_ge(self, build, op, p, q=None):
        """p, q (n, 128) raw coordinates -> (n, 128); the ops and layouts are in praos_hip.h"""
        p = np.ascontiguousarray(p, np.uint8)
        q = np.ascontiguousarray(q, np.uint8) if q is not None else np.zeros_like(p)
        n = len(p)
        out = np.zeros((n, 128), np.uint8)
        self.check(self.L.praos_debug_ge(self.h, build, op, n, ptr(p), ptr(q), ptr(out)))
        return out

    def debug_msm(self, variant, build, P, sp, Q=None, sq=None, sb=None):
        """P, Q (n, 32) encodings, sp, sq, sb (n, 32) scalars -> (n, 32) encodings of the variant's result"""
        n = len(P)
        a = [np.ascontiguousarray(x, np.uint8) if x is not None else None for x in (P, Q, sp, sq, sb)]
        out = np.zeros((n, 32), np.uint8)
        self.check(self.L.praos_debug_msm(self.h, variant, build, n, *[ptr(x) if x is not None else None for x in a],
                                          ptr(out)))
        return out

    def debug_hash_bytes(self, kind, arena, off, length, aux=None, parts=None):
        """The stored-byte hashes on a caller's arena (kinds and tables: praos_hip.h).  arena: bytes;
        off, length: the item table; aux: (n, 4) npre / pre bytes (kind 1) or nseg (kind 2);
        parts: (n_parts, 2) uint64 (kinds 3, 4).  Returns (items, 32) digests, (n, 64) for kind 3."""
        a = np.frombuffer(bytes(arena), np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        length = np.ascontiguousarray(length, np.uint32)
        aux = np.ascontiguousarray(aux, np.uint8) if aux is not None else None
        parts = np.ascontiguousarray(parts, np.uint64) if parts is not None else None
        n = len(aux) if kind == 2 else len(off)
        out = np.zeros((4 * n if kind == 2 else n, 64 if kind == 3 else 32), np.uint8)
        self.check(self.L.praos_debug_hash_bytes(self.h, kind, n, ptr(a) if len(a) else None, len(a), ptr(off, u64p),
                                                 ptr(length, u32p), ptr(aux), ptr(parts, u64p),
                                                 len(parts) if parts is not None else 0, ptr(out)))
        return out

    def debug_int(self, op, a, b=None, c=None):
        """One integer routine per item (ops: praos_hip.h).  a, b, c (n, 32) uint8, eight LE words
        each -> (n, 32)."""
        a, b, c = [np.ascontiguousarray(x, np.uint8) if x is not None else None for x in (a, b, c)]
        out = np.zeros((len(a), 32), np.uint8)
        self.check(self.L.praos_debug_int(self.h, op, len(a), ptr(a), ptr(b), ptr(c), ptr(out)))
        return out


    def debug_span_equal(self, arena, a_off, b_off, length):
        """The BlockFetch dedup's compare kernel alone: u8[n], 1 where arena[a_off[i]:+len[i]] ==
        arena[b_off[i]:+len[i]] (praos_debug_span_equal; one wave per pair)."""
        a = np.frombuffer(bytes(arena), np.uint8)
        a_off = np.ascontiguousarray(a_off, np.uint64)
        b_off = np.ascontiguousarray(b_off, np.uint64)
        length = np.ascontiguousarray(length, np.uint32)
        out = np.zeros(len(a_off), np.uint8)
        self.check(self.L.praos_debug_span_equal(self.h, len(a_off), ptr(a) if len(a) else None, len(a),
                                                 ptr(a_off, u64p), ptr(b_off, u64p), ptr(length, u32p), ptr(out)))
        return out

    def debug_row_set(self, flag, tag=None, key=None, tag_mask=0xffffffff, dedup=True, limit=None):
        """The row set of the wire calls alone (praos_debug_row_set): (item_row u32[n], n_rows).
        dedup: items with flag 0 and a tag below 32 in tag_mask classed by (tag, 32-byte key);
        without it every item with flag 0 below `limit` its own class.  Rows in order of first
        appearance; 0xFFFFFFFF (PRAOS_NO_ROW) for an item in no class."""
        flag = np.ascontiguousarray(flag, np.uint8)
        n = len(flag)
        tag = np.ascontiguousarray(tag if tag is not None else np.zeros(n), np.uint8)
        key = np.ascontiguousarray(key if key is not None else np.zeros((n, 32)), np.uint8).reshape(n, 32)
        lim = None if limit is None else np.array([limit], np.uint32)
        rows, total = np.zeros(n, np.uint32), np.zeros(1, np.uint32)
        self.check(self.L.praos_debug_row_set(self.h, n, ptr(flag), ptr(tag), ptr(key), tag_mask, 1 if dedup else 0,
                                              None if lim is None else ptr(lim, u32p), ptr(rows, u32p),
                                              ptr(total, u32p)))
        return rows, int(total[0])

class Group:
    """praos_group: one context per listed device (repeats allowed), batches split into
    contiguous shards run concurrently, outputs gathered in place (include/praos_hip.h)."""

    def __init__(self, devices):
        self.L = load()
        arr = np.ascontiguousarray(devices, dtype=np.int32)
        self.g = self.L.praos_group_open(ptr(arr, i32p), len(arr))
        if not self.g:
            raise PraosError(f"praos_group_open({list(devices)}) failed")
        self.size = self.L.praos_group_size(self.g)

    def close(self):
        if self.g:
            self.L.praos_group_close(self.g)
            self.g = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def check(self, rc):
        if rc != 0:
            msg = self.L.praos_group_last_error(self.g)
            raise PraosError(f"praos group rc={rc}: {msg.decode() if msg else ''}")

    def member(self, k):
        """A Context view of member k (not owned: closing the group closes it)."""
        c = Context.__new__(Context)
        c.L, c.h, c._keep = self.L, self.L.praos_group_ctx(self.g, k), []
        return c

    def set_option(self, opt, value):
        self.check(self.L.praos_group_set_option(self.g, opt, value))

    def set_epoch(self, eta0, pools, params: Params):
        arr = Context.pool_array(pools)
        e = None
        if eta0 is not None:
            eb = np.frombuffer(bytes(eta0), dtype=np.uint8).copy()
            e = ptr(eb)
        self.check(self.L.praos_group_set_epoch(self.g, e, arr, len(pools), ctypes.byref(params)))

    def verify_headers(self, H):
        n = len(H["slot"])
        hs = Context.headers_struct(H)
        o = Context.alloc_out(n)
        os_ = Context.out_struct(o)
        self.check(self.L.praos_group_verify_headers(self.g, ctypes.byref(hs), ctypes.byref(os_)))
        return o

    def verify_header_bytes(self, arena, off, length, decoded=False):
        arena, off, length = Context._chunk(arena, off, length)
        n = len(off)
        hb = Context.header_bytes_struct(arena, off, length)
        o = Context.alloc_out(n)
        os_ = Context.out_struct(o)
        D, d = Context.alloc_decoded(n) if decoded else (None, None)
        self.check(self.L.praos_group_verify_header_bytes(self.g, ctypes.byref(hb), ctypes.byref(os_),
                                                          ctypes.byref(d) if decoded else None))
        return (o, D) if decoded else o

    def verify_tpraos_headers(self, H):
        th = Context.tp_headers_struct(H)
        o, to = Context.tp_out(len(H["slot"]))
        self.check(self.L.praos_group_verify_tpraos_headers(self.g, ctypes.byref(th), ctypes.byref(to)))
        return o

    def set_overlay(self, d, f, epoch_base_slot, epoch_length, gen_delegs):
        """praos_group_set_overlay (Context.set_overlay on every member)."""
        if d is None:
            self.check(self.L.praos_group_set_overlay(self.g, None))
            return
        arr = (GenDeleg * max(1, len(gen_delegs)))()
        for k, (g, dl, v) in enumerate(gen_delegs):
            ctypes.memmove(arr[k].genesis_hash28, bytes(g), 28)
            ctypes.memmove(arr[k].delegate_hash28, bytes(dl), 28)
            ctypes.memmove(arr[k].vrf_hash32, bytes(v), 32)
        ov = Overlay(d.numerator, d.denominator, f.numerator, f.denominator, epoch_base_slot, epoch_length,
                     ctypes.cast(arr, ctypes.POINTER(GenDeleg)), len(gen_delegs))
        self.check(self.L.praos_group_set_overlay(self.g, ctypes.byref(ov)))

    def host_register(self, a):
        """praos_group_host_register: page-lock a numpy array once for every member."""
        assert a.flags["C_CONTIGUOUS"] and a.nbytes > 0
        self.check(self.L.praos_group_host_register(self.g, a.ctypes.data, a.nbytes))

    def host_unregister(self, a):
        self.check(self.L.praos_group_host_unregister(self.g, a.ctypes.data))

    def replay_immutable(self, path, pools, params: Params, epoch_info, state: dict, envelope: dict,
                         batch_max=1 << 16, verdicts_cap=0, counter_cap=1 << 16, tpraos=False, extra_entropy=None):
        """praos_group_replay_immutable[_tpraos]: Context.replay_immutable over the group's members."""
        fn = self.L.praos_group_replay_immutable_tpraos if tpraos else self.L.praos_group_replay_immutable
        return _replay(fn, self.g, self.check, path, pools, params, epoch_info, state, envelope, batch_max,
                       verdicts_cap, counter_cap, tpraos, extra_entropy)

    def verify_block_integrity(self, arena, off, length, slots_per_kes_period):
        """praos_group_verify_block_integrity: Context.verify_block_integrity sharded over the members."""
        arena, off, length = Context._chunk(arena, off, length)
        n = len(off)
        hb = Context.header_bytes_struct(arena, off, length)
        res = np.zeros(n, np.uint8)
        bh = np.zeros((n, 32), np.uint8)
        self.check(self.L.praos_group_verify_block_integrity(self.g, ctypes.byref(hb), slots_per_kes_period,
                                                             ptr(res), ptr(bh)))
        return res, bh

    def replay_immutable_views(self, path, views, params: Params, epoch_info, state: dict, envelope: dict,
                               batch_max=1 << 16, verdicts_cap=0, counter_cap=1 << 16):
        """praos_group_replay_immutable_views: Context.replay_immutable_views over the group's members."""
        return _replay_views(self.L.praos_group_replay_immutable_views, self.g, self.check, path, views, params,
                             epoch_info, state, envelope, batch_max, verdicts_cap, counter_cap)

    def verify_tpraos_header_bytes(self, arena, off, length, decoded=False):
        arena, off, length = Context._chunk(arena, off, length)
        n = len(off)
        hb = Context.header_bytes_struct(arena, off, length)
        o, to = Context.tp_out(n)
        D, d = Context.alloc_decoded(n, TP_SIGNED_STRIDE) if decoded else (None, None)
        lo = np.zeros((n, 64), np.uint8) if decoded else None
        lp = np.zeros((n, 80), np.uint8) if decoded else None
        self.check(self.L.praos_group_verify_tpraos_header_bytes(self.g, ctypes.byref(hb), ctypes.byref(to),
                                                                 ctypes.byref(d) if decoded else None,
                                                                 ptr(lo) if decoded else None,
                                                                 ptr(lp) if decoded else None))
        if not decoded:
            return o
        D["leader_out"], D["leader_proof"] = lo, lp
        return o, D


def _replay(fn, handle, check, path, pools, params, epoch_info, state, envelope, batch_max, verdicts_cap, counter_cap,
            tpraos, extra_entropy):
    """praos_[group_]replay_immutable[_tpraos] (the same arguments after the context / group)."""
    arr = Context.pool_array(pools)
    st, hk, cv = _state_struct(state, counter_cap)
    E = Envelope()
    tip = envelope.get("tip")
    E.tip_is_origin = int(tip is None)
    if tip is not None:
        E.tip_slot, E.tip_block_no = tip[0], tip[1]
        ctypes.memmove(E.tip_hash, bytes(tip[2]), 32)
    for k in ("max_major_pv", "lv_prot_major", "max_header_size", "max_body_size"):
        setattr(E, k, envelope[k])
    ei = EpochInfo(*epoch_info)
    verdict = np.zeros(max(verdicts_cap, 1), np.uint8)
    fails = np.zeros(max(verdicts_cap, 1), np.uint16)
    S = ReplayStats()
    if tpraos:
        xe = None
        if extra_entropy is not None:
            xe = Nonce()
            ctypes.memmove(xe.hash, bytes(extra_entropy), 32)
        check(fn(handle, os.fsencode(str(path)), arr, len(pools), ctypes.byref(params), ctypes.byref(ei),
                 ctypes.byref(xe) if xe is not None else None, ctypes.byref(E), ctypes.byref(st), batch_max,
                 ptr(verdict), ptr(fails, u16p), verdicts_cap, ctypes.byref(S)))
    else:
        check(fn(handle, os.fsencode(str(path)), arr, len(pools), ctypes.byref(params), ctypes.byref(ei),
                 ctypes.byref(E), ctypes.byref(st), batch_max, ptr(verdict), verdicts_cap, ctypes.byref(S)))
    envelope["tip"] = None if E.tip_is_origin else (int(E.tip_slot), int(E.tip_block_no), bytes(E.tip_hash))
    state.update(_state_from_struct(st, hk, cv))
    stats = {name: getattr(S, name) for name, _ in ReplayStats._fields_}
    if tpraos:
        return stats, verdict[:verdicts_cap], fails[:verdicts_cap]
    return stats, verdict[:verdicts_cap]


def _replay_views(fn, handle, check, path, views, params, epoch_info, state, envelope, batch_max, verdicts_cap,
                  counter_cap):
    """praos_[group_]replay_immutable_views (the same arguments after the context / group)."""
    keep = [Context.pool_array(pools) for _, pools, _ in views]
    V = (LedgerView * max(1, len(views)))()
    for j, (first, pools, lim) in enumerate(views):
        V[j].first_epoch = first
        V[j].pools = ctypes.cast(keep[j], ctypes.c_void_p)
        V[j].npools = len(pools)
        V[j].lv_prot_major = lim["lv_prot_major"]
        V[j].max_header_size = lim["max_header_size"]
        V[j].max_body_size = lim["max_body_size"]
    st, hk, cv = _state_struct(state, counter_cap)
    E = Envelope()
    tip = envelope.get("tip")
    E.tip_is_origin = int(tip is None)
    if tip is not None:
        E.tip_slot, E.tip_block_no = tip[0], tip[1]
        ctypes.memmove(E.tip_hash, bytes(tip[2]), 32)
    E.max_major_pv = envelope["max_major_pv"]
    ei = EpochInfo(*epoch_info)
    verdict = np.zeros(max(verdicts_cap, 1), np.uint8)
    S = ReplayStats()
    check(fn(handle, os.fsencode(str(path)), V, len(views), ctypes.byref(params), ctypes.byref(ei), ctypes.byref(E),
             ctypes.byref(st), batch_max, ptr(verdict), verdicts_cap, ctypes.byref(S)))
    envelope["tip"] = None if E.tip_is_origin else (int(E.tip_slot), int(E.tip_block_no), bytes(E.tip_hash))
    state.update(_state_from_struct(st, hk, cv))
    stats = {name: getattr(S, name) for name, _ in ReplayStats._fields_}
    return stats, verdict[:verdicts_cap]


def _state_struct(state, cap):
    st = ChainState()
    counters = state.get("counters", {})
    keys = list(counters.keys())
    hk = np.zeros(28 * max(cap, 1), np.uint8)
    cv = np.zeros(max(cap, 1), np.uint64)
    if keys:
        hk[:28 * len(keys)] = np.frombuffer(b"".join(keys), np.uint8)
        cv[:len(keys)] = np.fromiter((counters[k] for k in keys), np.uint64, count=len(keys))
    st.last_slot_origin = int(state.get("last_slot") is None)
    st.last_slot = state.get("last_slot") or 0
    st.counter_hash28, st.counter, st.m, st.cap = ptr(hk), ptr(cv, u64p), len(keys), cap
    for a, b in (("evolving", "evolving"), ("candidate", "candidate"), ("epoch_nonce", "epoch_nonce"),
                 ("lab", "lab"), ("last_epoch_block", "leb")):
        v = state.get(b)
        getattr(st, a).neutral = int(v is None)
        if v is not None:
            ctypes.memmove(getattr(st, a).hash, v, 32)
    return st, hk, cv


def state_encode(state):
    """PraosState CBOR (praos_state_encode, Praos.hs:274-310) of a state dict (the form
    Context.update_chain_dep_state uses)."""
    L = load()
    st, hk, cv = _state_struct(state, len(state.get("counters", {})))
    n = ctypes.c_size_t(0)
    L.praos_state_encode(ctypes.byref(st), None, 0, ctypes.byref(n))
    out = np.zeros(max(n.value, 1), np.uint8)
    rc = L.praos_state_encode(ctypes.byref(st), ptr(out), n.value, ctypes.byref(n))
    if rc != 0:
        raise PraosError(f"praos_state_encode rc={rc}")
    return bytes(out[:n.value])


def _state_from_struct(st, hk, cv):
    hb = hk[:28 * st.m].tobytes()
    state = {"last_slot": None if st.last_slot_origin else int(st.last_slot),
             "counters": {hb[28 * k:28 * k + 28]: v for k, v in enumerate(cv[:st.m].tolist())}}
    for a, b in (("evolving", "evolving"), ("candidate", "candidate"), ("epoch_nonce", "epoch_nonce"),
                 ("lab", "lab"), ("last_epoch_block", "leb")):
        x = getattr(st, a)
        state[b] = None if x.neutral else bytes(x.hash)
    return state


def ticked_epoch_nonce(state, epoch_info, slot):
    """praos_ticked_epoch_nonce: the epoch nonce at `slot` (None = NeutralNonce)."""
    L = load()
    st, hk, cv = _state_struct(state, len(state.get("counters", {})))
    out = Nonce()
    rc = L.praos_ticked_epoch_nonce(ctypes.byref(st), ctypes.byref(EpochInfo(*epoch_info)), slot, ctypes.byref(out))
    if rc != 0:
        raise PraosError(f"praos_ticked_epoch_nonce rc={rc}")
    return None if out.neutral else bytes(out.hash)


def state_decode(data: bytes, cap=1 << 16):
    L = load()
    st, hk, cv = _state_struct({}, cap)
    buf = np.frombuffer(bytes(data), np.uint8).copy()
    rc = L.praos_state_decode(ptr(buf), len(buf), ctypes.byref(st))
    if rc != 0:
        raise PraosError(f"praos_state_decode rc={rc}")
    return _state_from_struct(st, hk, cv)


def params(slots_per_kes_period=129600, max_kes_evo=62, c_raw=0, f_is_one=False, vrf_check_output=True):
    p = Params()
    p.slots_per_kes_period = slots_per_kes_period
    p.max_kes_evo = max_kes_evo
    p.f_is_one = int(bool(f_is_one))
    p.vrf_check_output = int(bool(vrf_check_output))
    ctypes.memmove(p.c_raw, (int(c_raw) & ((1 << 128) - 1)).to_bytes(16, "little"), 16)
    return p
