/*
 * praos_hip.h -- C ABI of libpraos_hip.so, the MI355X (gfx950) batch validator
 * for Ouroboros Praos block-header crypto.
 *
 * Drop-in boundary: the reference validates one header at a
 * time in Haskell, calling C crypto per signature through cardano-crypto-class
 * FFI (`foreign import ccall` into libsodium; result CInt 0 = ok / -1 = fail).
 * This ABI replaces, for a contiguous batch of headers of one epoch:
 *
 *   praos_verify_headers  <- Praos.validateKESSignature  (Praos.hs:558-606)
 *                            + Praos.validateVRFSignature (Praos.hs:528-556)
 *                            as composed by updateChainDepState (Praos.hs:441-459)
 *   praos_verify_ocert    <- DSIGN.verifySignedDSIGN vkcold (ocertToSignable oc) tau
 *                            (Praos.hs:580; Ed25519DSIGN -> libsodium verify_detached)
 *   praos_verify_kes      <- KES.verifySignedKES vk_hot t hvSigned hvSignature
 *                            (Praos.hs:582; Shelley/Protocol/Praos.hs:85 for integrity)
 *   praos_verify_vrf      <- VRF.verifyCertified vrfK (mkInputVRF slot eta0) vrfCert
 *                            (Praos.hs:543; PraosVRF -> crypto_vrf_ietfdraft03_verify)
 *   praos_check_leader    <- checkLeaderNatValue (vrfLeaderValue cert) sigma f
 *                            (Praos.hs:549)
 *   praos_decode_headers  <- DecCBOR (Annotator (Header c)) + HeaderBody decoding, the
 *                            signable re-serialisation and headerHash
 *                            (Praos/Header.hs:90-94, :147-151, :187-231) over stored
 *                            header bytes (ImmutableDB chunk + secondary index)
 *   praos_verify_header_bytes <- decode + praos_verify_headers in one device pass
 *   praos_apply_batch     <- the first-error-wins order of updateChainDepState plus
 *                            the OCert counter rule (Praos.hs:584-606) and the
 *                            reupdateChainDepState counter/nonce update (Praos.hs:468-502)
 *
 * Conventions (mirroring the reference FFI): plain pointers + sizes, caller-owned
 * host buffers, nothing retained after return.  Return value 0 = ok, < 0 = system
 * error (PRAOS_E_*).  Cryptographic failures are DATA (bits in the outputs),
 * never return codes.  One context per host thread; calls block.
 */
#ifndef PRAOS_HIP_H
#define PRAOS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRAOS_ABI_VERSION 15

/* ---- return codes ---- */
#define PRAOS_OK 0
#define PRAOS_E_HIP (-1)     /* HIP runtime error (see praos_last_error) */
#define PRAOS_E_ARG (-2)     /* bad argument / inconsistent sizes */
#define PRAOS_E_OOM (-3)     /* device allocation failed */
#define PRAOS_E_STATE (-4)   /* praos_set_epoch not called */

/* ---- per-header check bits (uint16), one per reference error constructor ---- */
#define PRAOS_BIT_KES_BEFORE_START   0x0001u /* KESBeforeStartOCERT c0 kp */
#define PRAOS_BIT_KES_AFTER_END      0x0002u /* KESAfterEndOCERT kp c0 maxKESEvo */
#define PRAOS_BIT_OCERT_SIG          0x0004u /* InvalidSignatureOCERT n c0 "Verification failed" */
#define PRAOS_BIT_KES_MERKLE         0x0008u /* InvalidKesSignatureOCERT kp c0 t "Reject" */
#define PRAOS_BIT_KES_LEAF           0x0010u /* InvalidKesSignatureOCERT kp c0 t (Ed25519 leaf) */
#define PRAOS_BIT_COUNTER_MISSING    0x0020u /* NoCounterForKeyHashOCERT (praos_apply_batch) */
#define PRAOS_BIT_COUNTER_TOO_SMALL  0x0040u /* CounterTooSmallOCERT (praos_apply_batch) */
#define PRAOS_BIT_COUNTER_OVER_INC   0x0080u /* CounterOverIncrementedOCERT (praos_apply_batch) */
#define PRAOS_BIT_VRF_KEY_UNKNOWN    0x0100u /* VRFKeyUnknown */
#define PRAOS_BIT_VRF_KEY_WRONG      0x0200u /* VRFKeyWrongVRFKey */
#define PRAOS_BIT_VRF_PROOF          0x0400u /* VRFKeyBadProof: draft-03 proof rejected */
#define PRAOS_BIT_VRF_OUTPUT         0x0800u /* VRFKeyBadProof: certified output != proof_to_hash */
#define PRAOS_BIT_LEADER             0x1000u /* VRFLeaderValueTooBig */
#define PRAOS_BIT_INPUT              0x8000u /* malformed batch entry (e.g. body out of range) */
/* TPraos (praos_verify_tpraos_headers) reuses bits 0-4, 8, 9, 12 and replaces 10/11: */
#define PRAOS_BIT_TP_VRF_NONCE       0x0400u /* VRFKeyBadNonce (eta cert: proof or output) */
#define PRAOS_BIT_TP_VRF_LEADER      0x0800u /* VRFKeyBadLeaderValue (leader cert) */
/* ... and, with an overlay schedule (praos_set_overlay, d > 0): */
#define PRAOS_BIT_TP_OVERLAY         0x2000u /* informational: an ACTIVE overlay slot (genesis delegate's
                                                slot); bits 8/9 then mean the two bits below and no
                                                pool lookup or leader test applies */
#define PRAOS_BIT_TP_GEN_COLD        0x0100u /* (with TP_OVERLAY) WrongGenesisColdKeyOVERLAY */
#define PRAOS_BIT_TP_GEN_VRF         0x0200u /* (with TP_OVERLAY) WrongGenesisVRFKeyOVERLAY */
#define PRAOS_BIT_TP_NOT_ACTIVE      0x4000u /* NotActiveSlotOVERLAY (an overlay slot nobody may fill;
                                                no VRF check is made) */

/* ---- verdict codes of praos_apply_batch (first failing check, Praos.hs order) ---- */
enum praos_verdict {
  PRAOS_V_OK = 0,
  PRAOS_V_KES_BEFORE_START = 1,
  PRAOS_V_KES_AFTER_END = 2,
  PRAOS_V_OCERT_SIG = 3,
  PRAOS_V_KES_SIG = 4,            /* detail: bit KES_MERKLE or KES_LEAF */
  PRAOS_V_COUNTER_MISSING = 5,
  PRAOS_V_COUNTER_TOO_SMALL = 6,
  PRAOS_V_COUNTER_OVER_INC = 7,
  PRAOS_V_VRF_KEY_UNKNOWN = 8,
  PRAOS_V_VRF_KEY_WRONG = 9,
  PRAOS_V_VRF_BAD_PROOF = 10,
  PRAOS_V_LEADER_TOO_BIG = 11,
  PRAOS_V_INPUT = 12,
  /* envelope (praos_validate_headers only): HeaderEnvelopeError, then PraosEnvelopeError */
  PRAOS_V_ENV_BLOCK_NO = 13,      /* UnexpectedBlockNo expected actual */
  PRAOS_V_ENV_SLOT_NO = 14,       /* UnexpectedSlotNo expected actual */
  PRAOS_V_ENV_PREV_HASH = 15,     /* UnexpectedPrevHash oldTip actual */
  PRAOS_V_ENV_OBSOLETE_NODE = 16, /* ObsoleteNode lvProtVerMajor maxMajorPV */
  PRAOS_V_ENV_HEADER_SIZE = 17,   /* HeaderSizeTooLarge size max */
  PRAOS_V_ENV_BLOCK_SIZE = 18     /* BlockSizeTooLarge size max */
};

typedef struct praos_ctx praos_ctx;
typedef struct praos_batch praos_batch;

/* PraosParams fields used by header validation (Praos.hs:184-210) and the
 * active slot coefficient in the form checkLeaderNatValue consumes. */
typedef struct {
  uint64_t slots_per_kes_period;  /* praosSlotsPerKESPeriod (must be > 0) */
  uint64_t max_kes_evo;           /* praosMaxKESEvo */
  int32_t f_is_one;               /* activeSlotVal f == maxBound -> leader check always true */
  int32_t vrf_check_output;       /* 1: verifyCertified also requires certified output == beta
                                     (cardano-crypto-class >= 2.1 semantics); 0: proof only */
  uint8_t c_raw[16];              /* activeSlotLog f: Fixed E34 raw value, int128 LE two's complement, <= 0 */
} praos_params;

/* One entry of the stake distribution (PoolDistr, Views.hs:41-51). */
typedef struct {
  uint8_t hash28[28];             /* KeyHash 'StakePool = Blake2b-224(cold vk) */
  uint8_t vrf_hash32[32];         /* individualPoolStakeVrf = Blake2b-256(vrf vk) */
  uint8_t sigma_fp[16];           /* fromRational individualPoolStake: Fixed E34 raw, uint128 LE */
} praos_pool;

/* Headers of one batch, struct-of-arrays over caller memory (HeaderView,
 * Views.hs:22-39).  Fixed-width fields are n records each. */
typedef struct {
  size_t n;
  const uint64_t* slot;           /* hvSlotNo */
  const uint8_t* cold_vk;         /* hvVK, n*32 */
  const uint8_t* vrf_vk;          /* hvVrfVK, n*32 */
  const uint8_t* vrf_out;         /* certifiedOutput of hvVrfRes, n*64 */
  const uint8_t* vrf_proof;       /* certifiedProof, n*80 */
  const uint8_t* hot_vk;          /* OCert ocertVkHot, n*32 */
  const uint64_t* ocert_n;        /* ocertN */
  const uint64_t* ocert_c0;       /* ocertKESPeriod */
  const uint8_t* ocert_sig;       /* ocertSigma, n*64 */
  const uint8_t* kes_sig;         /* hvSignature (Sum6KES raw), n*448 */
  const uint64_t* body_off;       /* hvSigned: offset of the signed body bytes in body_bytes */
  const uint32_t* body_len;       /* hvSigned length */
  const uint8_t* body_bytes;
  size_t body_bytes_len;
} praos_headers;

/* A Nonce (Praos.hs): 32-byte hash, or NeutralNonce. */
typedef struct {
  uint8_t hash[32];
  int32_t neutral;                /* 1 = NeutralNonce */
} praos_nonce;

/* Outputs (any pointer may be NULL except bits). */
typedef struct {
  uint16_t* bits;                 /* n: PRAOS_BIT_* (crypto + range checks) */
  int32_t* pool_idx;              /* n: index into the praos_set_epoch pool array, -1 unknown */
  uint8_t* beta;                  /* n*64: proof_to_hash (zeros if Gamma undecodable) */
  uint8_t* leader;                /* n*32: vrfLeaderValue, big-endian natural */
  uint8_t* nonce;                 /* n*32: vrfNonceValue */
} praos_out;

/* ---- context ---- */
/* device >= 0: a HIP device.  PRAOS_HOST_ONLY: a context without a device that
 * supports only the host-side sequential part (praos_set_epoch, praos_apply_batch,
 * praos_update_chain_dep_state); every GPU entry point then returns PRAOS_E_STATE.
 * There is no CPU crypto path. */
#define PRAOS_HOST_ONLY (-1)
praos_ctx* praos_open(int device);               /* NULL on failure */
void praos_close(praos_ctx* ctx);
const char* praos_last_error(praos_ctx* ctx);
int praos_abi_version(void);

/* Epoch-constant inputs: eta0 (NULL = NeutralNonce), pool distribution, params. */
int praos_set_epoch(praos_ctx* ctx, const uint8_t eta0[32], const praos_pool* pools, uint32_t npools,
                    const praos_params* params);

/* Blocking: H2D, all checks on the GPU, D2H. */
int praos_verify_headers(praos_ctx* ctx, const praos_headers* h, praos_out* out);

/* Device-resident pipeline (bench / streaming): upload once, run many times. */
praos_batch* praos_batch_upload(praos_ctx* ctx, const praos_headers* h);
int praos_batch_run(praos_ctx* ctx, praos_batch* b);          /* async on the ctx stream */
int praos_batch_sync(praos_ctx* ctx);
int praos_batch_download(praos_ctx* ctx, praos_batch* b, praos_out* out);
void praos_batch_free(praos_ctx* ctx, praos_batch* b);
/* Options.  PRAOS_OPT_CONCURRENT (default 1): run the OCert, KES and VRF
 * kernels on three streams so their tail waves overlap. */
#define PRAOS_OPT_CONCURRENT 1
/* PRAOS_OPT_KERNELS: bit mask of the crypto kernels praos_batch_run launches
 * (1 = OCert + KES-period checks, 2 = Sum6KES, 4 = VRF + leader; default 7).
 * Used by the single-primitive benchmark configs; skipped checks report 0 bits. */
#define PRAOS_OPT_KERNELS 2
/* PRAOS_OPT_KEYCACHE (default 2): a public key (cold key, VRF key) used by at
 * least this many headers of a batch is decoded once per run and expanded into
 * multi-power tables, so those headers' OCert / VRF-U scalar chains are 16
 * windows long instead of 64 (k_keys.hip).  0 disables the cache.  Verdicts
 * are identical either way (keys are matched byte for byte). */
#define PRAOS_OPT_KEYCACHE 3
/* PRAOS_OPT_DEDUP (default 1): the OCert signature check (Praos.hs:580) depends only
 * on the 144 bytes (cold vk, hot vk, n, c0, sigma); a pool forges every header of an
 * epoch under one operational certificate, so each distinct tuple of a batch is
 * verified once (tuples compared byte for byte on the device) and its verdict is
 * copied to every header carrying the same bytes; the KES-period checks stay per
 * header.  Verdicts are identical either way. */
#define PRAOS_OPT_DEDUP 4
/* PRAOS_OPT_PIPELINE (default 0 = auto): praos_verify_header_bytes uploads a batch in
 * this many chunks (1 = no pipeline, up to 8): the stored bytes of chunk k+1 move host ->
 * device on a copy stream while chunk k is decoded and its VRF stage V runs; the rest of
 * the batch runs once after the last chunk, and the VRF outputs move back while the KES
 * checks finish; auto = up to 8 chunks of at least 49,152 headers, the first a quarter of the
 * others' size (nothing runs until it has landed). */
#define PRAOS_OPT_PIPELINE 5
/* PRAOS_OPT_KES_PAIR (default -1 = automatic): the cached Sum6KES leaf verifies take two
 * headers per lane from this many cache hits on, encoding both R' with one field inversion
 * (0 = never).  Automatic: from 196,608 hits when the KES pass runs alone (PRAOS_OPT_KERNELS
 * == 2); beside the OCert / VRF passes the longer waves cost more than they save.  Verdicts
 * are identical either way. */
#define PRAOS_OPT_KES_PAIR 6
/* PRAOS_OPT_POOL_KEYS (default -1 = on inside praos_replay_immutable*, off otherwise): the
 * cold-key and VRF-key cache entries (decoded key, validity flags, multi-power tables) are
 * kept across runs of the context in a store of 16,384 entries per kind, so a key seen by an
 * earlier batch is a cache hit without being decoded and expanded again; new keys are cached
 * from their first use (they recur in the batches that follow).  Keys are matched byte for
 * byte; verdicts are identical either way.  1 = on, 0 = off, 2 = on and emptied before the
 * next run.  A store more than 3/4 full is emptied before a run. */
#define PRAOS_OPT_POOL_KEYS 7
/* PRAOS_OPT_KES_NOCACHE (default 58000): batches of fewer headers than this check every Sum6KES
 * leaf signature uncached (no leaf-key cache: the per-lane chains run beside the VRF's stage V,
 * and the key chain -- lists, precompute, tables -- is not on the step's critical path; the
 * 1/8-epoch shard of a strong-scaling run is below it).  0 = the cache at every size.  Verdicts
 * are identical either way. */
#define PRAOS_OPT_KES_NOCACHE 8
int praos_set_option(praos_ctx* ctx, int opt, int value);
/* The wide tier of the VRF key cache.  min_uses (default -1 = automatic): a cached VRF key used
 * by at least this many headers of a batch gets, instead of its chunk tables, a table for every
 * 6-bit digit position of the challenge (22 x 32 points, 88 KB), and the U chains of its headers
 * are 22 additions without a doubling.  0 = no wide tier.  Automatic: 43 uses (the break-even of the
 * tables' cost) in batches of 300,000 headers or more.  max_keys (default 4096; < 1 = the
 * default): at most this many wide keys per batch (and never more than batch size / min_uses);
 * further keys stay in the chunk tier.  A run that uses the pool-key store (PRAOS_OPT_POOL_KEYS)
 * has no wide tier: the store's entries are chunk-tier entries.  An explicit min_uses applies at
 * every batch size; below 300,000 headers it can be slower than 0, because the key tables are on
 * that step's critical path and the wide hits run the plain stage-U kernel while the chunk tier's
 * run the ILP-4 build.  Memory: a batch allocates its wide buffers (88 KB per wide key, at most
 * max_keys, plus a second hit list) in the first run that uses the tier and keeps them; a later
 * run that needs more keys (a lower min_uses, a higher max_keys) allocates a larger set, and the
 * smaller one stays owned by the batch until it is freed.  Verdicts and outputs are identical
 * either way.  Environment: PRAOS_VRF_WIDE,
 * PRAOS_VRF_WIDE_CAP at praos_open.  Returns 0. */
int praos_set_vrf_wide(praos_ctx* ctx, int min_uses, int max_keys);
/* Key-cache statistics of the last praos_batch_run (after praos_batch_sync):
 * out[0..2] = cold keys cached, OCert items on cached keys, OCert items
 * uncached; out[3..5] = the same for VRF keys; out[6..8] for the KES leaf keys
 * (the Ed25519 key each Sum6KES signature ends on).  With the pool-key store on
 * (PRAOS_OPT_POOL_KEYS) out[0] / out[3] count the store's entries after the run.  Returns 0. */
int praos_batch_stats(praos_ctx* ctx, praos_batch* b, uint32_t out[9]);
/* The wide tier of the VRF key cache in the last praos_batch_run: out[0] = wide keys, out[1] =
 * VRF items on wide keys (counted in praos_batch_stats out[4] as well).  Every wide key's tables
 * are built by the run that uses them.  Both 0 when the tier was off.  Returns 0. */
int praos_batch_wide_stats(praos_ctx* ctx, praos_batch* b, uint32_t out[2]);
/* OCert dedup of the last praos_batch_run: out[0] = distinct OCert tuples verified,
 * out[1] = headers (out[0] = 0 when the dedup did not run).  Returns 0. */
int praos_batch_dedup_stats(praos_ctx* ctx, praos_batch* b, uint32_t out[2]);
/* Per-kernel time of the last praos_batch_run (ms, HIP events on the ctx stream).
 * which: 0 = ocert, 1 = kes, 2 = vrf, 3 = leader, 4 = whole run, 5 = header
 * decode (batches from praos_batch_upload_bytes; 0 otherwise), 6 = the VRF stage-V
 * kernel k_vrf_v alone (events around its launch on its own stream), 7 = the cached
 * Sum6KES kernel k_kes_ck alone (events around its launch on the KES stream).  With concurrent
 * streams, 0-2 are measured from the common start to each kernel's end. */
float praos_batch_kernel_ms(praos_ctx* ctx, int which);

/* Page-locks [p, p + len) of caller memory (hipHostRegister) for the context's device, e.g.
 * a replay reader's chunk buffer or a Haskell pinned ByteString that lives across many calls;
 * uploads whose source lies inside a registered range move by direct DMA instead of through
 * the library's pinned staging buffers and host copy threads.  Returns 0, or PRAOS_E_HIP.
 * Unregister before freeing the memory. */
int praos_host_register(praos_ctx* ctx, void* p, size_t len);
int praos_host_unregister(praos_ctx* ctx, void* p);

/* ---- stored headers: decode on the GPU ----
 * Input: a byte arena (e.g. an ImmutableDB chunk file as read) and per header
 * the (offset, length) of its CBOR item -- blockOffset + headerOffset and
 * headerSize from the secondary index (ImmutableDB/Impl/Index/Secondary.hs:93-128).
 * The header is HeaderRaw = [body, kesSig] (Praos/Header.hs:201-231) with the
 * 10-field HeaderBody (:160-199).  The KES message is the canonical
 * re-serialisation of the decoded body (`serialize' hb`, :90-94): equal to the
 * stored slice when that is canonical, re-encoded on the GPU otherwise.
 * header_hash = Blake2b-256 of the stored header bytes (headerHash, :147-151). */
typedef struct {
  size_t n;
  const uint8_t* bytes;           /* arena */
  size_t bytes_len;
  const uint64_t* off;            /* n: header i = bytes[off[i], off[i] + len[i]) */
  const uint32_t* len;            /* n */
} praos_header_bytes;

/* decode status (uint16 per header): the first failure, or 0 / NONCANONICAL */
#define PRAOS_DEC_RANGE        0x01u /* slice outside the arena */
#define PRAOS_DEC_SYNTAX       0x02u /* truncated / wrong major type / wrong array length */
#define PRAOS_DEC_SIZE         0x04u /* fixed-size byte string of the wrong length */
#define PRAOS_DEC_UNSUPPORTED  0x08u /* indefinite-length item or tag (never emitted by the reference) */
#define PRAOS_DEC_TRAILING     0x10u /* bytes after the header item within len */
#define PRAOS_DEC_NONCANONICAL 0x20u /* informational: stored body not canonical; signed bytes re-encoded */
#define PRAOS_DEC_OVERFLOW     0x40u /* integer out of range (bodySize > Word32, ProtVer major > maxVersion) */
#define PRAOS_MAX_PROT_MAJOR   9     /* cardano-ledger-binary maxVersion at the reference's CHaP index-state */
#define PRAOS_DEC_FAILED       0x5Fu /* mask of the failure bits */
#define PRAOS_SIGNED_STRIDE    448   /* bytes per header in praos_decoded.signed_body */

/* Decoded fields (caller buffers; every pointer may be NULL = not returned).
 * A header that fails to decode has all fields zero and signed_len 0xffffffff. */
typedef struct {
  uint16_t* status;               /* n: PRAOS_DEC_* */
  uint64_t* block_no;             /* hbBlockNo */
  uint64_t* slot;                 /* hbSlotNo */
  uint8_t* prev_hash;             /* n*32 hbPrev (zeros when GenesisHash) */
  uint8_t* prev_is_genesis;       /* n */
  uint8_t* cold_vk;               /* n*32 hbVk */
  uint8_t* vrf_vk;                /* n*32 hbVrfVk */
  uint8_t* vrf_out;               /* n*64 */
  uint8_t* vrf_proof;             /* n*80 */
  uint32_t* body_size;            /* hbBodySize */
  uint8_t* body_hash;             /* n*32 hbBodyHash */
  uint8_t* hot_vk;                /* n*32 ocertVkHot */
  uint64_t* ocert_n;
  uint64_t* ocert_c0;
  uint8_t* ocert_sig;             /* n*64 */
  uint64_t* prot_major;
  uint64_t* prot_minor;
  uint8_t* kes_sig;               /* n*448 */
  uint32_t* signed_len;           /* n: length of the KES message */
  uint8_t* signed_body;           /* n*stride, the KES message (serialize' hb): stride PRAOS_SIGNED_STRIDE,
                                     PRAOS_TP_SIGNED_STRIDE for praos_verify_tpraos_header_bytes */
  uint8_t* header_hash;           /* n*32 */
} praos_decoded;

int praos_decode_headers(praos_ctx* ctx, const praos_header_bytes* in, praos_decoded* out);
/* Decode + full header validation on the device.  bits gets PRAOS_BIT_INPUT for
 * a header that does not decode; dec may be NULL. */
int praos_verify_header_bytes(praos_ctx* ctx, const praos_header_bytes* in, praos_out* out, praos_decoded* dec);
/* ABI 15: the streaming form (a node or db-analyser validating batch after batch).  The call is
 * queued and returns at once; a context keeps three calls in flight, so the next submits' uploads,
 * decodes and stage V run under this call's key chains.  Its outputs (out, dec) are written by
 * the third submit after it, which waits for it, or by praos_verify_drain; in, the bytes it
 * points to, out and dec must stay valid and unchanged until then.  Outputs equal the blocking
 * call's.  Batches too small for the chunked pipeline (PRAOS_OPT_PIPELINE) run the blocking call
 * after the calls in flight.  praos_verify_header_bytes and praos_close drain first. */
int praos_verify_header_bytes_submit(praos_ctx* ctx, const praos_header_bytes* in, praos_out* out,
                                     praos_decoded* dec);
int praos_verify_drain(praos_ctx* ctx);
/* Device-resident form: the batch keeps the arena; praos_batch_run decodes and
 * then validates (bench / streaming replay).  praos_batch_download_decoded
 * copies the decoded fields of the last run. */
praos_batch* praos_batch_upload_bytes(praos_ctx* ctx, const praos_header_bytes* in);
int praos_batch_download_decoded(praos_ctx* ctx, praos_batch* b, praos_decoded* dec);
/* Decode a from-bytes batch now (async on the ctx stream; praos_batch_run then skips
 * the decode): lets the caller read the decoded fields -- e.g. slots and the certified
 * VRF outputs that drive the epoch nonces -- before the crypto runs. */
int praos_batch_decode(praos_ctx* ctx, praos_batch* b);
/* Several epochs in one batch (same ledger view, consecutive epoch nonces): header i
 * is verified under etas[eta_idx[i]] (k <= 256 entries) instead of the praos_set_epoch
 * nonce, from the next praos_batch_run on.  mkInputVRF (Praos/VRF.hs:55-69) is the only
 * nonce-dependent input.  Fold such outputs with praos_validate_headers_nonces. */
int praos_batch_set_nonces(praos_ctx* ctx, praos_batch* b, const praos_nonce* etas, uint32_t k,
                           const uint8_t* eta_idx);

/* ---- ImmutableDB block-integrity batch ----
 * Replaces verifyBlockIntegrity spkp blk (Shelley/Ledger/Integrity.hs:14-20), the
 * check ImmutableDB validation runs per stored block (--validate-all-blocks):
 *   verifyHeaderIntegrity (Shelley/Protocol/Praos.hs:84-101): Sum6KES verify of the
 *     header at t = kp - c0 if kp >= c0 else 0 (no OCert / VRF / maxKESEvo checks);
 *   blockMatchesHeader (Shelley/Ledger/Block.hs:150-158): hashTxSeq of the stored
 *     segments (Blake2b-256 over the segments' Blake2b-256 hashes) == hbBodyHash.
 * Input: praos_header_bytes whose (off, len) describe whole stored blocks: the
 * HardForkBlock wrapper [eraTag 6|7, [header, s1..s4]] or a bare [header, s1..s3|s4].
 * result[i] = 0 (verifyBlockIntegrity True) or PRAOS_BLK_* bits; body_hash (may be
 * NULL) gets the computed hashTxSeq (zeros when the block does not decode). */
#define PRAOS_BLK_DECODE    0x01u /* block envelope, a segment or the header does not decode */
#define PRAOS_BLK_KES       0x02u /* verifyHeaderIntegrity False */
#define PRAOS_BLK_BODY_HASH 0x04u /* blockMatchesHeader False */
int praos_verify_block_integrity(praos_ctx* ctx, const praos_header_bytes* blocks, uint64_t slots_per_kes_period,
                                 uint8_t* result, uint8_t* body_hash);
/* Device-resident form (bench / streaming ImmutableDB validation): upload once,
 * run any number of times, download the last run's results. */
praos_batch* praos_block_batch_upload(praos_ctx* ctx, const praos_header_bytes* blocks);
int praos_block_batch_run(praos_ctx* ctx, praos_batch* b, uint64_t slots_per_kes_period);
int praos_block_batch_download(praos_ctx* ctx, praos_batch* b, uint8_t* result, uint8_t* body_hash);

/* ---- ImmutableDB chunk validation (added without a version bump; purely additive) ----
 * CRC-32 (zlib, System.FS.CRC) of each span; crc[i] for span i; len 0 -> 0.
 * A span outside the arena: PRAOS_E_ARG before anything is launched.
 * Replaces computeCRC (System.FS.CRC) over the stored blocks, the checksum column of
 * Secondary.Entry.  Kernel tile size: PRAOS_CRC_TILE bytes, counted from a span's start. */
#define PRAOS_CRC_TILE 16384
int praos_crc32(praos_ctx* ctx, const praos_header_bytes* spans, uint32_t* crc);
/* Device-resident form: CRC-32 of the block spans of a praos_block_batch_upload batch (bench /
 * streaming validation); a span outside the arena: PRAOS_E_ARG, nothing launched. */
int praos_block_batch_crc32(praos_ctx* ctx, praos_batch* b, uint32_t* crc);

/* praos_validate_chunk replaces parseChunkFile (Storage/ImmutableDB/Impl/Parser.hs:92-197,
 * block boundaries as Util/CBOR.hs:217-290 finds them) for Shelley-based chunks: the chunk
 * file goes in once; out come the valid prefix as rebuilt Secondary entries, the first
 * error and the truncation offset.  Block i starts where block i-1 ended (block 0 at 0) and
 * is the one CBOR item that starts there.  Per block, in file order, the first offending
 * block ending the parse (the blocks before it are yielded):
 *   UNSUPPORTED    the item is well-formed CBOR and is [0, ...] or [1, ...] (Byron): the
 *                  caller falls back to the reference parser;
 *   ERR_READ       the item does not decode: not a well-formed item, not a block envelope
 *                  (praos_verify_block_integrity's rules) or the header does not decode.
 *                  This is as far as this library decodes blocks; the reference's
 *                  transaction decoders are stricter (a block whose segments are well-formed
 *                  CBOR but not valid transactions is a ReadFailure there, accepted here);
 *   checkEntries   i < n_expected and crc(block) == expected_crc[i]: trusted; otherwise
 *                  verifyBlockIntegrity runs, non-zero bits -> ERR_CORRUPT
 *                  (ChunkErrCorrupt, with blockPoint);
 *   checkIfHashesLineUp  i > 0 and prevHash /= BlockHash (headerHash of block i-1), a
 *                  GenesisHash prev at i > 0 included -> ERR_HASH_MISMATCH.
 * truncate_at is the offending block's start, bytes_len when there is none.
 * block_off is a HINT only (the index's blockOffsets): the device checks that every
 * candidate [block_off[i], block_off[i+1]) is exactly one item (the last one running to the
 * end of the file); from the first candidate that is not -- or from 0 without hints, with
 * off[0] != 0, or from the first non-ascending / out-of-range offset -- the host walks the
 * items itself (rescanned_from, bytes_len when no walk was needed).  Hints never change the
 * outcome; expected_crc is positional by true block index. */
#define PRAOS_CHUNK_OK                0
#define PRAOS_CHUNK_ERR_READ          1 /* ChunkErrRead */
#define PRAOS_CHUNK_ERR_CORRUPT       2 /* ChunkErrCorrupt */
#define PRAOS_CHUNK_ERR_HASH_MISMATCH 3 /* ChunkErrHashMismatch */
#define PRAOS_CHUNK_UNSUPPORTED       4 /* a Byron block: not handled here */
#define PRAOS_CHUNK_ENTRY_SIZE        56
typedef struct {
  const uint8_t* bytes;           /* NNNNN.chunk as read */
  size_t bytes_len;
  const uint32_t* expected_crc;   /* parseChunkFile's [CRC]: checksums of the secondary index, in order */
  size_t n_expected;              /* 0 = index missing or invalid */
  const uint64_t* block_off;      /* NULL, or n_expected blockOffsets of the same entries */
} praos_chunk;
typedef struct {
  uint32_t outcome;               /* PRAOS_CHUNK_* */
  uint32_t integrity_bits;        /* ERR_CORRUPT: PRAOS_BLK_* of the offending block */
  uint64_t blocks;                /* blocks yielded (with PRAOS_E_ARG for a small out->cap: needed) */
  uint64_t checked;               /* blocks that took verifyBlockIntegrity */
  uint64_t truncate_at;
  uint64_t rescanned_from;
  uint64_t err_slot;              /* ERR_CORRUPT / ERR_HASH_MISMATCH: the offending block's point */
  uint8_t err_hash[32];
  uint8_t expected_prev[32];      /* ERR_HASH_MISMATCH: headerHash of the block before */
  uint8_t actual_prev[32];        /* ERR_HASH_MISMATCH: the block's prevHash (zeros: GenesisHash) */
  uint8_t actual_prev_is_genesis;
  uint8_t pad_[7];
} praos_chunk_result;
typedef struct {
  size_t cap;                     /* capacity of the buffers below, in blocks */
  uint8_t* entries;               /* cap*56: Secondary.Entry as on disk (Secondary.hs:93-128): blockOffset u64,
                                     headerOffset u16, headerSize u16, checksum u32 (computed), headerHash,
                                     blockOrEBB = slot u64, big-endian */
  uint64_t* block_no;             /* for the Tip */
  uint8_t* prev_hash;             /* cap*32 (zeros when GenesisHash) */
  uint8_t* prev_is_genesis;       /* cap; block 0's fit against the previous chunk stays the caller's
                                     (Validation.hs:389-399) */
  int8_t* integrity;              /* cap: -1 trusted by its CRC, 0 checked and passed */
} praos_chunk_out;
int praos_validate_chunk(praos_ctx* ctx, const praos_chunk* chunk, uint64_t slots_per_kes_period,
                         praos_chunk_result* res, praos_chunk_out* out);

/* ---- Byron blocks and EBBs in a chunk (added without a version bump; purely additive) ----
 * praos_validate_chunk_cfg is praos_validate_chunk with the Byron era switched on:
 * praos_validate_chunk(ctx, ch, spkp, res, out) is this call with byron_epoch_slots = 0 and
 * is_ebb = NULL, and with byron_epoch_slots = 0 the results are byte-identical to it (a Byron
 * item ends the parse with UNSUPPORTED).  With byron_epoch_slots > 0 a stored item
 * 82 00 83 <hdr> <body> <extra> (EBB) or 82 01 83 <hdr> <body> <extra> (main block,
 * Byron/Ledger/Serialisation.hs:165-177) is a block like any other; a chunk may hold both
 * kinds (the first Shelley block's prevHash is a Byron header hash):
 *   point / entry  headerOffset 3, headerSize = the header item's length, headerHash =
 *                  Blake2b-256(82 0k || header); slot = epoch * byron_epoch_slots
 *                  (+ slotInEpoch for a main block), blockNo = difficulty; the entry's
 *                  blockOrEBB is the slot of a main block and the EPOCH NUMBER of an EBB
 *                  (Secondary.hs:84-88); is_ebb[i] = 1 marks the EBBs (0 for every other block);
 *   prevHash       GenesisHash for an EBB of epoch 0 (its 32 bytes are the genesis hash, not a
 *                  block; parity unpinned), BlockHash otherwise (Block.hs:215-221);
 *   ERR_READ       the item is [0|1, ...] but not of the shapes in csrc/k_byron.hip: a wrong list
 *                  length, a hash that is not bytes32, a key or signature that is not bytes64, a
 *                  signature tag other than 2, an integer too wide (pm u32, slotInEpoch u16,
 *                  the rest u64), an item that is not well-formed, a body that is not 4 items or
 *                  whose txPayload is not a list of 2-item lists.  This is as far as the library
 *                  decodes Byron blocks: the reference's transaction, ssc, delegation and update
 *                  decoders are stricter (a body of well-formed CBOR that is not a valid payload
 *                  is a ReadFailure there, accepted here);
 *   checkEntries   an untrusted block takes verifyBlockIntegrity (Byron/Ledger/Integrity.hs:
 *                  21-53): an EBB passes; a main block needs pm == byron_protocol_magic
 *                  (PRAOS_BLK_PM), the PBFT signature -- Ed25519 under the first 32 bytes of the
 *                  delegate key over "01" || issuerXPub || 09 || CBOR(pm) || 85 || the stored
 *                  prev, proof, slot-id, difficulty and extra items (PRAOS_BLK_PBFT_SIG; the
 *                  delegation certificate's own signature is not part of this check) -- and
 *                  blockMatchesHeader (PRAOS_BLK_BODY_HASH): dlgHash, updHash, nTx, witHash and
 *                  txRoot against the stored body (the ssc proof is not compared);
 *   UNSUPPORTED    with Byron on, only this: an untrusted main block with nTx != 1 whose ONLY
 *                  failing check is txRoot.  The Merkle root for n = 0 and n >= 2 follows the
 *                  published Byron rule (leaf H(00 || tx), node H(01 || l || r), split at the
 *                  largest power of two below n, empty tree H("")) and no reference file pins
 *                  it, so the caller lets the reference decide; truncate_at is that block and
 *                  the blocks before it are yielded.
 * err_slot is the offending block's slot (an EBB's too). */
#define PRAOS_BLK_PBFT_SIG 0x08u /* Byron verifyHeaderIntegrity: the PBFT signature does not verify */
#define PRAOS_BLK_PM       0x10u /* Byron verifyHeaderIntegrity: protocol magic /= the configured one */
/* which of blockMatchesHeader's five comparisons failed (praos_verify_byron_integrity) */
#define PRAOS_BYRON_W_DLG  0x01u
#define PRAOS_BYRON_W_UPD  0x02u
#define PRAOS_BYRON_W_NTX  0x04u
#define PRAOS_BYRON_W_WIT  0x08u
#define PRAOS_BYRON_W_ROOT 0x10u
typedef struct {
  uint64_t slots_per_kes_period;
  uint64_t byron_epoch_slots;     /* 0 = Byron items are UNSUPPORTED */
  uint32_t byron_protocol_magic;
  uint32_t pad_;
} praos_chunk_cfg;
int praos_validate_chunk_cfg(praos_ctx* ctx, const praos_chunk* chunk, const praos_chunk_cfg* cfg,
                             praos_chunk_result* res, praos_chunk_out* out,
                             uint8_t* is_ebb /* out->cap bytes, may be NULL */);
/* The direct form (tests, GetVerifiedBlock): verifyBlockIntegrity of stored Byron blocks
 * arena[off[i], off[i] + len[i]).  result[i] = 0 or PRAOS_BLK_DECODE (not a Byron block of the
 * shapes above) / PRAOS_BLK_PM / PRAOS_BLK_PBFT_SIG / PRAOS_BLK_BODY_HASH; which[i] (may be
 * NULL) = PRAOS_BYRON_W_* of the failing body comparisons.  epoch_slots > 0. */
int praos_verify_byron_integrity(praos_ctx* ctx, const praos_header_bytes* blocks, uint64_t epoch_slots,
                                 uint32_t protocol_magic, uint8_t* result, uint8_t* which);

/* ---- Transaction index of stored blocks (additive: ABI version unchanged) ----
 * One row per transaction of each stored block, built on the device from the block bytes, and
 * the per-block statistics db-analyser's ledger-free analyses print.  Replaces, per block,
 * HasAnalysis.countTxOutputs / blockTxSizes / blockStats (Cardano/Tools/DBAnalyser/Block/
 * Shelley.hs:61-98, Block/Byron.hs:34-86) and, per row, txId (Blake2b-256 of the stored body).
 * blocks: whole stored blocks as praos_verify_block_integrity takes them.  A Shelley-based block
 * is [header, s1 bodies, s2 witness sets, s3 {index: aux}, (s4 [invalid indices])], arrays and
 * maps definite or indefinite at every level.  Row t of a block with n = |s1|:
 *   body / wit / aux   spans into blocks->bytes; aux_len = 0: no auxiliary data
 *   size               1 + body_len + wit_len + (aux_len or 1): sizeTxF, [body, wits, aux / null]
 *   n_out              items of the array under the body map's first key 1; no key 1: 0
 *   ex_steps           blocks with s4: the sum mod 2^64 of the steps of the redeemers under the
 *                      witness set's first key 5, [[tag, index, data, [mem, steps]], ...] or
 *                      {key: [data, [mem, steps]], ...}; blocks without s4 (and a witness set
 *                      that is no map or has no key 5): 0
 *   is_valid           0 when t is listed in s4
 *   tx_id              Blake2b-256 of the stored body bytes
 * Byron (cfg->byron != 0): an EBB has no rows; a main block one row per [tx, witnesses] item of
 * txPayload: body = tx, wit = witnesses, no aux, size = the length of the whole item, n_out =
 * items of tx[1], ex_steps 0, is_valid 1, tx_id = Blake2b-256 of the tx item.  With cfg->byron
 * == 0 a Byron item ([0, ...] / [1, ...]) is PRAOS_TXI_DECODE.
 * A block that is not PRAOS_TXI_OK has n_tx 0, zero statistics and no rows. */
#define PRAOS_TXI_OK     0u
#define PRAOS_TXI_DECODE 1u /* not accepted by the block split (k_block.hip / k_byron.hip), or a span outside the arena */
#define PRAOS_TXI_SHAPE  2u /* s1 / s2 / s4 no array, s3 no map, |s2| /= |s1|, an s3 key or s4 entry not an
                               unsigned integer < n, a body no map, key 1 no array, key 5 of neither redeemer
                               form (Byron: tx no array of two items at least, tx[1] no array) */
typedef struct {
  uint32_t byron;                 /* non-zero: Byron blocks and EBBs are indexed */
  uint32_t pad_;
} praos_txi_cfg;
typedef struct {                  /* per block; every pointer may be NULL = not returned */
  uint8_t* status;                /* n: PRAOS_TXI_* */
  uint32_t* n_tx;                 /* n */
  uint64_t* txs_size;             /* n: sum of size */
  uint64_t* n_out;                /* n: sum of n_out */
  uint64_t* ex_steps;             /* n: sum of ex_steps mod 2^64 */
  uint64_t* tx_first;             /* n + 1: exclusive prefix sum of n_tx; block i's rows are
                                     [tx_first[i], tx_first[i + 1]) */
} praos_txi_stats;
typedef struct {                  /* per row; caller buffers of cap rows, every pointer may be NULL */
  size_t cap;
  size_t n_rows;                  /* out: the rows of the call */
  uint32_t* block;                /* the row's block */
  uint64_t* body_off;
  uint32_t* body_len;
  uint64_t* wit_off;
  uint32_t* wit_len;
  uint64_t* aux_off;
  uint32_t* aux_len;
  uint32_t* size;
  uint32_t* n_out;
  uint64_t* ex_steps;
  uint8_t* is_valid;
  uint8_t* tx_id;                 /* cap * 32 */
} praos_txi_rows;
/* stats and rows may be NULL.  When a row array is given and rows->cap < n_rows: PRAOS_E_ARG with
 * rows->n_rows = the count needed and stats filled; with no row array given cap is not looked at
 * (the sizing call).  n = 0 is PRAOS_OK with tx_first[0] = 0. */
int praos_index_block_txs(praos_ctx* ctx, const praos_header_bytes* blocks, const praos_txi_cfg* cfg,
                          praos_txi_stats* stats, praos_txi_rows* rows);
/* The same over a praos_block_batch_upload batch, with no second upload (bench; callers that run
 * praos_block_batch_run and the index over one upload, in either order: the index works in
 * buffers of its own and leaves the batch's results as they are). */
int praos_block_batch_tx_index(praos_ctx* ctx, praos_batch* b, const praos_txi_cfg* cfg, praos_txi_stats* stats,
                               praos_txi_rows* rows);

/* ---- Key witnesses of stored blocks' transactions (additive: ABI version unchanged) ----
 * Every VKey witness and every bootstrap witness of the transactions of stored blocks checked
 * as an Ed25519 signature over the transaction's txId, on the device and from the bytes as
 * stored.  Replaces the per-witness signature check the reference runs on the CPU when it
 * applies a block rather than reapplies it: applyBlockLedgerResult with asoValidation =
 * STS.ValidateAll (Shelley/Ledger/Ledger.hs:335-352) and applyShelleyTx in the mempool
 * (Shelley/Ledger/Mempool.hs:215-239); reapplyBlockLedgerResult (Ledger.hs:354-373) skips it.
 * Signature validity only: whether the right keys signed (witsVKeyNeeded) and every other UTXOW
 * rule need ledger state and are not checked; key_hash is returned so that a caller holding the
 * ledger can make that comparison.
 * blocks: whole stored blocks as praos_index_block_txs takes them.  The call runs that index in
 * buffers of its own and reads its rows' wit spans and tx_id; a batch's integrity results and
 * the index's own outputs stay as they are.
 * Scanned: the witness set of every row of a PRAOS_TXI_OK Shelley-based block (is_valid = 0 rows
 * too: UTXOW runs before phase 2).  The witness set is a map, definite or indefinite, keys of any
 * head width.  The value under the FIRST key 0 is the VKey witnesses, items [vkey, sig]; the
 * value under the FIRST key 2 the bootstrap witnesses, items [vkey, sig, chain_code, attributes].
 * Each value is an array, definite or indefinite, optionally wrapped in tag 258 (Conway's set
 * form; accepted in every era, a leniency); each item an array of exactly 2 / 4 elements,
 * definite or indefinite; vkey a definite byte string of 32 bytes, sig one of 64; chain_code and
 * attributes are skipped as one item each; other keys are skipped; the walk ends when both keys
 * have been seen or the map ends.  A witness set that is no map, or has neither key, has no
 * witnesses.
 *   PRAOS_TXW_SHAPE    the transaction has no witness rows: key 0 or key 2 present but of another
 *                      form (no array, a tag other than 258), an item of the wrong arity, a key
 *                      or signature of the wrong length or type or an indefinite byte string, or
 *                      a map whose walk ends inside a pair
 *   PRAOS_TXW_SKIPPED  a Byron row (cfg->byron != 0): no witness rows; Byron's SignTag framing
 *                      is pinned by nothing in the reference tree
 * A witness is ok iff libsodium's crypto_sign_verify_detached(sig, tx_id, 32, vkey) accepts, the
 * same for both kinds (verifyBootstrapWit's address-root comparison is not made).
 * Witness rows: transactions in the index's row order; inside one transaction the key-0 items in
 * stored order, then the key-2 items in stored order, whichever key came first in the map. */
#define PRAOS_TXW_OK      0u
#define PRAOS_TXW_SHAPE   1u
#define PRAOS_TXW_SKIPPED 2u
typedef struct {
  uint32_t byron;                 /* non-zero: Byron blocks are indexed (their rows SKIPPED) */
  uint32_t max_lanes;             /* witnesses verified per launch, 0 = the library's default; the
                                     outputs do not depend on it */
} praos_txw_cfg;
typedef struct {                  /* per block; every pointer may be NULL = not returned */
  uint8_t* status;                /* n: PRAOS_TXI_* */
  uint32_t* n_tx;                 /* n */
  uint32_t* n_wit;                /* n: witnesses of the block's transactions */
  uint32_t* n_bad;                /* n: witnesses that do not verify */
  uint32_t* n_shape;              /* n: transactions PRAOS_TXW_SHAPE */
  uint64_t* tx_first;             /* n + 1: exclusive prefix sum of n_tx */
} praos_txw_blocks;
typedef struct {                  /* per transaction row; caller buffers of cap rows, every pointer may be NULL */
  size_t cap;
  size_t n_rows;                  /* out: the rows of the call */
  uint32_t* block;                /* the row's block */
  uint8_t* status;                /* PRAOS_TXW_* */
  uint32_t* n_vkey;
  uint32_t* n_boot;
  uint32_t* n_bad;                /* witnesses of the row that do not verify */
  uint8_t* tx_id;                 /* cap * 32 */
  uint64_t* wit_first;            /* cap + 1: exclusive prefix sum of n_vkey + n_boot (n_rows + 1 written) */
} praos_txw_txs;
typedef struct {                  /* per witness; caller buffers of cap witnesses, every pointer may be NULL */
  size_t cap;
  size_t n_wits;                  /* out: the witnesses of the call */
  uint32_t* tx;                   /* the witness's transaction row */
  uint8_t* kind;                  /* 0 VKey witness, 2 bootstrap witness */
  uint64_t* key_off;              /* the 32 key bytes, into blocks->bytes */
  uint64_t* sig_off;              /* the 64 signature bytes, into blocks->bytes */
  uint8_t* ok;                    /* 1: the signature verifies */
  uint8_t* key_hash;              /* cap * 28: Blake2b-224 of vkey for kind 0, zeros for kind 2 */
} praos_txw_wits;
/* blocks_out, txs and wits may be NULL.  When an array of txs (wits) is given and its cap is below
 * n_rows (n_wits): PRAOS_E_ARG with n_rows and n_wits = the counts needed and blocks_out filled;
 * with no array given cap is not looked at (the sizing call).  n = 0 is PRAOS_OK. */
int praos_verify_tx_witnesses(praos_ctx* ctx, const praos_header_bytes* blocks, const praos_txw_cfg* cfg,
                              praos_txw_blocks* blocks_out, praos_txw_txs* txs, praos_txw_wits* wits);
/* The same over a praos_block_batch_upload batch, with no second upload; in either order with
 * praos_block_batch_run and praos_block_batch_tx_index, whose results it leaves as they are. */
int praos_block_batch_tx_witnesses(praos_ctx* ctx, praos_batch* b, const praos_txw_cfg* cfg,
                                   praos_txw_blocks* blocks_out, praos_txw_txs* txs, praos_txw_wits* wits);

/* ---- TxSubmission transactions: wire GenTxs, each checked once (additive: ABI version unchanged) ----
 * The key-witness check above for transactions as a peer offers them, before the mempool's addTx:
 * the second caller of that check, applyShelleyTx (Shelley/Ledger/Mempool.hs:215-239).
 * items: wire GenTx spans in one arena, as praos_unwrap_wire_headers takes wire headers.
 *   Shelley-based eras  [eraIndex, #6.24(bytes)], the bytes one array [body, wits, aux / null]
 *                       (era index 1..3) or [body, wits, isValid, aux / null] (era index >= 4)
 *                       (decodeNS; Shelley/Ledger/Mempool.hs:186-193 wrapCBORinCBOR)
 *   Byron (era 0)       [0, [kind, payload]], kind 0..3 (Byron/Ledger/Mempool.hs encodeByronGenTx):
 *                       unwrapped only -- the payload is every byte after the kind up to the end of
 *                       the item, at least one; no row, no witnesses
 * The wrapper's heads are taken at any width; its lists and the byte string are definite and the
 * tag is 24, as for wire headers.  The inner array may be definite (of exactly 3 / 4 items) or
 * indefinite; body, wits and the last item are one well-formed CBOR item each.
 * Item status: PRAOS_WIRE_OK / RANGE / SYNTAX / ERA / TRAILING with their meaning above, and
 *   PRAOS_GTX_SHAPE   no row: the inner bytes are not one such array (wrong count, another type, a
 *                     malformed item, bytes after the array inside the byte string), the body is
 *                     no map, the third of four items is neither 0xf4 nor 0xf5, or (era >= 4) the
 *                     value under the witness set's first key 5 has neither redeemer form
 *   PRAOS_GTX_BYRON   an era-0 item of the form above; any other era-0 form is SYNTAX
 * Rows: one per distinct transaction.  With cfg->dedup two items share a row iff their era index
 * and their inner bytes are equal (Blake2b-256 of the inner bytes, whole hashes compared): the
 * same body under another witness set or another era index is another row.  Rows are numbered in
 * order of first appearance; without dedup every PRAOS_WIRE_OK item is its own row.
 * Witnesses: praos_verify_tx_witnesses' rules over the row's wit span and tx_id, word for word. */
#define PRAOS_GTX_SHAPE 5
#define PRAOS_GTX_BYRON 6
#define PRAOS_GTX_PER_TX_OVERHEAD 4u /* Shelley/Ledger/Mempool.hs:125-143 perTxOverhead */
typedef struct {
  uint32_t n_eras;                /* eras of the block type (7 for the reference's CardanoBlock); 1..32 */
  uint32_t dedup;                 /* non-zero: byte-identical transactions share a row */
  uint32_t max_lanes;             /* as praos_txw_cfg */
  uint32_t pad_;
} praos_gtx_cfg;
typedef struct {                  /* per item (n entries); every pointer may be NULL = not returned */
  uint8_t* status;                /* PRAOS_WIRE_* / PRAOS_GTX_* */
  uint8_t* era;                   /* the wire era index (0xff until it is read) */
  uint32_t* row;                  /* the item's distinct-transaction row, 0xffffffff: none */
  uint8_t* byron_kind;            /* PRAOS_GTX_BYRON: 0..3; otherwise 0xff */
  uint64_t* payload_off;          /* PRAOS_GTX_BYRON: the payload span, into items->bytes; otherwise 0 */
  uint32_t* payload_len;
} praos_gtx_items;
typedef struct {                  /* per distinct transaction; caller buffers of cap rows, every pointer may be NULL */
  size_t cap;
  size_t n_rows;                  /* out: the rows of the call */
  uint32_t* item;                 /* the lowest item index of the class */
  uint8_t* era;
  uint64_t* body_off;             /* spans into items->bytes */
  uint32_t* body_len;
  uint64_t* wit_off;
  uint32_t* wit_len;
  uint64_t* aux_off;
  uint32_t* aux_len;              /* 0 when the last item is null (0xf6) */
  uint32_t* size;                 /* 1 + body_len + wit_len + the last item's stored length: sizeTxF */
  uint32_t* in_block_size;        /* size + PRAOS_GTX_PER_TX_OVERHEAD: txInBlockSize */
  uint64_t* ex_mem;               /* totExUnits: the sums mod 2^64 over the redeemers under the */
  uint64_t* ex_steps;             /* witness set's first key 5, both forms; 0 for eras 1..3 */
  uint8_t* is_valid;              /* the third item (0xf5: 1) for eras >= 4; 1 for eras 1..3 */
  uint8_t* tx_id;                 /* cap * 32: Blake2b-256 of the body bytes */
  uint8_t* wstatus;               /* PRAOS_TXW_OK / PRAOS_TXW_SHAPE */
  uint32_t* n_vkey;
  uint32_t* n_boot;
  uint32_t* n_bad;                /* witnesses of the row that do not verify */
  uint64_t* wit_first;            /* cap + 1: exclusive prefix sum of n_vkey + n_boot (n_rows + 1 written) */
} praos_gtx_txs;
/* per_item, txs and wits may be NULL; wits->tx holds the row.  When an array of txs (wits) is given
 * and its cap is below n_rows (n_wits): PRAOS_E_ARG with n_rows and n_wits = the counts needed and
 * the per-item arrays filled; with no array given cap is not looked at (the sizing call).  n = 0
 * is PRAOS_OK. */
int praos_verify_gen_txs(praos_ctx* ctx, const praos_header_bytes* items, const praos_gtx_cfg* cfg,
                         praos_gtx_items* per_item, praos_gtx_txs* txs, praos_txw_wits* wits);

/* ---- BlockFetch blocks: wire blocks, each checked once (additive: ABI version unchanged) ----
 * The checks the BlockFetch client makes on every block it receives, and the key-witness check
 * above for those blocks -- the blocks that ChainSel applies (ApplyVal) rather than reapplies:
 * mkBlockFetchConsensusInterface (MiniProtocol/BlockFetch/ClientInterface.hs:157-176) tests that
 * the block is the one asked for and blockMatchesHeader (Shelley/Ledger/Block.hs:150-158,
 * Byron/Ledger/Block.hs:161-162).  In deadline mode the decision logic "does not avoid requesting
 * a block that is already in-flight from other peers" (ClientInterface.hs:208-221), so the same
 * block arrives from several peers.
 * items: wire block spans in one arena.  A wire block is #6.24(bytes) around the stored block
 * [diskTag, ...] as praos_verify_block_integrity, praos_verify_byron_integrity and
 * praos_index_block_txs take it (wrapCBORinCBOR (encodeDiskHfcBlock ccfg),
 * HardFork/Combinator/Serialisation/SerialiseNodeToNode.hs:113): disk tag 0 an EBB, 1 a Byron main
 * block, 2..7 Shelley to Conway; no era list around it.  The tag's and the byte string's heads are
 * taken at any width; the tag is 24, the byte string definite; the inner bytes start with a
 * definite array head of length 2 and an unsigned integer, at any width (PRAOS_WIRE_SYNTAX
 * otherwise), a disk tag above cfg->n_eras is PRAOS_WIRE_ERA, bytes after the byte string are
 * PRAOS_WIRE_TRAILING; bytes after the block inside the byte string fail the split.
 * ranges: range r holds items [item_first[r], item_first[r + 1]) -- one peer's answer to one
 * request, in arrival order -- and expects the points [exp_first[r], exp_first[r + 1]) of
 * exp_slot / exp_hash, the points of the requested headers in order: item j of the range is
 * held against point j.  item_first[0] = 0 and item_first[k] = items->n, both arrays ascending.
 * Per item: the split of the stored-block calls (k_block_split for tags >= 2, k_byron_split for 0
 * and 1), slot, block number and prev hash from their decoders, and the header hash (Blake2b-256
 * of the header item; of 82 0k || header for Byron).
 * Rows: one per distinct block.  With cfg->dedup the items that split and decode are classed by
 * (disk tag, header hash, inner length); the representative of a class is its lowest item, and
 * every other member is compared byte for byte with it: equal, it shares the representative's
 * row; not equal, it gets a row of its own (such deviants are not classed among themselves).
 * Different bytes never share a row, and a body is hashed once per row.  Rows are numbered in
 * order of first appearance of their lowest item.  Without dedup every item that splits and
 * decodes is its own row.
 * Per row: bits = PRAOS_BLK_BODY_HASH when blockMatchesHeader fails, else 0.  No KES, PBFT
 * signature or protocol-magic check: ChainSync validated the header and the hash carries that
 * over.  Tags >= 2: body_hash = hashTxSeq as computed.  Tags 0 / 1: praos_verify_byron_integrity's
 * body half with its PRAOS_BYRON_W_* in which; an EBB passes; body_hash is zeros.
 * With cfg->witnesses: praos_verify_tx_witnesses over the rows' inner bytes (byron = Byron on),
 * word for word; blocks_out, txs and wits are its outputs with "block" meaning row, and a row
 * whose body check failed is indexed all the same.
 * Verdict per item, the first that applies:
 *   PRAOS_BF_WIRE          status != PRAOS_WIRE_OK
 *   PRAOS_BF_TOO_MANY      its index in the range >= the range's expected points
 *   PRAOS_BF_UNSUPPORTED   a Byron item with byron_epoch_slots = 0; or a Byron main block of
 *                          n /= 1 transactions whose txRoot is the only failing comparison
 *   PRAOS_BF_DECODE        the envelope or the header does not split or decode: no row
 *   PRAOS_BF_WRONG_BLOCK   slot or header hash differs from the expected point (an EBB's slot:
 *                          epoch * byron_epoch_slots)
 *   PRAOS_BF_INVALID_BODY  the row's bits != 0
 *   PRAOS_BF_OK
 * Per range, folded on the host: stop = the index in the range of its first item that is not
 * PRAOS_BF_OK (the item count when there is none); the items after it read
 * PRAOS_BF_NOT_REACHED (their rows stay); accepted = stop; status COMPLETE, FAILED (an item is
 * not OK) or TOO_FEW (no failure, fewer items than points).
 * Host round trips: one for the row count, praos_verify_tx_witnesses' three with cfg->witnesses,
 * and the final wait for the downloads. */
#define PRAOS_BF_OK            0
#define PRAOS_BF_WIRE          1
#define PRAOS_BF_DECODE        2
#define PRAOS_BF_WRONG_BLOCK   3
#define PRAOS_BF_INVALID_BODY  4
#define PRAOS_BF_TOO_MANY      5
#define PRAOS_BF_UNSUPPORTED   6
#define PRAOS_BF_NOT_REACHED   255
#define PRAOS_BF_RANGE_COMPLETE 0
#define PRAOS_BF_RANGE_FAILED   1
#define PRAOS_BF_RANGE_TOO_FEW  2
#define PRAOS_BF_NO_ROW 0xffffffffu
typedef struct {
  size_t k;                       /* ranges */
  const uint64_t* item_first;     /* k + 1 */
  const uint64_t* exp_first;      /* k + 1 */
  const uint64_t* exp_slot;       /* exp_first[k] */
  const uint8_t* exp_hash;        /* exp_first[k] * 32 */
} praos_bf_ranges;
typedef struct {
  uint32_t n_eras;                /* the highest disk tag (7 for the reference's CardanoBlock); 1..31 */
  uint32_t dedup;                 /* non-zero: byte-identical blocks share a row */
  uint32_t witnesses;             /* 0: stop after the body check */
  uint32_t max_lanes;             /* as praos_txw_cfg */
  uint64_t byron_epoch_slots;     /* 0: Byron off */
} praos_bf_cfg;
typedef struct {                  /* per item (n entries); every pointer may be NULL = not returned */
  uint8_t* status;                /* PRAOS_WIRE_* */
  uint8_t* tag;                   /* the disk tag (0xff until it is read) */
  uint8_t* verdict;               /* PRAOS_BF_* */
  uint32_t* row;                  /* the item's distinct-block row, PRAOS_BF_NO_ROW: none */
} praos_bf_items;
typedef struct {                  /* per range (k entries); every pointer may be NULL */
  uint64_t* stop;
  uint64_t* accepted;
  uint8_t* status;                /* PRAOS_BF_RANGE_* */
} praos_bf_range_out;
typedef struct {                  /* per distinct block; caller buffers of cap rows, every pointer may be NULL */
  size_t cap;
  size_t n_rows;                  /* out: the rows of the call */
  uint32_t* item;                 /* the lowest item index of the row */
  uint8_t* tag;
  uint8_t* is_ebb;
  uint64_t* slot;
  uint64_t* block_no;
  uint8_t* header_hash;           /* cap * 32 */
  uint8_t* prev_hash;             /* cap * 32; zeros for Genesis */
  uint64_t* hdr_off;              /* the header item, into items->bytes */
  uint32_t* hdr_len;
  uint64_t* blk_off;              /* the inner bytes: the stored block */
  uint32_t* blk_len;
  uint8_t* body_hash;             /* cap * 32: as computed (tags >= 2) */
  uint8_t* bits;                  /* 0 or PRAOS_BLK_BODY_HASH */
  uint8_t* which;                 /* PRAOS_BYRON_W_* (tags 0 / 1) */
} praos_bf_rows;
/* per_item, per_range, rows, blocks_out, txs and wits may be NULL.  When an array of rows, txs or
 * wits is given and its cap is below the count: PRAOS_E_ARG with n_rows / n_wits = the counts
 * needed and the per-item and per-range arrays filled; with no array given cap is not looked at
 * (the sizing call).  blocks_out has a row per entry and no cap of its own: its arrays hold
 * rows->cap entries (tx_first rows->cap + 1), and they are written only when rows is given and
 * rows->cap >= n_rows -- never with rows NULL, never on a call whose rows do not fit.  At most
 * 2^30 items in one call.  n = 0 is PRAOS_OK (every range TOO_FEW or COMPLETE). */
int praos_verify_fetched_blocks(praos_ctx* ctx, const praos_header_bytes* items, const praos_bf_ranges* ranges,
                                const praos_bf_cfg* cfg, praos_bf_items* per_item, praos_bf_range_out* per_range,
                                praos_bf_rows* rows, praos_txw_blocks* blocks_out, praos_txw_txs* txs,
                                praos_txw_wits* wits);
/* ---- Byron header validation: PBFT (additive as the two sections above: ABI version unchanged) ----
 * validateHeader for Byron = validateEnvelope (HeaderValidation.hs:297-344 with the Byron
 * instance, Byron/Ledger/HeaderValidation.hs:39-75) + PBFT updateChainDepState
 * (Protocol/PBFT.hs:320-353, the window of Protocol/PBFT/State.hs:206-228), over the view
 * Byron/Ledger/PBFT.hs:43-69 builds.  Split as the Praos path is: the per-header work on the
 * GPU (praos_verify_pbft_headers), the sequential fold on the host
 * (praos_pbft_update_chain_dep_state).  One delegation map per call: the caller splits a batch
 * at a re-delegation.  Not checked (the Byron ledger's, not PBFT's): the delegation certificate's
 * own signature.  Ed25519 edge rules are ed25519_verify_core's, as praos_verify_byron_integrity's
 * (cardano-crypto's are not pinned by the reference tree). */
#define PRAOS_PBFT_BIT_DECODE       0x01u /* not a Byron header of the shapes in csrc/k_byron.hip (for its is_ebb) */
#define PRAOS_PBFT_BIT_SIG          0x02u /* PBftInvalidSignature (PBFT.hs:330-336) */
#define PRAOS_PBFT_BIT_NOT_DELEGATE 0x04u /* PBftNotGenesisDelegate (PBFT.hs:344-348): hashVerKey not in the map */
/* verdicts of the fold, after the ones in use */
#define PRAOS_V_PBFT_INVALID_SIG   20 /* PBftInvalidSignature */
#define PRAOS_V_PBFT_INVALID_SLOT  21 /* PBftInvalidSlot: slot < lastSignedSlot (PBFT.hs:341-342) */
#define PRAOS_V_PBFT_NOT_DELEGATE  22 /* PBftNotGenesisDelegate */
#define PRAOS_V_PBFT_EXCEEDED      23 /* PBftExceededSignThreshold gk n (PBFT.hs:351-352); aux = n */
#define PRAOS_V_ENV_EBB_IN_SLOT    24 /* UnexpectedEBBInSlot (Byron/Ledger/HeaderValidation.hs:58-60) */
typedef struct {
  uint64_t window_size;           /* k: PBftWindowSize */
  uint64_t threshold;             /* floor (pbftSignatureThreshold * k), computed by the caller: no float crosses the ABI */
  uint64_t epoch_slots;           /* > 0 */
  uint32_t protocol_magic;        /* the configured one: part of the signed message (mkByronContextDSIGN) */
  uint32_t pad_;
} praos_pbft_params;
typedef struct {
  uint8_t* bits;                  /* n: PRAOS_PBFT_BIT_* */
  int32_t* gk_idx;                /* n: index of the delegate's pair in delegs, -1 when absent (EBBs: -1) */
  uint64_t* slot;                 /* n: epoch * epoch_slots + slotInEpoch; an EBB's epoch * epoch_slots */
  uint64_t* block_no;             /* n: difficulty */
  uint8_t* prev_hash;             /* n*32 (zeros when GenesisHash) */
  uint8_t* prev_is_genesis;       /* n: an EBB of epoch 0 */
  uint8_t* header_hash;           /* n*32: Blake2b-256(82 0k || header) */
  uint8_t* delegate_hash;         /* n*28, may be NULL: hashVerKey of the delegate (zeros for an EBB) */
} praos_pbft_out;
/* hashVerKey of Byron (cardano-crypto-wrapper): Blake2b-224(SHA3-256(58 40 || xpub64)); keys64 n*64,
 * out28 n*28.  On the device of a device context, on the host of a host-only one. */
int praos_byron_key_hash(praos_ctx* ctx, const uint8_t* keys64, size_t n, uint8_t* out28);
/* The per-header half.  in: the stored headers (headerOffset / headerSize of the secondary
 * index); is_ebb: n bytes; delegs: n_delegs pairs of 56 bytes (genesis key hash 28, delegate key
 * hash 28), the Bimap of the ledger view: a duplicate in either column is PRAOS_E_ARG, a span
 * outside the arena too.  A main header that decodes gets its delegate looked up and its
 * signature verified; an EBB and a header that does not decode skip both.  PRAOS_OPT_KEYCACHE 0
 * turns the delegate-key cache off; results are the same either way.  Needs a device. */
int praos_verify_pbft_headers(praos_ctx* ctx, const praos_header_bytes* in, const uint8_t* is_ebb,
                              const praos_pbft_params* params, const uint8_t* delegs, uint32_t n_delegs,
                              praos_pbft_out* out);
/* Which kernels the context's last praos_verify_pbft_headers ran: out[0] = 1 when the delegate-key
 * cache ran (0: every verify uncached), out[1] = keys cached, out[2] = verifies on cached keys
 * (k_pbft_sig_ck), out[3] = uncached verifies (k_pbft_sig).  Results do not depend on any of this. */
int praos_pbft_stats(praos_ctx* ctx, uint32_t out[4]);
typedef struct {
  uint8_t origin;                 /* 1: no tip (Origin); the other fields are ignored */
  uint8_t is_ebb;
  uint8_t pad_[6];
  uint64_t slot;
  uint64_t block_no;
  uint8_t hash[32];
} praos_pbft_tip;
typedef struct {                  /* PBftState: the signers in the window, oldest first */
  uint64_t cap;                   /* capacity of the arrays; the fold needs cap >= window_size > 0 */
  uint64_t n;
  uint64_t* slot;                 /* cap */
  uint8_t* genesis_hash;          /* cap*28 */
} praos_pbft_state;
/* The sequential half, on the host (works on a host-only context), over the outputs above.  Per
 * header: PRAOS_PBFT_BIT_DECODE -> PRAOS_V_INPUT; then the envelope in the reference's order --
 * block number (0 at Origin; the tip's for an EBB after a non-EBB; the tip's + 1 otherwise:
 * PRAOS_V_ENV_BLOCK_NO, aux = expected), slot (>= 0 at Origin; >= the tip's for a non-EBB after an
 * EBB; >= the tip's + 1 otherwise: PRAOS_V_ENV_SLOT_NO, aux = the minimum), prev hash
 * (PRAOS_V_ENV_PREV_HASH), an EBB whose slot mod epoch_slots /= 0 (PRAOS_V_ENV_EBB_IN_SLOT) --
 * then, for a main header, PBFT in its order: signature, slot < lastSignedSlot, delegate, and the
 * window step: append (slot, genesis key), drop the oldest signer iff the window held exactly
 * window_size signers before the append, PRAOS_V_PBFT_EXCEEDED iff the key's count after that
 * exceeds threshold (aux = the count).  An EBB leaves the state alone.  Batch semantics are
 * praos_update_chain_dep_state's: *chain_stop = the first failing header (n when none), tip and
 * st on return are those at chain_stop, later headers get would-be verdicts against a working
 * copy that skips the invalid ones.  aux (n) may be NULL.  window_size = 0 is PRAOS_E_ARG (no
 * window the reference's append could keep a signer in). */
int praos_pbft_update_chain_dep_state(praos_ctx* ctx, size_t n, const praos_pbft_out* h, const uint8_t* is_ebb,
                                      const praos_pbft_params* params, const uint8_t* delegs, uint32_t n_delegs,
                                      praos_pbft_tip* tip, praos_pbft_state* st, uint8_t* verdict, uint64_t* aux,
                                      size_t* chain_stop);
/* encodePBftState / decodePBftState (Protocol/PBFT/State.hs:277-305): [1, {genesis key hash:
 * [_ slots, newest first]}], keys in ascending byte order, an empty window a0.  encode: *len
 * gets the size; PRAOS_E_ARG if cap is too small (call with cap 0 to size).  decode: the signers
 * sorted by slot, stable over (key order, stored order) as sortOn is; st->n gets the count,
 * PRAOS_E_ARG if it exceeds st->cap or the bytes are not that encoding. */
int praos_pbft_state_encode(const praos_pbft_state* st, uint8_t* out, size_t cap, size_t* len);
int praos_pbft_state_decode(const uint8_t* in, size_t len, praos_pbft_state* st);

/* ---- TPraos (Shelley..Alonzo), the d = 0 path of cardano-protocol-tpraos ----
 * Replaces SL.updateChainDepState's crypto (TPraos.hs:378-387): OVERLAY
 * praosVrfChecks (pool, VRF key, eta cert with mkSeed seedEta, leader cert with
 * mkSeed seedL, checkLeaderValue on the 64-byte leader output, bound 2^512) and
 * the OCERT rule (same predicates as Praos a2).  Overlay slots (d > 0, genesis
 * delegates) are not handled. */
typedef struct {
  praos_headers h;                /* vrf_out / vrf_proof = bheaderEta; body = the signed BHBody bytes */
  const uint8_t* leader_out;      /* bheaderL certified output, n*64 */
  const uint8_t* leader_proof;    /* n*80 */
} praos_tpraos_headers;
typedef struct {
  uint16_t* bits;                 /* n: PRAOS_BIT_* / PRAOS_BIT_TP_* */
  int32_t* pool_idx;              /* n */
  uint8_t* beta_eta;              /* n*64 */
  uint8_t* beta_leader;           /* n*64 */
  uint8_t* nonce;                 /* n*32: mkNonceFromOutputVRF (Blake2b-256 of the eta output) */
} praos_tpraos_out;
int praos_verify_tpraos_headers(praos_ctx* ctx, const praos_tpraos_headers* h, praos_tpraos_out* out);

/* TPraos headers from stored bytes (ImmutableDB chunk spans of Shelley..Alonzo blocks):
 * BHeader = [BHBody, kesSig] decoded on the device (cardano-protocol-tpraos
 * DecCBOR BHeader / BHBody: 15 fields, the eta and leader certificates as two
 * [output, proof] pairs, OCert and ProtVer inlined; the KES message is the canonical
 * re-encoding `serialize' bhb`, the stored slice when canonical), then the crypto of
 * praos_verify_tpraos_headers.  A header that does not decode gets PRAOS_BIT_INPUT.
 * dec (may be NULL) receives the decoded fields, signed_body with a
 * PRAOS_TP_SIGNED_STRIDE stride; leader_out / leader_proof (may be NULL, n*64 / n*80)
 * the leader certificate.  Replaces, per epoch, the header crypto of
 * TPraos.updateChainDepState (TPraos.hs:378-387) for eras Shelley..Alonzo
 * (HFEras.hs:43-49); the fold is praos_tpraos_update_chain_dep_state. */
#define PRAOS_TP_SIGNED_STRIDE 640
int praos_verify_tpraos_header_bytes(praos_ctx* ctx, const praos_header_bytes* in, praos_tpraos_out* out,
                                     praos_decoded* dec, uint8_t* leader_out, uint8_t* leader_proof);
/* Device-resident form (the TPraos replay): praos_batch_run on such a batch decodes and
 * runs the TPraos kernels (under per-header nonces after praos_batch_set_nonces);
 * praos_batch_download_decoded / praos_batch_download_tpraos copy the results. */
praos_batch* praos_batch_upload_tpraos_bytes(praos_ctx* ctx, const praos_header_bytes* in);
int praos_batch_download_tpraos(praos_ctx* ctx, praos_batch* b, praos_tpraos_out* out);

/* ---- TPraos decentralisation overlay (d > 0; Shelley..Alonzo before d reached 0) ----
 * cardano-protocol-tpraos OVERLAY (lookupInOverlaySchedule, the same call
 * TPraos.checkIsLeader makes at TPraos.hs:304-337): with s = slot - first slot of its
 * epoch, the slot is in the overlay schedule iff ceiling(s d) < ceiling((s + 1) d);
 * then position = ceiling(s d) is active iff position mod ascInv == 0 (ascInv =
 * floor(1 / f)), and its genesis key is the (position div ascInv) mod |genDelegs|-th
 * of the genesis key hashes in ascending byte order.  An active overlay slot must be
 * forged by that key's delegate (WrongGenesisColdKeyOVERLAY) with the delegate's VRF
 * key (WrongGenesisVRFKeyOVERLAY), both certificates verify (VRFKeyBadNonce /
 * VRFKeyBadLeaderValue), and no leader-value test applies; a non-active overlay slot
 * fails NotActiveSlotOVERLAY.  Other slots take the Praos checks (pool, VRF key,
 * certificates, leader value).  The OCERT rule runs for every header; genesis
 * delegates count as known issuers (currentIssueNo). */
typedef struct {
  uint8_t genesis_hash28[28];     /* KeyHash 'Genesis: a key of lvGenDelegs */
  uint8_t delegate_hash28[28];    /* genDelegKeyHash: the delegate's cold-key hash */
  uint8_t vrf_hash32[32];         /* genDelegVrfHash */
} praos_gen_deleg;
typedef struct {
  uint64_t d_num, d_den;          /* lvD, a UnitInterval: d = d_num / d_den (d_den > 0, d_num <= d_den) */
  uint64_t asc_num, asc_den;      /* activeSlotVal f = asc_num / asc_den (0 < f <= 1) */
  uint64_t epoch_base_slot;       /* fixed-size epochs (first slot of the slot's epoch = epochInfoFirst) */
  uint64_t epoch_length;
  const praos_gen_deleg* gen_delegs;  /* any order (sorted by genesis hash inside) */
  uint32_t n_gen_delegs;          /* > 0 when d > 0 */
} praos_overlay;
/* ov == NULL or d_num == 0: no overlay (the d = 0 behaviour).  Kept until replaced. */
int praos_set_overlay(praos_ctx* ctx, const praos_overlay* ov);
/* The schedule itself (host-side; host-only contexts too): cls[i] = -1 (not an overlay
 * slot), -2 (NonActiveSlot) or k >= 0 (ActiveSlot of the k-th genesis key in ascending
 * hash order). */
int praos_overlay_classify(praos_ctx* ctx, size_t n, const uint64_t* slots, int32_t* cls);


/* ---- single-primitive batches (configs C2-C4); outputs 1 = valid, 0 = invalid ---- */
/* Ed25519 over the OCert signable hot_vk || BE64(n) || BE64(c0). */
int praos_verify_ocert(praos_ctx* ctx, size_t n, const uint8_t* cold_vk, const uint8_t* hot_vk,
                       const uint64_t* ocert_n, const uint64_t* ocert_c0, const uint8_t* sig, uint8_t* ok);
/* Sum6KES: result 0 = ok, 1 = Merkle "Reject", 2 = leaf Ed25519 failure. */
int praos_verify_kes(praos_ctx* ctx, size_t n, const uint8_t* vk, const uint32_t* period, const uint8_t* sig,
                     const uint64_t* msg_off, const uint32_t* msg_len, const uint8_t* msg_bytes,
                     size_t msg_bytes_len, uint8_t* result);
/* ECVRF-ED25519-SHA512-Elligator2 draft-03 verify; alpha is 32 bytes per item. */
int praos_verify_vrf(praos_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* proof, const uint8_t* alpha,
                     uint8_t* ok, uint8_t* beta);
/* checkLeaderNatValue; leader = 32-byte big-endian naturals, sigma_fp per item. */
int praos_check_leader(praos_ctx* ctx, size_t n, const uint8_t* leader, const uint8_t* sigma_fp,
                       const praos_params* params, uint8_t* is_leader);

/* ---- host-side sequential part (Praos.hs:441-502 order and state) ----
 * Counter map: the OCert issue numbers of praosStateOCertCounters, keyed by
 * issuer hash (Blake2b-224 of cold vk).  Walks the batch in order: verdict =
 * first failing check, then (as the reference does after a valid header)
 * counters[hk] := n.  `assume_valid_prefix` semantics: every header is judged
 * against the state left by all earlier headers of the batch as if valid.
 * chain_stop receives the index of the first non-OK header (n if none). */
typedef struct {
  const uint8_t* hash28;          /* m*28, any order */
  uint64_t* counter;              /* m: in = current counters; updated in place for existing keys */
  size_t m;
} praos_counters;

int praos_apply_batch(praos_ctx* ctx, const praos_headers* h, const praos_out* crypto,
                      praos_counters* counters, uint8_t* verdict, size_t* chain_stop);

/* ---- full chain-dependent state fold (tickChainDepState + updateChainDepState +
 *      reupdateChainDepState, Praos.hs:407-502) over a batch ----
 * Nonce = NeutralNonce | Nonce (32-byte hash); a ⭒ b = Blake2b-256(a || b), Neutral is
 * the identity.  Epochs: fixed size from a base (epoch of slot s =
 * base_no + (s - base_slot) / length); stability_window = computeStabilityWindow k f
 * (Praos.hs:497-498; ceiling(3k/f), computed by the caller).
 * Per header i, in order: tick (isNewEpoch last_slot slot_i, Ledger/Util.hs:20-40:
 * epoch_nonce := candidate ⭒ last_epoch_block, last_epoch_block := lab); the ticked
 * epoch nonce must equal the ctx's eta0 (the nonce the crypto outputs were computed
 * with), else the fold stops there (*processed = i) so the caller can set_epoch and
 * verify the rest; verdict as praos_apply_batch; on OK the ticked state is kept and
 * reupdated: last_slot := slot, lab := prevHashToNonce prev_hash, evolving :=
 * evolving ⭒ vrfNonceValue, candidate := evolving' if slot + stability_window <
 * firstSlotNextEpoch, counters[hk] := n (new keys appended; PRAOS_E_ARG past cap). */

typedef struct {
  int32_t last_slot_origin;       /* praosStateLastSlot = Origin */
  uint64_t last_slot;
  uint8_t* counter_hash28;        /* praosStateOCertCounters: cap*28 */
  uint64_t* counter;              /* cap */
  size_t m;                       /* entries in use (in/out) */
  size_t cap;
  praos_nonce evolving;           /* praosStateEvolvingNonce */
  praos_nonce candidate;          /* praosStateCandidateNonce */
  praos_nonce epoch_nonce;        /* praosStateEpochNonce */
  praos_nonce lab;                /* praosStateLabNonce */
  praos_nonce last_epoch_block;   /* praosStateLastEpochBlockNonce */
} praos_chain_state;

typedef struct {
  uint64_t epoch_base_slot;
  uint64_t epoch_base_no;
  uint64_t epoch_length;          /* > 0 */
  uint64_t stability_window;
} praos_epoch_info;

/* prev_hash: n*32 (hvPrevHash); prev_is_genesis: n flags (GenesisHash), may be NULL. */
int praos_update_chain_dep_state(praos_ctx* ctx, const praos_headers* h, const uint8_t* prev_hash,
                                 const uint8_t* prev_is_genesis, const praos_out* crypto,
                                 const praos_epoch_info* ei, praos_chain_state* st, uint8_t* verdict,
                                 size_t* chain_stop, size_t* processed);

/* ---- PraosState CBOR (checkpoint / resume of a replay) ----
 * Serialise (PraosState c), Praos.hs:274-310: [0, [lastSlot, ocertCounters, evolving,
 * candidate, epoch, lab, lastEpochBlock]].  encode: *len gets the size; PRAOS_E_ARG
 * if cap is too small (call with cap 0 to size).  decode: counters into the caller's
 * arrays (st->cap entries). */
int praos_state_encode(const praos_chain_state* st, uint8_t* out, size_t cap, size_t* len);
int praos_state_decode(const uint8_t* in, size_t len, praos_chain_state* st);

/* ---- validateHeader over a batch (HeaderValidation.hs:413-432) ----
 * The envelope first -- validateEnvelope (:297-344: block number = tip + 1 (0 after
 * Origin), slot >= tip slot + 1 (>= 0 after Origin), prev hash = tip hash (GenesisHash
 * after Origin)) and the Praos additionalEnvelopeChecks (Shelley/Protocol/Praos.hs:66-80:
 * ObsoleteNode, HeaderSizeTooLarge, BlockSizeTooLarge) -- then updateChainDepState as
 * praos_update_chain_dep_state does.  The tip advances with every valid header; on
 * return env's tip (like st) is the one at chain_stop.  Per-header inputs come from
 * the decoder (praos_decoded: block_no, header_hash, body_size; header_size = the
 * stored header length). */
typedef struct {
  const uint64_t* block_no;       /* n: hbBlockNo */
  const uint8_t* header_hash;     /* n*32: headerHash (Blake2b-256 of the header bytes) */
  const uint32_t* header_size;    /* n: bhviewHSize, bytes of the serialised header */
  const uint32_t* body_size;      /* n: bhviewBSize = hbBodySize */
  int32_t tip_is_origin;          /* HeaderState tip before the batch (in / out) */
  uint64_t tip_slot;
  uint64_t tip_block_no;
  uint8_t tip_hash[32];
  uint64_t max_major_pv;          /* praosMaxMajorPV */
  uint64_t lv_prot_major;         /* pvMajor (lvProtocolVersion lv) */
  uint64_t max_header_size;       /* lvMaxHeaderSize */
  uint64_t max_body_size;         /* lvMaxBodySize */
} praos_envelope;

/* The epoch nonce tickChainDepState (Praos.hs:407-431) gives the state at `slot`:
 * candidate ⭒ lastEpochBlock when the slot is in a later epoch than the state's last
 * slot (isNewEpoch), else the current epoch nonce.  What praos_set_epoch needs before
 * validating headers of that slot's epoch.  Pure: st is not changed. */
int praos_ticked_epoch_nonce(const praos_chain_state* st, const praos_epoch_info* ei, uint64_t slot,
                             praos_nonce* out);
/* The TPraos tick (cardano-protocol-tpraos TICKN, TPraos.hs:361-376): candidate ⭒
 * lastEpochBlock ⭒ extra_entropy (NULL = NeutralNonce) on a new epoch. */
int praos_tpraos_ticked_epoch_nonce(const praos_chain_state* st, const praos_epoch_info* ei, uint64_t slot,
                                    const praos_nonce* extra_entropy, praos_nonce* out);

int praos_validate_headers(praos_ctx* ctx, const praos_headers* h, const uint8_t* prev_hash,
                           const uint8_t* prev_is_genesis, const praos_out* crypto, praos_envelope* env,
                           const praos_epoch_info* ei, praos_chain_state* st, uint8_t* verdict, size_t* chain_stop,
                           size_t* processed);

/* praos_validate_headers (env != NULL) / praos_update_chain_dep_state (env == NULL) over
 * outputs verified under per-header nonces (praos_batch_set_nonces): the fold goes on
 * while the nonce the state ticks to at header i equals etas[eta_idx[i]]. */
int praos_validate_headers_nonces(praos_ctx* ctx, const praos_headers* h, const uint8_t* prev_hash,
                                  const uint8_t* prev_is_genesis, const praos_out* crypto, praos_envelope* env,
                                  const praos_epoch_info* ei, praos_chain_state* st, const praos_nonce* etas,
                                  uint32_t k, const uint8_t* eta_idx, uint8_t* verdict, size_t* chain_stop,
                                  size_t* processed);

/* ---- TPraos chain-dependent state: SL.tickChainDepState + SL.updateChainDepState
 *      (TPraos.hs:361-387; cardano-protocol-tpraos TICKN, PRTCL = UPDN + OVERLAY + OCERT)
 * The state has the Praos shape (praos_chain_state: counters = csProtocol's OCert map,
 * evolving / candidate = eta_v / eta_c, epoch_nonce / last_epoch_block = TicknState eta_0 /
 * eta_h, lab = csLabNonce).  Per header: tick on a new epoch: epoch_nonce := candidate ⭒
 * last_epoch_block ⭒ extra_entropy, last_epoch_block := lab; the envelope (env != NULL;
 * chainChecks are the Praos envelope checks); then the predicate failures of PRTCL,
 * collected as the ledger's STS rules collect them (ValidateAll): OVERLAY's
 * Either-chains (first failure within praosVrfChecks / pbftVrfChecks) plus every OCERT
 * predicate, into failures[i] (PRAOS_TPF_*); verdict[i] = PRAOS_V_OK, PRAOS_V_ENV_*,
 * PRAOS_V_INPUT or PRAOS_V_TPRAOS (failures[i] != 0).  On a valid header: eta_v :=
 * eta_v ⭒ mkNonceFromOutputVRF(eta cert), eta_c := eta_v' if slot + window <
 * firstSlotNextEpoch (ei->stability_window: the caller's UPDN window), lab :=
 * prevHashToNonce prev, counters[hk] := n.  chain_stop / processed / state at the stop
 * as praos_update_chain_dep_state. */
#define PRAOS_V_TPRAOS 19
#define PRAOS_TPF_KES_BEFORE_START  0x0001u /* KESBeforeStartOCERT */
#define PRAOS_TPF_KES_AFTER_END     0x0002u /* KESAfterEndOCERT */
#define PRAOS_TPF_OCERT_SIG         0x0004u /* InvalidSignatureOCERT */
#define PRAOS_TPF_KES_SIG           0x0008u /* InvalidKesSignatureOCERT */
#define PRAOS_TPF_COUNTER_MISSING   0x0010u /* NoCounterForKeyHashOCERT */
#define PRAOS_TPF_COUNTER_TOO_SMALL 0x0020u /* CounterTooSmallOCERT */
#define PRAOS_TPF_COUNTER_OVER_INC  0x0040u /* CounterOverIncrementedOCERT */
#define PRAOS_TPF_VRF_KEY_UNKNOWN   0x0100u /* VRFKeyUnknown */
#define PRAOS_TPF_VRF_KEY_WRONG     0x0200u /* VRFKeyWrongVRFKey */
#define PRAOS_TPF_BAD_NONCE         0x0400u /* VRFKeyBadNonce */
#define PRAOS_TPF_BAD_LEADER        0x0800u /* VRFKeyBadLeaderValue */
#define PRAOS_TPF_LEADER_TOO_BIG    0x1000u /* VRFLeaderValueTooBig */
#define PRAOS_TPF_NOT_ACTIVE        0x2000u /* NotActiveSlotOVERLAY */
#define PRAOS_TPF_GEN_COLD          0x4000u /* WrongGenesisColdKeyOVERLAY */
#define PRAOS_TPF_GEN_VRF           0x8000u /* WrongGenesisVRFKeyOVERLAY */
int praos_tpraos_update_chain_dep_state(praos_ctx* ctx, const praos_tpraos_headers* h, const uint8_t* prev_hash,
                                        const uint8_t* prev_is_genesis, const praos_tpraos_out* crypto,
                                        praos_envelope* env, const praos_epoch_info* ei,
                                        const praos_nonce* extra_entropy, praos_chain_state* st, uint8_t* verdict,
                                        uint16_t* failures, size_t* chain_stop, size_t* processed);
/* The same fold over outputs verified under per-header nonces (praos_batch_set_nonces): it
 * goes on while the nonce the state ticks to at header i equals etas[eta_idx[i]]
 * (praos_validate_headers_nonces for TPraos). */
int praos_tpraos_validate_headers_nonces(praos_ctx* ctx, const praos_tpraos_headers* h, const uint8_t* prev_hash,
                                         const uint8_t* prev_is_genesis, const praos_tpraos_out* crypto,
                                         praos_envelope* env, const praos_epoch_info* ei,
                                         const praos_nonce* extra_entropy, praos_chain_state* st,
                                         const praos_nonce* etas, uint32_t k, const uint8_t* eta_idx,
                                         uint8_t* verdict, uint16_t* failures, size_t* chain_stop,
                                         size_t* processed);

/* ---- chain replay from an ImmutableDB directory (db-analyser) ----
 * Replaces the per-block loop of DBAnalyser/Analysis.hs:815-847 (processAllImmutableDB
 * driving benchmarkLedgerOps / validateHeader, :479-607) for the header-validation
 * pass.  Reads dir/NNNNN.chunk + dir/NNNNN.secondary (56-byte Entry per block,
 * Storage/ImmutableDB/Impl/Index/Secondary.hs:93-128) from chunk 0 up in batches of at
 * most batch_max headers (spanning up to 256 epochs).  Each batch is decoded on the
 * device, given per-header epoch nonces (tickChainDepState, Praos.hs:407-431, run ahead
 * over the certified VRF outputs), verified under them (praos_batch_set_nonces) and
 * folded with praos_validate_headers_nonces, which re-derives every nonce it relies on;
 * the fold of batch k overlaps the device work of batch k+1.  One ledger view (pools,
 * params) for the whole replay.  Ends at the first invalid header (stop_index,
 * stop_verdict) or at the end of the database (stop_index = headers).  *st and env's
 * tip are the state and tip after the last valid header; verdicts[i] (i < verdicts_cap,
 * may be NULL with cap 0) for every header up to and including the stop.  Resume: when
 * env's tip is not Origin (a checkpointed state, praos_state_decode), the blocks up to
 * and including the tip (matched by slot and header hash in the secondary index) are
 * skipped; indices count from the first block after it. */
typedef struct {
  uint64_t skipped;               /* blocks up to the resume tip, not replayed */
  uint64_t headers;               /* headers read and judged (through the stop) */
  uint64_t validated;             /* valid headers folded into *st */
  uint64_t stop_index;            /* first invalid header, or headers when none */
  uint32_t stop_verdict;          /* its PRAOS_V_* (0 when none) */
  uint32_t epochs;                /* distinct epoch nonces the headers were verified under */
  uint32_t batches;               /* device passes */
  uint32_t chunks;                /* chunk files read */
  double ms_io;                   /* reading chunks + secondary indexes, building batches */
  double ms_device;               /* upload + decode + crypto + download */
  double ms_fold;                 /* envelope + updateChainDepState on the host */
  double ms_nonce;                /* epoch nonces ahead of the crypto (host) */
} praos_replay_stats;

int praos_replay_immutable(praos_ctx* ctx, const char* dir, const praos_pool* pools, uint32_t npools,
                           const praos_params* params, const praos_epoch_info* ei, praos_envelope* env,
                           praos_chain_state* st, size_t batch_max, uint8_t* verdicts, size_t verdicts_cap,
                           praos_replay_stats* stats);
/* ABI 14.  The ledger view per epoch, as db-analyser sources it: the reference forecasts each
 * header's LedgerView from the ledger state it advances block by block (Analysis.hs:564-572,
 * ledgerViewForecastAt over applyTheBlock; Shelley/Ledger/SupportsProtocol.hs:100-125: lvPoolDistr
 * = nesPd, lvMaxHeaderSize / lvMaxBodySize / lvProtocolVersion from the epoch's protocol
 * parameters).  All of them change only at an epoch boundary (the NEWEPOCH rule), so one view
 * per epoch is the reference's per-header forecast.  views[] is sorted by first_epoch; epoch e
 * uses the last entry with first_epoch <= e (a view holds until the next entry's epoch). */
typedef struct {
  uint64_t first_epoch;
  const praos_pool* pools;        /* lvPoolDistr: hash28, VRF key hash, sigma (Fixed E34) */
  uint32_t npools;
  uint32_t reserved;              /* 0 */
  uint64_t lv_prot_major;         /* pvMajor (lvProtocolVersion) */
  uint64_t max_header_size;       /* lvMaxHeaderSize */
  uint64_t max_body_size;         /* lvMaxBodySize */
} praos_ledger_view;

/* praos_replay_immutable with a ledger view per epoch instead of one for the whole replay: a
 * batch never spans two views; each member's device gets a view's pool tables (hash, VRF key
 * hash, leader threshold x = -(sigma * c)) before the first batch that needs them, and the fold
 * of a batch uses that batch's view (PoolDistr membership for the OCert counters, the envelope
 * limits; env's limit fields are ignored).  Everything else -- pipeline, stop, resume, outputs --
 * as praos_replay_immutable.  PRAOS_E_ARG when no view covers a replayed epoch. */
int praos_replay_immutable_views(praos_ctx* ctx, const char* dir, const praos_ledger_view* views, uint32_t nviews,
                                 const praos_params* params, const praos_epoch_info* ei, praos_envelope* env,
                                 praos_chain_state* st, size_t batch_max, uint8_t* verdicts, size_t verdicts_cap,
                                 praos_replay_stats* stats);
/* The same replay over a TPraos (Shelley..Alonzo) ImmutableDB: stored BHeaders, the TPraos
 * nonce rules (mkNonceFromOutputVRF of the eta certificate; TICKN with extra_entropy, NULL
 * = NeutralNonce) and the TPraos fold; failures (may be NULL, verdicts_cap entries) gets
 * each header's PRAOS_TPF_* set.  Replaces db-analyser's header revalidation over the
 * TPraos eras (TPraos.hs:361-387 per block). */
int praos_replay_immutable_tpraos(praos_ctx* ctx, const char* dir, const praos_pool* pools, uint32_t npools,
                                  const praos_params* params, const praos_epoch_info* ei,
                                  const praos_nonce* extra_entropy, praos_envelope* env, praos_chain_state* st,
                                  size_t batch_max, uint8_t* verdicts, uint16_t* failures, size_t verdicts_cap,
                                  praos_replay_stats* stats);

/* ---- headers as the ChainSync client receives them (call stack 3) ----
 * A header arrives in the node-to-node encoding, not as a chunk-file span:
 *   Shelley-based eras  [eraIndex, #6.24(bytes)]  (decodeNS,
 *       HardFork/Combinator/Serialisation/Common.hs:451-463; Shelley/Node/Serialisation.hs:110-112)
 *   Byron               [0, [[kind, sizeHint], #6.24(bytes)]]  (Byron/Node/Serialisation.hs:83-99,
 *       version 2; kind 0 = EBB, 1 = main header)
 * The wire era index is not the disk tag (Babbage: 5 on the wire, 6 on disk).
 * praos_unwrap_wire_headers finds the inner header bytes of each item of `items` (spans are wire
 * items) on the device: status, era (the wire index, 0xff when not read), byron_kind (0 / 1, 0xff
 * outside Byron), size_hint (Byron), the inner span (off, len: into the same arena) and, when
 * header_hash is not NULL, the header hash: Blake2b-256 of the inner bytes for a Shelley-based item,
 * Blake2b-256(82 0k || header) for a Byron one (what praos_verify_pbft_headers reports).  Items
 * that do not unwrap have zero span and hash.  Heads of any width are taken (cborg's decoders
 * accept non-shortest forms); lists and the byte string must be definite; the tag must be 24; an
 * era index >= n_eras (7 for the reference's CardanoBlock) is PRAOS_WIRE_ERA; bytes after the item
 * inside its span are PRAOS_WIRE_TRAILING; Byron: kind 0 or 1, the hint fits 32 bits.  A TPraos or
 * Byron caller passes the inner spans on to praos_verify_tpraos_header_bytes /
 * praos_verify_pbft_headers. */
#define PRAOS_WIRE_OK       0
#define PRAOS_WIRE_RANGE    1 /* span outside the arena */
#define PRAOS_WIRE_SYNTAX   2 /* truncated, wrong type / length / tag, indefinite, kind > 1, hint > 32 bits */
#define PRAOS_WIRE_ERA      3 /* era index >= n_eras */
#define PRAOS_WIRE_TRAILING 4 /* bytes after the item within its span */
typedef struct {
  uint8_t* status;                /* n: PRAOS_WIRE_* */
  uint8_t* era;                   /* n */
  uint8_t* byron_kind;            /* n */
  uint32_t* size_hint;            /* n */
  uint64_t* off;                  /* n: inner header = bytes[off[i], off[i] + len[i]) */
  uint32_t* len;                  /* n */
  uint8_t* header_hash;           /* n*32, may be NULL */
} praos_wire_out;
int praos_unwrap_wire_headers(praos_ctx* ctx, const praos_header_bytes* items, uint32_t n_eras, praos_wire_out* out);

/* K candidate fragments of wire headers, each from its own HeaderState, in one call: what the
 * ChainSync clients of K peers do header by header (MiniProtocol/ChainSync/Client.hs:794-812:
 * the DoesntFit check against the fragment's head, then validateHeader).  The items are unwrapped
 * and hashed on the device, byte-identical headers (same era, same Blake2b-256) are found there,
 * and the header crypto runs once per distinct (header, epoch nonce) pair -- a row; each
 * fragment is then folded on the host from its own state, reading rows through the item-to-row
 * map.  One ledger view per call: the pools and parameters of praos_set_epoch, the limits below.
 *   verdict[i]: PRAOS_V_DOESNT_FIT when the header's prevHash is not the fragment's head hash
 *   (checked before the envelope, so never PRAOS_V_ENV_PREV_HASH); else validateHeader's verdict as
 *   praos_validate_headers_nonces gives it; PRAOS_V_INPUT for an item that did not unwrap, is of
 *   an era outside praos_eras or did not decode.  The client disconnects at the first failure:
 *   items after a fragment's chain_stop are PRAOS_V_NOT_REACHED, and so are the items from the
 *   first header with slot >= view_end_slot on (the forecast does not reach them: the client
 *   waits).  processed = items judged (through the stop, or up to the forecast horizon);
 *   chain_stop = first invalid item, or processed when none.  Each fragment's tip and state are
 *   those at its chain_stop.
 * Rows are numbered in order of first appearance (a header's first nonce takes the row of its
 * first item; a further nonce for the same bytes appends an extra row), so outputs do not depend
 * on scheduling.  PRAOS_E_ARG: rows_cap too small (n_rows = the count needed); more than 256
 * distinct epoch nonces (n_etas = the count). */
#define PRAOS_V_DOESNT_FIT  25  /* ChainSync DoesntFit: prevHash is not the candidate's head */
#define PRAOS_V_NOT_REACHED 255 /* after the fragment's stop, or beyond the forecast horizon */
#define PRAOS_NO_ROW 0xffffffffu
typedef struct {
  praos_header_bytes items;       /* N wire items, fragment after fragment */
  uint32_t n_eras;                /* eras of the block type (7) */
  uint32_t praos_eras;            /* bit mask of the wire indices judged here; 0 = (1 << 5) | (1 << 6) */
  uint64_t view_end_slot;         /* first slot the ledger view does not cover */
  praos_epoch_info ei;
  uint64_t max_major_pv;          /* the envelope limits (praos_envelope) */
  uint64_t lv_prot_major;
  uint64_t max_header_size;
  uint64_t max_body_size;
} praos_candidates_in;
typedef struct {
  int32_t tip_is_origin;          /* the fragment's head before the call (in / out) */
  uint64_t tip_slot;
  uint64_t tip_block_no;
  uint8_t tip_hash[32];
  praos_chain_state state;        /* in / out; counter arrays with room (cap) */
  size_t chain_stop;              /* out: relative to the fragment's first item */
  size_t processed;               /* out */
} praos_fragment;
typedef struct {
  size_t k;
  const size_t* frag_first;       /* k + 1: fragment j = items [frag_first[j], frag_first[j + 1]) */
  praos_fragment* frag;           /* k */
} praos_fragments;
typedef struct {
  uint8_t* wire_status;           /* N: PRAOS_WIRE_* */
  uint32_t* row;                  /* N: the item's row, PRAOS_NO_ROW when it has none */
  uint8_t* verdict;               /* N */
  size_t rows_cap;
  size_t n_rows;                  /* out */
  praos_out rows;                 /* rows_cap per array (bits may be NULL here) */
  praos_decoded dec;              /* rows_cap per array */
  uint8_t* eta_idx;               /* rows_cap, may be NULL: the row's nonce, index into etas */
  praos_nonce* etas;              /* 256, may be NULL */
  uint32_t n_etas;                /* out */
  uint64_t stats[5];              /* out: items, unwrapped Praos items, distinct headers, rows, extra rows */
} praos_candidates_out;
int praos_validate_candidates(praos_ctx* ctx, const praos_candidates_in* in, praos_fragments* frags,
                              praos_candidates_out* out);

/* The same call for the TPraos eras (Shelley .. Alonzo, wire indices 1 to 4; additive: ABI version
 * unchanged).  in: praos_candidates_in's fields with tpraos_eras (a bit mask of wire indices, 0 =
 * indices 1 to 4) in the place of praos_eras, and extra_entropy (TICKN's, may be NULL, as
 * praos_replay_immutable_tpraos takes it): each fragment's speculative nonce chain combines it at
 * every epoch tick, so two fragments that differ only in what they tick to land on different rows.
 * Fragments are praos_fragments.  The rows are decoded as praos_verify_tpraos_header_bytes decodes
 * them (the 15-field BHBody; dec's signed_body has the PRAOS_TP_SIGNED_STRIDE stride) and verified
 * by its kernels under the per-row nonces; the overlay installed with praos_set_overlay applies.
 *   verdict[i]: PRAOS_V_DOESNT_FIT before the envelope; then the envelope verdicts; then
 *   PRAOS_V_TPRAOS with failures[i] = the PRAOS_TPF_* set (0 with every other verdict);
 *   PRAOS_V_INPUT / PRAOS_V_NOT_REACHED as above.
 * rows_cap, n_rows, eta_idx, etas, n_etas, stats and the two PRAOS_E_ARG cases as above. */
typedef struct {
  praos_header_bytes items;       /* N wire items, fragment after fragment */
  uint32_t n_eras;                /* eras of the block type (7) */
  uint32_t tpraos_eras;           /* bit mask of the wire indices judged here; 0 = indices 1 to 4 */
  uint64_t view_end_slot;         /* first slot the ledger view does not cover */
  praos_epoch_info ei;
  uint64_t max_major_pv;          /* the envelope limits (praos_envelope) */
  uint64_t lv_prot_major;
  uint64_t max_header_size;
  uint64_t max_body_size;
  const praos_nonce* extra_entropy; /* may be NULL */
} praos_tpraos_candidates_in;
typedef struct {
  uint8_t* wire_status;           /* N: PRAOS_WIRE_* */
  uint32_t* row;                  /* N: the item's row, PRAOS_NO_ROW when it has none */
  uint8_t* verdict;               /* N */
  uint16_t* failures;             /* N, may be NULL: PRAOS_TPF_* of an item judged PRAOS_V_TPRAOS, else 0 */
  size_t rows_cap;
  size_t n_rows;                  /* out */
  praos_tpraos_out rows;          /* rows_cap per array (any may be NULL) */
  praos_decoded dec;              /* rows_cap per array; signed_body at PRAOS_TP_SIGNED_STRIDE */
  uint8_t* leader_out;            /* rows_cap*64, may be NULL */
  uint8_t* leader_proof;          /* rows_cap*80, may be NULL */
  uint8_t* eta_idx;               /* rows_cap, may be NULL: the row's nonce, index into etas */
  praos_nonce* etas;              /* 256, may be NULL */
  uint32_t n_etas;                /* out */
  uint64_t stats[5];              /* out: items, unwrapped TPraos items, distinct headers, rows, extra rows */
} praos_tpraos_candidates_out;
int praos_validate_candidates_tpraos(praos_ctx* ctx, const praos_tpraos_candidates_in* in, praos_fragments* frags,
                                     praos_tpraos_candidates_out* out);

/* The same for K candidate fragments of Byron wire headers (wire index 0), each from its own tip
 * and PBftState (additive: ABI version unchanged).  The items are unwrapped, hashed and
 * deduplicated on the device as above -- the key is (era 0, Blake2b-256(82 0k || header)), so the
 * same bytes sent as EBB and as main header are two rows, and size_hint is no part of it -- then
 * praos_verify_pbft_headers' kernels run once per row, straight from the wire arena, under its
 * rules (delegs: the Bimap, a duplicate in either column is PRAOS_E_ARG; PRAOS_OPT_KEYCACHE and
 * praos_pbft_stats apply to the rows), and each fragment is folded on the host as
 * praos_pbft_update_chain_dep_state folds, in the client's mode:
 *   verdict[i]: PRAOS_V_INPUT for an item that did not unwrap, is not of era 0 or whose header
 *   has PRAOS_PBFT_BIT_DECODE; PRAOS_V_DOESNT_FIT when the header's prev hash is not the
 *   fragment's tip hash (at an Origin tip: not the genesis hash), checked before the envelope, so
 *   never PRAOS_V_ENV_PREV_HASH; else the fold's verdict and aux.  The fold ends at the first
 *   failure; items after it, and the items from the first slot >= view_end_slot on, are
 *   PRAOS_V_NOT_REACHED (aux 0).  processed / chain_stop as in praos_fragment; tip and state on
 *   return are those at chain_stop.  Every state needs cap >= window_size > 0.
 * Rows are numbered by first appearance; there is no nonce, so rows = distinct headers.
 * PRAOS_E_ARG: rows_cap too small (n_rows = the count needed), before any signature is verified. */
typedef struct {
  praos_header_bytes items;       /* N wire items, fragment after fragment */
  uint32_t n_eras;                /* eras of the block type (7) */
  uint32_t n_delegs;
  uint64_t view_end_slot;         /* first slot the ledger view does not cover */
  praos_pbft_params params;
  const uint8_t* delegs;          /* n_delegs * 56 */
} praos_pbft_candidates_in;
typedef struct {
  praos_pbft_tip tip;             /* in / out */
  praos_pbft_state state;         /* in / out; cap >= window_size */
  size_t chain_stop;              /* out: relative to the fragment's first item */
  size_t processed;               /* out */
} praos_pbft_fragment;
typedef struct {
  size_t k;
  const size_t* frag_first;       /* k + 1 */
  praos_pbft_fragment* frag;      /* k */
} praos_pbft_fragments;
typedef struct {
  uint8_t* wire_status;           /* N: PRAOS_WIRE_* */
  uint32_t* row;                  /* N: the item's row, PRAOS_NO_ROW when it has none */
  uint8_t* verdict;               /* N */
  uint64_t* aux;                  /* N, may be NULL: as praos_pbft_update_chain_dep_state reports it */
  size_t rows_cap;
  size_t n_rows;                  /* out */
  praos_pbft_out rows;            /* rows_cap per array; any may be NULL */
  uint8_t* row_is_ebb;            /* rows_cap, may be NULL: the row's Byron kind is 0 */
  uint64_t stats[4];              /* out: items, unwrapped Byron items, distinct headers (= rows), signature verifies run */
} praos_pbft_candidates_out;
int praos_validate_candidates_pbft(praos_ctx* ctx, const praos_pbft_candidates_in* in, praos_pbft_fragments* frags,
                                   praos_pbft_candidates_out* out);

/* ---- several GPUs from one process ----
 * A group = one context per entry of devices[] (a device may repeat: several
 * contexts on one GPU), each driven by its own host thread.  Batch calls split the
 * n headers into contiguous shards (member k: [n*k/m, n*(k+1)/m)), run them
 * concurrently and write every output in place, so the caller's arrays look exactly
 * as after the single-context call.  The fold (praos_validate_headers) then runs
 * over the gathered outputs on praos_group_ctx(g, 0).  No exchange between devices
 * (headers of one epoch are independent, Praos.hs:441-459). */
typedef struct praos_group praos_group;
praos_group* praos_group_open(const int* devices, int ndev);     /* NULL on failure */
void praos_group_close(praos_group* g);
int praos_group_size(praos_group* g);
praos_ctx* praos_group_ctx(praos_group* g, int k);               /* member k's context */
const char* praos_group_last_error(praos_group* g);
int praos_group_set_option(praos_group* g, int opt, int value);
int praos_group_set_epoch(praos_group* g, const uint8_t eta0[32], const praos_pool* pools, uint32_t npools,
                          const praos_params* params);
int praos_group_verify_headers(praos_group* g, const praos_headers* h, praos_out* out);
int praos_group_verify_header_bytes(praos_group* g, const praos_header_bytes* in, praos_out* out,
                                    praos_decoded* dec);
/* TPraos batches over the group (ABI 12): praos_verify_tpraos_headers /
 * praos_verify_tpraos_header_bytes per shard (TPraos.hs:378-387), outputs in place; dec's
 * signed_body has the PRAOS_TP_SIGNED_STRIDE stride, leader_out / leader_proof may be NULL. */
int praos_group_verify_tpraos_headers(praos_group* g, const praos_tpraos_headers* h, praos_tpraos_out* out);
int praos_group_verify_tpraos_header_bytes(praos_group* g, const praos_header_bytes* in, praos_tpraos_out* out,
                                           praos_decoded* dec, uint8_t* leader_out, uint8_t* leader_proof);
/* ABI 13.  A caller buffer page-locked once for every member (the Haskell arena of an epoch:
 * each member's shard uploads by direct DMA), and the ImmutableDB replay over the group
 * (db-analyser's processAllImmutableDB, DBAnalyser/Analysis.hs:815-847, on several GPUs):
 * consecutive batches are dealt to the members in turn, the nonce chain and the fold
 * (envelope + updateChainDepState) run once in chain order on member 0; arguments, outputs,
 * stop and resume exactly as praos_replay_immutable[_tpraos] on one context. */
int praos_group_set_overlay(praos_group* g, const praos_overlay* ov);   /* praos_set_overlay on every member */
int praos_group_host_register(praos_group* g, void* p, size_t len);
int praos_group_host_unregister(praos_group* g, void* p);
int praos_group_replay_immutable(praos_group* g, const char* dir, const praos_pool* pools, uint32_t npools,
                                 const praos_params* params, const praos_epoch_info* ei, praos_envelope* env,
                                 praos_chain_state* st, size_t batch_max, uint8_t* verdicts, size_t verdicts_cap,
                                 praos_replay_stats* stats);
int praos_group_replay_immutable_tpraos(praos_group* g, const char* dir, const praos_pool* pools, uint32_t npools,
                                        const praos_params* params, const praos_epoch_info* ei,
                                        const praos_nonce* extra_entropy, praos_envelope* env, praos_chain_state* st,
                                        size_t batch_max, uint8_t* verdicts, uint16_t* failures, size_t verdicts_cap,
                                        praos_replay_stats* stats);
/* ABI 14: praos_verify_block_integrity over the group (ImmutableDB chunk validation on several
 * GPUs: contiguous shards of the blocks, results in place). */
int praos_group_verify_block_integrity(praos_group* g, const praos_header_bytes* blocks,
                                       uint64_t slots_per_kes_period, uint8_t* result, uint8_t* body_hash);
/* ABI 14: praos_replay_immutable_views over the group. */
int praos_group_replay_immutable_views(praos_group* g, const char* dir, const praos_ledger_view* views,
                                       uint32_t nviews, const praos_params* params, const praos_epoch_info* ei,
                                       praos_envelope* env, praos_chain_state* st, size_t batch_max,
                                       uint8_t* verdicts, size_t verdicts_cap, praos_replay_stats* stats);

/* ---- synthetic chain generator (db-synthesizer analogue, for benches) ----
 * Signs on the GPU: OCert (Ed25519), Sum6KES (Blake2b-256 tree + Ed25519 leaf),
 * VRF draft-03 proofs for alpha = mkInputVRF(slot, eta0).  Keys derive from
 * 32-byte seeds: cold/VRF/KES seed of pool i = Blake2b-256(tag || seed || i). */
typedef struct {
  uint64_t n;                     /* headers */
  uint32_t npools;
  uint64_t first_slot;
  uint64_t slot_stride;           /* slot of header i = first_slot + i * slot_stride */
  uint32_t body_len;              /* > 0: pseudo-random signed bodies of this length;
                                     0: the genuine canonical HeaderBody CBOR of each header
                                     (PRAOS_SIGNED_STRIDE bytes per header; praos_synthesize_tpraos:
                                     the 15-field BHBody, PRAOS_TP_SIGNED_STRIDE bytes) */
  uint32_t corrupt_per_10000;     /* seeded corruptions (Corruption.hs model: +1 at a byte) */
  uint32_t nkes;                  /* distinct Sum6KES keys (0 = one per pool); header of pool p uses key p mod nkes */
  uint8_t seed[32];
  const uint8_t* body_hash;       /* n*32 hbBodyHash of each CBOR body (e.g. hashTxSeq of the block's
                                     segments, for stored-block corpora); NULL = pseudo-random */
  /* Leader schedule (from praos_leader_schedule): header i is forged in slot
   * sched_slot[i] by pool sched_pool[i], blockNo = block_no0 + i.  NULL: slot of
   * header i = first_slot + i * slot_stride and pools assigned by hash -- such a
   * chain is NOT leader-valid (most headers fail VRFLeaderValueTooBig). */
  const uint64_t* sched_slot;
  const uint32_t* sched_pool;
  uint64_t block_no0;
  /* Chain linking (CBOR bodies, Praos or TPraos): link_prev = 1 makes hbPrev of header i the
   * headerHash of header i-1 -- header 0 gets prev0, or GenesisHash when prev0 is NULL --
   * re-signing each KES signature in order (sequential on the device: ~0.1 ms per
   * header).  header_hash (optional, n*32) receives the header hashes (before any
   * seeded corruption). */
  int32_t link_prev;
  const uint8_t* prev0;
  uint8_t* header_hash;
  /* Fields the seeded corruptions may hit (PRAOS_CORRUPT_* bits; 0 = all five: OCert
   * signature, KES signature, VRF proof, VRF output, signed body), so a single-primitive
   * batch corrupts only what its check reads (configs[1..3]: 1 % means 1 %). */
  uint32_t corrupt_fields;
} praos_synth_params;

#define PRAOS_CORRUPT_OCERT     0x01u  /* +1 at a byte of cold vk || hot vk || BE64 n || BE64 c0 || sigma
                                          (the 144 bytes of an OCert verify; signature only for CBOR bodies) */
#define PRAOS_CORRUPT_KES_SIG   0x02u
#define PRAOS_CORRUPT_VRF_PROOF 0x04u
#define PRAOS_CORRUPT_VRF_OUT   0x08u
#define PRAOS_CORRUPT_BODY      0x10u

/* Fills caller buffers (same layout as praos_headers; body_off/body_len/body_bytes
 * sized n, n, n*stride+8 with stride = round_up(body_len, 8), or PRAOS_SIGNED_STRIDE
 * when body_len = 0).  Also returns the pool table
 * (npools entries, sigma_fp left for the caller to set). */
int praos_synthesize(praos_ctx* ctx, const praos_synth_params* sp, const praos_params* params,
                     const uint8_t eta0[32], praos_pool* pools_out, uint64_t* slot, uint8_t* cold_vk,
                     uint8_t* vrf_vk, uint8_t* vrf_out, uint8_t* vrf_proof, uint8_t* hot_vk, uint64_t* ocert_n,
                     uint64_t* ocert_c0, uint8_t* ocert_sig, uint8_t* kes_sig, uint64_t* body_off,
                     uint32_t* body_len, uint8_t* body_bytes, uint8_t* corrupted);

/* Leader schedule of the generator's pools (db-synthesizer, Forging.hs:139-148):
 * the pools derived from `seed` (as praos_synthesize derives them, npools of them,
 * stake sigma_fp[p], Fixed E34 raw uint128 LE) are the forgers, tried in index
 * order.  For every slot s in [first_slot, first_slot + nslots): leader[s -
 * first_slot] = the first pool p for which checkIsLeader holds (Praos.hs:375-397:
 * meetsLeaderThreshold, :505-526, on evalCertified (mkInputVRF s eta0) under p's
 * VRF key), or -1 (no block in that slot).  tpraos = 1: the TPraos leader cert
 * (mkSeed seedL, 64-byte output, bound 2^512).  Cost: one VRF evaluation per
 * (slot, pool) pair up to the slot's leader, i.e. ~npools per empty slot. */
int praos_leader_schedule(praos_ctx* ctx, const uint8_t seed[32], uint32_t npools, const uint8_t* sigma_fp,
                          const praos_params* params, const uint8_t eta0[32], uint64_t first_slot, uint64_t nslots,
                          int tpraos, int32_t* leader);

/* TPraos variant of the generator: the VRF cert pair uses mkSeed alphas;
 * leader_out/leader_proof receive the leader cert (n*64, n*80). */
int praos_synthesize_tpraos(praos_ctx* ctx, const praos_synth_params* sp, const praos_params* params,
                            const uint8_t eta0[32], praos_pool* pools_out, uint64_t* slot, uint8_t* cold_vk,
                            uint8_t* vrf_vk, uint8_t* vrf_out, uint8_t* vrf_proof, uint8_t* hot_vk, uint64_t* ocert_n,
                            uint64_t* ocert_c0, uint8_t* ocert_sig, uint8_t* kes_sig, uint64_t* body_off,
                            uint32_t* body_len, uint8_t* body_bytes, uint8_t* leader_out, uint8_t* leader_proof,
                            uint8_t* corrupted);

/* ---- self-test entry points (unit tests of the device arithmetic) ---- */
/* op: 0 mul, 1 sq, 2 add, 3 sub, 4 invert (the build's: binary GCD unless PRAOS_INV_GCD=0), 5 pow22523,
   6 canon, 7 invert by Fermat's z^(p-2), 8 invert by the binary GCD; inputs/outputs n*32 bytes LE */
int praos_debug_fe(praos_ctx* ctx, int op, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* r);
/* SHA-512 of (64-byte prefix || msg) per item; out n*64 */
int praos_debug_sha512(praos_ctx* ctx, size_t n, const uint8_t* prefix, const uint64_t* msg_off,
                       const uint32_t* msg_len, const uint8_t* msg_bytes, size_t msg_bytes_len, uint8_t* out);
/* BLAKE2b-256 of 64-byte inputs; out n*32 */
int praos_debug_blake2b(praos_ctx* ctx, size_t n, const uint8_t* in64, uint8_t* out);
/* x mod L for 64-byte inputs; out n*32 */
int praos_debug_sc_reduce(praos_ctx* ctx, size_t n, const uint8_t* in64, uint8_t* out);
/* decode point (1 = ok) and re-encode; out n*32, ok n */
int praos_debug_decode(praos_ctx* ctx, size_t n, const uint8_t* in32, uint8_t* out, uint8_t* ok);
/* [s]B for 32-byte scalars (< 2^255); out n*32 */
int praos_debug_scalarmult_base(praos_ctx* ctx, size_t n, const uint8_t* s, uint8_t* out);
/* leader check with explicit x_raw per item (4 words LE); is_leader, iters out */
int praos_debug_leader(praos_ctx* ctx, size_t n, const uint8_t* leader, const uint8_t* x_raw16, uint8_t* is_leader,
                       int32_t* iters);
/* the same for the TPraos form: 64-byte big-endian leader values, bound 2^512 */
int praos_debug_leader512(praos_ctx* ctx, size_t n, const uint8_t* leader64, const uint8_t* x_raw16,
                          uint8_t* is_leader, int32_t* iters);
/* Elligator2 hash-to-curve of the VRF suite: h(pk, alpha); out n*32 */
int praos_debug_hash_to_curve(praos_ctx* ctx, size_t n, const uint8_t* pk, const uint8_t* alpha, uint8_t* out);

/* ---- additions (ABI stays 15): self tests of the field products, the group formulas and the
 * scalar-multiplication schedules.  Field elements are 32 bytes LE, any value below 2^256. ----
 *
 * praos_debug_fe, further ops: 9 neg, 10 chi (Legendre symbol z^((p-1)/2)), 11 predicates
 * (byte 0 = fe_iszero | fe_isnegative << 1, other bytes 0), 12 mul with r the object a,
 * 13 mul with r the object b, 14 sq with r the object a.
 *
 * praos_debug_fe_multi: the interleaved products.  in n*8*32: a1 b1 a2 b2 a3 b3 a4 b4; out n*4*32:
 * r1 .. r4 (outputs an op does not have are 0).  op: 0 fe_mul2, 1 fe_sq2, 2 fe_mul3, 3 fe_mul4,
 * 4 fe_sq4 (squarings read a only); op | 8: the aliased form, in which output m is the very object
 * that product (m + 1) mod M reads as its b (multiplies) or its a (squarings). */
int praos_debug_fe_multi(praos_ctx* ctx, int op, size_t n, const uint8_t* in, uint8_t* out);
/* One group formula per item on raw coordinates.  build: 0 the default formulas (fe_mul2 / fe_sq2),
 * 1 the ILP-4 module's (fe_mul3 / fe_mul4 / fe_sq4).  p, q, out: n*128 bytes, four field elements:
 * p3 and p1p1 X,Y,Z,T; p2 X,Y,Z,(ignored / 0); cached YpX,YmX,Z,T2d; niels ypx,ymx,xy2d,(ignored / 0).
 *   op 0 ge_p2_dbl          p p2                -> p1p1
 *   op 1 ge_add             p p3, q cached      -> p1p1
 *   op 2 ge_madd            p p3, q niels       -> p1p1
 *   op 3 ge_p1p1_to_p2      p p1p1              -> p2
 *   op 4 ge_p1p1_to_p3      p p1p1              -> p3
 *   op 5 ge_p3_to_cached    p p3                -> cached
 *   op 6 ge_p3_dbl_to_p3    p p3                -> p3
 *   op 7 build_cached_table(p) then select_cached with the digit d in [-8, 7]   -> cached ([d]p)
 *   op 8 select_niels over the context's table {1..128} 256^t B, d in [-128, 127], t < 32 -> niels
 * Ops 7 and 8 read d (int32 LE) from q's bytes 0..3 and t (uint32 LE) from bytes 4..7; a digit or
 * table out of range is PRAOS_E_ARG.  q is ignored by the other unary ops. */
int praos_debug_ge(praos_ctx* ctx, int build, int op, size_t n, const uint8_t* p, const uint8_t* q, uint8_t* out);
/* The scalar-multiplication chains with the product code's templates and arguments; out n*32, the
 * encoding of each item's result.  P, Q: n*32 point encodings (decoded as the product decodes
 * them); sp, sq, sb: n*32 scalars LE.  The product tables hold -A and -Y, so do these:
 *   variant 0  [sb]B - [sp]P   STRAUS<64,64,0,32,false>   (ed25519_verify_core)
 *   variant 1  [sb]B - [sp]P   STRAUS<33,33,0,16,true>    (uncached VRF U), sp < 2^128
 *   variant 2  [sp]P - [sq]Q   STRAUS<64,64,33,0,false>   (VRF V), sq < 2^128
 *   variant 3  [sb]B - [sp]P   straus_comb<16,false> over key tables of kind 0 and the 2^16 comb
 *   variant 4  [sb]B - [sp]P   straus_comb<8,true> over key tables of kind 1, sp < 2^128
 *   variant 5  [sp]P           ge_scalarmult_var
 *   variant 6  [sb]B - [sp]P   straus_pos over the wide tables of kind 1 and the 2^16 comb,
 *                              sp < 2^128, n <= 4096
 * Variants 3 and 4 build their tables with the key cache's own precompute (entry e = key e; its
 * first pass from the ILP-4 module when build = 1).  Arguments a variant does not use may be
 * null.  A scalar outside the recodings' range (sp, sb < 2^253; sq, and sp where noted, < 2^128)
 * is PRAOS_E_ARG. */
int praos_debug_msm(praos_ctx* ctx, int variant, int build, size_t n, const uint8_t* P, const uint8_t* Q,
                    const uint8_t* sp, const uint8_t* sq, const uint8_t* sb, uint8_t* out);

/* ---- addition (ABI stays 15): self test of the hashes over stored bytes.  The arena is uploaded
 * as the product paths upload theirs (length rounded up to 8, then 16 zero bytes); every kind
 * runs the product routine on it, one digest per item.  off / len are the item table:
 *   kind 0  b2b256_range(arena, off[i], len[i])                                   out n*32
 *   kind 1  b2b256_pre(arena, off[i], len[i], npre, pre): Blake2b-256 of the npre literal bytes
 *           followed by the range.  aux n*4: byte 0 npre (0..2), bytes 1..2 the literal bytes,
 *           byte 3 ignored.  off[i] >= npre (the routine overwrites the bytes before the range
 *           in registers)                                                        out n*32
 *   kind 2  the block check's own segment-hash kernel: off / len are seg_off / seg_len, 4n
 *           entries segment-major ([k][i]), aux n bytes nseg (0..4); slot (k, i) is hashed when
 *           k < nseg[i]                                out 4n*32, segment-major, 0 where inactive
 *   kind 3  the SHA-512 register stream (Byron's signed message), then its finalisation  out n*64
 *   kind 4  the Blake2b-256 register stream (Byron's witness hash)                        out n*32
 * Kinds 3 and 4: item i is the concatenation of parts off[i] .. off[i] + len[i] - 1 of the part
 * table, n_parts pairs of 64-bit words (a, b): b < 2^63 is the arena range [a, a + b) (b = 0: an
 * empty part); b = 2^63 | k, k in 1..8, is a literal, the k low bytes of a in little-endian order.
 * Parts are fed 8 bytes at a time and then the rest, as the Byron kernels feed theirs.
 * aux is unused by kinds 0, 3, 4 and parts by kinds 0 .. 2; either may be null there.
 * PRAOS_E_ARG, with nothing launched: an unknown kind, a range or segment that does not lie inside
 * [0, arena_len), kind 1 with npre > 2 or off < npre, nseg > 4, a part index outside the table, a
 * literal length outside 1..8, a part longer than the arena.  PRAOS_E_STATE on a host-only context. */
int praos_debug_hash_bytes(praos_ctx* ctx, int kind, size_t n, const uint8_t* arena, size_t arena_len,
                           const uint64_t* off, const uint32_t* len, const uint8_t* aux, const uint64_t* parts,
                           size_t n_parts, uint8_t* out);

/* ---- addition (ABI stays 15): self test of the integer routines under every verdict: scalars
 * mod L (sc25519.hpp), the signed-digit recoders (scalarmult.hpp) and the Fixed E34 helpers of the
 * leader check (leader.hpp).  One item per lane runs the product routine unchanged.  a, b, c, out:
 * n*32 bytes, eight 32-bit words LE per item; arrays an op does not read may be null.
 *   op 0  sc_reduce256    a mod L                                             out 8 words
 *   op 1  sc_muladd       (a * b + c) mod L, any 256-bit a, b, c               out 8 words
 *   op 2  sc_is_canonical a < L                                               out word 0 = 0 / 1
 *   op 3  sc_recode16     a + 0x88..88, a < 2^253                              out 8 words
 *   op 4  sc_recode256    a + 0x80..80, a < 2^253                              out 8 words
 *   op 5  sc_recode65536  a + 0x8000..8000, a < 2^253                          out 8 words
 *   op 6  sc_recode64     a + sum_k 32 * 64^k (k < 22), a < 2^128              out 5 words
 *   op 7  fx_div_R        floor(a / 10^34), any 256-bit a                      out 8 words
 *   op 8  mp_div_small    floor(a / k), k = word 0 of b, 2 <= k < 65536        out 8 words
 * Words of out an op does not write are 0.  (x mod L for 512-bit x is praos_debug_sc_reduce.)
 * PRAOS_E_ARG, with nothing launched and praos_last_error naming the function: an unknown op, a
 * null array the op reads when n > 0, a scalar outside the recoder's range (ops 3 .. 6), a divisor
 * outside 2 .. 65535 (op 8).  n = 0 is PRAOS_OK.  PRAOS_E_STATE on a host-only context. */
int praos_debug_int(praos_ctx* ctx, int op, size_t n, const uint8_t* a, const uint8_t* b, const uint8_t* c,
                    uint8_t* out);

/* ---- addition (ABI stays 15): self test of the BlockFetch dedup's compare kernel (k_blockfetch.hip).
 * out[i] = 1 iff arena[a_off[i], + len[i]) and
 * arena[b_off[i], + len[i]) hold the same bytes.  One wave per pair: the bytes up to the first
 * 16-byte boundary of a, then PRAOS_SPAN_EQ_VEC-byte vectors, PRAOS_SPAN_EQ_WAVE bytes per wave
 * step and PRAOS_SPAN_EQ_TILE bytes between two any-difference votes, then the bytes left.  Reads
 * the two spans only.  PRAOS_E_ARG, with nothing launched, for a span outside [0, arena_len). */
#define PRAOS_SPAN_EQ_VEC  16u
#define PRAOS_SPAN_EQ_WAVE 1024u
#define PRAOS_SPAN_EQ_TILE 4096u
int praos_debug_span_equal(praos_ctx* ctx, size_t n, const uint8_t* arena, size_t arena_len, const uint64_t* a_off,
                           const uint64_t* b_off, const uint32_t* len, uint8_t* out);

/* ---- addition (ABI stays 15): self test of the row set of the wire calls (k_wire.hip's k_hdr_*
 * kernels, as praos_validate_candidates*, praos_verify_gen_txs and praos_verify_fetched_blocks run
 * them).  dedup != 0: the items with flag[i] == 0 and tag[i] < 32 in tag_mask are classed by
 * (tag[i], key32[32 i, + 32)); limit is ignored.  dedup == 0: every item with flag[i] == 0 and
 * i < *limit (limit NULL: n) is a class of its own; tag, key32 and tag_mask are not read.  The
 * classes are numbered in order of first appearance: item_row[i] = the row of item i's class
 * (PRAOS_NO_ROW: in no class), *n_rows = the classes.  n < 2^24; n = 0 is PRAOS_OK with
 * *n_rows = 0.  PRAOS_E_STATE on a host-only context. */
int praos_debug_row_set(praos_ctx* ctx, size_t n, const uint8_t* flag, const uint8_t* tag, const uint8_t* key32,
                        uint32_t tag_mask, int dedup, const uint32_t* limit, uint32_t* item_row, uint32_t* n_rows);

#ifdef __cplusplus
}
#endif
#endif
