{-# LANGUAGE DataKinds                #-}
{-# LANGUAGE ForeignFunctionInterface #-}
{-# LANGUAGE NamedFieldPuns           #-}
{-# LANGUAGE ScopedTypeVariables      #-}

-- | Batched Praos header validation on AMD MI355X GPUs (libpraos_hip.so).
--
-- The binding a maintainer adds beside
-- @ouroboros-consensus-protocol/src/ouroboros-consensus-protocol/Ouroboros/Consensus/Protocol/Praos.hs@.
-- It replaces, for the headers of one epoch at a time, the per-header crypto of
-- 'updateChainDepState' (Praos.hs:441-459: validateKESSignature :558-606 and
-- validateVRFSignature :528-556) and, for db-analyser's header revalidation
-- (Cardano/Tools/DBAnalyser/Analysis.hs:479-607, streaming loop :815-847), the whole
-- validateHeader fold (envelope + updateChainDepState) over stored header bytes.
--
-- GHC is not available where this repository is built, so this module is shipped as
-- source.  Its exact foreign-call sequence is exercised from C by
-- integration/c/ffi_harness.c (tests/test_gpu_ffi.py), and the struct layouts below
-- are checked against the C header by tests/test_abi.py (the "-- struct" lines).
--
-- Link: @extra-libraries: praos_hip@ (and @amdhip64@), include-dirs: include/.
module Ouroboros.Consensus.Protocol.Praos.Batch
  ( -- * Context (one GPU, or a group of several)
    PraosBatchCtx
  , withPraosBatchCtx
  , withPraosBatchDevices
  , praosBatchMembers
  , PraosBatchError (..)
  , praosSetPoolKeyStore
    -- * Per epoch
  , PraosParamsC (..)
  , praosSetEpoch
  , praosTickedEpochNonce
    -- * Headers from stored bytes
  , BatchResult (..)
  , praosValidateHeaderBytes
    -- * Headers from stored bytes, Storable vectors (Batch.Validate)
  , SpanResult (..)
  , ArenaPin (..)
  , praosValidateHeaderSpans
  , praosHostRegister
  , praosHostUnregister
  , praosSubmitHeaderBytes
  , praosDrainHeaderBytes
    -- * TPraos (Shelley..Alonzo) headers from stored bytes
  , TPraosBatchResult (..)
  , praosTickedEpochNonceTPraos
  , OverlayC (..)
  , praosSetOverlay
  , praosValidateTPraosHeaderBytes
  , praosValidateTPraosHeaderSpans
    -- * Whole ImmutableDB replay (db-analyser)
  , ReplayStats (..)
  , praosReplayImmutable
  , praosReplayImmutableTPraos
  , LedgerViewC (..)
  , praosReplayImmutableViews
    -- * ImmutableDB chunk validation (verifyBlockIntegrity batched)
  , ChunkValidation (..)
  , verifyChunkIntegrity
  , ChunkOutcome (..)
  , ChunkParse (..)
  , validateChunkBatch
  , praosVerifyBlockIntegrity
    -- * Transaction index of stored blocks (db-analyser's block statistics)
  , BlockTxStats (..)
  , praosIndexBlockTxs
  , praosVerifyTxWitnesses
  , GenTxResults (..)
  , praosVerifyGenTxs
  , FetchedBlockResults (..)
  , praosVerifyFetchedBlocks
  , BlockWitnessStats (..)
    -- * Byron header validation (PBFT)
  , PBftParamsC (..)
  , PBftTipC
  , PBftBatchResult (..)
  , validatePBftHeaderBatch
    -- * Headers as the ChainSync client receives them (node-to-node encoding)
  , WireHeader (..)
  , unwrapWireHeaders
  , CandidateFragment (..)
  , CandidateLimits (..)
  , CandidatesResult (..)
  , validateCandidateFragments
  , TPraosCandidatesResult (..)
  , validateCandidateFragmentsTPraos
  , PBftCandidateFragment (..)
  , PBftCandidatesResult (..)
  , validateCandidateFragmentsPBft
    -- * Error reconstruction (typed constructors: module Batch.Errors)
  , verdictToError
  ) where

import           Control.Exception (Exception, bracket, bracket_, throwIO)
import           Control.Monad (forM_, when)
import qualified Data.ByteString as BS
import qualified Data.ByteString.Unsafe as BSU
import           Data.Maybe (fromMaybe)
import qualified Data.Vector.Storable as VS
import qualified Data.Vector.Storable.Mutable as VSM
import           Data.Ratio (denominator, numerator)
import           Data.Word (Word16, Word32, Word64, Word8)
import           Foreign
import           Foreign.C.String (CString, peekCString, withCString)
import           Foreign.C.Types (CInt (..), CSize (..))

-- ---------------------------------------------------------------- C ABI (include/praos_hip.h)

data PraosCtx
data PraosGroup

-- struct praos_params (40 bytes): slots_per_kes_period@0 max_kes_evo@8 f_is_one@16 vrf_check_output@20 c_raw@24
-- struct praos_pool (76 bytes): hash28@0 vrf_hash32@28 sigma_fp@60
-- struct praos_headers (120 bytes): n@0 slot@8 cold_vk@16 ocert_n@56 body_bytes_len@112
-- struct praos_header_bytes (40 bytes): n@0 bytes@8 bytes_len@16 off@24 len@32
-- struct praos_out (40 bytes): bits@0 pool_idx@8 beta@16 leader@24 nonce@32
-- struct praos_nonce (36 bytes): hash@0 neutral@32
-- struct praos_chain_state (232 bytes): last_slot_origin@0 last_slot@8 counter_hash28@16 counter@24 m@32 cap@40 evolving@48 candidate@84 epoch_nonce@120 lab@156 last_epoch_block@192
-- struct praos_epoch_info (32 bytes): epoch_base_slot@0 epoch_base_no@8 epoch_length@16 stability_window@24
-- struct praos_envelope (120 bytes): block_no@0 header_hash@8 header_size@16 body_size@24 tip_is_origin@32 tip_slot@40 tip_block_no@48 tip_hash@56 max_major_pv@88 lv_prot_major@96 max_header_size@104 max_body_size@112
-- struct praos_replay_stats (80 bytes): skipped@0 headers@8 validated@16 stop_index@24 stop_verdict@32 epochs@36 batches@40 chunks@44 ms_io@48 ms_device@56 ms_fold@64 ms_nonce@72
-- struct praos_decoded (168 bytes): status@0 block_no@8 slot@16 prev_hash@24 prev_is_genesis@32 cold_vk@40 body_size@72 ocert_n@96 header_hash@160
-- struct praos_tpraos_headers (136 bytes): h@0 leader_out@120 leader_proof@128
-- struct praos_tpraos_out (40 bytes): bits@0 pool_idx@8 beta_eta@16 beta_leader@24 nonce@32
-- struct praos_ledger_view (48 bytes): first_epoch@0 pools@8 npools@16 reserved@20 lv_prot_major@24 max_header_size@32 max_body_size@40

foreign import ccall safe "praos_open"        c_open        :: CInt -> IO (Ptr PraosCtx)
foreign import ccall safe "praos_close"       c_close       :: Ptr PraosCtx -> IO ()
foreign import ccall safe "praos_last_error"  c_last_error  :: Ptr PraosCtx -> IO CString
foreign import ccall safe "praos_abi_version" c_abi_version :: IO CInt
foreign import ccall safe "praos_set_option"  c_set_option  :: Ptr PraosCtx -> CInt -> CInt -> IO CInt
foreign import ccall safe "praos_set_epoch"   c_set_epoch
  :: Ptr PraosCtx -> Ptr Word8 -> Ptr () -> Word32 -> Ptr () -> IO CInt
foreign import ccall safe "praos_ticked_epoch_nonce" c_ticked_epoch_nonce
  :: Ptr () -> Ptr () -> Word64 -> Ptr () -> IO CInt
foreign import ccall safe "praos_verify_header_bytes" c_verify_header_bytes
  :: Ptr PraosCtx -> Ptr () -> Ptr () -> Ptr () -> IO CInt
foreign import ccall safe "praos_validate_headers" c_validate_headers
  :: Ptr PraosCtx -> Ptr () -> Ptr Word8 -> Ptr Word8 -> Ptr () -> Ptr () -> Ptr () -> Ptr ()
  -> Ptr Word8 -> Ptr CSize -> Ptr CSize -> IO CInt
foreign import ccall safe "praos_host_register" c_host_register
  :: Ptr PraosCtx -> Ptr Word8 -> CSize -> IO CInt
foreign import ccall safe "praos_host_unregister" c_host_unregister
  :: Ptr PraosCtx -> Ptr Word8 -> IO CInt
foreign import ccall safe "praos_state_encode" c_state_encode
  :: Ptr () -> Ptr Word8 -> CSize -> Ptr CSize -> IO CInt
foreign import ccall safe "praos_state_decode" c_state_decode
  :: Ptr Word8 -> CSize -> Ptr () -> IO CInt
foreign import ccall safe "praos_replay_immutable" c_replay_immutable
  :: Ptr PraosCtx -> CString -> Ptr () -> Word32 -> Ptr () -> Ptr () -> Ptr () -> Ptr ()
  -> CSize -> Ptr Word8 -> CSize -> Ptr () -> IO CInt
-- TPraos (include/praos_hip.h: praos_tpraos_*)
foreign import ccall safe "praos_tpraos_ticked_epoch_nonce" c_tpraos_ticked_epoch_nonce
  :: Ptr () -> Ptr () -> Word64 -> Ptr () -> Ptr () -> IO CInt
foreign import ccall safe "praos_verify_tpraos_header_bytes" c_verify_tpraos_header_bytes
  :: Ptr PraosCtx -> Ptr () -> Ptr () -> Ptr () -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe "praos_tpraos_update_chain_dep_state" c_tpraos_update_chain_dep_state
  :: Ptr PraosCtx -> Ptr () -> Ptr Word8 -> Ptr Word8 -> Ptr () -> Ptr () -> Ptr () -> Ptr () -> Ptr ()
  -> Ptr Word8 -> Ptr Word16 -> Ptr CSize -> Ptr CSize -> IO CInt
foreign import ccall safe "praos_set_overlay" c_set_overlay :: Ptr PraosCtx -> Ptr () -> IO CInt
foreign import ccall safe "praos_group_set_overlay" c_group_set_overlay :: Ptr PraosGroup -> Ptr () -> IO CInt
foreign import ccall safe "praos_replay_immutable_tpraos" c_replay_immutable_tpraos
  :: Ptr PraosCtx -> CString -> Ptr () -> Word32 -> Ptr () -> Ptr () -> Ptr () -> Ptr () -> Ptr ()
  -> CSize -> Ptr Word8 -> Ptr Word16 -> CSize -> Ptr () -> IO CInt
-- several GPUs (include/praos_hip.h: praos_group_*): shards of one batch, or consecutive
-- replay batches, on the members; outputs in place; the fold on member 0
foreign import ccall safe "praos_group_open"  c_group_open  :: Ptr CInt -> CInt -> IO (Ptr PraosGroup)
foreign import ccall safe "praos_group_close" c_group_close :: Ptr PraosGroup -> IO ()
foreign import ccall safe "praos_group_size"  c_group_size  :: Ptr PraosGroup -> IO CInt
foreign import ccall safe "praos_group_ctx"   c_group_ctx   :: Ptr PraosGroup -> CInt -> IO (Ptr PraosCtx)
foreign import ccall safe "praos_group_last_error" c_group_last_error :: Ptr PraosGroup -> IO CString
foreign import ccall safe "praos_group_set_option" c_group_set_option :: Ptr PraosGroup -> CInt -> CInt -> IO CInt
foreign import ccall safe "praos_group_set_epoch" c_group_set_epoch
  :: Ptr PraosGroup -> Ptr Word8 -> Ptr () -> Word32 -> Ptr () -> IO CInt
foreign import ccall safe "praos_group_verify_header_bytes" c_group_verify_header_bytes
  :: Ptr PraosGroup -> Ptr () -> Ptr () -> Ptr () -> IO CInt
foreign import ccall safe "praos_group_verify_tpraos_header_bytes" c_group_verify_tpraos_header_bytes
  :: Ptr PraosGroup -> Ptr () -> Ptr () -> Ptr () -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe "praos_group_host_register" c_group_host_register
  :: Ptr PraosGroup -> Ptr Word8 -> CSize -> IO CInt
foreign import ccall safe "praos_group_host_unregister" c_group_host_unregister
  :: Ptr PraosGroup -> Ptr Word8 -> IO CInt
foreign import ccall safe "praos_group_replay_immutable" c_group_replay_immutable
  :: Ptr PraosGroup -> CString -> Ptr () -> Word32 -> Ptr () -> Ptr () -> Ptr () -> Ptr ()
  -> CSize -> Ptr Word8 -> CSize -> Ptr () -> IO CInt
foreign import ccall safe "praos_group_replay_immutable_tpraos" c_group_replay_immutable_tpraos
  :: Ptr PraosGroup -> CString -> Ptr () -> Word32 -> Ptr () -> Ptr () -> Ptr () -> Ptr () -> Ptr ()
  -> CSize -> Ptr Word8 -> Ptr Word16 -> CSize -> Ptr () -> IO CInt
-- ABI 14: a ledger view per epoch in the replay; block integrity (ImmutableDB chunk validation)
foreign import ccall safe "praos_replay_immutable_views" c_replay_immutable_views
  :: Ptr PraosCtx -> CString -> Ptr () -> Word32 -> Ptr () -> Ptr () -> Ptr () -> Ptr ()
  -> CSize -> Ptr Word8 -> CSize -> Ptr () -> IO CInt
foreign import ccall safe "praos_group_replay_immutable_views" c_group_replay_immutable_views
  :: Ptr PraosGroup -> CString -> Ptr () -> Word32 -> Ptr () -> Ptr () -> Ptr () -> Ptr ()
  -> CSize -> Ptr Word8 -> CSize -> Ptr () -> IO CInt
foreign import ccall safe "praos_verify_block_integrity" c_verify_block_integrity
  :: Ptr PraosCtx -> Ptr () -> Word64 -> Ptr Word8 -> Ptr Word8 -> IO CInt
foreign import ccall safe "praos_group_verify_block_integrity" c_group_verify_block_integrity
  :: Ptr PraosGroup -> Ptr () -> Word64 -> Ptr Word8 -> Ptr Word8 -> IO CInt

-- ABI 15: the streaming form of praos_verify_header_bytes (three calls in flight per context)
foreign import ccall safe "praos_verify_header_bytes_submit" c_verify_header_bytes_submit
  :: Ptr PraosCtx -> Ptr () -> Ptr () -> Ptr () -> IO CInt
foreign import ccall safe "praos_verify_drain" c_verify_drain :: Ptr PraosCtx -> IO CInt

-- added without a version bump (purely additive): parseChunkFile as one call.  The structs it
-- pokes and peeks (checked against the C compiler by tests/test_chunk_abi.py; "layout", not
-- "struct": the lines above are the ones tests/test_abi.py owns):
-- layout praos_chunk (40 bytes): bytes@0 bytes_len@8 expected_crc@16 n_expected@24 block_off@32
-- layout praos_chunk_result (152 bytes): outcome@0 integrity_bits@4 blocks@8 checked@16 truncate_at@24 rescanned_from@32 err_slot@40 err_hash@48 expected_prev@80 actual_prev@112 actual_prev_is_genesis@144
-- layout praos_chunk_out (48 bytes): cap@0 entries@8 block_no@16 prev_hash@24 prev_is_genesis@32 integrity@40
foreign import ccall safe "praos_validate_chunk" c_validate_chunk
  :: Ptr PraosCtx -> Ptr () -> Word64 -> Ptr () -> Ptr () -> IO CInt
-- added without a version bump (purely additive): the same call with the Byron era switched on.
-- Its configuration struct (checked against the C compiler by tests/test_byron_abi.py;
-- "layout-byron": tests/test_chunk_abi.py owns the "layout" lines above and knows only its own structs):
-- layout-byron praos_chunk_cfg (24 bytes): slots_per_kes_period@0 byron_epoch_slots@8 byron_protocol_magic@16 pad_@20
foreign import ccall safe "praos_validate_chunk_cfg" c_validate_chunk_cfg
  :: Ptr PraosCtx -> Ptr () -> Ptr () -> Ptr () -> Ptr () -> Ptr Word8 -> IO CInt
-- additive as well (ABI version unchanged): the transaction index of stored blocks.  Its structs
-- (checked against the C compiler by tests/test_txindex_abi.py, which owns the "layout-txi" lines):
-- layout-txi praos_txi_cfg (8 bytes): byron@0 pad_@4
-- layout-txi praos_txi_stats (48 bytes): status@0 n_tx@8 txs_size@16 n_out@24 ex_steps@32 tx_first@40
-- layout-txi praos_txi_rows (112 bytes): cap@0 n_rows@8 block@16 body_off@24 body_len@32 wit_off@40 wit_len@48 aux_off@56 aux_len@64 size@72 n_out@80 ex_steps@88 is_valid@96 tx_id@104
foreign import ccall safe "praos_index_block_txs" c_index_block_txs
  :: Ptr PraosCtx -> Ptr () -> Ptr () -> Ptr () -> Ptr () -> IO CInt
-- additive as well (ABI version unchanged): the key witnesses of stored blocks' transactions.  Its
-- structs (checked against the C compiler by tests/test_txwit_abi.py, which owns the "layout-txw" lines):
-- layout-txw praos_txw_cfg (8 bytes): byron@0 max_lanes@4
-- layout-txw praos_txw_blocks (48 bytes): status@0 n_tx@8 n_wit@16 n_bad@24 n_shape@32 tx_first@40
-- layout-txw praos_txw_txs (72 bytes): cap@0 n_rows@8 block@16 status@24 n_vkey@32 n_boot@40 n_bad@48 tx_id@56 wit_first@64
-- layout-txw praos_txw_wits (64 bytes): cap@0 n_wits@8 tx@16 kind@24 key_off@32 sig_off@40 ok@48 key_hash@56
foreign import ccall safe "praos_verify_tx_witnesses" c_verify_tx_witnesses
  :: Ptr PraosCtx -> Ptr () -> Ptr () -> Ptr () -> Ptr () -> Ptr () -> IO CInt
-- additive as well (ABI version unchanged): wire transactions of the TxSubmission inbound side.
-- Its structs (checked against the C compiler by tests/test_gentx_abi.py, which owns the
-- "layout-gtx" lines; praos_txw_wits is the struct above):
-- layout-gtx praos_gtx_cfg (16 bytes): n_eras@0 dedup@4 max_lanes@8 pad_@12
-- layout-gtx praos_gtx_items (48 bytes): status@0 era@8 row@16 byron_kind@24 payload_off@32 payload_len@40
-- layout-gtx praos_gtx_txs (168 bytes): cap@0 n_rows@8 item@16 era@24 body_off@32 body_len@40 wit_off@48 wit_len@56 aux_off@64 aux_len@72 size@80 in_block_size@88 ex_mem@96 ex_steps@104 is_valid@112 tx_id@120 wstatus@128 n_vkey@136 n_boot@144 n_bad@152 wit_first@160
foreign import ccall safe "praos_verify_gen_txs" c_verify_gen_txs
  :: Ptr PraosCtx -> Ptr () -> Ptr () -> Ptr () -> Ptr () -> Ptr () -> IO CInt
-- additive as well (ABI version unchanged): wire blocks of the BlockFetch client.  Its structs
-- (checked against the C compiler by tests/test_blockfetch_abi.py, which owns the "layout-bf"
-- lines; the praos_txw_* structs are those above):
-- layout-bf praos_bf_ranges (40 bytes): k@0 item_first@8 exp_first@16 exp_slot@24 exp_hash@32
-- layout-bf praos_bf_cfg (24 bytes): n_eras@0 dedup@4 witnesses@8 max_lanes@12 byron_epoch_slots@16
-- layout-bf praos_bf_items (32 bytes): status@0 tag@8 verdict@16 row@24
-- layout-bf praos_bf_range_out (24 bytes): stop@0 accepted@8 status@16
-- layout-bf praos_bf_rows (128 bytes): cap@0 n_rows@8 item@16 tag@24 is_ebb@32 slot@40 block_no@48 header_hash@56 prev_hash@64 hdr_off@72 hdr_len@80 blk_off@88 blk_len@96 body_hash@104 bits@112 which@120
foreign import ccall safe "praos_verify_fetched_blocks" c_verify_fetched_blocks
  :: Ptr PraosCtx -> Ptr () -> Ptr () -> Ptr () -> Ptr () -> Ptr () -> Ptr () -> Ptr () -> Ptr () -> Ptr () -> IO CInt
-- additive as well (ABI version unchanged): Byron header validation.  The structs
-- validatePBftHeaderBatch pokes and peeks (checked against the C compiler by tests/test_pbft_abi.py;
-- "layout-pbft": the other layout lines belong to the tests named above):
-- layout-pbft praos_pbft_params (32 bytes): window_size@0 threshold@8 epoch_slots@16 protocol_magic@24 pad_@28
-- layout-pbft praos_pbft_out (64 bytes): bits@0 gk_idx@8 slot@16 block_no@24 prev_hash@32 prev_is_genesis@40 header_hash@48 delegate_hash@56
-- layout-pbft praos_pbft_tip (56 bytes): origin@0 is_ebb@1 pad_@2 slot@8 block_no@16 hash@24
-- layout-pbft praos_pbft_state (32 bytes): cap@0 n@8 slot@16 genesis_hash@24
foreign import ccall safe "praos_verify_pbft_headers" c_verify_pbft_headers
  :: Ptr PraosCtx -> Ptr () -> Ptr Word8 -> Ptr () -> Ptr Word8 -> Word32 -> Ptr () -> IO CInt
foreign import ccall safe "praos_pbft_update_chain_dep_state" c_pbft_update_chain_dep_state
  :: Ptr PraosCtx -> CSize -> Ptr () -> Ptr Word8 -> Ptr () -> Ptr Word8 -> Word32 -> Ptr () -> Ptr ()
  -> Ptr Word8 -> Ptr Word64 -> Ptr CSize -> IO CInt
foreign import ccall safe "praos_pbft_state_encode" c_pbft_state_encode
  :: Ptr () -> Ptr Word8 -> CSize -> Ptr CSize -> IO CInt
foreign import ccall safe "praos_pbft_state_decode" c_pbft_state_decode
  :: Ptr Word8 -> CSize -> Ptr () -> IO CInt
-- additive as well (ABI version unchanged): wire headers and the ChainSync candidates call.  The
-- structs unwrapWireHeaders and validateCandidateFragments poke and peek (checked against the C
-- compiler by tests/test_candidates_abi.py; "layout-wire"):
-- layout-wire praos_wire_out (56 bytes): status@0 era@8 byron_kind@16 size_hint@24 off@32 len@40 header_hash@48
-- layout-wire praos_candidates_in (120 bytes): items@0 n_eras@40 praos_eras@44 view_end_slot@48 ei@56 max_major_pv@88 lv_prot_major@96 max_header_size@104 max_body_size@112
-- layout-wire praos_fragment (304 bytes): tip_is_origin@0 tip_slot@8 tip_block_no@16 tip_hash@24 state@56 chain_stop@288 processed@296
-- layout-wire praos_fragments (24 bytes): k@0 frag_first@8 frag@16
-- layout-wire praos_candidates_out (312 bytes): wire_status@0 row@8 verdict@16 rows_cap@24 n_rows@32 rows@40 dec@80 eta_idx@248 etas@256 n_etas@264 stats@272
foreign import ccall safe "praos_unwrap_wire_headers" c_unwrap_wire_headers
  :: Ptr PraosCtx -> Ptr () -> Word32 -> Ptr () -> IO CInt
foreign import ccall safe "praos_validate_candidates" c_validate_candidates
  :: Ptr PraosCtx -> Ptr () -> Ptr () -> Ptr () -> IO CInt
-- additive again: the candidates calls for fragments of TPraos and of Byron headers.  The structs
-- validateCandidateFragmentsTPraos and validateCandidateFragmentsPBft poke and peek (checked
-- against the C compiler by tests/test_candidates_eras_abi.py; "layout-eras": the other layout
-- lines belong to the tests named above):
-- layout-eras praos_tpraos_candidates_in (128 bytes): items@0 n_eras@40 tpraos_eras@44 view_end_slot@48 ei@56 max_major_pv@88 lv_prot_major@96 max_header_size@104 max_body_size@112 extra_entropy@120
-- layout-eras praos_tpraos_candidates_out (336 bytes): wire_status@0 row@8 verdict@16 failures@24 rows_cap@32 n_rows@40 rows@48 dec@88 leader_out@256 leader_proof@264 eta_idx@272 etas@280 n_etas@288 stats@296
-- layout-eras praos_pbft_candidates_in (96 bytes): items@0 n_eras@40 n_delegs@44 view_end_slot@48 params@56 delegs@88
-- layout-eras praos_pbft_fragment (104 bytes): tip@0 state@56 chain_stop@88 processed@96
-- layout-eras praos_pbft_fragments (24 bytes): k@0 frag_first@8 frag@16
-- layout-eras praos_pbft_candidates_out (152 bytes): wire_status@0 row@8 verdict@16 aux@24 rows_cap@32 n_rows@40 rows@48 row_is_ebb@112 stats@120
foreign import ccall safe "praos_validate_candidates_tpraos" c_validate_candidates_tpraos
  :: Ptr PraosCtx -> Ptr () -> Ptr () -> Ptr () -> IO CInt
foreign import ccall safe "praos_validate_candidates_pbft" c_validate_candidates_pbft
  :: Ptr PraosCtx -> Ptr () -> Ptr () -> Ptr () -> IO CInt

abiVersion :: CInt
abiVersion = 15

-- ---------------------------------------------------------------- context

-- | One GPU (a praos_ctx), or a group of several (a praos_group: one context per device,
-- batches split into contiguous shards, replay batches dealt to the members in turn) together
-- with its member 0, on which the sequential fold runs.  Every entry point below takes either.
data PraosBatchCtx
  = PraosBatchCtx !(Ptr PraosCtx)
  | PraosBatchGroup !(Ptr PraosGroup) !(Ptr PraosCtx) !Int

data PraosBatchError = PraosBatchError !Int !String
  deriving Show
instance Exception PraosBatchError

-- | One context per GPU (device ordinal) and per Haskell thread that uses it; calls block
-- (the foreign imports are @safe@, so other Haskell threads keep running).
withPraosBatchCtx :: Int -> (PraosBatchCtx -> IO a) -> IO a
withPraosBatchCtx dev k = do
  v <- c_abi_version
  when (v /= abiVersion) $ throwIO (PraosBatchError (-2) ("libpraos_hip ABI " ++ show v))
  bracket (c_open (fromIntegral dev)) c_close $ \p -> do
    when (p == nullPtr) $ throwIO (PraosBatchError (-1) ("praos_open " ++ show dev))
    k (PraosBatchCtx p)

-- | The GPUs of one node as one batch context (SURVEY sec. 8e: an epoch's headers shard by
-- contiguous slot range, no exchange between devices).  One device is 'withPraosBatchCtx';
-- several are a praos_group (a device may repeat: several contexts on one GPU).
withPraosBatchDevices :: [Int] -> (PraosBatchCtx -> IO a) -> IO a
withPraosBatchDevices [] _ = throwIO (PraosBatchError (-1) "withPraosBatchDevices: no device")
withPraosBatchDevices [dev] k = withPraosBatchCtx dev k
withPraosBatchDevices devs k = do
  v <- c_abi_version
  when (v /= abiVersion) $ throwIO (PraosBatchError (-2) ("libpraos_hip ABI " ++ show v))
  let m = length devs
  bracket (withArray (map fromIntegral devs) $ \dp -> c_group_open dp (fromIntegral m)) c_group_close $ \g -> do
    when (g == nullPtr) $ throwIO (PraosBatchError (-1) ("praos_group_open " ++ show devs))
    c0 <- c_group_ctx g 0
    k (PraosBatchGroup g c0 m)

-- | Devices (contexts) a batch context spreads over.
praosBatchMembers :: PraosBatchCtx -> Int
praosBatchMembers (PraosBatchCtx _) = 1
praosBatchMembers (PraosBatchGroup _ _ m) = m

-- | The context the fold and the codecs run on (member 0 of a group).
ctxPtr :: PraosBatchCtx -> Ptr PraosCtx
ctxPtr (PraosBatchCtx p) = p
ctxPtr (PraosBatchGroup _ p _) = p

-- | PRAOS_OPT_POOL_KEYS (7): keep the cold-key and VRF-key cache entries across calls on
-- this context (a node validating batch after batch of one epoch sees the same pool keys);
-- verdicts are identical either way.  On by default inside the replay entry points.
praosSetPoolKeyStore :: PraosBatchCtx -> Bool -> IO ()
praosSetPoolKeyStore ctx on = check ctx $ case ctx of
  PraosBatchCtx p -> c_set_option p 7 (if on then 1 else 0)
  PraosBatchGroup g _ _ -> c_group_set_option g 7 (if on then 1 else 0)

-- | A batch call's return code: the group's error text for group calls, the context's otherwise.
check :: PraosBatchCtx -> IO CInt -> IO ()
check ctx act = do
  rc <- act
  when (rc /= 0) $ do
    msg <- case ctx of
      PraosBatchCtx p -> c_last_error p >>= peekCString
      PraosBatchGroup g _ _ -> c_group_last_error g >>= peekCString
    throwIO (PraosBatchError (fromIntegral rc) msg)

-- | A call on one context (the fold on member 0 of a group).
checkCtx :: Ptr PraosCtx -> IO CInt -> IO ()
checkCtx p = check (PraosBatchCtx p)

-- | praos_verify_header_bytes, or its group form (shards on the members, outputs in place).
verifyHeaderBytes :: PraosBatchCtx -> Ptr () -> Ptr () -> Ptr () -> IO ()
verifyHeaderBytes ctx hb out dec = check ctx $ case ctx of
  PraosBatchCtx p -> c_verify_header_bytes p hb out dec
  PraosBatchGroup g _ _ -> c_group_verify_header_bytes g hb out dec

-- | The streaming form of 'verifyHeaderBytes' (praos_verify_header_bytes_submit): the call is
-- queued and returns; its outputs are written by the third submit after it (a context keeps
-- three calls in flight, the next ones' uploads and stage V under this one's key chains) or by
-- 'praosDrainHeaderBytes'.  The header-bytes struct, the arena and the output arrays must stay
-- alive and unchanged until then.  A group runs the blocking call.
praosSubmitHeaderBytes :: PraosBatchCtx -> Ptr () -> Ptr () -> Ptr () -> IO ()
praosSubmitHeaderBytes ctx hb out dec = check ctx $ case ctx of
  PraosBatchCtx p -> c_verify_header_bytes_submit p hb out dec
  PraosBatchGroup g _ _ -> c_group_verify_header_bytes g hb out dec

-- | Every submitted call's outputs written (praos_verify_drain).
praosDrainHeaderBytes :: PraosBatchCtx -> IO ()
praosDrainHeaderBytes ctx = case ctx of
  PraosBatchCtx p -> check ctx (c_verify_drain p)
  PraosBatchGroup {} -> pure ()

verifyTPraosHeaderBytes :: PraosBatchCtx -> Ptr () -> Ptr () -> Ptr () -> IO ()
verifyTPraosHeaderBytes ctx hb out dec = check ctx $ case ctx of
  PraosBatchCtx p -> c_verify_tpraos_header_bytes p hb out dec nullPtr nullPtr
  PraosBatchGroup g _ _ -> c_group_verify_tpraos_header_bytes g hb out dec nullPtr nullPtr

-- | Who page-locks a batch's arena: 'PinForCall' -- the call registers it for its own
-- duration when it is 64 MiB or more -- or 'PinnedByCaller': the caller registered it once
-- ('praosHostRegister', e.g. an arena reused epoch after epoch and re-registered only when it
-- grows), so the call's time holds no pinning.
data ArenaPin = PinForCall | PinnedByCaller
  deriving (Eq, Show)

-- | praos_host_register (every member of a group): uploads from inside the range go by direct
-- DMA.  Pair with 'praosHostUnregister' before the buffer is freed or moved.
praosHostRegister :: PraosBatchCtx -> Ptr Word8 -> Int -> IO ()
praosHostRegister ctx ap alen = check ctx $ case ctx of
  PraosBatchCtx p -> c_host_register p ap (fromIntegral alen)
  PraosBatchGroup g _ _ -> c_group_host_register g ap (fromIntegral alen)

praosHostUnregister :: PraosBatchCtx -> Ptr Word8 -> IO ()
praosHostUnregister ctx ap = check ctx $ case ctx of
  PraosBatchCtx p -> c_host_unregister p ap
  PraosBatchGroup g _ _ -> c_group_host_unregister g ap

-- | The arena page-locked for the duration of the action when it is 64 MiB or more
-- (praos_host_register: the upload goes by direct DMA, no staging copy; a group pins it
-- once for every member) and the caller has not pinned it.  The unregister runs whatever the
-- action throws (a failing batch call), so a GHC-owned buffer is never freed while still
-- page-locked.
withRegisteredArena :: PraosBatchCtx -> ArenaPin -> Ptr Word8 -> Int -> IO a -> IO a
withRegisteredArena ctx pin ap alen act
  | pin == PinnedByCaller || alen < 64 * 1024 * 1024 = act
  | otherwise = bracket_ (praosHostRegister ctx ap alen) (praosHostUnregister ctx ap) act

-- ---------------------------------------------------------------- marshalling helpers

-- | Little-endian bytes of a non-negative Integer (Fixed E34 raw values, int128 two's
-- complement for activeSlotLog).
pokeLE :: Ptr Word8 -> Int -> Integer -> IO ()
pokeLE p n x = forM_ [0 .. n - 1] $ \i ->
  pokeByteOff p i (fromIntegral ((x `mod` 2 ^ (128 :: Int)) `shiftR` (8 * i)) :: Word8)

pokeBS :: Ptr a -> Int -> BS.ByteString -> IO ()
pokeBS p off bs = BSU.unsafeUseAsCStringLen bs $ \(src, n) -> copyBytes (p `plusPtr` off) (castPtr src) n

-- | PraosParams as the ABI wants them (praos_params): slotsPerKESPeriod, maxKESEvo,
-- f == 1, activeSlotLog f (unActiveSlotLog, Fixed E34 raw, <= 0), and whether
-- 'VRF.verifyCertified' compares the certified output with the proof's hash.
--
-- ppVrfCheckOutput: cardano-crypto-class >= 2.1 (the CHaP index-state this snapshot
-- pins, cabal.project:15-20) defines @verifyCertified ctx vk a c = verifyVRF ctx vk a
-- (certifiedProof c) == Just (certifiedOutput c)@ -- True, the default a caller should pass.
-- Older cardano-crypto-class releases (1.x: @verifyVRF ... (output, proof) -> Bool@ whose
-- PraosVRF instance ignored the output) correspond to False.  Either way the batch reports
-- both facts: PRAOS_BIT_VRF_PROOF (proof) and PRAOS_BIT_VRF_OUTPUT (output mismatch, set
-- only when checked).
data PraosParamsC = PraosParamsC
  { ppSlotsPerKESPeriod :: !Word64
  , ppMaxKESEvo         :: !Word64
  , ppFIsOne            :: !Bool
  , ppActiveSlotLogRaw  :: !Integer
  , ppVrfCheckOutput    :: !Bool
  }

withParams :: PraosParamsC -> (Ptr () -> IO a) -> IO a
withParams pp k = allocaBytes 40 $ \p -> do
  fillBytes p 0 40
  pokeByteOff p 0 (ppSlotsPerKESPeriod pp)
  pokeByteOff p 8 (ppMaxKESEvo pp)
  pokeByteOff p 16 (if ppFIsOne pp then 1 else 0 :: Word32)
  pokeByteOff p 20 (if ppVrfCheckOutput pp then 1 else 0 :: Word32)
  pokeLE (p `plusPtr` 24) 16 (ppActiveSlotLogRaw pp)
  k (castPtr p)

-- | PoolDistr entries: (KeyHash 'StakePool bytes, VRF key hash bytes, sigma as
-- Fixed E34 raw = floor (sigma * 10^34), i.e. fromRational individualPoolStake).
withPools :: [(BS.ByteString, BS.ByteString, Integer)] -> (Ptr () -> Word32 -> IO a) -> IO a
withPools pools k = allocaBytes (76 * max 1 (length pools)) $ \p -> do
  forM_ (zip [0 ..] pools) $ \(i, (hk, vrf, sigma)) -> do
    let q = p `plusPtr` (76 * i)
    pokeBS q 0 hk
    pokeBS q 28 vrf
    pokeLE (q `plusPtr` 60) 16 sigma
  k (castPtr p) (fromIntegral (length pools))

-- | A nonce: Nothing = NeutralNonce.
pokeNonce :: Ptr a -> Int -> Maybe BS.ByteString -> IO ()
pokeNonce p off mn = case mn of
  Nothing -> fillBytes (p `plusPtr` off) 0 32 >> pokeByteOff p (off + 32) (1 :: Word32)
  Just h  -> pokeBS p off h >> pokeByteOff p (off + 32) (0 :: Word32)

peekNonce :: Ptr a -> Int -> IO (Maybe BS.ByteString)
peekNonce p off = do
  neutral :: Word32 <- peekByteOff p (off + 32)
  if neutral /= 0 then pure Nothing else Just <$> BS.packCStringLen (castPtr (p `plusPtr` off), 32)

-- ---------------------------------------------------------------- per epoch

-- | praos_set_epoch: the epoch nonce (tickChainDepState's, see 'praosTickedEpochNonce'),
-- the PoolDistr of the ledger view and the protocol parameters.
praosSetEpoch :: PraosBatchCtx -> Maybe BS.ByteString -> [(BS.ByteString, BS.ByteString, Integer)]
              -> PraosParamsC -> IO ()
praosSetEpoch ctx eta0 pools pp =
  withPools pools $ \pp' np -> withParams pp $ \par ->
    case eta0 of
      Nothing -> set nullPtr pp' np par
      Just e  -> BSU.unsafeUseAsCString e $ \ep -> set (castPtr ep) pp' np par
  where
    set ep pp' np par = check ctx $ case ctx of
      PraosBatchCtx p -> c_set_epoch p ep pp' np par
      PraosBatchGroup g _ _ -> c_group_set_epoch g ep pp' np par

-- | The serialised PraosState (Praos.hs:274-310) the fold reads and writes; the ABI
-- takes the same CBOR through praos_state_encode / praos_state_decode, so the Haskell
-- side keeps its own PraosState and converts at batch boundaries.
withChainState :: BS.ByteString -> Int -> (Ptr () -> IO a) -> IO a
withChainState cbor cap k =
  allocaBytes 232 $ \st -> allocaBytes (28 * cap) $ \hk -> allocaBytes (8 * cap) $ \ctr -> do
    fillBytes st 0 232
    pokeByteOff st 16 hk
    pokeByteOff st 24 ctr
    pokeByteOff st 40 (fromIntegral cap :: CSize)
    BSU.unsafeUseAsCStringLen cbor $ \(src, n) -> do
      rc <- c_state_decode (castPtr src) (fromIntegral n) (castPtr st)
      when (rc /= 0) $ throwIO (PraosBatchError (fromIntegral rc) "praos_state_decode")
    k (castPtr st)

encodeChainState :: Ptr () -> IO BS.ByteString
encodeChainState st = alloca $ \lenp -> do
  _ <- c_state_encode st nullPtr 0 lenp
  n <- peek lenp
  allocaBytes (fromIntegral n) $ \buf -> do
    rc <- c_state_encode st buf n lenp
    when (rc /= 0) $ throwIO (PraosBatchError (fromIntegral rc) "praos_state_encode")
    BS.packCStringLen (castPtr buf, fromIntegral n)

withEpochInfo :: (Word64, Word64, Word64, Word64) -> (Ptr () -> IO a) -> IO a
withEpochInfo (baseSlot, baseNo, len, window) k = allocaBytes 32 $ \p -> do
  pokeByteOff p 0 baseSlot >> pokeByteOff p 8 baseNo >> pokeByteOff p 16 len >> pokeByteOff p 24 window
  k (castPtr p)

-- | tickChainDepState's epoch nonce at a slot (praos_ticked_epoch_nonce).
praosTickedEpochNonce :: BS.ByteString -> (Word64, Word64, Word64, Word64) -> Word64 -> IO (Maybe BS.ByteString)
praosTickedEpochNonce stateCbor ei slot =
  withChainState stateCbor (1 + 65536) $ \st -> withEpochInfo ei $ \eip -> allocaBytes 36 $ \out -> do
    rc <- c_ticked_epoch_nonce st eip slot (castPtr out)
    when (rc /= 0) $ throwIO (PraosBatchError (fromIntegral rc) "praos_ticked_epoch_nonce")
    peekNonce out 0

-- ---------------------------------------------------------------- headers from stored bytes

-- | One epoch's stored headers validated (validateHeader over the batch): per-header
-- verdicts (PRAOS_V_*), check bits, the chain stop and the state / tip after it.
data BatchResult = BatchResult
  { brVerdicts  :: ![Word8]
  , brBits      :: ![Word16]
  , brChainStop :: !Int
  , brState     :: !BS.ByteString          -- PraosState CBOR after the last valid header
  , brTip       :: !(Maybe (Word64, Word64, BS.ByteString))
  }

-- | Envelope limits of the ledger view: (praosMaxMajorPV, pvMajor lvProtocolVersion,
-- lvMaxHeaderSize, lvMaxBodySize).
type EnvLimits = (Word64, Word64, Word64, Word64)

-- | praos_verify_header_bytes (decode + all crypto on the GPU) then praos_validate_headers
-- (envelope, updateChainDepState) for the stored headers of one epoch, in chain order.
-- The epoch must have been installed with 'praosSetEpoch'.
praosValidateHeaderBytes :: PraosBatchCtx -> (Word64, Word64, Word64, Word64) -> EnvLimits
                         -> Maybe (Word64, Word64, BS.ByteString) -> BS.ByteString -> [BS.ByteString]
                         -> IO BatchResult
praosValidateHeaderBytes ctx ei (maxPV, pvMajor, maxHS, maxBS) tip stateCbor hdrs = do
  let n = length hdrs
      arena = BS.concat hdrs
      lens = map BS.length hdrs
      offs = take n (scanl (+) 0 lens)
  BSU.unsafeUseAsCString arena $ \ap ->
    withArray (map fromIntegral offs :: [Word64]) $ \offp ->
    withArray (map fromIntegral lens :: [Word32]) $ \lenp ->
    allocaBytes 40 $ \hb ->
    allocaArray n $ \(bits :: Ptr Word16) -> allocaArray n $ \(pidx :: Ptr Int32) ->
    allocaBytes (32 * n) $ \nonce ->
    allocaArray n $ \(slot :: Ptr Word64) -> allocaArray n $ \(bno :: Ptr Word64) ->
    allocaArray n $ \(ocn :: Ptr Word64) -> allocaArray n $ \(bsz :: Ptr Word32) ->
    allocaBytes (32 * n) $ \prev -> allocaBytes n $ \gen -> allocaBytes (32 * n) $ \cold ->
    allocaBytes (32 * n) $ \hh -> allocaBytes 168 $ \dec -> allocaBytes 40 $ \out ->
    allocaBytes 120 $ \hv -> allocaBytes 120 $ \env -> allocaArray n $ \(verdict :: Ptr Word8) ->
    alloca $ \stopp -> alloca $ \donep ->
    withChainState stateCbor (n + 65536) $ \st -> withEpochInfo ei $ \eip -> do
      pokeByteOff hb 0 (fromIntegral n :: CSize) >> pokeByteOff hb 8 ap
      pokeByteOff hb 16 (fromIntegral (BS.length arena) :: CSize)
      pokeByteOff hb 24 offp >> pokeByteOff hb 32 lenp
      fillBytes out 0 40 >> pokeByteOff out 0 bits >> pokeByteOff out 8 pidx >> pokeByteOff out 32 nonce
      fillBytes dec 0 168
      pokeByteOff dec 8 bno >> pokeByteOff dec 16 slot >> pokeByteOff dec 24 prev >> pokeByteOff dec 32 gen
      pokeByteOff dec 40 cold >> pokeByteOff dec 72 bsz >> pokeByteOff dec 96 ocn >> pokeByteOff dec 160 hh
      verifyHeaderBytes ctx (castPtr hb) (castPtr out) (castPtr dec)
      -- praos_headers: n, slot, cold_vk, ocert_n are what the fold reads
      fillBytes hv 0 120
      pokeByteOff hv 0 (fromIntegral n :: CSize) >> pokeByteOff hv 8 slot >> pokeByteOff hv 16 cold
      pokeByteOff hv 56 ocn
      fillBytes env 0 120
      pokeByteOff env 0 bno >> pokeByteOff env 8 hh >> pokeByteOff env 16 lenp >> pokeByteOff env 24 bsz
      case tip of
        Nothing -> pokeByteOff env 32 (1 :: Int32)
        Just (s, b, h) -> pokeByteOff env 40 s >> pokeByteOff env 48 b >> pokeBS env 56 h
      pokeByteOff env 88 maxPV >> pokeByteOff env 96 pvMajor >> pokeByteOff env 104 maxHS
      pokeByteOff env 112 maxBS
      checkCtx (ctxPtr ctx) (c_validate_headers (ctxPtr ctx) (castPtr hv) prev gen (castPtr out) (castPtr env) eip st
                                                verdict stopp donep)
      stop <- peek stopp
      vs <- peekArray n verdict
      bs <- peekArray n bits
      st' <- encodeChainState st
      origin :: Int32 <- peekByteOff env 32
      tip' <- if origin /= 0 then pure Nothing else do
        s <- peekByteOff env 40
        b <- peekByteOff env 48
        h <- BS.packCStringLen (castPtr (env `plusPtr` 56), 32)
        pure (Just (s, b, h))
      pure (BatchResult vs bs (fromIntegral stop) st' tip')

-- | 'praosValidateHeaderSpans'' result: the chain stop, the PraosState CBOR and the tip
-- after the last valid header.
data SpanResult = SpanResult
  { srChainStop :: !Int
  , srState     :: !BS.ByteString
  , srTip       :: !(Maybe (Word64, Word64, BS.ByteString))
  }

-- | 'praosValidateHeaderBytes' over Storable vectors: the stored header spans in one arena
-- with their offsets and lengths, the verdicts (PRAOS_V_*) and check bits (PRAOS_BIT_*)
-- written into the caller's mutable vectors (length n each).  An arena of 64 MiB or more is
-- page-locked for the call (praos_host_register: the upload goes by direct DMA, no staging
-- copy).  The decoded fields and nonce values the fold reads stay in one allocation of 157
-- bytes per header.
praosValidateHeaderSpans :: PraosBatchCtx -> (Word64, Word64, Word64, Word64) -> EnvLimits
                         -> Maybe (Word64, Word64, BS.ByteString) -> BS.ByteString -> ArenaPin -> BS.ByteString
                         -> VS.Vector Word64 -> VS.Vector Word32 -> VSM.IOVector Word8 -> VSM.IOVector Word16
                         -> IO SpanResult
praosValidateHeaderSpans ctx ei (maxPV, pvMajor, maxHS, maxBS) tip stateCbor pin arena offs lens
                         verdicts bits = do
  let n = VS.length offs
  when (VS.length lens /= n || VSM.length verdicts /= n || VSM.length bits /= n) $
    throwIO (PraosBatchError (-1) "praosValidateHeaderSpans: vector lengths differ")
  BSU.unsafeUseAsCStringLen arena $ \(ap, alen) ->
    VS.unsafeWith offs $ \offp -> VS.unsafeWith lens $ \lenp ->
    VSM.unsafeWith verdicts $ \verdict -> VSM.unsafeWith bits $ \bitp ->
    allocaBytes 40 $ \hb -> allocaArray n $ \(pidx :: Ptr Int32) ->
    -- decoded fields: slot, block no, ocert n (8 B each), prev hash, cold vk, header hash (32 B
    -- each), body size (4 B), prev-is-genesis (1 B), the nonce value of the certified VRF
    -- output (32 B, the fold evolves the nonce with it) = 157 B per header, one allocation
    allocaBytes (157 * n) $ \decbuf ->
    allocaBytes 168 $ \dec -> allocaBytes 40 $ \out -> allocaBytes 120 $ \hv -> allocaBytes 120 $ \env ->
    alloca $ \stopp -> alloca $ \donep ->
    withChainState stateCbor (n + 65536) $ \st -> withEpochInfo ei $ \eip -> do
      let slot = decbuf :: Ptr Word64
          bno = decbuf `plusPtr` (8 * n) :: Ptr Word64
          ocn = decbuf `plusPtr` (16 * n) :: Ptr Word64
          prev = decbuf `plusPtr` (24 * n) :: Ptr Word8
          cold = decbuf `plusPtr` (56 * n) :: Ptr Word8
          hh = decbuf `plusPtr` (88 * n) :: Ptr Word8
          bsz = decbuf `plusPtr` (120 * n) :: Ptr Word32
          gen = decbuf `plusPtr` (124 * n) :: Ptr Word8
          nonce = decbuf `plusPtr` (125 * n) :: Ptr Word8
      pokeByteOff hb 0 (fromIntegral n :: CSize) >> pokeByteOff hb 8 ap
      pokeByteOff hb 16 (fromIntegral alen :: CSize)
      pokeByteOff hb 24 offp >> pokeByteOff hb 32 lenp
      fillBytes out 0 40 >> pokeByteOff out 0 bitp >> pokeByteOff out 8 pidx >> pokeByteOff out 32 nonce
      fillBytes dec 0 168
      pokeByteOff dec 8 bno >> pokeByteOff dec 16 slot >> pokeByteOff dec 24 prev >> pokeByteOff dec 32 gen
      pokeByteOff dec 40 cold >> pokeByteOff dec 72 bsz >> pokeByteOff dec 96 ocn >> pokeByteOff dec 160 hh
      withRegisteredArena ctx pin (castPtr ap) alen $ verifyHeaderBytes ctx (castPtr hb) (castPtr out) (castPtr dec)
      fillBytes hv 0 120
      pokeByteOff hv 0 (fromIntegral n :: CSize) >> pokeByteOff hv 8 slot >> pokeByteOff hv 16 cold
      pokeByteOff hv 56 ocn
      fillBytes env 0 120
      pokeByteOff env 0 bno >> pokeByteOff env 8 hh >> pokeByteOff env 16 lenp >> pokeByteOff env 24 bsz
      case tip of
        Nothing -> pokeByteOff env 32 (1 :: Int32)
        Just (s, b, h) -> pokeByteOff env 40 s >> pokeByteOff env 48 b >> pokeBS env 56 h
      pokeByteOff env 88 maxPV >> pokeByteOff env 96 pvMajor >> pokeByteOff env 104 maxHS
      pokeByteOff env 112 maxBS
      checkCtx (ctxPtr ctx) (c_validate_headers (ctxPtr ctx) (castPtr hv) prev gen (castPtr out) (castPtr env) eip st
                                                verdict stopp donep)
      stop <- peek stopp
      st' <- encodeChainState st
      origin :: Int32 <- peekByteOff env 32
      tip' <- if origin /= 0 then pure Nothing else do
        s <- peekByteOff env 40
        b <- peekByteOff env 48
        h <- BS.packCStringLen (castPtr (env `plusPtr` 56), 32)
        pure (Just (s, b, h))
      pure (SpanResult (fromIntegral stop) st' tip')

-- ---------------------------------------------------------------- TPraos headers from stored bytes

-- | tickChainDepState's epoch nonce for TPraos (TICKN: candidate ⭒ lastEpochBlock ⭒ the
-- extra entropy of the protocol parameters; Nothing = NeutralNonce).
praosTickedEpochNonceTPraos :: BS.ByteString -> (Word64, Word64, Word64, Word64) -> Word64 -> Maybe BS.ByteString
                            -> IO (Maybe BS.ByteString)
praosTickedEpochNonceTPraos stateCbor ei slot extra =
  withChainState stateCbor (1 + 65536) $ \st -> withEpochInfo ei $ \eip -> allocaBytes 36 $ \xe ->
  allocaBytes 36 $ \out -> do
    pokeNonce xe 0 extra
    rc <- c_tpraos_ticked_epoch_nonce st eip slot (castPtr xe) (castPtr out)
    when (rc /= 0) $ throwIO (PraosBatchError (fromIntegral rc) "praos_tpraos_ticked_epoch_nonce")
    peekNonce out 0

-- | The decentralisation overlay of a TPraos ledger view (praos_overlay): d = lvD, f =
-- activeSlotVal, the fixed-size epoch layout, and lvGenDelegs as (genesis key hash, delegate
-- cold-key hash, delegate VRF key hash) triples.
data OverlayC = OverlayC
  { ovD           :: !Rational
  , ovF           :: !Rational
  , ovEpochBase   :: !Word64
  , ovEpochLength :: !Word64
  , ovGenDelegs   :: ![(BS.ByteString, BS.ByteString, BS.ByteString)]
  }

-- | praos_set_overlay (every member of a group): Nothing = no overlay (d = 0).
-- struct praos_gen_deleg (88 bytes): genesis_hash28@0 delegate_hash28@28 vrf_hash32@56
-- struct praos_overlay (64 bytes): d_num@0 d_den@8 asc_num@16 asc_den@24 epoch_base_slot@32 epoch_length@40 gen_delegs@48 n_gen_delegs@56
praosSetOverlay :: PraosBatchCtx -> Maybe OverlayC -> IO ()
praosSetOverlay ctx Nothing = check ctx $ case ctx of
  PraosBatchCtx p -> c_set_overlay p nullPtr
  PraosBatchGroup g _ _ -> c_group_set_overlay g nullPtr
praosSetOverlay ctx (Just OverlayC {ovD, ovF, ovEpochBase, ovEpochLength, ovGenDelegs}) =
  allocaBytes (88 * max 1 (length ovGenDelegs)) $ \gd -> allocaBytes 64 $ \ov -> do
    forM_ (zip [0 ..] ovGenDelegs) $ \(i, (gk, dk, vrf)) -> do
      let q = gd `plusPtr` (88 * i)
      pokeBS q 0 gk >> pokeBS q 28 dk >> pokeBS q 56 vrf
    fillBytes ov 0 64
    pokeByteOff ov 0 (fromIntegral (numerator ovD) :: Word64) >> pokeByteOff ov 8 (fromIntegral (denominator ovD) :: Word64)
    pokeByteOff ov 16 (fromIntegral (numerator ovF) :: Word64) >> pokeByteOff ov 24 (fromIntegral (denominator ovF) :: Word64)
    pokeByteOff ov 32 ovEpochBase >> pokeByteOff ov 40 ovEpochLength
    pokeByteOff ov 48 gd >> pokeByteOff ov 56 (fromIntegral (length ovGenDelegs) :: Word32)
    check ctx $ case ctx of
      PraosBatchCtx p -> c_set_overlay p (castPtr ov)
      PraosBatchGroup g _ _ -> c_group_set_overlay g (castPtr ov)

-- | One epoch's stored TPraos headers validated (TPraos.updateChainDepState over the
-- batch, TPraos.hs:378-387, with the envelope): verdicts (PRAOS_V_OK / _ENV_* / _INPUT /
-- PRAOS_V_TPRAOS), the PRTCL predicate-failure set of each header (PRAOS_TPF_*), the chain
-- stop and the state / tip after it.
data TPraosBatchResult = TPraosBatchResult
  { tbrVerdicts  :: ![Word8]
  , tbrFailures  :: ![Word16]
  , tbrBits      :: ![Word16]
  , tbrChainStop :: !Int
  , tbrState     :: !BS.ByteString
  , tbrTip       :: !(Maybe (Word64, Word64, BS.ByteString))
  }

-- | praos_verify_tpraos_header_bytes (BHeader decode + OCERT, KES, both VRF certificates
-- and the 2^512 leader test on the GPU) then praos_tpraos_update_chain_dep_state.  The
-- epoch must have been installed with 'praosSetEpoch' under
-- 'praosTickedEpochNonceTPraos''s nonce.
praosValidateTPraosHeaderBytes :: PraosBatchCtx -> (Word64, Word64, Word64, Word64) -> EnvLimits
                               -> Maybe BS.ByteString -> Maybe (Word64, Word64, BS.ByteString) -> BS.ByteString
                               -> [BS.ByteString] -> IO TPraosBatchResult
praosValidateTPraosHeaderBytes ctx ei (maxPV, pvMajor, maxHS, maxBS) extra tip stateCbor hdrs = do
  let n = length hdrs
      arena = BS.concat hdrs
      lens = map BS.length hdrs
      offs = take n (scanl (+) 0 lens)
  BSU.unsafeUseAsCString arena $ \ap ->
    withArray (map fromIntegral offs :: [Word64]) $ \offp ->
    withArray (map fromIntegral lens :: [Word32]) $ \lenp ->
    allocaBytes 40 $ \hb ->
    allocaArray n $ \(bits :: Ptr Word16) -> allocaArray n $ \(pidx :: Ptr Int32) ->
    allocaBytes (32 * n) $ \nonce ->
    allocaArray n $ \(slot :: Ptr Word64) -> allocaArray n $ \(bno :: Ptr Word64) ->
    allocaArray n $ \(ocn :: Ptr Word64) -> allocaArray n $ \(bsz :: Ptr Word32) ->
    allocaBytes (32 * n) $ \prev -> allocaBytes n $ \gen -> allocaBytes (32 * n) $ \cold ->
    allocaBytes (32 * n) $ \hh -> allocaBytes 168 $ \dec -> allocaBytes 40 $ \out ->
    allocaBytes 136 $ \th -> allocaBytes 120 $ \env -> allocaBytes 36 $ \xe ->
    allocaArray n $ \(verdict :: Ptr Word8) -> allocaArray n $ \(fails :: Ptr Word16) ->
    alloca $ \stopp -> alloca $ \donep ->
    withChainState stateCbor (n + 65536) $ \st -> withEpochInfo ei $ \eip -> do
      pokeByteOff hb 0 (fromIntegral n :: CSize) >> pokeByteOff hb 8 ap
      pokeByteOff hb 16 (fromIntegral (BS.length arena) :: CSize)
      pokeByteOff hb 24 offp >> pokeByteOff hb 32 lenp
      -- praos_tpraos_out: bits, pool_idx, (beta_eta, beta_leader not needed), nonce
      fillBytes out 0 40 >> pokeByteOff out 0 bits >> pokeByteOff out 8 pidx >> pokeByteOff out 32 nonce
      fillBytes dec 0 168
      pokeByteOff dec 8 bno >> pokeByteOff dec 16 slot >> pokeByteOff dec 24 prev >> pokeByteOff dec 32 gen
      pokeByteOff dec 40 cold >> pokeByteOff dec 72 bsz >> pokeByteOff dec 96 ocn >> pokeByteOff dec 160 hh
      verifyTPraosHeaderBytes ctx (castPtr hb) (castPtr out) (castPtr dec)
      -- praos_tpraos_headers: h = praos_headers (n, slot, cold_vk, ocert_n read by the fold)
      fillBytes th 0 136
      pokeByteOff th 0 (fromIntegral n :: CSize) >> pokeByteOff th 8 slot >> pokeByteOff th 16 cold
      pokeByteOff th 56 ocn
      fillBytes env 0 120
      pokeByteOff env 0 bno >> pokeByteOff env 8 hh >> pokeByteOff env 16 lenp >> pokeByteOff env 24 bsz
      case tip of
        Nothing -> pokeByteOff env 32 (1 :: Int32)
        Just (s, b, h) -> pokeByteOff env 40 s >> pokeByteOff env 48 b >> pokeBS env 56 h
      pokeByteOff env 88 maxPV >> pokeByteOff env 96 pvMajor >> pokeByteOff env 104 maxHS
      pokeByteOff env 112 maxBS
      pokeNonce xe 0 extra
      checkCtx (ctxPtr ctx) (c_tpraos_update_chain_dep_state (ctxPtr ctx) (castPtr th) prev gen (castPtr out)
                                                             (castPtr env) eip (castPtr xe) st verdict fails stopp donep)
      stop <- peek stopp
      vs <- peekArray n verdict
      fs <- peekArray n fails
      bs <- peekArray n bits
      st' <- encodeChainState st
      origin :: Int32 <- peekByteOff env 32
      tip' <- if origin /= 0 then pure Nothing else do
        s <- peekByteOff env 40
        b <- peekByteOff env 48
        h <- BS.packCStringLen (castPtr (env `plusPtr` 56), 32)
        pure (Just (s, b, h))
      pure (TPraosBatchResult vs fs bs (fromIntegral stop) st' tip')

-- | 'praosValidateTPraosHeaderBytes' over Storable vectors (as 'praosValidateHeaderSpans'):
-- verdicts (PRAOS_V_*), PRTCL failure sets (PRAOS_TPF_*) and check bits written into the
-- caller's vectors.  The epoch must have been installed with 'praosSetEpoch' under
-- 'praosTickedEpochNonceTPraos''s nonce.
praosValidateTPraosHeaderSpans :: PraosBatchCtx -> (Word64, Word64, Word64, Word64) -> EnvLimits -> Maybe BS.ByteString
                               -> Maybe (Word64, Word64, BS.ByteString) -> BS.ByteString -> ArenaPin -> BS.ByteString
                               -> VS.Vector Word64 -> VS.Vector Word32 -> VSM.IOVector Word8 -> VSM.IOVector Word16
                               -> VSM.IOVector Word16 -> IO SpanResult
praosValidateTPraosHeaderSpans ctx ei (maxPV, pvMajor, maxHS, maxBS) extra tip stateCbor pin arena offs lens verdicts
                               failures bits = do
  let n = VS.length offs
  when (VS.length lens /= n || VSM.length verdicts /= n || VSM.length failures /= n || VSM.length bits /= n) $
    throwIO (PraosBatchError (-1) "praosValidateTPraosHeaderSpans: vector lengths differ")
  BSU.unsafeUseAsCStringLen arena $ \(ap, alen) ->
    VS.unsafeWith offs $ \offp -> VS.unsafeWith lens $ \lenp ->
    VSM.unsafeWith verdicts $ \verdict -> VSM.unsafeWith failures $ \fails -> VSM.unsafeWith bits $ \bitp ->
    allocaBytes 40 $ \hb -> allocaArray n $ \(pidx :: Ptr Int32) ->
    allocaBytes (157 * n) $ \decbuf ->      -- the decoded fields the fold reads (praosValidateHeaderSpans)
    allocaBytes 168 $ \dec -> allocaBytes 40 $ \out -> allocaBytes 136 $ \th -> allocaBytes 120 $ \env ->
    allocaBytes 36 $ \xe -> alloca $ \stopp -> alloca $ \donep ->
    withChainState stateCbor (n + 65536) $ \st -> withEpochInfo ei $ \eip -> do
      let slot = decbuf :: Ptr Word64
          bno = decbuf `plusPtr` (8 * n) :: Ptr Word64
          ocn = decbuf `plusPtr` (16 * n) :: Ptr Word64
          prev = decbuf `plusPtr` (24 * n) :: Ptr Word8
          cold = decbuf `plusPtr` (56 * n) :: Ptr Word8
          hh = decbuf `plusPtr` (88 * n) :: Ptr Word8
          bsz = decbuf `plusPtr` (120 * n) :: Ptr Word32
          gen = decbuf `plusPtr` (124 * n) :: Ptr Word8
          nonce = decbuf `plusPtr` (125 * n) :: Ptr Word8
      pokeByteOff hb 0 (fromIntegral n :: CSize) >> pokeByteOff hb 8 ap
      pokeByteOff hb 16 (fromIntegral alen :: CSize)
      pokeByteOff hb 24 offp >> pokeByteOff hb 32 lenp
      fillBytes out 0 40 >> pokeByteOff out 0 bitp >> pokeByteOff out 8 pidx >> pokeByteOff out 32 nonce
      fillBytes dec 0 168
      pokeByteOff dec 8 bno >> pokeByteOff dec 16 slot >> pokeByteOff dec 24 prev >> pokeByteOff dec 32 gen
      pokeByteOff dec 40 cold >> pokeByteOff dec 72 bsz >> pokeByteOff dec 96 ocn >> pokeByteOff dec 160 hh
      withRegisteredArena ctx pin (castPtr ap) alen $ verifyTPraosHeaderBytes ctx (castPtr hb) (castPtr out) (castPtr dec)
      fillBytes th 0 136
      pokeByteOff th 0 (fromIntegral n :: CSize) >> pokeByteOff th 8 slot >> pokeByteOff th 16 cold
      pokeByteOff th 56 ocn
      fillBytes env 0 120
      pokeByteOff env 0 bno >> pokeByteOff env 8 hh >> pokeByteOff env 16 lenp >> pokeByteOff env 24 bsz
      case tip of
        Nothing -> pokeByteOff env 32 (1 :: Int32)
        Just (s, b, h) -> pokeByteOff env 40 s >> pokeByteOff env 48 b >> pokeBS env 56 h
      pokeByteOff env 88 maxPV >> pokeByteOff env 96 pvMajor >> pokeByteOff env 104 maxHS
      pokeByteOff env 112 maxBS
      pokeNonce xe 0 extra
      checkCtx (ctxPtr ctx) (c_tpraos_update_chain_dep_state (ctxPtr ctx) (castPtr th) prev gen (castPtr out)
                                                             (castPtr env) eip (castPtr xe) st verdict fails stopp donep)
      stop <- peek stopp
      st' <- encodeChainState st
      origin :: Int32 <- peekByteOff env 32
      tip' <- if origin /= 0 then pure Nothing else do
        s <- peekByteOff env 40
        b <- peekByteOff env 48
        h <- BS.packCStringLen (castPtr (env `plusPtr` 56), 32)
        pure (Just (s, b, h))
      pure (SpanResult (fromIntegral stop) st' tip')

-- ---------------------------------------------------------------- ImmutableDB replay

data ReplayStats = ReplayStats
  { rsSkipped, rsHeaders, rsValidated, rsStopIndex :: !Word64
  , rsStopVerdict, rsEpochs, rsBatches, rsChunks :: !Word32
  , rsMsIO, rsMsDevice, rsMsFold, rsMsNonce :: !Double
  } deriving Show

-- | praos_replay_immutable: the header-validation pass of db-analyser over an ImmutableDB
-- directory (chunk + secondary index files), from the given state and tip (Nothing =
-- Origin; otherwise a block of the database to resume after).  Returns the statistics,
-- the final PraosState CBOR and tip.  On a group context (praos_group_replay_immutable)
-- consecutive batches go to the members in turn; the nonce chain and the fold stay single,
-- in chain order, so the result is the one-GPU replay's.
praosReplayImmutable :: PraosBatchCtx -> FilePath -> [(BS.ByteString, BS.ByteString, Integer)] -> PraosParamsC
                     -> (Word64, Word64, Word64, Word64) -> EnvLimits -> Maybe (Word64, Word64, BS.ByteString)
                     -> BS.ByteString -> Int
                     -> IO (ReplayStats, BS.ByteString, Maybe (Word64, Word64, BS.ByteString))
praosReplayImmutable ctx dir pools pp ei (maxPV, pvMajor, maxHS, maxBS) tip stateCbor batchMax =
  withCString dir $ \cdir -> withPools pools $ \pp' np -> withParams pp $ \par ->
  withEpochInfo ei $ \eip -> withChainState stateCbor 65536 $ \st ->
  allocaBytes 120 $ \env -> allocaBytes 80 $ \rs -> do
    fillBytes env 0 120
    case tip of
      Nothing -> pokeByteOff env 32 (1 :: Int32)
      Just (s, b, h) -> pokeByteOff env 40 s >> pokeByteOff env 48 b >> pokeBS env 56 h
    pokeByteOff env 88 maxPV >> pokeByteOff env 96 pvMajor >> pokeByteOff env 104 maxHS
    pokeByteOff env 112 maxBS
    check ctx $ case ctx of
      PraosBatchCtx p -> c_replay_immutable p cdir pp' np par eip (castPtr env) st (fromIntegral batchMax) nullPtr 0
                                            (castPtr rs)
      PraosBatchGroup g _ _ -> c_group_replay_immutable g cdir pp' np par eip (castPtr env) st (fromIntegral batchMax)
                                                        nullPtr 0 (castPtr rs)
    stats <- ReplayStats <$> peekByteOff rs 0 <*> peekByteOff rs 8 <*> peekByteOff rs 16 <*> peekByteOff rs 24
                         <*> peekByteOff rs 32 <*> peekByteOff rs 36 <*> peekByteOff rs 40 <*> peekByteOff rs 44
                         <*> peekByteOff rs 48 <*> peekByteOff rs 56 <*> peekByteOff rs 64 <*> peekByteOff rs 72
    st' <- encodeChainState st
    origin :: Int32 <- peekByteOff env 32
    tip' <- if origin /= 0 then pure Nothing else do
      s <- peekByteOff env 40
      b <- peekByteOff env 48
      h <- BS.packCStringLen (castPtr (env `plusPtr` 56), 32)
      pure (Just (s, b, h))
    pure (stats, st', tip')

-- | praos_replay_immutable_tpraos: the same replay over a TPraos (Shelley..Alonzo)
-- ImmutableDB (TICKN's extra entropy, Nothing = NeutralNonce).  Also returns the PRTCL
-- failure set of every header up to the stop (PRAOS_TPF_*).
praosReplayImmutableTPraos :: PraosBatchCtx -> FilePath -> [(BS.ByteString, BS.ByteString, Integer)] -> PraosParamsC
                           -> (Word64, Word64, Word64, Word64) -> EnvLimits -> Maybe BS.ByteString
                           -> Maybe (Word64, Word64, BS.ByteString) -> BS.ByteString -> Int -> Int
                           -> IO (ReplayStats, [Word8], [Word16], BS.ByteString, Maybe (Word64, Word64, BS.ByteString))
praosReplayImmutableTPraos ctx dir pools pp ei (maxPV, pvMajor, maxHS, maxBS) extra tip stateCbor
                           batchMax cap =
  withCString dir $ \cdir -> withPools pools $ \pp' np -> withParams pp $ \par ->
  withEpochInfo ei $ \eip -> withChainState stateCbor 65536 $ \st ->
  allocaBytes 120 $ \env -> allocaBytes 80 $ \rs -> allocaBytes 36 $ \xe ->
  allocaArray (max 1 cap) $ \(verdicts :: Ptr Word8) -> allocaArray (max 1 cap) $ \(fails :: Ptr Word16) -> do
    fillBytes env 0 120
    case tip of
      Nothing -> pokeByteOff env 32 (1 :: Int32)
      Just (s, b, h) -> pokeByteOff env 40 s >> pokeByteOff env 48 b >> pokeBS env 56 h
    pokeByteOff env 88 maxPV >> pokeByteOff env 96 pvMajor >> pokeByteOff env 104 maxHS
    pokeByteOff env 112 maxBS
    pokeNonce xe 0 extra
    check ctx $ case ctx of
      PraosBatchCtx p -> c_replay_immutable_tpraos p cdir pp' np par eip (castPtr xe) (castPtr env) st
                                                   (fromIntegral batchMax) verdicts fails (fromIntegral cap) (castPtr rs)
      PraosBatchGroup g _ _ -> c_group_replay_immutable_tpraos g cdir pp' np par eip (castPtr xe) (castPtr env) st
                                                               (fromIntegral batchMax) verdicts fails
                                                               (fromIntegral cap) (castPtr rs)
    stats <- ReplayStats <$> peekByteOff rs 0 <*> peekByteOff rs 8 <*> peekByteOff rs 16 <*> peekByteOff rs 24
                         <*> peekByteOff rs 32 <*> peekByteOff rs 36 <*> peekByteOff rs 40 <*> peekByteOff rs 44
                         <*> peekByteOff rs 48 <*> peekByteOff rs 56 <*> peekByteOff rs 64 <*> peekByteOff rs 72
    let upto = min cap (fromIntegral (rsHeaders stats))
    vs <- peekArray upto verdicts
    fs <- peekArray upto fails
    st' <- encodeChainState st
    origin :: Int32 <- peekByteOff env 32
    tip' <- if origin /= 0 then pure Nothing else do
      s <- peekByteOff env 40
      b <- peekByteOff env 48
      h <- BS.packCStringLen (castPtr (env `plusPtr` 56), 32)
      pure (Just (s, b, h))
    pure (stats, vs, fs, st', tip')

-- | A LedgerView as the ABI takes it (praos_ledger_view): from which epoch on it holds, the
-- PoolDistr entries and the envelope limits (pvMajor lvProtocolVersion, lvMaxHeaderSize,
-- lvMaxBodySize).  db-analyser forecasts one per epoch from the ledger state it advances
-- (Analysis.hs:564-572; all of them change only at an epoch boundary).
data LedgerViewC = LedgerViewC
  { lvcFirstEpoch :: !Word64
  , lvcPools      :: ![(BS.ByteString, BS.ByteString, Integer)]
  , lvcProtMajor  :: !Word64
  , lvcMaxHeader  :: !Word64
  , lvcMaxBody    :: !Word64
  }

-- | praos_[group_]replay_immutable_views: 'praosReplayImmutable' with a ledger view per epoch
-- (the list sorted by first epoch; epoch e uses the last view starting at or before it) instead
-- of one for the whole database.  A batch never spans two views; the fold of each batch uses
-- its view's PoolDistr and envelope limits.
praosReplayImmutableViews :: PraosBatchCtx -> FilePath -> [LedgerViewC] -> PraosParamsC
                          -> (Word64, Word64, Word64, Word64) -> Word64 -> Maybe (Word64, Word64, BS.ByteString)
                          -> BS.ByteString -> Int
                          -> IO (ReplayStats, BS.ByteString, Maybe (Word64, Word64, BS.ByteString))
praosReplayImmutableViews ctx dir views pp ei maxPV tip stateCbor batchMax =
  withCString dir $ \cdir -> withViews views $ \vp nv -> withParams pp $ \par ->
  withEpochInfo ei $ \eip -> withChainState stateCbor 65536 $ \st ->
  allocaBytes 120 $ \env -> allocaBytes 80 $ \rs -> do
    fillBytes env 0 120
    case tip of
      Nothing -> pokeByteOff env 32 (1 :: Int32)
      Just (s, b, h) -> pokeByteOff env 40 s >> pokeByteOff env 48 b >> pokeBS env 56 h
    pokeByteOff env 88 maxPV             -- the limits of each view come from the view
    check ctx $ case ctx of
      PraosBatchCtx p -> c_replay_immutable_views p cdir vp nv par eip (castPtr env) st (fromIntegral batchMax)
                                                  nullPtr 0 (castPtr rs)
      PraosBatchGroup g _ _ -> c_group_replay_immutable_views g cdir vp nv par eip (castPtr env) st
                                                              (fromIntegral batchMax) nullPtr 0 (castPtr rs)
    stats <- ReplayStats <$> peekByteOff rs 0 <*> peekByteOff rs 8 <*> peekByteOff rs 16 <*> peekByteOff rs 24
                         <*> peekByteOff rs 32 <*> peekByteOff rs 36 <*> peekByteOff rs 40 <*> peekByteOff rs 44
                         <*> peekByteOff rs 48 <*> peekByteOff rs 56 <*> peekByteOff rs 64 <*> peekByteOff rs 72
    st' <- encodeChainState st
    origin :: Int32 <- peekByteOff env 32
    tip' <- if origin /= 0 then pure Nothing else do
      s <- peekByteOff env 40
      b <- peekByteOff env 48
      h <- BS.packCStringLen (castPtr (env `plusPtr` 56), 32)
      pure (Just (s, b, h))
    pure (stats, st', tip')

-- | The praos_ledger_view array (48 bytes each), every view's pool array kept alive around it.
withViews :: [LedgerViewC] -> (Ptr () -> Word32 -> IO a) -> IO a
withViews views k = allocaBytes (48 * max 1 (length views)) $ \vp -> go vp (zip [0 ..] views)
  where
    go vp [] = k (castPtr vp) (fromIntegral (length views))
    go vp ((i, LedgerViewC {lvcFirstEpoch, lvcPools, lvcProtMajor, lvcMaxHeader, lvcMaxBody}) : rest) =
      withPools lvcPools $ \pp np -> do
        let q = vp `plusPtr` (48 * i)
        fillBytes q 0 48
        pokeByteOff q 0 lvcFirstEpoch >> pokeByteOff q 8 pp >> pokeByteOff q 16 np
        pokeByteOff q 24 lvcProtMajor >> pokeByteOff q 32 lvcMaxHeader >> pokeByteOff q 40 lvcMaxBody
        go vp rest

-- ---------------------------------------------------------------- ImmutableDB chunk validation

-- | praos_[group_]verify_block_integrity: 'verifyBlockIntegrity' (Shelley/Ledger/Integrity.hs:14-20
-- = verifyHeaderIntegrity, KES at t = max 0 (kp - c0), and blockMatchesHeader, hashTxSeq of the
-- stored segments) of the blocks @arena[off_i .. off_i + len_i)@, in one GPU batch (sharded over
-- a group's members).  Per block 0 (True) or PRAOS_BLK_* bits (1 decode, 2 KES, 4 body hash).
praosVerifyBlockIntegrity :: PraosBatchCtx -> Word64 -> BS.ByteString -> VS.Vector Word64 -> VS.Vector Word32
                          -> IO (VS.Vector Word8)
praosVerifyBlockIntegrity ctx spkp arena offs lens = do
  let n = VS.length offs
  when (VS.length lens /= n) $ throwIO (PraosBatchError (-1) "praosVerifyBlockIntegrity: vector lengths differ")
  res <- VSM.new n
  BSU.unsafeUseAsCStringLen arena $ \(ap, alen) ->
    VS.unsafeWith offs $ \offp -> VS.unsafeWith lens $ \lenp -> VSM.unsafeWith res $ \rp ->
    allocaBytes 40 $ \hb -> do
      pokeByteOff hb 0 (fromIntegral n :: CSize) >> pokeByteOff hb 8 ap
      pokeByteOff hb 16 (fromIntegral alen :: CSize)
      pokeByteOff hb 24 offp >> pokeByteOff hb 32 lenp
      check ctx $ case ctx of
        PraosBatchCtx p -> c_verify_block_integrity p (castPtr hb) spkp rp nullPtr
        PraosBatchGroup g _ _ -> c_group_verify_block_integrity g (castPtr hb) spkp rp nullPtr
  VS.unsafeFreeze res

-- | Per stored block the outcome of the signature check of its transactions' key witnesses: the
-- check 'applyBlockLedgerResult' makes once per witness under @STS.ValidateAll@
-- (Shelley/Ledger/Ledger.hs:335-352) and 'reapplyBlockLedgerResult' skips.  Status as
-- 'btsStatus'; a block whose @bwsBad@ and @bwsShape@ are both 0 holds no witness whose signature
-- fails.  Which keys had to sign is the ledger's to say and is not looked at.
data BlockWitnessStats = BlockWitnessStats
  { bwsStatus :: !(VS.Vector Word8)
  , bwsNumTxs :: !(VS.Vector Word32)
  , bwsWits   :: !(VS.Vector Word32)    -- ^ VKey and bootstrap witnesses found
  , bwsBad    :: !(VS.Vector Word32)    -- ^ ... whose signature over the txId does not verify
  , bwsShape  :: !(VS.Vector Word32)    -- ^ transactions whose witness set is outside the shapes read
  }

-- | praos_verify_tx_witnesses over the blocks @arena[off_i .. off_i + len_i)@ (whole stored blocks,
-- as 'praosIndexBlockTxs' takes them), the per-block counts only.  @byron@: Byron blocks are
-- indexed (their transactions are skipped, not checked).
praosVerifyTxWitnesses :: PraosBatchCtx -> Bool -> BS.ByteString -> VS.Vector Word64 -> VS.Vector Word32
                       -> IO BlockWitnessStats
praosVerifyTxWitnesses ctx byron arena offs lens = do
  let n = VS.length offs
  when (VS.length lens /= n) $ throwIO (PraosBatchError (-1) "praosVerifyTxWitnesses: vector lengths differ")
  let p = ctxPtr ctx                           -- a group's first member: the check has no group form
  st <- VSM.new n
  ntx <- VSM.new n
  nwit <- VSM.new n
  nbad <- VSM.new n
  nshape <- VSM.new n
  BSU.unsafeUseAsCStringLen arena $ \(ap, alen) ->
    VS.unsafeWith offs $ \offp -> VS.unsafeWith lens $ \lenp ->
    VSM.unsafeWith st $ \stp -> VSM.unsafeWith ntx $ \ntxp -> VSM.unsafeWith nwit $ \nwitp ->
    VSM.unsafeWith nbad $ \nbadp -> VSM.unsafeWith nshape $ \nshapep ->
    allocaBytes 40 $ \hb -> allocaBytes 8 $ \wcfg -> allocaBytes 48 $ \blks -> allocaBytes 72 $ \txs ->
    allocaBytes 64 $ \wits -> do
      pokeByteOff hb 0 (fromIntegral n :: CSize) >> pokeByteOff hb 8 ap
      pokeByteOff hb 16 (fromIntegral alen :: CSize)
      pokeByteOff hb 24 offp >> pokeByteOff hb 32 lenp
      pokeByteOff wcfg 0 (if byron then 1 else 0 :: Word32) >> pokeByteOff wcfg 4 (0 :: Word32)
      fillBytes blks 0 48
      pokeByteOff blks 0 stp >> pokeByteOff blks 8 ntxp >> pokeByteOff blks 16 nwitp
      pokeByteOff blks 24 nbadp >> pokeByteOff blks 32 nshapep
      fillBytes txs 0 72 >> fillBytes wits 0 64      -- no row arrays: the caps are not looked at
      check ctx $ c_verify_tx_witnesses p (castPtr hb) (castPtr wcfg) (castPtr blks) (castPtr txs) (castPtr wits)
  BlockWitnessStats <$> VS.unsafeFreeze st <*> VS.unsafeFreeze ntx <*> VS.unsafeFreeze nwit <*> VS.unsafeFreeze nbad
                    <*> VS.unsafeFreeze nshape

-- | What the BlockFetch client learns about the blocks its peers sent, before ChainSel: per wire
-- item its verdict (0 OK, 1 the wire wrapper, 2 does not decode, 3 not the block asked for, 4 the
-- body does not match the header, 5 more blocks than points, 6 unsupported, 255 after the range's
-- first failure) and the row of its block (0xffffffff: none); per range how many blocks were
-- accepted and its status (0 complete, 1 failed, 2 too few); per distinct block its point and the
-- outcome of the key-witness signature check 'applyBlockLedgerResult' makes under ValidateAll
-- (Shelley/Ledger/Ledger.hs:335-352): @fbrBad@ witnesses fail, @fbrShape@ transactions have a
-- witness set outside the shapes read.
data FetchedBlockResults = FetchedBlockResults
  { fbrVerdict  :: !(VS.Vector Word8)
  , fbrRow      :: !(VS.Vector Word32)
  , fbrAccepted :: !(VS.Vector Word64)
  , fbrStatus   :: !(VS.Vector Word8)
  , fbrSlot     :: !(VS.Vector Word64)
  , fbrBlockNo  :: !(VS.Vector Word64)
  , fbrHash     :: !(VS.Vector Word8)     -- ^ rows x 32
  , fbrNumTxs   :: !(VS.Vector Word32)
  , fbrWits     :: !(VS.Vector Word32)
  , fbrBad      :: !(VS.Vector Word32)
  , fbrShape    :: !(VS.Vector Word32)
  }

-- | praos_verify_fetched_blocks over the wire blocks @arena[off_i .. off_i + len_i)@ (blocks in the
-- node-to-node encoding, as the peers sent them; MiniProtocol/BlockFetch/ClientInterface.hs:157-176),
-- byte-identical blocks sharing a row.  Range r holds the items @[itemFirst_r, itemFirst_(r+1))@
-- and expects the points @[expFirst_r, expFirst_(r+1))@ of @expSlot@ / @expHash@ (32 bytes each).
-- Two calls: the first, without row arrays, gives the number of distinct blocks; it costs a whole
-- run, witness verifies included (a caller that bounds the rows by the item count can skip it).
praosVerifyFetchedBlocks :: PraosBatchCtx -> Word32 -> Word64 -> BS.ByteString -> VS.Vector Word64 -> VS.Vector Word32
                         -> VS.Vector Word64 -> VS.Vector Word64 -> VS.Vector Word64 -> BS.ByteString
                         -> IO FetchedBlockResults
praosVerifyFetchedBlocks ctx nEras byronEpochSlots arena offs lens itemFirst expFirst expSlot expHash = do
  let n = VS.length offs
      k = VS.length itemFirst - 1
  when (VS.length lens /= n || k < 0 || VS.length expFirst /= k + 1 || BS.length expHash /= 32 * VS.length expSlot) $
    throwIO (PraosBatchError (-1) "praosVerifyFetchedBlocks: vector lengths differ")
  let p = ctxPtr ctx                           -- a group's first member: the check has no group form
  vd <- VSM.new n
  row <- VSM.new n
  acc <- VSM.new k
  rst <- VSM.new k
  BSU.unsafeUseAsCStringLen arena $ \(ap, alen) -> BSU.unsafeUseAsCStringLen expHash $ \(ehp, _) ->
    VS.unsafeWith offs $ \offp -> VS.unsafeWith lens $ \lenp -> VS.unsafeWith itemFirst $ \ifp ->
    VS.unsafeWith expFirst $ \efp -> VS.unsafeWith expSlot $ \esp ->
    VSM.unsafeWith vd $ \vdp -> VSM.unsafeWith row $ \rowp -> VSM.unsafeWith acc $ \accp -> VSM.unsafeWith rst $ \rstp ->
    allocaBytes 40 $ \hb -> allocaBytes 40 $ \rgs -> allocaBytes 24 $ \bcfg -> allocaBytes 32 $ \its ->
    allocaBytes 24 $ \rout -> allocaBytes 128 $ \rws -> allocaBytes 48 $ \blks -> allocaBytes 72 $ \txs ->
    allocaBytes 64 $ \wits -> do
      pokeByteOff hb 0 (fromIntegral n :: CSize) >> pokeByteOff hb 8 ap
      pokeByteOff hb 16 (fromIntegral alen :: CSize)
      pokeByteOff hb 24 offp >> pokeByteOff hb 32 lenp
      pokeByteOff rgs 0 (fromIntegral k :: CSize) >> pokeByteOff rgs 8 ifp >> pokeByteOff rgs 16 efp
      pokeByteOff rgs 24 esp >> pokeByteOff rgs 32 ehp
      pokeByteOff bcfg 0 nEras >> pokeByteOff bcfg 4 (1 :: Word32) >> pokeByteOff bcfg 8 (1 :: Word32)
      pokeByteOff bcfg 12 (0 :: Word32) >> pokeByteOff bcfg 16 byronEpochSlots
      fillBytes its 0 32
      pokeByteOff its 16 vdp >> pokeByteOff its 24 rowp
      fillBytes rout 0 24
      pokeByteOff rout 8 accp >> pokeByteOff rout 16 rstp
      fillBytes rws 0 128 >> fillBytes blks 0 48     -- no row arrays: the caps are not looked at
      fillBytes txs 0 72 >> fillBytes wits 0 64
      let call = check ctx $ c_verify_fetched_blocks p (castPtr hb) (castPtr rgs) (castPtr bcfg) (castPtr its)
                   (castPtr rout) (castPtr rws) (castPtr blks) (castPtr txs) (castPtr wits)
      call
      rows <- fromIntegral <$> (peekByteOff rws 8 :: IO CSize)
      slot <- VSM.new rows
      bno <- VSM.new rows
      hh <- VSM.new (32 * rows)
      ntx <- VSM.new rows
      nwit <- VSM.new rows
      nbad <- VSM.new rows
      nshape <- VSM.new rows
      VSM.unsafeWith slot $ \slotp -> VSM.unsafeWith bno $ \bnop -> VSM.unsafeWith hh $ \hhp ->
        VSM.unsafeWith ntx $ \ntxp -> VSM.unsafeWith nwit $ \nwitp -> VSM.unsafeWith nbad $ \nbadp ->
        VSM.unsafeWith nshape $ \nshapep -> do
          pokeByteOff rws 0 (fromIntegral rows :: CSize)
          pokeByteOff rws 40 slotp >> pokeByteOff rws 48 bnop >> pokeByteOff rws 56 hhp
          pokeByteOff blks 8 ntxp >> pokeByteOff blks 16 nwitp >> pokeByteOff blks 24 nbadp >> pokeByteOff blks 32 nshapep
          call
      FetchedBlockResults <$> VS.unsafeFreeze vd <*> VS.unsafeFreeze row <*> VS.unsafeFreeze acc <*> VS.unsafeFreeze rst
                          <*> VS.unsafeFreeze slot <*> VS.unsafeFreeze bno <*> VS.unsafeFreeze hh <*> VS.unsafeFreeze ntx
                          <*> VS.unsafeFreeze nwit <*> VS.unsafeFreeze nbad <*> VS.unsafeFreeze nshape

-- | What the TxSubmission inbound side learns about the transactions its peers offered, before
-- 'addTx': per wire item its status (0 OK, 1..4 the wire wrapper's, 5 not the shape of a
-- transaction, 6 a Byron item, unwrapped only) and the row of its transaction (0xffffffff: none);
-- per distinct transaction what the mempool measures ('txInBlockSize', 'totExUnits') and the
-- outcome of the key-witness signature check 'applyShelleyTx' makes
-- (Shelley/Ledger/Mempool.hs:215-239): @gtrBad@ witnesses fail, @gtrWitStatus@ 1 when the witness
-- set is outside the shapes read.  Which keys had to sign is the ledger's to say.
data GenTxResults = GenTxResults
  { gtrStatus      :: !(VS.Vector Word8)
  , gtrRow         :: !(VS.Vector Word32)
  , gtrTxId        :: !(VS.Vector Word8)     -- ^ rows x 32
  , gtrInBlockSize :: !(VS.Vector Word32)
  , gtrExMem       :: !(VS.Vector Word64)
  , gtrExSteps     :: !(VS.Vector Word64)
  , gtrWitStatus   :: !(VS.Vector Word8)
  , gtrBad         :: !(VS.Vector Word32)
  }

-- | praos_verify_gen_txs over the wire transactions @arena[off_i .. off_i + len_i)@ (GenTxs in the
-- node-to-node encoding, as the peers sent them), byte-identical transactions sharing a row.  Two
-- calls: the first, without row arrays, gives the number of distinct transactions.
praosVerifyGenTxs :: PraosBatchCtx -> Word32 -> BS.ByteString -> VS.Vector Word64 -> VS.Vector Word32
                  -> IO GenTxResults
praosVerifyGenTxs ctx nEras arena offs lens = do
  let n = VS.length offs
  when (VS.length lens /= n) $ throwIO (PraosBatchError (-1) "praosVerifyGenTxs: vector lengths differ")
  let p = ctxPtr ctx                           -- a group's first member: the check has no group form
  st <- VSM.new n
  row <- VSM.new n
  BSU.unsafeUseAsCStringLen arena $ \(ap, alen) ->
    VS.unsafeWith offs $ \offp -> VS.unsafeWith lens $ \lenp ->
    VSM.unsafeWith st $ \stp -> VSM.unsafeWith row $ \rowp ->
    allocaBytes 40 $ \hb -> allocaBytes 16 $ \gcfg -> allocaBytes 48 $ \its -> allocaBytes 168 $ \txs ->
    allocaBytes 64 $ \wits -> do
      pokeByteOff hb 0 (fromIntegral n :: CSize) >> pokeByteOff hb 8 ap
      pokeByteOff hb 16 (fromIntegral alen :: CSize)
      pokeByteOff hb 24 offp >> pokeByteOff hb 32 lenp
      pokeByteOff gcfg 0 nEras >> pokeByteOff gcfg 4 (1 :: Word32)
      pokeByteOff gcfg 8 (0 :: Word32) >> pokeByteOff gcfg 12 (0 :: Word32)
      fillBytes its 0 48
      pokeByteOff its 0 stp >> pokeByteOff its 16 rowp
      fillBytes txs 0 168 >> fillBytes wits 0 64     -- no row arrays: the caps are not looked at
      check ctx $ c_verify_gen_txs p (castPtr hb) (castPtr gcfg) (castPtr its) (castPtr txs) (castPtr wits)
      rows <- fromIntegral <$> (peekByteOff txs 8 :: IO CSize)
      txid <- VSM.new (32 * rows)
      ibs <- VSM.new rows
      mem <- VSM.new rows
      steps <- VSM.new rows
      wst <- VSM.new rows
      bad <- VSM.new rows
      VSM.unsafeWith txid $ \txidp -> VSM.unsafeWith ibs $ \ibsp -> VSM.unsafeWith mem $ \memp ->
        VSM.unsafeWith steps $ \stepsp -> VSM.unsafeWith wst $ \wstp -> VSM.unsafeWith bad $ \badp -> do
          pokeByteOff txs 0 (fromIntegral rows :: CSize)
          pokeByteOff txs 88 ibsp >> pokeByteOff txs 96 memp >> pokeByteOff txs 104 stepsp
          pokeByteOff txs 120 txidp >> pokeByteOff txs 128 wstp >> pokeByteOff txs 152 badp
          check ctx $ c_verify_gen_txs p (castPtr hb) (castPtr gcfg) (castPtr its) (castPtr txs) (castPtr wits)
      GenTxResults <$> VS.unsafeFreeze st <*> VS.unsafeFreeze row <*> VS.unsafeFreeze txid <*> VS.unsafeFreeze ibs
                   <*> VS.unsafeFreeze mem <*> VS.unsafeFreeze steps <*> VS.unsafeFreeze wst <*> VS.unsafeFreeze bad

-- | Per stored block what db-analyser's ledger-free analyses read off its transactions:
-- 'HasAnalysis.blockTxSizes' (its length and sum), 'HasAnalysis.countTxOutputs' and the execution
-- steps of 'HasAnalysis.blockStats' (Cardano/Tools/DBAnalyser/Block/Shelley.hs:61-98,
-- Block/Byron.hs:34-86).  Status 0, or 1 (the block does not decode) / 2 (not the shape of a block
-- of transactions), with zero statistics.
data BlockTxStats = BlockTxStats
  { btsStatus  :: !(VS.Vector Word8)
  , btsNumTxs  :: !(VS.Vector Word32)
  , btsTxsSize :: !(VS.Vector Word64)
  , btsOutputs :: !(VS.Vector Word64)
  , btsExSteps :: !(VS.Vector Word64)
  }

-- | praos_index_block_txs over the blocks @arena[off_i .. off_i + len_i)@ (whole stored blocks, as
-- 'praosVerifyBlockIntegrity' takes them), statistics only: no row array is asked for, so the
-- transaction ids are not computed.  @byron@: Byron blocks and EBBs are indexed too.
praosIndexBlockTxs :: PraosBatchCtx -> Bool -> BS.ByteString -> VS.Vector Word64 -> VS.Vector Word32
                   -> IO BlockTxStats
praosIndexBlockTxs ctx byron arena offs lens = do
  let n = VS.length offs
  when (VS.length lens /= n) $ throwIO (PraosBatchError (-1) "praosIndexBlockTxs: vector lengths differ")
  let p = ctxPtr ctx                           -- a group's first member: the index has no group form
  st <- VSM.new n
  ntx <- VSM.new n
  sz <- VSM.new n
  nout <- VSM.new n
  ex <- VSM.new n
  BSU.unsafeUseAsCStringLen arena $ \(ap, alen) ->
    VS.unsafeWith offs $ \offp -> VS.unsafeWith lens $ \lenp ->
    VSM.unsafeWith st $ \stp -> VSM.unsafeWith ntx $ \ntxp -> VSM.unsafeWith sz $ \szp ->
    VSM.unsafeWith nout $ \noutp -> VSM.unsafeWith ex $ \exp_ ->
    allocaBytes 40 $ \hb -> allocaBytes 8 $ \cfg -> allocaBytes 48 $ \stats -> allocaBytes 112 $ \rows -> do
      pokeByteOff hb 0 (fromIntegral n :: CSize) >> pokeByteOff hb 8 ap
      pokeByteOff hb 16 (fromIntegral alen :: CSize)
      pokeByteOff hb 24 offp >> pokeByteOff hb 32 lenp
      pokeByteOff cfg 0 (if byron then 1 else 0 :: Word32) >> pokeByteOff cfg 4 (0 :: Word32)
      fillBytes stats 0 48
      pokeByteOff stats 0 stp >> pokeByteOff stats 8 ntxp >> pokeByteOff stats 16 szp
      pokeByteOff stats 24 noutp >> pokeByteOff stats 32 exp_
      fillBytes rows 0 112                     -- no row arrays: cap is not looked at
      check ctx $ c_index_block_txs p (castPtr hb) (castPtr cfg) (castPtr stats) (castPtr rows)
  BlockTxStats <$> VS.unsafeFreeze st <*> VS.unsafeFreeze ntx <*> VS.unsafeFreeze sz <*> VS.unsafeFreeze nout
               <*> VS.unsafeFreeze ex

-- | One chunk's validation outcome: per block Nothing (its CRC matched the secondary index's
-- checksum: trusted without the integrity check) or the PRAOS_BLK_* bits (0 = intact), the first
-- corrupt block and the offset the chunk file is truncated at (its length when none).
data ChunkValidation = ChunkValidation
  { cvResults      :: ![Maybe Word8]
  , cvFirstCorrupt :: !(Maybe Int)
  , cvTruncateAt   :: !Word64
  }

-- | The expensive part of ImmutableDB chunk validation batched on the GPUs: parseChunkFile
-- (ImmutableDB/Impl/Parser.hs:118-141, called from validateChunk, Validation.hs:379-384) runs
-- @checkIntegrity@ (= verifyBlockIntegrity) on every block whose CRC32 does not match the
-- secondary index entry's checksum, in file order, and stops at the first corrupt block,
-- truncating the chunk file at its offset.  Here the blocks are the chunk bytes cut at the
-- entries' block offsets (block i ends where block i+1 starts, the last at the end of the
-- chunk, Secondary.hs:93-128); the CRCs are computed on the host ('computeCRC', as parseChunkFile
-- does for every block anyway) and the mismatching blocks go to 'praosVerifyBlockIntegrity' in
-- one call.  (The block decode, the CRC and the prev-hash line-up stay the reference's; this
-- replaces only the @isNotCorrupt@ calls.  Replayed from C by ffi_harness --chunk.)
verifyChunkIntegrity :: PraosBatchCtx -> Word64 -> (BS.ByteString -> Word32) -> BS.ByteString
                     -> [(Word64, Word32)] -> IO ChunkValidation
verifyChunkIntegrity ctx spkp crc32 chunk entries = do
  let n = length entries
      bounds = zip (map fst entries) (drop 1 (map fst entries) ++ [fromIntegral (BS.length chunk)])
      spans = [ (i, o, e - o) | (i, ((o, e), (_, want))) <- zip [0 ..] (zip bounds entries)
                              , crc32 (BS.take (fromIntegral (e - o)) (BS.drop (fromIntegral o) chunk)) /= want ]
  when (or [ e < o || e > fromIntegral (BS.length chunk) | (o, e) <- bounds ]) $
    throwIO (PraosBatchError (-2) "verifyChunkIntegrity: a secondary index entry outside its chunk")
  res <- praosVerifyBlockIntegrity ctx spkp chunk (VS.fromList [ o | (_, o, _) <- spans ])
                                   (VS.fromList [ fromIntegral l | (_, _, l) <- spans ])
  let checked = zip [ i | (i, _, _) <- spans ] (VS.toList res)
      results = [ lookup i checked | i <- [0 .. n - 1] ]
      firstBad = case [ i | (i, r) <- checked, r /= 0 ] of
        (i : _) -> Just i
        []      -> Nothing
  pure ChunkValidation
    { cvResults = results
    , cvFirstCorrupt = firstBad
    , cvTruncateAt = maybe (fromIntegral (BS.length chunk)) (\i -> fst (entries !! i)) firstBad }

-- | What parseChunkFile ended with (ChunkFileError, Parser.hs:60-90), or that the chunk holds
-- a block this library leaves to the reference parser: a Byron block when no Byron parameters
-- were given, or -- with them -- a Byron main block with nTx /= 1 whose only failing check is
-- the Merkle root of its transactions, a rule no reference file pins.
data ChunkOutcome
  = ChunkOK
  | ChunkErrRead                                  -- ^ ChunkErrRead (a ReadIncrementalErr)
  | ChunkErrCorrupt !Word32 !Word64 !BS.ByteString -- ^ PRAOS_BLK_* bits, blockPoint (slot, hash)
  | ChunkErrHashMismatch !BS.ByteString !(Maybe BS.ByteString)
    -- ^ headerHash of the block before, the block's prevHash (Nothing = GenesisHash)
  | ChunkUnsupported
  deriving (Eq, Show)

-- | parseChunkFile's yield: the rebuilt Secondary entries of the valid prefix in their on-disk
-- form (56 bytes each, Secondary.hs:93-128), block numbers and prev hashes (for the Tip and the
-- first block's fit against the previous chunk), the error that ended the parse and the offset
-- to truncate the chunk file at.
data ChunkParse = ChunkParse
  { cpOutcome       :: !ChunkOutcome
  , cpEntries       :: !BS.ByteString
  , cpBlockNos      :: !(VS.Vector Word64)
  , cpFirstPrev     :: !(Maybe (Maybe BS.ByteString))  -- ^ prevHash of block 0 (Just Nothing = GenesisHash)
  , cpChecked       :: !Word64
  , cpTruncateAt    :: !Word64
  , cpRescannedFrom :: !Word64
  , cpIsEBB         :: !(VS.Vector Word8)  -- ^ 1 for an EBB: its entry's blockOrEBB is the epoch number
  , cpByronEpochSlots :: !Word64           -- ^ the Byron epoch length the parse ran with (0: Byron off)
  }

-- | parseChunkFile (ImmutableDB/Impl/Parser.hs:92-197) as one device call: the chunk file as
-- read, the secondary index's checksums (parseChunkFile's [CRC], empty when the index is missing
-- or invalid) and its block offsets as a hint.  CRC-32 of every block, the block boundaries, the
-- header hashes, the prev-hash line-up and verifyBlockIntegrity of the blocks whose checksum does
-- not match all run on the GPU; validateChunk (Validation.hs:374-420) compares 'cpEntries' with
-- the index file's bytes and rewrites it when they differ (immutabledb-validation.patch).
-- Replayed from C by ffi_harness --validate-chunk.
--
-- The Byron parameters, @Just (epochSlots, protocolMagic)@ (epochSlots > 0), switch the Byron
-- era on (praos_validate_chunk_cfg; ffi_harness --validate-chunk-byron): EBBs and Byron main
-- blocks are decoded, PBFT-verified and matched against their body proof like any other block,
-- so a database validates from genesis.  @Nothing@ is the call as it was: a Byron item ends the
-- parse with 'ChunkUnsupported'.
validateChunkBatch :: PraosBatchCtx -> Word64 -> Maybe (Word64, Word32) -> BS.ByteString -> [(Word64, Word32)]
                   -> IO ChunkParse
validateChunkBatch (PraosBatchGroup _ _ _) _ _ _ _ =
  throwIO (PraosBatchError (-2) "validateChunkBatch: one context, not a group")
validateChunkBatch ctx@(PraosBatchCtx p) spkp byron chunk entries = go (max 64 (length entries))
  where
    (byronSlots, byronMagic) = fromMaybe (0, 0) byron
    nExp = length entries
    crcs = VS.fromList (map snd entries)
    offs = VS.fromList (map fst entries)
    go cap = do
      ents <- VSM.new (56 * cap) :: IO (VSM.IOVector Word8)
      bnos <- VSM.new cap :: IO (VSM.IOVector Word64)
      prevs <- VSM.new (32 * cap) :: IO (VSM.IOVector Word8)
      gens <- VSM.new cap :: IO (VSM.IOVector Word8)
      integ <- VSM.new cap :: IO (VSM.IOVector Word8)
      ebbs <- VSM.replicate cap 0 :: IO (VSM.IOVector Word8)
      r <- BSU.unsafeUseAsCStringLen chunk $ \(cp, clen) ->
        VS.unsafeWith crcs $ \crcp -> VS.unsafeWith offs $ \offp ->
        VSM.unsafeWith ents $ \ep -> VSM.unsafeWith bnos $ \bp -> VSM.unsafeWith prevs $ \pp ->
        VSM.unsafeWith gens $ \gp -> VSM.unsafeWith integ $ \ip -> VSM.unsafeWith ebbs $ \bbp ->
        allocaBytes 40 $ \ch -> allocaBytes 152 $ \res -> allocaBytes 48 $ \out -> allocaBytes 24 $ \cfg -> do
          pokeByteOff cfg 0 spkp >> pokeByteOff cfg 8 byronSlots
          pokeByteOff cfg 16 byronMagic >> pokeByteOff cfg 20 (0 :: Word32)
          pokeByteOff ch 0 cp >> pokeByteOff ch 8 (fromIntegral clen :: CSize)
          pokeByteOff ch 16 (if nExp == 0 then nullPtr else crcp)
          pokeByteOff ch 24 (fromIntegral nExp :: CSize)
          pokeByteOff ch 32 (if nExp == 0 then nullPtr else offp)
          pokeByteOff out 0 (fromIntegral cap :: CSize)
          pokeByteOff out 8 ep >> pokeByteOff out 16 bp >> pokeByteOff out 24 pp
          pokeByteOff out 32 gp >> pokeByteOff out 40 ip
          rc <- if byronSlots == 0
                  then c_validate_chunk p (castPtr ch) spkp (castPtr res) (castPtr out)
                  else c_validate_chunk_cfg p (castPtr ch) (castPtr cfg) (castPtr res) (castPtr out) bbp
          blocks <- peekByteOff res 8 :: IO Word64
          if rc == (-2) && blocks > fromIntegral cap
            then pure (Left (fromIntegral blocks))      -- out->cap too small: ask again
            else do
              check ctx (pure rc)
              outcome <- peekByteOff res 0 :: IO Word32
              bits <- peekByteOff res 4 :: IO Word32
              checked <- peekByteOff res 16
              trunc <- peekByteOff res 24
              rescan <- peekByteOff res 32
              slot <- peekByteOff res 40 :: IO Word64
              errHash <- BS.packCStringLen (castPtr res `plusPtr` 48, 32)
              expPrev <- BS.packCStringLen (castPtr res `plusPtr` 80, 32)
              actPrev <- BS.packCStringLen (castPtr res `plusPtr` 112, 32)
              actGen <- peekByteOff res 144 :: IO Word8
              pure (Right (outcome, bits, fromIntegral blocks :: Int, checked, trunc, rescan, slot, errHash,
                           expPrev, actPrev, actGen))
      case r of
        Left need -> go need
        Right (outcome, bits, y, checked, trunc, rescan, slot, errHash, expPrev, actPrev, actGen) -> do
          ev <- VS.unsafeFreeze ents
          bv <- VS.unsafeFreeze bnos
          pv <- VS.unsafeFreeze prevs
          gv <- VS.unsafeFreeze gens
          bbv <- VS.unsafeFreeze ebbs
          let firstPrev | y == 0 = Nothing
                        | gv VS.! 0 /= 0 = Just Nothing
                        | otherwise = Just (Just (BS.pack (VS.toList (VS.take 32 pv))))
              oc = case outcome of
                0 -> ChunkOK
                1 -> ChunkErrRead
                2 -> ChunkErrCorrupt bits slot errHash
                3 -> ChunkErrHashMismatch expPrev (if actGen /= 0 then Nothing else Just actPrev)
                _ -> ChunkUnsupported
          pure ChunkParse
            { cpOutcome = oc
            , cpEntries = BS.pack (VS.toList (VS.take (56 * y) ev))
            , cpBlockNos = VS.take y bv
            , cpFirstPrev = firstPrev
            , cpChecked = checked
            , cpTruncateAt = trunc
            , cpRescannedFrom = rescan
            , cpIsEBB = VS.take y bbv
            , cpByronEpochSlots = byronSlots }

-- ---------------------------------------------------------------- Byron header validation (PBFT)

-- | PBftWindowParams and the Byron block configuration the header check reads.  'pbThreshold' is
-- @floor (pbftSignatureThreshold * k)@ (pbftWindowParams, Protocol/PBFT.hs): the Double stays on
-- this side, the ABI takes the integer.
data PBftParamsC = PBftParamsC
  { pbWindowSize    :: !Word64   -- ^ k
  , pbThreshold     :: !Word64
  , pbEpochSlots    :: !Word64
  , pbProtocolMagic :: !Word32
  }

-- | The old tip: 'Nothing' = Origin, else (slot, block number, header hash, is EBB).
type PBftTipC = Maybe (Word64, Word64, BS.ByteString, Bool)

data PBftBatchResult = PBftBatchResult
  { pbrVerdicts  :: ![Word8]                 -- ^ PRAOS_V_* per header (Batch.Errors rebuilds the typed errors)
  , pbrAux       :: ![Word64]                -- ^ expected block number / minimum slot / the count n
  , pbrBits      :: ![Word8]                 -- ^ PRAOS_PBFT_BIT_*
  , pbrGkIdx     :: ![Int32]                 -- ^ index of the signing delegate's pair in the map, -1 when absent
  , pbrDelegate  :: ![BS.ByteString]         -- ^ hashVerKey of each header's delegate (28 bytes)
  , pbrChainStop :: !Int                     -- ^ the first invalid header (= the batch length when none)
  , pbrState     :: !BS.ByteString           -- ^ encodePBftState of the state at 'pbrChainStop'
  , pbrTip       :: !PBftTipC                -- ^ the tip at 'pbrChainStop'
  }

-- | validateHeader over a batch of stored Byron headers under one delegation map: the envelope
-- (HeaderValidation.hs:297-344, Byron/Ledger/HeaderValidation.hs:39-75), then PBFT
-- updateChainDepState (Protocol/PBFT.hs:320-353).  @headers@: (offset, length) of each header in
-- @arena@ (blockOffset + headerOffset, headerSize of the secondary index); @isEBB@: from the nested
-- context.  @delegs@: (genesis key hash, delegate key hash) pairs, the Bimap of the PBftLedgerView;
-- the caller splits a batch at a re-delegation.  @st@: encodePBftState bytes of the state before the
-- batch.  The per-header half runs on the GPU (praos_verify_pbft_headers), the fold on the host
-- (praos_pbft_update_chain_dep_state); the delegation certificate's own signature is the Byron
-- ledger's check, not this one's.  Replayed from C by ffi_harness --pbft-headers.
validatePBftHeaderBatch :: PraosBatchCtx -> PBftParamsC -> [(BS.ByteString, BS.ByteString)] -> BS.ByteString
                        -> [(Word64, Word32)] -> [Bool] -> PBftTipC -> BS.ByteString -> IO PBftBatchResult
validatePBftHeaderBatch (PraosBatchGroup _ _ _) _ _ _ _ _ _ _ =
  throwIO (PraosBatchError (-2) "validatePBftHeaderBatch: one context, not a group")
validatePBftHeaderBatch ctx@(PraosBatchCtx p) PBftParamsC{pbWindowSize, pbThreshold, pbEpochSlots, pbProtocolMagic}
                        delegs arena headers isEBB tip st = do
  let n = length headers
      nd = length delegs
      cap = fromIntegral (max 1 pbWindowSize) :: Int
      offs = VS.fromList (map fst headers)
      lens = VS.fromList (map snd headers)
      ebbs = VS.fromList (map (\b -> if b then 1 else 0 :: Word8) isEBB)
      dl = VS.fromList (concatMap (\(g, d) -> BS.unpack (pad28 g) ++ BS.unpack (pad28 d)) delegs)
      pad28 b = BS.take 28 (b <> BS.replicate 28 0)
  bits <- VSM.replicate (max 1 n) 0 :: IO (VSM.IOVector Word8)
  gks <- VSM.replicate (max 1 n) (-1) :: IO (VSM.IOVector Int32)
  slots <- VSM.new (max 1 n) :: IO (VSM.IOVector Word64)
  bnos <- VSM.new (max 1 n) :: IO (VSM.IOVector Word64)
  prevs <- VSM.new (32 * max 1 n) :: IO (VSM.IOVector Word8)
  gens <- VSM.new (max 1 n) :: IO (VSM.IOVector Word8)
  hhs <- VSM.new (32 * max 1 n) :: IO (VSM.IOVector Word8)
  dhs <- VSM.replicate (28 * max 1 n) 0 :: IO (VSM.IOVector Word8)
  verd <- VSM.replicate (max 1 n) 0 :: IO (VSM.IOVector Word8)
  aux <- VSM.replicate (max 1 n) 0 :: IO (VSM.IOVector Word64)
  sslot <- VSM.replicate cap 0 :: IO (VSM.IOVector Word64)
  shash <- VSM.replicate (28 * cap) 0 :: IO (VSM.IOVector Word8)
  (stop, enc, tip') <- BSU.unsafeUseAsCStringLen arena $ \(ap, alen) ->
    VS.unsafeWith offs $ \offp -> VS.unsafeWith lens $ \lenp -> VS.unsafeWith ebbs $ \ebbp ->
    VS.unsafeWith dl $ \dlp ->
    VSM.unsafeWith bits $ \bitp -> VSM.unsafeWith gks $ \gkp -> VSM.unsafeWith slots $ \slp ->
    VSM.unsafeWith bnos $ \bnp -> VSM.unsafeWith prevs $ \pvp -> VSM.unsafeWith gens $ \gnp ->
    VSM.unsafeWith hhs $ \hhp -> VSM.unsafeWith dhs $ \dhp -> VSM.unsafeWith verd $ \vp ->
    VSM.unsafeWith aux $ \axp -> VSM.unsafeWith sslot $ \ssp -> VSM.unsafeWith shash $ \shp ->
    allocaBytes 40 $ \hb -> allocaBytes 32 $ \prm -> allocaBytes 64 $ \out -> allocaBytes 56 $ \tp ->
    allocaBytes 32 $ \stp -> alloca $ \stopp -> alloca $ \lenq -> do
      -- praos_header_bytes: n, bytes, bytes_len, off, len
      pokeByteOff hb 0 (fromIntegral n :: CSize) >> pokeByteOff hb 8 ap
      pokeByteOff hb 16 (fromIntegral alen :: CSize) >> pokeByteOff hb 24 offp >> pokeByteOff hb 32 lenp
      pokeByteOff prm 0 pbWindowSize >> pokeByteOff prm 8 pbThreshold >> pokeByteOff prm 16 pbEpochSlots
      pokeByteOff prm 24 pbProtocolMagic >> pokeByteOff prm 28 (0 :: Word32)
      pokeByteOff out 0 bitp >> pokeByteOff out 8 gkp >> pokeByteOff out 16 slp >> pokeByteOff out 24 bnp
      pokeByteOff out 32 pvp >> pokeByteOff out 40 gnp >> pokeByteOff out 48 hhp >> pokeByteOff out 56 dhp
      -- the state before the batch
      pokeByteOff stp 0 (fromIntegral cap :: Word64) >> pokeByteOff stp 8 (0 :: Word64)
      pokeByteOff stp 16 ssp >> pokeByteOff stp 24 shp
      BSU.unsafeUseAsCStringLen st $ \(sp, sl) ->
        check ctx (c_pbft_state_decode (castPtr sp) (fromIntegral sl) (castPtr stp))
      fillBytes tp 0 56
      case tip of
        Nothing -> pokeByteOff tp 0 (1 :: Word8)
        Just (s, b, h, e) -> do
          pokeByteOff tp 1 (if e then 1 else 0 :: Word8)
          pokeByteOff tp 8 s >> pokeByteOff tp 16 b
          BSU.unsafeUseAsCStringLen (BS.take 32 (h <> BS.replicate 32 0)) $ \(hp, _) ->
            copyBytes (castPtr tp `plusPtr` 24) hp 32
      let dlq = if nd == 0 then nullPtr else dlp
      check ctx (c_verify_pbft_headers p (castPtr hb) ebbp (castPtr prm) dlq (fromIntegral nd) (castPtr out))
      check ctx (c_pbft_update_chain_dep_state p (fromIntegral n) (castPtr out) ebbp (castPtr prm) dlq
                   (fromIntegral nd) (castPtr tp) (castPtr stp) vp axp stopp)
      stop <- fromIntegral <$> peek stopp
      _ <- c_pbft_state_encode (castPtr stp) nullPtr 0 lenq
      need <- fromIntegral <$> peek lenq :: IO Int
      enc <- allocaBytes (max 1 need) $ \ep -> do
        check ctx (c_pbft_state_encode (castPtr stp) ep (fromIntegral need) lenq)
        BS.packCStringLen (castPtr ep, need)
      origin <- peekByteOff tp 0 :: IO Word8
      tip' <- if origin /= 0 then pure Nothing else do
        e <- peekByteOff tp 1 :: IO Word8
        s <- peekByteOff tp 8
        b <- peekByteOff tp 16
        h <- BS.packCStringLen (castPtr tp `plusPtr` 24, 32)
        pure (Just (s, b, h, e /= 0))
      pure (stop :: Int, enc, tip')
  vv <- VS.unsafeFreeze verd
  av <- VS.unsafeFreeze aux
  bv <- VS.unsafeFreeze bits
  gv <- VS.unsafeFreeze gks
  dv <- VS.unsafeFreeze dhs
  pure PBftBatchResult
    { pbrVerdicts = VS.toList (VS.take n vv)
    , pbrAux = VS.toList (VS.take n av)
    , pbrBits = VS.toList (VS.take n bv)
    , pbrGkIdx = VS.toList (VS.take n gv)
    , pbrDelegate = [BS.pack (VS.toList (VS.slice (28 * i) 28 dv)) | i <- [0 .. n - 1]]
    , pbrChainStop = stop
    , pbrState = enc
    , pbrTip = tip' }

-- ---------------------------------------------------------------- wire headers, ChainSync candidates

-- | One unwrapped node-to-node header (praos_unwrap_wire_headers): the wrapper of decodeNS
-- (HardFork/Combinator/Serialisation/Common.hs:451-463) around CBOR-in-CBOR bytes
-- (Shelley/Node/Serialisation.hs:110-112), or Byron's @[0, [[kind, sizeHint], #6.24(bytes)]]@
-- (Byron/Node/Serialisation.hs:83-99).  'whEra' is the wire index (Babbage 5), not the disk tag.
data WireHeader = WireHeader
  { whStatus    :: !Word8            -- ^ PRAOS_WIRE_*: 0 OK, 1 range, 2 syntax, 3 era, 4 trailing bytes
  , whEra       :: !Word8
  , whByronKind :: !Word8            -- ^ 0 EBB, 1 main header, 0xff outside Byron
  , whSizeHint  :: !Word32
  , whSpan      :: !(Word64, Word32) -- ^ the inner header in the same arena (offset, length)
  , whHash      :: !BS.ByteString    -- ^ the header hash (32 bytes; zeros unless 'whStatus' is 0)
  }

-- | Unwrap @items@ (offset, length of each wire item in @arena@) on the GPU.  @nEras@ = 7 for the
-- reference's CardanoBlock.  TPraos and Byron callers pass 'whSpan' on to
-- 'praosValidateTPraosHeaderSpans' / 'validatePBftHeaderBatch'.
unwrapWireHeaders :: PraosBatchCtx -> Word32 -> BS.ByteString -> [(Word64, Word32)] -> IO [WireHeader]
unwrapWireHeaders (PraosBatchGroup _ _ _) _ _ _ =
  throwIO (PraosBatchError (-2) "unwrapWireHeaders: one context, not a group")
unwrapWireHeaders ctx@(PraosBatchCtx p) nEras arena items = do
  let n = length items
      m = max 1 n
      offs = VS.fromList (map fst items)
      lens = VS.fromList (map snd items)
  stv <- VSM.replicate m 0 :: IO (VSM.IOVector Word8)
  erv <- VSM.replicate m 0 :: IO (VSM.IOVector Word8)
  kdv <- VSM.replicate m 0 :: IO (VSM.IOVector Word8)
  hnv <- VSM.replicate m 0 :: IO (VSM.IOVector Word32)
  iov <- VSM.replicate m 0 :: IO (VSM.IOVector Word64)
  ilv <- VSM.replicate m 0 :: IO (VSM.IOVector Word32)
  hhv <- VSM.replicate (32 * m) 0 :: IO (VSM.IOVector Word8)
  BSU.unsafeUseAsCStringLen arena $ \(ap, alen) ->
    VS.unsafeWith offs $ \offp -> VS.unsafeWith lens $ \lenp ->
    VSM.unsafeWith stv $ \stp -> VSM.unsafeWith erv $ \erp -> VSM.unsafeWith kdv $ \kdp ->
    VSM.unsafeWith hnv $ \hnp -> VSM.unsafeWith iov $ \iop -> VSM.unsafeWith ilv $ \ilp ->
    VSM.unsafeWith hhv $ \hhp -> allocaBytes 40 $ \hb -> allocaBytes 56 $ \wo -> do
      pokeByteOff hb 0 (fromIntegral n :: CSize) >> pokeByteOff hb 8 ap
      pokeByteOff hb 16 (fromIntegral alen :: CSize) >> pokeByteOff hb 24 offp >> pokeByteOff hb 32 lenp
      pokeByteOff wo 0 stp >> pokeByteOff wo 8 erp >> pokeByteOff wo 16 kdp >> pokeByteOff wo 24 hnp
      pokeByteOff wo 32 iop >> pokeByteOff wo 40 ilp >> pokeByteOff wo 48 hhp
      check ctx (c_unwrap_wire_headers p (castPtr hb) nEras (castPtr wo))
  st <- VS.unsafeFreeze stv
  er <- VS.unsafeFreeze erv
  kd <- VS.unsafeFreeze kdv
  hn <- VS.unsafeFreeze hnv
  io <- VS.unsafeFreeze iov
  il <- VS.unsafeFreeze ilv
  hh <- VS.unsafeFreeze hhv
  pure [ WireHeader (st VS.! i) (er VS.! i) (kd VS.! i) (hn VS.! i) (io VS.! i, il VS.! i)
                    (BS.pack (VS.toList (VS.slice (32 * i) 32 hh)))
       | i <- [0 .. n - 1] ]

-- | One peer's candidate: its wire headers (spans in the call's arena), the head of the fragment
-- ('Nothing' = Origin, else slot, block number, header hash) and the PraosState CBOR there.
data CandidateFragment = CandidateFragment
  { cfItems :: ![(Word64, Word32)]
  , cfTip   :: !(Maybe (Word64, Word64, BS.ByteString))
  , cfState :: !BS.ByteString
  }

-- | The envelope limits of the call's ledger view and how far its forecast reaches.
data CandidateLimits = CandidateLimits
  { clMaxMajorPV    :: !Word64
  , clProtMajor     :: !Word64
  , clMaxHeaderSize :: !Word64
  , clMaxBodySize   :: !Word64
  , clViewEndSlot   :: !Word64   -- ^ first slot the ledger view does not cover ('maxBound': no horizon)
  }

data CandidatesResult = CandidatesResult
  { crVerdicts  :: ![[Word8]]    -- ^ per fragment, per item: PRAOS_V_* (25 DoesntFit, 255 not reached)
  , crStops     :: ![(Int, Int)] -- ^ per fragment: (chain_stop, processed)
  , crTips      :: ![Maybe (Word64, Word64, BS.ByteString)] -- ^ the head at each fragment's stop
  , crStates    :: ![BS.ByteString]                         -- ^ the PraosState CBOR there
  , crStats     :: !(Word64, Word64, Word64, Word64, Word64) -- ^ items, unwrapped, distinct headers, rows, extra rows
  }

-- | What the ChainSync clients of K peers do header by header
-- (MiniProtocol/ChainSync/Client.hs:794-812: the DoesntFit check, then validateHeader), in one
-- call: the items are unwrapped, hashed and deduplicated on the GPU, the header crypto runs once
-- per distinct (header, epoch nonce) pair, each fragment is folded from its own state.  The pools
-- and parameters are those of 'praosSetEpoch'.  The service that collects headers from the
-- client threads into such calls is not part of this module.
validateCandidateFragments :: PraosBatchCtx -> (Word64, Word64, Word64, Word64) -> CandidateLimits
                           -> BS.ByteString -> [CandidateFragment] -> IO CandidatesResult
validateCandidateFragments (PraosBatchGroup _ _ _) _ _ _ _ =
  throwIO (PraosBatchError (-2) "validateCandidateFragments: one context, not a group")
validateCandidateFragments ctx@(PraosBatchCtx p) (baseSlot, baseNo, epochLen, window) lim arena frs = do
  let k = length frs
      items = concatMap cfItems frs
      n = length items
      m = max 1 n
      counts = map (length . cfItems) frs
      firsts = VS.fromList (map fromIntegral (scanl (+) 0 counts) :: [CSize])
      offs = VS.fromList (map fst items)
      lens = VS.fromList (map snd items)
      -- room in each fragment's counter map: the pools a state can name (65536, as withChainState
      -- sizes it) plus one new issuer per item of that fragment; the fragments' arrays lie back to
      -- back at the running offsets capOffs
      caps = map (\c -> 65536 + c) counts :: [Int]
      capOffs = scanl (+) 0 caps
      capTotal = max 1 (sum caps)
  wsv <- VSM.replicate m 0 :: IO (VSM.IOVector Word8)
  rwv <- VSM.replicate m 0 :: IO (VSM.IOVector Word32)
  vdv <- VSM.replicate m 0 :: IO (VSM.IOVector Word8)
  allocaBytes (304 * max 1 k) $ \fr -> allocaBytes (28 * capTotal) $ \hks ->
    allocaBytes (8 * capTotal) $ \ctrs -> do
    fillBytes fr 0 (304 * max 1 k)
    forM_ (zip3 [0 ..] frs (zip caps capOffs)) $ \(j, f, (cap, capOff)) -> do
      let fp = fr `plusPtr` (304 * j) :: Ptr ()
          st = fp `plusPtr` 56 :: Ptr ()
      case cfTip f of
        Nothing -> pokeByteOff fp 0 (1 :: Int32)
        Just (s, b, h) -> do
          pokeByteOff fp 0 (0 :: Int32) >> pokeByteOff fp 8 s >> pokeByteOff fp 16 b
          BSU.unsafeUseAsCStringLen (BS.take 32 (h <> BS.replicate 32 0)) $ \(hp, _) ->
            copyBytes (castPtr fp `plusPtr` 24) hp 32
      -- praos_chain_state: the counter arrays of fragment j, then the decoded state
      pokeByteOff st 16 (hks `plusPtr` (28 * capOff) :: Ptr Word8)
      pokeByteOff st 24 (ctrs `plusPtr` (8 * capOff) :: Ptr Word64)
      pokeByteOff st 40 (fromIntegral cap :: CSize)
      BSU.unsafeUseAsCStringLen (cfState f) $ \(src, sl) -> do
        rc <- c_state_decode (castPtr src) (fromIntegral sl) st
        when (rc /= 0) $ throwIO (PraosBatchError (fromIntegral rc) "praos_state_decode")
    stats <- BSU.unsafeUseAsCStringLen arena $ \(ap, alen) ->
      VS.unsafeWith firsts $ \ffp -> VS.unsafeWith offs $ \offp -> VS.unsafeWith lens $ \lenp ->
      VSM.unsafeWith wsv $ \wsp -> VSM.unsafeWith rwv $ \rwp -> VSM.unsafeWith vdv $ \vdp ->
      allocaBytes 120 $ \cin -> allocaBytes 24 $ \fs -> allocaBytes 312 $ \out -> do
        fillBytes cin 0 120 >> fillBytes out 0 312
        -- praos_candidates_in: items (praos_header_bytes), n_eras, praos_eras (0: 5 and 6), horizon,
        -- epoch info, limits
        pokeByteOff cin 0 (fromIntegral n :: CSize) >> pokeByteOff cin 8 ap
        pokeByteOff cin 16 (fromIntegral alen :: CSize) >> pokeByteOff cin 24 offp >> pokeByteOff cin 32 lenp
        pokeByteOff cin 40 (7 :: Word32) >> pokeByteOff cin 44 (0 :: Word32)
        pokeByteOff cin 48 (clViewEndSlot lim)
        pokeByteOff cin 56 baseSlot >> pokeByteOff cin 64 baseNo >> pokeByteOff cin 72 epochLen
        pokeByteOff cin 80 window
        pokeByteOff cin 88 (clMaxMajorPV lim) >> pokeByteOff cin 96 (clProtMajor lim)
        pokeByteOff cin 104 (clMaxHeaderSize lim) >> pokeByteOff cin 112 (clMaxBodySize lim)
        pokeByteOff fs 0 (fromIntegral k :: CSize) >> pokeByteOff fs 8 ffp >> pokeByteOff fs 16 fr
        -- praos_candidates_out: the per-item arrays; no per-row outputs are asked for (rows_cap = n
        -- bounds the rows, every rows / dec pointer stays NULL)
        pokeByteOff out 0 wsp >> pokeByteOff out 8 rwp >> pokeByteOff out 16 vdp
        pokeByteOff out 24 (fromIntegral n :: CSize)
        check ctx (c_validate_candidates p (castPtr cin) (castPtr fs) (castPtr out))
        s0 <- peekByteOff out 272
        s1 <- peekByteOff out 280
        s2 <- peekByteOff out 288
        s3 <- peekByteOff out 296
        s4 <- peekByteOff out 304
        pure (s0, s1, s2, s3, s4)
    vd <- VS.freeze vdv
    res <- mapM (\j -> do
      let fp = fr `plusPtr` (304 * j) :: Ptr ()
      origin <- peekByteOff fp 0 :: IO Int32
      tip <- if origin /= 0 then pure Nothing else do
        s <- peekByteOff fp 8
        b <- peekByteOff fp 16
        h <- BS.packCStringLen (castPtr fp `plusPtr` 24, 32)
        pure (Just (s, b, h))
      enc <- encodeChainState (fp `plusPtr` 56)
      stop <- peekByteOff fp 288 :: IO CSize
      done <- peekByteOff fp 296 :: IO CSize
      pure (tip, enc, (fromIntegral stop, fromIntegral done))) [0 .. k - 1]
    let starts = scanl (+) 0 counts
    pure CandidatesResult
      { crVerdicts = [VS.toList (VS.slice a c vd) | (a, c) <- zip starts counts]
      , crStops = [x | (_, _, x) <- res]
      , crTips = [t | (t, _, _) <- res]
      , crStates = [e | (_, e, _) <- res]
      , crStats = stats }

-- | 'CandidatesResult' of a TPraos call (verdict 19 = the PRTCL failures) and, per fragment and
-- item, the PRAOS_TPF_* set ("Batch.Errors" tpraosFailures rebuilds the typed failures from it).
data TPraosCandidatesResult = TPraosCandidatesResult
  { tcrResult   :: !CandidatesResult
  , tcrFailures :: ![[Word16]]
  }

-- | 'validateCandidateFragments' for fragments of TPraos headers (Shelley .. Alonzo, wire indices 1
-- to 4): the same pipeline in its TPraos modes.  @extra@: TICKN's extra entropy ('Nothing' =
-- NeutralNonce), combined at every epoch tick of every fragment's nonce chain.  The states are
-- PraosState CBOR as there (TPraos travels in the same praos_chain_state).  Replayed from C by
-- ffi_harness --candidates-tpraos.
validateCandidateFragmentsTPraos :: PraosBatchCtx -> (Word64, Word64, Word64, Word64) -> CandidateLimits
                                 -> Maybe BS.ByteString -> BS.ByteString -> [CandidateFragment]
                                 -> IO TPraosCandidatesResult
validateCandidateFragmentsTPraos (PraosBatchGroup _ _ _) _ _ _ _ _ =
  throwIO (PraosBatchError (-2) "validateCandidateFragmentsTPraos: one context, not a group")
validateCandidateFragmentsTPraos ctx@(PraosBatchCtx p) (baseSlot, baseNo, epochLen, window) lim extra arena frs = do
  let k = length frs
      items = concatMap cfItems frs
      n = length items
      m = max 1 n
      counts = map (length . cfItems) frs
      firsts = VS.fromList (map fromIntegral (scanl (+) 0 counts) :: [CSize])
      offs = VS.fromList (map fst items)
      lens = VS.fromList (map snd items)
      -- room in each fragment's counter map: the pools a state can name (65536, as withChainState
      -- sizes it) plus one new issuer per item of that fragment; the fragments' arrays lie back to
      -- back at the running offsets capOffs
      caps = map (\c -> 65536 + c) counts :: [Int]
      capOffs = scanl (+) 0 caps
      capTotal = max 1 (sum caps)
  wsv <- VSM.replicate m 0 :: IO (VSM.IOVector Word8)
  rwv <- VSM.replicate m 0 :: IO (VSM.IOVector Word32)
  vdv <- VSM.replicate m 0 :: IO (VSM.IOVector Word8)
  flv <- VSM.replicate m 0 :: IO (VSM.IOVector Word16)
  allocaBytes (304 * max 1 k) $ \fr -> allocaBytes (28 * capTotal) $ \hks ->
    allocaBytes (8 * capTotal) $ \ctrs -> do
    fillBytes fr 0 (304 * max 1 k)
    forM_ (zip3 [0 ..] frs (zip caps capOffs)) $ \(j, f, (cap, capOff)) -> do
      let fp = fr `plusPtr` (304 * j) :: Ptr ()
          st = fp `plusPtr` 56 :: Ptr ()
      case cfTip f of
        Nothing -> pokeByteOff fp 0 (1 :: Int32)
        Just (s, b, h) -> do
          pokeByteOff fp 0 (0 :: Int32) >> pokeByteOff fp 8 s >> pokeByteOff fp 16 b
          BSU.unsafeUseAsCStringLen (BS.take 32 (h <> BS.replicate 32 0)) $ \(hp, _) ->
            copyBytes (castPtr fp `plusPtr` 24) hp 32
      -- praos_chain_state: the counter arrays of fragment j, then the decoded state
      pokeByteOff st 16 (hks `plusPtr` (28 * capOff) :: Ptr Word8)
      pokeByteOff st 24 (ctrs `plusPtr` (8 * capOff) :: Ptr Word64)
      pokeByteOff st 40 (fromIntegral cap :: CSize)
      BSU.unsafeUseAsCStringLen (cfState f) $ \(src, sl) -> do
        rc <- c_state_decode (castPtr src) (fromIntegral sl) st
        when (rc /= 0) $ throwIO (PraosBatchError (fromIntegral rc) "praos_state_decode")
    stats <- BSU.unsafeUseAsCStringLen arena $ \(ap, alen) ->
      VS.unsafeWith firsts $ \ffp -> VS.unsafeWith offs $ \offp -> VS.unsafeWith lens $ \lenp ->
      VSM.unsafeWith wsv $ \wsp -> VSM.unsafeWith rwv $ \rwp -> VSM.unsafeWith vdv $ \vdp ->
      VSM.unsafeWith flv $ \flp ->
      allocaBytes 128 $ \cin -> allocaBytes 24 $ \fs -> allocaBytes 336 $ \out -> allocaBytes 36 $ \xe -> do
        fillBytes cin 0 128 >> fillBytes out 0 336 >> fillBytes xe 0 36
        -- praos_tpraos_candidates_in: items (praos_header_bytes), n_eras, tpraos_eras (0: 1 to 4),
        -- horizon, epoch info, limits, TICKN's extra entropy (a praos_nonce: hash, then neutral)
        pokeByteOff cin 0 (fromIntegral n :: CSize) >> pokeByteOff cin 8 ap
        pokeByteOff cin 16 (fromIntegral alen :: CSize) >> pokeByteOff cin 24 offp >> pokeByteOff cin 32 lenp
        pokeByteOff cin 40 (7 :: Word32) >> pokeByteOff cin 44 (0 :: Word32)
        pokeByteOff cin 48 (clViewEndSlot lim)
        pokeByteOff cin 56 baseSlot >> pokeByteOff cin 64 baseNo >> pokeByteOff cin 72 epochLen
        pokeByteOff cin 80 window
        pokeByteOff cin 88 (clMaxMajorPV lim) >> pokeByteOff cin 96 (clProtMajor lim)
        pokeByteOff cin 104 (clMaxHeaderSize lim) >> pokeByteOff cin 112 (clMaxBodySize lim)
        case extra of
          Nothing -> pokeByteOff xe 32 (1 :: Int32)
          Just e -> BSU.unsafeUseAsCStringLen (BS.take 32 (e <> BS.replicate 32 0)) $ \(ep, _) ->
            copyBytes (castPtr xe) ep 32
        pokeByteOff cin 120 (xe :: Ptr ())
        pokeByteOff fs 0 (fromIntegral k :: CSize) >> pokeByteOff fs 8 ffp >> pokeByteOff fs 16 fr
        -- praos_tpraos_candidates_out: the per-item arrays; no per-row outputs are asked for
        -- (rows_cap = n bounds the rows, every rows / dec / leader pointer stays NULL)
        pokeByteOff out 0 wsp >> pokeByteOff out 8 rwp >> pokeByteOff out 16 vdp >> pokeByteOff out 24 flp
        pokeByteOff out 32 (fromIntegral n :: CSize)
        check ctx (c_validate_candidates_tpraos p (castPtr cin) (castPtr fs) (castPtr out))
        s0 <- peekByteOff out 296
        s1 <- peekByteOff out 304
        s2 <- peekByteOff out 312
        s3 <- peekByteOff out 320
        s4 <- peekByteOff out 328
        pure (s0, s1, s2, s3, s4)
    vd <- VS.freeze vdv
    fl <- VS.freeze flv
    res <- mapM (\j -> do
      let fp = fr `plusPtr` (304 * j) :: Ptr ()
      origin <- peekByteOff fp 0 :: IO Int32
      tip <- if origin /= 0 then pure Nothing else do
        s <- peekByteOff fp 8
        b <- peekByteOff fp 16
        h <- BS.packCStringLen (castPtr fp `plusPtr` 24, 32)
        pure (Just (s, b, h))
      enc <- encodeChainState (fp `plusPtr` 56)
      stop <- peekByteOff fp 288 :: IO CSize
      done <- peekByteOff fp 296 :: IO CSize
      pure (tip, enc, (fromIntegral stop, fromIntegral done))) [0 .. k - 1]
    let starts = scanl (+) 0 counts
    pure TPraosCandidatesResult
      { tcrResult = CandidatesResult
          { crVerdicts = [VS.toList (VS.slice a c vd) | (a, c) <- zip starts counts]
          , crStops = [x | (_, _, x) <- res]
          , crTips = [t | (t, _, _) <- res]
          , crStates = [e | (_, e, _) <- res]
          , crStats = stats }
      , tcrFailures = [VS.toList (VS.slice a c fl) | (a, c) <- zip starts counts] }

-- | One peer's candidate of Byron headers: its wire headers (spans in the call's arena), the head
-- of the fragment and the encodePBftState bytes of the PBftState there.
data PBftCandidateFragment = PBftCandidateFragment
  { pcfItems :: ![(Word64, Word32)]
  , pcfTip   :: !PBftTipC
  , pcfState :: !BS.ByteString
  }

data PBftCandidatesResult = PBftCandidatesResult
  { pcrVerdicts :: ![[Word8]]      -- ^ per fragment, per item: PRAOS_V_* (25 DoesntFit, 255 not reached)
  , pcrAux      :: ![[Word64]]     -- ^ expected block number / minimum slot / the count n
  , pcrStops    :: ![(Int, Int)]   -- ^ per fragment: (chain_stop, processed)
  , pcrTips     :: ![PBftTipC]     -- ^ the head at each fragment's stop
  , pcrStates   :: ![BS.ByteString] -- ^ encodePBftState of the state there
  , pcrStats    :: !(Word64, Word64, Word64, Word64) -- ^ items, unwrapped Byron items, distinct headers, signature verifies
  }

-- | 'validateCandidateFragments' for fragments of Byron headers (wire index 0) under one delegation
-- map: the items are unwrapped, hashed and deduplicated on the GPU, the PBFT signature is verified
-- once per distinct header, and each fragment is folded from its own tip and PBftState with the
-- client's DoesntFit check ahead of the envelope.  @viewEnd@: the first slot the ledger view does
-- not cover ('maxBound': no horizon).  Replayed from C by ffi_harness --candidates-pbft.
validateCandidateFragmentsPBft :: PraosBatchCtx -> PBftParamsC -> [(BS.ByteString, BS.ByteString)] -> Word64
                               -> BS.ByteString -> [PBftCandidateFragment] -> IO PBftCandidatesResult
validateCandidateFragmentsPBft (PraosBatchGroup _ _ _) _ _ _ _ _ =
  throwIO (PraosBatchError (-2) "validateCandidateFragmentsPBft: one context, not a group")
validateCandidateFragmentsPBft ctx@(PraosBatchCtx p) PBftParamsC{pbWindowSize, pbThreshold, pbEpochSlots, pbProtocolMagic}
                               delegs viewEnd arena frs = do
  let k = length frs
      items = concatMap pcfItems frs
      n = length items
      m = max 1 n
      nd = length delegs
      counts = map (length . pcfItems) frs
      firsts = VS.fromList (map fromIntegral (scanl (+) 0 counts) :: [CSize])
      offs = VS.fromList (map fst items)
      lens = VS.fromList (map snd items)
      cap = fromIntegral (max 1 pbWindowSize) :: Int
      dl = VS.fromList (concatMap (\(g, d) -> BS.unpack (pad28 g) ++ BS.unpack (pad28 d)) delegs)
      pad28 b = BS.take 28 (b <> BS.replicate 28 0)
  wsv <- VSM.replicate m 0 :: IO (VSM.IOVector Word8)
  rwv <- VSM.replicate m 0 :: IO (VSM.IOVector Word32)
  vdv <- VSM.replicate m 0 :: IO (VSM.IOVector Word8)
  axv <- VSM.replicate m 0 :: IO (VSM.IOVector Word64)
  -- the fragments' window arrays lie back to back: cap signers each
  allocaBytes (104 * max 1 k) $ \fr -> allocaBytes (8 * cap * max 1 k) $ \sslots ->
    allocaBytes (28 * cap * max 1 k) $ \shashes -> do
    fillBytes fr 0 (104 * max 1 k)
    forM_ (zip [0 ..] frs) $ \(j, f) -> do
      let fp = fr `plusPtr` (104 * j) :: Ptr ()
          stp = fp `plusPtr` 56 :: Ptr ()
      case pcfTip f of
        Nothing -> pokeByteOff fp 0 (1 :: Word8)
        Just (s, b, h, e) -> do
          pokeByteOff fp 1 (if e then 1 else 0 :: Word8)
          pokeByteOff fp 8 s >> pokeByteOff fp 16 b
          BSU.unsafeUseAsCStringLen (BS.take 32 (h <> BS.replicate 32 0)) $ \(hp, _) ->
            copyBytes (castPtr fp `plusPtr` 24) hp 32
      -- praos_pbft_state: the arrays of fragment j, then the decoded state
      pokeByteOff stp 0 (fromIntegral cap :: Word64) >> pokeByteOff stp 8 (0 :: Word64)
      pokeByteOff stp 16 (sslots `plusPtr` (8 * cap * j) :: Ptr Word64)
      pokeByteOff stp 24 (shashes `plusPtr` (28 * cap * j) :: Ptr Word8)
      BSU.unsafeUseAsCStringLen (pcfState f) $ \(sp, sl) ->
        check ctx (c_pbft_state_decode (castPtr sp) (fromIntegral sl) (castPtr stp))
    stats <- BSU.unsafeUseAsCStringLen arena $ \(ap, alen) ->
      VS.unsafeWith firsts $ \ffp -> VS.unsafeWith offs $ \offp -> VS.unsafeWith lens $ \lenp ->
      VS.unsafeWith dl $ \dlp ->
      VSM.unsafeWith wsv $ \wsp -> VSM.unsafeWith rwv $ \rwp -> VSM.unsafeWith vdv $ \vdp ->
      VSM.unsafeWith axv $ \axp ->
      allocaBytes 96 $ \cin -> allocaBytes 24 $ \fs -> allocaBytes 152 $ \out -> do
        fillBytes cin 0 96 >> fillBytes out 0 152
        -- praos_pbft_candidates_in: items (praos_header_bytes), n_eras, n_delegs, horizon, params, delegs
        pokeByteOff cin 0 (fromIntegral n :: CSize) >> pokeByteOff cin 8 ap
        pokeByteOff cin 16 (fromIntegral alen :: CSize) >> pokeByteOff cin 24 offp >> pokeByteOff cin 32 lenp
        pokeByteOff cin 40 (7 :: Word32) >> pokeByteOff cin 44 (fromIntegral nd :: Word32)
        pokeByteOff cin 48 viewEnd
        pokeByteOff cin 56 pbWindowSize >> pokeByteOff cin 64 pbThreshold >> pokeByteOff cin 72 pbEpochSlots
        pokeByteOff cin 80 pbProtocolMagic >> pokeByteOff cin 84 (0 :: Word32)
        pokeByteOff cin 88 (if nd == 0 then nullPtr else dlp)
        pokeByteOff fs 0 (fromIntegral k :: CSize) >> pokeByteOff fs 8 ffp >> pokeByteOff fs 16 fr
        -- praos_pbft_candidates_out: the per-item arrays; no per-row outputs are asked for (rows_cap
        -- = n bounds the rows, every rows pointer stays NULL)
        pokeByteOff out 0 wsp >> pokeByteOff out 8 rwp >> pokeByteOff out 16 vdp >> pokeByteOff out 24 axp
        pokeByteOff out 32 (fromIntegral n :: CSize)
        check ctx (c_validate_candidates_pbft p (castPtr cin) (castPtr fs) (castPtr out))
        s0 <- peekByteOff out 120
        s1 <- peekByteOff out 128
        s2 <- peekByteOff out 136
        s3 <- peekByteOff out 144
        pure (s0, s1, s2, s3)
    vd <- VS.freeze vdv
    ax <- VS.freeze axv
    res <- mapM (\j -> alloca $ \lenq -> do
      let fp = fr `plusPtr` (104 * j) :: Ptr ()
          stp = fp `plusPtr` 56 :: Ptr ()
      origin <- peekByteOff fp 0 :: IO Word8
      tip <- if origin /= 0 then pure Nothing else do
        e <- peekByteOff fp 1 :: IO Word8
        s <- peekByteOff fp 8
        b <- peekByteOff fp 16
        h <- BS.packCStringLen (castPtr fp `plusPtr` 24, 32)
        pure (Just (s, b, h, e /= 0))
      _ <- c_pbft_state_encode (castPtr stp) nullPtr 0 lenq
      need <- fromIntegral <$> peek lenq :: IO Int
      enc <- allocaBytes (max 1 need) $ \ep -> do
        check ctx (c_pbft_state_encode (castPtr stp) ep (fromIntegral need) lenq)
        BS.packCStringLen (castPtr ep, need)
      stop <- peekByteOff fp 88 :: IO CSize
      done <- peekByteOff fp 96 :: IO CSize
      pure (tip, enc, (fromIntegral stop, fromIntegral done))) [0 .. k - 1]
    let starts = scanl (+) 0 counts
    pure PBftCandidatesResult
      { pcrVerdicts = [VS.toList (VS.slice a c vd) | (a, c) <- zip starts counts]
      , pcrAux = [VS.toList (VS.slice a c ax) | (a, c) <- zip starts counts]
      , pcrStops = [x | (_, _, x) <- res]
      , pcrTips = [t | (t, _, _) <- res]
      , pcrStates = [e | (_, e, _) <- res]
      , pcrStats = stats }

-- ---------------------------------------------------------------- errors

-- | The reference error a verdict stands for, by name (logs, traces).  The typed
-- constructors with their exact payloads (PraosValidationErr, PraosEnvelopeError,
-- HeaderEnvelopeError, the TPraos PRTCL failures) are built by
-- "Ouroboros.Consensus.Protocol.Praos.Batch.Errors".
-- The bits split KES failures into "Reject" (Merkle path, 0x08) and the Ed25519 leaf
-- ("Verification failed", 0x10), as verifySignedKES reports them.
verdictToError :: Word8 -> Word16 -> Maybe String
verdictToError v bits = case v of
  0  -> Nothing
  1  -> Just "KESBeforeStartOCERT"
  2  -> Just "KESAfterEndOCERT"
  3  -> Just "InvalidSignatureOCERT"
  4  -> Just ("InvalidKesSignatureOCERT " ++ if bits .&. 0x08 /= 0 then "Reject" else "Verification failed")
  5  -> Just "NoCounterForKeyHashOCERT"
  6  -> Just "CounterTooSmallOCERT"
  7  -> Just "CounterOverIncrementedOCERT"
  8  -> Just "VRFKeyUnknown"
  9  -> Just "VRFKeyWrongVRFKey"
  10 -> Just "VRFKeyBadProof"
  11 -> Just "VRFLeaderValueTooBig"
  12 -> Just "(undecodable header)"
  13 -> Just "UnexpectedBlockNo"
  14 -> Just "UnexpectedSlotNo"
  15 -> Just "UnexpectedPrevHash"
  16 -> Just "ObsoleteNode"
  17 -> Just "HeaderSizeTooLarge"
  18 -> Just "BlockSizeTooLarge"
  19 -> Just "ChainTransitionError (TPraos PRTCL failures)"
  20 -> Just "PBftInvalidSignature"
  21 -> Just "PBftInvalidSlot"
  22 -> Just "PBftNotGenesisDelegate"
  23 -> Just "PBftExceededSignThreshold"
  24 -> Just "UnexpectedEBBInSlot"
  25 -> Just "DoesntFit"
  _  -> Just ("unknown verdict " ++ show v)
