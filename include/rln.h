/* rln.h -- zerokit-compatible C ABI of the MI355X RLN backend (drop-in for `librln`).
 *
 * Same symbols, argument meaning, struct layouts, ownership and error convention as the header safer-ffi
 * generates from /root/reference/rln/src/ffi/{ffi_rln,ffi_tree,ffi_utils}.rs (cargo run --features headers
 * --bin generate_headers, rln/src/ffi/mod.rs:11-14).  Each declaration cites the #[ffi_export] it replaces.
 *
 *  - `T* const*` / `T**` arguments are safer-ffi's `&repr_c::Box<T>` / `&mut repr_c::Box<T>`: the address of
 *    the caller's pointer variable (see rln/ffi_c_examples/basic_proof.c:48-49).
 *  - Vec_T = { ptr, len, cap } (rln/ffi_nim_examples/rln.nim:28-46); strings are Vec_uint8_t, NUL-terminated
 *    when produced by the library.
 *  - CResult: `ok` is NULL (or an empty Vec) on failure and `err.ptr` is NULL on success
 *    (ffi_utils.rs:15-29).  Everything returned is caller-owned and released with its `ffi_*_free`.
 *  - CFr is opaque; elements of a Vec_CFr_t are contiguous CFr values reachable through ffi_vec_cfr_get
 *    (ffi_utils.rs:183-185).  In this implementation a CFr is the 32-byte little-endian canonical value.
 *
 * Scope: single and multi message-id circuits, full and partial proofs, the HBM-resident tree with the
 * PmTreeConfig semantics of config_path (path / temporary / tree_depth / flush_every_ms; a persistent tree is the directory
 * <path>: a checksummed snapshot rlnamd_tree.bin plus a write-ahead journal rlnamd_tree.wal.  Every mutating tree call
 * appends one record before it is applied, ffi_flush is an fdatasync of the journal, a flusher thread syncs every
 * flush_every_ms, the journal is folded into a new snapshot as it grows and when the object is freed, and one object at
 * a time may hold a path -- not sled's on-disk format, which belongs to a third-party crate).  Depth <= 30: the dense tree in HBM; depth 31 .. 63: a sparse tree (only written nodes are
 * kept, hashes in device batches -- OptimalMerkleTree's semantics, utils/src/merkle_tree/optimal_merkle_tree.rs);
 * depth >= 64 is the reference's InvalidDepth.  Replacing a dense tree (ffi_set_tree, ffi_init_tree_with_leaves) builds
 * the new one beside the old when the device can hold both and releases the old one first otherwise.  config_path may also carry "window_bits" and "max_batch" (prover sizing, see
 * INTEGRATION.md).  The ffi_rln_v3_* mirror is at the end of this file.
 * Extensions that the reference lacks are marked EXT (deterministic blinding, batch: any n, streamed through the
 * workspace slots).
 */
#ifndef RLN_H
#define RLN_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct CFr CFr_t;                                 /* ffi_utils.rs:34-36  #[repr(opaque)] */
typedef struct FFI_RLN FFI_RLN_t;                         /* ffi_rln.rs:16-18 */
typedef struct FFI_RLNProof FFI_RLNProof_t;               /* ffi_rln.rs:153-155 */
typedef struct FFI_RLNWitnessInput FFI_RLNWitnessInput_t; /* ffi_rln.rs:322-324 */
typedef struct FFI_RLNProofValues FFI_RLNProofValues_t;   /* ffi_rln.rs:714-716 */
typedef struct FFI_RLNPartialWitnessInput FFI_RLNPartialWitnessInput_t; /* ffi_rln.rs:562-564 */
typedef struct FFI_RLNPartialProof FFI_RLNPartialProof_t; /* ffi_rln.rs:239-241 */

typedef struct Vec_uint8 { uint8_t* ptr; size_t len; size_t cap; } Vec_uint8_t;
typedef struct Vec_CFr { CFr_t* ptr; size_t len; size_t cap; } Vec_CFr_t;
typedef struct Vec_size { size_t* ptr; size_t len; size_t cap; } Vec_size_t;
typedef struct Vec_bool { bool* ptr; size_t len; size_t cap; } Vec_bool_t;
typedef struct Vec_String { Vec_uint8_t* ptr; size_t len; size_t cap; } Vec_String_t; /* repr_c::Vec<repr_c::String> */

typedef struct CBoolResult { bool ok; Vec_uint8_t err; } CBoolResult_t;                  /* ffi_utils.rs:24-29 */
typedef struct FFI_MerkleProof { Vec_CFr_t path_elements; Vec_uint8_t path_index; } FFI_MerkleProof_t; /* ffi_tree.rs:13-18 */

typedef struct { FFI_RLN_t* ok; Vec_uint8_t err; } CResult_FFI_RLN_ptr_Vec_uint8_t;
typedef struct { FFI_RLNProof_t* ok; Vec_uint8_t err; } CResult_FFI_RLNProof_ptr_Vec_uint8_t;
typedef struct { FFI_RLNWitnessInput_t* ok; Vec_uint8_t err; } CResult_FFI_RLNWitnessInput_ptr_Vec_uint8_t;
typedef struct { FFI_RLNProofValues_t* ok; Vec_uint8_t err; } CResult_FFI_RLNProofValues_ptr_Vec_uint8_t;
typedef struct { FFI_MerkleProof_t* ok; Vec_uint8_t err; } CResult_FFI_MerkleProof_ptr_Vec_uint8_t;
typedef struct { FFI_RLNPartialWitnessInput_t* ok; Vec_uint8_t err; } CResult_FFI_RLNPartialWitnessInput_ptr_Vec_uint8_t;
typedef struct { FFI_RLNPartialProof_t* ok; Vec_uint8_t err; } CResult_FFI_RLNPartialProof_ptr_Vec_uint8_t;
typedef struct { CFr_t* ok; Vec_uint8_t err; } CResult_CFr_ptr_Vec_uint8_t;
typedef struct { Vec_CFr_t ok; Vec_uint8_t err; } CResult_Vec_CFr_Vec_uint8_t;
typedef struct { Vec_uint8_t ok; Vec_uint8_t err; } CResult_Vec_uint8_Vec_uint8_t;
typedef struct { Vec_bool_t ok; Vec_uint8_t err; } CResult_Vec_bool_Vec_uint8_t;

/* ---- RLN object ------------------------------------------------------------------------------------ */
CResult_FFI_RLN_ptr_Vec_uint8_t ffi_rln_new(size_t tree_depth, const char* config_path);      /* ffi_rln.rs:24-57 */
CResult_FFI_RLN_ptr_Vec_uint8_t ffi_rln_new_with_params(size_t tree_depth, const Vec_uint8_t* zkey_data,
                                                        const Vec_uint8_t* graph_data,
                                                        const char* config_path);             /* ffi_rln.rs:76-116 */
void ffi_rln_free(FFI_RLN_t* rln);                                                            /* ffi_rln.rs:137 */
size_t ffi_rln_get_tree_depth(FFI_RLN_t* const* rln);                                         /* ffi_rln.rs:142 */
size_t ffi_rln_get_max_out(FFI_RLN_t* const* rln);                                            /* ffi_rln.rs:147 */

/* ---- proofs ---------------------------------------------------------------------------------------- */
CResult_FFI_RLNProof_ptr_Vec_uint8_t ffi_generate_rln_proof(FFI_RLN_t* const* rln,
                                                            FFI_RLNWitnessInput_t* const* witness); /* ffi_rln.rs:852-872 */
CBoolResult_t ffi_verify_rln_proof(FFI_RLN_t* const* rln, FFI_RLNProof_t* const* proof, const CFr_t* x); /* :966-984 */
CBoolResult_t ffi_verify_with_roots(FFI_RLN_t* const* rln, FFI_RLNProof_t* const* proof, const Vec_CFr_t* roots,
                                    const CFr_t* x);                                          /* ffi_rln.rs:987-1010 */
/* proof from an externally calculated witness (decimal strings, one per witness signal) */
CResult_FFI_RLNProof_ptr_Vec_uint8_t ffi_generate_rln_proof_with_witness(FFI_RLN_t* const* rln,
                                                                         const Vec_String_t* calculated_witness,
                                                                         FFI_RLNWitnessInput_t* const* witness); /* ffi_rln.rs:875-920 */
/* slashing (protocol/slashing.rs:12-100) */
CResult_CFr_ptr_Vec_uint8_t ffi_compute_id_secret(const CFr_t* share1_x, const CFr_t* share1_y, const CFr_t* share2_x,
                                                  const CFr_t* share2_y);                       /* ffi_rln.rs:1015 */
CResult_CFr_ptr_Vec_uint8_t ffi_recover_id_secret(FFI_RLNProofValues_t* const* proof_values_1,
                                                  FFI_RLNProofValues_t* const* proof_values_2); /* ffi_rln.rs:1036 */
/* EXT: the step of a relay loop behind ffi_verify_rln_proofs_batch: the shares of n proof values through a nullifier
 * log kept on the device (rln_amd.h: rlnamd_nullifier_log_new makes it, the RLNAMD_SHARE_* codes and what a log refuses
 * are described there).  take: NULL, or the `ok` array of the verification -- a proof with take[i] == false is
 * RLNAMD_SHARE_SKIPPED and uses no record (so is a proof without a single share).  A single-message proof is one share
 * (nullifier, x, y, external_nullifier); a multi-message proof is one share per slot whose selector_used is set, in slot
 * order, all with the proof's x, external nullifier and tag (tags[i]; tags NULL: every share's own sequence number in
 * the log).  status[i] is the first of SPAM, FOREIGN, DUPLICATE, NEW that any share of proof i has; secrets[i] (n
 * contiguous CFr, or NULL) and first_tag[i] (or NULL) come from the lowest slot with that status: for SPAM the identity
 * secret recover_id_secret would return for the two proofs, zero otherwise.  Shares do not know which variant they came
 * from: a single-message and a multi-message proof with one nullifier do meet.  All shares of the call go to the log in
 * one observe; an error (null pointers, no room left in the log) leaves the log as it was. */
struct rlnamd_nullifier_log;
CBoolResult_t ffi_nullifier_log_observe(struct rlnamd_nullifier_log* log, FFI_RLNProofValues_t* const* values, size_t n,
                                        const bool* take, const uint64_t* tags, uint8_t* status, CFr_t* secrets,
                                        uint64_t* first_tag);
/* EXT: one log serves the whole window of epochs a relay accepts; when epochs leave it, every record under their k
 * external nullifiers (1 .. RLNAMD_LOG_RETIRE_MAX of them) goes, the rest stays as if those shares had never been
 * observed, and the log has room for *removed (may be NULL) more shares (rln_amd.h: rlnamd_nullifier_log_retire, where
 * the semantics and the refusals are described).  One function for V1 and V3 callers: shares do not know which variant
 * they came from. */
CBoolResult_t ffi_nullifier_log_retire(struct rlnamd_nullifier_log* log, const CFr_t* external_nullifiers, size_t k, size_t* removed); /* EXT */
/* EXT: the other side of the same removal: every record under an external nullifier that is NOT among the k given
 * (1 .. RLNAMD_LOG_RETIRE_MAX of them) goes, however many strangers there are; what a three-call loop does when its
 * clock moves, and after a gap in it.  Everything else is ffi_nullifier_log_retire's contract (rln_amd.h:
 * rlnamd_nullifier_log_retain, where the refusals are listed: a null pointer, k == 0, k too large, an element >= r).
 * One function for V1 and V3 callers. */
CBoolResult_t ffi_nullifier_log_retain(struct rlnamd_nullifier_log* log, const CFr_t* external_nullifiers, size_t k, size_t* removed); /* EXT */
/* EXT: generate_zk_proof_with_rs (protocol/proof.rs:753-777) -- explicit blinding scalars r, s */
CResult_FFI_RLNProof_ptr_Vec_uint8_t ffi_generate_rln_proof_with_rs(FFI_RLN_t* const* rln,
                                                                    FFI_RLNWitnessInput_t* const* witness,
                                                                    const CFr_t* r, const CFr_t* s);
/* EXT: n independent proofs in one device batch.  witnesses: array of n witness pointers; rs: NULL (random
 * blinding) or 2n CFr (r_0, s_0, r_1, ...); out: array of n proof pointers filled on success. */
CBoolResult_t ffi_generate_rln_proofs_batch(FFI_RLN_t* const* rln, FFI_RLNWitnessInput_t* const* witnesses, size_t n,
                                            const CFr_t* rs, FFI_RLNProof_t** out);
/* EXT: n proofs checked in one call.  roots: NULL = this object's current root (ffi_verify_rln_proof),
 * otherwise ffi_verify_with_roots' rule (an empty vector accepts any root).  ok[i] = 1 when proof i passes the
 * three checks of public.rs:725-771 (pairing, root, xs[i] == the proof's x), else 0.  The call itself fails only
 * for a call-level error (null pointers, a proof of the other circuit kind).  The pairing checks run on the device
 * when n is at least the object's "verify_gpu_min" (config JSON), on host threads below it; "verify_lanes" (1 | 8 | 0)
 * names the shape of those device passes (rln_amd.h: rlnamd_verify_many_gpu_ex; 0, the default: by the size of the
 * call).  With "verify_optimistic": true the passes that run a lane per proof try one combined pairing check per chunk
 * first; with "verify_optimistic_teams": true as well, the passes that take teams do too
 * (rln_amd.h: rlnamd_verify_many_gpu_optimistic_ex).  Both default to false. */
CBoolResult_t ffi_verify_rln_proofs_batch(FFI_RLN_t* const* rln, FFI_RLNProof_t* const* proofs, size_t n,
                                          const CFr_t* xs, const Vec_CFr_t* roots, bool* ok);
/* EXT: ffi_verify_rln_proofs_batch from the messages themselves: exactly that call with xs[i] =
 * hash_to_field(signals[i]), the n signals hashed in one call -- on the device when n is at least the object's
 * "hash_gpu_min" (config JSON; rln_amd.h: rlnamd_hasher_*), one by one on the calling thread below it.  A null
 * signals[i].ptr with length 0 is the empty message. */
CBoolResult_t ffi_verify_rln_signals_batch(FFI_RLN_t* const* rln, FFI_RLNProof_t* const* proofs, size_t n,
                                           const Vec_uint8_t* signals, const Vec_CFr_t* roots, bool* ok);
/* EXT: one step of a relay loop in one call: ffi_verify_rln_signals_batch and ffi_nullifier_log_observe(take = ok) over
 * the same inputs, with the cause of a refusal kept.  verdict[i] is RLNAMD_RELAY_OK (0), or the first failing check in
 * the order of ffi_verify_with_roots -- RLNAMD_RELAY_BAD_PROOF, _BAD_ROOT, _BAD_SIGNAL (rln_amd.h) -- so, for a pair
 * without an epoch window (ffi_relay_set_epochs, below), verdict[i] == 0 exactly where ffi_verify_rln_signals_batch
 * gives ok[i]; status, secrets (n contiguous CFr, or NULL) and first_tag (or
 * NULL) are ffi_nullifier_log_observe's, RLNAMD_SHARE_SKIPPED for a refused message.  roots: NULL checks against the
 * object's current root, an empty vector accepts any root.  From "relay_gpu_min" messages on (config JSON, default
 * 1 024: the smallest measured n, at which this call wins by about 0.1 ms of 13, profiles/relay_step.md) the call is ONE rlnamd_relay_step on
 * the device (rln_amd.h), over one relay per (object, log) made on first use with the process's hasher: the signals are
 * hashed beside the pairing kernels and the shares never return to the host.  Then it asks the log for room for n *
 * max_out shares before it starts.  An object with "verify_optimistic": true makes those relays with
 * RLNAMD_RELAY_OPTIMISTIC (and RLNAMD_RELAY_OPTIMISTIC_TEAMS for "verify_optimistic_teams"; rln_amd.h:
 * rlnamd_relay_new_ex), under its "verify_optimistic_cooldown".  Smaller calls and calls with more than
 * RLNAMD_RELAY_ROOTS_MAX roots take the composition of the existing calls.  A log
 * must not be freed while a step on it is running. */
CBoolResult_t ffi_relay_step(FFI_RLN_t* const* rln, struct rlnamd_nullifier_log* log, FFI_RLNProof_t* const* proofs, size_t n,
                             const Vec_uint8_t* signals, const Vec_CFr_t* roots /* NULL: the object's current root */,
                             const uint64_t* tags, uint8_t* verdict, uint8_t* status, CFr_t* secrets, uint64_t* first_tag);
/* EXT: the epoch window of ffi_relay_step for the pair (object, log): the k external nullifiers (0 .. RLNAMD_RELAY_
 * EPOCHS_MAX) the relay follows.  With k >= 1 the log retains the set (ffi_nullifier_log_retain; *removed, may be NULL,
 * is what that removed), whether or not a device relay exists for the pair yet, and only then is the set the window.
 * From then on a message that ffi_relay_step would give RLNAMD_RELAY_OK and whose external nullifier is not in the
 * window gets RLNAMD_RELAY_BAD_EPOCH, status RLNAMD_SHARE_SKIPPED, and never reaches the log; no other verdict changes
 * (rln_amd.h: rlnamd_relay_set_epochs).  The window lives with the pair's relay entry, which is made on first use as a
 * step makes it: it is pushed into the device relay when that exists, applied when the device relay is made later, and
 * judged on the host for the calls that take the composition, so ffi_relay_step gives the same answers on either side
 * of "relay_gpu_min".  k == 0 switches the window off and removes nothing.  Refused with the window and the log as
 * they were: what rlnamd_relay_set_epochs refuses, a null object, a null log.  The window goes with the log: a freed
 * log's entry is dropped. */
CBoolResult_t ffi_relay_set_epochs(FFI_RLN_t* const* rln, struct rlnamd_nullifier_log* log, const CFr_t* external_nullifiers,
                                   size_t k, size_t* removed); /* EXT */

/* EXT: n finishes in one call (single message-id): partials[i] is the partial proof witnesses[i] is finished from -- the
 * same pointer may repeat, one member's partial proof finished for n messages being what partial proofs are for
 * (rln/README.md:360-375); rs: NULL or 2n CFr; out: n proof pointers filled on success.  Any n: chunks of the
 * workspace's capacity, streamed.  The first request that cannot be finished fails the call. */
CBoolResult_t ffi_finish_rln_proofs_batch(FFI_RLN_t* const* rln, FFI_RLNPartialProof_t* const* partials,
                                          FFI_RLNWitnessInput_t* const* witnesses, size_t n, const CFr_t* rs,
                                          FFI_RLNProof_t** out);
/* EXT: n proofs for members of the object's own tree, named by leaf index (single message-id circuits only; a
 * multi-message-id object returns an error naming this function).  What ffi_get_merkle_proof + the witness constructor +
 * ffi_generate_rln_proofs_batch do with n path round trips through the caller, without them: the members' paths are read
 * from the tree on the device, straight into the batch's inputs, at the root the tree has when the call is made (all n
 * proofs at that one root; the object's tree is locked for the call).  Every CFr array holds n contiguous elements; rs:
 * NULL (random blinding) or 2n CFr (r_0, s_0, r_1, ...); out: n proof pointers filled on success.  The range checks and
 * error texts are the witness constructor's (a zero limit, a message_id that is not below the limit); a leaf index
 * >= 2^depth and a tree whose depth is not the circuit's are errors before anything runs.  n above max_batch is streamed
 * in chunks through the object's own prover (replica 0 of a "devices" pool) -- it is NOT dealt to the pool, because the
 * other replicas do not hold the tree.  n = 0 succeeds. */
CBoolResult_t ffi_generate_rln_proofs_for_members(FFI_RLN_t* const* rln, const size_t* leaf_indices, size_t n,
                                                  const CFr_t* identity_secrets, const CFr_t* user_message_limits,
                                                  const CFr_t* message_ids, const CFr_t* xs,
                                                  const CFr_t* external_nullifiers, const CFr_t* rs, FFI_RLNProof_t** out);
/* EXT: ffi_generate_rln_proofs_for_members with the message ids drawn on the device from a quota ledger (rln_amd.h:
 * rlnamd_quota_new makes it, rlnamd_quota_set_epochs opens the external nullifiers signed under; the RLNAMD_QUOTA_* codes
 * and the meaning of a draw are described there).  The caller brings secret, limit, x and external nullifier; request i
 * is (leaf_indices[i], external_nullifiers[i], user_message_limits[i]), ONE draw covers the call, status[i] (n bytes) is
 * its answer, and out[i] is a proof with the id drawn where status[i] is RLNAMD_QUOTA_OK and NULL where no proof was
 * made -- a member past its quota, an external nullifier outside the ledger's window.  No two proofs made through one
 * ledger carry the same (external nullifier, member, message id), so a relay's nullifier log never reports them as spam.
 * Locks: the object's prover, its tree, then the ledger.  Errors before anything is drawn: what
 * ffi_generate_rln_proofs_for_members refuses (a multi-message-id object among it), a null ledger, a ledger whose depth
 * is not the tree's or that lives on another device, a limit of 2^32 or more.  n = 0 succeeds. */
struct rlnamd_quota;
CBoolResult_t ffi_generate_rln_proofs_for_members_drawn(FFI_RLN_t* const* rln, struct rlnamd_quota* quota,
                                                        const size_t* leaf_indices, size_t n, const CFr_t* identity_secrets,
                                                        const CFr_t* user_message_limits, const CFr_t* xs,
                                                        const CFr_t* external_nullifiers, const CFr_t* rs, uint8_t* status,
                                                        FFI_RLNProof_t** out);
/* EXT: the same for a multi-message-id object, one proof of which uses up to max_out message slots.  counts[i] (n bytes,
 * 1 .. max_out) is the number of slots proof i uses; request i is (leaf_indices[i], external_nullifiers[i],
 * user_message_limits[i], counts[i]), ONE rlnamd_quota_draw_counts covers the call and grants each request a block of
 * counts[i] consecutive ids whole or not at all (rln_amd.h states the rule, and that a call is NOT what every split of
 * it gives: a refused request counts, with its whole block, in front of the later requests of its member in the same
 * call).  out[i] is a V1 proof with MultiV1 values -- message ids first .. first + counts[i] - 1 in its first counts[i]
 * slots, their selectors set, the others unused -- where status[i] is RLNAMD_QUOTA_OK, and NULL where no proof was made.
 * The witness constructor's checks apply to what the caller supplies (a zero limit).  Errors before anything is drawn:
 * a single message-id object, a null ledger, a count of 0 or above max_out, a ledger whose depth is not the tree's or
 * that lives on another device, a leaf index >= 2^depth, a limit of 2^32 or more.  n = 0 succeeds. */
CBoolResult_t ffi_generate_rln_proofs_for_members_drawn_multi(FFI_RLN_t* const* rln, struct rlnamd_quota* quota,
                                                              const size_t* leaf_indices, size_t n, const CFr_t* identity_secrets,
                                                              const CFr_t* user_message_limits, const uint8_t* counts,
                                                              const CFr_t* xs, const CFr_t* external_nullifiers, const CFr_t* rs,
                                                              uint8_t* status, FFI_RLNProof_t** out);

FFI_RLNProofValues_t* ffi_rln_proof_get_values(FFI_RLNProof_t* const* proof);                 /* ffi_rln.rs:158 */
uint8_t ffi_rln_proof_get_version_byte(FFI_RLNProof_t* const* proof);                         /* ffi_rln.rs:165 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_proof_to_bytes_le(FFI_RLNProof_t* const* proof);        /* ffi_rln.rs:170 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_proof_to_bytes_be(FFI_RLNProof_t* const* proof);        /* ffi_rln.rs:186 */
CResult_FFI_RLNProof_ptr_Vec_uint8_t ffi_bytes_le_to_rln_proof(const Vec_uint8_t* bytes);     /* ffi_rln.rs:202 */
CResult_FFI_RLNProof_ptr_Vec_uint8_t ffi_bytes_be_to_rln_proof(const Vec_uint8_t* bytes);     /* ffi_rln.rs:218 */
void ffi_rln_proof_free(FFI_RLNProof_t* proof);                                               /* ffi_rln.rs:234 */

/* ---- witness input --------------------------------------------------------------------------------- */
CResult_FFI_RLNWitnessInput_ptr_Vec_uint8_t ffi_rln_witness_input_new_single(
    const CFr_t* identity_secret, const CFr_t* user_message_limit, const CFr_t* message_id,
    const Vec_CFr_t* path_elements, const Vec_uint8_t* identity_path_index, const CFr_t* x,
    const CFr_t* external_nullifier);                                                          /* ffi_rln.rs:327-358 */
CResult_FFI_RLNWitnessInput_ptr_Vec_uint8_t ffi_rln_witness_input_new_multi(
    const CFr_t* identity_secret, const CFr_t* user_message_limit, const Vec_CFr_t* message_ids,
    const Vec_CFr_t* path_elements, const Vec_uint8_t* identity_path_index, const CFr_t* x,
    const CFr_t* external_nullifier, const Vec_bool_t* selector_used);                          /* ffi_rln.rs:361-396 */
Vec_CFr_t ffi_rln_witness_input_get_message_ids(FFI_RLNWitnessInput_t* const* w);              /* ffi_rln.rs:425 */
Vec_bool_t ffi_rln_witness_input_get_selector_used(FFI_RLNWitnessInput_t* const* w);           /* ffi_rln.rs:470 */
void ffi_vec_bool_free(Vec_bool_t v);
uint8_t ffi_rln_witness_input_get_version_byte(FFI_RLNWitnessInput_t* const* w);               /* ffi_rln.rs:399 */
CFr_t* ffi_rln_witness_input_get_identity_secret(FFI_RLNWitnessInput_t* const* w);             /* ffi_rln.rs:404 */
CFr_t* ffi_rln_witness_input_get_user_message_limit(FFI_RLNWitnessInput_t* const* w);          /* ffi_rln.rs:411 */
CFr_t* ffi_rln_witness_input_get_message_id(FFI_RLNWitnessInput_t* const* w);                  /* ffi_rln.rs:418 */
Vec_CFr_t ffi_rln_witness_input_get_path_elements(FFI_RLNWitnessInput_t* const* w);            /* ffi_rln.rs:438 */
Vec_uint8_t ffi_rln_witness_input_get_identity_path_index(FFI_RLNWitnessInput_t* const* w);    /* ffi_rln.rs:451 */
CFr_t* ffi_rln_witness_input_get_x(FFI_RLNWitnessInput_t* const* w);                           /* ffi_rln.rs:458 */
CFr_t* ffi_rln_witness_input_get_external_nullifier(FFI_RLNWitnessInput_t* const* w);          /* ffi_rln.rs:463 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_witness_to_bytes_le(FFI_RLNWitnessInput_t* const* w);    /* ffi_rln.rs:477 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_witness_to_bytes_be(FFI_RLNWitnessInput_t* const* w);    /* ffi_rln.rs:493 */
CResult_FFI_RLNWitnessInput_ptr_Vec_uint8_t ffi_bytes_le_to_rln_witness(const Vec_uint8_t* b); /* ffi_rln.rs:509 */
CResult_FFI_RLNWitnessInput_ptr_Vec_uint8_t ffi_bytes_be_to_rln_witness(const Vec_uint8_t* b); /* ffi_rln.rs:525 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_witness_to_bigint_json(FFI_RLNWitnessInput_t* const* w); /* ffi_rln.rs:541 */
void ffi_rln_witness_input_free(FFI_RLNWitnessInput_t* w);                                     /* ffi_rln.rs:557 */

/* ---- partial proofs (proof split: precompute the member-dependent part, finish per message) ----------- */
CResult_FFI_RLNPartialWitnessInput_ptr_Vec_uint8_t ffi_rln_partial_witness_input_new(
    const CFr_t* identity_secret, const CFr_t* user_message_limit, const Vec_CFr_t* path_elements,
    const Vec_uint8_t* identity_path_index);                                                    /* ffi_rln.rs:567-592 */
FFI_RLNPartialWitnessInput_t* ffi_rln_witness_to_partial_witness(FFI_RLNWitnessInput_t* const* w); /* ffi_rln.rs:636 */
uint8_t ffi_rln_partial_witness_input_get_version_byte(FFI_RLNPartialWitnessInput_t* const* w);  /* ffi_rln.rs:595 */
CFr_t* ffi_rln_partial_witness_input_get_identity_secret(FFI_RLNPartialWitnessInput_t* const* w); /* ffi_rln.rs:602 */
CFr_t* ffi_rln_partial_witness_input_get_user_message_limit(FFI_RLNPartialWitnessInput_t* const* w); /* :609 */
Vec_CFr_t ffi_rln_partial_witness_input_get_path_elements(FFI_RLNPartialWitnessInput_t* const* w); /* :616 */
Vec_uint8_t ffi_rln_partial_witness_input_get_identity_path_index(FFI_RLNPartialWitnessInput_t* const* w); /* :629 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_partial_witness_to_bytes_le(FFI_RLNPartialWitnessInput_t* const* w); /* :644 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_partial_witness_to_bytes_be(FFI_RLNPartialWitnessInput_t* const* w); /* :660 */
CResult_FFI_RLNPartialWitnessInput_ptr_Vec_uint8_t ffi_bytes_le_to_rln_partial_witness(const Vec_uint8_t* b); /* :676 */
CResult_FFI_RLNPartialWitnessInput_ptr_Vec_uint8_t ffi_bytes_be_to_rln_partial_witness(const Vec_uint8_t* b); /* :692 */
void ffi_rln_partial_witness_input_free(FFI_RLNPartialWitnessInput_t* w);                       /* ffi_rln.rs:708 */
CResult_FFI_RLNPartialProof_ptr_Vec_uint8_t ffi_generate_partial_zk_proof(
    FFI_RLN_t* const* rln, FFI_RLNPartialWitnessInput_t* const* partial_witness);               /* ffi_rln.rs:922-936 */
CResult_FFI_RLNProof_ptr_Vec_uint8_t ffi_finish_rln_proof(FFI_RLN_t* const* rln, FFI_RLNPartialProof_t* const* partial,
                                                          FFI_RLNWitnessInput_t* const* witness); /* ffi_rln.rs:939-960 */
/* EXT: finish_zk_proof_with_rs (protocol/proof.rs:821-849) */
CResult_FFI_RLNProof_ptr_Vec_uint8_t ffi_finish_rln_proof_with_rs(FFI_RLN_t* const* rln,
                                                                  FFI_RLNPartialProof_t* const* partial,
                                                                  FFI_RLNWitnessInput_t* const* witness,
                                                                  const CFr_t* r, const CFr_t* s);
uint8_t ffi_rln_partial_proof_get_version_byte(FFI_RLNPartialProof_t* const* partial);          /* ffi_rln.rs:245 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_partial_proof_to_bytes_le(FFI_RLNPartialProof_t* const* partial); /* ffi_rln.rs:252 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_partial_proof_to_bytes_be(FFI_RLNPartialProof_t* const* partial); /* ffi_rln.rs:289 */
CResult_FFI_RLNPartialProof_ptr_Vec_uint8_t ffi_bytes_le_to_rln_partial_proof(const Vec_uint8_t* bytes); /* ffi_rln.rs:268 */
CResult_FFI_RLNPartialProof_ptr_Vec_uint8_t ffi_bytes_be_to_rln_partial_proof(const Vec_uint8_t* bytes); /* ffi_rln.rs:305 */
void ffi_rln_partial_proof_free(FFI_RLNPartialProof_t* partial);                                /* ffi_rln.rs:284 */

/* ---- proof values ---------------------------------------------------------------------------------- */
CFr_t* ffi_rln_proof_values_get_root(FFI_RLNProofValues_t* const* pv);                         /* ffi_rln.rs:719 */
CFr_t* ffi_rln_proof_values_get_x(FFI_RLNProofValues_t* const* pv);                            /* ffi_rln.rs:724 */
CFr_t* ffi_rln_proof_values_get_external_nullifier(FFI_RLNProofValues_t* const* pv);           /* ffi_rln.rs:729 */
CResult_CFr_ptr_Vec_uint8_t ffi_rln_proof_values_get_y(FFI_RLNProofValues_t* const* pv);       /* ffi_rln.rs:736 */
CResult_CFr_ptr_Vec_uint8_t ffi_rln_proof_values_get_nullifier(FFI_RLNProofValues_t* const* pv); /* ffi_rln.rs:746 */
CResult_Vec_bool_Vec_uint8_t ffi_rln_proof_values_get_selector_used(FFI_RLNProofValues_t* const* pv); /* ffi_rln.rs:756 */
CResult_Vec_CFr_Vec_uint8_t ffi_rln_proof_values_get_ys(FFI_RLNProofValues_t* const* pv);      /* ffi_rln.rs:766 */
CResult_Vec_CFr_Vec_uint8_t ffi_rln_proof_values_get_nullifiers(FFI_RLNProofValues_t* const* pv); /* ffi_rln.rs:782 */
uint8_t ffi_rln_proof_values_get_version_byte(FFI_RLNProofValues_t* const* pv);                /* ffi_rln.rs:798 */
Vec_uint8_t ffi_rln_proof_values_to_bytes_le(FFI_RLNProofValues_t* const* pv);                 /* ffi_rln.rs:803 */
Vec_uint8_t ffi_rln_proof_values_to_bytes_be(FFI_RLNProofValues_t* const* pv);                 /* ffi_rln.rs:808 */
CResult_FFI_RLNProofValues_ptr_Vec_uint8_t ffi_bytes_le_to_rln_proof_values(const Vec_uint8_t* b); /* ffi_rln.rs:813 */
CResult_FFI_RLNProofValues_ptr_Vec_uint8_t ffi_bytes_be_to_rln_proof_values(const Vec_uint8_t* b); /* ffi_rln.rs:829 */
void ffi_rln_proof_values_free(FFI_RLNProofValues_t* pv);                                      /* ffi_rln.rs:845 */

/* ---- Merkle tree (ffi_tree.rs) --------------------------------------------------------------------- */
CBoolResult_t ffi_set_tree(FFI_RLN_t** rln, size_t tree_depth);                                /* ffi_tree.rs:28-41 */
CBoolResult_t ffi_delete_leaf(FFI_RLN_t** rln, size_t index);                                  /* ffi_tree.rs:44 */
CBoolResult_t ffi_set_leaf(FFI_RLN_t** rln, size_t index, const CFr_t* leaf);                  /* ffi_tree.rs:58 */
CResult_CFr_ptr_Vec_uint8_t ffi_get_leaf(FFI_RLN_t* const* rln, size_t index);                 /* ffi_tree.rs:72 */
size_t ffi_leaves_set(FFI_RLN_t* const* rln);                                                  /* ffi_tree.rs:89 */
CBoolResult_t ffi_set_next_leaf(FFI_RLN_t** rln, const CFr_t* leaf);                           /* ffi_tree.rs:94 */
CBoolResult_t ffi_set_leaves_from(FFI_RLN_t** rln, size_t index, const Vec_CFr_t* leaves);     /* ffi_tree.rs:108 */
CBoolResult_t ffi_init_tree_with_leaves(FFI_RLN_t** rln, const Vec_CFr_t* leaves);             /* ffi_tree.rs:127 */
CBoolResult_t ffi_atomic_operation(FFI_RLN_t** rln, size_t index, const Vec_CFr_t* leaves,
                                   const Vec_size_t* indices);                                 /* ffi_tree.rs:147 */
CBoolResult_t ffi_seq_atomic_operation(FFI_RLN_t** rln, const Vec_CFr_t* leaves,
                                       const Vec_uint8_t* indices);                            /* ffi_tree.rs:170 */
CFr_t* ffi_get_root(FFI_RLN_t* const* rln);                                                    /* ffi_tree.rs:191 */
CResult_FFI_MerkleProof_ptr_Vec_uint8_t ffi_get_merkle_proof(FFI_RLN_t* const* rln, size_t index); /* ffi_tree.rs:196 */
void ffi_merkle_proof_free(FFI_MerkleProof_t* proof);                                          /* ffi_tree.rs:21 */
CBoolResult_t ffi_set_metadata(FFI_RLN_t** rln, const Vec_uint8_t* metadata);                  /* ffi_tree.rs:231 */
CResult_Vec_uint8_Vec_uint8_t ffi_get_metadata(FFI_RLN_t* const* rln);                         /* ffi_tree.rs:244 */
CBoolResult_t ffi_flush(FFI_RLN_t** rln);                                                      /* ffi_tree.rs:257 */

/* ---- field / vector helpers (ffi_utils.rs) --------------------------------------------------------- */
CFr_t* ffi_cfr_zero(void);                                                                     /* ffi_utils.rs:70 */
CFr_t* ffi_cfr_one(void);                                                                      /* ffi_utils.rs:75 */
CResult_Vec_uint8_Vec_uint8_t ffi_cfr_to_bytes_le(const CFr_t* cfr);                           /* ffi_utils.rs:80 */
CResult_Vec_uint8_Vec_uint8_t ffi_cfr_to_bytes_be(const CFr_t* cfr);                           /* ffi_utils.rs:95 */
CResult_CFr_ptr_Vec_uint8_t ffi_bytes_le_to_cfr(const Vec_uint8_t* bytes);                     /* ffi_utils.rs:110 */
CResult_CFr_ptr_Vec_uint8_t ffi_bytes_be_to_cfr(const Vec_uint8_t* bytes);                     /* ffi_utils.rs:124 */
CFr_t* ffi_uint_to_cfr(uint32_t value);                                                        /* ffi_utils.rs:138 */
Vec_uint8_t ffi_cfr_debug(const CFr_t* cfr);                                                   /* ffi_utils.rs:143 */
void ffi_cfr_free(CFr_t* cfr);                                                                 /* ffi_utils.rs:151 */
Vec_CFr_t ffi_vec_cfr_new(size_t capacity);                                                    /* ffi_utils.rs:158 */
Vec_CFr_t ffi_vec_cfr_from_cfr(const CFr_t* cfr);                                              /* ffi_utils.rs:163 */
void ffi_vec_cfr_push(Vec_CFr_t* v, const CFr_t* cfr);                                         /* ffi_utils.rs:168 */
size_t ffi_vec_cfr_len(const Vec_CFr_t* v);                                                    /* ffi_utils.rs:178 */
const CFr_t* ffi_vec_cfr_get(const Vec_CFr_t* v, size_t i);                                    /* ffi_utils.rs:183 */
CResult_Vec_uint8_Vec_uint8_t ffi_vec_cfr_to_bytes_le(const Vec_CFr_t* v);                     /* ffi_utils.rs:188 */
CResult_Vec_uint8_Vec_uint8_t ffi_vec_cfr_to_bytes_be(const Vec_CFr_t* v);                     /* ffi_utils.rs:204 */
CResult_Vec_CFr_Vec_uint8_t ffi_bytes_le_to_vec_cfr(const Vec_uint8_t* bytes);                 /* ffi_utils.rs:220 */
CResult_Vec_CFr_Vec_uint8_t ffi_bytes_be_to_vec_cfr(const Vec_uint8_t* bytes);                 /* ffi_utils.rs:240 */
Vec_uint8_t ffi_vec_cfr_debug(const Vec_CFr_t* v);                                             /* ffi_utils.rs:259 */
void ffi_vec_cfr_free(Vec_CFr_t v);                                                            /* ffi_utils.rs:270 */
CResult_Vec_uint8_Vec_uint8_t ffi_vec_u8_to_bytes_le(const Vec_uint8_t* v);                    /* ffi_utils.rs:277 */
CResult_Vec_uint8_Vec_uint8_t ffi_vec_u8_to_bytes_be(const Vec_uint8_t* v);                    /* ffi_utils.rs:292 */
CResult_Vec_uint8_Vec_uint8_t ffi_bytes_le_to_vec_u8(const Vec_uint8_t* bytes);                /* ffi_utils.rs:307 */
CResult_Vec_uint8_Vec_uint8_t ffi_bytes_be_to_vec_u8(const Vec_uint8_t* bytes);                /* ffi_utils.rs:321 */
Vec_uint8_t ffi_vec_u8_debug(const Vec_uint8_t* v);                                            /* ffi_utils.rs:335 */
void ffi_vec_u8_free(Vec_uint8_t v);                                                           /* ffi_utils.rs:343 */
CFr_t* ffi_hash_to_field_le(const Vec_uint8_t* input);                                         /* ffi_utils.rs:349 */
CFr_t* ffi_hash_to_field_be(const Vec_uint8_t* input);                                         /* ffi_utils.rs:354 */
/* EXT: ffi_hash_to_field_le / _be of n signals in one call; out: n CFr.  Over one hasher per device for the whole process,
 * made on first use (rln_amd.h: rlnamd_hasher_*); small calls are hashed on the calling thread.  Both give the same
 * result, as the single calls do. */
CBoolResult_t ffi_hash_to_field_batch_le(const Vec_uint8_t* signals, size_t n, CFr_t* out);
CBoolResult_t ffi_hash_to_field_batch_be(const Vec_uint8_t* signals, size_t n, CFr_t* out);
/* The five functions below have no error channel in the reference ABI.  A device failure (no GPU, out of memory)
 * is reported on stderr and by a NULL pointer / an empty vector {NULL, 0, 0} -- never by a zero "result". */
CFr_t* ffi_poseidon_hash_pair(const CFr_t* a, const CFr_t* b);                                 /* ffi_utils.rs:359 */
Vec_CFr_t ffi_key_gen(void);                                                                   /* ffi_utils.rs:366 */
Vec_CFr_t ffi_seeded_key_gen(const Vec_uint8_t* seed);                                         /* ffi_utils.rs:372 */
Vec_CFr_t ffi_extended_key_gen(void);                                                          /* ffi_utils.rs:380 */
Vec_CFr_t ffi_seeded_extended_key_gen(const Vec_uint8_t* seed);                                /* ffi_utils.rs:392 */
void ffi_c_string_free(Vec_uint8_t s);                                                         /* ffi_utils.rs:407 */

/* ==== V3 mirror (rln/src/ffi/ffi_rln_v3.rs:323-1609) -- what rln/ffi_c_examples and rln/ffi_nim_examples call.
 * Same objects as above behind V3 names; differences: stateless / tree-flavour constructors, V3 error texts
 * (rln/src/error.rs:104-208), ffi_rln_v3_verify returning plain `false` on a signal mismatch, and the V3 wire
 * formats (protocol/serialize.rs): enum tag 0/1, values ordered y|root|nullifier|x|ext, proofs without a leading
 * version byte, "mixed" = LE proof + BE values; deserialisers accept trailing bytes.  All three tree flavours map
 * to the one device-resident tree; the pm-tree variant keeps no on-disk state. */
typedef struct FFI_RLNV3 FFI_RLNV3_t;                                   /* ffi_rln_v3.rs:310-312 */
typedef struct FFI_RLNV3WitnessInput FFI_RLNV3WitnessInput_t;           /* ffi_rln_v3.rs:612-614 */
typedef struct FFI_RLNV3PartialWitnessInput FFI_RLNV3PartialWitnessInput_t; /* ffi_rln_v3.rs:864-866 */
typedef struct FFI_RLNV3Proof FFI_RLNV3Proof_t;                         /* ffi_rln_v3.rs:1011-1013 */
typedef struct FFI_RLNV3PartialProof FFI_RLNV3PartialProof_t;           /* ffi_rln_v3.rs:1095-1097 */
typedef struct FFI_RLNV3ProofValues FFI_RLNV3ProofValues_t;             /* ffi_rln_v3.rs:1139-1141 */
typedef struct FFI_RLNV3MerkleProof { Vec_CFr_t path_elements; Vec_uint8_t path_index; } FFI_RLNV3MerkleProof_t; /* :1363-1368 */
typedef struct { FFI_RLNV3_t* ok; Vec_uint8_t err; } CResult_FFI_RLNV3_ptr_Vec_uint8_t;
typedef struct { FFI_RLNV3WitnessInput_t* ok; Vec_uint8_t err; } CResult_FFI_RLNV3WitnessInput_ptr_Vec_uint8_t;
typedef struct { FFI_RLNV3PartialWitnessInput_t* ok; Vec_uint8_t err; } CResult_FFI_RLNV3PartialWitnessInput_ptr_Vec_uint8_t;
typedef struct { FFI_RLNV3Proof_t* ok; Vec_uint8_t err; } CResult_FFI_RLNV3Proof_ptr_Vec_uint8_t;
typedef struct { FFI_RLNV3PartialProof_t* ok; Vec_uint8_t err; } CResult_FFI_RLNV3PartialProof_ptr_Vec_uint8_t;
typedef struct { FFI_RLNV3ProofValues_t* ok; Vec_uint8_t err; } CResult_FFI_RLNV3ProofValues_ptr_Vec_uint8_t;
typedef struct { FFI_RLNV3MerkleProof_t* ok; Vec_uint8_t err; } CResult_FFI_RLNV3MerkleProof_ptr_Vec_uint8_t;

FFI_RLNV3_t* ffi_rln_v3_new_stateless_default(void); /* ffi_rln_v3.rs:324 */
CResult_FFI_RLNV3_ptr_Vec_uint8_t ffi_rln_v3_new_stateless(const Vec_uint8_t* zkey_data, const Vec_uint8_t* graph_data); /* ffi_rln_v3.rs:330 */
FFI_RLNV3_t* ffi_rln_v3_new_with_full_merkle_tree_default(void); /* ffi_rln_v3.rs:350 */
CResult_FFI_RLNV3_ptr_Vec_uint8_t ffi_rln_v3_new_with_full_merkle_tree(size_t tree_depth, const Vec_uint8_t* zkey_data, const Vec_uint8_t* graph_data); /* ffi_rln_v3.rs:357 */
FFI_RLNV3_t* ffi_rln_v3_new_with_optimal_merkle_tree_default(void); /* ffi_rln_v3.rs:391 */
CResult_FFI_RLNV3_ptr_Vec_uint8_t ffi_rln_v3_new_with_optimal_merkle_tree(size_t tree_depth, const Vec_uint8_t* zkey_data, const Vec_uint8_t* graph_data); /* ffi_rln_v3.rs:399 */
FFI_RLNV3_t* ffi_rln_v3_new_with_pm_tree_default(void); /* ffi_rln_v3.rs:433 */
CResult_FFI_RLNV3_ptr_Vec_uint8_t ffi_rln_v3_new_with_pm_tree(size_t tree_depth, const Vec_uint8_t* zkey_data, const Vec_uint8_t* graph_data, const char* config_path); /* ffi_rln_v3.rs:440 */
void ffi_rln_v3_free(FFI_RLNV3_t* rln); /* ffi_rln_v3.rs:606 */
CResult_FFI_RLNV3Proof_ptr_Vec_uint8_t ffi_rln_v3_generate_proof(FFI_RLNV3_t* const* rln, FFI_RLNV3WitnessInput_t* const* witness); /* ffi_rln_v3.rs:507 */
CResult_FFI_RLNV3Proof_ptr_Vec_uint8_t ffi_rln_v3_generate_proof_with_rs(FFI_RLNV3_t* const* rln, FFI_RLNV3WitnessInput_t* const* witness, const CFr_t* r, const CFr_t* s); /* EXT */
CBoolResult_t ffi_rln_v3_verify(FFI_RLNV3_t* const* rln, FFI_RLNV3Proof_t* const* proof, const CFr_t* x); /* ffi_rln_v3.rs:524 */
CBoolResult_t ffi_rln_v3_verify_with_roots(FFI_RLNV3_t* const* rln, FFI_RLNV3Proof_t* const* proof, const Vec_CFr_t* roots, const CFr_t* x); /* ffi_rln_v3.rs:548 */
CResult_FFI_RLNV3PartialProof_ptr_Vec_uint8_t ffi_rln_v3_generate_partial_proof( FFI_RLNV3_t* const* rln, FFI_RLNV3PartialWitnessInput_t* const* partial_witness); /* ffi_rln_v3.rs:571 */
CResult_FFI_RLNV3Proof_ptr_Vec_uint8_t ffi_rln_v3_finish_proof(FFI_RLNV3_t* const* rln, FFI_RLNV3PartialProof_t* const* partial, FFI_RLNV3WitnessInput_t* const* witness); /* ffi_rln_v3.rs:588 */
CResult_FFI_RLNV3WitnessInput_ptr_Vec_uint8_t ffi_rln_v3_witness_input_new_single( const CFr_t* identity_secret, const CFr_t* user_message_limit, const CFr_t* message_id, const Vec_CFr_t* path_elements, const Vec_uint8_t* identity_path_index, const CFr_t* x, const CFr_t* external_nullifier); /* ffi_rln_v3.rs:617 */
CResult_FFI_RLNV3WitnessInput_ptr_Vec_uint8_t ffi_rln_v3_witness_input_new_multi( const CFr_t* identity_secret, const CFr_t* user_message_limit, const Vec_CFr_t* message_ids, const Vec_CFr_t* path_elements, const Vec_uint8_t* identity_path_index, const CFr_t* x, const CFr_t* external_nullifier, const Vec_bool_t* selector_used); /* ffi_rln_v3.rs:652 */
CFr_t* ffi_rln_v3_witness_input_get_identity_secret(FFI_RLNV3WitnessInput_t* const* w); /* ffi_rln_v3.rs:691 */
CFr_t* ffi_rln_v3_witness_input_get_user_message_limit(FFI_RLNV3WitnessInput_t* const* w); /* ffi_rln_v3.rs:698 */
CResult_CFr_ptr_Vec_uint8_t ffi_rln_v3_witness_input_get_message_id(FFI_RLNV3WitnessInput_t* const* w); /* ffi_rln_v3.rs:705 */
CResult_Vec_CFr_Vec_uint8_t ffi_rln_v3_witness_input_get_message_ids(FFI_RLNV3WitnessInput_t* const* w); /* ffi_rln_v3.rs:721 */
Vec_CFr_t ffi_rln_v3_witness_input_get_path_elements(FFI_RLNV3WitnessInput_t* const* w); /* ffi_rln_v3.rs:742 */
Vec_uint8_t ffi_rln_v3_witness_input_get_identity_path_index(FFI_RLNV3WitnessInput_t* const* w); /* ffi_rln_v3.rs:755 */
CFr_t* ffi_rln_v3_witness_input_get_x(FFI_RLNV3WitnessInput_t* const* w); /* ffi_rln_v3.rs:762 */
CFr_t* ffi_rln_v3_witness_input_get_external_nullifier(FFI_RLNV3WitnessInput_t* const* w); /* ffi_rln_v3.rs:769 */
CResult_Vec_bool_Vec_uint8_t ffi_rln_v3_witness_input_get_selector_used(FFI_RLNV3WitnessInput_t* const* w); /* ffi_rln_v3.rs:776 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_witness_to_bytes_le(FFI_RLNV3WitnessInput_t* const* w); /* ffi_rln_v3.rs:792 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_witness_to_bytes_be(FFI_RLNV3WitnessInput_t* const* w); /* ffi_rln_v3.rs:809 */
CResult_FFI_RLNV3WitnessInput_ptr_Vec_uint8_t ffi_bytes_le_to_rln_v3_witness(const Vec_uint8_t* bytes); /* ffi_rln_v3.rs:826 */
CResult_FFI_RLNV3WitnessInput_ptr_Vec_uint8_t ffi_bytes_be_to_rln_v3_witness(const Vec_uint8_t* bytes); /* ffi_rln_v3.rs:842 */
void ffi_rln_v3_witness_input_free(FFI_RLNV3WitnessInput_t* w); /* ffi_rln_v3.rs:858 */
CResult_FFI_RLNV3PartialWitnessInput_ptr_Vec_uint8_t ffi_rln_v3_partial_witness_input_new( const CFr_t* identity_secret, const CFr_t* user_message_limit, const Vec_CFr_t* path_elements, const Vec_uint8_t* identity_path_index); /* ffi_rln_v3.rs:869 */
CFr_t* ffi_rln_v3_partial_witness_input_get_identity_secret(FFI_RLNV3PartialWitnessInput_t* const* w); /* ffi_rln_v3.rs:897 */
CFr_t* ffi_rln_v3_partial_witness_input_get_user_message_limit(FFI_RLNV3PartialWitnessInput_t* const* w); /* ffi_rln_v3.rs:904 */
Vec_CFr_t ffi_rln_v3_partial_witness_input_get_path_elements(FFI_RLNV3PartialWitnessInput_t* const* w); /* ffi_rln_v3.rs:911 */
Vec_uint8_t ffi_rln_v3_partial_witness_input_get_identity_path_index(FFI_RLNV3PartialWitnessInput_t* const* w); /* ffi_rln_v3.rs:924 */
FFI_RLNV3PartialWitnessInput_t* ffi_rln_v3_witness_to_partial_witness(FFI_RLNV3WitnessInput_t* const* w); /* ffi_rln_v3.rs:931 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_partial_witness_to_bytes_le(FFI_RLNV3PartialWitnessInput_t* const* w); /* ffi_rln_v3.rs:939 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_partial_witness_to_bytes_be(FFI_RLNV3PartialWitnessInput_t* const* w); /* ffi_rln_v3.rs:956 */
CResult_FFI_RLNV3PartialWitnessInput_ptr_Vec_uint8_t ffi_bytes_le_to_rln_v3_partial_witness(const Vec_uint8_t* bytes); /* ffi_rln_v3.rs:973 */
CResult_FFI_RLNV3PartialWitnessInput_ptr_Vec_uint8_t ffi_bytes_be_to_rln_v3_partial_witness(const Vec_uint8_t* bytes); /* ffi_rln_v3.rs:989 */
void ffi_rln_v3_partial_witness_input_free(FFI_RLNV3PartialWitnessInput_t* w); /* ffi_rln_v3.rs:1005 */
FFI_RLNV3ProofValues_t* ffi_rln_v3_proof_get_values(FFI_RLNV3Proof_t* const* proof); /* ffi_rln_v3.rs:1016 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_proof_to_bytes_le(FFI_RLNV3Proof_t* const* proof); /* ffi_rln_v3.rs:1023 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_proof_to_bytes_mixed(FFI_RLNV3Proof_t* const* proof); /* ffi_rln_v3.rs:1040 */
CResult_FFI_RLNV3Proof_ptr_Vec_uint8_t ffi_bytes_le_to_rln_v3_proof(const Vec_uint8_t* bytes); /* ffi_rln_v3.rs:1057 */
CResult_FFI_RLNV3Proof_ptr_Vec_uint8_t ffi_bytes_mixed_to_rln_v3_proof(const Vec_uint8_t* bytes); /* ffi_rln_v3.rs:1073 */
void ffi_rln_v3_proof_free(FFI_RLNV3Proof_t* proof); /* ffi_rln_v3.rs:1089 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_partial_proof_to_bytes_le(FFI_RLNV3PartialProof_t* const* partial); /* ffi_rln_v3.rs:1100 */
CResult_FFI_RLNV3PartialProof_ptr_Vec_uint8_t ffi_bytes_le_to_rln_v3_partial_proof(const Vec_uint8_t* bytes); /* ffi_rln_v3.rs:1117 */
void ffi_rln_v3_partial_proof_free(FFI_RLNV3PartialProof_t* partial); /* ffi_rln_v3.rs:1133 */
CFr_t* ffi_rln_v3_proof_values_get_root(FFI_RLNV3ProofValues_t* const* pv); /* ffi_rln_v3.rs:1144 */
CFr_t* ffi_rln_v3_proof_values_get_x(FFI_RLNV3ProofValues_t* const* pv); /* ffi_rln_v3.rs:1151 */
CFr_t* ffi_rln_v3_proof_values_get_external_nullifier(FFI_RLNV3ProofValues_t* const* pv); /* ffi_rln_v3.rs:1156 */
CResult_CFr_ptr_Vec_uint8_t ffi_rln_v3_proof_values_get_y(FFI_RLNV3ProofValues_t* const* pv); /* ffi_rln_v3.rs:1163 */
CResult_CFr_ptr_Vec_uint8_t ffi_rln_v3_proof_values_get_nullifier(FFI_RLNV3ProofValues_t* const* pv); /* ffi_rln_v3.rs:1179 */
CResult_Vec_bool_Vec_uint8_t ffi_rln_v3_proof_values_get_selector_used(FFI_RLNV3ProofValues_t* const* pv); /* ffi_rln_v3.rs:1195 */
CResult_Vec_CFr_Vec_uint8_t ffi_rln_v3_proof_values_get_ys(FFI_RLNV3ProofValues_t* const* pv); /* ffi_rln_v3.rs:1211 */
CResult_Vec_CFr_Vec_uint8_t ffi_rln_v3_proof_values_get_nullifiers(FFI_RLNV3ProofValues_t* const* pv); /* ffi_rln_v3.rs:1232 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_proof_values_to_bytes_le(FFI_RLNV3ProofValues_t* const* pv); /* ffi_rln_v3.rs:1253 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_proof_values_to_bytes_be(FFI_RLNV3ProofValues_t* const* pv); /* ffi_rln_v3.rs:1270 */
CResult_FFI_RLNV3ProofValues_ptr_Vec_uint8_t ffi_bytes_le_to_rln_v3_proof_values(const Vec_uint8_t* bytes); /* ffi_rln_v3.rs:1287 */
CResult_FFI_RLNV3ProofValues_ptr_Vec_uint8_t ffi_bytes_be_to_rln_v3_proof_values(const Vec_uint8_t* bytes); /* ffi_rln_v3.rs:1303 */
void ffi_rln_v3_proof_values_free(FFI_RLNV3ProofValues_t* pv); /* ffi_rln_v3.rs:1319 */
CResult_CFr_ptr_Vec_uint8_t ffi_rln_v3_compute_id_secret(const CFr_t* share1_x, const CFr_t* share1_y, const CFr_t* share2_x, const CFr_t* share2_y); /* ffi_rln_v3.rs:1324 */
CResult_CFr_ptr_Vec_uint8_t ffi_rln_v3_recover_id_secret(FFI_RLNV3ProofValues_t* const* pv1, FFI_RLNV3ProofValues_t* const* pv2); /* ffi_rln_v3.rs:1345 */
CBoolResult_t ffi_rln_v3_relay_step(FFI_RLNV3_t* const* rln, struct rlnamd_nullifier_log* log, FFI_RLNV3Proof_t* const* proofs, size_t n, const Vec_uint8_t* signals, const Vec_CFr_t* roots, const uint64_t* tags, uint8_t* verdict, uint8_t* status, CFr_t* secrets, uint64_t* first_tag); /* EXT: ffi_relay_step over V3 proofs */
CBoolResult_t ffi_rln_v3_relay_set_epochs(FFI_RLNV3_t* const* rln, struct rlnamd_nullifier_log* log, const CFr_t* external_nullifiers, size_t k, size_t* removed); /* EXT: ffi_relay_set_epochs for a V3 object */
CBoolResult_t ffi_rln_v3_nullifier_log_observe(struct rlnamd_nullifier_log* log, FFI_RLNV3ProofValues_t* const* values, size_t n, const bool* take, const uint64_t* tags, uint8_t* status, CFr_t* secrets, uint64_t* first_tag); /* EXT: ffi_nullifier_log_observe over V3 values */
void ffi_rln_v3_merkle_proof_free(FFI_RLNV3MerkleProof_t* proof); /* ffi_rln_v3.rs:1371 */
CBoolResult_t ffi_rln_v3_delete_leaf(FFI_RLNV3_t** rln, size_t index); /* ffi_rln_v3.rs:1376 */
CBoolResult_t ffi_rln_v3_set_leaf(FFI_RLNV3_t** rln, size_t index, const CFr_t* leaf); /* ffi_rln_v3.rs:1390 */
CResult_CFr_ptr_Vec_uint8_t ffi_rln_v3_get_leaf(FFI_RLNV3_t* const* rln, size_t index); /* ffi_rln_v3.rs:1408 */
size_t ffi_rln_v3_leaves_set(FFI_RLNV3_t* const* rln); /* ffi_rln_v3.rs:1425 */
CBoolResult_t ffi_rln_v3_set_next_leaf(FFI_RLNV3_t** rln, const CFr_t* leaf); /* ffi_rln_v3.rs:1430 */
CBoolResult_t ffi_rln_v3_set_leaves_from(FFI_RLNV3_t** rln, size_t index, const Vec_CFr_t* leaves); /* ffi_rln_v3.rs:1444 */
CBoolResult_t ffi_rln_v3_init_tree_with_leaves(FFI_RLNV3_t** rln, const Vec_CFr_t* leaves); /* ffi_rln_v3.rs:1463 */
CBoolResult_t ffi_rln_v3_atomic_operation(FFI_RLNV3_t** rln, size_t index, const Vec_CFr_t* leaves, const Vec_size_t* indices); /* ffi_rln_v3.rs:1481 */
CBoolResult_t ffi_rln_v3_seq_atomic_operation(FFI_RLNV3_t** rln, const Vec_CFr_t* leaves, const Vec_uint8_t* indices); /* ffi_rln_v3.rs:1502 */
CFr_t* ffi_rln_v3_get_root(FFI_RLNV3_t* const* rln); /* ffi_rln_v3.rs:1531 */
CResult_FFI_RLNV3MerkleProof_ptr_Vec_uint8_t ffi_rln_v3_get_merkle_proof(FFI_RLNV3_t* const* rln, size_t index); /* ffi_rln_v3.rs:1537 */
CBoolResult_t ffi_rln_v3_set_metadata(FFI_RLNV3_t** rln, const Vec_uint8_t* metadata); /* ffi_rln_v3.rs:1565 */
CResult_Vec_uint8_Vec_uint8_t ffi_rln_v3_get_metadata(FFI_RLNV3_t* const* rln); /* ffi_rln_v3.rs:1582 */
CBoolResult_t ffi_rln_v3_flush(FFI_RLNV3_t** rln); /* ffi_rln_v3.rs:1598 */

#ifdef __cplusplus
}
#endif
#endif /* RLN_H */
