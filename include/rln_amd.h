/* rln_amd.h -- batch / device-resident extension entry points of the MI355X RLN backend.
 *
 * The zerokit-compatible drop-in surface is include/rln.h (same symbols and struct layouts as the header
 * safer-ffi generates from /root/reference/rln/src/ffi/).  The reference has NO batch, no deterministic
 * (r, s) and no device-resident API (SURVEY.md §8b "Threading" / "Determinism gap"); the functions below
 * add exactly those, with plain pointers and sizes only.  All field elements cross this boundary as
 * 32-byte little-endian canonical integers (the form `fr_to_bytes_le` produces,
 * /root/reference/rln/src/utils.rs:75-120).
 *
 * Every function returns 0 on success and a non-zero code on failure; the message is available from
 * rlnamd_last_error() (thread-local).  There is no CPU fallback: without a HIP device every compute
 * entry fails with RLNAMD_ERR_NO_DEVICE.
 */
#ifndef RLN_AMD_H
#define RLN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RLNAMD_OK 0
#define RLNAMD_ERR 1
#define RLNAMD_ERR_NO_DEVICE 2

#define RLNAMD_PROVER_STAGES 8

const char* rlnamd_last_error(void);
int rlnamd_device_count(void);
int rlnamd_set_device(int ordinal);
int rlnamd_get_device(int* ordinal);   /* the calling thread's current device */
int rlnamd_device_name(char* buf, size_t cap);

/* ---- hashing ----------------------------------------------------------------------------------------
 * Batched Poseidon: poseidon_hash / poseidon_hash_pair (rln/src/hashers.rs:32-54) over n independent
 * inputs.  inputs: n * arity * 32 bytes, out: n * 32 bytes (host memory). arity 1..8 (t = 2..9). */
int rlnamd_poseidon_hash(const uint8_t* inputs_le, size_t n, size_t arity, uint8_t* out_le);
/* hash_to_field_le / _be (rln/src/hashers.rs:73-93): Keccak-256 then reduction mod r.  Host only; many messages at
 * once, on the device: rlnamd_hasher_* below. */
int rlnamd_hash_to_field_le(const uint8_t* data, size_t len, uint8_t out_le[32]);
int rlnamd_hash_to_field_be(const uint8_t* data, size_t len, uint8_t out_le[32]);

/* ---- HBM-resident Poseidon Merkle tree ---------------------------------------------------------------
 * FullMerkleTree semantics (utils/src/merkle_tree/full_merkle_tree.rs).  Calls on one handle are serialised by the
 * handle's own mutex (one stream and shared staging buffers per tree: readers touch object state too), so a handle may
 * be shared between threads; different handles do not wait for each other. */
typedef struct rlnamd_tree rlnamd_tree;
int rlnamd_tree_new(size_t depth, rlnamd_tree** out);                         /* ::default(depth) :74-80 */
void rlnamd_tree_free(rlnamd_tree* t);
int rlnamd_tree_set_range(rlnamd_tree* t, size_t start, const uint8_t* leaves_le, size_t n); /* :197-223 */
/* k single-leaf writes (any order; a later entry for the same index wins) followed by ONE bottom-up pass over the union
 * of their paths -- what k set() calls (:141-147, depth hashes each) leave behind, in one pass */
int rlnamd_tree_set_leaves(rlnamd_tree* t, const uint64_t* indices, const uint8_t* leaves_le, size_t k);
int rlnamd_tree_root(rlnamd_tree* t, uint8_t out_le[32]);                                    /* :137-139 */
int rlnamd_tree_get_leaf(rlnamd_tree* t, size_t index, uint8_t out_le[32]);                  /* :149-154 */
/* one proof: elems = depth*32 bytes bottom-up, bits = depth bytes (1 = node is a right child) :288-304 */
int rlnamd_tree_proof(rlnamd_tree* t, size_t index, uint8_t* elems_le, uint8_t* bits);
/* `count` proofs for leaves [first, first+count) copied back to host buffers */
int rlnamd_tree_proofs(rlnamd_tree* t, size_t first, size_t count, uint8_t* elems_le, uint8_t* bits);
/* the batch form of rlnamd_tree_proof for k leaves in any order (repeats allowed): one launch and one wait for all of
 * them; elems_le = k*depth*32 bytes, bits = k*depth bytes, proof i at index i.  An index >= 2^depth fails the call before
 * anything is enqueued; k = 0 succeeds and writes nothing. */
int rlnamd_tree_proofs_at(rlnamd_tree* t, const uint64_t* indices, size_t k, uint8_t* elems_le, uint8_t* bits);
/* Device-resident workload of BASELINE config 3: leaves first_value + i generated in HBM, full rebuild,
 * all `count` proofs emitted into an internal HBM buffer and (if verify != 0) every proof recomputed to
 * the root on the device.  ms[0] = build, ms[1] = proof emission (HIP events); bad = failed proofs. */
int rlnamd_tree_fill_sequential(rlnamd_tree* t, size_t start, size_t n, uint64_t first_value);
int rlnamd_tree_bench(rlnamd_tree* t, size_t n_leaves, uint64_t first_value, int verify, float ms[2], size_t* bad);

/* ---- nullifier log on the device: find double signalling in batches --------------------------------------
 * The step of a relay loop behind verification: the log keeps every share (nullifier | x | y | external_nullifier, four
 * canonical little-endian Fr, 128 bytes) seen in the epochs of a relay's window, in HBM, and says of each new one whether its nullifier is new,
 * a repeat of the same message, or a second message of one member -- and then returns the member's identity secret
 * (compute_id_secret / recover_id_secret, protocol/slashing.rs:12-100).  Every observed share gets a record, repeats
 * included; a record's sequence number is its arrival index since the last clear, and `tags` are the caller's own names
 * for the messages (tags == NULL: the sequence numbers).
 *   NEW        the first record with this nullifier is the share itself
 *   FOREIGN    the first record has another external nullifier (recover_id_secret's ExternalNullifierMismatch)
 *   DUPLICATE  the first record has the same x: the same message again (compute_id_secret's DivisionByZero)
 *   SPAM       otherwise: secrets_le[i] is a0 of the line through the two shares; it is all zero for every other status
 * first_tag[i] is the tag of the first record with the share's nullifier (for NEW the share's own).  The meaning of a
 * call is that of observing its shares one by one in index order: a call of n shares gives what any split of it into
 * consecutive smaller calls gives.  observe refuses, each with its own text, before anything is enqueued and with the log
 * left exactly as it was: a null pointer with n > 0, n larger than the room left (capacity counts shares observed), a
 * field element >= r (the text names the first such share).  n = 0 succeeds and writes nothing.  The buffers that carried
 * a call's results back, recovered secrets among them, are overwritten on the device and in pinned memory before observe
 * returns.  Calls on one handle are
 * serialised by the handle's own mutex; different handles do not wait for each other.  The log lives on the device that
 * is current when it is made.
 * info: [0] capacity, [1] shares recorded, [2] table slots, [3] distinct nullifiers (shares judged NEW since the last
 * clear), [4] observe calls, [5] longest probe walk so far, [6] non-zero 16-byte words in those result buffers,
 * device and pinned (0 expected), [7] the seed in use.  [4] and [5] run over the life of the handle.
 *
 * Retiring.  One log serves a whole window of epochs: nullifiers of different epochs do not collide, and
 * retire(E), E a set of 1 .. RLNAMD_LOG_RETIRE_MAX external nullifiers, removes every record whose external nullifier
 * is in E when those epochs leave the window.  The survivors keep their arrival order, their tags and their sequence
 * numbers.  Afterwards every observe returns the statuses, secrets and first tags that a fresh log with the same seed
 * would return, had it been fed only the surviving shares with their stored tags in their original order; what differs
 * from that fresh log is default tags and the counters that run over the life of the handle.  "The first record with
 * this nullifier" becomes the first surviving one: a nullifier seen under two external nullifiers survives under the
 * one that was not retired, and that record is then the first.  capacity counts records held: after a retire info[1]
 * is the number of survivors, info[3] the number of distinct nullifiers among them, and observe has capacity - info[1]
 * rows of room.  A sequence number is never reused before the next clear: with tags == NULL a share's tag stays its
 * sequence number, the counter behind it is not lowered by a retire, and clear resets it.  rlnamd_nullifier_log_get
 * takes the sequence number; one that was retired is an error whose text says so, one never issued is the error it was.
 * A log that never retires behaves exactly as before.  retire refuses, each with its own text, before anything is
 * enqueued and with the log unchanged: a null pointer with k > 0, k > RLNAMD_LOG_RETIRE_MAX, an external nullifier >= r
 * (the text names the first such one).  A duplicate in E is not an error.  k = 0, or a set no record matches: removed =
 * 0 and nothing moves.  Retiring everything leaves what clear leaves, except that the default-tag counter is not reset.
 * A failed allocation during a retire leaves the log as it was.  From a log's first retire on its record memory doubles
 * (the survivors are moved into a spare set of record arrays, which then becomes the live one); a log that never
 * retires pays nothing.
 *
 * Retaining.  retain(W), W a set of 1 .. RLNAMD_LOG_RETIRE_MAX external nullifiers, removes every record whose external
 * nullifier is NOT in W, however many different ones the removed records carry: what a relay needs when its window
 * moves, and after a gap or a restart of its clock, when it can name the epochs it follows and not the strangers.
 * Everything else is retire's contract, word for word: the survivors keep their order, their tags and their sequence
 * numbers; afterwards every observe answers as a fresh log with the same seed would, had it been fed only the
 * survivors; sequence numbers are not reused; the spare record arrays appear with the first removal; a failed
 * allocation leaves the log as it was; retire_info [0] and [1] count a retain as a retire.  The two calls run the same
 * passes and differ in the sense of the mark alone.  retain refuses, each with its own text, before anything is
 * enqueued and with the log unchanged: a null pointer with k > 0; k == 0 (it would remove everything: use clear);
 * k > RLNAMD_LOG_RETIRE_MAX; an external nullifier >= r (the text names the first such one).  These are judged before
 * the handle is followed.  A duplicate in W is not an error.  A set every record matches: removed = 0, nothing moves.
 * retire_info: [0] retire and retain calls, [1] records removed over the life of the handle, [2] next default tag, [3] records
 * held, [4] longest probe walk of the last rebuild, [5] 1 once the spare arrays exist, [6..7] reserved 0. */
typedef struct rlnamd_nullifier_log rlnamd_nullifier_log;
#define RLNAMD_SHARE_NEW 0
#define RLNAMD_SHARE_DUPLICATE 1
#define RLNAMD_SHARE_SPAM 2
#define RLNAMD_SHARE_FOREIGN 3
#define RLNAMD_SHARE_SKIPPED 4   /* never from observe: rln.h's ffi_nullifier_log_observe (take[i] was false), rlnamd_relay_step */
int rlnamd_nullifier_log_new(size_t capacity, uint64_t seed, rlnamd_nullifier_log** out);  /* 1 <= capacity <= 2^31; seed 0 = random */
void rlnamd_nullifier_log_free(rlnamd_nullifier_log* l);
int rlnamd_nullifier_log_observe(rlnamd_nullifier_log* l, size_t n, const uint8_t* shares_le /* n*128 */,
                                 const uint64_t* tags /* NULL: the sequence numbers */, uint8_t* status /* n */,
                                 uint8_t* secrets_le /* n*32 or NULL */, uint64_t* first_tag /* n or NULL */);
int rlnamd_nullifier_log_clear(rlnamd_nullifier_log* l);      /* everything goes: empty table, count 0, same seed */
#define RLNAMD_LOG_RETIRE_MAX 64
int rlnamd_nullifier_log_retire(rlnamd_nullifier_log* l, const uint8_t* external_nullifiers_le /* k*32 */, size_t k,
                                uint64_t* removed /* or NULL */);
int rlnamd_nullifier_log_retain(rlnamd_nullifier_log* l, const uint8_t* external_nullifiers_le /* k*32 */, size_t k,
                                uint64_t* removed /* or NULL */);
int rlnamd_nullifier_log_retire_info(rlnamd_nullifier_log* l, uint64_t out[8]);
int rlnamd_nullifier_log_get(rlnamd_nullifier_log* l, uint64_t seq, uint8_t share_le[128], uint64_t* tag);
int rlnamd_nullifier_log_home_slot(rlnamd_nullifier_log* l, const uint8_t nullifier_le[32], uint64_t* slot); /* host only */
int rlnamd_nullifier_log_info(rlnamd_nullifier_log* l, uint64_t out[8]);

/* ---- signals to field elements on the device, in batches ------------------------------------------------------
 * The step of a relay loop in front of verification: x = hash_to_field(signal) (rln/src/hashers.rs:73-93: Keccak-256,
 * read little-endian, mod r) of n messages in one call, a lane per message.  Message i is data[offsets[i],
 * offsets[i + 1]); out_le row i is its field element, 32 canonical little-endian bytes -- what rlnamd_hash_to_field_le
 * (and _be) gives for it.  Messages are dealt to lanes by descending length.  A message larger than one half of the
 * staging is hashed on the calling thread while the device works, and so are the longest of the messages of more than
 * lane_max_blocks 136-byte blocks, for as long as the host is done with them before a lane would be (a lone long
 * message, a few among many short ones).  A call larger than the staging (stage_bytes: two pinned halves) goes through
 * it in chunks.  hash_to_field refuses, each
 * with its own text and before anything is enqueued: null pointers with n > 0, decreasing offsets, offsets[n] >
 * data_len, sizes that overflow (n >= 2^32).  n = 0 succeeds and writes nothing.  Signals are public: nothing is wiped.
 * Calls on one handle are serialised by the handle's own mutex; the hasher lives on the device that is current when
 * it is made.
 * info, of the last call: [0] messages hashed on the device, [1] on the host, [2] chunks, [3] blocks on the device,
 * [4] the longest lane in blocks; of the handle: [5] blocks per staging half, [6] lane_max_blocks, [7] calls so far. */
typedef struct rlnamd_hasher rlnamd_hasher;
int rlnamd_hasher_new(size_t stage_bytes /* 0: default */, size_t lane_max_blocks /* 0: default */, rlnamd_hasher** out);
void rlnamd_hasher_free(rlnamd_hasher* h);
int rlnamd_hasher_hash_to_field(rlnamd_hasher* h, const uint8_t* data, size_t data_len,
                                const uint64_t* offsets /* n + 1 */, size_t n, uint8_t* out_le /* n * 32 */);
int rlnamd_hasher_info(rlnamd_hasher* h, uint64_t out[8]);

/* ---- batched Groth16 prover --------------------------------------------------------------------------
 * Replaces generate_zk_proof_with_rs (rln/src/protocol/proof.rs:753-777) + proof_values_from_witness
 * (protocol/witness.rs:759-804) for n independent proofs at once. */
typedef struct rlnamd_prover rlnamd_prover;
/* zkey/graph: the bytes of rln_final.arkzkey and graph.bin (circuit/mod.rs:140-203).
 * max_batch: workspace capacity; window_bits: 0 = default / RLNAMD_WINDOW_BITS, else g1 + 10000 * g2 with each
 * spec = c + 100 * wide (c-bit windows, the first `wide` one bit wider; g2 = 0: same as g1). */
int rlnamd_prover_new(const uint8_t* zkey, size_t zkey_len, const uint8_t* graph, size_t graph_len,
                      size_t max_batch, int window_bits, rlnamd_prover** out);
void rlnamd_prover_free(rlnamd_prover* p);
typedef struct {
  uint64_t inputs_size;      /* slots of the witness-graph inputs buffer (slot 0 = 1) */
  uint64_t num_signals;      /* witness length */
  uint64_t domain_size;      /* NTT domain */
  uint64_t tree_depth, max_out;
  uint64_t capacity;         /* max batch */
  uint64_t table_bytes;      /* HBM held by the fixed-base tables */
  int32_t window_bits, windows;       /* G1 comb: narrow window width; table additions per G1 point and proof */
  int32_t window_bits_g2, windows_g2; /* the same for the G2 comb */
  int32_t glv;                        /* always 1: scalars are split k1 + lambda k2 and the combs cover 127 bits */
  int32_t reserved;
  uint64_t g1_rows, g2_rows;          /* rows a big batch walks per full proof: G2 the table rows (finite points); G1 the table
                                         rows minus the B1 rows that share their point with the A row of the same wire and are
                                         not walked (RLNAMD_SHARED_ROWS=0: every table row) */
} rlnamd_prover_info;
int rlnamd_prover_get_info(rlnamd_prover* p, rlnamd_prover_info* info);
/* the same for the prover behind an object of include/rln.h (FFI_RLN_t* / FFI_RLNV3_t*, passed as void*): shows how
 * the "window_bits" / "max_batch" keys of the config_path JSON (or RLNAMD_WINDOW_BITS / RLNAMD_MAX_BATCH) sized it */
int rlnamd_ffi_prover_info(const void* ffi_rln, rlnamd_prover_info* info);
/* The member memo of an object whose config_path JSON carries "auto_partial": N (0 = off, the default).  With it,
 * ffi_generate_rln_proof remembers the partial proof of up to N members (identity secret, limit, Merkle path): the first
 * proof of a member at a root is made from scratch and its partial proof follows on the device behind the call; later
 * proofs of that member at that root are finishes of it (rlnamd_prover_submit_finish: 0.8 instead of 2.1 ms), the same
 * proof for the same (r, s).  Opt-in because of what it keeps: the member's witness values on the device and the key
 * (identity secret included) in host memory until the entry is evicted, or the object freed.
 * out: [0] members remembered, [1] proofs that were finishes, [2] proofs from scratch, [3] 1 while a partial proof is pending */
int rlnamd_ffi_memo_stats(const void* ffi_rln, uint64_t out[4]);
/* The device verifier behind an FFI object (ffi_verify_rln_proofs_batch, ffi_verify_rln_signals_batch; config keys
 * "verify_gpu_min", "verify_lanes", "verify_optimistic", "verify_optimistic_teams", "verify_optimistic_cooldown"): out[0..7] as
 * rlnamd_verify_gpu_optimistic_stats, out[8] chunks run exactly with a lane per proof, out[9] in team form. */
int rlnamd_ffi_verify_stats(const void* ffi_rln, uint64_t out[10]);
/* The durable store of a persistent tree (config_path: "temporary": false + "path"): the directory `path`
 * holds a checksummed snapshot and a write-ahead journal, every mutating tree call appends ONE record before it is applied,
 * ffi_flush is an fdatasync of the journal and a flusher thread does the same every "flush_every_ms".
 * out: [0] snapshot generation, [1] journal bytes (header included), [2] records since the snapshot, [3] syncs so far,
 * [4] compactions so far, [5] records replayed at open, [6] torn bytes discarded at open, [7] appended bytes not yet
 * synced.  A temporary tree returns all zero. */
int rlnamd_ffi_tree_store_info(const void* ffi_rln, uint64_t out[8]);
/* Concurrent callers.  generate_rln_proof takes &self in the reference (rln/src/public.rs:624) and an RLN object may be
 * shared by threads; the prover proves one batch at a time, so the single-proof calls (ffi_generate_rln_proof,
 * ffi_rln_v3_generate_proof and their _with_rs twins) that arrive while a proof is on the device are gathered and go out
 * together, as one batch, when it returns -- each call gets its own proof or its own error text, a lone caller is a
 * batch of one as before.  "gather_calls": N in the config_path JSON (or RLNAMD_GATHER_CALLS) caps a batch (default:
 * the workspace's capacity; 0 or 1: off); on an object with "auto_partial" the gathered calls of remembered members go
 * out as one batch of finishes, the others one by one.  Threads that call in a
 * loop arrive just behind their results: the leader gives the callers it saw within the last 20 ms "gather_window_us"
 * (500; RLNAMD_GATHER_WINDOW_US; 0: none) to arrive before it takes the batch, so that T threads go out as batches of T
 * instead of two halves taking turns; a lone caller never waits, callers slower than the window make it stop waiting.
 * out: [0] batches led, [1] calls that went out in them, [2] the largest batch, [3] the cap (0: off), [4] batches whose
 * leader waited for a recent caller, [5] nanoseconds the leaders spent proving their batches; ffi_finish_rln_proof and
 * its twins (single message-id) are gathered the same way in a queue of their own: [6] its batches, [7] its calls */
int rlnamd_ffi_gather_stats(const void* ffi_rln, uint64_t out[8]);
/* offset/len of a named input signal in the inputs buffer (iden3calc.rs:122-146); returns RLNAMD_ERR if absent */
int rlnamd_prover_input_slot(rlnamd_prover* p, const char* name, uint32_t* offset, uint32_t* len);
/* inputs: n * inputs_size * 32 bytes (slot 0 must hold 1); rs: n * 64 bytes (r then s). */
int rlnamd_prover_upload(rlnamd_prover* p, size_t n, const uint8_t* inputs_le, const uint8_t* rs_le);
int rlnamd_prover_run(rlnamd_prover* p, size_t n);      /* inputs already resident; blocks until done */
/* Enqueue only: consecutive batches overlap on the device (front end of batch k+1 and back end of batch
 * k-1 beside the MSM of batch k); each batch ends with its proofs copied to pinned host memory.
 * rlnamd_prover_sync drains the pipeline; download refers to the last enqueued batch, stage_ms to the mean over the
 * batches still held in the workspace slots (the last <= 5 launches of the same kind). */
int rlnamd_prover_run_async(rlnamd_prover* p, size_t n);
int rlnamd_prover_sync(rlnamd_prover* p);
/* proofs: n*128 (ark-serialize compressed Proof), coords: n*256 (affine A|B|C) or NULL,
 * values: n*160 (y, root, nullifier, x, external_nullifier) or NULL, errors: n*4 or NULL */
int rlnamd_prover_download(rlnamd_prover* p, size_t n, uint8_t* proofs, uint8_t* coords, uint8_t* values,
                           uint32_t* errors);
/* ---- streamed batches: the path of SURVEY 8(d)'s timed region, "H2D of witness inputs -> D2H of proofs".  The reference
 * takes a fresh witness per call (rln/src/protocol/proof.rs:753-777, public.rs:624-631); rlnamd_prover_submit is n such
 * calls at once: it stages the inputs (n * inputs_size * 32 bytes), rs (n * 64) and, in RLNAMD_MODE_FINISH, the partial
 * points (n * 320, else NULL) in pinned memory owned by a workspace slot, copies them to that slot's own device buffers
 * on the batch's front-end stream and enqueues the batch.  It returns at once with a ticket (> 0) unless all
 * rlnamd_prover_slots() slots are in flight; consecutive submits of DIFFERENT batches overlap on the device exactly as
 * run_async's do.  rlnamd_prover_collect waits for that batch only (any output pointer may be NULL; partial320 is the
 * result of a RLNAMD_MODE_PARTIAL batch).  A ticket expires when its slot is reused, i.e. slots() submits later.
 * rlnamd_prover_prove_stream = submit / collect over any n in chunks of `capacity`, results in index order. */
int rlnamd_prover_slots(rlnamd_prover* p);
int rlnamd_prover_submit(rlnamd_prover* p, size_t n, const uint8_t* inputs_le, const uint8_t* rs_le, int mode,
                         const uint8_t* partial320, uint64_t* ticket);
int rlnamd_prover_collect(rlnamd_prover* p, uint64_t ticket, size_t n, uint8_t* proofs, uint8_t* coords, uint8_t* values,
                          uint32_t* errors, uint8_t* partial320);
/* public signals w[1..num_instance) of a finished batch (n * num_public * 32 bytes), circuit-generic.  Call it BEFORE
 * rlnamd_prover_collect: collect ends the batch -- see the next comment. */
int rlnamd_prover_collect_public(rlnamd_prover* p, uint64_t ticket, size_t n, uint8_t* out_le);
/* Secrets do not outlive the batch.  The reference zeroises the identity secret wherever it holds it (IdSecret,
 * rln/src/utils.rs:440-527) and the witness calculator's inputs (rln/src/circuit/iden3calc.rs:45-56).  Here
 * rlnamd_prover_collect (and prove_stream, the pool, every ffi_* proving call) overwrites the batch's staged inputs --
 * pinned host buffer and device copy -- its (r, s), its witness values and what was derived from them (the signed window
 * digits of both walks, a | b | c / h, the walks' partial sums: rlnamd_prover_residue) behind the copy-out; a later
 * rlnamd_prover_collect_public of that ticket is an error.  The resident-input calls (upload / run / download, kept for
 * the fetch_* parity taps) hold their data until rlnamd_prover_wipe or rlnamd_prover_free. */
int rlnamd_prover_wipe(rlnamd_prover* p);
/* the switches this prover was built with, "name=value ..." (ProverTuning, zerokit_amd/csrc/prover.h: every RLNAMD_*
 * variable the prover reads is read once, at construction, and listed there) */
int rlnamd_prover_describe(rlnamd_prover* p, char* buf, size_t cap);
/* where the constructor's wall time went, ms: [0] parsing the arkzkey / graph + the verifier's precomputation, [1] hipMalloc
 * of the comb tables, [2] building them on the device, [3] the rest (walk plans, constants, workspaces, pinned staging) */
int rlnamd_prover_init_ms(rlnamd_prover* p, float ms[4]);
int rlnamd_prover_prove_stream(rlnamd_prover* p, size_t n, const uint8_t* inputs_le, const uint8_t* rs_le,
                               uint8_t* proofs, uint8_t* values, uint32_t* errors);
/* ---- prove for members of a tree by leaf index.  rlnamd_prover_submit_members is rlnamd_prover_submit for n members of
 * `t`: inputs_le is what submit takes, but its pathElements / identityPathIndex slots are ignored -- the members' paths at
 * the tree's current root are read from the tree's nodes on the device, straight into the batch's staged inputs (the path
 * index as the field element 0 / 1).  Nothing waits on the host: the gather is ordered behind everything already enqueued
 * on the tree (every rlnamd_tree_set_* that has returned) and a later write to the tree is ordered behind the gather, so
 * all n proofs are at ONE root, the one the tree had when the call was made.  mode: RLNAMD_MODE_FULL or
 * RLNAMD_MODE_PARTIAL (a partial proof's inputs are secret, limit and path); RLNAMD_MODE_FINISH is an error.  The ticket
 * is collected, read (collect_public, collect_partial_cached) and wiped as any other; the leaf indices -- who proves is a
 * secret as the inputs are -- are staged in pinned memory, copied to the device and overwritten with the inputs (entry
 * [5] of rlnamd_prover_residue counts them).  A lone batch of at most RLNAMD_HINTS proofs, whose hints are hashed from the
 * path on the host, fetches its paths with one rlnamd_tree_proofs_at-like call instead and then takes submit's way; the
 * bytes are the same.  Errors, each before anything is enqueued: the witness graph names no pathElements /
 * identityPathIndex, the tree's depth is not the circuit's, tree and prover are on different devices, an index >= 2^depth.
 * rlnamd_prover_prove_stream_members: the chunked form over `capacity` (full proofs), the tree locked for the whole
 * call: all n proofs at one root. */
int rlnamd_prover_submit_members(rlnamd_prover* p, rlnamd_tree* t, size_t n, const uint64_t* leaf_indices,
                                 const uint8_t* inputs_le, const uint8_t* rs_le, int mode, uint64_t* ticket);
int rlnamd_prover_prove_stream_members(rlnamd_prover* p, rlnamd_tree* t, size_t n, const uint64_t* leaf_indices,
                                       const uint8_t* inputs_le, const uint8_t* rs_le, uint8_t* proofs,
                                       uint8_t* values, uint32_t* errors);
/* rlnamd_prover_prove_stream_members_public: the same call with EVERY public signal of a proof in values_public, n *
 * num_public * 32 bytes (rlnamd_prover_collect_public's rows), read before each chunk is collected.  The 160 bytes a proof
 * of the form above are the five values of the single message-id circuit and stay zero on any other: a multi-message-id
 * prover's caller uses this one (15 values a proof: ys | root | nullifiers | x | external nullifier | selectors). */
int rlnamd_prover_prove_stream_members_public(rlnamd_prover* p, rlnamd_tree* t, size_t n, const uint64_t* leaf_indices,
                                              const uint8_t* inputs_le, const uint8_t* rs_le, uint8_t* proofs,
                                              uint8_t* values_public /* n*num_public*32 */, uint32_t* errors);
int rlnamd_prover_stage_ms(rlnamd_prover* p, float ms[RLNAMD_PROVER_STAGES]);
const char* rlnamd_prover_stage_name(int i);
/* mean shader clock (MHz) under the G1 / G2 table walks since the previous call (the walks are VALU-issue bound: their
 * rate is SIMDs x clock / instructions); drains the pipeline */
int rlnamd_prover_walk_clock_mhz(rlnamd_prover* p, double mhz[2]);
/* parity taps of the last run: full witness (num_signals*32) / h (domain_size*32) of proof `index` */
int rlnamd_prover_fetch_witness(rlnamd_prover* p, size_t index, uint8_t* out_le);
int rlnamd_prover_fetch_h(rlnamd_prover* p, size_t index, uint8_t* out_le);
/* tap of the wipes: the number of 16-byte words that are not zero in the buffers of the slot the last batch used, whole
 * buffers: [0] G1 window digits, [1] G2 window digits, [2] a | b | c (the quotient's operands, then h), [3] / [4] partial
 * sums of the G1 / G2 walks and everything their reduction leaves behind (block sums, the unblinded A / B / C sums, the
 * affine points, the ladder's products and tables), [5] staged inputs + (r, s) + the leaf indices of a batch submitted
 * by member (device and pinned copy) + the witness given with rlnamd_prover_upload_witness.  All zero behind a collect
 * that wipes, and behind rlnamd_prover_wipe after a resident run. */
int rlnamd_prover_residue(rlnamd_prover* p, uint64_t out[6]);
/* the same tap for workspace slot `slot` (0 <= slot < rlnamd_prover_slots; anything else is an error), whichever batch
 * used it last, with the buffers rlnamd_prover_residue does not look at: [0] .. [5] as above for that slot, [6] the inputs
 * and (r, s) regions of the slot's pinned staging buffer, [7] the slot's pinned hints (rlnamd_prover_submit_hinted; the
 * first hint of a proof with the proof's public share gives the identity secret), [8] the witness interpreter's stored
 * values, [9] reserved, 0.  Whole buffers; the partial points staged behind (r, s) are handed out like a proof and not
 * counted.  Drains the pipeline as rlnamd_prover_residue does.  All zero behind a collect that wipes. */
int rlnamd_prover_residue_slot(rlnamd_prover* p, int slot, uint64_t out[10]);
/* ---- partial proofs (generate_partial_zk_proof / finish_zk_proof_with_rs, protocol/proof.rs:783-849;
 * Groth16Partial, partial_proof.rs:108-274).  mode: 0 full proof, 1 partial (inputs hold only identitySecret,
 * userMessageLimit, pathElements, identityPathIndex; other slots zero), 2 finish (full inputs + r, s + the
 * partial points given with rlnamd_prover_upload_partial).  A partial proof is four points per proof as
 * canonical LE affine coordinates [pi_a x,y | rho x,y | pi_b x.c0,x.c1,y.c0,y.c1 | pi_c x,y] = 320 bytes;
 * rlnamd_prover_known_mask returns, per witness signal, whether the partial witness fixes it
 * (PartialProof::mask is this vector without entry 0). */
#define RLNAMD_MODE_FULL 0
#define RLNAMD_MODE_PARTIAL 1
#define RLNAMD_MODE_FINISH 2
int rlnamd_prover_run_mode(rlnamd_prover* p, size_t n, int mode);
int rlnamd_prover_run_async_mode(rlnamd_prover* p, size_t n, int mode);
/* A few proofs per call: the witness graph as independent segments behind hints.  The depth-20 circuit is 22 Poseidon
 * hashes in a row -- nine tenths of its interpreter steps are that one dependency chain, and a dependent 256-bit product
 * costs a lone GPU wave 0.31 us against 0.02 us on a host core.  For a lone batch of at most RLNAMD_HINTS (24) proofs the
 * calling thread (and a helper thread per further proof) computes the values BETWEEN the hashes (identity commitment, rate commitment, the running hash after
 * every Merkle level, a1: depth + 2 hashes with the library's host Poseidon, ~0.3 ms), the device interprets the 24
 * segments those values separate all at once (the longest 268 steps instead of 4 813) and then compares every cut node's
 * own value with the hint its consumers were given.  Every witness value is still computed on the device; a hint that does
 * not check (not expected: test hook RLNAMD_HINT_FAULT) makes collect run the batch again over the whole graph.
 * The chain part of a member's hints (rate commitment, the running hash after every level) depends on public values only:
 * the last 64 (RLNAMD_HINT_CHAINS) are remembered under a fingerprint of (identity commitment, limit, path), so a member that proves
 * again at the same root costs the host two hashes (identity commitment, a1) instead of depth + 2.
 * out: [0] segments, [1] hints per proof, [2] steps of the longest segment, [3] steps of the whole graph, [4] batches
 * interpreted as segments, [5] of those, batches run again, [6] proofs whose chain was remembered. */
int rlnamd_prover_hint_stats(rlnamd_prover* p, uint64_t out[7]);
/* The hints may be computed ahead of the call, by any thread, one proof at a time -- a server whose request threads each
 * hash their own proof's chain while the device is busy: rlnamd_prover_hint_words() 32-bit words per proof (0: this
 * circuit has no such form), rlnamd_prover_hints_for() fills them from one proof's packed inputs (host only, no device
 * call, safe beside a running batch), rlnamd_prover_submit_hinted() is rlnamd_prover_submit (full proofs) for a batch of
 * at most 64 proofs whose hints (n x hint_words) are at hand: nothing is hashed inside the call and the batch takes the
 * segments whatever its members' chains would have cost.  The device checks every hint as always: hints that do not
 * belong to the inputs cost a run over the whole graph, never a wrong proof: the run takes the batch's own workspace
 * slot and ticket, however many other batches are pending and in whatever order they are collected.  The slot's pinned
 * copy of the hints is overwritten with the batch's inputs (a1 is a hint: see rlnamd_prover_residue_slot). */
uint32_t rlnamd_prover_hint_words(rlnamd_prover* p);
int rlnamd_prover_hints_for(rlnamd_prover* p, const uint8_t* inputs_le, uint32_t* hints);
int rlnamd_prover_submit_hinted(rlnamd_prover* p, size_t n, const uint8_t* inputs_le, const uint8_t* rs_le,
                                const uint32_t* hints, uint64_t* ticket);
/* Who else proves on this prover's device: bit 0 = another prover of this process, bit 1 = a prover of ANOTHER process
 * (every process with a prover on a device holds a read record lock on /dev/shm/rlnamd_<PCI bus id>.lock; probed at most
 * every 50 ms).  A shared device keeps the wide latency shapes off (they assume the chip is this prover's). */
int rlnamd_prover_device_shared(rlnamd_prover* p, int* who);
/* Finish without re-walking what the partial witness fixed (round 6).  finish_zk_proof_with_rs recomputes the whole
 * witness (protocol/proof.rs:822-849) although the identity commitment and the 20-level Merkle chain -- 21 488 of the
 * depth-20 circuit's 23 414 graph nodes, eleven twelfths of its multiplication depth -- came out of the partial run.
 * rlnamd_prover_collect_partial_cached = rlnamd_prover_collect of a RLNAMD_MODE_PARTIAL batch that also keeps, per
 * proof, the stored values of the KNOWN nodes in a device-resident cache entry (0.26 MB on the depth-20 circuit;
 * RLNAMD_PARTIAL_CACHE entries, 64 unless set) and returns an opaque handle per proof: 0 when the cache is full or off
 * -- such a proof finishes through the full interpreter.  rlnamd_prover_submit_finish = a RLNAMD_MODE_FINISH submit
 * with those handles: when every proof of a small batch (one the wave-per-proof interpreter takes) has a live handle,
 * the known rows are restored from the cache and only the cone evaluate_partial (iden3calc/graph.rs:274-312) leaves
 * unknown is interpreted.  Bytes are identical either way; a stale or foreign handle is treated as 0.  The PartialProof
 * wire form (partial_proof.rs:31-43) is untouched -- the handle travels beside it and means nothing to another prover.
 * An entry holds witness values, the identity secret among them: rlnamd_prover_release_partial overwrites and frees it,
 * rlnamd_prover_free overwrites what is left.  rlnamd_prover_partial_cache_info: [0] capacity, [1] entries in use,
 * [2] bytes per entry, [3] non-zero 16-byte words in the entries NOT in use (0: released entries were wiped),
 * [4] batches that took the cone, [5] nodes of the cone, [6] steps of the cone program, [7] steps of the full program. */
int rlnamd_prover_collect_partial_cached(rlnamd_prover* p, uint64_t ticket, size_t n, uint8_t* partial320, uint64_t* handles,
                                         uint32_t* errors);
int rlnamd_prover_submit_finish(rlnamd_prover* p, size_t n, const uint8_t* inputs_le, const uint8_t* rs_le,
                                const uint8_t* partial320, const uint64_t* handles, uint64_t* ticket);
int rlnamd_prover_release_partial(rlnamd_prover* p, const uint64_t* handles, size_t n);
int rlnamd_prover_partial_cache_info(rlnamd_prover* p, uint64_t out[8]);
int rlnamd_prover_upload_partial(rlnamd_prover* p, size_t n, const uint8_t* coords320);
int rlnamd_prover_download_partial(rlnamd_prover* p, size_t n, uint8_t* coords320);
int rlnamd_prover_known_mask(rlnamd_prover* p, uint8_t* out_num_signals);
/* Externally calculated witnesses (n x num_signals x 32 canonical LE) for the NEXT full run of n proofs; they
 * replace the witness-graph interpreter's output (generate_zk_proof_with_witness, protocol/proof.rs:705-732). */
int rlnamd_prover_upload_witness(rlnamd_prover* p, size_t n, const uint8_t* witness_le);
/* Public signals (the circuit outputs/inputs w[1..num_instance)) of the first n proofs of the last run, read
 * from the witness: n * num_public * 32 bytes.  Circuit-generic (multi message-id: ys, root, nullifiers, x,
 * external_nullifier, selector_used -- the verifier order of protocol/proof.rs:870-885). */
size_t rlnamd_prover_num_public(rlnamd_prover* p);
int rlnamd_prover_download_public(rlnamd_prover* p, size_t n, uint8_t* out_le);
/* generic-arity verification: n_values public inputs */
int rlnamd_verify_public(rlnamd_prover* p, const uint8_t proof[128], const uint8_t* values_le, size_t n_values, int* ok);
/* verify_zk_proof (protocol/proof.rs:856-894) on the host CPU, as in the reference.
 * values: y, root, nullifier, x, external_nullifier.  *ok = 1 valid, 0 invalid. */
int rlnamd_verify(rlnamd_prover* p, const uint8_t proof[128], const uint8_t values_le[160], int* ok);
/* n independent verifications on `threads` host threads (0 = one per hardware thread): proofs n * 128 bytes, values
 * n * n_values * 32 bytes, ok[i] = 1 valid, 0 invalid or malformed.  EXT: the reference verifies one proof per call
 * (protocol/proof.rs:856-894); a relay node verifies every message it forwards. */
int rlnamd_verify_many(rlnamd_prover* p, size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t n_values,
                       int threads, uint8_t* ok);
/* EXT: n independent verifications on the device.  Same inputs and the same verdicts as rlnamd_verify_many.  The
 * verifier has its own stream and buffers and never waits for a proving batch; calls from several threads serialise.
 * n = 0 succeeds and writes nothing.  The verifier chooses the shape by n: a team of 8 lanes per proof (verify_team.hip)
 * for calls that a lane per proof (verify.hip) cannot spread over the chip -- see rlnamd_verify_many_gpu_ex. */
int rlnamd_verify_many_gpu(rlnamd_prover* p, size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t n_values,
                           uint8_t* ok);
/* test / diagnosis: the final-exponentiated pairing product of each proof, 12 x 32 bytes canonical LE in
 * pairing.h's coefficient order (1 = accept); rows of proofs rejected before the pairing are all zero. */
int rlnamd_verify_many_gpu_gt(rlnamd_prover* p, size_t n, const uint8_t* proofs, const uint8_t* values_le,
                              size_t n_values, uint8_t* gt384);
/* The same with the shape named: lanes = 1 a lane per proof (chunks of 65 536), 8 a team of 8 lanes per proof (chunks
 * of 8 192; a verification's serial chain is about a third as long), 0 the verifier chooses -- teams for calls of at
 * most verify_team_max proofs (1 024), unless RLNAMD_VERIFY_LANES = 1 | 8 was set when the prover was built.  Any
 * other value of lanes is an error.  Both shapes give the same bytes.  ok (n bytes) and gt384 (n x 384 bytes) may
 * each be null. */
int rlnamd_verify_many_gpu_ex(rlnamd_prover* p, size_t n, const uint8_t* proofs, const uint8_t* values_le,
                              size_t n_values, int lanes, uint8_t* ok, uint8_t* gt384);
/* test / diagnosis: chunks the device verifier has run so far with a lane per proof (passes[0]) and in team form
 * (passes[1]) */
int rlnamd_verify_gpu_passes(rlnamd_prover* p, size_t passes[2]);
/* EXT: rlnamd_verify_many_gpu with an optimistic first pass (verify_agg.hip).  Same inputs, and the same verdicts up to
 * the probability below.  Per chunk of 65 536 proofs: the proofs that the per-proof checks refuse (a non-canonical
 * encoding, a point off its curve, B outside the order-r subgroup, an input >= r) get ok = 0 at once; every other
 * proof i gets a scalar r_i, uniform in [1, 2^128) and drawn inside the call (getrandom), after the proofs are fixed;
 * and ONE pairing check decides prod_i GT_i^(r_i) == 1 for the per-proof pairing products GT_i, at the cost of one
 * single-pair Miller loop per proof and one final exponentiation per chunk.  If it accepts, all those proofs get
 * ok = 1: since every GT_i lies in the order-r group, a chunk that holds an invalid proof is accepted with
 * probability about 2^-128 over the scalars.  If it rejects, the chunk runs through the exact pass of
 * rlnamd_verify_many_gpu, which names the bad proofs, and the next `cooldown` chunks (rlnamd_verify_gpu_set_cooldown;
 * default 16, a policy bound on the wasted work and not a measured optimum; 0 = none) go straight to the exact pass.
 * Taken only where the verifier would run a lane per proof (n > 1 024 unless RLNAMD_VERIFY_LANES says otherwise);
 * smaller calls are rlnamd_verify_many_gpu unchanged.  n = 0 succeeds; null pointers with n > 0, a wrong n_values and
 * a zero scalar in scalars16 are errors.  scalars16: NULL (drawn), or n x 16 bytes little-endian -- a test hook:
 * scalars known to the sender of the proofs void the bound. */
int rlnamd_verify_many_gpu_optimistic(rlnamd_prover* p, size_t n, const uint8_t* proofs, const uint8_t* values_le,
                                      size_t n_values, const uint8_t* scalars16, uint8_t* ok);
/* EXT: the same with the shape given and the combined check also in team form (verify_agg_team.hip).  lanes: 1 a lane
 * per proof, 8 a team of 8 lanes per proof, 0 the verifier's choice (teams up to 1 024 proofs: the threshold measured
 * for the exact forms); anything else is an error.  A call that takes teams runs the combined check with a team per
 * proof in chunks of 8 192, and a chunk it rejects runs through the exact team pass; the cool-down is the one above.
 * Everything else as rlnamd_verify_many_gpu_optimistic. */
int rlnamd_verify_many_gpu_optimistic_ex(rlnamd_prover* p, size_t n, const uint8_t* proofs, const uint8_t* values_le,
                                         size_t n_values, const uint8_t* scalars16, int lanes, uint8_t* ok);
/* out[0] chunks checked combined, [1] accepted, [2] fell back to the exact pass, [3] chunks that skipped the combined
 * check during a cool-down, [4] proofs the per-proof checks refused in combined checks, [5] cool-down chunks left,
 * [6] the cool-down setting, [7] the chunks of [0] that were checked in team form */
int rlnamd_verify_gpu_optimistic_stats(rlnamd_prover* p, uint64_t out[8]);
/* diagnosis: out[0] nanoseconds the combined checks have spent in the host's finish (L, -R alpha, one Miller loop of
 * three pairs and one final exponentiation per chunk; a host timer around it), out[1] the number of finishes */
int rlnamd_verify_gpu_finish_time(rlnamd_prover* p, uint64_t out[2]);
int rlnamd_verify_gpu_set_cooldown(rlnamd_prover* p, size_t chunks);
/* test / diagnosis: the final-exponentiated combined value prod_i GT_i^(r_i) of all n proofs, 12 x 32 bytes canonical
 * LE in pairing.h's coefficient order (1 = accept), with no fallback; rejected[i] = 1 where the per-proof checks
 * refuse proof i (it counts as 1 in the product).  scalars16 as above. */
int rlnamd_verify_gpu_aggregate(rlnamd_prover* p, size_t n, const uint8_t* proofs, const uint8_t* values_le,
                                size_t n_values, const uint8_t* scalars16, uint8_t gt384[384], uint8_t* rejected);
/* the same with the shape given: lanes 1 (as above, chunks of 65 536) or 8 (a team per proof, chunks of 8 192); the
 * chunk values are multiplied.  Anything else is an error. */
int rlnamd_verify_gpu_aggregate_ex(rlnamd_prover* p, size_t n, const uint8_t* proofs, const uint8_t* values_le,
                                   size_t n_values, const uint8_t* scalars16, int lanes, uint8_t gt384[384],
                                   uint8_t* rejected);
/* EXT: the scalars of a combined check derived from one 32-byte seed per chunk, as the relay step's combined check
 * derives them on the device (csrc/verify_agg_scalars.h, one permutation per 8 proofs).  Host only; out16 = n x 16
 * bytes.  Scalar i of chunk `chunk` is bytes [16 j, 16 j + 16) of S, little-endian, with g = i / 8, j = i % 8 and
 *   S = Keccak-f[1600]( seed[0..32) | "RLNAMD-AGG-SCAL1" (16 ASCII bytes) | chunk as 8 bytes LE | g as 8 bytes LE
 *                       | 0x01 | 70 zero bytes | 0x80 | 64 zero bytes )
 * that is, the 200-byte state is the one rate block (136 bytes) of the 64-byte message under the original Keccak pad
 * (the pad of hash_to_field) over a zero capacity, permuted ONCE; the state's bytes are its 25 lanes in order, each
 * little-endian.  A scalar that comes out 0 is replaced by 1.  Only bytes [0, 128) of S are used. */
int rlnamd_verify_agg_scalars(const uint8_t seed[32], uint64_t chunk, size_t n, uint8_t* out16);
/* test / diagnosis: rlnamd_verify_gpu_aggregate_ex, except that the scalars of chunk c of the call (c = 0, 1, ...; chunks
 * of 65 536 proofs for lanes = 1, of 8 192 for lanes = 8) are derived ON THE DEVICE from (seed32, c): the value equals
 * rlnamd_verify_gpu_aggregate_ex over rlnamd_verify_agg_scalars' output for each chunk.  A seed known to the sender of
 * the proofs voids the bound, as supplied scalars do. */
int rlnamd_verify_gpu_aggregate_seeded(rlnamd_prover* p, size_t n, const uint8_t* proofs, const uint8_t* values_le,
                                       size_t n_values, const uint8_t seed32[32], int lanes, uint8_t gt384[384],
                                       uint8_t* rejected);
/* its host-only twin from pairing.h alone (no GPU, none of the device form's folding): the product of the exact
 * per-proof pairing products raised to the scalars.  scalars16 must be given.  The value the device is judged by. */
int rlnamd_verify_aggregate_with_zkey(const uint8_t* zkey, size_t zkey_len, size_t n, const uint8_t* proofs,
                                      const uint8_t* values_le, size_t n_values, const uint8_t* scalars16,
                                      uint8_t gt384[384], uint8_t* rejected);
int rlnamd_verify_many_with_zkey(const uint8_t* zkey, size_t zkey_len, size_t n, const uint8_t* proofs,
                                 const uint8_t* values_le, size_t n_values, int threads, uint8_t* ok);
/* same check straight from arkzkey bytes; needs no GPU (host parser + host pairing only) */
int rlnamd_verify_with_zkey(const uint8_t* zkey, size_t zkey_len, const uint8_t proof[128],
                            const uint8_t values_le[160], int* ok);
/* host-only parse of the two circuit resources (zkey_from_raw / graph_from_raw, circuit/mod.rs:140-203);
 * counts[0..9] = instance vars, witness vars, constraints, a_nnz, b_nnz, |a_query|, |h_query|, |l_query|,
 * graph nodes, witness signals; counts[10] = tree depth, counts[11] = max_out, counts[12] = inputs size. */
int rlnamd_parse_resources(const uint8_t* zkey, size_t zkey_len, const uint8_t* graph, size_t graph_len,
                           uint64_t counts[13]);
/* ark-serialize point compression helpers (host): coords = A.x A.y B.x.c0 B.x.c1 B.y.c0 B.y.c1 C.x C.y */
int rlnamd_proof_compress(const uint8_t coords_le[256], uint8_t proof[128]);
int rlnamd_proof_decompress(const uint8_t proof[128], uint8_t coords_le[256]);

/* ---- relay step on the device: hash, verify and log n messages in one call -------------------------------------
 * The loop of a relay node over the three objects above -- rlnamd_hasher, the prover's device verifier and
 * rlnamd_nullifier_log -- as one object and one call.  A step gives exactly the composition of the three calls over the
 * same inputs: xs from rlnamd_hasher_hash_to_field (or xs_le as given), pass from rlnamd_verify_many_gpu_ex with the
 * relay's lanes, verdict[i] the first failing check in the reference's order proof -> root -> signal
 * (rln/src/public.rs:725-771), else RLNAMD_RELAY_OK; then the shares of the messages whose verdict is OK go through ONE
 * observe in index order, by the rule of ffi_nullifier_log_observe (rln.h): a single-message proof (n_values == 5: y |
 * root | nullifier | x | ext) gives one share, a multi-message proof (n_values == 3 k + 3, k the prover's max_out:
 * ys[k] | root | nullifiers[k] | x | ext | selector_used[k]) one share per slot whose selector is 1, in slot order; all
 * shares of a proof carry its x, its external nullifier and tags[i] (tags == NULL: each share's own sequence number).
 * status[i] is RLNAMD_SHARE_SKIPPED for a verdict other than OK and for a proof without a used slot, otherwise the
 * first of SPAM, FOREIGN, DUPLICATE, NEW that any of the proof's shares has; secrets_le[i] and first_tag[i] come from
 * the lowest slot with that status and are zero for SKIPPED.  A call of n messages gives what any split into
 * consecutive smaller calls gives.  The proofs' public values never return to the host between the stages, and
 * hashing runs beside the pairing kernels, on the hasher's stream.
 * The step refuses, each with its own text, before anything is enqueued and with the log, the hasher and the verifier
 * untouched: null pointers with n > 0; both or neither of (signals, signals_len, offsets) and xs_le; signals given to a
 * relay made without a hasher; what rlnamd_hasher_hash_to_field refuses (decreasing offsets, offsets[n] > signals_len);
 * n_values not the key's; n_roots > RLNAMD_RELAY_ROOTS_MAX; n * max(1, max_out) larger than the room left in the log.
 * The last is the one deliberate difference from the composition: how many shares a call records is known on the
 * device only and a step is all-or-nothing for the log, so it asks for room for the worst case.  n == 0 succeeds and
 * writes nothing.  rlnamd_relay_new borrows its three objects, which must outlive the relay, and refuses objects on
 * different devices; h may be NULL, then every step must bring xs_le.  A step holds the relay's mutex, then the
 * hasher's, the verifier's and the log's, in that order; between steps each borrowed object is usable on its own.
 * The results of a step hold recovered identity secrets: the relay's device and pinned buffers are overwritten before
 * the step returns, on every error path too.
 * info: [0] steps, [1] verifier chunks, [2] messages, [3] messages with verdict OK, [4] shares recorded, [5] non-zero
 * 16-byte words left in the relay's result buffers, device and pinned (0 expected), [6] messages hashed on the host
 * route, [7] messages refused RLNAMD_RELAY_BAD_EPOCH (0 for a relay that never sets a window).  The log's info[4] goes
 * up by one per chunk that records a share, its info[6] stays 0.
 *
 * The epoch window.  A member's quota is per external nullifier, so a relay must also decide WHICH external nullifiers
 * it relays for: a sender who proves under a fresh one for every message is otherwise never rate-limited, and a late
 * message of a retired epoch is recorded again and never removed.  The window W is the relay's state: k external
 * nullifiers, 0 <= k <= RLNAMD_RELAY_EPOCHS_MAX, kept on the device beside the roots; k = 0 (as made) is no window.
 * With a window a step is the windowless step with one change: a message whose verdict would be RLNAMD_RELAY_OK and
 * whose external nullifier is not in W gets RLNAMD_RELAY_BAD_EPOCH -- the check comes after proof, root and signal, so
 * no other verdict changes -- and status, secrets, first_tag and the log's records are what follows from those messages
 * never reaching the log.  The exact and the combined relay share the check and stay byte for byte equal.
 * rlnamd_relay_set_epochs with k >= 1 takes the relay's mutex and the log's, runs rlnamd_nullifier_log_retain on the
 * borrowed log with the new set, and only when that has succeeded installs the set; *removed is what the retain
 * removed.  So: everything the relay records lies in its window, and after every set_epochs the log holds only the
 * window.  A caller may still observe into the borrowed log directly; the next set_epochs sweeps what that brought in.
 * With k == 0 it switches the window off and removes nothing (*removed = 0).  It refuses what retain refuses for
 * k >= 1, and k > RLNAMD_RELAY_EPOCHS_MAX with a text of its own, before the handle is followed; a refused call and a
 * retain that fails leave both the window and the log as they were.  rlnamd_relay_epochs copies the window out, in the
 * order it was given (duplicates included): *k elements into out_le, which has room for RLNAMD_RELAY_EPOCHS_MAX.
 *
 * rlnamd_relay_new_ex: the same relay with flags; rlnamd_relay_new is flags = 0.
 *   RLNAMD_RELAY_OPTIMISTIC        every chunk that would run a lane per proof (more than 1 024 messages, or lanes = 1)
 *                                  takes the combined check of rlnamd_verify_many_gpu_optimistic instead of the exact
 *                                  pass: the per-proof checks, then ONE pairing check for the chunk
 *   RLNAMD_RELAY_OPTIMISTIC_TEAMS  the chunks in team form too (the rule of rlnamd_verify_many_gpu_optimistic_ex);
 *                                  alone it is an error, and so is any other bit
 * The flags are judged before the pointers, each refusal with its own text.  A step of such a relay returns what the
 * exact relay returns for the same inputs and log, byte for byte -- verdicts, statuses, secrets, first tags and the
 * log's records -- except that a chunk holding an invalid proof is accepted whole with probability about 2^-128.
 * The scalars are not drawn on the host: per chunk the step draws ONE seed of 32 bytes (getrandom) after the chunk's
 * proofs and values are in its staging buffer, sends it up with them, and a kernel derives the n scalars on the device
 * (rlnamd_verify_agg_scalars states the derivation; the chunk counter is the verifier's count of seeds drawn).  The
 * seed is uniform and unknown to the sender when the proofs are fixed, and each scalar is 128 bits of a keyed sponge's
 * output, so the bound holds up to the advantage of telling that output from uniform.
 * A chunk the combined check accepts runs no exact pass.  One it rejects runs the exact kernels of the same shape over
 * the proofs and values already on the device (no second copy in), which names the bad proofs, and starts the
 * verifier's cool-down: the next `cooldown` chunks of optimistic relays and calls (one setting and one set of
 * counters per prover: rlnamd_verify_gpu_set_cooldown, rlnamd_verify_gpu_optimistic_stats, rlnamd_verify_gpu_passes)
 * take the exact pass as a flags = 0 relay does.  A combined chunk waits twice on the host -- for the verifier's
 * stream before the host's share of the pairing check, then for the log's stream -- where an exact chunk waits once;
 * the hashing and the log's copy in run under the first wait.  rlnamd_relay_info is unchanged. */
#define RLNAMD_RELAY_OPTIMISTIC 1
#define RLNAMD_RELAY_OPTIMISTIC_TEAMS 2
typedef struct rlnamd_relay rlnamd_relay;
#define RLNAMD_RELAY_OK 0
#define RLNAMD_RELAY_BAD_PROOF 1    /* the verifier's ok == 0, or a selector element that is neither 0 nor 1 */
#define RLNAMD_RELAY_BAD_ROOT 2
#define RLNAMD_RELAY_BAD_SIGNAL 3
#define RLNAMD_RELAY_BAD_EPOCH 4     /* would be OK, but its external nullifier is not in the relay's window */
#define RLNAMD_RELAY_ROOTS_MAX 64
#define RLNAMD_RELAY_EPOCHS_MAX 64   /* = RLNAMD_LOG_RETIRE_MAX */
int rlnamd_relay_new(rlnamd_prover* p, rlnamd_nullifier_log* log, rlnamd_hasher* h /* or NULL */, int lanes /* 0 | 1 | 8 */,
                     rlnamd_relay** out);
int rlnamd_relay_new_ex(rlnamd_prover* p, rlnamd_nullifier_log* log, rlnamd_hasher* h /* or NULL */, int lanes /* 0 | 1 | 8 */,
                        int flags /* RLNAMD_RELAY_OPTIMISTIC [| RLNAMD_RELAY_OPTIMISTIC_TEAMS] */, rlnamd_relay** out);
void rlnamd_relay_free(rlnamd_relay* r);
int rlnamd_relay_step(rlnamd_relay* r, size_t n, const uint8_t* proofs /* n*128 */,
                      const uint8_t* values_le /* n*n_values*32, verifier order */, size_t n_values,
                      const uint8_t* signals, size_t signals_len, const uint64_t* offsets /* n+1 */, /* either these three ... */
                      const uint8_t* xs_le /* n*32 */,                                               /* ... or this, never both */
                      const uint8_t* roots_le, size_t n_roots /* 0: any root, ffi_verify_with_roots' rule */,
                      const uint64_t* tags /* n, or NULL */, uint8_t* verdict /* n */, uint8_t* status /* n */,
                      uint8_t* secrets_le /* n*32 or NULL */, uint64_t* first_tag /* n or NULL */);
int rlnamd_relay_set_epochs(rlnamd_relay* r, const uint8_t* external_nullifiers_le /* k*32 */, size_t k /* 0: no window */,
                            uint64_t* removed /* or NULL */);
int rlnamd_relay_epochs(rlnamd_relay* r, uint8_t* out_le /* RLNAMD_RELAY_EPOCHS_MAX*32 */, size_t* k);
int rlnamd_relay_info(rlnamd_relay* r, uint64_t out[8]);

/* ---- quota ledger: message ids drawn on the device, per member and external nullifier -----------------------------
 * The signer's counterpart of the relay's epoch window.  A second proof under one (external nullifier, member, message
 * id) is two shares on one line and gives the member's identity secret to every relay; a service that signs for many
 * members by leaf index (rlnamd_prover_submit_members) keeps that from happening by drawing each proof's message id
 * from a ledger.  The reference has no such state (zerokit leaves message ids to the caller); the meaning below is the
 * sequential text of zerokit_amd/csrc/quota_ledger.h.
 * rlnamd_quota_new: max_epochs x 2^depth 32-bit counters in device memory, zeroed, on the current device; 1 <= depth <=
 * 24, 1 <= max_epochs <= RLNAMD_RELAY_EPOCHS_MAX, anything else is refused with a text of its own.  used[slot][leaf]
 * is the next message id of member `leaf` under the external nullifier that holds `slot` of the window.  A ledger has a
 * mutex and a stream of its own; every call on a handle takes the mutex.
 * rlnamd_quota_set_epochs: the external nullifiers signed under from now on, 0 <= k <= max_epochs.  One that stays
 * keeps its slot and its counters; one that leaves has its slot zeroed on the device and freed; a new one gets a zeroed
 * slot; k = 0 empties the window; a duplicate in the list counts once and is no error.  Refused before anything is
 * enqueued, the ledger unchanged: a null pointer with k > 0, k > max_epochs, an element >= r.  (A device error behind
 * those checks is not a refusal and does change the ledger: the external nullifiers that leave are out of the window
 * before their slots are zeroed, the new ones are not in it; no id can repeat.)  rlnamd_quota_epochs copies
 * the window out in the order it was given, duplicates once: *k elements into out_le, which has room for
 * RLNAMD_RELAY_EPOCHS_MAX.
 *   AN EXTERNAL NULLIFIER THAT HAS LEFT THE WINDOW MUST NOT COME BACK: its counters are gone, and the ids drawn after
 *   its return repeat the ids drawn before it left.
 *   A LEDGER MADE BY rlnamd_quota_new IS NOT PERSISTED: a process that is restarted must not sign under an external
 *   nullifier that was open before the restart -- unless the ledger was opened on a directory, rlnamd_quota_open below.
 * rlnamd_quota_open: the same ledger on a directory that holds a checksummed snapshot (rlnamd_quota.bin) and a
 * write-ahead journal (rlnamd_quota.wal); the formats are in zerokit_amd/csrc/quota_store.h.  The store is created if
 * the directory is empty or absent and reopened otherwise.  journal_max_bytes: the journal's size behind which the call
 * that crossed it compacts (a new snapshot, an empty journal); 0 means max(1 MiB, the snapshot's bytes).  Every other
 * call keeps its meaning; what the store adds is an ORDER OF EVENTS:
 *   draw, draw_counts   1. the kernels run; 2. the draw's delta -- the counters it moved, as (key, absolute value) pairs
 *                       compacted on the device -- is copied back; 3. the record is appended and fdatasynced; 4. ONLY
 *                       THEN are ids and statuses copied into the caller's arrays.  A draw that granted nothing appends
 *                       nothing and syncs nothing.  If the append or the sync fails the call fails: ids_out and status
 *                       are untouched, the per-call buffers are wiped, the device counters stay advanced (those ids are
 *                       burnt, which is the safe side) and the ledger stays usable: the next record carries absolute
 *                       values.
 *   the *_members_drawn and *_members_drawn_counts proving calls
 *                       the same, the sync complete before anything is staged or enqueued for proving.  The streamed
 *                       forms draw all n ids first: one sync a call.
 *   set_epochs          1. the window record is appended and synced; 2. the window is applied.  A crash between the two
 *                       reopens into the new window, under which nothing was signed yet; a crash before the sync reopens
 *                       into the old one.  (A device error behind the record leaves the store refusing writes, and the
 *                       ledger so refusing draws, until it is reopened.)
 *   rlnamd_quota_free   compacts if the journal holds records, then closes.
 * AFTER REOPENING, HOWEVER THE PROCESS ENDED: the window is that of the last set_epochs that returned, or of one that was
 * in progress; every counter is >= one past the highest id of every call that returned; it may be higher by the ids of a
 * call that never returned; after a clean close it is exactly the counters.
 *   A LEDGER NEVER GOES BACKWARDS.  A record at the journal's end that is short, fails its CRC or is ill-formed is a torn
 *   tail -- it was never synced, so none of its ids left a call -- and is cut off.  A bad record with records behind it, a
 *   snapshot that fails its CRC, a damaged journal header, and a depth or max_epochs other than the caller's make
 *   rlnamd_quota_open FAIL, each with a text of its own (a bad record's names its offset).  No flag opens such a store
 *   anyway: removing the directory, and with it the duty not to sign under the epochs that were open, is the
 *   operator's decision.  A directory that another ledger holds (in this process or another: flock on the journal) is
 *   refused too, and so is a directory that is not empty and holds neither file.  An open that fails -- refused, or
 *   for want of device memory behind the store's own checks -- writes nothing: the directory is left as it was found.
 *   THE DIRECTORY IS AS SECRET AS THE LEDGER: the journal shows who signs how often.  Its files are created with mode
 *   0600 and are NOT encrypted.
 *   "An external nullifier that has left must not come back" stays the caller's duty, with a store as without.
 * rlnamd_quota_compact: the snapshot of the next generation and an empty journal, now.  Fails on a ledger without a store.
 * rlnamd_quota_store_info: [0] generation, [1] journal bytes, [2] records appended by this object, [3] syncs, [4]
 * compactions, [5] records replayed at open, [6] torn bytes cut at open, [7] (key, counter) pairs restored to the device
 * at open.  All zero for a ledger without a store.
 * rlnamd_quota_draw: n requests (leaf_indices[i], ext_le[i], limits[i]) -> ids_out[i], status[i].
 *   RLNAMD_QUOTA_NO_EPOCH  ext[i] is not in the window; the request touches nothing
 *   otherwise              rank_i = the number of requests j < i of this call with the same (external nullifier, leaf),
 *                          whatever their outcome; id_i = used + rank_i with `used` as it was before the call;
 *                          RLNAMD_QUOTA_OK iff id_i < limits[i], else RLNAMD_QUOTA_OVER
 *   afterwards             the counter is one more than the highest id issued for it in this call, and unchanged if none was
 * ids_out[i] is id_i for OK and limits[i] otherwise (never a valid message id: the circuit's range check fails for it).  The protocol
 * means one limit per member; with that this is drawing one by one in index order -- OVER consumes nothing, and a call
 * gives what any split of it into consecutive calls gives.  With differing limits for one member an id can be skipped
 * but none is issued twice.  Refused before anything is enqueued, the ledger unchanged: null pointers with n > 0, a
 * leaf index >= 2^depth, n >= 2^32.  n == 0 succeeds.  The time of a draw does not depend on how often members repeat:
 * n requests of one member and n requests of n members run the same passes (a stable radix sort by key, two running
 * maxima, one pass that issues, one that advances the counters).
 * Who signs how often is as secret as who proves: the staged leaf indices, the sort's keys and every other per-call word,
 * in device and in pinned memory, are overwritten before draw returns, on error paths too, and rlnamd_quota_free zeroes
 * the counters.
 * rlnamd_quota_draw_counts: blocks of ids, for the multi-message-id circuit, one proof of which uses up to max_out
 * message slots.  n requests (leaf_indices[i], ext_le[i], limits[i], counts[i]), counts[i] = 1 .. RLNAMD_QUOTA_COUNT_MAX
 * the number of ids the request asks for -> firsts_out[i], status[i].
 *   RLNAMD_QUOTA_NO_EPOCH  ext[i] is not in the window; the request touches nothing
 *   otherwise              rank_i = the sum of counts[j] over the requests j < i of this call with the same (external
 *                          nullifier, leaf), whatever their outcome; first_i = used + rank_i with `used` as it was
 *                          before the call; RLNAMD_QUOTA_OK iff first_i + counts[i] <= limits[i] (in 64 bits), and the
 *                          request then owns the ids first_i .. first_i + counts[i] - 1; else RLNAMD_QUOTA_OVER: a
 *                          request is granted whole or not at all
 *   afterwards             the counter is first + count of its last OK request of this call, and unchanged if none was
 * firsts_out[i] is first_i for OK and limits[i] otherwise.  With every count 1 this is rlnamd_quota_draw.  With one
 * limit per member the OK requests of a (external nullifier, leaf) are a prefix of its requests, and the blocks granted
 * for it, over any sequence of calls, are pairwise disjoint and each lies below its limit.
 *   A CALL IS NOT WHAT EVERY SPLIT OF IT GIVES: a refused request still counts, with its whole block, in the ranks
 *   behind it, so a smaller request of the same member later in the same call is refused although it would have
 *   fitted; the next call grants it.  Only the all-ones case keeps rlnamd_quota_draw's split property.
 * Refused before anything is enqueued, each with a text of its own, the ledger unchanged: what rlnamd_quota_draw
 * refuses, a null `counts`, a count of 0, a count above RLNAMD_QUOTA_COUNT_MAX (which a byte cannot hold: the text is
 * for callers that pack wider counts), n >= 2^24 (n x 255 then stays below 2^32; judged before any array is read).  The
 * passes are rlnamd_quota_draw's plus one gather of the counts into sorted order and one sum over them; one member n
 * times and n members cost the same here too.  The wipe is rlnamd_quota_draw's.
 * rlnamd_quota_used: the counters of n (leaf, external nullifier) pairs, for diagnostics and tests; in_window[i] = 0 and
 * used_out[i] = 0 for an external nullifier outside the window.
 * info: [0] external nullifiers in the window, [1] draws, [2] ids issued (a granted request of rlnamd_quota_draw_counts
 * counts with its count), [3] requests refused OVER, [4] requests
 * refused NO_EPOCH, [5] non-zero 16-byte words left in the ledger's per-call buffers, device and pinned (0 expected),
 * [6] depth, [7] max_epochs.
 * rlnamd_quota_plan (host only): the passes of a draw of n requests on a ledger of `depth` -- [0] sort passes, [1]
 * workgroups a pass, [2] scan levels over a pass's bins, [3] scan levels over the requests.  It holds for
 * rlnamd_quota_draw_counts as it stands: the sum over the counts is one more scan over the n requests, with the levels
 * of [3], and the gather has the workgroups of [1]; nothing it reports changes. */
typedef struct rlnamd_quota rlnamd_quota;
#define RLNAMD_QUOTA_OK 0
#define RLNAMD_QUOTA_OVER 1
#define RLNAMD_QUOTA_NO_EPOCH 2
int rlnamd_quota_new(size_t depth, size_t max_epochs, rlnamd_quota** out);
int rlnamd_quota_open(const char* dir, size_t depth, size_t max_epochs, uint64_t journal_max_bytes /* 0: max(1 MiB, snapshot bytes) */,
                      rlnamd_quota** out);
int rlnamd_quota_compact(rlnamd_quota* q);
int rlnamd_quota_store_info(rlnamd_quota* q, uint64_t out[8]);
void rlnamd_quota_free(rlnamd_quota* q);
int rlnamd_quota_set_epochs(rlnamd_quota* q, const uint8_t* external_nullifiers_le /* k*32 */, size_t k /* 0: empty */);
int rlnamd_quota_epochs(rlnamd_quota* q, uint8_t* out_le /* RLNAMD_RELAY_EPOCHS_MAX*32 */, size_t* k);
int rlnamd_quota_draw(rlnamd_quota* q, size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le /* n*32 */,
                      const uint32_t* limits /* n */, uint32_t* ids_out /* n */, uint8_t* status /* n */);
#define RLNAMD_QUOTA_COUNT_MAX 255 /* the most message slots a relay takes a proof (a share count is a byte) */
int rlnamd_quota_draw_counts(rlnamd_quota* q, size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le /* n*32 */,
                             const uint32_t* limits /* n */, const uint8_t* counts /* n bytes */, uint32_t* firsts_out /* n */,
                             uint8_t* status /* n */);
int rlnamd_quota_used(rlnamd_quota* q, size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le /* n*32 */,
                      uint32_t* used_out /* n */, uint8_t* in_window /* n */);
int rlnamd_quota_info(rlnamd_quota* q, uint64_t out[8]);
int rlnamd_quota_plan(size_t n, size_t depth, uint64_t out[4]);

/* ---- proving with drawn message ids.  rlnamd_prover_submit_members_drawn is rlnamd_prover_submit_members (full proofs
 * only) with the messageId slot of inputs_le ignored: each proof's limit and external nullifier are read from its own
 * input row (userMessageLimit, externalNullifier), ONE rlnamd_quota_draw covers the call, and status[i] is its answer.
 * A batch so needs only secret, limit, x and external nullifier from the caller.  A request that is not
 * RLNAMD_QUOTA_OK yields no proof: its messageId slot is filled with 0xFF bytes, which is no field element, so the
 * witness interpreter refuses the row as it refuses any input >= r, and collect gives errors[i] != 0, 128 zero proof
 * bytes and 160 zero value bytes for it (collect zeroes them, behind its copies, for every row of such a batch that has an error: every refused row is
 * evaluated with one and the same message id, and the y values of two of them would be two shares on one line).  Its
 * limit would not do: the interpreter evaluates the circuit's range check without asserting it.  On the device
 * route (rlnamd_prover_submit_members' rule) the ids never visit the host: one kernel behind the staging writes them
 * into the staged rows, ordered against the ledger's stream by events; the host route copies the batch's ids back once.
 * The staged bytes are the same.  The draw's block is overwritten before the call returns (rlnamd_quota_info[5] is 0).
 * Locks: the tree's, then the ledger's, both held for the call.  Refused before anything is drawn or enqueued, each with
 * a text of its own: what submit_members refuses; a graph without a single messageId input (the multi-message-id
 * circuit); a ledger whose depth is not the tree's; objects on different devices; a limit >= 2^32.
 * rlnamd_prover_prove_stream_members_drawn: the chunked form.  All n ids are drawn first and every chunk reads its
 * slice, so a call keeps the one-by-one meaning across chunks. */
int rlnamd_prover_submit_members_drawn(rlnamd_prover* p, rlnamd_tree* t, rlnamd_quota* q, size_t n, const uint64_t* leaf_indices,
                                       const uint8_t* inputs_le, const uint8_t* rs_le, uint8_t* status /* n */, uint64_t* ticket);
int rlnamd_prover_prove_stream_members_drawn(rlnamd_prover* p, rlnamd_tree* t, rlnamd_quota* q, size_t n,
                                             const uint64_t* leaf_indices, const uint8_t* inputs_le, const uint8_t* rs_le,
                                             uint8_t* status /* n */, uint8_t* proofs /* n*128 */, uint8_t* values /* n*160 */,
                                             uint32_t* errors /* n */);

/* ---- proving with drawn blocks of message ids: the multi-message-id circuit, one proof of which uses up to max_out
 * message slots.  rlnamd_prover_submit_members_drawn_counts is rlnamd_prover_submit_members_drawn with counts[i] = 1 ..
 * max_out, the number of slots proof i uses: ONE rlnamd_quota_draw_counts covers the call (its closed form and its
 * caveat -- a call is NOT what every split of it gives -- hold as stated there), and status[i] is its answer.  The
 * messageId and selectorUsed slots of inputs_le are ignored.  A granted row gets messageId[k] = first_i + k and
 * selectorUsed[k] = 1 for k < counts[i], and 0 in both above; a request that is not RLNAMD_QUOTA_OK gets 0xFF bytes in
 * EVERY message slot and zero selectors, the witness interpreter refuses the row, and collect and collect_public give
 * errors[i] != 0, 128 zero proof bytes and num_public * 32 zero value bytes for it.  Routes, events and locks are those
 * of rlnamd_prover_submit_members_drawn; one kernel behind the staging writes ids and selectors on the device route, and
 * the host route copies the batch's firsts back once and writes the same bytes.  rlnamd_quota_info[5] is 0 afterwards.
 * Refused before anything is drawn or enqueued, each with a text of its own: what submit_members refuses; a graph that
 * does not name userMessageLimit, externalNullifier, messageId[max_out] and selectorUsed[max_out] (a single message-id
 * graph names no selectors, needs none, and takes counts of 1: the call then gives what
 * rlnamd_prover_submit_members_drawn gives); a count of 0; a count above max_out; a ledger whose depth is not the
 * tree's; objects on different devices; a limit >= 2^32.
 * rlnamd_prover_prove_stream_members_drawn_counts: the chunked form, all n blocks drawn first, every chunk reading its
 * slice.  values_public is n * num_public * 32 bytes, every public signal of a proof: ys | root | nullifiers | x |
 * external nullifier | selectors on the multi-message-id circuit. */
int rlnamd_prover_submit_members_drawn_counts(rlnamd_prover* p, rlnamd_tree* t, rlnamd_quota* q, size_t n,
                                              const uint64_t* leaf_indices, const uint8_t* inputs_le, const uint8_t* rs_le,
                                              const uint8_t* counts /* n bytes */, uint8_t* status /* n */, uint64_t* ticket);
int rlnamd_prover_prove_stream_members_drawn_counts(rlnamd_prover* p, rlnamd_tree* t, rlnamd_quota* q, size_t n,
                                                    const uint64_t* leaf_indices, const uint8_t* inputs_le, const uint8_t* rs_le,
                                                    const uint8_t* counts /* n bytes */, uint8_t* status /* n */,
                                                    uint8_t* proofs /* n*128 */, uint8_t* values_public /* n*num_public*32 */,
                                                    uint32_t* errors /* n */);

/* ---- member directory on the device: register, resolve secrets, slash ----------------------------------------------
 * The object that closes the loop tree -> prove by member -> quota ledger / hasher -> verifier -> nullifier log -> relay:
 * for every RLNAMD_SHARE_SPAM a relay step returns the member's identity secret, and the directory answers whose secret
 * that is, which leaf it holds and what its limit is, and removes it.  The tree in HBM holds only rate commitments,
 * Poseidon(id_commitment, limit); the directory keeps, beside it, (id_commitment, limit) per leaf index and a keyed hash
 * table from id_commitment to leaf index.  The reference has no such state.  The meaning below is the sequential text of
 * zerokit_amd/csrc/member_directory.h.
 * rlnamd_directory_new: a directory D over the dense tree `tree`, which it BORROWS (the tree must outlive it), covering the
 * leaf indices [0, capacity), 1 <= capacity <= min(2^depth, 2^31); seed keys the table's hash, 0 = drawn from getrandom
 * (registrations arrive from outside: a sender who does not know the seed cannot aim commitments at one slot).  Per index D
 * holds a state, FREE or LIVE, and for a LIVE index the member's identity commitment (canonical Fr) and its limit (uint32 >=
 * 1, the type the quota ledger uses).  At most one LIVE index carries a given commitment.  D starts empty.  37 bytes per
 * index plus 4 bytes per table slot, 2 * capacity slots rounded up to a power of two (45 MiB at 2^20).
 *   D WRITES ONLY THE LEAVES OF INDICES IT REGISTERS OR REMOVES.  A leaf written behind its back through rlnamd_tree_set_*
 *   is not noticed: D still answers from its own rows.
 *   D IS NOT PERSISTED.  A directory made over a tree that already holds leaves is empty.  Registering the same events
 *   again rebuilds it: they write the same leaves, so the root does not move.  That is the way back after a restart.
 * Every call runs on the tree's stream and takes the directory's mutex and then the tree handle's, both for the call:
 * that orders it against rlnamd_tree_* and against the path gathers of rlnamd_prover_submit_members with no extra event.
 * rlnamd_directory_register: n requests (indices[i], idcs_le[i], limits[i]) -> status[i].  Refused as a whole before
 * anything is enqueued, each with a text of its own, D and the tree untouched: a null pointer with n > 0, an index >=
 * capacity, an index that occurs twice in the call, a commitment >= r, a limit of 0, n >= 2^32.  Otherwise the call is a
 * SET of requests, and its outcome does not depend on their order:
 *   RLNAMD_DIR_OCCUPIED  the index was LIVE before the call.  This is checked first.
 *   RLNAMD_DIR_KNOWN     not OCCUPIED, and either the commitment was LIVE somewhere before the call, or another request of
 *                        the call that is not OCCUPIED carries the same commitment at a lower index.
 *   RLNAMD_DIR_OK        otherwise: the index becomes LIVE with (commitment, limit), and its leaf becomes
 *                        Poseidon(commitment, Fr(limit)) (t = 3, rln/src/hashers.rs), computed and written on the device.
 * An OCCUPIED request never blocks another request that carries the same commitment at a free index.  After the call the
 * tree's root reflects the new leaves: one bottom-up pass runs over the union of the paths.
 *   A CALL WITH DUPLICATE COMMITMENTS IS NOT WHAT EVERY SPLIT OF IT GIVES: inside a call the lowest index wins, across
 *   calls the first call wins.
 * rlnamd_directory_find: n commitments -> RLNAMD_DIR_FOUND with the live index and its limit, else RLNAMD_DIR_UNKNOWN with
 * index UINT64_MAX and limit 0 (a commitment >= r is never LIVE, so it is UNKNOWN).
 * rlnamd_directory_resolve: n identity secrets -> the same outputs for Poseidon(secret) (t = 2), hashed on the device.
 * take may be NULL, which means all; take[i] == 0 gives RLNAMD_DIR_SKIPPED, the secret is not read, index and limit are
 * as for UNKNOWN.  A taken secret >= r refuses the call.  `take` exists so that status == RLNAMD_SHARE_SPAM of a relay step
 * goes in as it is, beside the step's secrets.
 * rlnamd_directory_slash: resolve's outputs, and every FOUND member is removed: state FREE, leaf = the tree's default
 * leaf, one pass over the union of the paths.  Two secrets of one member in a call are both FOUND with the same index;
 * *removed counts distinct members.  The call is exactly resolve followed by remove of the distinct found indices.
 * rlnamd_directory_remove: a withdrawal by index -> RLNAMD_DIR_REMOVED, or RLNAMD_DIR_VACANT: the index was not LIVE, and
 * nothing is written.  The refusals follow register's index rules.  A removed commitment may be registered again, at the
 * same index or another.
 * rlnamd_directory_get: n indices, repeats allowed -> live[i] (0 / 1), the commitment and the limit; FREE rows read as zero.
 *   RECOVERED SECRETS ARE AS SENSITIVE AS ANYWHERE ELSE HERE: resolve and slash overwrite their device and pinned staging
 *   before they return, on every error path too, as the relay does; info[7] proves it.
 * info: [0] capacity, [1] live members, [2] table slots, [3] slots taken, those of removed members included, [4] table
 * rebuilds (a removed member's slot is not handed out again, so before a call that could leave more than half of the slots
 * taken the table is rebuilt from the live rows), [5] longest walk of any call, [6] calls, [7] non-zero 16-byte words left in
 * the staging that held secrets, device and pinned (0 expected). */
typedef struct rlnamd_directory rlnamd_directory;
#define RLNAMD_DIR_OK 0
#define RLNAMD_DIR_OCCUPIED 1
#define RLNAMD_DIR_KNOWN 2
#define RLNAMD_DIR_FOUND 0
#define RLNAMD_DIR_UNKNOWN 1
#define RLNAMD_DIR_SKIPPED 2
#define RLNAMD_DIR_REMOVED 0
#define RLNAMD_DIR_VACANT 1
int rlnamd_directory_new(rlnamd_tree* tree, size_t capacity, uint64_t seed /* 0 = random */, rlnamd_directory** out);
void rlnamd_directory_free(rlnamd_directory* d);
int rlnamd_directory_register(rlnamd_directory* d, size_t n, const uint64_t* indices, const uint8_t* idcs_le /* n*32 */,
                              const uint32_t* limits /* n */, uint8_t* status /* n */);
int rlnamd_directory_find(rlnamd_directory* d, size_t n, const uint8_t* idcs_le /* n*32 */, uint8_t* status /* n */,
                          uint64_t* index /* n */, uint32_t* limit /* n */);
int rlnamd_directory_resolve(rlnamd_directory* d, size_t n, const uint8_t* secrets_le /* n*32 */, const uint8_t* take /* n or NULL */,
                             uint8_t* status /* n */, uint64_t* index /* n */, uint32_t* limit /* n */);
int rlnamd_directory_slash(rlnamd_directory* d, size_t n, const uint8_t* secrets_le /* n*32 */, const uint8_t* take /* n or NULL */,
                           uint8_t* status /* n */, uint64_t* index /* n */, uint32_t* limit /* n */, uint64_t* removed /* or NULL */);
int rlnamd_directory_remove(rlnamd_directory* d, size_t n, const uint64_t* indices, uint8_t* status /* n */);
int rlnamd_directory_get(rlnamd_directory* d, size_t n, const uint64_t* indices, uint8_t* live /* n */, uint8_t* idcs_le /* n*32 */,
                         uint32_t* limits /* n */);
int rlnamd_directory_info(rlnamd_directory* d, uint64_t out[8]);

/* ---- variable-base MSM on G1 / G2 (BASELINE config 5; north_star: "windowed Pippenger MSM on G1/G2") ---------
 * Replaces VariableBaseMSM::msm_bigint (ark-ec 0.5.0; call sites rln/src/partial_proof.rs:98-104,255-256: generic
 * over the group) for large n with bases that are not fixed.  Multi-GPU: every rank runs rlnamd_msm_run on its slice of
 * the points, the window sums (rlnamd_msm_window_sums_bytes_of(m) bytes per rank) are all-gathered, and
 * rlnamd_msm_combine adds them and folds the windows.
 * rlnamd_msm_new = G1: points are 64 bytes (x | y), results 64 bytes.  rlnamd_msm_new_g2 = G2: points and results are
 * 128 bytes (x.c0 | x.c1 | y.c0 | y.c1); every call below takes either handle (the *_xy_le buffers are
 * rlnamd_msm_point_bytes(m) bytes per point); the synthetic workload of a G2 handle is P_i = k_i G2 (the generator of
 * the twist's order-r subgroup) under the same SplitMix64 stream. */
typedef struct rlnamd_msm rlnamd_msm;
int rlnamd_msm_new(size_t capacity, rlnamd_msm** out);
int rlnamd_msm_new_g2(size_t capacity, rlnamd_msm** out);
void rlnamd_msm_free(rlnamd_msm* m);
size_t rlnamd_msm_point_bytes(rlnamd_msm* m);
size_t rlnamd_msm_window_sums_bytes_of(rlnamd_msm* m);
/* Device self-test: the 9 x 29-bit-limb group law the MSM walks use (csrc/fq29.h) against the 8 x 32-bit one on
 * `threads` pseudo-random walks of `iters` signed additions each (doublings, cancellations, restarts from infinity
 * included).  group 1 = G1, 2 = G2, 3 = G2 computed by lane pairs, 4 = G1 general additions by lane pairs (g2_gen_xy_le = generator x.c0 | x.c1 | y.c0 | y.c1,
 * canonical LE; NULL for G1).
 * *mismatches = number of walks whose affine results differ (0 expected). */
/* Parameter self-check, host only (no device, not a hashing path): derives the Poseidon parameters for `arity`
 * inputs (Grain LFSR, utils/src/poseidon/poseidon_constants.rs:207-261) and evaluates ONE hash twice on the host --
 * with the reference's dense rounds (poseidon_hash.rs:97-135) and with the equivalent sparse partial rounds the device
 * kernels use -- so the CPU test suite can compare both with the oracle. */
int rlnamd_poseidon_params_check(const uint8_t* inputs_le, size_t arity, uint8_t out_dense_le[32], uint8_t out_sparse_le[32]);
int rlnamd_selftest_fq29(int group, uint32_t threads, uint32_t iters, const uint8_t* g2_gen_xy_le, uint32_t* mismatches);
/* Arithmetic probes (test support): ONE device function per call, run on n operand tuples of the caller's choosing, one
 * lane per tuple; in = n x in_words and out = n x out_words 32-bit words in host memory, copied to the device and back
 * unchanged (no conversion, no reduction: the caller judges the raw words).  in_words / out_words are the words per tuple
 * and must be the operation's own (checked).  n = 0 returns RLNAMD_OK without a launch.
 *
 * rlnamd_probe_field: the 8 x 32-bit Montgomery field of csrc/field.h, field 0 = Fr, 1 = Fq; operands and results are
 * 8-word elements as the kernels hold them (in_words = 8 x operands, out_words = 8 x results):
 *   add sub mul (a, b); neg dbl sqr inv from_canonical to_canonical (a); dot2 dot2_sub (a, b, c, d: ab +- cd);
 *   dot3, dot4 (a0, b0, a1, b1, ...); Fq only: Fq2 mul (a.c0, a.c1, b.c0, b.c1 -> c0, c1), sqr, inv (a.c0, a.c1 -> c0, c1). */
enum {
  RLNAMD_PROBE_FP_ADD = 0, RLNAMD_PROBE_FP_SUB, RLNAMD_PROBE_FP_NEG, RLNAMD_PROBE_FP_DBL, RLNAMD_PROBE_FP_MUL,
  RLNAMD_PROBE_FP_SQR, RLNAMD_PROBE_FP_DOT2, RLNAMD_PROBE_FP_DOT3, RLNAMD_PROBE_FP_DOT4, RLNAMD_PROBE_FP_DOT2_SUB,
  RLNAMD_PROBE_FP_FROM_CANONICAL, RLNAMD_PROBE_FP_TO_CANONICAL, RLNAMD_PROBE_FP_INV,
  RLNAMD_PROBE_FQ2_MUL, RLNAMD_PROBE_FQ2_SQR, RLNAMD_PROBE_FQ2_INV, RLNAMD_PROBE_FP_OPS
};
int rlnamd_probe_field(int field, uint32_t op, uint32_t in_words, uint32_t out_words, size_t n, const uint32_t* in, uint32_t* out);
/* rlnamd_probe_f29: the 9 x 29-bit limb form of csrc/fq29.h, field 0 = Fr29, 1 = Fq29; a 9 x 29 element is 9 raw limb
 * words, an 8 x 32 element 8 words.  Per tuple:
 *   MUL (a, b)  MUL_ADD (a, b, add)  SQR (a)  SQR_ADD (a, add)  DOT2 (a0, b0, a1, b1)  DOT2_ADD (a0, b0, a1, b1, add)
 *   DOT3 / DOT3_WIDE / DOT4 / DOT4_WIDE (a0, b0, a1, b1, ...: masked / wide reduction rounds)
 *   DOTN5 (a0, b0, ... a4, b4: poseidon.h's poseidon_dotn29<5>, Fr29 only)
 *   SUB_K2 .. SUB_K8 (a, b -> a + K - b, normalised)   NEG_K2 .. NEG_K8 (b -> K - b, limb by limb)   NORMALIZE (a)
 *   IS_ZERO (a -> 1 word)   SLICE (8 words -> 9)   PACK_REDUCED (9 -> 8)   FROM_FQ (8 -> 9)   TO_FQ (9 -> 8)
 *   MUL_MONT (a: 8 words, w29: 9 words -> 8)   FROM_CANONICAL (8 -> 9: mul(slice(x), FROM_CANON), the witness
 *   interpreters' input conversion)   UNPACK29 (8 -> 9) and PACK29_REDUCED (9 -> 8), Fq29 only
 * and the lane forms of the group law, Fq29 only:
 *   G1_WALK / G2_WALK   a lane starts from infinity and applies madd for each of 1 .. 32 steps, the same count for every
 *                       lane: in_words = steps x (1 + 16 | 32): a flag word (bit 0: negate, bit 1: no entry at this step)
 *                       and a table entry (G1Affine29 x | y, G2Affine29 x0 | x1 | y0 | y1); out_words = steps x (36 | 72):
 *                       the raw accumulator X | Y | ZZ | ZZZ (G2: c0 | c1 each) after every step
 *   G1_ADD / G2_ADD     two raw accumulators -> a.add(b)
 *   G1_TABLE / G2_TABLE to_table29 of an affine point in the 8 x 32 Montgomery form (16 | 32 words in and out) */
enum {
  RLNAMD_PROBE_F29_MUL = 0, RLNAMD_PROBE_F29_MUL_ADD, RLNAMD_PROBE_F29_SQR, RLNAMD_PROBE_F29_SQR_ADD,
  RLNAMD_PROBE_F29_DOT2, RLNAMD_PROBE_F29_DOT2_ADD, RLNAMD_PROBE_F29_DOT3, RLNAMD_PROBE_F29_DOT3_WIDE,
  RLNAMD_PROBE_F29_DOT4, RLNAMD_PROBE_F29_DOT4_WIDE, RLNAMD_PROBE_F29_DOTN5,
  RLNAMD_PROBE_F29_SUB_K2, RLNAMD_PROBE_F29_SUB_K4, RLNAMD_PROBE_F29_SUB_K6, RLNAMD_PROBE_F29_SUB_K8,
  RLNAMD_PROBE_F29_NEG_K2, RLNAMD_PROBE_F29_NEG_K4, RLNAMD_PROBE_F29_NEG_K6, RLNAMD_PROBE_F29_NEG_K8,
  RLNAMD_PROBE_F29_NORMALIZE, RLNAMD_PROBE_F29_IS_ZERO, RLNAMD_PROBE_F29_SLICE, RLNAMD_PROBE_F29_PACK_REDUCED,
  RLNAMD_PROBE_F29_FROM_FQ, RLNAMD_PROBE_F29_TO_FQ, RLNAMD_PROBE_F29_MUL_MONT, RLNAMD_PROBE_F29_FROM_CANONICAL,
  RLNAMD_PROBE_F29_UNPACK29, RLNAMD_PROBE_F29_PACK29_REDUCED,
  RLNAMD_PROBE_G1_WALK, RLNAMD_PROBE_G2_WALK, RLNAMD_PROBE_G1_ADD, RLNAMD_PROBE_G2_ADD, RLNAMD_PROBE_G1_TABLE,
  RLNAMD_PROBE_G2_TABLE, RLNAMD_PROBE_F29_OPS
};
int rlnamd_probe_f29(int field, uint32_t op, uint32_t in_words, uint32_t out_words, size_t n, const uint32_t* in, uint32_t* out);
/* rlnamd_probe_witness_op: csrc/witness_ops.h.  in: n x 17 words (graph opcode, a, b: Fr in the 8 x 32 form), out: n x 9
 * (witness_slow_op's value, its error word).  Mul / Add / Sub, which the interpreters never hand to witness_slow_op,
 * are answered with the 8 x 32 operators. */
int rlnamd_probe_witness_op(size_t n, const uint32_t* in, uint32_t* out);
/* rlnamd_probe_log_positions: the position pass of rlnamd_nullifier_log_retire alone -- keep: n bytes (0 / non-zero) ->
 * pos: n exclusive positions, *kept: the number of non-zero bytes.  Runs the same kernels the retire runs, on buffers of
 * its own; n = 0 succeeds without a launch. */
int rlnamd_probe_log_positions(const uint8_t* keep, size_t n, uint32_t* pos, uint64_t* kept);
/* rlnamd_probe_quotient_transform: the three steps every vector of the quotient goes through -- inverse transform, x g^i
 * (g the root of the doubled domain), forward transform (circuit/qap.rs:60-90) -- launched by the function the prover
 * itself launches them with, at ANY domain size: lds = 0 the passes of ntt_pass_list(logn) (k_ntt_pass / k_ntt_turn, what
 * a big batch takes), lds = 1 the edge / mid / edge kernels of a small batch.  in / out: vectors x 2^logn x nb canonical
 * values of 8 words ([vector][index][lane], dense); on the device they sit in the prover's [index][B] layout, nb of the B
 * lanes live.  An error, before anything is launched: logn outside 1 .. 18, lds with logn outside 9 .. 18, nb = 0 or
 * nb > B, vectors outside 1 .. 3, more than 2^26 elements in the layout. */
int rlnamd_probe_quotient_transform(int logn, int lds, uint32_t B, uint32_t nb, uint32_t vectors, const uint32_t* in,
                                    uint32_t* out);
/* points: n x (x || y) canonical LE affine, all-zero = infinity; scalars: n x 32 bytes canonical LE */
int rlnamd_msm_set(rlnamd_msm* m, const uint8_t* points_xy_le, const uint8_t* scalars_le, size_t n);
/* synthetic config-5 workload generated in HBM: P_i = k_i G, scalars s_i, SplitMix64(seed) at index first+i */
int rlnamd_msm_generate(rlnamd_msm* m, uint64_t seed, uint64_t first_index, size_t n);
/* distribution variants of the same workload: mode bit 0 = every scalar equals s_0 (all n points in ONE bucket per
 * window), bit 1 = k_i = k_(i mod 4) (four distinct bases).  The library carries no expected value for its own
 * workload: the closed form (sum k_i s_i mod r) G lives in the oracle (oracle/c: oracle_msm_expected). */
#define RLNAMD_MSM_EQUAL_SCALARS 1u
#define RLNAMD_MSM_FOUR_POINTS 2u
int rlnamd_msm_generate_mode(rlnamd_msm* m, uint64_t seed, uint64_t first_index, size_t n, uint32_t mode);
/* reads points [first, first + count) of the loaded / generated workload back (affine x || y, scalars; canonical LE) */
int rlnamd_msm_fetch(rlnamd_msm* m, size_t first, size_t count, uint8_t* points_xy_le, uint8_t* scalars_le);
size_t rlnamd_msm_window_sums_bytes(void);
/* ms[0] digits + counting sort, ms[1] bucket accumulation, ms[2] bucket reduction */
int rlnamd_msm_run(rlnamd_msm* m, uint8_t* window_sums, float ms[3]);
int rlnamd_msm_combine(rlnamd_msm* m, const uint8_t* window_sums, size_t contributors, uint8_t out_xy_le[64]);


/* ---- multi-GPU (BASELINE configs 4 and 5) -----------------------------------------------------
 * rlnamd_pool: one prover replica and one host thread per device of THIS process.  rlnamd_pool_prove cuts n proofs
 * into contiguous index shards, one per replica (config 4: 65 536 proofs = 8 x 8 192), each replica streams its shard
 * (rlnamd_prover_prove_stream) and writes its results at their index: proofs n * 128, values n * 160, errors n * 4
 * (any may be NULL).  No data-path collective -- the proofs are independent (the reference's guidance is one worker per
 * proof, rln/README.md:324-332).  devices = NULL / n_devices = 0: every visible device.  An ordinal may repeat (two
 * replicas sharing one device, for tests on a 1-GPU box). */
typedef struct rlnamd_pool rlnamd_pool;
int rlnamd_pool_new(const uint8_t* zkey, size_t zkey_len, const uint8_t* graph, size_t graph_len, size_t max_batch,
                    int window_bits, const int* devices, size_t n_devices, rlnamd_pool** out);
void rlnamd_pool_free(rlnamd_pool* p);
size_t rlnamd_pool_size(rlnamd_pool* p);
int rlnamd_pool_device(rlnamd_pool* p, size_t replica);
int rlnamd_pool_get_info(rlnamd_pool* p, rlnamd_prover_info* info);
int rlnamd_pool_prove(rlnamd_pool* p, size_t n, const uint8_t* inputs_le, const uint8_t* rs_le, uint8_t* proofs,
                      uint8_t* values, uint32_t* errors);
int rlnamd_pool_last_ms(rlnamd_pool* p, float* ms_per_replica);   /* host wall time of each replica's last shard */
/* Assignment of a job's proofs to the replicas: 0 (default) = contiguous index shards, one per replica; 1 = dynamic, a
 * cursor shared by the replicas over chunks of max_batch proofs (a slower device takes fewer chunks; at most three chunks
 * in flight per replica).  The result is index-identical either way.  rlnamd_pool_last_proofs: how many proofs of the
 * last job each replica made. */
int rlnamd_pool_set_dynamic(rlnamd_pool* p, int on);
int rlnamd_pool_last_proofs(rlnamd_pool* p, size_t* proofs_per_replica);
/* test hook: replica `replica` fails (throws inside its worker) when it is handed its after_chunks-th next chunk; one
 * shot.  The job that meets the fault returns an error naming the device, the other replicas finish their chunks, the
 * witnesses of the failed replica's in-flight chunks are wiped, and the pool stays usable. */
int rlnamd_pool_inject_fault(rlnamd_pool* p, size_t replica, size_t after_chunks);
/* Failover.  rounds = 0 (default): a failing replica fails the job as described above.  rounds > 0: everything the
 * failed replica was handed in the job (finished or not) and what it had not reached of its shard is proved again by the
 * replicas that finished, up to `rounds` times per job; the failed replica is quarantined -- later jobs are cut among the
 * others -- until rlnamd_pool_revive.  The job fails only when no replica is left or the rounds are spent; its result
 * is index-identical to a job without faults.  rlnamd_pool_health: per replica, quarantined (0 / 1) and the number of
 * dispatches that ended in an error since the pool was built (either array may be NULL). */
int rlnamd_pool_set_failover(rlnamd_pool* p, int rounds);
/* Probation.  jobs = 0 (default): a quarantined replica stays out until rlnamd_pool_revive.  jobs > 0: it sits out that
 * many jobs and is then handed work again by itself (a replica that fails again is quarantined again, its chunks go to
 * the others as before); when every replica is quarantined all of them are tried again at once instead of failing the
 * call.  Behind an FFI object (config key "failover") this is on, 8 jobs unless "revive_after" says otherwise: a caller
 * of include/rln.h has no handle on the pool.  Replica 0 of an FFI object's pool is also its single-proof prover and
 * its tree's device: calls with n <= max_batch are NOT failed over. */
int rlnamd_pool_set_probation(rlnamd_pool* p, size_t jobs);
int rlnamd_pool_health(rlnamd_pool* p, int* quarantined_per_replica, size_t* failures_per_replica);
int rlnamd_pool_revive(rlnamd_pool* p, size_t replica);
int rlnamd_pool_verify_many(rlnamd_pool* p, size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t n_values,
                            int threads, uint8_t* ok);
/* RCCL communicator for the one path with an exchange step, the config-5 MSM.  Multi-process (one process per GPU,
 * e.g. under torchrun): rank 0 calls rlnamd_comm_unique_id, the 128 bytes reach the other ranks by any means, every
 * rank calls rlnamd_comm_init_rank with its device current.  Single process: rlnamd_comm_init_all fills one
 * communicator per listed device (ncclCommInitAll; ordinals must differ). */
#define RLNAMD_COMM_ID_BYTES 128
typedef struct rlnamd_comm rlnamd_comm;
int rlnamd_comm_unique_id(uint8_t id[RLNAMD_COMM_ID_BYTES]);
int rlnamd_comm_init_rank(const uint8_t id[RLNAMD_COMM_ID_BYTES], int nranks, int rank, rlnamd_comm** out);
int rlnamd_comm_init_all(const int* devices, size_t n_devices, rlnamd_comm** out_array);
void rlnamd_comm_free(rlnamd_comm* c);
int rlnamd_comm_rank(rlnamd_comm* c);
int rlnamd_comm_ranks(rlnamd_comm* c);
/* The whole of config 5 on one rank: local Pippenger on this rank's points down to the 16 window sums, ONE
 * ncclAllGather of 2 KiB per rank over xGMI on the MSM's own stream (RCCL has no elliptic-curve reduce op: the
 * "all-reduce of bucket partials" is gather + local add), then the add + Horner fold on every rank.  Collective: every
 * rank of the communicator calls it.  ms[0] digits + sort, ms[1] buckets, ms[2] all-gather, ms[3] combine (HIP events). */
int rlnamd_msm_run_sharded(rlnamd_msm* m, rlnamd_comm* c, uint8_t out_xy_le[64], float ms[4]);
/* the same for a caller that owns several devices in one process: a thread per device, generated points
 * (rlnamd_msm_generate_mode at the rank's index range), `repeats` timed runs; ms[0..3] = max over devices of the stage times
 * of the last run, ms[4] = its wall time */
int rlnamd_msm_generated_multi(const int* devices, size_t n_devices, uint64_t seed, size_t n_total, uint32_t mode,
                               int repeats, uint8_t out_xy_le[64], float ms[5]);

#ifdef __cplusplus
}
#endif
#endif /* RLN_AMD_H */
