// C ABI of the extension surface declared in include/rln_amd.h.
#include "../../include/rln_amd.h"

#include <string.h>

#include <algorithm>
#include <atomic>
#include <system_error>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <unordered_map>

#include "arith_probe.h"
#include "common.h"
#include "keccak.h"
#include "keccak_batch.h"
#include "member_directory.h"
#include "merkle.h"
#include "msm.h"
#include "nullifier_log.h"
#include "pairing.h"
#include "poseidon.h"
#include "prover.h"
#include "relay.h"
#include "verify.h"
#include "verify_agg_scalars.h"
#include "capi_util.h"

using namespace rlnamd;

namespace rlnamd {
thread_local std::string g_last_error;
int fail(const std::exception& e) {
  g_last_error = e.what();
  return g_last_error.find("no HIP device") != std::string::npos ? RLNAMD_ERR_NO_DEVICE : RLNAMD_ERR;
}
}  // namespace rlnamd

struct rlnamd_tree {
  // every rlnamd_tree_* call on one handle takes this: the tree has ONE stream and shared scratch (proof_host's
  // staging buffer, the host chain's pinned buffers), so readers mutate object state too
  std::mutex mu;
  MerkleTreeDev t;
  size_t host_max = 0;   // rlnamd_tree_set_leaves: up to this many distinct leaves take MerkleTreeDev::set_few
  DevBuf<uint8_t> bench_elems, bench_bits;
};

struct rlnamd_directory {
  // every rlnamd_directory_* call takes this and then the tree handle's mutex, and holds both for the call: the
  // directory's passes run on the tree's stream and write the tree's leaves
  std::mutex mu;
  rlnamd_tree* tree;   // borrowed: it outlives the directory
  std::unique_ptr<MemberDirectoryDev> dir;
  rlnamd_directory(rlnamd_tree* t, uint64_t capacity, uint64_t seed) : tree(t), dir(new MemberDirectoryDev(t->t, capacity, seed)) {}
};

struct rlnamd_relay {
  // a step takes this, then the hasher's, the verifier's and the log handle's, in that order, and holds them for the
  // call; between steps the borrowed objects are usable on their own
  std::mutex mu;
  rlnamd_nullifier_log* log;
  rlnamd_hasher* hasher;
  GpuVerifier& verifier;
  RelayDev relay;
  rlnamd_relay(rlnamd_prover* p, rlnamd_nullifier_log* l, rlnamd_hasher* h, int lanes, int flags)
      : log(l), hasher(h), verifier(p->p->gpu_verifier()),
        relay(verifier, p->p->graph().max_out, l->log, h ? &h->hasher : nullptr, lanes, flags) {}
};

static void verify_common(const Zkey& zk, const uint8_t proof[128], const uint8_t* values_le, int* ok, size_t nv = 5);

extern "C" {

const char* rlnamd_last_error(void) { return rlnamd::g_last_error.c_str(); }

int rlnamd_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int rlnamd_set_device(int ordinal) {
  RLN_TRY
  RLN_HIP(hipSetDevice(ordinal));
  RLN_CATCH
}

int rlnamd_get_device(int* ordinal) {
  RLN_TRY
  RLN_HIP(hipGetDevice(ordinal));
  RLN_CATCH
}

int rlnamd_device_name(char* buf, size_t cap) {
  RLN_TRY
  require_gpu();
  int dev = 0;
  RLN_HIP(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  RLN_HIP(hipGetDeviceProperties(&prop, dev));
  std::string s = std::string(prop.name) + " (" + prop.gcnArchName + ")";
  if (cap) {
    strncpy(buf, s.c_str(), cap - 1);
    buf[cap - 1] = 0;
  }
  RLN_CATCH
}

int rlnamd_poseidon_hash(const uint8_t* inputs_le, size_t n, size_t arity, uint8_t* out_le) {
  RLN_TRY
  require_gpu();
  // PoseidonError texts of utils/src/poseidon/error.rs:4-8; widths t = 2..9 (rln/src/hashers.rs:14-23)
  if (arity == 0) throw Error("Empty input provided");
  if (arity > 8) throw Error("No parameters found for input length " + std::to_string(arity));
  if (n == 0) return RLNAMD_OK;
  for (size_t i = 0; i < n * arity; i++) {
    uint32_t tmp[8];
    memcpy(tmp, inputs_le + 32 * i, 32);
    if (limbs_geq(tmp, FrParams::MOD)) throw Error("Non-canonical field element: value is not in [0, r-1]");
  }
  DevBuf<uint8_t> din(n * arity * 32), dout(n * 32);
  RLN_HIP(hipMemcpy(din.p, inputs_le, n * arity * 32, hipMemcpyHostToDevice));
  poseidon_hash_batch_device(din.p, n, (int)arity, dout.p, 0);
  RLN_HIP(hipMemcpy(out_le, dout.p, n * 32, hipMemcpyDeviceToHost));
  RLN_CATCH
}

int rlnamd_hash_to_field_le(const uint8_t* data, size_t len, uint8_t out_le[32]) {
  RLN_TRY
  hash_to_field_le(data, len, out_le);
  RLN_CATCH
}
int rlnamd_hash_to_field_be(const uint8_t* data, size_t len, uint8_t out_le[32]) {
  RLN_TRY
  hash_to_field_be(data, len, out_le);
  RLN_CATCH
}

// ---------------------------------------------------------------------------------------------- tree
int rlnamd_tree_new(size_t depth, rlnamd_tree** out) {
  RLN_TRY
  std::unique_ptr<rlnamd_tree> h(new rlnamd_tree);
  uint8_t zero[32] = {0};
  if (depth > 30) throw Error("InvalidDepth");
  h->t.init((int)depth, zero);
  h->host_max = MerkleTreeDev::host_max_from_env();
  *out = h.release();
  RLN_CATCH
}
void rlnamd_tree_free(rlnamd_tree* t) { delete t; }

int rlnamd_tree_set_range(rlnamd_tree* t, size_t start, const uint8_t* leaves_le, size_t n) {
  RLN_TRY
  std::lock_guard<std::mutex> tree_lk(t->mu);
  for (size_t i = 0; i < n; i++) {
    uint32_t tmp[8];
    memcpy(tmp, leaves_le + 32 * i, 32);
    if (limbs_geq(tmp, FrParams::MOD)) throw Error("field element is not canonical (>= modulus)");
  }
  t->t.set_range_host(start, leaves_le, n);
  RLN_CATCH
}
int rlnamd_tree_set_leaves(rlnamd_tree* t, const uint64_t* indices, const uint8_t* leaves_le, size_t k) {
  RLN_TRY
  std::lock_guard<std::mutex> tree_lk(t->mu);
  // any order, later entries win: brought to the strictly increasing form the pass wants
  std::vector<std::pair<uint64_t, size_t>> ord(k);
  for (size_t i = 0; i < k; i++) {
    uint32_t tmp[8];
    memcpy(tmp, leaves_le + 32 * i, 32);
    if (limbs_geq(tmp, FrParams::MOD)) throw Error("field element is not canonical (>= modulus)");
    if (indices[i] >= t->t.capacity()) throw Error("TooManySet");
    ord[i] = {indices[i], i};
  }
  std::stable_sort(ord.begin(), ord.end(), [](const std::pair<uint64_t, size_t>& a, const std::pair<uint64_t, size_t>& b) { return a.first < b.first; });
  std::vector<uint64_t> idx;
  std::vector<uint8_t> leaves;
  for (size_t i = 0; i < k; i++) {
    if (i + 1 < k && ord[i + 1].first == ord[i].first) continue;   // the last write to an index wins
    idx.push_back(ord[i].first);
    leaves.insert(leaves.end(), leaves_le + 32 * ord[i].second, leaves_le + 32 * ord[i].second + 32);
  }
  if (idx.size() <= t->host_max) t->t.set_few(idx.data(), leaves.data(), idx.size());
  else t->t.set_scattered(idx.data(), leaves.data(), idx.size());
  RLN_HIP(hipStreamSynchronize(t->t.stream));
  RLN_CATCH
}
int rlnamd_tree_root(rlnamd_tree* t, uint8_t out_le[32]) {
  RLN_TRY
  std::lock_guard<std::mutex> tree_lk(t->mu);
  t->t.get_node_host(0, out_le);
  RLN_CATCH
}
int rlnamd_tree_get_leaf(rlnamd_tree* t, size_t index, uint8_t out_le[32]) {
  RLN_TRY
  std::lock_guard<std::mutex> tree_lk(t->mu);
  if (index >= t->t.capacity()) throw Error("InvalidLeaf");
  t->t.get_node_host(t->t.capacity() - 1 + index, out_le);
  RLN_CATCH
}
int rlnamd_tree_proof(rlnamd_tree* t, size_t index, uint8_t* elems_le, uint8_t* bits) {
  RLN_TRY
  std::lock_guard<std::mutex> tree_lk(t->mu);
  t->t.proof_host(index, elems_le, bits);
  RLN_CATCH
}
int rlnamd_tree_proofs(rlnamd_tree* t, size_t first, size_t count, uint8_t* elems_le, uint8_t* bits) {
  RLN_TRY
  std::lock_guard<std::mutex> tree_lk(t->mu);
  if (count == 0 || t->t.depth == 0) return RLNAMD_OK;
  size_t d = t->t.depth;
  DevBuf<uint8_t> e(count * d * 32), b(count * d);
  t->t.proofs_device(first, count, e.p, b.p);
  RLN_HIP(hipMemcpyAsync(elems_le, e.p, count * d * 32, hipMemcpyDeviceToHost, t->t.stream));
  RLN_HIP(hipMemcpyAsync(bits, b.p, count * d, hipMemcpyDeviceToHost, t->t.stream));
  RLN_HIP(hipStreamSynchronize(t->t.stream));
  RLN_CATCH
}
int rlnamd_tree_proofs_at(rlnamd_tree* t, const uint64_t* indices, size_t k, uint8_t* elems_le, uint8_t* bits) {
  RLN_TRY
  std::lock_guard<std::mutex> tree_lk(t->mu);
  if (k == 0) return RLNAMD_OK;
  if (!indices || !elems_le || !bits) throw Error("rlnamd_tree_proofs_at: null pointer");
  t->t.proofs_at_host(indices, k, elems_le, bits);
  RLN_CATCH
}
int rlnamd_tree_fill_sequential(rlnamd_tree* t, size_t start, size_t n, uint64_t first_value) {
  RLN_TRY
  std::lock_guard<std::mutex> tree_lk(t->mu);
  t->t.fill_sequential_device(start, n, first_value);
  RLN_HIP(hipStreamSynchronize(t->t.stream));
  RLN_CATCH
}
int rlnamd_tree_bench(rlnamd_tree* t, size_t n_leaves, uint64_t first_value, int verify, float ms[2], size_t* bad) {
  RLN_TRY
  std::lock_guard<std::mutex> tree_lk(t->mu);
  MerkleTreeDev& T = t->t;
  if (n_leaves > T.capacity()) throw Error("TooManySet");
  size_t d = T.depth;
  if (t->bench_elems.n < n_leaves * d * 32) t->bench_elems.alloc(n_leaves * d * 32);
  if (t->bench_bits.n < n_leaves * d) t->bench_bits.alloc(n_leaves * d);
  hipEvent_t e0, e1, e2;
  RLN_HIP(hipEventCreate(&e0));
  RLN_HIP(hipEventCreate(&e1));
  RLN_HIP(hipEventCreate(&e2));
  RLN_HIP(hipEventRecord(e0, T.stream));
  T.fill_sequential_device(0, n_leaves, first_value);
  RLN_HIP(hipEventRecord(e1, T.stream));
  T.proofs_device(0, n_leaves, t->bench_elems.p, t->bench_bits.p);
  RLN_HIP(hipEventRecord(e2, T.stream));
  RLN_HIP(hipStreamSynchronize(T.stream));
  RLN_HIP(hipEventElapsedTime(&ms[0], e0, e1));
  RLN_HIP(hipEventElapsedTime(&ms[1], e1, e2));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipEventDestroy(e2);
  if (bad) *bad = verify ? T.verify_proofs_device(0, n_leaves, t->bench_elems.p, t->bench_bits.p) : 0;
  RLN_CATCH
}

// ------------------------------------------------------------------------------------ nullifier log
int rlnamd_nullifier_log_new(size_t capacity, uint64_t seed, rlnamd_nullifier_log** out) {
  RLN_TRY
  if (!out) throw Error("rlnamd_nullifier_log_new: null pointer");
  *out = new rlnamd_nullifier_log(capacity, seed);
  RLN_CATCH
}
void rlnamd_nullifier_log_free(rlnamd_nullifier_log* l) { delete l; }
int rlnamd_nullifier_log_observe(rlnamd_nullifier_log* l, size_t n, const uint8_t* shares_le, const uint64_t* tags,
                                 uint8_t* status, uint8_t* secrets_le, uint64_t* first_tag) {
  RLN_TRY
  if (!l) throw Error("rlnamd_nullifier_log_observe: null log");
  std::lock_guard<std::mutex> lk(l->mu);
  l->log.observe(n, shares_le, tags, status, secrets_le, first_tag);
  RLN_CATCH
}
int rlnamd_nullifier_log_clear(rlnamd_nullifier_log* l) {
  RLN_TRY
  if (!l) throw Error("rlnamd_nullifier_log_clear: null log");
  std::lock_guard<std::mutex> lk(l->mu);
  l->log.clear();
  RLN_CATCH
}
int rlnamd_nullifier_log_retire(rlnamd_nullifier_log* l, const uint8_t* external_nullifiers_le, size_t k, uint64_t* removed) {
  RLN_TRY
  if (!l) throw Error("rlnamd_nullifier_log_retire: null log");
  std::lock_guard<std::mutex> lk(l->mu);
  const uint64_t gone = l->log.retire(k, external_nullifiers_le);
  if (removed) *removed = gone;
  RLN_CATCH
}
int rlnamd_nullifier_log_retain(rlnamd_nullifier_log* l, const uint8_t* external_nullifiers_le, size_t k, uint64_t* removed) {
  RLN_TRY
  // what needs no object is checked before the handle is followed
  const std::string refused = nlog::retain_refusal(external_nullifiers_le, k);
  if (!refused.empty()) throw Error(refused);
  if (!l) throw Error("rlnamd_nullifier_log_retain: null log");
  std::lock_guard<std::mutex> lk(l->mu);
  const uint64_t gone = l->log.retain(k, external_nullifiers_le);
  if (removed) *removed = gone;
  RLN_CATCH
}
int rlnamd_nullifier_log_retire_info(rlnamd_nullifier_log* l, uint64_t out[8]) {
  RLN_TRY
  if (!l || !out) throw Error("rlnamd_nullifier_log_retire_info: null pointer");
  std::lock_guard<std::mutex> lk(l->mu);
  l->log.retire_info(out);
  RLN_CATCH
}
int rlnamd_nullifier_log_get(rlnamd_nullifier_log* l, uint64_t seq, uint8_t share_le[128], uint64_t* tag) {
  RLN_TRY
  if (!l) throw Error("rlnamd_nullifier_log_get: null log");
  std::lock_guard<std::mutex> lk(l->mu);
  l->log.get(seq, share_le, tag);
  RLN_CATCH
}
int rlnamd_nullifier_log_home_slot(rlnamd_nullifier_log* l, const uint8_t nullifier_le[32], uint64_t* slot) {
  RLN_TRY
  if (!l || !nullifier_le || !slot) throw Error("rlnamd_nullifier_log_home_slot: null pointer");
  *slot = l->log.home_slot(nullifier_le);
  RLN_CATCH
}
int rlnamd_nullifier_log_info(rlnamd_nullifier_log* l, uint64_t out[8]) {
  RLN_TRY
  if (!l || !out) throw Error("rlnamd_nullifier_log_info: null pointer");
  std::lock_guard<std::mutex> lk(l->mu);
  l->log.info(out);
  RLN_CATCH
}

// --------------------------------------------------------------------------------- member directory
// What needs no object is checked before the handle is followed (without one the bound of an index is the largest a
// directory can have).  Lock order: the directory's mutex, then the tree handle's; nothing takes them the other way round
// (the relay's order -- relay, hasher, verifier, log -- and the proving calls' -- tree, then ledger -- do not meet these two).
#define RLN_DIR_REFUSE(text)                     \
  {                                              \
    const std::string refused_ = (text);         \
    if (!refused_.empty()) throw Error(refused_); \
  }
#define RLN_DIR_LOCK(d)                              \
  std::lock_guard<std::mutex> dir_lk((d)->mu);       \
  std::lock_guard<std::mutex> tree_lk((d)->tree->mu)
int rlnamd_directory_new(rlnamd_tree* tree, size_t capacity, uint64_t seed, rlnamd_directory** out) {
  RLN_TRY
  RLN_DIR_REFUSE(mdir::new_refusal(capacity, tree ? (uint64_t)tree->t.depth : 63));
  if (!tree || !out) throw Error("rlnamd_directory_new: null pointer");
  std::lock_guard<std::mutex> tree_lk(tree->mu);
  *out = new rlnamd_directory(tree, capacity, seed);
  RLN_CATCH
}
void rlnamd_directory_free(rlnamd_directory* d) {
  if (!d) return;
  {
    RLN_DIR_LOCK(d);   // (the staging is released on the tree's stream)
    d->dir.reset();
  }
  delete d;
}
int rlnamd_directory_register(rlnamd_directory* d, size_t n, const uint64_t* indices, const uint8_t* idcs_le, const uint32_t* limits,
                              uint8_t* status) {
  RLN_TRY
  RLN_DIR_REFUSE(mdir::register_refusal(n, indices, idcs_le, limits, status, d ? d->dir->capacity() : mdir::MAX_CAPACITY));
  if (!d) throw Error("rlnamd_directory_register: null directory");
  RLN_DIR_LOCK(d);
  d->dir->do_register(n, indices, idcs_le, limits, status);
  RLN_CATCH
}
int rlnamd_directory_find(rlnamd_directory* d, size_t n, const uint8_t* idcs_le, uint8_t* status, uint64_t* index, uint32_t* limit) {
  RLN_TRY
  RLN_DIR_REFUSE(mdir::find_refusal(n, idcs_le, status, index, limit));
  if (!d) throw Error("rlnamd_directory_find: null directory");
  RLN_DIR_LOCK(d);
  d->dir->find(n, idcs_le, status, index, limit);
  RLN_CATCH
}
int rlnamd_directory_resolve(rlnamd_directory* d, size_t n, const uint8_t* secrets_le, const uint8_t* take, uint8_t* status,
                             uint64_t* index, uint32_t* limit) {
  RLN_TRY
  RLN_DIR_REFUSE(mdir::resolve_refusal("resolve", n, secrets_le, take, status, index, limit));
  if (!d) throw Error("rlnamd_directory_resolve: null directory");
  RLN_DIR_LOCK(d);
  d->dir->resolve(n, secrets_le, take, status, index, limit);
  RLN_CATCH
}
int rlnamd_directory_slash(rlnamd_directory* d, size_t n, const uint8_t* secrets_le, const uint8_t* take, uint8_t* status,
                           uint64_t* index, uint32_t* limit, uint64_t* removed) {
  RLN_TRY
  RLN_DIR_REFUSE(mdir::resolve_refusal("slash", n, secrets_le, take, status, index, limit));
  if (!d) throw Error("rlnamd_directory_slash: null directory");
  RLN_DIR_LOCK(d);
  d->dir->slash(n, secrets_le, take, status, index, limit, removed);
  RLN_CATCH
}
int rlnamd_directory_remove(rlnamd_directory* d, size_t n, const uint64_t* indices, uint8_t* status) {
  RLN_TRY
  RLN_DIR_REFUSE(mdir::remove_refusal(n, indices, status, d ? d->dir->capacity() : mdir::MAX_CAPACITY));
  if (!d) throw Error("rlnamd_directory_remove: null directory");
  RLN_DIR_LOCK(d);
  d->dir->remove(n, indices, status);
  RLN_CATCH
}
int rlnamd_directory_get(rlnamd_directory* d, size_t n, const uint64_t* indices, uint8_t* live, uint8_t* idcs_le, uint32_t* limits) {
  RLN_TRY
  RLN_DIR_REFUSE(mdir::get_refusal(n, indices, live, idcs_le, limits, d ? d->dir->capacity() : mdir::MAX_CAPACITY));
  if (!d) throw Error("rlnamd_directory_get: null directory");
  RLN_DIR_LOCK(d);
  d->dir->get(n, indices, live, idcs_le, limits);
  RLN_CATCH
}
int rlnamd_directory_info(rlnamd_directory* d, uint64_t out[8]) {
  RLN_TRY
  if (!d || !out) throw Error("rlnamd_directory_info: null pointer");
  RLN_DIR_LOCK(d);
  d->dir->info(out);
  RLN_CATCH
}

// ------------------------------------------------------------------------------------------- hasher
int rlnamd_hasher_new(size_t stage_bytes, size_t lane_max_blocks, rlnamd_hasher** out) {
  RLN_TRY
  if (!out) throw Error("rlnamd_hasher_new: null pointer");
  *out = new rlnamd_hasher(stage_bytes, lane_max_blocks);
  RLN_CATCH
}
void rlnamd_hasher_free(rlnamd_hasher* h) { delete h; }
int rlnamd_hasher_hash_to_field(rlnamd_hasher* h, const uint8_t* data, size_t data_len, const uint64_t* offsets, size_t n,
                                uint8_t* out_le) {
  RLN_TRY
  if (!h) throw Error("rlnamd_hasher_hash_to_field: null hasher");
  std::lock_guard<std::mutex> lk(h->mu);
  h->hasher.hash_to_field(data, data_len, offsets, n, out_le);
  RLN_CATCH
}
int rlnamd_hasher_info(rlnamd_hasher* h, uint64_t out[8]) {
  RLN_TRY
  if (!h || !out) throw Error("rlnamd_hasher_info: null pointer");
  std::lock_guard<std::mutex> lk(h->mu);
  h->hasher.info(out);
  RLN_CATCH
}

// -------------------------------------------------------------------------------------------- relay
static_assert(RLNAMD_RELAY_OPTIMISTIC == RelayDev::OPTIMISTIC && RLNAMD_RELAY_OPTIMISTIC_TEAMS == RelayDev::OPTIMISTIC_TEAMS,
              "the relay's flags");
int rlnamd_relay_new(rlnamd_prover* p, rlnamd_nullifier_log* log, rlnamd_hasher* h, int lanes, rlnamd_relay** out) {
  RLN_TRY
  if (!p || !log || !out) throw Error("rlnamd_relay_new: null pointer");
  if (lanes != 0 && lanes != 1 && lanes != 8) throw Error("rlnamd_relay_new: lanes must be 0, 1 or 8");
  *out = new rlnamd_relay(p, log, h, lanes, 0);
  RLN_CATCH
}
int rlnamd_relay_new_ex(rlnamd_prover* p, rlnamd_nullifier_log* log, rlnamd_hasher* h, int lanes, int flags, rlnamd_relay** out) {
  RLN_TRY
  // the flags need no object and no device: they are judged first
  if (const int unknown = flags & ~(RLNAMD_RELAY_OPTIMISTIC | RLNAMD_RELAY_OPTIMISTIC_TEAMS))
    throw Error("rlnamd_relay_new_ex: unknown flag bits " + std::to_string(unknown) + " in flags " + std::to_string(flags));
  if (const char* refused = RelayDev::check_flags(flags)) throw Error(std::string("rlnamd_relay_new_ex: ") + refused);
  if (!p || !log || !out) throw Error("rlnamd_relay_new_ex: null pointer");
  if (lanes != 0 && lanes != 1 && lanes != 8) throw Error("rlnamd_relay_new_ex: lanes must be 0, 1 or 8");
  *out = new rlnamd_relay(p, log, h, lanes, flags);
  RLN_CATCH
}
void rlnamd_relay_free(rlnamd_relay* r) { delete r; }
int rlnamd_relay_step(rlnamd_relay* r, size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t n_values,
                      const uint8_t* signals, size_t signals_len, const uint64_t* offsets, const uint8_t* xs_le,
                      const uint8_t* roots_le, size_t n_roots, const uint64_t* tags, uint8_t* verdict, uint8_t* status,
                      uint8_t* secrets_le, uint64_t* first_tag) {
  RLN_TRY
  // what needs no object is checked before the handle is followed
  if (const char* refused = relay::check_arguments(n, proofs, values_le, signals, offsets, xs_le, roots_le, n_roots, verdict, status))
    throw Error(refused);
  if (!r) throw Error("rlnamd_relay_step: null relay");
  if (n == 0) return RLNAMD_OK;
  std::lock_guard<std::mutex> lk(r->mu);
  std::unique_lock<std::mutex> lk_hasher;
  if (r->hasher) lk_hasher = std::unique_lock<std::mutex>(r->hasher->mu);
  std::lock_guard<std::mutex> lk_verifier(r->verifier.relay_mutex());
  std::lock_guard<std::mutex> lk_log(r->log->mu);
  r->relay.step(n, proofs, values_le, n_values, signals, signals_len, offsets, xs_le, roots_le, n_roots, tags, verdict, status,
                secrets_le, first_tag);
  RLN_CATCH
}
static_assert(RLNAMD_RELAY_EPOCHS_MAX == relay::EPOCHS_MAX && RLNAMD_RELAY_EPOCHS_MAX == RLNAMD_LOG_RETIRE_MAX &&
                  RLNAMD_RELAY_BAD_EPOCH == relay::BAD_EPOCH,
              "the relay's window");
int rlnamd_relay_set_epochs(rlnamd_relay* r, const uint8_t* external_nullifiers_le, size_t k, uint64_t* removed) {
  RLN_TRY
  // what needs no object is checked before the handle is followed
  const std::string refused = relay::epochs_refusal(external_nullifiers_le, k);
  if (!refused.empty()) throw Error(refused);
  if (!r) throw Error("rlnamd_relay_set_epochs: null relay");
  std::lock_guard<std::mutex> lk(r->mu);
  std::lock_guard<std::mutex> lk_log(r->log->mu);   // the step's order: the relay's, then the log's
  const uint64_t gone = r->relay.set_epochs(k, external_nullifiers_le);
  if (removed) *removed = gone;
  RLN_CATCH
}
int rlnamd_relay_epochs(rlnamd_relay* r, uint8_t* out_le, size_t* k) {
  RLN_TRY
  if (!r || !out_le || !k) throw Error("rlnamd_relay_epochs: null pointer");
  std::lock_guard<std::mutex> lk(r->mu);
  *k = r->relay.epochs(out_le);
  RLN_CATCH
}
int rlnamd_relay_info(rlnamd_relay* r, uint64_t out[8]) {
  RLN_TRY
  if (!r || !out) throw Error("rlnamd_relay_info: null pointer");
  std::lock_guard<std::mutex> lk(r->mu);
  std::lock_guard<std::mutex> lk_log(r->log->mu);   // the residue is read on the log's stream
  r->relay.info(out);
  RLN_CATCH
}

// ------------------------------------------------------------------------------------- quota ledger
static_assert(RLNAMD_QUOTA_OK == quota::OK && RLNAMD_QUOTA_OVER == quota::OVER && RLNAMD_QUOTA_NO_EPOCH == quota::NO_EPOCH &&
                  RLNAMD_RELAY_EPOCHS_MAX == quota::EPOCHS_MAX && RLNAMD_QUOTA_COUNT_MAX == quota::COUNT_MAX,
              "the ledger's statuses and window");
int rlnamd_quota_new(size_t depth, size_t max_epochs, rlnamd_quota** out) {
  RLN_TRY
  // what needs no device is checked before one is asked for
  const std::string refused = quota::new_refusal(depth, max_epochs);
  if (!refused.empty()) throw Error(refused);
  if (!out) throw Error("rlnamd_quota_new: null pointer");
  *out = new rlnamd_quota(depth, max_epochs);
  RLN_CATCH
}
int rlnamd_quota_open(const char* dir, size_t depth, size_t max_epochs, uint64_t journal_max_bytes, rlnamd_quota** out) {
  RLN_TRY
  // what needs no device is checked before one is asked for: the shape, and then the whole store (quota_store.h)
  const std::string refused = quota::new_refusal(depth, max_epochs);
  if (!refused.empty()) throw Error(refused);
  if (!out || !dir) throw Error("rlnamd_quota_open: null pointer");
  *out = new rlnamd_quota(dir, depth, max_epochs, journal_max_bytes);
  RLN_CATCH
}
int rlnamd_quota_compact(rlnamd_quota* q) {
  RLN_TRY
  if (!q) throw Error("rlnamd_quota_compact: null ledger");
  std::lock_guard<std::mutex> lk(q->mu);
  q->ledger.compact();
  RLN_CATCH
}
int rlnamd_quota_store_info(rlnamd_quota* q, uint64_t out[8]) {
  RLN_TRY
  if (!q || !out) throw Error("rlnamd_quota_store_info: null pointer");
  std::lock_guard<std::mutex> lk(q->mu);
  q->ledger.store_info(out);
  RLN_CATCH
}
void rlnamd_quota_free(rlnamd_quota* q) { delete q; }   // (a ledger with a store compacts, then closes: quota_ledger.hip)
int rlnamd_quota_set_epochs(rlnamd_quota* q, const uint8_t* external_nullifiers_le, size_t k) {
  RLN_TRY
  // what needs no object is judged without one (the ledger judges the same with its own max_epochs, before it enqueues)
  if (!q) {
    const std::string refused = quota::epochs_refusal(external_nullifiers_le, k, quota::EPOCHS_MAX);
    throw Error(refused.empty() ? "rlnamd_quota_set_epochs: null ledger" : refused);
  }
  std::lock_guard<std::mutex> lk(q->mu);
  q->ledger.set_epochs(k, external_nullifiers_le);
  RLN_CATCH
}
int rlnamd_quota_epochs(rlnamd_quota* q, uint8_t* out_le, size_t* k) {
  RLN_TRY
  if (!q || !out_le || !k) throw Error("rlnamd_quota_epochs: null pointer");
  std::lock_guard<std::mutex> lk(q->mu);
  *k = q->ledger.epochs(out_le);
  RLN_CATCH
}
int rlnamd_quota_draw(rlnamd_quota* q, size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le, const uint32_t* limits,
                      uint32_t* ids_out, uint8_t* status) {
  RLN_TRY
  // what needs no object is judged without one (the ledger judges the same with its own depth, before it enqueues)
  if (!q) {
    const std::string refused = quota::draw_refusal(n, leaf_indices, ext_le, limits, ids_out, status, quota::DEPTH_MAX);
    throw Error(refused.empty() ? "rlnamd_quota_draw: null ledger" : refused);
  }
  std::lock_guard<std::mutex> lk(q->mu);
  q->ledger.draw(n, leaf_indices, ext_le, limits, ids_out, status);
  RLN_CATCH
}
int rlnamd_quota_draw_counts(rlnamd_quota* q, size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le, const uint32_t* limits,
                             const uint8_t* counts, uint32_t* firsts_out, uint8_t* status) {
  RLN_TRY
  // what needs no object is judged without one (the ledger judges the same with its own depth, before it enqueues)
  if (!q) {
    const std::string refused = quota::draw_counts_refusal(n, leaf_indices, ext_le, limits, counts, firsts_out, status, quota::DEPTH_MAX);
    throw Error(refused.empty() ? "rlnamd_quota_draw_counts: null ledger" : refused);
  }
  std::lock_guard<std::mutex> lk(q->mu);
  q->ledger.draw_counts(n, leaf_indices, ext_le, limits, counts, firsts_out, status);
  RLN_CATCH
}
int rlnamd_quota_used(rlnamd_quota* q, size_t n, const uint64_t* leaf_indices, const uint8_t* ext_le, uint32_t* used_out,
                      uint8_t* in_window) {
  RLN_TRY
  if (!q) throw Error("rlnamd_quota_used: null ledger");
  std::lock_guard<std::mutex> lk(q->mu);
  q->ledger.used(n, leaf_indices, ext_le, used_out, in_window);
  RLN_CATCH
}
int rlnamd_quota_info(rlnamd_quota* q, uint64_t out[8]) {
  RLN_TRY
  if (!q || !out) throw Error("rlnamd_quota_info: null pointer");
  std::lock_guard<std::mutex> lk(q->mu);
  q->ledger.info(out);
  RLN_CATCH
}
int rlnamd_quota_plan(size_t n, size_t depth, uint64_t out[4]) {
  RLN_TRY
  if (!out) throw Error("rlnamd_quota_plan: null pointer");
  if (depth < 1 || depth > quota::DEPTH_MAX) throw Error(quota::new_refusal(depth, 1));
  const quota::DrawPlan P = quota::plan_for(n, (uint32_t)depth);
  out[0] = P.passes;
  out[1] = P.blocks;
  out[2] = P.bin_levels;
  out[3] = P.rank_levels;
  RLN_CATCH
}

// -------------------------------------------------------------------------------------------- prover
int rlnamd_prover_new(const uint8_t* zkey, size_t zkey_len, const uint8_t* graph, size_t graph_len, size_t max_batch,
                      int window_bits, rlnamd_prover** out) {
  RLN_TRY
  ProverConfig cfg;
  cfg.max_batch = max_batch ? max_batch : 64;
  cfg.window_bits = window_bits;
  std::unique_ptr<rlnamd_prover> h(new rlnamd_prover);
  h->p.reset(new Prover(zkey, zkey_len, graph, graph_len, cfg));
  *out = h.release();
  RLN_CATCH
}
void rlnamd_prover_free(rlnamd_prover* p) { delete p; }

int rlnamd_prover_get_info(rlnamd_prover* p, rlnamd_prover_info* info) {
  RLN_TRY
  rlnamd::fill_prover_info(*p->p, info);
  RLN_CATCH
}
}  // extern "C"
namespace rlnamd {
void fill_prover_info(const Prover& P, rlnamd_prover_info* info) {
  info->inputs_size = P.inputs_per_proof();
  info->num_signals = P.graph().signals.size();
  uint64_t dom = 1;
  while (dom < P.zkey().num_constraints + P.zkey().num_instance_variables) dom <<= 1;
  info->domain_size = dom;
  info->tree_depth = P.graph().tree_depth;
  info->max_out = P.graph().max_out;
  info->capacity = P.capacity();
  info->table_bytes = P.table_bytes();
  info->window_bits = P.window_bits();
  info->windows = P.windows();
  info->window_bits_g2 = P.window_bits_g2();
  info->windows_g2 = P.windows_g2();
  info->glv = 1;   // the walks always take the GLV split
  info->reserved = 0;
  info->g1_rows = P.g1_rows();
  info->g2_rows = P.g2_rows();
}
}  // namespace rlnamd
extern "C" {
int rlnamd_prover_input_slot(rlnamd_prover* p, const char* name, uint32_t* offset, uint32_t* len) {
  RLN_TRY
  auto& m = p->p->graph().input_mapping;
  auto it = m.find(name);
  if (it == m.end()) throw Error(std::string("MissingInput: ") + name);
  *offset = it->second.first;
  *len = it->second.second;
  RLN_CATCH
}
int rlnamd_prover_upload(rlnamd_prover* p, size_t n, const uint8_t* inputs_le, const uint8_t* rs_le) {
  RLN_TRY
  p->p->upload(n, inputs_le, rs_le);
  RLN_CATCH
}
int rlnamd_prover_run(rlnamd_prover* p, size_t n) {
  RLN_TRY
  p->p->run(n);
  RLN_CATCH
}
int rlnamd_prover_run_async(rlnamd_prover* p, size_t n) {
  RLN_TRY
  p->p->run_async(n);
  RLN_CATCH
}
int rlnamd_prover_sync(rlnamd_prover* p) {
  RLN_TRY
  p->p->sync();
  RLN_CATCH
}
int rlnamd_prover_slots(rlnamd_prover* p) { return p->p->slots(); }
int rlnamd_prover_submit(rlnamd_prover* p, size_t n, const uint8_t* inputs_le, const uint8_t* rs_le, int mode,
                         const uint8_t* partial320, uint64_t* ticket) {
  RLN_TRY
  *ticket = p->p->submit(n, inputs_le, rs_le, mode, partial320);
  RLN_CATCH
}
int rlnamd_prover_collect(rlnamd_prover* p, uint64_t ticket, size_t n, uint8_t* proofs, uint8_t* coords, uint8_t* values,
                          uint32_t* errors, uint8_t* partial320) {
  RLN_TRY
  p->p->collect(ticket, n, proofs, values, errors, coords, partial320);
  RLN_CATCH
}
uint32_t rlnamd_prover_hint_words(rlnamd_prover* p) { return p->p->hint_words(); }
int rlnamd_prover_hints_for(rlnamd_prover* p, const uint8_t* inputs_le, uint32_t* hints) {
  RLN_TRY
  p->p->hints_for(inputs_le, hints);
  RLN_CATCH
}
int rlnamd_prover_submit_hinted(rlnamd_prover* p, size_t n, const uint8_t* inputs_le, const uint8_t* rs_le,
                                const uint32_t* hints, uint64_t* ticket) {
  RLN_TRY
  *ticket = p->p->submit_hinted(n, inputs_le, rs_le, hints);
  RLN_CATCH
}
int rlnamd_prover_hint_stats(rlnamd_prover* p, uint64_t out[7]) {
  RLN_TRY
  static_assert(Prover::HINT_STATS_FIELDS == 7, "rln_amd.h states seven fields");
  p->p->hint_stats(out);
  RLN_CATCH
}
int rlnamd_prover_device_shared(rlnamd_prover* p, int* who) {
  RLN_TRY
  *who = p->p->device_shared();
  RLN_CATCH
}
int rlnamd_prover_collect_partial_cached(rlnamd_prover* p, uint64_t ticket, size_t n, uint8_t* partial320, uint64_t* handles,
                                         uint32_t* errors) {
  RLN_TRY
  p->p->collect_partial_cached(ticket, n, partial320, handles, errors);
  RLN_CATCH
}
int rlnamd_prover_submit_finish(rlnamd_prover* p, size_t n, const uint8_t* inputs_le, const uint8_t* rs_le,
                                const uint8_t* partial320, const uint64_t* handles, uint64_t* ticket) {
  RLN_TRY
  *ticket = p->p->submit_finish(n, inputs_le, rs_le, partial320, handles);
  RLN_CATCH
}
int rlnamd_prover_release_partial(rlnamd_prover* p, const uint64_t* handles, size_t n) {
  RLN_TRY
  p->p->release_partial(handles, n);
  RLN_CATCH
}
int rlnamd_prover_partial_cache_info(rlnamd_prover* p, uint64_t out[8]) {
  RLN_TRY
  static_assert(Prover::PARTIAL_CACHE_FIELDS == 8, "rln_amd.h states eight fields");
  p->p->partial_cache_info(out);
  RLN_CATCH
}
int rlnamd_prover_collect_public(rlnamd_prover* p, uint64_t ticket, size_t n, uint8_t* out_le) {
  RLN_TRY
  std::vector<uint8_t> v;
  p->p->collect_public(ticket, n, &v);
  memcpy(out_le, v.data(), v.size());
  RLN_CATCH
}
int rlnamd_prover_prove_stream(rlnamd_prover* p, size_t n, const uint8_t* inputs_le, const uint8_t* rs_le,
                               uint8_t* proofs, uint8_t* values, uint32_t* errors) {
  RLN_TRY
  p->p->prove_stream(n, inputs_le, rs_le, proofs, values, errors);
  RLN_CATCH
}
// (the tree's lock is held from the gather's first event to its last: see Prover::submit_members)
static MemberTree member_tree(rlnamd_tree* t) {
  MemberTree mt;
  mt.dense = &t->t;
  mt.depth = t->t.depth;
  return mt;
}
int rlnamd_prover_submit_members(rlnamd_prover* p, rlnamd_tree* t, size_t n, const uint64_t* leaf_indices,
                                 const uint8_t* inputs_le, const uint8_t* rs_le, int mode, uint64_t* ticket) {
  RLN_TRY
  if (!p || !t || !ticket) throw Error("rlnamd_prover_submit_members: null pointer");
  std::lock_guard<std::mutex> tree_lk(t->mu);
  *ticket = p->p->submit_members(member_tree(t), n, leaf_indices, inputs_le, rs_le, mode);
  RLN_CATCH
}
int rlnamd_prover_prove_stream_members(rlnamd_prover* p, rlnamd_tree* t, size_t n, const uint64_t* leaf_indices,
                                       const uint8_t* inputs_le, const uint8_t* rs_le, uint8_t* proofs, uint8_t* values,
                                       uint32_t* errors) {
  RLN_TRY
  if (!p || !t) throw Error("rlnamd_prover_prove_stream_members: null pointer");
  std::lock_guard<std::mutex> tree_lk(t->mu);
  p->p->prove_stream_members(member_tree(t), n, leaf_indices, inputs_le, rs_le, proofs, values, errors);
  RLN_CATCH
}
// (lock order: the tree's, then the ledger's; both are held from the draw to the wipe of its block)
int rlnamd_prover_submit_members_drawn(rlnamd_prover* p, rlnamd_tree* t, rlnamd_quota* q, size_t n, const uint64_t* leaf_indices,
                                       const uint8_t* inputs_le, const uint8_t* rs_le, uint8_t* status, uint64_t* ticket) {
  RLN_TRY
  if (!p || !t || !q || !ticket) throw Error("rlnamd_prover_submit_members_drawn: null pointer");
  std::lock_guard<std::mutex> tree_lk(t->mu);
  std::lock_guard<std::mutex> quota_lk(q->mu);
  *ticket = p->p->submit_members_drawn(member_tree(t), q->ledger, n, leaf_indices, inputs_le, rs_le, status);
  RLN_CATCH
}
int rlnamd_prover_prove_stream_members_drawn(rlnamd_prover* p, rlnamd_tree* t, rlnamd_quota* q, size_t n, const uint64_t* leaf_indices,
                                             const uint8_t* inputs_le, const uint8_t* rs_le, uint8_t* status, uint8_t* proofs,
                                             uint8_t* values, uint32_t* errors) {
  RLN_TRY
  if (!p || !t || !q) throw Error("rlnamd_prover_prove_stream_members_drawn: null pointer");
  std::lock_guard<std::mutex> tree_lk(t->mu);
  std::lock_guard<std::mutex> quota_lk(q->mu);
  p->p->prove_stream_members_drawn(member_tree(t), q->ledger, n, leaf_indices, inputs_le, rs_le, status, proofs, values, errors);
  RLN_CATCH
}
int rlnamd_prover_submit_members_drawn_counts(rlnamd_prover* p, rlnamd_tree* t, rlnamd_quota* q, size_t n, const uint64_t* leaf_indices,
                                              const uint8_t* inputs_le, const uint8_t* rs_le, const uint8_t* counts, uint8_t* status,
                                              uint64_t* ticket) {
  RLN_TRY
  if (!p || !t || !q || !ticket) throw Error("rlnamd_prover_submit_members_drawn_counts: null pointer");
  std::lock_guard<std::mutex> tree_lk(t->mu);
  std::lock_guard<std::mutex> quota_lk(q->mu);
  *ticket = p->p->submit_members_drawn_counts(member_tree(t), q->ledger, n, leaf_indices, inputs_le, rs_le, counts, status);
  RLN_CATCH
}
int rlnamd_prover_prove_stream_members_drawn_counts(rlnamd_prover* p, rlnamd_tree* t, rlnamd_quota* q, size_t n,
                                                    const uint64_t* leaf_indices, const uint8_t* inputs_le, const uint8_t* rs_le,
                                                    const uint8_t* counts, uint8_t* status, uint8_t* proofs, uint8_t* values_public,
                                                    uint32_t* errors) {
  RLN_TRY
  if (!p || !t || !q) throw Error("rlnamd_prover_prove_stream_members_drawn_counts: null pointer");
  std::lock_guard<std::mutex> tree_lk(t->mu);
  std::lock_guard<std::mutex> quota_lk(q->mu);
  p->p->prove_stream_members_drawn_counts(member_tree(t), q->ledger, n, leaf_indices, inputs_le, rs_le, counts, status, proofs,
                                          values_public, errors);
  RLN_CATCH
}
int rlnamd_prover_prove_stream_members_public(rlnamd_prover* p, rlnamd_tree* t, size_t n, const uint64_t* leaf_indices,
                                              const uint8_t* inputs_le, const uint8_t* rs_le, uint8_t* proofs, uint8_t* values_public,
                                              uint32_t* errors) {
  RLN_TRY
  if (!p || !t) throw Error("rlnamd_prover_prove_stream_members_public: null pointer");
  std::lock_guard<std::mutex> tree_lk(t->mu);
  p->p->prove_stream_members_public(member_tree(t), n, leaf_indices, inputs_le, rs_le, proofs, values_public, errors);
  RLN_CATCH
}
int rlnamd_prover_run_mode(rlnamd_prover* p, size_t n, int mode) {
  RLN_TRY
  p->p->run(n, mode);
  RLN_CATCH
}
int rlnamd_prover_run_async_mode(rlnamd_prover* p, size_t n, int mode) {
  RLN_TRY
  p->p->run_async(n, mode);
  RLN_CATCH
}
int rlnamd_prover_upload_partial(rlnamd_prover* p, size_t n, const uint8_t* coords320) {
  RLN_TRY
  p->p->upload_partial(n, coords320);
  RLN_CATCH
}
int rlnamd_prover_upload_witness(rlnamd_prover* p, size_t n, const uint8_t* witness_le) {
  RLN_TRY
  p->p->upload_witness(n, witness_le);
  RLN_CATCH
}
int rlnamd_prover_download_partial(rlnamd_prover* p, size_t n, uint8_t* coords320) {
  RLN_TRY
  p->p->download_partial(n, coords320);
  RLN_CATCH
}
int rlnamd_prover_known_mask(rlnamd_prover* p, uint8_t* out) {
  RLN_TRY
  const std::vector<uint8_t>& m = p->p->known_mask();
  memcpy(out, m.data(), m.size());
  RLN_CATCH
}
int rlnamd_prover_download(rlnamd_prover* p, size_t n, uint8_t* proofs, uint8_t* coords, uint8_t* values,
                           uint32_t* errors) {
  RLN_TRY
  std::vector<ProofOut> out(n);
  p->p->download(n, out.data());
  for (size_t i = 0; i < n; i++) {
    if (proofs) memcpy(proofs + i * 128, out[i].compressed, 128);
    if (coords) memcpy(coords + i * 256, out[i].coords, 256);
    if (values) memcpy(values + i * 160, out[i].values, 160);
    if (errors) errors[i] = out[i].error;
  }
  RLN_CATCH
}
int rlnamd_prover_stage_ms(rlnamd_prover* p, float ms[RLNAMD_PROVER_STAGES]) {
  RLN_TRY
  p->p->stage_ms(ms);
  RLN_CATCH
}
int rlnamd_prover_walk_clock_mhz(rlnamd_prover* p, double mhz[2]) {
  RLN_TRY
  p->p->walk_clock_mhz(mhz);
  RLN_CATCH
}
const char* rlnamd_prover_stage_name(int i) { return (i >= 0 && i < PROVER_STAGES) ? kProverStageNames[i] : ""; }

int rlnamd_prover_describe(rlnamd_prover* p, char* buf, size_t cap) {
  RLN_TRY
  std::string d = p->p->tuning().describe();
  if (cap) {
    strncpy(buf, d.c_str(), cap - 1);
    buf[cap - 1] = 0;
  }
  RLN_CATCH
}
int rlnamd_prover_init_ms(rlnamd_prover* p, float ms[4]) {
  RLN_TRY
  for (int k = 0; k < 4; k++) ms[k] = p->p->init_ms()[k];
  RLN_CATCH
}
int rlnamd_prover_wipe(rlnamd_prover* p) {
  RLN_TRY
  p->p->wipe(0);
  RLN_CATCH
}
int rlnamd_prover_fetch_witness(rlnamd_prover* p, size_t index, uint8_t* out_le) {
  RLN_TRY
  std::vector<uint8_t> w;
  p->p->fetch_witness(index, &w);
  memcpy(out_le, w.data(), w.size());
  RLN_CATCH
}
int rlnamd_prover_fetch_h(rlnamd_prover* p, size_t index, uint8_t* out_le) {
  RLN_TRY
  std::vector<uint8_t> h;
  p->p->fetch_h(index, &h);
  memcpy(out_le, h.data(), h.size());
  RLN_CATCH
}
int rlnamd_prover_residue(rlnamd_prover* p, uint64_t out[6]) {
  RLN_TRY
  static_assert(Prover::RESIDUE_FIELDS == 6, "rln_amd.h states six counters");
  p->p->residue(out);
  RLN_CATCH
}
int rlnamd_prover_residue_slot(rlnamd_prover* p, int slot, uint64_t out[10]) {
  RLN_TRY
  static_assert(Prover::RESIDUE_SLOT_FIELDS == 10, "rln_amd.h states ten counters");
  p->p->residue_slot(slot, out);
  RLN_CATCH
}

int rlnamd_verify(rlnamd_prover* p, const uint8_t proof[128], const uint8_t values_le[160], int* ok) {
  RLN_TRY
  verify_common(p->p->zkey(), proof, values_le, ok);
  RLN_CATCH
}

int rlnamd_msm_new(size_t capacity, rlnamd_msm** out) {
  RLN_TRY
  std::unique_ptr<rlnamd_msm> h(new rlnamd_msm);
  h->m.reset(new MsmG1(capacity ? capacity : 1));
  *out = h.release();
  RLN_CATCH
}
int rlnamd_msm_new_g2(size_t capacity, rlnamd_msm** out) {
  RLN_TRY
  std::unique_ptr<rlnamd_msm> h(new rlnamd_msm);
  h->m2.reset(new MsmG2(capacity ? capacity : 1));
  *out = h.release();
  RLN_CATCH
}
void rlnamd_msm_free(rlnamd_msm* m) { delete m; }
size_t rlnamd_msm_point_bytes(rlnamd_msm* m) { return m->m2 ? MsmG2::POINT_BYTES : MsmG1::POINT_BYTES; }
size_t rlnamd_msm_window_sums_bytes_of(rlnamd_msm* m) { return m->m2 ? MsmG2::window_sums_bytes() : MsmG1::window_sums_bytes(); }
int rlnamd_poseidon_params_check(const uint8_t* inputs_le, size_t arity, uint8_t out_dense_le[32], uint8_t out_sparse_le[32]) {
  RLN_TRY
  if (arity == 0) throw Error("Empty input provided");
  if (arity > 8) throw Error("No parameters found for input length " + std::to_string(arity));
  PoseidonParams P = poseidon_derive_params((int)arity + 1);
  std::vector<Fr> in(arity);
  for (size_t i = 0; i < arity; i++) {
    uint32_t tmp[8];
    memcpy(tmp, inputs_le + 32 * i, 32);
    if (limbs_geq(tmp, FrParams::MOD)) throw Error("Non-canonical field element: value is not in [0, r-1]");
    in[i] = Fr::from_canonical(tmp);
  }
  Fr d, sp;
  poseidon_params_eval_host(P, in.data(), &d, &sp);
  // the host hash of the tree's single-path chain (MerkleTreeDev::set_few) is that sparse form with fixed-size state
  if (poseidon_hash_host(poseidon_host_params((int)arity + 1), in.data()) != sp)
    throw Error("internal: poseidon_hash_host differs from the sparse evaluation");
  uint32_t c[8];
  d.to_canonical(c);
  memcpy(out_dense_le, c, 32);
  sp.to_canonical(c);
  memcpy(out_sparse_le, c, 32);
  RLN_CATCH
}
int rlnamd_selftest_fq29(int group, uint32_t threads, uint32_t iters, const uint8_t* g2_gen_xy_le, uint32_t* mismatches) {
  RLN_TRY
  *mismatches = selftest_fq29(group, threads, iters, g2_gen_xy_le);
  RLN_CATCH
}
int rlnamd_probe_field(int field, uint32_t op, uint32_t in_words, uint32_t out_words, size_t n, const uint32_t* in, uint32_t* out) {
  RLN_TRY
  probe_field(field, op, in_words, out_words, n, in, out);
  RLN_CATCH
}
int rlnamd_probe_f29(int field, uint32_t op, uint32_t in_words, uint32_t out_words, size_t n, const uint32_t* in, uint32_t* out) {
  RLN_TRY
  probe_f29(field, op, in_words, out_words, n, in, out);
  RLN_CATCH
}
int rlnamd_probe_quotient_transform(int logn, int lds, uint32_t B, uint32_t nb, uint32_t vectors, const uint32_t* in,
                                    uint32_t* out) {
  RLN_TRY
  probe_quotient_transform(logn, lds, B, nb, vectors, in, out);
  RLN_CATCH
}
int rlnamd_probe_log_positions(const uint8_t* keep, size_t n, uint32_t* pos, uint64_t* kept) {
  RLN_TRY
  probe_log_positions(keep, n, pos, kept);
  RLN_CATCH
}
int rlnamd_probe_witness_op(size_t n, const uint32_t* in, uint32_t* out) {
  RLN_TRY
  probe_witness_op(n, in, out);
  RLN_CATCH
}
int rlnamd_msm_set(rlnamd_msm* m, const uint8_t* points_xy_le, const uint8_t* scalars_le, size_t n) {
  RLN_TRY
  if (m->m2) m->m2->set_host(points_xy_le, scalars_le, n);
  else m->m->set_host(points_xy_le, scalars_le, n);
  RLN_CATCH
}
int rlnamd_msm_generate(rlnamd_msm* m, uint64_t seed, uint64_t first_index, size_t n) {
  RLN_TRY
  if (m->m2) m->m2->generate(seed, first_index, n);
  else m->m->generate(seed, first_index, n);
  RLN_CATCH
}
int rlnamd_msm_generate_mode(rlnamd_msm* m, uint64_t seed, uint64_t first_index, size_t n, uint32_t mode) {
  RLN_TRY
  if (mode > 3) throw Error("rlnamd_msm_generate_mode: unknown mode bits");
  if (m->m2) m->m2->generate(seed, first_index, n, mode);
  else m->m->generate(seed, first_index, n, mode);
  RLN_CATCH
}
int rlnamd_msm_fetch(rlnamd_msm* m, size_t first, size_t count, uint8_t* points_xy_le, uint8_t* scalars_le) {
  RLN_TRY
  if (m->m2) m->m2->fetch(first, count, points_xy_le, scalars_le);
  else m->m->fetch(first, count, points_xy_le, scalars_le);
  RLN_CATCH
}
size_t rlnamd_msm_window_sums_bytes(void) { return MsmG1::window_sums_bytes(); }
int rlnamd_msm_run(rlnamd_msm* m, uint8_t* window_sums, float ms[3]) {
  RLN_TRY
  if (m->m2) m->m2->run_windows(window_sums, ms);
  else m->m->run_windows(window_sums, ms);
  RLN_CATCH
}
int rlnamd_msm_run_sharded(rlnamd_msm* m, rlnamd_comm* c, uint8_t out_xy_le[64], float ms[4]) {
  RLN_TRY
  if (!c) throw Error("rlnamd_msm_run_sharded: no communicator");
  if (m->m2) m->m2->run_sharded(rlnamd_comm_handle(c), rlnamd_comm_size(c), out_xy_le, ms);
  else m->m->run_sharded(rlnamd_comm_handle(c), rlnamd_comm_size(c), out_xy_le, ms);
  RLN_CATCH
}
int rlnamd_msm_combine(rlnamd_msm* m, const uint8_t* window_sums, size_t contributors, uint8_t out_xy_le[64]) {
  RLN_TRY
  if (m->m2) m->m2->combine(window_sums, contributors, out_xy_le);
  else m->m->combine(window_sums, contributors, out_xy_le);
  RLN_CATCH
}

static void verify_common(const Zkey& zk, const uint8_t proof[128], const uint8_t* values_le, int* ok, size_t nv) {
  G1Affine A, C;
  G2Affine B;
  *ok = 0;
  // Validate::Yes of the reference's proof deserialiser: on the curve AND, for G2, in the order-r subgroup
  if (!g1_decompress(proof, &A) || !g2_decompress(proof + 32, &B) || !g1_decompress(proof + 96, &C) ||
      !g2_in_subgroup(B))
    throw Error("Proof serialization error: the input buffer contained invalid data");
  std::vector<Fr> in;
  for (size_t i = 0; i < nv; i++) {
    uint32_t c[8];
    memcpy(c, values_le + 32 * i, 32);
    if (limbs_geq(c, FrParams::MOD)) throw Error("Non-canonical field element: value is not in [0, r-1]");
    in.push_back(Fr::from_canonical(c));
  }
  *ok = groth16_verify(zk, A, B, C, in) ? 1 : 0;
}

// n independent verifications spread over host threads (verification stays on the CPU; a relay node
// verifies every message it forwards).  ok[i] = 1 valid, 0 invalid or malformed.
}  // extern "C"
namespace rlnamd {
void verify_many_common(const Zkey& zk, size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t nv,
                        int threads, uint8_t* ok) {
  if (nv + 1 != zk.gamma_abc_g1.size()) throw Error("MalformedVerifyingKey");
  (void)prepared(zk);  // once, before the workers only read it
  unsigned hw = std::thread::hardware_concurrency();
  if (!hw) hw = 1;
  size_t nt = threads > 0 ? (size_t)threads : hw;
  nt = std::max<size_t>(1, std::min({nt, n, (size_t)4 * hw}));   // more threads than that only cost memory
  std::atomic<size_t> next{0};
  auto work = [&]() {
    for (size_t i = next.fetch_add(1); i < n; i = next.fetch_add(1)) {
      int v = 0;
      try {
        verify_common(zk, proofs + 128 * i, values_le + 32 * nv * i, &v, nv);
      } catch (const std::exception&) {
        v = 0;
      }
      ok[i] = (uint8_t)v;
    }
  };
  std::vector<std::thread> pool;
  pool.reserve(nt);
  for (size_t t = 1; t < nt; t++) {
    try {
      pool.emplace_back(work);
    } catch (const std::system_error&) {
      break;  // no more threads to be had: the ones running (and this one) drain the queue
    }
  }
  work();
  for (auto& t : pool) t.join();
}
}  // namespace rlnamd
extern "C" {
int rlnamd_verify_many(rlnamd_prover* p, size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t n_values,
                       int threads, uint8_t* ok) {
  RLN_TRY
  if (n_values + 1 != p->p->zkey().gamma_abc_g1.size()) throw Error("MalformedVerifyingKey");
  verify_many_common(p->p->zkey(), n, proofs, values_le, n_values, threads, ok);
  RLN_CATCH
}
int rlnamd_verify_many_gpu(rlnamd_prover* p, size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t n_values,
                           uint8_t* ok) {
  RLN_TRY
  if (n_values + 1 != p->p->zkey().gamma_abc_g1.size()) throw Error("MalformedVerifyingKey");
  if (n) p->p->gpu_verifier().verify(n, proofs, values_le, n_values, ok, nullptr);
  RLN_CATCH
}
int rlnamd_verify_many_gpu_gt(rlnamd_prover* p, size_t n, const uint8_t* proofs, const uint8_t* values_le,
                              size_t n_values, uint8_t* gt384) {
  RLN_TRY
  if (n_values + 1 != p->p->zkey().gamma_abc_g1.size()) throw Error("MalformedVerifyingKey");
  if (n) p->p->gpu_verifier().verify(n, proofs, values_le, n_values, nullptr, gt384);
  RLN_CATCH
}
int rlnamd_verify_many_gpu_ex(rlnamd_prover* p, size_t n, const uint8_t* proofs, const uint8_t* values_le,
                              size_t n_values, int lanes, uint8_t* ok, uint8_t* gt384) {
  RLN_TRY
  if (lanes != 0 && lanes != 1 && lanes != 8) throw Error("rlnamd_verify_many_gpu_ex: lanes must be 0, 1 or 8");
  if (n_values + 1 != p->p->zkey().gamma_abc_g1.size()) throw Error("MalformedVerifyingKey");
  if (n && (ok || gt384)) p->p->gpu_verifier().verify(n, proofs, values_le, n_values, ok, gt384, lanes);
  RLN_CATCH
}
int rlnamd_verify_gpu_passes(rlnamd_prover* p, size_t passes[2]) {
  RLN_TRY
  p->p->gpu_verifier().passes(passes);
  RLN_CATCH
}
int rlnamd_verify_many_with_zkey(const uint8_t* zkey, size_t zkey_len, size_t n, const uint8_t* proofs,
                                 const uint8_t* values_le, size_t n_values, int threads, uint8_t* ok) {
  RLN_TRY
  Zkey zk = parse_arkzkey(zkey, zkey_len);
  if (n_values + 1 != zk.gamma_abc_g1.size()) throw Error("MalformedVerifyingKey");
  verify_many_common(zk, n, proofs, values_le, n_values, threads, ok);
  RLN_CATCH
}

int rlnamd_verify_many_gpu_optimistic(rlnamd_prover* p, size_t n, const uint8_t* proofs, const uint8_t* values_le,
                                      size_t n_values, const uint8_t* scalars16, uint8_t* ok) {
  RLN_TRY
  if (n_values + 1 != p->p->zkey().gamma_abc_g1.size())
    throw Error("MalformedVerifyingKey: rlnamd_verify_many_gpu_optimistic: n_values is not the key's input count");
  if (n && (!proofs || !values_le || !ok)) throw Error("rlnamd_verify_many_gpu_optimistic: null argument with n > 0");
  if (n) p->p->gpu_verifier().verify_optimistic(n, proofs, values_le, n_values, scalars16, ok);
  RLN_CATCH
}
int rlnamd_verify_many_gpu_optimistic_ex(rlnamd_prover* p, size_t n, const uint8_t* proofs, const uint8_t* values_le,
                                         size_t n_values, const uint8_t* scalars16, int lanes, uint8_t* ok) {
  RLN_TRY
  if (lanes != 0 && lanes != 1 && lanes != 8)
    throw Error("rlnamd_verify_many_gpu_optimistic_ex: lanes must be 0, 1 or 8");
  if (n_values + 1 != p->p->zkey().gamma_abc_g1.size())
    throw Error("MalformedVerifyingKey: rlnamd_verify_many_gpu_optimistic_ex: n_values is not the key's input count");
  if (n && (!proofs || !values_le || !ok)) throw Error("rlnamd_verify_many_gpu_optimistic_ex: null argument with n > 0");
  if (n) p->p->gpu_verifier().verify_optimistic(n, proofs, values_le, n_values, scalars16, ok, lanes, true);
  RLN_CATCH
}
int rlnamd_verify_gpu_optimistic_stats(rlnamd_prover* p, uint64_t out[8]) {
  RLN_TRY
  p->p->gpu_verifier().optimistic_stats(out);
  RLN_CATCH
}
int rlnamd_verify_gpu_finish_time(rlnamd_prover* p, uint64_t out[2]) {
  RLN_TRY
  p->p->gpu_verifier().finish_time(out);
  RLN_CATCH
}
int rlnamd_verify_gpu_set_cooldown(rlnamd_prover* p, size_t chunks) {
  RLN_TRY
  p->p->gpu_verifier().set_cooldown(chunks);
  RLN_CATCH
}
int rlnamd_verify_gpu_aggregate(rlnamd_prover* p, size_t n, const uint8_t* proofs, const uint8_t* values_le,
                                size_t n_values, const uint8_t* scalars16, uint8_t gt384[384], uint8_t* rejected) {
  RLN_TRY
  if (n_values + 1 != p->p->zkey().gamma_abc_g1.size())
    throw Error("MalformedVerifyingKey: rlnamd_verify_gpu_aggregate: n_values is not the key's input count");
  p->p->gpu_verifier().aggregate(n, proofs, values_le, n_values, scalars16, gt384, rejected);
  RLN_CATCH
}
int rlnamd_verify_agg_scalars(const uint8_t seed[32], uint64_t chunk, size_t n, uint8_t* out16) {
  RLN_TRY
  if (!seed || (n && !out16)) throw Error("rlnamd_verify_agg_scalars: null argument");
  aggsc::scalars_host(seed, chunk, n, out16);
  RLN_CATCH
}
int rlnamd_verify_gpu_aggregate_seeded(rlnamd_prover* p, size_t n, const uint8_t* proofs, const uint8_t* values_le,
                                       size_t n_values, const uint8_t seed32[32], int lanes, uint8_t gt384[384],
                                       uint8_t* rejected) {
  RLN_TRY
  if (lanes != 1 && lanes != 8) throw Error("rlnamd_verify_gpu_aggregate_seeded: lanes must be 1 or 8");
  if (!seed32) throw Error("rlnamd_verify_gpu_aggregate_seeded: null seed");
  if (n_values + 1 != p->p->zkey().gamma_abc_g1.size())
    throw Error("MalformedVerifyingKey: rlnamd_verify_gpu_aggregate_seeded: n_values is not the key's input count");
  p->p->gpu_verifier().aggregate_seeded(n, proofs, values_le, n_values, seed32, gt384, rejected, lanes);
  RLN_CATCH
}
int rlnamd_verify_gpu_aggregate_ex(rlnamd_prover* p, size_t n, const uint8_t* proofs, const uint8_t* values_le,
                                   size_t n_values, const uint8_t* scalars16, int lanes, uint8_t gt384[384],
                                   uint8_t* rejected) {
  RLN_TRY
  if (lanes != 1 && lanes != 8) throw Error("rlnamd_verify_gpu_aggregate_ex: lanes must be 1 or 8");
  if (n_values + 1 != p->p->zkey().gamma_abc_g1.size())
    throw Error("MalformedVerifyingKey: rlnamd_verify_gpu_aggregate_ex: n_values is not the key's input count");
  p->p->gpu_verifier().aggregate(n, proofs, values_le, n_values, scalars16, gt384, rejected, lanes);
  RLN_CATCH
}
}  // extern "C"
namespace rlnamd {
// f(i) for i < n on host threads
template <class F>
static void parallel_for(size_t n, F f) {
  unsigned hw = std::thread::hardware_concurrency();
  const size_t nt = std::max<size_t>(1, std::min<size_t>(hw ? hw : 1, n));
  std::atomic<size_t> next{0};
  auto work = [&](size_t t) {
    for (size_t i = next.fetch_add(1); i < n; i = next.fetch_add(1)) f(i, t);
  };
  std::vector<std::thread> pool;
  for (size_t t = 1; t < nt; t++) {
    try {
      pool.emplace_back(work, t);
    } catch (const std::system_error&) {
      break;
    }
  }
  work(0);
  for (auto& t : pool) t.join();
}
// The yardstick of the combined check, from pairing.h alone: prod_i GT_i^(r_i) over the exact per-proof pairing
// products GT_i = final_exponentiation(miller_loop_3(..) alpha_beta); a proof the host rules refuse counts as 1 and
// gets rejected[i] = 1.  Rows that repeat byte for byte share one pairing product.
static void aggregate_host(const Zkey& zk, size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t nv,
                           const uint8_t* scalars16, uint8_t gt384[384], uint8_t* rejected) {
  const PreparedVk& pv = prepared(zk);
  std::unordered_map<std::string, size_t> seen;
  std::vector<size_t> row_of(n), first;
  for (size_t i = 0; i < n; i++) {
    std::string key((const char*)proofs + 128 * i, 128);
    key.append((const char*)values_le + 32 * nv * i, 32 * nv);
    auto it = seen.emplace(std::move(key), first.size());
    if (it.second) first.push_back(i);
    row_of[i] = it.first->second;
  }
  std::vector<Fq12> gt(first.size(), Fq12::one());
  std::vector<uint8_t> refused(first.size(), 0);
  parallel_for(first.size(), [&](size_t d, size_t) {
    const uint8_t *proof = proofs + 128 * first[d], *vals = values_le + 32 * nv * first[d];
    G1Affine A, C;
    G2Affine B;
    bool ok = g1_decompress(proof, &A) && g2_decompress(proof + 32, &B) && g1_decompress(proof + 96, &C) &&
              g2_in_subgroup(B);
    std::vector<Fr> x(nv);
    for (size_t j = 0; ok && j < nv; j++) {
      uint32_t c[8];
      memcpy(c, vals + 32 * j, 32);
      ok = !limbs_geq(c, FrParams::MOD);
      if (ok) x[j] = Fr::from_canonical(c);
    }
    refused[d] = ok ? 0 : 1;
    if (!ok) return;
    const G1Affine ic = ic_combination(zk, pv, x).to_affine();
    gt[d] = final_exponentiation(f12_mul(miller_loop_3(A, B, ic.neg(), pv.gamma, C.neg(), pv.delta), pv.alpha_beta));
  });
  unsigned hw = std::thread::hardware_concurrency();
  std::vector<Fq12> part(hw ? hw : 1, Fq12::one());
  parallel_for(n, [&](size_t i, size_t t) {
    rejected[i] = refused[row_of[i]];
    if (rejected[i]) return;
    uint32_t k[4];
    memcpy(k, scalars16 + 16 * i, 16);
    const Fq12& g = gt[row_of[i]];   // in the cyclotomic subgroup: its squaring applies
    Fq12 r = Fq12::one();
    bool started = false;
    for (int b = 127; b >= 0; b--) {
      if (started) r = f12_cyclotomic_sqr(r);
      if ((k[b >> 5] >> (b & 31)) & 1) {
        r = started ? f12_mul(r, g) : g;
        started = true;
      }
    }
    part[t] = f12_mul(part[t], r);
  });
  Fq12 all = Fq12::one();
  for (const Fq12& f : part) all = f12_mul(all, f);
  for (int i = 0; i < 6; i++) {
    uint32_t a[8], b[8];
    all.c[i].c0.to_canonical(a);
    all.c[i].c1.to_canonical(b);
    memcpy(gt384 + 64 * i, a, 32);
    memcpy(gt384 + 64 * i + 32, b, 32);
  }
}
}  // namespace rlnamd
extern "C" {
int rlnamd_verify_aggregate_with_zkey(const uint8_t* zkey, size_t zkey_len, size_t n, const uint8_t* proofs,
                                      const uint8_t* values_le, size_t n_values, const uint8_t* scalars16,
                                      uint8_t gt384[384], uint8_t* rejected) {
  RLN_TRY
  Zkey zk = parse_arkzkey(zkey, zkey_len);
  if (n_values + 1 != zk.gamma_abc_g1.size()) throw Error("MalformedVerifyingKey");
  if (!gt384 || (n && (!proofs || !values_le || !scalars16 || !rejected)))
    throw Error("rlnamd_verify_aggregate_with_zkey: null argument");
  aggregate_host(zk, n, proofs, values_le, n_values, scalars16, gt384, rejected);
  RLN_CATCH
}

size_t rlnamd_prover_num_public(rlnamd_prover* p) { return p->p->num_public(); }
int rlnamd_prover_download_public(rlnamd_prover* p, size_t n, uint8_t* out_le) {
  RLN_TRY
  std::vector<uint8_t> v;
  p->p->fetch_public(n, &v);
  memcpy(out_le, v.data(), v.size());
  RLN_CATCH
}
int rlnamd_verify_public(rlnamd_prover* p, const uint8_t proof[128], const uint8_t* values_le, size_t n_values, int* ok) {
  RLN_TRY
  verify_common(p->p->zkey(), proof, values_le, ok, n_values);
  RLN_CATCH
}

int rlnamd_verify_with_zkey(const uint8_t* zkey, size_t zkey_len, const uint8_t proof[128],
                            const uint8_t values_le[160], int* ok) {
  RLN_TRY
  Zkey zk = parse_arkzkey(zkey, zkey_len);
  verify_common(zk, proof, values_le, ok);
  RLN_CATCH
}

int rlnamd_parse_resources(const uint8_t* zkey, size_t zkey_len, const uint8_t* graph, size_t graph_len,
                           uint64_t counts[13]) {
  RLN_TRY
  Zkey zk = parse_arkzkey(zkey, zkey_len);
  Graph g = parse_graph(graph, graph_len);
  counts[0] = zk.num_instance_variables;
  counts[1] = zk.num_witness_variables;
  counts[2] = zk.num_constraints;
  counts[3] = zk.a_nnz;
  counts[4] = zk.b_nnz;
  counts[5] = zk.a_query.size();
  counts[6] = zk.h_query.size();
  counts[7] = zk.l_query.size();
  counts[8] = g.nodes.size();
  counts[9] = g.signals.size();
  counts[10] = g.tree_depth;
  counts[11] = g.max_out;
  counts[12] = g.inputs_size;
  RLN_CATCH
}

int rlnamd_proof_compress(const uint8_t coords_le[256], uint8_t proof[128]) {
  RLN_TRY
  auto ld = [&](int k) {
    uint32_t c[8];
    memcpy(c, coords_le + 32 * k, 32);
    if (limbs_geq(c, FqParams::MOD)) throw Error("Non-canonical field element");
    return Fq::from_canonical(c);
  };
  G1Affine A{ld(0), ld(1)}, C{ld(6), ld(7)};
  G2Affine B{{ld(2), ld(3)}, {ld(4), ld(5)}};
  g1_compress(A, proof);
  g2_compress(B, proof + 32);
  g1_compress(C, proof + 96);
  RLN_CATCH
}
int rlnamd_proof_decompress(const uint8_t proof[128], uint8_t coords_le[256]) {
  RLN_TRY
  G1Affine A, C;
  G2Affine B;
  if (!g1_decompress(proof, &A) || !g2_decompress(proof + 32, &B) || !g1_decompress(proof + 96, &C))
    throw Error("Proof serialization error: the input buffer contained invalid data");
  auto st = [&](int k, const Fq& v) {
    uint32_t c[8];
    v.to_canonical(c);
    memcpy(coords_le + 32 * k, c, 32);
  };
  st(0, A.x); st(1, A.y); st(2, B.x.c0); st(3, B.x.c1); st(4, B.y.c0); st(5, B.y.c1); st(6, C.x); st(7, C.y);
  RLN_CATCH
}

}  // extern "C"
