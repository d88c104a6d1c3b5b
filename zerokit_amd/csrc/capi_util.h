// Shared by the translation units that implement include/rln_amd.h: error capture at the C boundary (never let an
// exception cross it) and the handle types.
#pragma once
#include <exception>
#include <memory>
#include <mutex>
#include <string>

#include "../../include/rln_amd.h"
#include "keccak_batch.h"
#include "msm.h"
#include "nullifier_log.h"
#include "prover.h"
#include "quota_ledger.h"

namespace rlnamd {
extern thread_local std::string g_last_error;
int fail(const std::exception& e);
void fill_prover_info(const Prover& P, rlnamd_prover_info* info);
// n verifications on host threads; throws MalformedVerifyingKey when nv does not match the key
// ffi.cpp: the relays ffi_relay_step keeps per (RLN object, log) are named by the log's id, which is never issued twice,
// and a log that is freed drops them (before its own members go)
uint64_t next_log_id();
void relay_registry_drop_log(uint64_t log_id);
void verify_many_common(const Zkey& zk, size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t nv, int threads,
                        uint8_t* ok);
}  // namespace rlnamd

#define RLN_TRY try {
#define RLN_CATCH                        \
  return RLNAMD_OK;                      \
  }                                      \
  catch (const std::exception& e) {      \
    return rlnamd::fail(e);              \
  }                                      \
  catch (...) {                          \
    rlnamd::g_last_error = "unknown error"; \
    return RLNAMD_ERR;                   \
  }

struct rlnamd_prover {
  std::unique_ptr<rlnamd::Prover> p;
};
struct rlnamd_nullifier_log {
  // one stream and one staging block per log: every call on a handle takes this
  std::mutex mu;
  rlnamd::NullifierLogDev log;
  const uint64_t id = rlnamd::next_log_id();
  rlnamd_nullifier_log(uint64_t capacity, uint64_t seed) : log(capacity, seed) {}
  ~rlnamd_nullifier_log() { rlnamd::relay_registry_drop_log(id); }
};
struct rlnamd_hasher {
  // one stream and one pair of staging halves per hasher: every call on a handle takes this
  std::mutex mu;
  rlnamd::HasherDev hasher;
  rlnamd_hasher(size_t stage_bytes, size_t lane_max_blocks) : hasher(stage_bytes, lane_max_blocks) {}
};
struct rlnamd_quota {
  // one stream and one per-call block per ledger: every call on a handle takes this
  std::mutex mu;
  rlnamd::QuotaLedgerDev ledger;
  rlnamd_quota(size_t depth, size_t max_epochs) : ledger(depth, max_epochs) {}
  rlnamd_quota(const char* dir, size_t depth, size_t max_epochs, uint64_t journal_max_bytes)
      : ledger(dir, depth, max_epochs, journal_max_bytes) {}
};
struct rlnamd_msm {   // one of the two (rlnamd_msm_new / rlnamd_msm_new_g2)
  std::unique_ptr<rlnamd::MsmG1> m;
  std::unique_ptr<rlnamd::MsmG2> m2;
};
// pool.cpp
rlnamd::Prover* rlnamd_pool_replica_prover(rlnamd_pool* p, size_t replica);   // owned by the pool
void* rlnamd_comm_handle(rlnamd_comm* c);   // the ncclComm_t
int rlnamd_comm_size(rlnamd_comm* c);
