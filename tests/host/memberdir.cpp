// The sequential member directory of zerokit_amd/csrc/member_directory.h behind a small C interface, for
// tests/test_member_directory_host.py (ctypes) and tests/host/memberdir_main.cpp (the sanitizer build); and the insert
// and commit passes of a register call on host threads over nlog::StdAtomics.  No HIP, no device, no Poseidon: the
// commitments of the secrets a resolve is given come from the caller.
#include <stdint.h>
#include <string.h>

#include <string>
#include <thread>
#include <vector>

#include "member_directory.h"

using namespace rlnamd;

static thread_local std::string g_said;
static const char* say(const std::string& s) {
  g_said = s;
  return g_said.c_str();
}
static int said(const std::string& s) { return say(s)[0] ? 1 : 0; }

extern "C" {

const char* md_last() { return g_said.c_str(); }
const char* md_new_refusal(uint64_t capacity, uint64_t depth) { return say(mdir::new_refusal(capacity, depth)); }
const char* md_register_refusal(size_t n, const uint64_t* indices, const uint8_t* idcs, const uint32_t* limits, const uint8_t* status,
                                uint64_t capacity) {
  return say(mdir::register_refusal(n, indices, idcs, limits, status, capacity));
}
const char* md_find_refusal(size_t n, const uint8_t* idcs, const uint8_t* status, const uint64_t* index, const uint32_t* limit) {
  return say(mdir::find_refusal(n, idcs, status, index, limit));
}
const char* md_resolve_refusal(const char* call, size_t n, const uint8_t* secrets, const uint8_t* take, const uint8_t* status,
                               const uint64_t* index, const uint32_t* limit) {
  return say(mdir::resolve_refusal(call, n, secrets, take, status, index, limit));
}
const char* md_remove_refusal(size_t n, const uint64_t* indices, const uint8_t* status, uint64_t capacity) {
  return say(mdir::remove_refusal(n, indices, status, capacity));
}
const char* md_get_refusal(size_t n, const uint64_t* indices, const uint8_t* live, const uint8_t* idcs, const uint32_t* limits,
                           uint64_t capacity) {
  return say(mdir::get_refusal(n, indices, live, idcs, limits, capacity));
}

void* md_new(uint64_t capacity, uint64_t seed) {
  if (!mdir::new_refusal(capacity, 63).empty()) return nullptr;
  return new mdir::SeqDirectory(capacity, seed);
}
void md_free(void* h) { delete (mdir::SeqDirectory*)h; }
int md_register(void* h, size_t n, const uint64_t* indices, const uint8_t* idcs, const uint32_t* limits, uint8_t* status) {
  return said(((mdir::SeqDirectory*)h)->do_register(n, indices, idcs, limits, status));
}
int md_find(void* h, size_t n, const uint8_t* idcs, uint8_t* status, uint64_t* index, uint32_t* limit) {
  return said(((mdir::SeqDirectory*)h)->do_find(n, idcs, status, index, limit));
}
int md_resolve(void* h, size_t n, const uint8_t* secrets, const uint8_t* keys, const uint8_t* take, uint8_t* status, uint64_t* index,
               uint32_t* limit) {
  return said(((mdir::SeqDirectory*)h)->do_resolve(n, secrets, keys, take, status, index, limit));
}
int md_slash(void* h, size_t n, const uint8_t* secrets, const uint8_t* keys, const uint8_t* take, uint8_t* status, uint64_t* index,
             uint32_t* limit, uint64_t* removed) {
  return said(((mdir::SeqDirectory*)h)->do_slash(n, secrets, keys, take, status, index, limit, removed));
}
int md_remove(void* h, size_t n, const uint64_t* indices, uint8_t* status) {
  return said(((mdir::SeqDirectory*)h)->do_remove(n, indices, status));
}
int md_get(void* h, size_t n, const uint64_t* indices, uint8_t* live, uint8_t* idcs, uint32_t* limits) {
  return said(((mdir::SeqDirectory*)h)->do_get(n, indices, live, idcs, limits));
}
void md_info(void* h, uint64_t out[8]) { ((mdir::SeqDirectory*)h)->info(out); }

// A register call whose insert and commit passes run on `threads` host threads over std::atomic table entries, request i
// on thread i % threads; the rows pass and the counters stay on the calling thread, and a join stands between the
// passes as a kernel boundary does on the device.
int md_register_threads(void* h, size_t n, const uint64_t* indices, const uint8_t* idcs, const uint32_t* limits, uint8_t* status,
                        unsigned threads) {
  mdir::SeqDirectory& S = *(mdir::SeqDirectory*)h;
  if (said(mdir::register_refusal(n, indices, idcs, limits, status, S.capacity))) return 1;
  S.calls++;
  S.make_room(n);
  const mdir::View D = S.view();
  for (size_t i = 0; i < n; i++) status[i] = mdir::claim_row(D, (uint32_t)indices[i], mdir::row_of(idcs + 32 * i));
  std::vector<uint32_t> longest(threads, 0);
  auto pass = [&](bool commit) {
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < threads; t++)
      pool.emplace_back([&, t] {
        for (size_t i = t; i < n; i += threads) {
          if (status[i] != mdir::PENDING) continue;
          uint32_t w = 0;
          if (commit) status[i] = mdir::commit<nlog::StdAtomics>(D, (uint32_t)indices[i], limits[i], &w);
          else w = mdir::insert<nlog::StdAtomics>(D, (uint32_t)indices[i]);
          if (w > longest[t]) longest[t] = w;
        }
      });
    for (std::thread& th : pool) th.join();
  };
  pass(false);
  pass(true);
  for (unsigned t = 0; t < threads; t++) S.walked(longest[t]);
  for (size_t i = 0; i < n; i++)
    if (status[i] == mdir::OK) S.live++, S.taken++;
  return 0;
}

}  // extern "C"
