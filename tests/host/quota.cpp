// The sequential quota ledger of zerokit_amd/csrc/quota_ledger.h behind a small C interface, for
// tests/test_quota_host.py (ctypes) and tests/host/quota_main.cpp (the sanitizer build).  No HIP, no device.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "quota_ledger.h"

using namespace rlnamd;

static thread_local std::string g_said;
static const char* say(const std::string& s) {
  g_said = s;
  return g_said.c_str();
}

extern "C" {

const char* ql_last() { return g_said.c_str(); }
const char* ql_new_refusal(size_t depth, size_t max_epochs) { return say(quota::new_refusal(depth, max_epochs)); }
const char* ql_epochs_refusal(const uint8_t* ext, size_t k, size_t max_epochs) { return say(quota::epochs_refusal(ext, k, max_epochs)); }
const char* ql_draw_refusal(size_t n, const uint64_t* leaf, const uint8_t* ext, const uint32_t* limits, const uint32_t* ids,
                            const uint8_t* status, uint32_t depth) {
  return say(quota::draw_refusal(n, leaf, ext, limits, ids, status, depth));
}

void* ql_new(size_t depth, size_t max_epochs) {
  if (!quota::new_refusal(depth, max_epochs).empty()) return nullptr;
  return new quota::SeqLedger((uint32_t)depth, (uint32_t)max_epochs);
}
void ql_free(void* h) { delete (quota::SeqLedger*)h; }
int ql_set_epochs(void* h, const uint8_t* ext, size_t k) { return say(((quota::SeqLedger*)h)->set_epochs(ext, k))[0] ? 1 : 0; }
size_t ql_epochs(void* h, uint8_t* out) { return ((quota::SeqLedger*)h)->epochs(out); }
int ql_draw(void* h, size_t n, const uint64_t* leaf, const uint8_t* ext, const uint32_t* limits, uint32_t* ids, uint8_t* status) {
  return say(((quota::SeqLedger*)h)->draw(n, leaf, ext, limits, ids, status))[0] ? 1 : 0;
}
// the counters of n (leaf, external nullifier) pairs; inside[i] = 0 outside the window
void ql_used(void* h, size_t n, const uint64_t* leaf, const uint8_t* ext, uint32_t* out, uint8_t* inside) {
  const quota::SeqLedger& L = *(quota::SeqLedger*)h;
  for (size_t i = 0; i < n; i++) {
    quota::Row32 e;
    memcpy(e.w, ext + 32 * i, 32);
    const uint32_t s = quota::slot_of(L.window.e, L.window.live, L.max_epochs, e);
    inside[i] = s != quota::NO_SLOT;
    out[i] = inside[i] ? L.used[quota::counter_of(quota::pack_key(s, (uint32_t)leaf[i]), L.depth)] : 0;
  }
}
// [window size, draws, issued, over, no_epoch, non-zero counters in slots that hold no external nullifier (0 expected)]
void ql_info(void* h, uint64_t out[6]) {
  const quota::SeqLedger& L = *(quota::SeqLedger*)h;
  out[0] = L.window.k;
  out[1] = L.draws;
  out[2] = L.issued;
  out[3] = L.over;
  out[4] = L.no_epoch;
  out[5] = 0;
  for (uint32_t s = 0; s < L.max_epochs; s++)
    if (!((L.window.live >> s) & 1))
      for (size_t i = 0; i < (size_t)1 << L.depth; i++) out[5] += L.used[((size_t)s << L.depth) + i] != 0;
}
void ql_plan(size_t n, uint32_t depth, uint64_t out[4]) {
  const quota::DrawPlan P = quota::plan_for(n, depth);
  out[0] = P.passes;
  out[1] = P.blocks;
  out[2] = P.bin_levels;
  out[3] = P.rank_levels;
}

}  // extern "C"
