// The sequential ledger's draw by count (zerokit_amd/csrc/quota_ledger.h: SeqLedger::draw_counts, issue_counts and the
// refusals) behind the small C interface of quota.cpp, which this file takes in whole, for
// tests/test_quota_counts_host.py (ctypes) and tests/host/quota_counts_main.cpp (the sanitizer build).  No HIP, no device.
#include "quota.cpp"

extern "C" {

const char* ql_count_refusal(size_t i, uint64_t count) { return say(quota::count_refusal(i, count)); }
const char* ql_draw_counts_refusal(size_t n, const uint64_t* leaf, const uint8_t* ext, const uint32_t* limits, const uint8_t* counts,
                                   const uint32_t* firsts, const uint8_t* status, uint32_t depth) {
  return say(quota::draw_counts_refusal(n, leaf, ext, limits, counts, firsts, status, depth));
}
int ql_draw_counts(void* h, size_t n, const uint64_t* leaf, const uint8_t* ext, const uint32_t* limits, const uint8_t* counts,
                   uint32_t* firsts, uint8_t* status) {
  return say(((quota::SeqLedger*)h)->draw_counts(n, leaf, ext, limits, counts, firsts, status))[0] ? 1 : 0;
}
// the rule on its own: out[0] = what goes into firsts_out, out[1] = the status
void ql_issue_counts(uint32_t used, uint32_t rank, uint32_t count, uint32_t limit, uint32_t out[2]) {
  const quota::Issue r = quota::issue_counts(used, rank, count, limit);
  out[0] = r.id;
  out[1] = r.status;
}
uint32_t ql_advance_counts(uint32_t used, uint32_t start, uint32_t last_ok, uint32_t rank_last, uint32_t count_last) {
  return quota::advance_counts(used, start, last_ok, rank_last, count_last);
}
// a counter set by hand, for the cases that start near 2^32 (in the window only)
int ql_set_used(void* h, uint64_t leaf, const uint8_t* ext, uint32_t value) {
  quota::SeqLedger& L = *(quota::SeqLedger*)h;
  quota::Row32 e;
  memcpy(e.w, ext, 32);
  const uint32_t s = quota::slot_of(L.window.e, L.window.live, L.max_epochs, e);
  if (s == quota::NO_SLOT || (leaf >> L.depth)) return 1;
  L.used[quota::counter_of(quota::pack_key(s, (uint32_t)leaf), L.depth)] = value;
  return 0;
}
uint32_t ql_count_max() { return quota::COUNT_MAX; }

}  // extern "C"
