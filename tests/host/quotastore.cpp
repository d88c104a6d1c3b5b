// The durable quota store (zerokit_amd/csrc/quota_store.h) driven by the sequential ledger of quota_ledger.h behind a
// small C interface, for tests/test_quota_store_host.py (ctypes) and tests/host/quotastore_main.cpp (the stand-alone
// programs).  The order of events is the device ledger's: a window record before the window is applied, and behind a
// draw one advance record of what the sequential ledger changed -- the counters that moved, with their absolute
// values -- before the answers are handed out.  No HIP, no device.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "quota_store.h"

using namespace rlnamd;
using namespace rlnamd::qstore;

struct HostLedger {
  QuotaStore st;
  quota::SeqLedger L;
  std::string err;
  HostLedger(uint32_t depth, uint32_t max_epochs) : L(depth, max_epochs) {}

  std::vector<uint32_t> keys_of(size_t n, const uint64_t* leaf, const uint8_t* ext) const {
    std::vector<uint32_t> keys;
    for (size_t i = 0; i < n; i++) {
      quota::Row32 e;
      memcpy(e.w, ext + 32 * i, 32);
      const uint32_t s = quota::slot_of(L.window.e, L.window.live, L.max_epochs, e);
      if (s != quota::NO_SLOT) keys.push_back(quota::pack_key(s, (uint32_t)leaf[i]));
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    return keys;
  }
  void slot_pairs(uint32_t slot, std::vector<uint32_t>& out) const {
    for (size_t leaf = 0; leaf < (size_t)1 << L.depth; leaf++) {
      const uint32_t used = L.used[((size_t)slot << L.depth) + leaf];
      if (used) out.push_back((uint32_t)leaf), out.push_back(used);
    }
  }
  int compact() {
    try {
      st.compact(L.window, [this](uint32_t slot, std::vector<uint32_t>& out) { slot_pairs(slot, out); });
    } catch (const std::exception& e) {
      err = e.what();
      return 1;
    }
    return 0;
  }
  // counts null: a plain draw.  The answers go to scratch first and reach the caller behind the record's sync.
  int draw(size_t n, const uint64_t* leaf, const uint8_t* ext, const uint32_t* limits, const uint8_t* counts, uint32_t* ids,
           uint8_t* status) {
    const std::string refused = counts ? quota::draw_counts_refusal(n, leaf, ext, limits, counts, ids, status, L.depth)
                                       : quota::draw_refusal(n, leaf, ext, limits, ids, status, L.depth);
    if (!refused.empty()) {
      err = refused;
      return 1;
    }
    const std::vector<uint32_t> keys = keys_of(n, leaf, ext);
    std::vector<uint32_t> before(keys.size()), got_ids(n), delta;
    std::vector<uint8_t> got_status(n);
    for (size_t i = 0; i < keys.size(); i++) before[i] = L.used[quota::counter_of(keys[i], L.depth)];
    err = counts ? L.draw_counts(n, leaf, ext, limits, counts, got_ids.data(), got_status.data())
                 : L.draw(n, leaf, ext, limits, got_ids.data(), got_status.data());
    if (!err.empty()) return 1;
    for (size_t i = 0; i < keys.size(); i++) {
      const uint32_t now = L.used[quota::counter_of(keys[i], L.depth)];
      if (now != before[i]) delta.push_back(keys[i]), delta.push_back(now);
    }
    try {
      if (!delta.empty()) st.append_advance(delta.size() / 2, delta.data());
    } catch (const std::exception& e) {
      err = e.what();
      return 1;
    }
    if (n) memcpy(ids, got_ids.data(), 4 * n), memcpy(status, got_status.data(), n);
    if (st.wants_compaction()) return compact();
    return 0;
  }
  int set_epochs(const uint8_t* ext, size_t k) {
    err = quota::epochs_refusal(ext, k, L.max_epochs);
    if (!err.empty()) return 1;
    try {
      st.append_window(k, ext);
    } catch (const std::exception& e) {
      err = e.what();
      return 1;
    }
    err = L.set_epochs(ext, k);
    if (!err.empty()) return 1;
    if (st.wants_compaction()) return compact();
    return 0;
  }
};

static HostLedger* host_open(const char* dir, uint64_t depth, uint64_t max_epochs, uint64_t journal_max_bytes, std::string& err) {
  if (!quota::new_refusal(depth, max_epochs).empty()) {
    err = quota::new_refusal(depth, max_epochs);
    return nullptr;
  }
  HostLedger* h = new HostLedger((uint32_t)depth, (uint32_t)max_epochs);
  try {
    Image im;
    h->st.open(dir, depth, max_epochs, journal_max_bytes, im);
    h->L.window = im.window;
    for (const auto& kv : im.used) h->L.used[quota::counter_of(kv.first, h->L.depth)] = kv.second;
    h->st.set_restored(im.used.size());
  } catch (const std::exception& e) {
    err = e.what();
    delete h;
    return nullptr;
  }
  return h;
}

extern "C" {

uint32_t qs_crc32c(const uint8_t* p, size_t n) { return crc32c(p, n); }

void* qs_open(const char* dir, uint64_t depth, uint64_t max_epochs, uint64_t journal_max_bytes, char* err, size_t cap) {
  std::string e;
  HostLedger* h = host_open(dir, depth, max_epochs, journal_max_bytes, e);
  if (!h && cap) {
    strncpy(err, e.c_str(), cap - 1);
    err[cap - 1] = 0;
  }
  return h;
}
// compact: 0 just closes; 1 compacts if the journal holds records, as freeing the device ledger does; 2 compacts anyway
int qs_close(void* hv, int compact) {
  HostLedger* h = (HostLedger*)hv;
  int rc = 0;
  if (compact == 2 || (compact == 1 && h->st.has_records())) rc = h->compact();
  delete h;
  return rc;
}
int qs_compact(void* h) { return ((HostLedger*)h)->compact(); }
const char* qs_error(void* h) { return ((HostLedger*)h)->err.c_str(); }
int qs_set_epochs(void* h, const uint8_t* ext, size_t k) { return ((HostLedger*)h)->set_epochs(ext, k); }
int qs_draw(void* h, size_t n, const uint64_t* leaf, const uint8_t* ext, const uint32_t* limits, uint32_t* ids, uint8_t* status) {
  return ((HostLedger*)h)->draw(n, leaf, ext, limits, nullptr, ids, status);
}
int qs_draw_counts(void* h, size_t n, const uint64_t* leaf, const uint8_t* ext, const uint32_t* limits, const uint8_t* counts,
                   uint32_t* firsts, uint8_t* status) {
  return ((HostLedger*)h)->draw(n, leaf, ext, limits, counts, firsts, status);
}
void qs_info(void* h, uint64_t out[8]) { ((HostLedger*)h)->st.info(out); }
// the window in the order it was given: k elements to ext_out, their slots to slots_out
size_t qs_window(void* hv, uint8_t* ext_out, uint32_t* slots_out) {
  const quota::Window& W = ((HostLedger*)hv)->L.window;
  for (uint32_t j = 0; j < W.k; j++) {
    memcpy(ext_out + 32 * j, W.e[W.order[j]].w, 32);
    slots_out[j] = W.order[j];
  }
  return W.k;
}
// every counter that is not zero, as (key, used) words in key order; returns their number (at most cap are written)
size_t qs_counters(void* hv, uint32_t* out, size_t cap) {
  const quota::SeqLedger& L = ((HostLedger*)hv)->L;
  size_t m = 0;
  for (uint32_t s = 0; s < L.max_epochs; s++)
    for (size_t leaf = 0; leaf < (size_t)1 << L.depth; leaf++) {
      const uint32_t used = L.used[((size_t)s << L.depth) + leaf];
      if (!used) continue;
      if (m < cap) out[2 * m] = quota::pack_key(s, (uint32_t)leaf), out[2 * m + 1] = used;
      m++;
    }
  return m;
}

}  // extern "C"
