// CPU build of the durable tree store (zerokit_amd/csrc/tree_store.h) for tests/test_tree_store_host.py.  Built with g++:
// the header makes no HIP call.  HostTree stands where ffi.cpp's FFI_RLN stands on the device side: it validates a call,
// appends its record, applies it to the tree -- here the host image itself -- and compacts when the store asks for it.
// The "root" it hands to a compaction is a digest of the image (CRC-32C under eight prefixes), so that the stored-root
// check of an open can be mirrored without Poseidon.  tests/host/treestore_main.cpp includes this file for the
// stand-alone programs.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "tree_store.h"

namespace {

using namespace rlnamd::tstore;

struct HostTree {
  TreeStore st;
  Image im;
  std::string err;

  uint64_t cap() const { return (uint64_t)1 << im.depth; }
  static void digest(const Image& im, uint8_t out[32]) {
    for (uint32_t k = 0; k < 8; k++) {
      uint32_t c = crc32c(&k, 4);
      c = crc32c(im.meta.data(), im.meta.size(), c);
      c = crc32c(im.leaves.data(), im.leaves.size(), c);
      put_u32(out + 4 * k, c);
    }
    out[0] |= 1;   // never the all-zero "none recorded"
  }
  void grow(uint64_t next_after) {
    im.leaves.resize(next_after * 32, 0);
    im.next = next_after;
  }
  void compact_now() {
    uint8_t root[32];
    digest(im, root);
    st.compact(im.next, im.meta.data(), im.meta.size(), im.leaves.data(), root);
  }
  void after_append() {
    if (st.wants_compaction()) compact_now();
  }
  // 0: done; 1: refused before anything was written (the index check of the FFI); 2: the store failed (err says how)
  int set_range(uint64_t start, uint64_t n, const uint8_t* leaves) {
    if (n > cap() || start > cap() - n) return 1;
    if (!n) return 0;
    try {
      const uint64_t next_after = std::max(im.next, start + n);
      st.append_range(start, n, leaves, next_after);
      grow(next_after);
      memcpy(im.leaves.data() + 32 * start, leaves, 32 * n);
      after_append();
    } catch (const std::exception& e) {
      err = e.what();
      return 2;
    }
    return 0;
  }
  int set_scatter(uint64_t k, const uint64_t* idx, const uint8_t* leaves) {
    uint64_t next_after = im.next;
    for (uint64_t i = 0; i < k; i++) {
      if (idx[i] >= cap()) return 1;
      next_after = std::max(next_after, idx[i] + 1);
    }
    if (!k) return 0;
    try {
      st.append_scatter(k, idx, leaves, next_after);
      grow(next_after);
      for (uint64_t i = 0; i < k; i++) memcpy(im.leaves.data() + 32 * idx[i], leaves + 32 * i, 32);
      after_append();
    } catch (const std::exception& e) {
      err = e.what();
      return 2;
    }
    return 0;
  }
  int set_meta(const uint8_t* meta, uint64_t len) {
    try {
      st.append_metadata(meta, len, im.next);
      im.meta.assign(meta, meta + len);
      after_append();
    } catch (const std::exception& e) {
      err = e.what();
      return 2;
    }
    return 0;
  }
};

HostTree* host_open(const char* dir, uint64_t depth, uint64_t flush_every_ms, uint64_t journal_max_bytes, int flusher,
                    std::string& err) {
  HostTree* t = new HostTree;
  try {
    Options opt;
    opt.flush_every_ms = flush_every_ms;
    opt.journal_max_bytes = journal_max_bytes;
    t->st.open(dir, depth, opt, t->im);
    if (t->im.has_root) {   // what ffi.cpp does with the device's root after the upload
      uint8_t root[32];
      HostTree::digest(t->im, root);
      if (memcmp(root, t->im.root, 32)) throw StoreError("Merkle tree error: " + t->st.snap_path() + " is corrupt (root)");
    }
    if (flusher) t->st.start_flusher();
    return t;
  } catch (const std::exception& e) {
    err = e.what();
    delete t;
    return nullptr;
  }
}

}  // namespace

extern "C" {

uint32_t ts_crc32c(const uint8_t* p, size_t n) { return crc32c(p, n); }
void* ts_open(const char* dir, uint64_t depth, uint64_t flush_every_ms, uint64_t journal_max_bytes, int flusher, char* err,
              size_t err_len) {
  std::string e;
  HostTree* t = host_open(dir, depth, flush_every_ms, journal_max_bytes, flusher, e);
  if (!t && err && err_len) snprintf(err, err_len, "%s", e.c_str());
  return t;
}
// compact = 1: what freeing the FFI object does (compact when the journal holds a record); 0: the store is just dropped
int ts_close(void* h, int compact) {
  HostTree* t = (HostTree*)h;
  int rc = 0;
  try {
    if (compact && t->st.records() > 0) t->compact_now();
  } catch (const std::exception&) {
    rc = 2;
  }
  delete t;
  return rc;
}
int ts_set_range(void* h, uint64_t start, uint64_t n, const uint8_t* leaves) { return ((HostTree*)h)->set_range(start, n, leaves); }
int ts_set_scatter(void* h, uint64_t k, const uint64_t* idx, const uint8_t* leaves) {
  return ((HostTree*)h)->set_scatter(k, idx, leaves);
}
int ts_set_meta(void* h, const uint8_t* meta, uint64_t len) { return ((HostTree*)h)->set_meta(meta, len); }
int ts_sync(void* h) {
  try {
    ((HostTree*)h)->st.sync();
    return 0;
  } catch (const std::exception& e) {
    ((HostTree*)h)->err = e.what();
    return 2;
  }
}
void ts_info(void* h, uint64_t out[8]) { ((HostTree*)h)->st.info(out); }
const char* ts_error(void* h) { return ((HostTree*)h)->err.c_str(); }
uint64_t ts_next(void* h) { return ((HostTree*)h)->im.next; }
uint64_t ts_meta_len(void* h) { return ((HostTree*)h)->im.meta.size(); }
void ts_state(void* h, uint8_t* leaves, uint8_t* meta) {
  HostTree* t = (HostTree*)h;
  if (!t->im.leaves.empty()) memcpy(leaves, t->im.leaves.data(), t->im.leaves.size());
  if (!t->im.meta.empty()) memcpy(meta, t->im.meta.data(), t->im.meta.size());
}

}  // extern "C"
