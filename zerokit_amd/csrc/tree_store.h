// tree_store.h -- the durable store behind a persistent membership tree: a checksummed snapshot plus a write-ahead
// journal, in the directory the config names.  Pure host code with no HIP call and no other header of this library, so
// the CPU suite builds it with g++ and the sanitizers (tests/host/treestore.cpp, treestore_main.cpp).  It deals in files
// and in a host image of the tree (next index, metadata bytes, next index x 32 bytes of canonical LE leaves); ffi.cpp
// feeds the device from that image and hands leaves and root back for a compaction.
//
//   <dir>/rlnamd_tree.bin   snapshot, form RLNAMDT2:
//       magic[8] | depth u64 | next u64 | meta_len u64 | generation u64 | root[32] | meta | leaves | CRC-32C u32
//     (the CRC covers every byte before it; a root of 32 zero bytes means "none recorded").  The older form RLNAMDT1
//     (magic | depth | next | meta_len | meta | leaves: no generation, no root, no checksum) still opens, as
//     generation 0; the first compaction rewrites it as T2.
//   <dir>/rlnamd_tree.wal   journal:
//       header  magic[8] "RLNAMDW1" | depth u64 | generation u64 | CRC-32C u32
//       record  length u64 | payload | CRC-32C(length, payload) u32
//       payload kind u8 | next_after u64 | ...
//                 1 range    start u64 | n u64 | n x 32 leaf bytes
//                 2 scatter  k u64 | k x index u64 | k x 32 leaf bytes
//                 3 metadata len u64 | bytes
//     One record per mutating call, appended BEFORE the call touches the tree, so a call is all or nothing after a crash.
//
// A journal belongs to the snapshot of the same generation; any other one is what a crash between the two renames of a
// compaction leaves behind, and is replaced.  Replay stops at the first record that is short or fails its CRC; the file
// is cut there (a torn tail is the normal shape of a crash).  All integers are little-endian.
//
// Syncs: sync() is an fdatasync of the journal.  A flusher thread per store wakes every flush_every_ms and syncs when
// something was appended since; with flush_every_ms = 0 there is no thread and every append syncs before it returns.
// The thread does file I/O only, under the store's own mutex.
//
// Exclusive use: flock(LOCK_EX | LOCK_NB) on the journal's descriptor while the store is open.  A compaction creates the
// next journal beside the old one and locks it before the rename, so the path never names an unlocked file.
#pragma once
#include <errno.h>
#include <fcntl.h>
#include <poll.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

namespace rlnamd {
namespace tstore {

struct StoreError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// CRC-32C (Castagnoli, reflected polynomial 0x82F63B78), software tables, eight bytes a step (a snapshot of 2^20 leaves is
// 32 MiB, summed on every open and every compaction); crc32c("123456789") = 0xE3069283.  `crc` continues an earlier
// call's result.
inline uint32_t crc32c(const void* data, size_t n, uint32_t crc = 0) {
  static const struct Table {
    uint32_t t[8][256];
    Table() {
      for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1) ? 0x82F63B78u : 0u);
        t[0][i] = c;
      }
      for (uint32_t i = 0; i < 256; i++)
        for (int k = 1; k < 8; k++) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 0xFF];
    }
  } T;
  const uint8_t* p = (const uint8_t*)data;
  crc = ~crc;
  for (; n >= 8; n -= 8, p += 8) {
    const uint32_t lo = crc ^ ((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
    crc = T.t[7][lo & 0xFF] ^ T.t[6][(lo >> 8) & 0xFF] ^ T.t[5][(lo >> 16) & 0xFF] ^ T.t[4][lo >> 24] ^ T.t[3][p[4]] ^
          T.t[2][p[5]] ^ T.t[1][p[6]] ^ T.t[0][p[7]];
  }
  for (size_t i = 0; i < n; i++) crc = T.t[0][(crc ^ p[i]) & 0xFF] ^ (crc >> 8);
  return ~crc;
}

inline void put_u32(uint8_t* p, uint32_t v) { for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i)); }
inline void put_u64(uint8_t* p, uint64_t v) { for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i)); }
inline uint32_t get_u32(const uint8_t* p) { uint32_t v = 0; for (int i = 0; i < 4; i++) v |= (uint32_t)p[i] << (8 * i); return v; }
inline uint64_t get_u64(const uint8_t* p) { uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)p[i] << (8 * i); return v; }

constexpr size_t SNAP_HEADER = 8 + 4 * 8 + 32;   // T2
constexpr size_t SNAP_HEADER_T1 = 8 + 3 * 8;
constexpr size_t WAL_HEADER = 8 + 8 + 8 + 4;
constexpr size_t REC_FRAME = 8 + 4;              // length + CRC around a payload
constexpr uint64_t MAX_META = (uint64_t)1 << 30;
constexpr const char* DEPTH_MISMATCH = "Merkle tree error: Tree depth exceeds maximum allowed (must be < 64)";

// the tree as the host sees it
struct Image {
  uint64_t depth = 0, next = 0, generation = 0;
  bool has_root = false;   // a T2 snapshot that recorded one
  uint8_t root[32] = {0};
  std::vector<uint8_t> meta, leaves;   // leaves.size() == next * 32
};

struct Options {
  uint64_t flush_every_ms = 500;    // the reference's default (pm_tree_adapter.rs:69); 0: every append syncs
  uint64_t journal_max_bytes = 0;   // compaction threshold; 0: max(1 MiB, bytes of the current snapshot)
};

enum { INFO_GENERATION, INFO_JOURNAL_BYTES, INFO_RECORDS, INFO_SYNCS, INFO_COMPACTIONS, INFO_REPLAYED, INFO_TORN, INFO_UNSYNCED };

// One journal record applied to the image; false (image untouched) when the payload is not a well-formed record for a
// tree of this depth.  A record that passed its CRC and fails here was not written by this code; replay stops at it.
inline bool apply_payload(Image& im, const uint8_t* p, uint64_t len) {
  if (len < 1 + 8 + 8) return false;
  const uint8_t kind = p[0];
  const uint64_t next_after = get_u64(p + 1), a = get_u64(p + 9), cap = (uint64_t)1 << im.depth;
  const uint8_t* body = p + 17;
  const uint64_t left = len - 17;
  if (next_after > cap || next_after < im.next) return false;
  auto grow = [&]() {
    im.leaves.resize(next_after * 32, 0);
    im.next = next_after;
  };
  if (kind == 1) {   // range: a = start, then n
    if (left < 8) return false;
    const uint64_t n = get_u64(body);
    if (n > cap || a > cap - n || a + n > next_after || (left - 8) / 32 != n || (left - 8) % 32) return false;
    grow();
    if (n) memcpy(im.leaves.data() + a * 32, body + 8, n * 32);
    return true;
  }
  if (kind == 2) {   // scatter: a = k
    if (a > cap || left / 40 != a || left % 40) return false;
    for (uint64_t i = 0; i < a; i++)
      if (get_u64(body + 8 * i) >= next_after) return false;
    grow();
    for (uint64_t i = 0; i < a; i++) memcpy(im.leaves.data() + get_u64(body + 8 * i) * 32, body + 8 * a + 32 * i, 32);
    return true;
  }
  if (kind == 3) {   // metadata: a = len
    if (a > MAX_META || left != a) return false;
    grow();
    im.meta.assign(body, body + a);
    return true;
  }
  return false;
}

class TreeStore {
 public:
  TreeStore() = default;
  TreeStore(const TreeStore&) = delete;
  TreeStore& operator=(const TreeStore&) = delete;
  ~TreeStore() { close(); }

  // Takes the lock, loads snapshot + journal into `im` (an empty generation-1 store is created when there is none) and
  // leaves the journal open for appends.  Throws StoreError; nothing stays open or locked then.
  void open(const std::string& dir, uint64_t depth, const Options& opt, Image& im) {
    close();
    std::lock_guard<std::mutex> g(mu_);
    try {
      open_locked(dir, depth, opt, im);
    } catch (...) {
      drop_fd();
      throw;
    }
  }
  // the timed syncs; a second call, or flush_every_ms = 0, starts nothing
  void start_flusher() {
    std::lock_guard<std::mutex> g(mu_);
    if (fd_ < 0 || opt_.flush_every_ms == 0 || flusher_.joinable()) return;
    if (pipe2(wake_, O_CLOEXEC) != 0) throw io_error("start the flusher of", dir_);
    stop_ = false;
    // The thread sleeps in poll() on a pipe, not in a timed wait on the mutex: the timeout runs on the monotonic clock,
    // and close() ends the sleep by writing a byte.
    const int wake = wake_[0], period = (int)std::min<uint64_t>(opt_.flush_every_ms, 3600000);
    flusher_ = std::thread([this, wake, period]() {
      for (;;) {
        struct pollfd p = {wake, POLLIN, 0};
        const int rc = poll(&p, 1, period);
        if (rc > 0 || (rc < 0 && errno != EINTR)) return;
        std::lock_guard<std::mutex> g(mu_);
        if (stop_) return;
        if (fd_ >= 0 && unsynced_ > 0 && fdatasync(fd_) == 0) {   // (a failing sync is met again by the next sync())
          unsynced_ = 0;
          syncs_++;
        }
      }
    });
  }
  // stops and joins the flusher, syncs what it has not, closes the journal (which releases the lock)
  void close() {
    {
      std::lock_guard<std::mutex> g(mu_);
      stop_ = true;
    }
    if (flusher_.joinable()) {
      const char byte = 0;
      while (write(wake_[1], &byte, 1) < 0 && errno == EINTR) {
      }
      flusher_.join();
      ::close(wake_[0]);
      ::close(wake_[1]);
      wake_[0] = wake_[1] = -1;
    }
    std::lock_guard<std::mutex> g(mu_);
    if (fd_ >= 0 && unsynced_ > 0 && fdatasync(fd_) == 0) syncs_++;
    drop_fd();
  }
  bool is_open() const {
    std::lock_guard<std::mutex> g(mu_);
    return fd_ >= 0;
  }

  void append_range(uint64_t start, uint64_t n, const uint8_t* leaves, uint64_t next_after) {
    std::vector<uint8_t> rec = frame(1 + 8 + 8 + 8 + n * 32);
    uint8_t* p = rec.data() + 8;
    p[0] = 1;
    put_u64(p + 1, next_after);
    put_u64(p + 9, start);
    put_u64(p + 17, n);
    if (n) memcpy(p + 25, leaves, n * 32);
    append(rec);
  }
  void append_scatter(uint64_t k, const uint64_t* idx, const uint8_t* leaves, uint64_t next_after) {
    std::vector<uint8_t> rec = frame(1 + 8 + 8 + k * 40);
    uint8_t* p = rec.data() + 8;
    p[0] = 2;
    put_u64(p + 1, next_after);
    put_u64(p + 9, k);
    for (uint64_t i = 0; i < k; i++) put_u64(p + 17 + 8 * i, idx[i]);
    if (k) memcpy(p + 17 + 8 * k, leaves, k * 32);
    append(rec);
  }
  void append_metadata(const uint8_t* meta, uint64_t len, uint64_t next_after) {
    if (len > MAX_META) throw StoreError("Merkle tree error: metadata of " + std::to_string(len) + " bytes is too long to store");
    std::vector<uint8_t> rec = frame(1 + 8 + 8 + len);
    uint8_t* p = rec.data() + 8;
    p[0] = 3;
    put_u64(p + 1, next_after);
    put_u64(p + 9, len);
    if (len) memcpy(p + 17, meta, len);
    append(rec);
  }
  // the journal's end: what rollback() takes to undo the append that follows
  uint64_t journal_bytes() const {
    std::lock_guard<std::mutex> g(mu_);
    return wal_bytes_;
  }
  uint64_t records() const {
    std::lock_guard<std::mutex> g(mu_);
    return records_;
  }
  // undoes the last append (the call it recorded failed on the tree): the journal is cut back to `offset`
  void rollback(uint64_t offset) {
    std::lock_guard<std::mutex> g(mu_);
    if (fd_ < 0 || offset >= wal_bytes_ || offset < WAL_HEADER) return;
    if (ftruncate(fd_, (off_t)offset) != 0 || fdatasync(fd_) != 0) {
      broken_ = "cannot take back a record of " + wal_path();
      return;
    }
    syncs_++;
    unsynced_ = 0;
    wal_bytes_ = offset;
    if (records_) records_--;
  }
  void sync() {
    std::lock_guard<std::mutex> g(mu_);
    sync_locked();
  }
  bool wants_compaction() const {
    std::lock_guard<std::mutex> g(mu_);
    const uint64_t limit = opt_.journal_max_bytes ? opt_.journal_max_bytes : std::max<uint64_t>((uint64_t)1 << 20, snap_bytes_);
    return fd_ >= 0 && records_ > 0 && wal_bytes_ > limit;
  }
  // the whole tree (leaves: next x 32 bytes) as the snapshot of the next generation, then an empty journal of that
  // generation.  A failure before the snapshot's rename changes nothing; one after it leaves the store refusing
  // appends, since the journal it holds is stale by then.
  void compact(uint64_t next, const uint8_t* meta, uint64_t meta_len, const uint8_t* leaves, const uint8_t root[32]) {
    std::lock_guard<std::mutex> g(mu_);
    require_open();
    write_snapshot(generation_ + 1, next, meta, meta_len, leaves, root);
    generation_++;
    records_ = 0;
    try {
      replace_journal();
    } catch (const StoreError& e) {
      broken_ = e.what();
      throw;
    }
    compactions_++;
  }
  void info(uint64_t out[8]) const {
    std::lock_guard<std::mutex> g(mu_);
    out[INFO_GENERATION] = generation_;
    out[INFO_JOURNAL_BYTES] = wal_bytes_;
    out[INFO_RECORDS] = records_;
    out[INFO_SYNCS] = syncs_;
    out[INFO_COMPACTIONS] = compactions_;
    out[INFO_REPLAYED] = replayed_;
    out[INFO_TORN] = torn_;
    out[INFO_UNSYNCED] = unsynced_;
  }
  const std::string& dir() const { return dir_; }
  std::string snap_path() const { return dir_ + "/rlnamd_tree.bin"; }
  std::string wal_path() const { return dir_ + "/rlnamd_tree.wal"; }

 private:
  mutable std::mutex mu_;
  std::thread flusher_;
  int wake_[2] = {-1, -1};   // the pipe that ends the flusher's sleep
  bool stop_ = false;
  std::string dir_, broken_;
  Options opt_;
  int fd_ = -1;   // the journal: open, locked, written with pwrite at wal_bytes_
  uint64_t depth_ = 0, generation_ = 0, wal_bytes_ = 0, records_ = 0, syncs_ = 0, compactions_ = 0, replayed_ = 0, torn_ = 0,
           unsynced_ = 0, snap_bytes_ = 0;

  static StoreError io_error(const std::string& what, const std::string& file) {
    return StoreError("Merkle tree error: cannot " + what + " " + file + ": " + strerror(errno));
  }
  void drop_fd() {
    if (fd_ >= 0) ::close(fd_);
    fd_ = -1;
  }
  void require_open() const {
    if (fd_ < 0) throw StoreError("Merkle tree error: store " + dir_ + " is not open");
    if (!broken_.empty()) throw StoreError("Merkle tree error: store " + dir_ + " takes no more writes after: " + broken_);
  }
  static std::vector<uint8_t> frame(uint64_t payload) {
    std::vector<uint8_t> rec(8 + payload + 4);
    put_u64(rec.data(), payload);
    return rec;
  }
  static bool write_all(int fd, const uint8_t* p, size_t n, off_t at) {
    while (n) {
      ssize_t k = pwrite(fd, p, n, at);
      if (k < 0 && errno == EINTR) continue;
      if (k <= 0) {
        if (k == 0) errno = ENOSPC;
        return false;
      }
      p += k;
      n -= (size_t)k;
      at += k;
    }
    return true;
  }
  static bool read_all(int fd, uint8_t* p, size_t n, off_t at) {
    while (n) {
      ssize_t k = pread(fd, p, n, at);
      if (k < 0 && errno == EINTR) continue;
      if (k <= 0) return false;
      p += k;
      n -= (size_t)k;
      at += k;
    }
    return true;
  }
  void sync_dir() const {
    int d = ::open(dir_.c_str(), O_RDONLY | O_DIRECTORY);
    if (d < 0) throw io_error("open", dir_);
    const int rc = fsync(d);
    ::close(d);
    if (rc != 0) throw io_error("sync", dir_);
  }
  void sync_locked() {
    require_open();
    if (fdatasync(fd_) != 0) throw io_error("sync", wal_path());
    unsynced_ = 0;
    syncs_++;
  }
  void append(std::vector<uint8_t>& rec) {
    put_u32(rec.data() + rec.size() - 4, crc32c(rec.data(), rec.size() - 4));
    std::lock_guard<std::mutex> g(mu_);
    require_open();
    if (!write_all(fd_, rec.data(), rec.size(), (off_t)wal_bytes_)) {
      const int e = errno;
      if (ftruncate(fd_, (off_t)wal_bytes_) != 0) broken_ = "a short write to " + wal_path();
      errno = e;
      throw io_error("append to", wal_path());
    }
    wal_bytes_ += rec.size();
    unsynced_ += rec.size();
    records_++;
    if (opt_.flush_every_ms == 0) {
      if (fdatasync(fd_) != 0) {   // the record is not durable: take it back, the call fails
        const int e = errno;
        wal_bytes_ -= rec.size();
        records_--;
        unsynced_ = 0;
        if (ftruncate(fd_, (off_t)wal_bytes_) != 0) broken_ = "a failed sync of " + wal_path();
        errno = e;
        throw io_error("sync", wal_path());
      }
      unsynced_ = 0;
      syncs_++;
    }
  }

  // written to <file>.tmp, synced, renamed into place, directory synced
  void write_snapshot(uint64_t generation, uint64_t next, const uint8_t* meta, uint64_t meta_len, const uint8_t* leaves,
                      const uint8_t root[32]) {
    const std::string file = snap_path(), tmp = file + ".tmp";
    int f = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (f < 0) throw io_error("write", tmp);
    uint8_t h[SNAP_HEADER];
    memcpy(h, "RLNAMDT2", 8);
    put_u64(h + 8, depth_);
    put_u64(h + 16, next);
    put_u64(h + 24, meta_len);
    put_u64(h + 32, generation);
    memcpy(h + 40, root, 32);
    uint32_t crc = crc32c(h, sizeof h);
    crc = crc32c(meta, meta_len, crc);
    crc = crc32c(leaves, next * 32, crc);
    uint8_t tail[4];
    put_u32(tail, crc);
    const off_t meta_at = sizeof h, leaves_at = meta_at + (off_t)meta_len, tail_at = leaves_at + (off_t)(next * 32);
    int e = 0;   // the first failure's errno
    if (!write_all(f, h, sizeof h, 0) || !write_all(f, meta, meta_len, meta_at) || !write_all(f, leaves, next * 32, leaves_at) ||
        !write_all(f, tail, 4, tail_at) || fsync(f) != 0)
      e = errno ? errno : EIO;
    if (::close(f) != 0 && !e) e = errno ? errno : EIO;
    if (!e && rename(tmp.c_str(), file.c_str()) != 0) e = errno ? errno : EIO;
    if (e) {
      unlink(tmp.c_str());
      errno = e;
      throw io_error("write", file);
    }
    sync_dir();
    snap_bytes_ = (uint64_t)tail_at + 4;
  }
  // an empty journal of generation_ beside the current one, locked before it takes the name; then the old one goes
  void replace_journal() {
    const std::string file = wal_path(), tmp = file + ".tmp";
    int f = ::open(tmp.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0666);
    if (f < 0) throw io_error("write", tmp);
    uint8_t h[WAL_HEADER];
    memcpy(h, "RLNAMDW1", 8);
    put_u64(h + 8, depth_);
    put_u64(h + 16, generation_);
    put_u32(h + 24, crc32c(h, 24));
    if (flock(f, LOCK_EX | LOCK_NB) != 0 || !write_all(f, h, sizeof h, 0) || fsync(f) != 0 ||
        rename(tmp.c_str(), file.c_str()) != 0) {
      const int e = errno;
      ::close(f);
      unlink(tmp.c_str());
      errno = e;
      throw io_error("write", file);
    }
    drop_fd();
    fd_ = f;
    wal_bytes_ = WAL_HEADER;
    records_ = 0;
    unsynced_ = 0;
    sync_dir();
  }

  void read_snapshot(uint64_t depth, Image& im, bool& found) {
    const std::string file = snap_path();
    int f = ::open(file.c_str(), O_RDONLY);
    found = f >= 0;
    if (!found) {
      if (errno != ENOENT) throw io_error("read", file);
      return;
    }
    struct Closer {
      int f;
      ~Closer() { ::close(f); }
    } closer{f};
    const StoreError not_ours("Merkle tree error: " + file + " is corrupt (not a tree snapshot of this library)");
    const StoreError bad_sum("Merkle tree error: " + file + " is corrupt (checksum)");
    struct stat st;
    if (fstat(f, &st) != 0) throw io_error("read", file);
    const uint64_t size = (uint64_t)st.st_size;
    uint8_t h[SNAP_HEADER];
    if (size < SNAP_HEADER_T1 || !read_all(f, h, SNAP_HEADER_T1, 0)) throw not_ours;
    const bool t2 = !memcmp(h, "RLNAMDT2", 8);
    if (!t2 && memcmp(h, "RLNAMDT1", 8)) throw not_ours;
    const size_t hs = t2 ? SNAP_HEADER : SNAP_HEADER_T1;
    if (t2 && (size < SNAP_HEADER + 4 || !read_all(f, h, SNAP_HEADER, 0))) throw bad_sum;
    const uint64_t d = get_u64(h + 8), next = get_u64(h + 16), meta_len = get_u64(h + 24);
    // the sizes a header claims are held against the file's before anything is allocated
    const bool sane = d < 64 && next <= ((uint64_t)1 << d) && d <= 40 && meta_len <= MAX_META &&
                      (t2 ? size == hs + meta_len + next * 32 + 4 : size >= hs + meta_len + next * 32);
    if (!sane) throw t2 ? bad_sum : not_ours;
    im.meta.resize(meta_len);
    im.leaves.resize(next * 32);
    if ((meta_len && !read_all(f, im.meta.data(), meta_len, (off_t)hs)) ||
        (next && !read_all(f, im.leaves.data(), next * 32, (off_t)(hs + meta_len))))
      throw t2 ? bad_sum : not_ours;
    if (t2) {
      uint8_t tail[4];
      if (!read_all(f, tail, 4, (off_t)(size - 4))) throw bad_sum;
      uint32_t crc = crc32c(h, SNAP_HEADER);
      crc = crc32c(im.meta.data(), meta_len, crc);
      crc = crc32c(im.leaves.data(), next * 32, crc);
      if (crc != get_u32(tail)) throw bad_sum;
      im.generation = get_u64(h + 32);
      memcpy(im.root, h + 40, 32);
      static const uint8_t zero[32] = {0};
      im.has_root = memcmp(im.root, zero, 32) != 0;
    }
    if (d != depth) throw StoreError(DEPTH_MISMATCH);
    im.depth = d;
    im.next = next;
    snap_bytes_ = size;
  }

  void open_locked(const std::string& dir, uint64_t depth, const Options& opt, Image& im) {
    dir_ = dir;
    opt_ = opt;
    depth_ = depth;
    broken_.clear();
    generation_ = wal_bytes_ = records_ = syncs_ = compactions_ = replayed_ = torn_ = unsynced_ = snap_bytes_ = 0;
    im = Image();
    im.depth = depth;
    if (depth >= 64) throw StoreError(DEPTH_MISMATCH);
    if (mkdir(dir.c_str(), 0777) != 0 && errno != EEXIST) throw io_error("create", dir);
    // the lock first: nothing of a store in use is touched.  The name may pass to another file while we wait for it
    // (a compaction's rename), so the locked descriptor must still be the file the name leads to.
    const std::string wal = wal_path();
    for (int tries = 0;; tries++) {
      fd_ = ::open(wal.c_str(), O_RDWR | O_CREAT, 0666);
      if (fd_ < 0) throw io_error("open", wal);
      if (flock(fd_, LOCK_EX | LOCK_NB) != 0) {
        if (errno == EWOULDBLOCK) throw StoreError("Merkle tree error: store " + dir + " is in use");
        throw io_error("lock", wal);
      }
      struct stat a, b;
      if (fstat(fd_, &a) == 0 && stat(wal.c_str(), &b) == 0 && a.st_ino == b.st_ino && a.st_dev == b.st_dev) break;
      drop_fd();
      if (tries == 8) throw StoreError("Merkle tree error: store " + dir + " is in use");
    }
    unlink((snap_path() + ".tmp").c_str());
    unlink((wal + ".tmp").c_str());

    bool found = false;
    read_snapshot(depth, im, found);
    generation_ = im.generation;
    if (!found) {
      static const uint8_t zero[32] = {0};
      generation_ = im.generation = 1;
      write_snapshot(1, 0, nullptr, 0, nullptr, zero);
    }

    // the journal: ours (header intact, this depth, this generation) is replayed; anything else is replaced
    struct stat st;
    if (fstat(fd_, &st) != 0) throw io_error("read", wal);
    const uint64_t size = (uint64_t)st.st_size;
    uint8_t h[WAL_HEADER];
    const bool header_ok = size >= WAL_HEADER && read_all(fd_, h, WAL_HEADER, 0) && !memcmp(h, "RLNAMDW1", 8) &&
                           crc32c(h, 24) == get_u32(h + 24);
    if (!header_ok || get_u64(h + 8) != depth || get_u64(h + 16) != generation_) {
      if (!header_ok) torn_ = size;   // (a stale journal is whole, and its records are in the snapshot already)
      replace_journal();
      return;
    }
    uint64_t at = WAL_HEADER;
    std::vector<uint8_t> rec;
    while (size - at >= REC_FRAME) {
      uint8_t lenb[8];
      if (!read_all(fd_, lenb, 8, (off_t)at)) break;
      const uint64_t len = get_u64(lenb);
      if (len > size - at - REC_FRAME) break;
      rec.resize(8 + len + 4);
      memcpy(rec.data(), lenb, 8);
      if (!read_all(fd_, rec.data() + 8, len + 4, (off_t)(at + 8))) break;
      if (crc32c(rec.data(), 8 + len) != get_u32(rec.data() + 8 + len)) break;
      if (!apply_payload(im, rec.data() + 8, len)) break;
      at += REC_FRAME + len;
      replayed_++;
    }
    if (at < size) {
      if (ftruncate(fd_, (off_t)at) != 0 || fdatasync(fd_) != 0) throw io_error("truncate", wal);
      torn_ = size - at;
    }
    wal_bytes_ = at;
    records_ = replayed_;
    if (replayed_) im.has_root = false;   // the stored root is the snapshot's, not this tree's
  }
};

}  // namespace tstore
}  // namespace rlnamd
