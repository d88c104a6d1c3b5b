// quota_store.h -- the durable store behind a quota ledger opened on a directory (rlnamd_quota_open): a checksummed
// snapshot plus a write-ahead journal, the shape of tree_store.h, whose CRC-32C and put_* / get_* helpers it uses.  Pure
// host code with no HIP call: the CPU suite builds it with g++ and the sanitizers (tests/host/quotastore.cpp,
// quotastore_main.cpp) and drives it with quota::SeqLedger.  It deals in files and in a host image of the ledger (the
// window and one entry per non-zero counter); quota_ledger.hip feeds the device from that image, hands it the delta of
// every draw, and gives the counters back, compacted, for a snapshot.
//
//   <dir>/rlnamd_quota.bin   snapshot:
//       magic[8] "RLNAMDQ1" | depth u64 | max_epochs u64 | generation u64 | k u64
//       | k x (slot u64 | ext[32])                    the window in the order set_epochs was given it
//       | per slot of that list: pairs u64 | pairs x (leaf u32 | used u32)    leaves ascending, used != 0
//       | CRC-32C u32                                 over every byte before it
//   <dir>/rlnamd_quota.wal   journal:
//       header  magic[8] "RLNAMDQW" | depth u64 | max_epochs u64 | generation u64 | CRC-32C u32
//       record  length u64 | payload | CRC-32C(length, payload) u32
//       payload kind u8 | ...
//                 1 window   k u64 | k x ext[32]               what set_epochs was called with; replay runs it through
//                                                              quota::next_window, so the slots after replay are the
//                                                              slots the live ledger had
//                 2 advance  m u64 | m x (key u32 | used u32)  key = quota::pack_key(slot, leaf), used the counter's
//                                                              ABSOLUTE value after the draw
//     Applying an advance is image[key] = max(image[key], used): a record is idempotent, and the order of its pairs
//     does not matter.  A pair whose slot is not live in the replayed window, whose leaf is >= 2^depth or whose value is 0,
//     m = 0, or a length that is not what k or m ask for makes a record ill-formed.
// All integers are little-endian.  Files are created with mode 0600, the directory with 0700: the journal shows who
// signs how often, so the directory is as secret as the ledger.  Nothing is encrypted.
//
// Every append is followed by an fdatasync before it returns: a draw's ids leave the call only behind it.  A failed
// write or sync takes the record back (the file is cut to where it was) and throws.
//
// A LEDGER MUST NEVER GO BACKWARDS.  tree_store.h stops replay at the first bad record and cuts the file there; here
// that would drop records from the middle and lower counters below ids that were issued.  The rule of this store:
//   a bad record is one that is short, fails its CRC or is ill-formed;
//   it is a torn tail only if nothing follows it -- the file is then cut there and the open succeeds: an append is
//   synced before the next one starts, so only the last record can be torn, and none of its ids ever left a call;
//   a bad record with something behind it makes the open FAIL, with a text that names the offset.  So do a snapshot
//   that fails its CRC, a journal header that is not intact, and a depth or max_epochs other than the caller's.
// "Something behind it": a record whose CRC holds (it is ill-formed, not damaged) ends where its length says, and any
// byte behind that end counts.  The length of a record whose CRC fails is under that CRC and proves nothing, so the
// bytes behind the record's start are searched for a whole record (a frame whose CRC holds); one found means records
// would be dropped.  The search is looser than the extent in one direction, and on purpose: a record whose CRC fails
// with nothing but bytes that form no whole record behind it is cut as a torn tail, whatever its length field claims --
// a torn last record and a flip in the last record look just like that, and nothing a call returned lies behind it.
// A tail of zero bytes alone is what a file system may leave of an append that was never synced.
// There is no flag that opens a damaged store anyway: removing the directory is the operator's decision.
//
// A journal belongs to the snapshot of the same generation; one of another generation is what a crash between the two
// renames of a compaction leaves behind, and is replaced.  A compaction is tree_store.h's: the next generation's
// snapshot in a tmp file, fsync, rename, directory fsync; a new journal created and locked before its rename.
//
// Exclusive use: flock(LOCK_EX | LOCK_NB) on the journal's descriptor while the store is open.  Not thread-safe: the
// ledger's handle serialises the calls.
#pragma once
#include <dirent.h>

#include <functional>
#include <map>
#include <string>
#include <vector>

#include "quota_ledger.h"
#include "tree_store.h"

namespace rlnamd {
namespace qstore {

using tstore::crc32c;
using tstore::get_u32;
using tstore::get_u64;
using tstore::put_u32;
using tstore::put_u64;
using tstore::StoreError;

constexpr size_t SNAP_HEADER = 8 + 4 * 8;
constexpr size_t WAL_HEADER = 8 + 3 * 8 + 4;
constexpr size_t REC_FRAME = tstore::REC_FRAME;
constexpr uint8_t REC_WINDOW = 1, REC_ADVANCE = 2;
constexpr const char* SNAP_NAME = "rlnamd_quota.bin";
constexpr const char* WAL_NAME = "rlnamd_quota.wal";

enum { INFO_GENERATION, INFO_JOURNAL_BYTES, INFO_RECORDS, INFO_SYNCS, INFO_COMPACTIONS, INFO_REPLAYED, INFO_TORN, INFO_RESTORED };

// the ledger as the host sees it: the window, and used[key] for every counter that is not zero
struct Image {
  uint32_t depth = 0, max_epochs = 0;
  uint64_t generation = 0;
  quota::Window window;
  std::map<uint32_t, uint32_t> used;   // quota::pack_key(slot, leaf) -> the next id
};

inline void wipe(std::vector<uint8_t>& v) {   // who signs how often: not left on the heap
  volatile uint8_t* p = v.data();
  for (size_t i = 0; i < v.size(); i++) p[i] = 0;
}

inline void drop_slot(Image& im, uint32_t slot) {
  im.used.erase(im.used.lower_bound(quota::pack_key(slot, 0)), im.used.lower_bound(quota::pack_key(slot + 1, 0)));
}

// the two lengths a payload's first count allows: what the search for a whole record and apply_payload both hold to
inline bool payload_shape(const uint8_t* p, uint64_t len) {
  if (len < 9) return false;
  const uint64_t c = get_u64(p + 1);
  if (p[0] == REC_WINDOW) return c <= quota::EPOCHS_MAX && len == 9 + 32 * c;
  if (p[0] == REC_ADVANCE) return c >= 1 && c <= (len - 9) / 8 && len == 9 + 8 * c;
  return false;
}

// One journal record applied to the image; false (image untouched) when the payload is ill-formed for this ledger.
inline bool apply_payload(Image& im, const uint8_t* p, uint64_t len) {
  if (!payload_shape(p, len)) return false;
  const uint64_t c = get_u64(p + 1);
  const uint8_t* body = p + 9;
  if (p[0] == REC_WINDOW) {
    if (c > im.max_epochs || !quota::epochs_refusal(body, c, im.max_epochs).empty()) return false;
    uint64_t leaving = 0;
    im.window = quota::next_window(im.window, body, c, im.max_epochs, &leaving);
    for (uint32_t s = 0; s < im.max_epochs; s++)
      if ((leaving >> s) & 1) drop_slot(im, s);
    return true;
  }
  for (uint64_t i = 0; i < c; i++) {
    const uint32_t key = get_u32(body + 8 * i), slot = quota::key_slot(key);
    if (slot >= im.max_epochs || !((im.window.live >> slot) & 1) || (quota::key_leaf(key) >> im.depth) || get_u32(body + 8 * i + 4) == 0)
      return false;
  }
  for (uint64_t i = 0; i < c; i++) {
    uint32_t& used = im.used[get_u32(body + 8 * i)];
    used = std::max(used, get_u32(body + 8 * i + 4));
  }
  return true;
}

// a frame whose CRC holds, starting at or behind `from`: the records a cut at a damaged one would drop
inline bool whole_record_behind(const uint8_t* b, uint64_t size, uint64_t from) {
  for (uint64_t o = from; o + REC_FRAME <= size; o++) {
    const uint64_t len = get_u64(b + o);
    if (len > size - o - REC_FRAME || !payload_shape(b + o + 8, len)) continue;
    if (crc32c(b + o, 8 + len) == get_u32(b + o + 8 + len)) return true;
  }
  return false;
}

// The records of a journal (b: the whole file, its header checked already) applied to the image.  *end: where the
// good records end; anything behind it is a torn tail, to be cut.  Throws when a bad record has something behind it.
inline void replay(const uint8_t* b, uint64_t size, Image& im, const std::string& file, uint64_t* end, uint64_t* replayed) {
  uint64_t at = WAL_HEADER;
  *replayed = 0;
  while (at < size) {
    const uint64_t left = size - at;
    uint64_t len = 0;
    bool framed = false, good = false;
    if (left >= REC_FRAME) {
      len = get_u64(b + at);
      framed = len <= left - REC_FRAME && crc32c(b + at, 8 + len) == get_u32(b + at + 8 + len);
      good = framed && apply_payload(im, b + at + 8, len);
    }
    if (good) {
      at += REC_FRAME + len;
      (*replayed)++;
      continue;
    }
    bool zeros = !framed;
    for (uint64_t o = at; zeros && o < size; o++) zeros = b[o] == 0;
    const bool follows = !zeros && (framed ? at + REC_FRAME + len < size : whole_record_behind(b, size, at + 1));
    if (follows)
      throw StoreError("quota ledger: " + file + " is corrupt (a " + (framed ? "record that is ill-formed" : "damaged record") +
                       " at offset " + std::to_string(at) + " with records behind it); the ledger is not opened below ids it has issued");
    break;
  }
  *end = at;
}

// a snapshot's bytes into the image; throws with "corrupt" for anything but a whole snapshot of this library
inline void parse_snapshot(const uint8_t* b, uint64_t size, const std::string& file, Image& im) {
  const StoreError bad_sum("quota ledger: " + file + " is corrupt (checksum)");
  const StoreError bad_form("quota ledger: " + file + " is corrupt (not a ledger snapshot of this library)");
  if (size < SNAP_HEADER + 4) throw bad_sum;
  if (crc32c(b, size - 4) != get_u32(b + size - 4)) throw bad_sum;
  if (memcmp(b, "RLNAMDQ1", 8)) throw bad_form;
  const uint64_t depth = get_u64(b + 8), max_epochs = get_u64(b + 16), k = get_u64(b + 32), body = size - 4;
  if (!quota::new_refusal(depth, max_epochs).empty() || k > max_epochs || body - SNAP_HEADER < 40 * k) throw bad_form;
  im.depth = (uint32_t)depth;
  im.max_epochs = (uint32_t)max_epochs;
  im.generation = get_u64(b + 24);
  im.window = quota::Window();
  im.used.clear();
  uint64_t at = SNAP_HEADER;
  for (uint64_t j = 0; j < k; j++, at += 40) {
    const uint64_t slot = get_u64(b + at);
    if (slot >= max_epochs || ((im.window.live >> slot) & 1) || !nlog::element_is_canonical(b + at + 8)) throw bad_form;
    memcpy(im.window.e[slot].w, b + at + 8, 32);
    im.window.live |= (uint64_t)1 << slot;
    im.window.order[im.window.k++] = (uint32_t)slot;
  }
  for (uint32_t j = 0; j < im.window.k; j++) {
    if (body - at < 8) throw bad_form;
    const uint64_t pairs = get_u64(b + at);
    at += 8;
    if (pairs > ((uint64_t)1 << depth) || (body - at) / 8 < pairs) throw bad_form;
    uint64_t above = 0;   // one more than the leaf before
    for (uint64_t i = 0; i < pairs; i++, at += 8) {
      const uint32_t leaf = get_u32(b + at), used = get_u32(b + at + 4);
      if (leaf < above || (leaf >> depth) || used == 0) throw bad_form;
      above = (uint64_t)leaf + 1;
      im.used.emplace_hint(im.used.end(), quota::pack_key(im.window.order[j], leaf), used);
    }
  }
  if (at != body) throw bad_form;
}

class QuotaStore {
 public:
  // the non-zero counters of one slot as (leaf, used) words, leaves ascending: what a compaction asks its caller for,
  // one slot at a time, in the window's order
  using SlotPairs = std::function<void(uint32_t slot, std::vector<uint32_t>& leaf_used)>;

  QuotaStore() = default;
  QuotaStore(const QuotaStore&) = delete;
  QuotaStore& operator=(const QuotaStore&) = delete;
  ~QuotaStore() { close(); }

  // Takes the lock, loads snapshot + journal into `im` (an empty generation-1 store is created when there is none) and
  // leaves the journal open for appends.  Throws StoreError; nothing stays open or locked then, and a store that was
  // refused for damage is left as it was found.
  void open(const std::string& dir, uint64_t depth, uint64_t max_epochs, uint64_t journal_max_bytes, Image& im) {
    close();
    try {
      open_locked(dir, depth, max_epochs, journal_max_bytes, im);
    } catch (...) {
      drop_fd();
      throw;
    }
  }
  void close() { drop_fd(); }   // (every append was synced when it was made)
  bool is_open() const { return fd_ >= 0; }

  // set_epochs(E), as it was called: appended and synced BEFORE the window is applied
  void append_window(size_t k, const uint8_t* external_nullifiers_le) {
    std::vector<uint8_t> rec(8 + 9 + 32 * k + 4);
    uint8_t* p = rec.data() + 8;
    p[0] = REC_WINDOW;
    put_u64(p + 1, k);
    if (k) memcpy(p + 9, external_nullifiers_le, 32 * k);
    append(rec);
  }
  // the counters a draw moved, m >= 1 (key, used) pairs with the absolute values: appended and synced BEFORE any id of
  // the draw leaves the call
  void append_advance(size_t m, const uint32_t* key_used) {
    std::vector<uint8_t> rec(8 + 9 + 8 * m + 4);
    uint8_t* p = rec.data() + 8;
    p[0] = REC_ADVANCE;
    put_u64(p + 1, m);
    for (size_t i = 0; i < 2 * m; i++) put_u32(p + 9 + 4 * i, key_used[i]);
    append(rec);
  }
  // Nothing more is written: what the ledger did and what the journal says may differ from here on (a set_epochs that
  // failed on the device behind its record).  Reopening settles it.
  void poison(const std::string& why) {
    if (broken_.empty()) broken_ = why;
  }
  void check_writable() const { require_open(); }   // throws what the next append would
  bool has_records() const { return fd_ >= 0 && wal_bytes_ > WAL_HEADER; }
  bool wants_compaction() const {
    const uint64_t limit = journal_max_bytes_ ? journal_max_bytes_ : std::max<uint64_t>((uint64_t)1 << 20, snap_bytes_);
    return has_records() && broken_.empty() && wal_bytes_ > limit;
  }
  // The whole ledger as the snapshot of the next generation, then an empty journal of that generation.  A failure
  // before the snapshot's rename changes nothing; one after it leaves the store refusing appends, since the journal it
  // holds is stale by then.
  void compact(const quota::Window& window, const SlotPairs& pairs_of) {
    require_open();
    write_snapshot(generation_ + 1, window, pairs_of);
    generation_++;
    try {
      replace_journal();
    } catch (const StoreError& e) {
      broken_ = e.what();
      throw;
    }
    compactions_++;
  }
  void set_restored(uint64_t pairs) { restored_ = pairs; }
  void info(uint64_t out[8]) const {
    out[INFO_GENERATION] = generation_;
    out[INFO_JOURNAL_BYTES] = wal_bytes_;
    out[INFO_RECORDS] = records_;
    out[INFO_SYNCS] = syncs_;
    out[INFO_COMPACTIONS] = compactions_;
    out[INFO_REPLAYED] = replayed_;
    out[INFO_TORN] = torn_;
    out[INFO_RESTORED] = restored_;
  }
  const std::string& dir() const { return dir_; }
  std::string snap_path() const { return dir_ + "/" + SNAP_NAME; }
  std::string wal_path() const { return dir_ + "/" + WAL_NAME; }

 private:
  std::string dir_, broken_;
  int fd_ = -1;   // the journal: open, locked, written with pwrite at wal_bytes_
  uint64_t depth_ = 0, max_epochs_ = 0, journal_max_bytes_ = 0, generation_ = 0, wal_bytes_ = 0, records_ = 0, syncs_ = 0,
           compactions_ = 0, replayed_ = 0, torn_ = 0, restored_ = 0, snap_bytes_ = 0;

  static StoreError io_error(const std::string& what, const std::string& file) {
    return StoreError("quota ledger: cannot " + what + " " + file + ": " + strerror(errno));
  }
  void drop_fd() {
    if (fd_ >= 0) ::close(fd_);
    fd_ = -1;
  }
  void require_open() const {
    if (fd_ < 0) throw StoreError("quota ledger: store " + dir_ + " is not open");
    if (!broken_.empty()) throw StoreError("quota ledger: store " + dir_ + " takes no more writes after: " + broken_);
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
  // the record's length is in place; its CRC is set here.  Written, synced, or taken back.
  void append(std::vector<uint8_t>& rec) {
    struct Wipe {
      std::vector<uint8_t>& v;
      ~Wipe() { wipe(v); }
    } wiped{rec};
    put_u64(rec.data(), rec.size() - REC_FRAME);
    put_u32(rec.data() + rec.size() - 4, crc32c(rec.data(), rec.size() - 4));
    require_open();
    const bool written = write_all(fd_, rec.data(), rec.size(), (off_t)wal_bytes_);
    if (!written || fdatasync(fd_) != 0) {   // the record is not durable: take it back, the call fails
      const int e = errno;
      if (ftruncate(fd_, (off_t)wal_bytes_) != 0) broken_ = std::string(written ? "a failed sync of " : "a short write to ") + wal_path();
      errno = e;
      throw io_error(written ? "sync" : "append to", wal_path());
    }
    wal_bytes_ += rec.size();
    records_++;
    syncs_++;
  }

  // written to <file>.tmp, synced, renamed into place, directory synced
  void write_snapshot(uint64_t generation, const quota::Window& window, const SlotPairs& pairs_of) {
    const std::string file = snap_path(), tmp = file + ".tmp";
    int f = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0600);
    if (f < 0) throw io_error("write", tmp);
    std::vector<uint8_t> buf(SNAP_HEADER + 40 * (size_t)window.k);
    memcpy(buf.data(), "RLNAMDQ1", 8);
    put_u64(buf.data() + 8, depth_);
    put_u64(buf.data() + 16, max_epochs_);
    put_u64(buf.data() + 24, generation);
    put_u64(buf.data() + 32, window.k);
    for (uint32_t j = 0; j < window.k; j++) {
      put_u64(buf.data() + SNAP_HEADER + 40 * j, window.order[j]);
      memcpy(buf.data() + SNAP_HEADER + 40 * j + 8, window.e[window.order[j]].w, 32);
    }
    uint32_t crc = 0;
    off_t at = 0;
    int e = 0;   // the first failure's errno
    auto put = [&]() {
      crc = crc32c(buf.data(), buf.size(), crc);
      if (!e && !write_all(f, buf.data(), buf.size(), at)) e = errno ? errno : EIO;
      at += (off_t)buf.size();
      wipe(buf);
    };
    put();
    std::vector<uint32_t> words;
    try {
      for (uint32_t j = 0; j < window.k && !e; j++) {
        words.clear();
        pairs_of(window.order[j], words);
        buf.resize(8 + 4 * words.size());
        put_u64(buf.data(), words.size() / 2);
        for (size_t i = 0; i < words.size(); i++) put_u32(buf.data() + 8 + 4 * i, words[i]);
        std::fill(words.begin(), words.end(), 0u);
        put();
      }
    } catch (...) {
      ::close(f);
      unlink(tmp.c_str());
      throw;
    }
    buf.resize(4);
    put_u32(buf.data(), crc);
    if (!e && !write_all(f, buf.data(), 4, at)) e = errno ? errno : EIO;
    at += 4;
    if (!e && (fchmod(f, 0600) != 0 || fsync(f) != 0)) e = errno ? errno : EIO;
    if (::close(f) != 0 && !e) e = errno ? errno : EIO;
    if (!e && rename(tmp.c_str(), file.c_str()) != 0) e = errno ? errno : EIO;
    if (e) {
      unlink(tmp.c_str());
      errno = e;
      throw io_error("write", file);
    }
    sync_dir();
    snap_bytes_ = (uint64_t)at;
  }
  // an empty journal of generation_ beside the current one, locked before it takes the name; then the old one goes
  void replace_journal() {
    const std::string file = wal_path(), tmp = file + ".tmp";
    int f = ::open(tmp.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0600);
    if (f < 0) throw io_error("write", tmp);
    uint8_t h[WAL_HEADER];
    memcpy(h, "RLNAMDQW", 8);
    put_u64(h + 8, depth_);
    put_u64(h + 16, max_epochs_);
    put_u64(h + 24, generation_);
    put_u32(h + 32, crc32c(h, 32));
    if (flock(f, LOCK_EX | LOCK_NB) != 0 || fchmod(f, 0600) != 0 || !write_all(f, h, sizeof h, 0) || fsync(f) != 0 ||
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
    sync_dir();
  }

  static bool slurp(int f, std::vector<uint8_t>& b) {
    struct stat st;
    if (fstat(f, &st) != 0) return false;
    b.resize((size_t)st.st_size);
    return b.empty() || read_all(f, b.data(), b.size(), 0);
  }
  StoreError other_shape(uint64_t depth, uint64_t max_epochs) const {
    return StoreError("quota ledger: store " + dir_ + " holds a ledger of depth " + std::to_string(depth) + " and max_epochs " +
                      std::to_string(max_epochs) + ", not of depth " + std::to_string(depth_) + " and max_epochs " +
                      std::to_string(max_epochs_));
  }

  void open_locked(const std::string& dir, uint64_t depth, uint64_t max_epochs, uint64_t journal_max_bytes, Image& im) {
    dir_ = dir;
    depth_ = depth;
    max_epochs_ = max_epochs;
    journal_max_bytes_ = journal_max_bytes;
    broken_.clear();
    generation_ = wal_bytes_ = records_ = syncs_ = compactions_ = replayed_ = torn_ = restored_ = snap_bytes_ = 0;
    im = Image();
    const std::string shape = quota::new_refusal(depth, max_epochs);
    if (!shape.empty()) throw StoreError(shape);
    // A store is created in a directory that is absent or empty, and only there: a directory that holds other files
    // and neither of ours is refused before anything is put into it.
    const std::string wal = wal_path(), snap = snap_path();
    bool made_dir = false, made_wal = false;
    if (mkdir(dir.c_str(), 0700) == 0) made_dir = true;
    else if (errno != EEXIST) throw io_error("create", dir);
    if (!made_dir && access(wal.c_str(), F_OK) != 0 && access(snap.c_str(), F_OK) != 0) {
      DIR* d = opendir(dir.c_str());
      if (!d) throw io_error("read", dir);
      bool empty = true;
      while (struct dirent* e = readdir(d))
        if (strcmp(e->d_name, ".") && strcmp(e->d_name, "..")) empty = false;
      closedir(d);
      if (!empty) throw StoreError("quota ledger: " + dir + " is not empty and holds no ledger store (neither " + SNAP_NAME + " nor " + WAL_NAME + ")");
    }
    // A refused open leaves the directory as it was found: a journal file that this call created goes again.
    struct Undo {
      const std::string& wal;
      bool& made_wal;
      bool keep = false;
      ~Undo() {
        if (made_wal && !keep) unlink(wal.c_str());
      }
    } undo{wal, made_wal};
    // the lock first: nothing of a store in use is touched.  The name may pass to another file while we wait for it
    // (a compaction's rename), so the locked descriptor must still be the file the name leads to.
    for (int tries = 0;; tries++) {
      fd_ = ::open(wal.c_str(), O_RDWR);
      if (fd_ < 0 && errno == ENOENT) {
        fd_ = ::open(wal.c_str(), O_RDWR | O_CREAT | O_EXCL, 0600);
        if (fd_ >= 0) made_wal = true;
        else if (errno == EEXIST) continue;   // another opener made it meanwhile: it is theirs to lock
      }
      if (fd_ < 0) throw io_error("open", wal);
      if (flock(fd_, LOCK_EX | LOCK_NB) != 0) {
        if (errno == EWOULDBLOCK) throw StoreError("quota ledger: store " + dir + " is in use by another ledger");
        throw io_error("lock", wal);
      }
      struct stat a, b;
      if (fstat(fd_, &a) == 0 && stat(wal.c_str(), &b) == 0 && a.st_ino == b.st_ino && a.st_dev == b.st_dev) break;
      drop_fd();
      if (tries == 8) throw StoreError("quota ledger: store " + dir + " is in use by another ledger");
    }

    // Everything is read and judged before anything is written: a refusal leaves the files as they were found.
    std::vector<uint8_t> bytes;
    struct Wiped {
      std::vector<uint8_t>& v;
      ~Wiped() { wipe(v); }
    } wiped{bytes};
    int f = ::open(snap.c_str(), O_RDONLY);
    const bool found = f >= 0;
    if (!found && errno != ENOENT) throw io_error("read", snap);
    if (found) {
      const bool read = slurp(f, bytes);
      ::close(f);
      if (!read) throw io_error("read", snap);
      parse_snapshot(bytes.data(), bytes.size(), snap, im);
      if (im.depth != depth || im.max_epochs != max_epochs) throw other_shape(im.depth, im.max_epochs);
      snap_bytes_ = bytes.size();
      wipe(bytes);
    } else {
      im.depth = (uint32_t)depth;
      im.max_epochs = (uint32_t)max_epochs;
    }
    generation_ = im.generation;
    if (!slurp(fd_, bytes)) throw io_error("read", wal);
    const uint64_t size = bytes.size();
    uint64_t end = size;
    bool ours = false;   // a journal of this snapshot: replayed.  A whole journal of another generation is replaced, and
                         // so is an empty file beside the first snapshot: a first open that got no further.  The header
                         // is synced before the journal takes its name, so nothing else leaves an empty or a short one.
    if (!size && found && generation_ != 1)
      throw StoreError("quota ledger: " + wal + " is corrupt (it is empty, at offset 0, beside a snapshot of generation " +
                       std::to_string(generation_) + ")");
    if (size) {
      const uint8_t* h = bytes.data();
      if (size < WAL_HEADER || memcmp(h, "RLNAMDQW", 8) || crc32c(h, 32) != get_u32(h + 32))
        throw StoreError("quota ledger: " + wal + " is corrupt (its header, at offset 0, is not a journal header of this library)");
      if (get_u64(h + 8) != depth || get_u64(h + 16) != max_epochs) throw other_shape(get_u64(h + 8), get_u64(h + 16));
      if (!found) throw StoreError("quota ledger: " + wal + " has no snapshot beside it (" + SNAP_NAME + " is missing)");
      ours = get_u64(h + 24) == generation_;
      if (ours) replay(h, size, im, wal, &end, &replayed_);
    }

    undo.keep = true;
    unlink((snap + ".tmp").c_str());
    unlink((wal + ".tmp").c_str());
    if (!found) {
      generation_ = im.generation = 1;
      write_snapshot(1, quota::Window(), [](uint32_t, std::vector<uint32_t>&) {});
    }
    if (!ours) {
      replace_journal();
      return;
    }
    if (end < size) {
      if (ftruncate(fd_, (off_t)end) != 0 || fdatasync(fd_) != 0) throw io_error("truncate", wal);
      torn_ = size - end;
    }
    wal_bytes_ = end;
  }
};

}  // namespace qstore
}  // namespace rlnamd
