// CPU build of the nullifier log's retire (zerokit_amd/csrc/nullifier_log.h: the keep predicate, the sequential retire
// and the sequence-number lookup), for tests/test_nullifier_retire_host.py.  Built with g++: the header makes no HIP
// call.  The log is the HostLog of nullifierlog.cpp with what a retire adds to it: the sequence numbers of the rows
// and the counter behind the default tags.  tests/host/nullifierretire_main.cpp includes this file for the sanitizer
// program.
#include "nullifierlog.cpp"

namespace {

struct RetireLog : HostLog {
  std::vector<uint64_t> seqs;
  uint64_t next_seq = 0, distinct = 0, rebuild_longest = 0;
  RetireLog(uint64_t capacity_, uint64_t seed_) : HostLog(capacity_, seed_), seqs(capacity_) {}

  // HostLog::observe on one thread, with the default tags and the sequence numbers of a log that may have retired
  int observe_seq(size_t n, const uint8_t* shares, const uint64_t* tg, uint8_t* status, uint8_t* secrets, uint64_t* first_tag) {
    std::vector<uint64_t> own(n);
    for (size_t i = 0; i < n; i++) own[i] = tg ? tg[i] : next_seq + i;
    const uint64_t first_row = count;
    const int rc = observe(n, shares, own.data(), status, secrets, first_tag, 0);
    if (rc != 0) return rc;
    for (size_t i = 0; i < n; i++) {
      seqs[first_row + i] = next_seq + i;
      distinct += status[i] == NEW;
    }
    next_seq += n;
    return 0;
  }

  // 0: done; 1: a null pointer with k > 0; 2: k > RETIRE_MAX; 3: an external nullifier >= r (*removed: which)
  int retire_set(size_t k, const uint8_t* ext, uint64_t* removed) {
    *removed = 0;
    if (k > 0 && !ext) return 1;
    if (k > RETIRE_MAX) return 2;
    for (size_t j = 0; j < k; j++)
      if (!element_is_canonical(ext + 32 * j)) {
        *removed = j;
        return 3;
      }
    RetireSet E;
    E.k = (uint32_t)k;
    for (size_t j = 0; j < k; j++) memcpy(E.e[j].w, ext + 32 * j, 32);
    const Records R{nul.data(), rest.data(), tags.data(), seqs.data()};
    uint32_t walk = 0;
    const uint64_t kept = retire<SeqAtomics>(R, table.data(), slots, seed, count, E, &distinct, &walk);
    if (kept != count) rebuild_longest = walk;
    *removed = count - kept;
    count = kept;
    return 0;
  }

  // 0: done; 1: never issued; 2: retired
  int get(uint64_t seq, uint8_t share[128], uint64_t* tag) const {
    if (seq >= next_seq) return 1;
    const uint64_t row = find_seq(seqs.data(), count, seq);
    if (row == count) return 2;
    memcpy(share, nul[row].w, 32);
    memcpy(share + 32, &rest[row], 96);
    *tag = tags[row];
    return 0;
  }
};

}  // namespace

extern "C" {

void* nr_new(uint64_t capacity, uint64_t seed) { return new RetireLog(capacity, seed); }
void nr_free(void* l) { delete (RetireLog*)l; }
int nr_observe(void* l, size_t n, const uint8_t* shares, const uint64_t* tags, uint8_t* status, uint8_t* secrets,
               uint64_t* first_tag) {
  return ((RetireLog*)l)->observe_seq(n, shares, tags, status, secrets, first_tag);
}
int nr_retire(void* l, size_t k, const uint8_t* ext, uint64_t* removed) { return ((RetireLog*)l)->retire_set(k, ext, removed); }
int nr_get(void* l, uint64_t seq, uint8_t share[128], uint64_t* tag) { return ((RetireLog*)l)->get(seq, share, tag); }
// [0] capacity, [1] records held, [2] slots, [3] distinct nullifiers, [4] next sequence number, [5] longest walk of the
// last rebuild
void nr_info(void* l, uint64_t out[6]) {
  RetireLog* h = (RetireLog*)l;
  out[0] = h->capacity;
  out[1] = h->count;
  out[2] = h->slots;
  out[3] = h->distinct;
  out[4] = h->next_seq;
  out[5] = h->rebuild_longest;
}
// nl_check_table over the log: taken entries, or -1 if a key cannot be reached from its home slot
int64_t nr_check_table(void* l) { return nl_check_table((HostLog*)(RetireLog*)l); }
// sequence numbers ascending over the rows held?
int nr_seqs_ascend(void* l) {
  RetireLog* h = (RetireLog*)l;
  for (uint64_t i = 1; i < h->count; i++)
    if (h->seqs[i - 1] >= h->seqs[i]) return 0;
  return 1;
}

}  // extern "C"
