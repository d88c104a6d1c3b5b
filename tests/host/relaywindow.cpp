// CPU build of the relay step's epoch window (zerokit_amd/csrc/relay.h: relay::gate with a window; nullifier_log.h: the
// keep predicate with the sense of the set, and through it the sequential retain) for tests/test_relay_window_host.py.
// Built with g++: the headers make no HIP call.  The log is the RetireLog of nullifierretire.cpp, which stores the
// sequence numbers of its rows, so that a step may follow a retain.  One step runs the passes in the device's order on
// one thread, as tests/host/relay.cpp does, with the window handed to the gate.
// tests/host/relaywindow_main.cpp includes this file for the sanitizer program.
#include "nullifierretire.cpp"
#include "relay.h"

namespace {

namespace rl = rlnamd::relay;

// 0: done; 1: the worst case does not fit; 2: not a layout; 3: too many roots or too large a window
int window_step(RetireLog& log, uint64_t max_out, size_t n_values, size_t n, const uint8_t* values, const uint8_t* ok,
                const uint8_t* xs, const uint8_t* roots, size_t n_roots, const uint8_t* window, size_t n_window,
                const uint64_t* tags, uint8_t* verdict, uint8_t* status, uint8_t* secrets, uint64_t* first_tag) {
  rl::Layout L;
  if (!rl::layout_for(n_values, max_out, &L)) return 2;
  if (n == 0) return 0;
  if (n_roots > rl::ROOTS_MAX || n_window > rl::EPOCHS_MAX) return 3;
  if (n > (log.capacity - log.count) / L.k) return 1;
  std::vector<uint32_t> vals(8 * n_values * n);
  memcpy(vals.data(), values, 32 * n_values * n);
  std::vector<Row32> x(n), root(n_roots ? n_roots : 1), win(n_window ? n_window : 1);
  memcpy(x.data(), xs, 32 * n);
  if (n_roots) memcpy(root.data(), roots, 32 * n_roots);
  if (n_window) memcpy(win.data(), window, 32 * n_window);
  // gate, scan
  std::vector<uint8_t> counts(n);
  std::vector<uint32_t> pos(n);
  uint32_t m = 0;
  for (size_t i = 0; i < n; i++) {
    const rl::Gate g = rl::gate(L, &vals[8 * n_values * i], ok[i], x[i], root.data(), (uint32_t)n_roots, win.data(), (uint32_t)n_window);
    verdict[i] = g.verdict;
    counts[i] = g.count;
    pos[i] = m;
    m += g.count;
  }
  // emit
  const Records R{log.nul.data(), log.rest.data(), log.tags.data(), log.seqs.data()};
  for (size_t i = 0; i < n; i++)
    if (counts[i])
      rl::emit(L, &vals[8 * n_values * i], counts[i], log.count + pos[i], log.next_seq + pos[i], tags != nullptr, tags ? tags[i] : 0, R,
               log.capacity);
  // insert, judge
  std::vector<uint8_t> sh_status(m ? m : 1);
  std::vector<Row32> sh_secret(m ? m : 1);
  std::vector<uint64_t> sh_first(m ? m : 1);
  uint32_t walk = 0;
  log.passes<SeqAtomics>((uint32_t)log.count, m, 0, 1, false, nullptr, nullptr, nullptr, &walk);
  log.passes<SeqAtomics>((uint32_t)log.count, m, 0, 1, true, sh_status.data(), (uint8_t*)sh_secret.data(), sh_first.data(), &walk);
  log.longest = std::max<uint64_t>(log.longest, walk);
  for (uint32_t j = 0; j < m; j++) log.distinct += sh_status[j] == NEW;
  log.count += m;
  log.next_seq += m;
  // fold
  for (size_t i = 0; i < n; i++) {
    const rl::Picked p = rl::fold(counts[i], &sh_status[pos[i]], &sh_secret[pos[i]], &sh_first[pos[i]]);
    status[i] = p.status;
    if (secrets) memcpy(secrets + 32 * i, p.secret.w, 32);
    if (first_tag) first_tag[i] = p.first_tag;
  }
  return 0;
}

// the sequential retain: RetireLog::retire_set with the sense of the set turned round.  0: done; 1: refused
// (rw_retain_refusal gives the text)
int retain_set(RetireLog& log, size_t k, const uint8_t* ext, uint64_t* removed) {
  *removed = 0;
  if (!rlnamd::nlog::retain_refusal(ext, k).empty()) return 1;
  RetireSet E;
  E.k = (uint32_t)k;
  E.retain = 1;
  for (size_t j = 0; j < k; j++) memcpy(E.e[j].w, ext + 32 * j, 32);
  const Records R{log.nul.data(), log.rest.data(), log.tags.data(), log.seqs.data()};
  uint32_t walk = 0;
  const uint64_t kept = retire<SeqAtomics>(R, log.table.data(), log.slots, log.seed, log.count, E, &log.distinct, &walk);
  if (kept != log.count) log.rebuild_longest = walk;
  *removed = log.count - kept;
  log.count = kept;
  return 0;
}

thread_local std::string g_text;

}  // namespace

extern "C" {

int rw_step(void* log, uint64_t max_out, size_t n_values, size_t n, const uint8_t* values, const uint8_t* ok, const uint8_t* xs,
            const uint8_t* roots, size_t n_roots, const uint8_t* window, size_t n_window, const uint64_t* tags, uint8_t* verdict,
            uint8_t* status, uint8_t* secrets, uint64_t* first_tag) {
  return window_step(*(RetireLog*)log, max_out, n_values, n, values, ok, xs, roots, n_roots, window, n_window, tags, verdict,
                     status, secrets, first_tag);
}
int rw_retain(void* log, size_t k, const uint8_t* ext, uint64_t* removed) { return retain_set(*(RetireLog*)log, k, ext, removed); }
// row `row` of the log: the share, its tag and its sequence number
void rw_row(void* l, uint64_t row, uint8_t share[128], uint64_t* tag, uint64_t* seq) {
  RetireLog* h = (RetireLog*)l;
  memcpy(share, h->nul[row].w, 32);
  memcpy(share + 32, &h->rest[row], 96);
  *tag = h->tags[row];
  *seq = h->seqs[row];
}
// the table, slot for slot
void rw_table(void* l, uint32_t* out) {
  RetireLog* h = (RetireLog*)l;
  memcpy(out, h->table.data(), 4 * h->slots);
}
const char* rw_retain_refusal(const uint8_t* ext, size_t k) {
  g_text = rlnamd::nlog::retain_refusal(ext, k);
  return g_text.c_str();
}
const char* rw_epochs_refusal(const uint8_t* ext, size_t k) {
  g_text = rl::epochs_refusal(ext, k);
  return g_text.c_str();
}

}  // extern "C"
