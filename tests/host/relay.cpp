// CPU build of the relay step's per-item logic (zerokit_amd/csrc/relay.h: what k_relay_gate, k_relay_emit and
// k_relay_fold inline) for tests/test_relay_host.py.  Built with g++: the header makes no HIP call.  One step runs the
// passes in the device's order on one thread -- gate over every message, an exclusive sum of the share counts, emit
// over every message, the sequential insert and judge of nullifier_log.h over the new rows, fold over every message --
// on the HostLog of nullifierlog.cpp.  tests/host/relay_main.cpp includes this file for the sanitizer program.
#include "nullifierlog.cpp"
#include "relay.h"

namespace {

namespace rl = rlnamd::relay;

// 0: done; 1: the worst case does not fit; 2: not a layout; 3: an argument check refused (rl_check gives the text)
int relay_step(HostLog& log, uint64_t max_out, size_t n_values, size_t n, const uint8_t* values, const uint8_t* ok,
               const uint8_t* xs, const uint8_t* roots, size_t n_roots, const uint64_t* tags, uint8_t* verdict, uint8_t* status,
               uint8_t* secrets, uint64_t* first_tag) {
  rl::Layout L;
  if (!rl::layout_for(n_values, max_out, &L)) return 2;
  if (n == 0) return 0;
  if (n_roots > rl::ROOTS_MAX) return 3;
  if (n > (log.capacity - log.count) / L.k) return 1;
  std::vector<uint32_t> vals(8 * n_values * n);
  memcpy(vals.data(), values, 32 * n_values * n);
  std::vector<Row32> x(n), root(n_roots ? n_roots : 1);
  memcpy(x.data(), xs, 32 * n);
  if (n_roots) memcpy(root.data(), roots, 32 * n_roots);
  // gate
  std::vector<uint8_t> counts(n);
  for (size_t i = 0; i < n; i++) {
    const rl::Gate g = rl::gate(L, &vals[8 * n_values * i], ok[i], x[i], root.data(), (uint32_t)n_roots);
    verdict[i] = g.verdict;
    counts[i] = g.count;
  }
  // scan
  std::vector<uint32_t> pos(n);
  uint32_t m = 0;
  for (size_t i = 0; i < n; i++) {
    pos[i] = m;
    m += counts[i];
  }
  // emit (the host log is dense: row == sequence number, no seqs[])
  const Records R{log.nul.data(), log.rest.data(), log.tags.data(), nullptr};
  for (size_t i = 0; i < n; i++)
    if (counts[i])
      rl::emit(L, &vals[8 * n_values * i], counts[i], log.count + pos[i], log.count + pos[i], tags != nullptr, tags ? tags[i] : 0, R,
               log.capacity);
  // insert, judge
  std::vector<uint8_t> sh_status(m ? m : 1);
  std::vector<Row32> sh_secret(m ? m : 1);
  std::vector<uint64_t> sh_first(m ? m : 1);
  uint32_t walk = 0;
  log.passes<SeqAtomics>((uint32_t)log.count, m, 0, 1, false, nullptr, nullptr, nullptr, &walk);
  log.passes<SeqAtomics>((uint32_t)log.count, m, 0, 1, true, sh_status.data(), (uint8_t*)sh_secret.data(), sh_first.data(), &walk);
  log.longest = std::max<uint64_t>(log.longest, walk);
  log.count += m;
  // fold
  for (size_t i = 0; i < n; i++) {
    const rl::Picked p = rl::fold(counts[i], &sh_status[pos[i]], &sh_secret[pos[i]], &sh_first[pos[i]]);
    status[i] = p.status;
    if (secrets) memcpy(secrets + 32 * i, p.secret.w, 32);
    if (first_tag) first_tag[i] = p.first_tag;
  }
  return 0;
}

}  // namespace

extern "C" {

int rl_step(void* log, uint64_t max_out, size_t n_values, size_t n, const uint8_t* values, const uint8_t* ok, const uint8_t* xs,
            const uint8_t* roots, size_t n_roots, const uint64_t* tags, uint8_t* verdict, uint8_t* status, uint8_t* secrets,
            uint64_t* first_tag) {
  return relay_step(*(HostLog*)log, max_out, n_values, n, values, ok, xs, roots, n_roots, tags, verdict, status, secrets,
                    first_tag);
}
// record `row` of the log as a share, nullifier | x | y | external_nullifier, and its tag
void rl_get(void* l, uint64_t row, uint8_t share[128], uint64_t* tag) {
  HostLog* h = (HostLog*)l;
  memcpy(share, h->nul[row].w, 32);
  memcpy(share + 32, &h->rest[row], 96);
  *tag = h->tags[row];
}
const char* rl_check(size_t n, const void* proofs, const void* values, const void* signals, const uint64_t* offsets, const void* xs,
                     const void* roots, size_t n_roots, const void* verdict, const void* status) {
  const char* t = rl::check_arguments(n, proofs, values, signals, offsets, xs, roots, n_roots, verdict, status);
  return t ? t : "";
}

}  // extern "C"
