// Stand-alone program over zerokit_amd/csrc/relay.h for the sanitizer build of tests/test_relay_host.py
// (-fsanitize=address,undefined).  It reads one case file, written by the test from tests/relay_cases.py:
//   8 x uint64   max_out, n_values, n, n_roots, log capacity, seed, 0, 0
//   the inputs   values 32 n_values n | ok n | xs 32 n | roots 32 n_roots | tags 8 n
//   the model's  verdicts n | statuses n | secrets 32 n | first tags 8 n
// and runs the messages through relay.cpp's step on a fresh log in one call and in calls of 1, 63 and 1 000, then asks
// for more room than the log has.  Prints "ok <messages judged>" and exits 0, or names the first message that is wrong.
#include <stdio.h>

#include "relay.cpp"

int main(int argc, char** argv) {
  if (argc < 2) {
    printf("usage: relay_main <case file>\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    printf("cannot open %s\n", argv[1]);
    return 2;
  }
  std::vector<uint8_t> raw;
  uint8_t buf[65536];
  for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) raw.insert(raw.end(), buf, buf + got);
  fclose(f);
  uint64_t h[8];
  if (raw.size() < sizeof h) {
    printf("short case file\n");
    return 2;
  }
  memcpy(h, raw.data(), sizeof h);
  const uint64_t k = h[0], nv = h[1], n = h[2], n_roots = h[3], capacity = h[4], seed = h[5];
  if (raw.size() != sizeof h + 32 * nv * n + n + 32 * n + 32 * n_roots + 8 * n + n + n + 32 * n + 8 * n) {
    printf("the case file has the wrong size\n");
    return 2;
  }
  const uint8_t* values = raw.data() + sizeof h;
  const uint8_t* ok = values + 32 * nv * n;
  const uint8_t* xs = ok + n;
  const uint8_t* roots = xs + 32 * n;
  std::vector<uint64_t> tags(n), want_first(n);
  memcpy(tags.data(), roots + 32 * n_roots, 8 * n);
  const uint8_t* want_verdict = roots + 32 * n_roots + 8 * n;
  const uint8_t* want_status = want_verdict + n;
  const uint8_t* want_secrets = want_status + n;
  memcpy(want_first.data(), want_secrets + 32 * n, 8 * n);

  size_t judged = 0;
  const size_t chunks[] = {(size_t)n, 1, 63, 1000};
  for (size_t chunk : chunks) {
    void* log = nl_new(capacity, seed);
    std::vector<uint8_t> verdict(n), status(n), secrets(32 * n);
    std::vector<uint64_t> first(n);
    for (size_t o = 0; o < n; o += chunk) {
      const size_t c = std::min(chunk, (size_t)n - o);
      if (rl_step(log, k, nv, c, values + 32 * nv * o, ok + o, xs + 32 * o, roots, n_roots, &tags[o], &verdict[o], &status[o],
                  &secrets[32 * o], &first[o]) != 0) {
        printf("the step refused the call at message %zu\n", o);
        return 1;
      }
    }
    for (size_t i = 0; i < n; i++, judged++)
      if (verdict[i] != want_verdict[i] || status[i] != want_status[i] || memcmp(&secrets[32 * i], want_secrets + 32 * i, 32) != 0 ||
          first[i] != want_first[i]) {
        printf("wrong answer: message %zu, calls of %zu: verdict %d status %d, expected %d %d\n", i, chunk, verdict[i], status[i],
               want_verdict[i], want_status[i]);
        return 1;
      }
    if (nl_check_table(log) < 0) {
      printf("the table is not a valid open-addressing table (calls of %zu)\n", chunk);
      return 1;
    }
    uint64_t info[4];
    nl_info(log, info);
    const size_t too_many = (size_t)((info[0] - info[1]) / k) + 1;
    if (too_many <= n && rl_step(log, k, nv, too_many, values, ok, xs, roots, n_roots, nullptr, verdict.data(), status.data(),
                                 nullptr, nullptr) != 1) {
      printf("a call whose worst case does not fit was not refused\n");
      return 1;
    }
    nl_free(log);
  }
  printf("ok %zu\n", judged);
  return 0;
}
