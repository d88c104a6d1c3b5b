// The relay step on the device: the kernels over relay.h and the RelayDev object.
//
// One step() call: the host checks (a refused call enqueues nothing), then per verifier chunk (65 536 messages with a
// lane per proof, 8 192 in team form, the shape chosen as GpuVerifier::verify chooses it)
//   verifier's stream   its copy in and its three kernels; proofs, values and verdicts stay on the device
//   hasher's stream     at the same time: the chunk's signals packed and hashed, the rows left in message order
//                       (k_hash_to_field_at; the host's share of the plan is hashed on the calling thread and copied
//                       into place); with xs_le the rows come with the step's one small copy in instead
//   log's stream        the copy in of roots, window and tags, then behind an event from each of the other two:
//     k_relay_gate                verdict[i] and the message's share count (the roots and the epoch window in LDS)
//     k_scan_up / k_scan_down     pos[i] = shares of the messages below i (log_scan.h)
//     k_relay_emit                the shares into rows [count + pos[i], ...) of the log's record arrays
//     k_relay_insert, k_relay_judge   nlog::insert and nlog::judge over the m new rows; m is known on the device only, so
//                                 the grids cover the worst case and a lane at or beyond m leaves at once
//     k_relay_fold                per message: status, secret and first tag by relay::fold
//     one copy back of [m, longest walk, NEW shares | secrets | first tags | verdicts | statuses], a memset of the
//     block behind it, ONE stream wait
// and on the host the log's counters move as observe() moves them.  Every kernel is one lane per item and the passes are
// ordered by kernel boundaries only: no lane waits for, or reads, what another lane of the same kernel writes.  The
// words lanes share are the table entries (agent-scope atomics, as in nullifier_log.hip) and three counters, each
// written with one atomic a workgroup.
//
// A relay made with RelayDev::OPTIMISTIC runs the verifier's combined check instead of its three kernels for the chunks
// the flags name (relay.h): the chunk is enqueued (GpuVerifier::relay_enqueue_combined), the hasher's and the log's
// stream get their work, THEN the verifier's stream is waited for and the host finishes the pairing check
// (relay_settle); a rejected chunk's exact kernels run behind that, over the inputs already resident.  Such a chunk has
// two stream waits.  An accepted chunk leaves reject flags where the exact pass leaves verdicts, and k_relay_gate is
// told which it reads.
//
// The chunks of a call run one after the other: the wait at the end of a chunk is also what lets the verifier's and the
// hasher's staging be packed again.  Within a chunk hashing runs beside the pairing kernels.
//
// Secrets.  The result block and the per-share scratch behind it hold recovered identity secrets: both are one device
// allocation that is zeroed behind the copy back, the pinned copy is wiped before step() returns, and a scope guard
// does both on every error path (observe()'s rule).  Proofs, values, signals, roots and tags are public.
#include "relay.h"

#include <string.h>

#include <string>
#include <vector>

#include "common.h"
#include "keccak_batch.h"
#include "log_scan.h"
#include "verify.h"

namespace rlnamd {

using nlog::DevAtomics;
using nlog::Records;
using nlog::Row32;
using nlog::View;
using relay::Layout;

namespace {

// hdr: 4 words at the head of the result block: [0] m, [1] the longest walk, [2] NEW shares, [3] unused

__global__ void __launch_bounds__(LOG_LANES) k_relay_gate(Layout L, const uint32_t* __restrict__ vals,
                                                          const uint8_t* __restrict__ ok, const Row32* __restrict__ xs,
                                                          const Row32* __restrict__ roots, uint32_t n_roots,
                                                          const Row32* __restrict__ window, uint32_t n_window, uint32_t n,
                                                          uint32_t ok_is_rejected, uint8_t* __restrict__ verdict,
                                                          ShareCount* __restrict__ counts) {
  __shared__ Row32 lds_roots[relay::ROOTS_MAX];
  __shared__ Row32 lds_window[relay::EPOCHS_MAX];
  for (uint32_t j = threadIdx.x; j < n_roots * 8; j += LOG_LANES) lds_roots[j >> 3].w[j & 7] = roots[j >> 3].w[j & 7];
  for (uint32_t j = threadIdx.x; j < n_window * 8; j += LOG_LANES) lds_window[j >> 3].w[j & 7] = window[j >> 3].w[j & 7];
  __syncthreads();
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i >= n) return;
  // behind an accepted combined check ok[] holds the reject flags, and every proof without one is valid
  const uint8_t valid = ok_is_rejected ? (ok[i] ? 0 : 1) : ok[i];
  const relay::Gate g = relay::gate(L, vals + (size_t)8 * L.n_values * i, valid, xs[i], lds_roots, n_roots, lds_window, n_window);
  verdict[i] = g.verdict;
  counts[i].v = g.count;
}

// tags: n, or null
__global__ void __launch_bounds__(LOG_LANES) k_relay_emit(Layout L, const uint32_t* __restrict__ vals,
                                                          const ShareCount* __restrict__ counts,
                                                          const uint32_t* __restrict__ pos, const uint32_t* __restrict__ total,
                                                          const uint64_t* __restrict__ tags, uint32_t n, Records R,
                                                          uint64_t first_row, uint64_t next_seq, uint64_t capacity,
                                                          uint32_t* __restrict__ hdr) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i == 0) hdr[0] = *total;
  if (i >= n || counts[i].v == 0) return;
  relay::emit(L, vals + (size_t)8 * L.n_values * i, counts[i].v, first_row + pos[i], next_seq + pos[i], tags != nullptr,
              tags ? tags[i] : 0, R, capacity);
}

// k_log_insert and k_log_judge of nullifier_log.hip with the number of shares read from the device: *m <= room
__global__ void __launch_bounds__(LOG_LANES) k_relay_insert(View L, uint32_t first_id, const uint32_t* __restrict__ m,
                                                            uint32_t room) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i < *m && i < room) nlog::insert<DevAtomics>(L, first_id + i);
}
__global__ void __launch_bounds__(LOG_LANES) k_relay_judge(View L, uint32_t first_id, const uint32_t* __restrict__ m,
                                                           uint32_t room, uint8_t* __restrict__ status,
                                                           Row32* __restrict__ secrets, uint64_t* __restrict__ first_tag,
                                                           uint32_t* __restrict__ hdr) {
  __shared__ uint32_t wg_walk, wg_new;
  if (threadIdx.x == 0) wg_walk = 0, wg_new = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i < *m && i < room) {
    const nlog::Verdict v = nlog::judge<DevAtomics>(L, first_id + i);
    status[i] = v.status;
    secrets[i] = v.secret;
    first_tag[i] = L.tags[v.first];
    atomicMax(&wg_walk, v.walk);
    if (v.status == nlog::NEW) atomicAdd(&wg_new, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0 && wg_walk) {
    __hip_atomic_fetch_max(&hdr[1], wg_walk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (wg_new) __hip_atomic_fetch_add(&hdr[2], wg_new, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void __launch_bounds__(LOG_LANES) k_relay_fold(const ShareCount* __restrict__ counts, const uint32_t* __restrict__ pos,
                                                          const uint8_t* __restrict__ sh_status,
                                                          const Row32* __restrict__ sh_secrets,
                                                          const uint64_t* __restrict__ sh_first, uint32_t n, uint32_t room,
                                                          uint8_t* __restrict__ status, Row32* __restrict__ secrets,
                                                          uint64_t* __restrict__ first_tag) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i >= n) return;
  uint32_t c = counts[i].v;
  const uint32_t p = pos[i];
  if (p > room || c > room - p) c = 0;   // (not reached: the counts sum to at most room)
  const relay::Picked k = relay::fold(c, sh_status + p, sh_secrets + p, sh_first + p);
  status[i] = k.status;
  secrets[i] = k.secret;
  first_tag[i] = k.first_tag;
}

// the stores go through a volatile pointer so that they cannot be elided as dead (ffi_wire.h: secure_zero)
void wipe_host(void* p, size_t n) {
  volatile uint8_t* v = (volatile uint8_t*)p;
  for (size_t i = 0; i < n; i++) v[i] = 0;
}

size_t nonzero_words16(const uint8_t* p, size_t bytes) {
  size_t c = 0;
  for (size_t o = 0; o + 16 <= bytes; o += 16) {
    uint8_t any = 0;
    for (int k = 0; k < 16; k++) any |= p[o + k];
    c += any != 0;
  }
  return c;
}

struct OnDevice {   // the relay's device for the length of a call, the caller's afterwards
  int prev = 0, dev;
  explicit OnDevice(int dev_) : dev(dev_) {
    RLN_HIP(hipGetDevice(&prev));
    if (prev != dev) RLN_HIP(hipSetDevice(dev));
  }
  ~OnDevice() {
    if (prev != dev) (void)hipSetDevice(prev);
  }
};

size_t pad16(size_t b) { return (b + 15) / 16 * 16; }

}  // namespace

struct RelayDev::Impl {
  GpuVerifier& V;
  NullifierLogDev& log;
  HasherDev* hasher;
  int lanes, flags, device = 0;
  Layout L;
  hipEvent_t ev_verified = nullptr, ev_hashed = nullptr;
  uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // the epoch window: n_window external nullifiers, 0 for none; copied in beside the roots with every chunk
  Row32 window[relay::EPOCHS_MAX];
  uint32_t n_window = 0;
  // buffers for a chunk of up to cap messages, K = L.k shares each at the most
  //   in  (pinned + device):  [roots 32 x 64][window 32 x 64][tags 8 n, padded to 16][xs 32 n]   (xs: copied with xs_le, written by the
  //                           hasher else)
  //   out (device):           [hdr 16][secrets 32 n][first tags 8 n][verdicts n][statuses n] = result(n), copied back,
  //                           then per share [secrets 32 nK][first tags 8 nK][statuses nK]
  //   out (pinned):           result(n)
  // `out` is all zero between steps, on the device and in the pinned copy.
  size_t cap = 0;
  uint8_t* in_host = nullptr;
  uint8_t* out_host = nullptr;
  DevBuf<uint8_t> in_dev, out_dev;
  DevBuf<ShareCount> counts;
  DevBuf<uint32_t> pos, sums;

  Impl(GpuVerifier& v, NullifierLogDev& l, HasherDev* h, int lanes_, int flags_)
      : V(v), log(l), hasher(h), lanes(lanes_), flags(flags_) {}

  static constexpr size_t IN_HEAD = 32 * (relay::ROOTS_MAX + relay::EPOCHS_MAX);   // roots and window
  static size_t in_bytes(size_t n) { return IN_HEAD + pad16(8 * n) + 32 * n; }
  static size_t result_bytes(size_t n) { return 16 + pad16(42 * n); }
  size_t out_bytes(size_t n) const { return result_bytes(n) + pad16(41 * n * L.k); }

  void reserve(size_t n, hipStream_t stream) {
    if (n <= cap) return;
    release();
    const size_t m = n < 1024 ? 1024 : n;
    RLN_HIP(hipHostMalloc((void**)&in_host, in_bytes(m), hipHostMallocDefault));
    RLN_HIP(hipHostMalloc((void**)&out_host, result_bytes(m), hipHostMallocDefault));
    memset(out_host, 0, result_bytes(m));
    in_dev.alloc(in_bytes(m));
    out_dev.alloc(out_bytes(m));
    counts.alloc(m);
    pos.alloc(m);
    sums.alloc(ScanPlan(m).words);
    RLN_HIP(hipMemsetAsync(out_dev.p, 0, out_bytes(m), stream));
    RLN_HIP(hipStreamSynchronize(stream));
    cap = m;
  }
  // (what held secrets is zero already -- step() wipes before it returns -- and is wiped once more before it is freed;
  // every step ends in a wait, so nothing is in flight here, and the blocking memset needs no stream of the log's: a
  // relay may be freed after its log)
  void release() {
    if (out_dev.p) (void)hipMemset(out_dev.p, 0, out_bytes(cap));
    if (out_host) {
      wipe_host(out_host, result_bytes(cap));
      (void)hipHostFree(out_host);
    }
    if (in_host) (void)hipHostFree(in_host);
    in_dev.release();
    out_dev.release();
    counts.release();
    pos.release();
    sums.release();
    in_host = out_host = nullptr;
    cap = 0;
  }
  ~Impl() {
    release();
    if (ev_verified) (void)hipEventDestroy(ev_verified);
    if (ev_hashed) (void)hipEventDestroy(ev_hashed);
  }

  void chunk(size_t n, bool team, const uint8_t* proofs, const uint8_t* values_le, const uint8_t* signals, size_t signals_len,
             const uint64_t* offsets, const uint8_t* xs_le, const uint8_t* roots_le, size_t n_roots, const uint64_t* tags,
             uint8_t* verdict, uint8_t* status, uint8_t* secrets_le, uint64_t* first_tag);
};

RelayDev::RelayDev(GpuVerifier& verifier, uint64_t max_out, NullifierLogDev& log, HasherDev* hasher, int lanes, int flags) {
  if (lanes != 0 && lanes != 1 && lanes != 8) throw Error("relay: lanes must be 0 (choose), 1 or 8");
  if (const char* refused = check_flags(flags)) throw Error(std::string("relay: ") + refused);
  Layout L;
  if (!relay::layout_for(verifier.n_values(), max_out, &L))
    throw Error("relay: a circuit of " + std::to_string(verifier.n_values()) + " public values and " + std::to_string(max_out) +
                " message slots has neither the single nor the multi-message layout");
  const int dev = verifier.device();
  if (log.device() != dev || (hasher && hasher->device() != dev))
    throw Error("relay: the prover, the log and the hasher are not on one device");
  Impl* m = new Impl(verifier, log, hasher, lanes, flags);
  try {
    m->L = L;
    m->device = dev;
    OnDevice on(dev);
    RLN_HIP(hipEventCreateWithFlags(&m->ev_verified, hipEventDisableTiming));
    RLN_HIP(hipEventCreateWithFlags(&m->ev_hashed, hipEventDisableTiming));
  } catch (...) {
    delete m;
    throw;
  }
  d = m;
}

RelayDev::~RelayDev() {
  if (!d) return;
  int prev = 0;
  const bool move = hipGetDevice(&prev) == hipSuccess && prev != d->device && hipSetDevice(d->device) == hipSuccess;
  delete d;
  if (move) (void)hipSetDevice(prev);
}

void RelayDev::step(size_t n, const uint8_t* proofs, const uint8_t* values_le, size_t n_values, const uint8_t* signals,
                    size_t signals_len, const uint64_t* offsets, const uint8_t* xs_le, const uint8_t* roots_le, size_t n_roots,
                    const uint64_t* tags, uint8_t* verdict, uint8_t* status, uint8_t* secrets_le, uint64_t* first_tag) {
  Impl& m = *d;
  if (n == 0) return;
  // the host checks: nothing is enqueued and nothing of the log, the hasher or the verifier changes before they pass
  if (const char* refused = relay::check_arguments(n, proofs, values_le, signals, offsets, xs_le, roots_le, n_roots, verdict, status))
    throw Error(refused);
  const bool hashing = xs_le == nullptr;
  if (hashing && !m.hasher) throw Error("relay step: signals were given to a relay made without a hasher");
  if (hashing)
    if (const char* refused = kbatch::check_call(signals, signals_len, offsets, n)) throw Error(refused);
  if (n_values != m.L.n_values) throw Error("MalformedVerifyingKey: relay step: n_values is not the key's input count");
  const NullifierLogDev::RelayRows at = m.log.relay_rows();
  const uint64_t room = at.capacity - at.count;
  if (n > room / m.L.k)
    throw Error("relay step: " + std::to_string(n) + " messages of up to " + std::to_string(m.L.k) + " shares do not fit: " +
                std::to_string(room) + " of " + std::to_string(at.capacity) + " records are left");

  OnDevice on(m.device);
  const bool team = m.V.relay_team(n, m.lanes);
  const size_t per = team ? GpuVerifier::TEAM_CHUNK : GpuVerifier::CHUNK;
  m.stats[0]++;
  for (size_t off = 0; off < n; off += per) {
    const size_t c = n - off < per ? n - off : per;
    m.chunk(c, team, proofs + 128 * off, values_le + 32 * n_values * off, signals, signals_len, hashing ? offsets + off : nullptr,
            hashing ? nullptr : xs_le + 32 * off, roots_le, n_roots, tags ? tags + off : nullptr, verdict + off, status + off,
            secrets_le ? secrets_le + 32 * off : nullptr, first_tag ? first_tag + off : nullptr);
  }
}

void RelayDev::Impl::chunk(size_t n, bool team, const uint8_t* proofs, const uint8_t* values_le, const uint8_t* signals,
                           size_t signals_len, const uint64_t* offsets, const uint8_t* xs_le, const uint8_t* roots_le,
                           size_t n_roots, const uint64_t* tags, uint8_t* verdict, uint8_t* status, uint8_t* secrets_le,
                           uint64_t* first_tag) {
  const NullifierLogDev::RelayRows at = log.relay_rows();
  hipStream_t ls = (hipStream_t)at.stream, vs = (hipStream_t)V.relay_stream();
  hipStream_t hs = hasher ? (hipStream_t)hasher->relay_stream() : nullptr;
  reserve(n, ls);
  const uint32_t n32 = (uint32_t)n, room = (uint32_t)(n * L.k);   // n <= 65 536, k <= 255

  uint8_t* d_roots = in_dev.p;
  uint8_t* d_window = d_roots + 32 * relay::ROOTS_MAX;
  uint8_t* d_tags = in_dev.p + IN_HEAD;
  uint8_t* d_xs = d_tags + pad16(8 * n);
  uint32_t* d_hdr = (uint32_t*)out_dev.p;
  uint8_t* d_secrets = out_dev.p + 16;
  uint8_t* d_first = d_secrets + 32 * n;
  uint8_t* d_verdict = d_first + 8 * n;
  uint8_t* d_status = d_verdict + n;
  uint8_t* d_sh_secrets = out_dev.p + result_bytes(n);
  uint8_t* d_sh_first = d_sh_secrets + 32 * (size_t)room;
  uint8_t* d_sh_status = d_sh_first + 8 * (size_t)room;

  struct Wipe {   // success or error: every stream is idle and what held secrets is zero again when the chunk is left
    Impl& m;
    size_t n;
    hipStream_t ls, vs, hs;
    bool device_done = false;
    ~Wipe() {
      if (!device_done) {
        (void)hipStreamSynchronize(vs);
        if (hs) (void)hipStreamSynchronize(hs);
        (void)hipMemsetAsync(m.out_dev.p, 0, m.out_bytes(n), ls);
        (void)hipStreamSynchronize(ls);
      }
      wipe_host(m.out_host, result_bytes(n));
    }
  } wipe{*this, n, ls, vs, hs};

  // 1. the verifier's pass: exact, or (flags, and no cool-down) the combined check, which is settled in step 3
  const bool combined = (flags & RelayDev::OPTIMISTIC) && (!team || (flags & RelayDev::OPTIMISTIC_TEAMS)) &&
                        !V.relay_cooldown_skip();
  GpuVerifier::RelayChunk vc{nullptr, nullptr, nullptr};
  if (combined) {
    V.relay_enqueue_combined(n, proofs, values_le, team);
  } else {
    vc = V.relay_enqueue(n, proofs, values_le, team);
    RLN_HIP(hipEventRecord(ev_verified, vs));
  }
  // 2. the signals beside it (offsets are the call's: the chunk's messages lie at offsets[0 .. n])
  if (offsets) {
    stats[6] += hasher->relay_hash(signals, signals_len, offsets, n, d_xs);
    RLN_HIP(hipEventRecord(ev_hashed, hs));
  }
  // 3. the log's stream
  size_t in_len = IN_HEAD + pad16(8 * n);
  if (n_roots) memcpy(in_host, roots_le, 32 * n_roots);
  if (n_window) memcpy(in_host + 32 * relay::ROOTS_MAX, window, 32 * n_window);
  if (tags) memcpy(in_host + IN_HEAD, tags, 8 * n);
  if (xs_le) {
    memcpy(in_host + in_len, xs_le, 32 * n);
    in_len += 32 * n;
  }
  RLN_HIP(hipMemcpyAsync(in_dev.p, in_host, in_len, hipMemcpyHostToDevice, ls));
  if (combined) {
    // the first of this chunk's two waits: the hashing and the copy above run under the combined kernels and the
    // host's finish.  An accepted chunk has nothing left on the verifier's stream; a rejected one its exact kernels.
    vc = V.relay_settle();
    RLN_HIP(hipEventRecord(ev_verified, vs));
  }
  RLN_HIP(hipStreamWaitEvent(ls, ev_verified, 0));
  if (offsets) RLN_HIP(hipStreamWaitEvent(ls, ev_hashed, 0));
  const dim3 per_message(div_up(n, LOG_LANES)), per_share(div_up(room, LOG_LANES)), block(LOG_LANES);
  hipLaunchKernelGGL(k_relay_gate, per_message, block, 0, ls, L, vc.vals, vc.ok, (const Row32*)d_xs, (const Row32*)d_roots,
                     (uint32_t)n_roots, (const Row32*)d_window, n_window, n32, vc.ok_is_rejected ? 1u : 0u, d_verdict, counts.p);
  const uint32_t* d_m = scan_positions((const ShareCount*)counts.p, n, pos.p, sums.p, ls);
  hipLaunchKernelGGL(k_relay_emit, per_message, block, 0, ls, L, vc.vals, (const ShareCount*)counts.p, (const uint32_t*)pos.p, d_m,
                     (const uint64_t*)(tags ? d_tags : nullptr), n32, at.rows, at.count, at.next_seq, at.capacity, d_hdr);
  const uint32_t first_id = (uint32_t)at.count;
  hipLaunchKernelGGL(k_relay_insert, per_share, block, 0, ls, at.view, first_id, d_m, room);
  hipLaunchKernelGGL(k_relay_judge, per_share, block, 0, ls, at.view, first_id, d_m, room, d_sh_status, (Row32*)d_sh_secrets,
                     (uint64_t*)d_sh_first, d_hdr);
  hipLaunchKernelGGL(k_relay_fold, per_message, block, 0, ls, (const ShareCount*)counts.p, (const uint32_t*)pos.p,
                     (const uint8_t*)d_sh_status, (const Row32*)d_sh_secrets, (const uint64_t*)d_sh_first, n32, room, d_status,
                     (Row32*)d_secrets, (uint64_t*)d_first);
  RLN_HIP(hipGetLastError());
  RLN_HIP(hipMemcpyAsync(out_host, out_dev.p, result_bytes(n), hipMemcpyDeviceToHost, ls));
  RLN_HIP(hipMemsetAsync(out_dev.p, 0, out_bytes(n), ls));   // behind the copy, in stream order
  RLN_HIP(hipStreamSynchronize(ls));   // behind both events: the verifier's and the hasher's streams have passed them
  wipe.device_done = true;

  // 4. the host's part of observe().  observe() moves count and next_seq right behind its launches, so that the ids the
  // table holds count as taken whatever happens next; here m exists on the device only until this copy back has been
  // waited for, so the commit cannot come sooner.  What that leaves open: if the copy or the wait above fails (a device
  // error), the table may hold ids at or beyond `count` that a later call would issue again.  Such a failure leaves the
  // device's context in error, and every later call on the log fails with it, so the ids are not reused in practice;
  // a log that saw a step fail with a HIP error should be cleared or dropped all the same.
  uint32_t hdr[4];
  memcpy(hdr, out_host, 16);
  if (hdr[0] > room) throw Error("relay step: internal error, the position pass counted more shares than there can be");
  if (hdr[0]) log.relay_commit(hdr[0], hdr[1], hdr[2]);
  const uint8_t* h_secrets = out_host + 16;
  const uint8_t* h_first = h_secrets + 32 * n;
  const uint8_t* h_verdict = h_first + 8 * n;
  const uint8_t* h_status = h_verdict + n;
  size_t accepted = 0, bad_epoch = 0;
  for (size_t i = 0; i < n; i++) {
    if (h_status[i] > relay::SKIPPED) throw Error("nullifier log: internal error, a share's key is not in the table");
    accepted += h_verdict[i] == relay::OK;
    bad_epoch += h_verdict[i] == relay::BAD_EPOCH;
  }
  stats[1]++;
  stats[2] += n;
  stats[3] += accepted;
  stats[4] += hdr[0];
  stats[7] += bad_epoch;
  memcpy(verdict, h_verdict, n);
  memcpy(status, h_status, n);
  if (secrets_le) memcpy(secrets_le, h_secrets, 32 * n);
  if (first_tag) memcpy(first_tag, h_first, 8 * n);
}

uint64_t RelayDev::set_epochs(size_t k, const uint8_t* external_nullifiers_le, bool retain) {
  Impl& m = *d;
  const std::string refused = relay::epochs_refusal(external_nullifiers_le, k);
  if (!refused.empty()) throw Error(refused);
  // the log first: a retain that throws leaves the log as it was, and the window with it
  const uint64_t gone = k && retain ? m.log.retain(k, external_nullifiers_le) : 0;
  if (k) memcpy(m.window, external_nullifiers_le, 32 * k);
  m.n_window = (uint32_t)k;
  return gone;
}

size_t RelayDev::epochs(uint8_t out_le[32 * relay::EPOCHS_MAX]) const {
  const Impl& m = *d;
  if (m.n_window) memcpy(out_le, m.window, 32 * (size_t)m.n_window);
  return m.n_window;
}

void RelayDev::info(uint64_t out[8]) {
  Impl& m = *d;
  for (int k = 0; k < 8; k++) out[k] = m.stats[k];
  out[5] = 0;
  if (m.cap) {
    OnDevice on(m.device);
    hipStream_t ls = (hipStream_t)m.log.relay_rows().stream;
    const size_t bytes = m.out_bytes(m.cap);
    std::vector<uint8_t> dev(bytes);
    RLN_HIP(hipMemcpyAsync(dev.data(), m.out_dev.p, bytes, hipMemcpyDeviceToHost, ls));
    RLN_HIP(hipStreamSynchronize(ls));
    out[5] = nonzero_words16(dev.data(), bytes) + nonzero_words16(m.out_host, Impl::result_bytes(m.cap));
  }
}

}  // namespace rlnamd
