// The nullifier log on the device: the kernels over nullifier_log.h and the NullifierLogDev object.
//
// One observe() call: a host check, the shares and tags copied into rows [count, count + n) of the record arrays,
// k_log_insert, k_log_judge, one copy back of statuses, secrets and first tags, one stream wait.  The records are
// written by the copy and read only by the kernels behind it, and the judge pass is a kernel of its own behind the
// insert pass, so nothing inside a kernel depends on another lane's plain store: the only words lanes share are the
// table entries, and those are touched with agent-scope atomics alone (the table is shared by all XCDs, whose L2s are
// not coherent with each other).
//
// One retire() call: a host check, then on the log's stream
//   k_log_mark                keep[i] = the record's external nullifier is not in the set (the set in LDS); a retain()
//                             call is a retire() whose mark keeps what IS in the set, and nothing else differs
//   k_scan_up / k_scan_down   pos[i] = kept records below i: block sums of block sums, one kernel per level up and one
//                             per level down, as many levels as the count asks for (256 items a block: 4 for 2^24 + 1)
//   k_log_move                kept row i -> row pos[i] of the spare record arrays, which then become the live ones
//   memset, k_log_insert      the table emptied and the survivors inserted again: the lowest surviving row of a key
//                             ends up in the key's slot
//   k_log_census              taken slots (= distinct nullifiers) and the longest walk, one pair of atomics a workgroup
//                             of a capped grid
// The same rule holds as above: no lane waits for, or reads, what another lane of the same kernel writes -- a level of
// the scan reads what the kernel before it wrote, the move reads positions the last scan kernel wrote and writes rows
// nobody reads before the insert pass.  A single-pass scan, in which a block looks back at its predecessors' sums,
// would be fewer launches and is exactly what that rule forbids: it spins on other workgroups' stores across XCDs.
// (The scan's kernels are in log_scan.h, which relay.hip shares.)
#include "nullifier_log.h"

#include <string.h>
#include <sys/random.h>

#include <algorithm>
#include <string>
#include <vector>

#include "common.h"
#include "log_scan.h"

namespace rlnamd {

using nlog::DevAtomics;
using nlog::Row32;
using nlog::Records;
using nlog::Row96;
using nlog::View;

namespace {

// one lane per share: record first_id + i takes its key's slot, or lowers the id that slot holds
__global__ void __launch_bounds__(LOG_LANES) k_log_insert(View L, uint32_t first_id, uint32_t n) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i < n) nlog::insert<DevAtomics>(L, first_id + i);
}

// one lane per share, behind the whole insert pass: the verdict, the secret of a SPAM share (zero otherwise), the tag of
// the first record with the nullifier; the longest walk of the call goes into *longest (one atomic per workgroup)
__global__ void __launch_bounds__(LOG_LANES) k_log_judge(View L, uint32_t first_id, uint32_t n, uint8_t* __restrict__ status,
                                                         Row32* __restrict__ secrets, uint64_t* __restrict__ first_tag,
                                                         uint32_t* __restrict__ longest) {
  __shared__ uint32_t wg_walk;
  if (threadIdx.x == 0) wg_walk = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i < n) {
    const nlog::Verdict v = nlog::judge<DevAtomics>(L, first_id + i);
    status[i] = v.status;
    secrets[i] = v.secret;
    first_tag[i] = L.tags[v.first];
    atomicMax(&wg_walk, v.walk);
  }
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_fetch_max(longest, wg_walk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------- retire
// keep[i]: record i stays (retain: the sense of the set, nlog::keeps).  The set goes to LDS once per workgroup; a lane
// reads the 32 bytes of its row's external nullifier and nothing else of the 96.
__global__ void __launch_bounds__(LOG_LANES) k_log_mark(const Row96* __restrict__ rest, uint32_t n,
                                                        const Row32* __restrict__ set, uint32_t k, uint32_t retain,
                                                        uint8_t* __restrict__ keep) {
  __shared__ Row32 lds_set[nlog::RETIRE_MAX];
  for (uint32_t j = threadIdx.x; j < k * 8; j += LOG_LANES) lds_set[j >> 3].w[j & 7] = set[j >> 3].w[j & 7];
  __syncthreads();
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i < n) keep[i] = nlog::keeps(rest[i].ext, lds_set, k, retain != 0) ? 1 : 0;
}

// kept row i -> row pos[i] of the other set of record arrays.  dense: no sequence numbers are stored yet, row i is
// sequence number i.
__global__ void __launch_bounds__(LOG_LANES) k_log_move(const Row32* __restrict__ nul, const Row96* __restrict__ rest,
                                                        const uint64_t* __restrict__ tags, const uint64_t* __restrict__ seqs,
                                                        Records to, const uint8_t* __restrict__ keep,
                                                        const uint32_t* __restrict__ pos, uint32_t n, int dense) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i >= n || !keep[i]) return;
  const uint32_t p = pos[i];   // the kept rows below i: at most i
  if (p > i) return;           // (not reached; a write past the arrays is not an answer to a wrong position)
  to.nul[p] = nul[i];
  to.rest[p] = rest[i];
  to.tags[p] = tags[i];
  to.seqs[p] = dense ? (uint64_t)i : seqs[i];
}

// Behind the insert pass of a rebuild, a lane per slot in a grid-stride loop: stat[0] += taken slots, stat[1] = max(the
// walk from a key's home slot to its slot), which is the longest walk that insert pass made.  The grid is capped at
// CENSUS_BLOCKS workgroups, each ending in one pair of atomics: with a workgroup per 256 slots the 2^17 pairs of a
// 2^25-slot table, all on the same two words, took 3.0 ms of a 4.9 ms retire (profiles/nullifier_log_retire.md).
constexpr uint32_t CENSUS_BLOCKS = 2048;
__global__ void __launch_bounds__(LOG_LANES) k_log_census(View L, uint32_t* __restrict__ stat) {
  __shared__ uint32_t wg_taken, wg_walk;
  if (threadIdx.x == 0) wg_taken = 0, wg_walk = 0;
  __syncthreads();
  uint32_t taken = 0, longest = 0;
  for (uint64_t s = (uint64_t)blockIdx.x * LOG_LANES + threadIdx.x; s < L.slots; s += (uint64_t)gridDim.x * LOG_LANES) {
    const uint32_t e = L.table[s];
    if (e == nlog::EMPTY) continue;
    const uint32_t walk = (uint32_t)((s - nlog::home_slot(L.nul[e], L.seed, L.slots)) & (L.slots - 1)) + 1;
    taken++;
    if (walk > longest) longest = walk;
  }
  if (taken) {
    atomicAdd(&wg_taken, taken);
    atomicMax(&wg_walk, longest);
  }
  __syncthreads();
  if (threadIdx.x == 0 && wg_taken) {
    __hip_atomic_fetch_add(&stat[0], wg_taken, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(&stat[1], wg_walk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// the sequence numbers of the rows of one observe call, once rows and sequence numbers have parted
__global__ void __launch_bounds__(LOG_LANES) k_log_number(uint64_t* __restrict__ seqs, uint64_t first_seq, uint32_t n) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i < n) seqs[i] = first_seq + i;
}

// get() after a retire, one lane: the row that carries `seq`, or `count`
__global__ void k_log_find(const uint64_t* __restrict__ seqs, uint64_t count, uint64_t seq, uint32_t* __restrict__ row) {
  *row = (uint32_t)nlog::find_seq(seqs, count, seq);
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

struct OnDevice {   // the log's device for the length of a call, the caller's afterwards
  int prev = 0, dev;
  explicit OnDevice(int dev_) : dev(dev_) {
    RLN_HIP(hipGetDevice(&prev));
    if (prev != dev) RLN_HIP(hipSetDevice(dev));
  }
  ~OnDevice() {
    if (prev != dev) (void)hipSetDevice(prev);
  }
};

}  // namespace

struct NullifierLogDev::Impl {
  int device = 0;
  hipStream_t stream = nullptr;
  uint64_t capacity = 0, slots = 0, seed = 0;
  uint64_t count = 0, distinct = 0, calls = 0, longest = 0;
  DevBuf<Row32> nul;
  DevBuf<Row96> rest;
  DevBuf<uint64_t> tags;
  DevBuf<uint32_t> table;
  // Retiring.  next_seq: the sequence number (and default tag) of the next share.  dense: row == sequence number, seqs
  // is not in use (until the first retire that removes something, and again after clear()).  The spare record arrays
  // and the scratch of the passes come with a log's first retire that reaches the device, all or none, and stay.
  uint64_t next_seq = 0, retires = 0, removed = 0, rebuild_longest = 0;
  bool dense = true, spare = false;
  DevBuf<uint64_t> seqs;
  DevBuf<Row32> spare_nul;
  DevBuf<Row96> spare_rest;
  DevBuf<uint64_t> spare_tags, spare_seqs;
  DevBuf<uint8_t> keep;
  DevBuf<uint32_t> pos, sums;
  DevBuf<uint32_t> stat;    // [0] taken slots, [1] longest walk of a rebuild, [3] the row get() asked for
  DevBuf<Row32> set_dev;
  nlog::RetireSet set_host;   // (a member: the copy to the device reads it)
  // staging of one call of up to stage_n shares
  //   in  (pinned):          [nullifiers 32 n][x | y | ext 96 n][tags 8 n]
  //   out (device + pinned): [longest walk: 16 B][secrets 32 n][first tags 8 n][statuses n]
  // `out` is all zero between calls, on the device and in the pinned copy: what a call wrote there is overwritten before
  // observe() returns -- the secrets because they are secrets, the rest with them so that no later, smaller call leaves
  // public bytes where info() looks for secrets -- and the same memset resets the walk counter for the next call.
  size_t stage_n = 0;
  uint8_t* in_host = nullptr;
  uint8_t* out_host = nullptr;
  DevBuf<uint8_t> out_dev;

  static size_t in_bytes(size_t n) { return n * 136; }
  static size_t out_bytes(size_t n) { return 16 + (n * 41 + 15) / 16 * 16; }
  View view() const { return View{nul.p, rest.p, tags.p, table.p, slots, seed}; }
  // the passes of retire() and retain() behind their host checks: 1 <= k <= RETIRE_MAX canonical elements
  uint64_t remove(size_t k, const uint8_t* external_nullifiers_le, bool retain);

  void reserve_retire() {
    if (spare) return;
    try {
      DevBuf<uint64_t> a_seqs(capacity), b_seqs(capacity), b_tags(capacity);
      DevBuf<Row32> b_nul(capacity), a_set(nlog::RETIRE_MAX);
      DevBuf<Row96> b_rest(capacity);
      DevBuf<uint8_t> a_keep(capacity);
      DevBuf<uint32_t> a_pos(capacity), a_sums(ScanPlan(capacity).words), a_stat(4);
      seqs = std::move(a_seqs);
      spare_seqs = std::move(b_seqs);
      spare_tags = std::move(b_tags);
      spare_nul = std::move(b_nul);
      spare_rest = std::move(b_rest);
      set_dev = std::move(a_set);
      keep = std::move(a_keep);
      pos = std::move(a_pos);
      sums = std::move(a_sums);
      stat = std::move(a_stat);
    } catch (...) {
      (void)hipGetLastError();   // what was allocated is freed again, and the log is as it was, its error state too
      throw;
    }
    spare = true;
  }
  void reserve(size_t n) {
    if (n <= stage_n) return;
    release_staging();
    const size_t m = n < 1024 ? 1024 : n;
    RLN_HIP(hipHostMalloc((void**)&in_host, in_bytes(m), hipHostMallocDefault));
    RLN_HIP(hipHostMalloc((void**)&out_host, out_bytes(m), hipHostMallocDefault));
    memset(out_host, 0, out_bytes(m));
    out_dev.alloc(out_bytes(m));
    RLN_HIP(hipMemsetAsync(out_dev.p, 0, out_bytes(m), stream));
    stage_n = m;
  }
  // (what held secrets is zero already -- observe() wipes before it returns -- and is wiped once more before it is freed)
  void release_staging() {
    if (out_dev.p) {
      (void)hipMemsetAsync(out_dev.p, 0, out_bytes(stage_n), stream);
      (void)hipStreamSynchronize(stream);
    }
    if (out_host) {
      wipe_host(out_host, out_bytes(stage_n));
      (void)hipHostFree(out_host);
    }
    if (in_host) (void)hipHostFree(in_host);
    out_dev.release();
    in_host = out_host = nullptr;
    stage_n = 0;
  }
  ~Impl() {
    if (stream) (void)hipStreamSynchronize(stream);
    release_staging();
    if (stream) (void)hipStreamDestroy(stream);
  }
};

NullifierLogDev::NullifierLogDev(uint64_t capacity, uint64_t seed) {
  if (capacity == 0) throw Error("nullifier log: the capacity must be at least 1");
  if (capacity > nlog::MAX_CAPACITY) throw Error("nullifier log: the capacity must be at most 2^31 shares");
  require_gpu();
  for (int tries = 0; seed == 0 && tries < 8; tries++)
    if (getrandom(&seed, sizeof seed, 0) != (ssize_t)sizeof seed) seed = 0;
  if (seed == 0) throw Error("nullifier log: getrandom gave no seed");
  Impl* m = new Impl;
  try {
    RLN_HIP(hipGetDevice(&m->device));
    RLN_HIP(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    m->capacity = capacity;
    m->slots = nlog::slots_for(capacity);
    m->seed = seed;
    m->nul.alloc(capacity);
    m->rest.alloc(capacity);
    m->tags.alloc(capacity);
    m->table.alloc(m->slots);
    RLN_HIP(hipMemsetAsync(m->table.p, 0xFF, m->slots * 4, m->stream));
    RLN_HIP(hipStreamSynchronize(m->stream));
  } catch (...) {
    delete m;
    throw;
  }
  d = m;
}

NullifierLogDev::~NullifierLogDev() {
  if (!d) return;
  int prev = 0;
  const bool move = hipGetDevice(&prev) == hipSuccess && prev != d->device && hipSetDevice(d->device) == hipSuccess;
  delete d;
  if (move) (void)hipSetDevice(prev);
}

void NullifierLogDev::observe(size_t n, const uint8_t* shares_le, const uint64_t* tags, uint8_t* status, uint8_t* secrets_le,
                              uint64_t* first_tag) {
  Impl& m = *d;
  if (n == 0) return;
  // the host check: nothing is enqueued and nothing of the log changes before it has passed
  if (!shares_le || !status) throw Error("nullifier log: observe was given a null pointer for n > 0 shares");
  if (n > m.capacity - m.count)
    throw Error("nullifier log: " + std::to_string(n) + " shares do not fit: " + std::to_string(m.capacity - m.count) +
                " of " + std::to_string(m.capacity) + " records are left");
  for (size_t i = 0; i < n; i++)
    if (!nlog::share_is_canonical(shares_le + 128 * i))
      throw Error("nullifier log: share " + std::to_string(i) + " holds a field element that is not canonical (>= r)");

  OnDevice on(m.device);
  m.reserve(n);
  uint8_t* h_nul = m.in_host;
  uint8_t* h_rest = h_nul + 32 * n;
  uint8_t* h_tags = h_rest + 96 * n;
  for (size_t i = 0; i < n; i++) {
    memcpy(h_nul + 32 * i, shares_le + 128 * i, 32);
    memcpy(h_rest + 96 * i, shares_le + 128 * i + 32, 96);
    const uint64_t t = tags ? tags[i] : m.next_seq + i;
    memcpy(h_tags + 8 * i, &t, 8);
  }
  uint8_t* d_secrets = m.out_dev.p + 16;
  uint8_t* d_first = d_secrets + 32 * n;
  uint8_t* d_status = d_first + 8 * n;
  struct Wipe {   // success or error: what held secrets is zero again when observe() returns
    Impl& m;
    size_t n;
    bool device_done = false;
    ~Wipe() {
      if (!device_done) {
        (void)hipMemsetAsync(m.out_dev.p, 0, Impl::out_bytes(n), m.stream);
        (void)hipStreamSynchronize(m.stream);
      }
      wipe_host(m.out_host, Impl::out_bytes(n));
    }
  } wipe{m, n};

  const uint32_t first_id = (uint32_t)m.count, n32 = (uint32_t)n;
  // one staging block, one copy per record array (the rows of a call are contiguous in each of the three)
  RLN_HIP(hipMemcpyAsync(m.nul.p + m.count, h_nul, 32 * n, hipMemcpyHostToDevice, m.stream));
  RLN_HIP(hipMemcpyAsync(m.rest.p + m.count, h_rest, 96 * n, hipMemcpyHostToDevice, m.stream));
  RLN_HIP(hipMemcpyAsync(m.tags.p + m.count, h_tags, 8 * n, hipMemcpyHostToDevice, m.stream));
  if (!m.dense)
    hipLaunchKernelGGL(k_log_number, dim3(div_up(n, LOG_LANES)), dim3(LOG_LANES), 0, m.stream, m.seqs.p + m.count, m.next_seq, n32);
  const View L = m.view();
  hipLaunchKernelGGL(k_log_insert, dim3(div_up(n, LOG_LANES)), dim3(LOG_LANES), 0, m.stream, L, first_id, n32);
  hipLaunchKernelGGL(k_log_judge, dim3(div_up(n, LOG_LANES)), dim3(LOG_LANES), 0, m.stream, L, first_id, n32, d_status,
                     (Row32*)d_secrets, (uint64_t*)d_first, (uint32_t*)m.out_dev.p);
  RLN_HIP(hipGetLastError());
  // from here on the table holds the call's ids: the records count as taken whatever happens next
  m.count += n;
  m.next_seq += n;
  m.calls++;
  RLN_HIP(hipMemcpyAsync(m.out_host, m.out_dev.p, Impl::out_bytes(n), hipMemcpyDeviceToHost, m.stream));
  RLN_HIP(hipMemsetAsync(m.out_dev.p, 0, Impl::out_bytes(n), m.stream));   // behind the copy, in stream order
  RLN_HIP(hipStreamSynchronize(m.stream));
  wipe.device_done = true;

  const uint8_t* h_secrets = m.out_host + 16;
  const uint8_t* h_first = h_secrets + 32 * n;
  const uint8_t* h_status = h_first + 8 * n;
  uint32_t walk = 0;
  memcpy(&walk, m.out_host, 4);
  if (walk > m.longest) m.longest = walk;
  size_t fresh = 0;
  for (size_t i = 0; i < n; i++) {
    if (h_status[i] > nlog::FOREIGN) throw Error("nullifier log: internal error, a share's key is not in the table");
    fresh += h_status[i] == nlog::NEW;
  }
  m.distinct += fresh;
  memcpy(status, h_status, n);
  if (secrets_le) memcpy(secrets_le, h_secrets, 32 * n);
  if (first_tag) memcpy(first_tag, h_first, 8 * n);
}

void NullifierLogDev::clear() {
  Impl& m = *d;
  OnDevice on(m.device);
  RLN_HIP(hipMemsetAsync(m.table.p, 0xFF, m.slots * 4, m.stream));
  RLN_HIP(hipStreamSynchronize(m.stream));
  m.count = 0;
  m.distinct = 0;
  m.next_seq = 0;
  m.dense = true;
}

uint64_t NullifierLogDev::retire(size_t k, const uint8_t* external_nullifiers_le) {
  Impl& m = *d;
  // the host check: nothing is enqueued and nothing of the log changes before it has passed
  if (k > 0 && !external_nullifiers_le)
    throw Error("nullifier log: retire was given a null pointer for k > 0 external nullifiers");
  if (k > nlog::RETIRE_MAX)
    throw Error("nullifier log: retire takes at most " + std::to_string(nlog::RETIRE_MAX) + " external nullifiers a call, not " +
                std::to_string(k));
  for (size_t j = 0; j < k; j++)
    if (!nlog::element_is_canonical(external_nullifiers_le + 32 * j))
      throw Error("nullifier log: external nullifier " + std::to_string(j) + " of the retire is not canonical (>= r)");
  if (k == 0 || m.count == 0) {
    m.retires++;
    return 0;
  }
  return m.remove(k, external_nullifiers_le, false);
}

uint64_t NullifierLogDev::retain(size_t k, const uint8_t* external_nullifiers_le) {
  Impl& m = *d;
  // the host check: nothing is enqueued and nothing of the log changes before it has passed
  const std::string refused = nlog::retain_refusal(external_nullifiers_le, k);
  if (!refused.empty()) throw Error(refused);
  if (m.count == 0) {
    m.retires++;
    return 0;
  }
  return m.remove(k, external_nullifiers_le, true);
}

uint64_t NullifierLogDev::Impl::remove(size_t k, const uint8_t* external_nullifiers_le, bool retain) {
  Impl& m = *this;
  OnDevice on(m.device);
  m.reserve_retire();
  m.retires++;
  memcpy(m.set_host.e, external_nullifiers_le, 32 * k);
  m.set_host.k = (uint32_t)k;
  m.set_host.retain = retain ? 1 : 0;
  const uint32_t n32 = (uint32_t)m.count;
  RLN_HIP(hipMemcpyAsync(m.set_dev.p, m.set_host.e, 32 * k, hipMemcpyHostToDevice, m.stream));
  hipLaunchKernelGGL(k_log_mark, dim3(div_up(m.count, LOG_LANES)), dim3(LOG_LANES), 0, m.stream, (const Row96*)m.rest.p, n32,
                     (const Row32*)m.set_dev.p, m.set_host.k, m.set_host.retain, m.keep.p);
  const uint32_t* d_kept = scan_positions(m.keep.p, m.count, m.pos.p, m.sums.p, m.stream);
  uint32_t kept = 0;
  RLN_HIP(hipMemcpyAsync(&kept, d_kept, 4, hipMemcpyDeviceToHost, m.stream));
  RLN_HIP(hipStreamSynchronize(m.stream));
  if (kept > m.count) throw Error("nullifier log: internal error, the position pass kept more records than there are");
  const uint64_t gone = m.count - kept;
  if (gone == 0) return 0;   // nothing matches: nothing moves
  uint32_t stat[2] = {0, 0};
  if (kept == 0) {
    RLN_HIP(hipMemsetAsync(m.table.p, 0xFF, m.slots * 4, m.stream));
    RLN_HIP(hipStreamSynchronize(m.stream));
  } else {
    const Records to{m.spare_nul.p, m.spare_rest.p, m.spare_tags.p, m.spare_seqs.p};
    hipLaunchKernelGGL(k_log_move, dim3(div_up(m.count, LOG_LANES)), dim3(LOG_LANES), 0, m.stream, (const Row32*)m.nul.p,
                       (const Row96*)m.rest.p, (const uint64_t*)m.tags.p, (const uint64_t*)m.seqs.p, to, (const uint8_t*)m.keep.p,
                       (const uint32_t*)m.pos.p, n32, m.dense ? 1 : 0);
    RLN_HIP(hipMemsetAsync(m.table.p, 0xFF, m.slots * 4, m.stream));
    RLN_HIP(hipMemsetAsync(m.stat.p, 0, 8, m.stream));
    const View L{to.nul, to.rest, to.tags, m.table.p, m.slots, m.seed};
    hipLaunchKernelGGL(k_log_insert, dim3(div_up(kept, LOG_LANES)), dim3(LOG_LANES), 0, m.stream, L, 0u, kept);
    hipLaunchKernelGGL(k_log_census, dim3(std::min<uint64_t>((m.slots + LOG_LANES - 1) / LOG_LANES, CENSUS_BLOCKS)), dim3(LOG_LANES), 0,
                       m.stream, L, m.stat.p);
    RLN_HIP(hipGetLastError());
    RLN_HIP(hipMemcpyAsync(stat, m.stat.p, 8, hipMemcpyDeviceToHost, m.stream));
    RLN_HIP(hipStreamSynchronize(m.stream));
    std::swap(m.nul, m.spare_nul);
    std::swap(m.rest, m.spare_rest);
    std::swap(m.tags, m.spare_tags);
    std::swap(m.seqs, m.spare_seqs);
  }
  m.count = kept;
  m.distinct = stat[0];
  m.rebuild_longest = stat[1];
  m.removed += gone;
  m.dense = false;
  return gone;
}

void NullifierLogDev::get(uint64_t seq, uint8_t share_le[128], uint64_t* tag) {
  Impl& m = *d;
  if (seq >= m.next_seq)
    throw Error("nullifier log: no record " + std::to_string(seq) + ", " + std::to_string(m.count) + " shares are recorded");
  if (!share_le) throw Error("nullifier log: get was given a null pointer");
  OnDevice on(m.device);
  if (!m.dense) {   // rows and sequence numbers have parted: the row by binary search on the device
    uint32_t row = (uint32_t)m.count;
    if (m.count) {
      hipLaunchKernelGGL(k_log_find, dim3(1), dim3(1), 0, m.stream, (const uint64_t*)m.seqs.p, m.count, seq, m.stat.p + 3);
      RLN_HIP(hipGetLastError());
      RLN_HIP(hipMemcpyAsync(&row, m.stat.p + 3, 4, hipMemcpyDeviceToHost, m.stream));
      RLN_HIP(hipStreamSynchronize(m.stream));
    }
    if (row >= m.count) throw Error("nullifier log: record " + std::to_string(seq) + " was retired");
    seq = row;
  }
  uint64_t t = 0;
  RLN_HIP(hipMemcpyAsync(share_le, m.nul.p + seq, 32, hipMemcpyDeviceToHost, m.stream));
  RLN_HIP(hipMemcpyAsync(share_le + 32, m.rest.p + seq, 96, hipMemcpyDeviceToHost, m.stream));
  RLN_HIP(hipMemcpyAsync(&t, m.tags.p + seq, 8, hipMemcpyDeviceToHost, m.stream));
  RLN_HIP(hipStreamSynchronize(m.stream));
  if (tag) *tag = t;
}

uint64_t NullifierLogDev::home_slot(const uint8_t nullifier_le[32]) const {
  Row32 key;
  memcpy(key.w, nullifier_le, 32);
  return nlog::home_slot(key, d->seed, d->slots);
}

void NullifierLogDev::info(uint64_t out[8]) {
  Impl& m = *d;
  out[0] = m.capacity;
  out[1] = m.count;
  out[2] = m.slots;
  out[3] = m.distinct;
  out[4] = m.calls;
  out[5] = m.longest;
  out[6] = 0;
  out[7] = m.seed;
  if (m.stage_n) {
    OnDevice on(m.device);
    const size_t bytes = Impl::out_bytes(m.stage_n);
    std::vector<uint8_t> dev(bytes);
    RLN_HIP(hipMemcpyAsync(dev.data(), m.out_dev.p, bytes, hipMemcpyDeviceToHost, m.stream));
    RLN_HIP(hipStreamSynchronize(m.stream));
    out[6] = nonzero_words16(dev.data(), bytes) + nonzero_words16(m.out_host, bytes);
  }
}

void NullifierLogDev::retire_info(uint64_t out[8]) {
  const Impl& m = *d;
  out[0] = m.retires;
  out[1] = m.removed;
  out[2] = m.next_seq;
  out[3] = m.count;
  out[4] = m.rebuild_longest;
  out[5] = m.spare ? 1 : 0;
  out[6] = out[7] = 0;
}

NullifierLogDev::RelayRows NullifierLogDev::relay_rows() {
  Impl& m = *d;
  return RelayRows{Records{m.nul.p, m.rest.p, m.tags.p, m.dense ? nullptr : m.seqs.p}, m.view(), m.count, m.capacity, m.next_seq,
                   (void*)m.stream, m.device};
}

int NullifierLogDev::device() const { return d->device; }

void NullifierLogDev::relay_commit(uint64_t n, uint32_t walk, uint64_t fresh) {
  Impl& m = *d;
  m.count += n;
  m.next_seq += n;
  m.calls++;
  m.distinct += fresh;
  if (walk > m.longest) m.longest = walk;
}

void probe_log_positions(const uint8_t* keep, size_t n, uint32_t* pos, uint64_t* kept) {
  if (kept) *kept = 0;
  if (n == 0) return;
  if (!keep || !pos) throw Error("probe_log_positions: null pointer");
  if (n > nlog::MAX_CAPACITY) throw Error("probe_log_positions: at most 2^31 items");
  require_gpu();
  DevBuf<uint8_t> d_keep(n);
  DevBuf<uint32_t> d_pos(n), d_sums(ScanPlan(n).words);
  RLN_HIP(hipMemcpyAsync(d_keep.p, keep, n, hipMemcpyHostToDevice, 0));
  const uint32_t* d_kept = scan_positions(d_keep.p, n, d_pos.p, d_sums.p, 0);
  uint32_t total = 0;
  RLN_HIP(hipMemcpyAsync(pos, d_pos.p, 4 * n, hipMemcpyDeviceToHost, 0));
  RLN_HIP(hipMemcpyAsync(&total, d_kept, 4, hipMemcpyDeviceToHost, 0));
  RLN_HIP(hipStreamSynchronize(0));
  if (kept) *kept = total;
}

}  // namespace rlnamd
