// The nullifier log on the device: the two kernels over nullifier_log.h and the NullifierLogDev object.
//
// One observe() call: a host check, the shares and tags copied into rows [count, count + n) of the record arrays,
// k_log_insert, k_log_judge, one copy back of statuses, secrets and first tags, one stream wait.  The records are
// written by the copy and read only by the kernels behind it, and the judge pass is a kernel of its own behind the
// insert pass, so nothing inside a kernel depends on another lane's plain store: the only words lanes share are the
// table entries, and those are touched with agent-scope atomics alone (the table is shared by all XCDs, whose L2s are
// not coherent with each other).
#include "nullifier_log.h"

#include <string.h>
#include <sys/random.h>

#include <string>
#include <vector>

#include "common.h"

namespace rlnamd {

using nlog::Row32;
using nlog::Row96;
using nlog::View;

namespace {

struct DevAtomics {
  static __device__ __forceinline__ uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) {
    __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expect;   // on failure the exchange has put the entry found there
  }
  static __device__ __forceinline__ void min(uint32_t* p, uint32_t v) {
    __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ uint32_t load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

constexpr uint32_t LOG_LANES = 256;

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
    const uint64_t t = tags ? tags[i] : m.count + i;
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
  const View L = m.view();
  hipLaunchKernelGGL(k_log_insert, dim3(div_up(n, LOG_LANES)), dim3(LOG_LANES), 0, m.stream, L, first_id, n32);
  hipLaunchKernelGGL(k_log_judge, dim3(div_up(n, LOG_LANES)), dim3(LOG_LANES), 0, m.stream, L, first_id, n32, d_status,
                     (Row32*)d_secrets, (uint64_t*)d_first, (uint32_t*)m.out_dev.p);
  RLN_HIP(hipGetLastError());
  // from here on the table holds the call's ids: the records count as taken whatever happens next
  m.count += n;
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
}

void NullifierLogDev::get(uint64_t seq, uint8_t share_le[128], uint64_t* tag) {
  Impl& m = *d;
  if (seq >= m.count)
    throw Error("nullifier log: no record " + std::to_string(seq) + ", " + std::to_string(m.count) + " shares are recorded");
  if (!share_le) throw Error("nullifier log: get was given a null pointer");
  OnDevice on(m.device);
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

}  // namespace rlnamd
