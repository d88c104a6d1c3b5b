// Signals to field elements on the device: the kernel over keccak_batch.h and the HasherDev object.
//
// One hash_to_field() call: the plan (host only; a refused call enqueues nothing), then for each chunk the pack into a
// pinned half, one copy of the packed chunk and one launch of k_hash_to_field -- behind the first chunk's launch the
// host's own messages, hashed on the calling thread while the device works --, then one copy back of every lane's row,
// one stream wait, and the rows put where their messages are.  A lane reads its own blocks, which the copy in front of
// the kernel wrote, and writes its own row: no lane reads what another lane writes, there is no atomic, no LDS and no
// barrier.
//
// A pinned half is packed again two chunks later: the event behind its copy is waited for first.  Its device twin
// needs no event, the stream orders the next copy into it behind the kernel that read it.
//
// Signals are public bytes (they travel in the clear beside the proof): nothing here is wiped.
#include "keccak_batch.h"

#include <stdlib.h>

#include <string>

#include "common.h"

namespace rlnamd {

namespace {

constexpr uint32_t HASH_LANES = 64;   // a wave per workgroup: 1 024 waves of a 65 536-message call spread over every CU

// lane j of the chunk: blocks [first_block[j], first_block[j + 1]) of `blocks`, result in row j of `rows`
__global__ void __launch_bounds__(HASH_LANES) k_hash_to_field(const uint32_t* __restrict__ first_block,
                                                              const uint64_t* __restrict__ blocks, uint32_t n,
                                                              uint4* __restrict__ rows) {
  const uint32_t j = blockIdx.x * HASH_LANES + threadIdx.x;
  if (j >= n) return;
  uint32_t v[8];
  kbatch::hash_blocks(blocks, first_block[j], first_block[j + 1], v);
  rows[2 * (size_t)j] = make_uint4(v[0], v[1], v[2], v[3]);
  rows[2 * (size_t)j + 1] = make_uint4(v[4], v[5], v[6], v[7]);
}

// the same lane, its row put where its message is: row order[j] (the relay step keeps the rows on the device)
__global__ void __launch_bounds__(HASH_LANES) k_hash_to_field_at(const uint32_t* __restrict__ first_block,
                                                                 const uint64_t* __restrict__ blocks,
                                                                 const uint32_t* __restrict__ order, uint32_t n,
                                                                 uint32_t n_rows, uint4* __restrict__ rows) {
  const uint32_t j = blockIdx.x * HASH_LANES + threadIdx.x;
  if (j >= n) return;
  uint32_t v[8];
  kbatch::hash_blocks(blocks, first_block[j], first_block[j + 1], v);
  const uint32_t i = order[j];
  if (i >= n_rows) return;   // (not reached: order is a permutation of the call's messages)
  rows[2 * (size_t)i] = make_uint4(v[0], v[1], v[2], v[3]);
  rows[2 * (size_t)i + 1] = make_uint4(v[4], v[5], v[6], v[7]);
}

struct OnDevice {   // the hasher's device for the length of a call, the caller's afterwards
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

struct HasherDev::Impl {
  int device = 0;
  hipStream_t stream = nullptr;
  size_t half_blocks = 0, lane_max_blocks = 0;
  bool sorted = true;
  uint8_t* half_host[2] = {nullptr, nullptr};
  DevBuf<uint8_t> half_dev[2];
  hipEvent_t copied[2] = {nullptr, nullptr};   // behind the last copy out of half_host[h]
  // every lane's row of a call, in lane order; grows with the largest call seen
  size_t rows_n = 0;
  uint8_t* rows_host = nullptr;
  DevBuf<uint8_t> rows_dev;
  uint64_t last[5] = {0, 0, 0, 0, 0}, calls = 0;
  kbatch::Plan plan;
  // relay_hash: the lanes' part of order[], and the rows of the host's messages on their way to the device
  size_t order_n = 0;
  uint32_t* order_host = nullptr;
  DevBuf<uint32_t> order_dev;
  size_t host_rows_n = 0;
  uint8_t* host_rows = nullptr;

  void reserve_order(size_t n) {
    if (n <= order_n) return;
    RLN_HIP(hipStreamSynchronize(stream));
    if (order_host) (void)hipHostFree(order_host);
    order_host = nullptr;
    order_n = 0;
    order_dev.release();
    RLN_HIP(hipHostMalloc((void**)&order_host, 4 * n, hipHostMallocDefault));
    order_dev.alloc(n);
    order_n = n;
  }
  void reserve_host_rows(size_t n) {
    if (n <= host_rows_n) return;
    RLN_HIP(hipStreamSynchronize(stream));
    if (host_rows) (void)hipHostFree(host_rows);
    host_rows = nullptr;
    host_rows_n = 0;
    const size_t m = n < 64 ? 64 : n;
    RLN_HIP(hipHostMalloc((void**)&host_rows, 32 * m, hipHostMallocDefault));
    host_rows_n = m;
  }

  void reserve_rows(size_t n) {
    if (n <= rows_n) return;
    RLN_HIP(hipStreamSynchronize(stream));
    if (rows_host) (void)hipHostFree(rows_host);
    rows_host = nullptr;
    rows_n = 0;
    rows_dev.release();
    RLN_HIP(hipHostMalloc((void**)&rows_host, 32 * n, hipHostMallocDefault));
    rows_dev.alloc(32 * n);
    rows_n = n;
  }
  ~Impl() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (int h = 0; h < 2; h++) {
      if (copied[h]) (void)hipEventDestroy(copied[h]);
      if (half_host[h]) (void)hipHostFree(half_host[h]);
    }
    if (rows_host) (void)hipHostFree(rows_host);
    if (order_host) (void)hipHostFree(order_host);
    if (host_rows) (void)hipHostFree(host_rows);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

HasherDev::HasherDev(size_t stage_bytes, size_t lane_max_blocks) {
  if (stage_bytes == 0) stage_bytes = kbatch::DEFAULT_STAGE_BYTES;
  if (lane_max_blocks == 0) lane_max_blocks = kbatch::DEFAULT_LANE_MAX_BLOCKS;
  if (stage_bytes < 2 * kbatch::RATE) throw Error("hasher: stage_bytes must hold two halves of at least one 136-byte block");
  if (stage_bytes > kbatch::MAX_STAGE_BYTES) throw Error("hasher: stage_bytes must be at most 2^30");
  require_gpu();
  Impl* m = new Impl;
  try {
    m->half_blocks = stage_bytes / 2 / kbatch::RATE;
    m->lane_max_blocks = lane_max_blocks;
    // RLNAMD_HASH_LANE_ORDER=0: lanes in index order (the measurement's row without the ordering)
    if (const char* e = getenv("RLNAMD_HASH_LANE_ORDER"))
      if (*e) m->sorted = atol(e) != 0;
    RLN_HIP(hipGetDevice(&m->device));
    RLN_HIP(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    for (int h = 0; h < 2; h++) {
      RLN_HIP(hipHostMalloc((void**)&m->half_host[h], kbatch::half_bytes(m->half_blocks), hipHostMallocDefault));
      m->half_dev[h].alloc(kbatch::half_bytes(m->half_blocks));
      RLN_HIP(hipEventCreateWithFlags(&m->copied[h], hipEventDisableTiming));
    }
    m->reserve_rows(std::min<size_t>(2 * m->half_blocks, 65536));
  } catch (...) {
    delete m;
    throw;
  }
  d = m;
}

HasherDev::~HasherDev() {
  if (!d) return;
  int prev = 0;
  const bool move = hipGetDevice(&prev) == hipSuccess && prev != d->device && hipSetDevice(d->device) == hipSuccess;
  delete d;
  if (move) (void)hipSetDevice(prev);
}

void HasherDev::hash_to_field(const uint8_t* data, size_t data_len, const uint64_t* offsets, size_t n, uint8_t* out_le) {
  Impl& m = *d;
  if (n == 0) return;
  if (!out_le) throw Error("hash_to_field: null output for n > 0 messages");
  kbatch::Plan& P = m.plan;
  if (const char* refused = kbatch::plan_call(data, data_len, offsets, n, m.half_blocks, m.lane_max_blocks, m.sorted, &P))
    throw Error(refused);

  OnDevice on(m.device);
  const size_t n_dev = P.n - P.n_host;
  m.reserve_rows(n_dev);
  // the host's messages, hashed behind the first chunk's launch: that chunk holds the longest lanes, the ones the
  // host's share was measured against
  auto host_share = [&]() {
    for (size_t j = 0; j < P.n_host; j++) {
      const uint32_t i = P.order[j];
      kbatch::hash_message(data + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), out_le + 32 * (size_t)i);
    }
  };
  for (size_t k = 0; k < P.chunks.size(); k++) {
    const kbatch::Chunk& c = P.chunks[k];
    const int h = (int)(k & 1);
    if (k >= 2) RLN_HIP(hipEventSynchronize(m.copied[h]));   // the copy of chunk k - 2 has left this half
    const size_t bytes = kbatch::pack_chunk(P, c, data, offsets, m.half_host[h]);
    RLN_HIP(hipMemcpyAsync(m.half_dev[h].p, m.half_host[h], bytes, hipMemcpyHostToDevice, m.stream));
    RLN_HIP(hipEventRecord(m.copied[h], m.stream));
    hipLaunchKernelGGL(k_hash_to_field, dim3(div_up(c.count, HASH_LANES)), dim3(HASH_LANES), 0, m.stream,
                       (const uint32_t*)m.half_dev[h].p, (const uint64_t*)(m.half_dev[h].p + kbatch::header_bytes(c.count)),
                       (uint32_t)c.count, (uint4*)(m.rows_dev.p + 32 * (c.first - P.n_host)));
    RLN_HIP(hipGetLastError());
    if (k == 0) host_share();
  }
  if (P.chunks.empty()) host_share();
  if (n_dev) RLN_HIP(hipMemcpyAsync(m.rows_host, m.rows_dev.p, 32 * n_dev, hipMemcpyDeviceToHost, m.stream));
  RLN_HIP(hipStreamSynchronize(m.stream));
  for (size_t j = 0; j < n_dev; j++) memcpy(out_le + 32 * (size_t)P.order[P.n_host + j], m.rows_host + 32 * j, 32);
  m.last[0] = n_dev;
  m.last[1] = P.n_host;
  m.last[2] = P.chunks.size();
  m.last[3] = P.device_blocks;
  m.last[4] = P.longest_lane;
  m.calls++;
}

size_t HasherDev::relay_hash(const uint8_t* data, size_t data_len, const uint64_t* offsets, size_t n, uint8_t* rows_dev) {
  Impl& m = *d;
  if (n == 0) return 0;
  if (!rows_dev) throw Error("hash_to_field: null output for n > 0 messages");
  kbatch::Plan& P = m.plan;
  if (const char* refused = kbatch::plan_call(data, data_len, offsets, n, m.half_blocks, m.lane_max_blocks, m.sorted, &P))
    throw Error(refused);

  OnDevice on(m.device);
  const size_t n_dev = P.n - P.n_host;
  m.reserve_order(n_dev);
  m.reserve_host_rows(P.n_host);
  if (n_dev) {
    memcpy(m.order_host, P.order.data() + P.n_host, 4 * n_dev);
    RLN_HIP(hipMemcpyAsync(m.order_dev.p, m.order_host, 4 * n_dev, hipMemcpyHostToDevice, m.stream));
  }
  // the host's messages behind the first chunk's launch, as hash_to_field has them; their rows go up one by one
  auto host_share = [&]() {
    for (size_t j = 0; j < P.n_host; j++) {
      const uint32_t i = P.order[j];
      kbatch::hash_message(data + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), m.host_rows + 32 * j);
      RLN_HIP(hipMemcpyAsync(rows_dev + 32 * (size_t)i, m.host_rows + 32 * j, 32, hipMemcpyHostToDevice, m.stream));
    }
  };
  for (size_t k = 0; k < P.chunks.size(); k++) {
    const kbatch::Chunk& c = P.chunks[k];
    const int h = (int)(k & 1);
    if (k >= 2) RLN_HIP(hipEventSynchronize(m.copied[h]));   // the copy of chunk k - 2 has left this half
    const size_t bytes = kbatch::pack_chunk(P, c, data, offsets, m.half_host[h]);
    RLN_HIP(hipMemcpyAsync(m.half_dev[h].p, m.half_host[h], bytes, hipMemcpyHostToDevice, m.stream));
    RLN_HIP(hipEventRecord(m.copied[h], m.stream));
    hipLaunchKernelGGL(k_hash_to_field_at, dim3(div_up(c.count, HASH_LANES)), dim3(HASH_LANES), 0, m.stream,
                       (const uint32_t*)m.half_dev[h].p, (const uint64_t*)(m.half_dev[h].p + kbatch::header_bytes(c.count)),
                       (const uint32_t*)(m.order_dev.p + (c.first - P.n_host)), (uint32_t)c.count, (uint32_t)n,
                       (uint4*)rows_dev);
    RLN_HIP(hipGetLastError());
    if (k == 0) host_share();
  }
  if (P.chunks.empty()) host_share();
  m.last[0] = n_dev;
  m.last[1] = P.n_host;
  m.last[2] = P.chunks.size();
  m.last[3] = P.device_blocks;
  m.last[4] = P.longest_lane;
  m.calls++;
  return P.n_host;
}

void* HasherDev::relay_stream() { return (void*)d->stream; }
int HasherDev::device() const { return d->device; }

void HasherDev::info(uint64_t out[8]) {
  Impl& m = *d;
  for (int k = 0; k < 5; k++) out[k] = m.last[k];
  out[5] = m.half_blocks;
  out[6] = m.lane_max_blocks;
  out[7] = m.calls;
}

}  // namespace rlnamd
