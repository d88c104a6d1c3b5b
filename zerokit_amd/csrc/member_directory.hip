// The member directory on the device: the kernels over member_directory.h and the MemberDirectoryDev object.
//
// Everything runs on the TREE's stream.  One register() call: a host check, the requests copied in, then
//   k_dir_leaves    leaf[i] = Poseidon(idc, Fr(limit)), a lane per request (one-lane t = 3: register-heavy, VALU-bound)
//   k_dir_rows      OCCUPIED, or the row written and marked a candidate
//   k_dir_insert    candidates take or lower their key's slot
//   k_dir_commit    OK (state, limit, the leaf into the tree's nodes) or KNOWN (the row taken back)
//   MerkleTreeDev::rehash_scattered over all requested indices, one copy back of the statuses, one stream wait.
// resolve(): secrets in, k_dir_commitments (one-lane t = 2), the secrets wiped behind it in stream order, k_dir_find.
// remove(): k_dir_remove (slot -> TOMB, row cleared, the default leaf into the nodes), rehash_scattered.
// slash() is resolve() and then remove() of the distinct indices found, with the one host wait its outputs need anyway.
// The Poseidon kernels are kept apart from the walk kernels: the walks are latency-bound and want occupancy.
// As in nullifier_log.hip, no lane waits for, or reads, what another lane of the same kernel writes: the rows a compare
// reads were written by an earlier kernel, and the only words lanes share are the table entries, touched with agent-scope
// atomics alone (the table is shared by all XCDs, whose L2s are not coherent with each other).
#include "member_directory.h"

#include <string.h>
#include <sys/random.h>

#include <algorithm>
#include <string>
#include <vector>

#include "common.h"
#include "log_scan.h"
#include "merkle.h"
#include "poseidon.h"

namespace rlnamd {

using mdir::View;
using nlog::DevAtomics;
using nlog::Row32;

namespace {

// the longest walk of a workgroup into *longest: one atomic per workgroup.  Every lane of the workgroup calls it.
__device__ __forceinline__ void note_walk(uint32_t walk, uint32_t* __restrict__ longest) {
  __shared__ uint32_t wg_walk;
  if (threadIdx.x == 0) wg_walk = 0;
  __syncthreads();
  if (walk) atomicMax(&wg_walk, walk);
  __syncthreads();
  if (threadIdx.x == 0 && wg_walk) __hip_atomic_fetch_max(longest, wg_walk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the Poseidon kernels (a lane per hash)
__global__ void __launch_bounds__(LOG_LANES) k_dir_leaves(const Row32* __restrict__ idcs, const uint32_t* __restrict__ limits,
                                                          uint32_t n, Fr* __restrict__ leaves, PoseidonView pv) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i >= n) return;
  uint32_t lim[8] = {limits[i], 0, 0, 0, 0, 0, 0, 0};
  const Fr in[2] = {Fr::from_canonical(idcs[i].w), Fr::from_canonical(lim)};
  leaves[i] = poseidon_hash_dev<3>(in, pv);
}
// keys[i] = Poseidon(secret i) where the secret is taken, zero elsewhere (the secret is not read)
__global__ void __launch_bounds__(LOG_LANES) k_dir_commitments(const Row32* __restrict__ secrets, const uint8_t* __restrict__ take,
                                                               uint32_t n, Row32* __restrict__ keys, PoseidonView pv) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i >= n) return;
  Row32 key = mdir::zero_row();
  if (!take || take[i]) {
    const Fr in = Fr::from_canonical(secrets[i].w);
    poseidon_hash_dev<2>(&in, pv).to_canonical(key.w);
  }
  keys[i] = key;
}

// ---- the walk kernels
__global__ void __launch_bounds__(LOG_LANES) k_dir_rows(View D, const uint32_t* __restrict__ indices, const Row32* __restrict__ idcs,
                                                        uint32_t n, uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i >= n) return;
  const uint32_t index = indices[i];
  if (index >= D.capacity) return;   // (not reached: the host check)
  status[i] = mdir::claim_row(D, index, idcs[i]);
}
__global__ void __launch_bounds__(LOG_LANES) k_dir_insert(View D, const uint32_t* __restrict__ indices, uint32_t n,
                                                          const uint8_t* __restrict__ status, uint32_t* __restrict__ longest) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  uint32_t walk = 0;
  if (i < n && status[i] == mdir::PENDING && indices[i] < D.capacity) walk = mdir::insert<DevAtomics>(D, indices[i]);
  note_walk(walk, longest);
}
__global__ void __launch_bounds__(LOG_LANES) k_dir_commit(View D, const uint32_t* __restrict__ indices, const uint32_t* __restrict__ limits,
                                                          const Fr* __restrict__ leaves, uint32_t n, uint8_t* __restrict__ status,
                                                          Fr* __restrict__ leaf_nodes, uint32_t* __restrict__ longest) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  uint32_t walk = 0;
  if (i < n && status[i] == mdir::PENDING && indices[i] < D.capacity) {
    const uint32_t index = indices[i];
    const uint8_t st = mdir::commit<DevAtomics>(D, index, limits[i], &walk);
    if (st == mdir::OK) leaf_nodes[index] = leaves[i];
    status[i] = st;
  }
  note_walk(walk, longest);
}
// take: null for find (every key is looked up); status SKIPPED where take[i] == 0
__global__ void __launch_bounds__(LOG_LANES) k_dir_find(View D, const Row32* __restrict__ keys, const uint8_t* __restrict__ take, uint32_t n,
                                                        uint8_t* __restrict__ status, uint32_t* __restrict__ index,
                                                        uint32_t* __restrict__ limit, uint32_t* __restrict__ longest) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  uint32_t walk = 0;
  if (i < n) {
    mdir::Found f{mdir::SKIPPED, mdir::NO_INDEX, 0};
    if (!take || take[i]) f = mdir::find<DevAtomics>(D, keys[i], &walk);
    status[i] = f.status;
    index[i] = (uint32_t)f.index;   // (NO_INDEX -> 0xFFFFFFFF; the host widens it again)
    limit[i] = f.limit;
  }
  note_walk(walk, longest);
}
__global__ void __launch_bounds__(LOG_LANES) k_dir_remove(View D, const uint32_t* __restrict__ indices, uint32_t n, uint8_t* __restrict__ status,
                                                          Fr* __restrict__ leaf_nodes, Fr default_leaf, uint32_t* __restrict__ longest) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  uint32_t walk = 0;
  if (i < n && indices[i] < D.capacity) {
    const uint32_t index = indices[i];
    const uint8_t st = mdir::remove<DevAtomics>(D, index, &walk);
    if (st == mdir::REMOVED) leaf_nodes[index] = default_leaf;
    status[i] = st;
  }
  note_walk(walk, longest);
}
// the rebuild, behind a fill of the table with EMPTY: a lane per row
__global__ void __launch_bounds__(LOG_LANES) k_dir_rebuild(View D, uint32_t* __restrict__ longest) {
  const uint64_t i = (uint64_t)blockIdx.x * LOG_LANES + threadIdx.x;
  uint32_t walk = 0;
  if (i < D.capacity) walk = mdir::reinsert<DevAtomics>(D, (uint32_t)i);
  note_walk(walk, longest);
}
__global__ void __launch_bounds__(LOG_LANES) k_dir_get(View D, const uint32_t* __restrict__ indices, uint32_t n, uint8_t* __restrict__ live,
                                                       Row32* __restrict__ idcs, uint32_t* __restrict__ limits) {
  const uint32_t i = blockIdx.x * LOG_LANES + threadIdx.x;
  if (i >= n || indices[i] >= D.capacity) return;
  const uint32_t index = indices[i];
  live[i] = D.state[index] == mdir::LIVE;
  idcs[i] = D.idc[index];
  limits[i] = D.limit[index];
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
struct OnDevice {   // the tree's device for the length of a call, the caller's afterwards
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

struct MemberDirectoryDev::Impl {
  MerkleTreeDev& tree;
  hipStream_t stream;
  uint64_t capacity = 0, slots = 0, seed = 0;
  uint64_t live = 0, taken = 0, rebuilds = 0, longest = 0, calls = 0;
  DevBuf<Row32> idc;
  DevBuf<uint32_t> limit, table;
  DevBuf<uint8_t> state;
  // staging of one call of up to stage_n requests
  //   in   (pinned + device): [idcs or keys 32 n][indices 4 n][limits 4 n][take n]
  //   out  (device + pinned): [longest walk: 16 B][indices 4 n][limits 4 n][statuses n]
  //   leaves (device):        the rate commitments of a register call, Montgomery
  //   sec  (pinned + device): the secrets of a resolve or slash, 32 n -- the only staging that ever holds a secret.  Both
  //                           copies are all zero between calls: they are overwritten before the call returns, on every path.
  size_t stage_n = 0;
  uint8_t *in_host = nullptr, *out_host = nullptr, *sec_host = nullptr;
  DevBuf<uint8_t> in_dev, out_dev, sec_dev;
  DevBuf<Fr> leaves;

  explicit Impl(MerkleTreeDev& t) : tree(t), stream(t.stream) {}
  static size_t in_bytes(size_t n) { return pad16(n * 41); }
  static size_t out_bytes(size_t n) { return 16 + pad16(n * 9); }
  View view() const { return View{idc.p, limit.p, state.p, table.p, capacity, slots, seed}; }
  Fr* leaf_nodes() const { return tree.nodes.p + (tree.capacity() - 1); }

  void reserve(size_t n) {
    if (n <= stage_n) return;
    RLN_HIP(hipStreamSynchronize(stream));
    release_staging();
    const size_t m = n < 1024 ? 1024 : n;
    RLN_HIP(hipHostMalloc((void**)&in_host, in_bytes(m), hipHostMallocDefault));
    RLN_HIP(hipHostMalloc((void**)&out_host, out_bytes(m), hipHostMallocDefault));
    RLN_HIP(hipHostMalloc((void**)&sec_host, 32 * m, hipHostMallocDefault));
    memset(sec_host, 0, 32 * m);
    in_dev.alloc(in_bytes(m));
    out_dev.alloc(out_bytes(m));
    sec_dev.alloc(32 * m);
    leaves.alloc(m);
    RLN_HIP(hipMemsetAsync(sec_dev.p, 0, 32 * m, stream));
    RLN_HIP(hipMemsetAsync(out_dev.p, 0, 16, stream));
    stage_n = m;
  }
  // (what held secrets is zero already -- resolve() wipes before it returns -- and is wiped once more before it is freed)
  void release_staging() {
    if (sec_dev.p) {
      (void)hipMemsetAsync(sec_dev.p, 0, 32 * stage_n, stream);
      (void)hipStreamSynchronize(stream);
    }
    if (sec_host) {
      wipe_host(sec_host, 32 * stage_n);
      (void)hipHostFree(sec_host);
    }
    if (in_host) (void)hipHostFree(in_host);
    if (out_host) (void)hipHostFree(out_host);
    in_dev.release();
    out_dev.release();
    sec_dev.release();
    leaves.release();
    in_host = out_host = sec_host = nullptr;
    stage_n = 0;
  }
  ~Impl() {
    (void)hipStreamSynchronize(stream);
    release_staging();
  }

  // the staged pieces of a call of n
  uint8_t* h_keys() const { return in_host; }
  uint32_t* h_indices(size_t n) const { return (uint32_t*)(in_host + 32 * n); }
  uint32_t* h_limits(size_t n) const { return (uint32_t*)(in_host + 36 * n); }
  uint8_t* h_take(size_t n) const { return in_host + 40 * n; }
  Row32* d_keys() const { return (Row32*)in_dev.p; }
  uint32_t* d_indices(size_t n) const { return (uint32_t*)(in_dev.p + 32 * n); }
  uint32_t* d_limits(size_t n) const { return (uint32_t*)(in_dev.p + 36 * n); }
  uint8_t* d_take(size_t n) const { return in_dev.p + 40 * n; }
  uint32_t* d_walk() const { return (uint32_t*)out_dev.p; }
  uint32_t* d_out_index() const { return (uint32_t*)(out_dev.p + 16); }
  uint32_t* d_out_limit(size_t n) const { return (uint32_t*)(out_dev.p + 16 + 4 * n); }
  uint8_t* d_status(size_t n) const { return out_dev.p + 16 + 8 * n; }

  // the outputs of a call back, the walk counter reset behind the copy, one wait
  void fetch(size_t n) {
    RLN_HIP(hipGetLastError());
    RLN_HIP(hipMemcpyAsync(out_host, out_dev.p, out_bytes(n), hipMemcpyDeviceToHost, stream));
    RLN_HIP(hipMemsetAsync(out_dev.p, 0, 16, stream));
    RLN_HIP(hipStreamSynchronize(stream));
    uint32_t walk = 0;
    memcpy(&walk, out_host, 4);
    if (walk > longest) longest = walk;
  }
  void lookup_out(size_t n, uint8_t* status, uint64_t* index, uint32_t* lim) const {
    const uint32_t* o_index = (const uint32_t*)(out_host + 16);
    const uint32_t* o_limit = (const uint32_t*)(out_host + 16 + 4 * n);
    const uint8_t* o_status = out_host + 16 + 8 * n;
    for (size_t i = 0; i < n; i++) {
      status[i] = o_status[i];
      index[i] = o_status[i] == mdir::FOUND ? (uint64_t)o_index[i] : mdir::NO_INDEX;
      lim[i] = o_status[i] == mdir::FOUND ? o_limit[i] : 0;
    }
  }

  void make_room(uint64_t n) {
    if (!mdir::needs_rebuild(taken, n, slots)) return;
    RLN_HIP(hipMemsetAsync(table.p, 0xFF, slots * 4, stream));
    hipLaunchKernelGGL(k_dir_rebuild, dim3(div_up(capacity, LOG_LANES)), dim3(LOG_LANES), 0, stream, view(), d_walk());
    RLN_HIP(hipGetLastError());
    taken = live;
    rebuilds++;
  }
  void rehash(std::vector<uint64_t>& idx) {
    std::sort(idx.begin(), idx.end());
    tree.rehash_scattered(idx.data(), idx.size());
  }
  void resolve(const char* call, size_t n, const uint8_t* secrets_le, const uint8_t* take, uint8_t* status, uint64_t* index,
               uint32_t* lim);
  void remove(size_t n, const uint64_t* indices, uint8_t* status);
};

MemberDirectoryDev::MemberDirectoryDev(MerkleTreeDev& tree, uint64_t capacity, uint64_t seed) {
  const std::string refused = mdir::new_refusal(capacity, (uint64_t)tree.depth);
  if (!refused.empty()) throw Error(refused);
  require_gpu();
  for (int tries = 0; seed == 0 && tries < 8; tries++)
    if (getrandom(&seed, sizeof seed, 0) != (ssize_t)sizeof seed) seed = 0;
  if (seed == 0) throw Error("member directory: getrandom gave no seed");
  OnDevice on(tree.device);
  Impl* m = new Impl(tree);
  try {
    m->capacity = capacity;
    m->slots = nlog::slots_for(capacity);
    m->seed = seed;
    m->idc.alloc(capacity);
    m->limit.alloc(capacity);
    m->state.alloc(capacity);
    m->table.alloc(m->slots);
    RLN_HIP(hipMemsetAsync(m->idc.p, 0, capacity * 32, m->stream));
    RLN_HIP(hipMemsetAsync(m->limit.p, 0, capacity * 4, m->stream));
    RLN_HIP(hipMemsetAsync(m->state.p, 0, capacity, m->stream));
    RLN_HIP(hipMemsetAsync(m->table.p, 0xFF, m->slots * 4, m->stream));
    RLN_HIP(hipStreamSynchronize(m->stream));
  } catch (...) {
    delete m;
    throw;
  }
  d = m;
}

MemberDirectoryDev::~MemberDirectoryDev() {
  if (!d) return;
  int prev = 0;
  const int dev = d->tree.device;
  const bool move = hipGetDevice(&prev) == hipSuccess && prev != dev && hipSetDevice(dev) == hipSuccess;
  delete d;
  if (move) (void)hipSetDevice(prev);
}

uint64_t MemberDirectoryDev::capacity() const { return d->capacity; }

void MemberDirectoryDev::do_register(size_t n, const uint64_t* indices, const uint8_t* idcs_le, const uint32_t* limits, uint8_t* status) {
  Impl& m = *d;
  // the host check: nothing is enqueued and nothing of the directory or the tree changes before it has passed
  const std::string refused = mdir::register_refusal(n, indices, idcs_le, limits, status, m.capacity);
  if (!refused.empty()) throw Error(refused);
  if (n == 0) return;
  OnDevice on(m.tree.device);
  m.reserve(n);
  RLN_HIP(hipStreamSynchronize(m.stream));   // (the pinned block may still be read by the copy of an earlier call that threw)
  std::vector<uint64_t> sorted(indices, indices + n);
  memcpy(m.h_keys(), idcs_le, 32 * n);
  for (size_t i = 0; i < n; i++) m.h_indices(n)[i] = (uint32_t)indices[i];
  memcpy(m.h_limits(n), limits, 4 * n);
  const uint32_t n32 = (uint32_t)n;
  const dim3 grid(div_up(n, LOG_LANES)), block(LOG_LANES);
  m.calls++;
  m.make_room(n);
  RLN_HIP(hipMemcpyAsync(m.in_dev.p, m.in_host, 40 * n, hipMemcpyHostToDevice, m.stream));
  const View D = m.view();
  hipLaunchKernelGGL(k_dir_leaves, grid, block, 0, m.stream, (const Row32*)m.d_keys(), (const uint32_t*)m.d_limits(n), n32, m.leaves.p,
                     poseidon_view(3));
  hipLaunchKernelGGL(k_dir_rows, grid, block, 0, m.stream, D, (const uint32_t*)m.d_indices(n), (const Row32*)m.d_keys(), n32,
                     m.d_status(n));
  hipLaunchKernelGGL(k_dir_insert, grid, block, 0, m.stream, D, (const uint32_t*)m.d_indices(n), n32, (const uint8_t*)m.d_status(n),
                     m.d_walk());
  hipLaunchKernelGGL(k_dir_commit, grid, block, 0, m.stream, D, (const uint32_t*)m.d_indices(n), (const uint32_t*)m.d_limits(n),
                     (const Fr*)m.leaves.p, n32, m.d_status(n), m.leaf_nodes(), m.d_walk());
  RLN_HIP(hipGetLastError());
  m.taken += n;   // until the statuses are back every request counts as a slot taken
  m.rehash(sorted);
  m.fetch(n);
  const uint8_t* o_status = m.out_host + 16 + 8 * n;
  size_t ok = 0;
  for (size_t i = 0; i < n; i++) {
    if (o_status[i] > mdir::KNOWN) throw Error("member directory: internal error, a candidate's key is not in the table");
    ok += o_status[i] == mdir::OK;
  }
  m.taken -= n - ok;
  m.live += ok;
  memcpy(status, o_status, n);
}

void MemberDirectoryDev::find(size_t n, const uint8_t* idcs_le, uint8_t* status, uint64_t* index, uint32_t* limit) {
  Impl& m = *d;
  const std::string refused = mdir::find_refusal(n, idcs_le, status, index, limit);
  if (!refused.empty()) throw Error(refused);
  if (n == 0) return;
  OnDevice on(m.tree.device);
  m.reserve(n);
  RLN_HIP(hipStreamSynchronize(m.stream));
  memcpy(m.h_keys(), idcs_le, 32 * n);
  m.calls++;
  RLN_HIP(hipMemcpyAsync(m.in_dev.p, m.in_host, 32 * n, hipMemcpyHostToDevice, m.stream));
  hipLaunchKernelGGL(k_dir_find, dim3(div_up(n, LOG_LANES)), dim3(LOG_LANES), 0, m.stream, m.view(), (const Row32*)m.d_keys(),
                     (const uint8_t*)nullptr, (uint32_t)n, m.d_status(n), m.d_out_index(), m.d_out_limit(n), m.d_walk());
  m.fetch(n);
  m.lookup_out(n, status, index, limit);
}

void MemberDirectoryDev::Impl::resolve(const char* call, size_t n, const uint8_t* secrets_le, const uint8_t* take, uint8_t* status,
                                       uint64_t* index, uint32_t* lim) {
  Impl& m = *this;
  // the host check: no secret is copied anywhere before it has passed
  const std::string refused = mdir::resolve_refusal(call, n, secrets_le, take, status, index, lim);
  if (!refused.empty()) throw Error(refused);
  if (n == 0) return;
  OnDevice on(m.tree.device);
  m.reserve(n);
  RLN_HIP(hipStreamSynchronize(m.stream));
  struct Wipe {   // success or error: what held secrets is zero again when the call returns
    Impl& m;
    size_t n;
    bool device_done = false;
    ~Wipe() {
      if (!device_done) {
        (void)hipMemsetAsync(m.sec_dev.p, 0, 32 * n, m.stream);
        (void)hipStreamSynchronize(m.stream);
      }
      wipe_host(m.sec_host, 32 * n);
    }
  } wipe{m, n};
  for (size_t i = 0; i < n; i++) {   // a secret that is not taken is not read
    if (!take || take[i]) memcpy(m.sec_host + 32 * i, secrets_le + 32 * i, 32);
    else memset(m.sec_host + 32 * i, 0, 32);
    m.h_take(n)[i] = !take || take[i];
  }
  m.calls++;
  const dim3 grid(div_up(n, LOG_LANES)), block(LOG_LANES);
  RLN_HIP(hipMemcpyAsync(m.sec_dev.p, m.sec_host, 32 * n, hipMemcpyHostToDevice, m.stream));
  RLN_HIP(hipMemcpyAsync(m.d_take(n), m.h_take(n), n, hipMemcpyHostToDevice, m.stream));
  hipLaunchKernelGGL(k_dir_commitments, grid, block, 0, m.stream, (const Row32*)m.sec_dev.p, (const uint8_t*)m.d_take(n), (uint32_t)n,
                     m.d_keys(), poseidon_view(2));
  RLN_HIP(hipMemsetAsync(m.sec_dev.p, 0, 32 * n, m.stream));   // behind the hashes, in stream order
  hipLaunchKernelGGL(k_dir_find, grid, block, 0, m.stream, m.view(), (const Row32*)m.d_keys(), (const uint8_t*)m.d_take(n), (uint32_t)n,
                     m.d_status(n), m.d_out_index(), m.d_out_limit(n), m.d_walk());
  m.fetch(n);
  wipe.device_done = true;
  m.lookup_out(n, status, index, lim);
}

void MemberDirectoryDev::resolve(size_t n, const uint8_t* secrets_le, const uint8_t* take, uint8_t* status, uint64_t* index,
                                 uint32_t* limit) {
  d->resolve("resolve", n, secrets_le, take, status, index, limit);
}

void MemberDirectoryDev::Impl::remove(size_t n, const uint64_t* indices, uint8_t* status) {
  Impl& m = *this;
  if (n == 0) return;
  OnDevice on(m.tree.device);
  m.reserve(n);
  RLN_HIP(hipStreamSynchronize(m.stream));
  std::vector<uint64_t> sorted(indices, indices + n);
  for (size_t i = 0; i < n; i++) m.h_indices(n)[i] = (uint32_t)indices[i];
  m.calls++;
  RLN_HIP(hipMemcpyAsync(m.d_indices(n), m.h_indices(n), 4 * n, hipMemcpyHostToDevice, m.stream));
  hipLaunchKernelGGL(k_dir_remove, dim3(div_up(n, LOG_LANES)), dim3(LOG_LANES), 0, m.stream, m.view(), (const uint32_t*)m.d_indices(n),
                     (uint32_t)n, m.d_status(n), m.leaf_nodes(), m.tree.zero_hashes[m.tree.depth], m.d_walk());
  RLN_HIP(hipGetLastError());
  m.rehash(sorted);   // all requested indices: the path of a VACANT one is rehashed to what it was
  m.fetch(n);
  const uint8_t* o_status = m.out_host + 16 + 8 * n;
  for (size_t i = 0; i < n; i++) {
    if (o_status[i] > mdir::VACANT) throw Error("member directory: internal error, a remove gave no status");
    m.live -= o_status[i] == mdir::REMOVED;
  }
  memcpy(status, o_status, n);
}

void MemberDirectoryDev::remove(size_t n, const uint64_t* indices, uint8_t* status) {
  const std::string refused = mdir::remove_refusal(n, indices, status, d->capacity);
  if (!refused.empty()) throw Error(refused);
  d->remove(n, indices, status);
}

void MemberDirectoryDev::slash(size_t n, const uint8_t* secrets_le, const uint8_t* take, uint8_t* status, uint64_t* index, uint32_t* limit,
                               uint64_t* removed) {
  if (removed) *removed = 0;
  d->resolve("slash", n, secrets_le, take, status, index, limit);
  std::vector<uint64_t> found;
  for (size_t i = 0; i < n; i++)
    if (status[i] == mdir::FOUND) found.push_back(index[i]);
  std::sort(found.begin(), found.end());
  found.erase(std::unique(found.begin(), found.end()), found.end());
  std::vector<uint8_t> st(found.size());
  d->remove(found.size(), found.data(), st.data());
  if (removed) *removed = found.size();
}

void MemberDirectoryDev::get(size_t n, const uint64_t* indices, uint8_t* live, uint8_t* idcs_le, uint32_t* limits) {
  Impl& m = *d;
  const std::string refused = mdir::get_refusal(n, indices, live, idcs_le, limits, m.capacity);
  if (!refused.empty()) throw Error(refused);
  if (n == 0) return;
  OnDevice on(m.tree.device);
  std::vector<uint32_t> idx(n);
  for (size_t i = 0; i < n; i++) idx[i] = (uint32_t)indices[i];
  DevBuf<uint32_t> d_idx(n), d_limits(n);
  DevBuf<uint8_t> d_live(n);
  DevBuf<Row32> d_idcs(n);
  RLN_HIP(hipMemcpyAsync(d_idx.p, idx.data(), 4 * n, hipMemcpyHostToDevice, m.stream));
  hipLaunchKernelGGL(k_dir_get, dim3(div_up(n, LOG_LANES)), dim3(LOG_LANES), 0, m.stream, m.view(), (const uint32_t*)d_idx.p, (uint32_t)n,
                     d_live.p, d_idcs.p, d_limits.p);
  RLN_HIP(hipGetLastError());
  RLN_HIP(hipMemcpyAsync(live, d_live.p, n, hipMemcpyDeviceToHost, m.stream));
  RLN_HIP(hipMemcpyAsync(idcs_le, d_idcs.p, 32 * n, hipMemcpyDeviceToHost, m.stream));
  RLN_HIP(hipMemcpyAsync(limits, d_limits.p, 4 * n, hipMemcpyDeviceToHost, m.stream));
  RLN_HIP(hipStreamSynchronize(m.stream));
}

void MemberDirectoryDev::info(uint64_t out[8]) {
  Impl& m = *d;
  out[0] = m.capacity;
  out[1] = m.live;
  out[2] = m.slots;
  out[3] = m.taken;
  out[4] = m.rebuilds;
  out[5] = m.longest;
  out[6] = m.calls;
  out[7] = 0;
  if (m.stage_n) {
    OnDevice on(m.tree.device);
    const size_t bytes = 32 * m.stage_n;
    std::vector<uint8_t> dev(bytes);
    RLN_HIP(hipMemcpyAsync(dev.data(), m.sec_dev.p, bytes, hipMemcpyDeviceToHost, m.stream));
    RLN_HIP(hipStreamSynchronize(m.stream));
    out[7] = nonzero_words16(dev.data(), bytes) + nonzero_words16(m.sec_host, bytes);
  }
}

}  // namespace rlnamd
