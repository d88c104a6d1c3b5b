// Signals to field elements in batches: x = hash_to_field(signal) = Keccak-256(signal), read little-endian, mod r
// (rln/src/hashers.rs:73-93) for n messages in one call.  Everything the kernel of keccak_batch.hip inlines is here, and
// so is the plan of a call; there is no HIP call in here: a plain C++ compiler builds the same source for the CPU tests
// (tests/host/keccakbatch.cpp).  keccak.h stays what the single-message entry points run, and is the second judge of
// the tests.
//
// Layout.  A call brings `data`, `data_len` and `offsets[n + 1]`: message i is data[offsets[i], offsets[i + 1]).  It has
// blocks(i) = len_i / 136 + 1 blocks of the rate (the pad always adds at least one byte).  The device sees only whole,
// padded blocks of 17 naturally aligned 64-bit words: the host pads while it copies a message into pinned staging -- a
// copy it has to make anyway --
//   zero fill, ^= 0x01 at byte len, ^= 0x80 at the last byte of the last block (one byte, 0x81, when len % 136 == 135)
// so a lane XORs 17 words into its state and permutes, once per block, and knows nothing of lengths.
//
// Lane order.  One lane hashes one message, and a wave runs as long as its longest lane: signals of mixed length in
// arrival order would make every wave pay for its longest message.  Messages are dealt to lanes in order of descending
// block count (a counting sort, stable: equal counts keep index order), so the lanes of a wave have equal or
// neighbouring counts.  order[j] is the message of lane j; a lane's result is row j of the output and the host puts it in
// row order[j] of the caller's while it copies out of pinned memory (a copy it has to make anyway, too).
//
// Host route.  One long message on a lone lane is a serial chain, and a host core runs that chain faster (HOST_PACE
// times faster, measured).  So the calling thread hashes some messages itself while the device works: those that do not
// fit one staging half, and, of the messages of more than `lane_max_blocks` blocks, the longest -- taken one by one,
// longest first, for as long as the host stays ahead of the lanes: a message of b blocks goes to the host while the
// blocks the host has taken, this one included, are at most HOST_PACE * b, that is while the host is done with all of
// them before a lane would be done with this one.  A lone long message, or a few among thousands of short ones, go to
// the host; of 65 536 equally long ones the host takes HOST_PACE and the lanes the rest.  They are the first `n_host`
// entries of `order`.
//
// Chunks.  Staging is two halves of `half_blocks` blocks.  The rest of `order` is cut at message boundaries into chunks
// of at most `half_blocks` blocks; chunk k is packed into half k & 1 while the device works on chunk k - 1.  A packed
// chunk is  [first_block: count + 1 uint32, a prefix sum][pad to 8 bytes][blocks]  in one piece, so one copy brings it
// to the device: lane j of the chunk hashes blocks [first_block[j], first_block[j + 1]).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "field.h"

namespace rlnamd {
namespace kbatch {

constexpr size_t RATE = 136, RATE_WORDS = 17;
constexpr uint64_t MAX_MESSAGES = 0xFFFFFFFFull;           // order[] and first_block[] are 32-bit
constexpr size_t MAX_STAGE_BYTES = (size_t)1 << 30;        // both halves together
constexpr size_t DEFAULT_STAGE_BYTES = (size_t)8 << 20;    // two halves of 4 MiB: 30 840 blocks each
// The block count at which a lone lane's chain takes as long as the fixed cost of a device call, rounded to a power of
// two (tools/hash_to_field_throughput.py, profiles/hash_to_field_batch.md: a call of 1 024 32-byte messages takes
// 0.061 ms, a lone lane 14.7 us per block: 4.2 blocks).  Shorter messages never leave the lanes.
constexpr size_t DEFAULT_LANE_MAX_BLOCKS = 4;
// A lone lane's time per block over a host core's (the same table: 14.7 us against 0.31 us, 47.6, taken as 50)
constexpr uint64_t HOST_PACE = 50;

struct RoundConstants {
  static constexpr uint64_t RC[24] = {
      0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL,
      0x000000000000808bULL, 0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL,
      0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
      0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL,
      0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
      0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
};

RLN_HD uint64_t rol64(uint64_t x, int n) { return (x << n) | (x >> (64 - n)); }

// Keccak-f[1600].  Every index into the state is a literal, so on the device the 25 words are 50 registers and nothing
// is addressed through scratch memory; only the loop over the rounds is rolled, and its index reads the constant table.
RLN_HD void permute(uint64_t (&a)[25]) {
  for (int round = 0; round < 24; round++) {
    // theta
    const uint64_t c0 = a[0] ^ a[5] ^ a[10] ^ a[15] ^ a[20], c1 = a[1] ^ a[6] ^ a[11] ^ a[16] ^ a[21],
                   c2 = a[2] ^ a[7] ^ a[12] ^ a[17] ^ a[22], c3 = a[3] ^ a[8] ^ a[13] ^ a[18] ^ a[23],
                   c4 = a[4] ^ a[9] ^ a[14] ^ a[19] ^ a[24];
    const uint64_t d0 = c4 ^ rol64(c1, 1), d1 = c0 ^ rol64(c2, 1), d2 = c1 ^ rol64(c3, 1), d3 = c2 ^ rol64(c4, 1),
                   d4 = c3 ^ rol64(c0, 1);
#define RLN_KB_THETA(o) a[o] ^= d0; a[o + 1] ^= d1; a[o + 2] ^= d2; a[o + 3] ^= d3; a[o + 4] ^= d4;
    RLN_KB_THETA(0) RLN_KB_THETA(5) RLN_KB_THETA(10) RLN_KB_THETA(15) RLN_KB_THETA(20)
#undef RLN_KB_THETA
    // rho and pi: the one cycle of 24 lanes, written out
    uint64_t t = a[1], b;
#define RLN_KB_RHOPI(j, r) b = a[j]; a[j] = rol64(t, r); t = b;
    RLN_KB_RHOPI(10, 1) RLN_KB_RHOPI(7, 3) RLN_KB_RHOPI(11, 6) RLN_KB_RHOPI(17, 10) RLN_KB_RHOPI(18, 15)
    RLN_KB_RHOPI(3, 21) RLN_KB_RHOPI(5, 28) RLN_KB_RHOPI(16, 36) RLN_KB_RHOPI(8, 45) RLN_KB_RHOPI(21, 55)
    RLN_KB_RHOPI(24, 2) RLN_KB_RHOPI(4, 14) RLN_KB_RHOPI(15, 27) RLN_KB_RHOPI(23, 41) RLN_KB_RHOPI(19, 56)
    RLN_KB_RHOPI(13, 8) RLN_KB_RHOPI(12, 25) RLN_KB_RHOPI(2, 43) RLN_KB_RHOPI(20, 62) RLN_KB_RHOPI(14, 18)
    RLN_KB_RHOPI(22, 39) RLN_KB_RHOPI(9, 61) RLN_KB_RHOPI(6, 20) RLN_KB_RHOPI(1, 44)
#undef RLN_KB_RHOPI
    // chi
#define RLN_KB_CHI(o)                                                                       \
  {                                                                                         \
    const uint64_t e0 = a[o], e1 = a[o + 1], e2 = a[o + 2], e3 = a[o + 3], e4 = a[o + 4];   \
    a[o] = e0 ^ (~e1 & e2);                                                                 \
    a[o + 1] = e1 ^ (~e2 & e3);                                                             \
    a[o + 2] = e2 ^ (~e3 & e4);                                                             \
    a[o + 3] = e3 ^ (~e4 & e0);                                                             \
    a[o + 4] = e4 ^ (~e0 & e1);                                                             \
  }
    RLN_KB_CHI(0) RLN_KB_CHI(5) RLN_KB_CHI(10) RLN_KB_CHI(15) RLN_KB_CHI(20)
#undef RLN_KB_CHI
    // iota
    a[0] ^= RoundConstants::RC[round];
  }
}

// one padded block into the state, and the permutation behind it
RLN_HD void absorb(uint64_t (&a)[25], const uint64_t* block) {
#pragma unroll
  for (int k = 0; k < (int)RATE_WORDS; k++) a[k] ^= block[k];
  permute(a);
}

// The first 32 bytes of the state as a little-endian integer, mod r: r is subtracted while the value is at least r, at
// most 5 times (2^256 < 6 r).  out: 8 canonical little-endian words.  Returns the quotient.
RLN_HD int squeeze_reduce(const uint64_t (&a)[25], uint32_t (&out)[8]) {
  out[0] = (uint32_t)a[0]; out[1] = (uint32_t)(a[0] >> 32);
  out[2] = (uint32_t)a[1]; out[3] = (uint32_t)(a[1] >> 32);
  out[4] = (uint32_t)a[2]; out[5] = (uint32_t)(a[2] >> 32);
  out[6] = (uint32_t)a[3]; out[7] = (uint32_t)(a[3] >> 32);
  int q = 0;
  while (limbs_geq(out, FrParams::MOD)) {
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint64_t s = (uint64_t)out[i] - FrParams::MOD[i] - borrow;
      out[i] = (uint32_t)s;
      borrow = (uint32_t)(s >> 63);
    }
    q++;
  }
  return q;
}

// what a lane does, on whole padded blocks
RLN_HD int hash_blocks(const uint64_t* blocks, uint32_t first, uint32_t end, uint32_t (&out)[8]) {
  uint64_t a[25];
#pragma unroll
  for (int k = 0; k < 25; k++) a[k] = 0;
  for (uint32_t b = first; b < end; b++) absorb(a, blocks + RATE_WORDS * (size_t)b);
  return squeeze_reduce(a, out);
}

// ----------------------------------------------------------------------------------------------- the host's side

inline uint64_t blocks_of(uint64_t len) { return len / RATE + 1; }

// message -> blocks_of(len) padded blocks at dst
inline void pack_message(const uint8_t* msg, size_t len, uint8_t* dst) {
  const size_t padded = (size_t)blocks_of(len) * RATE;
  if (len) memcpy(dst, msg, len);
  memset(dst + len, 0, padded - len);
  dst[len] ^= 0x01;
  dst[padded - 1] ^= 0x80;
}

// one message on the calling thread, by the text the lanes run: padded block by block through a 136-byte buffer.
// Returns the quotient of the reduction.
inline int hash_message(const uint8_t* msg, size_t len, uint8_t out_le[32]) {
  uint64_t a[25];
  memset(a, 0, sizeof a);
  uint64_t w[RATE_WORDS];
  size_t off = 0;
  for (; len - off >= RATE; off += RATE) {
    memcpy(w, msg + off, RATE);
    absorb(a, w);
  }
  uint8_t last[RATE];
  pack_message(len - off ? msg + off : nullptr, len - off, last);
  memcpy(w, last, RATE);
  absorb(a, w);
  uint32_t v[8];
  const int q = squeeze_reduce(a, v);
  memcpy(out_le, v, 32);
  return q;
}

struct Chunk {
  size_t first = 0, count = 0;   // order[first, first + count)
  uint64_t blocks = 0;
};

struct Plan {
  size_t n = 0;
  std::vector<uint32_t> order;     // a permutation of 0 .. n - 1: the host's messages, then the lanes' in lane order
  std::vector<uint64_t> nblocks;   // by message
  size_t n_host = 0;               // order[0, n_host) are hashed on the calling thread
  std::vector<Chunk> chunks;       // order[n_host, n), in order
  uint64_t device_blocks = 0, longest_lane = 0;
};

inline size_t header_bytes(size_t count) { return (4 * (count + 1) + 7) & ~(size_t)7; }
inline size_t chunk_bytes(const Chunk& c) { return header_bytes(c.count) + (size_t)c.blocks * RATE; }
// room for any chunk of at most half_blocks blocks (and so at most half_blocks messages)
inline size_t half_bytes(size_t half_blocks) { return header_bytes(half_blocks) + half_blocks * RATE; }

// what a call brings, checked: null, or the text of the refusal (n > 0)
inline const char* check_call(const uint8_t* data, uint64_t data_len, const uint64_t* offsets, uint64_t n) {
  if (!offsets) return "hash_to_field: null offsets for n > 0 messages";
  if (n > MAX_MESSAGES) return "hash_to_field: sizes overflow, a call takes at most 2^32 - 1 messages";
  for (uint64_t i = 0; i < n; i++)
    if (offsets[i + 1] < offsets[i]) return "hash_to_field: offsets decrease";
  if (offsets[n] > data_len) return "hash_to_field: the last offset lies beyond data_len";
  if (!data && offsets[n] > offsets[0]) return "hash_to_field: null data for messages that are not empty";
  return nullptr;
}

// The plan of a call.  Returns null, or the text of the refusal; a refused call has written nothing but *p.
// sorted = false keeps the lanes in index order (the measurement's other row).
inline const char* plan_call(const uint8_t* data, uint64_t data_len, const uint64_t* offsets, uint64_t n,
                             size_t half_blocks, size_t lane_max_blocks, bool sorted, Plan* p) {
  *p = Plan();
  if (n == 0) return nullptr;
  if (const char* refused = check_call(data, data_len, offsets, n)) return refused;
  if (half_blocks == 0 || lane_max_blocks == 0) return "hash_to_field: internal error, a hasher without staging";

  p->n = (size_t)n;
  p->nblocks.resize(p->n);
  p->order.resize(p->n);
  // what fits no half is the host's whatever it costs (the longest first); everything else by a counting sort,
  // descending and stable: bucket 0 is the host's, a message of b blocks goes to bucket longest - b + 1
  uint64_t longest = 0;
  for (size_t i = 0; i < p->n; i++) {
    p->nblocks[i] = blocks_of(offsets[i + 1] - offsets[i]);
    if (p->nblocks[i] <= half_blocks) longest = std::max(longest, p->nblocks[i]);
  }
  auto bucket = [&](uint64_t b) -> size_t { return b > half_blocks ? 0 : (size_t)(longest - b) + 1; };
  std::vector<size_t> start((size_t)longest + 3, 0);   // at most half_blocks + 3 entries
  for (size_t i = 0; i < p->n; i++) start[bucket(p->nblocks[i]) + 1]++;
  p->n_host = start[1];
  for (size_t k = 1; k < start.size(); k++) start[k] += start[k - 1];
  for (size_t i = 0; i < p->n; i++) p->order[start[bucket(p->nblocks[i])]++] = (uint32_t)i;
  std::stable_sort(p->order.begin(), p->order.begin() + p->n_host,
                   [&](uint32_t x, uint32_t y) { return p->nblocks[x] > p->nblocks[y]; });
  // then the longest above lane_max_blocks, for as long as the host keeps pace (see above)
  uint64_t taken = 0;
  for (size_t j = 0; j < p->n_host; j++) taken += p->nblocks[p->order[j]];
  while (p->n_host < p->n) {
    const uint64_t b = p->nblocks[p->order[p->n_host]];
    if (b <= lane_max_blocks || taken + b > HOST_PACE * b) break;
    taken += b;
    p->n_host++;
  }
  if (!sorted) {   // the lanes in index order
    std::vector<uint8_t> on_host(p->n, 0);
    for (size_t j = 0; j < p->n_host; j++) on_host[p->order[j]] = 1;
    size_t at = p->n_host;
    for (size_t i = 0; i < p->n; i++)
      if (!on_host[i]) p->order[at++] = (uint32_t)i;
  }

  Chunk c;
  c.first = p->n_host;
  for (size_t j = p->n_host; j < p->n; j++) {
    const uint64_t b = p->nblocks[p->order[j]];
    if (c.blocks + b > half_blocks) {
      p->chunks.push_back(c);
      c = Chunk();
      c.first = j;
    }
    c.count++;
    c.blocks += b;
    p->device_blocks += b;
    p->longest_lane = std::max(p->longest_lane, b);
  }
  if (c.count) p->chunks.push_back(c);
  return nullptr;
}

// chunk c of the plan into a staging half of half_bytes(half_blocks) bytes; returns chunk_bytes(c)
inline size_t pack_chunk(const Plan& p, const Chunk& c, const uint8_t* data, const uint64_t* offsets, uint8_t* half) {
  uint32_t* first_block = (uint32_t*)half;
  uint8_t* blocks = half + header_bytes(c.count);
  memset(half + 4 * (c.count + 1), 0, header_bytes(c.count) - 4 * (c.count + 1));
  uint32_t at = 0;
  for (size_t j = 0; j < c.count; j++) {
    const uint32_t i = p.order[c.first + j];
    first_block[j] = at;
    const size_t len = (size_t)(offsets[i + 1] - offsets[i]);
    pack_message(len ? data + offsets[i] : nullptr, len, blocks + (size_t)at * RATE);
    at += (uint32_t)p.nblocks[i];
  }
  first_block[c.count] = at;
  return chunk_bytes(c);
}

}  // namespace kbatch

// The hasher as a device-resident object (keccak_batch.hip): a non-blocking stream of its own, two pinned staging
// halves and their device twins, sized when it is made.  It lives on the device that is current when it is made.  Not
// thread-safe: the C ABI's handle (capi.cpp) holds a mutex.  Signals are public bytes: nothing is wiped.
// Every method throws rlnamd::Error.
struct HasherDev {
  struct Impl;
  Impl* d = nullptr;
  HasherDev(size_t stage_bytes, size_t lane_max_blocks);   // 0: the defaults above
  ~HasherDev();
  HasherDev(const HasherDev&) = delete;
  HasherDev& operator=(const HasherDev&) = delete;
  // out_le: n * 32 bytes, row i = hash_to_field(data[offsets[i], offsets[i + 1])), canonical little-endian.
  // Refused before anything is enqueued: see kbatch::plan_call, and a null out_le with n > 0.
  void hash_to_field(const uint8_t* data, size_t data_len, const uint64_t* offsets, size_t n, uint8_t* out_le);
  // the last call: messages on the device, on the host, chunks, blocks on the device, longest lane in blocks;
  // then staging blocks per half, lane_max_blocks, calls so far
  void info(uint64_t out[8]);

  // ---- for the relay step (relay.hip): the same plan, packing and lanes, but the rows stay on the device, row i of
  // rows_dev (n x 32 bytes of device memory) the element of message i: a lane writes row order[j], and the rows of the
  // messages the plan gives to the host are hashed on the calling thread and copied into place.  Everything is
  // enqueued on relay_stream() and NOT waited for: the caller waits for that stream before the hasher is used again
  // (the pinned halves are packed anew by the next call).  Returns the number of messages hashed on the host.
  // Refuses what hash_to_field refuses, before anything is enqueued.
  size_t relay_hash(const uint8_t* data, size_t data_len, const uint64_t* offsets, size_t n, uint8_t* rows_dev);
  void* relay_stream();   // a hipStream_t
  int device() const;
};

}  // namespace rlnamd
