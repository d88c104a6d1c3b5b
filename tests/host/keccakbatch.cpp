// CPU build of zerokit_amd/csrc/keccak_batch.h for tests/test_keccak_batch_host.py (a shared object through ctypes) and
// for tests/host/keccakbatch_main.cpp (the stand-alone sanitizer program, which includes this file): the permutation and
// the reduce the lanes run, the plan of a call, the packing, and kb_hash_call -- a whole call the way HasherDev makes
// it, with a loop over the lanes where the kernel is.  keccak.h is the second judge.
#include <stdio.h>

#include <string>
#include <vector>

#include "keccak.h"
#include "keccak_batch.h"

using namespace rlnamd;

namespace {
void put_error(const char* text, char* err, size_t cap) {
  if (err && cap) snprintf(err, cap, "%s", text);
}
}  // namespace

extern "C" {

int kb_hash_message(const uint8_t* msg, size_t len, uint8_t out_le[32]) { return kbatch::hash_message(msg, len, out_le); }
void kb_keccak_h(const uint8_t* msg, size_t len, uint8_t out_le[32]) { hash_to_field_le(msg, len, out_le); }
// n calls of a single-message entry point (rlnamd_hash_to_field_le, handed in by address) in a loop of C: the one host
// thread tools/hash_to_field_throughput.py measures against
typedef int (*kb_single_fn)(const uint8_t*, size_t, uint8_t*);
int kb_loop_single(kb_single_fn f, const uint8_t* data, const uint64_t* offsets, size_t n, uint8_t* out_le) {
  for (size_t i = 0; i < n; i++)
    if (int rc = f(data + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), out_le + 32 * i)) return rc;
  return 0;
}
size_t kb_header_bytes(size_t count) { return kbatch::header_bytes(count); }
size_t kb_half_bytes(size_t half_blocks) { return kbatch::half_bytes(half_blocks); }

// order: n, nblocks: n, meta: n_host, chunks, device_blocks, longest_lane; chunks: (first, count, blocks) * up to
// max_chunks.  Returns 0, or 1 with the refusal's text in err and nothing else written.
int kb_plan(const uint8_t* data, uint64_t data_len, const uint64_t* offsets, uint64_t n, size_t half_blocks,
            size_t lane_max_blocks, int sorted, uint32_t* order, uint64_t* nblocks, uint64_t meta[4], uint64_t* chunks,
            size_t max_chunks, char* err, size_t err_cap) {
  kbatch::Plan p;
  if (const char* refused = kbatch::plan_call(data, data_len, offsets, n, half_blocks, lane_max_blocks, sorted != 0, &p)) {
    put_error(refused, err, err_cap);
    return 1;
  }
  for (size_t i = 0; i < p.n; i++) order[i] = p.order[i], nblocks[i] = p.nblocks[i];
  meta[0] = p.n_host;
  meta[1] = p.chunks.size();
  meta[2] = p.device_blocks;
  meta[3] = p.longest_lane;
  for (size_t k = 0; k < p.chunks.size() && k < max_chunks; k++) {
    chunks[3 * k] = p.chunks[k].first;
    chunks[3 * k + 1] = p.chunks[k].count;
    chunks[3 * k + 2] = p.chunks[k].blocks;
  }
  return 0;
}

// chunk `k` of the call's plan as it is staged; returns its size, 0 when there is no such chunk or `cap` is too small
size_t kb_pack_chunk(const uint8_t* data, uint64_t data_len, const uint64_t* offsets, uint64_t n, size_t half_blocks,
                     size_t lane_max_blocks, size_t k, uint8_t* out, size_t cap) {
  kbatch::Plan p;
  if (kbatch::plan_call(data, data_len, offsets, n, half_blocks, lane_max_blocks, true, &p) || k >= p.chunks.size()) return 0;
  if (kbatch::chunk_bytes(p.chunks[k]) > cap) return 0;
  std::vector<uint64_t> half(kbatch::half_bytes(half_blocks) / 8 + 1);   // aligned as the pinned half is
  const size_t bytes = kbatch::pack_chunk(p, p.chunks[k], data, offsets, (uint8_t*)half.data());
  memcpy(out, half.data(), bytes);
  return bytes;
}

// a whole call: plan, every chunk packed into one of two halves of exactly half_bytes(half_blocks), every lane's
// blocks hashed out of the half, rows put where their messages are; the host's messages by hash_message
int kb_hash_call(const uint8_t* data, uint64_t data_len, const uint64_t* offsets, uint64_t n, size_t half_blocks,
                 size_t lane_max_blocks, int sorted, uint8_t* out_le, char* err, size_t err_cap) {
  kbatch::Plan p;
  if (const char* refused = kbatch::plan_call(data, data_len, offsets, n, half_blocks, lane_max_blocks, sorted != 0, &p)) {
    put_error(refused, err, err_cap);
    return 1;
  }
  // (operator new gives 16-byte alignment; the size is exact, so that a write past a half is seen by ASan)
  std::vector<uint8_t> half[2] = {std::vector<uint8_t>(kbatch::half_bytes(half_blocks)),
                                  std::vector<uint8_t>(kbatch::half_bytes(half_blocks))};
  for (size_t k = 0; k < p.chunks.size(); k++) {
    const kbatch::Chunk& c = p.chunks[k];
    uint8_t* h = half[k & 1].data();
    if (kbatch::pack_chunk(p, c, data, offsets, h) > half[k & 1].size()) return 2;
    const uint32_t* first_block = (const uint32_t*)h;
    const uint64_t* blocks = (const uint64_t*)(h + kbatch::header_bytes(c.count));
    for (size_t j = 0; j < c.count; j++) {
      uint32_t v[8];
      kbatch::hash_blocks(blocks, first_block[j], first_block[j + 1], v);
      memcpy(out_le + 32 * (size_t)p.order[c.first + j], v, 32);
    }
  }
  for (size_t j = 0; j < p.n_host; j++) {
    const uint32_t i = p.order[j];
    kbatch::hash_message(data + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), out_le + 32 * (size_t)i);
  }
  return 0;
}

// The cases of the sanitizer program, judged by keccak.h message by message.  Returns 0 and a digest (FNV-1a) of every
// output row, or the number of the case that went wrong.
int kb_selfcheck(uint64_t* digest) {
  uint64_t fnv = 0xcbf29ce484222325ull, rng = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    return rng >> 33;
  };
  char err[128];
  // lens: the messages; lead: bytes in front of the first (offsets[0] > 0); tail: bytes behind the last
  auto run = [&](const std::vector<size_t>& lens, size_t lead, size_t tail, size_t half_blocks, size_t lane_max, int sorted) {
    std::vector<uint64_t> offsets(1, lead);
    for (size_t l : lens) offsets.push_back(offsets.back() + l);
    std::vector<uint8_t> data((size_t)offsets.back() + tail);   // exact: reads past a message's end are seen
    for (auto& b : data) b = (uint8_t)rnd();
    std::vector<uint8_t> out(32 * lens.size() + 1, 0xAA);
    if (kb_hash_call(data.empty() ? nullptr : data.data(), data.size(), offsets.data(), lens.size(), half_blocks, lane_max,
                     sorted, out.data(), err, sizeof err))
      return false;
    if (out.back() != 0xAA) return false;
    for (size_t i = 0; i < lens.size(); i++) {
      uint8_t want[32];
      static const uint8_t none = 0;   // (keccak.h hands its pointer to memcpy, which takes no null one)
      hash_to_field_le(lens[i] ? data.data() + offsets[i] : &none, lens[i], want);
      if (memcmp(want, &out[32 * i], 32) != 0) return false;
    }
    for (size_t i = 0; i + 1 < out.size(); i++) fnv = (fnv ^ out[i]) * 0x100000001b3ull;
    return true;
  };
  // 1: ragged calls, one chunk and many, sorted and not, some messages on the host
  for (int rep = 0; rep < 6; rep++) {
    std::vector<size_t> lens(200 + 37 * rep);
    for (auto& l : lens) l = rnd() % 700;
    if (!run(lens, 0, 0, rep % 2 ? 16 : 4096, rep % 3 ? 4 : 1024, rep < 4)) return 1;
  }
  // 2: a staging half filled exactly: 16 blocks of 16 one-block messages, of 4 + 4 + 8 blocks, of one 16-block message
  if (!run(std::vector<size_t>(16, 135), 0, 0, 16, 1024, 1)) return 2;
  if (!run({4 * 136 - 1, 3 * 136, 8 * 136 - 1, 7 * 136 + 5, 0, 16 * 136 - 1, 15 * 136, 16 * 136}, 0, 0, 16, 1024, 1)) return 2;
  // 3: zero-length messages at both ends, alone, and with nothing else in `data`
  if (!run({0, 0, 5, 136, 271, 272, 0, 0}, 0, 0, 16, 1024, 1)) return 3;
  if (!run({0}, 0, 0, 1, 1, 1)) return 3;
  if (!run({0, 0, 0}, 0, 0, 2, 1, 0)) return 3;
  // 4: offsets[0] > 0 and bytes behind the last message
  if (!run({10, 0, 300, 135}, 7, 9, 16, 2, 1)) return 4;
  // 5: the refusals, each with its own text and the output untouched
  {
    const uint8_t data[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    uint8_t out[64];
    memset(out, 0x55, sizeof out);
    const uint64_t good[3] = {0, 3, 8}, down[3] = {0, 5, 3}, beyond[3] = {0, 3, 9};
    std::vector<std::string> texts;
    auto refused = [&](const uint8_t* d, uint64_t dl, const uint64_t* o, uint64_t n) {
      err[0] = 0;
      if (kb_hash_call(d, dl, o, n, 16, 4, 1, out, err, sizeof err) != 1 || !err[0]) return false;
      texts.push_back(err);
      return true;
    };
    if (!refused(data, 8, nullptr, 2) || !refused(nullptr, 8, good, 2) || !refused(data, 8, down, 2) ||
        !refused(data, 8, beyond, 2) || !refused(data, 8, good, (uint64_t)1 << 32))
      return 5;
    for (size_t a = 0; a < texts.size(); a++)
      for (size_t b = a + 1; b < texts.size(); b++)
        if (texts[a] == texts[b]) return 5;
    for (uint8_t b : out)
      if (b != 0x55) return 5;
    if (kb_hash_call(nullptr, 0, nullptr, 0, 16, 4, 1, nullptr, err, sizeof err) != 0) return 5;   // n = 0 is no refusal
  }
  *digest = fnv;
  return 0;
}

}  // extern "C"
