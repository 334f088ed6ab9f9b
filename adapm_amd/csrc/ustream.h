// Uniform key stream that reproduces numpy's
//   Generator(PCG64).integers(lo, hi, size=n, dtype=int64)
// bit for bit, for ranges whose bounded draw is numpy's 32-bit Lemire
// filter (0 < hi-lo-1 < 0xFFFFFFFF). Shared by the device kernels
// (kernels_hip.hip) and their CPU twin (kernels_cpu.cpp).
//
// Word stream. PCG64 steps state = state*MULT + inc (mod 2^128) and outputs
// rotr64(hi ^ lo, hi >> 58) of the NEW state; each 64-bit output yields two
// uint32 words, low half first, the high half being buffered in
// (has_uint32, uinteger). With output j = the output of the state advanced
// j steps, "virtual word" v is half (v & 1) of output (v >> 1). A stream
// whose buffer is full starts at v = 1 (the buffered high half of output
// 0), one whose buffer is empty at v = 2. Word w of a draw is v = v0 + w.
//
// Bounded draw. excl = hi - lo, thr = (2^32 - excl) % excl. A word u gives
// m = u * excl; it is accepted iff (uint32)m >= thr and then yields
// lo + (m >> 32). Acceptance depends on the word alone, so the result is the
// first n accepted words in stream order: generate, flag, compact.
#pragma once
#include <cstdint>

#if defined(__HIP__)
#define ADAPM_HD __host__ __device__
#else
#define ADAPM_HD
#endif

namespace adapm {

typedef unsigned __int128 u128;

// state words: [0] state hi, [1] state lo, [2] inc hi, [3] inc lo,
// [4] has_uint32, [5] uinteger; then the jump table of this `inc`: for
// k < 64 the LCG step composed 2^k times, as (mult hi, mult lo, plus hi,
// plus lo). A jump by delta applies one entry per set bit of delta.
constexpr int USTREAM_GEN_WORDS = 6;
constexpr int USTREAM_STATE_WORDS = USTREAM_GEN_WORDS + 64 * 4;
constexpr int USTREAM_CHUNK = 16;    // words per chunk (one thread)
constexpr int USTREAM_BLOCK = 256;   // chunks per block
constexpr int64_t USTREAM_REJECTED = INT64_MIN;  // never a key: lo > INT64_MIN

struct UStreamRange {
  int64_t lo;
  uint32_t excl;  // hi - lo, in (1, 0xFFFFFFFF]
  uint32_t thr;   // (2^32 - excl) % excl
};

inline int64_t ustream_chunks(int64_t words) { return (words + USTREAM_CHUNK - 1) / USTREAM_CHUNK; }
inline int64_t ustream_blocks(int64_t words) {
  return (ustream_chunks(words) + USTREAM_BLOCK - 1) / USTREAM_BLOCK;
}
// scratch layout: [block counts x blocks | keys x blocks*BLOCK*CHUNK], int64
constexpr int USTREAM_TMP_COUNTS = 0;
inline int64_t ustream_tmp_words(int64_t words) {
  int64_t nb = ustream_blocks(words);
  return USTREAM_TMP_COUNTS + nb + nb * USTREAM_BLOCK * USTREAM_CHUNK;
}

ADAPM_HD inline u128 ustream_mult() {
  return ((u128)0x2360ED051FC65DA4ULL << 64) | (u128)0x4385DF649FCCF645ULL;
}

ADAPM_HD inline uint64_t ustream_output(u128 s) {
  uint64_t hi = (uint64_t)(s >> 64), lo = (uint64_t)s;
  uint64_t x = hi ^ lo;
  unsigned rot = (unsigned)(hi >> 58);
  return (x >> rot) | (x << ((64 - rot) & 63));
}

// fills the jump table behind the generator words from st's inc (host side,
// once per imported state)
inline void ustream_build_table(uint64_t* st) {
  u128 cur_mult = ustream_mult(), cur_plus = ((u128)st[2] << 64) | st[3];
  uint64_t* t = st + USTREAM_GEN_WORDS;
  for (int k = 0; k < 64; ++k, t += 4) {
    t[0] = (uint64_t)(cur_mult >> 64), t[1] = (uint64_t)cur_mult;
    t[2] = (uint64_t)(cur_plus >> 64), t[3] = (uint64_t)cur_plus;
    cur_plus = (cur_mult + 1) * cur_plus;
    cur_mult *= cur_mult;
  }
}

// st's state advanced by `delta` steps: the LCG jump-ahead, one 128-bit
// multiply-add per set bit of delta
ADAPM_HD inline u128 ustream_advance(const uint64_t* st, uint64_t delta) {
  u128 s = ((u128)st[0] << 64) | st[1];
  const uint64_t* t = st + USTREAM_GEN_WORDS;
  for (; delta > 0; delta >>= 1, t += 4)
    if (delta & 1) s = s * (((u128)t[0] << 64) | t[1]) + (((u128)t[2] << 64) | t[3]);
  return s;
}

// Sequential reader of virtual words, positioned by one jump-ahead.
struct UStreamCursor {
  u128 s, inc;
  uint64_t j, out;
  uint64_t has0, uint0;

  ADAPM_HD UStreamCursor(const uint64_t* st, uint64_t j0) {
    inc = ((u128)st[2] << 64) | st[3];
    s = ustream_advance(st, j0);
    j = j0;
    out = ustream_output(s);
    has0 = st[4];
    uint0 = st[5];
  }
  ADAPM_HD uint32_t word(uint64_t v) {
    uint64_t jj = v >> 1;
    while (j < jj) {
      s = s * ustream_mult() + inc;
      out = ustream_output(s);
      ++j;
    }
    if (v == 1 && has0) return (uint32_t)uint0;  // the buffered half, as stored
    return (v & 1) ? (uint32_t)(out >> 32) : (uint32_t)out;
  }
};

ADAPM_HD inline uint64_t ustream_v0(const uint64_t* st) { return st[4] ? 1 : 2; }

ADAPM_HD inline int64_t ustream_key(const UStreamRange& r, uint32_t u) {
  uint64_t m = (uint64_t)u * r.excl;
  return ((uint32_t)m >= r.thr) ? r.lo + (int64_t)(m >> 32) : USTREAM_REJECTED;
}

// Chunk c: words [c*CHUNK, (c+1)*CHUNK) of the draw, cut at `words`. Writes
// key-or-REJECTED of word i of the chunk to chunk_keys[i*stride] and returns
// how many were accepted.
ADAPM_HD inline int ustream_gen_chunk(const uint64_t* st, const UStreamRange& r, int64_t words,
                                      int64_t c, int64_t* chunk_keys, int64_t stride) {
  const uint64_t v0 = ustream_v0(st);
  const int64_t w0 = c * USTREAM_CHUNK;
  UStreamCursor cur(st, (v0 + (uint64_t)w0) >> 1);
  int cnt = 0;
  for (int i = 0; i < USTREAM_CHUNK; ++i) {
    int64_t w = w0 + i;
    int64_t k = USTREAM_REJECTED;
    if (w < words) k = ustream_key(r, cur.word(v0 + (uint64_t)w));
    chunk_keys[i * stride] = k;
    cnt += (k != USTREAM_REJECTED);
  }
  return cnt;
}

// Last step of a draw, run by one thread. `total` keys were accepted among
// the first `words` words, and the compaction writes out[0 .. min(total, n));
// `consumed` is the word count up to and including the n-th accepted one
// when total >= n. Otherwise the stream is continued word by word into
// out[total .. n) until n keys exist (slow; the caller sizes `words` so that
// it practically never happens). Then the state is left where numpy leaves
// it.
ADAPM_HD inline void ustream_finish(uint64_t* st, const UStreamRange& r, int64_t n, int64_t words,
                                    int64_t total, int64_t consumed, int64_t* out) {
  const uint64_t v0 = ustream_v0(st);
  if (total < n) {
    UStreamCursor cur(st, (v0 + (uint64_t)words) >> 1);
    int64_t w = words;
    while (total < n) {
      int64_t k = ustream_key(r, cur.word(v0 + (uint64_t)w));
      ++w;
      if (k != USTREAM_REJECTED) out[total++] = k;
    }
    consumed = w;
  }
  const uint64_t v_end = v0 + (uint64_t)consumed;  // next unread virtual word
  const uint64_t has = v_end & 1;
  const uint64_t steps = has ? (v_end >> 1) : (v_end >> 1) - 1;
  u128 s = ustream_advance(st, steps);
  st[0] = (uint64_t)(s >> 64);
  st[1] = (uint64_t)s;
  st[4] = has;
  st[5] = has ? (ustream_output(s) >> 32) : 0;
}

}  // namespace adapm
