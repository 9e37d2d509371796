// jb_minhash.h — the MinHash rule (jb_minhash*, jiebahip.h): the hash family, the shingle fold, the slot
// value and the band key, shared by the host rule (jb_minhash.cpp) and the gfx950 kernels (jb_minhash.hip),
// which run the code below.  All arithmetic is unsigned and modulo 2^64 unless a width is stated.
//
// A token's hash t is jb_vocab_hash of its key (jb_ids_device's key, cut to its first JB_VOCAB_MAXKEY
// bytes; the empty key for a malformed span).  A shingle's hash folds the hashes of its c tokens:
// fin(mix(... mix(init(c), t_0) ..., t_{c-1})), and x is its low 32 bits.  Hash function j of a seed is
// (a_j, b_j), values 2j and 2j + 1 of the seed's splitmix64 sequence (a_j made odd); a slot holds the
// least (uint32_t)((a_j * x + b_j) >> 32) over its document's shingles.
#pragma once
#include "jb_vocab.h"

#define JB_MH_GOLDEN 0x9E3779B97F4A7C15ull

// Value i (0-based) of the splitmix64 sequence that starts from st = seed: its state is seed + (i + 1) * G,
// so every value can be had on its own.
JB_HD uint64_t jb_mh_draw(uint64_t seed, uint64_t i) {
    uint64_t z = seed + (i + 1u) * JB_MH_GOLDEN;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
JB_HD uint64_t jb_mh_a(uint64_t seed, uint32_t j) { return jb_mh_draw(seed, 2ull * j) | 1ull; }
JB_HD uint64_t jb_mh_b(uint64_t seed, uint32_t j) { return jb_mh_draw(seed, 2ull * j + 1u); }

// Multiply-shift: the high half of a 64 x 32-bit multiply-add.
JB_HD uint32_t jb_mh_slot(uint64_t a, uint64_t b, uint32_t x) { return (uint32_t)((a * (uint64_t)x + b) >> 32); }

// x of the shingle over the c token hashes t[0..c) (1 <= c <= JB_MH_MAXN).
JB_HD uint32_t jb_mh_shingle(const uint64_t* t, uint32_t c) {
    uint64_t g = jb_vocab_hash_init(c);
    for (uint32_t i = 0; i < c; i++) g = jb_vocab_mix(g, t[i]);
    return (uint32_t)jb_vocab_hash_fin(g);
}

// The shingles of a document of m tokens under width n: their number, and how many tokens each folds.
JB_HD uint32_t jb_mh_count(uint64_t m, uint32_t n) { return m == 0 ? 0u : m < n ? 1u : (uint32_t)(m - n + 1u); }
JB_HD uint32_t jb_mh_width(uint64_t m, uint32_t n) { return m < n ? (uint32_t)m : n; }

// The key of band `band` (R rows) of a signature row; never JB_MH_NOKEY (all ones).
JB_HD uint64_t jb_mh_band(const uint32_t* row, uint32_t band, uint32_t R) {
    uint64_t g = jb_vocab_mix(jb_vocab_hash_init(R), band);
    for (uint32_t r = 0; r < R; r++) g = jb_vocab_mix(g, row[(uint64_t)band * R + r]);
    g = jb_vocab_hash_fin(g);
    return g == ~0ull ? ~0ull - 1u : g;
}

// The first min(len, 24) bytes of a key as jb_vocab_hash's words (what k_mh_hash builds from aligned dwords).
JB_HD void jb_mh_words(const uint8_t* key, uint32_t len, uint32_t kw[6]) {
    for (uint32_t w = 0; w < 6u; w++) kw[w] = 0u;
    for (uint32_t i = 0; i < len && i < JB_VOCAB_INLINE; i++) kw[i >> 2] |= (uint32_t)key[i] << (8u * (i & 3u));
}

// The host side (jb_minhash.cpp).
#pragma GCC visibility push(hidden)
namespace jb {

// The limits the host rule and the device call share: JB_OK, or JB_EINVAL / JB_ELIMIT with the thread's
// message set.
int minhash_args(const char* who, uint64_t nbytes, uint64_t cap, uint32_t n, uint32_t K);
int minhash_band_args(const char* who, uint32_t K, uint32_t B, uint32_t R);

}  // namespace jb
#pragma GCC visibility pop
