// jb_wc.h — the word-count table (jb_wc_*): layout, fingerprint, probe, key store and key compare
// shared by the host code (jb_wc.cpp: the reader, the argument checks and a sequential insert) and the
// gfx950 kernels (jb_wc.hip), which run the code below.
//
// The table is one caller-owned device buffer:
//   header          JB_WC_HDR_BYTES: JbWcHeader (sizes, the five u64 totals, the claimed slots, the pool's fill)
//   fp[nslots]      u64  the slot's fingerprint: jb_wc_fp of its key's jb_vocab_hash (0: the slot is empty)
//   cnt[nslots]     u64  the tokens counted for the slot's key
//   key[nslots]     8 u32 each, the key slot of jb_vocab.h's layout:
//                     [0] length | tag << 8   (0: the bytes are not stored yet; JB_WC_DEAD: the pool had no
//                                              room for them, the slot's tokens are dropped)
//                     [1] the representative: the least index of a token that claimed the slot in the batch
//                         that claimed it (where jb_vocab.h keeps the id)
//                     [2..7] the key's bytes (length <= 24), or [2] its offset in the pool
//   pool[]          the bytes of the keys longer than 24 bytes, back to back
// nslots is a power of two >= JB_WC_MIN_SLOTS; a new key is accepted while fewer than nslots / 2 slots are
// claimed (lanes that claim at the same moment can pass the half, so no probe relies on an empty slot: each
// is bounded by nslots steps).  A fingerprint sits at the first slot from jb_wc_home(fp) on, stepping by
// one, that was empty when it came.
//
// jb_vocab_find's compare cannot be called on one slot (it owns the probe loop), so jb_wc_same below is
// that compare on its own: head first, then the inline words or the pool's bytes.
#pragma once
#include "jb_vocab.h"

#define JB_WC_HDR_BYTES 256u
#define JB_WC_MIN_SLOTS 8u
#define JB_WC_MAX_SLOTS (1u << 30)
#define JB_WC_SLOT_BYTES 48u                // fp, cnt and the key slot
#define JB_WC_MAGIC 0x31544357424Aull       // "JBWCT1"
#define JB_WC_DEAD 0x00000100u              // a head no key has: length 0, tag 1
#define JB_WC_NOREP 0xFFFFFFFFu
// d_work codes of the tokens that have no slot (slots are < JB_WC_MAX_SLOTS)
#define JB_WC_NOSLOT 0xFFFFFFFFu            // no slot found or claimed: looked up again by the count pass
#define JB_WC_BADSPAN 0xFFFFFFFEu
#define JB_WC_LONGKEY 0xFFFFFFFDu

enum { JB_WC_BAD = 0, JB_WC_LONG, JB_WC_DROPPED, JB_WC_COLLIDED, JB_WC_TOKENS, JB_WC_NCTR };

struct JbWcHeader {
    uint64_t magic, nslots, pool_bytes;
    uint64_t ctr[JB_WC_NCTR];               // JB_WC_*: totals over every batch added
    unsigned long long pool_used;           // bytes handed out (it passes pool_bytes when the pool ran out)
    uint32_t nclaimed;                      // slots whose fingerprint is set
    uint32_t pad;
};

// The table as the code below sees it (device pointers in a kernel, host pointers in the reader).
struct JbWcView {
    JbWcHeader* hdr;
    uint64_t* fp;
    uint64_t* cnt;
    uint32_t* key;   // nslots * JB_VOCAB_SLOT_WORDS
    uint8_t* pool;
    uint32_t mask;   // nslots - 1
    uint64_t pool_bytes;
};

JB_HD uint64_t jb_wc_r256(uint64_t x) { return (x + 255u) & ~(uint64_t)255u; }
// Bytes of a table (nslots is a valid slot count).
JB_HD uint64_t jb_wc_bytes(uint64_t nslots, uint64_t pool_bytes) {
    return JB_WC_HDR_BYTES + nslots * JB_WC_SLOT_BYTES + jb_wc_r256(pool_bytes);
}
JB_HD JbWcView jb_wc_view(void* base, uint64_t nslots, uint64_t pool_bytes) {
    uint8_t* b = (uint8_t*)base;
    JbWcView v;
    v.hdr = (JbWcHeader*)b;
    v.fp = (uint64_t*)(b + JB_WC_HDR_BYTES);
    v.cnt = v.fp + nslots;
    v.key = (uint32_t*)(v.cnt + nslots);
    v.pool = (uint8_t*)(v.key + nslots * JB_VOCAB_SLOT_WORDS);
    v.mask = (uint32_t)(nslots - 1u);
    v.pool_bytes = pool_bytes;
    return v;
}

// The fingerprint of a key whose jb_vocab_hash is h: its low `bits` bits (1..64), and 1 where they are 0,
// the empty marker.  (Hashes 0 and 1 then share a fingerprint: a collision like any other, reported.)
JB_HD uint64_t jb_wc_fp_of(uint64_t h, uint32_t bits) {
    if (bits < 64u) h &= (1ull << bits) - 1u;
    return h ? h : 1ull;
}
// The home slot depends on the fingerprint alone, so equal fingerprints walk the same chain.
JB_HD uint32_t jb_wc_home(uint64_t fp, uint32_t mask) { return (uint32_t)fp & mask; }

// The slot that holds fp, or JB_WC_NOSLOT: a read-only probe of at most nslots steps that ends at the
// first empty slot.
JB_HD uint32_t jb_wc_find(const uint64_t* fpv, uint32_t mask, uint64_t fp) {
    uint32_t s = jb_wc_home(fp, mask);
    for (uint32_t i = 0; i <= mask; i++, s = jb_vocab_next(s, mask)) {
        const uint64_t f = fpv[s];
        if (f == fp) return s;
        if (f == 0u) break;
    }
    return JB_WC_NOSLOT;
}

// Is the key stored in slot q (8 words; its head is neither 0 nor JB_WC_DEAD) the key (kw, tail, len) as
// jb_vocab_hash takes it, whose hash is h?  jb_vocab_find's compare: length and tag, then the bytes.
JB_HD bool jb_wc_same(const uint32_t* q, const uint8_t* pool, const uint32_t kw[6], const uint8_t* tail, uint32_t len,
                      uint64_t h) {
    if (q[0] != jb_vocab_head(len, h)) return false;
    if (len <= JB_VOCAB_INLINE) {
        if (q[2] != kw[0] || q[3] != kw[1]) return false;
        if (len > 8u && (q[4] != kw[2] || q[5] != kw[3] || q[6] != kw[4] || q[7] != kw[5])) return false;
        return true;
    }
    const uint8_t* k = pool + q[2];
    uint32_t i = 0;
    while (i < len && k[i] == tail[i]) i++;
    return i == len;
}

// Store the key (kw, tail, len) in slot q, whose head is 0; pool_off is where its bytes go when len > 24
// (the caller has made sure that pool_off + len <= pool_bytes).  The head is written last.
JB_HD void jb_wc_put(uint32_t* q, uint8_t* pool, const uint32_t kw[6], const uint8_t* tail, uint32_t len, uint64_t h,
                     uint32_t pool_off) {
    if (len <= JB_VOCAB_INLINE) {
        for (uint32_t w = 0; w < 6u; w++) q[2u + w] = kw[w];
    } else {
        q[2] = pool_off;
        for (uint32_t w = 3; w < JB_VOCAB_SLOT_WORDS; w++) q[w] = 0u;
        for (uint32_t i = 0; i < len; i++) pool[pool_off + i] = tail[i];
    }
    q[0] = jb_vocab_head(len, h);
}

// The first min(len, 24) bytes of a key as jb_vocab_hash's words (what k_wc_* build from aligned dwords).
JB_HD void jb_wc_words(const uint8_t* key, uint32_t len, uint32_t kw[6]) {
    for (uint32_t w = 0; w < 6u; w++) kw[w] = 0u;
    for (uint32_t i = 0; i < len && i < JB_VOCAB_INLINE; i++) kw[i >> 2] |= (uint32_t)key[i] << (8u * (i & 3u));
}

// The host side (jb_wc.cpp).
struct jb_wc_result;  // (jiebahip.h)
#pragma GCC visibility push(hidden)
namespace jb {

// The limits of a table's sizes: JB_OK, or JB_EINVAL / JB_ELIMIT with the thread's message set.
int wc_sizes(const char* who, uint64_t nslots, uint64_t pool_bytes);
// What every call that is handed a table checks: JB_OK, or JB_EINVAL with the thread's message set.
int wc_table_args(const char* who, const void* d_table, size_t ntable);
// One token of key[0..len) (1 <= len <= 255, the key already formed) added to a table in host memory: what
// the three kernels do to it, one token at a time and in order, through the code above (the sanitizer
// program builds tables with it).  k is the token's index in its batch, bits the fingerprint's width.
void wc_host_add(const JbWcView& v, const uint8_t* key, uint32_t len, uint32_t k, uint32_t bits);
// jb_wc_read on a table copied to host memory (ntable bytes): the header is checked, the stored keys with
// a count are sorted and filtered into out's arrays, the totals copied.  JB_EINVAL when no table is there.
int wc_read_host(const void* table, uint64_t ntable, uint64_t min_count, uint64_t max_keys, ::jb_wc_result* out);

}  // namespace jb
#pragma GCC visibility pop
