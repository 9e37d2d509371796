// jb_vocab.h — a caller's vocabulary as a flat hash table: layout, hash and probe
// shared by the host builder / lookup (jb_vocab.cpp) and the gfx950 kernel k_ids
// (jb_k_modes.hip), which run the same code below.
//
// The vocabulary is a list of byte strings (1..255 bytes, any content); a key's id is
// its index in the list.  It is not the trie: the trie holds only the all-Han keys
// buildDag can reach, a vocabulary holds whatever a caller's model numbers.
//
//   slots[nslots]   8 u32 each (32 bytes, so a slot never straddles a 64-byte sector):
//                     [0] length | tag << 8   (0: the slot is empty; tag = hash bits 40..63)
//                     [1] id
//                     [2..7] the key's bytes, little-endian, zero-padded (length <= 24), or
//                     [2] the key's offset in the pool (length > 24; [3..7] are 0)
//                   nslots is a power of two >= 2 * nkeys (at least JB_VOCAB_MIN_SLOTS); a key
//                   sits at the first free slot from hash & (nslots - 1), stepping by one.
//   pool[]          the bytes of the keys longer than 24 bytes, back to back
//
// A lookup of a token of up to 8 bytes reads 16 bytes of one slot per probe (length, tag,
// id and the 8 key bytes); up to 24 bytes, the slot's other 16; longer ones, the pool too.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "jb_common.h"

#define JB_VOCAB_UNK 0xFFFFFFFFu    // JB_ID_UNK (jiebahip.h)
#define JB_VOCAB_MAXKEY 255u        // bytes
#define JB_VOCAB_INLINE 24u         // key bytes held in the slot
#define JB_VOCAB_SLOT_WORDS 8u      // u32 per slot
#define JB_VOCAB_MIN_SLOTS 8u
#define JB_VOCAB_MAX_KEYS (1u << 30)  // (nslots fits 32 bits)

// One 8-byte word of the key (little-endian, zero-padded past the key's end) into the hash.
JB_HD uint64_t jb_vocab_mix(uint64_t h, uint64_t w) {
    h = (h ^ w) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 32);
}
JB_HD uint64_t jb_vocab_hash_init(uint32_t len) { return 0x243F6A8885A308D3ull ^ ((uint64_t)len * 0xFF51AFD7ED558CCDull); }
JB_HD uint64_t jb_vocab_hash_fin(uint64_t h) {
    h *= 0xD6E8FEB86659FD93ull;
    return h ^ (h >> 32);
}

// The hash of the key `len` bytes long whose first min(len, 24) bytes are kw[0..5] (little-endian
// words, zero past the key's end) and whose bytes from 24 on are at tail[24..len) (read only when
// len > 24; `tail` is the key's first byte).
JB_HD uint64_t jb_vocab_hash(const uint32_t kw[6], const uint8_t* tail, uint32_t len) {
    uint64_t h = jb_vocab_hash_init(len);
    h = jb_vocab_mix(h, kw[0] | ((uint64_t)kw[1] << 32));
    if (len > 8u) h = jb_vocab_mix(h, kw[2] | ((uint64_t)kw[3] << 32));
    if (len > 16u) h = jb_vocab_mix(h, kw[4] | ((uint64_t)kw[5] << 32));
    for (uint32_t p = JB_VOCAB_INLINE; p < len; p += 8u) {
        uint64_t w = 0;
        for (uint32_t k = 0; k < 8u && p + k < len; k++) w |= (uint64_t)tail[p + k] << (8u * k);
        h = jb_vocab_mix(h, w);
    }
    return jb_vocab_hash_fin(h);
}
JB_HD uint32_t jb_vocab_tag(uint64_t h) { return (uint32_t)(h >> 40); }
JB_HD uint32_t jb_vocab_home(uint64_t h, uint32_t mask) { return (uint32_t)h & mask; }
JB_HD uint32_t jb_vocab_next(uint32_t slot, uint32_t mask) { return (slot + 1u) & mask; }
JB_HD uint32_t jb_vocab_head(uint32_t len, uint64_t h) { return len | (jb_vocab_tag(h) << 8); }

// The table as a lookup sees it (host vectors or device arrays).
struct JbVocabView {
    const uint32_t* slots;  // nslots * JB_VOCAB_SLOT_WORDS, 32-byte aligned
    const uint8_t* pool;
    uint32_t mask;    // nslots - 1
    uint32_t maxlen;  // the longest key, bytes (0: no keys)
};

// The id of the key (kw, tail, len) as jb_vocab_hash takes it, or JB_VOCAB_UNK.  1 <= len <=
// JB_VOCAB_MAXKEY.  Length and tag are compared first, then the bytes.
JB_HD uint32_t jb_vocab_find(const JbVocabView& v, const uint32_t kw[6], const uint8_t* tail, uint32_t len) {
    if (len > v.maxlen) return JB_VOCAB_UNK;
    const uint64_t h = jb_vocab_hash(kw, tail, len);
    const uint32_t head = jb_vocab_head(len, h);
    // (an empty slot ends every chain: at most half the slots are taken)
    for (uint32_t s = jb_vocab_home(h, v.mask);; s = jb_vocab_next(s, v.mask)) {
        const uint32_t* q = v.slots + (uint64_t)s * JB_VOCAB_SLOT_WORDS;
#if defined(__HIP_DEVICE_COMPILE__)
        const uint4 a = *reinterpret_cast<const uint4*>(q);
        const uint32_t a0 = a.x, a1 = a.y, a2 = a.z, a3 = a.w;
#else
        const uint32_t a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3];
#endif
        if (a0 == 0u) return JB_VOCAB_UNK;
        if (a0 != head) continue;
        if (len <= JB_VOCAB_INLINE) {
            if (a2 != kw[0] || a3 != kw[1]) continue;
            if (len > 8u) {
#if defined(__HIP_DEVICE_COMPILE__)
                const uint4 b = *reinterpret_cast<const uint4*>(q + 4);
                const uint32_t b0 = b.x, b1 = b.y, b2 = b.z, b3 = b.w;
#else
                const uint32_t b0 = q[4], b1 = q[5], b2 = q[6], b3 = q[7];
#endif
                if (b0 != kw[2] || b1 != kw[3] || b2 != kw[4] || b3 != kw[5]) continue;
            }
            return a1;
        }
        const uint8_t* k = v.pool + a2;
        uint32_t i = 0;
        while (i < len && k[i] == tail[i]) i++;
        if (i == len) return a1;
    }
}

namespace jb {

// The table on the host; the device copy is these two arrays as they are.
struct Vocab {
    std::vector<uint32_t> slots;  // nslots * JB_VOCAB_SLOT_WORDS
    std::vector<uint8_t> pool;    // (+ 8 bytes of padding, so that pool.data() is never null)
    uint32_t nkeys = 0;
    uint32_t maxlen = 0;
    uint64_t nslots = 0;
    JbVocabView view() const {
        return JbVocabView{slots.data(), pool.data(), (uint32_t)(nslots - 1u), maxlen};
    }
};

// Key i = keys[key_off[i] .. key_off[i+1]); key_off has nkeys + 1 entries, key_off[0] == 0.
// Returns 0 or a negative JB_E* code (JB_EINVAL: an empty key, offsets that are not non-decreasing
// from 0, a duplicate key; JB_ELIMIT: a key over 255 bytes, too many keys; JB_ENOMEM); err
// receives a message.  nkeys == 0 gives a valid, empty vocabulary.
int vocab_build(const uint8_t* keys, const uint64_t* key_off, uint32_t nkeys, Vocab* out, std::string* err);
// The device probe on the host: the id of tok[0..len), or JB_VOCAB_UNK.
uint32_t vocab_lookup(const Vocab& v, const uint8_t* tok, size_t len);

}  // namespace jb

// The C ABI's handle of a table (jb_vocab_build).
struct jb_vocab {
    jb::Vocab v;
};
