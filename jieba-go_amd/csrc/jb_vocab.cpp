// jb_vocab.cpp — host side of the vocabulary table (layout, hash and probe: jb_vocab.h).
// No HIP dependency: the builder and the lookup the CPU tests and the device upload use.
#include "jb_vocab.h"

#include <string.h>

#include <cstdio>
#include <new>

#include "../../include/jiebahip.h"

namespace jb {

static int vfail(std::string* err, int code, const char* fmt, unsigned long long a = 0, unsigned long long b = 0,
                 unsigned long long c = 0) {
    if (err) {
        char buf[256];
        snprintf(buf, sizeof buf, fmt, a, b, c);
        *err = buf;
    }
    return code;
}

// The first min(len, 24) bytes of a key as jb_vocab_hash and the slots hold them.
static void key_words(const uint8_t* k, uint32_t len, uint32_t kw[6]) {
    uint8_t b[JB_VOCAB_INLINE] = {0};
    memcpy(b, k, len < JB_VOCAB_INLINE ? len : JB_VOCAB_INLINE);
    for (uint32_t i = 0; i < 6u; i++)
        kw[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) |
                ((uint32_t)b[4 * i + 3] << 24);
}

int vocab_build(const uint8_t* keys, const uint64_t* key_off, uint32_t nkeys, Vocab* out, std::string* err) {
    if (!out || (nkeys && (!keys || !key_off))) return vfail(err, JB_EINVAL, "jb_vocab_build: null argument");
    if (nkeys > JB_VOCAB_MAX_KEYS)
        return vfail(err, JB_ELIMIT, "vocabulary of %llu keys (limit %llu)", nkeys, JB_VOCAB_MAX_KEYS);
    if (nkeys && key_off[0] != 0) return vfail(err, JB_EINVAL, "key_off[0] is %llu, not 0", key_off[0]);
    uint64_t pool_bytes = 0;
    uint32_t maxlen = 0;
    for (uint32_t i = 0; i < nkeys; i++) {
        if (key_off[i + 1] < key_off[i])
            return vfail(err, JB_EINVAL, "key_off decreases at key %llu (%llu after %llu)", i, key_off[i + 1],
                         key_off[i]);
        const uint64_t len = key_off[i + 1] - key_off[i];
        if (len == 0) return vfail(err, JB_EINVAL, "key %llu is empty", i);
        if (len > JB_VOCAB_MAXKEY)
            return vfail(err, JB_ELIMIT, "key %llu has %llu bytes (limit %llu)", i, len, JB_VOCAB_MAXKEY);
        if (len > JB_VOCAB_INLINE) pool_bytes += len;
        if (len > maxlen) maxlen = (uint32_t)len;
    }
    if (pool_bytes >= (1ull << 32))
        return vfail(err, JB_ELIMIT, "%llu bytes of keys longer than %llu bytes (limit 4 GiB)", pool_bytes,
                     JB_VOCAB_INLINE);
    uint64_t nslots = JB_VOCAB_MIN_SLOTS;
    while (nslots < 2ull * nkeys) nslots <<= 1;
    Vocab v;
    try {
        v.slots.assign(nslots * JB_VOCAB_SLOT_WORDS, 0u);
        v.pool.reserve(pool_bytes + 8u);
    } catch (const std::bad_alloc&) {
        return vfail(err, JB_ENOMEM, "out of host memory for a vocabulary of %llu keys", nkeys);
    }
    v.nkeys = nkeys;
    v.maxlen = maxlen;
    v.nslots = nslots;
    const uint32_t mask = (uint32_t)(nslots - 1u);
    for (uint32_t i = 0; i < nkeys; i++) {
        const uint8_t* k = keys + key_off[i];
        const uint32_t len = (uint32_t)(key_off[i + 1] - key_off[i]);
        uint32_t kw[6];
        key_words(k, len, kw);
        const uint64_t h = jb_vocab_hash(kw, k, len);
        const uint32_t head = jb_vocab_head(len, h);
        uint32_t s = jb_vocab_home(h, mask);
        for (;; s = jb_vocab_next(s, mask)) {
            const uint32_t* q = &v.slots[(uint64_t)s * JB_VOCAB_SLOT_WORDS];
            if (q[0] == 0u) break;
            if (q[0] != head) continue;
            const bool same = len <= JB_VOCAB_INLINE ? memcmp(q + 2, kw, sizeof(uint32_t) * 6u) == 0
                                                     : memcmp(v.pool.data() + q[2], k, len) == 0;
            if (same) return vfail(err, JB_EINVAL, "keys %llu and %llu are the same", q[1], i);
        }
        uint32_t* q = &v.slots[(uint64_t)s * JB_VOCAB_SLOT_WORDS];
        q[0] = head;
        q[1] = i;
        if (len <= JB_VOCAB_INLINE) {
            memcpy(q + 2, kw, sizeof(uint32_t) * 6u);
        } else {
            q[2] = (uint32_t)v.pool.size();
            v.pool.insert(v.pool.end(), k, k + len);
        }
    }
    v.pool.resize(v.pool.size() + 8u, 0);
    *out = std::move(v);
    return JB_OK;
}

uint32_t vocab_lookup(const Vocab& v, const uint8_t* tok, size_t len) {
    if (!tok || len == 0 || len > v.maxlen || v.nslots == 0) return JB_VOCAB_UNK;
    uint32_t kw[6];
    key_words(tok, (uint32_t)len, kw);
    return jb_vocab_find(v.view(), kw, tok, (uint32_t)len);
}

}  // namespace jb
