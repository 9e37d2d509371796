// jb_wc.cpp — the host side of the word counts: jb_wc_count, the rule of jiebahip.h with an ordinary map
// (what the kernels of jb_wc.hip are pinned to), the size helpers, jb_wc_fp, the reader of a table copied
// to host memory (jb_wc_read's second half) and a sequential insert through jb_wc.h's shared code.  Host
// only, no HIP.
#include "jb_wc.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "jb_err.h"
#include "jiebahip.h"

static_assert(sizeof(JbWcHeader) <= JB_WC_HDR_BYTES, "the header fits its block");

namespace jb {

int wc_sizes(const char* who, uint64_t nslots, uint64_t pool_bytes) {
    if (nslots < JB_WC_MIN_SLOTS || (nslots & (nslots - 1u)) != 0)
        return fail(JB_EINVAL, "%s: nslots %llu (a power of two >= %u)", who, (unsigned long long)nslots, JB_WC_MIN_SLOTS);
    if (nslots > JB_WC_MAX_SLOTS)
        return fail(JB_ELIMIT, "%s: nslots %llu (limit 2^30)", who, (unsigned long long)nslots);
    if (pool_bytes >= (1ull << 32) - 256u)
        return fail(JB_ELIMIT, "%s: a pool of %llu bytes (limit 4 GiB)", who, (unsigned long long)pool_bytes);
    return JB_OK;
}

int wc_table_args(const char* who, const void* d_table, size_t ntable) {
    if (!d_table) return fail(JB_EINVAL, "%s: null table", who);
    if (((uintptr_t)d_table & 31u) != 0) return fail(JB_EINVAL, "%s: d_table must be 32-byte aligned", who);
    if (ntable < jb_wc_bytes(JB_WC_MIN_SLOTS, 0))
        return fail(JB_EINVAL, "%s: a table buffer of %llu bytes, the smallest table has %llu", who,
                    (unsigned long long)ntable, (unsigned long long)jb_wc_bytes(JB_WC_MIN_SLOTS, 0));
    return JB_OK;
}

void wc_host_add(const JbWcView& v, const uint8_t* key, uint32_t len, uint32_t k, uint32_t bits) {
    v.hdr->ctr[JB_WC_TOKENS]++;
    uint32_t kw[6];
    jb_wc_words(key, len, kw);
    const uint64_t h = jb_vocab_hash(kw, key, len), fp = jb_wc_fp_of(h, bits);
    uint32_t s = jb_wc_find(v.fp, v.mask, fp);
    if (s == JB_WC_NOSLOT && v.hdr->nclaimed < ((uint64_t)v.mask + 1u) / 2u) {  // claim
        s = jb_wc_home(fp, v.mask);
        for (uint32_t i = 0; i <= v.mask && v.fp[s] != 0u; i++) s = jb_vocab_next(s, v.mask);
        if (v.fp[s] == 0u) {
            v.fp[s] = fp;
            v.hdr->nclaimed++;
        } else {
            s = JB_WC_NOSLOT;  // (a table filled past its half by a device's concurrent claims)
        }
    }
    if (s == JB_WC_NOSLOT) {
        v.hdr->ctr[JB_WC_DROPPED]++;
        return;
    }
    uint32_t* q = v.key + (uint64_t)s * JB_VOCAB_SLOT_WORDS;
    if (q[0] == 0u) {  // store
        q[1] = k;
        uint32_t off = 0;
        bool room = true;
        if (len > JB_VOCAB_INLINE) {
            const unsigned long long o = v.hdr->pool_used;
            v.hdr->pool_used += len;
            room = o + len <= v.pool_bytes;
            off = (uint32_t)o;
        }
        if (room) jb_wc_put(q, v.pool, kw, key, len, h, off);
        else q[0] = JB_WC_DEAD;
    }
    if (q[0] == JB_WC_DEAD) v.hdr->ctr[JB_WC_DROPPED]++;  // count
    else if (jb_wc_same(q, v.pool, kw, key, len, h)) v.cnt[s]++;
    else v.hdr->ctr[JB_WC_COLLIDED]++;
}

namespace {

using Entry = std::pair<std::string, uint64_t>;

// `all` (distinct keys with their counts) in the rule's order, filtered, into out's arrays.
int wc_emit(const char* who, std::vector<Entry>& all, uint64_t min_count, uint64_t max_keys, jb_wc_result* out) {
    std::sort(all.begin(), all.end(), [](const Entry& a, const Entry& b) {
        if (a.second != b.second) return a.second > b.second;
        return a.first.compare(b.first) < 0;  // (memcmp, a proper prefix first)
    });
    uint64_t n = 0, nb = 0;
    for (const Entry& e : all) {
        if (e.second < min_count || (max_keys && n == max_keys)) break;
        n++;
        nb += e.first.size();
    }
    out->keys = (uint8_t*)malloc(nb ? nb : 1);
    out->key_off = (uint64_t*)malloc((n + 1) * sizeof(uint64_t));
    out->counts = (uint64_t*)malloc((n ? n : 1) * sizeof(uint64_t));
    if (!out->keys || !out->key_off || !out->counts) {
        jb_wc_result_free(out);
        return fail(JB_ENOMEM, "%s: out of host memory for %llu keys", who, (unsigned long long)n);
    }
    uint64_t pos = 0;
    for (uint64_t i = 0; i < n; i++) {
        out->key_off[i] = pos;
        memcpy(out->keys + pos, all[i].first.data(), all[i].first.size());
        pos += all[i].first.size();
        out->counts[i] = all[i].second;
    }
    out->key_off[n] = pos;
    out->nkeys = n;
    return JB_OK;
}

}  // namespace

int wc_read_host(const void* table, uint64_t ntable, uint64_t min_count, uint64_t max_keys, jb_wc_result* out) {
    const JbWcHeader* h = (const JbWcHeader*)table;
    if (ntable < JB_WC_HDR_BYTES || h->magic != JB_WC_MAGIC || h->nslots < JB_WC_MIN_SLOTS ||
        h->nslots > JB_WC_MAX_SLOTS || (h->nslots & (h->nslots - 1u)) != 0 || h->pool_bytes >= (1ull << 32) ||
        jb_wc_bytes(h->nslots, h->pool_bytes) > ntable)
        return fail(JB_EINVAL, "jb_wc_read: the buffer holds no table (jb_wc_init_device)");
    const JbWcView v = jb_wc_view(const_cast<void*>(table), h->nslots, h->pool_bytes);
    std::vector<Entry> all;
    try {
        for (uint64_t s = 0; s < h->nslots; s++) {
            const uint32_t* q = v.key + s * JB_VOCAB_SLOT_WORDS;
            const uint32_t len = q[0] & 0xFFu;
            if (v.fp[s] == 0u || len == 0u || v.cnt[s] == 0u) continue;  // (empty, not stored or dead, never counted)
            const uint8_t* p = (const uint8_t*)(q + 2);
            if (len > JB_VOCAB_INLINE) {
                if ((uint64_t)q[2] + len > h->pool_bytes) return fail(JB_EINVAL, "jb_wc_read: a key outside the pool");
                p = v.pool + q[2];
            }
            all.emplace_back(std::string((const char*)p, len), v.cnt[s]);
        }
    } catch (const std::bad_alloc&) {
        return fail(JB_ENOMEM, "jb_wc_read: out of host memory");
    }
    out->nbad = h->ctr[JB_WC_BAD];
    out->nlong = h->ctr[JB_WC_LONG];
    out->ndropped = h->ctr[JB_WC_DROPPED];
    out->ncollided = h->ctr[JB_WC_COLLIDED];
    out->ntokens = h->ctr[JB_WC_TOKENS];
    return wc_emit("jb_wc_read", all, min_count, max_keys, out);
}

}  // namespace jb

static size_t sat(uint64_t x) { return x > (uint64_t)SIZE_MAX ? SIZE_MAX : (size_t)x; }

extern "C" size_t jb_wc_table_bytes(uint64_t nslots, uint64_t pool_bytes) {
    uint64_t n = JB_WC_MIN_SLOTS;  // (the least valid slot count that is >= nslots, so that the size is monotone)
    while (n < nslots && n < (1ull << 62)) n <<= 1;
    if (n > (1ull << 40) || pool_bytes > (1ull << 48)) return SIZE_MAX;
    return sat(jb_wc_bytes(n, pool_bytes));
}

extern "C" size_t jb_wc_work_bytes(uint64_t max_tokens) {
    if (max_tokens > (1ull << 60)) return SIZE_MAX;
    return sat(jb_wc_r256(std::max<uint64_t>(max_tokens, 1u) * 4u));
}

extern "C" uint64_t jb_wc_fp(const uint8_t* key, size_t len, uint32_t bits) {
    if (!key || len == 0 || len > JB_VOCAB_MAXKEY || bits == 0 || bits > 64u) return 0;
    uint32_t kw[6];
    jb_wc_words(key, (uint32_t)len, kw);
    return jb_wc_fp_of(jb_vocab_hash(kw, key, (uint32_t)len), bits);
}

extern "C" void jb_wc_result_free(jb_wc_result* r) {
    if (!r) return;
    free(r->keys);
    free(r->key_off);
    free(r->counts);
    memset(r, 0, sizeof *r);
}

extern "C" int jb_wc_count(const uint8_t* text, uint64_t nbytes, const uint32_t* start, const uint32_t* end,
                           uint64_t ntok, uint64_t cap, uint64_t min_count, uint64_t max_keys, jb_wc_result* out) {
    if (!out) return fail(JB_EINVAL, "jb_wc_count: null argument");
    memset(out, 0, sizeof *out);
    if ((nbytes && !text) || (cap && (!start || !end))) return fail(JB_EINVAL, "jb_wc_count: null argument");
    if (nbytes >= (1ull << 31))
        return fail(JB_ELIMIT, "jb_wc_count: a text of %llu bytes (limit 2 GiB)", (unsigned long long)nbytes);
    const uint64_t n = std::min(ntok, cap);
    std::vector<jb::Entry> all;
    try {
        std::unordered_map<std::string, uint64_t> m;
        for (uint64_t k = 0; k < n; k++) {
            const uint64_t s = start[k], e = end[k];
            if (s >= e || e > nbytes) out->nbad++;  // (no text byte is read)
            else if (e - s > JB_VOCAB_MAXKEY) out->nlong++;
            else if (e - s == 1 && text[s] >= 0x80) m["\xEF\xBF\xBD"]++;
            else m[std::string((const char*)text + s, e - s)]++;
        }
        all.assign(m.begin(), m.end());
    } catch (const std::bad_alloc&) {
        return fail(JB_ENOMEM, "jb_wc_count: out of host memory");
    }
    out->ntokens = n;
    return jb::wc_emit("jb_wc_count", all, min_count, max_keys, out);
}
