// batch_layout_check — the layout of the host-text calls' first device buffer (jieba-go_amd/csrc/jb_batch.h:
// batch_layout, batch_chain_extra, Arena) on the CPU, under AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_batch_layout_host.py builds and runs it; the header's HIP-free part alone, nothing to link).
// Over a grid of batch sizes, document counts, span capacities and extra bytes: every piece starts on a 256-byte
// boundary, the pieces are disjoint, in order and in bounds, and the total is the sum that each entry point of
// jb_capi.cpp wrote out for itself before the front was shared.  Where the buffer is small enough to allocate,
// every piece is also written to its last byte, and an Arena walked over the same sizes lands on the same offsets.
// Prints "ok" and exits 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#define JB_BATCH_LAYOUT_ONLY
#include "jb_batch.h"

#define CHECK(c)                                                                                       \
    do {                                                                                               \
        if (!(c)) {                                                                                    \
            fprintf(stderr, "%s:%d: %s failed (nb %llu ndocs %u cap %llu extra %llu)\n", __FILE__, __LINE__, #c, \
                    (unsigned long long)g_nb, g_ndocs, (unsigned long long)g_cap, (unsigned long long)g_extra);   \
            exit(1);                                                                                   \
        }                                                                                              \
    } while (0)
static uint64_t g_nb, g_cap, g_extra;
static uint32_t g_ndocs;

static uint64_t R(uint64_t x) { return (x + 255u) / 256u * 256u; }  // (the test's own rounding)

static void check_point(uint64_t nb, uint32_t ndocs, uint64_t cap, uint64_t extra, bool chain) {
    g_nb = nb, g_ndocs = ndocs, g_cap = cap, g_extra = extra;
    const uint64_t ndoc8 = ((uint64_t)ndocs + 1) * 8;
    const size_t ex = chain ? batch_chain_extra(ndocs, extra) : extra;
    const BatchLayout l = batch_layout(nb, ndocs, cap, ex);
    // the parent's expressions: the span calls', and the chain's with its third ndocs + 1 array and extra0
    const uint64_t spans = R(nb + 64) + 2 * R(ndoc8) + R(16) + R(2 * cap * 4);
    CHECK(l.total == (chain ? spans + R(ndoc8) + extra : spans + extra));
    // the pieces, in order, each with the bytes its user writes or reads
    const struct {
        uint64_t off, len;
    } piece[] = {{l.text, nb + 64}, {l.doff, ndoc8}, {l.dtok, ndoc8}, {l.dcnt, 16}, {l.dse, 2 * cap * 4}, {l.extra, ex}};
    const int np = (int)(sizeof piece / sizeof piece[0]);
    CHECK(piece[0].off == 0);
    for (int k = 0; k < np; k++) {
        CHECK(piece[k].off % 256 == 0);
        CHECK(piece[k].off + piece[k].len <= (k + 1 < np ? piece[k + 1].off : l.total));
    }
    CHECK(l.doff - l.text >= nb + 64);  // the text piece holds the text and its padding
    if (chain) CHECK(ex >= ndoc8 + extra);
    if (l.total > (1u << 20)) return;
    // a real buffer of exactly `total` bytes
    uint8_t* buf = (uint8_t*)malloc(l.total ? l.total : 1);
    CHECK(buf != nullptr);
    for (int k = 0; k < np; k++) memset(buf + piece[k].off, k + 1, piece[k].len);
    for (int k = 0; k < np; k++)
        if (piece[k].len) CHECK(buf[piece[k].off] == k + 1 && buf[piece[k].off + piece[k].len - 1] == k + 1);
    Arena a;
    a.p = buf;
    for (int k = 0; k + 1 < np; k++) CHECK(a.take(piece[k].len) == buf + piece[k].off);
    CHECK(a.off == l.extra);
    if (chain) {  // the chain takes its term offsets first, then its caller takes extra0
        CHECK(a.take(ndoc8) == buf + l.extra);
        CHECK(a.off + extra == l.total);
    }
    free(buf);
}

int main() {
    const uint64_t nbs[] = {0, 1, 191, 192, 193, 255, 256, 257, (1ull << 31) - 1};
    const uint32_t nds[] = {1, 31, 32, 33, 5000};
    const uint64_t extras[] = {0, 1, 256};
    CHECK(r256(0) == 0 && r256(1) == 256 && r256(256) == 256 && r256(257) == 512);
    for (uint64_t nb : nbs)
        for (uint32_t nd : nds)
            for (uint64_t cap : {(uint64_t)1, nb, nb + 1})
                for (uint64_t extra : extras)
                    for (bool chain : {false, true}) check_point(nb, nd, cap, extra, chain);
    printf("ok\n");
    return 0;
}
