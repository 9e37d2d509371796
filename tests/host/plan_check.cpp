// plan_check — the host layer's planners (jieba-go_amd/csrc/jb_plan.cpp) on the CPU, under
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_plan_host.py builds and runs it with
// jb_plan.cpp and jb_err.cpp alone): plan_pieces' layout on hand-written and seeded doc_off arrays,
// plan_units' cuts on small texts that mix Han runs, ASCII and 4-byte runes, for 1, 2 and 3 devices.
//   plan_check          every property; prints "ok" and exits 0
//   plan_check --dump   the unit lists of the fixed inputs as JSON (tests/golden/plan_units.json holds
//                       what the code gave before the planners were split out of jb_capi.cpp)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "jb_common.h"
#include "jb_plan.h"
#include "jiebahip.h"

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #c, g_case.c_str()); \
            exit(1);                                                  \
        }                                                             \
    } while (0)
static std::string g_case;

// ---- plan_pieces ----------------------------------------------------------------------------
static std::vector<uint64_t> offsets(const std::vector<uint64_t>& lens, uint64_t base) {
    std::vector<uint64_t> off{base};
    for (uint64_t l : lens) off.push_back(off.back() + l);
    return off;
}

static void check_pieces(const std::vector<uint64_t>& off, uint32_t d0, uint32_t d1, uint64_t pb) {
    const uint64_t* o = off.data();
    const PiecePlan pl = plan_pieces(o, d0, d1, pb);
    CHECK(pl.pcs.empty() == (d0 >= d1));
    uint64_t dev = 0, slots = 0, maxb = 0;
    uint32_t maxd = 0, at = d0;
    for (size_t i = 0; i < pl.pcs.size(); i++) {
        const Piece& p = pl.pcs[i];
        CHECK(p.d0 == at && p.d1 > p.d0 && p.d1 <= d1);  // a partition of [d0, d1), in order
        at = p.d1;
        const uint64_t len = o[p.d1] - o[p.d0];
        if (p.d1 - p.d0 > 1) CHECK(len <= pb);
        for (uint32_t j = p.d0; j < p.d1; j++)
            if (o[j + 1] - o[j] > pb) CHECK(p.d1 - p.d0 == 1);  // a longer document is a piece of its own
        if (p.d1 < d1) CHECK(o[p.d1 + 1] - o[p.d0] > pb);      // greedy: the next document did not fit
        CHECK(p.off % 256 == 0 && p.off == dev);
        const uint64_t next = i + 1 < pl.pcs.size() ? pl.pcs[i + 1].off : pl.dev_bytes;
        CHECK(next >= p.off + len + 64);  // the piece's text and 64 bytes after it, before the next piece
        CHECK(p.slot == slots);
        dev += (len + 64 + 255) & ~255ull;
        slots += p.d1 - p.d0 + 1;
        maxb = std::max(maxb, len);
        maxd = std::max(maxd, p.d1 - p.d0);
    }
    if (!pl.pcs.empty()) CHECK(at == d1);
    CHECK(pl.dev_bytes == dev && pl.slots == slots && pl.maxb == maxb && pl.maxd == maxd);
}

static void pieces_cases() {
    const uint64_t pb = 1024;
    struct Case { const char* name; std::vector<uint64_t> lens; uint32_t d0, d1; };
    std::vector<uint64_t> empties{500};
    empties.insert(empties.end(), 1500, 0);  // a run of empty documents, more of them than a piece has bytes
    empties.push_back(600);
    const std::vector<Case> cases = {
        {"d0 > 0", {300, 300, 300, 500, 600, 100}, 2, 6},
        {"d0 > 0, d1 < ndocs", {300, 300, 300, 500, 600, 100}, 1, 4},
        {"empty documents at the start, in the middle and at the end", {0, 0, 400, 0, 0, 700, 300, 0, 0}, 0, 9},
        {"a long run of empty documents", empties, 0, (uint32_t)empties.size()},
        {"only empty documents", std::vector<uint64_t>(40, 0), 0, 40},
        {"piece_bytes exactly, and one more", {1024, 1025, 10, 1024, 1, 1023, 1, 1}, 0, 8},
        {"a single document", {5}, 0, 1},
        {"a single empty document", {0}, 0, 1},
        {"a single long document", {5000}, 0, 1},
        {"no documents", {7, 7}, 1, 1},
    };
    for (const Case& c : cases)
        for (uint64_t base : {0ull, 77ull, 1ull << 40}) {
            g_case = c.name;
            check_pieces(offsets(c.lens, base), c.d0, c.d1, pb);
        }
    std::mt19937_64 g(20240607);
    for (int it = 0; it < 400; it++) {
        g_case = "seeded " + std::to_string(it);
        const uint32_t nd = 1 + (uint32_t)(g() % 60);
        const uint64_t p = 1 + g() % 3000;
        std::vector<uint64_t> lens(nd);
        for (auto& l : lens) {
            const uint64_t k = g() % 8;
            l = k == 0 ? 0 : k == 1 ? p : k == 2 ? p + 1 : k == 3 ? g() % (4 * p) : g() % (p / 3 + 2);
        }
        const uint32_t a = (uint32_t)(g() % (nd + 1)), b = a + (uint32_t)(g() % (nd + 1 - a));
        check_pieces(offsets(lens, g() % 1000), a, b, p);
        check_pieces(offsets(lens, 0), 0, nd, p);
    }
}

// ---- plan_units -----------------------------------------------------------------------------
static void put_rune(std::string* s, uint32_t r) {
    if (r < 0x80) s->push_back((char)r);
    else if (r < 0x800) { s->push_back((char)(0xC0 | r >> 6)); s->push_back((char)(0x80 | (r & 63))); }
    else if (r < 0x10000) {
        s->push_back((char)(0xE0 | r >> 12)); s->push_back((char)(0x80 | (r >> 6 & 63))); s->push_back((char)(0x80 | (r & 63)));
    } else {
        s->push_back((char)(0xF0 | r >> 18)); s->push_back((char)(0x80 | (r >> 12 & 63)));
        s->push_back((char)(0x80 | (r >> 6 & 63))); s->push_back((char)(0x80 | (r & 63)));
    }
}

struct Batch {
    std::string text;
    std::vector<uint64_t> off;  // doc_off (off[0] may be past 0)
};

// Documents of Han runs (3-byte runes, some 4-byte ones), ASCII words, emoji (4-byte, not Han),
// 2-byte runes and a few stray bytes.  max_run: the longest Han run, in runes.
static Batch make_batch(uint64_t seed, uint32_t ndocs, uint64_t bytes, uint32_t max_run, uint64_t lead) {
    std::mt19937_64 g(seed);
    Batch b;
    b.text.assign(lead, 'x');
    b.off.push_back(lead);
    for (uint32_t d = 0; d < ndocs; d++) {
        const uint64_t want = g() % 5 == 0 ? 0 : bytes / ndocs / 2 + g() % (bytes / ndocs + 1);
        const uint64_t start = b.text.size();
        while (b.text.size() - start < want) {
            switch (g() % 6) {
            case 0: case 1:
                for (uint32_t n = 1 + (uint32_t)(g() % max_run); n; n--)
                    put_rune(&b.text, g() % 9 == 0 ? 0x20000u + (uint32_t)(g() % 0xA000) : 0x4E00u + (uint32_t)(g() % 0x5000));
                break;
            case 2:
                for (uint32_t n = 1 + (uint32_t)(g() % 12); n; n--) b.text.push_back((char)('a' + g() % 26));
                b.text.push_back(' ');
                break;
            case 3:
                for (uint32_t n = 1 + (uint32_t)(g() % 3); n; n--) put_rune(&b.text, 0x1F600u + (uint32_t)(g() % 64));
                break;
            case 4:
                put_rune(&b.text, 0xE9);
                put_rune(&b.text, 0x3002);  // an ideographic full stop: 3 bytes, not Han
                break;
            default:
                b.text.push_back((char)(g() % 2 ? 0x80 : 0xFF));  // a stray continuation byte, an invalid byte
            }
        }
        b.off.push_back(b.text.size());
    }
    return b;
}

// q is a Han-run start of the document [lo, hi): decoding rune by rune from lo reaches q, the rune
// there is Han and the rune before it is not.
static bool is_han_run_start(const uint8_t* t, uint64_t lo, uint64_t hi, uint64_t q) {
    bool prev_han = false;
    for (uint64_t p = lo; p < hi;) {
        uint32_t x = 0, r;
        const uint64_t lim = std::min<uint64_t>(4, hi - p);
        for (uint64_t k = 0; k < lim; k++) x |= (uint32_t)t[p + k] << (8 * k);
        const uint32_t w = jb_decode(x, (uint32_t)lim, &r);
        if (p == q) return jb_is_han(r) && !prev_han;
        if (p > q) return false;  // inside a rune
        prev_han = jb_is_han(r);
        p += w;
    }
    return false;
}

struct UnitCase {
    std::string name;
    Batch b;
    size_t nd;
    uint64_t pb;
};

static std::vector<UnitCase> unit_cases() {
    std::vector<UnitCase> v;
    const struct { const char* name; uint64_t seed; uint32_t ndocs; uint64_t bytes; uint32_t run; uint64_t lead; } texts[] = {
        {"mixed", 11, 12, 4096, 40, 0},
        {"mixed, doc_off[0] > 0", 12, 7, 3000, 25, 37},
        {"one document", 13, 1, 3500, 30, 0},
        {"Han runs longer than a piece", 14, 3, 4000, 400, 0},
        {"many short documents", 15, 60, 2500, 6, 0},
    };
    for (const auto& t : texts)
        for (size_t nd : {1, 2, 3})
            for (uint64_t pb : {256ull, 700ull, 1ull << 20})
                v.push_back(UnitCase{std::string(t.name) + ", " + std::to_string(nd) + " devices, piece " + std::to_string(pb),
                                     make_batch(t.seed, t.ndocs, t.bytes, t.run, t.lead), nd, pb});
    return v;
}

namespace {
struct UnitPlan {
    Units un;
    std::vector<uint64_t> cutb;
    bool split = false;
};
}  // namespace

static UnitPlan run_units(const UnitCase& c) {
    UnitPlan p;
    // (an exact-size heap copy: a read past the text's end is a report)
    std::vector<uint8_t> text(c.b.text.begin(), c.b.text.end());
    const std::vector<uint64_t> pbs(c.nd, c.pb);
    const int rc = plan_units(text.data(), c.b.off.data(), (uint32_t)c.b.off.size() - 1, pbs.data(), c.nd, &p.un, &p.cutb,
                              &p.split);
    CHECK(rc == JB_OK);
    return p;
}

static void check_units(const UnitCase& c) {
    g_case = c.name;
    const UnitPlan p = run_units(c);
    const std::vector<uint64_t>& doc_off = c.b.off;
    const uint32_t ndocs = (uint32_t)doc_off.size() - 1;
    const uint64_t b0 = doc_off[0], b1 = doc_off[ndocs];
    const uint8_t* t = reinterpret_cast<const uint8_t*>(c.b.text.data());
    bool longer = false;
    for (uint32_t j = 0; j < ndocs; j++) longer |= doc_off[j + 1] - doc_off[j] > c.pb;
    CHECK(p.cutb.size() == c.nd + 1 && p.cutb[0] == b0 && p.cutb[c.nd] == b1);
    CHECK(std::is_sorted(p.cutb.begin(), p.cutb.end()));
    if (c.nd == 1 && !longer) {  // the units are the documents
        CHECK(!p.split && p.un.off.empty() && p.un.doc.empty() && p.un.dev.empty());
        return;
    }
    CHECK(p.split);
    const Units& un = p.un;
    const size_t nu = un.doc.size();
    CHECK(un.off.size() == nu + 1 && un.off[0] == b0 && un.off[nu] == b1);  // the units tile [b0, b1)
    uint32_t docs_seen = 0;
    for (size_t u = 0; u < nu; u++) {
        const uint32_t j = un.doc[u];
        CHECK(j < ndocs && un.off[u] <= un.off[u + 1]);
        CHECK(doc_off[j] <= un.off[u] && un.off[u + 1] <= doc_off[j + 1]);  // inside its document
        if (u == 0 || un.doc[u - 1] != j) {  // a document's first unit starts the document; none is skipped
            CHECK(j == docs_seen && un.off[u] == doc_off[j]);
            docs_seen++;
        } else {  // a cut inside a document: a Han-run start, where han_run_start puts it
            CHECK(un.off[u] > doc_off[j] && un.off[u] < doc_off[j + 1]);
            CHECK(is_han_run_start(t, doc_off[j], doc_off[j + 1], un.off[u]));
            CHECK(han_run_start(t, doc_off[j], doc_off[j + 1], un.off[u]) == un.off[u]);
        }
    }
    CHECK(docs_seen == ndocs);
    CHECK(un.dev.size() == c.nd + 1 && un.dev[0] == 0 && un.dev[c.nd] == nu);
    CHECK(std::is_sorted(un.dev.begin(), un.dev.end()));
    for (size_t k = 0; k < c.nd; k++)  // a device's units start inside its byte range
        for (uint32_t u = un.dev[k]; u < un.dev[k + 1]; u++) CHECK(un.off[u] >= p.cutb[k] && un.off[u] <= p.cutb[k + 1]);
}

template <class T>
static void dump_list(const char* key, const std::vector<T>& v, const char* tail) {
    printf("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); i++) printf("%s%llu", i ? ", " : "", (unsigned long long)v[i]);
    printf("]%s", tail);
}

int main(int argc, char** argv) {
    const std::vector<UnitCase> cases = unit_cases();
    if (argc > 1 && !strcmp(argv[1], "--dump")) {
        printf("[\n");
        for (size_t i = 0; i < cases.size(); i++) {
            const UnitPlan p = run_units(cases[i]);
            printf("{\"name\": \"%s\", \"split\": %s, ", cases[i].name.c_str(), p.split ? "true" : "false");
            dump_list("cutb", p.cutb, ", ");
            dump_list("off", p.un.off, ", ");
            dump_list("doc", p.un.doc, ", ");
            dump_list("dev", p.un.dev, i + 1 < cases.size() ? "},\n" : "}\n");
        }
        printf("]\n");
        return 0;
    }
    pieces_cases();
    for (const UnitCase& c : cases) check_units(c);
    printf("ok\n");
    return 0;
}
