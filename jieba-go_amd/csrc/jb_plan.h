// jb_plan.h — the host layer's pure planners: how a batch is divided over devices, cut units and
// pipeline pieces.  Arithmetic over doc_off (and the text, for Han-run starts); no HIP, no device.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#pragma GCC visibility push(hidden)

// One pipeline piece of a range: documents [d0, d1), the byte offset of its text in the device (and
// pinned staging) buffer, and the first of its d1 - d0 + 1 slots in the offsets buffer.
struct Piece { uint32_t d0, d1; uint64_t off, slot; };

struct PiecePlan {
    std::vector<Piece> pcs;
    uint64_t dev_bytes = 0;  // text buffer: 64 zero bytes after each piece, 256-byte aligned starts
    uint64_t slots = 0;      // offsets buffer
    uint64_t maxb = 0;       // the longest piece, bytes
    uint32_t maxd = 0;       // the most documents in a piece
};

// Documents [d0, d1) in pieces of whole documents of at most piece_bytes (a longer document is a
// piece of its own), in order.
PiecePlan plan_pieces(const uint64_t* doc_off, uint32_t d0, uint32_t d1, uint64_t piece_bytes);

uint64_t han_run_start(const uint8_t* t, uint64_t lo, uint64_t hi, uint64_t pos);

// Cut units: documents, or parts of documents cut at Han-run starts (han_run_start),
// so that one large document spreads over several devices and over
// several pipeline pieces within a device.  Unit u is bytes [off[u], off[u+1]) of
// document doc[u]; device k owns units [dev[k], dev[k+1]).
struct Units {
    std::vector<uint64_t> off;
    std::vector<uint32_t> doc;
    std::vector<uint32_t> dev;
};

// The units of a batch over nd devices (device k's pipeline piece is piece_bytes[k]).  With one
// device and no document longer than its piece nothing is split: *split is false, the units are
// the documents and *un stays empty.  Otherwise the device ranges are byte-balanced
// (jb_split_points; (*cutb)[k] is device k's first byte) and parts longer than a piece are cut
// into units at Han-run starts.
int plan_units(const uint8_t* text, const uint64_t* doc_off, uint32_t ndocs, const uint64_t* piece_bytes, size_t nd,
               Units* un, std::vector<uint64_t>* cutb, bool* split);

#pragma GCC visibility pop
