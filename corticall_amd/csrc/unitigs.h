// Unitigs of a colour set: the compacted de Bruijn graph of a resident table.
//
// Vertices are the records with coverage in at least one colour of the set S, in both orientations (oriented vertex
// a = 2 * record + flip, flip = the k-mer is the record's reverse complement).  Adjacency is the record's own edge bytes ORed
// over S, oriented by string comparison with the canonical k-mer (TraversalUtils.getAllNextKmers / getAllPrevKmers,
// J/utils/traversal/TraversalUtils.java:510-557; the quirk-Q6 flip does not apply).  x -> y is a unitig edge iff out(x) = {y},
// in(y) = {x}, y is a vertex, canon(x) != canon(y) and neither is a palindrome.  A unitig is a maximal path of unitig edges;
// a pure cycle is cut at its smallest canonical k-mer.  Each unitig is reported once, in its alphanumerically lowest
// orientation, and unitigs are numbered in the record order of their first k-mer.
//
// Device tables (kept until the handle is freed):
//   lab[record]    u64  unitig id (bits 0..31, ~0 = not a vertex) | position (32..62) | orientation (63: the unitig holds the
//                       record's reverse complement)
//   off[U + 1]     u64  first base of unitig u in seq; off[U] = total bases
//   hd[U], tl[U]   u32  oriented vertex of the first and of the last k-mer of unitig u
//   cov[U][C]      u32  coverage of unitig u summed over its k-mers, every colour of the graph (wraps like a Java int)
//   seq[off[U]]    u8   the unitigs' bases, ASCII, back to back
#pragma once
#include <string>
#include <vector>

#include "devmem.h"
#include "graph.h"

namespace ldbg {

#define LDBG_UNITIG_NONE 0xFFFFFFFFu

// (ldbg_unitigs_write_gfa1 flags: LDBG_GFA_PLUS_STRAND, include/ldbg.h)

class Unitigs {
public:
    Unitigs(const Graph& g, const int* colors, int n_colors);
    const Graph& graph;
    int64_t count = 0;          // unitigs
    int64_t total_bases = 0;
    int64_t longest = 0;        // bases of the longest unitig
    int64_t members = 0;        // vertices (records) in unitigs
    double build_ms = 0;
    uint64_t color_mask = 0;

    // unitigs [first, first + n): offsets relative to off[first] (n + 1 entries) and their bases
    void get(int64_t first, int64_t n, int64_t* offsets, char* bases, int64_t capacity, bool device_out, rt::stream_t s) const;
    void coverage(int64_t first, int64_t n, uint32_t* cov) const;            // n x C, host
    void of_records(const int64_t* recs, int64_t n, int64_t* uid, int64_t* pos, int8_t* orient) const;
    void write_fasta(const std::string& path) const;
    void write_gfa1(const std::string& path, int sample_color, int flags) const;

    Unitigs(const Unitigs&) = delete;
    Unitigs& operator=(const Unitigs&) = delete;

private:
    uint64_t* d_lab_ = nullptr; uint64_t* d_off_ = nullptr; uint32_t* d_hd_ = nullptr; uint32_t* d_tl_ = nullptr;
    uint32_t* d_cov_ = nullptr; uint8_t* d_seq_ = nullptr;
    DevBlocks own_;             // holds them
};

}  // namespace ldbg
