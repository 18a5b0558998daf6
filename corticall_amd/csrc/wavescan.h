// What the batch lanes that mark, count and compact share (select.cpp, build.cpp, linkbuild.cpp): positions are walked in
// chunks, one wavefront per chunk -> one 64-bit ballot word per 64 positions and one count per chunk -> the chunk counts scanned by one
// wavefront -> the marked positions placed from the ballots and the offsets; and the LDS stage through which records of 13, 21, 29 ...
// bytes leave as whole dwords.  Every kernel is launched one wavefront per workgroup and uses wavefront primitives only: no workgroup
// waits for another and nothing is placed with an atomic.  Internal linkage, as bldpack.h: each source launches its own copy.
#pragma once
#include "rt.h"

namespace ldbg {
namespace {

#ifdef LDBG_HOSTSIM
#define LDBG_WS wave_size()    // (a simulated wavefront may be narrower than 64 lanes: a ballot word is assembled from 64 / lanes ballots then)
#else
#define LDBG_WS 64             // (the wavefront kernels are launched with 64-thread workgroups)
#endif

int waves_for(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>(items, 8192)); }

// positions of the chunk that starts at c0, to a whole ballot word
LDBG_DEV int chunk_lim(int64_t n, int64_t c0, int chunk) { return (int)std::min<int64_t>(chunk, (n - c0 + 63) & ~(int64_t)63); }

// One step of a chunk's walk, NP predicates side by side: ok[p] is the lane's answer to predicate p for position c0 + s + lane, whose
// ballot joins the word cur[p]; a finished word p goes to out[p][(c0 + s) >> 6].  Returns the answers in a finished word of the LAST predicate.
template <int NP>
LDBG_DEV uint32_t ballot_step(int64_t c0, int s, const bool (&ok)[NP], unsigned long long (&cur)[NP], unsigned long long* const (&out)[NP]) {
    uint32_t cnt = 0;
#pragma unroll
    for (int p = 0; p < NP; p++) cur[p] |= wave_ballot(ok[p]) << (s & 63);
    if (((s + LDBG_WS) & 63) == 0) {
#pragma unroll
        for (int p = 0; p < NP; p++) {
            if (wave_lane() == 0) out[p][(c0 + s) >> 6] = cur[p];
            if (p == NP - 1) cnt = (uint32_t)__builtin_popcountll(cur[p]);
            cur[p] = 0;
        }
    }
    return cnt;
}

// exclusive prefix sums of the chunk counts, by one wavefront; *total = their sum
template <class Off>
LDBG_WAVE_KERNEL void k_chunk_top(int64_t nchunks, const uint32_t* chunk_cnt, Off* chunk_off, Off* total) {
    const int ws = LDBG_WS, lane = wave_lane();
    if (global_tid() / ws != 0) return;
    Off run = 0;
    for (int64_t b = 0; b < nchunks; b += ws) {
        const int64_t i = b + lane;
        const uint32_t v = i < nchunks ? chunk_cnt[i] : 0u;
        const uint32_t incl = wave_incl_scan_u32(v);
        if (i < nchunks) chunk_off[i] = run + incl - v;
        run += wave_bcast_u32(incl, ws - 1);
    }
    wave_fence();
    if (lane == 0) *total = run;
}

// Ballot word g of the lane (0 past the last) and the answers before it: `run` counts those before the wavefront's words and moves on
// past them.
struct GroupWord { unsigned long long m, base; };
LDBG_DEV GroupWord group_word(const unsigned long long* words, int64_t g, int64_t ngroups, unsigned long long& run) {
    const unsigned long long m = g < ngroups ? words[g] : 0ull;
    const uint32_t c = (uint32_t)__builtin_popcountll(m), incl = wave_incl_scan_u32(c);
    const GroupWord w{m, run + incl - c};
    run += wave_bcast_u32(incl, LDBG_WS - 1);
    return w;
}

// Records of R bytes each, up to 64 of them, staged by a wavefront for dst: in LDS they start at stage_bytes(), shifted so that LDS and
// output agree modulo 4, and stage_write_out() writes the stretch as head bytes, whole dwords and tail bytes.
#define LDBG_STAGE_WORDS(colours) (64 * (32 + 5 * (colours)) / 4 + 2)
LDBG_DEV uint8_t* stage_bytes(uint32_t* stage, const uint8_t* dst) { return (uint8_t*)stage + ((uintptr_t)dst & 3u); }
LDBG_DEV void stage_write_out(const uint32_t* stage, uint8_t* dst, int nrec, int R) {
    const int ws = LDBG_WS, lane = wave_lane(), mis = (int)((uintptr_t)dst & 3u);
    const uint8_t* lb = (const uint8_t*)stage + mis;
    wave_fence();
    const int nbytes = nrec * R, head = mis ? std::min(nbytes, 4 - mis) : 0, nd = (nbytes - head) >> 2;
    for (int i = lane; i < head; i += ws) dst[i] = lb[i];
    const uint32_t* ls = stage + ((mis + head) >> 2);
    uint32_t* gd = (uint32_t*)(dst + head);
    for (int i = lane; i < nd; i += ws) gd[i] = ls[i];
    for (int i = head + 4 * nd + lane; i < nbytes; i += ws) dst[i] = lb[i];
    wave_fence();                                  // (the next stretch overwrites the stage)
}

// ---- exclusive prefix sums of n 32-bit values (modulo 2^32) in three launches: the sum of every chunk, the chunk sums scanned by
// one wavefront (k_chunk_top), every chunk scanned from its offset; out[n] = the total
#define LDBG_SCAN_CHUNK 4096        // elements one wavefront sums and scans: one entry of the scanned chunk sums
LDBG_WAVE_KERNEL void k_scan_chunk_sums(const uint32_t* in, int64_t n, uint32_t* sums) {
    const int ws = LDBG_WS, lane = wave_lane();
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws, nchunks = (n + LDBG_SCAN_CHUNK - 1) / LDBG_SCAN_CHUNK;
    for (int64_t ch = wave; ch < nchunks; ch += nwaves) {
        const int64_t c0 = ch * LDBG_SCAN_CHUNK;
        const int lim = (int)std::min<int64_t>(LDBG_SCAN_CHUNK, n - c0);
        uint32_t acc = 0;
        for (int t = lane; t < lim; t += ws) acc += in[c0 + t];
        const uint32_t incl = wave_incl_scan_u32(acc), tot = wave_bcast_u32(incl, ws - 1);
        if (lane == 0) sums[ch] = tot;
    }
}
LDBG_WAVE_KERNEL void k_scan_chunk_scan(const uint32_t* in, int64_t n, const uint32_t* offs, uint32_t* out) {
    const int ws = LDBG_WS, lane = wave_lane();
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws, nchunks = (n + LDBG_SCAN_CHUNK - 1) / LDBG_SCAN_CHUNK;
    for (int64_t ch = wave; ch < nchunks; ch += nwaves) {
        const int64_t c0 = ch * LDBG_SCAN_CHUNK;
        const int lim = (int)std::min<int64_t>(LDBG_SCAN_CHUNK, n - c0);
        uint32_t run = offs[ch];
        for (int t = 0; t < lim; t += ws) {
            const bool live = t + lane < lim;
            const uint32_t v = live ? in[c0 + t + lane] : 0u;
            const uint32_t incl = wave_incl_scan_u32(v);
            if (live) out[c0 + t + lane] = run + incl - v;
            run += wave_bcast_u32(incl, ws - 1);
        }
    }
    if (global_tid() == 0) out[n] = offs[nchunks];
}

// d_out[n + 1]; d_sums and d_offs hold one entry per chunk and one more
void scan_u32(const uint32_t* d_in, int64_t n, uint32_t* d_out, uint32_t* d_sums, uint32_t* d_offs, rt::stream_t s) {
    if (n <= 0) { rt::dmemset(d_out, 0, 4, s); return; }
    const int64_t nchunks = (n + LDBG_SCAN_CHUNK - 1) / LDBG_SCAN_CHUNK;
    LDBG_LAUNCH(k_scan_chunk_sums, waves_for(nchunks), 64, s, d_in, n, d_sums);
    LDBG_LAUNCH(k_chunk_top<uint32_t>, 1, 64, s, nchunks, (const uint32_t*)d_sums, d_offs, d_offs + nchunks);
    LDBG_LAUNCH(k_scan_chunk_scan, waves_for(nchunks), 64, s, d_in, n, (const uint32_t*)d_offs, d_out);
}

}  // namespace
}  // namespace ldbg
