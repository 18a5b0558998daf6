// SmithWaterman.align of n pairs on the device (sw.h): SmithWaterman.java:89-294 with EDNAFULL.
//   k_sw: one wavefront per pair.  The query is cut into strips of wave_size() rows; lane l owns row x0 + l and step t of a strip computes
//     the anti-diagonal cells (x0 + l, t - l + 1).  A lane keeps its left neighbour [x][y-1] in registers and receives [x-1][y] (M, C, R)
//     and the subject letter from lane l - 1 by a one-lane shift; [x-1][y-1] is what it received a step earlier.  Lane 0 takes the row above
//     the strip, and the subject, from blocks of wave_size() entries that all lanes load together and hand over one entry a step.  The last
//     lane's row is gathered the same way and stored a block at a time: it is the next strip's row above, in LDS up to SW_LDS_CELLS subject
//     letters and in a per-pair HBM scratch beyond.  One traceback byte per cell, [strip][step][lane].  Then a butterfly takes the maximum
//     (higher score, lower x, lower y) and lane 0 walks the traceback.
// int32 in half units throughout (score x 2, open 20, extend 1): every value the Java forms is a multiple of 0.5, so nothing is rounded.
// The TEST-ONLY host simulation runs the kernel as it is.
#include "sw.h"

#include <memory>

#include "devmem.h"
#include "graph.h"
#include "wavescan.h"

namespace ldbg {

namespace {

#define SW_LDS_CELLS 1024               // subject letters whose boundary row (M, C, R: 12 B) stays in LDS: 12 KiB a workgroup, 13 pairs on a compute unit
#define SW_X 16u                        // the code of 'X' (no row in the matrix: every pair with it scores 10000)
#define SW_OPEN 20
#define SW_EXTEND 1
#define SW_XSCORE 20000

// NUC.4.4 (ftp.ncbi.nih.gov/blast/matrices): rows and columns in the order of LDBG_SW_LETTERS
const int8_t NUC44[16][16] = {
    { 5, -4, -4, -4, -4,  1,  1, -4, -4,  1, -4, -1, -1, -1, -2, -4},
    {-4,  5, -4, -4, -4,  1, -4,  1,  1, -4, -1, -4, -1, -1, -2, -4},
    {-4, -4,  5, -4,  1, -4,  1, -4,  1, -4, -1, -1, -4, -1, -2, -4},
    {-4, -4, -4,  5,  1, -4, -4,  1, -4,  1, -1, -1, -1, -4, -2, -4},
    {-4, -4,  1,  1, -1, -4, -2, -2, -2, -2, -1, -1, -3, -3, -1, -4},
    { 1,  1, -4, -4, -4, -1, -2, -2, -2, -2, -3, -3, -1, -1, -1, -4},
    { 1, -4,  1, -4, -2, -2, -1, -4, -2, -2, -3, -1, -3, -1, -1, -4},
    {-4,  1, -4,  1, -2, -2, -4, -1, -2, -2, -1, -3, -1, -3, -1, -4},
    {-4,  1,  1, -4, -2, -2, -2, -2, -1, -4, -1, -3, -3, -1, -1, -4},
    { 1, -4, -4,  1, -2, -2, -2, -2, -4, -1, -3, -1, -1, -3, -1, -4},
    {-4, -1, -1, -1, -1, -3, -3, -1, -1, -3, -1, -2, -2, -2, -1, -4},
    {-1, -4, -1, -1, -1, -3, -1, -3, -3, -1, -2, -1, -2, -2, -1, -4},
    {-1, -1, -4, -1, -3, -1, -3, -1, -3, -1, -2, -2, -1, -2, -1, -4},
    {-1, -1, -1, -4, -3, -1, -1, -3, -1, -3, -2, -2, -2, -1, -1, -4},
    {-2, -2, -2, -2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -4},
    {-4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4, -4,  1},
};

struct SwArgs {
    int64_t first, n;                   // the slice: pairs [first, first + n) of the batch
    int lds_cells;                      // a subject of at most this many letters keeps the boundary row in LDS
    const uint64_t* rows;               // [16] a letter's row of the matrix, score + 4 in four bits per subject letter
    const uint8_t* run;                 // [n of the batch] 1: this pair runs on the device
    const int64_t* q_off; const uint8_t* qcode;           // the filtered letters as codes 0..16
    const int64_t* s_off; const uint8_t* scode;
    const int64_t* tb_off;              // [n of the batch] byte offset of the pair's traceback bytes in the arena
    const int64_t* scr_off;             // the same for its boundary row (3 x 4 B x |s|) where that is not in LDS
    uint8_t* arena;
    const int64_t* col_off;             // [n + 1] capacity |q| + |s| per pair that runs; the columns are written from the end backwards
    uint8_t* cols;
    int32_t* out;                       // [n][8] half units, end_q, end_s, begin_q, begin_s, columns, aligned_len, edits
};

template <bool L> LDBG_DEV int32_t sw_ld(const int32_t* p, int i) { if (L) return LDBG_LDS(const int32_t, p)[i]; return LDBG_GLOBAL(const int32_t, p)[i]; }
template <bool L> LDBG_DEV void sw_st(int32_t* p, int i, int32_t v) { if (L) LDBG_LDS(int32_t, p)[i] = v; else LDBG_GLOBAL(int32_t, p)[i] = v; }
LDBG_DEV int32_t sw_pos(int32_t v) { return v > 0 ? v : 0; }
// two values that travel between lanes together (one exchange of the host simulation; two 32-bit moves on the device either way)
LDBG_DEV uint64_t sw_pack(int32_t lo, int32_t hi) { return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo; }

template <bool L>
LDBG_DEV void sw_problem(const SwArgs& a, int64_t i, int32_t* row, int stride) {
    const int ws = LDBG_WS, lane = wave_lane();
    const int64_t q0 = a.q_off[i], s0 = a.s_off[i];
    const int Lq = (int)(a.q_off[i + 1] - q0), Ls = (int)(a.s_off[i + 1] - s0);
    const uint8_t* qc = a.qcode + q0;
    const uint8_t* sc = a.scode + s0;
    uint8_t* tb = a.arena + a.tb_off[i];
    const int64_t strip_bytes = (int64_t)(Ls + ws - 1) * ws;
    int32_t* rowM = row; int32_t* rowC = row + stride; int32_t* rowR = row + 2 * stride;
    int32_t best = 0, bx = 0x7fffffff, by = 0x7fffffff;          // the lane's maximum under getMaxScorePos' strict < (:281-291)
    const int nstrips = (Lq + ws - 1) / ws;
    for (int k = 0; k < nstrips; k++) {
        const int x = k * ws + lane + 1;
        const bool row_ok = x <= Lq;
        const uint32_t qcd = row_ok ? (uint32_t)LDBG_GLOBAL(const uint8_t, qc)[x - 1] : SW_X;
        const uint64_t qrow = LDBG_GLOBAL(const uint64_t, a.rows)[qcd & 15u];
        const bool first = k == 0, last = k == nstrips - 1;
        const int T = Ls + (last ? Lq - k * ws : ws) - 1;
        uint8_t* tbs = tb + (int64_t)k * strip_bytes;
        int32_t curM = 0, curC = 0, curR = 0, dM = 0, dC = 0, dR = 0, leftM = 0, leftC = 0;       // row 0 and column 0 are zero (:105-115)
        uint32_t sl_prev = SW_X;
        int32_t inM = 0, inC = 0, inR = 0, nxM = 0, nxC = 0, nxR = 0, keepM = 0, keepC = 0, keepR = 0;
        uint32_t inS = SW_X, nxS = SW_X;
        if (lane < Ls) {                // block 0 of the row above and of the subject
            nxS = LDBG_GLOBAL(const uint8_t, sc)[lane];
            if (!first) { nxM = sw_ld<L>(rowM, lane); nxC = sw_ld<L>(rowC, lane); nxR = sw_ld<L>(rowR, lane); }
        }
        for (int t = 0; t < T; t++) {
            const int j = t % ws;
            if (j == 0) {               // the next block is asked for a block ahead of its first use
                inM = nxM; inC = nxC; inR = nxR; inS = nxS;
                nxM = 0; nxC = 0; nxR = 0; nxS = SW_X;
                const int e = t + ws + lane;
                if (e < Ls) {
                    nxS = LDBG_GLOBAL(const uint8_t, sc)[e];
                    if (!first) { nxM = sw_ld<L>(rowM, e); nxC = sw_ld<L>(rowC, e); nxR = sw_ld<L>(rowR, e); }
                }
            }
            // [x-1][y] and the letter s[y-1]: from the lane below, lane 0 from entry t of the row above
            const uint64_t u0 = wave_shfl_up1_u64(sw_pack(curM, curC), wave_bcast_u64(sw_pack(inM, inC), j));
            const uint64_t u1 = wave_shfl_up1_u64(sw_pack(curR, (int32_t)sl_prev), wave_bcast_u64(sw_pack(inR, (int32_t)inS), j));
            const int32_t upM = (int32_t)(uint32_t)u0, upC = (int32_t)(u0 >> 32), upR = (int32_t)(uint32_t)u1;
            const uint32_t sl = (uint32_t)(u1 >> 32);
            const int y = t - lane + 1;
            if (row_ok && y >= 1 && y <= Ls) {
                const int32_t m = (qcd == SW_X || sl >= SW_X) ? SW_XSCORE : ((int32_t)((uint32_t)(qrow >> (4u * (sl & 15u))) & 15u) - 4) * 2;
                // MATCH from [x-1][y-1] (:118-143)
                const int32_t fm = sw_pos(dM + m), fc = sw_pos(dC + m), fr = sw_pos(dR + m);
                int32_t M; uint32_t bits;
                if (fm >= fr) { if (fm >= fc) { M = fm; bits = 0; } else { M = fc; bits = 1; } }
                else { if (fr > fc) { M = fr; bits = 2; } else { M = fc; bits = 1; } }
                // GAPINCOL from [x][y-1] (:147-162)
                const int32_t cm = sw_pos(leftM - SW_OPEN), cc = sw_pos(leftC - SW_EXTEND);
                int32_t Cv;
                if (cm >= cc) Cv = cm; else { Cv = cc; bits |= 4u; }
                // GAPINROW from [x-1][y] (:165-179)
                const int32_t rm = sw_pos(upM - SW_OPEN), rr = sw_pos(upR - SW_EXTEND);
                int32_t Rv;
                if (rm > rr) Rv = rm; else { Rv = rr; bits |= 8u; }
                if (M > 0) bits |= 16u;
                if (Cv > 0) bits |= 32u;
                if (Rv > 0) bits |= 64u;
                LDBG_GLOBAL(uint8_t, tbs)[(int64_t)t * ws + lane] = (uint8_t)bits;
                if (M > best) { best = M; bx = x; by = y; }
                if (Cv > best) { best = Cv; bx = x; by = y; }
                if (Rv > best) { best = Rv; bx = x; by = y; }
                curM = M; curC = Cv; curR = Rv; leftM = M; leftC = Cv;
            }
            dM = upM; dC = upC; dR = upR; sl_prev = sl;
            // the last lane's cell is entry e of the next strip's row above: gathered into lane e % ws, stored a block at a time
            const int e = t - (ws - 1);
            if (!last && e >= 0 && e < Ls) {
                const uint64_t o0 = wave_bcast_u64(sw_pack(curM, curC), ws - 1);
                const int32_t oM = (int32_t)(uint32_t)o0, oC = (int32_t)(o0 >> 32), oR = (int32_t)wave_bcast_u32((uint32_t)curR, ws - 1);
                const int jj = e % ws;
                if (lane == jj) { keepM = oM; keepC = oC; keepR = oR; }
                if ((jj == ws - 1 || e == Ls - 1) && lane <= jj) {
                    const int at = e - jj + lane;
                    sw_st<L>(rowM, at, keepM); sw_st<L>(rowC, at, keepC); sw_st<L>(rowR, at, keepR);
                }
            }
        }
    }
    // the maximum over the lanes: the higher score, then the lower x, then the lower y
    uint64_t pos = ((uint64_t)(uint32_t)bx << 32) | (uint32_t)by;
    for (int m = ws >> 1; m > 0; m >>= 1) {
        const uint64_t o = wave_shfl_xor_u64(((uint64_t)(uint32_t)best << 32), m);
        const uint64_t op = wave_shfl_xor_u64(pos, m);
        const int32_t ob = (int32_t)(o >> 32);
        if (ob > best || (ob == best && op < pos)) { best = ob; pos = op; }
    }
    wave_fence();                       // lane 0 reads the other lanes' traceback bytes
    if (lane != 0) return;
    // ---- :183-259
    int32_t* out = a.out + i * 8;
    if (best <= 0) {                    // new SWResult(): score -1
        out[0] = -2; out[1] = -1; out[2] = -1; out[3] = -1; out[4] = -1; out[5] = 0; out[6] = 0; out[7] = 0;
        return;
    }
    const int ex = (int)(pos >> 32), ey = (int)(uint32_t)pos;
    int cx = ex, cy = ey, lx = ex, ly = ey, ct = 0;
    int32_t ncols = 0, edits = 0;
    int64_t cp = a.col_off[i + 1];      // the columns are written from the end of the pair's room backwards
    uint8_t* cols = a.cols;
    auto differ = [&](int xx, int yy) { return LDBG_GLOBAL(const uint8_t, qc)[xx - 1] != LDBG_GLOBAL(const uint8_t, sc)[yy - 1]; };
    auto tb_at = [&](int xx, int yy) -> uint32_t {
        const int st = (xx - 1) / ws, l = (xx - 1) % ws;
        return LDBG_GLOBAL(const uint8_t, tb)[(int64_t)st * strip_bytes + (int64_t)(yy - 1 + l) * ws + l];
    };
    uint32_t b = tb_at(cx, cy);
    int cpt = (int)(b & 3u);
    LDBG_GLOBAL(uint8_t, cols)[--cp] = 0; ncols++;      // the pair at the maximum is appended before the loop (:203-204)
    if (differ(cx, cy)) edits++;
    for (;;) {
        if (ct == 0) { cx--; cy--; } else if (ct == 1) cy--; else cx--;
        ct = cpt;
        if (cx <= 0 || cy <= 0) break;  // row 0 and column 0 hold zeros: cs <= 0
        b = tb_at(cx, cy);
        if (!((b >> (4 + ct)) & 1u)) break;
        cpt = ct == 0 ? (int)(b & 3u) : ct == 1 ? (int)((b >> 2) & 1u) : (int)((b >> 3) & 1u) * 2;
        if (ct == 0) { LDBG_GLOBAL(uint8_t, cols)[--cp] = 0; if (differ(cx, cy)) edits++; lx = cx; ly = cy; }
        else if (ct == 1) { LDBG_GLOBAL(uint8_t, cols)[--cp] = 1; edits++; ly = cy; }
        else { LDBG_GLOBAL(uint8_t, cols)[--cp] = 2; edits++; lx = cx; }
        ncols++;
    }
    const int32_t ends = (lx - 1) + (ly - 1) + (Lq - ex) + (Ls - ey);      // the unaligned ends (:237-259): every column a gap
    out[0] = best; out[1] = ex; out[2] = ey; out[3] = lx; out[4] = ly; out[5] = ncols; out[6] = ncols + ends; out[7] = edits + ends;
}

LDBG_WAVE_KERNEL void k_sw(SwArgs a) {
#ifndef LDBG_HOSTSIM
    __shared__ int32_t lds[3 * SW_LDS_CELLS];
#else
    static int32_t lds[3 * SW_LDS_CELLS];             // (one simulated wavefront at a time: rt.h)
#endif
    const int ws = LDBG_WS;
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws;
    for (int64_t j = wave_uniform_i64(wave); j < a.n; j += nwaves) {
        const int64_t i = a.first + j;
        if (!a.run[i]) continue;
        const int64_t Ls = a.s_off[i + 1] - a.s_off[i];
        if (Ls <= a.lds_cells) sw_problem<true>(a, i, lds, SW_LDS_CELLS);
        else sw_problem<false>(a, i, (int32_t*)(a.arena + a.scr_off[i]), (int)Ls);
    }
}

void check_offsets(const int64_t* off, int64_t n, const char* what) {
    if (!off) throw StatusError(LDBG_ERR_ARG, std::string("sw: null ") + what);
    if (off[0] < 0) throw StatusError(LDBG_ERR_ARG, std::string("sw: negative ") + what);
    for (int64_t i = 0; i < n; i++)
        if (off[i + 1] < off[i]) throw StatusError(LDBG_ERR_ARG, std::string("sw: decreasing ") + what);
}

int64_t arena_budget() {
    if (const char* ev = getenv("LDBG_SW_ARENA_BYTES")) return std::max<int64_t>(1, atoll(ev));
    size_t free_b = 0, total_b = 0;
    rt::mem_info(&free_b, &total_b);
    return std::max<int64_t>(1, (int64_t)(free_b / 4));
}

int host_wave_size() {                  // the lanes of the wavefronts k_sw is launched with: the traceback bytes are laid out by it
#ifdef LDBG_HOSTSIM
    return std::min(64, sim::lanes_env());
#else
    return 64;
#endif
}

// Sequence.add (Sequence.java:48-61: \r and \n dropped) and EDNAFULL.filter (:63-80: NUL, '-' and '.' dropped, the 16 letters kept,
// everything else 'X'), of the bytes [b, e)
void filter(const char* b, const char* e, std::vector<uint8_t>& letters, std::vector<uint8_t>& codes, const uint8_t* code_of) {
    for (; b < e; b++) {
        const uint8_t c = (uint8_t)*b;
        if (c == '\r' || c == '\n' || c == 0 || c == '-' || c == '.') continue;
        const uint8_t cd = code_of[c];
        letters.push_back(cd == SW_X ? (uint8_t)'X' : c);
        codes.push_back(cd);
    }
}

}  // namespace

SwResult* sw_align_batch(int device, int64_t n, const char* queries, const int64_t* query_off, const char* subjects, const int64_t* subject_off) {
    if (n < 0) throw StatusError(LDBG_ERR_ARG, "sw: n < 0");
    std::unique_ptr<SwResult> res(new SwResult);
    res->n = n;
    res->status.assign((size_t)n, (uint8_t)LDBG_OK);
    res->score.assign((size_t)n, -1.0);
    res->end_q.assign((size_t)n, -1); res->end_s.assign((size_t)n, -1); res->begin_q.assign((size_t)n, -1); res->begin_s.assign((size_t)n, -1);
    res->aligned_len.assign((size_t)n, 0); res->edits.assign((size_t)n, 0);
    res->col_off.assign((size_t)n + 1, 0); res->q_off.assign((size_t)n + 1, 0); res->s_off.assign((size_t)n + 1, 0);
    if (n == 0) { profile_add("sw", 0.0); return res.release(); }
    check_offsets(query_off, n, "query offsets");
    check_offsets(subject_off, n, "subject offsets");
    if ((query_off[n] > query_off[0] && !queries) || (subject_off[n] > subject_off[0] && !subjects)) throw StatusError(LDBG_ERR_ARG, "sw: null sequences");

    uint8_t code_of[256];
    memset(code_of, (int)SW_X, sizeof(code_of));
    for (int c = 0; c < 16; c++) code_of[(uint8_t)LDBG_SW_LETTERS[c]] = (uint8_t)c;
    std::vector<uint8_t> qcode, scode;
    for (int64_t i = 0; i < n; i++) {
        if (query_off[i + 1] > query_off[i]) filter(queries + query_off[i], queries + query_off[i + 1], res->q_letters, qcode, code_of);
        if (subject_off[i + 1] > subject_off[i]) filter(subjects + subject_off[i], subjects + subject_off[i + 1], res->s_letters, scode, code_of);
        res->q_off[i + 1] = (int64_t)qcode.size(); res->s_off[i + 1] = (int64_t)scode.size();
    }

    // ---- per pair: refusals, the slices of the arena
    const int ws = host_wave_size();
    int lds_cells = SW_LDS_CELLS;
    if (const char* ev = getenv("LDBG_SW_LDS_CELLS")) lds_cells = (int)std::max<int64_t>(0, std::min<int64_t>(lds_cells, atoll(ev)));   // (tests: the HBM boundary row at small sizes)
    std::vector<uint8_t> run((size_t)n, 0);
    std::vector<int64_t> tb_off((size_t)n, 0), scr_off((size_t)n, -1), col_cap((size_t)n + 1, 0);
    struct Slice { int64_t first, n; };
    std::vector<Slice> slices;
    int64_t used = 0, max_slice = 0, budget = -1;
    for (int64_t i = 0; i < n; i++) {
        const int64_t Lq = res->q_off[i + 1] - res->q_off[i], Ls = res->s_off[i + 1] - res->s_off[i];
        col_cap[i + 1] = col_cap[i];
        if (Lq == 0 || Ls == 0) continue;                   // w or h is 1: nothing is positive, new SWResult()
        if (std::min(Lq, Ls) >= LDBG_SW_MIN_REFUSED || std::max(Lq, Ls) >= ((int64_t)1 << 30)) { res->status[i] = (uint8_t)LDBG_ERR_UNSUPPORTED; continue; }
        if (budget < 0) {
            if (rt::device_count() <= device || device < 0) throw StatusError(LDBG_ERR_HIP, "sw: no such device");
            rt::set_device(device);
            budget = arena_budget();
        }
        const int64_t tbb = (((Lq + ws - 1) / ws) * (Ls + ws - 1) * ws + 7) & ~(int64_t)7;
        const bool in_lds = Ls <= lds_cells;
        const int64_t need = tbb + (in_lds ? 0 : ((12 * Ls + 7) & ~(int64_t)7));
        if (need > budget) { res->status[i] = (uint8_t)LDBG_ERR_UNSUPPORTED; continue; }
        if (slices.empty() || used + need > budget) { slices.push_back({i, 0}); used = 0; }
        tb_off[i] = used;
        if (!in_lds) scr_off[i] = used + tbb;
        used += need;
        slices.back().n = i + 1 - slices.back().first;
        max_slice = std::max(max_slice, used);
        run[i] = 1;
        col_cap[i + 1] = col_cap[i] + Lq + Ls;
    }
    res->slices = (int)slices.size();
    if (slices.empty()) { profile_add("sw", 0.0); return res.release(); }      // nothing for the device: no allocation

    uint64_t rows[16];
    for (int q = 0; q < 16; q++) { rows[q] = 0; for (int s = 0; s < 16; s++) rows[q] |= (uint64_t)(NUC44[q][s] + 4) << (4 * s); }

    OwnStream own;
    rt::stream_t s = own.s;
    DevBlocks dev;
    auto up = [&](const void* h, size_t bytes) { void* d = dev.get<uint8_t>(std::max<size_t>(bytes, 1)); rt::h2d(d, h, bytes, s); return d; };
    const int64_t cap = col_cap[(size_t)n];
    SwArgs a{};
    a.lds_cells = lds_cells;
    a.rows = (const uint64_t*)up(rows, sizeof(rows));
    a.run = (const uint8_t*)up(run.data(), (size_t)n);
    a.q_off = (const int64_t*)up(res->q_off.data(), (size_t)(n + 1) * 8); a.qcode = (const uint8_t*)up(qcode.data(), qcode.size());
    a.s_off = (const int64_t*)up(res->s_off.data(), (size_t)(n + 1) * 8); a.scode = (const uint8_t*)up(scode.data(), scode.size());
    a.tb_off = (const int64_t*)up(tb_off.data(), (size_t)n * 8); a.scr_off = (const int64_t*)up(scr_off.data(), (size_t)n * 8);
    a.col_off = (const int64_t*)up(col_cap.data(), (size_t)(n + 1) * 8);
    a.arena = dev.get<uint8_t>((size_t)std::max<int64_t>(8, max_slice));
    a.cols = dev.get<uint8_t>((size_t)std::max<int64_t>(1, cap));
    a.out = dev.get<int32_t>((size_t)n * 8);
    rt::dmemset(a.out, 0, (size_t)n * 32, s);

    DevTimer tm;
    tm.begin(s);
    for (const Slice& sl : slices) {    // one after another on the stream: they share the arena
        a.first = sl.first; a.n = sl.n;
        LDBG_LAUNCH(k_sw, waves_for(sl.n), 64, s, a);
    }
    tm.end(s);
    std::vector<int32_t> out((size_t)n * 8);
    std::vector<uint8_t> cols((size_t)std::max<int64_t>(1, cap));
    rt::d2h(out.data(), a.out, (size_t)n * 32, s);
    rt::d2h(cols.data(), a.cols, (size_t)cap, s);
    rt::stream_sync(s);
    profile_add("sw", tm.ms);

    for (int64_t i = 0; i < n; i++) {
        res->col_off[i + 1] = res->col_off[i];
        if (!run[i]) continue;
        const int32_t* o = out.data() + i * 8;
        res->score[i] = (double)o[0] / 2.0;
        res->end_q[i] = o[1]; res->end_s[i] = o[2]; res->begin_q[i] = o[3]; res->begin_s[i] = o[4];
        res->aligned_len[i] = o[6]; res->edits[i] = o[7];
        res->col_off[i + 1] += o[5];
        res->cols.insert(res->cols.end(), cols.begin() + (col_cap[i + 1] - o[5]), cols.begin() + col_cap[i + 1]);
    }
    return res.release();
}

}  // namespace ldbg
