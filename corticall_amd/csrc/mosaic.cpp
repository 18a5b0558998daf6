// Tesserae.align of n problems on the device (mosaic.h): Tesserae.java:95-382.
//   k_mosaic: one wavefront per problem.  The cells of a column are the targets' positions laid end to end (S = sum of the target lengths).
//     Per column of the query: lanes stride over the cells for M and I (independent given the previous column and its maximum), a
//     butterfly takes the column's maximum with Java's tie order (first sequence, first position, M before I), the D chain runs in
//     chunks of cells with carries between the lanes (mo_d_chunks), and the column's traceback bytes leave coalesced along the cell axis.  Then lane 0 walks the traceback, every step
//     through Java's encode and decode in double (mosaic.h).
//   Two rolling columns of M, I, D and the column's traceback bytes (49 B per cell) live in LDS when they fit MOSAIC_LDS_BYTES, in a
//   per-problem HBM scratch otherwise.
// Double-precision adds and compares only; no multiply stands beside an add except in mosaic_tb_decode, which switches contraction off.
// The TEST-ONLY host simulation runs the kernel as it is.
#include "mosaic.h"

#include <math.h>

#include <memory>

#include "devmem.h"
#include "graph.h"
#include "wavescan.h"

namespace ldbg {

namespace {

#define MOSAIC_SMALL (-1e32)
#define MOSAIC_LDS_BYTES 40960          // per workgroup (one wavefront): four problems beside one another on a compute unit
#define MOSAIC_CELL_BYTES 49            // 2 columns x (M, I, D) x 8 B + 1 traceback byte
#define MOSAIC_NONE 0xFFFFFFFFu
#define MOSAIC_BATCH 4                  // cells a lane loads ahead of computing them (the LDS bounds the occupancy, not the registers)

struct MosaicConsts { double ldel, leps, lrho, lterm, lpiM, lpiI, lmm, lgm, ldm, lsm[25], lsi[5]; };

struct MosaicArgs {
    MosaicConsts k;
    int64_t first, n;                   // the slice: problems [first, first + n) of the batch
    int lds_cells;                      // a problem of at most this many cells keeps its columns in LDS
    const int64_t* q_off; const uint8_t* qcode;                          // convert() of the queries' bytes
    const int64_t* t_first; const int64_t* t_off; const uint8_t* tcode;  // convert() of the targets' bytes; bit 7: first cell of its target
    const double* lsize; const double* div; const int32_t* maxl;
    uint8_t* status;                    // [n of the batch] in: not LDBG_OK = skip; out: LDBG_ERR_UNSUPPORTED where the traceback leaves Java's arrays
    const int64_t* tb_off;              // [n of the batch] byte offset of the problem's l1 x S traceback bytes in the arena
    const int64_t* scr_off;             // the same for its columns (49 B x S, 8-aligned) where they are not in LDS
    uint8_t* arena;
    int32_t* rec;                       // [sum of l1][3] who, state, pos of the maximum of each column (the recombination source of the next)
    const int64_t* path_cap;            // [n + 1] entries: 2 maxl + 1 per problem
    int32_t* pcopy; int32_t* pstate; int32_t* ppos; int32_t* path_cp; double* llk;
};

template <bool L> LDBG_DEV double mo_ld(const double* p, int i) { if (L) return LDBG_LDS(const double, p)[i]; return LDBG_GLOBAL(const double, p)[i]; }
template <bool L> LDBG_DEV void mo_st(double* p, int i, double v) { if (L) LDBG_LDS(double, p)[i] = v; else LDBG_GLOBAL(double, p)[i] = v; }
template <bool L> LDBG_DEV uint8_t mo_ldb(const uint8_t* p, int i) { if (L) return LDBG_LDS(const uint8_t, p)[i]; return LDBG_GLOBAL(const uint8_t, p)[i]; }
template <bool L> LDBG_DEV void mo_stb(uint8_t* p, int i, uint8_t v) { if (L) LDBG_LDS(uint8_t, p)[i] = v; else LDBG_GLOBAL(uint8_t, p)[i] = v; }

LDBG_DEV double mo_from_bits(uint64_t b) { double d; __builtin_memcpy(&d, &b, 8); return d; }
LDBG_DEV uint64_t mo_bits(double d) { uint64_t b; __builtin_memcpy(&b, &d, 8); return b; }

// the maximum of (v, idx) over the wavefront: the greater value, at equal values the smaller index (cell x 2 + state - 1: Java's loop order)
LDBG_DEV void mo_wave_max(double& v, uint32_t& idx) {
    for (int m = wave_size() >> 1; m > 0; m >>= 1) {
        const double ov = mo_from_bits(wave_shfl_xor_u64(mo_bits(v), m));
        const uint32_t oi = (uint32_t)wave_shfl_xor_u64(idx, m);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
}

// the target (0-based) that owns cell c: the last one that starts at or before c (a target of length 0 owns none)
LDBG_DEV int mo_target_of(const int64_t* toff, int nt, int64_t c) {
    int lo = 0, hi = nt;                // first t in [0, nt] with toff[t] - toff[0] > c
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (toff[mid] - toff[0] > c) hi = mid; else lo = mid + 1; }
    return lo - 1;
}

// D of column q (Tesserae.java:234-240, 307-316), in chunks.  D[p] = max(M[p-1] + ldel, D[p-1] + leps) is the maximum over j < p of
// "M[j] + ldel, then p - 1 - j additions of leps one after the other": adding a constant is monotone and max is exact, so the maximum may
// be taken in any order as long as every chain adds in sequence.  Each lane owns a run of `run` consecutive cells (an odd number, meant to
// spread the lanes' LDS addresses over the banks; not measured) and chains it from nothing; then the value at the end of every run is carried into
// the next run, again by sequential additions, for as long as it improves a cell (a carry that is not greater at one cell is not greater
// at any later one), round after round until a ballot shows that no run's last cell changed.  Bit 4 of the traceback byte is
// D[p-1] + leps > M[p-1] + ldel: set by the local chain, and by a carry wherever it improves a cell.
template <bool L>
LDBG_DEV void mo_d_chunks(const MosaicConsts& k, const uint8_t* tc, int S, bool first_column, const double* Mc, double* Dc, uint8_t* tbcol) {
    const int ws = LDBG_WS, lane = wave_lane();
    const int run = ((S + ws - 1) / ws) | 1;
    const int s = std::min(S, lane * run), e = std::min(S, s + run);
    const double none = -__builtin_inf();
    double d = none;                    // (-inf + leps = -inf: no chain comes in from the left)
    for (int cb = s; cb < e; cb += 2 * MOSAIC_BATCH) {      // (the chain's operands that do not depend on it are loaded ahead of it, a batch at a time)
        uint8_t tcs[2 * MOSAIC_BATCH]; double pm[2 * MOSAIC_BATCH];
#pragma unroll
        for (int u = 0; u < 2 * MOSAIC_BATCH; u++) {
            const int c = cb + u;
            if (c >= e) break;
            tcs[u] = tc[c];
            pm[u] = (tcs[u] & 0x80u) ? MOSAIC_SMALL : mo_ld<L>(Mc, c - 1);
        }
#pragma unroll
        for (int u = 0; u < 2 * MOSAIC_BATCH; u++) {
            const int c = cb + u;
            if (c >= e) break;
            bool b = false;
            if (tcs[u] & 0x80u) {       // pos_seq = 1: M[0] and D[0] are SMALL in the first column; later columns leave vt_d[seq][1][.] SMALL (:307)
                if (first_column) { const double c0 = MOSAIC_SMALL + k.ldel, c1 = MOSAIC_SMALL + k.leps; b = c0 < c1; d = b ? c1 : c0; }
                else d = MOSAIC_SMALL;
            } else {
                const double c0 = pm[u] + k.ldel, c1 = d + k.leps;
                b = c0 < c1;            // argmax: the first maximum
                d = b ? c1 : c0;
            }
            mo_st<L>(Dc, c, d);
            if (b) mo_stb<L>(tbcol, c, (uint8_t)(mo_ldb<L>(tbcol, c) | 16u));
        }
    }
    double last = e > s ? d : none;
    for (;;) {
        double v = mo_from_bits(wave_shfl_u64(mo_bits(last), lane - 1));
        if (lane == 0) v = none;
        bool changed = false;
        for (int c = s; c < e; c++) {
            if (tc[c] & 0x80u) break;
            v += k.leps;
            if (!(v > mo_ld<L>(Dc, c))) break;
            mo_st<L>(Dc, c, v);
            mo_stb<L>(tbcol, c, (uint8_t)(mo_ldb<L>(tbcol, c) | 16u));
            if (c == e - 1) { last = v; changed = true; }
        }
        if (wave_ballot(changed) == 0ull) break;
    }
}

template <bool L>
LDBG_DEV void mo_problem(const MosaicArgs& a, int64_t i, double* cols, uint8_t* tbcol) {
    const int ws = LDBG_WS, lane = wave_lane();
    const MosaicConsts& k = a.k;
    const int64_t q0 = a.q_off[i], tf = a.t_first[i];
    const int l1 = (int)(a.q_off[i + 1] - q0), nt = (int)(a.t_first[i + 1] - tf);
    const int64_t* toff = a.t_off + tf;
    const int S = (int)(toff[nt] - toff[0]);
    const uint8_t* tc = a.tcode + toff[0];
    const uint8_t* qc = a.qcode + q0;
    const double lsz = a.lsize[i];
    uint8_t* tb = a.arena + a.tb_off[i];
    int32_t* rec = a.rec + q0 * 3;
    int cur_who = 0, cur_state = 0, cur_pos = 0;          // who_max, state_max, pos_max (lane 0's are read)
    int n_who = 0, n_state = 0, n_pos = 0;                // who_max_n, state_max_n, pos_max_n
    double max_r = MOSAIC_SMALL;
    for (int q = 1; q <= l1; q++) {
        double* Mc = cols + (size_t)((q & 1) * 3) * S; double* Ic = Mc + S; double* Dc = Ic + S;
        const double* Mp = cols + (size_t)(((q - 1) & 1) * 3) * S; const double* Ip = Mp + S; const double* Dp = Ip + S;
        const int qq = qc[q - 1];
        const double lsi_q = k.lsi[qq];
        double best; uint32_t bidx = MOSAIC_NONE;
        if (q == 1) {                   // :223-259
            best = MOSAIC_SMALL;
            for (int c = lane; c < S; c += ws) {
                double m = k.lpiM - lsz; m += k.lsm[qq * 5 + (tc[c] & 7)];
                double v = k.lpiI - lsz; v += lsi_q;
                mo_st<L>(Mc, c, m); mo_st<L>(Ic, c, v); mo_stb<L>(tbcol, c, 0);
                if (m > best) { best = m; bidx = 2u * (uint32_t)c; }
                if (v > best) { best = v; bidx = 2u * (uint32_t)c + 1u; }
            }
        } else {                        // :261-341
            const double rec_m = max_r + k.lrho + k.lpiM - lsz, rec_i = max_r + k.lrho + k.lpiI - lsz;
            best = MOSAIC_SMALL + max_r;
            // MOSAIC_BATCH cells per lane at a time: their loads are issued together, ahead of the first cell's stores
            for (int cb = lane; cb < S; cb += MOSAIC_BATCH * ws) {
              uint8_t tcs[MOSAIC_BATCH]; double pm[MOSAIC_BATCH], pi[MOSAIC_BATCH], pd[MOSAIC_BATCH], hm[MOSAIC_BATCH], hi[MOSAIC_BATCH];
#pragma unroll
              for (int u = 0; u < MOSAIC_BATCH; u++) {
                const int c = cb + u * ws;
                if (c >= S) break;
                tcs[u] = tc[c];
                const bool head = (tcs[u] & 0x80u) != 0;
                pm[u] = head ? MOSAIC_SMALL : mo_ld<L>(Mp, c - 1);
                pi[u] = head ? MOSAIC_SMALL : mo_ld<L>(Ip, c - 1);
                pd[u] = head ? MOSAIC_SMALL : mo_ld<L>(Dp, c - 1);
                hm[u] = mo_ld<L>(Mp, c); hi[u] = mo_ld<L>(Ip, c);
              }
#pragma unroll
              for (int u = 0; u < MOSAIC_BATCH; u++) {
                const int c = cb + u * ws;
                if (c >= S) break;
                const uint8_t tcc = tcs[u];
                const double a0 = pm[u] + k.lmm;
                const double a1 = pi[u] + k.lgm;
                const double a2 = pd[u] + k.ldm;
                int im = 0; double am = a0;
                if (am < a1) { im = 1; am = a1; }
                if (am < a2) { im = 2; am = a2; }
                double m = rec_m; uint8_t bits = 0;
                if (am > m) { m = am; bits = (uint8_t)(im + 1); }
                m += k.lsm[qq * 5 + (tcc & 7)];
                const double b0 = hm[u] + k.ldel, b1 = hi[u] + k.leps;
                const int ii = b0 < b1 ? 1 : 0;
                const double bm = ii ? b1 : b0;
                double v = rec_i;
                if (bm > v) { v = bm; bits |= (uint8_t)((ii + 1) << 2); }
                v += lsi_q;
                mo_st<L>(Mc, c, m); mo_st<L>(Ic, c, v); mo_stb<L>(tbcol, c, bits);
                if (m > best) { best = m; bidx = 2u * (uint32_t)c; }
                if (v > best) { best = v; bidx = 2u * (uint32_t)c + 1u; }
              }
            }
        }
        mo_wave_max(best, bidx);
        max_r = best;
        if (lane == 0) {
            // column 1 writes who_max itself (:242-253); a later column writes who_max_n and copies it at its end (:318-340), so a column
            // without a cell above SMALL + max_r hands on what who_max_n held, zeros at first, not the previous column's winner
            int& w = q == 1 ? cur_who : n_who; int& st = q == 1 ? cur_state : n_state; int& p = q == 1 ? cur_pos : n_pos;
            if (bidx != MOSAIC_NONE) {
                const int64_t c = (int64_t)(bidx >> 1);
                const int t = mo_target_of(toff, nt, c);
                w = t + 2; st = (int)(bidx & 1u) + 1; p = (int)(c - (toff[t] - toff[0])) + 1;
            }
            if (q > 1) { cur_who = n_who; cur_state = n_state; cur_pos = n_pos; }
            rec[3 * (q - 1)] = cur_who; rec[3 * (q - 1) + 1] = cur_state; rec[3 * (q - 1) + 2] = cur_pos;
        }
        wave_fence();                   // M of this column is read by the chains' lanes
        if (q == 1 || q < l1) mo_d_chunks<L>(k, tc, S, q == 1, Mc, Dc, tbcol);
        wave_fence();
        uint8_t* out = tb + (size_t)(q - 1) * (size_t)S;
        for (int c = lane; c < S; c += ws) LDBG_GLOBAL(uint8_t, out)[c] = mo_ldb<L>(tbcol, c);
    }
    wave_fence();
    if (lane != 0) return;
    // ---- :343-382
    a.llk[i] = max_r + k.lterm;
    const int maxl = a.maxl[i], nseq = nt + 1;
    const double div = a.div[i];
    const int64_t po = a.path_cap[i];
    int cp = 2 * maxl;
    int who = cur_who, state = cur_state, pos = cur_pos;
    a.pcopy[po + cp] = who; a.pstate[po + cp] = state; a.ppos[po + cp] = pos;
    double tbn = 0.0;
    int q = l1;
    bool thrown = false;
    while (q >= 1) {
        if (state >= 1 && state <= 3) {
            if (who < 0 || who > nseq || pos < 0 || pos > maxl) { thrown = true; break; }      // ArrayIndexOutOfBoundsException
            tbn = 0.0;                  // a cell the loops never wrote: the query's rows, position 0, positions past a target's end
            const int len = who >= 2 ? (int)(toff[who - 1] - toff[who - 2]) : 0;
            if (who >= 2 && pos >= 1 && pos <= len && q >= 2 && state != 3) {
                const int c = (int)(toff[who - 2] - toff[0]) + pos - 1;
                const uint8_t b = tb[(size_t)(q - 1) * (size_t)S + c];
                const int bits = state == 1 ? (b & 3) : ((b >> 2) & 3);
                if (bits == 0) tbn = mosaic_tb_encode(rec[3 * (q - 2)] * 10 + rec[3 * (q - 2) + 1], rec[3 * (q - 2) + 2], div);
                else tbn = mosaic_tb_encode(who * 10 + bits, state == 1 ? pos - 1 : pos, div);
            } else if (who >= 2 && pos >= 1 && pos <= len && state == 3 && (q == 1 || (q < l1 && pos > 1))) {
                const int c = (int)(toff[who - 2] - toff[0]) + pos - 1;
                const uint8_t b = tb[(size_t)(q - 1) * (size_t)S + c];
                tbn = mosaic_tb_encode(who * 10 + ((b >> 4) & 1) * 2 + 1, pos - 1, div);
            }
        }
        int w2, s2, p2;
        mosaic_tb_decode(tbn, div, &w2, &s2, &p2);
        cp--;
        if (cp < 0) { thrown = true; break; }
        a.pcopy[po + cp] = w2; a.pstate[po + cp] = s2; a.ppos[po + cp] = p2;
        const int before = state;
        who = w2; state = s2; pos = p2;
        if (before != 3) q--;
    }
    cp++;
    a.path_cp[i] = cp;
    if (thrown) a.status[i] = (uint8_t)LDBG_ERR_UNSUPPORTED;
}

LDBG_WAVE_KERNEL void k_mosaic(MosaicArgs a) {
#ifndef LDBG_HOSTSIM
    __shared__ double lds[MOSAIC_LDS_BYTES / 8];
#else
    static double lds[MOSAIC_LDS_BYTES / 8];          // (one simulated wavefront at a time: rt.h)
#endif
    const int ws = LDBG_WS;
    const int64_t wave = global_tid() / ws, nwaves = global_nthreads() / ws;
    for (int64_t j = wave_uniform_i64(wave); j < a.n; j += nwaves) {
        const int64_t i = a.first + j;
        if (a.status[i] != LDBG_OK) continue;
        const int64_t tf = a.t_first[i];
        const int64_t S = a.t_off[a.t_first[i + 1]] - a.t_off[tf];
        if (S <= a.lds_cells) {
            mo_problem<true>(a, i, lds, (uint8_t*)(lds + 6 * S));
        } else {
            double* cols = (double*)(a.arena + a.scr_off[i]);
            mo_problem<false>(a, i, cols, (uint8_t*)(cols + 6 * S));
        }
        wave_fence();                   // the next problem's first column overwrites what this one's lanes may still read
    }
}

LDBG_KERNEL void k_mosaic_roundtrip(double div, int64_t n, const int32_t* who, const int32_t* state, const int32_t* pos, int32_t* out) {
    for (int64_t i = global_tid(); i < n; i += global_nthreads()) {
        int w, s, p;
        mosaic_tb_decode(mosaic_tb_encode(who[i] * 10 + state[i], pos[i], div), div, &w, &s, &p);
        out[3 * i] = w; out[3 * i + 1] = s; out[3 * i + 2] = p;
    }
}

int convert(char c) {                   // Tesserae.java:497-506
    switch (c) { case 'T': return 1; case 'C': return 2; case 'A': return 3; case 'G': return 4; }
    return 0;
}

void check_offsets(const int64_t* off, int64_t n, const char* what) {
    if (!off) throw StatusError(LDBG_ERR_ARG, std::string("mosaic: null ") + what);
    if (off[0] < 0) throw StatusError(LDBG_ERR_ARG, std::string("mosaic: negative ") + what);
    for (int64_t i = 0; i < n; i++)
        if (off[i + 1] < off[i]) throw StatusError(LDBG_ERR_ARG, std::string("mosaic: decreasing ") + what);
}

int64_t arena_budget() {
    if (const char* ev = getenv("LDBG_MOSAIC_ARENA_BYTES")) return std::max<int64_t>(1, atoll(ev));
    size_t free_b = 0, total_b = 0;
    rt::mem_info(&free_b, &total_b);
    return std::max<int64_t>(1, (int64_t)(free_b / 4));
}

}  // namespace

MosaicResult* mosaic_align_batch(int device, const ldbg_mosaic_params& p, int64_t n, const char* queries, const int64_t* query_off, const int64_t* target_first,
                                 const char* targets, const int64_t* target_off) {
    if (n < 0) throw StatusError(LDBG_ERR_ARG, "mosaic: n < 0");
    std::unique_ptr<MosaicResult> res(new MosaicResult);
    res->n = n;
    res->status.assign((size_t)n, (uint8_t)LDBG_OK);
    res->llk.assign((size_t)n, 0.0);
    res->path_off.assign((size_t)n + 1, 0);
    if (n == 0) { profile_add("mosaic", 0.0); return res.release(); }
    check_offsets(query_off, n, "query offsets");
    check_offsets(target_first, n, "target ranges");
    if (target_first[0] != 0) throw StatusError(LDBG_ERR_ARG, "mosaic: the first problem's targets do not start at 0");
    const int64_t n_targets = target_first[n];
    check_offsets(target_off, n_targets, "target offsets");
    const int64_t qbytes = query_off[n] - query_off[0], tbytes = target_off[n_targets] - target_off[0];
    if ((qbytes > 0 && !queries) || (tbytes > 0 && !targets)) throw StatusError(LDBG_ERR_ARG, "mosaic: null sequences");
    if (rt::device_count() <= device || device < 0) throw StatusError(LDBG_ERR_HIP, "mosaic: no such device");
    rt::set_device(device);

    // ---- Tesserae.initialize (:105-168): the logs, once
    MosaicArgs a{};
    a.k.ldel = log(p.del); a.k.leps = log(p.eps); a.k.lrho = log(p.rho); a.k.lterm = log(p.term);
    const double piM = 0.75, piI = 1 - piM;
    a.k.lpiM = log(piM); a.k.lpiI = log(piI);
    a.k.lmm = log(1 - 2 * p.del - p.rho - p.term); a.k.lgm = log(1 - p.eps - p.rho - p.term); a.k.ldm = log(1 - p.eps);
    static const double emiss[5][5] = {{0.2, 0.2, 0.2, 0.2, 0.2}, {0.2, 0.9, 0.05, 0.025, 0.025}, {0.2, 0.05, 0.9, 0.025, 0.025},
                                       {0.2, 0.025, 0.025, 0.9, 0.05}, {0.2, 0.025, 0.025, 0.05, 0.9}};
    for (int x = 0; x < 5; x++) { a.k.lsi[x] = log(0.2); for (int y = 0; y < 5; y++) a.k.lsm[x * 5 + y] = log(emiss[x][y]); }

    // ---- per problem: sizes, refusals, the slices of the arena
    const int64_t budget = arena_budget();
    int lds_cells = MOSAIC_LDS_BYTES / MOSAIC_CELL_BYTES;
    if (const char* ev = getenv("LDBG_MOSAIC_LDS_CELLS")) lds_cells = (int)std::max<int64_t>(0, std::min<int64_t>(lds_cells, atoll(ev)));   // (tests: the HBM columns at small sizes)
    std::vector<double> lsize((size_t)n), div((size_t)n);
    std::vector<int32_t> maxl((size_t)n);
    std::vector<int64_t> tb_off((size_t)n, 0), scr_off((size_t)n, -1), path_cap((size_t)n + 1, 0), q_rel((size_t)n + 1), t_rel((size_t)n_targets + 1);
    for (int64_t i = 0; i <= n; i++) q_rel[(size_t)i] = query_off[i] - query_off[0];
    for (int64_t t = 0; t <= n_targets; t++) t_rel[(size_t)t] = target_off[t] - target_off[0];
    struct Slice { int64_t first, n, bytes; };
    std::vector<Slice> slices;
    int64_t used = 0, max_slice = 0;
    for (int64_t i = 0; i < n; i++) {
        const int64_t l1 = q_rel[i + 1] - q_rel[i], nt = target_first[i + 1] - target_first[i];
        const int64_t S = t_rel[target_first[i + 1]] - t_rel[target_first[i]];
        int64_t ml = l1;
        for (int64_t t = target_first[i]; t < target_first[i + 1]; t++) ml = std::max(ml, t_rel[t + 1] - t_rel[t]);
        path_cap[i + 1] = path_cap[i];
        // refused: Java throws on an empty query or no targets; with no target base at all its track builder does; maxl <= 2 packs garbage
        if (l1 == 0 || nt == 0 || S == 0 || ml <= 2 || ml > (1 << 28) || S > (1 << 30)) { res->status[i] = (uint8_t)LDBG_ERR_UNSUPPORTED; continue; }
        int64_t need = (l1 * S + 7) & ~(int64_t)7;
        const bool in_lds = S <= lds_cells;
        if (!in_lds) need += (MOSAIC_CELL_BYTES * S + 7) & ~(int64_t)7;
        if (need > budget) { res->status[i] = (uint8_t)LDBG_ERR_UNSUPPORTED; continue; }
        if (slices.empty() || used + need > budget) { slices.push_back({i, 0, 0}); used = 0; }
        tb_off[i] = used;
        if (!in_lds) scr_off[i] = used + ((l1 * S + 7) & ~(int64_t)7);
        used += need;
        slices.back().n = i + 1 - slices.back().first;
        slices.back().bytes = used;
        max_slice = std::max(max_slice, used);
        maxl[i] = (int32_t)ml;
        lsize[i] = log((double)S);                                     // :192-198
        div[i] = pow(10.0, (double)(int)log((double)ml));              // :144-145
        path_cap[i + 1] = path_cap[i] + 2 * ml + 1;
    }
    res->slices = (int)slices.size();

    // ---- convert() of every base
    std::vector<uint8_t> qcode((size_t)std::max<int64_t>(1, qbytes)), tcode((size_t)std::max<int64_t>(1, tbytes));
    for (int64_t b = 0; b < qbytes; b++) qcode[(size_t)b] = (uint8_t)convert(queries[query_off[0] + b]);
    for (int64_t b = 0; b < tbytes; b++) tcode[(size_t)b] = (uint8_t)convert(targets[target_off[0] + b]);
    for (int64_t t = 0; t < n_targets; t++) if (t_rel[t + 1] > t_rel[t]) tcode[(size_t)t_rel[t]] |= 0x80u;

    OwnStream own;
    rt::stream_t s = own.s;
    DevBlocks dev;
    auto up = [&](const void* h, size_t bytes) { void* d = dev.get<uint8_t>(std::max<size_t>(bytes, 1)); rt::h2d(d, h, bytes, s); return d; };
    const int64_t cap = path_cap[(size_t)n];
    a.lds_cells = lds_cells;
    a.q_off = (const int64_t*)up(q_rel.data(), q_rel.size() * 8); a.qcode = (const uint8_t*)up(qcode.data(), qcode.size());
    a.t_first = (const int64_t*)up(target_first, (size_t)(n + 1) * 8); a.t_off = (const int64_t*)up(t_rel.data(), t_rel.size() * 8);
    a.tcode = (const uint8_t*)up(tcode.data(), tcode.size());
    a.lsize = (const double*)up(lsize.data(), (size_t)n * 8); a.div = (const double*)up(div.data(), (size_t)n * 8); a.maxl = (const int32_t*)up(maxl.data(), (size_t)n * 4);
    a.status = (uint8_t*)up(res->status.data(), (size_t)n);
    a.tb_off = (const int64_t*)up(tb_off.data(), (size_t)n * 8); a.scr_off = (const int64_t*)up(scr_off.data(), (size_t)n * 8);
    a.path_cap = (const int64_t*)up(path_cap.data(), (size_t)(n + 1) * 8);
    a.arena = dev.get<uint8_t>((size_t)std::max<int64_t>(8, max_slice));
    a.rec = dev.get<int32_t>((size_t)std::max<int64_t>(1, qbytes) * 3);
    a.pcopy = dev.get<int32_t>((size_t)std::max<int64_t>(1, cap)); a.pstate = dev.get<int32_t>((size_t)std::max<int64_t>(1, cap));
    a.ppos = dev.get<int32_t>((size_t)std::max<int64_t>(1, cap));
    a.path_cp = dev.get<int32_t>((size_t)n); a.llk = dev.get<double>((size_t)n);
    rt::dmemset(a.path_cp, 0, (size_t)n * 4, s); rt::dmemset(a.llk, 0, (size_t)n * 8, s);

    DevTimer tm;
    tm.begin(s);
    for (const Slice& sl : slices) {    // one after another on the stream: they share the arena
        a.first = sl.first; a.n = sl.n;
        LDBG_LAUNCH(k_mosaic, waves_for(sl.n), 64, s, a);
    }
    tm.end(s);
    std::vector<int32_t> hc((size_t)std::max<int64_t>(1, cap)), hs(hc.size()), hp(hc.size()), cp((size_t)n);
    rt::d2h(hc.data(), a.pcopy, (size_t)cap * 4, s); rt::d2h(hs.data(), a.pstate, (size_t)cap * 4, s); rt::d2h(hp.data(), a.ppos, (size_t)cap * 4, s);
    rt::d2h(cp.data(), a.path_cp, (size_t)n * 4, s); rt::d2h(res->llk.data(), a.llk, (size_t)n * 8, s);
    rt::d2h(res->status.data(), a.status, (size_t)n, s);
    rt::stream_sync(s);
    profile_add("mosaic", tm.ms);

    // ---- maxpath_*[cp .. 2 maxl] of every problem, end to end
    for (int64_t i = 0; i < n; i++) {
        res->path_off[i + 1] = res->path_off[i];
        if (res->status[i] != LDBG_OK) { res->llk[i] = 0.0; continue; }
        const int64_t len = 2 * (int64_t)maxl[i] + 1 - cp[i];
        res->path_off[i + 1] += len;
        const int64_t from = path_cap[i] + cp[i];
        res->copy.insert(res->copy.end(), hc.begin() + from, hc.begin() + from + len);
        res->state.insert(res->state.end(), hs.begin() + from, hs.begin() + from + len);
        res->pos.insert(res->pos.end(), hp.begin() + from, hp.begin() + from + len);
    }
    return res.release();
}

void mosaic_tb_roundtrip(int device, double div, int64_t n, const int32_t* who, const int32_t* state, const int32_t* pos, int32_t* out) {
    if (n < 0 || (n > 0 && (!who || !state || !pos || !out))) throw StatusError(LDBG_ERR_ARG, "mosaic roundtrip: bad arguments");
    if (n == 0) return;
    if (rt::device_count() <= device || device < 0) throw StatusError(LDBG_ERR_HIP, "mosaic: no such device");
    rt::set_device(device);
    OwnStream own;
    DevBlocks dev;
    int32_t* dw = dev.get<int32_t>((size_t)n); int32_t* ds = dev.get<int32_t>((size_t)n); int32_t* dp = dev.get<int32_t>((size_t)n); int32_t* dout = dev.get<int32_t>((size_t)n * 3);
    rt::h2d(dw, who, (size_t)n * 4, own.s); rt::h2d(ds, state, (size_t)n * 4, own.s); rt::h2d(dp, pos, (size_t)n * 4, own.s);
    LDBG_LAUNCH(k_mosaic_roundtrip, grid_for(n), 256, own.s, div, n, (const int32_t*)dw, (const int32_t*)ds, (const int32_t*)dp, dout);
    rt::d2h(out, dout, (size_t)n * 12, own.s);
    rt::stream_sync(own.s);
}

}  // namespace ldbg
