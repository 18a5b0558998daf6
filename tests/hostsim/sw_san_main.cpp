// TEST-ONLY stand-alone program over the host simulation of libldbg (make -C corticall_amd/csrc hostsim-san-sw): runs
// ldbg_sw_align_batch on the boundary-length pairs — query lengths 0, 1, 2, 63, 64, 65, 127, 128, 129 against subject lengths 0, 1, 2, 63,
// 64, 65, 129, a long deletion and a long insertion, letters that filter drops or turns into X, a refused pair — with 1 lane and 64 lanes
// in lock step, the boundary row in (simulated) LDS and in the HBM scratch, the arena whole and in slices, so that the kernel of sw.cpp
// runs under AddressSanitizer and UBSan without loading the library into another process.  Checks what needs no second implementation:
// the values of DESIGN.md §20's table, that every variant of a run returns the same bytes, and that an alignment is well formed (its
// columns lead from the begin cell to the end cell, its counts follow from them).  Prints one line per case; exits non-zero on an error.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/ldbg.h"

extern "C" void ldbg_hostsim_set_lanes(int n);

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_rng >> 33); }
static std::string rand_seq(size_t n) { std::string s(n, 'A'); for (char& c : s) c = "ACGT"[rnd() & 3u]; return s; }

struct Pair { std::string q, s; };
struct Result {
    std::vector<uint8_t> status, cols, ql, sl;
    std::vector<double> score;
    std::vector<int32_t> end_q, end_s, begin_q, begin_s, alen, edits;
    std::vector<int64_t> col_off, q_off, s_off;
};

static int g_fail = 0;
#define EXPECT(c, ...) do { if (!(c)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); g_fail++; } } while (0)

static bool run(const std::vector<Pair>& ps, Result& r) {
    std::string q, s;
    std::vector<int64_t> qoff{0}, soff{0};
    for (const Pair& p : ps) { q += p.q; qoff.push_back((int64_t)q.size()); s += p.s; soff.push_back((int64_t)s.size()); }
    ldbg_sw_result* h = nullptr;
    if (ldbg_sw_align_batch(0, (int64_t)ps.size(), q.data(), qoff.data(), s.data(), soff.data(), &h) != LDBG_OK) {
        printf("FAIL align_batch: %s\n", ldbg_last_error());
        g_fail++;
        return false;
    }
    int64_t n = 0, nc = 0, nq = 0, ns = 0;
    ldbg_sw_result_sizes(h, &n, &nc, &nq, &ns);
    r.status.assign((size_t)n, 0); r.score.assign((size_t)n, 0);
    for (std::vector<int32_t>* v : {&r.end_q, &r.end_s, &r.begin_q, &r.begin_s, &r.alen, &r.edits}) v->assign((size_t)n, 0);
    for (std::vector<int64_t>* v : {&r.col_off, &r.q_off, &r.s_off}) v->assign((size_t)n + 1, 0);
    r.cols.assign((size_t)nc + 1, 0); r.ql.assign((size_t)nq + 1, 0); r.sl.assign((size_t)ns + 1, 0);
    const ldbg_sw_arrays a{r.status.data(), r.score.data(), r.end_q.data(), r.end_s.data(), r.begin_q.data(), r.begin_s.data(), r.alen.data(), r.edits.data(),
                           r.col_off.data(), r.cols.data(), r.q_off.data(), r.ql.data(), r.s_off.data(), r.sl.data()};
    ldbg_sw_result_get(h, &a);
    ldbg_sw_result_free(h);
    r.cols.resize((size_t)nc); r.ql.resize((size_t)nq); r.sl.resize((size_t)ns);
    return true;
}

static bool same(const Result& a, const Result& b) {
    return a.status == b.status && a.cols == b.cols && a.ql == b.ql && a.sl == b.sl && a.end_q == b.end_q && a.end_s == b.end_s && a.begin_q == b.begin_q &&
           a.begin_s == b.begin_s && a.alen == b.alen && a.edits == b.edits && a.col_off == b.col_off && a.q_off == b.q_off && a.s_off == b.s_off &&
           (a.score.empty() || memcmp(a.score.data(), b.score.data(), a.score.size() * 8) == 0);
}

static void well_formed(const Result& r, size_t refused, const char* what) {
    for (size_t i = 0; i < r.status.size(); i++) {
        EXPECT((r.status[i] != LDBG_OK) == (i == refused), "%s pair %zu: status %d", what, i, (int)r.status[i]);
        const int64_t lq = r.q_off[i + 1] - r.q_off[i], ls = r.s_off[i + 1] - r.s_off[i], nc = r.col_off[i + 1] - r.col_off[i];
        if (r.end_q[i] < 0) {
            EXPECT(nc == 0 && r.alen[i] == 0 && r.edits[i] == 0 && r.score[i] == -1.0 && r.begin_q[i] == -1, "%s pair %zu: an empty result with values", what, i);
            continue;
        }
        int64_t x = r.begin_q[i] - 1, y = r.begin_s[i] - 1, gaps = 0, differ = 0;
        for (int64_t c = r.col_off[i]; c < r.col_off[i + 1]; c++) {
            const int k = r.cols[(size_t)c];
            EXPECT(k <= 2, "%s pair %zu: column %d", what, i, k);
            if (k == 0) { if (x < lq && y < ls && r.ql[(size_t)(r.q_off[i] + x)] != r.sl[(size_t)(r.s_off[i] + y)]) differ++; x++; y++; }
            else if (k == 1) { y++; gaps++; } else { x++; gaps++; }
        }
        EXPECT(x == r.end_q[i] && y == r.end_s[i] && x <= lq && y <= ls, "%s pair %zu: the columns end at (%lld, %lld), the maximum is (%d, %d)", what, i, (long long)x,
               (long long)y, r.end_q[i], r.end_s[i]);
        const int64_t ends = (r.begin_q[i] - 1) + (r.begin_s[i] - 1) + (lq - r.end_q[i]) + (ls - r.end_s[i]);
        EXPECT(r.alen[i] == nc + ends && r.edits[i] == gaps + differ + ends, "%s pair %zu: aligned_len %d edits %d", what, i, r.alen[i], r.edits[i]);
        EXPECT(r.score[i] > 0 && r.score[i] * 2 == (double)(int64_t)(r.score[i] * 2), "%s pair %zu: score %g", what, i, r.score[i]);
    }
}

int main() {
    std::vector<Pair> ps;
    ps.push_back({"ACGTTGCATGCA", "ACGTGCATCCA"});
    ps.push_back({"ACGT", "ACGTACGT"});
    ps.push_back({"A", "T"});
    ps.push_back({"AC-G.T", "ACGT"});
    ps.push_back({"acgt", "ACGT"});
    const std::string base = rand_seq(140);
    for (size_t ql : {0, 1, 2, 63, 64, 65, 127, 128, 129})
        for (size_t sl : {0, 1, 2, 63, 64, 65, 129}) {
            std::string q = base.substr(3, ql), s = base.substr(0, sl);
            for (size_t b = 5; b < q.size(); b += 17) q[b] = "ACGT"[rnd() & 3u];
            if (s.size() > 40) s.erase(20, 3);
            ps.push_back({q, s});
        }
    const std::string left = rand_seq(100), mid = rand_seq(130), right = rand_seq(100);
    ps.push_back({left + mid + right, left + right});
    ps.push_back({left + right, left + mid + right});
    ps.push_back({std::string("AC\0GT\r\nRYKM*nN x", 16), "ACGTRYKM*NN"});
    const size_t refused = ps.size();
    ps.push_back({std::string(107374, 'A'), std::string(107374, 'A')});
    ps.push_back({left, left});

    Result ref;
    ldbg_hostsim_set_lanes(1);
    if (!run(ps, ref)) return 1;
    well_formed(ref, refused, "lane1");
    EXPECT(ref.score[0] == 36.0 && ref.alen[0] == 12 && ref.edits[0] == 2, "table row 1: score %g aligned_len %d edits %d", ref.score[0], ref.alen[0], ref.edits[0]);
    EXPECT(ref.score[1] == 20.0 && ref.alen[1] == 8 && ref.end_s[1] == 4, "table row 2: score %g", ref.score[1]);
    EXPECT(ref.score[2] == -1.0 && ref.end_q[2] == -1, "table row 3: score %g", ref.score[2]);
    EXPECT(ref.score[3] == 20.0 && ref.q_off[4] - ref.q_off[3] == 4, "table row 4: score %g", ref.score[3]);
    EXPECT(ref.score[4] == 40000.0, "X against a letter: score %g", ref.score[4]);
    printf("lane1: %zu pairs, %lld columns\n", ps.size(), (long long)ref.col_off.back());

    struct Variant { const char* name; int lanes; const char* lds_cells; const char* arena; };
    const Variant variants[] = {{"lanes64", 64, nullptr, nullptr}, {"lanes64 hbm row sliced", 64, "60", "120000"}, {"lane1 hbm row", 1, "0", nullptr},
                                {"lane1 sliced", 1, nullptr, "80000"}};
    for (const Variant& v : variants) {
        ldbg_hostsim_set_lanes(v.lanes);
        if (v.lds_cells) setenv("LDBG_SW_LDS_CELLS", v.lds_cells, 1); else unsetenv("LDBG_SW_LDS_CELLS");
        if (v.arena) setenv("LDBG_SW_ARENA_BYTES", v.arena, 1); else unsetenv("LDBG_SW_ARENA_BYTES");
        Result r;
        if (!run(ps, r)) return 1;
        EXPECT(same(ref, r), "%s differs from lane1", v.name);
        printf("%s: %s\n", v.name, same(ref, r) ? "identical" : "DIFFERENT");
    }
    if (g_fail) { printf("sw_san_main: %d failures\n", g_fail); return 1; }
    printf("sw_san_main: ok\n");
    return 0;
}
