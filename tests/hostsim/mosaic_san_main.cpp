// TEST-ONLY stand-alone program over the host simulation of libldbg (make -C corticall_amd/csrc hostsim-san-mosaic): runs
// ldbg_mosaic_align_batch on the boundary-length problems — target lengths 1, 3, 63, 64, 65, 129, query lengths 1, 2, 3, 64, 65, 1, 2, 3 and
// 65 targets, a target of length 0, the refused shapes — with 1 lane and 64 lanes in lock step, the columns in (simulated) LDS and in
// the HBM scratch, the arena whole and in slices, so that the kernel of mosaic.cpp runs under AddressSanitizer and UBSan without loading
// the library into another process.  Checks what needs no second implementation: TestTesserae.smallTest's documented layout, that every
// variant of a run returns the same bytes, and that a path is well formed (it consumes the query once, every entry names a base of its
// sequence).  Prints one line per case; exits non-zero on an error.
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

struct Problem { std::string query; std::vector<std::string> targets; };
struct Result { std::vector<uint8_t> status; std::vector<double> llk; std::vector<int64_t> off; std::vector<int32_t> copy, state, pos; };

static int g_fail = 0;
#define EXPECT(c, ...) do { if (!(c)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); g_fail++; } } while (0)

static bool run(const std::vector<Problem>& ps, Result& r) {
    std::string q, t;
    std::vector<int64_t> qoff{0}, tfirst{0}, toff{0};
    for (const Problem& p : ps) {
        q += p.query; qoff.push_back((int64_t)q.size());
        for (const std::string& s : p.targets) { t += s; toff.push_back((int64_t)t.size()); }
        tfirst.push_back((int64_t)toff.size() - 1);
    }
    const ldbg_mosaic_params par{0.025, 0.75, 0.0001, 0.001};
    ldbg_mosaic_result* h = nullptr;
    if (ldbg_mosaic_align_batch(0, &par, (int64_t)ps.size(), q.data(), qoff.data(), tfirst.data(), t.data(), toff.data(), &h) != LDBG_OK) {
        printf("FAIL align_batch: %s\n", ldbg_last_error());
        g_fail++;
        return false;
    }
    int64_t n = 0, ne = 0;
    ldbg_mosaic_result_sizes(h, &n, &ne);
    r.status.assign((size_t)n, 0); r.llk.assign((size_t)n, 0); r.off.assign((size_t)n + 1, 0);
    r.copy.assign((size_t)ne + 1, 0); r.state.assign((size_t)ne + 1, 0); r.pos.assign((size_t)ne + 1, 0);
    const ldbg_mosaic_arrays a{r.status.data(), r.llk.data(), r.off.data(), r.copy.data(), r.state.data(), r.pos.data()};
    ldbg_mosaic_result_get(h, &a);
    ldbg_mosaic_result_free(h);
    r.copy.resize((size_t)ne); r.state.resize((size_t)ne); r.pos.resize((size_t)ne);
    return true;
}

static bool same(const Result& a, const Result& b) {
    return a.status == b.status && a.off == b.off && a.copy == b.copy && a.state == b.state && a.pos == b.pos &&
           (a.llk.empty() || memcmp(a.llk.data(), b.llk.data(), a.llk.size() * 8) == 0);
}

static void well_formed(const std::vector<Problem>& ps, const Result& r, const char* what) {
    for (size_t i = 0; i < ps.size(); i++) {
        const Problem& p = ps[i];
        size_t maxl = p.query.size(), total = 0;
        for (const std::string& s : p.targets) { maxl = std::max(maxl, s.size()); total += s.size(); }
        const bool refused = p.query.empty() || p.targets.empty() || total == 0 || maxl <= 2;
        EXPECT((r.status[i] != LDBG_OK) == refused, "%s problem %zu: status %d", what, i, (int)r.status[i]);
        if (r.status[i] != LDBG_OK) { EXPECT(r.off[i + 1] == r.off[i], "%s problem %zu: a refused problem with a path", what, i); continue; }
        size_t consumed = 0;
        for (int64_t e = r.off[i]; e < r.off[i + 1]; e++) {
            const int c = r.copy[(size_t)e], s = r.state[(size_t)e], q = r.pos[(size_t)e];
            EXPECT(c >= 2 && c <= (int)p.targets.size() + 1 && s >= 1 && s <= 3, "%s problem %zu entry %lld: copy %d state %d", what, i, (long long)e, c, s);
            if (c >= 2 && c <= (int)p.targets.size() + 1) EXPECT(q >= 1 && q <= (int)p.targets[(size_t)c - 2].size(), "%s problem %zu: pos %d", what, i, q);
            if (s != 3) consumed++;
        }
        EXPECT(consumed == p.query.size(), "%s problem %zu: the path consumes %zu of %zu query bases", what, i, consumed, p.query.size());
        EXPECT(r.llk[i] < 0 && r.llk[i] > -1e6, "%s problem %zu: llk %g", what, i, r.llk[i]);
    }
}

int main() {
    std::vector<Problem> ps;
    ps.push_back({"GTAGGCGAGATGACGCCAT", {"GTAGGCGAGTCCCGTTTATA", "CCACAGAAGATGACGCCATT"}});
    for (size_t ql : {1, 2, 3, 64, 65})
        for (size_t tl : {1, 3, 63, 64, 65, 129}) {
            std::string t = rand_seq(tl), q = rand_seq(ql);
            for (size_t b = 0; b < ql; b++) if (b % 7 != 3) q[b] = t[b % tl];
            ps.push_back({q, {t}});
        }
    const std::string base = rand_seq(70);
    for (int nt : {1, 2, 3, 65}) {
        Problem p{base.substr(2, 20), {}};
        for (int j = 0; j < nt; j++) p.targets.push_back(base.substr((size_t)(j % 5), 3 + rnd() % 4));
        ps.push_back(p);
    }
    ps.push_back({base.substr(0, 30), {base.substr(0, 20), "", base.substr(10, 35)}});
    ps.push_back({"", {base}});
    ps.push_back({base.substr(0, 10), {}});
    ps.push_back({"AC", {"GT", "A"}});
    ps.push_back({"ACG", {"", ""}});
    ps.push_back({base.substr(0, 30) + rand_seq(70) + base.substr(30), {base}});          // an insert run
    ps.push_back({base.substr(0, 20) + base.substr(50), {base, "NNNNacgtNNNN"}});        // a delete run, non-bases

    Result ref;
    ldbg_hostsim_set_lanes(1);
    if (!run(ps, ref)) return 1;
    well_formed(ps, ref, "lane1");
    // smallTest: template0 (0-6), then template1 (7-18), all matches
    for (int e = 0; e < 19 && ref.off[1] == 19; e++)
        EXPECT(ref.copy[(size_t)e] == (e < 7 ? 2 : 3) && ref.state[(size_t)e] == 1 && ref.pos[(size_t)e] == e + 1, "smallTest entry %d", e);
    EXPECT(ref.off[1] == 19 && ref.llk[0] == -26.96475012162965, "smallTest: %lld entries, llk %.17g", (long long)ref.off[1], ref.llk[0]);
    printf("lane1: %zu problems, %lld path entries\n", ps.size(), (long long)ref.off.back());

    struct Variant { const char* name; int lanes; const char* lds_cells; const char* arena; };
    const Variant variants[] = {{"lanes64", 64, nullptr, nullptr}, {"lanes64 hbm columns", 64, "0", nullptr}, {"lane1 hbm columns", 1, "0", nullptr},
                                {"lanes64 sliced", 64, nullptr, "20000"}, {"lanes64 hbm columns sliced", 64, "0", "40000"}};
    for (const Variant& v : variants) {
        ldbg_hostsim_set_lanes(v.lanes);
        if (v.lds_cells) setenv("LDBG_MOSAIC_LDS_CELLS", v.lds_cells, 1); else unsetenv("LDBG_MOSAIC_LDS_CELLS");
        if (v.arena) setenv("LDBG_MOSAIC_ARENA_BYTES", v.arena, 1); else unsetenv("LDBG_MOSAIC_ARENA_BYTES");
        Result r;
        if (!run(ps, r)) return 1;
        EXPECT(same(ref, r), "%s differs from lane1", v.name);
        printf("%s: %s\n", v.name, same(ref, r) ? "identical" : "DIFFERENT");
    }
    // one lane of the roundtrip kernel
    {
        std::vector<int32_t> who{2, 66, 200}, state{1, 2, 3}, pos{0, 1096, 24999}, out(9);
        EXPECT(ldbg_mosaic_tb_roundtrip(0, 1e10, 3, who.data(), state.data(), pos.data(), out.data()) == LDBG_OK, "roundtrip: %s", ldbg_last_error());
        EXPECT(out[0] == 2 && out[1] == 1 && out[2] == 0, "roundtrip of (2, 1, 0): %d %d %d", out[0], out[1], out[2]);
    }
    if (g_fail) { printf("mosaic_san_main: %d failures\n", g_fail); return 1; }
    printf("mosaic_san_main: ok\n");
    return 0;
}
