// TEST-ONLY stand-alone program over the host simulation of libldbg (make -C corticall_amd/csrc hostsim-san-recover): writes two small
// graphs, runs ldbg_graph_recover, ldbg_selection_write_recovered and ldbg_selection_open_recovered on them so that the recover kernels
// of select.cpp run under AddressSanitizer and UBSan without loading the library into another process, and checks the counts against
// the reference's loop restated here.  Prints them; exits non-zero on an error.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/ldbg.h"

extern "C" void ldbg_hostsim_set_lanes(int n);

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_rng >> 33); }
static const uint32_t COV[5] = {0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};

struct Table {
    int k, C;
    std::vector<uint64_t> key;             // the last word of each k-mer; the words before it are 0 (leading A's: canonical, ascending)
    std::vector<uint32_t> cov;             // [N][C]
};

static void put32(std::vector<uint8_t>& o, uint32_t v) { for (int i = 0; i < 4; i++) o.push_back((uint8_t)(v >> (8 * i))); }
static void put64(std::vector<uint8_t>& o, uint64_t v) { for (int i = 0; i < 8; i++) o.push_back((uint8_t)(v >> (8 * i))); }

static bool write_ctx(const Table& t, const std::vector<std::string>& names, const std::string& path) {
    const int W = (t.k + 31) / 32;
    std::vector<uint8_t> o;
    o.insert(o.end(), {'C', 'O', 'R', 'T', 'E', 'X'});
    put32(o, 6); put32(o, (uint32_t)t.k); put32(o, (uint32_t)W); put32(o, (uint32_t)t.C);
    for (int c = 0; c < t.C; c++) put32(o, 0);
    for (int c = 0; c < t.C; c++) put64(o, 0);
    for (int c = 0; c < t.C; c++) { put32(o, (uint32_t)names[c].size()); o.insert(o.end(), names[c].begin(), names[c].end()); }
    for (int c = 0; c < 16 * t.C; c++) o.push_back(0);
    for (int c = 0; c < t.C; c++) { put32(o, 0); put32(o, 0); put32(o, 0); put32(o, 0); }
    o.insert(o.end(), {'C', 'O', 'R', 'T', 'E', 'X'});
    for (size_t i = 0; i < t.key.size(); i++) {
        for (int w = 0; w + 1 < W; w++) put64(o, 0);
        put64(o, t.key[i]);
        for (int c = 0; c < t.C; c++) put32(o, t.cov[i * t.C + c]);
        for (int c = 0; c < t.C; c++) o.push_back((uint8_t)(i * 7 + c));
    }
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(o.data(), 1, o.size(), f) == o.size();
    return fclose(f) == 0 && ok;
}

static long file_size(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return -1;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fclose(f);
    return n;
}

static int run(int64_t N, int k, int C, int child, int64_t n_dirty_own, const char* what) {
    Table g{k, C, {}, {}}, d{k, 1, {}, {}};
    std::map<uint64_t, uint32_t> dirty;
    for (int64_t i = 0; i < N; i++) {
        g.key.push_back((uint64_t)(3 * i + 1));
        for (int c = 0; c < C; c++) g.cov.push_back(COV[rnd() % 5]);
        if (rnd() % 4 == 0) dirty[g.key.back()] = COV[rnd() % 5];
    }
    for (int64_t i = 0; i < n_dirty_own; i++) dirty[(uint64_t)(6 * i + 2)] = 1u;
    for (auto& kv : dirty) { d.key.push_back(kv.first); d.cov.push_back(kv.second); }
    int64_t want_n = 0, want_rec = 0;                                   // RecoverExcludedKmers.java:50-93 on Java ints
    for (int64_t i = 0; i < N; i++) {
        if ((int32_t)g.cov[i * C + child] > 0) { want_n++; continue; }
        bool other = false;
        for (int c = 0; c < C; c++) other |= c != child && (int32_t)g.cov[i * C + c] > 0;
        auto it = dirty.find(g.key[i]);
        if (other && dirty.size() > 2 && it != dirty.end() && (int32_t)it->second > 0) { want_n++; want_rec++; }
    }
    const std::string base = std::string("/tmp/ldbg_recover_san_") + what, gp = base + "_g.ctx", dp = base + "_d.ctx", op = base + "_out.ctx";
    std::vector<std::string> names;
    for (int c = 0; c < C; c++) names.push_back("s" + std::to_string(c));
    if (!write_ctx(g, names, gp) || !write_ctx(d, {names[child]}, dp)) { printf("%s: cannot write the inputs\n", what); return 1; }
    ldbg_graph *gg = nullptr, *dg = nullptr, *rg = nullptr;
    ldbg_selection* sel = nullptr;
    int64_t n = -1, rec = -1, rn = -1;
    ldbg_status st = ldbg_graph_open(gp.c_str(), 0, &gg);
    if (st == LDBG_OK) st = ldbg_graph_open(dp.c_str(), 0, &dg);
    if (st == LDBG_OK) st = ldbg_graph_recover(gg, child, dg, &sel, &rec);
    if (st == LDBG_OK) st = ldbg_selection_count(sel, &n);
    std::vector<int32_t> col((size_t)(n > 0 ? n : 1));
    std::vector<int64_t> idx((size_t)(n > 0 ? n : 1));
    if (st == LDBG_OK) st = ldbg_selection_recovered_coverage(sel, 0, n, col.data());
    if (st == LDBG_OK) st = ldbg_selection_indices(sel, 0, n, idx.data());
    bool positive = true;
    for (int64_t i = 0; st == LDBG_OK && i < n; i++) positive = positive && col[(size_t)i] > 0 && idx[(size_t)i] < N;
    if (st == LDBG_OK) st = ldbg_selection_write_recovered(sel, op.c_str());
    if (st == LDBG_OK) st = ldbg_selection_open_recovered(sel, &rg);
    if (st == LDBG_OK) st = ldbg_graph_info(rg, nullptr, nullptr, nullptr, &rn, nullptr);
    const long header = 6 + 16 + 4 + 8 + 4 + (long)names[child].size() + 16 + 16 + 6, R = 8 * ((k + 31) / 32) + 5;
    const long size = file_size(op), want_size = header + R * (long)want_n;
    if (st != LDBG_OK) printf("%s: %s\n", what, ldbg_last_error());
    if (rg) ldbg_graph_close(rg);
    if (sel) ldbg_selection_free(sel);
    if (dg) ldbg_graph_close(dg);
    if (gg) ldbg_graph_close(gg);
    remove(gp.c_str()); remove(dp.c_str()); remove(op.c_str());
    printf("%-10s N=%-7lld k=%-3d C=%d child=%d dirty=%-6zu status %d written %lld/%lld recovered %lld/%lld resident %lld file %ld/%ld\n", what, (long long)N, k, C, child,
           dirty.size(), (int)st, (long long)n, (long long)want_n, (long long)rec, (long long)want_rec, (long long)rn, size, want_size);
    return st == LDBG_OK && n == want_n && rec == want_rec && rn == want_n && size == want_size && positive ? 0 : 1;
}

int main() {
    int bad = 0;
    for (int lanes : {1, 64}) {
        ldbg_hostsim_set_lanes(lanes);
        g_rng = 0x9E3779B97F4A7C15ull;                   // the same inputs at either width
        bad += run(70001, 31, 3, 0, 9000, "chunks");     // 18 chunks, the last one short
        bad += run(4097, 65, 4, 2, 500, "wide");         // three-word k-mers, the child in a middle colour
        bad += run(65, 31, 2, 1, 0, "small");
        bad += run(300, 31, 3, 0, 2, "q1");              // (the dirty graph below holds GRAPH k-mers too: more than two records)
        bad += run(0, 31, 3, 0, 5, "empty");
    }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
