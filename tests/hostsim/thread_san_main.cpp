// TEST-ONLY stand-alone program over the host simulation of libldbg (make -C corticall_amd/csrc hostsim-san-thread): writes small graphs,
// threads sequences through them with ldbg_graph_thread so that the kernels of thread.cpp run under AddressSanitizer and UBSan without
// loading the library into another process, and checks every window and every per-sequence value against the reference's loops
// restated here on strings (Call.java:2358-2381, :2425-2451).  Prints one line per case; exits non-zero on an error.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/ldbg.h"

extern "C" void ldbg_hostsim_set_lanes(int n);

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_rng >> 33); }
static std::string rand_seq(size_t n) { std::string s(n, 'A'); for (char& c : s) c = "ACGT"[rnd() & 3u]; return s; }
static std::string revcomp(const std::string& s) {
    std::string r(s.rbegin(), s.rend());
    for (char& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return r;
}
static bool is_bases(const std::string& s) { return s.find_first_not_of("ACGT") == std::string::npos; }
static std::string canonical(const std::string& s) { const std::string r = revcomp(s); return r < s ? r : s; }

static void put32(std::vector<uint8_t>& o, uint32_t v) { for (int i = 0; i < 4; i++) o.push_back((uint8_t)(v >> (8 * i))); }
static void put64(std::vector<uint8_t>& o, uint64_t v) { for (int i = 0; i < 8; i++) o.push_back((uint8_t)(v >> (8 * i))); }

// the k-mers (canonical, sorted: ASCII order is the packed order) as a one-colour .ctx with coverage 1
static bool write_ctx(const std::set<std::string>& kmers, int k, const std::string& path) {
    const int W = (k + 31) / 32;
    std::vector<uint8_t> o;
    o.insert(o.end(), {'C', 'O', 'R', 'T', 'E', 'X'});
    put32(o, 6); put32(o, (uint32_t)k); put32(o, (uint32_t)W); put32(o, 1);
    put32(o, 0); put64(o, 0);
    put32(o, 1); o.push_back('s');
    for (int c = 0; c < 16; c++) o.push_back(0);
    put32(o, 0); put32(o, 0); put32(o, 0); put32(o, 0);
    o.insert(o.end(), {'C', 'O', 'R', 'T', 'E', 'X'});
    for (const std::string& s : kmers) {
        std::vector<uint64_t> w((size_t)W, 0);
        for (int i = 0; i < k; i++) {
            const int bit = 2 * (k - 1 - i);
            const uint64_t v = s[(size_t)i] == 'A' ? 0 : s[(size_t)i] == 'C' ? 1 : s[(size_t)i] == 'G' ? 2 : 3;
            w[(size_t)(W - 1 - (bit >> 6))] |= v << (bit & 63);
        }
        for (uint64_t x : w) put64(o, x);
        put32(o, 1);
        o.push_back(0);
    }
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(o.data(), 1, o.size(), f) == o.size();
    return fclose(f) == 0 && ok;
}

static int run(const std::vector<std::string>& seqs, int k, unsigned pick_g, unsigned pick_r, const char* what) {
    std::set<std::string> gk, rk;
    for (const std::string& s : seqs)
        for (size_t i = 0; i + (size_t)k <= s.size(); i++) {
            const std::string sk = s.substr(i, (size_t)k);
            if (!is_bases(sk)) continue;
            if (rnd() % 100 < pick_g) gk.insert(canonical(sk));
            if (rnd() % 100 < pick_r) rk.insert(canonical(sk));
        }
    while (gk.size() < 3) gk.insert(canonical(rand_seq((size_t)k)));
    std::map<std::string, int64_t> gmap;
    for (const std::string& s : gk) { const int64_t i = (int64_t)gmap.size(); gmap[s] = i; }
    // the expected values
    std::vector<int64_t> want_rec, want_ws{0};
    std::vector<uint8_t> want_info;
    std::vector<int32_t> want_copy, want_first, want_last, want_hits, want_distinct;
    std::vector<std::pair<int32_t, int32_t>> want_regions;
    for (const std::string& s : seqs) {
        std::map<std::string, int32_t> seen;
        std::set<std::string> used;
        int32_t first = -1, last = -1, hits = 0, rs = -1, re = 0, n = 0;
        for (size_t i = 0; i + (size_t)k <= s.size(); i++, n++) {
            const std::string sk = s.substr(i, (size_t)k);
            bool hit = false;
            if (!is_bases(sk)) { want_rec.push_back(-1); want_info.push_back(0); want_copy.push_back(0); }
            else {
                const std::string r = revcomp(sk), c = r < sk ? r : sk;
                auto it = seen.find(sk);
                const int32_t ci = it == seen.end() ? (seen[sk] = 0) : ++it->second;
                hit = rk.count(c) != 0;
                want_rec.push_back(gmap.count(c) ? gmap[c] : -1);
                want_info.push_back((uint8_t)(1u | (r < sk ? 2u : 0u) | (r == sk ? 4u : 0u) | (hit ? 8u : 0u)));
                want_copy.push_back(ci);
                if (hit) used.insert(c);
            }
            if (hit) { if (first < 0) first = (int32_t)i; last = (int32_t)i; hits++; if (rs == -1) rs = (int32_t)i; re = (int32_t)i; }
            else if (rs > -1) { want_regions.push_back({rs, re}); rs = -1; re = 0; }
        }
        if (rs > -1) want_regions.push_back({rs, re});
        want_ws.push_back(want_ws.back() + n);
        want_first.push_back(first); want_last.push_back(last); want_hits.push_back(hits); want_distinct.push_back((int32_t)used.size());
    }
    const std::string base = std::string("/tmp/ldbg_thread_san_") + what, gp = base + "_g.ctx", rp = base + "_r.ctx";
    if (!write_ctx(gk, k, gp) || !write_ctx(rk, k, rp)) { printf("%s: cannot write the inputs\n", what); return 1; }
    std::string text;
    std::vector<int64_t> offs{0};
    for (const std::string& s : seqs) { text += s; offs.push_back((int64_t)text.size()); }
    ldbg_graph *g = nullptr, *r = nullptr;
    ldbg_threading* t = nullptr;
    ldbg_status st = ldbg_graph_open(gp.c_str(), 0, &g);
    if (st == LDBG_OK) st = ldbg_graph_open(rp.c_str(), 0, &r);
    if (st == LDBG_OK) st = ldbg_graph_thread(g, r, text.empty() ? "" : text.data(), offs.data(), (int64_t)seqs.size(), LDBG_THREAD_COPY_INDEX, &t);
    int64_t ns = -1, nw = -1, nr = -1;
    if (st == LDBG_OK) st = ldbg_threading_info(t, &ns, &nw, &nr, nullptr);
    bool same = st == LDBG_OK && ns == (int64_t)seqs.size() && nw == want_ws.back() && nr == (int64_t)want_regions.size();
    if (same) {
        const size_t M = (size_t)nw, S = seqs.size(), R = (size_t)nr;
        std::vector<int64_t> rec(M + 1), ws(S + 1), ro(S + 1);
        std::vector<uint8_t> info(M + 1), ends(S + 1);
        std::vector<int32_t> copy(M + 1), cov(M + 1), first(S + 1), last(S + 1), hits(S + 1), distinct(S + 1), rstart(R + 1), rstop(R + 1);
        st = ldbg_threading_windows(t, 0, nw, rec.data(), info.data(), copy.data());
        if (st == LDBG_OK) st = ldbg_threading_summary(t, 0, ns, ws.data(), first.data(), last.data(), hits.data(), distinct.data(), ends.data());
        if (st == LDBG_OK) st = ldbg_threading_regions(t, ro.data(), rstart.data(), rstop.data(), nr);
        const ldbg_status cs = ldbg_threading_coverage(t, 0, 0, nw, cov.data());
        bool any_null = false;
        for (size_t m = 0; m < M; m++) any_null |= want_rec[m] < 0;
        same = st == LDBG_OK && cs == (any_null ? LDBG_ERR_NULLPOINTER : LDBG_OK);
        for (size_t m = 0; same && m < M; m++) same = rec[m] == want_rec[m] && info[m] == want_info[m] && copy[m] == want_copy[m] && (want_rec[m] < 0 || cov[m] == 1);
        for (size_t s = 0; same && s < S; s++)
            same = ws[s + 1] == want_ws[s + 1] && first[s] == want_first[s] && last[s] == want_last[s] && hits[s] == want_hits[s] && distinct[s] == want_distinct[s];
        for (size_t x = 0; same && x < R; x++) same = rstart[x] == want_regions[x].first && rstop[x] == want_regions[x].second;
    }
    if (st != LDBG_OK) printf("%s: %s\n", what, ldbg_last_error());
    if (t) ldbg_threading_free(t);
    if (r) ldbg_graph_close(r);
    if (g) ldbg_graph_close(g);
    remove(gp.c_str()); remove(rp.c_str());
    printf("%-10s k=%-3d sequences %-5zu status %d windows %lld/%lld regions %lld/%zu %s\n", what, k, seqs.size(), (int)st, (long long)nw, (long long)want_ws.back(),
           (long long)nr, want_regions.size(), same ? "same" : "DIFFERENT");
    return same ? 0 : 1;
}

static int refused() {
    std::set<std::string> gk{"AAACC", "AACCA", "ACCAA"};
    const std::string gp = "/tmp/ldbg_thread_san_refused.ctx";
    if (!write_ctx(gk, 5, gp)) return 1;
    ldbg_graph* g = nullptr;
    ldbg_threading* t = nullptr;
    ldbg_status st = ldbg_graph_open(gp.c_str(), 0, &g);
    const char one = 'A';
    const int64_t dec[3] = {0, 9, 4}, huge[2] = {0, ((int64_t)1 << 31) + 4};
    const ldbg_status a = st == LDBG_OK ? ldbg_graph_thread(nullptr, nullptr, &one, dec, 2, 0, &t) : st;
    const ldbg_status b = st == LDBG_OK ? ldbg_graph_thread(g, nullptr, &one, dec, 2, 0, &t) : st;
    const ldbg_status c = st == LDBG_OK ? ldbg_graph_thread(g, nullptr, &one, huge, 1, 0, &t) : st;
    if (g) ldbg_graph_close(g);
    remove(gp.c_str());
    const bool ok = a == LDBG_ERR_ARG && b == LDBG_ERR_ARG && c == LDBG_ERR_UNSUPPORTED && t == nullptr;
    printf("%-10s no graph %d, decreasing offsets %d, 2^31 windows over one byte %d %s\n", "refused", (int)a, (int)b, (int)c, ok ? "same" : "DIFFERENT");
    return ok ? 0 : 1;
}

int main() {
    int bad = 0;
    for (int lanes : {1, 64}) {
        ldbg_hostsim_set_lanes(lanes);
        g_rng = 0x9E3779B97F4A7C15ull;                   // the same inputs at either width
        bad += run({rand_seq(4097 + 20)}, 21, 60, 40, "chunk");          // 4097 windows: a scan chunk and one more
        const std::string w = rand_seq(300);
        bad += run({w, w.substr(0, 64), w.substr(10, 65), rand_seq(66)}, 65, 70, 30, "wide");       // three-word k-mers, sequences of k - 1, k and k + 1 bytes
        const std::string x = rand_seq(31), sp = rand_seq(9);
        bad += run({sp + x + sp + x + sp + revcomp(x) + sp + x + sp, sp + x + sp}, 31, 100, 100, "repeats");
        std::string n = rand_seq(120);
        n[50] = 'N'; n[100] = 'a';
        bad += run({n, std::string(40, 'N')}, 31, 80, 50, "N");
        bad += run({}, 31, 0, 0, "empty");
        bad += run({"", "ACGT"}, 31, 0, 0, "short");
        bad += refused();
    }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
