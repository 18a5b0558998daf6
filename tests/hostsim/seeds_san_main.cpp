// TEST-ONLY stand-alone program over the host simulation of libldbg (make -C corticall_amd/csrc hostsim-san-seeds): writes small graphs
// with chosen edge bytes, takes their variant seeds with ldbg_graph_variant_seeds and the occurrences of a threading with
// ldbg_threading_occurrences, so that the kernels of seeds.cpp run under AddressSanitizer and UBSan without loading the library into
// another process, and checks the good seeds, the three counts and every record's occurrences against getVariantSeeds
// (ComputeAssemblyQuality.java:204-286) restated here on strings, maps and sets.  Prints one line per case; exits non-zero on an error.
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
static char comp(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }
static std::string revcomp(const std::string& s) {
    std::string r(s.rbegin(), s.rend());
    for (char& c : r) c = comp(c);
    return r;
}
static std::string canonical(const std::string& s) { const std::string r = revcomp(s); return r < s ? r : s; }
static int base_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3; }

static void put32(std::vector<uint8_t>& o, uint32_t v) { for (int i = 0; i < 4; i++) o.push_back((uint8_t)(v >> (8 * i))); }
static void put64(std::vector<uint8_t>& o, uint64_t v) { for (int i = 0; i < 8; i++) o.push_back((uint8_t)(v >> (8 * i))); }

// records (canonical k-mer -> coverage and edge byte of one colour) with chosen edges
struct Rec { uint32_t cov = 0; uint8_t edges = 0; };
struct Tab {
    int k;
    std::map<std::string, Rec> rec;
    void add(const std::string& v, uint32_t cov) { rec[canonical(v)].cov = cov; }
    // the edge a -> b written into a's record (which 'a') and / or b's record ('b')
    void edge(const std::string& a, const std::string& b, const char* declare = "ab") {
        const std::string ka = canonical(a), kb = canonical(b);
        if (strchr(declare, 'a') && rec.count(ka)) {
            if (a == ka) rec[ka].edges |= (uint8_t)(1u << base_of(b.back()));
            else rec[ka].edges |= (uint8_t)(1u << (4 + 3 - base_of(comp(b.back()))));
        }
        if (strchr(declare, 'b') && rec.count(kb)) {
            if (b == kb) rec[kb].edges |= (uint8_t)(1u << (4 + 3 - base_of(a[0])));
            else rec[kb].edges |= (uint8_t)(1u << base_of(comp(a[0])));
        }
    }
    bool write(const std::string& path) const {
        const int W = (k + 31) / 32;
        std::vector<uint8_t> o;
        o.insert(o.end(), {'C', 'O', 'R', 'T', 'E', 'X'});
        put32(o, 6); put32(o, (uint32_t)k); put32(o, (uint32_t)W); put32(o, 1);
        put32(o, 0); put64(o, 0);
        put32(o, 1); o.push_back('s');
        for (int c = 0; c < 16; c++) o.push_back(0);
        put32(o, 0); put32(o, 0); put32(o, 0); put32(o, 0);
        o.insert(o.end(), {'C', 'O', 'R', 'T', 'E', 'X'});
        for (const auto& kv : rec) {
            std::vector<uint64_t> w((size_t)W, 0);
            for (int i = 0; i < k; i++) {
                const int bit = 2 * (k - 1 - i);
                w[(size_t)(W - 1 - (bit >> 6))] |= (uint64_t)base_of(kv.first[(size_t)i]) << (bit & 63);
            }
            for (uint64_t x : w) put64(o, x);
            put32(o, kv.second.cov);
            o.push_back(kv.second.edges);
        }
        FILE* f = fopen(path.c_str(), "wb");
        if (!f) return false;
        const bool ok = fwrite(o.data(), 1, o.size(), f) == o.size();
        return fclose(f) == 0 && ok;
    }
};

struct Want { std::vector<int64_t> good; int64_t n_seeds = 0, n_unique = 0; };

// getVariantSeeds with the filter "singly connected, coverage > 0, unique[r]" over one colour
static Want yardstick(const Tab& t, const std::vector<uint8_t>& unique) {
    std::map<std::string, std::set<std::string>> succ, pred;
    std::vector<std::string> verts;
    auto vertex = [&](const std::string& x) { if (!succ.count(x)) { succ[x]; pred[x]; verts.push_back(x); } };
    auto edge = [&](const std::string& a, const std::string& b) { vertex(a); vertex(b); succ[a].insert(b); pred[b].insert(a); };
    Want w;
    std::map<std::string, int64_t> index;
    int64_t r = 0;
    for (const auto& kv : t.rec) {
        index[kv.first] = r;
        const uint8_t e = kv.second.edges;
        const bool in_s = (int32_t)kv.second.cov > 0 && __builtin_popcount(e >> 4) == 1 && __builtin_popcount(e & 15) == 1 && unique[(size_t)r];
        r++;
        if (!in_s) continue;
        w.n_seeds++;
        const std::string fw = kv.first, rv = revcomp(fw);
        vertex(fw); vertex(rv);
        for (int i = 0; i < 4; i++)
            if ((e >> 4) & (1 << (3 - i))) { const std::string p = std::string(1, "ACGT"[i]) + fw.substr(0, fw.size() - 1); edge(p, fw); edge(rv, revcomp(p)); }
        for (int i = 0; i < 4; i++)
            if ((e & 15) & (1 << i)) { const std::string n = fw.substr(1) + "ACGT"[i]; edge(fw, n); edge(revcomp(n), rv); }
    }
    std::set<int64_t> good;
    for (const std::string& sk : verts) {
        if (!pred[sk].empty() || succ[sk].size() != 1) continue;
        w.n_unique++;
        std::vector<std::string> contig{sk};
        std::string v = sk;
        while (succ[v].size() == 1) {
            v = *succ[v].begin();
            if (std::find(contig.begin(), contig.end(), v) != contig.end()) break;
            contig.push_back(v);
        }
        if (contig.size() > 3) good.insert(index.at(canonical(contig[1])));
    }
    w.good.assign(good.begin(), good.end());
    return w;
}

// one table: the seeds with every record unique (bytes), then with uniqueness from the occurrences of `seqs`
static int run(const Tab& t, const std::vector<std::string>& seqs, const char* what) {
    const std::string path = std::string("/tmp/ldbg_seeds_san_") + what + ".ctx";
    if (!t.write(path)) { printf("%s: cannot write the input\n", what); return 1; }
    const size_t N = t.rec.size();
    // occurrences by a plain loop
    std::map<std::string, int64_t> index;
    for (const auto& kv : t.rec) { const int64_t i = (int64_t)index.size(); index[kv.first] = i; }
    std::vector<uint32_t> want_count(N, 0);
    std::vector<int64_t> want_first(N, -1);
    int64_t wnum = 0;
    for (const std::string& s : seqs)
        for (size_t i = 0; i + (size_t)t.k <= s.size(); i++, wnum++) {
            const std::string sk = s.substr(i, (size_t)t.k);
            if (sk.find_first_not_of("ACGT") != std::string::npos) continue;
            auto it = index.find(canonical(sk));
            if (it == index.end()) continue;
            want_count[(size_t)it->second]++;
            if (want_first[(size_t)it->second] < 0) want_first[(size_t)it->second] = wnum;
        }
    std::vector<uint8_t> all(N, 1), once(N, 0);
    for (size_t i = 0; i < N; i++) once[i] = want_count[i] == 1;
    const Want w_all = yardstick(t, all), w_once = yardstick(t, once);

    std::string text;
    std::vector<int64_t> offs{0};
    for (const std::string& s : seqs) { text += s; offs.push_back((int64_t)text.size()); }
    ldbg_graph* g = nullptr;
    ldbg_threading* th = nullptr;
    ldbg_occurrences* occ = nullptr;
    ldbg_status st = ldbg_graph_open(path.c_str(), 0, &g);
    if (st == LDBG_OK) st = ldbg_graph_thread(g, nullptr, text.empty() ? "" : text.data(), offs.data(), (int64_t)seqs.size(), 0, &th);
    if (st == LDBG_OK) st = ldbg_threading_occurrences(th, &occ);
    bool same = st == LDBG_OK;
    if (same) {
        std::vector<uint32_t> count(N + 1, 7);
        std::vector<int64_t> first(N + 1, 7);
        st = ldbg_occurrences_get(occ, 0, (int64_t)N, count.data(), first.data());
        same = st == LDBG_OK;
        for (size_t i = 0; same && i < N; i++) same = count[i] == want_count[i] && first[i] == want_first[i];
    }
    for (int pass = 0; same && pass < 2; pass++) {
        const Want& w = pass ? w_once : w_all;
        ldbg_seed_filter f;
        memset(&f, 0, sizeof f);
        f.n_covered = 1;
        f.covered[0].mask = 1; f.covered[0].at_least = 1; f.covered[0].at_most = 1;
        f.n_unique = 1;
        f.unique[0].colour = pass ? 0 : -1;
        if (pass) f.unique[0].occurrences = occ; else f.unique[0].d_unique = all.data();      // (the simulation's device memory is host memory)
        ldbg_selection* sel = nullptr;
        ldbg_seed_counts cn;
        st = ldbg_graph_variant_seeds(g, &f, &sel, &cn);
        same = st == LDBG_OK && cn.n_seeds == w.n_seeds && cn.n_unique == w.n_unique && cn.n_good == (int64_t)w.good.size();
        if (same) {
            std::vector<int64_t> idx(w.good.size() + 1, -7);
            int64_t n = -1;
            st = ldbg_selection_count(sel, &n);
            if (st == LDBG_OK && n == (int64_t)w.good.size()) st = ldbg_selection_indices(sel, 0, n, idx.data());
            same = st == LDBG_OK && n == (int64_t)w.good.size() && std::equal(w.good.begin(), w.good.end(), idx.begin());
        }
        if (!same) printf("%s pass %d: seeds %lld/%lld starts %lld/%lld good %lld/%zu\n", what, pass, (long long)cn.n_seeds, (long long)w.n_seeds, (long long)cn.n_unique,
                          (long long)w.n_unique, (long long)cn.n_good, w.good.size());
        if (sel) ldbg_selection_free(sel);
    }
    if (st != LDBG_OK) printf("%s: %s\n", what, ldbg_last_error());
    if (occ) ldbg_occurrences_free(occ);
    if (th) ldbg_threading_free(th);
    if (g) ldbg_graph_close(g);
    remove(path.c_str());
    printf("%-12s records %-5zu seeds %-5lld starts %-4lld good %-4zu | once: seeds %-5lld good %-4zu %s\n", what, N, (long long)w_all.n_seeds, (long long)w_all.n_unique,
           w_all.good.size(), (long long)w_once.n_seeds, w_once.good.size(), same ? "same" : "DIFFERENT");
    return same ? 0 : 1;
}

static std::vector<std::string> windows(const std::string& s, int k) {
    std::vector<std::string> w;
    for (size_t i = 0; i + (size_t)k <= s.size(); i++) w.push_back(s.substr(i, (size_t)k));
    return w;
}

// N records on one path, two of every 37 without coverage, threaded with the path itself and a stretch of it again
static int chunk(int N) {
    const int k = 21;
    for (int attempt = 0; attempt < 50; attempt++) {
        const std::string s = rand_seq((size_t)(N + k + 1));
        const std::vector<std::string> vs = windows(s, k);
        Tab t{k, {}};
        for (int i = 0; i < N; i++) t.add(vs[(size_t)i + 1], i % 37 >= 35 ? 0u : 1u);
        if ((int)t.rec.size() != N) continue;
        for (size_t i = 0; i + 1 < vs.size(); i++) t.edge(vs[i], vs[i + 1]);
        char name[32];
        snprintf(name, sizeof name, "chunk%d", N);
        return run(t, {s, revcomp(s.substr(0, std::min<size_t>(s.size(), 60)))}, name);
    }
    printf("chunk%d: no input\n", N);
    return 1;
}

static std::string other_base(char not_this) { return std::string(1, not_this == 'G' ? 'T' : 'G'); }

static int asymmetric() {
    const int k = 11;
    int bad = 0;
    {   // a successor that does not declare the edge back, and names another predecessor
        const std::vector<std::string> vs = windows(rand_seq(15), k);
        const std::string x = other_base(vs[1][0]) + vs[2].substr(0, (size_t)k - 1);
        Tab t{k, {}};
        for (size_t i = 0; i < vs.size(); i++) t.add(vs[i], i >= 1 && i <= 3 ? 1u : 0u);
        t.edge(vs[0], vs[1]); t.edge(vs[1], vs[2], "a"); t.edge(x, vs[2], "b"); t.edge(vs[2], vs[3]); t.edge(vs[3], vs[4]);
        bad += run(t, {vs[0] + vs[1].back() + vs[2].back()}, "asym_a");
    }
    {   // a predecessor edge declared only by the neighbour, whose own successor is another k-mer
        const std::vector<std::string> vs = windows(rand_seq(16), k);
        const std::string y = vs[1].substr(1) + other_base(vs[2].back());
        Tab t{k, {}};
        for (size_t i = 0; i < vs.size(); i++) t.add(vs[i], i >= 1 && i <= 4 ? 1u : 0u);
        t.edge(vs[0], vs[1]); t.edge(vs[1], y, "a"); t.edge(vs[1], vs[2], "b");
        for (size_t i = 2; i + 1 < vs.size(); i++) t.edge(vs[i], vs[i + 1]);
        bad += run(t, {}, "asym_b");
    }
    {   // a homopolymer self loop reached from a start
        const std::string x(k, 'A'), s = "C" + x.substr(1);
        Tab t{k, {}};
        t.add(x, 1); t.add(s, 0);
        t.edge(s, x); t.edge(x, x, "a");
        bad += run(t, {x + "A"}, "loop");
    }
    return bad;
}

int main() {
    int bad = 0;
    for (int lanes : {1, 64}) {
        ldbg_hostsim_set_lanes(lanes);
        g_rng = 0x9E3779B97F4A7C15ull;                   // the same inputs at either width
        for (int N : {1, 2, 3, 63, 64, 65, 4095, 4096, 4097}) bad += chunk(N);
        bad += asymmetric();
    }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
