// TEST-ONLY stand-alone program over the host simulation of libldbg (make -C corticall_amd/csrc hostsim-san-variants): writes small
// two-colour graphs (a child and a parent that differ at clusters of substitutions and at indels), calls the variants of the child's
// k-mers with ldbg_engine_variant_batch so that the kernels of variants.cpp and the cursor batches under them run under AddressSanitizer
// and UBSan without loading the library into another process, and checks every value of the result against the three loops of
// ComputeInheritance.callVariant (:119-165), toContig and trimToAlleles (:406-433) restated here on strings (no links: a cursor takes the
// single next vertex while it is not in `seen`).  Prints one line per case; exits non-zero on an error.
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
static int idx(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3; }
static char comp(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }
static char other(char c) { return "ACGT"[(idx(c) + 1 + (int)(rnd() % 3u)) & 3]; }
static std::string revcomp(const std::string& s) {
    std::string r(s.rbegin(), s.rend());
    for (char& c : r) c = comp(c);
    return r;
}
static bool is_bases(const std::string& s) { return s.find_first_not_of("ACGT") == std::string::npos; }
static std::string canonical(const std::string& s) { const std::string r = revcomp(s); return r < s ? r : s; }

static void put32(std::vector<uint8_t>& o, uint32_t v) { for (int i = 0; i < 4; i++) o.push_back((uint8_t)(v >> (8 * i))); }
static void put64(std::vector<uint8_t>& o, uint64_t v) { for (int i = 0; i < 8; i++) o.push_back((uint8_t)(v >> (8 * i))); }

enum { NC = 2 };      // colour 0: the child, colour 1: the parent that does not share its alleles
struct Rec { uint32_t cov[NC] = {0, 0}; uint8_t edges[NC] = {0, 0}; };
typedef std::map<std::string, Rec> Table;

// canonical k-mer -> per colour coverage (windows) and edge byte (high nibble: in-edges, bit 3 - base; low nibble: out-edges, bit base)
static void add_sequence(Table& t, const std::string& s, int k, int c) {
    for (size_t i = 0; i + (size_t)k <= s.size(); i++) t[canonical(s.substr(i, (size_t)k))].cov[c]++;
    for (size_t i = 0; i + (size_t)k + 1 <= s.size(); i++) {
        const std::string a = s.substr(i, (size_t)k), b = s.substr(i + 1, (size_t)k);
        if (canonical(a) == a) t[a].edges[c] |= (uint8_t)(1u << idx(b.back()));
        else t[revcomp(a)].edges[c] |= (uint8_t)(1u << (4 + 3 - idx(comp(b.back()))));
        if (canonical(b) == b) t[b].edges[c] |= (uint8_t)(1u << (4 + 3 - idx(a[0])));
        else t[revcomp(b)].edges[c] |= (uint8_t)(1u << idx(comp(a[0])));
    }
}

static bool write_ctx(const Table& t, int k, const std::string& path) {
    const int W = (k + 31) / 32;
    std::vector<uint8_t> o;
    o.insert(o.end(), {'C', 'O', 'R', 'T', 'E', 'X'});
    put32(o, 6); put32(o, (uint32_t)k); put32(o, (uint32_t)W); put32(o, NC);
    for (int c = 0; c < NC; c++) put32(o, 0);
    for (int c = 0; c < NC; c++) put64(o, 0);
    for (int c = 0; c < NC; c++) { put32(o, 1); o.push_back((uint8_t)('a' + c)); }
    for (int c = 0; c < NC * 16; c++) o.push_back(0);
    for (int c = 0; c < NC; c++) { put32(o, 0); put32(o, 0); put32(o, 0); put32(o, 0); }
    o.insert(o.end(), {'C', 'O', 'R', 'T', 'E', 'X'});
    for (const auto& kv : t) {
        std::vector<uint64_t> w((size_t)W, 0);
        for (int i = 0; i < k; i++) {
            const int bit = 2 * (k - 1 - i);
            w[(size_t)(W - 1 - (bit >> 6))] |= (uint64_t)idx(kv.first[(size_t)i]) << (bit & 63);
        }
        for (uint64_t x : w) put64(o, x);
        for (int c = 0; c < NC; c++) put32(o, kv.second.cov[c]);
        for (int c = 0; c < NC; c++) o.push_back(kv.second.edges[c]);
    }
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(o.data(), 1, o.size(), f) == o.size();
    return fclose(f) == 0 && ok;
}

static std::string decode(const uint64_t* w, int k, int W) {
    std::string s((size_t)k, 'A');
    for (int i = 0; i < k; i++) {
        const int bit = 2 * (k - 1 - i);
        s[(size_t)i] = "ACGT"[(w[W - 1 - (bit >> 6)] >> (bit & 63)) & 3u];
    }
    return s;
}

// ---- the yardstick
typedef std::vector<std::pair<std::string, int64_t>> Verts;
struct Ref {
    const Table& t;
    std::map<std::string, int64_t> rec;
    int k;
    Ref(const Table& tt, int kk) : t(tt), k(kk) { for (const auto& kv : t) { const int64_t i = (int64_t)rec.size(); rec[kv.first] = i; } }
    int64_t record(const std::string& v) const { auto it = rec.find(canonical(v)); return it == rec.end() ? -1 : it->second; }
    int32_t cov(const std::string& v, int c) const { return (int32_t)t.find(canonical(v))->second.cov[c]; }
    std::vector<std::string> adjacent(const std::string& v, bool fwd, int c) const {
        std::vector<std::string> out;
        auto it = t.find(canonical(v));
        if (it == t.end()) return out;
        const bool flip = canonical(v) != v;
        const unsigned e = it->second.edges[c];
        for (int b = 0; b < 4; b++) {
            const bool use_out = fwd != flip;
            const int rb = flip ? 3 - b : b;
            const bool has = use_out ? (e >> rb) & 1u : (e >> (4 + 3 - rb)) & 1u;
            if (!has) continue;
            out.push_back(fwd ? v.substr(1) + "ACGT"[b] : std::string(1, "ACGT"[b]) + v.substr(0, (size_t)k - 1));
        }
        return out;
    }
    // seek(seed), then next() / previous() on an engine of colour c: stop_colour >= 0: until a vertex covered there; target: until it
    struct Dir { Verts v; int end; bool npe; };
    Dir direction(const std::string& seed, bool fwd, int c, int64_t max_steps, int stop_colour, const std::string* target) const {
        Dir d; d.end = LDBG_CURSOR_END; d.npe = false;
        if (!is_bases(seed)) return d;
        std::set<std::string> seen;
        std::vector<std::string> nb = adjacent(seed, fwd, c);
        bool has = nb.size() == 1;
        std::string nxt = has ? nb[0] : std::string();
        while (true) {
            if (!has) { d.end = LDBG_CURSOR_END; return d; }
            if ((int64_t)d.v.size() >= max_steps) { d.end = LDBG_CURSOR_LIMIT; return d; }
            const std::string cur = nxt;
            d.v.push_back({cur, record(cur)});
            if (stop_colour >= 0) {
                if (record(cur) < 0) { d.end = LDBG_CURSOR_FAILED; d.npe = true; return d; }
                if (cov(cur, stop_colour) > 0) { d.end = LDBG_CURSOR_STOP; return d; }
            }
            if (target && cur == *target) { d.end = LDBG_CURSOR_STOP; return d; }
            nb = adjacent(cur, fwd, c);
            has = false;
            if (nb.size() == 1 && (record(nb[0]) < 0 || !seen.count(nb[0]))) {
                if (record(nb[0]) >= 0) seen.insert(nb[0]);
                nxt = nb[0]; has = true;
            }
        }
    }
};

static std::string to_contig(const Verts& v) {
    std::string s = v.empty() ? std::string() : v[0].first;
    for (size_t i = 1; i < v.size(); i++) s += v[i].first.back();
    return s;
}

struct Want {
    int status = 0; int64_t src = -1, dst = -1; int n_child = 0, n_parent = 0, st = 0, e0 = 0, e1 = 0;
    int64_t sum[NC] = {0, 0}, psum = 0;
    std::string a0, a1;
    Verts child, parent;
};

static Want call(const Ref& ref, const std::string& seed, int64_t ms) {
    Want w;
    const Ref::Dir rv = ref.direction(seed, false, 0, ms, 1, nullptr), fw = ref.direction(seed, true, 0, ms, 1, nullptr);
    w.child.assign(rv.v.rbegin(), rv.v.rend());
    w.child.push_back({seed, is_bases(seed) ? ref.record(seed) : -1});
    w.child.insert(w.child.end(), fw.v.begin(), fw.v.end());
    w.n_child = (int)w.child.size();
    if (rv.end == LDBG_CURSOR_STOP) w.src = rv.v.back().second;
    if (fw.end == LDBG_CURSOR_STOP) w.dst = fw.v.back().second;
    if (rv.npe || fw.npe) { w.status = LDBG_VARIANT_NULLPOINTER; return w; }
    if (rv.end == LDBG_CURSOR_LIMIT || fw.end == LDBG_CURSOR_LIMIT) { w.status = LDBG_VARIANT_LIMIT; return w; }
    if (rv.end != LDBG_CURSOR_STOP) { w.status = LDBG_VARIANT_NO_SOURCE; return w; }
    if (fw.end != LDBG_CURSOR_STOP) { w.status = LDBG_VARIANT_NO_DESTINATION; return w; }
    const Ref::Dir pv = ref.direction(rv.v.back().first, true, 1, ms, -1, &fw.v.back().first);
    w.parent.push_back(rv.v.back());
    w.parent.insert(w.parent.end(), pv.v.begin(), pv.v.end());
    w.n_parent = (int)w.parent.size();
    if (pv.end == LDBG_CURSOR_LIMIT) { w.status = LDBG_VARIANT_LIMIT; return w; }
    if (pv.end != LDBG_CURSOR_STOP) { w.status = LDBG_VARIANT_NOT_REACHED; return w; }
    w.status = LDBG_VARIANT_CALLED;
    for (const auto& v : w.child) for (int c = 0; c < NC; c++) w.sum[c] += ref.cov(v.first, c);
    for (const auto& v : w.parent) w.psum += ref.cov(v.first, 1);
    // trimToAlleles, statement by statement
    const std::string s0 = to_contig(w.child), s1 = to_contig(w.parent);
    int s0start = 0, s0end = (int)s0.size(), s1start = 0, s1end = (int)s1.size();
    for (int i = 0, j = 0; i < (int)s0.size() && j < (int)s1.size(); i++, j++)
        if (s0[(size_t)i] != s1[(size_t)j]) { s0start = i; s1start = j; break; }
    for (int i = (int)s0.size() - 1, j = (int)s1.size() - 1; i >= 0 && j >= 0; i--, j--)
        if (s0[(size_t)i] != s1[(size_t)j] || i == s0start - 1 || j == s1start - 1) { s0end = i + 1; s1end = j + 1; break; }
    w.st = s0start; w.e0 = s0end; w.e1 = s1end;
    w.a0 = s0.substr((size_t)s0start, (size_t)(s0end - s0start));
    w.a1 = s1.substr((size_t)s1start, (size_t)(s1end - s1start));
    return w;
}

static std::set<int> g_lengths;      // base counts of the contigs of called seeds, over all cases

static int run(const Table& t, int k, const std::vector<std::string>& seeds, int64_t max_steps, const char* slots, const char* what) {
    const int W = (k + 31) / 32;
    const std::string gp = std::string("/tmp/ldbg_variants_san_") + what + ".ctx";
    if (!write_ctx(t, k, gp)) return 1;
    if (slots) setenv("LDBG_CURSOR_SLOTS", slots, 1); else unsetenv("LDBG_CURSOR_SLOTS");
    Ref ref(t, k);
    ldbg_graph* g = nullptr;
    ldbg_engine* e[2] = {nullptr, nullptr};
    ldbg_status st = ldbg_graph_open(gp.c_str(), 0, &g);
    for (int c = 0; c < 2 && st == LDBG_OK; c++) {
        ldbg_engine_config cfg;
        ldbg_engine_config_default(&cfg);
        cfg.graph = g; cfg.traversal_colors[0] = c; cfg.n_traversal = 1; cfg.max_branch_length = 500;
        st = ldbg_engine_create(&cfg, &e[c]);
    }
    const int64_t n = (int64_t)seeds.size(), ms = max_steps > 0 ? max_steps : 500;
    std::string flat;
    for (const std::string& s : seeds) flat += s;
    bool same = st == LDBG_OK;
    int called = 0;
    for (int pass = 0; same && pass < 2; pass++) {                 // the second batch runs on the pools the first one left
        ldbg_variant_result* r = nullptr;
        st = ldbg_engine_variant_batch(e[0], e[1], flat.c_str(), n, 1, max_steps, 3ull, &r);
        if (st != LDBG_OK) { same = false; break; }
        int64_t ns = -1, ab = -1, ncv = -1, npv = -1; int m = 0, w = 0;
        st = ldbg_variant_result_sizes(r, &ns, &m, &ab, &ncv, &npv, &w);
        same = st == LDBG_OK && ns == n && m == 2 && w == W;
        const size_t N = (size_t)n + 1;
        std::vector<uint8_t> status(N), cflag(2 * N), pflag(N);
        std::vector<int64_t> src(N), dst(N), csum(2 * N), psum(N), aoff(2 * N + 1), coff(N), crec((size_t)ncv + 1), poff(N), prec((size_t)npv + 1);
        std::vector<int32_t> nch(N), npa(N), s0(N), e0(N), e1(N);
        std::vector<uint64_t> cw((size_t)ncv * (size_t)W + 1), pw((size_t)npv * (size_t)W + 1);
        std::vector<char> text((size_t)ab + 1);
        ldbg_variant_arrays a;
        a.status = status.data(); a.source_rec = src.data(); a.dest_rec = dst.data(); a.n_child = nch.data(); a.n_parent = npa.data();
        a.st = s0.data(); a.s0end = e0.data(); a.s1end = e1.data(); a.child_sum = csum.data(); a.child_flag = cflag.data();
        a.parent_sum = psum.data(); a.parent_flag = pflag.data(); a.allele_offsets = aoff.data(); a.alleles = text.data();
        a.child_offsets = coff.data(); a.child_words = cw.data(); a.child_rec = crec.data();
        a.parent_offsets = poff.data(); a.parent_words = pw.data(); a.parent_rec = prec.data();
        if (same) { st = ldbg_variant_result_get(r, &a); same = st == LDBG_OK && aoff[0] == 0 && aoff[2 * (size_t)n] == ab; }
        for (int64_t i = 0; same && i < n; i++) {
            const size_t u = (size_t)i;
            const Want w_ = call(ref, seeds[u], ms);
            same = status[u] == w_.status && src[u] == w_.src && dst[u] == w_.dst && nch[u] == w_.n_child && npa[u] == w_.n_parent && s0[u] == w_.st &&
                   e0[u] == w_.e0 && e1[u] == w_.e1 && csum[2 * u] == w_.sum[0] && csum[2 * u + 1] == w_.sum[1] && psum[u] == w_.psum && !cflag[2 * u] &&
                   !cflag[2 * u + 1] && !pflag[u] && std::string(text.data() + aoff[2 * u], (size_t)(aoff[2 * u + 1] - aoff[2 * u])) == w_.a0 &&
                   std::string(text.data() + aoff[2 * u + 1], (size_t)(aoff[2 * u + 2] - aoff[2 * u + 1])) == w_.a1 &&
                   coff[u + 1] - coff[u] == (int64_t)w_.child.size() && poff[u + 1] - poff[u] == (int64_t)(w_.parent.empty() ? 0 : w_.parent.size() - 1);
            for (size_t j = 0; same && j < w_.child.size(); j++) {
                const size_t at = (size_t)coff[u] + j;
                same = crec[at] == w_.child[j].second && (!is_bases(seeds[u]) || decode(&cw[at * (size_t)W], k, W) == w_.child[j].first);
            }
            for (size_t j = 1; same && j < w_.parent.size(); j++) {
                const size_t at = (size_t)poff[u] + j - 1;
                same = prec[at] == w_.parent[j].second && decode(&pw[at * (size_t)W], k, W) == w_.parent[j].first;
            }
            if (w_.status == LDBG_VARIANT_CALLED) {
                called++;
                g_lengths.insert(w_.n_child + k - 1); g_lengths.insert(w_.n_parent + k - 1);
            }
            if (!same) printf("%s: seed %lld (%s) differs: status %d, expected %d\n", what, (long long)i, seeds[u].c_str(), (int)status[u], w_.status);
        }
        ldbg_variant_result_free(r);
    }
    if (st != LDBG_OK) printf("%s: %s\n", what, ldbg_last_error());
    for (int c = 0; c < 2; c++) if (e[c]) ldbg_engine_destroy(e[c]);
    if (g) ldbg_graph_close(g);
    remove(gp.c_str());
    printf("%-10s k=%-3d seeds %-5lld max_steps %-4lld slots %-4s status %d called %d %s\n", what, k, (long long)n, (long long)max_steps, slots ? slots : "-", (int)st,
           called / 2, same ? "same" : "DIFFERENT");
    return same ? 0 : 1;
}

// parent and child genomes: clusters of substitutions less than k apart whose span makes contigs of 2k + 1 + span bases, an insertion
// and a deletion of one base
static void genomes(int k, const std::vector<int>& spans, std::string& mom, std::string& kid) {
    mom = rand_seq(3 * (size_t)k); kid = mom;
    for (int span : spans) {
        std::string seg = rand_seq((size_t)span + 1), alt = seg;
        for (int p = 0;; p = std::min(p + k - 1, span)) { alt[(size_t)p] = other(seg[(size_t)p]); if (p == span) break; }
        const std::string fl = rand_seq(3 * (size_t)k);
        mom += seg + fl; kid += alt + fl;
    }
    std::string fl = rand_seq(3 * (size_t)k);
    mom += fl; kid += std::string(1, 'G') + fl;             // the child has a base more
    fl = rand_seq(3 * (size_t)k);
    mom += std::string(1, 'T') + fl; kid += fl;             // ... and a base less
}

static std::vector<std::string> child_seeds(const Table& t, size_t n, int k) {
    std::vector<std::string> all, out;
    for (const auto& kv : t) if (kv.second.cov[0] > 0 && kv.second.cov[1] == 0) all.push_back(kv.first);
    for (size_t i = 0; i < n; i++) { const std::string& s = all[(i * 7) % all.size()]; out.push_back(i & 1u ? s : revcomp(s)); }
    if (n > 8) { out[1] = rand_seq((size_t)k); out[2] = std::string((size_t)k, 'N'); out[3] = out[4]; }
    return out;
}

int main() {
    int bad = 0;
    for (int lanes : {1, 64}) {
        ldbg_hostsim_set_lanes(lanes);
        g_rng = 0x9E3779B97F4A7C15ull;                   // the same inputs at either width
        for (int k : {21, 33}) {
            // contigs of 63, 64, 65, 127, 128 and 129 bases where 2k + 1 allows them
            std::vector<int> spans{0};
            for (int len : {63, 64, 65, 127, 128, 129}) if (len - 2 * k - 1 > 0) spans.push_back(len - 2 * k - 1);
            std::string mom, kid;
            genomes(k, spans, mom, kid);
            Table t;
            add_sequence(t, kid, k, 0);
            add_sequence(t, mom, k, 1);
            std::vector<std::string> every;
            for (const auto& kv : t) if (kv.second.cov[0] > 0 && kv.second.cov[1] == 0) every.push_back(kv.first);
            bad += run(t, k, every, 0, nullptr, "lengths");
            bad += run(t, k, child_seeds(t, 65, k), 0, nullptr, "pool");
            bad += run(t, k, child_seeds(t, 65, k), 0, "3", "reuse");                // a capped pool: 130 + 65 items through three slots
            bad += run(t, k, child_seeds(t, 65, k), 5, "3", "limit");
            bad += run(t, k, child_seeds(t, 1, k), 0, nullptr, "one seed");
            bad += run(t, k, {}, 0, nullptr, "empty");
            // records taken away: the child's cursor steps onto vertices without a record under the colour rule
            Table d = t;
            size_t q = 0;
            for (auto it = d.begin(); it != d.end(); q++) { if (q % 29 == 4) it = d.erase(it); else ++it; }
            bad += run(d, k, child_seeds(d, 65, k), 0, "3", "dangling");
        }
        for (int len : {63, 64, 65, 127, 128, 129})
            if (!g_lengths.count(len)) { printf("no called contig of %d bases\n", len); bad++; }
    }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
