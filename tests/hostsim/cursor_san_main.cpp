// TEST-ONLY stand-alone program over the host simulation of libldbg (make -C corticall_amd/csrc hostsim-san-cursor): writes small one-colour
// graphs with their edges, advances cursors over them in batches with ldbg_engine_cursor_batch so that the batch kernels of cursor.cpp run
// under AddressSanitizer and UBSan without loading the library into another process, and checks every vertex, count, end reason and status
// against the cursor's loops restated here on strings (TraversalEngine.java:128-145 over :241-339, no links: the single next vertex is
// taken while it is not in `seen`).  Prints one line per case; exits non-zero on an error.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
static std::string revcomp(const std::string& s) {
    std::string r(s.rbegin(), s.rend());
    for (char& c : r) c = comp(c);
    return r;
}
static bool is_bases(const std::string& s) { return s.find_first_not_of("ACGT") == std::string::npos; }
static std::string canonical(const std::string& s) { const std::string r = revcomp(s); return r < s ? r : s; }

static void put32(std::vector<uint8_t>& o, uint32_t v) { for (int i = 0; i < 4; i++) o.push_back((uint8_t)(v >> (8 * i))); }
static void put64(std::vector<uint8_t>& o, uint64_t v) { for (int i = 0; i < 8; i++) o.push_back((uint8_t)(v >> (8 * i))); }

// canonical k-mer -> edge byte (high nibble: in-edges, bit 3 - base; low nibble: out-edges, bit base; CortexRecord.java:214-275)
typedef std::map<std::string, uint8_t> Table;

static void add_sequence(Table& t, const std::string& s, int k) {
    for (size_t i = 0; i + (size_t)k <= s.size(); i++) t[canonical(s.substr(i, (size_t)k))] |= 0;
    for (size_t i = 0; i + (size_t)k + 1 <= s.size(); i++) {
        const std::string a = s.substr(i, (size_t)k), b = s.substr(i + 1, (size_t)k);
        if (canonical(a) == a) t[a] |= (uint8_t)(1u << idx(b.back()));
        else t[revcomp(a)] |= (uint8_t)(1u << (4 + 3 - idx(comp(b.back()))));
        if (canonical(b) == b) t[b] |= (uint8_t)(1u << (4 + 3 - idx(a[0])));
        else t[revcomp(b)] |= (uint8_t)(1u << idx(comp(a[0])));
    }
}

static bool write_ctx(const Table& t, int k, const std::string& path) {
    const int W = (k + 31) / 32;
    std::vector<uint8_t> o;
    o.insert(o.end(), {'C', 'O', 'R', 'T', 'E', 'X'});
    put32(o, 6); put32(o, (uint32_t)k); put32(o, (uint32_t)W); put32(o, 1);
    put32(o, 0); put64(o, 0);
    put32(o, 1); o.push_back('s');
    for (int c = 0; c < 16; c++) o.push_back(0);
    put32(o, 0); put32(o, 0); put32(o, 0); put32(o, 0);
    o.insert(o.end(), {'C', 'O', 'R', 'T', 'E', 'X'});
    for (const auto& kv : t) {
        std::vector<uint64_t> w((size_t)W, 0);
        for (int i = 0; i < k; i++) {
            const int bit = 2 * (k - 1 - i);
            w[(size_t)(W - 1 - (bit >> 6))] |= (uint64_t)idx(kv.first[(size_t)i]) << (bit & 63);
        }
        for (uint64_t x : w) put64(o, x);
        put32(o, 1);
        o.push_back(kv.second);
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
struct Ref {
    const Table& t;
    std::map<std::string, int64_t> rec;
    int k;
    Ref(const Table& tt, int kk) : t(tt), k(kk) { for (const auto& kv : t) { const int64_t i = (int64_t)rec.size(); rec[kv.first] = i; } }
    int64_t record(const std::string& v) const { auto it = rec.find(canonical(v)); return it == rec.end() ? -1 : it->second; }
    // the vertices after (before) v, from the edges of its record in v's orientation
    std::vector<std::string> adjacent(const std::string& v, bool fwd) const {
        std::vector<std::string> out;
        auto it = t.find(canonical(v));
        if (it == t.end()) return out;
        const bool flip = canonical(v) != v;
        const unsigned e = it->second;
        for (int b = 0; b < 4; b++) {
            // forward from v: out-edges of the record, or (flipped) its in-edges complemented; backwards the mirror
            const bool use_out = fwd != flip;
            const int rb = flip ? 3 - b : b;
            const bool has = use_out ? (e >> rb) & 1u : (e >> (4 + 3 - rb)) & 1u;
            if (!has) continue;
            out.push_back(fwd ? v.substr(1) + "ACGT"[b] : std::string(1, "ACGT"[b]) + v.substr(0, (size_t)k - 1));
        }
        return out;
    }
    struct Dir { std::vector<std::pair<std::string, int64_t>> v; int end; };
    Dir direction(const std::string& seed, bool fwd, int64_t max_steps) const {
        Dir d; d.end = LDBG_CURSOR_END;
        if (!is_bases(seed)) return d;
        std::set<std::string> seen;
        std::vector<std::string> nb = adjacent(seed, fwd);
        bool has = nb.size() == 1;
        std::string nxt = has ? nb[0] : std::string();
        while (true) {
            if (!has) { d.end = LDBG_CURSOR_END; return d; }
            if ((int64_t)d.v.size() >= max_steps) { d.end = LDBG_CURSOR_LIMIT; return d; }
            const std::string cur = nxt;
            d.v.push_back({cur, record(cur)});
            nb = adjacent(cur, fwd);
            has = false;
            if (nb.size() == 1 && (record(nb[0]) < 0 || !seen.count(nb[0]))) {
                if (record(nb[0]) >= 0) seen.insert(nb[0]);
                nxt = nb[0]; has = true;
            }
        }
    }
};

static int run(Table t, int k, const std::vector<std::string>& seeds, int64_t max_steps, const char* slots, const char* epoch0, const char* what) {
    const int W = (k + 31) / 32;
    const std::string gp = std::string("/tmp/ldbg_cursor_san_") + what + ".ctx";
    if (!write_ctx(t, k, gp)) return 1;
    if (slots) setenv("LDBG_CURSOR_SLOTS", slots, 1); else unsetenv("LDBG_CURSOR_SLOTS");
    if (epoch0) setenv("LDBG_CURSOR_EPOCH0", epoch0, 1); else unsetenv("LDBG_CURSOR_EPOCH0");
    Ref ref(t, k);
    ldbg_graph* g = nullptr;
    ldbg_engine* e = nullptr;
    ldbg_status st = ldbg_graph_open(gp.c_str(), 0, &g);
    if (st == LDBG_OK) {
        ldbg_engine_config cfg;
        ldbg_engine_config_default(&cfg);
        cfg.graph = g; cfg.traversal_colors[0] = 0; cfg.n_traversal = 1; cfg.max_branch_length = 500;
        st = ldbg_engine_create(&cfg, &e);
    }
    const int64_t n = (int64_t)seeds.size();
    std::string flat;
    for (const std::string& s : seeds) flat += s;
    bool same = st == LDBG_OK;
    int64_t vertices = 0;
    const int64_t ms = max_steps > 0 ? max_steps : 500;
    for (int pass = 0; same && pass < 2; pass++)                 // the second batch runs on the pool the first one left
        for (int dir : {LDBG_DIR_BOTH, LDBG_DIR_FORWARD, LDBG_DIR_REVERSE}) {
            ldbg_cursor_result* r = nullptr;
            st = ldbg_engine_cursor_batch(e, flat.c_str(), n, dir, max_steps, nullptr, &r);
            if (st != LDBG_OK) { same = false; break; }
            int64_t ns = -1, nv = -1; int w = 0;
            st = ldbg_cursor_result_sizes(r, &ns, &nv, &w);
            std::vector<int64_t> off((size_t)n + 1), rec((size_t)nv + 1), srec((size_t)n + 1);
            std::vector<uint64_t> words((size_t)nv * (size_t)W + 1);
            std::vector<int32_t> nr((size_t)n + 1), nf((size_t)n + 1);
            std::vector<uint8_t> er((size_t)n + 1), ef((size_t)n + 1), stt((size_t)n + 1);
            if (st == LDBG_OK) st = ldbg_cursor_result_get(r, off.data(), words.data(), rec.data(), nr.data(), nf.data(), srec.data(), er.data(), ef.data(), stt.data());
            same = st == LDBG_OK && ns == n && w == W && off[0] == 0 && off[(size_t)n] == nv;
            for (int64_t i = 0; same && i < n; i++) {
                const std::string& s = seeds[(size_t)i];
                Ref::Dir rv, fw;
                rv.end = fw.end = LDBG_CURSOR_END;
                if (dir != LDBG_DIR_FORWARD) rv = ref.direction(s, false, ms);
                if (dir != LDBG_DIR_REVERSE) fw = ref.direction(s, true, ms);
                std::vector<std::pair<std::string, int64_t>> want(rv.v.rbegin(), rv.v.rend());
                const int64_t sr = is_bases(s) ? ref.record(s) : -1;
                if (dir == LDBG_DIR_BOTH) want.push_back({is_bases(s) ? s : std::string((size_t)k, 'A'), sr});
                want.insert(want.end(), fw.v.begin(), fw.v.end());
                same = nr[(size_t)i] == (int32_t)rv.v.size() && nf[(size_t)i] == (int32_t)fw.v.size() && er[(size_t)i] == rv.end && ef[(size_t)i] == fw.end &&
                       stt[(size_t)i] == LDBG_CURSOR_OK && srec[(size_t)i] == sr && off[(size_t)i + 1] - off[(size_t)i] == (int64_t)want.size();
                for (size_t j = 0; same && j < want.size(); j++) {
                    const int64_t at = off[(size_t)i] + (int64_t)j;
                    same = rec[(size_t)at] == want[j].second && decode(&words[(size_t)at * (size_t)W], k, W) == want[j].first;
                }
                if (!same) printf("%s: seed %lld (%s) direction %d differs\n", what, (long long)i, s.c_str(), dir);
            }
            vertices += nv;
            ldbg_cursor_result_free(r);
        }
    if (st != LDBG_OK) printf("%s: %s\n", what, ldbg_last_error());
    if (e) ldbg_engine_destroy(e);
    if (g) ldbg_graph_close(g);
    remove(gp.c_str());
    printf("%-10s k=%-3d seeds %-5lld max_steps %-4lld slots %-4s status %d vertices %lld %s\n", what, k, (long long)n, (long long)max_steps, slots ? slots : "-", (int)st,
           (long long)vertices, same ? "same" : "DIFFERENT");
    return same ? 0 : 1;
}

static std::vector<std::string> seeds_of(const Table& t, size_t n, int k) {
    std::vector<std::string> all, out;
    for (const auto& kv : t) all.push_back(kv.first);
    for (size_t i = 0; i < n; i++) { const std::string& s = all[rnd() % all.size()]; out.push_back(rnd() & 1u ? s : revcomp(s)); }
    if (n > 8) { out[1] = rand_seq((size_t)k); out[2] = std::string((size_t)k, 'N'); out[3] = out[4]; }
    return out;
}

int main() {
    int bad = 0;
    for (int lanes : {1, 64}) {
        ldbg_hostsim_set_lanes(lanes);
        g_rng = 0x9E3779B97F4A7C15ull;                   // the same inputs at either width
        for (int k : {21, 33}) {
            // a genome with a repeat met twice (forks) and a tandem repeat (a cycle)
            const std::string rep = rand_seq((size_t)k + 9), unit = rand_seq(7);
            const std::string genome = rand_seq(150) + rep + rand_seq(120) + unit + unit + unit + unit + unit + unit + unit + rand_seq(100) + rep + rand_seq(90);
            Table t;
            add_sequence(t, genome, k);
            add_sequence(t, rand_seq(60), k);
            bad += run(t, k, seeds_of(t, 65, k), 0, nullptr, nullptr, "pool");
            bad += run(t, k, seeds_of(t, 65, k), 0, "3", nullptr, "reuse");                // a capped pool: 130 items through three slots
            bad += run(t, k, seeds_of(t, 65, k), 0, "1", "16380", "wrap");                 // the epochs wrap around after three items
            bad += run(t, k, seeds_of(t, 65, k), 1, "3", nullptr, "one step");
            bad += run(t, k, seeds_of(t, 65, k), 1 << 20, "1", nullptr, "large");          // tables of 2^22 entries
            bad += run(t, k, seeds_of(t, 1, k), 7, nullptr, nullptr, "one seed");
            bad += run(t, k, {}, 0, nullptr, nullptr, "empty");
            // records taken away: edges dangle, cursors step onto vertices without a record
            Table d = t;
            size_t q = 0;
            for (auto it = d.begin(); it != d.end(); q++) { if (q % 9 == 4) it = d.erase(it); else ++it; }
            bad += run(d, k, seeds_of(d, 65, k), 0, "3", nullptr, "dangling");
        }
    }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
