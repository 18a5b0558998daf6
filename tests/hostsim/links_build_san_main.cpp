// TEST-ONLY stand-alone program over the host simulation of libldbg (make -C corticall_amd/csrc hostsim-san-links): builds graphs with
// ldbg_graph_build and threads reads through them with ldbg_links_build_ctp / ldbg_links_build so that linkbuild.cpp runs under
// AddressSanitizer and UBSan without loading the library into another process.  Prints the link counts; exits non-zero on an error.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../include/ldbg.h"

extern "C" void ldbg_hostsim_set_lanes(int n);

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_rng >> 33); }
static std::string rand_seq(size_t n) { std::string s(n, 'A'); for (auto& c : s) c = "ACGT"[rnd() & 3]; return s; }
// n bases with one stretch copied to two other places: forks and convergences
static std::string with_repeat(size_t n, size_t rep) {
    std::string a = rand_seq(n - 2 * rep);
    const std::string x = a.substr(n / 5, rep);
    return a.substr(0, a.size() / 2) + x + a.substr(a.size() / 2, a.size() / 2 - 100) + x + a.substr(a.size() - 100);
}

struct Reads { std::string text; std::vector<int64_t> offs{0}; void add(const std::string& s) { text += s; offs.push_back((int64_t)text.size()); } };

// want: the status both entry points must return
static int run(const std::string& genome, int k, const Reads& r, const int64_t* offs, int64_t n, ldbg_status want, const char* what) {
    const int64_t goffs[2] = {0, (int64_t)genome.size()};
    const ldbg_build_sample s{"s", genome.c_str(), goffs, 1};
    ldbg_graph* g = nullptr;
    if (ldbg_graph_build(&s, 1, k, 0, 0, &g) != LDBG_OK) { printf("%s: no graph\n", what); return 1; }
    int64_t nk = -1, nl = -1, nk2 = -1, nl2 = -1;
    const std::string path = std::string("/tmp/ldbg_links_san_") + what + ".ctp.gz";
    const ldbg_status st = ldbg_links_build_ctp(g, "s", r.text.c_str(), offs, n, 0, path.c_str(), &nk, &nl);
    remove(path.c_str());
    ldbg_links* l = nullptr;
    const ldbg_status st2 = ldbg_links_build(g, "s", r.text.c_str(), offs, n, 0, &l);
    if (l) { ldbg_links_info(l, nullptr, nullptr, nullptr, nullptr, &nk2, &nl2); ldbg_links_close(l); }
    ldbg_graph_close(g);
    printf("%-12s k=%-3d status %d/%d k-mers %lld/%lld links %lld/%lld\n", what, k, (int)st, (int)st2, (long long)nk, (long long)nk2, (long long)nl, (long long)nl2);
    return st == want && st2 == want && nk == nk2 && nl == nl2 && (want != LDBG_OK || nl > 0) ? 0 : 1;
}
static int run(const std::string& genome, int k, const Reads& r, ldbg_status want, const char* what) {
    return run(genome, k, r, r.offs.data(), (int64_t)r.offs.size() - 1, want, what);
}

int main() {
    int bad = 0;
    for (int lanes : {1, 64}) {
        ldbg_hostsim_set_lanes(lanes);
        g_rng = 0x9E3779B97F4A7C15ull;                   // the same inputs at either width
        const std::string g1 = with_repeat(1200, 60);
        Reads tiled;                                      // reads of 100 every 25, one twice, short ones, an empty one
        for (size_t i = 0; i + 100 <= g1.size(); i += 25) tiled.add(g1.substr(i, 100));
        tiled.add(g1.substr(50, 100)); tiled.add("ACG"); tiled.add("");
        bad += run(g1, 9, tiled, LDBG_OK, "tiled");
        const std::string g2 = with_repeat(4400, 60);
        Reads lng;                                        // one read of 4097 windows
        lng.add(g2.substr(150, 4097 + 11 - 1));
        bad += run(g2, 11, lng, LDBG_OK, "w4097");
        const std::string g3 = with_repeat(900, 90);
        Reads wide;                                       // three-word k-mers
        for (size_t i = 0; i + 200 <= g3.size(); i += 50) wide.add(g3.substr(i, 200));
        bad += run(g3, 65, wide, LDBG_OK, "k65");
        Reads err = tiled;                                // a window that is no k-mer of the graph: the call fails, cleanly
        err.add(g1.substr(300, 40) + "N" + g1.substr(341, 40));
        bad += run(g1, 9, err, LDBG_ERR_CORTEXJDK, "absent");
        const int64_t huge[2] = {0, (1ll << 31) + 9};     // refused from the offsets alone: the text is never read
        bad += run(g1, 9, tiled, huge, 1, LDBG_ERR_UNSUPPORTED, "refused");
    }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
