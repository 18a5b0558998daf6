// TEST-ONLY stand-alone program over the host simulation of libldbg (make -C corticall_amd/csrc hostsim-san-build): builds a few
// graphs through ldbg_graph_build_ctx / ldbg_graph_build so that build.cpp and the device-key entry of sort.cpp run under
// AddressSanitizer and UBSan without loading the library into another process.  Prints the record counts; exits non-zero on an error.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../include/ldbg.h"

extern "C" void ldbg_hostsim_set_lanes(int n);

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(g_rng >> 33); }
static std::string rand_seq(size_t n) { std::string s(n, 'A'); for (auto& c : s) c = "ACGT"[rnd() & 3]; return s; }

struct Sample { std::string name, text; std::vector<int64_t> offs{0}; void add(const std::string& s) { text += s; offs.push_back((int64_t)text.size()); } };

static int run(const std::vector<Sample>& ss, int k, int flags, const char* what) {
    std::vector<ldbg_build_sample> in;
    for (auto& s : ss) in.push_back({s.name.c_str(), s.text.c_str(), s.offs.data(), (int64_t)s.offs.size() - 1});
    int64_t n = -1, n2 = -1;
    const std::string path = std::string("/tmp/ldbg_build_san_") + what + ".ctx";
    ldbg_status st = ldbg_graph_build_ctx(in.data(), (int)in.size(), k, flags, 0, path.c_str(), &n);
    remove(path.c_str());
    ldbg_graph* g = nullptr;
    ldbg_status st2 = ldbg_graph_build(in.data(), (int)in.size(), k, flags, 0, &g);
    if (g) { ldbg_graph_info(g, nullptr, nullptr, nullptr, &n2, nullptr); ldbg_graph_close(g); }
    printf("%-12s k=%-3d status %d/%d records %lld/%lld\n", what, k, (int)st, (int)st2, (long long)n, (long long)n2);
    return st == LDBG_OK && st2 == LDBG_OK && n == n2 ? 0 : 1;
}

int main() {
    int bad = 0;
    for (int lanes : {1, 64}) {
        ldbg_hostsim_set_lanes(lanes);
        g_rng = 0x9E3779B97F4A7C15ull;                   // the same inputs at either width
        Sample one{"s"};                                  // 70,000 windows, one colour
        one.add(rand_seq(23333 + 30)); one.add(rand_seq(46667 + 30));
        bad += run({one}, 31, 0, "shape70000");
        Sample a{"a"}, b{"b"}, none{"none"};              // a heavy k-mer, reads of k..k+5, a sample without sequences, three-word k-mers
        a.add(std::string(20000 + 65, 'A'));
        const std::string g = rand_seq(3000);
        for (int i = 0; i < 2000; i++) b.add(g.substr(rnd() % 2900, 65 + rnd() % 6));
        b.add("acgt"); b.add("");
        bad += run({a, none, b}, 65, 0, "heavy_reads");
        Sample n{"n"};                                    // LDBG_BUILD_SPLIT_NON_ACGT
        n.add("N" + rand_seq(200) + "NNNN" + rand_seq(40) + "." + rand_seq(4) + "\n" + rand_seq(100) + "N");
        bad += run({n, one}, 31, LDBG_BUILD_SPLIT_NON_ACGT, "split");
        bad += run({n}, 31, 0, "refused") == 0;           // without the flag the call fails (LDBG_ERR_CORTEXJDK), cleanly
    }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
