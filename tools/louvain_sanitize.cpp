// Sanitizer check of schpf_debug_louvain, the host restatement of the Louvain clustering: a stand-alone
// program, CPU only -- no GPU is opened.  It clusters cliques joined in a ring and a hub of degree n - 1, and checks what
// comes back.  Build and run from the repository root (host code only, AddressSanitizer and UBSan on the host side):
//
//   hipcc -std=c++17 -O1 -g --offload-host-only -x hip -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tools/louvain_sanitize.cpp schpf_amd/csrc/host.cpp schpf_amd/csrc/plan.cpp schpf_amd/csrc/policy.cpp \
//       -o louvain_sanitize && ./louvain_sanitize
//
// Exit status 0 and "louvain_sanitize ok" when the labels are right and the sanitizers saw nothing.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../include/schpf_hip.h"

namespace schpf {
thread_local std::string g_err;   // the library keeps it in capi.hip, which is not part of this program
}
extern "C" const char *schpf_last_error(void) { return schpf::g_err.c_str(); }

namespace {

struct Graph {
    int n = 0;
    std::vector<int64_t> indptr;
    std::vector<int32_t> indices;
    std::vector<double> data;
};

// dense symmetric weights -> CSR, columns ascending
Graph from_dense(int n, const std::vector<double> &w)
{
    Graph g;
    g.n = n;
    g.indptr.push_back(0);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j)
            if (w[(size_t)i * n + j] > 0.0) {
                g.indices.push_back(j);
                g.data.push_back(w[(size_t)i * n + j]);
            }
        g.indptr.push_back((int64_t)g.indices.size());
    }
    return g;
}

int run(const Graph &g, double gamma, std::vector<int32_t> &labels, int64_t stats[4])
{
    labels.assign((size_t)g.n, -7);
    return schpf_debug_louvain(g.n, g.indptr.data(), g.indices.data(), g.data.data(), gamma, labels.data(), stats);
}

}  // namespace

int main()
{
    int failures = 0;
    std::vector<int32_t> labels;
    int64_t stats[4];

    // 12 cliques of 8 with unit weights, the last vertex of each joined to the first of the next by 1e-3
    const int cliques = 12, size = 8, n = cliques * size;
    std::vector<double> w((size_t)n * n, 0.0);
    for (int b = 0; b < cliques; ++b) {
        for (int x = 0; x < size; ++x)
            for (int y = 0; y < size; ++y)
                if (x != y) w[(size_t)(b * size + x) * n + b * size + y] = 1.0;
        const int u = b * size + size - 1, v = ((b + 1) % cliques) * size;
        w[(size_t)u * n + v] = w[(size_t)v * n + u] = 1e-3;
    }
    const Graph ring = from_dense(n, w);
    if (run(ring, 1.0, labels, stats) != 0) {
        std::printf("clique ring: %s\n", schpf_last_error());
        ++failures;
    } else {
        for (int i = 0; i < n; ++i) failures += labels[(size_t)i] != i / size;
        failures += stats[0] != cliques;
        std::printf("clique ring: %lld communities, %lld levels, %lld rounds\n", (long long)stats[0], (long long)stats[1],
                    (long long)stats[2]);
    }

    // a hub of degree n - 1 over a ring of the other vertices
    const int hn = 5000;
    Graph hub;
    hub.n = hn;
    hub.indptr.push_back(0);
    auto add = [&](int j, double v) {
        hub.indices.push_back(j);
        hub.data.push_back(v);
    };
    for (int j = 1; j < hn; ++j) add(j, 0.01);
    hub.indptr.push_back((int64_t)hub.indices.size());
    for (int i = 1; i < hn; ++i) {
        const int left = i == 1 ? hn - 1 : i - 1, right = i == hn - 1 ? 1 : i + 1;
        add(0, 0.01);
        add(left < right ? left : right, 1.0 + 0.001 * ((i + (left < right ? left : right)) % 7));
        add(left < right ? right : left, 1.0 + 0.001 * ((i + (left < right ? right : left)) % 7));
        hub.indptr.push_back((int64_t)hub.indices.size());
    }
    if (run(hub, 1.0, labels, stats) != 0) {
        std::printf("hub: %s\n", schpf_last_error());
        ++failures;
    } else {
        for (int i = 0; i < hn; ++i) failures += labels[(size_t)i] < 0 || labels[(size_t)i] >= stats[0];
        failures += !(stats[0] > 1 && stats[0] < hn && stats[1] >= 1);
        std::printf("hub: %lld communities, %lld levels, %lld rounds\n", (long long)stats[0], (long long)stats[1],
                    (long long)stats[2]);
    }

    // a refused call leaves its outputs
    Graph bad = ring;
    bad.data[5] = -1.0;
    stats[0] = -7;
    failures += run(bad, 1.0, labels, stats) == 0 || labels[0] != -7 || stats[0] != -7;

    std::printf(failures ? "louvain_sanitize FAILED (%d)\n" : "louvain_sanitize ok\n", failures);
    return failures ? 1 : 0;
}
