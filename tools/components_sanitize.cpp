// Sanitizer check of schpf_debug_components and schpf_debug_cluster_graph, the host restatements of the connected components
// and of the cluster graph: a stand-alone program, CPU only -- no GPU is opened.  It labels a path whose
// vertices are numbered at random, the same path stored in order, a hub of degree n - 1, two cliques joined through a vertex
// of another group (`within`), a graph without entries and one of a diagonal only; tabulates a ring of cliques with every
// group its own clique, with one group, with labels of -1 and without values; and checks that refused calls leave their
// outputs.  Build and run from the repository root (host code only, AddressSanitizer and UBSan on the host side):
//
//   hipcc -std=c++17 -O1 -g --offload-host-only -x hip -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tools/components_sanitize.cpp schpf_amd/csrc/host.cpp schpf_amd/csrc/plan.cpp schpf_amd/csrc/policy.cpp \
//       -o components_sanitize && ./components_sanitize
//
// Exit status 0 and "components_sanitize ok" when the results are right and the sanitizers saw nothing.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
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

// the entries (u, v) and (v, u) of every pair, rows in order, columns as they come
Graph from_pairs(int n, const std::vector<std::pair<int, int>> &pairs)
{
    std::vector<std::vector<int32_t>> rows((size_t)n);
    for (const auto &p : pairs) {
        rows[(size_t)p.first].push_back(p.second);
        rows[(size_t)p.second].push_back(p.first);
    }
    Graph g;
    g.n = n;
    g.indptr.push_back(0);
    for (int i = 0; i < n; ++i) {
        for (int32_t j : rows[(size_t)i]) {
            g.indices.push_back(j);
            g.data.push_back(0.5 + 0.125 * ((i + j) % 5));
        }
        g.indptr.push_back((int64_t)g.indices.size());
    }
    return g;
}

int components(const Graph &g, const int32_t *within, std::vector<int32_t> &comp, int64_t stats[6])
{
    comp.assign((size_t)g.n, -7);
    std::fill(stats, stats + 6, (int64_t)-7);
    return schpf_debug_components(g.n, g.indptr.data(), g.indices.data(), within, comp.data(), stats);
}

int expect(const char *what, bool ok)
{
    if (!ok) std::printf("%s: wrong (%s)\n", what, schpf_last_error());
    return ok ? 0 : 1;
}

}  // namespace

int main()
{
    int failures = 0;
    std::vector<int32_t> comp;
    int64_t stats[6];

    // a path of 4 097 vertices, numbered by a multiplicative walk (a permutation: 4 097 = 17 * 241, 5 is coprime to it)
    const int n = 4097;
    std::vector<std::pair<int, int>> pairs;
    for (int s = 0; s + 1 < n; ++s) pairs.emplace_back((int)((int64_t)s * 5 % n), (int)((int64_t)(s + 1) * 5 % n));
    failures += expect("shuffled path", components(from_pairs(n, pairs), nullptr, comp, stats) == 0 && stats[0] == 1 &&
                                            stats[1] == n && stats[2] == 0 && stats[3] == 2 * (n - 1) &&
                                            std::count(comp.begin(), comp.end(), 0) == n);
    pairs.clear();
    for (int s = 0; s + 1 < n; ++s) pairs.emplace_back(s, s + 1);
    Graph path = from_pairs(n, pairs);
    failures += expect("path in order", components(path, nullptr, comp, stats) == 0 && stats[0] == 1 && stats[1] == n);

    // within: the path cut into runs of 100, every 50th vertex in no group
    std::vector<int32_t> within((size_t)n);
    for (int i = 0; i < n; ++i) within[(size_t)i] = i % 50 == 0 ? -1 : i / 100;
    int ok = components(path, within.data(), comp, stats) == 0;
    // runs 1 .. 49 and 51 .. 99 of every hundred, the vertices of -1 alone: labels ascend along the path
    for (int i = 1; ok && i < n; ++i) {
        const bool joined = within[(size_t)i] >= 0 && within[(size_t)i] == within[(size_t)i - 1];
        ok = comp[(size_t)i] == comp[(size_t)i - 1] + (joined ? 0 : 1);
    }
    failures += expect("path within groups", ok && stats[0] == comp.back() + 1 && stats[1] == 49);

    // a hub of degree n - 1
    pairs.clear();
    for (int j = 1; j < 5000; ++j) pairs.emplace_back(0, j);
    failures += expect("hub", components(from_pairs(5000, pairs), nullptr, comp, stats) == 0 && stats[0] == 1 && stats[1] == 5000);

    // two cliques of 6 joined only through vertex 12, which belongs to another group with vertex 13
    pairs.clear();
    for (int lo : {0, 6})
        for (int x = 0; x < 6; ++x)
            for (int y = x + 1; y < 6; ++y) pairs.emplace_back(lo + x, lo + y);
    pairs.emplace_back(5, 12);
    pairs.emplace_back(6, 12);
    pairs.emplace_back(12, 13);
    const Graph cliques = from_pairs(14, pairs);
    std::vector<int32_t> group(14, 0);
    group[12] = group[13] = 1;
    failures += expect("cliques, whole graph", components(cliques, nullptr, comp, stats) == 0 && stats[0] == 1);
    ok = components(cliques, group.data(), comp, stats) == 0 && stats[0] == 3 && stats[1] == 6 && stats[2] == 0;
    for (int i = 0; ok && i < 14; ++i) ok = comp[(size_t)i] == (i < 6 ? 0 : i < 12 ? 1 : 2);
    failures += expect("cliques split within their group", ok);

    // no entries, a diagonal only, n = 0
    Graph none;
    none.n = 37;
    none.indptr.assign(38, 0);
    failures += expect("no entries", components(none, nullptr, comp, stats) == 0 && stats[0] == 37 && stats[1] == 1 &&
                                         stats[2] == 37 && stats[3] == 0 && comp[36] == 36);
    Graph diagonal;
    diagonal.n = 9;
    for (int i = 0; i <= 9; ++i) diagonal.indptr.push_back(i);
    for (int i = 0; i < 9; ++i) diagonal.indices.push_back(i);
    failures += expect("diagonal", components(diagonal, nullptr, comp, stats) == 0 && stats[0] == 9 && stats[3] == 0);
    failures += expect("n = 0", schpf_debug_components(0, nullptr, nullptr, nullptr, nullptr, stats) == 0 && stats[0] == 0);

    // refused: outputs untouched
    Graph bad = cliques;
    bad.indices[3] = 14;
    failures += expect("column refused", components(bad, nullptr, comp, stats) != 0 && comp[0] == -7 && stats[0] == -7);
    group[4] = -2;
    failures += expect("within refused", components(cliques, group.data(), comp, stats) != 0 && comp[0] == -7 && stats[0] == -7);
    group[4] = 0;

    // the cluster graph of the cliques: groups 0, 1 (the cliques) and 2 (the two others)
    std::vector<int32_t> labels(14);
    for (int i = 0; i < 14; ++i) labels[(size_t)i] = i < 6 ? 0 : i < 12 ? 1 : 2;
    std::vector<int64_t> cells(3, -7), count(9, -7), weight(9, -7);
    double wmax = -7.0;
    ok = schpf_debug_cluster_graph(14, cliques.indptr.data(), cliques.indices.data(), cliques.data.data(), labels.data(), 3,
                                   cells.data(), count.data(), weight.data(), &wmax) == 0;
    const int64_t want[9] = {30, 0, 1, 0, 30, 1, 1, 1, 2};
    failures += expect("cluster graph", ok && std::equal(count.begin(), count.end(), want) && cells[0] == 6 && cells[2] == 2 &&
                                            wmax == 1.0 && weight[0] > 0 && weight[1] == 0);
    labels[3] = -1;   // a vertex in no group: its 5 + 5 entries leave the first clique's cell
    ok = schpf_debug_cluster_graph(14, cliques.indptr.data(), cliques.indices.data(), nullptr, labels.data(), 3, cells.data(),
                                   count.data(), weight.data(), &wmax) == 0;
    failures += expect("cluster graph without values", ok && count[0] == 20 && cells[0] == 5 && weight[0] == count[0] << 30 && wmax == 1.0);
    std::vector<int32_t> one(14, 0);
    ok = schpf_debug_cluster_graph(14, cliques.indptr.data(), cliques.indices.data(), cliques.data.data(), one.data(), 1,
                                   cells.data(), count.data(), nullptr, &wmax) == 0;
    failures += expect("one group", ok && count[0] == (int64_t)cliques.indices.size() && cells[0] == 14);
    labels[3] = 3;
    count[0] = -7;
    failures += expect("labels refused", schpf_debug_cluster_graph(14, cliques.indptr.data(), cliques.indices.data(),
                                                                   cliques.data.data(), labels.data(), 3, cells.data(),
                                                                   count.data(), weight.data(), &wmax) != 0 && count[0] == -7);

    std::printf(failures ? "components_sanitize FAILED (%d)\n" : "components_sanitize ok\n", failures);
    return failures ? 1 : 0;
}
