// Sanitizer check of schpf_debug_geodesic, the host restatement of the shortest-path distances: a stand-alone
// program, CPU only -- no GPU is opened.  It walks a path whose vertices are numbered at random with stored zeros on it, a
// grid (Manhattan distances), a graph with entries stored twice under different lengths, a directed cycle beside an
// unreachable part, lengths that overflow, root sets that are empty, repeated and joint, a graph without values and one
// without entries; and checks that refused calls leave their outputs.  Build and run from the repository root (host code
// only, AddressSanitizer and UBSan on the host side):
//
//   hipcc -std=c++17 -O1 -g --offload-host-only -x hip -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tools/geodesic_sanitize.cpp schpf_amd/csrc/host.cpp schpf_amd/csrc/plan.cpp schpf_amd/csrc/policy.cpp \
//       -o geodesic_sanitize && ./geodesic_sanitize
//
// Exit status 0 and "geodesic_sanitize ok" when the results are right and the sanitizers saw nothing.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../include/schpf_hip.h"

namespace schpf {
thread_local std::string g_err;   // the library keeps it in capi.hip, which is not part of this program
}
extern "C" const char *schpf_last_error(void) { return schpf::g_err.c_str(); }

namespace {

const double INF = std::numeric_limits<double>::infinity();

struct Edge {
    int from, to;
    double length;
};

struct Graph {
    int n = 0;
    std::vector<int64_t> indptr;
    std::vector<int32_t> indices;
    std::vector<double> data;
};

// the entries in the order they come within a row: columns need not ascend, repeats stay
Graph from_edges(int n, const std::vector<Edge> &edges)
{
    std::vector<std::vector<Edge>> rows((size_t)n);
    for (const Edge &e : edges) rows[(size_t)e.from].push_back(e);
    Graph g;
    g.n = n;
    g.indptr.push_back(0);
    for (int i = 0; i < n; ++i) {
        for (const Edge &e : rows[(size_t)i]) {
            g.indices.push_back(e.to);
            g.data.push_back(e.length);
        }
        g.indptr.push_back((int64_t)g.indices.size());
    }
    return g;
}

struct Sets {
    std::vector<int64_t> ptr{0};
    std::vector<int32_t> roots;
    void add(std::initializer_list<int> members)
    {
        for (int m : members) roots.push_back(m);
        ptr.push_back((int64_t)roots.size());
    }
    int count() const { return (int)ptr.size() - 1; }
};

int geodesic(const Graph &g, bool values, int directed, const Sets &s, std::vector<double> &dist, int64_t stats[3])
{
    dist.assign((size_t)s.count() * (size_t)g.n, -7.0);
    std::fill(stats, stats + 3, (int64_t)-7);
    return schpf_debug_geodesic(g.n, g.indptr.data(), g.indices.data(), values ? g.data.data() : nullptr, directed, s.count(),
                                s.ptr.data(), s.roots.data(), dist.data(), stats);
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
    std::vector<double> dist;
    int64_t stats[3];

    // a path of 4 097 vertices, numbered by a multiplicative walk (a permutation: 4 097 = 17 * 241, 5 is coprime to it),
    // stored in one direction only; step s has length s % 4, so every fourth is a stored zero.  Sums of small integers: exact
    const int n = 4097;
    std::vector<Edge> edges;
    std::vector<int> name((size_t)n);
    for (int s = 0; s < n; ++s) name[(size_t)s] = (int)((int64_t)s * 5 % n);
    for (int s = 0; s + 1 < n; ++s) edges.push_back(Edge{name[(size_t)s], name[(size_t)s + 1], (double)(s % 4)});
    const Graph path = from_edges(n, edges);
    Sets ends;
    ends.add({name[0]});
    ends.add({name[(size_t)n - 1]});
    ends.add({});
    ends.add({name[0], name[(size_t)n - 1], name[0]});
    int ok = geodesic(path, true, 0, ends, dist, stats) == 0 && stats[0] == 3 * n && stats[1] == 0 && stats[2] == 0;
    std::vector<double> along((size_t)n, 0.0);
    for (int s = 1; s < n; ++s) along[(size_t)s] = along[(size_t)s - 1] + (double)((s - 1) % 4);
    for (int s = 0; ok && s < n; ++s) {
        const double back = along[(size_t)n - 1] - along[(size_t)s];
        ok = dist[(size_t)name[(size_t)s]] == along[(size_t)s] && dist[(size_t)n + (size_t)name[(size_t)s]] == back &&
             dist[2 * (size_t)n + (size_t)name[(size_t)s]] == INF &&
             dist[3 * (size_t)n + (size_t)name[(size_t)s]] == std::min(along[(size_t)s], back);
    }
    failures += expect("shuffled path, undirected", ok);
    // directed: nothing leads back to the start, and without values every step is 1
    ok = geodesic(path, false, 1, ends, dist, stats) == 0 && stats[0] == n + 1 + n;
    for (int s = 0; ok && s < n; ++s)
        ok = dist[(size_t)name[(size_t)s]] == (double)s && dist[(size_t)n + (size_t)name[(size_t)s]] == (s == n - 1 ? 0.0 : INF);
    failures += expect("shuffled path, directed hop counts", ok);

    // a 12 x 12 grid with unit edges stored in both directions: Manhattan distances from two corners and from both
    const int side = 12;
    edges.clear();
    for (int y = 0; y < side; ++y)
        for (int x = 0; x < side; ++x) {
            const int v = y * side + x;
            if (x + 1 < side) { edges.push_back(Edge{v, v + 1, 1.0}); edges.push_back(Edge{v + 1, v, 1.0}); }
            if (y + 1 < side) { edges.push_back(Edge{v, v + side, 1.0}); edges.push_back(Edge{v + side, v, 1.0}); }
            edges.push_back(Edge{v, v, 0.25});   // a diagonal entry: ignored
        }
    const Graph grid = from_edges(side * side, edges);
    Sets corners;
    corners.add({0});
    corners.add({side * side - 1, 0});
    ok = geodesic(grid, true, 1, corners, dist, stats) == 0 && stats[0] == 2 * side * side;
    for (int v = 0; ok && v < side * side; ++v) {
        const int x = v % side, y = v / side;
        ok = dist[(size_t)v] == x + y && dist[(size_t)(side * side + v)] == std::min(x + y, 2 * (side - 1) - x - y);
    }
    failures += expect("grid", ok);

    // entries stored twice with different lengths, both directions with different lengths, a zero, a tiny and a huge length,
    // a directed cycle 5 -> 6 -> 7 -> 5 that nothing enters, vertex 8 alone, and vertex 9 behind a second huge length
    edges = {{0, 1, 4.0}, {0, 1, 1.5}, {0, 1, 9.0}, {1, 0, 0.5}, {1, 2, 0.0}, {2, 3, 1e-300}, {3, 4, 1.2e308}, {0, 4, 1.7e308},
             {5, 6, 1.0}, {6, 7, 1.0}, {7, 5, 1.0}, {4, 2, 1.2e308}, {3, 9, 1.2e308}};
    const Graph odd = from_edges(10, edges);
    Sets zero;
    zero.add({0});
    zero.add({4});
    zero.add({8, 6});
    ok = geodesic(odd, true, 1, zero, dist, stats) == 0;
    // from 4, vertex 9 lies behind 4 -> 2 and 3 -> 9: the sum overflows to +inf, the same as unreachable
    const double want_directed[30] = {0, 1.5, 1.5, 1.5 + 1e-300, 1.5 + 1e-300 + 1.2e308, INF, INF, INF, INF, 1.5 + 1e-300 + 1.2e308,
                                      INF, INF, 1.2e308, 1.2e308 + 1e-300, 0, INF, INF, INF, INF, INF,
                                      INF, INF, INF, INF, INF, 2, 0, 1, 0, INF};
    failures += expect("odd graph, directed", ok && std::equal(dist.begin(), dist.end(), want_directed) && stats[0] == 6 + 3 + 4);
    ok = geodesic(odd, true, 0, zero, dist, stats) == 0;
    // undirected: {0, 1} is 0.5 by its smaller direction alone; 4 is reached over 3 and not over the longer 0 - 4; from 4
    // everything but 9 is one huge length away
    const double want_undirected[30] = {0, 0.5, 0.5, 0.5 + 1e-300, 0.5 + 1e-300 + 1.2e308, INF, INF, INF, INF, 0.5 + 1e-300 + 1.2e308,
                                        1.2e308 + 0.5, 1.2e308, 1.2e308, 1.2e308, 0, INF, INF, INF, INF, INF,
                                        INF, INF, INF, INF, INF, 1, 0, 1, 0, INF};
    failures += expect("odd graph, undirected", ok && std::equal(dist.begin(), dist.end(), want_undirected) && stats[0] == 6 + 5 + 4);

    // no entries, n = 0, nsets = 0
    Graph none;
    none.n = 37;
    none.indptr.assign(38, 0);
    Sets some;
    some.add({3});
    some.add({5, 5, 36});
    ok = geodesic(none, true, 0, some, dist, stats) == 0 && stats[0] == 3 && dist[3] == 0 && dist[4] == INF && dist[37 + 36] == 0;
    failures += expect("no entries", ok);
    failures += expect("n = 0", schpf_debug_geodesic(0, nullptr, nullptr, nullptr, 0, 4, nullptr, nullptr, nullptr, stats) == 0 &&
                                    stats[0] == 0);
    stats[0] = -7;
    failures += expect("nsets = 0", schpf_debug_geodesic(10, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, stats) == 0 &&
                                        stats[0] == 0);

    // refused: outputs untouched
    Graph bad = odd;
    bad.indices[3] = 10;
    failures += expect("column refused", geodesic(bad, true, 0, zero, dist, stats) != 0 && dist[0] == -7 && stats[0] == -7);
    bad = odd;
    bad.data[2] = -1.0;
    failures += expect("length refused", geodesic(bad, true, 0, zero, dist, stats) != 0 && dist[0] == -7 && stats[0] == -7);
    Sets wrong = zero;
    wrong.roots[2] = 10;
    failures += expect("root refused", geodesic(odd, true, 0, wrong, dist, stats) != 0 && dist[0] == -7 && stats[0] == -7);
    wrong = zero;
    wrong.ptr[2] = 0;
    failures += expect("set_ptr refused", geodesic(odd, true, 0, wrong, dist, stats) != 0 && dist[0] == -7 && stats[0] == -7);

    std::printf(failures ? "geodesic_sanitize FAILED (%d)\n" : "geodesic_sanitize ok\n", failures);
    return failures ? 1 : 0;
}
