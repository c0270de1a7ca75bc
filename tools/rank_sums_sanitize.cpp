// Sanitizer check of schpf_debug_rank_sums, the host restatement of the rank sums: a stand-alone program, CPU
// only -- no GPU is opened.  It ranks a gene that every one of 70 001 cells expresses (at one value, then at a few) and
// 3 000 genes of 0 to 3 entries each, and checks what comes back against what the ranks 1 .. N must add up to.  Build and
// run from the repository root (host code only, AddressSanitizer and UBSan on the host side):
//
//   hipcc -std=c++17 -O1 -g --offload-host-only -x hip -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tools/rank_sums_sanitize.cpp schpf_amd/csrc/host.cpp schpf_amd/csrc/plan.cpp schpf_amd/csrc/policy.cpp \
//       -o rank_sums_sanitize && ./rank_sums_sanitize
//
// Exit status 0 and "rank_sums_sanitize ok" when the sums are right and the sanitizers saw nothing.
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

struct Matrix {
    int ncells = 0, ngenes = 0;
    std::vector<int64_t> indptr{0};
    std::vector<int32_t> indices;
    std::vector<float> data;
    void close_gene()
    {
        indptr.push_back((int64_t)indices.size());
        ++ngenes;
    }
};

struct Sums {
    std::vector<int64_t> n, zeros, ties, nexpr, rank2;
};

int run(const Matrix &m, const std::vector<int32_t> &labels, int G, Sums &s)
{
    s.n.assign((size_t)G, -7);
    s.zeros.assign((size_t)m.ngenes, -7);
    s.ties.assign((size_t)m.ngenes, -7);
    s.nexpr.assign((size_t)G * m.ngenes, -7);
    s.rank2.assign((size_t)G * m.ngenes, -7);
    return schpf_debug_rank_sums(m.ncells, m.ngenes, m.indptr.data(), m.indices.data(), m.data.data(), labels.data(), G, s.n.data(),
                                 s.zeros.data(), s.ties.data(), s.nexpr.data(), s.rank2.data());
}

uint32_t next(uint32_t &state)   // a small generator: the same matrix everywhere
{
    state = state * 1664525u + 1013904223u;
    return state >> 8;
}

// every cell is in a group: the groups' rank sums of a gene add up to 2 (1 + .. + N), their cells to N
int check_totals(const Matrix &m, int G, const Sums &s)
{
    int failures = 0;
    const int64_t N = m.ncells, J = m.ngenes;
    int64_t cells = 0;
    for (int g = 0; g < G; ++g) cells += s.n[(size_t)g];
    failures += cells != N;
    for (int64_t j = 0; j < J; ++j) {
        int64_t ranks = 0, expressed = 0;
        for (int g = 0; g < G; ++g) {
            ranks += s.rank2[(size_t)(g * J + j)];
            expressed += s.nexpr[(size_t)(g * J + j)];
        }
        failures += ranks != N * (N + 1);
        failures += expressed != N - s.zeros[(size_t)j];
    }
    return failures;
}

}  // namespace

int main()
{
    int failures = 0;
    Sums s;
    uint32_t state = 12345u;

    // the dense genes: one value everywhere; the values 1 .. 4; every value different
    const int N = 70001, G = 20;
    Matrix dense;
    dense.ncells = N;
    for (int kind = 0; kind < 3; ++kind) {
        for (int i = 0; i < N; ++i) {
            dense.indices.push_back(i);
            dense.data.push_back(kind == 0 ? 3.0f : kind == 1 ? (float)(1 + next(state) % 4) : (float)(i + 1) * 0.5f);
        }
        dense.close_gene();
    }
    std::vector<int32_t> labels((size_t)N);
    for (int i = 0; i < N; ++i) labels[(size_t)i] = (int32_t)(next(state) % G);
    if (run(dense, labels, G, s) != 0) {
        std::printf("dense genes: %s\n", schpf_last_error());
        ++failures;
    } else {
        const int64_t n64 = N;
        failures += check_totals(dense, G, s);
        failures += s.zeros[0] != 0 || s.ties[0] != n64 * n64 * n64 - n64 || s.ties[2] != 0;
        for (int g = 0; g < G; ++g) failures += s.rank2[(size_t)g * 3] != s.n[(size_t)g] * (n64 + 1);   // all tie: the mean rank
        std::printf("dense genes: ties %lld, %lld, %lld\n", (long long)s.ties[0], (long long)s.ties[1], (long long)s.ties[2]);
    }

    // many short genes, stored zeros among their entries
    Matrix shorts;
    shorts.ncells = 500;
    for (int j = 0; j < 3000; ++j) {
        const int len = (int)(next(state) % 4);
        int cell = (int)(next(state) % 100);
        for (int e = 0; e < len; ++e) {
            shorts.indices.push_back(cell);
            shorts.data.push_back((float)(next(state) % 3));
            cell += 1 + (int)(next(state) % 100);
        }
        shorts.close_gene();
    }
    labels.assign(500, 0);
    for (int i = 0; i < 500; ++i) labels[(size_t)i] = (int32_t)(next(state) % 7);
    if (run(shorts, labels, 7, s) != 0) {
        std::printf("short genes: %s\n", schpf_last_error());
        ++failures;
    } else {
        failures += check_totals(shorts, 7, s);
        std::printf("short genes: %d genes, %lld entries\n", shorts.ngenes, (long long)shorts.indices.size());
    }

    // a refused call leaves its outputs
    Matrix bad = shorts;
    for (size_t e = 0; e < bad.data.size(); ++e)
        if (e % 50 == 7) bad.data[e] = -1.0f;
    failures += run(bad, labels, 7, s) == 0 || s.n[0] != -7 || s.rank2[0] != -7 || s.ties[0] != -7;
    labels[3] = 7;
    failures += run(shorts, labels, 7, s) == 0 || s.n[0] != -7 || s.zeros[0] != -7;

    std::printf(failures ? "rank_sums_sanitize FAILED (%d)\n" : "rank_sums_sanitize ok\n", failures);
    return failures ? 1 : 0;
}
