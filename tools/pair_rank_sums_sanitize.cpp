// Sanitizer check of schpf_debug_pair_rank_sums, the host restatement of the rank sums between pairs of groups (DESIGN.md
// 25): a stand-alone program, CPU only -- no GPU is opened.  It ranks three genes that every one of 70 001 cells expresses
// and 3 000 genes of 0 to 3 entries each, for all pairs of the groups, a repeated and a reversed pair, with cells in no
// group, and checks what comes back against the identities of the definition and, for two groups that hold every cell,
// against schpf_debug_rank_sums.  Build and run from the repository root (host code only, AddressSanitizer and UBSan on
// the host side):
//
//   hipcc -std=c++17 -O1 -g --offload-host-only -x hip -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tools/pair_rank_sums_sanitize.cpp schpf_amd/csrc/host.cpp schpf_amd/csrc/plan.cpp schpf_amd/csrc/policy.cpp \
//       -o pair_rank_sums_sanitize && ./pair_rank_sums_sanitize
//
// Exit status 0 and "pair_rank_sums_sanitize ok" when the sums are right and the sanitizers saw nothing.
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
    std::vector<int64_t> n, nexpr, u2, ties;
};

int run(const Matrix &m, const std::vector<int32_t> &labels, int G, const std::vector<int32_t> &pairs, Sums &s)
{
    const size_t P = pairs.size() / 2;
    s.n.assign((size_t)G, -7);
    s.nexpr.assign((size_t)G * m.ngenes, -7);
    s.u2.assign(P * m.ngenes + 1, -7);   // one more: a list without pairs still has an address
    s.ties.assign(P * m.ngenes + 1, -7);
    return schpf_debug_pair_rank_sums(m.ncells, m.ngenes, m.indptr.data(), m.indices.data(), m.data.data(), labels.data(), G,
                                      pairs.data(), (int)P, s.n.data(), s.nexpr.data(), s.u2.data(), s.ties.data());
}

uint32_t next(uint32_t &state)   // a small generator: the same matrix everywhere
{
    state = state * 1664525u + 1013904223u;
    return state >> 8;
}

// all a < b, then pair 0 again, then pair 0 reversed
std::vector<int32_t> pairs_of(int G)
{
    std::vector<int32_t> pairs;
    for (int a = 0; a < G; ++a)
        for (int b = a + 1; b < G; ++b) {
            pairs.push_back(a);
            pairs.push_back(b);
        }
    pairs.insert(pairs.end(), {0, 1, 1, 0});
    return pairs;
}

// the repeat equals its pair; the reversed pair has 2 n_a n_b - u2 and the same ties; 0 <= u2 <= 2 n_a n_b
int check_identities(const Matrix &m, const std::vector<int32_t> &pairs, const Sums &s)
{
    int failures = 0;
    const int64_t J = m.ngenes, P = (int64_t)pairs.size() / 2;
    for (int64_t j = 0; j < J; ++j) {
        const int64_t both = 2 * s.n[0] * s.n[1];
        failures += s.u2[(size_t)((P - 2) * J + j)] != s.u2[(size_t)j] || s.ties[(size_t)((P - 2) * J + j)] != s.ties[(size_t)j];
        failures += s.u2[(size_t)((P - 1) * J + j)] != both - s.u2[(size_t)j] || s.ties[(size_t)((P - 1) * J + j)] != s.ties[(size_t)j];
        for (int64_t p = 0; p < P; ++p) {
            const int64_t most = 2 * s.n[(size_t)pairs[(size_t)(2 * p)]] * s.n[(size_t)pairs[(size_t)(2 * p + 1)]];
            failures += s.u2[(size_t)(p * J + j)] < 0 || s.u2[(size_t)(p * J + j)] > most || s.ties[(size_t)(p * J + j)] < 0;
        }
    }
    return failures;
}

// two groups that hold every cell: the pair is the whole matrix, u2 = rank2[0] - n_0 (n_0 + 1) and the ties are the ties
int check_against_rank_sums(const Matrix &m, uint32_t &state)
{
    std::vector<int32_t> labels((size_t)m.ncells);
    for (auto &l : labels) l = (int32_t)(next(state) % 2);
    Sums s;
    if (run(m, labels, 2, {0, 1}, s) != 0) return 1;
    const size_t J = (size_t)m.ngenes;
    std::vector<int64_t> n(2), zeros(J), ties(J), nexpr(2 * J), rank2(2 * J);
    if (schpf_debug_rank_sums(m.ncells, m.ngenes, m.indptr.data(), m.indices.data(), m.data.data(), labels.data(), 2, n.data(),
                              zeros.data(), ties.data(), nexpr.data(), rank2.data()) != 0)
        return 1;
    int failures = n[0] != s.n[0] || n[1] != s.n[1];
    for (size_t j = 0; j < J; ++j)
        failures += s.u2[j] != rank2[j] - n[0] * (n[0] + 1) || s.ties[j] != ties[j] || s.nexpr[j] != nexpr[j] || s.nexpr[J + j] != nexpr[J + j];
    return failures;
}

}  // namespace

int main()
{
    int failures = 0;
    Sums s;
    uint32_t state = 12345u;

    // the dense genes: one value everywhere; the values 1 .. 4; every value different.  One cell in twenty is in no group
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
    for (int i = 0; i < N; ++i) labels[(size_t)i] = next(state) % 20 == 0 ? -1 : (int32_t)(next(state) % G);
    std::vector<int32_t> pairs = pairs_of(G);
    if (run(dense, labels, G, pairs, s) != 0) {
        std::printf("dense genes: %s\n", schpf_last_error());
        ++failures;
    } else {
        failures += check_identities(dense, pairs, s);
        const int64_t both = s.n[0] + s.n[1];
        failures += s.u2[0] != s.n[0] * s.n[1] || s.ties[0] != both * both * both - both || s.ties[2] != 0;   // all tie; none do
        std::printf("dense genes: %d pairs, u2 %lld, %lld, %lld\n", (int)(pairs.size() / 2), (long long)s.u2[0], (long long)s.u2[1],
                    (long long)s.u2[2]);
    }
    failures += check_against_rank_sums(dense, state);

    // many short genes, stored zeros among their entries; group 6 is empty
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
    for (int i = 0; i < 500; ++i) labels[(size_t)i] = (int32_t)(next(state) % 7) - 1;
    pairs = pairs_of(7);
    if (run(shorts, labels, 7, pairs, s) != 0) {
        std::printf("short genes: %s\n", schpf_last_error());
        ++failures;
    } else {
        failures += check_identities(shorts, pairs, s);
        failures += s.n[6] != 0;
        for (int j = 0; j < shorts.ngenes; ++j) failures += s.u2[(size_t)(5 * shorts.ngenes + j)] != 0;   // the pair (0, 6)
        std::printf("short genes: %d genes, %lld entries\n", shorts.ngenes, (long long)shorts.indices.size());
    }
    failures += check_against_rank_sums(shorts, state);
    failures += run(shorts, labels, 7, {}, s) != 0 || s.n[0] < 0 || s.nexpr[0] < 0 || s.u2[0] != -7;   // no pairs: n and nexpr

    // a refused call leaves its outputs
    Matrix bad = shorts;
    for (size_t e = 0; e < bad.data.size(); ++e)
        if (e % 50 == 7) bad.data[e] = -1.0f;
    failures += run(bad, labels, 7, pairs, s) == 0 || s.n[0] != -7 || s.u2[0] != -7 || s.ties[0] != -7;
    pairs[5] = pairs[4];
    failures += run(shorts, labels, 7, pairs, s) == 0 || s.n[0] != -7 || s.nexpr[0] != -7 || s.u2[0] != -7;
    failures += std::string(schpf_last_error()) != "pairs must name two different groups in [0, ngroups); offending pair 2";

    std::printf(failures ? "pair_rank_sums_sanitize FAILED (%d)\n" : "pair_rank_sums_sanitize ok\n", failures);
    return failures ? 1 : 0;
}
