// Sanitizer check of schpf_debug_group_stats, the host restatement of the pseudobulk sums: a stand-alone
// program, CPU only -- no GPU is opened.  It builds a matrix of the kind the kernel tests use (140 rows of 0, 1, 63, 64, 65
// and 300 and of 2 .. 120 entries over 3 301 columns, one column in every row, stored zeros, a value of 2^24), labels with
// cells in no group, an empty group in the middle and an empty last group, checks the statistics against sums kept while
// the matrix was made, with and without the sum of squares, with every cell its own group and with no entries, and checks
// that refused calls leave their outputs.  Build and run from the repository root (host code only, AddressSanitizer and
// UBSan on the host side):
//
//   hipcc -std=c++17 -O1 -g --offload-host-only -x hip -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tools/group_stats_sanitize.cpp schpf_amd/csrc/host.cpp schpf_amd/csrc/plan.cpp schpf_amd/csrc/policy.cpp \
//       -o group_stats_sanitize && ./group_stats_sanitize
//
// Exit status 0 and "group_stats_sanitize ok" when the results are right and the sanitizers saw nothing.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../include/schpf_hip.h"

namespace schpf {
thread_local std::string g_err;   // the library keeps it in capi.hip, which is not part of this program
}
extern "C" const char *schpf_last_error(void) { return schpf::g_err.c_str(); }

namespace {

uint32_t next(uint32_t &state)   // a small generator: the same matrix everywhere
{
    state = state * 1664525u + 1013904223u;
    return state >> 8;
}

struct Tables {   // exactly G and G * J long: one past them is caught
    std::vector<int64_t> n, nexpr, total, sumsq;
    void fill(size_t G, size_t J, int64_t v)
    {
        n.assign(G, v);
        nexpr.assign(G * J, v);
        total.assign(G * J, v);
        sumsq.assign(G * J, v);
    }
    bool all(int64_t v) const
    {
        for (const auto *t : {&n, &nexpr, &total, &sumsq})
            for (int64_t x : *t)
                if (x != v) return false;
        return true;
    }
};

}  // namespace

int main()
{
    int failures = 0;
    uint32_t state = 2025u;
    const int64_t N = 140, J = 3301, EVERY = 7, G = 6;   // groups 2 and 5 stay empty
    std::vector<int64_t> indptr{0};
    std::vector<int32_t> indices, val, labels((size_t)N);
    for (int64_t r = 0; r < N; ++r) {
        const int pick = (int)(next(state) % 5);   // 0 .. 3 -> groups 0, 1, 3, 4; 4 -> no group
        labels[(size_t)r] = pick == 4 ? -1 : pick >= 2 ? pick + 1 : pick;
    }
    labels[5] = 0;   // the long row is in a group
    Tables want;
    want.fill((size_t)G, (size_t)J, 0);
    const int lengths[6] = {0, 1, 63, 64, 65, 300};
    for (int64_t r = 0; r < N; ++r) {
        const int len = r < 6 ? lengths[r] : 2 + (int)(next(state) % 119);
        std::set<int32_t> cols;
        if (len > 0) cols.insert((int32_t)EVERY);
        if (r == 5) cols.insert({0, 2047, 2048, (int32_t)J - 1});
        while ((int)cols.size() < len) {
            const int32_t c = (int32_t)(next(state) % J);
            if (c != 11) cols.insert(c);   // column 11 stays empty
        }
        const int32_t g = labels[(size_t)r];
        if (g >= 0) ++want.n[(size_t)g];
        for (int32_t c : cols) {
            int64_t v = 1 + next(state) % 40;
            if (next(state) % 23 == 0 && c != EVERY) v = 0;
            if (r == 20 && c == EVERY) v = (int64_t)1 << 24;
            indices.push_back(c);
            val.push_back((int32_t)v);
            if (v == 0 || g < 0) continue;
            const size_t at = (size_t)(g * J + c);
            ++want.nexpr[at];
            want.total[at] += v;
            want.sumsq[at] += v * v;
        }
        indptr.push_back((int64_t)indices.size());
    }
    const int64_t nnz = (int64_t)indices.size();

    Tables got;
    const auto stats = [&](const std::vector<int32_t> &values, const std::vector<int32_t> &lab, int64_t groups, bool squares) {
        got.fill((size_t)groups, (size_t)J, -7);
        return schpf_debug_group_stats(N, J, nnz, indptr.data(), indices.data(), values.data(), SCHPF_VAL_I32, lab.data(), groups,
                                       got.n.data(), got.nexpr.data(), got.total.data(), squares ? got.sumsq.data() : nullptr);
    };
    if (stats(val, labels, G, true) != 0) {
        std::printf("statistics: %s\n", schpf_last_error());
        ++failures;
    } else {
        failures += got.n != want.n || got.nexpr != want.nexpr || got.total != want.total || got.sumsq != want.sumsq;
        failures += got.n[2] != 0 || got.n[5] != 0 || got.nexpr[11] != 0;
        int64_t inside = 0;
        for (int64_t n : got.n) inside += n;
        std::printf("statistics: %lld entries, %lld of %lld cells in %lld groups\n", (long long)nnz, (long long)inside, (long long)N, (long long)G);
    }
    // without the squares: they are left alone, the others are the same
    failures += stats(val, labels, G, false) != 0 || got.nexpr != want.nexpr || got.total != want.total || got.sumsq[0] != -7;
    // every cell its own group: the dense matrix
    std::vector<int32_t> own((size_t)N);
    for (int64_t r = 0; r < N; ++r) own[(size_t)r] = (int32_t)r;
    if (stats(val, own, N, true) != 0) {
        std::printf("every cell its own group: %s\n", schpf_last_error());
        ++failures;
    } else {
        int wrong = 0;
        int64_t seen = 0;
        for (int64_t r = 0; r < N; ++r)
            for (int64_t e = indptr[(size_t)r]; e < indptr[(size_t)r + 1]; ++e) {
                const size_t at = (size_t)(r * J + indices[(size_t)e]);
                wrong += got.total[at] != val[(size_t)e] || got.nexpr[at] != (val[(size_t)e] > 0);
                seen += val[(size_t)e];
            }
        int64_t sum = 0;
        for (int64_t t : got.total) sum += t;
        failures += wrong + (sum != seen);
        std::printf("every cell its own group: %lld counts\n", (long long)sum);
    }
    // refused calls leave their outputs: a bad value, a label below -1, a label of ngroups
    std::vector<int32_t> bad = val;
    bad[(size_t)nnz - 1] = -1;
    failures += stats(bad, labels, G, true) == 0 || !got.all(-7);
    for (int32_t wrong_label : {-2, (int32_t)G}) {
        std::vector<int32_t> lab = labels;
        lab[(size_t)N - 1] = wrong_label;
        lab[77] = wrong_label;
        failures += stats(val, lab, G, true) == 0 || !got.all(-7) ||
                    std::strcmp(schpf_last_error(), "group_stats: labels must be in [-1, ngroups); offending cell 77") != 0;
    }
    // no entries: the matrix is not read, the cells are counted
    got.fill((size_t)G, (size_t)J, -7);
    failures += schpf_debug_group_stats(N, J, 0, nullptr, nullptr, nullptr, SCHPF_VAL_I32, labels.data(), G, got.n.data(), got.nexpr.data(),
                                        got.total.data(), got.sumsq.data()) != 0 ||
                got.n != want.n || got.total != std::vector<int64_t>((size_t)(G * J), 0);

    std::printf(failures ? "group_stats_sanitize FAILED (%d)\n" : "group_stats_sanitize ok\n", failures);
    return failures ? 1 : 0;
}
