// Sanitizer check of schpf_debug_axis_stats and schpf_debug_submatrix, the host restatements of the cell and gene filtering
// (DESIGN.md 21): a stand-alone program, CPU only -- no GPU is opened.  It builds a matrix of the kind the kernel tests use
// (140 rows of 0, 1, 63, 64, 65 and 300 and of 2 .. 120 entries over 3 301 columns, one column in every row, stored zeros,
// a value of 2^24), checks the statistics against sums kept while the matrix was made, takes submatrices out of it (a
// list with repeats under a mask, every row without one, no gene kept, the sizing call alone) and checks that refused
// calls leave their outputs.  Build and run from the repository root (host code only, AddressSanitizer and UBSan on the
// host side):
//
//   hipcc -std=c++17 -O1 -g --offload-host-only -x hip -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tools/qc_sanitize.cpp schpf_amd/csrc/host.cpp schpf_amd/csrc/plan.cpp schpf_amd/csrc/policy.cpp \
//       -o qc_sanitize && ./qc_sanitize
//
// Exit status 0 and "qc_sanitize ok" when the results are right and the sanitizers saw nothing.
#include <cstdint>
#include <cstdio>
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

struct Stats {
    std::vector<int64_t> cell_n, cell_total, cell_set, gene_n, gene_total, gene_sumsq;
    void fill(size_t N, size_t J, size_t S)
    {
        cell_n.assign(N, -7);
        cell_total.assign(N, -7);
        cell_set.assign(N * S, -7);
        gene_n.assign(J, -7);
        gene_total.assign(J, -7);
        gene_sumsq.assign(J, -7);
    }
};

}  // namespace

int main()
{
    int failures = 0;
    uint32_t state = 2024u;
    const int64_t N = 140, J = 3301, EVERY = 7;
    const int S = 32;
    std::vector<int64_t> indptr{0};
    std::vector<int32_t> indices, val;
    std::vector<uint32_t> flags((size_t)J);
    for (auto &f : flags) f = next(state) * 2654435761u;
    Stats want;
    want.fill((size_t)N, (size_t)J, (size_t)S);
    for (auto *v : {&want.cell_n, &want.cell_total, &want.cell_set, &want.gene_n, &want.gene_total, &want.gene_sumsq})
        std::fill(v->begin(), v->end(), (int64_t)0);
    const int lengths[6] = {0, 1, 63, 64, 65, 300};
    for (int64_t r = 0; r < N; ++r) {
        const int len = r < 6 ? lengths[r] : 2 + (int)(next(state) % 119);
        std::set<int32_t> cols;
        if (len > 0) cols.insert((int32_t)EVERY);
        if (r == 5) cols.insert({0, 3071, 3072, (int32_t)J - 1});
        while ((int)cols.size() < len) {
            const int32_t c = (int32_t)(next(state) % J);
            if (c != 11) cols.insert(c);   // column 11 stays empty
        }
        for (int32_t c : cols) {
            int64_t v = 1 + next(state) % 40;
            if (next(state) % 23 == 0 && c != EVERY) v = 0;
            if (r == 20 && c == EVERY) v = (int64_t)1 << 24;
            indices.push_back(c);
            val.push_back((int32_t)v);
            if (v == 0) continue;
            ++want.cell_n[(size_t)r];
            want.cell_total[(size_t)r] += v;
            for (int s = 0; s < S; ++s)
                if ((flags[(size_t)c] >> s) & 1u) want.cell_set[(size_t)(s * N + r)] += v;
            ++want.gene_n[(size_t)c];
            want.gene_total[(size_t)c] += v;
            want.gene_sumsq[(size_t)c] += v * v;
        }
        indptr.push_back((int64_t)indices.size());
    }
    const int64_t nnz = (int64_t)indices.size();

    Stats got;
    const auto stats = [&](const std::vector<int32_t> &values, int n_sets) {
        got.fill((size_t)N, (size_t)J, (size_t)n_sets);
        return schpf_debug_axis_stats(N, J, nnz, indptr.data(), indices.data(), values.data(), SCHPF_VAL_I32, n_sets, flags.data(),
                                      got.cell_n.data(), got.cell_total.data(), got.cell_set.data(), got.gene_n.data(),
                                      got.gene_total.data(), got.gene_sumsq.data());
    };
    if (stats(val, S) != 0) {
        std::printf("statistics: %s\n", schpf_last_error());
        ++failures;
    } else {
        failures += got.cell_n != want.cell_n || got.cell_total != want.cell_total || got.cell_set != want.cell_set;
        failures += got.gene_n != want.gene_n || got.gene_total != want.gene_total || got.gene_sumsq != want.gene_sumsq;
        failures += got.gene_n[11] != 0 || got.gene_n[(size_t)EVERY] != N - 1;
        std::printf("statistics: %lld entries, largest sum of squares %lld\n", (long long)nnz, (long long)got.gene_sumsq[(size_t)EVERY]);
    }
    failures += stats(val, 0) != 0 || got.gene_n != want.gene_n;
    // a refused call leaves its outputs
    std::vector<int32_t> bad = val;
    bad[(size_t)nnz - 1] = -1;
    failures += stats(bad, 2) == 0 || got.cell_n[0] != -7 || got.gene_sumsq[(size_t)J - 1] != -7 || got.cell_set[0] != -7;

    // submatrices: a list with repeats under a mask, every row without one, no gene kept
    std::vector<int32_t> rows{5, 5, 0, 139, 2, 20, 5};
    for (int i = 0; i < 60; ++i) rows.push_back((int32_t)(next(state) % N));
    std::vector<uint8_t> keep((size_t)J);
    for (int64_t j = 0; j < J; ++j) keep[(size_t)j] = (uint8_t)(j % 2 == 0);
    const auto sub = [&](const std::vector<int32_t> *list, const std::vector<uint8_t> *mask, int64_t short_by, const char *what) {
        const int64_t n_rows = list ? (int64_t)list->size() : N;
        int64_t kept = -7;
        std::vector<int64_t> ptr((size_t)n_rows + 1, -7);
        if (schpf_debug_submatrix(N, J, nnz, indptr.data(), indices.data(), val.data(), SCHPF_VAL_I32, n_rows, list ? list->data() : nullptr,
                                  mask ? mask->data() : nullptr, &kept, ptr.data(), nullptr, nullptr, 0) != 0) {
            std::printf("%s, sizing call: %s\n", what, schpf_last_error());
            return 1;
        }
        const int64_t total = ptr[(size_t)n_rows];
        std::vector<int32_t> out_indices((size_t)total), out_values((size_t)total);   // exactly the total: one past it is caught
        std::vector<int64_t> again((size_t)n_rows + 1, -7);
        const int status = schpf_debug_submatrix(N, J, nnz, indptr.data(), indices.data(), val.data(), SCHPF_VAL_I32, n_rows,
                                                 list ? list->data() : nullptr, mask ? mask->data() : nullptr, &kept, again.data(),
                                                 out_indices.data(), out_values.data(), total - short_by);
        if (short_by) return (int)(status == 0 || again[0] != -7);
        if (status != 0) {
            std::printf("%s, filling call: %s\n", what, schpf_last_error());
            return 1;
        }
        int wrong = again != ptr;
        int64_t o = 0;
        for (int64_t s = 0; s < n_rows; ++s) {
            const int64_t r = list ? (*list)[(size_t)s] : s;
            for (int64_t e = indptr[(size_t)r]; e < indptr[(size_t)r + 1]; ++e) {
                const int32_t c = indices[(size_t)e];
                if (mask && !(*mask)[(size_t)c]) continue;
                wrong += out_indices[(size_t)o] != (mask ? c / 2 : c) || out_values[(size_t)o] != val[(size_t)e];
                ++o;
            }
            wrong += ptr[(size_t)s + 1] != o;
        }
        std::printf("%s: %lld rows, %lld genes, %lld entries\n", what, (long long)n_rows, (long long)kept, (long long)total);
        return wrong;
    };
    failures += sub(&rows, &keep, 0, "repeats under a mask");
    failures += sub(nullptr, nullptr, 0, "every row, every gene");
    failures += sub(&rows, &keep, 1, "a capacity one short");
    std::vector<uint8_t> none((size_t)J, 0);
    failures += sub(nullptr, &none, 0, "no gene kept");
    std::vector<int32_t> outside{3, (int32_t)N};
    int64_t kept = -7;
    std::vector<int64_t> ptr(3, -7);
    failures += schpf_debug_submatrix(N, J, nnz, indptr.data(), indices.data(), val.data(), SCHPF_VAL_I32, 2, outside.data(), nullptr, &kept,
                                      ptr.data(), nullptr, nullptr, 0) == 0 || kept != -7 || ptr[0] != -7;

    std::printf(failures ? "qc_sanitize FAILED (%d)\n" : "qc_sanitize ok\n", failures);
    return failures ? 1 : 0;
}
