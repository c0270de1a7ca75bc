// Sanitizer check of schpf_debug_transpose, the host restatement of the transpose to gene-major: a
// stand-alone program, CPU only -- no GPU is opened.  It builds a matrix of the kind the kernel tests use (140 rows of 0, 1,
// 63, 64, 65 and 300 and of 2 .. 120 entries over 6 200 columns, one column in every row, one column empty), transposes it
// with the bytes moved and with the values converted to float32, with and without out_source, into arrays of exactly the
// result's size, checks every entry against the definition, and checks that refused calls leave their outputs.  Build
// and run from the repository root (host code only, AddressSanitizer and UBSan on the host side):
//
//   hipcc -std=c++17 -O1 -g --offload-host-only -x hip -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer \
//       tools/transpose_sanitize.cpp schpf_amd/csrc/host.cpp schpf_amd/csrc/plan.cpp schpf_amd/csrc/policy.cpp \
//       -o transpose_sanitize && ./transpose_sanitize
//
// Exit status 0 and "transpose_sanitize ok" when the results are right and the sanitizers saw nothing.
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

}  // namespace

int main()
{
    int failures = 0;
    uint32_t state = 2027u;
    const int64_t N = 140, J = 6200, EVERY = 7, EMPTY = 11;
    std::vector<int64_t> indptr{0};
    std::vector<int32_t> indices;
    std::vector<double> val;
    const int lengths[6] = {0, 1, 63, 64, 65, 300};
    for (int64_t r = 0; r < N; ++r) {
        const int len = r < 6 ? lengths[r] : 2 + (int)(next(state) % 119);
        std::set<int32_t> cols;
        if (len > 0) cols.insert((int32_t)EVERY);
        if (r == 5) cols.insert({0, 3071, 3072, 6143, 6144, (int32_t)J - 1});
        while ((int)cols.size() < len) {
            const int32_t c = (int32_t)(next(state) % J);
            if (c != EMPTY) cols.insert(c);
        }
        for (int32_t c : cols) {
            indices.push_back(c);
            val.push_back(next(state) % 7 == 0 ? -0.0 : 0.1 * (double)(next(state) % 1000));
        }
        indptr.push_back((int64_t)indices.size());
    }
    const int64_t nnz = (int64_t)indices.size();

    // exactly the result's size: one past it is caught
    std::vector<int64_t> out_indptr((size_t)J + 1), out_source((size_t)nnz);
    std::vector<int32_t> out_cells((size_t)nnz);
    std::vector<double> moved((size_t)nnz);
    std::vector<float> converted((size_t)nnz);
    const auto fill = [&] {
        std::fill(out_indptr.begin(), out_indptr.end(), (int64_t)-7);
        std::fill(out_source.begin(), out_source.end(), (int64_t)-7);
        std::fill(out_cells.begin(), out_cells.end(), -7);
        std::fill(moved.begin(), moved.end(), -7.0);
        std::fill(converted.begin(), converted.end(), -7.0f);
    };
    const auto check = [&](bool as_float, bool with_source, const char *what) {
        fill();
        if (schpf_debug_transpose(N, J, nnz, indptr.data(), indices.data(), val.data(), SCHPF_VAL_F64, as_float ? SCHPF_VAL_F32 : SCHPF_VAL_F64,
                                  out_indptr.data(), out_cells.data(), as_float ? (void *)converted.data() : (void *)moved.data(),
                                  with_source ? out_source.data() : nullptr) != 0) {
            std::printf("%s: %s\n", what, schpf_last_error());
            return 1;
        }
        int wrong = out_indptr[0] != 0 || out_indptr[(size_t)J] != nnz;
        wrong += out_indptr[(size_t)EMPTY + 1] != out_indptr[(size_t)EMPTY] || out_indptr[(size_t)EVERY + 1] - out_indptr[(size_t)EVERY] != N - 1;
        std::vector<int64_t> seen((size_t)J, 0);   // the entries of every column met so far, rows ascending
        for (int64_t r = 0; r < N; ++r)
            for (int64_t e = indptr[(size_t)r]; e < indptr[(size_t)r + 1]; ++e) {
                const size_t c = (size_t)indices[(size_t)e], o = (size_t)(out_indptr[c] + seen[c]++);
                wrong += out_cells[o] != (int32_t)r;
                if (as_float) wrong += converted[o] != (float)val[(size_t)e];
                else wrong += __builtin_memcmp(&moved[o], &val[(size_t)e], sizeof(double)) != 0;   // -0.0 stays -0.0
                wrong += with_source ? out_source[o] != e : out_source[o] != -7;
            }
        for (int64_t j = 0; j < J; ++j) wrong += out_indptr[(size_t)j] + seen[(size_t)j] != out_indptr[(size_t)j + 1];
        std::printf("%s: %lld entries over %lld genes\n", what, (long long)nnz, (long long)J);
        return wrong;
    };
    failures += check(false, true, "bytes moved");
    failures += check(true, true, "values as float32");
    failures += check(false, false, "no out_source");

    // a refused call leaves its outputs
    const auto refused = [&](const std::vector<int64_t> &ptr, const std::vector<int32_t> &idx) {
        fill();
        const int status = schpf_debug_transpose(N, J, nnz, ptr.data(), idx.data(), val.data(), SCHPF_VAL_F64, SCHPF_VAL_F64, out_indptr.data(),
                                                 out_cells.data(), moved.data(), out_source.data());
        return (int)(status == 0 || out_indptr[0] != -7 || out_cells[0] != -7 || moved[(size_t)nnz - 1] != -7.0 || out_source[0] != -7);
    };
    std::vector<int64_t> bad_ptr = indptr;
    bad_ptr[(size_t)N] = nnz + 1;
    failures += refused(bad_ptr, indices);
    std::vector<int32_t> bad_idx = indices;
    bad_idx[(size_t)nnz - 1] = (int32_t)J;
    failures += refused(indptr, bad_idx);
    bad_idx = indices;
    bad_idx[(size_t)indptr[5] + 1] = bad_idx[(size_t)indptr[5]];
    failures += refused(indptr, bad_idx);
    failures += schpf_debug_transpose(0, J, 0, nullptr, nullptr, nullptr, SCHPF_VAL_F64, SCHPF_VAL_F64, out_indptr.data(), nullptr, nullptr, nullptr) != 0 ||
                out_indptr[(size_t)J] != 0;

    std::printf(failures ? "transpose_sanitize FAILED (%d)\n" : "transpose_sanitize ok\n", failures);
    return failures ? 1 : 0;
}
