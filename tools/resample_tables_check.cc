// resample_tables_check.cc -- h264r::resample_axis (arrow-h264_amd/csrc/resample_tables.h) on its own,
// for a build with -fsanitize=address,undefined: tests/test_output_resample.py compiles and runs it.
//
// Reads cases "filter in_size in0 in1 out_size" from standard input.  For each it asks for ksize alone,
// allocates xmin, count and kk on the heap at exactly the sizes the header states (out_size, out_size,
// out_size * ksize: one byte past any of them is the sanitizer's), fills them with a pattern, builds the
// table, and checks what the header promises: every entry written, xmin >= 0, 1 <= count <= ksize,
// xmin + count <= in_size, zeros from count on, xmin and xmin + count not decreasing, and the accumulator
// bound 255 * sum |kk| + 2^21 < 2^31 with every tap inside 24 bits.  Prints one line per case,
// "ksize checksum", for the caller to compare with its own tables, and exits non-zero on any violation.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "resample_tables.h"

static int fail(const char* what, int f, int s, int a, int b, int d)
{
    fprintf(stderr, "resample_tables_check: %s (filter %d in_size %d in0 %d in1 %d out_size %d)\n", what, f, s, a, b, d);
    return 1;
}

int main()
{
    int f, s, a, b, d, cases = 0;
    const int32_t pattern = (int32_t)0xA5A5A5A5;
    while (scanf("%d %d %d %d %d", &f, &s, &a, &b, &d) == 5) {
        int32_t ks = -1;
        if (h264r::resample_axis(f, s, a, b, d, nullptr, nullptr, nullptr, &ks) != H264R_OK || ks < 3 || !(ks & 1)) return fail("ksize", f, s, a, b, d);
        std::unique_ptr<int32_t[]> xmin(new int32_t[d]), count(new int32_t[d]), kk(new int32_t[(size_t)d * ks]);
        for (int i = 0; i < d; ++i) xmin[i] = count[i] = pattern;
        for (size_t i = 0; i < (size_t)d * ks; ++i) kk[i] = pattern;
        int32_t ks2 = -1;
        if (h264r::resample_axis(f, s, a, b, d, xmin.get(), count.get(), kk.get(), &ks2) != H264R_OK || ks2 != ks) return fail("status", f, s, a, b, d);
        uint64_t sum = 1469598103934665603ull;
        auto mix = [&sum](int64_t v) { sum = (sum ^ (uint64_t)v) * 1099511628211ull; };
        for (int i = 0; i < d; ++i) {
            if (xmin[i] < 0 || count[i] < 1 || count[i] > ks || xmin[i] + count[i] > s) return fail("window", f, s, a, b, d);
            if (i && (xmin[i] < xmin[i - 1] || xmin[i] + count[i] < xmin[i - 1] + count[i - 1])) return fail("order", f, s, a, b, d);
            int64_t mag = 0;
            for (int j = 0; j < ks; ++j) {
                const int32_t k = kk[(size_t)i * ks + j];
                if (k == pattern) return fail("unwritten tap", f, s, a, b, d);
                if (j >= count[i] && k != 0) return fail("tap behind count", f, s, a, b, d);
                if (k >= (1 << 23) || k < -(1 << 23)) return fail("tap beyond 24 bits", f, s, a, b, d);
                mag += k < 0 ? -(int64_t)k : k;
                mix(k);
            }
            if (255 * mag + (1 << 21) >= (int64_t)1 << 31) return fail("accumulator", f, s, a, b, d);
            mix(xmin[i]);
            mix(count[i]);
        }
        printf("%d %llu\n", ks, (unsigned long long)sum);
        ++cases;
    }
    // the refusals write nothing
    int32_t ks = 77, one = pattern;
    if (h264r::resample_axis(3, 4, 0, 4, 2, nullptr, nullptr, nullptr, &ks) != H264R_EINVAL ||
        h264r::resample_axis(0, 4, 2, 2, 2, nullptr, nullptr, nullptr, &ks) != H264R_EINVAL ||
        h264r::resample_axis(0, 4, 0, 5, 2, nullptr, nullptr, nullptr, &ks) != H264R_EINVAL ||
        h264r::resample_axis(0, 4, -1, 4, 2, nullptr, nullptr, nullptr, &ks) != H264R_EINVAL ||
        h264r::resample_axis(0, 4, 0, 4, 0, nullptr, nullptr, nullptr, &ks) != H264R_EINVAL ||
        h264r::resample_axis(0, 4, 0, 4, 16385, nullptr, nullptr, nullptr, &ks) != H264R_EINVAL ||
        h264r::resample_axis(0, 4, 0, 4, 2, nullptr, nullptr, nullptr, nullptr) != H264R_EINVAL ||
        h264r::resample_axis(0, 4, 0, 4, 1, &one, nullptr, nullptr, &ks) != H264R_EINVAL || ks != 77 || one != pattern)
        return fail("refusals", 0, 0, 0, 0, 0);
    return cases ? 0 : fail("no cases", 0, 0, 0, 0, 0);
}
