// Prints where sgpt_encode would cut a packed layout into two chains (sgpt_amd/csrc/encode_split.h): stdin holds one layout per line,
// "T n o_0 o_1 ... o_{n-1}" (n = B + 1 sequence starts), stdout "row seq" per layout.  Includes nothing of the library but that header.
#include <cstdio>
#include <vector>

#include "../sgpt_amd/csrc/encode_split.h"

int main() {
    long T, n;
    while (scanf("%ld %ld", &T, &n) == 2) {
        if (n < 1 || n > (1L << 24)) return 2;
        std::vector<int32_t> off((size_t)n);          // exactly B + 1 words: a read past them is the sanitizer's to report
        for (long i = 0; i < n; ++i) {
            long v;
            if (scanf("%ld", &v) != 1) return 2;
            off[(size_t)i] = (int32_t)v;
        }
        const EncodeSplit s = encode_split_point(off.data(), (int32_t)(n - 1), (int32_t)T);
        printf("%d %d\n", s.row, s.seq);
    }
    return 0;
}
