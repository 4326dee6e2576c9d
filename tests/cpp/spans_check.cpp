// spans_check: the span geometry of the accounting passes (ctstraffic_amd/csrc/cts_spans.hpp) as the launchers
// compute it, for tests/test_accounting_seams_cpu.py. Arguments: pairs "n cus"; one line "n cus grid span" per pair.
//   g++ -std=c++17 -Ictstraffic_amd/csrc tests/cpp/spans_check.cpp -o spans_check
#include <stdio.h>
#include <stdlib.h>

#include "cts_spans.hpp"

int main(int argc, char** argv)
{
    if (argc < 3 || (argc - 1) % 2 != 0) {
        fprintf(stderr, "usage: %s n cus [n cus ...]\n", argv[0]);
        return 2;
    }
    for (int k = 1; k + 1 < argc; k += 2) {
        const unsigned long long n = strtoull(argv[k], nullptr, 10);
        const long cus = strtol(argv[k + 1], nullptr, 10);
        if (n == 0 || n > 0xFFFFFFFFull) {
            fprintf(stderr, "n = %s is outside 1 .. 2^32 - 1\n", argv[k]);
            return 2;
        }
        const cts::SpanGeometry g = cts::span_geometry((uint32_t)n, (int)cus);
        printf("%llu %ld %u %u\n", n, cus, g.grid, g.span);
    }
    return 0;
}
