// grids_check: the grid rules of the data-path launches (ctstraffic_amd/csrc/cts_grids.hpp) as the launchers compute
// them, for tests/test_launch_depths_cpu.py. Arguments: tuples "n cus bpc chunk hint" (bpc stands for whichever
// blocks-per-CU value the rule takes); one line per tuple:
//   n cus bpc chunk hint  grid_for/1 grid_for/4 grid_for/16  contig.grid contig.per  batched ring  piece.grid piece.ppb
//   g++ -std=c++17 -Ictstraffic_amd/csrc tests/cpp/grids_check.cpp -o grids_check
#include <stdio.h>
#include <stdlib.h>

#include "cts_grids.hpp"

int main(int argc, char** argv)
{
    if (argc < 6 || (argc - 1) % 5 != 0) {
        fprintf(stderr, "usage: %s n cus bpc chunk hint [n cus bpc chunk hint ...]\n", argv[0]);
        return 2;
    }
    for (int k = 1; k + 4 < argc; k += 5) {
        const unsigned long long n = strtoull(argv[k], nullptr, 10);
        const long cus = strtol(argv[k + 1], nullptr, 10), bpc = strtol(argv[k + 2], nullptr, 10),
                   chunk = strtol(argv[k + 3], nullptr, 10);
        const unsigned long long hint = strtoull(argv[k + 4], nullptr, 10);
        if (n == 0 || n > 0xFFFFFFFFull || hint > 0xFFFFFFFFull || cus < 1) {
            fprintf(stderr, "n = %s, hint = %s or cus = %s is out of range\n", argv[k], argv[k + 4], argv[k + 1]);
            return 2;
        }
        const cts::ContigGrid cg = cts::contig_grid((uint32_t)n, (int)cus, (int)bpc, (int)chunk);
        const cts::PieceGrid pg = cts::piece_fill_grid((uint32_t)n, (uint32_t)hint, (int)cus, (int)bpc);
        printf("%llu %ld %ld %ld %llu %u %u %u %u %u %u %u %u %u\n", n, cus, bpc, chunk, hint,
               cts::grid_for((uint32_t)n, 1, (int)cus, (int)bpc), cts::grid_for((uint32_t)n, 4, (int)cus, (int)bpc),
               cts::grid_for((uint32_t)n, 16, (int)cus, (int)bpc), cg.grid, cg.per,
               cts::batched_fill_grid((uint32_t)n, (int)cus, (int)bpc), cts::ring_fill_grid((uint32_t)n, (int)cus, (int)bpc),
               pg.grid, pg.ppb);
    }
    return 0;
}
