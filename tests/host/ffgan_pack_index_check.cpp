// Host-side dump of the FireflyGAN head's fragment index map (stabletts_amd/csrc/ffgan_launch.h: ffg_frag_source, ffg_frag_offset),
// compiled by tests/test_ffgan_split_cpu.py with hipcc --cuda-host-only; no GPU.
//   ffgan_pack_index_check cout cin taps u planes out.bin      (planes: 1 = default mode, 2 = f16 pairs, 3 = bf16 triples)
// writes, for every element idx of the hi stream, five int64: the index into v (-1: zero), its weight-norm scale row, and the
// element's offsets in the 16-bit buffer for planes 0, 1, 2 (-1 where the mode has no such plane).  The test compares the table with
// its Python restatement of the map.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../stabletts_amd/csrc/ffgan_launch.h"

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    const int cout = atoi(argv[1]), cin = atoi(argv[2]), taps = atoi(argv[3]), u = atoi(argv[4]);
    const int planes = atoi(argv[5]);
    const bool split = planes > 1;
    const long long n = (long long)(st::ffg_frag_bytes(cout, cin, taps, planes) / (2 * planes));
    std::vector<long long> table((size_t)n * 5);
    for (long long idx = 0; idx < n; ++idx) {
        int row = -1;
        table[idx * 5 + 0] = st::ffg_frag_source(idx, cout, cin, taps, u, split, &row);
        table[idx * 5 + 1] = row;
        for (int p = 0; p < 3; ++p) table[idx * 5 + 2 + p] = p < planes ? st::ffg_frag_offset(idx, planes, p) : -1;
    }
    FILE* f = fopen(argv[6], "wb");
    if (!f) return 3;
    const size_t wrote = fwrite(table.data(), sizeof(long long), table.size(), f);
    fclose(f);
    printf("elements %lld\n", n);
    return wrote == table.size() ? 0 : 4;
}
