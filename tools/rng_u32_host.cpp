// Prints rng_u32 of csrc/vbg_common.h for a fixed list of (seed, stream, index): the fixture tests/golden/rng_u32.txt that ties
// tests/row_restate.py's numpy statement of the dropout RNG to the header itself.  Host only (rng_u32 is __host__ __device__):
//   hipcc --offload-host-only -x hip -O1 -I vibertgrid-pytorch_amd/csrc tools/rng_u32_host.cpp -o rng_u32_host && ./rng_u32_host > tests/golden/rng_u32.txt
#include <cstdio>

#include "vbg_common.h"

int main() {
    const unsigned long long seeds[] = {0ull, 1ull, 123ull, 0x5EEDull, 0x9E3779B1ull * 77 + 0x85EBCA6Bull, 0xFFFFFFFFFFFFFFFFull};
    const unsigned long long sids[] = {0ull, 1ull, 7ull, 1000ull, 1ull << 40, 0xFFFFFFFFFFFFFFFFull};
    const unsigned long long idxs[] = {0ull, 1ull, 2ull, 255ull, 768ull * 130 - 1, (1ull << 31) - 1, 1ull << 31, (1ull << 32) - 1, 1ull << 32,
                                       (1ull << 32) + 5, 3ull << 40, (1ull << 63) + 12345, 0xFFFFFFFFFFFFFFFFull};
    std::printf("# `seed stream index rng_u32` per line, then `thr p drop_threshold(p)`\n");
    for (unsigned long long seed : seeds)
        for (unsigned long long sid : sids)
            for (unsigned long long idx : idxs) std::printf("%llu %llu %llu %u\n", seed, sid, idx, vbg::rng_u32(seed, sid, idx));
    const float ps[] = {0.f, 0.1f, 0.5f, 0.25f, 0.9f, 0.999999f, 1e-10f};
    for (float p : ps) std::printf("thr %.9g %u\n", (double)p, vbg::drop_threshold(p));
    return 0;
}
