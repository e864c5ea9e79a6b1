// dev_hand_dump: hpe::build_dev_hand on the host alone.  Reads hpe_hand_params structs from the
// file argv[1], writes the DevHand built from each, one after the other, to argv[2]
// (tests/test_batch_hands_abi.py).  Built with hpe_host.cpp; no GPU, no libhpe.so.
#include <cstdio>
#include <vector>

#include "hpe_host.hpp"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 3;
    hpe_hand_params p;
    int n = 0;
    while (std::fread(&p, sizeof(p), 1, in) == 1) {
        DevHand h;
        hpe::build_dev_hand(p, h);
        if (std::fwrite(&h, sizeof(h), 1, out) != 1) return 4;
        ++n;
    }
    std::fclose(in);
    std::fclose(out);
    std::printf("dev_hand_dump ok: %d hands of %zu bytes\n", n, sizeof(DevHand));
    return 0;
}
