// eval_host_check.cpp — the error table's host arithmetic and mask packing (mystereomatching_amd/csrc/sm_eval_core.h,
// what sm_eval_stage_host and sm_upload_truth run) as a stand-alone program, so that tests/test_eval_host.py can run
// them under -fsanitize=address,undefined without loading anything into Python.
//
// usage: eval_host_check ROWS COLS PRESENT IN.bin     (thresholds 1 and 2)
//   IN.bin   int16 disp[n], float gt[n], uint8 nonocc[n], all[n], disc[n]   (n = ROWS * COLS)
//   PRESENT  bit r set: mask r is passed; clear: a null pointer
//   stdout   the three 32-byte records
// Every array lives in a heap block of exactly its size, so a read past either end is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../mystereomatching_amd/csrc/sm_eval_core.h"

template <typename T>
static std::unique_ptr<T[]> read_block(FILE* f, size_t n) {
    std::unique_ptr<T[]> p(new T[n]);
    if (fread(p.get(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
    return p;
}

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const size_t rows = (size_t)atoi(argv[1]), cols = (size_t)atoi(argv[2]), n = rows * cols;
    const int present = atoi(argv[3]);
    FILE* f = fopen(argv[4], "rb");
    if (!f || n == 0) return 2;
    auto disp = read_block<int16_t>(f, n);
    auto gt = read_block<float>(f, n);
    std::unique_ptr<uint8_t[]> m[3];
    for (int r = 0; r < 3; r++) m[r] = read_block<uint8_t>(f, n);
    fclose(f);
    std::unique_ptr<uint8_t[]> region(new uint8_t[n]);
    sm::eval_pack_regions(n, (present & 1) ? m[0].get() : nullptr, (present & 2) ? m[1].get() : nullptr,
                          (present & 4) ? m[2].get() : nullptr, region.get());
    const sm::EvalThres th{{1.0f, 2.0f, 0.f, 0.f}, 2};
    sm_stage_err out[3];
    memset(out, 0, sizeof out);
    sm::eval_stage_host(disp.get(), gt.get(), region.get(), n, th, out);
    return fwrite(out, sizeof(sm_stage_err), 3, stdout) == 3 ? 0 : 1;
}
