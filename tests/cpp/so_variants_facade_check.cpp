// so_variants_facade_check.cpp — the C++ facade (include/stereo_matching.hpp) with the scan-line optimiser variants:
//   so_variants_facade_check LEFT.ppm RIGHT.ppm MAXDISP VARIANT OUT0.i16 OUT1.i16
// sets optimization = "so" and SO_VARIANT (0 so, 1 so_R2L, 2 so_T2D) as a main_.cpp would before constructing the
// object, runs costCalculate -> SolveAll(smPsy, 1, 0.3) -> dispOptimize on one pair (main_.cpp:139-164) and writes
// DP[0] and DP[1] (int16, rows x cols each).  It prints the variant.
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "stereo_matching.hpp"

using namespace smamd;
using namespace std;

string StereoMatching::costcalculation = "censusGrad";
string StereoMatching::aggregation = "CBCA";
string StereoMatching::optimization = "so";
string StereoMatching::object = "";
const string StereoMatching::root = "";

static bool dump(const char* path, const Mat& m) {
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    for (int r = 0; r < m.rows; r++) fwrite(m.ptr<int16_t>(r), sizeof(int16_t), (size_t)m.cols, f);
    fclose(f);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 7) {
        cerr << "usage: so_variants_facade_check LEFT.ppm RIGHT.ppm MAXDISP VARIANT OUT0.i16 OUT1.i16" << endl;
        return 2;
    }
    Mat I1_c = imread(argv[1], 1), I2_c = imread(argv[2], 1);
    Mat I1 = imread(argv[1], 0), I2 = imread(argv[2], 0);
    if (I1_c.empty() || I2_c.empty()) {
        cout << "can't read original img" << endl;
        return -1;
    }
    try {
        static_assert(SM_SO_L2R == 0 && SM_SO_R2L == 1 && SM_SO_T2D == 2, "sm_so_config's variants");
        if (StereoMatching::SO_VARIANT != SM_SO_L2R || StereoMatching::SO_PN2 != SM_SO_PN_DEFAULT ||
            StereoMatching::SO_PN3 != SM_SO_PN_DEFAULT)
            return 5;   // the shipped call is the default
        StereoMatching::SO_VARIANT = atoi(argv[4]);
        printf("SO_VARIANT %d\n", StereoMatching::SO_VARIANT);
        StereoMatching::Parameters param(atoi(argv[3]), I1_c.rows, I1_c.cols);
        StereoMatching* smPsy[1] = {new StereoMatching(I1_c, I2_c, I1, I2, param)};
        smPsy[0]->costCalculate();
        SolveAll(smPsy, 1, 0.3f);
        smPsy[0]->dispOptimize();
        const bool ok = dump(argv[5], smPsy[0]->DP[0]) && dump(argv[6], smPsy[0]->DP[1]);
        delete smPsy[0];
        if (!ok) return 3;
    } catch (const std::exception& e) {
        cerr << e.what() << endl;
        return 4;
    }
    return 0;
}
