// Stand-alone driver around the reference's own cost / arms / CBCA / SGM / WTA / scan-line functions, cut out
// of a reference checkout by oracle/ref_core.mk into oracle/_ref/src/core/{class.inc, members.inc} and compiled
// here inside a class declaration that is ours, over a cv::Mat that is ours (ref_shim/opencv_min.h).
// TEST INFRASTRUCTURE ONLY: it gives the tests an answer that is not a restatement.
//
//   ref_core_driver IN OUT
//
// IN : int32 magic 0x524f4352, H, W, D, fill, intersect, nops; H*W*3 bytes left BGR, the same right;
//      H*W bytes left gray, the same right; then nops records of int32 op, a, b, c (+ payload for op 4).
// OUT: what every op dumps, in order.  One StereoMatching object lives through all ops, constructed as
//      main_.cpp:138-139 does (Parameters(D - 1, H, W, 13, 1, 2, 109, 10, "", 1): main_.cpp:60-64's literals).
//   1 CENSUS            censusCal's own set-up (h x w x varNum CV_64F, zeroed; window {3, 4}, cpp:815-841),
//                       genCensusCode_NC_Sur(I_g, code, 3, 4)          -> code[0], code[1]: H*W*varNum uint64
//   2 ARMS              cbca_aggregate's prologue (cpp:5675-5678): initArm(), calArms<uchar>(I_c, HVL,
//                       HVL_INTERSECTION, crossL[0], crossL_out[0], cTresh[0], cTresh_out[0])
//                                                                      -> HVL[0], HVL[1]: H*W*5 uint16
//   3 COST a            a = 0: censusGrad(vm); a = 1: censusCal(vm, 1) (costCalculate, cpp:971-976)
//                                                                      -> vm[0], vm[1]: H*W*D float
//   4 SETVM a           vm[a] = the payload (H*W*D floats)              -> nothing
//   5 CBCA a            the prologue of op 2 unless done, cbca_core(HVL, HVL_INTERSECTION, vm, a)
//                                                                      -> vm[0], vm[1]
//   6 SCALE a           SolveAll with one level (cpp:2169-2205): sum = 0; sum += w * vm; vm = sum, w = the
//                       float whose bits are a (its matrix inverse needs OpenCV and stays out), both views
//                                                                      -> vm[0], vm[1]
//   7 SGM a b c         sgm(vm[a], c) with numOfDirec = b              -> vm[a]
//   8 WTA a             DP[a].create(h, w, CV_16S) (cpp:1048), gen_dispFromVm(vm[a], DP[a]) -> DP[a]: H*W int16
//   9 SO a b            DP[a].create; b = 0: so(vm[a], DP[a], I_c); 1: so_R2L(..); 2: so_T2D on vm[a].clone()
//                       (cpp:1096-1100)                                -> DP[a], then the accumulated volume
// Written by us around the cut text: the class head and tail, a no-op saveDispMap (grad() calls it to write
// its gradient images), tileCrossL sized to two empty Mats (calgradvm takes a pointer into tileCrossL[num]
// that it never follows, cpp:404; with the member vector empty even that is undefined), and main().
// Exit status 0 on success, 2 on a malformed call; a CV_Assert or an unbuilt stub aborts.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iostream>
#include <limits>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "opencv_min.h"

using namespace std;
using namespace cv;

int cv::shim_fill = 0;
static int ref_core_sgm_paths = 4;

class NLCCA;   // named by declarations only

class StereoMatching {
public:
    // the image / table writer grad() calls outside DEBUG (h:2005): nothing to write here
    template <typename T> void saveDispMap(const cv::Mat&, const Mat&, string, bool = false) {}
#include "core/class.inc"
};

#include "core/members.inc"

namespace {

bool read_all(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
bool write_all(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }

int fail(const char* what) {
    fprintf(stderr, "ref_core_driver: %s\n", what);
    return 2;
}

void ensure_arms(StereoMatching& sm) {   // cbca_aggregate(0, vm), cpp:5675-5678
    if (!sm.param_.has_initArm) sm.initArm();
    if (!sm.param_.has_calArms)
        sm.calArms<uchar>(sm.I_c, sm.HVL, sm.HVL_INTERSECTION, sm.param_.cbca_crossL[0], sm.param_.cbca_crossL_out[0],
                          sm.param_.cbca_cTresh[0], sm.param_.cbca_cTresh_out[0]);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return fail("usage: ref_core_driver IN OUT");
    FILE* in = fopen(argv[1], "rb");
    if (!in) return fail("cannot open the input file");
    int32_t hdr[7];
    if (!read_all(in, hdr, sizeof hdr)) return fail("short header");
    const int h = hdr[1], w = hdr[2], D = hdr[3], nops = hdr[6];
    if (hdr[0] != 0x524f4352 || h < 1 || w < 1 || D < 1 || D > 512 || hdr[4] < 0 || hdr[4] > 255 || nops < 0)
        return fail("bad header");
    cv::shim_fill = hdr[4];
    const size_t npix = (size_t)h * (size_t)w, nvol = npix * (size_t)D;

    Mat Ic[2] = {Mat(h, w, CV_8UC3), Mat(h, w, CV_8UC3)}, Ig[2] = {Mat(h, w, CV_8UC1), Mat(h, w, CV_8UC1)};
    if (!read_all(in, Ic[0].data, npix * 3) || !read_all(in, Ic[1].data, npix * 3) || !read_all(in, Ig[0].data, npix) ||
        !read_all(in, Ig[1].data, npix))
        return fail("short images");
    Mat none;
    StereoMatching::Parameters param(D - 1, h, w, 13, 1, 2, 109, 10, "", 1);
    param.cbca_intersect = hdr[5] != 0;
    StereoMatching sm(Ic[0], Ic[1], Ig[0], Ig[1], none, none, none, none, param);
    sm.tileCrossL.resize(2);

    FILE* out = fopen(argv[2], "wb");
    if (!out) return fail("cannot open the output file");
    bool ok = true;
    for (int i = 0; i < nops && ok; i++) {
        int32_t op[4];
        if (!read_all(in, op, sizeof op)) return fail("short op record");
        const int a = op[1], b = op[2], c = op[3];
        const bool view_ok = a == 0 || a == 1;
        switch (op[0]) {
            case 1: {
                const int RV = 3, RU = 4;
                int len = (RV * 2 + 1) * (RU * 2 + 1) * sm.param_.census_channel;
                if (sm.param_.censusFunc == 3) len += 8 * sm.param_.census_channel;
                int sz[3] = {h, w, (int)ceil(len / 64.)};
                vector<Mat> code(2);
                for (int k = 0; k < 2; k++) {
                    code[k].create(3, sz, CV_64F);
                    code[k] = 0;
                }
                sm.genCensusCode_NC_Sur(sm.I_g, code, RV, RU);
                for (int k = 0; k < 2; k++) ok = ok && write_all(out, code[k].data, code[k].bytes());
                break;
            }
            case 2:
                ensure_arms(sm);
                for (int k = 0; k < 2; k++) ok = ok && write_all(out, sm.HVL[k].data, sm.HVL[k].bytes());
                break;
            case 3:
                if (a == 0) sm.censusGrad(sm.vm);
                else if (a == 1) sm.censusCal(sm.vm, 1);
                else return fail("bad cost kind");
                for (int k = 0; k < 2; k++) ok = ok && write_all(out, sm.vm[k].data, nvol * 4);
                break;
            case 4:
                if (!view_ok) return fail("bad view");
                if (!read_all(in, sm.vm[a].data, nvol * 4)) return fail("short volume");
                break;
            case 5:
                if (a < 0 || a > 64) return fail("bad iteration count");
                ensure_arms(sm);
                sm.cbca_core(sm.HVL, sm.HVL_INTERSECTION, sm.vm, a);
                for (int k = 0; k < 2; k++) ok = ok && write_all(out, sm.vm[k].data, nvol * 4);
                break;
            case 6: {
                float wgt;
                memcpy(&wgt, &op[1], 4);
                for (int k = 0; k < 2; k++) {
                    float* p = (float*)sm.vm[k].data;
                    for (size_t j = 0; j < nvol; j++) {
                        float sum = 0;
                        sum += wgt * p[j];
                        p[j] = sum;
                    }
                    ok = ok && write_all(out, p, nvol * 4);
                }
                break;
            }
            case 7:
                if (!view_ok || (b != 4 && b != 8)) return fail("bad sgm call");
                ref_core_sgm_paths = b;
                sm.sgm(sm.vm[a], c != 0);
                ok = write_all(out, sm.vm[a].data, nvol * 4);
                break;
            case 8:
                if (!view_ok) return fail("bad view");
                sm.DP[a].create(h, w, CV_16S);
                sm.gen_dispFromVm(sm.vm[a], sm.DP[a]);
                ok = write_all(out, sm.DP[a].data, npix * 2);
                break;
            case 9: {
                if (!view_ok || b < 0 || b > 2) return fail("bad so call");
                sm.DP[a].create(h, w, CV_16S);
                Mat acc = sm.vm[a];
                if (b == 0) sm.so(sm.vm[a], sm.DP[a], sm.I_c);
                else if (b == 1) sm.so_R2L(sm.vm[a], sm.DP[a], sm.I_c);
                else {
                    acc = sm.vm[a].clone();
                    sm.so_T2D(acc, sm.DP[a], sm.I_c);
                }
                ok = write_all(out, sm.DP[a].data, npix * 2) && write_all(out, acc.data, nvol * 4);
                break;
            }
            default:
                return fail("bad op");
        }
    }
    fclose(in);
    if (fclose(out) != 0 || !ok) return fail("cannot write the output file");
    return 0;
}
