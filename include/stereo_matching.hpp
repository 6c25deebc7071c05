// stereo_matching.hpp — header-only C++ facade with the reference's class API over sm_capi.h.
//
// Source-compatible with the reference driver's use of class StereoMatching (main_.cpp:130-178):
// a user replaces `#include "stereoMatching.h"` and OpenCV's Mat/imread/pyrDown by this header
// (`using namespace smamd;` in place of `using namespace cv;`) and keeps the call sequence:
//
//   string StereoMatching::costcalculation = "censusGrad";     // main_.cpp:15-19: the program
//   string StereoMatching::aggregation = "CBCA";               // defines the static selectors,
//   string StereoMatching::optimization = "sgm";               // exactly as the reference's
//   string StereoMatching::object = "";                        // header declares them (h:50-54)
//   const string StereoMatching::root = "...";
//   ...
//   StereoMatching::Parameters param(maxDisp, rows, cols, lamCen, lamG, M, lamc, ts, csv, disSc);  // main:138
//   smPsy[p] = new StereoMatching(I1_c, I2_c, I1, I2, DT, all, nonocc, disc, param);              // main:139
//   smPsy[p]->costCalculate();                                  // cpp:945-1021
//   pyrDown(I1_c, I1_c); ...                                    // main:145-154
//   SolveAll(smPsy, PY_LEV, REG_LAMBDA);                        // cpp:2142-2208
//   smPsy[0]->openCSV(); smPsy[0]->dispOptimize();              // main:159-163, cpp:1046-1136
//   if (StereoMatching::Do_refine) smPsy[0]->refine();          // main:165-166
//   smPsy[0]->closeCSV(); smPsy[0]->saveTime(time, "all");      // main:168-171
//   const int16_t* d = smPsy[0]->DP[0].ptr<int16_t>(0);         // public member DP (h:2724)
//
// smamd::Mat mirrors the part of cv::Mat the driver touches: reference-counted shallow copies
// (the reference's ctor keeps headers of the caller's images, cpp:2066-2075), rows/cols/step/data,
// empty(), channels(), ptr<T>(row), convertTo(CV_32F, alpha).  imread reads PNG (main_.cpp:92-107
// reads the Middlebury *.png files; decoded here with zlib, link -lz) and binary PNM (P5 gray, P6
// colour): flags 1 -> 3-channel BGR, 0 -> gray with libpng's rgb_to_gray weights, the formula
// OpenCV's PNG decoder uses.  All compute runs in libsm_hip.so on
// the GPU; the library does no file I/O, so openCSV/closeCSV/saveTime keep their records in memory
// (the reference wrote savePath files and exit()ed on failure, h:1727-1744).  Non-OK statuses
// become std::runtime_error (the reference threw cv::Exception from CV_Assert).
#pragma once
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
#include <iterator>
#include <memory>
#include <new>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "sm_capi.h"

#if __has_include(<zlib.h>)
#include <zlib.h>
#define SMAMD_HAVE_PNG 1
#else
#define SMAMD_HAVE_PNG 0
#endif

namespace smamd {

// OpenCV depth codes used by the driver (CV_8U images, CV_16S DP, CV_32F DT)
enum { CV_8U = 0, CV_16S = 3, CV_32F = 5 };

#ifndef CV_Assert
#define CV_Assert(expr) \
    do { if (!(expr)) throw std::runtime_error("Assertion failed: " #expr); } while (0)
#endif

inline int& default_device() {   // HIP device for the free functions (pyrDown); ctor takes its own
    static int dev = 0;
    return dev;
}

class Mat {
   public:
    int rows = 0, cols = 0;
    size_t step = 0;             // bytes per row
    uint8_t* data = nullptr;

    Mat() = default;
    Mat(int nrows, int ncols, int depth, int channels = 1) { create(nrows, ncols, depth, channels); }
    // non-owning view of caller memory (e.g. a cv::Mat: view(m.rows, m.cols, m.channels(), m.step, m.data))
    static Mat view(int nrows, int ncols, int channels, size_t row_step, const void* ptr0, int depth = CV_8U) {
        Mat m;
        m.rows = nrows, m.cols = ncols, m.cn_ = channels, m.depth_ = depth, m.step = row_step;
        m.data = (uint8_t*)ptr0;
        return m;
    }
    void create(int nrows, int ncols, int depth, int channels = 1) {
        rows = nrows, cols = ncols, depth_ = depth, cn_ = channels;
        step = (size_t)cols * elemSize();
        buf_ = std::make_shared<std::vector<uint8_t>>(step * rows);
        data = buf_->data();
    }
    bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
    int channels() const { return cn_; }
    int depth() const { return depth_; }
    int type() const { return depth_ + ((cn_ - 1) << 3); }   // CV_MAKETYPE
    size_t elemSize1() const { return depth_ == CV_8U ? 1 : depth_ == CV_16S ? 2 : 4; }
    size_t elemSize() const { return elemSize1() * cn_; }
    bool isContinuous() const { return step == (size_t)cols * elemSize(); }
    template <typename T> T* ptr(int r = 0) { return (T*)(data + (size_t)r * step); }
    template <typename T> const T* ptr(int r = 0) const { return (const T*)(data + (size_t)r * step); }
    Mat clone() const {
        Mat m(rows, cols, depth_, cn_);
        for (int r = 0; r < rows; r++) std::memcpy(m.ptr<uint8_t>(r), ptr<uint8_t>(r), (size_t)cols * elemSize());
        return m;
    }
    // Mat::convertTo(dst, rtype, alpha, beta) for u8 / s16 / f32 -> f32 (main_.cpp:127-129:
    // DT.convertTo(DT, CV_32F, 1.0 / disp_reduceCoeff)): (float)v * (float)alpha + (float)beta
    void convertTo(Mat& dst, int rtype, double alpha = 1, double beta = 0) const {
        if (rtype != CV_32F) throw std::invalid_argument("convertTo: only CV_32F targets are supported");
        Mat out(rows, cols, CV_32F, cn_);
        const float a = (float)alpha, b = (float)beta;
        for (int r = 0; r < rows; r++) {
            float* o = out.ptr<float>(r);
            for (int i = 0; i < cols * cn_; i++) {
                const float v = depth_ == CV_8U ? (float)ptr<uint8_t>(r)[i]
                                : depth_ == CV_16S ? (float)ptr<int16_t>(r)[i] : ptr<float>(r)[i];
                o[i] = b == 0.f ? v * a : v * a + b;
            }
        }
        dst = out;   // a new buffer; other headers of the old one keep it (cv::Mat semantics)
    }
    // rows x cols x channels packed copy of the pixels (host), element type T
    template <typename T> std::vector<T> packed() const {
        std::vector<T> v((size_t)rows * cols * cn_);
        for (int r = 0; r < rows; r++) std::memcpy(v.data() + (size_t)r * cols * cn_, ptr<uint8_t>(r), (size_t)cols * elemSize());
        return v;
    }

   private:
    int depth_ = CV_8U, cn_ = 1;
    std::shared_ptr<std::vector<uint8_t>> buf_;
};

namespace detail {

// Largest image imread accepts (pixels): header sizes above it, or whose products would overflow,
// are rejected before anything is allocated (a crafted header must not wrap a buffer size).
constexpr uint64_t kMaxImagePixels = 1ull << 28;
inline bool size_ok(int64_t w, int64_t h) { return w >= 1 && h >= 1 && (uint64_t)w * (uint64_t)h <= kMaxImagePixels; }

// Decoded 8-bit pixels: w x h, cin = 1 (gray) or 3 (R, G, B), row-major.
struct Pixels {
    int w = 0, h = 0, cin = 0;
    std::vector<uint8_t> px;
};

inline bool read_pnm(std::ifstream& f, Pixels& out) {
    std::string magic;
    int w = 0, h = 0, maxv = 0;
    if (!(f >> magic >> w >> h >> maxv) || (magic != "P6" && magic != "P5") || maxv != 255 || !size_ok(w, h))
        return false;
    f.get();
    out.w = w, out.h = h, out.cin = magic == "P6" ? 3 : 1;
    out.px.resize((size_t)w * h * out.cin);
    return (bool)f.read((char*)out.px.data(), (std::streamsize)out.px.size());
}

#if SMAMD_HAVE_PNG
inline uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// PNG (ISO/IEC 15948) the way OpenCV's PngDecoder delivers it to imread(.., 0 / 1): 8-bit samples
// (1/2/4-bit gray expanded to 8 bits, 16-bit samples stripped to their high byte as
// png_set_strip_16 does, palettes expanded to RGB, alpha dropped).  Non-interlaced images only.
inline bool read_png(const std::vector<uint8_t>& file, Pixels& out) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (file.size() < 8 || std::memcmp(file.data(), sig, 8) != 0) return false;
    int64_t w = 0, h = 0;
    int depth = 0, ctype = -1, interlace = 0;
    std::vector<uint8_t> idat, plte;
    for (size_t pos = 8; pos + 12 <= file.size();) {
        const uint32_t len = be32(&file[pos]);
        if (pos + 12 + (size_t)len > file.size()) return false;
        const uint8_t* type = &file[pos + 4];
        const uint8_t* data = &file[pos + 8];
        if (!std::memcmp(type, "IHDR", 4) && len >= 13) {
            w = be32(data), h = be32(data + 4), depth = data[8], ctype = data[9], interlace = data[12];
        } else if (!std::memcmp(type, "PLTE", 4)) {
            plte.assign(data, data + len);
        } else if (!std::memcmp(type, "IDAT", 4)) {
            idat.insert(idat.end(), data, data + len);
        } else if (!std::memcmp(type, "IEND", 4)) {
            break;
        }
        pos += 12 + (size_t)len;
    }
    // samples per pixel by colour type: 0 gray, 2 RGB, 3 palette index, 4 gray + alpha, 6 RGBA
    const int spp = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0;
    const bool depth_ok = depth == 8 || depth == 16 || ((ctype == 0 || ctype == 3) && (depth == 1 || depth == 2 || depth == 4));
    // (w * h <= 2^28 keeps every size below in 64-bit range: stride <= 8 w + 1)
    if (!size_ok(w, h) || spp == 0 || !depth_ok || interlace != 0 || (ctype == 3 && (plte.empty() || depth == 16)))
        return false;
    const size_t bpp = std::max<size_t>(1, (size_t)spp * depth / 8);     // filter byte distance
    const size_t stride = ((size_t)w * spp * depth + 7) / 8;             // bytes per scanline
    // zlib's deflate expands at most ~1032:1: an IDAT far too short for the header's size is
    // rejected before the scanline buffer is allocated
    if ((uint64_t)h * (stride + 1) > (uint64_t)idat.size() * 1100 + 4096) return false;
    std::vector<uint8_t> raw(h * (stride + 1));
    uLongf rlen = (uLongf)raw.size();
    if (uncompress(raw.data(), &rlen, idat.data(), (uLong)idat.size()) != Z_OK || rlen != raw.size()) return false;
    // undo the per-scanline filters (None, Sub, Up, Average, Paeth)
    std::vector<uint8_t> img((size_t)h * stride);
    for (int y = 0; y < h; y++) {
        const uint8_t ft = raw[(size_t)y * (stride + 1)];
        const uint8_t* src = &raw[(size_t)y * (stride + 1) + 1];
        uint8_t* cur = &img[(size_t)y * stride];
        const uint8_t* up = y > 0 ? &img[(size_t)(y - 1) * stride] : nullptr;
        for (size_t i = 0; i < stride; i++) {
            const int a = i >= bpp ? cur[i - bpp] : 0, b = up ? up[i] : 0, c = (up && i >= bpp) ? up[i - bpp] : 0;
            int x = src[i];
            switch (ft) {
                case 0: break;
                case 1: x += a; break;
                case 2: x += b; break;
                case 3: x += (a + b) / 2; break;
                case 4: {
                    const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
                    x += (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
                    break;
                }
                default: return false;
            }
            cur[i] = (uint8_t)x;
        }
    }
    out.w = (int)w, out.h = (int)h, out.cin = (ctype == 0 || ctype == 4) ? 1 : 3;
    out.px.assign((size_t)w * h * out.cin, 0);
    for (int y = 0; y < h; y++) {
        const uint8_t* row = &img[(size_t)y * stride];
        for (int x = 0; x < w; x++) {
            uint8_t* o = &out.px[((size_t)y * w + x) * out.cin];
            if (depth < 8) {   // packed gray / palette indices, most significant bits first
                const int per = 8 / depth, shift = 8 - depth * (x % per + 1);
                const int v = (row[x / per] >> shift) & ((1 << depth) - 1);
                if (ctype == 3) {
                    if ((size_t)v * 3 + 2 >= plte.size()) return false;
                    o[0] = plte[v * 3], o[1] = plte[v * 3 + 1], o[2] = plte[v * 3 + 2];
                } else {
                    o[0] = (uint8_t)(v * 255 / ((1 << depth) - 1));
                }
                continue;
            }
            const size_t bs = depth / 8;   // bytes per sample; 16-bit: the high byte comes first
            const uint8_t* p = row + (size_t)x * spp * bs;
            if (ctype == 3) {
                const int v = p[0];
                if ((size_t)v * 3 + 2 >= plte.size()) return false;
                o[0] = plte[v * 3], o[1] = plte[v * 3 + 1], o[2] = plte[v * 3 + 2];
            } else {
                for (int k = 0; k < out.cin; k++) o[k] = p[k * bs];
            }
        }
    }
    return true;
}
#endif

inline Mat imread_impl(const std::string& path, int flags) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return Mat();
    detail::Pixels d;
    const int first = f.peek();
#if SMAMD_HAVE_PNG
    if (first == 0x89) {
        std::vector<uint8_t> file((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (!detail::read_png(file, d)) return Mat();
    } else
#endif
        if (first != 'P' || !detail::read_pnm(f, d)) {
        return Mat();
    }
    const int w = d.w, h = d.h, cin = d.cin;
    const std::vector<uint8_t>& px = d.px;
    Mat m(h, w, CV_8U, flags == 0 ? 1 : 3);
    for (size_t i = 0; i < (size_t)w * h; i++) {
        const uint8_t R = px[i * cin], G = px[i * cin + (cin - 1) / 2], B = px[i * cin + cin - 1];
        if (flags == 0) {
            m.data[i] = cin == 1 ? R : (uint8_t)((R * 9798 + G * 19235 + B * 3735 + 16384) >> 15);
        } else {
            m.data[i * 3] = B, m.data[i * 3 + 1] = G, m.data[i * 3 + 2] = R;
        }
    }
    return m;
}
}  // namespace detail

// cv::imread for PNG (when zlib is available) and binary PNM (P6 RGB / P5 gray, maxval 255).
// flags 1: 3-channel BGR; flags 0: gray ((R*9798 + G*19235 + B*3735 + 16384) >> 15, libpng's
// rgb_to_gray).  Empty Mat on failure (main_.cpp:108 tests empty()).
inline Mat imread(const std::string& path, int flags = 1) {
    try {
        return detail::imread_impl(path, flags);
    } catch (const std::bad_alloc&) {   // an image too large for this host: empty Mat, as documented
        return Mat();
    } catch (const std::length_error&) {
        return Mat();
    }
}

// cv::pyrDown (main_.cpp:145-154) on the GPU: u8 with 1 or 3 channels (the inputs, masks) or
// 1-channel f32 (the ground truth DT).  dst gets a new buffer of (rows+1)/2 x (cols+1)/2.
inline void pyrDown(const Mat& src, Mat& dst) {
    if (src.empty()) throw std::invalid_argument("pyrDown: empty source");
    Mat out((src.rows + 1) / 2, (src.cols + 1) / 2, src.depth(), src.channels());
    sm_status s;
    if (src.depth() == CV_8U) {
        const std::vector<uint8_t> in = src.packed<uint8_t>();
        s = sm_pyr_down(default_device(), in.data(), src.rows, src.cols, src.channels(), out.data);
    } else if (src.depth() == CV_32F && src.channels() == 1) {
        const std::vector<float> in = src.packed<float>();
        s = sm_pyr_down_f32(default_device(), in.data(), src.rows, src.cols, (float*)out.data);
    } else {
        throw std::invalid_argument("pyrDown: u8 (1/3 channels) or 1-channel f32 only");
    }
    if (s != SM_OK) throw std::runtime_error(std::string("pyrDown: ") + sm_status_string(s));
    dst = out;
}

class StereoMatching {
   public:
    // static selectors (h:50-54): declared here, defined once by the program (main_.cpp:15-19)
    static const std::string root;
    static std::string costcalculation;
    static std::string aggregation;
    static std::string optimization;
    static std::string object;
    // compile-time switches (h:57-83); static const in the reference, settable here before a ctor
    static constexpr bool preMedBlur = false;      // h:66
    inline static bool Do_refine = false;          // h:70
    static constexpr bool Do_LRConsis = true;      // h:72
    inline static bool Do_regionVote = true;       // h:75
    // three more of refine()'s stages (h:73-81; sm_refine_ext_config), off in the shipped build: the peak-ratio
    // check (calPKR + signDp_UsingPKR), the background fill (BGIpol) and the sub-pixel map (subpixelEnhancement +
    // its float median), which refine() leaves in SE.  Set before the object is constructed.
    inline static bool Do_calPKR = false;
    inline static bool Do_bgIpol = false;
    inline static bool Do_subpixelEnhancement = false;
    // SE's form: false reproduces the reference's `disp -= diff` on a short (cpp:6161: the float difference
    // converted back, truncating toward zero), true keeps the float
    inline static bool SE_FLOAT = false;
    inline static float pkr_ratio = 0.1f;          // calPKR's local ratio_PKR (cpp:4093)
    // refine()'s discontinuity adjustment (h:78; sm_refine_da_config): equalizeHist, GaussianBlur and Canny on DP[0]
    // as 8 bits, then the raster-order pass of cpp:6069-6135; refine() leaves the edge map in DA_Edge.  The
    // thresholds and the blur's 8.8 fixed-point taps are the literals of cpp:6063-6064 in the restated form
    inline static bool Do_discontinuityAdjust = false;
    inline static int da_canny_low = 20, da_canny_high = 60, da_blur_side = 84, da_blur_centre = 87;
    // two source switches of refine() (sm_refine_outlier_config), commented out in the shipped build: LRC_CLASSIFY
    // runs LRConsistencyCheck (cpp:1367, 2284-2335: failed pixels become DISP_OCC / DISP_MIS, the mask is left in
    // LRC_Err_Mask) instead of LRConsistencyCheck_normal; RV_COMBINE_BG runs RV_combine_BG (cpp:1408, 7146-7216: a
    // float ratio, the filler chosen per class by Parameters::interpolateType) instead of regionVote_my
    inline static bool LRC_CLASSIFY = false;
    inline static bool RV_COMBINE_BG = false;
    // which scan-line optimiser dispOptimize's "so" branch calls (cpp:1096-1100; sm_so_config): SM_SO_L2R = so (the
    // shipped call), SM_SO_R2L = so_R2L (cpp:6683-6826), SM_SO_T2D = so_T2D (cpp:6580-6681, on a clone: vm[i] stays
    // as aggregated).  SO_PN2 / SO_PN3 replace the chosen function's literals (SM_SO_PN_DEFAULT keeps them)
    inline static int SO_VARIANT = SM_SO_L2R;
    inline static float SO_PN2 = SM_SO_PN_DEFAULT, SO_PN3 = SM_SO_PN_DEFAULT;
    // the scan-line optimisers' float-minima kernels (sm_create_ex, so_float_minima): -1 = automatic, on where "so"
    // follows GF, GFNL or BF over a gradient cost method (signed or NaN costs; the reference runs them without a
    // switch); 0 / 1 force it
    inline static int SO_FLOAT_MINIMA = -1;
    // the reference's err txt (saveFromDisp -> calErr after dispOptimize and after refine()'s stages; sm_eval_config):
    // with DT given, the table is built on the GPU while dispOptimize and refine() run; stageErrors() returns its rows
    inline static bool Do_stageErrors = false;
    inline static bool Do_properIpol = true;       // h:76
    inline static bool Do_lastMedianBlur = true;   // h:80
    // `#define MY_GUIDE` (h:38, commented out in the shipped build) as a switch: false = GF runs
    // cv::ximgproc::guidedFilter (cpp:4513), true = guideFilterCore_matlab (cpp:4509)
    inline static bool gf_my_guide = false;
    // costCalculate's "FIF" branch calls FIF_Improve (cpp:1010-1012, `//FIF();` commented out):
    // true selects the plain form FIF (cpp:4541-4705) instead
    inline static bool fif_plain = false;
    // AWS()'s function-local constants W_V_AWS, W_U_AWS (cpp:5715) and r_c (h:1478), read with
    // aggregation == "AWS" (sm_aws_config: radii in [0, 17], gamma_c > 0)
    inline static int aws_radius_v = 17, aws_radius_u = 17;
    inline static float aws_gamma_c = 5.0f;
    // BF()'s literal Size(12, 12) (cpp:1038; height, width) and GFNL()'s literal variance threshold
    // (cpp:4470), read with aggregation == "BF" / "GFNL" (sm_bf_config, sm_gfnl_config)
    inline static int bf_ksize_v = 12, bf_ksize_u = 12;
    inline static float gfnl_var_thresh = 400.0f;

    struct Parameters {  // StereoMatching::Parameters (h:85-351), the fields the hot path reads
        int numDisparities, rows, cols;
        int lamCen, lamG, disSc;
        int vmTop_Num, ts;
        float vmTop_thres;
        // dispOptimize's candidate-disparity selection (h:182-188, 320-326; sm_vmtop_config): set before the
        // object is constructed
        bool Do_vmTop = false;
        int vmTop_method = 0;
        int vmTop_thres_dirNum = 8;           // carried; genDispFromTopCostVm2 does not read it
        bool vmTop_hasCir2 = true;
        bool vmTop_cir3_doColorLimit = false;
        std::string errCsvName;
        int censusFunc = 3;                   // h:244
        int cbca_iterationNum = 2, cbca_minArmL = 1;
        // the three cross windows (h:140-143, 263-274).  Index 0 is CBCA's window; index 1 is the second window
        // of the double-window branch; index 2 is carried (no code path of the hot path reads it)
        unsigned char cbca_crossL[3] = {17, 23, 34};
        unsigned char cbca_crossL_out[3] = {34, 23, 34};
        unsigned char cbca_cTresh[3] = {20, 30, 30};
        unsigned char cbca_cTresh_out[3] = {6, 0, 0};
        // CBCA()'s double-window branch (h:144, 275; cpp:4337-4357; sm_cbca_double_config): set before the object
        // is constructed.  Both aggregations then do two iterations whatever cbca_iterationNum says.
        bool cbca_double_win = false;
        // h:139, 262; false: cross-based aggregation without arm intersection (sm_cbca_intersect_config): the view's
        // own arms, one area per pixel.  Set before the object is constructed; only "CBCA" reads it.
        bool cbca_intersect = true;
        // GF()'s double-window switch (h:145, 276): both arms of the reference's branch run guideFilter(0, vm)
        // (cpp:4406-4418), so the field is accepted and changes nothing
        bool GF_double_win = false;
        int sgm_scanNum = 4, sgm_corDifThres = 15, sgm_reduCoeffi1 = 4;
        int errorThreshold = 1;               // h:225
        float LRmaxDiff = 0;                  // h:212
        int DISP_OCC = -2 * 16;               // h:216
        int DISP_MIS = -3 * 16;               // h:217
        int DISP_PKR = -4 * 16;               // h:218
        int interpolateType = 0;              // h:178, 310: RV_combine_BG's filler (RV_COMBINE_BG)
        int bgIplDepth = 1000;                // h:311
        int region_vote_nums = 2;             // h:306
        // Parameters(maxDisp, h, w, lamCen, lamG, M, lamc, ts, errCsvName, disSc) — main_.cpp:138
        Parameters(int maxDisp, int h, int w, int lamCen_ = 13, int lamG_ = 1, int M = 2, int lamc = 109,
                   int ts_ = 10, const std::string& errCsvName_ = "", int disSc_ = 1)
            : numDisparities(maxDisp + 1), rows(h), cols(w), lamCen(lamCen_), lamG(lamG_), disSc(disSc_),
              vmTop_Num(M), ts(ts_), vmTop_thres((float)(lamc * 0.01)),   // the product in double, then one rounding (h:323)
              errCsvName(errCsvName_) {}
    };

    struct RegionErr {            // one line of calErr's report (h:1798-1799)
        std::string region;
        float PBM, RMS;
    };

    // StereoMatching(I1_c, I2_c, I1_g, I2_g, DT, all_mask, nonocc_mask, disc_mask, param) — cpp:2058;
    // main_.cpp:139.  DT and the masks are kept (shallow, like the reference's headers) for calErr.
    StereoMatching(Mat& I1_c, Mat& I2_c, Mat& I1_g, Mat& I2_g, Mat& DT_, Mat& all_mask, Mat& nonocc_mask,
                   Mat& disc_mask, const Parameters& param, int hip_device = 0)
        : param_(param), h_(I1_c.rows), w_(I1_c.cols), d_(param.numDisparities) {
        DT = DT_;
        I_mask[0] = nonocc_mask;   // cpp:2073-2075
        I_mask[1] = all_mask;
        I_mask[2] = disc_mask;
        init_or_release(I1_c, I2_c, I1_g, I2_g, hip_device);
    }
    // without ground truth (no calErr)
    StereoMatching(const Mat& I1_c, const Mat& I2_c, const Mat& I1_g, const Mat& I2_g, const Parameters& param,
                   int hip_device = 0)
        : param_(param), h_(I1_c.rows), w_(I1_c.cols), d_(param.numDisparities) {
        init_or_release(I1_c, I2_c, I1_g, I2_g, hip_device);
    }
    ~StereoMatching() { sm_destroy(ctx_); }
    StereoMatching(const StereoMatching&) = delete;
    StereoMatching& operator=(const StereoMatching&) = delete;

    void costCalculate() { check(sm_cost_calculate(ctx_), "costCalculate"); }
    void dispOptimize() {  // DP[0] (and DP[1] when Do_refine, or with "so": cpp:1093), cpp:1046-1136
        DP[0].create(h_, w_, CV_16S);
        check(sm_disp_optimize(ctx_, DP[0].ptr<int16_t>()), "dispOptimize");
        if (refine_on_ || (optimization == "so" && Do_LRConsis)) {
            DP[1].create(h_, w_, CV_16S);
            check(sm_get_disp(ctx_, 1, DP[1].ptr<int16_t>()), "DP[1]");
        }
    }
    void refine() {  // cpp:1138-1511; needs Do_refine at construction
        DP[0].create(h_, w_, CV_16S);
        check(sm_refine(ctx_, DP[0].ptr<int16_t>()), "refine");
        if (pkr_on_) {
            PKR_Err_Mask.create(h_, w_, CV_8U);
            check(sm_get_pkr_mask(ctx_, PKR_Err_Mask.ptr<uint8_t>()), "PKR_Err_Mask");
        }
        if (lrc_on_) {
            LRC_Err_Mask.create(h_, w_, CV_8U);
            check(sm_get_lrc_mask(ctx_, LRC_Err_Mask.ptr<uint8_t>()), "LRC_Err_Mask");
        }
        if (da_on_) {
            DA_Edge.create(h_, w_, CV_8U);
            check(sm_get_da_edges(ctx_, DA_Edge.ptr<uint8_t>()), "DA_Edge");
        }
        if (se_on_) {
            SE.create(h_, w_, CV_32F);
            check(sm_get_subpixel(ctx_, SE.ptr<float>()), "SE");
        }
    }
    void pipeline() {  // cpp:1950-1981 (no SolveAll)
        costCalculate();
        dispOptimize();
        if (Do_refine) refine();
    }
    std::vector<float> volume(int view = 0) {   // public member vm[view] (h:2720)
        std::vector<float> v((size_t)h_ * w_ * d_);
        check(sm_get_volume(ctx_, view, v.data()), "vm");
        return v;
    }

    // CSV of per-object error ratios (cpp:1940-1948): the rows calErr(.., calCSV = true) appends
    // are kept in csv() instead of a file under savePath.
    void openCSV() { csv_open_ = true; }
    void closeCSV() {
        if (csv_open_) csv_ << "\n";
        csv_open_ = false;
    }
    const std::string csv() const { return csv_.str(); }
    // saveTime(ms, procedure) (h:1727-1744): "procedure: ms" records, kept in times()
    void saveTime(long ms, const std::string& procedure) { times_.push_back(procedure + ": " + std::to_string(ms)); }
    const std::vector<std::string>& times() const { return times_; }

    // calErr<T>(DP, DT, procedure, calCSV) (h:1748-1825): per region mask (nonocc, all, disc; empty
    // masks skipped) the bad ratio PBM (DP < 0 or |DT - DP| > errorThreshold) and the RMS, printed
    // like the reference and returned; the float arithmetic is sm_cal_err's (the reference's order).
    template <typename T = int16_t>
    std::vector<RegionErr> calErr(Mat& DP_, Mat& DT_, const std::string& procedure, bool calCSV = false) {
        static_assert(sizeof(T) == 2, "DP is CV_16S");
        if (DP_.empty() || DT_.empty() || DT_.depth() != CV_32F || DP_.rows != DT_.rows || DP_.cols != DT_.cols)
            throw std::invalid_argument("calErr: DP (CV_16S) and DT (CV_32F) of one size required");
        static const char* names[3] = {"nonocc", "all", "disc"};
        std::vector<RegionErr> out;
        const std::vector<int16_t> dp = DP_.packed<int16_t>();
        const std::vector<float> dt = DT_.packed<float>();
        for (int region = 0; region < 3; region++) {
            if (I_mask[region].empty()) continue;
            const std::vector<uint8_t> m = I_mask[region].packed<uint8_t>();
            RegionErr e{names[region], 0.f, 0.f};
            check(sm_cal_err(dp.data(), dt.data(), m.data(), DP_.rows, DP_.cols, (float)param_.errorThreshold, &e.PBM,
                             &e.RMS),
                  "calErr");
            std::cout << "\n" << e.region << "\terrorRatio: " << e.PBM << " epe: " << e.RMS << " " + procedure << "\n";
            if (calCSV && csv_open_) csv_ << e.PBM << ",";
            out.push_back(e);
        }
        return out;
    }
    std::vector<RegionErr> calErr() { return calErr<int16_t>(DP[0], DT, "DP0"); }

    // The err-txt rows of the last dispOptimize (+ refine): one per stage at which the reference calls
    // saveFromDisp<short, 0> and per region whose mask was given, from the table the GPU built (sm_get_stage_errors),
    // with PBM = (float)bad / count and RMS = sqrtf((float)sum_sq / count), 0 for an empty region.
    struct StageErr {
        std::string procedure, region;
        float PBM, RMS;
    };
    std::vector<StageErr> stageErrors() {
        if (!eval_on_) throw std::logic_error("stageErrors needs StereoMatching::Do_stageErrors = true and DT at construction");
        static const char* names[3] = {"nonocc", "all", "disc"};
        const int S = sm_eval_stage_count(ctx_);
        std::vector<sm_stage_err> t((size_t)std::max(S, 1) * 3);
        check(sm_get_stage_errors(ctx_, 1, t.data()), "stageErrors");
        std::vector<StageErr> out;
        for (int s = 0; s < S; s++)
            for (int region = 0; region < 3; region++) {
                if (I_mask[region].empty()) continue;
                const sm_stage_err& e = t[(size_t)s * 3 + region];
                StageErr r{sm_eval_stage_name(ctx_, s), names[region], 0.f, 0.f};
                if (e.count) {
                    r.PBM = (float)e.bad[0] / e.count;
                    r.RMS = sqrtf((float)e.sum_sq / e.count);
                }
                out.push_back(r);
            }
        return out;
    }
    // the rows as calErr writes them to the err txt (h:1756, 1799, 1817): one line per stage
    std::string stageErrorsText() {
        std::ostringstream o;
        std::string last;
        bool first = true;
        for (const StageErr& r : stageErrors()) {
            if (first || r.procedure != last) o << (first ? "" : "\n") << r.procedure << "\t";
            o << r.region << "\tPBM: " << r.PBM << "\tRMS: " << r.RMS << "\t";
            last = r.procedure;
            first = false;
        }
        if (!first) o << "\n";
        return o.str();
    }

    Mat DP[2];        // int16 H x W disparity, -1 = invalid (h:2724)
    Mat DT;           // ground truth (cpp:2072)
    Mat SE;           // float H x W: refine()'s local SE after its median (cpp:1484-1490), with Do_subpixelEnhancement
    Mat PKR_Err_Mask; // uint8 H x W: calPKR's mask (cpp:1380), with Do_calPKR
    Mat DA_Edge;      // uint8 H x W: discontinuityAdjust's edge map (cpp:6064), with Do_discontinuityAdjust
    Mat LRC_Err_Mask; // uint8 H x W: LRConsistencyCheck's mask, 0 / 255 (cpp:2291-2309), with LRC_CLASSIFY
    Mat I_mask[3];    // nonocc, all, disc (cpp:2073-2075)
    Parameters param_;
    int h_, w_, d_;
    sm_ctx* ctx_ = nullptr;

   private:
    bool refine_on_ = false, csv_open_ = false;
    bool pkr_on_ = false, se_on_ = false, da_on_ = false, lrc_on_ = false, eval_on_ = false;
    std::ostringstream csv_;
    std::vector<std::string> times_;

    // a throwing constructor never runs the destructor: release the context (and its device
    // buffers) here before the exception leaves
    void init_or_release(const Mat& I1_c, const Mat& I2_c, const Mat& I1_g, const Mat& I2_g, int hip_device) {
        try {
            init(I1_c, I2_c, I1_g, I2_g, hip_device);
        } catch (...) {
            sm_destroy(ctx_);
            ctx_ = nullptr;
            throw;
        }
    }
    void init(const Mat& I1_c, const Mat& I2_c, const Mat& I1_g, const Mat& I2_g, int hip_device) {
        const Parameters& param = param_;
        if (I1_c.channels() != 3 || I2_c.channels() != 3 || I1_g.channels() != 1 || I2_g.channels() != 1 ||
            I1_c.depth() != CV_8U || I1_g.depth() != CV_8U)
            throw std::invalid_argument("expected BGR colour and single-channel gray u8 images");
        if (I2_c.rows != h_ || I2_c.cols != w_ || I1_g.rows != h_ || I1_g.cols != w_ || I2_g.rows != h_ ||
            I2_g.cols != w_ || I2_c.step != I1_c.step || I2_g.step != I1_g.step)
            throw std::invalid_argument("images of one size (and row stride per kind) required");
        sm_params p;
        sm_params_default(&p, param.numDisparities - 1, h_, w_);
        p.cost_method = costcalculation == "censusGrad" ? SM_COST_CENSUS_GRAD
                        : costcalculation == "Census"   ? SM_COST_CENSUS
                        : costcalculation == "ADCensus" ? SM_COST_AD_CENSUS
                        : costcalculation == "AD"       ? SM_COST_AD
                        : costcalculation == "SD"       ? SM_COST_SD
                        : costcalculation == "BT"       ? SM_COST_BT
                        : costcalculation == "grad"     ? SM_COST_GRAD
                        : costcalculation == "TruncAD"  ? SM_COST_TRUNC_AD
                        : costcalculation == "adGrad"   ? SM_COST_AD_GRAD
                        : costcalculation == "ADCensusGrad" ? SM_COST_AD_CENSUS_GRAD
                                                        : -1;
        if (p.cost_method < 0) throw std::invalid_argument("unsupported costcalculation: " + costcalculation);
        if (aggregation != "CBCA" && aggregation != "GF" && aggregation != "NL" && aggregation != "FIF" &&
            aggregation != "AWS" && aggregation != "BF" && aggregation != "GFNL" && !aggregation.empty())
            throw std::invalid_argument("unsupported aggregation: " + aggregation);
        if (optimization != "sgm" && optimization != "so" && !optimization.empty())
            throw std::invalid_argument("unsupported optimization: " + optimization);
        p.aggregation = aggregation == "CBCA" ? SM_AGG_CBCA
                        : aggregation == "GF" ? SM_AGG_GF
                        : aggregation == "NL" ? SM_AGG_NL
                        : aggregation == "FIF" ? SM_AGG_FIF
                        : aggregation == "AWS" ? SM_AGG_AWS
                        : aggregation == "BF" ? SM_AGG_BF
                        : aggregation == "GFNL" ? SM_AGG_GFNL
                                              : SM_AGG_NONE;
        p.optimization = optimization == "sgm" ? SM_OPT_SGM : (optimization == "so" ? SM_OPT_SO : SM_OPT_WTA);
        p.census_ring = param.censusFunc == 3;
        p.lam_cen = (float)param.lamCen;
        p.lam_g = (float)param.lamG;
        const int sc = param.disSc > 1 ? param.disSc : 1;   // calArms: L / scale (cpp:5367-5371)
        p.arm_l = param.cbca_crossL[0] / sc;
        p.arm_l_out = param.cbca_crossL_out[0] / sc;
        p.arm_c_thresh = param.cbca_cTresh[0];
        p.arm_c_thresh_out = param.cbca_cTresh_out[0];
        p.arm_min_l = param.cbca_minArmL;
        p.cbca_iterations = param.cbca_iterationNum;
        p.sgm_paths = param.sgm_scanNum;
        p.sgm_cor_dif_thres = param.sgm_corDifThres;
        p.sgm_redu_coeff = param.sgm_reduCoeffi1;
        refine_on_ = Do_refine;
        p.do_refine = Do_refine ? 1 : 0;
        p.lr_max_diff = param.LRmaxDiff;
        p.disp_occ = param.DISP_OCC;
        p.region_vote_nums = param.region_vote_nums;
        p.do_region_vote = Do_regionVote ? 1 : 0;
        p.do_proper_ipol = Do_properIpol ? 1 : 0;
        p.do_last_median_blur = Do_lastMedianBlur ? 1 : 0;
        p.gf_mode = gf_my_guide ? SM_GF_MY_GUIDE : SM_GF_XIMGPROC;
        p.fif_mode = fif_plain ? SM_FIF_PLAIN : SM_FIF_IMPROVE;
        p.lr_consis = Do_LRConsis ? 1 : 0;
        const bool so_on = optimization == "so";
        // refine()'s volume-reading stages after "so" read vm[0] as so left it (the reference's so accumulates in place)
        if (so_on && Do_refine && (Do_calPKR || Do_subpixelEnhancement || Do_discontinuityAdjust)) p.keep_final_volume = 1;
        const bool bf_inexact = aggregation == "BF" && (p.cost_method == SM_COST_GRAD || p.cost_method == SM_COST_AD_GRAD ||
                                                        p.cost_method == SM_COST_AD_CENSUS_GRAD);
        const bool fm = SO_FLOAT_MINIMA >= 0 ? SO_FLOAT_MINIMA != 0
                                             : so_on && (aggregation == "GF" || aggregation == "GFNL" || bf_inexact);
        if (fm) {
            sm_create_opts o;
            sm_create_opts_default(&o);
            o.so_float_minima = 1;
            check(sm_create_ex(&ctx_, &p, &o, hip_device), "sm_create_ex");
        } else {
            check(sm_create(&ctx_, &p, hip_device), "sm_create");
        }
        if (aggregation == "AWS") check(sm_aws_config(ctx_, aws_radius_v, aws_radius_u, aws_gamma_c), "sm_aws_config");
        if (aggregation == "BF") check(sm_bf_config(ctx_, bf_ksize_v, bf_ksize_u), "sm_bf_config");
        if (aggregation == "GFNL") check(sm_gfnl_config(ctx_, gfnl_var_thresh), "sm_gfnl_config");
        if (param.Do_vmTop)
            check(sm_vmtop_config(ctx_, 1, param.vmTop_method, param.vmTop_Num, param.vmTop_thres, param.ts,
                                  param.vmTop_hasCir2 ? 1 : 0, param.vmTop_cir3_doColorLimit ? 1 : 0),
                  "sm_vmtop_config");
        if (param.cbca_double_win && aggregation == "CBCA")   // armLthres = 5 (cpp:4297)
            check(sm_cbca_double_config(ctx_, 1, param.cbca_crossL[1] / sc, param.cbca_crossL_out[1] / sc, param.cbca_cTresh[1],
                                        param.cbca_cTresh_out[1], 5.0f),
                  "sm_cbca_double_config");
        if (!param.cbca_intersect && aggregation == "CBCA") check(sm_cbca_intersect_config(ctx_, 0), "sm_cbca_intersect_config");
        if (Do_refine && (Do_calPKR || Do_bgIpol || Do_subpixelEnhancement)) {
            check(sm_refine_ext_config(ctx_, Do_calPKR ? 1 : 0, pkr_ratio, param.DISP_PKR, Do_bgIpol ? 1 : 0, param.bgIplDepth,
                                       Do_subpixelEnhancement ? 1 : 0, SE_FLOAT ? SM_SE_FLOAT : SM_SE_REFERENCE),
                  "sm_refine_ext_config");
            pkr_on_ = Do_calPKR;
            se_on_ = Do_subpixelEnhancement;
        }
        if (Do_refine && Do_discontinuityAdjust) {
            check(sm_refine_da_config(ctx_, 1, da_canny_low, da_canny_high, da_blur_side, da_blur_centre), "sm_refine_da_config");
            da_on_ = true;
        }
        if (Do_refine && (LRC_CLASSIFY || RV_COMBINE_BG)) {
            check(sm_refine_outlier_config(ctx_, LRC_CLASSIFY ? 1 : 0, param.DISP_MIS, RV_COMBINE_BG ? 1 : 0, param.interpolateType),
                  "sm_refine_outlier_config");
            lrc_on_ = LRC_CLASSIFY;
        }
        if (optimization == "so" && (SO_VARIANT != SM_SO_L2R || SO_PN2 != SM_SO_PN_DEFAULT || SO_PN3 != SM_SO_PN_DEFAULT))
            check(sm_so_config(ctx_, SO_VARIANT, SO_PN2, SO_PN3), "sm_so_config");
        if (Do_stageErrors && !DT.empty()) {
            if (DT.depth() != CV_32F || DT.rows != h_ || DT.cols != w_) throw std::invalid_argument("Do_stageErrors: DT must be CV_32F H x W");
            const float th = (float)param.errorThreshold;
            check(sm_eval_config(ctx_, 1, 0, 1, &th), "sm_eval_config");
            const std::vector<float> dt = DT.packed<float>();
            std::vector<uint8_t> m[3];
            for (int r = 0; r < 3; r++)
                if (!I_mask[r].empty()) m[r] = I_mask[r].packed<uint8_t>();
            check(sm_upload_truth(ctx_, 1, dt.data(), m[0].empty() ? nullptr : m[0].data(), m[1].empty() ? nullptr : m[1].data(),
                                  m[2].empty() ? nullptr : m[2].data()),
                  "sm_upload_truth");
            eval_on_ = true;
        }
        check(sm_set_images(ctx_, I1_c.data, I2_c.data, I1_c.step, I1_g.data, I2_g.data, I1_g.step), "sm_set_images");
    }
    void check(sm_status s, const char* what) {
        if (s != SM_OK)
            throw std::runtime_error(std::string(what) + ": " + (ctx_ ? sm_last_error(ctx_) : sm_status_string(s)));
    }
    friend void SolveAll(StereoMatching** smPyr, int PY_LVL, float REG_LAMBDA);
};

// SolveAll (cpp:2142-2208): PY_LVL = 1 scales vm[0]; PY_LVL in [2, 3] combines the levels
// smPyr[0..PY_LVL-1] of main_.cpp:134-156's pyramid into smPyr[0].
inline void SolveAll(StereoMatching** smPyr, int PY_LVL, float REG_LAMBDA) {
    if (PY_LVL == 1) {
        smPyr[0]->check(sm_solve_all(smPyr[0]->ctx_, PY_LVL, REG_LAMBDA), "SolveAll");
        return;
    }
    std::vector<sm_ctx*> lv;
    for (int i = 0; i < PY_LVL; i++) lv.push_back(smPyr[i]->ctx_);
    smPyr[0]->check(sm_solve_all_pyr(lv.data(), PY_LVL, REG_LAMBDA), "SolveAll");
}

}  // namespace smamd
