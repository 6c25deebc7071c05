// A minimal cv::Mat for oracle/ref_core.mk -- TEST INFRASTRUCTURE ONLY.  Written from OpenCV's documented
// interface, for the handful of calls the reference's cost / CBCA / SGM / scan-line functions make; no
// OpenCV text.  What differs from OpenCV on purpose:
//   - a new buffer is filled with cv::shim_fill (a byte the driver is given): Mat::create does not zero
//     memory, and the tests run every case with two fill bytes to see what the reference leaves unwritten;
//   - every buffer is its own heap block of exactly the Mat's size, so a sanitizer build sees an access
//     past a Mat's end;
//   - ptr<T>() computes the address in integers: the reference forms (and never follows) pointers into
//     empty Mats, which is defined in integers and not in pointer arithmetic.
#ifndef SM_REF_SHIM_OPENCV_MIN_H
#define SM_REF_SHIM_OPENCV_MIN_H

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

typedef unsigned char uchar;
typedef unsigned short ushort;

#define CV_CN_SHIFT 3
#define CV_8U 0
#define CV_8S 1
#define CV_16U 2
#define CV_16S 3
#define CV_32S 4
#define CV_32F 5
#define CV_64F 6
#define CV_MAT_DEPTH(t) ((t) & ((1 << CV_CN_SHIFT) - 1))
#define CV_MAT_CN(t) ((((t) >> CV_CN_SHIFT) & 511) + 1)
#define CV_MAKETYPE(depth, cn) (CV_MAT_DEPTH(depth) + (((cn) - 1) << CV_CN_SHIFT))
#define CV_8UC1 CV_MAKETYPE(CV_8U, 1)
#define CV_8UC3 CV_MAKETYPE(CV_8U, 3)
#define CV_8UC(n) CV_MAKETYPE(CV_8U, (n))
#define CV_16UC(n) CV_MAKETYPE(CV_16U, (n))
#define CV_16SC(n) CV_MAKETYPE(CV_16S, (n))
#define CV_32SC(n) CV_MAKETYPE(CV_32S, (n))
#define CV_32FC1 CV_MAKETYPE(CV_32F, 1)
#define CV_32FC2 CV_MAKETYPE(CV_32F, 2)
#define CV_32FC(n) CV_MAKETYPE(CV_32F, (n))
#define CV_64FC(n) CV_MAKETYPE(CV_64F, (n))

#define CV_Assert(expr)                                                                      \
    do {                                                                                     \
        if (!(expr)) {                                                                       \
            std::fprintf(stderr, "CV_Assert failed: %s (%s:%d)\n", #expr, __FILE__, __LINE__); \
            std::abort();                                                                    \
        }                                                                                    \
    } while (0)

#define popcnt32 __builtin_popcount
#define popcnt64 __builtin_popcountll

namespace cv {

extern int shim_fill;   // the byte every new buffer is filled with (defined by the driver)

enum { BORDER_CONSTANT = 0, BORDER_REPLICATE = 1, BORDER_REFLECT = 2, BORDER_WRAP = 3, BORDER_REFLECT_101 = 4,
       BORDER_DEFAULT = 4 };

struct Scalar {
    double val[4];
    Scalar() : val{0, 0, 0, 0} {}
    Scalar(double v0, double v1 = 0, double v2 = 0, double v3 = 0) : val{v0, v1, v2, v3} {}
    static Scalar all(double v) { return Scalar(v, v, v, v); }
    double operator[](int i) const { return val[i]; }
};

struct Size {
    int width, height;
    Size() : width(0), height(0) {}
    Size(int w, int h) : width(w), height(h) {}
};

class Mat {
public:
    enum { MAX_DIM = 4 };
    struct MatSize {
        int p[MAX_DIM];
        int& operator[](int i) { return p[i]; }
        const int& operator[](int i) const { return p[i]; }
    };
    struct MatStep {
        size_t p[MAX_DIM];
        size_t& operator[](int i) { return p[i]; }
        const size_t& operator[](int i) const { return p[i]; }
    };

    int flags, dims, rows, cols;
    uchar* data;
    MatSize size;
    MatStep step;

    Mat() { reset(); }
    Mat(int r, int c, int type) { reset(); create(r, c, type); }
    Mat(int r, int c, int type, const Scalar& s) { reset(); create(r, c, type); *this = s; }
    Mat(int ndims, const int* sizes, int type) { reset(); create(ndims, sizes, type); }
    Mat(int ndims, const int* sizes, int type, const Scalar& s) { reset(); create(ndims, sizes, type); *this = s; }

    int type() const { return flags; }
    int depth() const { return CV_MAT_DEPTH(flags); }
    int channels() const { return CV_MAT_CN(flags); }
    size_t elemSize1() const {
        static const size_t sz[7] = {1, 1, 2, 2, 4, 4, 8};
        return sz[depth()];
    }
    size_t elemSize() const { return elemSize1() * (size_t)channels(); }
    bool empty() const { return data == nullptr || total() == 0; }
    size_t total() const {
        if (dims == 0) return 0;
        size_t n = 1;
        for (int i = 0; i < dims; i++) n *= (size_t)size.p[i];
        return n;
    }
    size_t bytes() const { return total() * elemSize(); }

    // As OpenCV: nothing happens when the Mat already has this shape and type.
    void create(int r, int c, int type) {
        const int sz[2] = {r, c};
        create(2, sz, type);
    }
    void create(int ndims, const int* sizes, int type) {
        CV_Assert(ndims >= 1 && ndims <= MAX_DIM);
        if (data && dims == ndims && flags == type) {
            bool same = true;
            for (int i = 0; i < ndims; i++) same = same && size.p[i] == sizes[i];
            if (same) return;
        }
        reset();
        flags = type;
        dims = ndims;
        for (int i = 0; i < ndims; i++) {
            CV_Assert(sizes[i] >= 0);
            size.p[i] = sizes[i];
        }
        size_t st = elemSize();
        for (int i = ndims - 1; i >= 0; i--) {
            step.p[i] = st;
            st *= (size_t)sizes[i];
        }
        if (ndims == 2) {
            rows = sizes[0];
            cols = sizes[1];
        } else {
            rows = cols = -1;
        }
        const size_t n = bytes();
        if (n) {
            buf_.reset(new uchar[n], std::default_delete<uchar[]>());
            data = buf_.get();
            std::memset(data, shim_fill, n);
        }
    }

    Mat& operator=(const Scalar& s) {   // setTo: every element's channel c becomes s[c] (channels beyond 4: s[0..3] of a 1-channel view)
        const int cn = channels();
        const size_t n = total();
        for (size_t i = 0; i < n; i++)
            for (int c = 0; c < cn; c++) store(i * (size_t)cn + (size_t)c, s.val[c < 4 ? c : 0]);
        return *this;
    }

    Mat clone() const {
        Mat m;
        copyTo(m);
        return m;
    }
    void copyTo(Mat& dst) const {
        if (dims == 0) {
            dst.reset();
            return;
        }
        dst.create(dims, size.p, flags);
        if (bytes()) std::memcpy(dst.data, data, bytes());
    }
    static Mat ones(int r, int c, int type) { return Mat(r, c, type, Scalar(1)); }
    static Mat zeros(int r, int c, int type) { return Mat(r, c, type, Scalar(0)); }

    template <typename T> T* ptr(int i0 = 0) { return (T*)at_(i0, 0, 0); }
    template <typename T> T* ptr(int i0, int i1) { return (T*)at_(i0, i1, 0); }
    template <typename T> T* ptr(int i0, int i1, int i2) { return (T*)at_(i0, i1, i2); }
    template <typename T> const T* ptr(int i0 = 0) const { return (const T*)at_(i0, 0, 0); }
    template <typename T> const T* ptr(int i0, int i1) const { return (const T*)at_(i0, i1, 0); }
    template <typename T> const T* ptr(int i0, int i1, int i2) const { return (const T*)at_(i0, i1, i2); }

private:
    std::shared_ptr<uchar> buf_;

    void reset() {
        flags = 0;
        dims = 0;
        rows = cols = 0;
        data = nullptr;
        for (int i = 0; i < MAX_DIM; i++) {
            size.p[i] = 0;
            step.p[i] = 0;
        }
        buf_.reset();
    }
    void* at_(int i0, int i1, int i2) const {
        const intptr_t a = (intptr_t)data + (intptr_t)i0 * (intptr_t)step.p[0] + (intptr_t)i1 * (intptr_t)step.p[1] +
                           (intptr_t)i2 * (intptr_t)step.p[2];
        return (void*)a;
    }
    void store(size_t i, double v) {
        switch (depth()) {
            case CV_8U: ((uchar*)data)[i] = (uchar)v; break;
            case CV_8S: ((signed char*)data)[i] = (signed char)v; break;
            case CV_16U: ((ushort*)data)[i] = (ushort)v; break;
            case CV_16S: ((short*)data)[i] = (short)v; break;
            case CV_32S: ((int*)data)[i] = (int)v; break;
            case CV_32F: ((float*)data)[i] = (float)v; break;
            default: ((double*)data)[i] = v; break;
        }
    }
};

template <typename T> struct shim_depth;
template <> struct shim_depth<float> { enum { value = CV_32F }; };
template <> struct shim_depth<int> { enum { value = CV_32S }; };
template <> struct shim_depth<uchar> { enum { value = CV_8U }; };
template <> struct shim_depth<short> { enum { value = CV_16S }; };

template <typename T> class Mat_ : public Mat {
public:
    Mat_() : Mat() {}
    Mat_(int r, int c) : Mat(r, c, shim_depth<T>::value) {}
    void create(int r, int c) { Mat::create(r, c, shim_depth<T>::value); }
    void create(int ndims, const int* sizes) { Mat::create(ndims, sizes, shim_depth<T>::value); }
};
typedef Mat_<float> Mat1f;
typedef Mat_<int> Mat1i;
typedef Mat_<uchar> Mat1b;

// OpenCV's borderInterpolate for BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba).
inline int shim_reflect101(int p, int len) {
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do {
        if (p < 0) p = -p;
        else p = 2 * len - p - 2;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

inline void copyMakeBorder(const Mat& src, Mat& dst, int top, int bottom, int left, int right, int borderType) {
    CV_Assert(src.dims == 2 && borderType == BORDER_REFLECT_101);
    Mat out(src.rows + top + bottom, src.cols + left + right, src.type());
    const size_t es = src.elemSize();
    for (int v = 0; v < out.rows; v++) {
        const int sv = shim_reflect101(v - top, src.rows);
        for (int u = 0; u < out.cols; u++) {
            const int su = shim_reflect101(u - left, src.cols);
            std::memcpy(out.data + (size_t)v * out.step.p[0] + (size_t)u * es,
                        src.data + (size_t)sv * src.step.p[0] + (size_t)su * es, es);
        }
    }
    dst = out;
}

// Unreachable with the default Parameters (doGF_bef_calArm = false): reaching it ends the program.
namespace ximgproc {
inline void guidedFilter(const Mat&, const Mat&, Mat&, int, double) {
    std::fprintf(stderr, "ref_core: ximgproc::guidedFilter is not built\n");
    std::abort();
}
}  // namespace ximgproc

}  // namespace cv

#endif
