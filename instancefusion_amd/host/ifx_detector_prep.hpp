// The host arithmetic of the detector-input stage (ifx_detector_input_size / ifx_detector_resize_taps, include/ifx_c_api.h): the output size of maskrcnn-benchmark's
// Resize and the tap tables of Pillow's 8-bit bilinear resampling.  Header-only, plain C++, no HIP: libifx.so and the stand-alone check (tests/cpp/
// detector_prep_check.cpp) share it.  The same rule is stated in numpy in tests/detector_input_numpy.py and executed by k_detector_input (csrc/ifx_detector.hip).
//
// Size rule (Resize.get_size, maskrcnn_benchmark/data/transforms/transforms.py:35-55; Python semantics, all in f64): size = min_size; with a max_size (> 0), if
// f64(max(w,h)) / f64(min(w,h)) * size > max_size then size = (int)rint(max_size * f64(min(w,h)) / f64(max(w,h))) -- rint rounds half to even, as Python 3's round
// does.  (w <= h and w == size) or (h <= w and h == size): the image keeps its size.  Else w < h: ow = size, oh = (int)(f64(size * h) / w); otherwise oh = size,
// ow = (int)(f64(size * w) / h).  Padded size (to_image_list, structures/image_list.py:54-61): with size_divisible = d > 0, W' = ceil(ow / d) * d, H' = ceil(oh / d) * d.
//
// Taps of one axis (Pillow's precompute_coeffs / normalize_coeffs_8bpc with the bilinear filter, PRECISION_BITS = 22): scale = in / out, fs = max(scale, 1),
// support = fs, ksize = 2 * ceil(support) + 1.  For output index xx: center = (xx + 0.5) * scale, xmin = max((int)(center - support + 0.5), 0),
// n = min((int)(center + support + 0.5), in) - xmin, w_x = tri((x + xmin - center + 0.5) * (1 / fs)) with tri(a) = 1 - |a| for |a| < 1 and 0 otherwise; the weights
// are summed in index order and each is divided by the sum (unless it is 0); k_x = (int)(0.5 + w_x * 2^22) ((int)(-0.5 + ...) for a negative weight, which the
// triangle never gives).  A pass is clip8(((1 << 21) + sum v * k) >> 22) per channel, horizontal first, each skipped when the axis keeps its size.
#ifndef IFX_DETECTOR_PREP_HPP_
#define IFX_DETECTOR_PREP_HPP_
#include <cmath>
#include <cstdint>
#include <vector>

#include "ifx_c_api.h"

namespace ifx_detprep {

enum { PRECISION_BITS = 22, MAX_SCALE = 8, MAX_KSIZE = 2 * MAX_SCALE + 1 };   // a scale above 8 is refused by the device entries: 17 taps at the most

// nullptr when the parameters are acceptable, else what is wrong with them
inline const char* check(const ifx_detector_prep* p)
{
    if (!p) return "NULL parameters";
    if (p->min_size < 1) return "min_size < 1";
    if (p->size_divisible < 0) return "size_divisible < 0";
    if (p->flags & ~(IFX_DET_SWAP_RB | IFX_DET_SCALE_255)) return "unknown flag bits";
    for (int c = 0; c < 3; c++) if (p->std[c] == 0.f) return "a std entry of 0";
    return nullptr;
}

// out4 = ow, oh, W', H'.  nullptr on success.
inline const char* input_size(int w, int h, const ifx_detector_prep* p, int32_t* out4)
{
    const char* bad = check(p);
    if (bad) return bad;
    if (!out4) return "NULL output";
    if (w < 1 || h < 1) return "width or height < 1";
    int64_t size = p->min_size;
    if (p->max_size > 0) {
        const double mn = (double)(w < h ? w : h), mx = (double)(w < h ? h : w);
        if (mx / mn * (double)size > (double)p->max_size) size = (int64_t)std::nearbyint((double)p->max_size * mn / mx);   // (default rounding mode: half to even)
    }
    int64_t ow, oh;
    if ((w <= h && w == size) || (h <= w && h == size)) { ow = w; oh = h; }
    else if (w < h) { ow = size; oh = (int64_t)((double)(size * h) / (double)w); }
    else { oh = size; ow = (int64_t)((double)(size * w) / (double)h); }
    if (ow < 1 || oh < 1) return "the resized image would be empty";
    const int64_t d = p->size_divisible;
    const int64_t Wp = d > 0 ? (ow + d - 1) / d * d : ow, Hp = d > 0 ? (oh + d - 1) / d * d : oh;
    if (Wp > INT32_MAX || Hp > INT32_MAX) return "the output is too large";
    out4[0] = (int32_t)ow; out4[1] = (int32_t)oh; out4[2] = (int32_t)Wp; out4[3] = (int32_t)Hp;
    return nullptr;
}

// ifx_molded_input_size: utils.resize_image (deps/mask_rcnn/utils.py:384-432) with padding, Python semantics in f64.  out8 = nw, nh, S, S, top, left, top + nh,
// left + nw.  nullptr on success.
inline const char* molded_input_size(int w, int h, int min_dim, int max_dim, int32_t* out8)
{
    if (!out8) return "NULL output";
    if (w < 1 || h < 1) return "width or height < 1";
    if (max_dim < 1) return "max_dim < 1";
    const double mn = (double)(w < h ? w : h), mx = (double)(w < h ? h : w);
    double s = 1.0;
    if (min_dim > 0) { s = (double)min_dim / mn; if (s < 1.0) s = 1.0; }                      // scale up but not down
    if (std::nearbyint(mx * s) > (double)max_dim) s = (double)max_dim / mx;                   // (default rounding mode: half to even, as Python 3's round)
    double nh = (double)h, nw = (double)w;
    if (s != 1.0) { nh = std::nearbyint((double)h * s); nw = std::nearbyint((double)w * s); }
    const double S = (double)max_dim;
    if (!(nh >= 1.0 && nh <= S && nw >= 1.0 && nw <= S)) return "the resized image is empty or larger than max_dim";
    if ((double)h / nh > (double)MAX_SCALE || (double)w / nw > (double)MAX_SCALE) return "the output is smaller than an eighth of the frame (resize scale above 8)";
    const int32_t ih = (int32_t)nh, iw = (int32_t)nw, top = (max_dim - ih) / 2, left = (max_dim - iw) / 2;   // (both differences >= 0: floor division)
    out8[0] = iw; out8[1] = ih; out8[2] = max_dim; out8[3] = max_dim; out8[4] = top; out8[5] = left; out8[6] = top + ih; out8[7] = left + iw;
    return nullptr;
}

// ifx_pyramid_level_thresholds: PyramidROIAlign's level rule (deps/mask_rcnn/model.py:351-357) as three thresholds on s = sqrt(h * w) of a normalised box.
// The reference takes k = round(log2(s / c)), c = 224 / sqrt(image_h * image_w), half to even, and level = min(5, max(2, 4 + k)); so level >= 3 iff log2(s / c) >
// -1.5 (-1.5 rounds to -2), level >= 4 iff log2(s / c) >= -0.5 (-0.5 rounds to -0) and level == 5 iff log2(s / c) > 0.5 (0.5 rounds to 0):
// level = 2 + (s > T0) + (s >= T1) + (s > T2) with T0 = c 2^-1.5, T1 = c 2^-0.5, T2 = c 2^0.5, in f64 (sqrt is correctly rounded, the powers of two below are
// sqrt(2) / 4, sqrt(2) / 2 and sqrt(2)) and rounded ONCE to f32.  nullptr on success.
inline const char* pyramid_level_thresholds(int image_h, int image_w, float* out3)
{
    if (!out3) return "NULL output";
    if (image_h < 1 || image_w < 1) return "image_h or image_w < 1";
    const double c = 224.0 / std::sqrt((double)image_h * (double)image_w), r2 = std::sqrt(2.0);
    out3[0] = (float)(c * (r2 / 4.0));
    out3[1] = (float)(c * (r2 / 2.0));
    out3[2] = (float)(c * r2);
    return nullptr;
}

inline int resize_ksize(int in_size, int out_size)
{
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    return (int)std::ceil(fs) * 2 + 1;
}

// first[out], count[out], coeff[out][ksize] (row-major, zero behind count).  Returns ksize, or -1 for sizes < 1 or ksize > max_ksize (nothing is written then).
inline int resize_taps(int in_size, int out_size, int32_t* first, int32_t* count, int32_t* coeff, int max_ksize)
{
    if (in_size < 1 || out_size < 1) return -1;
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = fs, ss = 1.0 / fs;
    const double kd = std::ceil(support) * 2 + 1;
    if (kd > (double)max_ksize) return -1;
    const int ksize = (int)kd;
    std::vector<double> w((size_t)ksize);
    for (int xx = 0; xx < out_size; xx++) {
        const double center = ((double)xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        const int n = xmax - xmin;
        double ww = 0.0;
        for (int x = 0; x < n; x++) {
            double a = ((double)(x + xmin) - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            w[x] = a < 1.0 ? 1.0 - a : 0.0;
            ww += w[x];
        }
        int32_t* k = coeff + (size_t)xx * ksize;
        for (int x = 0; x < ksize; x++) {
            if (x >= n) { k[x] = 0; continue; }
            const double v = (ww != 0.0 ? w[x] / ww : w[x]) * (double)(1 << PRECISION_BITS);
            k[x] = v < 0.0 ? (int32_t)(-0.5 + v) : (int32_t)(0.5 + v);
        }
        first[xx] = xmin; count[xx] = n;
    }
    return ksize;
}

}   // namespace ifx_detprep
#endif
