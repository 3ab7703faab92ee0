// ifx_detector.hip -- the detector's side of the library, in six sections:
//   1. the detector's input tensor, made on the device from the frame that is already there (ifx_detector_input[_image]; described below; the Keras model's
//      form of it, ifx_detector_input_molded[_image], is the same kernel with another tail)
//   2. ROIAlign forward and box NMS (ifx_roi_align_forward, ifx_nms)
//   3. the RPN's proposal stage of one level and the box decoding it contains (ifx_rpn_proposals, ifx_box_decode)
//   4. the box head's post-processing (ifx_box_detections)
//   5. the mask head's logits to ROI masks, resized boxes and class ids (ifx_mask_head_select; as a stage of ifx_process_segmentation_detections, ifx_instance.hip)
//   6. the default (Keras) detector's detections and masks to image-sized masks, boxes and class ids (ifx_unmold_detections; as a stage of
//      ifx_process_segmentation_unmolded, ifx_instance.hip)
// Sections 2 to 6 run on the caller's stream and touch no frame or map state; the three calls with an NMS in them share one block scan (block_excl_scan), one
// walk state (NmsWalk), one device-count mask kernel (k_nms_mask_dev) and the handle's one scratch buffer, carved by one Carver (ops_scratch).
//
//   ifx_detector_input[_image]  <-  COCODemo.build_transform       deps/maskrcnn-benchmark-master/demo/predictor.py:132-160
//                                   Resize.get_size / Normalize    maskrcnn_benchmark/data/transforms/transforms.py:35-55, 86-90
//                                   to_image_list                  maskrcnn_benchmark/structures/image_list.py:29-66
//
// The reference resizes the frame with Pillow on the CPU (8-bit bilinear resampling: two separable passes with 22-bit integer taps and a uint8 intermediate),
// converts to float, scales / flips / normalises, zero-pads to a multiple of SIZE_DIVISIBILITY and uploads 3 * H' * W' floats.  Here one launch reads the u8 frame
// where it lies and writes the same floats.  The rule in full: include/ifx_c_api.h and ../host/ifx_detector_prep.hpp, whose host arithmetic makes the tap tables
// this kernel reads; tests/detector_input_numpy.py states it in numpy.
#include "ifx_ctx.h"
#include "ifx_dev.h"
#include "../host/ifx_detector_prep.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int DI_TX = 64, DI_TY = 16;                 // the tile of the PADDED output a 256-thread block owns, all three channels
constexpr int DI_K = ifx_detprep::MAX_KSIZE;          // 17 taps at the scale cap of 8
constexpr int DI_ROWS = DI_TY * ifx_detprep::MAX_SCALE + DI_K;   // source rows under a tile at the cap: 145
constexpr int DI_HALF = 1 << (ifx_detprep::PRECISION_BITS - 1);

struct DetArgs {                                      // by value: every word arrives in SGPRs, nothing uniform is loaded per lane
    const uint8_t* src;                               // [h][w][3]
    float* out;                                       // [3][Hp][Wp]
    const int32_t *fx, *cx, *kx, *fy, *cy, *ky;       // first / count / coeff[.][ksx|ksy] of the two axes (an axis that keeps its size: the identity, ks = 1)
    int w, h, ow, oh, Wp, Hp, ksx, ksy, flags;
    float mean[3], stdv[3];
    int left, top, tx0, ty0, nhwc;                    // MOLD only: the window's corner in the S x S output (Wp = Hp = S), the tiles in front of it, the layout
    double meand[3];                                  // MOLD only: MEAN_PIXEL
};

// Phase 1: the source rows under the tile, first[y0] .. first[y1] + count[y1], resampled horizontally for the tile's 64 columns into LDS as bytes (copied when the
// width is kept); the tap records of the tile's columns and rows are staged first.  Phase 2: the vertical sum out of LDS, the float tail, three planar stores.
// LDS layout of the staged rows: [row][channel][64 columns] bytes.  A wave's 64 lanes sit on 64 consecutive columns, so a byte read or write of one (row, channel)
// touches 16 consecutive dwords -- 16 different banks, four lanes on each dword -- in phase 1 as in phase 2; the pixel-interleaved [row][64][3] would spread a wave
// over 48 dwords with three reads per lane landing in the same ones.  The tap coefficients are staged [column][17]: the odd stride keeps 32 lanes on 32 banks.
// Sums: every weight of the triangle filter is >= 0 and the 22-bit taps of an output sample add up to 2^22 give or take half a unit per tap, so
// 2^21 + sum v * k <= 2^21 + 255 * (2^22 + 9) < 2^31: 32-bit unsigned accumulators are exact (17 x 255 x 2^22 as a bound would not fit).
// VEC: a lane owns four consecutive x of one row and stores 16 bytes per channel (W' a multiple of 4 and an aligned pointer: chosen by the host as for
// k_mask_area's 16-B words); otherwise consecutive lanes sit on consecutive x and store 4 bytes each.
// MOLD (ifx_detector_input_molded[_image]; mold_inputs, deps/mask_rcnn/model.py:2247-2283): the same two phases on tiles of the RESIZED image that start tx0, ty0
// in front of it (multiples of the tile, so that no tile straddles the window's corner), another tail: the byte minus an f64 mean, rounded once, stored at
// (top + y, left + x) of the S x S output, f32(-mean) everywhere else, channels last or planar; consecutive lanes on consecutive x, never VEC.
template <bool VEC, bool MOLD = false>
__global__ void __launch_bounds__(256) k_detector_input(const DetArgs a)
{
    __shared__ int s_kx[DI_TX * DI_K], s_ky[DI_TY * DI_K];
    __shared__ int s_fx[DI_TX], s_cx[DI_TX], s_fy[DI_TY], s_cy[DI_TY];
    __shared__ uint8_t s_rows[DI_ROWS * 3 * DI_TX];
    const int t = threadIdx.x, x0 = blockIdx.x * DI_TX - (MOLD ? a.tx0 : 0), y0 = blockIdx.y * DI_TY - (MOLD ? a.ty0 : 0);
    const int nx = min(DI_TX, a.ow - x0), ny = min(DI_TY, a.oh - y0);   // the tile's share of the resized image (<= 0: wholly in the padding)
    const bool image = nx > 0 && ny > 0 && (!MOLD || (x0 >= 0 && y0 >= 0));
    int r0 = 0;
    if (image) {
        for (int i = t; i < nx * a.ksx; i += 256) { const int col = i / a.ksx, k = i - col * a.ksx; s_kx[col * DI_K + k] = a.kx[(size_t)(x0 + col) * a.ksx + k]; }
        for (int i = t; i < ny * a.ksy; i += 256) { const int row = i / a.ksy, k = i - row * a.ksy; s_ky[row * DI_K + k] = a.ky[(size_t)(y0 + row) * a.ksy + k]; }
        if (t < nx) { s_fx[t] = a.fx[x0 + t]; s_cx[t] = min(a.cx[x0 + t], a.ksx); }
        if (t >= 64 && t - 64 < ny) { s_fy[t - 64] = a.fy[y0 + t - 64]; s_cy[t - 64] = min(a.cy[y0 + t - 64], a.ksy); }
        __syncthreads();
        r0 = s_fy[0];
        const int nrows = min(s_fy[ny - 1] + s_cy[ny - 1] - r0, DI_ROWS);
        const int col = t & 63;
        if (col < nx) {
            const int f = s_fx[col], n = s_cx[col];
            const bool copy = a.ow == a.w;
            for (int r = t >> 6; r < nrows; r += 4) {
                const uint8_t* p = a.src + ((size_t)(r0 + r) * a.w + f) * 3;
                uint32_t b0, b1, b2;
                if (copy) { b0 = p[0]; b1 = p[1]; b2 = p[2]; }
                else {
                    uint32_t q0 = DI_HALF, q1 = DI_HALF, q2 = DI_HALF;
                    for (int k = 0; k < n; k++) {
                        const uint32_t kk = (uint32_t)s_kx[col * DI_K + k];
                        q0 += p[3 * k] * kk; q1 += p[3 * k + 1] * kk; q2 += p[3 * k + 2] * kk;
                    }
                    b0 = min(q0 >> ifx_detprep::PRECISION_BITS, 255u); b1 = min(q1 >> ifx_detprep::PRECISION_BITS, 255u); b2 = min(q2 >> ifx_detprep::PRECISION_BITS, 255u);
                }
                s_rows[(r * 3 + 0) * DI_TX + col] = (uint8_t)b0;
                s_rows[(r * 3 + 1) * DI_TX + col] = (uint8_t)b1;
                s_rows[(r * 3 + 2) * DI_TX + col] = (uint8_t)b2;
            }
        }
        __syncthreads();
    }
    if constexpr (MOLD) {
        const int xl = t & 63, ox = x0 + xl + a.left;
        if (ox < 0 || ox >= a.Wp) return;
        const size_t plane = (size_t)a.Hp * a.Wp;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int yl = (t >> 6) + 4 * i, oy = y0 + yl + a.top;
            if (oy < 0 || oy >= a.Hp) continue;
            double b[3] = {0.0, 0.0, 0.0};            // the padding: byte 0 before the mean is subtracted
            if (image && xl < nx && yl < ny) {
                const int fy = s_fy[yl] - r0, n = s_cy[yl];
                uint32_t q[3] = {DI_HALF, DI_HALF, DI_HALF};
                for (int k = 0; k < n; k++) {
                    const uint32_t kk = (uint32_t)s_ky[yl * DI_K + k];
                    const int row = min(fy + k, DI_ROWS - 1);
#pragma unroll
                    for (int c = 0; c < 3; c++) q[c] += s_rows[(row * 3 + c) * DI_TX + xl] * kk;
                }
#pragma unroll
                for (int c = 0; c < 3; c++) b[c] = (double)min(q[c] >> ifx_detprep::PRECISION_BITS, 255u);
            }
            const size_t px = (size_t)oy * a.Wp + ox;
#pragma unroll
            for (int c = 0; c < 3; c++) a.out[a.nhwc ? px * 3 + c : c * plane + px] = (float)(b[c] - a.meand[c]);
        }
        return;
    }
    const bool swap = a.flags & IFX_DET_SWAP_RB, s255 = a.flags & IFX_DET_SCALE_255;
    float v[3][4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int xl = VEC ? 4 * (t & 15) + i : (t & 63), yl = VEC ? (t >> 4) : (t >> 6) + 4 * i;
        v[0][i] = v[1][i] = v[2][i] = 0.f;   // the padding: literal zeros
        if (image && xl < nx && yl < ny) {
            const int fy = s_fy[yl] - r0, n = s_cy[yl];
            uint32_t q[3] = {DI_HALF, DI_HALF, DI_HALF};
            for (int k = 0; k < n; k++) {
                const uint32_t kk = (uint32_t)s_ky[yl * DI_K + k];
                const int row = min(fy + k, DI_ROWS - 1);
#pragma unroll
                for (int c = 0; c < 3; c++) q[c] += s_rows[(row * 3 + c) * DI_TX + xl] * kk;
            }
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const uint32_t b = min((swap ? q[2 - c] : q[c]) >> ifx_detprep::PRECISION_BITS, 255u);
                float tt = (float)b / 255.f;          // ToTensor: a true division (the reciprocal differs for 126 of the 256 bytes)
                if (s255) tt = tt * 255.f;
                v[c][i] = (tt - a.mean[c]) / a.stdv[c];   // Normalize: sub_ then div_, behind the channel flip
            }
        }
    }
    const size_t plane = (size_t)a.Hp * a.Wp;
    if (VEC) {
        const int x = x0 + 4 * (t & 15), y = y0 + (t >> 4);
        if (x < a.Wp && y < a.Hp) {
#pragma unroll
            for (int c = 0; c < 3; c++) *(float4*)(a.out + c * plane + (size_t)y * a.Wp + x) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        }
    } else {
        const int x = x0 + (t & 63);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int y = y0 + (t >> 6) + 4 * i;
            if (x < a.Wp && y < a.Hp) {
#pragma unroll
                for (int c = 0; c < 3; c++) a.out[c * plane + (size_t)y * a.Wp + x] = v[c][i];
            }
        }
    }
}

// the tap tables of one (w, h, ow, oh): the host copy (pinned, kept alive: the upload is asynchronous) and the device copy
struct DetTable {
    int w = 0, h = 0, ow = 0, oh = 0, ksx = 0, ksy = 0;
    size_t ints = 0, off_y = 0;
    int32_t *host = nullptr, *dev = nullptr;
    unsigned long long used = 0;
};
constexpr size_t DET_TABLES = 8;   // "a handful": min_size and the frame size rarely change; one more evicts the table used longest ago (hipFree waits for its readers)
struct DetPrep {
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    std::vector<DetTable> tabs;
    unsigned long long clock = 0;
};

// one axis into first / count / coeff at t; an axis that keeps its size gets the identity (the pass is skipped: its taps would be (2^22, 0), the same bytes)
int axis_table(int in, int out, int32_t* first, int32_t* count, int32_t* coeff)
{
    if (in != out) return ifx_detprep::resize_taps(in, out, first, count, coeff, DI_K);
    for (int i = 0; i < out; i++) { first[i] = i; count[i] = 1; coeff[i] = 1 << ifx_detprep::PRECISION_BITS; }
    return 1;
}

int det_table(ifx* h, DetPrep* dp, int w, int hh, int ow, int oh, DetTable** out)
{
    for (DetTable& t : dp->tabs)
        if (t.w == w && t.h == hh && t.ow == ow && t.oh == oh) { t.used = ++dp->clock; *out = &t; return IFX_OK; }
    DetTable t;
    t.w = w; t.h = hh; t.ow = ow; t.oh = oh;
    t.ksx = ow == w ? 1 : ifx_detprep::resize_ksize(w, ow);
    t.ksy = oh == hh ? 1 : ifx_detprep::resize_ksize(hh, oh);
    if (t.ksx > DI_K || t.ksy > DI_K) { h->err = "detector input: more than 17 taps"; return IFX_E_INVALID; }
    t.off_y = (size_t)ow * (2 + t.ksx);
    t.ints = t.off_y + (size_t)oh * (2 + t.ksy);
    HIPCHK(h, hipHostMalloc((void**)&t.host, t.ints * 4, hipHostMallocDefault));
    int32_t *fx = t.host, *cx = fx + ow, *kx = cx + ow, *fy = t.host + t.off_y, *cy = fy + oh, *ky = cy + oh;
    bool ok = axis_table(w, ow, fx, cx, kx) == t.ksx && axis_table(hh, oh, fy, cy, ky) == t.ksy;
    for (int y = 0; ok && y < oh; y += DI_TY) {   // what the kernel's LDS holds of a tile: cannot fail at a scale <= 8, checked all the same
        const int y1 = std::min(y + DI_TY, oh) - 1;
        ok = fy[y1] + cy[y1] - fy[y] <= DI_ROWS;
    }
    if (!ok) { hipHostFree(t.host); h->err = "detector input: tap tables out of the kernel's bounds"; return IFX_E_INVALID; }
    if (hipMalloc((void**)&t.dev, t.ints * 4) != hipSuccess) { hipHostFree(t.host); h->err = "detector input: hipMalloc of the tap tables failed"; return IFX_E_HIP; }
    if (dp->tabs.size() >= DET_TABLES) {
        size_t old = 0;
        for (size_t i = 1; i < dp->tabs.size(); i++) if (dp->tabs[i].used < dp->tabs[old].used) old = i;
        hipFree(dp->tabs[old].dev); hipHostFree(dp->tabs[old].host);
        dp->tabs.erase(dp->tabs.begin() + (long)old);
    }
    t.used = ++dp->clock;
    dp->tabs.push_back(t);
    DetTable& n = dp->tabs.back();
    HIPCHK(h, hipMemcpyAsync(n.dev, n.host, n.ints * 4, hipMemcpyHostToDevice, h->cur));
    *out = &n;
    return IFX_OK;
}

// the argument checks every device entry shares; out4: ow, oh, W', H'
int det_check(ifx* h, const char* who, int w, int hh, const ifx_detector_prep* p, const float* d_out, int64_t out_floats, int32_t* out4)
{
    if (!p || !d_out) { h->err = std::string(who) + ": NULL pointer"; return IFX_E_INVALID; }
    const char* bad = ifx_detprep::input_size(w, hh, p, out4);
    if (bad) { h->err = std::string(who) + ": " + bad; return IFX_E_INVALID; }
    if ((double)w / out4[0] > (double)ifx_detprep::MAX_SCALE || (double)hh / out4[1] > (double)ifx_detprep::MAX_SCALE) {
        h->err = std::string(who) + ": the output is smaller than an eighth of the frame (resize scale above 8)"; return IFX_E_INVALID;
    }
    if (out_floats < (int64_t)3 * out4[2] * out4[3]) { h->err = std::string(who) + ": out_floats < 3 * H' * W'"; return IFX_E_INVALID; }
    return IFX_OK;
}

// everything behind the checks.  ev_src: what the source image waits for (a ticket's snapshot), slot: the frame slot whose next copy-in is held off behind the read
struct MoldSpec { int left, top, nhwc; double mean[3]; };   // the molded form (p is NULL then): sz = nw, nh, S, S
int det_run(ifx* h, const uint8_t* d_rgb, int w, int hh, const ifx_detector_prep* p, const int32_t* sz, float* d_out, void* stream, hipEvent_t ev_src, FrameSlot* slot,
            const MoldSpec* mold = nullptr)
{
    if (!h->det_prep) h->det_prep = new DetPrep();
    DetPrep* dp = (DetPrep*)h->det_prep;
    if (!dp->ev_in) HIPCHK(h, hipEventCreateWithFlags(&dp->ev_in, hipEventDisableTiming));
    if (!dp->ev_out) HIPCHK(h, hipEventCreateWithFlags(&dp->ev_out, hipEventDisableTiming));
    DetTable* t = nullptr;
    int r = det_table(h, dp, w, hh, sz[0], sz[1], &t);
    if (r) return r;
    hipStream_t consumer = (hipStream_t)stream;
    const bool cross = consumer != h->cur;
    if (cross) {   // an earlier forward pass on the consumer's stream may still be reading d_out
        HIPCHK(h, hipEventRecord(dp->ev_in, consumer));
        HIPCHK(h, hipStreamWaitEvent(h->cur, dp->ev_in, 0));
    }
    if (ev_src) HIPCHK(h, hipStreamWaitEvent(h->cur, ev_src, 0));
    DetArgs a;
    a.src = d_rgb; a.out = d_out;
    a.fx = t->dev; a.cx = a.fx + sz[0]; a.kx = a.cx + sz[0];
    a.fy = t->dev + t->off_y; a.cy = a.fy + sz[1]; a.ky = a.cy + sz[1];
    a.w = w; a.h = hh; a.ow = sz[0]; a.oh = sz[1]; a.Wp = sz[2]; a.Hp = sz[3]; a.ksx = t->ksx; a.ksy = t->ksy; a.flags = p ? p->flags : 0;
    for (int c = 0; c < 3; c++) { a.mean[c] = p ? p->mean[c] : 0.f; a.stdv[c] = p ? p->std[c] : 1.f; a.meand[c] = mold ? mold->mean[c] : 0.0; }
    a.left = mold ? mold->left : 0; a.top = mold ? mold->top : 0; a.nhwc = mold ? mold->nhwc : 0;
    a.tx0 = cdiv(a.left, DI_TX) * DI_TX; a.ty0 = cdiv(a.top, DI_TY) * DI_TY;
    if (mold) {   // tiles of the resized image's grid from (-tx0, -ty0) to the output's far edges at (S - left, S - top)
        const dim3 grid((unsigned)cdiv(a.Wp - a.left + a.tx0, DI_TX), (unsigned)cdiv(a.Hp - a.top + a.ty0, DI_TY));
        LAUNCH(h, "detector_input_molded", grid, dim3(256), (k_detector_input<false, true>), a);
    } else {
        const dim3 grid((unsigned)cdiv(a.Wp, DI_TX), (unsigned)cdiv(a.Hp, DI_TY));
        if (a.Wp % 4 == 0 && (uintptr_t)d_out % 16 == 0) LAUNCH(h, "detector_input", grid, dim3(256), k_detector_input<true>, a);
        else LAUNCH(h, "detector_input", grid, dim3(256), k_detector_input<false>, a);
    }
    if (slot) {   // the side stream reuses the slot two frames on and waits only for the FRAME that used it: it is told about this reader as about a snapshot's copy
        if (!slot->snap_read) HIPCHK(h, hipEventCreateWithFlags(&slot->snap_read, hipEventDisableTiming));
        HIPCHK(h, hipEventRecord(slot->snap_read, h->cur));
        slot->snap_pending = 1;
    }
    if (cross) {
        HIPCHK(h, hipEventRecord(dp->ev_out, h->cur));
        HIPCHK(h, hipStreamWaitEvent(consumer, dp->ev_out, 0));
    }
    return IFX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------------------
// The detector's two operators of its own: ifx_roi_align_forward and ifx_nms (maskrcnn_benchmark._C.roi_align_forward / _C.nms; the rules in full: include/ifx_c_api.h,
// in numpy: tests/detector_ops_numpy.py).  They read and write the caller's buffers on the caller's stream and touch no frame or map state.

constexpr int RA_CH = 64;      // the run of channels a 256-thread block walks for its ROI
constexpr int RA_TAB = 512;    // axis samples (pooled * grid) an axis table holds in LDS; a longer axis (an adaptive grid on a huge ROI) is computed per use by the same function

// One sample position of one axis: the two texels and their weights (l: of hi, h: of lo); lo < 0: outside, the sample contributes +0.
struct RaSample { int lo, hi; float l, h; };

// bilinear_interpolate of ROIAlign_cuda.cu:16-62 / pre_calc_for_bilinear_interpolate of ROIAlign_cpu.cpp, one axis.  The position and the weights of a sample
// separate into a y part of (ph, iy) and an x part of (pw, ix): w1 = hy * hx and so on are formed from them where they are used, in the CPU file's order.
__device__ __forceinline__ RaSample ra_axis(float start, float bin, int p, int i, int grid, int size)
{
    float y = (start + (float)p * bin) + (((float)i + 0.5f) * bin) / (float)grid;
    RaSample s;
    if (y < -1.0f || y > (float)size) { s.lo = -1; s.hi = 0; s.l = 0.f; s.h = 0.f; return s; }
    if (y <= 0.f) y = 0.f;
    int lo = y == y ? (int)y : 0;      // y in [0, size] here (NaN: 0, as the conversion instruction gives)
    int hi;
    if (lo >= size - 1) { hi = lo = size - 1; y = (float)lo; }
    else hi = lo + 1;
    s.lo = lo; s.hi = hi;
    s.l = y - (float)lo;
    s.h = 1.f - s.l;
    return s;
}

// ceil(extent / pooled) as an int: >= 1 for every number (the extent is >= 1); NaN: 0 samples, and the division by a count of 0 makes the outputs NaN
__device__ __forceinline__ int ra_grid(float extent, int pooled)
{
    const float g = ceilf(extent / (float)pooled);
    if (!(g == g)) return 0;
    return g >= 1073741824.f ? (1 << 30) : (int)g;
}

struct RaArgs {
    const float* in;      // [batch][channels][height][width]
    const float* rois;    // [n][5]
    float* out;           // [n][channels][ph][pw]
    int batch, channels, height, width, ph, pw, ratio, chunks;
    float scale;
};

// A block owns one ROI and RA_CH channels.  Phase 1: the ROI's two axis tables into LDS, ph * grid_h + pw * grid_w entries (the CUDA layout recomputes all of a
// sample's arithmetic per output and channel).  Phase 2: consecutive lanes take consecutive outputs of the block's [channel][ph][pw] run, which is contiguous in the
// output (coalesced stores) and keeps a wave's gathers inside one or two channel planes.  A sample outside contributes +0 and is skipped: the accumulator starts at
// +0 and can never be -0 (x + -x and +0 + -0 are +0 in round-to-nearest), so acc + (+0) == acc bit for bit.
// The body of both ROIAlign kernels: ROI `r` (5 floats) against the map `in` [batch][channels][height][width] at `scale`, channels c0 .. c0 + RA_CH - 1 into `out`
// (the ROI's [channels][ph][pw] run from c0 on).  Every thread of the block calls it (it holds a barrier).
__device__ __forceinline__ void ra_block(const float* in, int batch, int channels, int height, int width, float scale, const float* r, int ph, int pw, int ratio, int c0,
                                         float* out, RaSample* s_y, RaSample* s_x)
{
    const int t = threadIdx.x;
    const int bins = ph * pw, total = min(RA_CH, channels - c0) * bins;
    const float fb = r[0];
    if (!(fb > -1.f && fb < (float)batch)) {       // (int)fb outside 0 .. batch - 1: zeros, and no read of the input
        for (int o = t; o < total; o += 256) out[o] = 0.f;
        return;
    }
    const int b = (int)fb;
    const float sw = r[1] * scale, sh = r[2] * scale, ew = r[3] * scale, eh = r[4] * scale;
    const float dw = ew - sw, dh = eh - sh;
    const float rw = dw < 1.f ? 1.f : dw, rh = dh < 1.f ? 1.f : dh;     // std::max(d, 1): malformed ROIs are 1 x 1
    const float bh = rh / (float)ph, bw = rw / (float)pw;
    const int gh = ratio > 0 ? ratio : ra_grid(rh, ph), gw = ratio > 0 ? ratio : ra_grid(rw, pw);
    const bool tab_y = (long long)ph * gh <= RA_TAB, tab_x = (long long)pw * gw <= RA_TAB;
    if (tab_y) for (int i = t; i < ph * gh; i += 256) { const int p = i / gh; s_y[i] = ra_axis(sh, bh, p, i - p * gh, gh, height); }
    if (tab_x) for (int i = t; i < pw * gw; i += 256) { const int p = i / gw; s_x[i] = ra_axis(sw, bw, p, i - p * gw, gw, width); }
    __syncthreads();
    const float count = (float)(int)((unsigned)gh * (unsigned)gw);
    const size_t plane = (size_t)height * width;
    const float* base = in + ((size_t)b * channels + c0) * plane;
    for (int o = t; o < total; o += 256) {
        const int c = o / bins, bin = o - c * bins, py = bin / pw, px = bin - py * pw;
        const float* img = base + (size_t)c * plane;
        float acc = 0.f;
        for (int iy = 0; iy < gh; iy++) {
            const RaSample y = tab_y ? s_y[py * gh + iy] : ra_axis(sh, bh, py, iy, gh, height);
            if (y.lo < 0) continue;
            const float *r0 = img + (size_t)y.lo * width, *r1 = img + (size_t)y.hi * width;
            for (int ix = 0; ix < gw; ix++) {
                const RaSample x = tab_x ? s_x[px * gw + ix] : ra_axis(sw, bw, px, ix, gw, width);
                if (x.lo < 0) continue;
                const float w1 = y.h * x.h, w2 = y.h * x.l, w3 = y.l * x.h, w4 = y.l * x.l;
                acc += ((w1 * r0[x.lo] + w2 * r0[x.hi]) + w3 * r1[x.lo]) + w4 * r1[x.hi];
            }
        }
        out[o] = acc / count;
    }
}

__global__ void __launch_bounds__(256) k_roi_align(const RaArgs a)
{
    __shared__ RaSample s_y[RA_TAB], s_x[RA_TAB];
    const int roi = blockIdx.x / a.chunks, c0 = (blockIdx.x - roi * a.chunks) * RA_CH;
    ra_block(a.in, a.batch, a.channels, a.height, a.width, a.scale, a.rois + (size_t)roi * 5, a.ph, a.pw, a.ratio, c0,
             a.out + ((size_t)roi * a.channels + c0) * ((size_t)a.ph * a.pw), s_y, s_x);
}

// ifx_fpn_roi_align: the FPN Pooler in one launch.  The level table travels by value; thr[j], j = 1 .. levels - 1, is the smallest v = sqrt(area) / s0 + eps that
// reaches level j (made on the host: fpn_thresholds), so the device needs a correctly rounded sqrt, an IEEE division, an addition and the compares.
constexpr int FPN_MAX = 8;
struct FpnArgs {
    const float* in[FPN_MAX];      // per level [batch][channels][height[l]][width[l]]
    int height[FPN_MAX], width[FPN_MAX];
    float scale[FPN_MAX], thr[FPN_MAX];
    const float* rois;             // [n][5]
    float* out;                    // [n][channels][ph][pw]
    int32_t* lev_out;              // NULL or [n]
    int levels, batch, channels, ph, pw, ratio, chunks;
    float s0, eps;
};

// k_roi_align's grid and body; in front of it lane 0 finds the ROI's level and LDS hands it to the block.  No level (-1): zeros, and no map is read.
__global__ void __launch_bounds__(256) k_fpn_roi_align(const FpnArgs a)
{
    __shared__ RaSample s_y[RA_TAB], s_x[RA_TAB];
    __shared__ int s_level;
    const int t = threadIdx.x;
    const int roi = blockIdx.x / a.chunks, c0 = (blockIdx.x - roi * a.chunks) * RA_CH;
    const float* r = a.rois + (size_t)roi * 5;
    float* out = a.out + ((size_t)roi * a.channels + c0) * ((size_t)a.ph * a.pw);
    if (t == 0) {
        int lv = 0;
        if (a.levels > 1) {                        // one level: no mapping at all
            const float area = (r[3] - r[1] + 1.f) * (r[4] - r[2] + 1.f);
            const float v = sqrtf(area) / a.s0 + a.eps;
            if (!(v >= 0.f)) lv = -1;              // a NaN or negative area, a negative v: log2 is NaN
            else {
#pragma unroll
                for (int j = 1; j < FPN_MAX; j++) lv += (j < a.levels && v >= a.thr[j]) ? 1 : 0;
            }
        }
        s_level = lv;
        if (c0 == 0 && a.lev_out) a.lev_out[roi] = lv;
    }
    __syncthreads();
    const int lv = __builtin_amdgcn_readfirstlane(s_level);
    if (lv < 0) {
        const int total = min(RA_CH, a.channels - c0) * a.ph * a.pw;
        for (int o = t; o < total; o += 256) out[o] = 0.f;
        return;
    }
    ra_block(a.in[lv], a.batch, a.channels, a.height[lv], a.width[lv], a.scale[lv], r, a.ph, a.pw, a.ratio, c0, out, s_y, s_x);
}

constexpr int NMS_MAX = 8192;          // boxes of one call: the sort's keys (64 KB) and the kept flags live in one block's LDS
constexpr int NMS_BLOCKS = NMS_MAX / 64;

// The order as one ascending 64-bit key: score descending (-0 == +0), a NaN score behind every number, equal scores by ascending index.  No number maps to the
// NaN's high word (all ones would need the bit pattern 0xFFFFFFFF, which is a NaN), and the padding key ~0 lies behind every box.
__device__ __forceinline__ unsigned long long nms_key(float s, int i)
{
    uint32_t k = 0xFFFFFFFFu;
    if (s == s) {
        uint32_t u = s == 0.f ? 0u : __float_as_uint(s);
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);    // ascending in the float's order
        k = ~u;
    }
    return ((unsigned long long)k << 32) | (uint32_t)i;
}

// The sorting network of a 1024-thread block on P = 2^k keys in LDS, ascending; the keys written before the call need no barrier of their own.
__device__ __forceinline__ void nms_bitonic(unsigned long long* s_key, int P, int t)
{
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < (P >> 1); i += 1024) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                const unsigned long long x = s_key[lo], y = s_key[hi];
                if ((x > y) == ((lo & k) == 0)) { s_key[lo] = y; s_key[hi] = x; }
            }
            __syncthreads();
        }
}

// One block: a bitonic sort of P = 2^k >= n keys in LDS (the key is a total order: stability is not needed), then the boxes and groups gathered into that order.
__global__ void __launch_bounds__(1024) k_nms_sort(const float* boxes, const float* scores, const int32_t* groups, int n, int P, int32_t* order, float4* sboxes, int32_t* sgroups)
{
    __shared__ unsigned long long s_key[NMS_MAX];
    const int t = threadIdx.x;
    for (int i = t; i < P; i += 1024) s_key[i] = i < n ? nms_key(scores[i], i) : ~0ull;
    nms_bitonic(s_key, P, t);
    for (int i = t; i < n; i += 1024) {
        const int idx = (int)(uint32_t)s_key[i];
        order[i] = idx;
        sboxes[i] = make_float4(boxes[4 * (size_t)idx], boxes[4 * (size_t)idx + 1], boxes[4 * (size_t)idx + 2], boxes[4 * (size_t)idx + 3]);   // (the caller's pointer need not be 16-B aligned)
        sgroups[i] = groups ? groups[idx] : 0;
    }
}

// The pair mask, nms.cu:26-68: one wave per 64 x 64 tile of the upper triangle, bit j of word (row, cb) = row suppresses box cb * 64 + j (IoU > threshold, strictly;
// a NaN IoU compares false; same group; on the diagonal tile only j > row's lane).  max / min as fmaxf / fminf, every operation f32 and unfused, a true division.
// (sgroups NULL: one group -- the proposal stage)
// TF (the Keras layers: ifx_keras_proposals, ifx_keras_detections): the pair's IoU by tf.image.non_max_suppression's rule instead -- boxes y1, x1, y2, x2 with the
// far corner outside (no + 1), the corners ordered first, a pair with an area <= 0 has IoU 0 -- nms_iou_tf below; everything else is the same tile.
struct TfBox { float ymin, xmin, ymax, xmax, area; };
__device__ __forceinline__ TfBox nms_tf_box(const float4 b)
{
    TfBox o;
    o.ymin = fminf(b.x, b.z); o.ymax = fmaxf(b.x, b.z); o.xmin = fminf(b.y, b.w); o.xmax = fmaxf(b.y, b.w);
    o.area = (o.ymax - o.ymin) * (o.xmax - o.xmin);
    return o;
}
__device__ __forceinline__ float nms_iou_tf(const TfBox& a, const TfBox& b)
{
    if (a.area <= 0.f || b.area <= 0.f) return 0.f;
    const float ih = fmaxf(fminf(a.ymax, b.ymax) - fmaxf(a.ymin, b.ymin), 0.f), iw = fmaxf(fminf(a.xmax, b.xmax) - fmaxf(a.xmin, b.xmin), 0.f);
    const float inter = ih * iw;
    return inter / (a.area + b.area - inter);
}
template <bool TF = false>
__device__ __forceinline__ void nms_mask_tile(const float4* sboxes, const int32_t* sgroups, int n, int nb, float thr, unsigned long long* mask)
{
    const int cb = blockIdx.x, rb = blockIdx.y, t = threadIdx.x;
    if (cb < rb) return;
    __shared__ float4 s_box[64];
    __shared__ int s_grp[64];
    const int cn = min(64, n - cb * 64), rn = min(64, n - rb * 64);
    if (t < cn) { s_box[t] = sboxes[cb * 64 + t]; s_grp[t] = sgroups ? sgroups[cb * 64 + t] : 0; }
    __syncthreads();
    if (t >= rn) return;
    const int row = rb * 64 + t;
    const float4 a = sboxes[row];
    const int ga = sgroups ? sgroups[row] : 0;
    const float sa = (a.z - a.x + 1.f) * (a.w - a.y + 1.f);
    const int first = rb == cb ? t + 1 : 0;
    unsigned long long word = 0;
    if (TF) {
        const TfBox ta = nms_tf_box(a);
        for (int j = 0; j < cn; j++) {
            const float iou = nms_iou_tf(ta, nms_tf_box(s_box[j]));
            if (iou > thr && s_grp[j] == ga && j >= first) word |= 1ull << j;
        }
        mask[(size_t)row * nb + cb] = word;
        return;
    }
    for (int j = 0; j < cn; j++) {
        const float4 b = s_box[j];
        const float left = fmaxf(a.x, b.x), right = fminf(a.z, b.z), top = fmaxf(a.y, b.y), bottom = fminf(a.w, b.w);
        const float w = fmaxf(right - left + 1.f, 0.f), hh = fmaxf(bottom - top + 1.f, 0.f);
        const float inter = w * hh;
        const float sb = (b.z - b.x + 1.f) * (b.w - b.y + 1.f);
        const float iou = inter / (sa + sb - inter);
        if (iou > thr && s_grp[j] == ga && j >= first) word |= 1ull << j;
    }
    mask[(size_t)row * nb + cb] = word;
}

__global__ void __launch_bounds__(64) k_nms_mask(const float4* sboxes, const int32_t* sgroups, int n, int nb, float thr, unsigned long long* mask)
{
    nms_mask_tile(sboxes, sgroups, n, nb, thr, mask);
}

// k_nms_mask where the number of boxes is on the device and the grid is sized for what the host knows of it: the proposal stage's survivors (one group: sgroups
// NULL; at most 8192 of them, the first test never fires) and the box head's candidates (the class as the group; above the cap nothing is done)
__global__ void __launch_bounds__(64) k_nms_mask_dev(const float4* sboxes, const int32_t* sgroups, const int32_t* n_dev, int nb, float thr, unsigned long long* mask)
{
    const int n = n_dev[0];
    if (n > NMS_MAX || (int)blockIdx.x * 64 >= n) return;      // (the column block; the row block is not behind it where the tile is computed)
    nms_mask_tile(sboxes, sgroups, n, nb, thr, mask);
}

// k_nms_mask_dev by TensorFlow's IoU: the Keras proposal layer (one group) and detection layer (the class as the group)
__global__ void __launch_bounds__(64) k_nms_mask_dev_tf(const float4* sboxes, const int32_t* sgroups, const int32_t* n_dev, int nb, float thr, unsigned long long* mask)
{
    const int n = n_dev[0];
    if (n > NMS_MAX || (int)blockIdx.x * 64 >= n) return;
    nms_mask_tile<true>(sboxes, sgroups, n, nb, thr, mask);
}

// Exclusive scan of one value per thread over a block of W waves (64 W threads, every one of them calls): __shfl_up inside the wave, the wave sums through the W
// words s_w, one barrier.  *total (may be NULL): the sum over the block.  The reuse rule, for every caller: s_w may be written again -- by a second scan through the
// same words as by anything aliased onto them -- only behind a barrier that FOLLOWS the return, since a wave may still be reading the sums when another has returned.
template <int W, class T>
__device__ __forceinline__ T block_excl_scan(T mine, T* s_w, T* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = mine;
    for (int d = 1; d < 64; d <<= 1) { const T v = __shfl_up(incl, d); if (lane >= d) incl += v; }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    T excl = incl - mine, sum = 0;
    for (int w = 0; w < W; w++) { const T v = s_w[w]; if (w < wave) excl += v; sum += v; }
    if (total) *total = sum;
    return excl;
}

// The LDS state of the walk and of the scan behind it: one instance per reduce kernel.  The arrays come first so that each starts on a multiple of 16 bytes
// (the wave sums are read as four 16-byte words).  The number of rows kept so far is no member: every thread adds up the same keepw words in a register; as a
// fifth member it would round the struct up to 9296 bytes and k_bd_reduce's LDS up by 8.
struct NmsWalk {
    unsigned long long remv[NMS_BLOCKS];   // per 64-box block: the boxes the kept rows in front of it suppress
    uint8_t flag[NMS_MAX];                 // the kept flags
    int wsum[16];                          // block_excl_scan's wave sums
    unsigned long long keepw;              // the kept rows of the block the walk is at
};

// The reduction nms.cu:99-123 does on the host, in one block, and the output.  Per 64-box block b: wave 0 takes the 64 diagonal words with one load per lane and
// resolves them in registers (64 steps of two lane reads, no memory in between); then all 16 waves OR the kept rows' words of the columns behind b into the removal
// words in LDS, 128 columns x 8 row groups, consecutive lanes on consecutive words of a row.  Two global round trips per 64 boxes, none per box.
// Then the kept flags by ORIGINAL index (LDS), a block scan, and the kept indices in ascending order, -1 behind them, the count.
// The walk over the 64-box blocks, for a 1024-thread block: on return s.flag[order ? order[row] : row] is 1 for every kept row in front of the block the walk
// stopped at.  It stops behind the block in which the kept rows reach `limit` (the proposal stage wants the first few hundred kept of thousands).
__device__ __forceinline__ void nms_walk(const unsigned long long* mask, const int32_t* order, int n, int nb, int limit, NmsWalk& s)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int kept = 0;
    if (t < NMS_BLOCKS) s.remv[t] = 0;
    for (int i = t; i < n; i += 1024) s.flag[i] = 0;
    __syncthreads();
    for (int b = 0; b * 64 < n; b++) {
        if (wave == 0) {
            const int row = b * 64 + lane;
            const unsigned long long d = row < n ? mask[(size_t)row * nb + b] : 0ull;
            const uint32_t dlo = (uint32_t)d, dhi = (uint32_t)(d >> 32);
            unsigned long long removed = s.remv[b], kw = 0;
#pragma unroll
            for (int i = 0; i < 64; i++) {
                const unsigned long long di = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)dhi, i) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)dlo, i);
                const unsigned long long m = ((removed >> i) & 1ull) ? 0ull : ~0ull;    // box i is kept: a suppressed box suppresses nothing
                kw |= (1ull << i) & m;
                removed |= di & m;
            }
            const int rows = min(64, n - b * 64);
            if (rows < 64) kw &= (1ull << rows) - 1ull;
            if (lane == 0) s.keepw = kw;
            if (row < n && ((kw >> lane) & 1ull)) s.flag[order ? order[row] : row] = 1;
        }
        __syncthreads();
        const unsigned long long kw = s.keepw;
        kept += __popcll(kw);
        if (kept >= limit) break;              // (uniform: every thread reads the same word behind the barrier, and nothing writes it before the next one)
        const int cg = t & (NMS_BLOCKS - 1), rg = t >> 7, c = b + 1 + cg;
        if (c * 64 < n) {
            unsigned long long acc = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int i = rg * 8 + k;
                if ((kw >> i) & 1ull) acc |= mask[(size_t)(b * 64 + i) * nb + c];    // kept rows are < n, columns behind b are in the upper triangle: all written
            }
            if (acc) atomicOr(&s.remv[c], acc);
        }
        __syncthreads();
    }
}

// Eight consecutive flags per thread of a 1024-thread block: the thread's set flags as bits, the rank of its first one among all set flags, and their number.
// (flags: s.flag, or the caller's own array of n flags; the scan goes through s.wsum either way -- block_excl_scan's reuse rule)
__device__ __forceinline__ void nms_flag_scan(NmsWalk& s, const uint8_t* flags, int n, uint32_t& bits, int& pos, int& total)
{
    const int t = threadIdx.x;
    int mine = 0;
    bits = 0;
    for (int k = 0; k < 8; k++) {
        const int i = t * 8 + k;
        if (i < n && flags[i]) { bits |= 1u << k; mine++; }
    }
    pos = block_excl_scan<16>(mine, s.wsum, &total);
}

__global__ void __launch_bounds__(1024) k_nms_reduce(const unsigned long long* mask, const int32_t* order, int n, int nb, long long* keep, int32_t* count)
{
    __shared__ NmsWalk s;
    const int t = threadIdx.x;
    nms_walk(mask, order, n, nb, 0x7FFFFFFF, s);
    uint32_t bits;
    int pos, total;
    nms_flag_scan(s, s.flag, n, bits, pos, total);           // by ORIGINAL index
    for (int k = 0; k < 8; k++)
        if (bits & (1u << k)) keep[pos++] = t * 8 + k;
    for (int i = total + t; i < n; i += 1024) keep[i] = -1;
    if (t == 0) count[0] = total;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------------------
// The RPN's proposal stage of one level of one image and the box decoding it contains: ifx_rpn_proposals and ifx_box_decode (RPNPostProcessor.
// forward_for_single_feature_map, maskrcnn_benchmark/modeling/rpn/inference.py:74-121; BoxCoder.decode, modeling/box_coder.py:52-95; the rule in full:
// include/ifx_c_api.h, in numpy: tests/rpn_proposals_numpy.py).  Select, decode, clip, filter, suppress, truncate: everything stays on the device.

// EXP of the rule: f64, exp(x) = 2^k * p(r) with Cody-Waite's two-word ln 2 and the Taylor sum to r^13 (|r| <= 0.35: the tail is below 2^-60), then ONE rounding
// to f32.  Every step a separate multiplication and addition (the build has -ffp-contract=off).
__device__ __forceinline__ float rpn_exp(float xf)
{
    if (xf != xf) return xf;
    double x = (double)xf;
    x = x < -104.0 ? -104.0 : (x > 90.0 ? 90.0 : x);
    const double k = rint(x * 1.4426950408889634);
    const double r = (x - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 1.0 / 2.0;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return (float)ldexp(p, (int)k);
}

struct BoxCode { float wx, wy, ww, wh, xform_clip, xmax, ymax; int clip; };   // xmax, ymax: image_w - 1, image_h - 1 of the clip (clip != 0)

// BoxCoder.decode of one box (box_coder.py:62-93, operation for operation) and BoxList.clip_to_image (bounding_box.py:214-219); a NaN stays a NaN in both
__device__ __forceinline__ float4 box_decode_one(const float4 b, float c0, float c1, float c2, float c3, const BoxCode& q)
{
    const float w = b.z - b.x + 1.f, h = b.w - b.y + 1.f;
    const float cx = b.x + 0.5f * w, cy = b.y + 0.5f * h;
    const float dx = c0 / q.wx, dy = c1 / q.wy;
    float dw = c2 / q.ww, dh = c3 / q.wh;
    dw = dw > q.xform_clip ? q.xform_clip : dw;
    dh = dh > q.xform_clip ? q.xform_clip : dh;
    const float pcx = dx * w + cx, pcy = dy * h + cy;
    const float pw = rpn_exp(dw) * w, ph = rpn_exp(dh) * h;
    float4 o = make_float4(pcx - 0.5f * pw, pcy - 0.5f * ph, pcx + 0.5f * pw - 1.f, pcy + 0.5f * ph - 1.f);
    if (q.clip) {
        o.x = o.x < 0.f ? 0.f : (o.x > q.xmax ? q.xmax : o.x);
        o.y = o.y < 0.f ? 0.f : (o.y > q.ymax ? q.ymax : o.y);
        o.z = o.z < 0.f ? 0.f : (o.z > q.xmax ? q.xmax : o.z);
        o.w = o.w < 0.f ? 0.f : (o.w > q.ymax ? q.ymax : o.w);
    }
    return o;
}

// ifx_box_decode: one thread, one output box; codes and out [n][4k], boxes [n][4]
__global__ void __launch_bounds__(256) k_box_decode(const float* codes, const float* boxes, long long total, int k, const BoxCode q, float* out)
{
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const long long row = o / k;
    const float4 b = make_float4(boxes[4 * row], boxes[4 * row + 1], boxes[4 * row + 2], boxes[4 * row + 3]);
    const float* c = codes + 4 * o;
    const float4 r = box_decode_one(b, c[0], c[1], c[2], c[3], q);
    out[4 * o] = r.x; out[4 * o + 1] = r.y; out[4 * o + 2] = r.z; out[4 * o + 3] = r.w;
}

// ---- selection: the K <= 8192 best of n > 8192 logits.  The order is nms_key's: its high word k32 ascending, then the flat anchor index ascending.
// A radix select finds T, the k32 of rank K, in three histogram passes over 11 + 11 + 10 bits (k_rpn_hist<0..2>: a block counts 2048 keys into LDS and adds its
// non-empty bins to the pass's global histogram; each later launch first picks the previous pass's digit out of that histogram, every block for itself).
// Winners: every key with k32 < T, and of those with k32 == T the first K - #less by ascending index.  k_rpn_count counts both kinds per block of 2048
// CONSECUTIVE anchor indices, k_rpn_compact turns the counts in front of a block and a scan inside it into each winner's place: no atomics, a fixed layout.
constexpr int RPN_CHUNK = 2048;       // keys of a 256-thread block: eight per thread
constexpr int RPN_BINS = 2048;
constexpr int RPN_MAX_N = 1 << 24;

__device__ __forceinline__ uint32_t rpn_key32(float s) { return (uint32_t)(nms_key(s, 0) >> 32); }

// the logit of flat anchor index i = (y * W + x) * A + a out of [A][H][W]: permute_and_flatten's indexing (rpn/utils.py), nothing is permuted in memory
// (S > 0, the Keras proposal layer: the scores lie flat, S floats apart, and A, HW are not read; S == 0 is the [A][H][W] form, compiled as it always was)
template <int S = 0>
__device__ __forceinline__ float rpn_logit(const float* obj, int i, int A, int HW)
{
    if (S) return obj[(size_t)i * S];
    const int cell = i / A;
    return obj[(size_t)(i - cell * A) * HW + cell];
}

// 256 threads: the bin that holds rank `rank` (0-based) of a 2048-bin histogram, and the rank inside that bin.  The histogram's total is > rank.
__device__ __forceinline__ void rpn_pick(const uint32_t* hist, uint32_t rank, uint32_t* s_w, uint32_t* s_out, uint32_t& digit, uint32_t& rest)
{
    const int t = threadIdx.x;
    uint32_t c[8], mine = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) { c[k] = hist[t * 8 + k]; mine += c[k]; }
    uint32_t excl = block_excl_scan<4, uint32_t>(mine, s_w, nullptr);
    if (excl <= rank && rank < excl + mine) {          // one thread
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if (rank < excl + c[k]) { s_out[0] = (uint32_t)(t * 8 + k); s_out[1] = rank - excl; break; }
            excl += c[k];
        }
    }
    __syncthreads();
    digit = s_out[0]; rest = s_out[1];
}

// state[2p], state[2p + 1], p = 1 .. 3: the key's leading bits fixed by the first p passes and the rank among the keys that share them
// (the bodies of the selection's kernels are device functions of one 256-thread block: the single-level kernels and the level-batched ones further down call them)
template <int PASS, int S = 0>
__device__ __forceinline__ void rpn_hist_block(const float* obj, int n, uint32_t K, uint32_t* hist, uint32_t* state)
{
    __shared__ uint32_t s_hist[RPN_BINS];
    __shared__ uint32_t s_w[4], s_out[2];
    const int t = threadIdx.x;
    for (int i = t; i < RPN_BINS; i += 256) s_hist[i] = 0;
    uint32_t prefix = 0;
    if (PASS > 0) {
        const uint32_t rank = PASS == 1 ? K - 1 : state[2 * (PASS - 1) + 1], lead = PASS == 1 ? 0u : state[2 * (PASS - 1)];
        uint32_t d, rest;
        rpn_pick(hist + (PASS - 1) * RPN_BINS, rank, s_w, s_out, d, rest);
        prefix = (lead << 11) | d;
        if (blockIdx.x == 0 && t == 0) { state[2 * PASS] = prefix; state[2 * PASS + 1] = rest; }
    } else __syncthreads();
    const int base = blockIdx.x * RPN_CHUNK;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int m = base + k * 256 + t;              // memory order: the histogram does not care, and the loads are contiguous
        if (m < n) {
            const uint32_t key = rpn_key32(S ? obj[(size_t)m * S] : obj[m]);
            if (PASS == 0) atomicAdd(&s_hist[key >> 21], 1u);
            else if (PASS == 1) { if ((key >> 21) == prefix) atomicAdd(&s_hist[(key >> 10) & 2047u], 1u); }
            else if ((key >> 10) == prefix) atomicAdd(&s_hist[key & 1023u], 1u);
        }
    }
    __syncthreads();
    for (int i = t; i < RPN_BINS; i += 256) { const uint32_t v = s_hist[i]; if (v) atomicAdd(&hist[PASS * RPN_BINS + i], v); }
}

template <int PASS, int S = 0>
__global__ void __launch_bounds__(256) k_rpn_hist(const float* obj, int n, uint32_t K, uint32_t* hist, uint32_t* state)
{
    rpn_hist_block<PASS, S>(obj, n, K, hist, state);
}

// a thread's eight consecutive anchor indices against T: bit k of less / equal
template <int S = 0>
__device__ __forceinline__ uint2 rpn_classify(const float* obj, int n, int A, int HW, int first, uint32_t T)
{
    uint32_t less = 0, equal = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int i = first + k;
        if (i < n) {
            const uint32_t key = rpn_key32(rpn_logit<S>(obj, i, A, HW));
            if (key < T) less |= 1u << k;
            else if (key == T) equal |= 1u << k;
        }
    }
    return make_uint2(less, equal);
}

// blk[b], blk[nblk + b]: how many keys of block b's 2048 anchor indices lie in front of T and on T
template <int S = 0>
__device__ __forceinline__ void rpn_count_block(const float* obj, int n, int A, int HW, const uint32_t* hist, uint32_t* state, uint32_t* blk, int nblk)
{
    __shared__ uint32_t s_w[4], s_out[2], s_sum[2];
    const int t = threadIdx.x;
    if (t < 2) s_sum[t] = 0;
    uint32_t d, rest;
    rpn_pick(hist + 2 * RPN_BINS, state[5], s_w, s_out, d, rest);
    const uint32_t T = (state[4] << 10) | d;
    if (blockIdx.x == 0 && t == 0) { state[6] = T; state[7] = rest; }
    const uint2 le = rpn_classify<S>(obj, n, A, HW, blockIdx.x * RPN_CHUNK + t * 8, T);
    const uint32_t less = le.x, equal = le.y;
    if (less) atomicAdd(&s_sum[0], (uint32_t)__popc(less));
    if (equal) atomicAdd(&s_sum[1], (uint32_t)__popc(equal));
    __syncthreads();
    if (t < 2) blk[t * nblk + blockIdx.x] = s_sum[t];
}

__global__ void __launch_bounds__(256) k_rpn_count(const float* obj, int n, int A, int HW, const uint32_t* hist, uint32_t* state, uint32_t* blk, int nblk)
{
    rpn_count_block(obj, n, A, HW, hist, state, blk, nblk);
}

// M lists of per-block counts, `stride` apart: the sums of list m's blk[0 .. b) into s_sum[m], for a 256-thread block.  They are complete behind the caller's next
// barrier (sums of integers: the arrival order cannot show).
template <int M>
__device__ __forceinline__ void block_sum_before(const uint32_t* blk, int stride, int b, uint32_t* s_sum)
{
    const int t = threadIdx.x;
    if (t < M) s_sum[t] = 0;
    __syncthreads();
    uint32_t v[M] = {};
    for (int i = t; i < b; i += 256)
        for (int m = 0; m < M; m++) v[m] += blk[m * stride + i];
    for (int m = 0; m < M; m++)
        if (v[m]) atomicAdd(&s_sum[m], v[m]);
}

// cand[0 .. K): the winners' 64-bit keys -- those in front of T in index order, then the first state[7] + 1 of those on T in index order
template <int S = 0>
__device__ __forceinline__ void rpn_compact_block(const float* obj, int n, int A, int HW, uint32_t K, const uint32_t* state, const uint32_t* blk, int nblk,
                                                  unsigned long long* cand)
{
    __shared__ uint32_t s_before[2], s_w[4];
    const int t = threadIdx.x, b = blockIdx.x;
    block_sum_before<2>(blk, nblk, b, s_before);
    const uint32_t T = state[6], take = state[7] + 1u;
    const uint2 le = rpn_classify<S>(obj, n, A, HW, b * RPN_CHUNK + t * 8, T);
    const uint32_t less = le.x, equal = le.y;
    const uint32_t mine = (uint32_t)__popc(less) | ((uint32_t)__popc(equal) << 16);     // both counts of a block are <= 2048: one scan for the two
    const uint32_t excl = block_excl_scan<4, uint32_t>(mine, s_w, nullptr);
    uint32_t pl = s_before[0] + (excl & 0xFFFFu), pe = s_before[1] + (excl >> 16);
    const uint32_t base = take <= K ? K - take : 0u;   // the keys in front of T: exactly K - take of them
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int i = b * RPN_CHUNK + t * 8 + k;
        if (less & (1u << k)) { if (pl < base) cand[pl] = ((unsigned long long)rpn_key32(rpn_logit<S>(obj, i, A, HW)) << 32) | (uint32_t)i; pl++; }
        else if (equal & (1u << k)) { if (pe < take && base + pe < K) cand[base + pe] = ((unsigned long long)T << 32) | (uint32_t)i; pe++; }
    }
}

__global__ void __launch_bounds__(256) k_rpn_compact(const float* obj, int n, int A, int HW, uint32_t K, const uint32_t* state, const uint32_t* blk, int nblk,
                                                      unsigned long long* cand)
{
    rpn_compact_block(obj, n, A, HW, K, state, blk, nblk, cand);
}

struct RpnArgs {
    const float *obj, *reg, *anc;                      // [A][H][W], [4A][H][W], [H W A][4]
    const unsigned long long* cand;                    // the selection's winners, NULL: every anchor is a candidate (n <= 8192)
    int n, A, HW, m, P;                                // m = min(pre_nms_top_n, n) candidates, P = 2^k >= the keys sorted
    BoxCode q;
    float min_size;
    float4* sboxes; float* slogit; int32_t* sindex; int32_t* ns;
};

// One block: the candidates into the order (k_nms_sort's network), then per thread eight consecutive candidates: the code and the anchor gathered through the
// [A][H][W] indexing, decode, clip, the small-box test; a block scan keeps the survivors in the candidates' order.  They are the sorted boxes the pair mask reads.
__device__ __forceinline__ void rpn_sort_decode_block(const RpnArgs& a)
{
    __shared__ unsigned long long s_key[NMS_MAX];
    const int t = threadIdx.x;
    if (a.cand) for (int i = t; i < a.P; i += 1024) s_key[i] = i < a.m ? a.cand[i] : ~0ull;
    else for (int i = t; i < a.P; i += 1024) s_key[i] = i < a.n ? nms_key(rpn_logit(a.obj, i, a.A, a.HW), i) : ~0ull;
    nms_bitonic(s_key, a.P, t);
    int idx[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int c = t * 8 + k;
        const uint32_t i = c < a.m ? (uint32_t)s_key[c] : 0xFFFFFFFFu;
        idx[k] = i < (uint32_t)a.n ? (int)i : -1;      // (every key holds an anchor index; the test keeps the gathers inside the inputs whatever the keys are)
    }
    __syncthreads();
    int* s_wsum = (int*)s_key;                         // (the keys are in registers: their LDS holds the scan's wave sums from here on)
    float4 box[8];
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if (idx[k] < 0) continue;
        const int i = idx[k], cell = i / a.A, an = i - cell * a.A;
        const float* c = a.reg + (size_t)(4 * an) * a.HW + cell;
        const float4 b = make_float4(a.anc[4 * (size_t)i], a.anc[4 * (size_t)i + 1], a.anc[4 * (size_t)i + 2], a.anc[4 * (size_t)i + 3]);
        box[k] = box_decode_one(b, c[0], c[a.HW], c[2 * (size_t)a.HW], c[3 * (size_t)a.HW], a.q);
        if (box[k].z - box[k].x + 1.f >= a.min_size && box[k].w - box[k].y + 1.f >= a.min_size) bits |= 1u << k;     // remove_small_boxes (boxlist_ops.py:34-48): a NaN is false
    }
    int total;
    int pos = block_excl_scan<16>((int)__popc(bits), s_wsum, &total);
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (bits & (1u << k)) {
            a.sboxes[pos] = box[k];
            a.slogit[pos] = rpn_logit(a.obj, idx[k], a.A, a.HW);
            a.sindex[pos] = idx[k];
            pos++;
        }
    if (t == 0) a.ns[0] = total;
}

__global__ void __launch_bounds__(1024) k_rpn_sort_decode(const RpnArgs a)
{
    rpn_sort_decode_block(a);
}

// k_nms_reduce's walk, stopped once `post` boxes are kept, and the output in the candidates' order: the first min(kept, post) kept rows with box, logit and index;
// zeros and -1 behind them up to post; the count
__device__ __forceinline__ void rpn_reduce_block(const unsigned long long* mask, const float4* sboxes, const float* slogit, const int32_t* sindex, const int32_t* ns, int nb,
                                                 int post, float* boxes, float* logits, long long* index, int32_t* count)
{
    __shared__ NmsWalk s;
    const int t = threadIdx.x, n = ns[0];
    nms_walk(mask, nullptr, n, nb, post, s);
    uint32_t bits;
    int pos, total;
    nms_flag_scan(s, s.flag, n, bits, pos, total);           // by sorted row
    for (int k = 0; k < 8; k++)
        if (bits & (1u << k)) {
            if (pos < post) {
                const int row = t * 8 + k;
                const float4 b = sboxes[row];
                boxes[4 * pos] = b.x; boxes[4 * pos + 1] = b.y; boxes[4 * pos + 2] = b.z; boxes[4 * pos + 3] = b.w;
                if (logits) logits[pos] = slogit[row];
                if (index) index[pos] = sindex[row];
            }
            pos++;
        }
    total = min(total, post);
    for (int i = total + t; i < post; i += 1024) {
        boxes[4 * i] = 0.f; boxes[4 * i + 1] = 0.f; boxes[4 * i + 2] = 0.f; boxes[4 * i + 3] = 0.f;
        if (logits) logits[i] = 0.f;
        if (index) index[i] = -1;
    }
    if (t == 0) count[0] = total;
}

__global__ void __launch_bounds__(1024) k_rpn_reduce(const unsigned long long* mask, const float4* sboxes, const float* slogit, const int32_t* sindex, const int32_t* ns, int nb,
                                                     int post, float* boxes, float* logits, long long* index, int32_t* count)
{
    rpn_reduce_block(mask, sboxes, slogit, sindex, ns, nb, post, boxes, logits, index, count);
}

// ---- the proposal stage over all levels of an FPN in one call: ifx_rpn_proposals_fpn (the rule: include/ifx_c_api.h, in numpy: tests/rpn_fpn_numpy.py).  The
// kernels above run per level side by side -- the level is a grid dimension, every block takes its level's entry of a table that travels in the kernel arguments
// -- and one more kernel merges the levels' kept lists (RPNPostProcessor.select_over_all_levels, inference.py:152-179).  The number of launches does not depend on
// the number of levels.
constexpr int RPN_MAX_LEVELS = 8;
constexpr size_t RPN_ZERO_WORDS = 3 * RPN_BINS + 8;    // of a level that selects: the three histograms and the selection's state

struct RpnLevel {
    const float *obj, *reg, *anc;                      // as RpnArgs
    int n, A, HW, m, P, nb;                            // nb: the 64-box blocks of the level's mask, m rounded up
    int nblk;                                          // 2048-key blocks of the selection, 0: n <= 8192, the level does not select
    int cap;                                           // min(post_nms_top_n, m): the rows of the kept lists
    unsigned long long *cand, *mask;                   // the level's slices of the scratch, each sized from its own m
    float4* sboxes; float* slogit; int32_t* sindex;
    uint32_t *blk, *hist;                              // hist: histograms and state, zeroed per call (NULL: the level does not select)
    float *kbox, *klogit; long long* kindex;           // the kept rows in the level's order: what ifx_rpn_proposals writes for the level, cap rows
};

struct RpnFpn {
    RpnLevel lv[RPN_MAX_LEVELS];
    int32_t *ns, *cnt;                                 // per level: the survivors in front of the suppression, and c_l
    int L;
};

// the selection's five kernels, blockIdx.y = the level, gridDim.x = the largest nblk: a block of a level that does not select, or behind its level's blocks,
// leaves before the first barrier (block-uniform)
template <int PASS>
__global__ void __launch_bounds__(256) k_rpn_fpn_hist(const RpnFpn f)
{
    const RpnLevel& v = f.lv[blockIdx.y];
    if ((int)blockIdx.x >= v.nblk) return;
    rpn_hist_block<PASS>(v.obj, v.n, (uint32_t)v.m, v.hist, v.hist + 3 * RPN_BINS);
}

__global__ void __launch_bounds__(256) k_rpn_fpn_count(const RpnFpn f)
{
    const RpnLevel& v = f.lv[blockIdx.y];
    if ((int)blockIdx.x >= v.nblk) return;
    rpn_count_block(v.obj, v.n, v.A, v.HW, v.hist, v.hist + 3 * RPN_BINS, v.blk, v.nblk);
}

__global__ void __launch_bounds__(256) k_rpn_fpn_compact(const RpnFpn f)
{
    const RpnLevel& v = f.lv[blockIdx.y];
    if ((int)blockIdx.x >= v.nblk) return;
    rpn_compact_block(v.obj, v.n, v.A, v.HW, (uint32_t)v.m, v.hist + 3 * RPN_BINS, v.blk, v.nblk, v.cand);
}

// one block per level: k_rpn_sort_decode on the level's entry (a level without anchors sorts two padding keys and counts no survivor)
__global__ void __launch_bounds__(1024) k_rpn_fpn_sort_decode(const RpnFpn f, const BoxCode q, float min_size)
{
    const RpnLevel& v = f.lv[blockIdx.x];
    RpnArgs a;
    a.obj = v.obj; a.reg = v.reg; a.anc = v.anc; a.cand = v.nblk ? v.cand : nullptr;
    a.n = v.n; a.A = v.A; a.HW = v.HW; a.m = v.m; a.P = v.P;
    a.q = q; a.min_size = min_size;
    a.sboxes = v.sboxes; a.slogit = v.slogit; a.sindex = v.sindex; a.ns = f.ns + blockIdx.x;
    rpn_sort_decode_block(a);
}

// grid (largest nb, largest nb, levels): k_nms_mask_dev per level; a tile beyond its level's blocks or survivors leaves
__global__ void __launch_bounds__(64) k_rpn_fpn_mask(const RpnFpn f, float thr)
{
    const RpnLevel& v = f.lv[blockIdx.z];
    const int n = f.ns[blockIdx.z];
    if ((int)blockIdx.x >= v.nb || (int)blockIdx.y >= v.nb || (int)blockIdx.x * 64 >= n) return;
    nms_mask_tile(v.sboxes, nullptr, n, v.nb, thr, v.mask);
}

// one block per level: k_rpn_reduce into the level's kept lists, c_l into cnt
__global__ void __launch_bounds__(1024) k_rpn_fpn_reduce(const RpnFpn f)
{
    const int l = blockIdx.x;
    const RpnLevel& v = f.lv[l];
    rpn_reduce_block(v.mask, v.sboxes, v.slogit, v.sindex, f.ns + l, v.nb, v.cap, v.kbox, v.klogit, v.kindex, f.cnt + l);
}

// The selection over the levels.  Every level's list is in the rule's order already: row r of level l, at position off_l + r of the concatenation, has the 64-bit
// key (k32 of its logit, off_l + r), a total order in which each list ascends.  Its rank is r plus, for every other level, the number of that level's rows with a
// smaller key: one binary search per other level, no sort, no atomics, no LDS.  The ranks are a permutation of 0 .. T - 1; rank < F writes output row rank.
// One thread per row of the lists' capacity (and per output row: rows T .. F - 1 are the padding); thread 0 writes the counts.
__global__ void __launch_bounds__(256) k_rpn_fpn_merge(const RpnFpn f, int F, float* boxes, float* logits, int32_t* level, long long* index, int32_t* count,
                                                       int32_t* level_counts)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    int mine = -1, r = 0, T = 0, capoff = 0;
    unsigned long long key = 0;
    float lg = 0.f;
    const float* kbox = nullptr;
    const long long* kindex = nullptr;
#pragma unroll
    for (int l = 0; l < RPN_MAX_LEVELS; l++) {
        if (l >= f.L) break;
        const int c = f.cnt[l], cap = f.lv[l].cap;
        if (g >= capoff && g - capoff < c) {           // (c <= cap: the row lies in level l's list)
            mine = l; r = g - capoff;
            lg = f.lv[l].klogit[r];
            key = ((unsigned long long)rpn_key32(lg) << 32) | (uint32_t)(T + r);
            kbox = f.lv[l].kbox; kindex = f.lv[l].kindex;
        }
        capoff += cap; T += c;
    }
    if (mine >= 0) {
        int rank = r, off = 0;
#pragma unroll
        for (int l = 0; l < RPN_MAX_LEVELS; l++) {
            if (l >= f.L) break;
            const int c = f.cnt[l];
            if (l != mine) {
                const float* kl = f.lv[l].klogit;
                int lo = 0, hi = c;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const unsigned long long k = ((unsigned long long)rpn_key32(kl[mid]) << 32) | (uint32_t)(off + mid);
                    if (k < key) lo = mid + 1; else hi = mid;
                }
                rank += lo;
            }
            off += c;
        }
        if (rank < F) {
            boxes[4 * rank] = kbox[4 * r]; boxes[4 * rank + 1] = kbox[4 * r + 1]; boxes[4 * rank + 2] = kbox[4 * r + 2]; boxes[4 * rank + 3] = kbox[4 * r + 3];
            if (logits) logits[rank] = lg;
            if (level) level[rank] = mine;
            if (index) index[rank] = kindex[r];
        }
    }
    if (g >= T && g < F) {
        boxes[4 * g] = 0.f; boxes[4 * g + 1] = 0.f; boxes[4 * g + 2] = 0.f; boxes[4 * g + 3] = 0.f;
        if (logits) logits[g] = 0.f;
        if (level) level[g] = -1;
        if (index) index[g] = -1;
    }
    if (g == 0) {
        count[0] = min(T, F);
        if (level_counts)
            for (int l = 0; l < f.L; l++) level_counts[l] = f.cnt[l];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------------------
// The box head's post-processing of one image: ifx_box_detections (PostProcessor.forward / filter_results, maskrcnn_benchmark/modeling/roi_heads/box_head/
// inference.py:43-146; the rule in full: include/ifx_c_api.h, in numpy: tests/box_detections_numpy.py).  Softmax, threshold, decode, clip, per-class suppression,
// the limit to detections_per_img: everything stays on the device, the number of candidates K included.
constexpr int BD_MAX_C = 1024;
constexpr int BD_CHUNK = 2048;         // plane positions of a 256-thread block of the count and the compaction: eight consecutive ones per thread

// One wave per row, four rows per block.  The lanes find the row's maximum (exact in any order) and a NaN, park e_j = EXP(x_j - m) in LDS, and then EVERY lane runs
// the same f64 sum over j = 0 .. C - 1 out of LDS (a broadcast read per step): the order of the additions is the rule, so no tree and no cross-lane reduction.
// Each lane forms p_j of its own j and writes it -- or a NaN where (r, j) is no candidate -- into the class-major plane [(C - 1)][R].
__global__ void __launch_bounds__(256) k_bd_softmax(const float* logits, int R, int C, float thresh, float* plane)
{
    __shared__ float s_e[4][BD_MAX_C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = blockIdx.x * 4 + wave;
    const bool live = r < R;
    const float* x = logits + (size_t)(live ? r : 0) * C;
    float m = -INFINITY;
    bool nan = false;
    if (live)
        for (int j = lane; j < C; j += 64) { const float v = x[j]; nan |= v != v; m = fmaxf(m, v); }
    for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    const bool bad = __any(nan) || !(fabsf(m) < INFINITY);
    if (live && !bad)
        for (int j = lane; j < C; j += 64) s_e[wave][j] = rpn_exp(x[j] - m);
    __syncthreads();
    if (!live) return;
    double s = 0.0;
    if (!bad)
        for (int j = 0; j < C; j++) s = s + (double)s_e[wave][j];
    for (int j = lane; j < C; j += 64) {
        if (j == 0) continue;
        float p = __uint_as_float(0x7FC00000u);
        if (!bad) { const float q = (float)((double)s_e[wave][j] / s); if (q > thresh) p = q; }
        plane[(size_t)(j - 1) * R + r] = p;
    }
}

// bit k: position first + k of the plane holds a candidate (a number)
__device__ __forceinline__ uint32_t bd_classify(const float* plane, int n, int first)
{
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int i = first + k;
        if (i < n) { const float v = plane[i]; if (v == v) bits |= 1u << k; }
    }
    return bits;
}

// blk[b]: the candidates among block b's 2048 consecutive plane positions
__global__ void __launch_bounds__(256) k_bd_count(const float* plane, int n, uint32_t* blk)
{
    __shared__ uint32_t s_sum;
    const int t = threadIdx.x;
    if (t == 0) s_sum = 0;
    __syncthreads();
    const uint32_t bits = bd_classify(plane, n, blockIdx.x * BD_CHUNK + t * 8);
    if (bits) atomicAdd(&s_sum, (uint32_t)__popc(bits));       // (a sum of integers: the arrival order cannot show)
    __syncthreads();
    if (t == 0) blk[blockIdx.x] = s_sum;
}

// cand[c]: the plane position of candidate c, c < 8192 -- the counts in front of a block and a scan inside it give every candidate its place (k_rpn_compact's
// pattern: no atomics that could show, a fixed layout); the last block leaves K in ktot[0]
__global__ void __launch_bounds__(256) k_bd_compact(const float* plane, int n, const uint32_t* blk, uint32_t* cand, int32_t* ktot)
{
    __shared__ uint32_t s_before, s_w[4];
    const int t = threadIdx.x, b = blockIdx.x;
    block_sum_before<1>(blk, 0, b, &s_before);
    const uint32_t bits = bd_classify(plane, n, b * BD_CHUNK + t * 8);
    uint32_t pos = block_excl_scan<4, uint32_t>((uint32_t)__popc(bits), s_w, nullptr);
    pos += s_before;                                   // (behind the scan's barrier: the sum is complete)
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (bits & (1u << k)) { if (pos < (uint32_t)NMS_MAX) cand[pos] = (uint32_t)(b * BD_CHUNK + t * 8 + k); pos++; }
    if (b == (int)gridDim.x - 1 && t == 255) ktot[0] = (int32_t)pos;      // (the last thread of the last block: everything in front of it and its own)
}

struct BdArgs {
    const float *plane, *reg, *prop;                   // [(C-1)][R], [R][4 Creg], [R][4]
    const uint32_t* cand;
    const int32_t* ktot;
    int R, C, Creg, n;                                 // n = (C - 1) R plane positions
    BoxCode q;
    float4* sboxes; int32_t* sgroups; float* sscore; int32_t* spos; int32_t* srow;
};

// One block: the K <= 8192 candidates into ifx_nms's order (k_nms_sort's network on (score, candidate position)), then per sorted row the decode of the class's
// code against the row's proposal and the clip.  Above the cap nothing is done: k_bd_reduce reports it.
__global__ void __launch_bounds__(1024) k_bd_sort_decode(const BdArgs a)
{
    __shared__ unsigned long long s_key[NMS_MAX];
    const int t = threadIdx.x, K = a.ktot[0];
    if (K > NMS_MAX) return;
    int P = 2;
    while (P < K) P <<= 1;
    for (int i = t; i < P; i += 1024) {
        unsigned long long key = ~0ull;
        if (i < K) { const uint32_t f = a.cand[i]; if (f < (uint32_t)a.n) key = nms_key(a.plane[f], i); }
        s_key[i] = key;
    }
    nms_bitonic(s_key, P, t);
    for (int c = t; c < K; c += 1024) {
        const uint32_t i = (uint32_t)s_key[c];
        const uint32_t f = i < (uint32_t)K ? a.cand[i] : 0xFFFFFFFFu;
        if (f >= (uint32_t)a.n) {                          // (cannot happen: every key holds a candidate; the test keeps the gathers inside the inputs whatever the keys are)
            a.sboxes[c] = make_float4(0.f, 0.f, 0.f, 0.f); a.sgroups[c] = -1 - c; a.sscore[c] = 0.f; a.spos[c] = 0; a.srow[c] = 0;
            continue;
        }
        const int j = (int)(f / (uint32_t)a.R) + 1, r = (int)(f - (uint32_t)(j - 1) * (uint32_t)a.R);
        const float* code = a.reg + (size_t)r * 4 * a.Creg + (a.Creg == 1 ? 0 : 4 * j);
        const float4 b = make_float4(a.prop[4 * (size_t)r], a.prop[4 * (size_t)r + 1], a.prop[4 * (size_t)r + 2], a.prop[4 * (size_t)r + 3]);
        a.sboxes[c] = box_decode_one(b, code[0], code[1], code[2], code[3], a.q);
        a.sgroups[c] = j;
        a.sscore[c] = a.plane[f];
        a.spos[c] = (int32_t)i;
        a.srow[c] = r;
    }
}

struct BdOut {
    float* boxes; float* scores; long long* labels; long long* index; int32_t* count; int32_t* stats;
    int max_out, limit;
};

// One block: the walk over all candidates, the limit, the output in candidate order.  t, the M-th largest kept score, is the score of the M-th kept row -- the rows
// are already in descending score; every kept row with score >= t stays.  The kept flags move from the sorted rows to the candidate positions, a scan over those
// gives each detection its place.
__global__ void __launch_bounds__(1024) k_bd_reduce(const unsigned long long* mask, const float4* sboxes, const int32_t* sgroups, const float* sscore, const int32_t* spos,
                                                    const int32_t* srow, const int32_t* ktot, int nb, const BdOut o)
{
    __shared__ NmsWalk s;
    __shared__ uint8_t s_stay[NMS_MAX];
    __shared__ uint16_t s_rowof[NMS_MAX];
    __shared__ float s_t;
    const int t = threadIdx.x, K = ktot[0];
    const bool over = K > NMS_MAX;
    const int n = over ? 0 : K;
    nms_walk(mask, nullptr, n, nb, 0x7FFFFFFF, s);
    uint32_t bits;
    int pos, total;
    nms_flag_scan(s, s.flag, n, bits, pos, total);           // by sorted row; total = D
    const int D = total;
    const bool cut = o.limit > 0 && D > o.limit;
    if (cut)
        for (int k = 0; k < 8; k++)
            if (bits & (1u << k)) { if (pos == o.limit - 1) s_t = sscore[t * 8 + k]; pos++; }
    for (int i = t; i < n; i += 1024) s_stay[i] = 0;
    __syncthreads();
    const float thr = cut ? s_t : 0.f;
    for (int row = t; row < n; row += 1024) {
        const int i = spos[row];
        if ((uint32_t)i >= (uint32_t)n) continue;          // (a candidate position: always inside)
        s_rowof[i] = (uint16_t)row;
        if (s.flag[row] && (!cut || sscore[row] >= thr)) s_stay[i] = 1;
    }
    __syncthreads();                                         // (with the one above: between the two scans through s.wsum)
    nms_flag_scan(s, s_stay, n, bits, pos, total);           // by candidate position
    for (int k = 0; k < 8; k++)
        if (bits & (1u << k)) {
            if (pos < o.max_out) {
                const int row = s_rowof[t * 8 + k];
                const float4 b = sboxes[row];
                o.boxes[4 * pos] = b.x; o.boxes[4 * pos + 1] = b.y; o.boxes[4 * pos + 2] = b.z; o.boxes[4 * pos + 3] = b.w;
                if (o.scores) o.scores[pos] = sscore[row];
                if (o.labels) o.labels[pos] = sgroups[row];
                if (o.index) o.index[pos] = srow[row];
            }
            pos++;
        }
    for (int i = min(total, o.max_out) + t; i < o.max_out; i += 1024) {
        o.boxes[4 * i] = 0.f; o.boxes[4 * i + 1] = 0.f; o.boxes[4 * i + 2] = 0.f; o.boxes[4 * i + 3] = 0.f;
        if (o.scores) o.scores[i] = 0.f;
        if (o.labels) o.labels[i] = -1;
        if (o.index) o.index[i] = -1;
    }
    if (t == 0) {
        o.count[0] = over ? -1 : total;
        if (o.stats) { o.stats[0] = K; o.stats[1] = D; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------------------
// The mask head's logits to ROI masks, boxes and class ids: ifx_mask_head_select (MaskPostProcessor.forward, maskrcnn_benchmark/modeling/roi_heads/mask_head/
// inference.py:27-61; BoxList.resize, structures/bounding_box.py:91-127; COCODemo.select_top_predictions, demo/predictor.py:224-243; the rule in full:
// include/ifx_c_api.h, in numpy: tests/mask_head_numpy.py).  Two launches; the number of kept rows stays on the device.
constexpr int MH_MAX_R = 1024;         // one thread of the select block per row
constexpr int MH_MAX_C = 1024;
constexpr int MH_MAX_M = 64;

struct MhArgs {
    const float *logits, *boxes, *scores;              // [R][C][M][M], [R][4], [R]
    const long long* labels;                           // [R]
    const int32_t *count, *class_map;                  // one int32 or NULL, [C] or NULL
    int R, C, MM, sort, P;                             // P: the power of two >= max(R, 2) the sort network runs on
    float thresh, rw, rh;
    float *masks, *boxes_out;                          // [R][M][M], [R][4]
    int32_t *class_ids, *rows, *kept;                  // [R], [R] or NULL, one
};

// One block, thread t on input row t and then on output row t.  The kept flags go through the block scan: its total is `kept`, and without the sort its
// exclusive sum is the row's place (a stable compaction).  With the sort the kept rows' keys (nms_key on (score, row)) and ~0 for every other thread go through
// ifx_nms's network; no key of a row equals ~0 (the low word is a row < 1024), so the first `kept` keys are the kept rows in the rule's order.
// The input row of output row k also goes into the first word of mask k (-1 behind kept): k_mh_sigmoid reads it there, whether or not the caller wants d_rows.
__global__ void __launch_bounds__(1024) k_mh_select(const MhArgs a)
{
    __shared__ unsigned long long s_key[MH_MAX_R];
    __shared__ int s_row[MH_MAX_R];
    __shared__ int s_w[16];
    const int t = threadIdx.x;
    int valid = a.R;
    if (a.count) { const int c = a.count[0]; valid = min(max(c, 0), a.R); }
    bool keep = false;
    float s = 0.f;
    if (t < valid) {
        s = a.scores[t];
        const long long lab = a.labels[t];
        keep = (a.thresh == -INFINITY || s > a.thresh) && lab >= 0 && lab < (long long)a.C;
    }
    int kept;
    const int pos = block_excl_scan<16, int>(keep ? 1 : 0, s_w, &kept);
    if (a.sort) {
        s_key[t] = keep ? nms_key(s, t) : ~0ull;
        nms_bitonic(s_key, a.P, t);                                 // (rows and kept keys are below R <= P; every key from R on is ~0)
        s_row[t] = (int)(uint32_t)s_key[t] & (MH_MAX_R - 1);       // (a row, whatever the key: the gathers below stay inside the inputs)
    } else if (keep) s_row[pos] = t;
    __syncthreads();
    if (t == 0) a.kept[0] = kept;
    if (t >= a.R) return;
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    int cls = -1, row = -1;
    if (t < kept) {
        row = min(s_row[t], a.R - 1);
        const int lab = (int)a.labels[row];                          // (0 .. C - 1: the row was kept)
        cls = a.class_map ? a.class_map[min(max(lab, 0), a.C - 1)] : lab;
        const float* q = a.boxes + 4 * (size_t)row;
        b = make_float4(q[0] * a.rw, q[1] * a.rh, q[2] * a.rw, q[3] * a.rh);
    }
    float* o = a.boxes_out + 4 * (size_t)t;
    o[0] = b.x; o[1] = b.y; o[2] = b.z; o[3] = b.w;
    a.class_ids[t] = cls;
    if (a.rows) a.rows[t] = row;
    a.masks[(size_t)t * a.MM] = __int_as_float(row);
}

// Block k: the M^2 probabilities of output row k out of the one channel the row's label names -- SIGMOID of the rule, three f32 steps behind the library's EXP --
// or M^2 zeros behind kept.  Consecutive threads on consecutive samples: the channel is contiguous in the input, the mask in the output.
__global__ void __launch_bounds__(256) k_mh_sigmoid(const MhArgs a)
{
    __shared__ int s_src;
    const int t = threadIdx.x, k = blockIdx.x;
    float* out = a.masks + (size_t)k * a.MM;
    if (t == 0) s_src = __float_as_int(out[0]);
    __syncthreads();                                                 // (every thread has the row before the first sample is overwritten)
    const int row = s_src;
    long long lab = -1;
    if (row >= 0 && row < a.R) lab = a.labels[row];
    if (lab < 0 || lab >= (long long)a.C) {
        for (int i = t; i < a.MM; i += 256) out[i] = 0.f;
        return;
    }
    const float* x = a.logits + ((size_t)row * a.C + (size_t)lab) * a.MM;
    for (int i = t; i < a.MM; i += 256) {
        const float e = rpn_exp(-x[i]);
        const float d = 1.0f + e;
        out[i] = 1.0f / d;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------------------
// The reference's default detector: detections [R,6] and mrcnn_mask to image-sized 0 / 1 masks, boxes and class ids: ifx_unmold_detections
// (MaskRCNN.unmold_detections, deps/mask_rcnn/model.py:2285-2344; utils.unmold_mask, deps/mask_rcnn/utils.py:490-507, behind scipy.misc.imresize; the rule in full:
// include/ifx_c_api.h, in numpy: tests/unmold_numpy.py).  Two launches around one memset; the number of kept rows stays on the device.
constexpr int UM_TX = 64;                     // the columns of the frame a paste block owns
constexpr int UM_KS = MH_MAX_M + 1;           // the stride of a tap row in LDS: first >= 0 and first + count <= M, so at most M <= 64 taps reach a sample
constexpr double UM_LIMIT = 16777216.0;       // +-2^24: a coordinate beyond it has no defined box

struct UmArgs {
    const float *det, *masks;                         // [R][6]; [R][M][M][C] or (nchw) [R][C][M][M]
    const int32_t* class_map;                         // [C] or NULL
    int R, M, C, nchw, W, H, wy1, wx1;
    double scale;
    uint8_t* out;                                     // [R][H * W]
    int32_t *class_ids, *boxes, *rows, *kept;         // [R], [R][4], [R] or NULL, one
    float* scores;                                    // [R] or NULL
};

// Steps 2, 3 and the row's share of step 8, the ONE statement of them for the select block and for the paste blocks.
struct UmRow { int y1, x1, y2, x2, c; bool survives, defined, valid; };
__device__ __forceinline__ UmRow um_row(const UmArgs& a, int r)
{
    const float* d = a.det + 6 * (size_t)r;
    double v[4];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float x = d[k];
        v[k] = ((double)x - (double)((k & 1) ? a.wx1 : a.wy1)) * a.scale;
        ok = ok && fabsf(x) <= (float)UM_LIMIT && fabs(v[k]) <= UM_LIMIT;     // (a NaN or an infinity compares false)
    }
    UmRow o;
    o.y1 = o.x1 = o.y2 = o.x2 = 0; o.survives = true; o.defined = false;
    if (ok) {
        o.y1 = (int)v[0]; o.x1 = (int)v[1]; o.y2 = (int)v[2]; o.x2 = (int)v[3];                 // toward zero, as astype(int32)
        o.survives = (long long)(o.y2 - o.y1) * (long long)(o.x2 - o.x1) > 0;
        o.defined = 0 <= o.y1 && o.y1 < o.y2 && o.y2 <= a.H && 0 <= o.x1 && o.x1 < o.x2 && o.x2 <= a.W;
    }
    const float cid = d[4];
    o.valid = cid >= 1.f && cid < (float)a.C;                                                   // (a NaN compares false)
    o.c = o.valid ? (int)cid : 0;
    o.defined = o.defined && o.valid;
    return o;
}

// One block, thread t on input row t: step 1 through an LDS minimum, steps 2 and 3, the block scan -- its total is `kept`, its exclusive sum the row's place (a
// stable compaction) -- and the scatter of the record; threads kept .. R - 1 write the padding.
__global__ void __launch_bounds__(1024) k_unmold_select(const UmArgs a)
{
    __shared__ int s_w[16];
    __shared__ int s_n;
    const int t = threadIdx.x;
    if (t == 0) s_n = a.R;
    __syncthreads();
    if (t < a.R && a.det[6 * (size_t)t + 4] == 0.f) atomicMin(&s_n, t);
    __syncthreads();
    UmRow row;
    bool keep = false;
    if (t < s_n) { row = um_row(a, t); keep = row.survives; }
    int kept;
    const int pos = block_excl_scan<16, int>(keep ? 1 : 0, s_w, &kept);
    if (keep) {
        int32_t* b = a.boxes + 4 * (size_t)pos;
        b[0] = row.y1; b[1] = row.x1; b[2] = row.y2; b[3] = row.x2;
        a.class_ids[pos] = row.valid ? (a.class_map ? a.class_map[row.c] : row.c) : 0;
        if (a.scores) a.scores[pos] = a.det[6 * (size_t)t + 5];
        if (a.rows) a.rows[pos] = t;
    }
    if (t >= kept && t < a.R) {
        int32_t* b = a.boxes + 4 * (size_t)t;
        b[0] = 0; b[1] = 0; b[2] = 0; b[3] = 0;
        a.class_ids[t] = -1;
        if (a.scores) a.scores[t] = 0.f;
        if (a.rows) a.rows[t] = -1;
    }
    if (t == 0) a.kept[0] = kept;
}

// Pillow's taps of output sample xx of one axis (precompute_coeffs / normalize_coeffs_8bpc, the bilinear filter): ifx_detprep::resize_taps' arithmetic, statement
// for statement, in f64 -- true divisions, no reciprocal instruction, nothing fused; the weights are summed in index order and made a second time for the division
// instead of being kept.  k: count <= in <= 64 taps.
__device__ void um_taps(int in, int out, int xx, int* k, int* first, int* count)
{
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = fs, ss = 1.0 / fs;
    const double center = ((double)xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    const int n = min(max(xmax - xmin, 0), in);
    double ww = 0.0;
    for (int x = 0; x < n; x++) {
        double w = ((double)(x + xmin) - center + 0.5) * ss;
        if (w < 0.0) w = -w;
        ww += w < 1.0 ? 1.0 - w : 0.0;
    }
    for (int x = 0; x < n; x++) {
        double w = ((double)(x + xmin) - center + 0.5) * ss;
        if (w < 0.0) w = -w;
        w = w < 1.0 ? 1.0 - w : 0.0;
        const double v = (ww != 0.0 ? w / ww : w) * (double)(1 << ifx_detprep::PRECISION_BITS);
        k[x] = v < 0.0 ? (int)(-0.5 + v) : (int)(0.5 + v);
    }
    *first = min(xmin, in - n);
    *count = n;
}

// Block (bx, k): the 64 columns of the frame from 64 bx on, output row k.  Thread t owns input rows 4t .. 4t + 3 in the scan that finds the k-th surviving row
// (k_unmold_select's count, test and scan); the block leaves when k >= kept, when the paste is not defined (step 8) or when the box misses its columns -- every
// one of these is the same for all its threads, and no barrier follows a return that is not.  Then: min / max of the row's channel (shuffles, four wave results
// in LDS), the M^2 bytes of step 4, the horizontal taps (thread c < 64 those of column c), the horizontal pass into s_mid [M][64] bytes, and per chunk of 64
// box rows the vertical taps (thread j < 64 those of row j) and the vertical pass: lane = column, a wave's rows four apart, consecutive lanes storing
// consecutive x.  An axis that keeps the size M gets the tap (2^22), the same bytes.  Sums: every weight is >= 0 and a sample's taps add up to 2^22 give or take
// half a unit per tap: 2^21 + 255 * (2^22 + 32) < 2^31, exact in 32-bit unsigned accumulators (k_detector_input's bound).
// Bounds: a pixel is stored only for a defined paste, 0 <= y1 < y2 <= H and 0 <= x1 < x2 <= W, at y1 + j < y2 and x1 <= x < x2; LDS reads stay below first + count <= M.
__global__ void __launch_bounds__(256) k_unmold_paste(const UmArgs a)
{
    __shared__ int s_w[4];
    __shared__ int s_n, s_src, s_bad;
    __shared__ float s_mn[4], s_mx[4];
    __shared__ int s_kx[UM_TX * UM_KS], s_ky[UM_TX * UM_KS];
    __shared__ int s_fx[UM_TX], s_cx[UM_TX], s_fy[UM_TX], s_cy[UM_TX];
    __shared__ uint8_t s_byte[MH_MAX_M * MH_MAX_M], s_mid[MH_MAX_M * UM_TX];
    const int t = threadIdx.x, k = blockIdx.y, x0 = blockIdx.x * UM_TX;
    if (t == 0) { s_n = a.R; s_src = -1; s_bad = 0; }
    __syncthreads();
    for (int i = 0; i < 4; i++) {
        const int r = 4 * t + i;
        if (r < a.R && a.det[6 * (size_t)r + 4] == 0.f) { atomicMin(&s_n, r); break; }
    }
    __syncthreads();
    const int N = s_n;
    bool kp[4];
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int r = 4 * t + i;
        kp[i] = r < N && um_row(a, r).survives;
        cnt += kp[i] ? 1 : 0;
    }
    int kept;
    int pos = block_excl_scan<4, int>(cnt, s_w, &kept);
    if (k >= kept) return;
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (kp[i]) { if (pos == k) s_src = 4 * t + i; pos++; }
    __syncthreads();
    const int src = s_src;
    if (src < 0 || src >= a.R) return;
    const UmRow row = um_row(a, src);
    const int xa = max(row.x1, x0), xb = min(row.x2, x0 + UM_TX);
    if (!row.defined || xa >= xb) return;

    const int M = a.M, MM = M * M;
    const float* ch = a.nchw ? a.masks + ((size_t)src * a.C + row.c) * MM : a.masks + (size_t)src * MM * a.C + row.c;
    const size_t step = a.nchw ? 1 : (size_t)a.C;
    float mn = INFINITY, mx = -INFINITY;
    bool bad = false;
    for (int i = t; i < MM; i += 256) {
        const float v = ch[i * step];
        bad = bad || !(fabsf(v) <= 3.402823466e+38f);
        mn = fminf(mn, v); mx = fmaxf(mx, v);
    }
    for (int d = 32; d >= 1; d >>= 1) { mn = fminf(mn, __shfl_xor(mn, d)); mx = fmaxf(mx, __shfl_xor(mx, d)); }
    if ((t & 63) == 0) { s_mn[t >> 6] = mn; s_mx[t >> 6] = mx; }
    if (bad) s_bad = 1;
    __syncthreads();
    const float cmin = fminf(fminf(s_mn[0], s_mn[1]), fminf(s_mn[2], s_mn[3])), cmax = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
    float cs = cmax - cmin;
    if (cs == 0.f) cs = 1.f;
    const float s = (float)(255.0 / (double)cs);
    if (s_bad || !(fabsf(cs) <= 3.402823466e+38f) || !(fabsf(s) <= 3.402823466e+38f)) return;
    for (int i = t; i < MM; i += 256) {
        const float d = ch[i * step] - cmin;
        const float q = fminf(fmaxf(d * s, 0.f), 255.f) + 0.5f;
        s_byte[i] = (uint8_t)(int)q;
    }
    const int bw = row.x2 - row.x1, bh = row.y2 - row.y1;
    if (t < UM_TX) {
        const int x = x0 + t;
        s_cx[t] = 0;
        if (x >= xa && x < xb) {
            if (bw == M) { s_fx[t] = x - row.x1; s_cx[t] = 1; s_kx[t * UM_KS] = 1 << ifx_detprep::PRECISION_BITS; }
            else um_taps(M, bw, x - row.x1, s_kx + t * UM_KS, &s_fx[t], &s_cx[t]);
        }
    }
    __syncthreads();
    const int col = t & 63, nxc = s_cx[col], fxc = s_fx[col];
    if (nxc > 0)
        for (int y = t >> 6; y < M; y += 4) {
            uint32_t q = DI_HALF;
            for (int i = 0; i < nxc; i++) q += s_byte[y * M + fxc + i] * (uint32_t)s_kx[col * UM_KS + i];
            s_mid[y * UM_TX + col] = (uint8_t)min(q >> ifx_detprep::PRECISION_BITS, 255u);
        }
    uint8_t* out = a.out + (size_t)k * a.H * a.W;
    for (int j0 = 0; j0 < bh; j0 += UM_TX) {
        __syncthreads();                                             // s_mid is complete; the previous chunk's readers are done with s_ky
        if (t < UM_TX && j0 + t < bh) {
            if (bh == M) { s_fy[t] = j0 + t; s_cy[t] = 1; s_ky[t * UM_KS] = 1 << ifx_detprep::PRECISION_BITS; }
            else um_taps(M, bh, j0 + t, s_ky + t * UM_KS, &s_fy[t], &s_cy[t]);
        }
        __syncthreads();
        const int nj = min(UM_TX, bh - j0);
        if (nxc > 0)
            for (int j = t >> 6; j < nj; j += 4) {
                const int f = s_fy[j], n = s_cy[j];
                uint32_t q = DI_HALF;
                for (int i = 0; i < n; i++) q += s_mid[(f + i) * UM_TX + col] * (uint32_t)s_ky[j * UM_KS + i];
                out[(size_t)(row.y1 + j0 + j) * a.W + x0 + col] = (q >> ifx_detprep::PRECISION_BITS) >= 128u ? 1 : 0;
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------------------
// The Keras Mask R-CNN's three layers that are no convolutions (deps/mask_rcnn/model.py): ifx_keras_proposals (ProposalLayer.call, :227-311), ifx_pyramid_roi_align
// (PyramidROIAlign.call, :323-424) and ifx_keras_detections (refine_detections_graph, :670-771).  The rules in full: include/ifx_c_api.h, in numpy:
// tests/keras_layers_numpy.py.  Boxes are y1, x1, y2, x2 with the far corner outside; the selection, the sort, the pair mask (its TF form) and the walk are the
// machinery above.
constexpr int KP_STRIDE = 2;           // rpn_probs [n][2]: the foreground score is every second float, read in place

__global__ void __launch_bounds__(256) k_kp_count(const float* score, int n, const uint32_t* hist, uint32_t* state, uint32_t* blk, int nblk)
{
    rpn_count_block<KP_STRIDE>(score, n, 1, 1, hist, state, blk, nblk);
}

__global__ void __launch_bounds__(256) k_kp_compact(const float* score, int n, uint32_t K, const uint32_t* state, const uint32_t* blk, int nblk, unsigned long long* cand)
{
    rpn_compact_block<KP_STRIDE>(score, n, 1, 1, K, state, blk, nblk, cand);
}

// apply_box_deltas_graph (model.py:185-206), operation for operation; b and the result are y1, x1, y2, x2 in .x .y .z .w
__device__ __forceinline__ float4 keras_decode(const float4 b, float d0, float d1, float d2, float d3)
{
    float h = b.z - b.x, w = b.w - b.y;
    float cy = b.x + 0.5f * h, cx = b.y + 0.5f * w;
    cy = cy + d0 * h;
    cx = cx + d1 * w;
    h = h * rpn_exp(d2);
    w = w * rpn_exp(d3);
    const float y1 = cy - 0.5f * h, x1 = cx - 0.5f * w;
    return make_float4(y1, x1, y1 + h, x1 + w);
}

// clip_boxes_graph's max(min(v, hi), lo) (model.py:209-224); a NaN stays a NaN
__device__ __forceinline__ float keras_clip(float v, float lo, float hi)
{
    v = v > hi ? hi : v;
    return v < lo ? lo : v;
}

struct KpArgs {
    const float *score, *bbox, *anc;                   // probs + 1 (KP_STRIDE apart), [n][4], [n][4] pixels
    const unsigned long long* cand;                    // the selection's winners, NULL: every anchor is a candidate (n <= 8192)
    int n, m, P;                                       // m = min(pre_nms_limit, n), P = 2^k >= the keys sorted
    float sd0, sd1, sd2, sd3, ih, iw;
    float4* sboxes; int32_t* sindex; int32_t* ns;
};

// One block: the candidates into the order (k_nms_sort's network), then per sorted row the deltas times the std-dev vector, the decode, the clip to the image and
// the division by its size.  Every candidate stays (the layer has no small-box filter): ns = m.
__global__ void __launch_bounds__(1024) k_kp_sort_decode(const KpArgs a)
{
    __shared__ unsigned long long s_key[NMS_MAX];
    const int t = threadIdx.x;
    if (a.cand) for (int i = t; i < a.P; i += 1024) s_key[i] = i < a.m ? a.cand[i] : ~0ull;
    else for (int i = t; i < a.P; i += 1024) s_key[i] = i < a.n ? nms_key(a.score[(size_t)i * KP_STRIDE], i) : ~0ull;
    nms_bitonic(s_key, a.P, t);
    for (int c = t; c < a.m; c += 1024) {
        const uint32_t i = (uint32_t)s_key[c];
        if (i >= (uint32_t)a.n) {                      // (cannot happen: every key holds an anchor index; the test keeps the gathers inside the inputs whatever the keys are)
            a.sboxes[c] = make_float4(0.f, 0.f, 0.f, 0.f); a.sindex[c] = -1;
            continue;
        }
        const float* an = a.anc + 4 * (size_t)i;
        const float* d = a.bbox + 4 * (size_t)i;
        float4 b = keras_decode(make_float4(an[0], an[1], an[2], an[3]), d[0] * a.sd0, d[1] * a.sd1, d[2] * a.sd2, d[3] * a.sd3);
        b.x = keras_clip(b.x, 0.f, a.ih) / a.ih;
        b.y = keras_clip(b.y, 0.f, a.iw) / a.iw;
        b.z = keras_clip(b.z, 0.f, a.ih) / a.ih;
        b.w = keras_clip(b.w, 0.f, a.iw) / a.iw;
        a.sboxes[c] = b;
        a.sindex[c] = (int32_t)i;
    }
    if (t == 0) a.ns[0] = a.m;
}

// ---- ifx_pyramid_roi_align: all levels and rows in one launch.  A block owns one box and PRA_UNITS of its outputs; it finds the box's level by three compares
// against thresholds made on the host, fills the two axis tables (one entry per output row / column: the two texels and the weight of tf.image.crop_and_resize's
// bilinear sample) in LDS and then only gathers and blends.
constexpr int PRA_TAB = 128;           // pool_h, pool_w at the most
constexpr int PRA_UNITS = 4096;        // outputs (16-byte groups of them in the vector form) of a block: sixteen per thread

struct PraAxis { int lo, hi; float l; };               // lo < 0: outside the map, the output is 0

__device__ __forceinline__ PraAxis pra_axis(float a1, float a2, int i, int pool, int size)
{
    const float sm1 = (float)(size - 1);
    float in;
    if (pool > 1) { const float scale = ((a2 - a1) * sm1) / (float)(pool - 1); in = a1 * sm1 + (float)i * scale; }
    else in = (0.5f * (a1 + a2)) * sm1;
    PraAxis s;
    if (!(in >= 0.f && in <= sm1)) { s.lo = -1; s.hi = 0; s.l = 0.f; return s; }     // (a NaN too)
    const float top = floorf(in);
    s.lo = (int)top; s.hi = (int)ceilf(in); s.l = in - top;                           // both inside 0 .. size - 1
    return s;
}

struct PraArgs {
    const float* in[4];                // P2 .. P5: [batch][C][H_l][W_l] or [batch][H_l][W_l][C]
    int height[4], width[4];
    float thr[3];
    const float* boxes;                // [batch n][4] normalised y1, x1, y2, x2
    float* out;                        // [batch n][C][ph][pw] or [batch n][ph][pw][C]
    int32_t* lev_out;                  // NULL or [batch n]
    int n, channels, ph, pw, chunks;
};

__device__ __forceinline__ float pra_blend(float tl, float tr, float bl, float br, float lx, float ly)
{
    const float top = tl + (tr - tl) * lx, bot = bl + (br - bl) * lx;
    return top + (bot - top) * ly;
}

// MODE 0: NCHW, consecutive lanes on consecutive output columns of a channel plane; 1: NHWC, the lanes along C; 2: NHWC, four channels per lane in 16-byte words
template <int MODE>
__global__ void __launch_bounds__(256) k_pyramid_roi_align(const PraArgs a)
{
    __shared__ PraAxis s_y[PRA_TAB], s_x[PRA_TAB];
    const int t = threadIdx.x;
    const int row = blockIdx.x / a.chunks, chunk = blockIdx.x - row * a.chunks;
    const float* bx = a.boxes + 4 * (size_t)row;
    const float y1 = bx[0], x1 = bx[1], y2 = bx[2], x2 = bx[3];
    const float s = sqrtf((y2 - y1) * (x2 - x1));
    const int lv = (s > a.thr[0] ? 1 : 0) + (s >= a.thr[1] ? 1 : 0) + (s > a.thr[2] ? 1 : 0);        // s zero or NaN: 0, the reference's clamp
    if (chunk == 0 && t == 0 && a.lev_out) a.lev_out[row] = 2 + lv;
    const int H = lv == 0 ? a.height[0] : lv == 1 ? a.height[1] : lv == 2 ? a.height[2] : a.height[3];
    const int W = lv == 0 ? a.width[0] : lv == 1 ? a.width[1] : lv == 2 ? a.width[2] : a.width[3];
    const float* map = lv == 0 ? a.in[0] : lv == 1 ? a.in[1] : lv == 2 ? a.in[2] : a.in[3];
    for (int i = t; i < a.ph; i += 256) s_y[i] = pra_axis(y1, y2, i, a.ph, H);
    for (int i = t; i < a.pw; i += 256) s_x[i] = pra_axis(x1, x2, i, a.pw, W);
    __syncthreads();
    const int C = a.channels, bins = a.ph * a.pw;
    const float* img = map + (size_t)(row / a.n) * C * ((size_t)H * W);
    float* out = a.out + (size_t)row * C * bins;
    const int units = MODE == 2 ? bins * (C >> 2) : bins * C;
    const int end = min(units, (chunk + 1) * PRA_UNITS);
    for (int o = chunk * PRA_UNITS + t; o < end; o += 256) {
        if (MODE == 0) {
            const int c = o / bins, bin = o - c * bins, py = bin / a.pw, px = bin - py * a.pw;
            const PraAxis y = s_y[py], x = s_x[px];
            float v = 0.f;
            if (y.lo >= 0 && x.lo >= 0) {
                const float *r0 = img + ((size_t)c * H + y.lo) * W, *r1 = img + ((size_t)c * H + y.hi) * W;
                v = pra_blend(r0[x.lo], r0[x.hi], r1[x.lo], r1[x.hi], x.l, y.l);
            }
            out[o] = v;
        } else {
            const int cg = MODE == 2 ? C >> 2 : C;
            const int bin = o / cg, c = o - bin * cg, py = bin / a.pw, px = bin - py * a.pw;
            const PraAxis y = s_y[py], x = s_x[px];
            const bool inside = y.lo >= 0 && x.lo >= 0;
            const size_t tl = ((size_t)y.lo * W + x.lo) * C, tr = ((size_t)y.lo * W + x.hi) * C, bl = ((size_t)y.hi * W + x.lo) * C, br = ((size_t)y.hi * W + x.hi) * C;
            if (MODE == 2) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (inside) {
                    const float4 q0 = *(const float4*)(img + tl + 4 * c), q1 = *(const float4*)(img + tr + 4 * c);
                    const float4 q2 = *(const float4*)(img + bl + 4 * c), q3 = *(const float4*)(img + br + 4 * c);
                    v.x = pra_blend(q0.x, q1.x, q2.x, q3.x, x.l, y.l);
                    v.y = pra_blend(q0.y, q1.y, q2.y, q3.y, x.l, y.l);
                    v.z = pra_blend(q0.z, q1.z, q2.z, q3.z, x.l, y.l);
                    v.w = pra_blend(q0.w, q1.w, q2.w, q3.w, x.l, y.l);
                }
                *(float4*)(out + 4 * (size_t)o) = v;
            } else {
                float v = 0.f;
                if (inside) v = pra_blend(img[tl + c], img[tr + c], img[bl + c], img[br + c], x.l, y.l);
                out[o] = v;
            }
        }
    }
}

// ---- ifx_keras_detections.  k_kd_rows, one wave per ROI row: the first maximum of the row's probabilities, the class's deltas, decode, image scale, window clip,
// rint; the row's record and its sort key (~0: the row is dropped).
struct KdArgs {
    const float *rois, *probs, *deltas;                // [R][4], [R][C], [R][C][4]
    int R, C, P;
    float sd0, sd1, sd2, sd3, minconf, ih, iw, wy1, wx1, wy2, wx2;
    unsigned long long* keys;                          // [R]
    float4* rbox; int32_t* rcls; float* rscore;        // per ROI row
    float4* sboxes; int32_t* sgroups; float* sscore; int32_t* srow; int32_t* ns;     // per sorted row
};

__global__ void __launch_bounds__(256) k_kd_rows(const KdArgs a)
{
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const float* p = a.probs + (size_t)r * a.C;
    // the sequential rule (best = 0; p[j] > p[best]: best = j) is: class 0 when p[0] is a NaN, else the lowest index of the largest number (a NaN never compares greater)
    float bv = -INFINITY;
    int bi = 0x7FFFFFFF;
    for (int j = lane; j < a.C; j += 64) { const float v = p[j]; if (v > bv || (v == bv && j < bi)) { bv = v; bi = j; } }
    for (int d = 32; d > 0; d >>= 1) {
        const float ov = __shfl_xor(bv, d);
        const int oi = __shfl_xor(bi, d);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    const float p0 = p[0];
    const int cls = (p0 != p0 || bi >= a.C) ? 0 : bi;   // (no number in the row: p[0] is a NaN)
    if (lane) return;
    const float score = p[cls];
    const float* d = a.deltas + ((size_t)r * a.C + cls) * 4;
    const float* ro = a.rois + 4 * (size_t)r;
    float4 b = keras_decode(make_float4(ro[0], ro[1], ro[2], ro[3]), d[0] * a.sd0, d[1] * a.sd1, d[2] * a.sd2, d[3] * a.sd3);
    b.x = keras_clip(b.x * a.ih, a.wy1, a.wy2);
    b.y = keras_clip(b.y * a.iw, a.wx1, a.wx2);
    b.z = keras_clip(b.z * a.ih, a.wy1, a.wy2);
    b.w = keras_clip(b.w * a.iw, a.wx1, a.wx2);
    bool keep = b.x == b.x && b.y == b.y && b.z == b.z && b.w == b.w && cls > 0;
    if (a.minconf != 0.f) keep = keep && score >= a.minconf;        // (`if config.DETECTION_MIN_CONFIDENCE:` -- 0 skips the test, and a NaN score then stays, ordered last)
    if (keep) {                                         // tf.to_int32(tf.rint(.)) and back to float: the window bounds the values to +-2^24, -0 becomes +0
        b.x = (float)(int)rintf(b.x); b.y = (float)(int)rintf(b.y); b.z = (float)(int)rintf(b.z); b.w = (float)(int)rintf(b.w);
    } else b = make_float4(0.f, 0.f, 0.f, 0.f);
    a.rbox[r] = b; a.rcls[r] = cls; a.rscore[r] = score;
    a.keys[r] = keep ? nms_key(score, r) : ~0ull;
}

// One block: the rows into the order (score descending, then ascending row; the dropped rows' keys ~0 behind all of them), the records gathered, the number of
// rows that stay
__global__ void __launch_bounds__(1024) k_kd_sort(const KdArgs a)
{
    __shared__ unsigned long long s_key[NMS_MAX];
    const int t = threadIdx.x;
    for (int i = t; i < a.P; i += 1024) s_key[i] = i < a.R ? a.keys[i] : ~0ull;
    nms_bitonic(s_key, a.P, t);
    if (t == 0 && s_key[0] == ~0ull) a.ns[0] = 0;
    for (int c = t; c < a.R; c += 1024) {
        const unsigned long long key = s_key[c];
        if (key == ~0ull) continue;
        if (c + 1 == a.P || s_key[c + 1] == ~0ull) a.ns[0] = c + 1;      // the last row that stays: one thread
        const uint32_t r = (uint32_t)key;
        if (r >= (uint32_t)a.R) { a.sboxes[c] = make_float4(0.f, 0.f, 0.f, 0.f); a.sgroups[c] = -1 - c; a.sscore[c] = 0.f; a.srow[c] = 0; continue; }   // (cannot happen)
        a.sboxes[c] = a.rbox[r]; a.sgroups[c] = a.rcls[r]; a.sscore[c] = a.rscore[r]; a.srow[c] = (int32_t)r;
    }
}

struct KdOut { float* det; float* boxes_norm; long long* index; int32_t* count; int max_inst; float ih, iw; };

// One block: the walk (the class is the pair mask's group: the per-class suppression in one pass), stopped once max_inst rows are kept, and the output.  The
// per-class cap needs no pass of its own: the rows are in descending score, so a row with max_inst kept rows of its own class in front of it has max_inst kept
// rows in front of it -- the cut across the classes drops it, and every row the cap drops lies behind that cut.  The first max_inst kept rows are the layer's output.
__global__ void __launch_bounds__(1024) k_kd_reduce(const unsigned long long* mask, const float4* sboxes, const int32_t* sgroups, const float* sscore, const int32_t* srow,
                                                    const int32_t* ns, int nb, const KdOut o)
{
    __shared__ NmsWalk s;
    const int t = threadIdx.x, n = min(ns[0], NMS_MAX);
    nms_walk(mask, nullptr, n, nb, o.max_inst, s);
    uint32_t bits;
    int pos, total;
    nms_flag_scan(s, s.flag, n, bits, pos, total);           // by sorted row
    for (int k = 0; k < 8; k++)
        if (bits & (1u << k)) {
            if (pos < o.max_inst) {
                const int row = t * 8 + k;
                const float4 b = sboxes[row];
                float* d = o.det + 6 * (size_t)pos;
                d[0] = b.x; d[1] = b.y; d[2] = b.z; d[3] = b.w; d[4] = (float)sgroups[row]; d[5] = sscore[row];
                if (o.boxes_norm) { float* q = o.boxes_norm + 4 * (size_t)pos; q[0] = b.x / o.ih; q[1] = b.y / o.iw; q[2] = b.z / o.ih; q[3] = b.w / o.iw; }
                if (o.index) o.index[pos] = srow[row];
            }
            pos++;
        }
    total = min(total, o.max_inst);
    for (int i = total + t; i < o.max_inst; i += 1024) {
        float* d = o.det + 6 * (size_t)i;
        d[0] = 0.f; d[1] = 0.f; d[2] = 0.f; d[3] = 0.f; d[4] = 0.f; d[5] = 0.f;
        if (o.boxes_norm) { float* q = o.boxes_norm + 4 * (size_t)i; q[0] = 0.f; q[1] = 0.f; q[2] = 0.f; q[3] = 0.f; }
        if (o.index) o.index[i] = -1;
    }
    if (t == 0) o.count[0] = total;
}

// the stream the LAUNCH macro and the kernel timing use, for the length of a call on the caller's stream
struct StreamScope {
    ifx* h; hipStream_t old;
    StreamScope(ifx* hh, hipStream_t s) : h(hh), old(hh->cur) { hh->cur = s; }
    ~StreamScope() { h->cur = old; }
};

// the one scratch buffer of ifx_nms, ifx_rpn_proposals and ifx_box_detections: allocated by the first call, grown on demand (hipFree waits for its readers), and
// ordered across streams by an event
struct DetOps {
    void* buf = nullptr;
    size_t bytes = 0;
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;
    bool used = false;
};

// A bump carver over the scratch: take<T>(count) returns base + offset (NULL while base is NULL: the sizing pass) and advances the offset, which stays a multiple
// of 16 bytes.
struct Carver {
    char* base;
    size_t off = 0;
    template <class T> T* take(size_t count)
    {
        T* p = base ? (T*)(base + off) : nullptr;
        off += (count * sizeof(T) + 15) & ~(size_t)15;
        return p;
    }
};

// The scratch of a call on `stream`, behind the previous call's use of it.  `layout` carves the call's arrays out of a Carver and is the ONE statement of where they
// lie: it runs on a NULL base for the size the buffer must have, then on the buffer, and a second pass that ends beyond the buffer is refused, not run.
template <class F>
int ops_scratch(ifx* h, const char* who, F layout, hipStream_t stream, DetOps** out)
{
    Carver size{nullptr};
    layout(size);
    const size_t bytes = size.off;
    if (!h->det_ops) h->det_ops = new DetOps();
    DetOps* ops = (DetOps*)h->det_ops;
    if (!ops->ev) HIPCHK(h, hipEventCreateWithFlags(&ops->ev, hipEventDisableTiming));
    if (bytes > ops->bytes) {
        if (ops->buf) { hipFree(ops->buf); ops->buf = nullptr; ops->bytes = 0; }
        if (hipMalloc(&ops->buf, bytes) != hipSuccess) { h->err = std::string(who) + ": hipMalloc of the scratch failed"; return IFX_E_HIP; }
        ops->bytes = bytes;
    }
    Carver c{(char*)ops->buf};
    layout(c);
    if (c.off > ops->bytes) { h->err = std::string(who) + ": the scratch layout ends beyond the buffer"; return IFX_E_STATE; }
    if (ops->used && ops->last != stream) HIPCHK(h, hipStreamWaitEvent(stream, ops->ev, 0));   // the previous call may still be using the scratch on its stream
    *out = ops;
    return IFX_OK;
}

// the end of a call that went through: the next call on another stream waits for this event
int ops_done(ifx* h, DetOps* ops, hipStream_t stream)
{
    HIPCHK(h, hipEventRecord(ops->ev, stream));
    ops->used = true;
    ops->last = stream;
    return IFX_OK;
}

int nms_run(ifx* h, const float* d_boxes, const float* d_scores, const int32_t* d_groups, int n, float threshold, int64_t* d_keep, int32_t* d_count, hipStream_t stream)
{
    int cap = 1024;
    while (cap < n) cap <<= 1;
    float4* sboxes; unsigned long long* mask; int32_t *order, *sgroups;
    DetOps* ops = nullptr;
    int r = ops_scratch(h, "ifx_nms", [&](Carver& c) {
        sboxes = c.take<float4>(cap);
        mask = c.take<unsigned long long>((size_t)cap * (cap / 64));
        order = c.take<int32_t>(cap);
        sgroups = c.take<int32_t>(cap);
    }, stream, &ops);
    if (r) return r;
    StreamScope scope(h, stream);
    int P = 2;
    while (P < n) P <<= 1;
    const int nb = cdiv(n, 64);
    LAUNCH(h, "nms_sort", dim3(1), dim3(1024), k_nms_sort, d_boxes, d_scores, d_groups, n, P, order, sboxes, sgroups);
    LAUNCH(h, "nms_mask", dim3((unsigned)nb, (unsigned)nb), dim3(64), k_nms_mask, (const float4*)sboxes, (const int32_t*)sgroups, n, nb, threshold, mask);
    LAUNCH(h, "nms_reduce", dim3(1), dim3(1024), k_nms_reduce, (const unsigned long long*)mask, (const int32_t*)order, n, nb, (long long*)d_keep, d_count);
    return ops_done(h, ops, stream);
}


// The proposal stage's launches.  Scratch, out of the handle's buffer: sorted boxes, mask words, the winners' keys, sorted logits and
// indices, the per-block counts, and -- zeroed by one memset per call -- the three histograms, the selection's state and the survivors' count.
int rpn_run(ifx* h, const float* d_obj, const float* d_reg, const float* d_anc, int A, int HW, const ifx_rpn_params* p, const BoxCode& q, float* d_boxes, float* d_logits,
            int64_t* d_index, int32_t* d_count, hipStream_t stream)
{
    const int n = A * HW, m = std::min(p->pre_nms_top_n, n), mc = cdiv(m, 64) * 64, nb = mc / 64, nblk = cdiv(n, RPN_CHUNK);
    const bool select = n > NMS_MAX;
    const size_t zero_words = 3 * RPN_BINS + 8 + 8;    // histograms, state, the survivors' count (and padding)
    float4* sboxes; unsigned long long *mask, *cand; float* slogit; int32_t* sindex; uint32_t *blk, *hist;
    DetOps* ops = nullptr;
    int r = ops_scratch(h, "ifx_rpn_proposals", [&](Carver& c) {
        sboxes = c.take<float4>(mc);
        mask = c.take<unsigned long long>((size_t)mc * nb);
        cand = c.take<unsigned long long>(mc);
        slogit = c.take<float>(mc);
        sindex = c.take<int32_t>(mc);
        blk = c.take<uint32_t>(2 * (size_t)nblk);
        hist = c.take<uint32_t>(zero_words);           // one take: one memset zeroes the histograms, the state and the count behind them
    }, stream, &ops);
    if (r) return r;
    uint32_t* state = hist + 3 * RPN_BINS;
    int32_t* ns = (int32_t*)(state + 8);
    StreamScope scope(h, stream);
    const uint32_t K = (uint32_t)m;
    if (select) {
        HIPCHK(h, hipMemsetAsync(hist, 0, zero_words * 4, stream));
        LAUNCH(h, "rpn_hist", dim3((unsigned)nblk), dim3(256), k_rpn_hist<0>, d_obj, n, K, hist, state);
        LAUNCH(h, "rpn_hist", dim3((unsigned)nblk), dim3(256), k_rpn_hist<1>, d_obj, n, K, hist, state);
        LAUNCH(h, "rpn_hist", dim3((unsigned)nblk), dim3(256), k_rpn_hist<2>, d_obj, n, K, hist, state);
        LAUNCH(h, "rpn_count", dim3((unsigned)nblk), dim3(256), k_rpn_count, d_obj, n, A, HW, (const uint32_t*)hist, state, blk, nblk);
        LAUNCH(h, "rpn_compact", dim3((unsigned)nblk), dim3(256), k_rpn_compact, d_obj, n, A, HW, K, (const uint32_t*)state, (const uint32_t*)blk, nblk, cand);
    }
    RpnArgs a;
    a.obj = d_obj; a.reg = d_reg; a.anc = d_anc; a.cand = select ? cand : nullptr;
    a.n = n; a.A = A; a.HW = HW; a.m = m;
    a.P = 2;
    while (a.P < (select ? m : n)) a.P <<= 1;
    a.q = q; a.min_size = p->min_size;
    a.sboxes = sboxes; a.slogit = slogit; a.sindex = sindex; a.ns = ns;
    LAUNCH(h, "rpn_sort_decode", dim3(1), dim3(1024), k_rpn_sort_decode, a);
    LAUNCH(h, "rpn_mask", dim3((unsigned)nb, (unsigned)nb), dim3(64), k_nms_mask_dev, (const float4*)sboxes, (const int32_t*)nullptr, (const int32_t*)ns, nb, p->nms_thresh, mask);
    LAUNCH(h, "rpn_reduce", dim3(1), dim3(1024), k_rpn_reduce, (const unsigned long long*)mask, (const float4*)sboxes, (const float*)slogit, (const int32_t*)sindex,
           (const int32_t*)ns, nb, p->post_nms_top_n, d_boxes, d_logits, (long long*)d_index, d_count);
    return ops_done(h, ops, stream);
}

// The proposal stage over the levels: one memset and nine launches whatever the number of levels (no level selects: four launches).  Scratch: per level the slices
// rpn_run takes, each sized from the level's own m, and the level's kept lists; behind them ns and c_l of all levels, and -- ONE take, zeroed by one memset per
// call -- the histograms and the state of the levels that select.
int rpn_fpn_run(ifx* h, const ifx_rpn_level* levels, int n_levels, const ifx_rpn_params* p, const BoxCode& q, int F, float* d_boxes, float* d_logits, int32_t* d_level,
                int64_t* d_index, int32_t* d_count, int32_t* d_level_counts, hipStream_t stream)
{
    RpnFpn f = {};
    f.L = n_levels;
    int nsel = 0, nblk_max = 0, nb_max = 1, rows = 0;
    for (int l = 0; l < n_levels; l++) {
        RpnLevel& v = f.lv[l];
        v.obj = levels[l].objectness; v.reg = levels[l].regression; v.anc = levels[l].anchors;
        v.A = levels[l].A; v.HW = levels[l].H * levels[l].W; v.n = v.A * v.HW;
        v.m = std::min(p->pre_nms_top_n, v.n);
        v.nb = cdiv(v.m, 64);
        v.nblk = v.n > NMS_MAX ? cdiv(v.n, RPN_CHUNK) : 0;
        v.cap = std::min(p->post_nms_top_n, v.m);
        v.P = 2;
        while (v.P < (v.nblk ? v.m : v.n)) v.P <<= 1;
        nsel += v.nblk > 0;
        nblk_max = std::max(nblk_max, v.nblk);
        nb_max = std::max(nb_max, v.nb);
        rows += v.cap;
    }
    uint32_t* zero = nullptr;
    DetOps* ops = nullptr;
    int r = ops_scratch(h, "ifx_rpn_proposals_fpn", [&](Carver& c) {
        for (int l = 0; l < n_levels; l++) {
            RpnLevel& v = f.lv[l];
            const size_t mc = (size_t)v.nb * 64;
            v.sboxes = c.take<float4>(mc);
            v.mask = c.take<unsigned long long>(mc * v.nb);
            v.cand = c.take<unsigned long long>(mc);
            v.slogit = c.take<float>(mc);
            v.sindex = c.take<int32_t>(mc);
            v.blk = c.take<uint32_t>(2 * (size_t)v.nblk);
            v.kbox = c.take<float>(4 * (size_t)v.cap);
            v.klogit = c.take<float>(v.cap);
            v.kindex = c.take<long long>(v.cap);
        }
        f.ns = c.take<int32_t>(2 * RPN_MAX_LEVELS);
        f.cnt = f.ns + RPN_MAX_LEVELS;
        zero = c.take<uint32_t>(nsel * RPN_ZERO_WORDS); // one take: one memset zeroes every selecting level's histograms and state
        for (int l = 0, s = 0; l < n_levels; l++) f.lv[l].hist = zero && f.lv[l].nblk ? zero + (s++) * RPN_ZERO_WORDS : nullptr;
    }, stream, &ops);
    if (r) return r;
    StreamScope scope(h, stream);
    const unsigned L = (unsigned)n_levels;
    if (nsel) {
        HIPCHK(h, hipMemsetAsync(zero, 0, nsel * RPN_ZERO_WORDS * 4, stream));
        const dim3 grid((unsigned)nblk_max, L);
        LAUNCH(h, "rpn_fpn_hist", grid, dim3(256), k_rpn_fpn_hist<0>, f);
        LAUNCH(h, "rpn_fpn_hist", grid, dim3(256), k_rpn_fpn_hist<1>, f);
        LAUNCH(h, "rpn_fpn_hist", grid, dim3(256), k_rpn_fpn_hist<2>, f);
        LAUNCH(h, "rpn_fpn_count", grid, dim3(256), k_rpn_fpn_count, f);
        LAUNCH(h, "rpn_fpn_compact", grid, dim3(256), k_rpn_fpn_compact, f);
    }
    LAUNCH(h, "rpn_fpn_sort_decode", dim3(L), dim3(1024), k_rpn_fpn_sort_decode, f, q, p->min_size);
    LAUNCH(h, "rpn_fpn_mask", dim3((unsigned)nb_max, (unsigned)nb_max, L), dim3(64), k_rpn_fpn_mask, f, p->nms_thresh);
    LAUNCH(h, "rpn_fpn_reduce", dim3(L), dim3(1024), k_rpn_fpn_reduce, f);
    LAUNCH(h, "rpn_fpn_merge", dim3((unsigned)cdiv(std::max(rows, F), 256)), dim3(256), k_rpn_fpn_merge, f, F, d_boxes, d_logits, d_level, (long long*)d_index, d_count,
           d_level_counts);
    return ops_done(h, ops, stream);
}

// The box head's post-processing: six launches.  Scratch, out of the handle's buffer: sorted boxes, mask words, then the 4-byte arrays --
// the plane of probabilities, the candidates' plane positions, the sorted groups / scores / candidate positions / rows, the per-block counts and K.  Every word a
// kernel reads is written by a kernel in front of it in the same call: nothing is zeroed.
int bd_run(ifx* h, const float* d_logits, const float* d_reg, const float* d_prop, int R, int C, int Creg, const ifx_box_det_params* p, const BoxCode& q, const BdOut& out,
           hipStream_t stream)
{
    const int n = (C - 1) * R, mc = cdiv(std::min(n, NMS_MAX), 64) * 64, nb = mc / 64, nblk = cdiv(n, BD_CHUNK);
    float4* sboxes; unsigned long long* mask; float *plane, *sscore; uint32_t *cand, *blk; int32_t *sgroups, *spos, *srow, *ktot;
    DetOps* ops = nullptr;
    int r = ops_scratch(h, "ifx_box_detections", [&](Carver& c) {
        sboxes = c.take<float4>(mc);
        mask = c.take<unsigned long long>((size_t)mc * nb);
        plane = c.take<float>(n);
        cand = c.take<uint32_t>(mc);
        sgroups = c.take<int32_t>(mc);
        sscore = c.take<float>(mc);
        spos = c.take<int32_t>(mc);
        srow = c.take<int32_t>(mc);
        blk = c.take<uint32_t>(nblk);
        ktot = c.take<int32_t>(4);                     // K (and padding)
    }, stream, &ops);
    if (r) return r;
    StreamScope scope(h, stream);
    LAUNCH(h, "bd_softmax", dim3((unsigned)cdiv(R, 4)), dim3(256), k_bd_softmax, d_logits, R, C, p->score_thresh, plane);
    LAUNCH(h, "bd_count", dim3((unsigned)nblk), dim3(256), k_bd_count, (const float*)plane, n, blk);
    LAUNCH(h, "bd_compact", dim3((unsigned)nblk), dim3(256), k_bd_compact, (const float*)plane, n, (const uint32_t*)blk, cand, ktot);
    BdArgs a;
    a.plane = plane; a.reg = d_reg; a.prop = d_prop; a.cand = cand; a.ktot = ktot;
    a.R = R; a.C = C; a.Creg = Creg; a.n = n; a.q = q;
    a.sboxes = sboxes; a.sgroups = sgroups; a.sscore = sscore; a.spos = spos; a.srow = srow;
    LAUNCH(h, "bd_sort_decode", dim3(1), dim3(1024), k_bd_sort_decode, a);
    LAUNCH(h, "bd_mask", dim3((unsigned)nb, (unsigned)nb), dim3(64), k_nms_mask_dev, (const float4*)sboxes, (const int32_t*)sgroups, (const int32_t*)ktot, nb, p->nms, mask);
    LAUNCH(h, "bd_reduce", dim3(1), dim3(1024), k_bd_reduce, (const unsigned long long*)mask, (const float4*)sboxes, (const int32_t*)sgroups, (const float*)sscore,
           (const int32_t*)spos, (const int32_t*)srow, (const int32_t*)ktot, nb, out);
    return ops_done(h, ops, stream);
}

// The stage's two launches on `stream` (R >= 1; the outputs are the caller's or the handle's scratch).
int mh_launch(ifx* h, const float* d_logits, const float* d_boxes, const float* d_scores, const int64_t* d_labels, const int32_t* d_count, const int32_t* d_class_map,
              int R, int C, int M, const ifx_mask_head_params* p, int out_w, int out_h, float* d_masks, float* d_boxes_out, int32_t* d_class_ids, int32_t* d_rows,
              int32_t* d_kept, hipStream_t stream)
{
    MhArgs a;
    a.logits = d_logits; a.boxes = d_boxes; a.scores = d_scores; a.labels = (const long long*)d_labels; a.count = d_count; a.class_map = d_class_map;
    a.R = R; a.C = C; a.MM = M * M; a.sort = p->sort_by_score != 0;
    a.P = 2;
    while (a.P < R) a.P <<= 1;
    a.thresh = p->score_thresh;
    a.rw = (float)((double)out_w / (double)p->in_w); a.rh = (float)((double)out_h / (double)p->in_h);
    a.masks = d_masks; a.boxes_out = d_boxes_out; a.class_ids = d_class_ids; a.rows = d_rows; a.kept = d_kept;
    StreamScope scope(h, stream);
    LAUNCH(h, "mh_select", dim3(1), dim3(1024), k_mh_select, a);
    LAUNCH(h, "mh_sigmoid", dim3((unsigned)R), dim3(256), k_mh_sigmoid, a);
    return IFX_OK;
}

// ifx_unmold_detections' select, memset and paste on `stream` (R >= 1, the arguments checked; the outputs are the caller's or the handle's scratch).
int um_launch(ifx* h, const float* d_det, const float* d_masks, const int32_t* window, const int32_t* d_class_map, int R, int M, int C, int layout, int W, int H,
              uint8_t* d_out, int32_t* d_class_ids, int32_t* d_boxes, float* d_scores, int32_t* d_rows, int32_t* d_kept, hipStream_t stream)
{
    UmArgs a;
    a.det = d_det; a.masks = d_masks; a.class_map = d_class_map;
    a.R = R; a.M = M; a.C = C; a.nchw = layout == IFX_UNMOLD_NCHW; a.W = W; a.H = H; a.wy1 = window[0]; a.wx1 = window[1];
    a.scale = std::min((double)H / (double)((int64_t)window[2] - window[0]), (double)W / (double)((int64_t)window[3] - window[1]));   // model.py:2314-2316
    a.out = d_out; a.class_ids = d_class_ids; a.boxes = d_boxes; a.rows = d_rows; a.kept = d_kept; a.scores = d_scores;
    StreamScope scope(h, stream);
    LAUNCH(h, "unmold_select", dim3(1), dim3(1024), k_unmold_select, a);
    HIPCHK(h, hipMemsetAsync(d_out, 0, (size_t)R * H * W, stream));
    LAUNCH(h, "unmold_paste", dim3((unsigned)cdiv(W, UM_TX), (unsigned)R), dim3(256), k_unmold_paste, a);
    return IFX_OK;
}

// no input: the padding alone -- `rows` zero boxes, zeros in the f32 array, -1 in the int64 arrays (each where it is given), a count of 0
int ops_padding(ifx* h, size_t rows, float* boxes, float* f32, int64_t* ia, int64_t* ib, int32_t* count, hipStream_t s)
{
    HIPCHK(h, hipMemsetAsync(boxes, 0, rows * 16, s));
    if (f32) HIPCHK(h, hipMemsetAsync(f32, 0, rows * 4, s));
    if (ia) HIPCHK(h, hipMemsetAsync(ia, 0xFF, rows * 8, s));
    if (ib) HIPCHK(h, hipMemsetAsync(ib, 0xFF, rows * 8, s));
    HIPCHK(h, hipMemsetAsync(count, 0, 4, s));
    return IFX_OK;
}

// weights and the clip of BoxCoder into the kernels' record; NULL: fine, else what is wrong
const char* box_code(const float weights[4], float xform_clip, int clip_w, int clip_h, BoxCode* q)
{
    for (int i = 0; i < 4; i++)
        if (!std::isfinite(weights[i]) || weights[i] == 0.f) return "a weight is 0 or not finite";
    if ((clip_w == 0) != (clip_h == 0) || clip_w < 0 || clip_h < 0) return "clip_w, clip_h: both 0 (no clip) or both >= 1";
    q->wx = weights[0]; q->wy = weights[1]; q->ww = weights[2]; q->wh = weights[3];
    q->xform_clip = xform_clip > 0.f ? xform_clip : (float)std::log(1000.0 / 16.0);      // (a NaN compares false: the default)
    q->clip = clip_w > 0;
    q->xmax = (float)(clip_w - 1); q->ymax = (float)(clip_h - 1);
    return nullptr;
}

// ifx_keras_proposals' launches: one memset and eight launches when the layer selects (n > 8192), three launches otherwise.  Scratch as rpn_run's, less the logits.
int kp_run(ifx* h, const float* d_probs, const float* d_bbox, const float* d_anc, int n, const ifx_keras_proposal_params* p, float* d_proposals, int64_t* d_index,
           int32_t* d_count, hipStream_t stream)
{
    const int m = std::min(p->pre_nms_limit, n), mc = cdiv(m, 64) * 64, nb = mc / 64, nblk = cdiv(n, RPN_CHUNK);
    const bool select = n > NMS_MAX;
    const size_t zero_words = 3 * RPN_BINS + 8 + 8;    // histograms, state, the count (and padding)
    float4* sboxes; unsigned long long *mask, *cand; int32_t* sindex; uint32_t *blk, *hist;
    DetOps* ops = nullptr;
    int r = ops_scratch(h, "ifx_keras_proposals", [&](Carver& c) {
        sboxes = c.take<float4>(mc);
        mask = c.take<unsigned long long>((size_t)mc * nb);
        cand = c.take<unsigned long long>(mc);
        sindex = c.take<int32_t>(mc);
        blk = c.take<uint32_t>(2 * (size_t)nblk);
        hist = c.take<uint32_t>(zero_words);           // one take: one memset zeroes the histograms and the state
    }, stream, &ops);
    if (r) return r;
    uint32_t* state = hist + 3 * RPN_BINS;
    int32_t* ns = (int32_t*)(state + 8);
    const float* score = d_probs + 1;                  // probs[i][1]
    StreamScope scope(h, stream);
    const uint32_t K = (uint32_t)m;
    if (select) {
        HIPCHK(h, hipMemsetAsync(hist, 0, zero_words * 4, stream));
        LAUNCH(h, "kp_hist", dim3((unsigned)nblk), dim3(256), (k_rpn_hist<0, KP_STRIDE>), score, n, K, hist, state);
        LAUNCH(h, "kp_hist", dim3((unsigned)nblk), dim3(256), (k_rpn_hist<1, KP_STRIDE>), score, n, K, hist, state);
        LAUNCH(h, "kp_hist", dim3((unsigned)nblk), dim3(256), (k_rpn_hist<2, KP_STRIDE>), score, n, K, hist, state);
        LAUNCH(h, "kp_count", dim3((unsigned)nblk), dim3(256), k_kp_count, score, n, (const uint32_t*)hist, state, blk, nblk);
        LAUNCH(h, "kp_compact", dim3((unsigned)nblk), dim3(256), k_kp_compact, score, n, K, (const uint32_t*)state, (const uint32_t*)blk, nblk, cand);
    }
    KpArgs a;
    a.score = score; a.bbox = d_bbox; a.anc = d_anc; a.cand = select ? cand : nullptr;
    a.n = n; a.m = m;
    a.P = 2;
    while (a.P < (select ? m : n)) a.P <<= 1;
    a.sd0 = p->std_dev[0]; a.sd1 = p->std_dev[1]; a.sd2 = p->std_dev[2]; a.sd3 = p->std_dev[3];
    a.ih = (float)p->image_h; a.iw = (float)p->image_w;
    a.sboxes = sboxes; a.sindex = sindex; a.ns = ns;
    LAUNCH(h, "kp_sort_decode", dim3(1), dim3(1024), k_kp_sort_decode, a);
    LAUNCH(h, "kp_mask", dim3((unsigned)nb, (unsigned)nb), dim3(64), k_nms_mask_dev_tf, (const float4*)sboxes, (const int32_t*)nullptr, (const int32_t*)ns, nb, p->nms_threshold,
           mask);
    LAUNCH(h, "kp_reduce", dim3(1), dim3(1024), k_rpn_reduce, (const unsigned long long*)mask, (const float4*)sboxes, (const float*)nullptr, (const int32_t*)sindex,
           (const int32_t*)ns, nb, p->proposal_count, d_proposals, (float*)nullptr, (long long*)d_index, d_count);
    return ops_done(h, ops, stream);
}

// ifx_keras_detections' four launches.  Every word a kernel reads is written by a kernel in front of it in the same call: nothing is zeroed.
int kd_run(ifx* h, const float* d_rois, const float* d_probs, const float* d_deltas, int R, int C, const ifx_keras_detection_params* p, const KdOut& out, hipStream_t stream)
{
    const int mc = cdiv(R, 64) * 64, nb = mc / 64;
    KdArgs a;
    unsigned long long* mask;
    DetOps* ops = nullptr;
    int r = ops_scratch(h, "ifx_keras_detections", [&](Carver& c) {
        a.sboxes = c.take<float4>(mc);
        mask = c.take<unsigned long long>((size_t)mc * nb);
        a.keys = c.take<unsigned long long>(mc);
        a.rbox = c.take<float4>(mc);
        a.rcls = c.take<int32_t>(mc);
        a.rscore = c.take<float>(mc);
        a.sgroups = c.take<int32_t>(mc);
        a.sscore = c.take<float>(mc);
        a.srow = c.take<int32_t>(mc);
        a.ns = c.take<int32_t>(4);                     // the rows that stay (and padding)
    }, stream, &ops);
    if (r) return r;
    a.rois = d_rois; a.probs = d_probs; a.deltas = d_deltas;
    a.R = R; a.C = C;
    a.P = 2;
    while (a.P < R) a.P <<= 1;
    a.sd0 = p->std_dev[0]; a.sd1 = p->std_dev[1]; a.sd2 = p->std_dev[2]; a.sd3 = p->std_dev[3];
    a.minconf = p->min_confidence; a.ih = (float)p->image_h; a.iw = (float)p->image_w;
    a.wy1 = p->window[0]; a.wx1 = p->window[1]; a.wy2 = p->window[2]; a.wx2 = p->window[3];
    StreamScope scope(h, stream);
    LAUNCH(h, "kd_rows", dim3((unsigned)cdiv(R, 4)), dim3(256), k_kd_rows, a);
    LAUNCH(h, "kd_sort", dim3(1), dim3(1024), k_kd_sort, a);
    LAUNCH(h, "kd_mask", dim3((unsigned)nb, (unsigned)nb), dim3(64), k_nms_mask_dev_tf, (const float4*)a.sboxes, (const int32_t*)a.sgroups, (const int32_t*)a.ns, nb,
           p->nms_threshold, mask);
    LAUNCH(h, "kd_reduce", dim3(1), dim3(1024), k_kd_reduce, (const unsigned long long*)mask, (const float4*)a.sboxes, (const int32_t*)a.sgroups, (const float*)a.sscore,
           (const int32_t*)a.srow, (const int32_t*)a.ns, nb, out);
    return ops_done(h, ops, stream);
}

}   // namespace

void ifx_detector_free(ifx* h)
{
    if (DetOps* ops = (DetOps*)h->det_ops) {
        if (ops->buf) hipFree(ops->buf);
        if (ops->ev) hipEventDestroy(ops->ev);
        delete ops;
        h->det_ops = nullptr;
    }
    DetPrep* dp = (DetPrep*)h->det_prep;
    if (!dp) return;
    for (DetTable& t : dp->tabs) { hipFree(t.dev); hipHostFree(t.host); }
    if (dp->ev_in) hipEventDestroy(dp->ev_in);
    if (dp->ev_out) hipEventDestroy(dp->ev_out);
    delete dp;
    h->det_prep = nullptr;
}

extern "C" int ifx_detector_input_size(int width, int height, const ifx_detector_prep* p, int32_t* out4)
{
    return ifx_detprep::input_size(width, height, p, out4) ? IFX_E_INVALID : IFX_OK;
}

extern "C" int ifx_detector_resize_taps(int in_size, int out_size, int32_t* first, int32_t* count, int32_t* coeff, int max_ksize)
{
    if (!first || !count || !coeff) return IFX_E_INVALID;
    const int ks = ifx_detprep::resize_taps(in_size, out_size, first, count, coeff, max_ksize);
    return ks < 0 ? IFX_E_INVALID : ks;
}

extern "C" int ifx_detector_input_image(ifx_t* h, const uint8_t* d_rgb, int width, int height, const ifx_detector_prep* p, float* d_out, int64_t out_floats, void* stream)
{
    if (!h) return IFX_E_INVALID;
    if (!d_rgb) { h->err = "ifx_detector_input_image: NULL pointer"; return IFX_E_INVALID; }
    int32_t sz[4];
    int r = det_check(h, "ifx_detector_input_image", width, height, p, d_out, out_floats, sz);
    if (r) return r;
    return det_run(h, d_rgb, width, height, p, sz, d_out, stream, nullptr, nullptr);
}

extern "C" int ifx_detector_input(ifx_t* h, int ticket, const ifx_detector_prep* p, float* d_out, int64_t out_floats, void* stream)
{
    if (!h) return IFX_E_INVALID;
    int32_t sz[4];
    int r = det_check(h, "ifx_detector_input", h->w, h->h, p, d_out, out_floats, sz);
    if (r) return r;
    const uint8_t* rgb = nullptr;
    hipEvent_t ev = nullptr;
    FrameSlot* slot = nullptr;
    if ((r = ifx_frame_for_reader(h, "ifx_detector_input", ticket, &rgb, &ev, &slot))) return r;
    return det_run(h, rgb, h->w, h->h, p, sz, d_out, stream, ev, slot);
}

extern "C" int ifx_roi_align_forward(ifx_t* h, const float* d_input, int batch, int channels, int height, int width, const float* d_rois, int n, float spatial_scale,
                                     int pooled_h, int pooled_w, int sampling_ratio, float* d_out, void* stream)
{
    if (!h) return IFX_E_INVALID;
    if (n < 0 || batch < 1 || channels < 1 || height < 1 || width < 1 || pooled_h < 1 || pooled_w < 1 || sampling_ratio < 0) {
        h->err = "ifx_roi_align_forward: n < 0, a size < 1 or sampling_ratio < 0"; return IFX_E_INVALID;
    }
    if (!std::isfinite(spatial_scale)) { h->err = "ifx_roi_align_forward: spatial_scale is not finite"; return IFX_E_INVALID; }
    if (n == 0) return IFX_OK;
    if (!d_input || !d_rois || !d_out) { h->err = "ifx_roi_align_forward: NULL pointer"; return IFX_E_INVALID; }
    const int chunks = cdiv(channels, RA_CH);
    if ((int64_t)n * chunks > 0x7FFFFFFF || (int64_t)pooled_h * pooled_w > (1 << 24) || (int64_t)height * width > 0x7FFFFFFF) {
        h->err = "ifx_roi_align_forward: more than 2^31 - 1 blocks (n x ceil(channels / 64)), more than 2^24 bins or more than 2^31 - 1 texels per plane"; return IFX_E_INVALID;
    }
    RaArgs a;
    a.in = d_input; a.rois = d_rois; a.out = d_out;
    a.batch = batch; a.channels = channels; a.height = height; a.width = width; a.ph = pooled_h; a.pw = pooled_w; a.ratio = sampling_ratio; a.chunks = chunks;
    a.scale = spatial_scale;
    StreamScope scope(h, (hipStream_t)stream);
    LAUNCH(h, "roi_align", dim3((unsigned)(n * chunks)), dim3(256), k_roi_align, a);
    return IFX_OK;
}

// k_min of the ladder scales[l] == 2^-(k_min + l), k_min >= 0 and every entry a normal number; -1 for any other list
static int fpn_ladder(const float* scales, int levels)
{
    int k = 0;
    while (k <= 126 && scales[0] != std::ldexp(1.f, -k)) k++;
    if (k + levels - 1 > 126) return -1;
    for (int l = 0; l < levels; l++)
        if (scales[l] != std::ldexp(1.f, -(k + l))) return -1;
    return k;
}

// floor(f32(lvl0 + f32(log2(v)))) >= target, the rule's two roundings included
static bool fpn_reaches(float v, float lvl0, float target)
{
    const float L = (float)std::log2((double)v);
    const float t = lvl0 + L;
    return std::floor(t) >= target;
}

// thr[j], j = 1 .. levels - 1: the smallest f32 v >= 0 that reaches level k_min + j, by bisection over the bit patterns 0 (-inf: reaches nothing) .. +inf
static void fpn_thresholds(int levels, int k_min, int canonical_level, float* thr)
{
    thr[0] = 0.f;
    for (int j = 1; j < levels; j++) {
        uint32_t lo = 0u, hi = 0x7F800000u;
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            float v;
            std::memcpy(&v, &mid, 4);
            if (fpn_reaches(v, (float)canonical_level, (float)(k_min + j))) hi = mid; else lo = mid;
        }
        std::memcpy(&thr[j], &hi, 4);
    }
}

extern "C" int ifx_fpn_level_thresholds(const float* scales, int levels, int canonical_level, float* out)
{
    if (!scales || !out || levels < 1 || levels > FPN_MAX) return IFX_E_INVALID;
    const int k_min = fpn_ladder(scales, levels);
    if (k_min < 0) return IFX_E_INVALID;
    float thr[FPN_MAX];
    fpn_thresholds(levels, k_min, canonical_level, thr);
    for (int j = 1; j < levels; j++) out[j - 1] = thr[j];
    return k_min;
}

extern "C" int ifx_fpn_roi_align(ifx_t* h, const float* const* d_features, const int32_t* heights, const int32_t* widths, const float* scales, int levels, int batch,
                                 int channels, const float* d_rois, int n, float canonical_scale, int canonical_level, float eps, int pooled_h, int pooled_w,
                                 int sampling_ratio, float* d_out, int32_t* d_levels, void* stream)
{
    if (!h) return IFX_E_INVALID;
    if (levels < 1 || levels > FPN_MAX) { h->err = "ifx_fpn_roi_align: levels outside 1 .. 8"; return IFX_E_INVALID; }
    if (!d_features || !heights || !widths || !scales) { h->err = "ifx_fpn_roi_align: NULL pointer"; return IFX_E_INVALID; }
    if (n < 0 || batch < 1 || channels < 1 || pooled_h < 1 || pooled_w < 1 || sampling_ratio < 0) {
        h->err = "ifx_fpn_roi_align: n < 0, a size < 1 or sampling_ratio < 0"; return IFX_E_INVALID;
    }
    for (int l = 0; l < levels; l++)
        if (heights[l] < 1 || widths[l] < 1) { h->err = "ifx_fpn_roi_align: n < 0, a size < 1 or sampling_ratio < 0"; return IFX_E_INVALID; }
    const int k_min = fpn_ladder(scales, levels);
    if (k_min < 0) { h->err = "ifx_fpn_roi_align: the scales are not 2^-k_min, 2^-(k_min + 1), ... for an integer k_min >= 0"; return IFX_E_INVALID; }
    if (!(canonical_scale > 0.f) || !std::isfinite(canonical_scale)) { h->err = "ifx_fpn_roi_align: canonical_scale is not a positive finite number"; return IFX_E_INVALID; }
    if (!std::isfinite(eps)) { h->err = "ifx_fpn_roi_align: eps is not finite"; return IFX_E_INVALID; }
    if (n == 0) return IFX_OK;
    if (!d_rois || !d_out) { h->err = "ifx_fpn_roi_align: NULL pointer"; return IFX_E_INVALID; }
    const int chunks = cdiv(channels, RA_CH);
    if ((int64_t)n * chunks > 0x7FFFFFFF || (int64_t)pooled_h * pooled_w > (1 << 24)) {
        h->err = "ifx_fpn_roi_align: more than 2^31 - 1 blocks (n x ceil(channels / 64)) or more than 2^24 bins"; return IFX_E_INVALID;
    }
    FpnArgs a;
    for (int l = 0; l < FPN_MAX; l++) {
        const int s = l < levels ? l : levels - 1;     // the unused entries repeat the last level
        if (!d_features[s]) { h->err = "ifx_fpn_roi_align: NULL pointer"; return IFX_E_INVALID; }
        if ((int64_t)heights[s] * widths[s] > 0x7FFFFFFF) { h->err = "ifx_fpn_roi_align: more than 2^31 - 1 texels per plane"; return IFX_E_INVALID; }
        a.in[l] = d_features[s]; a.height[l] = heights[s]; a.width[l] = widths[s]; a.scale[l] = scales[s];
        a.thr[l] = 0.f;
    }
    if (levels > 1) fpn_thresholds(levels, k_min, canonical_level, a.thr);
    a.rois = d_rois; a.out = d_out; a.lev_out = d_levels;
    a.levels = levels; a.batch = batch; a.channels = channels; a.ph = pooled_h; a.pw = pooled_w; a.ratio = sampling_ratio; a.chunks = chunks;
    a.s0 = canonical_scale; a.eps = eps;
    StreamScope scope(h, (hipStream_t)stream);
    LAUNCH(h, "fpn_roi_align", dim3((unsigned)(n * chunks)), dim3(256), k_fpn_roi_align, a);
    return IFX_OK;
}

extern "C" int ifx_nms(ifx_t* h, const float* d_boxes, const float* d_scores, const int32_t* d_groups, int n, float threshold, int64_t* d_keep, int32_t* d_count, void* stream)
{
    if (!h) return IFX_E_INVALID;
    if (n < 0 || n > NMS_MAX) { h->err = "ifx_nms: n outside 0 .. 8192"; return IFX_E_INVALID; }
    if (threshold != threshold) { h->err = "ifx_nms: the threshold is NaN"; return IFX_E_INVALID; }
    if (!d_count || (n > 0 && (!d_boxes || !d_scores || !d_keep))) { h->err = "ifx_nms: NULL pointer"; return IFX_E_INVALID; }
    if (n == 0) { HIPCHK(h, hipMemsetAsync(d_count, 0, 4, (hipStream_t)stream)); return IFX_OK; }
    return nms_run(h, d_boxes, d_scores, d_groups, n, threshold, d_keep, d_count, (hipStream_t)stream);
}

extern "C" int ifx_rpn_proposals(ifx_t* h, const float* d_objectness, const float* d_regression, const float* d_anchors, int A, int H, int W, const ifx_rpn_params* p,
                                 float* d_boxes, float* d_logits, int64_t* d_index, int32_t* d_count, void* stream)
{
    if (!h) return IFX_E_INVALID;
    if (!p || !d_boxes || !d_count) { h->err = "ifx_rpn_proposals: NULL pointer"; return IFX_E_INVALID; }
    if (A < 0 || H < 0 || W < 0 || (int64_t)A * H * W > RPN_MAX_N || (int64_t)H * W > RPN_MAX_N) { h->err = "ifx_rpn_proposals: a size < 0 or A x H x W above 2^24"; return IFX_E_INVALID; }
    if (p->pre_nms_top_n < 1 || p->pre_nms_top_n > NMS_MAX || p->post_nms_top_n < 1 || p->post_nms_top_n > NMS_MAX) {
        h->err = "ifx_rpn_proposals: pre_nms_top_n or post_nms_top_n outside 1 .. 8192"; return IFX_E_INVALID;
    }
    if (p->nms_thresh != p->nms_thresh) { h->err = "ifx_rpn_proposals: the threshold is NaN"; return IFX_E_INVALID; }
    if (p->image_w < 1 || p->image_h < 1) { h->err = "ifx_rpn_proposals: image_w or image_h < 1"; return IFX_E_INVALID; }
    BoxCode q;
    if (const char* bad = box_code(p->weights, p->xform_clip, p->image_w, p->image_h, &q)) { h->err = std::string("ifx_rpn_proposals: ") + bad; return IFX_E_INVALID; }
    const int n = A * H * W;
    if (n > 0 && (!d_objectness || !d_regression || !d_anchors)) { h->err = "ifx_rpn_proposals: NULL pointer"; return IFX_E_INVALID; }
    if (n == 0) return ops_padding(h, (size_t)p->post_nms_top_n, d_boxes, d_logits, d_index, nullptr, d_count, (hipStream_t)stream);   // no anchors
    return rpn_run(h, d_objectness, d_regression, d_anchors, A, H * W, p, q, d_boxes, d_logits, d_index, d_count, (hipStream_t)stream);
}

extern "C" int ifx_rpn_proposals_fpn(ifx_t* h, const ifx_rpn_level* levels, int n_levels, const ifx_rpn_params* p, int fpn_post_nms_top_n, float* d_boxes, float* d_logits,
                                     int32_t* d_level, int64_t* d_index, int32_t* d_count, int32_t* d_level_counts, void* stream)
{
    if (!h) return IFX_E_INVALID;
    if (!levels || !p || !d_boxes || !d_count) { h->err = "ifx_rpn_proposals_fpn: NULL pointer"; return IFX_E_INVALID; }
    if (n_levels < 1 || n_levels > RPN_MAX_LEVELS) { h->err = "ifx_rpn_proposals_fpn: n_levels outside 1 .. 8"; return IFX_E_INVALID; }
    if (fpn_post_nms_top_n < 1 || fpn_post_nms_top_n > NMS_MAX) { h->err = "ifx_rpn_proposals_fpn: fpn_post_nms_top_n outside 1 .. 8192"; return IFX_E_INVALID; }
    if (p->pre_nms_top_n < 1 || p->pre_nms_top_n > NMS_MAX || p->post_nms_top_n < 1 || p->post_nms_top_n > NMS_MAX) {
        h->err = "ifx_rpn_proposals_fpn: pre_nms_top_n or post_nms_top_n outside 1 .. 8192"; return IFX_E_INVALID;
    }
    if (p->nms_thresh != p->nms_thresh) { h->err = "ifx_rpn_proposals_fpn: the threshold is NaN"; return IFX_E_INVALID; }
    if (p->image_w < 1 || p->image_h < 1) { h->err = "ifx_rpn_proposals_fpn: image_w or image_h < 1"; return IFX_E_INVALID; }
    BoxCode q;
    if (const char* bad = box_code(p->weights, p->xform_clip, p->image_w, p->image_h, &q)) { h->err = std::string("ifx_rpn_proposals_fpn: ") + bad; return IFX_E_INVALID; }
    for (int l = 0; l < n_levels; l++) {
        const ifx_rpn_level& v = levels[l];
        if (v.A < 0 || v.H < 0 || v.W < 0 || (int64_t)v.A * v.H * v.W > RPN_MAX_N || (int64_t)v.H * v.W > RPN_MAX_N) {
            h->err = "ifx_rpn_proposals_fpn: a level with a size < 0 or A x H x W above 2^24"; return IFX_E_INVALID;
        }
        if (v.A && v.H && v.W && (!v.objectness || !v.regression || !v.anchors)) { h->err = "ifx_rpn_proposals_fpn: NULL pointer in a level with anchors"; return IFX_E_INVALID; }
    }
    return rpn_fpn_run(h, levels, n_levels, p, q, fpn_post_nms_top_n, d_boxes, d_logits, d_level, d_index, d_count, d_level_counts, (hipStream_t)stream);
}

extern "C" int ifx_box_decode(ifx_t* h, const float* d_codes, const float* d_boxes, int n, int k, const float weights[4], float xform_clip, int clip_w, int clip_h,
                              float* d_out, void* stream)
{
    if (!h) return IFX_E_INVALID;
    if (n < 0 || k < 1 || (int64_t)n * k > 0x7FFFFFFF) { h->err = "ifx_box_decode: n < 0, k < 1 or more than 2^31 - 1 boxes"; return IFX_E_INVALID; }
    if (!weights) { h->err = "ifx_box_decode: NULL pointer"; return IFX_E_INVALID; }
    BoxCode q;
    if (const char* bad = box_code(weights, xform_clip, clip_w, clip_h, &q)) { h->err = std::string("ifx_box_decode: ") + bad; return IFX_E_INVALID; }
    if (n == 0) return IFX_OK;
    if (!d_codes || !d_boxes || !d_out) { h->err = "ifx_box_decode: NULL pointer"; return IFX_E_INVALID; }
    const long long total = (long long)n * k;
    StreamScope scope(h, (hipStream_t)stream);
    LAUNCH(h, "box_decode", dim3((unsigned)((total + 255) / 256)), dim3(256), k_box_decode, d_codes, d_boxes, total, k, q, d_out);
    return IFX_OK;
}

extern "C" int ifx_box_detections(ifx_t* h, const float* d_logits, const float* d_regression, const float* d_proposals, int R, int C, int Creg, const ifx_box_det_params* p,
                                  float* d_boxes, float* d_scores, int64_t* d_labels, int64_t* d_index, int32_t* d_count, int32_t* d_stats, void* stream)
{
    if (!h) return IFX_E_INVALID;
    if (!p || !d_boxes || !d_count) { h->err = "ifx_box_detections: NULL pointer"; return IFX_E_INVALID; }
    if (R < 0 || C < 2 || C > BD_MAX_C || (int64_t)R * C > RPN_MAX_N) { h->err = "ifx_box_detections: R < 0, C outside 2 .. 1024 or R x C above 2^24"; return IFX_E_INVALID; }
    if (Creg != 1 && Creg != C) { h->err = "ifx_box_detections: Creg is neither C nor 1"; return IFX_E_INVALID; }
    if (p->max_out < 1 || p->max_out > NMS_MAX || p->detections_per_img > p->max_out) {
        h->err = "ifx_box_detections: max_out outside 1 .. 8192 or detections_per_img above max_out"; return IFX_E_INVALID;
    }
    if (p->score_thresh != p->score_thresh || p->nms != p->nms) { h->err = "ifx_box_detections: score_thresh or nms is NaN"; return IFX_E_INVALID; }
    if (p->image_w < 1 || p->image_h < 1) { h->err = "ifx_box_detections: image_w or image_h < 1"; return IFX_E_INVALID; }
    BoxCode q;
    if (const char* bad = box_code(p->weights, p->xform_clip, p->image_w, p->image_h, &q)) { h->err = std::string("ifx_box_detections: ") + bad; return IFX_E_INVALID; }
    if (R > 0 && (!d_logits || !d_regression || !d_proposals)) { h->err = "ifx_box_detections: NULL pointer"; return IFX_E_INVALID; }
    if (R == 0) {                                      // no rows
        if (d_stats) HIPCHK(h, hipMemsetAsync(d_stats, 0, 8, (hipStream_t)stream));
        return ops_padding(h, (size_t)p->max_out, d_boxes, d_scores, d_labels, d_index, d_count, (hipStream_t)stream);
    }
    BdOut o;
    o.boxes = d_boxes; o.scores = d_scores; o.labels = (long long*)d_labels; o.index = (long long*)d_index; o.count = d_count; o.stats = d_stats;
    o.max_out = p->max_out; o.limit = p->detections_per_img;
    return bd_run(h, d_logits, d_regression, d_proposals, R, C, Creg, p, q, o, (hipStream_t)stream);
}

// the argument checks the three mask-head entries share; they touch nothing (`own_out`: the stage entry, whose out_w, out_h count; the two process entries of
// ifx_instance.hip take the frame's size)
int ifx_mask_head_check(ifx* h, const char* who, const float* d_logits, const float* d_boxes, const float* d_scores, const int64_t* d_labels, int R, int C, int M,
                        const ifx_mask_head_params* p, bool own_out)
{
    if (!p) { h->err = std::string(who) + ": NULL pointer"; return IFX_E_INVALID; }
    if (M < 1 || M > MH_MAX_M || C < 1 || C > MH_MAX_C || R < 0 || R > MH_MAX_R) { h->err = std::string(who) + ": M outside 1 .. 64, C outside 1 .. 1024 or R outside 0 .. 1024"; return IFX_E_INVALID; }
    if (R > 0 && (!d_logits || !d_boxes || !d_scores || !d_labels)) { h->err = std::string(who) + ": NULL pointer"; return IFX_E_INVALID; }
    if (p->score_thresh != p->score_thresh) { h->err = std::string(who) + ": score_thresh is NaN"; return IFX_E_INVALID; }
    if (p->in_w < 1 || p->in_h < 1 || (own_out && (p->out_w < 1 || p->out_h < 1))) { h->err = std::string(who) + ": in_w, in_h, out_w or out_h < 1"; return IFX_E_INVALID; }
    return IFX_OK;
}

extern "C" int ifx_mask_head_select(ifx_t* h, const float* d_mask_logits, const float* d_boxes, const float* d_scores, const int64_t* d_labels, const int32_t* d_count,
                                    const int32_t* d_class_map, int R, int C, int M, const ifx_mask_head_params* p, float* d_roi_masks, float* d_boxes_out,
                                    int32_t* d_class_ids, int32_t* d_rows, int32_t* d_kept, void* stream)
{
    if (!h) return IFX_E_INVALID;
    int r = ifx_mask_head_check(h, "ifx_mask_head_select", d_mask_logits, d_boxes, d_scores, d_labels, R, C, M, p, true);
    if (r) return r;
    if (!d_kept || (R > 0 && (!d_roi_masks || !d_boxes_out || !d_class_ids))) { h->err = "ifx_mask_head_select: NULL pointer"; return IFX_E_INVALID; }
    if (R == 0) { HIPCHK(h, hipMemsetAsync(d_kept, 0, 4, (hipStream_t)stream)); return IFX_OK; }
    return mh_launch(h, d_mask_logits, d_boxes, d_scores, d_labels, d_count, d_class_map, R, C, M, p, p->out_w, p->out_h, d_roi_masks, d_boxes_out, d_class_ids, d_rows,
                     d_kept, (hipStream_t)stream);
}

// The stage of ifx_process_segmentation_[deferred_]detections (ifx_instance.hip): into the detector operators' scratch on the producer's stream at the handle's frame size, then the one 4-byte read of kept.
// The pointers stay good until the next detector operator on this handle; the segmentation call that reads them ends with the host waiting for its stream.
int ifx_mask_head_stage(ifx* h, const char* who, const float* d_logits, const float* d_boxes, const float* d_scores, const int64_t* d_labels, const int32_t* d_count,
                        const int32_t* d_class_map, int R, int C, int M, const ifx_mask_head_params* p, void* stream, const float** roi_masks, const float** boxes,
                        const int32_t** class_ids, int* kept)
{
    *roi_masks = nullptr; *boxes = nullptr; *class_ids = nullptr; *kept = 0;
    if (R == 0) return IFX_OK;
    hipStream_t s = (hipStream_t)stream;
    float *masks, *bout; int32_t *cls, *dkept;
    DetOps* ops = nullptr;
    int r = ops_scratch(h, who, [&](Carver& c) {
        masks = c.take<float>((size_t)R * M * M);
        bout = c.take<float>(4 * (size_t)R);
        cls = c.take<int32_t>(R);
        dkept = c.take<int32_t>(4);                    // kept (and padding)
    }, s, &ops);
    if (r) return r;
    if ((r = mh_launch(h, d_logits, d_boxes, d_scores, d_labels, d_count, d_class_map, R, C, M, p, h->w, h->h, masks, bout, cls, nullptr, dkept, s))) return r;
    if ((r = ops_done(h, ops, s))) return r;
    int32_t n = 0;
    HIPCHK(h, hipMemcpyAsync(&n, dkept, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    *roi_masks = masks; *boxes = bout; *class_ids = cls; *kept = n;
    return IFX_OK;
}

// the argument checks the three unmold entries share; they touch nothing (max_r: 1024 for the stage, 256 for the process entries, whose scratch is R x P bytes)
int ifx_unmold_check(ifx* h, const char* who, const float* d_det, const float* d_masks, const int32_t* window, int R, int M, int C, int layout, int max_r)
{
    if (M < 1 || M > MH_MAX_M || C < 2 || C > MH_MAX_C || R < 0 || R > max_r) {
        h->err = std::string(who) + ": M outside 1 .. 64, C outside 2 .. 1024 or R outside 0 .. " + std::to_string(max_r); return IFX_E_INVALID;
    }
    if (layout != IFX_UNMOLD_NHWC && layout != IFX_UNMOLD_NCHW) { h->err = std::string(who) + ": unknown layout"; return IFX_E_INVALID; }
    if (!window) { h->err = std::string(who) + ": NULL window"; return IFX_E_INVALID; }
    if (window[2] <= window[0] || window[3] <= window[1]) { h->err = std::string(who) + ": the window is empty (wy2 <= wy1 or wx2 <= wx1)"; return IFX_E_INVALID; }
    if (R > 0 && (!d_det || !d_masks)) { h->err = std::string(who) + ": NULL pointer"; return IFX_E_INVALID; }
    return IFX_OK;
}

extern "C" int ifx_unmold_detections(ifx_t* h, const float* d_detections, const float* d_masks, const int32_t* window, const int32_t* d_class_map, int R, int M, int C,
                                     int layout, int width, int height, uint8_t* d_masks_out, int32_t* d_class_ids, int32_t* d_boxes_out, float* d_scores_out,
                                     int32_t* d_rows, int32_t* d_kept, void* stream)
{
    if (!h) return IFX_E_INVALID;
    int r = ifx_unmold_check(h, "ifx_unmold_detections", d_detections, d_masks, window, R, M, C, layout, MH_MAX_R);
    if (r) return r;
    if (width < 1 || height < 1) { h->err = "ifx_unmold_detections: width or height < 1"; return IFX_E_INVALID; }
    if (!d_kept || (R > 0 && (!d_masks_out || !d_class_ids || !d_boxes_out))) { h->err = "ifx_unmold_detections: NULL pointer"; return IFX_E_INVALID; }
    if (R == 0) { HIPCHK(h, hipMemsetAsync(d_kept, 0, 4, (hipStream_t)stream)); return IFX_OK; }
    return um_launch(h, d_detections, d_masks, window, d_class_map, R, M, C, layout, width, height, d_masks_out, d_class_ids, d_boxes_out, d_scores_out, d_rows, d_kept,
                     (hipStream_t)stream);
}

// The stage of ifx_process_segmentation_[deferred_]unmolded (ifx_instance.hip): into the detector operators' scratch on the producer's stream at the handle's frame
// size, then the one 4-byte read of kept.  The pointers stay good until the next detector operator on this handle, as ifx_mask_head_stage's do.
int ifx_unmold_stage(ifx* h, const char* who, const float* d_det, const float* d_masks, const int32_t* window, const int32_t* d_class_map, int R, int M, int C, int layout,
                     void* stream, const uint8_t** masks_out, const int32_t** class_ids, int* kept)
{
    *masks_out = nullptr; *class_ids = nullptr; *kept = 0;
    if (R == 0) return IFX_OK;
    hipStream_t s = (hipStream_t)stream;
    uint8_t* masks; int32_t *cls, *boxes, *dkept;
    DetOps* ops = nullptr;
    int r = ops_scratch(h, who, [&](Carver& c) {
        masks = c.take<uint8_t>((size_t)R * h->P);
        cls = c.take<int32_t>(R);
        boxes = c.take<int32_t>(4 * (size_t)R);
        dkept = c.take<int32_t>(4);                    // kept (and padding)
    }, s, &ops);
    if (r) return r;
    if ((r = um_launch(h, d_det, d_masks, window, d_class_map, R, M, C, layout, h->w, h->h, masks, cls, boxes, nullptr, nullptr, dkept, s))) return r;
    if ((r = ops_done(h, ops, s))) return r;
    int32_t n = 0;
    HIPCHK(h, hipMemcpyAsync(&n, dkept, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    *masks_out = masks; *class_ids = cls; *kept = n;
    return IFX_OK;
}

extern "C" int ifx_molded_input_size(int width, int height, int min_dim, int max_dim, int32_t* out8)
{
    return ifx_detprep::molded_input_size(width, height, min_dim, max_dim, out8) ? IFX_E_INVALID : IFX_OK;
}

// the argument checks the two molded entries share; sz8: ifx_molded_input_size's
static int mold_check(ifx* h, const char* who, int w, int hh, int min_dim, int max_dim, const double* mean, int layout, const float* d_out, int64_t out_floats,
                      int32_t* sz8, MoldSpec* m)
{
    if (!mean || !d_out) { h->err = std::string(who) + ": NULL pointer"; return IFX_E_INVALID; }
    if (layout != IFX_MOLD_NHWC && layout != IFX_MOLD_NCHW) { h->err = std::string(who) + ": unknown layout"; return IFX_E_INVALID; }
    const char* bad = ifx_detprep::molded_input_size(w, hh, min_dim, max_dim, sz8);
    if (bad) { h->err = std::string(who) + ": " + bad; return IFX_E_INVALID; }
    if (out_floats < (int64_t)3 * sz8[2] * sz8[3]) { h->err = std::string(who) + ": out_floats < 3 * S * S"; return IFX_E_INVALID; }
    m->left = sz8[5]; m->top = sz8[4]; m->nhwc = layout == IFX_MOLD_NHWC;
    for (int c = 0; c < 3; c++) m->mean[c] = mean[c];
    return IFX_OK;
}

extern "C" int ifx_detector_input_molded_image(ifx_t* h, const uint8_t* d_rgb, int width, int height, int min_dim, int max_dim, const double* mean, int layout,
                                               float* d_out, int64_t out_floats, void* stream)
{
    if (!h) return IFX_E_INVALID;
    if (!d_rgb) { h->err = "ifx_detector_input_molded_image: NULL pointer"; return IFX_E_INVALID; }
    int32_t sz[8];
    MoldSpec m;
    int r = mold_check(h, "ifx_detector_input_molded_image", width, height, min_dim, max_dim, mean, layout, d_out, out_floats, sz, &m);
    if (r) return r;
    return det_run(h, d_rgb, width, height, nullptr, sz, d_out, stream, nullptr, nullptr, &m);
}

extern "C" int ifx_detector_input_molded(ifx_t* h, int ticket, int min_dim, int max_dim, const double* mean, int layout, float* d_out, int64_t out_floats, void* stream)
{
    if (!h) return IFX_E_INVALID;
    int32_t sz[8];
    MoldSpec m;
    int r = mold_check(h, "ifx_detector_input_molded", h->w, h->h, min_dim, max_dim, mean, layout, d_out, out_floats, sz, &m);
    if (r) return r;
    const uint8_t* rgb = nullptr;
    hipEvent_t ev = nullptr;
    FrameSlot* slot = nullptr;
    if ((r = ifx_frame_for_reader(h, "ifx_detector_input_molded", ticket, &rgb, &ev, &slot))) return r;
    return det_run(h, rgb, h->w, h->h, nullptr, sz, d_out, stream, ev, slot, &m);
}

// ---- the Keras Mask R-CNN's proposal, pyramid ROI and detection layers (the rules: include/ifx_c_api.h).  stream NULL: the handle's main stream.
extern "C" int ifx_keras_proposals(ifx_t* h, const float* d_rpn_probs, const float* d_rpn_bbox, const float* d_anchors, int n, const ifx_keras_proposal_params* p,
                                   float* d_proposals, int64_t* d_index, int32_t* d_count, void* stream)
{
    if (!h) return IFX_E_INVALID;
    if (!p || !d_rpn_probs || !d_rpn_bbox || !d_anchors || !d_proposals || !d_count) { h->err = "ifx_keras_proposals: NULL pointer"; return IFX_E_INVALID; }
    if (n < 1 || n >= RPN_MAX_N) { h->err = "ifx_keras_proposals: n outside 1 .. 2^24 - 1"; return IFX_E_INVALID; }
    if (p->pre_nms_limit < 1 || p->pre_nms_limit > NMS_MAX || p->proposal_count < 1 || p->proposal_count > NMS_MAX) {
        h->err = "ifx_keras_proposals: pre_nms_limit or proposal_count outside 1 .. 8192"; return IFX_E_INVALID;
    }
    if (p->image_h < 1 || p->image_w < 1) { h->err = "ifx_keras_proposals: image_h or image_w < 1"; return IFX_E_INVALID; }
    return kp_run(h, d_rpn_probs, d_rpn_bbox, d_anchors, n, p, d_proposals, d_index, d_count, stream ? (hipStream_t)stream : h->stream);
}

extern "C" int ifx_pyramid_level_thresholds(int image_h, int image_w, float* out3)
{
    return ifx_detprep::pyramid_level_thresholds(image_h, image_w, out3) ? IFX_E_INVALID : IFX_OK;
}

extern "C" int ifx_pyramid_roi_align(ifx_t* h, const float* const* d_features, const int32_t* heights, const int32_t* widths, int batch, int channels, int layout,
                                     const float* d_boxes, int n, int image_h, int image_w, int pool_h, int pool_w, float* d_out, int32_t* d_levels, void* stream)
{
    if (!h) return IFX_E_INVALID;
    if (!d_features || !heights || !widths || !d_boxes || !d_out) { h->err = "ifx_pyramid_roi_align: NULL pointer"; return IFX_E_INVALID; }
    if (layout != 0 && layout != 1) { h->err = "ifx_pyramid_roi_align: layout is neither 0 (NCHW) nor 1 (NHWC)"; return IFX_E_INVALID; }
    if (batch < 1 || channels < 1 || n < 1 || image_h < 1 || image_w < 1) { h->err = "ifx_pyramid_roi_align: batch, channels, n, image_h or image_w < 1"; return IFX_E_INVALID; }
    if (pool_h < 1 || pool_h > PRA_TAB || pool_w < 1 || pool_w > PRA_TAB) { h->err = "ifx_pyramid_roi_align: pool_h or pool_w outside 1 .. 128"; return IFX_E_INVALID; }
    PraArgs a;
    bool vec = layout == 1 && channels % 4 == 0 && ((uintptr_t)d_out & 15) == 0;
    for (int l = 0; l < 4; l++) {
        if (!d_features[l]) { h->err = "ifx_pyramid_roi_align: NULL pointer"; return IFX_E_INVALID; }
        if (heights[l] < 1 || widths[l] < 1 || (int64_t)heights[l] * widths[l] > 0x7FFFFFFF) {
            h->err = "ifx_pyramid_roi_align: a map with a size < 1 or more than 2^31 - 1 texels"; return IFX_E_INVALID;
        }
        a.in[l] = d_features[l]; a.height[l] = heights[l]; a.width[l] = widths[l];
        vec = vec && ((uintptr_t)d_features[l] & 15) == 0;
    }
    const int64_t rows = (int64_t)batch * n, per_row = (int64_t)channels * pool_h * pool_w;
    const int64_t units = vec ? per_row / 4 : per_row, chunks = (units + PRA_UNITS - 1) / PRA_UNITS;
    if (per_row > (1 << 30) || rows * chunks > 0x7FFFFFFF) {
        h->err = "ifx_pyramid_roi_align: more than 2^30 outputs per box or more than 2^31 - 1 blocks (batch x n x ceil(outputs / 4096))"; return IFX_E_INVALID;
    }
    if (ifx_detprep::pyramid_level_thresholds(image_h, image_w, a.thr)) { h->err = "ifx_pyramid_roi_align: image_h or image_w < 1"; return IFX_E_INVALID; }
    a.boxes = d_boxes; a.out = d_out; a.lev_out = d_levels;
    a.n = n; a.channels = channels; a.ph = pool_h; a.pw = pool_w; a.chunks = (int)chunks;
    StreamScope scope(h, stream ? (hipStream_t)stream : h->stream);
    const dim3 grid((unsigned)(rows * chunks));
    if (layout == 0) LAUNCH(h, "pyramid_roi_align", grid, dim3(256), k_pyramid_roi_align<0>, a);
    else if (!vec) LAUNCH(h, "pyramid_roi_align", grid, dim3(256), k_pyramid_roi_align<1>, a);
    else LAUNCH(h, "pyramid_roi_align", grid, dim3(256), k_pyramid_roi_align<2>, a);
    return IFX_OK;
}

extern "C" int ifx_keras_detections(ifx_t* h, const float* d_rois, const float* d_probs, const float* d_deltas, int R, int C, const ifx_keras_detection_params* p,
                                    float* d_detections, float* d_boxes_norm, int64_t* d_index, int32_t* d_count, void* stream)
{
    if (!h) return IFX_E_INVALID;
    if (!p || !d_rois || !d_probs || !d_deltas || !d_detections || !d_count) { h->err = "ifx_keras_detections: NULL pointer"; return IFX_E_INVALID; }
    if (R < 1 || R > NMS_MAX || C < 2 || C > BD_MAX_C) { h->err = "ifx_keras_detections: R outside 1 .. 8192 or C outside 2 .. 1024"; return IFX_E_INVALID; }
    if (p->max_instances < 1 || p->max_instances > NMS_MAX) { h->err = "ifx_keras_detections: max_instances outside 1 .. 8192"; return IFX_E_INVALID; }
    if (p->image_h < 1 || p->image_w < 1) { h->err = "ifx_keras_detections: image_h or image_w < 1"; return IFX_E_INVALID; }
    for (int i = 0; i < 4; i++)
        if (!(std::fabs(p->window[i]) <= 16777216.f)) { h->err = "ifx_keras_detections: a window coordinate is NaN or beyond +-2^24"; return IFX_E_INVALID; }
    KdOut o;
    o.det = d_detections; o.boxes_norm = d_boxes_norm; o.index = (long long*)d_index; o.count = d_count;
    o.max_inst = p->max_instances; o.ih = (float)p->image_h; o.iw = (float)p->image_w;
    return kd_run(h, d_rois, d_probs, d_deltas, R, C, p, o, stream ? (hipStream_t)stream : h->stream);
}
