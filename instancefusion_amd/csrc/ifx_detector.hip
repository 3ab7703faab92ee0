// ifx_detector.hip -- the detector's input tensor, made on the device from the frame that is already there.
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
template <bool VEC>
__global__ void __launch_bounds__(256) k_detector_input(const DetArgs a)
{
    __shared__ int s_kx[DI_TX * DI_K], s_ky[DI_TY * DI_K];
    __shared__ int s_fx[DI_TX], s_cx[DI_TX], s_fy[DI_TY], s_cy[DI_TY];
    __shared__ uint8_t s_rows[DI_ROWS * 3 * DI_TX];
    const int t = threadIdx.x, x0 = blockIdx.x * DI_TX, y0 = blockIdx.y * DI_TY;
    const int nx = min(DI_TX, a.ow - x0), ny = min(DI_TY, a.oh - y0);   // the tile's share of the resized image (<= 0: wholly in the padding)
    const bool image = nx > 0 && ny > 0;
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
int det_run(ifx* h, const uint8_t* d_rgb, int w, int hh, const ifx_detector_prep* p, const int32_t* sz, float* d_out, void* stream, hipEvent_t ev_src, FrameSlot* slot)
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
    a.w = w; a.h = hh; a.ow = sz[0]; a.oh = sz[1]; a.Wp = sz[2]; a.Hp = sz[3]; a.ksx = t->ksx; a.ksy = t->ksy; a.flags = p->flags;
    for (int c = 0; c < 3; c++) { a.mean[c] = p->mean[c]; a.stdv[c] = p->std[c]; }
    const dim3 grid((unsigned)cdiv(a.Wp, DI_TX), (unsigned)cdiv(a.Hp, DI_TY));
    if (a.Wp % 4 == 0 && (uintptr_t)d_out % 16 == 0) LAUNCH(h, "detector_input", grid, dim3(256), k_detector_input<true>, a);
    else LAUNCH(h, "detector_input", grid, dim3(256), k_detector_input<false>, a);
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
__global__ void __launch_bounds__(256) k_roi_align(const RaArgs a)
{
    __shared__ RaSample s_y[RA_TAB], s_x[RA_TAB];
    const int t = threadIdx.x;
    const int roi = blockIdx.x / a.chunks, c0 = (blockIdx.x - roi * a.chunks) * RA_CH;
    const int bins = a.ph * a.pw, total = min(RA_CH, a.channels - c0) * bins;
    const float* r = a.rois + (size_t)roi * 5;
    float* out = a.out + ((size_t)roi * a.channels + c0) * bins;
    const float fb = r[0];
    if (!(fb > -1.f && fb < (float)a.batch)) {       // (int)fb outside 0 .. batch - 1: zeros, and no read of the input
        for (int o = t; o < total; o += 256) out[o] = 0.f;
        return;
    }
    const int b = (int)fb;
    const float sw = r[1] * a.scale, sh = r[2] * a.scale, ew = r[3] * a.scale, eh = r[4] * a.scale;
    const float dw = ew - sw, dh = eh - sh;
    const float rw = dw < 1.f ? 1.f : dw, rh = dh < 1.f ? 1.f : dh;     // std::max(d, 1): malformed ROIs are 1 x 1
    const float bh = rh / (float)a.ph, bw = rw / (float)a.pw;
    const int gh = a.ratio > 0 ? a.ratio : ra_grid(rh, a.ph), gw = a.ratio > 0 ? a.ratio : ra_grid(rw, a.pw);
    const bool tab_y = (long long)a.ph * gh <= RA_TAB, tab_x = (long long)a.pw * gw <= RA_TAB;
    if (tab_y) for (int i = t; i < a.ph * gh; i += 256) { const int p = i / gh; s_y[i] = ra_axis(sh, bh, p, i - p * gh, gh, a.height); }
    if (tab_x) for (int i = t; i < a.pw * gw; i += 256) { const int p = i / gw; s_x[i] = ra_axis(sw, bw, p, i - p * gw, gw, a.width); }
    __syncthreads();
    const float count = (float)(int)((unsigned)gh * (unsigned)gw);
    const size_t plane = (size_t)a.height * a.width;
    const float* base = a.in + ((size_t)b * a.channels + c0) * plane;
    for (int o = t; o < total; o += 256) {
        const int c = o / bins, bin = o - c * bins, py = bin / a.pw, px = bin - py * a.pw;
        const float* img = base + (size_t)c * plane;
        float acc = 0.f;
        for (int iy = 0; iy < gh; iy++) {
            const RaSample y = tab_y ? s_y[py * gh + iy] : ra_axis(sh, bh, py, iy, gh, a.height);
            if (y.lo < 0) continue;
            const float *r0 = img + (size_t)y.lo * a.width, *r1 = img + (size_t)y.hi * a.width;
            for (int ix = 0; ix < gw; ix++) {
                const RaSample x = tab_x ? s_x[px * gw + ix] : ra_axis(sw, bw, px, ix, gw, a.width);
                if (x.lo < 0) continue;
                const float w1 = y.h * x.h, w2 = y.h * x.l, w3 = y.l * x.h, w4 = y.l * x.l;
                acc += ((w1 * r0[x.lo] + w2 * r0[x.hi]) + w3 * r1[x.lo]) + w4 * r1[x.hi];
            }
        }
        out[o] = acc / count;
    }
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

// One block: a bitonic sort of P = 2^k >= n keys in LDS (the key is a total order: stability is not needed), then the boxes and groups gathered into that order.
__global__ void __launch_bounds__(1024) k_nms_sort(const float* boxes, const float* scores, const int32_t* groups, int n, int P, int32_t* order, float4* sboxes, int32_t* sgroups)
{
    __shared__ unsigned long long s_key[NMS_MAX];
    const int t = threadIdx.x;
    for (int i = t; i < P; i += 1024) s_key[i] = i < n ? nms_key(scores[i], i) : ~0ull;
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
    for (int i = t; i < n; i += 1024) {
        const int idx = (int)(uint32_t)s_key[i];
        order[i] = idx;
        sboxes[i] = make_float4(boxes[4 * (size_t)idx], boxes[4 * (size_t)idx + 1], boxes[4 * (size_t)idx + 2], boxes[4 * (size_t)idx + 3]);   // (the caller's pointer need not be 16-B aligned)
        sgroups[i] = groups ? groups[idx] : 0;
    }
}

// The pair mask, nms.cu:26-68: one wave per 64 x 64 tile of the upper triangle, bit j of word (row, cb) = row suppresses box cb * 64 + j (IoU > threshold, strictly;
// a NaN IoU compares false; same group; on the diagonal tile only j > row's lane).  max / min as fmaxf / fminf, every operation f32 and unfused, a true division.
__global__ void __launch_bounds__(64) k_nms_mask(const float4* sboxes, const int32_t* sgroups, int n, int nb, float thr, unsigned long long* mask)
{
    const int cb = blockIdx.x, rb = blockIdx.y, t = threadIdx.x;
    if (cb < rb) return;
    __shared__ float4 s_box[64];
    __shared__ int s_grp[64];
    const int cn = min(64, n - cb * 64), rn = min(64, n - rb * 64);
    if (t < cn) { s_box[t] = sboxes[cb * 64 + t]; s_grp[t] = sgroups[cb * 64 + t]; }
    __syncthreads();
    if (t >= rn) return;
    const int row = rb * 64 + t;
    const float4 a = sboxes[row];
    const int ga = sgroups[row];
    const float sa = (a.z - a.x + 1.f) * (a.w - a.y + 1.f);
    const int first = rb == cb ? t + 1 : 0;
    unsigned long long word = 0;
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

// The reduction nms.cu:99-123 does on the host, in one block, and the output.  Per 64-box block b: wave 0 takes the 64 diagonal words with one load per lane and
// resolves them in registers (64 steps of two lane reads, no memory in between); then all 16 waves OR the kept rows' words of the columns behind b into the removal
// words in LDS, 128 columns x 8 row groups, consecutive lanes on consecutive words of a row.  Two global round trips per 64 boxes, none per box.
// Then the kept flags by ORIGINAL index (LDS), a block scan, and the kept indices in ascending order, -1 behind them, the count.
__global__ void __launch_bounds__(1024) k_nms_reduce(const unsigned long long* mask, const int32_t* order, int n, int nb, long long* keep, int32_t* count)
{
    __shared__ unsigned long long s_remv[NMS_BLOCKS];
    __shared__ unsigned long long s_keepw;
    __shared__ uint8_t s_flag[NMS_MAX];
    __shared__ int s_wsum[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t < NMS_BLOCKS) s_remv[t] = 0;
    for (int i = t; i < n; i += 1024) s_flag[i] = 0;
    __syncthreads();
    for (int b = 0; b < nb; b++) {
        if (wave == 0) {
            const int row = b * 64 + lane;
            const unsigned long long d = row < n ? mask[(size_t)row * nb + b] : 0ull;
            const uint32_t dlo = (uint32_t)d, dhi = (uint32_t)(d >> 32);
            unsigned long long removed = s_remv[b], kw = 0;
#pragma unroll
            for (int i = 0; i < 64; i++) {
                const unsigned long long di = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)dhi, i) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)dlo, i);
                const unsigned long long m = ((removed >> i) & 1ull) ? 0ull : ~0ull;    // box i is kept: a suppressed box suppresses nothing
                kw |= (1ull << i) & m;
                removed |= di & m;
            }
            const int rows = min(64, n - b * 64);
            if (rows < 64) kw &= (1ull << rows) - 1ull;
            if (lane == 0) s_keepw = kw;
            if (row < n && ((kw >> lane) & 1ull)) s_flag[order[row]] = 1;
        }
        __syncthreads();
        const unsigned long long kw = s_keepw;
        const int cg = t & (NMS_BLOCKS - 1), rg = t >> 7, c = b + 1 + cg;
        if (c < nb) {
            unsigned long long acc = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int i = rg * 8 + k;
                if ((kw >> i) & 1ull) acc |= mask[(size_t)(b * 64 + i) * nb + c];    // kept rows are < n, columns behind b are in the upper triangle: all written
            }
            if (acc) atomicOr(&s_remv[c], acc);
        }
        __syncthreads();
    }
    // eight consecutive original indices per thread
    int mine = 0;
    uint32_t bits = 0;
    for (int k = 0; k < 8; k++) {
        const int i = t * 8 + k;
        if (i < n && s_flag[i]) { bits |= 1u << k; mine++; }
    }
    int incl = mine;
    for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(incl, d); if (lane >= d) incl += v; }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int pos = incl - mine, total = 0;
    for (int w = 0; w < 16; w++) { const int v = s_wsum[w]; if (w < wave) pos += v; total += v; }
    for (int k = 0; k < 8; k++)
        if (bits & (1u << k)) keep[pos++] = t * 8 + k;
    for (int i = total + t; i < n; i += 1024) keep[i] = -1;
    if (t == 0) count[0] = total;
}

// the stream the LAUNCH macro and the kernel timing use, for the length of a call on the caller's stream
struct StreamScope {
    ifx* h; hipStream_t old;
    StreamScope(ifx* hh, hipStream_t s) : h(hh), old(hh->cur) { hh->cur = s; }
    ~StreamScope() { h->cur = old; }
};

// the scratch of ifx_nms: order, sorted groups, sorted boxes, mask words; allocated by the first call, grown on demand (hipFree waits for its readers), and
// ordered across streams by an event
struct DetOps {
    void* buf = nullptr;
    int cap = 0;
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;
    bool used = false;
};

int nms_run(ifx* h, const float* d_boxes, const float* d_scores, const int32_t* d_groups, int n, float threshold, int64_t* d_keep, int32_t* d_count, hipStream_t stream)
{
    if (!h->det_ops) h->det_ops = new DetOps();
    DetOps* ops = (DetOps*)h->det_ops;
    if (!ops->ev) HIPCHK(h, hipEventCreateWithFlags(&ops->ev, hipEventDisableTiming));
    if (n > ops->cap) {
        int cap = 1024;
        while (cap < n) cap <<= 1;
        if (ops->buf) { hipFree(ops->buf); ops->buf = nullptr; ops->cap = 0; }
        const size_t bytes = (size_t)cap * (4 + 4 + 16) + (size_t)cap * (cap / 64) * 8;
        if (hipMalloc(&ops->buf, bytes) != hipSuccess) { h->err = "ifx_nms: hipMalloc of the scratch failed"; return IFX_E_HIP; }
        ops->cap = cap;
    }
    float4* sboxes = (float4*)ops->buf;                                   // 16-B records first
    unsigned long long* mask = (unsigned long long*)(sboxes + ops->cap);
    int32_t* order = (int32_t*)(mask + (size_t)ops->cap * (ops->cap / 64));
    int32_t* sgroups = order + ops->cap;
    if (ops->used && ops->last != stream) HIPCHK(h, hipStreamWaitEvent(stream, ops->ev, 0));   // the previous call may still be using the scratch on its stream
    StreamScope scope(h, stream);
    int P = 2;
    while (P < n) P <<= 1;
    const int nb = cdiv(n, 64);
    LAUNCH(h, "nms_sort", dim3(1), dim3(1024), k_nms_sort, d_boxes, d_scores, d_groups, n, P, order, sboxes, sgroups);
    LAUNCH(h, "nms_mask", dim3((unsigned)nb, (unsigned)nb), dim3(64), k_nms_mask, (const float4*)sboxes, (const int32_t*)sgroups, n, nb, threshold, mask);
    LAUNCH(h, "nms_reduce", dim3(1), dim3(1024), k_nms_reduce, (const unsigned long long*)mask, (const int32_t*)order, n, nb, (long long*)d_keep, d_count);
    HIPCHK(h, hipEventRecord(ops->ev, stream));
    ops->used = true;
    ops->last = stream;
    return IFX_OK;
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

extern "C" int ifx_nms(ifx_t* h, const float* d_boxes, const float* d_scores, const int32_t* d_groups, int n, float threshold, int64_t* d_keep, int32_t* d_count, void* stream)
{
    if (!h) return IFX_E_INVALID;
    if (n < 0 || n > NMS_MAX) { h->err = "ifx_nms: n outside 0 .. 8192"; return IFX_E_INVALID; }
    if (threshold != threshold) { h->err = "ifx_nms: the threshold is NaN"; return IFX_E_INVALID; }
    if (!d_count || (n > 0 && (!d_boxes || !d_scores || !d_keep))) { h->err = "ifx_nms: NULL pointer"; return IFX_E_INVALID; }
    if (n == 0) { HIPCHK(h, hipMemsetAsync(d_count, 0, 4, (hipStream_t)stream)); return IFX_OK; }
    return nms_run(h, d_boxes, d_scores, d_groups, n, threshold, d_keep, d_count, (hipStream_t)stream);
}
