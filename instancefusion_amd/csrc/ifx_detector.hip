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

}   // namespace

void ifx_detector_free(ifx* h)
{
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
