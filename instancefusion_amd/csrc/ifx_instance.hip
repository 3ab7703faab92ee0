// ifx_instance.hip -- instance layer of the path for gfx950.
//
// Host flow mirrors InstanceFusion::processInstance (IF/Core/InstanceFusion.cpp:655-1067) with the
// Mask-RCNN call replaced by the caller's pre-computed masks.  Device work: mask clean-up, per-pixel
// vote gathering + bounding boxes (fused; the reference materialises a 119 MB [97][H][W] int image
// first), model depth image, the vote update and the per-surfel arg-max scan over the planar vote
// store (12 fully coalesced 16-B loads per lane).  The two CPU passes of the reference (box IoU
// matching, depth flood fill) stay on the host, as in the reference.
#include <chrono>
#include "ifx_ctx.h"
#include <string.h>
#include <vector>
#include <algorithm>
#include <cmath>

#define DEAD_TIME (-1.0e9f)
#define NI IFX_NUM_INSTANCES

int ifx_superpixel_refine(ifx* h, const uint8_t* rgb, const uint16_t* depth, int nm, int frame);
int ifx_superpixel_begin(ifx* h, const uint8_t* rgb, const uint16_t* depth);
int ifx_superpixel_begin_device(ifx* h, const uint8_t* d_rgb, const uint16_t* d_depth);
int ifx_superpixel_filter(ifx* h, int nm, bool prepared = false);
int ifx_superpixel_filter_prepare(ifx* h, int nm);
int ifx_superpixel_ahead(ifx* h);

// maskCleanOverlapKernel, IF/Core/InstanceFusionCuda.cu:118-131
__global__ void k_mask_clean_overlap(uint8_t* __restrict__ masks, int nm, int P)
{
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    int flag = 0;
    for (int m = nm - 1; m >= 0; m--) {
        size_t a = (size_t)m * P + p;
        uint8_t v = masks[a];
        if (flag && v) masks[a] = 0;
        if (!flag && v) flag = 1;
    }
}
// the same from the masks as they arrived (`ori`, kept: "BAK ORI MASK") into the working copy -- the copy and the clean in one pass -- and the per-mask verdict
// bytes of the call cleared on the way (the device-side call: two dispatches less)
__global__ void k_mask_clean_overlap_from(const uint8_t* __restrict__ ori, uint8_t* __restrict__ masks, int nm, int P, uint8_t* __restrict__ unavail)
{
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (unavail && p < nm) unavail[p] = 0;
    if (p >= P) return;
    int flag = 0;
    for (int m = nm - 1; m >= 0; m--) {
        size_t a = (size_t)m * P + p;
        const uint8_t v = ori[a];
        masks[a] = (flag && v) ? (uint8_t)0 : v;
        if (!flag && v) flag = 1;
    }
}

// ---- masks already on the device (ifx_process_segmentation_device): the bridge's two steps (build/mask_ori.py:87-124 -- binarise to 0/255, stable sort by area,
// descending) in place of the host's staging copy and upload.  A mask is n x P elements of T: uint8_t (inside iff non-zero) or float (inside iff > thr; NaN is
// outside).  Loads are 16 B wide where the pointer and P allow (V elements), element-wide otherwise: the caller's tensor is only element-aligned.
__device__ __forceinline__ bool mask_inside(uint8_t v, float) { return v != 0; }
__device__ __forceinline__ bool mask_inside(float v, float thr) { return v > thr; }
// the inside bits of the V elements of a 16-B word, bit j = element j
__device__ __forceinline__ uint32_t mask_bits(uint4 q, float, const uint8_t*)
{
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    uint32_t b = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) b |= (((w[k >> 2] >> (8 * (k & 3))) & 0xffu) != 0u ? 1u : 0u) << k;
    return b;
}
__device__ __forceinline__ uint32_t mask_bits(uint4 q, float thr, const float*)
{
    return (__uint_as_float(q.x) > thr ? 1u : 0u) | (__uint_as_float(q.y) > thr ? 2u : 0u) | (__uint_as_float(q.z) > thr ? 4u : 0u) | (__uint_as_float(q.w) > thr ? 8u : 0u);
}
#define MI_THREADS 256
#define MI_ITER 4      // k_mask_area: 16-B words per thread, a block covers MI_THREADS * MI_ITER of them of one mask
// Inside pixels per mask: grid (chunks, n).  Integer counts: any order of the sums is exact.  Per wave, then across the block's waves in LDS, then one atomic per
// block.  The counters are zero on entry (k_mask_order leaves them so).
template <typename T>
__global__ void __launch_bounds__(MI_THREADS) k_mask_area(const T* __restrict__ src, int P, float thr, int* __restrict__ area)
{
    constexpr int V = 16 / sizeof(T);
    const int m = blockIdx.y, tid = threadIdx.x;
    const T* row = src + (size_t)m * P;
    const int head = min(P, (int)((V - ((uintptr_t)row / sizeof(T)) % V) % V));   // elements before the first 16-B boundary
    const int nv = (P - head) / V, tail0 = head + nv * V;
    const uint4* vrow = (const uint4*)(row + head);
    int c = 0;
    const int v0 = blockIdx.x * (MI_THREADS * MI_ITER) + tid;
    uint4 q[MI_ITER];
#pragma unroll
    for (int it = 0; it < MI_ITER; it++) { const int v = v0 + it * MI_THREADS; q[it] = v < nv ? vrow[v] : make_uint4(0, 0, 0, 0); }
#pragma unroll
    for (int it = 0; it < MI_ITER; it++) if (v0 + it * MI_THREADS < nv) c += __popc(mask_bits(q[it], thr, (const T*)nullptr));
    if (blockIdx.x == 0) {   // the unaligned head and the tail (fewer than V elements each)
        if (tid < head) c += mask_inside(row[tid], thr) ? 1 : 0;
        if (tid < P - tail0) c += mask_inside(row[tail0 + tid], thr) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    __shared__ int s_c[MI_THREADS / 64];
    if ((tid & 63) == 0) s_c[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < MI_THREADS / 64; w++) sum += s_c[w];
        if (sum) atomicAdd(&area[m], sum);
    }
}
// The bridge's order in one workgroup: rank_i = #{j : a_j > a_i} + #{j < i : a_j == a_i} (Python's sorted(..., reverse=True) is stable: ties keep their input
// order).  order[rank] = input index; the class ids follow their masks.  The counters are cleared for the next call.
__global__ void __launch_bounds__(256) k_mask_order(int* __restrict__ area, const int32_t* __restrict__ cls_in, int nm, int* __restrict__ order, int* __restrict__ cls_out)
{
    __shared__ int s_a[256];
    const int i = threadIdx.x;
    if (i < nm) { s_a[i] = area[i]; area[i] = 0; }
    __syncthreads();
    if (i >= nm) return;
    const int a = s_a[i];
    int r = 0;
    for (int j = 0; j < nm; j++) { const int b = s_a[j]; r += (b > a || (b == a && j < i)) ? 1 : 0; }
    order[r] = i;
    cls_out[r] = cls_in[i];
}
// One pass per pixel, the masks in sorted order from the last to the first (k_mask_clean_overlap_from): the binarised masks in sorted order (0/255: the
// reference's "BAK ORI MASK"), the working copy after the overlap clean, and the per-mask verdict bytes of the call cleared.  A thread takes V consecutive
// pixels: 16-B loads (4 masks in flight) and V-byte stores when every mask starts on a 16-B boundary (vec), element loads otherwise.
template <typename T>
__global__ void __launch_bounds__(MI_THREADS) k_mask_gather(const T* __restrict__ src, int P, float thr, const int* __restrict__ order, int nm, int vec,
                                                            uint8_t* __restrict__ ori, uint8_t* __restrict__ masks, uint8_t* __restrict__ unavail)
{
    constexpr int V = 16 / sizeof(T);
    __shared__ int s_ord[256];
    const int g = blockIdx.x * MI_THREADS + threadIdx.x;
    for (int t = threadIdx.x; t < nm; t += MI_THREADS) s_ord[t] = order[t];
    if (unavail && g < nm) unavail[g] = 0;
    __syncthreads();
    const int p0 = g * V;
    if (p0 >= P) return;
    const int np = min(V, P - p0);
    auto put = [&](int s, uint32_t in, uint32_t kept) {
        uint8_t* o = ori + (size_t)s * P + p0;
        uint8_t* w = masks + (size_t)s * P + p0;
        if (vec) {
            uint32_t wo[V / 4], ww[V / 4];
#pragma unroll
            for (int k = 0; k < V / 4; k++) { wo[k] = 0; ww[k] = 0; }
#pragma unroll
            for (int j = 0; j < V; j++) { wo[j >> 2] |= ((in >> j) & 1u) * (0xffu << (8 * (j & 3))); ww[j >> 2] |= ((kept >> j) & 1u) * (0xffu << (8 * (j & 3))); }
            if constexpr (V == 16) { *(uint4*)o = make_uint4(wo[0], wo[1], wo[2], wo[3]); *(uint4*)w = make_uint4(ww[0], ww[1], ww[2], ww[3]); }
            else { *(uint32_t*)o = wo[0]; *(uint32_t*)w = ww[0]; }
        } else {
            for (int j = 0; j < np; j++) { o[j] = ((in >> j) & 1u) ? 255 : 0; w[j] = ((kept >> j) & 1u) ? 255 : 0; }
        }
    };
    uint32_t flag = 0;   // bit j: pixel p0 + j lies in a mask later in the sorted order
    int s = nm - 1;
    if (vec) {
        for (; s >= 3; s -= 4) {
            uint4 q[4];
#pragma unroll
            for (int k = 0; k < 4; k++) q[k] = *(const uint4*)(src + (size_t)s_ord[s - k] * P + p0);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t in = mask_bits(q[k], thr, (const T*)nullptr);
                put(s - k, in, in & ~flag);
                flag |= in;
            }
        }
    }
    for (; s >= 0; s--) {
        const T* row = src + (size_t)s_ord[s] * P + p0;
        uint32_t in;
        if (vec) in = mask_bits(*(const uint4*)row, thr, (const T*)nullptr);
        else { in = 0; for (int j = 0; j < np; j++) in |= (mask_inside(row[j], thr) ? 1u : 0u) << j; }
        put(s, in, in & ~flag);
        flag |= in;
    }
}

// ---- the mask head's own output (ifx_process_segmentation_rois): n ROI masks of M x M probabilities and n boxes, pasted into the image as maskrcnn-benchmark's
// Masker does on the CPU (paste_mask_in_image with expand_masks / expand_boxes, maskrcnn_benchmark/modeling/roi_heads/mask_head/inference.py:91-154: one sample of
// zero padding, the box grown by (M + 2) / M and truncated to integers, bilinear resize with align_corners = False to the box, > threshold, clip to the image).
// The arithmetic is the CPU statement's (tests/roi_paste_numpy.py), operation for operation in f32 with no contraction, so both kernels here and that statement
// decide every pixel alike.  Where the reference raises -- a box with no pixel in the image, a non-finite coordinate, one beyond +-2^24 -- the mask is empty.
#define ROI_M_MAX 64
#define ROI_PX 16      // consecutive pixels per thread
struct RoiRec { int b0, b1, X0, X1, Y0, Y1; float sx, sy; };   // the expanded integer box's corner, the clip rectangle [X0,X1) x [Y0,Y1) (empty: all zero), S / w and S / h
__device__ __forceinline__ RoiRec roi_record(const float* __restrict__ box, int S, float scale, int W, int H)
{
    const float x0 = box[0], y0 = box[1], x1 = box[2], y1 = box[3];
    RoiRec r = {0, 0, 0, 0, 0, 0, 0.f, 0.f};
    const float lim = 16777216.f;
    if (!(fabsf(x0) <= lim && fabsf(y0) <= lim && fabsf(x1) <= lim && fabsf(y1) <= lim)) return r;   // (NaN fails every comparison)
    float wh = (x1 - x0) * 0.5f, hh = (y1 - y0) * 0.5f;
    const float xc = (x1 + x0) * 0.5f, yc = (y1 + y0) * 0.5f;
    wh *= scale; hh *= scale;
    const int b0 = (int)(xc - wh), b1 = (int)(yc - hh), b2 = (int)(xc + wh), b3 = (int)(yc + hh);   // toward zero, as Tensor.to(int32); |b| < 2^26
    const int w = max(b2 - b0 + 1, 1), h = max(b3 - b1 + 1, 1);
    const int X0 = max(b0, 0), X1 = min(b2 + 1, W), Y0 = max(b1, 0), Y1 = min(b3 + 1, H);
    if (X1 <= X0 || Y1 <= Y0) return r;
    r.b0 = b0; r.b1 = b1; r.X0 = X0; r.X1 = X1; r.Y0 = Y0; r.Y1 = Y1;
    r.sx = __fdiv_rn((float)S, (float)w); r.sy = __fdiv_rn((float)S, (float)h);
    return r;
}
// source samples and weights of destination offset d on one axis (the resize's area_pixel source index, clamped at 0)
struct RoiAxis { int i0, i1; float l0, l1; };
__device__ __forceinline__ RoiAxis roi_axis(float s, int d, int S)
{
    const float r = fmaxf(s * ((float)d + 0.5f) - 0.5f, 0.f);
    RoiAxis a;
    a.i0 = min((int)r, S - 1);
    a.i1 = min(a.i0 + 1, S - 1);
    a.l1 = r - (float)a.i0;
    a.l0 = 1.f - a.l1;
    return a;
}
__device__ __forceinline__ float roi_blend(const RoiAxis& ay, const RoiAxis& ax, float p00, float p01, float p10, float p11)
{
    return ay.l0 * (ax.l0 * p00 + ax.l1 * p01) + ay.l1 * (ax.l0 * p10 + ax.l1 * p11);
}
// Inside pixels per ROI: grid (chunks, n), a block takes MI_THREADS * ROI_PX pixels of its ROI's clip rectangle in row-major order.  The rectangle is only known
// here, so the grid covers a whole image per ROI and the blocks past the rectangle leave at once.  The padded mask is staged in LDS, its border written here.
// Sums as k_mask_area: per wave, per block in LDS, one atomic per block; the counters are zero on entry.
__global__ void __launch_bounds__(MI_THREADS) k_roi_area(const float* __restrict__ rois, int M, const float* __restrict__ boxes, float scale, float thr, int W, int H, int* __restrict__ area)
{
    __shared__ float s_pm[(ROI_M_MAX + 2) * (ROI_M_MAX + 2)];
    __shared__ int s_c[MI_THREADS / 64];
    const int m = blockIdx.y, tid = threadIdx.x, S = M + 2;
    const RoiRec rc = roi_record(boxes + 4 * m, S, scale, W, H);
    const int rw = rc.X1 - rc.X0, n_px = rw * (rc.Y1 - rc.Y0);
    if (blockIdx.x * (MI_THREADS * ROI_PX) >= n_px) return;   // (the whole block)
    const float* src = rois + (size_t)m * M * M;
    for (int t = tid; t < S * S; t += MI_THREADS) {
        const int r = t / S, c = t - r * S;
        s_pm[t] = (r == 0 || r == S - 1 || c == 0 || c == S - 1) ? 0.f : src[(r - 1) * M + (c - 1)];
    }
    __syncthreads();
    int c = 0;
    const int i0 = (blockIdx.x * MI_THREADS + tid) * ROI_PX;
    if (i0 < n_px) {
        const int cnt = min(ROI_PX, n_px - i0);
        int ry = i0 / rw, rx = i0 - ry * rw;
        RoiAxis ay = roi_axis(rc.sy, rc.Y0 + ry - rc.b1, S);
        for (int j = 0; j < cnt; j++) {
            const RoiAxis ax = roi_axis(rc.sx, rc.X0 + rx - rc.b0, S);
            const float* r0 = s_pm + ay.i0 * S;
            const float* r1 = s_pm + ay.i1 * S;
            c += roi_blend(ay, ax, r0[ax.i0], r0[ax.i1], r1[ax.i0], r1[ax.i1]) > thr ? 1 : 0;
            if (++rx == rw) { rx = 0; ry++; ay = roi_axis(rc.sy, rc.Y0 + ry - rc.b1, S); }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((tid & 63) == 0) s_c[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < MI_THREADS / 64; w++) sum += s_c[w];
        if (sum) atomicAdd(&area[m], sum);
    }
}
// k_mask_gather's pass with the paste in place of the load: the ROIs in sorted order from the last to the first, a thread owns ROI_PX consecutive pixels (they
// may run over the end of a row; P is a multiple of 16 because width and height are multiples of 4, ifx_create), writes the 0/255 masks in sorted order and the overlap-cleaned copy, and the verdict bytes are cleared.  The per-ROI records sit
// in LDS in sorted order; a group that misses a ROI's clip rectangle stores zeros without evaluating anything; otherwise the y terms are shared along the row.
// The samples come through the cache (all ROIs of a call: a few KB to 4 MB); the border of the padded mask is never read.
__global__ void __launch_bounds__(MI_THREADS) k_roi_gather(const float* __restrict__ rois, int M, const float* __restrict__ boxes, float scale, float thr, int W, int H,
                                                           const int* __restrict__ order, int nm, uint8_t* __restrict__ ori, uint8_t* __restrict__ masks,
                                                           uint8_t* __restrict__ unavail)
{
    __shared__ RoiRec s_rec[256];
    __shared__ int s_src[256];
    const int P = W * H, S = M + 2, MM = M * M;
    const int g = blockIdx.x * MI_THREADS + threadIdx.x;
    for (int t = threadIdx.x; t < nm; t += MI_THREADS) {
        const int src = order[t];
        s_src[t] = src;
        s_rec[t] = roi_record(boxes + 4 * src, S, scale, W, H);
    }
    if (unavail && g < nm) unavail[g] = 0;
    __syncthreads();
    const int p0 = g * ROI_PX;
    if (p0 >= P) return;
    constexpr int np = ROI_PX;
    const int ya = p0 / W, xa = p0 - ya * W, yb = (p0 + np - 1) / W;
    uint32_t flag = 0;   // bit j: pixel p0 + j lies in a mask later in the sorted order
    for (int s = nm - 1; s >= 0; s--) {
        const RoiRec rc = s_rec[s];
        uint32_t in = 0;
        const bool miss = yb < rc.Y0 || ya >= rc.Y1 || (ya == yb && (xa + np <= rc.X0 || xa >= rc.X1));
        if (!miss) {
            const float* src = rois + (size_t)s_src[s] * MM;
            auto sample = [&](int yi, int xi) { return (yi >= 1 && yi <= M && xi >= 1 && xi <= M) ? src[(yi - 1) * M + (xi - 1)] : 0.f; };
            int x = xa, y = ya;
            bool yin = y >= rc.Y0 && y < rc.Y1;
            RoiAxis ay = roi_axis(rc.sy, yin ? y - rc.b1 : 0, S);
            for (int j = 0; j < np; j++) {
                if (yin && x >= rc.X0 && x < rc.X1) {
                    const RoiAxis ax = roi_axis(rc.sx, x - rc.b0, S);
                    in |= (roi_blend(ay, ax, sample(ay.i0, ax.i0), sample(ay.i0, ax.i1), sample(ay.i1, ax.i0), sample(ay.i1, ax.i1)) > thr ? 1u : 0u) << j;
                }
                if (++x == W) { x = 0; y++; yin = y >= rc.Y0 && y < rc.Y1; ay = roi_axis(rc.sy, yin ? y - rc.b1 : 0, S); }
            }
        }
        const uint32_t kept = in & ~flag;
        flag |= in;
        uint8_t* o = ori + (size_t)s * P + p0;
        uint8_t* w = masks + (size_t)s * P + p0;
        uint32_t wo[4] = {0, 0, 0, 0}, ww[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < ROI_PX; j++) { wo[j >> 2] |= ((in >> j) & 1u) * (0xffu << (8 * (j & 3))); ww[j >> 2] |= ((kept >> j) & 1u) * (0xffu << (8 * (j & 3))); }
        *(uint4*)o = make_uint4(wo[0], wo[1], wo[2], wo[3]);
        *(uint4*)w = make_uint4(ww[0], ww[1], ww[2], ww[3]);
    }
}

// ---- the device forms of a segmentation call on a sharded map (ifx_owner_segmentation_begin_device / _rois / _detections): the detector's rank packs what the
// other ranks need into one record of int32 words (layout: include/ifx_c_api.h), one broadcast carries it, every rank ingests from it.
//   header[8] | cls[max_n] | form 2: boxes f32[max_n][4], rois f32[max_n][M][M] | form 1: bits u32[max_n][ceil(P / 32)]
#define OSEG_MAGIC 0x49465852   // "IFXR"
#define OSEG_HDR 8
// header and class ids (the caller's order; rows >= n are zero).  n_hdr is n, or -- the detections form with more kept rows than the record holds -- that number with no rows
__global__ void __launch_bounds__(256) k_oseg_head(int32_t* __restrict__ rec, int form, int n_hdr, int n, int M, int P, int max_n, const int32_t* __restrict__ cls)
{
    const int hdr[OSEG_HDR] = {OSEG_MAGIC, form, n_hdr, M, P, max_n, 0, 0};
    for (int t = threadIdx.x; t < OSEG_HDR + max_n; t += 256) {
        int v = 0;
        if (t < OSEG_HDR) {
#pragma unroll
            for (int k = 0; k < OSEG_HDR; k++) if (t == k) v = hdr[k];
        } else if (t - OSEG_HDR < n) v = cls[t - OSEG_HDR];
        rec[t] = v;
    }
}
// form 2: n rows of boxes and ROI masks as they are, the tail zero.  dst = the record behind the class ids: [max_n * 4 | max_n * MM] words
__global__ void __launch_bounds__(256) k_oseg_pack_rois(uint32_t* __restrict__ dst, int n, int max_n, int MM, const uint32_t* __restrict__ boxes, const uint32_t* __restrict__ rois)
{
    const size_t nb = (size_t)max_n * 4, total = nb + (size_t)max_n * MM;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        uint32_t v = 0;
        if (t < nb) { if (t < (size_t)n * 4) v = boxes[t]; }
        else if (t - nb < (size_t)n * MM) v = rois[t - nb];
        dst[t] = v;
    }
}
// form 1: one pass over the caller's n x P elements to one bit per pixel, binarised by the bridge's rule (mask_inside); grid (chunks, max_n), rows >= n come out zero
// without a load.  Every lane of a wave stays to the end (ballot and shuffles).  vec: every row starts on a 16-B boundary -- a lane loads 16 B (V elements, V bits),
// the 32 / V lanes of a word OR their bits together and the first of them stores the word; otherwise a lane takes one pixel and the wave's ballot over its 64
// consecutive pixels is two words, stored by lanes 0 and 32 (the upper one only where the row still has it: P % 64 may be 32 or less).  Pixels past P give zero bits.
template <typename T>
__global__ void __launch_bounds__(MI_THREADS) k_oseg_pack_bits(const T* __restrict__ src, int P, float thr, int n, int vec, uint32_t* __restrict__ bits)
{
    constexpr int V = 16 / sizeof(T), LPW = 32 / V;
    const int m = blockIdx.y, NW = (P + 31) >> 5;
    const int g = blockIdx.x * MI_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    uint32_t* out = bits + (size_t)m * NW;
    const T* row = src + (size_t)m * P;
    if (vec) {
        uint32_t b = 0;
        if (m < n && g < P / V) b = mask_bits(*(const uint4*)(row + (size_t)g * V), thr, (const T*)nullptr) << (V * (lane % LPW));
#pragma unroll
        for (int o = 1; o < LPW; o <<= 1) b |= __shfl_xor(b, o, 64);
        const int j = g / LPW;
        if (lane % LPW == 0 && j < NW) out[j] = b;
    } else {
        const bool in = m < n && g < P && mask_inside(row[g], thr);
        const unsigned long long w = __ballot(in);
        const int j = (g - lane) >> 5;   // the wave's first word
        if (lane == 0 && j < NW) out[j] = (uint32_t)w;
        if (lane == 32 && j + 1 < NW) out[j + 1] = (uint32_t)(w >> 32);
    }
}
// ingest from the bits: the areas are popcounts (sums as k_mask_area: per wave, per block in LDS, one atomic per block; the counters are zero on entry) ...
__global__ void __launch_bounds__(MI_THREADS) k_bits_area(const uint32_t* __restrict__ bits, int NW, int* __restrict__ area)
{
    __shared__ int s_c[MI_THREADS / 64];
    const int m = blockIdx.y, tid = threadIdx.x, j = blockIdx.x * MI_THREADS + tid;
    int c = j < NW ? __popc(bits[(size_t)m * NW + j]) : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((tid & 63) == 0) s_c[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < MI_THREADS / 64; w++) sum += s_c[w];
        if (sum) atomicAdd(&area[m], sum);
    }
}
// ... and k_mask_gather's pass with half a word in place of the load: a thread owns 16 consecutive pixels (P is a multiple of 16, ifx_create), the masks in sorted
// order from the last to the first, 0/255 in sorted order and the overlap-cleaned copy as one 16-B store each, the verdict bytes cleared.
__global__ void __launch_bounds__(MI_THREADS) k_bits_gather(const uint32_t* __restrict__ bits, int NW, int P, const int* __restrict__ order, int nm,
                                                            uint8_t* __restrict__ ori, uint8_t* __restrict__ masks, uint8_t* __restrict__ unavail)
{
    __shared__ int s_ord[256];
    const int g = blockIdx.x * MI_THREADS + threadIdx.x;
    for (int t = threadIdx.x; t < nm; t += MI_THREADS) s_ord[t] = order[t];
    if (unavail && g < nm) unavail[g] = 0;
    __syncthreads();
    const int p0 = g * 16;
    if (p0 >= P) return;
    const int j = g >> 1, sh = (g & 1) * 16;
    uint32_t flag = 0;   // bit k: pixel p0 + k lies in a mask later in the sorted order
    for (int s = nm - 1; s >= 0; s--) {
        const uint32_t in = (bits[(size_t)s_ord[s] * NW + j] >> sh) & 0xffffu;
        const uint32_t kept = in & ~flag;
        flag |= in;
        uint32_t wo[4] = {0, 0, 0, 0}, ww[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 16; k++) { wo[k >> 2] |= ((in >> k) & 1u) * (0xffu << (8 * (k & 3))); ww[k >> 2] |= ((kept >> k) & 1u) * (0xffu << (8 * (k & 3))); }
        *(uint4*)(ori + (size_t)s * P + p0) = make_uint4(wo[0], wo[1], wo[2], wo[3]);
        *(uint4*)(masks + (size_t)s * P + p0) = make_uint4(ww[0], ww[1], ww[2], ww[3]);
    }
}

// checkProjectDepthAndInstanceKernel, IF/Core/InstanceFusionCuda.cu:736-760
__global__ void k_check_project(const DevState* __restrict__ st, const int32_t* __restrict__ ids, const float4* __restrict__ votes, int cap, int w, int h, int downsample,
                                int* __restrict__ counts)
{
    int gx = blockIdx.x * blockDim.x + threadIdx.x, gy = blockIdx.y * blockDim.y + threadIdx.y;
    int x = gx * downsample, y = gy * downsample;
    if (x >= w || y >= h) return;
    int id = ids[y * w + x];
    if (id > 0 && id < st->count) {
        int s = 0;
        for (int q = 0; q < 12; q++) {
            float4 v = VOTE4(votes, id, q);
            int a, b;
            vote_decode(v.x, a, b); s += a + b;
            vote_decode(v.y, a, b); s += a + b;
            vote_decode(v.z, a, b); s += a + b;
            vote_decode(v.w, a, b); s += a + b;
        }
        atomicAdd(&counts[0], s);
    } else atomicAdd(&counts[1], 1);
}

// getProjectInstanceListKernel + computeProjectBoundingBoxKernel fused,
// IF/Core/InstanceFusionCuda.cu:781-807, 909-952.  bbox layout: [96][4] project boxes then [nm][4] mask boxes.
__global__ void k_init_bbox(int* __restrict__ bbox, int n, int w, int h)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * 4) return;
    int t = i & 3;
    bbox[i] = t == 0 ? w + 1 : t == 1 ? -1 : t == 2 ? h + 1 : -1;
}
// extend a box {minX, maxX, minY, maxY}: almost every pixel lies inside the box already, so look (L2, no contention)
// before the atomic; a stale look can only cause a redundant atomic, never skip a needed one
__device__ __forceinline__ void bbox_extend(int* b, int x, int y)
{
    if (x < __hip_atomic_load(&b[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&b[0], x);
    if (x > __hip_atomic_load(&b[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&b[1], x);
    if (y < __hip_atomic_load(&b[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&b[2], y);
    if (y > __hip_atomic_load(&b[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&b[3], y);
}
// The pixels of a wave (2 rows x 32 columns of the 32 x 8 block) that extend the same box are reduced in the wave first: their ballot IS the reduction -- lowest /
// highest set bit of each row's half give min / max x, which halves are non-empty min / max y -- so a box costs a few scalar operations, one look and at most four
// atomics per wave (first four memory-side looks per pixel and box, then four shuffle reductions of six steps per box; the twelve vote floats4 and the mask bytes of a
// pixel are fetched in one batch each).  min / max commute: same boxes.
__device__ __forceinline__ void bbox_extend_ballot_lds(int* b, unsigned long long bal, int xb, int yb)
{
    const unsigned int lo = (unsigned int)bal, hi = (unsigned int)(bal >> 32);
    const int x0 = xb + min(lo ? __ffs(lo) - 1 : 32, hi ? __ffs(hi) - 1 : 32), x1 = xb + max(lo ? 31 - __clz(lo) : -1, hi ? 31 - __clz(hi) : -1);
    const int y0 = yb + (lo ? 0 : 1), y1 = yb + (hi ? 1 : 0);
    atomicMin(&b[0], x0); atomicMax(&b[1], x1); atomicMin(&b[2], y0); atomicMax(&b[3], y1);
}
// a block's box into the global one: almost every box lies inside it already, so look (L2) before the atomic; a stale look can only cause a redundant atomic
__device__ __forceinline__ void bbox_extend_box(int* b, const int* sb)
{
    if (sb[0] < __hip_atomic_load(&b[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&b[0], sb[0]);
    if (sb[1] > __hip_atomic_load(&b[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&b[1], sb[1]);
    if (sb[2] < __hip_atomic_load(&b[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&b[2], sb[2]);
    if (sb[3] > __hip_atomic_load(&b[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&b[3], sb[3]);
}
#define PB_ROWS 32   // k_project_bbox: blocks of 32 x PB_ROWS pixels
// MODE 0: instance boxes and mask boxes (the reference's two kernels as one).  The device-scheduled call splits them: MODE 1, the instance boxes -- the twelve vote
// float4 of every pixel's surfel, the heavy half, and nothing of the masks -- is on the queue BEFORE the host copies the masks into pinned memory (and writes the model
// depth under every pixel on the way: getProjectDepthMapKernel reads the same id); MODE 2, the mask boxes, follows the masks and needs one vote float4 per pixel.
// MODE 3 (option compare_map 2): MODE 1 plus the presence image of the mask rule -- bit i of a pixel's 96 says "counter i of the surfel under it is > 0"
// (instanceProjectMap[i][p] > 0 of getProjectInstanceListKernel, :781-807; no surfel: no bit) -- from the counters the pass decodes anyway.
template <int MODE>
__global__ void __launch_bounds__(32 * PB_ROWS) k_project_bbox(const DevState* __restrict__ st, const int32_t* __restrict__ ids, const float4* __restrict__ votes, int cap, const uint8_t* __restrict__ masks,
                               int nm, int w, int h, int* __restrict__ bbox, IdMap im, const float4* __restrict__ pc = nullptr, uint16_t* __restrict__ pdm = nullptr,
                               const float* __restrict__ cam = nullptr,   // cam: the row-major pose whose translation is the camera centre (SegView::cam; MODE 1 / 3 only)
                               uint4* __restrict__ pres = nullptr)       // MODE 3: [P] presence words (x, y, z: instances 0-31, 32-63, 64-95)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    const int lane = (threadIdx.y * blockDim.x + threadIdx.x) & 63;
    const int xb = blockIdx.x * 32, yb = blockIdx.y * blockDim.y + (threadIdx.y & ~1);   // origin of this wave's 32 x 2 pixels (blocks of 32 x PB_ROWS)
    // Boxes of the block first, in LDS: a wave that went to the global box itself made every box a hot spot of one L2 channel (4800 waves x a handful of boxes x four
    // looks at the same few lines: most of the kernel's 85 us); now a block of 16 waves settles in LDS and sends one look per box it touched.
    __shared__ int s_box[NI + 8][4];
    const int tid = threadIdx.y * blockDim.x + threadIdx.x, nthreads = blockDim.x * blockDim.y;
    for (int t = tid; t < (NI + 8) * 4; t += nthreads) s_box[t >> 2][t & 3] = (t & 1) ? (int)0x80000000 : 0x7fffffff;
    __syncthreads();
    const bool inside = x < w && y < h;
    const int P = w * h, k = inside ? y * w + x : 0;
    const int gid = inside ? ids[k] : 0;
    const int id = MODE == 0 ? segmap_slot(im, st->count, gid) : idmap_slot(im, st->count, gid);   // (MODE 0 is the sharded call's: its deferred form hands it slots; sharded map: the pixels whose surfel another rank owns extend that rank's partial boxes)
    bool has = inside && id >= 0;
    int maxNum = 0, maxID = -1, first = 0;
    if ((MODE == 1 || MODE == 3) && pdm && inside) {   // getProjectDepthMapKernel (k_project_depth) on the way
        uint16_t o = 0;
        if (id >= 0) {
            const float4 p = pc[id];
            const float dx = cam[3] - p.x, dy = cam[7] - p.y, dz = cam[11] - p.z;
            o = (uint16_t)(sqrtf(dx * dx + dy * dy + dz * dz) * 1186);
        }
        pdm[k] = o;
    }
    unsigned int pw[3] = {0u, 0u, 0u};
    if (MODE == 2) {
        if (has) { int b_; vote_decode(VOTE4(votes, id, 0).x, first, b_); }
    } else if (has) {
        float4 v[12];
#pragma unroll
        for (int q = 0; q < 12; q++) v[q] = VOTE4(votes, id, q);
#pragma unroll
        for (int q = 0; q < 12; q++) {
            const float f[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
            for (int t = 0; t < 4; t++) {
                int a, b;
                vote_decode(f[t], a, b);
                if (q == 0 && t == 0) first = a;
                if (a > maxNum) { maxNum = a; maxID = (q * 4 + t) * 2; }
                if (b > maxNum) { maxNum = b; maxID = (q * 4 + t) * 2 + 1; }
                if (MODE == 3) pw[q / 4] |= (a > 0 ? 1u << ((q * 4 + t) * 2 & 31) : 0u) | (b > 0 ? 1u << (((q * 4 + t) * 2 + 1) & 31) : 0u);
            }
        }
    }
    if (MODE == 3 && inside) pres[k] = make_uint4(pw[0], pw[1], pw[2], 0u);
    if (first == -1) has = false;   // instanceProjectMap[y*width+x] != -1 test (:915)
    // boxes of the projected instances: one reduction per distinct arg-max id in the wave (a wave rarely sees more than two or three)
    const int key = (MODE != 2 && has && maxID != -1) ? maxID : -1;
    unsigned long long todo = __ballot(key >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int pick = __shfl(key, leader, 64);
        const unsigned long long grp = __ballot(key == pick);
        if (lane == leader) bbox_extend_ballot_lds(s_box[pick], grp, xb, yb);
        todo &= ~grp;
    }
    // boxes of the masks
    for (int m0 = 0; (MODE == 0 || MODE == 2) && m0 < nm; m0 += 8) {
        uint8_t mb[8];
#pragma unroll
        for (int u = 0; u < 8; u++) mb[u] = (has && m0 + u < nm) ? masks[(size_t)(m0 + u) * P + k] : (uint8_t)0;
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const unsigned long long bal = __ballot(mb[u] > 0);
            if (bal && lane == u) bbox_extend_ballot_lds(s_box[NI + u], bal, xb, yb);
        }
        __syncthreads();
        if (tid < 8 && s_box[NI + tid][1] >= s_box[NI + tid][0]) bbox_extend_box(&bbox[(NI + m0 + tid) * 4], s_box[NI + tid]);
        if (m0 + 8 < nm) {   // (uniform) another chunk of masks follows: re-arm their eight boxes
            __syncthreads();
            if (tid < 32) s_box[NI + (tid >> 2)][tid & 3] = (tid & 1) ? (int)0x80000000 : 0x7fffffff;
            __syncthreads();
        }
    }
    __syncthreads();
    if (MODE != 2 && tid < NI && s_box[tid][1] >= s_box[tid][0]) bbox_extend_box(&bbox[tid * 4], s_box[tid]);
}

// getProjectDepthMapKernel, IF/Core/InstanceFusionCuda.cu:977-996
__global__ void k_project_depth(const DevState* __restrict__ st, const int32_t* __restrict__ ids, const float4* __restrict__ pc, int P, int ratio, uint16_t* __restrict__ pdm, IdMap im,
                                const float* __restrict__ cam)   // cam: the row-major pose whose translation is the camera centre (SegView::cam)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P) return;
    const int id = segmap_slot(im, st->count, ids[k]);
    uint16_t o = 0;
    if (id >= 0) {
        float4 p = pc[id];
        float dx = cam[3] - p.x, dy = cam[7] - p.y, dz = cam[11] - p.z;
        o = (uint16_t)(sqrtf(dx * dx + dy * dy + dz * dz) * ratio);
    }
    pdm[k] = o;
}

// updateSurfelMapInstanceKernel, IF/Core/InstanceFusionCuda.cu:1100-1139 (deleteNum = -1).  Like the
// reference this is a non-atomic read-modify-write: several pixels of one mask can see the same surfel;
// an atomicCAS loop makes the result independent of scheduling (every pixel's increment lands), which
// is also what the sequential oracle computes.
__global__ void k_vote_update(const DevState* __restrict__ st, const int32_t* __restrict__ ids, const uint8_t* __restrict__ mask, int P, int cap, int instanceID, int inc,
                              float* __restrict__ votes, IdMap im)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P) return;
    if (!(mask[k] > 0)) return;
    const int id = segmap_slot(im, st->count, ids[k]);
    if (id < 0) return;
    int fi = instanceID / 2, p = instanceID % 2;
    // planar float4 store: float fi of surfel id lives in plane fi/4, component fi%4
    unsigned int* addr = (unsigned int*)&VOTEF(votes, id, fi);
    unsigned int old = *addr, assumed;
    do {
        assumed = old;
        int a, b;
        vote_decode(__uint_as_float(assumed), a, b);
        if (p == 0) a += inc; else b += inc;
        if (a >= 65535) a = 65535;
        if (b >= 65535) b = 65535;
        old = atomicCAS(addr, assumed, __float_as_uint(vote_encode(a, b)));
    } while (old != assumed);
}

// countAndColourSurfelMapKernel, IF/Core/InstanceFusionCuda.cu:1158-1200: the label scan.  Per surfel
// 192 B of votes read as 12 coalesced float4 plane loads + 8 B colour RMW + 4 B label.
// countAndColourSurfelMapKernel restricted to what a segmentation call can have changed.  A call changes votes only of the surfels under the
// id image (k_vote_update), so labels and colours of all other surfels are what the previous scan left -- except the surfels created since then,
// which the full scan would move from "no colour" (0) to the default colour: pass A does that from 16 bytes per slot, pass B redoes the arg-max
// for the surfel under every pixel (192 bytes each, <= P of them) exactly as the full scan would.  5 M surfels: 83 MB + <= 59 MB instead of
// 1.1 GB.  Anything that rewrites votes wholesale (upload, table eviction) sets ifx::labels_stale_all and the next call scans everything.
// `gate` (all three scan kernels): the first two words of the device-side call's control block (SegCtl: ff_incomplete, evict_at).  A call that cannot finish on the
// device -- the flood fill needs more relaxations, the table is full at some mask -- must not colour anything yet: colours are assigned ONCE (c.y == 0 or the
// default), and an instance registered before an eviction may be gone after it.  The scan then runs once, behind the host-driven tail, as in the reference.
#define SCAN_GATED(gate) ((gate) && ((gate)[0] != 0 || (gate)[1] >= 0))
__global__ __launch_bounds__(256) void k_colour_default(const DevState* __restrict__ st, const float2* __restrict__ tm, float2* __restrict__ col, int32_t* __restrict__ labels,
                                                        const int* __restrict__ gate)
{
    if (SCAN_GATED(gate)) return;
    const float defaultColor = 7434609;
    const int n = st->count;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += blockDim.x * gridDim.x) {
        const float2 c = col[i];
        const bool live = tm[i].y > DEAD_TIME;
        if (c.y == 0 && live) col[i] = make_float2(c.x, defaultColor);   // (votes untouched since creation: no label, the default colour)
        if (!live && labels[i] != -1) labels[i] = -1;                    // a tombstone carries no label, as in the full scan (visible through ifx_owner_knn_export until a compaction)
    }
}
__global__ __launch_bounds__(256) void k_count_colour_px(const DevState* __restrict__ st, const int32_t* __restrict__ ids, int P, const float4* __restrict__ votes, int cap,
                                                         const float2* __restrict__ tm, float2* __restrict__ col, const float* __restrict__ inst_color, int32_t* __restrict__ labels,
                                                         IdMap im, const int* __restrict__ gate)
{
    if (SCAN_GATED(gate)) return;
    const float defaultColor = 7434609;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P) return;
    const int i = idmap_slot(im, st->count, ids[k]);
    if (i < 0) return;
    float4 v[12];
#pragma unroll
    for (int q = 0; q < 12; q++) v[q] = VOTE4(votes, i, q);
    int best = -1, bestCount = 0;
#pragma unroll
    for (int q = 0; q < 12; q++) {
        float f[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
        for (int t = 0; t < 4; t++) {
            int a, b;
            vote_decode(f[t], a, b);
            if (bestCount < a) { bestCount = a; best = (q * 4 + t) * 2; }
            if (bestCount < b) { bestCount = b; best = (q * 4 + t) * 2 + 1; }
        }
    }
    if (tm[i].y <= DEAD_TIME) { labels[i] = -1; return; }
    labels[i] = best;          // (several pixels can show the same surfel: they all write the same values)
    float2 c = col[i];
    if (c.y == 0 || c.y == defaultColor) {
        c.y = (best != -1) ? inst_color[best] : defaultColor;
        col[i] = c;
    }
}
__global__ __launch_bounds__(256) void k_count_colour(const DevState* __restrict__ st, const float4* __restrict__ votes, int cap, const float2* __restrict__ tm,
                                                      float2* __restrict__ col, const float* __restrict__ inst_color, int32_t* __restrict__ labels, const int* __restrict__ gate)
{
    if (SCAN_GATED(gate)) return;
    // the whole map: four lanes per surfel, each instruction of a wave reads 16 x 64 contiguous bytes of the 192-byte records; the arg-max of the four quarters is
    // merged "larger count, then smaller index" = the sequential first-maximum rule
    (void)cap;
    const float defaultColor = 7434609;
    const int n = st->count, r = threadIdx.x & 3;
    const int per = blockDim.x >> 2;
    for (int i0 = blockIdx.x * per; i0 < n; i0 += per * gridDim.x) {   // (uniform trip count per block: the shuffles below see whole groups)
        const int i = i0 + (threadIdx.x >> 2);
        int best = -1, bestCount = 0;
        if (i < n) {
            float4 v[3];
#pragma unroll
            for (int j = 0; j < 3; j++) v[j] = VOTE4(votes, i, j * 4 + r);
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int q = j * 4 + r;
                float f[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    int a, b;
                    vote_decode(f[t], a, b);
                    if (bestCount < a) { bestCount = a; best = (q * 4 + t) * 2; }
                    if (bestCount < b) { bestCount = b; best = (q * 4 + t) * 2 + 1; }
                }
            }
        }
#pragma unroll
        for (int o = 1; o < 4; o <<= 1) {
            const int oc = __shfl_xor(bestCount, o, 64), ob = __shfl_xor(best, o, 64);
            if (oc > bestCount || (oc == bestCount && oc > 0 && ob < best)) { bestCount = oc; best = ob; }
        }
        if (i >= n || r != 0) continue;
        if (tm[i].y <= DEAD_TIME) { labels[i] = -1; continue; }
        labels[i] = best;
        float2 c = col[i];
        if (c.y == 0 || c.y == defaultColor) {
            c.y = (best != -1) ? inst_color[best] : defaultColor;
            col[i] = c;
        }
    }
}

// computeMaxCountInMapKernel, IF/Core/InstanceFusionCuda.cu:1012-1036 (per-wave pre-reduction instead
// of 192 global atomics per surfel)
__global__ __launch_bounds__(256) void k_max_count(const DevState* __restrict__ st, const float4* __restrict__ votes, int cap, const float2* __restrict__ tm,
                                                   int* __restrict__ maxv, int* __restrict__ sumv)
{
    (void)cap;
    __shared__ int smax[NI], ssum[NI];
    for (int t = threadIdx.x; t < NI; t += blockDim.x) { smax[t] = 0; ssum[t] = 0; }
    __syncthreads();
    const size_t n4 = (size_t)st->count * 12;   // one thread per float4 of the records: consecutive threads, consecutive bytes
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < n4; g += (size_t)blockDim.x * gridDim.x) {
        const int i = (int)(g / 12), q = (int)(g - (size_t)i * 12);
        if (tm[i].y <= DEAD_TIME) continue;
        const float4 v = votes[g];
        const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int t = 0; t < 4; t++) {
            int a, b;
            const int k = (q * 4 + t) * 2;
            vote_decode(f[t], a, b);
            if (a > 0) atomicMax(&smax[k], a);
            if (b > 0) atomicMax(&smax[k + 1], b);
            if (a) atomicAdd(&ssum[k], a);
            if (b) atomicAdd(&ssum[k + 1], b);
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < NI; t += blockDim.x) {
        if (smax[t]) atomicMax(&maxv[t], smax[t]);
        if (ssum[t]) atomicAdd(&sumv[t], ssum[t]);
    }
}

// cleanInstanceTableMapKernel, IF/Core/InstanceFusionCuda.cu:1057-1084
__global__ void k_clean_table(const DevState* __restrict__ st, float* __restrict__ votes, int cap, const int* __restrict__ clean_list)
{
    (void)cap;
    const size_t nf = (size_t)st->count * IFX_VF;   // one thread per float of the records
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < nf; g += (size_t)blockDim.x * gridDim.x) {
        const int fi = (int)(g % IFX_VF);
        const int c1 = clean_list[2 * fi], c2 = clean_list[2 * fi + 1];
        if (!c1 && !c2) continue;
        int a, b;
        vote_decode(votes[g], a, b);
        if (c1) a = 0;
        if (c2) b = 0;
        votes[g] = vote_encode(a, b);
    }
}

// ------------------------------------------------------------------ host side
int ifx_alloc_instance(ifx* h)
{
    uint32_t s = 0x1F5u;
    for (int i = 0; i < NI; i++) {
        h->inst_class[i] = -1;
        // createInstanceTable (IF/Core/InstanceTable.cpp:11-35) draws colours from unseeded rand();
        // a fixed LCG is used instead -- the colours are arbitrary in the reference too.
        int c[3];
        for (int k = 0; k < 3; k++) { s = s * 1664525u + 1013904223u; c[k] = (int)((s >> 8) % 255u); }
        h->inst_color[i] = (float)((c[0] << 16) + (c[1] << 8) + c[2]);
    }
    HIPCHK(h, hipMalloc(&h->d_inst_color, NI * 4));
    HIPCHK(h, hipMemcpy(h->d_inst_color, h->inst_color, NI * 4, hipMemcpyHostToDevice));
    HIPCHK(h, hipMalloc(&h->d_pdm, (size_t)h->P * 2));
    HIPCHK(h, hipMalloc(&h->d_bbox, (NI + 256) * 16));
    HIPCHK(h, hipMalloc(&h->d_inst_stats, NI * 2 * 4));
    HIPCHK(h, hipMalloc(&h->d_clean_list, NI * 4));
    return IFX_OK;
}
void ifx_free_snapshots(ifx* h);
void ifx_free_instance(ifx* h)
{
    hipFree(h->d_inst_color); hipFree(h->d_masks); hipFree(h->d_masks_ori); hipFree(h->d_unavail); hipFree(h->d_ff_label); hipFree(h->d_pdm); hipFree(h->d_bbox); hipFree(h->d_inst_stats); hipFree(h->d_clean_list);
    hipFree(h->d_segctl); hipFree(h->d_mask_rank); hipFree(h->oseg_rec); hipFree(h->d_cmp_tab); hipFree(h->d_pres); hipFree(h->d_merge_plan);
    ifx_free_snapshots(h);
    ifx_detector_free(h);
    if (h->h_segctl) hipHostFree(h->h_segctl);
    if (h->h_masks_stage) hipHostFree(h->h_masks_stage);
}

int ifx_ensure_masks(ifx* h, size_t bytes)
{
    if (bytes <= h->masks_cap) return IFX_OK;
    if (h->d_masks) hipFree(h->d_masks);
    if (h->d_masks_ori) hipFree(h->d_masks_ori);
    h->d_masks = nullptr; h->d_masks_ori = nullptr; h->masks_cap = 0;
    HIPCHK(h, hipMalloc(&h->d_masks, bytes));
    HIPCHK(h, hipMalloc(&h->d_masks_ori, bytes));
    if (!h->d_unavail) HIPCHK(h, hipMalloc(&h->d_unavail, 512));
    h->masks_cap = bytes;
    return IFX_OK;
}

extern "C" int ifx_mask_clean_overlap(ifx_t* h, uint8_t* masks, int n)
{
    if (!h || !masks || n < 0) return IFX_E_INVALID;
    if (n == 0) return IFX_OK;
    size_t bytes = (size_t)n * h->P;
    int r = ifx_ensure_masks(h, bytes);
    if (r) return r;
    HIPCHK(h, hipMemcpyAsync(h->d_masks, masks, bytes, hipMemcpyHostToDevice, h->cur));
    LAUNCH(h, "mask_clean_overlap", dim3(cdiv(h->P, 256)), dim3(256), k_mask_clean_overlap, h->d_masks, n, h->P);
    HIPCHK(h, hipMemcpyAsync(masks, h->d_masks, bytes, hipMemcpyDeviceToHost, h->cur));
    HIPCHK(h, hipStreamSynchronize(h->cur));
    return IFX_OK;
}

// whetherDoSegmentation, IF/Core/InstanceFusion.cpp:192-238
static int mask_geometric_filter_device(ifx* h, const uint16_t* d_depth, uint8_t* d_masks, const uint8_t* d_ori, int nm, uint8_t* d_unavail, int fixed_rounds = 0, bool resume = false,
                                        bool verdict_by_caller = false);
// maskGeometricFilter as a stage (host buffers): depth = model depth under the camera (u16, 1186 units per metre as
// getProjectDepthMap produces it), masks in/out, ori = masks before clean-overlap, unavailable in/out
extern "C" int ifx_mask_geometric_filter(ifx_t* h, const uint16_t* depth, uint8_t* masks, const uint8_t* ori, int n, uint8_t* unavailable)
{
    if (!h || !depth || n < 0 || n > 256 || (n > 0 && (!masks || !ori || !unavailable))) return IFX_E_INVALID;
    if (n == 0) return IFX_OK;
    const size_t P = h->P, bytes = (size_t)n * P;
    int r = ifx_ensure_masks(h, bytes);
    if (r) return r;
    HIPCHK(h, hipMemcpyAsync(h->d_pdm, depth, P * 2, hipMemcpyHostToDevice, h->cur));
    HIPCHK(h, hipMemcpyAsync(h->d_masks, masks, bytes, hipMemcpyHostToDevice, h->cur));
    HIPCHK(h, hipMemcpyAsync(h->d_masks_ori, ori, bytes, hipMemcpyHostToDevice, h->cur));
    HIPCHK(h, hipMemcpyAsync(h->d_unavail, unavailable, n, hipMemcpyHostToDevice, h->cur));
    if ((r = mask_geometric_filter_device(h, h->d_pdm, h->d_masks, h->d_masks_ori, n, h->d_unavail))) return r;
    HIPCHK(h, hipMemcpyAsync(masks, h->d_masks, bytes, hipMemcpyDeviceToHost, h->cur));
    HIPCHK(h, hipMemcpyAsync(unavailable, h->d_unavail, n, hipMemcpyDeviceToHost, h->cur));
    HIPCHK(h, hipStreamSynchronize(h->cur));
    return IFX_OK;
}

extern "C" int ifx_should_segment(ifx_t* h, int frame)
{
    if (!h) return IFX_E_INVALID;
    const int downsample = 10, fixedL = 2, fixedH = 45;
    int count[2];
    if (h->seg_counts_valid) {
        // the frame that just ran accumulated the two sums while it rendered ids_after (k_raster_finish) and left them in the
        // pinned frame result: nothing to launch, only the frame to wait for (not the stream: the next frame's tracker may
        // already be queued behind it)
        HIPCHK(h, hipEventSynchronize(h->ev_result));
        // (the one place an asynchronous host looks at every frame's result: the sticky failures are reported here too, not only by ifx_sync)
        if (h->h_result->overflow) { h->err = "surfel store capacity exceeded"; return IFX_E_CAPACITY; }
        count[0] = h->h_result->seg_counts[0]; count[1] = h->h_result->seg_counts[1];
    } else {
        int* cnt = h->d_inst_stats;
        HIPCHK(h, hipMemsetAsync(cnt, 0, 8, h->cur));
        int gw = cdiv(h->w, downsample), gh = cdiv(h->h, downsample);
        LAUNCH(h, "check_project", dim3(cdiv(gw, 16), cdiv(gh, 16)), dim3(16, 16), k_check_project, h->d_state, h->ids_after, (const float4*)h->votes, h->cap, h->w, h->h, downsample, cnt);
        HIPCHK(h, hipMemcpyAsync(count, cnt, 8, hipMemcpyDeviceToHost, h->cur));
        HIPCHK(h, hipStreamSynchronize(h->cur));
    }
    int w = h->w, hh = h->h;
    bool test1 = count[0] > (w / downsample * hh / downsample * 0.48 * 30);
    bool test2 = count[1] < (w / downsample * hh / downsample * 0.2);
    const int gap = (test1 || test2) ? fixedH : fixedL;
    if (frame - h->last_seg_frame > gap) { h->last_seg_frame = frame; return 1; }
    // Not this frame -- but if the cadence says "the next one", that frame draws the WHOLE id image while it rasterises its prediction (one pass over the same lists:
    // ~20 us) instead of leaving the rest of the image to the call (a walk of its own over the view lists + a resolve at the head of the call: ~80 us).  A hint only:
    // the decision is taken again on the next frame's own sums, and a call that finds the sparse image renders the rest as before (ifx_ids_ensure).
    const bool next = frame + 1 - h->last_seg_frame > gap;
    if (next) h->ids_full_hint = 1;
    if (next || h->opt_slic_ahead == 2) {   // ... and its superpixels (frame-only work, half of a call) start now on the side stream, if the frame is announced
        int r = ifx_superpixel_ahead(h);    // (option value 2, for tests: for every announced frame, whatever the cadence says)
        if (r) return r;
    }
    return 0;
}

// getDepthThreshold, IF/Core/InstanceFusion.h:170-176
__device__ __forceinline__ float depth_threshold_dev(int depth)
{
    float t = 0.074f * depth - 246.0f;
    t = fmaxf(50.0f, t);
    t = fminf(420.0f, t);
    return t;
}

// filterAreaCompute + maskGeometricFilter, IF/Core/InstanceFusion.cpp:470-593, on the device.
// The reference floods each mask on the CPU: pixels (interior, mask set, model depth valid) are visited in row-major
// order, an unvisited one seeds a breadth-first fill along edges  now -> neighbour  that exist when
// |depth[now] - depth[neighbour]| < threshold(depth[now])  (the threshold of the SOURCE pixel, so an edge can be
// one-way beyond 4 m), and the seed's sequence number is the region id.  A filled region is closed under forward
// reachability, hence a pixel ends up in the region of the EARLIEST pixel (row-major) that reaches it:
//     label(p) = min { q : q ~> p }.
// That fixpoint is reached by monotone min-propagation along the directed edges in any order: 32x32 tiles relax
// in LDS until nothing changes, one pointer jump (label <- label[label], valid by transitivity) per launch carries
// labels across tiles, and launches repeat until a launch changes nothing.
#define FF_T 32
#define FF_SLOTS 64
struct FFArgs {
    const uint16_t* depth; uint8_t* masks; const uint8_t* ori; const uint8_t* skip;   // skip[m] != 0: mask left alone
    int* label; int* cnt; int* meta;   // meta[m*32 + 0] oriPoints, [1] kept count, [2] finalPoints, [4..24) kept region ids
    int* changed;                      // [it] set when relaxation launch `it` lowered a label (host-driven rounds use slot 0 only)
    const int* gate;                   // fixed schedule: the tail kernels run only when *gate == 0 (the last scheduled relaxation changed nothing: fixpoint); nullptr: always
    uint8_t* tile_active;              // [nm][tiles]: the tile holds a labelled pixel (a tile without one has nothing to relax, whatever its halo says: labels only ever move between mask pixels)
    int nm, w, h;
};

__global__ void k_ff_prep(FFArgs a, const uint8_t* __restrict__ unavail, uint8_t* __restrict__ skip, int n_tiles)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_tiles) a.tile_active[t] = 0;
    if (t < a.nm * 32) a.meta[t] = 0;
    if (t < FF_SLOTS) a.changed[t] = 0;
    if (t < a.nm) skip[t] = unavail[t];
}
__global__ void k_ff_init(FFArgs a)
{
    const int P = a.w * a.h, k = blockIdx.x * blockDim.x + threadIdx.x, m = blockIdx.y;
    bool in = k < P && !a.skip[m];
    int x = in ? k % a.w : 0, y = in ? k / a.w : 0;
    bool interior = in && x >= 1 && x < a.w - 1 && y >= 1 && y < a.h - 1;
    bool o = interior && a.ori[(size_t)m * P + k];
    if (k < P) {
        bool v = interior && a.masks[(size_t)m * P + k] && a.depth[k];
        a.label[(size_t)m * P + k] = v ? k : -1;
        a.cnt[(size_t)m * P + k] = 0;
        if (v) a.tile_active[(size_t)m * ((a.w + FF_T - 1) / FF_T) * ((a.h + FF_T - 1) / FF_T) + (y / FF_T) * ((a.w + FF_T - 1) / FF_T) + x / FF_T] = 1;   // (same value from every writer)
    }
    unsigned long long b = __ballot(o);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&a.meta[m * 32], __popcll(b));
}

// `it`: index of this launch in a fixed schedule.  A launch whose predecessor changed nothing has nothing to do either (that predecessor re-checked every edge:
// the fixpoint) and returns at its first instruction, leaving its own flag clear -- so the host can enqueue the whole schedule without looking.
//
// Inside a tile the relaxation runs as SWEEPS (round 3): a thread owns a row (then a column) of the 34 x 34 window and carries the minimum along it in one
// sequential pass -- left to right, right to left, top to bottom, bottom to top, halo cells as sources -- so a label crosses the whole tile in one pass instead of
// one pixel per barrier-separated iteration (the first version: up to 128 iterations of a 256-thread block, 140 us for the first launch of a call; now a handful of
// rounds of four passes on one wave).  Same fixpoint: min-propagation along the same directed edges (the threshold is the SOURCE pixel's), in another order.
__device__ __forceinline__ bool ff_pull(int& l, int dp_unused, int ql, int dq, int dp)
{
    (void)dp_unused;
    if (ql < 0 || ql >= l) return false;
    if ((float)abs(dq - dp) < depth_threshold_dev(dq)) { l = ql; return true; }   // edge q -> p, threshold of the source q
    return false;
}
__global__ void __launch_bounds__(256) k_ff_relax(FFArgs a, int it)
{
    __shared__ int s_lab[FF_T + 2][FF_T + 3];          // (+1 column: rows and columns land on different banks)
    __shared__ unsigned short s_d[FF_T + 2][FF_T + 4];
    if (it > 0 && a.changed[it - 1] == 0) return;
    const int P = a.w * a.h, m = blockIdx.z;
    if (a.skip[m] || !a.tile_active[((size_t)m * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x]) return;   // (most (mask, tile) pairs: the masks cover a fraction of the image)
    int* lab = a.label + (size_t)m * P;
    const int x0 = blockIdx.x * FF_T - 1, y0 = blockIdx.y * FF_T - 1, tid = threadIdx.x;
    {   // the window: all loads of a thread in one batch, then the pointer jumps of the tile's own pixels in a second one (two round trips, not ten)
        constexpr int NL = ((FF_T + 2) * (FF_T + 2) + 255) / 256;
        int l[NL], d[NL];
#pragma unroll
        for (int q = 0; q < NL; q++) {
            const int t = tid + q * 256, ly = t / (FF_T + 2), lx = t - ly * (FF_T + 2), x = x0 + lx, y = y0 + ly;
            const bool in = t < (FF_T + 2) * (FF_T + 2) && x >= 0 && x < a.w && y >= 0 && y < a.h;
            l[q] = in ? lab[y * a.w + x] : -1;
            d[q] = in ? a.depth[y * a.w + x] : 0;
        }
#pragma unroll
        for (int q = 0; q < NL; q++) {
            const int t = tid + q * 256, ly = t / (FF_T + 2), lx = t - ly * (FF_T + 2);
            const bool interior = lx >= 1 && lx <= FF_T && ly >= 1 && ly <= FF_T;
            const int g = (interior && l[q] >= 0) ? lab[l[q]] : -1;   // one pointer jump: my label reaches me, so does ITS label
            if (g >= 0 && g < l[q]) l[q] = g;
        }
#pragma unroll
        for (int q = 0; q < NL; q++) {
            const int t = tid + q * 256, ly = t / (FF_T + 2), lx = t - ly * (FF_T + 2);
            if (t < (FF_T + 2) * (FF_T + 2)) { s_lab[ly][lx] = l[q]; s_d[ly][lx] = (unsigned short)d[q]; }
        }
    }
    __syncthreads();
    // A thread pulls its line into registers, sweeps it forth and back there (no LDS latency inside the dependent chain) and writes back what changed.
    const int line = (tid & 31) + 1;   // the row / column of this thread: 1 .. FF_T (one half-wave sweeps; the whole block of 256 loads and stores)
    for (int round = 0; round < 4 * FF_T; round++) {
        int any = 0;
#pragma unroll 1
        for (int dir = 0; dir < 2; dir++) {   // 0: rows, 1: columns
            if (tid < 32) {
                int l[FF_T + 2], d[FF_T + 2];
#pragma unroll
                for (int x = 0; x < FF_T + 2; x++) { l[x] = dir ? s_lab[x][line] : s_lab[line][x]; d[x] = dir ? s_d[x][line] : s_d[line][x]; }
                unsigned int ch = 0;
#pragma unroll
                for (int x = 1; x <= FF_T; x++)
                    if (l[x] >= 0 && l[x - 1] >= 0 && l[x - 1] < l[x] && (float)abs(d[x - 1] - d[x]) < depth_threshold_dev(d[x - 1])) { l[x] = l[x - 1]; ch |= 1u << (x - 1); }
#pragma unroll
                for (int x = FF_T; x >= 1; x--)
                    if (l[x] >= 0 && l[x + 1] >= 0 && l[x + 1] < l[x] && (float)abs(d[x + 1] - d[x]) < depth_threshold_dev(d[x + 1])) { l[x] = l[x + 1]; ch |= 1u << (x - 1); }
                if (ch) {
                    any = 1;
#pragma unroll
                    for (int x = 1; x <= FF_T; x++)
                        if (ch & (1u << (x - 1))) { if (dir) s_lab[x][line] = l[x]; else s_lab[line][x] = l[x]; }
                }
            }
            __syncthreads();
        }
        if (!__syncthreads_or(any)) break;
    }
    int dirty = 0;
    for (int t = tid; t < FF_T * FF_T; t += 256) {
        const int ly = t / FF_T + 1, lx = t - (ly - 1) * FF_T + 1, x = x0 + lx, y = y0 + ly;
        if (x < a.w && y < a.h) {
            const int l = s_lab[ly][lx];
            if (l >= 0 && l != lab[y * a.w + x]) { lab[y * a.w + x] = l; dirty = 1; }
        }
    }
    if (__syncthreads_or(dirty) && tid == 0) a.changed[it] = 1;
}

// Union-find start of the fill (round 3).  Pixels joined by edges that exist in BOTH directions reach each other, so they end with the same label, whatever else
// happens: their components can be merged with the lock-free union-find of connected-component labelling instead of walking labels across the image one tile
// border per launch.  k_ff_tile_uf leaves every pixel pointing at the smallest pixel of its component INSIDE its tile (a forest of depth one, roots point at
// themselves); k_ff_merge unites the trees across every tile border edge (the larger root is hung under the smaller: atomicMin, retried until it sticks);
// k_ff_flatten points every pixel at its root = the smallest pixel of the whole component.  Every label is still "a pixel that reaches me", so the directed
// relaxation that follows starts from a valid state and -- where every edge is two-way (model depth under 4 m: one threshold) -- finds nothing left to do.
// Tile-local half: union-find in LDS over the two-way edges INSIDE a 32 x 32 tile (right and lower neighbour of every pixel: each edge once), then every pixel
// points at the smallest pixel of its component within the tile (row-major order inside a tile is the global order restricted to it).  No rounds, no halo: the
// edges across tile borders are k_ff_merge's.  (First version: the relaxation kernel restricted to two-way edges, sweeps to the local fixpoint, 64 us a call; this one 32.)
__device__ __forceinline__ int ff_find_lds(const volatile int* par, int x)
{
    int p = par[x];
    while (p != x) { x = p; p = par[x]; }
    return x;
}
__global__ void __launch_bounds__(256) k_ff_tile_uf(FFArgs a)
{
    __shared__ int par[FF_T * FF_T];
    __shared__ unsigned short dep[FF_T * FF_T];
    const int P = a.w * a.h, m = blockIdx.z;
    if (a.skip[m] || !a.tile_active[((size_t)m * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x]) return;
    int* lab = a.label + (size_t)m * P;
    const int x0 = blockIdx.x * FF_T, y0 = blockIdx.y * FF_T, tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < FF_T * FF_T / 256; q++) {
        const int t = tid + q * 256, ly = t / FF_T, lx = t - ly * FF_T, x = x0 + lx, y = y0 + ly;
        const bool in = x < a.w && y < a.h;
        par[t] = (in && lab[y * a.w + x] >= 0) ? t : -1;
        dep[t] = in ? a.depth[y * a.w + x] : (unsigned short)0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < FF_T * FF_T / 256; q++) {
        const int t = tid + q * 256, ly = t / FF_T, lx = t - ly * FF_T;
        if (par[t] < 0) continue;
        const int dp = dep[t];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            if (e == 0 ? lx + 1 >= FF_T : ly + 1 >= FF_T) continue;
            const int u = e == 0 ? t + 1 : t + FF_T;
            if (par[u] < 0) continue;
            const int dq = dep[u];
            const float dd = (float)abs(dp - dq);
            if (!(dd < depth_threshold_dev(dp) && dd < depth_threshold_dev(dq))) continue;
            int ra = t, rb = u;
            for (;;) {
                ra = ff_find_lds(par, ra); rb = ff_find_lds(par, rb);
                if (ra == rb) break;
                if (ra > rb) { const int s_ = ra; ra = rb; rb = s_; }
                const int old = atomicMin(&par[rb], ra);
                if (old == rb) break;
                rb = old;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < FF_T * FF_T / 256; q++) {
        const int t = tid + q * 256, ly = t / FF_T, lx = t - ly * FF_T;
        if (par[t] < 0) continue;
        const int r = ff_find_lds(par, t), ry = r / FF_T, rx = r - ry * FF_T;
        if (r != t) lab[(y0 + ly) * a.w + x0 + lx] = (y0 + ry) * a.w + x0 + rx;
    }
}
__device__ __forceinline__ int ff_find(const int* lab, int x)
{
    int p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) { x = p; p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    return x;
}
__global__ void k_ff_merge(FFArgs a)
{
    const int m = blockIdx.y;
    if (a.skip[m]) return;
    const int nbx = (a.w - 1) / FF_T, nby = (a.h - 1) / FF_T;   // vertical / horizontal tile borders inside the image
    const int t = blockIdx.x * blockDim.x + threadIdx.x, nv = nbx * a.h, nh = nby * a.w;
    if (t >= nv + nh) return;
    int p, q;
    if (t < nv) { const int b = t / a.h, y = t - b * a.h, x = (b + 1) * FF_T; p = y * a.w + x - 1; q = p + 1; }
    else { const int u = t - nv, b = u / a.w, x = u - b * a.w, y = (b + 1) * FF_T; p = (y - 1) * a.w + x; q = p + a.w; }
    int* lab = a.label + (size_t)m * a.w * a.h;
    if (lab[p] < 0 || lab[q] < 0) return;
    const int dp = a.depth[p], dq = a.depth[q];
    const float dd = (float)abs(dp - dq);
    if (!(dd < depth_threshold_dev(dp) && dd < depth_threshold_dev(dq))) return;
    int ra = p, rb = q;
    for (;;) {
        ra = ff_find(lab, ra); rb = ff_find(lab, rb);
        if (ra == rb) break;
        if (ra > rb) { const int s_ = ra; ra = rb; rb = s_; }
        const int old = atomicMin(lab + rb, ra);
        if (old == rb) break;   // rb was a root and now hangs under ra
        rb = old;               // somebody hung it elsewhere first: unite with that tree
    }
}
__global__ void k_ff_flatten(FFArgs a)
{
    const int P = a.w * a.h, k = blockIdx.x * blockDim.x + threadIdx.x, m = blockIdx.y;
    if (k >= P || a.skip[m]) return;
    int* lab = a.label + (size_t)m * P;
    const int l = lab[k];
    if (l < 0) return;
    const int r = ff_find(lab, l);
    if (r != l) __hip_atomic_store(lab + k, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// region sizes: one counter per root pixel; lanes of a wave grouped by label (regions are large)
__global__ void k_ff_count(FFArgs a)
{
    if (a.gate && *a.gate) return;
    const int P = a.w * a.h, k = blockIdx.x * blockDim.x + threadIdx.x, m = blockIdx.y;
    int l = (k < P && !a.skip[m]) ? a.label[(size_t)m * P + k] : -1;
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(l >= 0);
    while (todo) {
        int leader = __ffsll((long long)todo) - 1;
        int ll = __shfl(l, leader);
        unsigned long long grp = __ballot(l == ll);
        todo &= ~grp;
        if (lane == leader) atomicAdd(&a.cnt[(size_t)m * P + ll], __popcll(grp));
    }
}
// regions holding more than a quarter of the original mask are kept (IF/Core/InstanceFusion.cpp:560)
__global__ void k_ff_select(FFArgs a)
{
    if (a.gate && *a.gate) return;
    const int P = a.w * a.h, k = blockIdx.x * blockDim.x + threadIdx.x, m = blockIdx.y;
    if (k >= P || a.skip[m] || a.label[(size_t)m * P + k] != k) return;
    float points = (float)a.cnt[(size_t)m * P + k], oriPoints = (float)a.meta[m * 32];
    if (points / oriPoints > 0.25f) {
        int slot = atomicAdd(&a.meta[m * 32 + 1], 1);
        if (slot < 20) a.meta[m * 32 + 4 + slot] = k;
    }
}
// The reference's list holds the FIRST twenty qualifying regions in scan order (`if(p<20) list[p++]`, :557); k_ff_select's slots are handed out in whatever
// order its atomics land.  With twenty or fewer (every mask that lies inside its `ori`: at most three regions exceed a quarter of it) the two lists hold the
// same set.  With more -- `ori` much smaller than the mask, or empty, where every ratio is inf -- the block rebuilds the list itself: the twenty smallest
// qualifying roots, found by one wave scanning the labels in order.  Never taken in a run; a few hundred redundant scans of the image when it is.
__global__ void k_ff_apply(FFArgs a)
{
    if (a.gate && *a.gate) return;
    const int P = a.w * a.h, k = blockIdx.x * blockDim.x + threadIdx.x, m = blockIdx.y;
    __shared__ int s_first[20];
    const int found = a.skip[m] ? 0 : a.meta[m * 32 + 1];   // (the same for the whole block: the branch below is uniform)
    if (found > 20) {
        if (threadIdx.x < 64) {
            const float oriPoints = (float)a.meta[m * 32];
            int n = 0;
            for (int base = 0; base < P && n < 20; base += 64) {
                const int q = base + (int)threadIdx.x;
                const bool root = q < P && a.label[(size_t)m * P + q] == q && (float)a.cnt[(size_t)m * P + q] / oriPoints > 0.25f;   // k_ff_select's test
                const unsigned long long b = __ballot(root);
                const int pos = n + __popcll(b & ((1ull << threadIdx.x) - 1ull));
                if (root && pos < 20) s_first[pos] = q;
                n += __popcll(b);
            }
        }
        __syncthreads();
    }
    bool keep = false;
    if (k < P && !a.skip[m]) {
        const int l = a.label[(size_t)m * P + k];
        if (found > 20) { for (int j = 0; j < 20; j++) keep = keep || (l >= 0 && l == s_first[j]); }
        else for (int j = 0; j < found; j++) keep = keep || (l >= 0 && l == a.meta[m * 32 + 4 + j]);
        a.masks[(size_t)m * P + k] = keep ? 255 : 0;
    }
    unsigned long long b = __ballot(keep);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&a.meta[m * 32 + 2], __popcll(b));
}
// a mask that lost more than 35 % of its pixels is unusable (:590)
__global__ void k_ff_verdict(FFArgs a, uint8_t* unavailable)
{
    if (a.gate && *a.gate) return;
    int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.nm || a.skip[m]) return;
    float finalPoints = (float)a.meta[m * 32 + 2], oriPoints = (float)a.meta[m * 32];
    if (finalPoints / oriPoints < 0.65f) unavailable[m] = 1;
}

// d_unavail: [nm] bytes in/out (set entries are skipped, as `continue` at :520); masks / ori: device, [nm][P]
// fixed_rounds == 0: relaxations until a launch changes nothing, the host looking every 7 launches (stage API, sharded calls, slow path).
// fixed_rounds  > 0: exactly that many relaxation launches are enqueued -- the ones behind the fixpoint return at once -- and the tail (region sizes, selection,
//   verdict) only runs when the last one found nothing to change; otherwise *ff_gate() stays set and the caller finishes with resume = true.  No host look at all.
static FFArgs ff_args(ifx* h, const uint16_t* d_depth, uint8_t* d_masks, const uint8_t* d_ori, int nm)
{
    FFArgs a;
    a.depth = d_depth; a.masks = d_masks; a.ori = d_ori; a.nm = nm; a.w = h->w; a.h = h->h;
    a.label = h->d_ff_label; a.cnt = h->d_ff_label + h->ff_cap; a.meta = a.cnt + h->ff_cap; a.changed = a.meta + 256 * 32;
    uint8_t* d_skip = (uint8_t*)(a.changed + FF_SLOTS);
    a.skip = d_skip;
    a.tile_active = d_skip + 256;
    a.gate = nullptr;
    return a;
}
// verdict_by_caller: the last step (a mask that lost more than 35 % is unusable) is left to the kernel the caller launches next (k_seg_register: one dispatch less on the call's chain)
static int mask_geometric_filter_device(ifx* h, const uint16_t* d_depth, uint8_t* d_masks, const uint8_t* d_ori, int nm, uint8_t* d_unavail, int fixed_rounds, bool resume, bool verdict_by_caller)
{
    const int P = h->P;
    size_t need = (size_t)nm * P;
    if (need > h->ff_cap) {
        if (h->d_ff_label) hipFree(h->d_ff_label);
        h->d_ff_label = nullptr; h->ff_cap = 0;
        HIPCHK(h, hipMalloc(&h->d_ff_label, need * 2 * 4 + (size_t)256 * 32 * 4 + FF_SLOTS * 4 + 256 + (size_t)256 * cdiv(h->w, FF_T) * cdiv(h->h, FF_T)));
        h->ff_cap = need;
    }
    FFArgs a = ff_args(h, d_depth, d_masks, d_ori, nm);
    uint8_t* d_skip = (uint8_t*)a.skip;
    dim3 per_px(cdiv(P, 256), nm);
    dim3 tiles(cdiv(h->w, FF_T), cdiv(h->h, FF_T), nm);
    if (!resume) {
        // one launch re-arms the fill's bookkeeping (tile flags, per-mask counters, the schedule's "changed" words) and freezes who is skipped (the verdict must not
        // change that mid-way): three fills and a copy, four dispatches of a latency-bound chain, before
        LAUNCH(h, "ff_prep", dim3(cdiv(std::max(nm * cdiv(h->w, FF_T) * cdiv(h->h, FF_T), nm * 32), 256)), dim3(256), k_ff_prep, a, (const uint8_t*)d_unavail, d_skip,
               nm * cdiv(h->w, FF_T) * cdiv(h->h, FF_T));
        LAUNCH(h, "ff_init", per_px, dim3(256), k_ff_init, a);
        // the two-way edges by union-find: three launches for what took the relaxation a launch per tile border crossed
        const int pairs = ((h->w - 1) / FF_T) * h->h + ((h->h - 1) / FF_T) * h->w;
        LAUNCH(h, "ff_local", tiles, dim3(256), k_ff_tile_uf, a);
        if (pairs > 0) LAUNCH(h, "ff_merge", dim3(cdiv(pairs, 256), nm), dim3(256), k_ff_merge, a);
        LAUNCH(h, "ff_flatten", per_px, dim3(256), k_ff_flatten, a);
    }
    if (fixed_rounds > 0 && !resume) {
        if (fixed_rounds > FF_SLOTS) fixed_rounds = FF_SLOTS;
        for (int it = 0; it < fixed_rounds; it++) LAUNCH(h, "ff_relax", tiles, dim3(256), k_ff_relax, a, it);
        a.gate = a.changed + (fixed_rounds - 1);
    } else {
        for (int round = 0; round < 64; round++) {
            HIPCHK(h, hipMemsetAsync(a.changed, 0, 4, h->cur));
            for (int it = 0; it < 6; it++) LAUNCH(h, "ff_relax", tiles, dim3(256), k_ff_relax, a, 0);
            // the last launch of the batch decides: it re-checks every edge, so "no change" there is the fixpoint
            HIPCHK(h, hipMemsetAsync(a.changed, 0, 4, h->cur));
            LAUNCH(h, "ff_relax", tiles, dim3(256), k_ff_relax, a, 0);
            int changed = 0;
            HIPCHK(h, hipMemcpyAsync(&changed, a.changed, 4, hipMemcpyDeviceToHost, h->cur));
            HIPCHK(h, hipStreamSynchronize(h->cur));
            if (!changed) break;
        }
    }
    LAUNCH(h, "ff_count", per_px, dim3(256), k_ff_count, a);
    LAUNCH(h, "ff_select", per_px, dim3(256), k_ff_select, a);
    LAUNCH(h, "ff_apply", per_px, dim3(256), k_ff_apply, a);
    if (!verdict_by_caller) LAUNCH(h, "ff_verdict", dim3(cdiv(nm, 64)), dim3(64), k_ff_verdict, a, d_unavail);
    return IFX_OK;
}

// ------------------------------------------------------------------ the mask rule of the compare map (option compare_map 2; the reference's "PLAN B",
// compareMapType 2: maskCompareMapKernel, IF/Core/InstanceFusionCuda.cu:826-881, and the decision loop, IF/Core/InstanceFusion.cpp:805-870)
// I[m][i] = #{p : Md(m, p) and Id(i, p)}, A_M[m] = #{p : Md(m, p)}, A_I[i] = #{p : Id(i, p)} over all pixels, Md / Id the 3 x 3 dilations (inside the image) of
// mask m and of instance i's presence (k_project_bbox<3>); U = A_M + A_I - I is never counted.  The tables hold EVERY pair: the class test of the rule is made
// where they are read (k_seg_compare_iou, compare_map_iou, ifx_mask_compare_map's outputs).
// One workgroup per tile of 32 x 8 pixels.  Presence words and mask bits of the tile and its one-pixel halo go through LDS; a wave's ballot of "instance i is
// here" is taken once per instance the wave sees at all and kept in LDS, so that a mask's row of I is popcount(mask ballot & instance ballot) with the lanes over
// the instances; wave -> LDS accumulators of the workgroup -> one global integer add per cell it touched.  Integer adds only: exact in any order.
#define CM_TW 32
#define CM_TH 8
#define CM_HW (CM_TW + 2)
#define CM_HC (CM_HW * (CM_TH + 2))
#define CM_AI 0                         // table layout (ints): A_I[NI], A_M[256], I[256][NI]; behind them the box sink of the presence pass outside the device body
#define CM_AM NI
#define CM_I (NI + 256)
#define CM_INTS (NI + 256 + 256 * NI)
__global__ void __launch_bounds__(CM_TW * CM_TH) k_cmp_count(const uint4* __restrict__ pres, const uint8_t* __restrict__ masks, int nm, int w, int h, int* __restrict__ tab)
{
    __shared__ unsigned int s_p[3][CM_HC];
    __shared__ unsigned char s_mk[CM_HC];
    __shared__ unsigned long long s_bal[CM_TW * CM_TH / 64][NI];
    __shared__ int s_ai[NI], s_am[8], s_i[8 * NI];
    const int tid = threadIdx.y * CM_TW + threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int x0 = blockIdx.x * CM_TW - 1, y0 = blockIdx.y * CM_TH - 1, P = w * h;
    for (int c = tid; c < CM_HC; c += CM_TW * CM_TH) {
        const int cx = x0 + c % CM_HW, cy = y0 + c / CM_HW;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (cx >= 0 && cx < w && cy >= 0 && cy < h) v = pres[cy * w + cx];   // (neighbours outside the image are skipped: no bits)
        s_p[0][c] = v.x; s_p[1][c] = v.y; s_p[2][c] = v.z;
    }
    for (int t = tid; t < 8 * NI; t += CM_TW * CM_TH) s_i[t] = 0;
    if (tid < NI) s_ai[tid] = 0;
    if (tid < 8) s_am[tid] = 0;
    __syncthreads();
    const int x = blockIdx.x * CM_TW + threadIdx.x, y = blockIdx.y * CM_TH + threadIdx.y;
    const bool inside = x < w && y < h;
    const int c0 = threadIdx.y * CM_HW + threadIdx.x;   // the halo cell above and left of this pixel
    unsigned int idw[3] = {0u, 0u, 0u}, ow[3];
    if (inside) {
#pragma unroll
        for (int d = 0; d < 9; d++) { const int c = c0 + (d / 3) * CM_HW + d % 3; idw[0] |= s_p[0][c]; idw[1] |= s_p[1][c]; idw[2] |= s_p[2][c]; }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {   // the instances this wave sees at all (uniform), a ballot of each
        ow[k] = idw[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ow[k] |= __shfl_xor(ow[k], o, 64);
        unsigned int bits = ow[k];
        while (bits) {
            const int b = __ffs(bits) - 1;
            bits &= bits - 1;
            const unsigned long long bal = __ballot((idw[k] >> b) & 1u);
            if (lane == 0) { s_bal[wv][k * 32 + b] = bal; atomicAdd(&s_ai[k * 32 + b], __popcll(bal)); }
        }
    }
    for (int m0 = 0; m0 < nm; m0 += 8) {   // (uniform) the masks in chunks of eight, as k_project_bbox takes them: a bit each
        for (int c = tid; c < CM_HC; c += CM_TW * CM_TH) {
            const int cx = x0 + c % CM_HW, cy = y0 + c / CM_HW;
            unsigned int bits = 0;
            if (cx >= 0 && cx < w && cy >= 0 && cy < h) {
                const int k = cy * w + cx;
                uint8_t mb[8];
#pragma unroll
                for (int u = 0; u < 8; u++) mb[u] = m0 + u < nm ? masks[(size_t)(m0 + u) * P + k] : (uint8_t)0;
#pragma unroll
                for (int u = 0; u < 8; u++) bits |= (mb[u] > 0 ? 1u : 0u) << u;
            }
            s_mk[c] = (unsigned char)bits;
        }
        __syncthreads();   // (also: s_bal of this wave's lane 0 before its other lanes read it)
        unsigned int md = 0;
        if (inside) {
#pragma unroll
            for (int d = 0; d < 9; d++) md |= s_mk[c0 + (d / 3) * CM_HW + d % 3];
        }
        unsigned int om = md;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) om |= __shfl_xor(om, o, 64);
        while (om) {   // (uniform) the masks this wave sees; cells no lane touches cost nothing
            const int u = __ffs(om) - 1;
            om &= om - 1;
            const unsigned long long balm = __ballot((md >> u) & 1u);
            if (lane == 0) atomicAdd(&s_am[u], __popcll(balm));
            for (int i = lane; i < NI; i += 64) {
                if (!((ow[i >> 5] >> (i & 31)) & 1u)) continue;
                const int cnt = __popcll(balm & s_bal[wv][i]);
                if (cnt) atomicAdd(&s_i[u * NI + i], cnt);
            }
        }
        __syncthreads();
        for (int t = tid; t < 8 * NI; t += CM_TW * CM_TH) {
            const int v = s_i[t];
            if (v) { atomicAdd(&tab[CM_I + m0 * NI + t], v); s_i[t] = 0; }   // (a chunk's partial row u >= nm - m0 never counts: its bits are 0)
        }
        if (tid < 8 && s_am[tid]) { atomicAdd(&tab[CM_AM + m0 + tid], s_am[tid]); s_am[tid] = 0; }
        __syncthreads();
    }
    __syncthreads();
    if (tid < NI && s_ai[tid]) atomicAdd(&tab[CM_AI + tid], s_ai[tid]);
}

// the tables and the presence image: allocated by the first call that runs under the mask rule (hipMalloc may synchronise the device: that one call of a handle
// is not free of synchronisation in its middle, every later one is)
static int cmp_ensure(ifx* h)
{
    if (!h->d_cmp_tab) HIPCHK(h, hipMalloc(&h->d_cmp_tab, (size_t)(CM_INTS + NI * 4) * 4));
    if (!h->d_pres) HIPCHK(h, hipMalloc(&h->d_pres, (size_t)h->P * 16));
    return IFX_OK;
}
static int cmp_launch_count(ifx* h, int nm)
{
    HIPCHK(h, hipMemsetAsync(h->d_cmp_tab, 0, (size_t)(CM_I + nm * NI) * 4, h->cur));
    LAUNCH(h, "cmp_count", dim3(cdiv(h->w, CM_TW), cdiv(h->h, CM_TH)), dim3(CM_TW, CM_TH), k_cmp_count, (const uint4*)h->d_pres, (const uint8_t*)h->d_masks, nm, h->w, h->h, h->d_cmp_tab);
    return IFX_OK;
}
// the tables of the masks in d_masks under the id image `ids`, read back (the host-driven schedule, the eviction tail, the stage entry): the presence pass sends
// its instance boxes to a sink behind the tables, so that d_bbox stays what the box launches made it
static int cmp_tables_host(ifx* h, const int32_t* ids, int nm, std::vector<int>& tab)
{
    int r = cmp_ensure(h);
    if (r) return r;
    int* sink = h->d_cmp_tab + CM_INTS;
    LAUNCH(h, "init_bbox", dim3(cdiv(NI * 4, 256)), dim3(256), k_init_bbox, sink, NI, h->w, h->h);
    LAUNCH(h, "project_bbox_pres", dim3(cdiv(h->w, 32), cdiv(h->h, PB_ROWS)), dim3(32, PB_ROWS), k_project_bbox<3>, h->d_state, ids, (const float4*)h->votes, h->cap, (const uint8_t*)nullptr, nm,
           h->w, h->h, sink, ifx_idmap(h), (const float4*)nullptr, (uint16_t*)nullptr, (const float*)nullptr, (uint4*)h->d_pres);
    if ((r = cmp_launch_count(h, nm))) return r;
    tab.resize((size_t)CM_I + (size_t)nm * NI);
    HIPCHK(h, hipMemcpyAsync(tab.data(), h->d_cmp_tab, tab.size() * 4, hipMemcpyDeviceToHost, h->cur));
    HIPCHK(h, hipStreamSynchronize(h->cur));
    return IFX_OK;
}
// the decision over the tables (IF/Core/InstanceFusion.cpp:834-861) behind plan A's degenerate-box test: ascending instances of the mask's class, one f32 division,
// a candidate iff iou > 0.5, the best replaced iff iou > the best so far (equal maxima keep the lowest index; 0 / 0 matches nothing), and "if (best > 0)" at the end
static void compare_map_iou(ifx* h, const int* tab, const int* maskBBox, const int32_t* class_ids, int nm, std::vector<uint8_t>& unavailable, std::vector<int>& cmp)
{
    for (int m = 0; m < nm; m++) {
        const int minX_m = maskBBox[m * 4], maxX_m = maskBBox[m * 4 + 1], minY_m = maskBBox[m * 4 + 2], maxY_m = maskBBox[m * 4 + 3];
        if (maxX_m <= minX_m || maxY_m <= minY_m || unavailable[m]) { unavailable[m] = 1; continue; }
        int best = -1;
        float best_iou = 0;
        for (int q = 0; q < NI; q++) {
            if (h->inst_class[q] == -1 || class_ids[m] != h->inst_class[q]) continue;
            const int I = tab[CM_I + m * NI + q], U = tab[CM_AM + m] + tab[CM_AI + q] - I;
            const float iou = (float)I / (float)U;
            if (iou > 0.5f && iou > best_iou) { best = q; best_iou = iou; }
        }
        if (best > 0) cmp[best + m * NI] = 1;
    }
}

// computeCompareMap, IF/Core/InstanceFusion.cpp:595-651
static void compare_map(ifx* h, const int* maskBBox, const int* projBBox, const int32_t* class_ids, int nm, std::vector<uint8_t>& unavailable, std::vector<int>& cmp)
{
    for (int m = 0; m < nm; m++) {
        int minX_m = maskBBox[m * 4], maxX_m = maskBBox[m * 4 + 1], minY_m = maskBBox[m * 4 + 2], maxY_m = maskBBox[m * 4 + 3];
        if (maxX_m <= minX_m || maxY_m <= minY_m || unavailable[m]) { unavailable[m] = 1; continue; }
        int best = -1;
        for (int q = 0; q < NI; q++) {
            if (h->inst_class[q] == -1 || class_ids[m] != h->inst_class[q]) continue;
            int minX_i = projBBox[q * 4], maxX_i = projBBox[q * 4 + 1], minY_i = projBBox[q * 4 + 2], maxY_i = projBBox[q * 4 + 3];
            if (maxX_i <= minX_i || maxY_i <= minY_i) continue;
            float IW = (float)(std::min(maxX_i, maxX_m) - std::max(minX_i, minX_m));
            float IH = (float)(std::min(maxY_i, maxY_m) - std::max(minY_i, minY_m));
            if (IW <= 0 || IH <= 0) continue;
            float I = IW * IH;
            float U = (float)(((maxX_i - minX_i) * (maxY_i - minY_i)) + ((maxX_m - minX_m) * (maxY_m - minY_m))) - I;
            if (I / U > 0.5f) best = q;   // last match wins (:641-645)
        }
        if (best > 0) cmp[best + m * NI] = 1;   // instance 0 can never match (:649)
    }
}

static int first_not_used(ifx* h)
{
    for (int i = 0; i < NI; i++) if (h->inst_class[i] == -1) return i;
    return -1;
}

// (SegView: ifx_ctx.h)
static SegView seg_view_current(const ifx* h) { return SegView{h->ids_after, h->d_state->pose, nullptr, nullptr, ifx_idmap(h)}; }

// the boxes of the projected instances and of the nm masks under the view's id image (the host-driven loop and the owners' call read them back differently)
static void launch_bboxes(ifx* h, const SegView& v, int nm)
{
    LAUNCH(h, "init_bbox", dim3(cdiv((NI + nm) * 4, 256)), dim3(256), k_init_bbox, h->d_bbox, NI + nm, h->w, h->h);
    LAUNCH(h, "project_bbox", dim3(cdiv(h->w, 32), cdiv(h->h, PB_ROWS)), dim3(32, PB_ROWS), k_project_bbox<0>, h->d_state, v.ids, (const float4*)h->votes, h->cap, h->d_masks, nm, h->w, h->h,
           h->d_bbox, v.im);
}
static int run_bboxes(ifx* h, const SegView& v, int nm, std::vector<int>& bbox)
{
    launch_bboxes(h, v, nm);
    bbox.resize((size_t)(NI + nm) * 4);
    HIPCHK(h, hipMemcpyAsync(bbox.data(), h->d_bbox, bbox.size() * 4, hipMemcpyDeviceToHost, h->cur));
    HIPCHK(h, hipStreamSynchronize(h->cur));
    return IFX_OK;
}

// The eviction of a full instance table, behind k_max_count's statistics in d_inst_stats (max row, sum row): getInstanceTableCleanList
// (IF/Core/InstanceTable.cpp:185-224) -- the reference's selection sort on the sums as floats, all three arrays swapped, the first twenty of the result (ties fall
// as they fall there) -- then the table entries cleared and cleanInstanceTableMap on the votes.  Returns with the stream drained.
static int seg_evict_weakest(ifx* h)
{
    int stats[NI * 2];
    HIPCHK(h, hipMemcpyAsync(stats, h->d_inst_stats, sizeof(stats), hipMemcpyDeviceToHost, h->cur));
    HIPCHK(h, hipStreamSynchronize(h->cur));
    int* maxv = stats; int* sumv = stats + NI;
    int order[NI], cl[NI];
    for (int i = 0; i < NI; i++) order[i] = i;
    for (int i = 0; i < NI; i++)
        for (int j = i + 1; j < NI; j++)
            if ((float)sumv[j] < (float)sumv[i]) { std::swap(maxv[i], maxv[j]); std::swap(order[i], order[j]); std::swap(sumv[i], sumv[j]); }
    for (int i = 0; i < NI; i++) cl[i] = 0;
    for (int i = 0; i < 20; i++) cl[order[i]] = 1;
    for (int q = 0; q < NI; q++) if (cl[q] == 1) h->inst_class[q] = -1;
    HIPCHK(h, hipMemcpyAsync(h->d_clean_list, cl, sizeof(cl), hipMemcpyHostToDevice, h->cur));
    LAUNCH(h, "clean_table", dim3(1024), dim3(256), k_clean_table, h->d_state, h->votes, h->cap, h->d_clean_list);
    HIPCHK(h, hipStreamSynchronize(h->cur));
    return IFX_OK;
}

// ------------------------------------------------------------------ a segmentation call on a spatially sharded map
// Every rank runs the call on the same masks and the same (replicated) id image; what depends on a surfel's votes or position is computed by the
// rank that owns the surfel and merged at three kinds of exchange points (ifx_owner_exchange(h, 200, ...) names the buffers and the operation):
//   1  the projected boxes           partial min / max per instance (maxima negated: one MIN over 32-bit words)
//   2  the model depth under the camera (flood fill input)   disjoint supports: SUM
//   3  per-instance max / sum of the vote counters, when the instance table is full and its twenty weakest entries are evicted
//      (followed by another exchange of kind 1: the boxes after the eviction)
// The mask pipeline (overlap cleaning, superpixels, flood fill), the compare map and the instance table are image-space / host work and run
// replicated; vote updates and the label scan touch owned surfels only.  ifx_owner_segmentation_begin returns 1 while an exchange is pending
// (then: exchange, ifx_owner_segmentation_resume), 0 when the call is complete.  The kNN smoothing (flags & 1) needs every rank's positions and
// is not offered here.
__global__ void k_bbox_flip(int* __restrict__ bbox, int nboxes)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nboxes * 4 && (k & 1)) bbox[k] = -bbox[k];   // {minX, maxX, minY, maxY}: entries 1 and 3 are maxima
}
struct SegSnap;   // a pinned frame of ifx_segmentation_snapshot / ifx_owner_segmentation_snapshot (below): null for the ordinary entries
static int seg_view_snapshot(ifx* h, SegSnap* q, SegView* v);
extern "C" int ifx_segmentation_snapshot_release(ifx_t* h, int ticket);
// what the call in flight reads, settled once at its begin: the current id image, or (deferred call) the ticket's image in this rank's slots, pinned pose and frame
static int oseg_set_view(ifx* h, SegSnap* snap, int ticket)
{
    h->oseg_view = seg_view_current(h);
    h->oseg_ticket = snap ? ticket : -1;
    return snap ? seg_view_snapshot(h, snap, &h->oseg_view) : IFX_OK;
}
// a call that completed releases its ticket, on every rank alike (so do n == 0 and an empty shard; a call that failed keeps it)
static void oseg_release_ticket(ifx* h)
{
    if (h->oseg_ticket >= 0) ifx_segmentation_snapshot_release(h, h->oseg_ticket);
    h->oseg_ticket = -1;
}
static int oseg_launch_bboxes(ifx* h)
{
    const int nm = h->oseg_nm;
    launch_bboxes(h, h->oseg_view, nm);
    LAUNCH(h, "bbox_flip", dim3(cdiv((NI + nm) * 4, 256)), dim3(256), k_bbox_flip, h->d_bbox, NI + nm);
    h->oseg_pending = 1;
    return 1;
}
static int oseg_read_bboxes(ifx* h)
{
    const int nm = h->oseg_nm;
    LAUNCH(h, "bbox_flip", dim3(cdiv((NI + nm) * 4, 256)), dim3(256), k_bbox_flip, h->d_bbox, NI + nm);
    h->oseg_bbox.resize((size_t)(NI + nm) * 4);
    HIPCHK(h, hipMemcpyAsync(h->oseg_bbox.data(), h->d_bbox, h->oseg_bbox.size() * 4, hipMemcpyDeviceToHost, h->cur));
    HIPCHK(h, hipStreamSynchronize(h->cur));
    std::fill(h->oseg_cmp.begin(), h->oseg_cmp.end(), 0);
    compare_map(h, &h->oseg_bbox[NI * 4], &h->oseg_bbox[0], h->oseg_class.data(), nm, h->oseg_unavail, h->oseg_cmp);
    return IFX_OK;
}
// the loop over the masks (step 3) from mask oseg_m on; stops (returns 1) when the table is full and the eviction statistics must be merged
static int oseg_mask_loop(ifx* h, bool after_eviction)
{
    const int nm = h->oseg_nm, P = h->P;
    std::vector<int>& cmp = h->oseg_cmp;
    for (int m = h->oseg_m; m < nm; m++) {
        const bool resumed = after_eviction && m == h->oseg_m;   // this mask asked for room before the eviction: it goes on where the unsharded loop does (no second look at `exist`)
        bool need = resumed;
        if (!resumed) {
            bool exist = false;
            for (int q = 0; q < NI; q++) if (cmp[q + m * NI] == 1) { exist = true; break; }
            need = !exist && !h->oseg_unavail[m];
        }
        if (need) {
            int empty = first_not_used(h);
            if (empty == -1 && !resumed) {
                h->clean_times++;
                HIPCHK(h, hipMemsetAsync(h->d_inst_stats, 0, NI * 2 * 4, h->cur));
                LAUNCH(h, "max_count", dim3(1024), dim3(256), k_max_count, h->d_state, (const float4*)h->votes, h->cap, (const float2*)h->tm, h->d_inst_stats, h->d_inst_stats + NI);
                h->oseg_m = m; h->oseg_state = 3; h->oseg_pending = 3;
                return 1;
            }
            if (empty >= 0) { h->inst_class[empty] = h->oseg_class[m]; cmp[empty + m * NI] = 1; }
        }
        for (int q = 0; q < NI; q++)
            if (cmp[q + m * NI] == 1)
                LAUNCH(h, "vote_update", dim3(cdiv(P, 256)), dim3(256), k_vote_update, h->d_state, h->oseg_view.ids, h->d_masks + (size_t)m * P, P, h->cap, q, m + 1, h->votes, h->oseg_view.im);
    }
    // step 4: labels of the owned surfels
    LAUNCH(h, "count_colour", dim3(2048), dim3(256), k_count_colour, h->d_state, (const float4*)h->votes, h->cap, (const float2*)h->tm, (float2*)h->col, h->d_inst_color, h->labels, (const int*)nullptr);
    hipEvent_t eb = ifx_event_get(h);
    hipEventRecord(eb, h->cur);
    h->stage_pending.push_back({2, {h->oseg_ev, eb}});
    h->oseg_ev = nullptr;
    HIPCHK(h, hipStreamSynchronize(h->cur));
    h->oseg_state = 0; h->oseg_pending = 0;
    oseg_release_ticket(h);
    return 0;
}
// behind the masks and their refinement, the exchange points every form of the call shares
static int oseg_first_exchange(ifx* h)
{
    // option own_lazy_ids: the frame exchanged the sampled lattice only -- the exchange point in front of the boxes is the whole id image's keys (a deferred call never
    // comes by it: its ticket pinned a whole image)
    int r = h->oseg_ticket >= 0 ? 0 : ifx_owner_ids_begin_impl(h);
    if (r == 1) { h->oseg_state = 6; h->oseg_pending = 0; return 1; }
    if (r < 0) { h->oseg_state = 0; h->oseg_pending = 0; return r; }
    h->oseg_state = 1;
    r = oseg_launch_bboxes(h);
    if (r < 0) { h->oseg_state = 0; h->oseg_pending = 0; }
    return r;
}
// the host-mask form behind its checks; snap: the deferred entry's ticket (ifx_owner_segmentation_begin_deferred), null for the ordinary one
static int oseg_begin_host(ifx* h, SegSnap* snap, int ticket, const uint8_t* rgb, const uint16_t* depth, const uint8_t* masks_in, const int32_t* class_ids, int nm, int frame, int flags)
{
    ifx_vlist_reap(h);
    h->seg_counts_valid = 0;
    h->oseg_ev = ifx_event_get(h);
    hipEventRecord(h->oseg_ev, h->cur);
    HIPCHK(h, hipStreamSynchronize(h->cur));
    if (nm == 0) {   // (an empty shard still takes part: the other ranks wait for its boxes)
        h->event_pool.push_back(h->oseg_ev); h->oseg_ev = nullptr;
        if (snap) ifx_segmentation_snapshot_release(h, ticket);
        return 0;
    }
    const int P = h->P;
    const size_t mbytes = (size_t)nm * P;
    int r = ifx_ensure_masks(h, mbytes);
    if (r) return r;
    if ((r = oseg_set_view(h, snap, ticket))) return r;
    h->oseg_nm = nm; h->oseg_m = 0; h->oseg_flags = flags;
    h->oseg_unavail.assign(nm, 0);
    h->oseg_cmp.assign((size_t)nm * NI, 0);
    h->oseg_class.assign(class_ids, class_ids + nm);
    HIPCHK(h, hipMemcpyAsync(h->d_masks_ori, masks_in, mbytes, hipMemcpyHostToDevice, h->cur));
    HIPCHK(h, hipMemcpyAsync(h->d_masks, h->d_masks_ori, mbytes, hipMemcpyDeviceToDevice, h->cur));
    LAUNCH(h, "mask_clean_overlap", dim3(cdiv(P, 256)), dim3(256), k_mask_clean_overlap, h->d_masks, nm, P);
    if (flags & 2) {   // (a deferred call cuts the superpixels from the ticket's frame, read in place)
        r = snap ? ifx_superpixel_begin_device(h, h->oseg_view.d_rgb, h->oseg_view.d_depth) : ifx_superpixel_refine(h, rgb, depth, nm, frame);
        if (!r && snap) r = ifx_superpixel_filter(h, nm);
        if (r) return r;
    }
    return oseg_first_exchange(h);
}
extern "C" int ifx_owner_segmentation_begin(ifx_t* h, const uint8_t* rgb, const uint16_t* depth, const uint8_t* masks_in, const int32_t* class_ids, int nm, int frame, int flags)
{
    if (!h || nm < 0 || (nm > 0 && (!masks_in || !class_ids))) return IFX_E_INVALID;
    if (!h->own) { h->err = "ifx_owner_segmentation_begin: the handle was not created with n_ranks > 1"; return IFX_E_STATE; }
    if (flags & 1) { h->err = "kNN smoothing is not offered on a sharded map (it needs every rank's positions)"; return IFX_E_INVALID; }
    if (h->oseg_state) { h->err = "a segmentation call is already in flight"; return IFX_E_STATE; }
    if (nm > 256) { h->err = "too many masks"; return IFX_E_INVALID; }
    return oseg_begin_host(h, nullptr, -1, rgb, depth, masks_in, class_ids, nm, frame, flags);
}
static int oseg_resume(ifx* h);
static int oseg_resume_record(ifx* h);
extern "C" int ifx_owner_segmentation_resume(ifx_t* h)
{
    if (!h) return IFX_E_INVALID;
    if (!h->oseg_state) { h->err = "no segmentation call in flight"; return IFX_E_STATE; }
    const int r = oseg_resume(h);
    if (r < 0) {   // a failed call is over: the next _begin starts from scratch (a deferred call's ticket stays in use)
        h->oseg_state = 0; h->oseg_pending = 0; h->oseg_ticket = -1;
        if (h->oseg_ev) { h->event_pool.push_back(h->oseg_ev); h->oseg_ev = nullptr; }
    }
    return r;
}
static int oseg_resume(ifx* h)
{
    const int nm = h->oseg_nm, P = h->P;
    int r;
    switch (h->oseg_state) {
    case 7:   // the record arrived (device forms, root >= 0) -> the masks from it, then the exchange points of every form
        return oseg_resume_record(h);
    case 6:   // the id image's keys merged -> the image, then the boxes
        if ((r = ifx_owner_ids_resume_impl(h))) return r;
        h->oseg_state = 1;
        return oseg_launch_bboxes(h);
    case 1:   // boxes merged -> compare map; model depth of the owned surfels
        if ((r = oseg_read_bboxes(h))) return r;
        LAUNCH(h, "project_depth", dim3(cdiv(P, 256)), dim3(256), k_project_depth, h->d_state, h->oseg_view.ids, (const float4*)h->pc, P, 1186, h->d_pdm, h->oseg_view.im, h->oseg_view.cam);
        h->oseg_state = 2; h->oseg_pending = 2;
        return 1;
    case 2:   // model depth merged -> flood fill (replicated), then the masks
        HIPCHK(h, hipMemcpyAsync(h->d_unavail, h->oseg_unavail.data(), nm, hipMemcpyHostToDevice, h->cur));
        if ((r = mask_geometric_filter_device(h, h->d_pdm, h->d_masks, h->d_masks_ori, nm, h->d_unavail))) return r;
        HIPCHK(h, hipMemcpyAsync(h->oseg_unavail.data(), h->d_unavail, nm, hipMemcpyDeviceToHost, h->cur));
        HIPCHK(h, hipStreamSynchronize(h->cur));
        h->oseg_state = 5;
        return oseg_mask_loop(h, false);
    case 3:   // eviction statistics merged -> the twenty weakest leave the table, the boxes again
        if ((r = seg_evict_weakest(h))) return r;
        h->oseg_state = 4;
        return oseg_launch_bboxes(h);
    case 4:   // boxes after the eviction merged -> compare map again, the mask that asked for room goes on
        if ((r = oseg_read_bboxes(h))) return r;
        h->oseg_state = 5;
        return oseg_mask_loop(h, true);
    default: break;
    }
    h->err = "ifx_owner_segmentation_resume: bad state";
    return IFX_E_STATE;
}

// the masks of ifx_process_segmentation_device: the caller's n x P elements in device memory, their format, the class ids (device), and an event recorded on the
// producer's stream at entry (the ingestion waits for it; nothing before the ingestion does)
// ifx_process_segmentation_rois: roi = M > 0, d = n x M x M f32 ROI masks, d_boxes = n x 4 f32 (xyxy) -- pasted on the device in place of the n x P elements
struct DevMasks { const void* d; int fmt; float thr; const int32_t* d_cls; hipEvent_t ready; const float* d_boxes = nullptr; int roi = 0; };
// What a segmentation entry was handed, whichever form it came in: n masks on the host (0/255 bytes, sorted by the caller's bridge, with the optional host frame)
// or on the device (dm: image-sized masks, or ROI masks with boxes when dm.roi > 0; dm.ready is filled in by the entry body).
struct MaskSource {
    enum Kind { HOST, IMAGE, ROIS };
    int n; Kind kind;
    DevMasks dm;
    const uint8_t* rgb; const uint16_t* depth; const uint8_t* masks; const int32_t* cls;   // host form
};
static MaskSource src_host(const uint8_t* rgb, const uint16_t* depth, const uint8_t* masks, const int32_t* cls, int n) { return MaskSource{n, MaskSource::HOST, DevMasks{}, rgb, depth, masks, cls}; }
static MaskSource src_image(const void* d_masks, int fmt, float thr, const int32_t* d_cls, int n) { return MaskSource{n, MaskSource::IMAGE, DevMasks{d_masks, fmt, thr, d_cls, nullptr}, nullptr, nullptr, nullptr, nullptr}; }
static MaskSource src_rois(const float* d_rois, int M, const float* d_boxes, float thr, const int32_t* d_cls, int n)
{
    return MaskSource{n, MaskSource::ROIS, DevMasks{d_rois, IFX_MASK_F32, thr, d_cls, nullptr, d_boxes, M}, nullptr, nullptr, nullptr, nullptr};
}
static int process_segmentation_host(ifx_t* h, const uint8_t* rgb, const uint16_t* depth, const uint8_t* masks_in, const int32_t* class_ids, const DevMasks* dm, int nm, int frame, int flags);
static int process_segmentation_device(ifx_t* h, const uint8_t* rgb, const uint16_t* depth, const uint8_t* masks_in, const int32_t* class_ids, const DevMasks* dm, int nm, int frame, int flags,
                                       SegSnap* snap);
static int process_segmentation(ifx_t* h, const uint8_t* rgb, const uint16_t* depth, const uint8_t* masks_in, const int32_t* class_ids, const DevMasks* dm, int nm, int frame, int flags,
                                SegSnap* snap = nullptr);
static int seg_ingest_device(ifx* h, const DevMasks* dm, int nm, int* cls_out, uint8_t* unavail);
static int snap_for_call(ifx* h, const char* who, int ticket, int flags, SegSnap** out);

// ---- the one body behind the segmentation entries.  Its steps keep this order (the order decides which error a doubly-bad call reports): the arguments of the
// source's form, the refusal by mode, the producer's event, the call, the ticket's release.
static int seg_check_args(ifx* h, const char* who, const MaskSource& s)
{
    const char* bad = nullptr;
    if (s.n < 0 || s.n > 256) bad = ": n must be 0 .. 256";
    else if (s.kind == MaskSource::HOST) { if (s.n > 0 && (!s.masks || !s.cls)) bad = ": null masks or class ids"; }
    else if (s.kind == MaskSource::ROIS) {   // the mask head's ROI masks and boxes (maskrcnn_benchmark/modeling/roi_heads/mask_head/inference.py:91-154)
        if (s.dm.roi < 1 || s.dm.roi > ROI_M_MAX) bad = ": roi_size must be 1 .. 64";
        else if (s.n > 0 && (!s.dm.d || !s.dm.d_boxes || !s.dm.d_cls)) bad = ": null ROI masks, boxes or class ids";
    }
    else if (s.dm.fmt != IFX_MASK_U8 && s.dm.fmt != IFX_MASK_F32) bad = ": unknown mask format";
    else if (s.n > 0 && (!s.dm.d || !s.dm.d_cls)) bad = ": null masks or class ids";
    if (bad) { h->err = std::string(who) + bad; return IFX_E_INVALID; }
    return IFX_OK;
}
// ticket: the deferred entries' (snap_for_call refuses by mode and finds the pinned frame), null for the resident ones, of which only the device forms refuse a sharded map
static int seg_refuse_mode(ifx* h, const char* who, bool device, const int* ticket, int flags, SegSnap** snap)
{
    if (ticket) return snap_for_call(h, who, *ticket, flags, snap);
    if (device && (h->own || h->shard_n > 1)) { h->err = std::string(who) + ": a sharded map takes its masks from the host (ifx_owner_process_segmentation)"; return IFX_E_STATE; }
    return IFX_OK;
}
static int seg_record_ready(ifx* h, const char* who, DevMasks* dm, const PoolEvent& ready, void* stream)
{
    const hipError_t e = hipEventRecord(ready.ev, (hipStream_t)stream);   // what the producer enqueued before this call
    if (e != hipSuccess) { h->err = std::string(who) + ": hipEventRecord on the producer's stream: " + hipGetErrorString(e); return IFX_E_HIP; }
    dm->ready = ready.ev;
    return IFX_OK;
}
static int seg_run(ifx* h, const char* who, MaskSource& s, SegSnap* snap, const int* ticket, int frame, int flags, void* stream)
{
    int r;
    if (s.kind == MaskSource::HOST) r = process_segmentation(h, s.rgb, s.depth, s.masks, s.cls, nullptr, s.n, frame, flags, snap);
    else {
        PoolEvent ready(h);
        if ((r = seg_record_ready(h, who, &s.dm, ready, stream))) return r;
        r = process_segmentation(h, nullptr, nullptr, nullptr, nullptr, &s.dm, s.n, frame, flags, snap);
    }
    if (ticket && r == IFX_OK) ifx_segmentation_snapshot_release(h, *ticket);
    return r;
}
static int seg_entry(ifx* h, const char* who, MaskSource s, const int* ticket, int frame, int flags, void* stream)
{
    if (!h) return IFX_E_INVALID;
    SegSnap* snap = nullptr;
    int r = seg_check_args(h, who, s);
    if (r || (r = seg_refuse_mode(h, who, s.kind != MaskSource::HOST, ticket, flags, &snap))) return r;
    return seg_run(h, who, s, snap, ticket, frame, flags, stream);
}
// the ingestion alone (ifx_ingest_masks / ifx_paste_roi_masks): k_mask_area / k_roi_area, k_mask_order and the gather as the full call launches them, then what the caller asked to see
static int seg_stage_entry(ifx* h, const char* who, MaskSource s, void* stream, uint8_t* out_ori, uint8_t* out_clean, int32_t* out_order, int32_t* out_class_ids)
{
    if (!h) return IFX_E_INVALID;
    int r = seg_check_args(h, who, s);
    if (r) return r;
    if (h->own || h->shard_n > 1) { h->err = std::string(who) + ": not on a sharded map"; return IFX_E_STATE; }
    const int n = s.n;
    if (n == 0) return IFX_OK;
    const size_t bytes = (size_t)n * h->P;
    if ((r = ifx_ensure_masks(h, bytes))) return r;
    {
        PoolEvent ready(h);
        if ((r = seg_record_ready(h, who, &s.dm, ready, stream)) || (r = seg_ingest_device(h, &s.dm, n, nullptr, nullptr))) return r;
    }
    if (out_ori) HIPCHK(h, hipMemcpyAsync(out_ori, h->d_masks_ori, bytes, hipMemcpyDeviceToHost, h->cur));
    if (out_clean) HIPCHK(h, hipMemcpyAsync(out_clean, h->d_masks, bytes, hipMemcpyDeviceToHost, h->cur));
    if (out_order) HIPCHK(h, hipMemcpyAsync(out_order, h->d_mask_rank + 256, (size_t)n * 4, hipMemcpyDeviceToHost, h->cur));
    if (out_class_ids) HIPCHK(h, hipMemcpyAsync(out_class_ids, h->d_mask_rank + 512, (size_t)n * 4, hipMemcpyDeviceToHost, h->cur));
    HIPCHK(h, hipStreamSynchronize(h->cur));
    return IFX_OK;
}
// The mask head's logits (ifx_mask_head_select's inputs): behind the checks, the stage runs into the handle's scratch on the producer's stream, kept comes back, and
// the ROI form's path takes the scratch pointers -- seg_ingest_rois, k_roi_area, k_roi_gather and k_mask_order as they are.
static int seg_entry_detections(ifx* h, const char* who, const int* ticket, const float* d_mask_logits, const float* d_boxes, const float* d_scores, const int64_t* d_labels,
                                const int32_t* d_count, const int32_t* d_class_map, int R, int C, int M, const ifx_mask_head_params* p, float threshold, int frame, int flags,
                                void* stream, int32_t* out_kept)
{
    if (!h) return IFX_E_INVALID;
    SegSnap* snap = nullptr;
    int r = ifx_mask_head_check(h, who, d_mask_logits, d_boxes, d_scores, d_labels, R, C, M, p, false);
    if (r || (r = seg_refuse_mode(h, who, true, ticket, flags, &snap))) return r;
    const float *rois = nullptr, *boxes = nullptr;
    const int32_t* cls = nullptr;
    int kept = 0;
    if ((r = ifx_mask_head_stage(h, who, d_mask_logits, d_boxes, d_scores, d_labels, d_count, d_class_map, R, C, M, p, stream, &rois, &boxes, &cls, &kept))) return r;
    if (out_kept) *out_kept = kept;
    if (kept > 256) { h->err = std::string(who) + ": more than 256 detections kept (raise score_thresh)"; return IFX_E_CAPACITY; }
    MaskSource s = src_rois(rois, M, boxes, threshold, cls, kept);
    return seg_run(h, who, s, snap, ticket, frame, flags, stream);   // (the event: the stage, and what the producer enqueued before this call)
}
// The default detector's output (ifx_unmold_detections' inputs): behind the checks, the stage runs into the handle's scratch on the producer's stream, kept comes
// back, and the image form's path takes the scratch pointers as u8 masks -- seg_ingest_launch, k_mask_area, k_mask_order and the gather as they are.
static int seg_entry_unmolded(ifx* h, const char* who, const int* ticket, const float* d_det, const float* d_masks, const int32_t* window, const int32_t* d_class_map,
                              int R, int M, int C, int layout, int frame, int flags, void* stream, int32_t* out_kept)
{
    if (!h) return IFX_E_INVALID;
    SegSnap* snap = nullptr;
    int r = ifx_unmold_check(h, who, d_det, d_masks, window, R, M, C, layout, 256);
    if (r || (r = seg_refuse_mode(h, who, true, ticket, flags, &snap))) return r;
    const uint8_t* masks = nullptr;
    const int32_t* cls = nullptr;
    int kept = 0;
    if ((r = ifx_unmold_stage(h, who, d_det, d_masks, window, d_class_map, R, M, C, layout, stream, &masks, &cls, &kept))) return r;
    if (out_kept) *out_kept = kept;
    MaskSource s = src_image(masks, IFX_MASK_U8, 0.5f, cls, kept);
    return seg_run(h, who, s, snap, ticket, frame, flags, stream);   // (the event: the stage, and what the producer enqueued before this call)
}

extern "C" int ifx_process_segmentation(ifx_t* h, const uint8_t* rgb, const uint16_t* depth, const uint8_t* masks_in, const int32_t* class_ids, int nm, int frame, int flags)
{
    return seg_entry(h, "ifx_process_segmentation", src_host(rgb, depth, masks_in, class_ids, nm), nullptr, frame, flags, nullptr);
}
extern "C" int ifx_process_segmentation_device(ifx_t* h, const void* d_masks, int mask_format, float threshold, const int32_t* d_class_ids, int n, int frame, int flags, void* stream)
{
    return seg_entry(h, "ifx_process_segmentation_device", src_image(d_masks, mask_format, threshold, d_class_ids, n), nullptr, frame, flags, stream);
}
extern "C" int ifx_process_segmentation_rois(ifx_t* h, const float* d_roi_masks, int roi_size, const float* d_boxes, float threshold, const int32_t* d_class_ids, int n, int frame, int flags,
                                             void* stream)
{
    return seg_entry(h, "ifx_process_segmentation_rois", src_rois(d_roi_masks, roi_size, d_boxes, threshold, d_class_ids, n), nullptr, frame, flags, stream);
}
extern "C" int ifx_process_segmentation_detections(ifx_t* h, const float* d_mask_logits, const float* d_boxes, const float* d_scores, const int64_t* d_labels, const int32_t* d_count,
                                                   const int32_t* d_class_map, int R, int C, int M, const ifx_mask_head_params* p, float threshold, int frame, int flags, void* stream,
                                                   int32_t* out_kept)
{
    return seg_entry_detections(h, "ifx_process_segmentation_detections", nullptr, d_mask_logits, d_boxes, d_scores, d_labels, d_count, d_class_map, R, C, M, p, threshold, frame, flags,
                                stream, out_kept);
}
extern "C" int ifx_process_segmentation_deferred(ifx_t* h, int ticket, const uint8_t* masks_in, const int32_t* class_ids, int nm, int frame, int flags)
{
    return seg_entry(h, "ifx_process_segmentation_deferred", src_host(nullptr, nullptr, masks_in, class_ids, nm), &ticket, frame, flags, nullptr);
}
extern "C" int ifx_process_segmentation_deferred_device(ifx_t* h, int ticket, const void* d_masks, int mask_format, float threshold, const int32_t* d_class_ids, int n, int frame, int flags,
                                                        void* stream)
{
    return seg_entry(h, "ifx_process_segmentation_deferred_device", src_image(d_masks, mask_format, threshold, d_class_ids, n), &ticket, frame, flags, stream);
}
extern "C" int ifx_process_segmentation_deferred_rois(ifx_t* h, int ticket, const float* d_roi_masks, int roi_size, const float* d_boxes, float threshold, const int32_t* d_class_ids, int n,
                                                      int frame, int flags, void* stream)
{
    return seg_entry(h, "ifx_process_segmentation_deferred_rois", src_rois(d_roi_masks, roi_size, d_boxes, threshold, d_class_ids, n), &ticket, frame, flags, stream);
}
extern "C" int ifx_process_segmentation_deferred_detections(ifx_t* h, int ticket, const float* d_mask_logits, const float* d_boxes, const float* d_scores, const int64_t* d_labels,
                                                            const int32_t* d_count, const int32_t* d_class_map, int R, int C, int M, const ifx_mask_head_params* p, float threshold,
                                                            int frame, int flags, void* stream, int32_t* out_kept)
{
    return seg_entry_detections(h, "ifx_process_segmentation_deferred_detections", &ticket, d_mask_logits, d_boxes, d_scores, d_labels, d_count, d_class_map, R, C, M, p, threshold, frame,
                                flags, stream, out_kept);
}
extern "C" int ifx_process_segmentation_unmolded(ifx_t* h, const float* d_detections, const float* d_masks, const int32_t* window, const int32_t* d_class_map, int R, int M,
                                                 int C, int layout, int frame, int flags, void* stream, int32_t* out_kept)
{
    return seg_entry_unmolded(h, "ifx_process_segmentation_unmolded", nullptr, d_detections, d_masks, window, d_class_map, R, M, C, layout, frame, flags, stream, out_kept);
}
extern "C" int ifx_process_segmentation_deferred_unmolded(ifx_t* h, int ticket, const float* d_detections, const float* d_masks, const int32_t* window,
                                                          const int32_t* d_class_map, int R, int M, int C, int layout, int frame, int flags, void* stream,
                                                          int32_t* out_kept)
{
    return seg_entry_unmolded(h, "ifx_process_segmentation_deferred_unmolded", &ticket, d_detections, d_masks, window, d_class_map, R, M, C, layout, frame, flags, stream,
                              out_kept);
}
extern "C" int ifx_paste_roi_masks(ifx_t* h, const float* d_roi_masks, int roi_size, const float* d_boxes, float threshold, const int32_t* d_class_ids, int n, void* stream, uint8_t* out_ori,
                                   uint8_t* out_clean, int32_t* out_order, int32_t* out_class_ids)
{
    return seg_stage_entry(h, "ifx_paste_roi_masks", src_rois(d_roi_masks, roi_size, d_boxes, threshold, d_class_ids, n), stream, out_ori, out_clean, out_order, out_class_ids);
}
extern "C" int ifx_ingest_masks(ifx_t* h, const void* d_masks, int mask_format, float threshold, const int32_t* d_class_ids, int n, void* stream, uint8_t* out_ori, uint8_t* out_clean,
                                int32_t* out_order, int32_t* out_class_ids)
{
    return seg_stage_entry(h, "ifx_ingest_masks", src_image(d_masks, mask_format, threshold, d_class_ids, n), stream, out_ori, out_clean, out_order, out_class_ids);
}
static int process_segmentation(ifx_t* h, const uint8_t* rgb, const uint16_t* depth, const uint8_t* masks_in, const int32_t* class_ids, const DevMasks* dm, int nm, int frame, int flags,
                                SegSnap* snap)
{
    // The next frame's tracker is already queued on the main stream (enqueue_frame, "tracked ahead") and touches nothing this call does: the call's ~60 short
    // launches then go to the handle's third stream (the loop-closure tracker's: four streams is what the runtime's hardware queues hold) and run beside the tracker's 170 instead of behind them.  The call ends with the host waiting for its stream,
    // so whatever the caller enqueues next is ordered behind it as before.
    const bool aside = h->opt_seg_aside && h->stream_c && h->opt_two_streams && h->opt_seg_device && !h->own && h->tracked_ahead == h->tick && h->cur == h->stream &&
                       !h->lc_pending;   // (the third stream is busy with a loop-closure tracker: behind the frame tracker on the main stream is the shorter wait)
    if (aside) {
        if (h->ev_result) HIPCHK(h, hipStreamWaitEvent(h->stream_c, h->ev_result, 0));   // behind the frame the call belongs to
        h->cur = h->stream_c;
    }
    // (a deferred call always takes the device schedule: both give identical results, and only this one reads through the view everywhere)
    const int r = (h->opt_seg_device || snap) ? process_segmentation_device(h, rgb, depth, masks_in, class_ids, dm, nm, frame, flags, snap)
                                              : process_segmentation_host(h, rgb, depth, masks_in, class_ids, dm, nm, frame, flags);
    if (aside) { hipStreamSynchronize(h->stream_c); h->cur = h->stream; }
    // a call that failed part-way may have updated votes without the label scan that follows them: the incremental scan of the next call assumes
    // that votes outside its own id image are unchanged since the last scan, so the next call scans everything
    if (r != IFX_OK) h->labels_stale_all = 1;
    return r;
}

// step 2 on the host, behind run_bboxes: the box rule, or (option compare_map 2) the mask rule -- the count kernels of the device schedule, the tables read back
static int seg_compare_maps(ifx* h, const SegView& v, int nm, const int32_t* class_ids, const std::vector<int>& bbox, std::vector<uint8_t>& unavailable, std::vector<int>& cmp)
{
    if (h->opt_compare_map != 2) { compare_map(h, &bbox[NI * 4], &bbox[0], class_ids, nm, unavailable, cmp); return IFX_OK; }
    std::vector<int> tab;
    const int r = cmp_tables_host(h, v.ids, nm, tab);
    if (r) return r;
    compare_map_iou(h, tab.data(), &bbox[NI * 4], class_ids, nm, unavailable, cmp);
    return IFX_OK;
}

// step 3 of processInstance (IF/Core/InstanceFusion.cpp:955-1040) from mask m_start on, driven by the host: registration, the eviction of a full table
// (computeMaxCountInMap, getInstanceTableCleanList, cleanInstanceTableMap, boxes and compare map again), one vote launch per (mask, instance)
static int seg_host_mask_loop(ifx* h, const SegView& v, int nm, const int32_t* class_ids, int m_start, std::vector<int>& cmp, std::vector<uint8_t>& unavailable, std::vector<int>& bbox)
{
    const int P = h->P;
    int r;
    for (int m = m_start; m < nm; m++) {
        bool exist = false;
        int reg = -1;
        for (int q = 0; q < NI; q++) if (cmp[q + m * NI] == 1) { exist = true; break; }
        if (!exist && !unavailable[m]) {
            int empty = first_not_used(h);
            if (empty == -1) {
                h->clean_times++;
                HIPCHK(h, hipMemsetAsync(h->d_inst_stats, 0, NI * 2 * 4, h->cur));
                LAUNCH(h, "max_count", dim3(1024), dim3(256), k_max_count, h->d_state, (const float4*)h->votes, h->cap, (const float2*)h->tm, h->d_inst_stats, h->d_inst_stats + NI);
                if ((r = seg_evict_weakest(h))) return r;
                h->labels_stale_all = 1;   // votes of every surfel that carried an evicted instance changed
                r = run_bboxes(h, v, nm, bbox);
                if (r) return r;
                std::fill(cmp.begin(), cmp.end(), 0);
                if ((r = seg_compare_maps(h, v, nm, class_ids, bbox, unavailable, cmp))) return r;   // (the mask rule again under compare_map 2, on the votes as the eviction left them: DESIGN.md section 1)
                empty = first_not_used(h);
            }
            if (empty >= 0) { h->inst_class[empty] = class_ids[m]; cmp[empty + m * NI] = 1; reg = empty; }
        }
        // what the call decided for this mask (ifx_segmentation_matches): the match of the compare map the mask met (the one after an eviction it caused), and the
        // instance it votes for -- the slot it registered, if it did (as in the reference, a mask that the recomputed map matches after all votes for both)
        h->seg_last_best[m] = -1;
        for (int q = NI - 1; q >= 0; q--) if (cmp[q + m * NI] == 1 && q != reg) h->seg_last_best[m] = q;
        h->seg_last_target[m] = reg >= 0 ? reg : h->seg_last_best[m];
        for (int q = 0; q < NI; q++)
            if (cmp[q + m * NI] == 1)
                LAUNCH(h, "vote_update", dim3(cdiv(P, 256)), dim3(256), k_vote_update, h->d_state, v.ids, h->d_masks + (size_t)m * P, P, h->cap, q, m + 1, h->votes, ifx_idmap(h));
    }
    return IFX_OK;
}
// step 4: the label scan (countAndColourSurfelMap) -- restricted to what a call can have changed unless the votes were rewritten wholesale
// `gate`: device pointer to (ff_incomplete, evict_at) of the device-side call, or null.  Returns 1 when the scan enqueued was the full one.
// default_done: the caller already ran k_colour_default in this call (it reads nothing a call changes -- a surfel whose votes the call then touches is recoloured by
// k_count_colour_px, which treats the default colour as "none yet" -- so the device-scheduled call enqueues it before the masks are staged)
static int seg_label_scan(ifx* h, const SegView& v, const int* gate = nullptr, bool default_done = false)
{
    const int P = h->P;
    if (!h->labels_stale_all) {
        if (!default_done) LAUNCH(h, "colour_default", dim3(2048), dim3(256), k_colour_default, h->d_state, (const float2*)h->tm, (float2*)h->col, h->labels, gate);
        LAUNCH(h, "count_colour_px", dim3(cdiv(P, 256)), dim3(256), k_count_colour_px, h->d_state, v.ids, P, (const float4*)h->votes, h->cap, (const float2*)h->tm, (float2*)h->col,
               h->d_inst_color, h->labels, ifx_idmap(h), gate);
        return 0;
    }
    LAUNCH(h, "count_colour", dim3(2048), dim3(256), k_count_colour, h->d_state, (const float4*)h->votes, h->cap, (const float2*)h->tm, (float2*)h->col, h->d_inst_color, h->labels, gate);
    h->labels_stale_all = 0;
    return 1;
}

// The ingestion of the device entry's masks, behind the producer's event: inside-pixel counts, the bridge's order (class ids in that order to cls_out, device [nm]),
// then d_masks_ori / d_masks in sorted order and the verdict bytes cleared (unavail, or none) -- three launches for the host entry's upload + overlap clean.
template <typename T>
static int seg_ingest_launch(ifx* h, const T* src, float thr, const int32_t* d_cls, int nm, int* cls_out, uint8_t* unavail)
{
    constexpr int V = 16 / sizeof(T);
    const int P = h->P;
    int* area = h->d_mask_rank;
    int* order = area + 256;
    LAUNCH(h, "mask_area", dim3(std::max(1, cdiv(P / V, MI_THREADS * MI_ITER)), nm), dim3(MI_THREADS), k_mask_area<T>, src, P, thr, area);
    LAUNCH(h, "mask_order", dim3(1), dim3(256), k_mask_order, area, d_cls, nm, order, cls_out);
    const int vec = ((uintptr_t)src % 16 == 0 && P % V == 0) ? 1 : 0;   // every mask then starts on a 16-B boundary, and so does every V-pixel group of the outputs
    LAUNCH(h, "mask_gather", dim3(cdiv(cdiv(P, V), MI_THREADS)), dim3(MI_THREADS), k_mask_gather<T>, src, P, thr, (const int*)order, nm, vec, h->d_masks_ori, h->d_masks, unavail);
    return IFX_OK;
}
// The same three steps on ROI masks and boxes: k_roi_area counts what k_roi_gather will paste, k_mask_order as it is.  (M + 2) / M in double, rounded once, as
// expand_masks computes it in Python.
static int seg_ingest_rois(ifx* h, const DevMasks* dm, int nm, int* cls_out, uint8_t* unavail)
{
    const int P = h->P, M = dm->roi;
    const float* rois = (const float*)dm->d;
    const float scale = (float)((double)(M + 2) / (double)M);
    static_assert(ROI_PX == 16, "k_roi_gather stores its group as one 16-B word");
    if (P % ROI_PX) { h->err = "ROI paste: width x height is not a multiple of 16"; return IFX_E_STATE; }   // (ifx_create admits multiples of 4 only: every group of the outputs starts on a 16-B boundary)
    int* area = h->d_mask_rank;
    int* order = area + 256;
    LAUNCH(h, "roi_area", dim3(cdiv(P, MI_THREADS * ROI_PX), nm), dim3(MI_THREADS), k_roi_area, rois, M, dm->d_boxes, scale, dm->thr, h->w, h->h, area);
    LAUNCH(h, "mask_order", dim3(1), dim3(256), k_mask_order, area, dm->d_cls, nm, order, cls_out);
    LAUNCH(h, "roi_gather", dim3(cdiv(P / ROI_PX, MI_THREADS)), dim3(MI_THREADS), k_roi_gather, rois, M, dm->d_boxes, scale, dm->thr, h->w, h->h, (const int*)order, nm,
           h->d_masks_ori, h->d_masks, unavail);
    return IFX_OK;
}
static int seg_ingest_device(ifx* h, const DevMasks* dm, int nm, int* cls_out, uint8_t* unavail)
{
    if (!h->d_mask_rank) {
        HIPCHK(h, hipMalloc(&h->d_mask_rank, 3 * 256 * sizeof(int)));
        HIPCHK(h, hipMemsetAsync(h->d_mask_rank, 0, 256 * sizeof(int), h->cur));   // the counters; k_mask_order leaves them zero for the next call
    }
    HIPCHK(h, hipStreamWaitEvent(h->cur, dm->ready, 0));   // behind what the producer enqueued before the call (no host synchronisation)
    if (!cls_out) cls_out = h->d_mask_rank + 512;
    if (dm->roi) return seg_ingest_rois(h, dm, nm, cls_out, unavail);
    return dm->fmt == IFX_MASK_F32 ? seg_ingest_launch(h, (const float*)dm->d, dm->thr, dm->d_cls, nm, cls_out, unavail)
                                   : seg_ingest_launch(h, (const uint8_t*)dm->d, dm->thr, dm->d_cls, nm, cls_out, unavail);
}

// ------------------------------------------------------------------ the device forms of a segmentation call on a sharded map
// ifx_owner_segmentation_begin_device / _rois / _detections (include/ifx_c_api.h).  root = -1: every rank holds the tensors and ingests its own copy, the call goes on
// as the host form does behind its upload and overlap clean.  root = r: rank r packs the record on its main stream behind an event on the producer's stream (no host
// synchronisation), the call's first exchange point broadcasts it (ifx_owner_exchange(h, 200): op 4 | r << 8), and the first resume ingests from it on every rank,
// rank r included: identical kernels on identical bytes.
static size_t oseg_record_words(int form, int max_n, int M, int P)
{
    return OSEG_HDR + (size_t)max_n + (form == 2 ? (size_t)max_n * 4 + (size_t)max_n * M * M : (size_t)max_n * ((P + 31) / 32));
}
// the call is over before its end (a failure, or no masks): the event goes back, the state is cleared
static int oseg_end(ifx* h, int r)
{
    if (h->oseg_ev) { h->event_pool.push_back(h->oseg_ev); h->oseg_ev = nullptr; }
    h->oseg_state = 0; h->oseg_pending = 0;
    if (r == 0) oseg_release_ticket(h);   // (no masks: the call is complete)
    h->oseg_ticket = -1;
    return r;
}
// n masks are coming: the buffers and the host state of a call, as ifx_owner_segmentation_begin sets them
static int oseg_prepare(ifx* h, int n)
{
    int r = ifx_ensure_masks(h, (size_t)n * h->P);
    if (r) return r;
    h->oseg_nm = n; h->oseg_m = 0;
    h->oseg_unavail.assign(n, 0);
    h->oseg_cmp.assign((size_t)n * NI, 0);
    h->oseg_class.assign(n, 0);
    if (!h->d_mask_rank) {
        HIPCHK(h, hipMalloc(&h->d_mask_rank, 3 * 256 * sizeof(int)));
        HIPCHK(h, hipMemsetAsync(h->d_mask_rank, 0, 256 * sizeof(int), h->cur));   // the counters; k_mask_order leaves them zero for the next call
    }
    return IFX_OK;
}
// the class ids in sorted order, for the compare map (oseg_read_bboxes synchronises before it reads them)
static int oseg_read_classes(ifx* h)
{
    HIPCHK(h, hipMemcpyAsync(h->oseg_class.data(), h->d_mask_rank + 512, (size_t)h->oseg_nm * 4, hipMemcpyDeviceToHost, h->cur));
    return IFX_OK;
}
// s: the tensors of the reading rank (root = -1: every rank; otherwise rank root) -- ignored on the others; form 1 image masks, 2 ROI masks (M = roi_size)
// snap: the deferred entry's ticket (the superpixels are then cut from its frame, read in place: rgb / depth are null), null for the ordinary ones
static int oseg_begin_dev(ifx* h, const char* who, int root, int max_n, const uint8_t* rgb, const uint16_t* depth, MaskSource s, int n_hdr, int form, int M, float thr, int frame,
                          int flags, void* stream, SegSnap* snap = nullptr, int ticket = -1)
{
    const int P = h->P, n = s.n;
    const bool reader = root < 0 || root == h->cfg.rank;
    h->seg_counts_valid = 0;
    ifx_vlist_reap(h);
    h->oseg_ev = ifx_event_get(h);
    hipEventRecord(h->oseg_ev, h->cur);
    HIPCHK(h, hipStreamSynchronize(h->cur));
    h->oseg_flags = flags; h->oseg_root = root; h->oseg_form = form; h->oseg_M = form == 2 ? M : 0; h->oseg_maxn = max_n; h->oseg_thr = thr; h->oseg_who = who;
    int r;
    if ((r = oseg_set_view(h, snap, ticket))) { h->oseg_ticket = -1; return oseg_end(h, r); }
    const SegView& v = h->oseg_view;
    if (root < 0) {
        if (n == 0) return oseg_end(h, 0);
        if ((r = oseg_prepare(h, n))) return oseg_end(h, r);
        {
            PoolEvent ready(h);
            if ((r = seg_record_ready(h, who, &s.dm, ready, stream)) || (r = seg_ingest_device(h, &s.dm, n, nullptr, nullptr))) return oseg_end(h, r);
        }
        if ((r = oseg_read_classes(h))) return oseg_end(h, r);
        if ((flags & 2) && (r = snap ? ifx_superpixel_begin_device(h, v.d_rgb, v.d_depth) : ifx_superpixel_refine(h, rgb, depth, n, frame))) return oseg_end(h, r);
        if ((flags & 2) && snap && (r = ifx_superpixel_filter(h, n))) return oseg_end(h, r);
        r = oseg_first_exchange(h);
        return r < 0 ? oseg_end(h, r) : r;
    }
    const size_t words = oseg_record_words(form, max_n, h->oseg_M, P);
    if (words > h->oseg_rec_cap) {
        if (h->oseg_rec) hipFree(h->oseg_rec);
        h->oseg_rec = nullptr; h->oseg_rec_cap = 0;
        hipError_t e = hipMalloc(&h->oseg_rec, words * 4);
        if (e != hipSuccess) { h->err = std::string(who) + ": the record: " + hipGetErrorString(e); return oseg_end(h, IFX_E_HIP); }
        h->oseg_rec_cap = words;
    }
    h->oseg_rec_bytes = words * 4;
    if (reader) {
        PoolEvent ready(h);
        if ((r = seg_record_ready(h, who, &s.dm, ready, stream))) return oseg_end(h, r);
        HIPCHK(h, hipStreamWaitEvent(h->cur, ready.ev, 0));   // behind what the producer enqueued before the call (no host synchronisation)
        int32_t* rec = h->oseg_rec;
        LAUNCH(h, "oseg_head", dim3(1), dim3(256), k_oseg_head, rec, form, n_hdr, n, h->oseg_M, P, max_n, s.dm.d_cls);
        uint32_t* body = (uint32_t*)rec + OSEG_HDR + max_n;
        if (form == 2) {
            const size_t total = (size_t)max_n * (4 + (size_t)M * M);
            LAUNCH(h, "oseg_pack_rois", dim3((unsigned)std::min<size_t>((total + 255) / 256, 1024)), dim3(256), k_oseg_pack_rois, body, n, max_n, M * M, (const uint32_t*)s.dm.d_boxes,
                   (const uint32_t*)s.dm.d);
        } else {
            const int NW = (P + 31) / 32;
            if (s.dm.fmt == IFX_MASK_F32) {
                const int vec = ((uintptr_t)s.dm.d % 16 == 0 && P % 4 == 0) ? 1 : 0;
                LAUNCH(h, "oseg_pack_bits", dim3(cdiv(vec ? NW * 8 : NW * 32, MI_THREADS), max_n), dim3(MI_THREADS), k_oseg_pack_bits<float>, (const float*)s.dm.d, P, thr, n, vec, body);
            } else {
                const int vec = ((uintptr_t)s.dm.d % 16 == 0 && P % 16 == 0) ? 1 : 0;
                LAUNCH(h, "oseg_pack_bits", dim3(cdiv(vec ? NW * 2 : NW * 32, MI_THREADS), max_n), dim3(MI_THREADS), k_oseg_pack_bits<uint8_t>, (const uint8_t*)s.dm.d, P, thr, n, vec, body);
            }
        }
    }
    if ((flags & 2) && (r = snap ? ifx_superpixel_begin_device(h, v.d_rgb, v.d_depth) : ifx_superpixel_begin(h, rgb, depth))) return oseg_end(h, r);   // (the frame's superpixels need no mask: the host pointers are done with when this returns)
    h->oseg_state = 7; h->oseg_pending = 4;
    return 1;
}
// the first resume of a call with root >= 0: the header in one 32-byte copy, checked against this rank's arguments; then the ingestion from the record
static int oseg_resume_record(ifx* h)
{
    const int P = h->P, max_n = h->oseg_maxn, M = h->oseg_M;
    const std::string who = h->oseg_who;
    int32_t hdr[OSEG_HDR];
    HIPCHK(h, hipMemcpyAsync(hdr, h->oseg_rec, sizeof(hdr), hipMemcpyDeviceToHost, h->cur));
    HIPCHK(h, hipStreamSynchronize(h->cur));
    if (hdr[0] != OSEG_MAGIC || hdr[1] != h->oseg_form || hdr[3] != M || hdr[4] != P || hdr[5] != max_n || hdr[2] < 0) {
        h->err = who + ": the record's header does not match this rank's arguments (the form, roi_size / M, max_n and the frame size must be equal on all ranks)";
        return IFX_E_STATE;
    }
    const int n = hdr[2];
    if (n > max_n) { h->err = who + ": more than max_n detections kept (raise score_thresh)"; return IFX_E_CAPACITY; }
    if (n == 0) return oseg_end(h, 0);
    int r = oseg_prepare(h, n);
    if (r) return r;
    const int32_t* cls = h->oseg_rec + OSEG_HDR;
    int* area = h->d_mask_rank;
    int* order = area + 256;
    int* cls_out = area + 512;
    if (h->oseg_form == 2) {
        DevMasks dm{h->oseg_rec + OSEG_HDR + max_n + (size_t)max_n * 4, IFX_MASK_F32, h->oseg_thr, cls, nullptr, (const float*)(h->oseg_rec + OSEG_HDR + max_n), M};
        if ((r = seg_ingest_rois(h, &dm, n, cls_out, nullptr))) return r;
    } else {
        if (P % 16) { h->err = who + ": width x height is not a multiple of 16"; return IFX_E_STATE; }   // (ifx_create admits multiples of 4 only)
        const int NW = (P + 31) / 32;
        const uint32_t* bits = (const uint32_t*)h->oseg_rec + OSEG_HDR + max_n;
        LAUNCH(h, "bits_area", dim3(cdiv(NW, MI_THREADS), n), dim3(MI_THREADS), k_bits_area, bits, NW, area);
        LAUNCH(h, "mask_order", dim3(1), dim3(256), k_mask_order, area, cls, n, order, cls_out);
        LAUNCH(h, "bits_gather", dim3(cdiv(P / 16, MI_THREADS)), dim3(MI_THREADS), k_bits_gather, bits, NW, P, (const int*)order, n, h->d_masks_ori, h->d_masks, (uint8_t*)nullptr);
    }
    if ((r = oseg_read_classes(h))) return r;
    if ((h->oseg_flags & 2) && (r = ifx_superpixel_filter(h, n))) return r;
    return oseg_first_exchange(h);
}
// what every device form refuses before it touches anything; who leads the message
static int oseg_refuse(ifx* h, const char* who, int root, int max_n, int flags)
{
    const char* bad = nullptr;
    int code = IFX_E_INVALID;
    if (!h->own) { bad = ": the handle was not created for a sharded map"; code = IFX_E_STATE; }
    else if (h->oseg_state) { bad = ": a segmentation call is already in flight"; code = IFX_E_STATE; }
    else if (flags & 1) bad = ": kNN smoothing is not offered on a sharded map's begin / resume (it needs every rank's positions)";
    else if (root < -1 || root >= h->own_g) bad = ": root must be -1 or a rank of the map";
    else if (max_n < 1 || max_n > 256) bad = ": max_n must be 1 .. 256";
    if (bad) { h->err = std::string(who) + bad; return code; }
    return IFX_OK;
}
static int oseg_snap_for_call(ifx* h, const char* who, int ticket, int flags, SegSnap** out);
// ticket: the deferred entry's (null for the ordinary ones)
static int oseg_entry(ifx* h, const char* who, int root, int max_n, const uint8_t* rgb, const uint16_t* depth, MaskSource s, float thr, int frame, int flags, void* stream,
                      const int* ticket = nullptr)
{
    if (!h) return IFX_E_INVALID;
    SegSnap* snap = nullptr;
    int r = oseg_refuse(h, who, root, max_n, flags);
    if (r || (ticket && (r = oseg_snap_for_call(h, who, *ticket, flags, &snap)))) return r;
    const bool rois = s.kind == MaskSource::ROIS;
    if (rois && (s.dm.roi < 1 || s.dm.roi > ROI_M_MAX)) { h->err = std::string(who) + ": roi_size must be 1 .. 64"; return IFX_E_INVALID; }   // (every rank: the record's size depends on it)
    if (root < 0 || root == h->cfg.rank) {
        if ((r = seg_check_args(h, who, s))) return r;
        if (s.n > max_n) { h->err = std::string(who) + ": n is larger than max_n"; return IFX_E_INVALID; }
    } else s.n = 0;
    return oseg_begin_dev(h, who, root, max_n, rgb, depth, s, s.n, rois ? 2 : 1, s.dm.roi, thr, frame, flags, stream, snap, ticket ? *ticket : -1);
}
// A call in flight ends here on this rank: what a rank does whose peers' call is over (their begin refused, their resume failed) while it waits at an exchange point
extern "C" int ifx_owner_segmentation_abort(ifx_t* h)
{
    if (!h) return IFX_E_INVALID;
    if (!h->own) { h->err = "ifx_owner_segmentation_abort: the handle was not created for a sharded map"; return IFX_E_STATE; }
    if (!h->oseg_state) return IFX_OK;
    HIPCHK(h, hipStreamSynchronize(h->cur));
    h->labels_stale_all = 1;   // (votes may have been updated without the label scan that follows them)
    h->oseg_ticket = -1;       // (a deferred call that did not complete keeps its ticket)
    return oseg_end(h, IFX_OK);
}
extern "C" int ifx_owner_segmentation_begin_device(ifx_t* h, int root, int max_n, const uint8_t* rgb, const uint16_t* depth, const void* d_masks, int mask_format, float threshold,
                                                   const int32_t* d_class_ids, int n, int frame, int flags, void* stream)
{
    return oseg_entry(h, "ifx_owner_segmentation_begin_device", root, max_n, rgb, depth, src_image(d_masks, mask_format, threshold, d_class_ids, n), threshold, frame, flags, stream);
}
extern "C" int ifx_owner_segmentation_begin_rois(ifx_t* h, int root, int max_n, const uint8_t* rgb, const uint16_t* depth, const float* d_roi_masks, int roi_size, const float* d_boxes,
                                                 float threshold, const int32_t* d_class_ids, int n, int frame, int flags, void* stream)
{
    return oseg_entry(h, "ifx_owner_segmentation_begin_rois", root, max_n, rgb, depth, src_rois(d_roi_masks, roi_size, d_boxes, threshold, d_class_ids, n), threshold, frame, flags, stream);
}
// the mask head's stage runs on the reading rank (into the handle's scratch, on the producer's stream; kept comes back), its kept rows are the ROI form's tensors.  More
// kept rows than the record holds: with root = -1 every rank refuses alike; with a root the record carries the count and no rows, and every rank refuses at its first resume.
extern "C" int ifx_owner_segmentation_begin_detections(ifx_t* h, int root, int max_n, const uint8_t* rgb, const uint16_t* depth, const float* d_mask_logits, const float* d_boxes,
                                                       const float* d_scores, const int64_t* d_labels, const int32_t* d_count, const int32_t* d_class_map, int R, int C, int M,
                                                       const ifx_mask_head_params* p, float threshold, int frame, int flags, void* stream, int32_t* out_kept)
{
    const char* who = "ifx_owner_segmentation_begin_detections";
    if (!h) return IFX_E_INVALID;
    int r = oseg_refuse(h, who, root, max_n, flags);
    if (r) return r;
    if (M < 1 || M > ROI_M_MAX) { h->err = std::string(who) + ": M must be 1 .. 64"; return IFX_E_INVALID; }
    const float *rois = nullptr, *boxes = nullptr;
    const int32_t* cls = nullptr;
    int kept = 0;
    if (root < 0 || root == h->cfg.rank) {
        if ((r = ifx_mask_head_check(h, who, d_mask_logits, d_boxes, d_scores, d_labels, R, C, M, p, false))) return r;
        if ((r = ifx_mask_head_stage(h, who, d_mask_logits, d_boxes, d_scores, d_labels, d_count, d_class_map, R, C, M, p, stream, &rois, &boxes, &cls, &kept))) return r;
        if (out_kept) *out_kept = kept;
        if (kept > max_n && root < 0) { h->err = std::string(who) + ": more than max_n detections kept (raise score_thresh)"; return IFX_E_CAPACITY; }
    }
    return oseg_begin_dev(h, who, root, max_n, rgb, depth, src_rois(rois, M, boxes, threshold, cls, kept > max_n ? 0 : kept), kept, 2, M, threshold, frame, flags, stream);
}

static int process_segmentation_host(ifx_t* h, const uint8_t* rgb, const uint16_t* depth, const uint8_t* masks_in, const int32_t* class_ids, const DevMasks* dm, int nm, int frame, int flags)
{
    ifx_ids_ensure(h);   // the call reads the id image under every mask pixel
    // Only the kNN smoothing looks at surfels the id image does not show: a slot outside the cached view list that has outlived the age rule
    // (ifx_map.hip "View list") is unstable, so it was never in an id image, carries no votes and takes part in nothing else of this call.
    if (flags & 1) ifx_vlist_reap(h);
    h->seg_counts_valid = 0;
    h->seg_last_nm = 0;
    PoolEvent ea(h);   // (given back on every return but the last, where stage_pending takes it)
    hipEventRecord(ea.ev, h->cur);
    HIPCHK(h, hipStreamSynchronize(h->cur));
    int n = 0;
    HIPCHK(h, hipMemcpy(&n, &h->d_state->count, sizeof(int), hipMemcpyDeviceToHost));
    if (nm == 0 || n == 0) return IFX_OK;
    const int P = h->P;
    size_t mbytes = (size_t)nm * P;
    std::vector<uint8_t> unavailable(nm, 0);
    int r = ifx_ensure_masks(h, mbytes);
    if (r) return r;
    std::vector<int32_t> cls_sorted;
    if (dm) {   // the caller's device masks: sorted, binarised and cleaned on the device; the class ids in that order come back before compare_map (run_bboxes synchronises)
        if ((r = seg_ingest_device(h, dm, nm, nullptr, nullptr))) return r;
        cls_sorted.resize(nm);
        HIPCHK(h, hipMemcpyAsync(cls_sorted.data(), h->d_mask_rank + 512, (size_t)nm * 4, hipMemcpyDeviceToHost, h->cur));
        class_ids = cls_sorted.data();
    } else {
        // the masks stay on the device from here on: d_masks_ori = "BAK ORI MASK" (:705-706), d_masks = working copy
        HIPCHK(h, hipMemcpyAsync(h->d_masks_ori, masks_in, mbytes, hipMemcpyHostToDevice, h->cur));
        HIPCHK(h, hipMemcpyAsync(h->d_masks, h->d_masks_ori, mbytes, hipMemcpyDeviceToDevice, h->cur));
        // step 0_1
        LAUNCH(h, "mask_clean_overlap", dim3(cdiv(P, 256)), dim3(256), k_mask_clean_overlap, h->d_masks, nm, P);
    }
    // steps -1_1 .. -1_3 (superpixel refinement)
    if (flags & 2) {
        r = ifx_superpixel_refine(h, rgb, depth, nm, frame);
        if (r) return r;
    }
    // steps 1, 2
    const SegView v = seg_view_current(h);
    std::vector<int> bbox;
    r = run_bboxes(h, v, nm, bbox);
    if (r) return r;
    std::vector<int> cmp((size_t)nm * NI, 0);
    if ((r = seg_compare_maps(h, v, nm, class_ids, bbox, unavailable, cmp))) return r;
    // step 3_0: model depth under the camera, then the flood fill of every usable mask (device)
    LAUNCH(h, "project_depth", dim3(cdiv(P, 256)), dim3(256), k_project_depth, h->d_state, v.ids, (const float4*)h->pc, P, 1186, h->d_pdm, ifx_idmap(h), v.cam);
    HIPCHK(h, hipMemcpyAsync(h->d_unavail, unavailable.data(), nm, hipMemcpyHostToDevice, h->cur));
    r = mask_geometric_filter_device(h, h->d_pdm, h->d_masks, h->d_masks_ori, nm, h->d_unavail);
    if (r) return r;
    HIPCHK(h, hipMemcpyAsync(unavailable.data(), h->d_unavail, nm, hipMemcpyDeviceToHost, h->cur));
    HIPCHK(h, hipStreamSynchronize(h->cur));
    // step 3
    r = seg_host_mask_loop(h, v, nm, class_ids, 0, cmp, unavailable, bbox);
    if (r) return r;
    // step 4
    seg_label_scan(h, v);
    // flannKnnVoteSurfelMap (isflann, :1051)
    if (flags & 1) { r = ifx_knn_vote(h, nullptr); if (r) return r; }
    ifx_stage_span_end(h, 2, ea);
    HIPCHK(h, hipStreamSynchronize(h->cur));
    h->seg_last_nm = nm;
    return IFX_OK;
}

// ---- the same call without the host in the middle of it (default; ifx_set_option("seg_device", 0) restores the host-driven schedule above).
// Round 2's call cost 1.4-1.8 ms -- two frames -- of which the kernels were ~0.8: the host waited for the stream at entry (behind the NEXT frame's tracker, enqueued
// ahead), copied the masks from pageable memory, read the superpixel table back for connectSuperPixel, read the boxes back for computeCompareMap, looked at the
// flood fill every 7 relaxations, read the verdicts back, and decided registration mask by mask.  Here: pinned staging, connectSuperPixel on the device
// (ifx_slic.hip: k_sp_connect), compare map and registration in two tiny kernels on a device copy of the instance table, a FIXED schedule of flood-fill
// relaxations (the ones behind the fixpoint return at once), one vote launch per mask that looks its target up on the device -- and ONE synchronisation at the end,
// which brings back the table, the verdicts and two flags: "the fill did not converge inside its schedule" and "the table was full at mask m".  Both are rare and
// are finished the old way from exactly that point (results identical either way: tests/test_gpu_parity.py::test_segmentation_device_schedule_equals_host_schedule).
struct SegCtl { int ff_incomplete, evict_at, nm, pad; int inst_class[NI]; int cls[256]; int best[256]; int target[256]; };
// computeCompareMap (IF/Core/InstanceFusion.cpp:595-651): one thread per mask; the LAST instance over the threshold wins, instance 0 never matches
__global__ void k_seg_compare(SegCtl* __restrict__ s, const int* __restrict__ bbox, uint8_t* __restrict__ unavailable)
{
    __shared__ int s_cls[NI], s_box[NI * 4];
    for (int t = threadIdx.x; t < NI; t += blockDim.x) s_cls[t] = s->inst_class[t];
    for (int t = threadIdx.x; t < NI * 4; t += blockDim.x) s_box[t] = bbox[t];
    __syncthreads();
    // a wave per mask, its lanes over the instances: "the last instance over the threshold" is the largest matching index (one mask per thread walked the
    // 96 instances one after the other: 13 us on the call's chain)
    const int lane = threadIdx.x & 63, nm = s->nm;
    for (int m = threadIdx.x >> 6; m < nm; m += blockDim.x >> 6) {
        const int* mb = bbox + (NI + m) * 4;
        const int minX_m = mb[0], maxX_m = mb[1], minY_m = mb[2], maxY_m = mb[3];
        if (maxX_m <= minX_m || maxY_m <= minY_m || unavailable[m]) {   // (wave-uniform)
            if (lane == 0) { s->target[m] = -1; unavailable[m] = 1; s->best[m] = -1; }
            continue;
        }
        const int cls = s->cls[m];
        int best = -1;
        for (int q = lane; q < NI; q += 64) {
            if (s_cls[q] == -1 || cls != s_cls[q]) continue;
            const int minX_i = s_box[q * 4], maxX_i = s_box[q * 4 + 1], minY_i = s_box[q * 4 + 2], maxY_i = s_box[q * 4 + 3];
            if (maxX_i <= minX_i || maxY_i <= minY_i) continue;
            const float IW = (float)(min(maxX_i, maxX_m) - max(minX_i, minX_m));
            const float IH = (float)(min(maxY_i, maxY_m) - max(minY_i, minY_m));
            if (IW <= 0 || IH <= 0) continue;
            const float I = IW * IH;
            const float U = (float)(((maxX_i - minX_i) * (maxY_i - minY_i)) + ((maxX_m - minX_m) * (maxY_m - minY_m))) - I;
            if (I / U > 0.5f) best = q;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
        if (lane == 0) { s->target[m] = -1; s->best[m] = best > 0 ? best : -1; }
    }
}
// The mask rule's decision (compare_map_iou on the device; IF/Core/InstanceFusion.cpp:834-861) over the tables of k_cmp_count: a wave per mask, its lanes over the
// instances, reduced on (iou descending, index ascending) -- the sequential loop's "replace iff iou > best so far".  Same side effects as k_seg_compare.
__global__ void k_seg_compare_iou(SegCtl* __restrict__ s, const int* __restrict__ bbox, uint8_t* __restrict__ unavailable, const int* __restrict__ tab)
{
    __shared__ int s_cls[NI], s_ai[NI];
    for (int t = threadIdx.x; t < NI; t += blockDim.x) { s_cls[t] = s->inst_class[t]; s_ai[t] = tab[CM_AI + t]; }
    __syncthreads();
    const int lane = threadIdx.x & 63, nm = s->nm;
    for (int m = threadIdx.x >> 6; m < nm; m += blockDim.x >> 6) {
        const int* mb = bbox + (NI + m) * 4;
        const int minX_m = mb[0], maxX_m = mb[1], minY_m = mb[2], maxY_m = mb[3];
        if (maxX_m <= minX_m || maxY_m <= minY_m || unavailable[m]) {   // (wave-uniform) plan A's degenerate-box test
            if (lane == 0) { s->target[m] = -1; unavailable[m] = 1; s->best[m] = -1; }
            continue;
        }
        const int cls = s->cls[m], am = tab[CM_AM + m];
        int best = -1;
        float best_iou = 0;
        for (int q = lane; q < NI; q += 64) {
            if (s_cls[q] == -1 || cls != s_cls[q]) continue;
            const int I = tab[CM_I + m * NI + q], U = am + s_ai[q] - I;
            const float iou = (float)I / (float)U;
            if (iou > 0.5f && iou > best_iou) { best = q; best_iou = iou; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int ob = __shfl_xor(best, o, 64);
            const float oi = __shfl_xor(best_iou, o, 64);
            if (ob >= 0 && (best < 0 || oi > best_iou || (oi == best_iou && ob < best))) { best = ob; best_iou = oi; }
        }
        if (lane == 0) { s->target[m] = -1; s->best[m] = best > 0 ? best : -1; }
    }
}
// the registration decisions of the mask loop (:955-1010), sequential as in the reference: a mask without a match that is still usable takes the first free
// slot of the table; when there is none the loop stops there (evict_at) and the host evicts (rare: 96 slots).  The table and the per-mask inputs are staged in LDS
// by the whole block; one lane then walks the masks.
// ff_meta / ff_skip (optional): the flood fill's per-mask counters -- the fill's verdict (k_ff_verdict: a mask that kept less than 65 % of its pixels is unusable) is
// taken here, while the per-mask inputs are staged, instead of in a launch of its own.
__global__ void k_seg_register(SegCtl* __restrict__ s, uint8_t* __restrict__ unavailable, const int* __restrict__ ff_gate, const int* __restrict__ ff_meta, const uint8_t* __restrict__ ff_skip)
{
    __shared__ int s_cls[NI], s_best[256], s_mcls[256], s_tgt[256];
    __shared__ unsigned char s_un[256];
    const int nm = s->nm;
    const int gate = ff_gate ? *ff_gate : 0;
    for (int t = threadIdx.x; t < NI; t += blockDim.x) s_cls[t] = s->inst_class[t];
    for (int t = threadIdx.x; t < nm; t += blockDim.x) {
        unsigned char un = unavailable[t];
        if (ff_meta && !gate && !ff_skip[t]) {
            const float finalPoints = (float)ff_meta[t * 32 + 2], oriPoints = (float)ff_meta[t * 32];
            if (finalPoints / oriPoints < 0.65f) { un = 1; unavailable[t] = 1; }
        }
        s_best[t] = s->best[t]; s_mcls[t] = s->cls[t]; s_un[t] = un; s_tgt[t] = -1;
    }
    __syncthreads();
    __shared__ int s_evict;
    if (threadIdx.x == 0) {
        s_evict = -1;
        if (!gate) {
            int next_free = 0;
            for (int m = 0; m < nm; m++) {
                int t = s_best[m];
                if (t < 0 && !s_un[m]) {
                    while (next_free < NI && s_cls[next_free] != -1) next_free++;   // the first free slot: slots only fill up during the loop, so the scan never goes back
                    if (next_free >= NI) { s_evict = m; break; }
                    s_cls[next_free] = s_mcls[m];
                    t = next_free;
                }
                s_tgt[m] = t;
            }
        }
        s->evict_at = s_evict;
        s->ff_incomplete = gate ? 1 : 0;
    }
    __syncthreads();
    if (gate) return;
    for (int t = threadIdx.x; t < NI; t += blockDim.x) s->inst_class[t] = s_cls[t];
    for (int t = threadIdx.x; t < nm; t += blockDim.x) s->target[t] = s_tgt[t];
}
// updateSurfelMapInstance (IF/Core/InstanceFusionCuda.cu:1100-1150) for mask m with the instance the device chose for it; a mask without one (or behind the
// point where the host takes over) is passed over.
// ONE launch per mask, in mask order, as the reference runs updateSurfelMapInstanceKernel once per mask (IF/Core/InstanceFusion.cpp:986-1000): the packed counters are lossy
// while a word's low half is negative (a surfel of the FIRST frame starts with -1 in every word, init_unstable.vert): each read-modify-write of the high half then loses 1 to
// the borrow of the low one, until a vote for the low half's instance makes it non-negative.  How many votes a surfel keeps therefore depends on WHICH MASK comes first --
// within a mask every update goes to the same half with the same weight and commutes, across masks it does not.
__global__ void k_vote_update_mask(const DevState* __restrict__ st, const int32_t* __restrict__ ids, const uint8_t* __restrict__ masks, int P, int cap, const SegCtl* __restrict__ s, int nm,
                                   float* __restrict__ votes, IdMap im, int m)
{
    if (s->ff_incomplete) return;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P) return;
    const int last = s->evict_at >= 0 ? min(nm, s->evict_at) : nm;
    if (m >= last || !(masks[(size_t)m * P + k] > 0)) return;
    const int instanceID = s->target[m];
    if (instanceID < 0) return;
    const int id = idmap_slot(im, st->count, ids[k]);
    if (id < 0) return;
    const int fi = instanceID / 2, p = instanceID % 2, inc = m + 1;
    unsigned int* addr = (unsigned int*)&VOTEF(votes, id, fi);
    unsigned int old = *addr, assumed;
    do {
        assumed = old;
        int a, b;
        vote_decode(__uint_as_float(assumed), a, b);
        if (p == 0) a += inc; else b += inc;
        if (a >= 65535) a = 65535;
        if (b >= 65535) b = 65535;
        old = atomicCAS(addr, assumed, __float_as_uint(vote_encode(a, b)));
    } while (old != assumed);
}

static int seg_ensure_ctl(ifx* h, size_t mask_bytes)
{
    if (!h->d_segctl) {
        HIPCHK(h, hipMalloc(&h->d_segctl, sizeof(SegCtl)));
        HIPCHK(h, hipHostMalloc((void**)&h->h_segctl, sizeof(SegCtl) + 256, hipHostMallocDefault));
    }
    if (mask_bytes > h->h_masks_cap) {
        if (h->h_masks_stage) hipHostFree(h->h_masks_stage);
        h->h_masks_stage = nullptr; h->h_masks_cap = 0;
        HIPCHK(h, hipHostMalloc((void**)&h->h_masks_stage, mask_bytes, hipHostMallocDefault));
        h->h_masks_cap = mask_bytes;
    }
    return IFX_OK;
}

// ------------------------------------------------------------------ deferred segmentation: a slow detector's masks of frame t, applied at frame t + k
// (ifx_segmentation_snapshot / ifx_process_segmentation_deferred[_device]; the reference has no counterpart: its detector thread is off, IF/main.cpp:83).
// A snapshot pins what a call reads of ITS frame -- the id image, the pose, optionally the raw frame -- and names every surfel by its creation number (ifx::seq:
// ascending in slot order, carried by the compaction, never reused), so that the image can be re-addressed in whatever slots the map has when the masks arrive.
struct SnapHdr { float pose[16]; int tick, pad[15]; };   // what one lane copies out of the state: the host reads nothing at snapshot time
#define SNAP_NONE 0xFFFFFFFFu
// id -> {creation number, slot as a hint}: 8 bytes per pixel.  have[block]: pixels of the block that name a surfel (ifx_segmentation_snapshot_stats).
// OWN (a shard of a spatially sharded map): the replicated id image holds creation numbers already, and every rank pins the WHOLE image; the hint is this rank's own
// slot -- the one bisection a pixel ever costs, here and not in every later launch -- or SNAP_NONE where another rank owns the surfel.  have counts the whole image,
// the same on every rank.
template <int OWN>
__global__ void __launch_bounds__(256) k_seg_snapshot(const DevState* __restrict__ st, const int32_t* __restrict__ ids, const uint32_t* __restrict__ seq, int P, int tick,
                                                      uint2* __restrict__ px, SnapHdr* __restrict__ hdr, int* __restrict__ have)
{
    const int count = st->count;   // launch-uniform: read once, before the first store
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int id = k < P ? ids[k] : 0;
    const bool has = OWN ? id != 0 : (id > 0 && id < count);
    if (OWN) {
        IdMap im; im.seq = seq; im.own_n = 1;
        const int mine = has ? idmap_slot(im, count, id) : -1;
        if (k < P) px[k] = make_uint2((unsigned int)id, mine >= 0 ? (unsigned int)mine : SNAP_NONE);
    } else if (k < P) px[k] = has ? make_uint2(seq[id], (unsigned int)id) : make_uint2(0u, SNAP_NONE);
    __shared__ int s_n[4];
    const unsigned long long bal = __ballot(has);
    if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) have[blockIdx.x] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    if (blockIdx.x == 0 && threadIdx.x == 64) {
        for (int q = 0; q < 16; q++) hdr->pose[q] = st->pose[q];
        hdr->tick = tick;
    }
}
// The pinned image in today's slots.  Compaction only moves a surfel DOWN and creation numbers ascend with the slots, so the surfel of a pixel sits at or below
// its old slot: the first probe, seq[min(hint, count - 1)], is the only load while nothing was compacted since the snapshot (the normal case with lazy compaction);
// otherwise a gallop downwards with doubling steps brackets the number and a bisection of the bracket finds it (a full bisection of 5 M slots is 23 dependent loads
// per pixel: DESIGN.md section 7 has what that costs).  A pixel keeps its surfel if it is still in the store, alive, and not today's "surfel 0" (first_live: never
// voted for); everything else reads 0 = no surfel.  lost[block]: pixels of the block that named a surfel and lost it.
// OWN (a shard): only the pixels with a hint -- the surfels this rank owned at the snapshot; ownership never changes -- are probed, the same way.  "Surfel 0" is a
// creation number there, the lowest live one of any rank (flw: the word the last frame's id resolve used, ifx_map.hip FIRST_LIVE; null under own_first_live = 0:
// creation number 0, which no id image names), and the image is written as slot + 1 (IDMAP_SLOTS: slot 0 of a shard is an ordinary surfel), 0 = no surfel of this
// rank.  lost counts the pixels whose surfel THIS rank owned and lost.
template <int OWN>
__global__ void __launch_bounds__(256) k_seg_translate(const DevState* __restrict__ st, const uint2* __restrict__ px, const uint32_t* __restrict__ seq, const float2* __restrict__ tm, int P,
                                                       int32_t* __restrict__ out, int* __restrict__ lost, const unsigned int* __restrict__ flw = nullptr)
{
    const int count = st->count;   // launch-uniform words: read once, before the first store ("Uniform loads")
    const unsigned int fl = OWN ? (flw ? *flw : 0u) : (unsigned int)st->first_live;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    int slot = 0;
    bool had = false;
    if (k < P) {
        const uint2 e = px[k];
        had = e.y != SNAP_NONE;
        if (had && count > 0) {
            const unsigned int want = e.x;
            const int j = min((int)e.y, count - 1);
            unsigned int v = seq[j];
            int found = -1;
            if (v == want) found = j;
            else if (v > want) {
                int hi = j, lo = j - 1, step = 1;   // seq[hi] > want throughout
                while (lo >= 0 && (v = seq[lo]) > want) { hi = lo; step <<= 1; lo -= step; }
                if (lo >= 0 && v == want) found = lo;
                else {
                    int a = lo < 0 ? -1 : lo;       // seq[a] < want (or a = -1), seq[hi] > want: the number, if still stored, lies strictly between
                    while (hi - a > 1) {
                        const int mid = (a + hi) >> 1;
                        v = seq[mid];
                        if (v == want) { found = mid; break; }
                        if (v < want) a = mid; else hi = mid;
                    }
                }
            }   // (v < want: every slot up to j carries a smaller number and the surfel cannot sit above its old slot -- compacted away)
            if (OWN) { if (found >= 0 && want != fl && tm[found].y > DEAD_TIME) slot = found + 1; }
            else if (found > 0 && found != (int)fl && tm[found].y > DEAD_TIME) slot = found;
        }
        out[k] = slot;
    }
    __shared__ int s_n[4];
    const unsigned long long bal = __ballot(had && slot == 0);
    if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) lost[blockIdx.x] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
}

#define SNAP_MAX 8
struct SegSnap {
    int ticket = -1, in_use = 0, flags = 0, translated = 0;
    unsigned int generation = 0;       // ifx::seq_generation when it was taken
    uint2* px = nullptr;               // [P] creation number, slot hint
    SnapHdr* hdr = nullptr;
    int* counts = nullptr;             // [2][blocks]: pixels with a surfel (snapshot), pixels that lost it (last translate)
    uint8_t* rgb = nullptr;            // [P][3], [P]: the raw frame, allocated by the first snapshot of this slot that keeps one
    uint16_t* depth = nullptr;
    hipEvent_t ev = nullptr;           // behind the snapshot on the frame's stream
};
struct SegSnapSet { SegSnap s[SNAP_MAX]; };
static SegSnap* snap_find(ifx* h, int ticket, bool released_too = false)
{
    SegSnapSet* set = (SegSnapSet*)h->seg_snaps;
    if (!set || ticket < 0) return nullptr;
    for (SegSnap& q : set->s) if (q.ticket == ticket && (q.in_use || released_too)) return &q;
    return nullptr;
}
static int snap_in_use(const ifx* h)
{
    const SegSnapSet* set = (const SegSnapSet*)h->seg_snaps;
    int n = 0;
    if (set) for (const SegSnap& q : set->s) n += q.in_use;
    return n;
}
void ifx_free_snapshots(ifx* h)
{
    SegSnapSet* set = (SegSnapSet*)h->seg_snaps;
    if (set) {
        for (SegSnap& q : set->s) { hipFree(q.px); hipFree(q.hdr); hipFree(q.counts); hipFree(q.rgb); hipFree(q.depth); if (q.ev) hipEventDestroy(q.ev); }
        delete set;
    }
    h->seg_snaps = nullptr;
    hipFree(h->d_snap_ids); h->d_snap_ids = nullptr;
    for (FrameSlot& f : h->slot) if (f.snap_read) { hipEventDestroy(f.snap_read); f.snap_read = nullptr; }
}
// what every snapshot entry refuses alike (nothing enqueued, the handle stays usable)
static int snap_refuse_mode(ifx* h, const char* who)
{
    if (h->own || h->shard_n > 1) { h->err = std::string(who) + ": not offered on a sharded map"; return IFX_E_STATE; }
    if (h->cams.size() > 1) { h->err = std::string(who) + ": not offered with more than one camera context"; return IFX_E_STATE; }
    return IFX_OK;
}
// what the sharded map's snapshot and deferred entries refuse by mode (nothing enqueued, the handle stays usable)
static int osnap_refuse_mode(ifx* h, const char* who)
{
    if (!h->own) { h->err = std::string(who) + ": the handle was not created for a sharded map"; return IFX_E_STATE; }
    if (h->cams.size() > 1) { h->err = std::string(who) + ": not offered with more than one camera context"; return IFX_E_STATE; }
    if (h->oseg_state) { h->err = std::string(who) + ": a segmentation call is already in flight"; return IFX_E_STATE; }
    if (h->tick < 2) { h->err = std::string(who) + ": no frame has been processed yet"; return IFX_E_STATE; }
    return IFX_OK;
}
// the one body of ifx_segmentation_snapshot and ifx_owner_segmentation_snapshot (own), behind the refusal by mode
static int snap_take(ifx* h, const char* who, bool own, int flags)
{
    int r;
    if (h->tick < 2) { h->err = std::string(who) + ": no frame has been processed yet"; return IFX_E_STATE; }
    if (snap_in_use(h) >= h->opt_seg_snapshots) { h->err = std::string(who) + ": every ticket is in use (option seg_snapshots)"; return IFX_E_CAPACITY; }
    if (!h->seg_snaps) h->seg_snaps = new SegSnapSet();
    SegSnapSet* set = (SegSnapSet*)h->seg_snaps;
    SegSnap* q = nullptr;   // the free slot released longest ago: a released ticket's figures stay readable (ifx_segmentation_snapshot_stats) until its buffers are taken again
    for (SegSnap& c_ : set->s) if (!c_.in_use && (!q || c_.ticket < q->ticket)) q = &c_;
    if (!q) { h->err = std::string(who) + ": every ticket is in use"; return IFX_E_CAPACITY; }
    const int P = h->P, nb = cdiv(P, 256);
    // (each buffer on its own: an allocation that fails leaves the slot free and the ones before it in place for the next attempt)
    if (!q->px) HIPCHK(h, hipMalloc((void**)&q->px, (size_t)P * sizeof(uint2)));
    if (!q->hdr) HIPCHK(h, hipMalloc((void**)&q->hdr, sizeof(SnapHdr)));
    if (!q->counts) HIPCHK(h, hipMalloc((void**)&q->counts, (size_t)2 * nb * sizeof(int)));
    if (!q->ev) HIPCHK(h, hipEventCreateWithFlags(&q->ev, hipEventDisableTiming));
    if ((flags & 2) && !q->rgb) HIPCHK(h, hipMalloc((void**)&q->rgb, (size_t)P * 3));
    if ((flags & 2) && !q->depth) HIPCHK(h, hipMalloc((void**)&q->depth, (size_t)P * 2));
    // the whole id image, whatever id_rule / lazy_ids drew (a sharded map under own_lazy_ids: completed in place by the library's communicator, collectively; a
    // caller-driven transport is told to complete it first)
    if ((r = ifx_ids_ensure(h))) { if (own) h->err = std::string(who) + ": " + h->err; return r; }
    if (own) LAUNCH(h, "seg_snapshot_own", dim3(nb), dim3(256), k_seg_snapshot<1>, (const DevState*)h->d_state, (const int32_t*)h->ids_after, (const uint32_t*)h->seq, P, h->tick, q->px, q->hdr, q->counts);
    else LAUNCH(h, "seg_snapshot", dim3(nb), dim3(256), k_seg_snapshot<0>, (const DevState*)h->d_state, (const int32_t*)h->ids_after, (const uint32_t*)h->seq, P, h->tick, q->px, q->hdr, q->counts);
    if (flags & 2) {
        // the raw frame, device to device, out of its frame slot; the side stream reuses the slot two frames on and waits for the FRAME that used it only
        // (FrameSlot::released), so it is told about this reader too (enqueue_frame_side)
        FrameSlot& f = h->slot[(size_t)h->last_frame_slot];
        HIPCHK(h, hipMemcpyAsync(q->rgb, f.rgb, (size_t)P * 3, hipMemcpyDeviceToDevice, h->cur));
        HIPCHK(h, hipMemcpyAsync(q->depth, f.depth_raw, (size_t)P * 2, hipMemcpyDeviceToDevice, h->cur));
        if (!f.snap_read) HIPCHK(h, hipEventCreateWithFlags(&f.snap_read, hipEventDisableTiming));
        HIPCHK(h, hipEventRecord(f.snap_read, h->cur));
        f.snap_pending = 1;
    }
    HIPCHK(h, hipEventRecord(q->ev, h->cur));
    q->ticket = h->snap_next_ticket++; q->in_use = 1; q->flags = flags; q->translated = 0; q->generation = h->seq_generation;
    return q->ticket;
}
extern "C" int ifx_segmentation_snapshot(ifx_t* h, int flags)
{
    if (!h) return IFX_E_INVALID;
    if (flags & ~2) { h->err = "ifx_segmentation_snapshot: unknown flags (bit 1: keep the frame for the superpixels)"; return IFX_E_INVALID; }
    const int r = snap_refuse_mode(h, "ifx_segmentation_snapshot");
    return r ? r : snap_take(h, "ifx_segmentation_snapshot", false, flags);
}
extern "C" int ifx_owner_segmentation_snapshot(ifx_t* h, int flags)
{
    if (!h) return IFX_E_INVALID;
    const int r = osnap_refuse_mode(h, "ifx_owner_segmentation_snapshot");
    if (!r && (flags & ~2)) { h->err = "ifx_owner_segmentation_snapshot: unknown flags (bit 1: keep the frame for the superpixels)"; return IFX_E_INVALID; }
    return r ? r : snap_take(h, "ifx_owner_segmentation_snapshot", true, flags);
}
extern "C" int ifx_segmentation_snapshot_release(ifx_t* h, int ticket)
{
    if (!h) return IFX_E_INVALID;
    SegSnap* q = snap_find(h, ticket);
    if (!q) { h->err = "ifx_segmentation_snapshot_release: unknown or released ticket"; return IFX_E_INVALID; }
    q->in_use = 0;   // (buffers stay: whoever takes the slot next enqueues behind whatever still reads them, on the same stream or behind a synchronous call)
    return IFX_OK;
}
extern "C" int ifx_segmentation_snapshot_stats(ifx_t* h, int ticket, int32_t* out4)
{
    if (!h || !out4) return IFX_E_INVALID;
    SegSnap* q = snap_find(h, ticket, true);
    if (!q) { h->err = "ifx_segmentation_snapshot_stats: unknown ticket"; return IFX_E_INVALID; }
    const int nb = cdiv(h->P, 256);
    std::vector<int> c((size_t)2 * nb);
    SnapHdr hd;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(&hd, q->hdr, sizeof(hd), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(c.data(), q->counts, c.size() * sizeof(int), hipMemcpyDeviceToHost));
    int have = 0, lost = 0;
    for (int b = 0; b < nb; b++) { have += c[b]; lost += c[nb + b]; }
    out4[0] = hd.tick; out4[1] = have; out4[2] = q->translated ? lost : -1; out4[3] = snap_in_use(h);
    return IFX_OK;
}
// the view of a deferred call: behind the snapshot, the pinned image re-addressed in today's slots (a buffer of its own: ifx::ids_after is not touched)
static int seg_view_snapshot(ifx* h, SegSnap* q, SegView* v)
{
    const int P = h->P, nb = cdiv(P, 256);
    if (!h->d_snap_ids) HIPCHK(h, hipMalloc((void**)&h->d_snap_ids, (size_t)P * 4));
    HIPCHK(h, hipStreamWaitEvent(h->cur, q->ev, 0));   // (the call may run on the third stream)
    if (h->own) {   // this rank's slots, coded slot + 1; "surfel 0": the word behind the last frame's [key_splat | key_ids], which that frame's id resolve used
        LAUNCH(h, "seg_translate_own", dim3(nb), dim3(256), k_seg_translate<1>, (const DevState*)h->d_state, (const uint2*)q->px, (const uint32_t*)h->seq, (const float2*)h->tm, P, h->d_snap_ids,
               q->counts + nb, (h->opt_own_first_live && h->gfl_splat) ? (const unsigned int*)h->gfl_splat : (const unsigned int*)nullptr);
        v->im.seq = nullptr; v->im.own_n = IDMAP_SLOTS;
    } else
        LAUNCH(h, "seg_translate", dim3(nb), dim3(256), k_seg_translate<0>, (const DevState*)h->d_state, (const uint2*)q->px, (const uint32_t*)h->seq, (const float2*)h->tm, P, h->d_snap_ids,
               q->counts + nb, (const unsigned int*)nullptr);
    q->translated = 1;
    v->ids = h->d_snap_ids; v->cam = q->hdr->pose; v->d_rgb = q->rgb; v->d_depth = q->depth;
    if (!(q->flags & 2)) { v->d_rgb = nullptr; v->d_depth = nullptr; }
    return IFX_OK;
}
// the checks of the two deferred entries that need the ticket; *out: the snapshot
static int snap_for_call(ifx* h, const char* who, int ticket, int flags, SegSnap** out)
{
    int r = snap_refuse_mode(h, who);
    if (r) return r;
    SegSnap* q = snap_find(h, ticket);
    if (!q) { h->err = std::string(who) + ": unknown or released ticket"; return IFX_E_INVALID; }
    if ((flags & 2) && !(q->flags & 2)) { h->err = std::string(who) + ": superpixels need a ticket taken with the frame (ifx_segmentation_snapshot flags bit 1)"; return IFX_E_STATE; }
    if (q->generation != h->seq_generation) { h->err = std::string(who) + ": the map was uploaded since the ticket was taken (creation numbers renumbered)"; return IFX_E_STATE; }
    *out = q;
    return IFX_OK;
}
// the ticket of a deferred call on a sharded map: the refusal by mode, then what snap_for_call checks of the ticket
static int oseg_snap_for_call(ifx* h, const char* who, int ticket, int flags, SegSnap** out)
{
    int r = osnap_refuse_mode(h, who);
    if (r) return r;
    SegSnap* q = snap_find(h, ticket);
    if (!q) { h->err = std::string(who) + ": unknown or released ticket"; return IFX_E_INVALID; }
    if ((flags & 2) && !(q->flags & 2)) { h->err = std::string(who) + ": superpixels need a ticket taken with the frame (ifx_owner_segmentation_snapshot flags bit 1)"; return IFX_E_STATE; }
    if (q->generation != h->seq_generation) { h->err = std::string(who) + ": the map was uploaded since the ticket was taken (creation numbers renumbered)"; return IFX_E_STATE; }
    *out = q;
    return IFX_OK;
}
// Deferred segmentation on a spatially sharded map: ifx_owner_segmentation_begin[_device] on a ticket of ifx_owner_segmentation_snapshot.  Every rank re-addresses
// the pinned image in its own slots (k_seg_translate<1>: no exchange -- the image is replicated, ownership never changes), the call body reads slots, and the call
// goes on through ifx_owner_segmentation_resume and the same exchange points (never the id image's: the ticket pinned a whole one).  Out of scope here: the ROI,
// detections and unmolded forms (same record, same body), camera contexts, and moving the ordinary sharded call onto a translated image.
extern "C" int ifx_owner_segmentation_begin_deferred(ifx_t* h, int ticket, const uint8_t* masks_in, const int32_t* class_ids, int nm, int frame, int flags)
{
    const char* who = "ifx_owner_segmentation_begin_deferred";
    if (!h) return IFX_E_INVALID;
    if (h->own && (flags & 1)) { h->err = std::string(who) + ": kNN smoothing is not offered on a sharded map's begin / resume (it needs every rank's positions)"; return IFX_E_INVALID; }
    if (nm < 0 || nm > 256 || (nm > 0 && (!masks_in || !class_ids))) { h->err = std::string(who) + ": n must be 0 .. 256, with masks and class ids"; return IFX_E_INVALID; }
    SegSnap* snap = nullptr;
    const int r = oseg_snap_for_call(h, who, ticket, flags, &snap);
    return r ? r : oseg_begin_host(h, snap, ticket, nullptr, nullptr, masks_in, class_ids, nm, frame, flags);
}
extern "C" int ifx_owner_segmentation_begin_deferred_device(ifx_t* h, int ticket, int root, int max_n, const void* d_masks, int mask_format, float threshold, const int32_t* d_class_ids,
                                                            int n, int frame, int flags, void* stream)
{
    return oseg_entry(h, "ifx_owner_segmentation_begin_deferred_device", root, max_n, nullptr, nullptr, src_image(d_masks, mask_format, threshold, d_class_ids, n), threshold, frame, flags,
                      stream, &ticket);
}

// what ifx_detector_input (ifx_detector.hip) reads: the frame a ticket kept (ticket >= 0: *ev is the event behind the snapshot, the ticket stays in use) or the
// resident frame slot (*slot, whose next copy-in the caller holds off as the snapshot above does).  Refuses as the snapshot entries do.
int ifx_frame_for_reader(ifx* h, const char* who, int ticket, const uint8_t** rgb, hipEvent_t* ev, FrameSlot** slot)
{
    int r = snap_refuse_mode(h, who);
    if (r) return r;
    *ev = nullptr; *slot = nullptr;
    if (ticket >= 0) {
        SegSnap* q = snap_find(h, ticket);
        if (!q) { h->err = std::string(who) + ": unknown or released ticket"; return IFX_E_INVALID; }
        if (!(q->flags & 2)) { h->err = std::string(who) + ": the ticket was taken without its frame (ifx_segmentation_snapshot flags bit 1)"; return IFX_E_STATE; }
        if (q->generation != h->seq_generation) { h->err = std::string(who) + ": the map was uploaded since the ticket was taken"; return IFX_E_STATE; }
        *rgb = q->rgb; *ev = q->ev;
        return IFX_OK;
    }
    if (h->tick < 2) { h->err = std::string(who) + ": no frame has been processed yet"; return IFX_E_STATE; }
    *slot = &h->slot[(size_t)h->last_frame_slot];
    *rgb = (*slot)->rgb;
    return IFX_OK;
}

// The tail of the device schedule: registration, the votes in mask order, the gated label scan, the control block and the verdict bytes read back into the pinned
// block (SegCtl, then nm bytes), and the wait for them.  gate / meta / skip: the flood fill's counters for the first pass (k_seg_register), nulls for the pass after
// the host finished an incomplete fill.  enqueued(): called between the last enqueue and the wait (IFX_SEG_TRACE).  Returns 1 when the scan enqueued was the full one.
template <typename F>
static int seg_device_tail(ifx* h, const SegView& v, int nm, const int* gate, const int* meta, const uint8_t* skip, bool default_done, F&& enqueued)
{
    const int P = h->P;
    SegCtl* hc = (SegCtl*)h->h_segctl;
    SegCtl* dc = (SegCtl*)h->d_segctl;
    LAUNCH(h, "seg_register", dim3(1), dim3(64), k_seg_register, dc, h->d_unavail, gate, meta, skip);
    for (int m_ = 0; m_ < nm; m_++)   // (mask order is part of the result: see k_vote_update_mask)
        LAUNCH(h, "vote_update", dim3(cdiv(P, 256)), dim3(256), k_vote_update_mask, h->d_state, v.ids, (const uint8_t*)h->d_masks, P, h->cap, (const SegCtl*)dc, nm, h->votes, ifx_idmap(h), m_);
    // the scan kernels look at the control block themselves: when the call has to be finished by the host (fill incomplete / table full) they return at once and
    // the ONE scan of the call runs behind the host-driven tail, after every mask and the eviction -- colours are assigned once, so an early scan would be visible
    const int full_scan = seg_label_scan(h, v, (const int*)dc, default_done);
    uint8_t* h_un = (uint8_t*)h->h_segctl + sizeof(SegCtl);
    HIPCHK(h, hipMemcpyAsync(hc, dc, sizeof(SegCtl), hipMemcpyDeviceToHost, h->cur));
    HIPCHK(h, hipMemcpyAsync(h_un, h->d_unavail, nm, hipMemcpyDeviceToHost, h->cur));
    enqueued();
    HIPCHK(h, hipStreamSynchronize(h->cur));
    return full_scan;
}

static int process_segmentation_device(ifx_t* h, const uint8_t* rgb, const uint16_t* depth, const uint8_t* masks_in, const int32_t* class_ids, const DevMasks* dm, int nm, int frame, int flags,
                                       SegSnap* snap)
{
    static const bool trace = getenv("IFX_SEG_TRACE") != nullptr;   // diagnostic: where the host is inside a call (us since entry, to stderr)
    const auto t_in = std::chrono::steady_clock::now();
    auto us = [&]() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_in).count(); };
    double t_res = 0, t_ids = 0, t_stage = 0, t_enq = 0, t_sync = 0;
    if (flags & 1) ifx_vlist_reap(h);
    // the frame's result, not the stream: the next frame's tracker may already be queued behind it, and nothing here has to wait for that
    int n = 0;
    if (h->seg_counts_valid && h->ev_result) { HIPCHK(h, hipEventSynchronize(h->ev_result)); n = h->h_result->count; }
    else { HIPCHK(h, hipStreamSynchronize(h->cur)); HIPCHK(h, hipMemcpy(&n, &h->d_state->count, sizeof(int), hipMemcpyDeviceToHost)); }
    h->seg_counts_valid = 0;
    h->seg_last_nm = 0;
    if (nm == 0 || n == 0) return IFX_OK;
    t_res = us();
    if (!snap) ifx_ids_ensure(h);   // the call reads the id image under every mask pixel: the whole image, if the frame rendered only the sampled lattice (a snapshot pinned the whole one)
    t_ids = us();
    const int P = h->P;
    const size_t mbytes = (size_t)nm * P;
    int r = ifx_ensure_masks(h, mbytes);
    if (r) return r;
    if ((r = seg_ensure_ctl(h, dm ? 0 : mbytes))) return r;   // (device masks: no staging)
    SegCtl* hc = (SegCtl*)h->h_segctl;
    PoolEvent ea(h);   // (given back on every return but the last, where stage_pending takes it)
    hipEventRecord(ea.ev, h->cur);
    SegView v = seg_view_current(h);
    if (snap && (r = seg_view_snapshot(h, snap, &v))) return r;   // (deferred call: the pinned id image re-addressed in today's slots, the pinned pose and frame)
    if (flags & 2) {   // superpixels and their merge: on the queue before the masks are even copied (they need the frame only)
        if ((r = v.d_rgb ? ifx_superpixel_begin_device(h, v.d_rgb, v.d_depth) : ifx_superpixel_begin(h, rgb, depth))) return r;
    }
    // what needs the map and the id image but not the masks -- the boxes of the projected instances (the twelve vote float4 under every pixel: the heavy half of
    // getProjectInstanceList / computeProjectBoundingBox) and the model depth under every pixel -- runs while the host copies the masks into pinned memory
    LAUNCH(h, "init_bbox", dim3(cdiv((NI + nm) * 4, 256)), dim3(256), k_init_bbox, h->d_bbox, NI + nm, h->w, h->h);
    const bool mask_rule = h->opt_compare_map == 2;   // (the mask rule: the same pass also stores the presence image, so the votes are gathered once)
    if (mask_rule && (r = cmp_ensure(h))) return r;
    if (mask_rule)
        LAUNCH(h, "project_bbox_pres", dim3(cdiv(h->w, 32), cdiv(h->h, PB_ROWS)), dim3(32, PB_ROWS), k_project_bbox<3>, h->d_state, v.ids, (const float4*)h->votes, h->cap, (const uint8_t*)nullptr,
               nm, h->w, h->h, h->d_bbox, ifx_idmap(h), (const float4*)h->pc, h->d_pdm, v.cam, (uint4*)h->d_pres);
    else
        LAUNCH(h, "project_bbox_inst", dim3(cdiv(h->w, 32), cdiv(h->h, PB_ROWS)), dim3(32, PB_ROWS), k_project_bbox<1>, h->d_state, v.ids, (const float4*)h->votes, h->cap, (const uint8_t*)nullptr,
               nm, h->w, h->h, h->d_bbox, ifx_idmap(h), (const float4*)h->pc, h->d_pdm, v.cam);
    const bool default_early = !h->labels_stale_all;
    if (default_early) LAUNCH(h, "colour_default", dim3(2048), dim3(256), k_colour_default, h->d_state, (const float2*)h->tm, (float2*)h->col, h->labels, (const int*)nullptr);
    if (flags & 2) { if ((r = ifx_superpixel_filter_prepare(h, nm))) return r; }
    if (!dm) memcpy(h->h_masks_stage, masks_in, mbytes);
    hc->ff_incomplete = 0; hc->evict_at = -1; hc->nm = nm; hc->pad = 0;
    for (int i = 0; i < NI; i++) hc->inst_class[i] = h->inst_class[i];
    for (int m = 0; m < 256; m++) { hc->cls[m] = m < nm && !dm ? class_ids[m] : -1; hc->best[m] = -1; hc->target[m] = -1; }   // (device masks: k_mask_order writes the class ids)
    SegCtl* dc = (SegCtl*)h->d_segctl;
    if (dm) {   // the caller's device masks: sorted, binarised and cleaned on the device, the class ids in sorted order into the control block
        HIPCHK(h, hipMemcpyAsync(h->d_segctl, hc, sizeof(SegCtl), hipMemcpyHostToDevice, h->cur));
        if ((r = seg_ingest_device(h, dm, nm, dc->cls, h->d_unavail))) return r;
        t_stage = us();
    } else {
        t_stage = us();
        HIPCHK(h, hipMemcpyAsync(h->d_masks_ori, h->h_masks_stage, mbytes, hipMemcpyHostToDevice, h->cur));   // pinned: a true asynchronous copy
        HIPCHK(h, hipMemcpyAsync(h->d_segctl, hc, sizeof(SegCtl), hipMemcpyHostToDevice, h->cur));
        LAUNCH(h, "mask_clean_overlap", dim3(cdiv(P, 256)), dim3(256), k_mask_clean_overlap_from, (const uint8_t*)h->d_masks_ori, h->d_masks, nm, P, h->d_unavail);
    }
    if (flags & 2) {
        r = ifx_superpixel_filter(h, nm, true);
        if (r) return r;
    }
    LAUNCH(h, "project_bbox_mask", dim3(cdiv(h->w, 32), cdiv(h->h, PB_ROWS)), dim3(32, PB_ROWS), k_project_bbox<2>, h->d_state, v.ids, (const float4*)h->votes, h->cap, h->d_masks, nm, h->w, h->h,
           h->d_bbox, ifx_idmap(h));
    if (mask_rule) {   // (the mask-box launch stays: the degenerate-box test reads it)
        if ((r = cmp_launch_count(h, nm))) return r;
        LAUNCH(h, "seg_compare_iou", dim3(1), dim3(256), k_seg_compare_iou, dc, (const int*)h->d_bbox, h->d_unavail, (const int*)h->d_cmp_tab);
    } else {
        LAUNCH(h, "seg_compare", dim3(1), dim3(256), k_seg_compare, dc, (const int*)h->d_bbox, h->d_unavail);
    }
    const int rounds = h->opt_ff_rounds > 0 ? h->opt_ff_rounds : 4;   // (after the union-find start the first relaxation normally finds the fixpoint: the rest are spares for one-way edges)
    r = mask_geometric_filter_device(h, h->d_pdm, h->d_masks, h->d_masks_ori, nm, h->d_unavail, rounds, false, true);
    if (r) return r;
    const FFArgs fa = ff_args(h, h->d_pdm, h->d_masks, h->d_masks_ori, nm);
    const int* gate = fa.changed + (std::min(rounds, FF_SLOTS) - 1);
    const int full_scan = seg_device_tail(h, v, nm, gate, (const int*)fa.meta, fa.skip, default_early, [&] { t_enq = us(); });
    if (full_scan < 0) return full_scan;
    const uint8_t* h_un = (const uint8_t*)h->h_segctl + sizeof(SegCtl);
    t_sync = us();
    if (trace) fprintf(stderr, "seg call: result %.0f  ids %.0f  staged %.0f  enqueued %.0f  synced %.0f us (nm %d)\n", t_res, t_ids, t_stage, t_enq, t_sync, nm);
    if ((hc->ff_incomplete || hc->evict_at >= 0) && full_scan) h->labels_stale_all = 1;   // the gated scan did not run: whatever made it a full one still holds
    if (hc->ff_incomplete) {   // the fill needs more relaxations than the schedule holds: finish it with the host looking, then the tail again (nothing was voted yet)
        r = mask_geometric_filter_device(h, h->d_pdm, h->d_masks, h->d_masks_ori, nm, h->d_unavail, 0, true);
        if (r) return r;
        const int full2 = seg_device_tail(h, v, nm, nullptr, nullptr, nullptr, false, [] {});   // (gated again: the table may turn out full at some mask)
        if (full2 < 0) return full2;
        if (hc->evict_at >= 0 && full2) h->labels_stale_all = 1;
    }
    for (int i = 0; i < NI; i++) h->inst_class[i] = hc->inst_class[i];
    for (int m = 0; m < nm; m++) { h->seg_last_best[m] = hc->best[m]; h->seg_last_target[m] = hc->target[m]; }   // (ifx_segmentation_matches; the host-driven tail overwrites its masks)
    if (hc->evict_at >= 0) {   // the table is full at this mask: the reference evicts its twenty weakest instances and goes on -- from here the host-driven loop
        std::vector<uint8_t> unavailable(h_un, h_un + nm);
        std::vector<int> cmp((size_t)nm * NI, 0), bbox;
        for (int m = 0; m < nm; m++) if (hc->best[m] > 0) cmp[hc->best[m] + m * NI] = 1;
        r = seg_host_mask_loop(h, v, nm, dm ? hc->cls : class_ids, hc->evict_at, cmp, unavailable, bbox);   // (device masks: the class ids in sorted order, as read back)
        if (r) return r;
        seg_label_scan(h, v);
    }
    if (flags & 1) { r = ifx_knn_vote(h, nullptr); if (r) return r; }
    ifx_stage_span_end(h, 2, ea);
    HIPCHK(h, hipStreamSynchronize(h->cur));
    h->seg_last_nm = nm;
    return IFX_OK;
}

// The mask rule as a stage (host masks, used as given): the tables and the decision under the current id image, votes and instance table.  Map, votes, table
// and what ifx_segmentation_matches reports stay as they are; the call's scratch -- d_masks, d_bbox, the presence image and the tables -- is overwritten, as by the
// sibling stages, and the votes are gathered twice (the box pass for the degenerate-box test, then the presence pass with its boxes into the sink).
extern "C" int ifx_mask_compare_map(ifx_t* h, const uint8_t* masks, const int32_t* class_ids, int n, const uint8_t* unavailable, int32_t* out_I, int32_t* out_U, int32_t* out_best)
{
    if (!h) return IFX_E_INVALID;
    if (n < 0 || n > 256) { h->err = "ifx_mask_compare_map: n must be 0 .. 256"; return IFX_E_INVALID; }
    if (n > 0 && (!masks || !class_ids)) { h->err = "ifx_mask_compare_map: null masks or class ids"; return IFX_E_INVALID; }
    if (h->own || h->shard_n > 1) { h->err = "ifx_mask_compare_map: not on a sharded map"; return IFX_E_STATE; }
    if (n == 0) return IFX_OK;
    int r = ifx_ids_ensure(h);
    if (r) return r;
    const size_t bytes = (size_t)n * h->P;
    if ((r = ifx_ensure_masks(h, bytes))) return r;
    HIPCHK(h, hipMemcpyAsync(h->d_masks, masks, bytes, hipMemcpyHostToDevice, h->cur));
    const SegView v = seg_view_current(h);
    std::vector<int> bbox, tab, cmp((size_t)n * NI, 0);
    if ((r = run_bboxes(h, v, n, bbox)) || (r = cmp_tables_host(h, v.ids, n, tab))) return r;
    std::vector<uint8_t> un(n, 0);
    if (unavailable) un.assign(unavailable, unavailable + n);
    compare_map_iou(h, tab.data(), &bbox[NI * 4], class_ids, n, un, cmp);
    for (int m = 0; m < n; m++) {
        if (out_best) out_best[m] = -1;
        for (int q = 0; q < NI; q++) {
            const bool same = h->inst_class[q] != -1 && h->inst_class[q] == class_ids[m];   // pairs whose classes differ stay 0, as the reference leaves them
            const int I = tab[CM_I + m * NI + q];
            if (out_I) out_I[m * NI + q] = same ? I : 0;
            if (out_U) out_U[m * NI + q] = same ? tab[CM_AM + m] + tab[CM_AI + q] - I : 0;
            if (out_best && cmp[q + m * NI] == 1) out_best[m] = q;
        }
    }
    return IFX_OK;
}

extern "C" int ifx_segmentation_matches(ifx_t* h, int32_t* out_best, int32_t* out_target, int max_n)
{
    if (!h || max_n < 0) return IFX_E_INVALID;
    for (int m = 0; m < h->seg_last_nm && m < max_n; m++) {
        if (out_best) out_best[m] = h->seg_last_best[m];
        if (out_target) out_target[m] = h->seg_last_target[m];
    }
    return h->seg_last_nm;
}

__global__ void k_gather_labels(const DevState* __restrict__ st, const float2* __restrict__ tm, const int32_t* __restrict__ labels, const int* __restrict__ rank, int cap,
                                int32_t* __restrict__ out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap || i >= st->count) return;
    if (tm[i].y > DEAD_TIME) out[rank[i]] = labels[i];
}
__global__ void k_alive_flags2(const DevState* __restrict__ st, const float2* __restrict__ tm, int* __restrict__ flags, int cap)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap) return;
    flags[i] = (i < st->count && tm[i].y > DEAD_TIME) ? 1 : 0;
}

extern "C" int ifx_labels(ifx_t* h, int32_t* out, int max_n)
{
    if (h) ifx_vlist_reap(h);   // whole-map consumer: nothing outside the cached view list may outlive the age rule (ifx_map.hip "View list")
    if (!h || !out) return IFX_E_INVALID;
    // labels of the live surfels in map order: rank = exclusive scan of the alive flags
    LAUNCH(h, "alive_flags", dim3(cdiv(h->cap, 256)), dim3(256), k_alive_flags2, h->d_state, (const float2*)h->tm, h->scan_flags, h->cap);
    ifx_scan_exclusive(h, h->scan_flags, h->cap, h->scan_out, &h->d_state->seg_counts[1]);
    LAUNCH(h, "gather_labels", dim3(cdiv(h->cap, 256)), dim3(256), k_gather_labels, h->d_state, (const float2*)h->tm, h->labels, h->scan_out, h->cap, h->labels2);
    DevState hs;
    HIPCHK(h, hipStreamSynchronize(h->cur));
    HIPCHK(h, hipMemcpy(&hs, h->d_state, sizeof(hs), hipMemcpyDeviceToHost));
    int n = std::min(hs.seg_counts[1], max_n);
    HIPCHK(h, hipMemcpy(out, h->labels2, (size_t)n * 4, hipMemcpyDeviceToHost));
    return n;
}

// ---- instance ground truth (ScanNet evaluation of the reference)
// instanceGT argument of ElasticFusion::processFrame (EF/ElasticFusion.cpp:273-291): surfels created from now on remember the id under their pixel
extern "C" int ifx_set_instance_gt(ifx_t* h, const uint8_t* gt_hw)
{
    if (!h) return IFX_E_INVALID;
    if (!gt_hw) { h->inst_gt_on = 0; return IFX_OK; }
    if (!h->d_inst_gt) HIPCHK(h, hipMalloc(&h->d_inst_gt, (size_t)h->P));
    HIPCHK(h, hipMemcpyAsync(h->d_inst_gt, gt_hw, (size_t)h->P, hipMemcpyHostToDevice, h->cur));
    HIPCHK(h, hipStreamSynchronize(h->cur));   // gt_hw is the caller's
    h->inst_gt_on = 1;
    ifx_drop_tracked(h);
    return IFX_OK;
}
// computePrecisionAndRecallKernel, IF/Core/InstanceFusionCuda.cu:2085-2114
__global__ void k_precision_recall(const DevState* __restrict__ st, const float2* __restrict__ col, const float2* __restrict__ tm, const float4* __restrict__ ic,
                                   const float* __restrict__ inst_color, int* __restrict__ inst_num, int* __restrict__ gt_num, int* __restrict__ inst_gt_map)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= st->count || !(tm[s].y > -1.0e8f)) return;   // tombstones are not part of the map
    const float cc = col[s].y;
    int inst = -1;
    for (int i = 0; i < IFX_NUM_INSTANCES; i++) if (cc == inst_color[i]) { inst = i; break; }
    if (inst >= 0) atomicAdd(&inst_num[inst], 1);
    const int gt = (int)ic[s].w;
    if (gt >= 0 && gt < 256) atomicAdd(&gt_num[gt], 1);
    if (inst >= 0 && gt >= 0 && gt < 256) atomicAdd(&inst_gt_map[gt * IFX_NUM_INSTANCES + inst], 1);
}
extern "C" int ifx_precision_recall(ifx_t* h, int32_t* inst_num96, int32_t* gt_num256, int32_t* inst_gt_map)
{
    if (h) ifx_vlist_reap(h);   // whole-map consumer: nothing outside the cached view list may outlive the age rule (ifx_map.hip "View list")
    if (!h || !inst_num96 || !gt_num256 || !inst_gt_map) return IFX_E_INVALID;
    const size_t n = IFX_NUM_INSTANCES + 256 + 256 * IFX_NUM_INSTANCES;
    int* d = nullptr;
    HIPCHK(h, hipMalloc(&d, n * 4));
    hipMemsetAsync(d, 0, n * 4, h->cur);
    hipMemcpyAsync(h->d_inst_color, h->inst_color, sizeof(h->inst_color), hipMemcpyHostToDevice, h->cur);
    LAUNCH(h, "precision_recall", dim3(cdiv(h->cap, 256)), dim3(256), k_precision_recall, (const DevState*)h->d_state, (const float2*)h->col, (const float2*)h->tm,
           (const float4*)h->ic, (const float*)h->d_inst_color, d, d + IFX_NUM_INSTANCES, d + IFX_NUM_INSTANCES + 256);
    std::vector<int32_t> host(n);
    hipError_t e = hipMemcpyAsync(host.data(), d, n * 4, hipMemcpyDeviceToHost, h->cur);
    if (e == hipSuccess) e = hipStreamSynchronize(h->cur);
    hipFree(d);
    if (e != hipSuccess) { h->err = hipGetErrorString(e); return IFX_E_HIP; }
    memcpy(inst_num96, host.data(), IFX_NUM_INSTANCES * 4);
    memcpy(gt_num256, host.data() + IFX_NUM_INSTANCES, 256 * 4);
    memcpy(inst_gt_map, host.data() + IFX_NUM_INSTANCES + 256, (size_t)256 * IFX_NUM_INSTANCES * 4);
    return IFX_OK;
}

// renderProjectFrameKernel, IF/Core/InstanceFusionCuda.cu:1432-1498 (InstanceFusion::renderProjectMap without the boxes drawn on the host)
__global__ void k_render_project(const DevState* __restrict__ st, const int32_t* __restrict__ ids, const float2* __restrict__ col, int P, float4* __restrict__ out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P) return;
    const int id = ids[k];
    float4 c = make_float4(0.f, 0.f, 0.f, 1.f);
    if (id > 0 && id < st->count) {
        const int v = (int)col[id].y;
        c.x = (float)((v >> 16) & 0xFF) / 255.0f; c.y = (float)((v >> 8) & 0xFF) / 255.0f; c.z = (float)(v & 0xFF) / 255.0f;
    }
    out[k] = c;
}
extern "C" int ifx_render_project_map(ifx_t* h, float* out_rgba, float* d_out_rgba)
{
    if (!h || (!out_rgba && !d_out_rgba)) return IFX_E_INVALID;
    ifx_ids_ensure(h);
    float* dst = d_out_rgba;
    if (!dst) {
        if (!h->d_project) HIPCHK(h, hipMalloc(&h->d_project, (size_t)h->P * 16));
        dst = h->d_project;
    }
    LAUNCH(h, "render_project", dim3(cdiv(h->P, 256)), dim3(256), k_render_project, (const DevState*)h->d_state, (const int32_t*)h->ids_after, (const float2*)h->col, h->P, (float4*)dst);
    if (out_rgba) {
        HIPCHK(h, hipMemcpyAsync(out_rgba, dst, (size_t)h->P * 16, hipMemcpyDeviceToHost, h->cur));
        HIPCHK(h, hipStreamSynchronize(h->cur));
    }
    return IFX_OK;
}

extern "C" int ifx_instance_table(ifx_t* h, int32_t* out96)
{
    if (!h || !out96) return IFX_E_INVALID;
    memcpy(out96, h->inst_class, sizeof(h->inst_class));
    return IFX_OK;
}

// getLoopClosureInstanceTable, IF/Core/InstanceTable.cpp:98-121
extern "C" int ifx_loop_closure_instance_table(ifx_t* h, int32_t* out)
{
    if (!h || !out) return IFX_E_INVALID;
    for (int i = 0; i < NI; i++) {
        int c = (int)h->inst_color[i];
        out[5 * i + 0] = (c >> 16) & 0xFF; out[5 * i + 1] = (c >> 8) & 0xFF; out[5 * i + 2] = c & 0xFF;
        out[5 * i + 3] = h->inst_class[i];
        out[5 * i + 4] = i;
    }
    return IFX_OK;
}

// =========================================================================== f-3: duplicate instances after a loop closure
// InstanceFusion::checkLoopClosure (IF/Core/InstanceTable.cpp:122-169): loopClosureCopyMatchInstanceKernel (IF/Core/InstanceFusionCuda.cu:1370-1427) per pair, then
// cleanInstanceTable / cleanInstanceTableMap -- written by the reference and switched off (IF/main.cpp:143).  Here the copy and the clean are ONE pass over the
// 192-byte records: a block stages MG_RECS (128) records in LDS with 16-byte loads (only the quarters the plan names), one thread per record walks
// the pairs in ascending `from` on the staged words -- the reference's order, pair by pair on the words as the pairs before left them, because the packing is lossy
// and a decode / encode per pair is not a decode / encode per word -- then the clears with k_clean_table's arithmetic, and the block writes back the quarters of
// which a word changed, 16 bytes each.  Staged stride 13 float4 (52 words): a 16-byte aligned stride is a multiple of 4 words, so the record-per-lane word reads
// of the middle phase meet on 32 / gcd(stride, 32) banks: 8 banks (4-way) at 52, 2 banks (16-way) at the natural 48.
#define MG_RECS 128            // records per block and pass (27 KB staged: five blocks of two waves per CU, each with its own loads in flight)
#define MG_BLOCKS 1280          // 256 CUs x 5 resident blocks: one round of blocks, so that no CU idles behind a second one
#define MG_STRIDE 13
struct MergePlan {
    int n_pairs, n_clear;
    uint32_t qneed, pad;         // bit q: quarter q of a record holds a source or a target word
    uint32_t pair[NI];           // ascending `from`: source word | source half << 6 | target word << 8 | target half << 14   (half 0: the high one, instance 2 * word)
    uint32_t clear[IFX_VF];      // word | mask << 6   (bit 0: the high half, bit 1: the low half)
    float from_color[NI];        // the table colours of the cleared slots (k_merge_recolour)
};
__global__ __launch_bounds__(MG_RECS) void k_merge_votes(const DevState* __restrict__ st, float4* __restrict__ votes, int cap, const MergePlan* __restrict__ plan)
{
    __shared__ float4 s_rec[MG_RECS * MG_STRIDE];
    __shared__ uint32_t s_pair[NI], s_clear[IFX_VF], s_chg[MG_RECS];
    const int tid = threadIdx.x;
    const int np = min(plan->n_pairs, NI), nc = min(plan->n_clear, IFX_VF);
    const uint32_t qneed = plan->qneed;
    if (tid < np) s_pair[tid] = plan->pair[tid];
    if (tid < nc) s_clear[tid] = plan->clear[tid];
    const int n = min(st->count, cap);
    float* const w = (float*)s_rec + tid * (MG_STRIDE * 4);
    for (int r0 = blockIdx.x * MG_RECS; r0 < n; r0 += gridDim.x * MG_RECS) {   // (uniform per block: the barriers below see whole blocks)
        const int nrec = min(MG_RECS, n - r0);
        float4* const g = votes + (size_t)r0 * 12;
        // consecutive lanes, consecutive 16 bytes; the twelve loads of a lane are issued together and waited for once (a lane that has nothing to fetch re-reads a
        // quarter of the block's first record, which exists: a load per branch was one memory latency after the other, twelve per pass)
        float4 v[12];
#pragma unroll
        for (int j = 0; j < 12; j++) {
            const int slot = tid + j * MG_RECS, rec = slot / 12, q = slot - rec * 12;
            const bool want = rec < nrec && ((qneed >> q) & 1u);
            v[j] = g[want ? slot : q];
        }
#pragma unroll
        for (int j = 0; j < 12; j++) {
            const int slot = tid + j * MG_RECS, rec = slot / 12, q = slot - rec * 12;
            if (rec < nrec && ((qneed >> q) & 1u)) s_rec[rec * MG_STRIDE + q] = v[j];
        }
        __syncthreads();
        uint32_t chg = 0;
        if (tid < nrec) {
            for (int p = 0; p < np; p++) {
                const uint32_t e = s_pair[p];
                int a, b;
                vote_decode(w[e & 63u], a, b);
                const int f = ((e >> 6) & 1u) ? b : a;
                if (f <= 0) continue;   // nothing to give -- and the -1 of a first-frame surfel is no count
                const int tw = (e >> 8) & 63u;
                const float old = w[tw];
                vote_decode(old, a, b);
                if ((e >> 14) & 1u) { b += f; if (b >= 65535) b = 65535; }
                else { a += f; if (a >= 65535) a = 65535; }
                const float nw = vote_encode(a, b);
                if (__float_as_uint(nw) != __float_as_uint(old)) { w[tw] = nw; chg |= 1u << (tw >> 2); }
            }
            for (int c = 0; c < nc; c++) {   // cleanInstanceTableMapKernel on the from-halves
                const uint32_t e = s_clear[c];
                const int cw = e & 63u;
                const float old = w[cw];
                int a, b;
                vote_decode(old, a, b);
                if ((e >> 6) & 1u) a = 0;
                if ((e >> 7) & 1u) b = 0;
                const float nw = vote_encode(a, b);
                if (__float_as_uint(nw) != __float_as_uint(old)) { w[cw] = nw; chg |= 1u << (cw >> 2); }
            }
        }
        s_chg[tid] = chg;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 12; j++) {
            const int slot = tid + j * MG_RECS, rec = slot / 12, q = slot - rec * 12;
            if (rec < nrec && ((s_chg[rec] >> q) & 1u)) g[slot] = s_rec[rec * MG_STRIDE + q];
        }
        __syncthreads();   // (the next pass stages over these records)
    }
}
// Colours are assigned once (k_count_colour): a live surfel that carries the table colour of a cleared slot takes the colour of the label the scan just gave it
__global__ __launch_bounds__(256) void k_merge_recolour(const DevState* __restrict__ st, int cap, const float2* __restrict__ tm, float2* __restrict__ col, const float* __restrict__ inst_color,
                                                        const int32_t* __restrict__ labels, const MergePlan* __restrict__ plan)
{
    __shared__ float s_from[NI], s_col[NI];
    const int np = min(plan->n_pairs, NI);
    for (int t = threadIdx.x; t < NI; t += blockDim.x) { s_col[t] = inst_color[t]; if (t < np) s_from[t] = plan->from_color[t]; }
    __syncthreads();
    const float defaultColor = 7434609;
    const int n = min(st->count, cap);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += blockDim.x * gridDim.x) {
        if (!(tm[i].y > DEAD_TIME)) continue;
        float2 c = col[i];
        bool hit = false;
        for (int k = 0; k < np; k++) hit = hit || c.y == s_from[k];
        if (!hit) continue;
        const int l = labels[i];
        c.y = (l >= 0 && l < NI) ? s_col[l] : defaultColor;
        col[i] = c;
    }
}
// the checks of ifx_merge_instances and the plan of its pass, on the host; 0 or the refusal's text
static const char* merge_plan_build(const int32_t* inst_class, const float* inst_color, const int32_t* pairs, int n, MergePlan* mp)
{
    int to_of[NI];
    bool is_to[NI];
    for (int i = 0; i < NI; i++) { to_of[i] = -1; is_to[i] = false; }
    for (int k = 0; k < n; k++) {
        const int f = pairs[2 * k], t = pairs[2 * k + 1];
        if (f < 0 || f >= NI || t < 0 || t >= NI) return "an instance id outside 0 .. 95";
        if (f == t) return "a pair merges an instance into itself";
        if (inst_class[f] == -1 || inst_class[t] == -1) return "a pair names an unused slot of the instance table";
        if (to_of[f] != -1) return "an instance is the source of two pairs";
        to_of[f] = t; is_to[t] = true;
    }
    for (int i = 0; i < NI; i++) if (to_of[i] != -1 && is_to[i]) return "a chain: an instance is the target of one pair and the source of another (resolve it to its root first)";
    memset(mp, 0, sizeof(*mp));
    uint32_t cmask[IFX_VF] = {};
    for (int f = 0; f < NI; f++) {   // ascending `from`
        if (to_of[f] == -1) continue;
        const int t = to_of[f];
        mp->pair[mp->n_pairs] = (uint32_t)(f >> 1) | (uint32_t)(f & 1) << 6 | (uint32_t)(t >> 1) << 8 | (uint32_t)(t & 1) << 14;
        mp->from_color[mp->n_pairs++] = inst_color[f];
        cmask[f >> 1] |= 1u << (f & 1);
        mp->qneed |= 1u << (f >> 3) | 1u << (t >> 3);   // (word / 4: the 16-byte quarter)
    }
    for (int w = 0; w < IFX_VF; w++) if (cmask[w]) mp->clear[mp->n_clear++] = (uint32_t)w | cmask[w] << 6;
    return nullptr;
}
extern "C" int ifx_merge_instances(ifx_t* h, const int32_t* pairs, int n)
{
    if (!h) return IFX_E_INVALID;
    if (n < 0 || n > NI - 1) { h->err = "ifx_merge_instances: n must be 0 .. 95"; return IFX_E_INVALID; }
    if (n == 0) return IFX_OK;
    if (!pairs) { h->err = "ifx_merge_instances: null pairs"; return IFX_E_INVALID; }
    if (h->oseg_pending) { h->err = "ifx_merge_instances: a sharded segmentation call is waiting for an exchange"; return IFX_E_STATE; }
    MergePlan mp;
    if (const char* why = merge_plan_build(h->inst_class, h->inst_color, pairs, n, &mp)) { h->err = std::string("ifx_merge_instances: ") + why; return IFX_E_INVALID; }
    if (!h->d_merge_plan) HIPCHK(h, hipMalloc(&h->d_merge_plan, sizeof(MergePlan)));
    const MergePlan* dp = (const MergePlan*)h->d_merge_plan;
    HIPCHK(h, hipMemcpyAsync(h->d_merge_plan, &mp, sizeof(mp), hipMemcpyHostToDevice, h->cur));
    HIPCHK(h, hipMemcpyAsync(h->d_inst_color, h->inst_color, sizeof(h->inst_color), hipMemcpyHostToDevice, h->cur));
    LAUNCH(h, "merge_votes", dim3(std::max(1, std::min(cdiv(h->cap, MG_RECS), MG_BLOCKS))), dim3(MG_RECS), k_merge_votes, (const DevState*)h->d_state, (float4*)h->votes, h->cap, dp);
    for (int k = 0; k < n; k++) h->inst_class[pairs[2 * k]] = -1;
    h->labels_stale_all = 1;   // votes rewritten across the map, as after an eviction: the full scan, here and now
    h->seg_counts_valid = 0;
    seg_label_scan(h, seg_view_current(h));
    LAUNCH(h, "merge_recolour", dim3(1024), dim3(256), k_merge_recolour, (const DevState*)h->d_state, h->cap, (const float2*)h->tm, (float2*)h->col, (const float*)h->d_inst_color,
           (const int32_t*)h->labels, dp);
    HIPCHK(h, hipStreamSynchronize(h->cur));
    return IFX_OK;
}

// The duplicates of the current view: the box rule of computeCompareMap (IF/Core/InstanceFusion.cpp:595-651, k_seg_compare's float arithmetic) between the projected
// boxes of two registered instances of one class instead of a mask and an instance.  boxes: [96][4] {minX, maxX, minY, maxY}.  parent: per instance the lower
// instance it duplicates best (largest I / U over the threshold, ties to the lower index) or -1.
static void duplicates_decide(const int32_t* inst_class, const int* boxes, float thresh, int* parent)
{
    for (int hi = 0; hi < NI; hi++) {
        parent[hi] = -1;
        const int minX_m = boxes[hi * 4], maxX_m = boxes[hi * 4 + 1], minY_m = boxes[hi * 4 + 2], maxY_m = boxes[hi * 4 + 3];
        if (inst_class[hi] == -1 || maxX_m <= minX_m || maxY_m <= minY_m) continue;
        float best = 0;
        for (int q = 0; q < hi; q++) {
            if (inst_class[q] == -1 || inst_class[q] != inst_class[hi]) continue;
            const int minX_i = boxes[q * 4], maxX_i = boxes[q * 4 + 1], minY_i = boxes[q * 4 + 2], maxY_i = boxes[q * 4 + 3];
            if (maxX_i <= minX_i || maxY_i <= minY_i) continue;
            const float IW = (float)(std::min(maxX_i, maxX_m) - std::max(minX_i, minX_m));
            const float IH = (float)(std::min(maxY_i, maxY_m) - std::max(minY_i, minY_m));
            if (IW <= 0 || IH <= 0) continue;
            const float I = IW * IH;
            const float U = (float)(((maxX_i - minX_i) * (maxY_i - minY_i)) + ((maxX_m - minX_m) * (maxY_m - minY_m))) - I;
            const float iou = I / U;
            if (iou > thresh && (parent[hi] == -1 || iou > best)) { parent[hi] = q; best = iou; }
        }
    }
}
extern "C" int ifx_instance_duplicates(ifx_t* h, float iou_thresh, int32_t* out_pairs, int max_pairs)
{
    if (!h) return IFX_E_INVALID;
    if (max_pairs < 0 || (max_pairs > 0 && !out_pairs) || !(iou_thresh >= 0.0f)) { h->err = "ifx_instance_duplicates: a negative or NaN threshold, or no room for the pairs"; return IFX_E_INVALID; }
    if (h->own || h->shard_n > 1) { h->err = "ifx_instance_duplicates: not on a sharded map"; return IFX_E_STATE; }
    int r = ifx_ids_ensure(h);
    if (r) return r;
    const SegView v = seg_view_current(h);
    LAUNCH(h, "init_bbox", dim3(cdiv(NI * 4, 256)), dim3(256), k_init_bbox, h->d_bbox, NI, h->w, h->h);
    LAUNCH(h, "project_bbox_inst", dim3(cdiv(h->w, 32), cdiv(h->h, PB_ROWS)), dim3(32, PB_ROWS), k_project_bbox<1>, h->d_state, v.ids, (const float4*)h->votes, h->cap, (const uint8_t*)nullptr,
           0, h->w, h->h, h->d_bbox, ifx_idmap(h), (const float4*)nullptr, (uint16_t*)nullptr, (const float*)nullptr);
    int boxes[NI * 4], parent[NI], root[NI];
    HIPCHK(h, hipMemcpyAsync(boxes, h->d_bbox, sizeof(boxes), hipMemcpyDeviceToHost, h->cur));
    HIPCHK(h, hipStreamSynchronize(h->cur));
    duplicates_decide(h->inst_class, boxes, iou_thresh, parent);
    int n = 0;
    for (int i = 0; i < NI; i++) {   // (a parent is a lower index: its root is known)
        root[i] = parent[i] == -1 ? i : root[parent[i]];
        if (parent[i] == -1) continue;
        if (n < max_pairs) { out_pairs[2 * n] = i; out_pairs[2 * n + 1] = root[i]; }
        n++;
    }
    return n;
}

// =========================================================================== f-4: 3-D boxes and per-instance point clouds
// InstanceFusion::computeMapBoundingBox / getInstancePointCloud (IF/Core/InstanceFusion.cpp:1261-1590) with their kernels
// (IF/Core/InstanceFusionCuda.cu:1555-2083): the reference's display / export branch.  A surfel belongs to the instance whose table colour
// its instance colour equals (first match); its normal votes for the cells of an 18 x 36 longitude-latitude grid of the unit sphere whose
// centre lies within the cell's vertex-to-centre distance; the cell with most votes over the whole map gives the ground normal, every
// instance's own votes its heading around that normal; boxes are min / max of the integer-scaled coordinates in the ground (bbox_type 1)
// or instance (0) frame.  The reference evaluates the 648 cell centres with cos / sin inside the kernel for every surfel; here the table
// is built once on the host (the same libm the oracle uses, so the votes are comparable count for count) and staged in LDS.
#define BB_SEG 18
#define BB_CELLS (BB_SEG * BB_SEG * 2)
struct BBCell { float x, y, z, R; };

static void bb_cell_table(BBCell* t)
{
    const float pi = 3.1415926f;
    int p = 0;
    for (int i = -BB_SEG / 2; i < BB_SEG / 2; i++) {
        const float theta_v = i * pi / BB_SEG, d_v = cosf(theta_v), y_v = sinf(theta_v);
        const float theta_m = (i + 0.5f) * pi / BB_SEG, d_m = cosf(theta_m), y_m = sinf(theta_m);
        for (int j = 0; j < 2 * BB_SEG; j++) {
            const float alpha_v = j * pi / BB_SEG, x_v = d_v * cosf(alpha_v), z_v = d_v * sinf(alpha_v);
            const float alpha_m = (j + 0.5f) * pi / BB_SEG, x_m = d_m * cosf(alpha_m), z_m = d_m * sinf(alpha_m);
            const float dx = x_v - x_m, dy = y_v - y_m, dz = z_v - z_m;
            t[p].x = x_m; t[p].y = y_m; t[p].z = z_m; t[p].R = sqrtf(dx * dx + dy * dy + dz * dz);
            p++;
        }
    }
}
__device__ __forceinline__ int instance_of_colour(float cc, const float* __restrict__ inst_color)
{
    for (int i = 0; i < IFX_NUM_INSTANCES; i++) if (cc == inst_color[i]) return i;
    return -1;
}
// testAllSurfelNormalVoteKernel, IF/Core/InstanceFusionCuda.cu:1555-1637
__global__ __launch_bounds__(256) void k_normal_vote(const DevState* __restrict__ st, const float4* __restrict__ nr, const float2* __restrict__ col, const float2* __restrict__ tm,
                                                     const float* __restrict__ inst_color, const BBCell* __restrict__ cells, int* __restrict__ ground_vote, int* __restrict__ inst_vote)
{
    __shared__ BBCell s_cell[BB_CELLS];
    __shared__ int s_vote[BB_CELLS];
    __shared__ float s_col[IFX_NUM_INSTANCES];
    for (int k = threadIdx.x; k < BB_CELLS; k += blockDim.x) { s_cell[k] = cells[k]; s_vote[k] = 0; }
    for (int k = threadIdx.x; k < IFX_NUM_INSTANCES; k += blockDim.x) s_col[k] = inst_color[k];
    __syncthreads();
    const int n = st->count;
    for (int id = blockIdx.x * blockDim.x + threadIdx.x; id < n; id += blockDim.x * gridDim.x) {
        if (!(tm[id].y > DEAD_TIME)) continue;
        const int inst = instance_of_colour(col[id].y, s_col);
        const float4 n4 = nr[id];
        float nx = n4.x, ny = -n4.y, nz = -n4.z;   // "surfels normal in (Map) is inconsistent with (World)", :1574
        const float len = sqrtf(nx * nx + ny * ny + nz * nz);
        nx = nx / len; ny = ny / len; nz = nz / len;
        for (int p = 0; p < BB_CELLS; p++) {
            const float dx = nx - s_cell[p].x, dy = ny - s_cell[p].y, dz = nz - s_cell[p].z;
            if (sqrtf(dx * dx + dy * dy + dz * dz) < s_cell[p].R) {
                atomicAdd(&s_vote[p], 1);
                if (inst != -1) atomicAdd(&inst_vote[BB_CELLS * inst + p], 1);
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < BB_CELLS; k += blockDim.x) if (s_vote[k]) atomicAdd(&ground_vote[k], s_vote[k]);
}
// testAllSurfelFindBBoxKernel, IF/Core/InstanceFusionCuda.cu:1831-1901 (including its comparison of the frame coordinates with the WORLD ones)
__global__ __launch_bounds__(256) void k_find_bbox(const DevState* __restrict__ st, const float4* __restrict__ pc, const float2* __restrict__ col, const float2* __restrict__ tm,
                                                   const float* __restrict__ inst_color, float ratio, const float* __restrict__ gc_inv, const float* __restrict__ inst_inv,
                                                   int bbox_type, int* __restrict__ box)
{
    __shared__ float s_col[IFX_NUM_INSTANCES];
    for (int k = threadIdx.x; k < IFX_NUM_INSTANCES; k += blockDim.x) s_col[k] = inst_color[k];
    __syncthreads();
    const int n = st->count;
    for (int id = blockIdx.x * blockDim.x + threadIdx.x; id < n; id += blockDim.x * gridDim.x) {
        if (!(tm[id].y > DEAD_TIME)) continue;
        const int inst = instance_of_colour(col[id].y, s_col);
        if (inst == -1) continue;
        const float4 p = pc[id];
        const float* M = bbox_type ? gc_inv : inst_inv + 16 * inst;
        const float gx = M[0] * p.x + M[1] * p.y + M[2] * p.z + M[3] * 1.0f;
        const float gy = M[4] * p.x + M[5] * p.y + M[6] * p.z + M[7] * 1.0f;
        const float gz = M[8] * p.x + M[9] * p.y + M[10] * p.z + M[11] * 1.0f;
        const int vx = f2i_rz(gx * ratio), vy = f2i_rz(gy * ratio), vz = f2i_rz(gz * ratio);
        int minX = vx, minY = vy, minZ = vz, maxX = vx, maxY = vy, maxZ = vz;
        if (minX > p.x * ratio) minX--;
        if (minY > p.y * ratio) minY--;
        if (minZ > p.z * ratio) minZ--;
        if (maxX < p.x * ratio) maxX++;
        if (maxY < p.y * ratio) maxY++;
        if (maxZ < p.z * ratio) maxZ++;
        atomicMin(&box[6 * inst + 0], minX); atomicMin(&box[6 * inst + 2], minY); atomicMin(&box[6 * inst + 4], minZ);
        atomicMax(&box[6 * inst + 1], maxX); atomicMax(&box[6 * inst + 3], maxY); atomicMax(&box[6 * inst + 5], maxZ);
    }
}

// ---- the small per-instance part (setGroundandInstanceCoordinateKernel, :1675-1813: 97 threads in the reference) on the host
static void bb_normalize(float* v) { const float l = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); v[0] /= l; v[1] /= l; v[2] /= l; }
static void bb_cross(const float* a, const float* b, float* o) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; }
static void bb_rodrigues(float angle, const float* v, const float* k, float* r)
{
    const float c = cosf(angle), s = sinf(angle), kv = v[0] * k[0] + v[1] * k[1] + v[2] * k[2];
    const float cr[3] = {v[1] * k[2] - v[2] * k[1], v[2] * k[0] - v[0] * k[2], v[0] * k[1] - v[1] * k[0]};
    for (int q = 0; q < 3; q++) r[q] = c * v[q] + (1 - c) * kv * k[q] + s * cr[q];
}
static void bb_matrix(const float* bx, const float* by, const float* bz, float* m)
{
    m[0] = bx[0]; m[1] = by[0]; m[2] = bz[0]; m[3] = 0;
    m[4] = bx[1]; m[5] = by[1]; m[6] = bz[1]; m[7] = 0;
    m[8] = bx[2]; m[9] = by[2]; m[10] = bz[2]; m[11] = 0;
    m[12] = 0; m[13] = 0; m[14] = 0; m[15] = 1;
}
static void bb_frames(const float* ground_normal, const int* inst_vote, float* gc, float* instm)
{
    const float pi = 3.1415926f;
    float by[3] = {ground_normal[0], ground_normal[1], ground_normal[2]}, bx[3], bz[3];
    bb_normalize(by);
    {
        const float setZ[3] = {0, 0, 1};
        bb_cross(setZ, by, bx); bb_normalize(bx);
        bb_cross(by, bx, bz); bb_normalize(bz);
        bb_matrix(bx, by, bz, gc);
    }
    const float step = pi / BB_SEG;
    for (int id = 0; id < IFX_NUM_INSTANCES; id++) {
        const int* nv = inst_vote + id * BB_CELLS;
        int cross_vote[2 * BB_SEG] = {0};
        const float oriZ[3] = {0, 0, -1};
        float oriX[3];
        bb_cross(by, oriZ, oriX); bb_normalize(oriX);
        for (int i = 0; i < BB_CELLS; i++) {
            if (nv[i] == 0) continue;
            const int a = i / (2 * BB_SEG) - BB_SEG / 2, b = i % (2 * BB_SEG) - 1;
            const float theta = (a + 0.5f) * pi / BB_SEG, alpha = (b + 0.5f) * pi / BB_SEG, d = cosf(theta);
            float tz[3] = {d * cosf(alpha), sinf(theta), d * sinf(alpha)};
            bb_normalize(tz);
            const float cs = by[0] * tz[0] + by[1] * tz[1] + by[2] * tz[2];
            if (cs > 0.525f || -cs > 0.525f) continue;
            float best = 999999.9f;
            int best_j = -1;
            for (int j = 0; j < 2 * BB_SEG; j++) {
                float rv[3];
                bb_rodrigues(j * step, oriX, by, rv); bb_normalize(rv);
                const float dx = rv[0] - tz[0], dy = rv[1] - tz[1], dz = rv[2] - tz[2], dist = sqrtf(dx * dx + dy * dy + dz * dz);
                if (dist < best) { best_j = j; best = dist; }
            }
            cross_vote[best_j] += nv[i];
        }
        int vmax = 0, vid = 0;
        for (int i = 0; i < 2 * BB_SEG; i++) if (cross_vote[i] > vmax) { vmax = cross_vote[i]; vid = i; }
        float rv[3];
        bb_rodrigues(vid * step, oriX, by, rv); bb_normalize(rv);
        bb_cross(rv, by, bx); bb_normalize(bx);
        bb_cross(by, bx, bz); bb_normalize(bz);
        bb_matrix(bx, by, bz, instm + 16 * id);
    }
}
// inverse of [B 0; 0 1] with B orthonormal up to rounding: general 3x3 inverse in f64 (Eigen's Matrix4f::inverse in the reference)
static void bb_inverse(const float* m, float* o)
{
    const double a[9] = {m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]};
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c00 + a[1] * c01 + a[2] * c02, id = 1.0 / det;
    const double inv[9] = {c00 * id, (a[2] * a[7] - a[1] * a[8]) * id, (a[1] * a[5] - a[2] * a[4]) * id, c01 * id, (a[0] * a[8] - a[2] * a[6]) * id,
                           (a[2] * a[3] - a[0] * a[5]) * id, c02 * id, (a[1] * a[6] - a[0] * a[7]) * id, (a[0] * a[4] - a[1] * a[3]) * id};
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) o[r * 4 + c] = (float)inv[r * 3 + c]; o[r * 4 + 3] = 0; }
    o[12] = 0; o[13] = 0; o[14] = 0; o[15] = 1;
}

struct BBState { std::vector<float> gc_inv, inst_inv; };
static int bb_compute(ifx* h, float* ground_normal3, float* gc16, float* inst16, int32_t* ground_votes, float* d_inv /* [16 + 96*16] device, out */)
{
    BBCell cells[BB_CELLS];
    bb_cell_table(cells);
    const size_t nv = (size_t)BB_CELLS * (1 + IFX_NUM_INSTANCES);
    int* d_vote = nullptr;
    BBCell* d_cells = nullptr;
    HIPCHK(h, hipMalloc(&d_vote, nv * 4));
    if (hipMalloc(&d_cells, sizeof(cells)) != hipSuccess) { hipFree(d_vote); h->err = "hipMalloc failed"; return IFX_E_HIP; }
    hipMemsetAsync(d_vote, 0, nv * 4, h->cur);
    hipMemcpyAsync(d_cells, cells, sizeof(cells), hipMemcpyHostToDevice, h->cur);
    hipMemcpyAsync(h->d_inst_color, h->inst_color, sizeof(h->inst_color), hipMemcpyHostToDevice, h->cur);
    LAUNCH(h, "normal_vote", dim3(2048), dim3(256), k_normal_vote, (const DevState*)h->d_state, (const float4*)h->nr, (const float2*)h->col, (const float2*)h->tm,
           (const float*)h->d_inst_color, (const BBCell*)d_cells, d_vote, d_vote + BB_CELLS);
    std::vector<int> votes(nv);
    hipError_t e = hipMemcpyAsync(votes.data(), d_vote, nv * 4, hipMemcpyDeviceToHost, h->cur);
    if (e == hipSuccess) e = hipStreamSynchronize(h->cur);
    hipFree(d_vote); hipFree(d_cells);
    if (e != hipSuccess) { h->err = hipGetErrorString(e); return IFX_E_HIP; }
    // ground normal: the cell with most votes (IF/Core/InstanceFusion.cpp:1289-1328, including its `- 1` on the longitude index)
    float gn[3] = {0, -1, 0};
    int vmax = -1, vid = -1;
    for (int i = 0; i < BB_CELLS; i++) if (votes[i] > vmax) { vmax = votes[i]; vid = i; }
    if (vid != -1) {
        const float pi = 3.1415926f;
        const int i = vid / (2 * BB_SEG) - BB_SEG / 2, j = vid % (2 * BB_SEG) - 1;
        const float theta = (i + 0.5f) * pi / BB_SEG, alpha = (j + 0.5f) * pi / BB_SEG, d = cosf(theta);
        gn[0] = d * cosf(alpha); gn[1] = sinf(theta); gn[2] = d * sinf(alpha);
        bb_normalize(gn);
    }
    float gc[16], instm[16 * IFX_NUM_INSTANCES], inv[16 + 16 * IFX_NUM_INSTANCES];
    bb_frames(gn, votes.data() + BB_CELLS, gc, instm);
    bb_inverse(gc, inv);
    for (int i = 0; i < IFX_NUM_INSTANCES; i++) bb_inverse(instm + 16 * i, inv + 16 + 16 * i);
    if (ground_normal3) memcpy(ground_normal3, gn, 12);
    if (gc16) memcpy(gc16, gc, 64);
    if (inst16) memcpy(inst16, instm, sizeof(instm));
    if (ground_votes) memcpy(ground_votes, votes.data(), BB_CELLS * 4);
    HIPCHK(h, hipMemcpyAsync(d_inv, inv, sizeof(inv), hipMemcpyHostToDevice, h->cur));
    HIPCHK(h, hipStreamSynchronize(h->cur));
    return IFX_OK;
}

extern "C" int ifx_map_bounding_boxes(ifx_t* h, int bbox_type, float ratio, float* boxes96x6, float* ground_normal3, float* gc_matrix16, float* inst_matrix96x16, int32_t* ground_votes648)
{
    if (!h || !boxes96x6) return IFX_E_INVALID;
    ifx_vlist_reap(h);
    float* d_inv = nullptr;
    int* d_box = nullptr;
    HIPCHK(h, hipMalloc(&d_inv, (16 + 16 * IFX_NUM_INSTANCES) * 4));
    int r = bb_compute(h, ground_normal3, gc_matrix16, inst_matrix96x16, ground_votes648, d_inv);
    if (r) { hipFree(d_inv); return r; }
    if (hipMalloc(&d_box, IFX_NUM_INSTANCES * 6 * 4) != hipSuccess) { hipFree(d_inv); h->err = "hipMalloc failed"; return IFX_E_HIP; }
    int init[IFX_NUM_INSTANCES * 6];
    for (int i = 0; i < IFX_NUM_INSTANCES; i++) { init[i * 6] = init[i * 6 + 2] = init[i * 6 + 4] = 999999999; init[i * 6 + 1] = init[i * 6 + 3] = init[i * 6 + 5] = -999999999; }
    hipMemcpyAsync(d_box, init, sizeof(init), hipMemcpyHostToDevice, h->cur);
    LAUNCH(h, "find_bbox", dim3(2048), dim3(256), k_find_bbox, (const DevState*)h->d_state, (const float4*)h->pc, (const float2*)h->col, (const float2*)h->tm,
           (const float*)h->d_inst_color, ratio, (const float*)d_inv, (const float*)(d_inv + 16), bbox_type ? 1 : 0, d_box);
    hipError_t e = hipMemcpyAsync(init, d_box, sizeof(init), hipMemcpyDeviceToHost, h->cur);
    if (e == hipSuccess) e = hipStreamSynchronize(h->cur);
    hipFree(d_box); hipFree(d_inv);
    if (e != hipSuccess) { h->err = hipGetErrorString(e); return IFX_E_HIP; }
    for (int k = 0; k < IFX_NUM_INSTANCES * 6; k++) boxes96x6[k] = init[k] / ratio;   // :1424-1430
    return IFX_OK;
}

// mapCountInstanceByInstColorKernel + getSurfelToInstanceBufferKernel, IF/Core/InstanceFusionCuda.cu:1920-2066: the surfels of one instance
// as records {slot, position in the box frame, normal in the box frame (incl. the reference's homogeneous 1 on the direction), r, g, b}.
// The reference fills its buffers in the order the atomics land; here in slot order (flags, scan, scatter).
__global__ void k_inst_flags(const DevState* __restrict__ st, const float2* __restrict__ col, const float2* __restrict__ tm, const float* __restrict__ inst_color, int want, int cap,
                             int* __restrict__ flags, int* __restrict__ counts)
{
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= cap) return;
    int f = 0;
    if (id < st->count && tm[id].y > DEAD_TIME) {
        const int inst = instance_of_colour(col[id].y, inst_color);
        if (inst != -1) atomicAdd(&counts[inst], 1);
        f = inst == want;
    }
    flags[id] = f;
}
__global__ void k_inst_records(const int* __restrict__ flags, const int* __restrict__ rank, int cap, int max_rec, const float4* __restrict__ pc, const float4* __restrict__ nr,
                               const float2* __restrict__ col, const float* __restrict__ M, float* __restrict__ out)
{
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= cap || !flags[id]) return;
    const int k = rank[id];
    if (k >= max_rec) return;
    const float4 p = pc[id], n4 = nr[id];
    float nx = n4.x, ny = -n4.y, nz = -n4.z;
    const float len = sqrtf(nx * nx + ny * ny + nz * nz);
    nx = nx / len; ny = ny / len; nz = nz / len;
    float* o = out + (size_t)k * 10;
    o[0] = (float)id;
    o[1] = M[0] * p.x + M[1] * p.y + M[2] * p.z + M[3] * 1.0f;
    o[2] = M[4] * p.x + M[5] * p.y + M[6] * p.z + M[7] * 1.0f;
    o[3] = M[8] * p.x + M[9] * p.y + M[10] * p.z + M[11] * 1.0f;
    o[4] = M[0] * nx + M[1] * ny + M[2] * nz + M[3] * 1.0f;
    o[5] = M[4] * nx + M[5] * ny + M[6] * nz + M[7] * 1.0f;
    o[6] = M[8] * nx + M[9] * ny + M[10] * nz + M[11] * 1.0f;
    const int c = f2i_rz(col[id].x);
    o[7] = (float)(c >> 16 & 0xFF) / 255.0f; o[8] = (float)(c >> 8 & 0xFF) / 255.0f; o[9] = (float)(c & 0xFF) / 255.0f;
}
extern "C" int ifx_instance_point_cloud(ifx_t* h, int bbox_type, int32_t* counts96, int inst, float* out10, int max_records)
{
    if (!h || !counts96 || inst < -1 || inst >= IFX_NUM_INSTANCES || (inst >= 0 && (!out10 || max_records <= 0))) return IFX_E_INVALID;
    ifx_vlist_reap(h);
    float* d_inv = nullptr;
    HIPCHK(h, hipMalloc(&d_inv, (16 + 16 * IFX_NUM_INSTANCES) * 4));
    int r = bb_compute(h, nullptr, nullptr, nullptr, nullptr, d_inv);
    if (r) { hipFree(d_inv); return r; }
    int* d_cnt = h->d_inst_stats;
    hipMemsetAsync(d_cnt, 0, IFX_NUM_INSTANCES * 4, h->cur);
    const int n = h->cap;
    LAUNCH(h, "inst_flags", dim3(cdiv(n, 256)), dim3(256), k_inst_flags, (const DevState*)h->d_state, (const float2*)h->col, (const float2*)h->tm, (const float*)h->d_inst_color, inst, n,
           h->scan_flags, d_cnt);
    int written = 0;
    float* d_out = nullptr;
    if (inst >= 0) {
        ifx_scan_exclusive(h, h->scan_flags, n, h->scan_out, &h->d_state->seg_counts[1]);
        if (hipMalloc(&d_out, (size_t)max_records * 40) != hipSuccess) { hipFree(d_inv); h->err = "hipMalloc failed"; return IFX_E_HIP; }
        LAUNCH(h, "inst_records", dim3(cdiv(n, 256)), dim3(256), k_inst_records, (const int*)h->scan_flags, (const int*)h->scan_out, n, max_records, (const float4*)h->pc,
               (const float4*)h->nr, (const float2*)h->col, (const float*)(bbox_type ? d_inv : d_inv + 16 + 16 * inst), d_out);
    }
    hipError_t e = hipMemcpyAsync(counts96, d_cnt, IFX_NUM_INSTANCES * 4, hipMemcpyDeviceToHost, h->cur);
    if (e == hipSuccess) e = hipStreamSynchronize(h->cur);
    if (e == hipSuccess && inst >= 0) {
        written = std::min(counts96[inst], max_records);
        if (written > 0) e = hipMemcpy(out10, d_out, (size_t)written * 40, hipMemcpyDeviceToHost);
    }
    hipFree(d_out); hipFree(d_inv);
    if (e != hipSuccess) { h->err = hipGetErrorString(e); return IFX_E_HIP; }
    return written;
}
