// Heat-map confidences and confidence-gated view selection (include/handmv.h "heat-map confidences"): two stateless launches.
//
// hmv_op_heatmap_peaks is the reference's heatmaps_to_coordinates (models/utils.py:65-82): the maximum of every score map and where it
// lies, under the total order of torch.max -- the largest value wins, among equal values (+0 == -0) the lowest flat index, a NaN beats
// every number and the first NaN wins.  One wave64 per map, four per workgroup.  A map is contiguous: lanes read 16-byte vectors when
// h * w is a multiple of four and the base is 16-byte aligned, scalar floats otherwise, in groups whose loads are all issued before the
// first of them is used (misc_kernels.hip, soft_argmax_frame_kernel, for why).  Each lane keeps (value, index) over ascending indices
// and starts from "nothing yet" (index -1), never from -inf at index 0; the wave reduces by __shfl_xor with the same order; lane 0
// writes.  A wave beyond the last map returns at once: there is no barrier.  A load past the map is not issued, not discarded.
//
// hmv_op_confidence_select is the camera selection of the reference's triangulate_dlt (utils/triangulation.py:227-236): per joint the
// views whose confidence exceeds a threshold that is lowered by `step` until two remain.  The threshold is a double and is lowered by
// repeated subtraction, the comparison is conf > (float)t in fp32 (what numpy does with a float32 array and a Python float), and with
// carry == 1 what joint j lowered every later joint of the sample starts from, as in the reference, which never resets it.  One wave64
// per sample, four per workgroup: the sample's V * J confidences and usable bits are staged into LDS with coalesced loads, lane v < V
// owns view v, the count is a ballot and a popcount, t and the counters are wave-uniform, and the joint loop runs inside the wave.
// A wave beyond the last sample runs along on the last one and stores nothing, so the barriers stay block-wide.
//
// No atomics; vector stores in plain C++.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/handmv.h"
#include "kernels.h"

// t -= step stays a subtraction, rounded on its own.
#pragma clang fp contract(off)

namespace {

constexpr int kWave = 64;
constexpr int kRowsPerBlock = 4;
constexpr int kGroup = 4;      // loads a lane has in flight before it uses the first
constexpr int kMaxV = 16;
constexpr int kMaxJ = 64;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct PeaksParams {
    const float *heatmap;   // [maps][hw]
    long maps;
    int hw, w, vec;         // vec: 16-byte loads are allowed
    float *maxval;          // [maps] or null
    int *index;             // [maps] or null
    float *preds;           // [maps][2] or null
};

struct SelectParams {
    const float *conf;           // [B][V][J]
    const uint8_t *present;      // [B][V] or null
    const uint8_t *joint_mask;   // [B][V][J] or null
    int B, V, J, carry;
    double threshold, step;
    uint8_t *mask_out;           // [B][V][J]
    float *level;                // [B][J] or null
    int *lowered, *selected;     // [B][J] or null
};

// One more element of a lane's own ascending run: it replaces what the lane holds when there is nothing yet, or when what is held is a
// number and the element is larger or a NaN.  An equal value and a second NaN come later in the run and lose.
__device__ __forceinline__ void take(float &bv, int &bi, float v, int i) {
    if (bi < 0 || (bv == bv && !(v <= bv))) {
        bv = v;
        bi = i;
    }
}

// Does (v, i) come before (bv, bi) in torch.max's order?  An index of -1 is "nothing".
__device__ __forceinline__ bool beats(float v, int i, float bv, int bi) {
    if (i < 0) return false;
    if (bi < 0) return true;
    const bool n = v != v, bn = bv != bv;
    if (n || bn) return n && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

__global__ __launch_bounds__(kWave * kRowsPerBlock) void heatmap_peaks_kernel(const PeaksParams p) {
    const int lane = (int)threadIdx.x & (kWave - 1);
    const long map = (long)blockIdx.x * kRowsPerBlock + ((int)threadIdx.x >> 6);
    if (map >= p.maps) return;
    const int hw = p.hw;
    const float *src = p.heatmap + map * hw;
    float bv = 0.f;
    int bi = -1;
    if (p.vec) {
        const f32x4 *src4 = reinterpret_cast<const f32x4 *>(src);
        const int n4 = hw >> 2;
        for (int q0 = lane; q0 < n4; q0 += kWave * kGroup) {
            f32x4 raw[kGroup];
#pragma unroll
            for (int u = 0; u < kGroup; ++u) {
                const int q = q0 + kWave * u;
                if (q < n4) raw[u] = src4[q];
            }
#pragma unroll
            for (int u = 0; u < kGroup; ++u) {
                const int q = q0 + kWave * u;
                if (q < n4) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) take(bv, bi, raw[u][e], 4 * q + e);
                }
            }
        }
    } else {
        for (int i0 = lane; i0 < hw; i0 += kWave * kGroup) {
            float raw[kGroup];
#pragma unroll
            for (int u = 0; u < kGroup; ++u) {
                const int i = i0 + kWave * u;
                if (i < hw) raw[u] = src[i];
            }
#pragma unroll
            for (int u = 0; u < kGroup; ++u) {
                const int i = i0 + kWave * u;
                if (i < hw) take(bv, bi, raw[u], i);
            }
        }
    }
    for (int m = kWave / 2; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(bv, m, kWave);
        const int oi = __shfl_xor(bi, m, kWave);
        if (beats(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    if (lane == 0) {
        if (p.maxval) p.maxval[map] = bv;
        if (p.index) p.index[map] = bi;
        if (p.preds) {   // models/utils.py:73-81: the 1-based (x, y), zeroed unless maxval > 0
            const int y = bi / p.w, x = bi - y * p.w;
            const bool on = bv > 0.f;
            p.preds[map * 2] = on ? (float)(x + 1) : 0.f;
            p.preds[map * 2 + 1] = on ? (float)(y + 1) : 0.f;
        }
    }
}

__global__ __launch_bounds__(kWave * kRowsPerBlock) void confidence_select_kernel(const SelectParams p) {
    __shared__ float sC[kRowsPerBlock][kMaxV * kMaxJ];
    __shared__ uint8_t sU[kRowsPerBlock][kMaxV * kMaxJ];   // staged: 1 = usable;  after the joint loop: mask_out
    const int lane = (int)threadIdx.x & (kWave - 1), w = (int)threadIdx.x >> 6;
    long b = (long)blockIdx.x * kRowsPerBlock + w;
    const bool valid = b < p.B;
    if (!valid) b = p.B - 1;
    const int V = p.V, J = p.J, n = V * J;
    const long base = b * n;
    for (int i = lane; i < n; i += kWave) {
        sC[w][i] = p.conf[base + i];
        const bool here = !p.present || p.present[b * V + i / J] != 0;
        sU[w][i] = (here && (!p.joint_mask || p.joint_mask[base + i] == 0)) ? 1 : 0;
    }
    __syncthreads();
    double t = p.threshold;
    for (int j = 0; j < J; ++j) {
        if (!p.carry) t = p.threshold;
        const int at = (lane < V ? lane : 0) * J + j;
        const float c = sC[w][at];
        const bool usable = lane < V && sU[w][at] != 0;
        int low = 0, kept;
        bool sel;
        for (;;) {   // triangulation.py:228-236
            sel = usable && c > (float)t;   // (false for a NaN confidence)
            kept = __popcll((unsigned long long)__ballot(sel));
            if (t <= 0.0) break;
            if (kept > 1) break;
            t -= p.step;
            ++low;
        }
        if (lane < V) sU[w][at] = sel ? 0 : 1;
        if (valid && lane == 0) {
            const long row = b * J + j;
            if (p.level) p.level[row] = (float)t;
            if (p.lowered) p.lowered[row] = low;
            if (p.selected) p.selected[row] = kept;
        }
    }
    __syncthreads();
    if (valid)
        for (int i = lane; i < n; i += kWave) p.mask_out[base + i] = sU[w][i];
}

using hmv::bad_arg;
using hmv::hip_fail;

}  // namespace

extern "C" int hmv_op_heatmap_peaks(int32_t device, const hmv_peaks_args *a, void *stream) {
    const char *who = "hmv_op_heatmap_peaks";
    if (!a) return bad_arg(who, "args is NULL");
    if (a->struct_size != (int32_t)sizeof(hmv_peaks_args)) return bad_arg(who, "struct_size does not match this library's hmv_peaks_args");
    if (a->N < 1) return bad_arg(who, "N must be >= 1");
    if (a->J < 1) return bad_arg(who, "J must be >= 1");
    if (a->h < 1) return bad_arg(who, "h must be >= 1");
    if (a->w < 1) return bad_arg(who, "w must be >= 1");
    if ((int64_t)a->N * a->J > (1 << 24)) return bad_arg(who, "N * J must not exceed 2^24 maps");
    if ((int64_t)a->h * a->w > (1 << 20)) return bad_arg(who, "h * w must not exceed 2^20 pixels");
    if (!a->heatmap) return bad_arg(who, "heatmap is NULL");
    if (!a->maxval && !a->index && !a->preds) return bad_arg(who, "maxval, index and preds are all NULL: nothing to write");
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    const int hw = a->h * a->w;
    const int vec = (hw % 4 == 0 && ((uintptr_t)a->heatmap & 15) == 0) ? 1 : 0;
    const PeaksParams p{a->heatmap, (long)a->N * a->J, hw, a->w, vec, a->maxval, a->index, a->preds};
    const unsigned blocks = (unsigned)((p.maps + kRowsPerBlock - 1) / kRowsPerBlock);
    hipLaunchKernelGGL(heatmap_peaks_kernel, dim3(blocks), dim3(kWave * kRowsPerBlock), 0, (hipStream_t)stream, p);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}

extern "C" int hmv_op_confidence_select(int32_t device, const hmv_confidence_select_args *a, void *stream) {
    const char *who = "hmv_op_confidence_select";
    if (!a) return bad_arg(who, "args is NULL");
    if (a->struct_size != (int32_t)sizeof(hmv_confidence_select_args))
        return bad_arg(who, "struct_size does not match this library's hmv_confidence_select_args");
    if (a->B < 1) return bad_arg(who, "B must be >= 1");
    if (a->V < 1 || a->V > kMaxV) return bad_arg(who, "V must be in 1 .. 16");
    if (a->J < 1 || a->J > kMaxJ) return bad_arg(who, "J must be in 1 .. 64");
    if (a->carry != 0 && a->carry != 1) return bad_arg(who, "carry must be 0 or 1");
    if (!isfinite(a->threshold)) return bad_arg(who, "threshold must be finite");
    if (!isfinite(a->step) || !(a->step > 0.0)) return bad_arg(who, "step must be finite and > 0");
    if (a->threshold / a->step > 1024.0) return bad_arg(who, "threshold / step must not exceed 1024 levels");
    if (!a->conf) return bad_arg(who, "conf is NULL");
    if (!a->mask_out) return bad_arg(who, "mask_out is NULL");
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    const SelectParams p{a->conf, a->present, a->joint_mask, a->B, a->V, a->J, a->carry, a->threshold, a->step,
                         a->mask_out, a->level, a->lowered, a->selected};
    const unsigned blocks = (unsigned)(((long)a->B + kRowsPerBlock - 1) / kRowsPerBlock);
    hipLaunchKernelGGL(confidence_select_kernel, dim3(blocks), dim3(kWave * kRowsPerBlock), 0, (hipStream_t)stream, p);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}
